// mosaic_kernels.h -- the kernels of the beam-weighted mosaic, as prisim_mosaic_image (mosaic.hip) runs them chunk by chunk and
// prisim_clean_mosaic (mosclean.hip) once over all pixels for its first residual, with the functions that enqueue them:
//   k_mos_wsum   W_t[k] = sum_b w[t][b][k] as [nt][nchan], b ascending, and Wtot[k] = sum_t W_t[k], t ascending; one thread per
//                channel.  k_img_wtot sums Wtot over k for chan_avg.
//   k_mos_sum    the hot path, one launch per snapshot: the tile pass of that snapshot (img_tile_pass of imaging_kernels.h) on
//                (w Re V, w Im V).  The epilogue reads the thread's 32 beam values, puts 0 in their place where the direction is below
//                the horizon, and writes N = fma(A, acc, N) and Q = fma(A A, W_t, Q); snapshot 0 starts from 0 and reads nothing.
//   k_mos_finish the division, the mask Q >= pbmin^2 Wtot (else NaN) and pb_eff = sqrt(Q / Wtot) per (pixel, channel); or, with
//                chan_avg, k_mos_finish_band: the sums of N and Q over k ascending per pixel, then the same three.
// No atomics.  Every including file gets its own copy (an unnamed namespace); built with -ffp-contract=off.  Not part of the public ABI.
#ifndef PRISIM_MOSAIC_KERNELS_H
#define PRISIM_MOSAIC_KERNELS_H

#include "../csrc_addon/beam_setup.h"
#include "imaging_kernels.h"

namespace {

// grid: x over the channels.  wt [nt][nchan], wtot [nchan].  Why this is not k_img_wsum: see there (dirty_image.h)
__global__ void __launch_bounds__(kThreads) k_mos_wsum(ImgWeights W, int64_t nt, int64_t nbl, int nchan, double* __restrict__ wt,
                                                       double* __restrict__ wtot) {
  const int k = (int)blockIdx.x * kThreads + threadIdx.x;
  if (k >= nchan) return;
  double tot = 0.0;
  for (int64_t t = 0; t < nt; ++t) {
    const double* row = W.w ? W.w + t * W.st + k * W.sk : nullptr;
    double s = 0.0;
#pragma unroll 8
    for (int64_t b = 0; b < nbl; ++b) s += row ? row[b * W.sb] : 1.0;
    wt[t * nchan + k] = s;
    tot += s;
  }
  wtot[k] = tot;
}

struct MosParams {
  const double2* cube;      // [nt][nbl][nchan]
  ImgWeights W;
  const double* bl;         // [nbl][3]
  const double* freqs;      // [nchan]
  const double4* dd;        // [count] of the chunk at snapshot t: s - s0
  const double4* s4;        // [count] of the chunk at snapshot t: s, for the horizon
  const double* pb;         // [count][nchan] the beam tile of snapshot t
  const double* wt;         // [nchan] W_t
  double df;                // the step of a uniform grid (STEPPED)
  int64_t nbl, t, count;    // t: the snapshot of this launch; count: pixels of the chunk
  int nchan;
  double *N, *Q;            // [count][nchan] of the chunk: read unless t == 0, written
};

// grid: x = block of the chunk's pixels, y = channel tile.  LDS: kImagingLds
template <bool STEPPED>
__global__ void __launch_bounds__(kThreads) k_mos_sum(MosParams P) {
  __shared__ double2 sh_v[NB * CT];     // (w Re V, w Im V)
  __shared__ double sh_b[NB * 3];       // b / c
  __shared__ double sh_f[CT];           // the tile's frequencies; past the band: the last channel's (their operand rows are 0)
  const int tid = threadIdx.x;
  const int k0 = (int)blockIdx.y * CT;
  const int64_t pl_raw = (int64_t)blockIdx.x * kThreads + tid;
  const bool p_valid = pl_raw < P.count;
  const int64_t pl = p_valid ? pl_raw : P.count - 1;
  const int64_t t = P.t;
  if (tid < CT) sh_f[tid] = P.freqs[k0 + tid < P.nchan ? k0 + tid : P.nchan - 1];
  double acc[CT];
#pragma unroll
  for (int k = 0; k < CT; ++k) acc[k] = 0.0;
  const double f0 = P.freqs[k0];          // k0 < nchan: the grid has ceil(nchan / CT) tiles
  img_tile_pass<STEPPED, false>(t, P.dd[pl], P.bl, P.nbl, k0, f0, P.df, sh_v, sh_b, sh_f, acc, [&P](bool live, int64_t t, int64_t b, int, int k) {
    if (!live || k >= P.nchan) return make_double2(0.0, 0.0);
    const double w = P.W.at(t, b, k);
    const double2 x = P.cube[(t * P.nbl + b) * P.nchan + k];
    return make_double2(w * x.x, w * x.y);
  });
  if (!p_valid) return;
  const bool up = P.s4[pl].z >= 0.0;
  const int64_t at = pl * P.nchan + k0;
#pragma unroll
  for (int k = 0; k < CT; ++k)
    if (k0 + k < P.nchan) {
      const double A = up ? P.pb[at + k] : 0.0;
      P.N[at + k] = fma(A, acc[k], t ? P.N[at + k] : 0.0);
      P.Q[at + k] = fma(A * A, P.wt[k0 + k], t ? P.Q[at + k] : 0.0);
    }
}

// grid-stride over count * nchan
__global__ void __launch_bounds__(kThreads) k_mos_finish(const double* __restrict__ N, const double* __restrict__ Q, const double* __restrict__ wtot,
                                                         int64_t count, int nchan, double pbmin, double* __restrict__ mosaic,
                                                         double* __restrict__ pb_eff) {
  const int64_t total = count * nchan;
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kThreads) {
    const double w = wtot[e % nchan], q = Q[e];
    mosaic[e] = q >= (pbmin * pbmin) * w ? N[e] / q : NAN;
    pb_eff[e] = sqrt(q / w);
  }
}

// grid: x over the chunk's pixels.  wband[0] = sum_k wtot[k]
__global__ void __launch_bounds__(kThreads) k_mos_finish_band(const double* __restrict__ N, const double* __restrict__ Q,
                                                              const double* __restrict__ wband, int64_t count, int nchan, double pbmin,
                                                              double* __restrict__ mosaic, double* __restrict__ pb_eff) {
  const int64_t pl = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (pl >= count) return;
  double n = 0.0, q = 0.0;
  for (int k = 0; k < nchan; ++k) {
    n += N[pl * nchan + k];
    q += Q[pl * nchan + k];
  }
  const double w = wband[0];
  mosaic[pl] = q >= (pbmin * pbmin) * w ? n / q : NAN;
  pb_eff[pl] = sqrt(q / w);
}

// the checks of the fields of the beam and of pbmin, behind check_args of the shared fields
template <typename Args>
inline int check_mosaic_beam(prisim_ctx* ctx, const Args& a) {
  if (!(a.pbmin >= 0.0 && a.pbmin < 1.0)) return fail(ctx, PRISIM_EINVAL, "pbmin must lie in [0, 1)");
  if (int rc = check_beams(ctx, a.beam_kind, a.diameter_m, a.beam_pc_dircos, a.ext, a.n_ext, a.nt, "nt")) return rc;
  for (int64_t i = 0; a.beam_pc_snap && i < a.nt * 3; ++i)
    if (!std::isfinite(a.beam_pc_snap[i])) return fail(ctx, PRISIM_EINVAL, "beam_pc_snap of snapshot " + std::to_string(i / 3) + " is not finite");
  return PRISIM_OK;
}

// the beam of snapshot t on `count` directions s4 into pb [count][nchan], with unit flux (flux_ref = 1, spindex = 0: pb exp2(0) = pb
// exactly); ones and zeros hold at least `count` elements, d_bf as upload_beamformers leaves it
template <typename Args>
inline int enqueue_mos_beam(prisim_ctx* ctx, const Args& a, int64_t t, const std::vector<const double*>& d_bf, const double4* s4, int64_t count,
                            const double* freqs, const double* ones, const double* zeros, int32_t* flag, double* pb, hipStream_t s) {
  const int64_t e = a.n_ext == a.nt ? t : 0;
  BeamParams bp{};
  fill_beam(bp, a.beam_kind, a.diameter_m, a.beam_pc_snap ? a.beam_pc_snap + t * 3 : a.beam_pc_dircos, a.n_ext > 0 ? a.ext + e : nullptr,
            d_bf[(size_t)e]);
  bp.dirs = (const double*)s4;
  bp.flux_ref = ones;
  bp.spindex = zeros;
  bp.freqs = freqs;
  bp.ref_freq = 1.0;
  bp.flag = flag;
  bp.nsrc = count;
  bp.nchan = a.nchan;
  bp.pb_out = pb;
  HIPCHK(ctx, launch_beam_flux(bp, s));
  return PRISIM_OK;
}

// the weight sums of a call, once and before any pixel: wt [nt][nchan], wtot [nchan], wband [1]
inline int enqueue_mos_wsum(prisim_ctx* ctx, const ImgWeights& W, int64_t nt, int64_t nbl, int64_t nchan, double* wt, double* wtot, double* wband,
                            hipStream_t s) {
  if (int rc = launch(ctx, k_mos_wsum, dim3((unsigned)((nchan + kThreads - 1) / kThreads)), 0, s, W, nt, nbl, (int)nchan, wt, wtot)) return rc;
  hipLaunchKernelGGL(k_img_wtot, dim3(1), dim3(64), 0, s, (const double*)wtot, (int)nchan, wband);
  HIPCHK(ctx, hipGetLastError());
  return PRISIM_OK;
}

// snapshot P.t of P.count pixels in blocks of `block`, ntiles channel tiles
inline int enqueue_mos_sum(prisim_ctx* ctx, const MosParams& P, int64_t block, int64_t ntiles, bool stepped, hipStream_t s) {
  const dim3 grid((unsigned)((P.count + block - 1) / block), (unsigned)ntiles);
  return stepped ? launch(ctx, k_mos_sum<true>, grid, 0, s, P) : launch(ctx, k_mos_sum<false>, grid, 0, s, P);
}

// mosaic and pb_eff [count][nchan] or, with avg, [count] from N and Q [count][nchan]
inline int enqueue_mos_finish(prisim_ctx* ctx, bool avg, const double* N, const double* Q, const double* wtot, const double* wband, int64_t count,
                              int64_t nchan, double pbmin, double* mosaic, double* pb_eff, hipStream_t s) {
  if (avg)
    return launch(ctx, k_mos_finish_band, dim3((unsigned)((count + kThreads - 1) / kThreads)), 0, s, N, Q, wband, count, (int)nchan, pbmin, mosaic,
                  pb_eff);
  return launch(ctx, k_mos_finish, dim3((unsigned)grid_for(ctx, count * nchan)), 0, s, N, Q, wtot, count, (int)nchan, pbmin, mosaic, pb_eff);
}

}  // namespace

#endif  // PRISIM_MOSAIC_KERNELS_H
