// mosclean.hip -- CLEAN of the beam-weighted mosaic of the snapshots for gfx950 (include/prisim_mosclean.h, where the mathematics is).
// It joins what this directory already states and restates none of it: the mosaic's sums (mosaic_kernels.h), the bookkeeping of an
// image-space CLEAN (clean_kernels.h), the tile pass of the direct Fourier sum (img_tile_pass of imaging_kernels.h) and the fused
// analytic beam (launch_beam_flux by enqueue_mos_beam).  All pixels are resident; one stream.
//
// Once per call:
//   k_img_dirs, k_mos_wsum   the directions with their offsets, and the weight sums, as prisim_mosaic_image runs them.
//   the beam table           A[nt][npix][nchan]: per snapshot enqueue_mos_beam with unit flux, then k_mosclean_horizon writes 0 where
//                            s_z < 0.  It stays for the whole call: the staging of the update gathers A[t][q_k][k] from it, its epilogue
//                            reads A[t][p][k].
//   k_mos_sum                per snapshot, reading its beam tile from the table: R_N starts as the mosaic's N, and Q is the mosaic's,
//                            bit for bit.  With maxiter = 0 the call is a mosaic.
// Per iteration, three steps that never wait for the host:
//   k_mosclean_flat          the search image F = R_N / sqrt(Q Wtot) under the mask (NaN outside it), [npix][nc]; with chan_avg the
//                            band sums over k ascending.  Bound by device memory: 24 B read a (pixel, channel), 8 B written.
//   k_imclean_peak1, k_imclean_peak2   of clean_kernels.h, on F as it stands; the flux of a component is gain (R_N / Q) at the pick
//                            (MosaicFlux), the band sums with chan_avg.
//   k_mosclean_update        the hot path: img_tile_pass<STEPPED, false>, so the summation order of k_mos_sum.  The staged operand is
//                            computed: element (r, c) is (w (a_k A[t][q_k][k])) (cos phi_q, -sin phi_q), phi_q from the channel's true
//                            frequency by cycles_phasor as in k_imclean_update; a_k A[t][q_k][k] is formed once per snapshot and channel
//                            in LDS.  The snapshots are looped inside the launch: behind each, the thread flushes
//                            R_N = fma(-A[t][p][k], acc, R_N) into its own 32 elements and clears its accumulators -- the thread owns
//                            them, so nothing is synchronised and there is one set of accumulators.  Only where a_k != 0; a tile whose
//                            a_k are all 0 returns at once, so an ended channel keeps its bits.
// At the end F of the final R_N once more, k_mos_finish on R_N and Q (the residual in true fluxes, the effective beam) and
// k_imclean_restore on the residual.  No atomics, no sum split over workgroups.  Built with -ffp-contract=off; the fused multiply-adds
// are written as fma().  The results are gathered in host buffers and copied out when the call can no longer fail.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/prisim_mosclean.h"
#include "../csrc_addon/beam_setup.h"
#include "../csrc_addon/mosclean_plan.h"
#include "clean_kernels.h"
#include "imaging_kernels.h"
#include "mosaic_kernels.h"

namespace {

// grid-stride over count * nchan: the beam is 0 below the horizon
__global__ void __launch_bounds__(kThreads) k_mosclean_horizon(const double4* __restrict__ s4, int64_t count, int nchan, double* __restrict__ pb) {
  const int64_t total = count * nchan;
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kThreads)
    if (s4[e / nchan].z < 0.0) pb[e] = 0.0;
}

// grid-stride over npix * nchan: F = R_N / sqrt(Q Wtot) where Q >= pbmin^2 Wtot, else NaN
__global__ void __launch_bounds__(kThreads) k_mosclean_flat(const double* __restrict__ N, const double* __restrict__ Q, const double* __restrict__ wtot,
                                                            int64_t npix, int nchan, double pbmin, double* __restrict__ F) {
  const int64_t total = npix * nchan;
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kThreads) {
    const double w = wtot[e % nchan], q = Q[e];
    F[e] = q >= (pbmin * pbmin) * w ? N[e] / sqrt(q * w) : NAN;
  }
}

// grid: x over the pixels.  The band: the sums of k_mos_finish_band, k ascending; wband[0] = sum_k wtot[k]
__global__ void __launch_bounds__(kThreads) k_mosclean_flat_band(const double* __restrict__ N, const double* __restrict__ Q,
                                                                 const double* __restrict__ wband, int64_t npix, int nchan, double pbmin,
                                                                 double* __restrict__ F) {
  const int64_t pl = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (pl >= npix) return;
  double n = 0.0, q = 0.0;
  for (int k = 0; k < nchan; ++k) {
    n += N[pl * nchan + k];
    q += Q[pl * nchan + k];
  }
  const double w = wband[0];
  F[pl] = q >= (pbmin * pbmin) * w ? n / sqrt(q * w) : NAN;
}

// the flux of prisim_clean_mosaic: the mosaic value at the pick, from R_N and Q themselves
struct MosaicFlux {
  const double *N, *Q;      // [npix][nchan]
  int nchan, avg;
  __device__ __forceinline__ double operator()(int32_t p, int k) const {
    const int64_t at = (int64_t)p * nchan;
    if (!avg) return N[at + k] / Q[at + k];
    double n = 0.0, q = 0.0;
    for (int c = 0; c < nchan; ++c) {
      n += N[at + c];
      q += Q[at + c];
    }
    return n / q;
  }
};

struct MosUpdParams {
  ImgWeights W;
  const double* bl;         // [nbl][3]
  const double* freqs;      // [nchan]
  const double4* dd;        // [nt][npix]
  const double* A;          // [nt][npix][nchan] the beam table
  const int32_t* q;         // [nc] the picks
  const double* a;          // [nc] their fluxes
  double df;
  int64_t nbl, nt, npix;
  int nchan, avg;           // avg: one (q, a) for the band
  double* RN;               // [npix][nchan], updated in place
};

// grid: x = block of pixels, y = channel tile.  LDS: kImagingLds + 20 B per channel of the tile
template <bool STEPPED>
__global__ void __launch_bounds__(kThreads) k_mosclean_update(MosUpdParams P) {
  __shared__ double2 sh_v[NB * CT];     // (w (a_k A_q)) (cos phi_q, -sin phi_q)
  __shared__ double sh_b[NB * 3];       // b / c
  __shared__ double sh_f[CT];           // the tile's frequencies; past the band: the last channel's (their operand rows are 0)
  __shared__ double sh_a[CT];           // the tile's fluxes; past the band: 0
  __shared__ double sh_wa[CT];          // a_k A[t][q_k][k] of the snapshot in hand
  __shared__ int32_t sh_q[CT];
  const int tid = threadIdx.x;
  const int k0 = (int)blockIdx.y * CT;
  // a tile with nothing to subtract returns at once: every thread reads the same 32 fluxes, so the branch is uniform
  bool any = false;
  for (int c = 0; c < CT; ++c) any = any || (k0 + c < P.nchan && P.a[P.avg ? 0 : k0 + c] != 0.0);
  if (!any) return;
  const int64_t pl_raw = (int64_t)blockIdx.x * kThreads + tid;
  const bool p_valid = pl_raw < P.npix;
  const int64_t pl = p_valid ? pl_raw : P.npix - 1;
  double my_a = 0.0;                    // of thread tid < CT: the flux and the pick of channel k0 + tid
  int32_t my_q = 0;
  if (tid < CT) {
    const bool in = k0 + tid < P.nchan;
    my_a = in ? P.a[P.avg ? 0 : k0 + tid] : 0.0;
    my_q = in ? P.q[P.avg ? 0 : k0 + tid] : 0;
    sh_f[tid] = P.freqs[in ? k0 + tid : P.nchan - 1];
    sh_a[tid] = my_a;
    sh_q[tid] = my_q;
  }
  double acc[CT];
#pragma unroll
  for (int k = 0; k < CT; ++k) acc[k] = 0.0;
  const double f0 = P.freqs[k0];

  auto stage = [&P](bool live, int64_t t, int64_t b, int c, int k) {
    double2 v = make_double2(0.0, 0.0);
    const double ak = sh_wa[c];
    if (live && ak != 0.0) {                      // ak != 0 only inside the band, and where the pick is up in this snapshot
      const double w = P.W.at(t, b, k);
      const double4 dq = P.dd[t * P.npix + sh_q[c]];
      const double* bl = P.bl + b * 3;
      const double tau = ((bl[0] * kInvC) * dq.x + (bl[1] * kInvC) * dq.y) + (bl[2] * kInvC) * dq.z;
      double cq, sq;
      cycles_phasor(sh_f[c] * tau, cq, sq);
      const double wa = w * ak;
      v = make_double2(wa * cq, -(wa * sq));
    }
    return v;
  };
  double* rn = P.RN + pl * P.nchan + k0;
  for (int64_t t = 0; t < P.nt; ++t) {
    // the staging of the snapshot before is over for every thread (the second barrier of its last pass), and the first barrier of the
    // pass below stands between this write and the staging that reads it
    if (tid < CT) sh_wa[tid] = my_a != 0.0 ? my_a * P.A[(t * P.npix + my_q) * P.nchan + k0 + tid] : 0.0;
    img_tile_pass<STEPPED, false>(t, P.dd[t * P.npix + pl], P.bl, P.nbl, k0, f0, P.df, sh_v, sh_b, sh_f, acc, stage);
    const double* Ap = P.A + (t * P.npix + pl) * P.nchan + k0;
#pragma unroll
    for (int k = 0; k < CT; ++k) {
      if (p_valid && sh_a[k] != 0.0) rn[k] = fma(-Ap[k], acc[k], rn[k]);     // sh_a[k] != 0 only inside the band
      acc[k] = 0.0;
    }
  }
}

int clean_mosaic(prisim_ctx* ctx, const prisim_mosclean_args* a, double* out_residual, double* out_restored, double* out_residual_flat,
                 double* out_pb_eff, double* out_num, double* out_den, double* out_wsum, int32_t* out_comp_pixel, double* out_comp_flux,
                 int32_t* out_ncomp, int32_t* out_status, double* out_peak0, prisim_mosclean_stats* stats) {
  if (!ctx) return PRISIM_EINVAL;
  const WallTime wall0 = wall_now();
  if (!a) return fail(ctx, PRISIM_EINVAL, "the argument struct is NULL");
  if (!out_residual) return fail(ctx, PRISIM_EINVAL, "out_residual is NULL");
  if (!out_comp_pixel || !out_comp_flux || !out_ncomp || !out_status || !out_peak0)
    return fail(ctx, PRISIM_EINVAL, "out_comp_pixel, out_comp_flux, out_ncomp, out_status or out_peak0 is NULL");
  const ImgView v = imaging_view(*a);
  if (int rc = check_args(ctx, v)) return rc;
  if (int rc = check_mosaic_beam(ctx, *a)) return rc;
  const int64_t npix = a->npix, nbl = a->nbl, nchan = a->nchan, nt = a->nt, maxiter = a->maxiter;
  const bool avg = a->chan_avg != 0, restore = out_restored != nullptr;
  const int64_t nc = avg ? 1 : nchan;
  if (int rc = check_clean_args(ctx, *a, nc, restore)) return rc;
  ImgSetup su{};
  if (int rc = imaging_preamble(ctx, v, su)) return rc;
  const MoscleanPlan pl = mosclean_plan(npix, nbl, nchan, nt, avg, maxiter, a->budget_bytes, su.lds_max, a->route, su.uniform);
  if (pl.refusal)
    return fail(ctx, PRISIM_EINVAL, std::string(pl.refusal) + " (the resident buffers take " + std::to_string(pl.total) + " B, the workgroup " +
                                        std::to_string(pl.lds) + " B of LDS)");
  const ImcleanPlan& cp = pl.clean;
  const bool stepped = cp.route == kImagingStepped;
  const int batch = imclean_batch(a->poll_every);
  const bool timed = stats != nullptr;

  // the results wait here until the call is through: nothing reaches the caller's arrays from a call that fails
  const size_t nimg = (size_t)(npix * nc), nsum = (size_t)(npix * nchan);
  std::vector<double> h_res(nimg), h_rest(restore ? nimg : 0), h_flat(out_residual_flat ? nimg : 0), h_eff(out_pb_eff ? nimg : 0),
      h_num(out_num ? nsum : 0), h_den(out_den ? nsum : 0), h_wsum((size_t)nchan);
  CleanLists lists;
  CleanLoop loop;
  ImgTables T;

  Work wk;
  BatchEvents be;
  Streams& st = wk.st;
  if (int rc = st.create(ctx, 1, false)) return rc;
  hipStream_t s0 = st.s[0];
  if (timed)
    if (int rc = be.create(ctx, 2 * batch + 1)) return rc;

  if (int rc = upload_tables(ctx, wk.dev, v, s0, T)) return rc;
  const ImgWeights& W = T.W;
  int64_t upload = T.bytes;
  double *d_fwhm = nullptr, *d_ones = nullptr, *d_zeros = nullptr;
  uint8_t* d_window = nullptr;
  if (a->window) {
    DEV_UPLOAD(ctx, wk.dev, d_window, a->window, (size_t)npix, s0);
    upload += npix;
  }
  if (restore) {
    DEV_UPLOAD(ctx, wk.dev, d_fwhm, a->fwhm_rad, (size_t)nc, s0);
    upload += nc * 8;
  }
  // the unit flux of the beam statement: pb * 1 * exp2(0 * lg) = pb
  const std::vector<double> ones((size_t)npix, 1.0);
  DEV_UPLOAD(ctx, wk.dev, d_ones, ones, s0);
  DEV_ALLOC(ctx, wk.dev, d_zeros, npix * 8);
  HIPCHK(ctx, hipMemsetAsync(d_zeros, 0, (size_t)npix * 8, s0));
  upload += npix * 8;
  std::vector<const double*> d_bf;
  if (int rc = upload_beamformers(ctx, wk.dev, a->ext, a->n_ext, s0, d_bf, upload)) return rc;
  int32_t* d_flag = nullptr;
  DEV_ALLOC(ctx, wk.dev, d_flag, sizeof(int32_t));
  HIPCHK(ctx, hipMemsetAsync(d_flag, 0, sizeof(int32_t), s0));

  // the resident buffers of the plan
  double4 *d_s4 = nullptr, *d_dd = nullptr;
  double *d_A = nullptr, *d_N = nullptr, *d_Q = nullptr, *d_F = nullptr, *d_res = nullptr, *d_eff = nullptr, *d_wt = nullptr, *d_wtot = nullptr,
         *d_wband = nullptr;
  Peak* d_partial = nullptr;
  CleanState S{};
  DEV_ALLOC(ctx, wk.dev, d_s4, pl.dirs_bytes / 2);
  DEV_ALLOC(ctx, wk.dev, d_dd, pl.dirs_bytes / 2);
  DEV_ALLOC(ctx, wk.dev, d_A, pl.beam_bytes);
  DEV_ALLOC(ctx, wk.dev, d_N, pl.sums_bytes / 2);
  DEV_ALLOC(ctx, wk.dev, d_Q, pl.sums_bytes / 2);
  DEV_ALLOC(ctx, wk.dev, d_F, pl.flat_bytes);
  DEV_ALLOC(ctx, wk.dev, d_res, pl.out_bytes / 2);
  DEV_ALLOC(ctx, wk.dev, d_eff, pl.out_bytes / 2);
  DEV_ALLOC(ctx, wk.dev, d_partial, pl.partial_bytes);
  DEV_ALLOC(ctx, wk.dev, d_wt, nt * nchan * 8);
  DEV_ALLOC(ctx, wk.dev, d_wtot, nchan * 8);
  DEV_ALLOC(ctx, wk.dev, d_wband, 8);
  if (int rc = alloc_clean_state(ctx, wk.dev, S, nc, maxiter)) return rc;

  Events tev;                                           // [0] .. [1] the first residual, [2] .. [3] the finish and the restoration
  if (timed)
    if (int rc = tev.create(ctx)) return rc;
  // the kernels start behind whatever the context's stream still writes into the resident cube, which is read where it lies
  if (v.resident()) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));

  // ---- the first residual: the mosaic's N and Q of all pixels, the beam of every snapshot kept
  if (timed) HIPCHK(ctx, hipEventRecord(tev.e[0], s0));
  if (int rc = enqueue_mos_wsum(ctx, W, nt, nbl, nchan, d_wt, d_wtot, d_wband, s0)) return rc;
  if (int rc = launch(ctx, k_img_dirs, dim3((unsigned)grid_for(ctx, npix * nt)), 0, s0, T.uvec, T.frames, (int64_t)0, npix, nt, d_s4, d_dd)) return rc;
  MosParams M{};
  M.cube = T.cube;
  M.W = W;
  M.bl = T.bl; M.freqs = T.freqs;
  M.df = su.df;
  M.nbl = nbl; M.nchan = (int)nchan;
  M.count = npix;
  M.N = d_N; M.Q = d_Q;
  for (int64_t t = 0; t < nt; ++t) {
    double* At = d_A + t * npix * nchan;
    if (int rc = enqueue_mos_beam(ctx, *a, t, d_bf, d_s4 + t * npix, npix, T.freqs, d_ones, d_zeros, d_flag, At, s0)) return rc;
    if (int rc = launch(ctx, k_mosclean_horizon, dim3((unsigned)grid_for(ctx, npix * nchan)), 0, s0, (const double4*)(d_s4 + t * npix), npix,
                        (int)nchan, At))
      return rc;
    M.dd = d_dd + t * npix; M.s4 = d_s4 + t * npix;
    M.pb = At; M.wt = d_wt + t * nchan;
    M.t = t;
    if (int rc = enqueue_mos_sum(ctx, M, cp.block, cp.ntiles, stepped, s0)) return rc;
  }
  if (int rc = launch(ctx, k_imclean_init, dim3((unsigned)((nc + kThreads - 1) / kThreads)), 0, s0, S, (const double*)(avg ? d_wband : d_wtot), (int)nc))
    return rc;
  if (timed) HIPCHK(ctx, hipEventRecord(tev.e[1], s0));

  // ---- the iterations
  MosUpdParams U;
  U.W = W;
  U.bl = T.bl; U.freqs = T.freqs; U.dd = d_dd; U.A = d_A;
  U.q = S.q; U.a = S.a;
  U.df = su.df;
  U.nbl = nbl; U.nt = nt; U.npix = npix;
  U.nchan = (int)nchan; U.avg = avg ? 1 : 0;
  U.RN = d_N;
  const dim3 grid((unsigned)cp.nblocks, (unsigned)cp.ntiles), pixgrid((unsigned)((npix + kThreads - 1) / kThreads));
  const dim3 peakgrid((unsigned)cp.nslabs, (unsigned)cp.peak_cgroups);
  const MosaicFlux flux{d_N, d_Q, (int)nchan, avg ? 1 : 0};
  auto flat = [&]() -> int {
    if (avg)
      return launch(ctx, k_mosclean_flat_band, pixgrid, 0, s0, (const double*)d_N, (const double*)d_Q, (const double*)d_wband, npix, (int)nchan,
                    a->pbmin, d_F);
    return launch(ctx, k_mosclean_flat, dim3((unsigned)grid_for(ctx, npix * nchan)), 0, s0, (const double*)d_N, (const double*)d_Q,
                  (const double*)d_wtot, npix, (int)nchan, a->pbmin, d_F);
  };
  auto search = [&](bool first) -> int {
    if (int rc = flat()) return rc;
    if (int rc = launch(ctx, k_imclean_peak1, peakgrid, 0, s0, (const double*)d_F, (const uint8_t*)d_window, (const int32_t*)S.status, npix,
                        (int)nc, cp.slab, (int)cp.peak_cx, d_partial))
      return rc;
    hipLaunchKernelGGL(k_imclean_peak2<MosaicFlux>, dim3(1), dim3(kThreads), 0, s0, S, (const Peak*)d_partial, flux, (int)nc, cp.nslabs, maxiter,
                       a->gain, a->threshold, (int)a->threshold_relative, first ? 1 : 0);
    HIPCHK(ctx, hipGetLastError());
    return PRISIM_OK;
  };
  auto update = [&]() -> int {
    return stepped ? launch(ctx, k_mosclean_update<true>, grid, 0, s0, U) : launch(ctx, k_mosclean_update<false>, grid, 0, s0, U);
  };
  if (int rc = loop.run(ctx, s0, S, maxiter, batch, be, search, update)) return rc;

  // ---- the results: F of the final R_N, the residual in true fluxes under the mask, the effective beam
  if (timed) HIPCHK(ctx, hipEventRecord(tev.e[2], s0));
  if (int rc = flat()) return rc;
  if (int rc = enqueue_mos_finish(ctx, avg, d_N, d_Q, d_wtot, d_wband, npix, nchan, a->pbmin, d_res, d_eff, s0)) return rc;
  HIPCHK(ctx, hipMemcpyAsync(h_res.data(), d_res, nimg * 8, hipMemcpyDeviceToHost, s0));
  if (out_residual_flat) HIPCHK(ctx, hipMemcpyAsync(h_flat.data(), d_F, nimg * 8, hipMemcpyDeviceToHost, s0));
  if (out_pb_eff) HIPCHK(ctx, hipMemcpyAsync(h_eff.data(), d_eff, nimg * 8, hipMemcpyDeviceToHost, s0));
  if (out_num) HIPCHK(ctx, hipMemcpyAsync(h_num.data(), d_N, nsum * 8, hipMemcpyDeviceToHost, s0));
  if (out_den) HIPCHK(ctx, hipMemcpyAsync(h_den.data(), d_Q, nsum * 8, hipMemcpyDeviceToHost, s0));
  HIPCHK(ctx, hipMemcpyAsync(h_wsum.data(), d_wtot, (size_t)nchan * 8, hipMemcpyDeviceToHost, s0));
  if (int rc = lists.enqueue(ctx, S, nc, maxiter, s0)) return rc;
  if (restore) {
    if (int rc = launch(ctx, k_imclean_restore, dim3((unsigned)grid_for(ctx, npix * nc)), 0, s0, d_res, T.uvec, S, (const double*)d_fwhm, npix,
                        (int)nc, maxiter))
      return rc;
    HIPCHK(ctx, hipMemcpyAsync(h_rest.data(), d_res, nimg * 8, hipMemcpyDeviceToHost, s0));
  }
  if (timed) HIPCHK(ctx, hipEventRecord(tev.e[3], s0));
  HIPCHK(ctx, hipStreamSynchronize(s0));
  if (int rc = poly_beam_verdict(ctx, a->beam_kind, d_flag)) return rc;
  if (int rc = lists.lists(ctx, S, s0)) return rc;

  std::memcpy(out_residual, h_res.data(), nimg * 8);
  if (restore) std::memcpy(out_restored, h_rest.data(), nimg * 8);
  if (out_residual_flat) std::memcpy(out_residual_flat, h_flat.data(), nimg * 8);
  if (out_pb_eff) std::memcpy(out_pb_eff, h_eff.data(), nimg * 8);
  if (out_num) std::memcpy(out_num, h_num.data(), nsum * 8);
  if (out_den) std::memcpy(out_den, h_den.data(), nsum * 8);
  if (out_wsum) std::memcpy(out_wsum, h_wsum.data(), (size_t)nchan * 8);
  lists.write(out_comp_pixel, out_comp_flux, out_ncomp, out_status, out_peak0);
  if (stats) {
    // the first residual as prisim_mosaic_image counts its kernels, with the horizon pass (8 B a beam value where it writes, 32 B a
    // pixel read).  An iteration, counted with every channel active: the update reads per workgroup and (t, b) the tile's weights
    // (8 B a channel when there are any), the pick's offsets (32 B a channel) and the baseline twice (24 B), per pixel and snapshot its
    // offsets (32 B per tile), per (pixel, channel, snapshot) the beam (8 B) and R_N read and written (16 B), per workgroup, channel
    // and snapshot the beam at the pick (8 B); the search image reads R_N and Q (16 B) and writes F (8 B per image channel); the peak
    // search reads F and the window and writes and reads the partials.
    const int64_t wg = cp.nblocks * cp.ntiles;
    const int64_t row = cp.tile * (16 + (W.w ? 8 : 0)) + 24;
    const int64_t first_bytes = wg * nt * nbl * row + npix * nt * (24 + 64 + 32 + 32 + 64 * cp.ntiles) +
                                npix * nchan * (nt * (8 + 8 + 8 + 16) + (nt - 1) * 16) + (W.w ? nt * nbl * nchan * 8 : 0) + (nt + 2) * nchan * 8;
    const int64_t iter_bytes = wg * nt * (nbl * (cp.tile * (32 + (W.w ? 8 : 0)) + 48) + cp.tile * 8) + npix * nt * 32 * cp.ntiles +
                               npix * nchan * nt * 24 + npix * nchan * 16 + npix * nc * 16 + (a->window ? npix : 0) + cp.nslabs * nc * 32;
    const double mosaic_ms = elapsed_ms(tev.e[0], tev.e[1]), restore_ms = elapsed_ms(tev.e[2], tev.e[3]);
    stats->wall_ms = wall_ms_since(wall0);
    stats->kernel_ms = mosaic_ms + loop.peak_ms + loop.update_ms + restore_ms;
    stats->mosaic_ms = mosaic_ms;
    stats->peak_ms = loop.peak_ms;
    stats->update_ms = loop.update_ms;
    stats->restore_ms = restore_ms;
    stats->beam_values = npix * nchan * nt;
    stats->iterations = loop.counts[1];
    stats->components = lists.components;
    stats->polls = loop.polls;
    stats->chunks = 1;
    stats->chunk_pixels = npix;
    stats->kernel_bytes = first_bytes + loop.counts[1] * iter_bytes + npix * nchan * 16 + npix * nc * (8 + 16 + (restore ? 16 : 0));
    stats->upload_bytes = upload;
    stats->download_bytes = (npix * nc * (1 + (restore ? 1 : 0) + (out_residual_flat ? 1 : 0) + (out_pb_eff ? 1 : 0)) +
                             npix * nchan * ((out_num ? 1 : 0) + (out_den ? 1 : 0)) + nchan) * 8 + nc * 16 + nc * lists.longest * 12 + loop.polls * 16;
    stats->device_bytes = pl.total;
    stats->terms = npix * nbl * nchan * nt;
    stats->route = cp.route;
    stats->streams = 1;
    stats->chan_tile = (int32_t)cp.tile;
    stats->reseed = (int32_t)cp.reseed;
    stats->lds_bytes = (int32_t)pl.lds;
    stats->block_pixels = (int32_t)cp.block;
  }
  return PRISIM_OK;
}

}  // namespace

extern "C" {

int prisim_clean_mosaic(prisim_ctx* ctx, const prisim_mosclean_args* a, double* out_residual, double* out_restored, double* out_residual_flat,
                        double* out_pb_eff, double* out_num, double* out_den, double* out_wsum, int32_t* out_comp_pixel,
                        double* out_comp_flux, int32_t* out_ncomp, int32_t* out_status, double* out_peak0, prisim_mosclean_stats* stats) {
  return guarded(ctx, [&]() -> int {
    return clean_mosaic(ctx, a, out_residual, out_restored, out_residual_flat, out_pb_eff, out_num, out_den, out_wsum, out_comp_pixel,
                        out_comp_flux, out_ncomp, out_status, out_peak0, stats);
  });
}

}  // extern "C"
