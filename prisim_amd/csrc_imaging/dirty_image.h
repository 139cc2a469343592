// dirty_image.h -- the dirty image and the synthesized beam by the direct Fourier sum, as prisim_dirty_image (imaging.hip) runs it chunk
// by chunk, prisim_clean_image (imclean.hip) once over all pixels for its first residual and prisim_clean_image_cs (csclean.hip) once
// per major cycle, and over offsets of its own for its minor-cycle beam: the kernels, the one function that enqueues them and the one
// count of their bytes.  Once per call:
//   k_img_wsum   W[k] = sum_t sum_b w[t][b][k], one thread per channel, t ascending and b ascending inside t, and k_img_wtot their sum.
// Per chunk of pixels:
//   k_img_dirs   dd[t][pixel] = normalise(R_t (u + beta_t)) - s0[t] (imaging_kernels.h).
//   k_img_sum    the hot path: the tile pass of imaging_kernels.h over every snapshot, t ascending, on (w Re V, w Im V), or (w, 0) for
//                the beam.  chan_avg = 0: the thread divides by W[k] and writes the image rows; chan_avg = 1: it writes D[p][k] and
//   k_img_avg    sums D over k ascending per pixel and divides by sum_k W[k].
// Every including file gets its own copy (an unnamed namespace); built with -ffp-contract=off.  Not part of the public ABI.
#ifndef PRISIM_DIRTY_IMAGE_H
#define PRISIM_DIRTY_IMAGE_H

#include "imaging_kernels.h"

namespace {

// grid: x over the channels.  wsum [nchan].  Not one kernel with k_mos_wsum (mosaic_kernels.h): this one carries one running sum over
// (t, b), that one sums over b within each snapshot and then over t; for weights that are not integers the two orders give different
// bits, and each is pinned by its own checker.
__global__ void __launch_bounds__(kThreads) k_img_wsum(ImgWeights W, int64_t nt, int64_t nbl, int nchan, double* __restrict__ wsum) {
  const int k = (int)blockIdx.x * kThreads + threadIdx.x;
  if (k >= nchan) return;
  double s = 0.0;
  for (int64_t t = 0; t < nt; ++t) {
    const double* row = W.w ? W.w + t * W.st + k * W.sk : nullptr;
#pragma unroll 8
    for (int64_t b = 0; b < nbl; ++b) s += row ? row[b * W.sb] : 1.0;
  }
  wsum[k] = s;
}

struct ImgParams {
  const double2* cube;      // [nt][nbl][nchan]; not read for the PSF
  ImgWeights W;
  const double* bl;         // [nbl][3]
  const double* freqs;      // [nchan]
  const double4* dd;        // [nt][count] of the chunk
  const double* wsum;       // [nchan]
  double df;                // the step of a uniform grid (STEPPED)
  int64_t nbl, nt, count;   // count: pixels of the chunk
  int nchan, divide;        // divide: write D / W (chan_avg = 0), else D
  double* out;              // [count][nchan] of the chunk
};

// grid: x = block of the chunk's pixels, y = channel tile.  LDS: kImagingLds
template <bool STEPPED, bool PSF>
__global__ void __launch_bounds__(kThreads) k_img_sum(ImgParams P) {
  __shared__ double2 sh_v[NB * CT];     // (w Re V, w Im V); PSF: (w, 0)
  __shared__ double sh_b[NB * 3];       // b / c
  __shared__ double sh_f[CT];           // the tile's frequencies; past the band: the last channel's (their operand rows are 0)
  const int tid = threadIdx.x;
  const int k0 = (int)blockIdx.y * CT;
  const int64_t pl_raw = (int64_t)blockIdx.x * kThreads + tid;
  const bool p_valid = pl_raw < P.count;
  const int64_t pl = p_valid ? pl_raw : P.count - 1;
  if (tid < CT) sh_f[tid] = P.freqs[k0 + tid < P.nchan ? k0 + tid : P.nchan - 1];
  double acc[CT];
#pragma unroll
  for (int k = 0; k < CT; ++k) acc[k] = 0.0;
  const double f0 = P.freqs[k0];          // k0 < nchan: the grid has ceil(nchan / CT) tiles
  auto stage = [&P](bool live, int64_t t, int64_t b, int, int k) {
    double2 v = make_double2(0.0, 0.0);
    if (live && k < P.nchan) {
      const double w = P.W.at(t, b, k);
      if (PSF) {
        v.x = w;
      } else {
        const double2 x = P.cube[(t * P.nbl + b) * P.nchan + k];
        v = make_double2(w * x.x, w * x.y);
      }
    }
    return v;
  };
  for (int64_t t = 0; t < P.nt; ++t)
    img_tile_pass<STEPPED, PSF>(t, P.dd[t * P.count + pl], P.bl, P.nbl, k0, f0, P.df, sh_v, sh_b, sh_f, acc, stage);
  if (!p_valid) return;
  double* out = P.out + pl * P.nchan + k0;
#pragma unroll
  for (int k = 0; k < CT; ++k)
    if (k0 + k < P.nchan) out[k] = P.divide ? acc[k] / P.wsum[k0 + k] : acc[k];
}

// grid: x over the chunk's pixels.  avg[pixel] = sum_k D[pixel][k] / wtot, k ascending
__global__ void __launch_bounds__(kThreads) k_img_avg(const double* __restrict__ D, int64_t count, int nchan, const double* __restrict__ wtot,
                                                      double* __restrict__ avg) {
  const int64_t pl = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (pl >= count) return;
  double s = 0.0;
  for (int k = 0; k < nchan; ++k) s += D[pl * nchan + k];
  avg[pl] = s / wtot[0];
}

// One dirty image: what its kernels take besides the buffers of the pixels in hand.  wsum [nchan] and wtot [1] are the caller's.
struct DirtyImage {
  const ImgTables* T;
  double df;
  int64_t nbl, nchan, nt, block, ntiles;
  bool psf, avg, stepped;
  double *wsum, *wtot;
};
template <typename Plan>
inline DirtyImage dirty_image_of(const ImgView& v, const ImgTables& T, double df, const Plan& pl, double* wsum, double* wtot) {
  return DirtyImage{&T, df, v.nbl, v.nchan, v.nt, pl.block, pl.ntiles, v.psf(), v.chan_avg != 0, pl.route == kImagingStepped, wsum, wtot};
}

// the weight sums, once per call and before any pixel: on their own, so that an entry with more than one stream can wait for them
inline int enqueue_weight_sums(prisim_ctx* ctx, const DirtyImage& J, hipStream_t s) {
  if (int rc = launch(ctx, k_img_wsum, dim3((unsigned)((J.nchan + kThreads - 1) / kThreads)), 0, s, J.T->W, J.nt, J.nbl, (int)J.nchan, J.wsum))
    return rc;
  hipLaunchKernelGGL(k_img_wtot, dim3(1), dim3(64), 0, s, (const double*)J.wsum, (int)J.nchan, J.wtot);
  HIPCHK(ctx, hipGetLastError());
  return PRISIM_OK;
}

// `count` pixels whose offsets dd [nt][count] are there, behind the weight sums: sum -> band average.  rows [count][nchan], the image or,
// with chan_avg, D; avg [count], the band's image (chan_avg only).
inline int enqueue_dirty_sums(prisim_ctx* ctx, const DirtyImage& J, int64_t count, const double4* dd, double* rows, double* avg, hipStream_t s) {
  const ImgParams P{J.T->cube, J.T->W, J.T->bl, J.T->freqs, dd, J.wsum, J.df, J.nbl, J.nt, count, (int)J.nchan, J.avg ? 0 : 1, rows};
  const dim3 grid((unsigned)((count + J.block - 1) / J.block), (unsigned)J.ntiles);
  if (int rc = J.stepped ? (J.psf ? launch(ctx, k_img_sum<true, true>, grid, 0, s, P) : launch(ctx, k_img_sum<true, false>, grid, 0, s, P))
                         : (J.psf ? launch(ctx, k_img_sum<false, true>, grid, 0, s, P) : launch(ctx, k_img_sum<false, false>, grid, 0, s, P)))
    return rc;
  if (J.avg)
    return launch(ctx, k_img_avg, dim3((unsigned)((count + kThreads - 1) / kThreads)), 0, s, (const double*)rows, count, (int)J.nchan,
                  (const double*)J.wtot, avg);
  return PRISIM_OK;
}

// The pixels of sp behind the weight sums: directions -> sum -> band average.  dd [nt][count]; rows and avg as enqueue_dirty_sums
// takes them.
inline int enqueue_dirty(prisim_ctx* ctx, const DirtyImage& J, Span sp, double4* dd, double* rows, double* avg, hipStream_t s) {
  if (int rc = launch(ctx, k_img_dirs, dim3((unsigned)grid_for(ctx, sp.count * J.nt)), 0, s, J.T->uvec, J.T->frames, sp.first, sp.count, J.nt,
                      (double4*)nullptr, dd))
    return rc;
  return enqueue_dirty_sums(ctx, J, sp.count, dd, rows, avg, s);
}

// The bytes the kernels of one dirty image of all pixels read and write.  k_img_sum, per workgroup (block of pixels, channel tile) and
// (t, b): the tile's row of the cube (16 B a channel, not for the PSF) and of the weights (8 B a channel when there are any), and the
// baseline (24 B); per pixel and snapshot its offsets (32 B per tile); the rows of D or of the image written (8 B), read again and
// averaged with chan_avg.  k_img_dirs: 24 B read and 32 B written per (pixel, snapshot).  k_img_wsum: the weights once.
template <typename Plan>
inline int64_t dirty_kernel_bytes(const ImgView& v, const Plan& pl, bool weighted) {
  const bool avg = v.chan_avg != 0;
  const int64_t row = pl.tile * ((v.psf() ? 0 : 16) + (weighted ? 8 : 0)) + 24;
  return pl.nblocks * pl.ntiles * v.nt * v.nbl * row + v.npix * v.nt * (24 + 32 + 32 * pl.ntiles) + v.npix * v.nchan * 8 * (avg ? 2 : 1) +
         (avg ? v.npix * 8 : 0) + (weighted ? v.nt * v.nbl * v.nchan * 8 : 0) + v.nchan * 16;
}

}  // namespace

#endif  // PRISIM_DIRTY_IMAGE_H
