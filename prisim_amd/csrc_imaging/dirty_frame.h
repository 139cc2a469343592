// dirty_frame.h -- what stands around the sum of a dirty image and does not depend on how its terms are formed: the weight sums
// (k_img_wsum, with k_img_wtot of imaging_kernels.h), the arguments of a sum kernel, the band average (k_img_avg), the job of one dirty
// image with the function that enqueues its weight sums, and the count of the bytes.  dirty_image.h adds the fp64 sum, k_img_sum, and
// imaging32_kernels.h the fp32 one, k_img32_sum: an including file compiles the sum it launches and not the other.  Every including file
// gets its own copy (an unnamed namespace); built with -ffp-contract=off.  Not part of the public ABI.
#ifndef PRISIM_DIRTY_FRAME_H
#define PRISIM_DIRTY_FRAME_H

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

#endif  // PRISIM_DIRTY_FRAME_H
