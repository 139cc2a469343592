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
// The weight sums, the band average, the job and the count of the bytes are in dirty_frame.h, which the fp32 route (imaging32_kernels.h)
// shares.  Every including file gets its own copy (an unnamed namespace); built with -ffp-contract=off.  Not part of the public ABI.
#ifndef PRISIM_DIRTY_IMAGE_H
#define PRISIM_DIRTY_IMAGE_H

#include "dirty_frame.h"

namespace {

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

}  // namespace

#endif  // PRISIM_DIRTY_IMAGE_H
