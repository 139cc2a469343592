// mosclean_kernels.h -- what the two CLEANs of the mosaic share beside the mosaic's own kernels (mosaic_kernels.h):
// prisim_clean_mosaic (mosclean.hip) and prisim_clean_mosaic_cs (moscs.hip).
//   k_mosclean_horizon       the beam table is 0 where s_z < 0.
//   k_mosclean_flat, _band   the search image F = R_N / sqrt(Q Wtot) under the mask (NaN outside it), [npix][nc]; with chan_avg the
//                            band sums over k ascending.  Bound by device memory: 24 B read a (pixel, channel), 8 B written.
// and the two functions that enqueue them.  Every including file gets its own copy (an unnamed namespace); built with
// -ffp-contract=off.  Not part of the public ABI.
#ifndef PRISIM_MOSCLEAN_KERNELS_H
#define PRISIM_MOSCLEAN_KERNELS_H

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

// behind enqueue_mos_beam of a snapshot: its beam table At [npix][nchan] is 0 where the direction s4 is below the horizon
inline int enqueue_mosclean_horizon(prisim_ctx* ctx, const double4* s4, int64_t npix, int64_t nchan, double* At, hipStream_t s) {
  return launch(ctx, k_mosclean_horizon, dim3((unsigned)grid_for(ctx, npix * nchan)), 0, s, s4, npix, (int)nchan, At);
}

// F [npix][nc] from R_N and Q [npix][nchan]
inline int enqueue_mosclean_flat(prisim_ctx* ctx, bool avg, const double* N, const double* Q, const double* wtot, const double* wband, int64_t npix,
                                 int64_t nchan, double pbmin, double* F, hipStream_t s) {
  if (avg)
    return launch(ctx, k_mosclean_flat_band, dim3((unsigned)((npix + kThreads - 1) / kThreads)), 0, s, N, Q, wband, npix, (int)nchan, pbmin, F);
  return launch(ctx, k_mosclean_flat, dim3((unsigned)grid_for(ctx, npix * nchan)), 0, s, N, Q, wtot, npix, (int)nchan, pbmin, F);
}

}  // namespace

#endif  // PRISIM_MOSCLEAN_KERNELS_H
