// clean_update.h -- the update of an image-space CLEAN with the exact beam, the hot path of prisim_clean_image (imclean.hip) and
// prisim_clean_mosaic (mosclean.hip): what the component (q_k, a_k) of every channel adds to the visibilities, imaged and taken off.
// It is the tile pass of k_img_sum and k_mos_sum (img_tile_pass of imaging_kernels.h, where it is described), so the same summation
// order.  The staged operand is computed, not loaded: element (r, c) is w x_k (cos phi_q, -sin phi_q), phi_q = 2 pi f_k b_r . dd[t][q_k] / c
// from the channel's true frequency (cycles_phasor), four phasors per thread and pass.  The two entries differ in x_k and in the flush:
//   image    x_k = a_k.  Behind the last snapshot the thread subtracts acc / W[k] from R in place; with chan_avg every channel shares
//            (q, a), the numerators go to the scratch rows and k_imclean_avg_sub sums them over the band.
//   MOSAIC   x_k = a_k A[t][q_k][k], formed once per snapshot and channel in LDS.  Behind each snapshot the thread flushes
//            R_N = fma(-A[t][p][k], acc, R_N) into its own 32 elements and clears its accumulators -- the thread owns them, so nothing
//            is synchronised and there is one set of accumulators.
// Only where a_k != 0; a tile whose a_k are all 0 returns at once, so an ended channel keeps its bits.  No atomics, no sum split over
// workgroups.  Every including file gets its own copy (an unnamed namespace); built with -ffp-contract=off, the fused multiply-adds
// are written as fma().  Not part of the public ABI.
#ifndef PRISIM_CLEAN_UPDATE_H
#define PRISIM_CLEAN_UPDATE_H

#include "clean_kernels.h"

namespace {

struct CleanUpdParams {
  ImgWeights W;
  const double* bl;         // [nbl][3]
  const double* freqs;      // [nchan]
  const double4* dd;        // [nt][npix]
  const double* wsum;       // image: [nchan]
  const double* A;          // MOSAIC: [nt][npix][nchan] the beam table
  const int32_t* q;         // [nc] the picks
  const double* a;          // [nc] their fluxes
  double df;
  int64_t nbl, nt, npix;
  int nchan, avg;           // avg: one (q, a) for the band; image: and the numerators are written to out
  double* out;              // [npix][nchan], updated in place: R, or R_N (MOSAIC); image with avg: the scratch rows, written
};

// grid: x = block of pixels, y = channel tile.  LDS: kImagingLds + 12 B per channel of the tile, 20 B with MOSAIC
template <bool STEPPED, bool MOSAIC>
__global__ void __launch_bounds__(kThreads) k_clean_update(CleanUpdParams P) {
  __shared__ double2 sh_v[NB * CT];     // (w x_k) (cos phi_q, -sin phi_q)
  __shared__ double sh_b[NB * 3];       // b / c
  __shared__ double sh_f[CT];           // the tile's frequencies; past the band: the last channel's (their operand rows are 0)
  __shared__ double sh_a[CT];           // the tile's fluxes; past the band: 0
  __shared__ double sh_wa[CT];          // MOSAIC only (no other instantiation names it): a_k A[t][q_k][k] of the snapshot in hand
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
  if (tid < CT) {
    const bool in = k0 + tid < P.nchan;
    sh_f[tid] = P.freqs[in ? k0 + tid : P.nchan - 1];
    sh_a[tid] = in ? P.a[P.avg ? 0 : k0 + tid] : 0.0;
    sh_q[tid] = in ? P.q[P.avg ? 0 : k0 + tid] : 0;
  }
  double acc[CT];
#pragma unroll
  for (int k = 0; k < CT; ++k) acc[k] = 0.0;
  const double f0 = P.freqs[k0];

  auto stage = [&P](bool live, int64_t t, int64_t b, int c, int k) {
    double2 v = make_double2(0.0, 0.0);
    double ak;
    if constexpr (MOSAIC) ak = sh_wa[c]; else ak = sh_a[c];
    if (live && ak != 0.0) {                      // ak != 0 only inside the band, and (MOSAIC) where the pick is up in this snapshot
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
  double* out = P.out + pl * P.nchan + k0;
  for (int64_t t = 0; t < P.nt; ++t) {
    // thread tid < CT reads back the flux and the pick it wrote itself.  The staging of the snapshot before is over for every thread
    // (the second barrier of its last pass), and the first barrier of the pass below stands between this write and the staging that
    // reads it
    if constexpr (MOSAIC)
      if (tid < CT) {
        const double my_a = sh_a[tid];
        sh_wa[tid] = my_a != 0.0 ? my_a * P.A[(t * P.npix + sh_q[tid]) * P.nchan + k0 + tid] : 0.0;
      }
    img_tile_pass<STEPPED, false>(t, P.dd[t * P.npix + pl], P.bl, P.nbl, k0, f0, P.df, sh_v, sh_b, sh_f, acc, stage);
    if constexpr (MOSAIC) {
      const double* Ap = P.A + (t * P.npix + pl) * P.nchan + k0;
#pragma unroll
      for (int k = 0; k < CT; ++k) {
        if (p_valid && sh_a[k] != 0.0) out[k] = fma(-Ap[k], acc[k], out[k]);   // sh_a[k] != 0 only inside the band
        acc[k] = 0.0;
      }
    }
  }
  if constexpr (!MOSAIC) {
    if (!p_valid) return;
    if (P.avg) {
#pragma unroll
      for (int k = 0; k < CT; ++k)
        if (k0 + k < P.nchan) out[k] = acc[k];
    } else {
#pragma unroll
      for (int k = 0; k < CT; ++k)
        if (sh_a[k] != 0.0) out[k] -= acc[k] / P.wsum[k0 + k];
    }
  }
}

// one update over the call's grid, behind a decision: norm is W [nchan], or with MOSAIC the beam table; out as CleanUpdParams has it
template <bool MOSAIC>
inline int enqueue_clean_update(const CleanCall& c, const double4* dd, const double* norm, double* out) {
  CleanUpdParams U{};
  U.W = c.T.W;
  U.bl = c.T.bl; U.freqs = c.T.freqs; U.dd = dd;
  if (MOSAIC) U.A = norm; else U.wsum = norm;
  U.q = c.S.q; U.a = c.S.a;
  U.df = c.su.df;
  U.nbl = c.v.nbl; U.nt = c.v.nt; U.npix = c.npix;
  U.nchan = (int)c.nchan; U.avg = c.avg ? 1 : 0;
  U.out = out;
  const dim3 grid((unsigned)c.pl.nblocks, (unsigned)c.pl.ntiles);
  return c.pl.route == kImagingStepped ? launch(c.ctx, k_clean_update<true, MOSAIC>, grid, 0, c.s0, U)
                                       : launch(c.ctx, k_clean_update<false, MOSAIC>, grid, 0, c.s0, U);
}

}  // namespace

#endif  // PRISIM_CLEAN_UPDATE_H
