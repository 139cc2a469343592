// mosaic32_kernels.h -- the fp32 sum of the beam-weighted mosaic (include/prisim_mosaic32.h) and the function that enqueues it:
// k_mos32_sum is the fp32 tile pass of imaging32_kernels.h (img32_tile_pass, img32_rows and sincos_qcycles32.h as they stand) on the
// operand of the fp64 sum of mosaic_kernels.h, (w Re V, w Im V) of one snapshot, with that kernel's epilogue on the fp64 totals.  One
// launch per snapshot, for that kernel's reasons: the order in t, one beam tile for all snapshots, and the register budget -- the beam
// values are read one at a time when the totals are final.
//
// What is fp32 is what the tile pass makes fp32: the sine and cosine of the reduced seed and step phase, the operand rounded once, the
// recurrence along the channels and the partial sums of at most 32 terms.  The totals D_t[p][k], the beam value, W_t and both fused
// multiply-adds of the epilogue, N = fma(A, D_t, N) and Q = fma(A A, W_t, Q), are fp64: Q has the bits of the fp64 entry.  Every
// (pixel, channel) is added by one thread in an order fixed by (nt, nbl) alone; nothing is added by more than one thread.  Every
// including file gets its own copy (an unnamed namespace); built with -ffp-contract=off.  Not part of the public ABI.
#ifndef PRISIM_MOSAIC32_KERNELS_H
#define PRISIM_MOSAIC32_KERNELS_H

#include "imaging32_kernels.h"
#include "mosaic_kernels.h"

namespace {

// grid: x = block of the chunk's pixels, y = channel tile.  LDS: kImaging32Lds, that of k_img32_sum
__global__ void __launch_bounds__(kThreads) k_mos32_sum(MosParams P) {
  __shared__ f32x4 sh_q[R32 / 2 * CT];   // (x_even, x_odd, -y_even, -y_odd), x + i y = (w Re V, w Im V)
  __shared__ double sh_t[R32 * 3];       // b / c
  static_assert(sizeof(f32x4) * (R32 / 2 * CT) + sizeof(double) * (R32 * 3) == (size_t)kImaging32Lds, "the plan reports the LDS of the kernel");
  const int tid = threadIdx.x;
  const int k0 = (int)blockIdx.y * CT;
  const int64_t pl_raw = (int64_t)blockIdx.x * kThreads + tid;
  const bool p_valid = pl_raw < P.count;
  const int64_t pl = p_valid ? pl_raw : P.count - 1;
  const int64_t t = P.t;
  double tot[CT];
#pragma unroll
  for (int k = 0; k < CT; ++k) tot[k] = 0.0;
  const double fc = P.freqs[k0] + (double)KC * P.df;      // k0 < nchan; the centre of a short last tile lies past the band, on the grid's line
  img32_tile_pass<false>(t, P.dd[pl], P.bl, P.nbl, k0, fc, P.df, sh_q, sh_t, tot, [&P](bool live, int64_t t, int64_t b, int, int k) {
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
      P.N[at + k] = fma(A, tot[k], t ? P.N[at + k] : 0.0);
      P.Q[at + k] = fma(A * A, P.wt[k0 + k], t ? P.Q[at + k] : 0.0);
    }
}

// snapshot P.t of P.count pixels in blocks of `block`, ntiles channel tiles
inline int enqueue_mos32_sum(prisim_ctx* ctx, const MosParams& P, int64_t block, int64_t ntiles, hipStream_t s) {
  const dim3 grid((unsigned)((P.count + block - 1) / block), (unsigned)ntiles);
  return launch(ctx, k_mos32_sum, grid, 0, s, P);
}

}  // namespace

#endif  // PRISIM_MOSAIC32_KERNELS_H
