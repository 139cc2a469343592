// imaging32_kernels.h -- the fp32 tile pass of the dirty image and the synthesized beam (include/prisim_imaging32.h), the kernel that
// runs it and the function that enqueues it.  What stays fp64 is taken from imaging_kernels.h and dirty_frame.h as it is: the
// directions (k_img_dirs), the weight sums (k_img_wsum, k_img_wtot), the band average (k_img_avg), the checks and the tables.
//
// The shape is that of k_img_sum: a workgroup owns 256 pixels (one per thread) and a tile of CT = 32 channels; the rows of a pass are
// staged in LDS and read by every lane at the same address (a broadcast).  What differs:
//   * a pass stages R32 = 64 baselines, as float: the operand (w Re V, w Im V) is formed in fp64 by the caller's stage() and rounded
//     once.  Two consecutive rows make a pair, and the pair's operands are interleaved, (x_even, x_odd, -y_even, -y_odd) per channel, so
//     that one 128-bit read feeds both.
//   * per pair and pixel: tau = b . d / c of both rows in fp64, the products fc tau and df tau in fp64, fc = f[k0] + 16 df the
//     frequency of the tile's centre channel; the seed's product is reduced to a fraction of a cycle and sincos_qcycles reduces each to a
//     quadrant and a residual, all in fp64, and gives the fp32
//     sine and cosine of seed and step.
//   * the phasors of the pair are 2-vectors (c, s) and the step (sc, ss); the seed is walked up over the channels [16, 32) and down
//     over [0, 16) by one complex multiply a channel, two products and two FMAs on 2-vectors (v_pk_mul_f32, v_pk_fma_f32), and the
//     operand is accumulated by two more FMAs (one for the beam): six packed instructions for two terms.  No chain is longer than 16
//     steps; the two walks do not depend on each other.
//   * the fp32 partial sums acc[k] (a 2-vector: one half per row of the pair) are added into the fp64 totals tot[k] at the end of
//     every pass, tot[k] = (tot[k] + acc[k].x) + acc[k].y, and cleared: a partial sum never holds more than 32 terms.
// The order of a (pixel, channel) is fixed by (nt, nbl) alone -- t ascending, passes ascending, pairs ascending, the even row's half
// before the odd's at the flush -- and one thread adds all of it: the bits do not depend on chunks or streams.  The fused
// multiply-adds are written as builtins; the directory is built with -ffp-contract=off.  Every including file gets its own copy (an
// unnamed namespace).  Not part of the public ABI.
#ifndef PRISIM_IMAGING32_KERNELS_H
#define PRISIM_IMAGING32_KERNELS_H

#include "../csrc_addon/imaging32_plan.h"
#include "dirty_frame.h"
#include "sincos_qcycles32.h"

namespace {

constexpr int R32 = kImaging32Rows, KC = kImaging32Seed;
static_assert(kImaging32Pair == 2, "a packed chain carries two rows");
static_assert(R32 * CT % kThreads == 0 && R32 * 3 <= kThreads, "the workgroup stages the rows in whole sweeps and the baselines in one");

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x2 pk_fma(f32x2 a, f32x2 b, f32x2 c) { return __builtin_elementwise_fma(a, b, c); }

// x cycles less the whole ones, in [-1/2, 1/2]: exact in fp64.  The seed's phase goes through it because fc, the centre of a tile that
// ends the band early, can lie above the band's last frequency, which is what the 2^29-cycle check bounds; sincos_qcycles takes quarter
// cycles below 2^31 only.  The step's df tau is below the checked range as it is.
__device__ __forceinline__ double cycle_fraction(double x) { return x - __builtin_rint(x); }

// The pairs of one pass into the partial sums of a pixel.  sh_q [npair][CT] of (x_even, x_odd, -y_even, -y_odd); sh_t [2 npair][3] of
// b / c.  df4 = 4 df: sincos_qcycles takes quarter cycles, and the factor is exact.
template <bool PSF>
__device__ __forceinline__ void img32_rows(int npair, const f32x4* sh_q, const double* sh_t, double4 d, double fc, double df4, f32x2 (&acc)[CT]) {
  for (int j = 0; j < npair; ++j) {
    const double* b = sh_t + j * 6;
    const double tau0 = (b[0] * d.x + b[1] * d.y) + b[2] * d.z;
    const double tau1 = (b[3] * d.x + b[4] * d.y) + b[5] * d.z;
    f32x2 c, s, sc, ss;
    {
      float c0, s0, c1, s1;
      sincos_qcycles(4.0 * cycle_fraction(fc * tau0), c0, s0);
      sincos_qcycles(4.0 * cycle_fraction(fc * tau1), c1, s1);
      c = f32x2{c0, c1}; s = f32x2{s0, s1};
      sincos_qcycles(df4 * tau0, c0, s0);
      sincos_qcycles(df4 * tau1, c1, s1);
      sc = f32x2{c0, c1}; ss = f32x2{s0, s1};
    }
    const f32x4* row = sh_q + j * CT;
    f32x2 cu = c, su = s, cd = c, sd = s;
#pragma unroll
    for (int i = 0; i < KC; ++i) {
      // down first: the channel KC - 1 - i is i + 1 steps of e^{-i step} from the seed
      const f32x2 cdn = pk_fma(cd, sc, sd * ss);
      sd = pk_fma(sd, sc, -(cd * ss));
      cd = cdn;
      const f32x4 vd = row[KC - 1 - i];
      acc[KC - 1 - i] = pk_fma(f32x2{vd.x, vd.y}, cd, acc[KC - 1 - i]);
      if (!PSF) acc[KC - 1 - i] = pk_fma(f32x2{vd.z, vd.w}, sd, acc[KC - 1 - i]);
      // up: the channel KC + i is i steps of e^{+i step} from the seed
      const f32x4 vu = row[KC + i];
      acc[KC + i] = pk_fma(f32x2{vu.x, vu.y}, cu, acc[KC + i]);
      if (!PSF) acc[KC + i] = pk_fma(f32x2{vu.z, vu.w}, su, acc[KC + i]);
      if (i + 1 < KC) {
        const f32x2 cun = pk_fma(cu, sc, -(su * ss));
        su = pk_fma(cu, ss, su * sc);
        cu = cun;
      }
    }
  }
}

// The fp32 tile pass over the baselines of snapshot t, the counterpart of img_tile_pass (imaging_kernels.h) with the same stage():
// stage(live, t, b, c, k) gives the element of baseline b and channel k = k0 + c in fp64, zero where it has nothing to add, and is
// rounded to float here.  A row past the pass's last baseline is staged as zero with a zero baseline, so the odd row of the last
// pair adds +0.  fc: the frequency of the tile's centre channel.  tot: the fp64 totals, which take the partial sums after every pass.
template <bool PSF, typename Stage>
__device__ __forceinline__ void img32_tile_pass(int64_t t, double4 d, const double* bl, int64_t nbl, int k0, double fc, double df, f32x4* sh_q,
                                                double* sh_t, double (&tot)[CT], Stage stage) {
  const int tid = threadIdx.x;
  float* sh_f = reinterpret_cast<float*>(sh_q);
  for (int64_t b0 = 0; b0 < nbl; b0 += R32) {
    const int nb = nbl - b0 < R32 ? (int)(nbl - b0) : R32;
    __syncthreads();                      // the rows of the pass before are read
#pragma unroll
    for (int e = tid; e < R32 * CT; e += kThreads) {
      const int r = e / CT, c = e - r * CT;
      const double2 v = stage(r < nb, t, b0 + r, c, k0 + c);
      float* q = sh_f + ((r >> 1) * CT + c) * 4 + (r & 1);
      q[0] = (float)v.x;
      q[2] = -(float)v.y;               // the sign of - Im V sin phi is staged, not applied per term
    }
    if (tid < R32 * 3) sh_t[tid] = tid < nb * 3 ? bl[b0 * 3 + tid] * kInvC : 0.0;
    __syncthreads();
    f32x2 acc[CT];
#pragma unroll
    for (int k = 0; k < CT; ++k) acc[k] = f32x2{0.0f, 0.0f};
    img32_rows<PSF>((nb + 1) >> 1, sh_q, sh_t, d, fc, 4.0 * df, acc);
#pragma unroll
    for (int k = 0; k < CT; ++k) tot[k] = (tot[k] + (double)acc[k].x) + (double)acc[k].y;
  }
}

// grid: x = block of the chunk's pixels, y = channel tile.  LDS: kImaging32Lds.  The arguments and the outputs are those of k_img_sum
// (dirty_image.h) on its stepped route.
template <bool PSF>
__global__ void __launch_bounds__(kThreads) k_img32_sum(ImgParams P) {
  __shared__ f32x4 sh_q[R32 / 2 * CT];   // (x_even, x_odd, -y_even, -y_odd), x + i y = (w Re V, w Im V); PSF: (w, 0)
  __shared__ double sh_t[R32 * 3];       // b / c
  static_assert(sizeof(f32x4) * (R32 / 2 * CT) + sizeof(double) * (R32 * 3) == (size_t)kImaging32Lds, "the plan reports the LDS of the kernel");
  const int tid = threadIdx.x;
  const int k0 = (int)blockIdx.y * CT;
  const int64_t pl_raw = (int64_t)blockIdx.x * kThreads + tid;
  const bool p_valid = pl_raw < P.count;
  const int64_t pl = p_valid ? pl_raw : P.count - 1;
  double tot[CT];
#pragma unroll
  for (int k = 0; k < CT; ++k) tot[k] = 0.0;
  const double fc = P.freqs[k0] + (double)KC * P.df;      // k0 < nchan; the centre of a short last tile lies past the band, on the grid's line
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
  for (int64_t t = 0; t < P.nt; ++t) img32_tile_pass<PSF>(t, P.dd[t * P.count + pl], P.bl, P.nbl, k0, fc, P.df, sh_q, sh_t, tot, stage);
  if (!p_valid) return;
  double* out = P.out + pl * P.nchan + k0;
#pragma unroll
  for (int k = 0; k < CT; ++k)
    if (k0 + k < P.nchan) out[k] = P.divide ? tot[k] / P.wsum[k0 + k] : tot[k];
}

// The pixels of sp behind the weight sums, as enqueue_dirty (dirty_image.h) with the fp32 sum: directions -> sum -> band average
inline int enqueue_dirty32(prisim_ctx* ctx, const DirtyImage& J, Span sp, double4* dd, double* rows, double* avg, hipStream_t s) {
  if (int rc = launch(ctx, k_img_dirs, dim3((unsigned)grid_for(ctx, sp.count * J.nt)), 0, s, J.T->uvec, J.T->frames, sp.first, sp.count, J.nt,
                      (double4*)nullptr, dd))
    return rc;
  const ImgParams P{J.T->cube, J.T->W, J.T->bl, J.T->freqs, dd, J.wsum, J.df, J.nbl, J.nt, sp.count, (int)J.nchan, J.avg ? 0 : 1, rows};
  const dim3 grid((unsigned)((sp.count + J.block - 1) / J.block), (unsigned)J.ntiles);
  if (int rc = J.psf ? launch(ctx, k_img32_sum<true>, grid, 0, s, P) : launch(ctx, k_img32_sum<false>, grid, 0, s, P)) return rc;
  if (J.avg)
    return launch(ctx, k_img_avg, dim3((unsigned)((sp.count + kThreads - 1) / kThreads)), 0, s, (const double*)rows, sp.count, (int)J.nchan,
                  (const double*)J.wtot, avg);
  return PRISIM_OK;
}

}  // namespace

#endif  // PRISIM_IMAGING32_KERNELS_H
