// imaging_kernels.h -- the kernels and the argument checks that the entries of this directory share: prisim_dirty_image (imaging.hip)
// and prisim_clean_image (imclean.hip), whose first residual is the dirty image by these very kernels.  Every including file gets
// its own copy (an unnamed namespace); built with -ffp-contract=off.  Not part of the public ABI.
#ifndef PRISIM_IMAGING_KERNELS_H
#define PRISIM_IMAGING_KERNELS_H

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/prisim_imaging.h"
#include "../csrc_addon/addon_internal.h"
#include "../csrc_addon/imaging_plan.h"

namespace {

static_assert(kImagingBlock == kThreads, "k_img_sum gives one thread to every pixel of a block");
static_assert(kImagingReseed == kImagingTile, "k_img_sum seeds a tile once: its first channel is the only seed");
static_assert(kImagingRows * kImagingTile % kThreads == 0, "the workgroup stages the rows in whole passes");

constexpr int CT = kImagingTile, NB = kImagingRows;
constexpr double kInvC = 1.0 / 299792458.0;

struct ImgFrame { double rot[9], beta[3], pc[3], pad_; };   // per snapshot, 128 B

// grid-stride over nt * count: dd [nt][count] (dx, dy, dz, 0) of pixels [p0, p0 + count)
__global__ void __launch_bounds__(kThreads) k_img_dirs(const double* __restrict__ uvec, const ImgFrame* __restrict__ frames, int64_t p0,
                                                       int64_t count, int64_t nt, double4* __restrict__ dd) {
  const int64_t total = nt * count;
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kThreads) {
    const int64_t t = e / count, pl = e - t * count;
    const ImgFrame& fr = frames[t];
    const double* u = uvec + (p0 + pl) * 3;
    const double t0 = u[0] + fr.beta[0], t1 = u[1] + fr.beta[1], t2 = u[2] + fr.beta[2];
    const double v0 = (fr.rot[0] * t0 + fr.rot[1] * t1) + fr.rot[2] * t2;
    const double v1 = (fr.rot[3] * t0 + fr.rot[4] * t1) + fr.rot[5] * t2;
    const double v2 = (fr.rot[6] * t0 + fr.rot[7] * t1) + fr.rot[8] * t2;
    const double nrm = sqrt((v0 * v0 + v1 * v1) + v2 * v2);
    dd[e] = make_double4(v0 / nrm - fr.pc[0], v1 / nrm - fr.pc[1], v2 / nrm - fr.pc[2], 0.0);
  }
}

// the weight of (t, b, k): a broadcast axis has stride 0; w == null: 1
struct ImgWeights { const double* w; int64_t st, sb, sk; };

// grid: x over the channels.  wsum [nchan]
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

// the phasor (cos, sin) of x cycles: the fraction of a cycle is exact in fp64, sincospi rounds it once
__device__ __forceinline__ void cycles_phasor(double x, double& c, double& s) {
  const double r = x - rint(x);
  sincospi(2.0 * r, &s, &c);
}

// The rows of one pass into the accumulators of a pixel: for each of the nb staged baselines, tau = b . d / c and, per channel of the
// tile, acc[k] += row[k].x cos phi - row[k].y sin phi (PSF: the first product alone), phi = 2 pi f_k tau.  STEPPED seeds the phasor at
// f0, the tile's first frequency, and steps it by df; DIRECT takes every channel's own frequency from sh_f.
template <bool STEPPED, bool PSF>
__device__ __forceinline__ void img_rows(int nb, const double2* sh_v, const double* sh_b, const double* sh_f, double4 d, double f0, double df,
                                         double (&acc)[CT]) {
  for (int r = 0; r < nb; ++r) {
    const double tau = (sh_b[r * 3] * d.x + sh_b[r * 3 + 1] * d.y) + sh_b[r * 3 + 2] * d.z;
    const double2* row = sh_v + r * CT;
    if constexpr (STEPPED) {
      double c, s, sc, ss;
      cycles_phasor(f0 * tau, c, s);
      cycles_phasor(df * tau, sc, ss);
#pragma unroll
      for (int k = 0; k < CT; ++k) {
        const double2 v = row[k];
        acc[k] = fma(v.x, c, acc[k]);
        if (!PSF) acc[k] = fma(-v.y, s, acc[k]);
        const double cn = fma(c, sc, -(s * ss));
        s = fma(c, ss, s * sc);
        c = cn;
      }
    } else {
#pragma unroll 4
      for (int k = 0; k < CT; ++k) {
        double c, s;
        cycles_phasor(sh_f[k] * tau, c, s);
        const double2 v = row[k];
        acc[k] = fma(v.x, c, acc[k]);
        if (!PSF) acc[k] = fma(-v.y, s, acc[k]);
      }
    }
  }
}

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

  for (int64_t t = 0; t < P.nt; ++t) {
    const double4 d = P.dd[t * P.count + pl];
    for (int64_t b0 = 0; b0 < P.nbl; b0 += NB) {
      const int nb = P.nbl - b0 < NB ? (int)(P.nbl - b0) : NB;
      __syncthreads();                    // the rows of the block before are read (and sh_f is written, the first time)
#pragma unroll
      for (int e = tid; e < NB * CT; e += kThreads) {
        const int r = e / CT, c = e - r * CT, k = k0 + c;
        double2 v = make_double2(0.0, 0.0);
        if (r < nb && k < P.nchan) {
          const int64_t b = b0 + r;
          const double w = P.W.w ? P.W.w[t * P.W.st + b * P.W.sb + k * P.W.sk] : 1.0;
          if (PSF) {
            v.x = w;
          } else {
            const double2 x = P.cube[(t * P.nbl + b) * P.nchan + k];
            v = make_double2(w * x.x, w * x.y);
          }
        }
        sh_v[e] = v;
      }
      if (tid < nb * 3) sh_b[tid] = P.bl[b0 * 3 + tid] * kInvC;
      __syncthreads();
      img_rows<STEPPED, PSF>(nb, sh_v, sh_b, sh_f, d, f0, P.df, acc);
    }
  }
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

// wtot[0] = sum_k wsum[k], k ascending (one thread)
__global__ void k_img_wtot(const double* __restrict__ wsum, int nchan, double* __restrict__ wtot) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double s = 0.0;
  for (int k = 0; k < nchan; ++k) s += wsum[k];
  wtot[0] = s;
}

bool unit_to(const double* u, double tol) { return std::fabs(std::sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]) - 1.0) <= tol; }

int check_args(prisim_ctx* ctx, const prisim_imaging_args* a, const double* out_image) {
  if (!a) return fail(ctx, PRISIM_EINVAL, "the argument struct is NULL");
  if (!out_image) return fail(ctx, PRISIM_EINVAL, "out_image is NULL");
  if (!a->unitvec) return fail(ctx, PRISIM_EINVAL, "unitvec is NULL");
  if (!a->rot) return fail(ctx, PRISIM_EINVAL, "rot is NULL");
  if (!a->pc_dircos) return fail(ctx, PRISIM_EINVAL, "pc_dircos is NULL");
  if (!a->baselines) return fail(ctx, PRISIM_EINVAL, "baselines is NULL");
  if (!a->freqs_hz) return fail(ctx, PRISIM_EINVAL, "freqs_hz is NULL");
  if (a->npix < 1 || a->nbl < 1 || a->nchan < 1 || a->nt < 1) return fail(ctx, PRISIM_EINVAL, "need npix, nbl, nchan and nt >= 1");
  if (a->nchan > (int64_t)1 << 20) return fail(ctx, PRISIM_EINVAL, "nchan must be at most 2^20");
  if (a->nt > (int64_t)1 << 30 || a->nbl > (int64_t)1 << 30) return fail(ctx, PRISIM_EINVAL, "nt and nbl must be at most 2^30");
  if (a->npix > ((int64_t)1 << 46) / a->nchan) return fail(ctx, PRISIM_EINVAL, "npix * nchan must be at most 2^46");
  if (a->kind != PRISIM_IMAGE_DIRTY && a->kind != PRISIM_IMAGE_PSF) return fail(ctx, PRISIM_EINVAL, "unknown kind");
  if (a->route < PRISIM_IMAGE_AUTO || a->route > PRISIM_IMAGE_STEPPED) return fail(ctx, PRISIM_EINVAL, "unknown route");
  if (a->weight_form < PRISIM_IMAGE_W_NONE || a->weight_form > PRISIM_IMAGE_W_FULL) return fail(ctx, PRISIM_EINVAL, "unknown weight form");
  if (a->chan_avg != 0 && a->chan_avg != 1) return fail(ctx, PRISIM_EINVAL, "chan_avg must be 0 or 1");
  if (a->weight_form != PRISIM_IMAGE_W_NONE && !a->weights) return fail(ctx, PRISIM_EINVAL, "weights is NULL with a weight form that reads them");
  for (int64_t f = 0; f < a->nchan; ++f)
    if (!(a->freqs_hz[f] > 0.0) || !std::isfinite(a->freqs_hz[f]))
      return fail(ctx, PRISIM_EINVAL, "freqs_hz[" + std::to_string(f) + "] is not positive and finite");
  for (int64_t p = 0; p < a->npix; ++p)
    if (!unit_to(a->unitvec + p * 3, 1e-6))
      return fail(ctx, PRISIM_EINVAL, "unitvec[" + std::to_string(p) + "] does not have unit length (to 1e-6)");
  for (int64_t i = 0; i < a->nbl * 3; ++i)
    if (!std::isfinite(a->baselines[i])) return fail(ctx, PRISIM_EINVAL, "baseline " + std::to_string(i / 3) + " is not finite");
  for (int64_t t = 0; t < a->nt; ++t) {
    const double* R = a->rot + t * 9;
    for (int r = 0; r < 3; ++r)
      for (int q = r; q < 3; ++q) {
        double d = 0.0;
        for (int k = 0; k < 3; ++k) d += R[3 * r + k] * R[3 * q + k];
        if (!(std::fabs(d - (r == q ? 1.0 : 0.0)) <= 1e-9))
          return fail(ctx, PRISIM_EINVAL, "rot of snapshot " + std::to_string(t) + " is not a rotation matrix (rows must be orthonormal to 1e-9)");
      }
    if (a->aberr_beta) {
      const double* b = a->aberr_beta + t * 3;
      if (!((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2] < 1e-4))
        return fail(ctx, PRISIM_EINVAL, "aberr_beta of snapshot " + std::to_string(t) + " must be a velocity / c with |beta| < 0.01");
    }
    if (!unit_to(a->pc_dircos + t * 3, 1e-6))
      return fail(ctx, PRISIM_EINVAL, "pc_dircos of snapshot " + std::to_string(t) + " does not have unit length (to 1e-6)");
  }
  const int64_t nw = a->weight_form == PRISIM_IMAGE_W_NONE ? 0 : a->weight_form == PRISIM_IMAGE_W_BASELINE ? a->nbl : a->nt * a->nbl * a->nchan;
  for (int64_t i = 0; i < nw; ++i)
    if (!(a->weights[i] >= 0.0) || !std::isfinite(a->weights[i])) return fail(ctx, PRISIM_EINVAL, "weights must be finite and non-negative");
  return PRISIM_OK;
}

// the resident cube serves a call of these sizes: no array at all is a matter of state; a cube of another shape than asked for is a
// wrong argument
int check_resident_cube(prisim_ctx* ctx, int64_t nbl, int64_t nchan, int64_t nt) {
  if (!ctx->array_set || !ctx->cube.p) return fail(ctx, PRISIM_ESTATE, "no resident visibility cube: set the array first");
  if (nchan != ctx->nchan || nbl != ctx->nbl || nt > ctx->nt_max)
    return fail(ctx, PRISIM_EINVAL, "the resident cube has " + std::to_string(ctx->nt_max) + " slots of " + std::to_string(ctx->nbl) +
                                        " baselines and " + std::to_string(ctx->nchan) + " channels; asked for " + std::to_string(nt) + " of " +
                                        std::to_string(nbl) + " and " + std::to_string(nchan));
  return PRISIM_OK;
}

// the frames of the snapshots as k_img_dirs reads them
std::vector<ImgFrame> snapshot_frames(const prisim_imaging_args* a) {
  std::vector<ImgFrame> frames((size_t)a->nt);
  for (int64_t t = 0; t < a->nt; ++t) {
    ImgFrame& fr = frames[(size_t)t];
    for (int k = 0; k < 9; ++k) fr.rot[k] = a->rot[t * 9 + k];
    for (int k = 0; k < 3; ++k) {
      fr.beta[k] = a->aberr_beta ? a->aberr_beta[t * 3 + k] : 0.0;
      fr.pc[k] = a->pc_dircos[t * 3 + k];
    }
    fr.pad_ = 0.0;
  }
  return frames;
}

template <bool STEPPED>
int launch_sum(prisim_ctx* ctx, bool psf, dim3 grid, hipStream_t s, const ImgParams& P) {
  return psf ? launch(ctx, k_img_sum<STEPPED, true>, grid, 0, s, P) : launch(ctx, k_img_sum<STEPPED, false>, grid, 0, s, P);
}

}  // namespace

#endif  // PRISIM_IMAGING_KERNELS_H
