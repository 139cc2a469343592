// imaging.hip -- the dirty image and the synthesized beam of a visibility cube by the direct Fourier sum for gfx950
// (include/prisim_imaging.h): D[p][k] = sum_t sum_b w (Re V cos phi - Im V sin phi), phi = 2 pi f_k b . (s[p][t] - s0[t]) / c, the adjoint
// of the sky-sum (../csrc/skyvis_kernels.hip, k_skyvis_rec) with pixel <-> baseline and baseline <-> source exchanged: there a lane owns
// a baseline and the source's row of pb * flux is wave-uniform, here a lane owns a pixel and the baseline's row of w V is.
//
// Once per call:
//   k_img_wsum   W[k] = sum_t sum_b w[t][b][k], one thread per channel, t ascending and b ascending inside t.
// Per chunk of pixels (contiguous, a whole number of blocks of 256):
//   k_img_dirs   dd[t][pixel] = normalise(R_t (u + beta_t)) - s0[t], the statement of k_ap_dirs (../csrc_antpower/antpower.hip) operation
//                by operation, less the phase centre.
//   k_img_sum    the hot path.  A workgroup owns 256 pixels (one per thread) and a tile of 32 channels; a thread keeps 32 fp64
//                accumulators and the phasor, nothing else per lane.  For every snapshot, 32 baselines at a time, the workgroup stages
//                (w Re V, w Im V) of the tile and b / c in LDS; every lane then reads the same LDS address (a broadcast, no bank
//                conflict).  Per (pixel, t, b): tau = b . dd / c, then
//                  STEPPED  the seed e^{2 pi i f tau} at the tile's first channel from that channel's true frequency, the phase reduced
//                           to a fraction of a cycle in fp64 before sincospi, and the step e^{2 pi i df tau}; per channel two FMAs into the
//                           accumulator and one complex multiply (two products, two FMAs) on the phasor: 6 fp64 instructions, 10 flop;
//                  DIRECT   the reduced phase and sincospi of every channel.
//                The (t, b) terms of a (pixel, channel) are added by one thread, t ascending, b ascending: no atomics, no split of the
//                sum over workgroups, so the bits do not depend on the chunks.  The fused multiply-adds are written as fma(): the file
//                is built with -ffp-contract=off like the other add-ons, and nothing else is contracted.
//                chan_avg = 0: the thread divides by W[k] and writes the image rows of the chunk; chan_avg = 1: it writes D[p][k] and
//   k_img_avg    sums D over k ascending per pixel and divides by sum_k W[k].
// The chunks alternate between two streams with their own buffers; the results are gathered in a host buffer and copied to the caller's
// arrays when every chunk is in, so that a failed call writes nothing.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
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
      for (int r = 0; r < nb; ++r) {
        const double tau = (sh_b[r * 3] * d.x + sh_b[r * 3 + 1] * d.y) + sh_b[r * 3 + 2] * d.z;
        const double2* row = sh_v + r * CT;
        if constexpr (STEPPED) {
          double c, s, sc, ss;
          cycles_phasor(f0 * tau, c, s);
          cycles_phasor(P.df * tau, sc, ss);
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

template <bool STEPPED>
int launch_sum(prisim_ctx* ctx, bool psf, dim3 grid, hipStream_t s, const ImgParams& P) {
  return psf ? launch(ctx, k_img_sum<STEPPED, true>, grid, 0, s, P) : launch(ctx, k_img_sum<STEPPED, false>, grid, 0, s, P);
}

int dirty_image(prisim_ctx* ctx, const prisim_imaging_args* a, double* out_image, double* out_wsum, prisim_imaging_stats* stats) {
  if (!ctx) return PRISIM_EINVAL;
  const WallTime wall0 = wall_now();
  if (int rc = check_args(ctx, a, out_image)) return rc;
  const int64_t npix = a->npix, nbl = a->nbl, nchan = a->nchan, nt = a->nt;
  const bool psf = a->kind == PRISIM_IMAGE_PSF, avg = a->chan_avg != 0;
  const bool resident = !psf && !a->cube;
  if (resident) {
    // no array at all is a matter of state; a cube of another shape than asked for is a wrong argument
    if (!ctx->array_set || !ctx->cube.p) return fail(ctx, PRISIM_ESTATE, "no resident visibility cube: set the array first");
    if (nchan != ctx->nchan || nbl != ctx->nbl || nt > ctx->nt_max)
      return fail(ctx, PRISIM_EINVAL, "the resident cube has " + std::to_string(ctx->nt_max) + " slots of " + std::to_string(ctx->nbl) +
                                          " baselines and " + std::to_string(ctx->nchan) + " channels; asked for " + std::to_string(nt) + " of " +
                                          std::to_string(nbl) + " and " + std::to_string(nchan));
  }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int lds_max = 0;
  if (int rc = lds_limit(ctx, lds_max)) return rc;
  double df = 0.0;
  const bool uniform = imaging_grid_uniform(a->freqs_hz, nchan, df);
  const ImagingPlan pl = imaging_plan(npix, nbl, nchan, nt, a->weight_form, avg, a->budget_bytes, lds_max, a->route, uniform, kMaxStreams);
  if (pl.refusal)
    return fail(ctx, PRISIM_EINVAL, std::string(pl.refusal) + " (one block of " + std::to_string(pl.block) + " pixels takes " +
                                        std::to_string(pl.block * pl.pixel_bytes) + " B, the workgroup " + std::to_string(pl.lds) + " B of LDS)");
  const Chunks& ch = pl.chunks;
  const int nstreams = ch.nstreams;
  const bool stepped = pl.route == kImagingStepped;

  // the results wait here until every chunk is in: nothing reaches the caller's arrays from a call that fails.  Declared before the
  // streams, so that they outlive every copy in flight on any return path
  const int64_t per_out = avg ? 1 : nchan;
  std::vector<double> h_img((size_t)(npix * per_out));
  std::vector<double> h_wsum((size_t)(avg ? 1 : nchan));

  Work wk;
  Streams& st = wk.st;
  if (int rc = st.create(ctx, nstreams, true)) return rc;
  hipStream_t s0 = st.s[0];

  // the tables go up once on stream 0, outside the budget
  std::vector<ImgFrame> frames((size_t)nt);
  for (int64_t t = 0; t < nt; ++t) {
    ImgFrame& fr = frames[(size_t)t];
    for (int k = 0; k < 9; ++k) fr.rot[k] = a->rot[t * 9 + k];
    for (int k = 0; k < 3; ++k) {
      fr.beta[k] = a->aberr_beta ? a->aberr_beta[t * 3 + k] : 0.0;
      fr.pc[k] = a->pc_dircos[t * 3 + k];
    }
    fr.pad_ = 0.0;
  }
  double *d_uvec = nullptr, *d_frames = nullptr, *d_bl = nullptr, *d_freqs = nullptr, *d_w = nullptr, *d_wsum = nullptr, *d_wtot = nullptr;
  double2* d_cube = nullptr;
  int64_t upload = 0;
  const int64_t ncube = nt * nbl * nchan;
  DEV_UPLOAD(ctx, wk.dev, d_uvec, a->unitvec, (size_t)npix * 3, s0);
  DEV_UPLOAD(ctx, wk.dev, d_frames, reinterpret_cast<const double*>(frames.data()), (size_t)nt * 16, s0);
  DEV_UPLOAD(ctx, wk.dev, d_bl, a->baselines, (size_t)nbl * 3, s0);
  DEV_UPLOAD(ctx, wk.dev, d_freqs, a->freqs_hz, (size_t)nchan, s0);
  upload += npix * 24 + nt * 128 + nbl * 24 + nchan * 8;
  if (!psf && a->cube) {
    DEV_UPLOAD(ctx, wk.dev, d_cube, a->cube, (size_t)ncube * 2, s0);
    upload += ncube * 16;
  }
  ImgWeights W{nullptr, 0, 0, 0};
  if (a->weight_form == PRISIM_IMAGE_W_BASELINE) {
    DEV_UPLOAD(ctx, wk.dev, d_w, a->weights, (size_t)nbl, s0);
    W = ImgWeights{d_w, 0, 1, 0};
    upload += nbl * 8;
  } else if (a->weight_form == PRISIM_IMAGE_W_FULL) {
    DEV_UPLOAD(ctx, wk.dev, d_w, a->weights, (size_t)ncube, s0);
    W = ImgWeights{d_w, nbl * nchan, nchan, 1};
    upload += ncube * 8;
  }
  DEV_ALLOC(ctx, wk.dev, d_wsum, nchan * 8);
  DEV_ALLOC(ctx, wk.dev, d_wtot, 8);
  if (int rc = launch(ctx, k_img_wsum, dim3((unsigned)((nchan + kThreads - 1) / kThreads)), 0, s0, W, nt, nbl, (int)nchan, d_wsum)) return rc;
  hipLaunchKernelGGL(k_img_wtot, dim3(1), dim3(64), 0, s0, (const double*)d_wsum, (int)nchan, d_wtot);
  HIPCHK(ctx, hipGetLastError());

  // per stream: the buffers of one chunk
  double4* d_dd[kMaxStreams] = {};
  double *d_out[kMaxStreams] = {}, *d_avg[kMaxStreams] = {};
  for (int i = 0; i < nstreams; ++i) {
    DEV_ALLOC(ctx, wk.dev, d_dd[i], ch.size * nt * 32);
    DEV_ALLOC(ctx, wk.dev, d_out[i], ch.size * nchan * 8);
    if (avg) DEV_ALLOC(ctx, wk.dev, d_avg[i], ch.size * 8);
  }
  // the kernels start behind whatever the context's stream still writes into the resident cube
  if (resident) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(s0));              // stream 1 starts behind the uploads and the weight sums; the tables are caller memory

  ImgParams base;
  base.cube = psf ? nullptr : resident ? (const double2*)ctx->cube.p : d_cube;
  base.W = W;
  base.bl = d_bl; base.freqs = d_freqs; base.dd = nullptr; base.wsum = d_wsum;
  base.df = df;
  base.nbl = nbl; base.nt = nt; base.count = 0;
  base.nchan = (int)nchan; base.divide = avg ? 0 : 1;
  base.out = nullptr;

  auto kernels = [&](int64_t, Span sp, int i, hipStream_t sc) -> int {
    if (int rc = launch(ctx, k_img_dirs, dim3((unsigned)grid_for(ctx, sp.count * nt)), 0, sc, (const double*)d_uvec,
                        reinterpret_cast<const ImgFrame*>(d_frames), sp.first, sp.count, nt, d_dd[i]))
      return rc;
    ImgParams P = base;
    P.dd = d_dd[i]; P.count = sp.count; P.out = d_out[i];
    const dim3 grid((unsigned)((sp.count + pl.block - 1) / pl.block), (unsigned)pl.ntiles);
    if (int rc = stepped ? launch_sum<true>(ctx, psf, grid, sc, P) : launch_sum<false>(ctx, psf, grid, sc, P)) return rc;
    if (avg)
      return launch(ctx, k_img_avg, dim3((unsigned)((sp.count + kThreads - 1) / kThreads)), 0, sc, (const double*)d_out[i], sp.count, (int)nchan,
                    (const double*)d_wtot, d_avg[i]);
    return PRISIM_OK;
  };
  auto download = [&](int64_t, Span sp, int i, hipStream_t sc) -> int {
    HIPCHK(ctx, hipMemcpyAsync(h_img.data() + (size_t)(sp.first * per_out), avg ? d_avg[i] : d_out[i], (size_t)(sp.count * per_out) * 8,
                               hipMemcpyDeviceToHost, sc));
    return PRISIM_OK;
  };
  if (int rc = chunk_loop(ctx, st, ch, npix, no_step, kernels, download)) return rc;
  HIPCHK(ctx, hipMemcpy(h_wsum.data(), avg ? d_wtot : d_wsum, h_wsum.size() * 8, hipMemcpyDeviceToHost));

  std::memcpy(out_image, h_img.data(), h_img.size() * 8);
  if (out_wsum) std::memcpy(out_wsum, h_wsum.data(), h_wsum.size() * 8);
  if (stats) {
    // k_img_sum, per workgroup (block of pixels, channel tile) and (t, b): the tile's row of the cube (16 B a channel, not for the PSF)
    // and of the weights (8 B a channel when there are any), and the baseline (24 B); per pixel and snapshot its offsets (32 B per
    // tile); the rows of D or of the image written (8 B), read again and averaged with chan_avg.  k_img_dirs: 24 B read and 32 B
    // written per (pixel, snapshot).  k_img_wsum: the weights once.
    const int64_t wg = pl.nblocks * pl.ntiles;
    const int64_t row = pl.tile * ((psf ? 0 : 16) + (W.w ? 8 : 0)) + 24;
    stats->wall_ms = wall_ms_since(wall0);
    stats->kernel_ms = st.kernel_ms;
    stats->terms = npix * nbl * nchan * nt;
    stats->chunks = ch.count;
    stats->chunk_pixels = ch.size;
    stats->kernel_bytes = wg * nt * nbl * row + npix * nt * (24 + 32 + 32 * pl.ntiles) + npix * nchan * 8 * (avg ? 2 : 1) + (avg ? npix * 8 : 0) +
                          (W.w ? ncube * 8 : 0) + nchan * 16;
    stats->upload_bytes = upload;
    stats->download_bytes = (npix * per_out + (int64_t)h_wsum.size()) * 8;
    stats->route = pl.route;
    stats->streams = nstreams;
    stats->chan_tile = (int32_t)pl.tile;
    stats->reseed = (int32_t)pl.reseed;
    stats->lds_bytes = (int32_t)pl.lds;
    stats->block_pixels = (int32_t)pl.block;
  }
  return PRISIM_OK;
}

}  // namespace

extern "C" {

int prisim_dirty_image(prisim_ctx* ctx, const prisim_imaging_args* a, double* out_image, double* out_wsum, prisim_imaging_stats* stats) {
  return guarded(ctx, [&]() -> int { return dirty_image(ctx, a, out_image, out_wsum, stats); });
}

}  // extern "C"
