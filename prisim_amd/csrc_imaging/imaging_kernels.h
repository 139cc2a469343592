// imaging_kernels.h -- what the three entries of this directory share: prisim_dirty_image (imaging.hip), prisim_clean_image
// (imclean.hip) and prisim_mosaic_image (mosaic.hip).  On the device the direction kernel and the tile pass, the one statement of the
// hot loop of all three; on the host the view of the arguments the three take alike with its checks, the preamble, the upload of the
// tables, the refusal of a plan and the fields of the stats that come from one.  The dirty image itself, which the first two run, is in
// dirty_image.h.  Every including file gets its own copy (an unnamed namespace); built with -ffp-contract=off.  Not part of the
// public ABI.
#ifndef PRISIM_IMAGING_KERNELS_H
#define PRISIM_IMAGING_KERNELS_H

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/prisim_imaging.h"
#include "../csrc_addon/addon_internal.h"
#include "../csrc_addon/imaging_plan.h"

namespace {

static_assert(kImagingBlock == kThreads, "the tile pass gives one thread to every pixel of a block");
static_assert(kImagingReseed == kImagingTile, "the tile pass seeds a tile once: its first channel is the only seed");
static_assert(kImagingRows * kImagingTile % kThreads == 0, "the workgroup stages the rows in whole passes");

constexpr int CT = kImagingTile, NB = kImagingRows;
constexpr double kInvC = 1.0 / 299792458.0;

// ---- device ---------------------------------------------------------------------------------------------------------------------

struct ImgFrame { double rot[9], beta[3], pc[3], pad_; };   // per snapshot, 128 B

// grid-stride over nt * count, of pixels [p0, p0 + count): s = normalise(R_t (u + beta_t)), the statement of k_ap_dirs
// (../csrc_antpower/antpower.hip) operation by operation; dd [nt][count] = s - s0[t] as (dx, dy, dz, 0) and, unless s4 is null,
// s4 [nt][count] = s as (l, m, n, 0), the rows BeamParams.dirs reads
__global__ void __launch_bounds__(kThreads) k_img_dirs(const double* __restrict__ uvec, const ImgFrame* __restrict__ frames, int64_t p0,
                                                       int64_t count, int64_t nt, double4* __restrict__ s4, double4* __restrict__ dd) {
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
    const double l = v0 / nrm, m = v1 / nrm, n = v2 / nrm;
    if (s4) s4[e] = make_double4(l, m, n, 0.0);
    dd[e] = make_double4(l - fr.pc[0], m - fr.pc[1], n - fr.pc[2], 0.0);
  }
}

// the weight of (t, b, k): a broadcast axis has stride 0; w == null: 1
struct ImgWeights {
  const double* w;
  int64_t st, sb, sk;
  __device__ __forceinline__ double at(int64_t t, int64_t b, int k) const { return w ? w[t * st + b * sb + k * sk] : 1.0; }
};

// wtot[0] = sum_k wsum[k], k ascending (one thread)
__global__ void k_img_wtot(const double* __restrict__ wsum, int nchan, double* __restrict__ wtot) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double s = 0.0;
  for (int k = 0; k < nchan; ++k) s += wsum[k];
  wtot[0] = s;
}

// the phasor (cos, sin) of x cycles: the fraction of a cycle is exact in fp64, sincospi rounds it once
__device__ __forceinline__ void cycles_phasor(double x, double& c, double& s) {
  const double r = x - rint(x);
  sincospi(2.0 * r, &s, &c);
}

// the phasor of a point at the offset d from the phase centre on the baseline (b0, b1, b2) = b / c, at the true frequency f
__device__ __forceinline__ void point_phasor(double b0, double b1, double b2, double4 d, double f, double& c, double& s) {
  const double tau = (b0 * d.x + b1 * d.y) + b2 * d.z;
  cycles_phasor(f * tau, c, s);
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

// The tile pass: the hot loop of k_img_sum (dirty_image.h), k_mos_sum (mosaic_kernels.h) and k_clean_update (clean_update.h), whose bits
// agree because this is the one statement of it.  A workgroup owns 256 pixels (one per thread) and a tile of CT = 32 channels from k0
// on; a thread keeps 32 fp64 accumulators and the phasor, nothing else per lane.  For snapshot t, NB = 32 baselines at a time, the
// workgroup stages the operand of the tile in sh_v and b / c in sh_b; every lane then reads the same LDS address in img_rows (a
// broadcast, no bank conflict).  Per (pixel, t, b): tau = b . d / c with d the pixel's offset from the phase centre, then
//   STEPPED  the seed e^{2 pi i f tau} at the tile's first channel from that channel's true frequency f0, the phase reduced to a
//            fraction of a cycle in fp64 before sincospi, and the step e^{2 pi i df tau}; per channel two FMAs into the accumulator and
//            one complex multiply (two products, two FMAs) on the phasor: 6 fp64 instructions, 10 flop;
//   DIRECT   the reduced phase and sincospi of every channel, from the tile's frequencies in sh_f.
// stage(live, t, b, c, k) gives the staged element of baseline b and channel k = k0 + c: the (w Re V, w Im V) of the dirty image, (w, 0)
// of the beam, or what CLEAN subtracts, and zero where it has nothing to add: past the band, and wherever the row is not live, that is
// past the pass's last baseline, where it must not read anything by b.  (It is told so and not skipped, so that what it reads of its
// channel alone is read once per thread and pass, ahead of the test, as CLEAN's flux is: skipping costs k_clean_update<STEPPED, false> half
// a percent.)  The caller writes sh_f (and whatever else its stage reads from LDS) before the first pass without a barrier
// of its own: the first barrier here covers it.  The terms of a (pixel, channel) are added by one thread, b ascending, and the caller
// passes its snapshots ascending: no atomics, no split of the sum over workgroups, so the bits do not depend on chunks or streams.  The
// fused multiply-adds are written as fma(): nothing else is contracted.
template <bool STEPPED, bool PSF, typename Stage>
__device__ __forceinline__ void img_tile_pass(int64_t t, double4 d, const double* bl, int64_t nbl, int k0, double f0, double df, double2* sh_v,
                                              double* sh_b, const double* sh_f, double (&acc)[CT], Stage stage) {
  const int tid = threadIdx.x;
  for (int64_t b0 = 0; b0 < nbl; b0 += NB) {
    const int nb = nbl - b0 < NB ? (int)(nbl - b0) : NB;
    __syncthreads();                      // the rows of the block before are read (and the caller's LDS is written, the first time)
#pragma unroll
    for (int e = tid; e < NB * CT; e += kThreads) {
      const int r = e / CT, c = e - r * CT;
      sh_v[e] = stage(r < nb, t, b0 + r, c, k0 + c);
    }
    if (tid < nb * 3) sh_b[tid] = bl[b0 * 3 + tid] * kInvC;
    __syncthreads();
    img_rows<STEPPED, PSF>(nb, sh_v, sh_b, sh_f, d, f0, df, acc);
  }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------

// The fields prisim_imaging_args, prisim_mosaic_args and prisim_imclean_args have alike, under one name each.  kind is that of
// prisim_dirty_image, the one entry that has it; the others image the cube.
struct ImgView {
  int64_t npix, nbl, nchan, nt, budget_bytes;
  const double *unitvec, *rot, *aberr_beta, *pc_dircos, *baselines, *freqs_hz, *cube, *weights;
  int32_t kind, weight_form, chan_avg, route;
  bool psf() const { return kind == PRISIM_IMAGE_PSF; }
  bool resident() const { return !psf() && !cube; }     // the context's resident cube is read
};
template <typename Args>
inline ImgView imaging_view(const Args& a, int32_t kind = PRISIM_IMAGE_DIRTY) {
  return ImgView{a.npix, a.nbl, a.nchan, a.nt, a.budget_bytes, a.unitvec, a.rot, a.aberr_beta, a.pc_dircos, a.baselines, a.freqs_hz, a.cube,
                 a.weights, kind, a.weight_form, a.chan_avg, a.route};
}

inline bool unit_to(const double* u, double tol) { return std::fabs(std::sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]) - 1.0) <= tol; }

// the checks of the shared fields, behind the entry's own of its struct and its outputs
inline int check_args(prisim_ctx* ctx, const ImgView& a) {
  if (!a.unitvec) return fail(ctx, PRISIM_EINVAL, "unitvec is NULL");
  if (!a.rot) return fail(ctx, PRISIM_EINVAL, "rot is NULL");
  if (!a.pc_dircos) return fail(ctx, PRISIM_EINVAL, "pc_dircos is NULL");
  if (!a.baselines) return fail(ctx, PRISIM_EINVAL, "baselines is NULL");
  if (!a.freqs_hz) return fail(ctx, PRISIM_EINVAL, "freqs_hz is NULL");
  if (a.npix < 1 || a.nbl < 1 || a.nchan < 1 || a.nt < 1) return fail(ctx, PRISIM_EINVAL, "need npix, nbl, nchan and nt >= 1");
  if (a.nchan > (int64_t)1 << 20) return fail(ctx, PRISIM_EINVAL, "nchan must be at most 2^20");
  if (a.nt > (int64_t)1 << 30 || a.nbl > (int64_t)1 << 30) return fail(ctx, PRISIM_EINVAL, "nt and nbl must be at most 2^30");
  if (a.npix > ((int64_t)1 << 46) / a.nchan) return fail(ctx, PRISIM_EINVAL, "npix * nchan must be at most 2^46");
  if (a.kind != PRISIM_IMAGE_DIRTY && a.kind != PRISIM_IMAGE_PSF) return fail(ctx, PRISIM_EINVAL, "unknown kind");
  if (a.route < PRISIM_IMAGE_AUTO || a.route > PRISIM_IMAGE_STEPPED) return fail(ctx, PRISIM_EINVAL, "unknown route");
  if (a.weight_form < PRISIM_IMAGE_W_NONE || a.weight_form > PRISIM_IMAGE_W_FULL) return fail(ctx, PRISIM_EINVAL, "unknown weight form");
  if (a.chan_avg != 0 && a.chan_avg != 1) return fail(ctx, PRISIM_EINVAL, "chan_avg must be 0 or 1");
  if (a.weight_form != PRISIM_IMAGE_W_NONE && !a.weights) return fail(ctx, PRISIM_EINVAL, "weights is NULL with a weight form that reads them");
  for (int64_t f = 0; f < a.nchan; ++f)
    if (!(a.freqs_hz[f] > 0.0) || !std::isfinite(a.freqs_hz[f]))
      return fail(ctx, PRISIM_EINVAL, "freqs_hz[" + std::to_string(f) + "] is not positive and finite");
  for (int64_t p = 0; p < a.npix; ++p)
    if (!unit_to(a.unitvec + p * 3, 1e-6))
      return fail(ctx, PRISIM_EINVAL, "unitvec[" + std::to_string(p) + "] does not have unit length (to 1e-6)");
  for (int64_t i = 0; i < a.nbl * 3; ++i)
    if (!std::isfinite(a.baselines[i])) return fail(ctx, PRISIM_EINVAL, "baseline " + std::to_string(i / 3) + " is not finite");
  {
    // The phase range, by the rule and in the sentence of prisim_hip_set_array (../csrc/capi.cpp): |s - s0| <= 2 for unit vectors, so
    // below max|b| 2 max|f| / c = 2^29 cycles a phase keeps 2^-23 of a cycle and more in cycles_phasor's x - rint(x); past 2^52 cycles
    // that fraction would be 0 and every phasor 1.  Refused here, on the host and before any launch.
    double lmax = 0.0, fmax = 0.0;
    for (int64_t b = 0; b < a.nbl; ++b) {
      const double* v = a.baselines + b * 3;
      const double len = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
      if (std::isfinite(len)) lmax = std::fmax(lmax, len); else lmax = INFINITY;   // finite components whose square overflows
    }
    for (int64_t f = 0; f < a.nchan; ++f) fmax = std::fmax(fmax, a.freqs_hz[f]);
    const double cycles = lmax * 2.0 * fmax / 299792458.0;
    if (!(cycles < 536870912.0)) {
      char msg[200];
      snprintf(msg, sizeof msg, "phase range: max|b| * 2 * max|f| / c = %.6g cycles, the limit is below 2^29 = 536870912 cycles", cycles);
      return fail(ctx, PRISIM_EINVAL, msg);
    }
  }
  for (int64_t t = 0; t < a.nt; ++t) {
    const double* R = a.rot + t * 9;
    for (int r = 0; r < 3; ++r)
      for (int q = r; q < 3; ++q) {
        double d = 0.0;
        for (int k = 0; k < 3; ++k) d += R[3 * r + k] * R[3 * q + k];
        if (!(std::fabs(d - (r == q ? 1.0 : 0.0)) <= 1e-9))
          return fail(ctx, PRISIM_EINVAL, "rot of snapshot " + std::to_string(t) + " is not a rotation matrix (rows must be orthonormal to 1e-9)");
      }
    if (a.aberr_beta) {
      const double* b = a.aberr_beta + t * 3;
      if (!((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2] < 1e-4))
        return fail(ctx, PRISIM_EINVAL, "aberr_beta of snapshot " + std::to_string(t) + " must be a velocity / c with |beta| < 0.01");
    }
    if (!unit_to(a.pc_dircos + t * 3, 1e-6))
      return fail(ctx, PRISIM_EINVAL, "pc_dircos of snapshot " + std::to_string(t) + " does not have unit length (to 1e-6)");
  }
  const int64_t nw = a.weight_form == PRISIM_IMAGE_W_NONE ? 0 : a.weight_form == PRISIM_IMAGE_W_BASELINE ? a.nbl : a.nt * a.nbl * a.nchan;
  for (int64_t i = 0; i < nw; ++i)
    if (!(a.weights[i] >= 0.0) || !std::isfinite(a.weights[i])) return fail(ctx, PRISIM_EINVAL, "weights must be finite and non-negative");
  return PRISIM_OK;
}

// the resident cube serves a call of these sizes: no array at all is a matter of state; a cube of another shape than asked for is a
// wrong argument
inline int check_resident_cube(prisim_ctx* ctx, int64_t nbl, int64_t nchan, int64_t nt) {
  if (!ctx->array_set || !ctx->cube.p) return fail(ctx, PRISIM_ESTATE, "no resident visibility cube: set the array first");
  if (nchan != ctx->nchan || nbl != ctx->nbl || nt > ctx->nt_max)
    return fail(ctx, PRISIM_EINVAL, "the resident cube has " + std::to_string(ctx->nt_max) + " slots of " + std::to_string(ctx->nbl) +
                                        " baselines and " + std::to_string(ctx->nchan) + " channels; asked for " + std::to_string(nt) + " of " +
                                        std::to_string(nbl) + " and " + std::to_string(nchan));
  return PRISIM_OK;
}

// what a plan is made from besides the arguments: the LDS a workgroup may take, and whether the channels are a uniform grid of step df
struct ImgSetup { int lds_max; bool uniform; double df; };

// between the checks of an entry and its plan: the resident cube fits the call, the device is the context's, and the set-up
inline int imaging_preamble(prisim_ctx* ctx, const ImgView& v, ImgSetup& su) {
  if (v.resident())
    if (int rc = check_resident_cube(ctx, v.nbl, v.nchan, v.nt)) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (int rc = lds_limit(ctx, su.lds_max)) return rc;
  su.uniform = imaging_grid_uniform(v.freqs_hz, v.nchan, su.df);
  return PRISIM_OK;
}

// why an ImagingPlan (that of prisim_mosaic_image too) cannot run, in full
template <typename Plan> inline std::string plan_refusal(const Plan& pl) {
  return std::string(pl.refusal) + " (one block of " + std::to_string(pl.block) + " pixels takes " + std::to_string(pl.block * pl.pixel_bytes) +
         " B, the workgroup " + std::to_string(pl.lds) + " B of LDS)";
}

// the frames of the snapshots as k_img_dirs reads them
inline std::vector<ImgFrame> snapshot_frames(const ImgView& a) {
  std::vector<ImgFrame> frames((size_t)a.nt);
  for (int64_t t = 0; t < a.nt; ++t) {
    ImgFrame& fr = frames[(size_t)t];
    for (int k = 0; k < 9; ++k) fr.rot[k] = a.rot[t * 9 + k];
    for (int k = 0; k < 3; ++k) {
      fr.beta[k] = a.aberr_beta ? a.aberr_beta[t * 3 + k] : 0.0;
      fr.pc[k] = a.pc_dircos[t * 3 + k];
    }
    fr.pad_ = 0.0;
  }
  return frames;
}

// the tables of a call on the device: outside the budget, up once.  cube: the uploaded one or the context's resident one, null for the
// beam.  bytes: those copied up.  The frames as k_img_dirs reads them lie in host_frames until the copy's stream is synchronised.
struct ImgTables {
  std::vector<ImgFrame> host_frames;
  const double *uvec, *bl, *freqs;
  const ImgFrame* frames;
  const double2* cube;
  ImgWeights W;
  int64_t bytes;
};

inline int upload_tables(prisim_ctx* ctx, Dev& dev, const ImgView& v, hipStream_t s, ImgTables& T) {
  const int64_t ncube = v.nt * v.nbl * v.nchan;
  T.host_frames = snapshot_frames(v);
  double *d_uvec = nullptr, *d_bl = nullptr, *d_freqs = nullptr, *d_w = nullptr;
  ImgFrame* d_frames = nullptr;
  double2* d_cube = nullptr;
  DEV_UPLOAD(ctx, dev, d_uvec, v.unitvec, (size_t)v.npix * 3, s);
  DEV_UPLOAD(ctx, dev, d_frames, reinterpret_cast<const double*>(T.host_frames.data()), (size_t)v.nt * 16, s);
  DEV_UPLOAD(ctx, dev, d_bl, v.baselines, (size_t)v.nbl * 3, s);
  DEV_UPLOAD(ctx, dev, d_freqs, v.freqs_hz, (size_t)v.nchan, s);
  T.bytes = v.npix * 24 + v.nt * 128 + v.nbl * 24 + v.nchan * 8;
  if (!v.psf() && v.cube) {
    DEV_UPLOAD(ctx, dev, d_cube, v.cube, (size_t)ncube * 2, s);
    T.bytes += ncube * 16;
  }
  T.W = ImgWeights{nullptr, 0, 0, 0};
  if (v.weight_form == PRISIM_IMAGE_W_BASELINE) {
    DEV_UPLOAD(ctx, dev, d_w, v.weights, (size_t)v.nbl, s);
    T.W = ImgWeights{d_w, 0, 1, 0};
    T.bytes += v.nbl * 8;
  } else if (v.weight_form == PRISIM_IMAGE_W_FULL) {
    DEV_UPLOAD(ctx, dev, d_w, v.weights, (size_t)ncube, s);
    T.W = ImgWeights{d_w, v.nbl * v.nchan, v.nchan, 1};
    T.bytes += ncube * 8;
  }
  T.uvec = d_uvec; T.frames = d_frames; T.bl = d_bl; T.freqs = d_freqs;
  T.cube = v.psf() ? nullptr : v.resident() ? (const double2*)ctx->cube.p : d_cube;
  return PRISIM_OK;
}

// the fields every stats struct of this directory takes from the call's sizes and its plan
template <typename Stats, typename Plan>
inline void plan_stats(Stats* st, const ImgView& v, const Plan& pl, int streams) {
  st->terms = v.npix * v.nbl * v.nchan * v.nt;
  st->route = pl.route;
  st->streams = streams;
  st->chan_tile = (int32_t)pl.tile;
  st->reseed = (int32_t)pl.reseed;
  st->lds_bytes = (int32_t)pl.lds;
  st->block_pixels = (int32_t)pl.block;
}

}  // namespace

#endif  // PRISIM_IMAGING_KERNELS_H
