// cycle_kernels.h -- the major and minor cycles of a Cotton-Schwab CLEAN, as prisim_clean_image_cs (csclean.hip) and
// prisim_clean_mosaic_cs (moscs.hip) share them: the state of the cycles, the minor-cycle beam P of a lattice with the host code that
// builds it, the decision at the start of a cycle, the minor cycle and the update of the residual visibilities.  What differs between
// the two entries is two small functors: what a component's listed flux is (Flux) and what multiplies it in a snapshot (Beam).
//   k_csclean_offsets the offsets of the half-plane, per snapshot, in the layout k_img_sum reads.
//   k_csclean_mirror  P [nc][2 ny - 1][2 nx - 1] from the rows of the half-plane: a transposition and the mirror, copies only.
//   k_csclean_decide  the start of a cycle, one thread per image channel: reduces the partials of k_imclean_peak1, sets P0 and the
//                     threshold in cycle 0 and counts the channels that go on, each by the piece k_imclean_peak2 calls too
//                     (clean_kernels.h); between them, its own: it records the peak, ends the channel in the order of the header or
//                     sets the cycle's limit.
//   k_csclean_minor   the minor cycle: ONE workgroup per image channel for the whole cycle, which never waits for another (no flags,
//                     no spinning; its loop is bounded by min(cycle_niter, maxiter - ncomp) on the host's word).  The working image
//                     lives in LDS (8 B a pixel; gfx950 lets a workgroup hold 160 KiB, 128 x 128 pixels) or in a device scratch row;
//                     the arithmetic and the assignment of pixels to threads are the same, so the bits are.  A thread owns the pixels
//                     tid, tid + 256, ...; per component it subtracts c P[i_p - i_q][j_p - j_q] from each, c = gain img[q] -- P of the
//                     channel is read from device memory, where it is L2-sized -- and keeps the largest |value| of what it wrote; the
//                     (|value|, index) pairs are reduced under "larger, then lower index" across the lanes of a wave by shuffles and
//                     across the four waves through LDS: two barriers per component.  A NaN pixel stays NaN and never wins.  The
//                     flux that goes into the list is Flux(c, q, k): c itself (PlainFlux), or c times a scale table (FlatFlux).
//   k_csclean_model   Vres -= the cycle's new components: one thread per (t, b, k), components in list order, every phasor from the
//                     channel's true frequency (point_phasor of imaging_kernels.h), the amplitude Beam(a, t, q, k): a itself (NoBeam), or a times the
//                     beam table at the component's pixel (TableBeam).  Channels that did not run a cycle are not touched.
// No atomics, no floating-point reduction whose order depends on the launch.  Every including file gets its own copy (an unnamed
// namespace); built with -ffp-contract=off.  Not part of the public ABI.
#ifndef PRISIM_CYCLE_KERNELS_H
#define PRISIM_CYCLE_KERNELS_H

#include "../../include/prisim_csclean.h"
#include "../csrc_addon/csclean_plan.h"
#include "clean_kernels.h"
#include "dirty_image.h"

namespace {

static_assert(kCscleanAuto == PRISIM_CSCLEAN_AUTO && kCscleanLds == PRISIM_CSCLEAN_LDS && kCscleanGlobal == PRISIM_CSCLEAN_GLOBAL &&
                  kCscleanMaxMajor == PRISIM_CSCLEAN_MAX_MAJOR,
              "the plan and the header agree");
constexpr int kWave = 64, kWaves = kThreads / kWave;
static_assert(kWaves * (int)sizeof(Peak) == kCscleanMinorStatic, "the plan counts the partial peaks of the waves");

// what the cycles keep per image channel besides CleanState
struct CycleState {
  int32_t* go;              // [nc] 1: the channel runs this cycle
  int32_t* first;           // [nc] the components it held when the cycle started
  int32_t* ncycles;         // [nc] minor cycles run
  double* prev;             // [nc] the peak at the start of the last cycle that ran
  double* limit;            // [nc] L of this cycle
  int32_t* cycle_ncomp;     // [nc][max_major]
  double* cycle_peak;       // [nc][max_major + 1]
};

struct Lattice { double rho[3], kappa[3]; int64_t ny, nx; };

// one thread per image channel, behind k_imclean_init
__global__ void __launch_bounds__(kThreads) k_csclean_init(CycleState X, int nc) {
  const int k = (int)blockIdx.x * kThreads + threadIdx.x;
  if (k >= nc) return;
  X.go[k] = 0;
  X.first[k] = 0;
  X.ncycles[k] = 0;
  X.prev[k] = X.limit[k] = 0.0;
}

// grid-stride over nt * half: dd[t][h] = rot_t (di rho + dj kappa) as (x, y, z, 0), (di, dj) the offset h of the half-plane
__global__ void __launch_bounds__(kThreads) k_csclean_offsets(const ImgFrame* __restrict__ frames, Lattice L, int64_t nt, int64_t half,
                                                              double4* __restrict__ dd) {
  const int64_t w = 2 * L.nx - 1, f0 = (L.ny - 1) * w + (L.nx - 1), total = nt * half;
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kThreads) {
    const int64_t t = e / half, f = f0 + (e - t * half);
    const double di = (double)(f / w - (L.ny - 1)), dj = (double)(f % w - (L.nx - 1));
    const double t0 = di * L.rho[0] + dj * L.kappa[0], t1 = di * L.rho[1] + dj * L.kappa[1], t2 = di * L.rho[2] + dj * L.kappa[2];
    const ImgFrame& fr = frames[t];
    dd[e] = make_double4((fr.rot[0] * t0 + fr.rot[1] * t1) + fr.rot[2] * t2, (fr.rot[3] * t0 + fr.rot[4] * t1) + fr.rot[5] * t2,
                         (fr.rot[6] * t0 + fr.rot[7] * t1) + fr.rot[8] * t2, 0.0);
  }
}

// grid-stride over nc * full: P[k][f] = the half-plane's value at |f - f0|; src [half][stride] with the channel at [k], or, with
// chan_avg, [half] (stride 0)
__global__ void __launch_bounds__(kThreads) k_csclean_mirror(const double* __restrict__ src, int64_t stride, int nc, int64_t full, int64_t f0,
                                                             double* __restrict__ P) {
  const int64_t total = (int64_t)nc * full;
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kThreads) {
    const int64_t k = e / full, f = e - k * full, h = f >= f0 ? f - f0 : f0 - f;
    P[e] = stride ? src[h * stride + k] : src[h];
  }
}

// one workgroup, behind k_imclean_peak1 on the image the entry searches.  cycle: c of the header
__global__ void __launch_bounds__(kThreads) k_csclean_decide(CleanState S, CycleState X, const Peak* __restrict__ partial, int nc, int64_t nslabs,
                                                             int64_t maxiter, double threshold, int relative, double depth, int cycle,
                                                             int max_major) {
  int active = 0;
  for (int k = threadIdx.x; k < nc; k += kThreads) {
    X.go[k] = 0;
    if (S.status[k] != 0) continue;
    const Peak m = best_partial(partial, nc, nslabs, k);
    if (cycle == 0) set_first_peak(S, k, m, threshold, relative);
    X.cycle_peak[(int64_t)k * (max_major + 1) + cycle] = m.p >= 0 ? m.v : __longlong_as_double(0x7ff8000000000000LL);
    const double thr = S.thr[k];
    if (m.p < 0 || !(m.v > thr)) {
      S.status[k] = PRISIM_IMCLEAN_THRESHOLD;
    } else if (S.ncomp[k] >= maxiter) {
      S.status[k] = PRISIM_IMCLEAN_MAXITER;
    } else if (cycle > 0 && m.v > X.prev[k]) {
      S.status[k] = PRISIM_CSCLEAN_DIVERGED;
    } else if (cycle >= max_major) {
      S.status[k] = PRISIM_CSCLEAN_MAJOR;
    } else {
      X.go[k] = 1;
      X.first[k] = S.ncomp[k];
      X.prev[k] = m.v;
      X.limit[k] = fmax(thr, depth * m.v);
      ++active;
    }
  }
  publish_active(S, active);
}

struct MinorParams {
  const double* R;          // [npix][nc] the image the cycle starts from: the exact residual, or the flat-noise image
  const double* P;          // [nc][full]
  const uint8_t* window;    // [npix] or null
  double* scratch;          // [nc][npix] on the GLOBAL route
  CleanState S;
  CycleState X;
  int64_t maxiter, cycle_niter;
  double gain;
  int npix, nc, ny, nx, max_major;
};

// the listed flux of a component of amplitude c = gain img[q] at pixel q of image channel k; c is what the working image loses
struct PlainFlux {                                      // prisim_clean_image_cs: the amplitude itself
  __device__ __forceinline__ double operator()(double c, int32_t, int) const { return c; }
};
struct FlatFlux {                                       // prisim_clean_mosaic_cs: the true flux of a flat amplitude
  const double* s;          // [npix][nc]
  int nc;
  __device__ __forceinline__ double operator()(double c, int32_t q, int k) const { return c * s[(int64_t)q * nc + k]; }
};

// the best of the workgroup under peak_beats, in every thread: shuffles inside a wave, then the waves' partials through sh.  Begins
// with nothing outstanding on sh (the caller's barrier before) and ends behind a barrier; the caller sets one more before it writes
// what a thread may still be reading
__device__ __forceinline__ Peak workgroup_peak(Peak m, Peak* sh) {
#pragma unroll
  for (int off = kWave / 2; off >= 1; off >>= 1) {
    Peak o;
    o.v = __shfl_xor(m.v, off, kWave);
    o.p = __shfl_xor(m.p, off, kWave);
    o.pad_ = 0;
    if (peak_beats(o, m)) m = o;
  }
  if ((threadIdx.x & (kWave - 1)) == 0) sh[threadIdx.x / kWave] = m;
  __syncthreads();
  Peak best = sh[0];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) {
    const Peak o = sh[w];
    if (peak_beats(o, best)) best = o;
  }
  return best;
}

// grid: x = image channel.  LDS: 64 B, and with IN_LDS npix * 8 B of dynamic LDS
template <bool IN_LDS, typename Flux>
__global__ void __launch_bounds__(kThreads) k_csclean_minor(MinorParams M, Flux flux) {
  extern __shared__ double sh_img[];
  __shared__ Peak sh_pk[kWaves];
  const int k = (int)blockIdx.x, tid = threadIdx.x;
  if (!M.X.go[k]) return;                               // uniform: the whole workgroup leaves
  double* img = IN_LDS ? sh_img : M.scratch + (int64_t)k * M.npix;
  const double* Pk = M.P + (int64_t)k * (2 * M.ny - 1) * (2 * M.nx - 1);
  const int pw = 2 * M.nx - 1, si = kThreads / M.nx, sj = kThreads % M.nx;
  const double limit = M.X.limit[k];
  const int32_t first = M.X.first[k];
  int64_t cap = M.maxiter - first;
  if (M.cycle_niter > 0 && M.cycle_niter < cap) cap = M.cycle_niter;

  // the working image is the one handed over; a thread keeps the largest of its own pixels, ascending: the lowest index wins a tie
  Peak m{-1.0, -1, 0};
  for (int p = tid; p < M.npix; p += kThreads) {
    const double r = M.R[(int64_t)p * M.nc + k];
    img[p] = r;
    if (M.window && !M.window[p]) continue;
    const double v = fabs(r);
    if (v > m.v) { m.v = v; m.p = p; }
  }
  int64_t n = 0;
  for (; n < cap; ++n) {
    const Peak best = workgroup_peak(m, sh_pk);         // the barrier inside also covers the writes to img of the pass before
    if (best.p < 0 || !(best.v > limit)) break;         // uniform: every thread holds the same pair
    const double a = M.gain * img[best.p];
    __syncthreads();                                    // img[q] and sh_pk are read before either is written again
    if (tid == 0) {
      M.S.comp_pixel[(int64_t)k * M.maxiter + first + n] = best.p;
      M.S.comp_flux[(int64_t)k * M.maxiter + first + n] = flux(a, best.p, k);
    }
    const int iq = best.p / M.nx, jq = best.p - iq * M.nx;
    int i = tid / M.nx, j = tid - i * M.nx;
    m = Peak{-1.0, -1, 0};
    for (int p = tid; p < M.npix; p += kThreads) {
      const double r = img[p] - a * Pk[(int64_t)(i - iq + M.ny - 1) * pw + (j - jq + M.nx - 1)];
      img[p] = r;
      if (!M.window || M.window[p]) {
        const double v = fabs(r);
        if (v > m.v) { m.v = v; m.p = p; }
      }
      i += si;
      j += sj;
      if (j >= M.nx) { j -= M.nx; ++i; }
    }
  }
  if (tid == 0) {
    const int32_t held = first + (int32_t)n, c = M.X.ncycles[k];
    M.S.ncomp[k] = held;
    M.X.cycle_ncomp[(int64_t)k * M.max_major + c] = held;
    M.X.ncycles[k] = c + 1;
  }
}

struct ModelParams {
  double2* V;               // [nt][nbl][nchan] Vres
  const double* bl;         // [nbl][3]
  const double* freqs;      // [nchan]
  const double4* dd;        // [nt][npix]
  CleanState S;
  CycleState X;
  int64_t nt, nbl, npix, maxiter;
  int nchan, avg;
};

// what the listed flux a of a component at pixel q is worth in snapshot t and channel k
struct NoBeam {                                         // prisim_clean_image_cs: the flux itself
  __device__ __forceinline__ double operator()(double a, int64_t, int32_t, int) const { return a; }
};
struct TableBeam {                                      // prisim_clean_mosaic_cs: through the beam of the snapshot
  const double* A;          // [nt][npix][nchan]
  int64_t npix;
  int nchan;
  __device__ __forceinline__ double operator()(double a, int64_t t, int32_t q, int k) const { return a * A[(t * npix + q) * nchan + k]; }
};

// grid-stride over nt * nbl * nchan, the channel fastest.  Vres[t][b][k] -= sum_j Beam(a_j) (cos phi_j, -sin phi_j) over the new
// components of the channel's image channel, j ascending
template <typename Beam>
__global__ void __launch_bounds__(kThreads) k_csclean_model(ModelParams M, Beam beam) {
  const int64_t total = M.nt * M.nbl * M.nchan;
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kThreads) {
    const int64_t tb = e / M.nchan, t = tb / M.nbl, b = tb - t * M.nbl;
    const int k = (int)(e - tb * M.nchan), kc = M.avg ? 0 : k;
    if (!M.X.go[kc]) continue;
    const int32_t n0 = M.X.first[kc], n1 = M.S.ncomp[kc];
    const double f = M.freqs[k];
    const double b0 = M.bl[b * 3] * kInvC, b1 = M.bl[b * 3 + 1] * kInvC, b2 = M.bl[b * 3 + 2] * kInvC;
    const int32_t* pix = M.S.comp_pixel + (int64_t)kc * M.maxiter;
    const double* flux = M.S.comp_flux + (int64_t)kc * M.maxiter;
    const double4* ddt = M.dd + t * M.npix;
    double sx = 0.0, sy = 0.0;
    for (int32_t j = n0; j < n1; ++j) {
      const int32_t q = pix[j];
      double c, s;
      point_phasor(b0, b1, b2, ddt[q], f, c, s);
      const double a = beam(flux[j], t, q, k);
      sx += a * c;
      sy += -(a * s);
    }
    double2 x = M.V[e];
    x.x -= sx;
    x.y -= sy;
    M.V[e] = x;
  }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------

// lattice steps of the directions' own frame: each 0 where its axis has one pixel
inline Lattice lattice_of(const double* u, int64_t ny, int64_t nx) {
  Lattice L{};
  L.ny = ny;
  L.nx = nx;
  for (int i = 0; i < 3; ++i) {
    L.rho[i] = ny > 1 ? (u[((ny - 1) * nx + nx / 2) * 3 + i] - u[(nx / 2) * 3 + i]) / (double)(ny - 1) : 0.0;
    L.kappa[i] = nx > 1 ? (u[((ny / 2) * nx + nx - 1) * 3 + i] - u[((ny / 2) * nx) * 3 + i]) / (double)(nx - 1) : 0.0;
  }
  return L;
}

// the state of the cycles of nc image channels, on the device
inline int alloc_cycle_state(prisim_ctx* ctx, Dev& dev, CycleState& X, int64_t nc, int64_t max_major) {
  DEV_ALLOC(ctx, dev, X.go, nc * 4);
  DEV_ALLOC(ctx, dev, X.first, nc * 4);
  DEV_ALLOC(ctx, dev, X.ncycles, nc * 4);
  DEV_ALLOC(ctx, dev, X.prev, nc * 8);
  DEV_ALLOC(ctx, dev, X.limit, nc * 8);
  DEV_ALLOC(ctx, dev, X.cycle_ncomp, nc * max_major * 4);
  DEV_ALLOC(ctx, dev, X.cycle_peak, nc * (max_major + 1) * 8);
  return PRISIM_OK;
}

// The minor-cycle beam of a call: P [nc][full] and the buffers of its half-plane, by the plan's psf_half and psf_full.  Behind the
// weight sums of the PSF job of the call's view (enqueue_weight_sums): offsets(), then the entry's own call of the PSF pass of the
// dirty image over the half-plane -- enqueue_dirty_sums of that job on (half, pdd, prow, pavg) --, then mirror().
struct CycleBeam {
  double4* pdd = nullptr;
  double *P = nullptr, *prow = nullptr, *pavg = nullptr;
  int alloc(CleanCall& c, int64_t psf_bytes, int64_t half) {
    DEV_ALLOC(c.ctx, c.wk.dev, P, psf_bytes);
    DEV_ALLOC(c.ctx, c.wk.dev, pdd, c.v.nt * half * 32);
    DEV_ALLOC(c.ctx, c.wk.dev, prow, half * c.nchan * 8);
    if (c.avg) DEV_ALLOC(c.ctx, c.wk.dev, pavg, half * 8);
    return PRISIM_OK;
  }
  int offsets(const CleanCall& c, const Lattice& lat, int64_t half) const {
    const int64_t nt = c.v.nt;
    return launch(c.ctx, k_csclean_offsets, dim3((unsigned)grid_for(c.ctx, nt * half)), 0, c.s0, c.T.frames, lat, nt, half, pdd);
  }
  int mirror(const CleanCall& c, int64_t half, int64_t full) const {
    return launch(c.ctx, k_csclean_mirror, dim3((unsigned)grid_for(c.ctx, c.nc * full)), 0, c.s0, (const double*)(c.avg ? pavg : prow),
                  c.avg ? (int64_t)0 : c.nchan, (int)c.nc, full, full - half, P);
  }
};

// the minor cycles of the channels that go on, by the route of the plan
template <typename Flux>
inline int enqueue_minor(const CleanCall& c, const MinorParams& MP, const Flux& flux, bool in_lds) {
  return in_lds ? launch(c.ctx, k_csclean_minor<true, Flux>, dim3((unsigned)c.nc), (size_t)(c.npix * 8), c.s0, MP, flux)
                : launch(c.ctx, k_csclean_minor<false, Flux>, dim3((unsigned)c.nc), 0, c.s0, MP, flux);
}

// of the cycle tables on the host, the columns that any channel filled, and the copy into the caller's rows
struct CycleTables {
  std::vector<int32_t> ncycles, ncomp;
  std::vector<double> peak;
  int64_t cycles = 0, max_major = 0;
  int enqueue(const CleanCall& c, const CycleState& X, int64_t cycles_, int64_t max_major_) {
    prisim_ctx* ctx = c.ctx;
    cycles = cycles_; max_major = max_major_;
    const int64_t nc = c.nc;
    ncycles.resize((size_t)nc);
    ncomp.resize((size_t)(nc * cycles));
    peak.resize((size_t)(nc * (cycles + 1)));
    HIPCHK(ctx, hipMemcpyAsync(ncycles.data(), X.ncycles, (size_t)nc * 4, hipMemcpyDeviceToHost, c.s0));
    if (cycles > 0)
      HIPCHK(ctx, copy_rows(ncomp.data(), (size_t)cycles * 4, X.cycle_ncomp, (size_t)max_major * 4, (size_t)cycles * 4, (size_t)nc,
                            hipMemcpyDeviceToHost, c.s0));
    HIPCHK(ctx, copy_rows(peak.data(), (size_t)(cycles + 1) * 8, X.cycle_peak, (size_t)(max_major + 1) * 8, (size_t)(cycles + 1) * 8, (size_t)nc,
                          hipMemcpyDeviceToHost, c.s0));
    return PRISIM_OK;
  }
  // behind the drained stream
  int check(prisim_ctx* ctx) const {
    for (int32_t n : ncycles)
      if (n < 0 || n > cycles) return fail(ctx, PRISIM_EINTERNAL, "a cycle count beyond the cycles run");
    return PRISIM_OK;
  }
  void write(const CleanLists& lists, int32_t* out_ncycles, int32_t* out_cycle_ncomp, double* out_cycle_peak) const {
    const int64_t nc = (int64_t)ncycles.size();
    std::memcpy(out_ncycles, ncycles.data(), (size_t)nc * 4);
    for (int64_t k = 0; k < nc; ++k) {
      const size_t n = (size_t)ncycles[(size_t)k];
      if (n) std::memcpy(out_cycle_ncomp + k * max_major, ncomp.data() + k * cycles, n * 4);
      if (lists.status[(size_t)k] != PRISIM_IMCLEAN_DEAD) std::memcpy(out_cycle_peak + k * (max_major + 1), peak.data() + k * (cycles + 1), (n + 1) * 8);
    }
  }
};

}  // namespace

#endif  // PRISIM_CYCLE_KERNELS_H
