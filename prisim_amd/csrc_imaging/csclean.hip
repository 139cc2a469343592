// csclean.hip -- Cotton-Schwab CLEAN of a dirty image for gfx950 (include/prisim_csclean.h): minor cycles on one image channel with a
// shift-invariant beam P, major cycles through the residual visibilities Vres with the exact one.  The dirty images -- the first, and
// one per major cycle -- and P are what prisim_dirty_image enqueues (dirty_image.h): enqueue_dirty on Vres, and enqueue_dirty_sums of
// kind PSF over the offsets rot_t (di rho + dj kappa) of the half-plane.  What is new here:
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
//                     tid, tid + 256, ...; per component it subtracts a P[i_p - i_q][j_p - j_q] from each -- P of the channel is read
//                     from device memory, where it is L2-sized -- and keeps the largest |value| of what it wrote; the (|value|, index)
//                     pairs are reduced under "larger, then lower index" across the lanes of a wave by shuffles and across the four
//                     waves through LDS: two barriers per component.
//   k_csclean_model   Vres -= the cycle's new components: one thread per (t, b, k), components in list order, every phasor from the
//                     channel's true frequency (cycles_phasor).  Channels that did not run a cycle are not touched.
// The frame of the call (CleanCall), the peak search before a cycle, the state of the channels, the lists and the restoration are those
// of clean_kernels.h, and so are the buffers of the dirty-image residual (DirtyResidual), as prisim_clean_image (imclean.hip) has them.
// No atomics, no floating-point reduction whose order depends on the launch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

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

// one workgroup, behind k_imclean_peak1 on the exact residual.  cycle: c of the header
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
  const double* R;          // [npix][nc] the exact residual
  const double* P;          // [nc][full]
  const uint8_t* window;    // [npix] or null
  double* scratch;          // [nc][npix] on the GLOBAL route
  CleanState S;
  CycleState X;
  int64_t maxiter, cycle_niter;
  double gain;
  int npix, nc, ny, nx, max_major;
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
template <bool IN_LDS>
__global__ void __launch_bounds__(kThreads) k_csclean_minor(MinorParams M) {
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

  // the working image is the exact residual; a thread keeps the largest of its own pixels, ascending: the lowest index wins a tie
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
      M.S.comp_flux[(int64_t)k * M.maxiter + first + n] = a;
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

// grid-stride over nt * nbl * nchan, the channel fastest.  Vres[t][b][k] -= sum_j a_j (cos phi_j, -sin phi_j) over the new components
// of the channel's image channel, j ascending
__global__ void __launch_bounds__(kThreads) k_csclean_model(ModelParams M) {
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
      const double4 dq = ddt[pix[j]];
      const double tau = (b0 * dq.x + b1 * dq.y) + b2 * dq.z;
      double c, s;
      cycles_phasor(f * tau, c, s);
      const double a = flux[j];
      sx += a * c;
      sy += -(a * s);
    }
    double2 x = M.V[e];
    x.x -= sx;
    x.y -= sy;
    M.V[e] = x;
  }
}

// lattice steps of the directions' own frame: each 0 where its axis has one pixel
Lattice lattice_of(const double* u, int64_t ny, int64_t nx) {
  Lattice L{};
  L.ny = ny;
  L.nx = nx;
  for (int i = 0; i < 3; ++i) {
    L.rho[i] = ny > 1 ? (u[((ny - 1) * nx + nx / 2) * 3 + i] - u[(nx / 2) * 3 + i]) / (double)(ny - 1) : 0.0;
    L.kappa[i] = nx > 1 ? (u[((ny / 2) * nx + nx - 1) * 3 + i] - u[((ny / 2) * nx) * 3 + i]) / (double)(nx - 1) : 0.0;
  }
  return L;
}

int clean_image_cs(prisim_ctx* ctx, const prisim_csclean_args* a, double* out_residual, double* out_restored, int32_t* out_comp_pixel,
                   double* out_comp_flux, int32_t* out_ncomp, int32_t* out_status, double* out_peak0, double* out_wsum, int32_t* out_ncycles,
                   int32_t* out_cycle_ncomp, double* out_cycle_peak, double* out_psf, double* out_vres, prisim_csclean_stats* stats) {
  if (!ctx) return PRISIM_EINVAL;
  // the entry's own host buffers: declared before the frame, whose stream drains before they go.  The results wait in them until the
  // call is through, as the frame's do
  std::vector<double> h_psf, h_cyc_peak;
  std::vector<int32_t> h_ncycles, h_cyc_ncomp;
  DirtyResidual dr;
  CleanCall call(ctx, {out_residual, out_restored, out_comp_pixel, out_comp_flux, out_ncomp, out_status, out_peak0}, stats != nullptr);
  if (int rc = call.check_outputs(a)) return rc;
  if (!out_ncycles || !out_cycle_ncomp || !out_cycle_peak) return fail(ctx, PRISIM_EINVAL, "out_ncycles, out_cycle_ncomp or out_cycle_peak is NULL");
  if (int rc = call.check_inputs(*a)) return rc;
  const ImgView& v = call.v;
  const int64_t npix = a->npix, nbl = a->nbl, nchan = a->nchan, nt = a->nt, maxiter = a->maxiter, ny = a->ny, nx = a->nx, nc = call.nc;
  const bool avg = call.avg, restore = call.restore, timed = call.timed;
  const CscleanPlan cp = csclean_plan(npix, ny, nx, nbl, nchan, nt, avg, maxiter, a->cycle_depth, a->max_major, a->budget_bytes, call.su.lds_max,
                                      a->route, call.su.uniform, a->minor_route);
  const ImcleanPlan& pl = cp.base;
  if (cp.refusal) return fail(ctx, PRISIM_EINVAL, clean_refusal(cp.refusal, cp.total, "the workgroup of a minor cycle", cp.minor_lds));
  const int max_major = a->max_major;
  const bool in_lds = cp.minor_route == kCscleanLds;
  const int64_t half = cp.psf_half, full = cp.psf_full, ncube = nt * nbl * nchan;
  const Lattice lat = lattice_of(a->unitvec, ny, nx);

  h_psf.resize(out_psf ? (size_t)(nc * full) : 0);
  h_ncycles.resize((size_t)nc);
  if (int rc = call.open(pl)) return rc;
  hipStream_t s0 = call.s0;
  Dev& dev = call.wk.dev;
  ImgTables& T = call.T;
  const CleanState& S = call.S;
  BatchEvents be;
  if (timed)
    if (int rc = be.create(ctx, 12)) return rc;
  auto mark = [&](int i) -> int {
    if (timed) HIPCHK(ctx, hipEventRecord(be.ev[(size_t)i], s0));
    return PRISIM_OK;
  };
  auto span_ms = [&](int i, int j) { return timed ? elapsed_ms(be.ev[(size_t)i], be.ev[(size_t)j]) : 0.0; };

  // the resident buffers of the plan
  if (int rc = dr.alloc(call)) return rc;
  double4* d_pdd = nullptr;
  double *d_P = nullptr, *d_prow = nullptr, *d_pavg = nullptr, *d_minor = nullptr;
  double2* d_vres = nullptr;
  CycleState X{};
  DEV_ALLOC(ctx, dev, X.go, nc * 4);
  DEV_ALLOC(ctx, dev, X.first, nc * 4);
  DEV_ALLOC(ctx, dev, X.ncycles, nc * 4);
  DEV_ALLOC(ctx, dev, X.prev, nc * 8);
  DEV_ALLOC(ctx, dev, X.limit, nc * 8);
  DEV_ALLOC(ctx, dev, X.cycle_ncomp, nc * max_major * 4);
  DEV_ALLOC(ctx, dev, X.cycle_peak, nc * (max_major + 1) * 8);
  DEV_ALLOC(ctx, dev, d_P, cp.psf_bytes);
  DEV_ALLOC(ctx, dev, d_pdd, nt * half * 32);
  DEV_ALLOC(ctx, dev, d_prow, half * nchan * 8);
  if (avg) DEV_ALLOC(ctx, dev, d_pavg, half * 8);
  if (!in_lds) DEV_ALLOC(ctx, dev, d_minor, cp.minor_bytes);

  // Vres: the uploaded cube is the call's own; the resident one is copied, behind what the context's stream wrote into it (open)
  if (v.resident()) {
    DEV_ALLOC(ctx, dev, d_vres, cp.vres_bytes);
    HIPCHK(ctx, hipMemcpyAsync(d_vres, ctx->cube.p, (size_t)ncube * 16, hipMemcpyDeviceToDevice, s0));
    T.cube = d_vres;
  } else {
    d_vres = const_cast<double2*>(T.cube);
  }
  if (in_lds)
    if (int rc = allow_lds(ctx, k_csclean_minor<true>, npix * 8)) return rc;

  // ---- the weight sums, P, the first dirty image.  Events: [0] sums [1] P [2] dirty image [3]
  const DirtyImage job = dirty_image_of(v, T, call.su.df, pl, dr.wsum, dr.wtot);
  ImgView vp = v;
  vp.kind = PRISIM_IMAGE_PSF;
  const DirtyImage beam = dirty_image_of(vp, T, call.su.df, pl, dr.wsum, dr.wtot);
  if (int rc = mark(0)) return rc;
  if (int rc = enqueue_weight_sums(ctx, job, s0)) return rc;
  if (int rc = mark(1)) return rc;
  if (int rc = launch(ctx, k_csclean_offsets, dim3((unsigned)grid_for(ctx, nt * half)), 0, s0, T.frames, lat, nt, half, d_pdd)) return rc;
  if (int rc = enqueue_dirty_sums(ctx, beam, half, d_pdd, d_prow, d_pavg, s0)) return rc;
  if (int rc = launch(ctx, k_csclean_mirror, dim3((unsigned)grid_for(ctx, nc * full)), 0, s0, (const double*)(avg ? d_pavg : d_prow),
                      avg ? (int64_t)0 : nchan, (int)nc, full, full - half, d_P))
    return rc;
  if (int rc = mark(2)) return rc;
  if (int rc = enqueue_dirty(ctx, job, Span{0, npix}, dr.dd, dr.rows(), dr.R, s0)) return rc;
  if (int rc = call.init(dr.norm())) return rc;
  if (int rc = launch(ctx, k_csclean_init, dim3((unsigned)((nc + kThreads - 1) / kThreads)), 0, s0, X, (int)nc)) return rc;
  if (int rc = mark(3)) return rc;

  // ---- the cycles: max_major + 1 starts at most, whatever the device says.  Events of a cycle: [4] search and decision [5], then
  // behind the host's read [6] minor [7] model [8] dirty image [9]
  MinorParams MP{};
  MP.R = dr.R; MP.P = d_P; MP.window = call.d_window; MP.scratch = d_minor;
  MP.S = S; MP.X = X;
  MP.maxiter = maxiter; MP.cycle_niter = a->cycle_niter; MP.gain = a->gain;
  MP.npix = (int)npix; MP.nc = (int)nc; MP.ny = (int)ny; MP.nx = (int)nx; MP.max_major = max_major;
  ModelParams MM{};
  MM.V = d_vres; MM.bl = T.bl; MM.freqs = T.freqs; MM.dd = dr.dd;
  MM.S = S; MM.X = X;
  MM.nt = nt; MM.nbl = nbl; MM.npix = npix; MM.maxiter = maxiter;
  MM.nchan = (int)nchan; MM.avg = avg ? 1 : 0;
  double dirty_ms = 0.0, peak_ms = 0.0, minor_ms = 0.0, model_ms = 0.0;
  int64_t active[2] = {0, 0}, polls = 0, cycles = 0;   // what a poll reads: the channels that go on, the cycles in which any did
  for (int c = 0; c <= max_major; ++c) {
    if (int rc = mark(4)) return rc;
    if (int rc = call.search(dr.R)) return rc;
    if (int rc = launch(ctx, k_csclean_decide, dim3(1), 0, s0, S, X, (const Peak*)call.d_partial, (int)nc, pl.nslabs, maxiter, a->threshold,
                        (int)a->threshold_relative, a->cycle_depth, c, max_major))
      return rc;
    if (int rc = mark(5)) return rc;
    HIPCHK(ctx, hipMemcpyAsync(active, S.counts, 16, hipMemcpyDeviceToHost, s0));
    HIPCHK(ctx, hipStreamSynchronize(s0));
    ++polls;
    peak_ms += span_ms(4, 5);
    if (c > 0) {
      minor_ms += span_ms(6, 7);
      model_ms += span_ms(7, 8);
      dirty_ms += span_ms(8, 9);
    }
    if (active[0] <= 0) break;
    if (c == max_major) return fail(ctx, PRISIM_EINTERNAL, "channels still active after max_major cycles");
    ++cycles;
    if (int rc = mark(6)) return rc;
    if (int rc = in_lds ? launch(ctx, k_csclean_minor<true>, dim3((unsigned)nc), (size_t)(npix * 8), s0, MP)
                        : launch(ctx, k_csclean_minor<false>, dim3((unsigned)nc), 0, s0, MP))
      return rc;
    if (int rc = mark(7)) return rc;
    if (int rc = launch(ctx, k_csclean_model, dim3((unsigned)grid_for(ctx, ncube)), 0, s0, MM)) return rc;
    if (int rc = mark(8)) return rc;
    if (int rc = enqueue_dirty(ctx, job, Span{0, npix}, dr.dd, dr.rows(), dr.R, s0)) return rc;
    if (int rc = mark(9)) return rc;
  }

  // ---- the results
  if (int rc = dr.download_norm(call)) return rc;
  HIPCHK(ctx, hipMemcpyAsync(h_ncycles.data(), X.ncycles, (size_t)nc * 4, hipMemcpyDeviceToHost, s0));
  // of the cycle tables, the columns that any channel filled
  h_cyc_ncomp.resize((size_t)(nc * cycles));
  h_cyc_peak.resize((size_t)(nc * (cycles + 1)));
  if (cycles > 0)
    HIPCHK(ctx, copy_rows(h_cyc_ncomp.data(), (size_t)cycles * 4, X.cycle_ncomp, (size_t)max_major * 4, (size_t)cycles * 4, (size_t)nc,
                          hipMemcpyDeviceToHost, s0));
  HIPCHK(ctx, copy_rows(h_cyc_peak.data(), (size_t)(cycles + 1) * 8, X.cycle_peak, (size_t)(max_major + 1) * 8, (size_t)(cycles + 1) * 8, (size_t)nc,
                        hipMemcpyDeviceToHost, s0));
  if (out_psf) HIPCHK(ctx, hipMemcpyAsync(h_psf.data(), d_P, h_psf.size() * 8, hipMemcpyDeviceToHost, s0));
  if (int rc = call.close(dr.R, timed ? be.ev[10] : nullptr, timed ? be.ev[11] : nullptr)) return rc;
  if (int rc = call.gather()) return rc;
  const CleanLists& lists = call.lists;
  for (int64_t k = 0; k < nc; ++k)
    if (h_ncycles[(size_t)k] < 0 || h_ncycles[(size_t)k] > cycles) return fail(ctx, PRISIM_EINTERNAL, "a cycle count beyond the cycles run");
  // the residual visibilities go straight to the caller, as the last thing that can fail
  if (out_vres) {
    HIPCHK(ctx, hipMemcpyAsync(out_vres, d_vres, (size_t)ncube * 16, hipMemcpyDeviceToHost, s0));
    HIPCHK(ctx, hipStreamSynchronize(s0));
  }

  call.write();
  dr.write_norm(out_wsum);
  std::memcpy(out_ncycles, h_ncycles.data(), (size_t)nc * 4);
  for (int64_t k = 0; k < nc; ++k) {
    const size_t n = (size_t)h_ncycles[(size_t)k];
    if (n) std::memcpy(out_cycle_ncomp + k * max_major, h_cyc_ncomp.data() + k * cycles, n * 4);
    if (lists.status[(size_t)k] != PRISIM_IMCLEAN_DEAD) std::memcpy(out_cycle_peak + k * (max_major + 1), h_cyc_peak.data() + k * (cycles + 1), (n + 1) * 8);
  }
  if (out_psf) std::memcpy(out_psf, h_psf.data(), h_psf.size() * 8);
  if (stats) {
    const double psf_ms = span_ms(1, 2), restore_ms = restore ? span_ms(10, 11) : 0.0;
    dirty_ms += span_ms(0, 1) + span_ms(2, 3);
    call.common_stats(stats, cp.total);
    stats->kernel_ms = psf_ms + dirty_ms + peak_ms + minor_ms + model_ms + restore_ms;
    stats->psf_ms = psf_ms;
    stats->dirty_ms = dirty_ms;
    stats->peak_ms = peak_ms;
    stats->minor_ms = minor_ms;
    stats->model_ms = model_ms;
    stats->restore_ms = restore_ms;
    stats->cycles = cycles;
    stats->polls = polls;
    stats->psf_offsets = half;
    stats->download_bytes = npix * nc * 8 * (restore ? 2 : 1) + nc * 36 + nc * lists.longest * 12 + nc * (2 * cycles + 1) * 12 + polls * 16 +
                            (out_psf ? nc * full * 8 : 0) + (out_vres ? ncube * 16 : 0);
    stats->minor_route = cp.minor_route;
    stats->minor_lds_bytes = (int32_t)cp.minor_lds;
  }
  return PRISIM_OK;
}

}  // namespace

extern "C" {

int prisim_clean_image_cs(prisim_ctx* ctx, const prisim_csclean_args* a, double* out_residual, double* out_restored, int32_t* out_comp_pixel,
                          double* out_comp_flux, int32_t* out_ncomp, int32_t* out_status, double* out_peak0, double* out_wsum,
                          int32_t* out_ncycles, int32_t* out_cycle_ncomp, double* out_cycle_peak, double* out_psf, double* out_vres,
                          prisim_csclean_stats* stats) {
  return guarded(ctx, [&]() -> int {
    return clean_image_cs(ctx, a, out_residual, out_restored, out_comp_pixel, out_comp_flux, out_ncomp, out_status, out_peak0, out_wsum, out_ncycles,
                          out_cycle_ncomp, out_cycle_peak, out_psf, out_vres, stats);
  });
}

}  // extern "C"
