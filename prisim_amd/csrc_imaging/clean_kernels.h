// clean_kernels.h -- the bookkeeping of an image-space CLEAN, as prisim_clean_image (imclean.hip), prisim_clean_mosaic (mosclean.hip)
// and prisim_clean_image_cs (csclean.hip) share it: the peak search in two steps, the state of the channels with the component lists,
// the restoration, and on the host the frame of a call (CleanCall: the checks, the set-up, the launches on the state, the way down
// of the results), the loop that enqueues the iterations in batches and polls the active count, the gathering of the lists and the
// buffers of a residual that is a dirty image.  What differs between the entries -- the plan, the image the search runs on, where a
// component's flux comes from, the loop body and the extra outputs -- stays in their files; the update that the first two share is
// in clean_update.h.
//   k_imclean_peak1   reads the searched image channel-fastest.  A workgroup is cx channels by 256 / cx pixel lanes and owns a slab of
//                     pixels; a lane keeps the largest |value| of its pixels (by >, ascending pixels, so the lowest index wins a tie and
//                     a NaN never wins), the lanes are reduced in LDS under the associative rule "larger |value|, then lower index", and
//                     the partial (|value|, index) of (slab, channel) is written.  Channels that have ended are not read.
//   k_imclean_peak2   one workgroup, a thread per image channel: reduces the partials, applies the stop rule, appends the component and
//                     publishes (q_k, a_k) -- a_k = 0 once the channel has ended -- and the count of active channels.  The flux of the
//                     component is gain * flux(q, k), flux being the entry's own statement (a functor).  Its reduction, its
//                     first-iteration rule and its count are functions that k_csclean_decide calls too.
//   k_imclean_restore adds the components through a Gaussian beam, one thread per (pixel, channel), components in list order.
// No atomics, no floating-point reduction whose order depends on the launch.  Every including file gets its own copy (an unnamed
// namespace); built with -ffp-contract=off.  Not part of the public ABI.
#ifndef PRISIM_CLEAN_KERNELS_H
#define PRISIM_CLEAN_KERNELS_H

#include <algorithm>
#include <cstring>

#include "../../include/prisim_imclean.h"
#include "../csrc_addon/imclean_plan.h"
#include "imaging_kernels.h"

namespace {

static_assert(kImcleanPollDefault == PRISIM_IMCLEAN_POLL_DEFAULT && kImcleanPollMax == PRISIM_IMCLEAN_POLL_MAX, "the plan and the header agree");

struct Peak { double v; int32_t p, pad_; };             // |value| and pixel; (-1, -1): none

// larger |value|, then lower index: associative, so any tree gives the same answer
__device__ __forceinline__ bool peak_beats(const Peak& o, const Peak& m) { return o.v > m.v || (o.v == m.v && o.p < m.p); }

struct CleanState {
  int32_t* q;               // [nc] the pick of this iteration
  double* a;                // [nc] its flux; 0: the channel has ended
  double* thr;              // [nc]
  double* peak0;            // [nc]
  int32_t* ncomp;           // [nc]
  int32_t* status;          // [nc] 0: active
  int64_t* counts;          // [0] channels active in the last iteration, [1] iterations in which any was
  int32_t* comp_pixel;      // [nc][maxiter]
  double* comp_flux;        // [nc][maxiter]
};

// one thread per image channel.  wk: W[k], or their sum with chan_avg
__global__ void __launch_bounds__(kThreads) k_imclean_init(CleanState S, const double* __restrict__ wk, int nc) {
  const int k = (int)blockIdx.x * kThreads + threadIdx.x;
  if (k == 0) S.counts[0] = S.counts[1] = 0;
  if (k >= nc) return;
  const bool dead = wk[k] == 0.0;
  S.q[k] = 0;
  S.a[k] = 0.0;
  S.ncomp[k] = 0;
  S.status[k] = dead ? PRISIM_IMCLEAN_DEAD : 0;
  S.thr[k] = S.peak0[k] = __longlong_as_double(0x7ff8000000000000LL);   // set in the first iteration; a dead channel keeps NaN
}

// grid: x = slab of pixels, y = group of cx channels.  partial [nslabs][nc]
__global__ void __launch_bounds__(kThreads) k_imclean_peak1(const double* __restrict__ R, const uint8_t* __restrict__ window,
                                                            const int32_t* __restrict__ status, int64_t npix, int nc, int64_t slab, int cx,
                                                            Peak* __restrict__ partial) {
  __shared__ Peak sh[kThreads];
  const int tid = threadIdx.x, c = tid % cx, lane = tid / cx, lanes = kThreads / cx;
  const int k = (int)blockIdx.y * cx + c;
  const int64_t first = (int64_t)blockIdx.x * slab, end = first + slab < npix ? first + slab : npix;
  Peak m{-1.0, -1, 0};
  if (k < nc && status[k] == 0)
    for (int64_t p = first + lane; p < end; p += lanes) {
      if (window && !window[p]) continue;
      const double v = fabs(R[p * nc + k]);
      if (v > m.v) { m.v = v; m.p = (int32_t)p; }
    }
  sh[tid] = m;
  __syncthreads();
  for (int h = lanes / 2; h >= 1; h >>= 1) {
    if (lane < h) {
      const Peak o = sh[(lane + h) * cx + c];
      if (peak_beats(o, m)) { m = o; sh[tid] = m; }
    }
    __syncthreads();
  }
  if (lane == 0 && k < nc) partial[(int64_t)blockIdx.x * nc + k] = m;
}

// the flux of prisim_clean_image: the residual at the pick
struct ResidualFlux {
  const double* R;          // [npix][nc]
  int nc;
  __device__ __forceinline__ double operator()(int32_t p, int k) const { return R[(int64_t)p * nc + k]; }
};

// ---- what the decision kernels of the entries share (k_imclean_peak2 here, k_csclean_decide of csclean.hip) ----

// the best of channel k's slab partials
__device__ __forceinline__ Peak best_partial(const Peak* __restrict__ partial, int nc, int64_t nslabs, int k) {
  Peak m{-1.0, -1, 0};
  for (int64_t s = 0; s < nslabs; ++s) {
    const Peak o = partial[s * nc + k];
    if (peak_beats(o, m)) m = o;
  }
  return m;
}

// the first search of a call sets P0 of channel k, where it has a peak at all, and its threshold
__device__ __forceinline__ void set_first_peak(const CleanState& S, int k, const Peak& m, double threshold, int relative) {
  if (m.p >= 0) S.peak0[k] = m.v;
  S.thr[k] = relative ? threshold * m.v : threshold;
}

// one workgroup, every thread with the number of its channels that go on: publishes their sum and counts the iteration if any does
__device__ __forceinline__ void publish_active(const CleanState& S, int active) {
  __shared__ int sh_n[kThreads];
  sh_n[threadIdx.x] = active;
  __syncthreads();
  for (int h = kThreads / 2; h >= 1; h >>= 1) {
    if ((int)threadIdx.x < h) sh_n[threadIdx.x] += sh_n[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    S.counts[0] = sh_n[0];
    if (sh_n[0] > 0) S.counts[1] += 1;
  }
}

// one workgroup.  first: this is the first iteration, which sets P0 and the threshold.  flux(q, k): what gain multiplies
template <typename Flux>
__global__ void __launch_bounds__(kThreads) k_imclean_peak2(CleanState S, const Peak* __restrict__ partial, Flux flux, int nc, int64_t nslabs,
                                                            int64_t maxiter, double gain, double threshold, int relative, int first) {
  int active = 0;
  for (int k = threadIdx.x; k < nc; k += kThreads) {
    if (S.status[k] != 0) { S.a[k] = 0.0; continue; }
    const Peak m = best_partial(partial, nc, nslabs, k);
    if (first) set_first_peak(S, k, m, threshold, relative);
    double ak = 0.0;
    if (m.p < 0 || !(m.v > S.thr[k])) {
      S.status[k] = PRISIM_IMCLEAN_THRESHOLD;
    } else if (S.ncomp[k] >= maxiter) {
      S.status[k] = PRISIM_IMCLEAN_MAXITER;
    } else {
      const int32_t n = S.ncomp[k];
      ak = gain * flux(m.p, k);
      S.comp_pixel[(int64_t)k * maxiter + n] = m.p;
      S.comp_flux[(int64_t)k * maxiter + n] = ak;
      S.ncomp[k] = n + 1;
      S.q[k] = m.p;
      ++active;
    }
    S.a[k] = ak;
  }
  publish_active(S, active);
}

// grid-stride over npix * nc, in place: R[p][k] += sum of the components (q, a) of k, in list order, of a exp(-4 ln 2 theta^2 / fwhm_k^2)
__global__ void __launch_bounds__(kThreads) k_imclean_restore(double* __restrict__ R, const double* __restrict__ uvec, CleanState S,
                                                              const double* __restrict__ fwhm, int64_t npix, int nc, int64_t maxiter) {
  const int64_t total = npix * nc;
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kThreads) {
    const int64_t p = e / nc;
    const int k = (int)(e - p * nc);
    const double ux = uvec[p * 3], uy = uvec[p * 3 + 1], uz = uvec[p * 3 + 2];
    const double scale = -4.0 * 0.6931471805599453 / (fwhm[k] * fwhm[k]);
    const int32_t n = S.ncomp[k];
    double m = 0.0;
    for (int32_t i = 0; i < n; ++i) {
      const int64_t q = S.comp_pixel[(int64_t)k * maxiter + i];
      const double dx = ux - uvec[q * 3], dy = uy - uvec[q * 3 + 1], dz = uz - uvec[q * 3 + 2];
      const double theta = 2.0 * asin(fmin(1.0, 0.5 * sqrt((dx * dx + dy * dy) + dz * dz)));
      m += S.comp_flux[(int64_t)k * maxiter + i] * exp(scale * (theta * theta));
    }
    R[e] = R[e] + m;
  }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------

// the checks of the CLEAN arguments the two entries take alike, behind check_args of the shared fields; nc: image channels
template <typename Args>
inline int check_clean_args(prisim_ctx* ctx, const Args& a, int64_t nc, bool restore) {
  if (!(a.gain > 0.0 && a.gain <= 1.0)) return fail(ctx, PRISIM_EINVAL, "gain must lie in (0, 1]");
  if (!(a.threshold >= 0.0) || !std::isfinite(a.threshold)) return fail(ctx, PRISIM_EINVAL, "threshold must be finite and non-negative");
  if (a.threshold_relative != 0 && a.threshold_relative != 1) return fail(ctx, PRISIM_EINVAL, "threshold_relative must be 0 or 1");
  if (a.threshold_relative && !(a.threshold < 1.0)) return fail(ctx, PRISIM_EINVAL, "a relative threshold must be below 1");
  if (a.window && std::all_of(a.window, a.window + a.npix, [](uint8_t x) { return x == 0; }))
    return fail(ctx, PRISIM_EINVAL, "the window holds no pixel");
  if (restore && !a.fwhm_rad) return fail(ctx, PRISIM_EINVAL, "out_restored needs fwhm_rad");
  for (int64_t k = 0; restore && k < nc; ++k)
    if (!(a.fwhm_rad[k] > 0.0) || !std::isfinite(a.fwhm_rad[k]))
      return fail(ctx, PRISIM_EINVAL, "fwhm_rad[" + std::to_string(k) + "] is not positive and finite");
  return PRISIM_OK;
}

// the state of nc image channels with lists of maxiter entries, on the device
inline int alloc_clean_state(prisim_ctx* ctx, Dev& dev, CleanState& S, int64_t nc, int64_t maxiter) {
  DEV_ALLOC(ctx, dev, S.q, nc * 4);
  DEV_ALLOC(ctx, dev, S.a, nc * 8);
  DEV_ALLOC(ctx, dev, S.thr, nc * 8);
  DEV_ALLOC(ctx, dev, S.peak0, nc * 8);
  DEV_ALLOC(ctx, dev, S.ncomp, nc * 4);
  DEV_ALLOC(ctx, dev, S.status, nc * 4);
  DEV_ALLOC(ctx, dev, S.counts, 16);
  DEV_ALLOC(ctx, dev, S.comp_pixel, nc * maxiter * 4);
  DEV_ALLOC(ctx, dev, S.comp_flux, nc * maxiter * 8);
  return PRISIM_OK;
}

// the events of one batch: ev[0] before it, ev[2 i + 1] behind the peak search and ev[2 i + 2] behind the update of its iteration i
struct BatchEvents {
  std::vector<hipEvent_t> ev;
  ~BatchEvents() { for (hipEvent_t x : ev) if (x) (void)hipEventDestroy(x); }
  int create(prisim_ctx* ctx, int count) {
    ev.assign((size_t)count, nullptr);
    for (hipEvent_t& x : ev) HIPCHK(ctx, hipEventCreate(&x));
    return PRISIM_OK;
  }
};

inline double elapsed_ms(hipEvent_t e0, hipEvent_t e1) {
  float ms = 0.f;
  return hipEventElapsedTime(&ms, e0, e1) == hipSuccess ? (double)ms : 0.0;
}

// The state of the channels on the host: counts, statuses, first peaks and, of the lists, the columns that any channel filled.
// enqueue() behind the last iteration, lists() once s0 is idle, write() when the call can no longer fail.
struct CleanLists {
  std::vector<int32_t> ncomp, status, pix;
  std::vector<double> peak0, flux;
  int64_t nc = 0, maxiter = 0, longest = 0, components = 0;
  int enqueue(prisim_ctx* ctx, const CleanState& S, int64_t nc_, int64_t maxiter_, hipStream_t s0) {
    nc = nc_; maxiter = maxiter_;
    ncomp.resize((size_t)nc); status.resize((size_t)nc); peak0.resize((size_t)nc);
    HIPCHK(ctx, hipMemcpyAsync(ncomp.data(), S.ncomp, (size_t)nc * 4, hipMemcpyDeviceToHost, s0));
    HIPCHK(ctx, hipMemcpyAsync(status.data(), S.status, (size_t)nc * 4, hipMemcpyDeviceToHost, s0));
    HIPCHK(ctx, hipMemcpyAsync(peak0.data(), S.peak0, (size_t)nc * 8, hipMemcpyDeviceToHost, s0));
    return PRISIM_OK;
  }
  int lists(prisim_ctx* ctx, const CleanState& S, hipStream_t s0) {
    for (int64_t k = 0; k < nc; ++k) {
      if (ncomp[(size_t)k] < 0 || ncomp[(size_t)k] > maxiter) return fail(ctx, PRISIM_EINTERNAL, "a component count beyond maxiter");
      longest = std::max<int64_t>(longest, ncomp[(size_t)k]);
      components += ncomp[(size_t)k];
    }
    pix.resize((size_t)(nc * longest));
    flux.resize((size_t)(nc * longest));
    if (longest > 0) {
      HIPCHK(ctx, copy_rows(pix.data(), (size_t)longest * 4, S.comp_pixel, (size_t)maxiter * 4, (size_t)longest * 4, (size_t)nc,
                            hipMemcpyDeviceToHost, s0));
      HIPCHK(ctx, copy_rows(flux.data(), (size_t)longest * 8, S.comp_flux, (size_t)maxiter * 8, (size_t)longest * 8, (size_t)nc,
                            hipMemcpyDeviceToHost, s0));
      HIPCHK(ctx, hipStreamSynchronize(s0));
    }
    return PRISIM_OK;
  }
  void write(int32_t* out_comp_pixel, double* out_comp_flux, int32_t* out_ncomp, int32_t* out_status, double* out_peak0) const {
    for (int64_t k = 0; k < nc; ++k) {
      const size_t n = (size_t)ncomp[(size_t)k];
      if (n) std::memcpy(out_comp_pixel + k * maxiter, pix.data() + k * longest, n * 4);
      if (n) std::memcpy(out_comp_flux + k * maxiter, flux.data() + k * longest, n * 8);
    }
    std::memcpy(out_ncomp, ncomp.data(), (size_t)nc * 4);
    std::memcpy(out_status, status.data(), (size_t)nc * 4);
    std::memcpy(out_peak0, peak0.data(), (size_t)nc * 8);
  }
};

// why the plan of an entry cannot run, in full; lds_of: whose LDS the plan counted
inline std::string clean_refusal(const char* refusal, int64_t total, const char* lds_of, int64_t lds) {
  return std::string(refusal) + " (the resident buffers take " + std::to_string(total) + " B, " + lds_of + " " + std::to_string(lds) + " B of LDS)";
}

// what every entry returns: the two images and the state of the channels with their lists
struct CleanOutputs {
  double *residual, *restored;
  int32_t* comp_pixel;
  double* comp_flux;
  int32_t *ncomp, *status;
  double* peak0;
};

// The frame of a call, which the three entries step through alike around what is their own -- the plan, the first residual, the
// loop and the extra outputs:
//   check_outputs, check_inputs   in the order the entries report faults: the struct and the outputs, (the entry's further outputs,)
//                     the shared fields, the entry's own fields, those of the CLEAN, the resident cube and the set-up.
//   open              behind the plan, by its ImcleanPlan geometry: the one stream, the tables with the window and the restoring
//                     beams, the partials and the state; the context's stream is waited for where its resident cube is read.
//   init, search, decide   the launches on the state: k_imclean_init behind the first residual, k_imclean_peak1 over whichever image
//                     the entry searches, k_imclean_peak2 with the entry's flux.
//   close, gather, write   the residual, the state and, when asked, the restoration come down and the stream drains; gather() brings
//                     the filled columns of the lists; write() copies all of it out once the call can no longer fail: nothing
//                     reaches the caller's arrays from a call that fails.
// Lifetimes: the stream is drained when `wk` goes (~Streams), on every return path.  So `wk` is the last member, behind the tables'
// host frames, the lists and the host images, which then outlive every copy in flight; and an entry declares its own host buffers
// (a DirtyResidual among them) before its CleanCall, for the same reason.
struct CleanCall {
  prisim_ctx* const ctx;
  const CleanOutputs out;
  const bool timed;
  const WallTime wall0 = wall_now();
  ImgView v{};
  ImgSetup su{};
  int64_t npix = 0, nchan = 0, nc = 0, maxiter = 0;     // nc: image channels
  bool avg = false, restore = false;
  const uint8_t* window = nullptr;                      // the caller's
  const double* fwhm_rad = nullptr;
  ImcleanPlan pl{};
  hipStream_t s0 = nullptr;
  ImgTables T;
  uint8_t* d_window = nullptr;
  double* d_fwhm = nullptr;
  int64_t upload = 0;                                   // bytes copied up
  Peak* d_partial = nullptr;
  CleanState S{};
  CleanLists lists;
  std::vector<double> h_res, h_rest;
  Work wk;                                              // the last member: see above

  CleanCall(prisim_ctx* ctx_, const CleanOutputs& out_, bool timed_) : ctx(ctx_), out(out_), timed(timed_) {}

  template <typename Args>
  int check_outputs(const Args* a) const {
    if (!a) return fail(ctx, PRISIM_EINVAL, "the argument struct is NULL");
    if (!out.residual) return fail(ctx, PRISIM_EINVAL, "out_residual is NULL");
    if (!out.comp_pixel || !out.comp_flux || !out.ncomp || !out.status || !out.peak0)
      return fail(ctx, PRISIM_EINVAL, "out_comp_pixel, out_comp_flux, out_ncomp, out_status or out_peak0 is NULL");
    return PRISIM_OK;
  }
  // own(): the checks of the fields only this entry has, 0 or a PRISIM_E* code
  template <typename Args, typename Own>
  int check_inputs(const Args& a, Own&& own) {
    v = imaging_view(a);
    if (int rc = check_args(ctx, v)) return rc;
    if (int rc = own()) return rc;
    npix = a.npix; nchan = a.nchan; maxiter = a.maxiter;
    avg = a.chan_avg != 0; restore = out.restored != nullptr;
    nc = avg ? 1 : nchan;
    window = a.window; fwhm_rad = a.fwhm_rad;
    if (int rc = check_clean_args(ctx, a, nc, restore)) return rc;
    return imaging_preamble(ctx, v, su);
  }
  template <typename Args>
  int check_inputs(const Args& a) { return check_inputs(a, [] { return PRISIM_OK; }); }

  int open(const ImcleanPlan& plan) {
    pl = plan;
    h_res.resize((size_t)(npix * nc));
    h_rest.resize(restore ? (size_t)(npix * nc) : 0);
    if (int rc = wk.st.create(ctx, 1, false)) return rc;
    s0 = wk.st.s[0];
    if (int rc = upload_tables(ctx, wk.dev, v, s0, T)) return rc;
    upload = T.bytes;
    if (window) {
      DEV_UPLOAD(ctx, wk.dev, d_window, window, (size_t)npix, s0);
      upload += npix;
    }
    if (restore) {
      DEV_UPLOAD(ctx, wk.dev, d_fwhm, fwhm_rad, (size_t)nc, s0);
      upload += nc * 8;
    }
    DEV_ALLOC(ctx, wk.dev, d_partial, pl.partial_bytes);
    if (int rc = alloc_clean_state(ctx, wk.dev, S, nc, maxiter)) return rc;
    // the kernels start behind whatever the context's stream still writes into the resident cube, which is read where it lies
    if (v.resident()) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return PRISIM_OK;
  }

  // wk: W[k], or their sum with chan_avg
  int init(const double* wk_) { return launch(ctx, k_imclean_init, dim3((unsigned)((nc + kThreads - 1) / kThreads)), 0, s0, S, wk_, (int)nc); }
  int search(const double* image) {
    return launch(ctx, k_imclean_peak1, dim3((unsigned)pl.nslabs, (unsigned)pl.peak_cgroups), 0, s0, image, (const uint8_t*)d_window,
                  (const int32_t*)S.status, npix, (int)nc, pl.slab, (int)pl.peak_cx, d_partial);
  }
  template <typename Flux, typename Args>
  int decide(const Flux& flux, const Args& a, bool first) {
    return launch(ctx, k_imclean_peak2<Flux>, dim3(1), 0, s0, S, (const Peak*)d_partial, flux, (int)nc, pl.nslabs, maxiter, a.gain, a.threshold,
                  (int)a.threshold_relative, first ? 1 : 0);
  }

  // image [npix][nc]: the residual, restored in place behind its download.  The events, where there are any, are recorded before
  // and behind the restoring kernel and behind the last download
  int close(double* image, hipEvent_t before = nullptr, hipEvent_t after = nullptr, hipEvent_t end = nullptr) {
    HIPCHK(ctx, hipMemcpyAsync(h_res.data(), image, h_res.size() * 8, hipMemcpyDeviceToHost, s0));
    if (int rc = lists.enqueue(ctx, S, nc, maxiter, s0)) return rc;
    if (restore) {
      if (before) HIPCHK(ctx, hipEventRecord(before, s0));
      if (int rc = launch(ctx, k_imclean_restore, dim3((unsigned)grid_for(ctx, npix * nc)), 0, s0, image, T.uvec, S, (const double*)d_fwhm, npix,
                          (int)nc, maxiter))
        return rc;
      if (after) HIPCHK(ctx, hipEventRecord(after, s0));
      HIPCHK(ctx, hipMemcpyAsync(h_rest.data(), image, h_rest.size() * 8, hipMemcpyDeviceToHost, s0));
    }
    if (end) HIPCHK(ctx, hipEventRecord(end, s0));
    HIPCHK(ctx, hipStreamSynchronize(s0));
    return PRISIM_OK;
  }
  // behind close(), and behind whatever verdict of its own the entry reads from the idle stream before it
  int gather() { return lists.lists(ctx, S, s0); }
  void write() const {
    std::memcpy(out.residual, h_res.data(), h_res.size() * 8);
    if (restore) std::memcpy(out.restored, h_rest.data(), h_rest.size() * 8);
    lists.write(out.comp_pixel, out.comp_flux, out.ncomp, out.status, out.peak0);
  }
  // the fields every stats struct of the entries has: the wall time, the components, the bytes up, and those of the plan
  template <typename Stats>
  void common_stats(Stats* st, int64_t device_bytes) const {
    st->wall_ms = wall_ms_since(wall0);
    st->components = lists.components;
    st->upload_bytes = upload;
    st->device_bytes = device_bytes;
    plan_stats(st, v, pl, 1);
  }
};

// The iterations: maxiter + 1 at most end every channel, since an active channel gains a component in each.  They are enqueued
// `batch` at a time on the call's stream -- search(first) then update(), each returning 0 or a PRISIM_E* code -- and after each batch
// the host reads the 16 bytes of S.counts and stops at 0 active channels: the device never waits for the host inside a batch.  A
// timed call records 2 batch + 1 events per batch.
struct CleanLoop {
  int64_t counts[2] = {1, 0};                           // what the polls read: channels active, iterations in which any was
  int64_t polls = 0;
  double peak_ms = 0.0, update_ms = 0.0;
  template <typename Search, typename Update>
  int run(const CleanCall& c, int batch, Search&& search, Update&& update) {
    prisim_ctx* ctx = c.ctx;
    const CleanState& S = c.S;
    BatchEvents be;
    if (c.timed)
      if (int rc = be.create(ctx, 2 * batch + 1)) return rc;
    int64_t enqueued = 0;
    while (counts[0] > 0 && enqueued < c.maxiter + 1) {
      const int n = (int)std::min<int64_t>(batch, c.maxiter + 1 - enqueued);
      if (c.timed) HIPCHK(ctx, hipEventRecord(be.ev[0], c.s0));
      for (int i = 0; i < n; ++i) {
        if (int rc = search(enqueued + i == 0)) return rc;
        if (c.timed) HIPCHK(ctx, hipEventRecord(be.ev[(size_t)(2 * i + 1)], c.s0));
        if (int rc = update()) return rc;
        if (c.timed) HIPCHK(ctx, hipEventRecord(be.ev[(size_t)(2 * i + 2)], c.s0));
      }
      enqueued += n;
      HIPCHK(ctx, hipMemcpyAsync(counts, S.counts, 16, hipMemcpyDeviceToHost, c.s0));
      HIPCHK(ctx, hipStreamSynchronize(c.s0));
      ++polls;
      for (int i = 0; c.timed && i < n; ++i) {
        peak_ms += elapsed_ms(be.ev[(size_t)(2 * i)], be.ev[(size_t)(2 * i + 1)]);
        update_ms += elapsed_ms(be.ev[(size_t)(2 * i + 1)], be.ev[(size_t)(2 * i + 2)]);
      }
    }
    if (c.maxiter + 1 > 0 && counts[0] > 0) return fail(ctx, PRISIM_EINTERNAL, "channels still active after maxiter + 1 iterations");
    return PRISIM_OK;
  }
};

// The buffers of a CLEAN whose residual is the dirty image, by the plan: the offsets, the residual, with chan_avg the rows it is
// averaged from, the weight sums and their sum.  rows() and R are what enqueue_dirty (dirty_image.h) writes; norm() divides the image,
// starts the state (CleanCall::init) and is returned as wsum.  Declared before the CleanCall it serves: h_norm takes a copy in flight
struct DirtyResidual {
  double4* dd = nullptr;
  double *R = nullptr, *D = nullptr, *wsum = nullptr, *wtot = nullptr;
  bool avg = false;
  std::vector<double> h_norm;
  int alloc(CleanCall& c) {
    avg = c.avg;
    DEV_ALLOC(c.ctx, c.wk.dev, dd, c.pl.dd_bytes);
    DEV_ALLOC(c.ctx, c.wk.dev, R, c.pl.resid_bytes);
    if (avg) DEV_ALLOC(c.ctx, c.wk.dev, D, c.pl.scratch_bytes);
    DEV_ALLOC(c.ctx, c.wk.dev, wsum, c.nchan * 8);
    DEV_ALLOC(c.ctx, c.wk.dev, wtot, 8);
    return PRISIM_OK;
  }
  double* rows() const { return avg ? D : R; }
  const double* norm() const { return avg ? wtot : wsum; }
  int download_norm(const CleanCall& c) {
    h_norm.resize((size_t)c.nc);
    HIPCHK(c.ctx, hipMemcpyAsync(h_norm.data(), norm(), (size_t)c.nc * 8, hipMemcpyDeviceToHost, c.s0));
    return PRISIM_OK;
  }
  void write_norm(double* out_wsum) const {
    if (out_wsum) std::memcpy(out_wsum, h_norm.data(), h_norm.size() * 8);
  }
};

}  // namespace

#endif  // PRISIM_CLEAN_KERNELS_H
