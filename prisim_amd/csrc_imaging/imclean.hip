// imclean.hip -- Hogbom CLEAN of a dirty image with the exact beam for gfx950 (include/prisim_imclean.h).  The first residual is the
// dirty image as prisim_dirty_image enqueues it (dirty_image.h), over all pixels at once; then, per iteration, three launches that
// never wait for the host:
//   k_imclean_peak1   reads the residual channel-fastest.  A workgroup is cx channels by 256 / cx pixel lanes and owns a slab of pixels;
//                     a lane keeps the largest |R| of its pixels (by >, ascending pixels, so the lowest index wins a tie and a NaN never
//                     wins), the lanes are reduced in LDS under the associative rule "larger |value|, then lower index", and the
//                     partial (|value|, index) of (slab, channel) is written.  Channels that have ended are not read.
//   k_imclean_peak2   one workgroup, a thread per image channel: reduces the partials, applies the stop rule, appends the component and
//                     publishes (q_k, a_k) -- a_k = 0 once the channel has ended -- and the count of active channels.
//   k_imclean_update  the hot path: the tile pass of k_img_sum (img_tile_pass of imaging_kernels.h, where it is described), so the same
//                     summation order.  The staged operand is computed, not loaded: element (r, c) is
//                     w a_k (cos phi_q, -sin phi_q), phi_q = 2 pi f_k b_r . dd[t][q_k] / c from the channel's true frequency (cycles_phasor),
//                     four phasors per thread and pass.  The epilogue subtracts acc / W[k] from R in place, only where a_k != 0; a tile
//                     whose a_k are all 0 returns at once, so an ended channel keeps its bits.  With chan_avg every channel shares (q, a),
//                     the numerators go to the scratch rows and k_imclean_avg_sub sums them over the band, k ascending as k_img_avg does.
// No atomics, no floating-point reduction whose order depends on the launch.  k_imclean_restore adds the components through a
// Gaussian beam, one thread per (pixel, channel), components in list order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/prisim_imclean.h"
#include "../csrc_addon/imclean_plan.h"
#include "dirty_image.h"

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

// one workgroup.  first: this is the first iteration, which sets P0 and the threshold
__global__ void __launch_bounds__(kThreads) k_imclean_peak2(CleanState S, const Peak* __restrict__ partial, const double* __restrict__ R, int nc,
                                                            int64_t nslabs, int64_t maxiter, double gain, double threshold, int relative,
                                                            int first) {
  __shared__ int sh_n[kThreads];
  int active = 0;
  for (int k = threadIdx.x; k < nc; k += kThreads) {
    if (S.status[k] != 0) { S.a[k] = 0.0; continue; }
    Peak m{-1.0, -1, 0};
    for (int64_t s = 0; s < nslabs; ++s) {
      const Peak o = partial[s * nc + k];
      if (peak_beats(o, m)) m = o;
    }
    if (first) {
      if (m.p >= 0) S.peak0[k] = m.v;
      S.thr[k] = relative ? threshold * m.v : threshold;
    }
    double ak = 0.0;
    if (m.p < 0 || !(m.v > S.thr[k])) {
      S.status[k] = PRISIM_IMCLEAN_THRESHOLD;
    } else if (S.ncomp[k] >= maxiter) {
      S.status[k] = PRISIM_IMCLEAN_MAXITER;
    } else {
      const int32_t n = S.ncomp[k];
      ak = gain * R[(int64_t)m.p * nc + k];
      S.comp_pixel[(int64_t)k * maxiter + n] = m.p;
      S.comp_flux[(int64_t)k * maxiter + n] = ak;
      S.ncomp[k] = n + 1;
      S.q[k] = m.p;
      ++active;
    }
    S.a[k] = ak;
  }
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

struct UpdParams {
  ImgWeights W;
  const double* bl;         // [nbl][3]
  const double* freqs;      // [nchan]
  const double4* dd;        // [nt][npix]
  const double* wsum;       // [nchan]
  const int32_t* q;         // [nc] the picks
  const double* a;          // [nc] their fluxes
  double df;
  int64_t nbl, nt, npix;
  int nchan, avg;           // avg: one (q, a) for the band, and the numerators are written to out
  double* out;              // avg = 0: R [npix][nchan], updated in place; avg = 1: the scratch rows [npix][nchan]
};

// grid: x = block of pixels, y = channel tile.  LDS: kImagingLds + 12 B per channel of the tile
template <bool STEPPED>
__global__ void __launch_bounds__(kThreads) k_imclean_update(UpdParams P) {
  __shared__ double2 sh_v[NB * CT];     // w a_k (cos phi_q, -sin phi_q)
  __shared__ double sh_b[NB * 3];       // b / c
  __shared__ double sh_f[CT];           // the tile's frequencies; past the band: the last channel's (their operand rows are 0)
  __shared__ double sh_a[CT];           // the tile's fluxes; past the band: 0
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
    const double ak = sh_a[c];
    if (live && ak != 0.0) {                      // ak != 0 only inside the band
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
  for (int64_t t = 0; t < P.nt; ++t)
    img_tile_pass<STEPPED, false>(t, P.dd[t * P.npix + pl], P.bl, P.nbl, k0, f0, P.df, sh_v, sh_b, sh_f, acc, stage);
  if (!p_valid) return;
  double* out = P.out + pl * P.nchan + k0;
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

// grid: x over the pixels.  R[pixel] -= sum_k D[pixel][k] / wtot, k ascending; nothing when the band has ended
__global__ void __launch_bounds__(kThreads) k_imclean_avg_sub(const double* __restrict__ D, int64_t npix, int nchan, const double* __restrict__ wtot,
                                                              const double* __restrict__ a, double* __restrict__ R) {
  const int64_t pl = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (pl >= npix || a[0] == 0.0) return;
  double s = 0.0;
  for (int k = 0; k < nchan; ++k) s += D[pl * nchan + k];
  R[pl] -= s / wtot[0];
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

double elapsed_ms(hipEvent_t e0, hipEvent_t e1) {
  float ms = 0.f;
  return hipEventElapsedTime(&ms, e0, e1) == hipSuccess ? (double)ms : 0.0;
}

int clean_image(prisim_ctx* ctx, const prisim_imclean_args* a, double* out_residual, double* out_restored, int32_t* out_comp_pixel,
                double* out_comp_flux, int32_t* out_ncomp, int32_t* out_status, double* out_peak0, double* out_wsum,
                prisim_imclean_stats* stats) {
  if (!ctx) return PRISIM_EINVAL;
  const WallTime wall0 = wall_now();
  if (!a) return fail(ctx, PRISIM_EINVAL, "the argument struct is NULL");
  if (!out_residual) return fail(ctx, PRISIM_EINVAL, "out_residual is NULL");
  if (!out_comp_pixel || !out_comp_flux || !out_ncomp || !out_status || !out_peak0)
    return fail(ctx, PRISIM_EINVAL, "out_comp_pixel, out_comp_flux, out_ncomp, out_status or out_peak0 is NULL");
  const ImgView v = imaging_view(*a);
  if (int rc = check_args(ctx, v)) return rc;
  const int64_t npix = a->npix, nbl = a->nbl, nchan = a->nchan, nt = a->nt, maxiter = a->maxiter;
  const bool avg = a->chan_avg != 0, restore = out_restored != nullptr;
  const int64_t nc = avg ? 1 : nchan;
  if (!(a->gain > 0.0 && a->gain <= 1.0)) return fail(ctx, PRISIM_EINVAL, "gain must lie in (0, 1]");
  if (!(a->threshold >= 0.0) || !std::isfinite(a->threshold)) return fail(ctx, PRISIM_EINVAL, "threshold must be finite and non-negative");
  if (a->threshold_relative != 0 && a->threshold_relative != 1) return fail(ctx, PRISIM_EINVAL, "threshold_relative must be 0 or 1");
  if (a->threshold_relative && !(a->threshold < 1.0)) return fail(ctx, PRISIM_EINVAL, "a relative threshold must be below 1");
  if (a->window && std::all_of(a->window, a->window + npix, [](uint8_t x) { return x == 0; }))
    return fail(ctx, PRISIM_EINVAL, "the window holds no pixel");
  if (restore && !a->fwhm_rad) return fail(ctx, PRISIM_EINVAL, "out_restored needs fwhm_rad");
  for (int64_t k = 0; restore && k < nc; ++k)
    if (!(a->fwhm_rad[k] > 0.0) || !std::isfinite(a->fwhm_rad[k]))
      return fail(ctx, PRISIM_EINVAL, "fwhm_rad[" + std::to_string(k) + "] is not positive and finite");
  ImgSetup su{};
  if (int rc = imaging_preamble(ctx, v, su)) return rc;
  const ImcleanPlan pl = imclean_plan(npix, nbl, nchan, nt, avg, maxiter, a->budget_bytes, su.lds_max, a->route, su.uniform);
  if (pl.refusal)
    return fail(ctx, PRISIM_EINVAL, std::string(pl.refusal) + " (the resident buffers take " + std::to_string(pl.total) + " B, the workgroup " +
                                        std::to_string(pl.lds) + " B of LDS)");
  const bool stepped = pl.route == kImagingStepped;
  const int batch = imclean_batch(a->poll_every);
  const bool timed = stats != nullptr;

  // the results wait here until the call is through: nothing reaches the caller's arrays from a call that fails
  std::vector<double> h_res((size_t)(npix * nc)), h_rest(restore ? (size_t)(npix * nc) : 0), h_peak0((size_t)nc), h_wsum((size_t)nc);
  std::vector<int32_t> h_ncomp((size_t)nc), h_status((size_t)nc);
  std::vector<int32_t> h_pix;
  std::vector<double> h_flux;
  int64_t h_counts[2] = {1, 0};                         // what the polls read: channels active, iterations in which any was
  ImgTables T;

  Work wk;
  BatchEvents be;
  Streams& st = wk.st;
  if (int rc = st.create(ctx, 1, false)) return rc;
  hipStream_t s0 = st.s[0];
  if (timed)
    if (int rc = be.create(ctx, 2 * batch + 1)) return rc;

  if (int rc = upload_tables(ctx, wk.dev, v, s0, T)) return rc;
  const ImgWeights& W = T.W;
  int64_t upload = T.bytes;
  double* d_fwhm = nullptr;
  uint8_t* d_window = nullptr;
  if (a->window) {
    DEV_UPLOAD(ctx, wk.dev, d_window, a->window, (size_t)npix, s0);
    upload += npix;
  }
  if (restore) {
    DEV_UPLOAD(ctx, wk.dev, d_fwhm, a->fwhm_rad, (size_t)nc, s0);
    upload += nc * 8;
  }

  // the resident buffers of the plan
  double4* d_dd = nullptr;
  double *d_R = nullptr, *d_D = nullptr, *d_wsum = nullptr, *d_wtot = nullptr;
  Peak* d_partial = nullptr;
  CleanState S{};
  DEV_ALLOC(ctx, wk.dev, d_dd, pl.dd_bytes);
  DEV_ALLOC(ctx, wk.dev, d_R, pl.resid_bytes);
  if (avg) DEV_ALLOC(ctx, wk.dev, d_D, pl.scratch_bytes);
  DEV_ALLOC(ctx, wk.dev, d_partial, pl.partial_bytes);
  DEV_ALLOC(ctx, wk.dev, d_wsum, nchan * 8);
  DEV_ALLOC(ctx, wk.dev, d_wtot, 8);
  DEV_ALLOC(ctx, wk.dev, S.q, nc * 4);
  DEV_ALLOC(ctx, wk.dev, S.a, nc * 8);
  DEV_ALLOC(ctx, wk.dev, S.thr, nc * 8);
  DEV_ALLOC(ctx, wk.dev, S.peak0, nc * 8);
  DEV_ALLOC(ctx, wk.dev, S.ncomp, nc * 4);
  DEV_ALLOC(ctx, wk.dev, S.status, nc * 4);
  DEV_ALLOC(ctx, wk.dev, S.counts, 16);
  DEV_ALLOC(ctx, wk.dev, S.comp_pixel, nc * maxiter * 4);
  DEV_ALLOC(ctx, wk.dev, S.comp_flux, nc * maxiter * 8);

  Events tev;                                           // [0] .. [1] the dirty image, [2] .. [3] the restoration
  if (timed)
    if (int rc = tev.create(ctx)) return rc;
  // the kernels start behind whatever the context's stream still writes into the resident cube, which is read where it lies
  if (v.resident()) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));

  // ---- the dirty image of all pixels
  if (timed) HIPCHK(ctx, hipEventRecord(tev.e[0], s0));
  const DirtyImage job = dirty_image_of(v, T, su.df, pl, d_wsum, d_wtot);
  if (int rc = enqueue_weight_sums(ctx, job, s0)) return rc;
  if (int rc = enqueue_dirty(ctx, job, Span{0, npix}, d_dd, avg ? d_D : d_R, d_R, s0)) return rc;
  const dim3 grid((unsigned)pl.nblocks, (unsigned)pl.ntiles), pixgrid((unsigned)((npix + kThreads - 1) / kThreads));
  if (int rc = launch(ctx, k_imclean_init, dim3((unsigned)((nc + kThreads - 1) / kThreads)), 0, s0, S, (const double*)(avg ? d_wtot : d_wsum), (int)nc))
    return rc;
  if (timed) HIPCHK(ctx, hipEventRecord(tev.e[1], s0));

  // ---- the iterations: maxiter + 1 at most end every channel, since an active channel gains a component in each
  UpdParams U;
  U.W = W;
  U.bl = T.bl; U.freqs = T.freqs; U.dd = d_dd; U.wsum = d_wsum;
  U.q = S.q; U.a = S.a;
  U.df = su.df;
  U.nbl = nbl; U.nt = nt; U.npix = npix;
  U.nchan = (int)nchan; U.avg = avg ? 1 : 0;
  U.out = avg ? d_D : d_R;
  const dim3 peakgrid((unsigned)pl.nslabs, (unsigned)pl.peak_cgroups);
  int64_t enqueued = 0, polls = 0;
  double peak_ms = 0.0, update_ms = 0.0;
  while (h_counts[0] > 0 && enqueued < maxiter + 1) {
    const int n = (int)std::min<int64_t>(batch, maxiter + 1 - enqueued);
    if (timed) HIPCHK(ctx, hipEventRecord(be.ev[0], s0));
    for (int i = 0; i < n; ++i) {
      if (int rc = launch(ctx, k_imclean_peak1, peakgrid, 0, s0, (const double*)d_R, (const uint8_t*)d_window, (const int32_t*)S.status, npix,
                          (int)nc, pl.slab, (int)pl.peak_cx, d_partial))
        return rc;
      hipLaunchKernelGGL(k_imclean_peak2, dim3(1), dim3(kThreads), 0, s0, S, (const Peak*)d_partial, (const double*)d_R, (int)nc, pl.nslabs,
                         maxiter, a->gain, a->threshold, (int)a->threshold_relative, enqueued + i == 0 ? 1 : 0);
      HIPCHK(ctx, hipGetLastError());
      if (timed) HIPCHK(ctx, hipEventRecord(be.ev[(size_t)(2 * i + 1)], s0));
      if (int rc = stepped ? launch(ctx, k_imclean_update<true>, grid, 0, s0, U) : launch(ctx, k_imclean_update<false>, grid, 0, s0, U)) return rc;
      if (avg)
        if (int rc = launch(ctx, k_imclean_avg_sub, pixgrid, 0, s0, (const double*)d_D, npix, (int)nchan, (const double*)d_wtot,
                            (const double*)S.a, d_R))
          return rc;
      if (timed) HIPCHK(ctx, hipEventRecord(be.ev[(size_t)(2 * i + 2)], s0));
    }
    enqueued += n;
    HIPCHK(ctx, hipMemcpyAsync(h_counts, S.counts, 16, hipMemcpyDeviceToHost, s0));
    HIPCHK(ctx, hipStreamSynchronize(s0));
    ++polls;
    for (int i = 0; timed && i < n; ++i) {
      peak_ms += elapsed_ms(be.ev[(size_t)(2 * i)], be.ev[(size_t)(2 * i + 1)]);
      update_ms += elapsed_ms(be.ev[(size_t)(2 * i + 1)], be.ev[(size_t)(2 * i + 2)]);
    }
  }
  if (maxiter + 1 > 0 && h_counts[0] > 0) return fail(ctx, PRISIM_EINTERNAL, "channels still active after maxiter + 1 iterations");

  // ---- the results
  HIPCHK(ctx, hipMemcpyAsync(h_res.data(), d_R, h_res.size() * 8, hipMemcpyDeviceToHost, s0));
  HIPCHK(ctx, hipMemcpyAsync(h_ncomp.data(), S.ncomp, (size_t)nc * 4, hipMemcpyDeviceToHost, s0));
  HIPCHK(ctx, hipMemcpyAsync(h_status.data(), S.status, (size_t)nc * 4, hipMemcpyDeviceToHost, s0));
  HIPCHK(ctx, hipMemcpyAsync(h_peak0.data(), S.peak0, (size_t)nc * 8, hipMemcpyDeviceToHost, s0));
  HIPCHK(ctx, hipMemcpyAsync(h_wsum.data(), avg ? d_wtot : d_wsum, (size_t)nc * 8, hipMemcpyDeviceToHost, s0));
  if (restore) {
    if (timed) HIPCHK(ctx, hipEventRecord(tev.e[2], s0));
    if (int rc = launch(ctx, k_imclean_restore, dim3((unsigned)grid_for(ctx, npix * nc)), 0, s0, d_R, T.uvec, S,
                        (const double*)d_fwhm, npix, (int)nc, maxiter))
      return rc;
    if (timed) HIPCHK(ctx, hipEventRecord(tev.e[3], s0));
    HIPCHK(ctx, hipMemcpyAsync(h_rest.data(), d_R, h_rest.size() * 8, hipMemcpyDeviceToHost, s0));
  }
  HIPCHK(ctx, hipStreamSynchronize(s0));
  // of the lists, the columns that any channel filled
  int64_t longest = 0, components = 0;
  for (int64_t k = 0; k < nc; ++k) {
    if (h_ncomp[(size_t)k] < 0 || h_ncomp[(size_t)k] > maxiter) return fail(ctx, PRISIM_EINTERNAL, "a component count beyond maxiter");
    longest = std::max<int64_t>(longest, h_ncomp[(size_t)k]);
    components += h_ncomp[(size_t)k];
  }
  h_pix.resize((size_t)(nc * longest));
  h_flux.resize((size_t)(nc * longest));
  if (longest > 0) {
    HIPCHK(ctx, copy_rows(h_pix.data(), (size_t)longest * 4, S.comp_pixel, (size_t)maxiter * 4, (size_t)longest * 4, (size_t)nc,
                          hipMemcpyDeviceToHost, s0));
    HIPCHK(ctx, copy_rows(h_flux.data(), (size_t)longest * 8, S.comp_flux, (size_t)maxiter * 8, (size_t)longest * 8, (size_t)nc,
                          hipMemcpyDeviceToHost, s0));
    HIPCHK(ctx, hipStreamSynchronize(s0));
  }

  std::memcpy(out_residual, h_res.data(), h_res.size() * 8);
  if (restore) std::memcpy(out_restored, h_rest.data(), h_rest.size() * 8);
  for (int64_t k = 0; k < nc; ++k) {
    const size_t n = (size_t)h_ncomp[(size_t)k];
    if (n) std::memcpy(out_comp_pixel + k * maxiter, h_pix.data() + k * longest, n * 4);
    if (n) std::memcpy(out_comp_flux + k * maxiter, h_flux.data() + k * longest, n * 8);
  }
  std::memcpy(out_ncomp, h_ncomp.data(), (size_t)nc * 4);
  std::memcpy(out_status, h_status.data(), (size_t)nc * 4);
  std::memcpy(out_peak0, h_peak0.data(), (size_t)nc * 8);
  if (out_wsum) std::memcpy(out_wsum, h_wsum.data(), (size_t)nc * 8);
  if (stats) {
    // the dirty image as dirty_kernel_bytes counts it.  An iteration, counted with every channel active: the update reads
    // per workgroup and (t, b) the tile's weights (8 B a channel when there are any), the pick's offsets (32 B a channel) and the
    // baseline twice (24 B), per pixel and snapshot its offsets (32 B per tile), and reads and writes the residual (16 B; with
    // chan_avg the scratch rows written and read, and 16 B a pixel); the peak search reads the residual and the window and writes and
    // reads the partials.
    const int64_t wg = pl.nblocks * pl.ntiles;
    const int64_t dirty_bytes = dirty_kernel_bytes(v, pl, W.w != nullptr);
    const int64_t iter_bytes = wg * nt * nbl * (pl.tile * (32 + (W.w ? 8 : 0)) + 48) + npix * nt * 32 * pl.ntiles + npix * nchan * 16 +
                               (avg ? npix * 16 : 0) + npix * nc * 8 + (a->window ? npix : 0) + pl.nslabs * nc * 32;
    const double dirty_ms = elapsed_ms(tev.e[0], tev.e[1]), restore_ms = restore ? elapsed_ms(tev.e[2], tev.e[3]) : 0.0;
    stats->wall_ms = wall_ms_since(wall0);
    stats->kernel_ms = dirty_ms + peak_ms + update_ms + restore_ms;
    stats->dirty_ms = dirty_ms;
    stats->peak_ms = peak_ms;
    stats->update_ms = update_ms;
    stats->restore_ms = restore_ms;
    stats->iterations = h_counts[1];
    stats->components = components;
    stats->polls = polls;
    stats->chunks = 1;
    stats->chunk_pixels = npix;
    stats->kernel_bytes = dirty_bytes + h_counts[1] * iter_bytes + (restore ? npix * nc * 16 : 0);
    stats->upload_bytes = upload;
    stats->download_bytes = npix * nc * 8 * (restore ? 2 : 1) + nc * 32 + nc * longest * 12 + polls * 16;
    stats->device_bytes = pl.total;
    plan_stats(stats, v, pl, 1);
  }
  return PRISIM_OK;
}

}  // namespace

extern "C" {

int prisim_clean_image(prisim_ctx* ctx, const prisim_imclean_args* a, double* out_residual, double* out_restored, int32_t* out_comp_pixel,
                       double* out_comp_flux, int32_t* out_ncomp, int32_t* out_status, double* out_peak0, double* out_wsum,
                       prisim_imclean_stats* stats) {
  return guarded(ctx, [&]() -> int {
    return clean_image(ctx, a, out_residual, out_restored, out_comp_pixel, out_comp_flux, out_ncomp, out_status, out_peak0, out_wsum, stats);
  });
}

}  // extern "C"
