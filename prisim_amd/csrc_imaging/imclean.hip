// imclean.hip -- Hogbom CLEAN of a dirty image with the exact beam for gfx950 (include/prisim_imclean.h).  The first residual is the
// dirty image as prisim_dirty_image enqueues it (dirty_image.h), over all pixels at once; then, per iteration, three launches that
// never wait for the host:
//   k_imclean_peak1, k_imclean_peak2   the peak search and the stop rule of clean_kernels.h, on the residual itself; the flux of a
//                     component is gain times the residual at the pick (ResidualFlux).
//   k_imclean_update  the hot path: the tile pass of k_img_sum (img_tile_pass of imaging_kernels.h, where it is described), so the same
//                     summation order.  The staged operand is computed, not loaded: element (r, c) is
//                     w a_k (cos phi_q, -sin phi_q), phi_q = 2 pi f_k b_r . dd[t][q_k] / c from the channel's true frequency (cycles_phasor),
//                     four phasors per thread and pass.  The epilogue subtracts acc / W[k] from R in place, only where a_k != 0; a tile
//                     whose a_k are all 0 returns at once, so an ended channel keeps its bits.  With chan_avg every channel shares (q, a),
//                     the numerators go to the scratch rows and k_imclean_avg_sub sums them over the band, k ascending as k_img_avg does.
// No atomics, no floating-point reduction whose order depends on the launch.  k_imclean_restore (clean_kernels.h) adds the components
// through a Gaussian beam.  The state, the batches of iterations with their polls and the gathering of the lists are those of
// clean_kernels.h, which prisim_clean_mosaic (mosclean.hip) shares.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/prisim_imclean.h"
#include "../csrc_addon/imclean_plan.h"
#include "clean_kernels.h"
#include "dirty_image.h"

namespace {

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
  if (int rc = check_clean_args(ctx, *a, nc, restore)) return rc;
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
  std::vector<double> h_res((size_t)(npix * nc)), h_rest(restore ? (size_t)(npix * nc) : 0), h_wsum((size_t)nc);
  CleanLists lists;
  CleanLoop loop;
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
  if (int rc = alloc_clean_state(ctx, wk.dev, S, nc, maxiter)) return rc;

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
  const ResidualFlux flux{d_R, (int)nc};
  auto search = [&](bool first) -> int {
    if (int rc = launch(ctx, k_imclean_peak1, peakgrid, 0, s0, (const double*)d_R, (const uint8_t*)d_window, (const int32_t*)S.status, npix,
                        (int)nc, pl.slab, (int)pl.peak_cx, d_partial))
      return rc;
    hipLaunchKernelGGL(k_imclean_peak2<ResidualFlux>, dim3(1), dim3(kThreads), 0, s0, S, (const Peak*)d_partial, flux, (int)nc, pl.nslabs,
                       maxiter, a->gain, a->threshold, (int)a->threshold_relative, first ? 1 : 0);
    HIPCHK(ctx, hipGetLastError());
    return PRISIM_OK;
  };
  auto update = [&]() -> int {
    if (int rc = stepped ? launch(ctx, k_imclean_update<true>, grid, 0, s0, U) : launch(ctx, k_imclean_update<false>, grid, 0, s0, U)) return rc;
    if (avg)
      return launch(ctx, k_imclean_avg_sub, pixgrid, 0, s0, (const double*)d_D, npix, (int)nchan, (const double*)d_wtot, (const double*)S.a, d_R);
    return PRISIM_OK;
  };
  if (int rc = loop.run(ctx, s0, S, maxiter, batch, be, search, update)) return rc;
  const int64_t polls = loop.polls;
  const double peak_ms = loop.peak_ms, update_ms = loop.update_ms;

  // ---- the results
  HIPCHK(ctx, hipMemcpyAsync(h_res.data(), d_R, h_res.size() * 8, hipMemcpyDeviceToHost, s0));
  if (int rc = lists.enqueue(ctx, S, nc, maxiter, s0)) return rc;
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
  if (int rc = lists.lists(ctx, S, s0)) return rc;
  const int64_t longest = lists.longest, components = lists.components;

  std::memcpy(out_residual, h_res.data(), h_res.size() * 8);
  if (restore) std::memcpy(out_restored, h_rest.data(), h_rest.size() * 8);
  lists.write(out_comp_pixel, out_comp_flux, out_ncomp, out_status, out_peak0);
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
    stats->iterations = loop.counts[1];
    stats->components = components;
    stats->polls = polls;
    stats->chunks = 1;
    stats->chunk_pixels = npix;
    stats->kernel_bytes = dirty_bytes + loop.counts[1] * iter_bytes + (restore ? npix * nc * 16 : 0);
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
