// imclean.hip -- Hogbom CLEAN of a dirty image with the exact beam for gfx950 (include/prisim_imclean.h).  The first residual is the
// dirty image as prisim_dirty_image enqueues it (dirty_image.h), over all pixels at once; then, per iteration, three launches that
// never wait for the host:
//   k_imclean_peak1, k_imclean_peak2   the peak search and the stop rule of clean_kernels.h, on the residual itself; the flux of a
//                     component is gain times the residual at the pick (ResidualFlux).
//   k_clean_update    the hot path, of clean_update.h where it is described, in its image form: the dirty image of the components'
//                     own visibilities by the tile pass of k_img_sum, so the same summation order.  The epilogue subtracts acc / W[k]
//                     from R in place, only where a_k != 0.  With chan_avg every channel shares (q, a), the numerators go to the
//                     scratch rows and k_imclean_avg_sub sums them over the band, k ascending as k_img_avg does.
// No atomics, no floating-point reduction whose order depends on the launch.  k_imclean_restore (clean_kernels.h) adds the components
// through a Gaussian beam.  The frame of the call (CleanCall), the state, the batches of iterations with their polls and the gathering
// of the lists are those of clean_kernels.h, which prisim_clean_mosaic (mosclean.hip) and prisim_clean_image_cs (csclean.hip) share;
// the buffers of the dirty-image residual (DirtyResidual) are shared with the latter.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/prisim_imclean.h"
#include "../csrc_addon/imclean_plan.h"
#include "clean_update.h"
#include "dirty_image.h"

namespace {

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
  DirtyResidual dr;                                     // before the call's frame, as the loop's poll is: the stream drains first
  CleanLoop loop;
  CleanCall call(ctx, {out_residual, out_restored, out_comp_pixel, out_comp_flux, out_ncomp, out_status, out_peak0}, stats != nullptr);
  if (int rc = call.check_outputs(a)) return rc;
  if (int rc = call.check_inputs(*a)) return rc;
  const ImgView& v = call.v;
  const int64_t npix = a->npix, nbl = a->nbl, nchan = a->nchan, nt = a->nt, nc = call.nc;
  const bool avg = call.avg, restore = call.restore;
  const ImcleanPlan pl = imclean_plan(npix, nbl, nchan, nt, avg, a->maxiter, a->budget_bytes, call.su.lds_max, a->route, call.su.uniform);
  if (pl.refusal) return fail(ctx, PRISIM_EINVAL, clean_refusal(pl.refusal, pl.total, "the workgroup", pl.lds));
  if (int rc = call.open(pl)) return rc;
  hipStream_t s0 = call.s0;
  if (int rc = dr.alloc(call)) return rc;
  Events tev;                                           // [0] .. [1] the dirty image, [2] .. [3] the restoration
  if (call.timed)
    if (int rc = tev.create(ctx)) return rc;

  // ---- the dirty image of all pixels
  if (call.timed) HIPCHK(ctx, hipEventRecord(tev.e[0], s0));
  const DirtyImage job = dirty_image_of(v, call.T, call.su.df, pl, dr.wsum, dr.wtot);
  if (int rc = enqueue_weight_sums(ctx, job, s0)) return rc;
  if (int rc = enqueue_dirty(ctx, job, Span{0, npix}, dr.dd, dr.rows(), dr.R, s0)) return rc;
  if (int rc = call.init(dr.norm())) return rc;
  if (call.timed) HIPCHK(ctx, hipEventRecord(tev.e[1], s0));

  // ---- the iterations
  const dim3 pixgrid((unsigned)((npix + kThreads - 1) / kThreads));
  const ResidualFlux flux{dr.R, (int)nc};
  auto search = [&](bool first) -> int {
    if (int rc = call.search(dr.R)) return rc;
    return call.decide(flux, *a, first);
  };
  auto update = [&]() -> int {
    if (int rc = enqueue_clean_update<false>(call, dr.dd, dr.wsum, dr.rows())) return rc;
    if (avg)
      return launch(ctx, k_imclean_avg_sub, pixgrid, 0, s0, (const double*)dr.D, npix, (int)nchan, (const double*)dr.wtot, (const double*)call.S.a, dr.R);
    return PRISIM_OK;
  };
  if (int rc = loop.run(call, imclean_batch(a->poll_every), search, update)) return rc;

  // ---- the results
  if (int rc = dr.download_norm(call)) return rc;
  if (int rc = call.close(dr.R, tev.e[2], tev.e[3])) return rc;
  if (int rc = call.gather()) return rc;
  call.write();
  dr.write_norm(out_wsum);
  if (stats) {
    // the dirty image as dirty_kernel_bytes counts it.  An iteration, counted with every channel active: the update reads
    // per workgroup and (t, b) the tile's weights (8 B a channel when there are any), the pick's offsets (32 B a channel) and the
    // baseline twice (24 B), per pixel and snapshot its offsets (32 B per tile), and reads and writes the residual (16 B; with
    // chan_avg the scratch rows written and read, and 16 B a pixel); the peak search reads the residual and the window and writes and
    // reads the partials.
    const bool weighted = call.T.W.w != nullptr;
    const int64_t wg = pl.nblocks * pl.ntiles, polls = loop.polls;
    const int64_t dirty_bytes = dirty_kernel_bytes(v, pl, weighted);
    const int64_t iter_bytes = wg * nt * nbl * (pl.tile * (32 + (weighted ? 8 : 0)) + 48) + npix * nt * 32 * pl.ntiles + npix * nchan * 16 +
                               (avg ? npix * 16 : 0) + npix * nc * 8 + (a->window ? npix : 0) + pl.nslabs * nc * 32;
    const double dirty_ms = elapsed_ms(tev.e[0], tev.e[1]), restore_ms = restore ? elapsed_ms(tev.e[2], tev.e[3]) : 0.0;
    call.common_stats(stats, pl.total);
    stats->kernel_ms = dirty_ms + loop.peak_ms + loop.update_ms + restore_ms;
    stats->dirty_ms = dirty_ms;
    stats->peak_ms = loop.peak_ms;
    stats->update_ms = loop.update_ms;
    stats->restore_ms = restore_ms;
    stats->iterations = loop.counts[1];
    stats->polls = polls;
    stats->chunks = 1;
    stats->chunk_pixels = npix;
    stats->kernel_bytes = dirty_bytes + loop.counts[1] * iter_bytes + (restore ? npix * nc * 16 : 0);
    stats->download_bytes = npix * nc * 8 * (restore ? 2 : 1) + nc * 32 + nc * call.lists.longest * 12 + polls * 16;
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
