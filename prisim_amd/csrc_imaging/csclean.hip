// csclean.hip -- Cotton-Schwab CLEAN of a dirty image for gfx950 (include/prisim_csclean.h): minor cycles on one image channel with a
// shift-invariant beam P, major cycles through the residual visibilities Vres with the exact one.  The dirty images -- the first, and
// one per major cycle -- and P are what prisim_dirty_image enqueues (dirty_image.h): enqueue_dirty on Vres, and enqueue_dirty_sums of
// kind PSF over the offsets rot_t (di rho + dj kappa) of the half-plane.  The cycles themselves -- the beam P with the host code that
// builds it, the decision at the start of a cycle (k_csclean_decide, on best_partial(), set_first_peak() and publish_active() of
// clean_kernels.h), the minor cycle and the update of Vres (every phasor by cycles_phasor() of imaging_kernels.h) -- are those of cycle_kernels.h, which prisim_clean_mosaic_cs (moscs.hip)
// runs too; here with PlainFlux (a component's flux is gain times the working image at the pick) and NoBeam (its visibilities carry
// that flux as it is).
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

#include "clean_kernels.h"
#include "cycle_kernels.h"
#include "dirty_image.h"

namespace {

int clean_image_cs(prisim_ctx* ctx, const prisim_csclean_args* a, double* out_residual, double* out_restored, int32_t* out_comp_pixel,
                   double* out_comp_flux, int32_t* out_ncomp, int32_t* out_status, double* out_peak0, double* out_wsum, int32_t* out_ncycles,
                   int32_t* out_cycle_ncomp, double* out_cycle_peak, double* out_psf, double* out_vres, prisim_csclean_stats* stats) {
  if (!ctx) return PRISIM_EINVAL;
  // the entry's own host buffers: declared before the frame, whose stream drains before they go.  The results wait in them until the
  // call is through, as the frame's do
  std::vector<double> h_psf;
  CycleTables tables;
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
  double* d_minor = nullptr;
  double2* d_vres = nullptr;
  CycleState X{};
  CycleBeam cb;
  if (int rc = alloc_cycle_state(ctx, dev, X, nc, max_major)) return rc;
  if (int rc = cb.alloc(call, cp.psf_bytes, half)) return rc;
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
    if (int rc = allow_lds(ctx, k_csclean_minor<true, PlainFlux>, npix * 8)) return rc;

  // ---- the weight sums, P, the first dirty image.  Events: [0] sums [1] P [2] dirty image [3]
  const DirtyImage job = dirty_image_of(v, T, call.su.df, pl, dr.wsum, dr.wtot);
  ImgView vp = v;
  vp.kind = PRISIM_IMAGE_PSF;
  const DirtyImage beam = dirty_image_of(vp, T, call.su.df, pl, dr.wsum, dr.wtot);
  if (int rc = mark(0)) return rc;
  if (int rc = enqueue_weight_sums(ctx, job, s0)) return rc;
  if (int rc = mark(1)) return rc;
  if (int rc = cb.offsets(call, lat, half)) return rc;
  if (int rc = enqueue_dirty_sums(ctx, beam, half, cb.pdd, cb.prow, cb.pavg, s0)) return rc;
  if (int rc = cb.mirror(call, half, full)) return rc;
  if (int rc = mark(2)) return rc;
  if (int rc = enqueue_dirty(ctx, job, Span{0, npix}, dr.dd, dr.rows(), dr.R, s0)) return rc;
  if (int rc = call.init(dr.norm())) return rc;
  if (int rc = launch(ctx, k_csclean_init, dim3((unsigned)((nc + kThreads - 1) / kThreads)), 0, s0, X, (int)nc)) return rc;
  if (int rc = mark(3)) return rc;

  // ---- the cycles: max_major + 1 starts at most, whatever the device says.  Events of a cycle: [4] search and decision [5], then
  // behind the host's read [6] minor [7] model [8] dirty image [9]
  MinorParams MP{};
  MP.R = dr.R; MP.P = cb.P; MP.window = call.d_window; MP.scratch = d_minor;
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
    if (int rc = enqueue_minor(call, MP, PlainFlux{}, in_lds)) return rc;
    if (int rc = mark(7)) return rc;
    if (int rc = launch(ctx, k_csclean_model<NoBeam>, dim3((unsigned)grid_for(ctx, ncube)), 0, s0, MM, NoBeam{})) return rc;
    if (int rc = mark(8)) return rc;
    if (int rc = enqueue_dirty(ctx, job, Span{0, npix}, dr.dd, dr.rows(), dr.R, s0)) return rc;
    if (int rc = mark(9)) return rc;
  }

  // ---- the results
  if (int rc = dr.download_norm(call)) return rc;
  if (int rc = tables.enqueue(call, X, cycles, max_major)) return rc;
  if (out_psf) HIPCHK(ctx, hipMemcpyAsync(h_psf.data(), cb.P, h_psf.size() * 8, hipMemcpyDeviceToHost, s0));
  if (int rc = call.close(dr.R, timed ? be.ev[10] : nullptr, timed ? be.ev[11] : nullptr)) return rc;
  if (int rc = call.gather()) return rc;
  const CleanLists& lists = call.lists;
  if (int rc = tables.check(ctx)) return rc;
  // the residual visibilities go straight to the caller, as the last thing that can fail
  if (out_vres) {
    HIPCHK(ctx, hipMemcpyAsync(out_vres, d_vres, (size_t)ncube * 16, hipMemcpyDeviceToHost, s0));
    HIPCHK(ctx, hipStreamSynchronize(s0));
  }

  call.write();
  dr.write_norm(out_wsum);
  tables.write(lists, out_ncycles, out_cycle_ncomp, out_cycle_peak);
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
