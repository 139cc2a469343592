// moscs.hip -- Cotton-Schwab CLEAN of the beam-weighted mosaic of the snapshots for gfx950 (include/prisim_moscs.h, where the
// mathematics is).  It joins what this directory already states and restates none of it:
//   the state            the directions, the weight sums, the beam table A[nt][npix][nchan] with its horizon pass, and N and Q by
//                        k_mos_sum per snapshot from the table: as prisim_clean_mosaic (mosclean.hip) forms them, by mosaic_kernels.h
//                        and mosclean_kernels.h, so with maxiter = 0 or max_major = 0 the call is a mosaic bit for bit.
//   the cycles           cycle_kernels.h, as prisim_clean_image_cs (csclean.hip) runs them: P by the PSF pass of the dirty image over
//                        the half-plane of the lattice, the decision at the start of a cycle, the minor cycle with FlatFlux -- the
//                        working image is F, a component loses it gain F[q] and is listed with that times s[q] -- and the update of
//                        Vres with TableBeam, the listed flux times A[t][q][k].
//   the frame            of clean_kernels.h (CleanCall): the checks, the tables, the peak search, the lists, the restoration.
// What is new here is one kernel:
//   k_moscs_scale        s[p][kc] = sqrt(Wc / Qc[p]), once per call: one quotient, one square root; with chan_avg Qc is the band's sum
//                        over k ascending, as k_mosclean_flat_band forms it.
// The mask of the minor cycle is the NaNs of F and nothing else: k_mosclean_flat writes NaN where a pixel is not valid, a NaN stays
// NaN under the update and never wins `v > m.v`, so the minor kernel takes the call's [npix] window as it stands and no per-channel
// mask is built.  A major cycle is k_csclean_model on Vres and then k_mos_sum per snapshot, t ascending, on Vres: R_N is the mosaic's
// numerator of the residual visibilities, Q is written again with the same bits.  One stream; the host reads the 16 bytes of the
// active count once per cycle.  No atomics.  Built with -ffp-contract=off.  The results are gathered in host buffers and copied out
// when the call can no longer fail.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/prisim_moscs.h"
#include "../csrc_addon/beam_setup.h"
#include "../csrc_addon/moscs_plan.h"
#include "cycle_kernels.h"
#include "mosclean_kernels.h"

namespace {

// grid-stride over npix * nc: s = sqrt(Wc / Qc).  Q [npix][nchan]; wtot [nchan]; wband[0] = sum_k wtot[k]
__global__ void __launch_bounds__(kThreads) k_moscs_scale(const double* __restrict__ Q, const double* __restrict__ wtot,
                                                          const double* __restrict__ wband, int64_t npix, int nchan, int avg,
                                                          double* __restrict__ scale) {
  const int nc = avg ? 1 : nchan;
  const int64_t total = npix * nc;
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kThreads) {
    double q, w;
    if (avg) {
      q = 0.0;
      for (int k = 0; k < nchan; ++k) q += Q[e * nchan + k];
      w = wband[0];
    } else {
      q = Q[e];
      w = wtot[e % nchan];
    }
    scale[e] = sqrt(w / q);
  }
}

int clean_mosaic_cs(prisim_ctx* ctx, const prisim_moscs_args* a, double* out_residual, double* out_restored, double* out_residual_flat,
                    double* out_pb_eff, double* out_num, double* out_den, double* out_wsum, int32_t* out_comp_pixel, double* out_comp_flux,
                    int32_t* out_ncomp, int32_t* out_status, double* out_peak0, int32_t* out_ncycles, int32_t* out_cycle_ncomp,
                    double* out_cycle_peak, double* out_psf, double* out_vres, prisim_moscs_stats* stats) {
  if (!ctx) return PRISIM_EINVAL;
  // the entry's own host buffers: declared before the frame, whose stream drains before they go.  The results wait in them until the
  // call is through, as the frame's do
  std::vector<double> h_flat, h_eff, h_num, h_den, h_wsum, h_psf, ones;
  CycleTables tables;
  CleanCall call(ctx, {out_residual, out_restored, out_comp_pixel, out_comp_flux, out_ncomp, out_status, out_peak0}, stats != nullptr);
  if (int rc = call.check_outputs(a)) return rc;
  if (!out_ncycles || !out_cycle_ncomp || !out_cycle_peak) return fail(ctx, PRISIM_EINVAL, "out_ncycles, out_cycle_ncomp or out_cycle_peak is NULL");
  if (int rc = call.check_inputs(*a, [&] { return check_mosaic_beam(ctx, *a); })) return rc;
  const ImgView& v = call.v;
  const int64_t npix = a->npix, nbl = a->nbl, nchan = a->nchan, nt = a->nt, maxiter = a->maxiter, ny = a->ny, nx = a->nx, nc = call.nc;
  const bool avg = call.avg, restore = call.restore, timed = call.timed;
  const MoscsPlan pl = moscs_plan(npix, ny, nx, nbl, nchan, nt, avg, maxiter, a->cycle_depth, a->max_major, a->budget_bytes, call.su.lds_max,
                                  a->route, call.su.uniform, a->minor_route);
  if (pl.refusal) return fail(ctx, PRISIM_EINVAL, clean_refusal(pl.refusal, pl.total, "the workgroup of a minor cycle", pl.cyc.minor_lds));
  const ImcleanPlan& cp = pl.mos.clean;
  const bool stepped = cp.route == kImagingStepped, in_lds = pl.cyc.minor_route == kCscleanLds;
  const int max_major = a->max_major;
  const int64_t half = pl.cyc.psf_half, full = pl.cyc.psf_full, ncube = nt * nbl * nchan;
  const Lattice lat = lattice_of(a->unitvec, ny, nx);

  const size_t nimg = (size_t)(npix * nc), nsum = (size_t)(npix * nchan);
  h_flat.resize(out_residual_flat ? nimg : 0); h_eff.resize(out_pb_eff ? nimg : 0);
  h_num.resize(out_num ? nsum : 0); h_den.resize(out_den ? nsum : 0);
  h_wsum.resize((size_t)nchan);
  h_psf.resize(out_psf ? (size_t)(nc * full) : 0);

  if (int rc = call.open(cp)) return rc;
  hipStream_t s0 = call.s0;
  Dev& dev = call.wk.dev;
  ImgTables& T = call.T;
  const ImgWeights& W = T.W;
  const CleanState& S = call.S;
  double *d_ones = nullptr, *d_zeros = nullptr;
  // the unit flux of the beam statement: pb * 1 * exp2(0 * lg) = pb
  ones.assign((size_t)npix, 1.0);
  DEV_UPLOAD(ctx, dev, d_ones, ones, s0);
  DEV_ALLOC(ctx, dev, d_zeros, npix * 8);
  HIPCHK(ctx, hipMemsetAsync(d_zeros, 0, (size_t)npix * 8, s0));
  call.upload += npix * 8;
  std::vector<const double*> d_bf;
  if (int rc = upload_beamformers(ctx, dev, a->ext, a->n_ext, s0, d_bf, call.upload)) return rc;
  int32_t* d_flag = nullptr;
  DEV_ALLOC(ctx, dev, d_flag, sizeof(int32_t));
  HIPCHK(ctx, hipMemsetAsync(d_flag, 0, sizeof(int32_t), s0));

  // the resident buffers of the plan: those of prisim_clean_mosaic, then those of the cycles
  double4 *d_s4 = nullptr, *d_dd = nullptr;
  double *d_A = nullptr, *d_N = nullptr, *d_Q = nullptr, *d_F = nullptr, *d_res = nullptr, *d_eff = nullptr, *d_wt = nullptr, *d_wtot = nullptr,
         *d_wband = nullptr, *d_pw = nullptr, *d_pwtot = nullptr, *d_scale = nullptr, *d_minor = nullptr;
  double2* d_vres = nullptr;
  DEV_ALLOC(ctx, dev, d_s4, pl.mos.dirs_bytes / 2);
  DEV_ALLOC(ctx, dev, d_dd, pl.mos.dirs_bytes / 2);
  DEV_ALLOC(ctx, dev, d_A, pl.mos.beam_bytes);
  DEV_ALLOC(ctx, dev, d_N, pl.mos.sums_bytes / 2);
  DEV_ALLOC(ctx, dev, d_Q, pl.mos.sums_bytes / 2);
  DEV_ALLOC(ctx, dev, d_F, pl.mos.flat_bytes);
  DEV_ALLOC(ctx, dev, d_res, pl.mos.out_bytes / 2);
  DEV_ALLOC(ctx, dev, d_eff, pl.mos.out_bytes / 2);
  DEV_ALLOC(ctx, dev, d_wt, nt * nchan * 8);
  DEV_ALLOC(ctx, dev, d_wtot, nchan * 8);
  DEV_ALLOC(ctx, dev, d_wband, 8);
  DEV_ALLOC(ctx, dev, d_pw, nchan * 8);
  DEV_ALLOC(ctx, dev, d_pwtot, 8);
  DEV_ALLOC(ctx, dev, d_scale, pl.scale_bytes);
  CycleState X{};
  CycleBeam cb;
  if (int rc = alloc_cycle_state(ctx, dev, X, nc, max_major)) return rc;
  if (int rc = cb.alloc(call, pl.cyc.psf_bytes, half)) return rc;
  if (!in_lds) DEV_ALLOC(ctx, dev, d_minor, pl.cyc.minor_bytes);

  // Vres: the uploaded cube is the call's own; the resident one is copied, behind what the context's stream wrote into it (open)
  if (v.resident()) {
    DEV_ALLOC(ctx, dev, d_vres, pl.cyc.vres_bytes);
    HIPCHK(ctx, hipMemcpyAsync(d_vres, ctx->cube.p, (size_t)ncube * 16, hipMemcpyDeviceToDevice, s0));
    T.cube = d_vres;
  } else {
    d_vres = const_cast<double2*>(T.cube);
  }
  if (in_lds)
    if (int rc = allow_lds(ctx, k_csclean_minor<true, FlatFlux>, npix * 8)) return rc;
  BatchEvents be;
  if (timed)
    if (int rc = be.create(ctx, 14)) return rc;
  auto mark = [&](int i) -> int {
    if (timed) HIPCHK(ctx, hipEventRecord(be.ev[(size_t)i], s0));
    return PRISIM_OK;
  };
  auto span_ms = [&](int i, int j) { return timed ? elapsed_ms(be.ev[(size_t)i], be.ev[(size_t)j]) : 0.0; };

  // ---- once per call.  Events: [0] weight sums, directions [1] beam table [2] P [3] the first mosaic pass [4] scale, state [5]
  MosParams M{};
  M.cube = d_vres;
  M.W = W;
  M.bl = T.bl; M.freqs = T.freqs;
  M.df = call.su.df;
  M.nbl = nbl; M.nchan = (int)nchan;
  M.count = npix;
  M.N = d_N; M.Q = d_Q;
  // R_N = the mosaic's numerator of Vres as it stands, per snapshot from the beam table; Q comes out with the same bits each time
  auto mosaic_pass = [&]() -> int {
    for (int64_t t = 0; t < nt; ++t) {
      M.dd = d_dd + t * npix; M.s4 = d_s4 + t * npix;
      M.pb = d_A + t * npix * nchan; M.wt = d_wt + t * nchan;
      M.t = t;
      if (int rc = enqueue_mos_sum(ctx, M, cp.block, cp.ntiles, stepped, s0)) return rc;
    }
    return PRISIM_OK;
  };
  if (int rc = mark(0)) return rc;
  if (int rc = enqueue_mos_wsum(ctx, W, nt, nbl, nchan, d_wt, d_wtot, d_wband, s0)) return rc;
  if (int rc = launch(ctx, k_img_dirs, dim3((unsigned)grid_for(ctx, npix * nt)), 0, s0, T.uvec, T.frames, (int64_t)0, npix, nt, d_s4, d_dd)) return rc;
  if (int rc = mark(1)) return rc;
  for (int64_t t = 0; t < nt; ++t) {
    double* At = d_A + t * npix * nchan;
    if (int rc = enqueue_mos_beam(ctx, *a, t, d_bf, d_s4 + t * npix, npix, T.freqs, d_ones, d_zeros, d_flag, At, s0)) return rc;
    if (int rc = enqueue_mosclean_horizon(ctx, d_s4 + t * npix, npix, nchan, At, s0)) return rc;
  }
  if (int rc = mark(2)) return rc;
  ImgView vp = v;
  vp.kind = PRISIM_IMAGE_PSF;
  const DirtyImage beam = dirty_image_of(vp, T, call.su.df, cp, d_pw, d_pwtot);
  if (int rc = enqueue_weight_sums(ctx, beam, s0)) return rc;
  if (int rc = cb.offsets(call, lat, half)) return rc;
  if (int rc = enqueue_dirty_sums(ctx, beam, half, cb.pdd, cb.prow, cb.pavg, s0)) return rc;
  if (int rc = cb.mirror(call, half, full)) return rc;
  if (int rc = mark(3)) return rc;
  if (int rc = mosaic_pass()) return rc;
  if (int rc = mark(4)) return rc;
  if (int rc = launch(ctx, k_moscs_scale, dim3((unsigned)grid_for(ctx, npix * nc)), 0, s0, (const double*)d_Q, (const double*)d_wtot,
                      (const double*)d_wband, npix, (int)nchan, avg ? 1 : 0, d_scale))
    return rc;
  if (int rc = call.init(avg ? d_wband : d_wtot)) return rc;
  if (int rc = launch(ctx, k_csclean_init, dim3((unsigned)((nc + kThreads - 1) / kThreads)), 0, s0, X, (int)nc)) return rc;
  if (int rc = mark(5)) return rc;

  // ---- the cycles: max_major + 1 starts at most, whatever the device says.  Events of a cycle: [6] search image, search and decision
  // [7], then behind the host's read [8] minor [9] model [10] mosaic pass [11]
  auto flat = [&]() -> int { return enqueue_mosclean_flat(ctx, avg, d_N, d_Q, d_wtot, d_wband, npix, nchan, a->pbmin, d_F, s0); };
  MinorParams MP{};
  MP.R = d_F; MP.P = cb.P; MP.window = call.d_window; MP.scratch = d_minor;
  MP.S = S; MP.X = X;
  MP.maxiter = maxiter; MP.cycle_niter = a->cycle_niter; MP.gain = a->gain;
  MP.npix = (int)npix; MP.nc = (int)nc; MP.ny = (int)ny; MP.nx = (int)nx; MP.max_major = max_major;
  const FlatFlux flux{d_scale, (int)nc};
  ModelParams MM{};
  MM.V = d_vres; MM.bl = T.bl; MM.freqs = T.freqs; MM.dd = d_dd;
  MM.S = S; MM.X = X;
  MM.nt = nt; MM.nbl = nbl; MM.npix = npix; MM.maxiter = maxiter;
  MM.nchan = (int)nchan; MM.avg = avg ? 1 : 0;
  const TableBeam table{d_A, npix, (int)nchan};
  double mosaic_ms = 0.0, peak_ms = 0.0, minor_ms = 0.0, model_ms = 0.0;
  int64_t active[2] = {0, 0}, polls = 0, cycles = 0;   // what a poll reads: the channels that go on, the cycles in which any did
  for (int c = 0; c <= max_major; ++c) {
    if (int rc = mark(6)) return rc;
    if (int rc = flat()) return rc;
    if (int rc = call.search(d_F)) return rc;
    if (int rc = launch(ctx, k_csclean_decide, dim3(1), 0, s0, S, X, (const Peak*)call.d_partial, (int)nc, cp.nslabs, maxiter, a->threshold,
                        (int)a->threshold_relative, a->cycle_depth, c, max_major))
      return rc;
    if (int rc = mark(7)) return rc;
    HIPCHK(ctx, hipMemcpyAsync(active, S.counts, 16, hipMemcpyDeviceToHost, s0));
    HIPCHK(ctx, hipStreamSynchronize(s0));
    ++polls;
    peak_ms += span_ms(6, 7);
    if (c > 0) {
      minor_ms += span_ms(8, 9);
      model_ms += span_ms(9, 10);
      mosaic_ms += span_ms(10, 11);
    }
    if (active[0] <= 0) break;
    if (c == max_major) return fail(ctx, PRISIM_EINTERNAL, "channels still active after max_major cycles");
    ++cycles;
    if (int rc = mark(8)) return rc;
    if (int rc = enqueue_minor(call, MP, flux, in_lds)) return rc;
    if (int rc = mark(9)) return rc;
    if (int rc = launch(ctx, k_csclean_model<TableBeam>, dim3((unsigned)grid_for(ctx, ncube)), 0, s0, MM, table)) return rc;
    if (int rc = mark(10)) return rc;
    if (int rc = mosaic_pass()) return rc;
    if (int rc = mark(11)) return rc;
  }

  // ---- the results: F of the final R_N (the last cycle's, where no cycle followed it), the residual in true fluxes under the mask,
  // the effective beam.  Events: [12] .. [13]
  if (int rc = mark(12)) return rc;
  if (int rc = flat()) return rc;
  if (int rc = enqueue_mos_finish(ctx, avg, d_N, d_Q, d_wtot, d_wband, npix, nchan, a->pbmin, d_res, d_eff, s0)) return rc;
  if (out_residual_flat) HIPCHK(ctx, hipMemcpyAsync(h_flat.data(), d_F, nimg * 8, hipMemcpyDeviceToHost, s0));
  if (out_pb_eff) HIPCHK(ctx, hipMemcpyAsync(h_eff.data(), d_eff, nimg * 8, hipMemcpyDeviceToHost, s0));
  if (out_num) HIPCHK(ctx, hipMemcpyAsync(h_num.data(), d_N, nsum * 8, hipMemcpyDeviceToHost, s0));
  if (out_den) HIPCHK(ctx, hipMemcpyAsync(h_den.data(), d_Q, nsum * 8, hipMemcpyDeviceToHost, s0));
  HIPCHK(ctx, hipMemcpyAsync(h_wsum.data(), d_wtot, (size_t)nchan * 8, hipMemcpyDeviceToHost, s0));
  if (int rc = tables.enqueue(call, X, cycles, max_major)) return rc;
  if (out_psf) HIPCHK(ctx, hipMemcpyAsync(h_psf.data(), cb.P, h_psf.size() * 8, hipMemcpyDeviceToHost, s0));
  if (int rc = call.close(d_res, nullptr, nullptr, timed ? be.ev[13] : nullptr)) return rc;
  if (int rc = poly_beam_verdict(ctx, a->beam_kind, d_flag)) return rc;
  if (int rc = call.gather()) return rc;
  if (int rc = tables.check(ctx)) return rc;
  // the residual visibilities go straight to the caller, as the last thing that can fail
  if (out_vres) {
    HIPCHK(ctx, hipMemcpyAsync(out_vres, d_vres, (size_t)ncube * 16, hipMemcpyDeviceToHost, s0));
    HIPCHK(ctx, hipStreamSynchronize(s0));
  }

  call.write();
  if (out_residual_flat) std::memcpy(out_residual_flat, h_flat.data(), nimg * 8);
  if (out_pb_eff) std::memcpy(out_pb_eff, h_eff.data(), nimg * 8);
  if (out_num) std::memcpy(out_num, h_num.data(), nsum * 8);
  if (out_den) std::memcpy(out_den, h_den.data(), nsum * 8);
  if (out_wsum) std::memcpy(out_wsum, h_wsum.data(), (size_t)nchan * 8);
  tables.write(call.lists, out_ncycles, out_cycle_ncomp, out_cycle_peak);
  if (out_psf) std::memcpy(out_psf, h_psf.data(), h_psf.size() * 8);
  if (stats) {
    const double psf_ms = span_ms(2, 3), beam_ms = span_ms(1, 2) + span_ms(4, 5), restore_ms = span_ms(12, 13);
    mosaic_ms += span_ms(0, 1) + span_ms(3, 4);
    call.common_stats(stats, pl.total);
    stats->lds_bytes = (int32_t)pl.mos.lds;             // of the mosaic's workgroup, as prisim_clean_mosaic reports it
    stats->kernel_ms = psf_ms + beam_ms + mosaic_ms + peak_ms + minor_ms + model_ms + restore_ms;
    stats->psf_ms = psf_ms;
    stats->beam_ms = beam_ms;
    stats->mosaic_ms = mosaic_ms;
    stats->peak_ms = peak_ms;
    stats->minor_ms = minor_ms;
    stats->model_ms = model_ms;
    stats->restore_ms = restore_ms;
    stats->cycles = cycles;
    stats->polls = polls;
    stats->psf_offsets = half;
    stats->download_bytes = (npix * nc * (1 + (restore ? 1 : 0) + (out_residual_flat ? 1 : 0) + (out_pb_eff ? 1 : 0)) +
                             npix * nchan * ((out_num ? 1 : 0) + (out_den ? 1 : 0)) + nchan) * 8 + nc * 20 + nc * call.lists.longest * 12 +
                            nc * (2 * cycles + 1) * 12 + polls * 16 + (out_psf ? nc * full * 8 : 0) + (out_vres ? ncube * 16 : 0);
    stats->minor_route = pl.cyc.minor_route;
    stats->minor_lds_bytes = (int32_t)pl.cyc.minor_lds;
  }
  return PRISIM_OK;
}

}  // namespace

extern "C" {

int prisim_clean_mosaic_cs(prisim_ctx* ctx, const prisim_moscs_args* a, double* out_residual, double* out_restored, double* out_residual_flat,
                           double* out_pb_eff, double* out_num, double* out_den, double* out_wsum, int32_t* out_comp_pixel,
                           double* out_comp_flux, int32_t* out_ncomp, int32_t* out_status, double* out_peak0, int32_t* out_ncycles,
                           int32_t* out_cycle_ncomp, double* out_cycle_peak, double* out_psf, double* out_vres, prisim_moscs_stats* stats) {
  return guarded(ctx, [&]() -> int {
    return clean_mosaic_cs(ctx, a, out_residual, out_restored, out_residual_flat, out_pb_eff, out_num, out_den, out_wsum, out_comp_pixel,
                           out_comp_flux, out_ncomp, out_status, out_peak0, out_ncycles, out_cycle_ncomp, out_cycle_peak, out_psf, out_vres,
                           stats);
  });
}

}  // extern "C"
