// mosclean.hip -- CLEAN of the beam-weighted mosaic of the snapshots for gfx950 (include/prisim_mosclean.h, where the mathematics is).
// It joins what this directory already states and restates none of it: the mosaic's sums (mosaic_kernels.h), the bookkeeping of an
// image-space CLEAN with the frame of its call (clean_kernels.h), its update by the tile pass of the direct Fourier sum
// (clean_update.h) and the fused analytic beam (launch_beam_flux by enqueue_mos_beam).  The horizon pass of the beam table and the
// search image are in mosclean_kernels.h, which prisim_clean_mosaic_cs (moscs.hip) runs too.  All pixels are resident; one stream.
//
// Once per call:
//   k_img_dirs, k_mos_wsum   the directions with their offsets, and the weight sums, as prisim_mosaic_image runs them.
//   the beam table           A[nt][npix][nchan]: per snapshot enqueue_mos_beam with unit flux, then k_mosclean_horizon writes 0 where
//                            s_z < 0.  It stays for the whole call: the staging of the update gathers A[t][q_k][k] from it, its epilogue
//                            reads A[t][p][k].
//   k_mos_sum                per snapshot, reading its beam tile from the table: R_N starts as the mosaic's N, and Q is the mosaic's,
//                            bit for bit.  With maxiter = 0 the call is a mosaic.
// Per iteration, three steps that never wait for the host:
//   k_mosclean_flat          the search image F = R_N / sqrt(Q Wtot) under the mask (NaN outside it), [npix][nc]; with chan_avg the
//                            band sums over k ascending.  Bound by device memory: 24 B read a (pixel, channel), 8 B written.
//   k_imclean_peak1, k_imclean_peak2   of clean_kernels.h, on F as it stands; the flux of a component is gain (R_N / Q) at the pick
//                            (MosaicFlux), the band sums with chan_avg.
//   k_clean_update<., true>  the hot path, of clean_update.h where it is described, in its mosaic form: the tile pass of k_mos_sum, so
//                            its summation order, on the operand (w (a_k A[t][q_k][k])) (cos phi_q, -sin phi_q).  The snapshots are
//                            looped inside the launch: behind each, the thread flushes R_N = fma(-A[t][p][k], acc, R_N) into its own 32
//                            elements and clears its accumulators.
// At the end F of the final R_N once more, k_mos_finish on R_N and Q (the residual in true fluxes, the effective beam) and
// k_imclean_restore on the residual.  No atomics, no sum split over workgroups.  Built with -ffp-contract=off; the fused multiply-adds
// are written as fma().  The results are gathered in host buffers and copied out when the call can no longer fail.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/prisim_mosclean.h"
#include "../csrc_addon/beam_setup.h"
#include "../csrc_addon/mosclean_plan.h"
#include "clean_update.h"
#include "mosclean_kernels.h"

namespace {

// the flux of prisim_clean_mosaic: the mosaic value at the pick, from R_N and Q themselves
struct MosaicFlux {
  const double *N, *Q;      // [npix][nchan]
  int nchan, avg;
  __device__ __forceinline__ double operator()(int32_t p, int k) const {
    const int64_t at = (int64_t)p * nchan;
    if (!avg) return N[at + k] / Q[at + k];
    double n = 0.0, q = 0.0;
    for (int c = 0; c < nchan; ++c) {
      n += N[at + c];
      q += Q[at + c];
    }
    return n / q;
  }
};

int clean_mosaic(prisim_ctx* ctx, const prisim_mosclean_args* a, double* out_residual, double* out_restored, double* out_residual_flat,
                 double* out_pb_eff, double* out_num, double* out_den, double* out_wsum, int32_t* out_comp_pixel, double* out_comp_flux,
                 int32_t* out_ncomp, int32_t* out_status, double* out_peak0, prisim_mosclean_stats* stats) {
  if (!ctx) return PRISIM_EINVAL;
  // the entry's own host buffers and the loop's poll: declared before the frame, whose stream drains before they go.  The results wait
  // in them until the call is through, as the frame's do
  std::vector<double> h_flat, h_eff, h_num, h_den, h_wsum, ones;
  CleanLoop loop;
  CleanCall call(ctx, {out_residual, out_restored, out_comp_pixel, out_comp_flux, out_ncomp, out_status, out_peak0}, stats != nullptr);
  if (int rc = call.check_outputs(a)) return rc;
  if (int rc = call.check_inputs(*a, [&] { return check_mosaic_beam(ctx, *a); })) return rc;
  const int64_t npix = a->npix, nbl = a->nbl, nchan = a->nchan, nt = a->nt, nc = call.nc;
  const bool avg = call.avg, restore = call.restore;
  const MoscleanPlan pl = mosclean_plan(npix, nbl, nchan, nt, avg, a->maxiter, a->budget_bytes, call.su.lds_max, a->route, call.su.uniform);
  if (pl.refusal) return fail(ctx, PRISIM_EINVAL, clean_refusal(pl.refusal, pl.total, "the workgroup", pl.lds));
  const ImcleanPlan& cp = pl.clean;
  const bool stepped = cp.route == kImagingStepped;

  const size_t nimg = (size_t)(npix * nc), nsum = (size_t)(npix * nchan);
  h_flat.resize(out_residual_flat ? nimg : 0); h_eff.resize(out_pb_eff ? nimg : 0);
  h_num.resize(out_num ? nsum : 0); h_den.resize(out_den ? nsum : 0);
  h_wsum.resize((size_t)nchan);

  if (int rc = call.open(cp)) return rc;
  hipStream_t s0 = call.s0;
  Dev& dev = call.wk.dev;
  const ImgTables& T = call.T;
  const ImgWeights& W = T.W;
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

  // the resident buffers of the plan
  double4 *d_s4 = nullptr, *d_dd = nullptr;
  double *d_A = nullptr, *d_N = nullptr, *d_Q = nullptr, *d_F = nullptr, *d_res = nullptr, *d_eff = nullptr, *d_wt = nullptr, *d_wtot = nullptr,
         *d_wband = nullptr;
  DEV_ALLOC(ctx, dev, d_s4, pl.dirs_bytes / 2);
  DEV_ALLOC(ctx, dev, d_dd, pl.dirs_bytes / 2);
  DEV_ALLOC(ctx, dev, d_A, pl.beam_bytes);
  DEV_ALLOC(ctx, dev, d_N, pl.sums_bytes / 2);
  DEV_ALLOC(ctx, dev, d_Q, pl.sums_bytes / 2);
  DEV_ALLOC(ctx, dev, d_F, pl.flat_bytes);
  DEV_ALLOC(ctx, dev, d_res, pl.out_bytes / 2);
  DEV_ALLOC(ctx, dev, d_eff, pl.out_bytes / 2);
  DEV_ALLOC(ctx, dev, d_wt, nt * nchan * 8);
  DEV_ALLOC(ctx, dev, d_wtot, nchan * 8);
  DEV_ALLOC(ctx, dev, d_wband, 8);
  Events tev;                                           // [0] .. [1] the first residual, [2] .. [3] the finish and the restoration
  if (call.timed)
    if (int rc = tev.create(ctx)) return rc;

  // ---- the first residual: the mosaic's N and Q of all pixels, the beam of every snapshot kept
  if (call.timed) HIPCHK(ctx, hipEventRecord(tev.e[0], s0));
  if (int rc = enqueue_mos_wsum(ctx, W, nt, nbl, nchan, d_wt, d_wtot, d_wband, s0)) return rc;
  if (int rc = launch(ctx, k_img_dirs, dim3((unsigned)grid_for(ctx, npix * nt)), 0, s0, T.uvec, T.frames, (int64_t)0, npix, nt, d_s4, d_dd)) return rc;
  MosParams M{};
  M.cube = T.cube;
  M.W = W;
  M.bl = T.bl; M.freqs = T.freqs;
  M.df = call.su.df;
  M.nbl = nbl; M.nchan = (int)nchan;
  M.count = npix;
  M.N = d_N; M.Q = d_Q;
  for (int64_t t = 0; t < nt; ++t) {
    double* At = d_A + t * npix * nchan;
    if (int rc = enqueue_mos_beam(ctx, *a, t, d_bf, d_s4 + t * npix, npix, T.freqs, d_ones, d_zeros, d_flag, At, s0)) return rc;
    if (int rc = enqueue_mosclean_horizon(ctx, d_s4 + t * npix, npix, nchan, At, s0)) return rc;
    M.dd = d_dd + t * npix; M.s4 = d_s4 + t * npix;
    M.pb = At; M.wt = d_wt + t * nchan;
    M.t = t;
    if (int rc = enqueue_mos_sum(ctx, M, cp.block, cp.ntiles, stepped, s0)) return rc;
  }
  if (int rc = call.init(avg ? d_wband : d_wtot)) return rc;
  if (call.timed) HIPCHK(ctx, hipEventRecord(tev.e[1], s0));

  // ---- the iterations
  const MosaicFlux flux{d_N, d_Q, (int)nchan, avg ? 1 : 0};
  auto flat = [&]() -> int { return enqueue_mosclean_flat(ctx, avg, d_N, d_Q, d_wtot, d_wband, npix, nchan, a->pbmin, d_F, s0); };
  auto search = [&](bool first) -> int {
    if (int rc = flat()) return rc;
    if (int rc = call.search(d_F)) return rc;
    return call.decide(flux, *a, first);
  };
  auto update = [&]() -> int { return enqueue_clean_update<true>(call, d_dd, d_A, d_N); };
  if (int rc = loop.run(call, imclean_batch(a->poll_every), search, update)) return rc;

  // ---- the results: F of the final R_N, the residual in true fluxes under the mask, the effective beam
  if (call.timed) HIPCHK(ctx, hipEventRecord(tev.e[2], s0));
  if (int rc = flat()) return rc;
  if (int rc = enqueue_mos_finish(ctx, avg, d_N, d_Q, d_wtot, d_wband, npix, nchan, a->pbmin, d_res, d_eff, s0)) return rc;
  if (out_residual_flat) HIPCHK(ctx, hipMemcpyAsync(h_flat.data(), d_F, nimg * 8, hipMemcpyDeviceToHost, s0));
  if (out_pb_eff) HIPCHK(ctx, hipMemcpyAsync(h_eff.data(), d_eff, nimg * 8, hipMemcpyDeviceToHost, s0));
  if (out_num) HIPCHK(ctx, hipMemcpyAsync(h_num.data(), d_N, nsum * 8, hipMemcpyDeviceToHost, s0));
  if (out_den) HIPCHK(ctx, hipMemcpyAsync(h_den.data(), d_Q, nsum * 8, hipMemcpyDeviceToHost, s0));
  HIPCHK(ctx, hipMemcpyAsync(h_wsum.data(), d_wtot, (size_t)nchan * 8, hipMemcpyDeviceToHost, s0));
  if (int rc = call.close(d_res, nullptr, nullptr, tev.e[3])) return rc;
  if (int rc = poly_beam_verdict(ctx, a->beam_kind, d_flag)) return rc;
  if (int rc = call.gather()) return rc;

  call.write();
  if (out_residual_flat) std::memcpy(out_residual_flat, h_flat.data(), nimg * 8);
  if (out_pb_eff) std::memcpy(out_pb_eff, h_eff.data(), nimg * 8);
  if (out_num) std::memcpy(out_num, h_num.data(), nsum * 8);
  if (out_den) std::memcpy(out_den, h_den.data(), nsum * 8);
  if (out_wsum) std::memcpy(out_wsum, h_wsum.data(), (size_t)nchan * 8);
  if (stats) {
    // the first residual as prisim_mosaic_image counts its kernels, with the horizon pass (8 B a beam value where it writes, 32 B a
    // pixel read).  An iteration, counted with every channel active: the update reads per workgroup and (t, b) the tile's weights
    // (8 B a channel when there are any), the pick's offsets (32 B a channel) and the baseline twice (24 B), per pixel and snapshot its
    // offsets (32 B per tile), per (pixel, channel, snapshot) the beam (8 B) and R_N read and written (16 B), per workgroup, channel
    // and snapshot the beam at the pick (8 B); the search image reads R_N and Q (16 B) and writes F (8 B per image channel); the peak
    // search reads F and the window and writes and reads the partials.
    const int64_t wg = cp.nblocks * cp.ntiles;
    const int64_t row = cp.tile * (16 + (W.w ? 8 : 0)) + 24;
    const int64_t first_bytes = wg * nt * nbl * row + npix * nt * (24 + 64 + 32 + 32 + 64 * cp.ntiles) +
                                npix * nchan * (nt * (8 + 8 + 8 + 16) + (nt - 1) * 16) + (W.w ? nt * nbl * nchan * 8 : 0) + (nt + 2) * nchan * 8;
    const int64_t iter_bytes = wg * nt * (nbl * (cp.tile * (32 + (W.w ? 8 : 0)) + 48) + cp.tile * 8) + npix * nt * 32 * cp.ntiles +
                               npix * nchan * nt * 24 + npix * nchan * 16 + npix * nc * 16 + (a->window ? npix : 0) + cp.nslabs * nc * 32;
    const double mosaic_ms = elapsed_ms(tev.e[0], tev.e[1]), restore_ms = elapsed_ms(tev.e[2], tev.e[3]);
    call.common_stats(stats, pl.total);
    stats->lds_bytes = (int32_t)pl.lds;                 // of the mosaic's workgroup, which stages a_k A as well
    stats->kernel_ms = mosaic_ms + loop.peak_ms + loop.update_ms + restore_ms;
    stats->mosaic_ms = mosaic_ms;
    stats->peak_ms = loop.peak_ms;
    stats->update_ms = loop.update_ms;
    stats->restore_ms = restore_ms;
    stats->beam_values = npix * nchan * nt;
    stats->iterations = loop.counts[1];
    stats->polls = loop.polls;
    stats->chunks = 1;
    stats->chunk_pixels = npix;
    stats->kernel_bytes = first_bytes + loop.counts[1] * iter_bytes + npix * nchan * 16 + npix * nc * (8 + 16 + (restore ? 16 : 0));
    stats->download_bytes = (npix * nc * (1 + (restore ? 1 : 0) + (out_residual_flat ? 1 : 0) + (out_pb_eff ? 1 : 0)) +
                             npix * nchan * ((out_num ? 1 : 0) + (out_den ? 1 : 0)) + nchan) * 8 + nc * 16 + nc * call.lists.longest * 12 + loop.polls * 16;
  }
  return PRISIM_OK;
}

}  // namespace

extern "C" {

int prisim_clean_mosaic(prisim_ctx* ctx, const prisim_mosclean_args* a, double* out_residual, double* out_restored, double* out_residual_flat,
                        double* out_pb_eff, double* out_num, double* out_den, double* out_wsum, int32_t* out_comp_pixel,
                        double* out_comp_flux, int32_t* out_ncomp, int32_t* out_status, double* out_peak0, prisim_mosclean_stats* stats) {
  return guarded(ctx, [&]() -> int {
    return clean_mosaic(ctx, a, out_residual, out_restored, out_residual_flat, out_pb_eff, out_num, out_den, out_wsum, out_comp_pixel,
                        out_comp_flux, out_ncomp, out_status, out_peak0, stats);
  });
}

}  // extern "C"
