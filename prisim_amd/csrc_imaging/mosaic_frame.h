// mosaic_frame.h -- the host body of a beam-weighted mosaic, which does not depend on how the terms of a snapshot's sum are formed: the
// checks, the plan's refusal, the tables, the beamformers, the weight sums, the buffers of every stream, the chunk loop with the beam
// and the sum of every snapshot, the finish, the host buffers that keep a failed call from writing anything, and the statistics.
// prisim_mosaic_image (mosaic.hip) runs it with mosaic_plan and the fp64 sum of mosaic_kernels.h, prisim_mosaic_image_f32
// (mosaic32.hip) with mosaic32_plan and the fp32 sum of mosaic32_kernels.h: an including file compiles the sum it launches and not the
// other.  What the body does, step by step, is described in mosaic.hip.  Every including file gets its own copy (an unnamed
// namespace); built with -ffp-contract=off.  Not part of the public ABI.
#ifndef PRISIM_MOSAIC_FRAME_H
#define PRISIM_MOSAIC_FRAME_H

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/prisim_mosaic.h"
#include "../csrc_addon/beam_setup.h"
#include "imaging_kernels.h"
#include "mosaic_kernels.h"

namespace {

// plan(npix, nbl, nchan, nt, weight_form, chan_avg, budget_bytes, lds_max, asked, uniform, max_streams): an ImagingPlan, as mosaic_plan
// gives it.  sum(ctx, P, plan, stream): the launch of snapshot P.t of P.count pixels into P.N and P.Q
template <typename PlanFn, typename SumFn>
int mosaic_frame(prisim_ctx* ctx, const prisim_mosaic_args* a, double* out_mosaic, double* out_pb_eff, double* out_num, double* out_den,
                 double* out_wsum, prisim_mosaic_stats* stats, PlanFn plan, SumFn sum) {
  if (!ctx) return PRISIM_EINVAL;
  const WallTime wall0 = wall_now();
  if (!a) return fail(ctx, PRISIM_EINVAL, "the argument struct is NULL");
  if (!out_mosaic) return fail(ctx, PRISIM_EINVAL, "out_mosaic is NULL");
  const ImgView v = imaging_view(*a);
  if (int rc = check_args(ctx, v)) return rc;
  if (int rc = check_mosaic_beam(ctx, *a)) return rc;
  const int64_t npix = a->npix, nbl = a->nbl, nchan = a->nchan, nt = a->nt;
  const bool avg = a->chan_avg != 0;
  ImgSetup su{};
  if (int rc = imaging_preamble(ctx, v, su)) return rc;
  const auto pl = plan(npix, nbl, nchan, nt, a->weight_form, avg, a->budget_bytes, su.lds_max, a->route, su.uniform, kMaxStreams);
  if (pl.refusal) return fail(ctx, PRISIM_EINVAL, plan_refusal(pl));
  const Chunks& ch = pl.chunks;
  const int nstreams = ch.nstreams;

  // the results wait here until every chunk is in: nothing reaches the caller's arrays from a call that fails.  Declared before the
  // streams, so that they outlive every copy in flight on any return path
  const int64_t per_out = avg ? 1 : nchan;
  std::vector<double> h_mos((size_t)(npix * per_out)), h_wsum((size_t)nchan);
  std::vector<double> h_eff(out_pb_eff ? (size_t)(npix * per_out) : 0), h_num(out_num ? (size_t)(npix * nchan) : 0),
      h_den(out_den ? (size_t)(npix * nchan) : 0);
  ImgTables T;

  Work wk;
  Streams& st = wk.st;
  if (int rc = st.create(ctx, nstreams, true)) return rc;
  hipStream_t s0 = st.s[0];

  if (int rc = upload_tables(ctx, wk.dev, v, s0, T)) return rc;
  const ImgWeights& W = T.W;
  int64_t upload = T.bytes;
  double *d_wt = nullptr, *d_wtot = nullptr, *d_wband = nullptr, *d_ones = nullptr, *d_zeros = nullptr;
  // the unit flux of the beam statement: pb * 1 * exp2(0 * lg) = pb
  const std::vector<double> ones((size_t)ch.size, 1.0);
  DEV_UPLOAD(ctx, wk.dev, d_ones, ones, s0);
  DEV_ALLOC(ctx, wk.dev, d_zeros, ch.size * 8);
  HIPCHK(ctx, hipMemsetAsync(d_zeros, 0, (size_t)ch.size * 8, s0));
  upload += ch.size * 8;
  std::vector<const double*> d_bf;
  if (int rc = upload_beamformers(ctx, wk.dev, a->ext, a->n_ext, s0, d_bf, upload)) return rc;
  int32_t* d_flag = nullptr;
  DEV_ALLOC(ctx, wk.dev, d_flag, sizeof(int32_t));
  HIPCHK(ctx, hipMemsetAsync(d_flag, 0, sizeof(int32_t), s0));
  DEV_ALLOC(ctx, wk.dev, d_wt, nt * nchan * 8);
  DEV_ALLOC(ctx, wk.dev, d_wtot, nchan * 8);
  DEV_ALLOC(ctx, wk.dev, d_wband, 8);
  if (int rc = enqueue_mos_wsum(ctx, W, nt, nbl, nchan, d_wt, d_wtot, d_wband, s0)) return rc;

  // per stream: the buffers of one chunk
  double4 *d_s4[kMaxStreams] = {}, *d_dd[kMaxStreams] = {};
  double *d_pb[kMaxStreams] = {}, *d_N[kMaxStreams] = {}, *d_Q[kMaxStreams] = {}, *d_mos[kMaxStreams] = {}, *d_eff[kMaxStreams] = {};
  for (int i = 0; i < nstreams; ++i) {
    DEV_ALLOC(ctx, wk.dev, d_s4[i], ch.size * nt * 32);
    DEV_ALLOC(ctx, wk.dev, d_dd[i], ch.size * nt * 32);
    DEV_ALLOC(ctx, wk.dev, d_pb[i], ch.size * nchan * 8);
    DEV_ALLOC(ctx, wk.dev, d_N[i], ch.size * nchan * 8);
    DEV_ALLOC(ctx, wk.dev, d_Q[i], ch.size * nchan * 8);
    DEV_ALLOC(ctx, wk.dev, d_mos[i], ch.size * per_out * 8);
    DEV_ALLOC(ctx, wk.dev, d_eff[i], ch.size * per_out * 8);
  }
  // the kernels start behind whatever the context's stream still writes into the resident cube
  if (v.resident()) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(s0));              // stream 1 starts behind the uploads and the weight sums; the tables are caller memory

  MosParams base{};
  base.cube = T.cube;
  base.W = W;
  base.bl = T.bl; base.freqs = T.freqs;
  base.df = su.df;
  base.nbl = nbl; base.nchan = (int)nchan;

  auto kernels = [&](int64_t, Span sp, int i, hipStream_t sc) -> int {
    if (int rc = launch(ctx, k_img_dirs, dim3((unsigned)grid_for(ctx, sp.count * nt)), 0, sc, T.uvec, T.frames, sp.first, sp.count, nt, d_s4[i],
                        d_dd[i]))
      return rc;
    for (int64_t t = 0; t < nt; ++t) {
      if (int rc = enqueue_mos_beam(ctx, *a, t, d_bf, d_s4[i] + t * sp.count, sp.count, T.freqs, d_ones, d_zeros, d_flag, d_pb[i], sc)) return rc;
      MosParams P = base;
      P.dd = d_dd[i] + t * sp.count; P.s4 = d_s4[i] + t * sp.count;
      P.pb = d_pb[i]; P.wt = d_wt + t * nchan;
      P.t = t; P.count = sp.count;
      P.N = d_N[i]; P.Q = d_Q[i];
      if (int rc = sum(ctx, P, pl, sc)) return rc;
    }
    return enqueue_mos_finish(ctx, avg, d_N[i], d_Q[i], d_wtot, d_wband, sp.count, nchan, a->pbmin, d_mos[i], d_eff[i], sc);
  };
  auto download = [&](int64_t, Span sp, int i, hipStream_t sc) -> int {
    const size_t out_bytes = (size_t)(sp.count * per_out) * 8, sum_bytes = (size_t)(sp.count * nchan) * 8;
    HIPCHK(ctx, hipMemcpyAsync(h_mos.data() + (size_t)(sp.first * per_out), d_mos[i], out_bytes, hipMemcpyDeviceToHost, sc));
    if (out_pb_eff) HIPCHK(ctx, hipMemcpyAsync(h_eff.data() + (size_t)(sp.first * per_out), d_eff[i], out_bytes, hipMemcpyDeviceToHost, sc));
    if (out_num) HIPCHK(ctx, hipMemcpyAsync(h_num.data() + (size_t)(sp.first * nchan), d_N[i], sum_bytes, hipMemcpyDeviceToHost, sc));
    if (out_den) HIPCHK(ctx, hipMemcpyAsync(h_den.data() + (size_t)(sp.first * nchan), d_Q[i], sum_bytes, hipMemcpyDeviceToHost, sc));
    return PRISIM_OK;
  };
  if (int rc = chunk_loop(ctx, st, ch, npix, no_step, kernels, download)) return rc;
  if (int rc = poly_beam_verdict(ctx, a->beam_kind, d_flag)) return rc;
  HIPCHK(ctx, hipMemcpy(h_wsum.data(), d_wtot, h_wsum.size() * 8, hipMemcpyDeviceToHost));

  std::memcpy(out_mosaic, h_mos.data(), h_mos.size() * 8);
  if (out_pb_eff) std::memcpy(out_pb_eff, h_eff.data(), h_eff.size() * 8);
  if (out_num) std::memcpy(out_num, h_num.data(), h_num.size() * 8);
  if (out_den) std::memcpy(out_den, h_den.data(), h_den.size() * 8);
  if (out_wsum) std::memcpy(out_wsum, h_wsum.data(), h_wsum.size() * 8);
  if (stats) {
    // per snapshot.  The sum, per workgroup (block of pixels, channel tile) and b: the tile's row of the cube (16 B a channel) and
    // of the weights (8 B a channel when there are any), and the baseline (24 B); per pixel and tile its offset and its direction
    // (32 B each); per (pixel, channel) the beam value read (8 B), N and Q written (16 B) and, past snapshot 0, read (16 B).  The
    // beam: 32 B of direction read per pixel, 8 B written per (pixel, channel).  Once: k_img_dirs, 24 B read and 64 B written per
    // (pixel, snapshot); the finish, N and Q read and two outputs written, read once more per channel with chan_avg; k_mos_wsum, the
    // weights once.  The fp32 sum reads the same global bytes: its operand is rounded on the way into LDS.
    const int64_t wg = pl.nblocks * pl.ntiles;
    const int64_t row = pl.tile * (16 + (W.w ? 8 : 0)) + 24;
    stats->wall_ms = wall_ms_since(wall0);
    stats->kernel_ms = st.kernel_ms;
    stats->beam_values = npix * nchan * nt;
    stats->chunks = ch.count;
    stats->chunk_pixels = ch.size;
    stats->pixel_bytes = pl.pixel_bytes;
    stats->kernel_bytes = wg * nt * nbl * row + npix * nt * (24 + 64 + 32 + 64 * pl.ntiles) + npix * nchan * (nt * (8 + 8 + 16) + (nt - 1) * 16) +
                          npix * nchan * 16 + npix * per_out * 16 + (W.w ? nt * nbl * nchan * 8 : 0) + (nt + 2) * nchan * 8;
    stats->upload_bytes = upload;
    stats->download_bytes = (npix * per_out * (out_pb_eff ? 2 : 1) + npix * nchan * ((out_num ? 1 : 0) + (out_den ? 1 : 0)) + nchan) * 8;
    plan_stats(stats, v, pl, nstreams);
  }
  return PRISIM_OK;
}

}  // namespace

#endif  // PRISIM_MOSAIC_FRAME_H
