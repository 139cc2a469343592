// antpower.hip -- the power an antenna receives from the sky for gfx950 (include/prisim_antpower.h): prisim/interferometry.py
// antenna_power (:2169-2408), power[t][f] = sum_s pb(s, f) S_s(f) / sum_s pb(s, f) over the sources above the horizon, without an
// nsrc x nchan array ever leaving the device.
//
// Per (snapshot t, span of sources), a span being a contiguous range of catalogue indices and a whole number of blocks of SB sources:
//   k_ap_dirs    dirs[s] = (l, m, n, 0) = normalise(R_t (u_s + beta_t)) for every source of the span, the statement of cat_source
//                (../csrc/catalog_kernels.hip) operation by operation.  Sources below the horizon keep their row: nothing is compacted,
//                so the order of the sums never depends on the sky.  One workgroup per block; it also counts its sources with n >= 0.
//   launch_beam_flux (../csrc/aux_kernels.hip) with unit flux (flux_ref = 1, spindex = 0: pb exp2(0) = pb exactly) into the span's own
//                pb_tile[span][nchan].  The beam statement is reused by calling it, not by copying it.
//   k_ap_reduce  the hot path.  A workgroup owns one block of SB consecutive catalogue sources and a tile of channels; a thread owns one
//                channel and one of L source lanes, forms log2(f / ref_freq) once and walks the sources lane, lane + L, ... of the block
//                in ascending order: num += pb * S and den += pb where dirs[s].z >= 0, S from the table or flux_ref exp2(spindex lg)
//                (the statement of aux_kernels.hip).  It loads eight sources ahead of its sums, rows below the horizon included.
//                The L lanes are summed through LDS in lane order and the workgroup writes part[block][2][nchan].  No atomics.
// Per snapshot, behind its last span:
//   k_ap_finish  sums part over the blocks in ascending order, divides (IEEE: 0 / 0 = NaN) and writes the three output rows.
// SB, L and the tile come from (nsrc, nchan) alone (../csrc_addon/antpower_plan.h); the budget and the streams decide only the span
// and how many snapshots are in flight, so the outputs are bit-identical for any budget.  Snapshots alternate between two streams, each
// with its own dirs, pb_tile and part.  fp64 throughout, built with -ffp-contract=off: every product and sum rounds once.
//
// Cost, stated: going through pb_tile writes 8 B and reads 8 B per (source, channel) beside the 8 B of a tabulated spectrum; a
// reduction that evaluated the beam itself would read the 8 B alone, but needs the beam statement in a header of ../csrc, whose sources
// are pinned by the profile manifest.  And the beam is evaluated below the horizon too (up to 2x) for the fixed order; the stats carry
// sources_evaluated and sources_up.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/prisim_antpower.h"
#include "../csrc_addon/addon_internal.h"
#include "../csrc_addon/antpower_plan.h"
#include "../csrc_addon/beam_setup.h"

namespace {

static_assert(kAntpowerThreads == kThreads, "the reduction runs in the add-ons' workgroup");
static_assert(kAntpowerBlock == kThreads, "k_ap_dirs gives one thread to every source of a block");

struct ApFrame { double rot[9], beta[3]; };

// grid: x = block of the span.  dirs [count][4]; up[b0 + blockIdx.x] = sources of the block with n >= 0
__global__ void __launch_bounds__(kThreads) k_ap_dirs(const double* __restrict__ uvec, int64_t s0, int64_t count, ApFrame fr,
                                                      double4* __restrict__ dirs, int32_t* __restrict__ up, int64_t b0) {
  const int64_t sl = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  bool above = false;
  if (sl < count) {
    const double* u = uvec + (s0 + sl) * 3;
    const double t0 = u[0] + fr.beta[0], t1 = u[1] + fr.beta[1], t2 = u[2] + fr.beta[2];
    const double v0 = (fr.rot[0] * t0 + fr.rot[1] * t1) + fr.rot[2] * t2;
    const double v1 = (fr.rot[3] * t0 + fr.rot[4] * t1) + fr.rot[5] * t2;
    const double v2 = (fr.rot[6] * t0 + fr.rot[7] * t1) + fr.rot[8] * t2;
    const double nrm = sqrt((v0 * v0 + v1 * v1) + v2 * v2);
    const double n = v2 / nrm;
    dirs[sl] = make_double4(v0 / nrm, v1 / nrm, n, 0.0);
    above = n >= 0.0;
  }
  const int c = __syncthreads_count(above ? 1 : 0);
  if (threadIdx.x == 0) up[b0 + blockIdx.x] = c;
}

constexpr int kApBatch = 8;      // sources a thread of k_ap_reduce loads ahead of its sums

struct ApReduceParams {
  const double* dirs;       // [count][4] of the span
  const double* pb;         // [count][nchan] of the span
  const double* flux_ref;   // [nsrc] catalogue order; the power law, or
  const double* spindex;    // [nsrc]
  const double* spec;       // [nsrc][nchan]: non-null replaces the power law
  const double* freqs;      // [nchan]
  double ref_freq;
  int64_t s0, count, b0;    // the span: its first source, its sources, its first block (s0 / SB)
  int nchan, tile, lanes;
  double* part;             // [nblocks][2][nchan] of the snapshot
};

// grid: x = block of the span, y = channel tile.  LDS: [lanes][tile] (num, den)
__global__ void __launch_bounds__(kThreads) k_ap_reduce(ApReduceParams P) {
  __shared__ double2 sh[kThreads];
  const int c = threadIdx.x % P.tile, lane = threadIdx.x / P.tile;
  const int f = (int)blockIdx.y * P.tile + c;
  const bool valid = f < P.nchan;
  const int64_t lo = (int64_t)blockIdx.x * kAntpowerBlock, hi = lo + kAntpowerBlock < P.count ? lo + kAntpowerBlock : P.count;
  double num = 0.0, den = 0.0;
  if (valid) {
    const double lg_fr = P.spec ? 0.0 : log2(P.freqs[f] / P.ref_freq);
    // kApBatch sources of the lane at a time: their loads are issued together, for every row (a row below the horizon holds a beam
    // value too), and then added in ascending order where z >= 0 -- the order of a plain loop, without a load waiting on a branch
    for (int64_t base = lo + lane; base < hi; base += (int64_t)P.lanes * kApBatch) {
      double z[kApBatch], pb[kApBatch], a[kApBatch], b[kApBatch];
#pragma unroll
      for (int j = 0; j < kApBatch; ++j) {
        const int64_t sl = base + (int64_t)j * P.lanes;
        const int64_t q = sl < hi ? sl : base;            // past the block: a row of it, not added
        const int64_t s = P.s0 + q;
        z[j] = sl < hi ? P.dirs[q * 4 + 2] : -1.0;
        pb[j] = P.pb[q * P.nchan + f];
        a[j] = P.spec ? P.spec[s * P.nchan + f] : P.flux_ref[s];
        b[j] = P.spec ? 0.0 : P.spindex[s];
      }
#pragma unroll
      for (int j = 0; j < kApBatch; ++j) {
        if (!(z[j] >= 0.0)) continue;
        const double S = P.spec ? a[j] : a[j] * exp2(b[j] * lg_fr);
        num += pb[j] * S;
        den += pb[j];
      }
    }
  }
  sh[threadIdx.x] = make_double2(num, den);
  __syncthreads();
  if (lane == 0 && valid) {
    for (int l = 1; l < P.lanes; ++l) {
      const double2 o = sh[l * P.tile + c];
      num += o.x;
      den += o.y;
    }
    double* row = P.part + (P.b0 + blockIdx.x) * 2 * (int64_t)P.nchan;
    row[f] = num;
    row[P.nchan + f] = den;
  }
}

// grid: x over the channels.  Row t of out_power / out_num / out_den [nsnap][nchan]; workgroup 0 also sums the blocks' counts
__global__ void __launch_bounds__(kThreads) k_ap_finish(const double* __restrict__ part, const int32_t* __restrict__ up, int64_t nblocks,
                                                        int nchan, double* __restrict__ power, double* __restrict__ onum,
                                                        double* __restrict__ oden, int64_t* __restrict__ up_total) {
  __shared__ long long cnt[kThreads];
  const int f = (int)blockIdx.x * kThreads + threadIdx.x;
  if (f < nchan) {
    double num = 0.0, den = 0.0;
#pragma unroll 8
    for (int64_t b = 0; b < nblocks; ++b) {
      num += part[b * 2 * nchan + f];
      den += part[(b * 2 + 1) * nchan + f];
    }
    power[f] = num / den;
    onum[f] = num;
    oden[f] = den;
  }
  if (blockIdx.x != 0) return;
  long long n = 0;
  for (int64_t b = threadIdx.x; b < nblocks; b += kThreads) n += up[b];
  cnt[threadIdx.x] = n;
  __syncthreads();
  for (int h = kThreads / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) cnt[threadIdx.x] += cnt[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) *up_total = cnt[0];
}

int check_args(prisim_ctx* ctx, const prisim_antpower_args* a, const double* out_power) {
  if (!a) return fail(ctx, PRISIM_EINVAL, "the argument struct is NULL");
  if (!out_power) return fail(ctx, PRISIM_EINVAL, "out_power is NULL");
  if (!a->unitvec) return fail(ctx, PRISIM_EINVAL, "unitvec is NULL");
  if (!a->freqs_hz) return fail(ctx, PRISIM_EINVAL, "freqs_hz is NULL");
  if (!a->cel2enu) return fail(ctx, PRISIM_EINVAL, "cel2enu is NULL");
  if (a->nsrc < 1 || a->nchan < 1 || a->nsnap < 1) return fail(ctx, PRISIM_EINVAL, "need nsrc, nchan and nsnap >= 1");
  if (a->nchan > (int64_t)1 << 20) return fail(ctx, PRISIM_EINVAL, "nchan must be at most 2^20");
  if (a->nsrc > ((int64_t)1 << 46) / a->nchan) return fail(ctx, PRISIM_EINVAL, "nsrc * nchan must be at most 2^46");
  if (a->nsnap > (int64_t)1 << 30) return fail(ctx, PRISIM_EINVAL, "nsnap must be at most 2^30");
  const bool table = a->flux_spectrum != nullptr;
  if (!table && (!a->flux_ref || !a->spindex))
    return fail(ctx, PRISIM_EINVAL, "neither a power law (flux_ref and spindex) nor a flux_spectrum is given");
  if (!table && !(a->ref_freq_hz > 0.0 && std::isfinite(a->ref_freq_hz))) return fail(ctx, PRISIM_EINVAL, "ref_freq_hz must be positive with a power law");
  for (int64_t f = 0; f < a->nchan; ++f)
    if (!(a->freqs_hz[f] > 0.0) || !std::isfinite(a->freqs_hz[f]))
      return fail(ctx, PRISIM_EINVAL, "freqs_hz[" + std::to_string(f) + "] is not positive and finite");
  for (int64_t s = 0; s < a->nsrc; ++s) {
    const double* u = a->unitvec + s * 3;
    if (!(std::fabs(std::sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]) - 1.0) <= 1e-6))
      return fail(ctx, PRISIM_EINVAL, "unitvec[" + std::to_string(s) + "] does not have unit length (to 1e-6)");
  }
  for (int64_t t = 0; t < a->nsnap; ++t) {
    const double* R = a->cel2enu + t * 9;
    for (int r = 0; r < 3; ++r)
      for (int q = r; q < 3; ++q) {
        double d = 0.0;
        for (int k = 0; k < 3; ++k) d += R[3 * r + k] * R[3 * q + k];
        if (!(std::fabs(d - (r == q ? 1.0 : 0.0)) <= 1e-9))
          return fail(ctx, PRISIM_EINVAL, "cel2enu of snapshot " + std::to_string(t) + " is not a rotation matrix (rows must be orthonormal to 1e-9)");
      }
    if (a->aberr_beta) {
      const double* b = a->aberr_beta + t * 3;
      if (!((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2] < 1e-4))
        return fail(ctx, PRISIM_EINVAL, "aberr_beta of snapshot " + std::to_string(t) + " must be a velocity / c with |beta| < 0.01");
    }
  }
  return check_beams(ctx, a->beam_kind, a->diameter_m, a->beam_pc_dircos, a->ext, a->n_ext, a->nsnap, "nsnap");
}

int antenna_power(prisim_ctx* ctx, const prisim_antpower_args* a, double* out_power, double* out_num, double* out_den,
                  prisim_antpower_stats* stats) {
  if (!ctx) return PRISIM_EINVAL;
  const WallTime wall0 = wall_now();
  if (int rc = check_args(ctx, a, out_power)) return rc;
  const int64_t nsrc = a->nsrc, nchan = a->nchan, nsnap = a->nsnap;
  const bool table = a->flux_spectrum != nullptr;

  // development hook: another size of pb_tile than the planner's constant (tools/antpower_time.py times three)
  int64_t pb_tile_bytes = kAntpowerPbTileBytes;
  if (const char* env = getenv("PRISIM_ANTPOWER_TILE_BYTES")) {
    const long long v = atoll(env);
    if (v > 0) pb_tile_bytes = v;
  }
  const AntpowerPlan pl = antpower_plan(nsrc, nchan, nsnap, a->budget_bytes, pb_tile_bytes, kMaxStreams);
  const AntpowerShape& sh = pl.shape;
  if (!pl.ok)
    return fail(ctx, PRISIM_EINVAL, "budget_bytes cannot hold one block: " + std::to_string(pl.buffer_bytes) + " B for " + std::to_string(sh.block) +
                                        " sources of " + std::to_string(nchan) + " channels and the partial sums of " + std::to_string(sh.nblocks) +
                                        " blocks");
  const int64_t span = pl.spans.size;
  const int nstreams = pl.nstreams;
  HIPCHK(ctx, hipSetDevice(ctx->device));

  Work wk;
  Streams& st = wk.st;
  if (int rc = st.create(ctx, nstreams, true)) return rc;
  hipStream_t s0 = st.s[0];

  // the catalogue and the tables go up once on stream 0, outside the budget
  double *d_uvec = nullptr, *d_fref = nullptr, *d_spix = nullptr, *d_spec = nullptr, *d_freqs = nullptr, *d_ones = nullptr, *d_zeros = nullptr;
  int64_t upload = 0;
  DEV_UPLOAD(ctx, wk.dev, d_uvec, a->unitvec, (size_t)nsrc * 3, s0);
  upload += nsrc * 24;
  if (table) {
    DEV_UPLOAD(ctx, wk.dev, d_spec, a->flux_spectrum, (size_t)(nsrc * nchan), s0);
    upload += nsrc * nchan * 8;
  } else {
    DEV_UPLOAD(ctx, wk.dev, d_fref, a->flux_ref, (size_t)nsrc, s0);
    DEV_UPLOAD(ctx, wk.dev, d_spix, a->spindex, (size_t)nsrc, s0);
    upload += nsrc * 16;
  }
  DEV_UPLOAD(ctx, wk.dev, d_freqs, a->freqs_hz, (size_t)nchan, s0);
  upload += nchan * 8;
  const std::vector<double> ones((size_t)span, 1.0);
  DEV_UPLOAD(ctx, wk.dev, d_ones, ones, s0);
  DEV_ALLOC(ctx, wk.dev, d_zeros, span * 8);
  HIPCHK(ctx, hipMemsetAsync(d_zeros, 0, (size_t)span * 8, s0));
  std::vector<const double*> d_bf;
  if (int rc = upload_beamformers(ctx, wk.dev, a->ext, a->n_ext, s0, d_bf, upload)) return rc;
  int32_t* d_flag = nullptr;
  DEV_ALLOC(ctx, wk.dev, d_flag, sizeof(int32_t));
  HIPCHK(ctx, hipMemsetAsync(d_flag, 0, sizeof(int32_t), s0));

  // per stream: the buffers of one span and the partial sums of one snapshot; the outputs stay on the device until the end
  double4* d_dirs[kMaxStreams] = {};
  double *d_pb[kMaxStreams] = {}, *d_part[kMaxStreams] = {};
  int32_t* d_up[kMaxStreams] = {};
  for (int i = 0; i < nstreams; ++i) {
    DEV_ALLOC(ctx, wk.dev, d_dirs[i], span * kAntpowerDirBytes);
    DEV_ALLOC(ctx, wk.dev, d_pb[i], span * nchan * 8);
    DEV_ALLOC(ctx, wk.dev, d_part[i], antpower_partial_bytes(sh, nchan));
    DEV_ALLOC(ctx, wk.dev, d_up[i], sh.nblocks * 4);
  }
  double* d_out = nullptr;                              // [3][nsnap][nchan]: power, num, den
  int64_t* d_uptot = nullptr;                           // [nsnap]
  const int64_t nout = nsnap * nchan;
  DEV_ALLOC(ctx, wk.dev, d_out, 3 * nout * 8);
  DEV_ALLOC(ctx, wk.dev, d_uptot, nsnap * 8);
  HIPCHK(ctx, hipStreamSynchronize(s0));              // stream 1 starts behind the uploads; the tables are caller memory

  auto kernels = [&](int64_t, Span snaps, int i, hipStream_t sc) -> int {
    const int64_t t = snaps.first;
    ApFrame fr;
    for (int k = 0; k < 9; ++k) fr.rot[k] = a->cel2enu[t * 9 + k];
    for (int k = 0; k < 3; ++k) fr.beta[k] = a->aberr_beta ? a->aberr_beta[t * 3 + k] : 0.0;
    const int64_t e = a->n_ext == nsnap ? t : 0;
    BeamParams bp{};
    fill_beam(bp, a->beam_kind, a->diameter_m, a->beam_pc_dircos, a->n_ext > 0 ? a->ext + e : nullptr, d_bf[(size_t)e]);
    bp.dirs = (const double*)d_dirs[i];
    bp.flux_ref = d_ones;
    bp.spindex = d_zeros;
    bp.freqs = d_freqs;
    bp.ref_freq = 1.0;
    bp.flag = d_flag;
    bp.nchan = nchan;
    bp.pb_out = d_pb[i];
    ApReduceParams rp;
    rp.dirs = (const double*)d_dirs[i]; rp.pb = d_pb[i];
    rp.flux_ref = d_fref; rp.spindex = d_spix; rp.spec = d_spec; rp.freqs = d_freqs;
    rp.ref_freq = table ? 1.0 : a->ref_freq_hz;
    rp.nchan = (int)nchan; rp.tile = (int)sh.tile; rp.lanes = (int)sh.lanes;
    rp.part = d_part[i];
    for (int64_t k = 0; k < pl.spans.count; ++k) {
      const Span sp = pl.spans.span(k, nsrc);
      const unsigned blocks = (unsigned)((sp.count + sh.block - 1) / sh.block);
      const int64_t b0 = sp.first / sh.block;
      if (int rc = launch(ctx, k_ap_dirs, dim3(blocks), 0, sc, (const double*)d_uvec, sp.first, sp.count, fr, d_dirs[i], d_up[i], b0)) return rc;
      bp.nsrc = sp.count;
      HIPCHK(ctx, launch_beam_flux(bp, sc));
      rp.s0 = sp.first; rp.count = sp.count; rp.b0 = b0;
      if (int rc = launch(ctx, k_ap_reduce, dim3(blocks, (unsigned)sh.ntiles), 0, sc, rp)) return rc;
    }
    return launch(ctx, k_ap_finish, dim3((unsigned)((nchan + kThreads - 1) / kThreads)), 0, sc, (const double*)d_part[i], (const int32_t*)d_up[i],
                  sh.nblocks, (int)nchan, d_out + t * nchan, d_out + nout + t * nchan, d_out + 2 * nout + t * nchan, d_uptot + t);
  };
  if (int rc = chunk_loop(ctx, st, chunks_of(nsnap, 1, nstreams), nsnap, no_step, kernels, no_step)) return rc;

  if (int rc = poly_beam_verdict(ctx, a->beam_kind, d_flag)) return rc;
  std::vector<int64_t> uptot((size_t)nsnap, 0);
  HIPCHK(ctx, hipMemcpy(uptot.data(), d_uptot, (size_t)nsnap * 8, hipMemcpyDeviceToHost));
  HIPCHK(ctx, hipMemcpy(out_power, d_out, (size_t)nout * 8, hipMemcpyDeviceToHost));
  if (out_num) HIPCHK(ctx, hipMemcpy(out_num, d_out + nout, (size_t)nout * 8, hipMemcpyDeviceToHost));
  if (out_den) HIPCHK(ctx, hipMemcpy(out_den, d_out + 2 * nout, (size_t)nout * 8, hipMemcpyDeviceToHost));
  if (stats) {
    int64_t up = 0;
    for (int64_t v : uptot) up += v;
    // per snapshot.  k_ap_dirs: 24 B read and 32 B written per source.  The beam: 32 B of dirs read per source, 8 B written per
    // (source, channel).  k_ap_reduce, for every source: the altitude (8 B) per channel tile, 8 B of pb_tile per channel and the flux --
    // 8 B per channel of the table, or 16 B per channel tile of the power law; the partial sums written and read once (16 B per block
    // and channel, twice); three output rows.
    stats->wall_ms = wall_ms_since(wall0);
    stats->kernel_ms = st.kernel_ms;
    stats->sources_evaluated = nsnap * nsrc;
    stats->sources_up = up;
    stats->spans = pl.spans.count;
    stats->span_sources = span;
    stats->block_sources = sh.block;
    stats->kernel_bytes = nsnap * (nsrc * (24 + 32 + 32 + 16 * nchan + 8 * sh.ntiles + (table ? 8 * nchan : 16 * sh.ntiles)) +
                                   2 * antpower_partial_bytes(sh, nchan) + 3 * nchan * 8);
    stats->upload_bytes = upload + span * 8;
    stats->download_bytes = ((out_num ? 1 : 0) + (out_den ? 1 : 0) + 1) * nout * 8 + nsnap * 8;
    stats->streams = nstreams;
    stats->chan_tile = (int32_t)sh.tile;
    stats->lds_bytes = (int32_t)sh.lds;
    stats->reserved_ = 0;
  }
  return PRISIM_OK;
}

}  // namespace

extern "C" {

int prisim_antenna_power(prisim_ctx* ctx, const prisim_antpower_args* a, double* out_power, double* out_num, double* out_den,
                         prisim_antpower_stats* stats) {
  return guarded(ctx, [&]() -> int { return antenna_power(ctx, a, out_power, out_num, out_den, stats); });
}

}  // extern "C"
