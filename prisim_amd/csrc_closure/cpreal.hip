// cpreal.hip -- closure phases of thermal-noise realisations for gfx950 (include/prisim_cpreal.h): the draw of
// prisim/scriptUtils/replicatesim_util.py (:82-95) and the per-realisation closure phases of
// prisim/bispectrum_phase.py:write_PRISim_bispectrum_phase_to_npz (:211-249) in one kernel, from the visibilities to the stack
// [nt][n_realize][ntriads][nchan] without a noise cube.
//
// The inputs are the used rows, snapshot-major: rms and bpwts [nt][nrow][nchan]; the cube is an uploaded [nt][nrow][nchan] or the
// context's resident [nt][nbl][nchan] read through cube_row.  A leg is ((cube + n) * bpwts), conjugated where the table says so; n is
// noise_draw (../csrc/noise_draw.h) of (channel, bl_global[row], snapshot) under the key seed + first + r, the value k_noise gives.
//
//   k_cpr_direct: one thread per output element (pair, T, channel), channel fastest.  It draws the noise of its three legs itself,
//     so a baseline is drawn once per triad that uses it: 3 ntriads nchan draws a pair.
//   k_cpr_staged: one workgroup per (pair, tile of channels).  It draws every used row of the tile once into LDS, [nrow][tile]
//     complex128, then walks the triads from there, channel fastest: nrow nchan draws a pair.  Conjugation is a sign on the read,
//     which is exact because bpwts is real.  The workgroup is 256, 512 or 1024 threads by its LDS (cpreal_plan.h).
// Per output double the direct kernel spends three Philox-4x32-10 draws with log, sqrt and sincospi and one atan2 in fp64 against
// 8 bytes written and 96 read (mostly from cache: the rows are shared by the triads); the staged kernel spends 3 nrow / ntriads of a
// draw.  Neither is bound by memory.  Chunks of (snapshot, realisation) pairs alternate between two streams with their own output
// buffers.  fp64 throughout, built with -ffp-contract=off: every product and sum rounds once.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/prisim_cpreal.h"
#include "../csrc/noise_draw.h"
#include "../csrc_addon/addon_internal.h"
#include "../csrc_addon/cpreal_plan.h"

namespace {

constexpr int kStagedMaxThreads = 1024;

struct CprParams {
  const double2* cube;      // element (t, row i, f) at (t * cnb + (crow ? crow[i] : i)) * nchan + f; not read with noise alone
  const int32_t* crow;
  int64_t cnb;
  const int64_t* blg;       // [nrow] global baseline of each used row
  const double* rms;        // [nt][nrow][nchan]
  const double* bpw;        // [nt][nrow][nchan]
  const int32_t* legs;      // [ntriads][3]
  const int32_t* conj;      // [ntriads][3]
  int64_t ntriads, nreal;
  int64_t p0, pc;           // first pair of the chunk, pairs in it; pair = t * nreal + r
  uint64_t key0;            // seed + first
  int nrow, nchan, tile, ntiles, noisy;
  double* out;              // this chunk's [pc][ntriads][nchan]
};

// ((cube + n) * bpwts) of used row i, channel f, snapshot t under `key`
__device__ __forceinline__ double2 row_value(const CprParams& P, int64_t t, int i, int f, uint64_t key) {
  const int64_t at = (t * P.nrow + i) * P.nchan + f;
  double2 v = noise_draw(f, P.blg[i], t, key, P.rms[at]);
  if (P.noisy) v = cadd(P.cube[(t * P.cnb + (P.crow ? P.crow[i] : i)) * P.nchan + f], v);
  return rmul(v, P.bpw[at]);
}

// numpy.angle: finite for B == 0 (atan2 of two zeros is 0 or +-pi)
__device__ __forceinline__ double phase_of(double2 b) { return atan2(b.y, b.x); }

__global__ void __launch_bounds__(kThreads) k_cpr_direct(CprParams P) {
  const int64_t per = P.ntriads * P.nchan, total = P.pc * per;
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kThreads) {
    const int f = (int)(e % P.nchan);
    const int64_t T = (e / P.nchan) % P.ntriads, pair = P.p0 + e / per;
    const int64_t t = pair / P.nreal;
    const uint64_t key = P.key0 + (uint64_t)(pair - t * P.nreal);
    double2 B = make_double2(0.0, 0.0);
#pragma unroll
    for (int l = 0; l < 3; ++l) {
      double2 v = row_value(P, t, P.legs[T * 3 + l], f, key);
      if (P.conj[T * 3 + l]) v.y = -v.y;
      B = l == 0 ? v : cmul(B, v);
    }
    P.out[e] = phase_of(B);
  }
}

// grid: x = (pair of the chunk) * ntiles + (channel tile).  LDS: [nrow][tile] complex128
__global__ void __launch_bounds__(kStagedMaxThreads) k_cpr_staged(CprParams P) {
  extern __shared__ double2 rows[];
  const int64_t pl = blockIdx.x / P.ntiles, pair = P.p0 + pl;
  const int c0 = (int)(blockIdx.x % P.ntiles) * P.tile;
  const int cn = min(P.tile, P.nchan - c0);
  const int64_t t = pair / P.nreal;
  const uint64_t key = P.key0 + (uint64_t)(pair - t * P.nreal);
  for (int e = threadIdx.x; e < P.nrow * P.tile; e += blockDim.x) {
    const int i = e / P.tile, c = e - i * P.tile;
    if (c < cn) rows[e] = row_value(P, t, i, c0 + c, key);
  }
  __syncthreads();
  double* out = P.out + pl * P.ntriads * P.nchan + c0;
  for (int64_t e = threadIdx.x; e < P.ntriads * P.tile; e += blockDim.x) {
    const int64_t T = e / P.tile;
    const int c = (int)(e - T * P.tile);
    if (c >= cn) continue;
    double2 B = make_double2(0.0, 0.0);
#pragma unroll
    for (int l = 0; l < 3; ++l) {
      double2 v = rows[P.legs[T * 3 + l] * P.tile + c];
      if (P.conj[T * 3 + l]) v.y = -v.y;
      B = l == 0 ? v : cmul(B, v);
    }
    out[T * P.nchan + c] = phase_of(B);
  }
}

int closure_realizations(prisim_ctx* ctx, const double* cube, const int32_t* cube_row, const int64_t* bl_global, int64_t nt, int64_t nrow,
                         int64_t nchan, const double* rms, const double* bpwts, const int32_t* legs, const int32_t* conj, int64_t ntriads,
                         uint64_t seed, int64_t first, int64_t n_realize, int32_t kind, int32_t route, int64_t budget_bytes,
                         double* out_phase, prisim_cpreal_stats* stats) {
  if (!ctx) return PRISIM_EINVAL;
  const WallTime wall0 = wall_now();
  if (nt < 1 || nrow < 1 || nchan < 1 || ntriads < 1 || n_realize < 1)
    return fail(ctx, PRISIM_EINVAL, "need nt, nrow, nchan, ntriads and n_realize >= 1");
  if (nt > (int64_t)1 << 30 || nrow > (int64_t)1 << 30 || nchan > (int64_t)1 << 20 || ntriads > (int64_t)1 << 30 || n_realize > (int64_t)1 << 30)
    return fail(ctx, PRISIM_EINVAL, "nt, nrow, ntriads and n_realize must be at most 2^30 and nchan at most 2^20");
  if (!bl_global || !rms || !bpwts || !legs || !conj || !out_phase) return fail(ctx, PRISIM_EINVAL, "null array");
  if (kind != PRISIM_CPREAL_NOISY && kind != PRISIM_CPREAL_NOISE) return fail(ctx, PRISIM_EINVAL, "unknown kind");
  if (route < PRISIM_CPREAL_AUTO || route > PRISIM_CPREAL_STAGED) return fail(ctx, PRISIM_EINVAL, "unknown route");
  if (!cube) {
    if (!ctx->array_set || !ctx->cube.p) return fail(ctx, PRISIM_ESTATE, "no resident visibility cube: set the array first");
    if (!cube_row) return fail(ctx, PRISIM_EINVAL, "null array: resident input needs cube_row");
    if (nchan != ctx->nchan || nt > ctx->nt_max)
      return fail(ctx, PRISIM_EINVAL, "the resident cube has " + std::to_string(ctx->nt_max) + " slots of " + std::to_string(ctx->nchan) +
                                          " channels; asked for " + std::to_string(nt) + " of " + std::to_string(nchan));
    for (int64_t i = 0; i < nrow; ++i)
      if (cube_row[i] < 0 || cube_row[i] >= ctx->nbl)
        return fail(ctx, PRISIM_EINVAL, "cube_row " + std::to_string(i) + " is row " + std::to_string(cube_row[i]) + " of a resident cube of " +
                                            std::to_string(ctx->nbl) + " baselines");
  }
  for (int64_t i = 0; i < nrow; ++i)
    if (bl_global[i] < 0) return fail(ctx, PRISIM_EINVAL, "negative global baseline index");
  for (int64_t i = 0; i < ntriads * 3; ++i)
    if (legs[i] < 0 || legs[i] >= nrow)
      return fail(ctx, PRISIM_EINVAL, "leg " + std::to_string(i % 3) + " of triad " + std::to_string(i / 3) + " is row " +
                                          std::to_string(legs[i]) + " of " + std::to_string(nrow) + " used rows");
  const int64_t nin = nt * nrow * nchan;
  for (int64_t i = 0; i < nin; ++i)
    if (!(rms[i] >= 0.0) || !std::isfinite(rms[i])) return fail(ctx, PRISIM_EINVAL, "noise rms must be finite and non-negative");
  HIPCHK(ctx, hipSetDevice(ctx->device));

  // route, tile and chunks
  int lds_max = 0;
  if (int rc = lds_limit(ctx, lds_max)) return rc;
  const int rt = cpreal_route(route, nrow, lds_max);
  if (rt < 0)
    return fail(ctx, PRISIM_EINVAL, "the staged route holds 16 B per used row and channel in LDS: " + std::to_string(nrow) + " rows of " +
                                        std::to_string(kCprealMinTile) + " channels do not fit in " + std::to_string(lds_max) + " B");
  const bool staged = rt == kCprealStaged;
  const CprealTile tl = staged ? cpreal_tile(nrow, nchan, lds_max) : CprealTile{0, 0, 0, kThreads};
  const int64_t npairs = nt * n_realize, per = ntriads * nchan;
  const Chunks ch = cpreal_chunks(npairs, per * 8, budget_bytes, tl.ntiles, kMaxBlocks, kMaxStreams);
  const int nstreams = ch.nstreams;

  // the rows and the tables go up on stream 0 as they are allocated
  Work wk;
  Streams& st = wk.st;
  if (int rc = st.create(ctx, nstreams, true)) return rc;
  hipStream_t s0 = st.s[0];
  const bool noisy = kind == PRISIM_CPREAL_NOISY;
  double2* d_cube = nullptr;
  double *d_rms = nullptr, *d_bpw = nullptr;
  int64_t* d_blg = nullptr;
  int32_t *d_crow = nullptr, *d_legs = nullptr, *d_conj = nullptr;
  if (cube && noisy) DEV_UPLOAD(ctx, wk.dev, d_cube, cube, (size_t)(nin * 2), s0);
  if (!cube) DEV_UPLOAD(ctx, wk.dev, d_crow, cube_row, (size_t)nrow, s0);
  DEV_UPLOAD(ctx, wk.dev, d_blg, bl_global, (size_t)nrow, s0);
  DEV_UPLOAD(ctx, wk.dev, d_rms, rms, (size_t)nin, s0);
  DEV_UPLOAD(ctx, wk.dev, d_bpw, bpwts, (size_t)nin, s0);
  DEV_UPLOAD(ctx, wk.dev, d_legs, legs, (size_t)(ntriads * 3), s0);
  DEV_UPLOAD(ctx, wk.dev, d_conj, conj, (size_t)(ntriads * 3), s0);
  double* d_out[kMaxStreams] = {};
  for (int i = 0; i < nstreams; ++i) DEV_ALLOC(ctx, wk.dev, d_out[i], ch.size * per * 8);

  // the kernels start behind whatever the context's stream still writes into the resident cube
  if (!cube) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(s0));            // stream 1 starts behind the uploads; the tables are caller memory

  CprParams base;
  base.cube = cube ? d_cube : (const double2*)ctx->cube.p;
  base.crow = d_crow;
  base.cnb = cube ? nrow : ctx->nbl;
  base.blg = d_blg; base.rms = d_rms; base.bpw = d_bpw; base.legs = d_legs; base.conj = d_conj;
  base.ntriads = ntriads; base.nreal = n_realize;
  base.p0 = 0; base.pc = 0;
  base.key0 = seed + (uint64_t)first;
  base.nrow = (int)nrow; base.nchan = (int)nchan; base.tile = (int)tl.tile; base.ntiles = (int)tl.ntiles; base.noisy = noisy ? 1 : 0;
  base.out = nullptr;
  if (staged)
    if (int rc = allow_lds(ctx, k_cpr_staged, tl.lds)) return rc;

  auto kernels = [&](int64_t, Span sp, int i, hipStream_t sc) -> int {
    CprParams P = base;
    P.p0 = sp.first; P.pc = sp.count; P.out = d_out[i];
    if (!staged) return launch(ctx, k_cpr_direct, dim3((unsigned)grid_for(ctx, sp.count * per)), 0, sc, P);
    hipLaunchKernelGGL(k_cpr_staged, dim3((unsigned)(sp.count * tl.ntiles)), dim3((unsigned)tl.threads), (size_t)tl.lds, sc, P);
    HIPCHK(ctx, hipGetLastError());
    return PRISIM_OK;
  };
  auto download = [&](int64_t, Span sp, int i, hipStream_t sc) -> int {
    HIPCHK(ctx, hipMemcpyAsync(out_phase + (size_t)sp.first * per, d_out[i], (size_t)sp.count * per * 8, hipMemcpyDeviceToHost, sc));
    return PRISIM_OK;
  };
  if (int rc = chunk_loop(ctx, st, ch, npairs, no_step, kernels, download)) return rc;
  if (stats) {
    // per draw: the rms read (8 B); per row value: its weight (8 B) and, with the visibilities, its cube element (16 B); per output
    // point: the phase written (8 B).  The staged kernel forms a row value once a pair, the direct one three times a point.
    const int64_t values = npairs * (staged ? nrow * nchan : 3 * per);
    stats->wall_ms = wall_ms_since(wall0);
    stats->kernel_ms = st.kernel_ms;
    stats->pairs = npairs;
    stats->chunks = ch.count;
    stats->chunk_pairs = ch.size;
    stats->draws = values;
    stats->kernel_bytes = values * (8 + 8 + (noisy ? 16 : 0)) + npairs * per * 8;
    stats->download_bytes = npairs * per * 8;
    stats->route = rt;
    stats->streams = nstreams;
    stats->chan_tile = (int32_t)tl.tile;
    stats->lds_bytes = (int32_t)tl.lds;
  }
  return PRISIM_OK;
}

}  // namespace

extern "C" {

int prisim_closure_realizations(prisim_ctx* ctx, const double* cube, const int32_t* cube_row, const int64_t* bl_global, int64_t nt,
                                int64_t nrow, int64_t nchan, const double* rms, const double* bpwts, const int32_t* legs,
                                const int32_t* conj, int64_t ntriads, uint64_t seed, int64_t first, int64_t n_realize, int32_t kind,
                                int32_t route, int64_t budget_bytes, double* out_phase, prisim_cpreal_stats* stats) {
  return guarded(ctx, [&]() -> int {
    return closure_realizations(ctx, cube, cube_row, bl_global, nt, nrow, nchan, rms, bpwts, legs, conj, ntriads, seed, first, n_realize,
                                kind, route, budget_bytes, out_phase, stats);
  });
}

}  // extern "C"
