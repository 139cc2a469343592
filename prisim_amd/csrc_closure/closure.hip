// closure.hip -- visibility triplets and closure phases of antenna triads for gfx950 (include/prisim_closure.h): the per-triad body of
// prisim/interferometry.py:getClosurePhase (:7411-7651) for one cube.
//
// Element (baseline b, channel ch, snapshot t) of the cube sits at cube[b sb + ch sc + t st]: the context's resident slots are
// [nt][nbl][nchan] (sc = 1), an uploaded host cube is [nbl][nchan][nt] (st = 1).  The outputs are snapshot-fastest:
// triplets [T][3][nchan][nt], phases [T][nchan][nt]; the weights bpwts are [nbl][nchan][nt].
//
// No filter (PRISIM_CLOSURE_DIRECT): one kernel forms the three legs, their product and its phase; every output is written once.
//   k_cl_plain: one thread per (T, ch, t), snapshot-fastest.  An uploaded cube is read, and everything written, in runs of nt
//     elements; this is also the path of a resident cube of a few snapshots.
//   k_cl_tiled (resident cube, nt >= 16): one workgroup per (T, 32 channels, 32 snapshots).  Each leg's tile is read along the
//     channels (512-byte runs), turned through a [32][33] LDS tile (rows of 528 bytes: lane k of a column read starts at bank
//     4k mod 64, so the 16 lanes that a 128-bit read serves together touch 16 different 16-byte slots) and written along the snapshots.
// Delay filter: the triplets of a chunk first, then k_cl_phase over them.
//   fused (nchan a power of two): one workgroup per (T, leg, tile of snapshots).  The rows freq_wts * v are loaded into LDS, a
//     decimation-in-frequency radix-2 transform leaves fft(x) in bit-reversed order, position p is multiplied by mask[rev(p)] / nchan,
//     and a decimation-in-time transform with the conjugate twiddles takes that bit-reversed order back to the channels in natural
//     order: no reordering pass.  Rows are padded by one element, so that the snapshot-fastest read of the result walks the banks.
//   rocFFT (any other nchan): k_cl_prepare [row][t][nchan] -> forward rocFFT -> k_cl_mask -> inverse rocFFT -> k_cl_finish.
// Chunks of triads alternate between two streams with their own buffers.  The outputs are the caller's pageable arrays, and a
// device-to-host copy into pageable memory holds the host until it is done, so the kernels of chunk c + 1 are in practice launched
// after the copy of chunk c: the two streams order the reuse of the buffers, they were not seen to overlap anything.  Page-locking the
// outputs for the call (hipHostRegister) was measured and dropped: registering 5.3 GB cost more than the asynchronous copies gained
// (329-350 ms against 243-254 ms per call, four interleaved rounds in one process).  The kernels are under 4 % of the call.
// fp64 throughout, built with -ffp-contract=off: the products round as numpy's separate products do.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "closure_internal.h"

namespace {

constexpr int kTile = 32;                             // k_cl_tiled: channels and snapshots per tile
constexpr int kTiledMinNt = 16;                       // fewer snapshots than this: the plain kernel

struct ClParams {
  const double2* cube;
  int64_t sb, sc, st;       // element strides of (baseline, channel, snapshot)
  const double* bpw;        // [nbl][nchan][nt]
  const double* fw;         // [nchan]
  const double* masks;      // [nmask][nchan]
  const int32_t* midx;      // [nbl], or null: mask 0
  const int32_t* legs;      // [ntriads][3]
  const int32_t* conj;      // [ntriads][3]
  int64_t T0, tc;           // first triad of the chunk, triads in it
  int nchan, nt, logn, tile, ntiles;
  double2* trip;            // this chunk's [tc][3][nchan][nt]
  double* phase;            // this chunk's [tc][nchan][nt]
  double2* fbuf;            // rocFFT route: [tc * 3][nt][nchan]
};

// freq_wts[ch] * v of one leg (row `ind` of the cube, conjugated if cj)
__device__ __forceinline__ double2 leg_value(const ClParams& P, int ind, int cj, int ch, int t) {
  double2 v = P.cube[ind * P.sb + ch * P.sc + t * P.st];
  if (cj) v.y = -v.y;
  return rmul(v, P.fw[ch]);
}

__device__ __forceinline__ double bpw_value(const ClParams& P, int ind, int ch, int t) {
  return P.bpw[((int64_t)ind * P.nchan + ch) * P.nt + t];
}

// numpy.angle: finite for B == 0 (atan2 of two zeros is 0 or +-pi)
__device__ __forceinline__ double phase_of(double2 b) { return atan2(b.y, b.x); }

__global__ void __launch_bounds__(kThreads) k_cl_plain(ClParams P) {
  const int64_t per = (int64_t)P.nchan * P.nt, total = P.tc * per;
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kThreads) {
    const int t = (int)(e % P.nt);
    const int ch = (int)((e / P.nt) % P.nchan);
    const int64_t T = e / per;
    double2 B = make_double2(0.0, 0.0);
#pragma unroll
    for (int l = 0; l < 3; ++l) {
      const int ind = P.legs[(P.T0 + T) * 3 + l], cj = P.conj[(P.T0 + T) * 3 + l];
      const double2 v = rmul(leg_value(P, ind, cj, ch, t), bpw_value(P, ind, ch, t));
      P.trip[(T * 3 + l) * per + (int64_t)ch * P.nt + t] = v;
      B = l == 0 ? v : cmul(B, v);
    }
    P.phase[e] = phase_of(B);
  }
}

// resident cube (sc == 1).  grid: x = T * nct * ntt + (channel tile) * ntt + (snapshot tile)
__global__ void __launch_bounds__(kThreads) k_cl_tiled(ClParams P, int nct, int ntt) {
  __shared__ double2 tile[kTile][kTile + 1];
  const int64_t T = blockIdx.x / ((int64_t)nct * ntt);
  const int rem = (int)(blockIdx.x % ((int64_t)nct * ntt));
  const int c0 = (rem / ntt) * kTile, t0 = (rem % ntt) * kTile;
  const int lx = threadIdx.x % kTile, ly = threadIdx.x / kTile;      // ly < 8
  const int64_t per = (int64_t)P.nchan * P.nt;
  double2 B[kTile / 8];
#pragma unroll
  for (int l = 0; l < 3; ++l) {
    const int ind = P.legs[(P.T0 + T) * 3 + l], cj = P.conj[(P.T0 + T) * 3 + l];
#pragma unroll
    for (int i = 0; i < kTile / 8; ++i) {                              // lanes along the channels
      const int tt = ly + 8 * i, ch = c0 + lx, t = t0 + tt;
      if (ch < P.nchan && t < P.nt) tile[tt][lx] = leg_value(P, ind, cj, ch, t);
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kTile / 8; ++i) {                              // lanes along the snapshots
      const int cc = ly + 8 * i, ch = c0 + cc, t = t0 + lx;
      if (ch < P.nchan && t < P.nt) {
        const double2 v = rmul(tile[lx][cc], bpw_value(P, ind, ch, t));
        P.trip[(T * 3 + l) * per + (int64_t)ch * P.nt + t] = v;
        B[i] = l == 0 ? v : cmul(B[i], v);
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < kTile / 8; ++i) {
    const int ch = c0 + ly + 8 * i, t = t0 + lx;
    if (ch < P.nchan && t < P.nt) P.phase[T * per + (int64_t)ch * P.nt + t] = phase_of(B[i]);
  }
}

// phases of a chunk's finished triplets
__global__ void __launch_bounds__(kThreads) k_cl_phase(ClParams P) {
  const int64_t per = (int64_t)P.nchan * P.nt, total = P.tc * per;
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kThreads) {
    const int64_t T = e / per, r = e - T * per;
    const double2* p = P.trip + T * 3 * per + r;
    P.phase[e] = phase_of(cmul(cmul(p[0], p[per]), p[2 * per]));
  }
}

// fused filter.  grid: x = (T * 3 + leg) * ntiles + (snapshot tile).  LDS: buf [tile][nchan + 1] | tw [nchan / 2]
__global__ void __launch_bounds__(kThreads) k_cl_fused(ClParams P) {
  extern __shared__ double2 lds[];
  const int n = P.nchan, ld = n + 1, tile = P.tile, half = n / 2;
  double2* buf = lds;
  double2* tw = buf + (int64_t)tile * ld;
  const int64_t row = blockIdx.x / P.ntiles;                           // T * 3 + leg of the chunk
  const int t0 = (int)(blockIdx.x % P.ntiles) * tile;
  const int tcount = min(tile, P.nt - t0);
  const int ind = P.legs[P.T0 * 3 + row], cj = P.conj[P.T0 * 3 + row];
  const double* mask = P.masks + (int64_t)(P.midx ? P.midx[ind] : 0) * n;
  lds_twiddles(tw, n);
  for (int e = threadIdx.x; e < n * tile; e += kThreads) {
    int ch, tt;
    if (P.sc == 1) { tt = e / n; ch = e - tt * n; } else { ch = e / tile; tt = e - ch * tile; }      // the cube's fastest axis on the lanes
    buf[tt * ld + ch] = tt < tcount ? leg_value(P, ind, cj, ch, t0 + tt) : make_double2(0.0, 0.0);
  }
  __syncthreads();
  for (int h = half; h >= 1; h >>= 1) {                                // forward, decimation in frequency: W = e^{-2 pi i / (2h)}
    const int step = n / (2 * h);
    for (int i = threadIdx.x; i < tile * half; i += kThreads) {
      const int tt = i / half, ii = i - tt * half;
      const int pos = ii & (h - 1);
      const int a = tt * ld + ((ii - pos) << 1) + pos, b = a + h;
      const double2 u = buf[a], v = buf[b];
      buf[a] = cadd(u, v);
      buf[b] = cmulc(csub(u, v), tw[pos * step]);
    }
    __syncthreads();
  }
  const double inv = 1.0 / (double)n;
  for (int e = threadIdx.x; e < n * tile; e += kThreads) {             // position p holds fft(x)[rev(p)]
    const int tt = e / n, p = e - tt * n;
    const int j = bitrev(p, P.logn);
    buf[tt * ld + p] = rmul(buf[tt * ld + p], mask[j] * inv);
  }
  __syncthreads();
  lds_ifft_dit(buf, ld, tile, n, tw);                                  // inverse, decimation in time
  double2* dst = P.trip + row * n * (int64_t)P.nt + t0;
  for (int e = threadIdx.x; e < n * tile; e += kThreads) {
    const int ch = e / tile, tt = e - ch * tile;
    if (tt < tcount) dst[(int64_t)ch * P.nt + tt] = rmul(buf[tt * ld + ch], bpw_value(P, ind, ch, t0 + tt));
  }
}

// rocFFT route: fbuf[row][t][ch] = freq_wts * v
__global__ void __launch_bounds__(kThreads) k_cl_prepare(ClParams P) {
  const int64_t total = P.tc * 3 * (int64_t)P.nt * P.nchan;
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kThreads) {
    const int ch = (int)(e % P.nchan);
    const int64_t line = e / P.nchan;
    const int t = (int)(line % P.nt);
    const int64_t row = line / P.nt;
    P.fbuf[e] = leg_value(P, P.legs[P.T0 * 3 + row], P.conj[P.T0 * 3 + row], ch, t);
  }
}

// between the forward and the (unnormalised) inverse transform
__global__ void __launch_bounds__(kThreads) k_cl_mask(ClParams P) {
  const int64_t total = P.tc * 3 * (int64_t)P.nt * P.nchan;
  const double inv = 1.0 / (double)P.nchan;
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kThreads) {
    const int j = (int)(e % P.nchan);
    const int64_t row = e / ((int64_t)P.nchan * P.nt);
    const int ind = P.legs[P.T0 * 3 + row];
    P.fbuf[e] = rmul(P.fbuf[e], P.masks[(int64_t)(P.midx ? P.midx[ind] : 0) * P.nchan + j] * inv);
  }
}

// trip[row][ch][t] = fbuf[row][t][ch] * bpwts
__global__ void __launch_bounds__(kThreads) k_cl_finish(ClParams P) {
  const int64_t total = P.tc * 3 * (int64_t)P.nt * P.nchan;
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kThreads) {
    const int t = (int)(e % P.nt);
    const int64_t line = e / P.nt;
    const int ch = (int)(line % P.nchan);
    const int64_t row = line / P.nchan;
    P.trip[e] = rmul(P.fbuf[(row * P.nt + t) * P.nchan + ch], bpw_value(P, P.legs[P.T0 * 3 + row], ch, t));
  }
}

}  // namespace

// The call itself.  With a sink (closure_internal.h) the phases of every chunk are handed on where they lie, and the caller's
// out_triplets / out_phase may each be null: what is null is not downloaded.
int closure_phase_chunks(prisim_ctx* ctx, const double* cube, int64_t nt, int64_t nbl, int64_t nchan, const int32_t* legs,
                         const int32_t* conj, int64_t ntriads, const double* freq_wts, const double* bpwts, const double* masks,
                         int64_t nmask, const int32_t* mask_index, int32_t route, int64_t budget_bytes, double* out_triplets,
                         double* out_phase, prisim_closure_stats* stats, const ClosureSink* sink) {
  if (!ctx) return PRISIM_EINVAL;
  const WallTime wall0 = wall_now();
  if (nt < 1 || nbl < 1 || nchan < 1 || ntriads < 1) return fail(ctx, PRISIM_EINVAL, "need nt, nbl, nchan and ntriads >= 1");
  if (nt > (int64_t)1 << 30 || nchan > (int64_t)1 << 30 || nbl > (int64_t)1 << 30)
    return fail(ctx, PRISIM_EINVAL, "nt, nbl and nchan must fit in 32 bits");
  if (!legs || !conj || !freq_wts || !bpwts || (!sink && (!out_triplets || !out_phase))) return fail(ctx, PRISIM_EINVAL, "null array");
  if (!cube) {
    if (!ctx->array_set || !ctx->cube.p) return fail(ctx, PRISIM_ESTATE, "no resident visibility cube: set the array first");
    if (nbl != ctx->nbl || nchan != ctx->nchan || nt > ctx->nt_max)
      return fail(ctx, PRISIM_EINVAL, "the resident cube has " + std::to_string(ctx->nt_max) + " slots of " + std::to_string(ctx->nbl) +
                                          " x " + std::to_string(ctx->nchan) + "; asked for " + std::to_string(nt) + " of " +
                                          std::to_string(nbl) + " x " + std::to_string(nchan));
  }
  for (int64_t i = 0; i < ntriads * 3; ++i)
    if (legs[i] < 0 || legs[i] >= nbl)
      return fail(ctx, PRISIM_EINVAL, "leg " + std::to_string(i % 3) + " of triad " + std::to_string(i / 3) + " is row " +
                                          std::to_string(legs[i]) + " of a cube of " + std::to_string(nbl) + " baselines");
  const bool filter = masks != nullptr;
  if (route < PRISIM_CLOSURE_AUTO || route > PRISIM_CLOSURE_ROCFFT) return fail(ctx, PRISIM_EINVAL, "unknown route");
  bool pow2;
  const int logn = ceil_log2(nchan, pow2);
  int rt = PRISIM_CLOSURE_DIRECT;
  if (filter) {
    if (nmask < 1) return fail(ctx, PRISIM_EINVAL, "the delay filter needs at least one mask");
    if (nchan > PRISIM_CLOSURE_MAX_LEN)
      return fail(ctx, PRISIM_EINVAL, "the delay filter takes rows of 1 to " + std::to_string(PRISIM_CLOSURE_MAX_LEN) +
                                          " channels (PRISIM_CLOSURE_MAX_LEN); got " + std::to_string(nchan));
    if (mask_index)
      for (int64_t b = 0; b < nbl; ++b)
        if (mask_index[b] < 0 || mask_index[b] >= nmask) return fail(ctx, PRISIM_EINVAL, "mask_index out of range");
    if (route == PRISIM_CLOSURE_DIRECT) return fail(ctx, PRISIM_EINVAL, "the direct route takes no delay filter");
    if (route == PRISIM_CLOSURE_FUSED && !pow2)
      return fail(ctx, PRISIM_EINVAL, "the fused route takes a power-of-two nchan; got " + std::to_string(nchan));
    rt = (route == PRISIM_CLOSURE_ROCFFT || (route == PRISIM_CLOSURE_AUTO && !pow2)) ? PRISIM_CLOSURE_ROCFFT : PRISIM_CLOSURE_FUSED;
  } else if (route == PRISIM_CLOSURE_FUSED || route == PRISIM_CLOSURE_ROCFFT) {
    return fail(ctx, PRISIM_EINVAL, "the fused and rocFFT routes are those of the delay filter; no masks were given");
  }
  HIPCHK(ctx, hipSetDevice(ctx->device));

  // tile, LDS and chunking
  const bool tiled = rt == PRISIM_CLOSURE_DIRECT && !cube && nt >= kTiledMinNt;
  int64_t tile = tiled ? 1 : 0, ntiles = 1, lds = tiled ? (int64_t)sizeof(double2) * kTile * (kTile + 1) : 0;
  if (rt == PRISIM_CLOSURE_FUSED) {
    int lds_max = 0;
    if (int rc = lds_limit(ctx, lds_max)) return rc;
    const SnapshotTile sn = snapshot_tile(nt, 16 * (nchan + 1), 16 * std::max<int64_t>(nchan / 2, 1));
    tile = sn.tile; ntiles = sn.ntiles; lds = sn.lds;
    if (lds > lds_max) {                              // (not on gfx950: a row of PRISIM_CLOSURE_MAX_LEN channels takes 96 KiB of its 160)
      if (route == PRISIM_CLOSURE_FUSED) return fail(ctx, PRISIM_EINVAL, "a row does not fit in LDS (" + std::to_string(lds) + " B needed)");
      rt = PRISIM_CLOSURE_ROCFFT;
      tile = 0; ntiles = 1; lds = 0;
    }
  }
  if (rt == PRISIM_CLOSURE_ROCFFT)
    if (int rc = ensure_rocfft(ctx)) return rc;
  const int64_t nct = (nchan + kTile - 1) / kTile, ntt = (nt + kTile - 1) / kTile;
  const int64_t per = nchan * nt;
  const int64_t trip_triad = 3 * per * 16, phase_triad = per * 8, fbuf_triad = rt == PRISIM_CLOSURE_ROCFFT ? 3 * per * 16 : 0;
  const int64_t per_triad = trip_triad + phase_triad + fbuf_triad + (sink ? sink->bytes_per_triad : 0);
  const int64_t fit = plan_chunks(ntriads, per_triad, budget_bytes, kMaxStreams).size;
  const int64_t blocks_triad = tiled ? nct * ntt : 3 * ntiles;                      // grid x of the tiled kernels
  const int64_t grid_max = std::max<int64_t>(1, (((int64_t)1 << 31) - 1) / blocks_triad);
  const Chunks ch = chunks_of(ntriads, std::min(fit, grid_max), kMaxStreams);
  const int64_t tc = ch.size, nchunks = ch.count;
  const int nstreams = ch.nstreams;

  // the cube and the tables go up on stream 0 as they are allocated
  Work wk;
  Streams& st = wk.st;
  if (int rc = st.create(ctx, nstreams, true)) return rc;
  hipStream_t s0 = st.s[0];
  double2* d_cube = nullptr;
  double *d_bpw = nullptr, *d_fw = nullptr, *d_masks = nullptr;
  int32_t *d_midx = nullptr, *d_legs = nullptr, *d_conj = nullptr;
  if (cube) DEV_UPLOAD(ctx, wk.dev, d_cube, cube, (size_t)(nbl * per * 2), s0);
  DEV_UPLOAD(ctx, wk.dev, d_bpw, bpwts, (size_t)(nbl * per), s0);
  DEV_UPLOAD(ctx, wk.dev, d_fw, freq_wts, (size_t)nchan, s0);
  DEV_UPLOAD(ctx, wk.dev, d_legs, legs, (size_t)(ntriads * 3), s0);
  DEV_UPLOAD(ctx, wk.dev, d_conj, conj, (size_t)(ntriads * 3), s0);
  if (filter) {
    DEV_UPLOAD(ctx, wk.dev, d_masks, masks, (size_t)(nmask * nchan), s0);
    if (mask_index) DEV_UPLOAD(ctx, wk.dev, d_midx, mask_index, (size_t)nbl, s0);
  }
  double2* d_trip[kMaxStreams] = {};
  double* d_phase[kMaxStreams] = {};
  double2* d_fbuf[kMaxStreams] = {};
  for (int i = 0; i < nstreams; ++i) {
    DEV_ALLOC(ctx, wk.dev, d_trip[i], tc * trip_triad);
    DEV_ALLOC(ctx, wk.dev, d_phase[i], tc * phase_triad);
    if (fbuf_triad) DEV_ALLOC(ctx, wk.dev, d_fbuf[i], tc * fbuf_triad);
  }
  if (sink)
    if (int rc = sink->prepare(tc, ch.last, nstreams, st.s)) return rc;
  if (rt == PRISIM_CLOSURE_ROCFFT) {
    const size_t b0 = (size_t)tc * 3 * (size_t)nt, b1 = (size_t)ch.last * 3 * (size_t)nt;
    if (int rc = wk.fft.create(ctx, wk.dev, (size_t)nchan, {{false, b0}, {true, b0}, {false, b1}, {true, b1}}, st.s, nstreams)) return rc;
  }

  // the kernels start behind whatever the context's stream still writes into the resident cube
  if (!cube) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(s0));            // stream 1 starts behind the uploads; the tables are caller memory

  ClParams base;
  base.cube = cube ? d_cube : (const double2*)ctx->cube.p;
  if (cube) { base.sb = per; base.sc = nt; base.st = 1; } else { base.sb = nchan; base.sc = 1; base.st = nbl * nchan; }
  base.bpw = d_bpw; base.fw = d_fw; base.masks = d_masks; base.midx = d_midx; base.legs = d_legs; base.conj = d_conj;
  base.T0 = 0; base.tc = 0;
  base.nchan = (int)nchan; base.nt = (int)nt; base.logn = logn; base.tile = (int)tile; base.ntiles = (int)ntiles;
  base.trip = nullptr; base.phase = nullptr; base.fbuf = nullptr;
  if (rt == PRISIM_CLOSURE_FUSED)
    if (int rc = allow_lds(ctx, k_cl_fused, lds)) return rc;

  auto kernels = [&](int64_t, Span sp, int i, hipStream_t sc) -> int {
    const int64_t T0 = sp.first, tn = sp.count;
    ClParams P = base;
    P.T0 = T0; P.tc = tn; P.trip = d_trip[i]; P.phase = d_phase[i]; P.fbuf = d_fbuf[i];
    const int64_t ne = tn * per;
    if (rt == PRISIM_CLOSURE_DIRECT) {
      if (int rc = tiled ? launch(ctx, k_cl_tiled, dim3((unsigned)(tn * nct * ntt)), 0, sc, P, (int)nct, (int)ntt)
                         : launch(ctx, k_cl_plain, dim3((unsigned)grid_for(ctx, ne)), 0, sc, P)) return rc;
    } else {
      if (rt == PRISIM_CLOSURE_FUSED) {
        if (int rc = launch(ctx, k_cl_fused, dim3((unsigned)(tn * 3 * ntiles)), (size_t)lds, sc, P)) return rc;
      } else {
        const int g = grid_for(ctx, 3 * ne);
        const size_t batch = (size_t)tn * 3 * (size_t)nt;
        if (int rc = launch(ctx, k_cl_prepare, dim3((unsigned)g), 0, sc, P)) return rc;
        if (int rc = wk.fft.run(ctx, false, batch, d_fbuf[i], i)) return rc;
        if (int rc = launch(ctx, k_cl_mask, dim3((unsigned)g), 0, sc, P)) return rc;
        if (int rc = wk.fft.run(ctx, true, batch, d_fbuf[i], i)) return rc;
        if (int rc = launch(ctx, k_cl_finish, dim3((unsigned)g), 0, sc, P)) return rc;
      }
      if (int rc = launch(ctx, k_cl_phase, dim3((unsigned)grid_for(ctx, ne)), 0, sc, P)) return rc;
    }
    return sink ? sink->kernels(i, sc, T0, tn, d_phase[i]) : PRISIM_OK;
  };
  auto download = [&](int64_t, Span sp, int i, hipStream_t sc) -> int {
    const int64_t T0 = sp.first, tn = sp.count;
    if (out_triplets)
      HIPCHK(ctx, hipMemcpyAsync(out_triplets + 2 * (size_t)T0 * 3 * per, d_trip[i], (size_t)tn * trip_triad, hipMemcpyDeviceToHost, sc));
    if (out_phase) HIPCHK(ctx, hipMemcpyAsync(out_phase + (size_t)T0 * per, d_phase[i], (size_t)tn * phase_triad, hipMemcpyDeviceToHost, sc));
    return sink ? sink->download(i, sc, T0, tn) : PRISIM_OK;
  };
  if (int rc = chunk_loop(ctx, st, ch, ntriads, no_step, kernels, download)) return rc;
  if (stats) {
    // per output point: three legs read (16 B) with their weights (8 B) and written (16 B), one phase written (8 B); the filter's
    // phase kernel reads the triplets again, and the rocFFT route passes its row buffer through five kernels (read and write)
    int64_t point = 3 * (16 + 8 + 16) + 8;
    if (rt != PRISIM_CLOSURE_DIRECT) point += 3 * 16;
    if (rt == PRISIM_CLOSURE_ROCFFT) point += 3 * 16 * 8;
    stats->wall_ms = wall_ms_since(wall0);
    stats->kernel_ms = st.kernel_ms;
    stats->triads = ntriads;
    stats->chunks = nchunks;
    stats->chunk_triads = tc;
    stats->kernel_bytes = ntriads * per * point;
    stats->download_bytes = ntriads * ((out_triplets ? trip_triad : 0) + (out_phase ? phase_triad : 0));
    stats->route = rt;
    stats->streams = nstreams;
    stats->tile = (int32_t)tile;
    stats->lds_bytes = (int32_t)lds;
  }
  return PRISIM_OK;
}

extern "C" {

int prisim_closure_phase(prisim_ctx* ctx, const double* cube, int64_t nt, int64_t nbl, int64_t nchan, const int32_t* legs,
                         const int32_t* conj, int64_t ntriads, const double* freq_wts, const double* bpwts, const double* masks,
                         int64_t nmask, const int32_t* mask_index, int32_t route, int64_t budget_bytes, double* out_triplets,
                         double* out_phase, prisim_closure_stats* stats) {
  return guarded(ctx, [&]() -> int {
    return closure_phase_chunks(ctx, cube, nt, nbl, nchan, legs, conj, ntriads, freq_wts, bpwts, masks, nmask, mask_index, route,
                                budget_bytes, out_triplets, out_phase, stats, nullptr);
  });
}

}  // extern "C"
