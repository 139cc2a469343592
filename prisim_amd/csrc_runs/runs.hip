// runs.hip -- delay spectra and delay power spectra of stacks of runs for gfx950 (include/prisim_runs.h):
// prisim/delay_spectrum.py:delay_transform_allruns (:1475-1618), subband_delay_transform_allruns (:2252-2513) and the product of
// compute_power_spectrum_allruns (:4067-4195), on the caller's arrays in the reference's layout.
//
// A row is one (run, baseline, snapshot): channel n of row (p, t) sits at vis[(p nchan + n) nt + t], p = run * nbl + baseline.  Every
// kernel maps consecutive lanes to consecutive snapshots of one channel, so that the [nchan][nt] block of a pair is read, and the
// [nout][nt] block of the spectra written, in contiguous runs of nt elements.
//
// The transform, the shift, the resampled bins and their direct sum are csrc_addon/delay_lines.h's, with the scale s = scale / m.
// Fused route (m a power of two): one workgroup per (pair, window, tile of TT snapshots); the selected lags are written.
// rocFFT route (any other m): k_runs_prepare writes the windowed padded rows [w][pair][t][m] -> batched inverse rocFFT in place ->
// k_runs_finish shifts, scales, selects and writes [w][pair][j][t].
// Resampling (out_mode PRISIM_RUNS_RESAMPLE, any m): k_runs_resample forms every bin Y[k] in LDS and sums over the bins inside the
// span of the window's nonzero channels (Feeds::kSpan); the m-lag spectra never exist.
// The power kernel forms Re(v1 conj(v2)) * factor (* 2) as numpy rounds it.
// Chunks of pairs are spread over two streams with their own buffers: the copies of one chunk overlap the kernels of the other.
// fp64 throughout (complex64 input is widened on load), built with -ffp-contract=off; the one fused product is an explicit fma().
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../csrc_addon/delay_lines.h"
#include "../../include/prisim_runs.h"

namespace {

struct RunParams {
  const void* vis;          // this chunk's [pc][nchan][nt] (complex128 or complex64), or null: ones
  int c64;
  const double* bp;         // weights over (baseline, channel, snapshot), or null
  int64_t bs0, bs1, bs2;
  const double* wts;
  int64_t ws0, ws1, ws2;
  const double* win;        // [nwin][nchan], or null
  int nwin, nchan, nt, m, logm, nout, mode, tile, ntiles;
  int64_t nbl, p0, pc;      // first global pair of the chunk, pairs in the chunk
  double s;                 // scale / m
  double factor;            // PRISIM_RUNS_INTERP: lag position step
  const int32_t* rs_in;     // [2][nout] input bins of the resampled spectrum (-1: none)
  const double2* rs_c;      // [2][nout] their coefficients map_w (scale / m) e^{-2 pi i k_in floor(m/2) / m}
  const double2* rtw;       // [nout] e^{+2 pi i q / nout}
  const int32_t* klist;     // bins each window can make nonzero: klist[kofs[w] .. kofs[w + 1])
  const int32_t* kofs;
  double2* out;             // this chunk's [nwin][pc][nout][nt]
  double2* fbuf;            // rocFFT route: [nwin][pc][nt][m]
};

// x[n] of row (local pair pl, snapshot t) under window w: ((vis * bp) * wts) * win, as numpy multiplies a complex array by real ones
__device__ __forceinline__ double2 row_value(const RunParams& P, int64_t pl, int n, int t, int w) {
  double2 v = make_double2(1.0, 0.0);
  const int64_t i = (pl * P.nchan + n) * (int64_t)P.nt + t;
  if (P.vis) {
    if (P.c64) {
      const float2 f = reinterpret_cast<const float2*>(P.vis)[i];
      v = make_double2((double)f.x, (double)f.y);
    } else {
      v = reinterpret_cast<const double2*>(P.vis)[i];
    }
  }
  const int64_t b = (P.p0 + pl) % P.nbl;
  if (P.bp) v = rmul(v, P.bp[b * P.bs0 + n * P.bs1 + t * P.bs2]);
  if (P.wts) v = rmul(v, P.wts[b * P.ws0 + n * P.ws1 + t * P.ws2]);
  if (P.win) v = rmul(v, P.win[(int64_t)w * P.nchan + n]);
  return v;
}

// output lag j of a shifted spectrum row: the lag itself, or dsp_readings.downsampler's linear interpolation at j * factor
template <typename Get>
__device__ __forceinline__ double2 select_lag(const RunParams& P, int j, Get get) {
  if (P.mode != PRISIM_RUNS_INTERP) return get(j);
  const double pos = (double)j * P.factor;
  int i0 = (int)floor(pos);
  const double frac = pos - (double)i0;
  i0 = min(i0, P.m - 1);
  const int i1 = min(i0 + 1, P.m - 1);
  const double2 x0 = get(i0), x1 = get(i1);
  return cadd(x0, rmul(csub(x1, x0), frac));
}

// fused route.  LDS: buf [tile][m] | tw [m/2]
__global__ void __launch_bounds__(kThreads) k_runs_fused(RunParams P) {
  extern __shared__ double2 lds[];
  const int m = P.m, tile = P.tile;
  double2* buf = lds;
  double2* tw = buf + (int64_t)tile * m;
  const int64_t pl = blockIdx.x / P.ntiles;
  const int t0 = (int)(blockIdx.x % P.ntiles) * tile;
  const int w = blockIdx.y;
  const int tcount = min(tile, P.nt - t0);
  lds_twiddles(tw, m);
  for (int e = threadIdx.x; e < m * tile; e += kThreads) {
    const int n = e / tile, tt = e - n * tile;
    LdsOperand x = shifted_zero(n, P.logm);
    if (n < P.nchan && tt < tcount) x = shifted_operand(row_value(P, pl, n, t0 + tt, w), n, m, P.logm, P.s);
    buf[tt * m + x.slot] = x.v;
  }
  __syncthreads();
  lds_ifft_dit(buf, m, tile, m, tw);
  double2* dst = P.out + ((int64_t)w * P.pc + pl) * P.nout * P.nt + t0;
  for (int e = threadIdx.x; e < P.nout * tile; e += kThreads) {
    const int j = e / tile, tt = e - j * tile;
    if (tt >= tcount) continue;
    const double2* row = buf + tt * m;
    dst[(int64_t)j * P.nt + tt] = select_lag(P, j, [&](int i) { return row[i]; });
  }
}

// rocFFT route, before the transform: fbuf[w][pl][t][n] = x[n] (zero for n >= nchan)
__global__ void __launch_bounds__(kThreads) k_runs_prepare(RunParams P) {
  const int64_t total = (int64_t)P.nwin * P.pc * P.nt * P.m;
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kThreads) {
    const int n = (int)(e % P.m);
    const int64_t line = e / P.m;
    const int t = (int)(line % P.nt);
    const int64_t wp = line / P.nt;
    const int64_t pl = wp % P.pc;
    const int w = (int)(wp / P.pc);
    P.fbuf[e] = n < P.nchan ? row_value(P, pl, n, t, w) : make_double2(0.0, 0.0);
  }
}

// rocFFT route, after the unnormalised inverse transform: every selected lag gathers its transform bins
__global__ void __launch_bounds__(kThreads) k_runs_finish(RunParams P) {
  const int m = P.m;
  const int64_t total = (int64_t)P.nwin * P.pc * P.nout * P.nt;
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kThreads) {
    const int t = (int)(e % P.nt);
    const int64_t r = e / P.nt;
    const int j = (int)(r % P.nout);
    const int64_t wp = r / P.nout;
    const double2* row = P.fbuf + (wp * P.nt + t) * m;
    P.out[e] = select_lag(P, j, [&](int i) { return rmul(row[shift_source(i, m)], P.s); });
  }
}

// resampling.  LDS: z [nout][tile]
__global__ void __launch_bounds__(kThreads) k_runs_resample(RunParams P) {
  extern __shared__ double2 lds[];
  const int nout = P.nout, tile = P.tile;
  double2* z = lds;
  const int64_t pl = blockIdx.x / P.ntiles;
  const int t0 = (int)(blockIdx.x % P.ntiles) * tile;
  const int w = blockIdx.y;
  const int tcount = min(tile, P.nt - t0);
  for (int e = threadIdx.x; e < nout * tile; e += kThreads) {
    const int k = e / tile, tt = e - k * tile;
    double2 v = make_double2(0.0, 0.0);
    if (tt < tcount)
      v = resampled_bin([&](int i) { return row_value(P, pl, i, t0 + tt, w); }, P.rs_in, P.rs_c, nout, k);
    z[e] = v;
  }
  __syncthreads();
  const int32_t* kl = P.klist + P.kofs[w];
  const int nk = P.kofs[w + 1] - P.kofs[w];
  double2* dst = P.out + ((int64_t)w * P.pc + pl) * nout * P.nt + t0;
  for (int e = threadIdx.x; e < nout * tile; e += kThreads) {
    const int q = e / tile, tt = e - q * tile;
    const double2 acc = direct_sum<false>(z + tt, tile, kl, nk, q, nout, P.rtw);
    if (tt < tcount) dst[(int64_t)q * P.nt + tt] = acc;
  }
}

__device__ __forceinline__ float fmaf_or_fma(float a, float b, float c) { return fmaf(a, b, c); }
__device__ __forceinline__ double fmaf_or_fma(double a, double b, double c) { return fma(a, b, c); }

// power: out[e] = Re(a conj(b)) * factor[(e0 + e) / inner] (* 2).  numpy's complex product a * conj(b) has the real part
// ar br - ai (-bi); its SIMD loop fuses that into fma(ar, br, ai bi).  The complex64 product is rounded in fp32 and then widened.
template <typename T>
__global__ void __launch_bounds__(kThreads) k_runs_power(const T* a, const T* b, const double* factor, int64_t e0, int64_t n, int64_t inner,
                                                         int cross, int fused, double* out) {
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < n; e += (int64_t)gridDim.x * kThreads) {
    const T x = a[e], y = b[e];
    double p;
    if (fused) p = (double)fmaf_or_fma(x.x, y.x, x.y * y.y);
    else p = (double)(x.x * y.x + x.y * y.y);
    double v = p * factor[(e0 + e) / inner];
    if (cross) v = v * 2.0;
    out[e] = v;
  }
}

// ---- host side --------------------------------------------------------------------------------------------------------------

// elements a strided weight array spans (strides >= 0)
int64_t span_of(const int64_t* st, int64_t nbl, int64_t nchan, int64_t nt) {
  return (nbl - 1) * st[0] + (nchan - 1) * st[1] + (nt - 1) * st[2] + 1;
}

}  // namespace

extern "C" {

int prisim_runs_transform(prisim_ctx* ctx, int64_t R, int64_t nbl, int64_t nchan, int64_t nt, const void* vis, int32_t vis_is_c64,
                          const double* bp, const int64_t* bp_strides, const double* wts, const int64_t* wts_strides, int32_t nwin,
                          const double* win, int64_t m, double scale, int32_t out_mode, int64_t nout, double factor, int64_t nmap,
                          const int64_t* map_out, const int64_t* map_in, const double* map_w, int32_t route, int64_t budget_bytes,
                          double* out, prisim_runs_stats* stats) {
  return guarded(ctx, [&]() -> int {
  if (!ctx) return PRISIM_EINVAL;
  const WallTime wall0 = wall_now();
  if (m < 1 || m > PRISIM_RUNS_MAX_LEN)
    return fail(ctx, PRISIM_EINVAL, "delay spectra of runs take 1 to " + std::to_string(PRISIM_RUNS_MAX_LEN) +
                                        " lags (PRISIM_SUBBAND_MAX_LEN); got m = " + std::to_string(m));
  if (out_mode < PRISIM_RUNS_ALL || out_mode > PRISIM_RUNS_RESAMPLE) return fail(ctx, PRISIM_EINVAL, "unknown out_mode");
  if (out_mode == PRISIM_RUNS_ALL && nout != m) return fail(ctx, PRISIM_EINVAL, "out_mode PRISIM_RUNS_ALL writes nout == m lags");
  if (nout < 1 || nout > PRISIM_RUNS_MAX_LEN)
    return fail(ctx, PRISIM_EINVAL, "delay spectra of runs write 1 to " + std::to_string(PRISIM_RUNS_MAX_LEN) +
                                        " lags (PRISIM_SUBBAND_MAX_LEN); got nout = " + std::to_string(nout));
  if (out_mode == PRISIM_RUNS_INTERP && !(factor > 0.0 && (double)(nout - 1) * factor < (double)m + 1.0))
    return fail(ctx, PRISIM_EINVAL, "out_mode PRISIM_RUNS_INTERP needs factor > 0 and positions inside the m lags");
  if (R < 1 || nbl < 1 || nt < 1 || nchan < 1 || nchan > m || nwin < 1 || nwin > 65535 || (!win && nwin != 1))
    return fail(ctx, PRISIM_EINVAL, "need R, nbl, nt >= 1, 1 <= nchan <= m and 1 <= nwin <= 65535 (nwin == 1 without windows)");
  if (nt > (int64_t)1 << 30 || nchan > (int64_t)1 << 30) return fail(ctx, PRISIM_EINVAL, "nt and nchan must fit in 32 bits");
  if (!out || (bp && !bp_strides) || (wts && !wts_strides)) return fail(ctx, PRISIM_EINVAL, "null array");
  for (int i = 0; i < 3; ++i)
    if ((bp && bp_strides[i] < 0) || (wts && wts_strides[i] < 0)) return fail(ctx, PRISIM_EINVAL, "weight strides must be >= 0");
  if (route < PRISIM_RUNS_AUTO || route > PRISIM_RUNS_ROCFFT) return fail(ctx, PRISIM_EINVAL, "unknown route");
  bool pow2;
  const int logm = ceil_log2(m, pow2);
  const bool resample = out_mode == PRISIM_RUNS_RESAMPLE;
  if (route == PRISIM_RUNS_FUSED && !pow2 && !resample)
    return fail(ctx, PRISIM_EINVAL, "the fused route takes power-of-two m; got m = " + std::to_string(m));
  const int rt = resample ? PRISIM_RUNS_DIRECT : (route == PRISIM_RUNS_ROCFFT || (route == PRISIM_RUNS_AUTO && !pow2))
                                                    ? PRISIM_RUNS_ROCFFT : PRISIM_RUNS_FUSED;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (rt == PRISIM_RUNS_ROCFFT)
    if (int rc = ensure_rocfft(ctx)) return rc;

  // the resampling tables: per output bin at most two input bins (padding bins dropped), and per window the bins it can make nonzero
  ResampleTables rs;
  std::vector<int32_t> klist, kofs;
  std::vector<double> rs_c;
  const double s = scale / (double)m;
  if (resample) {
    if (int rc = build_resample_tables(ctx, nout, m, nchan, s, nmap, map_out, map_in, map_w, rs, &rs_c)) return rc;
    fed_bins(rs, nout, nwin, nchan, win, Feeds::kSpan, kofs, klist);
  }

  // snapshot tile, LDS and chunking
  int lds_max = 0;
  if (int rc = lds_limit(ctx, lds_max)) return rc;
  SnapshotTile sn = {1, nt, 0};                       // rocFFT route: no tiled kernel
  if (rt == PRISIM_RUNS_FUSED) sn = snapshot_tile(nt, 16 * m, 16 * std::max<int64_t>(m / 2, 1));
  if (rt == PRISIM_RUNS_DIRECT) sn = snapshot_tile(nt, 16 * nout, 0);
  const int64_t tile = sn.tile, ntiles = sn.ntiles, lds = sn.lds;
  if (lds > lds_max) return fail(ctx, PRISIM_EINVAL, "rows do not fit in LDS (" + std::to_string(lds) + " B needed)");
  const int64_t P = R * nbl;
  const int64_t in_pair = vis ? nchan * nt * (vis_is_c64 ? 8 : 16) : 0;
  const int64_t out_pair = (int64_t)nwin * nout * nt * 16;
  const int64_t fbuf_pair = rt == PRISIM_RUNS_ROCFFT ? (int64_t)nwin * nt * m * 16 : 0;
  const int64_t per_pair = in_pair + out_pair + fbuf_pair;
  const int64_t fit = plan_chunks(P, per_pair, budget_bytes, kMaxStreams).size;
  const int64_t grid_max = ((int64_t)1 << 31) / std::max<int64_t>(ntiles, 1) - 1;          // grid x of the tiled kernels
  const Chunks ch = chunks_of(P, std::min(fit, grid_max), kMaxStreams);
  const int64_t pc = ch.size, nchunks = ch.count;
  const int nstreams = ch.nstreams;

  // the tables go up on stream 0 as they are allocated; stream 1 waits for them
  Work wk;
  Streams& st = wk.st;
  if (int rc = st.create(ctx, nstreams, false)) return rc;
  hipStream_t s0 = st.s[0];
  const int64_t bp_n = bp ? span_of(bp_strides, nbl, nchan, nt) : 0, wts_n = wts ? span_of(wts_strides, nbl, nchan, nt) : 0;
  double *d_bp = nullptr, *d_wts = nullptr, *d_win = nullptr;
  ResampleDev rd;
  if (bp) DEV_UPLOAD(ctx, wk.dev, d_bp, bp, (size_t)bp_n, s0);
  if (wts) DEV_UPLOAD(ctx, wk.dev, d_wts, wts, (size_t)wts_n, s0);
  if (win) DEV_UPLOAD(ctx, wk.dev, d_win, win, (size_t)nwin * nchan, s0);
  if (resample)
    if (int rc = upload_resample(ctx, wk.dev, rd, rs.in, rs_c, rs.rtw, kofs, klist, s0)) return rc;
  void* d_in[kMaxStreams] = {};
  double2* d_out[kMaxStreams] = {};
  double2* d_fbuf[kMaxStreams] = {};
  for (int i = 0; i < nstreams; ++i) {
    if (vis) DEV_ALLOC(ctx, wk.dev, d_in[i], pc * in_pair);
    DEV_ALLOC(ctx, wk.dev, d_out[i], pc * out_pair);
    if (fbuf_pair) DEV_ALLOC(ctx, wk.dev, d_fbuf[i], pc * fbuf_pair);
  }
  if (rt == PRISIM_RUNS_ROCFFT) {
    const size_t lines = (size_t)nwin * (size_t)nt;
    if (int rc = wk.fft.create(ctx, wk.dev, (size_t)m, {{true, lines * (size_t)pc}, {true, lines * (size_t)ch.last}}, st.s, nstreams)) return rc;
  }
  HIPCHK(ctx, hipStreamSynchronize(s0));            // the tables are host vectors of this call and caller memory

  RunParams base;
  base.vis = nullptr; base.c64 = vis_is_c64 != 0;
  base.bp = d_bp; base.bs0 = bp ? bp_strides[0] : 0; base.bs1 = bp ? bp_strides[1] : 0; base.bs2 = bp ? bp_strides[2] : 0;
  base.wts = d_wts; base.ws0 = wts ? wts_strides[0] : 0; base.ws1 = wts ? wts_strides[1] : 0; base.ws2 = wts ? wts_strides[2] : 0;
  base.win = d_win;
  base.nwin = nwin; base.nchan = (int)nchan; base.nt = (int)nt; base.m = (int)m; base.logm = logm; base.nout = (int)nout;
  base.mode = out_mode; base.tile = (int)tile; base.ntiles = (int)ntiles;
  base.nbl = nbl; base.p0 = 0; base.pc = 0; base.s = s; base.factor = factor;
  base.rs_in = rd.in; base.rs_c = rd.c; base.rtw = rd.rtw; base.klist = rd.list; base.kofs = rd.ofs;
  base.out = nullptr; base.fbuf = nullptr;
  if (rt == PRISIM_RUNS_FUSED)
    if (int rc = allow_lds(ctx, k_runs_fused, lds)) return rc;
  if (rt == PRISIM_RUNS_DIRECT)
    if (int rc = allow_lds(ctx, k_runs_resample, lds)) return rc;

  auto upload = [&](int64_t, Span sp, int i, hipStream_t sc) -> int {
    if (vis) HIPCHK(ctx, hipMemcpyAsync(d_in[i], (const char*)vis + (size_t)sp.first * (size_t)in_pair, (size_t)sp.count * in_pair,
                                        hipMemcpyHostToDevice, sc));
    return PRISIM_OK;
  };
  auto kernels = [&](int64_t, Span sp, int i, hipStream_t sc) -> int {
    const int64_t pn = sp.count;
    RunParams Pm = base;
    Pm.p0 = sp.first; Pm.pc = pn; Pm.out = d_out[i]; Pm.fbuf = d_fbuf[i];
    if (vis) Pm.vis = d_in[i];
    if (rt == PRISIM_RUNS_FUSED) {
      if (int rc = launch(ctx, k_runs_fused, dim3((unsigned)(pn * ntiles), (unsigned)nwin), (size_t)lds, sc, Pm)) return rc;
    } else if (rt == PRISIM_RUNS_DIRECT) {
      if (int rc = launch(ctx, k_runs_resample, dim3((unsigned)(pn * ntiles), (unsigned)nwin), (size_t)lds, sc, Pm)) return rc;
    } else {
      const int64_t nf = (int64_t)nwin * pn * nt * m, no = (int64_t)nwin * pn * nout * nt;
      if (int rc = launch(ctx, k_runs_prepare, dim3((unsigned)grid_for(ctx, nf)), 0, sc, Pm)) return rc;
      if (int rc = wk.fft.run(ctx, true, (size_t)nwin * (size_t)nt * (size_t)pn, d_fbuf[i], i)) return rc;
      if (int rc = launch(ctx, k_runs_finish, dim3((unsigned)grid_for(ctx, no)), 0, sc, Pm)) return rc;
    }
    return PRISIM_OK;
  };
  auto download = [&](int64_t, Span sp, int i, hipStream_t sc) -> int {
    const size_t blk = (size_t)sp.count * nout * nt;  // complex elements of one window's block
    for (int w = 0; w < nwin; ++w)
      HIPCHK(ctx, hipMemcpyAsync(out + 2 * (((size_t)w * P + sp.first) * nout * nt), d_out[i] + (size_t)w * blk, blk * 16,
                                 hipMemcpyDeviceToHost, sc));
    return PRISIM_OK;
  };
  if (int rc = chunk_loop(ctx, st, ch, P, upload, kernels, download)) return rc;
  if (stats) {
    stats->wall_ms = wall_ms_since(wall0);
    stats->pairs = P;
    stats->chunks = nchunks;
    stats->chunk_pairs = pc;
    stats->route = rt;
    stats->streams = nstreams;
    stats->tile = (int32_t)tile;
    stats->lds_bytes = (int32_t)lds;
  }
  return PRISIM_OK;
  });
}

int prisim_runs_power(prisim_ctx* ctx, int64_t nf, int64_t inner, const void* v1, const void* v2, int32_t is_c64, const double* factor,
                      int32_t cross, int32_t fused_product, int64_t budget_bytes, double* out, prisim_runs_stats* stats) {
  return guarded(ctx, [&]() -> int {
  if (!ctx) return PRISIM_EINVAL;
  const WallTime wall0 = wall_now();
  if (nf < 1 || inner < 1) return fail(ctx, PRISIM_EINVAL, "need nf >= 1 and inner >= 1");
  if (!v1 || !factor || !out) return fail(ctx, PRISIM_EINVAL, "null array");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const int64_t n = nf * inner;
  const int64_t esz = is_c64 ? 8 : 16;
  const int64_t per = esz * (v2 ? 2 : 1) + 8;
  const Chunks ch = plan_chunks(n, per, budget_bytes, kMaxStreams);
  const int64_t ce = ch.size, nchunks = ch.count;
  const int nstreams = ch.nstreams;
  Work wk;
  Streams& st = wk.st;
  if (int rc = st.create(ctx, nstreams, false)) return rc;
  double* d_f;
  DEV_UPLOAD(ctx, wk.dev, d_f, factor, (size_t)nf, st.s[0]);
  void* d_a[kMaxStreams] = {};
  void* d_b[kMaxStreams] = {};
  double* d_o[kMaxStreams] = {};
  for (int i = 0; i < nstreams; ++i) {
    DEV_ALLOC(ctx, wk.dev, d_a[i], ce * esz);
    if (v2) DEV_ALLOC(ctx, wk.dev, d_b[i], ce * esz);
    DEV_ALLOC(ctx, wk.dev, d_o[i], ce * 8);
  }
  HIPCHK(ctx, hipStreamSynchronize(st.s[0]));
  auto upload = [&](int64_t, Span sp, int i, hipStream_t sc) -> int {
    const int64_t e0 = sp.first, en = sp.count;
    HIPCHK(ctx, hipMemcpyAsync(d_a[i], (const char*)v1 + e0 * esz, en * esz, hipMemcpyHostToDevice, sc));
    if (v2) HIPCHK(ctx, hipMemcpyAsync(d_b[i], (const char*)v2 + e0 * esz, en * esz, hipMemcpyHostToDevice, sc));
    return PRISIM_OK;
  };
  auto kernels = [&](int64_t, Span sp, int i, hipStream_t sc) -> int {
    const int64_t e0 = sp.first, en = sp.count;
    const void* b = v2 ? d_b[i] : d_a[i];
    const dim3 grid((unsigned)grid_for(ctx, en));
    if (is_c64)
      return launch(ctx, k_runs_power<float2>, grid, 0, sc, (const float2*)d_a[i], (const float2*)b, (const double*)d_f, e0, en, inner,
                    (int)(cross != 0), (int)(fused_product != 0), d_o[i]);
    return launch(ctx, k_runs_power<double2>, grid, 0, sc, (const double2*)d_a[i], (const double2*)b, (const double*)d_f, e0, en, inner,
                  (int)(cross != 0), (int)(fused_product != 0), d_o[i]);
  };
  auto download = [&](int64_t, Span sp, int i, hipStream_t sc) -> int {
    HIPCHK(ctx, hipMemcpyAsync(out + sp.first, d_o[i], sp.count * 8, hipMemcpyDeviceToHost, sc));
    return PRISIM_OK;
  };
  if (int rc = chunk_loop(ctx, st, ch, n, upload, kernels, download)) return rc;
  if (stats) {
    stats->wall_ms = wall_ms_since(wall0);
    stats->pairs = n;
    stats->chunks = nchunks;
    stats->chunk_pairs = ce;
    stats->route = PRISIM_RUNS_DIRECT;
    stats->streams = nstreams;
    stats->tile = 0;
    stats->lds_bytes = 0;
  }
  return PRISIM_OK;
  });
}

}  // extern "C"
