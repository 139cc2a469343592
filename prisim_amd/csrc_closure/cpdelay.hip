// cpdelay.hip -- delay spectra of closure phases and their power spectra for gfx950 (include/prisim_cpdelay.h):
// prisim/delay_spectrum.py:subband_delay_transform_closure_phase (:2932-2962) and the arithmetic of
// compute_individual_closure_phase_power_spectrum (:4346) / compute_averaged_closure_phase_power_spectrum (:4536-4538).
//
// The phases of a chunk of rows lie on the device as [row][nchan][nt], snapshot-fastest: uploaded by this file's loop, or left there by
// closure.hip's loop (closure_internal.h), which then calls this file's kernels as its sink -- no triplet and no phase crosses the
// host link on that path.  The outputs are snapshot-fastest too, [row][window][lag][nt], while the transform runs along the lags.
// The transform, the shift, the resampled bins, their direct sum and the power are csrc_addon/delay_lines.h's.  Particular to this file:
//   k_cpd_fused (m a power of two): one workgroup per (row, window, tile of snapshots).  x = (cos phi, -sin phi) wts is read, and the
//     spectrum written, along the snapshots; the LDS rows are m + 1 double2 (16 (m + 1) bytes: lane k of a snapshot-fastest access starts
//     at bank 4 k mod 64, so the 16 lanes a 128-bit access serves together touch 16 different 16-byte slots).
//   rocFFT route (any other m): k_cpd_prepare turns [ch][t] into the padded rows [line][t][m] through a [32][33] double2 LDS tile
//     (closure.hip's k_cl_tiled pattern) -> batched inverse rocFFT in place -> k_cpd_finish shifts, scales by df and turns back.
//   k_cpd_resample (both routes): the host folds wts, df and the map's weights into one coefficient per (window, kept bin, term) and
//     drops the bins whose channels the window zeroes; one workgroup per (row, window, tile of snapshots)
//     forms the kept Y in LDS and sums them.
//   k_cpp_accumulate / k_cpp_finish: the power spectra; every thread owns points of the contiguous trailing axes, loops over the
//     chunk's entries of axis 0 and keeps sum |x|^2 and sum x in device arrays between chunks.  No atomics.
// Chunks of rows alternate between two streams with their own buffers, as in closure.hip.
// fp64 throughout, built with -ffp-contract=off.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "closure_internal.h"
#include "../csrc_addon/delay_lines.h"
#include "../../include/prisim_cpdelay.h"

namespace {

constexpr int kTile = 32;                             // turning kernels of the rocFFT route: lags and snapshots per tile
constexpr int64_t kMaxGrid = (int64_t(1) << 31) - 1;

struct CdParams {
  const double* phase;      // this chunk's [rows][nchan][nt]
  const double* wts;        // [nwin][nchan]
  const double* pscale;     // [nwin], or null
  int nwin, nchan, nt, m, logm, nres;
  int tile, ntiles;         // fused: snapshots per workgroup, tiles per line
  int rtile, rntiles;       // resampling: the same
  double df;
  const int32_t* rs_o;      // [nwin + 1] kept bins of the resampled spectrum: rs_k[rs_o[w] .. rs_o[w + 1]), increasing
  const int32_t* rs_k;
  const int32_t* rs_in;     // [nwin][2][nres] their channels, by kept bin (-1: none)
  const double2* rs_c;      // [nwin][2][nres] wts * weight * df e^{-2 pi i k_in floor(m/2) / m}
  const double2* rtw;       // [nres] e^{+2 pi i q / nres}
  double2* over;            // this chunk's [rows][nwin][m][nt]
  double* over_pow;
  double2* res;             // this chunk's [rows][nwin][nres][nt]
  double* res_pow;
  double2* fbuf;            // rocFFT route: [rows][nwin][nt][m]
};

// exp(-i phi)
__device__ __forceinline__ double2 phasor(double phi) {
  double s, c;
  sincos(phi, &s, &c);
  return make_double2(c, -s);
}

// fused route.  grid: x = (line - line0) * ntiles + (snapshot tile), line = row * nwin + window.  LDS: buf [tile][m + 1] | tw [m / 2]
__global__ void __launch_bounds__(kThreads) k_cpd_fused(CdParams P, int64_t line0) {
  extern __shared__ double2 lds[];
  const int m = P.m, ld = m + 1, tile = P.tile;
  double2* buf = lds;
  double2* tw = buf + (int64_t)tile * ld;
  const int64_t line = line0 + blockIdx.x / P.ntiles;
  const int t0 = (int)(blockIdx.x % P.ntiles) * tile;
  const int tcount = min(tile, P.nt - t0);
  const int64_t row = line / P.nwin;
  const int w = (int)(line - row * P.nwin);
  const double* ph = P.phase + row * (int64_t)P.nchan * P.nt + t0;
  const double* wt = P.wts + (int64_t)w * P.nchan;
  lds_twiddles(tw, m);
  for (int e = threadIdx.x; e < m * tile; e += kThreads) {             // lanes along the snapshots
    const int n = e / tile, tt = e - n * tile;
    LdsOperand x = shifted_zero(n, P.logm);
    if (n < P.nchan && tt < tcount) {
      const double wv = wt[n];
      if (wv != 0.0) x = shifted_operand(rmul(phasor(ph[(int64_t)n * P.nt + tt]), wv), n, m, P.logm, P.df);
    }
    buf[tt * ld + x.slot] = x.v;
  }
  __syncthreads();
  lds_ifft_dit(buf, ld, tile, m, tw);
  const int64_t o = line * m * (int64_t)P.nt + t0;
  const double ps = P.pscale ? P.pscale[w] : 0.0;
  for (int e = threadIdx.x; e < m * tile; e += kThreads) {
    const int j = e / tile, tt = e - j * tile;
    if (tt < tcount) {
      const double2 v = buf[tt * ld + j];
      if (P.over) P.over[o + (int64_t)j * P.nt + tt] = v;
      if (P.over_pow) P.over_pow[o + (int64_t)j * P.nt + tt] = power_of(v, ps);
    }
  }
}

// rocFFT route, before the transform.  grid: x = ((line - line0) * nct + (lag tile)) * ntt + (snapshot tile)
__global__ void __launch_bounds__(kThreads) k_cpd_prepare(CdParams P, int64_t line0, int nct, int ntt) {
  __shared__ double2 tile[kTile][kTile + 1];
  const int64_t line = line0 + blockIdx.x / ((int64_t)nct * ntt);
  const int rem = (int)(blockIdx.x % ((int64_t)nct * ntt));
  const int c0 = (rem / ntt) * kTile, t0 = (rem % ntt) * kTile;
  const int lx = threadIdx.x % kTile, ly = threadIdx.x / kTile;      // ly < 8
  const int64_t row = line / P.nwin;
  const int w = (int)(line - row * P.nwin);
  const double* ph = P.phase + row * (int64_t)P.nchan * P.nt;
  const double* wt = P.wts + (int64_t)w * P.nchan;
#pragma unroll
  for (int i = 0; i < kTile / 8; ++i) {                                // lanes along the snapshots
    const int cc = ly + 8 * i, n = c0 + cc, t = t0 + lx;
    double2 v = make_double2(0.0, 0.0);
    if (n < P.nchan && t < P.nt) {
      const double wv = wt[n];
      if (wv != 0.0) v = rmul(phasor(ph[(int64_t)n * P.nt + t]), wv);
    }
    tile[cc][lx] = v;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < kTile / 8; ++i) {                                // lanes along the lags
    const int tt = ly + 8 * i, n = c0 + lx, t = t0 + tt;
    if (n < P.m && t < P.nt) P.fbuf[(line * P.nt + t) * P.m + n] = tile[lx][tt];
  }
}

// rocFFT route, after the unnormalised inverse transform: transform bin jf scatters to its lag.  grid as k_cpd_prepare
__global__ void __launch_bounds__(kThreads) k_cpd_finish(CdParams P, int64_t line0, int nct, int ntt) {
  __shared__ double2 tile[kTile][kTile + 1];
  const int64_t line = line0 + blockIdx.x / ((int64_t)nct * ntt);
  const int rem = (int)(blockIdx.x % ((int64_t)nct * ntt));
  const int c0 = (rem / ntt) * kTile, t0 = (rem % ntt) * kTile;
  const int lx = threadIdx.x % kTile, ly = threadIdx.x / kTile;
  const int w = (int)(line % P.nwin);
#pragma unroll
  for (int i = 0; i < kTile / 8; ++i) {                                // lanes along the lags
    const int tt = ly + 8 * i, jf = c0 + lx, t = t0 + tt;
    if (jf < P.m && t < P.nt) tile[tt][lx] = P.fbuf[(line * P.nt + t) * P.m + jf];
  }
  __syncthreads();
  const double ps = P.pscale ? P.pscale[w] : 0.0;
#pragma unroll
  for (int i = 0; i < kTile / 8; ++i) {                                // lanes along the snapshots
    const int cc = ly + 8 * i, jf = c0 + cc, t = t0 + lx;
    if (jf < P.m && t < P.nt) {
      const double2 v = rmul(tile[lx][cc], P.df);
      const int64_t o = (line * P.m + shift_target(jf, P.m)) * P.nt + t;
      if (P.over) P.over[o] = v;
      if (P.over_pow) P.over_pow[o] = power_of(v, ps);
    }
  }
}

// resampled spectra.  grid: x = (line - line0) * rntiles + (snapshot tile).  LDS: Y [nres][rtile]
__global__ void __launch_bounds__(kThreads) k_cpd_resample(CdParams P, int64_t line0) {
  extern __shared__ double2 lds[];
  double2* Y = lds;
  const int nres = P.nres, tile = P.rtile;
  const int64_t line = line0 + blockIdx.x / P.rntiles;
  const int t0 = (int)(blockIdx.x % P.rntiles) * tile;
  const int tcount = min(tile, P.nt - t0);
  const int64_t row = line / P.nwin;
  const int w = (int)(line - row * P.nwin);
  const double* ph = P.phase + row * (int64_t)P.nchan * P.nt + t0;
  const int nz = P.rs_o[w + 1] - P.rs_o[w];
  const int32_t* kin = P.rs_in + (int64_t)w * 2 * nres;
  const double2* coef = P.rs_c + (int64_t)w * 2 * nres;
  const int32_t* kout = P.rs_k + P.rs_o[w];
  for (int e = threadIdx.x; e < nz * tile; e += kThreads) {            // lanes along the snapshots
    const int i = e / tile, tt = e - i * tile;
    double2 v = make_double2(0.0, 0.0);
    if (tt < tcount)                                                   // the window's own tables, by kept bin
      v = resampled_bin([&](int ch) { return phasor(ph[(int64_t)ch * P.nt + tt]); }, kin, coef, nres, i);
    Y[i * tile + tt] = v;
  }
  __syncthreads();
  const int64_t o = line * nres * (int64_t)P.nt + t0;
  const double ps = P.pscale ? P.pscale[w] : 0.0;
  for (int e = threadIdx.x; e < nres * tile; e += kThreads) {
    const int q = e / tile, tt = e - q * tile;
    if (tt >= tcount) continue;
    const double2 acc = direct_sum<true>(Y + tt, tile, kout, nz, q, nres, P.rtw);
    if (P.res) P.res[o + (int64_t)q * P.nt + tt] = acc;
    if (P.res_pow) P.res_pow[o + (int64_t)q * P.nt + tt] = power_of(acc, ps);
  }
}

// power spectra: x [rows][npts] of this chunk, point p = w * inner + (lag, snapshot)
__global__ void __launch_bounds__(kThreads) k_cpp_accumulate(const double2* x, int64_t rows, int64_t npts, int64_t inner, const double* scale,
                                                             double* individual, double* sumsq, double2* sum) {
  for (int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x; p < npts; p += (int64_t)gridDim.x * kThreads) {
    const double sc = scale[p / inner];
    double a = sumsq ? sumsq[p] : 0.0;
    double2 s = sum ? sum[p] : make_double2(0.0, 0.0);
    for (int64_t r = 0; r < rows; ++r) {
      const double2 v = x[r * npts + p];
      const double q = v.x * v.x + v.y * v.y;
      if (individual) individual[r * npts + p] = q * sc;
      a += q;
      s = cadd(s, v);
    }
    if (sumsq) sumsq[p] = a;
    if (sum) sum[p] = s;
  }
}

__global__ void __launch_bounds__(kThreads) k_cpp_finish(int64_t n0, int64_t npts, int64_t inner, const double* scale, const double* sumsq,
                                                         const double2* sum, double* out_auto, double* out_cross) {
  for (int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x; p < npts; p += (int64_t)gridDim.x * kThreads) {
    const double sc = scale[p / inner], n = (double)n0;
    const double au = (sumsq[p] / n) * sc;
    if (out_auto) out_auto[p] = au;
    if (out_cross) {
      const double2 s = sum[p];
      out_cross[p] = (1.0 / (n * (n - 1.0))) * (sc * (s.x * s.x + s.y * s.y) - n * au);
    }
  }
}

// ---- host side --------------------------------------------------------------------------------------------------------------

// the transform of the chunks: the tables, the per-stream output buffers, the launches and the downloads
struct Transform {
  prisim_ctx* ctx;
  int64_t nchan, nt, m, nres;
  int nwin, logm;
  bool fused, w_over, w_opow, w_res, w_rpow;
  int64_t tile = 0, ntiles = 1, lds = 0, rtile = 0, rntiles = 1, rlds = 0;
  double *over, *over_pow, *res, *res_pow;          // the caller's
  Work wk;                                          // st: the streams of the phases form; from a cube, closure.hip's loop has its own
  CdParams base;
  double2 *d_over[kMaxStreams] = {}, *d_res[kMaxStreams] = {}, *d_fbuf[kMaxStreams] = {};
  double *d_opow[kMaxStreams] = {}, *d_rpow[kMaxStreams] = {};
  // the host tables, formed before any device work
  std::vector<int32_t> rs_o, rs_k, rs_in;
  std::vector<double> rs_c, rtw;
  const double *wts, *pscale;
  double df;

  bool want_over() const { return w_over || w_opow; }
  bool want_res() const { return w_res || w_rpow; }

  int64_t bytes_per_row() const {
    const int64_t lines = (int64_t)nwin * nt;
    return lines * (m * (16 * (int64_t)w_over + 8 * (int64_t)w_opow + ((!fused && want_over()) ? 16 : 0)) +
                    nres * (16 * (int64_t)w_res + 8 * (int64_t)w_rpow));
  }

  int64_t download_per_row() const {
    return (int64_t)nwin * nt * (m * (16 * (int64_t)w_over + 8 * (int64_t)w_opow) + nres * (16 * (int64_t)w_res + 8 * (int64_t)w_rpow));
  }

  int prepare(int64_t tc, int64_t last, int nstreams, const hipStream_t* streams) {
    const int64_t lines = tc * nwin * nt;
    double *d_wts, *d_ps = nullptr;
    ResampleDev rd;
    hipStream_t s0 = streams[0];
    DEV_UPLOAD(ctx, wk.dev, d_wts, wts, (size_t)nwin * nchan, s0);
    if (pscale) DEV_UPLOAD(ctx, wk.dev, d_ps, pscale, (size_t)nwin, s0);
    if (int rc = upload_resample(ctx, wk.dev, rd, rs_in, rs_c, rtw, rs_o, rs_k, s0)) return rc;
    for (int i = 0; i < nstreams; ++i) {
      if (w_over) DEV_ALLOC(ctx, wk.dev, d_over[i], (size_t)lines * m * 16);
      if (w_opow) DEV_ALLOC(ctx, wk.dev, d_opow[i], (size_t)lines * m * 8);
      if (w_res) DEV_ALLOC(ctx, wk.dev, d_res[i], (size_t)lines * nres * 16);
      if (w_rpow) DEV_ALLOC(ctx, wk.dev, d_rpow[i], (size_t)lines * nres * 8);
      if (!fused && want_over()) DEV_ALLOC(ctx, wk.dev, d_fbuf[i], (size_t)lines * m * 16);
    }
    if (!fused && want_over()) {
      const size_t per_row = (size_t)nwin * (size_t)nt;
      if (int rc = wk.fft.create(ctx, wk.dev, (size_t)m, {{true, per_row * (size_t)tc}, {true, per_row * (size_t)last}}, streams, nstreams)) return rc;
    }
    HIPCHK(ctx, hipStreamSynchronize(s0));          // the other stream starts behind the tables
    base.phase = nullptr;
    base.wts = d_wts; base.pscale = d_ps;
    base.nwin = nwin; base.nchan = (int)nchan; base.nt = (int)nt; base.m = (int)m; base.logm = logm; base.nres = (int)std::max<int64_t>(nres, 1);
    base.tile = (int)tile; base.ntiles = (int)ntiles; base.rtile = (int)rtile; base.rntiles = (int)rntiles;
    base.df = df;
    base.rs_o = rd.ofs; base.rs_k = rd.list; base.rs_in = rd.in; base.rs_c = rd.c; base.rtw = rd.rtw;
    base.over = nullptr; base.over_pow = nullptr; base.res = nullptr; base.res_pow = nullptr; base.fbuf = nullptr;
    if (fused && want_over())
      if (int rc = allow_lds(ctx, k_cpd_fused, lds)) return rc;
    return want_res() ? allow_lds(ctx, k_cpd_resample, rlds) : PRISIM_OK;
  }

  // `kernel` over `lines` lines of `per_line` workgroups each, in as many launches as the grid's x extent asks for
  template <typename K, typename... A>
  int launch_lines(K kernel, int64_t lines, int64_t per_line, size_t lds_bytes, hipStream_t s, const CdParams& P, A... a) {
    const int64_t step = std::max<int64_t>(1, kMaxGrid / per_line);
    for (int64_t l0 = 0; l0 < lines; l0 += step) {
      if (int rc = launch(ctx, kernel, dim3((unsigned)(std::min(step, lines - l0) * per_line)), lds_bytes, s, P, l0, a...)) return rc;
    }
    return PRISIM_OK;
  }

  int kernels(int i, hipStream_t s, int64_t tn, const double* d_phase) {
    CdParams P = base;
    P.phase = d_phase;
    P.over = d_over[i]; P.over_pow = d_opow[i]; P.res = d_res[i]; P.res_pow = d_rpow[i]; P.fbuf = d_fbuf[i];
    const int64_t lines = tn * nwin;
    if (want_over()) {
      if (fused) {
        if (int rc = launch_lines(k_cpd_fused, lines, ntiles, (size_t)lds, s, P)) return rc;
      } else {
        const int64_t nct = (m + kTile - 1) / kTile, ntt = (nt + kTile - 1) / kTile;
        if (int rc = launch_lines(k_cpd_prepare, lines, nct * ntt, 0, s, P, (int)nct, (int)ntt)) return rc;
        if (int rc = wk.fft.run(ctx, true, (size_t)lines * (size_t)nt, d_fbuf[i], i)) return rc;
        if (int rc = launch_lines(k_cpd_finish, lines, nct * ntt, 0, s, P, (int)nct, (int)ntt)) return rc;
      }
    }
    return want_res() ? launch_lines(k_cpd_resample, lines, rntiles, (size_t)rlds, s, P) : PRISIM_OK;
  }

  int download(int i, hipStream_t s, int64_t T0, int64_t tn) {
    const size_t no = (size_t)tn * nwin * m * nt, nr = (size_t)tn * nwin * nres * nt;
    const size_t oo = (size_t)T0 * nwin * m * nt, orr = (size_t)T0 * nwin * nres * nt;
    if (w_over) HIPCHK(ctx, hipMemcpyAsync(over + 2 * oo, d_over[i], no * 16, hipMemcpyDeviceToHost, s));
    if (w_opow) HIPCHK(ctx, hipMemcpyAsync(over_pow + oo, d_opow[i], no * 8, hipMemcpyDeviceToHost, s));
    if (w_res) HIPCHK(ctx, hipMemcpyAsync(res + 2 * orr, d_res[i], nr * 16, hipMemcpyDeviceToHost, s));
    if (w_rpow) HIPCHK(ctx, hipMemcpyAsync(res_pow + orr, d_rpow[i], nr * 8, hipMemcpyDeviceToHost, s));
    return PRISIM_OK;
  }
};

}  // namespace

extern "C" {

int prisim_closure_delay_spectra(prisim_ctx* ctx, const double* phases, int64_t nrows, const double* cube, int64_t nt, int64_t nbl,
                                 int64_t nchan, const int32_t* legs, const int32_t* conj, const double* freq_wts, const double* bpwts,
                                 const double* masks, int64_t nmask, const int32_t* mask_index, int32_t phase_route, int32_t nwin,
                                 const double* wts, int64_t m, double df, int64_t nres, int64_t nmap, const int64_t* map_out,
                                 const int64_t* map_in, const double* map_w, const double* pscale, int32_t want, int32_t route,
                                 int64_t budget_bytes, double* out_phase, double* over, double* over_pow, double* res, double* res_pow,
                                 prisim_cpdelay_stats* stats) {
  return guarded(ctx, [&]() -> int {
  if (!ctx) return PRISIM_EINVAL;
  const WallTime wall0 = wall_now();
  if (m < 1 || m > PRISIM_CPDELAY_MAX_LEN)
    return fail(ctx, PRISIM_EINVAL, "closure-phase delay spectra take 1 to " + std::to_string(PRISIM_CPDELAY_MAX_LEN) +
                                        " lags (PRISIM_CPDELAY_MAX_LEN); got m = " + std::to_string(m));
  Transform tr;
  tr.ctx = ctx;
  tr.w_over = want & PRISIM_CPDELAY_OVER; tr.w_opow = want & PRISIM_CPDELAY_OVER_POWER;
  tr.w_res = want & PRISIM_CPDELAY_RES; tr.w_rpow = want & PRISIM_CPDELAY_RES_POWER;
  if (tr.want_res() && (nres < 1 || nres > PRISIM_CPDELAY_MAX_LEN))
    return fail(ctx, PRISIM_EINVAL, "resampled closure-phase delay spectra take 1 to " + std::to_string(PRISIM_CPDELAY_MAX_LEN) +
                                        " lags (PRISIM_CPDELAY_MAX_LEN); got nres = " + std::to_string(nres));
  if (!tr.want_res()) nres = 0;
  if (nrows < 1 || nt < 1 || nchan < 1 || nchan > m || nwin < 1)
    return fail(ctx, PRISIM_EINVAL, "need nrows >= 1, nt >= 1, nwin >= 1 and 1 <= nchan <= m");
  if (nt > (int64_t)1 << 30) return fail(ctx, PRISIM_EINVAL, "nt must fit in 32 bits");
  if (!(tr.want_over() || tr.want_res())) return fail(ctx, PRISIM_EINVAL, "nothing requested (want)");
  if (!wts || (tr.w_over && !over) || (tr.w_opow && !over_pow) || (tr.w_res && !res) || (tr.w_rpow && !res_pow) ||
      ((tr.w_opow || tr.w_rpow) && !pscale))
    return fail(ctx, PRISIM_EINVAL, "null array");
  if (route < PRISIM_CPDELAY_AUTO || route > PRISIM_CPDELAY_ROCFFT) return fail(ctx, PRISIM_EINVAL, "unknown route");
  bool pow2;
  const int logm = ceil_log2(m, pow2);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int lds_max = 0;
  if (int rc = lds_limit(ctx, lds_max)) return rc;
  const SnapshotTile ft = snapshot_tile(nt, 16 * (m + 1), 16 * std::max<int64_t>(m / 2, 1));
  const int64_t flds = ft.lds;
  const bool fused_ok = pow2 && flds <= lds_max;
  if (route == PRISIM_CPDELAY_FUSED && !fused_ok)
    return fail(ctx, PRISIM_EINVAL, "the fused route takes a power-of-two m whose rows fit in LDS (" + std::to_string(flds) +
                                        " B needed); got m = " + std::to_string(m));
  tr.fused = route == PRISIM_CPDELAY_FUSED || (route == PRISIM_CPDELAY_AUTO && fused_ok);
  tr.nchan = nchan; tr.nt = nt; tr.m = m; tr.nres = nres; tr.nwin = nwin; tr.logm = logm;
  tr.over = over; tr.over_pow = over_pow; tr.res = res; tr.res_pow = res_pow;
  tr.wts = wts; tr.pscale = (tr.w_opow || tr.w_rpow) ? pscale : nullptr; tr.df = df;
  if (tr.fused) {
    tr.tile = ft.tile; tr.ntiles = ft.ntiles; tr.lds = flds;
  } else {
    tr.lds = (int64_t)sizeof(double2) * kTile * (kTile + 1);
  }
  if (tr.want_res()) {
    const SnapshotTile rt = snapshot_tile(nt, 16 * nres, 0);
    tr.rtile = rt.tile; tr.rntiles = rt.ntiles; tr.rlds = rt.lds;
    if (tr.rlds > lds_max) return fail(ctx, PRISIM_EINVAL, "a resampled row does not fit in LDS");
  }
  if (!tr.fused && tr.want_over()) {
    if (int rc = ensure_rocfft(ctx)) return rc;
  }

  // the resampling tables: per window, the output bins that some nonzero channel of the window feeds, and their terms compacted,
  // with the window's weight folded into the coefficient
  const int64_t nr = std::max<int64_t>(nres, 1);
  ResampleTables rs;
  if (int rc = build_resample_tables(ctx, nres, m, nchan, df, nmap, map_out, map_in, map_w, rs, nullptr)) return rc;
  fed_bins(rs, nres, nwin, nchan, wts, Feeds::kNonzero, tr.rs_o, tr.rs_k);
  tr.rs_in.assign((size_t)nwin * 2 * nr, -1);
  tr.rs_c.assign((size_t)nwin * 4 * nr, 0.0);
  tr.rtw = rs.rtw;
  for (int w = 0; w < nwin; ++w)
    for (int32_t n = 0; n < tr.rs_o[(size_t)w + 1] - tr.rs_o[(size_t)w]; ++n) {
      const int64_t k = tr.rs_k[(size_t)tr.rs_o[(size_t)w] + n];
      int terms = 0;
      for (int sl = 0; sl < 2; ++sl) {
        const size_t e = (size_t)sl * nres + k;
        const int64_t kin = rs.in[e];
        if (kin < 0 || wts[(int64_t)w * nchan + kin] == 0.0) continue;          // none, a bin of the zero padding, or outside the window
        const double sc = wts[(int64_t)w * nchan + kin] * rs.w[e] * df;          // weight * (m df) * (1 / m)
        const size_t at = ((size_t)w * 2 + terms++) * nr + n;
        tr.rs_in[at] = (int32_t)kin;
        tr.rs_c[2 * at] = sc * rs.phase[2 * e];
        tr.rs_c[2 * at + 1] = sc * rs.phase[2 * e + 1];
      }
    }

  const int64_t per = nchan * nt;
  const int64_t tables = (int64_t)nwin * nchan * 8 + (int64_t)nwin * 8 + (int64_t)nwin * nr * 44 + nr * 16;
  int64_t nchunks = 0, tc = 0, upload = tables;
  int nstreams = 0, phase_rt = -1;
  double kernel_ms = 0.0;
  if (!phases) {
    // from a cube: closure.hip's loop forms the phases of every chunk and hands them on
    ClosureSink sink;
    sink.bytes_per_triad = tr.bytes_per_row();
    sink.prepare = [&](int64_t c, int64_t last, int ns, const hipStream_t* streams) { return tr.prepare(c, last, ns, streams); };
    sink.kernels = [&](int i, hipStream_t s, int64_t, int64_t tn, const double* d_phase) { return tr.kernels(i, s, tn, d_phase); };
    sink.download = [&](int i, hipStream_t s, int64_t T0, int64_t tn) { return tr.download(i, s, T0, tn); };
    prisim_closure_stats cs = {};
    if (int rc = closure_phase_chunks(ctx, cube, nt, nbl, nchan, legs, conj, nrows, freq_wts, bpwts, masks, nmask, mask_index, phase_route,
                                      budget_bytes, nullptr, out_phase, &cs, &sink))
      return rc;
    nchunks = cs.chunks; tc = cs.chunk_triads; nstreams = cs.streams; phase_rt = cs.route; kernel_ms = cs.kernel_ms;
    upload += (cube ? nbl * per * 16 : 0) + nbl * per * 8 + nchan * 8 + nrows * 24 + (masks ? nmask * nchan * 8 + (mask_index ? nbl * 4 : 0) : 0);
  } else {
    const Chunks ch = plan_chunks(nrows, per * 8 + tr.bytes_per_row(), budget_bytes, kMaxStreams);
    tc = ch.size; nchunks = ch.count; nstreams = ch.nstreams;
    double* d_phase[kMaxStreams] = {};
    for (int i = 0; i < nstreams; ++i) DEV_ALLOC(ctx, tr.wk.dev, d_phase[i], tc * per * 8);
    Streams& st = tr.wk.st;
    if (int rc = st.create(ctx, nstreams, true)) return rc;
    if (int rc = tr.prepare(tc, ch.last, nstreams, st.s)) return rc;
    auto send = [&](int64_t, Span sp, int i, hipStream_t sc) -> int {
      HIPCHK(ctx, hipMemcpyAsync(d_phase[i], phases + (size_t)sp.first * per, (size_t)sp.count * per * 8, hipMemcpyHostToDevice, sc));
      return PRISIM_OK;
    };
    auto kernels = [&](int64_t, Span sp, int i, hipStream_t sc) { return tr.kernels(i, sc, sp.count, d_phase[i]); };
    auto fetch = [&](int64_t, Span sp, int i, hipStream_t sc) { return tr.download(i, sc, sp.first, sp.count); };
    if (int rc = chunk_loop(ctx, st, ch, nrows, send, kernels, fetch)) return rc;
    kernel_ms = st.kernel_ms;
    upload += nrows * per * 8;
  }
  if (stats) {
    stats->wall_ms = wall_ms_since(wall0);
    stats->kernel_ms = kernel_ms;
    stats->rows = nrows;
    stats->chunks = nchunks;
    stats->chunk_rows = tc;
    stats->upload_bytes = upload;
    stats->download_bytes = nrows * (tr.download_per_row() + ((!phases && out_phase) ? per * 8 : 0));
    stats->route = tr.fused ? PRISIM_CPDELAY_FUSED : PRISIM_CPDELAY_ROCFFT;
    stats->phase_route = phase_rt;
    stats->streams = nstreams;
    stats->tile = (int32_t)tr.tile;
    stats->lds_bytes = (int32_t)tr.lds;
    stats->reserved_ = 0;
  }
  return PRISIM_OK;
  });
}

int prisim_closure_power(prisim_ctx* ctx, int64_t n0, int64_t nwin, int64_t inner, const double* spectra, const double* scale,
                         int32_t want, int64_t budget_bytes, double* out_individual, double* out_auto, double* out_cross,
                         prisim_cpdelay_stats* stats) {
  return guarded(ctx, [&]() -> int {
  if (!ctx) return PRISIM_EINVAL;
  const WallTime wall0 = wall_now();
  const bool w_ind = want & PRISIM_CPPOWER_INDIVIDUAL, w_auto = want & PRISIM_CPPOWER_AUTO, w_cross = want & PRISIM_CPPOWER_CROSS;
  if (n0 < 1 || nwin < 1 || inner < 1) return fail(ctx, PRISIM_EINVAL, "need n0, nwin and inner >= 1");
  if (!(w_ind || w_auto || w_cross)) return fail(ctx, PRISIM_EINVAL, "nothing requested (want)");
  if (w_cross && n0 < 2) return fail(ctx, PRISIM_EINVAL, "the cross power needs at least two entries on axis 0");
  if (!spectra || !scale || (w_ind && !out_individual) || (w_auto && !out_auto) || (w_cross && !out_cross))
    return fail(ctx, PRISIM_EINVAL, "null array");
  if (nwin > (int64_t)1 << 30 || inner > ((int64_t)1 << 40) / nwin) return fail(ctx, PRISIM_EINVAL, "nwin * inner is too large");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const int64_t npts = nwin * inner;
  const bool sums = w_auto || w_cross;
  const int64_t per_row = npts * (16 + (w_ind ? 8 : 0));
  const Chunks ch = plan_chunks(n0, per_row, budget_bytes, 1);
  const int64_t rc_rows = ch.size, nchunks = ch.count;
  Work wk;
  Streams& st = wk.st;
  if (int rc = st.create(ctx, 1, true)) return rc;
  hipStream_t s = st.s[0];
  double2 *d_x, *d_sum = nullptr;
  double *d_scale, *d_ind = nullptr, *d_sumsq = nullptr, *d_auto = nullptr, *d_cross = nullptr;
  DEV_ALLOC(ctx, wk.dev, d_x, rc_rows * npts * 16);
  DEV_UPLOAD(ctx, wk.dev, d_scale, scale, (size_t)nwin, s);
  if (w_ind) DEV_ALLOC(ctx, wk.dev, d_ind, rc_rows * npts * 8);
  if (sums) {
    DEV_ALLOC(ctx, wk.dev, d_sumsq, npts * 8);
    DEV_ALLOC(ctx, wk.dev, d_sum, npts * 16);
    DEV_ALLOC(ctx, wk.dev, d_auto, npts * 8);
    if (w_cross) DEV_ALLOC(ctx, wk.dev, d_cross, npts * 8);
  }
  if (sums) {
    HIPCHK(ctx, hipMemsetAsync(d_sumsq, 0, npts * 8, s));
    HIPCHK(ctx, hipMemsetAsync(d_sum, 0, npts * 16, s));
  }
  const int g = grid_for(ctx, npts);
  auto upload = [&](int64_t, Span sp, int, hipStream_t) -> int {
    HIPCHK(ctx, hipMemcpyAsync(d_x, spectra + 2 * (size_t)sp.first * npts, (size_t)sp.count * npts * 16, hipMemcpyHostToDevice, s));
    return PRISIM_OK;
  };
  auto kernels = [&](int64_t c, Span sp, int, hipStream_t) -> int {
    if (int rc = launch(ctx, k_cpp_accumulate, dim3((unsigned)g), 0, s, d_x, sp.count, npts, inner, d_scale, d_ind, d_sumsq, d_sum)) return rc;
    if (!sums || c < nchunks - 1) return PRISIM_OK;
    return launch(ctx, k_cpp_finish, dim3((unsigned)g), 0, s, n0, npts, inner, d_scale, d_sumsq, d_sum, d_auto, d_cross);
  };
  auto download = [&](int64_t, Span sp, int, hipStream_t) -> int {
    if (w_ind) HIPCHK(ctx, hipMemcpyAsync(out_individual + (size_t)sp.first * npts, d_ind, (size_t)sp.count * npts * 8, hipMemcpyDeviceToHost, s));
    return PRISIM_OK;
  };
  if (int rc = chunk_loop(ctx, st, ch, n0, upload, kernels, download)) return rc;   // one stream: its order guards d_x, d_ind and the sums
  if (w_auto) HIPCHK(ctx, hipMemcpyAsync(out_auto, d_auto, npts * 8, hipMemcpyDeviceToHost, s));
  if (w_cross) HIPCHK(ctx, hipMemcpyAsync(out_cross, d_cross, npts * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipStreamSynchronize(s));
  if (stats) {
    stats->wall_ms = wall_ms_since(wall0);
    stats->kernel_ms = st.kernel_ms;
    stats->rows = n0;
    stats->chunks = nchunks;
    stats->chunk_rows = rc_rows;
    stats->upload_bytes = n0 * npts * 16 + nwin * 8;
    stats->download_bytes = npts * ((w_ind ? n0 * 8 : 0) + (w_auto ? 8 : 0) + (w_cross ? 8 : 0));
    stats->route = 0;
    stats->phase_route = -1;
    stats->streams = 1;
    stats->tile = 0;
    stats->lds_bytes = 0;
    stats->reserved_ = 0;
  }
  return PRISIM_OK;
  });
}

}  // extern "C"
