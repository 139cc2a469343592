// subband.hip -- sub-band delay spectra for gfx950 (include/prisim_subband.h): prisim/delay_spectrum.py:subband_delay_transform
// (:2196-2236) for every (snapshot, baseline) row of one or more cubes, every frequency window, and the FFT resampling of the spectra.
//
// The transform, the shift, the resampled bins, their direct sum and the power are csrc_addon/delay_lines.h's.  Particular to this file:
// Fused route (m a power of two, LDS permitting): one workgroup per row.  Per cube the row times its bandpass is read once into LDS;
// then for every window w
//   oversampled: x[n] = row[n] bp[n] wts[w][n] on the window's nonzero channel span [lo, hi), zero elsewhere up to m;
//   resampled: from the row in LDS, without the m lags.  Only the terms inside [lo, hi) count; wave 0 compacts the nonzero Y[k_out] on
//     the device (the kept bins are the lowest and highest ~nres/2 channels, so a window away from channel 0 has none and writes zeros).
// Each output element is written once.
// rocFFT route (any other m): k_sb_prepare writes the windowed padded rows [cube][row][window][m] (and the resampled spectra, as above)
// -> batched inverse rocFFT in place -> k_sb_finish shifts, scales by df and forms the power.
// fp64 throughout, built with -ffp-contract=off (the products round as numpy's).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../csrc_addon/delay_lines.h"
#include "../../include/prisim_subband.h"

namespace {

constexpr int64_t kMaxGridRows = int64_t(1) << 22;     // rows per launch: grid x threads stays far inside 32 bits

struct SbParams {
  const double2* src;       // row r of cube c: src + c * cube_stride + r * nchan
  int64_t cube_stride;
  const double* bp;         // [nbp][nchan]
  int bp_mode;              // 0: one row; 1: r % nbl; 2: row r
  int64_t nbl, nrows;
  const double* wts;        // [nwin][nchan]
  const int32_t* span;      // [nwin][2] nonzero channel span [lo, hi)
  int ncubes, nwin, nchan, m, logm, nres;
  double df;
  const int32_t* rs_in;     // [2][nres] bins of the resampled spectrum (-1: none)
  const double2* rs_c;      // [2][nres] their coefficients, weight df e^{-2 pi i k_in floor(m/2) / m}
  const double2* rtw;       // [nres] e^{+2 pi i q / nres}
  const double* pscale;     // [nwin]
  double2* over;            // [ncubes][nrows][nwin][m]
  double* over_pow;
  double2* res;             // [ncubes][nrows][nwin][nres]
  double* res_pow;
  double2* fbuf;            // rocFFT route: [ncubes][nrows][nwin][m]
  int64_t row0;             // first row of this launch (launches cover at most kMaxGridRows rows)
};

__device__ __forceinline__ const double* bp_row(const SbParams& P, int64_t r) {
  return P.bp + (P.bp_mode == 0 ? 0 : (P.bp_mode == 1 ? r % P.nbl : r)) * (int64_t)P.nchan;
}

// xs[n] = row[n] * bp[n] for one cube
__device__ __forceinline__ void load_row(const SbParams& P, int c, int64_t r, double2* xs) {
  const double2* row = P.src + (int64_t)c * P.cube_stride + r * (int64_t)P.nchan;
  const double* b = bp_row(P, r);
  for (int n = threadIdx.x; n < P.nchan; n += kThreads) xs[n] = rmul(row[n], b[n]);
}

// resampled spectrum of window w (and its power) from xs; z: [nres] double2, zi: [nres] int, cnt: one int of LDS
__device__ void resample_window(const SbParams& P, const double2* xs, int c, int64_t r, int w, int lo, int hi, double2* z, int* zi,
                                int* cnt) {
  const double* wt = P.wts + (int64_t)w * P.nchan;
  const int nres = P.nres;
  for (int k = threadIdx.x; k < nres; k += kThreads) {
    z[k] = resampled_bin([&](int i) { return rmul(xs[i], wt[i]); }, P.rs_in, P.rs_c, nres, k, lo, hi);   // the window's span alone
  }
  __syncthreads();
  if (threadIdx.x < 64) {                       // wave 0 compacts the nonzero bins in increasing order
    const int lane = threadIdx.x;
    int total = 0;
    for (int base = 0; base < nres; base += 64) {
      const int k = base + lane;
      const bool nz = k < nres && (z[k].x != 0.0 || z[k].y != 0.0);
      const uint64_t mask = __ballot(nz);
      if (nz) zi[total + __popcll(mask & ((1ull << lane) - 1ull))] = k;
      total += __popcll(mask);
    }
    if (lane == 0) *cnt = total;
  }
  __syncthreads();
  const int nz = *cnt;
  const int64_t o = (((int64_t)c * P.nrows + r) * P.nwin + w) * nres;
  const double ps = P.pscale ? P.pscale[w] : 0.0;
  for (int q = threadIdx.x; q < nres; q += kThreads) {
    const double2 acc = direct_sum<false>(z, 1, zi, nz, q, nres, P.rtw);
    if (P.res) P.res[o + q] = acc;
    if (P.res_pow) P.res_pow[o + q] = power_of(acc, ps);
  }
  __syncthreads();
}

// fused route.  LDS: xs [nchan] | buf [m] | tw [m/2] | z [nres] | zi [nres] int | cnt
__global__ void __launch_bounds__(kThreads) k_sb_fused(SbParams P) {
  extern __shared__ double2 lds[];
  const int m = P.m, nchan = P.nchan;
  double2* xs = lds;
  double2* buf = xs + nchan;
  double2* tw = buf + m;
  double2* z = tw + (m / 2 > 0 ? m / 2 : 1);
  int* zi = reinterpret_cast<int*>(z + P.nres);
  int* cnt = zi + P.nres;
  const int64_t r = P.row0 + blockIdx.x;
  const bool want_over = P.over || P.over_pow, want_res = P.res || P.res_pow;
  lds_twiddles(tw, m);
  for (int c = 0; c < P.ncubes; ++c) {
    load_row(P, c, r, xs);
    __syncthreads();
    for (int w = 0; w < P.nwin; ++w) {
      const int lo = P.span[2 * w], hi = P.span[2 * w + 1];
      if (want_over) {
        const double* wt = P.wts + (int64_t)w * nchan;
        for (int n = threadIdx.x; n < m; n += kThreads) {
          LdsOperand x = shifted_zero(n, P.logm);
          if (n >= lo && n < hi) x = shifted_operand(rmul(xs[n], wt[n]), n, m, P.logm, P.df);
          buf[x.slot] = x.v;
        }
        __syncthreads();
        lds_ifft_dit(buf, m, 1, m, tw);
        const int64_t o = (((int64_t)c * P.nrows + r) * P.nwin + w) * m;
        const double ps = P.pscale ? P.pscale[w] : 0.0;
        for (int j = threadIdx.x; j < m; j += kThreads) {
          const double2 v = buf[j];
          if (P.over) P.over[o + j] = v;
          if (P.over_pow) P.over_pow[o + j] = power_of(v, ps);
        }
        __syncthreads();
      }
      if (want_res) resample_window(P, xs, c, r, w, lo, hi, z, zi, cnt);
    }
    __syncthreads();
  }
}

// rocFFT route, before the transform.  LDS: xs [nchan] | z [nres] | zi [nres] int | cnt
__global__ void __launch_bounds__(kThreads) k_sb_prepare(SbParams P) {
  extern __shared__ double2 lds[];
  double2* xs = lds;
  double2* z = xs + P.nchan;
  int* zi = reinterpret_cast<int*>(z + P.nres);
  int* cnt = zi + P.nres;
  const int64_t r = P.row0 + blockIdx.x;
  const bool want_over = P.over || P.over_pow, want_res = P.res || P.res_pow;
  for (int c = 0; c < P.ncubes; ++c) {
    load_row(P, c, r, xs);
    __syncthreads();
    for (int w = 0; w < P.nwin; ++w) {
      const int lo = P.span[2 * w], hi = P.span[2 * w + 1];
      if (want_over) {
        const double* wt = P.wts + (int64_t)w * P.nchan;
        double2* dst = P.fbuf + (((int64_t)c * P.nrows + r) * P.nwin + w) * P.m;
        for (int n = threadIdx.x; n < P.m; n += kThreads)
          dst[n] = (n >= lo && n < hi) ? rmul(xs[n], wt[n]) : make_double2(0.0, 0.0);
      }
      if (want_res) resample_window(P, xs, c, r, w, lo, hi, z, zi, cnt);
    }
    __syncthreads();
  }
}

// rocFFT route, after the unnormalised inverse transform: lag j gathers its transform bin
__global__ void __launch_bounds__(kThreads) k_sb_finish(SbParams P, int64_t nlines) {
  const int m = P.m;
  const int64_t total = nlines * m;
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kThreads) {
    const int64_t line = e / m;
    const int j = (int)(e - line * m);
    const double2 v = rmul(P.fbuf[line * m + shift_source(j, m)], P.df);
    if (P.over) P.over[e] = v;
    if (P.over_pow) P.over_pow[e] = power_of(v, P.pscale[line % P.nwin]);
  }
}

// ---- host side --------------------------------------------------------------------------------------------------------------

int lds_fused(int64_t nchan, int64_t m, int64_t nres) {
  return (int)(16 * (nchan + m + std::max<int64_t>(m / 2, 1) + nres) + 4 * nres + 16);
}
int lds_prepare(int64_t nchan, int64_t nres) { return (int)(16 * (nchan + nres) + 4 * nres + 16); }

}  // namespace

extern "C" {

int prisim_subband_transform(prisim_ctx* ctx, int32_t ncubes, int64_t nt, int64_t nbl, int64_t nchan, const double* cubes, int64_t t0,
                             const double* bp, int64_t nbp, int32_t nwin, const double* wts, int64_t m, double df, int64_t nres,
                             int64_t nmap, const int64_t* map_out, const int64_t* map_in, const double* map_w, const double* pscale,
                             int32_t want, int32_t route, double* over, double* over_pow, double* res, double* res_pow,
                             prisim_subband_stats* stats) {
  return guarded(ctx, [&]() -> int {
  if (!ctx) return PRISIM_EINVAL;
  if (m < 1 || m > PRISIM_SUBBAND_MAX_LEN)
    return fail(ctx, PRISIM_EINVAL, "sub-band spectra take 1 to " + std::to_string(PRISIM_SUBBAND_MAX_LEN) +
                                        " lags (PRISIM_SUBBAND_MAX_LEN); got m = " + std::to_string(m));
  const bool w_over = want & PRISIM_SUBBAND_OVER, w_opow = want & PRISIM_SUBBAND_OVER_POWER;
  const bool w_res = want & PRISIM_SUBBAND_RES, w_rpow = want & PRISIM_SUBBAND_RES_POWER;
  if ((w_res || w_rpow) && (nres < 1 || nres > PRISIM_SUBBAND_MAX_LEN))
    return fail(ctx, PRISIM_EINVAL, "resampled sub-band spectra take 1 to " + std::to_string(PRISIM_SUBBAND_MAX_LEN) +
                                        " lags (PRISIM_SUBBAND_MAX_LEN); got nres = " + std::to_string(nres));
  if (!(w_res || w_rpow)) nres = 0;
  if (ncubes < 1 || nt < 0 || nbl < 1 || nchan < 1 || nchan > m || nwin < 1)
    return fail(ctx, PRISIM_EINVAL, "need ncubes >= 1, nt >= 0, nbl >= 1, nwin >= 1 and 1 <= nchan <= m");
  if (!(w_over || w_opow || w_res || w_rpow)) return fail(ctx, PRISIM_EINVAL, "nothing requested (want)");
  if (!bp || !wts || (w_over && !over) || (w_opow && !over_pow) || (w_res && !res) || (w_rpow && !res_pow) ||
      ((w_opow || w_rpow) && !pscale))
    return fail(ctx, PRISIM_EINVAL, "null array");
  const int64_t nrows = nt * nbl;
  int bp_mode;
  if (nbp == 1) bp_mode = 0;
  else if (nbp == nbl) bp_mode = 1;
  else if (nbp == nrows) bp_mode = 2;
  else return fail(ctx, PRISIM_EINVAL, "nbp must be 1, nbl or nt * nbl");
  if (!cubes) {
    if (!ctx->array_set) return fail(ctx, PRISIM_ESTATE, "resident input needs set_array first");
    if (ncubes != 1 || nbl != ctx->nbl || nchan != ctx->nchan) return fail(ctx, PRISIM_EINVAL, "resident input is one cube of the array's shape");
    if (t0 < 0 || t0 + nt > ctx->nt_max) return fail(ctx, PRISIM_EINVAL, "resident slots out of range");
  }
  if (route < PRISIM_SUBBAND_AUTO || route > PRISIM_SUBBAND_ROCFFT) return fail(ctx, PRISIM_EINVAL, "unknown route");
  bool pow2;
  const int logm = ceil_log2(m, pow2);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int lds_max = 0;
  if (int rc = lds_limit(ctx, lds_max)) return rc;
  const int lf = lds_fused(nchan, m, nres), lp = lds_prepare(nchan, nres);
  const bool fused_ok = pow2 && lf <= lds_max;
  if (route == PRISIM_SUBBAND_FUSED && !fused_ok)
    return fail(ctx, PRISIM_EINVAL, "the fused sub-band kernel takes power-of-two m whose rows fit in LDS (" + std::to_string(lf) +
                                        " B needed, " + std::to_string(lds_max) + " B per workgroup)");
  const bool fused = route == PRISIM_SUBBAND_FUSED || (route == PRISIM_SUBBAND_AUTO && fused_ok);
  if (!fused && lp > lds_max) return fail(ctx, PRISIM_EINVAL, "sub-band rows do not fit in LDS");
  const bool want_over = w_over || w_opow;
  if (!fused && want_over) {
    if (int rc = ensure_rocfft(ctx)) return rc;
  }

  // window spans and the resampling tables
  std::vector<int32_t> span(2 * (size_t)nwin);
  for (int w = 0; w < nwin; ++w) {
    int64_t lo = nchan, hi = 0;
    for (int64_t n = 0; n < nchan; ++n)
      if (wts[w * nchan + n] != 0.0) { lo = std::min(lo, n); hi = n + 1; }
    span[2 * w] = (int32_t)(lo < hi ? lo : 0);
    span[2 * w + 1] = (int32_t)(lo < hi ? hi : 0);
  }
  ResampleTables rt;
  std::vector<double> rs_c;
  // weight * (m df) * (1 / m): the ifft's 1 / nres times resample's nres / m
  if (int rc = build_resample_tables(ctx, nres, m, nchan, df, nmap, map_out, map_in, map_w, rt, &rs_c)) return rc;

  Work wk;
  Events ev;
  if (int rc = ev.create(ctx)) return rc;
  const size_t in_bytes = (size_t)ncubes * nrows * nchan * 16;
  const size_t bp_bytes = (size_t)nbp * nchan * 8, w_bytes = (size_t)nwin * nchan * 8;
  const int64_t nlines = (int64_t)ncubes * nrows * nwin;
  const size_t over_n = (size_t)nlines * m, res_n = (size_t)nlines * std::max<int64_t>(nres, 0);
  double2* d_in = nullptr;
  double *d_bp, *d_wts, *d_ps;
  int32_t *d_span, *d_rsin;
  double2 *d_rsc, *d_rtw, *d_over = nullptr, *d_res = nullptr, *d_fbuf = nullptr;
  double *d_opow = nullptr, *d_rpow = nullptr;
  if (cubes) DEV_ALLOC(ctx, wk.dev, d_in, in_bytes);
  DEV_ALLOC(ctx, wk.dev, d_bp, bp_bytes);
  DEV_ALLOC(ctx, wk.dev, d_wts, w_bytes);
  DEV_ALLOC(ctx, wk.dev, d_ps, (size_t)nwin * 8);
  DEV_ALLOC(ctx, wk.dev, d_span, span.size() * 4);
  DEV_ALLOC(ctx, wk.dev, d_rsin, rt.in.size() * 4);
  DEV_ALLOC(ctx, wk.dev, d_rsc, rs_c.size() * 8);
  DEV_ALLOC(ctx, wk.dev, d_rtw, rt.rtw.size() * 8);
  if (w_over) DEV_ALLOC(ctx, wk.dev, d_over, over_n * 16);
  if (w_opow) DEV_ALLOC(ctx, wk.dev, d_opow, over_n * 8);
  if (w_res) DEV_ALLOC(ctx, wk.dev, d_res, res_n * 16);
  if (w_rpow) DEV_ALLOC(ctx, wk.dev, d_rpow, res_n * 8);
  if (!fused && want_over) DEV_ALLOC(ctx, wk.dev, d_fbuf, over_n * 16);
  if (!fused && want_over && nlines > 0)
    if (int rc = wk.fft.create(ctx, wk.dev, (size_t)m, {{true, (size_t)nlines}}, &ctx->stream, 1)) return rc;

  HIPCHK(ctx, hipEventRecord(ev.e[0], ctx->stream));
  if (cubes && in_bytes) HIPCHK(ctx, hipMemcpyAsync(d_in, cubes, in_bytes, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(d_bp, bp, bp_bytes, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(d_wts, wts, w_bytes, hipMemcpyHostToDevice, ctx->stream));
  if (pscale) HIPCHK(ctx, hipMemcpyAsync(d_ps, pscale, (size_t)nwin * 8, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(d_span, span.data(), span.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(d_rsin, rt.in.data(), rt.in.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(d_rsc, rs_c.data(), rs_c.size() * 8, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(d_rtw, rt.rtw.data(), rt.rtw.size() * 8, hipMemcpyHostToDevice, ctx->stream));

  SbParams P;
  P.src = cubes ? d_in : (const double2*)ctx->cube.p + t0 * nbl * nchan;
  P.cube_stride = nrows * nchan;
  P.bp = d_bp; P.bp_mode = bp_mode; P.nbl = nbl; P.nrows = nrows;
  P.wts = d_wts; P.span = d_span;
  P.ncubes = ncubes; P.nwin = nwin; P.nchan = (int)nchan; P.m = (int)m; P.logm = logm; P.nres = (int)nres;
  P.df = df;
  P.rs_in = d_rsin; P.rs_c = d_rsc; P.rtw = d_rtw;
  P.pscale = pscale ? d_ps : nullptr;
  P.over = d_over; P.over_pow = d_opow; P.res = d_res; P.res_pow = d_rpow; P.fbuf = d_fbuf; P.row0 = 0;
  const int lds = fused ? lf : lp;
  HIPCHK(ctx, hipEventRecord(ev.e[1], ctx->stream));
  if (nrows > 0) {
    if (fused) {
      if (int rc = allow_lds(ctx, k_sb_fused, lds)) return rc;
      for (int64_t r0 = 0; r0 < nrows; r0 += kMaxGridRows) {
        P.row0 = r0;
        if (int rc = launch(ctx, k_sb_fused, dim3((unsigned)std::min(kMaxGridRows, nrows - r0)), (size_t)lds, ctx->stream, P)) return rc;
      }
    } else {
      if (int rc = allow_lds(ctx, k_sb_prepare, lds)) return rc;
      for (int64_t r0 = 0; r0 < nrows; r0 += kMaxGridRows) {
        P.row0 = r0;
        if (int rc = launch(ctx, k_sb_prepare, dim3((unsigned)std::min(kMaxGridRows, nrows - r0)), (size_t)lds, ctx->stream, P)) return rc;
      }
      if (want_over) {
        if (int rc = wk.fft.run(ctx, true, (size_t)nlines, d_fbuf, 0)) return rc;
        const int64_t blocks = std::min<int64_t>((int64_t)over_n / kThreads + 1, (int64_t)std::max(ctx->cu_count, 1) * 16);
        if (int rc = launch(ctx, k_sb_finish, dim3((unsigned)blocks), 0, ctx->stream, P, nlines)) return rc;
      }
    }
  }
  HIPCHK(ctx, hipEventRecord(ev.e[2], ctx->stream));
  if (nlines > 0) {
    if (w_over) HIPCHK(ctx, hipMemcpyAsync(over, d_over, over_n * 16, hipMemcpyDeviceToHost, ctx->stream));
    if (w_opow) HIPCHK(ctx, hipMemcpyAsync(over_pow, d_opow, over_n * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (w_res) HIPCHK(ctx, hipMemcpyAsync(res, d_res, res_n * 16, hipMemcpyDeviceToHost, ctx->stream));
    if (w_rpow) HIPCHK(ctx, hipMemcpyAsync(res_pow, d_rpow, res_n * 8, hipMemcpyDeviceToHost, ctx->stream));
  }
  HIPCHK(ctx, hipEventRecord(ev.e[3], ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  if (stats) {
    float ms = 0.0f, kms = 0.0f;
    HIPCHK(ctx, hipEventElapsedTime(&ms, ev.e[0], ev.e[3]));
    HIPCHK(ctx, hipEventElapsedTime(&kms, ev.e[1], ev.e[2]));
    stats->device_ms = ms;
    stats->kernel_ms = kms;
    stats->rows = (int64_t)ncubes * nrows;
    stats->route = fused ? PRISIM_SUBBAND_FUSED : PRISIM_SUBBAND_ROCFFT;
    stats->lds_bytes = lds;
  }
  return PRISIM_OK;
  });
}

}  // extern "C"
