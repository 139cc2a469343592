// cpft.hip -- delay spectra of binned closure phasors for gfx950 (include/prisim_cpft.h): the transforms of
// prisim/bispectrum_phase.py:ClosurePhaseDelaySpectrum.FT (:2719-2757) and their FFT resampling (:2770-2779).
//
// A row is one (LST bin, day bin or day-bin combination, triad).  Inputs, weights and outputs are all channel- or lag-fastest, so a
// wavefront reads and writes consecutive pieces of a row and nothing is transposed.
//   k_cpft_rows<true> (fused, m a power of two): one workgroup per group of R consecutive rows (R = 1 from m = 2048 on, more for
//     small m).  It reads the group's weights once into LDS, reduces their means there and turns them into fw = w / mean (0 for a row
//     of mean 0).  Then, for every input and the lag kernel (a "pass") and every window, it transforms x = in fw wts vscale in LDS
//     rows of m double2 (csrc_addon/delay_lines.h, as the shift, the resampled bins and their direct sum) and writes the rows out.
//     LDS: 16 R m (rows) + 8 m (twiddles) + 8 R nchan + 2 KiB (weights and their reduction) + 68 R; at m = 4096 and nchan = 2048 that
//     is 64 + 32 + 16 + 2 KiB of the 160 KiB of a CU, one workgroup per CU; from m = 1024 down, two or more.
//   rocFFT route (any other m): k_cpft_rows<false>, the same kernel without the transform, writes the padded rows x -> batched
//     inverse rocFFT in place -> k_cpft_finish shifts and scales by df.
//   k_cpft_resample (both routes): one workgroup per group of rows forms, per pass and window, the Y of the bins that the window
//     feeds (Feeds::kNonzero) in LDS and sums them.
// An input with a leading extent of 1 is uploaded once and read with stride 0; the others are streamed with the rows.  Chunks of
// rows alternate between two streams with their own buffers, so that the upload of one chunk, the kernels of the other and the
// downloads overlap.  No atomics, no scratch.  fp64 throughout, built with -ffp-contract=off.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../csrc_addon/delay_lines.h"
#include "../../include/prisim_cpft.h"

using namespace pint;

namespace {

constexpr int kMaxIn = PRISIM_CPFT_MAX_IN;
constexpr int kMaxPass = kMaxIn + 1;                  // the inputs and the lag kernel
constexpr int kMaxGroup = 64;                         // rows per workgroup at most
constexpr int kGroupElems = 2048;                     // lags a workgroup of the fused kernel holds in LDS when m is small

struct FtIn {
  const double2* p;         // chunked: this chunk's [rn][nchan]; else the whole stack [b0][b1][b2][nchan]
  int64_t s0, s1, s2;       // rows between neighbours on the three leading axes (0: an extent of 1)
  int32_t chunked, pad_;
};

struct FtParams {
  FtIn in[kMaxIn];
  const double* w;          // this chunk's [rn][nchan], or null
  const double* wts;        // [nwin][nchan]
  const double* vscale;     // [nwin][n0], or null
  int64_t row0, rn;         // the chunk's first row and its rows
  int64_t n0, n1, n2;
  int nin, lagk;            // passes: the inputs, then (lagk) the lag kernel
  int nwin, nchan, m, logm, nres;
  int R, G;                 // rows per workgroup; threads per row in the reduction of the weights (R * G <= kThreads)
  double df;
  double2* over[kMaxPass];  // per pass this chunk's [nwin][rn][m], or null
  double2* res[kMaxPass];   // per pass this chunk's [nwin][rn][nres], or null
  double2* fbuf;            // rocFFT route: [pass - fpass0][nwin][rn][m]
  int fpass0;
  const int32_t* rs_o;      // [nwin + 1] bins of the resampled spectrum that window k feeds: rs_k[rs_o[k] .. rs_o[k + 1]), increasing
  const int32_t* rs_k;
  const int32_t* rs_in;     // [2][nres] channels of a bin (-1: none)
  const double2* rs_c;      // [2][nres] weight df e^{-2 pi i k_in floor(m/2) / m}
  const double2* rtw;       // [nres] e^{+2 pi i q / nres}
};

// what a workgroup knows of its rows: LDS behind the kernel's own arrays, roff [R][kMaxIn] int64 | fw [R][nchan] | red [kThreads] | i0 [R]
struct Group {
  int64_t l0;               // first row, within the chunk
  int rc;                   // rows (<= R)
  int64_t* roff;
  double* fw;               // null without weights
  int* i0;
};

__host__ __device__ inline size_t group_lds(int R, int nchan, bool has_w) {
  return (size_t)R * kMaxIn * 8 + (has_w ? (size_t)R * nchan * 8 + kThreads * 8 : 0) + (size_t)R * 4;
}

// by the whole workgroup; ends with a barrier
__device__ __forceinline__ void group_begin(const FtParams& P, char* base, Group& g) {
  const int R = P.R, nchan = P.nchan, tid = threadIdx.x;
  g.l0 = (int64_t)blockIdx.x * R;
  g.rc = (int)min((int64_t)R, P.rn - g.l0);
  g.roff = reinterpret_cast<int64_t*>(base);
  double* fw = reinterpret_cast<double*>(g.roff + (size_t)R * kMaxIn);
  double* red = fw + (P.w ? (size_t)R * nchan : 0);
  g.fw = P.w ? fw : nullptr;
  g.i0 = reinterpret_cast<int*>(red + (P.w ? kThreads : 0));
  for (int e = tid; e < g.rc * kMaxIn; e += kThreads) {
    const int rr = e / kMaxIn, i = e - rr * kMaxIn;
    const int64_t lrow = g.l0 + rr, row = P.row0 + lrow;
    const int64_t a = row / (P.n1 * P.n2), rem = row - a * (P.n1 * P.n2), b = rem / P.n2, c = rem - b * P.n2;
    if (i == 0) g.i0[rr] = (int)a;
    int64_t off = 0;
    if (i < P.nin) off = P.in[i].chunked ? lrow : a * P.in[i].s0 + b * P.in[i].s1 + c * P.in[i].s2;
    g.roff[e] = off * nchan;
  }
  if (P.w) {
    const double* src = P.w + g.l0 * nchan;
    const int n = g.rc * nchan;
    for (int e = tid; e < n; e += kThreads) fw[e] = src[e];
    __syncthreads();
    const int G = P.G, rr = tid / G, l = tid - rr * G;
    double s = 0.0;
    if (rr < g.rc)
      for (int ch = l; ch < nchan; ch += G) s += fw[rr * nchan + ch];
    red[tid] = s;
    __syncthreads();
    for (int h = G >> 1; h >= 1; h >>= 1) {
      if (l < h) red[tid] += red[tid + h];
      __syncthreads();
    }
    for (int e = tid; e < n; e += kThreads) {
      const double mu = red[(e / nchan) * G] / (double)nchan;
      fw[e] = mu == 0.0 ? 0.0 : fw[e] / mu;
    }
  }
  __syncthreads();
}

// x[n] of row rr of the group, pass p, window k (n < nchan)
__device__ __forceinline__ double2 x_value(const FtParams& P, const Group& g, int p, int k, int rr, int n) {
  double s = P.wts[k * P.nchan + n];
  if (g.fw) s = g.fw[rr * P.nchan + n] * s;
  if (p >= P.nin) return make_double2(s, 0.0);
  if (P.vscale) s = s * P.vscale[(int64_t)k * P.n0 + g.i0[rr]];
  if (s == 0.0) return make_double2(0.0, 0.0);
  return rmul(P.in[p].p[g.roff[rr * kMaxIn + p] + n], s);
}

// grid: x = group of R rows of the chunk.  LDS: FUSED: buf [R][m] | tw [max(m / 2, 1)] |; then the group's (group_lds)
template <bool FUSED>
__global__ void __launch_bounds__(kThreads) k_cpft_rows(const FtParams P) {
  extern __shared__ double2 lds[];
  const int R = P.R, m = P.m, nchan = P.nchan;
  double2* buf = lds;
  double2* tw = buf + (FUSED ? (size_t)R * m : 0);
  Group g;
  if (FUSED) lds_twiddles(tw, m);
  group_begin(P, reinterpret_cast<char*>(tw + (FUSED ? max(m / 2, 1) : 0)), g);
  const int npass = P.nin + P.lagk;
  for (int p = 0; p < npass; ++p) {
    if (!P.over[p]) continue;
    double2* out = FUSED ? P.over[p] : P.fbuf + (int64_t)(p - P.fpass0) * P.nwin * P.rn * m;
    for (int k = 0; k < P.nwin; ++k) {
      double2* orow = out + ((int64_t)k * P.rn + g.l0) * m;
      for (int e = threadIdx.x; e < g.rc * m; e += kThreads) {
        const int rr = FUSED ? e >> P.logm : e / m, n = e - rr * m;
        double2 v = make_double2(0.0, 0.0);
        if (n < nchan) v = x_value(P, g, p, k, rr, n);
        if (!FUSED) { orow[e] = v; continue; }
        const LdsOperand x = shifted_operand(v, n, m, P.logm, P.df);    // the padding too: its odd samples are 0 * -df
        buf[rr * m + x.slot] = x.v;
      }
      if (FUSED) {
        __syncthreads();
        lds_ifft_dit(buf, m, g.rc, m, tw);
        for (int e = threadIdx.x; e < g.rc * m; e += kThreads) orow[e] = buf[e];
        __syncthreads();
      }
    }
  }
}

// rocFFT route, after the unnormalised inverse transform: transform bin jf scatters to its lag.  Grid-stride over the lines.
__global__ void __launch_bounds__(kThreads) k_cpft_finish(const FtParams P) {
  const int m = P.m, npass = P.nin + P.lagk;
  const int64_t per = (int64_t)P.nwin * P.rn * m;
  for (int p = 0; p < npass; ++p) {
    if (!P.over[p]) continue;
    const double2* src = P.fbuf + (int64_t)(p - P.fpass0) * per;
    double2* dst = P.over[p];
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < per; e += (int64_t)gridDim.x * kThreads) {
      const int64_t line = e / m;
      const int jf = (int)(e - line * m);
      dst[line * m + shift_target(jf, m)] = rmul(src[e], P.df);
    }
  }
}

// resampled spectra.  grid: x = group of R rows of the chunk.  LDS: Y [R][nres] |; then the group's (group_lds)
__global__ void __launch_bounds__(kThreads) k_cpft_resample(const FtParams P) {
  extern __shared__ double2 lds[];
  const int R = P.R, nres = P.nres;
  double2* Y = lds;
  Group g;
  group_begin(P, reinterpret_cast<char*>(Y + (size_t)R * nres), g);
  const int npass = P.nin + P.lagk;
  for (int p = 0; p < npass; ++p) {
    if (!P.res[p]) continue;
    for (int k = 0; k < P.nwin; ++k) {
      const int nz = P.rs_o[k + 1] - P.rs_o[k];
      const int32_t* kout = P.rs_k + P.rs_o[k];
      for (int e = threadIdx.x; e < g.rc * nz; e += kThreads) {
        const int rr = e / nz, i = e - rr * nz, kk = kout[i];
        Y[rr * nres + i] = resampled_bin([&](int ch) { return x_value(P, g, p, k, rr, ch); }, P.rs_in, P.rs_c, nres, kk);
      }
      __syncthreads();
      double2* orow = P.res[p] + ((int64_t)k * P.rn + g.l0) * nres;
      for (int e = threadIdx.x; e < g.rc * nres; e += kThreads) {
        const int rr = e / nres, q = e - rr * nres;
        orow[e] = direct_sum<true>(Y + rr * nres, 1, kout, nz, q, nres, P.rtw);
      }
      __syncthreads();
    }
  }
}

int pow2_at_least(int64_t n) {
  int p = 1;
  while (p < n) p <<= 1;
  return p;
}

}  // namespace

extern "C" {

int prisim_cphase_ft(prisim_ctx* ctx, int64_t n0, int64_t n1, int64_t n2, int64_t nchan, int32_t nin, const double* const* inputs,
                     const int64_t* in_shape, const double* w, int32_t nwin, const double* wts, const double* vscale, int64_t m, double df,
                     int64_t nres, int64_t nmap, const int64_t* map_out, const int64_t* map_in, const double* map_w, int32_t want,
                     int32_t route, int64_t budget_bytes, double* const* over, double* const* res, double* lag_kernel,
                     double* lag_kernel_res, prisim_cpft_stats* stats) {
  return guarded(ctx, [&]() -> int {
  if (!ctx) return PRISIM_EINVAL;
  const WallTime wall0 = wall_now();
  const bool w_over = want & PRISIM_CPFT_OVER, w_res = want & PRISIM_CPFT_RES, w_lag = want & PRISIM_CPFT_LAG;
  if (want < 1 || want > 7 || !(w_over || w_res || w_lag)) return fail(ctx, PRISIM_EINVAL, "nothing requested, or unknown bits (want)");
  if (n0 < 1 || n1 < 1 || n2 < 1 || nchan < 1 || nwin < 1) return fail(ctx, PRISIM_EINVAL, "need n0, n1, n2, nchan and nwin >= 1");
  if (m < nchan || m > PRISIM_CPFT_MAX_LEN)
    return fail(ctx, PRISIM_EINVAL, "closure-phasor delay spectra take nchan to " + std::to_string(PRISIM_CPFT_MAX_LEN) +
                                        " lags (PRISIM_CPFT_MAX_LEN); got m = " + std::to_string(m));
  if (w_res && (nres < 1 || nres > PRISIM_CPFT_MAX_LEN))
    return fail(ctx, PRISIM_EINVAL, "resampled closure-phasor delay spectra take 1 to " + std::to_string(PRISIM_CPFT_MAX_LEN) +
                                        " lags (PRISIM_CPFT_MAX_LEN); got nres = " + std::to_string(nres));
  if (!w_res) nres = 0;
  if (n0 > (int64_t)1 << 24 || n1 > (int64_t)1 << 24 || n2 > (int64_t)1 << 24 || nwin > 1 << 16 ||
      n0 * n1 > ((int64_t)1 << 30) / n2)
    return fail(ctx, PRISIM_EINVAL, "the stack is too large (2^30 rows and 2^16 windows at most)");
  if (nin < 0 || nin > kMaxIn) return fail(ctx, PRISIM_EINVAL, "need 0 <= nin <= " + std::to_string(kMaxIn) + " input stacks");
  if (nin > 0 && (!inputs || !in_shape)) return fail(ctx, PRISIM_EINVAL, "null inputs");
  const int64_t full[3] = {n0, n1, n2};
  for (int i = 0; i < nin; ++i) {
    if (!inputs[i]) return fail(ctx, PRISIM_EINVAL, "input " + std::to_string(i) + " is NULL");
    for (int a = 0; a < 3; ++a)
      if (in_shape[3 * i + a] != full[a] && in_shape[3 * i + a] != 1)
        return fail(ctx, PRISIM_EINVAL, "input " + std::to_string(i) + ": axis " + std::to_string(a) + " has " +
                                            std::to_string(in_shape[3 * i + a]) + " entries, neither the full extent nor 1");
  }
  if (!wts) return fail(ctx, PRISIM_EINVAL, "null wts");
  if (!(w_over || w_res)) nin = 0;                  // only the lag kernel is wanted: no input is read
  const bool in_over = w_over && nin > 0, in_res = w_res && nin > 0, lag_res = w_lag && w_res;
  if ((in_over && !over) || (in_res && !res)) return fail(ctx, PRISIM_EINVAL, "an output is NULL");
  for (int i = 0; i < nin; ++i)
    if ((in_over && !over[i]) || (in_res && !res[i])) return fail(ctx, PRISIM_EINVAL, "an output is NULL");
  if ((w_lag && !lag_kernel) || (lag_res && !lag_kernel_res)) return fail(ctx, PRISIM_EINVAL, "an output is NULL");
  if (!(in_over || in_res || w_lag)) return fail(ctx, PRISIM_EINVAL, "nothing requested: no input and no lag kernel");
  if (route < PRISIM_CPFT_AUTO || route > PRISIM_CPFT_ROCFFT) return fail(ctx, PRISIM_EINVAL, "unknown route");
  bool pow2;
  const int logm = ceil_log2(m, pow2);
  if (route == PRISIM_CPFT_FUSED && !pow2)
    return fail(ctx, PRISIM_EINVAL, "the fused route takes a power-of-two m; got m = " + std::to_string(m));
  ResampleTables rs;
  std::vector<double> rs_c;
  if (int rc = build_resample_tables(ctx, nres, m, nchan, df, nmap, map_out, map_in, map_w, rs, &rs_c)) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int lds_max = 0;
  if (int rc = lds_limit(ctx, lds_max)) return rc;

  const bool has_w = w != nullptr;
  const size_t fused_row = (size_t)m * 16 + (size_t)std::max<int64_t>(m / 2, 1) * 16 + group_lds(1, (int)nchan, has_w);
  const bool fused_ok = pow2 && fused_row <= (size_t)lds_max;
  if (route == PRISIM_CPFT_FUSED && !fused_ok)
    return fail(ctx, PRISIM_EINVAL, "a row of the fused route does not fit in LDS (" + std::to_string(fused_row) + " B needed)");
  const bool fused = route != PRISIM_CPFT_ROCFFT && fused_ok;
  const bool any_over = in_over || w_lag, any_res = in_res || lag_res;
  const int64_t rows = n0 * n1 * n2;
  // rows per workgroup and LDS of the two kernels, from the shapes alone (so that every chunking reduces a row's weights alike)
  auto rows_lds = [&](int R) { return (fused ? (size_t)R * m * 16 + (size_t)std::max<int64_t>(m / 2, 1) * 16 : 0) + group_lds(R, (int)nchan, has_w); };
  int R = (int)std::max<int64_t>(1, std::min<int64_t>(kMaxGroup, kGroupElems / m));
  while (R > 1 && rows_lds(R) > (size_t)lds_max) R >>= 1;
  if (any_over && rows_lds(R) > (size_t)lds_max)
    return fail(ctx, PRISIM_EINVAL, "a row does not fit in LDS (" + std::to_string(rows_lds(R)) + " B needed)");
  const int64_t nr = std::max<int64_t>(nres, 1);
  auto res_lds = [&](int Rr) { return (size_t)Rr * nr * 16 + group_lds(Rr, (int)nchan, has_w); };
  int Rr = (int)std::max<int64_t>(1, std::min<int64_t>(kMaxGroup, 512 / nr));
  while (Rr > 1 && res_lds(Rr) > (size_t)lds_max) Rr >>= 1;
  if (any_res && res_lds(Rr) > (size_t)lds_max) return fail(ctx, PRISIM_EINVAL, "a resampled row does not fit in LDS");
  if (!fused && any_over) {
    if (int rc = ensure_rocfft(ctx)) return rc;
  }

  // the bins of the resampled spectrum that a window feeds
  std::vector<int32_t> rs_o, rs_k;
  fed_bins(rs, nres, nwin, nchan, wts, Feeds::kNonzero, rs_o, rs_k);

  // passes: the inputs, then the lag kernel.  With weights the lag kernel is one more output per row; without, one row of its own.
  const int lag_rows = (w_lag && has_w) ? 1 : 0;
  const int npass_over = (in_over ? nin : 0) + lag_rows, npass_res = (in_res ? nin : 0) + (lag_res && has_w ? 1 : 0);
  int nstreamed = 0;
  int64_t bcast_bytes = 0;
  bool chunked[kMaxIn] = {};
  int64_t in_rows[kMaxIn] = {};
  for (int i = 0; i < nin; ++i) {
    in_rows[i] = in_shape[3 * i] * in_shape[3 * i + 1] * in_shape[3 * i + 2];
    chunked[i] = in_rows[i] == rows;
    if (chunked[i]) ++nstreamed;
    else bcast_bytes += in_rows[i] * nchan * 16;
  }
  const int64_t row_bytes = nstreamed * nchan * 16 + (has_w ? nchan * 8 : 0) +
                            (int64_t)nwin * (npass_over * m * 16 * (fused ? 1 : 2) + npass_res * nres * 16);
  const Chunks ch = plan_chunks(rows, row_bytes, budget_bytes, kMaxStreams);
  const int64_t tc = ch.size, nchunks = ch.count;
  const int nstreams = ch.nstreams;

  // the tables go up on stream 0 as they are allocated
  Work wk;
  Streams& st = wk.st;
  if (int rc = st.create(ctx, nstreams, true)) return rc;
  hipStream_t s0 = st.s[0];
  double *d_wts, *d_vs = nullptr;
  ResampleDev rd;
  DEV_UPLOAD(ctx, wk.dev, d_wts, wts, (size_t)nwin * nchan, s0);
  if (vscale) DEV_UPLOAD(ctx, wk.dev, d_vs, vscale, (size_t)nwin * n0, s0);
  if (int rc = upload_resample(ctx, wk.dev, rd, rs.in, rs_c, rs.rtw, rs_o, rs_k, s0)) return rc;
  double2* d_bcast[kMaxIn] = {};
  for (int i = 0; i < nin; ++i)
    if (!chunked[i]) DEV_UPLOAD(ctx, wk.dev, d_bcast[i], inputs[i], (size_t)in_rows[i] * nchan * 2, s0);
  double2 *d_in[kMaxStreams][kMaxIn] = {}, *d_over[kMaxStreams][kMaxPass] = {}, *d_res[kMaxStreams][kMaxPass] = {}, *d_fbuf[kMaxStreams] = {};
  double* d_w[kMaxStreams] = {};
  const int fpass0 = in_over ? 0 : nin;
  for (int s = 0; s < nstreams; ++s) {
    for (int i = 0; i < nin; ++i)
      if (chunked[i]) DEV_ALLOC(ctx, wk.dev, d_in[s][i], (size_t)tc * nchan * 16);
    if (has_w) DEV_ALLOC(ctx, wk.dev, d_w[s], (size_t)tc * nchan * 8);
    for (int p = 0; p < nin + lag_rows; ++p) {
      const bool is_lag = p >= nin;
      if (is_lag || in_over) DEV_ALLOC(ctx, wk.dev, d_over[s][p], (size_t)nwin * tc * m * 16);
      if (is_lag ? lag_res : in_res) DEV_ALLOC(ctx, wk.dev, d_res[s][p], (size_t)nwin * tc * nres * 16);
    }
    if (!fused && npass_over) DEV_ALLOC(ctx, wk.dev, d_fbuf[s], (size_t)npass_over * nwin * tc * m * 16);
  }
  // without weights: the one row of the lag kernel per window
  double2 *d_lagk = nullptr, *d_lagk_res = nullptr, *d_lagk_f = nullptr;
  const bool lone_lag = w_lag && !has_w;
  if (lone_lag) {
    DEV_ALLOC(ctx, wk.dev, d_lagk, (size_t)nwin * m * 16);
    if (lag_res) DEV_ALLOC(ctx, wk.dev, d_lagk_res, (size_t)nwin * nres * 16);
    if (!fused) DEV_ALLOC(ctx, wk.dev, d_lagk_f, (size_t)nwin * m * 16);
  }
  if (!fused && any_over) {
    std::vector<std::pair<bool, size_t>> plans;
    if (npass_over) {
      plans.push_back({true, (size_t)npass_over * nwin * tc});
      plans.push_back({true, (size_t)npass_over * nwin * ch.last});
    }
    if (lone_lag) plans.push_back({true, (size_t)nwin});
    if (int rc = wk.fft.create(ctx, wk.dev, (size_t)m, plans, st.s, nstreams)) return rc;
  }
  HIPCHK(ctx, hipStreamSynchronize(s0));            // the other stream starts behind the tables
  const int64_t tables = (int64_t)nwin * nchan * 8 + (vscale ? (int64_t)nwin * n0 * 8 : 0) + (int64_t)nwin * 4 + (int64_t)nwin * nr * 4 +
                         nr * (8 + 32 + 16);

  FtParams base = {};
  for (int i = 0; i < nin; ++i) {
    FtIn& I = base.in[i];
    I.chunked = chunked[i] ? 1 : 0;
    I.p = d_bcast[i];
    const int64_t b0 = in_shape[3 * i], b1 = in_shape[3 * i + 1], b2 = in_shape[3 * i + 2];
    I.s2 = b2 == 1 ? 0 : 1;
    I.s1 = b1 == 1 ? 0 : b2;
    I.s0 = b0 == 1 ? 0 : b1 * b2;
  }
  base.wts = d_wts; base.vscale = d_vs;
  base.n0 = n0; base.n1 = n1; base.n2 = n2;
  base.nin = nin; base.lagk = lag_rows;
  base.nwin = nwin; base.nchan = (int)nchan; base.m = (int)m; base.logm = logm; base.nres = (int)nr;
  base.df = df;
  base.fpass0 = fpass0;
  base.rs_o = rd.ofs; base.rs_k = rd.list; base.rs_in = rd.in; base.rs_c = rd.c; base.rtw = rd.rtw;
  const size_t lds_rows = rows_lds(R), lds_res = res_lds(Rr);
  if (any_over)
    if (int rc = fused ? allow_lds(ctx, k_cpft_rows<true>, lds_rows) : allow_lds(ctx, k_cpft_rows<false>, lds_rows)) return rc;
  if (any_res)
    if (int rc = allow_lds(ctx, k_cpft_resample, lds_res)) return rc;

  // the kernels of one set of rows on stream s: P holds the rows, the passes and their buffers
  auto run_rows = [&](FtParams P, int si, size_t batch) -> int {
    hipStream_t s = st.s[si];
    bool has_over = false, has_res = false;
    for (int p = 0; p < P.nin + P.lagk; ++p) {
      has_over = has_over || P.over[p];
      has_res = has_res || P.res[p];
    }
    if (has_over) {
      P.R = R;
      P.G = kThreads / pow2_at_least(R);
      const unsigned blocks = (unsigned)((P.rn + R - 1) / R);
      if (fused) {
        if (int rc = launch(ctx, k_cpft_rows<true>, dim3(blocks), lds_rows, s, P)) return rc;
      } else {
        if (int rc = launch(ctx, k_cpft_rows<false>, dim3(blocks), lds_rows, s, P)) return rc;
        if (int rc = wk.fft.run(ctx, true, batch, P.fbuf, si)) return rc;
        if (int rc = launch(ctx, k_cpft_finish, dim3((unsigned)grid_for(ctx, (int64_t)P.nwin * P.rn * m)), 0, s, P)) return rc;
      }
    }
    if (has_res) {
      P.R = Rr;
      P.G = kThreads / pow2_at_least(Rr);
      if (int rc = launch(ctx, k_cpft_resample, dim3((unsigned)((P.rn + Rr - 1) / Rr)), lds_res, s, P)) return rc;
    }
    return PRISIM_OK;
  };

  int64_t upload = tables + bcast_bytes, download = 0;
  auto upload_rows = [&](int64_t, Span sp, int si, hipStream_t s) -> int {
    const int64_t r0 = sp.first, rn = sp.count;
    for (int i = 0; i < nin; ++i)
      if (chunked[i]) HIPCHK(ctx, hipMemcpyAsync(d_in[si][i], inputs[i] + 2 * (size_t)r0 * nchan, (size_t)rn * nchan * 16, hipMemcpyHostToDevice, s));
    if (has_w) HIPCHK(ctx, hipMemcpyAsync(d_w[si], w + (size_t)r0 * nchan, (size_t)rn * nchan * 8, hipMemcpyHostToDevice, s));
    upload += rn * nchan * (nstreamed * 16 + (has_w ? 8 : 0));
    return PRISIM_OK;
  };
  auto kernels = [&](int64_t c, Span sp, int si, hipStream_t) -> int {
    const int64_t r0 = sp.first, rn = sp.count;
    FtParams P = base;
    for (int i = 0; i < nin; ++i)
      if (chunked[i]) P.in[i].p = d_in[si][i];
    P.w = d_w[si];
    P.row0 = r0; P.rn = rn;
    for (int p = 0; p < nin + lag_rows; ++p) {
      P.over[p] = d_over[si][p];
      P.res[p] = d_res[si][p];
    }
    P.fbuf = d_fbuf[si];
    if (int rc = run_rows(P, si, (size_t)npass_over * nwin * rn)) return rc;
    if (lone_lag && c == 0) {
      FtParams L = base;
      L.nin = 0; L.lagk = 1; L.w = nullptr; L.vscale = nullptr;
      L.row0 = 0; L.rn = 1; L.n0 = L.n1 = L.n2 = 1;
      L.over[0] = d_lagk; L.res[0] = d_lagk_res; L.fbuf = d_lagk_f; L.fpass0 = 0;
      if (int rc = run_rows(L, si, (size_t)nwin)) return rc;
    }
    return PRISIM_OK;
  };
  auto fetch_rows = [&](int64_t c, Span sp, int si, hipStream_t s) -> int {
    const int64_t r0 = sp.first, rn = sp.count;
    // a chunk's [nwin][rn][len] into the caller's [nwin][rows][len]
    auto fetch = [&](double* host, const double2* dev, int64_t len) -> int {
      HIPCHK(ctx, copy_rows(host + 2 * (size_t)r0 * len, (size_t)rows * len * 16, dev, (size_t)rn * len * 16, (size_t)rn * len * 16, (size_t)nwin,
                            hipMemcpyDeviceToHost, s));
      download += (int64_t)nwin * rn * len * 16;
      return PRISIM_OK;
    };
    for (int p = 0; p < nin + lag_rows; ++p) {
      const bool is_lag = p >= nin;
      if (d_over[si][p])
        if (int rc = fetch(is_lag ? lag_kernel : over[p], d_over[si][p], m)) return rc;
      if (d_res[si][p])
        if (int rc = fetch(is_lag ? lag_kernel_res : res[p], d_res[si][p], nres)) return rc;
    }
    if (lone_lag && c == 0) {
      HIPCHK(ctx, hipMemcpyAsync(lag_kernel, d_lagk, (size_t)nwin * m * 16, hipMemcpyDeviceToHost, s));
      if (lag_res) HIPCHK(ctx, hipMemcpyAsync(lag_kernel_res, d_lagk_res, (size_t)nwin * nres * 16, hipMemcpyDeviceToHost, s));
      download += (int64_t)nwin * (m + nres) * 16;
    }
    return PRISIM_OK;
  };
  if (int rc = chunk_loop(ctx, st, ch, rows, upload_rows, kernels, fetch_rows)) return rc;
  if (stats) {
    stats->wall_ms = wall_ms_since(wall0);
    stats->kernel_ms = st.kernel_ms;
    stats->rows = rows;
    stats->chunks = nchunks;
    stats->chunk_rows = tc;
    stats->row_bytes = row_bytes;
    stats->kernel_bytes = bcast_bytes + rows * nchan * (nstreamed * 16 + (has_w ? 8 : 0)) +
                          (int64_t)nwin * 16 * (rows * (npass_over * m + npass_res * nres) + (lone_lag ? m + nres : 0));
    stats->upload_bytes = upload;
    stats->download_bytes = download;
    stats->route = fused ? PRISIM_CPFT_FUSED : PRISIM_CPFT_ROCFFT;
    stats->streams = nstreams;
    stats->group_rows = R;
    stats->lds_bytes = (int32_t)lds_rows;
  }
  return PRISIM_OK;
  });
}

}  // extern "C"
