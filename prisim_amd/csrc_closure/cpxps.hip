// cpxps.hip -- cross power of closure-phase delay spectra for gfx950 (include/prisim_cpxps.h): the cross products of
// prisim/bispectrum_phase.py:ClosurePhaseDelaySpectrum.compute_power_spectrum (:3468-3551) and their collapses.
//
// Everything is independent per window and per lag, and the lag is the fastest axis of the inputs, of every buffer and of the output.
// A chunk is one window and a range of lags (the whole row when the budget allows).  Within a chunk a buffer is a tensor
// [d1a][d1b][d2a][d2b][d3a][d3b][cl]: per axis a pair of extents, (n, 1) for an axis that is not crossed, (nshift, n1) for the LST
// axis and (n, n) for days and triads when crossed, and (nshift, 1) or (2n-1, 1) once collapsed.
//   k_xp_cross    writes P = (factor (a wa)) conj(b wb) of the chunk, one thread per element, from the two resident inputs.
//   k_xp_lst_mean, k_xp_lst_median, k_xp_trace
//                 one per collapsed axis, in the caller's order: reads [outer][da][db][inner] and writes [outer][dout][inner] into the
//                 other of two ping-pong buffers, one thread per output element, the reduction sequential in increasing i.  The median
//                 selects by rank counting as cpbins.hip does: for every element that is not NaN one walk over the others counts those
//                 below it, ties broken by position; the values of rank (m - 1) / 2 and m / 2 are kept.  Its second walk finds its
//                 operands in L2.
// Threads run along the flattened fastest extents, which end in the lags, so every load and store of a wavefront is contiguous.  No
// atomics, no LDS, no scratch.  The last buffer is copied into the caller's output with its lag pitch; when no axis is collapsed that
// is the cross kernel's buffer.  Chunks alternate between two streams with their own buffers, so that the kernels of one overlap the
// download of the other.  fp64 throughout, built with -ffp-contract=off.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../csrc_addon/addon_internal.h"
#include "../../include/prisim_cpxps.h"

using namespace pint;

namespace {

constexpr int64_t kMaxExtent = int64_t(1) << 20;      // of an axis, and of the shifts
constexpr int64_t kMaxElems = int64_t(1) << 40;       // of the uncollapsed product per window and lag

struct XpCross {
  const double2 *a, *b;     // this window's [n1][n2][n3][nlags]
  const double2* w[3];      // per axis [n]
  const int64_t* shifts;    // [nshift]
  double factor;
  int64_t n2, n3, nlags;
  int64_t l0, cl;           // the chunk's first lag and its lags
  int64_t da[3], db[3];     // the pair of extents per axis
  int32_t crossed[3];
  int64_t total;            // elements of the chunk
  double2* out;
};

struct XpCollapse {
  const double2* in;        // [outer][da][db][inner]
  double2* out;             // [outer][dout][inner]
  int64_t outer, da, db, dout, inner;
};

__device__ __forceinline__ bool cnan(double2 v) { return isnan(v.x) || isnan(v.y); }
__device__ __forceinline__ bool cless(double2 u, double2 v) { return u.x < v.x || (u.x == v.x && u.y < v.y); }

__global__ void __launch_bounds__(kThreads) k_xp_cross(const XpCross P) {
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < P.total; e += (int64_t)gridDim.x * kThreads) {
    int64_t t = e / P.cl;
    const int64_t l = e - t * P.cl;
    int64_t ia[3], ib[3];
#pragma unroll
    for (int x = 2; x >= 0; --x) {
      const int64_t u = t / P.db[x], jb = t - u * P.db[x];
      t = u / P.da[x];
      const int64_t ja = u - t * P.da[x];
      if (!P.crossed[x]) { ia[x] = ja; ib[x] = ja; }
      else if (x == 0) { ia[x] = jb; ib[x] = jb - P.shifts[ja]; }
      else { ia[x] = ja; ib[x] = jb; }
    }
    double2 v = make_double2(nan, nan);
    if (ib[0] >= 0) {
      const double2 wa = cmul(cmul(P.w[0][ia[0]], P.w[1][ia[1]]), P.w[2][ia[2]]);
      const double2 wb = cmul(cmul(P.w[0][ib[0]], P.w[1][ib[1]]), P.w[2][ib[2]]);
      const double2 av = P.a[((ia[0] * P.n2 + ia[1]) * P.n3 + ia[2]) * P.nlags + P.l0 + l];
      const double2 bv = P.b[((ib[0] * P.n2 + ib[1]) * P.n3 + ib[2]) * P.nlags + P.l0 + l];
      v = cmulc(cmul(make_double2(P.factor, 0.0), cmul(av, wa)), cmul(bv, wb));
    }
    P.out[e] = v;
  }
}

// the mean over i of the elements [s][i] that are not NaN
__global__ void __launch_bounds__(kThreads) k_xp_lst_mean(const XpCollapse P) {
  const int64_t total = P.outer * P.dout * P.inner;
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kThreads) {
    const int64_t or_ = e / P.inner, q = e - or_ * P.inner, o = or_ / P.dout, s = or_ - o * P.dout;
    const double2* src = P.in + ((o * P.da + s) * P.db) * P.inner + q;
    double2 sum = make_double2(0.0, 0.0);
    int64_t cnt = 0;
    for (int64_t i = 0; i < P.db; ++i) {
      const double2 v = src[i * P.inner];
      if (!cnan(v)) { sum = cadd(sum, v); ++cnt; }
    }
    P.out[e] = make_double2(sum.x / (double)cnt, sum.y / (double)cnt);      // none left: 0 / 0
  }
}

// the median over i of the elements [s][i] that are not NaN
__global__ void __launch_bounds__(kThreads) k_xp_lst_median(const XpCollapse P) {
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  const int64_t total = P.outer * P.dout * P.inner;
  const int n = (int)P.db;
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kThreads) {
    const int64_t or_ = e / P.inner, q = e - or_ * P.inner, o = or_ / P.dout, s = or_ - o * P.dout;
    const double2* src = P.in + ((o * P.da + s) * P.db) * P.inner + q;
    int m = 0;
    for (int i = 0; i < n; ++i) m += cnan(src[i * P.inner]) ? 0 : 1;
    const int rlo = (m - 1) / 2, rhi = m / 2;
    double2 lo = make_double2(nan, nan), hi = lo;
    for (int i = 0; i < n && m > 0; ++i) {
      const double2 v = src[i * P.inner];
      if (cnan(v)) continue;
      int rank = 0;
      for (int j = 0; j < n; ++j) {
        const double2 u = src[j * P.inner];
        if (cnan(u)) continue;
        rank += (cless(u, v) || (j < i && !cless(v, u))) ? 1 : 0;
      }
      if (rank == rlo) lo = v;
      if (rank == rhi) hi = v;
    }
    P.out[e] = rlo == rhi ? lo : rmul(cadd(lo, hi), 0.5);
  }
}

// the mean along the diagonals of offset k = r - (n - 1): (sum over i of [i][i + k]) / (n - |k|)
__global__ void __launch_bounds__(kThreads) k_xp_trace(const XpCollapse P) {
  const int64_t total = P.outer * P.dout * P.inner, n = P.da;
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kThreads) {
    const int64_t or_ = e / P.inner, q = e - or_ * P.inner, o = or_ / P.dout, r = or_ - o * P.dout;
    const int64_t k = r - (n - 1), i0 = k < 0 ? -k : 0, i1 = k < 0 ? n : n - k;
    const double2* src = P.in + (o * n * n) * P.inner + q;
    double2 sum = make_double2(0.0, 0.0);
    for (int64_t i = i0; i < i1; ++i) sum = cadd(sum, src[(i * n + i + k) * P.inner]);
    const double cnt = (double)(i1 - i0);
    P.out[e] = make_double2(sum.x / cnt, sum.y / cnt);
  }
}

}  // namespace

extern "C" {

int prisim_cphase_xpower(prisim_ctx* ctx, int64_t nspw, int64_t n1, int64_t n2, int64_t n3, int64_t nlags, const double* a, const double* b,
                         const double* factor, const double* const* weights, const int32_t* modes, int64_t nshift, const int64_t* shifts,
                         int32_t ncollapse, const int32_t* order, int32_t stat, int64_t budget_bytes, double* out, prisim_cpxps_stats* stats) {
  return guarded(ctx, [&]() -> int {
  if (!ctx) return PRISIM_EINVAL;
  const WallTime wall0 = wall_now();
  const int64_t n[3] = {n1, n2, n3};
  if (nspw < 1 || n1 < 1 || n2 < 1 || n3 < 1 || nlags < 1) return fail(ctx, PRISIM_EINVAL, "need nspw, n1, n2, n3 and nlags >= 1");
  if (nspw > kMaxExtent || n1 > kMaxExtent || n2 > kMaxExtent || n3 > kMaxExtent || nlags > kMaxExtent)
    return fail(ctx, PRISIM_EINVAL, "an extent is too large (2^20 at most)");
  if (!a || !factor || !modes || !out) return fail(ctx, PRISIM_EINVAL, "null a, factor, modes or out");
  int want_collapse = 0;
  for (int x = 0; x < 3; ++x) {
    if (modes[x] < PRISIM_CPXPS_NONE || modes[x] > PRISIM_CPXPS_COLLAPSE)
      return fail(ctx, PRISIM_EINVAL, "unknown mode of axis " + std::to_string(x + 1));
    if (modes[x] == PRISIM_CPXPS_COLLAPSE) ++want_collapse;
  }
  if (stat != PRISIM_CPXPS_MEAN && stat != PRISIM_CPXPS_MEDIAN) return fail(ctx, PRISIM_EINVAL, "unknown statistic");
  const bool lst_crossed = modes[0] != PRISIM_CPXPS_NONE;
  if (lst_crossed) {
    if (nshift < 1 || nshift > kMaxExtent || !shifts) return fail(ctx, PRISIM_EINVAL, "a crossed LST axis needs 1 to 2^20 shifts");
    for (int64_t i = 0; i < nshift; ++i)
      if (shifts[i] < 0 || shifts[i] >= n1)
        return fail(ctx, PRISIM_EINVAL, "LST shift " + std::to_string(shifts[i]) + " is not in [0, n1 = " + std::to_string(n1) + ")");
  } else {
    nshift = 0;
  }
  if (ncollapse != want_collapse || (ncollapse > 0 && !order))
    return fail(ctx, PRISIM_EINVAL, "the order must list every collapsed axis once (" + std::to_string(want_collapse) + " of them)");
  bool seen[3] = {};
  for (int c = 0; c < ncollapse; ++c) {
    const int x = order[c] - 1;
    if (x < 0 || x > 2 || modes[x] != PRISIM_CPXPS_COLLAPSE || seen[x])
      return fail(ctx, PRISIM_EINVAL, "the order must list every collapsed axis (1, 2, 3) once; got " + std::to_string(order[c]));
    seen[x] = true;
  }
  if (modes[0] == PRISIM_CPXPS_COLLAPSE && stat == PRISIM_CPXPS_MEDIAN && n1 > PRISIM_CPXPS_MAX_MEDIAN)
    return fail(ctx, PRISIM_EINVAL, "the median takes " + std::to_string(PRISIM_CPXPS_MAX_MEDIAN) + " LST bins at most (PRISIM_CPXPS_MAX_MEDIAN); got " +
                                        std::to_string(n1));

  // the pairs of extents per axis: of the cross product, and as the collapses leave them
  int64_t da[3], db[3];
  for (int x = 0; x < 3; ++x) {
    const bool crossed = modes[x] != PRISIM_CPXPS_NONE;
    da[x] = !crossed ? n[x] : x == 0 ? nshift : n[x];
    db[x] = crossed ? n[x] : 1;
  }
  auto elems = [&]() {
    double p = 1.0;
    for (int x = 0; x < 3; ++x) p *= (double)da[x] * (double)db[x];
    return p;
  };
  if (elems() > (double)kMaxElems) return fail(ctx, PRISIM_EINVAL, "the cross product is too large (2^40 elements per window and lag at most)");
  const int64_t pe = (int64_t)elems();
  // elements per lag of the buffer behind every collapse; the two ping-pong buffers take the largest of the even and of the odd ones
  int64_t stage[4] = {pe, 0, 0, 0}, fa[3], fb[3];
  std::copy(da, da + 3, fa);
  std::copy(db, db + 3, fb);
  for (int c = 0; c < ncollapse; ++c) {
    const int x = order[c] - 1;
    fa[x] = x == 0 ? nshift : 2 * n[x] - 1;
    fb[x] = 1;
    stage[c + 1] = fa[0] * fb[0] * fa[1] * fb[1] * fa[2] * fb[2];
  }
  const int64_t oe = stage[ncollapse];
  const int64_t buf_elems[2] = {std::max(stage[0], stage[2]), std::max(stage[1], stage[3])};
  const int64_t lag_bytes = 16 * (buf_elems[0] + buf_elems[1]);
  const Chunks ch = plan_chunks(nlags, lag_bytes, budget_bytes, kMaxStreams);
  const int64_t tc = ch.size, nchunks = nspw * ch.count;
  const int nstreams = (int)std::min<int64_t>(kMaxStreams, nchunks);

  HIPCHK(ctx, hipSetDevice(ctx->device));
  Work wk;
  Streams& st = wk.st;
  if (int rc = st.create(ctx, nstreams, true)) return rc;
  hipStream_t s0 = st.s[0];
  const size_t in_elems = (size_t)nspw * n1 * n2 * n3 * nlags;
  double2 *d_a, *d_b, *d_w[3];
  int64_t* d_shifts;
  DEV_UPLOAD(ctx, wk.dev, d_a, a, in_elems * 2, s0);
  d_b = d_a;
  if (b) DEV_UPLOAD(ctx, wk.dev, d_b, b, in_elems * 2, s0);
  int64_t tables = 0;
  for (int x = 0; x < 3; ++x) {
    const double* w = weights ? weights[x] : nullptr;
    std::vector<double> ones;
    if (!w) {
      ones.assign(2 * (size_t)n[x], 0.0);
      for (int64_t i = 0; i < n[x]; ++i) ones[2 * i] = 1.0;
      w = ones.data();
    }
    DEV_UPLOAD(ctx, wk.dev, d_w[x], w, (size_t)n[x] * 2, s0);
    HIPCHK(ctx, hipStreamSynchronize(s0));            // `ones` goes
    tables += n[x] * 16;
  }
  DEV_UPLOAD(ctx, wk.dev, d_shifts, shifts, (size_t)nshift, s0);
  tables += nshift * 8;
  double2* d_buf[kMaxStreams][2] = {};
  for (int s = 0; s < nstreams; ++s)
    for (int k = 0; k < 2; ++k) DEV_ALLOC(ctx, wk.dev, d_buf[s][k], (size_t)buf_elems[k] * tc * 16);
  HIPCHK(ctx, hipStreamSynchronize(s0));              // the other stream starts behind the inputs

  int64_t download = 0;
  // chunk c: a range of the lags of window c / ch.count
  auto kernels = [&](int64_t c, Span sp, int si, hipStream_t s) -> int {
    const int64_t w = c / ch.count, l0 = sp.first, cl = sp.count;
    XpCross X = {};
    X.a = d_a + (size_t)w * n1 * n2 * n3 * nlags;
    X.b = d_b + (size_t)w * n1 * n2 * n3 * nlags;
    for (int x = 0; x < 3; ++x) {
      X.w[x] = d_w[x];
      X.da[x] = da[x];
      X.db[x] = db[x];
      X.crossed[x] = modes[x] != PRISIM_CPXPS_NONE;
    }
    X.shifts = d_shifts;
    X.factor = factor[w];
    X.n2 = n2; X.n3 = n3; X.nlags = nlags;
    X.l0 = l0; X.cl = cl;
    X.total = pe * cl;
    X.out = d_buf[si][0];
    if (int rc = launch(ctx, k_xp_cross, dim3((unsigned)grid_for(ctx, X.total)), 0, s, X)) return rc;
    int64_t ca[3], cb[3];
    std::copy(da, da + 3, ca);
    std::copy(db, db + 3, cb);
    for (int k = 0; k < ncollapse; ++k) {
      const int x = order[k] - 1;
      XpCollapse C = {};
      C.in = d_buf[si][k & 1];
      C.out = d_buf[si][(k + 1) & 1];
      C.outer = 1;
      C.inner = cl;
      for (int y = 0; y < x; ++y) C.outer *= ca[y] * cb[y];
      for (int y = x + 1; y < 3; ++y) C.inner *= ca[y] * cb[y];
      C.da = ca[x]; C.db = cb[x];
      C.dout = x == 0 ? nshift : 2 * n[x] - 1;
      const unsigned blocks = (unsigned)grid_for(ctx, C.outer * C.dout * C.inner);
      if (int rc = launch(ctx, x != 0 ? k_xp_trace : stat == PRISIM_CPXPS_MEAN ? k_xp_lst_mean : k_xp_lst_median, dim3(blocks), 0, s, C)) return rc;
      ca[x] = C.dout;
      cb[x] = 1;
    }
    return PRISIM_OK;
  };
  // the chunk's [oe][cl] into the caller's [nspw][oe][nlags]
  auto fetch = [&](int64_t c, Span sp, int si, hipStream_t s) -> int {
    const int64_t w = c / ch.count, l0 = sp.first, cl = sp.count;
    HIPCHK(ctx, copy_rows(out + 2 * ((size_t)w * oe * nlags + l0), (size_t)nlags * 16, d_buf[si][ncollapse & 1], (size_t)cl * 16, (size_t)cl * 16,
                          (size_t)oe, hipMemcpyDeviceToHost, s));
    download += oe * cl * 16;
    return PRISIM_OK;
  };
  if (int rc = chunk_loop(ctx, st, ch, nlags, no_step, kernels, fetch, nspw)) return rc;
  if (stats) {
    int64_t moved = 0;                                // per window and lag: every buffer written once, and read once by the next kernel
    for (int k = 0; k <= ncollapse; ++k) moved += stage[k] * (k < ncollapse ? 2 : 1);
    stats->wall_ms = wall_ms_since(wall0);
    stats->kernel_ms = st.kernel_ms;
    stats->chunks = nchunks;
    stats->chunk_lags = tc;
    stats->kernel_bytes = (int64_t)in_elems * 16 * (b ? 2 : 1) + nspw * nlags * moved * 16;
    stats->upload_bytes = (int64_t)in_elems * 16 * (b ? 2 : 1) + tables;
    stats->download_bytes = download;
    stats->cross_bytes = nspw * nlags * pe * 16;
  }
  return PRISIM_OK;
  });
}

}  // extern "C"
