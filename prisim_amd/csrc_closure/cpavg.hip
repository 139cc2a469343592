// cpavg.hip -- incoherent averages of closure-phase power spectra for gfx950 (include/prisim_cpavg.h): the sums of
// prisim/bispectrum_phase.py:incoherent_cross_power_spectrum_average (:1116-1119, :1169-1195) and incoherent_kbin_averaging (:1479-1486).
//
// prisim_cphase_xavg.  The lag is the fastest axis of the arrays, of every buffer and of every output; a chunk is a range of lags over
// all the other axes (the rows).  The arrays are resident, one behind the other; the weights are expanded on the host to their common
// shape U and resident too.
//   k_avg_den      den = sum of the sets' weights, per element of U; once per call.
//   k_avg_wout     per combination, the sum of den over its selected positions, per element of U with the reduced axes at 1; once.
//   k_avg_stage1   avg = (sum over the sets of a w) / den of the chunk, one thread per element.
//   k_avg_stage2   per combination, (sum over the selected positions of avg W) / wout, one thread per output element; the positions
//                  are a table of row and weight offsets that the host lists in increasing flattened index.
// Threads run along the flattened (row, lag) index, so every load and store of a wavefront is contiguous in the lags.  Chunks
// alternate between two streams with their own buffers.
//
// prisim_cphase_kbin.  A chunk is one window and a range of its rows; one thread per (row, bin) walks the bin's members in order.
//   k_kbin<true>   a workgroup stages a tile of whole rows in LDS with coalesced loads and walks the members from there: folding puts
//                  lag j and lag nlags - j in one bin, so the walk itself gathers.
//   k_kbin<false>  the same walk straight from global memory, for rows that do not fit in LDS.
// Both call kb_walk and give the same bits.  No atomics; fp64 throughout, built with -ffp-contract=off.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../csrc_addon/addon_internal.h"
#include "../../include/prisim_cpavg.h"

using namespace pint;

namespace {

constexpr int kMaxRowAxes = PRISIM_CPAVG_MAX_DIM - 1;  // the axes of a row index: all but the lags
constexpr int64_t kMaxExtent = int64_t(1) << 20;      // of an axis, of the sets, of the combinations and of the bins
constexpr int64_t kMaxElems = int64_t(1) << 40;       // of an array, and of all arrays together
constexpr int64_t kTileLdsBytes = 65536;              // LDS a tile of several rows may fill; a single longer row may take the device's limit

__device__ __forceinline__ bool cnan(double2 v) { return isnan(v.x) || isnan(v.y); }

// ---- prisim_cphase_xavg ---------------------------------------------------------------------------------------------------------

// a row index over dim[0 .. nd) and the strides (0 along an axis of extent 1) of up to two arrays that broadcast against it
struct AvgAxes {
  int32_t nd;
  int64_t dim[kMaxRowAxes], s0[kMaxRowAxes], s1[kMaxRowAxes], s2[kMaxRowAxes];
};

// I: the type the index is taken apart in, uint32_t where the count allows it (a 64-bit division costs several times a 32-bit one)
template <typename I>
__device__ __forceinline__ void offsets_of(const AvgAxes& A, I t, int64_t& o0, int64_t& o1, int64_t& o2) {
  o0 = o1 = o2 = 0;
  for (int x = A.nd - 1; x >= 0; --x) {
    const I d = (I)A.dim[x], u = t / d;
    const int64_t i = (int64_t)(t - u * d);
    o0 += i * A.s0[x];
    o1 += i * A.s1[x];
    o2 += i * A.s2[x];
    t = u;
  }
}

__global__ void __launch_bounds__(kThreads) k_avg_den(const double* __restrict__ w, int64_t nsets, int64_t wtotal, double* __restrict__ den) {
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < wtotal; e += (int64_t)gridDim.x * kThreads) {
    double d = 0.0;
    for (int64_t i = 0; i < nsets; ++i) {
      const double v = w[i * wtotal + e];
      d += isnan(v) ? 0.0 : v;
    }
    den[e] = d;
  }
}

struct AvgStage1 {
  AvgAxes ax;               // the rows; s0: strides of U
  const double2* a;         // [nsets][rows][nlags]
  const double* w;          // [nsets][U]
  const double* den;        // [U]
  int64_t nsets, elems, wtotal, nlags, l0, cl, count;   // elems = rows * nlags; count = rows * cl
  double2* avg;             // [rows][cl]
};

template <typename I>
__global__ void __launch_bounds__(kThreads) k_avg_stage1(const AvgStage1 P) {
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < P.count; e += (int64_t)gridDim.x * kThreads) {
    const I t = (I)e / (I)P.cl;
    const int64_t l = (int64_t)((I)e - t * (I)P.cl);
    int64_t u, o1, o2;
    offsets_of<I>(P.ax, t, u, o1, o2);
    const double2* src = P.a + (int64_t)t * P.nlags + P.l0 + l;
    double2 num = make_double2(0.0, 0.0);
    for (int64_t i = 0; i < P.nsets; ++i) {
      const double2 v = src[i * P.elems];
      const double wv = P.w[i * P.wtotal + u];
      const double2 pr = make_double2(v.x * wv, v.y * wv);
      if (!cnan(pr)) num = cadd(num, pr);
    }
    const double d = P.den[u];
    P.avg[e] = make_double2(num.x / d, num.y / d);
  }
}

struct AvgWout {
  AvgAxes ax;               // the elements of wout; s0: strides of U
  const double* den;        // [U]
  const int64_t* sel_w;     // [nsel] offsets in U of the selected positions
  int64_t nsel, count;
  double* wout;
};

__global__ void __launch_bounds__(kThreads) k_avg_wout(const AvgWout P) {
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < P.count; e += (int64_t)gridDim.x * kThreads) {
    int64_t u, o1, o2;
    offsets_of<int64_t>(P.ax, e, u, o1, o2);
    double s = 0.0;
    for (int64_t k = 0; k < P.nsel; ++k) s += P.den[u + P.sel_w[k]];
    P.wout[e] = s;
  }
}

struct AvgStage2 {
  AvgAxes ax;               // the rows of out; s0: strides of U, s1: strides of the rows of avg, s2: strides of wout
  const double2* avg;       // [rows][cl]
  const double* den;        // [U]
  const double* wout;
  const int64_t *sel_t, *sel_w;   // [nsel] row offsets in avg and offsets in U of the selected positions
  int64_t nsel, cl, count;  // count = rows of out * cl
  double2* out;             // [rows of out][cl]
};

template <typename I>
__global__ void __launch_bounds__(kThreads) k_avg_stage2(const AvgStage2 P) {
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < P.count; e += (int64_t)gridDim.x * kThreads) {
    const I t = (I)e / (I)P.cl;
    const int64_t l = (int64_t)((I)e - t * (I)P.cl);
    int64_t u, r, o;
    offsets_of<I>(P.ax, t, u, r, o);
    double2 s = make_double2(0.0, 0.0);
    for (int64_t k = 0; k < P.nsel; ++k) {
      const double2 v = P.avg[(r + P.sel_t[k]) * P.cl + l];
      const double wv = P.den[u + P.sel_w[k]];
      s = cadd(s, make_double2(v.x * wv, v.y * wv));
    }
    const double d = P.wout[o];
    P.out[e] = make_double2(s.x / d, s.y / d);
  }
}

// ---- prisim_cphase_kbin ---------------------------------------------------------------------------------------------------------

struct Kbin {
  const double2* p;         // the chunk's rows [cr][nlags]
  const double* k;          // the window's kprll [nlags]
  const int64_t* off;       // the window's [nk + 1], positions in mem
  const int32_t* mem;
  int64_t cr, nlags, nk;
  int32_t tile;             // rows per tile of the LDS route
  double2 *ps, *del2;       // [cr][nk]
  double* kc;
};

// the three averages of one bin of one row
__device__ __forceinline__ void kb_walk(const double2* row, const double* kk, const int32_t* mem, int64_t lo, int64_t hi, double2& ps,
                                        double2& del2, double& kc) {
  double2 s = make_double2(0.0, 0.0), s3 = s;
  double sk = 0.0, sa = 0.0;
  int64_t n = 0, n3 = 0;
  for (int64_t q = lo; q < hi; ++q) {
    const int32_t j = mem[q];
    const double2 v = row[j];
    const double k = fabs(kk[j]);
    if (!cnan(v)) { s = cadd(s, v); ++n; }
    const double k3 = (k * k) * k;
    const double2 t = make_double2(k3 * v.x, k3 * v.y);
    if (!cnan(t)) { s3 = cadd(s3, t); ++n3; }
    const double a = hypot(v.x, v.y), ka = k * a;
    if (!isnan(ka)) sk += ka;
    if (!isnan(a)) sa += a;
  }
  const double c = 2.0 * M_PI * M_PI;
  ps = make_double2(s.x / (double)n, s.y / (double)n);                 // nothing left, or an empty bin: 0 / 0
  del2 = make_double2((s3.x / (double)n3) / c, (s3.y / (double)n3) / c);
  kc = sk / sa;
}

template <bool LDS>
__global__ void __launch_bounds__(kThreads) k_kbin(const Kbin P) {
  if (LDS) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double2* rows = reinterpret_cast<double2*>(smem);
    const int64_t ntiles = (P.cr + P.tile - 1) / P.tile;
    for (int64_t tl = blockIdx.x; tl < ntiles; tl += gridDim.x) {
      const int64_t r0 = tl * P.tile, nr = P.cr - r0 < P.tile ? P.cr - r0 : (int64_t)P.tile;
      const double2* src = P.p + r0 * P.nlags;
      for (int64_t i = threadIdx.x; i < nr * P.nlags; i += kThreads) rows[i] = src[i];
      __syncthreads();
      for (int64_t i = threadIdx.x; i < nr * P.nk; i += kThreads) {
        const int64_t r = i / P.nk, b = i - r * P.nk, e = (r0 + r) * P.nk + b;
        double2 ps, d2;
        double kc;
        kb_walk(rows + r * P.nlags, P.k, P.mem, P.off[b], P.off[b + 1], ps, d2, kc);
        P.ps[e] = ps;
        P.del2[e] = d2;
        P.kc[e] = kc;
      }
      __syncthreads();                                // the next tile overwrites the rows
    }
  } else {
    const int64_t total = P.cr * P.nk;
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kThreads) {
      const int64_t r = e / P.nk, b = e - r * P.nk;
      double2 ps, d2;
      double kc;
      kb_walk(P.p + r * P.nlags, P.k, P.mem, P.off[b], P.off[b + 1], ps, d2, kc);
      P.ps[e] = ps;
      P.del2[e] = d2;
      P.kc[e] = kc;
    }
  }
}

// row-major strides of `dim` with 0 along the axes of extent 1, and the number of elements
int64_t strides_of(const int64_t* dim, int nd, int64_t* str) {
  int64_t n = 1;
  for (int x = nd - 1; x >= 0; --x) {
    str[x] = dim[x] == 1 ? 0 : n;
    n *= dim[x];
  }
  return n;
}

}  // namespace

extern "C" {

int prisim_cphase_xavg(prisim_ctx* ctx, int32_t ndim, const int64_t* shape, int64_t nsets, const double* const* arrays,
                       const double* const* weights, const int64_t* wshapes, int32_t ncombo, const int32_t* reduce,
                       const uint8_t* const* masks, int64_t budget_bytes, double* avg, double* wsum, double* const* out, double* const* wout,
                       prisim_cpavg_stats* stats) {
  return guarded(ctx, [&]() -> int {
  if (!ctx) return PRISIM_EINVAL;
  const WallTime wall0 = wall_now();
  if (ndim < PRISIM_CPAVG_MIN_DIM || ndim > PRISIM_CPAVG_MAX_DIM)
    return fail(ctx, PRISIM_EINVAL, "need " + std::to_string(PRISIM_CPAVG_MIN_DIM) + " <= ndim <= " + std::to_string(PRISIM_CPAVG_MAX_DIM));
  if (!shape || !arrays || !weights || !wshapes) return fail(ctx, PRISIM_EINVAL, "null shape, arrays, weights or wshapes");
  if (nsets < 1 || nsets > kMaxExtent) return fail(ctx, PRISIM_EINVAL, "need 1 <= nsets <= 2^20");
  if (ncombo < 0 || ncombo > kMaxExtent) return fail(ctx, PRISIM_EINVAL, "need 0 <= ncombo <= 2^20");
  if (ncombo > 0 && (!reduce || !masks || !out || !wout)) return fail(ctx, PRISIM_EINVAL, "null reduce, masks, out or wout");
  const int nd = ndim - 1;
  double elems_d = 1.0;
  for (int x = 0; x < ndim; ++x) {
    if (shape[x] < 1 || shape[x] > kMaxExtent)
      return fail(ctx, PRISIM_EINVAL, "axis " + std::to_string(x) + " needs 1 to 2^20 entries; got " + std::to_string(shape[x]));
    elems_d *= (double)shape[x];
  }
  if (elems_d * (double)nsets > (double)kMaxElems) return fail(ctx, PRISIM_EINVAL, "the arrays are too large (2^40 elements at most)");
  const int64_t nlags = shape[nd];
  int64_t udim[kMaxRowAxes], ustr[kMaxRowAxes], rstr[kMaxRowAxes];
  for (int x = 0; x < nd; ++x) udim[x] = 1;
  for (int64_t i = 0; i < nsets; ++i) {
    if (!arrays[i] || !weights[i]) return fail(ctx, PRISIM_EINVAL, "null array or weights of set " + std::to_string(i));
    const int64_t* ws = wshapes + i * ndim;
    for (int x = 0; x < ndim; ++x) {
      if (ws[x] != 1 && (x == nd || ws[x] != shape[x]))
        return fail(ctx, PRISIM_EINVAL, "set " + std::to_string(i) + ": the weights have " + std::to_string(ws[x]) + " entries on axis " +
                                            std::to_string(x) + (x == nd ? ", the lags, which takes 1" : ", neither 1 nor the axis'"));
      if (x < nd) udim[x] = std::max(udim[x], ws[x]);
    }
  }
  const int64_t wtotal = strides_of(udim, nd, ustr);
  int64_t rdim[kMaxRowAxes];
  std::copy(shape, shape + nd, rdim);
  const int64_t rows = strides_of(rdim, nd, rstr);

  // the combinations: the rows of out and of wout, and the selected positions in increasing flattened index
  struct Combo {
    int64_t odim[kMaxRowAxes], wodim[kMaxRowAxes], orows, worows, first;   // first: its first row among those of all combinations
    std::vector<int64_t> sel_t, sel_w;
  };
  std::vector<Combo> combos((size_t)ncombo);
  int64_t all_orows = 0;
  for (int c = 0; c < ncombo; ++c) {
    Combo& C = combos[(size_t)c];
    if (!out[c] || !wout[c]) return fail(ctx, PRISIM_EINVAL, "null out or wout of combination " + std::to_string(c));
    const int32_t* red = reduce + (size_t)c * ndim;
    if (red[0] || red[nd]) return fail(ctx, PRISIM_EINVAL, "combination " + std::to_string(c) + " reduces the windows or the lags");
    C.sel_t.assign(1, 0);
    C.sel_w.assign(1, 0);
    for (int x = 0; x < nd; ++x) {
      C.odim[x] = red[x] ? 1 : rdim[x];
      C.wodim[x] = red[x] ? 1 : udim[x];
      if (!red[x]) continue;
      const uint8_t* mk = masks[(size_t)c * ndim + x];
      if (!mk) return fail(ctx, PRISIM_EINVAL, "combination " + std::to_string(c) + ": null mask of the reduced axis " + std::to_string(x));
      std::vector<int64_t> pos;
      for (int64_t i = 0; i < rdim[x]; ++i)
        if (mk[i]) pos.push_back(i);
      if (pos.empty()) return fail(ctx, PRISIM_EINVAL, "combination " + std::to_string(c) + " selects nothing on axis " + std::to_string(x));
      // the axes come in increasing order, so appending the positions of this one inside the earlier ones keeps the flattened order
      std::vector<int64_t> nt, nw;
      nt.reserve(C.sel_t.size() * pos.size());
      nw.reserve(nt.capacity());
      for (size_t k = 0; k < C.sel_t.size(); ++k)
        for (int64_t i : pos) {
          nt.push_back(C.sel_t[k] + i * rstr[x]);
          nw.push_back(C.sel_w[k] + i * ustr[x]);
        }
      C.sel_t.swap(nt);
      C.sel_w.swap(nw);
    }
    int64_t tmp[kMaxRowAxes];
    C.orows = strides_of(C.odim, nd, tmp);
    C.worows = strides_of(C.wodim, nd, tmp);
    C.first = all_orows;
    all_orows += C.orows;
  }

  // every weight at the shape U
  std::vector<double> wexp((size_t)nsets * (size_t)wtotal);
  for (int64_t i = 0; i < nsets; ++i) {
    const int64_t* ws = wshapes + i * ndim;
    int64_t sstr[kMaxRowAxes];
    strides_of(ws, nd, sstr);
    for (int64_t e = 0; e < wtotal; ++e) {
      int64_t t = e, o = 0;
      for (int x = nd - 1; x >= 0; --x) {
        const int64_t u = t / udim[x];
        o += (t - u * udim[x]) * sstr[x];
        t = u;
      }
      wexp[(size_t)(i * wtotal + e)] = weights[i][o];
    }
  }

  const int64_t lag_bytes = 16 * (rows + all_orows);
  const Chunks ch = plan_chunks(nlags, lag_bytes, budget_bytes, kMaxStreams);
  const int64_t tc = ch.size, nchunks = ch.count;
  const int nstreams = (int)std::min<int64_t>(kMaxStreams, nchunks);
  const int64_t elems = rows * nlags;

  HIPCHK(ctx, hipSetDevice(ctx->device));
  Work wk;
  Streams& st = wk.st;
  if (int rc = st.create(ctx, nstreams, true)) return rc;
  hipStream_t s0 = st.s[0];
  double2* d_a;
  DEV_ALLOC(ctx, wk.dev, d_a, (size_t)nsets * (size_t)elems * 16);
  for (int64_t i = 0; i < nsets; ++i)
    HIPCHK(ctx, hipMemcpyAsync(d_a + (size_t)i * (size_t)elems, arrays[i], (size_t)elems * 16, hipMemcpyHostToDevice, s0));
  double *d_w, *d_den;
  DEV_UPLOAD(ctx, wk.dev, d_w, wexp, s0);
  DEV_ALLOC(ctx, wk.dev, d_den, (size_t)wtotal * 8);
  int64_t tables = nsets * wtotal * 8;
  std::vector<int64_t*> d_sel_t((size_t)ncombo), d_sel_w((size_t)ncombo);
  std::vector<double*> d_wout((size_t)ncombo);
  for (int c = 0; c < ncombo; ++c) {
    DEV_UPLOAD(ctx, wk.dev, d_sel_t[(size_t)c], combos[(size_t)c].sel_t, s0);
    DEV_UPLOAD(ctx, wk.dev, d_sel_w[(size_t)c], combos[(size_t)c].sel_w, s0);
    DEV_ALLOC(ctx, wk.dev, d_wout[(size_t)c], (size_t)combos[(size_t)c].worows * 8);
    tables += 16 * (int64_t)combos[(size_t)c].sel_t.size();
  }
  double2 *d_avg[kMaxStreams] = {}, *d_out[kMaxStreams] = {};
  for (int s = 0; s < nstreams; ++s) {
    DEV_ALLOC(ctx, wk.dev, d_avg[s], (size_t)rows * tc * 16);
    DEV_ALLOC(ctx, wk.dev, d_out[s], (size_t)all_orows * tc * 16);
  }

  int64_t download = 0;
  auto axes = [&](const int64_t* dim, const int64_t* a0, const int64_t* a1, const int64_t* a2) {
    AvgAxes A = {};
    A.nd = nd;
    for (int x = 0; x < nd; ++x) {
      A.dim[x] = dim[x];
      A.s0[x] = dim[x] == 1 ? 0 : a0[x];
      A.s1[x] = (a1 && dim[x] != 1) ? a1[x] : 0;
      A.s2[x] = (a2 && dim[x] != 1) ? a2[x] : 0;
    }
    return A;
  };
  // the weight sums, once, on the first stream
  if (int rc = st.open(ctx, 0)) return rc;
  if (int rc = launch(ctx, k_avg_den, dim3((unsigned)grid_for(ctx, wtotal)), 0, s0, d_w, nsets, wtotal, d_den)) return rc;
  for (int c = 0; c < ncombo; ++c) {
    const Combo& C = combos[(size_t)c];
    AvgWout W = {};
    W.ax = axes(C.wodim, ustr, nullptr, nullptr);
    W.den = d_den;
    W.sel_w = d_sel_w[(size_t)c];
    W.nsel = (int64_t)C.sel_w.size();
    W.count = C.worows;
    W.wout = d_wout[(size_t)c];
    if (int rc = launch(ctx, k_avg_wout, dim3((unsigned)grid_for(ctx, W.count)), 0, s0, W)) return rc;
  }
  if (int rc = st.close(ctx, 0)) return rc;
  if (wsum) {
    HIPCHK(ctx, hipMemcpyAsync(wsum, d_den, (size_t)wtotal * 8, hipMemcpyDeviceToHost, s0));
    download += wtotal * 8;
  }
  for (int c = 0; c < ncombo; ++c) {
    HIPCHK(ctx, hipMemcpyAsync(wout[c], d_wout[(size_t)c], (size_t)combos[(size_t)c].worows * 8, hipMemcpyDeviceToHost, s0));
    download += combos[(size_t)c].worows * 8;
  }
  HIPCHK(ctx, hipStreamSynchronize(s0));              // the other stream starts behind the inputs and the weight sums; chunk 0 harvests

  auto kernels = [&](int64_t, Span sp, int si, hipStream_t s) -> int {
    const int64_t l0 = sp.first, cl = sp.count;
    AvgStage1 S = {};
    S.ax = axes(rdim, ustr, nullptr, nullptr);
    S.a = d_a;
    S.w = d_w;
    S.den = d_den;
    S.nsets = nsets; S.elems = elems; S.wtotal = wtotal; S.nlags = nlags;
    S.l0 = l0; S.cl = cl;
    S.count = rows * cl;
    S.avg = d_avg[si];
    const bool narrow = rows * cl <= (int64_t)UINT32_MAX;   // every count of this chunk fits 32 bits: rows * cl is the largest
    if (int rc = launch(ctx, narrow ? k_avg_stage1<uint32_t> : k_avg_stage1<int64_t>, dim3((unsigned)grid_for(ctx, S.count)), 0, s, S)) return rc;
    for (int k = 0; k < ncombo; ++k) {
      const Combo& C = combos[(size_t)k];
      int64_t wostr[kMaxRowAxes];
      strides_of(C.wodim, nd, wostr);
      AvgStage2 T = {};
      T.ax = axes(C.odim, ustr, rstr, wostr);        // ustr and wostr are 0 along an axis that the weights broadcast over
      T.avg = d_avg[si];
      T.den = d_den;
      T.wout = d_wout[(size_t)k];
      T.sel_t = d_sel_t[(size_t)k];
      T.sel_w = d_sel_w[(size_t)k];
      T.nsel = (int64_t)C.sel_t.size();
      T.cl = cl;
      T.count = C.orows * cl;
      T.out = d_out[si] + (size_t)C.first * cl;
      if (int rc = launch(ctx, narrow ? k_avg_stage2<uint32_t> : k_avg_stage2<int64_t>, dim3((unsigned)grid_for(ctx, T.count)), 0, s, T)) return rc;
    }
    return PRISIM_OK;
  };
  // the chunk's [rows][cl] into the caller's [rows][nlags]
  auto fetch = [&](int64_t, Span sp, int si, hipStream_t s) -> int {
    const int64_t l0 = sp.first, cl = sp.count;
    if (avg) {
      HIPCHK(ctx, copy_rows(avg + 2 * (size_t)l0, (size_t)nlags * 16, d_avg[si], (size_t)cl * 16, (size_t)cl * 16, (size_t)rows,
                            hipMemcpyDeviceToHost, s));
      download += rows * cl * 16;
    }
    for (int k = 0; k < ncombo; ++k) {
      const Combo& C = combos[(size_t)k];
      HIPCHK(ctx, copy_rows(out[k] + 2 * (size_t)l0, (size_t)nlags * 16, d_out[si] + (size_t)C.first * cl, (size_t)cl * 16, (size_t)cl * 16,
                            (size_t)C.orows, hipMemcpyDeviceToHost, s));
      download += C.orows * cl * 16;
    }
    return PRISIM_OK;
  };
  if (int rc = chunk_loop(ctx, st, ch, nlags, no_step, kernels, fetch)) return rc;
  if (stats) {
    int64_t moved = nsets * elems * 16 + elems * 16;  // the arrays once, avg written once
    for (const Combo& C : combos) moved += C.orows * nlags * 16 * ((int64_t)C.sel_t.size() + 1);   // its selected rows read, out written
    stats->wall_ms = wall_ms_since(wall0);
    stats->kernel_ms = st.kernel_ms;
    stats->chunks = nchunks;
    stats->kernel_bytes = moved;
    stats->upload_bytes = nsets * elems * 16 + tables;
    stats->download_bytes = download;
    stats->route = PRISIM_CPAVG_AUTO;
    stats->lds_limit = 0;
  }
  return PRISIM_OK;
  });
}

int prisim_cphase_kbin(prisim_ctx* ctx, int64_t nspw, int64_t m, int64_t nlags, int64_t nk, const double* p, const double* kprll,
                       const int64_t* offsets, const int32_t* members, int32_t route, int64_t budget_bytes, double* ps, double* del2,
                       double* kc, prisim_cpavg_stats* stats) {
  return guarded(ctx, [&]() -> int {
  if (!ctx) return PRISIM_EINVAL;
  const WallTime wall0 = wall_now();
  if (nspw < 1 || m < 1 || nlags < 1 || nk < 1) return fail(ctx, PRISIM_EINVAL, "need nspw, m, nlags and nk >= 1");
  if (nspw > kMaxExtent || m > kMaxExtent || nlags > kMaxExtent || nk > kMaxExtent)
    return fail(ctx, PRISIM_EINVAL, "an extent is too large (2^20 at most)");
  if ((double)nspw * (double)m * (double)std::max(nlags, nk) > (double)kMaxElems)
    return fail(ctx, PRISIM_EINVAL, "the arrays are too large (2^40 elements at most)");
  if (!p || !kprll || !offsets || !ps || !del2 || !kc) return fail(ctx, PRISIM_EINVAL, "null p, kprll, offsets, ps, del2 or kc");
  if (route < PRISIM_CPAVG_AUTO || route > PRISIM_CPAVG_GLOBAL) return fail(ctx, PRISIM_EINVAL, "unknown route");
  // the offsets as positions in the concatenated members
  std::vector<int64_t> off((size_t)nspw * (size_t)(nk + 1));
  int64_t base = 0;
  for (int64_t w = 0; w < nspw; ++w) {
    const int64_t* o = offsets + w * (nk + 1);
    if (o[0] != 0) return fail(ctx, PRISIM_EINVAL, "window " + std::to_string(w) + ": the offsets must start at 0");
    for (int64_t b = 0; b < nk; ++b)
      if (o[b + 1] < o[b] || o[b + 1] - o[b] > nlags)
        return fail(ctx, PRISIM_EINVAL, "window " + std::to_string(w) + ": the offsets of bin " + std::to_string(b) +
                                            " decrease or hold more members than there are lags");
    if (o[nk] > 0 && !members) return fail(ctx, PRISIM_EINVAL, "null members");
    for (int64_t b = 0; b < nk; ++b)
      for (int64_t q = o[b]; q < o[b + 1]; ++q) {
        const int64_t j = members[base + q];
        if (j < 0 || j >= nlags || (q > o[b] && j <= members[base + q - 1]))
          return fail(ctx, PRISIM_EINVAL, "window " + std::to_string(w) + ", bin " + std::to_string(b) + ": member " + std::to_string(j) +
                                              " is not a lag in [0, " + std::to_string(nlags) + ") or not above the member before it");
      }
    for (int64_t b = 0; b <= nk; ++b) off[(size_t)(w * (nk + 1) + b)] = base + o[b];
    base += o[nk];
  }
  const int64_t nmem = base;

  HIPCHK(ctx, hipSetDevice(ctx->device));
  int lds_max = 0;
  if (int rc = lds_limit(ctx, lds_max)) return rc;
  const bool row_fits = nlags * 16 <= (int64_t)lds_max;
  if (route == PRISIM_CPAVG_LDS && !row_fits)
    return fail(ctx, PRISIM_EINVAL, "a row of the LDS route does not fit in LDS (" + std::to_string(nlags * 16) + " B needed, " +
                                        std::to_string(lds_max) + " B there)");
  const bool lds = route != PRISIM_CPAVG_GLOBAL && row_fits;

  const Chunks ch = plan_chunks(m, 40 * nk, budget_bytes, kMaxStreams);
  const int64_t tc = ch.size, nchunks = nspw * ch.count;
  const int nstreams = (int)std::min<int64_t>(kMaxStreams, nchunks);
  // rows per tile: as many as fit in kTileLdsBytes, one where a single row is longer than that
  const int64_t tile = std::max<int64_t>(1, std::min<int64_t>(tc, kTileLdsBytes / (16 * nlags)));
  const int64_t lds_bytes = lds ? tile * nlags * 16 : 0;
  if (lds_bytes > (int64_t)lds_max) return fail(ctx, PRISIM_EINTERNAL, "internal: the tile exceeds the LDS");

  Work wk;
  Streams& st = wk.st;
  if (int rc = st.create(ctx, nstreams, true)) return rc;
  hipStream_t s0 = st.s[0];
  const size_t in_elems = (size_t)nspw * (size_t)m * (size_t)nlags;
  double2* d_p;
  double* d_k;
  int64_t* d_off;
  int32_t* d_mem;
  DEV_UPLOAD(ctx, wk.dev, d_p, p, in_elems * 2, s0);
  DEV_UPLOAD(ctx, wk.dev, d_k, kprll, (size_t)nspw * (size_t)nlags, s0);
  DEV_UPLOAD(ctx, wk.dev, d_off, off, s0);
  DEV_UPLOAD(ctx, wk.dev, d_mem, members, (size_t)nmem, s0);
  double2 *d_ps[kMaxStreams] = {}, *d_d2[kMaxStreams] = {};
  double* d_kc[kMaxStreams] = {};
  for (int s = 0; s < nstreams; ++s) {
    DEV_ALLOC(ctx, wk.dev, d_ps[s], (size_t)tc * nk * 16);
    DEV_ALLOC(ctx, wk.dev, d_d2[s], (size_t)tc * nk * 16);
    DEV_ALLOC(ctx, wk.dev, d_kc[s], (size_t)tc * nk * 8);
  }
  if (lds)
    if (int rc = allow_lds(ctx, k_kbin<true>, lds_bytes)) return rc;
  HIPCHK(ctx, hipStreamSynchronize(s0));              // the other stream starts behind the inputs; `off` may go

  int64_t download = 0;
  // chunk c: a range of the rows of window c / ch.count
  auto kernels = [&](int64_t c, Span sp, int si, hipStream_t s) -> int {
    const int64_t w = c / ch.count, r0 = sp.first, cr = sp.count;
    Kbin K = {};
    K.p = d_p + ((size_t)w * m + r0) * nlags;
    K.k = d_k + (size_t)w * nlags;
    K.off = d_off + (size_t)w * (nk + 1);
    K.mem = d_mem;
    K.cr = cr; K.nlags = nlags; K.nk = nk;
    K.tile = (int32_t)tile;
    K.ps = d_ps[si]; K.del2 = d_d2[si]; K.kc = d_kc[si];
    if (!lds) return launch(ctx, k_kbin<false>, dim3((unsigned)grid_for(ctx, cr * nk)), 0, s, K);
    const int64_t ntiles = (cr + tile - 1) / tile;
    const unsigned blocks = (unsigned)std::min<int64_t>(ntiles, (int64_t)std::max(ctx->cu_count, 1) * 16);
    return launch(ctx, k_kbin<true>, dim3(blocks), (size_t)lds_bytes, s, K);
  };
  auto fetch = [&](int64_t c, Span sp, int si, hipStream_t s) -> int {
    const int64_t w = c / ch.count, r0 = sp.first, cr = sp.count;
    const size_t o = ((size_t)w * m + r0) * nk, n = (size_t)cr * nk;
    HIPCHK(ctx, hipMemcpyAsync(ps + 2 * o, d_ps[si], n * 16, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipMemcpyAsync(del2 + 2 * o, d_d2[si], n * 16, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipMemcpyAsync(kc + o, d_kc[si], n * 8, hipMemcpyDeviceToHost, s));
    download += (int64_t)n * 40;
    return PRISIM_OK;
  };
  if (int rc = chunk_loop(ctx, st, ch, m, no_step, kernels, fetch, nspw)) return rc;
  if (stats) {
    const int64_t tables = nspw * nlags * 8 + nspw * (nk + 1) * 8 + nmem * 4;
    stats->wall_ms = wall_ms_since(wall0);
    stats->kernel_ms = st.kernel_ms;
    stats->chunks = nchunks;
    stats->kernel_bytes = (int64_t)in_elems * 16 + tables + nspw * m * nk * 40;
    stats->upload_bytes = (int64_t)in_elems * 16 + tables;
    stats->download_bytes = download;
    stats->route = lds ? PRISIM_CPAVG_LDS : PRISIM_CPAVG_GLOBAL;
    stats->lds_limit = lds_max;
  }
  return PRISIM_OK;
  });
}

}  // extern "C"
