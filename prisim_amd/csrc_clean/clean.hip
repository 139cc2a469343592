// clean.hip -- delay-spectrum CLEAN for gfx950 (include/prisim_clean.h): the Hogbom CLEAN of prisim/delay_spectrum.py:complex1dClean
// (:133-352) on every (baseline, snapshot) row at once, and the delayClean chain around it (:1736-1815).
//
// Kernel shape: one wave64 per row, rows handed out by an atomic counter (iteration counts differ 30x between rows), no workgroup
// barrier after the prologue.  A row lives in LDS, permuted so that the clean box comes first: positions [0, nb) hold the in-box lags
// in increasing lag order, [nb, m) the others, perm[p] the lag of position p.  Per iteration:
//   argmax of |res| over the box (first lag on ties; index 0 when the box is all zero, as NP.argmax(abs(res * cbox)));
//   cc[ind] += gain res[ind]; res -= ccval roll(kernel, ind - kmaxind) (kernel normalised to max modulus 1, one copy per workgroup in
//   LDS when every row shares it);
//   inrms / outrms = median(|x - median(x)|) over the box / the rest: exact order statistics by a 2-bit-per-pass radix select on
//   order-preserving 64-bit keys, counted with ballots (at most 32 passes per 64-bit key, fewer once one candidate is left).  The complex median is numpy's: lexicographic
//   (real, then imaginary; the imaginary keys are only consulted on ties of the real part), mean of the two middle elements when the
//   count is even.
// fp64 throughout, built with -ffp-contract=off: the medians' means and x - median round as numpy's separate operations, and the
// AXPY's complex product as numpy's vector loop rounds it where the processor fuses (fma(ar, br, -(ai bi)), fma(ar, bi, ai br)), so
// residuals, and with them the two rms, follow the reference's fixtures to the last bits.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <string>
#include <vector>

#include "../csrc_addon/addon_internal.h"
#include "../../include/prisim_clean.h"

namespace {

constexpr int kWave = 64;
constexpr int kMaxWaves = 16;           // rows in flight per workgroup
constexpr int kCuLds = 160 * 1024;      // LDS per CU on MI355X

__device__ __forceinline__ void wave_sync() {
  // cross-lane hand-over through LDS inside one wave: keep the compiler from moving LDS accesses across phase boundaries
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ int wcount(bool p) { return __popcll(__ballot(p)); }

__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int m) {
  const unsigned lo = __shfl_xor((unsigned)(v & 0xffffffffu), m);
  const unsigned hi = __shfl_xor((unsigned)(v >> 32), m);
  return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ double shfl_xor_f64(double v, int m) {
  return __longlong_as_double((long long)shfl_xor_u64((uint64_t)__double_as_longlong(v), m));
}

// order-preserving key of a double (numpy's order: -0.0 == +0.0, so -0 is keyed as +0)
__device__ __forceinline__ uint64_t okey(double x) {
  const uint64_t u = (uint64_t)__double_as_longlong(x == 0.0 ? 0.0 : x);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

__device__ __forceinline__ double from_okey(uint64_t k) {
  const uint64_t u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double((long long)u);
}

// k-th smallest (0-based, k < #selected) of key(p) over the positions p0 + i, i < n, with sel(p); on return k is the rank of the
// result among the selected elements equal to it.  Wave-uniform n and k; at most 32 passes of 2 bits, and as soon as one element
// is left under the prefix, one more pass reads it (distinct doubles of one magnitude part after a few mantissa digits).
template <class Key, class Sel>
__device__ uint64_t radix_select(int p0, int n, int& k, Key key, Sel sel) {
  const int lane = threadIdx.x & (kWave - 1);
  uint64_t prefix = 0, hmask = 0;
  for (int b = 62; b >= 0; b -= 2) {
    int c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    for (int base = 0; base < n; base += kWave) {
      const int i = base + lane;
      bool ok = false;
      unsigned d = 0;
      if (i < n && sel(p0 + i)) {
        const uint64_t kk = key(p0 + i);
        ok = (kk & hmask) == prefix;
        d = (unsigned)(kk >> b) & 3u;
      }
      c0 += wcount(ok && d == 0);
      c1 += wcount(ok && d == 1);
      c2 += wcount(ok && d == 2);
      c3 += wcount(ok && d == 3);
    }
    uint64_t dsel;
    int left;
    if (k < c0) {
      dsel = 0; left = c0;
    } else if (k < c0 + c1) {
      dsel = 1; k -= c0; left = c1;
    } else if (k < c0 + c1 + c2) {
      dsel = 2; k -= c0 + c1; left = c2;
    } else {
      dsel = 3; k -= c0 + c1 + c2; left = c3;
    }
    prefix |= dsel << b;
    hmask |= 3ull << b;
    if (left == 1 && b > 0) {
      uint64_t v = 0;
      for (int base = 0; base < n; base += kWave) {
        const int i = base + lane;
        if (i < n && sel(p0 + i)) {
          const uint64_t kk = key(p0 + i);
          if ((kk & hmask) == prefix) v = kk;
        }
      }
      for (int o = 32; o >= 1; o >>= 1) v |= shfl_xor_u64(v, o);
      k = 0;
      return v;
    }
  }
  return prefix;
}

struct RowLds {
  double2* r;        // [m] the row, permuted
  uint64_t* sk;      // [m] keys of the current selection
  uint16_t* perm;    // [m] lag of every position
};

// numpy median of the complex values r[p0 .. p0+n) (n >= 1); leaves sk[p0 ..) holding the real keys
__device__ double2 cmedian(const RowLds& L, int p0, int n) {
  const int lane = threadIdx.x & (kWave - 1);
  for (int i = lane; i < n; i += kWave) L.sk[p0 + i] = okey(L.r[p0 + i].x);
  wave_sync();
  auto rkey = [&](int p) { return L.sk[p]; };
  auto all = [](int) { return true; };
  auto select = [&](int k, uint64_t& ik) -> uint64_t {
    int rank = k;
    const uint64_t rk = radix_select(p0, n, rank, rkey, all);
    int eq = 0;
    uint64_t im = 0;
    for (int base = 0; base < n; base += kWave) {
      const int i = base + lane;
      const bool e = i < n && L.sk[p0 + i] == rk;
      eq += wcount(e);
      if (e) im |= okey(L.r[p0 + i].y);
    }
    if (eq == 1) {
      for (int o = 32; o >= 1; o >>= 1) im |= shfl_xor_u64(im, o);
      ik = im;
    } else {
      ik = radix_select(p0, n, rank, [&](int p) { return okey(L.r[p].y); }, [&](int p) { return L.sk[p] == rk; });
    }
    return rk;
  };
  const int h = n / 2;
  uint64_t ilo;
  const uint64_t rlo = select((n & 1) ? h : h - 1, ilo);
  if (n & 1) return make_double2(from_okey(rlo), from_okey(ilo));
  // the next element in lexicographic order: rank h is lo itself when more than h elements are <= lo, else the least one above lo
  int le = 0;
  uint64_t ar = ~0ull, ai = ~0ull;
  for (int base = 0; base < n; base += kWave) {
    const int i = base + lane;
    bool l = false;
    if (i < n) {
      const uint64_t a = L.sk[p0 + i], b = okey(L.r[p0 + i].y);
      l = a < rlo || (a == rlo && b <= ilo);
      if (!l && (a < ar || (a == ar && b < ai))) { ar = a; ai = b; }
    }
    le += wcount(l);
  }
  for (int o = 32; o >= 1; o >>= 1) {
    const uint64_t orr = shfl_xor_u64(ar, o), oi = shfl_xor_u64(ai, o);
    if (orr < ar || (orr == ar && oi < ai)) { ar = orr; ai = oi; }
  }
  const double lor = from_okey(rlo), loi = from_okey(ilo);
  const double hir = le > h ? lor : from_okey(ar), hii = le > h ? loi : from_okey(ai);
  return make_double2((lor + hir) / 2.0, (loi + hii) / 2.0);
}

// numpy median of the non-negative doubles whose bits are sk[p0 .. p0+n)
__device__ double rmedian(const RowLds& L, int p0, int n) {
  const int lane = threadIdx.x & (kWave - 1);
  auto key = [&](int p) { return L.sk[p]; };
  auto all = [](int) { return true; };
  const int h = n / 2;
  int k = (n & 1) ? h : h - 1;
  const uint64_t lo = radix_select(p0, n, k, key, all);
  const double dlo = __longlong_as_double((long long)lo);
  if (n & 1) return dlo;
  int le = 0;
  uint64_t mn = ~0ull;
  for (int base = 0; base < n; base += kWave) {
    const int i = base + lane;
    bool l = false;
    if (i < n) {
      const uint64_t a = L.sk[p0 + i];
      l = a <= lo;
      if (!l && a < mn) mn = a;
    }
    le += wcount(l);
  }
  for (int o = 32; o >= 1; o >>= 1) {
    const uint64_t x = shfl_xor_u64(mn, o);
    if (x < mn) mn = x;
  }
  const double dhi = le > h ? dlo : __longlong_as_double((long long)mn);
  return (dlo + dhi) / 2.0;
}

// median(|x - median(x)|) over positions [p0, p0 + n); NaN for an empty set (numpy's median of nothing)
__device__ double mad(const RowLds& L, int p0, int n) {
  if (n == 0) return __longlong_as_double(0x7ff8000000000000ll);
  const int lane = threadIdx.x & (kWave - 1);
  const double2 med = cmedian(L, p0, n);
  wave_sync();
  for (int i = lane; i < n; i += kWave) {
    const double2 v = L.r[p0 + i];
    L.sk[p0 + i] = (uint64_t)__double_as_longlong(hypot(v.x - med.x, v.y - med.y));
  }
  wave_sync();
  return rmedian(L, p0, n);
}

struct CleanParams {
  const double2* inp;       // [nrows][m]
  int64_t nrows;
  int m;
  int row_mod;              // kidx / cbox row of CLEAN row r: r % row_mod
  const double2* knorm;     // [nkern][m] normalised kernels
  const int* kmax;          // [nkern]
  const int32_t* kidx;      // [row_mod] or null
  const uint8_t* cbox;      // [row_mod][m]
  double gain;
  int maxiter;
  double threshold;
  int thr_abs;
  int kern_in_lds;
  int wave_bytes;
  double2* cc;              // [nrows][m], zeroed by the caller
  double2* res;             // [nrows][m]
  int32_t* iters;
  int32_t* flags;
  double2* rms;             // [nrows] (inrms, outrms)
  unsigned long long* counter;
};

__device__ void clean_row(const CleanParams& P, const RowLds& L, const double2* kl, int64_t row) {
  const int lane = threadIdx.x & (kWave - 1);
  const int m = P.m;
  const int64_t brow = row % P.row_mod;
  const uint8_t* box = P.cbox + brow * m;
  const double2* in = P.inp + row * m;
  const int ki = P.kidx ? P.kidx[brow] : 0;
  const double2* kg = P.kern_in_lds ? kl : P.knorm + (int64_t)ki * m;
  const int kmaxind = P.kmax[ki];
  const uint64_t lt = (1ull << lane) - 1ull;

  // stable partition: the box first
  int nb = 0;
  for (int base = 0; base < m; base += kWave) {
    const int j = base + lane;
    const bool b = j < m && box[j] != 0;
    const uint64_t bal = __ballot(b);
    if (b) L.perm[nb + __popcll(bal & lt)] = (uint16_t)j;
    nb += __popcll(bal);
  }
  int no = nb;
  for (int base = 0; base < m; base += kWave) {
    const int j = base + lane;
    const bool b = j < m && box[j] == 0;
    const uint64_t bal = __ballot(b);
    if (b) L.perm[no + __popcll(bal & lt)] = (uint16_t)j;
    no += __popcll(bal);
  }
  wave_sync();
  double mx = 0.0;
  int pos0 = -1;
  for (int p = lane; p < m; p += kWave) {
    const int j = L.perm[p];
    const double2 v = in[j];
    L.r[p] = v;
    mx = fmax(mx, hypot(v.x, v.y));
    if (j == 0) pos0 = p;
  }
  for (int o = 32; o >= 1; o >>= 1) {
    mx = fmax(mx, shfl_xor_f64(mx, o));
    pos0 = max(pos0, __shfl_xor(pos0, o));
  }
  wave_sync();
  double2* cc = P.cc + row * m;
  double2* res = P.res + row * m;
  const double lolim = P.thr_abs ? P.threshold / mx : P.threshold;       // :212-215
  if (lolim >= 1.0) {                                                      // :216-217: the host raises the reference's ValueError
    for (int j = lane; j < m; j += kWave) res[j] = in[j];
    if (lane == 0) {
      P.iters[row] = 0;
      P.flags[row] = PRISIM_CLEAN_BAD_THRESHOLD;
      const double nan = __longlong_as_double(0x7ff8000000000000ll);
      P.rms[row] = make_double2(nan, nan);
    }
    wave_sync();           // as the other exit: lane 0's stores above and the next hand-out's lane-0 atomic must not merge into one branch
    return;
  }
  const double bound = lolim * mx;
  const int nout = m - nb;
  const bool have_out = nout > 2;
  int itr = 0;
  bool c1 = false, c2 = false, c3 = false;
  double inr = 0.0, outr = __longlong_as_double(0x7ff8000000000000ll);
  for (;;) {
    ++itr;
    double bv = -1.0;
    int bj = INT_MAX;
    double2 bx = make_double2(0.0, 0.0);
    for (int p = lane; p < nb; p += kWave) {
      const double2 v = L.r[p];
      const double a = hypot(v.x, v.y);
      if (a > bv) { bv = a; bj = L.perm[p]; bx = v; }
    }
    for (int o = 32; o >= 1; o >>= 1) {
      const double ov = shfl_xor_f64(bv, o);
      const int oj = __shfl_xor(bj, o);
      const double ox = shfl_xor_f64(bx.x, o), oy = shfl_xor_f64(bx.y, o);
      if (ov > bv || (ov == bv && oj < bj)) { bv = ov; bj = oj; bx = make_double2(ox, oy); }
    }
    int ind;
    double2 mr;
    if (bv > 0.0) {
      ind = bj; mr = bx;
    } else {                 // every searched entry is zero: NP.argmax of all zeros is 0
      ind = 0; mr = L.r[pos0];
    }
    const double2 cv = make_double2(P.gain * mr.x, P.gain * mr.y);
    if (lane == 0) {
      double2 c = cc[ind];
      cc[ind] = make_double2(c.x + cv.x, c.y + cv.y);
    }
    const int s = ind - kmaxind;                                           // roll(kernel, ind - kmaxind)
    for (int p = lane; p < m; p += kWave) {
      int kj = (int)L.perm[p] - s;
      kj = kj < 0 ? kj + m : (kj >= m ? kj - m : kj);
      const double2 k = kg[kj];
      const double2 v = L.r[p];
      const double tr = fma(cv.x, k.x, -(cv.y * k.y));                  // numpy's complex product on a processor with fused
      const double ti = fma(cv.x, k.y, cv.y * k.x);                     // multiply-add: one product rounded, the other fused into the sum
      L.r[p] = make_double2(v.x - tr, v.y - ti);
    }
    wave_sync();
    c1 = hypot(mr.x, mr.y) <= bound;
    c2 = itr >= P.maxiter;
    if (have_out) {
      inr = mad(L, 0, nb);
      wave_sync();
      outr = mad(L, nb, nout);
      wave_sync();
      c3 = inr <= outr;
    }
    if (c1 || c2 || c3) break;
  }
  if (!have_out) inr = mad(L, 0, nb);
  for (int p = lane; p < m; p += kWave) res[L.perm[p]] = L.r[p];
  if (lane == 0) {
    P.iters[row] = itr;
    P.flags[row] = (c1 ? PRISIM_CLEAN_THRESHOLD : 0) | (c2 ? PRISIM_CLEAN_MAXITER : 0) | (c3 ? PRISIM_CLEAN_INRMS : 0) |
                   (have_out ? 0 : PRISIM_CLEAN_NO_OUTRMS);
    P.rms[row] = make_double2(inr, outr);
  }
  wave_sync();
}

__global__ void __launch_bounds__(kWave * kMaxWaves) k_clean_rows(CleanParams P) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  const int m = P.m;
  double2* kl = nullptr;
  size_t off = 0;
  if (P.kern_in_lds) {
    kl = reinterpret_cast<double2*>(smem);
    for (int j = threadIdx.x; j < m; j += blockDim.x) kl[j] = P.knorm[j];
    off = (size_t)m * 16;
  }
  __syncthreads();
  unsigned char* w = smem + off + (size_t)wv * P.wave_bytes;
  RowLds L;
  L.r = reinterpret_cast<double2*>(w);
  L.sk = reinterpret_cast<uint64_t*>(w + (size_t)m * 16);
  L.perm = reinterpret_cast<uint16_t*>(w + (size_t)m * 24);
  for (;;) {
    // The whole wave meets here before lane 0 draws a row: the shuffle below reads lane 0.  Without a convergent operation between a
    // lane-0-only tail of clean_row and this lane-0-only atomic the compiler threads lane 0 from one to the other and sends the other
    // lanes straight back to the shuffle, where they read row 0 for ever (a row rejected for its threshold hung the wave).
    wave_sync();
    unsigned long long row = 0;
    if (lane == 0) row = atomicAdd(P.counter, 1ull);
    row = ((unsigned long long)(unsigned)__shfl((int)(row >> 32), 0) << 32) | (unsigned)__shfl((int)(row & 0xffffffffu), 0);
    if (row >= (unsigned long long)P.nrows) break;
    clean_row(P, L, kl, (int64_t)row);
  }
}

// |z| rounded correctly (but for a true value within 2^-100 of a midpoint): hypot is within an ulp, and the residual x^2 + y^2 - h^2,
// formed without rounding error by fused products, says which neighbour is nearer.  Every normalised tap inherits the peak's modulus,
// so its last bit is worth this once per kernel; values whose squares leave the double range keep hypot's answer.
__device__ __forceinline__ double modulus_rounded(double x, double y) {
  const double h = hypot(x, y);
  const double xx = x * x, yy = y * y, hh = h * h;
  if (!(h > 0x1p-500 && h < 0x1p500)) return h;
  const double ex = fma(x, x, -xx), ey = fma(y, y, -yy), eh = fma(h, h, -hh);
  const double big = fmax(xx, yy), small = fmin(xx, yy);
  const double d = big - hh;                       // exact: hh is within a factor 2 of big
  const double t = d + small;
  const double et = (d - (t - (t - d))) + (small - (t - d));   // two-sum error of d + small
  const double r = t + (et + ((ex + ey) - eh));
  return h + r / (2.0 * h);
}

// kernel /= max|kernel| as numpy divides a complex array by a float (Smith's branch with a zero imaginary part), then the first argmax
__global__ void __launch_bounds__(kWave) k_clean_norm(const double2* kin, double2* kout, int* kmax, int m) {
  const int lane = threadIdx.x;
  const double2* k = kin + (int64_t)blockIdx.x * m;
  double2* o = kout + (int64_t)blockIdx.x * m;
  double mx = 0.0;
  for (int j = lane; j < m; j += kWave) mx = fmax(mx, modulus_rounded(k[j].x, k[j].y));
  for (int s = 32; s >= 1; s >>= 1) mx = fmax(mx, shfl_xor_f64(mx, s));
  const double rat = 0.0 / mx;
  const double scl = 1.0 / (mx + 0.0 * rat);
  double bv = -1.0;
  int bj = INT_MAX;
  for (int j = lane; j < m; j += kWave) {
    const double2 v = k[j];
    const double2 q = make_double2((v.x + v.y * rat) * scl, (v.y - v.x * rat) * scl);
    o[j] = q;
    const double a = hypot(q.x, q.y);
    if (a > bv) { bv = a; bj = j; }
  }
  for (int s = 32; s >= 1; s >>= 1) {
    const double ov = shfl_xor_f64(bv, s);
    const int oj = __shfl_xor(bj, s);
    if (ov > bv || (ov == bv && oj < bj)) { bv = ov; bj = oj; }
  }
  if (lane == 0) kmax[blockIdx.x] = bj < m ? bj : 0;       // (no finite modulus at all: lag 0, never an index past the row)
}

// x = (x * s1) * s2 (s2 == 1: one product), complex times real as numpy: both parts scaled
__global__ void k_clean_scale(double2* x, int64_t n, double s1, double s2, int two) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    double2 v = x[i];
    v.x = v.x * s1; v.y = v.y * s1;
    if (two) { v.x = v.x * s2; v.y = v.y * s2; }
    x[i] = v;
  }
}

// ---- host side --------------------------------------------------------------------------------------------------------------

int check_common(prisim_ctx* ctx, int64_t nrows, int64_t m, int64_t nkern, const int32_t* kidx, int64_t nkidx, double gain,
                 int64_t maxiter, double threshold) {
  if (m < 1 || m > PRISIM_CLEAN_MAX_LEN)
    return fail(ctx, PRISIM_EINVAL, "delay CLEAN takes rows of 1 to " + std::to_string(PRISIM_CLEAN_MAX_LEN) +
                                        " lags (PRISIM_CLEAN_MAX_LEN); got " + std::to_string(m));
  if (nrows < 0 || nkern < 1) return fail(ctx, PRISIM_EINVAL, "nrows must be >= 0 and nkern >= 1");
  if (nkern > 1 && !kidx) return fail(ctx, PRISIM_EINVAL, "kidx is required when nkern > 1");
  if (kidx)
    for (int64_t i = 0; i < nkidx; ++i)
      if (kidx[i] < 0 || kidx[i] >= nkern) return fail(ctx, PRISIM_EINVAL, "kidx entry out of range");
  if (!(gain > 0.0 && gain < 1.0)) return fail(ctx, PRISIM_EINVAL, "gain must lie between 0 and 1");
  if (maxiter < 1) return fail(ctx, PRISIM_EINVAL, "maxiter must be positive");
  if (!(threshold > 0.0)) return fail(ctx, PRISIM_EINVAL, "input threshold must be positive");
  return PRISIM_OK;
}

// normalise the kernels, size the launch and CLEAN `nrows` rows already on the device
int run_clean(prisim_ctx* ctx, Dev& dev, const double2* d_inp, int64_t nrows, int m, int64_t row_mod, const double2* d_kern,
              int64_t nkern, const int32_t* d_kidx, const uint8_t* d_cbox, double gain, int64_t maxiter, double threshold, int thr_abs,
              double2* d_cc, double2* d_res, int32_t* d_iters, int32_t* d_flags, double2* d_rms, prisim_clean_stats* st,
              hipEvent_t e0, hipEvent_t e1) {
  double2* knorm;
  int* kmax;
  unsigned long long* counter;
  DEV_ALLOC(ctx, dev, knorm, (size_t)nkern * m * 16);
  DEV_ALLOC(ctx, dev, kmax, (size_t)nkern * sizeof(int));
  DEV_ALLOC(ctx, dev, counter, sizeof(unsigned long long));
  HIPCHK(ctx, hipMemsetAsync(counter, 0, sizeof(unsigned long long), ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(d_cc, 0, (size_t)nrows * m * 16, ctx->stream));
  hipLaunchKernelGGL(k_clean_norm, dim3((unsigned)nkern), dim3(kWave), 0, ctx->stream, d_kern, knorm, kmax, m);
  HIPCHK(ctx, hipGetLastError());

  int lds_max = 0;
  if (int rc = lds_limit(ctx, lds_max)) return rc;
  const int wave_bytes = (26 * m + 15) / 16 * 16;          // r (16 B), sk (8 B), perm (2 B) per lag; every row 16-B aligned
  const int kern_bytes = 16 * m;
  const bool kern_lds = nkern == 1 && kern_bytes + wave_bytes <= lds_max;
  const int avail = lds_max - (kern_lds ? kern_bytes : 0);
  int waves = std::min(kMaxWaves, avail / wave_bytes);
  if (waves < 1)
    return fail(ctx, PRISIM_EINVAL, "a CLEAN row of " + std::to_string(m) + " lags needs " + std::to_string(wave_bytes) +
                                        " B of LDS; the device offers " + std::to_string(lds_max) + " B per workgroup");
  waves = (int)std::max<int64_t>(1, std::min<int64_t>(waves, (nrows + ctx->cu_count - 1) / std::max(1, ctx->cu_count)));
  const size_t lds = (size_t)(kern_lds ? kern_bytes : 0) + (size_t)waves * wave_bytes;
  if (int rc = allow_lds(ctx, k_clean_rows, (int64_t)lds)) return rc;
  const int64_t per_cu = std::max<int64_t>(1, kCuLds / (int64_t)lds);
  const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>((nrows + waves - 1) / waves, (int64_t)ctx->cu_count * per_cu));

  CleanParams P;
  P.inp = d_inp; P.nrows = nrows; P.m = m; P.row_mod = (int)row_mod;
  P.knorm = knorm; P.kmax = kmax; P.kidx = d_kidx; P.cbox = d_cbox;
  P.gain = gain; P.maxiter = (int)std::min<int64_t>(maxiter, INT_MAX); P.threshold = threshold; P.thr_abs = thr_abs;
  P.kern_in_lds = kern_lds ? 1 : 0; P.wave_bytes = wave_bytes;
  P.cc = d_cc; P.res = d_res; P.iters = d_iters; P.flags = d_flags; P.rms = d_rms; P.counter = counter;
  HIPCHK(ctx, hipEventRecord(e0, ctx->stream));
  if (nrows > 0) {
    hipLaunchKernelGGL(k_clean_rows, dim3((unsigned)blocks), dim3(kWave * waves), lds, ctx->stream, P);
    HIPCHK(ctx, hipGetLastError());
  }
  HIPCHK(ctx, hipEventRecord(e1, ctx->stream));
  if (st) {
    st->rows = nrows;
    st->waves_per_block = waves;
    st->kernel_in_lds = kern_lds ? 1 : 0;
    st->lds_bytes = (int64_t)lds;
  }
  return PRISIM_OK;
}

int finish_stats(prisim_ctx* ctx, const Events& ev, const int32_t* iters, int64_t n, prisim_clean_stats* st) {
  if (!st) return PRISIM_OK;
  float ms = 0.0f, cms = 0.0f;
  HIPCHK(ctx, hipEventElapsedTime(&ms, ev.e[0], ev.e[3]));
  HIPCHK(ctx, hipEventElapsedTime(&cms, ev.e[1], ev.e[2]));
  st->device_ms = ms;
  st->clean_ms = cms;
  int64_t s = 0;
  for (int64_t i = 0; i < n; ++i) s += iters[i];
  st->sum_iter = s;
  return PRISIM_OK;
}

}  // namespace

extern "C" {

int prisim_clean_rows(prisim_ctx* ctx, int64_t nrows, int64_t m, const double* inp, int64_t nkern, const double* kern,
                      const int32_t* kidx, const uint8_t* cbox, double gain, int64_t maxiter, double threshold,
                      int32_t threshold_absolute, double* cc, double* res, int32_t* iters, int32_t* flags, double* rms,
                      prisim_clean_stats* stats) {
  return guarded(ctx, [&]() -> int {
  if (!ctx) return PRISIM_EINVAL;
  int rc;
  if ((rc = check_common(ctx, nrows, m, nkern, kidx, nrows, gain, maxiter, threshold))) return rc;
  if (nrows > 0 && (!inp || !kern || !cbox || !cc || !res || !iters || !flags || !rms)) return fail(ctx, PRISIM_EINVAL, "null array");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  Dev dev;
  Events ev;
  if ((rc = ev.create(ctx))) return rc;
  const size_t rb = (size_t)nrows * m * 16;
  double2 *d_inp, *d_kern, *d_cc, *d_res, *d_rms;
  int32_t *d_kidx = nullptr, *d_iters, *d_flags;
  uint8_t* d_cbox;
  DEV_ALLOC(ctx, dev, d_inp, rb);
  DEV_ALLOC(ctx, dev, d_kern, (size_t)nkern * m * 16);
  DEV_ALLOC(ctx, dev, d_cc, rb);
  DEV_ALLOC(ctx, dev, d_res, rb);
  DEV_ALLOC(ctx, dev, d_rms, (size_t)nrows * 16);
  DEV_ALLOC(ctx, dev, d_iters, (size_t)nrows * 4);
  DEV_ALLOC(ctx, dev, d_flags, (size_t)nrows * 4);
  DEV_ALLOC(ctx, dev, d_cbox, (size_t)nrows * m);
  if (kidx) DEV_ALLOC(ctx, dev, d_kidx, (size_t)nrows * 4);
  HIPCHK(ctx, hipEventRecord(ev.e[0], ctx->stream));
  if (nrows > 0) {
    HIPCHK(ctx, hipMemcpyAsync(d_inp, inp, rb, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(d_cbox, cbox, (size_t)nrows * m, hipMemcpyHostToDevice, ctx->stream));
    if (kidx) HIPCHK(ctx, hipMemcpyAsync(d_kidx, kidx, (size_t)nrows * 4, hipMemcpyHostToDevice, ctx->stream));
  }
  HIPCHK(ctx, hipMemcpyAsync(d_kern, kern, (size_t)nkern * m * 16, hipMemcpyHostToDevice, ctx->stream));
  if ((rc = run_clean(ctx, dev, d_inp, nrows, (int)m, std::max<int64_t>(nrows, 1), d_kern, nkern, d_kidx, d_cbox, gain, maxiter,
                      threshold, threshold_absolute ? 1 : 0, d_cc, d_res, d_iters, d_flags, d_rms, stats, ev.e[1], ev.e[2])))
    return rc;
  if (nrows > 0) {
    HIPCHK(ctx, hipMemcpyAsync(cc, d_cc, rb, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(res, d_res, rb, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(iters, d_iters, (size_t)nrows * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(flags, d_flags, (size_t)nrows * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(rms, d_rms, (size_t)nrows * 16, hipMemcpyDeviceToHost, ctx->stream));
  }
  HIPCHK(ctx, hipEventRecord(ev.e[3], ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return finish_stats(ctx, ev, iters, nrows, stats);
  });
}

int prisim_clean_delay(prisim_ctx* ctx, int32_t ncubes, int64_t nrows, int64_t nchan, int64_t m, const double* win, int64_t nkern,
                       const double* kwin, const int32_t* kidx, const uint8_t* cbox, double lag_scale, double freq_scale1,
                       double freq_scale2, double gain, int64_t maxiter, double threshold, int32_t threshold_absolute, double* lag,
                       double* kern_lag, double* cc, double* res, double* cc_freq, double* res_freq, int32_t* iters, int32_t* flags,
                       double* rms, prisim_clean_stats* stats) {
  return guarded(ctx, [&]() -> int {
  if (!ctx) return PRISIM_EINVAL;
  int rc;
  if ((rc = check_common(ctx, nrows, m, nkern, kidx, nrows, gain, maxiter, threshold))) return rc;
  if (ncubes < 1 || nchan < 1 || nchan > m) return fail(ctx, PRISIM_EINVAL, "ncubes must be >= 1 and 1 <= nchan <= m");
  if (!win || !kwin || !cbox || !lag || !kern_lag || !cc || !res || !cc_freq || !res_freq || !iters || !flags || !rms)
    return fail(ctx, PRISIM_EINVAL, "null array");
  if ((rc = ensure_rocfft(ctx))) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  Work wk;
  Dev& dev = wk.dev;
  Events ev;
  if ((rc = ev.create(ctx))) return rc;
  const int64_t nclean = (int64_t)ncubes * nrows, nall = nclean + nkern;
  const size_t rb = (size_t)nclean * m * 16;
  double2 *d_x, *d_cc, *d_res, *d_ccf, *d_resf, *d_rms;
  int32_t *d_kidx = nullptr, *d_iters, *d_flags;
  uint8_t* d_cbox;
  DEV_ALLOC(ctx, dev, d_x, (size_t)nall * m * 16);
  DEV_ALLOC(ctx, dev, d_cc, rb);
  DEV_ALLOC(ctx, dev, d_res, rb);
  DEV_ALLOC(ctx, dev, d_ccf, rb);
  DEV_ALLOC(ctx, dev, d_resf, rb);
  DEV_ALLOC(ctx, dev, d_rms, (size_t)nclean * 16);
  DEV_ALLOC(ctx, dev, d_iters, (size_t)nclean * 4);
  DEV_ALLOC(ctx, dev, d_flags, (size_t)nclean * 4);
  DEV_ALLOC(ctx, dev, d_cbox, (size_t)std::max<int64_t>(nrows, 1) * m);
  if (kidx) DEV_ALLOC(ctx, dev, d_kidx, (size_t)std::max<int64_t>(nrows, 1) * 4);
  std::vector<std::pair<bool, size_t>> plans = {{true, (size_t)nall}};            // the inverse of every row; forward of the CLEANed ones
  if (nclean > 0) plans.push_back({false, (size_t)nclean});
  if ((rc = wk.fft.create(ctx, dev, (size_t)m, plans, &ctx->stream, 1))) return rc;

  HIPCHK(ctx, hipEventRecord(ev.e[0], ctx->stream));
  // zero-padded rows (:1738-1740): the windowed channels first, m - nchan zeros after them
  HIPCHK(ctx, hipMemsetAsync(d_x, 0, (size_t)nall * m * 16, ctx->stream));
  if (nclean > 0)
    HIPCHK(ctx, hipMemcpy2DAsync(d_x, (size_t)m * 16, win, (size_t)nchan * 16, (size_t)nchan * 16, (size_t)nclean,
                                 hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpy2DAsync(d_x + nclean * m, (size_t)m * 16, kwin, (size_t)nchan * 16, (size_t)nchan * 16, (size_t)nkern,
                               hipMemcpyHostToDevice, ctx->stream));
  if (nrows > 0) {
    HIPCHK(ctx, hipMemcpyAsync(d_cbox, cbox, (size_t)nrows * m, hipMemcpyHostToDevice, ctx->stream));
    if (kidx) HIPCHK(ctx, hipMemcpyAsync(d_kidx, kidx, (size_t)nrows * 4, hipMemcpyHostToDevice, ctx->stream));
  }
  if ((rc = wk.fft.run(ctx, true, (size_t)nall, d_x, 0))) return rc;
  // rocFFT's inverse is unnormalised: m df ifft(x) = df * sum_n x[n] e^{+2 pi i k n / m}
  hipLaunchKernelGGL(k_clean_scale, dim3(1024), dim3(256), 0, ctx->stream, d_x, nall * m, lag_scale, 1.0, 0);
  HIPCHK(ctx, hipGetLastError());
  if ((rc = run_clean(ctx, dev, d_x, nclean, (int)m, std::max<int64_t>(nrows, 1), d_x + nclean * m, nkern, d_kidx, d_cbox, gain,
                      maxiter, threshold, threshold_absolute ? 1 : 0, d_cc, d_res, d_iters, d_flags, d_rms, stats, ev.e[1], ev.e[2])))
    return rc;
  if (nclean > 0) {
    // NP.fft.fft(.) * deta * pad_factor (:1808-1811)
    HIPCHK(ctx, hipMemcpyAsync(d_ccf, d_cc, rb, hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(d_resf, d_res, rb, hipMemcpyDeviceToDevice, ctx->stream));
    if ((rc = wk.fft.run(ctx, false, (size_t)nclean, d_ccf, 0)) || (rc = wk.fft.run(ctx, false, (size_t)nclean, d_resf, 0))) return rc;
    hipLaunchKernelGGL(k_clean_scale, dim3(1024), dim3(256), 0, ctx->stream, d_ccf, nclean * m, freq_scale1, freq_scale2, 1);
    hipLaunchKernelGGL(k_clean_scale, dim3(1024), dim3(256), 0, ctx->stream, d_resf, nclean * m, freq_scale1, freq_scale2, 1);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(lag, d_x, rb, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(cc, d_cc, rb, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(res, d_res, rb, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(cc_freq, d_ccf, rb, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(res_freq, d_resf, rb, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(iters, d_iters, (size_t)nclean * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(flags, d_flags, (size_t)nclean * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(rms, d_rms, (size_t)nclean * 16, hipMemcpyDeviceToHost, ctx->stream));
  }
  HIPCHK(ctx, hipMemcpyAsync(kern_lag, d_x + nclean * m, (size_t)nkern * m * 16, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipEventRecord(ev.e[3], ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return finish_stats(ctx, ev, iters, nclean, stats);
  });
}

}  // extern "C"
