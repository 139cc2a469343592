// gains.hip -- instrument gain tables for gfx950 (include/prisim_gains.h): the evaluation behind prisim/interferometry.py:GainInfo
// (spline_gains :3382-3597, nearest_gains :3599-3723) and the product of InterferometerArray.add_noise (:6697-6722),
// vis = gains * skyvis + noise, with the gain of baseline (A2, A1) conj(g[A1]) g[A2] g_bl.
//
// Evaluation: k_basis finds, for every spline and every time / channel, the knot span and the kx + 1 (ky + 1) non-zero B-splines with
// FITPACK's fpbspl recursion; k_eval sums the (kx + 1)(ky + 1) coefficients of both splines of a row per (t, row, f) in fpbisp's order
// and writes the table [nt][nrows][nchan].  Gather: the nearest-neighbour table from host index maps.
// Apply: one pass over the cube [nt][nbl][nchan], streamed in chunks of whole snapshots; per element the sky, the noise and the output
// move (48 B of the algorithm) plus the table rows of the factors, which many baselines share (whether the caches serve them has not
// been measured).  No gain cube is formed.
// fp64 throughout, built with -ffp-contract=off (the products round as numpy's).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "../csrc_addon/addon_internal.h"
#include "../../include/prisim_gains.h"

struct prisim_gains_table {
  prisim_ctx* ctx = nullptr;   // compared against, never dereferenced by prisim_gains_table_free
  int device = 0;
  int64_t nt = 0, nrows = 0, nchan = 0;
  double2* d = nullptr;       // [nt][nrows][nchan]
};

namespace {

using pint::fail;
using pint::guarded;

constexpr int kMaxK = PRISIM_GAINS_MAX_DEGREE;
constexpr int kW = kMaxK + 1;                 // B-spline weights stored per point
constexpr size_t kApplyChunkBytes = size_t(512) << 20;   // device bytes per streamed cube (sky, noise, output) of one apply chunk

__device__ __forceinline__ double2 cconj(double2 a) { return make_double2(a.x, -a.y); }

int fill_stats(prisim_ctx* ctx, Events& ev, int64_t elements, prisim_gains_stats* stats) {
  if (!stats) return PRISIM_OK;
  float ms = 0.0f, kms = 0.0f;
  HIPCHK(ctx, hipEventElapsedTime(&ms, ev.e[0], ev.e[3]));
  HIPCHK(ctx, hipEventElapsedTime(&kms, ev.e[1], ev.e[2]));
  stats->device_ms = ms;
  stats->kernel_ms = kms;
  stats->elements = elements;
  return PRISIM_OK;
}

// FITPACK fpbspl: the k + 1 non-zero B-splines of degree k at x, t[l] <= x < t[l + 1] (l 0-based)
__device__ void fpbspl(const double* t, int k, double x, int64_t l, double* h) {
  double hh[kMaxK];
  h[0] = 1.0;
  for (int j = 1; j <= k; ++j) {
    for (int i = 0; i < j; ++i) hh[i] = h[i];
    h[0] = 0.0;
    for (int i = 1; i <= j; ++i) {
      const int64_t li = l + i, lj = li - j;
      if (t[li] == t[lj]) {
        h[i] = 0.0;
        continue;
      }
      const double f = hh[i - 1] / (t[li] - t[lj]);
      h[i - 1] = h[i - 1] + f * (t[li] - x);
      h[i] = f * (x - t[lj]);
    }
  }
}

struct BasisParams {
  const int64_t* n;         // [nspl] knot counts of this axis
  const int64_t* off;       // [nspl] knot offsets of this axis
  const double* knots;
  int k;
  const double* pts;        // [npts]
  int64_t npts, nspl;
  int32_t* span;            // [nspl][npts] first coefficient index along this axis
  double* w;                // [nspl][npts][kW]
};

// one thread per (spline, point): fpbisp's span search (clamped to [t[k], t[n - k - 1]]) and the weights
__global__ void __launch_bounds__(kThreads) k_basis(BasisParams P) {
  const int64_t total = P.nspl * P.npts;
  for (int64_t i = blockIdx.x * (int64_t)kThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kThreads) {
    const int64_t s = i / P.npts, p = i - s * P.npts;
    const double* t = P.knots + P.off[s];
    const int64_t n = P.n[s];
    const int k = P.k;
    const double tb = t[k], te = t[n - k - 1];
    double arg = P.pts[p];
    if (arg < tb) arg = tb;
    if (arg > te) arg = te;
    int64_t l = k;
    while (!(arg < t[l + 1] || l == n - k - 2)) ++l;
    double h[kW];
    for (int j = 0; j < kW; ++j) h[j] = 0.0;
    fpbspl(t, k, arg, l, h);
    P.span[i] = (int32_t)(l - k);
    for (int j = 0; j < kW; ++j) P.w[i * kW + j] = h[j];
  }
}

struct EvalParams {
  const int64_t* ny;        // [nspl]
  const int64_t* c_off;     // [nspl]
  const double* coefs;
  int kx, ky;
  int64_t nt, nrows, nchan;
  const int32_t* sx;        // [nspl][nt]
  const double* wx;         // [nspl][nt][kW]
  const int32_t* sy;        // [nspl][nchan]
  const double* wy;         // [nspl][nchan][kW]
  double2* out;             // [nt][nrows][nchan]
  int64_t nchunk;           // channel chunks of kThreads per row
};

__device__ __forceinline__ double eval_one(const EvalParams& P, int64_t s, int64_t t, int64_t f) {
  const int64_t ncy = P.ny[s] - P.ky - 1;
  const double* c = P.coefs + P.c_off[s];
  const int64_t lx = P.sx[s * P.nt + t], ly = P.sy[s * P.nchan + f];
  const double* hx = P.wx + (s * P.nt + t) * kW;
  const double* hy = P.wy + (s * P.nchan + f) * kW;
  double sp = 0.0;
  int64_t l1 = lx * ncy + ly;
  for (int i1 = 0; i1 <= P.kx; ++i1) {          // fpbisp: sp = sp + c(l2) * h(i1) * wy(j, j1), left to right
    const double h = hx[i1];
    for (int j1 = 0; j1 <= P.ky; ++j1) sp = sp + c[l1 + j1] * h * hy[j1];
    l1 += ncy;
  }
  return sp;
}

// one workgroup per (t, row, channel chunk)
__global__ void __launch_bounds__(kThreads) k_eval(EvalParams P) {
  const int64_t nwork = P.nt * P.nrows * P.nchunk;
  for (int64_t wi = blockIdx.x; wi < nwork; wi += gridDim.x) {
    const int64_t line = wi / P.nchunk, chunk = wi - line * P.nchunk;
    const int64_t f = chunk * kThreads + threadIdx.x;
    if (f >= P.nchan) continue;
    const int64_t t = line / P.nrows, r = line - t * P.nrows;
    P.out[line * P.nchan + f] = make_double2(eval_one(P, 2 * r, t, f), eval_one(P, 2 * r + 1, t, f));
  }
}

// nearest-neighbour table: out[t][r][f] = g[r][fi[f]][ti[t]]
__global__ void __launch_bounds__(kThreads) k_gather(const double2* g, int64_t nrows, int64_t ngf, int64_t ngt, const int64_t* fi,
                                                     const int64_t* ti, int64_t nt, int64_t nchan, double2* out) {
  const int64_t total = nt * nrows * nchan;
  for (int64_t i = blockIdx.x * (int64_t)kThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kThreads) {
    const int64_t f = i % nchan, line = i / nchan;
    const int64_t t = line / nrows, r = line - t * nrows;
    out[i] = g[(r * ngf + fi[f]) * ngt + ti[t]];
  }
}

struct Factor {
  const double2* d = nullptr;   // table [tnt][nrows][tnf]; nullptr: absent
  int64_t nrows = 0, tnt = 1, tnf = 1;
  int mode = PRISIM_GAINS_ANTENNA;
  const int64_t* a = nullptr;   // [nbl]
  const int64_t* c = nullptr;   // [nbl]
};

// t: snapshot of the whole call (the table's time index when it has more than one)
__device__ __forceinline__ double2 factor(const Factor& F, int64_t t, int64_t b, int64_t f) {
  const int64_t tt = F.tnt == 1 ? 0 : t, ff = F.tnf == 1 ? 0 : f;
  const double2* base = F.d + tt * F.nrows * F.tnf + ff;
  const int64_t a = F.a[b], c = F.c[b];
  if (a < 0) return make_double2(1.0, 0.0);           // a row without gains (padding rows of a shard)
  if (F.mode == PRISIM_GAINS_ANTENNA) return cmul(cconj(base[a * F.tnf]), base[c * F.tnf]);
  const double2 g = base[a * F.tnf];
  return c ? cconj(g) : g;
}

struct ApplyParams {
  Factor fa, fb;
  const double2* sky;           // [nt][nbl][nchan]
  const double2* noise;         // [nt][nbl][nchan] or nullptr
  double2* out;
  int64_t nt, nbl, nchan, nchunk;
  int64_t t_base;               // snapshot of the whole call at t = 0 of this launch (launches stream over snapshot chunks)
  int sky_c64, want_gain;
};

// one workgroup per (t, b, channel chunk): the sky, noise and output rows stream coalesced along the channels
__global__ void __launch_bounds__(kThreads) k_apply(ApplyParams P) {
  const int64_t nwork = P.nt * P.nbl * P.nchunk;
  for (int64_t wi = blockIdx.x; wi < nwork; wi += gridDim.x) {
    const int64_t line = wi / P.nchunk, chunk = wi - line * P.nchunk;
    const int64_t f = chunk * kThreads + threadIdx.x;
    if (f >= P.nchan) continue;
    const int64_t t = line / P.nbl, b = line - t * P.nbl;
    double2 g = make_double2(1.0, 0.0);
    const int64_t tg = t + P.t_base;
    if (P.fa.d && P.fb.d) g = cmul(factor(P.fa, tg, b, f), factor(P.fb, tg, b, f));
    else if (P.fa.d) g = factor(P.fa, tg, b, f);
    else if (P.fb.d) g = factor(P.fb, tg, b, f);
    const int64_t e = line * P.nchan + f;
    if (P.want_gain) {
      P.out[e] = g;
      continue;
    }
    double2 s = P.sky[e];
    if (P.sky_c64) s = make_double2((double)(float)s.x, (double)(float)s.y);
    double2 v = cmul(g, s);
    if (P.noise) {
      const double2 n = P.noise[e];
      v = make_double2(v.x + n.x, v.y + n.y);
    }
    P.out[e] = v;
  }
}

int64_t blocks_for(prisim_ctx* ctx, int64_t work) {
  return std::max<int64_t>(1, std::min<int64_t>(work, std::max<int64_t>((int64_t)std::max(ctx->cu_count, 1) * 32, 1024)));
}

int new_table(prisim_ctx* ctx, int64_t nt, int64_t nrows, int64_t nchan, prisim_gains_table** out) {
  auto* tab = new prisim_gains_table;
  tab->ctx = ctx;
  tab->device = ctx->device;
  tab->nt = nt;
  tab->nrows = nrows;
  tab->nchan = nchan;
  const size_t bytes = std::max<size_t>((size_t)nt * nrows * nchan * sizeof(double2), 16);
  const hipError_t e = hipMalloc(&tab->d, bytes);
  if (e != hipSuccess) {
    delete tab;
    return fail(ctx, PRISIM_ENOMEM, std::string("hipMalloc(") + std::to_string(bytes) + " B) for a gain table: " + hipGetErrorString(e));
  }
  *out = tab;
  return PRISIM_OK;
}

bool factor_ok(const prisim_gains_table* tab, int32_t mode, const int64_t* a, const int64_t* c, int64_t nt, int64_t nchan, int64_t nbl,
               prisim_ctx* ctx, std::string& why) {
  if (!tab) return true;
  if (tab->ctx != ctx) { why = "a gain table belongs to another context"; return false; }
  if (mode != PRISIM_GAINS_ANTENNA && mode != PRISIM_GAINS_BASELINE) { why = "unknown factor mode"; return false; }
  if (!a || !c) { why = "null factor index array"; return false; }
  if (!(tab->nt == nt || tab->nt == 1) || !(tab->nchan == nchan || tab->nchan == 1)) {
    why = "a gain table's snapshots / channels must match the cube's or be 1";
    return false;
  }
  for (int64_t b = 0; b < nbl; ++b) {
    if (a[b] < -1 || a[b] >= tab->nrows) { why = "factor row out of range at baseline " + std::to_string(b); return false; }
    if (mode == PRISIM_GAINS_ANTENNA && a[b] >= 0 && (c[b] < 0 || c[b] >= tab->nrows)) {
      why = "factor row out of range at baseline " + std::to_string(b);
      return false;
    }
  }
  return true;
}

}  // namespace

extern "C" {

int prisim_gains_eval_spline(prisim_ctx* ctx, int64_t nrows, int32_t kx, int32_t ky, const int64_t* nx, const int64_t* ny,
                             const int64_t* kx_off, const int64_t* ky_off, const int64_t* c_off, int64_t nknots, const double* knots,
                             int64_t ncoefs, const double* coefs, int64_t nt, const double* times, int64_t nchan, const double* freqs,
                             prisim_gains_table** out, prisim_gains_stats* stats) {
  return guarded(ctx, [&]() -> int {
  if (!ctx) return PRISIM_EINVAL;
  if (!out) return fail(ctx, PRISIM_EINVAL, "out is NULL");
  *out = nullptr;
  if (nrows < 1 || nt < 1 || nchan < 1) return fail(ctx, PRISIM_EINVAL, "need nrows, nt and nchan >= 1");
  if (kx < 0 || ky < 0 || kx > kMaxK || ky > kMaxK)
    return fail(ctx, PRISIM_EINVAL, "spline degrees must be 0 to " + std::to_string(kMaxK));
  if (!nx || !ny || !kx_off || !ky_off || !c_off || !knots || !coefs || !times || !freqs) return fail(ctx, PRISIM_EINVAL, "null array");
  const int64_t nspl = 2 * nrows;
  for (int64_t s = 0; s < nspl; ++s) {
    if (nx[s] < 2 * kx + 2 || ny[s] < 2 * ky + 2) return fail(ctx, PRISIM_EINVAL, "spline " + std::to_string(s) + " has too few knots");
    if (kx_off[s] < 0 || kx_off[s] + nx[s] > nknots || ky_off[s] < 0 || ky_off[s] + ny[s] > nknots)
      return fail(ctx, PRISIM_EINVAL, "knots of spline " + std::to_string(s) + " out of range");
    const int64_t nc = (nx[s] - kx - 1) * (ny[s] - ky - 1);
    if (c_off[s] < 0 || c_off[s] + nc > ncoefs) return fail(ctx, PRISIM_EINVAL, "coefficients of spline " + std::to_string(s) + " out of range");
    for (int64_t i = 1; i < nx[s]; ++i)
      if (knots[kx_off[s] + i] < knots[kx_off[s] + i - 1]) return fail(ctx, PRISIM_EINVAL, "knots must not decrease");
    for (int64_t i = 1; i < ny[s]; ++i)
      if (knots[ky_off[s] + i] < knots[ky_off[s] + i - 1]) return fail(ctx, PRISIM_EINVAL, "knots must not decrease");
  }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  Dev dev;
  Events ev;
  int rc;
  if ((rc = ev.create(ctx))) return rc;
  int64_t *d_nx, *d_ny, *d_kxo, *d_kyo, *d_co;
  double *d_kn, *d_c, *d_t, *d_f, *d_wx, *d_wy;
  int32_t *d_sx, *d_sy;
  DEV_ALLOC(ctx, dev, d_nx, nspl * 8);
  DEV_ALLOC(ctx, dev, d_ny, nspl * 8);
  DEV_ALLOC(ctx, dev, d_kxo, nspl * 8);
  DEV_ALLOC(ctx, dev, d_kyo, nspl * 8);
  DEV_ALLOC(ctx, dev, d_co, nspl * 8);
  DEV_ALLOC(ctx, dev, d_kn, nknots * 8);
  DEV_ALLOC(ctx, dev, d_c, ncoefs * 8);
  DEV_ALLOC(ctx, dev, d_t, nt * 8);
  DEV_ALLOC(ctx, dev, d_f, nchan * 8);
  DEV_ALLOC(ctx, dev, d_sx, nspl * nt * 4);
  DEV_ALLOC(ctx, dev, d_sy, nspl * nchan * 4);
  DEV_ALLOC(ctx, dev, d_wx, nspl * nt * kW * 8);
  DEV_ALLOC(ctx, dev, d_wy, nspl * nchan * kW * 8);
  prisim_gains_table* tab = nullptr;
  if ((rc = new_table(ctx, nt, nrows, nchan, &tab))) return rc;
  struct Guard {
    prisim_gains_table*& t;
    ~Guard() { if (t) prisim_gains_table_free(t); }
  } guard{tab};
  hipStream_t st = ctx->stream;
  HIPCHK(ctx, hipEventRecord(ev.e[0], st));
  HIPCHK(ctx, hipMemcpyAsync(d_nx, nx, nspl * 8, hipMemcpyHostToDevice, st));
  HIPCHK(ctx, hipMemcpyAsync(d_ny, ny, nspl * 8, hipMemcpyHostToDevice, st));
  HIPCHK(ctx, hipMemcpyAsync(d_kxo, kx_off, nspl * 8, hipMemcpyHostToDevice, st));
  HIPCHK(ctx, hipMemcpyAsync(d_kyo, ky_off, nspl * 8, hipMemcpyHostToDevice, st));
  HIPCHK(ctx, hipMemcpyAsync(d_co, c_off, nspl * 8, hipMemcpyHostToDevice, st));
  if (nknots) HIPCHK(ctx, hipMemcpyAsync(d_kn, knots, nknots * 8, hipMemcpyHostToDevice, st));
  if (ncoefs) HIPCHK(ctx, hipMemcpyAsync(d_c, coefs, ncoefs * 8, hipMemcpyHostToDevice, st));
  HIPCHK(ctx, hipMemcpyAsync(d_t, times, nt * 8, hipMemcpyHostToDevice, st));
  HIPCHK(ctx, hipMemcpyAsync(d_f, freqs, nchan * 8, hipMemcpyHostToDevice, st));
  HIPCHK(ctx, hipEventRecord(ev.e[1], st));
  BasisParams bx{d_nx, d_kxo, d_kn, kx, d_t, nt, nspl, d_sx, d_wx};
  BasisParams by{d_ny, d_kyo, d_kn, ky, d_f, nchan, nspl, d_sy, d_wy};
  hipLaunchKernelGGL(k_basis, dim3((unsigned)blocks_for(ctx, (nspl * nt + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, bx);
  HIPCHK(ctx, hipGetLastError());
  hipLaunchKernelGGL(k_basis, dim3((unsigned)blocks_for(ctx, (nspl * nchan + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, by);
  HIPCHK(ctx, hipGetLastError());
  EvalParams P{d_ny, d_co, d_c, kx, ky, nt, nrows, nchan, d_sx, d_wx, d_sy, d_wy, tab->d, (nchan + kThreads - 1) / kThreads};
  hipLaunchKernelGGL(k_eval, dim3((unsigned)blocks_for(ctx, nt * nrows * P.nchunk)), dim3(kThreads), 0, st, P);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipEventRecord(ev.e[2], st));
  HIPCHK(ctx, hipEventRecord(ev.e[3], st));
  HIPCHK(ctx, hipStreamSynchronize(st));        // the scratch above is freed on return
  if ((rc = fill_stats(ctx, ev, nt * nrows * nchan, stats))) return rc;
  *out = tab;
  tab = nullptr;
  return PRISIM_OK;
  });
}

int prisim_gains_gather(prisim_ctx* ctx, int64_t nrows, int64_t ngf, int64_t ngt, const double* gains, int64_t nchan, const int64_t* fidx,
                        int64_t nt, const int64_t* tidx, prisim_gains_table** out, prisim_gains_stats* stats) {
  return guarded(ctx, [&]() -> int {
  if (!ctx) return PRISIM_EINVAL;
  if (!out) return fail(ctx, PRISIM_EINVAL, "out is NULL");
  *out = nullptr;
  if (nrows < 1 || ngf < 1 || ngt < 1 || nchan < 1 || nt < 1) return fail(ctx, PRISIM_EINVAL, "need every size >= 1");
  if (!gains || !fidx || !tidx) return fail(ctx, PRISIM_EINVAL, "null array");
  for (int64_t f = 0; f < nchan; ++f)
    if (fidx[f] < 0 || fidx[f] >= ngf) return fail(ctx, PRISIM_EINVAL, "frequency index out of range");
  for (int64_t t = 0; t < nt; ++t)
    if (tidx[t] < 0 || tidx[t] >= ngt) return fail(ctx, PRISIM_EINVAL, "time index out of range");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  Dev dev;
  Events ev;
  int rc;
  if ((rc = ev.create(ctx))) return rc;
  double2* d_g;
  int64_t *d_fi, *d_ti;
  const size_t gbytes = (size_t)nrows * ngf * ngt * 16;
  DEV_ALLOC(ctx, dev, d_g, gbytes);
  DEV_ALLOC(ctx, dev, d_fi, nchan * 8);
  DEV_ALLOC(ctx, dev, d_ti, nt * 8);
  prisim_gains_table* tab = nullptr;
  if ((rc = new_table(ctx, nt, nrows, nchan, &tab))) return rc;
  struct Guard {
    prisim_gains_table*& t;
    ~Guard() { if (t) prisim_gains_table_free(t); }
  } guard{tab};
  hipStream_t st = ctx->stream;
  HIPCHK(ctx, hipEventRecord(ev.e[0], st));
  HIPCHK(ctx, hipMemcpyAsync(d_g, gains, gbytes, hipMemcpyHostToDevice, st));
  HIPCHK(ctx, hipMemcpyAsync(d_fi, fidx, nchan * 8, hipMemcpyHostToDevice, st));
  HIPCHK(ctx, hipMemcpyAsync(d_ti, tidx, nt * 8, hipMemcpyHostToDevice, st));
  HIPCHK(ctx, hipEventRecord(ev.e[1], st));
  const int64_t total = nt * nrows * nchan;
  hipLaunchKernelGGL(k_gather, dim3((unsigned)blocks_for(ctx, (total + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, d_g, nrows, ngf,
                     ngt, d_fi, d_ti, nt, nchan, tab->d);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipEventRecord(ev.e[2], st));
  HIPCHK(ctx, hipEventRecord(ev.e[3], st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  if ((rc = fill_stats(ctx, ev, total, stats))) return rc;
  *out = tab;
  tab = nullptr;
  return PRISIM_OK;
  });
}

int prisim_gains_table_shape(const prisim_gains_table* tab, int64_t* nt, int64_t* nrows, int64_t* nchan) {
  if (!tab || !nt || !nrows || !nchan) return PRISIM_EINVAL;
  *nt = tab->nt;
  *nrows = tab->nrows;
  *nchan = tab->nchan;
  return PRISIM_OK;
}

int prisim_gains_table_get(prisim_ctx* ctx, const prisim_gains_table* tab, double* out) {
  return guarded(ctx, [&]() -> int {
  if (!ctx) return PRISIM_EINVAL;
  if (!tab || !out) return fail(ctx, PRISIM_EINVAL, "null table or output");
  if (tab->ctx != ctx) return fail(ctx, PRISIM_EINVAL, "the gain table belongs to another context");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipMemcpyAsync(out, tab->d, (size_t)tab->nt * tab->nrows * tab->nchan * 16, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return PRISIM_OK;
  });
}

void prisim_gains_table_free(prisim_gains_table* tab) {
  if (!tab) return;
  if (tab->d) {
    int prev = -1;
    const bool had = hipGetDevice(&prev) == hipSuccess;
    (void)hipSetDevice(tab->device);
    (void)hipFree(tab->d);
    if (had && prev != tab->device) (void)hipSetDevice(prev);      // the calling thread keeps its current device
  }
  delete tab;
}

int prisim_gains_apply(prisim_ctx* ctx, int64_t nt, int64_t nbl, int64_t nchan, const prisim_gains_table* ta, int32_t mode_a,
                       const int64_t* a_a, const int64_t* c_a, const prisim_gains_table* tb, int32_t mode_b, const int64_t* a_b,
                       const int64_t* c_b, const double* sky, int64_t t0, int32_t sky_c64, const double* noise, int32_t want_gain,
                       double* vis, prisim_gains_stats* stats) {
  return guarded(ctx, [&]() -> int {
  if (!ctx) return PRISIM_EINVAL;
  if (nt < 1 || nbl < 1 || nchan < 1) return fail(ctx, PRISIM_EINVAL, "need nt, nbl and nchan >= 1");
  if (!vis) return fail(ctx, PRISIM_EINVAL, "vis is NULL");
  std::string why;
  if (!factor_ok(ta, mode_a, a_a, c_a, nt, nchan, nbl, ctx, why) || !factor_ok(tb, mode_b, a_b, c_b, nt, nchan, nbl, ctx, why))
    return fail(ctx, PRISIM_EINVAL, why);
  if (!want_gain && !sky) {
    if (!ctx->array_set) return fail(ctx, PRISIM_ESTATE, "resident sky needs set_array first");
    if (nbl != ctx->nbl || nchan != ctx->nchan) return fail(ctx, PRISIM_EINVAL, "the resident sky has the array's nbl and nchan");
    if (t0 < 0 || t0 + nt > ctx->nt_max) return fail(ctx, PRISIM_EINVAL, "resident slots out of range");
  }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  Dev dev;
  Events ev;
  int rc;
  if ((rc = ev.create(ctx))) return rc;
  const int64_t nel = nt * nbl * nchan;
  const size_t snap_bytes = (size_t)nbl * nchan * 16;
  // the cube streams through the device in chunks of whole snapshots: sky, noise and output buffers of at most kApplyChunkBytes each
  const int64_t tc = std::max<int64_t>(1, std::min<int64_t>(nt, (int64_t)(kApplyChunkBytes / std::max<size_t>(snap_bytes, 1))));
  const size_t cbytes = (size_t)tc * snap_bytes;
  double2 *d_sky = nullptr, *d_noise = nullptr, *d_out;
  int64_t *d_aa = nullptr, *d_ca = nullptr, *d_ab = nullptr, *d_cb = nullptr;
  DEV_ALLOC(ctx, dev, d_out, cbytes);
  if (!want_gain && sky) DEV_ALLOC(ctx, dev, d_sky, cbytes);
  if (!want_gain && noise) DEV_ALLOC(ctx, dev, d_noise, cbytes);
  if (ta) { DEV_ALLOC(ctx, dev, d_aa, nbl * 8); DEV_ALLOC(ctx, dev, d_ca, nbl * 8); }
  if (tb) { DEV_ALLOC(ctx, dev, d_ab, nbl * 8); DEV_ALLOC(ctx, dev, d_cb, nbl * 8); }
  hipStream_t st = ctx->stream;
  HIPCHK(ctx, hipEventRecord(ev.e[0], st));
  if (ta) {
    HIPCHK(ctx, hipMemcpyAsync(d_aa, a_a, nbl * 8, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(d_ca, c_a, nbl * 8, hipMemcpyHostToDevice, st));
  }
  if (tb) {
    HIPCHK(ctx, hipMemcpyAsync(d_ab, a_b, nbl * 8, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(d_cb, c_b, nbl * 8, hipMemcpyHostToDevice, st));
  }
  ApplyParams P;
  if (ta) P.fa = Factor{ta->d, ta->nrows, ta->nt, ta->nchan, mode_a, d_aa, d_ca};
  if (tb) P.fb = Factor{tb->d, tb->nrows, tb->nt, tb->nchan, mode_b, d_ab, d_cb};
  P.noise = want_gain ? nullptr : d_noise;
  P.out = d_out;
  P.nbl = nbl; P.nchan = nchan; P.nchunk = (nchan + kThreads - 1) / kThreads;
  P.sky_c64 = sky_c64 ? 1 : 0;
  P.want_gain = want_gain ? 1 : 0;
  double kernel_ms = 0.0;
  for (int64_t c0 = 0; c0 < nt; c0 += tc) {
    const int64_t n = std::min<int64_t>(tc, nt - c0);
    const size_t off = (size_t)c0 * nbl * nchan, bytes = (size_t)n * snap_bytes;
    if (d_sky) HIPCHK(ctx, hipMemcpyAsync(d_sky, sky + 2 * off, bytes, hipMemcpyHostToDevice, st));
    if (d_noise) HIPCHK(ctx, hipMemcpyAsync(d_noise, noise + 2 * off, bytes, hipMemcpyHostToDevice, st));
    P.sky = want_gain ? nullptr : (sky ? d_sky : (const double2*)ctx->cube.p + (t0 + c0) * nbl * nchan);
    P.nt = n;
    P.t_base = c0;
    HIPCHK(ctx, hipEventRecord(ev.e[1], st));
    hipLaunchKernelGGL(k_apply, dim3((unsigned)std::min<int64_t>(n * nbl * P.nchunk, kMaxBlocks)), dim3(kThreads), 0, st, P);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipEventRecord(ev.e[2], st));
    HIPCHK(ctx, hipMemcpyAsync(vis + 2 * off, d_out, bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipEventSynchronize(ev.e[2]));
    float kms = 0.0f;
    HIPCHK(ctx, hipEventElapsedTime(&kms, ev.e[1], ev.e[2]));
    kernel_ms += kms;
  }
  HIPCHK(ctx, hipEventRecord(ev.e[3], st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  if (stats) {
    float ms = 0.0f;
    HIPCHK(ctx, hipEventElapsedTime(&ms, ev.e[0], ev.e[3]));
    stats->device_ms = ms;
    stats->kernel_ms = kernel_ms;
    stats->elements = nel;
  }
  return PRISIM_OK;
  });
}

}  // extern "C"
