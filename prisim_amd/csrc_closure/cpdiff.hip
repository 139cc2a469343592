// cpdiff.hip -- differences of day sub-samples of binned closure phases for gfx950 (include/prisim_cpdiff.h): the last step of
// prisim/bispectrum_phase.py:ClosurePhase.subsample_differencing (:2209-2249).
//
// The stack lies on the device as prisim_cphase_bin left it, [n0][n1][triad][nchan], channel fastest (mean phase, median phase and
// weights): a whole resident stack, or a chunk of triads uploaded by this file's loop.  The outputs are [n0][ncomb][triad][nchan].
// k_cpdiff gives one thread to (i0, a run of kRun consecutive pairs of pairs, triad, channel), channel fastest across the wavefront,
// so that every member read and every store of a wavefront is one coalesced piece of a row (1 KiB of complex128, 512 B of float64,
// 64 B of uint8).  A thread keeps the four members (i, j, k, m) of its current pair of pairs in registers -- index, weight and the
// two unit phasors -- and, walking its run, takes a member anew (three loads, two sincos) only where the index changed: in the
// reference's enumeration (i, j) stays for many steps and k for several, so a step costs about one member, not four.  The index
// comparison is uniform across a wavefront that lies within one row.
//
// Every input element is used by 12 C(n1, 4) / n1 outputs; a chunk's input is n1 / (3 C(n1, 4)) * 24 / 82 of its output, a few
// per cent from n1 = 6 on, and what one run re-reads are the same 512 B pieces that its neighbours on the other runs read.  The
// expectation, not yet confirmed by a counter run, is that the re-reads are served by L2 (and mostly the vector L1), so that device
// memory sees every input element about once.  No atomics, no LDS, no scratch.
//
// Roofline: the kernel is bound by its stores, 82 B per output element (4 x 16 + 2 x 8 + 2 x 1) against at most 24 B read:
//   t >= 82 B * n0 * ncomb * ntriads * nchan / BW,  BW = 8.0 TB/s peak HBM3E, about 6.2 TB/s achievable for plain stores.
// With n0 = 20, n1 = 8 (ncomb = 210), 30 triads and 1024 channels that is 10.6 GB: 1.3 ms at the peak, 1.7 ms achievable.  The
// arithmetic beside it is about three fp64 sincos per element.  fp64, built with -ffp-contract=off.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/prisim_cpdiff.h"
#include "cpstack_internal.h"

namespace {

constexpr int kRun = 16;     // pairs of pairs per thread

struct DiffParams {
  // input: element (i0, i1, t, c) of the launch lies at (i0 * n1 + i1) * in_pitch + t * nc + c
  const double* pm;
  const double* pd;
  const double* w;
  int64_t in_pitch;
  // output element (i0, q, t, c) lies at (i0 * ncomb + q) * out_pitch + t * nc + c of its array (complex outputs: in double2)
  double2* diff[4];          // g = 0 mean, g = 0 median, g = 1 mean, g = 1 median
  double* wts[2];
  uint8_t* mask[2];
  int64_t out_pitch;         // = tn * nc
  const int4* pairs;         // [ncomb] (i, j, k, m)
  int64_t n0, n1, ncomb, nruns;
};

struct Member {
  int idx;
  double w;
  double2 em, ed;            // (cos, sin) of the mean and of the median phase
};

__device__ __forceinline__ void take(const DiffParams& p, int64_t base, int a, Member& m) {
  if (a == m.idx) return;
  const int64_t e = base + (int64_t)a * p.in_pitch;
  m.idx = a;
  m.w = p.w[e];
  sincos(p.pm[e], &m.em.y, &m.em.x);
  sincos(p.pd[e], &m.ed.y, &m.ed.x);
}

__device__ __forceinline__ void put(const DiffParams& p, int g, int64_t o, const Member& a, const Member& b) {
  const bool masked = !(a.w > 0.0) || !(b.w > 0.0);
  p.mask[g][o] = masked ? 1 : 0;
  p.wts[g][o] = sqrt(b.w * b.w + a.w * a.w);
  const double2 zero = make_double2(0.0, 0.0);
  p.diff[2 * g][o] = masked ? zero : make_double2(0.5 * (b.em.x - a.em.x), 0.5 * (b.em.y - a.em.y));
  p.diff[2 * g + 1][o] = masked ? zero : make_double2(0.5 * (b.ed.x - a.ed.x), 0.5 * (b.ed.y - a.ed.y));
}

__global__ __launch_bounds__(kThreads) void k_cpdiff(const DiffParams p) {
  const int64_t per_row = p.out_pitch;
  const int64_t total = p.n0 * p.nruns * per_row;
  for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * kThreads) {
    const int64_t r = idx / per_row, tc = idx - r * per_row;
    const int64_t i0 = r / p.nruns, run = r - i0 * p.nruns;
    const int64_t base = i0 * p.n1 * p.in_pitch + tc;
    const int64_t q0 = run * kRun, q1 = min(q0 + (int64_t)kRun, p.ncomb);
    Member mi, mj, mk, mm;
    mi.idx = mj.idx = mk.idx = mm.idx = -1;
    for (int64_t q = q0; q < q1; ++q) {
      const int4 pr = p.pairs[q];
      take(p, base, pr.x, mi);
      take(p, base, pr.y, mj);
      take(p, base, pr.z, mk);
      take(p, base, pr.w, mm);
      const int64_t o = (i0 * p.ncomb + q) * per_row + tc;
      put(p, 0, o, mi, mj);
      put(p, 1, o, mk, mm);
    }
  }
}

}  // namespace

extern "C" {

int prisim_cphase_diff(prisim_ctx* ctx, const double* in_mean, const double* in_median, const double* in_wts, int64_t n0, int64_t n1,
                       int64_t ntriads, int64_t nchan, prisim_cphase_stack* resident, int64_t ncomb, const int32_t* pairs,
                       int64_t budget_bytes, double* out_diff0_mean, double* out_diff0_median, double* out_diff1_mean,
                       double* out_diff1_median, double* out_wts0, double* out_wts1, uint8_t* out_mask0, uint8_t* out_mask1,
                       prisim_cpdiff_stats* stats) {
  return guarded(ctx, [&]() -> int {
  if (!ctx) return PRISIM_EINVAL;
  const WallTime wall0 = wall_now();
  if (n0 < 1 || n1 < 1 || ntriads < 1 || nchan < 1) return fail(ctx, PRISIM_EINVAL, "need n0, n1, ntriads and nchan >= 1");
  if (n0 > (int64_t)1 << 24 || n1 > (int64_t)1 << 24 || ntriads > (int64_t)1 << 24 || nchan > (int64_t)1 << 24 ||
      n0 * n1 > ((int64_t)1 << 38) / (ntriads * nchan))
    return fail(ctx, PRISIM_EINVAL, "the stack is too large (2^38 elements at most)");
  if (ncomb < 1) return fail(ctx, PRISIM_EINVAL, "need ncomb >= 1 pairs of pairs");
  if (ncomb > (int64_t)1 << 24 || n0 * ncomb > ((int64_t)1 << 38) / (ntriads * nchan))
    return fail(ctx, PRISIM_EINVAL, "the outputs are too large (2^38 elements at most)");
  if (resident && (resident->kind != PRISIM_CPBINS_BINNED || resident->n0 != n0 || resident->n1 != n1 || resident->nt != ntriads ||
                   resident->nc != nchan || resident->device != ctx->device))
    return fail(ctx, PRISIM_EINVAL, "the resident stack is not of kind BINNED, or of another shape or device");
  if (!resident && (!in_mean || !in_median || !in_wts)) return fail(ctx, PRISIM_EINVAL, "null input array");
  if (!pairs) return fail(ctx, PRISIM_EINVAL, "null pairs");
  for (int64_t q = 0; q < ncomb; ++q) {
    const int32_t* pr = pairs + 4 * q;
    for (int s = 0; s < 4; ++s)
      if (pr[s] < 0 || pr[s] >= n1)
        return fail(ctx, PRISIM_EINVAL, "pair of pairs " + std::to_string(q) + " holds " + std::to_string(pr[s]) + ", not an index of axis 1");
    if (pr[0] == pr[1] || pr[2] == pr[3])
      return fail(ctx, PRISIM_EINVAL, "pair of pairs " + std::to_string(q) + " holds a pair of one index with itself");
  }
  if (!out_diff0_mean || !out_diff0_median || !out_diff1_mean || !out_diff1_median || !out_wts0 || !out_wts1 || !out_mask0 || !out_mask1)
    return fail(ctx, PRISIM_EINVAL, "an output is NULL");
  HIPCHK(ctx, hipSetDevice(ctx->device));

  const int64_t rows_in = n0 * n1, rows_out = n0 * ncomb, row_elems = ntriads * nchan;
  // chunks of triads: the chunk's input (unless resident) and its outputs within the budget
  const int64_t per_triad = (resident ? 0 : rows_in * nchan * 24) + rows_out * nchan * PRISIM_CPDIFF_OUT_BYTES;
  const Chunks ch = plan_chunks(ntriads, per_triad, budget_bytes, 1);
  const int64_t tc = ch.size, nchunks = ch.count;

  Work wk;
  Streams& st = wk.st;
  if (int rc = st.create(ctx, 1, true)) return rc;
  hipStream_t s = st.s[0];
  int4* d_pairs;
  DEV_UPLOAD(ctx, wk.dev, d_pairs, pairs, (size_t)ncomb * 4, s);
  double *d_a = nullptr, *d_b = nullptr, *d_w = nullptr;
  if (!resident) {
    DEV_ALLOC(ctx, wk.dev, d_a, rows_in * tc * nchan * 8);
    DEV_ALLOC(ctx, wk.dev, d_b, rows_in * tc * nchan * 8);
    DEV_ALLOC(ctx, wk.dev, d_w, rows_in * tc * nchan * 8);
  }
  // the eight outputs: four complex128, two float64, two uint8
  constexpr size_t es[8] = {16, 16, 16, 16, 8, 8, 1, 1};
  void* const host_out[8] = {out_diff0_mean, out_diff0_median, out_diff1_mean, out_diff1_median, out_wts0, out_wts1, out_mask0, out_mask1};
  char* d_out[8] = {};
  for (int o = 0; o < 8; ++o) DEV_ALLOC(ctx, wk.dev, d_out[o], rows_out * tc * nchan * (int64_t)es[o]);
  int64_t upload_bytes = ncomb * 16, download_bytes = 0;

  DiffParams p{};                                     // of the chunk in hand
  auto upload = [&](int64_t, Span sp, int, hipStream_t) -> int {
    const int64_t T0 = sp.first, tn = sp.count;
    p = DiffParams{};
    if (resident) {
      const int64_t o = T0 * nchan;
      p.pm = resident->a + o;
      p.pd = resident->b + o;
      p.w = resident->w + o;
      p.in_pitch = row_elems;
    } else {
      const size_t hp = (size_t)row_elems * 8, w = (size_t)(tn * nchan) * 8;
      HIPCHK(ctx, copy_rows(d_a, w, in_mean + T0 * nchan, hp, w, rows_in, hipMemcpyHostToDevice, s));
      HIPCHK(ctx, copy_rows(d_b, w, in_median + T0 * nchan, hp, w, rows_in, hipMemcpyHostToDevice, s));
      HIPCHK(ctx, copy_rows(d_w, w, in_wts + T0 * nchan, hp, w, rows_in, hipMemcpyHostToDevice, s));
      upload_bytes += rows_in * tn * nchan * 24;
      p.pm = d_a;
      p.pd = d_b;
      p.w = d_w;
      p.in_pitch = tn * nchan;
    }
    for (int o = 0; o < 4; ++o) p.diff[o] = reinterpret_cast<double2*>(d_out[o]);
    for (int g = 0; g < 2; ++g) {
      p.wts[g] = reinterpret_cast<double*>(d_out[4 + g]);
      p.mask[g] = reinterpret_cast<uint8_t*>(d_out[6 + g]);
    }
    p.out_pitch = tn * nchan;
    p.pairs = d_pairs;
    p.n0 = n0;
    p.n1 = n1;
    p.ncomb = ncomb;
    p.nruns = (ncomb + kRun - 1) / kRun;
    return PRISIM_OK;
  };
  auto kernels = [&](int64_t, Span sp, int, hipStream_t) -> int {
    const int64_t total = n0 * p.nruns * sp.count * nchan;
    const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>((total + kThreads - 1) / kThreads, kMaxBlocks));
    return launch(ctx, k_cpdiff, dim3((unsigned)blocks), 0, s, p);
  };
  auto download = [&](int64_t, Span sp, int, hipStream_t) -> int {
    const int64_t T0 = sp.first, tn = sp.count;
    for (int o = 0; o < 8; ++o) {
      HIPCHK(ctx, copy_rows(static_cast<char*>(host_out[o]) + (size_t)(T0 * nchan) * es[o], (size_t)row_elems * es[o], d_out[o],
                            (size_t)(tn * nchan) * es[o], (size_t)(tn * nchan) * es[o], rows_out, hipMemcpyDeviceToHost, s));
      download_bytes += rows_out * tn * nchan * (int64_t)es[o];
    }
    return PRISIM_OK;
  };
  if (int rc = chunk_loop(ctx, st, ch, ntriads, upload, kernels, download)) return rc;   // one stream: its order guards the reused buffers
  if (stats) {
    stats->wall_ms = wall_ms_since(wall0);
    stats->kernel_ms = st.kernel_ms;
    stats->elements = rows_out * row_elems;
    stats->chunks = nchunks;
    stats->chunk_triads = tc;
    stats->kernel_bytes = rows_in * row_elems * 24 + rows_out * row_elems * PRISIM_CPDIFF_OUT_BYTES;
    stats->upload_bytes = upload_bytes;
    stats->download_bytes = download_bytes;
    stats->resident_in = resident ? 1 : 0;
    stats->ncomb = (int32_t)ncomb;
  }
  return PRISIM_OK;
  });
}

}  // extern "C"
