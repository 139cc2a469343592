// cpbins.hip -- flagged binning of closure phases along the day or the LST axis for gfx950 (include/prisim_cpbins.h): the per-bin
// arithmetic of prisim/bispectrum_phase.py:ClosurePhase.smooth_in_tbins (:1791-1797, :1816-1835, :1914-1933).
//
// The stack lies on the device as the host has it, [n0][n1][triad][nchan], channel fastest: a chunk of triads uploaded by this file's
// loop (rows of tn * nchan elements out of rows of ntriads * nchan, a 2-D copy), or a whole resident stack.  k_cpbins gives one
// thread to every output element (row = (bin, index on the other axis), triad, channel), channel fastest across the wavefront, so
// that every member read of a wavefront is one coalesced piece of a row.  A thread walks the members of its bin:
//   pass 1  weights, count, phasor sum, phase sum                             (one sincos per unmasked member)
//   pass 2  sum of squared deviations from the mean phase                     (no sincos)
//   pass 3  the medians of cos pd and of sin pd by rank counting: for every unmasked member i one walk over the unmasked members j
//           counts those below it, ties broken by the position in the bin, for both components at once (one sincos per j, recomputed
//           rather than stored: no scratch, no LDS, no divergent sort); the values of rank (n - 1) / 2 and n / 2 are kept
//   pass 4  the same selection over |pd - cp_median| for the mad
// Only pass 1 misses the caches: the members of a wavefront's bin are n pieces of 512 B that the later passes find in L2 (and mostly
// in the vector L1), so device memory sees every input element about once.  No atomics, no LDS.  fp64, built with -ffp-contract=off.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "../../include/prisim_cpbins.h"
#include "cpstack_internal.h"

namespace {

constexpr int kKept = PRISIM_CPBINS_WTS | PRISIM_CPBINS_CP_MEAN | PRISIM_CPBINS_CP_MEDIAN;

struct BinParams {
  // input: element (i0, i1, t, c) of the launch lies at (i0 * n1 + i1) * in_pitch + t * nc + c
  const double* pm;
  const double* pd;
  const double* w;           // BINNED: the weights; null with flags
  const uint8_t* flags;      // PHASE_FLAGS
  int64_t in_pitch;
  // output element (row, t, c) lies at row * pitch + t * nc + c of its array (complex outputs: in double2)
  double* wts;
  double2* eicp_mean;
  double2* eicp_median;
  double* cp_mean;
  double* cp_median;
  double* rms;
  double* mad;
  int64_t pitch_kept;        // rows of wts, cp_mean, cp_median
  int64_t pitch_chunk;       // rows of the others
  const int64_t* offsets;    // [nbins + 1]
  const int32_t* members;
  int64_t n1;                // second axis of the input
  int64_t nother;            // length of the axis that is not binned
  int64_t nbins, tn, nc;
  int axis, mad_all;
};

struct Member {
  bool masked;
  double wv;
};

__device__ __forceinline__ Member member_of(const BinParams& p, int64_t e) {
  Member m;
  if (p.flags) {
    m.masked = p.flags[e] != 0;
    m.wv = m.masked ? 0.0 : 1.0;
  } else {
    m.wv = p.w[e];
    m.masked = !(m.wv > 0.0);
  }
  return m;
}

__global__ __launch_bounds__(kThreads) void k_cpbins(const BinParams p) {
  const int64_t per_row = p.tn * p.nc;
  const int64_t total = p.nbins * p.nother * per_row;
  for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * kThreads) {
    const int64_t row = idx / per_row, tc = idx - row * per_row;
    // output rows: (bin, i1) when axis 0 is binned, (i0, bin) when axis 1 is
    const int64_t bin = p.axis == 0 ? row / p.nother : row % p.nbins;
    const int64_t other = p.axis == 0 ? row % p.nother : row / p.nbins;
    const int64_t beg = p.offsets[bin], end = p.offsets[bin + 1];
    const int64_t mstride = (p.axis == 0 ? p.n1 : 1) * p.in_pitch;
    const int64_t base = (p.axis == 0 ? other : other * p.n1) * p.in_pitch + tc;
    auto elem = [&](int64_t q) { return base + (int64_t)p.members[q] * mstride; };

    const bool need_mean = p.eicp_mean || p.cp_mean;
    const bool need_median = p.eicp_median || p.cp_median || p.mad;
    // pass 1
    double wsum = 0.0, sr = 0.0, si = 0.0, sp = 0.0;
    int n = 0;
    for (int64_t q = beg; q < end; ++q) {
      const int64_t e = elem(q);
      const Member m = member_of(p, e);
      wsum += m.wv;
      if (m.masked) continue;
      ++n;
      const double a = p.pm[e];
      sp += a;
      if (need_mean) {
        double s, c;
        sincos(a, &s, &c);
        sr += c;
        si += s;
      }
    }
    double2 em = make_double2(1.0, 0.0), ed = make_double2(1.0, 0.0);
    double cm = 0.0, cd = 0.0, rms = 0.0, mad = 0.0;
    if (n > 0) {
      const double dn = (double)n;
      if (need_mean) {
        const double a = atan2(si / dn, sr / dn);
        double s, c;
        sincos(a, &s, &c);
        em = make_double2(c, s);
        cm = atan2(s, c);
      }
      if (p.rms) {   // pass 2
        const double mu = sp / dn;
        double ss = 0.0;
        for (int64_t q = beg; q < end; ++q) {
          const int64_t e = elem(q);
          if (member_of(p, e).masked) continue;
          const double d = p.pm[e] - mu;
          ss += d * d;
        }
        rms = sqrt(ss / dn);
      }
      if (need_median) {   // pass 3
        const int klo = (n - 1) >> 1, khi = n >> 1;
        double clo = 0.0, chi = 0.0, slo = 0.0, shi = 0.0;
        for (int64_t qi = beg; qi < end; ++qi) {
          const int64_t ei = elem(qi);
          if (member_of(p, ei).masked) continue;
          double s_i, c_i;
          sincos(p.pd[ei], &s_i, &c_i);
          int rc = 0, rs = 0;
          for (int64_t qj = beg; qj < end; ++qj) {
            const int64_t ej = elem(qj);
            if (member_of(p, ej).masked) continue;
            double s_j, c_j;
            sincos(p.pd[ej], &s_j, &c_j);
            rc += (c_j < c_i || (c_j == c_i && qj < qi)) ? 1 : 0;
            rs += (s_j < s_i || (s_j == s_i && qj < qi)) ? 1 : 0;
          }
          if (rc == klo) clo = c_i;
          if (rc == khi) chi = c_i;
          if (rs == klo) slo = s_i;
          if (rs == khi) shi = s_i;
        }
        const double a = atan2((slo + shi) / 2.0, (clo + chi) / 2.0);
        double s, c;
        sincos(a, &s, &c);
        ed = make_double2(c, s);
        cd = atan2(s, c);
        if (p.mad) {   // pass 4
          const int nm = p.mad_all ? (int)(end - beg) : n;
          const int mlo = (nm - 1) >> 1, mhi = nm >> 1;
          double dlo = 0.0, dhi = 0.0;
          for (int64_t qi = beg; qi < end; ++qi) {
            const int64_t ei = elem(qi);
            if (!p.mad_all && member_of(p, ei).masked) continue;
            const double d_i = fabs(p.pd[ei] - cd);
            int r = 0;
            for (int64_t qj = beg; qj < end; ++qj) {
              const int64_t ej = elem(qj);
              if (!p.mad_all && member_of(p, ej).masked) continue;
              const double d_j = fabs(p.pd[ej] - cd);
              r += (d_j < d_i || (d_j == d_i && qj < qi)) ? 1 : 0;
            }
            if (r == mlo) dlo = d_i;
            if (r == mhi) dhi = d_i;
          }
          mad = (dlo + dhi) / 2.0;
        }
      }
    }
    const int64_t ok = row * p.pitch_kept + tc, oc = row * p.pitch_chunk + tc;
    if (p.wts) p.wts[ok] = wsum;
    if (p.cp_mean) p.cp_mean[ok] = cm;
    if (p.cp_median) p.cp_median[ok] = cd;
    if (p.eicp_mean) p.eicp_mean[oc] = em;
    if (p.eicp_median) p.eicp_median[oc] = ed;
    if (p.rms) p.rms[oc] = rms;
    if (p.mad) p.mad[oc] = mad;
  }
}

// ---- host side --------------------------------------------------------------------------------------------------------------

#define CB_STACK_ALLOC(ctx, field, bytes)                                                              \
  do {                                                                                                 \
    void* p_ = nullptr;                                                                                \
    HIPCHK(ctx, hipMalloc(&p_, std::max<size_t>((size_t)(bytes), 16)));                                \
    (field) = reinterpret_cast<decltype(field)>(p_);                                                   \
  } while (0)

}  // namespace

extern "C" {

void prisim_cphase_stack_free(prisim_cphase_stack* stack) {
  if (!stack) return;
  (void)hipSetDevice(stack->device);
  delete stack;
}

int prisim_cphase_bin(prisim_ctx* ctx, int32_t kind, const double* in_mean, const double* in_median, const double* in_wts,
                      const uint8_t* in_flags, int64_t n0, int64_t n1, int64_t ntriads, int64_t nchan, int32_t axis, int64_t nbins,
                      const int64_t* offsets, const int32_t* members, int32_t want, int32_t mad_ignores_flags, int64_t budget_bytes,
                      prisim_cphase_stack** resident_in, prisim_cphase_stack** keep_out, double* out_wts, double* out_eicp_mean,
                      double* out_eicp_median, double* out_cp_mean, double* out_cp_median, double* out_rms, double* out_mad,
                      prisim_cpbins_stats* stats) {
  return guarded(ctx, [&]() -> int {
  if (!ctx) return PRISIM_EINVAL;
  const WallTime wall0 = wall_now();
  const bool pf = kind == PRISIM_CPBINS_PHASE_FLAGS;
  if (!pf && kind != PRISIM_CPBINS_BINNED) return fail(ctx, PRISIM_EINVAL, "unknown input kind");
  if (n0 < 1 || n1 < 1 || ntriads < 1 || nchan < 1) return fail(ctx, PRISIM_EINVAL, "need n0, n1, ntriads and nchan >= 1");
  if (n0 > (int64_t)1 << 24 || n1 > (int64_t)1 << 24 || ntriads > (int64_t)1 << 24 || nchan > (int64_t)1 << 24 ||
      n0 * n1 > ((int64_t)1 << 38) / (ntriads * nchan))
    return fail(ctx, PRISIM_EINVAL, "the stack is too large (2^38 elements at most)");
  if (axis != 0 && axis != 1) return fail(ctx, PRISIM_EINVAL, "axis must be 0 or 1");
  if (want & ~PRISIM_CPBINS_ALL) return fail(ctx, PRISIM_EINVAL, "unknown bit in want");
  prisim_cphase_stack* rin = resident_in ? *resident_in : nullptr;
  const bool was_resident = rin != nullptr;
  if (rin && (rin->kind != kind || rin->n0 != n0 || rin->n1 != n1 || rin->nt != ntriads || rin->nc != nchan || rin->device != ctx->device))
    return fail(ctx, PRISIM_EINVAL, "the resident stack is of another kind, shape or device");
  if (!rin && (!in_mean || (pf ? !in_flags : (!in_median || !in_wts)))) return fail(ctx, PRISIM_EINVAL, "null input array");
  const bool upload_only = nbins == 0 && want == 0 && !keep_out;
  if (upload_only && !(resident_in && !rin)) return fail(ctx, PRISIM_EINVAL, "nothing requested (nbins, want)");
  if (!upload_only && (nbins < 1 || !offsets)) return fail(ctx, PRISIM_EINVAL, "need nbins >= 1 and the bin offsets");
  if (!upload_only && !want && !keep_out) return fail(ctx, PRISIM_EINVAL, "nothing requested (want)");
  const int64_t naxis = axis == 0 ? n0 : n1, nother = axis == 0 ? n1 : n0;
  int64_t nmem = 0, max_bin = 0;
  if (!upload_only) {
    if (nbins > (int64_t)1 << 24 || nbins * nother > ((int64_t)1 << 38) / (ntriads * nchan))
      return fail(ctx, PRISIM_EINVAL, "the outputs are too large (2^38 elements at most)");
    if (offsets[0] != 0) return fail(ctx, PRISIM_EINVAL, "offsets must start at 0");
    for (int64_t k = 0; k < nbins; ++k) {
      const int64_t cnt = offsets[k + 1] - offsets[k];
      if (cnt < 0) return fail(ctx, PRISIM_EINVAL, "offsets must not decrease");
      if (cnt > PRISIM_CPBINS_MAX_BIN)
        return fail(ctx, PRISIM_EINVAL, "bin " + std::to_string(k) + " has " + std::to_string(cnt) + " members: more than PRISIM_CPBINS_MAX_BIN (" +
                                            std::to_string(PRISIM_CPBINS_MAX_BIN) + ")");
      max_bin = std::max(max_bin, cnt);
    }
    nmem = offsets[nbins];
    if (nmem > 0 && !members) return fail(ctx, PRISIM_EINVAL, "null members");
    for (int64_t q = 0; q < nmem; ++q)
      if (members[q] < 0 || members[q] >= naxis) return fail(ctx, PRISIM_EINVAL, "member " + std::to_string(q) + " is not an index of the binned axis");
    double* const outs[7] = {out_wts, out_eicp_mean, out_eicp_median, out_cp_mean, out_cp_median, out_rms, out_mad};
    for (int o = 0; o < 7; ++o)
      if ((want >> o & 1) && !outs[o]) return fail(ctx, PRISIM_EINVAL, "a wanted output is NULL");
  }
  HIPCHK(ctx, hipSetDevice(ctx->device));

  const int64_t rows_in = n0 * n1, row_elems = ntriads * nchan;
  int64_t upload_bytes = 0, download_bytes = 0;
  // a stack to leave resident: uploaded whole
  std::unique_ptr<prisim_cphase_stack> made_in;
  if (resident_in && !rin) {
    made_in.reset(new prisim_cphase_stack());
    made_in->device = ctx->device;
    made_in->kind = kind;
    made_in->n0 = n0; made_in->n1 = n1; made_in->nt = ntriads; made_in->nc = nchan;
    const size_t ne = (size_t)(rows_in * row_elems);
    CB_STACK_ALLOC(ctx, made_in->a, ne * 8);
    HIPCHK(ctx, hipMemcpy(made_in->a, in_mean, ne * 8, hipMemcpyHostToDevice));
    if (pf) {
      CB_STACK_ALLOC(ctx, made_in->f, ne);
      HIPCHK(ctx, hipMemcpy(made_in->f, in_flags, ne, hipMemcpyHostToDevice));
      upload_bytes += (int64_t)ne * 9;
    } else {
      CB_STACK_ALLOC(ctx, made_in->b, ne * 8);
      HIPCHK(ctx, hipMemcpy(made_in->b, in_median, ne * 8, hipMemcpyHostToDevice));
      CB_STACK_ALLOC(ctx, made_in->w, ne * 8);
      HIPCHK(ctx, hipMemcpy(made_in->w, in_wts, ne * 8, hipMemcpyHostToDevice));
      upload_bytes += (int64_t)ne * 24;
    }
    rin = made_in.get();
  }
  if (upload_only) {
    *resident_in = made_in.release();
    if (stats) {
      *stats = prisim_cpbins_stats{};
      stats->wall_ms = wall_ms_since(wall0);
      stats->upload_bytes = upload_bytes;
    }
    return PRISIM_OK;
  }

  const int64_t rows_out = nbins * nother;
  const int comp = want | (keep_out ? kKept : 0);
  std::unique_ptr<prisim_cphase_stack> kept;
  if (keep_out) {
    kept.reset(new prisim_cphase_stack());
    kept->device = ctx->device;
    kept->kind = PRISIM_CPBINS_BINNED;
    kept->n0 = axis == 0 ? nbins : n0; kept->n1 = axis == 0 ? n1 : nbins; kept->nt = ntriads; kept->nc = nchan;
    const size_t nb = (size_t)(rows_out * row_elems) * 8;
    CB_STACK_ALLOC(ctx, kept->a, nb);
    CB_STACK_ALLOC(ctx, kept->b, nb);
    CB_STACK_ALLOC(ctx, kept->w, nb);
  }

  // chunks of triads: the chunk's input (unless resident) and its outputs (unless kept) within the budget
  const int64_t in_per_triad = rin ? 0 : rows_in * nchan * (pf ? 9 : 24);
  int64_t out_doubles = 0;
  for (int o = 0; o < 7; ++o)
    if (comp >> o & 1) {
      const bool is_kept = keep_out && (kKept >> o & 1);
      if (!is_kept) out_doubles += (o == 1 || o == 2) ? 2 : 1;
    }
  const int64_t per_triad = in_per_triad + rows_out * nchan * 8 * out_doubles;
  const Chunks ch = per_triad > 0 ? plan_chunks(ntriads, per_triad, budget_bytes, 1) : chunks_of(ntriads, ntriads, 1);
  const int64_t tc = ch.size, nchunks = ch.count;

  Work wk;
  Streams& st = wk.st;
  if (int rc = st.create(ctx, 1, true)) return rc;
  hipStream_t s = st.s[0];
  int64_t* d_off;
  int32_t* d_mem;
  DEV_UPLOAD(ctx, wk.dev, d_off, offsets, (size_t)nbins + 1, s);
  DEV_UPLOAD(ctx, wk.dev, d_mem, members, (size_t)nmem, s);
  double *d_a = nullptr, *d_b = nullptr, *d_w = nullptr;
  uint8_t* d_f = nullptr;
  if (!rin) {
    DEV_ALLOC(ctx, wk.dev, d_a, rows_in * tc * nchan * 8);
    if (pf) {
      DEV_ALLOC(ctx, wk.dev, d_f, rows_in * tc * nchan);
    } else {
      DEV_ALLOC(ctx, wk.dev, d_b, rows_in * tc * nchan * 8);
      DEV_ALLOC(ctx, wk.dev, d_w, rows_in * tc * nchan * 8);
    }
  }
  double* d_out[7] = {};
  for (int o = 0; o < 7; ++o)
    if ((comp >> o & 1) && !(keep_out && (kKept >> o & 1))) DEV_ALLOC(ctx, wk.dev, d_out[o], rows_out * tc * nchan * ((o == 1 || o == 2) ? 16 : 8));
  upload_bytes += (nbins + 1) * 8 + nmem * 4;

  double* const host_out[7] = {out_wts, out_eicp_mean, out_eicp_median, out_cp_mean, out_cp_median, out_rms, out_mad};
  BinParams p{};                                      // of the chunk in hand
  auto upload = [&](int64_t, Span sp, int, hipStream_t) -> int {
    const int64_t T0 = sp.first, tn = sp.count;
    p = BinParams{};
    if (rin) {
      const int64_t o = T0 * nchan;
      p.pm = rin->a + o;
      p.pd = pf ? p.pm : rin->b + o;
      p.w = pf ? nullptr : rin->w + o;
      p.flags = pf ? rin->f + o : nullptr;
      p.in_pitch = row_elems;
    } else {
      const size_t hp = (size_t)row_elems, w = (size_t)(tn * nchan);
      HIPCHK(ctx, copy_rows(d_a, w * 8, in_mean + T0 * nchan, hp * 8, w * 8, rows_in, hipMemcpyHostToDevice, s));
      if (pf) {
        HIPCHK(ctx, copy_rows(d_f, w, in_flags + T0 * nchan, hp, w, rows_in, hipMemcpyHostToDevice, s));
      } else {
        HIPCHK(ctx, copy_rows(d_b, w * 8, in_median + T0 * nchan, hp * 8, w * 8, rows_in, hipMemcpyHostToDevice, s));
        HIPCHK(ctx, copy_rows(d_w, w * 8, in_wts + T0 * nchan, hp * 8, w * 8, rows_in, hipMemcpyHostToDevice, s));
      }
      upload_bytes += rows_in * tn * nchan * (pf ? 9 : 24);
      p.pm = d_a;
      p.pd = pf ? d_a : d_b;
      p.w = d_w;
      p.flags = d_f;
      p.in_pitch = tn * nchan;
    }
    p.pitch_chunk = tn * nchan;
    if (keep_out) {
      p.pitch_kept = row_elems;
      p.wts = kept->w + T0 * nchan;
      p.cp_mean = kept->a + T0 * nchan;
      p.cp_median = kept->b + T0 * nchan;
    } else {
      p.pitch_kept = tn * nchan;
      p.wts = d_out[0];
      p.cp_mean = d_out[3];
      p.cp_median = d_out[4];
    }
    p.eicp_mean = reinterpret_cast<double2*>(d_out[1]);
    p.eicp_median = reinterpret_cast<double2*>(d_out[2]);
    p.rms = d_out[5];
    p.mad = d_out[6];
    p.offsets = d_off;
    p.members = d_mem;
    p.n1 = n1;
    p.nother = nother;
    p.nbins = nbins;
    p.tn = tn;
    p.nc = nchan;
    p.axis = axis;
    p.mad_all = mad_ignores_flags ? 1 : 0;
    return PRISIM_OK;
  };
  auto kernels = [&](int64_t, Span sp, int, hipStream_t) -> int {
    const int64_t total = rows_out * sp.count * nchan;
    const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>((total + kThreads - 1) / kThreads, kMaxBlocks));
    return launch(ctx, k_cpbins, dim3((unsigned)blocks), 0, s, p);
  };
  auto download = [&](int64_t, Span sp, int, hipStream_t) -> int {
    const int64_t T0 = sp.first, tn = sp.count;
    for (int o = 0; o < 7; ++o) {
      if (!(want >> o & 1)) continue;
      const size_t es = (o == 1 || o == 2) ? 16 : 8;
      const bool is_kept = keep_out && (kKept >> o & 1);
      const double* src = is_kept ? (o == 0 ? p.wts : o == 3 ? p.cp_mean : p.cp_median) : d_out[o];
      const size_t spitch = (size_t)(is_kept ? p.pitch_kept : p.pitch_chunk) * es;
      HIPCHK(ctx, copy_rows(reinterpret_cast<char*>(host_out[o]) + (size_t)(T0 * nchan) * es, (size_t)row_elems * es, src, spitch,
                            (size_t)(tn * nchan) * es, rows_out, hipMemcpyDeviceToHost, s));
      download_bytes += rows_out * tn * nchan * (int64_t)es;
    }
    return PRISIM_OK;
  };
  if (int rc = chunk_loop(ctx, st, ch, ntriads, upload, kernels, download)) return rc;   // one stream: its order guards the reused buffers
  if (made_in) *resident_in = made_in.release();
  if (keep_out) *keep_out = kept.release();
  if (stats) {
    int64_t outb = 0;
    for (int o = 0; o < 7; ++o)
      if (comp >> o & 1) outb += (o == 1 || o == 2) ? 16 : 8;
    stats->wall_ms = wall_ms_since(wall0);
    stats->kernel_ms = st.kernel_ms;
    stats->elements = rows_out * row_elems;
    stats->chunks = nchunks;
    stats->chunk_triads = tc;
    stats->kernel_bytes = rows_in * row_elems * (pf ? 9 : 24) + rows_out * row_elems * outb;
    stats->upload_bytes = upload_bytes;
    stats->download_bytes = download_bytes;
    stats->max_bin = (int32_t)max_bin;
    stats->resident_in = was_resident ? 1 : 0;
  }
  return PRISIM_OK;
  });
}

}  // extern "C"
