// addon_internal.h -- what the add-on entries share (csrc_clean, csrc_subband, csrc_gains, csrc_runs, csrc_closure): the per-call
// device buffers, streams, events and rocFFT plans of their chunk loops on the host, and the complex helpers and the in-LDS radix-2 inverse
// transform of their fused kernels on the device (delay_lines.h has the delay add-ons' arithmetic around it).  Not part of the public ABI.
#ifndef PRISIM_ADDON_INTERNAL_H
#define PRISIM_ADDON_INTERNAL_H

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../csrc/ctx_internal.h"
#include "addon_plan.h"

namespace pint {

constexpr int kThreads = 256;                         // threads per workgroup of the add-on kernels
constexpr int kMaxStreams = 2;
constexpr int64_t kMaxBlocks = int64_t(1) << 20;

// ---- host side --------------------------------------------------------------------------------------------------------------

struct Dev {
  std::vector<void*> ptrs;
  ~Dev() { for (void* p : ptrs) (void)hipFree(p); }
};

#define DEV_ALLOC(ctx, dev, ptr, bytes)                                                                \
  do {                                                                                                 \
    void* p_ = nullptr;                                                                                \
    HIPCHK(ctx, hipMalloc(&p_, std::max<size_t>((size_t)(bytes), 16)));                                \
    (dev).ptrs.push_back(p_);                                                                          \
    (ptr) = reinterpret_cast<decltype(ptr)>(p_);                                                       \
  } while (0)

// a table: `count` elements of T allocated and, where there are any on the host, copied up on stream s.  ptr may point to a type
// that packs whole T's (double2 for pairs of doubles, int4 for four int32): count is in T's, and the one byte count serves both.
template <typename P, typename T>
inline int dev_upload(prisim_ctx* ctx, Dev& dev, P*& ptr, const T* host, size_t count, hipStream_t s) {
  static_assert(sizeof(P) % sizeof(T) == 0, "the device element is a whole number of host elements");
  DEV_ALLOC(ctx, dev, ptr, count * sizeof(T));
  if (host && count) HIPCHK(ctx, hipMemcpyAsync(ptr, host, count * sizeof(T), hipMemcpyHostToDevice, s));
  return PRISIM_OK;
}
template <typename P, typename T>
inline int dev_upload(prisim_ctx* ctx, Dev& dev, P*& ptr, const std::vector<T>& host, hipStream_t s) {
  return dev_upload(ctx, dev, ptr, host.data(), host.size(), s);
}

#define DEV_UPLOAD(ctx, dev, ptr, ...)                                                                 \
  do {                                                                                                 \
    if (int rc_ = dev_upload(ctx, dev, ptr, __VA_ARGS__)) return rc_;                                  \
  } while (0)

// A call's own streams, each with an optional pair of kernel-timing events.  Drained when they go.  chunk_loop (below) runs the
// chunks over them.  Without events open and close do nothing and kernel_ms stays 0.
struct Streams {
  hipStream_t s[kMaxStreams] = {};
  hipEvent_t k0[kMaxStreams] = {}, k1[kMaxStreams] = {};
  bool timed[kMaxStreams] = {};
  int n = 0;
  double kernel_ms = 0.0;                             // of the chunks harvested so far
  ~Streams() {
    for (int i = 0; i < n; ++i) {
      (void)hipStreamSynchronize(s[i]);
      if (k0[i]) (void)hipEventDestroy(k0[i]);
      if (k1[i]) (void)hipEventDestroy(k1[i]);
      (void)hipStreamDestroy(s[i]);
    }
  }
  int create(prisim_ctx* ctx, int count, bool events) {
    for (int i = 0; i < count; ++i) {
      HIPCHK(ctx, hipStreamCreateWithFlags(&s[i], hipStreamNonBlocking));
      n = i + 1;
      if (events) {
        HIPCHK(ctx, hipEventCreate(&k0[i]));
        HIPCHK(ctx, hipEventCreate(&k1[i]));
      }
    }
    return PRISIM_OK;
  }
  // waits for the kernels of the chunk stream i ran last, if any, and adds their time (between k0 and k1) to kernel_ms
  int harvest(prisim_ctx* ctx, int i) {
    if (!timed[i]) return PRISIM_OK;
    HIPCHK(ctx, hipEventSynchronize(k1[i]));
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, k0[i], k1[i]) == hipSuccess) kernel_ms += ms;
    timed[i] = false;
    return PRISIM_OK;
  }
  int open(prisim_ctx* ctx, int i) {
    if (k0[i]) HIPCHK(ctx, hipEventRecord(k0[i], s[i]));
    return PRISIM_OK;
  }
  int close(prisim_ctx* ctx, int i) {
    if (k1[i]) HIPCHK(ctx, hipEventRecord(k1[i], s[i]));
    timed[i] = k1[i] != nullptr;
    return PRISIM_OK;
  }
  // every stream idle and harvested
  int drain(prisim_ctx* ctx) {
    for (int i = 0; i < n; ++i) {
      HIPCHK(ctx, hipStreamSynchronize(s[i]));
      if (int rc = harvest(ctx, i)) return rc;
    }
    return PRISIM_OK;
  }
};

// The frame of a chunk loop over the call's streams: the chunks `ch` of n items, `reps` times over (chunk c is chunk c % ch.count of
// repeat c / ch.count).  Chunk c goes to stream i = c % st.n: harvest(i) waits for the kernels of the chunk that last used the
// stream's buffers and books their time, then upload, open(i), kernels, close(i), download, each called as step(c, the chunk's
// items, i, st.s[i]) and returning 0 or a PRISIM_E* code, which ends the loop; drain() at the end.  A loop on one stream
// needs no drain() between chunks either: everything of a chunk is enqueued behind everything of the chunk before it, and that
// order alone protects the reused chunk buffers and the sums a kernel keeps on the device between chunks.
template <typename Upload, typename Kernels, typename Download>
inline int chunk_loop(prisim_ctx* ctx, Streams& st, const Chunks& ch, int64_t n, Upload&& upload, Kernels&& kernels, Download&& download,
                      int64_t reps = 1) {
  for (int64_t c = 0; c < reps * ch.count; ++c) {
    const int i = (int)(c % st.n);
    const Span sp = ch.span(c % ch.count, n);
    if (int rc = st.harvest(ctx, i)) return rc;
    if (int rc = upload(c, sp, i, st.s[i])) return rc;
    if (int rc = st.open(ctx, i)) return rc;
    if (int rc = kernels(c, sp, i, st.s[i])) return rc;
    if (int rc = st.close(ctx, i)) return rc;
    if (int rc = download(c, sp, i, st.s[i])) return rc;
  }
  return st.drain(ctx);
}

// a step of chunk_loop that has nothing to do
inline int no_step(int64_t, Span, int, hipStream_t) { return PRISIM_OK; }

// in-place fp64 1-D rocFFT plans by (inverse, batch) and one execution info per stream
struct FftPlans {
  std::map<std::pair<bool, size_t>, rocfft_plan> plans;
  rocfft_execution_info info[kMaxStreams] = {};
  ~FftPlans() {
    for (auto& kv : plans) g_rocfft.plan_destroy(kv.second);
    for (rocfft_execution_info i : info) if (i) g_rocfft.execution_info_destroy(i);
  }
  // the plan of (inverse, batch) on `buffer`, on the stream of info[i]
  int run(prisim_ctx* ctx, bool inverse, size_t batch, void* buffer, int i) const {
    void* b[1] = {buffer};
    const bool ok = g_rocfft.execute(plans.at({inverse, batch}), b, nullptr, info[i]) == rocfft_status_success;
    return ok ? PRISIM_OK : fail(ctx, PRISIM_ELIB, "rocfft_execute failed");
  }
  // plans of length len for every (inverse, batch) of want (repeats are made once); the infos run on streams[0 .. nstreams) and
  // each gets a work buffer from dev that serves the largest plan
  int create(prisim_ctx* ctx, Dev& dev, size_t len, const std::vector<std::pair<bool, size_t>>& want, const hipStream_t* streams,
             int nstreams) {
    RocfftApi& F = g_rocfft;
    size_t wmax = 0;
    for (const auto& key : want) {
      if (plans.count(key)) continue;
      rocfft_plan p = nullptr;
      if (F.plan_create(&p, rocfft_placement_inplace, key.first ? rocfft_transform_type_complex_inverse : rocfft_transform_type_complex_forward,
                        rocfft_precision_double, 1, &len, key.second, nullptr) != rocfft_status_success)
        return fail(ctx, PRISIM_ELIB, "rocfft_plan_create failed");
      plans[key] = p;
      size_t wb = 0;
      F.plan_get_work_buffer_size(p, &wb);
      wmax = std::max(wmax, wb);
    }
    for (int i = 0; i < nstreams; ++i) {
      if (F.execution_info_create(&info[i]) != rocfft_status_success) {
        info[i] = nullptr;
        return fail(ctx, PRISIM_ELIB, "rocfft_execution_info_create failed");
      }
      if (F.execution_info_set_stream(info[i], streams[i]) != rocfft_status_success)
        return fail(ctx, PRISIM_ELIB, "rocfft_execution_info_set_stream failed");
      if (wmax) {
        void* wb;
        DEV_ALLOC(ctx, dev, wb, wmax);
        if (F.execution_info_set_work_buffer(info[i], wb, wmax) != rocfft_status_success)
          return fail(ctx, PRISIM_ELIB, "rocfft_execution_info_set_work_buffer failed");
      }
    }
    return PRISIM_OK;
  }
};

// What a call owns on the device.  The buffers must outlive the streams that use them, and members go in reverse order: the
// streams are drained and destroyed first, then the plans, then the buffers are freed -- on every return path.  An entry that
// runs on the context's stream leaves st empty and synchronises that stream itself before it returns.
struct Work {
  Dev dev;
  FftPlans fft;
  Streams st;
};

// the four events of the entries that run on the context's stream: e[0] .. e[3] span the call, e[1] .. e[2] its kernels
struct Events {
  hipEvent_t e[4] = {};
  ~Events() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
  int create(prisim_ctx* ctx) {
    for (hipEvent_t& x : e) HIPCHK(ctx, hipEventCreate(&x));
    return PRISIM_OK;
  }
};

// rocFFT loaded and set up, once per process
inline int ensure_rocfft(prisim_ctx* ctx) {
  std::string lerr;
  if (!load_rocfft(lerr)) return fail(ctx, PRISIM_ELIB, lerr);
  if (!g_rocfft.setup_done) {
    if (g_rocfft.setup() != rocfft_status_success) return fail(ctx, PRISIM_ELIB, "rocfft_setup failed");
    g_rocfft.setup_done = true;
  }
  return PRISIM_OK;
}

// `kernel` in workgroups of kThreads, and what the launch itself reports
template <typename K, typename... A>
inline int launch(prisim_ctx* ctx, K kernel, dim3 grid, size_t lds, hipStream_t s, A... a) {
  hipLaunchKernelGGL(kernel, grid, dim3(kThreads), lds, s, a...);
  HIPCHK(ctx, hipGetLastError());
  return PRISIM_OK;
}

// workgroups of a grid-stride kernel over n elements
inline int grid_for(const prisim_ctx* ctx, int64_t n) {
  return (int)std::max<int64_t>(1, std::min<int64_t>((n + kThreads - 1) / kThreads, (int64_t)std::max(ctx->cu_count, 1) * 16));
}

// `rows` rows of `width` bytes between arrays whose rows are dpitch and spitch bytes apart
inline hipError_t copy_rows(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t rows, hipMemcpyKind kind,
                            hipStream_t s) {
  if (width == dpitch && width == spitch) return hipMemcpyAsync(dst, src, width * rows, kind, s);
  return hipMemcpy2DAsync(dst, dpitch, src, spitch, width, rows, kind, s);
}

using WallTime = std::chrono::steady_clock::time_point;
inline WallTime wall_now() { return std::chrono::steady_clock::now(); }
inline double wall_ms_since(WallTime t0) { return std::chrono::duration<double, std::milli>(wall_now() - t0).count(); }

// the LDS a workgroup may have on the context's device
inline int lds_limit(prisim_ctx* ctx, int& lds_max) {
  HIPCHK(ctx, hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->device));
  return PRISIM_OK;
}

// lets `kernel` take `bytes` of dynamic LDS: beyond 64 KiB a kernel has to be told
template <typename K>
inline int allow_lds(prisim_ctx* ctx, K* kernel, int64_t bytes) {
  if (bytes > 65536) HIPCHK(ctx, hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  return PRISIM_OK;
}

// resample_tables (addon_plan.h), a refusal as PRISIM_EINVAL; with rs_c, the coefficients under one scale for every term:
// rs_c [2][nout] = (map_w * scale) e^{-2 pi i k_in floor(m/2) / m}
inline int build_resample_tables(prisim_ctx* ctx, int64_t nout, int64_t m, int64_t nchan, double scale, int64_t nmap, const int64_t* map_out,
                                 const int64_t* map_in, const double* map_w, ResampleTables& t, std::vector<double>* rs_c) {
  if (const char* err = resample_tables(nout, m, nchan, nmap, map_out, map_in, map_w, t)) return fail(ctx, PRISIM_EINVAL, err);
  if (rs_c) rs_c->assign(t.phase.size(), 0.0);
  for (size_t at = 0; rs_c && at < t.in.size(); ++at) {
    if (t.in[at] < 0) continue;
    const double sc = t.w[at] * scale;
    (*rs_c)[2 * at] = sc * t.phase[2 * at];
    (*rs_c)[2 * at + 1] = sc * t.phase[2 * at + 1];
  }
  return PRISIM_OK;
}

// ---- device side: fp64 without contraction (the including files are built with -ffp-contract=off) -------------------------------

__device__ __forceinline__ double2 cadd(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ double2 csub(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ double2 cmul(double2 a, double2 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ double2 cmulc(double2 a, double2 b) { return make_double2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y); }   // a conj(b)
__device__ __forceinline__ double2 rmul(double2 a, double s) { return make_double2(a.x * s, a.y * s); }

// tw[k] = e^{+2 pi i k / m}, k < m / 2, by the whole workgroup (no barrier)
__device__ __forceinline__ void lds_twiddles(double2* tw, int m) {
  for (int k = threadIdx.x; k < m / 2; k += kThreads) {
    double sn, cs;
    sincospi(2.0 * (double)k / (double)m, &sn, &cs);
    tw[k] = make_double2(cs, sn);
  }
}

// n < 2^logm with its logm bits reversed
__device__ __forceinline__ int bitrev(int n, int logm) { return logm ? (int)(__brev((unsigned)n) >> (32 - logm)) : 0; }

// Radix-2 decimation-in-time butterflies with the twiddles e^{+2 pi i / m} over `tile` rows of m elements, ld apart, that were stored
// bit-reversed: sum_n x[n] e^{+2 pi i j n / m} in natural order.  By the whole workgroup, behind a barrier that the caller sets after
// its stores; ends with a barrier.
__device__ __forceinline__ void lds_ifft_dit(double2* buf, int ld, int tile, int m, const double2* tw) {
  const int half = m / 2;
  for (int h = 1; h < m; h <<= 1) {                 // butterflies of span 2h; twiddle W_{2h}^pos = tw[pos * m / (2h)]
    const int step = m / (2 * h);
    for (int i = threadIdx.x; i < tile * half; i += kThreads) {
      const int tt = tile == 1 ? 0 : i / half, ii = i - tt * half;   // one row: the compiler drops the division
      const int pos = ii & (h - 1);
      const int a = tt * ld + ((ii - pos) << 1) + pos, b = a + h;
      const double2 u = buf[a], v = cmul(buf[b], tw[pos * step]);
      buf[a] = cadd(u, v);
      buf[b] = csub(u, v);
    }
    __syncthreads();
  }
}

}  // namespace pint

#endif  // PRISIM_ADDON_INTERNAL_H
