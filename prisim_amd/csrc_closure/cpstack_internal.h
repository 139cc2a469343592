// cpstack_internal.h -- what cpbins.hip and cpdiff.hip share: the resident stack of closure phases (include/prisim_cpbins.h declares
// it opaque) and the per-call device buffers, stream and pitched copies of their chunk loops.  Not part of the public ABI.
#ifndef PRISIM_CPSTACK_INTERNAL_H
#define PRISIM_CPSTACK_INTERNAL_H

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "../csrc/ctx_internal.h"
#include "../../include/prisim_cpbins.h"

struct prisim_cphase_stack {
  int device = 0;
  int32_t kind = 0;
  int64_t n0 = 0, n1 = 0, nt = 0, nc = 0;
  double* a = nullptr;       // the phases (PHASE_FLAGS) or the mean phases (BINNED)
  double* b = nullptr;       // BINNED: the median phases
  double* w = nullptr;       // BINNED: the weights
  uint8_t* f = nullptr;      // PHASE_FLAGS: the flags
  ~prisim_cphase_stack() {
    if (a) (void)hipFree(a);
    if (b) (void)hipFree(b);
    if (w) (void)hipFree(w);
    if (f) (void)hipFree(f);
  }
};

namespace cpint {

constexpr int64_t kDefaultBudget = int64_t(1) << 30;
constexpr int64_t kMaxBlocks = int64_t(1) << 20;

struct Dev {
  std::vector<void*> ptrs;
  ~Dev() { for (void* p : ptrs) (void)hipFree(p); }
};

#define CB_ALLOC(ctx, dev, ptr, bytes)                                                                 \
  do {                                                                                                 \
    void* p_ = nullptr;                                                                                \
    HIPCHK(ctx, hipMalloc(&p_, std::max<size_t>((size_t)(bytes), 16)));                                \
    (dev).ptrs.push_back(p_);                                                                          \
    (ptr) = reinterpret_cast<decltype(ptr)>(p_);                                                       \
  } while (0)

// the call's stream and its timing events: drained before the buffers it uses are freed (declared after them)
struct Stream {
  hipStream_t s = nullptr;
  hipEvent_t k0 = nullptr, k1 = nullptr;
  ~Stream() {
    if (s) (void)hipStreamSynchronize(s);
    if (k0) (void)hipEventDestroy(k0);
    if (k1) (void)hipEventDestroy(k1);
    if (s) (void)hipStreamDestroy(s);
  }
};

// `rows` rows of `width` bytes between arrays whose rows are dpitch and spitch bytes apart
inline hipError_t copy_rows(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t rows, hipMemcpyKind kind,
                            hipStream_t s) {
  if (width == dpitch && width == spitch) return hipMemcpyAsync(dst, src, width * rows, kind, s);
  return hipMemcpy2DAsync(dst, dpitch, src, spitch, width, rows, kind, s);
}

}  // namespace cpint

#endif  // PRISIM_CPSTACK_INTERNAL_H
