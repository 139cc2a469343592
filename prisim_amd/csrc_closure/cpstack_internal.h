// cpstack_internal.h -- what cpbins.hip and cpdiff.hip share: the resident stack of closure phases (include/prisim_cpbins.h declares
// it opaque).  Not part of the public ABI.
#ifndef PRISIM_CPSTACK_INTERNAL_H
#define PRISIM_CPSTACK_INTERNAL_H

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../csrc_addon/addon_internal.h"
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

#endif  // PRISIM_CPSTACK_INTERNAL_H
