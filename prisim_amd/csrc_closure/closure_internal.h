// closure_internal.h -- the chunk loop of prisim_closure_phase (closure.hip) for code inside the library that consumes the phases of
// a chunk of triads where they lie on the device (cpdelay.hip).  Not part of the C-ABI.
#ifndef PRISIM_CLOSURE_INTERNAL_H
#define PRISIM_CLOSURE_INTERNAL_H

#include <hip/hip_runtime.h>

#include <cstdint>
#include <functional>

#include "../csrc_addon/addon_internal.h"
#include "../../include/prisim_closure.h"

// What follows the phases of a chunk.  The loop sizes its chunks so that its own buffers and bytes_per_triad of the sink's, per triad
// and stream, stay within the budget; then, once, prepare(triads per full chunk, triads of the last chunk, streams in use, the
// streams); per chunk, on the chunk's stream, kernels(stream index, stream, first triad, triads, the chunk's phases [tn][nchan][nt])
// inside the timed span and download(...) after the loop's own copies.  Each returns 0 or a PRISIM_E* code.  The streams are drained
// before closure_phase_chunks returns, on every path, so the sink's buffers must only outlive that call.
struct ClosureSink {
  int64_t bytes_per_triad = 0;
  std::function<int(int64_t tc, int64_t last, int nstreams, const hipStream_t* streams)> prepare;
  std::function<int(int i, hipStream_t s, int64_t T0, int64_t tn, const double* d_phase)> kernels;
  std::function<int(int i, hipStream_t s, int64_t T0, int64_t tn)> download;
};

// prisim_closure_phase's arguments and a sink (null: none).  With a sink, out_triplets and out_phase may each be null: not downloaded.
// The caller runs it inside guarded().
int closure_phase_chunks(prisim_ctx* ctx, const double* cube, int64_t nt, int64_t nbl, int64_t nchan, const int32_t* legs,
                         const int32_t* conj, int64_t ntriads, const double* freq_wts, const double* bpwts, const double* masks,
                         int64_t nmask, const int32_t* mask_index, int32_t route, int64_t budget_bytes, double* out_triplets,
                         double* out_phase, prisim_closure_stats* stats, const ClosureSink* sink);

#endif
