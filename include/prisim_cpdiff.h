/*
 * prisim_cpdiff.h -- differences of day sub-samples of binned closure phases on the GPU (libprisim_hip.so,
 * prisim_amd/csrc_closure/cpdiff.hip).
 *
 * The last step of prisim/bispectrum_phase.py:ClosurePhase.subsample_differencing (:2209-2249): for every pair of disjoint pairs
 * {i, j}, {k, m} of day bins of a day- and LST-binned stack (n0, n1, ntriads, nchan), the half differences of the unit phasors of the
 * two bins of each pair, the root of the sum of their squared weights, and the mask.  The day and the LST binning before it are
 * prisim_cphase_bin (prisim_cpbins.h), whose kept stack this entry reads where it lies; the list of pairs of pairs is host work of
 * prisim_amd/bispectrum_phase.py.
 *
 * Conventions as in prisim_cpbins.h: C-contiguous caller-owned host arrays, complex arrays interleaved (re, im), 0 or a negative
 * PRISIM_E* code, the message from prisim_hip_last_error().  The entry uses only the context's device; each call creates and destroys
 * its own stream and chunk buffers and streams the triad axis in chunks whose buffers take no more than `budget_bytes` of device
 * memory (0: 1 GiB).  A resident input lies outside that budget.  fp64 throughout.
 */
#ifndef PRISIM_CPDIFF_H
#define PRISIM_CPDIFF_H

#include <stdint.h>

#include "prisim_cpbins.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct prisim_cpdiff_stats {
  double wall_ms;          /* the whole call on the host clock, copies included */
  double kernel_ms;        /* the kernels of all chunks, from stream events */
  int64_t elements;        /* output elements per output array: n0 * ncomb * ntriads * nchan */
  int64_t chunks;          /* chunks the triad axis was streamed in */
  int64_t chunk_triads;    /* triads per full chunk */
  int64_t kernel_bytes;    /* bytes the kernel has to move to and from device memory: every input element once, every output once */
  int64_t upload_bytes;    /* bytes copied to the device (a resident input is not copied) */
  int64_t download_bytes;  /* bytes copied back to the host */
  int32_t resident_in;     /* 1: the input was read from a resident stack */
  int32_t ncomb;           /* pairs of pairs */
} prisim_cpdiff_stats;

/* bytes of the eight outputs per output element: four complex128, two float64, two uint8 */
#define PRISIM_CPDIFF_OUT_BYTES 82

/* Input, a stack [n0][n1][ntriads][nchan] of mean phases, median phases (radians) and weights, one of
 *   resident != NULL: that stack; it must be of kind PRISIM_CPBINS_BINNED, of this shape and on the context's device (as left by
 *                     prisim_cphase_bin(..., keep_out)); the host inputs are ignored.
 *   resident == NULL: in_mean, in_median, in_wts float64, uploaded by the entry chunk by chunk.
 * pairs: int32 [ncomb][4] = (i, j, k, m), indices on axis 1, ncomb >= 1, every index in [0, n1), i != j and k != m.
 *
 * Every output has the shape [n0][ncomb][ntriads][nchan].  For g in {0, 1} with (a, b) = (i, j) for g = 0 and (k, m) for g = 1, and
 * x in {mean, median}, for every element of the other three axes:
 *   mask_g   = !(w[a] > 0) || !(w[b] > 0)                               uint8, 1: masked
 *   wts_g    = sqrt(w[b]^2 + w[a]^2)                                     written always, also under the mask (the reference's .data, :2233)
 *   diff_g_x = 0.5 * ((cos p_x[b], sin p_x[b]) - (cos p_x[a], sin p_x[a])), one sincos per member, subtracted component by component
 * Under the mask diff_g_x = 0 + 0i.  The reference leaves the values under its mask unspecified (MA.empty filled from arrays whose
 * own masked values are unspecified); 0 is the reading of its commented-out .filled(0.0) at :2728.  The masks are the reference's.
 * A phase under the mask reaches no output.
 *
 * All eight outputs are required.  On an argument error (PRISIM_EINVAL) nothing is written to them; a device
 * error in a later chunk leaves the chunks before it written.  stats may be NULL. */
int prisim_cphase_diff(prisim_ctx* ctx, const double* in_mean, const double* in_median, const double* in_wts, int64_t n0, int64_t n1,
                       int64_t ntriads, int64_t nchan, prisim_cphase_stack* resident, int64_t ncomb, const int32_t* pairs,
                       int64_t budget_bytes, double* out_diff0_mean, double* out_diff0_median, double* out_diff1_mean,
                       double* out_diff1_median, double* out_wts0, double* out_wts1, uint8_t* out_mask0, uint8_t* out_mask1,
                       prisim_cpdiff_stats* stats);

#ifdef __cplusplus
}
#endif

#endif /* PRISIM_CPDIFF_H */
