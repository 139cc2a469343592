/*
 * prisim_cpbins.h -- flagged binning of closure phases along the day or the LST axis on the GPU (libprisim_hip.so,
 * prisim_amd/csrc_closure/cpbins.hip).
 *
 * The per-bin arithmetic of prisim/bispectrum_phase.py:ClosurePhase.smooth_in_tbins (:1791-1797, :1816-1835, :1914-1933): for every
 * bin of one axis of a (n0, n1, ntriads, nchan) stack and every element of the other three axes, the sum of the weights, the phase of
 * the mean phasor, the phase of the component-wise median phasor, the masked standard deviation of the phases and the median absolute
 * deviation of the phases from the median phase.  The bins themselves (edges, reverse indices, array_split) are host work of
 * prisim_amd/bispectrum_phase.py and arrive as a CSR pair.
 *
 * Conventions as in prisim_closure.h: C-contiguous caller-owned host arrays, complex arrays interleaved (re, im), 0 or a negative
 * PRISIM_E* code, the message from prisim_hip_last_error().  The entry uses only the context's device; each call creates and destroys
 * its own stream and chunk buffers and streams the triad axis in chunks whose buffers take no more than `budget_bytes` of device
 * memory (0: 1 GiB).  Resident stacks (below) lie outside that budget.  fp64 throughout.
 */
#ifndef PRISIM_CPBINS_H
#define PRISIM_CPBINS_H

#include <stdint.h>

#include "prisim_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* largest number of members of one bin.  The medians are selected by rank counting, n^2 steps per output element for a bin of n
 * members; the reference's bins are tens of members. */
#define PRISIM_CPBINS_MAX_BIN 256

/* input kinds */
enum {
  PRISIM_CPBINS_PHASE_FLAGS = 0,   /* phases and uint8 flags (nonzero: flagged): the native stack.  A member's weight is 1, or 0 when flagged */
  PRISIM_CPBINS_BINNED = 1         /* mean phases, median phases and weights of an earlier pass; a member is masked where its weight <= 0 */
};

/* bits of `want`: the outputs copied to the host */
enum {
  PRISIM_CPBINS_WTS = 1,           /* out_wts          float64 */
  PRISIM_CPBINS_EICP_MEAN = 2,     /* out_eicp_mean    complex128 */
  PRISIM_CPBINS_EICP_MEDIAN = 4,   /* out_eicp_median  complex128 */
  PRISIM_CPBINS_CP_MEAN = 8,       /* out_cp_mean      float64 */
  PRISIM_CPBINS_CP_MEDIAN = 16,    /* out_cp_median    float64 */
  PRISIM_CPBINS_RMS = 32,          /* out_rms          float64 */
  PRISIM_CPBINS_MAD = 64,          /* out_mad          float64 */
  PRISIM_CPBINS_ALL = 127
};

/* a stack that stays on the device between calls: the uploaded input of a call, or the (mean phase, median phase, weights) a call
 * produced, of kind PRISIM_CPBINS_BINNED.  It belongs to the context it was made on and must be freed before it. */
typedef struct prisim_cphase_stack prisim_cphase_stack;

typedef struct prisim_cpbins_stats {
  double wall_ms;          /* the whole call on the host clock, copies included */
  double kernel_ms;        /* the kernels of all chunks, from stream events */
  int64_t elements;        /* output elements per output array */
  int64_t chunks;          /* chunks the triad axis was streamed in */
  int64_t chunk_triads;    /* triads per full chunk */
  int64_t kernel_bytes;    /* bytes the kernel has to move to and from device memory: every input element once, every output once */
  int64_t upload_bytes;    /* bytes copied to the device (a resident input is not copied) */
  int64_t download_bytes;  /* bytes copied back to the host */
  int32_t max_bin;         /* members of the largest bin */
  int32_t resident_in;     /* 1: the input was read from a resident stack */
} prisim_cpbins_stats;

/* Bins of axis `axis` (0 or 1) of a stack [n0][n1][ntriads][nchan].  Bin k has the members members[offsets[k]] ... members[offsets[k+1]-1],
 * indices on that axis, in that order (offsets [nbins+1] int64 from 0, non-decreasing; members int32; an empty bin is allowed; no bin
 * above PRISIM_CPBINS_MAX_BIN members).  The outputs have the stack's shape with `axis` replaced by nbins.
 *
 * Input, one of
 *   kind PHASE_FLAGS: in_mean = the phases (radians) float64, in_flags uint8; in_median, in_wts ignored.  pm = pd = the phase.
 *   kind BINNED:      in_mean, in_median, in_wts float64; in_flags ignored.  pm = the mean phase, pd = the median phase.
 *   *resident_in != NULL: that stack (kind, n0, n1, ntriads, nchan must be its own); the host inputs are ignored.
 *   resident_in != NULL and *resident_in == NULL: the host inputs are uploaded whole, and *resident_in receives the stack.
 * For every output element, with U the unmasked members of its bin in bin order and n = |U|:
 *   wts        = sum over ALL members of the member's weight, in bin order
 *   z_mean     = (sum_U cos pm, sum_U sin pm) / n, sums in bin order;  a_mean = atan2(Im z_mean, Re z_mean)
 *   z_median   = (median_U cos pd, median_U sin pd);                    a_median = atan2(Im z_median, Re z_median)
 *                a median is the middle value, or half the sum of the two middle values when n is even
 *   eicp_x     = (cos a_x, sin a_x) of one sincos;  cp_x = atan2(sin a_x, cos a_x)        (x = mean, median)
 *   rms        = sqrt(sum_U (pm - mu)^2 / n), mu = (sum_U pm) / n: the two-pass population deviation
 *   mad        = median over U of |pd - cp_median|, not wrapped; with mad_ignores_flags != 0 the median is over all members of the bin
 * Where n = 0 (every member masked, or an empty bin): eicp_mean = eicp_median = 1 + 0i and cp_mean = cp_median = rms = mad = 0.
 * Phases must be finite, also under the flags.
 *
 * Outputs: each out_* is written when its bit is in `want` (it must then not be NULL).  keep_out != NULL: cp_mean, cp_median and wts
 * also stay on the device as a new stack of kind BINNED, *keep_out; with want = 0 nothing is copied back.  nbins = 0 with want = 0 and
 * keep_out = NULL only uploads (resident_in).  On an error nothing is written to the outputs and no stack is made.  stats may be NULL. */
int prisim_cphase_bin(prisim_ctx* ctx, int32_t kind, const double* in_mean, const double* in_median, const double* in_wts,
                      const uint8_t* in_flags, int64_t n0, int64_t n1, int64_t ntriads, int64_t nchan, int32_t axis, int64_t nbins,
                      const int64_t* offsets, const int32_t* members, int32_t want, int32_t mad_ignores_flags, int64_t budget_bytes,
                      prisim_cphase_stack** resident_in, prisim_cphase_stack** keep_out, double* out_wts, double* out_eicp_mean,
                      double* out_eicp_median, double* out_cp_mean, double* out_cp_median, double* out_rms, double* out_mad,
                      prisim_cpbins_stats* stats);

/* frees a resident stack (NULL: nothing) */
void prisim_cphase_stack_free(prisim_cphase_stack* stack);

#ifdef __cplusplus
}
#endif

#endif /* PRISIM_CPBINS_H */
