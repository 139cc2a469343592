/*
 * prisim_cpxps.h -- cross power of closure-phase delay spectra on the GPU (libprisim_hip.so, prisim_amd/csrc_closure/cpxps.hip).
 *
 * The cross products of prisim/bispectrum_phase.py:ClosurePhaseDelaySpectrum.compute_power_spectrum (:3468-3551) and of
 * compute_power_spectrum_uncertainty: two stacks of delay spectra (nspw, LST bins, day bins or day-bin combinations, triads, lags) are
 * multiplied over pairs of LST bins, of day bins and of triads, and the pairs are collapsed again: a NaN-aware mean or median over the
 * LST bins, a trace along every diagonal for days and triads.  The uncollapsed product stays in device memory; only the collapsed
 * result is copied back.
 *
 * Conventions as in prisim_cpft.h: C-contiguous caller-owned host arrays, complex arrays interleaved (re, im), 0 or a negative
 * PRISIM_E* code, the message from prisim_hip_last_error().  The entry uses only the context's device; each call creates and destroys
 * its own streams and buffers.  The two inputs are uploaded once and lie outside `budget_bytes` (0: 1 GiB), which bounds the chunk
 * buffers; an input that does not fit on the device is PRISIM_ENOMEM.  fp64 throughout, no contraction.
 */
#ifndef PRISIM_CPXPS_H
#define PRISIM_CPXPS_H

#include <stdint.h>

#include "prisim_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* most LST bins a median is taken over */
#define PRISIM_CPXPS_MAX_MEDIAN 256

/* what becomes of an axis */
enum {
  PRISIM_CPXPS_NONE = 0,      /* not crossed: index i on both sides */
  PRISIM_CPXPS_FULL = 1,      /* crossed, every pair kept */
  PRISIM_CPXPS_COLLAPSE = 2   /* crossed and collapsed */
};

/* statistic of the LST collapse */
enum { PRISIM_CPXPS_MEAN = 0, PRISIM_CPXPS_MEDIAN = 1 };

typedef struct prisim_cpxps_stats {
  double wall_ms;          /* the whole call on the host clock, copies included */
  double kernel_ms;        /* the kernels of all chunks, from stream events */
  int64_t chunks;          /* chunks (one window, a range of lags) the call ran in */
  int64_t chunk_lags;      /* lags per full chunk */
  int64_t kernel_bytes;    /* bytes the kernels have to move: the inputs once, every buffer written once and read once by the next kernel */
  int64_t upload_bytes;    /* bytes copied to the device */
  int64_t download_bytes;  /* bytes copied back to the host */
  int64_t cross_bytes;     /* size of the uncollapsed product; with a collapsed axis it never leaves the device */
} prisim_cpxps_stats;

/* a, b      complex128 [nspw][n1][n2][n3][nlags]; b NULL: b = a.  Axes 1, 2, 3 are LST bins, day bins (or day-bin combinations), triads.
 * factor    float64 [nspw].
 * weights   NULL, or 3 pointers, one per axis: a complex128 vector of the axis' length or NULL (1).
 * modes     int32 [3], PRISIM_CPXPS_NONE / FULL / COLLAPSE per axis.
 * shifts    int64 [nshift], the LST shifts 0 <= s < n1; read when axis 1 is FULL or COLLAPSE (then nshift >= 1).
 * order     int32 [ncollapse], the collapsed axes (1, 2, 3) in the order in which they are collapsed: every axis in COLLAPSE once.
 * stat      the statistic of the LST collapse.
 *
 * With wa = (w1[i1] w2[i2]) w3[i3] at the indices of a, wb likewise at those of b, and numpy's complex product
 * (ar br - ai bi, ar bi + ai br) for every product, the real factor as factor + 0i:
 *   P = (factor (a wa)) conj(b wb)
 * Axis in NONE: index i on both sides.  Axes 2 and 3 in FULL: output axes (i, j), a at i, b at j.  Axis 1 in FULL: output axes
 * (shift, i), a at i, b at i - s, and NaN + NaN i where i < s.
 * Axes 2 and 3 in COLLAPSE: offsets k = -(n-1) .. n-1, out[k] = (sum over i of P[i, i+k]) / (n - |k|), summed in increasing i; NaN
 * propagates.  Axis 1 in COLLAPSE: over i, the mean or the median of the elements that are not NaN (an element is NaN when its real
 * or its imaginary part is; none left: NaN), which leaves [nshift].  The median orders by the real part, then the imaginary part, and
 * is the middle value or half the sum of the two middle ones; it takes at most PRISIM_CPXPS_MAX_MEDIAN LST bins.  The collapses are
 * applied in the given order.
 *
 * out       complex128 [nspw], then per axis [n] (NONE), [nshift][n1] or [n][n] (FULL), [nshift] or [2n-1] (COLLAPSE), then [nlags].
 *
 * Every reduction is sequential in a fixed order: the result does not depend on the chunks.  On an argument error (PRISIM_EINVAL)
 * nothing is written to out; a device error in a later chunk leaves the chunks before it written.  stats may be NULL. */
int prisim_cphase_xpower(prisim_ctx* ctx, int64_t nspw, int64_t n1, int64_t n2, int64_t n3, int64_t nlags, const double* a, const double* b,
                         const double* factor, const double* const* weights, const int32_t* modes, int64_t nshift, const int64_t* shifts,
                         int32_t ncollapse, const int32_t* order, int32_t stat, int64_t budget_bytes, double* out, prisim_cpxps_stats* stats);

#ifdef __cplusplus
}
#endif

#endif /* PRISIM_CPXPS_H */
