/*
 * prisim_cpavg.h -- incoherent averages of closure-phase power spectra on the GPU (libprisim_hip.so, prisim_amd/csrc_closure/cpavg.hip).
 *
 * The sums of prisim/bispectrum_phase.py:incoherent_cross_power_spectrum_average (:1116-1119, :1169-1195) and of
 * incoherent_kbin_averaging (:1479-1486): the weighted average of the cross-power spectra of several data sets and of chosen diagonals
 * of their collapsed axes, and the averages of a power spectrum in bins of |k_parallel|.
 *
 * Conventions as in prisim_cpxps.h: C-contiguous caller-owned host arrays, complex arrays interleaved (re, im), 0 or a negative
 * PRISIM_E* code, the message from prisim_hip_last_error().  The entries use only the context's device; each call creates and destroys
 * its own streams and buffers.  The inputs are uploaded once and lie outside `budget_bytes` (0: 1 GiB), which bounds the chunk buffers;
 * an input that does not fit on the device is PRISIM_ENOMEM.  fp64 throughout, no contraction, no atomics.  Every reduction is
 * sequential in the order stated below: the result does not depend on the chunks or on the grid.  On an argument error (PRISIM_EINVAL)
 * nothing is written to any output; a device error in a later chunk leaves the chunks before it written.  stats may be NULL.
 */
#ifndef PRISIM_CPAVG_H
#define PRISIM_CPAVG_H

#include <stdint.h>

#include "prisim_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* axes of an array of prisim_cphase_xavg */
#define PRISIM_CPAVG_MIN_DIM 5
#define PRISIM_CPAVG_MAX_DIM 8

/* routes of prisim_cphase_kbin */
enum {
  PRISIM_CPAVG_AUTO = -1,     /* LDS when a row fits, else GLOBAL */
  PRISIM_CPAVG_LDS = 0,       /* whole rows staged in LDS with coalesced loads, the members walked from there */
  PRISIM_CPAVG_GLOBAL = 1     /* the members read from global memory */
};

typedef struct prisim_cpavg_stats {
  double wall_ms;          /* the whole call on the host clock, copies included */
  double kernel_ms;        /* the kernels of all chunks, from stream events */
  int64_t chunks;          /* chunks the call ran in (xavg: ranges of lags; kbin: one window, a range of rows) */
  int64_t kernel_bytes;    /* bytes the kernels have to move: the inputs once, every buffer written once and read once by the next kernel */
  int64_t upload_bytes;    /* bytes copied to the device */
  int64_t download_bytes;  /* bytes copied back to the host */
  int32_t route;           /* kbin: the route taken, PRISIM_CPAVG_LDS or PRISIM_CPAVG_GLOBAL; xavg: PRISIM_CPAVG_AUTO */
  int32_t lds_limit;       /* kbin: the LDS bytes a workgroup may have on this device (a row of 16 nlags bytes has to fit); xavg: 0 */
} prisim_cpavg_stats;

/* The average of nsets arrays under weights, and averages of that over chosen positions of chosen axes.
 *
 * ndim, shape   PRISIM_CPAVG_MIN_DIM <= ndim <= PRISIM_CPAVG_MAX_DIM; axis 0 is the spectral window, the last axis the lags.
 * arrays        nsets >= 1 pointers, each complex128 of `shape`.
 * weights       nsets pointers, each float64 of the shape wshapes[set][ndim]: every extent is 1 or the array's, the last is 1.
 *               With U the shape that is, per axis, the largest of the sets' weight extents, every weight is read as broadcast to U.
 * reduce        int32 [ncombo][ndim], non-zero where the combination reduces the axis; never axis 0 or the lags.
 * masks         ncombo * ndim pointers; masks[c * ndim + x] is, for a reduced axis, uint8 [shape[x]], non-zero at the selected
 *               positions (at least one); it is not read for the other axes.
 *
 * Stage 1, per element e (u its position in U):
 *   num = sum over the sets i, in order, of (re a_i[e] w_i[u], im a_i[e] w_i[u]); a product with NaN in either part counts as 0 + 0i
 *   den = sum over the sets i, in order, of w_i[u]; a NaN weight counts as 0
 *   avg[e] = (re num / den, im num / den), wsum[u] = den
 * so an element that is NaN in one set contributes nothing to num while its weight still counts in den.
 * Stage 2, per combination c, over the outer product of the selected positions of its reduced axes, in increasing flattened index
 * (W = wsum broadcast to `shape`):
 *   wout[c] = sum of W,  out[c] = (sum of (re avg W, im avg W)) / wout[c]
 * NaN propagates here.  Reduced axes keep the length 1.
 *
 * avg           complex128 of `shape`, or NULL: then it is not copied back.
 * wsum          float64 of the shape U, or NULL.
 * out           ncombo pointers, each complex128 of `shape` with the reduced axes at 1.
 * wout          ncombo pointers, each float64 of the shape U with the reduced axes at 1.
 *
 * A chunk is a range of lags; per lag the chunk buffers take 16 (E + sum over c of E_c) bytes on each of two streams, E the elements
 * of an array per lag and E_c those of out[c]. */
int prisim_cphase_xavg(prisim_ctx* ctx, int32_t ndim, const int64_t* shape, int64_t nsets, const double* const* arrays,
                       const double* const* weights, const int64_t* wshapes, int32_t ncombo, const int32_t* reduce,
                       const uint8_t* const* masks, int64_t budget_bytes, double* avg, double* wsum, double* const* out, double* const* wout,
                       prisim_cpavg_stats* stats);

/* Averages of a power spectrum in bins of |k_parallel|.
 *
 * p             complex128 [nspw][m][nlags].
 * kprll         float64 [nspw][nlags].
 * offsets       int64 [nspw][nk + 1], per window the CSR offsets of its nk >= 1 bins: offsets[w][0] = 0, not decreasing.
 * members       int32, the windows' members one window after the other (window w has offsets[w][nk] of them): lag indices
 *               0 <= j < nlags, strictly increasing within a bin.
 * route         PRISIM_CPAVG_AUTO, _LDS (PRISIM_EINVAL when a row of 16 nlags bytes exceeds the LDS of a workgroup) or _GLOBAL.
 *
 * Per window w, row r and bin b, walking the bin's members j in order, with k_j = |kprll[w][j]| and p_j = p[w][r][j] (a complex
 * number is NaN when its real or its imaginary part is):
 *   ps   = (sum of the p_j that are not NaN) / their number
 *   del2 = ((sum of the (k3 re p_j, k3 im p_j) that are not NaN, k3 = (k_j k_j) k_j) / their number) / (2 pi^2)
 *   kc   = (sum of the k_j |p_j| that are not NaN) / (sum of the |p_j| that are not NaN), |p_j| = hypot(re p_j, im p_j)
 * Nothing left to sum gives 0 / 0 = NaN; an empty bin is NaN in all three.  Both routes do the same arithmetic in the same order and
 * agree bit for bit.
 *
 * ps, del2      complex128 [nspw][m][nk].
 * kc            float64 [nspw][m][nk].
 *
 * A chunk is one window and a range of its rows; per row the chunk buffers take 40 nk bytes on each of two streams. */
int prisim_cphase_kbin(prisim_ctx* ctx, int64_t nspw, int64_t m, int64_t nlags, int64_t nk, const double* p, const double* kprll,
                       const int64_t* offsets, const int32_t* members, int32_t route, int64_t budget_bytes, double* ps, double* del2,
                       double* kc, prisim_cpavg_stats* stats);

#ifdef __cplusplus
}
#endif

#endif /* PRISIM_CPAVG_H */
