/*
 * prisim_clean.h -- delay-spectrum CLEAN on the GPU (libprisim_hip.so, prisim_amd/csrc_clean/).
 *
 * Hogbom CLEAN of complex 1-D rows as prisim/delay_spectrum.py:complex1dClean (:133-352), and the chain of
 * DelaySpectrum.delayClean (:1622-1838) around it: padded inverse FFT to lags, CLEAN of every (baseline, snapshot) row,
 * forward FFTs of the clean components and residuals.  Conventions as in prisim_hip.h: C-contiguous caller-owned host
 * arrays, complex arrays interleaved (re, im), 0 or a negative PRISIM_E* code, the message from prisim_hip_last_error().
 * These entries use only the context's device and stream; each allocates its own device scratch for the call.
 */
#ifndef PRISIM_CLEAN_H
#define PRISIM_CLEAN_H

#include <stdint.h>

#include "prisim_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* longest row (lag count M) the CLEAN kernel takes */
#define PRISIM_CLEAN_MAX_LEN 4096

/* bits of the per-row flags */
enum {
  PRISIM_CLEAN_THRESHOLD = 1,       /* cond1: |maxres| <= lolim * max|inp| at the last iteration */
  PRISIM_CLEAN_MAXITER = 2,         /* cond2: itr >= maxiter */
  PRISIM_CLEAN_INRMS = 4,           /* cond3: inrms <= outrms at the last iteration */
  PRISIM_CLEAN_NO_OUTRMS = 8,       /* <= 2 entries outside the box: outrms is undefined (the reference's None), cond3 false */
  PRISIM_CLEAN_BAD_THRESHOLD = 16   /* lolim >= 1 on this row (:216-217): the row was not cleaned */
};

typedef struct prisim_clean_stats {
  double device_ms;          /* wall time of the call's device work (events on the context stream) */
  double clean_ms;           /* the CLEAN kernel alone */
  int64_t sum_iter;          /* iterations summed over every row */
  int64_t rows;              /* rows cleaned */
  int32_t waves_per_block;   /* rows in flight per workgroup (one wave64 per row) */
  int32_t kernel_in_lds;     /* 1: the one deconvolving kernel was held in LDS; 0: read from global memory */
  int64_t lds_bytes;         /* dynamic LDS per workgroup */
} prisim_clean_stats;

/* CLEAN `nrows` rows of length m (<= PRISIM_CLEAN_MAX_LEN).
 *   inp     [nrows][m] complex128
 *   kern    [nkern][m] complex128 deconvolving kernels (not normalised: each is divided by its max modulus here, :206-207)
 *   kidx    [nrows] int32 kernel of every row, or NULL when nkern == 1
 *   cbox    [nrows][m] uint8 clean box (nonzero = searched)
 *   threshold_absolute: 0 lolim = threshold, 1 lolim = threshold / max|inp| per row
 * Outputs: cc, res [nrows][m] complex128; iters, flags [nrows] int32; rms [nrows][2] float64 (final inrms, outrms; NaN where
 * undefined).  stats may be NULL. */
int prisim_clean_rows(prisim_ctx* ctx, int64_t nrows, int64_t m, const double* inp, int64_t nkern, const double* kern,
                      const int32_t* kidx, const uint8_t* cbox, double gain, int64_t maxiter, double threshold,
                      int32_t threshold_absolute, double* cc, double* res, int32_t* iters, int32_t* flags, double* rms,
                      prisim_clean_stats* stats);

/* The delayClean chain for `ncubes` cubes of `nrows` windowed rows of `nchan` channels each, zero-padded to m lags:
 *   win     [ncubes][nrows][nchan] complex128: visibilities x bandpass x window (:1738-1739)
 *   kwin    [nkern][nchan] complex128: bandpass x window of every distinct kernel (:1740); kidx [nrows] or NULL (nkern == 1)
 *   cbox    [nrows][m] uint8, shared by the cubes
 *   lag_scale = df: lags = df * sum_n x[n] e^{+2 pi i k n / m} (= m df ifft, :1738-1740)
 *   freq_scale1, freq_scale2: the forward FFTs are multiplied by freq_scale1 then freq_scale2 (deta, pad_factor, :1808-1811)
 * Outputs (unshifted, lag order of fftfreq(m)): lag [ncubes][nrows][m], kern_lag [nkern][m], cc, res, cc_freq, res_freq
 * [ncubes][nrows][m] complex128; iters, flags [ncubes][nrows]; rms [ncubes][nrows][2]. */
int prisim_clean_delay(prisim_ctx* ctx, int32_t ncubes, int64_t nrows, int64_t nchan, int64_t m, const double* win, int64_t nkern,
                       const double* kwin, const int32_t* kidx, const uint8_t* cbox, double lag_scale, double freq_scale1,
                       double freq_scale2, double gain, int64_t maxiter, double threshold, int32_t threshold_absolute, double* lag,
                       double* kern_lag, double* cc, double* res, double* cc_freq, double* res_freq, int32_t* iters, int32_t* flags,
                       double* rms, prisim_clean_stats* stats);

#ifdef __cplusplus
}
#endif

#endif /* PRISIM_CLEAN_H */
