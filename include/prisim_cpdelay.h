/*
 * prisim_cpdelay.h -- delay spectra of closure phases and their power spectra on the GPU (libprisim_hip.so,
 * prisim_amd/csrc_closure/cpdelay.hip).
 *
 * prisim_closure_delay_spectra is the transform of prisim/delay_spectrum.py:DelaySpectrum.subband_delay_transform_closure_phase
 * (:2932-2962): the sub-band delay transform of exp(-i phi) for every triad, snapshot and frequency window, oversampled and FFT-resampled
 * (DSP.downsampler read as scipy.signal.resample, prisim_amd/dsp_readings.py).  prisim_closure_power is the arithmetic of
 * DelayPowerSpectrum.compute_individual_closure_phase_power_spectrum (:4346) and compute_averaged_closure_phase_power_spectrum
 * (:4536-4538).
 *
 * Conventions as in prisim_closure.h and prisim_runs.h: C-contiguous caller-owned host arrays, complex arrays interleaved (re, im), 0 or
 * a negative PRISIM_E* code, the message from prisim_hip_last_error().  The entries use only the context's device; each call creates and
 * destroys its own streams and device buffers and streams its rows in chunks whose buffers take no more than `budget_bytes` of device
 * memory (0: 1 GiB).  fp64 throughout.
 */
#ifndef PRISIM_CPDELAY_H
#define PRISIM_CPDELAY_H

#include <stdint.h>

#include "prisim_closure.h"

#ifdef __cplusplus
extern "C" {
#endif

/* longest oversampled (m) and resampled (nres) spectrum: the sub-band limit */
#define PRISIM_CPDELAY_MAX_LEN 4096

/* bits of `want` of prisim_closure_delay_spectra (those of prisim_subband.h) */
enum {
  PRISIM_CPDELAY_OVER = 1,          /* the m-lag oversampled spectra */
  PRISIM_CPDELAY_OVER_POWER = 2,    /* |oversampled|^2 * pscale[w] */
  PRISIM_CPDELAY_RES = 4,           /* the nres-lag FFT-resampled spectra */
  PRISIM_CPDELAY_RES_POWER = 8      /* |resampled|^2 * pscale[w] */
};

/* routes of the oversampled transform.  AUTO takes the fused LDS kernel when m is a power of two and a row fits in LDS (on gfx950 every
 * m up to PRISIM_CPDELAY_MAX_LEN does), rocFFT between a prepare and a finish kernel otherwise.  The resampled spectra are formed by one
 * kernel on either route. */
enum { PRISIM_CPDELAY_AUTO = -1, PRISIM_CPDELAY_FUSED = 0, PRISIM_CPDELAY_ROCFFT = 1 };

/* bits of `want` of prisim_closure_power */
enum { PRISIM_CPPOWER_INDIVIDUAL = 1, PRISIM_CPPOWER_AUTO = 2, PRISIM_CPPOWER_CROSS = 4 };

typedef struct prisim_cpdelay_stats {
  double wall_ms;          /* the whole call on the host clock, copies included */
  double kernel_ms;        /* the kernels (and rocFFT) of all chunks, from stream events; from a cube: the phase kernels too */
  int64_t rows;            /* rows (triads) transformed; prisim_closure_power: entries of axis 0 */
  int64_t chunks;          /* chunks the call was streamed in */
  int64_t chunk_rows;      /* rows per full chunk */
  int64_t upload_bytes;    /* bytes copied to the device, counted from the algorithm (a resident cube is not copied) */
  int64_t download_bytes;  /* bytes copied back to the host */
  int32_t route;           /* PRISIM_CPDELAY_FUSED or PRISIM_CPDELAY_ROCFFT; prisim_closure_power: 0 */
  int32_t phase_route;     /* from a cube: the PRISIM_CLOSURE_* route that formed the phases; from phases: -1 */
  int32_t streams;         /* streams the chunks were spread over */
  int32_t tile;            /* FUSED: snapshots per workgroup */
  int32_t lds_bytes;       /* FUSED: dynamic LDS per workgroup; ROCFFT: that of the turning kernels */
  int32_t reserved_;
} prisim_cpdelay_stats;

/* Delay spectra of the closure phases of `nrows` rows, nchan channels, nt snapshots.  The phases are one of
 *   phases   host [nrows][nchan][nt] float64 (radians; nrows is the product of all leading axes of the caller's array); cube, legs,
 *            conj, freq_wts, bpwts, masks, mask_index are then ignored and nbl, nmask may be 0; or
 *   phases == NULL: the closure phases of `nrows` triads of a cube, formed on the device by the code of prisim_closure_phase from
 *            exactly its arguments (cube or NULL for the resident slots, nbl, legs, conj, freq_wts, bpwts, masks, nmask, mask_index and
 *            phase_route = its `route`), and transformed where they lie.  The triplets are never downloaded; the phases are downloaded
 *            only when out_phase [nrows][nchan][nt] is not NULL.
 * For every row T, snapshot t and window w of wts [nwin][nchan], with M = m lags (nchan <= m <= PRISIM_CPDELAY_MAX_LEN):
 *   x[ch]          = exp(-i phi[T][ch][t]) * wts[w][ch], zero-padded to m; the phasor is (cos phi, -sin phi) of one sincos
 *   oversampled[j] = m df fftshift(ifft(x))[j]
 *   resampled      = scipy.signal.resample(oversampled, nres) (1 <= nres <= PRISIM_CPDELAY_MAX_LEN), formed from x directly as
 *                    prisim_subband.h describes, with the selection map (nmap, map_out, map_in, map_w) of
 *                    prisim_amd/dsp_readings.py:resample_map(m, nres)
 * Outputs, each NULL unless its bit is in `want`: over [nrows][nwin][m][nt] complex128, res [nrows][nwin][nres][nt] complex128 -- the
 * reference's layouts, snapshot fastest, each element written once -- and over_pow / res_pow, float64 of the same shapes,
 * |.|^2 * pscale[w] (pscale [nwin], needed with either power bit).
 *
 * Where a bispectrum is exactly zero (a flagged channel) prisim_closure_phase promises a finite phase only (0 or +-pi, by the signs of
 * the zeros).  This entry inherits that: the phase prisim_closure_phase would write for such a point is the phase that is transformed,
 * on both input forms, so both give the same spectra for the same phases; numpy's angle() of a bispectrum formed differently may
 * choose the other value there.
 * route: PRISIM_CPDELAY_AUTO or the route itself.  stats may be NULL. */
int prisim_closure_delay_spectra(prisim_ctx* ctx, const double* phases, int64_t nrows, const double* cube, int64_t nt, int64_t nbl,
                                 int64_t nchan, const int32_t* legs, const int32_t* conj, const double* freq_wts, const double* bpwts,
                                 const double* masks, int64_t nmask, const int32_t* mask_index, int32_t phase_route, int32_t nwin,
                                 const double* wts, int64_t m, double df, int64_t nres, int64_t nmap, const int64_t* map_out,
                                 const int64_t* map_in, const double* map_w, const double* pscale, int32_t want, int32_t route,
                                 int64_t budget_bytes, double* out_phase, double* over, double* over_pow, double* res, double* res_pow,
                                 prisim_cpdelay_stats* stats);

/* Power spectra of closure-phase delay spectra x [n0][nwin][inner] complex128 (inner = nlags * nt) with scale [nwin]; any of
 *   PRISIM_CPPOWER_INDIVIDUAL  out_individual [n0][nwin][inner] = |x|^2 * scale[w]; |.|^2 is re^2 + im^2 throughout (within 2 u of the exact value;
 *                              numpy's abs(.)**2, a squared hypot, may differ from it by a few u)
 *   PRISIM_CPPOWER_AUTO        out_auto [nwin][inner] = ((sum over axis 0 of |x|^2) / n0) * scale[w]
 *   PRISIM_CPPOWER_CROSS       out_cross [nwin][inner] = (1 / (n0 (n0 - 1))) * (scale[w] |sum over axis 0 of x|^2 - n0 auto); n0 >= 2
 * float64.  Axis 0 is streamed in chunks in its order; the sums are recursive and stay on the device. */
int prisim_closure_power(prisim_ctx* ctx, int64_t n0, int64_t nwin, int64_t inner, const double* spectra, const double* scale,
                         int32_t want, int64_t budget_bytes, double* out_individual, double* out_auto, double* out_cross,
                         prisim_cpdelay_stats* stats);

#ifdef __cplusplus
}
#endif

#endif /* PRISIM_CPDELAY_H */
