/*
 * prisim_subband.h -- sub-band delay spectra on the GPU (libprisim_hip.so, prisim_amd/csrc_subband/).
 *
 * The transform of prisim/delay_spectrum.py:DelaySpectrum.subband_delay_transform (:2196-2242) for every (snapshot, baseline) row of
 * one or more visibility cubes and every frequency window, and the FFT resampling of those spectra (:2220-2236, DSP.downsampler read
 * as scipy.signal.resample, prisim_amd/dsp_readings.py).  Conventions as in prisim_hip.h: C-contiguous caller-owned arrays, complex
 * arrays interleaved (re, im), 0 or a negative PRISIM_E* code, the message from prisim_hip_last_error().  The entry uses only the
 * context's device and stream and allocates its own device scratch for the call.
 */
#ifndef PRISIM_SUBBAND_H
#define PRISIM_SUBBAND_H

#include <stdint.h>

#include "prisim_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* longest oversampled (m) and resampled (nres) spectrum the entry takes */
#define PRISIM_SUBBAND_MAX_LEN 4096

/* bits of `want` */
enum {
  PRISIM_SUBBAND_OVER = 1,          /* the m-lag oversampled spectra */
  PRISIM_SUBBAND_OVER_POWER = 2,    /* |oversampled|^2 * pscale[w] */
  PRISIM_SUBBAND_RES = 4,           /* the nres-lag FFT-resampled spectra */
  PRISIM_SUBBAND_RES_POWER = 8      /* |resampled|^2 * pscale[w] */
};

/* routes */
enum { PRISIM_SUBBAND_AUTO = -1, PRISIM_SUBBAND_FUSED = 0, PRISIM_SUBBAND_ROCFFT = 1 };

typedef struct prisim_subband_stats {
  double device_ms;       /* the call's device work, uploads and downloads included (events on the context stream) */
  double kernel_ms;       /* the transform kernels (and rocFFT) alone */
  int64_t rows;           /* input rows transformed: ncubes * nt * nbl */
  int32_t route;          /* PRISIM_SUBBAND_FUSED or PRISIM_SUBBAND_ROCFFT */
  int32_t lds_bytes;      /* dynamic LDS per workgroup of the row kernel */
} prisim_subband_stats;

/* Sub-band delay spectra of `ncubes` cubes of nt * nbl rows [t][b] of nchan channels (complex128):
 *   cubes   host [ncubes][nt][nbl][nchan], or NULL: the context's resident visibility slots [t0, t0 + nt) (ncubes == 1, the array's nbl
 *           and nchan)
 *   bp      [nbp][nchan] float64 bandpass rows: nbp == 1 (every row), nbl (row r uses r % nbl) or nt * nbl (one per row)
 *   wts     [nwin][nchan] float64 frequency windows
 * For every row, window w and cube: x = row * bp_row * wts[w] zero-padded to m lags (nchan <= m <= PRISIM_SUBBAND_MAX_LEN),
 *   oversampled[j] = m df fftshift(ifft(x))[j]                                                  (:2196-2199)
 *   resampled      = scipy.signal.resample(oversampled, nres) (1 <= nres <= PRISIM_SUBBAND_MAX_LEN), formed from x directly:
 *                    the FFT of the oversampled series is m df e^{-2 pi i k floor(m/2) / m} x[k], and resample's spectrum is
 *                    Y[map_out[e]] += map_w[e] X[map_in[e]] over the nmap entries of the selection map (at most two per output bin;
 *                    prisim_amd/dsp_readings.py:resample_map(m, nres) is the reading), then ifft * nres / m
 * Outputs, each NULL unless its bit is in `want`: over [ncubes][nt][nbl][nwin][m] complex128, over_pow same shape float64,
 * res [ncubes][nt][nbl][nwin][nres] complex128, res_pow float64; pscale [nwin] (needed with either power bit).
 * route: PRISIM_SUBBAND_AUTO takes the fused kernel when m is a power of two and its LDS fits, rocFFT otherwise.  stats may be NULL. */
int prisim_subband_transform(prisim_ctx* ctx, int32_t ncubes, int64_t nt, int64_t nbl, int64_t nchan, const double* cubes, int64_t t0,
                             const double* bp, int64_t nbp, int32_t nwin, const double* wts, int64_t m, double df, int64_t nres,
                             int64_t nmap, const int64_t* map_out, const int64_t* map_in, const double* map_w, const double* pscale,
                             int32_t want, int32_t route, double* over, double* over_pow, double* res, double* res_pow,
                             prisim_subband_stats* stats);

#ifdef __cplusplus
}
#endif

#endif /* PRISIM_SUBBAND_H */
