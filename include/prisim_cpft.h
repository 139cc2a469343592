/*
 * prisim_cpft.h -- delay spectra of binned closure phasors on the GPU (libprisim_hip.so, prisim_amd/csrc_closure/cpft.hip).
 *
 * The transforms of prisim/bispectrum_phase.py:ClosurePhaseDelaySpectrum.FT (:2719-2757, :2770-2779): for stacks of stored complex
 * numbers (nlst, ndays or day-bin combinations, ntriads, nchan) -- the binned phasors of ClosurePhase.smooth_in_tbins, the residuals and
 * the sub-model of subtract, the half differences of subsample_differencing -- the delay transform of every row under flag weights
 * normalised by their mean over the channels, a frequency window and a visibility scale, oversampled and FFT-resampled, and the same
 * transform of the weights alone (the lag kernel).
 *
 * Conventions as in prisim_cpdiff.h: C-contiguous caller-owned host arrays, complex arrays interleaved (re, im), 0 or a negative
 * PRISIM_E* code, the message from prisim_hip_last_error().  The entry uses only the context's device; each call creates and destroys
 * its own streams and chunk buffers and streams the rows in chunks whose buffers take no more than `budget_bytes` of device memory
 * (0: 1 GiB).  The tables and the broadcast inputs (below), which are small, lie outside that budget.  fp64 throughout.
 */
#ifndef PRISIM_CPFT_H
#define PRISIM_CPFT_H

#include <stdint.h>

#include "prisim_cpdelay.h"

#ifdef __cplusplus
extern "C" {
#endif

/* longest oversampled (m) and resampled (nres) spectrum, and the most input stacks of one call */
#define PRISIM_CPFT_MAX_LEN PRISIM_CPDELAY_MAX_LEN
#define PRISIM_CPFT_MAX_IN 8

/* bits of `want` */
enum {
  PRISIM_CPFT_OVER = 1,     /* the m-lag oversampled spectra of the inputs */
  PRISIM_CPFT_RES = 2,      /* their nres-lag FFT-resampled spectra */
  PRISIM_CPFT_LAG = 4       /* the lag kernel: oversampled, and with PRISIM_CPFT_RES also resampled */
};

/* routes of the oversampled transform.  AUTO takes the fused LDS kernel when m is a power of two, rocFFT between a prepare and a
 * finish kernel otherwise.  The resampled spectra are formed by one kernel on either route. */
enum { PRISIM_CPFT_AUTO = -1, PRISIM_CPFT_FUSED = 0, PRISIM_CPFT_ROCFFT = 1 };

typedef struct prisim_cpft_stats {
  double wall_ms;          /* the whole call on the host clock, copies included */
  double kernel_ms;        /* the kernels (and rocFFT) of all chunks, from stream events */
  int64_t rows;            /* n0 * n1 * n2 */
  int64_t chunks;          /* chunks the rows were streamed in */
  int64_t chunk_rows;      /* rows per full chunk */
  int64_t row_bytes;       /* device bytes of the chunk buffers per row and stream: chunk_rows = budget / (2 row_bytes) */
  int64_t kernel_bytes;    /* bytes the kernels have to move to and from device memory: every input and weight once, every output once */
  int64_t upload_bytes;    /* bytes copied to the device */
  int64_t download_bytes;  /* bytes copied back to the host */
  int32_t route;           /* PRISIM_CPFT_FUSED or PRISIM_CPFT_ROCFFT */
  int32_t streams;         /* streams the chunks alternated over */
  int32_t group_rows;      /* rows per workgroup of the transforming (FUSED) or preparing (ROCFFT) kernel */
  int32_t lds_bytes;       /* dynamic LDS per workgroup of that kernel */
} prisim_cpft_stats;

/* A row is one element of the three leading axes (n0, n1, n2): LST bins, day bins or day-bin combinations, triads.
 *
 * inputs    nin pointers (0 <= nin <= PRISIM_CPFT_MAX_IN) to complex128 stacks; stack i has the shape in_shape[3 i .. 3 i + 2] =
 *           (b0, b1, b2), each the full extent or 1, times nchan.  An extent of 1 is read with stride 0 on the device (numpy's
 *           broadcast_to); such a stack is uploaded once as it is.  Full stacks are streamed with the rows.
 * w         float64 [n0][n1][n2][nchan], the flag weights shared by all inputs, or NULL (no weights).
 * wts       float64 [nwin][nchan], the frequency windows.
 * vscale    float64 [nwin][n0], the visibility scale per window and LST bin, or NULL (1).
 * m         lags of the oversampled spectra, nchan <= m <= PRISIM_CPFT_MAX_LEN; nres (1 <= nres <= PRISIM_CPFT_MAX_LEN, needed with
 *           PRISIM_CPFT_RES) those of the resampled spectra, with the selection map (nmap, map_out, map_in, map_w) of
 *           prisim_amd/dsp_readings.py:resample_map(m, nres) as in prisim_cpdelay.h.
 *
 * For row r = (i0, i1, i2), window k and input i:
 *   mu_r            = (sum over ch of w[r][ch]) / nchan
 *   fw[r][ch]       = w[r][ch] / mu_r; 1 without w; 0 for the whole row where mu_r == 0
 *   x[ch]           = in_i[r][ch] * (fw[r][ch] * wts[k][ch] * vscale[k][i0]), zero-padded to m; where the real factor is exactly 0
 *                     x[ch] is 0 whatever the input holds
 *   over_i[k][r][j] = m df fftshift(ifft(x))[j]
 *   res_i[k][r][:]  = scipy.signal.resample(over_i[k][r], nres), formed from x directly as prisim_subband.h describes
 *   lag_kernel[k][r][:] and lag_kernel_res[k][r][:]: the same transforms of fw[r][ch] * wts[k][ch], with no input and no vscale;
 *                     without w there is one such row per window.
 * Outputs, complex128, each element written once: over[i] [nwin][n0][n1][n2][m] and res[i] [nwin][n0][n1][n2][nres] for every input
 * (the arrays of pointers may be NULL when their bit is not in `want`), lag_kernel [nwin][n0][n1][n2][m] and lag_kernel_res
 * [...][nres] with w, [nwin][1][1][1][m] and [...][nres] without.
 *
 * On an argument error (PRISIM_EINVAL) nothing is written to the outputs; a device error in a later chunk leaves the chunks before it
 * written.  route: PRISIM_CPFT_AUTO or the route itself; FUSED with an m that is no power of two is an argument error.  stats may be
 * NULL. */
int prisim_cphase_ft(prisim_ctx* ctx, int64_t n0, int64_t n1, int64_t n2, int64_t nchan, int32_t nin, const double* const* inputs,
                     const int64_t* in_shape, const double* w, int32_t nwin, const double* wts, const double* vscale, int64_t m, double df,
                     int64_t nres, int64_t nmap, const int64_t* map_out, const int64_t* map_in, const double* map_w, int32_t want,
                     int32_t route, int64_t budget_bytes, double* const* over, double* const* res, double* lag_kernel,
                     double* lag_kernel_res, prisim_cpft_stats* stats);

#ifdef __cplusplus
}
#endif

#endif /* PRISIM_CPFT_H */
