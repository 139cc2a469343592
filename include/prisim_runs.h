/*
 * prisim_runs.h -- delay spectra and delay power spectra of stacks of runs on the GPU (libprisim_hip.so, prisim_amd/csrc_runs/).
 *
 * The transforms of prisim/delay_spectrum.py:DelaySpectrum.delay_transform_allruns (:1475-1618) and subband_delay_transform_allruns
 * (:2252-2513), and the product of DelayPowerSpectrum.compute_power_spectrum_allruns (:4067-4195), on caller arrays in the reference's
 * layout: visibilities [R][nbl][nchan][nt] (R = the product of the leading "run" axes), spectra [nwin][R][nbl][nout][nt].  Conventions
 * as in prisim_hip.h: C-contiguous caller-owned host arrays, complex arrays interleaved (re, im), 0 or a negative PRISIM_E* code, the
 * message from prisim_hip_last_error().  The entries use only the context's device; each call creates and destroys its own streams and
 * device buffers and streams its input in chunks of (run, baseline) pairs no larger than `budget_bytes` of device memory.
 */
#ifndef PRISIM_RUNS_H
#define PRISIM_RUNS_H

#include <stdint.h>

#include "prisim_hip.h"
#include "prisim_subband.h"

#ifdef __cplusplus
extern "C" {
#endif

/* longest padded (m) and resampled (nout) spectrum the transform takes: the sub-band limit */
#define PRISIM_RUNS_MAX_LEN PRISIM_SUBBAND_MAX_LEN

/* output modes of prisim_runs_transform */
enum {
  PRISIM_RUNS_ALL = 1,        /* every one of the m lags */
  PRISIM_RUNS_INTERP = 2,     /* lag positions j * factor, j < nout, linearly interpolated (every factor-th lag for an integer factor) */
  PRISIM_RUNS_RESAMPLE = 3    /* scipy.signal.resample of the m lags to nout lags, through the selection map */
};

/* routes */
enum { PRISIM_RUNS_AUTO = -1, PRISIM_RUNS_FUSED = 0, PRISIM_RUNS_ROCFFT = 1, PRISIM_RUNS_DIRECT = 2 };

typedef struct prisim_runs_stats {
  double wall_ms;          /* the whole call on the host clock, copies included */
  int64_t pairs;           /* (run, baseline) pairs (transform) or elements (power) processed */
  int64_t chunks;          /* chunks the call was streamed in */
  int64_t chunk_pairs;     /* pairs (elements) per full chunk */
  int32_t route;           /* PRISIM_RUNS_FUSED, PRISIM_RUNS_ROCFFT or PRISIM_RUNS_DIRECT (resampling and power) */
  int32_t streams;         /* streams the chunks were spread over */
  int32_t tile;            /* snapshots per workgroup */
  int32_t lds_bytes;       /* dynamic LDS per workgroup */
} prisim_runs_stats;

/* Delay spectra of every (run, baseline, snapshot) row and every window w < nwin:
 *   vis      host [R][nbl][nchan][nt], complex128 (vis_is_c64 == 0) or complex64 (upcast on the device), or NULL: unit visibilities
 *            (the lag kernel of the weights)
 *   bp, wts  float64 weights over (baseline, channel, snapshot) with element strides bp_strides[3] / wts_strides[3] (0: broadcast);
 *            either may be NULL (ones)
 *   win      [nwin][nchan] float64 windows, or NULL (nwin == 1, ones)
 *   x[n] = ((vis * bp) * wts) * win[w] on channels n < nchan, zero up to m lags (nchan <= m <= PRISIM_RUNS_MAX_LEN);
 *   spectrum[j] = scale * fftshift(ifft(x))[j], j < m.
 * out_mode PRISIM_RUNS_ALL: nout == m; PRISIM_RUNS_INTERP: nout positions j * factor (x0 + frac (x1 - x0), indices clamped to m - 1);
 * PRISIM_RUNS_RESAMPLE: scipy.signal.resample(spectrum, nout), Y[map_out[e]] += map_w[e] X[map_in[e]] over the nmap entries of
 * prisim_amd/dsp_readings.py:resample_map(m, nout), formed from x directly (the FFT of the spectrum is scale e^{-2 pi i k floor(m/2)/m}
 * x[k]).  out: [nwin][R][nbl][nout][nt] complex128, each element written once.
 * route: PRISIM_RUNS_AUTO takes the fused LDS kernel for power-of-two m, rocFFT otherwise (the resampling mode has one direct kernel).
 * stats may be NULL. */
int prisim_runs_transform(prisim_ctx* ctx, int64_t R, int64_t nbl, int64_t nchan, int64_t nt, const void* vis, int32_t vis_is_c64,
                          const double* bp, const int64_t* bp_strides, const double* wts, const int64_t* wts_strides, int32_t nwin,
                          const double* win, int64_t m, double scale, int32_t out_mode, int64_t nout, double factor, int64_t nmap,
                          const int64_t* map_out, const int64_t* map_in, const double* map_w, int32_t route, int64_t budget_bytes,
                          double* out, prisim_runs_stats* stats);

/* Power of nf * inner elements: out[e] = Re(v1[e] conj(v2[e])) * factor[e / inner] (* 2 when cross != 0), as numpy rounds
 * (v1 * v2.conj() * factor).real: the complex product in the inputs' precision (complex64: fp32, then widened), its real part
 * fma(re1, re2, im1 * im2) when fused_product != 0 (numpy's SIMD complex loop) or re1 * re2 + im1 * im2 otherwise.  v2 NULL: v1 (auto
 * power).  v1, v2 host complex128 (is_c64 == 0) or complex64; factor [nf] float64; out host float64. */
int prisim_runs_power(prisim_ctx* ctx, int64_t nf, int64_t inner, const void* v1, const void* v2, int32_t is_c64, const double* factor,
                      int32_t cross, int32_t fused_product, int64_t budget_bytes, double* out, prisim_runs_stats* stats);

#ifdef __cplusplus
}
#endif

#endif /* PRISIM_RUNS_H */
