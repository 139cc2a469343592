/*
 * prisim_closure.h -- closure phases (bispectrum phases) of antenna triads on the GPU (libprisim_hip.so, prisim_amd/csrc_closure/).
 *
 * The per-triad body of prisim/interferometry.py:InterferometerArray.getClosurePhase (:7411-7651) for one visibility cube: the gather
 * of the three legs of every triad with their conjugations (:7427-7485), the spectral weights (:7613-7623) or the delay filter
 * (:7536-7599), the bandpass weights (:7625-7627), and the phase of the product of the three legs (:7647-7649).  The triads themselves
 * (getThreePointCombinations, :6989-7085) and the leg table (:7418-7473) are host work of prisim_amd/interferometry.py.
 *
 * DSP.FT1D is not in the reference tree.  Its reading here is the one the delay CLEAN path uses (tests/clean_checker.py,
 * prisim_amd/dsp_readings.py): inverse=False is numpy.fft.fft, inverse=True is numpy.fft.ifft, so that the filter of a row x is
 * ifft(mask * fft(freq_wts * x)).
 *
 * Conventions as in prisim_runs.h: C-contiguous caller-owned host arrays, complex arrays interleaved (re, im), 0 or a negative
 * PRISIM_E* code, the message from prisim_hip_last_error().  The entry uses only the context's device; the call creates and destroys
 * its own streams and device buffers.  The cube and its weights stay on the device for the call; the outputs are streamed in chunks
 * of triads whose buffers take no more than `budget_bytes` of device memory.  An uploaded cube (16 B per element) and bpwts (8 B per
 * element) are outside that budget.
 */
#ifndef PRISIM_CLOSURE_H
#define PRISIM_CLOSURE_H

#include <stdint.h>

#include "prisim_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* longest row (nchan) the delay filter takes: the sub-band limit */
#define PRISIM_CLOSURE_MAX_LEN 4096

/* routes.  PRISIM_CLOSURE_DIRECT is the route of a call without a delay filter; with one, PRISIM_CLOSURE_AUTO takes the fused LDS
 * kernel when nchan is a power of two and a row fits in LDS (on gfx950 every row up to PRISIM_CLOSURE_MAX_LEN does), rocFFT otherwise */
enum { PRISIM_CLOSURE_AUTO = -1, PRISIM_CLOSURE_DIRECT = 0, PRISIM_CLOSURE_FUSED = 1, PRISIM_CLOSURE_ROCFFT = 2 };

typedef struct prisim_closure_stats {
  double wall_ms;          /* the whole call on the host clock, copies included */
  double kernel_ms;        /* the kernels (and rocFFT) of all chunks, from stream events */
  int64_t triads;          /* triads processed */
  int64_t chunks;          /* chunks the call was streamed in */
  int64_t chunk_triads;    /* triads per full chunk */
  int64_t kernel_bytes;    /* bytes the kernels read and write in device memory, counted from the algorithm */
  int64_t download_bytes;  /* bytes copied back to the host */
  int32_t route;           /* PRISIM_CLOSURE_DIRECT, PRISIM_CLOSURE_FUSED or PRISIM_CLOSURE_ROCFFT */
  int32_t streams;         /* streams the chunks were spread over */
  int32_t tile;            /* DIRECT: 1 when rows are transposed through an LDS tile, else 0; FUSED: snapshots per workgroup */
  int32_t lds_bytes;       /* LDS per workgroup */
} prisim_closure_stats;

/* Visibility triplets and closure phases of `ntriads` triads of one cube of nbl baselines, nchan channels and nt snapshots:
 *   cube      host [nbl][nchan][nt] complex128, uploaded once; or NULL: the context's resident visibility slots [0, nt), which lie
 *             on the device as [nt][nbl][nchan] (nbl and nchan must be the array's)
 *   legs      [ntriads][3] int32 rows of the cube for the legs 12, 23, 31; conj [ntriads][3] int32, nonzero: the leg is conjugated
 *   freq_wts  [nchan] float64 spectral weights (ones for none)
 *   bpwts     host [nbl][nchan][nt] float64, bp * bp_wts
 *   masks     NULL: no delay filter.  Else [nmask][nchan] float64 filter_unmask vectors on the unshifted FFT delay axis, and
 *             mask_index [nbl] int32, the mask of each cube row (NULL: mask 0 for every row)
 * For leg l of triad T, v = cube[legs[T][l]], conjugated if conj[T][l]:
 *   no filter:  out_triplets[T][l][ch][t] = (freq_wts[ch] * v[ch][t]) * bpwts[legs[T][l]][ch][t], each factor real, every product
 *               rounded once (fp64, no contraction): the values numpy gives
 *   filter:     out_triplets[T][l][:][t] = ifft(mask * fft(freq_wts * v[:][t])) * bpwts[legs[T][l]][:][t]   (1 <= nchan <=
 *               PRISIM_CLOSURE_MAX_LEN)
 *   out_phase[T][ch][t] = atan2(Im B, Re B), B = (t12 * t23) * t31 with unfused complex products; finite (0 or +-pi) where B == 0.
 * out_triplets [ntriads][3][nchan][nt] complex128, out_phase [ntriads][nchan][nt] float64; each element written once.
 * route: PRISIM_CLOSURE_AUTO, or the route itself (DIRECT only without masks, FUSED / ROCFFT only with).  stats may be NULL. */
int prisim_closure_phase(prisim_ctx* ctx, const double* cube, int64_t nt, int64_t nbl, int64_t nchan, const int32_t* legs,
                         const int32_t* conj, int64_t ntriads, const double* freq_wts, const double* bpwts, const double* masks,
                         int64_t nmask, const int32_t* mask_index, int32_t route, int64_t budget_bytes, double* out_triplets,
                         double* out_phase, prisim_closure_stats* stats);

#ifdef __cplusplus
}
#endif

#endif /* PRISIM_CLOSURE_H */
