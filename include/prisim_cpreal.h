/*
 * prisim_cpreal.h -- closure phases of thermal-noise realisations of one noiseless run, drawn and closed on the GPU
 * (libprisim_hip.so, prisim_amd/csrc_closure/cpreal.hip).
 *
 * The two steps that join the simulator to the closure-phase analysis in the reference: prisim/scriptUtils/replicatesim_util.py
 * (:82-95) draws n_realize noise realisations of one run, and prisim/bispectrum_phase.py:write_PRISim_bispectrum_phase_to_npz
 * (:211-249) takes the closure phases of every one and stacks them as (nlst, n_realize, ntriads, nchan).  Here one kernel goes from
 * the visibilities to that stack: a noise cube never exists, and only the baselines that the triads use are touched.
 *
 * Conventions as in prisim_closure.h: C-contiguous caller-owned host arrays, complex arrays interleaved (re, im), 0 or a negative
 * PRISIM_E* code, the message from prisim_hip_last_error().  The entry uses only the context's device; the call creates and destroys
 * its own streams and device buffers.  The output is streamed in chunks of (snapshot, realisation) pairs whose buffers take no more
 * than `budget_bytes` of device memory; the uploaded rows (cube 16 B, rms 8 B, bpwts 8 B per element) are outside that budget.
 */
#ifndef PRISIM_CPREAL_H
#define PRISIM_CPREAL_H

#include <stdint.h>

#include "prisim_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* routes.  DIRECT: one thread per output element, which draws the noise of its three legs itself: every draw of a baseline is
 * repeated once per triad that uses it.  STAGED: a workgroup owns (snapshot, realisation, tile of channels), draws every used row of
 * the tile once into LDS (16 B per row and channel) and walks the triads from there.  AUTO: STAGED when the rows fit in the LDS of
 * the device at the narrowest tile (8 channels: 1280 rows in the 160 KiB of gfx950), DIRECT otherwise.  Both give the same bits. */
enum { PRISIM_CPREAL_AUTO = -1, PRISIM_CPREAL_DIRECT = 0, PRISIM_CPREAL_STAGED = 1 };
/* what is closed: the visibilities with the noise added, or the noise alone */
enum { PRISIM_CPREAL_NOISY = 0, PRISIM_CPREAL_NOISE = 1 };

typedef struct prisim_cpreal_stats {
  double wall_ms;          /* the whole call on the host clock, copies included */
  double kernel_ms;        /* the kernels of all chunks, from stream events */
  int64_t pairs;           /* (snapshot, realisation) pairs processed: nt * n_realize */
  int64_t chunks;          /* chunks the call was streamed in */
  int64_t chunk_pairs;     /* pairs per full chunk */
  int64_t draws;           /* complex noise values drawn, counted from the algorithm */
  int64_t kernel_bytes;    /* bytes the kernels read and write in device memory, counted from the algorithm */
  int64_t download_bytes;  /* bytes copied back to the host */
  int32_t route;           /* PRISIM_CPREAL_DIRECT or PRISIM_CPREAL_STAGED */
  int32_t streams;         /* streams the chunks were spread over */
  int32_t chan_tile;       /* STAGED: channels per workgroup; DIRECT: 0 */
  int32_t lds_bytes;       /* LDS per workgroup */
} prisim_cpreal_stats;

/* Closure phases of `ntriads` triads for n_realize noise realisations of nt snapshots of nrow baselines ("used rows") and nchan channels:
 *   cube       host [nt][nrow][nchan] complex128: the visibilities the noise is added to, used rows only; or NULL: the context's
 *              resident visibility slots [0, nt), row cube_row[i] of slot t (nchan must be the array's).  Checked, and not read, with
 *              PRISIM_CPREAL_NOISE
 *   cube_row   [nrow] int32 rows of the resident cube (read with resident input only)
 *   bl_global  [nrow] int64 global baseline index of each used row: the draw's counter, as in prisim_hip_noise_indexed
 *   rms        [nt][nrow][nchan] float64 noise rms (vis_rms_freq of the used rows), finite and non-negative
 *   bpwts      [nt][nrow][nchan] float64, bp * bp_wts
 *   legs       [ntriads][3] int32 used rows (0 <= leg < nrow) of the legs 12, 23, 31; conj [ntriads][3] int32, nonzero: conjugated
 *   seed, first, n_realize   realisation r < n_realize is drawn under the key seed + first + r (mod 2^64)
 *   kind       PRISIM_CPREAL_NOISY or PRISIM_CPREAL_NOISE;  route: PRISIM_CPREAL_AUTO or the route itself
 * With n[t][i][f] the value prisim_hip_noise_indexed gives for snapshot t, global baseline bl_global[i], channel f and rms[t][i][f]
 * under the key of realisation r, and v = cube + n (NOISY) or n (NOISE), leg l of triad T is (conj ? conj(v) : v) * bpwts and
 *   out_phase[t][r][T][f] = atan2(Im B, Re B), B = (t12 * t23) * t31
 * with unfused complex products, every product and sum rounded once (fp64, no contraction): the no-filter branch of
 * prisim_closure_phase with freq_wts = 1 on the cube that generate_noise and add_noise would form.  Finite (0 or +-pi) where B == 0.
 * out_phase [nt][n_realize][ntriads][nchan] float64, each element written once.  stats may be NULL.
 * PRISIM_EINVAL: a null required array, a size < 1 (or above 2^30; nchan above 2^20), a leg outside [0, nrow), a negative bl_global, an rms that is negative or not
 * finite, an unknown kind or route, STAGED when the rows do not fit in LDS, resident input with nt above the slots held, another
 * nchan than the array's or a cube_row outside the array.  PRISIM_ESTATE: resident input without a resident cube. */
int prisim_closure_realizations(prisim_ctx* ctx, const double* cube, const int32_t* cube_row, const int64_t* bl_global, int64_t nt,
                                int64_t nrow, int64_t nchan, const double* rms, const double* bpwts, const int32_t* legs,
                                const int32_t* conj, int64_t ntriads, uint64_t seed, int64_t first, int64_t n_realize, int32_t kind,
                                int32_t route, int64_t budget_bytes, double* out_phase, prisim_cpreal_stats* stats);

#ifdef __cplusplus
}
#endif

#endif /* PRISIM_CPREAL_H */
