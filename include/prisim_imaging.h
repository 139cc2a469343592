/*
 * prisim_imaging.h -- the dirty image and the synthesized beam of a visibility cube by the direct Fourier sum, on the GPU
 * (libprisim_hip.so, prisim_amd/csrc_imaging/imaging.hip).
 *
 * prisim/interferometry.py:ApertureSynthesis (:8990-9255) of the reference promises "aperture synthesis of visibility measurements"
 * and stops at uvw coordinates and an empty grid.  Here the image is made exactly, as the adjoint of the sky-sum this library is built
 * around: the sky-sum is V[b][f][t] = sum_s x_s e^{-i phi}, the image is I[p][f] ~ sum_{b,t} w Re(V e^{+i phi}) with the same phase
 * phi = 2 pi f b . (s - s0) / c.  No uv grid, no gridding kernel and no w-term approximation are involved.
 *
 * Conventions as in prisim_antpower.h and prisim_cpreal.h: C-contiguous caller-owned host arrays, complex arrays interleaved (re, im),
 * 0 or a negative PRISIM_E* code, the message from prisim_hip_last_error().  The entry uses only the context's device, creates and
 * destroys its own streams and device buffers, and does not disturb the context's array, sky or catalogue; with cube == NULL it reads
 * the context's resident visibility slots.  The pixels are streamed in chunks (contiguous ranges of pixels, a whole number of blocks
 * of 256) whose buffers take no more than `budget_bytes` of device memory; the uploaded tables (the cube 16 B and the weights 8 B per
 * element, the baselines, the frames) are outside that budget.
 *
 * The sum is deterministic: every (pixel, channel) adds its (t, b) terms in one thread, t ascending and b ascending inside t -- an
 * order that depends on (nt, nbl) alone.  No atomic is used and the (t, b) sum is never split over workgroups.  The chunks only decide
 * which pixels are in flight together: the outputs are bit-identical for any budget.
 *
 * No horizon test is made: a direction is imaged wherever it is, below the horizon too.
 *
 * Domain.  The phase range is that of prisim_hip_set_array: max|b| * 2 * max|f| / c >= 2^29 = 536870912 cycles is PRISIM_EINVAL, in
 * the same sentence, on the host, before any launch and with nothing written (|s - s0| <= 2 for unit vectors, so no phase reaches
 * 2^29 cycles; the fp64 fraction of a cycle, x - rint(x), would be 0 past 2^52).  prisim_mosaic_image, prisim_clean_image,
 * prisim_clean_mosaic and the Cotton-Schwab entries make the same check.
 *
 * Accuracy.  With u = 2^-53, N_b = max|f| max_b sum_i |b_i| / c the longest baseline in wavelengths and N' = max|f| max sum_i
 * |b_i| |s_i - s0_i| / c the largest phase in cycles, every element of an image is within
 *     (1e-11 + 2 pi u (13 N_b + 7 N')) sum w|V| / sum w            (8 N' for STEPPED, plus 2 pi N' / f times what the grid is off its line)
 * of the exact sum: the directions are computed here, in fp64, and their rounding acts on the whole baseline in wavelengths however
 * narrow the field is.  The count is that of tests/imaging_reference.py, which holds the device to it against a 40-digit reference;
 * measured, the deviation is about 0.2 * 2 pi u N_b.  So an image keeps the project's 1e-11 of its scale while 2 pi u (13 N_b + 7 N')
 * is small against 1e-11: the two are equal at N_b = N' = 7e2 wavelengths (1.4 km at 150 MHz).  As measured on the MI355X the
 * deviation is 3e-12 of the scale at N_b = 2e4 (30 km at 150 MHz), passes 1e-11 near 7e4 (140 km), is 3e-11 at 2e5 (300 km) and grows
 * in proportion.  The bit equalities among the entries do not depend on it.
 */
#ifndef PRISIM_IMAGING_H
#define PRISIM_IMAGING_H

#include <stdint.h>

#include "prisim_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* what is imaged: the visibilities, or V = 1 (the synthesized beam; the cube is neither required nor read) */
enum { PRISIM_IMAGE_DIRTY = 0, PRISIM_IMAGE_PSF = 1 };
/* routes.  DIRECT evaluates sin and cos of every term from the channel's own frequency; it takes any channel grid.  STEPPED, the
 * production route: a thread owns a pixel and a tile of channels, seeds e^{i phi} at the tile's first channel from that channel's
 * true frequency (and again every `reseed` channels; tile == reseed here, so every tile is seeded once) and steps it by
 * e^{2 pi i tau df} with one complex multiply per channel.  It needs a uniform channel grid, by the rule of the sky-sum's recurrence
 * kernels (prisim_hip_set_array): with df = (f[nchan-1] - f[0]) / (nchan - 1), or 0 for one channel, every
 * |f[k] - (f[0] + k df)| <= 1e-7 Hz.  AUTO is STEPPED exactly when the grid is uniform by that rule and DIRECT otherwise; an explicit
 * STEPPED on another grid is PRISIM_EINVAL.  The two routes agree to rounding (2e-11 of the natural scale), not to the bit. */
enum { PRISIM_IMAGE_AUTO = -1, PRISIM_IMAGE_DIRECT = 0, PRISIM_IMAGE_STEPPED = 1 };
/* weights: none (w = 1), one per baseline [nbl], or one per visibility [nt][nbl][nchan].  A broadcast axis is read with stride 0 on
 * the device; nothing is expanded on the host. */
enum { PRISIM_IMAGE_W_NONE = 0, PRISIM_IMAGE_W_BASELINE = 1, PRISIM_IMAGE_W_FULL = 2 };

typedef struct prisim_imaging_stats {
  double wall_ms;          /* the whole call on the host clock, copies included */
  double kernel_ms;        /* the kernels of all chunks, from stream events, summed over the streams (which overlap) */
  int64_t terms;           /* npix * nbl * nchan * nt */
  int64_t chunks;          /* chunks the pixels were streamed in */
  int64_t chunk_pixels;    /* pixels per full chunk, a multiple of block_pixels */
  int64_t kernel_bytes;    /* bytes the kernels read and write in device memory, counted from the algorithm */
  int64_t upload_bytes;    /* bytes copied to the device */
  int64_t download_bytes;  /* bytes copied back to the host */
  int32_t route;           /* PRISIM_IMAGE_DIRECT or PRISIM_IMAGE_STEPPED */
  int32_t streams;         /* streams the chunks were dealt to */
  int32_t chan_tile;       /* channels per thread: its accumulators, one double each */
  int32_t reseed;          /* STEPPED: channels between two seeds from the true frequency; DIRECT: 1 */
  int32_t lds_bytes;       /* LDS per workgroup: the staged rows of the visibility operand */
  int32_t block_pixels;    /* pixels per workgroup, one per thread */
} prisim_imaging_stats;

typedef struct prisim_imaging_args {
  int64_t npix, nbl, nchan, nt;  /* directions, baselines, channels, snapshots: each >= 1, nchan <= 2^20, npix * nchan <= 2^46 */
  const double* unitvec;         /* [npix][3] the directions in their own frame, |u| = 1 to 1e-6 */
  const double* rot;             /* [nt][9] row-major rotation of that frame into East-North-Up per snapshot, orthonormal to 1e-9
                                    (the identity for local directions) */
  const double* aberr_beta;      /* [nt][3] aberration velocity / c in the directions' frame, |beta| < 0.01; or NULL = none */
  const double* pc_dircos;       /* [nt][3] East-North-Up phase centre of each snapshot, a unit vector to 1e-6 */
  const double* baselines;       /* [nbl][3] East-North-Up, metres */
  const double* freqs_hz;        /* [nchan] positive and finite */
  const double* cube;            /* [nt][nbl][nchan] complex128 on the host; or NULL: the context's resident slots [0, nt), as
                                    prisim_closure_realizations reads them.  Not read with PRISIM_IMAGE_PSF */
  const double* weights;         /* by weight_form: not read, [nbl], or [nt][nbl][nchan]; finite and >= 0 */
  int32_t kind;                  /* PRISIM_IMAGE_DIRTY or PRISIM_IMAGE_PSF */
  int32_t weight_form;           /* PRISIM_IMAGE_W_* */
  int32_t chan_avg;              /* 0: one image per channel; 1: one image of the band */
  int32_t route;                 /* PRISIM_IMAGE_AUTO or the route itself */
  int64_t budget_bytes;          /* device bytes of the per-chunk buffers; <= 0: 1 GiB */
} prisim_imaging_args;

/* With s[p][t] = normalise(R_t (u_p + beta_t)) the East-North-Up direction of pixel p at snapshot t (the statement of
 * prisim_antpower.h), s0[t] = pc_dircos[t], tau = b_b . (s[p][t] - s0[t]) / c and phi = 2 pi f_k tau, in fp64:
 *     D[p][k] = sum_t sum_b w[t][b][k] (Re V[t][b][k] cos phi - Im V[t][b][k] sin phi)          (V = 1 with PRISIM_IMAGE_PSF)
 *     W[k]    = sum_t sum_b w[t][b][k]
 *     out_image[p][k] = D[p][k] / W[k]                      chan_avg = 0: [npix][nchan]
 *     out_image[p]    = sum_k D[p][k] / sum_k W[k]          chan_avg = 1: [npix]
 * (IEEE division; the sums over k ascending).  out_wsum, [nchan] or [1], may be NULL; stats may be NULL.  A zero weight sum gives NaN
 * in out_image (0 / 0), as prisim_antenna_power does for an empty sky: a flagged-out channel does not come back as a plausible 0.
 * The result is in the units of the visibilities, per beam: a point source of flux S seen through a delta beam images to S at its own
 * direction, and the PSF is 1 at the phase centre.
 * Nothing is written unless the call succeeds.
 * PRISIM_EINVAL: a null a, out_image, unitvec, rot, pc_dircos, baselines or freqs_hz, or null weights with a weight form that reads
 * them; a size < 1, nchan above 2^20, nt or nbl above 2^30, or npix * nchan beyond the chunk arithmetic (2^46); a unit vector or a
 * pc_dircos row whose norm is off by more than 1e-6; a rotation that is not orthonormal to 1e-9 or a |beta| >= 0.01; a baseline that
 * is not finite; a phase range max|b| * 2 * max|f| / c of 2^29 cycles or more; a frequency that is not positive and finite; a weight
 * that is negative or not finite; an unknown kind, route or weight form; STEPPED on a grid that is not uniform; PRISIM_IMAGE_DIRTY with cube == NULL and a resident cube that has fewer than nt slots,
 * another nchan or another nbl than asked for; a budget that cannot hold one block of pixels.
 * PRISIM_ESTATE: PRISIM_IMAGE_DIRTY with cube == NULL and no resident cube at all (no array set). */
int prisim_dirty_image(prisim_ctx* ctx, const prisim_imaging_args* a, double* out_image, double* out_wsum, prisim_imaging_stats* stats);

#ifdef __cplusplus
}
#endif

#endif /* PRISIM_IMAGING_H */
