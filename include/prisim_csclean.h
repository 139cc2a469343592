/*
 * prisim_csclean.h -- Cotton-Schwab CLEAN of the dirty image of a visibility cube: minor cycles in image space with a shift-invariant
 * beam, major cycles through the visibilities with the exact one, on the GPU (libprisim_hip.so, prisim_amd/csrc_imaging/csclean.hip).
 *
 * prisim_clean_image (prisim_imclean.h) subtracts the exact beam for every component, a full direct Fourier pass each.  This entry
 * keeps what that buys -- after every major cycle the residual is the dirty image of V - model, to rounding -- and pays per component
 * only a step on one image channel with an approximate beam.  Notation and conventions of prisim_imclean.h: dd[t][p], W[k], window,
 * gain, maxiter, threshold, the pick rule (compared by > on |.|, the lowest p wins a tie, a NaN never wins), nc = nchan image channels
 * or nc = 1 with chan_avg.  In fp64 throughout.
 *
 *   lattice     the npix directions are taken as ny rows of nx, row-major with nx fastest (pixel p = i nx + j).  With u[i][j] their
 *               unit vectors in their own frame, rho = (u[ny-1][nx/2] - u[0][nx/2]) / (ny - 1) and kappa = (u[ny/2][nx-1] - u[ny/2][0])
 *               / (nx - 1) are the lattice steps, each 0 where its axis has one pixel.
 *   beam        for di in [-(ny-1), ny-1], dj in [-(nx-1), nx-1]:
 *                   P[k][di][dj] = sum_t sum_b w[t][b][k] cos(2 pi f_k b . (rot_t (di rho + dj kappa)) / c) / W[k]
 *               and with chan_avg the sum over the band over sum_k W[k].  It is the synthesized beam of prisim_dirty_image (kind PSF)
 *               at the offsets rot_t delta, by the same kernel: aberration and the curvature of the grid are left to the major
 *               cycles.  P is even: the half-plane (di > 0, or di = 0 and dj >= 0) is computed and the other half is its mirror, bit
 *               for bit.  P[k][0][0] = 1.
 *   residual visibilities   Vres[nt][nbl][nchan], owned by the call: the uploaded cube itself, or a device copy of the resident
 *               cube, which is never written.
 *   cycle c = 0, 1, ... for every image channel still active, on the exact residual R:
 *     1. Pc = max_{p in window} |R[p][k]|; cycle 0 sets P0 = Pc and thr as prisim_clean_image does.
 *     2. in this order: Pc <= thr, or nothing in the window is a number: PRISIM_IMCLEAN_THRESHOLD; maxiter components held:
 *        PRISIM_IMCLEAN_MAXITER; c > 0 and Pc above the peak at the start of the cycle before: PRISIM_CSCLEAN_DIVERGED (the components
 *        stay, the residual is still exact); c == max_major: PRISIM_CSCLEAN_MAJOR.
 *     3. minor cycle: L = max(thr, cycle_depth * Pc), R' = R[:, k].  Repeat: q = argmax_{window} |R'|; stop when |R'[q]| <= L, when
 *        the cycle holds cycle_niter components, or when the channel holds maxiter; otherwise append (q, a = gain * R'[q]) and, for
 *        ALL pixels, R'[p] -= a * P[k][i_p - i_q][j_p - j_q] (one product, one difference).  A cycle that starts adds at least one
 *        component.
 *     4. major cycle: for all (t, b) and the channel (every channel with chan_avg), s = sum over the cycle's new components, in list
 *        order, of a_j (cos phi_j, -sin phi_j), phi_j = 2 pi f_k b . dd[t][q_j] / c from the channel's true frequency, and
 *        Vres -= s.  Then R = the dirty image of Vres as prisim_dirty_image computes it.  The visibilities of a channel that has ended
 *        are not touched, so its image comes back with the same bits.
 * A channel whose W[k] is 0 is PRISIM_IMCLEAN_DEAD from the start, as in prisim_clean_image.
 *
 * The minor cycle of a channel is one workgroup that never waits for another; its working image lives in LDS (PRISIM_CSCLEAN_LDS:
 * npix * 8 B and 64 B of bookkeeping within what a workgroup may hold) or in a device scratch [nc][npix] (PRISIM_CSCLEAN_GLOBAL); the two give
 * the same bits.  The host reads 16 bytes once per major cycle (the channels still active) and runs max_major + 1 cycles at most.
 * dd, the residual, Vres, P with the buffers of its half-plane, the lists, the cycle tables, the window and the scratch are resident
 * within `budget_bytes`; a call that does not fit is refused with the bytes it needs.
 *
 * Accuracy of P.  With u = 2^-53 and N_delta = max|f| max_{t,b,di,dj} sum_i |b_i| sum_j |rot_t,ij| (|di rho_j| + |dj kappa_j|) / c, the
 * largest phase of the lattice in cycles, every element of P is within
 *     1e-12 + 2 pi u 13 N_delta            (14 for STEPPED, plus 2 pi N_delta / f times what the grid is off its line)
 * of the exact sum.  It is N_delta that counts and NOT the baseline in wavelengths, unlike the dirty image: rho and kappa are differences
 * of the given unit vectors, formed first and rounded relative to the difference, and every later operation (the two products, their
 * sum, the rotation, b . delta / c, f tau) rounds relative to an offset, never to a vector of length 1.  A lattice that shrinks as
 * the baselines grow keeps the P of short baselines: with N_delta = 88 cycles the deviation is below 1e-14 at 300 m, at 300 km and
 * at 2400 km alike (N_b = 2e2, 2e5, 2e6), and on a fixed lattice it grows with N_delta, 9e-12 at N_delta = 9e4; some 0.15 * 2 pi u N_delta.
 * The count is that of tests/mosaic_reference.py, which holds the device to it against a 40-digit reference.  The dirty images of the
 * major cycles and the model visibilities (phi_j from the directions of the pixels) carry the law of prisim_imaging.h.
 *
 * Deterministic: the sums of the dirty image and of P as prisim_dirty_image orders them; the peak searches are trees of
 * (|value|, index) pairs under an associative rule; a visibility is updated by one thread, components in list order.  No atomics.
 */
#ifndef PRISIM_CSCLEAN_H
#define PRISIM_CSCLEAN_H

#include <stdint.h>

#include "prisim_hip.h"
#include "prisim_imaging.h"
#include "prisim_imclean.h"

#ifdef __cplusplus
extern "C" {
#endif

/* out_status, besides PRISIM_IMCLEAN_THRESHOLD, _MAXITER and _DEAD */
enum { PRISIM_CSCLEAN_MAJOR = 8, PRISIM_CSCLEAN_DIVERGED = 16 };
/* minor_route: where the working image of a minor cycle lives */
enum { PRISIM_CSCLEAN_AUTO = -1, PRISIM_CSCLEAN_LDS = 0, PRISIM_CSCLEAN_GLOBAL = 1 };
/* max_major at most */
enum { PRISIM_CSCLEAN_MAX_MAJOR = 65536 };

typedef struct prisim_csclean_stats {
  double wall_ms;          /* the whole call on the host clock, copies included */
  double kernel_ms;        /* psf_ms + dirty_ms + peak_ms + minor_ms + model_ms + restore_ms */
  double psf_ms;           /* P: the offsets, the half-plane by the dirty image's kernel, the mirror (stream events) */
  double dirty_ms;         /* the dirty images: the first and one per major cycle, directions and weight sums included */
  double peak_ms;          /* the start-of-cycle peak searches and decisions */
  double minor_ms;         /* the minor cycles */
  double model_ms;         /* the updates of Vres */
  double restore_ms;       /* the restoration */
  int64_t terms;           /* npix * nbl * nchan * nt: of one dirty image */
  int64_t cycles;          /* major cycles run: cycles in which any channel was active */
  int64_t components;      /* components of all channels */
  int64_t polls;           /* reads of the active count */
  int64_t psf_offsets;     /* offsets of the half-plane of P */
  int64_t upload_bytes;    /* bytes copied to the device */
  int64_t download_bytes;  /* bytes copied back to the host */
  int64_t device_bytes;    /* bytes of the resident buffers: what the budget is held against */
  int32_t route;           /* PRISIM_IMAGE_DIRECT or PRISIM_IMAGE_STEPPED */
  int32_t minor_route;     /* PRISIM_CSCLEAN_LDS or PRISIM_CSCLEAN_GLOBAL */
  int32_t streams;         /* 1 */
  int32_t chan_tile;       /* channels per thread of the dirty image */
  int32_t reseed;          /* STEPPED: channels between two seeds from the true frequency; DIRECT: 1 */
  int32_t lds_bytes;       /* LDS per workgroup of the dirty image */
  int32_t minor_lds_bytes; /* LDS per workgroup of the minor cycle */
  int32_t block_pixels;    /* pixels per workgroup of the dirty image, one per thread */
} prisim_csclean_stats;

typedef struct prisim_csclean_args {
  int64_t npix, nbl, nchan, nt;  /* as prisim_imclean_args */
  const double* unitvec;         /* [npix][3] = [ny][nx][3] */
  const double* rot;             /* [nt][9] */
  const double* aberr_beta;      /* [nt][3] or NULL */
  const double* pc_dircos;       /* [nt][3] */
  const double* baselines;       /* [nbl][3] */
  const double* freqs_hz;        /* [nchan] */
  const double* cube;            /* [nt][nbl][nchan] complex128 on the host; or NULL: the context's resident slots [0, nt), copied
                                    on the device behind the context's stream, never written */
  const double* weights;         /* by weight_form */
  const uint8_t* window;         /* [npix] or NULL, as prisim_imclean_args */
  const double* fwhm_rad;        /* [nc] or NULL: no restoration */
  double gain;                   /* in (0, 1] */
  double threshold;              /* finite and >= 0; relative: < 1 */
  int64_t maxiter;               /* components per image channel at most, >= 0 */
  int64_t budget_bytes;          /* device bytes of the resident buffers; <= 0: 1 GiB */
  int32_t weight_form;           /* PRISIM_IMAGE_W_* */
  int32_t chan_avg;              /* 0 or 1 */
  int32_t route;                 /* PRISIM_IMAGE_AUTO or the route itself, of the dirty images and of P */
  int32_t threshold_relative;    /* 0: absolute; 1: a fraction of P0[k] */
  int64_t ny, nx;                /* the lattice: ny * nx == npix, nx fastest */
  double cycle_depth;            /* in (0, 1): a minor cycle runs down to this fraction of its first peak */
  int64_t cycle_niter;           /* components per channel and cycle at most; <= 0: no cap */
  int32_t max_major;             /* major cycles at most, in [0, PRISIM_CSCLEAN_MAX_MAJOR] */
  int32_t minor_route;           /* PRISIM_CSCLEAN_AUTO (LDS when the image fits) or the route itself */
} prisim_csclean_args;

/* out_residual, out_restored, out_comp_pixel, out_comp_flux, out_ncomp, out_status, out_peak0, out_wsum: as prisim_clean_image; the
 *     status is PRISIM_IMCLEAN_THRESHOLD, _MAXITER, _DEAD, PRISIM_CSCLEAN_MAJOR or _DIVERGED.
 * out_ncycles [nc]: the minor cycles the channel ran.
 * out_cycle_ncomp [nc][max_major]: the components held at the end of each cycle; of row k the first out_ncycles[k] entries are
 *     written, the others left alone.
 * out_cycle_peak [nc][max_major + 1]: Pc of every cycle entered and of the test that ended the channel; of row k the first
 *     out_ncycles[k] + 1 entries are written (none for a dead channel); NaN where nothing in the window was a number.
 * out_psf [nc][2 ny - 1][2 nx - 1] or NULL: P, the offset (di, dj) at [di + ny - 1][dj + nx - 1].
 * out_vres [nt][nbl][nchan] complex128 or NULL: the residual visibilities; out_residual is their dirty image bit for bit.
 * stats may be NULL.  Every validation happens before any device work, and nothing is written unless the call succeeds.
 * PRISIM_EINVAL: what prisim_clean_image refuses of these arguments; a null out_ncycles, out_cycle_ncomp or out_cycle_peak;
 * ny * nx != npix or either below 1; a cycle_depth outside (0, 1); max_major outside [0, PRISIM_CSCLEAN_MAX_MAJOR]; an unknown
 * minor_route; PRISIM_CSCLEAN_LDS with an image that does not fit in the LDS of a workgroup; a budget that does not hold the resident
 * buffers (the message names the bytes needed).
 * PRISIM_ESTATE: cube == NULL and no resident cube at all. */
int prisim_clean_image_cs(prisim_ctx* ctx, const prisim_csclean_args* a, double* out_residual, double* out_restored, int32_t* out_comp_pixel,
                          double* out_comp_flux, int32_t* out_ncomp, int32_t* out_status, double* out_peak0, double* out_wsum,
                          int32_t* out_ncycles, int32_t* out_cycle_ncomp, double* out_cycle_peak, double* out_psf, double* out_vres,
                          prisim_csclean_stats* stats);

#ifdef __cplusplus
}
#endif

#endif /* PRISIM_CSCLEAN_H */
