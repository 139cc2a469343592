/*
 * prisim_mosclean.h -- CLEAN of the beam-weighted mosaic of the snapshots of a visibility cube, on the GPU
 * (libprisim_hip.so, prisim_amd/csrc_imaging/mosclean.hip).
 *
 * prisim_clean_image (prisim_imclean.h) deconvolves apparent fluxes; prisim_mosaic_image (prisim_mosaic.h) returns true fluxes, but
 * every source still carries the sidelobes of every other one.  This entry joins the two.  A component of true flux a at pixel q has
 * the model visibilities A[t][q][k] a e^{-i phi_q} in snapshot t, what the sky-sum simulates for it.  In the weighted visibility space
 * that atom has the inner product N[q][k] with the data and the squared norm Q[q][k], the mosaic's numerator and denominator: the
 * mosaic value N / Q is the least-squares flux of a component at q, choosing the pixel of the largest N^2 / Q is matching pursuit, and
 * sum w |V_res|^2 cannot grow for 0 < gain <= 1, for any drift and any chromaticity of the beam.
 *
 * Notation of prisim_imaging.h, prisim_mosaic.h and prisim_imclean.h: dd[t][p] = s[p][t] - s0[t]; A[t][p][k] the power pattern of
 * snapshot t, 0 where s_z < 0; W_t[k], Wtot[k], N, Q of prisim_mosaic.h; nc = nchan image channels, or nc = 1 with chan_avg.  In fp64
 * throughout and in this order:
 *
 *   state       R_N[p][k], per channel always, starts as the mosaic's N.  Q, Wtot and the mask valid[p][kc] = Q >= (pbmin * pbmin) * Wtot
 *               never change; with chan_avg the mask is that of the band sums, k ascending, as prisim_mosaic_image forms them.
 *   search      F[p][k] = R_N / sqrt(Q * Wtot[k]), with chan_avg F[p] = sum_k R_N / sqrt(sum_k Q * sum_k Wtot): the flat-noise image, in
 *               the units and at the noise level of prisim_dirty_image; NaN where not valid.  By Cauchy-Schwarz the response of F at
 *               any other pixel to a component never exceeds its response at the component's own pixel.
 *   threshold, pick, stop   those of prisim_imclean.h word for word, applied to |F| over window and valid: P0[k], thr[k] (relative or
 *               absolute, in the units of F), the lowest index wins a tie, a NaN never wins; PRISIM_IMCLEAN_THRESHOLD, _MAXITER, and
 *               _DEAD for Wtot[k] == 0 (the band's sum with chan_avg).  A channel whose window holds no valid pixel ends with
 *               PRISIM_IMCLEAN_THRESHOLD in the first iteration, with a NaN P0.
 *   component   a = gain * (R_N[q][k] / Q[q][k]), with chan_avg a = gain * (sum_k R_N[q][k] / sum_k Q[q][k]): a true flux.
 *   update      for ALL pixels, t ascending and b ascending inside it:
 *                   D_t[p][k] = sum_b (w[t][b][k] * (a_k * A[t][q_k][k])) * cos(2 pi f_k b . (dd[t][p] - dd[t][q_k]) / c)
 *                   R_N[p][k] = fma(-A[t][p][k], D_t[p][k], R_N[p][k])
 *               with chan_avg every channel takes the band's one (q, a).  A component whose pixel is below the horizon in snapshot t
 *               has A = 0 there and adds nothing in that snapshot.  A channel that has ended has a = 0 and keeps its bits.
 *
 * The beam is evaluated once per call into a resident table A[nt][npix][nchan]; with dd, s, R_N, Q, F, the outputs, the component
 * lists and the window it is resident within `budget_bytes`, and an image that does not fit is refused with the bytes it needs.  The
 * uploaded tables are outside that budget.  The device never waits for the host inside an iteration; iterations are enqueued
 * `poll_every` at a time as in prisim_imclean.h, and no result depends on poll_every.
 *
 * Deterministic: the first residual is prisim_mosaic_image's own N and Q, bit for bit (maxiter = 0 is a mosaic); the update adds the
 * b terms of a (pixel, channel, snapshot) in one thread, b ascending, and flushes the snapshots in that thread, t ascending; the peak
 * search is that of prisim_clean_image.  No atomics; no sum is split over workgroups.
 */
#ifndef PRISIM_MOSCLEAN_H
#define PRISIM_MOSCLEAN_H

#include <stdint.h>

#include "prisim_hip.h"
#include "prisim_imaging.h"
#include "prisim_imclean.h"
#include "prisim_mosaic.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct prisim_mosclean_stats {
  double wall_ms;          /* the whole call on the host clock, copies included */
  double kernel_ms;        /* mosaic_ms + peak_ms + update_ms + restore_ms */
  double mosaic_ms;        /* the first residual: directions, weight sums, the beam table, N and Q (stream events) */
  double peak_ms;          /* the search images and the peak searches of all iterations */
  double update_ms;        /* the updates of all iterations */
  double restore_ms;       /* the last search image, the division and the restoration */
  int64_t terms;           /* npix * nbl * nchan * nt: of the first residual and of every update */
  int64_t beam_values;     /* npix * nchan * nt: evaluations of the beam, once per call */
  int64_t iterations;      /* iterations in which a channel was active */
  int64_t components;      /* components of all channels */
  int64_t polls;           /* reads of the active count */
  int64_t chunks;          /* 1: the whole image is resident */
  int64_t chunk_pixels;    /* npix */
  int64_t kernel_bytes;    /* bytes the kernels read and write in device memory, counted from the algorithm */
  int64_t upload_bytes;    /* bytes copied to the device */
  int64_t download_bytes;  /* bytes copied back to the host */
  int64_t device_bytes;    /* bytes of the resident buffers: what the budget is held against */
  int32_t route;           /* PRISIM_IMAGE_DIRECT or PRISIM_IMAGE_STEPPED */
  int32_t streams;         /* 1 */
  int32_t chan_tile;       /* channels per thread of the first residual and of the update */
  int32_t reseed;          /* STEPPED: channels between two seeds from the true frequency; DIRECT: 1 */
  int32_t lds_bytes;       /* LDS per workgroup of the update */
  int32_t block_pixels;    /* pixels per workgroup, one per thread */
} prisim_mosclean_stats;

typedef struct prisim_mosclean_args {
  int64_t npix, nbl, nchan, nt;  /* the fields of prisim_mosaic_args, in their order; npix <= 2^28 */
  const double* unitvec;         /* [npix][3] */
  const double* rot;             /* [nt][9] */
  const double* aberr_beta;      /* [nt][3] or NULL */
  const double* pc_dircos;       /* [nt][3] the phase centres */
  const double* baselines;       /* [nbl][3] */
  const double* freqs_hz;        /* [nchan] */
  const double* cube;            /* [nt][nbl][nchan] complex128, or NULL: the context's resident slots [0, nt) */
  const double* weights;         /* by weight_form */
  int32_t weight_form;           /* PRISIM_IMAGE_W_* */
  int32_t chan_avg;              /* 0: every channel cleaned on its own; 1: the band's mosaic cleaned, nc = 1 */
  int32_t route;                 /* PRISIM_IMAGE_AUTO or the route itself, of the first residual and of the updates */
  int32_t beam_kind;             /* PRISIM_BEAM_*: the beam of prisim_mosaic_args */
  double  diameter_m;
  double  beam_pc_dircos[3];
  const double* beam_pc_snap;    /* [nt][3] or NULL */
  const prisim_beam_ext* ext;    /* NULL, or n_ext structs */
  int64_t n_ext;                 /* 0, 1 or nt */
  double  pbmin;                 /* in [0, 1): the mask of the search and of the outputs */
  int64_t budget_bytes;          /* device bytes of the resident buffers; <= 0: 1 GiB */
  double  gain;                  /* in (0, 1] */
  int64_t maxiter;               /* components per image channel at most, >= 0; 0: the call is a mosaic */
  double  threshold;             /* finite and >= 0, in the units of F; relative: < 1 */
  int32_t threshold_relative;    /* 0: absolute; 1: a fraction of P0[k] */
  const uint8_t* window;         /* [npix] non-zero: the pixel may hold components; or NULL: every pixel.  All zero: PRISIM_EINVAL */
  const double* fwhm_rad;        /* [nc] the restoring beam per image channel, > 0 and finite; or NULL: no restoration */
  int32_t poll_every;            /* iterations per batch; <= 0: PRISIM_IMCLEAN_POLL_DEFAULT; at most PRISIM_IMCLEAN_POLL_MAX are taken */
} prisim_mosclean_args;

/* out_residual [npix][nc]: R_N / Q under the mask when every channel has ended, NaN where masked: true fluxes (the expressions of
 *     prisim_mosaic_image's out_mosaic on R_N).
 * out_restored [npix][nc] or NULL (then fwhm_rad is not read): out_residual + the components through the restoring beam of
 *     prisim_clean_image; NaN where the residual is.
 * out_residual_flat [npix][nc] or NULL: F of the final R_N.
 * out_pb_eff [npix][nc], out_num (the final R_N) and out_den (Q) [npix][nchan], out_wsum (Wtot) [nchan]: as prisim_mosaic_image; each
 *     may be NULL.
 * out_comp_pixel, out_comp_flux [nc][maxiter], out_ncomp, out_status, out_peak0 [nc]: as prisim_clean_image; the fluxes are true
 *     fluxes and out_peak0 is in the units of F.  stats may be NULL.
 * Every validation happens before any device work, and nothing is written unless the call succeeds.
 * PRISIM_EINVAL: what prisim_mosaic_image and prisim_clean_image refuse of these arguments (out_residual in the place of out_mosaic),
 * by their own checks; a budget that does not hold the whole image (the message names the bytes needed).
 * PRISIM_ESTATE: cube == NULL and no resident cube at all. */
int prisim_clean_mosaic(prisim_ctx* ctx, const prisim_mosclean_args* a, double* out_residual, double* out_restored, double* out_residual_flat,
                        double* out_pb_eff, double* out_num, double* out_den, double* out_wsum, int32_t* out_comp_pixel,
                        double* out_comp_flux, int32_t* out_ncomp, int32_t* out_status, double* out_peak0, prisim_mosclean_stats* stats);

#ifdef __cplusplus
}
#endif

#endif /* PRISIM_MOSCLEAN_H */
