/*
 * prisim_moscs.h -- Cotton-Schwab CLEAN of the beam-weighted mosaic of the snapshots of a visibility cube: minor cycles on the
 * flat-noise image with a shift-invariant beam, major cycles through the residual visibilities with the exact beam weights, on the GPU
 * (libprisim_hip.so, prisim_amd/csrc_imaging/moscs.hip).
 *
 * prisim_clean_mosaic (prisim_mosclean.h) pays one full mosaic pass per component.  This entry is to it what prisim_clean_image_cs
 * (prisim_csclean.h) is to prisim_clean_image: it keeps what the pass buys -- after every major cycle R_N is the mosaic's numerator
 * of V - model, to rounding -- and pays per component only a step on one image channel.  Notation of prisim_mosclean.h (dd[t][p],
 * A[t][p][k], W_t, Wtot, N, Q, R_N, F, valid, nc) and of prisim_csclean.h (the lattice ny x nx with rho and kappa, P, Vres, the
 * cycles).  In fp64 throughout.
 *
 * Why the minor cycle of prisim_csclean.h serves: in F = R_N / sqrt(Q Wtot) a component of flat amplitude c at pixel q has the true
 * flux a = c sqrt(Wtot / Q[q]) and the response c N_c[p] / sqrt(Q[p] Q[q]), N_c the numerator of a unit component at q.  That is c at
 * p = q, never above c anywhere (Cauchy-Schwarz), and near q, where the beam weights of p and q are proportional over the snapshots,
 * c times the synthesized beam.  What this leaves behind -- drift, chromaticity, curvature, aberration, the w-term -- the major cycle
 * corrects, and the major cycle is exact.
 *
 *   state       the beam table A[nt][npix][nchan] (0 below the horizon), Q, W_t, Wtot, the mask valid and R_N, which starts as the
 *               mosaic's numerator: exactly as prisim_clean_mosaic forms them, by its own kernels, bit for bit.  Q is never recomputed.
 *   residual visibilities   Vres[nt][nbl][nchan], owned by the call as in prisim_clean_image_cs: the uploaded cube itself, or a device
 *               copy of the resident cube, which is never written.
 *   beam        P[nc][2 ny - 1][2 nx - 1] of prisim_csclean.h, by its code: the synthesized beam of the weights at the lattice offsets,
 *               over the weight sums of prisim_dirty_image.  ny * nx == npix, nx fastest.
 *   scale       s[p][kc] = sqrt(Wc[kc] / Qc[p][kc]), Wc and Qc the band sums with chan_avg, k ascending: one quotient, one square
 *               root, once per call.
 *   cycle c = 0, 1, ... for every image channel still active:
 *     1. F from R_N as prisim_clean_mosaic forms it; Pc = max |F| over window and valid (a NaN never wins).  Cycle 0 sets P0 and thr, in
 *        the units of F, as prisim_clean_mosaic does.
 *     2. the tests of prisim_csclean.h step 2, in its order: PRISIM_IMCLEAN_THRESHOLD (also when nothing in the window is valid; P0 is
 *        then NaN), PRISIM_IMCLEAN_MAXITER, PRISIM_CSCLEAN_DIVERGED, PRISIM_CSCLEAN_MAJOR.  PRISIM_IMCLEAN_DEAD where Wtot = 0 (the
 *        band's sum with chan_avg).
 *     3. the minor cycle of prisim_csclean.h step 3 on R' = F[:, kc], down to L = max(thr, cycle_depth * Pc).  A component is (q, a)
 *        with c_flat = gain * R'[q] and a = c_flat * s[q][kc]: the true flux goes into the list.  The update is
 *        R'[p] -= c_flat * P[kc][i_p - i_q][j_p - j_q] for ALL pixels.  A masked pixel holds NaN, stays NaN and never wins the
 *        comparison: the mask of the minor cycle is the NaNs of F, nothing else.
 *     4. the major cycle: for all (t, b) and the channel (every channel with chan_avg),
 *            Vres -= sum_j (a_j * A[t][q_j][k]) * (cos phi_j, -sin phi_j)
 *        over the cycle's new components in list order, phi_j = 2 pi f_k b . dd[t][q_j] / c from the channel's true frequency.  Then
 *        R_N is the mosaic's numerator of Vres, per snapshot from the beam table, as the first residual of prisim_clean_mosaic is.  A
 *        channel that has ended keeps its visibilities and gets the same bits again; a component below the horizon in snapshot t has
 *        A = 0 there and contributes nothing.
 *
 * The minor cycle of a channel is one workgroup; its working image lives in LDS (PRISIM_CSCLEAN_LDS) or in a device scratch
 * (PRISIM_CSCLEAN_GLOBAL), with the same bits.  The host reads 16 bytes once per major cycle and starts max_major + 1 cycles at most.
 * With maxiter = 0 or max_major = 0 the call is prisim_mosaic_image, bit for bit.  Everything is resident within `budget_bytes`: what
 * prisim_clean_mosaic holds, and Vres, P with the buffers of its half-plane and its weight sums, the cycle state and tables, the
 * scale and the scratch of the GLOBAL route; a call that does not fit is refused with the bytes it needs.
 *
 * Accuracy.  P is that of prisim_csclean.h and carries its law: 1e-12 + 2 pi u 13 N_delta, on the phase of the lattice and not on the
 * baseline in wavelengths.  The numerator of every major cycle carries the law of prisim_mosaic.h, and a component's visibilities
 * A[t][q] a e^{-i phi_q} the chain of its pixel's direction (prisim_imaging.h) and 1e-12 |a| of the beam.  tests/mosaic_reference.py
 * holds all three to a 40-digit reference from 300 m to 2400 km.
 *
 * Deterministic: one GPU, one stream, no atomics; every sum in the order of the entries it is taken from.
 */
#ifndef PRISIM_MOSCS_H
#define PRISIM_MOSCS_H

#include <stdint.h>

#include "prisim_csclean.h"
#include "prisim_hip.h"
#include "prisim_imaging.h"
#include "prisim_imclean.h"
#include "prisim_mosaic.h"
#include "prisim_mosclean.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The statuses are PRISIM_IMCLEAN_THRESHOLD, _MAXITER, _DEAD and PRISIM_CSCLEAN_MAJOR, _DIVERGED; the routes PRISIM_IMAGE_* and
 * PRISIM_CSCLEAN_AUTO, _LDS, _GLOBAL. */

typedef struct prisim_moscs_stats {
  double wall_ms;          /* the whole call on the host clock, copies included */
  double kernel_ms;        /* psf_ms + beam_ms + mosaic_ms + peak_ms + minor_ms + model_ms + restore_ms */
  double psf_ms;           /* P: its weight sums, the offsets, the half-plane by the dirty image's kernel, the mirror (stream events) */
  double mosaic_ms;        /* the mosaic passes: the first and one per major cycle, directions and weight sums included */
  double peak_ms;          /* the search images, the start-of-cycle peak searches and decisions */
  double minor_ms;         /* the minor cycles */
  double model_ms;         /* the updates of Vres */
  double restore_ms;       /* the last search image, the division and the restoration */
  int64_t terms;           /* npix * nbl * nchan * nt: of one mosaic pass */
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
  int32_t chan_tile;       /* channels per thread of a mosaic pass */
  int32_t reseed;          /* STEPPED: channels between two seeds from the true frequency; DIRECT: 1 */
  int32_t lds_bytes;       /* LDS per workgroup of a mosaic pass */
  int32_t minor_lds_bytes; /* LDS per workgroup of the minor cycle */
  int32_t block_pixels;    /* pixels per workgroup of a mosaic pass, one per thread */
  double beam_ms;          /* the beam table, the horizon pass and the scale, once per call */
} prisim_moscs_stats;

typedef struct prisim_moscs_args {
  int64_t npix, nbl, nchan, nt;  /* the fields of prisim_mosclean_args less its polling, in their order; npix <= 2^28 */
  const double* unitvec;         /* [npix][3] = [ny][nx][3] */
  const double* rot;             /* [nt][9] */
  const double* aberr_beta;      /* [nt][3] or NULL */
  const double* pc_dircos;       /* [nt][3] the phase centres */
  const double* baselines;       /* [nbl][3] */
  const double* freqs_hz;        /* [nchan] */
  const double* cube;            /* [nt][nbl][nchan] complex128 on the host; or NULL: the context's resident slots [0, nt), copied
                                    on the device behind the context's stream, never written */
  const double* weights;         /* by weight_form */
  int32_t weight_form;           /* PRISIM_IMAGE_W_* */
  int32_t chan_avg;              /* 0: every channel cleaned on its own; 1: the band's mosaic cleaned, nc = 1 */
  int32_t route;                 /* PRISIM_IMAGE_AUTO or the route itself, of the mosaic passes and of P */
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
  int64_t ny, nx;                /* the lattice: ny * nx == npix, nx fastest */
  double  cycle_depth;           /* in (0, 1): a minor cycle runs down to this fraction of its first peak */
  int64_t cycle_niter;           /* components per channel and cycle at most; <= 0: no cap */
  int32_t max_major;             /* major cycles at most, in [0, PRISIM_CSCLEAN_MAX_MAJOR]; 0: the call is a mosaic */
  int32_t minor_route;           /* PRISIM_CSCLEAN_AUTO (LDS when the image fits) or the route itself */
} prisim_moscs_args;

/* out_residual, out_restored, out_residual_flat, out_pb_eff, out_num, out_den, out_wsum, out_comp_pixel, out_comp_flux, out_ncomp,
 *     out_status, out_peak0: as prisim_clean_mosaic; the status is PRISIM_IMCLEAN_THRESHOLD, _MAXITER, _DEAD, PRISIM_CSCLEAN_MAJOR or
 *     _DIVERGED.  out_num is the mosaic's numerator of out_vres, bit for bit.
 * out_ncycles [nc], out_cycle_ncomp [nc][max_major], out_cycle_peak [nc][max_major + 1] (in the units of F), out_psf
 *     [nc][2 ny - 1][2 nx - 1] or NULL, out_vres [nt][nbl][nchan] complex128 or NULL: as prisim_clean_image_cs defines them.
 * stats may be NULL.  Every validation happens before any device work, and nothing is written unless the call succeeds.
 * PRISIM_EINVAL: what prisim_clean_mosaic and prisim_clean_image_cs refuse of these arguments, by their own checks; a budget that
 * does not hold the resident buffers (the message names the bytes needed).
 * PRISIM_ESTATE: cube == NULL and no resident cube at all. */
int prisim_clean_mosaic_cs(prisim_ctx* ctx, const prisim_moscs_args* a, double* out_residual, double* out_restored, double* out_residual_flat,
                           double* out_pb_eff, double* out_num, double* out_den, double* out_wsum, int32_t* out_comp_pixel,
                           double* out_comp_flux, int32_t* out_ncomp, int32_t* out_status, double* out_peak0, int32_t* out_ncycles,
                           int32_t* out_cycle_ncomp, double* out_cycle_peak, double* out_psf, double* out_vres, prisim_moscs_stats* stats);

#ifdef __cplusplus
}
#endif

#endif /* PRISIM_MOSCS_H */
