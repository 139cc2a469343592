/*
 * prisim_imclean.h -- Hogbom CLEAN of the dirty image of a visibility cube with the exact beam, on the GPU
 * (libprisim_hip.so, prisim_amd/csrc_imaging/imclean.hip).
 *
 * prisim_dirty_image (prisim_imaging.h) shows every source convolved with the sidelobes of every other one.  This entry takes them
 * apart in image space, with the vocabulary of the delay-space CLEAN (prisim_clean.h: gain, maxiter, threshold, relative or
 * absolute).  Notation of prisim_imaging.h: dd[t][p] = s[p][t] - s0[t], W[k] the weight sums, R0[p][k] the dirty image of the call
 * (nc = nchan image channels, or nc = 1 with chan_avg), window[p] the pixels that may hold components.  In fp64 throughout:
 *
 *   threshold   P0[k] = max_{p in window} |R0[p][k]|; thr[k] = threshold * P0[k] (relative) or threshold (absolute).
 *   pick        for every image channel still active, q = argmax_{p in window} |R[p][k]|: compared by > on |.|, the lowest p wins a
 *               tie, a NaN never wins.  |R[q][k]| <= thr[k] ends the channel with PRISIM_IMCLEAN_THRESHOLD; otherwise maxiter
 *               components already held end it with PRISIM_IMCLEAN_MAXITER; otherwise the component (q, a = gain * R[q][k]) is
 *               appended to the channel's list.
 *   update      for ALL pixels R[p][k] -= B[p][k],
 *                   B[p][k] = (sum_t sum_b w[t][b][k] a_k cos(2 pi f_k b . (dd[t][p] - dd[t][q_k]) / c)) / W[k]
 *               and with chan_avg, one (q, a) for the band, B[p] = a sum_k sum_t sum_b w cos(...) / sum_k W[k].
 *
 * B is the dirty image of the component's own visibilities a e^{-i phi_q}: the exact beam at that place, w-term and frames included,
 * with no shift invariance assumed.  So the residual always is the dirty image of V - sum of the components' visibilities, to
 * rounding, and a step is one of matching pursuit in the weighted visibility space: sum w |V_res|^2 cannot grow for 0 < gain <= 1.
 * That is why there is no divergence guard here.
 *
 * A channel whose W[k] is 0 is PRISIM_IMCLEAN_DEAD from the start: its residual is NaN as in prisim_dirty_image, it holds no
 * components and it never delays the others.  A channel that has ended has a = 0 from then on and its residual keeps its bits: its
 * tiles are skipped, nothing is recomputed.
 *
 * Conventions as in prisim_imaging.h.  dd of all pixels, the residual, the component lists and the window are resident on the device
 * for the whole call, within `budget_bytes`; an image that does not fit is refused with the bytes it needs -- nothing is streamed in
 * pixel chunks here.  The uploaded tables (cube, weights, baselines, frames, directions, frequencies) are outside that budget.  The
 * device never waits for the host inside an iteration: the picks are published in device memory, iterations are enqueued `poll_every`
 * at a time, and after each batch the host reads 16 bytes (the channels still active, the iterations that had any) and stops at 0.  No result depends on
 * poll_every: an iteration with nothing active does nothing.
 *
 * Deterministic: the update adds the (t, b) terms of a (pixel, channel) in one thread, t ascending and b ascending inside t, as
 * prisim_dirty_image does; the peak search is a tree of (|value|, index) pairs under an associative rule; no atomic is used.
 */
#ifndef PRISIM_IMCLEAN_H
#define PRISIM_IMCLEAN_H

#include <stdint.h>

#include "prisim_hip.h"
#include "prisim_imaging.h"

#ifdef __cplusplus
extern "C" {
#endif

/* out_status: how an image channel ended */
enum { PRISIM_IMCLEAN_THRESHOLD = 1, PRISIM_IMCLEAN_MAXITER = 2, PRISIM_IMCLEAN_DEAD = 4 };
/* iterations enqueued between two reads of the active count when poll_every <= 0, and at most */
enum { PRISIM_IMCLEAN_POLL_DEFAULT = 32, PRISIM_IMCLEAN_POLL_MAX = 1024 };

typedef struct prisim_imclean_stats {
  double wall_ms;          /* the whole call on the host clock, copies included */
  double kernel_ms;        /* dirty_ms + peak_ms + update_ms + restore_ms */
  double dirty_ms;         /* the initial dirty image: directions, weight sums, the sum, the band average (stream events) */
  double peak_ms;          /* the peak searches of all iterations */
  double update_ms;        /* the updates of all iterations */
  double restore_ms;       /* the restoration */
  int64_t terms;           /* npix * nbl * nchan * nt: of the dirty image and of every update */
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
  int32_t chan_tile;       /* channels per thread of the dirty image and of the update */
  int32_t reseed;          /* STEPPED: channels between two seeds from the true frequency; DIRECT: 1 */
  int32_t lds_bytes;       /* LDS per workgroup of the update */
  int32_t block_pixels;    /* pixels per workgroup, one per thread */
} prisim_imclean_stats;

typedef struct prisim_imclean_args {
  int64_t npix, nbl, nchan, nt;  /* as prisim_imaging_args; npix <= 2^28 */
  const double* unitvec;         /* [npix][3] */
  const double* rot;             /* [nt][9] */
  const double* aberr_beta;      /* [nt][3] or NULL */
  const double* pc_dircos;       /* [nt][3] */
  const double* baselines;       /* [nbl][3] */
  const double* freqs_hz;        /* [nchan] */
  const double* cube;            /* [nt][nbl][nchan] complex128 on the host; or NULL: the context's resident slots [0, nt), read
                                    where they lie behind the context's stream, never written or copied */
  const double* weights;         /* by weight_form */
  const uint8_t* window;         /* [npix] non-zero: the pixel may hold components; or NULL: every pixel.  All zero: PRISIM_EINVAL */
  const double* fwhm_rad;        /* [nc] the restoring beam per image channel, > 0 and finite; or NULL: no restoration */
  double gain;                   /* in (0, 1] */
  double threshold;              /* finite and >= 0; relative: < 1 */
  int64_t maxiter;               /* components per image channel at most, >= 0; 0: the residual is the dirty image bit for bit */
  int64_t budget_bytes;          /* device bytes of the resident buffers; <= 0: 1 GiB */
  int32_t weight_form;           /* PRISIM_IMAGE_W_* */
  int32_t chan_avg;              /* 0: every channel cleaned on its own; 1: the band's image cleaned, nc = 1 */
  int32_t route;                 /* PRISIM_IMAGE_AUTO or the route itself, of the dirty image and of the updates */
  int32_t threshold_relative;    /* 0: absolute; 1: a fraction of P0[k] */
  int32_t poll_every;            /* iterations per batch; <= 0: PRISIM_IMCLEAN_POLL_DEFAULT; at most PRISIM_IMCLEAN_POLL_MAX are taken */
  int32_t reserved_;
} prisim_imclean_args;

/* out_residual [npix][nc]: R when every channel has ended.
 * out_restored [npix][nc] or NULL (then fwhm_rad is not read): R[p][k] + sum over the components (q, a) of k, in list order, of
 *     a exp(-4 ln 2 theta^2 / fwhm_k^2), theta = 2 asin(min(1, |u_p - u_q| / 2)) the angle between the two directions in their own frame.
 * out_comp_pixel, out_comp_flux [nc][maxiter]: the lists; of row k the first out_ncomp[k] entries are written, the others left alone.
 * out_ncomp, out_status [nc]: the components held and PRISIM_IMCLEAN_THRESHOLD, _MAXITER or _DEAD.
 * out_peak0 [nc]: P0 (NaN for a dead channel).  out_wsum [nc] or NULL: as prisim_dirty_image.  stats may be NULL.
 * Every validation happens before any device work, and nothing is written unless the call succeeds.
 * PRISIM_EINVAL: what prisim_dirty_image refuses of these arguments; a null out_residual, out_comp_pixel, out_comp_flux, out_ncomp,
 * out_status or out_peak0; out_restored without fwhm_rad; a gain outside (0, 1]; maxiter < 0 or beyond 2^30; a threshold that is
 * negative or not finite, or >= 1 when relative; a window without a pixel; an fwhm_rad that is not positive and finite; npix beyond
 * 2^28; a budget that does not hold the whole image (the message names the bytes needed).
 * PRISIM_ESTATE: cube == NULL and no resident cube at all. */
int prisim_clean_image(prisim_ctx* ctx, const prisim_imclean_args* a, double* out_residual, double* out_restored, int32_t* out_comp_pixel,
                       double* out_comp_flux, int32_t* out_ncomp, int32_t* out_status, double* out_peak0, double* out_wsum,
                       prisim_imclean_stats* stats);

#ifdef __cplusplus
}
#endif

#endif /* PRISIM_IMCLEAN_H */
