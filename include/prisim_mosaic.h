/*
 * prisim_mosaic.h -- the beam-weighted linear mosaic of the snapshots of a visibility cube, on the GPU
 * (libprisim_hip.so, prisim_amd/csrc_imaging/mosaic.hip).
 *
 * prisim_dirty_image (prisim_imaging.h) gives apparent fluxes: what the array sees through its primary beam.  A drift scan moves that
 * beam across the sky from snapshot to snapshot, and a chromatic beam changes it from channel to channel, so no single beam divides the
 * finished image back to true fluxes.  Here the beam goes in per snapshot, before the snapshots are added: with D_t the direct Fourier
 * sum of snapshot t alone, W_t its weight sum and A_t the power pattern of the primary beam at the pixel,
 *     mosaic = sum_t A_t D_t / sum_t A_t^2 W_t,
 * the least-squares estimate of the true flux of a pixel from the snapshots.  A source of true flux S simulated through this beam has
 * D_t = A_t S W_t at its own pixel, so the mosaic returns S for any number of snapshots, any drift and any beam chromaticity.
 *
 * Conventions as in prisim_imaging.h, whose direct Fourier sum, routes, weight forms, chunks and resident cube this entry shares, and
 * prisim_antpower.h, whose beam description (the fused analytic beam of prisim_hip_set_sky_analytic, with unit flux) it takes.  The sum
 * is deterministic: every (pixel, channel) adds its b terms in one thread, b ascending, and its snapshots in that same thread, t
 * ascending.  No atomic is used and no sum is split over workgroups: the outputs are bit-identical for any budget and stream count.
 *
 * Accuracy.  D_t is the sum of prisim_dirty_image and carries its law (prisim_imaging.h: 1e-11 + 2 pi u (13 N_b + 7 N') of the natural
 * scale, N_b the longest baseline in wavelengths), the beam is within 1e-12 of the exact pattern, W_t has no phase in it.  So per element
 *     |N - N_exact| <= sum_t (1e-11 + 2 pi u (13 N_b + 7 N'_t)) A_t sum_b w|V| + 1e-12 sum_{t,b} w|V|
 *     |Q - Q_exact| <= 1e-11 sum_t A_t^2 W_t + 2e-12 sum_t A_t W_t
 * and like the image the mosaic keeps 1e-11 of its scale to baselines of some 1e5 wavelengths as measured (7e2 by the bound), however
 * narrow the field.  tests/mosaic_reference.py counts this and holds the device to it against a 40-digit reference from 300 m to
 * 2400 km; measured, N is at most 0.09 of the bound and Q at 1e-3 of its own.  The horizon test and the mask compare rounded numbers:
 * a direction within some 1e-15 of the horizon, or a Q within rounding of pbmin^2 Wtot, may fall on either side.
 */
#ifndef PRISIM_MOSAIC_H
#define PRISIM_MOSAIC_H

#include <stdint.h>

#include "prisim_hip.h"
#include "prisim_imaging.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct prisim_mosaic_stats {
  double wall_ms;          /* the whole call on the host clock, copies included */
  double kernel_ms;        /* the kernels of all chunks, from stream events, summed over the streams (which overlap) */
  int64_t terms;          /* npix * nbl * nchan * nt */
  int64_t beam_values;     /* npix * nchan * nt: evaluations of the beam, below the horizon included */
  int64_t chunks;          /* chunks the pixels were streamed in */
  int64_t chunk_pixels;    /* pixels per full chunk, a multiple of block_pixels */
  int64_t pixel_bytes;     /* device bytes one pixel of a chunk takes: 64 nt + 24 nchan + (chan_avg ? 16 : 16 nchan) */
  int64_t kernel_bytes;    /* bytes the kernels read and write in device memory, counted from the algorithm */
  int64_t upload_bytes;    /* bytes copied to the device */
  int64_t download_bytes;  /* bytes copied back to the host */
  int32_t route;           /* PRISIM_IMAGE_DIRECT or PRISIM_IMAGE_STEPPED */
  int32_t streams;         /* streams the chunks were dealt to */
  int32_t chan_tile;       /* channels per thread: its accumulators, one double each */
  int32_t reseed;          /* STEPPED: channels between two seeds from the true frequency; DIRECT: 1 */
  int32_t lds_bytes;       /* LDS per workgroup: the staged rows of the visibility operand */
  int32_t block_pixels;    /* pixels per workgroup, one per thread */
} prisim_mosaic_stats;

typedef struct prisim_mosaic_args {
  int64_t npix, nbl, nchan, nt;  /* as prisim_imaging_args, field by field, less `kind` */
  const double* unitvec;         /* [npix][3] */
  const double* rot;             /* [nt][9] */
  const double* aberr_beta;      /* [nt][3] or NULL */
  const double* pc_dircos;       /* [nt][3] the phase centres */
  const double* baselines;       /* [nbl][3] */
  const double* freqs_hz;        /* [nchan] */
  const double* cube;            /* [nt][nbl][nchan] complex128, or NULL: the context's resident slots [0, nt) */
  const double* weights;         /* by weight_form */
  int32_t weight_form;           /* PRISIM_IMAGE_W_* */
  int32_t chan_avg;              /* 0: one mosaic per channel; 1: one of the band */
  int32_t route;                 /* PRISIM_IMAGE_AUTO or the route itself */
  int32_t beam_kind;             /* PRISIM_BEAM_*: the beam of prisim_antpower_args */
  double  diameter_m;            /* dish diameter / dipole length; not read for PRISIM_BEAM_DELTA and PRISIM_BEAM_POLY */
  double  beam_pc_dircos[3];     /* element pointing, East-North-Up, of every snapshot (a drift scan), unless ... */
  const double* beam_pc_snap;    /* ... [nt][3], finite: the element pointing of each snapshot (a tracking dish); or NULL */
  const prisim_beam_ext* ext;    /* NULL, or n_ext structs */
  int64_t n_ext;                 /* 0, 1 (shared) or nt (one per snapshot: a beamformer's delays follow the pointing) */
  double  pbmin;                 /* in [0, 1): a pixel is kept where its effective beam is at least pbmin; 0 masks Q == 0 only */
  int64_t budget_bytes;          /* device bytes of the per-chunk buffers; <= 0: 1 GiB */
} prisim_mosaic_args;

/* With s[p][t], phi, w and V exactly as in prisim_imaging.h, and A[t][p][k] the power pattern of the beam (beam_kind, diameter_m,
 * beam_pc_snap[t] or beam_pc_dircos, ext[n_ext == nt ? t : 0]) at (s[p][t], f_k), set to 0 where s_z < 0 (the horizon mask), in fp64
 * and in this order:
 *     D_t[p][k] = sum_b w[t][b][k] (Re V cos phi - Im V sin phi)          b ascending
 *     W_t[k]    = sum_b w[t][b][k]                                        b ascending
 *     N[p][k]   = sum_t A D_t                                             t ascending from 0, N = fma(A, D_t, N)
 *     Q[p][k]   = sum_t A^2 W_t                                           t ascending from 0, Q = fma(A * A, W_t, Q)
 *     Wtot[k]   = sum_t W_t[k]                                            t ascending
 *     out_mosaic[p][k] = N / Q          where Q >= (pbmin * pbmin) * Wtot[k], else NaN         chan_avg = 0: [npix][nchan]
 *     out_pb_eff[p][k] = sqrt(Q / Wtot[k])                                the effective beam; the noise of the mosaic goes as 1 / pb_eff
 *     chan_avg = 1: out_mosaic[p] = sum_k N / sum_k Q where sum_k Q >= (pbmin * pbmin) * sum_k Wtot, else NaN, and
 *                   out_pb_eff[p] = sqrt(sum_k Q / sum_k Wtot), the sums over k ascending: [npix]
 * (IEEE division and square root).  out_num and out_den are N and Q, [npix][nchan] whatever chan_avg is; out_wsum is Wtot, [nchan].
 * out_pb_eff, out_num, out_den, out_wsum and stats may be NULL.  A pixel below the horizon in every snapshot, and a channel without
 * weight, have Q == 0 and come back NaN (0 / 0), not as a plausible 0.  With a delta beam, nt = 1 and every direction up, out_mosaic
 * has the bits of prisim_dirty_image and out_den == out_wsum.
 * Nothing is written unless the call succeeds.
 * PRISIM_EINVAL: what prisim_dirty_image refuses in the fields the two share (out_mosaic in the place of out_image); n_ext not 0, 1 or
 * nt, or ext null with n_ext > 0; what the fused beam refuses in beam_kind, diameter_m and every ext; a beam_pc_snap row that is not
 * finite; pbmin outside [0, 1) or not finite; for PRISIM_BEAM_POLY, the two validity messages of prisim_antenna_power.
 * PRISIM_ESTATE: cube == NULL and no resident cube at all. */
int prisim_mosaic_image(prisim_ctx* ctx, const prisim_mosaic_args* a, double* out_mosaic, double* out_pb_eff, double* out_num,
                        double* out_den, double* out_wsum, prisim_mosaic_stats* stats);

#ifdef __cplusplus
}
#endif

#endif /* PRISIM_MOSAIC_H */
