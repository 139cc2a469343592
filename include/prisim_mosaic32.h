/*
 * prisim_mosaic32.h -- the beam-weighted linear mosaic of the snapshots of a visibility cube with the per-term arithmetic of every
 * snapshot's sum in fp32, on the GPU (libprisim_hip.so, prisim_amd/csrc_imaging/mosaic32.hip).
 *
 * The mosaic of prisim_mosaic.h, for the user who ran the simulation in its float32 mode: a mosaic of a cube that is good to 1e-6 does
 * not need 1e-11 arithmetic in every snapshot.  One entry, prisim_mosaic_image_f32, with the arguments, the outputs, the layouts, the
 * conventions and the refusals of prisim_mosaic_image; both structs and all enums are those of prisim_mosaic.h and prisim_imaging.h.
 * The cube stays complex128, on the host or in the context's resident slots; every output stays float64.
 *
 * N, Q, Wtot, the mask, out_pb_eff and the chan_avg form are those of prisim_mosaic.h, statement for statement.  What is
 * fp64 and what is fp32 is the division of prisim_imaging32.h applied per snapshot:
 *   fp64, unchanged: the directions s[p][t] and their offsets from the phase centre; tau = b . (s - s0) / c; the products f tau and
 *     df tau and their reduction; the beam A_t (the fused analytic beam with unit flux); W_t, Wtot and their band sum; the totals
 *     D_t[p][k] that take the partial sums; N = fma(A, D_t, N) and Q = fma(A * A, W_t, Q); the division, the mask and the square root.
 *   fp32: the sine and the cosine of the reduced seed phase and of the reduced step phase; the operand (w Re V, w Im V), formed in fp64
 *     and rounded once; the recurrence that carries the phasor from channel to channel; the partial sums of at most 32 terms.
 * So out_den, out_wsum, out_pb_eff and the position of every NaN have the bits of prisim_mosaic_image on the same arguments: their
 * statements are untouched.  Only N differs, and out_mosaic with it.  With a delta beam, nt = 1 and every direction up, out_mosaic has
 * the bits of prisim_dirty_image_f32.
 *
 * The chain of a snapshot is that of prisim_imaging32.h: a thread owns a pixel and a tile of 32 channels, seeds the phasor at the
 * tile's centre channel and walks it up and down; the baselines are taken 64 at a time, two to a packed chain, and after every 64 (and
 * at the end of the snapshot) the fp32 partial sums are added into the fp64 totals.  Every (pixel, channel) is added by one thread in an
 * order fixed by (nt, nbl) alone, and no atomic is used: the outputs are bit-identical for any budget and either number of streams.
 *
 * Routes.  PRISIM_IMAGE_AUTO and PRISIM_IMAGE_STEPPED on a grid that is uniform by the rule of prisim_imaging.h.  There is no fp32
 * DIRECT form: PRISIM_IMAGE_DIRECT, and a grid that is not uniform with either of the other two, are PRISIM_EINVAL with a message
 * that names prisim_mosaic_image.
 *
 * Accuracy.  Per element |N - N_64| <= 5e-6 sum_t A_t sum_b w|V|: the bound of prisim_imaging32.h holds for every D_t, A_t <= 1
 * carries it through the sum over t by the triangle inequality, and the fp64 multiply-adds of the epilogue add nothing visible at that
 * scale.  The phase range is that of prisim_dirty_image, refused in the same sentence.
 */
#ifndef PRISIM_MOSAIC32_H
#define PRISIM_MOSAIC32_H

#include <stdint.h>

#include "prisim_mosaic.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The outputs as prisim_mosaic_image states them, with the terms of D_t formed and summed as above.  stats: route is
 * PRISIM_IMAGE_STEPPED, chan_tile 32, reseed 32 (one seed per tile, at its centre), lds_bytes and block_pixels those of this entry's
 * kernel; pixel_bytes and the chunks are those of prisim_mosaic_image for the same sizes and budget.  out_pb_eff, out_num, out_den,
 * out_wsum and stats may be NULL.
 * Nothing is written unless the call succeeds.
 * PRISIM_EINVAL: what prisim_mosaic_image refuses, in its sentences; PRISIM_IMAGE_DIRECT; a grid that is not uniform.
 * PRISIM_ESTATE: cube == NULL and no resident cube at all. */
int prisim_mosaic_image_f32(prisim_ctx* ctx, const prisim_mosaic_args* a, double* out_mosaic, double* out_pb_eff, double* out_num,
                            double* out_den, double* out_wsum, prisim_mosaic_stats* stats);

#ifdef __cplusplus
}
#endif

#endif /* PRISIM_MOSAIC32_H */
