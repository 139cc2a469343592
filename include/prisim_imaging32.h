/*
 * prisim_imaging32.h -- the dirty image and the synthesized beam of a visibility cube by the direct Fourier sum with the per-term
 * arithmetic in fp32, on the GPU (libprisim_hip.so, prisim_amd/csrc_imaging/imaging32.hip).
 *
 * The image of prisim_imaging.h, for the user who ran the simulation in its float32 mode: an image of a cube that is good to 1e-6
 * does not need 1e-11 arithmetic.  One entry, prisim_dirty_image_f32, with the arguments, the outputs, the layouts, the conventions
 * and the refusals of prisim_dirty_image; both structs and all enums are those of prisim_imaging.h.  The cube stays complex128, on the
 * host or in the context's resident slots; out_image and out_wsum stay float64.
 *
 * What is fp64 and what is fp32.
 *   fp64, as in prisim_dirty_image: the directions s[p][t] and their offsets from the phase centre; tau = b . (s - s0) / c; the
 *     products f tau and df tau, and their reduction to a quadrant and a fraction of a cycle; the weight sums W[k], which have the bits
 *     of prisim_dirty_image; the operand (w Re V, w Im V) before it is rounded; the totals D[p][k]; the final division.
 *   fp32: the sine and the cosine of the reduced seed phase and of the reduced step phase (polynomials good to about 1 ulp, not the
 *     hardware's sine and cosine); the operand, rounded once; the recurrence that carries the phasor from channel to channel; the
 *     partial sums of at most 32 terms.
 * So a long baseline costs nothing extra: the phase loses nothing before it is a fraction of a cycle.  The phase range is that of
 * prisim_dirty_image, max|b| * 2 * max|f| / c below 2^29 cycles, refused in the same sentence.
 *
 * The chain.  A thread owns a pixel and a tile of 32 channels from k0 on.  Per (t, b) it seeds the phasor at the tile's centre channel,
 * from fc = f[k0] + 16 df, and walks it up over the channels [16, 32) and down over [0, 16) with the step e^{+-2 pi i df tau}: no
 * phasor is further than 16 complex multiplies from its seed.  The baselines of a snapshot are taken 64 at a time, two to a packed
 * chain; after every 64 (and at the end of a snapshot) the fp32 partial sums are added into the fp64 totals, the even baseline's
 * before the odd one's, and cleared.
 *
 * The sum is deterministic: the order of a (pixel, channel) -- t ascending, b ascending, the points at which the partial sums are
 * added a function of (nt, nbl) alone -- is fixed, one thread adds all of it, and no atomic is used.  The outputs are bit-identical
 * for any budget and either number of streams.
 *
 * Routes.  PRISIM_IMAGE_AUTO and PRISIM_IMAGE_STEPPED on a grid that is uniform by the rule of prisim_imaging.h.  There is no fp32
 * DIRECT form: PRISIM_IMAGE_DIRECT, and a grid that is not uniform with either of the other two, are PRISIM_EINVAL with a message
 * that names prisim_dirty_image.
 *
 * Accuracy.  Every element of every image is within 5e-6 sum w|V| / sum w of the fp64 sum (1 for the beam, the band's scale with
 * chan_avg): the project's bar for its float32 mode.  The count, with e = 2^-24: a term's phasor is off by the seed (about 1.5 e), 16
 * steps of the recurrence (about 2 e each, adding as a random walk unless the step's own error, about 1 e, repeats: 16 e at worst),
 * the rounding of the operand (e) and of the accumulate (e of the running partial sum); a single baseline, where nothing averages,
 * measures 1.5e-6 in the worst of 3000 pixels x 33 channels, and sums of many baselines 1.5e-7 or less.  The partial sums hold 32
 * terms, so a fully coherent sum (every term equal, the beam at the phase centre) loses at most 16 e of its value, 1e-6, before it
 * is in fp64.
 */
#ifndef PRISIM_IMAGING32_H
#define PRISIM_IMAGING32_H

#include <stdint.h>

#include "prisim_imaging.h"

#ifdef __cplusplus
extern "C" {
#endif

/* D, W and out_image as prisim_dirty_image states them, with the terms w (Re V cos phi - Im V sin phi) formed and summed as above.
 * stats: route is PRISIM_IMAGE_STEPPED, chan_tile 32, reseed 32 (one seed per tile, at its centre), lds_bytes and block_pixels those of
 * this entry's kernel.  out_wsum and stats may be NULL.  A zero weight sum gives NaN in out_image.
 * Nothing is written unless the call succeeds.
 * PRISIM_EINVAL: what prisim_dirty_image refuses, in its sentences; PRISIM_IMAGE_DIRECT; a grid that is not uniform.
 * PRISIM_ESTATE: PRISIM_IMAGE_DIRTY with cube == NULL and no resident cube at all (no array set). */
int prisim_dirty_image_f32(prisim_ctx* ctx, const prisim_imaging_args* a, double* out_image, double* out_wsum, prisim_imaging_stats* stats);

#ifdef __cplusplus
}
#endif

#endif /* PRISIM_IMAGING32_H */
