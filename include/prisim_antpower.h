/*
 * prisim_antpower.h -- the power an antenna receives from the sky, per snapshot (LST) and channel, reduced on the GPU
 * (libprisim_hip.so, prisim_amd/csrc_antpower/antpower.hip).
 *
 * prisim/interferometry.py:antenna_power (:2169-2408) of the reference: for every LST the primary beam is evaluated on the sources
 * above the horizon and
 *     power[t][f] = sum_s pb(s, f) S_s(f) / sum_s pb(s, f).
 * With a diffuse model in kelvin this is the antenna temperature, with point sources the beam-weighted flux.  Here the rotation into
 * the local frame, the beam (the fused kernel of prisim_hip_set_sky_analytic, with unit flux) and the two sums run on the device: an
 * nsrc x nchan array never leaves it and only nsnap x nchan doubles per output come back.
 *
 * Conventions as in prisim_cpreal.h: C-contiguous caller-owned host arrays, 0 or a negative PRISIM_E* code, the message from
 * prisim_hip_last_error().  The entry uses only the context's device, creates and destroys its own streams and device buffers, and
 * neither reads nor disturbs the context's array, sky or catalogue.  The sources are streamed in spans (contiguous ranges of catalogue
 * indices) whose buffers and the partial sums in flight take no more than `budget_bytes` of device memory; the uploaded catalogue
 * (unit vectors 24 B per source, flux_ref and spindex 16 B, or the spectra 8 B per source and channel) is outside that budget.
 *
 * The sums are deterministic: every source keeps its place in a fixed summation order that depends on (nsrc, nchan) alone, sources
 * below the horizon included (they are evaluated and skipped, never compacted away), and no atomic is used.  The outputs are
 * bit-identical for any budget.
 */
#ifndef PRISIM_ANTPOWER_H
#define PRISIM_ANTPOWER_H

#include <stdint.h>

#include "prisim_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct prisim_antpower_stats {
  double wall_ms;             /* the whole call on the host clock, copies included */
  double kernel_ms;           /* the kernels of all snapshots, from stream events, summed over the streams (which overlap) */
  int64_t sources_evaluated;  /* beam evaluations per channel: nsnap * nsrc, below the horizon included */
  int64_t sources_up;         /* (snapshot, source) pairs with s_z >= 0: the terms of the sums */
  int64_t spans;              /* spans a snapshot's sources were streamed in */
  int64_t span_sources;       /* sources per full span, a multiple of block_sources */
  int64_t block_sources;      /* consecutive catalogue sources one workgroup sums (fixed by nsrc and nchan) */
  int64_t kernel_bytes;       /* bytes the kernels read and write in device memory, counted from the algorithm */
  int64_t upload_bytes;       /* bytes copied to the device */
  int64_t download_bytes;     /* bytes copied back to the host */
  int32_t streams;            /* streams the snapshots were dealt to */
  int32_t chan_tile;          /* channels per workgroup of the reduction */
  int32_t lds_bytes;          /* LDS per workgroup of the reduction */
  int32_t reserved_;
} prisim_antpower_stats;

typedef struct prisim_antpower_args {
  int64_t nsrc, nchan, nsnap;   /* sources, channels, snapshots (LSTs): each >= 1, nchan <= 2^20 */
  const double* unitvec;        /* [nsrc][3] catalogue-frame unit vectors (as prisim_catalog.unitvec), |u| = 1 to 1e-6 */
  const double* flux_ref;       /* [nsrc]   power law S = flux_ref (f / ref_freq_hz)^spindex, evaluated on the device ... */
  const double* spindex;        /* [nsrc] */
  double        ref_freq_hz;    /* > 0 with a power law; not read with spectra */
  const double* flux_spectrum;  /* ... or [nsrc][nchan]; non-NULL replaces the power law */
  const double* freqs_hz;       /* [nchan], positive and finite; need not be the context's array grid */
  const double* cel2enu;        /* [nsnap][9] row-major rotation catalogue frame -> East-North-Up, orthonormal to 1e-9
                                   (prisim_snapshot.cel2enu) */
  const double* aberr_beta;     /* [nsnap][3] aberration velocity / c in the catalogue frame, |beta| < 0.01; or NULL = none */
  int32_t beam_kind; int32_t reserved_;   /* PRISIM_BEAM_* */
  double  diameter_m;           /* dish diameter / dipole length; not read for PRISIM_BEAM_DELTA and PRISIM_BEAM_POLY */
  double  beam_pc_dircos[3];    /* element pointing, East-North-Up (zenith for every case the reference reaches) */
  const prisim_beam_ext* ext;   /* NULL, or n_ext structs: dipole axis, array factor, ground plane, beamformer, polynomial */
  int64_t n_ext;                /* 0, 1 (shared) or nsnap (one per snapshot: a beamformer's delays follow the pointing) */
  int64_t budget_bytes;         /* device bytes of the per-span buffers and the partial sums; <= 0: 1 GiB */
} prisim_antpower_args;

/* With s = normalise(R_t (u + beta_t)) the East-North-Up direction of source u at snapshot t, pb the power pattern of the beam
 * (beam_kind, diameter_m, beam_pc_dircos, ext[n_ext == nsnap ? t : 0]) at (s, f) and S the flux of the source at f, over the sources
 * with s_z >= 0 (the reference's alt >= 0.0, :2398):
 *     out_num[t][f] = sum pb S,   out_den[t][f] = sum pb,   out_power[t][f] = out_num / out_den     (IEEE division)
 * in fp64, products and sums unfused, in a fixed order.  A snapshot with no source up, or with out_den == 0, gives NaN in out_power
 * as the reference does (0 / 0): an antenna temperature of 0 would be a wrong answer that looks right.
 * out_power [nsnap][nchan]; out_num, out_den [nsnap][nchan] or NULL; stats may be NULL.  Nothing is written unless the call succeeds.
 * PRISIM_EINVAL: a null a, out_power, unitvec, freqs_hz or cel2enu; a size < 1, nchan above 2^20 or nsrc * nchan beyond the span
 * arithmetic (2^46); neither a power law (flux_ref and spindex) nor a spectrum; ref_freq_hz <= 0 with a power law; a frequency that is
 * not positive and finite; a unit vector whose norm is off by more than 1e-6; a rotation that is not orthonormal to 1e-9 or a
 * |beta| >= 0.01; n_ext not 0, 1 or nsnap, or ext null with n_ext > 0; what the fused beam refuses in beam_kind, diameter_m and every
 * ext (prisim_hip_set_sky_analytic); a budget that cannot hold one block of sources; for PRISIM_BEAM_POLY, the reference's two
 * validity messages (a NaN, or a value of 1.01 and more). */
int prisim_antenna_power(prisim_ctx* ctx, const prisim_antpower_args* a, double* out_power, double* out_num, double* out_den,
                         prisim_antpower_stats* stats);

#ifdef __cplusplus
}
#endif

#endif /* PRISIM_ANTPOWER_H */
