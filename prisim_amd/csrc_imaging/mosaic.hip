// mosaic.hip -- the beam-weighted linear mosaic of the snapshots of a visibility cube for gfx950 (include/prisim_mosaic.h):
// mosaic[p][k] = sum_t A_t D_t / sum_t A_t^2 W_t, with D_t[p][k] = sum_b w (Re V cos phi - Im V sin phi) the direct Fourier sum of
// snapshot t alone (imaging.hip), W_t[k] = sum_b w, and A_t[p][k] the power pattern of the primary beam at the pixel's direction in
// that snapshot, 0 below the horizon.  It joins two statements this library already has and restates neither: the fused analytic beam
// (launch_beam_flux of ../csrc/aux_kernels.hip with unit flux, as antpower.hip calls it) and the tile pass of the direct Fourier sum
// (img_tile_pass of imaging_kernels.h, as it stands, where the hot loop is described).
//
// The kernels and the functions that enqueue them are in mosaic_kernels.h, which prisim_clean_mosaic (mosclean.hip) shares: k_mos_sum<STEPPED>
// is img_tile_pass<STEPPED, false>(...) with the epilogue below.  Once per call:
//   k_mos_wsum   W_t[k] = sum_b w[t][b][k] as [nt][nchan], b ascending, and Wtot[k] = sum_t W_t[k], t ascending; one thread per
//                channel.  k_img_wtot sums Wtot over k for chan_avg.
// Per chunk of pixels (contiguous, a whole number of blocks of 256), on the chunk's stream:
//   k_img_dirs   with both outputs: s[t][pixel] = normalise(R_t (u + beta_t)) as (l, m, n, 0), the rows BeamParams.dirs reads, and
//                dd = s - s0[t].
//   then for t = 0 .. nt - 1, in this order:
//     launch_beam_flux(bp, stream) by enqueue_mos_beam, with unit flux (flux_ref = 1, spindex = 0: pb exp2(0) = pb exactly) on the chunk's directions of snapshot t
//                into pb_tile[count][nchan], the one tile of the stream: 8 nchan bytes a pixel, not 8 nt nchan.
//     k_mos_sum  the hot path, one launch per snapshot: the tile pass of that snapshot on (w Re V, w Im V), the operand of the dirty
//                image.  The epilogue reads the thread's 32 beam values, puts 0 in their place where the direction is below the
//                horizon, and writes N = fma(A, acc, N) and Q = fma(A A, W_t, Q); snapshot 0 starts from 0 and reads nothing.
//                The launch per snapshot is what fixes the order in t, keeps the register budget of k_img_sum (the beam values are
//                read when the accumulators are done, one at a time) and lets one beam tile serve every snapshot; a t loop inside one
//                launch would need the beam of all snapshots resident (8 nt nchan bytes a pixel) or a second set of 32 accumulators
//                for N beside D_t (64 more VGPRs: half the occupancy).  Its price is N and Q read and written once per snapshot,
//                32 B per (pixel, channel, snapshot) against the nbl rows the snapshot stages.
//   k_mos_finish the division, the mask Q >= pbmin^2 Wtot (else NaN) and pb_eff = sqrt(Q / Wtot) per (pixel, channel); or, with
//                chan_avg, k_mos_finish_band: the sums of N and Q over k ascending per pixel, then the same three.
// No atomics, and neither the b sum nor the t sum is split: the bits do not depend on the chunks or the streams.  Built with
// -ffp-contract=off like the other add-ons; the fused multiply-adds are written as fma().  The results are gathered in host buffers and
// copied to the caller's arrays when every chunk is in, so that a failed call writes nothing.
//
// The host body of all this is mosaic_frame.h's, parameterised on the plan and on the sum's enqueue: prisim_mosaic_image_f32
// (mosaic32.hip) runs the same body with mosaic32_plan and the fp32 sum of mosaic32_kernels.h.
#include <hip/hip_runtime.h>

#include "../../include/prisim_mosaic.h"
#include "../csrc_addon/beam_setup.h"
#include "../csrc_addon/mosaic_plan.h"
#include "imaging_kernels.h"
#include "mosaic_kernels.h"
#include "mosaic_frame.h"

namespace {

int mosaic_image(prisim_ctx* ctx, const prisim_mosaic_args* a, double* out_mosaic, double* out_pb_eff, double* out_num, double* out_den,
                 double* out_wsum, prisim_mosaic_stats* stats) {
  return mosaic_frame(ctx, a, out_mosaic, out_pb_eff, out_num, out_den, out_wsum, stats, mosaic_plan,
                      [](prisim_ctx* c, const MosParams& P, const MosaicPlan& pl, hipStream_t s) {
                        return enqueue_mos_sum(c, P, pl.block, pl.ntiles, pl.route == kImagingStepped, s);
                      });
}

}  // namespace

extern "C" {

int prisim_mosaic_image(prisim_ctx* ctx, const prisim_mosaic_args* a, double* out_mosaic, double* out_pb_eff, double* out_num,
                        double* out_den, double* out_wsum, prisim_mosaic_stats* stats) {
  return guarded(ctx, [&]() -> int { return mosaic_image(ctx, a, out_mosaic, out_pb_eff, out_num, out_den, out_wsum, stats); });
}

}  // extern "C"
