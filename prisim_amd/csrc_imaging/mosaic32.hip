// mosaic32.hip -- the beam-weighted linear mosaic of the snapshots of a visibility cube with the per-term arithmetic of every snapshot's
// sum in fp32, for gfx950 (include/prisim_mosaic32.h): the mosaic of mosaic.hip, sum_t A_t D_t / sum_t A_t^2 W_t, with D_t formed as
// prisim_dirty_image_f32 forms its sum -- the phase and its reduction fp64, the phasor, the recurrence and the partial sums fp32 -- and
// everything else as prisim_mosaic_image has it: the directions, the beam tile, the weight sums, the fp64 totals, both fused
// multiply-adds of the epilogue and the finish.  So Q, wsum, pb_eff and the mask have the bits of the fp64 entry; only N differs.
//
// The host body is mosaic_frame.h's, the one prisim_mosaic_image runs: the checks and their sentences, the tables, the beam of every
// snapshot, the chunk loop, the host buffers that keep a failed call from writing anything.  Here it gets mosaic32_plan
// (../csrc_addon/mosaic32_plan.h) and the sum of mosaic32_kernels.h.
#include <hip/hip_runtime.h>

#include "../../include/prisim_mosaic32.h"
#include "../csrc_addon/mosaic32_plan.h"
#include "mosaic32_kernels.h"
#include "mosaic_frame.h"

namespace {

int mosaic_image_f32(prisim_ctx* ctx, const prisim_mosaic_args* a, double* out_mosaic, double* out_pb_eff, double* out_num, double* out_den,
                     double* out_wsum, prisim_mosaic_stats* stats) {
  return mosaic_frame(ctx, a, out_mosaic, out_pb_eff, out_num, out_den, out_wsum, stats, mosaic32_plan,
                      [](prisim_ctx* c, const MosParams& P, const MosaicPlan& pl, hipStream_t s) {
                        return enqueue_mos32_sum(c, P, pl.block, pl.ntiles, s);
                      });
}

}  // namespace

extern "C" {

int prisim_mosaic_image_f32(prisim_ctx* ctx, const prisim_mosaic_args* a, double* out_mosaic, double* out_pb_eff, double* out_num,
                            double* out_den, double* out_wsum, prisim_mosaic_stats* stats) {
  return guarded(ctx, [&]() -> int { return mosaic_image_f32(ctx, a, out_mosaic, out_pb_eff, out_num, out_den, out_wsum, stats); });
}

}  // extern "C"
