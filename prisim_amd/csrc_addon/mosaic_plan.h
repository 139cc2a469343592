// mosaic_plan.h -- how prisim_mosaic_image (../csrc_imaging/mosaic.hip) plans a call: the route, the channel tile, the pixels and the
// LDS of a workgroup are those of prisim_dirty_image, by imaging_plan.h's own rules and constants; the chunks of pixels are planned by
// the same arithmetic over buffers that hold more per pixel.  Plain C++ without HIP, so that a host program can check it
// (tests/test_mosaic.py).  Not part of the public ABI.
#ifndef PRISIM_MOSAIC_PLAN_H
#define PRISIM_MOSAIC_PLAN_H

#include <cstdint>

#include "imaging_plan.h"

namespace pint {

// bytes one pixel of a chunk takes in the buffers of one stream: per snapshot its direction (l, m, n, 0) for the beam and its offset
// from the phase centre for the phase (32 B each); per channel one beam value of the snapshot in hand (8 B, not 8 nt: the tile is
// evaluated, used and overwritten snapshot by snapshot), N and Q (16 B); and the outputs, mosaic and effective beam, per channel
// (16 B) or, with chan_avg, per pixel (16 B):  64 nt + 24 nchan + (chan_avg ? 16 : 16 nchan)
inline int64_t mosaic_pixel_bytes(int64_t nchan, int64_t nt, bool chan_avg) { return 64 * nt + 24 * nchan + (chan_avg ? 16 : 16 * nchan); }

// The plan of a call, field for field that of imaging_plan: AUTO is STEPPED exactly when the grid is uniform, an explicit STEPPED on
// another grid is refused; tile, reseed, block and LDS are the constants of k_img_sum; the chunks are whole numbers of blocks of
// kImagingBlock pixels, the largest of which `nstreams` fit in the budget at mosaic_pixel_bytes a pixel.  refusal: null, or why the
// call cannot run.
using MosaicPlan = ImagingPlan;
inline MosaicPlan mosaic_plan(int64_t npix, int64_t nbl, int64_t nchan, int64_t nt, int weight_form, bool chan_avg, int64_t budget_bytes,
                              int64_t lds_max, int asked, bool uniform, int max_streams) {
  return pixel_plan(npix, nbl, nchan, nt, weight_form, mosaic_pixel_bytes(nchan, nt, chan_avg), budget_bytes, lds_max, asked, uniform,
                    max_streams);
}

}  // namespace pint

#endif  // PRISIM_MOSAIC_PLAN_H
