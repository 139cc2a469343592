// mosaic32_plan.h -- how prisim_mosaic_image_f32 (../csrc_imaging/mosaic32.hip) plans a call.  The chunks of pixels are mosaic_plan's
// (mosaic_plan.h), called and not restated: the chunk buffers are those of the fp64 entry (directions, the beam tile, N, Q and the
// outputs stay fp64), so the chunk lists equal mosaic_plan's span for span.  What the fp32 sum adds are the refusals and the constants of
// imaging32_plan.h, read from there by name.  Plain C++ without HIP, so that a host program can check it (tests/test_mosaic32.py).
// Not part of the public ABI.
#ifndef PRISIM_MOSAIC32_PLAN_H
#define PRISIM_MOSAIC32_PLAN_H

#include <cstdint>

#include "imaging32_plan.h"
#include "mosaic_plan.h"

namespace pint {

// The plan of a call of the fp32 entry, with mosaic_plan's arguments.  It reports the LDS and the reseed interval of the fp32 tile
// pass; the tile and the block are pixel_plan's, which that pass shares.  refusal: null, or why the call cannot run: whatever
// mosaic_plan refuses, the DIRECT route and a grid that is not uniform under AUTO or STEPPED, each in a sentence of its own that names
// the fp64 entry, and an LDS the device lacks.
inline MosaicPlan mosaic32_plan(int64_t npix, int64_t nbl, int64_t nchan, int64_t nt, int weight_form, bool chan_avg, int64_t budget_bytes,
                                int64_t lds_max, int asked, bool uniform, int max_streams) {
  MosaicPlan p = mosaic_plan(npix, nbl, nchan, nt, weight_form, chan_avg, budget_bytes, lds_max, asked, uniform || asked == kImagingStepped,
                             max_streams);                                                              // the grid is judged below
  p.reseed = kImaging32Reseed;
  p.lds = kImaging32Lds;
  if (p.refusal) return p;
  if (asked == kImagingDirect)
    p.refusal = "the fp32 route has no DIRECT form: call prisim_mosaic_image";
  else if (!uniform)
    p.refusal = "the fp32 route needs a uniform channel grid: call prisim_mosaic_image";
  else if (p.lds > lds_max)
    p.refusal = "the staged rows do not fit in the LDS of the device";
  return p;
}

}  // namespace pint

#endif  // PRISIM_MOSAIC32_PLAN_H
