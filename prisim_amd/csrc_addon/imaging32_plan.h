// imaging32_plan.h -- how prisim_dirty_image_f32 (../csrc_imaging/imaging32.hip) plans a call.  The route and the chunks of pixels are
// pixel_plan's (imaging_plan.h), called and not restated; what the fp32 tile pass adds is stated here as named constants: the rows of a
// pass, the interval at which the fp32 partial sums go into the fp64 totals, the channel of the tile the phasor is seeded at, and the
// LDS of a workgroup.  Plain C++ without HIP, so that a host program can check it (tests/test_imaging32.py).  Not part of the public ABI.
#ifndef PRISIM_IMAGING32_PLAN_H
#define PRISIM_IMAGING32_PLAN_H

#include <cstdint>

#include "imaging_plan.h"

namespace pint {

constexpr int kImaging32Rows = 64;       // baselines of one snapshot staged in LDS at a time, as float: the bytes of 32 fp64 rows
constexpr int kImaging32Pair = 2;        // rows of one packed chain: the two halves of every 2-vector of the loop
constexpr int kImaging32Flush = 64;      // rows between two additions of the fp32 partial sums into the fp64 totals: every pass.  A
                                         // partial sum is one half of a pair, so it holds kImaging32Flush / kImaging32Pair = 32 terms
constexpr int kImaging32Seed = 16;       // the channel of the tile the phasor is seeded at, from f[k0] + 16 df; walked up over
                                         // [16, 32) and down over [0, 16): no chain is longer than 16 steps
constexpr int kImaging32Reseed = 32;     // channels between two seeds: the tile is seeded once (stats->reseed)

// LDS of a workgroup: the staged rows [kImaging32Rows / 2][kImagingTile] of (x_even, x_odd, -y_even, -y_odd) as float, x + i y the
// operand (w Re V, w Im V) rounded once, and the rows' baselines / c (x, y, z) as double
constexpr int64_t kImaging32Lds = int64_t(kImaging32Rows) * kImagingTile * 8 + kImaging32Rows * 24;

static_assert(kImaging32Rows % kImaging32Pair == 0 && kImaging32Flush % kImaging32Rows == 0 && kImaging32Flush == kImaging32Rows,
              "the partial sums are flushed at the end of every pass");
static_assert(kImaging32Seed * 2 == kImagingTile && kImaging32Reseed == kImagingTile, "one seed at the tile's centre");

static_assert(kImaging32Lds >= kImagingLds, "a device that holds this pass holds pixel_plan's: its LDS check is implied by the one here");

// ImagingPlan with the constants of the fp32 pass beside it; plan_stats and the entry read it under ImagingPlan's names
struct Imaging32Plan : ImagingPlan {
  int64_t rows, flush, seed;
};

// The plan of a call of the fp32 entry: asked, weight_form, the budget and the streams as imaging_plan takes them.  The chunk buffers
// are those of the fp64 entry (the offsets, the rows of D and the averaged value stay fp64), so the chunks are imaging_plan's for the
// same sizes and budget.  refusal: null, or why the call cannot run: whatever pixel_plan refuses, an LDS the device lacks, the DIRECT
// route and a grid that is not uniform under AUTO or STEPPED, each in a sentence of its own that names the fp64 entry.
inline Imaging32Plan imaging32_plan(int64_t npix, int64_t nbl, int64_t nchan, int64_t nt, int weight_form, bool chan_avg, int64_t budget_bytes,
                                    int64_t lds_max, int asked, bool uniform, int max_streams) {
  Imaging32Plan p{};
  static_cast<ImagingPlan&>(p) = pixel_plan(npix, nbl, nchan, nt, weight_form, imaging_pixel_bytes(nchan, nt, chan_avg), budget_bytes, lds_max,
                                            asked, uniform || asked == kImagingStepped, max_streams);   // the grid is judged below
  p.rows = kImaging32Rows;
  p.flush = kImaging32Flush;
  p.seed = kImaging32Seed;
  p.reseed = kImaging32Reseed;
  p.lds = kImaging32Lds;
  if (p.refusal) return p;
  if (asked == kImagingDirect)
    p.refusal = "the fp32 route has no DIRECT form: call prisim_dirty_image";
  else if (!uniform)
    p.refusal = "the fp32 route needs a uniform channel grid: call prisim_dirty_image";
  else if (p.lds > lds_max)
    p.refusal = "the staged rows do not fit in the LDS of the device";
  return p;
}

}  // namespace pint

#endif  // PRISIM_IMAGING32_PLAN_H
