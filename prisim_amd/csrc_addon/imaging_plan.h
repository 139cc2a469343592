// imaging_plan.h -- how prisim_dirty_image (../csrc_imaging/imaging.hip) plans a call: the route, the channel tile and the reseed
// interval of a thread, the pixels and the LDS of a workgroup, and the chunks of pixels.  Plain C++ without HIP, so that a host program
// can check it (tests/test_imaging.py).  Not part of the public ABI.
#ifndef PRISIM_IMAGING_PLAN_H
#define PRISIM_IMAGING_PLAN_H

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "addon_plan.h"

namespace pint {

constexpr int kImagingDirect = 0, kImagingStepped = 1;   // PRISIM_IMAGE_DIRECT, PRISIM_IMAGE_STEPPED
constexpr int kImagingBlock = 256;                    // pixels per workgroup, one per thread (kThreads of addon_internal.h)
constexpr int kImagingTile = 32;                      // channels per thread: 32 fp64 accumulators, 64 VGPRs
constexpr int kImagingReseed = 32;                    // K: channels between two seeds from the true frequency; the tile is seeded once
constexpr int kImagingRows = 32;                      // baselines of one snapshot staged in LDS at a time
constexpr int64_t kImagingMaxGrid = int64_t(1) << 20; // blocks of a chunk at most: the x extent of a grid
constexpr double kImagingGridTol = 1e-7;              // Hz: the uniform-grid rule of prisim_hip_set_array

// LDS of a workgroup: the staged rows [kImagingRows][kImagingTile] of (w Re V, w Im V), their baselines / c (x, y, z) and the tile's
// frequencies
constexpr int64_t kImagingLds = int64_t(kImagingRows) * kImagingTile * 16 + kImagingRows * 24 + kImagingTile * 8;

// f[k] = f[0] + k df to within kImagingGridTol with df = (f[n-1] - f[0]) / (n - 1), 0 for one channel: what the sky-sum's recurrence
// kernels accept as a uniform grid
inline bool imaging_grid_uniform(const double* f, int64_t n, double& df) {
  df = n > 1 ? (f[n - 1] - f[0]) / (double)(n - 1) : 0.0;
  for (int64_t k = 0; k < n; ++k)
    if (!(std::fabs(f[k] - (f[0] + (double)k * df)) <= kImagingGridTol)) return false;
  return true;
}

// bytes one pixel of a chunk takes in the buffers of one stream: its direction offsets (32 B per snapshot), its row of D or of the
// image (8 B per channel) and, with chan_avg, its averaged value
inline int64_t imaging_pixel_bytes(int64_t nchan, int64_t nt, bool chan_avg) { return 32 * nt + 8 * nchan + (chan_avg ? 8 : 0); }

// The plan of a call.  asked: -1 (auto) or a route; weight_form 0, 1 or 2.  route: AUTO is STEPPED exactly when the grid is uniform.
// The chunks are whole numbers of blocks of kImagingBlock pixels (the last one ragged with npix), the largest of which `nstreams`
// (max_streams at most, fewer when the budget holds one block only then) fit in the budget.  refusal: null, or why the call cannot run
// (then the other fields are those of one block on one stream).  Neither the budget nor the streams enter the tile, the reseed interval
// or the block: they decide only which pixels are in flight together.
struct ImagingPlan {
  int route;
  int64_t tile, ntiles, reseed, block, nblocks, lds, pixel_bytes, buffer_bytes;
  Chunks chunks;
  const char* refusal;
};
// ... of an entry whose chunk buffers take pixel_bytes a pixel (prisim_mosaic_image plans with this too, mosaic_plan.h)
inline ImagingPlan pixel_plan(int64_t npix, int64_t nbl, int64_t nchan, int64_t nt, int weight_form, int64_t pixel_bytes, int64_t budget_bytes,
                              int64_t lds_max, int asked, bool uniform, int max_streams) {
  ImagingPlan p{};
  p.tile = kImagingTile;
  p.ntiles = (nchan + p.tile - 1) / p.tile;
  p.block = kImagingBlock;
  p.nblocks = (npix + p.block - 1) / p.block;
  p.lds = kImagingLds;
  p.pixel_bytes = pixel_bytes;
  p.route = asked == kImagingDirect ? kImagingDirect : asked == kImagingStepped ? kImagingStepped : uniform ? kImagingStepped : kImagingDirect;
  p.reseed = p.route == kImagingStepped ? kImagingReseed : 1;
  p.chunks = chunks_of(npix, p.block, 1);
  p.buffer_bytes = p.block * p.pixel_bytes;
  if (npix < 1 || nbl < 1 || nchan < 1 || nt < 1) { p.refusal = "need npix, nbl, nchan and nt >= 1"; return p; }
  if (weight_form < 0 || weight_form > 2) { p.refusal = "unknown weight form"; return p; }
  if (asked < -1 || asked > kImagingStepped) { p.refusal = "unknown route"; return p; }
  if (asked == kImagingStepped && !uniform) { p.refusal = "the stepped route needs a uniform channel grid"; return p; }
  if (p.lds > lds_max) { p.refusal = "the staged rows do not fit in the LDS of the device"; return p; }
  const int64_t budget = budget_or_default(budget_bytes), whole = p.nblocks * p.block;
  int64_t chunk = 0;
  int ns = (int)std::min<int64_t>(std::max(max_streams, 1), p.nblocks);
  for (; ns >= 1; --ns) {
    const int64_t fit = budget / (ns * p.pixel_bytes) / p.block;          // blocks per chunk with ns chunks in flight
    chunk = std::min(std::min(fit, kImagingMaxGrid) * p.block, whole);
    if (chunk >= p.block) break;
  }
  if (chunk < p.block) { p.refusal = "budget_bytes cannot hold one block of pixels"; return p; }
  p.chunks = chunks_of(npix, chunk, ns);
  p.buffer_bytes = p.chunks.nstreams * chunk * p.pixel_bytes;
  return p;
}
inline ImagingPlan imaging_plan(int64_t npix, int64_t nbl, int64_t nchan, int64_t nt, int weight_form, bool chan_avg, int64_t budget_bytes,
                                int64_t lds_max, int asked, bool uniform, int max_streams) {
  return pixel_plan(npix, nbl, nchan, nt, weight_form, imaging_pixel_bytes(nchan, nt, chan_avg), budget_bytes, lds_max, asked, uniform,
                    max_streams);
}

}  // namespace pint

#endif  // PRISIM_IMAGING_PLAN_H
