// imclean_plan.h -- how prisim_clean_image (../csrc_imaging/imclean.hip) plans a call: the route and the launch geometry of the dirty
// image and of the update (those of imaging_plan.h), the slabs of the peak search, and the device bytes by buffer.  The whole image
// is resident for the whole call: one that does not fit the budget is refused with the bytes it needs, nothing is streamed in pixel
// chunks.  Plain C++ without HIP, so that a host program can check it (tests/imclean_plan_main.cpp).  Not part of the public ABI.
#ifndef PRISIM_IMCLEAN_PLAN_H
#define PRISIM_IMCLEAN_PLAN_H

#include <algorithm>
#include <cstdint>

#include "imaging_plan.h"

namespace pint {

constexpr int64_t kImcleanMaxPixels = int64_t(1) << 28;   // kImagingMaxGrid blocks of kImagingBlock pixels: one grid holds the image
constexpr int64_t kImcleanMaxIter = int64_t(1) << 30;
constexpr int64_t kImcleanMaxSlabs = 256;                 // partial peaks per image channel at most: one workgroup reduces them
constexpr int kImcleanPollDefault = 32, kImcleanPollMax = 1024;   // PRISIM_IMCLEAN_POLL_DEFAULT, PRISIM_IMCLEAN_POLL_MAX

// iterations enqueued between two reads of the active count
inline int imclean_batch(int64_t poll_every) {
  return poll_every <= 0 ? kImcleanPollDefault : (int)std::min<int64_t>(poll_every, kImcleanPollMax);
}

// The plan of a call.  nc: image channels (1 with chan_avg).  The peak search reads the residual channel-fastest: a workgroup of 256
// threads is peak_cx channels (a power of two, 32 at most) by 256 / peak_cx pixel lanes and owns a slab of `slab` pixels (a whole
// number of blocks, kImcleanMaxSlabs slabs at most); peak_cgroups such workgroups cover the channels.
// Device bytes, all resident for the whole call:
//   dd        [nt][npix] the direction offsets, 32 B
//   resid     [npix][nc] the residual, 8 B
//   scratch   [npix][nchan] with chan_avg: the numerators of the dirty image, then of every update, before the sum over the band
//   lists     [nc][maxiter] the components: pixel 4 B, flux 8 B
//   partials  [nslabs][nc] (|value|, index) 16 B
//   state     per image channel: q 4, a 8, thr 8, P0 8, ncomp 4, status 4, W 8 (nchan of them) and 8 for their sum; 16 for the counts
//   window    [npix] 1 B
// refusal: null, or why the call cannot run; `total` is then still the bytes the image needs (0 where the sizes themselves are
// refused).
struct ImcleanPlan {
  int route;
  int64_t nc, tile, ntiles, reseed, block, nblocks, lds;
  int64_t slab, nslabs, peak_cx, peak_cgroups;
  int64_t dd_bytes, resid_bytes, scratch_bytes, list_bytes, partial_bytes, state_bytes, window_bytes, total;
  const char* refusal;
};
inline ImcleanPlan imclean_plan(int64_t npix, int64_t nbl, int64_t nchan, int64_t nt, bool chan_avg, int64_t maxiter, int64_t budget_bytes,
                                int64_t lds_max, int asked, bool uniform) {
  ImcleanPlan p{};
  p.nc = chan_avg ? 1 : nchan;
  p.tile = kImagingTile;
  p.block = kImagingBlock;
  p.lds = kImagingLds + kImagingTile * 12;              // the staged rows, and the tile's (q, a): 4 + 8 B a channel
  p.route = asked == kImagingDirect ? kImagingDirect : asked == kImagingStepped ? kImagingStepped : uniform ? kImagingStepped : kImagingDirect;
  p.reseed = p.route == kImagingStepped ? kImagingReseed : 1;
  if (npix < 1 || nbl < 1 || nchan < 1 || nt < 1) { p.refusal = "need npix, nbl, nchan and nt >= 1"; return p; }
  if (npix > kImcleanMaxPixels) { p.refusal = "npix must be at most 2^28"; return p; }
  if (nchan > (int64_t(1) << 20) || nt > (int64_t(1) << 30) || nbl > (int64_t(1) << 30)) { p.refusal = "nchan must be at most 2^20, nt and nbl 2^30"; return p; }
  if (npix > (int64_t(1) << 46) / nchan) { p.refusal = "npix * nchan must be at most 2^46"; return p; }
  if (maxiter < 0 || maxiter > kImcleanMaxIter) { p.refusal = "maxiter must lie in [0, 2^30]"; return p; }
  if (asked < -1 || asked > kImagingStepped) { p.refusal = "unknown route"; return p; }
  p.ntiles = (nchan + p.tile - 1) / p.tile;
  p.nblocks = (npix + p.block - 1) / p.block;
  p.peak_cx = 1;
  while (p.peak_cx < 32 && p.peak_cx < p.nc) p.peak_cx *= 2;
  p.peak_cgroups = (p.nc + p.peak_cx - 1) / p.peak_cx;
  p.slab = p.block * ((p.nblocks + kImcleanMaxSlabs - 1) / kImcleanMaxSlabs);
  p.nslabs = (npix + p.slab - 1) / p.slab;
  // sizes within the limits above: nt * npix <= 2^58 would overflow times 32, so the products are formed against the largest budget
  constexpr int64_t cap = int64_t(1) << 56;
  auto times = [](int64_t a, int64_t b) { return a > cap / std::max<int64_t>(b, 1) ? cap : a * b; };
  p.dd_bytes = times(times(nt, npix), 32);
  p.resid_bytes = times(times(npix, p.nc), 8);
  p.scratch_bytes = chan_avg ? times(times(npix, nchan), 8) : 0;
  p.list_bytes = times(times(p.nc, maxiter), 12);
  p.partial_bytes = times(times(p.nslabs, p.nc), 16);
  p.state_bytes = p.nc * 36 + nchan * 8 + 8 + 16;
  p.window_bytes = npix;
  p.total = std::min(cap, p.dd_bytes + p.resid_bytes + p.scratch_bytes + p.list_bytes + p.partial_bytes + p.state_bytes + p.window_bytes);
  if (asked == kImagingStepped && !uniform) { p.refusal = "the stepped route needs a uniform channel grid"; return p; }
  if (p.lds > lds_max) { p.refusal = "the staged rows do not fit in the LDS of the device"; return p; }
  if (p.total > budget_or_default(budget_bytes)) { p.refusal = "budget_bytes cannot hold the whole image"; return p; }
  return p;
}

}  // namespace pint

#endif  // PRISIM_IMCLEAN_PLAN_H
