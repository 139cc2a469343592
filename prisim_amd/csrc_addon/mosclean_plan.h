// mosclean_plan.h -- how prisim_clean_mosaic (../csrc_imaging/mosclean.hip) plans a call.  The route, the channel tile, the block, the
// slabs of the peak search, the lists, the partials and every limit on the sizes are those of imclean_plan.h, asked of it and not
// restated; what this header adds is the bytes of the buffers a mosaic holds per pixel and the LDS of its update.  The whole image is
// resident for the whole call, as in imclean_plan.h: one that does not fit the budget is refused with the bytes it needs, nothing is
// streamed in pixel chunks.  Plain C++ without HIP, so that a host program can check it (tests/mosclean_plan_main.cpp).  Not part of
// the public ABI.
#ifndef PRISIM_MOSCLEAN_PLAN_H
#define PRISIM_MOSCLEAN_PLAN_H

#include <algorithm>
#include <cstdint>

#include "imclean_plan.h"

namespace pint {

// The plan of a call.  clean: the plan of prisim_clean_image for the same sizes under a budget that refuses nothing, from which the
// route, tile, ntiles, reseed, block, nblocks, slab, nslabs, peak_cx, peak_cgroups, nc, list_bytes and partial_bytes are read.
// Device bytes, all resident for the whole call:
//   dirs      [nt][npix] the directions (l, m, n, 0) and their offsets from the phase centre, 64 B
//   beam      [nt][npix][nchan] the power pattern, 0 below the horizon, 8 B
//   sums      [npix][nchan] R_N and Q, 16 B
//   flat      [npix][nc] the search image F, 8 B
//   out       [npix][nc] the residual and the effective beam, 16 B
//   window    [npix] 1 B
//   lists     [nc][maxiter] the components: pixel 4 B, flux 8 B            (imclean_plan.h)
//   partials  [nslabs][nc] (|value|, index) 16 B                           (imclean_plan.h)
//   state     per image channel: q 4, a 8, thr 8, P0 8, ncomp 4, status 4; per channel W_t (nt of them) and Wtot 8; 8 for the band's
//             weight; 16 for the counts
// lds: the staged rows of imaging_plan.h and, per channel of the tile, the flux (8 B), the pick (4 B) and the flux times the beam
// at the pick in the snapshot in hand (8 B).
// refusal: null, or why the call cannot run; `total` is then still the bytes the image needs (0 where the sizes themselves are
// refused).
struct MoscleanPlan {
  ImcleanPlan clean;
  int64_t lds;
  int64_t dirs_bytes, beam_bytes, sums_bytes, flat_bytes, out_bytes, window_bytes, list_bytes, partial_bytes, state_bytes, total;
  const char* refusal;
};
inline MoscleanPlan mosclean_plan(int64_t npix, int64_t nbl, int64_t nchan, int64_t nt, bool chan_avg, int64_t maxiter, int64_t budget_bytes,
                                  int64_t lds_max, int asked, bool uniform) {
  MoscleanPlan p{};
  constexpr int64_t cap = int64_t(1) << 56;             // that of imclean_plan: no total is formed beyond it
  p.clean = imclean_plan(npix, nbl, nchan, nt, chan_avg, maxiter, cap, lds_max, asked, uniform);
  p.lds = kImagingLds + kImagingTile * 20;
  // the sizes, the route and the LDS of the smaller workgroup: refused there.  Its budget refuses nothing it can count
  if (p.clean.refusal) { p.refusal = p.clean.refusal; return p; }
  auto times = [](int64_t a, int64_t b) { return a > cap / std::max<int64_t>(b, 1) ? cap : a * b; };
  const int64_t nc = p.clean.nc;
  p.dirs_bytes = times(times(nt, npix), 64);
  p.beam_bytes = times(times(times(nt, npix), nchan), 8);
  p.sums_bytes = times(times(npix, nchan), 16);
  p.flat_bytes = times(times(npix, nc), 8);
  p.out_bytes = times(times(npix, nc), 16);
  p.window_bytes = npix;
  p.list_bytes = p.clean.list_bytes;
  p.partial_bytes = p.clean.partial_bytes;
  p.state_bytes = std::min(cap, nc * 36 + times(nt + 1, nchan) * 8 + 8 + 16);
  int64_t total = 0;
  for (int64_t b : {p.dirs_bytes, p.beam_bytes, p.sums_bytes, p.flat_bytes, p.out_bytes, p.window_bytes, p.list_bytes, p.partial_bytes,
                    p.state_bytes})
    total = std::min(cap, total + b);                   // nine terms of at most 2^56: no overflow
  p.total = total;
  if (p.lds > lds_max) { p.refusal = "the staged rows do not fit in the LDS of the device"; return p; }
  if (p.total > budget_or_default(budget_bytes)) { p.refusal = "budget_bytes cannot hold the whole image"; return p; }
  return p;
}

}  // namespace pint

#endif  // PRISIM_MOSCLEAN_PLAN_H
