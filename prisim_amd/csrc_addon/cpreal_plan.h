// cpreal_plan.h -- how prisim_closure_realizations (../csrc_closure/cpreal.hip) plans a call: the route, the channel tile and the
// workgroup of the staged kernel, and the chunks of (snapshot, realisation) pairs.  Plain C++ without HIP, so that a host program can
// check it (tests/test_cpreal.py).  Not part of the public ABI.
#ifndef PRISIM_CPREAL_PLAN_H
#define PRISIM_CPREAL_PLAN_H

#include <algorithm>
#include <cstdint>

#include "addon_plan.h"

namespace pint {

constexpr int kCprealDirect = 0, kCprealStaged = 1;   // PRISIM_CPREAL_DIRECT, PRISIM_CPREAL_STAGED
constexpr int kCprealMinTile = 8;                     // the narrowest channel tile: 128 B of LDS per used row, 64-byte runs of output
constexpr int kCprealMaxTile = 64;
constexpr int64_t kCprealCell = 16;                   // LDS bytes per (used row, channel): one complex128

// The staged kernel's workgroup.  tile: channels per workgroup, the widest power of two in [kCprealMinTile, kCprealMaxTile] that is
// not wider than the band (so a ragged band still splits into tiles) and whose rows fit in kTileLds, so that at least two workgroups
// share a CU of 160 KiB; the narrowest when only that fits in lds_max; 0 when not even that does.  threads: 256 while four workgroups
// fit in a CU by their LDS (40 KiB each), 512 for two, 1024 for one: 16 waves per CU in every case, four per SIMD, for a kernel whose
// time is in dependent fp64 chains (log, sqrt, sincospi, atan2) and not in memory.
struct CprealTile { int64_t tile, ntiles, lds; int threads; };
inline CprealTile cpreal_tile(int64_t nrow, int64_t nchan, int64_t lds_max) {
  const int64_t row = std::max<int64_t>(nrow, 1) * kCprealCell;
  if (row * kCprealMinTile > lds_max) return {0, 0, 0, 0};
  int64_t tile = kCprealMinTile;
  while (tile * 2 <= kCprealMaxTile && tile * 2 <= nchan && row * tile * 2 <= std::min<int64_t>(lds_max, kTileLds)) tile *= 2;
  const int64_t lds = row * tile;
  return {tile, (nchan + tile - 1) / tile, lds, lds <= 40960 ? 256 : lds <= 81920 ? 512 : 1024};
}

// The route a call takes: asked is -1 (auto) or a route.  AUTO is STAGED exactly when the narrowest tile fits.  -1: STAGED was asked
// for and does not fit.
inline int cpreal_route(int asked, int64_t nrow, int64_t lds_max) {
  const bool fits = std::max<int64_t>(nrow, 1) * kCprealCell * kCprealMinTile <= lds_max;
  if (asked == kCprealDirect) return kCprealDirect;
  if (asked == kCprealStaged) return fits ? kCprealStaged : -1;
  return fits ? kCprealStaged : kCprealDirect;
}

// The chunks of npairs (snapshot, realisation) pairs: as many pairs as max_streams chunk buffers of bytes_per_pair a pair hold within
// the budget, and no more than a grid of max_blocks workgroups at blocks_per_pair a pair covers (0: a grid-stride kernel, no limit).
inline Chunks cpreal_chunks(int64_t npairs, int64_t bytes_per_pair, int64_t budget_bytes, int64_t blocks_per_pair, int64_t max_blocks,
                            int max_streams) {
  const int64_t fit = plan_chunks(npairs, bytes_per_pair, budget_bytes, max_streams).size;
  const int64_t grid = blocks_per_pair > 0 ? std::max<int64_t>(1, max_blocks / blocks_per_pair) : npairs;
  return chunks_of(npairs, std::min(fit, grid), max_streams);
}

}  // namespace pint

#endif  // PRISIM_CPREAL_PLAN_H
