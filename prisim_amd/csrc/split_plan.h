// split_plan.h -- how many source splits a sky-sum grid is cut into (host only, no HIP: it compiles alone).
//
// The grid of a sky-sum is tiles x groups blocks (channel tiles x groups of 256 summed baselines) and runs in rounds of `slots`
// resident blocks (CUs x blocks per CU).  A grid shallower than 6 rounds is deepened by cutting the sources into nsplit pieces, each
// writing a partial cube that k_reduce_partials sums again:
//   want = round(7.5 slots / (tiles groups))     measured on 1/2, 1/4 and 1/8 baseline shards of config 3 (tools/shard_nsplit_sweep.py,
//          candidates alternating): the step time is lowest when the grid is again about 7.5 rounds deep, like the unsplit full problem
//          (nsplit = 2 / 4 / 8: 1.00 / 1.02 / 1.03 x the ideal T1/N against 1.03 / 1.06 / 1.10 x unsplit) -- blocks then start and
//          finish out of step and the tail is short.  Grids that are already >= 6 rounds deep keep nsplit = 1 (alternating A/B on the
//          full config 3, tools/full_nsplit.py: 1 / 2 / 4 splits within 0.4 % of each other);
//   floor:  at least 32 sources per split, before and behind the cap;
//   cap:    the partial-cube traffic (~3 TB/s effective) stays under ~3 % of the sky-sum's own time, but never below one round of
//          resident blocks.  One rank's share of config 4 at N = 8 (1016 bl x 768 ch x 24 576 sources): 2.86 ms at 16 splits against
//          3.13 ms at the 64 the round rule alone asks for.  Splits up to 16 keep the round rule; deeper ones go where that sweep's
//          optimum sits, a grid of ~1.5 rounds -- the second, half-empty round runs one block per CU, and a lone wave per SIMD issues
//          packed FMAs at 3/4 of the full rate -- 2.53 ms at 16 splits against 3.28 at 19 and 2.75 at 10 or 24 on the config-4 share;
//   bounds: 1 <= nsplit <= 64.
// make_plan (skyvis_plan.h) then realises the count in whole source chunks.
#pragma once
#include <algorithm>
#include <cstdint>

namespace prisim {

constexpr int64_t kMaxSplits = 64;
constexpr int64_t kMinSplitSources = 32;

// nbl, nchan: rows and channels the sky-sum computes; f32 / taper select the term rate of the kernel the cap is held against.
inline int split_count(int64_t tiles, int64_t groups, int64_t slots, int64_t nsrc, int64_t nbl, int64_t nchan, bool f32, bool taper) {
  const int64_t base = std::max<int64_t>(tiles * groups, 1);
  slots = std::max<int64_t>(slots, 1);
  int64_t want = 1;
  if (base * 10 < slots * 60) want = (slots * 15 / 2 + base / 2) / base;       // round(7.5 * slots / base)
  want = std::min<int64_t>(want, std::max<int64_t>(1, nsrc / kMinSplitSources));      // (before the deep branch: it decides whether that is entered)
  const double rate = f32 ? (taper ? 7.0e12 : 1.0e13) : (taper ? 2.8e12 : 5.0e12);       // terms/s of the big kernels
  const double t_compute = (double)nbl * (double)nchan * (double)nsrc / rate;
  const double t_split = 2.0 * (double)nbl * (double)nchan * (f32 ? 8.0 : 16.0) / 3.0e12;
  const int64_t cap = std::max<int64_t>((slots + base - 1) / base, (int64_t)(0.03 * t_compute / t_split));
  const int64_t floor_splits = std::max<int64_t>(1, nsrc / kMinSplitSources);
  if (want > 16) want = std::max<int64_t>(16, std::min<int64_t>((3 * slots / 2 + base / 2) / base, cap));
  // (the deep branch is bounded by the cap, which is at least one round of blocks whatever the sky: a sky of a few hundred sources on a
  // grid of a few blocks once left it with fewer than 32 sources per split.  The floor stands behind it too.)
  want = std::min<int64_t>(want, floor_splits);
  return (int)std::max<int64_t>(1, std::min<int64_t>(want, kMaxSplits));
}

}  // namespace prisim
