// tail_plan.h -- the last source piece of a split sky-sum cut into small ones, and the per-XCD slab table that goes with unequal
// pieces (host only, no HIP: it compiles alone).
//
// make_plan (skyvis_plan.h) cuts the sources of a shallow grid into n0 equal pieces; a work item (piece, tile, baseline group) of the
// headline step then lasts 1/8.6 of the launch, and what still runs alone at the end of the launch is that coarse.  Every piece costs
// a partial cube, so only the LAST piece is cut finer: the small items are every XCD's last ones and fill the end of the launch.
//   pieces 0 .. n0-2       the plan's, [src_lo + i per, src_lo + (i + 1) per)
//   the plan's last piece  L = src_hi - src_lo - (n0 - 1) per sources: one piece of round_up(L / 2, chunk), then pieces of
//                          round_up(L / 8, chunk) -- at most four, the last of them takes what is left (the quotients are rounded
//                          up as real numbers, so no piece is longer than the one before it); empty pieces are dropped: n <= n0 + 4
// and only when
//   n0 >= 2, count and chunk are the planner's (a set_tuning count or chunk is honoured exactly),
//   L / 8 >= 64 and every tail piece has at least 64 sources (the kernel's L2 warm-up stays on; split_plan.h's floor of 32 per split),
//   n <= 64 (kMaxSplits), and
//   tiles groups n0 >= 3 slots: the grid is at least three rounds of resident blocks deep -- the deep branch of split_plan.h runs
//   grids of about 1.5 rounds, another regime, and stays as it is.
// Otherwise the plan's pieces come back unchanged.  kTailForce (a test mode for small shapes) drops the depth condition and the
// 64-source floor: whole pieces are at least one chunk by construction and the last may be any non-empty remainder.
//
// With unequal pieces, block_item's cut of the slab-major items into 8 ranges by COUNT would give the XCDs unequal work.
// tail_slab_table deals the slabs (piece, tile) -- pieces in order, tiles inner -- round-robin to the 8 XCDs, the rotation carried on
// from piece to piece: every XCD holds its share of every size within one slab, the big ones first and the small ones last.
// tests/test_tail_plan.py holds both to a restatement and to a list-scheduling model of the launch.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace prisim {

constexpr int kTailMaxPieces = 64;        // = kMaxSplits of split_plan.h
constexpr int kTailExtra = 4;             // pieces the rule adds at most
constexpr int64_t kTailMinSources = 64;   // the packed kernel's warm-up threshold (pf_on)
constexpr int kTailXcds = 8;

enum TailMode { kTailOff = 0, kTailRule = 1, kTailForce = 2 };

struct TailPieces {
  int n;                                  // pieces
  int ntail;                              // how many of them the rule made of the plan's last piece (0: the plan's pieces)
  int64_t lo[kTailMaxPieces + 1];         // piece i = sources [lo[i], lo[i + 1])
};

// n0, src_per_split, chunk: the plan's; [src_lo, src_hi): the launch's sources; tuned: the count or the chunk came from set_tuning.
inline TailPieces tail_pieces(int n0, int64_t src_per_split, int64_t chunk, int64_t src_lo, int64_t src_hi, int64_t ntiles, int64_t nbgroups,
                              int64_t slots, int mode, bool tuned) {
  TailPieces t{};
  n0 = std::max(1, std::min(n0, kTailMaxPieces));
  chunk = std::max<int64_t>(chunk, 1);
  for (int i = 0; i < n0; ++i) t.lo[i] = std::min(src_lo + (int64_t)i * src_per_split, src_hi);
  t.lo[n0] = src_hi;
  t.n = n0;
  if (mode == kTailOff || tuned || n0 < 2 || n0 + 1 > kTailMaxPieces) return t;
  if (mode != kTailForce && ntiles * nbgroups * (int64_t)n0 < 3 * std::max<int64_t>(slots, 1)) return t;
  const int64_t start = src_lo + (int64_t)(n0 - 1) * src_per_split;
  const int64_t L = src_hi - start;
  if (L <= 0 || L > src_per_split) return t;      // (not a plan of make_plan's: leave it alone)
  const int64_t floor_src = mode == kTailForce ? 1 : kTailMinSources;
  if (L < 8 * floor_src) return t;                // an eighth is under the floor
  auto up = [&](int64_t num, int64_t den) { return ((num + den - 1) / den + chunk - 1) / chunk * chunk; };      // round_up(ceil(num / den), chunk)
  const int64_t half = up(L, 2), eighth = up(L, 8);
  int64_t cut[kTailExtra + 2];
  int nt = 0;
  int64_t at = 0;
  cut[0] = 0;
  for (int k = 0; k <= kTailExtra && at < L; ++k) {
    const int64_t len = k == 0 ? half : (k == kTailExtra ? L - at : eighth);
    at = std::min(L, at + len);
    cut[++nt] = at;
  }
  if (nt < 2 || n0 - 1 + nt > kTailMaxPieces) return t;      // the half is the whole piece: nothing to cut
  for (int k = 0; k < nt; ++k)
    if (cut[k + 1] - cut[k] < floor_src) return t;
  for (int k = 0; k <= nt; ++k) t.lo[n0 - 1 + k] = start + cut[k];
  t.n = n0 - 1 + nt;
  t.ntail = nt;
  return t;
}

// tab: [8][per_xcd_slabs] pairs (piece, tile), -1 where an XCD has no slab left.  Returns per_xcd_slabs.
inline int tail_slab_table(int npieces, int ntiles, std::vector<int32_t>& tab) {
  const int64_t slabs = (int64_t)std::max(npieces, 0) * std::max(ntiles, 0);
  const int per = (int)((slabs + kTailXcds - 1) / kTailXcds);
  tab.assign((size_t)kTailXcds * (size_t)per * 2, -1);
  int64_t k = 0;
  for (int piece = 0; piece < npieces; ++piece)
    for (int tile = 0; tile < ntiles; ++tile, ++k) {
      const size_t at = ((size_t)(k % kTailXcds) * (size_t)per + (size_t)(k / kTailXcds)) * 2;
      tab[at] = piece;
      tab[at + 1] = tile;
    }
  return per;
}

}  // namespace prisim
