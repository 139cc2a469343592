// antpower_plan.h -- how prisim_antenna_power (../csrc_antpower/antpower.hip) plans a call: the block of sources, the source lanes and
// the channel tile of a workgroup of the reduction, and the spans of sources a snapshot is streamed in.  Plain C++ without HIP, so that
// a host program can check it (tests/test_antpower.py).  Not part of the public ABI.
#ifndef PRISIM_ANTPOWER_PLAN_H
#define PRISIM_ANTPOWER_PLAN_H

#include <algorithm>
#include <cstdint>

#include "addon_plan.h"

namespace pint {

constexpr int kAntpowerThreads = 256;                 // threads of a workgroup of the reduction (kThreads of addon_internal.h)
constexpr int kAntpowerMaxChanTile = 64;              // channels per workgroup: 512-byte runs of a row of pb_tile
constexpr int64_t kAntpowerBlock = 256;               // SB: consecutive catalogue sources one workgroup sums
// pb_tile of a span, [span][nchan] float64, is written by the beam kernel and read back by the reduction right behind it: it should
// still be in the 256 MiB Infinity Cache of the device then.  16, 64 and 256 MiB were timed.
constexpr int64_t kAntpowerPbTileBytes = int64_t(64) << 20;
constexpr int64_t kAntpowerMaxGrid = int64_t(1) << 20;   // blocks of a span at most: the x extent of a grid of the reduction
constexpr int64_t kAntpowerDirBytes = 32;             // dirs: one double4 per source of the span
constexpr int64_t kAntpowerUnitBytes = 16;            // the unit flux of the beam launch: flux_ref = 1 and spindex = 0 per source, shared by the streams

// The workgroup of the reduction, from (nsrc, nchan) alone: it decides the order of the sums, so nothing else may enter.
//   tile   channels per workgroup: the power of two that covers the band, kAntpowerMaxChanTile at most
//   lanes  L = kAntpowerThreads / tile source lanes: lane l walks the sources l, l + L, ... of its block in ascending order
//   block  SB sources; nblocks blocks cover the catalogue; ntiles channel tiles cover the band
struct AntpowerShape { int64_t block, nblocks, tile, ntiles, lanes, lds; };
inline AntpowerShape antpower_shape(int64_t nsrc, int64_t nchan) {
  int64_t tile = 1;
  while (tile < nchan && tile < kAntpowerMaxChanTile) tile *= 2;
  const int64_t block = kAntpowerBlock;
  return {block, (nsrc + block - 1) / block, tile, (nchan + tile - 1) / tile, kAntpowerThreads / tile, (int64_t)kAntpowerThreads * 16};
}

// bytes one source of a span takes in the buffers of one stream, and the partial sums part[nblocks][2][nchan] of one snapshot in flight
inline int64_t antpower_source_bytes(int64_t nchan) { return kAntpowerDirBytes + 8 * nchan; }
inline int64_t antpower_partial_bytes(const AntpowerShape& sh, int64_t nchan) { return sh.nblocks * 2 * nchan * 8; }

// The spans of a snapshot's nsrc sources, a whole number of blocks each (the last one ragged with the catalogue), and the streams the
// nsnap snapshots are dealt to.  Each stream holds the buffers of one span (dirs and pb_tile) and the partial sums of one snapshot;
// the unit flux is shared.  The span is the largest that fits in the budget beside the partial sums, pb_tile_bytes of pb_tile at
// most.  ok = false: the budget cannot hold one block (then with one stream).  The budget and the streams decide only how much is in
// flight: the shape, and with it every sum, is the same.
struct AntpowerPlan { AntpowerShape shape; Chunks spans; int nstreams; int64_t buffer_bytes; bool ok; };
inline AntpowerPlan antpower_plan(int64_t nsrc, int64_t nchan, int64_t nsnap, int64_t budget_bytes, int64_t pb_tile_bytes, int max_streams) {
  AntpowerPlan p{};
  p.shape = antpower_shape(nsrc, nchan);
  const int64_t sb = p.shape.block, budget = budget_or_default(budget_bytes);
  const int64_t per_source = antpower_source_bytes(nchan), part = antpower_partial_bytes(p.shape, nchan);
  const int64_t whole = p.shape.nblocks * sb;                                        // the catalogue rounded up to blocks
  // blocks of a span: by pb_tile, one at least, and no more than a grid takes
  const int64_t cap = std::min(kAntpowerMaxGrid, std::max<int64_t>(1, std::max<int64_t>(pb_tile_bytes, 1) / (8 * nchan * sb)));
  int64_t span = 0;
  for (int ns = (int)std::min<int64_t>(std::max(max_streams, 1), nsnap); ns >= 1 && span < sb; --ns) {
    // ns * (span * per_source + part) + span * kAntpowerUnitBytes <= budget
    const int64_t room = budget - ns * part;
    const int64_t fit = room > 0 ? plan_chunks(whole, ns * per_source + kAntpowerUnitBytes, room, 1).size : 0;
    span = std::min(std::min(fit / sb, cap) * sb, whole);
    p.nstreams = ns;
  }
  p.ok = span >= sb;
  if (!p.ok) span = sb;
  p.spans = chunks_of(nsrc, span, 1);
  p.buffer_bytes = p.nstreams * (span * per_source + part) + span * kAntpowerUnitBytes;
  return p;
}

}  // namespace pint

#endif  // PRISIM_ANTPOWER_PLAN_H
