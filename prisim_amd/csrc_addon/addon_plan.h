// addon_plan.h -- the arithmetic that the add-on entries plan their calls with: the transform length as a power of two, the
// chunks of a chunk loop, the snapshot tile of the tiled kernels and the tables of the resampled spectra.  Plain C++ without HIP, so
// that a host program can check it (tests/test_addon_plan.py).  Not part of the public ABI.
#ifndef PRISIM_ADDON_PLAN_H
#define PRISIM_ADDON_PLAN_H

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

namespace pint {

constexpr int64_t kDefaultBudget = int64_t(1) << 30;  // device bytes of a call's chunk buffers when the caller gives none

inline int64_t budget_or_default(int64_t budget) { return budget > 0 ? budget : kDefaultBudget; }

// ceil(log2(m)) for m >= 1; pow2: m is a power of two
inline int ceil_log2(int64_t m, bool& pow2) {
  int logm = 0;
  while ((int64_t(1) << logm) < m) ++logm;
  pow2 = (int64_t(1) << logm) == m;
  return logm;
}

constexpr int kMaxTile = 64;                          // snapshots per workgroup of the tiled fused kernels
constexpr int kTileLds = 65536;                       // LDS their snapshot rows may fill

struct Span { int64_t first, count; };                // items [first, first + count)

// n items in `count` chunks of `size` (the last of `last`, 1 <= last <= size), dealt round-robin to nstreams streams
struct Chunks {
  int64_t size, count, last;
  int nstreams;
  Span span(int64_t c, int64_t n) const { return {c * size, std::min(size, n - c * size)}; }   // chunk c of the n items
};

// the chunks of `size` items each, 1 <= size
inline Chunks chunks_of(int64_t n, int64_t size, int max_streams) {
  const int64_t count = (n + size - 1) / size;
  return {size, count, n - (count - 1) * size, (int)std::min<int64_t>(max_streams, count)};
}

// the largest chunks of which max_streams, at bytes_per_item a piece (0 counts as 1), fit in the budget: at least one item, at most n
inline Chunks plan_chunks(int64_t n, int64_t bytes_per_item, int64_t budget_bytes, int max_streams) {
  const int64_t per = max_streams * std::max<int64_t>(bytes_per_item, 1);
  return chunks_of(n, std::max<int64_t>(1, std::min<int64_t>(n, budget_or_default(budget_bytes) / per)), max_streams);
}

// The snapshots a workgroup of a tiled kernel takes: as many rows of row_bytes as fit in kTileLds beside fixed_bytes (a twiddle
// table), kMaxTile and nt at most, one at least; the tiles of the nt snapshots and the LDS of a workgroup.
struct SnapshotTile { int64_t tile, ntiles, lds; };
inline SnapshotTile snapshot_tile(int64_t nt, int64_t row_bytes, int64_t fixed_bytes) {
  const int64_t tile = std::max<int64_t>(1, std::min<int64_t>({nt, (int64_t)kMaxTile, (kTileLds - fixed_bytes) / row_bytes}));
  return {tile, (nt + tile - 1) / tile, tile * row_bytes + fixed_bytes};
}

// scipy.signal.resample's spectrum from the caller's selection map (prisim_amd/dsp_readings.py:resample_map): output bin k < nout
// sums at most two input bins, slot s < 2 in the map's order, at [s * nout + k]: x[in] times the map's weight, the caller's scale and
// the phase.  The pieces stay apart, so that every caller multiplies them in its own order.  nout < 1: tables of one empty bin.
struct ResampleTables {
  std::vector<int32_t> in;     // [2][nout] input bin; -1: none, or a bin of the zero padding (>= nchan)
  std::vector<double> w;       // [2][nout] the map's weight
  std::vector<double> phase;   // [2][nout] (cos, sin) of -2 pi ((in floor(m/2)) mod m) / m
  std::vector<double> rtw;     // [nout] (cos, sin) of +2 pi q / nout
};

// fills t; returns null, or what is wrong with the map
inline const char* resample_tables(int64_t nout, int64_t m, int64_t nchan, int64_t nmap, const int64_t* map_out, const int64_t* map_in,
                                   const double* map_w, ResampleTables& t) {
  const int64_t nr = std::max<int64_t>(nout, 1);
  t.in.assign(2 * (size_t)nr, -1);
  t.w.assign(2 * (size_t)nr, 0.0);
  t.phase.assign(4 * (size_t)nr, 0.0);
  t.rtw.assign(2 * (size_t)nr, 0.0);
  if (nout < 1) return nullptr;
  if (nmap < 1 || !map_out || !map_in || !map_w) return "the resampled spectra need the selection map";
  std::vector<int> used((size_t)nout, 0);
  const int64_t half = m / 2;
  for (int64_t e = 0; e < nmap; ++e) {
    const int64_t k = map_out[e], kin = map_in[e];
    if (k < 0 || k >= nout || kin < 0 || kin >= m) return "selection map entry out of range";
    if (used[(size_t)k] == 2) return "selection map: more than two entries for one output bin";
    const size_t at = (size_t)used[(size_t)k]++ * nout + k;
    if (kin >= nchan) continue;                    // a bin of the zero padding
    const int64_t red = (kin * half) % m;          // e^{-2 pi i k_in floor(m/2) / m}
    const double a = -2.0 * M_PI * (double)red / (double)m;
    t.in[at] = (int32_t)kin;
    t.w[at] = map_w[e];
    t.phase[2 * at] = std::cos(a);
    t.phase[2 * at + 1] = std::sin(a);
  }
  for (int64_t q = 0; q < nout; ++q) {
    const double a = 2.0 * M_PI * (double)q / (double)nout;
    t.rtw[2 * q] = std::cos(a);
    t.rtw[2 * q + 1] = std::sin(a);
  }
  return nullptr;
}

// The bins of the resampled spectrum that each of nwin windows win [nwin][nchan] (null: all ones) feeds, increasing, in CSR form:
// list[ofs[w] .. ofs[w + 1]).  Fed: a term inside the span of the window's nonzero channels, or only a term at a nonzero channel.
enum class Feeds { kSpan, kNonzero };
inline void fed_bins(const ResampleTables& t, int64_t nout, int64_t nwin, int64_t nchan, const double* win, Feeds rule,
                     std::vector<int32_t>& ofs, std::vector<int32_t>& list) {
  ofs.assign((size_t)nwin + 1, 0);
  list.clear();
  for (int64_t w = 0; w < nwin; ++w) {
    const double* x = win ? win + w * nchan : nullptr;
    int64_t lo = x ? nchan : 0, hi = x ? 0 : nchan;
    for (int64_t n = 0; x && n < nchan; ++n)           // the span of the nonzero channels
      if (x[n] != 0.0) { lo = std::min(lo, n); hi = n + 1; }
    for (int64_t k = 0; k < nout; ++k)
      for (int s = 0; s < 2; ++s) {
        const int32_t i = t.in[(size_t)s * nout + k];
        if (i >= lo && i < hi && (rule == Feeds::kSpan || !x || x[i] != 0.0)) { list.push_back((int32_t)k); break; }
      }
    ofs[(size_t)w + 1] = (int32_t)list.size();
  }
}

}  // namespace pint

#endif  // PRISIM_ADDON_PLAN_H
