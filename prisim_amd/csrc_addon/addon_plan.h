// addon_plan.h -- the arithmetic that the add-on entries plan their calls with: the transform length as a power of two and the
// chunks of a chunk loop.  Plain C++ without HIP, so that a host program can check it (tests/test_addon_plan.py).  Not part of
// the public ABI.
#ifndef PRISIM_ADDON_PLAN_H
#define PRISIM_ADDON_PLAN_H

#include <algorithm>
#include <cstdint>

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

// n items in `count` chunks of `size` (the last of `last`, 1 <= last <= size), dealt round-robin to nstreams streams
struct Chunks {
  int64_t size, count, last;
  int nstreams;
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

}  // namespace pint

#endif  // PRISIM_ADDON_PLAN_H
