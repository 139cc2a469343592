// baseline_fold.h -- fold map of an array's baseline vectors (host only, no HIP: it compiles alone).
//
// Every sky-sum kernel computes a row of the cube from that row's (bx, by, bz) and wave-uniform operands only, so rows whose vectors
// are equal receive equal sums.  fold_baselines() lists the distinct vectors in order of first appearance (`rep`: the first row that
// carries each) and maps every row to its entry (`map`).  Equality is by IEEE value with -0.0 == +0.0; the caller has rejected
// non-finite components.  Near-equal vectors are NOT merged: a row's result stays exactly what the kernel computes for its vector.
// First-appearance order keeps the length sorting of the rows, which the per-group tables (longest / shortest baseline of a group of
// 256) rely on.  O(nbl): one open-addressing table over a hash of the 24-byte key.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

namespace prisim {

// bl_enu: [nbl][3].  rep: [nu] row indices, ascending.  map: [nbl], map[b] in [0, nu), rep[map[b]] <= b.
inline void fold_baselines(const double* bl_enu, int64_t nbl, std::vector<int64_t>& rep, std::vector<int32_t>& map) {
  rep.clear();
  map.assign((size_t)(nbl > 0 ? nbl : 0), 0);
  if (nbl <= 0) return;
  uint64_t cap = 16;
  while (cap < (uint64_t)nbl * 2) cap <<= 1;
  std::vector<int32_t> slot((size_t)cap, -1);       // entry of `rep`, or -1
  std::vector<uint64_t> keys;                       // [nu][3] canonical bit patterns
  keys.reserve((size_t)nbl * 3);
  for (int64_t b = 0; b < nbl; ++b) {
    uint64_t k[3];
    for (int i = 0; i < 3; ++i) {
      double v = bl_enu[3 * b + i];
      if (v == 0.0) v = 0.0;                        // -0.0 -> +0.0
      memcpy(&k[i], &v, sizeof v);
    }
    uint64_t h = 0x9E3779B97F4A7C15ull;
    for (int i = 0; i < 3; ++i) {                   // splitmix64 finaliser over the three words
      h ^= k[i];
      h ^= h >> 30; h *= 0xBF58476D1CE4E5B9ull;
      h ^= h >> 27; h *= 0x94D049BB133111EBull;
      h ^= h >> 31;
    }
    uint64_t at = h & (cap - 1);
    for (;;) {
      const int32_t e = slot[(size_t)at];
      if (e < 0) {
        slot[(size_t)at] = (int32_t)rep.size();
        map[(size_t)b] = (int32_t)rep.size();
        rep.push_back(b);
        keys.insert(keys.end(), k, k + 3);
        break;
      }
      const uint64_t* q = &keys[(size_t)e * 3];
      if (q[0] == k[0] && q[1] == k[1] && q[2] == k[2]) { map[(size_t)b] = e; break; }
      at = (at + 1) & (cap - 1);
    }
  }
}

}  // namespace prisim
