// baseline_fold.h -- fold maps of an array's baseline vectors (host only, no HIP: it compiles alone).
//
// Every sky-sum kernel computes a row of the cube from that row's (bx, by, bz) and wave-uniform operands only, so rows whose vectors
// are equal receive equal sums.  fold_baselines() lists the distinct vectors in order of first appearance (`rep`: the first row that
// carries each) and maps every row to its entry (`map`).  Equality is by IEEE value with -0.0 == +0.0; the caller has rejected
// non-finite components.  First-appearance order keeps the length sorting of the rows, which the per-group tables (longest / shortest
// baseline of a group of 256) rely on.  O(nbl): one open-addressing table over a hash of the 24-byte key.
//
// fold_baselines_near() also merges vectors equal to rounding.  A redundant layout built by floating-point arithmetic gives
// lattice-equal baselines of different antenna pairs vectors that differ in their last bits (HERA-350: 10 999 distinct IEEE values, 7 090
// distinct vectors).  The rule: walk the rows in order; a row joins the earliest-founded cluster whose representative -- the cluster's
// first row -- lies within `tol` of it in EVERY component (|d| <= tol, so a row at exactly tol joins); otherwise it founds a cluster.
// Hence every member is within tol of its representative per component and nothing chains (a, a + 0.75 tol, a + 1.5 tol are two
// clusters: the third row is compared with a, never with the second), representatives are pairwise further apart than tol in some
// component, and `rep` ascends in first-appearance order as above.  The rows of a cluster are summed with the representative's vector,
// so a row's result moves by at most the phase 2 pi f / c |s - s_pc| |b - b_rep| <= 2 pi f / c * 2 * max_dev; `max_dev` returns the
// largest 2-norm |b - b_rep| of any row, and the caller (prisim_hip_set_array) holds that bound to its budget or keeps the exact fold.
// tol = 0 gives fold_baselines' result exactly.  O(nbl): a hash grid of cubic cells at least 2 tol wide; the representatives that can
// lie within tol of a row are in its cell or one of the 26 around it.
#pragma once
#include <cmath>
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

// As fold_baselines, with rows within `tol` (metres, per component) of a cluster's first row mapped to it (the rule above).
// max_dev: the largest 2-norm distance of a row from the representative it was mapped to.
inline void fold_baselines_near(const double* bl_enu, int64_t nbl, double tol, std::vector<int64_t>& rep, std::vector<int32_t>& map,
                                double& max_dev) {
  max_dev = 0.0;
  if (!(tol > 0.0)) { fold_baselines(bl_enu, nbl, rep, map); return; }
  rep.clear();
  map.assign((size_t)(nbl > 0 ? nbl : 0), 0);
  if (nbl <= 0) return;
  // Cell width: 2 tol, and at least 2^-50 of the largest |component| so that the cell indices stay below 2^51 in int64.  A quotient
  // v / w is then rounded by at most 1/8, two vectors within tol of each other have quotients at most 1/2 + 2/8 apart, and their
  // cell indices differ by at most one per axis.
  double pmax = 0.0;
  for (int64_t i = 0; i < 3 * nbl; ++i) pmax = std::fmax(pmax, std::fabs(bl_enu[i]));
  const double w = std::fmax(2.0 * tol, std::ldexp(pmax, -50));
  uint64_t cap = 16;
  while (cap < (uint64_t)nbl * 2) cap <<= 1;
  std::vector<int32_t> slot((size_t)cap, -1);       // entry of `cells`, or -1
  std::vector<int64_t> cells;                       // [ncell][3] cell indices
  std::vector<int32_t> head;                        // [ncell] last-founded cluster of the cell
  std::vector<int32_t> next;                        // [nu] the cluster founded before it in the same cell, or -1
  cells.reserve((size_t)nbl * 3);
  auto find_cell = [&](const int64_t c[3], bool insert) -> int32_t {
    uint64_t h = 0x9E3779B97F4A7C15ull;
    for (int i = 0; i < 3; ++i) {
      h ^= (uint64_t)c[i];
      h ^= h >> 30; h *= 0xBF58476D1CE4E5B9ull;
      h ^= h >> 27; h *= 0x94D049BB133111EBull;
      h ^= h >> 31;
    }
    uint64_t at = h & (cap - 1);
    for (;;) {
      const int32_t e = slot[(size_t)at];
      if (e < 0) {
        if (!insert) return -1;
        slot[(size_t)at] = (int32_t)head.size();
        cells.insert(cells.end(), c, c + 3);
        head.push_back(-1);
        return (int32_t)head.size() - 1;
      }
      const int64_t* q = &cells[(size_t)e * 3];
      if (q[0] == c[0] && q[1] == c[1] && q[2] == c[2]) return e;
      at = (at + 1) & (cap - 1);
    }
  };
  for (int64_t b = 0; b < nbl; ++b) {
    const double* v = bl_enu + 3 * b;
    int64_t c[3];
    for (int i = 0; i < 3; ++i) c[i] = (int64_t)std::floor(v[i] / w);
    int64_t best = -1;                              // the earliest-founded cluster within tol
    for (int64_t dx = -1; dx <= 1; ++dx)
      for (int64_t dy = -1; dy <= 1; ++dy)
        for (int64_t dz = -1; dz <= 1; ++dz) {
          const int64_t n[3] = {c[0] + dx, c[1] + dy, c[2] + dz};
          const int32_t cell = find_cell(n, false);
          if (cell < 0) continue;
          for (int32_t e = head[(size_t)cell]; e >= 0; e = next[(size_t)e]) {
            if (best >= 0 && e > best) continue;
            const double* r = bl_enu + 3 * rep[(size_t)e];
            if (std::fabs(v[0] - r[0]) <= tol && std::fabs(v[1] - r[1]) <= tol && std::fabs(v[2] - r[2]) <= tol) best = e;
          }
        }
    if (best < 0) {
      const int32_t cell = find_cell(c, true);
      next.push_back(head[(size_t)cell]);
      head[(size_t)cell] = (int32_t)rep.size();
      map[(size_t)b] = (int32_t)rep.size();
      rep.push_back(b);
    } else {
      map[(size_t)b] = (int32_t)best;
      const double* r = bl_enu + 3 * rep[(size_t)best];
      const double d0 = v[0] - r[0], d1 = v[1] - r[1], d2 = v[2] - r[2];
      max_dev = std::fmax(max_dev, std::sqrt(d0 * d0 + d1 * d1 + d2 * d2));
    }
  }
}

// ---- which fold prisim_hip_set_array takes ----
// The tolerance is rounding noise of the layout arithmetic, scaled with the coordinates: 16 ulp of the largest |component| P (2.07e-12 m
// for HERA-350's 583 m).  An array whose coordinates carry a large offset simply merges nothing.
inline double fold_near_tol(const double* bl_enu, int64_t nbl) {
  double pmax = 0.0;
  for (int64_t i = 0; i < 3 * nbl; ++i) pmax = std::fmax(pmax, std::fabs(bl_enu[i]));
  return 16.0 * 0x1p-52 * pmax;
}

// The phase a merged row can move by: 2 pi f_max / c |s - s_pc| |b - b_rep| with |s - s_pc| <= 2.  The budget of 1e-12 rad is a tenth
// of the fp64 tolerance (1e-11 of sum|pbflux|) and 2e-7 of the fp32 one.
constexpr double kFoldNearPhaseBudget = 1e-12;
inline double fold_near_phase_bound(double max_dev, double fmax_hz) {
  return 2.0 * 3.14159265358979323846 * std::fabs(fmax_hz) / 299792458.0 * 2.0 * max_dev;
}

enum FoldKind { kFoldNone = 0, kFoldExact = 1, kFoldNear = 2 };
// A fold is worth its expansion pass when it removes at least an eighth of the rows, and it must leave more than `min_rows` (one
// baseline group) so that a folded context never enters the small-array paths.  The merged fold is taken when it has fewer rows than
// the exact one, meets those conditions and realises a phase bound within the budget; otherwise the exact fold under the same
// conditions; otherwise none.
inline FoldKind choose_fold(int64_t nbl, int64_t n_exact, int64_t n_near, double near_phase_bound, int64_t min_rows, bool allow_near) {
  if (allow_near && n_near < n_exact && n_near * 8 <= nbl * 7 && n_near > min_rows && near_phase_bound <= kFoldNearPhaseBudget) return kFoldNear;
  if (n_exact * 8 <= nbl * 7 && n_exact > min_rows) return kFoldExact;
  return kFoldNone;
}

}  // namespace prisim
