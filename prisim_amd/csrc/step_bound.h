// step_bound.h -- largest channel-to-channel step phase of a baseline group (host only, no HIP: it compiles alone).
//
// The leapfrog (lifting) rotation and the non-re-anchored taper bodies are used for a group of 256 baselines only when the step
// phase theta = b . (s - s_pc) df / c stays within 1/8 cycle (fp32; 1/4 cycle in fp64) for every baseline of the group and every
// source of the sky.  Two rigorous bounds of max |b . e|, e = s - s_pc, from tables that exist per group and per sky:
//   whole vectors (Cauchy-Schwarz):  |b . e| <= |b| |e|                              <= maxlen dmax
//   per axis (horizontal, vertical): |b . e| <= |b_xy| |e_xy| + |b_z| |e_z|          <= maxh hmax + maxz zmax
// with maxlen / maxh / maxz the group's largest |b|, |b_xy|, |b_z| and dmax / hmax / zmax the sky's largest |e|, |e_xy|, |e_z|.
// The second does not charge a horizontal baseline for the vertical part of e; the smaller of the two is used.  k_lift_flags
// (catalog_kernels.hip) evaluates the same products, sum, minimum, product and quotient in the same order with separately rounded
// operations, so the host's count and the device's flags agree group for group.
#pragma once
#include <cmath>

namespace prisim {

constexpr double kStepBoundC = 299792458.0;      // m / s

// Largest |step phase| of the group, in cycles.
inline double step_bound_cycles(double maxlen, double maxh, double maxz, double dmax, double hmax, double zmax, double df) {
  const double whole = maxlen * dmax;
  const double h = maxh * hmax;
  const double z = maxz * zmax;
  const double axes = h + z;
  const double m = whole < axes ? whole : axes;
  return m * std::fabs(df) / kStepBoundC;
}

// The limit the bound is held against: 1/8 cycle for the fp32 kernels, 1/4 cycle for the fp64 kernels (where the angle error
// alpha * eps is irrelevant and only tan(alpha / 2) must stay bounded), a hair inside.
inline double step_limit_cycles(bool f32) { return (f32 ? 0.125 : 0.25) * (1.0 - 1e-9); }

inline bool step_flag(double maxlen, double maxh, double maxz, double dmax, double hmax, double zmax, double df, bool f32) {
  return step_bound_cycles(maxlen, maxh, maxz, dmax, hmax, zmax, df) <= step_limit_cycles(f32);
}

}  // namespace prisim
