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

// The WIDE limit of the fp32 leapfrog (the packed kernel without the taper only), a hair inside like step_limit_cycles.  Past 1/8 cycle
// the leapfrog needs a sine that holds its relative precision there (sin_2pi_y_wide) and its conditioning 1 / cos(alpha) grows
// smoothly: 1.41 at 1/8 cycle, 2.12 at the value below, 2.61 at 3/16.  The value is MEASURED (profiles/LOG.md 4.1.10): the
// largest multiple of 1/64 cycle at which the worst error of a single source carrying all the flux, at the direction of the group's
// largest step and for both signs of the step, stays within half the fp32 tolerance (2.5e-6 of the flux) on the GPU.  Measured over
// 2.1e6 (baseline, channel) chains per step: 1.84e-6 at 9/64, 2.08e-6 at 10/64, 2.48e-6 at 11/64, 2.98e-6 at 12/64, 4.75e-6 at 13/64.
constexpr double kStepWideCycles = 11.0 / 64.0;
inline double step_wide_limit_cycles() { return kStepWideCycles * (1.0 - 1e-9); }

// 0: plain rotation; 1: within step_limit_cycles (what step_flag says); 2: beyond it but within the wide limit (fp32 only: the fp64
// limit is 1/4 cycle already).  The device forms tier >= 1 as a second table of k_lift_flags with the wide limit.
inline int step_tier(double maxlen, double maxh, double maxz, double dmax, double hmax, double zmax, double df, bool f32) {
  const double step = step_bound_cycles(maxlen, maxh, maxz, dmax, hmax, zmax, df);
  if (step <= step_limit_cycles(f32)) return 1;
  return (f32 && step <= step_wide_limit_cycles()) ? 2 : 0;
}

}  // namespace prisim
