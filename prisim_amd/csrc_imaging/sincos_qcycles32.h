// sincos_qcycles32.h -- the fp32 sine and cosine of a phase that was reduced in fp64, for the fp32 imaging route (imaging32_kernels.h).
// A restatement, operation by operation and constant by constant, of sincos_qcycles(double, float&, float&) of
// ../csrc/skyvis_kernels.hip, which stays where it is: the committed profiles are pinned to the text of ../csrc (profiles/r06_MANIFEST.json,
// tests/test_host_logic.py), so nothing there is edited for a lift that would leave the sky-sum's code as it was.  Change the two together.
// Device code only.  Every fused operation is written as a builtin, so the bits do not depend on -ffp-contract.  Not part of the public
// ABI.
#ifndef PRISIM_SINCOS_QCYCLES32_H
#define PRISIM_SINCOS_QCYCLES32_H

#include <hip/hip_runtime.h>

namespace {

// ------------------------------------------------------------------------------------------
// sincos of an angle given in QUARTER CYCLES (a4 = 4 * phase[cycles], any magnitude < 2^31):
// returns (cos, sin) of 2 pi * phase.  The quadrant q = rint(a4) and the residual
// y = (a4 - q)/4 in [-1/8, 1/8] cycle are formed in fp64 (exact), so no separate reduction modulo
// one cycle is needed: q mod 4 selects the quadrant.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void sincos_qcycles(double a4, float& c, float& s) {
  const double q = __builtin_rint(a4);
  const float y = (float)((a4 - q) * 0.25);
  const int qi = (int)q;
  const float y2 = y * y;
  // sin(2 pi y) = y * (2pi + y^2 * (-(2pi)^3/3! + y^2 * ((2pi)^5/5! + y^2 * (-(2pi)^7/7! + y^2 * (2pi)^9/9!))))
  float ps = 42.058693944897655f;                          // (2pi)^9/9!
  ps = __builtin_fmaf(ps, y2, -76.70585975306136f);        // -(2pi)^7/7!
  ps = __builtin_fmaf(ps, y2, 81.60524927607504f);         // (2pi)^5/5!
  ps = __builtin_fmaf(ps, y2, -41.341702240399755f);       // -(2pi)^3/3!
  float sy = __builtin_fmaf(y * y2, ps, y * 6.2831855f);   // fl32(2pi) = 6.28318548
  sy = __builtin_fmaf(y, -1.7484555e-7f, sy);              // + y * (2pi - fl32(2pi))
  // cos(2 pi y) = 1 + y^2 * (-(2pi)^2/2 + y^2 * ((2pi)^4/4! + y^2 * (-(2pi)^6/6! + y^2 * ((2pi)^8/8! - y^2 (2pi)^10/10!))))
  float pc = -26.42625678337438f;                          // -(2pi)^10/10!
  pc = __builtin_fmaf(pc, y2, 60.24464137187666f);         // (2pi)^8/8!
  pc = __builtin_fmaf(pc, y2, -85.45681720669373f);        // -(2pi)^6/6!
  pc = __builtin_fmaf(pc, y2, 64.93939402266829f);         // (2pi)^4/4!
  pc = __builtin_fmaf(pc, y2, -19.739208802178716f);       // -(2pi)^2/2
  const float cy = __builtin_fmaf(pc, y2, 1.0f);
  // rotate by q quarter turns: q=0:(c,s) 1:(-s,c) 2:(-c,-s) 3:(s,-c)
  const bool swap = (qi & 1) != 0;
  const float cc = swap ? sy : cy;
  const float ss = swap ? cy : sy;
  c = (((qi + 1) & 2) != 0) ? -cc : cc;    // q mod 4 in {1,2}
  s = ((qi & 2) != 0) ? -ss : ss;          // q mod 4 in {2,3}
}

}  // namespace

#endif  // PRISIM_SINCOS_QCYCLES32_H
