// noise_draw.h -- the thermal-noise draw: Philox-4x32-10 counter-based normals (Salmon et al. 2011) and the Box-Muller statement, for
// the two translation units that draw noise (aux_kernels.hip: k_noise; ../csrc_closure/cpreal.hip), so that they cannot drift.
// aux_kernels.hip is built with contraction on and the add-ons with it off; the statement has no a * b + c shape, and the pragma pins
// that: both units round every product and sum once.  Not part of the public ABI.
#ifndef PRISIM_NOISE_DRAW_H
#define PRISIM_NOISE_DRAW_H

#include <hip/hip_runtime.h>

#include <cstdint>

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t out[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    const uint32_t n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// rms/sqrt(2) * (n1 + i n2) of (channel f, global baseline g, snapshot t) under the key `seed`: counter = (f, g low, t, g high)
__device__ __forceinline__ double2 noise_draw(int64_t f, int64_t g, int64_t t, uint64_t seed, double rms) {
#pragma clang fp contract(off)
  uint32_t r[4];
  philox4x32_10((uint32_t)f, (uint32_t)g, (uint32_t)t, (uint32_t)((uint64_t)g >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), r);
  // two 52-bit uniforms in (0,1], Box-Muller
  const double u1 = ((double)(((uint64_t)r[0] << 20) | (r[1] >> 12)) + 1.0) * (1.0 / 4503599627370496.0);
  const double u2 = ((double)(((uint64_t)r[2] << 20) | (r[3] >> 12))) * (1.0 / 4503599627370496.0);
  const double rad = sqrt(-2.0 * log(u1));
  double sn, cs;
  sincospi(2.0 * u2, &sn, &cs);
  const double sc = rms * 0.70710678118654752440;                      // :6692 sqrt(2) split
  return make_double2(sc * rad * cs, sc * rad * sn);
}

#endif  // PRISIM_NOISE_DRAW_H
