// delay_lines.h -- the arithmetic of a delay line, stated once for the add-ons that turn rows of channels into delay spectra (subband.hip,
// runs.hip, cpdelay.hip, cpft.hip).  The device functions round the same products in the same order as the kernels that wrote them out
// did.  Not part of the public ABI.
#ifndef PRISIM_DELAY_LINES_H
#define PRISIM_DELAY_LINES_H

#include "addon_internal.h"
#include "../../include/prisim_cpft.h"
#include "../../include/prisim_runs.h"

namespace pint {

// the resampling tables on the device: per term of a bin its channel (-1: none) and coefficient, [..][2][nres]; the twiddles e^{+2 pi i q / nres};
// the bins window w feeds, list[ofs[w] .. ofs[w + 1]) (fed_bins)
struct ResampleDev { int32_t *in = nullptr, *ofs = nullptr, *list = nullptr; double2 *c = nullptr, *rtw = nullptr; };
inline int upload_resample(prisim_ctx* ctx, Dev& dev, ResampleDev& d, const std::vector<int32_t>& in, const std::vector<double>& c,
                           const std::vector<double>& rtw, const std::vector<int32_t>& ofs, const std::vector<int32_t>& list, hipStream_t s) {
  DEV_UPLOAD(ctx, dev, d.in, in, s);
  DEV_UPLOAD(ctx, dev, d.c, c, s);
  DEV_UPLOAD(ctx, dev, d.rtw, rtw, s);
  DEV_UPLOAD(ctx, dev, d.ofs, ofs, s);
  DEV_UPLOAD(ctx, dev, d.list, list, s);
  return PRISIM_OK;
}

// The shifted inverse transform.  With even m, m df fftshift(ifft(x))[j] = df sum_n x[n] (-1)^n e^{+2 pi i j n / m}: the sign and the scale s
// are folded into sample n as it is stored bit-reversed into LDS, and lds_ifft_dit leaves the shifted spectrum in natural order (m = 1 has
// no shift).  A sample that does not exist (padding, outside a window) is shifted_zero's +0, not 0 * -s.
struct LdsOperand { int slot; double2 v; };
__device__ __forceinline__ LdsOperand shifted_operand(double2 v, int n, int m, int logm, double s) { return {bitrev(n, logm), rmul(v, (m > 1 && (n & 1)) ? -s : s)}; }
__device__ __forceinline__ LdsOperand shifted_zero(int n, int logm) { return {bitrev(n, logm), make_double2(0.0, 0.0)}; }

// The same shift behind rocFFT's unnormalised inverse transform F, spectrum[i] = s F[(i - floor(m/2)) mod m]: the transform bin that lag i
// gathers, and the lag that transform bin jf scatters to.
__device__ __forceinline__ int shift_source(int i, int m) { return (i + m - m / 2) % m; }
__device__ __forceinline__ int shift_target(int jf, int m) { return (jf + m / 2) % m; }

// Bin k of scipy.signal.resample's spectrum: at most two terms x(in) c, slot 0 then slot 1, from tables [2][stride]; a term whose channel
// is outside [lo, hi), as -1 is, is none.  x and c are read inside the condition: loading an absent term's coefficient measured slower.
template <typename X>
__device__ __forceinline__ double2 resampled_bin(X x, const int32_t* in, const double2* c, int stride, int k, int lo = 0, int hi = INT32_MAX) {
  double2 v = make_double2(0.0, 0.0);
  for (int s = 0; s < 2; ++s)                         // two constant trips: unrolled
    if (const int i = in[s * stride + k]; i >= lo && i < hi) v = cadd(v, cmul(x(i), c[s * stride + k]));
  return v;
}

// y[q] = sum_i Y e^{+2 pi i k q / nres} over the nz fed bins k = bins[i], in increasing i from (0, 0).  Y is `stride` apart and indexed by
// the bin k, or (COMPACT) by its place i in the list.  k q is reduced in 32 bits: k, q < 4096, so k q < 2^24.
template <bool COMPACT>
__device__ __forceinline__ double2 direct_sum(const double2* Y, int stride, const int* bins, int nz, int q, int nres, const double2* rtw) {
  static_assert(PRISIM_SUBBAND_MAX_LEN <= 4096 && PRISIM_RUNS_MAX_LEN <= 4096 && PRISIM_CPDELAY_MAX_LEN <= 4096 && PRISIM_CPFT_MAX_LEN <= 4096, "");
  double2 acc = make_double2(0.0, 0.0);
  for (int i = 0; i < nz; ++i) acc = cadd(acc, cmul(Y[(COMPACT ? i : bins[i]) * stride], rtw[(bins[i] * q) % nres]));
  return acc;
}

__device__ __forceinline__ double power_of(double2 v, double ps) { return (v.x * v.x + v.y * v.y) * ps; }   // |v|^2 ps

}  // namespace pint

#endif  // PRISIM_DELAY_LINES_H
