// csclean_plan.h -- how prisim_clean_image_cs (../csrc_imaging/csclean.hip) plans a call: what imclean_plan.h plans of the dirty
// image and of the peak search, the offset lattice of the minor-cycle beam with its half-plane, where the working image of a minor
// cycle lives, and the device bytes by buffer.  Everything is resident for the whole call: one that does not fit the budget is refused
// with the bytes it needs.  Plain C++ without HIP, so that a host program can check it (tests/csclean_plan_main.cpp).  Not part of
// the public ABI.
#ifndef PRISIM_CSCLEAN_PLAN_H
#define PRISIM_CSCLEAN_PLAN_H

#include <algorithm>
#include <cstdint>

#include "imclean_plan.h"

namespace pint {

constexpr int kCscleanAuto = -1, kCscleanLds = 0, kCscleanGlobal = 1;   // PRISIM_CSCLEAN_AUTO, _LDS, _GLOBAL
constexpr int64_t kCscleanMaxMajor = 65536;                              // PRISIM_CSCLEAN_MAX_MAJOR
constexpr int64_t kCscleanMinorStatic = 64;                              // LDS of a minor-cycle workgroup besides the image: one partial peak per wave

// The plan of a call: `base` is that of prisim_clean_image for the same image (its budget is not looked at), the rest is what the
// cycles add.  psf_full = (2 ny - 1)(2 nx - 1) offsets of P, of which the psf_half = ny (2 nx - 1) - nx + 1 from the centre on, in
// row-major order, are computed and the others mirrored.
// Device bytes, all resident for the whole call, beside those of `base` (dd, resid, scratch, lists, partials, state, window):
//   vres      [nt][nbl][nchan] complex128: the uploaded cube itself, or the copy of the resident one
//   psf       [nc][psf_full] P, 8 B
//   psf_work  the half-plane: its offsets [nt][psf_half] 32 B and its rows [psf_half][nchan] 8 B, with chan_avg its band sums
//             [psf_half] 8 B
//   cycles    per image channel: the cycle's flag, first component and count of cycles 4 B each, the peak of the cycle before and
//             the limit 8 B each; the tables [nc][max_major] 4 B and [nc][max_major + 1] 8 B
//   minor     [nc][npix] 8 B, the working images of the GLOBAL route; 0 on the LDS route
// refusal: null, or why the call cannot run; `total` is then still the bytes the call needs (0 where the sizes themselves are
// refused).
struct CscleanPlan {
  ImcleanPlan base;
  int minor_route;
  int64_t ny, nx, psf_full, psf_half, minor_lds;
  int64_t vres_bytes, psf_bytes, psf_work_bytes, cycle_bytes, minor_bytes, total;
  const char* refusal;
};
inline CscleanPlan csclean_plan(int64_t npix, int64_t ny, int64_t nx, int64_t nbl, int64_t nchan, int64_t nt, bool chan_avg, int64_t maxiter,
                                double cycle_depth, int64_t max_major, int64_t budget_bytes, int64_t lds_max, int asked, bool uniform,
                                int asked_minor) {
  CscleanPlan p{};
  p.base = imclean_plan(npix, nbl, nchan, nt, chan_avg, maxiter, int64_t(1) << 62, lds_max, asked, uniform);
  p.ny = ny;
  p.nx = nx;
  p.minor_route = asked_minor == kCscleanGlobal ? kCscleanGlobal : kCscleanLds;
  if (npix < 1 || nbl < 1 || nchan < 1 || nt < 1 || npix > kImcleanMaxPixels || nchan > (int64_t(1) << 20) || nt > (int64_t(1) << 30) ||
      nbl > (int64_t(1) << 30) || npix > (int64_t(1) << 46) / nchan || maxiter < 0 || maxiter > kImcleanMaxIter || asked < -1 ||
      asked > kImagingStepped) {
    p.refusal = p.base.refusal;                         // the sizes themselves: nothing is counted
    return p;
  }
  if (ny < 1 || nx < 1 || ny > npix || nx > npix || ny * nx != npix) { p.refusal = "ny * nx must be npix, both at least 1"; return p; }
  if (!(cycle_depth > 0.0 && cycle_depth < 1.0)) { p.refusal = "cycle_depth must lie in (0, 1)"; return p; }
  if (max_major < 0 || max_major > kCscleanMaxMajor) { p.refusal = "max_major must lie in [0, 65536]"; return p; }
  if (asked_minor < kCscleanAuto || asked_minor > kCscleanGlobal) { p.refusal = "unknown minor_route"; return p; }
  constexpr int64_t cap = int64_t(1) << 56;
  auto times = [](int64_t a, int64_t b) { return a > cap / std::max<int64_t>(b, 1) ? cap : a * b; };
  p.psf_full = (2 * ny - 1) * (2 * nx - 1);             // npix <= 2^28: below 2^30
  p.psf_half = ny * (2 * nx - 1) - nx + 1;
  p.minor_lds = npix * 8 + kCscleanMinorStatic;
  const bool fits = p.minor_lds <= lds_max;
  if (asked_minor == kCscleanAuto) p.minor_route = fits ? kCscleanLds : kCscleanGlobal;
  if (p.minor_route == kCscleanGlobal) p.minor_lds = kCscleanMinorStatic;
  p.vres_bytes = times(times(times(nt, nbl), nchan), 16);
  p.psf_bytes = times(times(p.base.nc, p.psf_full), 8);
  p.psf_work_bytes = std::min(cap, times(times(nt, p.psf_half), 32) + times(times(p.psf_half, nchan), 8) + (chan_avg ? p.psf_half * 8 : 0));
  p.cycle_bytes = std::min(cap, p.base.nc * 28 + times(p.base.nc, max_major) * 4 + times(p.base.nc, max_major + 1) * 8);
  p.minor_bytes = p.minor_route == kCscleanGlobal ? times(times(p.base.nc, npix), 8) : 0;
  p.total = std::min(cap, p.base.total + p.vres_bytes + p.psf_bytes + p.psf_work_bytes + p.cycle_bytes + p.minor_bytes);
  if (p.base.refusal) { p.refusal = p.base.refusal; return p; }     // the route and the LDS of the dirty image
  if (asked_minor == kCscleanLds && !fits) { p.refusal = "the working image of a minor cycle does not fit in the LDS of the device"; return p; }
  if (p.total > budget_or_default(budget_bytes)) { p.refusal = "budget_bytes cannot hold the resident buffers"; return p; }
  return p;
}

}  // namespace pint

#endif  // PRISIM_CSCLEAN_PLAN_H
