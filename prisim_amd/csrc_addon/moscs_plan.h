// moscs_plan.h -- how prisim_clean_mosaic_cs (../csrc_imaging/moscs.hip) plans a call: the bytes of prisim_clean_mosaic
// (mosclean_plan.h) and what the cycles of prisim_clean_image_cs add to an image (csclean_plan.h), each asked of its own header and
// not restated, plus the scale table of the flat-noise image.  Everything is resident for the whole call: one that does not fit the
// budget is refused with the bytes it needs.  Plain C++ without HIP, so that a host program can check it (tests/moscs_plan_main.cpp).
// Not part of the public ABI.
#ifndef PRISIM_MOSCS_PLAN_H
#define PRISIM_MOSCS_PLAN_H

#include <algorithm>
#include <cstdint>

#include "csclean_plan.h"
#include "mosclean_plan.h"

namespace pint {

// The plan of a call.  mos: the plan of prisim_clean_mosaic for the same sizes and cyc: that of prisim_clean_image_cs, both under a
// budget that refuses nothing they can count; from mos the geometry of the passes and of the peak search and its bytes, from cyc the
// lattice of P, the route of the minor cycle and the bytes of the cycles.
// Device bytes, all resident for the whole call:
//   mos.total            what prisim_clean_mosaic holds: dirs, beam, sums, flat, out, window, lists, partials, state
//   cyc.vres_bytes       [nt][nbl][nchan] complex128: the uploaded cube itself, or the copy of the resident one
//   cyc.psf_bytes        [nc][psf_full] P
//   cyc.psf_work_bytes   the half-plane of P: its offsets, its rows, with chan_avg its band sums
//   psf_norm_bytes       the weight sums P is divided by, in the order of prisim_dirty_image: 8 B a channel and 8 for their sum
//   cyc.cycle_bytes      the cycle state and tables
//   cyc.minor_bytes      [nc][npix] 8 B, the working images of the GLOBAL route; 0 on the LDS route
//   scale_bytes          [npix][nc] 8 B: s = sqrt(Wc / Qc)
// refusal: null, or why the call cannot run -- the union of the parents' refusals, each through its own check, the mosaic's first;
// `total` is then still the bytes the call needs (0 where the sizes themselves are refused).
struct MoscsPlan {
  MoscleanPlan mos;
  CscleanPlan cyc;
  int64_t psf_norm_bytes, scale_bytes, total;
  const char* refusal;
};
inline MoscsPlan moscs_plan(int64_t npix, int64_t ny, int64_t nx, int64_t nbl, int64_t nchan, int64_t nt, bool chan_avg, int64_t maxiter,
                            double cycle_depth, int64_t max_major, int64_t budget_bytes, int64_t lds_max, int asked, bool uniform,
                            int asked_minor) {
  MoscsPlan p{};
  constexpr int64_t cap = int64_t(1) << 56;             // that of the parents: no total is formed beyond it
  p.mos = mosclean_plan(npix, nbl, nchan, nt, chan_avg, maxiter, cap, lds_max, asked, uniform);
  p.cyc = csclean_plan(npix, ny, nx, nbl, nchan, nt, chan_avg, maxiter, cycle_depth, max_major, cap, lds_max, asked, uniform, asked_minor);
  // the sizes, the route and the LDS of a pass; then the lattice, the depth, the cycles and the route of the minor cycle
  if (p.mos.refusal && p.mos.total == 0) { p.refusal = p.mos.refusal; return p; }
  if (p.cyc.refusal && p.cyc.total == 0) { p.refusal = p.cyc.refusal; return p; }
  auto times = [](int64_t a, int64_t b) { return a > cap / std::max<int64_t>(b, 1) ? cap : a * b; };
  p.psf_norm_bytes = nchan * 8 + 8;
  p.scale_bytes = times(times(npix, p.mos.clean.nc), 8);
  int64_t total = 0;
  for (int64_t b : {p.mos.total, p.cyc.vres_bytes, p.cyc.psf_bytes, p.cyc.psf_work_bytes, p.psf_norm_bytes, p.cyc.cycle_bytes, p.cyc.minor_bytes,
                    p.scale_bytes})
    total = std::min(cap, total + b);                   // eight terms of at most 2^56: no overflow
  p.total = total;
  if (p.mos.refusal) { p.refusal = p.mos.refusal; return p; }
  if (p.cyc.refusal) { p.refusal = p.cyc.refusal; return p; }
  if (p.total > budget_or_default(budget_bytes)) { p.refusal = "budget_bytes cannot hold the resident buffers"; return p; }
  return p;
}

}  // namespace pint

#endif  // PRISIM_MOSCS_PLAN_H
