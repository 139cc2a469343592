// Stand-alone check of prisim_amd/csrc_addon/moscs_plan.h (tests/test_moscs.py builds it with -fsanitize=address,undefined and runs
// it): the bytes of prisim_clean_mosaic and what the cycles of prisim_clean_image_cs add, stated by hand and asked of the parents'
// plans, the scale table, the budget from one byte short to ample, every route request and the refusals of both parents.  Grid: 1 to
// 2^20 pixels, square and not, x 1, 33, 1024 channels x 1, 3 snapshots x chan_avg.  Prints "checked N bad M" and returns 1 when
// anything is wrong.
#include "moscs_plan.h"

#include <cstdint>
#include <cstdio>
#include <cstring>

using namespace pint;

namespace {

long bad = 0, checked = 0;

void expect(bool ok, const char* what, int64_t a = 0, int64_t b = 0, int64_t c = 0) {
  ++checked;
  if (ok) return;
  ++bad;
  std::printf("%s (%lld, %lld, %lld)\n", what, (long long)a, (long long)b, (long long)c);
}

// the bytes of a call by the statements of the three headers, buffer by buffer
int64_t by_hand(int64_t ny, int64_t nx, int64_t nbl, int64_t nchan, int64_t nt, bool avg, int64_t maxiter, int64_t max_major, bool global) {
  const int64_t nc = avg ? 1 : nchan, npix = ny * nx, full = (2 * ny - 1) * (2 * nx - 1), half = (full + 1) / 2;
  const int64_t block = kImagingBlock, nblocks = (npix + block - 1) / block, slab = block * ((nblocks + kImcleanMaxSlabs - 1) / kImcleanMaxSlabs),
                nslabs = (npix + slab - 1) / slab;
  // prisim_clean_mosaic: dirs, beam, sums, flat, out, window, lists, partials, state
  const int64_t mos = 64 * nt * npix + 8 * nt * npix * nchan + 16 * npix * nchan + 8 * npix * nc + 16 * npix * nc + npix + 12 * nc * maxiter +
                      16 * nslabs * nc + (36 * nc + 8 * (nt + 1) * nchan + 8 + 16);
  // the cycles: Vres, P, its half-plane, its weight sums, the state and tables, the scratch, the scale
  return mos + 16 * nt * nbl * nchan + 8 * nc * full + (32 * nt * half + 8 * half * nchan + (avg ? 8 * half : 0)) + (8 * nchan + 8) +
         (28 * nc + 4 * nc * max_major + 8 * nc * (max_major + 1)) + (global ? 8 * nc * npix : 0) + 8 * npix * nc;
}

}  // namespace

int main() {
  const int64_t lds950 = 160 * 1024, nbl = 300, maxiter = 25, max_major = 4;
  const int64_t grids[][2] = {{1, 1}, {7, 9}, {9, 7}, {63, 1}, {1, 63}, {25, 40}, {40, 25}, {128, 128}, {144, 144}, {1024, 1024}, {512, 2048}, {1, 1 << 20}};
  const int64_t chans[] = {1, 33, 1024};
  const int64_t snaps[] = {1, 3};
  for (const auto& g : grids)
    for (int64_t nchan : chans)
      for (int64_t nt : snaps)
        for (int avg = 0; avg < 2; ++avg) {
          const int64_t ny = g[0], nx = g[1], npix = ny * nx, nc = avg ? 1 : nchan;
          const bool fits = npix * 8 + kCscleanMinorStatic <= lds950;
          for (int minor = -1; minor <= 1; ++minor) {
            const bool global = minor == kCscleanGlobal || (minor == kCscleanAuto && !fits);
            const MoscsPlan free_plan = moscs_plan(npix, ny, nx, nbl, nchan, nt, avg != 0, maxiter, 0.3, max_major, int64_t(1) << 60, lds950, -1, true, minor);
            if (minor == kCscleanLds && !fits) {
              expect(free_plan.refusal && std::strstr(free_plan.refusal, "LDS"), "an LDS route that does not fit accepted", ny, nx, nchan);
              continue;
            }
            expect(!free_plan.refusal, "an ample budget is refused", ny, nx, nchan);
            const int64_t need = free_plan.total;
            expect(need == by_hand(ny, nx, nbl, nchan, nt, avg != 0, maxiter, max_major, global), "the bytes are not those of the statement", ny, nx, need);
            expect(need > 0 && need < (int64_t(1) << 56), "the total overflowed", ny, nx, need);
            // the parents, asked on their own
            const MoscleanPlan mos = mosclean_plan(npix, nbl, nchan, nt, avg != 0, maxiter, int64_t(1) << 60, lds950, -1, true);
            const CscleanPlan cyc = csclean_plan(npix, ny, nx, nbl, nchan, nt, avg != 0, maxiter, 0.3, max_major, int64_t(1) << 60, lds950, -1, true, minor);
            expect(!mos.refusal && !cyc.refusal && need == mos.total + (cyc.total - cyc.base.total) + 8 * nchan + 8 + 8 * npix * nc,
                   "the bytes are not the parents' with the scale and the weight sums of P", ny, nx, need);
            const int64_t budgets[] = {need - 1, need, need + 1, 2 * need, 0};
            for (int64_t budget : budgets)
              for (int asked = -1; asked <= 1; ++asked)
                for (int uniform = 0; uniform < 2; ++uniform) {
                  const MoscsPlan p = moscs_plan(npix, ny, nx, nbl, nchan, nt, avg != 0, maxiter, 0.3, max_major, budget, lds950, asked, uniform != 0, minor);
                  if (asked == kImagingStepped && !uniform) {
                    expect(p.refusal && std::strstr(p.refusal, "uniform"), "stepped on a non-uniform grid accepted", ny, nx);
                    continue;
                  }
                  const int64_t sum = p.mos.total + p.cyc.vres_bytes + p.cyc.psf_bytes + p.cyc.psf_work_bytes + p.psf_norm_bytes + p.cyc.cycle_bytes +
                                      p.cyc.minor_bytes + p.scale_bytes;
                  expect(sum == p.total && p.total == need, "the buffers do not sum to the total", ny, nx, p.total);
                  if (need > budget_or_default(budget)) {
                    expect(p.refusal && std::strstr(p.refusal, "resident buffers"), "a call beyond the budget accepted", ny, nx, budget);
                    continue;
                  }
                  bool ok = p.refusal == nullptr;
                  const int route = asked >= 0 ? asked : uniform ? kImagingStepped : kImagingDirect;
                  ok = ok && p.mos.clean.route == route && p.cyc.base.route == route && p.mos.clean.nc == nc;
                  ok = ok && p.cyc.minor_route == (global ? kCscleanGlobal : kCscleanLds);
                  ok = ok && p.cyc.minor_lds == (global ? kCscleanMinorStatic : npix * 8 + kCscleanMinorStatic) && p.cyc.minor_lds <= lds950;
                  ok = ok && (global ? p.cyc.minor_bytes == 8 * nc * npix : p.cyc.minor_bytes == 0) && p.scale_bytes == 8 * nc * npix;
                  ok = ok && 2 * p.cyc.psf_half - 1 == p.cyc.psf_full && p.cyc.vres_bytes == 16 * nt * nbl * nchan && p.mos.lds == kImagingLds + 20 * kImagingTile;
                  expect(ok, "an unsound plan", ny, nx, budget);
                }
          }
        }
  // the arguments themselves: the union of the parents' refusals
  const int64_t big = int64_t(1) << 60;
  auto plan = [&](int64_t npix, int64_t ny, int64_t nx, int64_t nchan, int64_t maxit, double depth, int64_t major, int64_t lds, int asked, bool uniform,
                  int minor) { return moscs_plan(npix, ny, nx, 10, nchan, 1, false, maxit, depth, major, big, lds, asked, uniform, minor); };
  expect(plan(63, 7, 9, 5, 5, 0.3, 4, lds950, -1, true, -1).refusal == nullptr, "7 x 9");
  expect(plan(63, 7, 8, 5, 5, 0.3, 4, lds950, -1, true, -1).refusal != nullptr, "7 x 8 for 63 pixels");
  expect(plan(63, 0, 63, 5, 5, 0.3, 4, lds950, -1, true, -1).refusal != nullptr, "ny 0");
  expect(plan(63, -7, -9, 5, 5, 0.3, 4, lds950, -1, true, -1).refusal != nullptr, "negative sides");
  expect(plan(63, int64_t(1) << 40, int64_t(1) << 40, 5, 5, 0.3, 4, lds950, -1, true, -1).refusal != nullptr, "sides whose product wraps");
  const double depths[] = {0.0, 1.0, -0.1, 1.5, __builtin_nan("")};
  for (double d : depths) expect(plan(63, 7, 9, 5, 5, d, 4, lds950, -1, true, -1).refusal != nullptr, "a cycle_depth outside (0, 1)");
  expect(plan(63, 7, 9, 5, 5, 0.3, -1, lds950, -1, true, -1).refusal != nullptr, "max_major -1");
  expect(plan(63, 7, 9, 5, 5, 0.3, kCscleanMaxMajor + 1, lds950, -1, true, -1).refusal != nullptr, "max_major beyond the limit");
  expect(plan(63, 7, 9, 5, 5, 0.3, 4, lds950, -1, true, 2).refusal != nullptr, "minor_route 2");
  expect(plan(63, 7, 9, 5, 5, 0.3, 4, lds950, -1, true, -2).refusal != nullptr, "minor_route -2");
  expect(plan(63, 7, 9, 5, -1, 0.3, 4, lds950, -1, true, -1).refusal != nullptr, "maxiter -1");
  expect(plan(63, 7, 9, 5, kImcleanMaxIter + 1, 0.3, 4, lds950, -1, true, -1).refusal != nullptr, "maxiter beyond the limit");
  expect(plan(0, 0, 0, 5, 5, 0.3, 4, lds950, -1, true, -1).refusal != nullptr, "npix 0");
  expect(plan(63, 7, 9, (int64_t(1) << 20) + 1, 5, 0.3, 4, lds950, -1, true, -1).refusal != nullptr, "nchan beyond the limit");
  expect(plan(63, 7, 9, 5, 5, 0.3, 4, lds950, 2, true, -1).refusal != nullptr, "route 2");
  expect(plan(63, 7, 9, 5, 5, 0.3, 4, lds950, 1, false, -1).refusal != nullptr, "stepped on a non-uniform grid");
  // the LDS of a mosaic pass stages a_k A as well: 20 B a channel of the tile, where the dirty image takes 12
  expect(plan(63, 7, 9, 5, 5, 0.3, 4, kImagingLds + 20 * kImagingTile, -1, true, 1).refusal == nullptr, "the LDS of the pass, exactly");
  const MoscsPlan shy = plan(63, 7, 9, 5, 5, 0.3, 4, kImagingLds + 20 * kImagingTile - 1, -1, true, 1);
  expect(shy.refusal && std::strstr(shy.refusal, "LDS") && shy.total > 0, "the LDS of the pass one byte short", shy.total);
  // the largest sizes: refused for the budget, with a total that did not wrap
  const MoscsPlan huge = moscs_plan(kImcleanMaxPixels, 1 << 14, 1 << 14, int64_t(1) << 30, int64_t(1) << 18, int64_t(1) << 30, false, kImcleanMaxIter, 0.3,
                                    kCscleanMaxMajor, 0, lds950, -1, true, -1);
  expect(huge.refusal && huge.total > (int64_t(1) << 55) && huge.total <= (int64_t(1) << 56), "the largest sizes", huge.total);
  // the figures the documents quote: HERA-350, 1024 channels, 64 x 64 directions, four snapshots, maxiter 100, four major cycles
  const MoscsPlan h = moscs_plan(4096, 64, 64, 61075, 1024, 4, false, 100, 0.3, 4, int64_t(5) << 30, lds950, -1, true, -1);
  expect(!h.refusal && h.cyc.minor_route == kCscleanLds && h.cyc.vres_bytes == 4002611200 && h.scale_bytes == 33554432, "the quoted plan", h.total);
  std::printf("the quoted plan takes %lld B\n", (long long)h.total);
  expect(moscs_plan(4096, 64, 64, 61075, 1024, 4, false, 100, 0.3, 4, 0, lds950, -1, true, -1).refusal != nullptr, "the quoted plan in the default budget");
  std::printf("checked %ld bad %ld\n", checked, bad);
  return bad ? 1 : 0;
}
