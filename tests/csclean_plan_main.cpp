// Stand-alone check of prisim_amd/csrc_addon/csclean_plan.h (tests/test_csclean.py builds it with -fsanitize=address,undefined and runs
// it): the lattice, the half-plane of the minor-cycle beam, where the working image of a minor cycle lives, and the device bytes by
// buffer against the budget, from one byte short to ample, for every route request.  Prints "checked N bad M" and returns 1 when
// anything is wrong.
#include "csclean_plan.h"

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

// what the cycles add to the bytes of prisim_clean_image, by the statement of the header
int64_t added_by_hand(int64_t ny, int64_t nx, int64_t nbl, int64_t nchan, int64_t nt, bool avg, int64_t max_major, bool global) {
  const int64_t nc = avg ? 1 : nchan, npix = ny * nx, full = (2 * ny - 1) * (2 * nx - 1), half = (full + 1) / 2;
  return 16 * nt * nbl * nchan + 8 * nc * full + (32 * nt * half + 8 * half * nchan + (avg ? 8 * half : 0)) +
         (28 * nc + 4 * nc * max_major + 8 * nc * (max_major + 1)) + (global ? 8 * nc * npix : 0);
}

}  // namespace

int main() {
  const int64_t lds950 = 160 * 1024, nbl = 300, maxiter = 25;
  const int64_t grids[][2] = {{1, 1}, {7, 9}, {9, 7}, {63, 1}, {1, 63}, {25, 40}, {40, 25}, {1000, 1}, {128, 128}, {1024, 1024}, {512, 2048}, {1, 1 << 20}};
  const int64_t chans[] = {1, 33, 1024};
  const int64_t majors[] = {0, 4, 32};
  for (const auto& g : grids)
    for (int64_t nchan : chans)
      for (int64_t max_major : majors)
        for (int avg = 0; avg < 2; ++avg) {
          const int64_t ny = g[0], nx = g[1], npix = ny * nx, nt = npix > 4096 ? 1 : 3, nc = avg ? 1 : nchan;
          const bool fits = npix * 8 + kCscleanMinorStatic <= lds950;
          for (int minor = -1; minor <= 1; ++minor) {
            const bool global = minor == kCscleanGlobal || (minor == kCscleanAuto && !fits);
            const CscleanPlan free_plan = csclean_plan(npix, ny, nx, nbl, nchan, nt, avg != 0, maxiter, 0.3, max_major, int64_t(1) << 60, lds950, -1, true, minor);
            if (minor == kCscleanLds && !fits) {
              expect(free_plan.refusal && std::strstr(free_plan.refusal, "LDS"), "an LDS route that does not fit accepted", ny, nx, nchan);
              continue;
            }
            expect(!free_plan.refusal, "an ample budget is refused", ny, nx, nchan);
            const ImcleanPlan base = imclean_plan(npix, nbl, nchan, nt, avg != 0, maxiter, int64_t(1) << 60, lds950, -1, true);
            const int64_t need = free_plan.total;
            expect(need == base.total + added_by_hand(ny, nx, nbl, nchan, nt, avg != 0, max_major, global), "the bytes are not those of the statement", ny, nx, need);
            expect(need > 0 && need < (int64_t(1) << 56), "the total overflowed", ny, nx, need);
            const int64_t budgets[] = {need - 1, need, need + 1, 2 * need, 0};
            for (int64_t budget : budgets)
              for (int asked = -1; asked <= 1; ++asked)
                for (int uniform = 0; uniform < 2; ++uniform) {
                  const CscleanPlan p = csclean_plan(npix, ny, nx, nbl, nchan, nt, avg != 0, maxiter, 0.3, max_major, budget, lds950, asked, uniform != 0, minor);
                  if (asked == kImagingStepped && !uniform) {
                    expect(p.refusal && std::strstr(p.refusal, "uniform"), "stepped on a non-uniform grid accepted", ny, nx);
                    continue;
                  }
                  const int64_t sum = p.base.total + p.vres_bytes + p.psf_bytes + p.psf_work_bytes + p.cycle_bytes + p.minor_bytes;
                  expect(sum == p.total && p.total == need, "the buffers do not sum to the total", ny, nx, p.total);
                  if (need > budget_or_default(budget)) {
                    expect(p.refusal && std::strstr(p.refusal, "resident buffers"), "a call beyond the budget accepted", ny, nx, budget);
                    continue;
                  }
                  bool ok = p.refusal == nullptr;
                  ok = ok && p.base.route == (asked >= 0 ? asked : uniform ? kImagingStepped : kImagingDirect) && p.base.nc == nc;
                  // AUTO picks LDS exactly when the image fits; an explicit route is itself
                  ok = ok && p.minor_route == (global ? kCscleanGlobal : kCscleanLds);
                  ok = ok && p.minor_lds == (global ? kCscleanMinorStatic : npix * 8 + kCscleanMinorStatic) && p.minor_lds <= lds950;
                  ok = ok && (global ? p.minor_bytes == 8 * nc * npix : p.minor_bytes == 0);
                  // the half-plane: the centre, what follows it in row-major order, and nothing else; the other half mirrors into it
                  ok = ok && p.psf_full == (2 * ny - 1) * (2 * nx - 1) && 2 * p.psf_half - 1 == p.psf_full && p.psf_bytes == 8 * nc * p.psf_full;
                  ok = ok && p.vres_bytes == 16 * nt * nbl * nchan && p.ny == ny && p.nx == nx;
                  expect(ok, "an unsound plan", ny, nx, budget);
                }
          }
        }
  // the arguments themselves
  const int64_t big = int64_t(1) << 60;
  expect(csclean_plan(63, 7, 9, 10, 5, 1, false, 5, 0.3, 4, big, lds950, -1, true, -1).refusal == nullptr, "7 x 9");
  expect(csclean_plan(63, 7, 8, 10, 5, 1, false, 5, 0.3, 4, big, lds950, -1, true, -1).refusal != nullptr, "7 x 8 for 63 pixels");
  expect(csclean_plan(63, 0, 63, 10, 5, 1, false, 5, 0.3, 4, big, lds950, -1, true, -1).refusal != nullptr, "ny 0");
  expect(csclean_plan(63, -7, -9, 10, 5, 1, false, 5, 0.3, 4, big, lds950, -1, true, -1).refusal != nullptr, "negative sides");
  expect(csclean_plan(63, int64_t(1) << 40, int64_t(1) << 40, 10, 5, 1, false, 5, 0.3, 4, big, lds950, -1, true, -1).refusal != nullptr, "sides whose product wraps");
  const double depths[] = {0.0, 1.0, -0.1, 1.5, 0.0 / 1.0 - 1.0, __builtin_nan("")};
  for (double d : depths) expect(csclean_plan(63, 7, 9, 10, 5, 1, false, 5, d, 4, big, lds950, -1, true, -1).refusal != nullptr, "a cycle_depth outside (0, 1)");
  expect(csclean_plan(63, 7, 9, 10, 5, 1, false, 5, 0.999, 4, big, lds950, -1, true, -1).refusal == nullptr, "cycle_depth 0.999");
  expect(csclean_plan(63, 7, 9, 10, 5, 1, false, 5, 0.3, -1, big, lds950, -1, true, -1).refusal != nullptr, "max_major -1");
  expect(csclean_plan(63, 7, 9, 10, 5, 1, false, 5, 0.3, kCscleanMaxMajor + 1, big, lds950, -1, true, -1).refusal != nullptr, "max_major beyond the limit");
  expect(csclean_plan(63, 7, 9, 10, 5, 1, false, 5, 0.3, 4, big, lds950, -1, true, 2).refusal != nullptr, "minor_route 2");
  expect(csclean_plan(63, 7, 9, 10, 5, 1, false, 5, 0.3, 4, big, lds950, -1, true, -2).refusal != nullptr, "minor_route -2");
  expect(csclean_plan(63, 7, 9, 10, 5, 1, false, -1, 0.3, 4, big, lds950, -1, true, -1).refusal != nullptr, "maxiter -1");
  expect(csclean_plan(0, 0, 0, 10, 5, 1, false, 5, 0.3, 4, big, lds950, -1, true, -1).refusal != nullptr, "npix 0");
  expect(csclean_plan(63, 7, 9, 10, 5, 1, false, 5, 0.3, 4, big, kImagingLds + 12 * kImagingTile - 1, -1, true, 1).refusal != nullptr, "the LDS of the dirty image one byte short");
  // 128 x 128 pixels are the most a workgroup of gfx950 holds: 131136 B of its 160 KiB; 144 x 144 do not fit
  const CscleanPlan m = csclean_plan(16384, 128, 128, 10, 5, 1, false, 5, 0.3, 4, big, lds950, -1, true, -1);
  expect(!m.refusal && m.minor_route == kCscleanLds && m.minor_lds == 131136, "128 x 128 in LDS", m.minor_lds);
  expect(csclean_plan(20736, 144, 144, 10, 5, 1, false, 5, 0.3, 4, big, lds950, -1, true, -1).minor_route == kCscleanGlobal, "144 x 144 in LDS");
  // the largest sizes: refused for the budget, with a total that did not wrap
  const CscleanPlan huge = csclean_plan(kImcleanMaxPixels, 1 << 14, 1 << 14, int64_t(1) << 30, int64_t(1) << 18, int64_t(1) << 30, false, kImcleanMaxIter, 0.3,
                                        kCscleanMaxMajor, 0, lds950, -1, true, -1);
  expect(huge.refusal && huge.total > (int64_t(1) << 55) && huge.total <= (int64_t(1) << 56), "the largest sizes", huge.total);
  // the figures the documents quote: HERA-350, 1024 channels, 64 x 64 directions, one snapshot, maxiter 100, four major cycles
  const CscleanPlan h = csclean_plan(4096, 64, 64, 61075, 1024, 1, false, 100, 0.3, 4, int64_t(2) << 30, lds950, -1, true, -1);
  expect(!h.refusal && h.minor_route == kCscleanLds && h.minor_lds == 32832 && h.psf_full == 16129 && h.psf_half == 8065 &&
             h.vres_bytes == 1000652800 && h.psf_bytes == 132128768, "the quoted plan", h.total);
  expect(csclean_plan(4096, 64, 64, 61075, 1024, 1, false, 100, 0.3, 4, 0, lds950, -1, true, -1).refusal != nullptr, "the quoted plan in the default budget");
  std::printf("checked %ld bad %ld\n", checked, bad);
  return bad ? 1 : 0;
}
