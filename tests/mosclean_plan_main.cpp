// Stand-alone check of prisim_amd/csrc_addon/mosclean_plan.h (tests/test_mosclean.py builds it with -fsanitize=address,undefined and runs
// it): the fields it takes from imclean_plan.h, the device bytes by buffer against the budget, from one byte short to ample, over the
// grid of tests/imclean_plan_main.cpp times nt in {1, 3, 120}, up to the largest sizes the entry takes.  Prints "checked N bad M" and
// returns 1 when anything is wrong.
#include "mosclean_plan.h"

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

// the bytes of an accepted or a budget-refused plan, by the statement of the header
int64_t bytes_by_hand(int64_t npix, int64_t nchan, int64_t nt, bool avg, int64_t maxiter, int64_t nslabs) {
  const int64_t nc = avg ? 1 : nchan;
  return 64 * nt * npix + 8 * nt * nchan * npix + 16 * nchan * npix + 8 * nc * npix + 16 * nc * npix + npix + 12 * nc * maxiter + 16 * nslabs * nc +
         (36 * nc + 8 * (nt + 1) * nchan + 24);
}

}  // namespace

int main() {
  const int64_t lds950 = 160 * 1024, ample = int64_t(1) << 55;
  const int64_t pixs[] = {1, 63, 257, 1000, int64_t(1) << 20};
  const int64_t chans[] = {1, 32, 33, 1024};
  const int64_t snaps[] = {1, 3, 120};
  const int64_t iters[] = {0, 25, 10000};
  for (int64_t npix : pixs)
    for (int64_t nchan : chans)
      for (int64_t nt : snaps)
        for (int64_t maxiter : iters)
          for (int avg = 0; avg < 2; ++avg) {
            const MoscleanPlan free_plan = mosclean_plan(npix, 300, nchan, nt, avg != 0, maxiter, ample, lds950, -1, true);
            expect(!free_plan.refusal, "an ample budget is refused", npix, nchan, maxiter);
            const int64_t need = free_plan.total;
            expect(need == bytes_by_hand(npix, nchan, nt, avg != 0, maxiter, free_plan.clean.nslabs), "the bytes are not those of the statement", npix,
                   nchan, need);
            const ImcleanPlan ic = imclean_plan(npix, 300, nchan, nt, avg != 0, maxiter, ample, lds950, -1, true);
            const int64_t budgets[] = {need - 1, need, need + 1, 2 * need, 0};
            for (int64_t budget : budgets)
              for (int asked = -1; asked <= 1; ++asked)
                for (int uniform = 0; uniform < 2; ++uniform) {
                  const MoscleanPlan p = mosclean_plan(npix, 300, nchan, nt, avg != 0, maxiter, budget, lds950, asked, uniform != 0);
                  const int64_t have = budget_or_default(budget);
                  if (asked == kImagingStepped && !uniform) {
                    expect(p.refusal && std::strstr(p.refusal, "uniform"), "stepped on a non-uniform grid accepted", npix, nchan);
                    continue;
                  }
                  // the bytes by buffer sum to the total, and the call runs exactly when the total is within the budget
                  const int64_t sum = p.dirs_bytes + p.beam_bytes + p.sums_bytes + p.flat_bytes + p.out_bytes + p.window_bytes + p.list_bytes +
                                      p.partial_bytes + p.state_bytes;
                  expect(sum == p.total && p.total == need, "the buffers do not sum to the total", npix, nchan, p.total);
                  if (need > have) {
                    expect(p.refusal && std::strstr(p.refusal, "whole image"), "an image beyond the budget accepted", npix, nchan, budget);
                    continue;
                  }
                  bool ok = p.refusal == nullptr;
                  // the route and the geometry are imclean_plan's own, field for field
                  const ImcleanPlan& c = p.clean;
                  ok = ok && c.route == (asked >= 0 ? asked : uniform ? kImagingStepped : kImagingDirect);
                  ok = ok && c.reseed == (c.route == kImagingStepped ? kImagingReseed : 1);
                  ok = ok && c.nc == ic.nc && c.tile == ic.tile && c.ntiles == ic.ntiles && c.block == ic.block && c.nblocks == ic.nblocks &&
                       c.slab == ic.slab && c.nslabs == ic.nslabs && c.peak_cx == ic.peak_cx && c.peak_cgroups == ic.peak_cgroups &&
                       p.list_bytes == ic.list_bytes && p.partial_bytes == ic.partial_bytes;
                  ok = ok && p.lds == kImagingLds + 20 * kImagingTile && p.lds <= lds950;
                  ok = ok && p.beam_bytes == 8 * nt * nchan * npix && p.dirs_bytes == 64 * nt * npix && p.sums_bytes == 16 * nchan * npix &&
                       p.flat_bytes == 8 * c.nc * npix;
                  expect(ok, "an unsound plan", npix, nchan, budget);
                }
            // an LDS limit one byte short is refused, the limit itself is not
            expect(mosclean_plan(npix, 300, nchan, nt, avg != 0, maxiter, ample, free_plan.lds - 1, -1, true).refusal != nullptr, "LDS one byte short accepted");
            expect(!mosclean_plan(npix, 300, nchan, nt, avg != 0, maxiter, ample, free_plan.lds, -1, true).refusal, "the LDS limit itself refused");
          }
  // the sizes themselves: imclean_plan's refusals, passed on
  expect(mosclean_plan(0, 10, 10, 1, false, 5, 0, lds950, -1, true).refusal != nullptr, "npix 0");
  expect(mosclean_plan(10, 0, 10, 1, false, 5, 0, lds950, -1, true).refusal != nullptr, "nbl 0");
  expect(mosclean_plan(10, 10, 10, 1, false, -1, 0, lds950, -1, true).refusal != nullptr, "maxiter -1");
  expect(mosclean_plan(10, 10, 10, 1, false, kImcleanMaxIter + 1, 0, lds950, -1, true).refusal != nullptr, "maxiter beyond 2^30");
  expect(mosclean_plan(kImcleanMaxPixels + 1, 10, 1, 1, false, 5, 0, lds950, -1, true).refusal != nullptr, "npix beyond 2^28");
  expect(mosclean_plan(10, 10, 10, 1, false, 5, 0, lds950, 2, true).refusal != nullptr, "route 2");
  expect(mosclean_plan(10, 10, 10, 1, false, 5, 0, lds950, -2, true).refusal != nullptr, "route -2");
  // the largest sizes: refused for the budget, with a total that did not wrap
  const MoscleanPlan big = mosclean_plan(kImcleanMaxPixels, int64_t(1) << 30, int64_t(1) << 18, int64_t(1) << 30, true, kImcleanMaxIter, 0, lds950, -1, true);
  expect(big.refusal && std::strstr(big.refusal, "whole image") && big.total == (int64_t(1) << 56) && big.beam_bytes == (int64_t(1) << 56), "the largest sizes", big.total);
  const MoscleanPlan wide = mosclean_plan(1 << 20, 1, int64_t(1) << 20, 1, false, kImcleanMaxIter, 0, lds950, -1, true);
  expect(wide.refusal && wide.total > (int64_t(1) << 50) && wide.total <= (int64_t(1) << 56), "2^20 channels of 2^30 components", wide.total);
  // the figures the documents quote: 64 x 64 directions of 1024 channels, four snapshots, ten components
  const MoscleanPlan h = mosclean_plan(4096, 61075, 1024, 4, false, 10, 0, lds950, -1, true);
  expect(!h.refusal && h.clean.route == kImagingStepped && h.clean.ntiles == 32 && h.clean.nblocks == 16 && h.lds == 17792 + 256 &&
             h.beam_bytes == 134217728 && h.sums_bytes == 67108864 && h.dirs_bytes == 1048576, "the quoted plan", h.total);
  std::printf("checked %ld bad %ld\n", checked, bad);
  return bad ? 1 : 0;
}
