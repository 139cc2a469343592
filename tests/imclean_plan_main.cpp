// Stand-alone check of prisim_amd/csrc_addon/imclean_plan.h (tests/test_imclean.py builds it with -fsanitize=address,undefined and runs it):
// the route rule, the launch geometry, the slabs of the peak search, and the device bytes by buffer against the budget, from one byte
// short to ample, up to the largest sizes the entry takes.  Prints "checked N bad M" and returns 1 when anything is wrong.
#include "imclean_plan.h"

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
  return 32 * nt * npix + 8 * npix * nc + (avg ? 8 * npix * nchan : 0) + 12 * nc * maxiter + 16 * nslabs * nc + (36 * nc + 8 * nchan + 24) + npix;
}

}  // namespace

int main() {
  const int64_t lds950 = 160 * 1024;
  const int64_t pixs[] = {1, 63, 257, 1000, int64_t(1) << 20};
  const int64_t chans[] = {1, 32, 33, 1024};
  const int64_t snaps[] = {1, 3};
  const int64_t iters[] = {0, 25, 10000};
  for (int64_t npix : pixs)
    for (int64_t nchan : chans)
      for (int64_t nt : snaps)
        for (int64_t maxiter : iters)
          for (int avg = 0; avg < 2; ++avg) {
            const ImcleanPlan free_plan = imclean_plan(npix, 300, nchan, nt, avg != 0, maxiter, int64_t(1) << 50, lds950, -1, true);
            expect(!free_plan.refusal, "an ample budget is refused", npix, nchan, maxiter);
            const int64_t need = free_plan.total;
            expect(need == bytes_by_hand(npix, nchan, nt, avg != 0, maxiter, free_plan.nslabs), "the bytes are not those of the statement", npix, nchan, need);
            const int64_t budgets[] = {need - 1, need, need + 1, 2 * need, 0};
            for (int64_t budget : budgets)
              for (int asked = -1; asked <= 1; ++asked)
                for (int uniform = 0; uniform < 2; ++uniform) {
                  const ImcleanPlan p = imclean_plan(npix, 300, nchan, nt, avg != 0, maxiter, budget, lds950, asked, uniform != 0);
                  const int64_t have = budget_or_default(budget);
                  if (asked == kImagingStepped && !uniform) {
                    expect(p.refusal && std::strstr(p.refusal, "uniform"), "stepped on a non-uniform grid accepted", npix, nchan);
                    continue;
                  }
                  // the bytes by buffer sum to the total, and the call runs exactly when the total is within the budget
                  const int64_t sum = p.dd_bytes + p.resid_bytes + p.scratch_bytes + p.list_bytes + p.partial_bytes + p.state_bytes + p.window_bytes;
                  expect(sum == p.total && p.total == need, "the buffers do not sum to the total", npix, nchan, p.total);
                  if (need > have) {
                    expect(p.refusal && std::strstr(p.refusal, "whole image"), "an image beyond the budget accepted", npix, nchan, budget);
                    continue;
                  }
                  bool ok = p.refusal == nullptr;
                  // AUTO is STEPPED exactly when the grid is uniform; an explicit route is itself
                  ok = ok && p.route == (asked >= 0 ? asked : uniform ? kImagingStepped : kImagingDirect);
                  ok = ok && p.reseed == (p.route == kImagingStepped ? kImagingReseed : 1);
                  ok = ok && p.nc == (avg ? 1 : nchan) && p.tile == kImagingTile && p.block == kImagingBlock && p.lds == kImagingLds + 12 * kImagingTile &&
                       p.lds <= lds950;
                  ok = ok && p.ntiles * p.tile >= nchan && (p.ntiles - 1) * p.tile < nchan && p.nblocks * p.block >= npix &&
                       (p.nblocks - 1) * p.block < npix && p.nblocks <= kImagingMaxGrid;
                  // the slabs: whole blocks, at most kImcleanMaxSlabs, covering the pixels with none empty
                  ok = ok && p.slab >= p.block && p.slab % p.block == 0 && p.nslabs >= 1 && p.nslabs <= kImcleanMaxSlabs &&
                       p.nslabs * p.slab >= npix && (p.nslabs - 1) * p.slab < npix;
                  // the channel groups of the peak search: a power of two of channels, 32 at most, no wider than needed
                  ok = ok && p.peak_cx >= 1 && p.peak_cx <= 32 && (p.peak_cx & (p.peak_cx - 1)) == 0 && kImagingBlock % p.peak_cx == 0 &&
                       (p.peak_cx == 32 || p.peak_cx >= p.nc) && (p.peak_cx == 1 || p.peak_cx / 2 < p.nc) &&
                       p.peak_cgroups * p.peak_cx >= p.nc && (p.peak_cgroups - 1) * p.peak_cx < p.nc && p.peak_cgroups <= 65535;
                  ok = ok && (avg ? p.scratch_bytes == 8 * npix * nchan : p.scratch_bytes == 0);
                  expect(ok, "an unsound plan", npix, nchan, budget);
                }
            // an LDS limit one byte short is refused, the limit itself is not
            expect(imclean_plan(npix, 300, nchan, nt, avg != 0, maxiter, 0, free_plan.lds - 1, -1, true).refusal != nullptr, "LDS one byte short accepted");
            expect(need > kDefaultBudget || !imclean_plan(npix, 300, nchan, nt, avg != 0, maxiter, 0, free_plan.lds, -1, true).refusal, "the LDS limit itself refused");
          }
  // the sizes themselves
  expect(imclean_plan(0, 10, 10, 1, false, 5, 0, lds950, -1, true).refusal != nullptr, "npix 0");
  expect(imclean_plan(10, 0, 10, 1, false, 5, 0, lds950, -1, true).refusal != nullptr, "nbl 0");
  expect(imclean_plan(10, 10, 10, 1, false, -1, 0, lds950, -1, true).refusal != nullptr, "maxiter -1");
  expect(imclean_plan(10, 10, 10, 1, false, kImcleanMaxIter + 1, 0, lds950, -1, true).refusal != nullptr, "maxiter beyond 2^30");
  expect(imclean_plan(kImcleanMaxPixels + 1, 10, 1, 1, false, 5, 0, lds950, -1, true).refusal != nullptr, "npix beyond 2^28");
  expect(imclean_plan(10, 10, 10, 1, false, 5, 0, lds950, 2, true).refusal != nullptr, "route 2");
  expect(imclean_plan(10, 10, 10, 1, false, 5, 0, lds950, -2, true).refusal != nullptr, "route -2");
  // the largest sizes: refused for the budget, with a total that did not wrap
  const ImcleanPlan big = imclean_plan(kImcleanMaxPixels, int64_t(1) << 30, int64_t(1) << 18, int64_t(1) << 30, true, kImcleanMaxIter, 0, lds950, -1, true);
  expect(big.refusal && big.total > (int64_t(1) << 55) && big.nslabs == kImcleanMaxSlabs && big.nblocks == kImagingMaxGrid, "the largest sizes", big.total);
  const ImcleanPlan wide = imclean_plan(1 << 20, 1, int64_t(1) << 20, 1, false, kImcleanMaxIter, 0, lds950, -1, true);
  expect(wide.refusal && wide.total > (int64_t(1) << 50), "2^20 channels of 2^30 components", wide.total);
  // the batches of the host loop
  expect(imclean_batch(0) == 32 && imclean_batch(-5) == 32 && imclean_batch(1) == 1 && imclean_batch(7) == 7 && imclean_batch(1024) == 1024 &&
             imclean_batch(int64_t(1) << 40) == 1024, "the batches");
  // the figures the documents quote: 64 x 64 directions of 1024 channels, one snapshot, the default maxiter, in the default budget
  const ImcleanPlan h = imclean_plan(4096, 61075, 1024, 1, false, 10000, 0, lds950, -1, true);
  expect(!h.refusal && h.route == kImagingStepped && h.ntiles == 32 && h.nblocks == 16 && h.nslabs == 16 && h.slab == 256 && h.peak_cx == 32 &&
             h.peak_cgroups == 32 && h.lds == 17792 && h.list_bytes == 122880000 && h.resid_bytes == 33554432, "the quoted plan", h.total);
  std::printf("checked %ld bad %ld\n", checked, bad);
  return bad ? 1 : 0;
}
