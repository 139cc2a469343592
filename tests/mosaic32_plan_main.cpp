// mosaic32_plan_main.cpp -- TEST INFRASTRUCTURE: prisim_amd/csrc_addon/mosaic32_plan.h compiled alone (tests/test_mosaic32.py builds
// this with -fsanitize=address,undefined) over the size grid tests/test_mosaic.py uses for mosaic_plan.h.  The chunks of an accepted
// call are mosaic_plan's for the same sizes and budget, span for span; the three refusals carry their sentences; the constants the plan
// reports are imaging32_plan.h's.  Prints the constants as "name value" lines, then "checked N bad M"; exit status 1 when anything is bad.
#include "mosaic32_plan.h"

#include <cstdint>
#include <cstdio>
#include <cstring>

using namespace pint;

static bool says(const char* refusal, const char* a, const char* b = "") { return refusal && std::strstr(refusal, a) && std::strstr(refusal, b); }

int main() {
  long bad = 0, checked = 0;
  const int64_t lds950 = 160 * 1024;
  const int64_t pixs[] = {1, 63, 65, 1000, int64_t(1) << 20};
  const int64_t chans[] = {1, 5, kImagingReseed, kImagingReseed + 1, 1024};
  const int64_t snaps[] = {1, 3};
  for (int64_t npix : pixs)
    for (int64_t nchan : chans)
      for (int64_t nt : snaps)
        for (int form = 0; form < 3; ++form)
          for (int avg = 0; avg < 2; ++avg) {
            const int64_t per = mosaic_pixel_bytes(nchan, nt, avg != 0), one = kImagingBlock * per;
            const int64_t budgets[] = {0, one, one + 1, 2 * one - 1, 2 * one, 3 * one + 12345, int64_t(1) << 24, int64_t(1) << 30};
            for (int64_t budget : budgets)
              for (int asked = -1; asked <= 1; ++asked)
                for (int uniform = 0; uniform < 2; ++uniform) {
                  const MosaicPlan p = mosaic32_plan(npix, 300, nchan, nt, form, avg != 0, budget, lds950, asked, uniform != 0, 2);
                  // the fp64 plan of the same sizes and budget on a uniform grid
                  const MosaicPlan q = mosaic_plan(npix, 300, nchan, nt, form, avg != 0, budget, lds950, kImagingStepped, true, 2);
                  ++checked;
                  bool ok;
                  if (q.refusal) {                                     // (1 << 24 does not hold one block of 1024 channels)
                    ok = says(p.refusal, "cannot hold one block") && says(q.refusal, "cannot hold one block");
                  } else if (asked == kImagingDirect) {
                    ok = says(p.refusal, "DIRECT", "call prisim_mosaic_image");
                  } else if (!uniform) {
                    ok = says(p.refusal, "uniform", "call prisim_mosaic_image");
                  } else {
                    ok = !p.refusal && p.route == kImagingStepped;
                    ok = ok && p.chunks.size == q.chunks.size && p.chunks.count == q.chunks.count && p.chunks.last == q.chunks.last &&
                         p.chunks.nstreams == q.chunks.nstreams && p.pixel_bytes == q.pixel_bytes && p.pixel_bytes == per &&
                         p.buffer_bytes == q.buffer_bytes;
                    for (int64_t k = 0; ok && k < p.chunks.count; ++k)
                      ok = p.chunks.span(k, npix).first == q.chunks.span(k, npix).first && p.chunks.span(k, npix).count == q.chunks.span(k, npix).count;
                    ok = ok && p.tile == kImagingTile && p.ntiles == q.ntiles && p.block == kImagingBlock && p.nblocks == q.nblocks;
                    // what stats reports of this pass: the LDS and the reseed interval of the fp32 tile pass
                    ok = ok && p.lds == kImaging32Lds && p.reseed == kImaging32Reseed;
                  }
                  if (!ok) {
                    std::printf("plan32(%lld, %lld, %lld, form %d, avg %d, budget %lld, asked %d, uniform %d): %s\n", (long long)npix, (long long)nchan,
                                (long long)nt, form, avg, (long long)budget, asked, uniform, p.refusal ? p.refusal : "-");
                    ++bad;
                  }
                }
            // one byte short of one block, and an LDS limit one byte short, are refused; the fp64 pass alone fitting is not enough
            if (!says(mosaic32_plan(npix, 300, nchan, nt, form, avg != 0, one - 1, lds950, -1, true, 2).refusal, "cannot hold one block")) ++bad;
            if (!says(mosaic32_plan(npix, 300, nchan, nt, form, avg != 0, 0, kImaging32Lds - 1, -1, true, 2).refusal, "LDS")) ++bad;
            if (!says(mosaic32_plan(npix, 300, nchan, nt, form, avg != 0, 0, kImagingLds, 1, true, 2).refusal, "LDS")) ++bad;
            if (mosaic32_plan(npix, 300, nchan, nt, form, avg != 0, 0, kImaging32Lds, -1, true, 2).refusal) ++bad;
            checked += 4;
          }
  // what pixel_plan refuses stays refused, in its sentence
  if (!says(mosaic32_plan(10, 10, 10, 1, 3, false, 0, lds950, -1, true, 2).refusal, "unknown weight form") ||
      !says(mosaic32_plan(10, 10, 10, 1, 0, false, 0, lds950, 2, true, 2).refusal, "unknown route") ||
      !says(mosaic32_plan(0, 10, 10, 1, 0, false, 0, lds950, -1, true, 2).refusal, ">= 1"))
    ++bad;
  // the timed workload of the documents: 64 x 64 directions of 1024 channels, four snapshots, in the default budget
  const MosaicPlan h = mosaic32_plan(4096, 61075, 1024, 4, 0, false, 0, lds950, -1, true, 2);
  if (h.refusal || h.ntiles != 32 || h.nblocks != 16 || h.chunks.count != 1 || h.pixel_bytes != 41216) ++bad;
  // the smallest budget tests/test_gpu_mosaic32.py gives: 1000 pixels in four chunks of one block
  const MosaicPlan s = mosaic32_plan(1000, 37, 33, 3, 2, false, 256 * mosaic_pixel_bytes(33, 3, false), lds950, -1, true, 2);
  if (s.refusal || s.chunks.size != 256 || s.chunks.count != 4 || s.chunks.nstreams != 1) ++bad;
  checked += 3;
  std::printf("reseed %d\nlds %lld\ntile %d\nblock %d\n", kImaging32Reseed, (long long)kImaging32Lds, kImagingTile, kImagingBlock);
  std::printf("reported_reseed %lld\nreported_lds %lld\nreported_tile %lld\nreported_block %lld\n", (long long)h.reseed, (long long)h.lds,
              (long long)h.tile, (long long)h.block);
  std::printf("checked %ld bad %ld\n", checked, bad);
  return bad ? 1 : 0;
}
