// imaging32_plan_main.cpp -- TEST INFRASTRUCTURE: prisim_amd/csrc_addon/imaging32_plan.h compiled alone (tests/test_imaging32.py builds
// this with -fsanitize=address,undefined) over the size grid tests/test_imaging.py uses for imaging_plan.h.  The chunks of an accepted
// call are imaging_plan's for the same sizes and budget; the refusals carry their sentences; the constants are what the plan reports.
// Prints the constants as "name value" lines, then "checked N bad M"; exit status 1 when anything is bad.
#include "imaging32_plan.h"

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
            const int64_t per = imaging_pixel_bytes(nchan, nt, avg != 0), one = kImagingBlock * per;
            const int64_t budgets[] = {0, one, one + 1, 2 * one - 1, 2 * one, 3 * one + 12345, int64_t(1) << 24, int64_t(1) << 30};
            for (int64_t budget : budgets)
              for (int asked = -1; asked <= 1; ++asked)
                for (int uniform = 0; uniform < 2; ++uniform) {
                  const Imaging32Plan p = imaging32_plan(npix, 300, nchan, nt, form, avg != 0, budget, lds950, asked, uniform != 0, 2);
                  ++checked;
                  bool ok;
                  if (asked == kImagingDirect) {
                    ok = says(p.refusal, "DIRECT", "call prisim_dirty_image");
                  } else if (!uniform) {
                    ok = says(p.refusal, "uniform", "call prisim_dirty_image");
                  } else {
                    // the fp64 plan of the same call: its chunks, pixel for pixel
                    const ImagingPlan q = imaging_plan(npix, 300, nchan, nt, form, avg != 0, budget, lds950, asked, true, 2);
                    ok = !p.refusal && !q.refusal && p.route == kImagingStepped && q.route == kImagingStepped;
                    ok = ok && p.chunks.size == q.chunks.size && p.chunks.count == q.chunks.count && p.chunks.last == q.chunks.last &&
                         p.chunks.nstreams == q.chunks.nstreams && p.pixel_bytes == q.pixel_bytes && p.buffer_bytes == q.buffer_bytes;
                    for (int64_t k = 0; ok && k < p.chunks.count; ++k)
                      ok = p.chunks.span(k, npix).first == q.chunks.span(k, npix).first && p.chunks.span(k, npix).count == q.chunks.span(k, npix).count;
                    ok = ok && p.tile == kImagingTile && p.ntiles == q.ntiles && p.block == kImagingBlock && p.nblocks == q.nblocks;
                    // what stats reports of this pass: its own LDS and reseed interval; and the constants beside them
                    ok = ok && p.lds == kImaging32Lds && p.reseed == kImaging32Reseed && p.rows == kImaging32Rows && p.flush == kImaging32Flush &&
                         p.seed == kImaging32Seed;
                  }
                  if (!ok) {
                    std::printf("plan32(%lld, %lld, %lld, form %d, avg %d, budget %lld, asked %d, uniform %d): %s\n", (long long)npix, (long long)nchan,
                                (long long)nt, form, avg, (long long)budget, asked, uniform, p.refusal ? p.refusal : "-");
                    ++bad;
                  }
                }
            // one byte short of one block, and an LDS limit one byte short, are refused; the fp64 pass alone fitting is not enough
            if (!says(imaging32_plan(npix, 300, nchan, nt, form, avg != 0, one - 1, lds950, -1, true, 2).refusal, "cannot hold one block")) ++bad;
            if (!says(imaging32_plan(npix, 300, nchan, nt, form, avg != 0, 0, kImaging32Lds - 1, -1, true, 2).refusal, "LDS")) ++bad;
            if (!says(imaging32_plan(npix, 300, nchan, nt, form, avg != 0, 0, kImagingLds, 1, true, 2).refusal, "LDS")) ++bad;
            if (imaging32_plan(npix, 300, nchan, nt, form, avg != 0, 0, kImaging32Lds, -1, true, 2).refusal) ++bad;
            checked += 4;
          }
  // what pixel_plan refuses stays refused, in its sentence
  if (!says(imaging32_plan(10, 10, 10, 1, 3, false, 0, lds950, -1, true, 2).refusal, "unknown weight form") ||
      !says(imaging32_plan(10, 10, 10, 1, 0, false, 0, lds950, 2, true, 2).refusal, "unknown route") ||
      !says(imaging32_plan(0, 10, 10, 1, 0, false, 0, lds950, -1, true, 2).refusal, ">= 1"))
    ++bad;
  // the constants against each other: whole pairs, a flush at the end of every pass, one seed at the tile's centre, and the LDS that
  // the staged rows take
  if (kImaging32Rows % kImaging32Pair || kImaging32Flush != kImaging32Rows || 2 * kImaging32Seed != kImagingTile ||
      kImaging32Lds != int64_t(kImaging32Rows / 2) * kImagingTile * 16 + kImaging32Rows * 24 || kImaging32Lds != 17920 || kImaging32Lds > 64 * 1024)
    ++bad;
  // the timed workload of the documents: 64 x 64 directions of 1024 channels, one snapshot, in the default budget
  const Imaging32Plan h = imaging32_plan(4096, 61075, 1024, 1, 0, false, 0, lds950, -1, true, 2);
  if (h.refusal || h.ntiles != 32 || h.nblocks != 16 || h.chunks.count != 1) ++bad;
  checked += 3;
  std::printf("rows %d\nflush %d\nseed %d\nreseed %d\nlds %lld\ntile %d\nblock %d\n", kImaging32Rows, kImaging32Flush, kImaging32Seed, kImaging32Reseed,
              (long long)kImaging32Lds, kImagingTile, kImagingBlock);
  std::printf("checked %ld bad %ld\n", checked, bad);
  return bad ? 1 : 0;
}
