"""prisim_amd/csrc_addon/addon_plan.h, the planning arithmetic of the add-on entries, compiled on its own by the host compiler and
checked against the loops and formulas that the entries used to write out by hand."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r'''
#include "addon_plan.h"

#include <algorithm>
#include <cstdint>
#include <cstdio>

using namespace pint;

int main() {
  long bad = 0, checked = 0;
  // the power-of-two test as runs.hip, subband.hip, cpdelay.hip and cpft.hip wrote it
  for (int64_t m = 1; m <= 4097; ++m) {
    int logm = 0;
    while ((int64_t(1) << logm) < m) ++logm;
    const bool pow2 = (int64_t(1) << logm) == m;
    bool got_pow2 = !pow2;
    const int got = ceil_log2(m, got_pow2);
    if (got != logm || got_pow2 != pow2) {
      std::printf("ceil_log2(%lld): %d %d, the loop %d %d\n", (long long)m, got, (int)got_pow2, logm, (int)pow2);
      ++bad;
    }
    ++checked;
  }
  // the chunk plan as the entries wrote it, with cpft.hip's guard of the byte count
  const int64_t ns[] = {1, 2, 3, 5, 64, int64_t(1) << 30};
  const int64_t pers[] = {0, 1, 24, int64_t(1) << 20, int64_t(1) << 33};
  const int64_t budgets[] = {0, 1, 47, 48, 49, int64_t(1) << 30, int64_t(1) << 40};
  const int streams[] = {1, 2};
  for (int64_t n : ns)
    for (int64_t per_item : pers)
      for (int64_t budget_bytes : budgets)
        for (int kMaxStreams : streams) {
          const int64_t budget = budget_bytes > 0 ? budget_bytes : int64_t(1) << 30;
          const int64_t tc = std::max<int64_t>(1, std::min<int64_t>(n, budget / (kMaxStreams * std::max<int64_t>(per_item, 1))));
          const int64_t nchunks = (n + tc - 1) / tc, last = n - (nchunks - 1) * tc;
          const int nstreams = (int)std::min<int64_t>(kMaxStreams, nchunks);
          const Chunks c = plan_chunks(n, per_item, budget_bytes, kMaxStreams);
          const bool same = c.size == tc && c.count == nchunks && c.last == last && c.nstreams == nstreams;
          const bool sound = c.size * (c.count - 1) + c.last == n && 1 <= c.last && c.last <= c.size && c.nstreams <= c.count &&
                             1 <= c.nstreams;
          // the same chunks again from their size, as the entries with a grid limit ask for them
          const Chunks d = chunks_of(n, c.size, kMaxStreams);
          const bool again = d.size == c.size && d.count == c.count && d.last == c.last && d.nstreams == c.nstreams;
          if (!same || !sound || !again) {
            std::printf("plan_chunks(%lld, %lld, %lld, %d): {%lld, %lld, %lld, %d}, by hand {%lld, %lld, %lld, %d}\n", (long long)n,
                        (long long)per_item, (long long)budget_bytes, kMaxStreams, (long long)c.size, (long long)c.count,
                        (long long)c.last, c.nstreams, (long long)tc, (long long)nchunks, (long long)last, nstreams);
            ++bad;
          }
          ++checked;
        }
  // a size below the plan's, as a grid limit gives it: five items in chunks of two
  const Chunks e = chunks_of(5, 2, 2);
  if (e.size != 2 || e.count != 3 || e.last != 1 || e.nstreams != 2) ++bad;
  ++checked;
  std::printf("checked %ld bad %ld\n", checked, bad);
  return bad ? 1 : 0;
}
'''


def test_addon_plan_matches_the_handwritten_arithmetic(tmp_path):
    src = tmp_path / 'plan_check.cpp'
    src.write_text(PROGRAM)
    exe = tmp_path / 'plan_check'
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'prisim_amd', 'csrc_addon'), str(src),
                           '-o', str(exe)])
    res = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = res.stdout.decode()
    assert res.returncode == 0, out
    assert out.strip().splitlines()[-1] == 'checked %d bad 0' % (4097 + 6 * 5 * 7 * 2 + 1), out
