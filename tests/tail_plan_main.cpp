// Stand-alone driver of prisim_amd/csrc/tail_plan.h for tests/test_tail_plan.py (built with -fsanitize=address,undefined).
// usage: tail_plan_main <file of int64>
//   the file: (n0, src_per_split, chunk, src_lo, src_hi, ntiles, nbgroups, slots, mode, tuned(0|1)) per case
//   stdout:   one line per case: n ntail per_xcd_slabs, the n + 1 boundaries, then the 8 x per_xcd_slabs (piece, tile) pairs of the table
#include <cstdint>
#include <cstdio>
#include <vector>

#include "tail_plan.h"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  std::vector<int64_t> rows;
  int64_t buf[10];
  while (fread(buf, sizeof(int64_t), 10, f) == 10) rows.insert(rows.end(), buf, buf + 10);
  fclose(f);
  std::vector<int32_t> tab;
  for (size_t i = 0; i + 9 < rows.size(); i += 10) {
    const int64_t* r = &rows[i];
    const prisim::TailPieces t = prisim::tail_pieces((int)r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], (int)r[8], r[9] != 0);
    const int per = prisim::tail_slab_table(t.n, (int)r[5], tab);
    printf("%d %d %d", t.n, t.ntail, per);
    for (int k = 0; k <= t.n; ++k) printf(" %lld", (long long)t.lo[k]);
    for (int32_t v : tab) printf(" %d", (int)v);
    printf("\n");
  }
  return 0;
}
