// Stand-alone driver of prisim_amd/csrc/split_plan.h for tests/test_split_plan.py (built with -fsanitize=address,undefined).
// usage: split_plan_main <file of int64>
//   the file: (tiles, groups, slots, nsrc, nbl, nchan, f32(0|1), taper(0|1)) per case
//   stdout:   one line per case: the split count
#include <cstdint>
#include <cstdio>
#include <vector>

#include "split_plan.h"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  std::vector<int64_t> rows;
  int64_t buf[8];
  while (fread(buf, sizeof(int64_t), 8, f) == 8) rows.insert(rows.end(), buf, buf + 8);
  fclose(f);
  for (size_t i = 0; i + 7 < rows.size(); i += 8)
    printf("%d\n", prisim::split_count(rows[i], rows[i + 1], rows[i + 2], rows[i + 3], rows[i + 4], rows[i + 5], rows[i + 6] != 0, rows[i + 7] != 0));
  return 0;
}
