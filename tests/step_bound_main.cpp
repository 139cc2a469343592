// Stand-alone driver of prisim_amd/csrc/step_bound.h for tests/test_step_bound.py (built with -fsanitize=address,undefined).
// usage: step_bound_main <file of float64>
//   the file: dmax hmax zmax df f32(0|1), then (maxlen, maxh, maxz) per baseline group
//   stdout:   one line per group: the group's largest step phase in cycles (17 significant digits) and its flag
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "step_bound.h"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  double head[5];
  if (fread(head, sizeof(double), 5, f) != 5) { fclose(f); return 4; }
  std::vector<double> grp;
  double buf[3];
  while (fread(buf, sizeof(double), 3, f) == 3) grp.insert(grp.end(), buf, buf + 3);
  fclose(f);
  const bool f32 = head[4] != 0.0;
  for (size_t g = 0; g + 2 < grp.size(); g += 3) {
    const double step = prisim::step_bound_cycles(grp[g], grp[g + 1], grp[g + 2], head[0], head[1], head[2], head[3]);
    const bool flag = prisim::step_flag(grp[g], grp[g + 1], grp[g + 2], head[0], head[1], head[2], head[3], f32);
    printf("%.17g %d\n", step, flag ? 1 : 0);
  }
  return 0;
}
