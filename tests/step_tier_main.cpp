// Stand-alone driver of prisim_amd/csrc/step_bound.h's second tier for tests/test_step_tier.py (built with -fsanitize=address,undefined).
// usage: step_tier_main <file of float64>
//   the file: dmax hmax zmax df f32(0|1), then (maxlen, maxh, maxz) per baseline group
//   stdout:   first line: the wide limit in cycles; then one line per group: the group's largest step phase in cycles (17 significant
//             digits), its flag (step_flag) and its tier (step_tier)
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
  printf("%.17g\n", prisim::step_wide_limit_cycles());
  for (size_t g = 0; g + 2 < grp.size(); g += 3) {
    const double step = prisim::step_bound_cycles(grp[g], grp[g + 1], grp[g + 2], head[0], head[1], head[2], head[3]);
    const bool flag = prisim::step_flag(grp[g], grp[g + 1], grp[g + 2], head[0], head[1], head[2], head[3], f32);
    const int tier = prisim::step_tier(grp[g], grp[g + 1], grp[g + 2], head[0], head[1], head[2], head[3], f32);
    printf("%.17g %d %d\n", step, flag ? 1 : 0, tier);
  }
  return 0;
}
