// Stand-alone driver of prisim_amd/csrc/baseline_fold.h for tests/test_baseline_fold.py (built with -fsanitize=address,undefined).
// usage: baseline_fold_main <file of nbl x 3 float64>   ->   stdout: "nu nbl", then the nu entries of rep, then the nbl entries of map
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "baseline_fold.h"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  std::vector<double> bl;
  double buf[3];
  while (fread(buf, sizeof(double), 3, f) == 3) bl.insert(bl.end(), buf, buf + 3);
  fclose(f);
  const int64_t nbl = (int64_t)(bl.size() / 3);
  std::vector<int64_t> rep;
  std::vector<int32_t> map;
  prisim::fold_baselines(bl.data(), nbl, rep, map);
  if ((int64_t)map.size() != nbl) return 4;
  printf("%lld %lld\n", (long long)rep.size(), (long long)nbl);
  for (int64_t r : rep) printf("%lld\n", (long long)r);
  for (int32_t m : map) printf("%d\n", (int)m);
  return 0;
}
