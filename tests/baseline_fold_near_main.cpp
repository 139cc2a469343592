// Stand-alone driver of fold_baselines_near / choose_fold (prisim_amd/csrc/baseline_fold.h) for tests/test_baseline_fold_near.py
// (built with -fsanitize=address,undefined).
// usage: baseline_fold_near_main <file of nbl x 3 float64> <tol in metres | auto> [f_max in Hz] [allow_near]
//   ->   stdout: "nu nbl n_exact kind", "tol max_dev phase_bound" (%.17g), then the nu entries of rep, then the nbl entries of map
// `auto` is set_array's tolerance (fold_near_tol); kind is choose_fold's answer with 256 rows per group.  With tol = 0 the program
// itself checks that the result is fold_baselines' (exit status 5 otherwise).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "baseline_fold.h"

int main(int argc, char** argv) {
  if (argc < 3 || argc > 5) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  std::vector<double> bl;
  double buf[3];
  while (fread(buf, sizeof(double), 3, f) == 3) bl.insert(bl.end(), buf, buf + 3);
  fclose(f);
  const int64_t nbl = (int64_t)(bl.size() / 3);
  const double tol = strcmp(argv[2], "auto") == 0 ? prisim::fold_near_tol(bl.data(), nbl) : strtod(argv[2], nullptr);
  const double fmax = argc > 3 ? strtod(argv[3], nullptr) : 0.0;
  const bool allow_near = argc > 4 ? atoi(argv[4]) != 0 : true;
  std::vector<int64_t> rep, rep_x;
  std::vector<int32_t> map, map_x;
  double max_dev = -1.0;
  prisim::fold_baselines(bl.data(), nbl, rep_x, map_x);
  prisim::fold_baselines_near(bl.data(), nbl, tol, rep, map, max_dev);
  if ((int64_t)map.size() != nbl) return 4;
  if (tol == 0.0 && (rep != rep_x || map != map_x || max_dev != 0.0)) return 5;
  const double phase = prisim::fold_near_phase_bound(max_dev, fmax);
  const int kind = (int)prisim::choose_fold(nbl, (int64_t)rep_x.size(), (int64_t)rep.size(), phase, 256, allow_near);
  printf("%lld %lld %lld %d\n", (long long)rep.size(), (long long)nbl, (long long)rep_x.size(), kind);
  printf("%.17g %.17g %.17g\n", tol, max_dev, phase);
  for (int64_t r : rep) printf("%lld\n", (long long)r);
  for (int32_t m : map) printf("%d\n", (int)m);
  return 0;
}
