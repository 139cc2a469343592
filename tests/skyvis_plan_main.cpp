// Stand-alone driver of prisim_amd/csrc/skyvis_plan.h for tests/test_skyvis_plan.py (built with -fsanitize=address,undefined).
// usage: skyvis_plan_main <file of float64>     one line of numbers per case (72 doubles each, the layout of CASE_FIELDS in the test):
//          base plan (10) | route: family sum_family, its plan (10), layout taper_group cull cull_prec by_run nsets part_f32 alloc_sets
//          may_defer last_taper_group zero_lift_counts nlaunch | nlaunch x launch (14) | split_eligible | batch plan (6)
//        skyvis_plan_main --toggles           the hooks as read_sky_toggles() finds them in the environment, one line
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "skyvis_plan.h"

using namespace prisim;

static void print_plan(const Plan& p) {
  printf("%d %d %d %d %d %lld %lld %d %d %d ", p.kernel, (int)p.f32, p.ct, p.chunk, p.nsplit, (long long)p.src_per_split, (long long)p.nsrc_pad,
         p.ntiles, p.nbgroups, (int)p.pk);
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  if (!strcmp(argv[1], "--toggles")) {
    const SkyToggles t = read_sky_toggles();
    printf("%d %d %d %d %d %d %d %d %d %d %d\n", (int)t.flush_src, t.taper_group, (int)t.taper_split, (int)t.taper_f64_group, (int)t.grad_taper_group,
           (int)t.wave_items, (int)t.fused_grad, (int)t.wave_batch, (int)t.wave_batch_grad, (int)t.wave_batch_single, (int)t.batch_fp32_as_fp64);
    return 0;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  constexpr int kFields = 72;
  std::vector<double> rows;
  double buf[kFields];
  while (fread(buf, sizeof(double), kFields, f) == (size_t)kFields) rows.insert(rows.end(), buf, buf + kFields);
  fclose(f);
  for (size_t i = 0; i + kFields <= rows.size(); i += kFields) {
    const double* c = &rows[i];
    SkyShape s{};
    s.nbl = (int64_t)c[0]; s.nbl_sum = (int64_t)c[1]; s.nchan = (int64_t)c[2]; s.nsrc = (int64_t)c[3];
    s.f0 = c[4]; s.df = c[5];
    s.uniform = c[6] != 0; s.taper = c[7] != 0; s.folded = c[8] != 0;
    s.cu_count = (int)c[9];
    s.tune_ct = (int)c[10]; s.tune_chunk = (int)c[11]; s.tune_nsplit = (int)c[12];
    s.nruns = (int)c[13];
    if (s.nruns < 0 || s.nruns > kMaxRuns + 1) return 4;
    for (int r = 0; r < kMaxRuns + 1; ++r) s.runs[r] = SkyRun{(int64_t)c[14 + 4 * r], (int64_t)c[15 + 4 * r], c[16 + 4 * r], (int)c[17 + 4 * r]};
    s.ngroups = (int64_t)c[50]; s.lmax = c[51];
    s.cull_any[0] = c[52] != 0; s.cull_any[1] = c[53] != 0; s.cull_staged = c[54] != 0; s.have_lift_flags = c[55] != 0;
    SkyToggles t;
    t.flush_src = (int32_t)c[56]; t.taper_group = (int)c[57];
    t.taper_split = c[58] != 0; t.taper_f64_group = c[59] != 0; t.grad_taper_group = c[60] != 0; t.wave_items = c[61] != 0;
    t.fused_grad = c[62] != 0; t.wave_batch = c[63] != 0; t.wave_batch_grad = c[64] != 0; t.wave_batch_single = c[65] != 0;
    t.batch_fp32_as_fp64 = c[66] != 0;
    s.flush_src = flush_sources(t);
    const int precision = (int)c[67], kernel = (int)c[68];
    const bool want_grad = c[69] != 0, split_ready = c[70] != 0;
    const int64_t kc = (int64_t)c[71];
    const Plan base = make_plan(s, t, precision, kernel);
    const SkyRoute rt = route(s, t, base, want_grad, split_ready);
    print_plan(base);
    printf("%d %d ", rt.family, rt.sum_family);
    print_plan(rt.pl);
    printf("%d %d %d %d %d %d %d %d %d %d %d %d ", rt.layout, rt.taper_group, (int)rt.cull, rt.cull_prec, (int)rt.by_run, rt.nsets, (int)rt.part_f32,
           rt.alloc_sets, (int)rt.may_defer, rt.last_taper_group, (int)rt.zero_lift_counts, rt.nlaunch);
    if (rt.nlaunch < 1 || rt.nlaunch > kMaxRunSets) return 5;
    for (int l = 0; l < rt.nlaunch; ++l) {
      const SkyLaunch& q = rt.launch[l];
      printf("%d %lld %lld %lld %d %d %.17g %d %d %d %d %d %d %d ", q.family, (long long)q.src_lo, (long long)q.src_hi, (long long)q.src_per_split,
             q.accumulate, q.out_set, q.kappa0, q.cull_row, q.flags_row, q.taper, q.wave_nbw, q.wave_nsplit, q.nbgroups, (int)q.repack_pairs);
    }
    printf("%d ", (int)split_eligible(s, t, rt.pl, rt.taper_group));
    const BatchPlan b = batch_plan(s, t, precision, kc, want_grad);
    printf("%d %d %d %d %lld %lld\n", (int)b.eligible, b.ct, b.ntiles, b.nbw, (long long)b.npad, (long long)b.nsplit);
  }
  return 0;
}
