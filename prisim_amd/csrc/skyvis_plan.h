// skyvis_plan.h -- which kernels one sky-sum runs, on which tiling, and in which launches (host only, no HIP: it compiles alone).
//
// compute() (capi.cpp) and the batched catalogue chunk (catalog.cpp) describe the array and the sky in a SkyShape, read the A/B and
// test hooks once into a SkyToggles, and follow what comes back: make_plan() chooses tile, chunk and source split, route() the kernel
// family, the row layout, the partial-cube sets and the ordered launches, batch_plan() the one launch of a chunk of snapshots.  Nothing
// in here touches the device; tests/test_skyvis_plan.py holds every field to a restatement of the rules and to the launchers' own
// preconditions.  DESIGN.md ("Kernel families of the sky-sum") says in a sentence each which shapes reach which family.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>

#include "../../include/prisim_hip.h"
#include "split_plan.h"

namespace prisim {

constexpr int kPlanBlock = 256;      // rows of a baseline group (= kBlockThreads of skyvis_kernels.h: four wavefronts, lanes = baselines)
constexpr int kMaxRuns = 8;          // runs of one source size a sky is described by; a sky of more has sizes that "vary source by source"
constexpr int kMaxRunSets = 8;       // runs of one source size a split sky may have and still be summed run by run (partial-cube sets)
constexpr double kPlanC = 299792458.0;

inline int64_t round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }

struct SkyRun { int64_t lo, hi; double kappa; int tab_row; };      // sources [lo, hi) of one size; tab_row: this run's row of the cull table

// Everything the decisions read from the context, and nothing else.
struct SkyShape {
  int64_t nbl;             // cube rows
  int64_t nbl_sum;         // rows the sky-sum computes (the distinct vectors of a folded array)
  int64_t nchan, nsrc;
  double f0, df;
  bool uniform, taper, folded;
  int cu_count;
  int tune_ct, tune_chunk, tune_nsplit;      // set_tuning (0: the planner's choice)
  int nruns;               // 0: sizes vary source by source
  SkyRun runs[kMaxRuns + 1];      // (one more than a sky is ever described by: the rules for more than kMaxRunSets runs stay testable)
  int64_t ngroups;         // entries of the baseline-group tables
  double lmax;             // their largest baseline length
  bool cull_any[2];        // [precision] anything culled at all
  bool cull_staged;        // the cull tables of this sky are on the device
  bool have_lift_flags;
  int32_t flush_src;
};

// The A/B and test hooks of a compute.  -1: not set.
struct SkyToggles {
  int32_t flush_src = 0;           // PRISIM_HIP_FLUSH_SRC (test hook: the read-modify-write flush on small skies); 0: the default
  int taper_group = -1;            // PRISIM_HIP_TAPER_GROUP: forces the grouped packed fp32 taper recurrence on (1) or off (0)
  bool taper_split = true;         // PRISIM_HIP_TAPER_SPLIT=0: no split form of the packed fp32 taper
  bool taper_f64_group = true;     // PRISIM_HIP_TAPER_F64_GROUP=0: fp64 taper requests run the exact second-order kernel, not the grouped one
  bool grad_taper_group = true;    // PRISIM_HIP_GRAD_TAPER_GROUP=0: fp64 gradients of a tapered sky run the exact form on 16-channel tiles
  bool wave_items = true;          // PRISIM_HIP_WAVE_ITEMS=0: block items
  bool fused_grad = true;          // PRISIM_HIP_FUSED_GRAD=0: the four-pass gradient
  bool wave_batch = true;          // PRISIM_HIP_WAVE_BATCH=0: the per-snapshot loop
  bool wave_batch_grad = true;     // PRISIM_HIP_WAVE_BATCH_GRAD=0: gradients take the per-snapshot loop
  bool wave_batch_single = true;   // PRISIM_HIP_WAVE_BATCH_SINGLE=0: one snapshot per call takes the per-snapshot chain
  bool batch_fp32_as_fp64 = true;  // PRISIM_HIP_BATCH_FP32_AS_FP64=0: fp32 requests keep the per-snapshot fp32 chain
};

// The one place the hooks above are read.  Called per compute() and per catalogue chunk: the tests flip them inside one process.
inline SkyToggles read_sky_toggles() {
  SkyToggles t;
  auto off = [](const char* name) { const char* env = getenv(name); return env && atoi(env) == 0; };
  if (const char* env = getenv("PRISIM_HIP_FLUSH_SRC")) {
    const long v = atol(env);
    if (v > 0 && v < (1L << 30)) t.flush_src = (int32_t)v;
  }
  if (const char* env = getenv("PRISIM_HIP_TAPER_GROUP")) t.taper_group = atoi(env) != 0 ? 1 : 0;
  t.taper_split = !off("PRISIM_HIP_TAPER_SPLIT");
  t.taper_f64_group = !off("PRISIM_HIP_TAPER_F64_GROUP");
  t.grad_taper_group = !off("PRISIM_HIP_GRAD_TAPER_GROUP");
  t.wave_items = !off("PRISIM_HIP_WAVE_ITEMS");
  t.fused_grad = !off("PRISIM_HIP_FUSED_GRAD");
  t.wave_batch = !off("PRISIM_HIP_WAVE_BATCH");
  t.wave_batch_grad = !off("PRISIM_HIP_WAVE_BATCH_GRAD");
  t.wave_batch_single = !off("PRISIM_HIP_WAVE_BATCH_SINGLE");
  t.batch_fp32_as_fp64 = !off("PRISIM_HIP_BATCH_FP32_AS_FP64");
  return t;
}

// fp32 accumulators are flushed into the fp64 cube every flush_src sources: the rounding error of a sequential
// fp32 sum grows like eps/2*sqrt(n/3) relative to sum|pbflux| in the fully coherent worst case (1.1e-6 at n = 16384,
// tolerance 5e-6), and every flush is a read-modify-write pass over the whole cube, so flush as rarely as that allows.
constexpr int32_t kFlushSrc = 16384;
inline int32_t flush_sources(const SkyToggles& t) { return t.flush_src > 0 ? t.flush_src : kFlushSrc; }

// The grouped taper recurrences (skyvis_kernels.hip) hold on fine channel grids only: second-order residual
// (11.09 (df/f)^2)^2 * 0.565 <= 1e-8 of sum|pbflux| when |df| <= 3.4e-3 f_min.
inline bool fine_channel_grid(const SkyShape& s) {
  const double fmin = std::min(std::fabs(s.f0), std::fabs(s.f0 + s.df * (double)(s.nchan - 1)));
  return fmin > 0.0 && std::fabs(s.df) <= 3.4e-3 * fmin;
}

// packed fp32 taper: 1 = grouped recurrence, 0 = exact per-step form
inline int taper_group(const SkyShape& s, const SkyToggles& t) {
  if (t.taper_group >= 0) return (t.taper_group != 0 && s.taper) ? 1 : 0;
  return (s.taper && fine_channel_grid(s)) ? 1 : 0;
}

struct Plan {
  int kernel;      // PRISIM_KERNEL_*
  bool f32;
  int ct;
  int chunk;
  int nsplit;
  int64_t src_per_split;
  int64_t nsrc_pad;
  int ntiles;
  int nbgroups;
  bool pk;         // packed-fp32 kernel (k_skyvis_rec_f32pk) with interleaved pbflux pairs
};

// wave items (arrays of at most 256 baselines, grouped fp64 taper kernel): sources per split when nsrc sources are cut into s_want pieces
inline int64_t wave_split_sources(int64_t nsrc, int64_t s_want) {
  return round_up((std::max<int64_t>(nsrc, 1) + s_want - 1) / std::max<int64_t>(s_want, 1), 4);
}

inline Plan make_plan(const SkyShape& s, const SkyToggles& t, int precision, int kernel) {
  Plan pl{};
  pl.f32 = (precision == PRISIM_FP32);
  pl.kernel = kernel;
  if (kernel == PRISIM_KERNEL_AUTO) pl.kernel = s.uniform ? PRISIM_KERNEL_RECURRENCE : PRISIM_KERNEL_DIRECT;
  const int64_t nbl = s.nbl_sum, nchan = s.nchan, nsrc = s.nsrc;      // (the rows the sky-sum computes: baseline folding)
  pl.nbgroups = (int)((nbl + kPlanBlock - 1) / kPlanBlock);
  // channel tile: the cheapest tile (seed + 5 instructions per term, tiles past nchan are wasted work) that still yields enough
  // blocks to fill 256 CUs x 4 blocks
  // (fp64 48-channel tiles were tried: 5.98 instead of 6.47 instructions per term, but 22 tiles x 239 groups = 10.3 rounds of resident
  // blocks end in a 7 % tail against 14.9 rounds at 32 channels -- measured 128 ms against 125 ms on the same box)
  int max_ct = pl.f32 ? 64 : 32;
  // coarse channel grids with the taper run the exact per-step amplitude recurrence (the grouped form needs a fine_channel_grid):
  // its rounding grows with the chain length (5.8e-6 of one term at 32 steps and df/f = 3 %, tools/fuzz_parity.py),
  // so such runs use 32-channel tiles (16 steps from the seed)
  if (pl.f32 && s.taper && !fine_channel_grid(s)) max_ct = 32;
  int ct = s.tune_ct;
  if (ct == 0) {
    const int64_t want_blocks = 1024;
    const int64_t max_split = std::max<int64_t>(1, nsrc / 64);
    const double seed = pl.f32 ? 30.0 : 48.0;             // instructions per (source, baseline, tile) outside the pair loop (ISA census)
    const double per_term = pl.f32 ? 2.5 : 5.0;
    double best = 0.0;
    ct = 8;
    // Small problems (config 2: 171 baselines = 3 wavefronts) cannot fill the chip whatever the tiling; what matters then is that
    // every SIMD has work and that the seed is amortised over as many channels as the wave count allows.  Measured on config 2
    // (tools/small_problem_census.py, profiles/r03_small_problem_census.jsonl): fp64 16-channel tiles 75.6 us against 85.8 at 8 and
    // 81.0 at 32 (fp64 wants ~2 waves per SIMD to cover its dependent-issue latency), packed fp32 32-channel tiles 39.8 us against 54.2
    // at 8 (a single wave issues v_pk_fma_f32 at near the full rate, the 2-cycle v_fma_f32 of the narrow tiles does not).  So a wider
    // tile is admitted as soon as it still yields 1024 (fp64) / 512 (fp32) active wavefronts, even if that is fewer than 1024 blocks.
    const int64_t active_waves_per_tile = (int64_t)(pl.nbgroups - 1) * (kPlanBlock / 64) +
                                          std::min<int64_t>(kPlanBlock / 64, (nbl - (int64_t)(pl.nbgroups - 1) * kPlanBlock + 63) / 64);
    const int64_t want_waves = pl.f32 ? 512 : 1024;
    for (int cand : {64, 32, 16, 8}) {
      if (cand > max_ct) continue;
      const int64_t tiles = (nchan + cand - 1) / cand;
      if (cand > 8 && tiles * pl.nbgroups * max_split < want_blocks && tiles * active_waves_per_tile * max_split < want_waves) continue;
      const double cost = (double)tiles * (seed + per_term * cand);
      if (best == 0.0 || cost < best * (1.0 - 1e-9)) { best = cost; ct = cand; }
    }
  }
  if (ct > max_ct) ct = max_ct;          // a tuning request never overrides the accuracy cap (or the register budget) above
  pl.ct = ct;
  pl.pk = pl.f32 && (ct == 32 || ct == 64) && pl.kernel == PRISIM_KERNEL_RECURRENCE;
  pl.ntiles = (int)((nchan + ct - 1) / ct);
  // source chunk: granularity of the zero padding and of the source split (the kernels stream rows through scalar loads)
  const int esz = pl.f32 ? 4 : 8;
  int chunk = s.tune_chunk ? s.tune_chunk : 64;
  const int max_chunk = 16384 / (ct * esz);
  if (chunk > max_chunk) chunk = max_chunk;
  if (chunk > 256) chunk = 256;
  if (chunk < 1) chunk = 1;
  pl.chunk = chunk;
  pl.nsrc_pad = round_up(std::max<int64_t>(nsrc, 1), chunk);
  // source split so that small problems still fill the GPU; each split is a multiple of the chunk
  int nsplit = s.tune_nsplit;
  if (nsplit == 0) {
    // resident blocks per CU = waves per SIMD the kernels are built for (PK_WAVES / WavesPerEU in skyvis_kernels.hip)
    // (fp64: the 16 KiB phasor table + 36 KiB flush buffer + prefetch area = 56 KiB of LDS per block allow 2 blocks per CU)
    const int per_cu = pl.pk ? 2 : (pl.f32 ? 4 : 2);
    const int64_t slots = (int64_t)std::max(s.cu_count, 1) * per_cu;
    // the grid runs in rounds of `slots` resident blocks: split_plan.h holds the rule and what it was measured on
    nsplit = split_count(pl.ntiles, pl.nbgroups, slots, nsrc, nbl, nchan, pl.f32, s.taper);
  }
  if (!pl.f32 && s.taper && (ct == 16 || ct == 32) && pl.kernel == PRISIM_KERNEL_RECURRENCE && nbl <= kPlanBlock && !s.tune_chunk &&
      t.taper_f64_group) {
    // One baseline group, fp64 with the taper: wave items (route) -- two wavefronts on every SIMD, and at least 16 sources per
    // item.  Config 2 (3 baseline waves x 16 tiles): 42 splits of 36 sources = 2016 wavefronts in 512 blocks.  A requested split
    // count (set_tuning) is cut by the same rule: a single launch then partitions a sky exactly as a batched launch
    // (prisim_hip_observe_catalog) with that split count does.
    const int64_t nbw = (nbl + 63) / 64;
    int64_t s_want;
    if (s.tune_nsplit) {
      s_want = s.tune_nsplit;
    } else {
      const int64_t waves = 2LL * 4 * std::max(s.cu_count, 1);
      s_want = std::max<int64_t>(1, waves / (pl.ntiles * nbw));
      s_want = std::min<int64_t>(s_want, std::max<int64_t>(1, nsrc / 16));
    }
    if (s_want > 1) {
      const int64_t per = wave_split_sources(nsrc, s_want);
      pl.chunk = 4;
      pl.nsrc_pad = round_up(std::max<int64_t>(nsrc, 1), 16);
      pl.src_per_split = per;
      pl.nsplit = (int)std::max<int64_t>(1, (nsrc + per - 1) / per);
      return pl;
    }
  }
  if (!s.tune_chunk && (!pl.f32 || s.tune_nsplit)) {
    // (fp64; the packed fp32 kernel's time barely moves with the split count -- 40.3 us at 47 splits against 42.2 at 24 on config 2 -- and
    // every split costs its share of k_reduce_partials: 65.7 us per snapshot against 61.7, r04_cfg2_probe_f32.jsonl.)
    // A small sky cut into many pieces (config 2: 1504 sources, 32 splits fill the 512 block slots exactly): 64-source chunks would cap
    // the split count at nsrc / 64 = 24 -- 62 us against 76 with 16-source chunks and 32 splits (tools/config2_fullwave_probe.py)
    auto realised = [&](int c) {          // split count a chunk size allows: whole chunks per split
      const int64_t nch = round_up(std::max<int64_t>(nsrc, 1), c) / c;
      const int64_t per = (nch + nsplit - 1) / std::max(nsplit, 1);
      return (nch + per - 1) / std::max<int64_t>(per, 1);
    };
    while (chunk > 16 && realised(chunk) < nsplit) chunk /= 2;
    pl.chunk = chunk;
    pl.nsrc_pad = round_up(std::max<int64_t>(nsrc, 1), chunk);
  }
  const int64_t nchunks = pl.nsrc_pad / chunk;
  if (nsplit > nchunks) nsplit = (int)nchunks;
  if (nsplit < 1) nsplit = 1;
  const int64_t chunks_per_split = (nchunks + nsplit - 1) / nsplit;
  pl.src_per_split = chunks_per_split * chunk;
  pl.nsplit = (int)((nchunks + chunks_per_split - 1) / chunks_per_split);
  return pl;
}

// ---- the route of one sky-sum -------------------------------------------------------------------------------------------------------

enum SkyFamily {
  kFamDirect = 0,          // k_skyvis_direct
  kFamRec,                 // k_skyvis_rec<T, CT, TAPER>: the plain recurrence, the exact taper, the narrow fp32 tiles
  kFamPackedF32,           // k_skyvis_rec_f32pk
  kFamPackedF32Split,      // k_skyvis_rec_f32pk_split, run by run (point-source runs: the plain packed bodies)
  kFamTaperF64Block,       // k_skyvis_taper_f64 in block items
  kFamTaperF64Wave,        // k_skyvis_taper_f64_wave
  kFamGradF32,             // k_skyvis_grad_f32pk
  kFamGradF64,             // k_skyvis_grad_f64<32, false>
  kFamGradF64TaperGroup,   // k_skyvis_grad_taper_f64 (32-channel tiles)
  kFamGradF64TaperExact,   // k_skyvis_grad_f64<16, true>
  kFamGradFourPass,        // visibilities, then three component passes through the families above
  kFamCount
};

enum RowLayout { kRowsPairs = 0, kRowsNatural, kRowsGrad };      // (up, down) pairs; natural channel order; pre-multiplied by (1, l, m, n)

struct SkyLaunch {
  int family;              // the kernel of this launch (never kFamGradFourPass)
  int64_t src_lo, src_hi, src_per_split;
  int accumulate;          // 1: adds to what an earlier launch wrote into the same set
  int out_set;             // which set of nsplit partial cubes (0: the only one, or the destination itself)
  double kappa0;           // split form: the run's source size
  int cull_row;            // tab_row of the cull table this launch skips its leading sources by, or -1
  int flags_row;           // row of the split flags, or -1
  int taper;
  int wave_nbw, wave_nsplit, nbgroups;      // wave items (then the launch runs with nsplit = 1), or zeros: the plan's own
  bool repack_pairs;       // the run's rows are packed again as (up, down) pairs first
};

struct SkyRoute {
  int family;              // what the sky-sum is; kFamGradFourPass where the gradient takes three more passes
  int sum_family;          // the family of the visibility pass itself (= family but for kFamGradFourPass)
  Plan pl;                 // final tile, chunk, split, padding (the fused gradient's own applied)
  int layout;              // RowLayout
  int taper_group;
  bool cull;
  int cull_prec;           // precision row of the cull tables
  bool by_run;
  int nsets;               // sets of nsplit partial cubes the launches write
  bool part_f32;           // the partial cubes are complex64
  int alloc_sets;          // sets to allocate: >= nsets whatever the split form's preparation reports
  bool may_defer;          // reduce / expand may run on the post stream under the next snapshot
  int last_taper_group;    // prisim_timing mirrors
  bool zero_lift_counts;
  int nlaunch;
  SkyLaunch launch[kMaxRunSets];
};

// Whether this packed fp32 taper pass may run in the split form.  Needs: the packed
// 64-channel kernel, the grouped recurrence's channel-grid condition, sources in <= 8 runs of one size each (exactly one when the
// sources are split into partial cubes), in-loop exponents kappa (|b| f / c)^2 <= 30 with a per-step exponent <= 1/8 (fp32 range and
// the series of exp2m1_small).  (The per-group bound on the parabola the uncorrected grouped form leaves is formed on the device:
// capi.cpp, split_flags_prepare.)
inline bool split_eligible(const SkyShape& s, const SkyToggles& t, const Plan& pl, int tgroup) {
  if (!(pl.pk && s.taper && pl.ct == 64 && tgroup && s.nruns > 0)) return false;
  // (with a source split every run of the sky writes its own set of partial cubes)
  if (s.nruns > kMaxRunSets) return false;
  if (!t.taper_split) return false;
  const double fmax = std::max(std::fabs(s.f0), std::fabs(s.f0 + s.df * (double)(s.nchan - 1)));
  const double fmin = std::min(std::fabs(s.f0), std::fabs(s.f0 + s.df * (double)(s.nchan - 1)));
  double kmax = 0.0;
  bool any_taper = false;
  for (int r = 0; r < s.nruns; ++r) { kmax = std::max(kmax, s.runs[r].kappa); any_taper = any_taper || s.runs[r].kappa > 0.0; }
  if (!any_taper) return false;
  const double umax = kmax * (s.lmax * fmax / kPlanC) * (s.lmax * fmax / kPlanC);
  if (!(umax <= 30.0) || !(2.0 * umax * std::fabs(s.df) <= 0.125 * fmin)) return false;
  return (int64_t)pl.nbgroups == s.ngroups && s.have_lift_flags;
}

// base: make_plan's.  split_ready: the split form's device flags are prepared (false: a pass that cannot take the split form -- a
// gradient component -- or a preparation that failed; the packed kernel then runs unsplit).  Everything but the launches, by_run,
// nsets and part_f32 is the same either way, so compute() may size its buffers before the flags exist.
inline SkyRoute route(const SkyShape& s, const SkyToggles& t, const Plan& base, bool want_grad, bool split_ready) {
  SkyRoute rt{};
  Plan& pl = rt.pl;
  pl = base;
  rt.nsets = rt.alloc_sets = 1;
  rt.nlaunch = 1;
  rt.taper_group = taper_group(s, t);
  SkyLaunch whole{};
  whole.src_lo = 0; whole.src_hi = s.nsrc; whole.cull_row = whole.flags_row = -1; whole.taper = s.taper ? 1 : 0;
  if (pl.kernel == PRISIM_KERNEL_DIRECT) {
    rt.family = rt.sum_family = whole.family = kFamDirect;
    whole.src_per_split = pl.src_per_split;
    rt.launch[0] = whole;
    if (want_grad) rt.family = kFamGradFourPass;
    return rt;
  }
  // Visibility + baseline gradient on a uniform channel grid: ONE fused pass -- fp64: the MFMA kernel k_skyvis_grad_f64 (2.4 x a plain
  // fp64 pass instead of 4 x); fp32: the GRAD bodies of the packed kernel on 16-channel tiles (13 packed instructions per pair of terms
  // against 4 passes x 5).  PRISIM_HIP_FUSED_GRAD=0: the four-pass form (the A/B baseline; non-uniform grids use the direct kernel).
  if (want_grad && t.fused_grad) {
    // fp32: 4 x 2 x 16 packed accumulators = 128 VGPRs; fp64: the taper's per-lane recurrence state does not fit beside 128 at 32
    // fp64 with the taper: the grouped single-chain kernel on 32-channel tiles (k_skyvis_grad_taper_f64); PRISIM_HIP_GRAD_TAPER_GROUP=0 =
    // round 3's exact form on 16-channel tiles (the A/B baseline)
    pl.ct = pl.f32 ? 16 : ((s.taper && !t.grad_taper_group) ? 16 : 32);
    pl.pk = pl.f32;
    pl.ntiles = (int)((s.nchan + pl.ct - 1) / pl.ct);
    pl.nsplit = 1;
    pl.nsrc_pad = round_up(pl.nsrc_pad, 4);       // the fp64 kernel walks the sources four at a time (zero rows past nsrc)
    pl.src_per_split = pl.nsrc_pad;
    whole.src_per_split = pl.nsrc_pad;
    if (pl.f32) {
      whole.family = kFamGradF32;
      rt.layout = s.taper ? kRowsPairs : kRowsGrad;
    } else {
      // (the grouped fp64 taper kernel takes its rows in natural channel order, everything else (up, down) pairs)
      whole.family = !s.taper ? kFamGradF64 : (pl.ct == 32 ? kFamGradF64TaperGroup : kFamGradF64TaperExact);
      rt.layout = whole.family == kFamGradF64TaperGroup ? kRowsNatural : kRowsPairs;
      whole.nbgroups = (int)((s.nbl_sum + 63) / 64);      // the MFMA kernel's blocks own 64 baselines; lift flags stay per 256 (it reads [group >> 2])
    }
    rt.family = rt.sum_family = whole.family;
    rt.launch[0] = whole;
    rt.last_taper_group = (pl.pk && rt.taper_group) ? 1 : 0;
    rt.zero_lift_counts = s.taper && pl.pk;
    return rt;
  }
  rt.last_taper_group = (pl.pk && rt.taper_group) ? 1 : 0;
  // the packed taper kernel folds the amplitude into the phasor (a scaled rotation: no lifting there, the flags only select its
  // re-anchored body); every other kernel lifts the flagged groups
  rt.zero_lift_counts = s.taper && pl.pk;
  rt.may_defer = pl.nsplit > 1;
  // (a sky of several runs of one source size may write one set of partial cubes per run; this bound over-allocates for the forms that
  // turn out not to go run by run -- the unsplit packed form, the exact fp64 taper)
  rt.alloc_sets = (s.taper && s.nruns > 1 && s.nruns <= kMaxRunSets) ? s.nruns : 1;
  // fp64 with the source-shape taper (the reference's default precision on every run_prisim.py sky): the grouped kernel
  // k_skyvis_taper_f64 on 16- / 32-channel tiles, rows in natural channel order (PRISIM_HIP_TAPER_F64_GROUP=0: the exact second-order
  // form, k_skyvis_rec<double, CT, true> -- the A/B baseline and the 8-channel tiles' kernel)
  const bool g64 = !pl.f32 && s.taper && (pl.ct == 16 || pl.ct == 32) && t.taper_f64_group;
  rt.layout = g64 ? kRowsNatural : kRowsPairs;
  // Packed fp32 taper on a sky whose sources come in a few runs of one size each (every HEALPix sky; point sources + diffuse): the
  // split form, run by run (skyvis_kernels.hip: TGROUP 2 / 3) -- size-0 runs take the plain (no-taper) bodies.
  const bool split = split_ready && split_eligible(s, t, pl, rt.taper_group);
  // Run by run under a SOURCE SPLIT (baseline shards of a mixed sky: point sources + a diffuse map): every run is cut into nsplit pieces
  // of its own and writes its own set of nsplit partial cubes; k_reduce_partials then sums nruns x nsplit of them, in fixed order.
  // (Before, a split sky of several runs fell back to ONE launch of the unsplit-form kernels over the whole sky: 510 ms against
  // 453 ideal for one rank's half of config 3 + diffuse, profiles/r04_shard_balance.json.)
  rt.by_run = (split || g64) && s.nruns > 1 && s.nruns <= kMaxRunSets;
  rt.nsets = (pl.nsplit > 1 && rt.by_run) ? s.nruns : 1;
  auto run_per_split = [&](const SkyRun& run) { return round_up(((run.hi - run.lo) + pl.nsplit - 1) / pl.nsplit, pl.chunk); };
  int64_t max_per = pl.src_per_split;
  if (rt.nsets > 1) {
    max_per = 0;
    for (int r = 0; r < s.nruns; ++r) max_per = std::max(max_per, run_per_split(s.runs[r]));
  }
  // fp32 kernels whose splits each flush exactly once store their partial sums as complex64: half the partial traffic
  rt.part_f32 = pl.nsplit > 1 && pl.f32 && max_per <= (int64_t)s.flush_src;
  // taper culling: per baseline group the first source it still has to sum (tables staged by set_sky_*); a launch over the whole sky
  // can only skip the leading sources of the FIRST run
  rt.cull_prec = pl.f32 ? 1 : 0;
  rt.cull = (pl.pk || g64) && s.taper && s.cull_any[rt.cull_prec] && s.cull_staged && s.nruns > 0 &&
            (int64_t)pl.nbgroups == s.ngroups;             // (the packed fp32 kernels and the grouped fp64 kernel)
  // Wave items (k_skyvis_taper_f64_wave): the grouped fp64 taper kernel on an array of one baseline group whose sources are split --
  // the unit of work is a wavefront (baseline wave, split), four per block.  PRISIM_HIP_WAVE_ITEMS=0: block items (the A/B baseline).
  const bool wave = g64 && pl.kernel == PRISIM_KERNEL_RECURRENCE && pl.nsplit > 1 && s.nbl <= kPlanBlock && t.wave_items;
  auto taper_f64 = [&](SkyLaunch& q) {
    q.family = wave ? kFamTaperF64Wave : kFamTaperF64Block;
    if (wave) {
      q.wave_nbw = (int)((s.nbl + 63) / 64);
      q.wave_nsplit = pl.nsplit;
      q.nbgroups = (q.wave_nbw * pl.nsplit + kPlanBlock / 64 - 1) / (kPlanBlock / 64);
    }
  };
  whole.src_per_split = pl.src_per_split;
  if (rt.cull && !split) whole.cull_row = s.runs[0].tab_row;
  if (split || (g64 && rt.by_run)) {
    // run by run when the sky comes in runs of one source size (so that every run's leading sources can be culled); with a source
    // split each run writes its own set of partial cubes, without one a later run adds to what the first wrote
    rt.nlaunch = s.nruns;
    for (int r = 0; r < s.nruns; ++r) {
      const SkyRun& run = s.runs[r];
      SkyLaunch q = whole;
      q.src_lo = run.lo; q.src_hi = run.hi;
      if (pl.nsplit == 1) q.src_per_split = round_up(run.hi - run.lo, pl.chunk);
      else if (rt.nsets > 1) q.src_per_split = run_per_split(run);                     // (a split sky of ONE run: the plan's pieces stand)
      q.accumulate = (r > 0 && rt.nsets == 1) ? 1 : 0;
      q.out_set = rt.nsets == 1 ? 0 : r;
      q.cull_row = -1;
      if (run.kappa > 0.0) {
        if (rt.cull) q.cull_row = run.tab_row;
        if (split) { q.family = kFamPackedF32Split; q.kappa0 = run.kappa; q.flags_row = r; }
        else taper_f64(q);
      } else {
        // point sources: w = 1 (:6270 sigma = inf).  Packed fp32: the lifting / plain bodies.  fp64: the kernel without the taper (6.2
        // instead of 9.8 instructions per term); its rows are (up, down) pairs: this run's rows are re-packed in that layout
        q.taper = 0;
        q.family = split ? kFamPackedF32 : kFamRec;
        q.repack_pairs = !split;
      }
      rt.launch[r] = q;
    }
    rt.family = split ? kFamPackedF32Split : (wave ? kFamTaperF64Wave : kFamTaperF64Block);
  } else {
    if (pl.pk) whole.family = kFamPackedF32;
    else if (g64) taper_f64(whole);
    else whole.family = kFamRec;
    rt.family = whole.family;
    rt.launch[0] = whole;
  }
  rt.sum_family = rt.family;
  if (want_grad) { rt.family = kFamGradFourPass; rt.may_defer = false; }
  return rt;
}

// ---- many snapshots of a small array in one launch (catalog.cpp: run_wave_batch) ----------------------------------------------------

struct BatchPlan {
  bool eligible;           // as far as shape and hooks decide (the beam, the catalogue's order and the cull threshold: catalog.cpp)
  int ct, ntiles, nbw;
  int64_t npad, nsplit;
};

// s.nsrc: the size of the resident catalogue; kc: snapshots of the chunk.  A function of the array, the catalogue and the chunk length
// -- never of the counts, which the host has not seen.
inline BatchPlan batch_plan(const SkyShape& s, const SkyToggles& t, int precision, int64_t kc, bool want_grad) {
  BatchPlan b{};
  // precision: a request for fp32 arithmetic (PRISim's memsave) on an array this small is served by the SAME fp64 launch -- the cost of
  // a small array's snapshot is its launches, not its arithmetic (HERA-19: 26 us per snapshot batched in fp64 against a 45-50 us launch
  // chain per snapshot in either precision), and the result is the fp64 one (well inside the fp32 tolerance).
  // want_grad: the grouped fp64 gradient kernel on wave items of 16 baselines (k_skyvis_grad_taper_f64_batch), 32-channel tiles
  // One snapshot per call (observe() on a small array) takes the batched launch too -- 16-channel tiles, one round of wave slots, prepared
  // on the preparation stream under the previous snapshot's sky-sum, queued without a count (run_wave_batch): 100 us per observe() of
  // HERA-19 against 115 through the per-snapshot chain (tools/observe_single_ab.py).
  b.eligible = t.wave_batch && t.wave_items && (precision == PRISIM_FP64 || t.batch_fp32_as_fp64) &&
               !(kc < 1 || !s.uniform || s.nbl > kPlanBlock || s.nchan < 16) &&
               (!want_grad || (t.grad_taper_group && t.wave_batch_grad && t.fused_grad)) && (kc >= 2 || t.wave_batch_single) &&
               t.taper_f64_group && !s.tune_chunk;
  // 32-channel tiles (the seed of a (source, baseline, tile) triple is 26 % of a 32-channel tile's instructions, 41 % of a
  // 16-channel tile's), source splits so that the grid is about three rounds of two wavefronts per SIMD.
  // (one snapshot alone: 16-channel tiles and one round of wave slots -- the cut the single-launch planner arrives at for HERA-19)
  // (V + gradient: the MFMA kernel's wave follows 16 baselines x 4 sources on 32-channel tiles)
  int ct = s.tune_ct ? s.tune_ct : ((s.nchan >= 32 && kc > 1) ? 32 : 16);
  if (ct != 16 && ct != 32) ct = 32;
  if (want_grad) ct = 32;
  b.ct = ct;
  b.ntiles = (int)((s.nchan + ct - 1) / ct);
  b.nbw = want_grad ? (int)((s.nbl + 15) / 16) : (int)((s.nbl + 63) / 64);
  b.npad = round_up(std::max<int64_t>(s.nsrc, 1), 4);
  int64_t nsplit = s.tune_nsplit;
  if (nsplit == 0) {
    const int64_t slots = 2LL * 4 * std::max(s.cu_count, 1);
    const int64_t items0 = std::max<int64_t>(kc * b.nbw * b.ntiles, 1);
    const int64_t lo = std::max<int64_t>(1, ((kc > 1 ? 5 * slots / 2 : slots) + items0 - 1) / items0);
    // ... and of those counts the one whose last round is fullest (config 2 x 64 snapshots: 3 splits = 2.25 rounds 1.66 ms, 4 = 3.0 rounds
    // 1.52 ms, 5 = 3.75 rounds 1.58 ms; tools/config2_batch_sweep.py)
    double best = 1e30;
    nsplit = lo;
    for (int64_t n = lo; n <= 2 * lo; ++n) {
      const double r = (double)(items0 * n) / (double)slots;
      const double waste = std::ceil(r) / r + 0.002 * (double)(n - lo);
      if (waste < best - 1e-12) { best = waste; nsplit = n; }
    }
    if (kc == 1) nsplit = std::max<int64_t>(1, slots / items0);              // one snapshot alone: ONE round of wave slots, never a second
    nsplit = std::min<int64_t>(nsplit, std::max<int64_t>(1, s.nsrc / 32));   // (a horizon region of interest holds about half the catalogue)
    nsplit = std::min<int64_t>(nsplit, 64);
  }
  b.nsplit = nsplit;
  return b;
}

}  // namespace prisim
