// capi.cpp -- C-ABI of libprisim_hip.so (declared in include/prisim_hip.h).
//
// Owns the per-GPU context: HIP stream, resident array (baselines, channels), per-snapshot sky,
// the device visibility cube, and lazily dlopen()ed rocFFT / RCCL handles.  No C++ exception
// crosses the ABI; every export returns 0 or a negative PRISIM_E* code.
#include "ctx_internal.h"

namespace pint {

std::string g_create_error;
RcclApi g_rccl;
RocfftApi g_rocfft;

bool load_rccl(std::string& err) {
  if (g_rccl.handle) return true;
  // The ROCm RCCL this library was compiled against (<rccl/rccl.h> of /opt/rocm) first, by absolute path: a bare soname would
  // resolve to whatever librccl the process already carries (a python process that imported torch carries torch's bundled one).
  void* h = nullptr;
  std::string path;
  if (const char* env = getenv("PRISIM_RCCL_LIB")) { h = dlopen(env, RTLD_NOW | RTLD_LOCAL); if (h) path = env; }
  for (const char* cand : {"/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so", "librccl.so.1", "librccl.so"}) {
    if (h) break;
    h = dlopen(cand, RTLD_NOW | RTLD_LOCAL);
    if (h) path = cand;
  }
  if (!h) { err = std::string("cannot load librccl: ") + dlerror(); return false; }
  bool ok = load_sym(h, "ncclGetUniqueId", g_rccl.GetUniqueId) && load_sym(h, "ncclCommInitRank", g_rccl.CommInitRank) &&
            load_sym(h, "ncclAllGather", g_rccl.AllGather) && load_sym(h, "ncclCommDestroy", g_rccl.CommDestroy) &&
            load_sym(h, "ncclGetErrorString", g_rccl.GetErrorString);
  if (!ok) { err = "librccl lacks a required symbol"; dlclose(h); return false; }
  if (!(load_sym(h, "ncclSend", g_rccl.Send) && load_sym(h, "ncclRecv", g_rccl.Recv) && load_sym(h, "ncclGroupStart", g_rccl.GroupStart) &&
        load_sym(h, "ncclGroupEnd", g_rccl.GroupEnd)))
    g_rccl.Send = nullptr;                              // gather-to-root then reports PRISIM_ELIB
  (void)load_sym(h, "ncclGetVersion", g_rccl.GetVersion);
  (void)load_sym(h, "ncclGetLastError", g_rccl.GetLastError);
  g_rccl.path = path;
  g_rccl.handle = h;
  return true;
}

bool load_rocfft(std::string& err) {
  if (g_rocfft.handle) return true;
  void* h = dlopen("librocfft.so.0", RTLD_NOW | RTLD_LOCAL);
  if (!h) h = dlopen("librocfft.so", RTLD_NOW | RTLD_LOCAL);
  if (!h) h = dlopen("/opt/rocm/lib/librocfft.so.0", RTLD_NOW | RTLD_LOCAL);
  if (!h) { err = std::string("cannot load librocfft: ") + dlerror(); return false; }
  RocfftApi& a = g_rocfft;
  bool ok = load_sym(h, "rocfft_setup", a.setup) && load_sym(h, "rocfft_plan_create", a.plan_create) &&
            load_sym(h, "rocfft_plan_destroy", a.plan_destroy) &&
            load_sym(h, "rocfft_plan_get_work_buffer_size", a.plan_get_work_buffer_size) &&
            load_sym(h, "rocfft_execution_info_create", a.execution_info_create) &&
            load_sym(h, "rocfft_execution_info_destroy", a.execution_info_destroy) &&
            load_sym(h, "rocfft_execution_info_set_stream", a.execution_info_set_stream) &&
            load_sym(h, "rocfft_execution_info_set_work_buffer", a.execution_info_set_work_buffer) &&
            load_sym(h, "rocfft_execute", a.execute);
  if (!ok) { err = "librocfft lacks a required symbol"; dlclose(h); return false; }
  a.handle = h;
  return true;
}

}  // namespace pint


extern "C" {

const char* prisim_hip_version(void) { return "prisim_hip 0.5 gfx950"; }     // 0.5: the snapshot carries its frame; shard map

const char* prisim_hip_last_error(const prisim_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int prisim_hip_create(int device, prisim_ctx** out) {
  return guarded(nullptr, [&]() -> int {
  if (!out) return fail(nullptr, PRISIM_EINVAL, "out is NULL");
  *out = nullptr;
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0)
    return fail(nullptr, PRISIM_ENODEV, std::string("no HIP device available: ") + hipGetErrorString(e));
  if (device < 0 || device >= ndev)
    return fail(nullptr, PRISIM_EINVAL, "device index out of range (" + std::to_string(ndev) + " visible)");
  prisim_ctx* ctx = new (std::nothrow) prisim_ctx();
  if (!ctx) return fail(nullptr, PRISIM_ENOMEM, "out of host memory");
  ctx->device = device;
  e = hipSetDevice(device);
  if (e == hipSuccess) e = hipStreamCreate(&ctx->stream);
  for (int i = 0; i < prisim_ctx::kTimingRing && e == hipSuccess; ++i) {
    if ((e = hipEventCreate(&ctx->ev_c0[i])) != hipSuccess || (e = hipEventCreate(&ctx->ev_c1[i])) != hipSuccess ||
        (e = hipEventCreate(&ctx->ev_k0[i])) != hipSuccess || (e = hipEventCreate(&ctx->ev_k1[i])) != hipSuccess)
      break;
  }
  if (e != hipSuccess) {
    std::string m = std::string("HIP context setup failed: ") + hipGetErrorString(e);
    prisim_hip_destroy(ctx);
    return fail(nullptr, PRISIM_ENODEV, m);
  }
  // the catalogue path's two priority streams and their events belong to the context too (5 ms to create: not in front of a run's first
  // snapshot); a failure here is not fatal -- the path tries again when it is first used and reports it then
  if (catalog_streams(ctx) != PRISIM_OK) { ctx->err.clear(); (void)hipGetLastError(); }
  // the post stream of the deferred reduce / expand pass (ctx_internal.h): non-blocking and of the highest priority, as the side streams
  // above -- two short memory passes that must be scheduled beside a sky-sum grid occupying every CU.  Not fatal either: without it
  // every compute() keeps the single-stream order.
  {
    int least = 0, greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) { least = greatest = 0; (void)hipGetLastError(); }
    bool ok = hipStreamCreateWithPriority(&ctx->post_stream, hipStreamNonBlocking, greatest) == hipSuccess;
    if (!ok) { (void)hipGetLastError(); ctx->post_stream = nullptr; ok = hipStreamCreateWithFlags(&ctx->post_stream, hipStreamNonBlocking) == hipSuccess; }
    for (int i = 0; i < 2 && ok; ++i) ok = hipEventCreateWithFlags(&ctx->ev_post[i], hipEventDisableTiming) == hipSuccess;
    if (!ok) {
      (void)hipGetLastError();
      for (hipEvent_t& ev : ctx->ev_post) { if (ev) (void)hipEventDestroy(ev); ev = nullptr; }
      if (ctx->post_stream) (void)hipStreamDestroy(ctx->post_stream);
      ctx->post_stream = nullptr;
    }
  }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess) {
    snprintf(ctx->devname, sizeof(ctx->devname), "%s (%s)", prop.name, prop.gcnArchName);
    ctx->cu_count = prop.multiProcessorCount;
    ctx->clock_khz = prop.clockRate;
  }
  *out = ctx;
  return PRISIM_OK;
  });
}

void prisim_hip_destroy(prisim_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  if (ctx->post_stream) (void)hipStreamSynchronize(ctx->post_stream);
  catalog_destroy(ctx);
  if (ctx->comm_stream) (void)hipStreamSynchronize(ctx->comm_stream);
  if (ctx->comm && g_rccl.CommDestroy) g_rccl.CommDestroy(ctx->comm);
  if (ctx->copy_stream) (void)hipStreamSynchronize(ctx->copy_stream);
  if (ctx->ev_slot_done) (void)hipEventDestroy(ctx->ev_slot_done);
  for (int i = 0; i < prisim_ctx::kCommRing; ++i)
    for (hipEvent_t ev : {ctx->ev_gc[i], ctx->ev_g0[i], ctx->ev_g1[i], ctx->ev_gu[i]})
      if (ev) (void)hipEventDestroy(ev);
  if (ctx->comm_stream) (void)hipStreamDestroy(ctx->comm_stream);
  if (ctx->ev_copy_ready) (void)hipEventDestroy(ctx->ev_copy_ready);
  if (ctx->copy_stream) (void)hipStreamDestroy(ctx->copy_stream);
  if (ctx->fft_plan && g_rocfft.plan_destroy) g_rocfft.plan_destroy(ctx->fft_plan);
  if (ctx->fft_info && g_rocfft.execution_info_destroy) g_rocfft.execution_info_destroy(ctx->fft_info);
  for (DevBuf* b : {&ctx->blx, &ctx->bly, &ctx->blz, &ctx->ublx, &ctx->ubly, &ctx->ublz, &ctx->fold_map, &ctx->fold_vis, &ctx->fold_grad, &ctx->freqs, &ctx->fsq, &ctx->fsq_pairs, &ctx->cube, &ctx->grad, &ctx->dirs,
                    &ctx->partial, &ctx->partial_b, &ctx->tail_lo, &ctx->tail_tab, &ctx->scratch, &ctx->gathered, &ctx->sendbuf, &ctx->shard_map, &ctx->stage_main, &ctx->stage_comm, &ctx->ext_table,
                    &ctx->ext_work, &ctx->ext_colmax, &ctx->sky_flux, &ctx->sky_sp, &ctx->sky_bf, &ctx->sky_flag,
                    &ctx->dl_stage, &ctx->grp_hz, &ctx->fft_work, &ctx->fft_buf, &ctx->dt_out, &ctx->dt_pow, &ctx->dt_wts, &ctx->dt_lag_all, &ctx->dt_pow_all, &ctx->dt_tw})
    release(*b);
  for (SkyBufs& k : ctx->skb) {
    for (DevBuf* b : {&k.pb, &k.packed, &k.dirs_prep, &k.dirs_c32, &k.lift_flags, &k.wide_flags, &k.split_flags, &k.moments, &k.moments_part, &k.split_count, &k.cull_first,
                      &k.dirs_sorted, &k.idx_sorted, &k.batch_tab})
      release(*b);
    if (k.ev_prep) (void)hipEventDestroy(k.ev_prep);
    if (k.ev_sum) (void)hipEventDestroy(k.ev_sum);
  }
  for (int i = 0; i < prisim_ctx::kTimingRing; ++i)
    for (hipEvent_t ev : {ctx->ev_c0[i], ctx->ev_c1[i], ctx->ev_k0[i], ctx->ev_k1[i]})
      if (ev) (void)hipEventDestroy(ev);
  for (hipEvent_t ev : ctx->ev_post) if (ev) (void)hipEventDestroy(ev);
  if (ctx->post_stream) (void)hipStreamDestroy(ctx->post_stream);
  if (ctx->ev_stage) (void)hipEventDestroy(ctx->ev_stage);
  if (ctx->ev_d0) (void)hipEventDestroy(ctx->ev_d0);
  if (ctx->ev_d1) (void)hipEventDestroy(ctx->ev_d1);
  if (ctx->h_stage) (void)hipHostFree(ctx->h_stage);
  if (ctx->h_split_count) (void)hipHostFree(ctx->h_split_count);
  if (ctx->ev_tail) (void)hipEventDestroy(ctx->ev_tail);
  if (ctx->h_tail) (void)hipHostFree(ctx->h_tail);
  if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
}

int prisim_hip_set_array(prisim_ctx* ctx, const double* bl_enu, int64_t nbl, const double* freqs_hz, int64_t nchan,
                         int64_t nt_max) {
  return guarded(ctx, [&]() -> int {
  if (!ctx) return PRISIM_EINVAL;
  if (!bl_enu || !freqs_hz) return fail(ctx, PRISIM_EINVAL, "bl_enu / freqs_hz is NULL");
  if (nbl <= 0 || nchan <= 0 || nt_max <= 0) return fail(ctx, PRISIM_EINVAL, "nbl, nchan and nt_max must be positive");
  if (nbl > (int64_t)1 << 30 || nchan > (int64_t)1 << 24) return fail(ctx, PRISIM_EINVAL, "nbl or nchan too large");
  for (int64_t i = 0; i < nchan; ++i)
    if (!std::isfinite(freqs_hz[i])) return fail(ctx, PRISIM_EINVAL, "non-finite channel frequency");
  {
    // The phase range of the kernels (prisim_hip.h): they take the quadrant of 4 x phase with (int)q, so |4 phase| < 2^31 must hold for
    // every term; |s - s_pc| <= 2 for unit vectors, so max|b| 2 max|f| / c < 2^29 cycles guarantees it.  Refused here, on the host,
    // before any state changes: no kernel ever runs past the range.  (A non-finite length is left to the per-component
    // check below.)
    double lmax = 0.0, fmax = 0.0;
    for (int64_t b = 0; b < nbl; ++b) {
      const double len = std::sqrt(bl_enu[3 * b] * bl_enu[3 * b] + bl_enu[3 * b + 1] * bl_enu[3 * b + 1] + bl_enu[3 * b + 2] * bl_enu[3 * b + 2]);
      if (std::isfinite(len)) lmax = std::max(lmax, len);
    }
    for (int64_t i = 0; i < nchan; ++i) fmax = std::max(fmax, std::fabs(freqs_hz[i]));
    const double cycles = lmax * 2.0 * fmax / kC;
    if (cycles >= 536870912.0) {
      char msg[200];
      snprintf(msg, sizeof msg, "phase range: max|b| * 2 * max|f| / c = %.6g cycles, the limit is below 2^29 = 536870912 cycles", cycles);
      return fail(ctx, PRISIM_EINVAL, msg);
    }
  }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  ctx->array_set = false;
  ctx->sky_set = false;
  ctx->ext_nside = 0;   // the external-beam table is per channel grid
  if (ctx->cat.gstream) HIPCHK(ctx, hipStreamSynchronize(ctx->cat.gstream));
  if (ctx->prep_stream) HIPCHK(ctx, hipStreamSynchronize(ctx->prep_stream));
  ctx->prep_async = false;
  ctx->sk = &ctx->skb[0];
  ctx->cat.loaded = false;   // ... and so are the catalogue's spectra
  ctx->cat.cur = -1;
  std::vector<double> x(nbl), y(nbl), z(nbl);
  for (int64_t b = 0; b < nbl; ++b) {
    x[b] = bl_enu[3 * b]; y[b] = bl_enu[3 * b + 1]; z[b] = bl_enu[3 * b + 2];
    if (!std::isfinite(x[b]) || !std::isfinite(y[b]) || !std::isfinite(z[b]))
      return fail(ctx, PRISIM_EINVAL, "non-finite baseline component");
  }
  // Fold map: rows of equal vectors are summed once and expanded into the cube (baseline_fold.h).  On when it removes at least an
  // eighth of the rows and the folded array is still more than one baseline group, so that a folded context never enters the
  // wave-item or batched small-array paths (those are chosen by ctx->nbl <= kBlockThreads).  PRISIM_HIP_FOLD=0: off (the A/B hook).
  // Vectors equal to rounding (within 16 ulp of the largest coordinate, per component) are merged onto the first of them when that
  // leaves fewer rows and the phase it can cost, 2 pi f_max / c * 2 * max|b - b_rep|, is within 1e-12 rad (choose_fold): the kernels
  // then see the representatives' vectors.  PRISIM_HIP_FOLD_NEAR=0: the exact fold only (the A/B hook, the bits of the form without it).
  std::vector<int64_t> fold_rep;
  std::vector<int32_t> fold_map;
  fold_baselines(bl_enu, nbl, fold_rep, fold_map);
  {
    std::vector<int64_t> near_rep;
    std::vector<int32_t> near_map;
    double max_dev = 0.0, fmax = 0.0;
    fold_baselines_near(bl_enu, nbl, fold_near_tol(bl_enu, nbl), near_rep, near_map, max_dev);
    for (int64_t i = 0; i < nchan; ++i) fmax = std::max(fmax, std::fabs(freqs_hz[i]));
    bool allow_near = true, allow = true;
    if (const char* env = getenv("PRISIM_HIP_FOLD_NEAR")) allow_near = atoi(env) != 0;
    if (const char* env = getenv("PRISIM_HIP_FOLD")) allow = atoi(env) != 0;
    ctx->fold_exact_nbl = (int64_t)fold_rep.size();
    ctx->fold_near_nbl = (int64_t)near_rep.size();
    ctx->fold_near_max_dev = max_dev;
    ctx->fold_near_phase = fold_near_phase_bound(max_dev, fmax);
    const FoldKind kind = !allow ? kFoldNone : choose_fold(nbl, ctx->fold_exact_nbl, ctx->fold_near_nbl, ctx->fold_near_phase, kBlockThreads, allow_near);
    ctx->fold_near_used = kind == kFoldNear;
    if (kind == kFoldNear) { fold_rep.swap(near_rep); fold_map.swap(near_map); }
    else if (kind == kFoldNone) { fold_rep.clear(); }
  }
  const int64_t nbl_u = (int64_t)fold_rep.size();
  const bool fold = nbl_u > 0;
  // PRISIM_HIP_WIDE_LEAPFROG=0: no group takes the wide tier of the fp32 leapfrog (step_bound.h); the A/B hook, bit-identical to the form without it
  ctx->wide_leapfrog = true;
  if (const char* env = getenv("PRISIM_HIP_WIDE_LEAPFROG")) ctx->wide_leapfrog = atoi(env) != 0;
  // PRISIM_HIP_DEFER_POST=0: reduce / expand stay on the compute stream behind their sky-sum (the A/B hook of the deferred post-pass)
  ctx->defer_post = true;
  if (const char* env = getenv("PRISIM_HIP_DEFER_POST")) ctx->defer_post = atoi(env) != 0;
  // PRISIM_HIP_TAIL_PIECES (tail_plan.h): 0 = the plan's equal source pieces (the A/B hook, the bits of the form without the rule),
  // "force" = the rule without its depth condition and 64-source floor (the test mode for small shapes); unset: the rule
  ctx->tail_mode = kTailRule;
  if (const char* env = getenv("PRISIM_HIP_TAIL_PIECES")) ctx->tail_mode = strcmp(env, "force") == 0 ? kTailForce : (atoi(env) != 0 ? kTailRule : kTailOff);
  ctx->tail_key[0] = -1;      // (the tables are formed again for this array)
  // Four workgroups per CU.  Measured on the headline step beside the next sky-sum (profiles/LOG.md 4.1.9): the kernels' own grids
  // (8192 workgroups) flood the CUs and the memory system while the next snapshot's pack / prep and first round of sky-sum blocks start,
  // one or two per CU keep the passes resident for a millisecond and cost the sky-sum more than they hide.
  ctx->post_blocks = 4 * std::max(ctx->cu_count, 1);
  if (const char* env = getenv("PRISIM_HIP_POST_BLOCKS")) { const int v = atoi(env); if (v >= 0 && v <= 8192) ctx->post_blocks = v; }      // (0: unbounded)
  const int64_t nbl_sum = fold ? nbl_u : nbl;
  std::vector<double> ux, uy, uz;
  if (fold) {
    ux.resize((size_t)nbl_u); uy.resize((size_t)nbl_u); uz.resize((size_t)nbl_u);
    for (int64_t u = 0; u < nbl_u; ++u) { ux[u] = x[fold_rep[u]]; uy[u] = y[fold_rep[u]]; uz[u] = z[fold_rep[u]]; }
  }
  const std::vector<double>&sx = fold ? ux : x, &sy = fold ? uy : y, &sz = fold ? uz : z;      // the array the sky-sum kernels see
  int rc;
  const size_t bb = (size_t)nbl * sizeof(double);
  ctx->folded = false;
  if (fold) {
    const size_t ub = (size_t)nbl_u * sizeof(double);
    if ((rc = ensure(ctx, ctx->ublx, ub)) || (rc = ensure(ctx, ctx->ubly, ub)) || (rc = ensure(ctx, ctx->ublz, ub)) ||
        (rc = ensure(ctx, ctx->fold_map, (size_t)nbl * sizeof(int32_t))) ||
        (rc = ensure(ctx, ctx->fold_vis, (size_t)nbl_u * nchan * 2 * sizeof(double))))
      return rc;
    HIPCHK(ctx, hipMemcpyAsync(ctx->ublx.p, ux.data(), ub, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ctx->ubly.p, uy.data(), ub, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ctx->ublz.p, uz.data(), ub, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ctx->fold_map.p, fold_map.data(), (size_t)nbl * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  } else {
    for (DevBuf* b : {&ctx->ublx, &ctx->ubly, &ctx->ublz, &ctx->fold_map, &ctx->fold_vis}) release(*b);
  }
  release(ctx->fold_grad);           // (sized by compute() when a gradient is first asked for)
  if ((rc = ensure(ctx, ctx->blx, bb)) || (rc = ensure(ctx, ctx->bly, bb)) || (rc = ensure(ctx, ctx->blz, bb))) return rc;
  ctx->nchan_pad = round_up(nchan, 64);
  if ((rc = ensure(ctx, ctx->freqs, (size_t)nchan * sizeof(double)))) return rc;
  if ((rc = ensure(ctx, ctx->fsq, (size_t)ctx->nchan_pad * sizeof(float)))) return rc;
  const size_t cube_bytes = (size_t)nt_max * nbl * nchan * 2 * sizeof(double);
  if ((rc = ensure(ctx, ctx->cube, cube_bytes))) return rc;
  HIPCHK(ctx, hipMemcpyAsync(ctx->blx.p, x.data(), bb, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(ctx->bly.p, y.data(), bb, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(ctx->blz.p, z.data(), bb, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(ctx->freqs.p, freqs_hz, (size_t)nchan * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(ctx->cube.p, 0, cube_bytes, ctx->stream));
  HIPCHK(ctx, launch_fsq((const double*)ctx->freqs.p, (float*)ctx->fsq.p, nchan, ctx->nchan_pad, 1e-8, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  ctx->h_freqs.assign(freqs_hz, freqs_hz + nchan);
  // (last_lift_groups is reported in the caller's units, groups of 256 cube rows: their longest baselines, folded or not)
  ctx->row_grp_maxlen.assign((size_t)((nbl + kBlockThreads - 1) / kBlockThreads), 0.0);
  for (int64_t b = 0; b < nbl; ++b) {
    const double len = std::sqrt(x[b] * x[b] + y[b] * y[b] + z[b] * z[b]);
    const size_t g = (size_t)(b / kBlockThreads);
    if (len > ctx->row_grp_maxlen[g]) ctx->row_grp_maxlen[g] = len;
  }
  ctx->grp_maxlen.assign((size_t)((nbl_sum + kBlockThreads - 1) / kBlockThreads), 0.0);
  ctx->grp_maxh.assign(ctx->grp_maxlen.size(), 0.0);
  ctx->grp_maxz.assign(ctx->grp_maxlen.size(), 0.0);
  ctx->grp_minh.assign(ctx->grp_maxlen.size(), 1e300);
  ctx->grp_lmax = 0.0;
  ctx->fsq_pairs_ct = ctx->fsq_pairs_ntiles = -1;
  for (SkyBufs& k : ctx->skb) k.lift_key_k[0] = -1.0;             // the cached lifting flags belong to the previous array
  for (int64_t b = 0; b < nbl_sum; ++b) {
    const double len = std::sqrt(sx[b] * sx[b] + sy[b] * sy[b] + sz[b] * sz[b]);
    const size_t g = (size_t)(b / kBlockThreads);
    if (len > ctx->grp_maxlen[g]) ctx->grp_maxlen[g] = len;
    if (len > ctx->grp_lmax) ctx->grp_lmax = len;
    const double hl = std::sqrt(sx[b] * sx[b] + sy[b] * sy[b]);
    if (hl < ctx->grp_minh[g]) ctx->grp_minh[g] = hl;
    if (hl > ctx->grp_maxh[g]) ctx->grp_maxh[g] = hl;
    if (std::fabs(sz[b]) > ctx->grp_maxz[g]) ctx->grp_maxz[g] = std::fabs(sz[b]);
  }
  {
    const size_t ng = ctx->grp_maxh.size();
    std::vector<double> hz(4 * ng);
    for (size_t g = 0; g < ng; ++g) { hz[g] = ctx->grp_maxh[g]; hz[ng + g] = ctx->grp_maxz[g]; hz[2 * ng + g] = ctx->grp_maxlen[g]; hz[3 * ng + g] = ctx->grp_minh[g]; }
    if ((rc = ensure(ctx, ctx->grp_hz, 4 * ng * sizeof(double)))) return rc;
    HIPCHK(ctx, hipMemcpy(ctx->grp_hz.p, hz.data(), 4 * ng * sizeof(double), hipMemcpyHostToDevice));
  }
  ctx->nbl = nbl; ctx->nchan = nchan; ctx->nt_max = nt_max;
  ctx->nbl_sum = nbl_sum; ctx->folded = fold;
  // uniform channel grid?  f_k = f0 + k*df to within 1e-7 Hz (phase error <= 1e-13 cycles at 1 us delay)
  ctx->f0 = freqs_hz[0];
  ctx->df = nchan > 1 ? (freqs_hz[nchan - 1] - freqs_hz[0]) / (double)(nchan - 1) : 0.0;
  ctx->uniform = true;
  for (int64_t k = 0; k < nchan; ++k)
    if (std::fabs(freqs_hz[k] - (ctx->f0 + (double)k * ctx->df)) > 1e-7) { ctx->uniform = false; break; }
  release(ctx->grad);
  release(ctx->gathered);
  release(ctx->sendbuf);
  release(ctx->stage_main); release(ctx->stage_comm);
  if (ctx->nbl_total > 0 && (int64_t)ctx->shard_map_h.size() != (int64_t)ctx->nranks * nbl) {   // a shard map is per shard size
    ctx->nbl_total = 0; ctx->shard_map_h.clear(); release(ctx->shard_map);
  }
  release(ctx->dt_lag_all);
  release(ctx->dt_pow_all);
  ctx->dt_nt = ctx->dt_nout = 0;
  ctx->dt_have_lag = ctx->dt_have_pow = false;
  ctx->array_set = true;
  return PRISIM_OK;
  });
}

// Directions + source-shape constants of one snapshot -> ctx->dirs, through the pinned staging area (no synchronisation).
// `extra_stage_bytes`: staging the caller will use for its own small uploads in the same group (it calls stage_end()).
}  // extern "C"
namespace pint {
int upload_common(prisim_ctx* ctx, int64_t nsrc, const double* dircos, const double* pc_dircos,
                         const double* fwhm_deg, size_t extra_stage_bytes) {
  if (nsrc < 0) return fail(ctx, PRISIM_EINVAL, "nsrc must be non-negative");
  if (nsrc > (int64_t)0x7fff0000) return fail(ctx, PRISIM_EINVAL, "nsrc must be below 2^31 (the kernels index sources with 32 bits)");
  if (nsrc > 0 && !dircos) return fail(ctx, PRISIM_EINVAL, "dircos is NULL");
  if (!pc_dircos) return fail(ctx, PRISIM_EINVAL, "pc_dircos is NULL");
  for (int i = 0; i < 3; ++i)
    if (!std::isfinite(pc_dircos[i])) return fail(ctx, PRISIM_EINVAL, "non-finite pc_dircos");
  const size_t d4_bytes = (size_t)std::max<int64_t>(nsrc, 1) * 4 * sizeof(double);
  const size_t cull_bytes = 2 * 8 * ctx->grp_maxlen.size() * sizeof(int32_t) + 512;      // [precision][<= 8 runs][groups]
  int rc;
  if ((rc = stage_begin(ctx, d4_bytes + extra_stage_bytes + cull_bytes + 4096))) return rc;
  double* d4 = (double*)stage_alloc(ctx, d4_bytes);
  if (!d4) return fail(ctx, PRISIM_EINTERNAL, "staging area too small");
  d4[0] = d4[1] = d4[2] = d4[3] = 0.0;
  double dmax2 = 0.0, hmax2 = 0.0, zmax2 = 0.0;        // extrema of e = s - s_pc: |e|^2, its horizontal part, its vertical part (step_bound.h)
  for (int64_t s = 0; s < nsrc; ++s) {
    {
      const double ex = dircos[3 * s] - pc_dircos[0], ey = dircos[3 * s + 1] - pc_dircos[1], ez = dircos[3 * s + 2] - pc_dircos[2];
      const double h2 = ex * ex + ey * ey, z2 = ez * ez;
      const double e2 = h2 + z2;
      if (e2 > dmax2) dmax2 = e2;
      if (h2 > hmax2) hmax2 = h2;
      if (z2 > zmax2) zmax2 = z2;
    }
    for (int i = 0; i < 3; ++i) {
      const double v = dircos[3 * s + i];
      if (!std::isfinite(v)) return fail(ctx, PRISIM_EINVAL, "non-finite direction cosine");
      d4[4 * s + i] = v;
    }
    double kappa = 0.0;
    if (fwhm_deg) {
      const double fw = fwhm_deg[s];
      if (!std::isfinite(fw) || fw < 0.0) return fail(ctx, PRISIM_EINVAL, "invalid source FWHM");
      // interferometry.py:6268-6283:  w = exp(-ln2 * (2 sin(FWHM/2))^2 * (|b|^2 - (b.s)^2) * f^2 / c^2)
      const double fd = 2.0 * std::sin(0.5 * fw * M_PI / 180.0);
      kappa = M_LN2 * fd * fd;
    }
    d4[4 * s + 3] = kappa;
  }
  ctx->kappa_runs.clear();
  if (fwhm_deg && nsrc > 0) {
    int64_t lo = 0;
    for (int64_t s = 1; s <= nsrc; ++s) {
      if (s == nsrc || d4[4 * s + 3] != d4[4 * lo + 3]) {
        if (ctx->kappa_runs.size() == (size_t)kMaxRuns) { ctx->kappa_runs.clear(); break; }     // sizes vary source by source: no runs
        ctx->kappa_runs.push_back({lo, s, d4[4 * lo + 3], (int)ctx->kappa_runs.size()});
        lo = s;
      }
    }
  }
  if ((rc = ensure(ctx, ctx->dirs, d4_bytes))) return rc;
  HIPCHK(ctx, stage_send(ctx, ctx->dirs.p, d4, d4_bytes));
  if (ctx->prep_async) {             // the previous sky was prepared on the preparation stream: let it drain, then back to one stream
    HIPCHK(ctx, hipStreamSynchronize(ctx->prep_stream));
    ctx->prep_async = false;
  }
  ctx->sk = &ctx->skb[0];
  ctx->dirs_p = static_cast<const double*>(ctx->dirs.p);       // an uploaded sky: no catalogue indirection
  ctx->src_index = nullptr;
  ctx->cat.cur = -1;
  // Taper culling.  w = exp(-kappa (|b|^2 - (b.s)^2) f^2/c^2), and for a baseline of horizontal length h and height z and a source at
  // (rho, n) = (sin, cos) of the zenith angle, (b.s)^2 <= (h rho + |z| |n|)^2, i.e. |b|^2 - (b.s)^2 >= (h |n| - |z| rho)^2 when
  // h |n| >= |z| rho (the identity h^2 + z^2 - (h rho + |z||n|)^2 = (h|n| - |z| rho)^2).  So for every baseline of a group (smallest
  // horizontal length Hmin, largest |b_z| Z) and every channel the exponent of source s is at least
  //   x_s = kappa_s max(Hmin |n_s| - Z rho_s, 0)^2 fmin^2/c^2 .
  // The leading sources of a run whose x_s >= T contribute together at most exp(-T) sum|pbflux|: T = 18 (1.5e-8) for fp32 requests --
  // far inside the 5e-6 tolerance -- and the packed fp32 kernels start the group's source loop behind them; T = 28 (7e-13 against
  // fp64's 1e-11) for fp64 requests, used by the grouped fp64 kernel k_skyvis_taper_f64 (skyvis_plan.h: route).
  // Long baselines over coarse diffuse pixels (config 4: MWA to 2.5 km, nside 64) shed the sources nearest the zenith this way when
  // the caller lists a run's sources by decreasing altitude (InterferometerArray.observe does); unordered skies just cull little.
  ctx->cull_any[0] = ctx->cull_any[1] = false;
  ctx->cull_frac[0] = ctx->cull_frac[1] = 0.0;
  ctx->cull_nruns = 0;
  {
    const char* env = getenv("PRISIM_HIP_TAPER_CULL");
    const size_t ng = ctx->grp_maxlen.size();
    const size_t nruns = ctx->kappa_runs.size();
    if (nruns > 0 && ng > 0 && !(env && atoi(env) == 0)) {
      const double fmin = std::min(std::fabs(ctx->h_freqs.front()), std::fabs(ctx->h_freqs.back()));
      const double fc2 = (fmin / kC) * (fmin / kC);
      int32_t* tab = (int32_t*)stage_alloc(ctx, 2 * nruns * ng * sizeof(int32_t));
      if (tab) {
        const double thr[2] = {28.0, 18.0};                      // index = precision (PRISIM_FP64 = 0, PRISIM_FP32 = 1)
        double culled[2] = {0.0, 0.0};
        // Serial host work per snapshot, so kept small: a run is only looked at when its longest-baseline group could cull anything at
        // all, (rho, |n|) of its sources are formed once (not per group and precision), and the fp64 walk (the higher threshold) never
        // goes past where the fp32 walk of the same group stopped.
        double hmax = 0.0;
        for (size_t g = 0; g < ng; ++g) hmax = std::max(hmax, ctx->grp_minh[g]);
        std::vector<double>& rho = ctx->cull_rho;
        std::vector<double>& an = ctx->cull_an;
        for (size_t r = 0; r < nruns; ++r) {
          const auto& run = ctx->kappa_runs[r];
          const bool any_possible = run.kappa > 0.0 && run.kappa * hmax * hmax * fc2 >= thr[1];
          int64_t nlead = 0;                                       // leading sources whose (rho, |n|) are formed so far
          if (any_possible) { rho.clear(); an.clear(); }
          for (size_t g = 0; g < ng; ++g) {
            int64_t first32 = run.lo;
            for (int pr = 1; pr >= 0; --pr) {                      // fp32 (threshold 18) first: the fp64 walk (28) stops no later
              int64_t sfirst = run.lo;
              const int64_t limit = pr == 1 ? run.hi : first32;
              if (any_possible && run.kappa * ctx->grp_minh[g] * ctx->grp_minh[g] * fc2 >= thr[pr]) {
                const double H = ctx->grp_minh[g], Z = ctx->grp_maxz[g];
                while (sfirst < limit) {
                  const int64_t i = sfirst - run.lo;
                  if (i >= nlead) {
                    const double l = d4[4 * sfirst], m = d4[4 * sfirst + 1];
                    rho.push_back(std::sqrt(l * l + m * m));
                    an.push_back(std::fabs(d4[4 * sfirst + 2]));
                    nlead = i + 1;
                  }
                  const double perp = H * an[(size_t)i] - Z * rho[(size_t)i];
                  if (!(perp > 0.0 && run.kappa * perp * perp * fc2 >= thr[pr])) break;
                  ++sfirst;
                }
              }
              if (pr == 1) first32 = sfirst;
              tab[(pr * nruns + r) * ng + g] = (int32_t)sfirst;
              if (sfirst > run.lo) {
                ctx->cull_any[pr] = true;
                const int64_t nb = std::min<int64_t>(kBlockThreads, ctx->nbl_sum - (int64_t)g * kBlockThreads);
                culled[pr] += (double)(sfirst - run.lo) * (double)nb;
              }
            }
          }
        }
        if (ctx->cull_any[0] || ctx->cull_any[1]) {
          if ((rc = ensure(ctx, ctx->sk->cull_first, 2 * nruns * ng * sizeof(int32_t)))) return rc;
          HIPCHK(ctx, stage_send(ctx, ctx->sk->cull_first.p, tab, 2 * nruns * ng * sizeof(int32_t)));
          ctx->cull_nruns = (int)nruns;
          for (int pr = 0; pr < 2; ++pr) ctx->cull_frac[pr] = culled[pr] / ((double)nsrc * (double)ctx->nbl_sum);
        }
      }
    }
  }
  ctx->nsrc = nsrc;
  ctx->dmax = std::sqrt(dmax2);
  ctx->hmax = std::sqrt(hmax2);
  ctx->zmax = std::sqrt(zmax2);
  ctx->taper = fwhm_deg != nullptr;
  for (int i = 0; i < 3; ++i) ctx->pc[i] = pc_dircos[i];
  return PRISIM_OK;
}

// Upload a caller array of `bytes`: staged (asynchronous) when small, otherwise straight from the caller's memory followed by
// a stream synchronisation (the caller may reuse the array as soon as the call returns).
int upload_any(prisim_ctx* ctx, void* dst, const void* src, size_t bytes, bool* synced) {
  if (bytes <= kStageMaxBytes && ctx->h_stage_used + bytes + 256 <= ctx->h_stage_bytes) {
    HIPCHK(ctx, stage_upload(ctx, dst, src, bytes));
    return PRISIM_OK;
  }
  HIPCHK(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  if (synced) *synced = true;
  return PRISIM_OK;
}
}  // namespace pint
extern "C" {

int prisim_hip_set_sky(prisim_ctx* ctx, const prisim_sky* sky) {
  return guarded(ctx, [&]() -> int {
  if (!ctx) return PRISIM_EINVAL;
  if (!sky) return fail(ctx, PRISIM_EINVAL, "sky is NULL");
  if (!ctx->array_set) return fail(ctx, PRISIM_ESTATE, "set_array must be called before set_sky");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  ctx->sky_set = false;
  if (sky->nsrc > 0 && !sky->pbflux) return fail(ctx, PRISIM_EINVAL, "pbflux is NULL");
  const int64_t n = sky->nsrc * ctx->nchan;
  const size_t pb_bytes = (size_t)std::max<int64_t>(n, 0) * (sky->pbflux_is_f32 ? sizeof(float) : sizeof(double));
  const size_t fl_bytes = sky->fluxes ? (size_t)std::max<int64_t>(n, 0) * sizeof(double) : 0;
  const size_t stage_extra = (pb_bytes <= kStageMaxBytes ? pb_bytes : 0) + (fl_bytes <= kStageMaxBytes ? fl_bytes : 0) + 1024;
  int rc = upload_common(ctx, sky->nsrc, sky->dircos, sky->pc_dircos, sky->fwhm_deg, stage_extra);
  if (rc) return rc;
  if ((rc = ensure(ctx, ctx->sk->pb, (size_t)std::max<int64_t>(n, 1) * sizeof(double)))) return rc;
  if (n > 0) {
    if (sky->pbflux_is_f32) {
      if ((rc = ensure(ctx, ctx->sky_flux, (size_t)n * sizeof(float)))) return rc;
      if ((rc = upload_any(ctx, ctx->sky_flux.p, sky->pbflux, (size_t)n * sizeof(float), nullptr))) return rc;
      HIPCHK(ctx, launch_f32_to_f64((const float*)ctx->sky_flux.p, (double*)ctx->sk->pb.p, n, ctx->stream));
    } else {
      if ((rc = upload_any(ctx, ctx->sk->pb.p, sky->pbflux, (size_t)n * sizeof(double), nullptr))) return rc;
    }
    if (sky->fluxes) {   // pbfluxes = pb * fluxes (:6254) on the device
      if ((rc = ensure(ctx, ctx->sky_sp, (size_t)n * sizeof(double)))) return rc;
      if ((rc = upload_any(ctx, ctx->sky_sp.p, sky->fluxes, (size_t)n * sizeof(double), nullptr))) return rc;
      HIPCHK(ctx, launch_mul_inplace((double*)ctx->sk->pb.p, (const double*)ctx->sky_sp.p, n, ctx->stream));
    }
  }
  stage_end(ctx);
  ctx->sky_set = true;
  return PRISIM_OK;
  }, /*join=*/false);      // (a sky setter touches the sky's own buffers only: the next sky-sum still runs over a deferred post-pass)
}

}  // extern "C"
namespace pint {

// argument checks of a fused analytic beam (prisim_beam_sky / prisim_obs)
int check_beam_spec(prisim_ctx* ctx, int beam_kind, double diameter_m, const double* beam_pc_dircos, const prisim_beam_ext* ext) {
  if (beam_kind < PRISIM_BEAM_DELTA || beam_kind > PRISIM_BEAM_POLY) return fail(ctx, PRISIM_EINVAL, "unknown beam_kind");
  if (beam_kind == PRISIM_BEAM_DIPOLE && !ext) return fail(ctx, PRISIM_EINVAL, "PRISIM_BEAM_DIPOLE needs a prisim_beam_ext (dipole axis)");
  if (beam_kind == PRISIM_BEAM_POLY && !ext) return fail(ctx, PRISIM_EINVAL, "PRISIM_BEAM_POLY needs a prisim_beam_ext (poly_coef)");
  if (ext) {
    const prisim_beam_ext* x = ext;
    if (x->dipole_mode < PRISIM_DIPOLE_GENERAL || x->dipole_mode > PRISIM_DIPOLE_HALFWAVE)
      return fail(ctx, PRISIM_EINVAL, "unknown dipole_mode");
    if (x->array_nax1 < 0 || x->array_nax2 < 0 || (x->array_nax1 > 0) != (x->array_nax2 > 0))
      return fail(ctx, PRISIM_EINVAL, "array_nax1 and array_nax2 must both be positive or both zero");
    if (x->array_nax1 > 0 && !(x->array_sep1 > 0.0 && x->array_sep2 > 0.0))
      return fail(ctx, PRISIM_EINVAL, "array element separations must be positive");
    if (!std::isfinite(x->ground_height) || !std::isfinite(x->array_east2ax1_deg))
      return fail(ctx, PRISIM_EINVAL, "non-finite beam extension parameter");
    if (x->bf_nelem < 0 || x->bf_nelem > 4096) return fail(ctx, PRISIM_EINVAL, "bf_nelem must be in 0 ... 4096");
    if (x->bf_nelem > 0) {
      if (x->bf_nrand < 1 || x->bf_nrand > 256) return fail(ctx, PRISIM_EINVAL, "bf_nrand must be in 1 ... 256");
      if (!x->bf_pos || !x->bf_delays || !x->bf_gains) return fail(ctx, PRISIM_EINVAL, "beamformer positions / delays / gains is NULL");
      if (x->array_nax1 > 0) return fail(ctx, PRISIM_EINVAL, "the beamformer replaces the analytic array factor: set array_nax1 = array_nax2 = 0");
      for (int64_t i = 0; i < (int64_t)x->bf_nelem * 3; ++i)
        if (!std::isfinite(x->bf_pos[i])) return fail(ctx, PRISIM_EINVAL, "non-finite beamformer element position");
      for (int64_t i = 0; i < (int64_t)x->bf_nelem * x->bf_nrand; ++i)
        if (!std::isfinite(x->bf_delays[i]) || !std::isfinite(x->bf_gains[i]))
          return fail(ctx, PRISIM_EINVAL, "non-finite beamformer delay / gain");
    }
  }
  if (beam_kind != PRISIM_BEAM_DELTA && beam_kind != PRISIM_BEAM_POLY && !(diameter_m > 0.0))
    return fail(ctx, PRISIM_EINVAL, "diameter_m must be positive");
  if (!beam_pc_dircos) return fail(ctx, PRISIM_EINVAL, "beam_pc_dircos is NULL");
  return PRISIM_OK;
}

size_t beamformer_doubles(const prisim_beam_ext* ext) {
  const int bf_n = ext ? ext->bf_nelem : 0, bf_r = bf_n > 0 ? ext->bf_nrand : 0;
  return (size_t)bf_n * 3 + 2 * (size_t)bf_n * bf_r;
}

// pbflux[s][f] = beam(dirs_p[s], f) x flux(src_index ? src_index[s] : s, f) of the current sky (ns sources) into ctx->sk->pb.  The flux
// pointers are device arrays (power law: d_flux_ref / d_spindex; tabulated: d_flux_spec).  A beamformer's element arrays (host, in ext)
// are sent through the OPEN staging group (the caller ran stage_begin with room for beamformer_doubles(ext) doubles and ends it).
int sky_beam_flux(prisim_ctx* ctx, int64_t ns, int beam_kind, double diameter_m, const double* beam_pc_dircos, const prisim_beam_ext* ext,
                  const double* d_flux_ref, const double* d_spindex, const double* d_flux_spec, double ref_freq, const int32_t* src_index) {
  int rc;
  const int bf_n = ext ? ext->bf_nelem : 0, bf_r = bf_n > 0 ? ext->bf_nrand : 0;
  if ((bf_n > 0 && (rc = ensure(ctx, ctx->sky_bf, beamformer_doubles(ext) * sizeof(double)))) || (rc = ensure(ctx, ctx->sky_flag, sizeof(int32_t))))
    return rc;
  if (bf_n > 0) {
    double* b = (double*)ctx->sky_bf.p;
    if ((rc = upload_any(ctx, b, ext->bf_pos, (size_t)bf_n * 3 * sizeof(double), nullptr)) ||
        (rc = upload_any(ctx, b + (size_t)bf_n * 3, ext->bf_delays, (size_t)bf_n * bf_r * sizeof(double), nullptr)) ||
        (rc = upload_any(ctx, b + (size_t)bf_n * 3 + (size_t)bf_n * bf_r, ext->bf_gains, (size_t)bf_n * bf_r * sizeof(double), nullptr)))
      return rc;
  }
  BeamParams bp{};
  bp.dirs = ctx->dirs_p;
  bp.flux_ref = d_flux_ref;
  bp.spindex = d_spindex;
  bp.flux_spec = d_flux_spec;
  bp.src_index = src_index;
  bp.freqs = (const double*)ctx->freqs.p;
  bp.ref_freq = d_flux_spec ? 1.0 : ref_freq;
  bp.beam_kind = beam_kind;
  bp.diameter = diameter_m;
  bp.bpc_x = beam_pc_dircos[0]; bp.bpc_y = beam_pc_dircos[1]; bp.bpc_z = beam_pc_dircos[2];
  if (ext) {
    const prisim_beam_ext* x = ext;
    bp.dip_x = x->dipole_dircos[0]; bp.dip_y = x->dipole_dircos[1]; bp.dip_z = x->dipole_dircos[2];
    bp.dipole_mode = x->dipole_mode;
    bp.nax1 = x->array_nax1; bp.nax2 = x->array_nax2; bp.sep1 = x->array_sep1; bp.sep2 = x->array_sep2;
    const double ang = x->array_east2ax1_deg * M_PI / 180.0;
    bp.rot_c = std::cos(ang); bp.rot_s = std::sin(ang);
    bp.apc_x = x->array_pc_dircos[0]; bp.apc_y = x->array_pc_dircos[1]; bp.apc_z = x->array_pc_dircos[2];
    bp.gp_height = x->ground_height; bp.gp_modify = x->ground_modify; bp.gp_scale = x->ground_scale; bp.gp_max = x->ground_max;
    if (bf_n > 0) {
      bp.bf_nelem = bf_n; bp.bf_nrand = bf_r;
      bp.bf_pos = (const double*)ctx->sky_bf.p;
      bp.bf_delays = bp.bf_pos + (size_t)bf_n * 3;
      bp.bf_gains = bp.bf_delays + (size_t)bf_n * bf_r;
    }
  }
  if (beam_kind == PRISIM_BEAM_POLY)
    for (int i = 0; i < 4; ++i) bp.poly[i] = ext->poly_coef[i];
  bp.flag = (int32_t*)ctx->sky_flag.p;
  bp.nsrc = ns; bp.nchan = ctx->nchan;
  bp.pb_out = (double*)ctx->sk->pb.p;
  HIPCHK(ctx, hipMemsetAsync(ctx->sky_flag.p, 0, sizeof(int32_t), pstream(ctx)));
  HIPCHK(ctx, launch_beam_flux(bp, pstream(ctx)));
  return PRISIM_OK;
}

// only the polynomial beams can trip the reference's validity checks (:510-512, :802-807): the one case that reads back
int check_poly_beam_flag(prisim_ctx* ctx) {
  int32_t hflag = 0;
  HIPCHK(ctx, hipMemcpyAsync(&hflag, ctx->sky_flag.p, sizeof(int32_t), hipMemcpyDeviceToHost, pstream(ctx)));
  HIPCHK(ctx, hipStreamSynchronize(pstream(ctx)));
  if (hflag & 2)
    return fail(ctx, PRISIM_EINVAL, "Primary beam values were found to be NaN in some case(s). Check if the polynomial equations are valid for the frequencies specified.");
  if (hflag & 1)
    return fail(ctx, PRISIM_EINVAL, "Primary beam exceeds unity by a significant amount. Check the validity of the Primary beam equation for the angles specified.");
  return PRISIM_OK;
}

}  // namespace pint
extern "C" {

int prisim_hip_set_sky_analytic(prisim_ctx* ctx, const prisim_beam_sky* sky) {
  return guarded(ctx, [&]() -> int {
  if (!ctx) return PRISIM_EINVAL;
  if (!sky) return fail(ctx, PRISIM_EINVAL, "sky is NULL");
  if (!ctx->array_set) return fail(ctx, PRISIM_ESTATE, "set_array must be called before set_sky_analytic");
  int rc;
  if ((rc = check_beam_spec(ctx, sky->beam_kind, sky->diameter_m, sky->beam_pc_dircos, sky->ext))) return rc;
  const bool have_spec = sky->flux_spectrum != nullptr;
  if (sky->nsrc > 0 && !have_spec && (!sky->flux_ref || !sky->spindex))
    return fail(ctx, PRISIM_EINVAL, "flux_ref / spindex is NULL and no flux_spectrum given");
  if (!have_spec && !(sky->ref_freq_hz > 0.0)) return fail(ctx, PRISIM_EINVAL, "ref_freq_hz must be positive");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  ctx->sky_set = false;
  const int64_t ns = sky->nsrc;
  const int64_t n = ns * ctx->nchan;
  const size_t frb = have_spec ? (size_t)n * sizeof(double) : (size_t)ns * sizeof(double);
  const size_t stage_extra = (frb <= kStageMaxBytes ? frb : 0) + (size_t)ns * sizeof(double) + beamformer_doubles(sky->ext) * sizeof(double) + 4096;
  rc = upload_common(ctx, ns, sky->dircos, sky->pc_dircos, sky->fwhm_deg, stage_extra);
  if (rc) return rc;
  if ((rc = ensure(ctx, ctx->sk->pb, (size_t)std::max<int64_t>(n, 1) * sizeof(double)))) return rc;
  if (ns > 0) {
    if ((rc = ensure(ctx, ctx->sky_flux, frb)) || (rc = ensure(ctx, ctx->sky_sp, (size_t)ns * sizeof(double)))) return rc;
    if ((rc = upload_any(ctx, ctx->sky_flux.p, have_spec ? sky->flux_spectrum : sky->flux_ref, frb, nullptr))) return rc;
    if (!have_spec && (rc = upload_any(ctx, ctx->sky_sp.p, sky->spindex, (size_t)ns * sizeof(double), nullptr))) return rc;
    if ((rc = sky_beam_flux(ctx, ns, sky->beam_kind, sky->diameter_m, sky->beam_pc_dircos, sky->ext, have_spec ? nullptr : (const double*)ctx->sky_flux.p,
                            have_spec ? nullptr : (const double*)ctx->sky_sp.p, have_spec ? (const double*)ctx->sky_flux.p : nullptr,
                            sky->ref_freq_hz, nullptr)))
      return rc;
    stage_end(ctx);
    if (sky->beam_kind == PRISIM_BEAM_POLY && (rc = check_poly_beam_flag(ctx))) return rc;
  } else {
    stage_end(ctx);
  }
  ctx->sky_set = true;
  return PRISIM_OK;
  }, /*join=*/false);      // (a sky setter touches the sky's own buffers only: the next sky-sum still runs over a deferred post-pass)
}

int prisim_hip_set_external_beam(prisim_ctx* ctx, const double* beam, int64_t npix, int64_t nfreq, const double* interp_matrix) {
  return guarded(ctx, [&]() -> int {
  if (!ctx) return PRISIM_EINVAL;
  if (!ctx->array_set) return fail(ctx, PRISIM_ESTATE, "set_array must be called before set_external_beam");
  if (!beam || !interp_matrix) return fail(ctx, PRISIM_EINVAL, "beam / interp_matrix is NULL");
  if (npix < 12 || nfreq < 1) return fail(ctx, PRISIM_EINVAL, "npix must be 12*nside^2 and nfreq >= 1");
  const int64_t nside = (int64_t)std::llround(std::sqrt((double)npix / 12.0));
  if (12 * nside * nside != npix || nside > (1 << 13)) return fail(ctx, PRISIM_EINVAL, "npix is not 12*nside^2");
  for (int64_t i = 0; i < npix * nfreq; ++i)
    if (!(beam[i] > 0.0) || !std::isfinite(beam[i]))
      return fail(ctx, PRISIM_EINVAL, "external beam values must be finite and > 0 (log10 is interpolated, run_prisim.py:2094)");
  for (int64_t i = 0; i < ctx->nchan * nfreq; ++i)
    if (!std::isfinite(interp_matrix[i])) return fail(ctx, PRISIM_EINVAL, "non-finite spectral interpolation weight");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  ctx->ext_nside = 0;
  DevBuf dbeam, dm;
  int rc;
  if ((rc = ensure(ctx, dbeam, (size_t)npix * nfreq * sizeof(double))) || (rc = ensure(ctx, dm, (size_t)ctx->nchan * nfreq * sizeof(double))) ||
      (rc = ensure(ctx, ctx->ext_table, (size_t)npix * ctx->nchan * sizeof(double)))) {
    release(dbeam); release(dm);
    return rc;
  }
  hipError_t e = hipMemcpyAsync(dbeam.p, beam, (size_t)npix * nfreq * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(dm.p, interp_matrix, (size_t)ctx->nchan * nfreq * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = launch_extbeam_table((const double*)dbeam.p, (const double*)dm.p, (double*)ctx->ext_table.p, npix, nfreq, ctx->nchan, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  release(dbeam); release(dm);
  HIPCHK(ctx, e);
  ctx->ext_nside = (int)nside;
  return PRISIM_OK;
  });
}

// beam table -> pbflux for the current directions; fluxes: device [nsrc][nchan] table, or NULL with flux_ref / spindex (device [nsrc])
}  // extern "C"
namespace pint {
int extbeam_sky(prisim_ctx* ctx, int64_t nsrc, const double* d_fluxes, const double* d_flux_ref, const double* d_spindex,
                double ref_freq, const int32_t* src_index) {
  const int64_t n = nsrc * ctx->nchan;
  int rc;
  // (grown with headroom: the region of interest of a drift scan grows by a few sources per snapshot, and an exact fit would re-allocate
  // -- and so drain the queue of -- almost every snapshot)
  if ((rc = ensure_grow(ctx, ctx->ext_work, (size_t)n * sizeof(double))) ||
      (rc = ensure(ctx, ctx->ext_colmax, (size_t)1025 * ctx->nchan * sizeof(double))))
    return rc;
  HIPCHK(ctx, launch_extbeam_sky((const double*)ctx->ext_table.p, ctx->ext_nside, ctx->dirs_p, d_fluxes, d_flux_ref, d_spindex,
                                 (const double*)ctx->freqs.p, ref_freq, (double*)ctx->ext_work.p, (double*)ctx->ext_colmax.p,
                                 (double*)ctx->sk->pb.p, nsrc, ctx->nchan, pstream(ctx), src_index));
  return PRISIM_OK;
}
}  // namespace pint
extern "C" {

int prisim_hip_set_sky_external(prisim_ctx* ctx, const prisim_sky* sky) {
  return guarded(ctx, [&]() -> int {
  if (!ctx) return PRISIM_EINVAL;
  if (!sky) return fail(ctx, PRISIM_EINVAL, "sky is NULL");
  if (!ctx->array_set) return fail(ctx, PRISIM_ESTATE, "set_array must be called before set_sky_external");
  if (ctx->ext_nside <= 0) return fail(ctx, PRISIM_ESTATE, "set_external_beam must be called before set_sky_external");
  if (sky->pbflux) return fail(ctx, PRISIM_EINVAL, "pbflux must be NULL: the beam comes from the external table");
  if (sky->nsrc > 0 && !sky->fluxes) return fail(ctx, PRISIM_EINVAL, "fluxes is NULL");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  ctx->sky_set = false;
  const int64_t n = sky->nsrc * ctx->nchan;
  const size_t fl_bytes = (size_t)std::max<int64_t>(n, 0) * sizeof(double);
  int rc = upload_common(ctx, sky->nsrc, sky->dircos, sky->pc_dircos, sky->fwhm_deg, (fl_bytes <= kStageMaxBytes ? fl_bytes : 0) + 1024);
  if (rc) return rc;
  if ((rc = ensure(ctx, ctx->sk->pb, (size_t)std::max<int64_t>(n, 1) * sizeof(double)))) return rc;
  if (n > 0) {
    if ((rc = ensure(ctx, ctx->sky_flux, fl_bytes))) return rc;
    if ((rc = upload_any(ctx, ctx->sky_flux.p, sky->fluxes, fl_bytes, nullptr))) return rc;
    if ((rc = extbeam_sky(ctx, sky->nsrc, (const double*)ctx->sky_flux.p, nullptr, nullptr, 1.0, nullptr))) return rc;
  }
  stage_end(ctx);
  ctx->sky_set = true;
  return PRISIM_OK;
  }, /*join=*/false);      // (a sky setter touches the sky's own buffers only: the next sky-sum still runs over a deferred post-pass)
}

int prisim_hip_set_sky_external_analytic(prisim_ctx* ctx, const prisim_beam_sky* sky) {
  return guarded(ctx, [&]() -> int {
  if (!ctx) return PRISIM_EINVAL;
  if (!sky) return fail(ctx, PRISIM_EINVAL, "sky is NULL");
  if (!ctx->array_set) return fail(ctx, PRISIM_ESTATE, "set_array must be called before set_sky_external_analytic");
  if (ctx->ext_nside <= 0) return fail(ctx, PRISIM_ESTATE, "set_external_beam must be called before set_sky_external_analytic");
  const bool have_spec = sky->flux_spectrum != nullptr;
  if (sky->nsrc > 0 && !have_spec && (!sky->flux_ref || !sky->spindex))
    return fail(ctx, PRISIM_EINVAL, "flux_ref / spindex is NULL and no flux_spectrum given");
  if (!have_spec && !(sky->ref_freq_hz > 0.0)) return fail(ctx, PRISIM_EINVAL, "ref_freq_hz must be positive");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  ctx->sky_set = false;
  const int64_t ns = sky->nsrc;
  const int64_t n = ns * ctx->nchan;
  const size_t frb = have_spec ? (size_t)std::max<int64_t>(n, 0) * sizeof(double) : (size_t)std::max<int64_t>(ns, 0) * sizeof(double);
  int rc = upload_common(ctx, ns, sky->dircos, sky->pc_dircos, sky->fwhm_deg,
                         (frb <= kStageMaxBytes ? frb : 0) + (size_t)std::max<int64_t>(ns, 0) * sizeof(double) + 2048);
  if (rc) return rc;
  if ((rc = ensure(ctx, ctx->sk->pb, (size_t)std::max<int64_t>(n, 1) * sizeof(double)))) return rc;
  if (ns > 0) {
    if ((rc = ensure(ctx, ctx->sky_flux, frb)) || (rc = ensure(ctx, ctx->sky_sp, (size_t)ns * sizeof(double)))) return rc;
    if ((rc = upload_any(ctx, ctx->sky_flux.p, have_spec ? sky->flux_spectrum : sky->flux_ref, frb, nullptr))) return rc;
    if (!have_spec && (rc = upload_any(ctx, ctx->sky_sp.p, sky->spindex, (size_t)ns * sizeof(double), nullptr))) return rc;
    if ((rc = extbeam_sky(ctx, ns, have_spec ? (const double*)ctx->sky_flux.p : nullptr, have_spec ? nullptr : (const double*)ctx->sky_flux.p,
                          have_spec ? nullptr : (const double*)ctx->sky_sp.p, have_spec ? 1.0 : sky->ref_freq_hz, nullptr)))
      return rc;
  }
  stage_end(ctx);
  ctx->sky_set = true;
  return PRISIM_OK;
  }, /*join=*/false);      // (a sky setter touches the sky's own buffers only: the next sky-sum still runs over a deferred post-pass)
}

int prisim_hip_get_pbflux(prisim_ctx* ctx, double* out) {
  return guarded(ctx, [&]() -> int {
  if (!ctx) return PRISIM_EINVAL;
  if (!ctx->sky_set) return fail(ctx, PRISIM_ESTATE, "no sky set");
  if (!out) return fail(ctx, PRISIM_EINVAL, "out is NULL");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const int64_t n = ctx->nsrc * ctx->nchan;
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  if (ctx->prep_async) HIPCHK(ctx, hipStreamSynchronize(ctx->prep_stream));
  if (n > 0) HIPCHK(ctx, hipMemcpy(out, ctx->sk->pb.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
  return PRISIM_OK;
  });
}

// kernel parameters of the current sky under route `rt`; every launch then sets its own (run_pass)
static void sky_params(prisim_ctx* ctx, const SkyShape& s, const SkyRoute& rt, SkyvisParams& p) {
  const Plan& pl = rt.pl;
  fill_params(ctx, p);
  p.dirs = ctx->dirs_p;
  p.fsq_pairs = (const float*)ctx->fsq_pairs.p;
  p.lift_flags = ctx->sk->lift_flags.p ? (const int32_t*)ctx->sk->lift_flags.p : nullptr;   // taper kernels: which groups need no re-anchoring
  // the wide tier: fp32 skies without the taper (the table is formed with lift_flags for every fp32 plan; a tapered sky's point-source runs keep the plain body)
  p.wide_flags = (pl.f32 && !ctx->taper && ctx->sk->wide_flags.p) ? (const int32_t*)ctx->sk->wide_flags.p : nullptr;
  p.nsrc = ctx->nsrc; p.nsrc_pad = pl.nsrc_pad;
  p.pc_x = ctx->pc[0]; p.pc_y = ctx->pc[1]; p.pc_z = ctx->pc[2];
  p.taper = ctx->taper ? 1 : 0;
  p.ntiles = pl.ntiles; p.nbgroups = pl.nbgroups; p.nsplit = pl.nsplit; p.src_per_split = pl.src_per_split;
  p.src_chunk = pl.chunk;
  p.flush_src = s.flush_src;
  p.src_lo = 0; p.src_hi = ctx->nsrc;
  p.taper_group = rt.taper_group;
  ctx->timing.last_taper_group = rt.last_taper_group;
}

// The device half of the packed fp32 taper's split form (skyvis_plan.h: split_eligible): its per-run, per-group flags.  Per baseline
// group, a bound on the parabola the uncorrected grouped form leaves: relative to a term it is at most
// 16 kappa (b.s)^2 df^2 / c^2 with (b.s)^2 <= (H rho_s + Z |n_s|)^2 (H, Z: the group's largest horizontal length and |b_z|), so
// relative to sum|pbflux| it is at most 16 kappa df^2/c^2 (H^2 M2 + 2 H Z M11 + Z^2 M02) with the beam-weighted moments
// M = sum_s |p_s| (.) / sum_s |p_s| of the run's sources, maximised over the channels (k_taper_moments: one pass over pbflux;
// k_split_flags turns them into the per-group flags ON THE DEVICE, so nothing is downloaded and a snapshot's launches never wait for
// the previous snapshot's sky-sum).  Groups above 2e-7 keep the correction (flag bit 1).  false: the unsplit packed kernel runs.
static bool split_flags_prepare(prisim_ctx* ctx) {
  const int64_t nchan = ctx->nchan;
  const size_t nruns = ctx->kappa_runs.size();
  const size_t ng = ctx->grp_maxh.size();
  if (ensure(ctx, ctx->sk->moments, (size_t)4 * nchan * sizeof(double) * nruns) != PRISIM_OK) return false;
  if (ensure(ctx, ctx->sk->split_flags, nruns * ng * sizeof(int32_t)) != PRISIM_OK) return false;
  if (ensure(ctx, ctx->sk->split_count, 8 * sizeof(int32_t)) != PRISIM_OK) return false;
  if (!ctx->h_split_count && hipHostMalloc((void**)&ctx->h_split_count, 8 * sizeof(int32_t), hipHostMallocDefault) != hipSuccess) {
    ctx->h_split_count = nullptr;
    return false;
  }
  // moments -> flags entirely on the stream: no download, so a snapshot's launches never wait for the previous snapshot's sky-sum
  if (hipMemsetAsync(ctx->sk->split_count.p, 0, 8 * sizeof(int32_t), pstream(ctx)) != hipSuccess) return false;
  for (size_t r = 0; r < nruns; ++r) {
    const auto& run = ctx->kappa_runs[r];
    if (run.kappa <= 0.0) continue;
    double* mom = (double*)ctx->sk->moments.p + r * (size_t)4 * nchan;
    if (ensure(ctx, ctx->sk->moments_part, (size_t)taper_moments_chunks(run.lo, run.hi) * 4 * nchan * sizeof(double)) != PRISIM_OK) return false;
    if (launch_taper_moments((const double*)ctx->sk->pb.p, ctx->dirs_p, run.lo, run.hi, nchan, (double*)ctx->sk->moments_part.p, mom,
                             pstream(ctx)) != hipSuccess)
      return false;
    const double c16 = 16.0 * run.kappa * (ctx->df / kC) * (ctx->df / kC);
    if (launch_split_flags(mom, nchan, (const double*)ctx->grp_hz.p, (const double*)ctx->grp_hz.p + ng, (const int32_t*)ctx->sk->lift_flags.p, (int)ng, c16,
                           2.0e-7, (int32_t*)ctx->sk->split_flags.p + r * ng, (int32_t*)ctx->sk->split_count.p + r, pstream(ctx)) != hipSuccess)
      return false;
  }
  // the counts travel to pinned host memory behind the flags kernels; get_timing reads them after the compute's events have completed
  if (hipMemcpyAsync(ctx->h_split_count, ctx->sk->split_count.p, 8 * sizeof(int32_t), hipMemcpyDeviceToHost, pstream(ctx)) != hipSuccess) return false;
  ctx->split_count_runs = (int)nruns;
  return true;
}

static hipError_t launch_family(const SkyvisParams& q, int family, const Plan& pl, hipStream_t stream) {
  switch (family) {
    case kFamRec: return launch_skyvis_rec(q, pl.f32, pl.ct, stream);
    case kFamPackedF32: return launch_skyvis_rec_f32pk(q, pl.ct, stream);
    case kFamPackedF32Split: return launch_skyvis_rec_f32pk_split(q, pl.ct, stream);
    case kFamTaperF64Block: case kFamTaperF64Wave: return launch_skyvis_taper_f64(q, pl.ct, stream);
  }
  return hipErrorInvalidValue;
}

// The source pieces of route rt's sky-sum (tail_plan.h).  Only one family cuts its last piece: packed fp32 without the taper and without
// a gradient, one launch over one set of complex64 partial cubes; everything else keeps the plan's pieces (ntail = 0).
static TailPieces route_tail(const prisim_ctx* ctx, const SkyShape& s, const SkyRoute& rt, int scale_comp) {
  const Plan& pl = rt.pl;
  const bool family = scale_comp < 0 && rt.family == kFamPackedF32 && !s.taper && rt.nlaunch == 1 && rt.launch[0].family == kFamPackedF32 &&
                      rt.launch[0].taper == 0 && rt.nsets == 1 && rt.part_f32 && pl.nsplit > 1;
  const SkyLaunch& l = rt.launch[0];
  return tail_pieces(pl.nsplit, l.src_per_split, pl.chunk, l.src_lo, l.src_hi, pl.ntiles, pl.nbgroups, 2 * (int64_t)std::max(ctx->cu_count, 1),
                     family ? ctx->tail_mode : kTailOff, s.tune_nsplit != 0 || s.tune_chunk != 0);
}

// The device tables of tail pieces tp: boundaries and per-XCD slab table, uploaded on the compute stream when the pieces or the grid
// are not those of the last upload (ctx_internal.h).  The sky-sums that read the old tables are ahead of the copy on the same stream.
static int tail_tables(prisim_ctx* ctx, const TailPieces& tp, const Plan& pl) {
  const int64_t key[9] = {tp.n, tp.ntail, tp.lo[0], tp.lo[1], tp.lo[tp.n - tp.ntail], tp.lo[tp.n - tp.ntail + 1], tp.lo[tp.n], pl.ntiles, pl.chunk};
  if (std::equal(key, key + 9, ctx->tail_key) && ctx->tail_lo.p && ctx->tail_tab.p) return PRISIM_OK;
  std::vector<int32_t> tab;
  const int per = tail_slab_table(tp.n, pl.ntiles, tab);
  const size_t lo_bytes = (size_t)(tp.n + 1) * sizeof(int64_t), tab_bytes = tab.size() * sizeof(int32_t);
  int rc;
  if ((rc = ensure(ctx, ctx->tail_lo, (size_t)(kTailMaxPieces + 1) * sizeof(int64_t))) || (rc = ensure_grow(ctx, ctx->tail_tab, tab_bytes))) return rc;
  if (!ctx->ev_tail) HIPCHK(ctx, hipEventCreateWithFlags(&ctx->ev_tail, hipEventDisableTiming));
  if (ctx->tail_pending) {      // the pinned area is free once the previous upload has read it
    HIPCHK(ctx, hipEventSynchronize(ctx->ev_tail));
    ctx->tail_pending = false;
  }
  const size_t need = 1024 + tab_bytes;      // boundaries in the first KiB, the table behind them
  if (need > ctx->h_tail_bytes) {
    if (ctx->h_tail) { (void)hipHostFree(ctx->h_tail); ctx->h_tail = nullptr; ctx->h_tail_bytes = 0; }
    if (hipHostMalloc(&ctx->h_tail, need + need / 4, hipHostMallocDefault) != hipSuccess) {
      ctx->h_tail = nullptr;
      return fail(ctx, PRISIM_ENOMEM, "hipHostMalloc for the tail-piece tables failed");
    }
    ctx->h_tail_bytes = need + need / 4;
  }
  static_assert((kTailMaxPieces + 1) * sizeof(int64_t) <= 1024, "the boundaries fit the first KiB of the pinned area");
  memcpy(ctx->h_tail, tp.lo, lo_bytes);
  memcpy((char*)ctx->h_tail + 1024, tab.data(), tab_bytes);
  ctx->tail_key[0] = -1;      // (a failed copy leaves no key behind)
  HIPCHK(ctx, hipMemcpyAsync(ctx->tail_lo.p, ctx->h_tail, lo_bytes, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(ctx->tail_tab.p, (char*)ctx->h_tail + 1024, tab_bytes, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipEventRecord(ctx->ev_tail, ctx->stream));
  ctx->tail_pending = true;
  ctx->tail_per_xcd = per;
  std::copy(key, key + 9, ctx->tail_key);
  return PRISIM_OK;
}

// One sky-sum pass into `dst` ([nbl_sum][nchan] complex128: the cube slot, or the compact buffer of a folded array) along route rt0
// (skyvis_plan.h; formed without the split form): rows in the route's layout, the split form's flags where it is eligible, then the
// route's launches.  scale_comp >= 0 multiplies pbflux rows by dircos[:,comp] (a gradient component: never the split form).
// post_set >= 0 (a deferred compute(), ctx_internal.h): the partial cubes are those of set post_set, and k_reduce_partials runs on the
// post stream behind the sky-sum's event ev_k1 (timed is then set).
static int run_pass(prisim_ctx* ctx, const SkyShape& s, const SkyToggles& t, const SkyRoute& rt0, double* dst, int scale_comp, bool timed,
                    bool prep = false, int post_set = -1) {
  DevBuf& part = post_set == 1 ? ctx->partial_b : ctx->partial;
  const Plan& pl = rt0.pl;
  SkyvisParams p{};
  sky_params(ctx, s, rt0, p);
  p.scale_comp = scale_comp;
  if (pl.kernel == PRISIM_KERNEL_DIRECT) {
    p.out = dst;
    if (prep) { int rcj = join_prep(ctx); if (rcj) return rcj; }
    if (timed) HIPCHK(ctx, hipEventRecord(ctx->ev_k0[ctx->ring_head], ctx->stream));
    HIPCHK(ctx, launch_skyvis_direct(p, (const double*)ctx->freqs.p, (const double*)ctx->sk->pb.p,
                                     scale_comp >= 0 ? ctx->dirs_p : nullptr, ctx->stream));
    if (timed) HIPCHK(ctx, hipEventRecord(ctx->ev_k1[ctx->ring_head], ctx->stream));
    return PRISIM_OK;
  }
  const int interleave = rt0.layout == kRowsNatural ? 0 : 1;
  if (prep && scale_comp < 0)      // the snapshot's first pass: rows and directions in one launch
    HIPCHK(ctx, launch_pack_prep((const double*)ctx->sk->pb.p, ctx->sk->packed.p, pl.f32, ctx->nsrc, pl.nsrc_pad, ctx->nchan, pl.ct, pl.ntiles,
                                 interleave, ctx->dirs_p, (double*)ctx->sk->dirs_prep.p, ctx->pc[0], ctx->pc[1], ctx->pc[2],
                                 1.0 / kC, pstream(ctx)));
  else
    HIPCHK(ctx, launch_pack((const double*)ctx->sk->pb.p, ctx->sk->packed.p, pl.f32, ctx->nsrc, pl.nsrc_pad, ctx->nchan, pl.ct,
                            pl.ntiles, ctx->dirs_p, scale_comp, interleave, ctx->stream));
  const bool split = scale_comp < 0 && split_eligible(s, t, pl, rt0.taper_group) && split_flags_prepare(ctx);
  const SkyRoute rt_split = split ? route(s, t, pl, false, true) : SkyRoute{};
  const SkyRoute& rt = split ? rt_split : rt0;
  if (prep) { int rcj = join_prep(ctx); if (rcj) return rcj; }      // rows, directions, flags are ready: the sums run on the compute stream
  p.out_f32 = rt.part_f32 ? 1 : 0;
  // tail pieces (tail_plan.h): the launch then writes tp.n partial cubes, piece by piece, and the reduction sums them in piece order
  const TailPieces tp = route_tail(ctx, s, rt, scale_comp);
  const int ncubes = tp.ntail > 0 ? tp.n : pl.nsplit * rt.nsets;
  if (tp.ntail > 0) {
    if (int rct = tail_tables(ctx, tp, pl)) return rct;
    p.tail_lo = (const int64_t*)ctx->tail_lo.p;
    p.tail_tab = (const int32_t*)ctx->tail_tab.p;
    p.tail_per_xcd = ctx->tail_per_xcd;
  }
  if (scale_comp < 0) {
    ctx->last_sum_pieces = pl.nsplit > 1 ? ncubes : 1;
    ctx->last_tail_pieces = tp.ntail;
  }
  const size_t set_reals = (size_t)pl.nsplit * (size_t)ctx->nbl_sum * (size_t)ctx->nchan * 2;       // reals of one run's partial cubes
  auto set_out = [&](int r) -> double* {
    if (pl.nsplit == 1) return dst;
    return rt.part_f32 ? (double*)((float*)part.p + (size_t)r * set_reals) : (double*)part.p + (size_t)r * set_reals;
  };
  auto cull_table = [&](int row) {
    return (const int32_t*)ctx->sk->cull_first.p + ((size_t)rt.cull_prec * ctx->cull_nruns + (size_t)row) * (size_t)pl.nbgroups;
  };
  ctx->timing.last_culled_fraction = rt.cull ? ctx->cull_frac[rt.cull_prec] : 0.0;
  ctx->cull_frac_pending = (rt.cull && ctx->cat.cur >= 0) ? rt.cull_prec + 1 : 0;      // catalogue path: the device's count is read once the events are in
  // (the post-pass that last read this set of partial cubes, two computes ago, has to be through before the sky-sum writes it)
  if (post_set >= 0 && ctx->post_rec[post_set]) HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_post[post_set], 0));
  if (timed) HIPCHK(ctx, hipEventRecord(ctx->ev_k0[ctx->ring_head], ctx->stream));
  for (int i = 0; i < rt.nlaunch; ++i) {
    const SkyLaunch& l = rt.launch[i];
    SkyvisParams q = p;
    q.src_lo = l.src_lo; q.src_hi = l.src_hi; q.src_per_split = l.src_per_split;
    q.accumulate = l.accumulate;
    q.out = set_out(l.out_set);
    q.kappa0 = l.kappa0;
    q.taper = l.taper;
    if (l.cull_row >= 0) q.src_first = cull_table(l.cull_row);
    if (l.flags_row >= 0) q.split_flags = (const int32_t*)ctx->sk->split_flags.p + (size_t)l.flags_row * (size_t)pl.nbgroups;
    if (l.wave_nbw > 0) { q.wave_nbw = l.wave_nbw; q.wave_nsplit = l.wave_nsplit; q.nsplit = 1; q.nbgroups = l.nbgroups; }
    if (l.repack_pairs)
      HIPCHK(ctx, launch_pack((const double*)ctx->sk->pb.p, ctx->sk->packed.p, false, ctx->nsrc, pl.nsrc_pad, ctx->nchan, pl.ct, pl.ntiles,
                              ctx->dirs_p, scale_comp, 1, ctx->stream, l.src_lo, l.src_hi));
    HIPCHK(ctx, launch_family(q, l.family, pl, ctx->stream));
  }
  if (split) ctx->timing.last_taper_split = rt.nlaunch;
  if (timed) HIPCHK(ctx, hipEventRecord(ctx->ev_k1[ctx->ring_head], ctx->stream));
  hipStream_t rs = ctx->stream;
  if (post_set >= 0) {
    rs = ctx->post_stream;
    HIPCHK(ctx, hipStreamWaitEvent(rs, ctx->ev_k1[ctx->ring_head], 0));
  }
  if (pl.nsplit > 1)
    HIPCHK(ctx, launch_reduce_partials(part.p, rt.part_f32, dst, ctx->nbl_sum * ctx->nchan * 2, ncubes, rs,
                                       post_set >= 0 ? (unsigned)ctx->post_blocks : 0u));
  return PRISIM_OK;
}

// V + the three baseline-gradient sums of one snapshot in one pass: dst [nbl_sum][nchan], gdst [3][nbl_sum][nchan] complex128.
// fp64: k_skyvis_grad_f64 (MFMA 4x4x4, groups of 64 baselines); fp32: the GRAD bodies of the packed kernel (16-channel tiles).
static int run_grad_pass(prisim_ctx* ctx, const SkyShape& s, const SkyRoute& rt, double* dst, double* gdst) {
  const Plan& pl = rt.pl;
  SkyvisParams p{};
  sky_params(ctx, s, rt, p);
  p.out = dst;
  p.grad_out = gdst;
  if (rt.layout == kRowsGrad) {
    // rows pre-multiplied by the gradient coefficients (1, l, m, n): 64 floats per (source, 16-channel tile)
    int rc2;
    if ((rc2 = ensure(ctx, ctx->sk->packed, (size_t)pl.ntiles * pl.nsrc_pad * 64 * sizeof(float)))) return rc2;
    p.pb_packed = ctx->sk->packed.p;
    HIPCHK(ctx, launch_pack_grad((const double*)ctx->sk->pb.p, (float*)ctx->sk->packed.p, ctx->nsrc, pl.nsrc_pad, ctx->nchan, pl.ntiles,
                                 ctx->dirs_p, pstream(ctx)));
  } else {
    HIPCHK(ctx, launch_pack((const double*)ctx->sk->pb.p, ctx->sk->packed.p, pl.f32, ctx->nsrc, pl.nsrc_pad, ctx->nchan, pl.ct, pl.ntiles,
                            ctx->dirs_p, -1, rt.layout == kRowsNatural ? 0 : 1, pstream(ctx)));
  }
  { int rcj = join_prep(ctx); if (rcj) return rcj; }
  HIPCHK(ctx, hipEventRecord(ctx->ev_k0[ctx->ring_head], ctx->stream));
  if (pl.f32) {
    p.dirs_c32 = (const float*)ctx->sk->dirs_c32.p;
    HIPCHK(ctx, launch_skyvis_grad_f32(p, ctx->stream));
  } else {
    p.nbgroups = rt.launch[0].nbgroups;
    HIPCHK(ctx, launch_skyvis_grad_f64(p, pl.ct, ctx->stream));
  }
  HIPCHK(ctx, hipEventRecord(ctx->ev_k1[ctx->ring_head], ctx->stream));
  return PRISIM_OK;
}

int prisim_hip_compute(prisim_ctx* ctx, int precision, int kernel, int want_grad, int64_t slot) {
  return guarded(ctx, [&]() -> int {
  if (!ctx) return PRISIM_EINVAL;
  if (!ctx->array_set || !ctx->sky_set) return fail(ctx, PRISIM_ESTATE, "set_array and set_sky must precede compute");
  if (precision != PRISIM_FP64 && precision != PRISIM_FP32) return fail(ctx, PRISIM_EINVAL, "unknown precision");
  if (kernel < PRISIM_KERNEL_AUTO || kernel > PRISIM_KERNEL_DIRECT) return fail(ctx, PRISIM_EINVAL, "unknown kernel id");
  if (slot < 0 || slot >= ctx->nt_max) return fail(ctx, PRISIM_EINVAL, "slot out of range");
  if (kernel == PRISIM_KERNEL_RECURRENCE && !ctx->uniform)
    return fail(ctx, PRISIM_EINVAL, "recurrence kernel needs a uniform channel grid");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  // Deferred post-pass (ctx_internal.h): a folded array, a source split, the recurrence kernel, no gradient.  The plan decides the rest
  // below; every compute() that cannot be deferred joins the post stream before it enqueues anything.
  bool defer = ctx->defer_post && ctx->post_stream && ctx->folded && !want_grad && ctx->nsrc > 0;
  int rc;
  if (!defer && (rc = join_post(ctx))) return rc;
  harvest_timing(ctx, /*max_wait=*/ctx->ring_pending >= prisim_ctx::kTimingRing ? 1 : 0);   // a full ring waits for its oldest entry only
  const size_t slot_elems = (size_t)ctx->nbl * ctx->nchan * 2;
  double* dst = (double*)ctx->cube.p + (size_t)slot * slot_elems;
  if (want_grad) {
    const size_t gbytes = (size_t)ctx->nt_max * 3 * slot_elems * sizeof(double);
    if (!ctx->grad.p) {
      if ((rc = ensure(ctx, ctx->grad, gbytes))) return rc;
      HIPCHK(ctx, hipMemsetAsync(ctx->grad.p, 0, gbytes, ctx->stream));
    }
  }
  if (ctx->nsrc == 0) {   // interferometry.py:6378-6382: visibilities stay zero
    HIPCHK(ctx, hipMemsetAsync(dst, 0, slot_elems * sizeof(double), ctx->stream));
    if (want_grad)
      HIPCHK(ctx, hipMemsetAsync((double*)ctx->grad.p + (size_t)slot * 3 * slot_elems, 0, 3 * slot_elems * sizeof(double), ctx->stream));
    ctx->timing.last_terms = 0;
    ctx->last_sum_baselines = ctx->nbl_sum; ctx->last_terms_evaluated = 0;
    catalog_after_compute(ctx);      // (an empty region of interest still releases the catalogue's buffer set in stream order)
    return PRISIM_OK;
  }
  // A folded array (set_array): everything below sums the nbl_sum distinct vectors into the compact buffers, and k_expand_rows copies
  // compact row fold_map[b] into row b of the slot (and of its gradient block) at the end.
  const size_t sum_elems = (size_t)ctx->nbl_sum * ctx->nchan * 2;
  double* const slot_dst = dst;
  if (ctx->folded) {
    dst = (double*)ctx->fold_vis.p;
    if (want_grad && (rc = ensure(ctx, ctx->fold_grad, 3 * sum_elems * sizeof(double)))) return rc;
  }
  double* const gbase = !want_grad ? nullptr : ctx->folded ? (double*)ctx->fold_grad.p : (double*)ctx->grad.p + (size_t)slot * 3 * slot_elems;
  // The plan and the route of this sky-sum (skyvis_plan.h), formed without the packed taper's split form: run_pass takes that up once
  // its device flags are prepared, and nothing used before then depends on it.
  const SkyToggles tog = read_sky_toggles();
  SkyShape shape = sky_shape(ctx, tog);
  const SkyRoute rt = route(shape, tog, make_plan(shape, tog, precision, kernel), want_grad != 0, /*split_ready=*/false);
  const Plan& pl = rt.pl;
  const bool fused_grad = want_grad && rt.family != kFamGradFourPass;
  if (defer && !rt.may_defer) {      // (nothing of this compute() is enqueued yet)
    defer = false;
    if ((rc = join_post(ctx))) return rc;
  }
  const int post_set = defer ? ctx->part_next : -1;
  ctx->timing.last_lift_groups = 0;
  ctx->last_sum_lift_groups = 0;
  ctx->last_sum_wide_groups = 0;
  ctx->timing.last_taper_group = 0;
  ctx->timing.last_taper_split = 0;
  ctx->timing.last_split_uncorrected_groups = 0;
  ctx->timing.last_culled_fraction = 0.0;
  ctx->timing.last_batch_snapshots = 1;
  ctx->last_sum_pieces = 1;
  ctx->last_tail_pieces = 0;
  if (pl.kernel == PRISIM_KERNEL_RECURRENCE) {
    const size_t pbytes = (size_t)pl.ntiles * pl.nsrc_pad * pl.ct * (pl.f32 ? 4 : 8);
    if ((rc = ensure(ctx, ctx->sk->packed, pbytes))) return rc;
    if ((rc = ensure(ctx, ctx->sk->dirs_prep, (size_t)pl.nsrc_pad * 4 * sizeof(double)))) return rc;
    // (tail pieces: the one family that takes them writes tp.n complex64 cubes into one set)
    const size_t part_cubes = std::max((size_t)rt.alloc_sets * (size_t)pl.nsplit, (size_t)route_tail(ctx, shape, rt, -1).n);
    if (pl.nsplit > 1 && (rc = ensure(ctx, post_set == 1 ? ctx->partial_b : ctx->partial, part_cubes * sum_elems * sizeof(double))))
      return rc;
    {
      // lifting rotation is used for a baseline group only when |step phase| <= 1/8 cycle (fp32; 1/4 cycle in fp64, where the
      // angle error alpha*eps is irrelevant and only tan(alpha/2) must stay bounded) is guaranteed for every source:
      // |theta| = |b . (s - s_pc)| |df| / c <= min(max|b| max_s|e|, max|b_xy| max_s|e_xy| + max|b_z| max_s|e_z|) |df| / c, e = s - s_pc
      // (step_bound.h: the per-axis form does not charge a horizontal baseline for the vertical part of e)
      const double adf = std::fabs(ctx->df);
      const double k = ctx->dmax * adf / kC;
      const double lift_limit = prisim::step_limit_cycles(pl.f32);
      const double key[3] = {ctx->dmax * adf, ctx->hmax * adf, ctx->zmax * adf};
      const size_t ng = ctx->grp_maxlen.size();
      if ((size_t)pl.nbgroups != ng) return fail(ctx, PRISIM_EINTERNAL, "the plan's baseline groups are not those of the group tables");
      if (key[0] != ctx->sk->lift_key_k[0] || key[1] != ctx->sk->lift_key_k[1] || key[2] != ctx->sk->lift_key_k[2] ||
          (int)pl.f32 != ctx->sk->lift_key_f32 || ctx->sk->lift_groups != pl.nbgroups) {
        // formed on the device from the groups' tables (resident since set_array): the extrema of s - s_pc change with every snapshot
        // of a drift scan, and a host-side table would need a stream synchronisation before it could be rewritten
        if ((rc = ensure(ctx, ctx->sk->lift_flags, (size_t)pl.nbgroups * sizeof(int32_t)))) return rc;
        HIPCHK(ctx, launch_lift_flags((const double*)ctx->grp_hz.p, pl.nbgroups, ctx->dmax, ctx->hmax, ctx->zmax, adf, lift_limit,
                                      (int32_t*)ctx->sk->lift_flags.p, pstream(ctx)));
        if (pl.f32) {
          // the wide tier's table (fp32 only): the same kernel under the wide limit; the hook off = a limit no step meets = all zero
          if ((rc = ensure(ctx, ctx->sk->wide_flags, (size_t)pl.nbgroups * sizeof(int32_t)))) return rc;
          HIPCHK(ctx, launch_lift_flags((const double*)ctx->grp_hz.p, pl.nbgroups, ctx->dmax, ctx->hmax, ctx->zmax, adf,
                                        ctx->wide_leapfrog ? prisim::step_wide_limit_cycles() : -1.0, (int32_t*)ctx->sk->wide_flags.p, pstream(ctx)));
        }
        for (int i = 0; i < 3; ++i) ctx->sk->lift_key_k[i] = key[i];
        ctx->sk->lift_key_f32 = (int)pl.f32;
        ctx->sk->lift_groups = pl.nbgroups;
      }
      // last_sum_lift_groups (prisim_hip_get_fold_info) is the kernel's own flag count: the groups of 256 SUMMED rows (the rows
      // themselves on an unfolded array) that pass step_bound.h's rule, formed here as the device forms its flags.
      // last_lift_groups stays the length-rule count per group of 256 CUBE rows (the caller's units): the groups whose longest baseline
      // passes max|b| max_s|e| alone.  It is a lower bound of what lifts on an unfolded array; on a folded one a cube row within the
      // limit whose vector shares a summed group with a longer one runs the plain rotation, which is valid for every step angle.
      // last_sum_wide_groups (prisim_hip_get_step_tiers): the groups of tier 2, where the kernel that reads the wide table runs -- the
      // packed fp32 kernel without the taper, not the fused gradient.
      int nlift = 0, nlift_sum = 0, nwide_sum = 0;
      for (double len : ctx->row_grp_maxlen) nlift += (len * k <= lift_limit) ? 1 : 0;
      for (size_t g = 0; g < ng; ++g) {
        const int tier = prisim::step_tier(ctx->grp_maxlen[g], ctx->grp_maxh[g], ctx->grp_maxz[g], ctx->dmax, ctx->hmax, ctx->zmax, ctx->df, pl.f32);
        nlift_sum += tier == 1 ? 1 : 0;
        nwide_sum += tier == 2 ? 1 : 0;
      }
      ctx->timing.last_lift_groups = rt.zero_lift_counts ? 0 : nlift;
      ctx->last_sum_lift_groups = rt.zero_lift_counts ? 0 : nlift_sum;
      ctx->last_sum_wide_groups = (ctx->wide_leapfrog && rt.sum_family == kFamPackedF32 && !ctx->taper && !fused_grad) ? nwide_sum : 0;
      shape.have_lift_flags = ctx->sk->lift_flags.p != nullptr;      // (formed above, now or by an earlier compute() of this sky-buffer set)
    }
    if (pl.f32 && ctx->taper) {
      if ((rc = ensure(ctx, ctx->fsq_pairs, (size_t)pl.ntiles * pl.ct * sizeof(float)))) return rc;
      if (ctx->fsq_pairs_ct != pl.ct || ctx->fsq_pairs_ntiles != pl.ntiles) {      // (a function of the tiling only: once per plan)
        HIPCHK(ctx, launch_fsq_pairs((const float*)ctx->fsq.p, (float*)ctx->fsq_pairs.p, pl.ct, pl.ntiles, ctx->stream));
        ctx->fsq_pairs_ct = pl.ct; ctx->fsq_pairs_ntiles = pl.ntiles;
      }
    }
  }
  HIPCHK(ctx, hipEventRecord(ctx->ev_c0[ctx->ring_head], ctx->stream));
  if (pl.kernel == PRISIM_KERNEL_RECURRENCE && fused_grad) {
    float* c32 = nullptr;
    if (pl.f32) {
      if ((rc = ensure(ctx, ctx->sk->dirs_c32, (size_t)pl.nsrc_pad * 8 * sizeof(float)))) return rc;
      c32 = (float*)ctx->sk->dirs_c32.p;
    }
    HIPCHK(ctx, launch_prep_dirs(ctx->dirs_p, (double*)ctx->sk->dirs_prep.p, c32, ctx->nsrc, pl.nsrc_pad, ctx->pc[0],
                                 ctx->pc[1], ctx->pc[2], 1.0 / kC, pstream(ctx)));
  }
  // (a deferred compute() that fails half-way leaves no post-pass behind that nobody would wait for: the post stream is drained)
  auto post_abort = [&](int code) { if (defer) (void)hipStreamSynchronize(ctx->post_stream); return code; };
  if (fused_grad) {
    if ((rc = run_grad_pass(ctx, shape, rt, dst, gbase))) return rc;
  } else if ((rc = run_pass(ctx, shape, tog, rt, dst, -1, true, /*prep=*/true, post_set))) {      // (prepares the directions with its first launch)
    return post_abort(rc);
  }
  if (want_grad && !fused_grad) {
    for (int comp = 0; comp < 3; ++comp) {
      double* gdst = gbase + (size_t)comp * sum_elems;
      if ((rc = run_pass(ctx, shape, tog, rt, gdst, comp, false))) return rc;
    }
  }
  // the stream the compute() ends on: deferred, the post stream -- run_pass has queued the reduction there behind the sky-sum, and the
  // expansion and ev_c1 follow it, so that last_compute_ms still spans the expansion
  const hipStream_t end_stream = defer ? ctx->post_stream : ctx->stream;
  if (ctx->folded) {      // inside last_compute_ms; last_kernel_ms stays the sky-sum alone
    if (launch_expand_rows(dst, gbase, (const int32_t*)ctx->fold_map.p, slot_dst,
                           want_grad ? (double*)ctx->grad.p + (size_t)slot * 3 * slot_elems : nullptr, ctx->nbl, ctx->nbl_sum, ctx->nchan,
                           end_stream, defer ? (unsigned)ctx->post_blocks : 0u) != hipSuccess)
      return post_abort(fail(ctx, PRISIM_ENODEV, "launch of k_expand_rows failed"));
  }
  if (hipEventRecord(ctx->ev_c1[ctx->ring_head], end_stream) != hipSuccess)
    return post_abort(fail(ctx, PRISIM_ENODEV, "hipEventRecord(end of compute) failed"));
  if (defer) {
    if (hipEventRecord(ctx->ev_post[post_set], ctx->post_stream) != hipSuccess)
      return post_abort(fail(ctx, PRISIM_ENODEV, "hipEventRecord(deferred post-pass) failed"));
    ctx->post_rec[post_set] = true;
    ctx->post_last = post_set;
    ctx->part_next = post_set ^ 1;
  }
  if (ctx->prep_async) {
    HIPCHK(ctx, hipEventRecord(ctx->sk->ev_sum, ctx->stream));
    ctx->sk->sum_recorded = true;
  }
  catalog_after_compute(ctx);
  ctx->ring_head = (ctx->ring_head + 1) % prisim_ctx::kTimingRing;
  ctx->ring_pending += 1;
  ctx->timing.last_terms = ctx->nbl * ctx->nchan * ctx->nsrc;          // delivered; the kernels evaluated nbl_sum rows of them
  ctx->last_sum_baselines = ctx->nbl_sum;
  ctx->last_terms_evaluated = ctx->nbl_sum * ctx->nchan * ctx->nsrc;
  ctx->timing.last_kernel_id = pl.kernel;
  ctx->timing.last_chan_tile = pl.kernel == PRISIM_KERNEL_RECURRENCE ? pl.ct : 1;
  ctx->timing.last_nsplit = pl.kernel == PRISIM_KERNEL_RECURRENCE ? pl.nsplit : 1;
  return PRISIM_OK;
  }, /*join=*/false);
}

static void to_c64(const double* in, float* out, size_t n2) {
  for (size_t i = 0; i < n2; ++i) out[i] = (float)in[i];
}

int prisim_hip_get_vis(prisim_ctx* ctx, int64_t slot, void* vis, void* grad, int out_is_c64) {
  return guarded(ctx, [&]() -> int {
  if (!ctx) return PRISIM_EINVAL;
  if (!ctx->array_set) return fail(ctx, PRISIM_ESTATE, "set_array has not been called");
  if (slot < 0 || slot >= ctx->nt_max) return fail(ctx, PRISIM_EINVAL, "slot out of range");
  if (!vis) return fail(ctx, PRISIM_EINVAL, "vis is NULL");
  if (grad && !ctx->grad.p) return fail(ctx, PRISIM_ESTATE, "no gradient has been computed");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  harvest_timing(ctx);
  const size_t slot_elems = (size_t)ctx->nbl * ctx->nchan * 2;
  const double* src = (const double*)ctx->cube.p + (size_t)slot * slot_elems;
  const double* gsrc = grad ? (const double*)ctx->grad.p + (size_t)slot * 3 * slot_elems : nullptr;
  if (!out_is_c64) {
    HIPCHK(ctx, hipMemcpy(vis, src, slot_elems * sizeof(double), hipMemcpyDeviceToHost));
    if (grad) HIPCHK(ctx, hipMemcpy(grad, gsrc, 3 * slot_elems * sizeof(double), hipMemcpyDeviceToHost));
  } else {
    std::vector<double> tmp;
    try { tmp.resize(grad ? 3 * slot_elems : slot_elems); } catch (...) { return fail(ctx, PRISIM_ENOMEM, "host staging"); }
    HIPCHK(ctx, hipMemcpy(tmp.data(), src, slot_elems * sizeof(double), hipMemcpyDeviceToHost));
    to_c64(tmp.data(), (float*)vis, slot_elems);
    if (grad) {
      HIPCHK(ctx, hipMemcpy(tmp.data(), gsrc, 3 * slot_elems * sizeof(double), hipMemcpyDeviceToHost));
      to_c64(tmp.data(), (float*)grad, 3 * slot_elems);
    }
  }
  return PRISIM_OK;
  });
}

int prisim_hip_set_vis(prisim_ctx* ctx, int64_t slot, const double* vis) {
  return guarded(ctx, [&]() -> int {
  if (!ctx) return PRISIM_EINVAL;
  if (!ctx->array_set) return fail(ctx, PRISIM_ESTATE, "set_array has not been called");
  if (slot < 0 || slot >= ctx->nt_max) return fail(ctx, PRISIM_EINVAL, "slot out of range");
  if (!vis) return fail(ctx, PRISIM_EINVAL, "vis is NULL");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const size_t slot_elems = (size_t)ctx->nbl * ctx->nchan * 2;
  HIPCHK(ctx, hipMemcpyAsync((double*)ctx->cube.p + (size_t)slot * slot_elems, vis, slot_elems * sizeof(double),
                             hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return PRISIM_OK;
  });
}

int prisim_hip_skyvis(prisim_ctx* ctx, const prisim_sky* sky, int precision, int kernel, void* vis, void* grad,
                      int out_is_c64) {
  return guarded(ctx, [&]() -> int {
  int rc = prisim_hip_set_sky(ctx, sky);
  if (rc) return rc;
  if ((rc = prisim_hip_compute(ctx, precision, kernel, grad != nullptr, 0))) return rc;
  return prisim_hip_get_vis(ctx, 0, vis, grad, out_is_c64);
  });
}

int prisim_hip_sync(prisim_ctx* ctx) {
  return guarded(ctx, [&]() -> int {
  if (!ctx) return PRISIM_EINVAL;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (ctx->prep_stream) HIPCHK(ctx, hipStreamSynchronize(ctx->prep_stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  if (ctx->post_stream) HIPCHK(ctx, hipStreamSynchronize(ctx->post_stream));
  if (ctx->comm_stream && ctx->comm_pending) { HIPCHK(ctx, hipStreamSynchronize(ctx->comm_stream)); ctx->comm_pending = false; }
  if (ctx->copy_stream && ctx->copy_pending) { HIPCHK(ctx, hipStreamSynchronize(ctx->copy_stream)); ctx->copy_pending = false; }
  harvest_timing(ctx);
  harvest_comm(ctx, true);
  return PRISIM_OK;
  });
}

int prisim_hip_get_timing(prisim_ctx* ctx, prisim_timing* out, int reset) {
  return guarded(ctx, [&]() -> int {
  if (!ctx) return PRISIM_EINVAL;
  if (!out) return fail(ctx, PRISIM_EINVAL, "out is NULL");
  if (ctx->ring_pending > 0) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    harvest_timing(ctx);
  }
  if (ctx->ev_d1 && ctx->timing.last_delay_ms < 0.0) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    float ms = 0.f;
    if (hipEventSynchronize(ctx->ev_d1) == hipSuccess && hipEventElapsedTime(&ms, ctx->ev_d0, ctx->ev_d1) == hipSuccess)
      ctx->timing.last_delay_ms = ms;
  }
  if (ctx->cull_frac_pending && ctx->cat.culled_host && ctx->ring_pending == 0) {
    // (catalogue path: the cull table was built on the device; its count copy was queued before the compute whose events are now in)
    const int pr = ctx->cull_frac_pending - 1;
    const double pairs = (double)ctx->nsrc * (double)ctx->nbl;
    ctx->cull_frac[pr] = pairs > 0.0 ? (double)ctx->cat.culled_host[pr] / pairs : 0.0;
    ctx->timing.last_culled_fraction = ctx->cull_frac[pr];
    ctx->cull_frac_pending = 0;
  }
  if (ctx->timing.last_taper_split > 0 && ctx->h_split_count && ctx->ring_pending == 0) {
    // (every compute's events have completed: the count copy queued before them has landed)
    int n = 0;
    for (int r = 0; r < ctx->split_count_runs && r < 8; ++r) n += ctx->h_split_count[r];
    ctx->timing.last_split_uncorrected_groups = n;
  }
  *out = ctx->timing;
  if (reset) { ctx->timing.sum_kernel_ms = 0.0; ctx->timing.n_kernel = 0; }
  return PRISIM_OK;
  });
}

int prisim_hip_get_fold_info(prisim_ctx* ctx, int64_t* last_sum_baselines, int64_t* last_terms_evaluated, int64_t* last_sum_lift_groups) {
  return guarded(ctx, [&]() -> int {
  if (!ctx) return PRISIM_EINVAL;
  if (last_sum_baselines) *last_sum_baselines = ctx->last_sum_baselines;
  if (last_terms_evaluated) *last_terms_evaluated = ctx->last_terms_evaluated;
  if (last_sum_lift_groups) *last_sum_lift_groups = ctx->last_sum_lift_groups;
  return PRISIM_OK;
  });
}

int prisim_hip_get_fold_near(prisim_ctx* ctx, int64_t* exact_baselines, int64_t* near_baselines, double* max_dev_m, double* phase_bound_rad, int* used) {
  return guarded(ctx, [&]() -> int {
  if (!ctx) return PRISIM_EINVAL;
  if (exact_baselines) *exact_baselines = ctx->fold_exact_nbl;
  if (near_baselines) *near_baselines = ctx->fold_near_nbl;
  if (max_dev_m) *max_dev_m = ctx->fold_near_max_dev;
  if (phase_bound_rad) *phase_bound_rad = ctx->fold_near_phase;
  if (used) *used = ctx->fold_near_used ? 1 : 0;
  return PRISIM_OK;
  });
}

int prisim_hip_get_step_tiers(prisim_ctx* ctx, int64_t* last_sum_wide_groups, double* wide_limit_cycles) {
  return guarded(ctx, [&]() -> int {
  if (!ctx) return PRISIM_EINVAL;
  if (last_sum_wide_groups) *last_sum_wide_groups = ctx->last_sum_wide_groups;
  if (wide_limit_cycles) *wide_limit_cycles = prisim::step_wide_limit_cycles();
  return PRISIM_OK;
  });
}

int prisim_hip_get_tail_pieces(prisim_ctx* ctx, int64_t* pieces, int64_t* tail_pieces) {
  return guarded(ctx, [&]() -> int {
  if (!ctx) return PRISIM_EINVAL;
  if (pieces) *pieces = ctx->last_sum_pieces;
  if (tail_pieces) *tail_pieces = ctx->last_tail_pieces;
  return PRISIM_OK;
  });
}

int prisim_hip_device_info(prisim_ctx* ctx, int* cu_count, int* clock_khz, char name[64]) {
  return guarded(ctx, [&]() -> int {
  if (!ctx) return PRISIM_EINVAL;
  if (cu_count) *cu_count = ctx->cu_count;
  if (clock_khz) *clock_khz = ctx->clock_khz;
  if (name) { memcpy(name, ctx->devname, 64); name[63] = 0; }
  return PRISIM_OK;
  });
}

int prisim_hip_set_tuning(prisim_ctx* ctx, int chan_tile, int src_chunk, int nsplit) {
  return guarded(ctx, [&]() -> int {
  if (!ctx) return PRISIM_EINVAL;
  if (chan_tile != 0 && chan_tile != 8 && chan_tile != 16 && chan_tile != 32 && chan_tile != 64)
    return fail(ctx, PRISIM_EINVAL, "chan_tile must be 0, 8, 16, 32 or 64");
  if (src_chunk < 0 || src_chunk > 256 || nsplit < 0 || nsplit > 4096)
    return fail(ctx, PRISIM_EINVAL, "src_chunk must be in [0,256], nsplit in [0,4096]");
  ctx->tune_ct = chan_tile; ctx->tune_chunk = src_chunk; ctx->tune_nsplit = nsplit;
  return PRISIM_OK;
  });
}

// ---- delay transform ------------------------------------------------------------------------

namespace {

struct DelayGeom {
  int64_t npad, nfft, nout;
  double factor;
  bool fused;          // integer 1 + pad and a power-of-two channel count: one LDS kernel, no padding, no rocFFT
};

DelayGeom delay_geom(const prisim_ctx* ctx, double pad) {
  DelayGeom g{};
  const int64_t nchan = ctx->nchan;
  g.npad = (int64_t)((double)nchan * pad);                                // :8123
  g.nfft = nchan + g.npad;
  g.factor = 1.0 + pad;                                                   // :8131
  g.nout = (int64_t)std::ceil((double)g.nfft / g.factor - 1e-12);         // len(arange(0, nfft, factor))
  const double fr = std::round(g.factor);
  g.fused = delay_fft_supported(nchan) && std::fabs(g.factor - fr) == 0.0 && fr >= 1.0 && g.nfft == nchan * (int64_t)fr && g.nout == nchan;
  if (const char* env = getenv("PRISIM_HIP_DT_FUSED")) g.fused = g.fused && atoi(env) != 0;      // A/B hook
  return g;
}

// Upload the window [nbl][nchan] (or none) and make sure the fused kernel's twiddle table / the rocFFT plan exist.
int delay_prepare(prisim_ctx* ctx, const DelayGeom& g, const double* bpwts, int64_t wts_rows, int64_t nrows_batch) {
  int rc;
  const int64_t nchan = ctx->nchan, nbl = ctx->nbl;
  if (bpwts) {
    if (wts_rows != 1 && wts_rows != nbl) return fail(ctx, PRISIM_EINVAL, "wts_rows must be 1 or nbl");
    if ((rc = ensure(ctx, ctx->dt_wts, (size_t)wts_rows * nchan * sizeof(double)))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(ctx->dt_wts.p, bpwts, (size_t)wts_rows * nchan * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));     // bpwts is caller-owned
  }
  if (g.fused) {
    if (ctx->dt_tw_n != nchan) {
      std::vector<double> tw((size_t)nchan);            // nchan / 2 complex values W_N^m = exp(+2 pi i m / N)
      for (int64_t m = 0; m < nchan / 2; ++m) {
        const double a = 2.0 * M_PI * (double)m / (double)nchan;
        tw[(size_t)2 * m] = std::cos(a);
        tw[(size_t)2 * m + 1] = std::sin(a);
      }
      if ((rc = ensure(ctx, ctx->dt_tw, tw.size() * sizeof(double)))) return rc;
      HIPCHK(ctx, hipMemcpy(ctx->dt_tw.p, tw.data(), tw.size() * sizeof(double), hipMemcpyHostToDevice));
      ctx->dt_tw_n = nchan;
    }
    return PRISIM_OK;
  }
  std::string lerr;
  if (!load_rocfft(lerr)) return fail(ctx, PRISIM_ELIB, lerr);
  RocfftApi& F = g_rocfft;
  if (!F.setup_done) {
    if (F.setup() != rocfft_status_success) return fail(ctx, PRISIM_ELIB, "rocfft_setup failed");
    F.setup_done = true;
  }
  if ((rc = ensure(ctx, ctx->fft_buf, (size_t)nrows_batch * g.nfft * 2 * sizeof(double)))) return rc;
  return PRISIM_OK;
}

// Transform `nrows` = ntc * nbl rows starting at snapshot slot t0 into the device buffers d_out ([nrows][nout] complex128) and/or
// d_pow ([nrows][nout] float64).  Asynchronous on the context stream.
int delay_batch(prisim_ctx* ctx, const DelayGeom& g, int64_t t0, int64_t nrows, bool have_wts, int64_t wts_rows, double* d_out, double* d_pow,
                double power_scale) {
  const int64_t nchan = ctx->nchan, nbl = ctx->nbl;
  const size_t slot_elems = (size_t)nbl * nchan * 2;
  const double* src = (const double*)ctx->cube.p + (size_t)t0 * slot_elems;
  const double* wts = have_wts ? (const double*)ctx->dt_wts.p : nullptr;
  // rocFFT's inverse is unnormalised: sum_n x[n] e^{+2 pi i k n / N'}.  The reference forms ifft(x) * N' * df (:8125) = that sum times df.
  const double scale = ctx->df;
  if (g.fused) {
    HIPCHK(ctx, launch_delay_fft(src, wts, wts_rows, (const double*)ctx->dt_tw.p, d_out, d_pow, nrows, nbl, nchan, scale, power_scale,
                                 ctx->cu_count, ctx->stream));
    return PRISIM_OK;
  }
  RocfftApi& F = g_rocfft;
  int rc;
  if (!ctx->fft_plan || ctx->fft_len != (size_t)g.nfft || ctx->fft_batch != (size_t)nrows) {
    if (ctx->fft_plan) { F.plan_destroy(ctx->fft_plan); ctx->fft_plan = nullptr; }
    size_t len = (size_t)g.nfft;
    if (F.plan_create(&ctx->fft_plan, rocfft_placement_inplace, rocfft_transform_type_complex_inverse,
                      rocfft_precision_double, 1, &len, (size_t)nrows, nullptr) != rocfft_status_success) {
      ctx->fft_plan = nullptr;
      return fail(ctx, PRISIM_ELIB, "rocfft_plan_create failed");
    }
    ctx->fft_len = (size_t)g.nfft; ctx->fft_batch = (size_t)nrows;
    if (!ctx->fft_info && F.execution_info_create(&ctx->fft_info) != rocfft_status_success)
      return fail(ctx, PRISIM_ELIB, "rocfft_execution_info_create failed");
    if (F.execution_info_set_stream(ctx->fft_info, ctx->stream) != rocfft_status_success)
      return fail(ctx, PRISIM_ELIB, "rocfft_execution_info_set_stream failed");
    size_t wbytes = 0;
    F.plan_get_work_buffer_size(ctx->fft_plan, &wbytes);
    if (wbytes) {
      if ((rc = ensure(ctx, ctx->fft_work, wbytes))) return rc;
      if (F.execution_info_set_work_buffer(ctx->fft_info, ctx->fft_work.p, wbytes) != rocfft_status_success)
        return fail(ctx, PRISIM_ELIB, "rocfft_execution_info_set_work_buffer failed");
    }
  }
  HIPCHK(ctx, launch_dt_prepare(src, wts, wts_rows, (double*)ctx->fft_buf.p, nrows, nbl, nchan, g.nfft, ctx->stream));
  void* bufs[1] = {ctx->fft_buf.p};
  if (F.execute(ctx->fft_plan, bufs, nullptr, ctx->fft_info) != rocfft_status_success)
    return fail(ctx, PRISIM_ELIB, "rocfft_execute failed");
  HIPCHK(ctx, launch_dt_finish((const double*)ctx->fft_buf.p, d_out, d_pow, nrows, g.nfft, g.nout, g.factor, scale, power_scale, ctx->stream));
  return PRISIM_OK;
}

// snapshots per batch of the rocFFT pipeline so that its padded work buffer stays <= 4 GiB whatever nt is
// (config 5: 120 x 61075 rows of 2048 would be 240 GB at once); the fused kernel needs no work buffer
int64_t delay_batch_snapshots(const prisim_ctx* ctx, const DelayGeom& g, int64_t nt) {
  if (g.fused && !getenv("PRISIM_HIP_DT_BATCH_BYTES")) return nt;
  const int64_t row_bytes = g.nfft * 2 * (int64_t)sizeof(double);
  int64_t budget = (int64_t)4 << 30;
  if (const char* env = getenv("PRISIM_HIP_DT_BATCH_BYTES")) {   // test hook: force several batches on small cubes
    const long long v = atoll(env);
    if (v > 0) budget = v;
  }
  int64_t nt_b = std::max<int64_t>(1, budget / (ctx->nbl * row_bytes));
  return std::min(nt_b, nt);
}

void delay_lags(const prisim_ctx* ctx, double* lags_out) {
  // DSP.spectral_axis(nchan, delx=df, shift=True) (:8114) == fftshift(fftfreq(nchan, df))
  for (int64_t i = 0; i < ctx->nchan; ++i) {
    const int64_t k = i - ctx->nchan / 2;
    lags_out[i] = (double)k / ((double)ctx->nchan * ctx->df);
  }
}

int delay_check(prisim_ctx* ctx, int64_t nt, double& pad) {
  if (!ctx->array_set) return fail(ctx, PRISIM_ESTATE, "set_array has not been called");
  if (nt <= 0 || nt > ctx->nt_max) return fail(ctx, PRISIM_EINVAL, "nt out of range");
  if (!(pad >= 0.0) || !std::isfinite(pad)) pad = 0.0;   // interferometry.py:8091-8092
  if (!ctx->uniform || ctx->nchan < 2) return fail(ctx, PRISIM_EINVAL, "delay transform needs >= 2 uniformly spaced channels");
  return PRISIM_OK;
}

}  // namespace

int prisim_hip_delay_transform(prisim_ctx* ctx, int64_t nt, const double* bpwts, double pad, double* out,
                               double* lags_out, double* out_power, double power_scale) {
  return guarded(ctx, [&]() -> int {
  if (!ctx) return PRISIM_EINVAL;
  int rc;
  if ((rc = delay_check(ctx, nt, pad))) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const DelayGeom g = delay_geom(ctx, pad);
  const int64_t nbl = ctx->nbl, nout = g.nout;
  // the host-output form always goes batch by batch through two staging buffers
  int64_t nt_b = delay_batch_snapshots(ctx, g, nt);
  if (g.fused) nt_b = std::min<int64_t>(nt, std::max<int64_t>(1, ((int64_t)2 << 30) / (nbl * nout * 16)));
  if ((rc = delay_prepare(ctx, g, bpwts, nbl, nt_b * nbl))) return rc;
  if (out && (rc = ensure(ctx, ctx->dt_out, (size_t)(nt_b * nbl) * nout * 2 * sizeof(double)))) return rc;
  if (out_power && (rc = ensure(ctx, ctx->dt_pow, (size_t)(nt_b * nbl) * nout * sizeof(double)))) return rc;
  for (int64_t t0 = 0; t0 < nt; t0 += nt_b) {
    const int64_t ntc = std::min(nt_b, nt - t0);
    const int64_t nrows = ntc * nbl;
    if ((rc = delay_batch(ctx, g, t0, nrows, bpwts != nullptr, nbl, out ? (double*)ctx->dt_out.p : nullptr,
                          out_power ? (double*)ctx->dt_pow.p : nullptr, power_scale)))
      return rc;
    if (out)
      HIPCHK(ctx, hipMemcpyAsync(out + (size_t)t0 * nbl * nout * 2, ctx->dt_out.p, (size_t)nrows * nout * 2 * sizeof(double),
                                 hipMemcpyDeviceToHost, ctx->stream));
    if (out_power)
      HIPCHK(ctx, hipMemcpyAsync(out_power + (size_t)t0 * nbl * nout, ctx->dt_pow.p, (size_t)nrows * nout * sizeof(double),
                                 hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));     // the staging buffers are reused by the next batch
  }
  if (lags_out) delay_lags(ctx, lags_out);
  return PRISIM_OK;
  });
}

int prisim_hip_delay_transform_device(prisim_ctx* ctx, int64_t nt, const double* bpwts, int64_t wts_rows, double pad, int want_lag, int want_power,
                                      double power_scale, double* lags_out, int64_t* nout_out) {
  return guarded(ctx, [&]() -> int {
  if (!ctx) return PRISIM_EINVAL;
  int rc;
  if ((rc = delay_check(ctx, nt, pad))) return rc;
  if (!want_lag && !want_power) return fail(ctx, PRISIM_EINVAL, "nothing to compute: want_lag and want_power are both 0");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const DelayGeom g = delay_geom(ctx, pad);
  const int64_t nbl = ctx->nbl, nout = g.nout;
  const int64_t nt_b = delay_batch_snapshots(ctx, g, nt);
  if ((rc = delay_prepare(ctx, g, bpwts, wts_rows, nt_b * nbl))) return rc;
  ctx->dt_have_lag = ctx->dt_have_pow = false;
  if (want_lag && (rc = ensure(ctx, ctx->dt_lag_all, (size_t)nt * nbl * nout * 2 * sizeof(double)))) return rc;
  if (want_power && (rc = ensure(ctx, ctx->dt_pow_all, (size_t)nt * nbl * nout * sizeof(double)))) return rc;
  if (!ctx->ev_d0) {
    HIPCHK(ctx, hipEventCreate(&ctx->ev_d0));
    HIPCHK(ctx, hipEventCreate(&ctx->ev_d1));
  }
  HIPCHK(ctx, hipEventRecord(ctx->ev_d0, ctx->stream));
  for (int64_t t0 = 0; t0 < nt; t0 += nt_b) {
    const int64_t ntc = std::min(nt_b, nt - t0);
    double* d_out = want_lag ? (double*)ctx->dt_lag_all.p + (size_t)t0 * nbl * nout * 2 : nullptr;
    double* d_pow = want_power ? (double*)ctx->dt_pow_all.p + (size_t)t0 * nbl * nout : nullptr;
    if ((rc = delay_batch(ctx, g, t0, ntc * nbl, bpwts != nullptr, wts_rows, d_out, d_pow, power_scale))) return rc;
  }
  HIPCHK(ctx, hipEventRecord(ctx->ev_d1, ctx->stream));
  ctx->dt_nt = nt; ctx->dt_nout = nout;
  ctx->dt_have_lag = want_lag != 0; ctx->dt_have_pow = want_power != 0;
  ctx->timing.last_delay_fused = g.fused ? 1 : 0;
  ctx->timing.last_delay_ms = -1.0;         // filled in by get_timing once the events have completed
  if (lags_out) delay_lags(ctx, lags_out);
  if (nout_out) *nout_out = nout;
  return PRISIM_OK;
  });
}

// Copy rows of the resident spectra to the host.  rows == NULL: all nbl baselines.
static int get_resident(prisim_ctx* ctx, const DevBuf& buf, bool have, int reals, int64_t t0, int64_t nt, const int64_t* rows, int64_t nrows,
                        double* out) {
  if (!have || !buf.p) return fail(ctx, PRISIM_ESTATE, "delay_transform_device has not produced this quantity");
  if (!out) return fail(ctx, PRISIM_EINVAL, "out is NULL");
  if (t0 < 0 || nt <= 0 || t0 + nt > ctx->dt_nt) return fail(ctx, PRISIM_EINVAL, "snapshot range outside the resident spectra");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  const int64_t nbl = ctx->nbl, nout = ctx->dt_nout;
  const size_t row_bytes = (size_t)nout * reals * sizeof(double);
  const char* base = (const char*)buf.p;
  if (!rows) {
    HIPCHK(ctx, hipMemcpy(out, base + (size_t)t0 * nbl * row_bytes, (size_t)nt * nbl * row_bytes, hipMemcpyDeviceToHost));
    return PRISIM_OK;
  }
  if (nrows <= 0) return fail(ctx, PRISIM_EINVAL, "nrows must be positive when rows is given");
  for (int64_t i = 0; i < nrows; ++i)
    if (rows[i] < 0 || rows[i] >= nbl) return fail(ctx, PRISIM_EINVAL, "row index out of range");
  for (int64_t t = 0; t < nt; ++t)
    for (int64_t i = 0; i < nrows; ++i)
      HIPCHK(ctx, hipMemcpyAsync((char*)out + ((size_t)t * nrows + i) * row_bytes, base + ((size_t)(t0 + t) * nbl + rows[i]) * row_bytes, row_bytes,
                                 hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return PRISIM_OK;
}

int prisim_hip_get_lags(prisim_ctx* ctx, int64_t t0, int64_t nt, const int64_t* rows, int64_t nrows, double* out) {
  return guarded(ctx, [&]() -> int {
  if (!ctx) return PRISIM_EINVAL;
  return get_resident(ctx, ctx->dt_lag_all, ctx->dt_have_lag, 2, t0, nt, rows, nrows, out);
  });
}

int prisim_hip_get_delay_power(prisim_ctx* ctx, int64_t t0, int64_t nt, const int64_t* rows, int64_t nrows, double* out) {
  return guarded(ctx, [&]() -> int {
  if (!ctx) return PRISIM_EINVAL;
  return get_resident(ctx, ctx->dt_pow_all, ctx->dt_have_pow, 1, t0, nt, rows, nrows, out);
  });
}

int prisim_hip_phase_rotate(prisim_ctx* ctx, int64_t nt, const double* diff_dircos) {
  return guarded(ctx, [&]() -> int {
  if (!ctx) return PRISIM_EINVAL;
  if (!ctx->array_set) return fail(ctx, PRISIM_ESTATE, "set_array has not been called");
  if (nt <= 0 || nt > ctx->nt_max) return fail(ctx, PRISIM_EINVAL, "nt out of range");
  if (!diff_dircos) return fail(ctx, PRISIM_EINVAL, "diff_dircos is NULL");
  for (int64_t i = 0; i < 3 * nt; ++i)
    if (!std::isfinite(diff_dircos[i])) return fail(ctx, PRISIM_EINVAL, "non-finite phase-centre offset");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int rc;
  if ((rc = ensure(ctx, ctx->scratch, std::max<size_t>(1025, (size_t)3 * nt) * sizeof(double)))) return rc;
  HIPCHK(ctx, hipMemcpyAsync(ctx->scratch.p, diff_dircos, (size_t)3 * nt * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, launch_phase_rotate((double*)ctx->cube.p, (const double*)ctx->blx.p, (const double*)ctx->bly.p, (const double*)ctx->blz.p,
                                  (const double*)ctx->freqs.p, (const double*)ctx->scratch.p, nt, ctx->nbl, ctx->nchan, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // diff_dircos is caller-owned
  return PRISIM_OK;
  });
}

int prisim_hip_noise(prisim_ctx* ctx, int64_t nt, const double* rms, uint64_t seed, int64_t bl_offset, double* out) {
  return guarded(ctx, [&]() -> int {
  if (!ctx) return PRISIM_EINVAL;
  if (!ctx->array_set) return fail(ctx, PRISIM_ESTATE, "set_array has not been called");
  if (nt <= 0 || !rms || !out || bl_offset < 0) return fail(ctx, PRISIM_EINVAL, "bad noise arguments");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const size_t n = (size_t)ctx->nbl * ctx->nchan;
  for (size_t i = 0; i < n * (size_t)nt; ++i)
    if (!(rms[i] >= 0.0) || !std::isfinite(rms[i])) return fail(ctx, PRISIM_EINVAL, "noise rms must be finite and non-negative");
  DevBuf drms, dout;
  int rc;
  if ((rc = ensure(ctx, drms, n * sizeof(double))) || (rc = ensure(ctx, dout, n * 2 * sizeof(double)))) {
    release(drms); release(dout);
    return rc;
  }
  hipError_t e = hipSuccess;
  for (int64_t t = 0; t < nt && e == hipSuccess; ++t) {
    e = hipMemcpyAsync(drms.p, rms + (size_t)t * n, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = launch_noise((const double*)drms.p, (double*)dout.p, ctx->nbl, ctx->nchan, t, bl_offset, seed, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out + (size_t)t * n * 2, dout.p, n * 2 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  }
  release(drms); release(dout);
  HIPCHK(ctx, e);
  return PRISIM_OK;
  });
}

int prisim_hip_noise_indexed(prisim_ctx* ctx, int64_t nt, const double* rms, uint64_t seed, const int64_t* bl_index, double* out) {
  return guarded(ctx, [&]() -> int {
  if (!ctx) return PRISIM_EINVAL;
  if (!ctx->array_set) return fail(ctx, PRISIM_ESTATE, "set_array has not been called");
  if (nt <= 0 || !rms || !out || !bl_index) return fail(ctx, PRISIM_EINVAL, "bad noise arguments");
  for (int64_t b = 0; b < ctx->nbl; ++b)
    if (bl_index[b] < 0) return fail(ctx, PRISIM_EINVAL, "negative global baseline index");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const size_t n = (size_t)ctx->nbl * ctx->nchan;
  for (size_t i = 0; i < n * (size_t)nt; ++i)
    if (!(rms[i] >= 0.0) || !std::isfinite(rms[i])) return fail(ctx, PRISIM_EINVAL, "noise rms must be finite and non-negative");
  DevBuf drms, dout;
  int rc;
  if ((rc = ensure(ctx, drms, n * sizeof(double))) || (rc = ensure(ctx, dout, n * 2 * sizeof(double)))) {
    release(drms); release(dout);
    return rc;
  }
  hipError_t e = hipSuccess;
  for (int64_t t = 0; t < nt && e == hipSuccess; ++t) {
    e = hipMemcpyAsync(drms.p, rms + (size_t)t * n, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
    // one launch per run of consecutive global indices: the generator's counter is (channel, global baseline, snapshot)
    for (int64_t b0 = 0; b0 < ctx->nbl && e == hipSuccess;) {
      int64_t b1 = b0 + 1;
      while (b1 < ctx->nbl && bl_index[b1] == bl_index[b1 - 1] + 1) ++b1;
      e = launch_noise((const double*)drms.p + (size_t)b0 * ctx->nchan, (double*)dout.p + (size_t)b0 * ctx->nchan * 2, b1 - b0, ctx->nchan, t,
                       bl_index[b0], seed, ctx->stream);
      b0 = b1;
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out + (size_t)t * n * 2, dout.p, n * 2 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  }
  release(drms); release(dout);
  HIPCHK(ctx, e);
  return PRISIM_OK;
  });
}

// ---- multi-GPU ------------------------------------------------------------------------------

int prisim_hip_comm_unique_id(char id[128]) {
  return guarded(nullptr, [&]() -> int {
  if (!id) return PRISIM_EINVAL;
  std::string lerr;
  if (!load_rccl(lerr)) return fail(nullptr, PRISIM_ELIB, lerr);
  ncclUniqueId uid;
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is expected to be 128 bytes");
  ncclResult_t r = g_rccl.GetUniqueId(&uid);
  if (r != ncclSuccess) return fail(nullptr, PRISIM_ELIB, std::string("ncclGetUniqueId: ") + g_rccl.GetErrorString(r));
  memcpy(id, &uid, 128);
  return PRISIM_OK;
  });
}

int prisim_hip_comm_version(char out[128]) {
  return guarded(nullptr, [&]() -> int {
  if (!out) return PRISIM_EINVAL;
  std::string lerr;
  if (!load_rccl(lerr)) return fail(nullptr, PRISIM_ELIB, lerr);
  int v = 0;
  if (g_rccl.GetVersion) (void)g_rccl.GetVersion(&v);
  // NCCL_VERSION_CODE: major * 10000 + minor * 100 + patch (2.9 and later)
  snprintf(out, 128, "librccl %d.%d.%d (%s)", v / 10000, (v / 100) % 100, v % 100, g_rccl.path.c_str());
  return PRISIM_OK;
  });
}

int prisim_hip_comm_last_error(char out[512]) {
  // Deliberately NOT through guarded() and without touching any context or the HIP runtime: this is what a watchdog thread calls while
  // the main thread sits inside ncclCommInitRank -- it must not wait for anything that thread holds.
  if (!out) return PRISIM_EINVAL;
  out[0] = 0;
  if (!g_rccl.handle) { snprintf(out, 512, "librccl not loaded"); return PRISIM_OK; }
  const char* msg = g_rccl.GetLastError ? g_rccl.GetLastError(nullptr) : nullptr;
  snprintf(out, 512, "%s", (msg && msg[0]) ? msg : "(librccl reports no error text; NCCL_DEBUG=WARN prints its warnings on stderr)");
  return PRISIM_OK;
}

int prisim_hip_device_pci(int device, char out[64]) {
  return guarded(nullptr, [&]() -> int {
  if (!out) return PRISIM_EINVAL;
  out[0] = 0;
  if (hipDeviceGetPCIBusId(out, 64, device) != hipSuccess) { (void)hipGetLastError(); snprintf(out, 64, "unknown"); }
  return PRISIM_OK;
  });
}

int prisim_hip_comm_init(prisim_ctx* ctx, const char id[128], int nranks, int rank) {
  return guarded(ctx, [&]() -> int {
  if (!ctx) return PRISIM_EINVAL;
  if (!id || nranks <= 0 || rank < 0 || rank >= nranks) return fail(ctx, PRISIM_EINVAL, "bad communicator arguments");
  std::string lerr;
  if (!load_rccl(lerr)) return fail(ctx, PRISIM_ELIB, lerr);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (ctx->comm) { g_rccl.CommDestroy(ctx->comm); ctx->comm = nullptr; }
  ncclUniqueId uid;
  memcpy(&uid, id, 128);
  ncclResult_t r = g_rccl.CommInitRank(&ctx->comm, nranks, uid, rank);
  if (r != ncclSuccess) {
    ctx->comm = nullptr;
    return fail(ctx, PRISIM_ELIB, std::string("ncclCommInitRank: ") + g_rccl.GetErrorString(r));
  }
  if (nranks != ctx->nranks && ctx->nbl_total > 0) {
    // a shard map is a table of nranks x nbl_shard rows: one made for another communicator size must not be walked with this one
    ctx->nbl_total = 0; ctx->shard_map_h.clear(); release(ctx->shard_map); release(ctx->gathered);
  }
  ctx->nranks = nranks; ctx->rank = rank;
  return PRISIM_OK;
  });
}

// Gather snapshot `slot` of every rank on stream `st`.  src_all: this rank's [nt][planes][nbl][row] complex128 (the visibility cube, the
// resident lag spectra, or the gradient cube with planes = 3).  Without a shard map the snapshot lands in gathered[slot][rank][planes][b][row]
// (rank blocks as the all-gather leaves them); with one (prisim_hip_set_shard_map) it lands in a staging block of that stream and the
// un-deal kernel behind it writes gathered[slot][planes][global baseline][row] -- the reference's order (run_prisim.py:2233-2242).
static int gather_one_slot(prisim_ctx* ctx, const double* src_all, int64_t row, int planes, int64_t slot, int as_c64, hipStream_t st, int ring = -1) {
  const size_t shard = (size_t)ctx->nbl * row * 2 * (size_t)planes;   // reals per snapshot shard
  const size_t esz = as_c64 ? sizeof(float) : sizeof(double);
  const double* src = src_all + (size_t)slot * shard;
  const void* send = src;
  if (as_c64) {
    float* sb = (float*)ctx->sendbuf.p + (size_t)slot * shard;
    HIPCHK(ctx, launch_f64_to_f32(src, sb, (int64_t)shard, st));
    send = sb;
  }
  const bool receiver = ctx->gather_root < 0 || ctx->gather_root == ctx->rank;
  const bool ordered = ctx->nbl_total > 0;
  if (ordered && ctx->shard_map_h.size() != (size_t)ctx->nranks * (size_t)ctx->nbl)
    return fail(ctx, PRISIM_ESTATE, "the shard map does not match the communicator size and the shard size (set it after comm_init and set_array)");
  char* dst = nullptr;
  if (receiver) {
    if (ordered) {
      DevBuf& stage = (st == ctx->comm_stream && ctx->comm_stream) ? ctx->stage_comm : ctx->stage_main;
      int rc;
      if ((rc = ensure(ctx, stage, shard * (size_t)ctx->nranks * esz))) return rc;
      dst = (char*)stage.p;
    } else {
      dst = (char*)ctx->gathered.p + (size_t)slot * shard * (size_t)ctx->nranks * esz;
    }
  }
  if (ctx->nranks == 1 && !ctx->comm) {
    HIPCHK(ctx, hipMemcpyAsync(dst, send, shard * esz, hipMemcpyDeviceToDevice, st));
  } else {
    if (!ctx->comm) return fail(ctx, PRISIM_ESTATE, "comm_init has not been called");
    const ncclDataType_t ty = as_c64 ? ncclFloat : ncclDouble;
    if (ctx->gather_root < 0) {
      ncclResult_t r = g_rccl.AllGather(send, dst, shard, ty, ctx->comm, st);
      if (r != ncclSuccess) return fail(ctx, PRISIM_ELIB, std::string("ncclAllGather: ") + g_rccl.GetErrorString(r));
    } else {
      // gather to ONE rank (SURVEY 8(e) `gather_to_root`): the other GPUs keep no copy of the whole cube -- 120 GB at config 5.  One
      // grouped call: the root posts a receive per peer into that peer's block, every other rank one send; the root's own block is a copy.
      if (!g_rccl.Send) return fail(ctx, PRISIM_ELIB, "this librccl has no ncclSend / ncclRecv: gather to a root is unavailable");
      ncclResult_t r = g_rccl.GroupStart();
      if (r == ncclSuccess) {
        if (receiver) {
          for (int q = 0; q < ctx->nranks && r == ncclSuccess; ++q)
            if (q != ctx->rank) r = g_rccl.Recv(dst + (size_t)q * shard * esz, shard, ty, q, ctx->comm, st);
        } else {
          r = g_rccl.Send(send, shard, ty, ctx->gather_root, ctx->comm, st);
        }
        const ncclResult_t r2 = g_rccl.GroupEnd();
        if (r == ncclSuccess) r = r2;
      }
      if (r != ncclSuccess) return fail(ctx, PRISIM_ELIB, std::string("ncclSend/ncclRecv (gather to root): ") + g_rccl.GetErrorString(r));
      if (receiver) HIPCHK(ctx, hipMemcpyAsync(dst + (size_t)ctx->rank * shard * esz, send, shard * esz, hipMemcpyDeviceToDevice, st));
    }
  }
  if (ordered && receiver) {
    if (ring >= 0) HIPCHK(ctx, hipEventRecord(ctx->ev_gu[ring], st));
    const size_t row_words = (size_t)row * 2 * esz / 8;               // a row of complex numbers in 8-byte words
    char* out = (char*)ctx->gathered.p + (size_t)slot * (size_t)planes * (size_t)ctx->nbl_total * row_words * 8;
    HIPCHK(ctx, launch_undeal(dst, out, (const int64_t*)ctx->shard_map.p, ctx->nranks, ctx->nbl, ctx->nbl_total, planes, (int64_t)row_words, st));
  }
  return PRISIM_OK;
}

// bytes of the gathered cube for nt snapshots of rows of `row` complex numbers (x planes)
static size_t gathered_bytes(const prisim_ctx* ctx, int64_t nt, int64_t row_total, bool c64) {
  const size_t esz = c64 ? sizeof(float) : sizeof(double);
  const size_t rows = ctx->nbl_total > 0 ? (size_t)ctx->nbl_total : (size_t)ctx->nbl * (size_t)ctx->nranks;
  return (size_t)nt * rows * (size_t)row_total * 2 * esz;
}

static int ensure_gather_buffers(prisim_ctx* ctx, int64_t row, int as_c64) {
  const size_t shard = (size_t)ctx->nbl * row * 2;
  int rc;
  if (ctx->gathered.p && (ctx->gathered_c64 != (as_c64 != 0) || ctx->gathered_row != row)) release(ctx->gathered);
  const bool receiver = ctx->gather_root < 0 || ctx->gather_root == ctx->rank;       // only receivers hold the whole cube
  if ((rc = ensure(ctx, ctx->gathered, receiver ? gathered_bytes(ctx, ctx->nt_max, row, as_c64 != 0) : 16))) return rc;
  if (as_c64 && (rc = ensure(ctx, ctx->sendbuf, shard * (size_t)ctx->nt_max * sizeof(float)))) return rc;
  ctx->gathered_c64 = as_c64 != 0;
  ctx->gathered_row = row;
  return PRISIM_OK;
}

int prisim_hip_allgather(prisim_ctx* ctx, int64_t nt, int as_c64) {
  return guarded(ctx, [&]() -> int {
  if (!ctx) return PRISIM_EINVAL;
  if (!ctx->array_set) return fail(ctx, PRISIM_ESTATE, "set_array has not been called");
  if (nt <= 0 || nt > ctx->nt_max) return fail(ctx, PRISIM_EINVAL, "nt out of range");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int rc;
  if (ctx->comm_stream && ctx->comm_pending) { HIPCHK(ctx, hipStreamSynchronize(ctx->comm_stream)); ctx->comm_pending = false; }
  if ((rc = ensure_gather_buffers(ctx, ctx->nchan, as_c64))) return rc;
  for (int64_t t = 0; t < nt; ++t)
    if ((rc = gather_one_slot(ctx, (const double*)ctx->cube.p, ctx->nchan, 1, t, as_c64, ctx->stream))) return rc;
  return PRISIM_OK;
  });
}

int prisim_hip_allgather_lags(prisim_ctx* ctx, int64_t nt) {
  return guarded(ctx, [&]() -> int {
  if (!ctx) return PRISIM_EINVAL;
  if (!ctx->array_set) return fail(ctx, PRISIM_ESTATE, "set_array has not been called");
  if (!ctx->dt_have_lag || !ctx->dt_lag_all.p) return fail(ctx, PRISIM_ESTATE, "delay_transform_device(want_lag) must be called first");
  if (nt <= 0 || nt > ctx->dt_nt || nt > ctx->nt_max) return fail(ctx, PRISIM_EINVAL, "nt does not match the resident lag spectra");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int rc;
  if (ctx->comm_stream && ctx->comm_pending) { HIPCHK(ctx, hipStreamSynchronize(ctx->comm_stream)); ctx->comm_pending = false; }
  if ((rc = ensure_gather_buffers(ctx, ctx->dt_nout, 0))) return rc;
  for (int64_t t = 0; t < nt; ++t)
    if ((rc = gather_one_slot(ctx, (const double*)ctx->dt_lag_all.p, ctx->dt_nout, 1, t, 0, ctx->stream))) return rc;
  return PRISIM_OK;
  });
}

int prisim_hip_allgather_slot_async(prisim_ctx* ctx, int64_t slot, int as_c64) {
  return guarded(ctx, [&]() -> int {
  if (!ctx) return PRISIM_EINVAL;
  if (!ctx->array_set) return fail(ctx, PRISIM_ESTATE, "set_array has not been called");
  if (slot < 0 || slot >= ctx->nt_max) return fail(ctx, PRISIM_EINVAL, "slot out of range");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int rc;
  if ((rc = ensure_comm_stream(ctx))) return rc;
  if (!ctx->gathered.p || ctx->gathered_c64 != (as_c64 != 0) || ctx->gathered_row != ctx->nchan) {
    // (re)allocation must not race with gathers in flight
    HIPCHK(ctx, hipStreamSynchronize(ctx->comm_stream));
    if ((rc = ensure_gather_buffers(ctx, ctx->nchan, as_c64))) return rc;
  }
  if (ctx->cring_pending >= prisim_ctx::kCommRing) {          // a full ring waits for its oldest entry only
    const int o = (ctx->cring_head - ctx->cring_pending + 2 * prisim_ctx::kCommRing) % prisim_ctx::kCommRing;
    HIPCHK(ctx, hipEventSynchronize(ctx->ev_g1[o]));
  }
  harvest_comm(ctx, false);
  const int ri = ctx->cring_head;
  // the gather of slot t waits for everything enqueued so far on the compute stream (i.e. compute(slot t)) ...
  HIPCHK(ctx, hipEventRecord(ctx->ev_gc[ri], ctx->stream));
  HIPCHK(ctx, hipStreamWaitEvent(ctx->comm_stream, ctx->ev_gc[ri], 0));
  // ... and for the deferred post-pass that writes the slot: the communication stream joins it, not the compute stream, so that the next
  // sky-sum still runs over the post-pass and the gather
  if ((rc = join_post_on(ctx, ctx->comm_stream))) return rc;
  // ... and runs on the (highest-priority) communication stream, overlapping the next snapshot's compute
  HIPCHK(ctx, hipEventRecord(ctx->ev_g0[ri], ctx->comm_stream));
  if ((rc = gather_one_slot(ctx, (const double*)ctx->cube.p, ctx->nchan, 1, slot, as_c64, ctx->comm_stream, ri))) return rc;
  HIPCHK(ctx, hipEventRecord(ctx->ev_g1[ri], ctx->comm_stream));
  ctx->cring_head = (ctx->cring_head + 1) % prisim_ctx::kCommRing;
  ctx->cring_pending += 1;
  ctx->cstats.bytes_per_peer = (int64_t)((size_t)ctx->nbl * ctx->nchan * 2 * (as_c64 ? sizeof(float) : sizeof(double)));
  ctx->cstats.nranks = ctx->nranks;
  ctx->comm_pending = true;
  return PRISIM_OK;
  }, /*join=*/false);
}

int prisim_hip_get_gathered(prisim_ctx* ctx, int64_t nt, void* out) {
  return guarded(ctx, [&]() -> int {
  if (!ctx) return PRISIM_EINVAL;
  if (!out) return fail(ctx, PRISIM_EINVAL, "out is NULL");
  if (!ctx->gathered.p) return fail(ctx, PRISIM_ESTATE, "allgather has not been called");
  if (ctx->gather_root >= 0 && ctx->gather_root != ctx->rank) return fail(ctx, PRISIM_ESTATE, "the cube was gathered to another rank (set_gather_root)");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const size_t bytes = gathered_bytes(ctx, nt, ctx->gathered_row, ctx->gathered_c64);
  if (nt <= 0 || bytes > ctx->gathered.bytes) return fail(ctx, PRISIM_EINVAL, "nt does not match the gathered cube");
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  if (ctx->comm_stream) { HIPCHK(ctx, hipStreamSynchronize(ctx->comm_stream)); ctx->comm_pending = false; }
  HIPCHK(ctx, hipMemcpy(out, ctx->gathered.p, bytes, hipMemcpyDeviceToHost));
  return PRISIM_OK;
  });
}

int prisim_hip_gathered_checksum(prisim_ctx* ctx, int64_t nt, double* out) {
  return guarded(ctx, [&]() -> int {
  if (!ctx) return PRISIM_EINVAL;
  if (!out) return fail(ctx, PRISIM_EINVAL, "out is NULL");
  if (!ctx->gathered.p) return fail(ctx, PRISIM_ESTATE, "allgather has not been called");
  if (ctx->gather_root >= 0 && ctx->gather_root != ctx->rank) return fail(ctx, PRISIM_ESTATE, "the cube was gathered to another rank (set_gather_root)");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const size_t esz = ctx->gathered_c64 ? sizeof(float) : sizeof(double);
  const int64_t n = (int64_t)(gathered_bytes(ctx, nt, ctx->gathered_row, ctx->gathered_c64) / esz);
  if (nt <= 0 || (size_t)n * esz > ctx->gathered.bytes) return fail(ctx, PRISIM_EINVAL, "nt does not match the gathered cube");
  int rc;
  if ((rc = ensure(ctx, ctx->scratch, 1025 * sizeof(double)))) return rc;
  if (ctx->comm_stream) { HIPCHK(ctx, hipStreamSynchronize(ctx->comm_stream)); ctx->comm_pending = false; }
  HIPCHK(ctx, launch_checksum(ctx->gathered.p, ctx->gathered_c64, n, (double*)ctx->scratch.p, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(out, ctx->scratch.p, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return PRISIM_OK;
  });
}

int prisim_hip_allgather_grad(prisim_ctx* ctx, int64_t nt, int as_c64) {
  return guarded(ctx, [&]() -> int {
  if (!ctx) return PRISIM_EINVAL;
  if (!ctx->array_set) return fail(ctx, PRISIM_ESTATE, "set_array has not been called");
  if (!ctx->grad.p) return fail(ctx, PRISIM_ESTATE, "no gradient has been computed");
  if (nt <= 0 || nt > ctx->nt_max) return fail(ctx, PRISIM_EINVAL, "nt out of range");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int rc;
  if (ctx->comm_stream && ctx->comm_pending) { HIPCHK(ctx, hipStreamSynchronize(ctx->comm_stream)); ctx->comm_pending = false; }
  // a snapshot's gradient block is [3][nbl][nchan]: the same exchange with rows of 3 nchan -> gathered [nt][nranks][3][nbl][nchan]
  if ((rc = ensure_gather_buffers(ctx, 3 * ctx->nchan, as_c64))) return rc;
  for (int64_t t = 0; t < nt; ++t)
    if ((rc = gather_one_slot(ctx, (const double*)ctx->grad.p, ctx->nchan, 3, t, as_c64, ctx->stream))) return rc;
  return PRISIM_OK;
  });
}

int prisim_hip_set_shard_map(prisim_ctx* ctx, const int64_t* bl_index, int64_t nbl_total) {
  return guarded(ctx, [&]() -> int {
  if (!ctx) return PRISIM_EINVAL;
  if (!ctx->array_set) return fail(ctx, PRISIM_ESTATE, "set_array (and comm_init on more than one rank) must be called before set_shard_map");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const size_t n = (size_t)ctx->nranks * (size_t)ctx->nbl;
  std::vector<int64_t> map;
  if (bl_index) {
    if (nbl_total <= 0 || (size_t)nbl_total > n) return fail(ctx, PRISIM_EINVAL, "nbl_total must be in [1, nranks x nbl_shard]");
    // every global baseline exactly once; anything else is padding (-1)
    std::vector<uint8_t> seen((size_t)nbl_total, 0);
    map.assign(bl_index, bl_index + n);
    for (size_t i = 0; i < n; ++i) {
      if (map[i] < 0) { map[i] = -1; continue; }
      if (map[i] >= nbl_total) return fail(ctx, PRISIM_EINVAL, "shard map: global baseline index out of range");
      if (seen[(size_t)map[i]]) return fail(ctx, PRISIM_EINVAL, "shard map: a global baseline is listed twice (padding rows must be -1)");
      seen[(size_t)map[i]] = 1;
    }
    for (int64_t g = 0; g < nbl_total; ++g)
      if (!seen[(size_t)g]) return fail(ctx, PRISIM_EINVAL, "shard map: a global baseline is missing");
  }
  // gathers in flight use the old layout
  if (ctx->comm_stream && ctx->comm_pending) { HIPCHK(ctx, hipStreamSynchronize(ctx->comm_stream)); ctx->comm_pending = false; }
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  release(ctx->gathered);                  // its layout follows the map
  if (!bl_index) {
    ctx->nbl_total = 0; ctx->shard_map_h.clear(); release(ctx->shard_map);
    return PRISIM_OK;
  }
  int rc;
  if ((rc = ensure(ctx, ctx->shard_map, n * sizeof(int64_t)))) return rc;
  HIPCHK(ctx, hipMemcpy(ctx->shard_map.p, map.data(), n * sizeof(int64_t), hipMemcpyHostToDevice));
  ctx->shard_map_h.swap(map);
  ctx->nbl_total = nbl_total;
  return PRISIM_OK;
  });
}

int prisim_hip_set_gather_root(prisim_ctx* ctx, int root) {
  return guarded(ctx, [&]() -> int {
  if (!ctx) return PRISIM_EINVAL;
  if (root < -1 || root >= ctx->nranks) return fail(ctx, PRISIM_EINVAL, "root must be -1 (all ranks) or a rank of the communicator");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (ctx->comm_stream && ctx->comm_pending) { HIPCHK(ctx, hipStreamSynchronize(ctx->comm_stream)); ctx->comm_pending = false; }
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  if (root != ctx->gather_root) release(ctx->gathered);          // its size depends on who receives
  ctx->gather_root = root;
  return PRISIM_OK;
  });
}

int prisim_hip_comm_selftest(prisim_ctx* ctx, int64_t bytes) {
  return guarded(ctx, [&]() -> int {
  if (!ctx) return PRISIM_EINVAL;
  if (bytes < 4 || bytes > ((int64_t)1 << 30)) return fail(ctx, PRISIM_EINVAL, "selftest size must be in [4 B, 1 GiB]");
  if (ctx->nranks > 1 && !ctx->comm) return fail(ctx, PRISIM_ESTATE, "comm_init has not been called");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const size_t n = (size_t)bytes / 4;
  const int nr = ctx->nranks;
  std::vector<uint32_t> h(n * (size_t)nr);
  auto pattern = [](int r, size_t i) { return (uint32_t)(r + 1) * 0x9E3779B1u ^ (uint32_t)(i * 0x85EBCA6Bu + 0x1234567u); };
  for (size_t i = 0; i < n; ++i) h[i] = pattern(ctx->rank, i);
  DevBuf dsend, drecv;
  int rc;
  if ((rc = ensure(ctx, dsend, n * 4)) || (rc = ensure(ctx, drecv, n * 4 * (size_t)nr))) { release(dsend); release(drecv); return rc; }
  hipError_t e = hipMemcpyAsync(dsend.p, h.data(), n * 4, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemsetAsync(drecv.p, 0, n * 4 * (size_t)nr, ctx->stream);
  std::string nerr;
  if (e == hipSuccess) {
    if (ctx->comm) {
      ncclResult_t r = g_rccl.AllGather(dsend.p, drecv.p, n, ncclUint32, ctx->comm, ctx->stream);
      if (r != ncclSuccess) nerr = std::string("ncclAllGather (self-test): ") + g_rccl.GetErrorString(r);
    } else {
      e = hipMemcpyAsync(drecv.p, dsend.p, n * 4, hipMemcpyDeviceToDevice, ctx->stream);
    }
  }
  if (e == hipSuccess && nerr.empty()) e = hipMemcpyAsync(h.data(), drecv.p, n * 4 * (size_t)nr, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess && nerr.empty()) e = hipStreamSynchronize(ctx->stream);
  release(dsend); release(drecv);
  if (!nerr.empty()) return fail(ctx, PRISIM_ELIB, nerr);
  HIPCHK(ctx, e);
  for (int r = 0; r < nr; ++r)
    for (size_t i = 0; i < n; ++i)
      if (h[(size_t)r * n + i] != pattern(r, i))
        return fail(ctx, PRISIM_ELIB, "RCCL self-test: block of rank " + std::to_string(r) + " arrived corrupted at word " + std::to_string(i) +
                                          " on rank " + std::to_string(ctx->rank));
  return PRISIM_OK;
  });
}

int prisim_hip_get_comm_stats(prisim_ctx* ctx, prisim_comm_stats* out, int reset) {
  return guarded(ctx, [&]() -> int {
  if (!ctx) return PRISIM_EINVAL;
  if (!out) return fail(ctx, PRISIM_EINVAL, "out is NULL");
  if (ctx->cring_pending > 0) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    harvest_comm(ctx, true);
  }
  ctx->cstats.nranks = ctx->nranks;
  *out = ctx->cstats;
  if (reset) {
    ctx->cstats.n_gathers = 0;
    ctx->cstats.sum_gather_ms = ctx->cstats.max_gather_ms = ctx->cstats.last_gather_ms = ctx->cstats.last_gather_after_compute_ms = 0.0;
    ctx->cstats.sum_undeal_ms = ctx->cstats.last_undeal_ms = 0.0;
  }
  return PRISIM_OK;
  });
}

// ---- host-visible results without a serial PCIe tail --------------------------------------------

int prisim_hip_host_alloc(int64_t bytes, void** out) {
  return guarded(nullptr, [&]() -> int {
  if (!out) return fail(nullptr, PRISIM_EINVAL, "out is NULL");
  *out = nullptr;
  if (bytes <= 0) return fail(nullptr, PRISIM_EINVAL, "bytes must be positive");
  void* p = nullptr;
  hipError_t e = hipHostMalloc(&p, (size_t)bytes, hipHostMallocDefault);
  if (e != hipSuccess) return fail(nullptr, e == hipErrorOutOfMemory ? PRISIM_ENOMEM : PRISIM_ENODEV,
                                   std::string("hipHostMalloc(") + std::to_string(bytes) + " B): " + hipGetErrorString(e));
  *out = p;
  return PRISIM_OK;
  });
}

int prisim_hip_host_free(void* p) {
  return guarded(nullptr, [&]() -> int {
  if (p && hipHostFree(p) != hipSuccess) return fail(nullptr, PRISIM_EINVAL, "hipHostFree: not a prisim_hip_host_alloc pointer");
  return PRISIM_OK;
  });
}

int prisim_hip_get_vis_async(prisim_ctx* ctx, int64_t slot, void* vis, void* grad, int out_is_c64) {
  return guarded(ctx, [&]() -> int {
  if (!ctx) return PRISIM_EINVAL;
  if (!ctx->array_set) return fail(ctx, PRISIM_ESTATE, "set_array has not been called");
  if (slot < 0 || slot >= ctx->nt_max) return fail(ctx, PRISIM_EINVAL, "slot out of range");
  if (!vis) return fail(ctx, PRISIM_EINVAL, "vis is NULL");
  if (grad && !ctx->grad.p) return fail(ctx, PRISIM_ESTATE, "no gradient has been computed");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int rc;
  if ((rc = ensure_copy_stream(ctx))) return rc;
  const size_t slot_elems = (size_t)ctx->nbl * ctx->nchan * 2;
  const double* src = (const double*)ctx->cube.p + (size_t)slot * slot_elems;
  const double* gsrc = grad ? (const double*)ctx->grad.p + (size_t)slot * 3 * slot_elems : nullptr;
  // the download waits for everything enqueued so far on the compute stream (the snapshot's sky-sum) and then runs on the copy stream,
  // under the next snapshot's compute
  HIPCHK(ctx, hipEventRecord(ctx->ev_copy_ready, ctx->stream));
  HIPCHK(ctx, hipStreamWaitEvent(ctx->copy_stream, ctx->ev_copy_ready, 0));
  if ((rc = join_post_on(ctx, ctx->copy_stream))) return rc;      // (the deferred post-pass writes the slot: the copy stream joins it)
  if (!out_is_c64) {
    HIPCHK(ctx, hipMemcpyAsync(vis, src, slot_elems * sizeof(double), hipMemcpyDeviceToHost, ctx->copy_stream));
    if (grad) HIPCHK(ctx, hipMemcpyAsync(grad, gsrc, 3 * slot_elems * sizeof(double), hipMemcpyDeviceToHost, ctx->copy_stream));
  } else {
    // rounded to complex64 on the device (the reference's memsave dtype, :6183): half the PCIe bytes.  One staging buffer is enough --
    // conversion and copy of slot t+1 follow the copy of slot t in stream order.
    if (ctx->dl_stage.bytes < 4 * slot_elems * sizeof(float)) {
      HIPCHK(ctx, hipStreamSynchronize(ctx->copy_stream));      // a copy in flight may still read the old buffer
      if ((rc = ensure(ctx, ctx->dl_stage, 4 * slot_elems * sizeof(float)))) return rc;
    }
    float* st = (float*)ctx->dl_stage.p;
    HIPCHK(ctx, launch_f64_to_f32(src, st, (int64_t)slot_elems, ctx->copy_stream));
    HIPCHK(ctx, hipMemcpyAsync(vis, st, slot_elems * sizeof(float), hipMemcpyDeviceToHost, ctx->copy_stream));
    if (grad) {
      HIPCHK(ctx, launch_f64_to_f32(gsrc, st + slot_elems, (int64_t)(3 * slot_elems), ctx->copy_stream));
      HIPCHK(ctx, hipMemcpyAsync(grad, st + slot_elems, 3 * slot_elems * sizeof(float), hipMemcpyDeviceToHost, ctx->copy_stream));
    }
  }
  ctx->copy_pending = true;
  return PRISIM_OK;
  }, /*join=*/false);
}

int prisim_hip_wait_downloads(prisim_ctx* ctx) {
  return guarded(ctx, [&]() -> int {
  if (!ctx) return PRISIM_EINVAL;
  if (ctx->copy_stream && ctx->copy_pending) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->copy_stream));
    ctx->copy_pending = false;
  }
  return PRISIM_OK;
  });
}

}  // extern "C"
