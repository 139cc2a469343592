// imaging32.hip -- the dirty image and the synthesized beam of a visibility cube by the direct Fourier sum with the per-term arithmetic
// in fp32, for gfx950 (include/prisim_imaging32.h): the sum of imaging.hip, D[p][k] = sum_t sum_b w (Re V cos phi - Im V sin phi), with
// the phase formed and reduced in fp64 and the phasor, the recurrence and the partial sums in fp32.
//
// The tile pass and its kernel are in imaging32_kernels.h; the directions, the weight sums, the band average, the checks, the preamble
// and the tables are those of prisim_dirty_image (dirty_frame.h, imaging_kernels.h), called as they are.  Here, as in imaging.hip: the
// chunks of pixels alternate between two streams with their own buffers; the results are gathered in a host buffer and copied to the
// caller's arrays when every chunk is in, so that a failed call writes nothing.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/prisim_imaging32.h"
#include "imaging32_kernels.h"

namespace {

int dirty_image_f32(prisim_ctx* ctx, const prisim_imaging_args* a, double* out_image, double* out_wsum, prisim_imaging_stats* stats) {
  if (!ctx) return PRISIM_EINVAL;
  const WallTime wall0 = wall_now();
  if (!a) return fail(ctx, PRISIM_EINVAL, "the argument struct is NULL");
  if (!out_image) return fail(ctx, PRISIM_EINVAL, "out_image is NULL");
  const ImgView v = imaging_view(*a, a->kind);
  if (int rc = check_args(ctx, v)) return rc;
  const int64_t npix = v.npix, nchan = v.nchan, nt = v.nt;
  const bool avg = v.chan_avg != 0;
  ImgSetup su{};
  if (int rc = imaging_preamble(ctx, v, su)) return rc;
  const Imaging32Plan pl =
      imaging32_plan(npix, v.nbl, nchan, nt, v.weight_form, avg, v.budget_bytes, su.lds_max, v.route, su.uniform, kMaxStreams);
  if (pl.refusal) return fail(ctx, PRISIM_EINVAL, plan_refusal(pl));
  const Chunks& ch = pl.chunks;
  const int nstreams = ch.nstreams;

  // the results wait here until every chunk is in: nothing reaches the caller's arrays from a call that fails.  Declared before the
  // streams, so that they outlive every copy in flight on any return path
  const int64_t per_out = avg ? 1 : nchan;
  std::vector<double> h_img((size_t)(npix * per_out));
  std::vector<double> h_wsum((size_t)(avg ? 1 : nchan));
  ImgTables T;

  Work wk;
  Streams& st = wk.st;
  if (int rc = st.create(ctx, nstreams, true)) return rc;
  hipStream_t s0 = st.s[0];

  if (int rc = upload_tables(ctx, wk.dev, v, s0, T)) return rc;
  double *d_wsum = nullptr, *d_wtot = nullptr;
  DEV_ALLOC(ctx, wk.dev, d_wsum, nchan * 8);
  DEV_ALLOC(ctx, wk.dev, d_wtot, 8);
  const DirtyImage job = dirty_image_of(v, T, su.df, pl, d_wsum, d_wtot);
  if (int rc = enqueue_weight_sums(ctx, job, s0)) return rc;

  // per stream: the buffers of one chunk, fp64 as in prisim_dirty_image
  double4* d_dd[kMaxStreams] = {};
  double *d_out[kMaxStreams] = {}, *d_avg[kMaxStreams] = {};
  for (int i = 0; i < nstreams; ++i) {
    DEV_ALLOC(ctx, wk.dev, d_dd[i], ch.size * nt * 32);
    DEV_ALLOC(ctx, wk.dev, d_out[i], ch.size * nchan * 8);
    if (avg) DEV_ALLOC(ctx, wk.dev, d_avg[i], ch.size * 8);
  }
  // the kernels start behind whatever the context's stream still writes into the resident cube
  if (v.resident()) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(s0));              // stream 1 starts behind the uploads and the weight sums; the tables are caller memory

  auto kernels = [&](int64_t, Span sp, int i, hipStream_t sc) -> int { return enqueue_dirty32(ctx, job, sp, d_dd[i], d_out[i], d_avg[i], sc); };
  auto download = [&](int64_t, Span sp, int i, hipStream_t sc) -> int {
    HIPCHK(ctx, hipMemcpyAsync(h_img.data() + (size_t)(sp.first * per_out), avg ? d_avg[i] : d_out[i], (size_t)(sp.count * per_out) * 8,
                               hipMemcpyDeviceToHost, sc));
    return PRISIM_OK;
  };
  if (int rc = chunk_loop(ctx, st, ch, npix, no_step, kernels, download)) return rc;
  HIPCHK(ctx, hipMemcpy(h_wsum.data(), avg ? d_wtot : d_wsum, h_wsum.size() * 8, hipMemcpyDeviceToHost));

  std::memcpy(out_image, h_img.data(), h_img.size() * 8);
  if (out_wsum) std::memcpy(out_wsum, h_wsum.data(), h_wsum.size() * 8);
  if (stats) {
    stats->wall_ms = wall_ms_since(wall0);
    stats->kernel_ms = st.kernel_ms;
    stats->chunks = ch.count;
    stats->chunk_pixels = ch.size;
    stats->kernel_bytes = dirty_kernel_bytes(v, pl, T.W.w != nullptr);
    stats->upload_bytes = T.bytes;
    stats->download_bytes = (npix * per_out + (int64_t)h_wsum.size()) * 8;
    plan_stats(stats, v, pl, nstreams);
  }
  return PRISIM_OK;
}

}  // namespace

extern "C" {

int prisim_dirty_image_f32(prisim_ctx* ctx, const prisim_imaging_args* a, double* out_image, double* out_wsum, prisim_imaging_stats* stats) {
  return guarded(ctx, [&]() -> int { return dirty_image_f32(ctx, a, out_image, out_wsum, stats); });
}

}  // extern "C"
