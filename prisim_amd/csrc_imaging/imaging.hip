// imaging.hip -- the dirty image and the synthesized beam of a visibility cube by the direct Fourier sum for gfx950
// (include/prisim_imaging.h): D[p][k] = sum_t sum_b w (Re V cos phi - Im V sin phi), phi = 2 pi f_k b . (s[p][t] - s0[t]) / c, the adjoint
// of the sky-sum (../csrc/skyvis_kernels.hip, k_skyvis_rec) with pixel <-> baseline and baseline <-> source exchanged: there a lane owns
// a baseline and the source's row of pb * flux is wave-uniform, here a lane owns a pixel and the baseline's row of w V is.
//
// The kernels are in imaging_kernels.h, which prisim_clean_image (imclean.hip) shares.  Once per call:
//   k_img_wsum   W[k] = sum_t sum_b w[t][b][k], one thread per channel, t ascending and b ascending inside t.
// Per chunk of pixels (contiguous, a whole number of blocks of 256):
//   k_img_dirs   dd[t][pixel] = normalise(R_t (u + beta_t)) - s0[t], the statement of k_ap_dirs (../csrc_antpower/antpower.hip) operation
//                by operation, less the phase centre.
//   k_img_sum    the hot path.  A workgroup owns 256 pixels (one per thread) and a tile of 32 channels; a thread keeps 32 fp64
//                accumulators and the phasor, nothing else per lane.  For every snapshot, 32 baselines at a time, the workgroup stages
//                (w Re V, w Im V) of the tile and b / c in LDS; every lane then reads the same LDS address (a broadcast, no bank
//                conflict).  Per (pixel, t, b): tau = b . dd / c, then
//                  STEPPED  the seed e^{2 pi i f tau} at the tile's first channel from that channel's true frequency, the phase reduced
//                           to a fraction of a cycle in fp64 before sincospi, and the step e^{2 pi i df tau}; per channel two FMAs into the
//                           accumulator and one complex multiply (two products, two FMAs) on the phasor: 6 fp64 instructions, 10 flop;
//                  DIRECT   the reduced phase and sincospi of every channel.
//                The (t, b) terms of a (pixel, channel) are added by one thread, t ascending, b ascending: no atomics, no split of the
//                sum over workgroups, so the bits do not depend on the chunks.  The fused multiply-adds are written as fma(): the file
//                is built with -ffp-contract=off like the other add-ons, and nothing else is contracted.
//                chan_avg = 0: the thread divides by W[k] and writes the image rows of the chunk; chan_avg = 1: it writes D[p][k] and
//   k_img_avg    sums D over k ascending per pixel and divides by sum_k W[k].
// The chunks alternate between two streams with their own buffers; the results are gathered in a host buffer and copied to the caller's
// arrays when every chunk is in, so that a failed call writes nothing.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "imaging_kernels.h"

namespace {

int dirty_image(prisim_ctx* ctx, const prisim_imaging_args* a, double* out_image, double* out_wsum, prisim_imaging_stats* stats) {
  if (!ctx) return PRISIM_EINVAL;
  const WallTime wall0 = wall_now();
  if (int rc = check_args(ctx, a, out_image)) return rc;
  const int64_t npix = a->npix, nbl = a->nbl, nchan = a->nchan, nt = a->nt;
  const bool psf = a->kind == PRISIM_IMAGE_PSF, avg = a->chan_avg != 0;
  const bool resident = !psf && !a->cube;
  if (resident) {
    if (int rc = check_resident_cube(ctx, nbl, nchan, nt)) return rc;
  }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int lds_max = 0;
  if (int rc = lds_limit(ctx, lds_max)) return rc;
  double df = 0.0;
  const bool uniform = imaging_grid_uniform(a->freqs_hz, nchan, df);
  const ImagingPlan pl = imaging_plan(npix, nbl, nchan, nt, a->weight_form, avg, a->budget_bytes, lds_max, a->route, uniform, kMaxStreams);
  if (pl.refusal)
    return fail(ctx, PRISIM_EINVAL, std::string(pl.refusal) + " (one block of " + std::to_string(pl.block) + " pixels takes " +
                                        std::to_string(pl.block * pl.pixel_bytes) + " B, the workgroup " + std::to_string(pl.lds) + " B of LDS)");
  const Chunks& ch = pl.chunks;
  const int nstreams = ch.nstreams;
  const bool stepped = pl.route == kImagingStepped;

  // the results wait here until every chunk is in: nothing reaches the caller's arrays from a call that fails.  Declared before the
  // streams, so that they outlive every copy in flight on any return path
  const int64_t per_out = avg ? 1 : nchan;
  std::vector<double> h_img((size_t)(npix * per_out));
  std::vector<double> h_wsum((size_t)(avg ? 1 : nchan));

  Work wk;
  Streams& st = wk.st;
  if (int rc = st.create(ctx, nstreams, true)) return rc;
  hipStream_t s0 = st.s[0];

  // the tables go up once on stream 0, outside the budget
  const std::vector<ImgFrame> frames = snapshot_frames(a);
  double *d_uvec = nullptr, *d_frames = nullptr, *d_bl = nullptr, *d_freqs = nullptr, *d_w = nullptr, *d_wsum = nullptr, *d_wtot = nullptr;
  double2* d_cube = nullptr;
  int64_t upload = 0;
  const int64_t ncube = nt * nbl * nchan;
  DEV_UPLOAD(ctx, wk.dev, d_uvec, a->unitvec, (size_t)npix * 3, s0);
  DEV_UPLOAD(ctx, wk.dev, d_frames, reinterpret_cast<const double*>(frames.data()), (size_t)nt * 16, s0);
  DEV_UPLOAD(ctx, wk.dev, d_bl, a->baselines, (size_t)nbl * 3, s0);
  DEV_UPLOAD(ctx, wk.dev, d_freqs, a->freqs_hz, (size_t)nchan, s0);
  upload += npix * 24 + nt * 128 + nbl * 24 + nchan * 8;
  if (!psf && a->cube) {
    DEV_UPLOAD(ctx, wk.dev, d_cube, a->cube, (size_t)ncube * 2, s0);
    upload += ncube * 16;
  }
  ImgWeights W{nullptr, 0, 0, 0};
  if (a->weight_form == PRISIM_IMAGE_W_BASELINE) {
    DEV_UPLOAD(ctx, wk.dev, d_w, a->weights, (size_t)nbl, s0);
    W = ImgWeights{d_w, 0, 1, 0};
    upload += nbl * 8;
  } else if (a->weight_form == PRISIM_IMAGE_W_FULL) {
    DEV_UPLOAD(ctx, wk.dev, d_w, a->weights, (size_t)ncube, s0);
    W = ImgWeights{d_w, nbl * nchan, nchan, 1};
    upload += ncube * 8;
  }
  DEV_ALLOC(ctx, wk.dev, d_wsum, nchan * 8);
  DEV_ALLOC(ctx, wk.dev, d_wtot, 8);
  if (int rc = launch(ctx, k_img_wsum, dim3((unsigned)((nchan + kThreads - 1) / kThreads)), 0, s0, W, nt, nbl, (int)nchan, d_wsum)) return rc;
  hipLaunchKernelGGL(k_img_wtot, dim3(1), dim3(64), 0, s0, (const double*)d_wsum, (int)nchan, d_wtot);
  HIPCHK(ctx, hipGetLastError());

  // per stream: the buffers of one chunk
  double4* d_dd[kMaxStreams] = {};
  double *d_out[kMaxStreams] = {}, *d_avg[kMaxStreams] = {};
  for (int i = 0; i < nstreams; ++i) {
    DEV_ALLOC(ctx, wk.dev, d_dd[i], ch.size * nt * 32);
    DEV_ALLOC(ctx, wk.dev, d_out[i], ch.size * nchan * 8);
    if (avg) DEV_ALLOC(ctx, wk.dev, d_avg[i], ch.size * 8);
  }
  // the kernels start behind whatever the context's stream still writes into the resident cube
  if (resident) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(s0));              // stream 1 starts behind the uploads and the weight sums; the tables are caller memory

  ImgParams base;
  base.cube = psf ? nullptr : resident ? (const double2*)ctx->cube.p : d_cube;
  base.W = W;
  base.bl = d_bl; base.freqs = d_freqs; base.dd = nullptr; base.wsum = d_wsum;
  base.df = df;
  base.nbl = nbl; base.nt = nt; base.count = 0;
  base.nchan = (int)nchan; base.divide = avg ? 0 : 1;
  base.out = nullptr;

  auto kernels = [&](int64_t, Span sp, int i, hipStream_t sc) -> int {
    if (int rc = launch(ctx, k_img_dirs, dim3((unsigned)grid_for(ctx, sp.count * nt)), 0, sc, (const double*)d_uvec,
                        reinterpret_cast<const ImgFrame*>(d_frames), sp.first, sp.count, nt, d_dd[i]))
      return rc;
    ImgParams P = base;
    P.dd = d_dd[i]; P.count = sp.count; P.out = d_out[i];
    const dim3 grid((unsigned)((sp.count + pl.block - 1) / pl.block), (unsigned)pl.ntiles);
    if (int rc = stepped ? launch_sum<true>(ctx, psf, grid, sc, P) : launch_sum<false>(ctx, psf, grid, sc, P)) return rc;
    if (avg)
      return launch(ctx, k_img_avg, dim3((unsigned)((sp.count + kThreads - 1) / kThreads)), 0, sc, (const double*)d_out[i], sp.count, (int)nchan,
                    (const double*)d_wtot, d_avg[i]);
    return PRISIM_OK;
  };
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
    // k_img_sum, per workgroup (block of pixels, channel tile) and (t, b): the tile's row of the cube (16 B a channel, not for the PSF)
    // and of the weights (8 B a channel when there are any), and the baseline (24 B); per pixel and snapshot its offsets (32 B per
    // tile); the rows of D or of the image written (8 B), read again and averaged with chan_avg.  k_img_dirs: 24 B read and 32 B
    // written per (pixel, snapshot).  k_img_wsum: the weights once.
    const int64_t wg = pl.nblocks * pl.ntiles;
    const int64_t row = pl.tile * ((psf ? 0 : 16) + (W.w ? 8 : 0)) + 24;
    stats->wall_ms = wall_ms_since(wall0);
    stats->kernel_ms = st.kernel_ms;
    stats->terms = npix * nbl * nchan * nt;
    stats->chunks = ch.count;
    stats->chunk_pixels = ch.size;
    stats->kernel_bytes = wg * nt * nbl * row + npix * nt * (24 + 32 + 32 * pl.ntiles) + npix * nchan * 8 * (avg ? 2 : 1) + (avg ? npix * 8 : 0) +
                          (W.w ? ncube * 8 : 0) + nchan * 16;
    stats->upload_bytes = upload;
    stats->download_bytes = (npix * per_out + (int64_t)h_wsum.size()) * 8;
    stats->route = pl.route;
    stats->streams = nstreams;
    stats->chan_tile = (int32_t)pl.tile;
    stats->reseed = (int32_t)pl.reseed;
    stats->lds_bytes = (int32_t)pl.lds;
    stats->block_pixels = (int32_t)pl.block;
  }
  return PRISIM_OK;
}

}  // namespace

extern "C" {

int prisim_dirty_image(prisim_ctx* ctx, const prisim_imaging_args* a, double* out_image, double* out_wsum, prisim_imaging_stats* stats) {
  return guarded(ctx, [&]() -> int { return dirty_image(ctx, a, out_image, out_wsum, stats); });
}

}  // extern "C"
