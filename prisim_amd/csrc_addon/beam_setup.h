// beam_setup.h -- what the add-on entries that evaluate the fused analytic beam share on the host (../csrc_antpower/antpower.hip,
// ../csrc_imaging/mosaic.hip): the checks of a beam description with its n_ext extensions, the prisim_beam_ext -> BeamParams mapping,
// the upload of the beamformers' element arrays and the verdict of the polynomial beams' validity flag.  The beam statement itself is
// launch_beam_flux (../csrc/aux_kernels.hip), called with unit flux.  Not part of the public ABI.
#ifndef PRISIM_BEAM_SETUP_H
#define PRISIM_BEAM_SETUP_H

#include <cmath>
#include <cstdint>
#include <vector>

#include "addon_internal.h"

namespace pint {

// the prisim_beam_ext -> BeamParams mapping of sky_beam_flux (../csrc/capi.cpp), restated; bf: the device copy of the beamformer's
// element arrays (positions, delays, gains, in that order) or null
inline void fill_beam(BeamParams& bp, int32_t beam_kind, double diameter_m, const double* beam_pc_dircos, const prisim_beam_ext* x,
                      const double* bf) {
  bp.beam_kind = beam_kind;
  bp.diameter = diameter_m;
  bp.bpc_x = beam_pc_dircos[0]; bp.bpc_y = beam_pc_dircos[1]; bp.bpc_z = beam_pc_dircos[2];
  if (x) {
    const int bf_n = x->bf_nelem, bf_r = bf_n > 0 ? x->bf_nrand : 0;
    bp.dip_x = x->dipole_dircos[0]; bp.dip_y = x->dipole_dircos[1]; bp.dip_z = x->dipole_dircos[2];
    bp.dipole_mode = x->dipole_mode;
    bp.nax1 = x->array_nax1; bp.nax2 = x->array_nax2; bp.sep1 = x->array_sep1; bp.sep2 = x->array_sep2;
    const double ang = x->array_east2ax1_deg * M_PI / 180.0;
    bp.rot_c = std::cos(ang); bp.rot_s = std::sin(ang);
    bp.apc_x = x->array_pc_dircos[0]; bp.apc_y = x->array_pc_dircos[1]; bp.apc_z = x->array_pc_dircos[2];
    bp.gp_height = x->ground_height; bp.gp_modify = x->ground_modify; bp.gp_scale = x->ground_scale; bp.gp_max = x->ground_max;
    if (bf_n > 0) {
      bp.bf_nelem = bf_n; bp.bf_nrand = bf_r;
      bp.bf_pos = bf;
      bp.bf_delays = bp.bf_pos + (size_t)bf_n * 3;
      bp.bf_gains = bp.bf_delays + (size_t)bf_n * bf_r;
    }
    if (beam_kind == PRISIM_BEAM_POLY)
      for (int i = 0; i < 4; ++i) bp.poly[i] = x->poly_coef[i];
  }
}

// n_ext is 0, 1 or nsnap (called `nsnap_name` in the message), ext is there when n_ext > 0, and the fused beam takes every description
inline int check_beams(prisim_ctx* ctx, int32_t beam_kind, double diameter_m, const double* beam_pc_dircos, const prisim_beam_ext* ext,
                       int64_t n_ext, int64_t nsnap, const char* nsnap_name) {
  if (n_ext != 0 && n_ext != 1 && n_ext != nsnap) return fail(ctx, PRISIM_EINVAL, std::string("n_ext must be 0, 1 or ") + nsnap_name);
  if (n_ext > 0 && !ext) return fail(ctx, PRISIM_EINVAL, "ext is NULL with n_ext > 0");
  if (n_ext == 0) return check_beam_spec(ctx, beam_kind, diameter_m, beam_pc_dircos, nullptr);
  for (int64_t e = 0; e < n_ext; ++e)
    if (int rc = check_beam_spec(ctx, beam_kind, diameter_m, beam_pc_dircos, ext + e)) return rc;
  return PRISIM_OK;
}

// d_bf[e]: the device copy of the element arrays of ext[e] on stream s, null without a beamformer (one null entry when n_ext == 0);
// upload grows by the bytes copied
inline int upload_beamformers(prisim_ctx* ctx, Dev& dev, const prisim_beam_ext* ext, int64_t n_ext, hipStream_t s,
                              std::vector<const double*>& d_bf, int64_t& upload) {
  d_bf.assign((size_t)std::max<int64_t>(n_ext, 1), nullptr);
  for (int64_t e = 0; e < n_ext; ++e) {
    const prisim_beam_ext* x = ext + e;
    if (x->bf_nelem <= 0) continue;
    const size_t np = (size_t)x->bf_nelem * 3, nd = (size_t)x->bf_nelem * x->bf_nrand;
    double* b = nullptr;
    DEV_ALLOC(ctx, dev, b, beamformer_doubles(x) * sizeof(double));
    HIPCHK(ctx, hipMemcpyAsync(b, x->bf_pos, np * 8, hipMemcpyHostToDevice, s));
    HIPCHK(ctx, hipMemcpyAsync(b + np, x->bf_delays, nd * 8, hipMemcpyHostToDevice, s));
    HIPCHK(ctx, hipMemcpyAsync(b + np + nd, x->bf_gains, nd * 8, hipMemcpyHostToDevice, s));
    d_bf[(size_t)e] = b;
    upload += (int64_t)(np + 2 * nd) * 8;
  }
  return PRISIM_OK;
}

// the reference's validity checks of the polynomial beams (primary_beams.py:510-512, :802-807) on the flag the beam kernel sets; the
// streams that ran it are idle
inline int poly_beam_verdict(prisim_ctx* ctx, int32_t beam_kind, const int32_t* d_flag) {
  if (beam_kind != PRISIM_BEAM_POLY) return PRISIM_OK;
  int32_t hflag = 0;
  HIPCHK(ctx, hipMemcpy(&hflag, d_flag, sizeof(int32_t), hipMemcpyDeviceToHost));
  if (hflag & 2)
    return fail(ctx, PRISIM_EINVAL, "Primary beam values were found to be NaN in some case(s). Check if the polynomial equations are valid for the frequencies specified.");
  if (hflag & 1)
    return fail(ctx, PRISIM_EINVAL, "Primary beam exceeds unity by a significant amount. Check the validity of the Primary beam equation for the angles specified.");
  return PRISIM_OK;
}

}  // namespace pint

#endif  // PRISIM_BEAM_SETUP_H
