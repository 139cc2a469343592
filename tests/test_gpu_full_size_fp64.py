"""GPU (-m gpu): the DEFAULT precision at full BASELINE size.  InterferometerArray.observe() runs fp64 unless the caller asks for
memsave (interferometry.py:6182-6185, 6332-6343), and every sky run_prisim.py builds carries the source-shape taper, so what most runs
execute is the grouped fp64 taper kernel (k_skyvis_taper_f64 on 16- / 32-channel tiles), its culling table at exp(-28), the run-by-run
dispatch of a mixed sky (point sources through the fp64 kernel without the taper, rows re-packed as (up, down) pairs) and, with
gradient_mode='baseline', k_skyvis_grad_taper_f64.  Each test checks a body-class sample of baselines against the C oracle at the stated
fp64 tolerance (1e-11 S_f, S_f = sum_s |pbflux[s, f]|), asserts the timing fields that show which path ran, and compares the result
with a second path: exact versus grouped form, cull on versus off, shard versus full array, V(-b) versus conj V(b), source sets
versus the whole sky.  Each prints its measured max error over S_f."""
import os

import numpy as NP
import pytest

from conftest import body_class_sample
from oracle import c_oracle as CO, beams_oracle as BO
from prisim_amd import _abi, workloads as W, geometry as GEOM, sharding
from prisim_amd import interferometry as RI, skymodel as SM

pytestmark = pytest.mark.gpu

TOL64 = 1e-11
ZEN = NP.array([0.0, 0.0, 1.0])


def _kappa(fwhm_deg):
    return float(NP.log(2.0) * (2.0 * NP.sin(0.5 * NP.radians(NP.max(fwhm_deg)))) ** 2)


def _err(v, ref, scale):
    return float(NP.max(NP.abs(v - ref) / scale))


def _with_env(name, value, fn):
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        return fn()
    finally:
        if old is None:
            del os.environ[name]
        else:
            os.environ[name] = old


def _config3_skymodel(sky):
    n = sky['dircos'].shape[0]
    return SM.SkyModel(location=sky['altaz'], flux_ref=sky['flux_ref'], spindex=sky['spindex'], ref_freq=sky['ref_freq'],
                       src_shape=NP.stack((sky['fwhm_deg'], sky['fwhm_deg'], NP.zeros(n)), axis=1))


def _config3_array(bl, ch, lat):
    return RI.InterferometerArray(['b%d' % i for i in range(bl.shape[0])], bl, ch,
                                  telescope={'id': 'hera', 'orientation': [90.0, 270.0], 'ocoords': 'altaz'},
                                  latitude=lat, skycoords='altaz', pointing_coords='hadec')


def test_config3_mixed_sky_fp64_grouped_exact_and_points():
    """BASELINE config 3 as worded (1e4 point sources + nside-128 diffuse map, taper on; 61 075 HERA-350 baselines x 1024 channels) through
    observe(..., memsave=False): the mixed sky runs run by run -- the point sources through k_skyvis_rec<double> on re-packed (up, down)
    rows, the diffuse run through k_skyvis_taper_f64 with `accumulate` set -- on the grouped kernel's 16- / 32-channel tiles.  Checked:
    the body-class sample (fp64 lift threshold) against the C oracle; the sample's baselines negated, as extra rows of the same array,
    against conj V(b); the whole cube against the exact second-order form (PRISIM_HIP_TAPER_F64_GROUP=0).  Then the 1e4 point sources
    alone (k_skyvis_rec<double>; every group lifts on this sky) through the C-ABI against the oracle.  HERA's baselines
    (<= 0.9 km) over nside-128 pixels do not reach the exp(-28) cull threshold: nothing is culled here.  On an MI355X the planner takes
    32-channel tiles and no source split at this size (nsplit 1: the diffuse run accumulates onto the point-source run), 238 of 239
    groups lift, and the grouped sum takes about 1.9 s."""
    cfg = W.config3(with_diffuse=True)
    bl, ch, sky = cfg['baselines'], cfg['channels'], cfg['sky']
    lat = -30.7224
    nbl = bl.shape[0]
    n = sky['dircos'].shape[0]
    npts = int(NP.sum(sky['fwhm_deg'] == 0.0))
    assert n > 100000 and npts == 10000 and NP.all(sky['fwhm_deg'][:npts] == 0.0)     # one point-source run, then the diffuse run
    sel, lift = body_class_sample(bl, ch, sky['dircos'], ZEN, f32=False, kappa=_kappa(sky['fwhm_deg']))
    assert sel.size >= 12 and lift.any() and (~lift).any() and sel[-1] == nbl - 1
    skymod = _config3_skymodel(sky)
    bl_run = NP.vstack((bl, -bl[sel]))
    ia = _config3_array(bl_run, ch, lat)

    def observe():
        ia.observe((2457000.5, 0.0), {'Tnet': 100.0}, NP.ones(ch.size), [0.0, lat], skymod, 10.7, memsave=False)
        tm = ia._ctx.timing()
        vis = ia._ctx.get_vis(slot=0)
        return vis, tm

    grouped, tm = observe()
    print('config 3 fp64 (grouped): timing', tm)
    assert tm['last_terms'] == bl_run.shape[0] * ch.size * n
    assert tm['last_chan_tile'] in (16, 32), tm                          # the grouped fp64 taper kernel's tiles
    ng = (nbl + 255) // 256
    # the whole sky's max|s - s_pc| (horizon pixels) keeps the ragged last group off the lift: both bodies of both kernels run
    assert tm['last_lift_groups'] == int(lift.sum()) and 0 < tm['last_lift_groups'] < ng, tm
    pb = BO.airy_disk_pattern(14.0, sky['altaz'], ch, pointing_altaz=[90.0, 270.0]) * skymod.generate_spectrum(frequency=ch)
    scale = NP.sum(NP.abs(pb), axis=0)[None, :]
    ref = CO.skyvis(bl[sel], ch, sky['dircos'], pb, ZEN, fwhm_deg=sky['fwhm_deg'])
    err = _err(grouped[sel], ref, scale)
    err_conj = _err(grouped[nbl:], NP.conj(grouped[sel]), scale)
    print('config 3 fp64: max err / S_f = %.3e against the oracle (%d baselines), %.3e for V(-b) - conj V(b)' % (err, sel.size, err_conj))
    assert err <= TOL64
    assert err_conj <= TOL64
    exact, tm_exact = _with_env('PRISIM_HIP_TAPER_F64_GROUP', '0', observe)
    assert tm_exact['last_chan_tile'] == tm['last_chan_tile'], tm_exact
    err_form = _err(exact, grouped, scale)
    print('config 3 fp64: grouped vs exact second-order form, whole cube: max diff / S_f = %.3e' % err_form)
    assert err_form <= 1e-12
    del grouped, exact, ia
    # the point sources alone, no taper: k_skyvis_rec<double>.  They stand within a smaller max|s - s_pc| than the diffuse map, and
    # at fp64's 1/4-cycle threshold every group of the array lifts (the plain body ran in the mixed pass above)
    pts = slice(0, npts)
    with _abi.Context(0) as ctx:
        ctx.set_array(bl, ch)
        ctx.set_sky_analytic(sky['dircos'][pts], sky['flux_ref'][pts], sky['spindex'][pts], sky['ref_freq'], _abi.PRISIM_BEAM_AIRY, 14.0,
                             ZEN, ZEN)
        ctx.compute(precision=_abi.PRISIM_FP64)
        tp = ctx.timing()
        vis = ctx.get_vis()
        pbp = ctx.get_pbflux()
    print('config 3 points fp64: timing', tp)
    selp, liftp = body_class_sample(bl, ch, sky['dircos'][pts], ZEN, f32=False)
    assert tp['last_terms'] == nbl * ch.size * npts and tp['last_taper_group'] == 0, tp
    assert tp['last_lift_groups'] == int(liftp.sum()) == ng, tp
    refp = CO.skyvis(bl[selp], ch, sky['dircos'][pts], pbp, ZEN)
    errp = _err(vis[selp], refp, NP.sum(NP.abs(pbp), axis=0)[None, :])
    print('config 3 points fp64: max err / S_f = %.3e (%d baselines, %d of %d groups lifting)' % (errp, selp.size, tp['last_lift_groups'], ng))
    assert errp <= TOL64
    del vis


def test_config3_mixed_sky_fp64_baseline_gradient():
    """Config 3 as worded with gradient_mode='baseline' at fp64: k_skyvis_grad_taper_f64 on the diffuse run (with the point-source run
    beside it), on the full array and all 1024 channels.  V and the three baseline-gradient sums (interferometry.py:6330, 6338, 6343) on
    the body-class sample against the C oracle's gradient entry (oracle_skyvis_grad_f64).  The sky is the full nside-128 one: the
    gradient sum takes about 4.0 s on an MI355X (32-channel tiles, nsplit 1)."""
    cfg = W.config3(with_diffuse=True)
    bl, ch, sky = cfg['baselines'], cfg['channels'], cfg['sky']
    lat = -30.7224
    skymod = _config3_skymodel(sky)
    ia = _config3_array(bl, ch, lat)
    ia.observe((2457000.5, 0.0), {'Tnet': 100.0}, NP.ones(ch.size), [0.0, lat], skymod, 10.7, memsave=False, gradient_mode='baseline')
    tm = ia._ctx.timing()
    print('config 3 fp64 gradient: timing', tm)
    assert tm['last_terms'] == bl.shape[0] * ch.size * sky['dircos'].shape[0]
    vis, grad = ia._ctx.get_vis(slot=0, want_grad=True)
    assert vis.dtype == NP.complex128 and grad.shape == (3,) + vis.shape
    sel, _ = body_class_sample(bl, ch, sky['dircos'], ZEN, f32=False, kappa=_kappa(sky['fwhm_deg']))
    vis, grad = vis[sel], grad[:, sel]
    del ia
    pb = BO.airy_disk_pattern(14.0, sky['altaz'], ch, pointing_altaz=[90.0, 270.0]) * skymod.generate_spectrum(frequency=ch)
    scale = NP.sum(NP.abs(pb), axis=0)[None, :]
    ref, gref = CO.skyvis(bl[sel], ch, sky['dircos'], pb, ZEN, fwhm_deg=sky['fwhm_deg'], gradient=True)
    errs = [_err(vis, ref, scale)] + [_err(grad[k], gref[k], scale) for k in range(3)]
    print('config 3 fp64 gradient: max err / S_f = %.3e (V), %.3e %.3e %.3e (grad x y z), %d baselines' % (tuple(errs) + (sel.size,)))
    assert max(errs) <= TOL64, errs
    assert NP.max(NP.abs(gref[2])) > 0.0


def test_config4_fp64_culling_full_array_and_last_shard():
    """Config 4 (MWA-128T, 8128 baselines to 2.5 km x 768 channels at 185 MHz, nside-64 diffuse sky, external HEALPix beam), one snapshot
    at fp64.  observe() lists the sources by decreasing altitude and the fp64 cull table (exp(-28) of S_f) lets the long-baseline groups
    skip their zenith-most sources.  Checked: culled fraction > 0.05; the body-class sample (with the culling groups) against the C oracle;
    the whole cube against a rerun with culling off (PRISIM_HIP_TAPER_CULL=0) at the cull bound 1e-12.  Then the baselines of the last
    rank of 8 (sharding.shard_index(8128, 8, 7): four groups of 254 dealt round-robin, the array's longest included, 1016 baselines in
    four kernel groups with a ragged last one): the planner splits the sources (last_nsplit > 1), so every run writes its own partial
    cubes and the culled prefix meets split starts; its rows equal the full array's at 2e-12 (each side within exp(-28) S_f of the uncut
    sum under its own group layout) and its own body-class sample matches the oracle.  Observed on an MI355X: the full array splits its
    sources too (nsplit 5, 12 % culled), the shard takes nsplit 16 (19 % culled), both on 32-channel tiles."""
    from oracle import healpix_oracle as H
    cfg = W.config4(n_acc=1)
    bl, ch, sky, lat = cfg['baselines'], cfg['channels'], cfg['sky'], cfg['latitude']
    kappa = _kappa(sky['fwhm_deg'])
    lst0 = 40.0
    hadec = GEOM.altaz2hadec(sky['altaz'], lat, units='degrees')
    radec = NP.stack(((lst0 - hadec[:, 0]) % 360.0, hadec[:, 1]), axis=1)
    nsky = radec.shape[0]
    skymod = SM.SkyModel(location=radec, flux_ref=sky['flux_ref'], spindex=sky['spindex'], ref_freq=sky['ref_freq'],
                         src_shape=NP.stack((sky['fwhm_deg'], sky['fwhm_deg'], NP.zeros(nsky)), axis=1), epoch=None)
    dc, altaz, keep = W.drift_snapshot_directions(sky, lat, 0.0)
    flux = sky['flux_ref'][keep, None] * (ch[None, :] / sky['ref_freq']) ** sky['spindex'][keep, None]
    # the reference stores a supplied beam as float32 (interferometry.py:4466) before pb * fluxes (:6254): so does the checker
    beam = H.external_beam(cfg['beam_table'], cfg['beam_freqs'], NP.pi / 2 - NP.radians(altaz[:, 0]), NP.radians(altaz[:, 1]), ch)
    pb = beam.astype(NP.float32).astype(NP.float64) * flux
    fw = sky['fwhm_deg'][keep]
    scale = NP.sum(NP.abs(pb), axis=0)[None, :]

    def make(bl_):
        ia = RI.InterferometerArray(['b%d' % i for i in range(bl_.shape[0])], bl_, ch, telescope={'id': 'mwa'}, latitude=lat,
                                    skycoords='radec', pointing_coords='hadec')
        ia.set_external_beam(cfg['beam_table'], cfg['beam_freqs'], spec_interp='cubic')
        return ia

    def observe(ia):
        ia.observe((2457000.5, lst0), {'Tnet': 100.0}, NP.ones(ch.size), [0.0, lat], skymod, cfg['t_acc'], memsave=False)
        assert NP.array_equal(ia.obs_catalog_indices[-1], NP.flatnonzero(keep))
        return ia._ctx.get_vis(slot=0), ia._ctx.timing()

    sel, _ = body_class_sample(bl, ch, dc, ZEN, f32=False, kappa=kappa)
    ia = make(bl)
    full, tm = observe(ia)
    print('config 4 fp64 full array: timing', tm)
    culled = tm['last_culled_fraction']
    print('config 4 fp64: taper culling skipped %.2f %% of the (source, baseline) pairs' % (100 * culled))
    assert culled > 0.05
    err = _err(full[sel], CO.skyvis(bl[sel], ch, dc, pb, ZEN, fwhm_deg=fw), scale)
    print('config 4 fp64 full array: max err / S_f = %.3e (%d baselines)' % (err, sel.size))
    assert err <= TOL64
    uncut, tm_uncut = _with_env('PRISIM_HIP_TAPER_CULL', '0', lambda: observe(ia))
    assert tm_uncut['last_culled_fraction'] == 0.0, tm_uncut
    err_cull = _err(full, uncut, scale)
    print('config 4 fp64: cull on vs off, whole cube: max diff / S_f = %.3e' % err_cull)
    assert err_cull <= 1e-12
    del uncut, ia
    # the last rank of 8
    shard = sharding.shard_index(bl.shape[0], 8, 7)
    assert shard.size == 1016 and shard[-1] == bl.shape[0] - 1
    bls = bl[shard]
    ias = make(bls)
    part, tms = observe(ias)
    print('config 4 fp64 shard 7 of 8: timing', tms)
    print('config 4 fp64 shard 7 of 8: last_nsplit = %d, culled %.2f %%' % (tms['last_nsplit'], 100 * tms['last_culled_fraction']))
    assert tms['last_nsplit'] > 1, tms
    assert tms['last_culled_fraction'] > 0.05, tms
    err_shard = _err(part, full[shard], scale)
    print('config 4 fp64 shard 7 of 8: rows vs the full array: max diff / S_f = %.3e' % err_shard)
    assert err_shard <= 2e-12
    sels, _ = body_class_sample(bls, ch, dc, ZEN, f32=False, kappa=kappa)
    err_s = _err(part[sels], CO.skyvis(bls[sels], ch, dc, pb, ZEN, fwhm_deg=fw), scale)
    print('config 4 fp64 shard 7 of 8: max err / S_f = %.3e (%d baselines)' % (err_s, sels.size))
    assert err_s <= TOL64
    del part, full, ias


def test_config5_snapshot_fp64():
    """One snapshot of config 5 at fp64 through the C-ABI (HERA-350 x 1024 channels x the nside-256 diffuse sky above the horizon,
    392 704 sources of one size, taper on): one chain of the grouped fp64 kernel per 16- / 32-channel tile over the whole sky, lifting
    and plain bodies chosen at fp64's 1/4-cycle threshold.  Checked: the body-class sample against the C oracle, and additivity over two
    disjoint source sets (two runs of the grouped kernel with other chain lengths against the one)."""
    cfg = W.config5(n_acc=1)
    bl, ch, sky = cfg['baselines'], cfg['channels'], cfg['sky']
    n = sky['dircos'].shape[0]
    assert n > 390000
    with _abi.Context(0) as ctx:
        ctx.set_array(bl, ch)

        def run(s):
            ctx.set_sky_analytic(sky['dircos'][s], sky['flux_ref'][s], sky['spindex'][s], sky['ref_freq'], _abi.PRISIM_BEAM_AIRY, 14.0,
                                 ZEN, ZEN, fwhm_deg=sky['fwhm_deg'][s])
            ctx.compute(precision=_abi.PRISIM_FP64)
            return ctx.get_vis(), ctx.timing()

        full, tm = run(slice(None))
        print('config 5 fp64: timing', tm)
        assert tm['last_chan_tile'] in (16, 32) and tm['last_terms'] == bl.shape[0] * ch.size * n, tm
        pb = ctx.get_pbflux()
        odd = NP.arange(n) % 3 == 1
        a, _ = run(odd)
        b, _ = run(~odd)
        parts = a + b
        del a, b
    assert NP.all(NP.isfinite(full.view(NP.float64)))
    scale = NP.sum(NP.abs(pb), axis=0)[None, :]
    sel, lift = body_class_sample(bl, ch, sky['dircos'], ZEN, f32=False)
    assert sel.size >= 12 and lift.any() and (~lift).any()
    assert tm['last_lift_groups'] == int(lift.sum()), tm
    err = _err(full[sel], CO.skyvis(bl[sel], ch, sky['dircos'], pb, ZEN, fwhm_deg=sky['fwhm_deg']), scale)
    err_add = _err(parts, full, scale)
    print('config 5 fp64: max err / S_f = %.3e (%d baselines); source sets vs whole sky: %.3e' % (err, sel.size, err_add))
    assert err <= TOL64
    assert err_add <= TOL64
    del full, parts
