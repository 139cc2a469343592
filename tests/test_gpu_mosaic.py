"""GPU: the beam-weighted mosaic of the snapshots on the device (include/prisim_mosaic.h) -- through the C-ABI against the numpy
checker (tests/mosaic_checker.py), against prisim_dirty_image for a delta beam, the horizon and the pbmin mask, the bit equality
between budgets, streams and the resident cube, the refusals, and through prisim_amd.interferometry.ApertureSynthesis on a drift scan
that observe() simulated.

Bounds, the project's own: the image sums are held to 1e-11 of their natural scale (tests/test_gpu_imaging.py) and the device beams to
1e-12 absolute against oracle.beams_oracle (tests/test_gpu_antpower.py), so per element
    |N - N_ref| <= 1e-11 sum_t A_ref sum_b w|V| + 1e-12 sum_{t,b} w|V|
    |Q - Q_ref| <= 1e-11 sum_t A_ref^2 W_t + 2e-12 sum_t A_ref W_t.
The quotient, the mask and the effective beam are asserted exactly: recomputed in numpy from the returned num, den and wsum with the
expressions of the header and compared with array_equal, NaN positions included.  No element is left out of any comparison."""
import ctypes as C
import os
import sys

import numpy as NP
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import imaging_cases as IC  # noqa: E402
import imaging_checker as IK  # noqa: E402
import mosaic_cases as MC  # noqa: E402
import mosaic_checker as MK  # noqa: E402

from prisim_amd import _abi, skymodel as SM  # noqa: E402
from prisim_amd import interferometry as RI  # noqa: E402

pytestmark = pytest.mark.gpu
K = 32
SHAPES = [(1, 1, 1, 1), (37, 5, 63, 1), (300, 70, 65, 3), (37, K + 1, 1000, 3)]
BEAMS = ['gaussian', 'airy', 'dipole_ground', 'beamformer']


def call(ctx, c, beam, weights=None, **kw):
    kind, dia, ext, _ = beam
    return ctx.mosaic_image(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], kind, dia, ext=ext, cube=kw.pop('cube', c['cube']),
                            weights=weights, aberr_beta=c['beta'], **kw)


def same(a, b):
    return NP.array_equal(a, b, equal_nan=True)


def held_to_the_checker(got, ref, pbmin, chan_avg, label):
    """num and den within their bounds, and mosaic and pb_eff exactly what the header's expressions make of num, den and wsum"""
    mosaic, num, den, wsum, st = got
    for what, have, want, bound in (('num', num, ref['num'], ref['bound_num']), ('den', den, ref['den'], ref['bound_den'])):
        err = NP.abs(have - want)
        with NP.errstate(invalid='ignore', divide='ignore'):
            worst = float(NP.nanmax(NP.where(bound > 0.0, err / bound, NP.where(err > 0.0, NP.inf, 0.0))))
        print('%s %s: max err / bound = %.3e' % (label, what, worst))
        assert NP.all(err <= bound), (label, what, worst)
    assert NP.allclose(wsum, ref['wsum'], rtol=1e-13, atol=0)
    want_mosaic, want_eff = MK.quotient(num, den, wsum, pbmin, chan_avg)
    assert mosaic.shape == want_mosaic.shape and same(mosaic, want_mosaic), label
    assert same(st['pb_eff'], want_eff), label


# ---- M1: parity -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(str(v) for v in s))
def test_m1_entry_against_the_checker(ctx, shape):
    nbl, nchan, npix, nt = shape
    c = IC.case(nbl, nchan, npix, nt)
    beams = MC.beam_setups(nt)
    assert len(beams['beamformer'][2]) == nt                          # n_ext == nt
    if nbl >= 7:
        assert NP.count_nonzero(c['w_bl'] == 0.0) == nbl // 7
    A = None
    for form, weights in (('none', None), ('baseline', c['w_bl']), ('full', c['w_full'])):
        sums = MK.snapshot_sums(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], c['cube'], weights=weights, aberr_beta=c['beta'])
        if A is None:
            A = {name: MK.beams(sums['s'], c['freqs'], beams[name][3]) for name in BEAMS}       # once per shape
        for name in BEAMS:
            ref = MK.combine(sums, A[name])
            for chan_avg in (False, True):
                for route in ('direct', 'stepped'):
                    got = call(ctx, c, beams[name], weights=weights, chan_avg=chan_avg, route=route)
                    st = got[4]
                    assert st['route'] == route and st['terms'] == npix * nbl * nchan * nt and st['chan_tile'] == K and st['block_pixels'] == 256
                    assert st['reseed'] == (K if route == 'stepped' else 1) and st['resident'] is False and st['beam_values'] == npix * nchan * nt
                    assert st['pixel_bytes'] == 64 * nt + 24 * nchan + (16 if chan_avg else 16 * nchan)
                    held_to_the_checker(got, ref, 0.1, chan_avg, '%s %s weights=%s chan_avg=%d %s' % (shape, name, form, chan_avg, route))
    # AUTO on this uniform grid is the stepped route, bit for bit
    auto = call(ctx, c, beams['airy'], weights=c['w_full'])
    assert auto[4]['route'] == 'stepped' and same(auto[0], call(ctx, c, beams['airy'], weights=c['w_full'], route='stepped')[0])


def test_m1_non_uniform_grid_is_direct_and_refuses_the_stepped_route(ctx):
    c = IC.case(37, 70, 65, 3, uniform=False)
    beam = MC.beam_setups(3)['gaussian']
    ref = MK.mosaic(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], c['cube'], beam[3], weights=c['w_full'], aberr_beta=c['beta'])
    got = call(ctx, c, beam, weights=c['w_full'])
    assert got[4]['route'] == 'direct' and got[4]['reseed'] == 1
    held_to_the_checker(got, ref, 0.1, False, 'non-uniform grid, auto')
    with pytest.raises(ValueError, match='uniform'):
        call(ctx, c, beam, weights=c['w_full'], route='stepped')
    assert same(call(ctx, c, beam, weights=c['w_full'], route='direct')[0], got[0])       # and the context goes on as before


# ---- M2: a delta beam on one snapshot is the dirty image ----------------------------------------------------------------------------------

def test_m2_delta_beam_on_one_snapshot_has_the_bits_of_the_dirty_image(ctx):
    c = MC.up_case(37, K + 1, 300, 1)
    assert NP.min(IK.directions(c['unitvec'], c['rot'], c['beta'])[..., 2]) > 0.04
    delta = MC.beam_setups(1)['delta']
    for scale in (1.0, 1000.0):                                       # to 300 m, and to 300 km where tests/imaging_reference.py holds the image
        c = dict(c, baselines=c['baselines'] * scale)
        for weights in (None, c['w_bl'], c['w_full']):
            for route in ('direct', 'stepped'):
                for chan_avg in (False, True):
                    mosaic, num, den, wsum, st = call(ctx, c, delta, weights=weights, route=route, chan_avg=chan_avg)
                    img, wimg, _ = ctx.dirty_image(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], cube=c['cube'], weights=weights,
                                                   aberr_beta=c['beta'], route=route, chan_avg=chan_avg)
                    assert NP.all(NP.isfinite(img)) and NP.array_equal(mosaic, img), (scale, route, chan_avg)
                    assert NP.array_equal(den, NP.broadcast_to(wsum, den.shape))
                    assert chan_avg or NP.array_equal(wsum, wimg)
                    assert NP.array_equal(st['pb_eff'], NP.ones_like(mosaic))


# ---- M3: the horizon and the mask -----------------------------------------------------------------------------------------------------------

def test_m3_a_snapshot_below_the_horizon_contributes_exactly_nothing(ctx):
    c = MC.up_case(37, K + 1, 65, 3, flip=(1,))
    s = IK.directions(c['unitvec'], c['rot'], c['beta'])
    assert NP.min(s[0, :, 2]) > 0.04 and NP.max(s[1, :, 2]) < -0.04 and NP.min(s[2, :, 2]) > 0.04
    less = c['w_full'].copy()
    less[1] = 0.0
    for name in ('delta', 'airy'):
        beam = MC.beam_setups(3)[name]
        for route in ('direct', 'stepped'):
            full = call(ctx, c, beam, weights=c['w_full'], route=route, pbmin=0.0)
            cut = call(ctx, c, beam, weights=less, route=route, pbmin=0.0)
            assert NP.all(NP.isfinite(full[0])) and NP.array_equal(full[1], cut[1]) and NP.array_equal(full[2], cut[2])
            assert NP.array_equal(full[0], cut[0]) and not NP.array_equal(full[3], cut[3])      # the same mosaic under another weight sum


def test_m3_below_the_horizon_in_every_snapshot_is_nan(ctx):
    c = MC.up_case(37, K + 1, 65, 3, down=20)
    s = IK.directions(c['unitvec'], c['rot'], c['beta'])
    up = NP.arange(65) < 45
    assert NP.min(s[:, up, 2]) > 0.04 and NP.max(s[:, ~up, 2]) < -0.04
    for name in ('delta', 'gaussian'):
        beam = MC.beam_setups(3)[name]
        for chan_avg in (False, True):
            mosaic, num, den, wsum, st = call(ctx, c, beam, weights=c['w_bl'], pbmin=0.0, chan_avg=chan_avg)
            assert NP.all(NP.isnan(mosaic[~up])) and NP.all(NP.isfinite(mosaic[up]))
            assert NP.all(num[~up] == 0.0) and NP.all(den[~up] == 0.0) and NP.all(den[up] > 0.0) and NP.all(st['pb_eff'][~up] == 0.0)


def test_m3_the_pbmin_mask(ctx):
    c = MC.mask_case()
    beam = MC.beam_setups(3)['gaussian']
    ref = MK.mosaic(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], c['cube'], beam[3], weights=c['w_full'], aberr_beta=c['beta'],
                    pbmin=MC.MASK_PBMIN)
    MK.assert_mask_is_decided(ref, MC.MASK_PBMIN)
    for route in ('direct', 'stepped'):
        got = call(ctx, c, beam, weights=c['w_full'], pbmin=MC.MASK_PBMIN, route=route)
        held_to_the_checker(got, ref, MC.MASK_PBMIN, False, 'mask ' + route)
        assert NP.array_equal(NP.isnan(got[0]), NP.isnan(ref['mosaic']))
        assert NP.array_equal(NP.isnan(got[0]), got[4]['pb_eff'] < MC.MASK_PBMIN)


def test_m3_a_channel_without_weight_is_nan_and_nothing_else_is(ctx):
    c = MC.up_case(37, 70, 65, 3)
    w = c['w_full'].copy()
    w[:, :, 41] = 0.0
    live = NP.arange(70) != 41
    beam = MC.beam_setups(3)['gaussian']
    for route in ('direct', 'stepped'):
        mosaic, num, den, wsum, st = call(ctx, c, beam, weights=w, route=route, pbmin=0.0)
        assert NP.array_equal(NP.isnan(mosaic), NP.broadcast_to(~live, mosaic.shape)) and wsum[41] == 0.0 and NP.all(wsum[live] >= 1.0)
        assert NP.all(NP.isnan(st['pb_eff'][:, 41])) and NP.all(NP.isfinite(st['pb_eff'][:, live]))
        band = call(ctx, c, beam, weights=w, route=route, pbmin=0.0, chan_avg=True)
        assert NP.all(NP.isfinite(band[0])) and same(band[0], MK.quotient(num, den, wsum, 0.0, True)[0])


# ---- M4: the same bits however it is streamed -------------------------------------------------------------------------------------------------

def test_m4_budget_streams_and_the_resident_cube_leave_the_bits_unchanged(ctx):
    c = IC.case(37, K + 1, 1000, 3)
    beam = MC.beam_setups(3)['airy']
    for chan_avg in (False, True):
        one_block = 256 * (64 * 3 + 24 * (K + 1) + (16 if chan_avg else 16 * (K + 1)))
        for route in ('direct', 'stepped'):
            full = call(ctx, c, beam, weights=c['w_full'], route=route, chan_avg=chan_avg)
            assert full[4]['chunks'] == 1 and full[4]['streams'] == 1
            for budget, streams in ((one_block, 1), (2 * one_block, 2)):
                got = call(ctx, c, beam, weights=c['w_full'], route=route, chan_avg=chan_avg, budget_bytes=budget)
                assert got[4]['chunks'] == 4 and got[4]['chunk_pixels'] == 256 and got[4]['streams'] == streams
                assert all(same(x, y) for x, y in zip(full[:4], got[:4])) and same(full[4]['pb_eff'], got[4]['pb_eff']), (route, chan_avg, streams)
            with pytest.raises(ValueError, match='cannot hold one block'):
                call(ctx, c, beam, weights=c['w_full'], route=route, chan_avg=chan_avg, budget_bytes=one_block - 1)
    host = call(ctx, c, beam, weights=c['w_bl'])
    ctx.set_array(c['baselines'], c['freqs'], nt_max=3)
    for t in range(3):
        ctx.set_vis(NP.ascontiguousarray(c['cube'][t]), slot=t)
    res = call(ctx, c, beam, weights=c['w_bl'], cube=None)
    assert res[4]['resident'] is True and all(same(x, y) for x, y in zip(host[:4], res[:4]))
    # one shared ext against three copies of it
    kind, dia, ext, _ = MC.beam_setups(3)['dipole_ground']
    one = call(ctx, c, (kind, dia, ext, None), weights=c['w_bl'])
    three = call(ctx, c, (kind, dia, [ext] * 3, None), weights=c['w_bl'])
    assert all(same(x, y) for x, y in zip(one[:4], three[:4]))
    # one element pointing against three copies of it, and a pointing that moves against the checker
    kind, dia, ext, setup = MC.beam_setups(3)['gaussian']
    zen = NP.array([0.0, 0.0, 1.0])
    args = (c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], kind, dia)
    kw = dict(cube=c['cube'], weights=c['w_bl'], aberr_beta=c['beta'])
    assert all(same(x, y) for x, y in zip(ctx.mosaic_image(*args, beam_pc_dircos=zen, **kw)[:4],
                                          ctx.mosaic_image(*args, beam_pc_dircos=NP.repeat(zen[None], 3, axis=0), **kw)[:4]))
    moving = IC.unit(NP.array([[0.0, 0.0, 1.0], [0.3, 0.1, 1.0], [-0.2, 0.4, 1.0]]))
    ref = MK.mosaic(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], c['cube'], MK.setups_of(kind, dia, moving, None, 3),
                    weights=c['w_bl'], aberr_beta=c['beta'])
    held_to_the_checker(ctx.mosaic_image(*args, beam_pc_dircos=moving, **kw), ref, 0.1, False, 'a pointing that moves')


# ---- M5: refusals ---------------------------------------------------------------------------------------------------------------------------

def test_m5_refusals_write_nothing(ctx):
    c = IC.case(37, K + 1, 65, 3)
    odd = IC.case(37, K + 1, 65, 3, uniform=False)
    p, lib, h = _abi._ptr, ctx._lib, ctx._h
    rot = NP.ascontiguousarray(c['rot'].reshape(-1, 9))
    outs = [NP.full((65, K + 1), -7.0) for _ in range(4)] + [NP.full(K + 1, -7.0)]
    good_ext = _abi.make_beam_ext({'dipole_dircos': [1.0, 0.0, 0.0]})
    bad_ext = _abi.make_beam_ext({'dipole_dircos': [1.0, 0.0, 0.0]})
    bad_ext.dipole_mode = 17

    def entry(mosaic=True, null=False, **kw):
        a = ctx.PrisimMosaicArgs()
        v = dict(npix=65, nbl=37, nchan=K + 1, nt=3, unitvec=c['unitvec'], rot=rot, aberr_beta=c['beta'], pc_dircos=c['pc'],
                 baselines=c['baselines'], freqs_hz=c['freqs'], cube=c['cube'], weights=c['w_full'], weight_form=2, chan_avg=0, route=-1,
                 beam_kind=_abi.PRISIM_BEAM_AIRY, diameter_m=MC.beam_setups(3)['airy'][1], pbmin=0.1, budget_bytes=0)
        v.update(kw)
        keep = []
        for name, val in v.items():
            if isinstance(val, NP.ndarray):
                val = NP.ascontiguousarray(val)
                keep.append(val)
                val = p(val)
            setattr(a, name, val)
        a.beam_pc_dircos[:] = [0.0, 0.0, 1.0]
        rc = lib.prisim_mosaic_image(h, None if null else C.byref(a), p(outs[0]) if mosaic else None, p(outs[1]), p(outs[2]), p(outs[3]),
                                     p(outs[4]), None)
        return rc, lib.prisim_hip_last_error(h).decode()

    def changed(name, index, value):
        x = NP.array(rot if name == 'rot' else c[name], dtype=NP.float64)
        x[index] = value
        return x

    one_block = 256 * (64 * 3 + 24 * (K + 1) + 16 * (K + 1))
    ext_of = lambda x: C.cast(C.pointer(x), C.c_void_p)               # noqa: E731
    refusals = [({'null': True}, 'argument struct is NULL'), ({'mosaic': False}, 'out_mosaic is NULL'),
                # those of prisim_dirty_image
                ({'unitvec': None}, 'unitvec is NULL'), ({'rot': None}, 'rot is NULL'), ({'pc_dircos': None}, 'pc_dircos is NULL'),
                ({'baselines': None}, 'baselines is NULL'), ({'freqs_hz': None}, 'freqs_hz is NULL'), ({'weights': None}, 'weights is NULL'),
                ({'npix': 0}, '>= 1'), ({'nbl': 0}, '>= 1'), ({'nchan': -1}, '>= 1'), ({'nt': 0}, '>= 1'), ({'nchan': (1 << 20) + 1}, '2^20'),
                ({'npix': 1 << 45}, '2^46'), ({'route': 2}, 'unknown route'), ({'route': -2}, 'unknown route'),
                ({'weight_form': 3}, 'unknown weight form'), ({'chan_avg': 2}, 'chan_avg'),
                ({'unitvec': changed('unitvec', (3, 0), 1.5)}, 'unitvec[3]'), ({'rot': changed('rot', (1, 4), 0.5)}, 'rot of snapshot 1'),
                ({'aberr_beta': changed('beta', (2, 1), 0.02)}, 'aberr_beta of snapshot 2'),
                ({'pc_dircos': changed('pc', (0, 2), 1.1)}, 'pc_dircos of snapshot 0'),
                ({'freqs_hz': changed('freqs', 5, 0.0)}, 'freqs_hz[5]'), ({'freqs_hz': changed('freqs', 5, NP.inf)}, 'freqs_hz[5]'),
                ({'weights': changed('w_full', (1, 2, 3), -1.0)}, 'finite and non-negative'),
                ({'weights': changed('w_full', (1, 2, 3), NP.nan)}, 'finite and non-negative'),
                ({'baselines': changed('baselines', (4, 1), NP.nan)}, 'baseline 4'),
                ({'budget_bytes': one_block - 1}, 'cannot hold one block'), ({'freqs_hz': odd['freqs'], 'route': 1}, 'uniform'),
                # those of prisim_antenna_power for the beam
                ({'n_ext': 2, 'ext': ext_of(good_ext)}, 'n_ext must be 0, 1 or nt'), ({'n_ext': 1}, 'ext is NULL'),
                ({'beam_kind': 9}, 'unknown beam_kind'), ({'diameter_m': 0.0}, 'diameter_m must be positive'),
                ({'beam_kind': _abi.PRISIM_BEAM_DIPOLE}, 'PRISIM_BEAM_DIPOLE needs'),
                ({'n_ext': 1, 'ext': ext_of(bad_ext)}, 'unknown dipole_mode'),
                ({'beam_pc_snap': NP.array([[0.0, 0.0, 1.0], [0.0, NP.nan, 1.0], [0.0, 0.0, 1.0]])}, 'beam_pc_snap of snapshot 1'),
                # its own
                ({'pbmin': -0.1}, 'pbmin'), ({'pbmin': 1.0}, 'pbmin'), ({'pbmin': NP.nan}, 'pbmin'), ({'pbmin': NP.inf}, 'pbmin')]
    for kw, msg in refusals:
        rc, err = entry(**kw)
        assert rc == _abi.PRISIM_EINVAL and msg in err, (list(kw), rc, err)
        assert all(NP.all(o == -7.0) for o in outs), list(kw)         # nothing is written unless the call succeeds
    # the validity messages of the polynomial beams come after the kernels have run: still nothing is written
    for coef, text in (([5.0, 0.0, 0.0, 0.0], 'exceeds unity'), ([NP.nan, 0.0, 0.0, 0.0], 'found to be NaN')):
        x = _abi.make_beam_ext({'poly': coef})
        rc, err = entry(beam_kind=_abi.PRISIM_BEAM_POLY, n_ext=1, ext=ext_of(x))
        assert rc == _abi.PRISIM_EINVAL and text in err and all(NP.all(o == -7.0) for o in outs), (text, err)
    with _abi.Context(0) as fresh:
        with pytest.raises(RuntimeError, match='no resident'):
            call(fresh, c, MC.beam_setups(3)['airy'], cube=None)      # PRISIM_ESTATE: no array was ever set
    rc, err = entry(budget_bytes=one_block)
    assert rc == _abi.PRISIM_OK, err
    want = call(ctx, c, MC.beam_setups(3)['airy'], weights=c['w_full'])
    assert same(outs[0], want[0]) and same(outs[1], want[4]['pb_eff']) and same(outs[2], want[1]) and same(outs[3], want[2])
    assert same(outs[4], want[3])


# ---- M6: end to end ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('coords', ['radec', 'altaz'])
def test_m6_a_drift_scan_returns_the_flux_of_the_catalogue(coords):
    """observe() simulates one source through a 14 m Gaussian beam that stays at the zenith while the sky drifts by; the mosaic at
    the source's position is its flux, the dirty image there is not."""
    S, nbl, nt = MC.FLUX, 37, 3
    src = MC.SOURCE_RADEC if coords == 'radec' else MC.SOURCE_ALTAZ
    sky = SM.SkyModel(location=src, flux_ref=[S], spindex=[0.0], ref_freq=150e6)
    bl = MC.e2e_baselines(nbl)
    ia = RI.InterferometerArray([(str(i + 1), '0') for i in range(nbl)], bl, MC.CH, telescope=MC.GAUSS14, latitude=MC.LAT, skycoords=coords,
                                pointing_coords='altaz')
    ia.frame_model = 'date'
    for j in range(nt):
        ia.observe((MC.JD0 + j / 64.0, MC.LSTS[j]), {'Tnet': 200.0}, NP.ones(MC.CH.size), MC.ZENITH, sky, 10.7)
    aps = RI.ApertureSynthesis(ia)
    others = NP.stack((src[0, 0] + NP.linspace(-3.0, 3.0, 8), src[0, 1] + NP.linspace(2.0, -2.0, 8)), axis=1)
    dirs = NP.vstack((src, others))
    mosaic = aps.mosaic(dirs, coords=coords)
    st = aps.image_stats
    assert mosaic.shape == (9, MC.CH.size) and st['route'] == 'stepped' and st['num'].shape == st['den'].shape == (9, MC.CH.size)
    assert st['wsum'].shape == (MC.CH.size,) and st['pb_eff'].shape == mosaic.shape and st['terms'] == 9 * nbl * MC.CH.size * nt
    # the bound, from the checker on the very cube observe() left
    uv, rot, beta, pc, _, _ = aps._prepare('dirty', dirs, coords, 'noiseless', None, None, 'auto')
    cube = NP.transpose(NP.asarray(ia.skyvis_freq), (2, 0, 1))
    ref = MK.mosaic(uv, rot, pc, bl, MC.CH, cube, {'element': 'gaussian', 'size': 14.0}, aberr_beta=beta)
    A = ref['A'][:, 0, :]
    assert 0.2 < A.min() and A.max() < 0.9 and (coords == 'altaz' or A[0].max() < 0.8 * A[2].min())      # well off the centre, and drifting
    bound = (ref['bound_num'][0] + S * ref['bound_den'][0]) / ref['den'][0]
    dev = NP.abs(mosaic[0] - S)
    print('%s: |mosaic - S| is at most %.3e, %.3e of its bound' % (coords, dev.max(), float(NP.max(dev / bound))))
    assert NP.all(dev <= bound), float(NP.max(dev / bound))
    assert same(mosaic, MK.quotient(st['num'], st['den'], st['wsum'], 0.1)[0])
    img = aps.image(dirs, coords=coords)
    assert NP.all(NP.abs(img[0] - S) > 0.01 * S)                      # the apparent flux: the beam is still in it
    assert NP.all(NP.abs(img[0] - S) > 1e6 * bound)
