"""GPU: the fp32 route of the beam-weighted mosaic on the device (include/prisim_mosaic32.h, prisim_mosaic_image_f32) -- through the
C-ABI against the numpy checker (tests/mosaic_checker.py), beside the fp64 entry whose Q, wsum, pb_eff and NaN positions it must give
bit for bit, against prisim_dirty_image_f32 for a delta beam, the horizon and the pbmin mask, the bit equality between budgets,
streams and the resident cube, the refusals, and through prisim_amd.interferometry.ApertureSynthesis on a drift scan.

Bound.  Per element |N - N_ref| <= 5e-6 sum_t A_ref sum_b w|V| plus the fp64 terms tests/test_gpu_mosaic.py allows for the beam and the
checker (1e-11 of the same sum and 1e-12 sum_{t,b} w|V|): 5e-6 of the natural scale is the project's bar for its float32 mode
(DESIGN 2), tests/test_gpu_imaging32.py holds every D_t to it, and A_t <= 1 with the triangle inequality carries it through the sum
over t.  Q is not held to a bound: it is array_equal to the fp64 entry's.  The quotient is recomputed in numpy from the returned num,
den and wsum and compared with array_equal.  No element is left out of any comparison.  tests/test_mosaic32.py holds a numpy model
of the same chain to half the bound beforehand."""
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
BOUND = 5e-6
K = 32                                                               # the channel tile; one seed per tile (stats['reseed'])
LDS = 17920                                                          # kImaging32Lds of prisim_amd/csrc_addon/imaging32_plan.h
# (nbl, nchan, npix, nt): one of everything; one baseline over a full tile plus one channel, where nothing averages the chain's error,
# with a short last tile whose centre lies past the band; 37 baselines, an odd row count: a zero odd row in the last pair; 65: one full
# pass of 64 rows and a pass of one, with 257 pixels that cross a block; 300 baselines, 70 channels, three snapshots; 1000 pixels in
# four blocks
SHAPES = [(1, 1, 1, 1), (1, K + 1, 1000, 1), (37, 5, 63, 1), (65, K + 1, 257, 2), (300, 70, 65, 3), (37, K + 1, 1000, 3)]
BEAMS = ['gaussian', 'airy', 'dipole_ground', 'beamformer']


def call(ctx, c, beam, weights=None, precision='single', **kw):
    kind, dia, ext, _ = beam
    return ctx.mosaic_image(c['unitvec'], c['rot'], c['pc'], kw.pop('baselines', c['baselines']), c['freqs'], kind, dia, ext=ext,
                            cube=kw.pop('cube', c['cube']), weights=weights, aberr_beta=c['beta'], precision=precision, **kw)


def same(a, b):
    return NP.array_equal(a, b, equal_nan=True)


def share_of_the_bound(num, ref):
    """(the largest |num - num_ref| over 5e-6 sum_t A_ref sum_b w|V|, whether every element is within that plus the fp64 terms of
    tests/test_gpu_mosaic.py); an element whose bound is 0 must be exact"""
    scale = NP.einsum('tpk,tk->pk', ref['A'], ref['absV'])
    err = NP.abs(num - ref['num'])
    with NP.errstate(invalid='ignore', divide='ignore'):
        share = float(NP.max(NP.where(scale > 0.0, err / (BOUND * scale), NP.where(err > ref['bound_num'], NP.inf, 0.0))))
    return share, bool(NP.all(err <= BOUND * scale + ref['bound_num']))


def beside_the_fp64_entry(got, got64, pbmin, chan_avg, label):
    """den, wsum, pb_eff and every NaN of the mosaic have the bits of the fp64 entry; the mosaic is the header's quotient of num, den, wsum"""
    mosaic, num, den, wsum, st = got
    mosaic64, num64, den64, wsum64, st64 = got64
    assert st['precision'] == 'single' and st64['precision'] == 'double', label
    assert NP.array_equal(den, den64) and NP.array_equal(wsum, wsum64) and same(st['pb_eff'], st64['pb_eff']), label
    assert mosaic.shape == mosaic64.shape and NP.array_equal(NP.isnan(mosaic), NP.isnan(mosaic64)), label
    want_mosaic, want_eff = MK.quotient(num, den, wsum, pbmin, chan_avg)
    assert same(mosaic, want_mosaic) and same(st['pb_eff'], want_eff), label


# ---- G1: parity -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(str(v) for v in s))
def test_g1_entry_against_the_checker_and_beside_the_fp64_entry(ctx, shape):
    nbl, nchan, npix, nt = shape
    c = IC.case(nbl, nchan, npix, nt)
    beams = MC.beam_setups(nt)
    assert len(beams['beamformer'][2]) == nt                          # n_ext == nt
    if nbl >= 7:
        assert NP.count_nonzero(c['w_bl'] == 0.0) == nbl // 7
    A, worst = None, 0.0
    for form, weights in (('none', None), ('baseline', c['w_bl']), ('full', c['w_full'])):
        sums = MK.snapshot_sums(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], c['cube'], weights=weights, aberr_beta=c['beta'])
        if A is None:
            A = {name: MK.beams(sums['s'], c['freqs'], beams[name][3]) for name in BEAMS}       # once per shape
        for name in BEAMS:
            ref = dict(MK.combine(sums, A[name]), absV=sums['absV'])
            for chan_avg in (False, True):
                label = '%s %s weights=%s chan_avg=%d' % (shape, name, form, chan_avg)
                got = call(ctx, c, beams[name], weights=weights, chan_avg=chan_avg)
                got64 = call(ctx, c, beams[name], weights=weights, chan_avg=chan_avg, precision='double', route='stepped')
                st = got[4]
                assert st['route'] == 'stepped' and st['terms'] == npix * nbl * nchan * nt and st['chan_tile'] == K and st['reseed'] == K
                assert st['block_pixels'] == 256 and st['lds_bytes'] == LDS and st['resident'] is False and st['beam_values'] == npix * nchan * nt
                assert st['pixel_bytes'] == 64 * nt + 24 * nchan + (16 if chan_avg else 16 * nchan) == got64[4]['pixel_bytes']
                share, held = share_of_the_bound(got[1], ref)
                worst = max(worst, share)
                print('%s: |num - num_ref| at most %.3f of the bound %.1e sum_t A sum_b w|V|' % (label, share, BOUND))
                assert held, (label, share)
                beside_the_fp64_entry(got, got64, 0.1, chan_avg, label)
                if nbl * nchan * npix * nt > 1:
                    assert not NP.array_equal(got[1], got64[1]), label              # the fp32 kernel ran, not the fp64 one
    print('%s: worst %.3f of the bound' % (shape, worst))
    # an explicit STEPPED is the same call
    assert all(same(x, y) for x, y in zip(call(ctx, c, beams['airy'], weights=c['w_full'], route='stepped')[:4],
                                          call(ctx, c, beams['airy'], weights=c['w_full'])[:4]))


# ---- G2: a delta beam on one snapshot is the fp32 dirty image -----------------------------------------------------------------------------

def test_g2_delta_beam_on_one_snapshot_has_the_bits_of_the_fp32_dirty_image(ctx):
    c = MC.up_case(37, K + 1, 300, 1)
    assert NP.min(IK.directions(c['unitvec'], c['rot'], c['beta'])[..., 2]) > 0.04
    delta = MC.beam_setups(1)['delta']
    for weights in (None, c['w_bl'], c['w_full']):
        for route in ('auto', 'stepped'):
            for chan_avg in (False, True):
                mosaic, num, den, wsum, st = call(ctx, c, delta, weights=weights, route=route, chan_avg=chan_avg)
                img, wimg, sti = ctx.dirty_image(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], cube=c['cube'], weights=weights,
                                                 aberr_beta=c['beta'], route=route, chan_avg=chan_avg, precision='single')
                assert st['precision'] == 'single' == sti['precision']
                assert NP.all(NP.isfinite(img)) and NP.array_equal(mosaic, img), (route, chan_avg)
                assert NP.array_equal(den, NP.broadcast_to(wsum, den.shape))
                assert chan_avg or NP.array_equal(wsum, wimg)
                assert NP.array_equal(st['pb_eff'], NP.ones_like(mosaic))


# ---- G3: the horizon and the mask -----------------------------------------------------------------------------------------------------------

def test_g3_a_snapshot_below_the_horizon_contributes_exactly_nothing(ctx):
    c = MC.up_case(37, K + 1, 65, 3, flip=(1,))
    s = IK.directions(c['unitvec'], c['rot'], c['beta'])
    assert NP.min(s[0, :, 2]) > 0.04 and NP.max(s[1, :, 2]) < -0.04 and NP.min(s[2, :, 2]) > 0.04
    less = c['w_full'].copy()
    less[1] = 0.0
    for name in ('delta', 'airy'):
        beam = MC.beam_setups(3)[name]
        full = call(ctx, c, beam, weights=c['w_full'], pbmin=0.0)
        cut = call(ctx, c, beam, weights=less, pbmin=0.0)
        assert NP.all(NP.isfinite(full[0])) and NP.array_equal(full[1], cut[1]) and NP.array_equal(full[2], cut[2])
        assert NP.array_equal(full[0], cut[0]) and not NP.array_equal(full[3], cut[3])          # the same mosaic under another weight sum


def test_g3_below_the_horizon_in_every_snapshot_is_nan(ctx):
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


def test_g3_a_channel_without_weight_is_nan_and_nothing_else_is(ctx):
    c = MC.up_case(37, 70, 65, 3)
    w = c['w_full'].copy()
    w[:, :, 41] = 0.0
    live = NP.arange(70) != 41
    beam = MC.beam_setups(3)['gaussian']
    mosaic, num, den, wsum, st = call(ctx, c, beam, weights=w, pbmin=0.0)
    assert NP.array_equal(NP.isnan(mosaic), NP.broadcast_to(~live, mosaic.shape)) and wsum[41] == 0.0 and NP.all(wsum[live] >= 1.0)
    assert NP.all(num[:, 41] == 0.0) and NP.all(NP.isnan(st['pb_eff'][:, 41])) and NP.all(NP.isfinite(st['pb_eff'][:, live]))
    band = call(ctx, c, beam, weights=w, pbmin=0.0, chan_avg=True)
    assert NP.all(NP.isfinite(band[0])) and same(band[0], MK.quotient(num, den, wsum, 0.0, True)[0])


def test_g3_the_pbmin_mask_is_the_fp64_entrys(ctx):
    c = MC.mask_case()
    beam = MC.beam_setups(3)['gaussian']
    got = call(ctx, c, beam, weights=c['w_full'], pbmin=MC.MASK_PBMIN)
    got64 = call(ctx, c, beam, weights=c['w_full'], pbmin=MC.MASK_PBMIN, precision='double')
    masked = NP.isnan(got[0])
    assert NP.array_equal(masked, NP.isnan(got64[0])) and 0.1 <= float(NP.mean(masked)) <= 0.9
    assert NP.array_equal(masked, got[4]['pb_eff'] < MC.MASK_PBMIN)
    beside_the_fp64_entry(got, got64, MC.MASK_PBMIN, False, 'mask')


# ---- G4: the same bits however it is streamed -------------------------------------------------------------------------------------------------

def test_g4_budget_streams_and_the_resident_cube_leave_the_bits_unchanged(ctx):
    c = IC.case(37, K + 1, 1000, 3)
    beam = MC.beam_setups(3)['airy']
    for chan_avg in (False, True):
        one_block = 256 * (64 * 3 + 24 * (K + 1) + (16 if chan_avg else 16 * (K + 1)))
        full = call(ctx, c, beam, weights=c['w_full'], chan_avg=chan_avg)
        assert full[4]['chunks'] == 1 and full[4]['streams'] == 1 and full[4]['precision'] == 'single'
        for budget, streams in ((one_block, 1), (2 * one_block, 2)):
            got = call(ctx, c, beam, weights=c['w_full'], chan_avg=chan_avg, budget_bytes=budget)
            assert got[4]['chunks'] == 4 and got[4]['chunk_pixels'] == 256 and got[4]['streams'] == streams
            assert all(same(x, y) for x, y in zip(full[:4], got[:4])) and same(full[4]['pb_eff'], got[4]['pb_eff']), (chan_avg, streams)
        with pytest.raises(ValueError, match='cannot hold one block'):
            call(ctx, c, beam, weights=c['w_full'], chan_avg=chan_avg, budget_bytes=one_block - 1)
    host = call(ctx, c, beam, weights=c['w_bl'])
    ctx.set_array(c['baselines'], c['freqs'], nt_max=3)
    for t in range(3):
        ctx.set_vis(NP.ascontiguousarray(c['cube'][t]), slot=t)
    res = call(ctx, c, beam, weights=c['w_bl'], cube=None)
    assert res[4]['resident'] is True and res[4]['precision'] == 'single' and all(same(x, y) for x, y in zip(host[:4], res[:4]))


# ---- G5: refusals ---------------------------------------------------------------------------------------------------------------------------

def test_g5_refusals_write_nothing_and_shared_faults_are_answered_alike(ctx):
    c = IC.case(37, K + 1, 65, 3)
    odd = IC.case(37, K + 1, 65, 3, uniform=False)
    p, lib, h = _abi._ptr, ctx._lib, ctx._h
    rot = NP.ascontiguousarray(c['rot'].reshape(-1, 9))
    names = ('prisim_mosaic_image', 'prisim_mosaic_image_f32')
    outs = {name: [NP.full((65, K + 1), -7.0) for _ in range(4)] + [NP.full(K + 1, -7.0)] for name in names}
    airy = MC.beam_setups(3)['airy']

    def entry(name, **kw):
        a = ctx.PrisimMosaicArgs()
        v = dict(npix=65, nbl=37, nchan=K + 1, nt=3, unitvec=c['unitvec'], rot=rot, aberr_beta=c['beta'], pc_dircos=c['pc'],
                 baselines=c['baselines'], freqs_hz=c['freqs'], cube=c['cube'], weights=c['w_full'], weight_form=2, chan_avg=0, route=-1,
                 beam_kind=_abi.PRISIM_BEAM_AIRY, diameter_m=airy[1], pbmin=0.1, budget_bytes=0)
        v.update(kw)
        keep = []
        for field, val in v.items():
            if isinstance(val, NP.ndarray):
                val = NP.ascontiguousarray(val)
                keep.append(val)
                val = p(val)
            setattr(a, field, val)
        a.beam_pc_dircos[:] = [0.0, 0.0, 1.0]
        o = outs[name]
        rc = getattr(lib, name)(h, C.byref(a), p(o[0]), p(o[1]), p(o[2]), p(o[3]), p(o[4]), None)
        return rc, lib.prisim_hip_last_error(h).decode()

    def untouched():
        return all(NP.all(o == -7.0) for group in outs.values() for o in group)

    def changed(name, index, value):
        x = NP.array(rot if name == 'rot' else c[name], dtype=NP.float64)
        x[index] = value
        return x

    # this route's own: DIRECT, and a grid that is not uniform under AUTO and under STEPPED; each names the fp64 entry
    for kw, msg in (({'route': _abi.PRISIM_IMAGE_DIRECT}, 'DIRECT'), ({'freqs_hz': odd['freqs'], 'route': _abi.PRISIM_IMAGE_AUTO}, 'uniform'),
                    ({'freqs_hz': odd['freqs'], 'route': _abi.PRISIM_IMAGE_STEPPED}, 'uniform')):
        rc, err = entry('prisim_mosaic_image_f32', **kw)
        assert rc == _abi.PRISIM_EINVAL and msg in err and err.split(' (one block')[0].endswith('call prisim_mosaic_image'), (kw.get('route'), rc, err)
        assert untouched()
    with pytest.raises(ValueError, match='call prisim_mosaic_image'):
        call(ctx, c, airy, route='direct')
    with pytest.raises(ValueError, match='call prisim_mosaic_image'):
        call(ctx, odd, airy)
    with pytest.raises(ValueError, match='precision'):
        call(ctx, c, airy, precision='half')
    # the shared faults: one code and one sentence from both entries
    snap = NP.array([[0.0, 0.0, 1.0], [0.0, NP.nan, 1.0], [0.0, 0.0, 1.0]])
    faults = [({'pbmin': -0.1}, 'pbmin must lie in [0, 1)'), ({'pbmin': 1.0}, 'pbmin must lie in [0, 1)'), ({'pbmin': NP.nan}, 'pbmin'),
              ({'pbmin': NP.inf}, 'pbmin'), ({'beam_pc_snap': snap}, 'beam_pc_snap of snapshot 1 is not finite'),
              ({'unitvec': changed('unitvec', (3, 0), 1.5)}, 'unitvec[3]'), ({'rot': changed('rot', (1, 4), 0.5)}, 'rot of snapshot 1'),
              ({'weights': changed('w_full', (1, 2, 3), -1.0)}, 'finite and non-negative'), ({'nchan': 0}, '>= 1'), ({'route': 2}, 'unknown route'),
              ({'n_ext': 1}, 'ext is NULL'), ({'beam_kind': 9}, 'unknown beam_kind'), ({'diameter_m': 0.0}, 'diameter_m must be positive'),
              ({'budget_bytes': 256 * (64 * 3 + 40 * (K + 1)) - 1}, 'cannot hold one block'),
              ({'baselines': changed('baselines', (4, 1), 6e8)}, 'phase range: max|b| * 2 * max|f| / c = ')]
    for kw, msg in faults:
        answers = {name: entry(name, **kw) for name in names}
        rc, err = answers['prisim_mosaic_image_f32']
        assert rc == _abi.PRISIM_EINVAL and msg in err, (list(kw), rc, err)
        if 'budget_bytes' in kw:                                      # the plan's refusal names the LDS of the entry's own kernel behind the sentence
            assert answers['prisim_mosaic_image'][0] == rc and answers['prisim_mosaic_image'][1].split(' (one block')[0] == err.split(' (one block')[0]
        else:
            assert len(set(answers.values())) == 1, (list(kw), answers)
        assert untouched(), list(kw)
    # a null struct and a null output
    o = outs['prisim_mosaic_image_f32']
    assert lib.prisim_mosaic_image_f32(h, None, p(o[0]), None, None, None, None, None) == _abi.PRISIM_EINVAL and untouched()
    # and the unchanged arguments are taken by both, into the arrays that were left alone so far
    assert all(entry(name)[0] == _abi.PRISIM_OK for name in names)
    want = call(ctx, c, airy, weights=c['w_full'])
    assert same(o[0], want[0]) and same(o[1], want[4]['pb_eff']) and same(o[2], want[1]) and same(o[3], want[2]) and same(o[4], want[3])
    o64 = outs['prisim_mosaic_image']
    assert same(o64[1], o[1]) and same(o64[3], o[3]) and same(o64[4], o[4]) and not same(o64[2], o[2])


# ---- G6: long baselines ---------------------------------------------------------------------------------------------------------------------

def test_g6_long_baselines_and_the_phase_range(ctx):
    c = IC.case(33, K + 1, 65, 2)
    far = c['baselines'] * 300.0                                      # 90 km: 4.5e4 wavelengths
    beams = MC.beam_setups(2)
    sums = MK.snapshot_sums(c['unitvec'], c['rot'], c['pc'], far, c['freqs'], c['cube'], weights=c['w_full'], aberr_beta=c['beta'])
    for name in ('gaussian', 'airy'):
        ref = dict(MK.combine(sums, MK.beams(sums['s'], c['freqs'], beams[name][3])), absV=sums['absV'])
        got = call(ctx, c, beams[name], weights=c['w_full'], baselines=far)
        got64 = call(ctx, c, beams[name], weights=c['w_full'], baselines=far, precision='double')
        share, held = share_of_the_bound(got[1], ref)
        print('90 km %s: |num - num_ref| at most %.3f of the bound %.1e sum_t A sum_b w|V|' % (name, share, BOUND))
        assert held, (name, share)
        beside_the_fp64_entry(got, got64, 0.1, False, '90 km ' + name)
    # the 2^29-cycle refusal, in the fp64 entry's sentence
    out = c['baselines'].copy()
    out[4, 1] = 6e8
    said = {}
    for precision in ('double', 'single'):
        with pytest.raises(ValueError, match='phase range') as e:
            call(ctx, c, beams['airy'], weights=c['w_full'], baselines=out, precision=precision)
        said[precision] = str(e.value).split(' failed: ', 1)[1]      # the library's sentence, behind the name of the entry
    assert said['single'] == said['double'] and 'the limit is below 2^29 = 536870912 cycles' in said['single']


# ---- G7: end to end -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('coords', ['radec', 'altaz'])
def test_g7_a_drift_scan_returns_the_flux_of_the_catalogue(coords):
    """The drift scan of tests/test_gpu_mosaic.py's M6 with precision = 'single': for one source sum_t A_t sum_b w|V| / Q = S, so the
    bound on num is 5e-6 S on the mosaic at the source's position."""
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
    plain = aps.mosaic(dirs, coords=coords)                           # an object that was never told otherwise: the fp64 route
    st64 = aps.image_stats
    assert st64['precision'] == 'double'
    aps.precision = 'single'
    mosaic = aps.mosaic(dirs, coords=coords)
    st = aps.image_stats
    assert mosaic.shape == (9, MC.CH.size) and st['precision'] == 'single' and st['route'] == 'stepped' and st['lds_bytes'] == LDS
    assert st['terms'] == 9 * nbl * MC.CH.size * nt and st['num'].shape == st['den'].shape == (9, MC.CH.size)
    dev = float(NP.max(NP.abs(mosaic[0] - S)) / S)
    print('%s: |mosaic - S| at the source is at most %.3e of S (%.3f of the bound %.1e)' % (coords, dev, dev / BOUND, BOUND))
    assert dev <= BOUND
    assert same(mosaic, MK.quotient(st['num'], st['den'], st['wsum'], 0.1)[0])
    assert NP.array_equal(st['den'], st64['den']) and NP.array_equal(st['wsum'], st64['wsum']) and same(st['pb_eff'], st64['pb_eff'])
    assert not NP.array_equal(st['num'], st64['num']) and NP.array_equal(NP.isnan(mosaic), NP.isnan(plain))
    with pytest.raises(ValueError, match='direct'):
        aps.mosaic(dirs, coords=coords, route='direct')
    aps.precision = 'double'
    assert same(plain, aps.mosaic(dirs, coords=coords)) and aps.image_stats['precision'] == 'double'
    assert same(plain, RI.ApertureSynthesis(ia).mosaic(dirs, coords=coords))
