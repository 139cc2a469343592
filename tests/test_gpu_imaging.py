"""GPU: dirty images and synthesized beams by the direct Fourier sum on the device (include/prisim_imaging.h) -- through the C-ABI
against the numpy checker (tests/imaging_checker.py), the NaN of a channel without weight, the bit equality between budgets, and
through prisim_amd.interferometry.ApertureSynthesis against the project's own sky-sum (the dot-product identity) and a point source.

Bounds.  The project's tolerance for the fp64 sky-sum, 1e-11 of the natural scale (README), here sum_{t,b} w|V| / sum w per channel
(per image with chan_avg; 1 for the synthesized beam): every element of every image is held to it against the checker.  That checker
agrees to 1e-14 of the scale with its own phase and sum arithmetic redone in longdouble (tests/test_imaging.py) -- from float64
directions in both arms, on these baselines of 300 m at most: no independent check of the directions, and none of long baselines.
Both are in tests/test_gpu_imaging_reference.py, against the 40-digit reference of tests/imaging_reference.py out to 2400 km, where
this checker itself is past 1e-11 from 300 km on.  The two routes are within twice the bound of each other.  The dot-product identity carries the bound once for the sky-sum and once for the image:
2e-11 sum|x| sum w|V|.  No element is left out of any comparison."""
import os
import sys
import warnings

import numpy as NP
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import imaging_cases as IC  # noqa: E402
import imaging_checker as IK  # noqa: E402

from prisim_amd import _abi, skymodel as SM  # noqa: E402
from prisim_amd import interferometry as RI  # noqa: E402

pytestmark = pytest.mark.gpu
BOUND = 1e-11
K = 32                                                               # the reseed interval of the stepped route (stats['reseed'])

# (nbl, nchan, npix, nt): every size of the issue's lists at least once -- one pixel, one baseline, one channel; 63 and 65 pixels
# about a wavefront; 1000 pixels in four blocks; 5, K + 1 (two tiles, the second of one channel) and 70 channels (three tiles)
SHAPES = [(1, 1, 1, 1), (37, 5, 63, 1), (300, 70, 65, 3), (37, K + 1, 1000, 3)]


def call(ctx, c, weights=None, **kw):
    return ctx.dirty_image(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], cube=kw.pop('cube', c['cube']), weights=weights,
                           aberr_beta=c['beta'], **kw)


def check(c, weights, kind, chan_avg, nonzero=None):
    return IK.dirty_image(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], cube=c['cube'], weights=weights, kind=kind,
                          chan_avg=chan_avg, aberr_beta=c['beta'], nonzero=nonzero)


def deviation(got, want):
    """the largest |got - want| in units of the scale, over every element"""
    return float(NP.max(NP.abs(got - want['image']) / want['scale']))


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(str(v) for v in s))
def test_g1_entry_against_the_checker(ctx, shape):
    nbl, nchan, npix, nt = shape
    c = IC.case(nbl, nchan, npix, nt)
    for form, weights in (('none', None), ('baseline', c['w_bl']), ('full', c['w_full'])):
        if nbl >= 7:
            assert NP.count_nonzero(NP.asarray(c['w_bl']) == 0.0) == nbl // 7
        for kind in ('dirty', 'psf'):
            both = check(c, weights, kind, False)                     # one evaluation serves the band's image too
            for chan_avg in (False, True):
                want = both['band'] if chan_avg else both
                got = {}
                for route in ('direct', 'stepped'):
                    img, wsum, st = call(ctx, c, weights=weights, kind=kind, chan_avg=chan_avg, route=route)
                    assert img.shape == want['image'].shape and img.dtype == NP.float64
                    assert st['route'] == route and st['terms'] == npix * nbl * nchan * nt and st['chan_tile'] == K
                    assert st['reseed'] == (K if route == 'stepped' else 1) and st['resident'] is False and st['block_pixels'] == 256
                    assert NP.allclose(wsum, want['wsum'], rtol=1e-13, atol=0)
                    dev = deviation(img, want)
                    print('%s %s weights=%s chan_avg=%d %s: %.3e of the scale (bound %.1e)' % (shape, kind, form, chan_avg, route, dev, BOUND))
                    assert dev <= BOUND, (shape, kind, form, chan_avg, route, dev)
                    got[route] = img
                between = float(NP.max(NP.abs(got['direct'] - got['stepped']) / want['scale']))
                assert between <= 2 * BOUND, (shape, kind, form, chan_avg, between)
    # AUTO on this uniform grid is the stepped route, bit for bit
    img, _, st = call(ctx, c, weights=c['w_full'])
    assert st['route'] == 'stepped' and NP.array_equal(img, call(ctx, c, weights=c['w_full'], route='stepped')[0])


def test_g1_non_uniform_grid_is_direct_and_refuses_the_stepped_route(ctx):
    c = IC.case(37, 70, 65, 3, uniform=False)
    want = check(c, c['w_full'], 'dirty', False)
    img, _, st = call(ctx, c, weights=c['w_full'])
    assert st['route'] == 'direct' and st['reseed'] == 1
    dev = deviation(img, want)
    print('non-uniform grid, auto: %.3e of the scale' % dev)
    assert dev <= BOUND
    with pytest.raises(ValueError, match='uniform'):
        call(ctx, c, weights=c['w_full'], route='stepped')
    assert NP.array_equal(call(ctx, c, weights=c['w_full'], route='direct')[0], img)      # and the context goes on as before


def test_g1_resident_cube_and_refusals(ctx):
    c = IC.case(37, K + 1, 65, 3)
    host, _, _ = call(ctx, c, weights=c['w_bl'])
    with _abi.Context(0) as fresh:
        with pytest.raises(RuntimeError, match='no resident'):
            call(fresh, c, cube=None)                                 # PRISIM_ESTATE: no array was ever set
        assert call(fresh, c, cube=None, kind='psf')[0].shape == (65, K + 1)      # the beam needs no cube of either kind
    ctx.set_array(c['baselines'], c['freqs'], nt_max=3)
    for t in range(3):
        ctx.set_vis(NP.ascontiguousarray(c['cube'][t]), slot=t)
    img, _, st = call(ctx, c, cube=None, weights=c['w_bl'])
    assert st['resident'] is True and NP.array_equal(img, host)
    ctx.set_array(c['baselines'], c['freqs'], nt_max=2)
    with pytest.raises(ValueError, match='resident cube has 2 slots'):
        call(ctx, c, cube=None)
    p, lib, h = _abi._ptr, ctx._lib, ctx._h
    rot = NP.ascontiguousarray(c['rot'].reshape(-1, 9))
    out = NP.full((65, K + 1), -7.0)

    def entry(**kw):
        a = ctx.PrisimImagingArgs()
        v = dict(npix=65, nbl=37, nchan=K + 1, nt=3, unitvec=c['unitvec'], rot=rot, aberr_beta=c['beta'], pc_dircos=c['pc'],
                 baselines=c['baselines'], freqs_hz=c['freqs'], cube=c['cube'], weights=c['w_full'], kind=0, weight_form=2, chan_avg=0,
                 route=-1, budget_bytes=0)
        v.update(kw)
        keep = []
        for name, val in v.items():
            if isinstance(val, NP.ndarray):
                val = NP.ascontiguousarray(val)
                keep.append(val)
                val = p(val)
            setattr(a, name, val)
        rc = lib.prisim_dirty_image(h, _abi.C.byref(a), p(out), None, None)
        return rc, lib.prisim_hip_last_error(h).decode()

    def changed(name, index, value):
        x = NP.array(rot if name == 'rot' else c[name], dtype=NP.float64)
        x[index] = value
        return x

    one_block = 256 * (32 * 3 + 8 * (K + 1))
    refusals = [({'unitvec': None}, 'unitvec is NULL'), ({'rot': None}, 'rot is NULL'), ({'pc_dircos': None}, 'pc_dircos is NULL'),
                ({'baselines': None}, 'baselines is NULL'), ({'freqs_hz': None}, 'freqs_hz is NULL'), ({'weights': None}, 'weights is NULL'),
                ({'npix': 0}, '>= 1'), ({'nbl': 0}, '>= 1'), ({'nchan': -1}, '>= 1'), ({'nt': 0}, '>= 1'), ({'nchan': (1 << 20) + 1}, '2^20'),
                ({'npix': 1 << 45}, '2^46'), ({'kind': 2}, 'unknown kind'), ({'route': 2}, 'unknown route'), ({'route': -2}, 'unknown route'),
                ({'weight_form': 3}, 'unknown weight form'), ({'chan_avg': 2}, 'chan_avg'),
                ({'unitvec': changed('unitvec', (3, 0), 1.5)}, 'unitvec[3]'), ({'rot': changed('rot', (1, 4), 0.5)}, 'rot of snapshot 1'),
                ({'aberr_beta': changed('beta', (2, 1), 0.02)}, 'aberr_beta of snapshot 2'),
                ({'pc_dircos': changed('pc', (0, 2), 1.1)}, 'pc_dircos of snapshot 0'),
                ({'freqs_hz': changed('freqs', 5, 0.0)}, 'freqs_hz[5]'), ({'freqs_hz': changed('freqs', 5, NP.inf)}, 'freqs_hz[5]'),
                ({'weights': changed('w_full', (1, 2, 3), -1.0)}, 'finite and non-negative'),
                ({'weights': changed('w_full', (1, 2, 3), NP.nan)}, 'finite and non-negative'),
                ({'baselines': changed('baselines', (4, 1), NP.nan)}, 'baseline 4'),
                ({'budget_bytes': one_block - 1}, 'cannot hold one block'), ({'cube': None, 'nbl': 36}, 'resident cube has 2 slots')]
    for kw, msg in refusals:
        rc, err = entry(**kw)
        assert rc == _abi.PRISIM_EINVAL and msg in err, (list(kw), rc, err)
        assert NP.all(out == -7.0)                                    # nothing is written unless the call succeeds
    rc, err = entry(budget_bytes=one_block)
    assert rc == _abi.PRISIM_OK, err
    assert NP.array_equal(out, call(ctx, c, weights=c['w_full'])[0])


def test_g1_the_three_entries_refuse_a_shared_argument_alike(ctx):
    """prisim_dirty_image, prisim_mosaic_image and prisim_clean_image check the arguments they have in common by one function: a faulty
    one gets the same code and the same sentence from each, on the host and before any launch, and no output is written."""
    c = IC.case(37, K + 1, 65, 3)
    p, lib, h, byref = _abi._ptr, ctx._lib, ctx._h, _abi.C.byref
    npix, nchan, maxiter = 65, K + 1, 5
    rot = NP.ascontiguousarray(c['rot'].reshape(-1, 9))
    image = [NP.full((npix, nchan), -7.0) for _ in range(6)] + [NP.full(nchan, -7.0) for _ in range(4)]
    lists = [NP.full((nchan, maxiter), -7, dtype=NP.int32), NP.full((nchan, maxiter), -7.0), NP.full(nchan, -7, dtype=NP.int32),
             NP.full(nchan, -7, dtype=NP.int32)]
    shared = dict(npix=npix, nbl=37, nchan=nchan, nt=3, unitvec=c['unitvec'], rot=rot, aberr_beta=c['beta'], pc_dircos=c['pc'],
                  baselines=c['baselines'], freqs_hz=c['freqs'], cube=c['cube'], weights=c['w_full'], weight_form=2, chan_avg=0, route=-1,
                  budget_bytes=0)
    own = {'prisim_dirty_image': (ctx.PrisimImagingArgs, dict(kind=0)),
           'prisim_mosaic_image': (ctx.PrisimMosaicArgs, dict(beam_kind=_abi.PRISIM_BEAM_AIRY, diameter_m=2.0, pbmin=0.1)),
           'prisim_clean_image': (ctx.PrisimImcleanArgs, dict(gain=0.3, threshold=0.1, maxiter=maxiter, threshold_relative=1, poll_every=0))}

    def entry(name, **kw):
        a, keep = own[name][0](), []
        for field, val in dict(shared, **own[name][1], **kw).items():
            if isinstance(val, NP.ndarray):
                val = NP.ascontiguousarray(val)
                keep.append(val)
                val = p(val)
            setattr(a, field, val)
        if name == 'prisim_dirty_image':
            rc = lib.prisim_dirty_image(h, byref(a), p(image[0]), p(image[6]), None)
        elif name == 'prisim_mosaic_image':
            a.beam_pc_dircos[:] = [0.0, 0.0, 1.0]
            rc = lib.prisim_mosaic_image(h, byref(a), p(image[1]), p(image[2]), p(image[3]), p(image[4]), p(image[7]), None)
        else:
            rc = lib.prisim_clean_image(h, byref(a), p(image[5]), None, p(lists[0]), p(lists[1]), p(lists[2]), p(lists[3]), p(image[8]),
                                        p(image[9]), None)
        return rc, lib.prisim_hip_last_error(h).decode()

    def changed(name, index, value):
        x = NP.array(rot if name == 'rot' else c[name], dtype=NP.float64)
        x[index] = value
        return x

    faults = [({'unitvec': changed('unitvec', (3, 0), 1.5)}, 'unitvec[3]'), ({'rot': changed('rot', (1, 4), 0.5)}, 'rot of snapshot 1'),
              ({'aberr_beta': changed('beta', (2, 1), 0.02)}, 'aberr_beta of snapshot 2'),
              ({'weights': changed('w_full', (1, 2, 3), -1.0)}, 'finite and non-negative'), ({'nchan': 0}, '>= 1'),
              ({'route': 2}, 'unknown route'),
              # the phase range, in the sentence of prisim_hip_set_array: 2^29 cycles of max|b| 2 max|f| / c and beyond
              ({'baselines': changed('baselines', (4, 1), 6e8)}, 'phase range: max|b| * 2 * max|f| / c = '),
              ({'baselines': changed('baselines', (4, 1), 1e200)}, 'the limit is below 2^29 = 536870912 cycles')]
    for kw, msg in faults:
        answers = {name: entry(name, **kw) for name in own}
        assert len(set(answers.values())) == 1, (list(kw), answers)
        rc, err = answers['prisim_dirty_image']
        assert rc == _abi.PRISIM_EINVAL and msg in err, (list(kw), rc, err)
        assert all(NP.all(o == -7) for o in image + lists), list(kw)  # nothing is written unless the call succeeds
    assert all(entry(name)[0] == _abi.PRISIM_OK for name in own)      # and the unchanged arguments are taken by all three


def test_g2_a_channel_without_weight_is_nan_and_nothing_else_is(ctx):
    c = IC.case(37, 70, 65, 3)
    w = c['w_full'].copy()
    w[:, :, 41] = 0.0
    meant = NP.ones(70, dtype=bool)
    meant[41] = False
    for route in ('direct', 'stepped'):
        for kind in ('dirty', 'psf'):
            want = check(c, w, kind, False, nonzero=meant)
            img, wsum, _ = call(ctx, c, weights=w, kind=kind, route=route)
            assert NP.array_equal(NP.isnan(img), NP.broadcast_to(~meant, img.shape)) and wsum[41] == 0.0 and NP.all(wsum[meant] >= 1.0)
            assert float(NP.max(NP.abs(img[:, meant] - want['image'][:, meant]) / want['scale'][meant])) <= BOUND
            want = check(c, w, kind, True, nonzero=meant)
            img, wsum, _ = call(ctx, c, weights=w, kind=kind, route=route, chan_avg=True)
            assert NP.all(NP.isfinite(img)) and wsum.shape == (1,) and deviation(img, want) <= BOUND
            for chan_avg in (False, True):
                img, wsum, _ = call(ctx, c, weights=NP.zeros_like(w), kind=kind, route=route, chan_avg=chan_avg)
                assert NP.all(NP.isnan(img)) and NP.all(wsum == 0.0)
    img, wsum, _ = call(ctx, c, weights=NP.zeros(37))
    assert NP.all(NP.isnan(img)) and NP.all(wsum == 0.0)


def test_g3_the_budget_leaves_the_bits_unchanged(ctx):
    c = IC.case(37, 70, 1000, 3)
    for chan_avg in (False, True):
        smallest = 256 * (32 * 3 + 8 * 70 + (8 if chan_avg else 0))      # one block of pixels on one stream
        for route in ('direct', 'stepped'):
            for kind in ('dirty', 'psf'):
                full, wf, st = call(ctx, c, weights=c['w_full'], kind=kind, route=route, chan_avg=chan_avg)
                assert st['chunks'] == 1 and st['streams'] == 1
                small, ws, st = call(ctx, c, weights=c['w_full'], kind=kind, route=route, chan_avg=chan_avg, budget_bytes=smallest)
                assert st['chunks'] == 4 and st['chunk_pixels'] == 256 and st['streams'] == 1
                assert NP.array_equal(full, small) and NP.array_equal(wf, ws), (route, kind, chan_avg)
                two, _, st = call(ctx, c, weights=c['w_full'], kind=kind, route=route, chan_avg=chan_avg, budget_bytes=2 * smallest)
                assert st['chunks'] == 4 and st['streams'] == 2 and NP.array_equal(full, two), (route, kind, chan_avg)
                with pytest.raises(ValueError, match='cannot hold one block'):
                    call(ctx, c, weights=c['w_full'], kind=kind, route=route, chan_avg=chan_avg, budget_bytes=smallest - 1)


# ---- through the classes ----------------------------------------------------------------------------------------------------------------

LAT = -30.7224
CH = 150e6 + 1e5 * NP.arange(K + 1)
TELESCOPE = {'id': 'custom', 'shape': 'delta', 'size': 14.0, 'ocoords': 'altaz', 'orientation': NP.array([[90.0, 270.0]]), 'groundplane': None}
LSTS = [30.0, 31.5, 34.0]


def _array(nbl, pointing_coords, skycoords, reserve=0):
    rng = NP.random.default_rng(77)
    bl = rng.uniform(-1.0, 1.0, (nbl, 3)) * NP.array([200.0, 200.0, 5.0])
    labels = [(str(i + 1), '0') for i in range(nbl)]
    ia = RI.InterferometerArray(labels, bl, CH, telescope=TELESCOPE, latitude=LAT, skycoords=skycoords, pointing_coords=pointing_coords)
    ia.frame_model = 'date'
    if reserve:
        ia.reserve(reserve)
    return ia


def _observe(ia, sky, pointing, nt):
    for j in range(nt):
        ia.observe((2457000.5 + j / 64.0, LSTS[j]), {'Tnet': 200.0}, NP.ones(CH.size), pointing, sky, 10.7)


@pytest.mark.parametrize('coords', ['altaz', 'radec'])
def test_g4_dot_product_identity_against_the_sky_sum(coords):
    """<x, image(V)> = <V_sim(x), V>: the image is the adjoint of the sky-sum observe() ran, with its sign, its phase centres and, for a
    'radec' sky, its frame per snapshot."""
    rng = NP.random.default_rng(4)
    nsrc, nbl, nt = 40, 37, 3
    if coords == 'altaz':
        loc = NP.stack((rng.uniform(25.0, 88.0, nsrc), rng.uniform(0.0, 360.0, nsrc)), axis=1)
        pointing, pcoords = [90.0, 270.0], 'altaz'
    else:
        loc = NP.stack((rng.uniform(5.0, 60.0, nsrc), rng.uniform(-60.0, 0.0, nsrc)), axis=1)      # up at every one of the three LSTs
        pointing, pcoords = [31.0, -25.0], 'radec'                    # a phase centre that moves across the local sky
    x = rng.uniform(0.5, 2.0, nsrc)
    sky = SM.SkyModel(location=loc, flux_ref=x, spindex=NP.zeros(nsrc), ref_freq=150e6)
    ia = _array(nbl, pcoords, coords)
    _observe(ia, sky, pointing, nt)
    vsim = NP.array(ia.skyvis_freq, dtype=NP.complex128)              # (nbl, nchan, nt)
    assert vsim.shape == (nbl, CH.size, nt) and NP.abs(vsim).max() > 1.0
    if coords == 'radec':
        pc = ia._pc_dircos(ia.phase_center, 'radec')
        assert NP.abs(pc[0] - pc[2]).max() > 1e-2
    v = rng.standard_normal(vsim.shape) + 1j * rng.standard_normal(vsim.shape)
    w = rng.uniform(0.0, 1.0, vsim.shape)
    ia.skyvis_freq = v
    aps = RI.ApertureSynthesis(ia)
    for route in ('stepped', 'direct'):
        img = aps.image(loc, coords=coords, weights=w, route=route)
        assert img.shape == (nsrc, CH.size) and aps.image_stats['route'] == route and aps.image_stats['resident'] is False
        D = img * aps.image_stats['wsum'][NP.newaxis, :]
        lhs = NP.einsum('p,pk->k', x, D)
        rhs = NP.einsum('bkt,bkt->k', w * v, vsim.conj()).real
        bound = 2 * BOUND * NP.abs(x).sum() * NP.einsum('bkt->k', w * NP.abs(v))
        dev = float(NP.max(NP.abs(lhs - rhs) / bound))
        print('%s %s: |<x, D> - Re<wV, V_sim>| is %.3e of its bound' % (coords, route, dev))
        assert NP.all(NP.abs(lhs - rhs) <= bound), (coords, route, dev)
        # a wrong sign or phase centre would leave the two sides unrelated: they are of the size of the bound's factors, not of the bound
        assert NP.abs(rhs).max() > 1e6 * bound.max()


def test_g5_a_point_source_images_to_its_flux():
    S, nbl, nt = 2.75, 37, 2
    src = NP.array([[62.0, 140.0]])
    sky = SM.SkyModel(location=src, flux_ref=[S], spindex=[0.0], ref_freq=150e6)
    others = NP.stack((NP.linspace(20.0, 89.0, 64), NP.linspace(0.0, 350.0, 64)), axis=1)
    dirs = NP.vstack((src, others))
    res = _array(nbl, 'altaz', 'altaz', reserve=nt)
    _observe(res, sky, [90.0, 270.0], nt)
    aps = RI.ApertureSynthesis(res)
    img = aps.image(dirs, coords='altaz', datakey='noiseless')
    st = aps.image_stats
    assert img.shape == (65, CH.size) and st['resident'] is True and st['route'] == 'stepped' and st['terms'] == 65 * nbl * CH.size * nt
    dev = float(NP.max(NP.abs(img[0] - S)) / S)
    print('point source at its own direction: %.3e of S (bound %.1e)' % (dev, 2 * BOUND))
    assert dev <= 2 * BOUND
    assert NP.all(NP.abs(img[1:]) <= S * (1.0 + 2 * BOUND))           # nowhere brighter than at the source
    beam = aps.psf(NP.array([[0.0, 0.0, 1.0]]), coords='dircos')
    assert beam.shape == (1, CH.size) and float(NP.max(NP.abs(beam - 1.0))) <= BOUND
    assert aps.image_stats['resident'] is False and aps.image_stats['route'] == 'stepped'
    # the same run without reserve(): the cube is handed over, and the image has the same bits
    host = _array(nbl, 'altaz', 'altaz')
    _observe(host, sky, [90.0, 270.0], nt)
    aph = RI.ApertureSynthesis(host)
    img_h = aph.image(dirs, coords='altaz', datakey='noiseless')
    assert aph.image_stats['resident'] is False and NP.array_equal(img_h, img)
    # the band's image and the other cubes
    assert float(abs(aps.image(dirs, coords='altaz', chan_avg=True)[0] - S)) <= 2 * BOUND * S
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        host.generate_noise(seed=11)
        host.add_noise()
    noisy, noise = aph.image(dirs, coords='altaz', datakey='noisy'), aph.image(dirs, coords='altaz', datakey='noise')
    assert NP.max(NP.abs(noisy - (img_h + noise))) <= 1e-11 * (S + NP.abs(noise).max())
