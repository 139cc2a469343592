"""GPU: the fp32 route of dirty images and synthesized beams on the device (include/prisim_imaging32.h, prisim_dirty_image_f32) --
through the C-ABI against the numpy checker (tests/imaging_checker.py), beside the fp64 entry whose weight sums it must give bit for
bit, and through prisim_amd.interferometry.ApertureSynthesis.

Bound.  BOUND = 5e-6 of the natural scale, sum_{t,b} w|V| / sum w per channel (per image with chan_avg; 1 for the synthesized beam):
the project's bar for its float32 mode.  Every element of every image is held to it against the checker, whose own error
on these baselines is 1e-14 of the scale (tests/test_imaging.py) and out to 90 km below 1e-11 (tests/imaging_reference.py).  No
element is left out of any comparison.  tests/test_imaging32.py holds a numpy model of the same chain to half the bound beforehand."""
import os
import sys

import numpy as NP
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import imaging32_model as M  # noqa: E402
import imaging_cases as IC  # noqa: E402
import imaging_checker as IK  # noqa: E402
import test_gpu_imaging as TG  # noqa: E402  (the arrays and the observing run of the fp64 tests)

from prisim_amd import _abi, skymodel as SM  # noqa: E402
from prisim_amd import interferometry as RI  # noqa: E402

pytestmark = pytest.mark.gpu
BOUND = 5e-6
K = 32                                                               # the channel tile; one seed per tile (stats['reseed'])
LDS = 17920                                                          # kImaging32Lds of prisim_amd/csrc_addon/imaging32_plan.h

# (nbl, nchan, npix, nt): one of everything; one baseline over a full tile plus one channel, where nothing averages the chain's error;
# 63 and 65 pixels about a wavefront; 300 baselines (four full passes of 64 and one of 44) and 37 (one odd pass); 1000 pixels in four
# blocks; 5, K + 1 and 70 channels
SHAPES = [(1, 1, 1, 1), (1, K + 1, 1000, 1), (37, 5, 63, 1), (300, 70, 65, 3), (37, K + 1, 1000, 3)]


def call(ctx, c, weights=None, precision='single', **kw):
    return ctx.dirty_image(c['unitvec'], c['rot'], c['pc'], kw.pop('baselines', c['baselines']), c['freqs'], cube=kw.pop('cube', c['cube']),
                           weights=weights, aberr_beta=c['beta'], precision=precision, **kw)


def check(c, weights, kind, chan_avg, nonzero=None, baselines=None):
    return IK.dirty_image(c['unitvec'], c['rot'], c['pc'], c['baselines'] if baselines is None else baselines, c['freqs'], cube=c['cube'],
                          weights=weights, kind=kind, chan_avg=chan_avg, aberr_beta=c['beta'], nonzero=nonzero)


def deviation(got, want):
    """the largest |got - want| in units of the scale, over every element"""
    return float(NP.max(NP.abs(got - want['image']) / want['scale']))


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(str(v) for v in s))
def test_f1_entry_against_the_checker_and_beside_the_fp64_entry(ctx, shape):
    nbl, nchan, npix, nt = shape
    c = IC.case(nbl, nchan, npix, nt)
    worst = 0.0
    for form, weights in (('none', None), ('baseline', c['w_bl']), ('full', c['w_full'])):
        if nbl >= 7:
            assert NP.count_nonzero(NP.asarray(c['w_bl']) == 0.0) == nbl // 7
        for kind in ('dirty', 'psf'):
            both = check(c, weights, kind, False)                     # one evaluation serves the band's image too
            for chan_avg in (False, True):
                want = both['band'] if chan_avg else both
                img, wsum, st = call(ctx, c, weights=weights, kind=kind, chan_avg=chan_avg)
                img64, wsum64, st64 = call(ctx, c, weights=weights, kind=kind, chan_avg=chan_avg, precision='double', route='stepped')
                assert img.shape == want['image'].shape and img.dtype == NP.float64 and wsum.dtype == NP.float64
                assert st['precision'] == 'single' and st64['precision'] == 'double' and st['route'] == 'stepped'
                assert st['terms'] == npix * nbl * nchan * nt and st['chan_tile'] == K and st['reseed'] == K and st['block_pixels'] == 256
                assert st['lds_bytes'] == LDS and st['resident'] is False
                assert NP.array_equal(wsum, wsum64)                   # W[k] comes from the fp64 entry's kernels
                dev = deviation(img, want)
                worst = max(worst, dev)
                print('%s %s weights=%s chan_avg=%d: %.3e of the scale (%.3f of the bound %.1e)' % (shape, kind, form, chan_avg, dev, dev / BOUND, BOUND))
                assert dev <= BOUND, (shape, kind, form, chan_avg, dev)
                assert not NP.array_equal(img, img64), (shape, kind, form, chan_avg)      # the fp32 kernel ran, not the fp64 one
    print('%s: worst %.3e of the scale, %.3f of the bound' % (shape, worst, worst / BOUND))
    # an explicit STEPPED is the same call
    assert NP.array_equal(call(ctx, c, weights=c['w_full'], route='stepped')[0], call(ctx, c, weights=c['w_full'])[0])


@pytest.mark.parametrize('weight', [0.7, 0.1])
def test_f2_coherent_accumulation(ctx, weight):
    """The beam of 20000 equally weighted baselines: at the phase centre every term is +fl32(weight), so a float32 sum that is never
    flushed drifts by 1e-4 (tests/test_imaging32.py shows it on the model)."""
    c = M.coherent_case()
    assert c['nbl'] == 20000 and c['nchan'] == 2 and c['npix'] == 65 and c['nt'] == 1
    w = NP.full(c['nbl'], weight)
    want = check(c, w, 'psf', False)
    img, wsum, st = call(ctx, c, weights=w, kind='psf')
    centre, dev = float(NP.max(NP.abs(img[0] - 1.0))), deviation(img, want)
    print('coherent beam, w = %.1f: %.3e at the phase centre, %.3e over all 65 (%.3f of the bound)' % (weight, centre, dev, dev / BOUND))
    assert st['precision'] == 'single' and centre <= BOUND and dev <= BOUND


def test_f3_long_baselines_and_the_phase_range(ctx):
    c = IC.case(33, 33, 65, 2)
    far = c['baselines'] * 300.0                                      # 90 km: 4.5e4 wavelengths
    for kind in ('dirty', 'psf'):
        want = check(c, c['w_full'], kind, False, baselines=far)
        img, _, st = call(ctx, c, weights=c['w_full'], kind=kind, baselines=far)
        dev = deviation(img, want)
        print('90 km %s: %.3e of the scale (%.3f of the bound)' % (kind, dev, dev / BOUND))
        assert st['precision'] == 'single' and dev <= BOUND, (kind, dev)
    # the 2^29-cycle refusal, in the fp64 entry's sentence
    out = c['baselines'].copy()
    out[4, 1] = 6e8
    said = {}
    for precision in ('double', 'single'):
        with pytest.raises(ValueError, match='phase range') as e:
            call(ctx, c, weights=c['w_full'], baselines=out, precision=precision)
        said[precision] = str(e.value).split(' failed: ', 1)[1]      # the library's sentence, behind the name of the entry
    assert said['single'] == said['double'] and 'the limit is below 2^29 = 536870912 cycles' in said['single']


def test_f4_a_channel_without_weight_is_nan_and_nothing_else_is(ctx):
    c = IC.case(37, 70, 65, 3)
    w = c['w_full'].copy()
    w[:, :, 41] = 0.0
    meant = NP.ones(70, dtype=bool)
    meant[41] = False
    for kind in ('dirty', 'psf'):
        want = check(c, w, kind, False, nonzero=meant)
        img, wsum, _ = call(ctx, c, weights=w, kind=kind)
        assert NP.array_equal(NP.isnan(img), NP.broadcast_to(~meant, img.shape)) and wsum[41] == 0.0 and NP.all(wsum[meant] >= 1.0)
        assert float(NP.max(NP.abs(img[:, meant] - want['image'][:, meant]) / want['scale'][meant])) <= BOUND
        want = check(c, w, kind, True, nonzero=meant)
        img, wsum, _ = call(ctx, c, weights=w, kind=kind, chan_avg=True)
        assert NP.all(NP.isfinite(img)) and wsum.shape == (1,) and deviation(img, want) <= BOUND
        for chan_avg in (False, True):
            img, wsum, _ = call(ctx, c, weights=NP.zeros_like(w), kind=kind, chan_avg=chan_avg)
            assert NP.all(NP.isnan(img)) and NP.all(wsum == 0.0)
    img, wsum, _ = call(ctx, c, weights=NP.zeros(37))
    assert NP.all(NP.isnan(img)) and NP.all(wsum == 0.0)


def test_f5_the_budget_leaves_the_bits_unchanged(ctx):
    c = IC.case(37, 70, 1000, 3)
    for chan_avg in (False, True):
        smallest = 256 * (32 * 3 + 8 * 70 + (8 if chan_avg else 0))      # one block of pixels on one stream
        for kind in ('dirty', 'psf'):
            full, wf, st = call(ctx, c, weights=c['w_full'], kind=kind, chan_avg=chan_avg)
            assert st['chunks'] == 1 and st['streams'] == 1 and st['precision'] == 'single'
            small, ws, st = call(ctx, c, weights=c['w_full'], kind=kind, chan_avg=chan_avg, budget_bytes=smallest)
            assert st['chunks'] == 4 and st['chunk_pixels'] == 256 and st['streams'] == 1
            assert NP.array_equal(full, small) and NP.array_equal(wf, ws), (kind, chan_avg)
            two, _, st = call(ctx, c, weights=c['w_full'], kind=kind, chan_avg=chan_avg, budget_bytes=2 * smallest)
            assert st['chunks'] == 4 and st['streams'] == 2 and NP.array_equal(full, two), (kind, chan_avg)
            with pytest.raises(ValueError, match='cannot hold one block'):
                call(ctx, c, weights=c['w_full'], kind=kind, chan_avg=chan_avg, budget_bytes=smallest - 1)


def test_f6_refusals_write_nothing_and_shared_faults_are_answered_alike(ctx):
    c = IC.case(37, K + 1, 65, 3)
    odd = IC.case(37, K + 1, 65, 3, uniform=False)
    p, lib, h, byref = _abi._ptr, ctx._lib, ctx._h, _abi.C.byref
    npix, nchan = 65, K + 1
    rot = NP.ascontiguousarray(c['rot'].reshape(-1, 9))
    out = {name: (NP.full((npix, nchan), -7.0), NP.full(nchan, -7.0)) for name in ('prisim_dirty_image', 'prisim_dirty_image_f32')}
    shared = dict(npix=npix, nbl=37, nchan=nchan, nt=3, unitvec=c['unitvec'], rot=rot, aberr_beta=c['beta'], pc_dircos=c['pc'],
                  baselines=c['baselines'], freqs_hz=c['freqs'], cube=c['cube'], weights=c['w_full'], kind=0, weight_form=2, chan_avg=0, route=-1,
                  budget_bytes=0)

    def entry(name, **kw):
        a, keep = ctx.PrisimImagingArgs(), []
        for field, val in dict(shared, **kw).items():
            if isinstance(val, NP.ndarray):
                val = NP.ascontiguousarray(val)
                keep.append(val)
                val = p(val)
            setattr(a, field, val)
        rc = getattr(lib, name)(h, byref(a), p(out[name][0]), p(out[name][1]), None)
        return rc, lib.prisim_hip_last_error(h).decode()

    def untouched():
        return all(NP.all(o == -7.0) for pair in out.values() for o in pair)

    def changed(name, index, value):
        x = NP.array(rot if name == 'rot' else c[name], dtype=NP.float64)
        x[index] = value
        return x

    # this route's own: DIRECT, and a grid that is not uniform under AUTO and under STEPPED; each names the fp64 entry
    for kw, msg in (({'route': _abi.PRISIM_IMAGE_DIRECT}, 'DIRECT'), ({'freqs_hz': odd['freqs'], 'route': _abi.PRISIM_IMAGE_AUTO}, 'uniform'),
                    ({'freqs_hz': odd['freqs'], 'route': _abi.PRISIM_IMAGE_STEPPED}, 'uniform')):
        rc, err = entry('prisim_dirty_image_f32', **kw)
        assert rc == _abi.PRISIM_EINVAL and msg in err and 'call prisim_dirty_image' in err, (kw.get('route'), rc, err)
        assert untouched()
    with pytest.raises(ValueError, match='call prisim_dirty_image'):
        call(ctx, c, route='direct')
    with pytest.raises(ValueError, match='call prisim_dirty_image'):
        call(ctx, odd)
    # the shared faults of test_g1_the_three_entries_refuse_a_shared_argument_alike: one code and one sentence from both entries
    faults = [({'unitvec': changed('unitvec', (3, 0), 1.5)}, 'unitvec[3]'), ({'rot': changed('rot', (1, 4), 0.5)}, 'rot of snapshot 1'),
              ({'aberr_beta': changed('beta', (2, 1), 0.02)}, 'aberr_beta of snapshot 2'),
              ({'weights': changed('w_full', (1, 2, 3), -1.0)}, 'finite and non-negative'), ({'nchan': 0}, '>= 1'),
              ({'route': 2}, 'unknown route'),
              ({'baselines': changed('baselines', (4, 1), 6e8)}, 'phase range: max|b| * 2 * max|f| / c = '),
              ({'baselines': changed('baselines', (4, 1), 1e200)}, 'the limit is below 2^29 = 536870912 cycles')]
    for kw, msg in faults:
        answers = {name: entry(name, **kw) for name in out}
        assert len(set(answers.values())) == 1, (list(kw), answers)
        rc, err = answers['prisim_dirty_image_f32']
        assert rc == _abi.PRISIM_EINVAL and msg in err, (list(kw), rc, err)
        assert untouched(), list(kw)
    # a null struct and a null output
    assert lib.prisim_dirty_image_f32(h, None, p(out['prisim_dirty_image_f32'][0]), None, None) == _abi.PRISIM_EINVAL and untouched()
    # and the unchanged arguments are taken by both, into the arrays that were left alone so far
    assert all(entry(name)[0] == _abi.PRISIM_OK for name in out)
    img, wsum, _ = call(ctx, c, weights=c['w_full'])
    assert NP.array_equal(out['prisim_dirty_image_f32'][0], img) and NP.array_equal(out['prisim_dirty_image_f32'][1], wsum)
    assert NP.array_equal(out['prisim_dirty_image'][1], wsum) and not NP.array_equal(out['prisim_dirty_image'][0], img)


def test_f7_resident_cube(ctx):
    c = IC.case(37, K + 1, 65, 3)
    host, _, st = call(ctx, c, weights=c['w_bl'])
    assert st['resident'] is False
    with _abi.Context(0) as fresh:
        with pytest.raises(RuntimeError, match='no resident'):
            call(fresh, c, cube=None)                                 # PRISIM_ESTATE: no array was ever set
        assert call(fresh, c, cube=None, kind='psf')[0].shape == (65, K + 1)      # the beam needs no cube of either kind
    ctx.set_array(c['baselines'], c['freqs'], nt_max=3)
    for t in range(3):
        ctx.set_vis(NP.ascontiguousarray(c['cube'][t]), slot=t)
    img, _, st = call(ctx, c, cube=None, weights=c['w_bl'])
    assert st['resident'] is True and st['precision'] == 'single' and NP.array_equal(img, host)
    ctx.set_array(c['baselines'], c['freqs'], nt_max=2)
    with pytest.raises(ValueError, match='resident cube has 2 slots'):
        call(ctx, c, cube=None)


def test_f8_through_the_class_a_point_source_images_to_its_flux():
    S, nbl, nt = 2.75, 37, 2
    src = NP.array([[62.0, 140.0]])
    sky = SM.SkyModel(location=src, flux_ref=[S], spindex=[0.0], ref_freq=150e6)
    others = NP.stack((NP.linspace(20.0, 89.0, 64), NP.linspace(0.0, 350.0, 64)), axis=1)
    dirs = NP.vstack((src, others))
    res = TG._array(nbl, 'altaz', 'altaz', reserve=nt)
    TG._observe(res, sky, [90.0, 270.0], nt)
    aps = RI.ApertureSynthesis(res)
    aps.precision = 'single'
    img = aps.image(dirs, coords='altaz', datakey='noiseless')
    st = aps.image_stats
    assert img.shape == (65, TG.CH.size) and img.dtype == NP.float64 and st['precision'] == 'single' and st['resident'] is True
    assert st['route'] == 'stepped' and st['terms'] == 65 * nbl * TG.CH.size * nt
    dev = float(NP.max(NP.abs(img[0] - S)) / S)
    print('point source at its own direction: %.3e of S (bound %.1e)' % (dev, 2 * BOUND))
    assert dev <= 2 * BOUND
    assert NP.all(NP.abs(img[1:]) <= S * (1.0 + 2 * BOUND))           # nowhere brighter than at the source
    beam = aps.psf(NP.array([[0.0, 0.0, 1.0]]), coords='dircos')
    assert beam.shape == (1, TG.CH.size) and float(NP.max(NP.abs(beam - 1.0))) <= BOUND and aps.image_stats['precision'] == 'single'
    with pytest.raises(ValueError, match='direct'):
        aps.image(dirs, coords='altaz', route='direct')
    # an object that was never told otherwise takes the fp64 route, the same call and the same bits as precision = 'double'
    plain = RI.ApertureSynthesis(res).image(dirs, coords='altaz')
    aps.precision = 'double'
    assert NP.array_equal(plain, aps.image(dirs, coords='altaz')) and aps.image_stats['precision'] == 'double'
    assert not NP.array_equal(plain, img) and float(NP.max(NP.abs(plain[0] - S)) / S) <= 2e-11
