"""GPU (-m gpu): the imaging family -- k_img_dirs, img_tile_pass / img_rows / cycles_phasor of prisim_amd/csrc_imaging/imaging_kernels.h
and their callers k_img_sum and k_clean_update -- through the C-ABI against the 40-digit reference of tests/imaging_reference.py, not
against tests/imaging_checker.py, whose own error passes 1e-11 of the scale beyond 30 km baselines.  Seeded cases of
tests/imaging_cases.py with their baselines scaled by 1, 10, 100, 1000 and 8000 (300 m to 2400 km), on the whole sphere and on a field
of 0.01 rad, under THE RULE stated in that module: every element of every image, the output finite everywhere, nothing excused.

Shapes (nbl, nchan, npix, nt): the smallest there is; exact fits of the 32-row LDS pass, the 32-channel tile and a wave; a second pass
of one row, a second tile of one channel and a ragged block; three tiles and a second block of one pixel.  The bit equalities among the
entries (tests/test_gpu_mosaic.py, test_gpu_imclean.py, test_gpu_csclean.py) carry what is held here over to the mosaic and the CLEANs
at the 300 km decade as well.

The mosaic with a beam that is not 1, its fp32 route, prisim_clean_mosaic and the Cotton-Schwab entries with their lattice beam P are
held at the same baselines by tests/test_gpu_mosaic_reference.py against tests/mosaic_reference.py, which builds on this reference."""
import os
import sys

import numpy as NP
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import imaging_reference as R  # noqa: E402
import imclean_checker as CK  # noqa: E402
import skyvis_reference as SR  # noqa: E402

pytestmark = pytest.mark.gpu
K = R.TILE
FORMS = ('none', 'baseline', 'full')
CONFIGS = R.CONFIGS          # (33, 33, 65, 2) on all five decades, the other shapes on the first and the fourth; both pixel sets


def ident(v):
    return 'x'.join(str(x) for x in v) if isinstance(v, tuple) else str(v)


def call(ctx, c, weights=None, **kw):
    return ctx.dirty_image(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], cube=kw.pop('cube', c['cube']), weights=weights,
                           aberr_beta=c['beta'], **kw)


def held(ctx, c, geo, ref, weights, kind, route, chan_avg, label, asked=None):
    """One call under THE RULE; returns the worst deviation in units of the scale and of the bound."""
    img, wsum, st = call(ctx, c, weights=weights, kind=kind, chan_avg=chan_avg, route=asked or route)
    nt, npix, nbl, nchan = geo.cos.shape
    assert st['route'] == route and st['reseed'] == (K if route == 'stepped' else 1) and st['terms'] == npix * nbl * nchan * nt
    want, scale, wwant = (ref.band_image, ref.band_scale, ref.band_wsum) if chan_avg else (ref.image, ref.scale, ref.wsum)
    assert img.shape == want.shape and img.dtype == NP.float64 and NP.all(NP.isfinite(img))
    assert NP.all(NP.abs(wsum - wwant) <= nt * nbl * R.U * wwant)
    bound = R.bound(geo, c['freqs'], route, band=chan_avg)
    dev = NP.abs(img - want) / scale
    worst = float(NP.max(dev / (bound[0] if chan_avg else bound)))
    print('%s %s chan_avg=%d %s: %.3e of the scale, %.3f of the bound' % (label, kind, chan_avg, route, float(dev.max()), worst))
    assert worst <= 1.0, (label, kind, chan_avg, route, float(dev.max()), worst)
    return float(dev.max()), worst


def all_ways(ctx, c, geo, weights, label, routes=('direct', 'stepped')):
    for kind in ('dirty', 'psf'):
        ref = R.image(geo, c['cube'], weights, kind)
        for chan_avg in (False, True):
            for route in routes:
                held(ctx, c, geo, ref, weights, kind, route, chan_avg, label)


@pytest.mark.parametrize('shape, scale, field', CONFIGS, ids=ident)
def test_r1_every_element_under_the_rule(ctx, shape, scale, field):
    c, geo = R.case(shape, scale, field), R.geometry_of(shape, scale, field)
    forms = FORMS if (shape, scale) == ((33, 33, 65, 2), 1000) else ('full',)
    for form in forms:
        all_ways(ctx, c, geo, R.weights_of(c, form), '%s x%d %s weights=%s' % (shape, scale, field, form))


@pytest.mark.parametrize('scale', (1, 1000))
def test_r2_non_uniform_grid_is_direct(ctx, scale):
    shape = (33, 33, 65, 2)
    c, geo = R.case(shape, scale, 'sphere', False), R.geometry_of(shape, scale, 'sphere', False)
    ref = R.image(geo, c['cube'], c['w_full'], 'dirty')
    for chan_avg in (False, True):
        held(ctx, c, geo, ref, c['w_full'], 'dirty', 'direct', chan_avg, 'non-uniform x%d' % scale, asked='auto')


@pytest.mark.parametrize('scale', (100, 1000))
def test_r2_a_grid_at_the_edge_of_the_uniform_rule_is_stepped_within_its_gap_term(ctx, scale):
    """Channels three units in the last place (8.9e-8 Hz) either side of their line, inside the 1e-7 Hz rule: AUTO steps, and the stepped
    phase (f0 + j df) tau is off the true one by up to grid_gap tau_max cycles, which THE RULE carries."""
    c = R.edge_grid_case(scale)
    f = c['freqs']
    geo = R.geometry_case(c)
    gap_term = 2.0 * NP.pi * R.grid_gap(f) * geo.tau_max
    print('x%d: the gap term is %.3e, the rule without it %.3e' % (scale, gap_term, float(R.bound(geo, f, 'direct').max())))
    for kind in ('dirty', 'psf'):
        ref = R.image(geo, c['cube'], c['w_full'], kind)
        for chan_avg in (False, True):
            held(ctx, c, geo, ref, c['w_full'], kind, 'stepped', chan_avg, 'edge grid x%d' % scale, asked='auto')


@pytest.mark.parametrize('scale', (1, 1000))
def test_r3_edges_of_the_geometry(ctx, scale):
    """R = I and beta = 0: a pixel at the phase centre exactly, its antipode, pixels on the axes, a zero baseline, baselines along one axis."""
    c = R.edges_case(scale)
    geo = R.geometry_case(c)
    assert NP.all(geo.d[0, 0] == 0.0) and NP.array_equal(geo.d[0, 1], [0.0, 0.0, -2.0]) and NP.all(c['baselines'][0] == 0.0)
    assert NP.all(geo.cos[0, 0] == 1) and NP.all(geo.sin[0, 0] == 0) and NP.all(geo.cos[0, :, 0] == 1)
    for form in ('none', 'full'):
        all_ways(ctx, c, geo, R.weights_of(c, form), 'edges x%d weights=%s' % (scale, form))
    # the pixel at the phase centre: every phasor is 1 on the device too, so D = sum w Re V to the roundings of the sum alone
    img, _, _ = call(ctx, c, weights=c['w_full'], route='direct')
    want = R.image(geo, c['cube'], c['w_full'], 'dirty')
    assert NP.all(NP.abs(img[0] - want.image[0]) <= 2 * c['nbl'] * R.U * want.scale)
    psf, _, _ = call(ctx, c, weights=c['w_full'], kind='psf', route='stepped')
    assert NP.all(NP.abs(psf[0] - 1.0) <= 2 * c['nbl'] * R.U)


def test_r3_whole_and_half_cycles(ctx):
    """f = 2^27 Hz, baselines c 2^-k m along East, pixels East, West and the zenith: the reference's phasors are (1, 0) and (-1, 0)
    exactly, and the device, whose b / c is rounded, stays inside THE RULE of 2^27 / 2^24 = 8 cycles."""
    c = R.exact_case()
    geo = R.geometry_case(c)
    sign = NP.array([1, 1, 1, 1, -1])
    assert NP.all(geo.cos[0, 0, :, 0] == sign) and NP.all(geo.cos[0, 1, :, 0] == sign) and NP.all(geo.cos[0, 2, :, 0] == 1) and NP.all(geo.sin == 0)
    for form in FORMS:
        all_ways(ctx, c, geo, R.weights_of(c, form), 'whole and half cycles weights=%s' % form)


def test_r4_the_largest_accepted_phase_range_is_finite_and_under_the_rule(ctx):
    """One baseline, one channel, five pixels at the last length below 2^29 cycles of max|b| 2 max|f| / c; the next double up is refused."""
    c = R.largest_case()
    length, top = R.range_edge()
    geo = R.geometry_case(c)
    assert 2.0 ** 29 * (1.0 - 1e-12) < 2.0 * geo.Nb[0] < 2.0 ** 29
    all_ways(ctx, c, geo, None, 'the largest accepted range')
    before = call(ctx, c)[0]
    c['baselines'] = NP.array([[top, 0.0, 0.0]])
    with pytest.raises(ValueError, match=r'phase range: max\|b\| \* 2 \* max\|f\| / c = 5.36871e\+08 cycles, the limit is below 2\^29 = 536870912 cycles'):
        call(ctx, c)
    c['baselines'] = NP.array([[0.0, 1e200, 1e200]])                    # finite components, a length that overflows
    with pytest.raises(ValueError, match='phase range'):
        call(ctx, c)
    c['baselines'] = NP.array([[length, 0.0, 0.0]])
    assert NP.array_equal(call(ctx, c)[0], before)                       # and the context goes on as before


@pytest.mark.parametrize('scale', (1, 100, 1000, 8000))
def test_r5_clean_replay_at_long_baselines(ctx, scale):
    """prisim_clean_image followed by the replay of tests/imclean_checker.py on the reference's phasors: every pick, flux, stop and
    residual within THE RULE of the scale plus the update's two-chain rule of sum |a|."""
    shape = (33, 33, 65, 2)
    c, geo = R.case(shape, scale), R.geometry_of(shape, scale)
    E = (geo.cos.astype(NP.float64) + 1j * geo.sin.astype(NP.float64))
    for chan_avg in (False, True):
        pb = CK.Problem(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], c['cube'], weights=c['w_full'], aberr_beta=c['beta'],
                        chan_avg=chan_avg, E=E)
        ref = R.image_of(shape, scale)
        assert NP.allclose(pb.scale, ref.band_scale if chan_avg else ref.scale, rtol=1e-14, atol=0)
        for route in ('direct', 'stepped'):
            got = ctx.clean_image(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], cube=c['cube'], weights=c['w_full'],
                                  aberr_beta=c['beta'], chan_avg=chan_avg, route=route, gain=0.3, maxiter=8, threshold=0.0,
                                  threshold_relative=False)
            assert got['stats']['route'] == route and NP.all(got['ncomp'] == 8) and NP.all(NP.isfinite(got['residual']))
            bound = (R.bound(geo, c['freqs'], route, band=chan_avg), R.update_bound(geo, c['freqs'], route, band=chan_avg))
            worst = CK.replay(pb, got, 0.3, 8, 0.0, False, bound=bound)
            print('clean x%d chan_avg=%d %s: %.3f of the tolerance' % (scale, chan_avg, route, worst))
            assert worst <= 1.0


def test_r6_adjoint_of_the_sky_sum_at_300_km(ctx):
    """<x, D> = Re <w V, V_sim(x)>: the fp64 sky-sum (ctx.skyvis) on the reference's directions rounded to doubles, the image with R = I
    and beta = 0 on the same doubles.  The bound is the sum of the two modules' rules, and of the one thing that separates the two
    statements: the image normalises its unit vectors, the sky-sum takes them as they are, | |u| - 1 | on N_b."""
    shape, scale = (33, 33, 65, 2), 1000
    base, g0 = R.case(shape, scale), R.geometry_of(shape, scale)
    u = NP.ascontiguousarray(g0.s[0])
    npix, nbl, nchan = u.shape[0], base['nbl'], base['nchan']
    c = dict(base, nt=1, unitvec=u, rot=NP.eye(3)[None].copy(), beta=NP.zeros((1, 3)), pc=base['pc'][:1].copy(), w_full=base['w_full'][:1].copy())
    geo = R.geometry_case(c)
    off = max(abs(R.MP.sqrt(sum(R.MP.mpf(float(v)) ** 2 for v in row)) - 1) for row in u)
    rng = NP.random.default_rng(6)
    x = rng.uniform(0.5, 2.0, npix)
    ctx.set_array(c['baselines'], c['freqs'])
    vsim = ctx.skyvis(u, x[:, None] * NP.ones((1, nchan)), c['pc'][0])
    v = (vsim + 0.3 * NP.abs(vsim).mean() * (rng.standard_normal(vsim.shape) + 1j * rng.standard_normal(vsim.shape)))[None]
    w = c['w_full']
    n_sky = NP.max(NP.abs(c['baselines']) @ NP.abs(u - c['pc'][0]).T, axis=1)[:, None] * c['freqs'][None, :] / R.C_LIGHT      # (nbl, nchan)
    sky_rule = SR.f64_bound(max(SR.R_RECURRENCE, SR.R_DIRECT), n_sky)
    for route in ('direct', 'stepped'):
        img, wsum, st = call(ctx, c, cube=v, weights=w, route=route)
        assert st['route'] == route
        lhs = NP.einsum('p,pk->k', x, img * wsum[None, :])
        rhs = NP.einsum('bk,bk->k', w[0] * v[0], vsim.conj()).real
        img_rule = R.bound(geo, c['freqs'], route) + 2.0 * NP.pi * float(off) * geo.Nb
        bound = NP.abs(x).sum() * NP.einsum('bk,bk->k', w[0] * NP.abs(v[0]), img_rule[None, :] + sky_rule)
        dev = float(NP.max(NP.abs(lhs - rhs) / bound))
        print('adjoint at 300 km, %s: |<x, D> - Re<wV, V_sim>| is %.3e of its bound (%.3e of sum|x| sum w|V|)'
              % (route, dev, float(NP.max(NP.abs(lhs - rhs) / (NP.abs(x).sum() * NP.einsum('bk->k', w[0] * NP.abs(v[0])))))))
        assert NP.all(NP.abs(lhs - rhs) <= bound), (route, dev)
        assert NP.abs(rhs).max() > 1e6 * bound.max()
