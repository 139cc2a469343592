"""GPU: Hogbom CLEAN of dirty images with the exact beam on the device (include/prisim_imclean.h) -- through the C-ABI against the replay
of tests/imclean_checker.py, which follows the device's component lists and rebuilds every residual in complex128, and through
prisim_amd.interferometry.ApertureSynthesis.clean on a simulated two-source sky.

Bounds.  The replay's tolerance per image channel is 1e-11 (the project's fp64 bound) of the natural scale of the dirty image plus
the sum of |a| of the components so far, the scale of the model visibilities the updates have imaged; every pick, every flux, every
stop and every pixel of the final residual is held to it, nothing is skipped.  Two sources on a grid whose worst beam sidelobe s is
below 1/3: the peak stays on a source, and at the stop each source keeps at most thr P0 / (1 - s) <= 1.5 thr P0 of its flux.
Restoration: 1e-12 of sum |a| plus the residual, a thousand roundings of the exponentials' sum."""
import os
import sys

import numpy as NP
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import imaging_cases as IC  # noqa: E402
import imaging_checker as IK  # noqa: E402
import imclean_checker as CK  # noqa: E402

from prisim_amd import _abi, skymodel as SM  # noqa: E402
from prisim_amd import interferometry as RI  # noqa: E402

pytestmark = pytest.mark.gpu
K = 32
THRESHOLD, MAXITER, DEAD = _abi.PRISIM_IMCLEAN_THRESHOLD, _abi.PRISIM_IMCLEAN_MAXITER, _abi.PRISIM_IMCLEAN_DEAD
# (nbl, nchan, npix, nt): the smallest there is; 63 pixels of one ragged block; 1000 pixels in four blocks with a second channel tile of
# one channel
SHAPES = [(1, 1, 1, 1), (37, 5, 63, 1), (37, K + 1, 1000, 3)]
FORMS = ('none', 'baseline', 'full')
_CASES, _PHASORS = {}, {}


def case(shape, uniform=True):
    """The seeded inputs of a shape and their phasors, made once for the module."""
    key = (shape, uniform)
    if key not in _CASES:
        c = _CASES[key] = IC.case(*shape, uniform=uniform)
        _PHASORS[key] = CK.Problem(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], c['cube'], aberr_beta=c['beta']).E
    return _CASES[key], _PHASORS[key]


def weights_of(c, form):
    return {'none': None, 'baseline': c['w_bl'], 'full': c['w_full']}[form]


def problem(c, E, weights, chan_avg, window=None, nonzero=None):
    return CK.Problem(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], c['cube'], weights=weights, aberr_beta=c['beta'],
                      chan_avg=chan_avg, window=window, nonzero=nonzero, E=E)


def run(ctx, c, weights=None, **kw):
    return ctx.clean_image(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], cube=kw.pop('cube', c['cube']), weights=weights,
                           aberr_beta=c['beta'], **kw)


def same_bits(a, b):
    return all(NP.array_equal(a[n], b[n], equal_nan=True) for n in ('residual', 'comp_pixel', 'comp_flux', 'ncomp', 'status', 'peak0', 'wsum')) \
        and (a['restored'] is None) == (b['restored'] is None) and (a['restored'] is None or NP.array_equal(a['restored'], b['restored'], equal_nan=True))


@pytest.mark.parametrize('form', FORMS)
def test_g1_no_iterations_leave_the_dirty_image_bit_for_bit(ctx, form):
    c, _ = case(SHAPES[2])
    w = weights_of(c, form)
    for scale in (1.0, 1000.0):                                       # to 300 m, and to 300 km where tests/imaging_reference.py holds the image
        c = dict(c, baselines=c['baselines'] * scale)
        for chan_avg in (False, True):
            for route in ('direct', 'stepped'):
                want, wsum, _ = ctx.dirty_image(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], cube=c['cube'], weights=w,
                                                aberr_beta=c['beta'], chan_avg=chan_avg, route=route)
                got = run(ctx, c, weights=w, chan_avg=chan_avg, route=route, maxiter=0, threshold=0.0, threshold_relative=False)
                nc = 1 if chan_avg else K + 1
                assert got['residual'].shape == want.shape and NP.array_equal(got['residual'], want), (form, scale, chan_avg, route)
                assert NP.array_equal(got['wsum'], wsum) and got['restored'] is None
                assert got['comp_pixel'].shape == (nc, 0) and got['comp_flux'].shape == (nc, 0) and NP.all(got['ncomp'] == 0)
                assert NP.all(got['status'] == MAXITER)                   # a peak above the threshold and no component allowed
                assert NP.array_equal(got['peak0'], NP.abs(want).reshape(want.shape[0], nc).max(axis=0))
                st = got['stats']
                assert st['route'] == route and st['iterations'] == 0 and st['components'] == 0 and st['polls'] == 1 and st['resident'] is False
                assert st['terms'] == 1000 * 37 * (K + 1) * 3 and st['chan_tile'] == K and st['block_pixels'] == 256 and st['lds_bytes'] == 17792


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(str(v) for v in s))
def test_g2_replay_parity(ctx, shape, form):
    c, E = case(shape)
    nbl = shape[0]
    w = weights_of(c, form)
    if nbl >= 7:
        assert NP.count_nonzero(NP.asarray(c['w_bl']) == 0.0) == nbl // 7
    for chan_avg in (False, True):
        pb = problem(c, E, w, chan_avg)
        for route in ('direct', 'stepped'):
            got = run(ctx, c, weights=w, chan_avg=chan_avg, route=route, gain=0.3, maxiter=25, threshold=0.0, threshold_relative=False)
            assert got['stats']['route'] == route and got['residual'].dtype == NP.float64
            worst = CK.replay(pb, got, 0.3, 25, 0.0, False)
            print('%s weights=%s chan_avg=%d %s: %d components, worst deviation %.2e of its tolerance'
                  % (shape, form, chan_avg, route, int(got['ncomp'].sum()), worst))
            # with a threshold of 0 nothing stops early but a residual that is exactly 0 (one pixel, one baseline)
            assert NP.all((got['status'] == MAXITER) | (got['ncomp'] < 25))
            assert got['stats']['components'] == int(got['ncomp'].sum()) and got['stats']['iterations'] == int(got['ncomp'].max())


def test_g2_non_uniform_grid_and_a_window(ctx):
    c, E = case(SHAPES[2], uniform=False)
    pb = problem(c, E, c['w_full'], False)
    got = run(ctx, c, weights=c['w_full'], gain=0.3, maxiter=25, threshold=0.0, threshold_relative=False)
    assert got['stats']['route'] == 'direct' and got['stats']['reseed'] == 1          # AUTO on this grid
    print('non-uniform grid: worst deviation %.2e of its tolerance' % CK.replay(pb, got, 0.3, 25, 0.0, False))
    with pytest.raises(ValueError, match='uniform'):
        run(ctx, c, weights=c['w_full'], route='stepped')
    # every odd pixel excluded: no component there, every pixel updated all the same
    c, E = case(SHAPES[2])
    window = NP.arange(1000) % 2 == 0
    for chan_avg in (False, True):
        pb = problem(c, E, c['w_bl'], chan_avg, window=window)
        got = run(ctx, c, weights=c['w_bl'], chan_avg=chan_avg, gain=0.3, maxiter=25, threshold=0.0, threshold_relative=False, window=window)
        assert got['stats']['route'] == 'stepped' and NP.all(got['comp_pixel'] % 2 == 0)
        print('window, chan_avg=%d: worst deviation %.2e of its tolerance' % (chan_avg, CK.replay(pb, got, 0.3, 25, 0.0, False)))
        free = run(ctx, c, weights=c['w_bl'], chan_avg=chan_avg, gain=0.3, maxiter=25, threshold=0.0, threshold_relative=False)
        assert NP.any(free['comp_pixel'] % 2 == 1)                    # the window was what kept them away


# ---- two sources -------------------------------------------------------------------------------------------------------------------------

def two_sources():
    """150 baselines to 300 m, 33 channels, a 17 x 17 grid of direction cosines to 0.2, one snapshot, identity frames, zenith phase
    centre; 1.0 Jy on pixel (row 5, column 3) and 0.6 Jy on (11, 12), the cube by the checker's sky-sum."""
    base = IC.case(150, K + 1, 289, 1)
    grid = RI.ApertureSynthesis.dircos_grid(17, 0.2)
    src = NP.array([5 * 17 + 3, 11 * 17 + 12])
    flux = NP.array([1.0, 0.6])
    c = {'unitvec': grid, 'rot': NP.eye(3)[None], 'beta': None, 'pc': NP.array([[0.0, 0.0, 1.0]]), 'baselines': base['baselines'],
         'freqs': base['freqs'], 'w_bl': base['w_bl']}
    c['cube'] = IK.skysum(grid[src][None], flux, c['pc'], c['baselines'], c['freqs'])
    c['w_full'] = None
    return c, src, flux


def worst_sidelobe(pb, channels):
    """The largest |beam| between two different pixels, over the given channels, from the checker's phasors and weights: the beam
    centred on pixel q, at pixel p, is Re sum_{t,b} w E_p conj(E_q) / sum w."""
    worst = 0.0
    for k in channels:
        A, w = pb.E[:, :, :, k], pb.w[:, :, k]
        beam = NP.einsum('tpb,tb,tqb->pq', A, w, A.conj()).real / w.sum()
        assert NP.allclose(NP.diag(beam), 1.0, rtol=0, atol=1e-12)
        worst = max(worst, float(NP.max(NP.abs(beam - NP.diag(NP.diag(beam))))))
    return worst


@pytest.mark.parametrize('chan_avg', [False, True], ids=['per_channel', 'chan_avg'])
@pytest.mark.parametrize('form', ['none', 'baseline'])
def test_g3_two_sources_are_recovered(ctx, form, chan_avg):
    if 'g3' not in _CASES:
        _CASES['g3'] = two_sources()
        c = _CASES['g3'][0]
        _PHASORS['g3'] = CK.Problem(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], c['cube']).E
    (c, src, flux), E = _CASES['g3'], _PHASORS['g3']
    weights = weights_of(c, form)
    pb = CK.Problem(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], c['cube'], weights=weights, chan_avg=chan_avg, E=E)
    s = worst_sidelobe(pb, (0, K))
    print('worst sidelobe at the band edges, weights %s: %.3f' % (form, s))
    assert s < 1.0 / 3.0
    got = run(ctx, c, weights=weights, chan_avg=chan_avg)             # the defaults: gain 0.1, relative 5e-3
    nc = 1 if chan_avg else K + 1
    assert NP.all(got['status'] == THRESHOLD), got['status']
    used = got['comp_pixel'][got['comp_pixel'] >= 0]
    assert NP.all(NP.isin(used, src)), NP.unique(used)
    for k in range(nc):
        n = got['ncomp'][k]
        for q, S in zip(src, flux):
            total = got['comp_flux'][k, :n][got['comp_pixel'][k, :n] == q].sum()
            assert abs(S - total) <= 1.5 * 5e-3 * got['peak0'][k], (chan_avg, k, q, S, total)
    worst = CK.replay(pb, got, 0.1, 10000, 5e-3, True)
    print('two sources, chan_avg=%d: %d iterations, worst deviation %.2e of its tolerance' % (chan_avg, got['stats']['iterations'], worst))


def test_g4_a_channel_without_weight_is_dead_and_delays_nobody(ctx):
    c, E = case(SHAPES[2])
    w = c['w_full'].copy()
    w[:, :, 20] = 0.0
    meant = NP.ones(K + 1, dtype=bool)
    meant[20] = False
    for route in ('direct', 'stepped'):
        got = run(ctx, c, weights=w, route=route, gain=0.3, maxiter=25, threshold=0.0, threshold_relative=False)
        assert NP.array_equal(got['status'] == DEAD, ~meant) and got['ncomp'][20] == 0 and NP.isnan(got['peak0'][20])
        assert NP.array_equal(NP.isnan(got['residual']), NP.broadcast_to(~meant, got['residual'].shape))
        assert NP.all(got['ncomp'][meant] == 25) and got['stats']['iterations'] == 25
        CK.replay(problem(c, E, w, False, nonzero=meant), got, 0.3, 25, 0.0, False)
        band = run(ctx, c, weights=w, route=route, chan_avg=True, gain=0.3, maxiter=25, threshold=0.0, threshold_relative=False)
        assert NP.all(NP.isfinite(band['residual'])) and band['status'][0] == MAXITER
        CK.replay(problem(c, E, w, True, nonzero=meant), band, 0.3, 25, 0.0, False)
        for chan_avg in (False, True):
            none = run(ctx, c, weights=NP.zeros_like(w), route=route, chan_avg=chan_avg, fwhm_rad=0.01)
            assert NP.all(none['status'] == DEAD) and NP.all(none['ncomp'] == 0) and NP.all(NP.isnan(none['residual']))
            assert NP.all(NP.isnan(none['restored'])) and NP.all(NP.isnan(none['peak0'])) and none['stats']['iterations'] == 0


def test_g5_polling_and_repetition_leave_the_bits_unchanged(ctx):
    """A relative threshold of a half: the channels end after different numbers of iterations, so ended channels sit through the
    updates of the others, and batches of 1, 7 and 32 iterations end at different places."""
    c, _ = case(SHAPES[2])
    for chan_avg in (False, True):
        for route in ('direct', 'stepped'):
            kw = dict(weights=c['w_full'], chan_avg=chan_avg, route=route, gain=0.3, maxiter=25, threshold=0.5, fwhm_rad=0.02)
            first = run(ctx, c, **kw)
            if not chan_avg:
                assert len(set(first['ncomp'].tolist())) > 1 and NP.any(first['status'] == THRESHOLD)
            assert first['stats']['polls'] == 1
            for poll in (1, 7):
                other = run(ctx, c, poll_every=poll, **kw)
                assert same_bits(first, other), (chan_avg, route, poll)
                assert other['stats']['iterations'] == first['stats']['iterations'] and other['stats']['polls'] >= first['stats']['iterations'] // poll
            assert same_bits(first, run(ctx, c, **kw)), (chan_avg, route)


def test_g6_refusals_write_nothing(ctx):
    c, _ = case((37, K + 1, 63, 1))
    p, lib, h = _abi._ptr, ctx._lib, ctx._h
    npix, nchan, maxiter = 63, K + 1, 5
    rot = NP.ascontiguousarray(c['rot'].reshape(-1, 9))
    outs = {'out_residual': NP.full((npix, nchan), -7.0), 'out_restored': NP.full((npix, nchan), -7.0),
            'out_comp_pixel': NP.full((nchan, maxiter), -7, dtype=NP.int32), 'out_comp_flux': NP.full((nchan, maxiter), -7.0),
            'out_ncomp': NP.full(nchan, -7, dtype=NP.int32), 'out_status': NP.full(nchan, -7, dtype=NP.int32),
            'out_peak0': NP.full(nchan, -7.0), 'out_wsum': NP.full(nchan, -7.0)}
    order = ('out_residual', 'out_restored', 'out_comp_pixel', 'out_comp_flux', 'out_ncomp', 'out_status', 'out_peak0', 'out_wsum')
    window = NP.ones(npix, dtype=NP.uint8)
    fwhm = NP.full(nchan, 0.01)

    def entry(null=(), **kw):
        a = ctx.PrisimImcleanArgs()
        v = dict(npix=npix, nbl=37, nchan=nchan, nt=1, unitvec=c['unitvec'], rot=rot, aberr_beta=c['beta'], pc_dircos=c['pc'],
                 baselines=c['baselines'], freqs_hz=c['freqs'], cube=c['cube'], weights=c['w_full'], window=window, fwhm_rad=fwhm, gain=0.3,
                 threshold=0.1, maxiter=maxiter, budget_bytes=0, weight_form=2, chan_avg=0, route=-1, threshold_relative=1, poll_every=0)
        v.update(kw)
        keep = []
        for name, val in v.items():
            if isinstance(val, NP.ndarray):
                val = NP.ascontiguousarray(val)
                keep.append(val)
                val = p(val)
            setattr(a, name, val)
        rc = lib.prisim_clean_image(h, _abi.C.byref(a), *[None if n in null else p(outs[n]) for n in order], None)
        return rc, lib.prisim_hip_last_error(h).decode()

    def changed(x, index, value):
        x = NP.array(x)
        x[index] = value
        return x

    need = 32 * npix + 8 * npix * nchan + 12 * nchan * maxiter + 16 * nchan + (36 * nchan + 8 * nchan + 24) + npix
    refusals = [(dict(unitvec=None), 'unitvec is NULL'), (dict(freqs_hz=None), 'freqs_hz is NULL'), (dict(weights=None), 'weights is NULL'),
                (dict(null=('out_residual',)), 'out_residual is NULL'), (dict(null=('out_comp_flux',)), 'out_comp_flux'),
                (dict(null=('out_status',)), 'out_status'), (dict(null=('out_peak0',)), 'out_peak0'),
                (dict(fwhm_rad=None), 'needs fwhm_rad'),
                (dict(gain=0.0), 'gain'), (dict(gain=1.5), 'gain'), (dict(gain=NP.nan), 'gain'), (dict(maxiter=-1), 'maxiter'),
                (dict(threshold=1.0), 'below 1'), (dict(threshold=NP.inf, threshold_relative=0), 'finite'), (dict(threshold=NP.nan), 'finite'),
                (dict(threshold=-0.1), 'finite and non-negative'), (dict(window=NP.zeros(npix, dtype=NP.uint8)), 'window holds no pixel'),
                (dict(fwhm_rad=changed(fwhm, 3, 0.0)), 'fwhm_rad[3]'), (dict(fwhm_rad=changed(fwhm, 3, NP.inf)), 'fwhm_rad[3]'),
                (dict(route=1, freqs_hz=c['freqs'] + 3e4 * NP.sin(NP.arange(nchan))), 'uniform'), (dict(route=2), 'unknown route'),
                (dict(budget_bytes=need - 1), 'cannot hold the whole image (the resident buffers take %d B' % need),
                (dict(weights=changed(c['w_full'], (0, 2, 3), -1.0)), 'finite and non-negative'), (dict(npix=0), '>= 1')]
    for kw, msg in refusals:
        rc, err = entry(**kw)
        assert rc == _abi.PRISIM_EINVAL and msg in err, (list(kw), rc, err)
        assert all(NP.all(o == -7) for o in outs.values()), list(kw)  # nothing is written unless the call succeeds
    # the resident cube: none at all is a matter of state, one of another shape a wrong argument
    with _abi.Context(0) as fresh:
        with pytest.raises(RuntimeError, match='no resident'):
            run(fresh, c, cube=None)
    ctx.set_array(c['baselines'][:36], c['freqs'], nt_max=1)
    rc, err = entry(cube=None)
    assert rc == _abi.PRISIM_EINVAL and 'resident cube has 1 slots of 36 baselines' in err and all(NP.all(o == -7) for o in outs.values())
    # and the budget that just holds the image runs, with the results of the wrapper
    rc, err = entry(budget_bytes=need)
    assert rc == _abi.PRISIM_OK, err
    want = run(ctx, c, weights=c['w_full'], gain=0.3, threshold=0.1, maxiter=maxiter, fwhm_rad=fwhm)
    assert NP.array_equal(outs['out_residual'], want['residual']) and NP.array_equal(outs['out_restored'], want['restored'])
    assert NP.array_equal(outs['out_ncomp'], want['ncomp']) and NP.array_equal(outs['out_status'], want['status'])
    for k in range(nchan):
        n = want['ncomp'][k]
        assert NP.array_equal(outs['out_comp_pixel'][k, :n], want['comp_pixel'][k, :n]) and NP.all(outs['out_comp_pixel'][k, n:] == -7)
        assert NP.array_equal(outs['out_comp_flux'][k, :n], want['comp_flux'][k, :n]) and NP.all(outs['out_comp_flux'][k, n:] == -7.0)
    # the resident cube read where it lies gives the bits of the handed-over one
    ctx.set_array(c['baselines'], c['freqs'], nt_max=1)
    ctx.set_vis(NP.ascontiguousarray(c['cube'][0]), slot=0)
    res = run(ctx, c, cube=None, weights=c['w_full'], gain=0.3, threshold=0.1, maxiter=maxiter, fwhm_rad=fwhm)
    assert res['stats']['resident'] is True and same_bits(res, want)


def test_g7_restoration_against_numpy(ctx):
    c, _ = case(SHAPES[2])
    for chan_avg in (False, True):
        nc = 1 if chan_avg else K + 1
        fwhm = NP.linspace(0.02, 0.05, nc)
        got = run(ctx, c, weights=c['w_bl'], chan_avg=chan_avg, gain=0.3, maxiter=25, threshold=0.2, fwhm_rad=fwhm)
        want = CK.restored(got['residual'], c['unitvec'], got['comp_pixel'], got['comp_flux'], got['ncomp'], fwhm)
        spent = NP.abs(got['comp_flux']).sum(axis=1)
        bound = 1e-12 * (spent + NP.abs(got['residual']).reshape(1000, nc))
        dev = NP.abs(got['restored'].reshape(1000, nc) - want.reshape(1000, nc))
        print('restoration, chan_avg=%d: %.3e of its bound' % (chan_avg, float(NP.max(dev / bound))))
        assert got['restored'].shape == got['residual'].shape and NP.all(dev <= bound)
        assert NP.max(NP.abs(got['restored'] - got['residual'])) > 0.0
        assert same_bits(dict(got, restored=None), run(ctx, c, weights=c['w_bl'], chan_avg=chan_avg, gain=0.3, maxiter=25, threshold=0.2))


# ---- through the classes ----------------------------------------------------------------------------------------------------------------

LAT = -30.7224
CH = 150e6 + 1e5 * NP.arange(K + 1)
TELESCOPE = {'id': 'custom', 'shape': 'delta', 'size': 14.0, 'ocoords': 'altaz', 'orientation': NP.array([[90.0, 270.0]]), 'groundplane': None}
LSTS = [30.0, 31.5]


def _observed(sky, nbl, reserve):
    rng = NP.random.default_rng(77)
    bl = rng.uniform(-1.0, 1.0, (nbl, 3)) * NP.array([200.0, 200.0, 5.0])
    ia = RI.InterferometerArray([(str(i + 1), '0') for i in range(nbl)], bl, CH, telescope=TELESCOPE, latitude=LAT, skycoords='altaz',
                                pointing_coords='altaz')
    ia.frame_model = 'date'
    if reserve:
        ia.reserve(len(LSTS))
    for j, lst in enumerate(LSTS):
        ia.observe((2457000.5 + j / 64.0, lst), {'Tnet': 200.0}, NP.ones(CH.size), [90.0, 270.0], sky, 10.7)
    return ia


def test_g8_through_the_classes_on_a_simulated_sky():
    flux = NP.array([1.0, 0.6])
    src = NP.array([[62.0, 140.0], [75.0, 310.0]])
    sky = SM.SkyModel(location=src, flux_ref=flux, spindex=[0.0, 0.0], ref_freq=150e6)
    others = NP.stack((NP.linspace(30.0, 88.0, 14), NP.linspace(5.0, 340.0, 14)), axis=1)
    dirs = NP.vstack((src, others))
    res = _observed(sky, 150, reserve=True)
    aps = RI.ApertureSynthesis(res)
    # the worst sidelobe between two of the directions, from the checker
    uv, rot, beta, pc, _, _ = aps._prepare('psf', dirs, 'altaz', None, None, None, 'auto')
    zero = NP.zeros((len(LSTS), 150, K + 1), dtype=NP.complex128)
    s = worst_sidelobe(CK.Problem(uv, rot, pc, res._baselines_local(), CH, zero, aberr_beta=beta), (0, K))
    print('worst sidelobe among the directions: %.3f' % s)
    assert s < 1.0 / 3.0
    out = aps.clean(dirs, coords='altaz')
    st = aps.image_stats
    assert st['resident'] is True and st['route'] == 'stepped' and st['terms'] == 16 * 150 * (K + 1) * 2 and st['wsum'].shape == (K + 1,)
    assert set(out) == {'residual', 'restored', 'model', 'components', 'status', 'peak0', 'threshold', 'fwhm'}
    assert out['residual'].shape == out['restored'].shape == out['model'].shape == (16, K + 1)
    assert NP.all(out['status'] == THRESHOLD) and NP.allclose(out['threshold'], 5e-3 * out['peak0'], rtol=1e-15)
    pix, flx, count = out['components']['pixel'], out['components']['flux'], out['components']['count']
    assert NP.all(NP.isin(pix[pix >= 0], (0, 1)))
    model = NP.zeros((16, K + 1))
    for k in range(K + 1):
        NP.add.at(model[:, k], pix[k, :count[k]], flx[k, :count[k]])
    assert NP.array_equal(out['model'], model) and NP.all(out['model'][2:] == 0.0)
    assert NP.all(NP.abs(out['model'][:2] - flux[:, None]) <= 1.5 * 5e-3 * out['peak0'][None, :])
    # the same run without reserve(): the cube is handed over, every output has the same bits
    host = _observed(sky, 150, reserve=False)
    aph = RI.ApertureSynthesis(host)
    other = aph.clean(dirs, coords='altaz')
    assert aph.image_stats['resident'] is False
    for name in ('residual', 'restored', 'model', 'status', 'peak0', 'threshold', 'fwhm'):
        assert NP.array_equal(out[name], other[name]), name
    assert all(NP.array_equal(out['components'][n], other['components'][n]) for n in ('pixel', 'flux', 'count'))
    band = aps.clean(dirs, coords='altaz', chan_avg=True, restore=False)
    assert band['residual'].shape == (16,) and band['restored'] is None and band['fwhm'].shape == (1,)
    assert NP.all(NP.abs(band['model'][:2] - flux) <= 1.5 * 5e-3 * band['peak0'][0])
