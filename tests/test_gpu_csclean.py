"""GPU: Cotton-Schwab CLEAN of dirty images on the device (include/prisim_csclean.h) -- through the C-ABI against the replay of
tests/csclean_checker.py, which follows the device's component lists and cycle tables, rebuilds the exact residual of every major
cycle in complex128 and asserts every decision, and through prisim_amd.interferometry.ApertureSynthesis.clean_cotton_schwab on a
simulated two-source sky.

Bounds.  The replay's tolerance per image channel is 1e-11 (the project's fp64 bound) of the natural scale of the dirty image plus
the sum of |a| of the components so far; every Pc, pick, flux, end of a cycle, status, the final residual and the residual
visibilities are held to it, nothing is skipped.  Two sources on a grid whose worst beam sidelobe s is below 1/3: at the stop each
source keeps at most thr P0 / (1 - s) <= 1.5 thr P0 of its flux, the bound of tests/test_gpu_imclean.py.  The minor-cycle beam against
the exact one, for baselines without a third component: both are sums of cosines whose phases reach 10^3 rad and carry a few units in
the last place of the direction differences, 10^3 * 4 * 2^-52 = 1e-12."""
import os
import sys

import numpy as NP
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import csclean_cases as CC  # noqa: E402
import csclean_checker as CS  # noqa: E402
import imaging_cases as IC  # noqa: E402
import imaging_checker as IK  # noqa: E402
import imclean_checker as CK  # noqa: E402

from prisim_amd import _abi, skymodel as SM  # noqa: E402
from prisim_amd import interferometry as RI  # noqa: E402

pytestmark = pytest.mark.gpu
K = 32
THRESHOLD, MAXITER, DEAD = _abi.PRISIM_IMCLEAN_THRESHOLD, _abi.PRISIM_IMCLEAN_MAXITER, _abi.PRISIM_IMCLEAN_DEAD
MAJOR, DIVERGED = _abi.PRISIM_CSCLEAN_MAJOR, _abi.PRISIM_CSCLEAN_DIVERGED
# (nbl, nchan, ny, nx, nt): the smallest there is; 63 pixels of one ragged block, neither side a divisor of 256; 1000 pixels in four
# blocks, wider than high, with a second channel tile of one channel and three snapshots of different frames
SHAPES = [(1, 1, 1, 1, 1), (37, 5, 9, 7, 1), (37, K + 1, 25, 40, 3)]
FORMS = ('none', 'baseline', 'full')
# gain 0.3, maxiter 25, absolute threshold 0, then (cycle_depth, cycle_niter, max_major)
SETTING_A = dict(gain=0.3, maxiter=25, threshold=0.0, threshold_relative=False, cycle_depth=0.5, cycle_niter=4, max_major=10)
SETTING_B = dict(gain=0.3, maxiter=25, threshold=0.0, threshold_relative=False, cycle_depth=0.8, cycle_niter=0, max_major=4)
NAMES = ('residual', 'comp_pixel', 'comp_flux', 'ncomp', 'status', 'peak0', 'wsum', 'ncycles', 'cycle_ncomp', 'cycle_peak', 'psf', 'vres', 'restored')
_CASES, _PHASORS = {}, {}


def case(shape, uniform=True):
    """The seeded inputs of a shape and their phasors, made once for the module."""
    key = (shape, uniform)
    if key not in _CASES:
        c = _CASES[key] = CC.case(*shape, uniform=uniform)
        _PHASORS[key] = CK.Problem(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], c['cube'], aberr_beta=c['beta']).E
    return _CASES[key], _PHASORS[key]


def weights_of(c, form):
    return {'none': None, 'baseline': c['w_bl'], 'full': c['w_full']}[form]


def problem(c, E, weights, chan_avg, window=None, nonzero=None):
    return CK.Problem(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], c['cube'], weights=weights, aberr_beta=c['beta'],
                      chan_avg=chan_avg, window=window, nonzero=nonzero, E=E)


def beam_of(c, pb):
    return CS.beam(pb, c['unitvec'], c['rot'], c['baselines'], c['freqs'], c['ny'], c['nx'])


def run(ctx, c, weights=None, **kw):
    return ctx.clean_image_cs(c['unitvec'], (c['ny'], c['nx']), c['rot'], c['pc'], c['baselines'], c['freqs'], cube=kw.pop('cube', c['cube']),
                              weights=weights, aberr_beta=c['beta'], **kw)


def replay_args(kw):
    return tuple(kw[n] for n in ('gain', 'maxiter', 'threshold', 'threshold_relative', 'cycle_depth', 'cycle_niter', 'max_major'))


def same_bits(a, b):
    return all((a[n] is None) == (b[n] is None) and (a[n] is None or NP.array_equal(a[n], b[n], equal_nan=True)) for n in NAMES)


@pytest.mark.parametrize('form', FORMS)
def test_g1_no_cycle_and_no_component_leave_the_dirty_image_bit_for_bit(ctx, form):
    c, _ = case(SHAPES[2])
    w = weights_of(c, form)
    for scale in (1.0, 1000.0):                                       # to 300 m, and to 300 km where tests/imaging_reference.py holds the image
        c = dict(c, baselines=c['baselines'] * scale)
        for chan_avg in (False, True):
            for route in ('direct', 'stepped'):
                want, wsum, _ = ctx.dirty_image(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], cube=c['cube'], weights=w,
                                                aberr_beta=c['beta'], chan_avg=chan_avg, route=route)
                nc = 1 if chan_avg else K + 1
                for kw, status in ((dict(max_major=0, maxiter=25), MAJOR), (dict(max_major=4, maxiter=0), MAXITER), (dict(max_major=0, maxiter=0), MAXITER)):
                    got = run(ctx, c, weights=w, chan_avg=chan_avg, route=route, threshold=0.0, threshold_relative=False, want_vis=True, **kw)
                    assert got['residual'].shape == want.shape and NP.array_equal(got['residual'], want), (form, scale, chan_avg, route, kw)
                    assert NP.array_equal(got['wsum'], wsum) and got['restored'] is None and NP.array_equal(got['vres'], c['cube'])
                    assert got['comp_pixel'].shape == (nc, 0) and NP.all(got['ncomp'] == 0) and NP.all(got['ncycles'] == 0)
                    assert NP.all(got['status'] == status) and got['cycle_ncomp'].shape == (nc, 0)
                    peak = NP.abs(want).reshape(want.shape[0], nc).max(axis=0)
                    assert NP.array_equal(got['peak0'], peak) and NP.array_equal(got['cycle_peak'], peak[:, None])
                    st = got['stats']
                    assert st['route'] == route and st['cycles'] == 0 and st['components'] == 0 and st['polls'] == 1 and st['resident'] is False
                    assert st['terms'] == 1000 * 37 * (K + 1) * 3 and st['minor_route'] == 'lds' and st['minor_lds_bytes'] == 8064
                    assert st['psf_offsets'] == 25 * 79 - 40 + 1


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(str(v) for v in s))
def test_g2_replay_parity(ctx, shape, form):
    c, E = case(shape)
    w = weights_of(c, form)
    for chan_avg in (False, True):
        pb = problem(c, E, w, chan_avg)
        P = beam_of(c, pb)
        for name, kw in (('A', SETTING_A), ('B', SETTING_B)):
            seen = set()
            for route in ('direct', 'stepped'):
                got = run(ctx, c, weights=w, chan_avg=chan_avg, route=route, minor_route='lds', want_psf=True, want_vis=True, **kw)
                assert got['stats']['route'] == route and got['stats']['minor_route'] == 'lds' and got['residual'].dtype == NP.float64
                worst = CS.replay(pb, P, c['ny'], c['nx'], got, *replay_args(kw))
                seen |= set(got['status'].tolist())
                print('%s weights=%s chan_avg=%d %s %s: %d components, %d cycles, statuses %s, worst deviation %.2e of its tolerance'
                      % (shape, form, chan_avg, name, route, int(got['ncomp'].sum()), got['stats']['cycles'], sorted(set(got['status'].tolist())), worst))
                # the beam: even bit for bit, 1 at the centre, the checker's to rounding
                psf = got['psf']
                assert NP.array_equal(psf, psf[:, ::-1, ::-1]) and NP.all(psf[:, c['ny'] - 1, c['nx'] - 1] == 1.0)
                assert NP.max(NP.abs(psf - P)) <= 1e-12
                assert got['stats']['components'] == int(got['ncomp'].sum()) and got['stats']['cycles'] == int(got['ncycles'].max())
                assert got['stats']['polls'] == got['stats']['cycles'] + 1
                # the working image in device memory: the same bits
                other = run(ctx, c, weights=w, chan_avg=chan_avg, route=route, minor_route='global', want_psf=True, want_vis=True, **kw)
                assert other['stats']['minor_route'] == 'global' and other['stats']['minor_lds_bytes'] == 64 and same_bits(got, other), (chan_avg, name, route)
            # every status is exercised where the prototype of the definition met it
            if not chan_avg and shape != SHAPES[0]:
                if name == 'A':
                    assert {MAXITER, DIVERGED} <= seen, seen
                elif shape == SHAPES[1]:
                    assert {MAXITER, MAJOR} <= seen, seen


def test_g2_a_window_and_a_non_uniform_grid(ctx):
    c, E = case(SHAPES[2])
    window = NP.arange(1000) % 2 == 0                                 # every odd pixel excluded: no component there, every pixel updated
    for chan_avg in (False, True):
        pb = problem(c, E, c['w_bl'], chan_avg, window=window)
        P = beam_of(c, pb)
        got = run(ctx, c, weights=c['w_bl'], chan_avg=chan_avg, window=window, want_vis=True, **SETTING_A)
        assert got['stats']['route'] == 'stepped' and NP.all(got['comp_pixel'][got['comp_pixel'] >= 0] % 2 == 0)
        print('window, chan_avg=%d: worst deviation %.2e of its tolerance' % (chan_avg, CS.replay(pb, P, 25, 40, got, *replay_args(SETTING_A))))
        free = run(ctx, c, weights=c['w_bl'], chan_avg=chan_avg, **SETTING_A)
        assert NP.any(free['comp_pixel'][free['comp_pixel'] >= 0] % 2 == 1)                  # the window was what kept them away
    c, E = case(SHAPES[2], uniform=False)
    pb = problem(c, E, c['w_full'], False)
    got = run(ctx, c, weights=c['w_full'], want_vis=True, **SETTING_B)
    assert got['stats']['route'] == 'direct' and got['stats']['reseed'] == 1              # AUTO on this grid
    print('non-uniform grid: worst deviation %.2e of its tolerance' % CS.replay(pb, beam_of(c, pb), 25, 40, got, *replay_args(SETTING_B)))
    with pytest.raises(ValueError, match='uniform'):
        run(ctx, c, weights=c['w_full'], route='stepped')


# ---- two sources -------------------------------------------------------------------------------------------------------------------------

def two_sources(flat=False):
    """The scene of tests/test_gpu_imclean.py: 150 baselines to 300 m, 33 channels, a 17 x 17 grid of direction cosines to 0.2, one
    snapshot, identity frames, zenith phase centre; 1.0 Jy on pixel (row 5, column 3) and 0.6 Jy on (11, 12), the cube by the checker's
    sky-sum.  flat: the baselines without their third component."""
    base = IC.case(150, K + 1, 289, 1)
    grid = RI.ApertureSynthesis.dircos_grid(17, 0.2)
    src = NP.array([5 * 17 + 3, 11 * 17 + 12])
    flux = NP.array([1.0, 0.6])
    bl = base['baselines'].copy()
    if flat:
        bl[:, 2] = 0.0
    c = {'unitvec': grid, 'ny': 17, 'nx': 17, 'rot': NP.eye(3)[None], 'beta': None, 'pc': NP.array([[0.0, 0.0, 1.0]]), 'baselines': bl,
         'freqs': base['freqs'], 'w_bl': base['w_bl'], 'w_full': None}
    c['cube'] = IK.skysum(grid[src][None], flux, c['pc'], c['baselines'], c['freqs'])
    return c, src, flux


def scene(flat):
    key = ('g3', flat)
    if key not in _CASES:
        _CASES[key] = two_sources(flat)
        c = _CASES[key][0]
        _PHASORS[key] = CK.Problem(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], c['cube']).E
    return _CASES[key], _PHASORS[key]


def recovered(got, src, flux, nc):
    """every component on a source, and every source's flux to 1.5 thr P0"""
    used = got['comp_pixel'][got['comp_pixel'] >= 0]
    assert NP.all(NP.isin(used, src)), NP.unique(used)
    worst = 0.0
    for k in range(nc):
        n = got['ncomp'][k]
        for q, S in zip(src, flux):
            total = got['comp_flux'][k, :n][got['comp_pixel'][k, :n] == q].sum()
            worst = max(worst, abs(S - total) / (5e-3 * got['peak0'][k]))
            assert abs(S - total) <= 1.5 * 5e-3 * got['peak0'][k], (k, q, S, total)
    return worst


@pytest.mark.parametrize('chan_avg', [False, True], ids=['per_channel', 'chan_avg'])
@pytest.mark.parametrize('form', ['none', 'baseline'])
def test_g3_two_sources_are_recovered(ctx, form, chan_avg):
    (c, src, flux), E = scene(False)
    weights = weights_of(c, form)
    pb = CK.Problem(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], c['cube'], weights=weights, chan_avg=chan_avg, E=E)
    got = run(ctx, c, weights=weights, chan_avg=chan_avg, want_vis=True)                  # the defaults: gain 0.1, relative 5e-3, depth 0.3
    nc = 1 if chan_avg else K + 1
    assert NP.all(got['status'] == THRESHOLD), got['status']
    worst = recovered(got, src, flux, nc)
    assert got['ncycles'].max() <= 8
    dev = CS.replay(pb, beam_of(c, pb), 17, 17, got, 0.1, 10000, 5e-3, True, 0.3, 0, 32)
    print('two sources, weights %s, chan_avg=%d: %d to %d cycles, %d to %d components, fluxes to %.2f thr P0, worst deviation %.2e of its tolerance'
          % (form, chan_avg, got['ncycles'].min(), got['ncycles'].max(), got['ncomp'].min(), got['ncomp'].max(), worst, dev))


@pytest.mark.parametrize('chan_avg', [False, True], ids=['per_channel', 'chan_avg'])
def test_g3_without_a_w_term_the_minor_beam_is_the_exact_one(ctx, chan_avg):
    (c, src, flux), E = scene(True)
    pb = CK.Problem(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], c['cube'], weights=c['w_bl'], chan_avg=chan_avg, E=E)
    nc = 1 if chan_avg else K + 1
    got = run(ctx, c, weights=c['w_bl'], chan_avg=chan_avg, cycle_depth=0.1, want_psf=True)
    for q in (0, int(src[0]), 288):
        exact = pb.beams([0] if chan_avg else NP.arange(nc), [q] * nc, NP.ones(nc))
        mine = NP.stack([CS.shifted(got['psf'][k], q, 17, 17) for k in range(nc)], axis=1)
        print('the minor beam against the exact one at pixel %d: %.2e' % (q, NP.max(NP.abs(exact - mine))))
        assert NP.max(NP.abs(exact - mine)) <= 1e-12
    assert NP.all(got['status'] == THRESHOLD) and NP.all(got['ncycles'] == 3), got['ncycles']
    recovered(got, src, flux, nc)
    hogbom = ctx.clean_image(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], cube=c['cube'], weights=c['w_bl'], chan_avg=chan_avg)
    assert NP.all(NP.abs(got['ncomp'] - hogbom['ncomp']) <= 3), (got['ncomp'], hogbom['ncomp'])
    CS.replay(pb, beam_of(c, pb), 17, 17, got, 0.1, 10000, 5e-3, True, 0.1, 0, 32)


def test_g4_a_channel_without_weight_is_dead_and_delays_nobody(ctx):
    c, E = case(SHAPES[2])
    w = c['w_full'].copy()
    w[:, :, 20] = 0.0
    meant = NP.ones(K + 1, dtype=bool)
    meant[20] = False
    for route in ('direct', 'stepped'):
        got = run(ctx, c, weights=w, route=route, want_vis=True, **SETTING_A)
        assert NP.array_equal(got['status'] == DEAD, ~meant) and got['ncomp'][20] == 0 and got['ncycles'][20] == 0 and NP.isnan(got['peak0'][20])
        assert NP.array_equal(NP.isnan(got['residual']), NP.broadcast_to(~meant, got['residual'].shape))
        assert NP.all(NP.isnan(got['cycle_peak'][20])) and NP.all(got['cycle_ncomp'][20] == -1) and NP.array_equal(got['vres'][:, :, 20], c['cube'][:, :, 20])
        assert NP.all(got['ncycles'][meant] >= 2) and NP.all((got['ncomp'][meant] == 25) | (got['status'][meant] == DIVERGED))
        pb = problem(c, E, w, False, nonzero=meant)
        CS.replay(pb, beam_of(c, pb), 25, 40, got, *replay_args(SETTING_A))
        band = run(ctx, c, weights=w, route=route, chan_avg=True, want_vis=True, **SETTING_A)
        assert NP.all(NP.isfinite(band['residual'])) and band['status'][0] in (MAXITER, DIVERGED)
        pb = problem(c, E, w, True, nonzero=meant)
        CS.replay(pb, beam_of(c, pb), 25, 40, band, *replay_args(SETTING_A))
        for chan_avg in (False, True):
            none = run(ctx, c, weights=NP.zeros_like(w), route=route, chan_avg=chan_avg, fwhm_rad=0.01)
            assert NP.all(none['status'] == DEAD) and NP.all(none['ncomp'] == 0) and NP.all(NP.isnan(none['residual']))
            assert NP.all(NP.isnan(none['restored'])) and NP.all(NP.isnan(none['peak0'])) and none['stats']['cycles'] == 0


def test_g5_repetition_and_routes_leave_the_bits_unchanged(ctx):
    """A relative threshold of a half: the channels end after different numbers of cycles, so ended channels sit through the major
    cycles of the others and must come back with the same bits each time."""
    c, _ = case(SHAPES[2])
    for chan_avg in (False, True):
        for route in ('direct', 'stepped'):
            kw = dict(weights=c['w_full'], chan_avg=chan_avg, route=route, gain=0.3, maxiter=25, threshold=0.5, cycle_depth=0.7, cycle_niter=3,
                      max_major=10, fwhm_rad=0.02, want_psf=True, want_vis=True)
            first = run(ctx, c, **kw)
            if not chan_avg:
                assert len(set(first['ncycles'].tolist())) > 1 and NP.any(first['status'] == THRESHOLD)
            assert first['stats']['minor_route'] == 'lds' and NP.max(NP.abs(first['restored'] - first['residual'])) > 0.0
            assert same_bits(first, run(ctx, c, **kw)), (chan_avg, route)
            assert same_bits(first, run(ctx, c, minor_route='global', **kw)), (chan_avg, route)
            # the residual is the dirty image of the residual visibilities, bit for bit
            image, _, _ = ctx.dirty_image(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], cube=first['vres'], weights=c['w_full'],
                                          aberr_beta=c['beta'], chan_avg=chan_avg, route=route)
            assert NP.array_equal(image, first['residual']), (chan_avg, route)
            want = CK.restored(first['residual'], c['unitvec'], first['comp_pixel'], first['comp_flux'], first['ncomp'], NP.full(first['ncomp'].size, 0.02))
            bound = 1e-12 * (NP.abs(first['comp_flux']).sum(axis=1) + NP.abs(first['residual']).reshape(1000, -1))
            assert NP.all(NP.abs(first['restored'].reshape(1000, -1) - want.reshape(1000, -1)) <= bound)


def test_g6_refusals_write_nothing(ctx):
    c, _ = case((37, K + 1, 9, 7, 1))
    p, lib, h = _abi._ptr, ctx._lib, ctx._h
    npix, nchan, maxiter, major = 63, K + 1, 5, 3
    rot = NP.ascontiguousarray(c['rot'].reshape(-1, 9))
    outs = {'out_residual': NP.full((npix, nchan), -7.0), 'out_restored': NP.full((npix, nchan), -7.0),
            'out_comp_pixel': NP.full((nchan, maxiter), -7, dtype=NP.int32), 'out_comp_flux': NP.full((nchan, maxiter), -7.0),
            'out_ncomp': NP.full(nchan, -7, dtype=NP.int32), 'out_status': NP.full(nchan, -7, dtype=NP.int32),
            'out_peak0': NP.full(nchan, -7.0), 'out_wsum': NP.full(nchan, -7.0), 'out_ncycles': NP.full(nchan, -7, dtype=NP.int32),
            'out_cycle_ncomp': NP.full((nchan, major), -7, dtype=NP.int32), 'out_cycle_peak': NP.full((nchan, major + 1), -7.0),
            'out_psf': NP.full((nchan, 17, 13), -7.0), 'out_vres': NP.full((1, 37, nchan), -7.0 + 0j)}
    order = ('out_residual', 'out_restored', 'out_comp_pixel', 'out_comp_flux', 'out_ncomp', 'out_status', 'out_peak0', 'out_wsum', 'out_ncycles',
             'out_cycle_ncomp', 'out_cycle_peak', 'out_psf', 'out_vres')
    window = NP.ones(npix, dtype=NP.uint8)
    fwhm = NP.full(nchan, 0.01)

    def entry(null=(), **kw):
        a = ctx.PrisimCscleanArgs()
        v = dict(npix=npix, nbl=37, nchan=nchan, nt=1, unitvec=c['unitvec'], rot=rot, aberr_beta=c['beta'], pc_dircos=c['pc'],
                 baselines=c['baselines'], freqs_hz=c['freqs'], cube=c['cube'], weights=c['w_full'], window=window, fwhm_rad=fwhm, gain=0.3,
                 threshold=0.1, maxiter=maxiter, budget_bytes=0, weight_form=2, chan_avg=0, route=-1, threshold_relative=1, ny=9, nx=7,
                 cycle_depth=0.5, cycle_niter=2, max_major=major, minor_route=-1)
        v.update(kw)
        keep = []
        for name, val in v.items():
            if isinstance(val, NP.ndarray):
                val = NP.ascontiguousarray(val)
                keep.append(val)
                val = p(val)
            setattr(a, name, val)
        rc = lib.prisim_clean_image_cs(h, _abi.C.byref(a), *[None if n in null else p(outs[n]) for n in order], None)
        return rc, lib.prisim_hip_last_error(h).decode()

    def changed(x, index, value):
        x = NP.array(x)
        x[index] = value
        return x

    def untouched():
        return all(NP.all(o == -7) for o in outs.values())

    half = 9 * 13 - 7 + 1
    need = (32 * npix + 8 * npix * nchan + 12 * nchan * maxiter + 16 * nchan + (36 * nchan + 8 * nchan + 24) + npix            # prisim_clean_image's
            + 16 * 37 * nchan + 8 * nchan * 17 * 13 + (32 * half + 8 * half * nchan) + (28 * nchan + 4 * nchan * major + 8 * nchan * (major + 1)))
    refusals = [(dict(ny=9, nx=8), 'ny * nx must be npix'), (dict(ny=0, nx=63), 'ny * nx'), (dict(ny=-9, nx=-7), 'ny * nx'),
                (dict(cycle_depth=0.0), 'cycle_depth'), (dict(cycle_depth=1.0), 'cycle_depth'), (dict(cycle_depth=NP.nan), 'cycle_depth'),
                (dict(max_major=-1), 'max_major'), (dict(max_major=65537), 'max_major'), (dict(minor_route=2), 'minor_route'),
                (dict(budget_bytes=need - 1), 'cannot hold the resident buffers (the resident buffers take %d B' % need),
                (dict(null=('out_ncycles',)), 'out_ncycles'), (dict(null=('out_cycle_ncomp',)), 'out_cycle_ncomp'), (dict(null=('out_cycle_peak',)), 'out_cycle_peak'),
                # those of prisim_clean_image
                (dict(unitvec=None), 'unitvec is NULL'), (dict(freqs_hz=None), 'freqs_hz is NULL'), (dict(weights=None), 'weights is NULL'),
                (dict(null=('out_residual',)), 'out_residual is NULL'), (dict(null=('out_comp_flux',)), 'out_comp_flux'),
                (dict(null=('out_status',)), 'out_status'), (dict(null=('out_peak0',)), 'out_peak0'), (dict(fwhm_rad=None), 'needs fwhm_rad'),
                (dict(gain=0.0), 'gain'), (dict(gain=1.5), 'gain'), (dict(gain=NP.nan), 'gain'), (dict(maxiter=-1), 'maxiter'),
                (dict(threshold=1.0), 'below 1'), (dict(threshold=NP.inf, threshold_relative=0), 'finite'), (dict(threshold=NP.nan), 'finite'),
                (dict(threshold=-0.1), 'finite and non-negative'), (dict(window=NP.zeros(npix, dtype=NP.uint8)), 'window holds no pixel'),
                (dict(fwhm_rad=changed(fwhm, 3, 0.0)), 'fwhm_rad[3]'), (dict(fwhm_rad=changed(fwhm, 3, NP.inf)), 'fwhm_rad[3]'),
                (dict(route=1, freqs_hz=c['freqs'] + 3e4 * NP.sin(NP.arange(nchan))), 'uniform'), (dict(route=2), 'unknown route'),
                (dict(weights=changed(c['w_full'], (0, 2, 3), -1.0)), 'finite and non-negative'), (dict(npix=0), '>= 1')]
    for kw, msg in refusals:
        rc, err = entry(**kw)
        assert rc == _abi.PRISIM_EINVAL and msg in err, (list(kw), rc, err)
        assert untouched(), list(kw)                                  # nothing is written unless the call succeeds
    # a working image that does not fit in the LDS of a workgroup: 144 x 144 pixels of 8 B against 160 KiB; AUTO takes the device memory
    big = CC.case(3, 1, 144, 144, 1)
    with pytest.raises(ValueError, match='does not fit in the LDS'):
        run(ctx, big, minor_route='lds', maxiter=2, max_major=1)
    auto = run(ctx, big, maxiter=2, max_major=1)
    assert auto['stats']['minor_route'] == 'global' and NP.all(auto['ncomp'] == 2)
    # ... and one beyond 64 KiB that does: 96 x 96 pixels, which a kernel has to be allowed
    mid = CC.case(3, 2, 96, 96, 1)
    lds = run(ctx, mid, minor_route='lds', maxiter=3, max_major=2, want_vis=True)
    assert lds['stats']['minor_lds_bytes'] == 96 * 96 * 8 + 64 and NP.all(lds['ncomp'] == 3)
    assert same_bits(lds, run(ctx, mid, minor_route='global', maxiter=3, max_major=2, want_vis=True))
    # the resident cube: none at all is a matter of state, one of another shape a wrong argument
    with _abi.Context(0) as fresh:
        with pytest.raises(RuntimeError, match='no resident'):
            run(fresh, c, cube=None)
    ctx.set_array(c['baselines'][:36], c['freqs'], nt_max=1)
    rc, err = entry(cube=None)
    assert rc == _abi.PRISIM_EINVAL and 'resident cube has 1 slots of 36 baselines' in err and untouched()
    # and the budget that just holds the call runs, with the results of the wrapper
    rc, err = entry(budget_bytes=need)
    assert rc == _abi.PRISIM_OK, err
    kw = dict(weights=c['w_full'], gain=0.3, threshold=0.1, maxiter=maxiter, cycle_depth=0.5, cycle_niter=2, max_major=major, fwhm_rad=fwhm,
              window=window, want_psf=True, want_vis=True)
    want = run(ctx, c, **kw)
    assert want['stats']['device_bytes'] == need
    for name, key in (('out_residual', 'residual'), ('out_restored', 'restored'), ('out_ncomp', 'ncomp'), ('out_status', 'status'), ('out_peak0', 'peak0'),
                      ('out_wsum', 'wsum'), ('out_ncycles', 'ncycles'), ('out_psf', 'psf'), ('out_vres', 'vres')):
        assert NP.array_equal(outs[name], want[key]), name
    for k in range(nchan):
        n, m = want['ncomp'][k], want['ncycles'][k]
        assert NP.array_equal(outs['out_comp_pixel'][k, :n], want['comp_pixel'][k, :n]) and NP.all(outs['out_comp_pixel'][k, n:] == -7)
        assert NP.array_equal(outs['out_comp_flux'][k, :n], want['comp_flux'][k, :n]) and NP.all(outs['out_comp_flux'][k, n:] == -7.0)
        assert NP.array_equal(outs['out_cycle_ncomp'][k, :m], want['cycle_ncomp'][k, :m]) and NP.all(outs['out_cycle_ncomp'][k, m:] == -7)
        assert NP.array_equal(outs['out_cycle_peak'][k, :m + 1], want['cycle_peak'][k, :m + 1]) and NP.all(outs['out_cycle_peak'][k, m + 1:] == -7.0)
    # the resident cube, copied on the device, gives the bits of the handed-over one and keeps its own
    ctx.set_array(c['baselines'], c['freqs'], nt_max=1)
    ctx.set_vis(NP.ascontiguousarray(c['cube'][0]), slot=0)
    res = run(ctx, c, cube=None, **kw)
    assert res['stats']['resident'] is True and same_bits(res, want) and NP.any(res['vres'] != c['cube'])
    assert NP.array_equal(ctx.get_vis(slot=0), c['cube'][0])


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


def test_g7_through_the_classes_on_a_simulated_sky():
    # a 7 x 9 lattice of direction cosines around the zenith as (alt, az), the two sources on two of its pixels
    l, m = NP.meshgrid(NP.linspace(-0.32, 0.32, 9), NP.linspace(-0.27, 0.27, 7))
    l, m = l.ravel(), m.ravel()
    dirs = NP.degrees(NP.stack((NP.arcsin(NP.sqrt(1.0 - l * l - m * m)), NP.arctan2(l, m) % (2 * NP.pi)), axis=1))
    at = NP.array([2 * 9 + 6, 5 * 9 + 1])
    flux = NP.array([1.0, 0.6])
    sky = SM.SkyModel(location=dirs[at], flux_ref=flux, spindex=[0.0, 0.0], ref_freq=150e6)
    res = _observed(sky, 150, reserve=True)
    aps = RI.ApertureSynthesis(res)
    # the worst sidelobe between two of the directions, from the checker
    uv, rot, beta, pc, _, _ = aps._prepare('psf', dirs, 'altaz', None, None, None, 'auto')
    zero = NP.zeros((len(LSTS), 150, K + 1), dtype=NP.complex128)
    pb = CK.Problem(uv, rot, pc, res._baselines_local(), CH, zero, aberr_beta=beta)
    s = 0.0
    for k in (0, K):
        A = pb.E[:, :, :, k]
        b = NP.einsum('tpb,tqb->pq', A, A.conj()).real / (len(LSTS) * 150)
        s = max(s, float(NP.max(NP.abs(b - NP.diag(NP.diag(b))))))
    print('worst sidelobe among the directions: %.3f' % s)
    assert s < 1.0 / 3.0
    out = aps.clean_cotton_schwab(dirs, (7, 9), coords='altaz', return_vis=True)
    st = aps.image_stats
    assert st['resident'] is True and st['route'] == 'stepped' and st['minor_route'] == 'lds' and st['terms'] == 63 * 150 * (K + 1) * 2
    assert set(out) == {'residual', 'restored', 'model', 'components', 'status', 'peak0', 'threshold', 'fwhm', 'cycles', 'residual_vis'}
    assert out['residual'].shape == out['restored'].shape == out['model'].shape == (63, K + 1) and out['residual_vis'].shape == (150, K + 1, 2)
    assert NP.all(out['status'] == THRESHOLD) and NP.allclose(out['threshold'], 5e-3 * out['peak0'], rtol=1e-15)
    pix, count = out['components']['pixel'], out['components']['count']
    assert NP.all(NP.isin(pix[pix >= 0], at)) and out['cycles']['count'].max() <= 8
    assert NP.all(out['cycles']['ncomp'][NP.arange(K + 1), out['cycles']['count'] - 1] == count)
    assert NP.all(NP.abs(out['model'][at] - flux[:, None]) <= 1.5 * 5e-3 * out['peak0'][None, :])
    assert NP.all(NP.delete(out['model'], at, axis=0) == 0.0)
    # the same run without reserve(): the cube is handed over, every output has the same bits
    host = _observed(sky, 150, reserve=False)
    aph = RI.ApertureSynthesis(host)
    other = aph.clean_cotton_schwab(dirs, (7, 9), coords='altaz', return_vis=True)
    assert aph.image_stats['resident'] is False
    for name in ('residual', 'restored', 'model', 'status', 'peak0', 'threshold', 'fwhm', 'residual_vis'):
        assert NP.array_equal(out[name], other[name]), name
    assert all(NP.array_equal(out['components'][n], other['components'][n]) for n in ('pixel', 'flux', 'count'))
    assert all(NP.array_equal(out['cycles'][n], other['cycles'][n], equal_nan=True) for n in ('count', 'ncomp', 'peak'))
    # the resident cube is what it was: clean() of it finds the full fluxes again
    again = aps.clean(dirs, coords='altaz', restore=False)
    assert NP.all(NP.abs(again['model'][at] - flux[:, None]) <= 1.5 * 5e-3 * again['peak0'][None, :])
    band = aps.clean_cotton_schwab(dirs, (7, 9), coords='altaz', chan_avg=True, restore=False)
    assert band['residual'].shape == (63,) and band['restored'] is None and band['fwhm'].shape == (1,) and band['residual_vis'] is None
    assert NP.all(NP.abs(band['model'][at] - flux) <= 1.5 * 5e-3 * band['peak0'][0])
