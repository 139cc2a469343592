"""GPU: Cotton-Schwab CLEAN of the beam-weighted mosaic on the device (include/prisim_moscs.h) -- through the C-ABI against
prisim_mosaic_image bit for bit with no cycle, against the replay of the numpy checker (tests/moscs_checker.py), which follows the
device's component lists and cycle tables, rebuilds the mosaic's numerator of V - model at every major cycle in complex128 and asserts
every decision; on two sources seen through a drifting chromatic beam; on the edge cases of the weights, the mask and the horizon; the
bit equality between repeated calls, the two routes of the minor cycle, the resident cube and the mosaic of the residual
visibilities; the refusals; and through prisim_amd.interferometry.ApertureSynthesis on a drift scan that observe() simulated.

Bounds: those of the checker, derived in its docstring from the project's 1e-11 of an fp64 image sum and 1e-12 of a device beam value;
the quotients and the mask are asserted exactly from the returned num, den and wsum; P to 1e-12 (tests/test_gpu_csclean.py).  The two
sources and the drift scan: 1.5 thresholds in the units of F plus the replay's tolerance of a flux, the bounds of
tests/test_gpu_mosclean.py.  No element is left out of any comparison.

G4, the snapshot with everything down.  Its beam is 0, so it adds exactly nothing to N and Q: with no component the call has the bits
of the same call with that snapshot's weights at 0 (num, den, residual), and that is asserted.  Once a component is taken the two
calls are different problems by the header's own definition -- Wtot, which scales F, and P, the synthesized beam of ALL weights, which
the primary beam does not enter, both hold the weights of the snapshot that is down -- so their lists agree to rounding at best and
cannot agree bit for bit; both are held to the replay instead.  What "contributes exactly nothing" does mean after cycles is asserted
bit for bit: every output is unchanged when that snapshot's visibilities are replaced by others, and its residual visibilities come
back as they went in."""
import ctypes as C
import os
import sys

import numpy as NP
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mosaic_cases as MC  # noqa: E402
import mosclean_checker as QK  # noqa: E402
import moscs_cases as XC  # noqa: E402
import moscs_checker as XK  # noqa: E402

from prisim_amd import _abi, skymodel as SM  # noqa: E402
from prisim_amd import interferometry as RI  # noqa: E402

pytestmark = pytest.mark.gpu
K = XC.K
THRESHOLD, MAXITER, DEAD = _abi.PRISIM_IMCLEAN_THRESHOLD, _abi.PRISIM_IMCLEAN_MAXITER, _abi.PRISIM_IMCLEAN_DEAD
MAJOR, DIVERGED = _abi.PRISIM_CSCLEAN_MAJOR, _abi.PRISIM_CSCLEAN_DIVERGED
NAMES = ('residual', 'residual_flat', 'pb_eff', 'num', 'den', 'wsum', 'comp_pixel', 'comp_flux', 'ncomp', 'status', 'peak0', 'ncycles', 'cycle_ncomp',
         'cycle_peak', 'psf', 'vres', 'restored')
_MEMO = {}
_WORST = [0.0]


def base(shape, beam='gaussian', uniform=True):
    """The seeded inputs of a shape and the phasors and beams of the checker, made once for the module"""
    key = (shape, beam, uniform)
    if key not in _MEMO:
        c = XC.case(shape, uniform=uniform)
        _MEMO[key] = (c, XC.problem(c, beam=beam))
    return _MEMO[key]


def run(ctx, c, beam='gaussian', weights=None, **kw):
    kw.setdefault('pbmin', c['pbmin'])
    return ctx.clean_mosaic_cs(c['unitvec'], (c['ny'], c['nx']), c['rot'], c['pc'], c['baselines'], c['freqs'], XC.BEAMS[beam], c['dish'],
                               beam_pc_dircos=c['bpc'], cube=kw.pop('cube', c['cube']), weights=weights, aberr_beta=c['beta'], **kw)


def mosaic(ctx, c, beam='gaussian', weights=None, **kw):
    kw.setdefault('pbmin', c['pbmin'])
    return ctx.mosaic_image(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], XC.BEAMS[beam], c['dish'], beam_pc_dircos=c['bpc'],
                            cube=kw.pop('cube', c['cube']), weights=weights, aberr_beta=c['beta'], **kw)


def same(a, b):
    return NP.array_equal(a, b, equal_nan=True)


def same_bits(a, b, names=NAMES):
    return all((a[n] is None) == (b[n] is None) and (a[n] is None or same(a[n], b[n])) for n in names)


def replayed(pb, c, got, kw):
    if not hasattr(pb, 'minor_beam'):
        pb.minor_beam = XK.beam(pb, c['ny'], c['nx'])                 # once per problem: the runs of a test share it
    worst = XK.replay(pb, pb.minor_beam, c['ny'], c['nx'], got, *XC.replay_args(kw))
    _WORST[0] = max(_WORST[0], worst)
    return worst


# ---- G1: no cycle and no component leave the mosaic -----------------------------------------------------------------------------------

@pytest.mark.parametrize('form', XC.FORMS)
def test_g1_no_cycle_and_no_component_leave_the_mosaic_bit_for_bit(ctx, form):
    c, _ = base(XC.SHAPES[2])
    w = XC.weights_of(c, form)
    for chan_avg in (False, True):
        for route in ('direct', 'stepped'):
            want, num, den, wsum, st = mosaic(ctx, c, weights=w, chan_avg=chan_avg, route=route)
            nc = 1 if chan_avg else K + 1
            for kw, status in ((dict(max_major=0, maxiter=25), MAJOR), (dict(max_major=4, maxiter=0), MAXITER), (dict(max_major=0, maxiter=0), MAXITER)):
                got = run(ctx, c, weights=w, chan_avg=chan_avg, route=route, threshold=0.0, threshold_relative=False, want_vis=True, **kw)
                for name, ref in (('num', num), ('den', den), ('wsum', wsum), ('pb_eff', st['pb_eff']), ('residual', want)):
                    assert got[name].shape == ref.shape and same(got[name], ref), (name, form, chan_avg, route, kw)
                assert NP.any(NP.isnan(want)) and NP.any(NP.isfinite(want)) and got['restored'] is None and same(got['vres'], c['cube'])
                assert got['comp_pixel'].shape == (nc, 0) and NP.all(got['ncomp'] == 0) and NP.all(got['ncycles'] == 0)
                assert NP.all(got['status'] == status) and got['cycle_ncomp'].shape == (nc, 0)
                assert same(got['residual_flat'], QK.flat_of(num, den, wsum, c['pbmin'], chan_avg))
                peak = NP.nanmax(NP.abs(got['residual_flat']).reshape(1000, nc), axis=0)
                assert NP.array_equal(got['peak0'], peak) and NP.array_equal(got['cycle_peak'], peak[:, None])
                gs = got['stats']
                assert gs['route'] == route and gs['cycles'] == 0 and gs['components'] == 0 and gs['polls'] == 1 and gs['resident'] is False
                assert gs['terms'] == 1000 * 37 * (K + 1) * 3 and gs['minor_route'] == 'lds' and gs['minor_lds_bytes'] == 8064
                assert gs['psf_offsets'] == 25 * 79 - 40 + 1 and gs['lds_bytes'] == 17792 + 8 * K and gs['block_pixels'] == 256


# ---- G2: replay parity ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('form', XC.FORMS)
@pytest.mark.parametrize('shape', XC.SHAPES, ids=lambda s: 'x'.join(str(v) for v in s))
def test_g2_replay_parity(ctx, shape, form):
    c, shared = base(shape)
    nbl, nchan, ny, nx, nt = shape
    w = XC.weights_of(c, form)
    if nbl >= 7:
        assert NP.count_nonzero(NP.asarray(c['w_bl']) == 0.0) == nbl // 7
    for chan_avg in (False, True):
        pb = XC.problem(c, weights=w, chan_avg=chan_avg, share=shared)
        for name, kw in XC.SETTINGS.items():
            seen = set()
            # both routes of the passes; the long lists of setting C once, on the route AUTO takes
            for route in (('stepped',) if name == 'C' else ('direct', 'stepped')):
                got = run(ctx, c, weights=w, chan_avg=chan_avg, route=route, minor_route='lds', want_psf=True, want_vis=True, **kw)
                assert got['stats']['route'] == route and got['stats']['minor_route'] == 'lds' and got['residual'].dtype == NP.float64
                worst = replayed(pb, c, got, kw)
                seen |= set(got['status'].tolist())
                print('%s weights=%s chan_avg=%d %s %s: %d components, %d cycles, statuses %s, worst deviation %.2e of its tolerance'
                      % (shape, form, chan_avg, name, route, int(got['ncomp'].sum()), got['stats']['cycles'], sorted(set(got['status'].tolist())), worst))
                psf = got['psf']
                assert same(psf, psf[:, ::-1, ::-1]) and NP.all(psf[:, ny - 1, nx - 1] == 1.0)       # even bit for bit, 1 at the centre
                assert got['stats']['components'] == int(got['ncomp'].sum()) and got['stats']['cycles'] == int(got['ncycles'].max())
                assert got['stats']['polls'] == got['stats']['cycles'] + 1
                # the working image in device memory: the same bits
                other = run(ctx, c, weights=w, chan_avg=chan_avg, route=route, minor_route='global', want_psf=True, want_vis=True, **kw)
                assert other['stats']['minor_route'] == 'global' and other['stats']['minor_lds_bytes'] == 64 and same_bits(got, other), (chan_avg, name, route)
            # every status is exercised where the prototype of the definition met it
            if not chan_avg and shape != XC.SHAPES[0]:
                if name == 'A':
                    assert seen == {MAXITER}, seen
                elif name == 'B':
                    assert MAJOR in seen and (shape == XC.SHAPES[1] or DIVERGED in seen), seen
                elif shape == XC.SHAPES[2]:
                    assert {THRESHOLD, MAXITER, DIVERGED} <= seen, seen


def test_g2_a_window_a_non_uniform_grid_and_the_airy_dish(ctx):
    c, shared = base(XC.SHAPES[2])
    window = NP.arange(1000) % 2 == 0                                 # every odd pixel excluded: no component there, every pixel updated
    kw = XC.SETTINGS['B']
    for chan_avg in (False, True):
        pb = XC.problem(c, weights=c['w_bl'], chan_avg=chan_avg, window=window, share=shared)
        got = run(ctx, c, weights=c['w_bl'], chan_avg=chan_avg, window=window, want_vis=True, **kw)
        assert got['stats']['route'] == 'stepped' and NP.all(got['comp_pixel'][got['comp_pixel'] >= 0] % 2 == 0)
        print('window, chan_avg=%d: worst deviation %.2e of its tolerance' % (chan_avg, replayed(pb, c, got, kw)))
        free = run(ctx, c, weights=c['w_bl'], chan_avg=chan_avg, **kw)
        assert NP.any(free['comp_pixel'][free['comp_pixel'] >= 0] % 2 == 1)                  # the window was what kept them away
    u, ushared = base(XC.SHAPES[2], uniform=False)
    pb = XC.problem(u, weights=u['w_full'], share=ushared)
    got = run(ctx, u, weights=u['w_full'], want_vis=True, want_psf=True, **XC.SETTINGS['A'])
    assert got['stats']['route'] == 'direct' and got['stats']['reseed'] == 1              # AUTO on this grid
    print('non-uniform grid: worst deviation %.2e of its tolerance' % replayed(pb, u, got, XC.SETTINGS['A']))
    with pytest.raises(ValueError, match='uniform'):
        run(ctx, u, weights=u['w_full'], route='stepped')
    a, ashared = base(XC.SHAPES[2], beam='airy')
    for chan_avg in (False, True):
        pb = XC.problem(a, beam='airy', weights=a['w_full'], chan_avg=chan_avg, share=ashared)
        assert 0.1 <= float(NP.mean(~pb.valid)) <= 0.9
        got = run(ctx, a, beam='airy', weights=a['w_full'], chan_avg=chan_avg, want_vis=True, want_psf=True, **kw)
        print('airy, chan_avg=%d: worst deviation %.2e of its tolerance' % (chan_avg, replayed(pb, a, got, kw)))


# ---- G3: two sources through a drifting chromatic beam ----------------------------------------------------------------------------------

def test_g3_two_sources_come_back_in_true_flux(ctx):
    c, band = XC.two_sources()
    pb = XC.problem(c, pbmin=0.1, share=band)
    A = pb.A[:, XC.QC.SRC, :]
    assert 0.3 <= A.min() and A.max() <= 0.9
    got = run(ctx, c, pbmin=0.1, want_vis=True, want_psf=True)        # the defaults: gain 0.1, relative 5e-3, depth 0.3, 32 cycles
    assert NP.all(got['status'] == THRESHOLD), got['status']
    used = got['comp_pixel'][got['comp_pixel'] >= 0]
    assert NP.all(NP.isin(used, XC.QC.SRC)), NP.unique(used)
    kw = dict(gain=0.1, maxiter=10000, threshold=5e-3, threshold_relative=True, cycle_depth=0.3, cycle_niter=0, max_major=32)
    dev = replayed(pb, c, got, kw)
    # the replay tolerance of a sum of fluxes at the end of the run: the tolerance of one flux at gain 1, over the final numerator
    spent_q, spent = NP.zeros((3, K + 1)), NP.zeros(K + 1)
    for k in range(K + 1):
        for q, a in zip(got['comp_pixel'][k, :got['ncomp'][k]], got['comp_flux'][k, :got['ncomp'][k]]):
            spent_q[:, k] += abs(a) * pb.A[:, q, k]
            spent[k] += abs(a)
    tol_N, _, _ = pb.tolerances(got['num'], spent_q, spent)
    worst = 0.0
    for k in range(K + 1):
        n = got['ncomp'][k]
        for q, S in zip(XC.QC.SRC, XC.QC.FLUX):
            total = got['comp_flux'][k, :n][got['comp_pixel'][k, :n] == q].sum()
            bound = 1.5 * 5e-3 * got['peak0'][k] + pb.tol_flux(got['num'], tol_N, q, k, 1.0) * got['pb_eff'][q, k]
            worst = max(worst, abs(S - total) * got['pb_eff'][q, k] / (5e-3 * got['peak0'][k]))
            assert abs(S - total) * got['pb_eff'][q, k] <= bound, (k, q, S, total, bound)
    hogbom = ctx.clean_mosaic(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], XC.BEAMS['gaussian'], c['dish'], beam_pc_dircos=c['bpc'],
                              cube=c['cube'], pbmin=0.1)
    assert NP.all(hogbom['status'] == THRESHOLD) and NP.all(NP.abs(got['ncomp'] - hogbom['ncomp']) <= 3), (got['ncomp'], hogbom['ncomp'])
    assert NP.all(10 * got['ncycles'] < got['ncomp']), (got['ncycles'], got['ncomp'])      # fewer major cycles than a tenth of the components
    print('two sources: %d to %d cycles, %d to %d components (Hogbom %d to %d), fluxes to %.3f thresholds, worst deviation %.2e of its tolerance'
          % (got['ncycles'].min(), got['ncycles'].max(), got['ncomp'].min(), got['ncomp'].max(), hogbom['ncomp'].min(), hogbom['ncomp'].max(), worst, dev))
    bandpb = XC.problem(c, chan_avg=True, pbmin=0.1, share=band)
    bandgot = run(ctx, c, pbmin=0.1, chan_avg=True, want_vis=True)
    assert bandgot['status'][0] == THRESHOLD and NP.all(NP.isin(bandgot['comp_pixel'][0, :bandgot['ncomp'][0]], XC.QC.SRC))
    replayed(bandpb, c, bandgot, kw)


# ---- G4: edge cases -------------------------------------------------------------------------------------------------------------------

def test_g4_dead_channels_masked_windows_and_the_horizon(ctx):
    c, shared = base(XC.SHAPES[2])
    kw = XC.SETTINGS['B']
    # a channel without weight: DEAD, NaN, and it delays nobody
    w = c['w_full'].copy()
    w[:, :, 20] = 0.0
    live = NP.arange(K + 1) != 20
    for route in ('direct', 'stepped'):
        got = run(ctx, c, weights=w, route=route, want_vis=True, want_psf=True, **kw)
        assert NP.array_equal(got['status'] == DEAD, ~live) and got['ncomp'][20] == 0 and got['ncycles'][20] == 0 and NP.isnan(got['peak0'][20])
        assert NP.all(NP.isnan(got['residual'][:, 20])) and NP.all(NP.isnan(got['residual_flat'][:, 20])) and got['wsum'][20] == 0.0
        assert NP.all(NP.isnan(got['cycle_peak'][20])) and NP.all(got['cycle_ncomp'][20] == -1) and same(got['vres'][:, :, 20], c['cube'][:, :, 20])
        assert NP.all(got['ncycles'][live] >= 2)
        replayed(XC.problem(c, weights=w, share=shared), c, got, kw)
        bandgot = run(ctx, c, weights=w, route=route, chan_avg=True, want_vis=True, **kw)
        assert NP.any(NP.isfinite(bandgot['residual'])) and bandgot['status'][0] in (MAJOR, DIVERGED)
        replayed(XC.problem(c, weights=w, chan_avg=True, share=shared), c, bandgot, kw)
        for chan_avg in (False, True):
            none = run(ctx, c, weights=NP.zeros_like(w), route=route, chan_avg=chan_avg, fwhm_rad=0.01, **kw)
            assert NP.all(none['status'] == DEAD) and NP.all(none['ncomp'] == 0) and NP.all(NP.isnan(none['residual']))
            assert NP.all(NP.isnan(none['restored'])) and NP.all(NP.isnan(none['peak0'])) and none['stats']['cycles'] == 0
    # a window that holds no valid pixel: THRESHOLD at once, no cycle, a NaN first peak; the mosaic is untouched
    pb = XC.problem(c, weights=c['w_bl'], share=shared)
    window = ~pb.valid.any(axis=1)
    assert window.sum() >= 10
    got = run(ctx, c, weights=c['w_bl'], window=window, want_vis=True, **kw)
    assert NP.all(got['status'] == THRESHOLD) and NP.all(got['ncomp'] == 0) and NP.all(NP.isnan(got['peak0'])) and got['stats']['cycles'] == 0
    assert NP.all(got['ncycles'] == 0) and got['cycle_peak'].shape == (K + 1, 1) and NP.all(NP.isnan(got['cycle_peak'])) and same(got['vres'], c['cube'])
    assert same(got['num'], mosaic(ctx, c, weights=c['w_bl'])[1])
    replayed(XC.problem(c, weights=c['w_bl'], window=window, share=shared), c, got, kw)
    # the last snapshot has everything down (see the module's docstring): no component -- the bits of the call with its weights at 0
    assert NP.all(shared.A[2] == 0.0)
    less = c['w_full'].copy()
    less[2] = 0.0
    for route in ('direct', 'stepped'):
        for chan_avg in (False, True):
            full = run(ctx, c, weights=c['w_full'], route=route, chan_avg=chan_avg, maxiter=0, pbmin=0.0)      # (the mask itself holds Wtot)
            cut = run(ctx, c, weights=less, route=route, chan_avg=chan_avg, maxiter=0, pbmin=0.0)
            assert not same(full['wsum'], cut['wsum'])
            for name in ('num', 'den', 'residual', 'comp_pixel', 'comp_flux', 'ncomp', 'status'):
                assert same(full[name], cut[name]), (name, route, chan_avg)
    # ... with components, each call against its own replay, and other visibilities in that snapshot change nothing at all
    other = c['cube'].copy()
    other[2] = other[2, ::-1] * (0.5 - 2.0j)
    for route in ('direct', 'stepped'):
        full = run(ctx, c, weights=c['w_full'], route=route, want_vis=True, want_psf=True, fwhm_rad=0.02, **kw)
        cut = run(ctx, c, weights=less, route=route, want_vis=True, pbmin=0.25, **kw)      # (at 0.3 a pixel sits on the rim of this mask)
        replayed(XC.problem(c, weights=c['w_full'], share=shared), c, full, kw)
        replayed(XC.problem(c, weights=less, pbmin=0.25, share=shared), c, cut, kw)
        assert same(full['vres'][2], c['cube'][2]) and NP.any(full['vres'][0] != c['cube'][0])
        swapped = run(ctx, c, weights=c['w_full'], route=route, cube=other, want_vis=True, want_psf=True, fwhm_rad=0.02, **kw)
        assert same_bits(full, swapped, [n for n in NAMES if n != 'vres']) and same(swapped['vres'][:2], full['vres'][:2])
        assert same(swapped['vres'][2], other[2])


# ---- G5: bit equality -----------------------------------------------------------------------------------------------------------------

def test_g5_repetition_routes_and_the_resident_cube_leave_the_bits_unchanged(ctx):
    """A relative threshold of 0.3 with seven components a cycle: the channels end after different numbers of cycles, so ended channels
    sit through the major cycles of the others and must come back with the same bits each time."""
    c, _ = base(XC.SHAPES[2])
    for chan_avg in (False, True):
        for route in ('direct', 'stepped'):
            kw = dict(weights=c['w_full'], chan_avg=chan_avg, route=route, gain=0.2, maxiter=60, threshold=0.3, cycle_depth=0.5, cycle_niter=7,
                      max_major=12, fwhm_rad=0.02, want_psf=True, want_vis=True)
            first = run(ctx, c, **kw)
            if not chan_avg:
                assert len(set(first['ncycles'].tolist())) > 1 and NP.any(first['status'] == THRESHOLD)
            assert first['stats']['minor_route'] == 'lds' and same(NP.isnan(first['restored']), NP.isnan(first['residual']))
            assert NP.nanmax(NP.abs(first['restored'] - first['residual'])) > 0.0
            assert same_bits(first, run(ctx, c, **kw)), (chan_avg, route)
            assert same_bits(first, run(ctx, c, minor_route='global', **kw)), (chan_avg, route)
            # num is the mosaic's numerator of the residual visibilities, bit for bit, and so are the quotients
            image, num, den, wsum, st = mosaic(ctx, c, weights=c['w_full'], chan_avg=chan_avg, route=route, cube=first['vres'])
            assert same(num, first['num']) and same(den, first['den']) and same(image, first['residual']) and same(st['pb_eff'], first['pb_eff'])
    kw = dict(weights=c['w_bl'], gain=0.2, maxiter=60, threshold=0.3, cycle_depth=0.5, cycle_niter=7, max_major=12, want_vis=True, want_psf=True)
    host = run(ctx, c, **kw)
    ctx.set_array(c['baselines'], c['freqs'], nt_max=3)
    for t in range(3):
        ctx.set_vis(NP.ascontiguousarray(c['cube'][t]), slot=t)
    res = run(ctx, c, cube=None, **kw)
    assert res['stats']['resident'] is True and host['stats']['resident'] is False and same_bits(host, res) and NP.any(res['vres'] != c['cube'])
    for t in range(3):
        assert NP.array_equal(ctx.get_vis(slot=t), c['cube'][t])      # the resident cube is what it was


# ---- G6: refusals ---------------------------------------------------------------------------------------------------------------------

def test_g6_refusals_write_nothing(ctx):
    c = XC.case((38, K + 1, 9, 7, 1))                                 # 38 baselines: a seeded frame that leaves the lattice up (asserted below)
    odd = XC.case((38, K + 1, 9, 7, 1), uniform=False)
    p, lib, h = _abi._ptr, ctx._lib, ctx._h
    npix, nbl, nchan, maxiter, major = 63, 38, K + 1, 5, 3
    rot = NP.ascontiguousarray(c['rot'].reshape(-1, 9))
    outs = {'out_residual': NP.full((npix, nchan), -7.0), 'out_restored': NP.full((npix, nchan), -7.0), 'out_residual_flat': NP.full((npix, nchan), -7.0),
            'out_pb_eff': NP.full((npix, nchan), -7.0), 'out_num': NP.full((npix, nchan), -7.0), 'out_den': NP.full((npix, nchan), -7.0),
            'out_wsum': NP.full(nchan, -7.0), 'out_comp_pixel': NP.full((nchan, maxiter), -7, dtype=NP.int32),
            'out_comp_flux': NP.full((nchan, maxiter), -7.0), 'out_ncomp': NP.full(nchan, -7, dtype=NP.int32),
            'out_status': NP.full(nchan, -7, dtype=NP.int32), 'out_peak0': NP.full(nchan, -7.0), 'out_ncycles': NP.full(nchan, -7, dtype=NP.int32),
            'out_cycle_ncomp': NP.full((nchan, major), -7, dtype=NP.int32), 'out_cycle_peak': NP.full((nchan, major + 1), -7.0),
            'out_psf': NP.full((nchan, 17, 13), -7.0), 'out_vres': NP.full((1, nbl, nchan), -7.0 + 0j)}
    window = NP.ones(npix, dtype=NP.uint8)
    fwhm = NP.full(nchan, 0.01)
    good_ext = _abi.make_beam_ext({'dipole_dircos': [1.0, 0.0, 0.0]})

    def entry(null=False, without=(), **kw):
        a = ctx.PrisimMoscsArgs()
        v = dict(npix=npix, nbl=nbl, nchan=nchan, nt=1, unitvec=c['unitvec'], rot=rot, aberr_beta=c['beta'], pc_dircos=c['pc'],
                 baselines=c['baselines'], freqs_hz=c['freqs'], cube=c['cube'], weights=c['w_full'], weight_form=2, chan_avg=0, route=-1,
                 beam_kind=_abi.PRISIM_BEAM_GAUSSIAN, diameter_m=6.0, beam_pc_snap=c['bpc'], pbmin=0.3, budget_bytes=0, gain=0.3, maxiter=maxiter,
                 threshold=0.1, threshold_relative=1, window=window, fwhm_rad=fwhm, ny=9, nx=7, cycle_depth=0.5, cycle_niter=2, max_major=major,
                 minor_route=-1)
        v.update(kw)
        keep = []
        for name, val in v.items():
            if isinstance(val, NP.ndarray):
                val = NP.ascontiguousarray(val)
                keep.append(val)
                val = p(val)
            setattr(a, name, val)
        a.beam_pc_dircos[:] = c['bpc'][0].tolist()
        args = [None if name in without else p(arr) for name, arr in outs.items()]
        rc = lib.prisim_clean_mosaic_cs(h, None if null else C.byref(a), *(args + [None]))
        return rc, lib.prisim_hip_last_error(h).decode()

    def changed(x, index, value):
        x = NP.array(x, dtype=NP.float64)
        x[index] = value
        return x

    def untouched():
        return all(NP.all(o == -7) for o in outs.values())

    half = 9 * 13 - 7 + 1
    need = (npix * (64 + 8 * nchan + 16 * nchan + 8 * nchan + 16 * nchan + 1) + 12 * nchan * maxiter + 16 * nchan + 36 * nchan + 8 * 2 * nchan + 24      # prisim_clean_mosaic's
            + 16 * nbl * nchan + 8 * nchan * 17 * 13 + (32 * half + 8 * half * nchan) + (8 * nchan + 8) + (28 * nchan + 4 * nchan * major + 8 * nchan * (major + 1))
            + 8 * npix * nchan)
    ext_of = lambda x: C.cast(C.pointer(x), C.c_void_p)               # noqa: E731
    refusals = [({'null': True}, 'argument struct is NULL'), ({'without': ('out_residual',)}, 'out_residual is NULL'),
                ({'without': ('out_ncomp',)}, 'out_ncomp'), ({'without': ('out_comp_flux',)}, 'out_comp_flux'),
                ({'without': ('out_ncycles',)}, 'out_ncycles'), ({'without': ('out_cycle_ncomp',)}, 'out_cycle_ncomp'),
                ({'without': ('out_cycle_peak',)}, 'out_cycle_peak'),
                # those of prisim_dirty_image
                ({'unitvec': None}, 'unitvec is NULL'), ({'rot': None}, 'rot is NULL'), ({'pc_dircos': None}, 'pc_dircos is NULL'),
                ({'baselines': None}, 'baselines is NULL'), ({'freqs_hz': None}, 'freqs_hz is NULL'), ({'weights': None}, 'weights is NULL'),
                ({'npix': 0}, '>= 1'), ({'nbl': 0}, '>= 1'), ({'nchan': -1}, '>= 1'), ({'nt': 0}, '>= 1'), ({'nchan': (1 << 20) + 1}, '2^20'),
                ({'route': 2}, 'unknown route'), ({'weight_form': 3}, 'unknown weight form'), ({'chan_avg': 2}, 'chan_avg'),
                ({'unitvec': changed(c['unitvec'], (3, 0), 1.5)}, 'unitvec[3]'), ({'rot': changed(rot, (0, 4), 0.5)}, 'rot of snapshot 0'),
                ({'aberr_beta': changed(c['beta'], (0, 1), 0.02)}, 'aberr_beta of snapshot 0'),
                ({'pc_dircos': changed(c['pc'], (0, 2), 1.1)}, 'pc_dircos of snapshot 0'), ({'freqs_hz': changed(c['freqs'], 5, 0.0)}, 'freqs_hz[5]'),
                ({'weights': changed(c['w_full'], (0, 2, 3), -1.0)}, 'finite and non-negative'),
                ({'baselines': changed(c['baselines'], (4, 1), NP.nan)}, 'baseline 4'), ({'freqs_hz': odd['freqs'], 'route': 1}, 'uniform'),
                # those of prisim_mosaic_image: the beam and pbmin
                ({'n_ext': 2, 'ext': ext_of(good_ext)}, 'n_ext must be 0, 1 or nt'), ({'n_ext': 1}, 'ext is NULL'),
                ({'beam_kind': 9}, 'unknown beam_kind'), ({'diameter_m': 0.0}, 'diameter_m must be positive'),
                ({'beam_kind': _abi.PRISIM_BEAM_DIPOLE}, 'PRISIM_BEAM_DIPOLE needs'),
                ({'beam_pc_snap': NP.array([[0.0, NP.nan, 1.0]])}, 'beam_pc_snap of snapshot 0'),
                ({'pbmin': -0.1}, 'pbmin'), ({'pbmin': 1.0}, 'pbmin'), ({'pbmin': NP.nan}, 'pbmin'),
                # those of prisim_clean_image
                ({'gain': 0.0}, 'gain'), ({'gain': 1.5}, 'gain'), ({'gain': NP.nan}, 'gain'), ({'threshold': -1.0}, 'threshold'),
                ({'threshold': NP.inf, 'threshold_relative': 0}, 'threshold'), ({'threshold_relative': 2}, 'threshold_relative'),
                ({'threshold': 1.0}, 'below 1'), ({'window': NP.zeros(npix, dtype=NP.uint8)}, 'window holds no pixel'),
                ({'fwhm_rad': None}, 'needs fwhm_rad'), ({'fwhm_rad': NP.where(NP.arange(nchan) == 3, -1.0, 0.02)}, 'fwhm_rad[3]'),
                ({'maxiter': -1}, 'maxiter'), ({'maxiter': (1 << 30) + 1}, 'maxiter'),
                # those of prisim_clean_image_cs
                ({'ny': 9, 'nx': 8}, 'ny * nx must be npix'), ({'ny': 0, 'nx': 63}, 'ny * nx'), ({'ny': -9, 'nx': -7}, 'ny * nx'),
                ({'cycle_depth': 0.0}, 'cycle_depth'), ({'cycle_depth': 1.0}, 'cycle_depth'), ({'cycle_depth': NP.nan}, 'cycle_depth'),
                ({'max_major': -1}, 'max_major'), ({'max_major': 65537}, 'max_major'), ({'minor_route': 2}, 'minor_route'),
                # its own: a budget one byte short, with the bytes needed
                ({'budget_bytes': need - 1}, 'cannot hold the resident buffers (the resident buffers take %d B' % need)]
    for kw, msg in refusals:
        rc, err = entry(**kw)
        assert rc == _abi.PRISIM_EINVAL and msg in err, (list(kw), rc, err)
        assert untouched(), list(kw)                                  # nothing is written unless the call succeeds
    # a working image that does not fit in the LDS of a workgroup: 144 x 144 pixels of 8 B against 160 KiB; AUTO takes the device memory
    big = XC.case((4, 1, 144, 144, 1))                                # (with 3 baselines the seeded frame puts the whole lattice down)
    with pytest.raises(ValueError, match='does not fit in the LDS'):
        run(ctx, big, minor_route='lds', maxiter=2, max_major=1)
    auto = run(ctx, big, maxiter=2, max_major=1, want_vis=True)
    assert auto['stats']['minor_route'] == 'global' and NP.all(auto['ncomp'] == 2)
    # the resident cube: none at all is a matter of state, one of another shape a wrong argument
    with _abi.Context(0) as fresh:
        with pytest.raises(RuntimeError, match='no resident'):
            run(fresh, c, cube=None)
    ctx.set_array(c['baselines'][:37], c['freqs'], nt_max=1)
    rc, err = entry(cube=None)
    assert rc == _abi.PRISIM_EINVAL and 'resident cube has 1 slots of 37 baselines' in err and untouched()
    # and the budget that just holds the call runs, with the results of the wrapper
    rc, err = entry(budget_bytes=need)
    assert rc == _abi.PRISIM_OK, err
    want = run(ctx, c, weights=c['w_full'], gain=0.3, threshold=0.1, maxiter=maxiter, cycle_depth=0.5, cycle_niter=2, max_major=major, fwhm_rad=fwhm,
               window=window, want_psf=True, want_vis=True)
    assert want['stats']['device_bytes'] == need and NP.all(want['ncomp'] >= 2) and NP.all(want['ncycles'] >= 1)
    for name in ('residual', 'restored', 'residual_flat', 'pb_eff', 'num', 'den', 'wsum', 'ncomp', 'status', 'peak0', 'ncycles', 'psf', 'vres'):
        assert same(outs['out_' + name], want[name]), name
    for k in range(nchan):
        n, m = want['ncomp'][k], want['ncycles'][k]
        assert NP.array_equal(outs['out_comp_pixel'][k, :n], want['comp_pixel'][k, :n]) and NP.all(outs['out_comp_pixel'][k, n:] == -7)
        assert NP.array_equal(outs['out_comp_flux'][k, :n], want['comp_flux'][k, :n]) and NP.all(outs['out_comp_flux'][k, n:] == -7.0)
        assert NP.array_equal(outs['out_cycle_ncomp'][k, :m], want['cycle_ncomp'][k, :m]) and NP.all(outs['out_cycle_ncomp'][k, m:] == -7)
        assert NP.array_equal(outs['out_cycle_peak'][k, :m + 1], want['cycle_peak'][k, :m + 1]) and NP.all(outs['out_cycle_peak'][k, m + 1:] == -7.0)


# ---- G7: through the classes ----------------------------------------------------------------------------------------------------------

def test_g7_a_drift_scan_is_cleaned_to_the_flux_of_the_catalogue():
    """observe() simulates one source through a 14 m Gaussian beam that stays at the zenith while the sky drifts by (the case of
    tests/test_gpu_mosaic.py), imaged on a 3 x 3 lattice of (RA, Dec) around it: clean_mosaic_cotton_schwab() puts its flux into
    components on its pixel, within the bound tests/test_gpu_mosclean.py holds clean_mosaic() to."""
    S, nbl, nt = MC.FLUX, 37, 3
    src = MC.SOURCE_RADEC
    sky = SM.SkyModel(location=src, flux_ref=[S], spindex=[0.0], ref_freq=150e6)
    bl = MC.e2e_baselines(nbl)
    ia = RI.InterferometerArray([(str(i + 1), '0') for i in range(nbl)], bl, MC.CH, telescope=MC.GAUSS14, latitude=MC.LAT, skycoords='radec',
                                pointing_coords='altaz')
    ia.frame_model = 'date'
    for j in range(nt):
        ia.observe((MC.JD0 + j / 64.0, MC.LSTS[j]), {'Tnet': 200.0}, NP.ones(MC.CH.size), MC.ZENITH, sky, 10.7)
    aps = RI.ApertureSynthesis(ia)
    dec, ra = NP.meshgrid(src[0, 1] + NP.array([-2.0, 0.0, 2.0]), src[0, 0] + NP.array([-3.0, 0.0, 3.0]), indexing='ij')
    dirs = NP.stack((ra.ravel(), dec.ravel()), axis=1)                # 3 rows of 3, the source at the centre
    at = 4
    out = aps.clean_mosaic_cotton_schwab(dirs, (3, 3), coords='radec', return_vis=True)
    st = aps.image_stats
    nchan = MC.CH.size
    assert set(out) == {'residual', 'restored', 'residual_flat', 'model', 'components', 'status', 'peak0', 'threshold', 'fwhm', 'cycles', 'residual_vis'}
    assert out['residual'].shape == out['restored'].shape == out['residual_flat'].shape == out['model'].shape == (9, nchan)
    assert out['residual_vis'].shape == (nbl, nchan, nt) and st['route'] == 'stepped' and st['minor_route'] == 'lds'
    assert st['num'].shape == st['den'].shape == st['pb_eff'].shape == (9, nchan) and st['wsum'].shape == (nchan,)
    assert st['terms'] == 9 * nbl * nchan * nt and NP.all(out['status'] == THRESHOLD) and out['cycles']['count'].max() <= 8
    # the replay, from the checker on the very cube observe() left
    uv, rot, beta, pc, _, _ = aps._prepare('dirty', dirs, 'radec', 'noiseless', None, None, 'auto')
    cube = NP.transpose(NP.asarray(ia.skyvis_freq), (2, 0, 1))
    pb = QK.Problem(uv, rot, pc, bl, MC.CH, cube, {'element': 'gaussian', 'size': 14.0}, aberr_beta=beta, pbmin=0.1)
    got = {'comp_pixel': out['components']['pixel'], 'comp_flux': out['components']['flux'], 'ncomp': out['components']['count'],
           'status': out['status'], 'peak0': out['peak0'], 'residual': out['residual'], 'residual_flat': out['residual_flat'],
           'num': st['num'], 'den': st['den'], 'wsum': st['wsum'], 'pb_eff': st['pb_eff'], 'ncycles': out['cycles']['count'],
           'cycle_ncomp': out['cycles']['ncomp'], 'cycle_peak': out['cycles']['peak'], 'vres': NP.transpose(out['residual_vis'], (2, 0, 1))}
    worst = XK.replay(pb, XK.beam(pb, 3, 3), 3, 3, got, 0.1, 10000, 5e-3, True, 0.3, 0, 32)
    _WORST[0] = max(_WORST[0], worst)
    print('drift scan: %d cycles at most, worst deviation %.2e of its tolerance' % (out['cycles']['count'].max(), worst))
    spent_q = NP.abs(out['components']['flux']).sum(axis=1)[NP.newaxis, :] * pb.A[:, at, :]
    tol_N, _, _ = pb.tolerances(st['num'], spent_q, NP.abs(out['components']['flux']).sum(axis=1))
    for k in range(nchan):
        assert NP.all(out['components']['pixel'][k, :out['components']['count'][k]] == at)
        bound = 1.5 * out['threshold'][k] + pb.tol_flux(st['num'], tol_N, at, k, 1.0) * st['pb_eff'][at, k]
        assert abs(S - out['model'][at, k]) * st['pb_eff'][at, k] <= bound, (k, out['model'][at, k], bound)


def test_zz_the_figures_of_this_module():
    """Not a check of the device: prints what the design document quotes of this module's run."""
    print('largest replay deviation of the module: %.3e of its tolerance' % _WORST[0])
    assert _WORST[0] <= 1.0
