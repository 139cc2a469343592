"""GPU: CLEAN of the beam-weighted mosaic on the device (include/prisim_mosclean.h) -- through the C-ABI against prisim_mosaic_image bit
for bit with no iteration, against the replay of the numpy checker (tests/mosclean_checker.py), on two sources seen through a
drifting chromatic beam, on the edge cases of the horizon, the mask and the weights, the bit equality between batch sizes, repeated
calls and the resident cube, the refusals, and through prisim_amd.interferometry.ApertureSynthesis on a drift scan that observe()
simulated.

Bounds: those of the checker, derived in its docstring from the project's 1e-11 of an fp64 image sum and 1e-12 of a device beam value;
the quotients and the mask are asserted exactly from the returned num, den and wsum.  No element is left out of any comparison.

C2 takes the three shapes, three weight forms, chan_avg and both routes of the issue with both dishes.  The mask: pbmin is chosen per
dish so that the reference masks and keeps at least a tenth each (asserted); the shape of one pixel and one channel cannot do both,
there pbmin is 0.01 and the one element is asserted to be kept, away from the rim (its effective beam is 0.019 and 0.21)."""
import ctypes as C
import os
import sys

import numpy as NP
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import imaging_cases as IC  # noqa: E402
import mosaic_cases as MC  # noqa: E402
import mosaic_checker as MK  # noqa: E402
import mosclean_cases as QC  # noqa: E402
import mosclean_checker as QK  # noqa: E402

from prisim_amd import _abi, skymodel as SM  # noqa: E402
from prisim_amd import interferometry as RI  # noqa: E402

pytestmark = pytest.mark.gpu
K = QC.K
THRESHOLD, MAXITER, DEAD = _abi.PRISIM_IMCLEAN_THRESHOLD, _abi.PRISIM_IMCLEAN_MAXITER, _abi.PRISIM_IMCLEAN_DEAD
PBMIN = {'gaussian': 0.03, 'airy': 0.1}          # of the 2 m dishes over the upper hemisphere: masks and keeps at least a tenth each
_MEMO = {}
_WORST = [0.0]


def base(shape, beam, uniform=True):
    """The seeded inputs of a shape and the phasors and beams of the checker, made once for the module"""
    key = (shape, beam, uniform)
    if key not in _MEMO:
        c = QC.parity_case(shape, uniform=uniform)
        _MEMO[key] = (c, QC.problem(c, beam, pbmin=PBMIN[beam]))
    return _MEMO[key]


def run(ctx, c, beam, weights=None, **kw):
    return ctx.clean_mosaic(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], QC.BEAMS[beam], c.get('dish', QC.DISH),
                            beam_pc_dircos=kw.pop('bpc', c['bpc']), cube=kw.pop('cube', c['cube']), weights=weights, aberr_beta=c['beta'], **kw)


def mosaic(ctx, c, beam, weights=None, **kw):
    return ctx.mosaic_image(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], QC.BEAMS[beam], c.get('dish', QC.DISH),
                            beam_pc_dircos=c['bpc'], cube=c['cube'], weights=weights, aberr_beta=c['beta'], **kw)


def same(a, b):
    return NP.array_equal(a, b, equal_nan=True)


NAMES = ('residual', 'residual_flat', 'pb_eff', 'num', 'den', 'wsum', 'comp_pixel', 'comp_flux', 'ncomp', 'status', 'peak0')


def same_bits(a, b):
    return all(same(a[n], b[n]) for n in NAMES) and (a['restored'] is None) == (b['restored'] is None) and \
        (a['restored'] is None or same(a['restored'], b['restored']))


def replayed(pb, got, *args):
    worst = QK.replay(pb, got, *args)
    _WORST[0] = max(_WORST[0], worst)
    return worst


# ---- C1: no iteration is a mosaic -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('form', QC.FORMS)
def test_c1_no_iterations_leave_the_mosaic_bit_for_bit(ctx, form):
    c, _ = base(QC.SHAPES[2], 'airy')
    w = QC.weights_of(c, form)
    for chan_avg in (False, True):
        for route in ('direct', 'stepped'):
            want, num, den, wsum, st = mosaic(ctx, c, 'airy', weights=w, chan_avg=chan_avg, route=route, pbmin=0.1)
            got = run(ctx, c, 'airy', weights=w, chan_avg=chan_avg, route=route, pbmin=0.1, maxiter=0, threshold=0.0, threshold_relative=False)
            nc = 1 if chan_avg else K + 1
            for name, ref in (('num', num), ('den', den), ('wsum', wsum), ('pb_eff', st['pb_eff']), ('residual', want)):
                assert got[name].shape == ref.shape and same(got[name], ref), (name, form, chan_avg, route)
            assert NP.any(NP.isnan(want)) and NP.any(NP.isfinite(want)) and got['restored'] is None
            assert got['comp_pixel'].shape == (nc, 0) and NP.all(got['ncomp'] == 0) and NP.all(got['status'] == MAXITER)
            assert same(got['residual_flat'], QK.flat_of(num, den, wsum, 0.1, chan_avg))
            assert NP.array_equal(got['peak0'], NP.nanmax(NP.abs(got['residual_flat']).reshape(1000, nc), axis=0))
            gs = got['stats']
            assert gs['route'] == route and gs['iterations'] == 0 and gs['components'] == 0 and gs['polls'] == 1 and gs['resident'] is False
            assert gs['terms'] == 1000 * 37 * (K + 1) * 3 and gs['beam_values'] == 1000 * (K + 1) * 3 and gs['chan_tile'] == K
            assert gs['block_pixels'] == 256 and gs['lds_bytes'] == 17792 + 8 * K and gs['reseed'] == (K if route == 'stepped' else 1)


# ---- C2: replay parity ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('beam', ['gaussian', 'airy'])
@pytest.mark.parametrize('form', QC.FORMS)
@pytest.mark.parametrize('shape', QC.SHAPES, ids=lambda s: 'x'.join(str(v) for v in s))
def test_c2_replay_parity(ctx, shape, form, beam):
    c, shared = base(shape, beam)
    nbl, nchan, npix, nt = shape
    w = QC.weights_of(c, form)
    if nbl >= 7:
        assert NP.count_nonzero(NP.asarray(c['w_bl']) == 0.0) == nbl // 7
    assert c['bpc'].shape == (nt, 3) and (nt == 1 or not NP.array_equal(c['bpc'][0], c['bpc'][1]))      # a pointing that moves
    window = NP.arange(npix) % 2 == 0
    pbmin = PBMIN[beam] if npix > 1 else 0.01
    for chan_avg in (False, True):
        pb = QC.problem(c, beam, weights=w, chan_avg=chan_avg, window=window, pbmin=pbmin, share=shared)
        if npix > 1:
            QC.assert_mask_keeps_and_cuts(pb)
        else:
            assert NP.all(pb.valid)
        for route in ('direct', 'stepped'):
            got = run(ctx, c, beam, weights=w, chan_avg=chan_avg, route=route, pbmin=pbmin, gain=0.3, maxiter=25, threshold=0.0,
                      threshold_relative=False, window=window)
            assert got['stats']['route'] == route and got['residual'].dtype == NP.float64
            worst = replayed(pb, got, 0.3, 25, 0.0, False)
            print('%s %s weights=%s chan_avg=%d %s: %d components, worst deviation %.2e of its tolerance'
                  % (shape, beam, form, chan_avg, route, int(got['ncomp'].sum()), worst))
            assert NP.all(got['comp_pixel'][got['comp_pixel'] >= 0] % 2 == 0)
            # with a threshold of 0 nothing stops early but a search image that is exactly 0
            assert NP.all((got['status'] == MAXITER) | (got['ncomp'] < 25))
            assert got['stats']['components'] == int(got['ncomp'].sum()) and got['stats']['iterations'] == int(got['ncomp'].max())


def test_c2_non_uniform_grid_is_direct(ctx):
    c, shared = base(QC.SHAPES[2], 'airy', uniform=False)
    window = NP.arange(1000) % 2 == 0
    pb = QC.problem(c, 'airy', weights=c['w_full'], window=window, pbmin=0.1, share=shared)
    kw = dict(weights=c['w_full'], pbmin=0.1, gain=0.3, maxiter=25, threshold=0.0, threshold_relative=False, window=window)
    got = run(ctx, c, 'airy', **kw)
    assert got['stats']['route'] == 'direct' and got['stats']['reseed'] == 1          # AUTO on this grid
    print('non-uniform grid: worst deviation %.2e of its tolerance' % replayed(pb, got, 0.3, 25, 0.0, False))
    with pytest.raises(ValueError, match='uniform'):
        run(ctx, c, 'airy', route='stepped', **kw)
    free = run(ctx, c, 'airy', **dict(kw, window=None))
    assert NP.any(free['comp_pixel'] % 2 == 1)                        # the window was what kept them away


# ---- C3: two sources through a drifting chromatic beam ----------------------------------------------------------------------------------

def test_c3_two_sources_come_back_in_true_flux(ctx):
    c, band = QC.two_sources()
    pb = QC.problem(c, 'gaussian', pbmin=0.1, share=band)
    A = pb.A[:, QC.SRC, :]
    assert 0.3 <= A.min() and A.max() <= 0.9
    worst = 0.0
    for k in (0, K):
        for q in QC.SRC:
            norm = QK.response(pb, int(q), k)[2][:, k].copy()
            norm[q] = 0.0
            worst = max(worst, float(NP.max(norm)))
    print('worst normalised off-pixel response at the band edges: %.3f' % worst)
    assert worst < 1.0 / 3.0
    got = run(ctx, c, 'gaussian', pbmin=0.1)                          # the defaults: gain 0.1, relative 5e-3
    assert NP.all(got['status'] == THRESHOLD), got['status']
    used = got['comp_pixel'][got['comp_pixel'] >= 0]
    assert NP.all(NP.isin(used, QC.SRC)), NP.unique(used)
    dev = replayed(pb, got, 0.1, 10000, 5e-3, True)
    print('two sources: %d iterations, %d components, worst deviation %.2e of its tolerance'
          % (got['stats']['iterations'], got['stats']['components'], dev))
    # the replay tolerance of a sum of fluxes at the end of the run: the tolerance of one flux at gain 1, over the final numerator
    spent_q = NP.zeros((3, K + 1))
    spent = NP.zeros(K + 1)
    for k in range(K + 1):
        for q, a in zip(got['comp_pixel'][k, :got['ncomp'][k]], got['comp_flux'][k, :got['ncomp'][k]]):
            spent_q[:, k] += abs(a) * pb.A[:, q, k]
            spent[k] += abs(a)
    tol_N, _, _ = pb.tolerances(got['num'], spent_q, spent)
    image = ctx.clean_image(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], cube=c['cube'])
    assert NP.all(image['status'] == THRESHOLD)
    for k in range(K + 1):
        n, m = got['ncomp'][k], image['ncomp'][k]
        for q, S in zip(QC.SRC, QC.FLUX):
            total = got['comp_flux'][k, :n][got['comp_pixel'][k, :n] == q].sum()
            bound = 1.5 * 5e-3 * got['peak0'][k] + pb.tol_flux(got['num'], tol_N, q, k, 1.0) * got['pb_eff'][q, k]
            assert abs(S - total) * got['pb_eff'][q, k] <= bound, (k, q, S, total, bound)
            # what the feature adds: CLEAN of the dirty image returns the apparent flux, off by far more than that
            apparent = image['comp_flux'][k, :m][image['comp_pixel'][k, :m] == q].sum()
            assert abs(S - apparent) * got['pb_eff'][q, k] > 10 * bound, (k, q, S, apparent, bound)


# ---- C4: edge cases -------------------------------------------------------------------------------------------------------------------

def test_c4_dead_channels_masked_windows_and_the_horizon(ctx):
    c, shared = base(QC.SHAPES[2], 'airy')
    kw = dict(pbmin=0.1, gain=0.3, maxiter=25, threshold=0.0, threshold_relative=False)
    # a channel without weight: DEAD, NaN, and it delays nobody
    w = c['w_full'].copy()
    w[:, :, 20] = 0.0
    live = NP.arange(K + 1) != 20
    for route in ('direct', 'stepped'):
        got = run(ctx, c, 'airy', weights=w, route=route, **kw)
        assert NP.array_equal(got['status'] == DEAD, ~live) and got['ncomp'][20] == 0 and NP.isnan(got['peak0'][20])
        assert NP.all(NP.isnan(got['residual'][:, 20])) and NP.all(NP.isnan(got['residual_flat'][:, 20])) and got['wsum'][20] == 0.0
        assert NP.all(got['ncomp'][live] == 25) and got['stats']['iterations'] == 25
        replayed(QC.problem(c, 'airy', weights=w, pbmin=0.1, share=shared), got, 0.3, 25, 0.0, False)
        bandgot = run(ctx, c, 'airy', weights=w, route=route, chan_avg=True, **kw)
        assert bandgot['status'][0] == MAXITER
        replayed(QC.problem(c, 'airy', weights=w, chan_avg=True, pbmin=0.1, share=shared), bandgot, 0.3, 25, 0.0, False)
        for chan_avg in (False, True):
            none = run(ctx, c, 'airy', weights=NP.zeros_like(w), route=route, chan_avg=chan_avg, fwhm_rad=0.01, **kw)
            assert NP.all(none['status'] == DEAD) and NP.all(none['ncomp'] == 0) and NP.all(NP.isnan(none['residual']))
            assert NP.all(NP.isnan(none['restored'])) and NP.all(NP.isnan(none['peak0'])) and none['stats']['iterations'] == 0
    # a window that is wholly masked: THRESHOLD at once, no component, a NaN first peak; the mosaic is untouched
    pb = QC.problem(c, 'airy', weights=c['w_bl'], pbmin=0.1, share=shared)
    window = ~pb.valid.any(axis=1)
    assert window.sum() >= 10
    got = run(ctx, c, 'airy', weights=c['w_bl'], window=window, **kw)
    assert NP.all(got['status'] == THRESHOLD) and NP.all(got['ncomp'] == 0) and NP.all(NP.isnan(got['peak0'])) and got['stats']['iterations'] == 0
    assert same(got['num'], mosaic(ctx, c, 'airy', weights=c['w_bl'], pbmin=0.1)[1])
    replayed(QC.problem(c, 'airy', weights=c['w_bl'], window=window, pbmin=0.1, share=shared), got, 0.3, 25, 0.0, False)
    # a snapshot in which everything is down adds exactly what zero weights add
    f = MC.up_case(37, K + 1, 65, 3, flip=(1,))
    f['bpc'] = QC.pointings(3)
    less = f['w_full'].copy()
    less[1] = 0.0
    for route in ('direct', 'stepped'):
        full = run(ctx, f, 'airy', weights=f['w_full'], route=route, **dict(kw, pbmin=0.0))
        cut = run(ctx, f, 'airy', weights=less, route=route, **dict(kw, pbmin=0.0))
        assert NP.all(full['ncomp'] == 25) and not same(full['wsum'], cut['wsum'])
        for name in ('num', 'den', 'residual', 'comp_pixel', 'comp_flux', 'ncomp', 'status'):
            assert same(full[name], cut[name]), (name, route)
    # a component whose pixel sets between snapshots: the frame of snapshot 1 is tilted about East by a right angle, so that the
    # northern half of the sky is below the horizon there and up in snapshots 0 and 2
    s = MC.up_case(37, K + 1, 65, 3, down=20)
    s['bpc'] = QC.pointings(3)
    tilt = NP.array([[1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, -1.0, 0.0]])              # about East by 90 degrees: North goes down
    s['rot'] = NP.stack([s['rot'][0], tilt.dot(s['rot'][1]), s['rot'][2]])
    pbs = QC.problem(s, 'airy', weights=s['w_bl'], pbmin=0.0)
    up = pbs.A[:, :, 0] > 0.0
    sets = up[0] & ~up[1]
    assert sets.sum() >= 5 and (up[0] & up[1]).sum() >= 5
    for route in ('direct', 'stepped'):
        got = run(ctx, s, 'airy', weights=s['w_bl'], route=route, **dict(kw, pbmin=0.0))
        replayed(pbs, got, 0.3, 25, 0.0, False)
        assert NP.any(sets[got['comp_pixel'][got['comp_pixel'] >= 0]])                  # components were put on pixels that set


# ---- C5: bit equality -----------------------------------------------------------------------------------------------------------------

def test_c5_polling_repetition_and_the_resident_cube_leave_the_bits_unchanged(ctx):
    """A relative threshold of a half: the channels end after different numbers of iterations, so ended channels sit through the
    updates of the others, and batches of 1, 7 and 32 iterations end at different places."""
    c, _ = base(QC.SHAPES[2], 'airy')
    for chan_avg in (False, True):
        for route in ('direct', 'stepped'):
            kw = dict(weights=c['w_full'], chan_avg=chan_avg, route=route, pbmin=0.1, gain=0.3, maxiter=25, threshold=0.5, fwhm_rad=0.02)
            first = run(ctx, c, 'airy', **kw)
            if not chan_avg:
                assert len(set(first['ncomp'].tolist())) > 2 and NP.any(first['status'] == THRESHOLD)
            assert first['stats']['polls'] == 1 and same(NP.isnan(first['restored']), NP.isnan(first['residual']))
            for poll in (1, 7, 32):
                again = run(ctx, c, 'airy', poll_every=poll, **kw)
                assert same_bits(first, again), (chan_avg, route, poll)
                assert again['stats']['polls'] == -(-(again['stats']['iterations'] + 1) // poll)
            assert same_bits(first, run(ctx, c, 'airy', **kw))
    kw = dict(weights=c['w_bl'], pbmin=0.1, gain=0.3, maxiter=25, threshold=0.5)
    host = run(ctx, c, 'airy', **kw)
    ctx.set_array(c['baselines'], c['freqs'], nt_max=3)
    for t in range(3):
        ctx.set_vis(NP.ascontiguousarray(c['cube'][t]), slot=t)
    res = run(ctx, c, 'airy', cube=None, **kw)
    assert res['stats']['resident'] is True and host['stats']['resident'] is False and same_bits(host, res)


# ---- C6: refusals ---------------------------------------------------------------------------------------------------------------------

def test_c6_refusals_write_nothing(ctx):
    c = IC.case(37, K + 1, 65, 3)
    odd = IC.case(37, K + 1, 65, 3, uniform=False)
    p, lib, h = _abi._ptr, ctx._lib, ctx._h
    rot = NP.ascontiguousarray(c['rot'].reshape(-1, 9))
    nchan, maxiter = K + 1, 4
    outs = {'out_residual': NP.full((65, nchan), -7.0), 'out_restored': NP.full((65, nchan), -7.0), 'out_residual_flat': NP.full((65, nchan), -7.0),
            'out_pb_eff': NP.full((65, nchan), -7.0), 'out_num': NP.full((65, nchan), -7.0), 'out_den': NP.full((65, nchan), -7.0),
            'out_wsum': NP.full(nchan, -7.0), 'out_comp_pixel': NP.full((nchan, maxiter), -7, dtype=NP.int32),
            'out_comp_flux': NP.full((nchan, maxiter), -7.0), 'out_ncomp': NP.full(nchan, -7, dtype=NP.int32),
            'out_status': NP.full(nchan, -7, dtype=NP.int32), 'out_peak0': NP.full(nchan, -7.0)}
    fwhm = NP.full(nchan, 0.02)
    window = NP.ones(65, dtype=NP.uint8)
    good_ext = _abi.make_beam_ext({'dipole_dircos': [1.0, 0.0, 0.0]})

    def entry(null=False, without=(), **kw):
        a = ctx.PrisimMoscleanArgs()
        v = dict(npix=65, nbl=37, nchan=nchan, nt=3, unitvec=c['unitvec'], rot=rot, aberr_beta=c['beta'], pc_dircos=c['pc'],
                 baselines=c['baselines'], freqs_hz=c['freqs'], cube=c['cube'], weights=c['w_full'], weight_form=2, chan_avg=0, route=-1,
                 beam_kind=_abi.PRISIM_BEAM_AIRY, diameter_m=2.0, pbmin=0.1, budget_bytes=0, gain=0.3, maxiter=maxiter, threshold=0.0,
                 threshold_relative=0, window=window, fwhm_rad=fwhm, poll_every=0)
        v.update(kw)
        keep = []
        for name, val in v.items():
            if isinstance(val, NP.ndarray):
                val = NP.ascontiguousarray(val)
                keep.append(val)
                val = p(val)
            setattr(a, name, val)
        a.beam_pc_dircos[:] = [0.0, 0.0, 1.0]
        args = [None if name in without else p(arr) for name, arr in outs.items()]
        rc = lib.prisim_clean_mosaic(h, None if null else C.byref(a), *(args + [None]))
        return rc, lib.prisim_hip_last_error(h).decode()

    def changed(name, index, value):
        x = NP.array(rot if name == 'rot' else c[name], dtype=NP.float64)
        x[index] = value
        return x

    need = 65 * (64 * 3 + 8 * 3 * nchan + 16 * nchan + 8 * nchan + 16 * nchan + 1) + 12 * nchan * maxiter + 16 * nchan + 36 * nchan + 8 * 4 * nchan + 24
    ext_of = lambda x: C.cast(C.pointer(x), C.c_void_p)               # noqa: E731
    refusals = [({'null': True}, 'argument struct is NULL'), ({'without': ('out_residual',)}, 'out_residual is NULL'),
                ({'without': ('out_ncomp',)}, 'out_ncomp'), ({'without': ('out_comp_flux',)}, 'out_comp_flux'),
                # those of prisim_dirty_image
                ({'unitvec': None}, 'unitvec is NULL'), ({'rot': None}, 'rot is NULL'), ({'pc_dircos': None}, 'pc_dircos is NULL'),
                ({'baselines': None}, 'baselines is NULL'), ({'freqs_hz': None}, 'freqs_hz is NULL'), ({'weights': None}, 'weights is NULL'),
                ({'npix': 0}, '>= 1'), ({'nbl': 0}, '>= 1'), ({'nchan': -1}, '>= 1'), ({'nt': 0}, '>= 1'), ({'nchan': (1 << 20) + 1}, '2^20'),
                ({'route': 2}, 'unknown route'), ({'weight_form': 3}, 'unknown weight form'), ({'chan_avg': 2}, 'chan_avg'),
                ({'unitvec': changed('unitvec', (3, 0), 1.5)}, 'unitvec[3]'), ({'rot': changed('rot', (1, 4), 0.5)}, 'rot of snapshot 1'),
                ({'aberr_beta': changed('beta', (2, 1), 0.02)}, 'aberr_beta of snapshot 2'),
                ({'pc_dircos': changed('pc', (0, 2), 1.1)}, 'pc_dircos of snapshot 0'), ({'freqs_hz': changed('freqs', 5, 0.0)}, 'freqs_hz[5]'),
                ({'weights': changed('w_full', (1, 2, 3), -1.0)}, 'finite and non-negative'),
                ({'baselines': changed('baselines', (4, 1), NP.nan)}, 'baseline 4'), ({'freqs_hz': odd['freqs'], 'route': 1}, 'uniform'),
                # those of prisim_mosaic_image: the beam and pbmin
                ({'n_ext': 2, 'ext': ext_of(good_ext)}, 'n_ext must be 0, 1 or nt'), ({'n_ext': 1}, 'ext is NULL'),
                ({'beam_kind': 9}, 'unknown beam_kind'), ({'diameter_m': 0.0}, 'diameter_m must be positive'),
                ({'beam_kind': _abi.PRISIM_BEAM_DIPOLE}, 'PRISIM_BEAM_DIPOLE needs'),
                ({'beam_pc_snap': NP.array([[0.0, 0.0, 1.0], [0.0, NP.nan, 1.0], [0.0, 0.0, 1.0]])}, 'beam_pc_snap of snapshot 1'),
                ({'pbmin': -0.1}, 'pbmin'), ({'pbmin': 1.0}, 'pbmin'), ({'pbmin': NP.nan}, 'pbmin'),
                # those of prisim_clean_image
                ({'gain': 0.0}, 'gain'), ({'gain': 1.5}, 'gain'), ({'gain': NP.nan}, 'gain'), ({'threshold': -1.0}, 'threshold'),
                ({'threshold': NP.inf}, 'threshold'), ({'threshold_relative': 2}, 'threshold_relative'),
                ({'threshold': 1.0, 'threshold_relative': 1}, 'below 1'), ({'window': NP.zeros(65, dtype=NP.uint8)}, 'window holds no pixel'),
                ({'fwhm_rad': None}, 'needs fwhm_rad'), ({'fwhm_rad': NP.where(NP.arange(nchan) == 3, -1.0, 0.02)}, 'fwhm_rad[3]'),
                ({'maxiter': -1}, 'maxiter'), ({'maxiter': (1 << 30) + 1}, 'maxiter'),
                # its own: a budget one byte short, with the bytes needed
                ({'budget_bytes': need - 1}, 'cannot hold the whole image (the resident buffers take %d B' % need)]
    for kw, msg in refusals:
        rc, err = entry(**kw)
        assert rc == _abi.PRISIM_EINVAL and msg in err, (list(kw), rc, err)
        assert all(NP.all(o == -7) for o in outs.values()), list(kw)  # nothing is written unless the call succeeds
    c['bpc'] = NP.array([0.0, 0.0, 1.0])
    with _abi.Context(0) as fresh:
        with pytest.raises(RuntimeError, match='no resident'):
            run(fresh, c, 'airy', cube=None)                          # PRISIM_ESTATE: no array was ever set
    rc, err = entry(budget_bytes=need)
    assert rc == _abi.PRISIM_OK, err
    want = run(ctx, c, 'airy', weights=c['w_full'], pbmin=0.1, gain=0.3, maxiter=maxiter, threshold=0.0, threshold_relative=False,
               window=window, fwhm_rad=fwhm)
    for name in ('residual', 'restored', 'residual_flat', 'pb_eff', 'num', 'den', 'wsum', 'ncomp', 'status', 'peak0'):
        assert same(outs['out_' + name], want[name]), name
    assert same(outs['out_comp_pixel'], want['comp_pixel']) and same(outs['out_comp_flux'], want['comp_flux']) and NP.all(want['ncomp'] == maxiter)
    assert want['stats']['device_bytes'] == need


# ---- C7: through the classes ----------------------------------------------------------------------------------------------------------

def test_c7_a_drift_scan_is_cleaned_to_the_flux_of_the_catalogue():
    """observe() simulates one source through a 14 m Gaussian beam that stays at the zenith while the sky drifts by (the case of
    tests/test_gpu_mosaic.py): clean_mosaic() puts its flux into components on its pixel, clean() the apparent flux."""
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
    others = NP.stack((src[0, 0] + NP.linspace(-3.0, 3.0, 8), src[0, 1] + NP.linspace(2.0, -2.0, 8)), axis=1)
    dirs = NP.vstack((src, others))
    out = aps.clean_mosaic(dirs, coords='radec')
    st = aps.image_stats
    nchan = MC.CH.size
    assert out['residual'].shape == out['restored'].shape == out['residual_flat'].shape == out['model'].shape == (9, nchan)
    assert st['route'] == 'stepped' and st['num'].shape == st['den'].shape == st['pb_eff'].shape == (9, nchan) and st['wsum'].shape == (nchan,)
    assert st['terms'] == 9 * nbl * nchan * nt and NP.all(out['status'] == THRESHOLD)
    assert same(out['residual'], MK.quotient(st['num'], st['den'], st['wsum'], 0.1)[0])
    # the replay, from the checker on the very cube observe() left
    uv, rot, beta, pc, _, _ = aps._prepare('dirty', dirs, 'radec', 'noiseless', None, None, 'auto')
    cube = NP.transpose(NP.asarray(ia.skyvis_freq), (2, 0, 1))
    pb = QK.Problem(uv, rot, pc, bl, MC.CH, cube, {'element': 'gaussian', 'size': 14.0}, aberr_beta=beta, pbmin=0.1)
    got = {'comp_pixel': out['components']['pixel'], 'comp_flux': out['components']['flux'], 'ncomp': out['components']['count'],
           'status': out['status'], 'peak0': out['peak0'], 'residual': out['residual'], 'residual_flat': out['residual_flat'],
           'num': st['num'], 'den': st['den'], 'wsum': st['wsum'], 'pb_eff': st['pb_eff']}
    print('drift scan: worst deviation %.2e of its tolerance' % replayed(pb, got, 0.1, 10000, 5e-3, True))
    image = aps.clean(dirs, coords='radec')
    spent_q = NP.abs(out['components']['flux']).sum(axis=1)[NP.newaxis, :] * pb.A[:, 0, :]
    tol_N, _, _ = pb.tolerances(st['num'], spent_q, NP.abs(out['components']['flux']).sum(axis=1))
    for k in range(nchan):
        assert NP.all(out['components']['pixel'][k, :out['components']['count'][k]] == 0)
        bound = 1.5 * out['threshold'][k] + pb.tol_flux(st['num'], tol_N, 0, k, 1.0) * st['pb_eff'][0, k]
        assert abs(S - out['model'][0, k]) * st['pb_eff'][0, k] <= bound, (k, out['model'][0, k], bound)
        assert abs(S - image['model'][0, k]) * st['pb_eff'][0, k] > 10 * bound, (k, image['model'][0, k])      # the apparent flux


def test_zz_the_figures_of_this_module():
    """Not a check of the device: prints what the design document quotes of this module's run."""
    print('largest replay deviation of the module: %.3e of its tolerance' % _WORST[0])
    assert _WORST[0] <= 1.0
