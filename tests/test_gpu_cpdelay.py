"""GPU: delay spectra of closure phases and their power spectra (include/prisim_cpdelay.h), through the C-ABI and through
DelaySpectrum.subband_delay_transform_closure_phase / DelayPowerSpectrum.compute_*_closure_phase_power_spectrum, against
tests/golden/golden_cpdelay.npz (the reference's statements executed) and the numpy checker (tests/cpdelay_checker.py).

Bounds.  Spectra: 1e-12, the package's bound for its two FFT routes (tests/test_gpu_subband.py, tests/test_gpu_closure.py),
of df * sum_ch wts[w][ch] -- the largest value a spectrum of unit phasors can take; a row maximum would reward rows that happen to
cancel.  Phases formed on the device may differ from the reference's by 32 u on the unit circle (tests/test_gpu_closure.py derives it),
which moves a spectrum by at most 32 u of the same scale: the same bound covers it.  Power: individual within 4 u relative (one |x|^2,
one product) of the exact value, which tests/cpdelay_checker.py forms in extended precision -- numpy's own abs(x)**2 * scale, a squared
hypot, is itself up to ~4 u from it, so a comparison of two rounded values could not hold a 4 u bound; auto within (n0 + 8) u scale[w] (sum over axis 0 of |x|)^2 / n0 and cross within the same / (n0 (n0 - 1)) (recursive
summation of n0 terms, Higham's gamma_n, plus the products); cross subtracts nearly equal numbers, so it is judged against that scale."""
import json
import os
import sys
import warnings

import numpy as NP
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cpdelay_checker as CC  # noqa: E402

from prisim_amd import _abi, layouts as LAY, skymodel as SM, workloads as W  # noqa: E402
from prisim_amd import delay_spectrum as DS, interferometry as RI  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = NP.load(os.path.join(HERE, 'golden', 'golden_cpdelay.npz'))
GOLD_CLOSURE = NP.load(os.path.join(HERE, 'golden', 'golden_closure.npz'))
pytestmark = pytest.mark.gpu
KEYS = ('closure_phase_skyvis', 'closure_phase_vis', 'closure_phase_noise')
BOUND = 1e-12
U = 2.0 ** -53


def _check(got, want, wts, df, what):
    assert got.shape == want.shape and NP.all(NP.isfinite(got.view(NP.float64))), what
    err = CC.spectrum_error(got, want, wts, df)
    print(what, 'error %.3e of df sum wts (bound %.1e)' % (err, BOUND))
    assert err <= BOUND, (what, err)


@pytest.mark.parametrize('i', [0, 1, 2])
def test_spectra_from_given_phases_against_the_reference(ctx, i):
    pre = 'c%d_' % i
    p = json.loads(str(GOLD[pre + 'params']))
    wts = GOLD[pre + 'o_freq_wts']
    m = GOLD[pre + 'o_lags'].size
    nres = GOLD[pre + 'r_closure_phase_skyvis'].shape[-2]
    pow2 = m & (m - 1) == 0
    for route in (('auto', 'fused', 'rocfft') if pow2 else ('auto', 'rocfft')):
        for key in KEYS:
            out = ctx.closure_delay_spectra(wts, m, p['df'], phases=GOLD[pre + 'in_' + key], nres=nres, want=('over', 'res'), route=route)
            assert out['stats']['route'] == ('rocfft' if route == 'rocfft' or not pow2 else 'fused') and out['stats']['phase_route'] is None
            _check(out['over'], GOLD[pre + 'o_' + key], wts, p['df'], '%s %s over %s' % (pre, route, key))
            _check(out['res'], GOLD[pre + 'r_' + key], wts, p['df'], '%s %s res %s' % (pre, route, key))
    if not pow2:
        with pytest.raises(ValueError, match='power-of-two'):
            ctx.closure_delay_spectra(wts, m, p['df'], phases=GOLD[pre + 'in_' + KEYS[0]], want=('over',), route='fused')


def _windows(rng, nwin, nchan):
    wts = NP.zeros((nwin, nchan))
    for w in range(nwin):
        lo = int(rng.integers(0, max(1, nchan // 2)))
        hi = int(rng.integers(lo + 1, nchan + 1))
        wts[w, lo:hi] = rng.uniform(0.2, 1.5, hi - lo)
    return wts


@pytest.mark.parametrize('nchan,m,nt,nrows', [(2048, 4096, 1, 3), (3000, 4096, 3, 2), (70, 128, 37, 5), (70, 100, 37, 5), (1, 1, 2, 2),
                                                (2, 2, 3, 3), (5, 8, 65, 3), (7, 12, 5, 5)])
def test_long_rows_odd_tiles_and_streaming(ctx, nchan, m, nt, nrows):
    """m = 4096 (98320 B of LDS, above the 64 KiB a kernel gets without asking), nt = 1, an nt that is no multiple of the tile, and
    budgets that force several chunks with a partial last one: every budget gives the one-chunk output, bit for bit."""
    rng = NP.random.default_rng(nchan + m)
    df, nwin = 1e5, 2
    ph = rng.uniform(-NP.pi, NP.pi, (nrows, nchan, nt))
    wts = _windows(rng, nwin, nchan)
    nres = max(1, m // 7)
    ps = rng.uniform(0.5, 2.0, nwin)
    want_o, want_r = CC.delay_spectra(ph, wts, m, df, nres)
    pow2 = m & (m - 1) == 0
    want = ('over', 'over_power', 'res', 'res_power')
    for route in (('fused', 'rocfft') if pow2 else ('rocfft',)):
        first = None
        per_row = nchan * nt * 8 + nwin * nt * (m * (24 + (0 if route == 'fused' else 16)) + nres * 24)
        for budget in (_abi.CLOSURE_BUDGET, 2 * 2 * per_row):
            out = ctx.closure_delay_spectra(wts, m, df, phases=ph, nres=nres, pscale=ps, want=want, route=route, budget_bytes=budget)
            st = out['stats']
            assert st['route'] == route
            if budget != _abi.CLOSURE_BUDGET:
                assert st['chunk_rows'] == 2 and st['chunks'] == (nrows + 1) // 2 and st['streams'] == min(2, st['chunks'])
            if route == 'fused' and m == 4096:
                assert st['tile'] == 1 and st['lds_bytes'] == 16 * (m + 1) + 8 * m > 65536
            _check(out['over'], want_o, wts, df, 'm %d %s over' % (m, route))
            _check(out['res'], want_r, wts, df, 'm %d %s res' % (m, route))
            for name, x in (('over_power', out['over']), ('res_power', out['res'])):
                ref = (x.real ** 2 + x.imag ** 2) * ps.reshape(-1, 1, 1)
                assert NP.all(NP.abs(out[name] - ref) <= 4 * U * ref), name
            if first is None:
                first = out
            else:
                assert all(NP.array_equal(out[k], first[k]) for k in want)


def _gold_legs():
    import types
    labels = [tuple(x) for x in GOLD_CLOSURE['cp_labels'].tolist()]
    s = types.SimpleNamespace(labels=labels, baselines=GOLD_CLOSURE['cp_baselines'], bl_reversemap=None)
    return RI.InterferometerArray.closure_leg_table(s, [tuple(t) for t in GOLD_CLOSURE['cp_triplets'].tolist()])[:2]


def test_spectra_from_a_cube_against_the_reference(ctx):
    """The golden closure case without its flagged channel: uploaded and resident cube, one chunk and several; the phases downloaded
    on request are those prisim_closure_phase writes, bit for bit, and the spectra of the two forms are then equal bit for bit."""
    G = GOLD_CLOSURE
    p = json.loads(str(GOLD['cube_params']))
    legs, conj = _gold_legs()
    bpw = GOLD['cube_bp'] * G['cp_bp_wts']
    wts = GOLD['cube_o_freq_wts']
    m = GOLD['cube_o_lags'].size
    nres = GOLD['cube_r_closure_phase_skyvis'].shape[-2]
    for key, cube in zip(KEYS, ('cp_skyvis_freq', 'cp_vis_freq', 'cp_vis_noise_freq')):
        x = G[cube]
        nbl, nchan, nt = x.shape
        _, ph, _ = ctx.closure_phase(x, legs, conj, bpw)
        ctx.set_array(G['cp_baselines'], G['cp_channels'], nt_max=nt)
        for t in range(nt):
            ctx.set_vis(NP.ascontiguousarray(x[:, :, t]), slot=t)
        per_triad = nchan * nt * (3 * 16 + 8) + 2 * nt * (2 * m + nres) * 16      # triplets, phases; spectra, the rocFFT rows
        for c, kw in ((x, {}), (None, {'nt': nt})):
            for budget in (_abi.CLOSURE_BUDGET, 2 * 5 * per_triad):
                out = ctx.closure_delay_spectra(wts, m, p['df'], cube=c, legs=legs, conj=conj, bpwts=bpw, nres=nres, want=('over', 'res'),
                                                want_phase=True, budget_bytes=budget, **kw)
                st = out['stats']
                assert st['phase_route'] == 'direct' and st['route'] == 'rocfft' and st['resident'] == (c is None)
                if budget != _abi.CLOSURE_BUDGET:
                    assert st['chunks'] == 3 and st['chunk_rows'] == 5
                assert NP.array_equal(out['phase'], ph)
                _check(out['over'], GOLD['cube_o_' + key], wts, p['df'], 'cube over ' + key)
                _check(out['res'], GOLD['cube_r_' + key], wts, p['df'], 'cube res ' + key)
                same = ctx.closure_delay_spectra(wts, m, p['df'], phases=ph, nres=nres, want=('over', 'res'))
                assert NP.array_equal(same['over'], out['over']) and NP.array_equal(same['res'], out['res'])
        # nothing but the resampled spectra crosses the link when nothing else is asked for
        out = ctx.closure_delay_spectra(wts, m, p['df'], cube=x, legs=legs, conj=conj, bpwts=bpw, nres=nres, want=('res',))
        assert 'phase' not in out and out['stats']['download_bytes'] == out['res'].nbytes


def test_a_cube_in_three_chunks_is_the_one_chunk_output(ctx):
    """Five triads of an uploaded cube in chunks of 2, 2 and 1 on two streams: phases and spectra bit for bit those of one chunk."""
    rng = NP.random.default_rng(78)
    nbl, nchan, nt, ntriads, m, nres, nwin = 5, 8, 4, 5, 16, 6, 2
    x = rng.standard_normal((nbl, nchan, nt)) + 1j * rng.standard_normal((nbl, nchan, nt))
    bpw = rng.uniform(0.5, 1.5, (nbl, nchan, nt))
    legs = rng.integers(0, nbl, (ntriads, 3)).astype(NP.int32)
    conj = rng.integers(0, 2, (ntriads, 3)).astype(NP.int32)
    wts = _windows(rng, nwin, nchan)
    kw = dict(cube=x, legs=legs, conj=conj, bpwts=bpw, nres=nres, want=('over', 'res'), want_phase=True)
    per_triad = nchan * nt * (3 * 16 + 8) + nwin * nt * (m + nres) * 16         # triplets, phases; the fused route's spectra
    one = ctx.closure_delay_spectra(wts, m, 1e5, **kw)
    three = ctx.closure_delay_spectra(wts, m, 1e5, budget_bytes=2 * 2 * per_triad, **kw)
    st = three['stats']
    assert one['stats']['chunks'] == 1 and st['route'] == 'fused' and st['phase_route'] == 'direct'
    assert st['chunks'] == 3 and st['chunk_rows'] == 2 and st['streams'] == 2
    assert all(NP.array_equal(one[k], three[k]) for k in ('phase', 'over', 'res'))


def test_power_in_three_chunks_is_the_one_chunk_output(ctx):
    """Five spectra in chunks of 2, 2 and 1 on the entry's one stream: every output bit for bit that of one chunk."""
    rng = NP.random.default_rng(79)
    n0, nwin, nlags, nt = 5, 2, 16, 4
    x = rng.standard_normal((n0, nwin, nlags, nt)) + 1j * rng.standard_normal((n0, nwin, nlags, nt))
    scale = rng.uniform(1e-12, 1e-10, nwin)
    want = ('individual', 'auto', 'cross')
    one = ctx.closure_power(x, scale, want=want)
    three = ctx.closure_power(x, scale, want=want, budget_bytes=2 * nwin * nlags * nt * 24)
    st = three['stats']
    assert one['stats']['chunks'] == 1 and st['chunks'] == 3 and st['chunk_rows'] == 2 and st['streams'] == 1
    assert all(NP.array_equal(one[k], three[k]) for k in want)


def test_entry_rejects_bad_input(ctx):
    ph = NP.zeros((2, 8, 3))
    wts = NP.ones((1, 8))
    with pytest.raises(ValueError, match='PRISIM_CPDELAY_MAX_LEN'):
        ctx.closure_delay_spectra(wts, 4097, 1e5, phases=ph, want=('over',))
    with pytest.raises(ValueError, match='nchan <= m'):
        ctx.closure_delay_spectra(wts, 4, 1e5, phases=ph, want=('over',))
    with pytest.raises(ValueError, match='got nres'):
        ctx.closure_delay_spectra(wts, 16, 1e5, phases=ph, nres=0, want=('res',))
    with pytest.raises(ValueError, match='null array'):
        ctx.closure_delay_spectra(wts, 16, 1e5, phases=ph, want=('over_power',))
    with pytest.raises(ValueError, match='at least two entries'):
        ctx.closure_power(NP.ones((1, 1, 4), dtype=NP.complex128), [1.0], want=('cross',))


@pytest.mark.parametrize('n0,budget_rows', [(2, None), (23, 5), (300, 64)])
def test_power_spectra_against_the_derived_bounds(ctx, n0, budget_rows):
    rng = NP.random.default_rng(n0)
    nwin, nlags, nt = 2, 11, 7
    common = rng.standard_normal((1, nwin, nlags, nt)) + 1j * rng.standard_normal((1, nwin, nlags, nt))
    x = common + 0.3 * (rng.standard_normal((n0, nwin, nlags, nt)) + 1j * rng.standard_normal((n0, nwin, nlags, nt)))
    scale = rng.uniform(1e-12, 1e-10, nwin)
    budget = _abi.CLOSURE_BUDGET if budget_rows is None else budget_rows * nwin * nlags * nt * 24
    out = ctx.closure_power(x, scale, want=('individual', 'auto', 'cross'), budget_bytes=budget)
    if budget_rows is not None:
        assert out['stats']['chunk_rows'] == budget_rows and out['stats']['chunks'] == -(-n0 // budget_rows) > 1
    worst = CC.individual_error(out['individual'], x, scale)
    print(n0, 'individual: %.2f u from the exact value (bound 4 u); numpy\'s abs()**2 * scale: %.2f u'
          % (worst, CC.individual_error(CC.power_individual(x, scale), x, scale)))
    assert out['individual'].shape == x.shape and worst <= 4
    auto, cross = CC.power_averaged(x, scale)
    b_auto, b_cross = CC.power_bounds(x, scale)
    assert out['auto'].shape == out['cross'].shape == (1, nwin, nlags, nt)
    print(n0, 'auto %.2f of its bound, cross %.2f of its bound' % (NP.max(NP.abs(out['auto'] - auto) / b_auto),
                                                                   NP.max(NP.abs(out['cross'] - cross) / b_cross)))
    assert NP.all(NP.abs(out['auto'] - auto) <= b_auto) and NP.all(NP.abs(out['cross'] - cross) <= b_cross)
    only = ctx.closure_power(x, scale, want=('cross',), budget_bytes=budget)
    assert NP.array_equal(only['cross'], out['cross']) and set(only) == {'cross', 'stats'}


# ---- through the classes ----------------------------------------------------------------------------------------------------------

def _hera19_array(nt, flagged=None, noise_seed=None):
    cfg = W.config2()
    pos = LAY.array_layout('HERA-19')
    bl, ids = LAY.fold_and_sort_baselines(*LAY.baseline_generator(pos))
    labels = [(str(int(a)), str(int(b))) for a, b in ids]
    ch, sky = cfg['channels'], cfg['sky']
    shape = None if sky.get('fwhm_deg') is None else NP.stack((sky['fwhm_deg'], sky['fwhm_deg'], NP.zeros_like(sky['fwhm_deg'])), axis=1)
    skymod = SM.SkyModel(location=sky['altaz'], flux_ref=sky['flux_ref'], spindex=sky['spindex'], ref_freq=sky['ref_freq'], src_shape=shape)
    layout = {'positions': pos, 'labels': NP.array([str(i) for i in range(len(pos))]), 'ids': NP.arange(len(pos)), 'coords': 'ENU'}
    ia = RI.InterferometerArray(labels, bl, ch, telescope={'id': 'hera', 'shape': 'delta', 'size': 14.0, 'ocoords': 'altaz',
                                                           'orientation': NP.array([[90.0, 270.0]]), 'groundplane': None},
                                latitude=-30.7224, skycoords='altaz', pointing_coords='altaz', layout=layout)
    ia.reserve(nt)
    bpass = 0.6 + 0.4 * NP.hanning(ch.size + 2)[1:-1]
    if flagged is not None:
        bpass[flagged] = 0.0
    for j in range(nt):
        ia.observe((2457000.5 + j / 64.0, 30.0 + 0.25 * j), {'Tnet': 200.0}, bpass, [90.0, 270.0], skymod, 10.7)
    if noise_seed is not None:
        ia.generate_noise(seed=noise_seed)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            ia.add_noise()
    return ia


def _subbands(ia):
    f, df = ia.channels, ia.freq_resolution
    return NP.asarray([0.2 * f.size * df]), {'freq_center': NP.asarray([f[int(0.7 * f.size)], f[int(0.3 * f.size)]]), 'shape': 'bhw',
                                             'pad': 1.0, 'verbose': False}


@pytest.mark.parametrize('filtered', [False, True])
def test_both_input_forms_agree_on_a_flagged_channel(filtered):
    """cpinfo=getClosurePhase(...) and cpinfo=None with the same arguments, on an array with a flagged channel (every bispectrum there is
    exactly zero): the phase prisim_closure_phase writes there is the phase that is transformed, on both forms."""
    ia = _hera19_array(3, flagged=7, noise_seed=21)
    few = ia.getThreePointCombinations()[0][::300]
    kw_cp = {'antenna_triplets': few}
    if filtered:
        kw_cp.update(delay_filter_info={'type': 'horizon', 'mode': 'discard', 'width': 2.0},
                     spectral_window_info={'freq_center': None, 'bw_eff': None, 'shape': 'bhw', 'fftpow': None})
    cp = ia.getClosurePhase(**kw_cp)
    if not filtered:
        zero = NP.prod(cp['skyvis'], axis=1) == 0
        assert zero[:, 7, :].all() and zero.sum() == zero[:, 7, :].size and NP.all(NP.isfinite(cp['closure_phase_skyvis']))
    ds = DS.DelaySpectrum(ia)
    bw, kw = _subbands(ia)
    for action in ('return_oversampled', None):
        a = ds.subband_delay_transform_closure_phase(bw, cpinfo=cp, action=action, **kw)
        b = ds.subband_delay_transform_closure_phase(bw, action=action, **kw_cp, **kw)
        st = ia.closure_delay_stats
        assert set(st) == set(KEYS) and st[KEYS[0]]['resident'] and not st[KEYS[1]]['resident']
        assert all(v['phase_route'] == ('fused' if filtered else 'direct') and v['route'] == 'fused' for v in st.values())
        for key in KEYS:
            _check(b[key], a[key], a['freq_wts'], ia.freq_resolution, 'forms %s %s' % (action, key))
        assert sorted(a) == sorted(b)
    cp2 = ia.getClosurePhase(**kw_cp)                                     # getClosurePhase itself is untouched by the calls between
    assert all(NP.array_equal(cp[k], cp2[k]) for k in KEYS + ('skyvis', 'vis', 'noisevis'))


def test_end_to_end_hera19_unique_triads():
    """observe, getClosurePhase, the closure-phase delay spectra and both power spectra in sequence on the 162 unique triads."""
    nt = 4
    ia = _hera19_array(nt, noise_seed=22)
    trip = ia.getThreePointCombinations(unique=True)[0]
    assert len(trip) == 162
    cp = ia.getClosurePhase(antenna_triplets=trip)
    ds = DS.DelaySpectrum(ia)
    bw, kw = _subbands(ia)
    nchan, df = ia.channels.size, ia.freq_resolution
    m = 2 * nchan
    res = ds.subband_delay_transform_closure_phase(bw, antenna_triplets=trip, **kw)
    over = ds.subband_delay_transform_closure_phase(bw, antenna_triplets=trip, action='return_oversampled', **kw)
    nres = res['closure_phase_skyvis'].shape[-2]
    assert nres == int(round(m / NP.min(m * df / bw)))
    for key in KEYS:
        assert res[key].shape == (162, 2, nres, nt) and over[key].shape == (162, 2, m, nt)
        want_o, want_r = CC.delay_spectra(cp[key], res['freq_wts'], m, df, nres)       # the checker fed the device's own phases
        _check(res[key], want_r, res['freq_wts'], df, 'end to end res ' + key)
        _check(over[key], want_o, res['freq_wts'], df, 'end to end over ' + key)
    assert res['lag_kernel'].shape == (1, 2, res['lags'].size, 1) and len(res['baseline_triplets']) == 162
    dps = DS.DelayPowerSpectrum(ds)
    ind = dps.compute_individual_closure_phase_power_spectrum(res)
    avg = dps.compute_averaged_closure_phase_power_spectrum(res)
    assert ind['kprll'].shape == (2, res['lags'].size) and ind['kperp'].shape == (2, 162, 3)
    assert ind['horizon_kprll_limits'].shape == (nt, 2, 162, 3, 2)
    z = DS.REST_FREQ_HI / res['freq_center'] - 1
    factor = dps.comoving_los_depth(res['bw_eff'], z, action='return') / res['bw_eff'] ** 2
    for key in KEYS:
        worst = CC.individual_error(ind[key], res[key], factor)
        print('end to end individual %s: %.2f u from the exact value (bound 4 u)' % (key, worst))
        assert ind[key].shape == res[key].shape and NP.all(NP.isfinite(ind[key])) and worst <= 4
        auto, cross = CC.power_averaged(res[key], factor)
        b_auto, b_cross = CC.power_bounds(res[key], factor)
        assert avg['auto'][key].shape == avg['cross'][key].shape == (1, 2, nres, nt)
        assert NP.all(NP.abs(avg['auto'][key] - auto) <= b_auto) and NP.all(NP.abs(avg['cross'][key] - cross) <= b_cross)
