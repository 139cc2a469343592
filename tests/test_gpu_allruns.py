"""GPU: delay spectra and power spectra of stacks of runs (include/prisim_runs.h) against the reference's fixtures
(tests/golden/golden_allruns.npz), against the numpy restatement (tests/allruns_checker.py) on a seeded sweep through every route, against
DelaySpectrum.delay_transform / subband_delay_transform on an observed array, and config 2 with two independent noise realisations as
runs: their cross power has no noise bias, their auto power has."""
import json
import os
import sys

import numpy as NP
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import allruns_checker as CK  # noqa: E402
import test_allruns as TA  # noqa: E402

from prisim_amd import _abi, delay_spectrum as DS, skymodel as SM, workloads as W  # noqa: E402

pytestmark = pytest.mark.gpu


def test_fixtures_through_the_device():
    g = NP.load(TA.GOLD)
    with _abi.Context(0) as ctx:
        for i in range(int(g['nfull'])):
            pre = 'f%d_' % i
            if pre + 'raises' in g.files:
                continue
            res = TA.run_full(g, i, ctx)
            for key in ('vis_lag', 'lag_kernel'):
                assert res[key].shape == g[pre + 'out_' + key].shape
                assert TA.rel_err(res[key], g[pre + 'out_' + key]) <= 1e-12, (i, key)
            assert NP.array_equal(res['lags'], g[pre + 'out_lags'])
        for i in range(int(g['nsub'])):
            pre = 's%d_' % i
            if pre + 'raises' in g.files:
                with pytest.raises(ValueError):
                    TA.run_sub(g, i, ctx)
                continue
            res = TA.run_sub(g, i, ctx)
            # sub-bands away from channel 0 resample to round-off (prisim_amd/dsp_readings.py:downsampler): errors are measured
            # against the oversampled spectra the resampling starts from
            _, vis, bp, _, f, _, _ = TA.sub_case(g, i)
            nbl, nchan, nt = bp.shape
            m = nchan + int(res['npad'])
            wins = res['freq_wts'].reshape(-1, nchan)
            for key, x in (('vis_lag', vis), ('lag_kernel', None)):
                over = CK.transform(x, nbl, nchan, nt, bp=bp, win=wins, m=m, scale=m * TA.DF)
                want = g[pre + 'out_' + key]
                assert res[key].shape == want.shape
                assert NP.max(NP.abs(res[key] - want)) <= 1e-12 * NP.max(NP.abs(over)), (i, key)
        same_numpy = list(g['numpy_fused']) == [_abi.numpy_fuses_complex_product(NP.complex128),
                                                _abi.numpy_fuses_complex_product(NP.complex64)]
        for i in range(int(g['npow'])):
            p, dspec, want = TA.power_case(g, i)
            ds = TA.make_ds(150e6 + TA.DF * NP.arange(24), NP.ones((1, 24, 1)), NP.ones((1, 24, 1)), ctx)
            dps = TA.make_dps(ds)
            key = 'subband' if p['subband'] else 'fullband'
            got = dps.compute_power_spectrum_allruns(dict(dspec), subband=p['subband'])[key]
            if same_numpy:
                assert NP.array_equal(got, want), i
            else:
                assert TA.rel_err(got, want) <= 1e-6, i


def test_power_is_the_numpy_statement_bit_for_bit():
    rng = NP.random.default_rng(17)
    with _abi.Context(0) as ctx:
        for dt in (NP.complex128, NP.complex64):
            shp = (3, 2, 5, 64, 7)
            v1 = (rng.standard_normal(shp) + 1j * rng.standard_normal(shp)).astype(dt)
            v2 = (rng.standard_normal(shp) + 1j * rng.standard_normal(shp)).astype(dt)
            fac = rng.uniform(1e6, 1e8, 3)
            for cross in (False, True):
                for budget in (_abi.RUNS_BUDGET, 64 * 1024):
                    got, st = ctx.runs_power(v1, v2 if cross else None, fac, cross=cross, budget_bytes=budget)
                    assert NP.array_equal(got, CK.power(v1, v2 if cross else None, fac, cross)), (dt, cross, budget)
                    assert (st['chunks'] > 1) == (budget < _abi.RUNS_BUDGET)


def test_seeded_sweep_through_every_route():
    rng = NP.random.default_rng(23)
    cases = [  # (lead, nbl, nchan, nt, pad, mode, c64, route, budget, weights)
        ((3,), 5, 64, 7, 1.0, 'interp', False, 'auto', _abi.RUNS_BUDGET, 'dense'),
        ((3,), 5, 64, 7, 1.0, 'interp', False, 'rocfft', _abi.RUNS_BUDGET, 'dense'),
        ((2, 3), 4, 100, 5, 1.0, 'interp', True, 'auto', 200 * 1024, 'chan'),
        ((4,), 3, 96, 9, 0.5, 'interp', False, 'auto', 128 * 1024, 'bl'),
        ((4,), 3, 64, 9, 0.5, 'all', False, 'auto', 128 * 1024, 'chan_t'),
        ((2,), 3, 128, 3, 1.0, 'resample', True, 'auto', 64 * 1024, 'dense'),
        ((2,), 3, 100, 70, 0.0, 'all', False, 'auto', _abi.RUNS_BUDGET, 'dense'),
        ((1,), 2, 2048, 2, 1.0, 'all', False, 'auto', _abi.RUNS_BUDGET, 'chan'),        # m = PRISIM_SUBBAND_MAX_LEN, fused
        ((1,), 2, 2000, 2, 1.0, 'interp', False, 'auto', _abi.RUNS_BUDGET, 'chan'),     # m = 4000, rocFFT
        ((2,), 2, 1, 3, 0.0, 'all', False, 'fused', _abi.RUNS_BUDGET, 'dense'),         # m = 1: no bit to reverse, no butterfly
        ((2,), 2, 2, 3, 0.0, 'all', False, 'fused', _abi.RUNS_BUDGET, 'dense'),         # m = 2: one butterfly
        ((2,), 2, 8, 65, 0.0, 'all', False, 'fused', _abi.RUNS_BUDGET, 'dense'),        # a full tile of 64 snapshots and one more
        ((3,), 3, 12, 5, 0.0, 'all', False, 'auto', 2 * 2 * 3 * 12 * 5 * 16, 'dense'),  # m = 12, rocFFT: four chunks of 2 pairs, one of 1
        ((2,), 2, 3, 4, 0.0, 'resample', False, 'auto', _abi.RUNS_BUDGET, 'dense'),     # resampled to 1 lag
        ((2,), 2, 15, 4, 0.0, 'resample', False, 'auto', _abi.RUNS_BUDGET, 'dense'),    # resampled to 5 lags
    ]
    with _abi.Context(0) as ctx:
        routes = set()
        for lead, nbl, nchan, nt, pad, mode, c64, route, budget, weights in cases:
            shp = lead + (nbl, nchan, nt)
            vis = rng.standard_normal(shp) + 1j * rng.standard_normal(shp)
            vis = vis.astype(NP.complex64 if c64 else NP.complex128)
            bp = 0.5 + rng.uniform(size=(nbl, nchan, nt))
            wts = {'dense': rng.uniform(size=(nbl, nchan, nt)), 'chan': rng.uniform(size=(nchan, 1)),
                   'bl': rng.uniform(size=(nbl, nchan, 1)), 'chan_t': rng.uniform(size=(nchan, nt))}[weights]
            win = rng.uniform(size=(2, nchan)) if mode == 'resample' else None
            m = nchan + int(nchan * pad)
            nout = {'all': m, 'interp': NP.arange(0, m, 1 + pad).size, 'resample': m // 3}[mode]
            kw = dict(bp=bp, wts=wts, win=win, m=m, scale=m * 1e5, mode=mode, nout=nout, factor=1 + pad)
            got, st = ctx.runs_transform(vis, nbl, nchan, nt, route=route, budget_bytes=budget, **kw)
            routes.add(st['route'])
            want = CK.transform(vis, nbl, nchan, nt, **kw)
            assert got.shape == want.shape
            assert TA.rel_err(got, want) <= 1e-12, (shp, mode, route)
            if budget < _abi.RUNS_BUDGET:
                assert st['chunks'] > 2 and st['streams'] == 2
            k, _ = ctx.runs_transform(None, nbl, nchan, nt, **kw)
            assert TA.rel_err(k, CK.transform(None, nbl, nchan, nt, **kw)) <= 1e-12
        assert routes == {'fused', 'rocfft', 'direct'}
        with pytest.raises(ValueError, match='PRISIM_SUBBAND_MAX_LEN'):
            ctx.runs_transform(NP.ones((1, 1, 8, 1), complex), 1, 8, 1, m=_abi.PRISIM_SUBBAND_MAX_LEN + 1)


@pytest.mark.parametrize('m', [16, 12])
def test_transform_in_three_chunks_is_the_one_chunk_output(m):
    """Five (run, baseline) pairs in chunks of 2, 2 and 1 on two streams, fused (m = 16) and through rocFFT (m = 12, whose plan for the
    last chunk has another batch): bit for bit the output of one chunk."""
    rng = NP.random.default_rng(m)
    nbl, nchan, nt = 5, 8, 4
    vis = rng.standard_normal((1, nbl, nchan, nt)) + 1j * rng.standard_normal((1, nbl, nchan, nt))
    kw = dict(bp=0.5 + rng.uniform(size=(nbl, nchan, nt)), wts=rng.uniform(size=(nbl, nchan, nt)), m=m, scale=m * 1e5)
    route = 'fused' if m == 16 else 'rocfft'
    per_pair = nchan * nt * 16 + m * nt * 16 + (m * nt * 16 if route == 'rocfft' else 0)      # input, output, the rocFFT rows
    with _abi.Context(0) as ctx:
        one, st1 = ctx.runs_transform(vis, nbl, nchan, nt, **kw)
        three, st3 = ctx.runs_transform(vis, nbl, nchan, nt, budget_bytes=2 * 2 * per_pair, **kw)
    assert st1['chunks'] == 1 and st1['route'] == st3['route'] == route
    assert st3['chunks'] == 3 and st3['chunk_pairs'] == 2 and st3['streams'] == 2
    assert NP.array_equal(one, three)


@pytest.mark.parametrize('cross', [False, True])
def test_power_in_three_chunks_is_the_one_chunk_output(cross):
    """Five elements in chunks of 2, 2 and 1 on two streams: bit for bit the output of one chunk."""
    rng = NP.random.default_rng(31)
    v1 = rng.standard_normal(5) + 1j * rng.standard_normal(5)
    v2 = rng.standard_normal(5) + 1j * rng.standard_normal(5) if cross else None
    per = 16 * (2 if cross else 1) + 8                                                       # the inputs and the output
    with _abi.Context(0) as ctx:
        one, st1 = ctx.runs_power(v1, v2, 3e7, cross=cross)
        three, st3 = ctx.runs_power(v1, v2, 3e7, cross=cross, budget_bytes=2 * 2 * per)
    assert st1['chunks'] == 1 and st3['chunks'] == 3 and st3['chunk_pairs'] == 2 and st3['streams'] == 2
    assert NP.array_equal(one, three) and NP.array_equal(one, CK.power(v1, v2, 3e7, cross))


def test_a_selection_map_with_three_entries_for_one_bin_is_refused(monkeypatch):
    from prisim_amd import dsp_readings as D
    monkeypatch.setattr(D, 'resample_map', lambda m, n: (NP.zeros(3, dtype=NP.int64), NP.arange(3, dtype=NP.int64), NP.ones(3)))
    with _abi.Context(0) as ctx:
        with pytest.raises(ValueError, match='more than two entries'):
            ctx.runs_transform(NP.ones((1, 1, 8, 1), complex), 1, 8, 1, m=8, mode='resample', nout=5)


def _config2_array(nt, noise=False):
    from prisim_amd import interferometry as RI
    cfg = W.config2()
    bl, ch, sky = cfg['baselines'], cfg['channels'], cfg['sky']
    skymod = SM.SkyModel(location=sky['altaz'], flux_ref=sky['flux_ref'], spindex=sky['spindex'], ref_freq=sky['ref_freq'],
                         src_shape=NP.stack((sky['fwhm_deg'], sky['fwhm_deg'], NP.zeros_like(sky['fwhm_deg'])), axis=1))
    ia = RI.InterferometerArray(['b%d' % i for i in range(bl.shape[0])], bl, ch, telescope={'id': 'hera'}, latitude=-30.7224,
                                skycoords='altaz', pointing_coords='altaz')
    ia.reserve(nt)
    bpass = 0.6 + 0.4 * NP.hanning(ch.size + 2)[1:-1]
    for j in range(nt):
        ia.observe((2457000.5 + j / 64.0, 30.0 + 0.25 * j), {'Tnet': 200.0}, bpass, [90.0, 270.0], skymod, 10.7)
    return ia


def test_cross_checks_with_the_existing_delay_transforms():
    nt = 4
    ia = _config2_array(nt)
    ds = DS.DelaySpectrum(ia)
    sky = NP.asarray(ia.skyvis_freq)
    for pad in (1.0, 0.5):
        want = ds.delay_transform(pad=pad, verbose=False)['skyvis_lag']
        got = ds.delay_transform_allruns(sky[None], pad=pad, verbose=False)['vis_lag'][0]
        assert got.shape == want.shape and TA.rel_err(got, want) <= 1e-12, pad
    f, df, nchan = ds.f, ds.df, ds.f.size
    fc = f[[nchan // 4, nchan // 2, 3 * nchan // 4]]
    bw = nchan * df / 8
    ds.subband_delay_transform({'sim': bw, 'cc': bw}, freq_center={'sim': fc, 'cc': fc}, shape={'sim': 'bnw', 'cc': 'bnw'},
                               pad={'sim': 1.0, 'cc': 1.0}, verbose=False)
    want = NP.transpose(ds.subband_delay_spectra_resampled['sim']['skyvis_lag'], (1, 0, 2, 3))        # (n_win, nbl, nres, nt)
    res = ds.subband_delay_transform_allruns(sky[None], bw, freq_center=fc, shape='bnw', pad=1.0, action='return_resampled',
                                             verbose=False)
    got = res['vis_lag'][:, 0]
    over = NP.max(NP.abs(ds.subband_delay_spectra['sim']['skyvis_lag']))     # windows away from channel 0 resample to round-off
    assert got.shape == want.shape and NP.max(NP.abs(got - want)) <= 1e-12 * over
    kern = NP.transpose(ds.subband_delay_spectra_resampled['sim']['lag_kernel'], (1, 0, 2, 3))
    assert TA.rel_err(res['lag_kernel'][:, 0], kern) <= 1e-12
    assert NP.allclose(res['lags'], ds.subband_delay_spectra_resampled['sim']['lags'], rtol=1e-15, atol=0)


def test_config2_noise_runs_cross_power_is_unbiased():
    """HERA-19 (171 baselines, 256 channels): the sky plus two independent seeded noise realisations, as runs.  The cross power of the
    two noise-only runs averages to zero within its scatter; the auto power of each run carries the noise bias."""
    nt = 8
    ia = _config2_array(nt)
    ds = DS.DelaySpectrum(ia)
    sky = NP.asarray(ia.skyvis_freq)
    nbl, nchan = sky.shape[:2]
    rng = NP.random.default_rng(2026)
    sigma = 0.5 * NP.std(sky)
    noise = sigma * (rng.standard_normal((2,) + sky.shape) + 1j * rng.standard_normal((2,) + sky.shape))
    runs = NP.stack([sky, sky + noise[0], sky + noise[1], noise[0], noise[1]])          # (5, nbl, nchan, nt)
    lag = ds.delay_transform_allruns(runs, pad=1.0, verbose=False)['vis_lag']
    dps = DS.DelayPowerSpectrum(ds)
    factor = float(NP.ravel(dps.jacobian1 * dps.jacobian2 * dps.Jy2K ** 2)[0])
    cross = dps.compute_power_spectrum_allruns({'vislag1': lag[3], 'vislag2': lag[4]})['fullband']
    auto = [dps.compute_power_spectrum_allruns({'vislag1': lag[i]})['fullband'] for i in range(3)]
    assert NP.array_equal(cross, 2 * (lag[3] * lag[4].conj() * factor).real)
    # expected noise power per lag: factor df^2 sum_n (bp bp_wts)^2 E|n|^2, E|n|^2 = 2 sigma^2
    w2 = NP.sum((NP.asarray(ia.bp) * NP.asarray(ia.bp_wts)) ** 2, axis=1)                          # (nbl, nt)
    bias = factor * ds.df ** 2 * 2 * sigma ** 2 * w2[:, None, :]
    n = cross.size
    assert abs(NP.mean(cross / bias)) <= 5 * NP.std(cross / bias) / NP.sqrt(n)
    for i in (1, 2):
        excess = NP.mean((auto[i] - auto[0]) / bias)
        assert 0.9 <= excess <= 1.1, (i, excess)
    sky_cross = dps.compute_power_spectrum_allruns({'vislag1': lag[1], 'vislag2': lag[2]})['fullband']
    assert abs(NP.mean((sky_cross / 2 - auto[0]) / bias)) <= 0.1
