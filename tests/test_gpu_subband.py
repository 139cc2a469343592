"""GPU: sub-band delay spectra (include/prisim_subband.h) against the reference's fixtures (tests/golden/golden_subband.npz), against the
numpy checker (tests/subband_checker.py) on a seeded sweep through both routes, the power-only call against the complex one, and
subband_delay_transform -> compute_power_spectrum after observe -> delayClean at config-2 size."""
import json
import os
import sys

import numpy as NP
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import subband_checker as CK  # noqa: E402

from prisim_amd import _abi, delay_spectrum as DS, dsp_readings as D, skymodel as SM, workloads as W  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'golden_subband.npz')
pytestmark = pytest.mark.gpu
CC = ('skyvis', 'vis', 'skyvis_res', 'vis_res', 'skyvis_net', 'vis_net')


def _to_ref(a):
    """(ncubes, nt, nbl, nwin, lags) -> [(nbl, nwin, lags, nt)]"""
    return [NP.transpose(a[c], (1, 2, 3, 0)) for c in range(a.shape[0])]


def test_fixtures_through_the_device():
    g = NP.load(GOLD)
    routes = set()
    with _abi.Context(0) as ctx:
        for i in range(int(g['n'])):
            pre = 'c%d_' % i
            p = json.loads(str(g[pre + 'params']))
            f, bp = g[pre + 'f'], g[pre + 'bp']
            nchan, df = f.size, p['df']
            keys = {'sim': ('skyvis', 'vis', 'vis_noise')}
            if p['with_cc']:
                keys['cc'] = CC
            npad_last = int(nchan * p['pad']['sim'])
            for key, names in keys.items():
                fw = g['%so_%s_freq_wts' % (pre, key)]
                m = nchan + int(g['%so_%s_npad' % (pre, key)])
                factor = NP.min((nchan + npad_last) * df / NP.asarray(p['bw_eff'][key]))
                nres = D.fft_downsample_length(m, factor)
                src = [g[pre + (n + '_freq' if key == 'sim' else 'cc_%s_freq' % n)][:, :nchan, :] for n in names]
                x = NP.stack([NP.transpose(s, (2, 0, 1)) for s in src])
                bprow = NP.transpose(bp, (2, 0, 1)).reshape(-1, nchan)
                for route in ('fused', 'rocfft'):
                    if route == 'fused' and m & (m - 1):
                        continue
                    out = ctx.subband_transform(x, bprow, fw, m, df, nres=nres, want=('over', 'res'), route=route)
                    routes.add(out['stats']['route'])
                    for c, n in enumerate(names):
                        want = g['%so_%s_%s_lag' % (pre, key, n)]
                        assert CK.rel_err(_to_ref(out['over'])[c], want) <= 1e-12, (i, key, n, route)
                        assert CK.rel_err(_to_ref(out['res'])[c], g['%sr_%s_%s_lag' % (pre, key, n)], scale_of=want) <= 1e-12, (i, key, n, route)
                    k = ctx.subband_transform(bprow.astype(complex).reshape(1, 1, -1, nchan), NP.ones((1, nchan)), fw, m, df, want=('over',),
                                              route=route)
                    assert CK.rel_err(_to_ref(k['over'].reshape(1, p['nt'], p['nbl'], fw.shape[0], m))[0],
                                      g['%so_%s_lag_kernel' % (pre, key)]) <= 1e-12, (i, key, route)
    assert routes == {'fused', 'rocfft'}


def test_seeded_sweep_against_the_checker():
    rng = NP.random.default_rng(2026)
    routes, df = set(), 97.65625e3
    with _abi.Context(0) as ctx:
        for nchan in (31, 64, 100, 256, 1024):
            f = 100e6 + df * NP.arange(nchan)
            for pad in (0.0, 0.37, 1.0, 3.0):
                m = nchan + int(nchan * pad)
                if m > _abi.PRISIM_SUBBAND_MAX_LEN:
                    continue
                shape = ('rect', 'bhw', 'bnw')[int(rng.integers(3))]
                nwin = int(rng.integers(1, 9))
                nbl, nt = 3, 2
                bw = rng.uniform(0.05, 0.5, nwin) * nchan * df
                fc = f[rng.integers(1, nchan - 1, nwin)]
                fw = CK.freq_wts(f, df, bw, fc, shape)
                x = rng.normal(size=(2, nbl, nchan, nt)) + 1j * rng.normal(size=(2, nbl, nchan, nt))
                bp = 0.5 + rng.uniform(size=(nbl, nchan, 1))
                factor = NP.min(m * df / bw)
                nres = D.fft_downsample_length(m, factor)
                ps = rng.uniform(1.0, 2.0, nwin)
                xin = NP.stack([NP.transpose(c, (2, 0, 1)) for c in x])
                for route in ('auto', 'rocfft'):
                    out = ctx.subband_transform(xin, bp[:, :, 0], fw, m, df, nres=nres, pscale=ps,
                                                want=('over', 'over_power', 'res', 'res_power'), route=route)
                    routes.add(out['stats']['route'])
                    assert out['stats']['rows'] == 2 * nbl * nt
                    for c in range(2):
                        want = CK.transform(x[c], bp, fw, m - nchan, df)
                        wres = D.resample(want, nres, axis=2)
                        assert CK.rel_err(_to_ref(out['over'])[c], want) <= 1e-12, (nchan, pad, route)
                        assert CK.rel_err(_to_ref(out['res'])[c], wres, scale_of=want) <= 1e-12, (nchan, pad, route)
                        pw = NP.abs(want) ** 2 * ps.reshape(1, -1, 1, 1)
                        assert CK.rel_err(_to_ref(out['over_power'])[c], pw) <= 1e-12
                        assert NP.allclose(_to_ref(out['res_power'])[c], NP.abs(_to_ref(out['res'])[c]) ** 2 * ps.reshape(1, -1, 1, 1),
                                           rtol=1e-13, atol=0)
    assert routes == {'fused', 'rocfft'}


@pytest.mark.parametrize('nchan,m,nt,route,nres', [(1, 1, 2, 'fused', 1), (2, 2, 2, 'fused', 1), (5, 8, 3, 'fused', 5), (7, 12, 3, 'rocfft', 5),
                                                   (7, 12, 3, 'rocfft', 1)])
def test_shortest_rows_and_shortest_resampled_spectra(nchan, m, nt, route, nres):
    """m = 1 and 2 (no bit to reverse, one butterfly), m = 8, and m = 12 through rocFFT; resampled to 1 and to 5 lags."""
    rng = NP.random.default_rng(100 * m + nres)
    nbl, nwin, df = 3, 2, 97.65625e3
    fw = rng.uniform(0.2, 1.5, (nwin, nchan))
    x = rng.normal(size=(2, nbl, nchan, nt)) + 1j * rng.normal(size=(2, nbl, nchan, nt))
    bp = 0.5 + rng.uniform(size=(nbl, nchan, 1))
    ps = rng.uniform(1.0, 2.0, nwin)
    xin = NP.stack([NP.transpose(c, (2, 0, 1)) for c in x])
    with _abi.Context(0) as ctx:
        out = ctx.subband_transform(xin, bp[:, :, 0], fw, m, df, nres=nres, pscale=ps, want=('over', 'over_power', 'res', 'res_power'),
                                    route=route)
    assert out['stats']['route'] == route and out['res'].shape[-1] == nres
    for c in range(2):
        want = CK.transform(x[c], bp, fw, m - nchan, df)
        assert CK.rel_err(_to_ref(out['over'])[c], want) <= 1e-12
        assert CK.rel_err(_to_ref(out['res'])[c], D.resample(want, nres, axis=2), scale_of=want) <= 1e-12
        assert CK.rel_err(_to_ref(out['over_power'])[c], NP.abs(want) ** 2 * ps.reshape(1, -1, 1, 1)) <= 1e-12
        assert NP.allclose(_to_ref(out['res_power'])[c], NP.abs(_to_ref(out['res'])[c]) ** 2 * ps.reshape(1, -1, 1, 1), rtol=1e-13, atol=0)


def test_a_selection_map_with_three_entries_for_one_bin_is_refused(monkeypatch):
    monkeypatch.setattr(D, 'resample_map', lambda m, n: (NP.zeros(3, dtype=NP.int64), NP.arange(3, dtype=NP.int64), NP.ones(3)))
    with _abi.Context(0) as ctx:
        with pytest.raises(ValueError, match='more than two entries'):
            ctx.subband_transform(NP.ones((1, 1, 1, 8), dtype=complex), NP.ones((1, 8)), NP.ones((1, 8)), 8, 1.0, nres=5, want=('res',))


def test_length_limit_is_a_clear_error():
    with _abi.Context(0) as ctx:
        x = NP.ones((1, 1, 1, 8), dtype=complex)
        with pytest.raises(ValueError, match='PRISIM_SUBBAND_MAX_LEN'):
            ctx.subband_transform(x, NP.ones((1, 8)), NP.ones((1, 8)), _abi.PRISIM_SUBBAND_MAX_LEN + 1, 1.0, want=('over',))
        with pytest.raises(ValueError, match='PRISIM_SUBBAND_MAX_LEN'):
            ctx.subband_transform(x, NP.ones((1, 8)), NP.ones((1, 8)), 16, 1.0, nres=_abi.PRISIM_SUBBAND_MAX_LEN + 1, want=('res',))
        with pytest.raises(ValueError, match='fused'):
            ctx.subband_transform(x, NP.ones((1, 8)), NP.ones((1, 8)), 12, 1.0, want=('over',), route='fused')


def _config2_array(nt):
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
    ia.generate_noise(seed=11)
    ia.add_noise()
    return ia


def test_config2_end_to_end_and_power_only_call():
    nt = 64
    ia = _config2_array(nt)
    nbl, nchan = ia.baselines.shape[0], ia.channels.size
    ds = DS.DelaySpectrum(ia)
    ds.delayClean(pad=1.0, verbose=False)
    f, df = ds.f, ds.df
    fc = {'cc': f[[nchan // 4, nchan // 2, 3 * nchan // 4]], 'sim': f[[nchan // 4, nchan // 2, 3 * nchan // 4]]}
    bw = {'cc': nchan * df / 8, 'sim': nchan * df / 8}
    ds.subband_delay_transform(bw, freq_center=fc, shape={'cc': 'bhw', 'sim': 'bnw'}, pad={'cc': 1.0, 'sim': 1.0}, verbose=False)
    assert ds._subband_stats['rows'] > 0
    cubes = {'sim': {'skyvis': NP.asarray(ia.skyvis_freq), 'vis': NP.asarray(ia.vis_freq), 'vis_noise': NP.asarray(ia.vis_noise_freq)},
             'cc': {n: getattr(ds, 'cc_%s_freq' % n) for n in CC}}
    rng = NP.random.default_rng(9)
    body = NP.sort(rng.choice(nbl, 12, replace=False))
    sub = {k: {n: v[body] for n, v in d.items()} for k, d in cubes.items()}
    bp = NP.asarray(ia.bp)[body]
    res, rres = CK.subband(f, df, sub, bp, {k: NP.repeat(bw[k], 3) for k in bw}, fc, {'cc': 'bhw', 'sim': 'bnw'},
                           {'cc': 1.0, 'sim': 1.0})
    for key in ('cc', 'sim'):
        o, r = ds.subband_delay_spectra[key], ds.subband_delay_spectra_resampled[key]
        assert NP.array_equal(o['freq_wts'], res[key]['freq_wts'])
        for name, want in res[key].items():
            if not (name.endswith('_lag') or name == 'lag_kernel'):
                continue
            scale = NP.max(NP.abs(want))
            assert NP.max(NP.abs(o[name][body] - want)) <= 1e-10 * scale, (key, name)
            assert NP.max(NP.abs(r[name][body] - rres[key][name])) <= 1e-10 * scale, (key, name)
    dps = DS.DelayPowerSpectrum(ds)
    dps.compute_power_spectrum()
    for key in ('cc', 'sim'):
        p = dps.subband_delay_power_spectra[key]
        assert p['factor'].shape == (3,) and p['kprll'].shape == (3, 2 * nchan)
        assert p['horizon_kprll_limits'].shape == (nt, 3, nbl, 2)
        fac = p['factor'].reshape(1, -1, 1, 1)
        assert NP.array_equal(p['skyvis_lag'], NP.abs(ds.subband_delay_spectra[key]['skyvis_lag']) ** 2 * fac)
        pr = dps.subband_delay_power_spectra_resampled[key]
        assert NP.array_equal(pr['vis_lag'], NP.abs(ds.subband_delay_spectra_resampled[key]['vis_lag']) ** 2 * fac)
    assert 'vis_noise_lag' in dps.subband_delay_power_spectra['sim'] and 'vis_net_lag' in dps.subband_delay_power_spectra['cc']

    # the power-only call on the resident snapshots against |complex|^2 * factor
    fw = ds.subband_delay_spectra['sim']['freq_wts']
    fac = dps.subband_delay_power_spectra['sim']['factor']
    nres = ds.subband_delay_spectra_resampled['sim']['skyvis_lag'].shape[2]
    po, pr, st = ia._ctx.subband_power_resident(0, nt, NP.asarray(ia.bp)[:, :, 0], fw, 2 * nchan, df, fac, nres=nres)
    assert st['rows'] == nt * nbl
    want_o = NP.abs(ds.subband_delay_spectra['sim']['skyvis_lag']) ** 2 * fac.reshape(1, -1, 1, 1)
    want_r = NP.abs(ds.subband_delay_spectra_resampled['sim']['skyvis_lag']) ** 2 * fac.reshape(1, -1, 1, 1)
    assert NP.max(NP.abs(NP.transpose(po, (1, 2, 3, 0)) - want_o)) <= 1e-12 * NP.max(want_o)
    assert NP.max(NP.abs(NP.transpose(pr, (1, 2, 3, 0)) - want_r)) <= 1e-12 * NP.max(want_o)
