"""CPU: sub-band delay spectra -- the astroutils readings (prisim_amd/dsp_readings.py) by known answers, the numpy checker against the
reference's fixtures (tests/golden/golden_subband.npz), and DelaySpectrum.subband_delay_transform's host logic on a stand-in context:
argument checks, the reference's literal behaviours, the departures, validate-then-commit."""
import json
import os
import sys

import numpy as NP
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import subband_checker as CK  # noqa: E402
import subband_standin as SI  # noqa: E402

from prisim_amd import delay_spectrum as DS, dsp_readings as D  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'golden_subband.npz')
ARGS = dict(bw_eff={'cc': 4 * 97.65625e3, 'sim': 4 * 97.65625e3}, verbose=False)


# ---- the readings ----
@pytest.mark.parametrize('shape,width', [('rect', 1.0), ('bhw', 0.2579634), ('bnw', 0.2612254)])
def test_window_N2width_known_answers(shape, width):
    assert abs(D.window_N2width(shape=shape) - width) < 5e-8
    assert D.window_N2width(shape=shape.upper()) == D.window_N2width(shape=shape)


def test_window_coefficients_and_symmetry():
    n = NP.arange(9)
    a = (0.35875, 0.48829, 0.14128, 0.01168)
    want = a[0] - a[1] * NP.cos(2 * NP.pi * n / 8) + a[2] * NP.cos(4 * NP.pi * n / 8) - a[3] * NP.cos(6 * NP.pi * n / 8)
    assert NP.allclose(D.windowing(9, 'bhw', power_normalize=False), want, rtol=0, atol=1e-15)
    w = D.windowing(9, 'bnw', power_normalize=False)
    assert NP.allclose(w, w[::-1], rtol=0, atol=1e-15) and abs(w[4] - 1.0) < 1e-6
    assert NP.array_equal(D.windowing(7, 'rect', power_normalize=False), NP.ones(7))
    assert abs(NP.sum(D.windowing(50, 'bhw') ** 2) - 1.0) < 1e-14


@pytest.mark.parametrize('shape', ['bhw', 'bnw'])
def test_even_windows_lead_with_a_zero_and_peak_at_n_over_2(shape):
    for n in (6, 10, 64):
        w = D.windowing(n, shape, power_normalize=False)
        assert w[0] == 0.0 and int(NP.argmax(w)) == n // 2
        assert NP.allclose(w[1:], D.windowing(n - 1, shape, power_normalize=False), rtol=0, atol=0)
    assert int(NP.argmax(D.windowing(11, shape))) == 5


@pytest.mark.parametrize('shape', ['rect', 'bhw', 'bnw'])
def test_reference_window_has_unit_peak_and_effective_bandwidth(shape):
    df = 97.65625e3
    fw = D.window_N2width(shape=shape)
    for bw_eff in (10 * df, 37.3 * df, 200 * df):
        n = int(NP.round(bw_eff / fw / df))
        w = NP.sqrt(fw * n) * D.window_fftpow(n, shape=shape, fftpow=1.0)       # :2166
        assert abs(w.max() - 1.0) < (0.06 if n < 60 else 0.02)
        assert abs(NP.sum(w ** 2) * df - bw_eff) <= 0.5 * fw * df + 1e-6 * bw_eff


def test_fftpow_other_than_one_is_not_read():
    with pytest.raises(NotImplementedError, match='window_fftpow'):
        D.window_fftpow(16, 'bhw', fftpow=2.0)
    with pytest.raises(NotImplementedError, match='window_N2width'):
        D.window_N2width(shape='bhw', fftpow=0.5)


def test_find_1NN_ties_go_low_and_out_of_band_points_drop():
    ref = NP.arange(5.0)
    iq, ir, d = D.find_1NN(ref, NP.array([-0.6, 0.5, 2.2, 3.5, 4.5, 4.6]), distance_ULIM=0.5)
    assert iq.tolist() == [1, 2, 3, 4] and ir.tolist() == [0, 2, 3, 4]
    assert NP.allclose(d, [0.5, 0.2, 0.5, 0.5])


def test_resample_restatement_matches_scipy():
    signal = pytest.importorskip('scipy.signal')
    rng = NP.random.default_rng(3)
    for nx in (7, 8, 31, 64, 101):
        for num in (1, 2, 3, 5, 8, 13, 50, 64, 99, 128, 201):
            x = rng.normal(size=(2, nx, 3)) + 1j * rng.normal(size=(2, nx, 3))
            assert NP.max(NP.abs(D.resample(x, num, axis=1) - signal.resample(x, num, axis=1))) < 1e-12, (nx, num)
            assert D.downsampler(x, nx / float(num), axis=1, method='FFT').shape[1] == D.fft_downsample_length(nx, nx / float(num))


def test_finding_fft_resampling_of_an_off_centre_subband_is_near_zero():
    """The documented finding: the FFT of fftshift(ifft(x_pad)) M df keeps x_pad's lowest and highest bins, so resampling
    a sub-band spectrum whose window is away from channel 0 leaves rounding noise."""
    nchan, df = 256, 1.0
    m = 2 * nchan
    rng = NP.random.default_rng(5)
    x = rng.normal(size=nchan) + 1j * rng.normal(size=nchan)
    peaks = {}
    for centre in (128, 100, 40):
        n = 60
        w = NP.zeros(nchan)
        w[centre - n // 2:centre - n // 2 + n] = D.windowing(n, 'bhw')
        xp = NP.zeros(m, dtype=complex)
        xp[:nchan] = x * w
        over = NP.fft.fftshift(NP.fft.ifft(xp)) * m * df
        # the identity the device uses
        k = NP.arange(m)
        assert NP.allclose(NP.fft.fft(over), m * df * NP.exp(-2j * NP.pi * k * (m // 2) / m) * xp, rtol=0, atol=1e-9 * m)
        peaks[centre] = (NP.abs(over).max(), NP.abs(D.downsampler(over, 8.0, method='FFT')).max())
    assert peaks[128][1] < 1e-12 * peaks[128][0]                  # nothing left of a centred window
    assert peaks[100][1] < 1e-12 * peaks[100][0]                  # nor of one whose channels (70 ... 129) miss bins 0 ... 32
    assert peaks[40][1] > 0.01 * peaks[40][0]                     # a window over channels 10 ... 69 keeps the part on bins 10 ... 32


# ---- the checker against the reference's fixtures ----
def _fixture_case(g, i):
    pre = 'c%d_' % i
    p = json.loads(str(g[pre + 'params']))
    cubes = {'sim': {'skyvis': g[pre + 'skyvis_freq'], 'vis': g[pre + 'vis_freq'], 'vis_noise': g[pre + 'vis_noise_freq']}}
    if p['with_cc']:
        cubes['cc'] = {n: g[pre + 'cc_%s_freq' % n] for n in ('skyvis', 'vis', 'skyvis_res', 'vis_res', 'skyvis_net', 'vis_net')}
    return p, cubes


def test_checker_against_reference_fixtures():
    g = NP.load(GOLD)
    for i in range(int(g['n'])):
        p, cubes = _fixture_case(g, i)
        pre = 'c%d_' % i
        res, rres = CK.subband(g[pre + 'f'], p['df'], cubes, g[pre + 'bp'], {k: NP.asarray(v) for k, v in p['bw_eff'].items()},
                               {k: NP.asarray(v) for k, v in p['freq_center'].items()}, p['shape'], p['pad'])
        for tag, out in (('o', res), ('r', rres)):
            for key, d in out.items():
                for field, v in d.items():
                    name = '%s%s_%s_%s' % (pre, tag, key, field)
                    if field == 'shape':
                        continue
                    want = g[name]
                    assert NP.shape(v) == want.shape, name
                    if field.endswith('_lag') or field == 'lag_kernel':
                        ref = None if tag == 'o' else res[key][field]
                        assert CK.rel_err(v, want, scale_of=ref) <= 1e-12, name
                    else:
                        assert NP.allclose(v, want, rtol=1e-13, atol=0), name


# ---- the method's host logic on a stand-in context ----
def test_method_matches_the_checker_on_the_standin():
    ds = SI.add_clean(SI.make_ds(nchan=40, nt=3))
    fc = {'cc': ds.f[[30, 8]], 'sim': ds.f[[25, 12, 3]]}
    bw = {'cc': NP.array([3.0, 5.0]) * ds.df, 'sim': 4.0 * ds.df}
    out = ds.subband_delay_transform(bw, freq_center=fc, shape={'cc': 'bnw', 'sim': 'bhw'}, pad={'cc': 0.5, 'sim': 1.0},
                                     action='return_oversampled', verbose=False)
    cubes = {'sim': {'skyvis': ds.ia.skyvis_freq, 'vis': ds.ia.vis_freq, 'vis_noise': ds.ia.vis_noise_freq},
             'cc': {n: getattr(ds, 'cc_%s_freq' % n) for n in ('skyvis', 'vis', 'skyvis_res', 'vis_res', 'skyvis_net', 'vis_net')}}
    res, rres = CK.subband(ds.f, ds.df, cubes, ds.ia.bp, {'cc': bw['cc'], 'sim': NP.repeat(4.0 * ds.df, 3)}, fc,
                           {'cc': 'bnw', 'sim': 'bhw'}, {'cc': 0.5, 'sim': 1.0})
    assert out is ds.subband_delay_spectra
    for key in ('cc', 'sim'):
        for name, v in res[key].items():
            if name.endswith('_lag') or name == 'lag_kernel':
                assert CK.rel_err(out[key][name], v) <= 1e-12, (key, name)
                assert CK.rel_err(ds.subband_delay_spectra_resampled[key][name], rres[key][name], scale_of=v) <= 1e-12, (key, name)
        assert NP.array_equal(ds.subband_delay_spectra_resampled[key]['lags'], rres[key]['lags'])


def test_argument_checks_raise_the_reference_exceptions():
    ds = SI.make_ds()
    bw = ARGS['bw_eff']
    for kw, exc in ((dict(bw_eff=5.0), TypeError), (dict(bw_eff={'cc': 'x', 'sim': 1.0}), TypeError),
                    (dict(bw_eff={'cc': 1.0, 'sim': -1.0}), ValueError), (dict(bw_eff={'sim': 1e5}), KeyError),
                    (dict(bw_eff=bw, freq_center=1.5e8), TypeError), (dict(bw_eff=bw, freq_center={'sim': ds.f[5]}), KeyError),
                    (dict(bw_eff=bw, freq_center={'cc': ds.f[5], 'sim': 'a'}), TypeError),
                    (dict(bw_eff=bw, freq_center={'cc': ds.f[0], 'sim': ds.f[5]}), ValueError),
                    (dict(bw_eff={'cc': [1e5, 2e5], 'sim': [1e5, 2e5]}, freq_center={'cc': ds.f[[3, 4, 5]], 'sim': ds.f[4]}), ValueError),
                    (dict(bw_eff=bw, shape='bhw'), TypeError), (dict(bw_eff=bw, shape={'cc': 'bhw', 'sim': 3}), TypeError),
                    (dict(bw_eff=bw, shape={'cc': 'bhw', 'sim': 'hann'}), ValueError), (dict(bw_eff=bw, shape={'sim': 'bhw'}), KeyError),
                    (dict(bw_eff=bw, fftpow=1.0), TypeError), (dict(bw_eff=bw, fftpow={'cc': 1.0, 'sim': 'a'}), TypeError),
                    (dict(bw_eff=bw, fftpow={'cc': 1.0, 'sim': -1.0}), ValueError),
                    (dict(bw_eff=bw, fftpow={'cc': 1.0, 'sim': 2.0}), NotImplementedError),
                    (dict(bw_eff=bw, pad=1.0), TypeError), (dict(bw_eff=bw, pad={'cc': 1.0, 'sim': '1'}), TypeError),
                    (dict(bw_eff=bw, bpcorrect=1), TypeError)):
        with pytest.raises(exc):
            ds.subband_delay_transform(verbose=False, **kw)
        assert ds.subband_delay_spectra == {} and ds.subband_delay_spectra_resampled == {}


def test_windows_sorted_by_channel_centres_kept_in_given_order():
    ds = SI.make_ds(nchan=48)
    fc = ds.f[[40, 6, 22]]
    bw = NP.array([3.0, 5.0, 4.0]) * ds.df
    out = ds.subband_delay_transform({'cc': 1e5, 'sim': bw}, freq_center={'cc': ds.f[20], 'sim': fc}, shape={'cc': 'rect', 'sim': 'rect'},
                                     action='return_oversampled', verbose=False)['sim']
    assert NP.array_equal(out['freq_center'], fc) and NP.array_equal(out['bw_eff'], bw)
    peaks = [int(NP.argmax(w)) for w in out['freq_wts']]
    assert peaks == sorted(peaks)
    widths = [int(NP.count_nonzero(w)) for w in out['freq_wts']]
    assert widths == [5, 4, 3]                                     # n_window follows the sort (6 -> 5, 22 -> 4, 40 -> 3 channels)


def test_windows_truncated_at_both_band_edges():
    ds = SI.make_ds(nchan=40)
    fw = DS.subband_freq_wts(ds.f, ds.df, NP.array([6.0, 6.0]) * ds.df, ds.f[[1, 38]], 'bhw', 1.0)
    full = NP.sqrt(D.window_N2width(shape='bhw') * 23) * D.windowing(23, 'bhw')
    assert fw[0, 0] == full[10] and NP.count_nonzero(fw[0]) == 13          # samples 10 ... 22 of the 23 land on channels 0 ... 12
    assert fw[1, 39] == full[12] and NP.all(fw[1, :27] == 0.0)


def test_resampling_factor_uses_the_npad_of_the_last_key():
    ds = SI.add_clean(SI.make_ds(nchan=32))
    bw = {'cc': 4 * ds.df, 'sim': 4 * ds.df}
    ds.subband_delay_transform(bw, pad={'cc': 0.5, 'sim': 2.0}, verbose=False)
    m_cc, m_sim = 32 + 16, 32 + 64
    factor = m_sim * ds.df / (4 * ds.df)                          # sim's npad, also for 'cc' (:2225)
    r = ds.subband_delay_spectra_resampled
    assert r['cc']['skyvis_lag'].shape[2] == int(round(m_cc / factor)) == 2
    assert r['sim']['skyvis_lag'].shape[2] == int(round(m_sim / factor))
    assert r['cc']['lags'].size == int(NP.ceil(m_cc / factor))


def test_interp_lags_and_fft_spectra_can_differ_in_length():
    ds = SI.make_ds(nchan=30)
    ds.subband_delay_transform({'cc': 1e5, 'sim': 7.3 * ds.df}, pad={'cc': 1.0, 'sim': 1.0}, verbose=False)
    r = ds.subband_delay_spectra_resampled['sim']
    factor = 60 * ds.df / (7.3 * ds.df)
    assert r['lags'].size == int(NP.ceil(60 / factor)) == 8
    assert r['skyvis_lag'].shape[2] == int(round(60 / factor)) == 7
    assert r['lag_kernel'].shape[2] == r['lags'].size


def test_lag_corr_length_both_ways():
    ds = SI.make_ds(nchan=32)
    ds.subband_delay_transform({'cc': 1e5, 'sim': [3 * ds.df, 6 * ds.df]}, freq_center={'cc': ds.f[9], 'sim': ds.f[[9, 20]]},
                               shape={'cc': 'rect', 'sim': 'bnw'}, verbose=False)
    o, r = ds.subband_delay_spectra['sim'], ds.subband_delay_spectra_resampled['sim']
    assert NP.array_equal(o['lag_corr_length'], 32 / NP.sum(o['freq_wts'], axis=1))
    assert NP.allclose(r['lag_corr_length'], (1 / o['bw_eff']) / (r['lags'][1] - r['lags'][0]), rtol=1e-15)


def test_bpcorrect_is_recorded_and_has_no_effect():
    out = {}
    for flag in (False, True):
        ds = SI.add_clean(SI.make_ds())
        ds.subband_delay_transform(ARGS['bw_eff'], bpcorrect=flag, verbose=False)
        out[flag] = ds.subband_delay_spectra['cc']
        assert out[flag]['bpcorrect'] is flag
    for name in ('skyvis_lag', 'vis_lag', 'skyvis_res_lag', 'vis_res_lag', 'skyvis_net_lag', 'vis_net_lag'):
        assert NP.array_equal(out[False][name], out[True][name])


def test_cc_key_only_after_clean():
    ds = SI.make_ds()
    ds.subband_delay_transform(ARGS['bw_eff'], verbose=False)
    assert list(ds.subband_delay_spectra) == ['sim'] and list(ds.subband_delay_spectra_resampled) == ['sim']
    SI.add_clean(ds)
    ds.subband_delay_transform(ARGS['bw_eff'], verbose=False)
    assert sorted(ds.subband_delay_spectra) == ['cc', 'sim']
    assert 'vis_noise_lag' in ds.subband_delay_spectra['sim'] and 'vis_res_lag' in ds.subband_delay_spectra['cc']


def test_departure_default_freq_center_is_the_integer_middle_channel():
    ds = SI.make_ds(nchan=33)
    out = ds.subband_delay_transform(ARGS['bw_eff'], action='return_oversampled', verbose=False)['sim']
    assert NP.array_equal(out['freq_center'], [ds.f[16]])
    assert NP.flatnonzero(out['freq_wts'][0]).tolist() == [14, 15, 16, 17]       # 4 channels from 16 - int(4 / 2)


def test_departure_noiseless_array_gives_none():
    ds = SI.make_ds(noise=False)
    r = ds.subband_delay_transform(ARGS['bw_eff'], action='return_resampled', verbose=False)['sim']
    assert r['vis_lag'] is None and r['vis_noise_lag'] is None and r['skyvis_lag'] is not None
    assert ds.subband_delay_spectra['sim']['vis_noise_lag'] is None


def test_departure_caller_dictionaries_are_left_alone():
    ds = SI.make_ds()
    bw, pad = {'cc': 1e5, 'sim': 2e5}, {'cc': -1.0, 'sim': 1.0}
    ds.subband_delay_transform(bw, pad=pad, verbose=False)
    assert bw == {'cc': 1e5, 'sim': 2e5} and pad == {'cc': -1.0, 'sim': 1.0}


def test_action_returns_and_always_stores():
    ds = SI.make_ds()
    assert ds.subband_delay_transform(ARGS['bw_eff'], verbose=False) is None
    r = ds.subband_delay_transform(ARGS['bw_eff'], action='return_resampled', verbose=False)
    assert r is ds.subband_delay_spectra_resampled
    assert ds.subband_delay_spectra['sim']['skyvis_lag'].shape == (3, 1, 64, 2)


def test_failed_call_changes_no_attribute():
    ds = SI.add_clean(SI.make_ds())
    ds.subband_delay_transform(ARGS['bw_eff'], verbose=False)
    before = (ds.subband_delay_spectra, ds.subband_delay_spectra_resampled, dict(vars(ds)))
    ds.ia._ctx = SI.StandinContext(fail_after=2)                  # the 'cc' key's transforms pass, the 'sim' key's fail
    with pytest.raises(RuntimeError, match='stand-in'):
        ds.subband_delay_transform({'cc': 2e5, 'sim': 2e5}, pad={'cc': 0.0, 'sim': 0.5}, verbose=False)
    assert ds.subband_delay_spectra is before[0] and ds.subband_delay_spectra_resampled is before[1]
    after = dict(vars(ds))
    after.pop('ia')
    want = dict(before[2])
    want.pop('ia')
    assert after.keys() == want.keys() and all(after[k] is want[k] for k in want)
    with pytest.raises(ValueError):
        ds.subband_delay_transform({'cc': 2e5, 'sim': 2e5}, pad={'cc': 1.0, 'sim': 200.0}, verbose=False)   # M over the limit
    assert ds.subband_delay_spectra is before[0]


def test_lag_kernel_transforms_each_distinct_bandpass_row_once():
    ds = SI.make_ds(nchan=32, nbl=3, nt=4)
    bp = ds.ia.bp
    bp[:, :, 2] = bp[:, :, 0]                                     # snapshots 0 and 2 share a layer; 1 and 3 differ
    out = ds.subband_delay_transform({'cc': 1e5, 'sim': 4 * ds.df}, action='return_oversampled', verbose=False)['sim']
    kern_calls = [sh for sh in ds.ia._ctx.shapes if sh[:2] == (1, 1)]
    assert kern_calls == [(1, 1, 3 * 3, 32)]                      # 3 distinct layers x 3 baselines, not 4 x 3
    want = CK.transform(NP.ones_like(bp, dtype=complex), bp, out['freq_wts'], 32, ds.df)
    assert CK.rel_err(out['lag_kernel'], want) <= 1e-12
