"""CPU: delay spectra and power spectra of stacks of runs (DelaySpectrum.delay_transform_allruns, subband_delay_transform_allruns,
DelayPowerSpectrum.compute_power_spectrum_allruns).  The reference's fixtures (tests/golden/golden_allruns.npz) against the numpy
restatement of the device entries (tests/allruns_checker.py), the methods on a stand-in context against the fixtures, the argument
checks, every literal quirk and departure, and a build guard on the kernels' registers."""
import json
import os
import shutil
import subprocess
import sys
import types

import numpy as NP
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import allruns_checker as CK  # noqa: E402

from prisim_amd import _abi, delay_spectrum as DS, dsp_readings as D  # noqa: E402

GOLD = os.path.join(HERE, 'golden', 'golden_allruns.npz')
DF = 97.65625e3
JACOBIAN1, JACOBIAN2, JY2K = 2.5e-3, 7.1e7, 3.3e-3


def beam3dvol_standin(freq_wts=None):
    return 1e-2 * NP.sum(NP.atleast_2d(NP.asarray(freq_wts, dtype=NP.float64)) ** 2, axis=-1) + 0.5


def make_ds(f, bp, bp_wts, ctx=None):
    """A DelaySpectrum over a stand-in array (baselines, channels, bp, bp_wts) whose context is ``ctx`` (default: the numpy stand-in)."""
    nbl, nchan, nt = bp.shape
    ia = types.SimpleNamespace(baselines=NP.zeros((nbl, 3)), channels=f, freq_resolution=DF, n_acc=nt, bp=bp, bp_wts=bp_wts, _stacks={},
                               _ctx=ctx if ctx is not None else CK.StandinRunsContext())
    ds = DS.DelaySpectrum.__new__(DS.DelaySpectrum)
    ds.ia, ds.f, ds.df, ds.n_acc = ia, f, DF, nt
    ds._bp_wts_override = None
    return ds


def make_dps(ds):
    dps = DS.DelayPowerSpectrum.__new__(DS.DelayPowerSpectrum)
    dps.ds, dps.cosmo = ds, DS.cosmo100
    dps.jacobian1, dps.jacobian2, dps.Jy2K = NP.float64(JACOBIAN1), NP.float64(JACOBIAN2), NP.float64(JY2K)
    dps.beam3Dvol = beam3dvol_standin
    return dps


def rel_err(a, b):
    scale = max(NP.max(NP.abs(b)), 1e-300)
    return NP.max(NP.abs(NP.asarray(a) - NP.asarray(b))) / scale


def full_case(g, i):
    pre = 'f%d_' % i
    p = json.loads(str(g[pre + 'params']))
    fw = g[pre + 'in_freq_wts'] if pre + 'in_freq_wts' in g.files else None
    return p, g[pre + 'in_vis'], g[pre + 'in_bp'], g[pre + 'in_bp_wts'], g[pre + 'in_f'], fw


def sub_case(g, i):
    pre = 's%d_' % i
    return (json.loads(str(g[pre + 'params'])), g[pre + 'in_vis'], g[pre + 'in_bp'], g[pre + 'in_bp_wts'], g[pre + 'in_f'],
            g[pre + 'in_bw_eff'], g[pre + 'in_freq_center'])


def run_full(g, i, ctx=None):
    p, vis, bp, bpw, f, fw = full_case(g, i)
    ds = make_ds(f, bp, bpw, ctx)
    return ds.delay_transform_allruns(vis, pad=p['pad'], freq_wts=fw, downsample=p['downsample'], verbose=False)


def run_sub(g, i, ctx=None):
    p, vis, bp, bpw, f, bw, fc = sub_case(g, i)
    ds = make_ds(f, bp, bpw, ctx)
    return ds.subband_delay_transform_allruns(vis, bw, freq_center=fc, shape=p['shape'], pad=p['pad'], action=p['action'], verbose=False)


def power_case(g, i):
    pre = 'p%d_' % i
    p = json.loads(str(g[pre + 'params']))
    dspec = {k[len(pre) + 3:]: g[k] for k in g.files if k.startswith(pre + 'in_')}
    return p, dspec, g[pre + 'out_' + ('subband' if p['subband'] else 'fullband')]


# ---- the fixtures against the numpy restatement of the entries -----------------------------------------------------------------------
def test_fixtures_cover_the_cases_the_issue_lists():
    g = NP.load(GOLD)
    fp = [json.loads(str(g['f%d_params' % i])) for i in range(int(g['nfull']))]
    assert {len(p['lead']) + 3 for p in fp} == {3, 4, 5}
    assert {p['pad'] for p in fp} >= {0.0, 0.5, 1.0} and {p['downsample'] for p in fp} == {True, False}
    assert {p['nt'] for p in fp} >= {1, 2} and any(p['nchan'] & (p['nchan'] - 1) for p in fp) and any(p['nchan'] == 32 for p in fp)
    assert {p['form'] for p in fp} >= {None, 'f', 'ft', 'bf', 'bft', 'vis'}
    sp = [json.loads(str(g['s%d_params' % i])) for i in range(int(g['nsub']))]
    assert None in [p['action'] for p in sp] and len({p['action'] for p in sp}) >= 3
    pp = [json.loads(str(g['p%d_params' % i])) for i in range(int(g['npow']))]
    assert {(p['subband'], p['cross']) for p in pp} == {(False, False), (False, True), (True, False), (True, True)}


def test_fixtures_against_the_checker():
    """The reference's outputs are the entries' contract: scale fftshift(ifft(.)) of the weighted rows, then the lag selection."""
    g = NP.load(GOLD)
    for i in range(int(g['nfull'])):
        p, vis, bp, bpw, f, fw = full_case(g, i)
        if 'f%d_raises' % i in g.files:
            continue
        nbl, nchan, nt = bp.shape
        pad = max(p['pad'], 0.0)
        m = nchan + int(nchan * pad)
        rep = g['f%d_out_freq_wts' % i]                                 # the weights as the reference reshaped them
        w = NP.broadcast_to(rep.reshape(rep.shape[-3:]) if rep.ndim > 3 else rep, (nbl, nchan, nt))
        kw = dict(m=m, scale=m * DF, mode='interp' if p['downsample'] else 'all', factor=1 + pad, nout=NP.arange(0, m, 1 + pad).size)
        got = CK.transform(vis, nbl, nchan, nt, bp=bp, wts=w, **kw)[0].reshape(g['f%d_out_vis_lag' % i].shape)
        assert rel_err(got, g['f%d_out_vis_lag' % i]) <= 1e-13, i
    for i in range(int(g['npow'])):
        p, dspec, want = power_case(g, i)
        assert want.dtype == NP.float64


# ---- the methods on the stand-in context against the fixtures ------------------------------------------------------------------------
def test_delay_transform_allruns_against_the_fixtures():
    g = NP.load(GOLD)
    for i in range(int(g['nfull'])):
        pre = 'f%d_' % i
        if pre + 'raises' in g.files:
            with pytest.raises(getattr(__builtins__, str(g[pre + 'raises'])) if isinstance(__builtins__, types.ModuleType)
                               else __builtins__[str(g[pre + 'raises'])]):
                run_full(g, i)
            continue
        res = run_full(g, i)
        assert set(res) == {'freq_wts', 'pad', 'lags', 'vis_lag', 'lag_kernel'}
        for key in ('vis_lag', 'lag_kernel'):
            assert res[key].shape == g[pre + 'out_' + key].shape, (i, key)
            assert rel_err(res[key], g[pre + 'out_' + key]) <= 1e-12, (i, key)
        assert NP.array_equal(res['lags'], g[pre + 'out_lags']), i
        assert NP.array_equal(NP.asarray(res['freq_wts']), g[pre + 'out_freq_wts']) and res['freq_wts'].shape == g[pre + 'out_freq_wts'].shape
        assert res['pad'] == float(g[pre + 'out_pad'])


def test_subband_delay_transform_allruns_against_the_fixtures():
    g = NP.load(GOLD)
    for i in range(int(g['nsub'])):
        pre = 's%d_' % i
        if pre + 'raises' in g.files:
            with pytest.raises(ValueError, match='Invalid value specified for keyword input action'):
                run_sub(g, i)
            continue
        res = run_sub(g, i)
        want = {k[len(pre) + 4:] for k in g.files if k.startswith(pre + 'out_')}
        assert set(res) == want
        for key in ('vis_lag', 'lag_kernel'):
            assert res[key].shape == g[pre + 'out_' + key].shape, (i, key)
            assert rel_err(res[key], g[pre + 'out_' + key]) <= 1e-12, (i, key)
        for key in ('freq_center', 'freq_wts', 'bw_eff', 'npad', 'lags', 'lag_corr_length'):
            assert NP.allclose(res[key], g[pre + 'out_' + key], rtol=1e-14, atol=0), (i, key)
            assert NP.shape(res[key]) == g[pre + 'out_' + key].shape, (i, key)
        assert res['shape'] == str(g[pre + 'out_shape'])


def test_compute_power_spectrum_allruns_against_the_fixtures_bit_for_bit():
    g = NP.load(GOLD)
    same_numpy = list(g['numpy_fused']) == [_abi.numpy_fuses_complex_product(NP.complex128), _abi.numpy_fuses_complex_product(NP.complex64)]
    for i in range(int(g['npow'])):
        p, dspec, want = power_case(g, i)
        dps = make_dps(make_ds(150e6 + DF * NP.arange(24), NP.ones((1, 24, 1)), NP.ones((1, 24, 1))))
        res = dps.compute_power_spectrum_allruns(dict(dspec), subband=p['subband'])
        key = 'subband' if p['subband'] else 'fullband'
        assert list(res) == [key] and res[key].dtype == NP.float64 and res[key].shape == want.shape
        if same_numpy:
            assert NP.array_equal(res[key], want), i
        else:
            assert rel_err(res[key], want) <= 1e-6, i


# ---- argument checks ------------------------------------------------------------------------------------------------------------------
def _small(nt=2, nbl=2, nchan=16):
    rng = NP.random.default_rng(3)
    f = 150e6 + DF * NP.arange(nchan)
    ds = make_ds(f, 0.5 + rng.uniform(size=(nbl, nchan, nt)), NP.ones((nbl, nchan, nt)))
    vis = rng.standard_normal((2, nbl, nchan, nt)) + 1j * rng.standard_normal((2, nbl, nchan, nt))
    return ds, vis


def test_argument_checks_raise_the_reference_exceptions():
    ds, vis = _small()
    ctx = ds.ia._ctx
    with pytest.raises(TypeError):
        ds.delay_transform_allruns(list(vis.ravel()), verbose=False)
    with pytest.raises(ValueError, match='at least 3-dimensional'):
        ds.delay_transform_allruns(vis[0, 0], verbose=False)
    with pytest.raises(ValueError, match='compatible shape'):
        ds.delay_transform_allruns(vis[..., :1], verbose=False)
    with pytest.raises(TypeError, match='pad'):
        ds.delay_transform_allruns(vis, pad='1', verbose=False)
    with pytest.raises(TypeError, match='downsample'):
        ds.delay_transform_allruns(vis, downsample=1, verbose=False)
    with pytest.raises(ValueError, match='window shape'):
        ds.delay_transform_allruns(vis, freq_wts=NP.ones(7), verbose=False)
    with pytest.raises(TypeError, match='effective bandwidth'):
        ds.subband_delay_transform_allruns(vis, 'wide', action='x', verbose=False)
    with pytest.raises(ValueError, match='strictly positive'):
        ds.subband_delay_transform_allruns(vis, -1.0, action='x', verbose=False)
    with pytest.raises(ValueError, match='strictly inside'):
        ds.subband_delay_transform_allruns(vis, 4 * DF, freq_center=ds.f[0], action='x', verbose=False)
    with pytest.raises(TypeError, match='frequency center'):
        ds.subband_delay_transform_allruns(vis, 4 * DF, freq_center='c', action='x', verbose=False)
    with pytest.raises(ValueError, match='same number'):
        ds.subband_delay_transform_allruns(vis, [4 * DF, 5 * DF], freq_center=ds.f[[4, 6, 8]], action='x', verbose=False)
    with pytest.raises(TypeError, match='string'):
        ds.subband_delay_transform_allruns(vis, 4 * DF, shape=3, action='x', verbose=False)
    with pytest.raises(ValueError, match='window shape'):
        ds.subband_delay_transform_allruns(vis, 4 * DF, shape='hann', action='x', verbose=False)
    with pytest.raises(ValueError, match='positive'):
        ds.subband_delay_transform_allruns(vis, 4 * DF, fftpow=-1.0, action='x', verbose=False)
    with pytest.raises(TypeError, match='pad'):
        ds.subband_delay_transform_allruns(vis, 4 * DF, pad='1', action='x', verbose=False)
    dps = make_dps(ds)
    with pytest.raises(TypeError):
        dps.compute_power_spectrum_allruns([vis])
    with pytest.raises(KeyError):
        dps.compute_power_spectrum_allruns({'vislag2': vis})
    with pytest.raises(TypeError, match='vislag1'):
        dps.compute_power_spectrum_allruns({'vislag1': list(vis.ravel())})
    with pytest.raises(TypeError, match='vislag2'):
        dps.compute_power_spectrum_allruns({'vislag1': vis, 'vislag2': 1.0})
    with pytest.raises(ValueError, match='same shape'):
        dps.compute_power_spectrum_allruns({'vislag1': vis, 'vislag2': vis[:1]})
    with pytest.raises(TypeError, match='boolean'):
        dps.compute_power_spectrum_allruns({'vislag1': vis}, subband=1)
    assert ctx.calls == []                            # every check comes before any device work


# ---- literal quirks -------------------------------------------------------------------------------------------------------------------
def test_quirk_freq_wts_of_the_vis_shape_raises():
    ds, vis = _small()
    with pytest.raises(ValueError, match='tiemstamps'):
        ds.delay_transform_allruns(vis, freq_wts=NP.ones(vis.shape), verbose=False)


def test_quirk_any_action_returns_the_resampled_dictionary():
    ds, vis = _small(nchan=32)
    a = ds.subband_delay_transform_allruns(vis, 4 * DF, freq_center=ds.f[16], action='return_oversampled', verbose=False)
    b = ds.subband_delay_transform_allruns(vis, 4 * DF, freq_center=ds.f[16], action='whatever', verbose=False)
    m = 64
    assert a['vis_lag'].shape[-2] == D.fft_downsample_length(m, m * DF / (4 * DF)) != m
    assert NP.array_equal(a['vis_lag'], b['vis_lag']) and 'lag_corr_length' in a
    assert [c[2] for c in ds.ia._ctx.calls] == ['resample', 'interp'] * 2     # the oversampled spectra are never formed


def test_quirk_negative_pad_is_reset_to_zero():
    ds, vis = _small()
    res = ds.delay_transform_allruns(vis, pad=-0.5, verbose=False)
    assert res['pad'] == 0.0 and res['vis_lag'].shape[-2] == ds.f.size


def test_quirk_lag_kernel_has_leading_axes_of_one_and_is_formed_once():
    ds, vis = _small()
    vis5 = NP.stack([vis, vis, vis])
    res = ds.delay_transform_allruns(vis5, pad=1.0, verbose=False)
    assert res['lag_kernel'].shape == (1, 1) + res['vis_lag'].shape[2:]
    assert [c[1] for c in ds.ia._ctx.calls] == [vis5.shape, None]


# ---- departures -----------------------------------------------------------------------------------------------------------------------
def test_departure_weights_varying_per_run_raise_not_implemented():
    ds, vis = _small()
    with pytest.raises(NotImplementedError, match='vary from run to run'):
        ds.delay_transform_allruns(vis, freq_wts=NP.ones((2, 1, ds.f.size, 1)), verbose=False)


def test_departure_weights_broadcasting_over_trailing_axes_are_taken():
    ds, vis = _small()
    w = 0.5 + NP.arange(ds.f.size, dtype=float).reshape(1, -1, 1) / ds.f.size
    res = ds.delay_transform_allruns(vis, freq_wts=w, pad=1.0, verbose=False)
    want = ds.delay_transform_allruns(vis, freq_wts=w[0, :, 0], pad=1.0, verbose=False)
    assert NP.allclose(res['vis_lag'], want['vis_lag'], rtol=0, atol=1e-12 * NP.max(NP.abs(want['vis_lag'])))
    assert res['freq_wts'] is not None and res['freq_wts'].shape == w.shape


def test_departure_action_none_raises_before_any_device_work():
    ds, vis = _small()
    with pytest.raises(ValueError, match='Invalid value specified for keyword input action'):
        ds.subband_delay_transform_allruns(vis, 4 * DF, freq_center=ds.f[8], verbose=False)
    assert ds.ia._ctx.calls == []


def test_departure_default_freq_center_is_the_middle_channel():
    ds, vis = _small(nchan=17)
    res = ds.subband_delay_transform_allruns(vis, 4 * DF, action='x', verbose=False)
    assert NP.array_equal(res['freq_center'], [ds.f[8]])


def test_departure_fftpow_other_than_one_is_not_implemented():
    ds, vis = _small()
    with pytest.raises(NotImplementedError):
        ds.subband_delay_transform_allruns(vis, 4 * DF, freq_center=ds.f[8], fftpow=2.0, action='x', verbose=False)


def test_departure_caller_dspec_is_left_unmodified():
    ds, vis = _small()
    dspec = {'vislag1': vis, 'freq_center': [ds.f[8]], 'bw_eff': 4 * DF, 'freq_wts': NP.ones((1, ds.f.size)), 'lags': NP.arange(16)}
    before = dict(dspec)
    make_dps(ds).compute_power_spectrum_allruns(dspec, subband=True)
    assert set(dspec) == set(before) and all(dspec[k] is before[k] for k in dspec)


def test_departure_spectra_above_the_length_limit_raise_before_device_work():
    nchan = 2100
    ds, vis = _small(nt=1, nbl=1, nchan=nchan)
    with pytest.raises(ValueError, match='PRISIM_SUBBAND_MAX_LEN'):
        ds.delay_transform_allruns(vis, pad=1.0, verbose=False)
    with pytest.raises(ValueError, match='PRISIM_SUBBAND_MAX_LEN'):
        ds.subband_delay_transform_allruns(vis, 40 * DF, freq_center=ds.f[1000], pad=1.0, action='x', verbose=False)
    assert ds.ia._ctx.calls == []


def test_methods_set_nothing_on_self_and_leave_inputs_alone():
    ds, vis = _small()
    v0, w = vis.copy(), NP.ones(ds.f.size)
    before = dict(vars(ds))
    ds.delay_transform_allruns(vis, freq_wts=w, verbose=False)
    ds.subband_delay_transform_allruns(vis, 4 * DF, freq_center=ds.f[8], action='x', verbose=False)
    assert set(vars(ds)) == set(before) and all(vars(ds)[k] is before[k] for k in before)
    assert NP.array_equal(vis, v0) and NP.array_equal(w, NP.ones(ds.f.size))


def test_numpy_complex_product_probe_matches_numpy():
    """The rounding the power entry is told to use reproduces numpy's own product on random data of both precisions."""
    rng = NP.random.default_rng(5)
    for dt, rt in ((NP.complex128, NP.float64), (NP.complex64, NP.float32)):
        a = (rng.standard_normal(4096) + 1j * rng.standard_normal(4096)).astype(dt)
        b = (rng.standard_normal(4096) + 1j * rng.standard_normal(4096)).astype(dt)
        p = (a * b.conj()).real
        plain = a.real * b.real + a.imag * b.imag
        if _abi.numpy_fuses_complex_product(dt):
            assert not NP.array_equal(p, plain)
        else:
            assert NP.array_equal(p, plain)
        assert p.dtype == rt


# ---- build guard ----------------------------------------------------------------------------------------------------------------------
def test_runs_kernels_use_no_scratch_and_do_not_spill(tmp_path):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    src = os.path.join(ROOT, 'prisim_amd', 'csrc_runs', 'runs.hip')
    out = tmp_path / 'runs.s'
    res = subprocess.run([hipcc, '-O3', '-std=c++17', '--offload-arch=gfx950', '-I/opt/rocm/include', '-ffp-contract=off', '-S',
                          '--cuda-device-only', src, '-o', str(out)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_meta as KM
    rows = [r for r in KM.kernel_meta(out.read_text()) if 'k_runs_' in r['name']]
    assert len(rows) == 6
    for r in rows:
        assert r['scratch'] == 0 and r['vgpr_spill'] == 0 and r['sgpr_spill'] == 0, r
