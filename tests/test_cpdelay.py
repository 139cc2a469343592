"""CPU: the host logic of DelaySpectrum.subband_delay_transform_closure_phase and of the closure-phase power spectra of
DelayPowerSpectrum on stand-ins (tests/cpdelay_standin.py), against tests/golden/golden_cpdelay.npz (the reference's statements
executed, tests/golden/make_golden_cpdelay.py); the numpy checker against the same fixture; every exception, literal quirk and
departure the docstrings list; the ctypes mirror of prisim_cpdelay_stats against the compiled header.

Bound of the spectra: 1e-12 of df * sum_ch wts[w][ch] (tests/test_gpu_cpdelay.py states it); on the CPU both sides are numpy FFTs."""
import json
import os
import subprocess
import types

import numpy as NP
import pytest

import cpdelay_checker as CC
import cpdelay_standin as SI
from prisim_amd import _abi
from prisim_amd import delay_spectrum as DS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = NP.load(os.path.join(ROOT, 'tests', 'golden', 'golden_cpdelay.npz'))
KEYS = ('closure_phase_skyvis', 'closure_phase_vis', 'closure_phase_noise')
BOUND = 1e-12


def params(pre):
    return json.loads(str(GOLD[pre + 'params']))


def plain_ds(f, df, ctx=None):
    ds = DS.DelaySpectrum.__new__(DS.DelaySpectrum)
    ds.f, ds.df = f, df
    ds.ia = types.SimpleNamespace(_ctx=ctx if ctx is not None else SI.StandinContext())
    return ds


def case(i):
    pre = 'c%d_' % i
    p = params(pre)
    f = 150e6 + p['df'] * NP.arange(p['nchan'])
    ntrip = p['lead'][0]
    cpinfo = {key: GOLD[pre + 'in_' + key] for key in KEYS}
    cpinfo['antenna_triplets'] = [(str(a), str(a + 1), str(a + 2)) for a in range(ntrip)]
    cpinfo['baseline_triplets'] = list(GOLD[pre + 'in_baseline_triplets'])
    kw = {'freq_center': NP.asarray(p['freq_center']), 'shape': p['shape'], 'fftpow': 1.0, 'pad': p['pad'], 'verbose': False}
    return pre, p, f, cpinfo, NP.asarray(p['bw_eff']), kw


def compare(d, pre, wts, df):
    assert sorted(d.keys()) == GOLD[pre + 'keys'].tolist()
    for k, v in d.items():
        if k in ('antenna_triplets', 'baseline_triplets'):
            continue
        ref = GOLD[pre + k]
        if k == 'shape':
            assert v == str(ref)
        elif k in KEYS:
            assert v.shape == ref.shape and v.dtype == NP.complex128, k
            err = CC.spectrum_error(v, ref, wts, df)
            print(pre, k, 'error %.3e of df sum wts' % err)
            assert err <= BOUND, (pre, k, err)
        elif k == 'lag_kernel':
            assert v.shape == ref.shape and NP.max(NP.abs(v - ref)) <= BOUND * NP.max(CC.scale_of(wts, df)), k
        else:
            assert NP.shape(v) == ref.shape and NP.allclose(v, ref, rtol=1e-13, atol=0.0), k


@pytest.mark.parametrize('i', [0, 1, 2])
def test_checker_equals_the_reference(i):
    pre, p, f, cpinfo, bw_eff, kw = case(i)
    wts = GOLD[pre + 'o_freq_wts']
    m = GOLD[pre + 'o_lags'].size
    nres = GOLD[pre + 'r_closure_phase_skyvis'].shape[-2]
    assert m == p['nchan'] + int(p['nchan'] * p['pad'])
    for key in KEYS:
        over, res = CC.delay_spectra(cpinfo[key], wts, m, p['df'], nres)
        assert CC.spectrum_error(over, GOLD[pre + 'o_' + key], wts, p['df']) <= BOUND
        assert CC.spectrum_error(res, GOLD[pre + 'r_' + key], wts, p['df']) <= BOUND
    # the bound's scale is attained by nothing larger: a spectrum of unit phasors is at most df sum wts
    assert NP.all(NP.abs(GOLD[pre + 'o_closure_phase_skyvis']) <= CC.scale_of(wts, p['df']).reshape(-1, 1, 1) * (1 + 1e-12))


@pytest.mark.parametrize('i', [0, 1, 2])
@pytest.mark.parametrize('action', ['return_oversampled', 'return_resampled', None, 'RETURN_RESAMPLED'])
def test_given_phases_against_the_reference(i, action):
    pre, p, f, cpinfo, bw_eff, kw = case(i)
    ctx = SI.StandinContext()
    ds = plain_ds(f, p['df'], ctx)
    before = dict(vars(ds))
    d = ds.subband_delay_transform_closure_phase(bw_eff, cpinfo=cpinfo, action=action, **kw)
    over = action == 'return_oversampled'
    compare(d, pre + ('o_' if over else 'r_'), GOLD[pre + 'o_freq_wts'], p['df'])
    assert vars(ds) == before                                           # no attribute of self is set
    assert all(c == ('spectra', 'phases', ('over',) if over else ('res',)) for c in ctx.calls) and len(ctx.calls) == 3
    if not over:
        assert d['antenna_triplets'] is cpinfo['antenna_triplets'] and d['baseline_triplets'] is cpinfo['baseline_triplets']


def test_literal_quirks():
    pre, p, f, cpinfo, bw_eff, kw = case(1)                              # two windows given out of channel order, a middle axis
    ds = plain_ds(f, p['df'])
    o = ds.subband_delay_transform_closure_phase(bw_eff, cpinfo=cpinfo, action='return_oversampled', **kw)
    r = ds.subband_delay_transform_closure_phase(bw_eff, cpinfo=cpinfo, **kw)
    assert 'antenna_triplets' not in o and 'baseline_triplets' not in o                     # :2937 rebinds the result
    assert 'antenna_triplets' in r and 'baseline_triplets' in r and 'npad' not in r and 'shape' not in r
    peak = NP.argmax(o['freq_wts'], axis=1)
    assert peak[0] < peak[1] and o['freq_center'][0] > o['freq_center'][1]                    # windows sorted, centres as given
    assert NP.array_equal(o['freq_center'], kw['freq_center']) and NP.array_equal(o['bw_eff'], bw_eff)
    m = p['nchan'] + int(p['nchan'] * p['pad'])
    assert o['lag_kernel'].shape == (1, 1, 2, m, 1) and o['closure_phase_vis'].shape == (3, 2, 2, m, 3)
    assert r['lag_kernel'].shape == (1, 1, 2, r['lags'].size, 1)
    assert NP.array_equal(r['lag_corr_length'], (1 / bw_eff) / (r['lags'][1] - r['lags'][0]))
    assert NP.array_equal(o['lag_corr_length'], p['nchan'] / NP.sum(o['freq_wts'], axis=-1))
    factor = NP.min(m * p['df'] / bw_eff)
    assert r['closure_phase_vis'].shape[-2] == int(round(m / factor)) and r['lags'].size == NP.arange(0, m, factor).size


def test_departures():
    pre, p, f, cpinfo, bw_eff, kw = case(0)
    ctx = SI.StandinContext()
    ds = plain_ds(f, p['df'], ctx)
    # default freq_center: f[int(nchan / 2)]
    d = ds.subband_delay_transform_closure_phase(bw_eff, cpinfo=cpinfo, shape='rect', verbose=False)
    assert NP.array_equal(d['freq_center'], NP.asarray(f[int(f.size / 2)]).reshape(-1))
    # a None entry is skipped and comes back as None
    info = dict(cpinfo, closure_phase_vis=None, closure_phase_noise=None)
    n = len(ctx.calls)
    d = ds.subband_delay_transform_closure_phase(bw_eff, cpinfo=info, **kw)
    assert d['closure_phase_vis'] is None and d['closure_phase_noise'] is None and len(ctx.calls) == n + 1
    assert d['closure_phase_skyvis'].shape == GOLD[pre + 'r_closure_phase_skyvis'].shape
    n = len(ctx.calls)
    with pytest.raises(NotImplementedError):
        ds.subband_delay_transform_closure_phase(bw_eff, cpinfo=cpinfo, **dict(kw, fftpow=2.0))
    with pytest.raises(ValueError, match='none of closure_phase_skyvis'):
        ds.subband_delay_transform_closure_phase(bw_eff, cpinfo={'antenna_triplets': [], 'baseline_triplets': []}, **kw)
    with pytest.raises(ValueError, match='Invalid action'):
        ds.subband_delay_transform_closure_phase(bw_eff, cpinfo=cpinfo, action='store', **kw)
    with pytest.raises(ValueError, match='exceed PRISIM_CPDELAY_MAX_LEN'):
        ds.subband_delay_transform_closure_phase(bw_eff, cpinfo=cpinfo, **dict(kw, pad=4096.0 / f.size))
    with pytest.raises(ValueError, match='ntriplets x ... x nchan x ntimes'):
        ds.subband_delay_transform_closure_phase(bw_eff, cpinfo=dict(cpinfo, closure_phase_vis=NP.zeros((3, f.size + 1, 2))), **kw)
    assert len(ctx.calls) == n                                          # all of them before any device work


def test_argument_checks_are_the_references():
    pre, p, f, cpinfo, bw_eff, kw = case(0)
    ds = plain_ds(f, p['df'])
    call = lambda b=bw_eff, **over: ds.subband_delay_transform_closure_phase(b, cpinfo=cpinfo, **dict(kw, **over))
    with pytest.raises(TypeError, match='effective bandwidth must be a scalar'):
        call('wide')
    with pytest.raises(ValueError, match='strictly positive'):
        call([1e5, -1.0])
    with pytest.raises(TypeError, match='frequency center must be scalar'):
        call(freq_center='mid')
    with pytest.raises(ValueError, match='strictly inside the observing band'):
        call(freq_center=f[0])
    with pytest.raises(ValueError, match='same number of elements'):
        call([1e5, 2e5, 3e5], freq_center=[f[3], f[9]])
    with pytest.raises(TypeError, match='Window shape must be a string'):
        call(shape=3)
    with pytest.raises(ValueError, match='Invalid value for window shape'):
        call(shape='hann')
    with pytest.raises(TypeError, match='window FFT by must be a scalar'):
        call(fftpow='1')
    with pytest.raises(ValueError, match='must be positive'):
        call(fftpow=-1.0)
    with pytest.raises(TypeError, match='pad fraction must be a scalar'):
        call(pad='1')
    with pytest.raises(TypeError, match='cpinfo must be a dictionary'):
        ds.subband_delay_transform_closure_phase(bw_eff, cpinfo=[1], **kw)
    neg = call(pad=-2.0, action='return_oversampled')                   # a negative pad is reset to none
    assert neg['npad'] == 0 and neg['lags'].size == f.size


def cube_kwargs():
    p = params('cube_')
    return p, {'freq_center': NP.asarray(p['freq_center']), 'shape': p['shape'], 'fftpow': 1.0, 'pad': p['pad'], 'verbose': False}


@pytest.mark.parametrize('action', ['return_oversampled', None])
def test_cube_path_against_the_reference(action):
    """cpinfo=None on the golden closure case without its flagged channel: the stand-in's phases differ from the reference's by at most
    32 u on the unit circle, which moves a spectrum by at most 32 u of the bound's scale."""
    p, kw = cube_kwargs()
    ctx = SI.StandinContext()
    ds = SI.make_ds(bp=GOLD['cube_bp'], ctx=ctx)
    d = ds.subband_delay_transform_closure_phase(NP.asarray(p['bw_eff']), antenna_triplets=SI.gold_triplets(), action=action, **kw)
    compare(d, 'cube_o_' if action else 'cube_r_', GOLD['cube_o_freq_wts'], p['df'])
    assert [c[1] for c in ctx.calls] == ['cube'] * 3 and not hasattr(ds, 'subband_delay_spectra')
    assert set(ds.ia.closure_delay_stats) == set(KEYS)
    if action is None:
        assert d['antenna_triplets'] == SI.gold_triplets() and len(d['baseline_triplets']) == 12


def test_cube_path_prepares_what_getClosurePhase_prepares():
    """A noiseless array: vis and noise come back as None; specsmooth_info and the delay-filter checks are getClosurePhase's; a delay
    filter and a spectral window reach the device call as masks and spectral weights."""
    p, kw = cube_kwargs()
    ctx = SI.StandinContext()
    ds = SI.make_ds(noise=False, ctx=ctx)
    bw = NP.asarray(p['bw_eff'])
    trip = SI.gold_triplets()
    d = ds.subband_delay_transform_closure_phase(bw, antenna_triplets=trip, **kw)
    assert d['closure_phase_vis'] is None and d['closure_phase_noise'] is None and len(ctx.calls) == 1
    with pytest.raises(NotImplementedError, match='specsmooth_info'):
        ds.subband_delay_transform_closure_phase(bw, antenna_triplets=trip, specsmooth_info={'op_type': 'median'}, **kw)
    with pytest.raises(ValueError, match='Invalid delay filter mode'):
        ds.subband_delay_transform_closure_phase(bw, antenna_triplets=trip, delay_filter_info={'mode': 'keep'}, **kw)
    with pytest.raises(TypeError, match='list of triplet tuples'):
        ds.subband_delay_transform_closure_phase(bw, antenna_triplets=tuple(trip), **kw)
    assert len(ctx.calls) == 1
    f = ds.f
    d2 = ds.subband_delay_transform_closure_phase(bw, antenna_triplets=trip[:4], delay_filter_info={'type': 'regular', 'min': 0.0, 'width': 3.0},
                                                  spectral_window_info={'freq_center': None, 'bw_eff': None, 'shape': 'bhw', 'fftpow': None},
                                                  **kw)
    assert d2['closure_phase_skyvis'].shape[0] == 4 and not NP.allclose(d2['closure_phase_skyvis'], d['closure_phase_skyvis'][:4])
    # the same through the phases form of a stand-in getClosurePhase result
    import closure_checker as CK
    legs, conj, _ = ds.ia.closure_leg_table(trip[:4])
    dtau = 1.0 / (f.size * ds.df)
    wts = DS.subband_freq_wts(f, ds.df, NP.asarray([0.5 * f.size * ds.df]), NP.asarray([f[f.size // 2]]), 'bhw', 1.0)[0]
    _, ph = CK.closure_phase(ds.ia.skyvis_freq, legs, conj, ds.ia.bp, ds.ia.bp_wts, freq_wts=wts,
                             delay_filter=('regular', 'discard', 0.0, 3.0 * dtau), baseline_lengths=ds.ia.baseline_lengths, df=ds.df)
    d3 = ds.subband_delay_transform_closure_phase(bw, cpinfo={'closure_phase_skyvis': ph, 'antenna_triplets': trip[:4],
                                                             'baseline_triplets': d2['baseline_triplets']}, **kw)
    assert CC.spectrum_error(d3['closure_phase_skyvis'], d2['closure_phase_skyvis'], d2['freq_wts'], ds.df) <= 1e-9


# ---- power spectra ----------------------------------------------------------------------------------------------------------------

def resampled_dict(i):
    pre, p, f, cpinfo, bw_eff, kw = case(i)
    ds = plain_ds(f, p['df'])
    d = ds.subband_delay_transform_closure_phase(bw_eff, cpinfo=cpinfo, **kw)
    for key in KEYS:                                                    # the reference's own spectra: the powers are judged on equal input
        assert d[key].shape == GOLD[pre + 'r_' + key].shape
        d[key] = GOLD[pre + 'r_' + key]
    return pre, p, f, d


@pytest.mark.parametrize('i', [0, 2])
def test_individual_power_against_the_reference(i):
    pre, p, f, d = resampled_dict(i)
    ctx = SI.StandinContext()
    dps = SI.make_dps(f, p['nt'], ctx)
    keys_before = {k: (v.copy() if isinstance(v, NP.ndarray) else v) for k, v in d.items()}
    out = dps.compute_individual_closure_phase_power_spectrum(d)
    assert set(out) == {'z', 'kprll', 'kperp', 'horizon_kprll_limits'} | set(KEYS)
    ntrip = p['lead'][0]
    assert out['kprll'].shape == (1, d['lags'].size) and out['kperp'].shape == (1, ntrip, 3)
    assert out['horizon_kprll_limits'].shape == (p['nt'], 1, ntrip, 3, 2)
    for k, v in out.items():
        ref = GOLD[pre + 'pi_' + k]
        assert v.shape == ref.shape and NP.all(NP.abs(v - ref) <= (4 * 2.0 ** -53 if k in KEYS else 1e-13) * NP.abs(ref)), k
    assert set(d) == set(keys_before) and all(NP.array_equal(d[k], keys_before[k]) for k in d if isinstance(d[k], NP.ndarray))
    assert [c[2] for c in ctx.calls] == [('individual',)] * 3


@pytest.mark.parametrize('i', [0, 1, 2])
def test_averaged_power_against_the_reference(i):
    pre, p, f, d = resampled_dict(i)
    dps = SI.make_dps(f, p['nt'])
    out = dps.compute_averaged_closure_phase_power_spectrum(d)
    assert set(out) == {'z', 'kprll', 'kperp', 'horizon_kprll_limits', 'auto', 'cross'}
    for mode in ('auto', 'cross'):
        for key in KEYS:
            ref = GOLD[pre + 'pa_%s_%s' % (mode, key)]
            got = out[mode][key]
            assert got.shape == ref.shape == (1,) + d[key].shape[1:]
            x = d[key]
            nmid = int(NP.prod(x.shape[1:-3]))
            bound_auto, bound_cross = CC.power_bounds(x.reshape(x.shape[0], nmid * x.shape[-3], -1),
                                                      NP.tile(_factor(dps, d), nmid))
            bound = (bound_auto if mode == 'auto' else bound_cross).reshape(ref.shape)
            assert NP.all(NP.abs(got - ref) <= bound), (mode, key)


def _factor(dps, d):
    z = DS.REST_FREQ_HI / d['freq_center'] - 1
    return dps.comoving_los_depth(d['bw_eff'], z, action='return') / d['bw_eff'] ** 2


def test_power_literals_and_departures():
    pre, p, f, d = resampled_dict(1)                                    # five axes: a middle axis
    ctx = SI.StandinContext()
    dps = SI.make_dps(f, p['nt'], ctx)
    with pytest.raises(ValueError, match='ntriplets x n_win x nlags x nt'):
        dps.compute_individual_closure_phase_power_spectrum(d)          # (1, -1, 1, 1): 4-D spectra only
    one = dict(d)
    for key in KEYS:
        one[key] = d[key][:1]
    with pytest.raises(ValueError, match='n0 \\(n0 - 1\\)'):
        dps.compute_averaged_closure_phase_power_spectrum(one)          # the reference: ZeroDivisionError in the cross term
    assert not ctx.calls
    some = dict(d, closure_phase_vis=None)
    del some['closure_phase_noise']
    out = dps.compute_averaged_closure_phase_power_spectrum(some)
    assert out['auto']['closure_phase_vis'] is None and out['cross']['closure_phase_vis'] is None
    assert 'closure_phase_noise' not in out['auto'] and out['auto']['closure_phase_skyvis'].shape == (1,) + d['closure_phase_skyvis'].shape[1:]


def test_length_limit_is_the_subband_limit():
    assert _abi.PRISIM_CPDELAY_MAX_LEN == _abi.PRISIM_SUBBAND_MAX_LEN          # the values themselves: tests/test_abi_headers.py


def test_new_kernels_use_no_scratch(tmp_path):
    """hipcc -S of cpdelay.hip for gfx950: no kernel of the file spills to scratch (tools/kernel_meta.py reads the metadata)."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_meta
    hipcc = '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    asm = tmp_path / 'cpdelay.s'
    subprocess.check_call([hipcc, '-O3', '-std=c++17', '--offload-arch=gfx950', '-ffp-contract=off', '-I/opt/rocm/include',
                           '--cuda-device-only', '-S', os.path.join(ROOT, 'prisim_amd', 'csrc_closure', 'cpdelay.hip'), '-o', str(asm)])
    rows = [r for r in kernel_meta.kernel_meta(asm.read_text()) if 'k_cp' in r['name']]
    assert len(rows) == 6, [r['name'] for r in rows]
    for r in rows:
        print(r)
        assert r['scratch'] == 0 and r['vgpr_spill'] == 0, r['name']
