"""CPU: the numpy checker of the closure-phasor delay spectra (tests/cpft_checker.py) against tests/golden/golden_cpft.npz (the
reference's ClosurePhaseDelaySpectrum.FT executed, tests/golden/make_golden_cpft.py); prisim_amd.bispectrum_phase.
ClosurePhaseDelaySpectrum on a stand-in context computed by that checker: the result's keys, shapes and values against the fixture, and
every error of the module docstring, raised before the context is touched."""
import os
import sys

import numpy as NP
import numpy.ma as MA
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cpft_checker as FK  # noqa: E402

from prisim_amd import _abi  # noqa: E402
from prisim_amd import bispectrum_phase as BSP  # noqa: E402

NAMES = [c['name'] for c in FK.cases()]


class Untouchable(object):
    """a context that fails on any use"""

    def __getattr__(self, name):
        raise AssertionError('the context was touched: ' + name)


def closure_phase(name, ctx, fill=True):
    """a ClosurePhase from the fixture's raw inputs with the fixture's processed and errinfo assigned"""
    cp = BSP.ClosurePhase({'raw': {k: v.copy() for k, v in FK.raw(name).items()}}, FK.freqs(name).copy(), ctx=ctx)
    if fill:
        proc, err = FK.cpinfo(name)
        cp.cpinfo['processed'].update(proc)
        cp.cpinfo['errinfo'] = err
    return cp


def ft_args(name, **over):
    c, S = FK.case(name), FK.setup(name)
    kw = {'freq_center': S['freq_center'].copy(), 'shape': c['shape'], 'pad': c['pad'], 'visscaleinfo': FK.visscaleinfo(name),
          'resample': c['resample'], 'apply_flags': c['apply_flags']}
    kw.update(over)
    return S['bw_eff'].copy(), kw


def check_result(got, name, tag, label):
    """keys, host-side entries and shapes of a result dictionary of FT against the fixture's, then the spectra"""
    g, ref = FK.gold(), FK.gold_result(name, tag)
    assert sorted(got.keys()) == sorted(g['%s_%s_keys' % (name, tag)].tolist())
    for k in ('freq_center', 'freq_wts', 'bw_eff', 'lags', 'lag_corr_length'):
        assert NP.shape(got[k]) == ref[k].shape, k
        NP.testing.assert_allclose(got[k], ref[k], rtol=1e-13, atol=0, err_msg=k)
    assert got['shape'] == ref['shape'] and got['fftpow'] == ref['fftpow'] and got['npad'] == ref['npad']
    proc, err = FK.cpinfo(name)
    for d, w in ((got['whole']['dspec'], proc['prelim']['wts']), (got['residual']['dspec'], proc['prelim']['wts']),
                 (got['errinfo']['dspec0'], err['wts']['0']), (got['errinfo']['dspec1'], err['wts']['1'])):
        assert isinstance(d['twts'], MA.MaskedArray) and NP.array_equal(MA.getdata(d['twts']), MA.getdata(w))
    for p in FK.POOLS:
        assert (FK.pool(got, p) is None) == (FK.pool(ref, p) is None), p
    assert ('submodel' in proc) == (got['submodel'] != {})
    return FK.compare_spectra(got, name, tag, label=label)


@pytest.mark.parametrize('name', NAMES)
def test_checker_against_the_reference(name):
    """the checker's three calls on the fixture's cpinfo against the reference's spectra: this pins the checker"""
    res, _ = FK.entry_results(FK.CheckerContext(), name)
    assert sorted(res) == (['o', 'r'] if FK.case(name)['resample'] else ['o'])
    for tag in res:
        FK.compare_spectra(res[tag], name, tag, label='checker')


def test_spectrum_error():
    want = NP.zeros((1, 2, 4), dtype=NP.complex128)
    got = want.copy()
    got[0, 0, 1] = 3e-3
    assert FK.spectrum_error(got, want, NP.array([[3.0, 0.0]]), 0.5) == pytest.approx(2e-3)
    got[0, 1, 2] = 1e-300                                     # a row with x = 0 must be exact
    assert FK.spectrum_error(got, want, NP.array([[3.0, 0.0]]), 0.5) == NP.inf
    got[0, 1, 2] = NP.nan
    assert FK.spectrum_error(got, want, NP.array([[3.0, 1.0]]), 0.5) == NP.inf


def test_flag_weights_of_a_zero_row():
    w = NP.array([[0.0, 0.0, 0.0], [1.0, 0.0, 2.0]])
    assert NP.array_equal(FK.flag_weights(w), [[0.0, 0.0, 0.0], [1.0, 0.0, 2.0]])
    x = FK.padded(NP.full((1, 1, 2, 3), NP.nan + 0j), NP.ones((1, 3)), 4, weights=w.reshape(1, 1, 2, 3))
    assert NP.all(x[0, 0, 0, 0] == 0) and x[0, 0, 0, 1, 1] == 0 and NP.isnan(x[0, 0, 0, 1, 0])


@pytest.mark.parametrize('name', NAMES)
def test_class_on_the_checker_context(name):
    """FT on a context computed by the checker: keys, shapes, dtypes and values of the reference's result, oversampled and resampled;
    one context call per weight set"""
    ctx = FK.CheckerContext()
    cp = closure_phase(name, ctx)
    ds = BSP.ClosurePhaseDelaySpectrum(cp)
    assert ds.cPhase is cp and ds.f is cp.f and ds.df == cp.df and ds.cPhaseDS is None and ds.cPhaseDS_resampled is None
    bw, kw = ft_args(name)
    res = ds.FT(bw, **kw)
    assert ctx.calls == 3 and sorted(ds.ft_stats) == ['errinfo0', 'errinfo1', 'prelim']
    check_result(ds.cPhaseDS, name, 'o', 'class')
    if kw['resample']:
        assert res is ds.cPhaseDS_resampled
        check_result(res, name, 'r', 'class')
    else:
        assert res is ds.cPhaseDS and ds.cPhaseDS_resampled is None
    S = FK.setup(name)
    nrows = MA.getdata(cp.cpinfo['processed']['prelim']['wts']).shape[:3]
    klead = nrows if kw['apply_flags'] else (1, 1, 1)
    assert ds.cPhaseDS['lag_kernel'].shape == (S['bw_eff'].size,) + klead + (S['m'],)
    assert ds.cPhaseDS['whole']['dspec']['mean'].shape == (S['bw_eff'].size,) + nrows + (S['m'],)
    if kw['resample']:
        assert res['whole']['dspec']['mean'].shape == (S['bw_eff'].size,) + nrows + (S['nres'],)
        assert res['lags'].size == res['lag_kernel'].shape[-1] == int(NP.ceil(S['m'] / S['factor']))


def test_defaults_on_the_checker_context():
    """freq_center=None is f[f.size // 2]; pad < 0 is no padding, silently; visscaleinfo=None is a scale of 1: the all-ones case
    divided by sqrt(1/3)"""
    name = 'm32'
    cp = closure_phase(name, FK.CheckerContext())
    ds = BSP.ClosurePhaseDelaySpectrum(cp)
    bw, kw = ft_args(name, freq_center=None, pad=-0.5, visscaleinfo=None, resample=False)
    res = ds.FT(bw, **kw)
    assert NP.array_equal(res['freq_center'], [cp.f[cp.f.size // 2]]) and res['npad'] == 0 and res['lags'].size == cp.f.size
    bw, kw = ft_args(name, visscaleinfo=None)
    res = ds.FT(bw, **kw)
    FK.compare_spectra(res, name, 'r', label='no visscaleinfo', scale=1.0 / NP.sqrt(1.0 / 3.0))
    FK.compare_spectra(ds.cPhaseDS, name, 'o', label='no visscaleinfo', scale=1.0 / NP.sqrt(1.0 / 3.0))


def test_errors_come_before_the_context():
    name = 'm32'
    with pytest.raises(TypeError, match='instance of class ClosurePhase'):
        BSP.ClosurePhaseDelaySpectrum(object())
    cp = closure_phase(name, Untouchable())
    ds = BSP.ClosurePhaseDelaySpectrum(cp)
    bw, kw = ft_args(name)
    vis = FK.visscaleinfo(name)

    def fails(exc, match, bw_=bw, **over):
        with pytest.raises(exc, match=match):
            ds.FT(bw_, **dict(kw, **over))

    fails(TypeError, 'effective bandwidth', bw_='wide')
    fails(ValueError, 'strictly positive', bw_=[0.0])
    fails(ValueError, 'strictly inside', freq_center=cp.f[0])
    fails(TypeError, 'frequency center', freq_center='mid')
    fails(ValueError, 'same number of elements', bw_=[1e5, 2e5], freq_center=[cp.f[3], cp.f[4], cp.f[5]])
    fails(TypeError, 'Window shape', shape=3)
    fails(ValueError, 'window shape', shape='hann')
    fails(TypeError, 'window FFT', fftpow='2')
    fails(ValueError, 'must be positive', fftpow=-1.0)
    fails(NotImplementedError, 'fftpow', fftpow=2.0)
    fails(TypeError, 'pad fraction', pad='1')
    fails(TypeError, 'datapool', datapool=1)
    fails(ValueError, 'datapool not supported', datapool='native')
    fails(TypeError, 'method', method=1)
    fails(ValueError, 'FFT method not supported', method='dft')
    fails(NotImplementedError, 'nufft', method='nufft')
    fails(TypeError, 'apply_flags', apply_flags=1)
    fails(TypeError, 'visscaleinfo must be a dictionary', visscaleinfo=3)
    fails(KeyError, 'vis', visscaleinfo={'lst': vis['lst']})
    fails(KeyError, 'lst', visscaleinfo={'vis': vis['vis']})
    fails(TypeError, 'numpy or a masked array', visscaleinfo={'vis': [1.0], 'lst': vis['lst']})
    fails(NotImplementedError, 'several reference LSTs', visscaleinfo={'vis': NP.repeat(vis['vis'], 2, axis=1), 'lst': NP.array([1.0, 2.0])})
    fails(NotImplementedError, 'InterferometerArray', visscaleinfo={'vis': type('IA', (), {'skyvis_freq': None})(), 'lst': vis['lst']})
    fails(ValueError, 'exceeds', pad=4096.0)
    # missing inputs name the step to run
    for drop, step in ((('processed', 'prelim', 'eicp'), 'smooth_in_tbins'), (('processed', 'prelim', 'wts'), 'smooth_in_tbins'),
                       (('errinfo', 'wts'), 'subsample_differencing'), (('errinfo', 'eicp_diff'), 'subsample_differencing')):
        cp2 = closure_phase(name, Untouchable())
        d = cp2.cpinfo
        for k in drop[:-1]:
            d = d[k]
        del d[drop[-1]]
        with pytest.raises(ValueError, match=step):
            BSP.ClosurePhaseDelaySpectrum(cp2).FT(bw, **kw)
    with pytest.raises(ValueError, match='smooth_in_tbins'):
        BSP.ClosurePhaseDelaySpectrum(closure_phase(name, Untouchable(), fill=False)).FT(bw, **kw)
    assert ds.cPhaseDS is None and ds.cPhaseDS_resampled is None


def test_abi_lists_the_entry():
    assert _abi.CPFT_EXPORTS == ('prisim_cphase_ft',)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'prisim_cpft.h')).read()
    assert 'int prisim_cphase_ft(' in hdr
    assert [f[0] for f in _abi.PrisimCpftStats._fields_] == ['wall_ms', 'kernel_ms', 'rows', 'chunks', 'chunk_rows', 'row_bytes', 'kernel_bytes',
                                                             'upload_bytes', 'download_bytes', 'route', 'streams', 'group_rows', 'lds_bytes']
    for f in ('kernel_bytes', 'row_bytes', 'group_rows'):
        assert f in hdr
    assert (_abi.PRISIM_CPFT_OVER, _abi.PRISIM_CPFT_RES, _abi.PRISIM_CPFT_LAG) == (1, 2, 4)
