"""CPU: the power spectra of closure-phase delay spectra (prisim_amd.bispectrum_phase.ClosurePhaseDelaySpectrum.subset,
compute_power_spectrum, compute_power_spectrum_uncertainty) on a checker context, and the checker itself (tests/cpxps_checker.py),
against tests/golden/golden_cpxps.npz, the reference's own statements executed (tests/golden/make_golden_cpxps.py).

Bounds.  The checker against the reference: the entry's, (L + 8) 2^-52 S per element (cpxps_checker.bound).  The class against the
reference, where the host weights, normalises and averages the collapsed result: cpxps_checker.class_bound, per window."""
import copy
import os
import sys
import types

import numpy as NP
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cpxps_checker as XK  # noqa: E402

from prisim_amd import _abi  # noqa: E402
from prisim_amd import bispectrum_phase as BSP  # noqa: E402
from prisim_amd import delay_spectrum as DS  # noqa: E402
from prisim_amd import dsp_readings as DSP  # noqa: E402

NAMES = [c['name'] for c in XK.cases()]


class Untouchable(object):
    """a context that no call may reach: every error is raised before any device work"""

    def __getattr__(self, name):
        raise AssertionError('the context was touched: ' + name)


def spectrum_object(ctx, cpinfo=None, cpds=None, f=None):
    """a ClosurePhaseDelaySpectrum over the fixture's cpinfo and FT results, on the context ctx"""
    gf, gcpinfo, gcpds = XK.gold_inputs()
    cpinfo, cpds, f = cpinfo or gcpinfo, cpds or gcpds, gf if f is None else f
    obj = BSP.ClosurePhaseDelaySpectrum.__new__(BSP.ClosurePhaseDelaySpectrum)
    obj.cPhase = types.SimpleNamespace(cpinfo=cpinfo, _ctx=ctx, _context=lambda: ctx)
    obj.f, obj.df = f, f[1] - f[0]
    obj.cPhaseDS, obj.cPhaseDS_resampled = cpds.get('oversampled'), cpds.get('resampled')
    obj.ft_stats, obj.xps_stats = {}, {}
    return obj


def run_case(obj, name, **kw):
    spec = XK.case(name)
    sel, auto, xinfo = XK.gold_arguments(spec)
    method = obj.compute_power_spectrum_uncertainty if spec['unc'] else obj.compute_power_spectrum
    return method(selection=sel, autoinfo=auto, xinfo=xinfo, units='Jy', **kw)


def check_case(res, name, cpds, label=''):
    """keys, shapes, what goes with the spectra, and the spectra within class_bound of the reference's; returns the worst share"""
    spec, meta = XK.case(name), XK.gold_meta(name)
    for k in ('triads', 'triads_ind', 'lst', 'lst_ind', 'dlst', 'days', 'day_ind', 'dday', 'lstXoffsets'):
        want = XK.gold_top(name, k)
        assert NP.shape(res[k]) == want.shape and NP.allclose(res[k], want, rtol=1e-15, atol=0), (name, k)
    worst = 0.0
    outputs = XK.gold_outputs(name)
    assert outputs
    for smp in XK.SAMPLINGS:
        for k in ('z', 'kprll'):
            assert NP.array_equal(res[smp][k], XK.gold()['in__%s__%s' % (smp, k)]), (name, smp, k)
        assert set(res[smp].keys()) == {'z', 'kprll', 'lags', 'freq_center', 'bw_eff', 'shape', 'freq_wts', 'lag_corr_length'} | \
            ({'errinfo'} if spec['unc'] else {'whole', 'submodel', 'residual'})
    for (smp, pool, stat), want in outputs.items():
        r = res[smp][pool]
        assert set(r.keys()) == {'mean', 'median', 'diagoffsets', 'diagweights', 'axesmap', 'nsamples_incoh', 'nsamples_coh'}
        for key in ('diagoffsets', 'diagweights', 'axesmap'):
            assert {str(ax) for ax in r[key]} == set(meta[key]), (name, key)
            for ax, v in r[key].items():
                assert NP.array_equal(NP.asarray(v), NP.asarray(meta[key][str(ax)])), (name, key, ax)
        assert r['nsamples_incoh'] == meta['nsamples_incoh'] and r['nsamples_coh'] == meta['nsamples_coh']
        got = r[stat]
        assert got.shape == want.shape and got.dtype == NP.complex128, (name, smp, pool, stat, got.shape, want.shape)
        gn, wn = XK.cnan(got), XK.cnan(want)
        assert NP.array_equal(gn, wn), (name, smp, pool, stat, 'NaN positions')
        lim = XK.class_bound(spec, cpds, smp, pool, XK.gold()['in__%s__factor' % smp]).reshape((-1,) + (1,) * (got.ndim - 1))
        share = float(NP.max(NP.where(gn, 0.0, NP.abs(NP.where(gn, 0.0, got - want))) / lim))
        print('%s %s %s %s %s: %.3f of the bound' % (label, name, smp, pool, stat, share))
        assert share <= 1.0, (name, smp, pool, stat, share)
        worst = max(worst, share)
    return worst


def test_array_trace_reading():
    x = NP.arange(18.0).reshape(2, 3, 3, 1) + 1j
    tr, off, cnt = DSP.array_trace(x, axis1=1, axis2=2, outaxis='axis1')
    assert tr.shape == (2, 5, 1) and NP.array_equal(off, [-2, -1, 0, 1, 2]) and NP.array_equal(cnt, [1, 2, 3, 2, 1])
    assert tr[0, 2, 0] == x[0, 0, 0, 0] + x[0, 1, 1, 0] + x[0, 2, 2, 0] and tr[1, 3, 0] == x[1, 0, 1, 0] + x[1, 1, 2, 0]
    assert tr[1, 0, 0] == x[1, 2, 0, 0]
    y = NP.moveaxis(x, 3, 0)                                                   # (1, 2, 3, 3)
    tr2, _, _ = DSP.array_trace(y, axis1=2, axis2=3, outaxis='axis2')
    assert tr2.shape == (1, 2, 5) and NP.array_equal(tr2[0], tr[..., 0])
    x[0, 1, 1, 0] = NP.nan
    assert NP.isnan(DSP.array_trace(x, axis1=1, axis2=2)[0][0, 2, 0])
    with pytest.raises(ValueError):
        DSP.array_trace(NP.zeros((2, 3)))
    with pytest.raises(ValueError):
        DSP.array_trace(NP.zeros((3, 3)), offsets=[3])


def test_the_checkers_median_is_numpys():
    rng = NP.random.default_rng(3)
    x = rng.integers(-2, 3, (6, 7, 5)) + 1j * rng.integers(-2, 3, (6, 7, 5))   # many ties in the real part
    x = x.astype(NP.complex128)
    x[0, :, 0] = NP.nan
    x[1, :3, 1] = complex(NP.nan, 0.0)
    x[2, 4, :] = complex(1.0, NP.nan)
    with NP.errstate(all='ignore'):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            want = NP.nanmedian(x, axis=1)
    got = XK.select_median(x, 1)
    assert NP.array_equal(XK.cnan(got), NP.isnan(want)) and NP.isnan(want[0, 0])
    assert NP.array_equal(got[~NP.isnan(want)], want[~NP.isnan(want)])


def test_checker_layout_against_a_loop():
    """every index convention of the header, element by element"""
    rng = NP.random.default_rng(11)
    shape = (2, 3, 2, 3, 2)
    a = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    b = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    w = [rng.standard_normal(n) + 1j * rng.standard_normal(n) for n in shape[1:4]]
    f = NP.asarray([2.0, 0.5])
    sh = [0, 2]
    p = XK.cross(a, b, f, w, ('full', 'none', 'full'), sh)
    assert p.shape == (2, 2, 3, 2, 3, 3, 2)
    for s, i, d, t, u in [(0, 1, 0, 2, 1), (1, 2, 1, 0, 2), (1, 1, 0, 1, 1)]:
        if i < sh[s]:
            assert NP.all(XK.cnan(p[:, s, i, d, t, u]))
            continue
        want = f[:, None] * (a[:, i, d, t] * (w[0][i] * w[1][d] * w[2][t])) * NP.conj(b[:, i - sh[s], d, u] * (w[0][i - sh[s]] * w[1][d] * w[2][u]))
        assert NP.allclose(p[:, s, i, d, t, u], want, rtol=1e-14, atol=0)
    out = XK.xpower(a, b, f, w, ('full', 'none', 'collapse'), sh, [3])
    assert out.shape == (2, 2, 3, 2, 5, 2)
    assert NP.allclose(out[:, 0, 1, 1, 3], (p[:, 0, 1, 1, 0, 1] + p[:, 0, 1, 1, 1, 2]) / 2, rtol=1e-14, atol=0)
    assert _abi.Context.cphase_xpower_shape(shape, ('full', 'none', 'collapse'), 2) == out.shape
    assert _abi.Context.cphase_xpower_shape(shape, ('collapse', 'full', 'none'), 2) == (2, 2, 2, 2, 3, 2)


@pytest.mark.parametrize('name,modes,order', [('x13_c13', ('collapse', 'none', 'collapse'), [1, 3]), ('x23_c23', ('none', 'collapse', 'collapse'), [2, 3]),
                                              ('selection', ('full', 'collapse', 'full'), [2]), ('unc_x13_c3', ('full', 'none', 'collapse'), [3])])
def test_checker_against_the_fixture(name, modes, order):
    """the cases of the fixture that are one call of the entry: the checker within the entry's bound of the reference"""
    spec = XK.case(name)
    _, _, cpds = XK.gold_inputs()
    outputs = XK.gold_outputs(name)
    assert outputs
    for (smp, pool, stat), want in outputs.items():
        ds = cpds[smp]
        if pool == 'errinfo':
            a, b = ds['errinfo']['dspec0'][stat], ds['errinfo']['dspec1'][stat]
        else:
            a, b = (ds[pool]['dspec'] if pool == 'submodel' else ds[pool]['dspec'][stat]), None
        if 'selection' in spec:
            lst = NP.asarray(spec['selection']['lst'])
            tri = NP.asarray([XK.gold()['in__triads'].tolist().index(t) for t in spec['selection']['triads']])
            a = a[:, lst][:, :, :, tri]
        fac = XK.gold()['in__%s__factor' % smp]
        args = (a, b, fac, None, modes, [0, 1], order, stat)
        got, lim = XK.as_reference(XK.xpower(*args), modes), XK.as_reference(XK.bound(*args), modes)
        assert got.shape == want.shape
        bad = XK.cnan(want)
        assert NP.array_equal(XK.cnan(got), bad) and bad.mean() == XK.nan_share(modes, [0, 1], a.shape[1])
        share = float(NP.max(NP.abs(got - want)[~bad] / lim[~bad]))
        print('%s %s %s %s: %.3f of the bound' % (name, smp, pool, stat, share))
        assert share <= 1.0


@pytest.mark.parametrize('name', NAMES)
def test_class_on_the_checker_context_against_the_fixture(name):
    ctx = XK.CheckerContext()
    _, _, cpds = XK.gold_inputs()
    res = run_case(spectrum_object(ctx), name)
    check_case(res, name, cpds, label='checker')
    spec = XK.case(name)
    assert ctx.calls == (4 if spec["unc"] else 12)                              # one call per pool, statistic and sampling
    for call in ctx.xcalls:
        assert call['collapse'] == tuple(ax for ax in spec['xinfo']['collapse_axes'] if not (spec['unc'] and ax == 2))


def test_the_callers_dictionaries_are_not_modified():
    spec = XK.case('weights')
    sel, auto, xinfo = XK.gold_arguments(spec)
    sel = {'lst': NP.asarray([0, 1, 2, 3])}
    before = copy.deepcopy((sel, auto, xinfo))
    obj = spectrum_object(XK.CheckerContext())
    cpds = {'oversampled': obj.cPhaseDS}
    obj.compute_power_spectrum(cpds=cpds, selection=sel, autoinfo=auto, xinfo=xinfo, units='Jy')
    for x, y in zip(before, (sel, auto, xinfo)):
        assert repr(x) == repr(y)
    assert set(cpds.keys()) == {'oversampled'}


def test_jy_factor_closed_form():
    """factor = drz_los / bw_eff^2 with drz_los = c (1 + z)^2 bw_eff / (f21 H0 E(z)), in Mpc/h with H0 = 100 km/s/Mpc"""
    import scipy.constants as FCNST
    obj = spectrum_object(Untouchable())
    ds = obj.cPhaseDS
    z, kprll, factor = obj.power_factor(ds, units='Jy')
    fc, bw = ds['freq_center'], ds['bw_eff']
    zz = DS.REST_FREQ_HI / fc - 1
    c = DS.cosmo100
    ez = NP.sqrt(c.Om0 * (1 + zz) ** 3 + c.Or0 * (1 + zz) ** 4 + (1 - c.Om0 - c.Or0))
    want = (FCNST.c / 1e3) * (1 + zz) ** 2 / (DS.REST_FREQ_HI * 100.0 * ez) / bw
    assert NP.allclose(z, zz, rtol=1e-15) and NP.allclose(factor, want, rtol=1e-14, atol=0)
    assert kprll.shape == (fc.size, ds['lags'].size)
    assert NP.allclose(kprll, (2 * NP.pi * 100.0 * DS.REST_FREQ_HI * ez / FCNST.c / (1 + zz) ** 2 * 1e3)[:, None] * ds['lags'][None, :], rtol=1e-14)
    with pytest.raises(ValueError):
        obj.power_factor(ds, units='mK')


def test_subset():
    obj = spectrum_object(Untouchable())
    t, l, d, p = obj.subset()
    assert NP.array_equal(t, [0, 1, 2]) and NP.array_equal(l, NP.arange(4)) and NP.array_equal(d, NP.arange(3)) and NP.array_equal(p, NP.arange(3))
    sel = {'triads': [(1, 2, 4), (0, 1, 2)], 'lst': [3, 1], 'days': NP.asarray([0, 1, 2, 3])}
    with pytest.raises(ValueError, match='out of bounds'):
        obj.subset(sel)                                                          # the prelim stack has three day bins
    sel['days'] = [0, 1]
    before = copy.deepcopy(sel)
    t, l, d, p = obj.subset(sel)
    assert NP.array_equal(t, [2, 0]) and NP.array_equal(l, [3, 1]) and NP.array_equal(d, [0, 1]) and p.size == 0
    assert sel == before
    obj.cPhase.cpinfo['processed']['prelim']['wts'] = NP.ma.zeros((4, 4, 3, 6))
    assert NP.array_equal(obj.subset({'days': [0, 1, 2, 3]})[3], [0, 1, 2])
    assert NP.array_equal(obj.subset({'days': [0, 3, 1, 2]})[3], [0, 1, 2])
    assert obj.subset({'days': [0, 1, 2]})[3].size == 0
    with pytest.raises(TypeError):
        obj.subset([1])
    with pytest.raises(TypeError):
        obj.subset({'lst': 2})
    with pytest.raises(ValueError):
        obj.subset({'lst': [4]})
    with pytest.raises(ValueError):
        obj.subset({'triads': [(9, 9, 9)]})
    del obj.cPhase.cpinfo['processed']['prelim']['wts']
    with pytest.raises(ValueError, match='LST index selection'):
        obj.subset()


def test_errors_are_raised_before_any_device_work():
    obj = spectrum_object(Untouchable())
    cps = obj.compute_power_spectrum
    x13 = {'axes': [1, 3], 'collapse_axes': [3]}
    with pytest.raises(TypeError):
        cps(units=1, xinfo=x13)
    with pytest.raises(ValueError):
        cps(units='mK', xinfo=x13)
    with pytest.raises(TypeError):
        cps(units='K', beamparms=None, xinfo=x13)
    with pytest.raises(NotImplementedError, match='beamfile'):
        cps(units='K', beamparms={'beamfile': 'beam.fits', 'telescope': {}}, xinfo=x13)
    with pytest.raises(KeyError):
        cps(units='K', beamparms={}, xinfo=x13)
    with pytest.raises(TypeError):
        cps(units='K', beamparms={'telescope': {}, 'nside': 16.0}, xinfo=x13)
    for bad in ({'autoinfo': 3}, {'xinfo': 3}, {'selection': 3}, {'cpds': 3}, {'autoinfo': {'axes': 'a'}}, {'xinfo': {'axes': 1.5}},
                {'autoinfo': {'axes': [2], 'wts': NP.ones(3)}}, {'xinfo': {'axes': [1], 'wts': []}},
                {'xinfo': {'axes': [1], 'wts': {'preX': NP.ones(1), 'postX': [NP.ones(1)]}}},
                {'xinfo': {'axes': [1], 'wts': {'preX': [NP.ones(1)], 'postX': [NP.ones(1)], 'postXnorm': 1}}},
                {'xinfo': {'axes': [1], 'avgcov': 1}}, {'xinfo': {'axes': [1], 'collapse_axes': 'x'}}):
        with pytest.raises(TypeError):
            cps(units='Jy', **bad)
    for bad in ({'autoinfo': {'axes': [2], 'wts': [NP.ones(3), NP.ones(3)]}}, {'xinfo': {'axes': [1, 3], 'wts': {'preX': [NP.ones(1)], 'postX': [NP.ones(1)]}}},
                {'autoinfo': {'axes': [2, 3]}, 'xinfo': {'axes': [1, 3]}}, {'xinfo': {'axes': [1, 4]}}, {'xinfo': {'axes': [1], 'collapse_axes': [3]}},
                {'xinfo': {'axes': [1, 3], 'avgcov': True}},                          # avgcov without a collapsed axis
                {'xinfo': {'axes': [3], 'wts': {'preX': [NP.ones(2)], 'postX': [NP.ones(1)]}}},
                {'xinfo': {'axes': [3], 'collapse_axes': [3], 'wts': {'preX': [NP.ones(3)], 'postX': [NP.ones(4)]}}},
                {'xinfo': {'axes': [1, 3]}, 'selection': {'lst': [0]}},                        # the shift 1 leaves no LST bin of one
                {'autoinfo': {'axes': [2], 'wts': [NP.ones(2)]}}):
        with pytest.raises(ValueError):
            cps(units='Jy', **bad)
    with pytest.raises(NotImplementedError, match='preXnorm'):
        cps(units='Jy', xinfo={'axes': [1], 'wts': {'preX': [NP.ones(1)], 'postX': [NP.ones(1)], 'preXnorm': True}})
    unc = obj.compute_power_spectrum_uncertainty
    with pytest.raises(ValueError, match='cross'):
        unc(units='Jy', xinfo={'axes': [2]})                                          # no incoherent axis is left
    with pytest.raises(ValueError, match='cross'):
        unc(units='Jy')
    obj.cPhaseDS = obj.cPhaseDS_resampled = None
    with pytest.raises(ValueError, match='FT'):
        cps(units='Jy', xinfo=x13)


def test_no_crossed_axis_gives_factor_times_the_squared_modulus():
    """autoinfo=None, xinfo=None and xinfo={'axes': None}: no coherent and no incoherent axes; the reference cannot run these"""
    obj = spectrum_object(Untouchable())
    for kw in ({}, {'xinfo': {'axes': None}}, {'autoinfo': None, 'xinfo': None}, {'xinfo': {'axes': [], 'collapse_axes': []}}):
        res = obj.compute_power_spectrum(units='Jy', **kw)
        for smp in XK.SAMPLINGS:
            fac = XK.gold()['in__%s__factor' % smp]
            r = res[smp]['residual']
            assert r['diagoffsets'] == {} and r['diagweights'] == {} and r['axesmap'] == {} and r['nsamples_incoh'] == 1 and r['nsamples_coh'] == 1
            want = fac.reshape(-1, 1, 1, 1, 1) * NP.abs(obj.cPhaseDS_resampled['residual']['dspec']['median'] if smp == 'resampled' else
                                                        obj.cPhaseDS['residual']['dspec']['median']) ** 2
            assert r['median'].dtype == NP.complex128 and NP.array_equal(r['median'], want)
    res = obj.compute_power_spectrum(units='Jy', autoinfo={'axes': [1, 2, 3]})
    assert res['oversampled']['whole']['mean'].shape == (2, 1, 1, 1, 8) and res['oversampled']['whole']['nsamples_coh'] == 36


def test_full_cross_power_without_a_collapsed_axis_and_a_selection_with_coherent_axes():
    """no collapsed axis: the full matrix with empty diagoffsets / diagweights; a selection with coherent axes is indexed once"""
    ctx = XK.CheckerContext()
    obj = spectrum_object(ctx)
    res = obj.compute_power_spectrum(units='Jy', autoinfo={'axes': [2]}, xinfo={'axes': [1, 3]}, selection={'lst': [1, 3], 'days': [0, 2]},
                                     cpds={'resampled': obj.cPhaseDS_resampled})
    assert 'oversampled' not in res and NP.array_equal(res['day_ind'], [0, 2])
    r = res['resampled']['whole']
    assert r['mean'].shape == (2, 2, 2, 1, 3, 3, 4) and r['diagoffsets'] == {} and r['diagweights'] == {}
    assert NP.array_equal(r['axesmap'][1], [1, 2]) and NP.array_equal(r['axesmap'][3], [4, 5]) and r['nsamples_coh'] == 2
    x = obj.cPhaseDS_resampled['whole']['dspec']['mean'][:, [1, 3]][:, :, [0, 2]]
    tw = XK.gold()['in__twts']
    tw = tw[..., [int(NP.argmax(NP.sum(tw, axis=(0, 1, 2))))]][[1, 3]][:, [0, 2]][None]
    a = NP.sum(tw * x, axis=2, keepdims=True) / NP.sum(tw, axis=2, keepdims=True)
    fac = XK.gold()['in__resampled__factor']
    want = fac[:, None] * a[:, 1, 0, 2] * NP.conj(a[:, 0, 0, 1])                   # shift 1, LST 1 of the selection; a at the second triad index
    assert NP.allclose(r['mean'][:, 1, 1, 0, 1, 2], want, rtol=1e-13, atol=0)
    assert NP.all(XK.cnan(r['mean'][:, 1, 0])) and not NP.any(XK.cnan(r['mean'][:, 0]))


def test_stats_struct_mirrors_the_header():
    """PrisimCpxpsStats field by field against include/prisim_cpxps.h, and its dict: keys in order, ints and floats as ctypes hands them"""
    import ctypes as C
    import re
    st_type = _abi.Context.PrisimCpxpsStats
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'prisim_cpxps.h')).read()
    body = re.sub(r'/\*.*?\*/', '', header[header.index('typedef struct prisim_cpxps_stats'):header.index('} prisim_cpxps_stats;')], flags=re.S)
    fields = re.findall(r'(double|int64_t|int32_t)\s+(\w+);', body)
    assert [(n, {'double': C.c_double, 'int64_t': C.c_int64, 'int32_t': C.c_int32}[t]) for t, n in fields] == list(st_type._fields_)
    st = st_type()
    for k, (name, ctype) in enumerate(st_type._fields_):
        setattr(st, name, k + 1.5 if ctype is C.c_double else k + 2)
    got = _abi._stats_dict(st)
    assert list(got) == ['wall_ms', 'kernel_ms', 'chunks', 'chunk_lags', 'kernel_bytes', 'upload_bytes', 'download_bytes', 'cross_bytes']
    assert got == {'wall_ms': 1.5, 'kernel_ms': 2.5, 'chunks': 4, 'chunk_lags': 5, 'kernel_bytes': 6, 'upload_bytes': 7, 'download_bytes': 8,
                   'cross_bytes': 9}
    assert all(type(got[k]) is (float if k.endswith('_ms') else int) for k in got)
    assert _abi.CPXPS_EXPORTS == ('prisim_cphase_xpower',) and hasattr(_abi.load_library(), 'prisim_cphase_xpower')
    assert _abi.PRISIM_CPXPS_MAX_MEDIAN == int(re.search(r'#define PRISIM_CPXPS_MAX_MEDIAN (\d+)', header).group(1))
