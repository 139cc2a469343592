"""CPU: the incoherent averages of closure-phase power spectra (prisim_amd.bispectrum_phase.incoherent_cross_power_spectrum_average,
incoherent_kbin_averaging) on a checker context, and the checker itself (tests/cpavg_checker.py), against
tests/golden/golden_cpavg.npz, the reference's own statements executed (tests/golden/make_golden_cpavg.py).

Bounds: those of the entries, derived in cpavg_checker's docstring.  The functions add no arithmetic to the entries', so they are held
to the same bounds."""
import copy
import ctypes as C
import os
import re
import sys

import numpy as NP
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cpavg_checker as AK  # noqa: E402

from prisim_amd import _abi  # noqa: E402
from prisim_amd import bispectrum_phase as BSP  # noqa: E402

AVG_CASES = [c['name'] for c in AK.cases() if c['kind'] == 'avg']
KBIN_CASES = [c['name'] for c in AK.cases() if c['kind'] == 'kbin']
POOLS = ('whole', 'submodel', 'residual', 'errinfo')


class Untouchable(object):
    """a context that no call may reach: every error is raised before any device work"""

    def __getattr__(self, name):
        raise AssertionError('the context was touched: ' + name)


def entry_arguments(sets, smp, pool, stat, combos, skip=()):
    """(arrays, weights, masks) of the entry for one sampling, pool and statistic, written from the header: the weights are the outer
    product of the diagweights at their axes (or the array given), the masks select the offsets of each combination"""
    arrays = [NP.asarray(d[smp][pool][stat]) for d in sets]
    weights = []
    for d, a in zip(sets, arrays):
        dw = d[smp][pool]['diagweights']
        if isinstance(dw, dict):
            w = NP.ones((1,) * a.ndim)
            for ax, v in dw.items():
                shp = [1] * a.ndim
                shp[int(d[smp][pool]['axesmap'][ax][0])] = -1
                w = w * NP.asarray(v, dtype=NP.float64).reshape(shp)
        else:
            w = NP.asarray(dw, dtype=NP.float64)
        weights.append(w)
    masks = []
    for combo in combos or []:
        p0 = sets[0][smp][pool]
        masks.append({int(p0['axesmap'][ax][0]): NP.isin(p0['diagoffsets'][ax], combo[ax]) for ax in combo if ax not in skip})
    return arrays, weights, masks


def pools_of(res):
    for smp in AK.SAMPLINGS:
        for pool in POOLS:
            if smp in res and pool in res[smp]:
                for stat in ('mean', 'median'):
                    if stat in res[smp][pool]:
                        yield smp, pool, stat


def check_average(got, name, which, sets, label):
    """a result of incoherent_cross_power_spectrum_average against the fixture's: keys, shapes, lists per combination, diagweights,
    and the values within the entry's bounds; the worst share"""
    spec, want = AK.case(name), AK.gold_average(name, which)
    combos = AK.diagoffsets_of(spec)
    skip = (2,) if which == 'e' else ()
    assert set(got.keys()) == set(AK.TOP_KEYS) | {smp for smp in AK.SAMPLINGS if smp in sets[0]}
    for key in AK.TOP_KEYS:
        assert NP.array_equal(got[key], sets[0][key]), key
    worst, seen = 0.0, 0
    for smp, pool, stat in pools_of(want):
        assert set(got[smp].keys()) == set(AK.SAMPLING_KEYS) | {p for p in POOLS if p in sets[0][smp]}
        r, w = got[smp][pool], want[smp][pool]
        assert set(r.keys()) == {'diagoffsets', 'axesmap', 'diagweights'} | {s for s in ('mean', 'median') if s in sets[0][smp][pool]}
        for key in ('diagoffsets', 'axesmap'):
            assert set(r[key]) == set(w[key]) and all(NP.array_equal(r[key][ax], w[key][ax]) for ax in w[key])
        arrays, weights, masks = entry_arguments(sets, smp, pool, stat, combos, skip)
        model = AK.xavg(arrays, weights, [m for m in masks if m], bounds=True)
        tag = '%s %s %s %s %s %s' % (label, name, which, smp, pool, stat)
        if combos is None:
            assert isinstance(r[stat], NP.ndarray) and not isinstance(r[stat], NP.ma.MaskedArray)
            worst = max(worst, AK.compare(r[stat], w[stat], model['avg_bound'], tag))
            worst = max(worst, AK.compare(r['diagweights'], w['diagweights'], 4 * AK.EPS * NP.abs(w['diagweights']), tag + ' diagweights'))
        else:
            assert isinstance(r[stat], list) and len(r[stat]) == len(r['diagweights']) == len(combos)
            bounds = iter(model['out_bound'])
            for c, m in enumerate(masks):
                assert type(r[stat][c]) is NP.ndarray and type(r['diagweights'][c]) is NP.ndarray
                bound = next(bounds) if m else model['avg_bound']
                worst = max(worst, AK.compare(r[stat][c], w[stat][c], bound, '%s [%d]' % (tag, c)))
                worst = max(worst, AK.compare(r['diagweights'][c], w['diagweights'][c], 64 * AK.EPS * NP.abs(w['diagweights'][c]),
                                              '%s diagweights [%d]' % (tag, c)))
        assert not NP.any(AK.cnan(NP.concatenate([NP.ravel(x) for x in (r[stat] if isinstance(r[stat], list) else [r[stat]])])))
        seen += 1
    assert seen
    return worst


def check_kbin(got, name, xin, label):
    """a result of incoherent_kbin_averaging against the fixture's: keys, kbininfo, shapes and the values within the entry's bounds"""
    want = AK.gold_kbin(name)
    assert set(got.keys()) == set(AK.TOP_KEYS) | set(AK.SAMPLINGS)
    worst = 0.0
    empty = total = 0
    for smp in AK.SAMPLINGS:
        assert set(got[smp].keys()) == {'z', 'freq_center', 'bw_eff', 'shape', 'freq_wts', 'lag_corr_length', 'kbininfo', 'whole'}
        gi, wi = got[smp]['kbininfo'], want[smp]['kbininfo']
        assert set(gi.keys()) == {'counts', 'kbin_edges', 'kbinnum', 'ri', 'whole'}
        for key in ('counts', 'kbin_edges', 'kbinnum', 'ri'):
            assert len(gi[key]) == AK.NSPW and all(NP.array_equal(a, b) for a, b in zip(gi[key], wi[key])), (name, smp, key)
        kprll = NP.asarray(xin[smp]['kprll'])
        nk = wi['counts'][0].size
        lists = [[ri[ri[b]:ri[b + 1]] for b in range(nk)] for ri in wi['ri']]
        offsets = NP.asarray([NP.concatenate(([0], NP.cumsum([len(m) for m in l]))) for l in lists])
        members = [NP.concatenate(l).astype(NP.int64) if l else NP.zeros(0, dtype=NP.int64) for l in lists]
        assert set(got[smp]['whole'].keys()) == {'diagoffsets', 'diagweights', 'axesmap'} | set(want[smp]['whole'])
        for stat in want[smp]['whole']:
            ncombo = len(want[smp]['whole'][stat]['PS'])
            assert ncombo == len(xin[smp]['whole'][stat]) == len(got[smp]['whole'][stat]['PS']) == len(gi['whole'][stat])
            for c in range(ncombo):
                model = AK.kbin(xin[smp]['whole'][stat][c], kprll, offsets, members, bounds=True)
                tag = '%s %s %s %s [%d]' % (label, name, smp, stat, c)
                for key, g, w in (('ps', got[smp]['whole'][stat]['PS'][c], want[smp]['whole'][stat]['PS'][c]),
                                  ('del2', got[smp]['whole'][stat]['Del2'][c], want[smp]['whole'][stat]['Del2'][c]),
                                  ('kc', gi['whole'][stat][c], wi['whole'][stat][c])):
                    assert type(g) is NP.ndarray
                    worst = max(worst, AK.compare(g, w, model[key + '_bound'], tag + ' ' + key))
                    bad = AK.cnan(g)
                    empty += int(bad.sum())
                    total += bad.size
                    assert bad.mean() == float(NP.mean(NP.asarray(wi['counts']) == 0)), (tag, key, 'NaN share')
    return worst, empty, total


# ---- the checker against the fixture ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', AVG_CASES)
def test_checker_against_the_fixture_averages(name):
    spec = AK.case(name)
    xs, es = AK.case_inputs(spec)
    combos = AK.diagoffsets_of(spec)
    seen = 0
    for which, sets, skip in (('x', xs, ()), ('e', es, (2,))):
        want = AK.gold_average(name, which)
        if want is None:
            continue
        for smp, pool, stat in pools_of(want):
            arrays, weights, masks = entry_arguments(sets, smp, pool, stat, combos, skip)
            res = AK.xavg(arrays, weights, masks, bounds=True)
            tag = 'checker %s %s %s %s %s' % (name, which, smp, pool, stat)
            if combos is None:
                AK.compare(res['avg'], want[smp][pool][stat], res['avg_bound'], tag)
                assert NP.array_equal(res['wsum'], want[smp][pool]['diagweights'])
            else:
                for c in range(len(combos)):
                    AK.compare(res['out'][c], want[smp][pool][stat][c], res['out_bound'][c], '%s [%d]' % (tag, c))
                    AK.compare(res['wout'][c], want[smp][pool]['diagweights'][c], 64 * AK.EPS * res['wout'][c], '%s wout [%d]' % (tag, c))
            seen += 1
    assert seen


@pytest.mark.parametrize('name', KBIN_CASES)
def test_checker_against_the_fixture_kbins(name):
    spec = AK.case(name)
    xin = AK.gold_average(spec['from'], 'x')
    res = BSP.incoherent_kbin_averaging(xin, ctx=AK.CheckerContext(), **AK.kbin_arguments(spec))
    worst, empty, total = check_kbin(res, name, xin, 'checker')
    print('%s: worst %.3f of the bounds, %d of %d values NaN' % (name, worst, empty, total))
    assert (empty > 0) == (name != 'k_linear')


def test_checker_layout_against_a_loop():
    """every index convention of the header, element by element"""
    rng = NP.random.default_rng(5)
    shape = (2, 3, 4, 3, 2)
    arrays = [rng.standard_normal(shape) + 1j * rng.standard_normal(shape) for _ in range(3)]
    weights = [rng.uniform(0.5, 2.0, (1, 3, 1, 3, 1)), rng.uniform(0.5, 2.0, (1, 1, 4, 1, 1)), rng.uniform(0.5, 2.0, (1, 3, 4, 3, 1))]
    arrays[1][1, 2, 3, 0, 1] = complex(NP.nan, 1.0)
    combo = {1: NP.asarray([True, False, True]), 3: NP.asarray([False, True, True])}
    res = AK.xavg(arrays, weights, [combo])
    assert res['wsum'].shape == (1, 3, 4, 3, 1) and res['out'][0].shape == (2, 1, 4, 1, 2) and res['wout'][0].shape == (1, 1, 4, 1, 1)
    W = weights[0] + weights[1] + weights[2]
    assert NP.allclose(res['wsum'], W, rtol=1e-15)
    e = (1, 2, 3, 0, 1)
    num = arrays[0][e] * weights[0][0, 2, 0, 0, 0] + arrays[2][e] * weights[2][0, 2, 3, 0, 0]      # the NaN of set 1 counts as 0 ...
    assert NP.allclose(res['avg'][e], num / W[0, 2, 3, 0, 0], rtol=1e-14)                        # ... and its weight still counts
    tot = wt = 0.0
    for i in (0, 2):
        for t in (1, 2):
            tot, wt = tot + res['avg'][0, i, 1, t, 1] * W[0, i, 1, t, 0], wt + W[0, i, 1, t, 0]
    assert NP.allclose(res['out'][0][0, 0, 1, 0, 1], tot / wt, rtol=1e-14) and NP.allclose(res['wout'][0][0, 0, 1, 0, 0], wt, rtol=1e-15)
    arrays[0][0, 0, 0, 1, 0] = NP.nan                                              # stage 2 propagates NaN only where stage 1 left it:
    assert not NP.any(AK.cnan(AK.xavg(arrays, weights, [combo])['out'][0]))        # 0 / weights there
    p = rng.standard_normal((2, 3, 5)) + 1j * rng.standard_normal((2, 3, 5))
    p[0, 1, 2] = NP.nan
    k = NP.asarray([[-2.0, -1.0, 0.0, 1.0, 2.0], [-4.0, -2.0, 0.0, 2.0, 4.0]])
    off, mem = NP.asarray([[0, 1, 3, 3], [0, 1, 1, 3]]), [NP.asarray([2, 1, 3]), NP.asarray([2, 0, 4])]
    res = AK.kbin(p, k, off, mem)
    assert res['ps'].shape == (2, 3, 3) and NP.all(AK.cnan(res['ps'][0, :, 2])) and NP.all(NP.isnan(res['kc'][1, :, 1]))
    assert NP.allclose(res['ps'][0, 0, 1], (p[0, 0, 1] + p[0, 0, 3]) / 2) and res['ps'][0, 1, 0] != res['ps'][0, 1, 0]
    assert NP.allclose(res['del2'][1, 2, 2], 64.0 * (p[1, 2, 0] + p[1, 2, 4]) / 2 / (2 * NP.pi ** 2))
    assert NP.allclose(res['kc'][1, 0, 2], 4.0) and NP.allclose(res['kc'][0, 1, 1], 1.0) and res['kc'][0, 0, 0] == 0.0 and NP.isnan(res['kc'][0, 1, 0])   # k = 0; nothing left: 0 / 0


# ---- the functions on the checker context -------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', AVG_CASES)
def test_average_on_the_checker_context_against_the_fixture(name):
    spec = AK.case(name)
    xs, es = AK.case_inputs(spec)
    ctx = AK.CheckerContext()
    before = copy.deepcopy((xs, es))
    outx, oute = BSP.incoherent_cross_power_spectrum_average(xs, excpdps=es, diagoffsets=AK.diagoffsets_of(spec), ctx=ctx)
    assert repr(before) == repr((xs, es))
    check_average(outx, name, 'x', xs, 'checker')
    if AK.gold_average(name, 'e') is not None:
        check_average(oute, name, 'e', es, 'checker')
    ncalls = sum(1 for d in (xs[0], es[0]) for _ in pools_of(d))
    assert len(ctx.xavg_calls) == ncalls                                        # one call per sampling, pool and statistic
    assert all(call['nsets'] == len(xs) for call in ctx.xavg_calls)
    assert NP.array_equal(outx['lstXoffsets'], xs[0]['lstXoffsets'])


def test_kbin_calls_one_per_combination_and_inputs_unmodified():
    xin = AK.gold_average('combos', 'x')
    before = copy.deepcopy(xin)
    ctx = AK.CheckerContext()
    res = BSP.incoherent_kbin_averaging(xin, kbintype='linear', ctx=ctx)
    assert repr(before) == repr(xin)
    assert len(ctx.kbin_calls) == 3 * 3                                         # 3 (sampling, statistic) pairs with 3 combinations each
    assert [c['nk'] for c in ctx.kbin_calls] == [5] * 3 + [3] * 6
    assert res['oversampled']['whole']['mean']['PS'][0].shape == (2, 1, 5, 5, 5)
    assert NP.array_equal(res['lstXoffsets'], xin['lstXoffsets'])


# ---- the departures -----------------------------------------------------------------------------------------------------------------

def test_departures_of_the_average():
    x0, x1, e0 = AK.data_set('x0'), AK.data_set('x1'), AK.data_set('e0')
    ctx = AK.CheckerContext()
    # excpdps=None: the second result is None
    outx, oute = BSP.incoherent_cross_power_spectrum_average(x0, ctx=ctx)
    assert oute is None and isinstance(outx['resampled']['whole']['median'], NP.ndarray)
    # one set under its own weights: the average is the set (0 / weights aside), the weights are the outer product of the diagweights
    assert NP.allclose(outx['resampled']['whole']['mean'], x0['resampled']['whole']['mean'], rtol=1e-15)
    assert outx['resampled']['whole']['diagweights'].shape == (1, 3, 5, 5, 1)
    assert outx['resampled']['whole']['diagweights'][0, 1, 2, 3, 0] == 3 * 3 * 2
    # a combination of axis 2 alone leaves no axis for excpdps: the stage-1 array itself
    _, oute = BSP.incoherent_cross_power_spectrum_average(x0, excpdps=e0, diagoffsets=[{2: [0]}, {3: [0]}], ctx=ctx)
    r = oute['oversampled']['errinfo']
    assert NP.array_equal(r['mean'][0], AK.xavg(*entry_arguments([e0], 'oversampled', 'errinfo', 'mean', None))['avg'])
    assert r['mean'][1].shape == (2, 3, 3, 1, 8) and r['diagweights'][0].shape == (1, 3, 1, 5, 1) and r['diagweights'][1].shape == (1, 3, 1, 1, 1)
    assert ctx.xavg_calls[-1]['want_avg'] and ctx.xavg_calls[-1]['combos'] == [[3]]
    # the stage-1 quirk: a NaN element becomes 0 / weights, so an all-NaN element comes out as 0
    x0['oversampled']['whole']['mean'][1, 2, 3, 4, 5] = NP.nan
    x1['oversampled']['whole']['mean'][1, 2, 3, 4, 5] = NP.nan
    outx, _ = BSP.incoherent_cross_power_spectrum_average([x0, x1], ctx=ctx)
    assert outx['oversampled']['whole']['mean'][1, 2, 3, 4, 5] == 0.0 and not NP.any(AK.cnan(outx['oversampled']['whole']['mean']))
    # axes of diagweights absent from diagoffsets (avgcov=True) have weight 1
    x2 = AK.data_set('x0')
    pool = x2['resampled']['whole']
    del pool['diagoffsets'][3]
    pool['mean'], pool['median'] = pool['mean'][:, :, :, :1], pool['median'][:, :, :, :1]
    outx, _ = BSP.incoherent_cross_power_spectrum_average(x2, diagoffsets={2: [0, 1]}, ctx=ctx)
    assert outx['resampled']['whole']['diagweights'][0].shape == (1, 3, 1, 1, 1) and outx['resampled']['whole']['mean'][0].shape == (2, 3, 1, 1, 4)
    assert NP.array_equal(outx['resampled']['whole']['diagweights'][0].ravel(), NP.asarray([4, 3, 2]) * 5.0)
    # lstXoffsets is carried when present and not asked for
    del x2['lstXoffsets']
    assert 'lstXoffsets' not in BSP.incoherent_cross_power_spectrum_average(x2, ctx=ctx)[0]


def test_departures_of_the_kbins():
    xin = AK.gold_average('combos', 'x')
    ctx = AK.CheckerContext()
    # a bare array is a list of one
    bare = copy.deepcopy(xin)
    for smp in AK.SAMPLINGS:
        for stat in AK.XSTATS[smp]:
            bare[smp]['whole'][stat] = bare[smp]['whole'][stat][1]
    res = BSP.incoherent_kbin_averaging(bare, kbintype='linear', ctx=ctx)
    full = BSP.incoherent_kbin_averaging(xin, kbintype='linear', ctx=ctx)
    assert len(res['resampled']['whole']['median']['PS']) == 1
    assert NP.array_equal(res['resampled']['whole']['median']['PS'][0], full['resampled']['whole']['median']['PS'][1])
    # kprll.shape[1] // 2 + 1 linear edges behind the edge at -eps: bin 0 holds k = 0 alone
    info = full['oversampled']['kbininfo']
    assert info['kbin_edges'][0].size == 8 // 2 + 2 and info['kbin_edges'][0][0] == -1e-10 and info['kbin_edges'][0][1] == 1e-10
    assert NP.array_equal(info['counts'][0], [1, 2, 2, 2, 1]) and NP.array_equal(info['ri'][0][:6], [6, 7, 9, 11, 13, 14])
    assert NP.array_equal(info['ri'][0][6:], [4, 3, 5, 2, 6, 1, 7, 0]) and NP.array_equal(info['kbinnum'][0], [5, 4, 3, 2, 1, 2, 3, 4])
    # 'log' without num_kbins: 10 bins and the bin of k = 0; the next sampling takes the number of bins of the one before, as the reference does
    res = BSP.incoherent_kbin_averaging(xin, ctx=ctx)
    assert res['oversampled']['kbininfo']['counts'][0].size == 11 and res['resampled']['kbininfo']['counts'][0].size == 12
    # explicit edges are used as given and lags outside every bin are dropped
    res = BSP.incoherent_kbin_averaging(xin, kbins=[0.1, 1e9], ctx=ctx)
    assert NP.array_equal(res['oversampled']['kbininfo']['counts'][0], [7]) and NP.array_equal(res['oversampled']['kbininfo']['kbin_edges'][1], [0.1, 1e9])
    assert NP.array_equal(res['oversampled']['kbininfo']['kbinnum'][0], [1, 1, 1, 1, 0, 1, 1, 1])


# ---- the errors ---------------------------------------------------------------------------------------------------------------------

def test_errors_are_raised_before_any_device_work():
    x0, e0 = AK.data_set('x0'), AK.data_set('e0')
    avg = BSP.incoherent_cross_power_spectrum_average
    no = Untouchable()
    for bad in (dict(xcpdps=3), dict(xcpdps=x0, excpdps=3), dict(xcpdps=x0, diagoffsets=3), dict(xcpdps=x0, diagoffsets=[3]),
                dict(xcpdps=x0, diagoffsets={1: 0})):
        with pytest.raises(TypeError):
            avg(ctx=no, **bad)
    with pytest.raises(ValueError, match='unequal'):
        avg([x0, x0], excpdps=[e0], ctx=no)
    with pytest.raises(ValueError, match='empty'):
        avg([], ctx=no)
    with pytest.raises(ValueError, match='not a collapsed axis'):
        avg(AK.data_set('f0'), diagoffsets={3: [0]}, ctx=no)                    # the triads of f0 are crossed and not collapsed
    with pytest.raises(ValueError, match='not a collapsed axis'):
        avg(x0, excpdps=e0, diagoffsets={4: [0]}, ctx=no)
    with pytest.raises(ValueError, match='no offset'):
        avg(x0, diagoffsets=[{1: [0]}, {3: [7]}], ctx=no)
    bad = AK.data_set('x0')
    for smp in AK.SAMPLINGS:
        bad[smp]['whole'].update(diagweights={}, diagoffsets={})
    avg(bad, ctx=AK.CheckerContext())                                            # nothing collapsed: a plain average
    with pytest.raises(ValueError, match='not a collapsed axis'):
        avg(bad, diagoffsets={1: [0]}, ctx=no)
    for smp in AK.SAMPLINGS:
        bad[smp]['whole'].update(diagoffsets=x0[smp]['whole']['diagoffsets'])
    with pytest.raises(ValueError, match='there are none'):
        avg(bad, diagoffsets={1: [0]}, ctx=no)                                  # an empty diagweights together with diagoffsets
    bad = AK.data_set('x0')
    bad['resampled']['whole']['diagweights'] = [1.0]
    with pytest.raises(TypeError, match='Diagonal weights'):
        avg(bad, ctx=no)
    bad['resampled']['whole']['diagweights'] = NP.ones((1, 3, 5, 4, 1))
    with pytest.raises(ValueError, match='broadcast'):
        avg(bad, ctx=no)
    bad = AK.data_set('x1')
    bad['resampled']['whole']['mean'] = bad['resampled']['whole']['mean'][:, :2]
    with pytest.raises(ValueError):
        avg([x0, bad], ctx=no)
    xin = AK.gold_average('combos', 'x')
    kb = BSP.incoherent_kbin_averaging
    for bad in (dict(xcpdps=[xin]), dict(xcpdps=xin, kbins=3), dict(xcpdps=xin, kbintype=3), dict(xcpdps=xin, num_kbins=2.5)):
        with pytest.raises(TypeError):
            kb(ctx=no, **bad)
    for bad in (dict(kbintype='cubic'), dict(num_kbins=0), dict(kbins=[1.0]), dict(kbins=[2.0, 1.0])):
        with pytest.raises(ValueError):
            kb(xin, ctx=no, **bad)
    short = copy.deepcopy(xin)
    short['resampled']['whole']['mean'][2] = short['resampled']['whole']['mean'][2][..., :3]
    with pytest.raises(ValueError, match='lags of kprll'):
        kb(short, kbintype='linear', ctx=no)


def test_the_context_validates_before_the_call():
    """Context.cphase_xavg and cphase_kbin check shapes and dtypes in Python: on an object whose library cannot be reached"""
    ctx = _abi.Context.__new__(_abi.Context)
    a, w = NP.zeros((2, 3, 3, 5, 4), dtype=NP.complex128), NP.ones((1, 3, 1, 5, 1))
    for arrays, weights, combos in (([], [], ()), ([a], [], ()), ([a, a[:1]], [w, w], ()), ([a[0]], [w[0]], ()), ([a], [NP.ones((1, 2, 1, 5, 1))], ()),
                                    ([a], [NP.ones((1, 3, 1, 5, 4))], ()), ([a], [w], [{}]), ([a], [w], [{0: [True, True]}]),
                                    ([a], [w], [{4: [True] * 4}]), ([a], [w], [{1: [True, False]}]), ([a], [w], [{1: [False] * 3}])):
        with pytest.raises(ValueError):
            ctx.cphase_xavg(arrays, weights, combos)
    p, k = NP.zeros((2, 6, 4), dtype=NP.complex128), NP.zeros((2, 4))
    off, mem = NP.asarray([[0, 2, 3], [0, 0, 1]]), [NP.asarray([0, 3, 1]), NP.asarray([2])]
    with pytest.raises(KeyError):
        ctx.cphase_kbin(p, k, off, mem, route='texture')
    for bad in (dict(p=p[:1]), dict(p=p[..., :3]), dict(offsets=off[:, :1]), dict(offsets=off[:1]), dict(members=mem[:1]),
                dict(offsets=NP.asarray([[1, 2, 3], [0, 0, 1]])), dict(offsets=NP.asarray([[0, 2, 1], [0, 0, 1]])),
                dict(members=[NP.asarray([0, 4, 1]), mem[1]]), dict(members=[NP.asarray([3, 0, 1]), mem[1]]),
                dict(members=[NP.asarray([0, 0, 1]), mem[1]]), dict(members=[NP.asarray([0, 3]), mem[1]])):
        args = dict(p=p, kprll=k, offsets=off, members=mem)
        args.update(bad)
        with pytest.raises(ValueError):
            ctx.cphase_kbin(**args)


# ---- the bindings -------------------------------------------------------------------------------------------------------------------

def test_stats_struct_mirrors_the_header():
    """PrisimCpavgStats field by field against include/prisim_cpavg.h, and its dict: keys in order, ints and floats as ctypes hands them"""
    st_type = _abi.Context.PrisimCpavgStats
    assert not any(k.startswith('Prisim') and 'Cpavg' in k for k in vars(_abi))
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'prisim_cpavg.h')).read()
    body = re.sub(r'/\*.*?\*/', '', header[header.index('typedef struct prisim_cpavg_stats'):header.index('} prisim_cpavg_stats;')], flags=re.S)
    fields = re.findall(r'(double|int64_t|int32_t)\s+(\w+);', body)
    assert [(n, {'double': C.c_double, 'int64_t': C.c_int64, 'int32_t': C.c_int32}[t]) for t, n in fields] == list(st_type._fields_)
    st = st_type()
    for k, (name, ctype) in enumerate(st_type._fields_):
        setattr(st, name, k + 1.5 if ctype is C.c_double else k + 2)
    st.route = _abi.PRISIM_CPAVG_GLOBAL
    got = _abi._stats_dict(st, route=_abi.CPAVG_ROUTES)
    assert got == {'wall_ms': 1.5, 'kernel_ms': 2.5, 'chunks': 4, 'kernel_bytes': 5, 'upload_bytes': 6, 'download_bytes': 7, 'route': 'global',
                   'lds_limit': 9}
    assert list(got) == [n for n, _ in st_type._fields_]
    assert all(type(got[k]) is (float if k.endswith('_ms') else str if k == 'route' else int) for k in got)
    assert _abi.CPAVG_EXPORTS == ('prisim_cphase_xavg', 'prisim_cphase_kbin')
    lib = _abi.load_library()
    assert all(hasattr(lib, name) for name in _abi.CPAVG_EXPORTS)
    for name in ('PRISIM_CPAVG_MIN_DIM', 'PRISIM_CPAVG_MAX_DIM'):
        assert getattr(_abi, name) == int(re.search(r'#define %s (\d+)' % name, header).group(1))
    for name in ('AUTO', 'LDS', 'GLOBAL'):
        assert getattr(_abi, 'PRISIM_CPAVG_' + name) == int(re.search(r'PRISIM_CPAVG_%s = (-?\d+)' % name, header).group(1))
