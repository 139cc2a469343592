"""GPU: the incoherent averages of closure-phase power spectra (prisim_cphase_xavg, prisim_cphase_kbin) and
prisim_amd.bispectrum_phase.incoherent_cross_power_spectrum_average / incoherent_kbin_averaging against the numpy checker
tests/cpavg_checker.py and tests/golden/golden_cpavg.npz (the reference's statements executed).

Bounds: cpavg_checker's docstring derives them; NaN positions match exactly.  Chunks and routes give the same bits."""
import ctypes as C
import os
import sys
import warnings

import numpy as NP
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cpavg_checker as AK  # noqa: E402
from test_cpft import closure_phase, ft_args  # noqa: E402
from test_cpavg import check_average, check_kbin  # noqa: E402

from prisim_amd import _abi  # noqa: E402
from prisim_amd import bispectrum_phase as BSP  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    with _abi.Context(0) as c:
        yield c


def sets(shape, seed, nsets=2, wshapes=None):
    """arrays and positive weights: by default every weight spans the axes 1 .. ndim - 2"""
    rng = NP.random.default_rng(seed)
    arrays = [rng.standard_normal(shape) + 1j * rng.standard_normal(shape) for _ in range(nsets)]
    full = (1,) + tuple(shape[1:-1]) + (1,)
    weights = [rng.uniform(0.5, 2.0, (wshapes[i] if wshapes else full)) for i in range(nsets)]
    return arrays, weights


def mask(n, *sel):
    m = NP.zeros(n, dtype=bool)
    m[list(sel)] = True
    return m


def run_xavg(ctx, arrays, weights, combos, label, **kw):
    res = ctx.cphase_xavg(arrays, weights, combos, **kw)
    worst = AK.compare_xavg(res, arrays, weights, combos, label=label)
    print('%s: worst %.3f of the bounds' % (label, worst))
    return res


def folded(kprll, edges):
    """(offsets, members) of the bins `edges` of |kprll| per window, as binned_count reads them"""
    offs, mems = [], []
    for row in NP.abs(kprll):
        counts, ri = BSP.binned_count(row, edges)
        offs.append(NP.concatenate(([0], NP.cumsum(counts))))
        mems.append(ri[counts.size + 1:])
    return NP.asarray(offs, dtype=NP.int64), mems


def spectra(nspw, m, nlags, seed):
    rng = NP.random.default_rng(seed)
    p = rng.standard_normal((nspw, m, nlags)) + 1j * rng.standard_normal((nspw, m, nlags))
    kprll = NP.asarray([0.4, 0.43])[:nspw].reshape(-1, 1) * (NP.arange(nlags) - nlags // 2).reshape(1, -1)
    return p, kprll


def kbin_edges(kprll, kind):
    eps, kmax, nlags = 1e-10, NP.abs(kprll).max(), kprll.shape[1]
    if kind == 'linear':
        return NP.insert(NP.linspace(eps, kmax + eps, num=nlags // 2 + 1), 0, -eps)
    if kind == 'log':
        return NP.insert(NP.geomspace(eps, kmax + eps, num=5), 0, -eps)
    return NP.asarray([0.0, 0.3 * kmax, 0.55 * kmax, 0.8 * kmax])


def run_kbin(ctx, p, kprll, off, mem, label, **kw):
    res = ctx.cphase_kbin(p, kprll, off, mem, **kw)
    worst = AK.compare_kbin(res, p, kprll, off, mem, label=label)
    print('%s: worst %.3f of the bounds, route %s' % (label, worst, res['stats']['route']))
    return res


# ---- the entries against the checker --------------------------------------------------------------------------------------------------

SHAPE = (2, 3, 3, 5, 5)
COMBOS = {'one axis': [{1: mask(3, 0, 1)}, {3: mask(5, 1, 2, 3)}, {2: mask(3, 2)}],
          'two axes': [{1: mask(3, 0), 3: mask(5, 2)}, {2: mask(3, 0, 2), 3: mask(5, 0, 1, 2, 3, 4)}, {1: mask(3, 0, 1, 2), 2: mask(3, 1), 3: mask(5, 4)}]}


@pytest.mark.parametrize('which', sorted(COMBOS))
def test_xavg_against_the_checker(ctx, which):
    arrays, weights = sets(SHAPE, 1)
    res = run_xavg(ctx, arrays, weights, COMBOS[which], which)
    assert res['stats']['chunks'] == 1 and res['stats']['route'] == -1 and res['stats']['lds_limit'] == 0
    assert not NP.any(AK.cnan(res['avg']))
    # weights of different broadcast shapes, one of them along one axis only; and without combinations only avg and wsum come back
    arrays, weights = sets(SHAPE, 2, nsets=3, wshapes=[(1, 3, 1, 5, 1), (1, 1, 3, 1, 1), (1, 1, 1, 1, 1)])
    res = run_xavg(ctx, arrays, weights, COMBOS[which], which + ', mixed weights')
    assert res['wsum'].shape == (1, 3, 3, 5, 1)
    res = run_xavg(ctx, arrays, weights, (), which + ', no combination')
    assert res['out'] == [] and res['wout'] == []
    assert run_xavg(ctx, arrays, weights, COMBOS[which], which + ', avg not wanted', want_avg=False)['avg'] is None


def test_xavg_carries_a_full_axis(ctx):
    arrays, weights = sets((2, 3, 3, 3, 5, 5), 3, wshapes=[(1, 3, 3, 1, 1, 1)] * 2)
    res = run_xavg(ctx, arrays, weights, [{1: mask(3, 0, 2)}, {2: mask(3, 1), 1: mask(3, 1, 2)}], 'a full axis carried')
    assert res['out'][1].shape == (2, 1, 1, 3, 5, 5) and res['wout'][0].shape == (1, 1, 3, 1, 1, 1)
    arrays, weights = sets((1, 2, 1, 2, 3, 1, 2, 3), 4)
    run_xavg(ctx, arrays, weights, [{3: mask(2, 1), 6: mask(2, 0, 1)}], 'eight axes')


def test_xavg_nan_elements(ctx):
    """one NaN element counts as 0 in the sum while its weight counts; an element that is NaN in every set comes out as 0; a NaN
    weight counts as 0 in both sums"""
    arrays, weights = sets(SHAPE, 5)
    arrays[0][1, 2, 0, 3, 4] = complex(NP.nan, 1.0)
    for a in arrays:
        a[0, 1, 1, 2, 0] = complex(2.0, NP.nan)
    res = run_xavg(ctx, arrays, weights, COMBOS['two axes'] + COMBOS['one axis'], 'NaN elements')
    assert not NP.any(AK.cnan(res['avg'])) and res['avg'][0, 1, 1, 2, 0] == 0.0
    weights[1][0, 0, 0, 0, 0] = NP.nan
    res = run_xavg(ctx, arrays, weights, COMBOS['one axis'][2:], 'a NaN weight')
    assert res['wsum'][0, 0, 0, 0, 0] == weights[0][0, 0, 0, 0, 0] and not NP.any(AK.cnan(res['avg']))


@pytest.mark.parametrize('nlags', [8, 7])
@pytest.mark.parametrize('kind', ['linear', 'log', 'edges'])
def test_kbin_against_the_checker(ctx, kind, nlags):
    p, kprll = spectra(2, 6, nlags, 6)
    off, mem = folded(kprll, kbin_edges(kprll, kind))
    p[1, 2, 1] = complex(NP.nan, 0.5)                                          # one NaN member
    p[0, 4, nlags // 2] = NP.nan                                               # all of bin 0 (k = 0 alone) of one row
    res = run_kbin(ctx, p, kprll, off, mem, '%s, %d lags' % (kind, nlags))
    empty = NP.diff(off, axis=1) == 0
    assert empty.any() or kind != 'log'                                        # 4 log bins from 1e-10 on: most are empty
    alone = off[0, 1] == 1 and mem[0][0] == nlags // 2                         # bin 0 of window 0 holds k = 0 alone: all NaN in row 4
    bad = AK.cnan(res['ps'])
    assert NP.array_equal(bad[:, 0], empty) and int(bad.sum()) == 6 * int(empty.sum()) + int(alone) and (alone or kind == 'edges')
    assert res['stats']['route'] == 'lds' and res['stats']['lds_limit'] >= 65536


def test_chunks_give_the_same_bits(ctx):
    arrays, weights = sets(SHAPE, 7)
    combos = COMBOS['two axes']
    one = ctx.cphase_xavg(arrays, weights, combos)
    assert one['stats']['chunks'] == 1
    rows, orows = 2 * 3 * 3 * 5, 2 * 3 + 2 * 3 + 2                             # per lag the chunk buffers hold avg and every out
    many = ctx.cphase_xavg(arrays, weights, combos, budget_bytes=2 * 2 * 16 * (rows + orows))
    assert many['stats']['chunks'] == 3                                         # 5 lags in ranges of 2
    for key in ('avg', 'wsum'):
        assert NP.array_equal(many[key].view(NP.uint64), one[key].view(NP.uint64))
    for key in ('out', 'wout'):
        assert all(NP.array_equal(a.view(NP.uint64), b.view(NP.uint64)) for a, b in zip(many[key], one[key]))
    assert many['stats']['download_bytes'] == one['stats']['download_bytes'] == sum(x.nbytes for x in [one['avg'], one['wsum']] + one['out'] + one['wout'])
    p, kprll = spectra(2, 6, 8, 8)
    off, mem = folded(kprll, kbin_edges(kprll, 'linear'))
    for route in ('lds', 'global'):
        one = ctx.cphase_kbin(p, kprll, off, mem, route=route)
        assert one['stats']['chunks'] == 2                                      # one per window
        many = ctx.cphase_kbin(p, kprll, off, mem, route=route, budget_bytes=2 * 2 * 40 * (off.shape[1] - 1))
        assert many['stats']['chunks'] == 6                                     # 6 rows in ranges of 2, per window
        for key in ('ps', 'del2', 'kc'):
            assert NP.array_equal(many[key].view(NP.uint64), one[key].view(NP.uint64)), (route, key)


def test_kbin_routes(ctx):
    """each route forced on one small input: the same bits; the global route alone takes a row one lag longer than the LDS holds"""
    p, kprll = spectra(2, 6, 7, 9)
    p[0, 1, 2] = NP.nan
    off, mem = folded(kprll, kbin_edges(kprll, 'log'))
    res = {route: run_kbin(ctx, p, kprll, off, mem, 'route ' + route, route=route) for route in ('auto', 'lds', 'global')}
    assert [res[r]['stats']['route'] for r in ('auto', 'lds', 'global')] == ['lds', 'lds', 'global']
    for key in ('ps', 'del2', 'kc'):
        assert NP.array_equal(res['lds'][key].view(NP.uint64), res['global'][key].view(NP.uint64)), key
        assert NP.array_equal(res['lds'][key].view(NP.uint64), res['auto'][key].view(NP.uint64)), key
    nlags = res['lds']['stats']['lds_limit'] // 16 + 1
    p, kprll = spectra(2, 2, nlags, 10)
    off, mem = folded(kprll, NP.insert(NP.geomspace(1e-10, NP.abs(kprll).max() + 1e-10, num=7), 0, -1e-10))
    assert run_kbin(ctx, p, kprll, off, mem, 'a row of %d lags' % nlags)['stats']['route'] == 'global'
    run_kbin(ctx, p, kprll, off, mem, 'a row of %d lags, forced' % nlags, route='global')
    with pytest.raises(ValueError, match='does not fit in LDS'):
        ctx.cphase_kbin(p, kprll, off, mem, route='lds')
    p, kprll = p[:, :, :nlags - 1], kprll[:, :nlags - 1]                        # the longest row that the LDS holds
    off, mem = folded(kprll, NP.insert(NP.geomspace(1e-10, NP.abs(kprll).max() + 1e-10, num=7), 0, -1e-10))
    a = run_kbin(ctx, p, kprll, off, mem, 'a row of %d lags' % (nlags - 1))
    b = ctx.cphase_kbin(p, kprll, off, mem, route='global')
    assert a['stats']['route'] == 'lds' and all(NP.array_equal(a[k].view(NP.uint64), b[k].view(NP.uint64)) for k in ('ps', 'del2', 'kc'))


# ---- the functions on the device ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', [c['name'] for c in AK.cases() if c['kind'] == 'avg'])
def test_average_against_the_fixture(ctx, name):
    spec = AK.case(name)
    xs, es = AK.case_inputs(spec)
    outx, oute = BSP.incoherent_cross_power_spectrum_average(xs, excpdps=es, diagoffsets=AK.diagoffsets_of(spec), ctx=ctx)
    worst = check_average(outx, name, 'x', xs, 'device')                       # asserts a NaN share of 0 too
    if AK.gold_average(name, 'e') is not None:
        worst = max(worst, check_average(oute, name, 'e', es, 'device'))
    print('%s: worst %.3f of the bounds against the reference' % (name, worst))


@pytest.mark.parametrize('name', [c['name'] for c in AK.cases() if c['kind'] == 'kbin'])
def test_kbins_against_the_fixture(ctx, name):
    spec = AK.case(name)
    xin = AK.gold_average(spec['from'], 'x')
    res = BSP.incoherent_kbin_averaging(xin, ctx=ctx, **AK.kbin_arguments(spec))
    worst, empty, total = check_kbin(res, name, xin, 'device')                  # asserts the NaN share empty bins / nk per array
    print('%s: worst %.3f of the bounds against the reference, %d of %d values NaN' % (name, worst, empty, total))


class Checked(object):
    """the device context with every cphase_xavg and cphase_kbin call compared against the checker on the call's own arguments"""

    def __init__(self, ctx):
        self._ctx, self.device, self.worst, self.calls = ctx, ctx.device, 0.0, {'xavg': 0, 'kbin': 0}

    def __getattr__(self, name):
        return getattr(self._ctx, name)

    def cphase_xavg(self, arrays, weights, combos=(), **kw):
        res = self._ctx.cphase_xavg(arrays, weights, combos, **kw)
        self.worst = max(self.worst, AK.compare_xavg(res, arrays, weights, combos, label='end to end xavg'))
        self.calls['xavg'] += 1
        return res

    def cphase_kbin(self, p, kprll, offsets, members, **kw):
        res = self._ctx.cphase_kbin(p, kprll, offsets, members, **kw)
        self.worst = max(self.worst, AK.compare_kbin(res, p, kprll, offsets, members, label='end to end kbin'))
        self.calls['kbin'] += 1
        return res


def test_end_to_end_from_raw_phases(ctx):
    """smooth_in_tbins, subsample_differencing, FT, both power spectra, their incoherent average and the k-bins on the device from raw
    phases; every call of the two new entries against the checker on its own arguments"""
    name = 'noflags'
    chk = Checked(ctx)
    cp = closure_phase(name, chk, fill=False)
    cp.cpinfo['raw']['triads'] = NP.asarray([[0, 1, 2]])
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        cp.smooth_in_tbins(ndaybins=2, lstbinsize=1008.0)
        cp.subsample_differencing(ndaybins=4, lstbinsize=1008.0)
    ds = BSP.ClosurePhaseDelaySpectrum(cp)
    bw, kw = ft_args(name, apply_flags=True)
    ds.FT(bw, **kw)
    xps = ds.compute_power_spectrum(xinfo={'axes': [1, 2], 'collapse_axes': [2, 1], 'avgcov': False}, units='Jy')
    unc = ds.compute_power_spectrum_uncertainty(xinfo={'axes': [1, 2, 3], 'collapse_axes': [1]}, units='Jy')
    combos = [{2: [0]}, {1: [0], 2: [-1, 0, 1]}]
    avx, ave = BSP.incoherent_cross_power_spectrum_average([xps, xps], excpdps=[unc, unc], diagoffsets=combos, ctx=chk)
    assert chk.calls['xavg'] == 2 * 2 + 2 * 2                                   # 'whole' and 'errinfo': 2 samplings x 2 statistics each
    nlags = {'oversampled': ds.cPhaseDS['lags'].size, 'resampled': ds.cPhaseDS_resampled['lags'].size}
    for smp in nlags:
        r, e = avx[smp]['whole'], ave[smp]['errinfo']
        assert [a.shape for a in r['mean']] == [(1, 2, 1, 1, nlags[smp]), (1, 1, 1, 1, nlags[smp])]
        assert [a.shape for a in e['median']] == [(1, 2, 3, 1, 1, nlags[smp]), (1, 1, 3, 1, 1, nlags[smp])]   # axis 2 does not apply
        assert r['diagweights'][1].shape == (1, 1, 1, 1, 1) and r['diagweights'][1].ravel()[0] == 2 * 2 * (1 + 2 + 1)
        # two copies of one data set average to that set
        assert NP.allclose(r['mean'][0], xps[smp]['whole']['mean'][:, :, [1]], rtol=1e-14, atol=0)
        assert all(NP.all(NP.isfinite(a)) for a in r['mean'] + r['median'])
    psx = BSP.incoherent_kbin_averaging(avx, kbintype='linear', ctx=chk)
    pse = BSP.incoherent_kbin_averaging(ave, kbintype='log', num_kbins=4, ctx=chk)
    assert chk.calls['kbin'] == 2 * (2 * 2 * 2)
    for smp in nlags:
        nk = nlags[smp] // 2 + 1
        assert psx[smp]['whole']['mean']['PS'][0].shape == (1, 2, 1, 1, nk) and psx[smp]['kbininfo']['whole']['median'][1].shape == (1, 1, 1, 1, nk)
        counts = psx[smp]['kbininfo']['counts'][0]
        assert NP.array_equal(AK.cnan(psx[smp]['whole']['mean']['Del2'][1])[0, 0, 0, 0], counts == 0)
        assert 'errinfo' in pse[smp] and len(pse[smp]['errinfo']['mean']['PS']) == 2
    print('end to end: worst %.3f of the bounds over %d + %d calls' % (chk.worst, chk.calls['xavg'], chk.calls['kbin']))


# ---- argument errors on the C entries -------------------------------------------------------------------------------------------------

def test_argument_errors_leave_the_outputs_untouched(ctx):
    lib, P = ctx._lib, _abi._ptr
    shape = NP.asarray([2, 3, 3, 5, 4], dtype=NP.int64)
    a = NP.ones(tuple(shape), dtype=NP.complex128)
    w = NP.ones((1, 3, 1, 5, 1))
    wshape = NP.asarray([[1, 3, 1, 5, 1]], dtype=NP.int64)
    sel = NP.ones(5, dtype=NP.uint8)
    avg, wsum, out, wout = NP.full(a.shape, 7.0 + 7.0j), NP.full(w.shape, 7.0), NP.full((2, 1, 3, 5, 4), 7.0 + 7.0j), NP.full((1, 1, 1, 5, 1), 7.0)

    def xavg(h=ctx._h, shape=shape, wshape=wshape, reduce=(0, 1, 0, 0, 0), ncombo=1):
        red = NP.asarray([reduce], dtype=NP.int32)
        masks = (C.c_void_p * 5)(*[sel.ctypes.data if r else None for r in reduce])
        return lib.prisim_cphase_xavg(h, 5, P(shape), 1, (C.c_void_p * 1)(a.ctypes.data), (C.c_void_p * 1)(w.ctypes.data), P(wshape), ncombo,
                                      P(red), masks, 0, P(avg), P(wsum), (C.c_void_p * 1)(out.ctypes.data), (C.c_void_p * 1)(wout.ctypes.data),
                                      None)

    assert xavg(h=None) == _abi.PRISIM_EINVAL                                   # a NULL context
    zero = shape.copy()
    zero[4] = 0
    assert xavg(shape=zero) == _abi.PRISIM_EINVAL                               # zero lags
    assert xavg(wshape=NP.asarray([[1, 2, 1, 5, 1]], dtype=NP.int64)) == _abi.PRISIM_EINVAL      # neither 1 nor the axis'
    assert xavg(wshape=NP.asarray([[1, 3, 1, 5, 4]], dtype=NP.int64)) == _abi.PRISIM_EINVAL      # weights along the lags
    assert xavg(reduce=(1, 0, 0, 0, 0)) == _abi.PRISIM_EINVAL                   # a combination that reduces the windows
    assert xavg(reduce=(0, 0, 0, 0, 1)) == _abi.PRISIM_EINVAL                   # ... or the lags
    assert 'reduces the windows or the lags' in lib.prisim_hip_last_error(ctx._h).decode()
    sel[:] = 0
    assert xavg() == _abi.PRISIM_EINVAL                                         # nothing selected
    sel[:] = 1
    assert all(NP.all(x == 7.0 + 7.0j) for x in (avg, out)) and all(NP.all(x == 7.0) for x in (wsum, wout))
    assert xavg() == _abi.PRISIM_OK and NP.all(avg == 1.0) and NP.all(out == 1.0) and NP.all(wsum == 1.0) and NP.all(wout == 3.0)

    p, kprll = NP.ones((2, 3, 4), dtype=NP.complex128), NP.ones((2, 4))
    ps, del2, kc = NP.full((2, 3, 2), 7.0 + 7.0j), NP.full((2, 3, 2), 7.0 + 7.0j), NP.full((2, 3, 2), 7.0)

    def kbin(h=ctx._h, nlags=4, off=((0, 2, 3), (0, 1, 3)), mem=(0, 3, 1, 2, 0, 1), route=-1):
        off, mem = NP.asarray(off, dtype=NP.int64), NP.asarray(mem, dtype=NP.int32)
        return lib.prisim_cphase_kbin(h, 2, 3, nlags, 2, P(p), P(kprll), P(off), P(mem), route, 0, P(ps), P(del2), P(kc), None)

    assert kbin(h=None) == _abi.PRISIM_EINVAL
    assert kbin(nlags=0) == _abi.PRISIM_EINVAL
    assert kbin(mem=(0, 4, 1, 2, 0, 1)) == _abi.PRISIM_EINVAL                   # a member out of range
    assert kbin(mem=(0, -1, 1, 2, 0, 1)) == _abi.PRISIM_EINVAL
    assert kbin(mem=(3, 0, 1, 2, 0, 1)) == _abi.PRISIM_EINVAL                   # members that do not increase
    assert kbin(mem=(0, 0, 1, 2, 0, 1)) == _abi.PRISIM_EINVAL
    assert kbin(off=((0, 2, 1), (0, 1, 3))) == _abi.PRISIM_EINVAL               # offsets that decrease
    assert kbin(off=((1, 2, 3), (0, 1, 3))) == _abi.PRISIM_EINVAL               # ... or do not start at 0
    assert kbin(route=2) == _abi.PRISIM_EINVAL
    assert NP.all(ps == 7.0 + 7.0j) and NP.all(del2 == 7.0 + 7.0j) and NP.all(kc == 7.0)
    assert kbin() == _abi.PRISIM_OK and NP.all(ps == 1.0) and NP.all(kc == 1.0)


# ---- one larger shape -----------------------------------------------------------------------------------------------------------------

def timing(st, label):
    print('   %s: kernel %.3f ms, wall %.3f ms, %.1f GB/s of %d kernel bytes, %d chunks' % (
        label, st['kernel_ms'], st['wall_ms'], st['kernel_bytes'] / max(st['kernel_ms'], 1e-9) / 1e6, st['kernel_bytes'], st['chunks']))


def test_a_larger_shape(ctx):
    """informational timings, no threshold"""
    p, kprll = spectra(2, 600, 1024, 11)
    off, mem = folded(kprll, kbin_edges(kprll, 'linear'))
    want = AK.kbin(p, kprll, off, mem, bounds=True)
    for route in ('lds', 'global'):
        res = ctx.cphase_kbin(p, kprll, off, mem, route=route)
        worst = max(AK.compare(res[key], want[key], want[key + '_bound'], 'kbin (2, 600, 1024) %s %s' % (route, key)) for key in ('ps', 'del2', 'kc'))
        assert res['stats']['route'] == route and res['stats']['chunks'] == 2 and worst <= 1.0
        timing(res['stats'], 'kbin (2, 600, 1024), %d bins, route %s' % (off.shape[1] - 1, route))
    arrays, weights = sets((2, 2, 5, 47, 1024), 12)
    combos = [{3: mask(47, *range(20, 27))}, {2: mask(5, 2), 3: mask(47, 23)}]
    res = run_xavg(ctx, arrays, weights, combos, 'xavg 2 x (2, 2, 5, 47, 1024)')
    timing(res['stats'], 'xavg 2 sets of (2, 2, 5, 47, 1024), 2 combinations')
