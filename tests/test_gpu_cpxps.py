"""GPU: the cross power of closure-phase delay spectra (prisim_cphase_xpower) and the power spectra of
prisim_amd.bispectrum_phase.ClosurePhaseDelaySpectrum against tests/golden/golden_cpxps.npz (the reference's statements executed) and
the numpy checker tests/cpxps_checker.py.

Bounds (cpxps_checker.compare).  Uncollapsed outputs equal the checker bit for bit, NaN positions included.  Collapsed outputs:
|got - want| <= (L + 8) 2^-52 S, L the terms of the longest reduction behind the element, S = factor sum |a wa| |b wb| over those terms
(the largest term for a median).  The share of NaN is exactly sum s / (nshift n1) where the LST axis is crossed and not collapsed and
0 otherwise."""
import os
import sys
import warnings

import numpy as NP
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cpxps_checker as XK  # noqa: E402
from test_cpft import closure_phase, ft_args  # noqa: E402
from test_cpxps import check_case, run_case, spectrum_object  # noqa: E402

from prisim_amd import _abi  # noqa: E402
from prisim_amd import bispectrum_phase as BSP  # noqa: E402
from prisim_amd import delay_spectrum as DS  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    with _abi.Context(0) as c:
        yield c


def stacks(shape, seed, same=False):
    """a, b, factor and complex weights of the three axes"""
    rng = NP.random.default_rng(seed)
    a = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    b = None if same else rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    w = [rng.uniform(0.5, 1.5, n) * NP.exp(2j * NP.pi * rng.uniform(size=n)) for n in shape[1:4]]
    return a, b, rng.uniform(0.5, 2.0, shape[0]), w


def run(ctx, a, b, f, w, modes, shifts, order, stat, label, **kw):
    res = ctx.cphase_xpower(a, b=b, factor=f, weights=w, modes=modes, shifts=shifts, collapse=order, stat=stat,
                            budget_bytes=kw.pop('budget_bytes', 0))
    XK.compare(res['out'], a, b, f, w, modes, shifts, order, stat, label=label, **kw)
    return res


@pytest.mark.parametrize('name,modes,order', [('x13_c13', ('collapse', 'none', 'collapse'), [1, 3]), ('x23_c23', ('none', 'collapse', 'collapse'), [2, 3]),
                                              ('selection', ('full', 'collapse', 'full'), [2]), ('unc_x13_c3', ('full', 'none', 'collapse'), [3])])
def test_entry_against_the_fixture(ctx, name, modes, order):
    """the cases of the fixture that are one call of the entry, within the entry's bound of the reference"""
    spec = XK.case(name)
    _, _, cpds = XK.gold_inputs()
    for (smp, pool, stat), want in XK.gold_outputs(name).items():
        ds = cpds[smp]
        if pool == 'errinfo':
            a, b = ds['errinfo']['dspec0'][stat], ds['errinfo']['dspec1'][stat]
        else:
            a, b = (ds[pool]['dspec'] if pool == 'submodel' else ds[pool]['dspec'][stat]), None
        if 'selection' in spec:
            lst = NP.asarray(spec['selection']['lst'])
            tri = NP.asarray([XK.gold()['in__triads'].tolist().index(t) for t in spec['selection']['triads']])
            a = NP.ascontiguousarray(a[:, lst][:, :, :, tri])
        fac = XK.gold()['in__%s__factor' % smp]
        res = ctx.cphase_xpower(a, b=b, factor=fac, modes=modes, shifts=[0, 1], collapse=order, stat=stat)
        got = XK.as_reference(res['out'], modes)
        lim = XK.as_reference(XK.bound(a, b, fac, None, modes, [0, 1], order, stat), modes)
        bad = XK.cnan(want)
        assert got.shape == want.shape and NP.array_equal(XK.cnan(got), bad) and bad.mean() == XK.nan_share(modes, [0, 1], a.shape[1])
        share = float(NP.max(NP.abs(got - want)[~bad] / lim[~bad]))
        print('%s %s %s %s: %.3f of the bound against the reference' % (name, smp, pool, stat, share))
        assert share <= 1.0
        assert res['stats']['chunks'] == 2 and res['stats']['chunk_lags'] == a.shape[4]


# n1 = 5 with the shifts 0, 2, 4: medians of 5, 3 and 1 values; every mode of every axis; both orders of a pair of collapses
COMBOS = [(('none', 'none', 'none'), []), (('full', 'full', 'full'), []), (('full', 'none', 'collapse'), [3]),
          (('collapse', 'none', 'collapse'), [1, 3]), (('collapse', 'none', 'collapse'), [3, 1]), (('full', 'collapse', 'collapse'), [3, 2]),
          (('collapse', 'collapse', 'collapse'), [2, 1, 3]), (('collapse', 'full', 'none'), [1]), (('none', 'collapse', 'full'), [2])]


@pytest.mark.parametrize('stat', ['mean', 'median'])
@pytest.mark.parametrize('modes,order', COMBOS)
def test_entry_against_the_checker(ctx, modes, order, stat):
    a, b, f, w = stacks((2, 5, 3, 4, 7), 1)
    run(ctx, a, b, f, w, modes, [0, 2, 4], order, stat, 'b != a %s %s %s' % (modes, order, stat))


@pytest.mark.parametrize('stat', ['mean', 'median'])
def test_one_triad_even_medians_and_b_is_a(ctx, stat):
    """n3 = 1; n1 = 4 with the shifts 0 and 1: medians of 4 and 3 values; b = a without weights"""
    a, _, f, w = stacks((2, 4, 2, 1, 5), 2, same=True)
    run(ctx, a, None, f, w, ('collapse', 'full', 'collapse'), [0, 1], [3, 1], stat, 'n3 = 1 ' + stat)
    run(ctx, a, None, None, None, ('collapse', 'collapse', 'full'), [0, 1, 2, 3], [1, 2], stat, 'b = a, no weights ' + stat)


@pytest.mark.parametrize('stat', ['mean', 'median'])
def test_an_input_row_of_nan(ctx, stat):
    """a row of NaN in a: it is skipped by the LST collapse and propagates through a trace, as in numpy"""
    a, b, f, w = stacks((2, 5, 2, 3, 6), 3)
    a[:, 2, 1, 0, :] = NP.nan
    a[0, 4, 0, 1, 2] = complex(NP.nan, 1.0)                                     # NaN in the real part alone
    b[1, 0, 1, 2, 3] = complex(2.0, NP.nan)                                     # and in the imaginary part alone
    for modes, order in ((('collapse', 'none', 'full'), [1]), (('collapse', 'none', 'collapse'), [3, 1]), (('collapse', 'none', 'collapse'), [1, 3]),
                         (('full', 'none', 'collapse'), [3]), (('full', 'full', 'none'), [])):
        res = run(ctx, a, b, f, w, modes, [0, 1, 3], order, stat, 'NaN row %s %s %s' % (modes, order, stat), structural_only=False)
        if order == [1]:
            assert not NP.any(XK.cnan(res['out']))                              # every other LST bin is left
        if order == [3]:
            assert XK.nan_share(modes, [0, 1, 3], 5) < XK.cnan(res['out']).mean() < 1.0     # the traces over the row are NaN too


def test_lag_ranges_give_the_same_bits(ctx):
    """nlags = 33 under a budget that holds 11 lags per chunk: three lag ranges per window, bit for bit the result of one chunk"""
    a, b, f, w = stacks((2, 5, 3, 4, 33), 4)
    for modes, order, stat, elems in ((('collapse', 'none', 'collapse'), [1, 3], 'median', (3 * 5 * 3 * 16, 3 * 3 * 16)),
                                      (('collapse', 'none', 'collapse'), [3, 1], 'mean', (3 * 5 * 3 * 16, 3 * 5 * 3 * 7)),
                                      (('full', 'none', 'full'), [], 'mean', (3 * 5 * 3 * 16, 0))):
        one = run(ctx, a, b, f, w, modes, [0, 2, 4], order, stat, 'one chunk %s' % (order,))
        assert one['stats']['chunks'] == 2 and one['stats']['chunk_lags'] == 33
        # per lag the two ping-pong buffers hold the product and the result of the first collapse; two streams share the budget
        budget = 2 * 11 * 16 * sum(elems)
        many = ctx.cphase_xpower(a, b=b, factor=f, weights=w, modes=modes, shifts=[0, 2, 4], collapse=order, stat=stat, budget_bytes=budget)
        assert many['stats']['chunk_lags'] == 11 and many['stats']['chunks'] == 6
        assert NP.array_equal(many['out'].view(NP.uint64), one['out'].view(NP.uint64))
        assert many['stats']['cross_bytes'] == 2 * 33 * elems[0] * 16 == one['stats']['cross_bytes']
        if order:
            assert many['stats']['download_bytes'] == many['out'].nbytes < many['stats']['cross_bytes']


def test_median_limit(ctx):
    """256 LST bins are the most a median takes; 257 are refused for the median only"""
    a, _, f, _ = stacks((1, 256, 1, 1, 3), 5, same=True)
    run(ctx, a, None, f, None, ('collapse', 'none', 'none'), [0, 1], [1], 'median', 'n1 = 256 median')
    a, _, f, _ = stacks((1, 257, 1, 1, 3), 6, same=True)
    with pytest.raises(ValueError, match='PRISIM_CPXPS_MAX_MEDIAN'):
        ctx.cphase_xpower(a, factor=f, modes=('collapse', 'none', 'none'), shifts=[0, 1], collapse=[1], stat='median')
    run(ctx, a, None, f, None, ('collapse', 'none', 'none'), [0, 1], [1], 'mean', 'n1 = 257 mean')
    run(ctx, a, None, f, None, ('full', 'none', 'none'), [0, 256], [], 'median', 'n1 = 257 uncollapsed')


def test_a_larger_shape(ctx):
    a, b, f, w = stacks((2, 6, 1, 24, 256), 7)
    for order, stat in (([3, 1], 'median'), ([1, 3], 'mean')):
        res = run(ctx, a, b, f, w, ('collapse', 'none', 'collapse'), [0, 1], order, stat, 'n3 = 24, 256 lags %s %s' % (order, stat))
        st = res['stats']
        assert st['chunks'] == 2 and st['cross_bytes'] == 2 * 256 * (2 * 6 * 24 * 24) * 16 and st['download_bytes'] == res['out'].nbytes
        print('   kernel %.3f ms, wall %.3f ms, %.1f GB/s of %d kernel bytes' % (st['kernel_ms'], st['wall_ms'],
                                                                              st['kernel_bytes'] / max(st['kernel_ms'], 1e-9) / 1e6, st['kernel_bytes']))


def test_argument_errors(ctx):
    a, b, f, w = stacks((2, 3, 2, 2, 4), 8)
    ok = dict(modes=('collapse', 'none', 'collapse'), shifts=[0, 1], collapse=[1, 3])
    for bad in (dict(ok, shifts=[0, 3]), dict(ok, shifts=[-1]), dict(ok, shifts=[]), dict(ok, collapse=[1]), dict(ok, collapse=[1, 2]),
                dict(ok, collapse=[1, 1]), dict(ok, collapse=[1, 3, 2]), dict(ok, modes=('none', 'none', 'none')),
                dict(ok, factor=NP.ones(3)), dict(ok, weights=[NP.ones(2), None, None]), dict(ok, b=a[:1])):
        with pytest.raises(ValueError):
            ctx.cphase_xpower(a, **bad)
    with pytest.raises(KeyError):
        ctx.cphase_xpower(a, stat='mode', **ok)
    with pytest.raises(KeyError):
        ctx.cphase_xpower(a, modes=('all', 'none', 'none'))
    lib, out = ctx._lib, NP.full(8, 7.0)
    modes = NP.zeros(3, dtype=NP.int32)
    fac = NP.ones(1)
    assert lib.prisim_cphase_xpower(ctx._h, 1, 1, 1, 1, 0, _abi._ptr(a), None, _abi._ptr(fac), None, _abi._ptr(modes), 0, None, 0, None, 0, 0,
                                    _abi._ptr(out), None) == _abi.PRISIM_EINVAL
    assert lib.prisim_cphase_xpower(ctx._h, 1, 1, 1, 1, 1, _abi._ptr(a), None, _abi._ptr(fac), None, _abi._ptr(modes), 0, None, 0, None, 2, 0,
                                    _abi._ptr(out), None) == _abi.PRISIM_EINVAL
    assert lib.prisim_cphase_xpower(None, 1, 1, 1, 1, 1, _abi._ptr(a), None, _abi._ptr(fac), None, _abi._ptr(modes), 0, None, 0, None, 0, 0,
                                    _abi._ptr(out), None) == _abi.PRISIM_EINVAL
    assert NP.all(out == 7.0)                                                   # nothing is written on an argument error


@pytest.mark.parametrize('name', [c['name'] for c in XK.cases()])
def test_class_against_the_fixture(ctx, name):
    _, _, cpds = XK.gold_inputs()
    obj = spectrum_object(ctx)
    res = run_case(obj, name)
    check_case(res, name, cpds, label='device')
    assert len(obj.xps_stats) == (4 if XK.case(name)['unc'] else 12)


class Checked(object):
    """the device context with every cphase_xpower call compared against the checker on the call's own arguments"""

    def __init__(self, ctx):
        self._ctx, self.device, self.worst, self.calls = ctx, ctx.device, 0.0, 0

    def __getattr__(self, name):
        return getattr(self._ctx, name)

    def cphase_xpower(self, a, b=None, factor=None, weights=None, modes=('none', 'none', 'none'), shifts=None, collapse=(), stat='mean',
                      budget_bytes=0):
        res = self._ctx.cphase_xpower(a, b=b, factor=factor, weights=weights, modes=modes, shifts=shifts, collapse=collapse, stat=stat,
                                      budget_bytes=budget_bytes)
        self.worst = max(self.worst, XK.compare(res['out'], a, b, factor, weights, modes, shifts, list(collapse), stat,
                                                label='end to end %s %s %s' % (modes, list(collapse), stat)))
        self.calls += 1
        return res


def test_end_to_end_from_raw_phases(ctx):
    """smooth_in_tbins, subsample_differencing, FT and both power spectra on the device from raw phases; every cross-power call against
    the checker fed FT's output"""
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
    xinfo = {'axes': [1, 2], 'collapse_axes': [2, 1], 'avgcov': False}
    res = ds.compute_power_spectrum(xinfo=xinfo, units='Jy')
    nlst, ndays = cp.cpinfo['processed']['prelim']['wts'].shape[:2]
    assert (nlst, ndays) == (2, 2) and chk.calls == 4                           # no model was subtracted: 'whole' x 2 statistics x 2 samplings
    for smp, m in (('oversampled', ds.cPhaseDS), ('resampled', ds.cPhaseDS_resampled)):
        r = res[smp]['whole']
        assert r['mean'].shape == (1, 2, 2 * ndays - 1, 1, m['lags'].size) and r['median'].dtype == NP.complex128
        assert NP.array_equal(r['diagoffsets'][2], [-1, 0, 1]) and NP.array_equal(r['diagweights'][1], [2, 1])
        assert NP.all(NP.isfinite(r['mean'])) and NP.all(NP.isfinite(r['median']))
    unc = ds.compute_power_spectrum_uncertainty(xinfo={'axes': [1, 2, 3], 'collapse_axes': [1]}, units='Jy')
    assert chk.calls == 8
    assert unc['oversampled']['errinfo']['mean'].shape == (1, 2, 3, 1, 1, ds.cPhaseDS['lags'].size)
    print('end to end: worst %.3f of the bound over %d calls' % (chk.worst, chk.calls))


def test_kelvin_over_jansky_is_the_ratio_of_the_factors(ctx):
    """units='K' with a Gaussian element at nside 16: the K result over the Jy result is the ratio of the two factors, formed here from
    delay_spectrum's own functions, to 1e-13"""
    import scipy.constants as FCNST
    obj = spectrum_object(ctx)
    tel = {'shape': 'gaussian', 'size': 14.0}
    xinfo = {'axes': [1, 3], 'collapse_axes': [3]}
    cpds = {'oversampled': obj.cPhaseDS}
    jy = obj.compute_power_spectrum(cpds=cpds, xinfo=xinfo, units='Jy')
    for parms in ({'telescope': tel, 'nside': 16}, {'telescope': tel, 'nside': 16, 'chromatic': False}):
        before = dict(parms)
        kk = obj.compute_power_spectrum(cpds=cpds, xinfo=xinfo, units='K', beamparms=parms)
        assert parms == before
        fc, bw = obj.cPhaseDS['freq_center'], obj.cPhaseDS['bw_eff']
        z = DS.REST_FREQ_HI / fc - 1
        f = obj.f if parms.get('chromatic', True) else NP.asarray([NP.mean(obj.f)])
        omega = DS.beam3Dvol(DS.healpix_power_pattern(f, tel, nside=16), obj.f, freq_wts=obj.cPhaseDS['freq_wts'])
        rz = DS.cosmo100.comoving_distance(z).to('Mpc').value
        ratio = bw * rz ** 2 / omega * ((FCNST.c / fc) ** 2 * DS.JY / (2 * FCNST.k)) ** 2
        with NP.errstate(invalid='ignore'):
            got = kk['oversampled']['whole']['mean'] / jy['oversampled']['whole']['mean']
        ok = ~XK.cnan(jy['oversampled']['whole']['mean'])
        assert NP.array_equal(XK.cnan(kk['oversampled']['whole']['mean']), ~ok)
        err = NP.max(NP.abs(got / ratio.reshape(-1, 1, 1, 1, 1, 1) - 1.0)[ok])
        print('K over Jy (chromatic %s): ratio %s, largest relative deviation %.3e' % (parms.get('chromatic', True), ratio, err))
        assert err <= 1e-13
