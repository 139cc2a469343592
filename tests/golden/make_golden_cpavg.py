"""Regenerate tests/golden/golden_cpavg.npz from the reference's own incoherent_cross_power_spectrum_average and
incoherent_kbin_averaging.

At generation time this reads the statements of the two functions (prisim/bispectrum_phase.py :1068-1231 and :1411-1493) from a PRISim
checkout and executes them under Python 3.  The stand-in namespace supplies an ndarray subclass with .si, .value and .unit in the place
of a Quantity; U.Unit(...) = U.Mpc = 1; NP.int / bool / complex / float; an NP.linspace that truncates `num` (the reference's / is
Python 2); OPS.binned_statistic in the reading of prisim_amd.bispectrum_phase.binned_statistic_count; a progress bar and a print that do
nothing.  No reference text is stored: only inputs and outputs.

The inputs are seeded random power spectra with the dictionary layout of compute_power_spectrum (tests/cpavg_checker.py:SETS and
data_set state it).  This script asserts that the averaged outputs hold no NaN and no masked element and that the k-binned outputs are
NaN exactly at the bins whose count is 0, and refuses to write the file otherwise.

    python tests/golden/make_golden_cpavg.py /path/to/PRISim
"""
import copy
import io
import json
import os
import sys
import textwrap
import types
import warnings

import numpy as NP
import numpy.ma as MA

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
from prisim_amd import dsp_readings as DSP  # noqa: E402
from prisim_amd import bispectrum_phase as BSP  # noqa: E402
import cpavg_checker as AK  # noqa: E402

NAN_AT = (((1 * 3 + 1) * 5 + 2) * 5 + 2) * 8 + 3          # window 1, shift 1, day offset 0, triad offset 0, lag 3 of x0
COMBOS = [{'1': [0, 1]}, {'3': [-1, 0, 1]}, {'1': [0], '3': [0]}]
CASES = [
    {'name': 'two_sources', 'kind': 'avg', 'x': ['x0', 'x1'], 'e': ['e0', 'e1'], 'diagoffsets': None, 'keep': ['x'], 'keep_sampling': ['resampled']},
    {'name': 'combos', 'kind': 'avg', 'x': ['x0'], 'e': ['e0'], 'diagoffsets': COMBOS, 'keep': ['x', 'e']},
    {'name': 'axis2', 'kind': 'avg', 'x': ['x0'], 'e': ['e0'], 'diagoffsets': [{'2': [-1, 0, 1], '3': [0]}, {'2': [0], '1': [0, 1]}], 'keep': ['x', 'e']},
    {'name': 'full_axis', 'kind': 'avg', 'x': ['f0', 'f1'], 'e': ['e0', 'e1'], 'diagoffsets': [{'1': [0, 2]}, {'2': [0], '1': [1]}], 'keep': ['x']},
    {'name': 'nan', 'kind': 'avg', 'x': ['x0', 'x1'], 'e': ['e0', 'e1'], 'diagoffsets': [{'3': [0, 1]}], 'keep': ['x'],
     'nan': [0, 'oversampled', 'whole', 'mean', NAN_AT]},
    {'name': 'ndarray_weights', 'kind': 'avg', 'from': 'two_sources', 'x': [], 'e': ['e0'], 'diagoffsets': [{'1': [0, 1]}], 'keep': ['x']},
    {'name': 'k_linear', 'kind': 'kbin', 'from': 'combos', 'kbintype': 'linear', 'num_kbins': None, 'kbins': False},
    {'name': 'k_log4', 'kind': 'kbin', 'from': 'combos', 'kbintype': 'log', 'num_kbins': 4, 'kbins': False},
    {'name': 'k_edges', 'kind': 'kbin', 'from': 'combos', 'kbintype': 'log', 'num_kbins': None, 'kbins': True},
]


class Q(NP.ndarray):
    """what the reference's statements ask of a Quantity, with every unit 1"""
    si = property(lambda self: self)
    value = property(lambda self: NP.asarray(self))
    unit = property(lambda self: NP.asarray(1.0).view(Q))


def _lines(path, a, b):
    with open(path) as fh:
        return ''.join(fh.readlines()[a - 1:b])


def _functions(ref_root):
    src = os.path.join(ref_root, 'prisim', 'bispectrum_phase.py')
    np_ns = types.SimpleNamespace(**{k: getattr(NP, k) for k in dir(NP) if not k.startswith('__')})
    np_ns.int, np_ns.float, np_ns.complex, np_ns.bool = int, float, complex, bool
    np_ns.linspace = lambda a, b, num=50, **kw: NP.linspace(a, b, num=int(num), **kw)

    class Bar(object):
        def __init__(self, *a, **kw):
            pass

        def start(self):
            return self

        def update(self, n):
            pass

        def finish(self):
            pass

    nothing = lambda *a, **kw: None  # noqa: E731
    ns = {'NP': np_ns, 'MA': MA, 'copy': copy, 'U': types.SimpleNamespace(Unit=lambda s: 1, Mpc=1),
          'OPS': types.SimpleNamespace(binned_statistic=lambda x, statistic=None, bins=None: BSP.binned_statistic_count(x, bins)),
          'PGB': types.SimpleNamespace(ProgressBar=Bar, Percentage=nothing, Bar=nothing, Counter=nothing, ETA=nothing), 'print': nothing}
    exec('def average(xcpdps, excpdps=None, diagoffsets=None):\n' + textwrap.indent(textwrap.dedent(_lines(src, 1068, 1231)), '    '), ns)
    exec('def kbinned(xcpdps, kbins=None, num_kbins=None, kbintype="log"):\n' + textwrap.indent(textwrap.dedent(_lines(src, 1411, 1493)), '    '), ns)
    return ns['average'], ns['kbinned']


def inputs(rng):
    """the arrays that cpavg_checker.data_set builds the data sets from"""
    g = {}
    g['in__top__triads'] = NP.asarray([[0, 1, 2], [0, 2, 3], [1, 2, 4]])
    g['in__top__triads_ind'], g['in__top__lst_ind'], g['in__top__day_ind'] = NP.arange(3), NP.arange(4), NP.arange(3)
    g['in__top__lst'], g['in__top__dlst'] = 1.0 + 0.07 * NP.arange(4), NP.full(4, 0.07)
    g['in__top__days'], g['in__top__dday'] = 2458000.0 + 2.0 * NP.arange(3), NP.full(3, 2.0)
    g['in__top__lstXoffsets'] = 0.07 * NP.arange(3)
    fw = rng.uniform(0.1, 1.0, (AK.NSPW, 6))
    for smp, nlags in AK.NLAGS.items():
        pre = 'in__%s__' % smp
        lags = DSP.spectral_axis(nlags, delx=1e5 * 12 / nlags, shift=True)
        g[pre + 'lags'] = lags
        g[pre + 'z'] = NP.asarray([8.46, 8.45])
        g[pre + 'kprll'] = NP.asarray([5.0e5, 5.2e5]).reshape(-1, 1) * lags.reshape(1, -1)
        g[pre + 'freq_center'], g[pre + 'bw_eff'] = NP.asarray([150.15e6, 150.35e6]), NP.asarray([2.0e5, 3.0e5])
        g[pre + 'shape'] = NP.array('bhw')
        g[pre + 'freq_wts'], g[pre + 'lag_corr_length'] = fw, 6 / NP.sum(fw, axis=-1)
    for name, (pool, stats, shape, _, _, _) in AK.SETS.items():
        for smp in stats:
            for stat in stats[smp]:
                shp = shape + (AK.NLAGS[smp],)
                g['set__%s__%s__%s' % (name, smp, stat)] = rng.standard_normal(shp) + 1j * rng.standard_normal(shp)
    return g


def quantities(d):
    """a data set with its spectra as stand-in quantities (lists of them behind a stage 2)"""
    d = copy.deepcopy(d)
    for smp in AK.SAMPLINGS:
        for pool in ('whole', 'submodel', 'residual', 'errinfo'):
            for stat in ('mean', 'median'):
                if smp in d and pool in d[smp] and stat in d[smp][pool]:
                    x = d[smp][pool][stat]
                    d[smp][pool][stat] = [NP.array(MA.getdata(a)).view(Q) for a in x] if isinstance(x, list) else NP.array(MA.getdata(x)).view(Q)
    return d


def plain(x):
    assert not NP.any(MA.getmaskarray(x)), 'a masked element in an averaged output'
    x = NP.array(MA.getdata(x))
    assert not NP.any(NP.isnan(x)), 'NaN in an averaged output'
    return x


def main(ref_root):
    rng = NP.random.default_rng(20261118)
    average, kbinned = _functions(ref_root)
    g = inputs(rng)
    kmax = NP.abs(g['in__oversampled__kprll']).max()
    g['in__kbins'] = NP.asarray([0.0, 0.3 * kmax, 0.55 * kmax, 0.8 * kmax])       # the lags beyond 0.8 kmax are left out
    g['cases'] = NP.array(json.dumps(CASES))
    for spec in CASES:
        name = spec['name']
        with warnings.catch_warnings(), NP.errstate(all='ignore'):
            warnings.simplefilter('ignore')
            if spec['kind'] == 'avg':
                xs, es = AK.case_inputs(spec, g)
                res = average([quantities(d) for d in xs], [quantities(d) for d in es], copy.deepcopy(AK.diagoffsets_of(spec)))
            else:
                res = kbinned(quantities(AK.gold_average(spec['from'], 'x', g)), **AK.kbin_arguments(spec, g))
        if spec['kind'] == 'avg':
            for which, r in zip('xe', res):
                if which not in spec['keep']:
                    continue
                for smp in spec.get('keep_sampling', AK.SAMPLINGS):
                    for pool in ('whole', 'errinfo'):
                        if smp not in r or pool not in r[smp]:
                            continue
                        stem = '%s__%s__%s__%s__' % (name, which, smp, pool)
                        for key in ('mean', 'median', 'diagweights'):
                            if key not in r[smp][pool]:
                                continue
                            v = r[smp][pool][key]
                            if spec['diagoffsets'] is None:
                                g[stem + key] = plain(v)
                            else:
                                assert len(v) == len(spec['diagoffsets'])
                                for c, a in enumerate(v):
                                    g['%s%s__%d' % (stem, key, c)] = plain(a)
                                r[smp][pool][key] = [plain(a) for a in v]
            continue
        nbad = ntot = 0
        for smp in AK.SAMPLINGS:
            info = res[smp]['kbininfo']
            stem = '%s__%s__' % (name, smp)
            counts = NP.asarray(info['counts'])
            g[stem + 'kbininfo__counts'], g[stem + 'kbininfo__kbin_edges'] = counts, NP.asarray(info['kbin_edges'])
            g[stem + 'kbininfo__kbinnum'] = NP.asarray(info['kbinnum'])
            for spw, ri in enumerate(info['ri']):
                g['%skbininfo__ri__%d' % (stem, spw)] = NP.asarray(ri)
            for stat in AK.XSTATS[smp]:
                for c in range(len(COMBOS)):
                    for key, x in (('PS', res[smp]['whole'][stat]['PS'][c]), ('Del2', res[smp]['whole'][stat]['Del2'][c]),
                                   ('kc', info['whole'][stat][c])):
                        x = NP.array(x)
                        empty = NP.broadcast_to((counts == 0).reshape((AK.NSPW,) + (1,) * (x.ndim - 2) + (-1,)), x.shape)
                        assert NP.array_equal(AK.cnan(x), empty), (name, smp, stat, c, key, 'NaN elsewhere than in the empty bins')
                        nbad += int(empty.sum())
                        ntot += x.size
                        g['%swhole__%s__%s__%d' % (stem, stat, key, c)] = x
        print('%s: %d of %d output values are NaN, all in empty bins' % (name, nbad, ntot))
    buf = io.BytesIO()
    NP.savez_compressed(buf, **g)
    size = buf.getbuffer().nbytes
    print('golden_cpavg.npz: %d bytes, %d arrays' % (size, len(g)))
    assert size < 400000, 'the fixture is too large'
    with open(os.path.join(HERE, 'golden_cpavg.npz'), 'wb') as fh:
        fh.write(buf.getvalue())


if __name__ == '__main__':
    main(sys.argv[1])
