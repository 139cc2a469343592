"""numpy statement of include/prisim_cpavg.h: the weighted average of several arrays and of selected positions of their axes
(prisim_cphase_xavg) and the averages of a power spectrum in bins of |k_parallel| (prisim_cphase_kbin) -- the sums of
prisim/bispectrum_phase.py:incoherent_cross_power_spectrum_average (:1116-1119, :1169-1195) and incoherent_kbin_averaging
(:1479-1486).  The checker of the two entries and of prisim_amd.bispectrum_phase's two functions; tests/test_cpavg.py pins it to
tests/golden/golden_cpavg.npz, the reference's own statements executed (tests/golden/make_golden_cpavg.py).

Bounds, with u = 2^-52.  A sequential or pairwise sum of L products is within (L + 2) u S of exact, S the sum of the terms' magnitudes;
a quotient of two such sums doubles that.  The slack of 8 is the project's (cpxps_checker.bound) and covers numpy's complex division
by a real, which multiplies by a rounded reciprocal; so no quotient has to match bit for bit.
  stage 1   (2 L + 8) u S / D per element: L the sets, S = sum |a_i| |w_i| over the products that are not NaN, D = |sum w_i|.
  stage 2   the stage-1 bounds propagated, sum(b1 |W|) / |sum W|, plus (2 L' + 8) u sum(|avg| |W|) / |sum W|, L' the selected positions.
  ps        (L + 8) u S / n: L the members of the bin, S = sum |p_j| and n the number of the members that are not NaN.
  del2      (L + 12) u S3 / n3 / (2 pi^2), S3 = sum k_j^3 |p_j|: its terms include the cube and the division by the constant.
  kc        (2 L + 8) u kc.
NaN positions must match exactly everywhere.
"""
import json
import os
import warnings

import numpy as NP

EPS = 2.0 ** -52


def _complex(re, im):
    out = NP.empty(NP.broadcast(re, im).shape, dtype=NP.complex128)
    out.real, out.imag = re, im
    return out


def cnan(x):
    x = NP.asarray(x)
    return NP.isnan(x.real) | NP.isnan(x.imag)


def _quiet(fn):
    def call(*args, **kw):
        with warnings.catch_warnings(), NP.errstate(all='ignore'):
            warnings.simplefilter('ignore')
            return fn(*args, **kw)
    return call


# ---- prisim_cphase_xavg ---------------------------------------------------------------------------------------------------------------

def _union(shape, weights):
    return tuple(max(w.shape[x] for w in weights) for x in range(len(shape)))


def _select(x, masks, shape):
    """x, which broadcasts against `shape`, at the selected positions of the reduced axes"""
    full = tuple(shape[ax] if ax in masks else n for ax, n in enumerate(x.shape))
    x = NP.broadcast_to(x, full)
    for ax, sel in masks.items():
        x = NP.take(x, NP.nonzero(NP.asarray(sel).astype(bool))[0], axis=ax)
    return x


@_quiet
def xavg(arrays, weights, combos=(), bounds=False):
    """{'avg', 'wsum', 'out': [...], 'wout': [...]} of the header; with bounds also 'avg_bound' and 'out_bound': [...]"""
    arrays = [NP.asarray(a, dtype=NP.complex128) for a in arrays]
    weights = [NP.asarray(w, dtype=NP.float64) for w in weights]
    shape = arrays[0].shape
    u = _union(shape, weights)
    num, den, S = NP.zeros(shape, dtype=NP.complex128), NP.zeros(u), NP.zeros(shape)
    for a, w in zip(arrays, weights):
        pr = _complex(a.real * w, a.imag * w)
        bad = cnan(pr)
        num = num + NP.where(bad, 0.0, pr)
        S = S + NP.where(bad, 0.0, NP.abs(a) * NP.abs(w))
        den = den + NP.where(NP.isnan(w), 0.0, NP.broadcast_to(w, NP.broadcast_shapes(w.shape, u)))
    avg = _complex(num.real / den, num.imag / den)
    res = {'avg': avg, 'wsum': den, 'out': [], 'wout': []}
    b1 = (2 * len(arrays) + 8) * EPS * S / NP.abs(den)
    if bounds:
        res['avg_bound'], res['out_bound'] = b1, []
    for combo in combos:
        axes = tuple(sorted(int(ax) for ax in combo))
        masks = {int(ax): combo[ax] for ax in combo}
        sa, sw = _select(avg, masks, shape), _select(den, masks, shape)
        wout = NP.sum(sw, axis=axes, keepdims=True)
        tot = NP.sum(_complex(sa.real * sw, sa.imag * sw), axis=axes, keepdims=True)
        res['out'].append(_complex(tot.real / wout, tot.imag / wout))
        res['wout'].append(wout)
        if bounds:
            nsel = int(NP.prod([sa.shape[ax] for ax in axes]))
            sb = _select(b1, masks, shape)
            res['out_bound'].append((NP.sum(sb * NP.abs(sw), axis=axes, keepdims=True)
                                     + (2 * nsel + 8) * EPS * NP.sum(NP.abs(sa) * NP.abs(sw), axis=axes, keepdims=True)) / NP.abs(wout))
    return res


# ---- prisim_cphase_kbin ---------------------------------------------------------------------------------------------------------------

@_quiet
def kbin(p, kprll, offsets, members, bounds=False):
    """{'ps', 'del2', 'kc'} of the header, each (nspw, ..., nk); with bounds also 'ps_bound', 'del2_bound' and 'kc_bound'"""
    p = NP.asarray(p, dtype=NP.complex128)
    k = NP.abs(NP.asarray(kprll, dtype=NP.float64))
    off = NP.asarray(offsets, dtype=NP.int64)
    nk = off.shape[1] - 1
    shape = p.shape[:-1] + (nk,)
    res = {'ps': NP.full(shape, complex(NP.nan, NP.nan)), 'del2': NP.full(shape, complex(NP.nan, NP.nan)), 'kc': NP.full(shape, NP.nan)}
    bnd = {key + '_bound': NP.full(shape, NP.nan) for key in res}
    c = 2.0 * NP.pi * NP.pi
    for w in range(p.shape[0]):
        mem = NP.asarray(members[w]).reshape(-1)
        for b in range(nk):
            ind = mem[off[w, b]:off[w, b + 1]]
            if ind.size == 0:
                continue
            v, kj = p[w][..., ind], k[w, ind]
            ok = ~cnan(v)
            n = NP.sum(ok, axis=-1)
            s = NP.sum(NP.where(ok, v, 0.0), axis=-1)
            res['ps'][w][..., b] = _complex(s.real / n, s.imag / n)
            k3 = (kj * kj) * kj
            t = _complex(k3 * v.real, k3 * v.imag)
            ok3 = ~cnan(t)
            n3 = NP.sum(ok3, axis=-1)
            s3 = NP.sum(NP.where(ok3, t, 0.0), axis=-1)
            res['del2'][w][..., b] = _complex((s3.real / n3) / c, (s3.imag / n3) / c)
            a = NP.hypot(v.real, v.imag)
            ka = kj * a
            kc = NP.sum(NP.where(NP.isnan(ka), 0.0, ka), axis=-1) / NP.sum(NP.where(NP.isnan(a), 0.0, a), axis=-1)
            res['kc'][w][..., b] = kc
            L = ind.size
            bnd['ps_bound'][w][..., b] = (L + 8) * EPS * NP.sum(NP.where(ok, a, 0.0), axis=-1) / n
            bnd['del2_bound'][w][..., b] = (L + 12) * EPS * NP.sum(NP.where(ok3, k3 * a, 0.0), axis=-1) / n3 / c
            bnd['kc_bound'][w][..., b] = (2 * L + 8) * EPS * NP.abs(kc)
    if bounds:
        res.update(bnd)
    return res


def compare(got, want, bound, label=''):
    """got against want: the same shape, dtype and NaN positions, |got - want| <= bound elsewhere.  Prints and returns the worst share
    of the bound."""
    got, want = NP.asarray(got), NP.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (label, got.shape, want.shape, got.dtype, want.dtype)
    gn, wn = cnan(got), cnan(want)
    assert NP.array_equal(gn, wn), (label, 'NaN positions differ', int(gn.sum()), int(wn.sum()))
    err = NP.abs(NP.where(gn, 0.0, got) - NP.where(wn, 0.0, want))[~gn]
    lim = NP.broadcast_to(bound, got.shape)[~gn]
    assert NP.all(NP.isfinite(lim)), (label, 'the bound is not finite')
    worst = float(NP.max(NP.where(lim > 0, err / NP.where(lim > 0, lim, 1.0), NP.where(err == 0, 0.0, NP.inf)))) if err.size else 0.0
    print('%s: worst error %.3f of the bound; NaN share %.4f' % (label, worst, gn.mean() if gn.size else 0.0))
    assert worst <= 1.0, (label, worst)
    return worst


def compare_xavg(res, arrays, weights, combos=(), label=''):
    """a result of cphase_xavg against the checker on the same arguments; the worst share of the bounds"""
    want = xavg(arrays, weights, combos, bounds=True)
    worst = 0.0
    if res['avg'] is not None:
        worst = compare(res['avg'], want['avg'], want['avg_bound'], label + ' avg')
    worst = max(worst, compare(res['wsum'], want['wsum'], (len(arrays) + 2) * EPS * NP.abs(want['wsum']), label + ' wsum'))
    assert len(res['out']) == len(res['wout']) == len(combos)
    for c in range(len(combos)):
        worst = max(worst, compare(res['out'][c], want['out'][c], want['out_bound'][c], '%s out[%d]' % (label, c)))
        nsel = res['avg'].size // res['out'][c].size if res['avg'] is not None else want['avg'].size // want['out'][c].size
        worst = max(worst, compare(res['wout'][c], want['wout'][c], (nsel + len(arrays) + 4) * EPS * NP.abs(want['wout'][c]), '%s wout[%d]' % (label, c)))
    return worst


def compare_kbin(res, p, kprll, offsets, members, label=''):
    want = kbin(p, kprll, offsets, members, bounds=True)
    return max(compare(res[key], want[key], want[key + '_bound'], label + ' ' + key) for key in ('ps', 'del2', 'kc'))


class CheckerContext(object):
    """cphase_xavg and cphase_kbin of prisim_amd._abi.Context computed by this module behind the Context's own argument checks: the
    stand-in context of the CPU tests"""

    def __init__(self):
        self.xavg_calls, self.kbin_calls = [], []

    def cphase_xavg(self, arrays, weights, combos=(), want_avg=True, budget_bytes=0):
        from prisim_amd import _abi
        arrays, weights, masks = _abi.Context.cphase_xavg_arguments(arrays, weights, combos)
        self.xavg_calls.append({'nsets': len(arrays), 'shape': arrays[0].shape, 'combos': [sorted(m) for m in masks], 'want_avg': want_avg})
        res = xavg(arrays, weights, masks)
        if not want_avg:
            res['avg'] = None
        res['stats'] = {}
        return res

    def cphase_kbin(self, p, kprll, offsets, members, route='auto', budget_bytes=0):
        from prisim_amd import _abi
        _abi._route_code(route, _abi.CPAVG_ROUTES)
        p3, k, off, mem, lead = _abi.Context.cphase_kbin_arguments(p, kprll, offsets, members)
        self.kbin_calls.append({'shape': NP.shape(p), 'nk': off.shape[1] - 1})
        res = kbin(NP.asarray(p, dtype=NP.complex128), k, off, members)
        res['stats'] = {}
        return res


# ---- the fixture ------------------------------------------------------------------------------------------------------------------

SAMPLINGS = ('oversampled', 'resampled')
NLAGS = {'oversampled': 8, 'resampled': 4}
NSPW = 2
SHIFTS, DAYOFF, TRIOFF = [0, 1, 2], [-2, -1, 0, 1, 2], [-2, -1, 0, 1, 2]
TOP_KEYS = ('triads', 'triads_ind', 'lst', 'lst_ind', 'dlst', 'days', 'day_ind', 'dday', 'lstXoffsets')
SAMPLING_KEYS = ('z', 'kprll', 'lags', 'freq_center', 'bw_eff', 'shape', 'freq_wts', 'lag_corr_length')
TRACE = [1, 2, 3, 2, 1]
# the data sets: pool, statistics by sampling, shape without the lags, and what goes with the spectra.  x: two sources with 4 and 5
# LST bins behind the three shifts; e: their sub-sample differences (3 pairs of day-bin pairs, not crossed); f: the triads crossed and
# not collapsed, carried along as a full axis
XSTATS = {'oversampled': ('mean',), 'resampled': ('mean', 'median')}
ESTATS = {'oversampled': ('mean',), 'resampled': ('mean',)}
FSTATS = {'resampled': ('mean',)}
SETS = {
    'x0': ('whole', XSTATS, (NSPW, 3, 5, 5), {1: SHIFTS, 2: DAYOFF, 3: TRIOFF}, {1: [4, 3, 2], 2: TRACE, 3: TRACE},
           {1: [1], 2: [2], 3: [3]}),
    'x1': ('whole', XSTATS, (NSPW, 3, 5, 5), {1: SHIFTS, 2: DAYOFF, 3: TRIOFF}, {1: [5, 4, 3], 2: TRACE, 3: TRACE},
           {1: [1], 2: [2], 3: [3]}),
    'e0': ('errinfo', ESTATS, (NSPW, 3, 3, 5), {1: SHIFTS, 3: TRIOFF}, {1: [4, 3, 2], 3: TRACE}, {1: [1], 3: [3]}),
    'e1': ('errinfo', ESTATS, (NSPW, 3, 3, 5), {1: SHIFTS, 3: TRIOFF}, {1: [5, 4, 3], 3: TRACE}, {1: [1], 3: [3]}),
    'f0': ('whole', FSTATS, (NSPW, 3, 5, 3, 3), {1: SHIFTS, 2: DAYOFF}, {1: [4, 3, 2], 2: TRACE}, {1: [1], 2: [2], 3: [3, 4]}),
    'f1': ('whole', FSTATS, (NSPW, 3, 5, 3, 3), {1: SHIFTS, 2: DAYOFF}, {1: [5, 4, 3], 2: TRACE}, {1: [1], 2: [2], 3: [3, 4]}),
}

_GOLD = {}


def gold():
    if not _GOLD:
        _GOLD['npz'] = NP.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'golden_cpavg.npz'))
    return _GOLD['npz']


def _files(g):
    return g.files if hasattr(g, 'files') else list(g)


def cases(g=None):
    return json.loads(str((g or gold())['cases']))


def case(name, g=None):
    return [c for c in cases(g) if c['name'] == name][0]


def data_set(name, g=None):
    """the data set `name` as compute_power_spectrum (or its uncertainty) returns it, from the arrays of the fixture (or of g)"""
    g = g or gold()
    pool, stats, shape, doff, dwts, amap = SETS[name]
    d = {key: NP.copy(g['in__top__' + key]) for key in TOP_KEYS}
    for smp in stats:
        d[smp] = {key: (str(g['in__%s__shape' % smp]) if key == 'shape' else NP.copy(g['in__%s__%s' % (smp, key)])) for key in SAMPLING_KEYS}
        d[smp][pool] = {'diagoffsets': {ax: NP.asarray(v) for ax, v in doff.items()}, 'diagweights': {ax: NP.asarray(v) for ax, v in dwts.items()},
                        'axesmap': {ax: NP.asarray(v) for ax, v in amap.items()}, 'nsamples_incoh': 12, 'nsamples_coh': 1}
        for stat in stats[smp]:
            d[smp][pool][stat] = NP.copy(g['set__%s__%s__%s' % (name, smp, stat)])
    return d


def diagoffsets_of(spec):
    """the diagoffsets argument of a case: None, or a list of {axis: list of offsets}"""
    if spec['diagoffsets'] is None:
        return None
    return [{int(ax): list(v) for ax, v in combo.items()} for combo in spec['diagoffsets']]


def case_inputs(spec, g=None):
    """(xcpdps, excpdps) of an averaging case, each a list of data sets; a case with 'nan' has one element of one set at NaN; a case
    with 'from' takes the reference's result of that case as its only set"""
    g = g or gold()
    xs, es = [data_set(n, g) for n in spec['x']], [data_set(n, g) for n in spec['e']]
    if spec.get('from'):
        xs = [gold_average(spec['from'], 'x', g)]
    if spec.get('nan'):
        i, smp, pool, stat, flat = spec['nan']
        xs[i][smp][pool][stat].reshape(-1)[flat] = complex(NP.nan, NP.nan)
    return xs, es


def gold_average(name, which, g=None):
    """the reference's result of the averaging case `name` for xcpdps ('x') or excpdps ('e'), as far as the fixture keeps it: the
    dictionary of incoherent_cross_power_spectrum_average, or None"""
    g = g or gold()
    spec = case(name, g)
    pre = '%s__%s__' % (name, which)
    if not any(key.startswith(pre) for key in _files(g)):
        return None
    xs, es = case_inputs(spec, g)
    first = (xs if which == 'x' else es)[0]
    out = {key: first[key] for key in TOP_KEYS}
    ncombo = None if spec['diagoffsets'] is None else len(spec['diagoffsets'])
    for smp in SAMPLINGS:
        if smp not in first:
            continue
        out[smp] = {key: first[smp][key] for key in SAMPLING_KEYS}
        for pool in ('whole', 'submodel', 'residual', 'errinfo'):
            if pool not in first[smp] or (pre + smp + '__' + pool + '__diagweights' + ('' if ncombo is None else '__0')) not in _files(g):
                continue
            stem = pre + smp + '__' + pool + '__'
            r = {'diagoffsets': first[smp][pool]['diagoffsets'], 'axesmap': first[smp][pool]['axesmap']}
            for stat in ('mean', 'median'):
                if stat in first[smp][pool]:
                    r[stat] = g[stem + stat] if ncombo is None else [g['%s%s__%d' % (stem, stat, c)] for c in range(ncombo)]
            r['diagweights'] = g[stem + 'diagweights'] if ncombo is None else [g['%sdiagweights__%d' % (stem, c)] for c in range(ncombo)]
            out[smp][pool] = r
    return out


def gold_kbin(name, g=None):
    """the reference's result of the k-binning case `name`: per sampling 'kbininfo' ('counts', 'kbin_edges', 'kbinnum', 'ri' and the
    centres of 'whole') and 'whole' -> statistic -> 'PS' / 'Del2', lists with one array per combination"""
    g = g or gold()
    out = {}
    for smp in SAMPLINGS:
        stem = '%s__%s__' % (name, smp)
        info = {key: list(g[stem + 'kbininfo__' + key]) for key in ('counts', 'kbin_edges', 'kbinnum')}
        info['ri'] = [g['%skbininfo__ri__%d' % (stem, spw)] for spw in range(NSPW)]
        info['whole'] = {}
        out[smp] = {'kbininfo': info, 'whole': {}}
        for stat in ('mean', 'median'):
            n = len([key for key in _files(g) if key.startswith('%swhole__%s__PS__' % (stem, stat))])
            if n == 0:
                continue
            out[smp]['whole'][stat] = {key: [g['%swhole__%s__%s__%d' % (stem, stat, key, c)] for c in range(n)] for key in ('PS', 'Del2')}
            info['whole'][stat] = [g['%swhole__%s__kc__%d' % (stem, stat, c)] for c in range(n)]
    return out


def kbin_arguments(spec, g=None):
    g = g or gold()
    kw = {'kbintype': spec['kbintype']}
    if spec.get('num_kbins') is not None:
        kw['num_kbins'] = spec['num_kbins']
    if spec.get('kbins'):
        kw['kbins'] = NP.asarray(g['in__kbins'])
    return kw
