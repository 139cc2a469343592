"""numpy statement of include/prisim_cpxps.h: the cross power P = (factor (a wa)) conj(b wb) of two stacks of delay spectra
(nspw, n1, n2, n3, nlags) over pairs of LST bins, day bins and triads, and its collapses -- the cross products of
prisim/bispectrum_phase.py:ClosurePhaseDelaySpectrum.compute_power_spectrum (:3468-3551).  The checker of prisim_cphase_xpower and of
the power spectra of prisim_amd.bispectrum_phase.ClosurePhaseDelaySpectrum; tests/test_cpxps.py pins it to
tests/golden/golden_cpxps.npz, the reference's own statements executed (tests/golden/make_golden_cpxps.py).

Every complex product is written out on the real and imaginary parts, (ar br - ai bi, ar bi + ai br), each product and sum rounded
once: that is the entry's arithmetic whatever numpy's own complex loops fuse (prisim_amd/_abi.py:numpy_fuses_complex_product), so the
uncollapsed product can be compared bit for bit.

Bound of a collapsed element: |got - want| <= (L + 8) 2^-52 S, with L the number of terms of the longest reduction behind the element
and S = factor sum |a wa| |b wb| over those terms (the largest term where a median selects).  Three complex products and one real one
per term (each within 2^-52 of the product of the moduli, relatively), a sequential sum of L terms and one division, on both sides.
"""
import warnings

import numpy as NP

from prisim_amd import dsp_readings as DSP

EPS = 2.0 ** -52


def _complex(re, im):
    out = NP.empty(NP.broadcast(re, im).shape, dtype=NP.complex128)
    out.real, out.imag = re, im
    return out


def cmul(a, b):
    a, b = NP.asarray(a, dtype=NP.complex128), NP.asarray(b, dtype=NP.complex128)
    return _complex(a.real * b.real - a.imag * b.imag, a.real * b.imag + a.imag * b.real)


def cmulc(a, b):
    """a conj(b)"""
    a, b = NP.asarray(a, dtype=NP.complex128), NP.asarray(b, dtype=NP.complex128)
    return _complex(a.real * b.real + a.imag * b.imag, a.imag * b.real - a.real * b.imag)


def cnan(x):
    return NP.isnan(x.real) | NP.isnan(x.imag)


def _weights(shape, weights):
    """W (n1, n2, n3) = (w1[i1] w2[i2]) w3[i3]"""
    ws = [NP.ones(n, dtype=NP.complex128) if (weights is None or weights[ax] is None) else NP.asarray(weights[ax], dtype=NP.complex128).reshape(-1)
          for ax, n in enumerate(shape[1:4])]
    return cmul(cmul(ws[0][:, None, None], ws[1][None, :, None]), ws[2][None, None, :])


def cross(a, b=None, factor=None, weights=None, modes=('none', 'none', 'none'), shifts=None, magnitude=False):
    """The uncollapsed product: (nspw,) + per axis (n,) or (nshift, n1) / (n, n) + (nlags,).  magnitude: |factor| |a wa| |b wb| in its
    place, NaN where the product is structurally NaN."""
    a = NP.asarray(a, dtype=NP.complex128)
    b = a if b is None else NP.asarray(b, dtype=NP.complex128)
    f = NP.ones(a.shape[0]) if factor is None else NP.asarray(factor, dtype=NP.float64).reshape(-1)
    W = _weights(a.shape, weights)[None, ..., None]
    xa, xb = cmul(a, W), cmul(b, W)
    if magnitude:
        ya, xb = NP.abs(f)[:, None, None, None, None] * NP.abs(xa), NP.abs(xb)
    else:
        ya = cmul(_complex(f, 0.0 * f)[:, None, None, None, None], xa)
    for ax in (3, 2):
        if modes[ax - 1] != 'none':
            ya, xb = NP.expand_dims(ya, ax + 1), NP.expand_dims(xb, ax)
    if modes[0] != 'none':
        sh = NP.asarray(shifts, dtype=NP.int64).reshape(-1)
        rolled = NP.full((xb.shape[0], sh.size) + xb.shape[1:], NP.nan if magnitude else complex(NP.nan, NP.nan), dtype=xb.dtype)
        for k, s in enumerate(sh):
            rolled[:, k, s:] = xb[:, :xb.shape[1] - s]
        ya, xb = NP.expand_dims(ya, 1), rolled
    return ya * xb if magnitude else cmulc(ya, xb)


def _position(modes, done, ax):
    """where the (first) output axis of input axis `ax` lies now"""
    return 1 + sum(2 if (modes[y - 1] != 'none' and y not in done) else 1 for y in range(1, ax))


def select_median(p, axis):
    """numpy's nanmedian of complex numbers along `axis`: order by the real part, then the imaginary part, the middle value or half
    the sum of the two middle ones of the elements that are not NaN; NaN where none is left"""
    p = NP.where(cnan(p), complex(NP.nan, NP.nan), p)
    srt = NP.moveaxis(NP.sort(p, axis=axis), axis, -1)                          # NaN + NaN i sorts last
    m = NP.sum(~cnan(srt), axis=-1, keepdims=True)
    lo = NP.take_along_axis(srt, NP.maximum((m - 1) // 2, 0), axis=-1)[..., 0]
    hi = NP.take_along_axis(srt, m // 2, axis=-1)[..., 0]
    m = m[..., 0]
    out = NP.where(m % 2 == 1, lo, _complex(0.5 * (lo.real + hi.real), 0.5 * (lo.imag + hi.imag)))
    return NP.where(m == 0, complex(NP.nan, NP.nan), out)


def collapse(p, modes, order, stat='mean', magnitude=False):
    """The collapses of `order` (axes 1, 2, 3) applied to the product p in turn.  magnitude: the bound's S from cross(magnitude=True):
    sums without the division, the largest candidate of a median."""
    done = []
    with warnings.catch_warnings(), NP.errstate(all='ignore'):
        warnings.simplefilter('ignore')
        for ax in order:
            pos = _position(modes, done, ax)
            if ax == 1:
                if magnitude:
                    p = NP.nansum(p, axis=pos + 1) if stat == 'mean' else NP.nanmax(p, axis=pos + 1)
                elif stat == 'mean':
                    bad = cnan(p)
                    cnt = NP.sum(~bad, axis=pos + 1)
                    tot = NP.sum(NP.where(bad, 0.0, p), axis=pos + 1)
                    p = _complex(tot.real / cnt, tot.imag / cnt)
                else:
                    p = select_median(p, pos + 1)
            else:
                tr, _, cnt = DSP.array_trace(p, axis1=pos, axis2=pos + 1, outaxis='axis1')
                if not magnitude:
                    cnt = cnt.reshape((-1,) + (1,) * (tr.ndim - pos - 1)).astype(NP.float64)
                    tr = _complex(tr.real / cnt, tr.imag / cnt)
                p = tr
            done.append(ax)
    return p


def xpower(a, b=None, factor=None, weights=None, modes=('none', 'none', 'none'), shifts=None, collapse_order=(), stat='mean'):
    return collapse(cross(a, b, factor, weights, modes, shifts), modes, collapse_order, stat)


def as_reference(p, modes):
    """A result in the reference's layout: for days and triads the reference has a at the second and b at the first index of a pair
    (:3482, :3509), the entry a at the first: the two axes of a full pair are swapped and the offsets of a collapsed one reversed.
    `modes` are those of the call; the collapsed axes must all be collapsed already."""
    for ax in (2, 3):
        pos = 1 + sum(2 if modes[y - 1] == 'full' else 1 for y in range(1, ax))
        if modes[ax - 1] == 'full':
            p = NP.swapaxes(p, pos, pos + 1)
        elif modes[ax - 1] == 'collapse':
            p = NP.flip(p, axis=pos)
    return p


def bound(a, b=None, factor=None, weights=None, modes=('none', 'none', 'none'), shifts=None, collapse_order=(), stat='mean'):
    """(L + 8) 2^-52 S per element of the collapsed result (NaN where the result is structurally NaN)"""
    S = collapse(cross(a, b, factor, weights, modes, shifts, magnitude=True), modes, collapse_order, stat, magnitude=True)
    L = max([1] + [NP.shape(a)[ax] for ax in collapse_order])
    return (L + 8) * EPS * S


def nan_share(modes, shifts, n1):
    """the share of NaN in a result: sum s / (nshift n1) where LST is 'full', 0 otherwise"""
    if modes[0] != 'full':
        return 0.0
    sh = NP.asarray(shifts).reshape(-1)
    return float(NP.sum(sh)) / (sh.size * n1)


def compare(got, a, b=None, factor=None, weights=None, modes=('none', 'none', 'none'), shifts=None, collapse_order=(), stat='mean',
            label='', structural_only=True):
    """got against the checker: bit for bit (NaN positions included) where nothing is collapsed, within bound() otherwise; the share of
    NaN is exactly nan_share().  Returns the largest error relative to the bound (0 where nothing is collapsed)."""
    want = xpower(a, b, factor, weights, modes, shifts, collapse_order, stat)
    assert got.shape == want.shape and got.dtype == NP.complex128, (label, got.shape, want.shape, got.dtype)
    gn, wn = cnan(got), cnan(want)
    assert NP.array_equal(gn, wn), (label, 'NaN positions differ', int(gn.sum()), int(wn.sum()))
    if structural_only:
        assert gn.mean() == nan_share(modes, shifts, NP.shape(a)[1]), (label, gn.mean(), nan_share(modes, shifts, NP.shape(a)[1]))
    if len(collapse_order) == 0:
        assert NP.array_equal(got[~gn], want[~gn]), (label, 'the uncollapsed product differs', float(NP.max(NP.abs(got[~gn] - want[~gn]))))
        print('%s: uncollapsed, bit for bit; NaN share %.4f' % (label, gn.mean()))
        return 0.0
    bnd = bound(a, b, factor, weights, modes, shifts, collapse_order, stat)
    assert bnd.shape == want.shape
    err = NP.abs(got - want)[~gn]
    lim = bnd[~gn]
    assert NP.all(NP.isfinite(lim))
    worst = float(NP.max(NP.where(lim > 0, err / NP.where(lim > 0, lim, 1.0), NP.where(err == 0, 0.0, NP.inf)))) if err.size else 0.0
    print('%s: worst error %.3e of the bound (L + 8) 2^-52 S; NaN share %.4f' % (label, worst, gn.mean()))
    assert worst <= 1.0, (label, worst)
    return worst


class CheckerContext(object):
    """cphase_xpower of prisim_amd._abi.Context computed by this module (and cphase_ft by tests/cpft_checker.py): the stand-in context
    of the CPU tests"""

    def __init__(self):
        self.calls = 0
        self.xcalls = []

    def cphase_ft(self, *args, **kw):
        import cpft_checker as FK
        return FK.CheckerContext().cphase_ft(*args, **kw)

    @staticmethod
    def cphase_xpower_shape(shape, modes, nshift):
        from prisim_amd import _abi
        return _abi.Context.cphase_xpower_shape(shape, modes, nshift)

    def cphase_xpower(self, a, b=None, factor=None, weights=None, modes=('none', 'none', 'none'), shifts=None, collapse=(), stat='mean',
                      budget_bytes=0):
        self.calls += 1
        self.xcalls.append({'modes': tuple(modes), 'collapse': tuple(int(c) for c in collapse), 'stat': stat,
                            'shifts': None if shifts is None else NP.asarray(shifts).copy()})
        if stat == 'median' and 1 in collapse and NP.shape(a)[1] > 256:
            raise ValueError('the median takes 256 LST bins at most')
        return {'out': xpower(a, b, factor, weights, modes, shifts, collapse, stat), 'stats': {}}


# ---- the fixture ------------------------------------------------------------------------------------------------------------------

_GOLD = {}
SAMPLINGS = ('oversampled', 'resampled')


def gold():
    if not _GOLD:
        import os
        _GOLD['npz'] = NP.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'golden_cpxps.npz'))
    return _GOLD['npz']


def cases():
    import json
    return json.loads(str(gold()['cases']))


def case(name):
    return [c for c in cases() if c['name'] == name][0]


def gold_inputs():
    """(f, cpinfo, cpds): the frequencies, the cpinfo of the stand-in ClosurePhase and FT's result by sampling, as the reference got them"""
    import numpy.ma as MA
    g = gold()

    def masked(x):
        return MA.array(x.copy(), mask=NP.zeros(x.shape, dtype=bool))

    cpinfo = {'raw': {'triads': g['in__triads'].copy()}, 'processed': {'prelim': {'wts': masked(g['in__twts'])}},
              'errinfo': {'list_of_pair_of_pairs': g['in__pairs'].tolist()}}
    for grp, d in (('prelim', cpinfo['processed']['prelim']), ('errinfo', cpinfo['errinfo'])):
        for k in ('lstbins', 'dlstbins', 'daybins', 'diff_dbins'):
            d[k] = g['in__%s__%s' % (grp, k)].copy()
    cpds = {}
    for smp in SAMPLINGS:
        pre = 'in__%s__' % smp
        ds = {k: g[pre + k].copy() for k in ('freq_center', 'bw_eff', 'freq_wts', 'lag_corr_length', 'lags')}
        ds['shape'] = str(g[pre + 'shape'])
        tw = cpinfo['processed']['prelim']['wts']
        ds['whole'] = {'dspec': {'twts': tw, 'mean': g[pre + 'whole__mean'].copy(), 'median': g[pre + 'whole__median'].copy()}}
        ds['residual'] = {'dspec': {'twts': tw, 'mean': g[pre + 'residual__mean'].copy(), 'median': g[pre + 'residual__median'].copy()}}
        ds['submodel'] = {'dspec': g[pre + 'submodel'].copy()}
        ds['errinfo'] = {q: {'twts': masked(g[pre + q + '__twts']), 'mean': g[pre + q + '__mean'].copy(), 'median': g[pre + q + '__median'].copy()}
                         for q in ('dspec0', 'dspec1')}
        cpds[smp] = ds
    return g['in__f'].copy(), cpinfo, cpds


def gold_arguments(spec):
    """(selection, autoinfo, xinfo) of a case as the methods take them"""
    auto = dict(spec['autoinfo'])
    if 'wts' in auto:
        auto['wts'] = [NP.asarray(w, dtype=NP.float64) for w in auto['wts']]
    xinfo = dict(spec['xinfo'])
    if 'wts' in xinfo:
        xinfo['wts'] = {k: ([NP.asarray(w, dtype=NP.float64) for w in v] if isinstance(v, list) else v) for k, v in xinfo['wts'].items()}
    sel = None
    if 'selection' in spec:
        sel = {'lst': NP.asarray(spec['selection']['lst']), 'triads': [tuple(t) for t in spec['selection']['triads']], 'days': None}
    return sel, auto, xinfo


def gold_meta(name):
    import json
    return json.loads(str(gold()[name + '__meta']))


def gold_top(name, key):
    return gold()['%s__top__%s' % (name, key)]


def gold_outputs(name):
    """{(sampling, pool, statistic): the reference's power spectrum} of what the fixture keeps of a case"""
    pre = name + '__'
    out = {}
    for key in gold().files:
        parts = key.split('__')
        if key.startswith(pre) and len(parts) == 4 and parts[1] in SAMPLINGS and parts[3] in ('mean', 'median'):
            out[(parts[1], parts[2], parts[3])] = gold()[key]
    return out


def class_bound(spec, cpds, smp, pool, factor):
    """The bound of a result of the class against the reference's, per window (nspw,): (N + 16) 2^-52 M G.  Every output value is a
    combination of at most N = n1 n2 n3 nshift ... products (the elements of the uncollapsed product per window and lag) with weights
    that sum to G at most -- the averages of the collapses and of avgcov are convex, the postX weights of the fixture are positive:
    G = max postX, or max postX / sum postX per axis with postXnorm -- each rounded within 2^-52 of M, the largest modulus a product can
    take: |factor| (max |a| max |wa|) (max |b| max |wb|) with the maxima over the whole window, which the coherent averages (convex
    too) do not exceed; 16 more roundings for the products themselves and the divisions."""
    xi = spec['xinfo']
    ds = cpds[smp]
    if pool == 'errinfo':
        xa = NP.maximum(NP.abs(ds['errinfo']['dspec0']['mean']), NP.abs(ds['errinfo']['dspec0']['median']))
        xb = NP.maximum(NP.abs(ds['errinfo']['dspec1']['mean']), NP.abs(ds['errinfo']['dspec1']['median']))
    else:
        x = ds[pool]['dspec']
        xa = xb = NP.abs(x) if pool == 'submodel' else NP.maximum(NP.abs(x['mean']), NP.abs(x['median']))
    wmax = 1.0
    gain = 1.0
    wts = xi.get('wts', {})
    for w in wts.get('preX', []):
        wmax *= NP.max(NP.abs(w))
    for w in wts.get('postX', [])[:len(xi['collapse_axes'])]:
        gain *= NP.max(NP.abs(w)) / (NP.abs(NP.sum(w)) if wts.get('postXnorm') else 1.0)
    n = 1
    for ax in xi['axes']:
        n *= xa.shape[ax] ** 2
    M = NP.abs(factor) * NP.max(xa, axis=(1, 2, 3, 4)) * NP.max(xb, axis=(1, 2, 3, 4)) * wmax ** 2
    return (n + 16) * EPS * M * gain
