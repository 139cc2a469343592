"""numpy.ma restatement of ClosurePhase.subsample_differencing and ClosurePhase.subtract (prisim/bispectrum_phase.py:2023-2249,
:1978-2019), the checker of prisim_cphase_diff and of prisim_amd.bispectrum_phase.  tests/test_cpdiff.py pins it to
tests/golden/golden_cpdiff.npz, the reference's own statements executed (tests/golden/make_golden_cpdiff.py).

The day and the LST pass are those of tests/cphase_bins_checker.py.  diff_step is the last step in the terms of
include/prisim_cpdiff.h.  Under its masks the reference leaves unspecified values (MA.empty); diff_step writes there what the device
documents: 0 for the differences, sqrt(w_j^2 + w_i^2) for the weights.  Several LSTs with lstbinsize=None, where the reference fails,
take the single-LST route, as the module documents."""
import warnings

import numpy as NP
import numpy.ma as MA

import cphase_bins_checker as CK

U, MOD_MIN, MAX_SHARE = CK.U, CK.MOD_MIN, CK.MAX_SHARE
OUTPUTS = ('diff0_mean', 'diff0_median', 'diff1_mean', 'diff1_median', 'wts0', 'wts1', 'mask0', 'mask1')
# |got - ref| of a difference whose members' phases are the same on both sides: each side takes one sincos per member (2 u per
# component and side, 4 u per member between the sides), halves the difference (exact) after one subtraction (1 u per side)
DIFF_CONST = (0.5 * (4.0 + 4.0) + 2.0) * U


def pairs_of_pairs(ndaybins):
    """Every unordered pair of disjoint pairs of day bins once, as [i, j, k, m] with i < j and k < m: sorted by (i, j), then (k, m),
    each kept under the lexicographically smaller of its two pairs first -- the order in which the reference meets them."""
    from itertools import combinations
    two = list(combinations(range(ndaybins), 2))
    return [[p[0], p[1], q[0], q[1]] for p in two for q in two if p < q and not set(p) & set(q)]


def diff_step(cp_mean, cp_median, wts, pairs):
    """the eight outputs of include/prisim_cpdiff.h from a binned stack (n0, n1, ntriads, nchan)"""
    cp_mean, cp_median, wts = (NP.asarray(a, dtype=NP.float64) for a in (cp_mean, cp_median, wts))
    pairs = NP.asarray(pairs).reshape(-1, 4)
    e = {'mean': NP.exp(1j * cp_mean), 'median': NP.exp(1j * cp_median)}
    masked = wts <= 0.0
    shape = (wts.shape[0], pairs.shape[0]) + wts.shape[2:]
    out = {k: NP.zeros(shape, dtype=NP.complex128 if k.startswith('diff') else (NP.float64 if k.startswith('wts') else bool)) for k in OUTPUTS}
    for q, row in enumerate(pairs.tolist()):
        for g, (a, b) in enumerate((row[:2], row[2:])):
            m = masked[:, b] | masked[:, a]
            out['mask%d' % g][:, q] = m
            out['wts%d' % g][:, q] = NP.sqrt(wts[:, b] ** 2 + wts[:, a] ** 2)
            for stat in ('mean', 'median'):
                out['diff%d_%s' % (g, stat)][:, q] = NP.where(m, 0.0, 0.5 * (e[stat][:, b] - e[stat][:, a]))
    return out


def errinfo_of(res):
    """the masked arrays of cpinfo['errinfo'] from the eight outputs"""
    return {'wts': {str(g): MA.array(res['wts%d' % g], mask=res['mask%d' % g]) for g in range(2)},
            'eicp_diff': {str(g): {s: MA.array(res['diff%d_%s' % (g, s)], mask=res['mask%d' % g]) for s in ('mean', 'median')} for g in range(2)}}


def subsample_differencing(cpinfo, daybinsize=None, ndaybins=4, lstbinsize=None, detail=None):
    """The method on cpinfo = {'raw': {'cphase', 'flags', 'lst', 'days'}}: returns what it puts into cpinfo['errinfo'].  detail: a dict
    that receives the bin_pass results under 'day' and 'lst', the LST bins under 'lst_bins' and the final stack under 'binned'."""
    raw = cpinfo['raw']
    if (ndaybins is not None) and (daybinsize is not None):
        raise ValueError('Only one of daybinsize or ndaybins should be set')
    days = NP.asarray(raw['days'])
    if daybinsize is not None:
        dres = NP.diff(days).min()
        dextent = days.max() - days.min() + dres
        assert daybinsize > dres
        daybinsize = NP.clip(daybinsize, dres, dextent)
        edges, centers, widths = CK._edges(days.min(), days.max(), dres, daybinsize)
        if edges.size - 1 < 4:
            raise ValueError('Could not find at least 4 bins along repeating days. Adjust binning interval.')
        counts, ri = CK.binned_count(days, edges)
        off, mem = CK.csr([ri[ri[k]:ri[k + 1]] for k in range(counts.size)])
        ndaybins = counts.size
    else:
        if ndaybins < 4:
            raise ValueError('Input ndaybins must be greater than or equal to 4')
        split = NP.array_split(days, ndaybins)
        centers = NP.asarray([NP.mean(d) for d in split])
        widths = NP.asarray([d.max() - d.min() for d in split])
        off, mem = CK.csr(NP.array_split(NP.arange(days.size), ndaybins))
    res = CK.native_pass(raw['cphase'], raw['flags'], 1, off, mem, daybinsize is None)
    err = {'daybins': centers, 'diff_dbins': widths}
    if detail is not None:
        detail['day'] = res
    rawlst = NP.degrees(NP.unwrap(NP.radians(NP.asarray(raw['lst']) * 15.0), discont=NP.pi, axis=0)) / 15.0
    if NP.any(rawlst > 24.0):
        rawlst -= 24.0
    if rawlst.shape[0] > 1 and lstbinsize is not None:
        size = lstbinsize / 3.6e3
        col = rawlst[:, 0]
        tres = NP.diff(col).min()
        textent = col.max() - col.min() + tres
        eps = 1e-10
        if size > tres:
            size = NP.clip(size, tres, textent)
            edges, err['lstbins'], err['dlstbins'] = CK._edges(col.min(), col.max(), tres, size)
            counts, ri = CK.binned_count(col, edges)
            lists = [ri[ri[k]:ri[k + 1]] for k in range(counts.size)]
        else:
            warnings.warn('LST bin size found to be smaller than the LST resolution in the data. No LST binning/averaging will be performed.')
            edges = NP.arange(col.min(), col.max() + tres + eps, tres)
            n = edges.size - 1
            err['dlstbins'] = edges[1:] - edges[:-1] if n > 1 else NP.asarray(tres).reshape(-1)
            err['lstbins'] = edges[:-1]
            err['lstbins'][0] += eps
            err['lstbins'][-1] -= eps
            lists = [[k] for k in range(n)]
        loff, lmem = CK.csr(lists)
        res = CK.binned_pass(res['cp_mean'], res['cp_median'], res['wts'], 0, loff, lmem)
        if detail is not None:
            detail['lst'] = res
            detail['lst_bins'] = (loff, lmem)
    else:
        err['lstbins'] = NP.mean(rawlst, axis=1)
        err['dlstbins'] = NP.asarray(lstbinsize).reshape(-1) if lstbinsize is not None else NP.zeros(1)
    pairs = pairs_of_pairs(ndaybins)
    err['list_of_pair_of_pairs'] = pairs
    if detail is not None:
        detail['binned'] = (res['cp_mean'], res['cp_median'], res['wts'])
    err.update(errinfo_of(diff_step(res['cp_mean'], res['cp_median'], res['wts'], pairs)))
    return err


def subtract(prelim, cphase):
    """(submodel, residual) of ClosurePhase.subtract on a prelim dictionary; 0 under the masks"""
    if not isinstance(cphase, MA.MaskedArray):
        cphase = MA.array(cphase, mask=NP.isnan(cphase))
    ndim = prelim['cphase']['median'].ndim
    cphase = cphase.reshape((1,) * (ndim - cphase.ndim) + cphase.shape)
    mm = MA.getmaskarray(cphase)
    cphase = MA.array(NP.where(mm, 0.0, cphase.data), mask=mm)
    model = NP.exp(1j * cphase.data)
    sub = {'cphase': cphase, 'eicp': MA.array(NP.where(mm, 0.0, model), mask=mm)}
    res = {'eicp': {}, 'cphase': {}}
    for key in ('mean', 'median'):
        pre = prelim['eicp'][key]
        mask = MA.getmaskarray(pre) | mm
        res['eicp'][key] = MA.array(NP.where(mask, 0.0, pre.data - model), mask=mask)
        res['cphase'][key] = MA.array(NP.where(mask, 0.0, NP.angle(pre.data / model)), mask=mask)
    return sub, res


# ---- bounds ---------------------------------------------------------------------------------------------------------------------

def member_bounds(detail):
    """(B_mean, B_median, ill) per element of the final binned stack: the phasor bound of tests/cphase_bins_checker.py:compare
    (phasor_bound(nbin, mod), plus in_err / mod after two passes) and whether the element is ill-conditioned: unmasked, with a mean or
    median phasor modulus below MOD_MIN in its own pass or, after two passes, in a day-pass member of its LST bin."""
    d = detail['day']
    low = (d['wts'] > 0.0) & ((d['mod_mean'] < MOD_MIN) | (d['mod_median'] < MOD_MIN))
    last, e1 = d, 0.0
    if 'lst' in detail:
        last = detail['lst']
        e1 = float(NP.max(CK.phasor_bound(d['nbin'], NP.minimum(d['mod_mean'], d['mod_median']))[d['wts'] > 0.0]))
        first_low = low
        low = (last['wts'] > 0.0) & ((last['mod_mean'] < MOD_MIN) | (last['mod_median'] < MOD_MIN))
        loff, lmem = detail['lst_bins']
        for k in range(len(loff) - 1):
            low[k] |= NP.any(first_low[lmem[loff[k]:loff[k + 1]]], axis=0)
    bm = CK.phasor_bound(last['nbin'], last['mod_mean']) + e1 / NP.maximum(last['mod_mean'], MOD_MIN)
    bd = CK.phasor_bound(last['nbin'], last['mod_median']) + e1 / NP.maximum(last['mod_median'], MOD_MIN)
    return bm, bd, low


def ill_elements(ill, pairs):
    """per difference element (n0, ncomb, ntriads, nchan): any of its four members is ill-conditioned"""
    return NP.stack([ill[:, r[0]] | ill[:, r[1]] | ill[:, r[2]] | ill[:, r[3]] for r in pairs], axis=1)


def ill_share(ill, pairs, masks):
    bad = ill_elements(ill, pairs)
    return sum(int(NP.sum(bad & ~m)) for m in masks), sum(int(NP.sum(~m)) for m in masks)


def compare_errinfo(got, ref, detail, label='', exact_members=False):
    """got, ref: errinfo dictionaries ('wts', 'eicp_diff', 'list_of_pair_of_pairs').  Masks equal; weights within 2 u relative; a
    difference of members a, b within 0.5 (B_a + B_b) + DIFF_CONST (exact_members: the members' phases are the same on both sides,
    B = 0, and no element is left out).  Otherwise ill-conditioned elements are left out, must be finite and stay within MAX_SHARE.  Returns the largest deviations."""
    pairs = [list(r) for r in ref['list_of_pair_of_pairs']]
    assert [list(r) for r in got['list_of_pair_of_pairs']] == pairs, (label, 'pairs')
    bm, bd, ill = member_bounds(detail)
    if exact_members:
        bm, bd = NP.zeros_like(bm), NP.zeros_like(bd)
    bad = ill_elements(ill, pairs)
    masks = [MA.getmaskarray(ref['wts'][str(g)]) for g in range(2)]
    nbad, ntot = ill_share(ill, pairs, masks)
    assert nbad <= MAX_SHARE * max(ntot, 1), (label, 'share of ill-conditioned points', nbad, ntot)
    worst = {}
    for g in range(2):
        key = str(g)
        cols = [(r[2 * g], r[2 * g + 1]) for r in pairs]
        gw, rw = got['wts'][key], ref['wts'][key]
        assert isinstance(gw, MA.MaskedArray) and gw.shape == rw.shape and gw.dtype == rw.dtype == NP.float64, (label, 'wts', key)
        assert NP.array_equal(MA.getmaskarray(gw), masks[g]), (label, 'wts mask', key)
        ok = ~masks[g]
        dev = NP.abs(gw.data - rw.data) / NP.where(ok, rw.data, 1.0)
        worst['wts' + key] = float(NP.max(dev[ok])) if NP.any(ok) else 0.0
        print('%s wts %s: largest relative deviation %.1f u' % (label, key, worst['wts' + key] / U))
        assert NP.all(dev[ok] <= 2.0 * U), (label, 'wts', key)
        for stat, b in (('mean', bm), ('median', bd)):
            gd, rd = got['eicp_diff'][key][stat], ref['eicp_diff'][key][stat]
            assert isinstance(gd, MA.MaskedArray) and gd.shape == rd.shape and gd.dtype == rd.dtype == NP.complex128, (label, stat, key)
            assert NP.array_equal(MA.getmaskarray(gd), masks[g]) and NP.array_equal(MA.getmaskarray(rd), masks[g]), (label, stat, key, 'mask')
            assert NP.all(NP.isfinite(gd.data)), (label, stat, key, 'not finite')
            bound = NP.stack([0.5 * (b[:, a] + b[:, c]) for a, c in cols], axis=1) + DIFF_CONST
            use = ok if exact_members else ok & ~bad
            dev = NP.abs(gd.data - rd.data)
            w = float(NP.max(dev[use])) if NP.any(use) else 0.0
            worst['diff%s_%s' % (key, stat)] = w
            print('%s eicp_diff %s %s: largest deviation %.3e (%.1f u), smallest bound %.1f u' % (
                label, key, stat, w, w / U, (float(NP.min(bound[use])) if NP.any(use) else 0.0) / U))
            assert NP.all(dev[use] <= bound[use]), (label, stat, key, w / U)
    return worst


# ---- the fixture ------------------------------------------------------------------------------------------------------------------

_GOLD = {}


def gold():
    import os
    if not _GOLD:
        _GOLD['npz'] = NP.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'golden_cpdiff.npz'))
    return _GOLD['npz']


def cases():
    import json
    return json.loads(str(gold()['cases']))


def case(name, pre='%s_in_'):
    """(raw, nchan, keyword arguments) of a case of the fixture"""
    nchan, kw = [(c[2], c[3]) for c in cases() if c[0] == name][0]
    return {k: gold()[(pre % name) + k] for k in ('cphase', 'flags', 'lst', 'days')}, nchan, kw


def _masked(key):
    g = gold()
    return MA.array(g[key], mask=g[key + '__mask']) if key + '__mask' in g.files else g[key]


def gold_errinfo(name):
    """the fixture's errinfo dictionary of a case, masked arrays rebuilt"""
    pre = name + '_out_'
    out = {k: gold()[pre + k] for k in ('daybins', 'diff_dbins', 'lstbins', 'dlstbins')}
    out['list_of_pair_of_pairs'] = gold()[pre + 'list_of_pair_of_pairs'].tolist()
    out['wts'] = {str(g): _masked(pre + 'wts_%d' % g) for g in range(2)}
    out['eicp_diff'] = {str(g): {s: _masked(pre + 'eicp_diff_%d_%s' % (g, s)) for s in ('mean', 'median')} for g in range(2)}
    return out


def gold_subtract(model):
    """(model, submodel, residual) of a subtract case of the fixture"""
    pre = 'subtract_%s_' % model
    sub = {k: _masked(pre + 'submodel_' + k) for k in ('cphase', 'eicp')}
    res = {q: {s: _masked(pre + 'residual_%s_%s' % (q, s)) for s in ('mean', 'median')} for q in ('eicp', 'cphase')}
    return gold()[pre + 'model'], sub, res


_REF = {}


def reference(name):
    """the checker's run of a case, computed once: (errinfo, detail)"""
    if name not in _REF:
        raw, nchan, kw = case(name)
        detail = {}
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            err = subsample_differencing({'raw': raw}, detail=detail, **kw)
        _REF[name] = (err, detail)
    return _REF[name]
