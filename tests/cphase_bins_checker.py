"""numpy.ma restatement of the day and LST binning of closure phases (prisim/bispectrum_phase.py:ClosurePhase.smooth_in_tbins,
:1755-1974), the checker of prisim_cphase_bin and of prisim_amd.bispectrum_phase.  tests/test_cphase_bins.py pins it to
tests/golden/golden_cphase.npz, the reference's own statements executed (tests/golden/make_golden_cphase.py).

bin_pass is one pass in the terms of include/prisim_cpbins.h (a stack, an axis, a CSR pair of bins) written with numpy.ma's mean,
median and std, so that it states what the reference's masked-array calls give.  Where no member of a bin is unmasked the reference
leaves unspecified values under its mask; bin_pass writes there what the device documents (eicp = 1, everything else 0).  It also
returns, for the bounds of the GPU tests, the moduli of the mean and of the median phasor before normalisation.

smooth_in_tbins is the whole method on a cpinfo dictionary, every branch."""
import warnings

import numpy as NP
import numpy.ma as MA

QUANTITIES = ('wts', 'eicp_mean', 'eicp_median', 'cp_mean', 'cp_median', 'rms', 'mad')


def binned_count(x, edges):
    """The reading of OPS.binned_statistic(x, statistic='count', bins=edges) (astroutils is not a dependency): bin k holds the
    indices i with edges[k] <= x[i] < edges[k+1], in increasing i.  Returns (counts, ri), ri IDL's reverse-index vector: ri[ri[k]:ri[k+1]]
    are the members of bin k."""
    x = NP.asarray(x, dtype=NP.float64).ravel()
    edges = NP.asarray(edges, dtype=NP.float64).ravel()
    nb = edges.size - 1
    lists = [NP.nonzero((x >= edges[k]) & (x < edges[k + 1]))[0] for k in range(nb)]
    counts = NP.asarray([l.size for l in lists], dtype=NP.int64)
    head = nb + 1 + NP.concatenate(([0], NP.cumsum(counts)))
    return counts, NP.concatenate([head] + lists).astype(NP.int64)


def csr(lists):
    """offsets (nbins + 1,) int64 and members int32 of a list of index lists"""
    offsets = NP.concatenate(([0], NP.cumsum([len(l) for l in lists]))).astype(NP.int64)
    members = NP.concatenate([NP.asarray(l, dtype=NP.int32).ravel() for l in lists] + [NP.zeros(0, dtype=NP.int32)]).astype(NP.int32)
    return offsets, members


def bin_pass(pm, pd, wts, mask, axis, offsets, members, mad_ignores_flags=False):
    """One pass: pm the phases the mean and the rms are taken of, pd those of the median and the mad, wts the weights (their data are
    summed over all members), mask the members left out; all (n0, n1, ntriads, nchan).  Returns a dict of QUANTITIES, each with `axis`
    replaced by the bins, and 'mod_mean' / 'mod_median' (|mean phasor|, |median phasor|; 0 where nothing is unmasked), 'n' (unmasked
    members), 'nbin' (members of the bin)."""
    pm, pd, wts, mask = (NP.moveaxis(NP.asarray(a), axis, 0) for a in (pm, pd, wts, mask))
    nb = len(offsets) - 1
    shape = (nb,) + pm.shape[1:]
    out = {q: NP.zeros(shape, dtype=NP.complex128 if q.startswith('eicp') else NP.float64) for q in QUANTITIES}
    out['eicp_mean'] += 1.0
    out['eicp_median'] += 1.0
    out.update(mod_mean=NP.zeros(shape), mod_median=NP.zeros(shape), n=NP.zeros(shape, dtype=NP.int64),
               nbin=NP.zeros(shape, dtype=NP.int64))
    for k in range(nb):
        ind = NP.asarray(members[offsets[k]:offsets[k + 1]], dtype=NP.int64)
        out['nbin'][k] = ind.size
        if ind.size == 0:
            continue
        m = mask[ind]
        out['wts'][k] = NP.sum(wts[ind], axis=0)
        out['n'][k] = NP.sum(~m, axis=0)
        zmean = MA.mean(MA.array(NP.exp(1j * pm[ind]), mask=m), axis=0)
        emean = NP.exp(1j * NP.angle(zmean))
        zmed = MA.median(MA.array(NP.cos(pd[ind]), mask=m), axis=0) + 1j * MA.median(MA.array(NP.sin(pd[ind]), mask=m), axis=0)
        emed = NP.exp(1j * NP.angle(zmed))
        rms = MA.std(MA.array(pm[ind], mask=m), axis=0)
        amed = MA.array(NP.angle(emed))
        dev = NP.abs(MA.array(pd[ind], mask=(MA.getmaskarray(amed)[NP.newaxis] | NP.zeros(m.shape, dtype=bool)) if mad_ignores_flags else m)
                     - amed[NP.newaxis])
        mad = MA.median(dev, axis=0)
        out['mod_mean'][k] = MA.filled(NP.abs(zmean), 0.0)
        out['mod_median'][k] = MA.filled(NP.abs(zmed), 0.0)
        out['eicp_mean'][k] = MA.filled(emean, 1.0)
        out['eicp_median'][k] = MA.filled(emed, 1.0)
        out['cp_mean'][k] = MA.filled(NP.angle(emean), 0.0)
        out['cp_median'][k] = MA.filled(NP.angle(emed), 0.0)
        out['rms'][k] = MA.filled(rms, 0.0)
        out['mad'][k] = MA.filled(mad, 0.0)
    return {q: NP.moveaxis(v, 0, axis) for q, v in out.items()}


def native_pass(cphase, flags, axis, offsets, members, mad_ignores_flags=False):
    flags = NP.asarray(flags, dtype=bool)
    return bin_pass(cphase, cphase, NP.logical_not(flags).astype(NP.float64), flags, axis, offsets, members, mad_ignores_flags)


def binned_pass(cp_mean, cp_median, wts, axis, offsets, members):
    """A pass over the products of an earlier one: masked where its weights are <= 0"""
    return bin_pass(cp_mean, cp_median, wts, NP.asarray(wts) <= 0.0, axis, offsets, members)


def _store(prelim, res):
    mask = res['wts'] <= 0.0
    prelim['wts'] = MA.array(res['wts'], mask=mask)
    prelim['eicp'] = {'mean': MA.array(res['eicp_mean'], mask=mask), 'median': MA.array(res['eicp_median'], mask=mask)}
    prelim['cphase'] = {'mean': MA.array(res['cp_mean'], mask=mask), 'median': MA.array(res['cp_median'], mask=mask),
                        'rms': MA.array(res['rms'], mask=mask), 'mad': MA.array(res['mad'], mask=mask)}


def _edges(lo, hi, res, size, eps=1e-10):
    edges = NP.arange(lo, hi + res + eps, size)
    n = edges.size
    edges = NP.concatenate((edges, [edges[-1] + size + eps]))
    if n > 1:
        widths = edges[1:] - edges[:-1]
        centers = edges[:-1] + 0.5 * widths
    else:
        widths = NP.asarray(size).reshape(-1)
        centers = edges[0] + 0.5 * widths
    return edges, centers, widths


def smooth_in_tbins(cpinfo, daybinsize=None, ndaybins=None, lstbinsize=None, detail=None):
    """The method on cpinfo = {'raw': {'cphase', 'flags', 'lst', 'days'}, 'processed': {'prelim': {...}}}: fills and returns
    cpinfo['processed']['prelim'].  detail: a dict that receives the bin_pass result of every pass run, under 'day' and 'lst'."""
    raw = cpinfo['raw']
    prelim = cpinfo.setdefault('processed', {}).setdefault('prelim', {})
    if (ndaybins is not None) and (daybinsize is not None):
        raise ValueError('Only one of daybinsize or ndaybins should be set')
    days = NP.asarray(raw['days'])
    if daybinsize is not None:
        dres = NP.diff(days).min()
        dextent = days.max() - days.min() + dres
        if not daybinsize > dres:
            raise ValueError('daybinsize must exceed the day resolution')
        daybinsize = NP.clip(daybinsize, dres, dextent)
        edges, centers, widths = _edges(days.min(), days.max(), dres, daybinsize)
        counts, ri = binned_count(days, edges)
        off, mem = csr([ri[ri[k]:ri[k + 1]] for k in range(counts.size)])
        res = native_pass(raw['cphase'], raw['flags'], 1, off, mem, False)
    elif ndaybins is not None:
        split = NP.array_split(days, ndaybins)
        centers = NP.asarray([NP.mean(d) for d in split])
        widths = NP.asarray([d.max() - d.min() for d in split])
        off, mem = csr(NP.array_split(NP.arange(days.size), ndaybins))
        res = native_pass(raw['cphase'], raw['flags'], 1, off, mem, True)
    if (daybinsize is not None) or (ndaybins is not None):
        prelim['daybins'], prelim['diff_dbins'] = centers, widths
        if detail is not None:
            detail['day'] = res
        _store(prelim, res)

    rawlst = NP.degrees(NP.unwrap(NP.radians(NP.asarray(raw['lst']) * 15.0), discont=NP.pi, axis=0)) / 15.0
    if NP.any(rawlst > 24.0):
        rawlst -= 24.0
    if rawlst.shape[0] > 1 and lstbinsize is not None:
        lstbinsize = lstbinsize / 3.6e3
        col = rawlst[:, 0]
        tres = NP.diff(col).min()
        textent = col.max() - col.min() + tres
        eps = 1e-10
        if lstbinsize > tres:
            lstbinsize = NP.clip(lstbinsize, tres, textent)
            edges, centers, widths = _edges(col.min(), col.max(), tres, lstbinsize)
            prelim['lstbins'], prelim['dlstbins'] = centers, widths
            counts, ri = binned_count(col, edges)
            lists = [ri[ri[k]:ri[k + 1]] for k in range(counts.size)]
        else:
            warnings.warn('LST bin size found to be smaller than the LST resolution in the data. No LST binning/averaging will be performed.')
            lstbinsize = tres
            edges = NP.arange(col.min(), col.max() + lstbinsize + eps, lstbinsize)
            n = edges.size - 1
            prelim['dlstbins'] = edges[1:] - edges[:-1] if n > 1 else NP.asarray(lstbinsize).reshape(-1)
            prelim['lstbins'] = edges[:-1]
            prelim['lstbins'][0] += eps
            prelim['lstbins'][-1] -= eps
            lists = [[k] for k in range(n)]
        off, mem = csr(lists)
        if 'wts' not in prelim:
            res = native_pass(raw['cphase'], raw['flags'], 0, off, mem, False)
        else:
            res = binned_pass(prelim['cphase']['mean'].data, prelim['cphase']['median'].data, prelim['wts'].data, 0, off, mem)
        _store(prelim, res)
        if detail is not None:
            detail['lst'] = res
    if rawlst.shape[0] <= 1 or lstbinsize is None:
        prelim['lstbins'] = NP.mean(rawlst, axis=1)
        prelim['dlstbins'] = NP.asarray(lstbinsize).reshape(-1) if lstbinsize is not None else NP.zeros(1)
    return prelim


# ---- bounds of the comparisons, in units of u = 2^-53 (tests/test_gpu_cphase_bins.py derives them) ------------------------------------

U = 2.0 ** -53
MOD_MIN = 0.05          # points whose phasor modulus |z| / n is below this are left out of the phasor and mad comparisons
MAX_SHARE = 0.02        # and may be this share of the unmasked points at most
PASS_TO_PRELIM = {'wts': ('wts',), 'eicp_mean': ('eicp', 'mean'), 'eicp_median': ('eicp', 'median'), 'cp_mean': ('cphase', 'mean'),
                  'cp_median': ('cphase', 'median'), 'rms': ('cphase', 'rms'), 'mad': ('cphase', 'mad')}


def phasor_bound(nbin, mod):
    return (4.0 * nbin + 8.0) * U / NP.maximum(mod, MOD_MIN) + 32.0 * U


def rms_bound(nbin):
    return (4.0 * nbin + 8.0) * U * NP.pi


def phasor_deviation(a, b):
    """|exp(ia) - exp(ib)| of two arrays of phases, or |a - b| of two arrays of unit phasors"""
    if NP.iscomplexobj(a):
        return NP.abs(a - b)
    return NP.abs(NP.exp(1j * a) - NP.exp(1j * b))


def compare(got, ref, aux, in_err=0.0, label=''):
    """got, ref: dicts of QUANTITIES (plain arrays; masked arrays are also compared mask for mask); aux: a bin_pass result of the same
    bins, for 'mod_mean', 'mod_median' and 'nbin'; in_err: bound of the error of the input phases of `got` against those of `ref` (a
    second pass over device products).  Asserts the bounds and returns the largest deviations per quantity."""
    for q in QUANTITIES:
        if isinstance(ref[q], MA.MaskedArray) and isinstance(got[q], MA.MaskedArray):
            assert NP.array_equal(MA.getmaskarray(got[q]), MA.getmaskarray(ref[q])), (label, q, 'mask')
    g = {q: MA.getdata(got[q]) for q in QUANTITIES}
    r = {q: MA.getdata(ref[q]) for q in QUANTITIES}
    for q in QUANTITIES:
        assert g[q].shape == r[q].shape and g[q].dtype == r[q].dtype, (label, q, g[q].shape, r[q].shape)
        assert NP.all(NP.isfinite(g[q])), (label, q, 'not finite')
    good = r['wts'] > 0.0
    assert NP.array_equal(g['wts'][good], r['wts'][good]) and NP.array_equal(g['wts'] <= 0.0, ~good), (label, 'wts')
    nbin = aux['nbin']
    okm, okd = good & (aux['mod_mean'] >= MOD_MIN), good & (aux['mod_median'] >= MOD_MIN)
    ngood = max(int(NP.sum(good)), 1)
    assert 1.0 - NP.sum(okm & okd) / float(ngood) <= MAX_SHARE, (label, 'share of ill-conditioned points')
    bm = phasor_bound(nbin, aux['mod_mean']) + in_err / NP.maximum(aux['mod_mean'], MOD_MIN)
    bd = phasor_bound(nbin, aux['mod_median']) + in_err / NP.maximum(aux['mod_median'], MOD_MIN)
    worst = {}
    for q, ok, bound in (('eicp_mean', okm, bm), ('cp_mean', okm, bm), ('eicp_median', okd, bd), ('cp_median', okd, bd),
                         ('rms', good, rms_bound(nbin) + 2.0 * in_err), ('mad', okd, rms_bound(nbin) + 2.0 * in_err + bd)):
        dev = NP.abs(g[q] - r[q]) if q in ('rms', 'mad') else phasor_deviation(g[q], r[q])
        bound = NP.broadcast_to(bound, dev.shape)
        worst[q] = float(NP.max(dev[ok])) if NP.any(ok) else 0.0
        print('%s %s: largest deviation %.3e (%.1f u), smallest bound %.3e' % (label, q, worst[q], worst[q] / U,
                                                                                  float(NP.min(bound[ok])) if NP.any(ok) else 0.0))
        assert NP.all(dev[ok] <= bound[ok]), (label, q, worst[q])
    return worst


def prelim_quantities(prelim):
    """the seven binned quantities of a cpinfo['processed']['prelim'] under the names of a pass"""
    out = {}
    for q, path in PASS_TO_PRELIM.items():
        v = prelim
        for k in path:
            v = v[k]
        out[q] = v
    return out
