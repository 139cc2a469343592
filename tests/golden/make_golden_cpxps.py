"""Regenerate tests/golden/golden_cpxps.npz from the reference's own compute_power_spectrum and compute_power_spectrum_uncertainty.

At generation time this reads statements of ClosurePhaseDelaySpectrum (prisim/bispectrum_phase.py) from a PRISim checkout and executes
them under Python 3 on a stand-in ``self``: subset (:2823-2884); of compute_power_spectrum the normalisation of its arguments up to the
head of the loop over the samplings (:3261-3393) and the body of that loop behind the astropy lines (:3418-3601); of
compute_power_spectrum_uncertainty the matching ranges (:3993-4139, :4164-4357).  In place of the astropy lines (:3395-3416) wl, z,
kprll and factor are injected, computed by this package (prisim_amd.bispectrum_phase.ClosurePhaseDelaySpectrum.power_factor, units
'Jy').  The stand-in namespace supplies U.Unit(...) = U.Jy = 1; an ndarray subclass with .si, .value, .unit and .to in the place of a
Quantity; list-returning map and zip; NP.int / float / complex / bool; NP.sum and NP.median taking an array as axis; NP.nanmean,
NP.nanmedian and NP.nansum that keep the subclass; and OPS.array_trace in the reading of prisim_amd/dsp_readings.py.  No reference
text is stored: only inputs and outputs.

The spectra are seeded random numbers, all finite.  This script asserts that the only non-finite outputs are the structural NaN of LST
axes that are crossed and not collapsed (LST bin i < shift s) and refuses to write the file otherwise.

    python tests/golden/make_golden_cpxps.py /path/to/PRISim
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
sys.path.insert(0, HERE)
from prisim_amd import dsp_readings as DSP  # noqa: E402
from prisim_amd import bispectrum_phase as BSP  # noqa: E402

NSPW, NLST, NDAYS, NPAIRS, NTRIADS, NCHAN = 2, 4, 3, 3, 3, 6
NLAGS = {'oversampled': 8, 'resampled': 4}
TRIADS = [[0, 1, 2], [0, 2, 3], [1, 2, 4]]
POOLS = ('whole', 'submodel', 'residual')

# 'unc': compute_power_spectrum_uncertainty.  Weights are real so that the cases are plain JSON.  'keep': the (sampling, pool) pairs whose
# outputs are stored, 'all' for the small results: the reference computes every pool of both samplings in every case, and the file has
# to stay small.
CASES = [
    {'name': 'cohdays_x13_c3', 'unc': False, 'autoinfo': {'axes': [2]}, 'xinfo': {'axes': [1, 3], 'collapse_axes': [3]},
     'keep': [['oversampled', 'whole']]},
    {'name': 'x13_c13', 'unc': False, 'autoinfo': {'axes': None}, 'xinfo': {'axes': [1, 3], 'collapse_axes': [1, 3]},
     'keep': [['oversampled', 'whole'], ['oversampled', 'submodel']]},
    {'name': 'x13_c31_avgcov', 'unc': False, 'autoinfo': {'axes': None}, 'xinfo': {'axes': [1, 3], 'collapse_axes': [3, 1], 'avgcov': True},
     'keep': 'all'},
    {'name': 'x23_c23', 'unc': False, 'autoinfo': {'axes': None}, 'xinfo': {'axes': [2, 3], 'collapse_axes': [2, 3]},
     'keep': [['oversampled', 'whole']]},
    {'name': 'weights', 'unc': False, 'autoinfo': {'axes': [2], 'wts': [[1.0, 0.5, 2.0]]},
     'xinfo': {'axes': [1, 3], 'collapse_axes': [1, 3], 'dlst_range': [0, 12],
               'wts': {'preX': [[1.0, 0.8, 1.25, 0.9], [0.7, 1.0, 1.3]], 'postX': [[1.0, 0.5, 0.25], [0.2, 0.6, 1.0, 0.6, 0.2]],
                       'preXnorm': False, 'postXnorm': True}}, 'keep': 'all'},
    {'name': 'selection', 'unc': False, 'autoinfo': {'axes': None}, 'xinfo': {'axes': [1, 2, 3], 'collapse_axes': [2]},
     'selection': {'lst': [0, 2, 3], 'triads': [[1, 2, 4], [0, 1, 2]]}, 'keep': [['resampled', 'residual']]},
    {'name': 'unc_x13_c3', 'unc': True, 'autoinfo': {'axes': None}, 'xinfo': {'axes': [1, 3], 'collapse_axes': [3]},
     'keep': [['oversampled', 'errinfo']]},
    {'name': 'unc_x123_c123_avgcov', 'unc': True, 'autoinfo': {'axes': None},
     'xinfo': {'axes': [1, 2, 3], 'collapse_axes': [1, 2, 3], 'avgcov': True}, 'keep': 'all'},
]


class Q(NP.ndarray):
    """what the reference's statements ask of a Quantity, with every unit 1"""
    si = property(lambda self: self)
    value = property(lambda self: NP.asarray(self))
    unit = property(lambda self: NP.asarray(1.0).view(Q))

    def to(self, unit):
        return self


def _lines(path, a, b):
    with open(path) as fh:
        return ''.join(fh.readlines()[a - 1:b])


def _namespace():
    np_ns = types.SimpleNamespace(**{k: getattr(NP, k) for k in dir(NP) if not k.startswith('__')})
    np_ns.int, np_ns.float, np_ns.complex, np_ns.bool = int, float, complex, bool

    def axis_arg(fn):
        def call(x, axis=None, **kw):
            if isinstance(axis, (list, NP.ndarray)):
                axis = tuple(int(ax) for ax in NP.asarray(axis).reshape(-1))
            return fn(x, axis=axis, **kw)
        return call

    def keeps(fn):
        def call(x, *args, **kw):
            out = fn(NP.asarray(x), *args, **kw)
            return NP.asarray(out).view(Q) if isinstance(x, Q) else out
        return call

    np_ns.sum, np_ns.median = axis_arg(NP.sum), axis_arg(NP.median)
    np_ns.nanmean, np_ns.nanmedian, np_ns.nansum = keeps(NP.nanmean), keeps(NP.nanmedian), keeps(NP.nansum)
    return {'NP': np_ns, 'MA': MA, 'copy': copy, 'U': types.SimpleNamespace(Unit=lambda s: 1, Jy=1),
            'OPS': types.SimpleNamespace(array_trace=DSP.array_trace), 'map': lambda *a: list(map(*a)), 'zip': lambda *a: list(zip(*a))}


def _functions(ref_root, inject):
    src = os.path.join(ref_root, 'prisim', 'bispectrum_phase.py')
    ns = _namespace()
    ns['_inject'] = inject
    exec('def subset(self, selection=None):\n' + textwrap.indent(textwrap.dedent(_lines(src, 2823, 2884)), '    '), ns)
    sig = '(self, cpds=None, selection=None, autoinfo=None, xinfo=None, cosmo=None, units="Jy", beamparms=None):\n'
    line = ' ' * 12 + 'wl, z, kprll, factor = _inject(cpds[smplng])\n'
    for name, (a0, a1), (b0, b1) in (('cps', (3261, 3393), (3418, 3601)), ('cpsu', (3993, 4139), (4164, 4357))):
        exec('def ' + name + sig + textwrap.indent(textwrap.dedent(_lines(src, a0, a1) + line + _lines(src, b0, b1)), '    '), ns)
    return ns['subset'], ns['cps'], ns['cpsu']


def inputs(rng):
    """the stand-in's cpinfo and the two samplings of FT's result, from seeded random numbers"""
    def spectra(n2, nlags):
        return rng.standard_normal((NSPW, NLST, n2, NTRIADS, nlags)) + 1j * rng.standard_normal((NSPW, NLST, n2, NTRIADS, nlags))

    def twts(n2):
        w = rng.integers(1, 6, size=(NLST, n2, NTRIADS, NCHAN)).astype(NP.float64)
        return MA.array(w, mask=NP.zeros(w.shape, dtype=bool))

    f = 150e6 + 1e5 * NP.arange(NCHAN)
    bins = {'lstbins': 1.0 + 0.07 * NP.arange(NLST), 'dlstbins': NP.full(NLST, 0.07)}
    cpinfo = {'raw': {'triads': NP.asarray(TRIADS)},
              'processed': {'prelim': dict(bins, daybins=2458000.0 + 2.0 * NP.arange(NDAYS), diff_dbins=NP.full(NDAYS, 2.0), wts=twts(NDAYS))},
              'errinfo': dict(bins, daybins=2458000.0 + 1.5 * NP.arange(4), diff_dbins=NP.full(4, 1.5),
                              list_of_pair_of_pairs=[[0, 1, 2, 3], [0, 2, 1, 3], [0, 3, 1, 2]])}
    tw, tw0, tw1 = cpinfo['processed']['prelim']['wts'], twts(NPAIRS), twts(NPAIRS)
    fw = rng.uniform(0.1, 1.0, (NSPW, NCHAN))
    cpds = {}
    for smp, nlags in NLAGS.items():
        cpds[smp] = {'freq_center': NP.asarray([150.15e6, 150.35e6]), 'bw_eff': NP.asarray([2.0e5, 3.0e5]), 'shape': 'bhw', 'freq_wts': fw,
                     'lag_corr_length': NCHAN / NP.sum(fw, axis=-1), 'lags': DSP.spectral_axis(nlags, delx=1e5 * 12 / nlags, shift=True),
                     'whole': {'dspec': {'twts': tw, 'mean': spectra(NDAYS, nlags), 'median': spectra(NDAYS, nlags)}},
                     'submodel': {'dspec': spectra(NDAYS, nlags)},
                     'residual': {'dspec': {'twts': tw, 'mean': spectra(NDAYS, nlags), 'median': spectra(NDAYS, nlags)}},
                     'errinfo': {'dspec0': {'twts': tw0, 'mean': spectra(NPAIRS, nlags), 'median': spectra(NPAIRS, nlags)},
                                 'dspec1': {'twts': tw1, 'mean': spectra(NPAIRS, nlags), 'median': spectra(NPAIRS, nlags)}}}
    return f, cpinfo, cpds


def arguments(spec):
    """(selection, autoinfo, xinfo) of a case as the methods take them: lists of weights as lists of numpy arrays"""
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


def structural_nan(spec, x, nshift_first):
    """where an output of the case may be NaN: LST bin i < shift s of an LST axis that is crossed and not collapsed"""
    xi = spec['xinfo']
    if 1 not in xi['axes'] or 1 in xi['collapse_axes']:
        return NP.zeros(x.shape, dtype=bool)
    s = NP.asarray(nshift_first).reshape(-1, 1)
    assert s.size == x.shape[1]
    bad = NP.arange(x.shape[2]).reshape(1, -1) < s
    return NP.broadcast_to(bad.reshape((1,) + bad.shape + (1,) * (x.ndim - 3)), x.shape)


def main(ref_root):
    rng = NP.random.default_rng(20261101)
    f, cpinfo, cpds = inputs(rng)
    maker = BSP.ClosurePhaseDelaySpectrum.__new__(BSP.ClosurePhaseDelaySpectrum)

    def inject(ds):
        z, kprll, factor = maker.power_factor(ds, units='Jy')
        return NP.asarray(ds['freq_center']) * 0 + 1.0, z, kprll, NP.asarray(factor).view(Q)

    subset, cps, cpsu = _functions(ref_root, inject)
    self = types.SimpleNamespace(cPhase=types.SimpleNamespace(cpinfo=cpinfo), f=f, cPhaseDS=cpds['oversampled'],
                                 cPhaseDS_resampled=cpds['resampled'])
    self.subset = lambda selection=None: subset(self, selection)

    out = {'cases': NP.array(json.dumps(CASES)), 'in__f': f, 'in__triads': cpinfo['raw']['triads'],
           'in__pairs': NP.asarray(cpinfo['errinfo']['list_of_pair_of_pairs'])}
    for grp, d in (('prelim', cpinfo['processed']['prelim']), ('errinfo', cpinfo['errinfo'])):
        for k in ('lstbins', 'dlstbins', 'daybins', 'diff_dbins'):
            out['in__%s__%s' % (grp, k)] = d[k]
    for smp, ds in cpds.items():
        pre = 'in__%s__' % smp
        for k in ('freq_center', 'bw_eff', 'freq_wts', 'lag_corr_length', 'lags'):
            out[pre + k] = NP.asarray(ds[k])
        out[pre + 'shape'] = NP.array(ds['shape'])
        z, kprll, factor = maker.power_factor(ds, units='Jy')
        out[pre + 'z'], out[pre + 'kprll'], out[pre + 'factor'] = z, kprll, factor
        out[pre + 'submodel'] = ds['submodel']['dspec']
        for pool in ('whole', 'residual'):
            for stat in ('mean', 'median'):
                out[pre + pool + '__' + stat] = ds[pool]['dspec'][stat]
        for q in ('dspec0', 'dspec1'):
            out[pre + q + '__twts'] = MA.getdata(ds['errinfo'][q]['twts'])
            for stat in ('mean', 'median'):
                out[pre + q + '__' + stat] = ds['errinfo'][q][stat]
    out['in__twts'] = MA.getdata(cpinfo['processed']['prelim']['wts'])

    for spec in CASES:
        name = spec['name']
        sel, auto, xinfo = arguments(spec)
        with warnings.catch_warnings(), NP.errstate(all='ignore'):
            warnings.simplefilter('ignore')
            res = (cpsu if spec['unc'] else cps)(self, cpds=None, selection=sel, autoinfo=auto, xinfo=xinfo, units='Jy')
        for k in ('triads', 'triads_ind', 'lst', 'lst_ind', 'dlst', 'days', 'day_ind', 'dday', 'lstXoffsets'):
            out['%s__top__%s' % (name, k)] = NP.asarray(res[k])
        dlstbin = NP.mean(cpinfo['processed']['prelim']['dlstbins'])
        first = NP.rint(NP.asarray(res['lstXoffsets']) / dlstbin).astype(int)
        nbad = ntot = 0
        meta = None
        for smp in NLAGS:
            for pool in (('errinfo',) if spec['unc'] else POOLS):
                r = res[smp][pool]
                pre = '%s__%s__%s__' % (name, smp, pool)
                for stat in ('mean', 'median'):
                    x = NP.asarray(r[stat])
                    assert x.dtype == NP.complex128, (name, smp, pool, stat, x.dtype)
                    bad = ~NP.isfinite(x)
                    assert NP.array_equal(bad, structural_nan(spec, x, first)), (name, smp, pool, stat, 'non-finite values that are not structural')
                    nbad += int(bad.sum())
                    ntot += bad.size
                    if spec['keep'] == 'all' or [smp, pool] in spec['keep']:
                        out[pre + stat] = x
                # what goes with the spectra (the same for every pool and sampling of a case), as JSON
                this = {key: {str(ax): NP.asarray(v).tolist() for ax, v in r[key].items()} for key in ('diagoffsets', 'diagweights', 'axesmap')}
                this.update({'nsamples_incoh': int(r['nsamples_incoh']), 'nsamples_coh': int(r['nsamples_coh'])})
                assert meta is None or meta == this, (name, smp, pool)
                meta = this
        out[name + '__meta'] = NP.array(json.dumps(meta))
        print('%s: %d of %d output values are structural NaN' % (name, nbad, ntot))
    buf = io.BytesIO()
    NP.savez_compressed(buf, **out)
    size = buf.getbuffer().nbytes
    print('golden_cpxps.npz: %d bytes, %d arrays' % (size, len(out)))
    assert size < 400000, 'the fixture is too large'
    with open(os.path.join(HERE, 'golden_cpxps.npz'), 'wb') as fh:
        fh.write(buf.getvalue())


if __name__ == '__main__':
    main(sys.argv[1])
