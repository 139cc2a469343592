"""Regenerate tests/golden/golden_cpdiff.npz from the reference's own subsample_differencing and subtract.

At generation time this reads the bodies of ClosurePhase.subsample_differencing (prisim/bispectrum_phase.py:2053-2249) and
ClosurePhase.subtract (:1996-2019) from a PRISim checkout and executes them under Python 3 on a stand-in ``self`` whose cpinfo holds
seeded inputs, as tests/golden/make_golden_cphase.py does for smooth_in_tbins (whose executed body gives subtract its binned phases).
The stand-in namespace supplies xrange = range, NP.int / NP.float / NP.complex, copy, OPS.binned_statistic in the reading of
tests/cphase_bins_checker.py:binned_count and OPS.is_broadcastable as numpy.broadcast_shapes.  No reference text is stored: only inputs
and outputs.  What the reference leaves under its masks (MA.empty) is stored as 0.

Inputs are those of make_golden_cphase.py:inputs (6 days, 3 triads, 0.4 rad of scatter, 30 % random flags and a fully flagged line);
the single-LST cases take the first LST of such a stack.

The GPU tests leave out difference elements of which any of the four members is ill-conditioned (a mean or median phasor modulus
below MOD_MIN in either pass, tests/cpdiff_checker.py:member_bounds); this script refuses to write a fixture in which their share of
the unmasked difference elements exceeds MAX_SHARE.

    python tests/golden/make_golden_cpdiff.py /path/to/PRISim
"""
import copy
import json
import os
import sys
import textwrap
import types
import warnings

import numpy as NP
import numpy.ma as MA

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import cphase_bins_checker as CK  # noqa: E402
import cpdiff_checker as DK  # noqa: E402
import make_golden_cphase as GC  # noqa: E402

MOD_MIN, MAX_SHARE = GC.MOD_MIN, GC.MAX_SHARE
# name, nlst, nchan, keyword arguments
CASES = [
    ('nd4_lst', 7, 5, {'ndaybins': 4, 'lstbinsize': 800.0}),        # 3 combinations
    ('nd5_lst', 7, 5, {'ndaybins': 5, 'lstbinsize': 800.0}),        # 15 combinations
    ('size_lst', 7, 5, {'daybinsize': 1.5, 'ndaybins': None, 'lstbinsize': 800.0}),   # 5 uneven bins
    ('below', 7, 5, {'ndaybins': 4, 'lstbinsize': 100.0}),          # no LST averaging
    ('onelst', 1, 5, {}),
    ('onelst_size', 1, 5, {'lstbinsize': 800.0}),                   # dlstbins = [800]
    ('nd4_lst_67', 7, 67, {'ndaybins': 4, 'lstbinsize': 800.0}),    # a wavefront boundary inside a row
]
SUBTRACT_SMOOTH = {'ndaybins': 2, 'lstbinsize': 800.0}


def _functions(ref_root):
    src = os.path.join(ref_root, 'prisim', 'bispectrum_phase.py')
    np_ns = types.SimpleNamespace(**{k: getattr(NP, k) for k in dir(NP) if not k.startswith('__')})
    np_ns.int, np_ns.float, np_ns.complex = int, float, complex

    def binned_statistic(x, statistic='count', bins=None):
        assert statistic == 'count'
        counts, ri = CK.binned_count(x, bins)
        return counts, NP.asarray(bins), None, ri

    def is_broadcastable(shp1, shp2):
        try:
            NP.broadcast_shapes(tuple(shp1), tuple(shp2))
        except ValueError:
            return False
        return True

    ns = {'NP': np_ns, 'MA': MA, 'OPS': types.SimpleNamespace(binned_statistic=binned_statistic, is_broadcastable=is_broadcastable),
          'xrange': range, 'warnings': warnings, 'copy': copy}
    exec('def ssd(self, daybinsize=None, ndaybins=4, lstbinsize=None):\n' + textwrap.indent(textwrap.dedent(GC._lines(src, 2053, 2249)), '    '), ns)
    exec('def subtract(self, cphase):\n' + textwrap.indent(textwrap.dedent(GC._lines(src, 1996, 2019)), '    '), ns)
    return ns['ssd'], ns['subtract']


def inputs(rng, nlst, nchan):
    raw = GC.inputs(rng, nchan=nchan)
    if nlst == 1:
        raw = {k: (v if k == 'days' else v[:1].copy()) for k, v in raw.items()}
    return raw


def standin(raw):
    self = GC.standin(raw)
    self.cpinfo['errinfo'] = {}
    return self


def _flatten(out, pre, d):
    for k, v in d.items():
        if isinstance(v, dict):
            _flatten(out, pre + k + '_', v)
        elif isinstance(v, MA.MaskedArray):
            mask = MA.getmaskarray(v)
            out[pre + k] = NP.where(mask, 0, NP.asarray(v.data))
            out[pre + k + '__mask'] = mask
        else:
            out[pre + k] = NP.asarray(v)


def main(ref_root):
    ssd, subtract = _functions(ref_root)
    smooth = GC._function(ref_root)
    rng = NP.random.default_rng(20261018)
    out = {'cases': NP.array(json.dumps([list(c) for c in CASES]))}
    low = total = 0
    for name, nlst, nchan, kw in CASES:
        raw = inputs(rng, nlst, nchan)
        self = standin(raw)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            ssd(self, **kw)
        pre = name + '_'
        for k, v in raw.items():
            out[pre + 'in_' + k] = v
        err = self.cpinfo['errinfo']
        out[pre + 'keys'] = NP.array(sorted(err.keys()))
        _flatten(out, pre + 'out_', err)
        # the share of ill-conditioned difference elements, under the reference's own masks
        detail = {}
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            DK.subsample_differencing({'raw': raw}, detail=detail, **kw)
        _, _, ill = DK.member_bounds(detail)
        nbad, ntot = DK.ill_share(ill, err['list_of_pair_of_pairs'], [MA.getmaskarray(err['wts'][str(g)]) for g in range(2)])
        low += nbad
        total += ntot
    share = low / float(total)
    print('difference elements with an ill-conditioned member (|z| / n < %g): %d of %d unmasked (%.3f %%)' % (MOD_MIN, low, total, 100 * share))
    assert share <= MAX_SHARE, 'too many ill-conditioned points for the GPU tests: choose other inputs'

    # subtract, after the reference's smooth_in_tbins
    raw = inputs(rng, 7, 5)
    base = standin(raw)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        smooth(base, **SUBTRACT_SMOOTH)
    shape = base.cpinfo['processed']['prelim']['cphase']['median'].shape
    full = 0.5 * rng.standard_normal(shape)
    full[1, 0, 2, 3] = NP.nan
    models = {'triadchan': 0.5 * rng.standard_normal(shape[2:]), 'full_nan': full}
    out['subtract_smooth'] = NP.array(json.dumps(SUBTRACT_SMOOTH))
    for k, v in raw.items():
        out['subtract_in_' + k] = v
    for mname, model in models.items():
        self = copy.deepcopy(base)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            subtract(self, model.copy())
        out['subtract_%s_model' % mname] = model
        for key in ('submodel', 'residual'):
            _flatten(out, 'subtract_%s_%s_' % (mname, key), self.cpinfo['processed'][key])
    path = os.path.join(HERE, 'golden_cpdiff.npz')
    NP.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print('golden_cpdiff.npz: %d bytes, %d arrays' % (size, len(out)))
    assert size < 400000


if __name__ == '__main__':
    main(sys.argv[1])
