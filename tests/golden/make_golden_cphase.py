"""Regenerate tests/golden/golden_cphase.npz from the reference's own day and LST binning of closure phases.

At generation time this reads the body of ClosurePhase.smooth_in_tbins (prisim/bispectrum_phase.py:1755-1974) from a PRISim checkout
and executes it under Python 3 on a stand-in ``self`` whose cpinfo holds seeded inputs.  The stand-in namespace supplies xrange = range,
NP.int / NP.float, and OPS.binned_statistic(x, statistic='count', bins=edges) in the reading of tests/cphase_bins_checker.py:binned_count
(bin k holds the indices i with edges[k] <= x[i] < edges[k+1], in increasing i; ri is IDL's reverse-index vector).  No reference text
is stored: only inputs and outputs.

One case per branch (CASES).  Phases are a smooth model plus 0.4 rad of Gaussian scatter, wrapped to (-pi, pi]; 30 % of the samples
are flagged at random; one (lst, triad, channel) line is flagged on every day at two neighbouring LSTs, so that fully masked bins
occur on both axes; and two bins are left with exactly two unflagged members, for the even-count median.

The GPU tests leave points whose phasor modulus |z| / n is below MOD_MIN out of the phasor and mad comparisons; this script refuses to
write a fixture in which their share of the unmasked points exceeds MAX_SHARE.

    python tests/golden/make_golden_cphase.py /path/to/PRISim
"""
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
import cphase_bins_checker as CK  # noqa: E402

MOD_MIN, MAX_SHARE = 0.05, 0.02
DAYS = [0.0, 1.0, 2.0, 3.0, 5.0, 6.0]
# name, nchan, keyword arguments
CASES = [
    ('daybinsize', 5, {'daybinsize': 2.5}),                        # uneven bins: 3, 1 and 2 days
    ('ndaybins', 5, {'ndaybins': 4}),                              # array_split: 2, 2, 1, 1
    ('lst', 5, {'lstbinsize': 800.0}),                             # on an LST axis that wraps through 24 h
    ('day_lst', 5, {'ndaybins': 2, 'lstbinsize': 800.0}),          # the LST pass on the day-binned stack
    ('below', 5, {'lstbinsize': 100.0}),                           # below the resolution of 360 s
    ('none', 5, {}),
    ('day_lst_67', 67, {'ndaybins': 2, 'lstbinsize': 800.0}),      # a wavefront boundary inside a row
]


def _lines(path, a, b):
    with open(path) as fh:
        return ''.join(fh.readlines()[a - 1:b])


def _function(ref_root):
    src = os.path.join(ref_root, 'prisim', 'bispectrum_phase.py')
    np_ns = types.SimpleNamespace(**{k: getattr(NP, k) for k in dir(NP) if not k.startswith('__')})
    np_ns.int, np_ns.float = int, float

    def binned_statistic(x, statistic='count', bins=None):
        assert statistic == 'count'
        counts, ri = CK.binned_count(x, bins)
        return counts, NP.asarray(bins), None, ri

    ns = {'NP': np_ns, 'MA': MA, 'OPS': types.SimpleNamespace(binned_statistic=binned_statistic), 'xrange': range, 'warnings': warnings}
    body = textwrap.indent(textwrap.dedent(_lines(src, 1755, 1974)), '    ')
    exec('def smooth(self, daybinsize=None, ndaybins=None, lstbinsize=None):\n' + body, ns)
    return ns['smooth']


def inputs(rng, nlst=7, ntriads=3, nchan=5):
    days = NP.asarray(DAYS)
    nd = days.size
    lst = (23.71 + 0.1 * NP.arange(nlst)[:, None] + 0.001 * NP.arange(nd)[None, :]) % 24.0
    model = (NP.asarray([0.3, 3.0, -1.5])[None, None, :, None] + 0.8 * NP.sin(2 * NP.pi * NP.arange(nchan) / nchan)[None, None, None, :]
             + 0.03 * NP.arange(nlst)[:, None, None, None] + NP.zeros((nlst, nd, ntriads, nchan)))
    cphase = model + 0.4 * rng.standard_normal(model.shape)
    cphase = -((-cphase + NP.pi) % (2 * NP.pi) - NP.pi)                # (-pi, pi]
    flags = rng.uniform(size=model.shape) < 0.3
    flags[3:5, :, 0, 1] = True                                         # a line flagged on every day, at both LSTs of one LST bin
    flags[0, 0:3, 1, 2] = [False, True, False]                         # exactly two unflagged members of a day bin of three
    flags[0:3, 0, 2, 3] = [False, True, False]                         # and of an LST bin of three
    return {'cphase': cphase, 'flags': flags, 'lst': lst, 'days': days}


def standin(raw):
    cp = MA.array(raw['cphase'].astype(NP.float64), mask=raw['flags'])
    native = {'cphase': cp, 'eicp': NP.exp(1j * cp), 'wts': MA.array(NP.logical_not(raw['flags']).astype(float), mask=raw['flags'])}
    return types.SimpleNamespace(cpinfo={'raw': {k: v.copy() for k, v in raw.items()}, 'processed': {'native': native, 'prelim': {}}})


def _flatten(out, pre, d):
    for k, v in d.items():
        if isinstance(v, dict):
            _flatten(out, pre + k + '_', v)
        elif isinstance(v, MA.MaskedArray):
            out[pre + k] = NP.asarray(v.data)
            out[pre + k + '__mask'] = MA.getmaskarray(v)
        else:
            out[pre + k] = NP.asarray(v)


def main(ref_root):
    smooth = _function(ref_root)
    rng = NP.random.default_rng(20261017)
    out = {'cases': NP.array(json.dumps([[name, nchan, kw] for name, nchan, kw in CASES]))}
    low = total = 0
    for name, nchan, kw in CASES:
        raw = inputs(rng, nchan=nchan)
        self = standin(raw)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            smooth(self, **kw)
        pre = name + '_'
        for k, v in raw.items():
            out[pre + 'in_' + k] = v
        prelim = self.cpinfo['processed']['prelim']
        out[pre + 'keys'] = NP.array(sorted(prelim.keys()))
        _flatten(out, pre + 'out_', prelim)
        # the share of ill-conditioned points, from the reference's own inputs and masks
        detail = {}
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            CK.smooth_in_tbins({'raw': raw}, detail=detail, **kw)
        for res in detail.values():
            good = res['wts'] > 0.0
            low += int(NP.sum(good & ((res['mod_mean'] < MOD_MIN) | (res['mod_median'] < MOD_MIN))))
            total += int(NP.sum(good))
    share = low / float(total)
    print('points with |z| / n < %g: %d of %d unmasked (%.3f %%)' % (MOD_MIN, low, total, 100 * share))
    assert share <= MAX_SHARE, 'too many ill-conditioned points for the GPU tests: choose other inputs'
    path = os.path.join(HERE, 'golden_cphase.npz')
    NP.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print('golden_cphase.npz: %d bytes, %d arrays' % (size, len(out)))
    assert size < 400000


if __name__ == '__main__':
    main(sys.argv[1])
