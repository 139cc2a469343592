"""Regenerate tests/golden/golden_cpft.npz from the reference's own ClosurePhaseDelaySpectrum.FT.

At generation time this reads the body of ClosurePhaseDelaySpectrum.FT (prisim/bispectrum_phase.py:2573-2784) from a PRISim checkout
and executes it under Python 3 on a stand-in ``self`` whose cPhase.cpinfo comes from the reference's own smooth_in_tbins, subtract and
subsample_differencing (executed as tests/golden/make_golden_cphase.py and make_golden_cpdiff.py do) on the seeded inputs of
make_golden_cphase.py:inputs, cut to the case's LSTs and triads.  The stand-in namespace supplies the DSP / LKP modules of
make_golden_subband.py (prisim_amd/dsp_readings.py; FT1D read as fftshift(ifft(.))), NP.int / NP.float / NP.float_, copy and an
RI.InterferometerArray that nothing is an instance of.  No reference text is stored: only inputs and outputs.

Before FT is executed the data under every mask of its inputs are set to the values this package documents (1 + 0i under the masks
of the binned phasors, 0 under those of the residuals, the sub-model and the differences): the reference transforms the .data under
its masks, whose content it leaves unspecified.

Every case passes freq_center and the visibilities of one reference LST (without them the reference cannot run), one case all-ones
visibilities, where the scale is exactly sqrt(1/3).  Every case flags one whole (LST bin, day bin, triad) row, whose weights then
average to 0: the reference divides 0 by 0 there.  This script asserts that the reference's non-finite rows are exactly the rows of
zero mean weight and that they are at most 10 % of the rows of the case's spectra, and refuses to write the file otherwise.

    python tests/golden/make_golden_cpft.py /path/to/PRISim
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
import cpft_checker as FK  # noqa: E402
import make_golden_cphase as GC  # noqa: E402
import make_golden_cpdiff as GD  # noqa: E402
from make_golden_subband import _namespace  # noqa: E402

DF = 1e5
# bw_eff and freq_center in channels.  nlst 1: one LST, four day bins; nlst 5: two LST bins of 1008 s, two day bins.
CASES = [
    {'name': 'm32', 'nchan': 16, 'pad': 1.0, 'shape': 'rect', 'bw_eff': [8.0], 'freq_center': [8.0], 'apply_flags': True,
     'resample': True, 'model': 'triadchan', 'vis_ones': True, 'nlst': 1, 'ntriads': 2},
    {'name': 'm128_bhw', 'nchan': 64, 'pad': 1.0, 'shape': 'bhw', 'bw_eff': [6.0, 4.2], 'freq_center': [40.0, 17.0], 'apply_flags': True,
     'resample': True, 'model': None, 'vis_ones': False, 'nlst': 1, 'ntriads': 1},
    {'name': 'm30', 'nchan': 20, 'pad': 0.5, 'shape': 'rect', 'bw_eff': [6.0], 'freq_center': [9.0], 'apply_flags': True,
     'resample': False, 'model': None, 'vis_ones': False, 'nlst': 5, 'ntriads': 1},
    {'name': 'm134', 'nchan': 67, 'pad': 1.0, 'shape': 'bhw', 'bw_eff': [5.0], 'freq_center': [30.0], 'apply_flags': True,
     'resample': True, 'model': None, 'vis_ones': False, 'nlst': 1, 'ntriads': 1},
    {'name': 'noflags', 'nchan': 16, 'pad': 1.0, 'shape': 'rect', 'bw_eff': [6.0], 'freq_center': [7.0], 'apply_flags': False,
     'resample': True, 'model': 'full_nan', 'vis_ones': False, 'nlst': 5, 'ntriads': 1},
]


def _ft(ref_root):
    src = os.path.join(ref_root, 'prisim', 'bispectrum_phase.py')
    ns = _namespace()
    ns['NP'].float = float
    ns.update({'MA': MA, 'copy': copy, 'RI': types.SimpleNamespace(InterferometerArray=type('InterferometerArray', (), {})),
               'OPS': types.SimpleNamespace()})
    body = textwrap.indent(textwrap.dedent(GC._lines(src, 2573, 2784)), '    ')
    exec("def FT(self, bw_eff, freq_center=None, shape=None, fftpow=None, pad=None, datapool='prelim', visscaleinfo=None, method='fft', "
         "resample=True, apply_flags=True):\n" + body, ns)
    return ns['FT']


def inputs(rng, spec):
    raw = GC.inputs(rng, nlst=max(spec['nlst'], 5), nchan=spec['nchan'])
    nt = spec['ntriads']
    raw = {k: (v if k == 'days' else (v[:spec['nlst'], :, :nt].copy() if v.ndim == 4 else v[:spec['nlst']].copy())) for k, v in raw.items()}
    if spec['nlst'] == 1:
        raw['flags'][0, 4, 0, :] = True               # day 4 is a day bin of its own among four
    else:
        raw['flags'][3:5, 0:3, 0, :] = True           # the second LST bin, the first of two day bins
    return raw


def binning(spec):
    if spec['nlst'] == 1:
        return {'ndaybins': 4}, {'ndaybins': 4}
    return {'ndaybins': 2, 'lstbinsize': 1008.0}, {'ndaybins': 4, 'lstbinsize': 1008.0}


def fill_under_masks(cpinfo):
    """this package's values under the masks of what FT transforms"""
    proc, err = cpinfo['processed'], cpinfo['errinfo']

    def fill(x, value):
        x = MA.array(x)
        return MA.array(NP.where(MA.getmaskarray(x), value, MA.getdata(x)), mask=MA.getmaskarray(x))

    pre = proc['prelim']
    assert NP.all(MA.getdata(pre['wts'])[MA.getmaskarray(pre['wts'])] == 0.0)
    for s in pre['eicp']:
        pre['eicp'][s] = fill(pre['eicp'][s], 1.0 + 0.0j)
    if 'submodel' in proc:
        proc['submodel']['eicp'] = fill(proc['submodel']['eicp'], 0.0)
        for s in proc['residual']['eicp']:
            proc['residual']['eicp'][s] = fill(proc['residual']['eicp'][s], 0.0)
    for q in err['eicp_diff']:
        for s in err['eicp_diff'][q]:
            err['eicp_diff'][q][s] = fill(err['eicp_diff'][q][s], 0.0)


def _put(out, key, v):
    if isinstance(v, MA.MaskedArray):
        out[key] = NP.asarray(MA.getdata(v))
        out[key + '__mask'] = MA.getmaskarray(v)
    else:
        out[key] = NP.asarray(v)


def main(ref_root):
    FT = _ft(ref_root)
    ssd, subtract = GD._functions(ref_root)
    smooth = GC._function(ref_root)
    rng = NP.random.default_rng(20261019)
    out = {'cases': NP.array(json.dumps(CASES))}
    for spec in CASES:
        name, nchan = spec['name'], spec['nchan']
        f = 150e6 + DF * NP.arange(nchan)
        raw = inputs(rng, spec)
        kw_smooth, kw_ssd = binning(spec)
        cp = GD.standin(raw)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            smooth(cp, **kw_smooth)
            shape = cp.cpinfo['processed']['prelim']['cphase']['median'].shape
            if spec['model'] == 'triadchan':
                subtract(cp, 0.5 * rng.standard_normal(shape[2:]))
            elif spec['model'] == 'full_nan':
                model = 0.5 * rng.standard_normal(shape)
                model[-1, -1, 0, 3] = NP.nan
                subtract(cp, model)
            ssd(cp, **kw_ssd)
        fill_under_masks(cp.cpinfo)
        vis = NP.ones((3, 1, nchan), dtype=NP.complex128) if spec['vis_ones'] else \
            rng.uniform(0.5, 3.0, (3, 1, nchan)) * NP.exp(2j * NP.pi * rng.uniform(size=(3, 1, nchan)))
        vis_lst = NP.asarray([23.9])
        self = types.SimpleNamespace(cPhase=cp, f=f, df=DF, cPhaseDS=None, cPhaseDS_resampled=None)
        bw_eff, fc = NP.asarray(spec['bw_eff']) * DF, f[0] + NP.asarray(spec['freq_center']) * DF
        with warnings.catch_warnings(), NP.errstate(all='ignore'):
            warnings.simplefilter('ignore')
            res = FT(self, bw_eff.copy(), freq_center=fc.copy(), shape=spec['shape'], fftpow=None, pad=spec['pad'],
                     visscaleinfo={'vis': vis.copy(), 'lst': vis_lst.copy()}, resample=spec['resample'], apply_flags=spec['apply_flags'])
        results = {'o': self.cPhaseDS}
        if spec['resample']:
            assert res is self.cPhaseDS_resampled
            results['r'] = res
        else:
            assert res is self.cPhaseDS and self.cPhaseDS_resampled is None

        pre = name + '_'
        for k, v in raw.items():
            out[pre + 'in_' + k] = v
        out[pre + 'f'] = f
        out[pre + 'vis'], out[pre + 'vis_lst'] = vis, vis_lst
        proc, err = cp.cpinfo['processed'], cp.cpinfo['errinfo']
        _put(out, pre + 'cp_prelim_wts', proc['prelim']['wts'])
        _put(out, pre + 'cp_prelim_lstbins', proc['prelim']['lstbins'])
        for s in ('mean', 'median'):
            _put(out, pre + 'cp_prelim_eicp_' + s, proc['prelim']['eicp'][s])
        if 'submodel' in proc:
            _put(out, pre + 'cp_submodel_eicp', proc['submodel']['eicp'])
            for s in ('mean', 'median'):
                _put(out, pre + 'cp_residual_eicp_' + s, proc['residual']['eicp'][s])
        for q in ('0', '1'):
            _put(out, pre + 'cp_errinfo_wts_' + q, err['wts'][q])
            for s in ('mean', 'median'):
                _put(out, pre + 'cp_errinfo_eicp_diff_%s_%s' % (q, s), err['eicp_diff'][q][s])

        # the reference's non-finite rows are exactly the rows of zero mean weight, and few
        zero = {'prelim': NP.mean(MA.getdata(proc['prelim']['wts']), axis=-1) == 0.0,
                'dspec0': NP.mean(MA.getdata(err['wts']['0']), axis=-1) == 0.0, 'dspec1': NP.mean(MA.getdata(err['wts']['1']), axis=-1) == 0.0}
        nbad = nrows = 0
        for tag, r in results.items():
            out[pre + tag + '_keys'] = NP.array(sorted(r.keys()))
            for k in ('freq_center', 'freq_wts', 'bw_eff', 'lags', 'lag_corr_length', 'lag_kernel', 'shape', 'fftpow', 'npad'):
                out[pre + tag + '_' + k] = NP.asarray(r[k])
            for p in FK.POOLS:
                x = FK.pool(r, p)
                if x is None:
                    continue
                assert not isinstance(x, MA.MaskedArray) and x.dtype == NP.complex128
                out[pre + tag + '_' + '_'.join(q for q in p if q)] = x
                bad = ~NP.all(NP.isfinite(x), axis=-1)                      # nwin x rows
                z = zero[p[1] if p[0] == 'errinfo' else 'prelim'] if spec['apply_flags'] else NP.zeros(x.shape[1:-1], dtype=bool)
                assert NP.array_equal(bad, NP.broadcast_to(z, bad.shape)), (name, tag, p)
                nbad += int(bad.sum())
                nrows += bad.size
            lk = r['lag_kernel']
            z = zero['prelim'] if spec['apply_flags'] else NP.zeros((1, 1, 1), dtype=bool)
            assert NP.array_equal(~NP.all(NP.isfinite(lk), axis=-1), NP.broadcast_to(z, lk.shape[:-1])), (name, tag, 'lag_kernel')
        assert any(z.any() for z in zero.values()), name
        share = nbad / float(nrows)
        print('%s: %d of %d rows of zero mean weight (%.1f %%)' % (name, nbad, nrows, 100 * share))
        assert spec['apply_flags'] is False or nbad > 0
        assert share <= FK.MAX_ZERO_SHARE, 'too many rows of zero mean weight: choose other inputs'
    buf = io.BytesIO()
    NP.savez_compressed(buf, **out)
    size = buf.getbuffer().nbytes
    print('golden_cpft.npz: %d bytes, %d arrays' % (size, len(out)))
    assert size < 400000, 'the fixture is too large'
    with open(os.path.join(HERE, 'golden_cpft.npz'), 'wb') as fh:
        fh.write(buf.getvalue())


if __name__ == '__main__':
    main(sys.argv[1])
