"""Regenerate tests/golden/golden_allruns.npz from the reference's own statements for stacks of runs.

At generation time this reads the bodies of DelaySpectrum.delay_transform_allruns (prisim/delay_spectrum.py:1539-1618),
DelaySpectrum.subband_delay_transform_allruns (:2393-2513) and DelayPowerSpectrum.compute_power_spectrum_allruns (:4138-4195) from a
PRISim checkout and executes them on stand-in ``self`` objects with seeded inputs, with stand-in DSP / LKP modules built from
prisim_amd/dsp_readings.py (FT1D read as fftshift(ifft(.)); DSP.downsampler's default method read as 'interp', as
DelaySpectrum.delay_transform and oracle/delay_oracle.py read it) and NP.int / NP.float_ aliases.  No reference text is stored: only
inputs, outputs and the classes of the exceptions raised.

    python tests/golden/make_golden_allruns.py /path/to/PRISim
"""
import json
import os
import sys
import textwrap
import types

import numpy as NP
import scipy.constants as FCNST

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from prisim_amd import dsp_readings as R  # noqa: E402
from prisim_amd import delay_spectrum as DS  # noqa: E402

DF = 97.65625e3
JACOBIAN1, JACOBIAN2, JY2K = 2.5e-3, 7.1e7, 3.3e-3       # the full-band scalars of the stand-in DelayPowerSpectrum


def beam3dvol_standin(freq_wts=None):
    """The stand-in DelayPowerSpectrum.beam3Dvol of the power cases (tests/test_allruns.py uses the same)."""
    return 1e-2 * NP.sum(NP.atleast_2d(NP.asarray(freq_wts, dtype=NP.float64)) ** 2, axis=-1) + 0.5


def _lines(path, a, b):
    with open(path) as fh:
        return ''.join(fh.readlines()[a - 1:b])


def _namespace():
    np_ns = types.SimpleNamespace(**{k: getattr(NP, k) for k in dir(NP) if not k.startswith('__')})
    np_ns.int = int
    np_ns.float_ = NP.float64
    dsp = types.SimpleNamespace(window_N2width=R.window_N2width, window_fftpow=R.window_fftpow, windowing=R.windowing,
                                spectral_axis=R.spectral_axis,
                                downsampler=lambda x, factor, axis=-1, method='interp', kind='linear': R.downsampler(x, factor, axis, method,
                                                                                                                     kind),
                                FT1D=lambda x, ax=-1, inverse=False, use_real=False, shift=False:
                                    NP.fft.fftshift(NP.fft.ifft(x, axis=ax) if inverse else NP.fft.fft(x, axis=ax), axes=ax)
                                    if shift else (NP.fft.ifft(x, axis=ax) if inverse else NP.fft.fft(x, axis=ax)))
    lkp = types.SimpleNamespace(find_1NN=R.find_1NN)
    cnst = types.SimpleNamespace(rest_freq_HI=DS.REST_FREQ_HI, Jy=DS.JY)
    return {'NP': np_ns, 'DSP': dsp, 'LKP': lkp, 'CNST': cnst, 'FCNST': FCNST}


def _define(ns, name, args, src, a, b):
    body = textwrap.indent(textwrap.dedent(_lines(src, a, b)), '    ')
    exec('def %s(%s):\n' % (name, args) + body, ns)
    return ns[name]


def _vis(rng, f, lead, nbl, nt):
    tau = rng.uniform(-4e-7, 4e-7, lead + (nbl, 1, nt, 4))
    a = rng.uniform(0.2, 3.0, lead + (nbl, 1, nt, 4)) * NP.exp(2j * NP.pi * rng.uniform(size=lead + (nbl, 1, nt, 4)))
    v = (a * NP.exp(-2j * NP.pi * f.reshape((-1, 1, 1)) * tau)).sum(axis=-1)
    return v + 0.05 * (rng.standard_normal(v.shape) + 1j * rng.standard_normal(v.shape))


def _self(rng, nchan, nbl, nt):
    f = 150e6 + DF * NP.arange(nchan)
    bp = 0.6 + 0.4 * rng.uniform(size=(nbl, nchan, nt))
    bp_wts = 0.5 + 0.5 * rng.uniform(size=(nbl, nchan, nt))
    return types.SimpleNamespace(f=f, df=DF, n_acc=nt, bp=bp, bp_wts=bp_wts, ia=types.SimpleNamespace(baselines=rng.normal(size=(nbl, 3))))


def _store(out, pre, d):
    for k, v in d.items():
        if isinstance(v, str):
            out[pre + k] = NP.array(v)
        elif isinstance(v, (NP.ndarray, float, int, NP.floating)) and not isinstance(v, bool):
            out[pre + k] = NP.asarray(v)


def main(ref_root):
    src = os.path.join(ref_root, 'prisim', 'delay_spectrum.py')
    ns = _namespace()
    full = _define(ns, 'full', 'self, vis, pad, freq_wts, downsample, verbose', src, 1539, 1618)
    sub = _define(ns, 'sub', 'self, vis, bw_eff, freq_center, shape, fftpow, pad, bpcorrect, action, verbose', src, 2393, 2511)
    pw = _define(ns, 'pw', 'self, dspec, subband', src, 4138, 4195)
    rng = NP.random.default_rng(20261016)
    out = {}

    # full band: (lead, nchan, nbl, nt, pad, downsample, freq_wts form)
    fspecs = [((), 32, 3, 1, 1.0, True, None), ((2,), 24, 2, 3, 0.5, True, 'f'), ((2, 2), 16, 2, 2, 0.0, True, 'ft'),
              ((3,), 20, 2, 2, 1.0, False, 'bf'), ((2,), 32, 2, 4, 0.5, False, 'bft'), ((2,), 12, 2, 2, 1.0, True, 'vis'),
              ((), 12, 2, 3, -0.3, True, 'b1f1'), ((2,), 30, 2, 2, 1.0, True, None)]
    for i, (lead, nchan, nbl, nt, pad, downsample, form) in enumerate(fspecs):
        s = _self(rng, nchan, nbl, nt)
        vis = _vis(rng, s.f, lead, nbl, nt)
        shapes = {None: None, 'f': (nchan,), 'ft': (nchan, nt), 'bf': (nbl, nchan), 'bft': (nbl, nchan, nt), 'vis': vis.shape,
                  'b1f1': (1, nchan, 1)}
        fw = None if form is None else 0.5 + 0.5 * rng.uniform(size=shapes[form])
        pre = 'f%d_' % i
        out[pre + 'params'] = NP.array(json.dumps({'lead': list(lead), 'nchan': nchan, 'nbl': nbl, 'nt': nt, 'pad': pad,
                                                   'downsample': downsample, 'form': form}))
        _store(out, pre + 'in_', {'vis': vis, 'bp': s.bp, 'bp_wts': s.bp_wts, 'f': s.f})
        if fw is not None:
            out[pre + 'in_freq_wts'] = fw
        try:
            res = full(s, vis, pad, fw, downsample, False)
        except Exception as exc:                               # noqa: BLE001 -- the class is the recorded result
            out[pre + 'raises'] = NP.array(type(exc).__name__)
            continue
        _store(out, pre + 'out_', res)
    out['nfull'] = len(fspecs)

    # sub-bands: (lead, nchan, nbl, nt, shape, pad, centre channels, bw_eff in channels, action)
    sspecs = [((), 32, 2, 1, 'rect', 1.0, [16.0], [8.0], 'return_resampled'),
              ((2,), 33, 2, 2, 'bhw', 0.5, [30.2, 3.0, 16.0], [2.6], 'return_oversampled'),
              ((2, 2), 40, 2, 2, 'bnw', 0.0, [20.0, 9.0], [3.0, 4.5], 'anything'),
              ((2,), 24, 2, 3, 'rect', 1.0, [12.0], [3.0], None)]
    for i, (lead, nchan, nbl, nt, shape, pad, fcc, bwc, action) in enumerate(sspecs):
        s = _self(rng, nchan, nbl, nt)
        vis = _vis(rng, s.f, lead, nbl, nt)
        bw_eff = NP.asarray(bwc) * DF
        fc = s.f[0] + NP.asarray(fcc) * DF
        pre = 's%d_' % i
        out[pre + 'params'] = NP.array(json.dumps({'lead': list(lead), 'nchan': nchan, 'nbl': nbl, 'nt': nt, 'shape': shape, 'pad': pad,
                                                   'action': action}))
        _store(out, pre + 'in_', {'vis': vis, 'bp': s.bp, 'bp_wts': s.bp_wts, 'f': s.f, 'bw_eff': bw_eff, 'freq_center': fc})
        try:
            res = sub(s, vis, bw_eff, fc, shape, None, pad, False, action, False)
        except Exception as exc:                               # noqa: BLE001
            out[pre + 'raises'] = NP.array(type(exc).__name__)
            continue
        _store(out, pre + 'out_', res)
    out['nsub'] = len(sspecs)

    # power: (subband, cross, complex64, shape)
    pspecs = [(False, False, False, (2, 3, 16, 2)), (False, True, False, (2, 2, 3, 16, 2)), (True, False, False, (3, 2, 3, 12, 2)),
              (True, True, False, (2, 2, 3, 12, 1)), (False, True, True, (2, 3, 16, 2)), (True, True, True, (2, 2, 3, 12, 2))]
    nchan = 24
    f = 150e6 + DF * NP.arange(nchan)
    for i, (subband, cross, c64, shp) in enumerate(pspecs):
        dt = NP.complex64 if c64 else NP.complex128
        v1 = (rng.standard_normal(shp) + 1j * rng.standard_normal(shp)).astype(dt) * dt(1e3)
        dspec = {'vislag1': v1}
        if cross:
            dspec['vislag2'] = (rng.standard_normal(shp) + 1j * rng.standard_normal(shp)).astype(dt) * dt(1e3)
        if subband:
            nwin = shp[0]
            dspec['freq_center'] = list(f[0] + DF * NP.sort(rng.uniform(4, 20, nwin)))
            dspec['bw_eff'] = NP.full(nwin, 3.0 * DF)
            dspec['freq_wts'] = rng.uniform(size=(nwin,) + (1,) * (len(shp) - 4) + (1, nchan, 1))
            dspec['lags'] = NP.fft.fftshift(NP.fft.fftfreq(shp[-2], DF))
        pre = 'p%d_' % i
        out[pre + 'params'] = NP.array(json.dumps({'subband': subband, 'cross': cross, 'c64': c64, 'shape': list(shp)}))
        _store(out, pre + 'in_', {k: NP.asarray(v) for k, v in dspec.items()})
        dps = DS.DelayPowerSpectrum.__new__(DS.DelayPowerSpectrum)
        dps.cosmo = DS.cosmo100
        dps.jacobian1, dps.jacobian2, dps.Jy2K = NP.float64(JACOBIAN1), NP.float64(JACOBIAN2), NP.float64(JY2K)
        dps.bl_length = NP.array([14.6, 25.3, 29.2])
        dps.f0 = f[nchan // 2]
        dps.wl0 = FCNST.c / dps.f0
        dps.beam3Dvol = beam3dvol_standin
        res = pw(dps, dict(dspec), subband)
        key = 'subband' if subband else 'fullband'
        out[pre + 'out_' + key] = res[key]
    out['npow'] = len(pspecs)
    out['numpy_fused'] = NP.array([DS._abi.numpy_fuses_complex_product(NP.complex128), DS._abi.numpy_fuses_complex_product(NP.complex64)])
    NP.savez_compressed(os.path.join(HERE, 'golden_allruns.npz'), **out)


if __name__ == '__main__':
    main(sys.argv[1])
