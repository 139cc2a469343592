"""Regenerate tests/golden/golden_subband.npz from the reference's own sub-band statements.

At generation time this reads DelaySpectrum.subband_delay_transform's body (prisim/delay_spectrum.py:2073-2242) from a PRISim checkout and
executes it on a stand-in ``self`` with seeded inputs, with stand-in DSP / LKP modules built from prisim_amd/dsp_readings.py (FT1D read as
fftshift(ifft(.))).  That pins the reference's structure -- window placement, sorting, truncation, padding, products, resampling -- not
the readings themselves.  No reference text is stored: only inputs and outputs.

    python tests/golden/make_golden_subband.py /path/to/PRISim
"""
import json
import os
import sys
import textwrap
import types

import numpy as NP

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from prisim_amd import dsp_readings as R  # noqa: E402

SPECTRA = {'sim': ('skyvis', 'vis', 'vis_noise'), 'cc': ('skyvis', 'vis', 'skyvis_res', 'vis_res', 'skyvis_net', 'vis_net')}


def _lines(path, a, b):
    with open(path) as fh:
        return ''.join(fh.readlines()[a - 1:b])


def _namespace():
    np_ns = types.SimpleNamespace(**{k: getattr(NP, k) for k in dir(NP) if not k.startswith('__')})
    np_ns.int = int                                          # NP.int / NP.float_ (removed from numpy)
    np_ns.float_ = NP.float64
    dsp = types.SimpleNamespace(window_N2width=R.window_N2width, window_fftpow=R.window_fftpow, windowing=R.windowing,
                                spectral_axis=R.spectral_axis, downsampler=R.downsampler,
                                FT1D=lambda x, ax=-1, inverse=False, use_real=False, shift=False:
                                    NP.fft.fftshift(NP.fft.ifft(x, axis=ax) if inverse else NP.fft.fft(x, axis=ax), axes=ax)
                                    if shift else (NP.fft.ifft(x, axis=ax) if inverse else NP.fft.fft(x, axis=ax)))
    lkp = types.SimpleNamespace(find_1NN=R.find_1NN)
    return {'NP': np_ns, 'DSP': dsp, 'LKP': lkp}


def _sky(rng, f, nbl, nt, amp=1.0):
    tau = rng.uniform(-4e-7, 4e-7, (nbl, 1, nt, 5))
    a = rng.uniform(0.2, 3.0, (nbl, 1, nt, 5)) * NP.exp(2j * NP.pi * rng.uniform(size=(nbl, 1, nt, 5)))
    return amp * (a * NP.exp(-2j * NP.pi * f[None, :, None, None] * tau)).sum(axis=3)


def main(ref_root):
    src = os.path.join(ref_root, 'prisim', 'delay_spectrum.py')
    ns = _namespace()
    body = textwrap.indent(textwrap.dedent(_lines(src, 2073, 2242)), '    ')
    exec('def subband(self, bw_eff, freq_center, shape, fftpow, pad, bpcorrect, action, verbose):\n' + body, ns)
    fn = ns['subband']
    rng = NP.random.default_rng(20261016)
    df = 97.65625e3
    # (nchan, nbl, nt, {key: (shape, pad, freq_center channels, bw_eff in channels)}, with cc)
    specs = [
        (32, 2, 2, {'sim': ('rect', 1.0, [16.0], [8.0]), 'cc': ('rect', 1.0, [16.0], [8.0])}, True),
        (33, 2, 2, {'sim': ('bhw', 0.5, [30.2, 3.0, 16.0], [2.6, 2.6, 2.6]), 'cc': ('bhw', 2.0, [5.0, 25.0], [3.1])}, True),
        (40, 2, 2, {'sim': ('bnw', 0.0, [20.0, 9.0], [3.0, 4.5]), 'cc': ('BNW', 0.5, [12.0], [2.0, 3.3])}, True),
        (37, 2, 2, {'sim': ('bhw', 2.0, [1.4, 35.0], [2.0]), 'cc': ('rect', 0.0, [18.0], [10.0])}, True),
        (24, 2, 3, {'sim': ('bnw', 1.0, [12.0], [3.0]), 'cc': ('rect', 1.0, [12.0], [3.0])}, False),
    ]
    out = {'n': len(specs)}
    for i, (nchan, nbl, nt, keys, with_cc) in enumerate(specs):
        f = 150e6 + df * NP.arange(nchan)
        ia = types.SimpleNamespace(skyvis_freq=_sky(rng, f, nbl, nt))
        ia.vis_noise_freq = 0.05 * (rng.standard_normal((nbl, nchan, nt)) + 1j * rng.standard_normal((nbl, nchan, nt)))
        ia.vis_freq = ia.skyvis_freq + ia.vis_noise_freq
        bp = 0.6 + 0.4 * rng.uniform(size=(nbl, nchan, nt))
        self = types.SimpleNamespace(f=f, df=df, ia=ia, bp=bp, bp_wts=NP.ones_like(bp), n_acc=nt, cc_lags=None)
        mcc = nchan + int(nchan * 1.0)
        if with_cc:
            self.cc_lags = NP.fft.fftfreq(mcc, df)
            for name in SPECTRA['cc']:
                setattr(self, 'cc_%s_freq' % name, _sky(rng, f[0] + df * NP.arange(mcc), nbl, nt, 0.3))
        bw_eff = {k: NP.asarray(v[3]) * df for k, v in keys.items()}
        fc = {k: f[0] + NP.asarray(v[2]) * df for k, v in keys.items()}
        shape = {k: v[0] for k, v in keys.items()}
        pad = {k: v[1] for k, v in keys.items()}
        params = {'nchan': nchan, 'nbl': nbl, 'nt': nt, 'df': df, 'with_cc': with_cc, 'shape': dict(shape), 'pad': dict(pad),
                  'bw_eff': {k: v.tolist() for k, v in bw_eff.items()}, 'freq_center': {k: v.tolist() for k, v in fc.items()}}
        fn(self, bw_eff, fc, shape, {'cc': 1.0, 'sim': 1.0}, pad, False, None, False)
        pre = 'c%d_' % i
        out[pre + 'params'] = NP.array(json.dumps(params))
        out[pre + 'f'] = f
        out[pre + 'bp'] = bp
        for name in ('skyvis_freq', 'vis_freq', 'vis_noise_freq'):
            out[pre + name] = getattr(ia, name)
        if with_cc:
            for name in SPECTRA['cc']:
                out[pre + 'cc_%s_freq' % name] = getattr(self, 'cc_%s_freq' % name)
        for tag, res in (('o', self.subband_delay_spectra), ('r', self.subband_delay_spectra_resampled)):
            for key, d in res.items():
                for field, v in d.items():
                    if isinstance(v, (NP.ndarray, float, int)) and not isinstance(v, bool):
                        out['%s%s_%s_%s' % (pre, tag, key, field)] = NP.asarray(v)
    NP.savez_compressed(os.path.join(HERE, 'golden_subband.npz'), **out)


if __name__ == '__main__':
    main(sys.argv[1])
