"""Regenerate tests/golden/golden_clean.npz from the reference's own delay CLEAN statements.

At generation time this reads complex1dClean (prisim/delay_spectrum.py:133-352), the box statement of delayClean (:1764) and its
post-processing (:1808-1838) from a PRISim checkout and executes them on seeded inputs (the post-processing on a stand-in ``self``).  No
reference text is stored: only inputs and outputs.

    python tests/golden/make_golden_clean.py /path/to/PRISim
"""
import os
import sys
import textwrap
import types

import numpy as NP

HERE = os.path.dirname(os.path.abspath(__file__))


def _lines(path, a, b):
    with open(path) as fh:
        return ''.join(fh.readlines()[a - 1:b])


def _namespace():
    np_ns = types.SimpleNamespace(**{k: getattr(NP, k) for k in dir(NP) if not k.startswith('__')})
    if not hasattr(NP, 'bool') or NP.bool is not bool:
        np_ns.bool = bool                                    # the reference's NP.bool (removed from numpy 1.24)
    return {'NP': np_ns}


def synth_rows(rng, nrows, nchan, pad, nsrc=6, noise=0.0):
    """Delay spectra of a few tones at delays inside +-tau_max, windowed by a Blackman-Harris-like window, FT1D reading (ifft)."""
    df = 97.65625e3
    m = nchan + int(nchan * pad)
    f = 150e6 + df * NP.arange(nchan)
    win = 0.35875 - 0.48829 * NP.cos(2 * NP.pi * NP.arange(nchan) / (nchan - 1)) + 0.14128 * NP.cos(4 * NP.pi * NP.arange(nchan) / (nchan - 1))
    rows = []
    for _ in range(nrows):
        tau = rng.uniform(-3e-7, 3e-7, nsrc)
        amp = rng.uniform(0.2, 5.0, nsrc) * NP.exp(2j * NP.pi * rng.uniform(size=nsrc))
        v = (amp[:, None] * NP.exp(-2j * NP.pi * f[None, :] * tau[:, None])).sum(axis=0)
        v = v + noise * (rng.standard_normal(nchan) + 1j * rng.standard_normal(nchan))
        x = NP.zeros(m, dtype=complex)
        x[:nchan] = v * win
        rows.append(m * df * NP.fft.ifft(x))
    k = NP.zeros(m, dtype=complex)
    k[:nchan] = win
    return NP.array(rows), m * df * NP.fft.ifft(k), NP.fft.fftfreq(m, df), df * nchan


def main(ref_root):
    src = os.path.join(ref_root, 'prisim', 'delay_spectrum.py')
    ns = _namespace()
    exec(_lines(src, 133, 352), ns)                         # def complex1dClean(...)
    clean = ns['complex1dClean']
    rng = NP.random.default_rng(20261015)
    cases = []
    # (nchan, pad, gain, maxiter, threshold, threshold_type, box half-width in lags, noise)
    specs = [(32, 1.0, 0.1, 10000, 5e-3, 'relative', 5, 0.05),        # M 64 even, box 11 in (odd), 53 out (odd)
             (31, 1.0, 0.5, 10000, 5e-3, 'relative', 4, 0.05),        # M 62 even, box 9, out 53
             (32, 0.5, 0.1, 10000, 1e-3, 'absolute', 6, 0.02),        # M 48, absolute threshold
             (33, 0.5, 0.5, 10000, 2e-2, 'absolute', 3, 0.0),         # M 49 odd, box 7 (odd), out 42 (even)
             (40, 1.0, 0.1, 7, 5e-3, 'relative', 8, 0.0),             # stops on maxiter
             (37, 1.0, 0.1, 10000, 1e-9, 'relative', 5, 0.5),         # stops on inrms <= outrms (noise-dominated)
             (36, 0.0, 0.5, 10000, 5e-3, 'relative', 6, 0.1)]         # M 36, box 12 (even), out 24 (even)
    for nchan, pad, gain, maxiter, thr, ttype, half, noise in specs:
        rows, kern, lags, bw = synth_rows(rng, 4, nchan, pad, noise=noise)
        m = rows.shape[1]
        for r in range(rows.shape[0]):
            box = NP.zeros(m, dtype=int)
            width = half + r % 2                                    # alternate even / odd counts inside the box
            box[:width + 1] = 1
            box[m - width:] = 1
            cases.append((rows[r], kern, box, gain, maxiter, thr, ttype))
    zero_m = 40
    zbox = NP.zeros(zero_m, dtype=int)
    zbox[:5] = 1
    zbox[-4:] = 1
    cases.append((NP.zeros(zero_m, dtype=complex), synth_rows(rng, 1, 20, 1.0)[1], zbox, 0.1, 10000, 5e-3, 'relative'))   # all-zero row
    out = {'n': len(cases)}
    for i, (inp, kern, box, gain, maxiter, thr, ttype) in enumerate(cases):
        o = clean(inp.copy(), kern.copy(), cbox=box.copy(), gain=gain, maxiter=maxiter, threshold=thr, threshold_type=ttype)
        out['inp_%d' % i], out['kernel_%d' % i], out['cbox_%d' % i] = inp, kern, box.astype(NP.uint8)
        out['params_%d' % i] = NP.array([gain, maxiter, thr, 1.0 if ttype == 'absolute' else 0.0])
        out['cc_%d' % i], out['res_%d' % i] = o['cc'], o['res']
        out['iter_%d' % i] = o['iter']
        out['cond_%d' % i] = NP.array([o['termination']['threshold'], o['termination']['maxiter'], o['termination']['inrms<outrms']], dtype=bool)
        out['rms_%d' % i] = NP.array([o['inrms'][-1], o['outrms'][-1]])

    # delayClean: the box (:1764, the parallel branch's fresh box per row) and the post-processing (:1808-1838) on a stand-in self
    nbl, nchan, nt, pad, buf = 3, 24, 2, 1.0, 1.0
    df = 97.65625e3
    npad = int(nchan * pad)
    m = nchan + npad
    blen = NP.array([14.6, 29.2, 50.6])
    hdl = NP.zeros((nt, nbl, 2))
    hdl[:, :, 0] = -blen / 299792458.0 - NP.array([[0.0], [3e-9]])
    hdl[:, :, 1] = blen / 299792458.0 - NP.array([[0.0], [3e-9]])
    lags = NP.fft.fftfreq(m, df)
    bw = df * nchan
    self = types.SimpleNamespace(horizon_delay_limits=hdl, f=150e6 + df * NP.arange(nchan))
    box_stmt = textwrap.dedent(_lines(src, 1764, 1764))
    boxes = NP.zeros((nt, nbl, m), dtype=NP.uint8)
    for ti in range(nt):
        for bli in range(nbl):
            env = dict(ns, self=self, lags=lags, clean_window_buffer=buf, bw=bw, ti=ti, bli=bli, clean_area=NP.zeros(m, dtype=int))
            exec(box_stmt, env)
            boxes[ti, bli] = env['clean_area']
    skyvis_lag = NP.zeros((nbl, m, nt), dtype=complex)
    vis_lag = NP.zeros((nbl, m, nt), dtype=complex)
    rows, kern, _, _ = synth_rows(rng, 2 * nbl * nt, nchan, pad, noise=0.05)
    lag_kernel = NP.repeat(NP.repeat(kern[None, :, None], nbl, axis=0), nt, axis=2)
    comps = {k: NP.zeros((nbl, m, nt), dtype=complex) for k in ('cn', 'rn', 'cy', 'ry')}
    for bli in range(nbl):
        for ti in range(nt):
            skyvis_lag[bli, :, ti] = rows[2 * (bli * nt + ti)]
            vis_lag[bli, :, ti] = rows[2 * (bli * nt + ti) + 1]
            a = clean(skyvis_lag[bli, :, ti].copy(), kern.copy(), cbox=boxes[ti, bli].astype(int), gain=0.1, maxiter=10000, threshold=5e-3)
            b = clean(vis_lag[bli, :, ti].copy(), kern.copy(), cbox=boxes[ti, bli].astype(int), gain=0.1, maxiter=10000, threshold=5e-3)
            comps['cn'][bli, :, ti], comps['rn'][bli, :, ti] = a['cc'], a['res']
            comps['cy'][bli, :, ti], comps['ry'][bli, :, ti] = b['cc'], b['res']
    post = textwrap.dedent(_lines(src, 1808, 1838))
    env = dict(ns, self=self, lags=lags, npad=npad, skyvis_lag=skyvis_lag, vis_lag=vis_lag, lag_kernel=lag_kernel,
               ccomponents_noiseless=comps['cn'], ccres_noiseless=comps['rn'], ccomponents_noisy=comps['cy'], ccres_noisy=comps['ry'],
               clean_window_buffer=buf)
    exec(post, env)
    out['dc_hdl'], out['dc_boxes'], out['dc_df'], out['dc_nchan'], out['dc_pad'] = hdl, boxes, df, nchan, pad
    out['dc_skyvis_lag_in'], out['dc_vis_lag_in'], out['dc_kernel'] = skyvis_lag, vis_lag, kern
    for name in ('lags', 'skyvis_lag', 'vis_lag', 'lag_kernel', 'cc_lag_kernel', 'cc_skyvis_lag', 'cc_skyvis_res_lag', 'cc_vis_lag',
                 'cc_vis_res_lag', 'cc_skyvis_net_lag', 'cc_vis_net_lag', 'cc_lags', 'cc_skyvis_freq', 'cc_skyvis_res_freq', 'cc_vis_freq',
                 'cc_vis_res_freq', 'cc_skyvis_net_freq', 'cc_vis_net_freq'):
        out['dc_' + name] = getattr(self, name)
    path = os.path.join(HERE, 'golden_clean.npz')
    NP.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes,', len(cases), 'rows, iterations',
          [int(out['iter_%d' % i]) for i in range(len(cases))])


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit('usage: make_golden_clean.py /path/to/PRISim')
    main(sys.argv[1])
