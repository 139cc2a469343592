"""Numpy restatement of DelaySpectrum.subband_delay_transform (prisim/delay_spectrum.py:2147-2242), pinned to the reference's own
statements by tests/golden/golden_subband.npz (tests/test_subband.py), and the yardstick of the device tests.  The astroutils readings
(windows, nearest channel, FFT resampling) are prisim_amd/dsp_readings.py's: they are pinned by known answers, not by these fixtures."""
import numpy as NP

from prisim_amd import dsp_readings as D


def freq_wts(f, df, bw_eff, freq_center, shape):
    """(n_win, nchan) windows, rows in channel order (:2159-2177)."""
    nchan = f.size
    fw = D.window_N2width(shape=shape)
    nwin = NP.round(bw_eff / fw / df).astype(int)
    _, chans, _ = D.find_1NN(f, freq_center, distance_ULIM=0.5 * df)
    order = NP.argsort(chans)
    out = NP.zeros((bw_eff.size, nchan))
    for i, (c, n) in enumerate(zip(chans[order], nwin[order])):
        w = NP.sqrt(fw * n) * D.windowing(n, shape=shape)
        pos = c + NP.arange(n) - int(n / 2)                                     # channel of every window sample
        ok = (pos >= 0) & (pos < nchan)
        out[i, pos[ok]] = w[ok]
    return out


def transform(x, bp, wts, npad, df):
    """(nbl, n_win, nchan + npad, nt) spectra of x (nbl, nchan, nt) times bp (nbl | 1, nchan, nt | 1) times every window (:2196-2199)."""
    nchan = x.shape[1]
    xp = x[:, NP.newaxis, :, :] * bp[:, NP.newaxis, :, :] * wts[NP.newaxis, :, :, NP.newaxis]
    xp = NP.pad(xp, ((0, 0), (0, 0), (0, npad), (0, 0)), mode='constant')
    return NP.fft.fftshift(NP.fft.ifft(xp, axis=2), axes=2) * (npad + nchan) * df


def subband(f, df, cubes, bp, bw_eff, freq_center, shape, pad):
    """cubes: {'sim': {'skyvis': ..., 'vis': ..., 'vis_noise': ...}, 'cc': {...6 cubes...}} (a key absent: not transformed); bw_eff,
    freq_center: arrays per key of equal size; shape, pad per key.  Returns (result, result_resampled) as the reference's dictionaries."""
    nchan = f.size
    res, rres = {}, {}
    keys = [k for k in ('cc', 'sim') if k in cubes]
    npads = {k: int(nchan * pad[k]) for k in keys}
    bw_eff, freq_center = dict(bw_eff), dict(freq_center)
    for k in keys:                                                                 # :2117-2123
        b, c = NP.asarray(bw_eff[k]).reshape(-1), NP.asarray(freq_center[k]).reshape(-1)
        bw_eff[k], freq_center[k] = NP.broadcast_to(b, (max(b.size, c.size),)), NP.broadcast_to(c, (max(b.size, c.size),))
    for k in keys:
        w = freq_wts(f, df, bw_eff[k], freq_center[k], shape[k])
        npad, m = npads[k], nchan + npads[k]
        lags = NP.fft.fftshift(NP.fft.fftfreq(m, df))
        r = {'freq_center': freq_center[k], 'shape': shape[k], 'freq_wts': w, 'bw_eff': bw_eff[k], 'npad': npad, 'lags': lags,
             'lag_kernel': transform(NP.ones_like(bp, dtype=complex), bp, w, npad, df), 'lag_corr_length': nchan / w.sum(axis=1)}
        for name, x in cubes[k].items():
            r[name + '_lag'] = None if x is None else transform(x[:, :nchan, :], bp, w, npad, df)
        res[k] = r
        factor = NP.min((nchan + npads[keys[-1]]) * df / bw_eff[k])                 # :2225, npad of the last key
        rr = {'freq_center': freq_center[k], 'bw_eff': bw_eff[k]}
        rr['lags'] = D.downsampler(lags, factor, axis=-1, method='interp')
        rr['lag_kernel'] = D.downsampler(r['lag_kernel'], factor, axis=2, method='interp')
        for name in cubes[k]:
            x = r[name + '_lag']
            rr[name + '_lag'] = None if x is None else D.downsampler(x, factor, axis=2, method='FFT')
        rr['lag_corr_length'] = (1 / bw_eff[k]) / (rr['lags'][1] - rr['lags'][0])
        rres[k] = rr
    return res, rres


def rel_err(got, want, scale_of=None):
    """max over (row, window) of max|got - want| / max|scale_of| on that (baseline, window, snapshot); arrays (nbl, n_win, lags, nt).
    scale_of defaults to want; the resampled spectra are measured against their oversampled spectrum (a window away from channel 0
    resamples to rounding noise, whose own maximum is no scale)."""
    scale = NP.max(NP.abs(want if scale_of is None else scale_of), axis=2, keepdims=True)
    scale = NP.where(scale > 0, scale, 1.0)
    return float(NP.max(NP.abs(got - want) / scale))
