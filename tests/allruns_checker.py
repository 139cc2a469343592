"""numpy restatement of include/prisim_runs.h (TEST INFRASTRUCTURE): what prisim_runs_transform and prisim_runs_power compute, in the
reference's layout, for the CPU tests and as the stand-in context's device."""
import numpy as NP

from prisim_amd import dsp_readings as D


def transform(vis, nbl, nchan, nt, bp=None, wts=None, win=None, m=None, scale=1.0, mode='all', nout=None, factor=1.0):
    """(nwin, R, nbl, nout, nt) complex128: scale fftshift(ifft(((vis bp) wts) win[w], m)) along the channel axis, then every lag,
    the linear interpolation at arange(0, m, factor) or scipy.signal.resample to nout lags."""
    m = nchan if m is None else int(m)
    x = NP.ones((1, nbl, nchan, nt), dtype=NP.complex128) if vis is None else \
        NP.asarray(vis).astype(NP.complex128).reshape((-1, nbl, nchan, nt))
    if bp is not None:
        x = x * NP.asarray(bp, dtype=NP.float64)
    if wts is not None:
        x = x * NP.asarray(wts, dtype=NP.float64)
    w = NP.ones((1, nchan)) if win is None else NP.asarray(win, dtype=NP.float64).reshape(-1, nchan)
    xw = x[NP.newaxis] * w[:, NP.newaxis, NP.newaxis, :, NP.newaxis]
    xp = NP.zeros(xw.shape[:3] + (m, nt), dtype=NP.complex128)
    xp[:, :, :, :nchan, :] = xw
    spec = NP.fft.fftshift(NP.fft.ifft(xp, axis=3), axes=3) * scale
    if mode == 'all':
        return spec
    if mode == 'interp':
        return D.downsampler(spec, factor, axis=3, method='interp')
    if mode == 'resample':
        return D.resample(spec, nout, axis=3)
    raise ValueError(mode)


def power(v1, v2, factor, cross):
    """The reference statement of compute_power_spectrum_allruns (:4188-4193) with factor one value per leading index (or one)."""
    v2 = v1 if v2 is None else v2
    f = NP.asarray(factor, dtype=NP.float64).ravel()
    f = f.reshape((-1,) + (1,) * (v1.ndim - 1)) if f.size > 1 else f.reshape((1,) * v1.ndim)
    p = (v1 * v2.conj() * f).real
    if cross:
        p *= 2
    return p


class StandinRunsContext(object):
    """runs_transform / runs_power with the device calls' contract restated in numpy; ``calls`` records the calls."""

    def __init__(self):
        self.calls = []

    def runs_transform(self, vis, nbl, nchan, nt, bp=None, wts=None, win=None, m=None, scale=1.0, mode='all', nout=None, factor=1.0,
                       route='auto', budget_bytes=None):
        self.calls.append(('transform', None if vis is None else vis.shape, mode))
        return transform(vis, nbl, nchan, nt, bp, wts, win, m, scale, mode, nout, factor), {'route': 'standin'}

    def runs_power(self, vislag1, vislag2=None, factor=1.0, cross=False, budget_bytes=None):
        self.calls.append(('power', vislag1.shape, cross))
        return power(vislag1, vislag2, factor, cross), {'route': 'standin'}
