"""A DelaySpectrum on a stand-in array whose context computes prisim_subband_transform in numpy (tests/subband_checker.py's
statements), so that the host logic of subband_delay_transform runs without a GPU."""
import types

import numpy as NP

from prisim_amd import delay_spectrum as DS, dsp_readings as D


class StandinContext(object):
    """subband_transform with the device call's contract, restated in numpy; ``calls`` counts the calls, ``fail_after`` makes the
    n-th call raise (to test that a failed call changes nothing)."""

    def __init__(self, fail_after=None):
        self.calls = 0
        self.fail_after = fail_after
        self.shapes = []

    def subband_transform(self, cubes, bp, wts, m, df, nres=0, pscale=None, want=('over', 'res'), route='auto', **kw):
        self.calls += 1
        if self.fail_after is not None and self.calls > self.fail_after:
            raise RuntimeError('stand-in device failure')
        x = NP.asarray(cubes)                                           # (ncubes, nt, nbl, nchan)
        self.shapes.append(x.shape)
        ncubes, nt, nbl, nchan = x.shape
        b = NP.asarray(bp, dtype=NP.float64).reshape(-1, nchan)
        b = NP.broadcast_to(b, (nbl, nchan)) if b.shape[0] in (1, nbl) else b.reshape(nt, nbl, nchan)
        b = NP.broadcast_to(b, (nt, nbl, nchan))
        xp = NP.zeros((ncubes, nt, nbl, wts.shape[0], m), dtype=NP.complex128)
        xp[..., :nchan] = (x * b)[:, :, :, NP.newaxis, :] * wts[NP.newaxis, NP.newaxis, NP.newaxis]
        over = NP.fft.fftshift(NP.fft.ifft(xp, axis=-1), axes=-1) * m * df
        out = {'stats': {'device_ms': 0.0, 'kernel_ms': 0.0, 'rows': ncubes * nt * nbl, 'route': 'standin', 'lds_bytes': 0}}
        if 'over' in want:
            out['over'] = over
        if 'res' in want:
            out['res'] = D.resample(over, nres, axis=-1)
        return out


def make_ds(nchan=32, nbl=3, nt=2, noise=True, seed=0, ctx=None):
    """A DelaySpectrum over a stand-in InterferometerArray with seeded sky / noise cubes and a per-snapshot bandpass."""
    rng = NP.random.default_rng(seed)
    df = 97.65625e3
    f = 150e6 + df * NP.arange(nchan)
    ia = types.SimpleNamespace(channels=f, freq_resolution=df, n_acc=nt, baselines=rng.normal(size=(nbl, 3)) * 30.0, _stacks={},
                               _ctx=ctx if ctx is not None else StandinContext())
    ia.skyvis_freq = rng.normal(size=(nbl, nchan, nt)) + 1j * rng.normal(size=(nbl, nchan, nt))
    ia.vis_noise_freq = (0.1 * (rng.normal(size=(nbl, nchan, nt)) + 1j * rng.normal(size=(nbl, nchan, nt)))) if noise else None
    ia.vis_freq = ia.skyvis_freq + ia.vis_noise_freq if noise else None
    ia.bp = 0.6 + 0.4 * rng.uniform(size=(nbl, nchan, nt))
    ia.bp_wts = NP.ones((nbl, nchan, nt))
    ds = DS.DelaySpectrum.__new__(DS.DelaySpectrum)
    ds.ia, ds.f, ds.df, ds.n_acc = ia, f, df, nt
    ds.pad, ds.lags = 0.0, NP.fft.fftshift(NP.fft.fftfreq(nchan, df))
    ds._bp_wts_override = None
    for name in ('cc_lags', 'cc_skyvis_freq', 'cc_skyvis_res_freq', 'cc_vis_freq', 'cc_vis_res_freq', 'cc_skyvis_net_freq',
                 'cc_vis_net_freq'):
        setattr(ds, name, None)
    ds.subband_delay_spectra, ds.subband_delay_spectra_resampled = {}, {}
    return ds


def add_clean(ds, seed=1):
    """CLEAN-like cc_*_freq cubes of 2 nchan samples (delayClean's layout with pad 1) and cc_lags."""
    rng = NP.random.default_rng(seed)
    nbl, nchan, nt = ds.ia.skyvis_freq.shape
    m = 2 * nchan
    ds.cc_lags = NP.fft.fftshift(NP.fft.fftfreq(m, ds.df))
    for name in ('skyvis', 'vis'):
        cc = rng.normal(size=(nbl, m, nt)) + 1j * rng.normal(size=(nbl, m, nt))
        res = 0.1 * (rng.normal(size=(nbl, m, nt)) + 1j * rng.normal(size=(nbl, m, nt)))
        setattr(ds, 'cc_%s_freq' % name, cc)
        setattr(ds, 'cc_%s_res_freq' % name, res)
        setattr(ds, 'cc_%s_net_freq' % name, cc + res)
    return ds
