"""numpy restatement of include/prisim_cpdelay.h: the delay spectra of closure phases and their power spectra, for the CPU and GPU tests
of tests/test_cpdelay.py and tests/test_gpu_cpdelay.py.  The resampling is prisim_amd/dsp_readings.py's reading of scipy.signal.resample."""
import numpy as NP

from prisim_amd import dsp_readings as D


def delay_spectra(phases, wts, m, df, nres=None):
    """phases (..., nchan, nt), wts (nwin, nchan) -> oversampled (..., nwin, m, nt) = m df fftshift(ifft(exp(-i phi) wts, padded to m))
    along the lag axis, and (with nres) that resampled to nres lags."""
    ph = NP.asarray(phases, dtype=NP.float64)
    w = NP.asarray(wts, dtype=NP.float64).reshape(-1, ph.shape[-2])
    nchan, nt = ph.shape[-2:]
    x = NP.zeros(ph.shape[:-2] + (w.shape[0], int(m), nt), dtype=NP.complex128)
    x[..., :nchan, :] = NP.exp(-1j * ph)[..., NP.newaxis, :, :] * w[:, :, NP.newaxis]
    over = NP.fft.fftshift(NP.fft.ifft(x, axis=-2), axes=-2) * (int(m) * df)
    return over, (None if nres is None else D.resample(over, int(nres), axis=-2))


def scale_of(wts, df):
    """(nwin,) df * sum_ch wts[w][ch]: the largest modulus a spectrum of unit phasors can take (wts >= 0)."""
    return df * NP.sum(NP.abs(NP.asarray(wts, dtype=NP.float64)), axis=-1)


def spectrum_error(got, want, wts, df):
    """max |got - want| / (df sum_ch wts[w]) over everything; the window axis is -3"""
    sc = scale_of(wts, df).reshape(-1, 1, 1)
    return float(NP.max(NP.abs(NP.asarray(got) - NP.asarray(want)) / sc))


def power_individual(x, scale):
    x = NP.asarray(x)
    return NP.abs(x) ** 2 * NP.asarray(scale, dtype=NP.float64).reshape((-1,) + (1,) * (x.ndim - 2))


def power_averaged(x, scale):
    """(auto, cross) over axis 0 with scale on axis 1, axis 0 kept: mean |x|^2 scale and (scale |sum x|^2 - n0 auto) / (n0 (n0 - 1))"""
    x = NP.asarray(x)
    sc = NP.asarray(scale, dtype=NP.float64).reshape((-1,) + (1,) * (x.ndim - 2))
    n0 = x.shape[0]
    auto = NP.mean(NP.abs(x) ** 2, axis=0, keepdims=True) * sc
    cross = 1.0 / (n0 * (n0 - 1)) * (sc * NP.abs(NP.sum(x, axis=0, keepdims=True)) ** 2 - n0 * auto)
    return auto, cross


def power_bounds(x, scale):
    """The derived bounds of the averaged powers: (n0 + 8) u scale[w] (sum over axis 0 of |x|)^2 / n0 for auto and the same
    / (n0 (n0 - 1)) for cross (recursive summation of n0 terms, Higham's gamma_n, plus the products)."""
    x = NP.asarray(x)
    sc = NP.asarray(scale, dtype=NP.float64).reshape((-1,) + (1,) * (x.ndim - 2))
    n0 = x.shape[0]
    s = NP.sum(NP.abs(x), axis=0, keepdims=True) ** 2
    u = 2.0 ** -53
    return (n0 + 8) * u * sc * s / n0, (n0 + 8) * u * sc * s / (n0 * (n0 - 1))


def power_individual_exact(x, scale):
    """|x|^2 scale in extended precision (x86's 80-bit long double: 64 bits of mantissa), rounded to nothing: the value the 4 u bound
    of the individual power is derived against -- one |x|^2 (two squares and a sum: 2 u) and one product."""
    assert NP.finfo(NP.longdouble).eps <= 2.0 ** -63, 'no extended precision on this host'
    x = NP.asarray(x)
    re, im = x.real.astype(NP.longdouble), x.imag.astype(NP.longdouble)
    return (re * re + im * im) * NP.asarray(scale, dtype=NP.longdouble).reshape((-1,) + (1,) * (x.ndim - 2))


def individual_error(got, x, scale):
    """largest |got - exact| / exact in units of u = 2^-53 (points whose exact power is zero must be zero)"""
    exact = power_individual_exact(x, scale)
    got = NP.asarray(got).astype(NP.longdouble)
    nz = exact != 0
    assert NP.all(got[~nz] == 0)
    return float(NP.max(NP.abs(got[nz] - exact[nz]) / exact[nz]) / 2.0 ** -53) if nz.any() else 0.0
