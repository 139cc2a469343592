"""Readings of the astroutils functions that prisim/delay_spectrum.py:subband_delay_transform (:2073-2250) calls and that have no
source and no fixtures here: ``DSP.windowing`` / ``DSP.window_fftpow``, ``DSP.window_N2width``, ``LKP.find_1NN`` and
``DSP.downsampler``; ``OPS.array_trace``, which the closure-phase power spectra of prisim/bispectrum_phase.py (:3542) collapse their
covariances with; and ``NMO.find_list_in_list``, which the gain tables of prisim/interferometry.py (read_gaintable, extract_gains,
GainInfo) use to match axis names and antenna / baseline labels.  Each function below is ONE explicit reading of its name -- PARITY UNPINNED against astroutils --
pinned by known answers in tests/test_subband.py (array_trace: tests/test_cpxps.py), and the only place the reading lives: the host chain, the device call and the
fixtures' stand-in modules all use these functions.

No scipy: ``downsampler(..., method='FFT')`` restates ``scipy.signal.resample`` in numpy (checked against scipy where it is installed).
"""
import numpy as NP

# generalised cosine coefficients a_k of the symmetric windows (sum_k (-1)^k a_k cos(2 pi k n / (L - 1)))
WINDOW_COEFFS = {
    'rect': (1.0,),
    'bhw': (0.35875, 0.48829, 0.14128, 0.01168),            # 4-term Blackman-Harris
    'bnw': (0.3635819, 0.4891775, 0.1365995, 0.0106411),    # Blackman-Nuttall
}


def _shape_key(shape):
    key = str(shape).lower()
    if key not in WINDOW_COEFFS:
        raise ValueError('Invalid value for window shape specified.')
    return key


def _cosine_window(L, a):
    if L == 1:
        return NP.ones(1)
    n = NP.arange(L, dtype=NP.float64)
    w = NP.zeros(L)
    for k, ak in enumerate(a):
        w += (-1) ** k * ak * NP.cos(2 * NP.pi * k * n / (L - 1))
    return w


def windowing(N, shape='rect', centering=True, peak=None, area_normalize=False, power_normalize=True):
    """READING of DSP.windowing: an N-point window whose peak sits at index int(N/2), the index subband_delay_transform's
    window_chans (:2168) puts on the centre channel.
      rect: ones;  bhw / bnw: the symmetric generalised cosine of WINDOW_COEFFS over L points.
      Odd N: L = N.  Even N: one zero followed by the (N - 1)-point symmetric window.
    Scaling: peak (not None) -> max = peak; else area_normalize -> sum = 1; else power_normalize -> sum w^2 = 1."""
    N = int(N)
    if N < 1:
        raise ValueError('window length must be positive')
    key = _shape_key(shape)
    a = WINDOW_COEFFS[key]
    if key == 'rect':
        w = NP.ones(N)
    elif N % 2 == 1:
        w = _cosine_window(N, a)
    else:
        w = NP.concatenate(([0.0], _cosine_window(N - 1, a))) if N > 1 else NP.zeros(1)
    if peak is not None:
        w = w * (peak / NP.abs(w).max())
    elif area_normalize:
        w = w / NP.sum(w)
    elif power_normalize:
        w = w / NP.sqrt(NP.sum(w ** 2))
    return w


def _unread_fftpow(name, fftpow):
    if float(fftpow) != 1.0:
        raise NotImplementedError('DSP.%s with fftpow = %r has no reading here (only fftpow = 1.0, where it equals DSP.windowing)'
                                  % (name, fftpow))


def window_fftpow(N, shape='rect', fftpow=1.0, centering=True, peak=None, area_normalize=False, power_normalize=True):
    """READING of DSP.window_fftpow: at fftpow = 1 the window whose FFT is raised to the first power is the window itself, so this is
    ``windowing`` (the reference's commented-out alternative at :2167 calls that instead).  Any other fftpow raises
    NotImplementedError (a departure: no reading of the general case)."""
    _unread_fftpow('window_fftpow', fftpow)
    return windowing(N, shape=shape, centering=centering, peak=peak, area_normalize=area_normalize, power_normalize=power_normalize)


def window_N2width(n_window=None, shape='rect', fftpow=1, area_normalize=False, power_normalize=True):
    """READING of DSP.window_N2width: the large-N power width of the peak-normalised window, mean(w^2) = a0^2 + (a1^2 + a2^2 + a3^2) / 2
    (1 for rect, 0.2579634 for bhw, 0.2612254 for bnw).  So sqrt(frac_width n_window) * windowing(n_window) (:2166) has peak ~ 1 and
    sum w^2 = frac_width n_window, i.e. sum w^2 df ~ bw_eff.  fftpow other than 1 raises NotImplementedError."""
    _unread_fftpow('window_N2width', fftpow)
    a = NP.asarray(WINDOW_COEFFS[_shape_key(shape)])
    return float(a[0] ** 2 + NP.sum(a[1:] ** 2) / 2.0)


def find_1NN(ref, query, distance_ULIM=NP.inf, remove_oob=True):
    """READING of LKP.find_1NN for 1-D points: the nearest reference point of every query point (a point exactly halfway between two
    reference points goes to the LOWER index), kept where the distance is <= distance_ULIM (out-of-band points dropped when
    remove_oob).  Returns (indices into query, indices into ref, distances), in query order."""
    r = NP.asarray(ref, dtype=NP.float64).reshape(-1)
    q = NP.asarray(query, dtype=NP.float64).reshape(-1)
    d = NP.abs(q[:, NP.newaxis] - r[NP.newaxis, :])
    nn = NP.argmin(d, axis=1)                       # first minimum: the lower index on a tie
    dist = d[NP.arange(q.size), nn]
    keep = NP.arange(q.size) if not remove_oob else NP.where(dist <= distance_ULIM)[0]
    return keep, nn[keep], dist[keep]


def resample_map(nx, num):
    """scipy.signal.resample's spectrum selection for complex input of length nx resampled to num samples: entries (k_out, k_in, weight)
    with Y[k_out] = sum weight X[k_in] over the entries (the low bins, the high bins, the Nyquist bin split or joined); then
    y = ifft(Y) * num / nx."""
    nx, num = int(nx), int(num)
    N = min(num, nx)
    nyq = N // 2 + 1
    ent = {}
    for k in range(min(nyq, N)):
        ent[k] = [(k, 1.0)]
    if N > 2:
        for j in range(nyq - N, 0):
            ent[num + j] = [(nx + j, 1.0)]
    if N % 2 == 0:
        if num < nx and N > 2:          # (scipy's slice(-N//2, -N//2 + 1) is empty at N = 2)
            ent.setdefault(num - N // 2, []).append((nx - N // 2, 1.0))
        elif nx < num:
            half = [(k, w * 0.5) for k, w in ent[N // 2]]
            ent[N // 2] = half
            ent[num - N // 2] = list(half)
    out = [(ko, ki, w) for ko in sorted(ent) for ki, w in ent[ko]]
    return (NP.array([e[0] for e in out], dtype=NP.int64), NP.array([e[1] for e in out], dtype=NP.int64),
            NP.array([e[2] for e in out], dtype=NP.float64))


def resample(x, num, axis=-1):
    """numpy restatement of scipy.signal.resample(x, num, axis) for complex (or real, returned real) x."""
    x = NP.asarray(x)
    real = not NP.iscomplexobj(x)
    xs = NP.moveaxis(x, axis, -1)
    nx = xs.shape[-1]
    X = NP.fft.fft(xs, axis=-1)
    ko, ki, w = resample_map(nx, num)
    Y = NP.zeros(xs.shape[:-1] + (int(num),), dtype=NP.complex128)
    for k_out, k_in, wt in zip(ko, ki, w):
        Y[..., k_out] += wt * X[..., k_in]
    y = NP.fft.ifft(Y, axis=-1) * (float(num) / float(nx))
    y = NP.moveaxis(y, -1, axis)
    return y.real if real else y


def downsampler(x, factor, axis=-1, method='FFT', kind='linear'):
    """READING of DSP.downsampler.
      method 'FFT':    scipy.signal.resample(x, round(N / factor), axis) (``resample`` above).
      method 'interp': linear interpolation of x at arange(0, N, factor) (every factor-th sample for an integer factor), the reading
                       oracle/delay_oracle.py uses for delay_transform: ceil(N / factor) samples.
    Finding: for a zero-padded transform fftshift(ifft(x_pad)) M df, the FFT of that lag series is M df e^{-2 pi i k floor(M/2) / M}
    x_pad[k]; 'FFT' keeps its lowest and highest ~num/2 bins only, so a sub-band centred away from channel 0 resamples to ~0."""
    x = NP.asarray(x)
    n = x.shape[axis]
    if method == 'FFT':
        return resample(x, fft_downsample_length(n, factor), axis=axis)
    if method == 'interp':
        if kind != 'linear':
            raise NotImplementedError('DSP.downsampler(method="interp") is read for kind="linear" only')
        pos = NP.arange(0, n, factor, dtype=NP.float64)
        i0 = NP.floor(pos).astype(int)
        frac = pos - i0
        i0 = NP.minimum(i0, n - 1)
        i1 = NP.minimum(i0 + 1, n - 1)
        x0 = NP.take(x, i0, axis=axis)
        x1 = NP.take(x, i1, axis=axis)
        shp = [1] * x.ndim
        shp[axis] = -1
        return x0 + frac.reshape(shp) * (x1 - x0)
    raise ValueError('Invalid method for downsampling')


def spectral_axis(length, delx=1.0, shift=False, use_real=False):
    """DSP.spectral_axis (:2188): fftfreq(length, delx), fftshifted when shift."""
    f = NP.fft.rfftfreq(length, delx) if use_real else NP.fft.fftfreq(length, delx)
    return NP.fft.fftshift(f) if shift else f


def fft_downsample_length(n, factor):
    """Samples of downsampler(x of n samples, factor, method='FFT'): round(n / factor) (Python's rounding, halves to even)."""
    return int(round(n / float(factor)))


def array_trace(inparr, offsets=None, axis1=0, axis2=1, outaxis='axis1'):
    """READING of OPS.array_trace (prisim/bispectrum_phase.py:3542): numpy.trace of `inparr` over (axis1, axis2), which must be of
    equal length n, for every diagonal offset k = -(n-1) .. n-1 (or those of `offsets`); a[i, i + k] is summed in increasing i and NaN
    propagates.  Returns (traces, offsets, diagwts): the traces as the one axis that replaces the two, at the place of axis1 (`outaxis`
    'axis1') or of axis2 ('axis2'); the offsets; and diagwts = n - |k|, the number of elements of every diagonal.  The caller divides."""
    inparr = NP.asarray(inparr)
    axis1, axis2 = axis1 % inparr.ndim, axis2 % inparr.ndim
    if axis1 == axis2 or inparr.shape[axis1] != inparr.shape[axis2]:
        raise ValueError('array_trace needs two different axes of equal length')
    if outaxis not in ('axis1', 'axis2'):
        raise ValueError('outaxis must be "axis1" or "axis2"')
    n = inparr.shape[axis1]
    offsets = NP.arange(-(n - 1), n) if offsets is None else NP.asarray(offsets, dtype=int).reshape(-1)
    if NP.any(NP.abs(offsets) >= n):
        raise ValueError('array_trace: an offset lies outside the array')
    traces = [NP.trace(inparr, offset=int(k), axis1=axis1, axis2=axis2) for k in offsets]
    keep = axis1 if outaxis == 'axis1' else axis2
    gone = axis2 if outaxis == 'axis1' else axis1
    return NP.stack(traces, axis=keep - (1 if gone < keep else 0)), offsets, n - NP.abs(offsets)


def _key(x):
    """Hashable form of one element: structured records and array rows become tuples, bytes become str."""
    if isinstance(x, NP.void) or isinstance(x, (tuple, list, NP.ndarray)):
        return tuple(_key(v) for v in (x.tolist() if isinstance(x, (NP.void, NP.ndarray)) else x))
    if isinstance(x, bytes):
        return x.decode()
    if isinstance(x, NP.generic):
        return x.item()
    return x


def find_list_in_list(reference_array, inp):
    """READING of NMO.find_list_in_list: for every element of `inp` (the rows of a structured array, the items of a list) the index of
    its FIRST equal element in `reference_array`.  Returns a masked int64 array of inp's length; the mask marks the elements that are
    not in the reference (their data is -1).  Strings and bytes compare by text; records compare field by field."""
    if not isinstance(reference_array, (list, tuple, NP.ndarray)):
        raise TypeError('reference_array must be a list or numpy array')
    if not isinstance(inp, (list, tuple, NP.ndarray)):
        raise TypeError('inp must be a list or numpy array')
    first = {}
    for i, x in enumerate(reference_array):
        first.setdefault(_key(x), i)
    ind = NP.asarray([first.get(_key(x), -1) for x in inp], dtype=NP.int64).reshape(-1)
    return NP.ma.masked_array(ind, mask=ind < 0)
