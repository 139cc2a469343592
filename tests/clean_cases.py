"""Seeded inputs of the delay CLEAN edge tests (tests/test_clean_exact.py, tests/test_gpu_delay_clean_edges.py), TEST INFRASTRUCTURE.

Tie rows: values from a small alphabet of dyadic Gaussian numbers (components in {0, +-1 .. +-4} x 2^k) with repeats, sign flips, -0.0
and runs of zeros; kernels exact in double (unit taps off lag 0 with real, imaginary and negative peaks, a three-tap kernel, two taps of
equal modulus); gain 0.5 or 0.25, so every operation of the CLEAN is exact and ties persist across iterations.  One batch is one call of
the device entry: rows of one length sharing gain, maxiter and threshold, one row per kind of box.  Their arbiter is tests/clean_exact.py.

Shifted-kernel rows: continuous random rows whose kernel is roll(ifft(window), s) * (0.6 + 0.8j), s != 0, shared or per row; their
reference is tests/clean_checker.py."""
import functools

import numpy as NP

import clean_checker as CK
import clean_exact as CE

SEED = 4117
TIE_M = (1, 2, 3, 5, 24, 63, 64, 65, 130)
BOXES = ('empty', 'lag0', 'last', 'wrap', 'alternate', 'full', 'but1', 'but2', 'but3', 'zero_box', 'zero_row')
THRESHOLD = 1.0 / 64
# (gain, maxiter, absolute threshold, one shared kernel, the kind of row scaled by 2^-12 to a peak under the absolute threshold)
VARIANTS = ((0.5, 12, False, False, None), (0.25, 12, True, False, None), (0.5, 12, False, True, None), (0.25, 1, True, True, None),
            (0.25, 12, True, False, 'but2'))
BAD_THRESHOLD = (24, 4, 1)                   # the batch with a rejected, non-zero row among good ones
# Rows drawn again (the value is the number of the draw): on the first draws their exact run met a deciding comparison between equal
# moduli of values that differ by more than signs, or a zero gap against the threshold (tests/test_clean_exact.py states the condition).
REDRAW = {'m130-v0-but1-0': 1, 'm130-v2-alternate-0': 1, 'm24-v0-alternate-2': 2, 'm24-v0-but2-3': 1, 'm24-v0-full-3': 1, 'm24-v3-but2-0': 1,
          'm24-v4-but1-0': 1,
          'm3-v0-wrap-0': 1, 'm3-v2-zero_box-0': 1, 'm63-v0-but3-0': 1, 'm64-v2-wrap-0': 2, 'm64-v3-alternate-0': 2}


def tie_kernels(m):
    """Kernels exact in double, peaks of modulus 1, 2 and 4 (normalisation divides exactly)."""
    out = []
    for lag, peak in ((0, 1.0), (3, 2j), (m - 1, -4.0), (3, -4.0), (m - 1, 2j), (0, 2j)):
        k = NP.zeros(m, dtype=complex)
        k[lag % m] = peak
        out.append(k)
    if m >= 3:
        for lag in (0, 3 % m, m - 1):
            k = NP.zeros(m, dtype=complex)
            k[lag], k[(lag - 1) % m], k[(lag + 1) % m] = 1.0, 0.5, 0.5j
            out.append(k)
    if m >= 2:
        for a, b in ((m // 2, m - 1), (0, 1)):                                     # two taps of equal modulus: the first is the peak
            k = NP.zeros(m, dtype=complex)
            k[a], k[b] = 2.0, -2.0
            out.append(k)
    return out


def _wrap(m):
    box = NP.zeros(m, dtype=NP.uint8)
    w = max(1, m // 6)
    box[:w + 1] = 1
    box[m - w:] = 1
    return box


def _tie_box(kind, m):
    if kind == 'empty':
        return NP.zeros(m, dtype=NP.uint8)
    if kind in ('lag0', 'last'):
        box = NP.zeros(m, dtype=NP.uint8)
        box[0 if kind == 'lag0' else m - 1] = 1
        return box
    if kind == 'alternate':
        return (NP.arange(m) % 2 == 0).astype(NP.uint8)
    if kind in ('full', 'but1', 'but2', 'but3'):
        box = NP.ones(m, dtype=NP.uint8)
        for i in range(0 if kind == 'full' else int(kind[-1])):
            box[(m // 2 + 7 * i) % m] = 0
        return box
    return _wrap(m)                                                                  # 'wrap', 'zero_box', 'zero_row'


def _tie_row(kind, m, rng):
    scale = 2.0 ** int(rng.integers(-2, 3))
    alphabet = (rng.integers(-4, 5, size=(int(rng.integers(2, 6)), 2)) * scale).astype(float)
    if rng.random() < 0.5:
        alphabet[1:, 0] = 0.0                                                        # real parts +-0 nearly everywhere: the median falls among them
    v = alphabet[rng.integers(alphabet.shape[0], size=m)]
    v = v * NP.where(rng.random((m, 2)) < 0.3, -1.0, 1.0)                           # sign flips; 0.0 * -1.0 is -0.0
    if m >= 5 and rng.random() < 0.5:
        start, n = int(rng.integers(m)), int(rng.integers(1, m // 3 + 1))
        v[(start + NP.arange(n)) % m] *= 0.0
    row = v[:, 0] + 1j * v[:, 1]
    if kind == 'zero_box':
        row[_wrap(m) > 0] *= 0.0
        if not NP.any(row):
            row[m // 2] = scale * complex(rng.integers(1, 5), -rng.integers(1, 5))
    if kind == 'zero_row':
        row *= 0.0
    return row


@functools.lru_cache(maxsize=None)
def tie_batch(m, variant, repeats=1):
    """One device call: {'inp', 'kern', 'kidx' (None: one kernel), 'box', 'gain', 'maxiter', 'threshold', 'absolute', 'ids'}."""
    gain, maxiter, absolute, shared, shrink = VARIANTS[variant]
    kernels = tie_kernels(m)
    rows, boxes, kidx, ids = [], [], [], []
    for rep in range(repeats):
        for ib, kind in enumerate(BOXES):
            name = 'm%d-v%d-%s-%d' % (m, variant, kind, rep)
            rng = NP.random.default_rng([SEED, m, variant, ib, rep, REDRAW.get(name, 0)])
            rows.append(_tie_row(kind, m, rng) * (2.0 ** -12 if kind == shrink else 1.0))
            boxes.append(_tie_box(kind, m))
            kidx.append((ib + 3 * variant + 5 * rep) % len(kernels))
            ids.append(name)
    if shared:
        kern = kernels[(7 if variant == 2 else 2) % len(kernels)][None]               # the three-tap kernel at lag 3; the -4 tap at lag m - 1
        kidx = None
    else:
        kern, kidx = NP.stack(kernels), NP.array(kidx, dtype=NP.int32)
    return {'inp': NP.stack(rows), 'kern': kern, 'kidx': kidx, 'box': NP.stack(boxes), 'gain': gain, 'maxiter': maxiter,
            'threshold': THRESHOLD, 'absolute': absolute, 'ids': ids}


def tie_batches():
    return [(m, v, 4 if m == 24 and v == 0 else 1) for m in TIE_M for v in range(4)] + [BAD_THRESHOLD]


@functools.lru_cache(maxsize=None)
def tie_reference(m, variant, repeats=1):
    """The exact run of a batch, computed once: cc, res, iters, flags, rms, min_gap, ties_symmetric.  Read only."""
    b = tie_batch(m, variant, repeats)
    out = CE.clean_rows(b['inp'], b['kern'], b['box'], b['gain'], b['maxiter'], b['threshold'], b['absolute'], b['kidx'])
    for a in out:
        a.setflags(write=False)
    return out


SHIFTED = ((24, 64), (37, 48), (64, 32), (65, 32), (512, 8))                         # (m, rows)
SHIFTED_MAXITER = 200
# two rows each, one shared kernel, 40 iterations: a length that keeps the shared kernel in LDS, the two lengths about the limit of a
# 160 KiB workgroup (16 m + ceil16(26 m) bytes), an odd length near the top and the top
LDS_EDGE = (2048, 3900, 3901, 4095, 4096)
LDS_EDGE_MAXITER = 40


@functools.lru_cache(maxsize=None)
def shifted_batch(m, nrows, per_row, maxiter=SHIFTED_MAXITER):
    """Lag-like rows (a few tones plus noise under a tapered window of about m / 2 channels) and kernels whose peak is complex and sits
    off lag 0."""
    rng = NP.random.default_rng([SEED, m, nrows, int(per_row)])
    nchan = m // 2 + (m % 2)
    f = NP.arange(nchan)
    nk = nrows if per_row else 1
    shift = rng.integers(1, m, size=nk) if per_row else [1 + m // 3]
    wins, kern = NP.empty((nk, nchan)), NP.empty((nk, m), dtype=complex)
    for i in range(nk):
        power = rng.uniform(0.5, 3.0) if per_row else 2.0
        while True:
            # The checker divides the kernel by numpy's abs of its peak, which is not correctly rounded everywhere (it depends on the
            # processor's vector path); the device rounds that modulus correctly.  Keep the windows on which the two agree, so that both
            # sides start from one normalised kernel whatever the machine (tests/test_clean_exact.py asserts it).
            wins[i] = NP.sin(NP.pi * (f + 0.5) / nchan) ** power
            kz = NP.zeros(m, dtype=complex)
            kz[:nchan] = wins[i]
            kern[i] = NP.roll(NP.fft.ifft(kz) * m, int(shift[i])) * (0.6 + 0.8j)
            if NP.abs(kern[i]).max() == CE.rounded_modulus(kern[i][NP.argmax(NP.abs(kern[i]))]):
                break
            power = rng.uniform(0.5, 3.0)
    x = NP.zeros((nrows, m), dtype=complex)
    for r in range(nrows):
        tau = rng.uniform(-0.15, 0.15, 5)
        amp = rng.uniform(0.2, 5.0, 5) * NP.exp(2j * NP.pi * rng.uniform(size=5))
        v = (amp[:, None] * NP.exp(-2j * NP.pi * f[None, :] * tau[:, None])).sum(axis=0)
        v += rng.uniform(0.0, 0.3) * (rng.standard_normal(nchan) + 1j * rng.standard_normal(nchan))
        x[r, :nchan] = v * wins[r if per_row else 0]
    lag = NP.fft.ifft(x, axis=1) * m
    half = rng.integers(1, max(2, m // 10), size=nrows)
    box = NP.zeros((nrows, m), dtype=NP.uint8)
    for r in range(nrows):
        box[r, :half[r] + 1] = 1
        box[r, m - half[r] - (r % 2):] = 1
    return {'inp': lag, 'kern': kern, 'kidx': NP.arange(nrows, dtype=NP.int32) if per_row else None, 'box': box, 'gain': 0.3,
            'maxiter': maxiter, 'threshold': 0.03, 'absolute': False}


@functools.lru_cache(maxsize=None)
def shifted_reference(m, nrows, per_row, maxiter=SHIFTED_MAXITER):
    """The checker's run of a shifted batch: cc, res, iters, flags, rms, margins.  Read only."""
    b = shifted_batch(m, nrows, per_row, maxiter)
    nrows = b['inp'].shape[0]
    cc, res = NP.zeros_like(b['inp']), NP.zeros_like(b['inp'])
    iters, flags, rms, margins = NP.zeros(nrows, NP.int32), NP.zeros(nrows, NP.int32), NP.full((nrows, 2), NP.nan), NP.zeros(nrows)
    for r in range(nrows):
        o = CK.clean_row(b['inp'][r], b['kern'][0 if b['kidx'] is None else b['kidx'][r]], b['box'][r], b['gain'], b['maxiter'],
                         b['threshold'])
        cc[r], res[r], iters[r], margins[r] = o['cc'], o['res'], o['iter'], o['margin']
        flags[r] = o['cond1'] * 1 | o['cond2'] * 2 | o['cond3'] * 4 | (o['outrms'] is None) * 8
        rms[r] = (o['inrms'], NP.nan if o['outrms'] is None else o['outrms'])
    out = (cc, res, iters, flags, rms, margins)
    for a in out:
        a.setflags(write=False)
    return out


DELAY_SHAPES = ((12, 18), (7, 7), (1, 1))                                            # (nchan, m)


@functools.lru_cache(maxsize=None)
def delay_case(nchan, m, ncubes=3, nrows=5):
    """Inputs of the delayClean chain entry: windowed rows (ncubes, nrows, nchan), three kernel windows, a kernel index and a box per
    row, and the scale factors of a 100 kHz channel."""
    rng = NP.random.default_rng([SEED, nchan, m, ncubes, nrows])
    f = NP.arange(nchan)
    kwin = NP.stack([(0.3 + NP.sin(NP.pi * (f + 0.5) / nchan) ** p) * NP.exp(1j * ph) for p, ph in ((1.0, 0.0), (2.0, 0.7), (0.5, -1.9))])
    kidx = NP.array([2, 0, 1, 0, 2], dtype=NP.int32)[:nrows]
    win = NP.empty((ncubes, nrows, nchan), dtype=complex)
    for c in range(ncubes):
        for r in range(nrows):
            tau = rng.uniform(-0.2, 0.2, 3)
            amp = rng.uniform(0.5, 4.0, 3) * NP.exp(2j * NP.pi * rng.uniform(size=3))
            v = (amp[:, None] * NP.exp(-2j * NP.pi * f[None, :] * tau[:, None])).sum(axis=0)
            win[c, r] = (v + 0.1 * (rng.standard_normal(nchan) + 1j * rng.standard_normal(nchan))) * NP.abs(kwin[kidx[r]])
    box = NP.zeros((nrows, m), dtype=NP.uint8)
    for r in range(nrows):
        box[r, :1 + r % max(1, m - 2)] = 1
        if r % 2 and m > 4:
            box[r, m - 1 - r // 2:] = 1
    df = 1e5
    return {'win': win, 'kwin': kwin, 'kidx': kidx, 'box': box, 'm': m, 'lag_scale': df, 'freq_scale1': 1.0 / (m * df),
            'freq_scale2': 1.0 * m / nchan, 'gain': 0.2, 'maxiter': 60, 'threshold': 5e-3}


@functools.lru_cache(maxsize=None)
def delay_reference(nchan, m, ncubes=3, nrows=5):
    """The checker's chain for delay_case: to_lag, clean_row per (cube, row) with the row's own kernel and box, fft * deta * pad_factor.
    Returns a dict of lag, kern_lag, cc, res, cc_freq, res_freq, iters, flags, rms and the smallest margin.  Read only."""
    c = delay_case(nchan, m, ncubes, nrows)

    def to_lag(x):
        xp = NP.zeros(x.shape[:-1] + (m,), dtype=complex)
        xp[..., :nchan] = x
        return NP.fft.ifft(xp, axis=-1) * m * c['lag_scale']

    out = {'lag': to_lag(c['win']), 'kern_lag': to_lag(c['kwin'])}
    for name in ('cc', 'res'):
        out[name] = NP.zeros_like(out['lag'])
    out['iters'], out['flags'] = NP.zeros((ncubes, nrows), NP.int32), NP.zeros((ncubes, nrows), NP.int32)
    out['rms'] = NP.full((ncubes, nrows, 2), NP.nan)
    margin = NP.inf
    for cube in range(ncubes):
        for r in range(nrows):
            o = CK.clean_row(out['lag'][cube, r], out['kern_lag'][c['kidx'][r]], c['box'][r], c['gain'], c['maxiter'], c['threshold'])
            out['cc'][cube, r], out['res'][cube, r], out['iters'][cube, r] = o['cc'], o['res'], o['iter']
            out['flags'][cube, r] = o['cond1'] * 1 | o['cond2'] * 2 | o['cond3'] * 4 | (o['outrms'] is None) * 8
            out['rms'][cube, r] = (o['inrms'], NP.nan if o['outrms'] is None else o['outrms'])
            margin = min(margin, o['margin'])
    out['cc_freq'] = NP.fft.fft(out['cc'], axis=-1) * c['freq_scale1'] * c['freq_scale2']
    out['res_freq'] = NP.fft.fft(out['res'], axis=-1) * c['freq_scale1'] * c['freq_scale2']
    out['margin'] = margin
    for a in out.values():
        if isinstance(a, NP.ndarray):
            a.setflags(write=False)
    return out
