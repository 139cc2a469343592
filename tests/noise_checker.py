"""Independent statement of the thermal-noise draw, in Python integers, numpy and mpmath: Philox-4x32-10 as published (Salmon, Moraes,
Dror & Shaw 2011, "Parallel random numbers: as easy as 1, 2, 3"; the known-answer vectors of Random123's kat_vectors are in
test_noise_checker.py), two 52-bit uniforms and Box-Muller:

    counter = (f, g mod 2^32, t, g div 2^32)          f channel, g GLOBAL baseline (bl_offset + b, or bl_index[b]), t snapshot
    key     = (seed mod 2^32, seed div 2^32)          seed taken mod 2^64
    r       = Philox-4x32-10(counter, key)
    u1      = ((r0 << 20 | r1 >> 12) + 1) / 2^52      in (0, 1]
    u2      =  (r2 << 20 | r3 >> 12)      / 2^52      in [0, 1)
    value   = rms * 0.70710678118654752440 * sqrt(-2 ln u1) * (cos 2 pi u2 + i sin 2 pi u2)

A round of Philox-4x32 multiplies counter words 0 and 2 by two constants to 64 bits; the new words are (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2),
hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)), and after every round the key words grow by the Weyl constants (golden ratio and sqrt(3) - 1).  Nothing
here is taken from the package's sources.  Two evaluations of the value: `exact=True` in mpmath at 160 bits, rounded once to fp64 (a few
thousand elements); the default in numpy, with the angle reduced exactly so that the components near the zeros of sine and cosine keep
their relative accuracy (millions of elements).  FAST_SLACK is what the numpy evaluation may miss the exact one by
(test_noise_checker.py measures and holds it).  Used by the CPU and the GPU suites; never by the package."""
import numpy as NP

PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57          # the multipliers of Philox-4x32
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85          # the key increments (Weyl sequence)
MASK32 = 0xFFFFFFFF
INV_SQRT2 = '0.70710678118654752440'
U = 2.0 ** -53                                         # unit roundoff of fp64
FAST_SLACK = 8                                         # u: 2 x the largest componentwise deviation of the numpy evaluation (3.97 u)
K_CEILING = 32                                         # u: what the device may never need (one log, sqrt, sincospi and three products)


# ---- Philox-4x32 ---------------------------------------------------------------------------------------------------------------
def philox4x32_int(counter4, key2, rounds=10, mult=(PHILOX_M0, PHILOX_M1), weyl=(PHILOX_W0, PHILOX_W1)):
    """Scalar form on Python integers.  rounds / mult / weyl are for the mutants of test_noise_checker.py only."""
    c0, c1, c2, c3 = (int(c) & MASK32 for c in counter4)
    k0, k1 = (int(k) & MASK32 for k in key2)
    for _ in range(rounds):
        p0, p1 = mult[0] * c0, mult[1] * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK32, (p0 >> 32) ^ c3 ^ k1, p0 & MASK32
        k0, k1 = (k0 + weyl[0]) & MASK32, (k1 + weyl[1]) & MASK32
    return c0, c1, c2, c3


def philox4x32_np(counter4, key2, rounds=10, mult=(PHILOX_M0, PHILOX_M1), weyl=(PHILOX_W0, PHILOX_W1)):
    """Vectorised form: the six words are (broadcastable) arrays; they are held as uint64 masked to 32 bits, so that the 32 x 32 bit
    products are exact.  Returns four uint64 arrays of the broadcast shape."""
    m32 = NP.uint64(MASK32)
    s32 = NP.uint64(32)
    words = NP.broadcast_arrays(*[NP.asarray(w, dtype=NP.uint64) & m32 for w in tuple(counter4) + tuple(key2)])
    c0, c1, c2, c3, k0, k1 = (NP.array(w, dtype=NP.uint64) for w in words)
    m0, m1, w0, w1 = NP.uint64(mult[0]), NP.uint64(mult[1]), NP.uint64(weyl[0]), NP.uint64(weyl[1])
    for _ in range(rounds):
        p0, p1 = m0 * c0, m1 * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & m32, (p0 >> s32) ^ c3 ^ k1, p0 & m32
        k0, k1 = (k0 + w0) & m32, (k1 + w1) & m32
    return c0, c1, c2, c3


def philox4x32_10(counter4, key2):
    """Philox-4x32-10 of four counter words under two key words: Python integers in, four integers out; arrays in, four uint64 arrays."""
    if all(isinstance(w, int) for w in tuple(counter4) + tuple(key2)):
        return philox4x32_int(counter4, key2)
    return philox4x32_np(counter4, key2)


# ---- the uniforms ---------------------------------------------------------------------------------------------------------------
def uniforms(r, shift=12, plus=1):
    """(u1, u2) of four random words, as fp64 -- both are multiples of 2^-52 in [0, 1] and therefore exact.  shift / plus: mutants only."""
    if all(isinstance(w, int) for w in r):
        return (((r[0] << 20) | (r[1] >> shift)) + plus) / 2.0 ** 52, ((r[2] << 20) | (r[3] >> shift)) / 2.0 ** 52
    r0, r1, r2, r3 = (NP.asarray(w, dtype=NP.uint64) for w in r)
    m1 = ((r0 << NP.uint64(20)) | (r1 >> NP.uint64(shift))) + NP.uint64(plus)
    m2 = (r2 << NP.uint64(20)) | (r3 >> NP.uint64(shift))
    return m1.astype(NP.float64) / 2.0 ** 52, m2.astype(NP.float64) / 2.0 ** 52       # < 2^53: the conversions are exact


def counter_key(f, g, t, seed):
    """The counter and key words of (channel f, global baseline g, snapshot t) under `seed`; Python integers or integer arrays."""
    if all(isinstance(w, int) for w in (f, g, t)):
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        return (f & MASK32, g & MASK32, t & MASK32, (g >> 32) & MASK32), (seed & MASK32, seed >> 32)
    f, g, t = (NP.asarray(w, dtype=NP.uint64) for w in (f, g, t))
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return (f, g & NP.uint64(MASK32), t, g >> NP.uint64(32)), (NP.uint64(seed & MASK32), NP.uint64(seed >> 32))


# ---- Box-Muller -----------------------------------------------------------------------------------------------------------------
def box_muller_exact(u1, u2, rms, bits=160):
    """rms * 0.7071... * sqrt(-2 ln u1) * (cospi(2 u2) + i sinpi(2 u2)) in mpmath at `bits` bits, each component rounded once to fp64.
    2 u2 is exact in fp64 and mpmath's cospi / sinpi reduce it exactly.  Returns (values complex128, rad fp64) of u1's shape."""
    import mpmath
    u1, u2, rms = NP.broadcast_arrays(NP.asarray(u1, dtype=NP.float64), NP.asarray(u2, dtype=NP.float64), NP.asarray(rms, dtype=NP.float64))
    out = NP.empty(u1.shape, dtype=NP.complex128)
    rad = NP.empty(u1.shape, dtype=NP.float64)
    with mpmath.workprec(bits):
        c = mpmath.mpf(INV_SQRT2)
        for i in NP.ndindex(u1.shape):
            r = mpmath.sqrt(-2 * mpmath.log(mpmath.mpf(float(u1[i]))))
            x = 2 * mpmath.mpf(float(u2[i]))
            a = mpmath.mpf(float(rms[i])) * c * r
            out[i] = complex(float(a * mpmath.cospi(x)), float(a * mpmath.sinpi(x)))
            rad[i] = float(r)
    return out, rad


def box_muller_fast(u1, u2, rms):
    """The same in numpy.  u2 = q / 4 + s with q the nearest quarter turn and |s| <= 1/8, both exact (u2 and q / 4 are multiples of
    2^-52 below 2), so cos and sin are taken of 2 pi s in [-pi/4, pi/4] -- near a zero of a component that is sin(pi * small), which
    keeps its relative accuracy -- and turned by q quarter turns exactly.  Returns (values complex128, rad fp64)."""
    u1, u2, rms = NP.broadcast_arrays(NP.asarray(u1, dtype=NP.float64), NP.asarray(u2, dtype=NP.float64), NP.asarray(rms, dtype=NP.float64))
    rad = NP.sqrt(-2.0 * NP.log(u1))
    q = NP.rint(4.0 * u2)
    small = 2.0 * (u2 - 0.25 * q)                                                     # in [-1/4, 1/4] half turns, exact
    c, s = NP.cos(NP.pi * small), NP.sin(NP.pi * small)
    q = q.astype(NP.int64) & 3
    cs = NP.choose(q, (c, -s, -c, s))
    sn = NP.choose(q, (s, c, -s, -c))
    a = (rms * float(INV_SQRT2)) * rad
    out = NP.empty(u1.shape, dtype=NP.complex128)
    out.real, out.imag = a * cs, a * sn
    return out, rad


def draw(f, g, t, seed, rms, exact=False):
    """The noise of (channel f, global baseline g, snapshot t) under `seed`, scalars or broadcastable arrays."""
    scalar = all(isinstance(w, int) for w in (f, g, t))
    u1, u2 = uniforms(philox4x32_10(*counter_key(f, g, t, seed)))
    val = (box_muller_exact if exact else box_muller_fast)(u1, u2, rms)[0]
    return complex(val) if scalar and NP.ndim(rms) == 0 else val


def indices(shape, bl_offset, bl_index):
    nt, nbl, nchan = shape
    if bl_index is None:
        g = NP.array([int(bl_offset) + b for b in range(nbl)], dtype=NP.uint64)
    else:
        g = NP.array([int(b) for b in NP.asarray(bl_index).ravel()], dtype=NP.uint64)
        if g.size != nbl:
            raise ValueError('bl_index must have one entry per baseline')
    return (NP.arange(nchan, dtype=NP.uint64)[NP.newaxis, NP.newaxis, :], g[NP.newaxis, :, NP.newaxis],
            NP.arange(nt, dtype=NP.uint64)[:, NP.newaxis, NP.newaxis])


def reference(rms, seed, bl_offset=0, bl_index=None, exact=False):
    """(noise (nt, nbl, nchan) complex128, the scale rms * rad / sqrt(2) of every element) for rms (nt, nbl, nchan)."""
    rms = NP.asarray(rms, dtype=NP.float64)
    if rms.ndim != 3:
        raise ValueError('rms must have shape (nt, nbl, nchan)')
    f, g, t = indices(rms.shape, bl_offset, bl_index)
    u1, u2 = uniforms(philox4x32_np(*counter_key(f, g, t, seed)))
    val, rad = (box_muller_exact if exact else box_muller_fast)(u1, u2, rms)
    return val, rms * rad * float(INV_SQRT2)


def noise(rms, seed, bl_offset=0, bl_index=None, exact=False):
    """Context.noise restated: complex noise (nt, nbl, nchan) for per-element rms of that shape."""
    return reference(rms, seed, bl_offset=bl_offset, bl_index=bl_index, exact=exact)[0]


# ---- the comparison that the GPU tests call -------------------------------------------------------------------------------------
def _parts(z):
    z = NP.asarray(z, dtype=NP.complex128)
    return NP.stack((z.real, z.imag), axis=-1)


def deviation(got, ref, scale=None):
    """The largest deviation of got from ref in units of u = 2^-53: componentwise, relative to |ref| of that component (scale None) or
    to the element's scale.  Where the yardstick is 0 the two must be equal; otherwise the deviation is infinite.  NaN counts as infinite."""
    g, r = _parts(got), _parts(ref)
    if g.shape != r.shape:
        raise AssertionError('shape {0} against the reference\'s {1}'.format(g.shape[:-1], r.shape[:-1]))
    y = NP.abs(r) if scale is None else NP.repeat(NP.asarray(scale, dtype=NP.float64)[..., NP.newaxis], 2, axis=-1)
    d = NP.abs(g - r)
    with NP.errstate(divide='ignore', invalid='ignore'):
        rel = NP.where(y > 0.0, d / y, NP.where(d == 0.0, 0.0, NP.inf))
    rel = NP.where(NP.isfinite(g) & ~NP.isnan(rel), rel, NP.inf)
    return float(rel.max() / U) if rel.size else 0.0


def assert_matches(got, rms, seed, bl_offset=0, bl_index=None, K=K_CEILING, exact=True, ref=None):
    """Hold `got` (nt, nbl, nchan) to the statement above.  exact: against the mpmath reference, every component within K u of its own
    magnitude, and exactly 0 where rms is 0.  Otherwise against the numpy reference, every component within (K + FAST_SLACK) u of the
    element's rms * rad / sqrt(2).  `ref`: reference(...) of the same arguments if the caller has it already.  Returns the deviation in u."""
    val, scale = reference(rms, seed, bl_offset=bl_offset, bl_index=bl_index, exact=exact) if ref is None else ref
    dev = deviation(got, val, None if exact else scale)
    bound = K if exact else K + FAST_SLACK
    if not dev <= bound:
        raise AssertionError('noise deviates from the {0} reference by {1:.3g} u, allowed {2} u (seed {3:#x})'.format(
            'exact' if exact else 'numpy', dev, bound, int(seed) & 0xFFFFFFFFFFFFFFFF))
    return dev


# ---- the cases that the CPU and the GPU suites share ----------------------------------------------------------------------------
SEEDS = (0, 1, 1 << 32, 0xa4093822299f31d0, 2 ** 64 - 1)
SMALL_SHAPE = (3, 7, 37)                                # snapshots, baselines, channels
HIGH_OFFSETS = (2 ** 32 - 3, 2 ** 40 + 3)               # 7 baselines from the first cross 2^32


def small_rms():
    """rms of the small exact case: uniform in [0.5, 2] with one exact 0 and one 1e300."""
    rms = NP.random.default_rng(20261020).uniform(0.5, 2.0, SMALL_SHAPE)
    rms[1, 3, 11] = 0.0
    rms[2, 6, 36] = 1e300
    return rms
