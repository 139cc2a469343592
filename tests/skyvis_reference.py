"""40-digit reference of the per-baseline sky-sum and its baseline gradient (TEST INFRASTRUCTURE).

What prisim_amd/csrc/skyvis_kernels.hip states in its header, for baseline b, channel f and the sources s:
    V[b][f]   = sum_s pbflux[s][f] w[s][b][f] exp(-2 pi i phase[s][b][f]),      G[k][b][f] = sum_s s_k (the same term)
    phase     = f (tau - b.s_pc / c) = f b.(s - s_pc) / c   cycles,             tau = b.s / c
    w         = exp(-kappa_s max(|b|^2 - (c tau)^2, 0) f^2 / c^2),              kappa_s = ln 2 (2 sin(fwhm_s / 2))^2  (fwhm_s > 0; else w = 1)
The clamp at 0 is the project's known difference from the upstream code (head of oracle/skyvis_oracle.c): doubles that are not exactly
unit vectors can make the exact expression negative.  This module shares no code with oracle/ or prisim_amd.  Baselines, frequencies,
directions, the phase centre, fluxes and source sizes are taken exactly as the doubles they are; c = 299792458 and pi are exact.

Two routes.
  * reference_mp: every term in mpmath at 40 digits, summed there.  About 0.2 ms per term: a sub-sample only.
  * reference: the route the tests use (a case of 1e5 terms in about a second).  Every double is an integer times a power of two and c
    is an integer, so f b.(s - s_pc) / c is a ratio of integers: it is reduced modulo one cycle EXACTLY, in integer arithmetic, to
    [-1/2, 1/2) and only then divided (72 fractional bits).  |b|^2 - (b.s)^2 is formed exactly the same way, whatever cancels.
    Sine, cosine and the taper's exp run in numpy.longdouble (x87, 64-bit mantissa) and the sources are summed in longdouble; the
    result is rounded to complex128 at the end (the longdouble sums are kept beside it).
  tests/test_skyvis_reference.py holds the second route to the first on a seeded sub-sample of every case below: they must agree to
  1e-17 of S_f.  Measured 2026-10-21 on x86-64: the largest gap over all cases is 2.0e-19 of S_f (V and G alike; edges with the taper).

THE RULE (ISSUE "Hold every sky-sum kernel family to a 40-digit reference"; tests/test_gpu_skyvis_reference.py, no element excused,
output finite everywhere), with S_f = sum_s |pbflux[s][f]| and u = 2^-53:
    fp32 families:   |got - ref| <= 5e-6 S_f                       (the project's bar; the phase is reduced in fp64, so its length term is
                                                                    below 1e-9 even at 5e6 cycles and is not added)
    fp64 families:   |got - ref| <= (1e-11 + 2 pi r u N(b,f)) S_f  (1e-11 is the project's bar)
N'(b,f) = max_s |f| sum_i |b_i| |s_i - s_pc,i| / c is the phase scale: every rounding of the chain that forms one phase moves it by at
most u times a partial sum that this 1-norm bounds, so r roundings move the phase by at most r u N' cycles = 2 pi r u N' radians, and a
sum of unit phasors weighted by pbflux w (w <= 1) moves by at most that times S_f.  r is counted from the code, not fitted:

  R_RECURRENCE = 10, every kernel of skyvis_kernels.hip that seeds a phasor and steps it (k_skyvis_rec, _rec_f32pk, _taper_f64, _grad_*):
      1  s - s_pc, per component                     prep_dirs, skyvis_kernels.hip:2147
      1  inv_c = fl(1 / c), a rounded constant       ctx_internal.h:577
      1  the product with inv_c, per component       skyvis_kernels.hip:2147
      3  the dot product: one product and two FMAs   skyvis_kernels.hip:592 (front)
      2  f_c = f0 + (k0 + HC) df                     skyvis_kernels.hip:496 (one if contracted to an FMA; exact on the grids used here)
      1  the product d f_c N (N a power of two)      skyvis_kernels.hip:608
      1  the step d df N: the rounded step angle is applied up to CT / 2 times, (CT / 2) |df| <= |f| on every grid of the cases
         (skyvis_kernels.hip:609)
  R_DIRECT = 7, k_skyvis_direct: the first three rows (skyvis_kernels.hip:2041), the dot product (:2058) and d f (:2059); the
      reduction ph - rint(ph) is exact.
  R_ROTATE = 7, k_phase_rotate (aux_kernels.hip:581-582) on the given difference vector d = s_pc2 - s_pc: three products and two sums of
      the dot product (five roundings; three if contracted), the division by c, the product with f.  Its scale is N' with d in the place
      of s - s_pc.
  R_ORACLE = 10, oracle/skyvis_oracle.{py,c}: tau = (b.s) / c and tau_pc = (b.s_pc) / c are rounded SEPARATELY (five roundings of the dot
      product, one of the division, each), then tau - tau_pc (1), fl(2 pi) (1), the product with it (1) and with f (1).  The first six
      act on |b|.|s| and on |b|.|s_pc|, not on their difference, so the oracle's scale is N_abs = max_s |f| sum_i |b_i| (|s_i| + |s_pc,i|) / c
      >= N': the reason it loses the 1e-11 bar with the baseline length whatever the field of view.

FLOOR OF THE TWO ORACLES against this reference, the worst |oracle - ref| / S_f per set as tests/test_skyvis_reference.py prints it
(measured 2026-10-21 on x86-64, numpy 64-bit libm / gcc libm; V and G together; numpy oracle | C oracle):
    len_3e2  5.2e-14 | 5.7e-14 (N_abs 1.9e2)      len_3e3  5.3e-13 | 4.9e-13 (1.9e3)      len_3e4  5.8e-12 | 6.3e-12 (1.9e4)
    len_3e5  4.3e-11 | 4.6e-11 (1.9e5)            len_3e6  5.2e-10 | 4.5e-10 (1.9e6)      -- with the taper 5.2e-14 ... 3.7e-10 | 5.7e-14 ... 2.5e-10
    ragged 1.3e-13 | 1.1e-13    grids 1.3e-13 | 1.2e-13    sources 7.8e-14 | 6.5e-14    edges 1.9e-13 | 1.9e-13    taper 1.7e-13 | 2.0e-13
    (the numpy restatement returns NaN on the tapered edges set and on its rows +-b/|b| alone: the upstream square root of a rounded-negative
    |b|^2 - (c tau)^2; those sets are held on the C oracle only)
The error grows linearly with the phase, 2.4e-16 ... 3.4e-16 of S_f per cycle of N_abs: about 0.4 of ONE rounding of the bound's ten.
So both oracles keep 1e-11 of S_f up to the 30 km decade (6e4 cycles) and lose it from the 300 km decade on (ORACLE_KEEPS / ORACLE_LOSES
below, asserted); the derived bound holds on every set.
"""
import collections
import functools

import mpmath
import numpy as NP

LD = NP.longdouble
if NP.finfo(LD).eps > 1.1e-19:
    raise ImportError('skyvis_reference needs an x87 long double (64-bit mantissa); numpy.longdouble has eps = %g' % NP.finfo(LD).eps)

MP = mpmath.mp.clone()
MP.dps = 40

C_LIGHT = 299792458
U = 2.0 ** -53
BAR_F64 = 1e-11
BAR_F32 = 5e-6
R_RECURRENCE = 10
R_DIRECT = 7
R_ROTATE = 7
R_ORACLE = 10
ROUTE_GAP = 1e-17
ORACLE_KEEPS = ('len_3e2', 'len_3e3', 'len_3e4')          # decades on which both oracles are inside 1e-11 S_f
ORACLE_LOSES = ('len_3e5', 'len_3e6')                     # ... and outside it

_FRAC_BITS = 72

Case = collections.namedtuple('Case', 'name bl ch dc pb pc fw')
Ref = collections.namedtuple('Ref', 'V G S N Nabs v_ld g_ld')


def f64_bound(r, scale):
    """(1e-11 + 2 pi r u scale): the fp64 rule relative to S_f, scale = N' (device) or N_abs (oracle), any shape."""
    return BAR_F64 + 2.0 * NP.pi * r * U * NP.asarray(scale, dtype=NP.float64)


# ---- doubles as integers -------------------------------------------------------------------------------------------------------------
def ints(a):
    """(object array of Python ints n, k) with a == n * 2**-k exactly, element by element."""
    a = NP.asarray(a, dtype=NP.float64)
    m, e = NP.frexp(a)
    mi = NP.ldexp(m, 53).astype(NP.int64)                                # exact: |m| < 1 carries 53 bits
    ex = e.astype(NP.int64) - 53
    nz = mi != 0
    emin = int(ex[nz].min()) if nz.any() else 0
    out = NP.empty(a.shape, dtype=object)
    flat_m, flat_e, flat_o = mi.ravel(), ex.ravel(), out.ravel()
    for i in range(flat_m.size):
        flat_o[i] = int(flat_m[i]) << int(flat_e[i] - emin) if flat_m[i] else 0
    return out, -emin


def _int_to_ld(n, k):
    """The integer n times 2**-k as a longdouble (100 leading bits kept: 2^-100 relative)."""
    if n == 0:
        return LD(0)
    sign = -1 if n < 0 else 1
    n = abs(n)
    sh = max(n.bit_length() - 100, 0)
    t = n >> sh
    v = LD(float(t >> 50)) * LD(2.0 ** 50) + LD(float(t & ((1 << 50) - 1)))
    return sign * NP.ldexp(v, sh - k)


def to_ld(v):
    hi = float(v)
    return LD(hi) + LD(float(v - hi))


def ld_to_mp(v):
    hi = float(v)
    return MP.mpf(hi) + MP.mpf(float(v - LD(hi)))


def _kappa_mp(fwhm_deg):
    if not fwhm_deg > 0.0:
        return None
    return MP.log(2) * (2 * MP.sin(MP.mpf(float(fwhm_deg)) * MP.pi / 360)) ** 2


# ---- the fast route ------------------------------------------------------------------------------------------------------------------
def frac_cycles(num, k):
    """num * 2**-k / c modulo one cycle, in [-1/2, 1/2), as longdouble; num an object array of ints."""
    if k < 0:
        num, k = num * (1 << -k), 0
    den = C_LIGHT << k
    r = num % den
    r = NP.where((2 * r >= den).astype(bool), r - den, r)
    neg = (r < 0).astype(bool)
    q = (NP.where(neg, -r, r) * (1 << _FRAC_BITS)) // den                # truncated towards zero (V(-b) = conj V(b) bit for bit): 2^-72 cycle
    hi = (q // (1 << 32)).astype(NP.float64)                             # hi < 2^40 and lo < 2^32: exact in doubles
    lo = (q % (1 << 32)).astype(NP.float64)
    mag = NP.ldexp(hi.astype(LD) * LD(2.0 ** 32) + lo.astype(LD), -_FRAC_BITS)
    return NP.where(neg, -mag, mag)


def reference(bl, ch, dc, pb, pc, fwhm_deg=None, diff=None):
    """Ref(V [nbl][nchan] complex128, G [3][nbl][nchan], S_f [nchan], N' [nbl][nchan], N_abs [nbl][nchan], and the longdouble sums
    (re, im) behind V and G).  With `diff` (3,) given, s - s_pc is replaced by that one vector for every source (the phasor of a
    phase-centre rotation: pass one source of unit flux)."""
    bl = NP.ascontiguousarray(bl, dtype=NP.float64).reshape(-1, 3)
    ch = NP.ascontiguousarray(ch, dtype=NP.float64).ravel()
    dc = NP.ascontiguousarray(dc, dtype=NP.float64).reshape(-1, 3)
    pb = NP.ascontiguousarray(pb, dtype=NP.float64).reshape(dc.shape[0], ch.size)
    pc = NP.ascontiguousarray(pc, dtype=NP.float64).ravel()
    nbl, nchan, nsrc = bl.shape[0], ch.size, dc.shape[0]
    B, kb = ints(bl)
    F, kf = ints(ch)
    SP, kd = ints(NP.vstack((dc, pc[None, :], (NP.zeros(3) if diff is None else NP.asarray(diff, dtype=NP.float64))[None, :])))
    S, P, DV = SP[:nsrc], SP[nsrc], SP[nsrc + 1]
    D = NP.empty((nsrc, 3), dtype=object)
    for s in range(nsrc):
        for i in range(3):
            D[s, i] = DV[i] if diff is not None else S[s, i] - P[i]
    M = D[:, None, 0] * B[None, :, 0] + D[:, None, 1] * B[None, :, 1] + D[:, None, 2] * B[None, :, 2]          # [s][b], 2^-(kb + kd)
    frac = frac_cycles(M[:, :, None] * F[None, None, :], kb + kd + kf)                                        # [s][b][f]
    ang = frac * (LD(2) * to_ld(MP.pi))
    amp = pb.astype(LD)[:, None, :] * NP.ones((1, nbl, 1), dtype=LD)
    if fwhm_deg is not None:
        fw = NP.ascontiguousarray(fwhm_deg, dtype=NP.float64).ravel()
        BS = S[:, None, 0] * B[None, :, 0] + S[:, None, 1] * B[None, :, 1] + S[:, None, 2] * B[None, :, 2]     # b.s, 2^-(kb + kd)
        B2 = B[:, 0] * B[:, 0] + B[:, 1] * B[:, 1] + B[:, 2] * B[:, 2]                                         # |b|^2, 2^-(2 kb)
        f2 = ch.astype(LD) ** 2 / LD(C_LIGHT) ** 2
        for s in range(nsrc):
            kap = _kappa_mp(fw[s])
            if kap is None:
                continue
            kap = to_ld(kap)
            for b in range(nbl):
                p2 = B2[b] * (1 << (2 * kd)) - BS[s, b] * BS[s, b] if kd >= 0 else B2[b] - BS[s, b] * BS[s, b] * (1 << (-2 * kd))
                perp2 = _int_to_ld(max(p2, 0), 2 * kb + (2 * kd if kd >= 0 else 0))
                amp[s, b, :] *= NP.exp(-(kap * perp2) * f2)
    re = amp * NP.cos(ang)
    im = -(amp * NP.sin(ang))
    v_ld = (re.sum(axis=0), im.sum(axis=0))
    g_ld = tuple((NP.sum(dc[:, k].astype(LD)[:, None, None] * re, axis=0), NP.sum(dc[:, k].astype(LD)[:, None, None] * im, axis=0))
                 for k in range(3))
    V = v_ld[0].astype(NP.float64) + 1j * v_ld[1].astype(NP.float64)
    G = NP.stack([g[0].astype(NP.float64) + 1j * g[1].astype(NP.float64) for g in g_ld])
    d = NP.abs(dc - pc[None, :]) if diff is None else NP.abs(NP.asarray(diff, dtype=NP.float64))[None, :] * NP.ones((nsrc, 1))
    n1 = NP.max(NP.abs(bl) @ d.T, axis=1) if nsrc else NP.zeros(nbl)
    nabs = NP.max(NP.abs(bl) @ (NP.abs(dc) + NP.abs(pc)[None, :]).T, axis=1) if nsrc else NP.zeros(nbl)
    scale = NP.abs(ch)[None, :] / float(C_LIGHT)
    return Ref(V, G, NP.sum(NP.abs(pb), axis=0), n1[:, None] * scale, nabs[:, None] * scale, v_ld, g_ld)


# ---- the 40-digit route --------------------------------------------------------------------------------------------------------------
def reference_mp(bl, ch, dc, pb, pc, fwhm_deg, outputs):
    """[(V, G0, G1, G2)] as mpmath complex numbers for the (b, f) pairs of `outputs`, every term evaluated and summed at 40 digits."""
    bl = NP.ascontiguousarray(bl, dtype=NP.float64).reshape(-1, 3)
    dc = NP.ascontiguousarray(dc, dtype=NP.float64).reshape(-1, 3)
    c = MP.mpf(C_LIGHT)
    pcm = [MP.mpf(float(v)) for v in NP.ravel(pc)]
    res = []
    for b, k in outputs:
        bm = [MP.mpf(float(v)) for v in bl[b]]
        f = MP.mpf(float(ch[k]))
        taupc = sum(x * y for x, y in zip(bm, pcm)) / c
        blen2 = sum(x * x for x in bm)
        acc = [MP.mpc(0), MP.mpc(0), MP.mpc(0), MP.mpc(0)]
        for s in range(dc.shape[0]):
            sm = [MP.mpf(float(v)) for v in dc[s]]
            tau = sum(x * y for x, y in zip(bm, sm)) / c
            term = MP.mpf(float(pb[s][k])) * MP.expjpi(-2 * f * (tau - taupc))
            kap = _kappa_mp(fwhm_deg[s]) if fwhm_deg is not None else None
            if kap is not None:
                term = term * MP.exp(-kap * max(blen2 - (c * tau) ** 2, MP.zero) * f * f / (c * c))
            acc[0] += term
            for i in range(3):
                acc[1 + i] += sm[i] * term
        res.append(tuple(acc))
    return res


def route_gap(case, ref, nsample=24, seed=0):
    """Largest |fast route - mpmath route| / S_f over a seeded sub-sample of the case's outputs (the corners always), V and G."""
    rng = NP.random.default_rng(seed)
    nbl, nchan = ref.V.shape
    outs = {(0, 0), (nbl - 1, nchan - 1), (0, nchan - 1), (nbl - 1, 0)}
    while len(outs) < min(nsample, nbl * nchan):
        outs.add((int(rng.integers(nbl)), int(rng.integers(nchan))))
    outs = sorted(outs)
    worst = 0.0
    for (b, k), want in zip(outs, reference_mp(case.bl, case.ch, case.dc, case.pb, case.pc, case.fw, outs)):
        for (re, im), w in zip((ref.v_ld,) + tuple(ref.g_ld), want):
            gap = abs(MP.mpc(ld_to_mp(re[b, k]), ld_to_mp(im[b, k])) - w)
            if ref.S[k] == 0.0:                                          # the zero-flux row alone: both routes give 0 exactly
                assert gap == 0
                continue
            worst = max(worst, float(gap / MP.mpf(float(ref.S[k]))))
    return worst


# ---- the seeded case sets ------------------------------------------------------------------------------------------------------------
def altaz2dircos(alt_deg, az_deg):
    alt, az = NP.radians(NP.asarray(alt_deg, dtype=NP.float64)), NP.radians(NP.asarray(az_deg, dtype=NP.float64))
    return NP.stack((NP.cos(alt) * NP.sin(az), NP.cos(alt) * NP.cos(az), NP.sin(alt)), axis=-1)


PC = altaz2dircos(80.0, 30.0)
PC2 = altaz2dircos(62.0, 210.0)                           # the second phase centre of the k_phase_rotate cases
CH33 = 200e6 + 97656.25 * NP.arange(33)
LENGTHS = (('3e2', 3e2), ('3e3', 3e3), ('3e4', 3e4), ('3e5', 3e5), ('3e6', 3e6))


def _sky(rng, nsrc, nchan, alt_lo=5.0):
    alt = NP.degrees(NP.arcsin(rng.uniform(NP.sin(NP.radians(alt_lo)), 1.0, nsrc)))
    dc = altaz2dircos(alt, rng.uniform(0.0, 360.0, nsrc))
    pb = rng.uniform(0.5, 10.0, size=(nsrc, 1)) * rng.uniform(0.3, 1.0, size=(nsrc, nchan))
    return dc, pb


def _baselines(rng, nbl, lmax, lmin_frac=0.02):
    """Lengths up to lmax (the last row has it), the Up component 1 % of the horizontal draw."""
    length = rng.uniform(lmin_frac, 1.0, nbl) * lmax
    length[-1] = lmax
    ang = rng.uniform(0.0, 2.0 * NP.pi, nbl)
    bl = NP.stack((NP.cos(ang), NP.sin(ang), 0.01 * rng.uniform(-1.0, 1.0, nbl)), axis=1)
    return bl / NP.sqrt(NP.sum(bl ** 2, axis=1))[:, None] * length[:, None]


def _len_case(tag, lmax, taper):
    """70 baselines (two wavefronts, the second ragged), |b| <= 0.8 L so that the 3e2 array's one group keeps its step inside 1/8 cycle
    under sources 95 degrees from the phase centre (0.8 x 300 m x 1.48 x df / c = 0.116) and lifts."""
    rng = NP.random.default_rng(int(float(tag)) % 99991 + 7)
    bl = _baselines(rng, 70, 0.8 * lmax)
    dc, pb = _sky(rng, 21, CH33.size)
    fw = None
    if taper:
        # three runs of one size each (point sources, then two pixel sizes): the run-by-run and split forms are reachable; the sizes
        # that vary source by source are the second sky of the taper set
        fw = NP.concatenate((NP.zeros(5), NP.full(8, 0.008), NP.full(8, 0.02)))
    return Case('len_' + tag + ('_taper' if taper else ''), bl, CH33, dc, pb, PC, fw)


def _ragged_sky(ch, name, taper=False, seed=41):
    rng = NP.random.default_rng(seed)
    bl = _baselines(rng, 257, 300.0)
    dc, pb = _sky(rng, 5, ch.size)
    fw = rng.uniform(0.05, 0.8, 5) if taper else None
    return Case(name, bl, ch, dc, pb, PC, fw)


def _sources_case(nsrc, taper):
    rng = NP.random.default_rng(500 + nsrc)
    bl = _baselines(rng, 3, 280.0)
    ch = 150e6 + 97656.25 * NP.arange(64)
    dc, pb = _sky(rng, nsrc, 64)
    fw = NP.full(nsrc, 0.3) if taper else None
    return Case('sources_%d%s' % (nsrc, '_taper' if taper else ''), bl, ch, dc, pb, PC, fw)


EDGE_CH = 180e6 + 97656.25 * NP.arange(17)


def _edges_case(taper):
    rng = NP.random.default_rng(613)
    bl = _baselines(rng, 12, 250.0)
    bl[0] = 0.0                                                           # the zero vector
    bl[1] = (0.0, 0.0, 37.5)                                              # pure Up
    bl[2] = (1e-9, 0.0, 0.0)                                              # 1e-9 m
    bl[3] = -bl[7]                                                        # the negative of another row
    dc, pb = _sky(rng, 16, EDGE_CH.size)
    unit = bl[9] / NP.sqrt(NP.sum(bl[9] ** 2))
    dc[0] = PC                                                            # the phase centre itself
    dc[1] = (0.0, 0.0, 1.0)                                               # the zenith
    dc[2] = (NP.cos(0.7), NP.sin(0.7), 0.0)                               # z = +0.0
    dc[3] = (NP.cos(2.9), NP.sin(2.9), -0.0)                              # z = -0.0
    dc[4] = altaz2dircos(-1.0, 140.0)                                     # 1 degree below the horizon
    dc[5] = unit                                                          # +b / |b| of row 9: the taper clamp
    dc[6] = -unit
    dc[7] = dc[12]                                                        # an exact duplicate of another row
    pb[8] = 0.0                                                           # zero flux
    pb[9] = -pb[9]                                                        # negative flux
    fw = None
    if taper:
        fw = rng.uniform(0.05, 1.0, 16)
        fw[1] = 0.0
    return Case('edges_taper' if taper else 'edges', bl, EDGE_CH, dc, pb, PC, fw)


EDGE_ROWS = ('phase centre', 'zenith', 'z = +0', 'z = -0', 'below horizon', '+b/|b|', '-b/|b|', 'duplicate', 'zero flux', 'negative flux',
             'seeded')


def _edge_single(row, taper):
    c = _edges_case(taper)
    i = min(row, 10) if row < 10 else 10
    return Case('%s_row%d' % (c.name, row), c.bl, c.ch, c.dc[i:i + 1], c.pb[i:i + 1], c.pc, None if c.fw is None else c.fw[i:i + 1])


TAPER_FWHM = (0.0, 1e-6, 0.02, 0.4, 1.5, 30.0)


def _taper_case(fwhm):
    """64 baselines up to 1.2 km; fwhm None: mixed source by source."""
    rng = NP.random.default_rng(808)
    bl = _baselines(rng, 64, 1200.0, lmin_frac=0.005)
    dc, pb = _sky(rng, 24, CH33.size)
    dc = dc[NP.argsort(-dc[:, 2])]                                        # by decreasing altitude: the culled sources lead
    if fwhm is None:
        fw = NP.asarray(TAPER_FWHM)[rng.integers(0, len(TAPER_FWHM), 24)]
        return Case('taper_mixed', bl, CH33, dc, pb, PC, fw)
    return Case('taper_%g' % fwhm, bl, CH33, dc, pb, PC, NP.full(24, fwhm))


def _build():
    cases = collections.OrderedDict()

    def add(c):
        cases[c.name] = c
    for tag, lmax in LENGTHS:
        add(_len_case(tag, lmax, False))
        add(_len_case(tag, lmax, True))
    ch65 = 160e6 + 97656.25 * NP.arange(65)
    for taper in (False, True):
        sfx = '_taper' if taper else ''
        add(_ragged_sky(ch65, 'ragged' + sfx, taper))
        add(_ragged_sky(ch65[::-1].copy(), 'grids_descending' + sfx, taper))
        add(_ragged_sky(ch65[:1].copy(), 'grids_one_channel' + sfx, taper))
        add(_ragged_sky(30e6 + 390625.0 * NP.arange(65), 'grids_coarse' + sfx, taper))
        add(_ragged_sky(NP.sort(NP.random.default_rng(43).uniform(100e6, 200e6, 37)), 'grids_nonuniform' + sfx, taper))
        for n in (1, 3, 4, 5, 63, 64, 65, 130):
            add(_sources_case(n, taper))
        add(_edges_case(taper))
        for row in range(11):
            add(_edge_single(row, taper))
    for fw in TAPER_FWHM:
        add(_taper_case(fw))
    add(_taper_case(None))
    return cases


CASES = _build()
MAX_TERMS = 110000


def _decade(name):
    return float(name.split('_')[1]) if name.startswith('len_') else None


@functools.lru_cache(maxsize=None)
def get(name):
    """(Case, Ref) of a named set, computed once per process and checked on the reference alone."""
    c = CASES[name]
    assert c.bl.shape[0] * c.ch.size * c.dc.shape[0] <= MAX_TERMS, name
    r = reference(c.bl, c.ch, c.dc, c.pb, c.pc, c.fw)
    for a in (r.V, r.G, r.S, r.N, r.Nabs):
        assert NP.all(NP.isfinite(a.view(NP.float64) if NP.iscomplexobj(a) else a)), name
        a.setflags(write=False)
    single_zero_flux = c.dc.shape[0] == 1 and not NP.any(c.pb)
    assert single_zero_flux or NP.all(r.S > 0.0), name
    lmax = _decade(name)
    if lmax is not None:
        # the decade the case is named for: L f / c cycles at the band's top, within a factor sqrt(10) either way
        centre = lmax * float(c.ch.max()) / C_LIGHT
        assert centre / NP.sqrt(10.0) <= r.N.max() <= centre * NP.sqrt(10.0), (name, r.N.max(), centre)
        assert 4.0 * r.Nabs.max() < 2.0 ** 31
    return c, r


@functools.lru_cache(maxsize=None)
def rotation(name):
    """Phasor exp(-2 pi i f b.d / c) of the rotation from PC to PC2 on the case's array, d = PC2 - PC as the doubles the device is given:
    (d, phasor (re, im) in longdouble [nbl][nchan], its phase scale [nbl][nchan])."""
    c = CASES[name]
    d = PC2 - c.pc
    r = reference(c.bl, c.ch, NP.zeros((1, 3)), NP.ones((1, c.ch.size)), c.pc, None, diff=d)
    return d, r.v_ld, r.N
