"""40-digit reference of the analytic primary beams (TEST INFRASTRUCTURE).

What k_beam_flux<KIND> / k_beam_flux_plain<KIND> (prisim_amd/csrc/aux_kernels.hip, beam_flux_body) compute for one source s and channel f:
    power[s][f] = (element_field x array_factor)^2 x ground_field^2,        pbflux[s][f] = power x flux_ref (f / ref_freq)^spindex
This module shares no code with oracle/beams_oracle.py or prisim_amd.  Direction cosines, pointing, frequencies and parameters are taken
exactly as the doubles they are, and the function the kernel states is evaluated on them in mpmath at 40 digits (pi, c = 299792458 and the
rotation by east2ax1 exact); the flux runs in numpy.longdouble.

It also builds the seeded edge direction sets that tests/test_beam_reference.py (CPU: the fp64 restatement oracle/beams_oracle.py against
this reference) and tests/test_gpu_beam_edges.py (the device against it) share, and states the acceptance rule.

THE RULE.  Every power value is held to |got - reference| <= BOUND = 1e-12 absolute (the bar the suite sets for these kernels against
the goldens; peak power is 1, so it is relative to the peak as well), output finite everywhere, blank elements exactly 0.0, no element
excused.  With a flux, |got - reference x flux| <= BOUND x flux, the flux formed in longdouble.  For the rule to be unconditional each
set is checked when it is built, on the reference alone (_check_set):
  * no non-blank row of a dish set has |cosx| < 1e-9 -- there the sign of a rounded dot product decides the blanking -- unless the
    pointing is a coordinate axis (the zenith): then two of the three products are exact zeros, cosx IS the source's z in any fp64
    evaluation order, with or without FMA contraction, and the rows a hair above the horizon can be held under that pointing too;
  * no row has 0 < |z| < 1e-300 other than the one named denormal;
  * every reference value is finite.
"""
import collections
import functools
import math

import mpmath
import numpy as NP

LD = NP.longdouble
if NP.finfo(LD).eps > 1.1e-19:
    raise ImportError('beam_reference needs an x87 long double (64-bit mantissa); numpy.longdouble has eps = %g' % NP.finfo(LD).eps)

MP = mpmath.mp.clone()
MP.dps = 40

C_LIGHT = 299792458
BOUND = 1e-12
CHANNELS = 150e6 + 4e6 * (NP.arange(5) - 2.0)
MID = 2
J1_ZEROS = (3.8317059702075125, 7.015586669815619, 10.173468135062722)
DENORMAL = 5e-324

# Largest |oracle/beams_oracle.py - this reference| (power, absolute) per family of sets, as tests/test_beam_reference.py prints them:
# the floor of an fp64 restatement.  Measured 2026-10-21 on x86-64 (numpy 64-bit libm, scipy j1):
#     airy 2.0e-15 (+array +ground 1.8e-15)   gaussian 1.4e-15 (+array +ground 1.5e-15)
#     dipole short 2.8e-16   halfwave 3.9e-16   general 6.0e-16          ground plane 3.3e-16
#     array 4x4 at 1.1 m 2.0e-16   4x3 at 4, 5 m 8.8e-15   5x2 at 4, 5 m 1.2e-15   -- off the grating lobes of the nax 3 and nax 5 axes;
#     ON them the literal sin(n phi/2) / sin(phi/2) / n is off by 1.13 (4x3, the lobe itself), 0.29 (5x2), 9.4e-3 ... 5.7e-3 at a
#     relative distance of 1e-14, 1.1e-4 at 1e-12, 1.1e-7 at 1e-9, 1.9e-9 at 1e-7, 1.9e-10 at 1e-6, 9.4e-13 at 1e-4, 9.5e-14 at 1e-3
#     launch cases (Airy D = 14 m, 17 and 61 channels) 1.3e-15
# The device is held to BOUND = 1e-12, not to a multiple of these.  (The alt-az statement of the restatement cannot carry a source
# less than the spacing of doubles at 90 above the horizon under a zenith pointing -- 90 - alt == 90 -- so the rows 'z = 5e-324' and
# 'alt 1e-14 deg' of the zenith dish sets are held on the device only.)

Spec = collections.namedtuple('Spec', 'kind size pointing dipole_axis dipole_mode array ground')
Spec.__new__.__defaults__ = ('delta', 0.0, (0.0, 0.0, 1.0), (1.0, 0.0, 0.0), 'general', None, None)
Array = collections.namedtuple('Array', 'nax1 nax2 sep1 sep2 east2ax1 pointing')
Ground = collections.namedtuple('Ground', 'height scale max')          # scale = max = None: no modifier
Ground.__new__.__defaults__ = (None, None)

ZENITH = (0.0, 0.0, 1.0)


# ---- the function, 40 digits --------------------------------------------------------------------------------------------------------
def _mpf(v):
    return MP.mpf(float(v))


def _to_ld(v):
    hi = float(v)
    return LD(hi) + LD(float(v - hi))


def _airy(a):
    return 2 * MP.besselj(1, a) / a


def _dipole_field(spec, s, kh):
    dot = sum(_mpf(u) * c for u, c in zip(spec.dipole_axis, s))
    dot = min(max(dot, MP.mpf(-1)), MP.mpf(1))
    ang = MP.acos(dot)
    if spec.dipole_mode == 'short':
        return MP.sin(ang)
    mx = MP.one if spec.dipole_mode == 'halfwave' else 1 - MP.cos(kh)
    if abs(abs(dot) - 1) < _mpf(1e-10):                                  # the L'Hospital branch, both modes
        return kh * MP.sin(kh * MP.cos(ang)) * MP.tan(ang) / mx
    if spec.dipole_mode == 'halfwave':
        return MP.cos(MP.pi / 2 * MP.cos(ang)) / MP.sin(ang)
    return (MP.cos(kh * MP.cos(ang)) - MP.cos(kh)) / MP.sin(ang) / mx


def _array_term(n, phi):
    if abs(phi) < _mpf(1e-10):
        return MP.cos(n * phi / 2) / MP.cos(phi / 2)
    return MP.sin(n * phi / 2) / MP.sin(phi / 2) / n


def _array_rel(arr, s):
    """(rx, ry): the source's and the array pointing's direction cosines in the array's axes, their difference."""
    ang = _mpf(arr.east2ax1) * MP.pi / 180
    rc, rs = MP.cos(ang), MP.sin(ang)
    ax, ay = _mpf(arr.pointing[0]), _mpf(arr.pointing[1])
    return (rc * s[0] + rs * s[1]) - (rc * ax + rs * ay), (-rs * s[0] + rc * s[1]) - (-rs * ax + rc * ay)


def _ground_field(gnd, z, k):
    nz = min(max(z, MP.mpf(-1)), MP.mpf(1))
    gp = MP.sin(k * _mpf(gnd.height) * nz)
    if gnd.scale is not None or gnd.max is not None:
        val = MP.inf if z == 0 else 1 / MP.sqrt(abs(z))
        if gnd.scale is not None:
            val = val * _mpf(gnd.scale)
        if gnd.max is not None:
            val = min(max(val, MP.zero), _mpf(gnd.max))
        gp = gp * val
    return gp / MP.sin(k * _mpf(gnd.height))


def power(spec, dircos, freqs):
    """Reference power [n, nf] (longdouble), blank mask [n], cosx [n] (float) of Spec `spec` at direction cosines [n, 3] and `freqs`."""
    dc = NP.ascontiguousarray(dircos, dtype=NP.float64).reshape(-1, 3)
    fr = NP.ascontiguousarray(freqs, dtype=NP.float64).ravel()
    out = NP.zeros((dc.shape[0], fr.size), dtype=LD)
    blank = NP.zeros(dc.shape[0], dtype=bool)
    cosxs = NP.zeros(dc.shape[0])
    p = [_mpf(v) for v in spec.pointing]
    dish = spec.kind in ('airy', 'gaussian')
    tol = _mpf(1e-10)
    per_f = []
    for f in fr:
        f = _mpf(f)
        k, lam = 2 * MP.pi * f / C_LIGHT, C_LIGHT / f
        half = k * _mpf(spec.size) / 2
        sigma_aprtr = _mpf(spec.size) / (2 * MP.sqrt(2 * MP.log(2))) / lam
        per_f.append((k, lam, half, _airy(half * MP.sin(tol)) if spec.kind == 'airy' else None,
                      1 / (2 * MP.pi * sigma_aprtr) if spec.kind == 'gaussian' else None))
    for i in range(dc.shape[0]):
        s = [_mpf(v) for v in dc[i]]
        cr = (s[1] * p[2] - s[2] * p[1], s[2] * p[0] - s[0] * p[2], s[0] * p[1] - s[1] * p[0])
        sinx = MP.sqrt(cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2])
        cosx = s[0] * p[0] + s[1] * p[1] + s[2] * p[2]
        cosxs[i] = float(cosx)
        blank[i] = dish and (cosx <= 0 or s[2] <= 0)
        if blank[i]:
            continue
        if spec.array is not None:
            rx, ry = _array_rel(spec.array, s)
        for j, (k, lam, half, airy0, sigma_dircos) in enumerate(per_f):
            if spec.kind == 'gaussian':
                ep = MP.exp(-(sinx / sigma_dircos) ** 2 / 2)
            elif spec.kind == 'airy':
                ep = _airy(half * max(sinx, MP.sin(tol))) / airy0
            elif spec.kind == 'dipole':
                ep = _dipole_field(spec, s, half)
            else:
                ep = MP.one
            af = MP.one
            if spec.array is not None:
                a = spec.array
                af = _array_term(a.nax1, 2 * MP.pi * _mpf(a.sep1) * rx / lam) * _array_term(a.nax2, 2 * MP.pi * _mpf(a.sep2) * ry / lam)
            pw = (ep * af) ** 2
            if spec.ground is not None:
                pw = pw * _ground_field(spec.ground, s[2], k) ** 2
            out[i, j] = _to_ld(pw) if MP.isfinite(pw) else LD(NP.nan)
    return out, blank, cosxs


def flux(flux_ref, spindex, ref_freq, freqs):
    """flux_ref (f / ref_freq)^spindex [n, nf] in longdouble."""
    ratio = NP.asarray(freqs, dtype=NP.float64).astype(LD) / LD(ref_freq)
    return NP.asarray(flux_ref, dtype=NP.float64).astype(LD)[:, None] * NP.power(ratio[None, :], NP.asarray(spindex, dtype=NP.float64).astype(LD)[:, None])


def deviation(got, ref):
    """|got - reference| per element, as doubles (formed in longdouble)."""
    return NP.abs(NP.asarray(got, dtype=NP.float64).astype(LD) - ref).astype(NP.float64)


# ---- direction sets -----------------------------------------------------------------------------------------------------------------
def altaz2dircos(alt_deg, az_deg):
    alt, az = math.radians(alt_deg), math.radians(az_deg)
    return NP.array([math.cos(alt) * math.sin(az), math.cos(alt) * math.cos(az), math.sin(alt)])


def dircos2altaz(d):
    return NP.array([math.degrees(math.asin(max(-1.0, min(1.0, d[2])))), math.degrees(math.atan2(d[0], d[1])) % 360.0])


class _Rows:
    def __init__(self):
        self.labels, self.dircos, self.altaz = [], [], []

    def add(self, label, dircos, altaz=None):
        d = NP.asarray(dircos, dtype=NP.float64)
        self.labels.append(label)
        self.dircos.append(d)
        self.altaz.append(dircos2altaz(d) if altaz is None else NP.asarray(altaz, dtype=NP.float64))

    def arrays(self):
        return list(self.labels), NP.ascontiguousarray(NP.stack(self.dircos)), NP.stack(self.altaz)


OFF_ZENITH_ALTAZ = (70.0, 200.0)
HORIZON_AZ = 200.0


def dish_rows(diameter, zenith, seed):
    """The dish set: see the module docstring of tests/test_gpu_beam_edges.py for the list.  zenith: pointing (0, 0, 1) and rows built
    from (zenith angle, azimuth), whose alt-az is (90 - t, a); else pointing alt 70, az 200 and rows p cos t + e sin t, alt-az derived."""
    rng = NP.random.default_rng(seed)
    rows = _Rows()
    if zenith:
        p = NP.array(ZENITH)

        def at(t, b):
            return NP.array([math.sin(t) * math.sin(b), math.sin(t) * math.cos(b), math.cos(t)]), (90.0 - math.degrees(t), math.degrees(b) % 360.0)
    else:
        p = altaz2dircos(*OFF_ZENITH_ALTAZ)
        alt0, az0 = math.radians(OFF_ZENITH_ALTAZ[0]), math.radians(OFF_ZENITH_ALTAZ[1])
        e1 = NP.array([math.cos(az0), -math.sin(az0), 0.0])                                     # along increasing azimuth
        e2 = NP.array([-math.sin(alt0) * math.sin(az0), -math.sin(alt0) * math.cos(az0), math.cos(alt0)])     # along increasing altitude

        def at(t, b):
            return p * math.cos(t) + (e1 * math.cos(b) + e2 * math.sin(b)) * math.sin(t), None
    rows.add('pointing', p, (90.0, 0.0) if zenith else OFF_ZENITH_ALTAZ)
    for t in (1e-11, 7e-11, 1.2e-10, 3e-10):
        rows.add('offset %g' % t, *at(t, 0.7))
    k0_half = 2 * math.pi * CHANNELS[MID] / C_LIGHT * 0.5 * diameter
    for m, zero in enumerate(J1_ZEROS):
        sx = zero / k0_half
        if sx >= 1.0:
            continue                                                                            # not on the sky (D = 0.5 m)
        if zenith:                                                                              # azimuth 0: |s x p| is the y component
            for lab, y in (('J1 zero %d' % (m + 1), sx), ('J1 zero %d, next double' % (m + 1), NP.nextafter(sx, 1.0))):
                rows.add(lab, [0.0, y, math.sqrt((1.0 - y) * (1.0 + y))], (90.0 - math.degrees(math.asin(y)), 0.0))
        else:
            d, _ = at(math.asin(sx), 0.7)
            rows.add('J1 zero %d' % (m + 1), d)
            d2 = d.copy()
            d2[0] = NP.nextafter(d2[0], 2.0)
            rows.add('J1 zero %d, next double' % (m + 1), d2)
    rows.add('1 rad off axis', *at(1.0, 0.0))
    az = math.radians(HORIZON_AZ)
    for lab, z in (('z = 5e-324', DENORMAL), ('z = +0.0', 0.0), ('z = -0.0', -0.0)):
        rows.add(lab, [math.sin(az), math.cos(az), z])
    for alt in (1e-14, 1e-7, -1e-9):
        rows.add('alt %g deg' % alt, altaz2dircos(alt, HORIZON_AZ), (alt, HORIZON_AZ))
    for _ in range(12):
        rows.add('seeded', *at(rng.uniform(0.02, 1.0), rng.uniform(0.0, 2 * math.pi)))
    return p, rows.arrays()


DIPOLE_ROTATIONS = (1e-6, 1.3e-5, 1.41e-5, 1.4143e-5, 1.5e-5, 2e-5, 1e-4, 1e-3)
TILTED_AXIS_ALTAZ = (20.0, 35.0)


def dipole_rows(tilted, seed):
    """The dipole set about the axis [1, 0, 0] or the tilted one (alt 20, az 35): rotations u cos t + m sin t, m perpendicular to u."""
    rng = NP.random.default_rng(seed)
    rows = _Rows()
    if tilted:
        u = altaz2dircos(*TILTED_AXIS_ALTAZ)
        h = math.hypot(u[0], u[1])
        v = NP.array([-u[1] / h, u[0] / h, 0.0])
        w = NP.cross(u, v)
    else:
        u, v, w = NP.array([1.0, 0.0, 0.0]), NP.array([0.0, 1.0, 0.0]), NP.array([0.0, 0.0, 1.0])
    m = 0.6 * v + 0.8 * w
    rows.add('axis', u)
    rows.add('opposite', -u)
    for t in DIPOLE_ROTATIONS:
        rows.add('rotated %g' % t, u * math.cos(t) + m * math.sin(t))
    for t in (1.41e-5, 1.4143e-5):
        rows.add('mirror of rotated %g' % t, -u * math.cos(t) + m * math.sin(t))
    rows.add('broadside', m)
    rows.add('broadside, up', w)
    for _ in range(12):
        z, a = rng.uniform(0.05, 1.0), rng.uniform(0.0, 2 * math.pi)
        r = math.sqrt((1.0 - z) * (1.0 + z))
        rows.add('seeded', [r * math.sin(a), r * math.cos(a), z])
    return tuple(float(c) for c in u), rows.arrays()


ARRAY_POINTING_ALTAZ = (70.0, 120.0)
ARRAY_EAST2AX1 = 30.0
LOBE_DISPLACEMENTS = (1e-14, 1e-12, 1e-9, 1e-7, 1e-6, 1e-4, 1e-3)


def array_rows(nax1, nax2, sep1, sep2, seed):
    """The array set.  Labels of the grating-lobe rows: 'lobe axis<1|2> <+|-> displaced <d>' (d = 0 at the lobe)."""
    rng = NP.random.default_rng(seed)
    rows = _Rows()
    pc = altaz2dircos(*ARRAY_POINTING_ALTAZ)
    ang = math.radians(ARRAY_EAST2AX1)
    axes = (NP.array([math.cos(ang), math.sin(ang)]), NP.array([-math.sin(ang), math.cos(ang)]))
    lam0 = C_LIGHT / CHANNELS[MID]

    def place(label, r1, r2):
        xy = pc[:2] + r1 * axes[0] + r2 * axes[1]
        q = xy[0] * xy[0] + xy[1] * xy[1]
        if q < 1.0:                                                                             # else not on the sky: dropped
            rows.add(label, [xy[0], xy[1], math.sqrt(1.0 - q)])
    rows.add('pointing', pc)
    for ax, sep in ((0, sep1), (1, sep2)):
        for ph in (6e-12, 2e-10):
            r = ph * lam0 / (2 * math.pi * sep)
            place('|phi| %g axis%d' % (ph, ax + 1), *((r, 0.0) if ax == 0 else (0.0, r)))
        for sg in (1.0, -1.0):
            lobe = sg * lam0 / sep
            for d in (0.0,) + LOBE_DISPLACEMENTS:
                r = lobe * (1.0 + d)
                place('lobe axis%d %s displaced %g' % (ax + 1, '+' if sg > 0 else '-', d), *((r, 0.0) if ax == 0 else (0.0, r)))
            for frac, lab in ((0.5, 'half'), (0.25, 'quarter')):
                r = lobe * frac
                place('%s lobe axis%d %s' % (lab, ax + 1, '+' if sg > 0 else '-'), *((r, 0.0) if ax == 0 else (0.0, r)))
    for _ in range(10):
        z, a = rng.uniform(0.05, 1.0), rng.uniform(0.0, 2 * math.pi)
        r = math.sqrt((1.0 - z) * (1.0 + z))
        rows.add('seeded', [r * math.sin(a), r * math.cos(a), z])
    return tuple(float(c) for c in pc), rows.arrays()


def ground_rows(with_max, seed):
    rng = NP.random.default_rng(seed)
    rows = _Rows()
    rows.add('zenith', ZENITH, (90.0, 0.0))
    for alt in (30.0, 1e-3, 1e-7):
        rows.add('alt %g deg' % alt, altaz2dircos(alt, 40.0), (alt, 40.0))
    if with_max:
        rows.add('z = 0', [math.sin(0.3), math.cos(0.3), 0.0])
    for _ in range(8):
        z, a = rng.uniform(0.01, 1.0), rng.uniform(0.0, 2 * math.pi)
        r = math.sqrt((1.0 - z) * (1.0 + z))
        rows.add('seeded', [r * math.sin(a), r * math.cos(a), z])
    return rows.arrays()


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
DISH_KINDS = ('airy', 'gaussian')
DIAMETERS = (0.5, 14.0, 300.0)
POINTINGS = ('zenith', 'offzenith')
DIPOLE_LENGTHS = (0.74, 1.5, 2.0)
DIPOLE_MODES = ('short', 'halfwave', 'general')
DIPOLE_AXES = ('x', 'tilted')
ARRAYS = ((4, 4, 1.1, 1.1), (4, 3, 4.0, 5.0), (5, 2, 4.0, 5.0))
GROUND_HEIGHTS = (0.3, 0.4)
GROUND_MODIFIER = {'scale': 0.8, 'max': 2.5}

DISH_CASES = [(k, d, p) for k in DISH_KINDS for d in DIAMETERS for p in POINTINGS]
DIPOLE_CASES = [(ln, ax, m) for ln in DIPOLE_LENGTHS for ax in DIPOLE_AXES for m in DIPOLE_MODES]
GROUND_CASES = [(h, mod) for h in GROUND_HEIGHTS for mod in (False, True)]

Case = collections.namedtuple('Case', 'name spec labels dircos altaz freqs ref blank cosx')


def _check_set(name, spec, labels, dircos, ref, blank, cosx):
    dish = spec.kind in ('airy', 'gaussian')
    axis_pointing = sorted(abs(c) for c in spec.pointing) == [0.0, 0.0, 1.0]
    for i, lab in enumerate(labels):
        z = dircos[i, 2]
        assert not (0.0 < abs(z) < 1e-300) or (lab == 'z = 5e-324' and z == DENORMAL), (name, lab)
        if dish and not blank[i] and not axis_pointing:
            assert abs(cosx[i]) >= 1e-9, (name, lab, cosx[i])
    assert NP.all(NP.isfinite(ref.astype(NP.float64))), name
    assert NP.all(ref[blank] == 0)
    assert len(labels) <= 64, name


def _case(name, spec, labels, dircos, altaz, freqs=CHANNELS):
    ref, blank, cosx = power(spec, dircos, freqs)
    _check_set(name, spec, labels, dircos, ref, blank, cosx)
    return Case(name, spec, labels, dircos, altaz, NP.asarray(freqs, dtype=NP.float64), ref, blank, cosx)


@functools.lru_cache(maxsize=None)
def dish_case(kind, diameter, pointing, extras=False):
    """extras: under a (4, 4, 1.1, 1.1) array factor pointed at the beam's pointing and a 0.3 m ground plane (k_beam_flux<KIND>)."""
    p, (labels, dc, altaz) = dish_rows(diameter, pointing == 'zenith', seed=int(10 * diameter) + (0 if pointing == 'zenith' else 1))
    p = tuple(float(c) for c in p)
    spec = Spec(kind=kind, size=diameter, pointing=p)
    if extras:
        spec = spec._replace(array=Array(4, 4, 1.1, 1.1, 0.0, p), ground=Ground(0.3))
    return _case('%s D=%g %s%s' % (kind, diameter, pointing, ' +array +ground' if extras else ''), spec, labels, dc, altaz)


@functools.lru_cache(maxsize=None)
def dipole_case(length, axis, mode):
    u, (labels, dc, altaz) = dipole_rows(axis == 'tilted', seed=int(100 * length) + (axis == 'tilted'))
    return _case('dipole L=%g %s %s' % (length, axis, mode), Spec(kind='dipole', size=length, dipole_axis=u, dipole_mode=mode), labels, dc, altaz)


@functools.lru_cache(maxsize=None)
def array_case(nax1, nax2, sep1, sep2):
    pc, (labels, dc, altaz) = array_rows(nax1, nax2, sep1, sep2, seed=10 * nax1 + nax2)
    return _case('array %dx%d %g,%g m' % (nax1, nax2, sep1, sep2), Spec(array=Array(nax1, nax2, sep1, sep2, ARRAY_EAST2AX1, pc)), labels, dc, altaz)


@functools.lru_cache(maxsize=None)
def ground_case(height, modifier):
    labels, dc, altaz = ground_rows(modifier, seed=int(10 * height) + modifier)
    gnd = Ground(height, GROUND_MODIFIER['scale'], GROUND_MODIFIER['max']) if modifier else Ground(height)
    return _case('ground h=%g%s' % (height, ' modified' if modifier else ''), Spec(ground=gnd), labels, dc, altaz)


def noisy_lobe_rows(case):
    """Rows of an array case on a grating lobe (any displacement) of an axis whose nax is not a power of two -- where the literal
    sin(n phi/2) / sin(phi/2) is noise in fp64 -- and, of those, the rows displaced by 1e-7 or less."""
    a = case.spec.array
    noisy = [ax for ax, n in ((1, a.nax1), (2, a.nax2)) if n & (n - 1)]
    lobe = NP.array([lab.startswith('lobe axis') and int(lab[9]) in noisy for lab in case.labels])
    near = NP.array([bool(lb) and float(lab.split()[-1]) <= 1e-7 for lb, lab in zip(lobe, case.labels)])
    return lobe, near


LAUNCH_SHAPES = ((20011, 17), (70001, 61))


@functools.lru_cache(maxsize=None)
def launch_case(nsrc, nchan):
    """Rows drawn with repeats from the distinct directions of the Airy D = 14 m off-zenith dish set, channels 150e6 + 1e5 k, each row
    its own power-law flux.  Returns (Case on the distinct directions at these channels, rows [nsrc], flux_ref, spindex, ref_freq)."""
    base = dish_case('airy', 14.0, 'offzenith')
    freqs = 150e6 + 1e5 * NP.arange(nchan)
    case = _case('launch %d x %d' % (nsrc, nchan), base.spec, base.labels, base.dircos, base.altaz, freqs)
    rng = NP.random.default_rng(nsrc)
    rows = NP.concatenate([rng.permutation(len(base.labels)), rng.integers(0, len(base.labels), nsrc - len(base.labels))])
    rng.shuffle(rows)
    return case, rows, rng.uniform(0.1, 10.0, nsrc), rng.uniform(-3.0, 1.0, nsrc), float(freqs[nchan // 2])
