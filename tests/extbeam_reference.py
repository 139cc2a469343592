"""40-digit reference of the external HEALPix beam (TEST INFRASTRUCTURE).

What the device chain k_extbeam_table / k_extbeam_gather / k_colmax_* / k_extbeam_finish computes (scripts/run_prisim.py:2091-2103):
    table[p][c] = sum_j M[c][j] log10(beam[p][j])
    work[s][c]  = bilinear HEALPix interpolation of table[.][c] at source s      (Healpix_Base::get_interpol, RING scheme)
    pb[s][c]    = float32( 10 ** (work[s][c] - max(nanmax_s work[s][c], 0)) )

This module shares no code with oracle/healpix_oracle.py or prisim_amd.geometry: ring latitudes, start pixels, ring lengths and shifts
are the closed forms of Gorski et al. 2005 (ApJ 622, 759; eqs. 4-9).  The geometry (zenith angle, azimuth, ring above, four pixels and
their weights) runs in mpmath at 40 digits on the direction cosines taken exactly as the doubles they are; the arithmetic on the map
(the sum over frequency, the four-pixel sum, the column maximum, 10 ** x) runs in numpy.longdouble (64-bit mantissa).

It also builds the seeded beams, matrices and edge direction sets that tests/test_extbeam_reference.py (CPU: the fp64 restatement
against this reference) and tests/test_gpu_extbeam_edges.py (the device against it) share, and holds the acceptance rule.
"""
import functools

import mpmath
import numpy as NP

LD = NP.longdouble
if NP.finfo(LD).eps > 1.1e-19:
    raise ImportError('extbeam_reference needs an x87 long double (64-bit mantissa); numpy.longdouble has eps = %g' % NP.finfo(LD).eps)

MP = mpmath.mp.clone()
MP.dps = 40

# Largest relative deviation of the fp64 restatement's 10 ** work (oracle/healpix_oracle.py, theta = atan2(hypot(x, y), z)) from this
# reference over every direction set of cases(): measured 2026-10-20 on x86-64, per nside
#     1: 4.3e-15   2: 8.2e-15   3: 1.8e-14   6: 5.9e-14   8: 3.9e-14   64: 2.573e-13
# (test_extbeam_reference.py prints them).  DELTA = 8 x the largest: the device's own log10, exp10, atan2 and FMA contraction each cost a
# few ulp more than numpy's and do not grow with anything.
FLOOR_MEASURED = 2.6e-13
DELTA = 8 * FLOOR_MEASURED
EXCUSED_SHARE = 1e-3

NSIDES = (1, 2, 3, 6, 8, 64)
RINGS_64 = (1, 2, 63, 64, 65, 128, 191, 192, 193, 254, 255)


# ---- geometry, 40 digits ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ring(nside, ir):
    """(start pixel, pixels in ring, colatitude [mpf], shift) of ring ir in 1 .. 4 nside - 1; pixel centres of the ring sit at azimuth
    (j + shift / 2) 2 pi / nr, j = 0 .. nr - 1 (Gorski et al. 2005 eqs. 4-9)."""
    npix = 12 * nside * nside
    north = min(ir, 4 * nside - ir)
    if north < nside:
        z = 1 - MP.mpf(north * north) / (3 * nside * nside)
        nr, start, shift = 4 * north, 2 * north * (north - 1), 1
    else:
        z = MP.mpf(2 * (2 * nside - north)) / (3 * nside)
        nr, start, shift = 4 * nside, 2 * nside * (nside - 1) + (north - nside) * 4 * nside, 1 - (north - nside) % 2
    theta = MP.acos(z)
    if ir > 2 * nside:
        theta, start = MP.pi - theta, npix - start - nr
    return start, nr, theta, shift


def weights_at(nside, theta, phi):
    """The four pixels and mpf weights of Healpix_Base::get_interpol at colatitude theta in [0, pi] and azimuth phi in [0, 2 pi) (mpf)."""
    npix = 12 * nside * nside
    zc = MP.cos(theta)
    az = abs(zc)
    if az <= MP.mpf(2) / 3:
        ir1 = int(MP.floor(nside * (2 - 1.5 * zc)))
    else:
        irr = int(MP.floor(nside * MP.sqrt(3 * (1 - az))))
        ir1 = irr if zc > 0 else 4 * nside - irr - 1
    ir2 = ir1 + 1
    pix, wgt, th = [0, 0, 0, 0], [MP.zero] * 4, [None, None]
    for k, ir in enumerate((ir1, ir2)):
        if not 1 <= ir <= 4 * nside - 1:
            continue
        start, nr, th[k], shift = ring(nside, ir)
        tmp = phi * nr / (2 * MP.pi) - MP.mpf(shift) / 2
        i1 = int(MP.floor(tmp))
        w1 = tmp - i1
        pix[2 * k], pix[2 * k + 1] = start + i1 % nr, start + (i1 + 1) % nr
        wgt[2 * k], wgt[2 * k + 1] = 1 - w1, w1
    if ir1 == 0:                                           # north polar cap: ring 1 and, opposite, the mean of its four pixels
        wth = theta / th[1]
        fac = (1 - wth) / 4
        wgt = [fac, fac, wgt[2] * wth + fac, wgt[3] * wth + fac]
        pix[0], pix[1] = (pix[2] + 2) & 3, (pix[3] + 2) & 3
    elif ir2 == 4 * nside:                                 # south polar cap
        wth = (theta - th[0]) / (MP.pi - th[0])
        fac = wth / 4
        wgt = [wgt[0] * (1 - wth) + fac, wgt[1] * (1 - wth) + fac, fac, fac]
        pix[2], pix[3] = ((pix[0] + 2) & 3) + npix - 4, ((pix[1] + 2) & 3) + npix - 4
    else:
        wth = (theta - th[0]) / (th[1] - th[0])
        wgt = [wgt[0] * (1 - wth), wgt[1] * (1 - wth), wgt[2] * wth, wgt[3] * wth]
    return pix, wgt


def _to_ld(v):
    hi = float(v)
    return LD(hi) + LD(float(v - hi))


def interpol(nside, dircos):
    """(pix [n, 4] int64, wgt [n, 4] longdouble) for direction cosines (East, North, Up) [n, 3], each double taken exactly:
    theta = atan2(hypot(x, y), z), phi = atan2(x, y) mod 2 pi."""
    dc = NP.ascontiguousarray(dircos, dtype=NP.float64).reshape(-1, 3)
    pix = NP.zeros((dc.shape[0], 4), dtype=NP.int64)
    wgt = NP.zeros((dc.shape[0], 4), dtype=LD)
    two_pi = 2 * MP.pi
    for s in range(dc.shape[0]):
        x, y, z = MP.mpf(float(dc[s, 0])), MP.mpf(float(dc[s, 1])), MP.mpf(float(dc[s, 2]))
        theta = MP.atan2(MP.sqrt(x * x + y * y), z)
        phi = MP.atan2(x, y)
        if phi < 0:
            phi += two_pi
        if phi >= two_pi:
            phi -= two_pi
        p, w = weights_at(nside, theta, phi)
        pix[s] = p
        wgt[s] = [_to_ld(v) for v in w]
    return pix, wgt


# ---- arithmetic, longdouble ---------------------------------------------------------------------------------------------------------
def log_table(beam, matrix):
    """table [npix, nchan] = sum over frequency of M * log10(beam), longdouble."""
    logb = NP.log10(NP.asarray(beam, dtype=NP.float64).astype(LD))
    m = NP.asarray(matrix, dtype=NP.float64).astype(LD)
    table = NP.zeros((logb.shape[0], m.shape[0]), dtype=LD)
    for j in range(m.shape[1]):
        table += logb[:, j:j + 1] * m[None, :, j]
    return table


def interpolate(pix, wgt, table):
    """work [n, ncol] = four-pixel sum of a longdouble table [npix, ncol]."""
    table = NP.asarray(table, dtype=LD)
    work = NP.zeros((pix.shape[0], table.shape[1]), dtype=LD)
    for k in range(4):
        work += table[pix[:, k]] * wgt[:, k:k + 1]
    return work


def finish(work):
    """Per-channel max(nanmax, 0) subtracted, 10 ** x; the double, the float32 rounding and the relative distance of the reference from the
    nearest float32 rounding midpoint."""
    colmax = NP.maximum(NP.nanmax(work, axis=0), LD(0))
    ref = NP.power(LD(10), work - colmax[None, :])
    f32 = ref.astype(NP.float32)
    up = NP.nextafter(f32, NP.float32(NP.inf)).astype(LD)
    dn = NP.nextafter(f32, NP.float32(-NP.inf)).astype(LD)
    f = f32.astype(LD)
    mid = NP.minimum(NP.abs(ref - (f + up) / 2), NP.abs(ref - (f + dn) / 2)) / ref
    return {'ref_ld': ref, 'ref': ref.astype(NP.float64), 'f32': f32, 'mid': mid.astype(NP.float64), 'work': work, 'colmax': colmax}


def reference(nside, dircos, beam, matrix, rows=None):
    """The reference beam of sources `dircos` [n, 3] (or, with `rows`, of the source list dircos[rows]: the geometry runs once per distinct
    direction) through beam [npix, nfreq] and M [nchan, nfreq]."""
    beam = NP.asarray(beam)
    assert beam.shape[0] == 12 * nside * nside
    pix, wgt = interpol(nside, dircos)
    work = interpolate(pix, wgt, log_table(beam, matrix))
    return finish(work if rows is None else work[rows])


def judge(got, res, delta=None):
    """The acceptance rule.  got == float32(reference) bit for bit, except where the reference lies within `delta` (relative) of a float32
    rounding midpoint: there one float32 ulp either way is allowed.  Returns (failed, excused, worst): the number of elements that break the
    rule, the number that needed the exception, and the largest |got / reference - 1|."""
    delta = DELTA if delta is None else delta
    got = NP.asarray(got, dtype=NP.float64)
    g32 = got.astype(NP.float32)
    exact32 = g32.astype(NP.float64) == got                  # the beam is stored as float32: anything else is wrong outright
    f32 = res['f32']
    same = g32 == f32
    one_ulp = (g32 == NP.nextafter(f32, NP.float32(NP.inf))) | (g32 == NP.nextafter(f32, NP.float32(-NP.inf)))
    excused = ~same & one_ulp & (res['mid'] <= delta) & exact32
    failed = ~((same & exact32) | excused)
    worst = float(NP.max(NP.abs(got.astype(LD) / res['ref_ld'] - 1)))
    return int(failed.sum()), int(excused.sum()), worst


# ---- seeded inputs ------------------------------------------------------------------------------------------------------------------
def rough_beam(nside, nfreq=3, seed=0):
    """log10(beam) uniform in [-3, 0] per pixel and plane: a wrong pixel or weight shows at full size."""
    rng = NP.random.default_rng(1000 * nside + seed)
    return 10.0 ** rng.uniform(-3.0, 0.0, (12 * nside * nside, nfreq))


def matrix_5x3(seed=5):
    rng = NP.random.default_rng(seed)
    m = NP.zeros((5, 3))
    m[0] = [0.0, 1.0, 0.0]                                   # picks a plane
    m[1] = -rng.uniform(0.1, 0.4, 3)                         # log10(beam) <= 0: the column maximum is positive, the clamp is not taken
    m[2] = [1.2, 0.0, -0.2]                                  # a negative weight and an exact zero (the m != 0 skip)
    m[3] = 0.0                                               # beam exactly 1 everywhere
    m[4] = rng.uniform(-0.5, 1.5, 3)
    return m


def _unit(z, phi):
    z, phi = NP.broadcast_arrays(NP.asarray(z, dtype=NP.float64), NP.asarray(phi, dtype=NP.float64))
    s = NP.sqrt((1.0 - z) * (1.0 + z))
    return NP.stack((s * NP.sin(phi), s * NP.cos(phi), z), axis=-1).reshape(-1, 3)


def _ring_z(nside, ir):
    north = min(ir, 4 * nside - ir)
    z = 1.0 - north * north / (3.0 * nside * nside) if north < nside else 2.0 * (2 * nside - north) / (3.0 * nside)
    return z if ir <= 2 * nside else -z


def random_directions(n=1500, seed=77):
    """Seeded directions over the whole sphere (the entry does not refuse the lower hemisphere)."""
    rng = NP.random.default_rng(seed)
    return _unit(rng.uniform(-1.0, 1.0, n), rng.uniform(0.0, 2 * NP.pi, n))


def edge_directions(nside, seed=11):
    """The direction set of one nside, as direction cosines (the doubles are the input):
    every pixel centre (nside 64: of the rings RINGS_64); on each of those ring latitudes, one ulp of z either side of it and midway to the
    next ring -- the four cardinal azimuths, x = +-k 2^-53 y (k = 1 .. 8: the issue's survey counted to 8, its plan asks for 1 .. 4), six
    seeded azimuths and, for nside <= 3, every pixel boundary and centre of the ring +-1 ulp; zenith angle 0, 1e-12, 1e-8, 1e-5, 1e-3 from
    both poles at four azimuths; |z| = 2/3 at the nearest double, +-1 ulp, +-1e-9 in both hemispheres; 1500 seeded directions."""
    rng = NP.random.default_rng(100 * nside + seed)
    rings = [r for r in (RINGS_64 if nside == 64 else range(1, 4 * nside))]
    out = []
    for ir in rings:
        north = min(ir, 4 * nside - ir)
        nr = 4 * north if north < nside else 4 * nside
        shift = 1 if north < nside else 1 - (north - nside) % 2
        z0 = _ring_z(nside, ir)
        out.append(_unit(z0, (NP.arange(nr) + 0.5 * shift) * (2 * NP.pi / nr)))                     # pixel centres
        t0 = NP.arccos(z0)
        t1 = NP.arccos(_ring_z(nside, ir + 1)) if ir + 1 < 4 * nside else NP.pi
        for z in (z0, NP.nextafter(z0, 2.0), NP.nextafter(z0, -2.0), NP.cos(0.5 * (t0 + t1))):
            s = NP.sqrt((1.0 - z) * (1.0 + z))
            out.append(NP.array([[0.0, s, z], [s, 0.0, z], [0.0, -s, z], [-s, 0.0, z]]))
            for y in (s, -s):
                out.append(NP.array([[sg * k * 2.0 ** -53 * y, y, z] for k in range(1, 9) for sg in (1.0, -1.0)]))
            out.append(_unit(z, rng.uniform(0.0, 2 * NP.pi, 6)))
            if nside <= 3:
                edges = NP.arange(2 * nr + 1) * (NP.pi / nr)                                         # boundaries and centres, 0 .. 2 pi
                out.append(_unit(z, NP.concatenate((edges, NP.nextafter(edges, 10.0), NP.nextafter(edges, -10.0)))))
    for t in (0.0, 1e-12, 1e-8, 1e-5, 1e-3):
        for a in (0.3, 1.9, 3.5, 5.1):
            for sg in (1.0, -1.0):
                out.append(NP.array([[NP.sin(t) * NP.sin(a), NP.sin(t) * NP.cos(a), sg * NP.cos(t)]]))
    z23 = 2.0 / 3.0
    for z in (z23, NP.nextafter(z23, 1.0), NP.nextafter(z23, 0.0), z23 + 1e-9, z23 - 1e-9):
        phis = NP.concatenate(([0.0, 0.5 * NP.pi, NP.pi, 1.5 * NP.pi], rng.uniform(0.0, 2 * NP.pi, 6)))
        out.append(_unit(z, phis))
        out.append(_unit(-z, phis))
    out.append(random_directions())
    return NP.ascontiguousarray(NP.concatenate(out, axis=0))


@functools.lru_cache(maxsize=None)
def case_nside(nside):
    """(dircos, beam, M, reference) of the edge case of one nside; computed once per process."""
    dc, beam, m = edge_directions(nside), rough_beam(nside), matrix_5x3()
    return dc, beam, m, reference(nside, dc, beam, m)


@functools.lru_cache(maxsize=None)
def case_wide():
    """nside 2, 257 channels through a seeded 257 x 4 matrix, 300 of the random directions."""
    rng = NP.random.default_rng(257)
    dc, beam, m = random_directions()[:300], rough_beam(2, nfreq=4, seed=3), rng.uniform(-0.5, 1.5, (257, 4))
    return dc, beam, m, reference(2, dc, beam, m)


@functools.lru_cache(maxsize=None)
def case_many(target_row):
    """16384 + 37 rows drawn with replacement from the nside-8 set, three channels whose column maximum is positive; the source on the
    centre of the pixel that holds channel 0's largest table value appears at `target_row` only (a negative row counts from the end).
    Returns (dircos [nsrc, 3], beam, M, reference, target_row)."""
    nside, nsrc = 8, 16384 + 37
    target_row %= nsrc
    distinct, beam = edge_directions(nside), rough_beam(nside)
    m = NP.array([[-1.0, 0.0, 0.0], [-0.5, 0.0, -0.5], [0.0, -0.25, -0.75]])
    pmax = int(NP.argmax(log_table(beam, m)[:, 0]))
    ir = next(r for r in range(1, 4 * nside) if ring(nside, r)[0] <= pmax < ring(nside, r)[0] + ring(nside, r)[1])
    start, nr, _, shift = ring(nside, ir)
    centre = _unit(_ring_z(nside, ir), (pmax - start + 0.5 * shift) * (2 * NP.pi / nr))
    near = NP.flatnonzero(NP.max(NP.abs(distinct - centre), axis=1) < 1e-9)       # the set's own copy of that centre stays out of the draw
    pool = NP.setdiff1d(NP.arange(distinct.shape[0]), near)
    rows = NP.random.default_rng(16384).choice(pool, nsrc)
    distinct = NP.concatenate((distinct, centre), axis=0)
    rows[target_row] = distinct.shape[0] - 1
    res = reference(nside, distinct, beam, m, rows=rows)
    return NP.ascontiguousarray(distinct[rows]), beam, m, res, target_row
