"""The 40-digit reference of the external HEALPix beam (tests/extbeam_reference.py): known answers that do not come from its own
algorithm, and the fp64 restatement oracle/healpix_oracle.py held against it on the edge direction sets the device is held to."""
import numpy as NP
import pytest

import extbeam_reference as R
from oracle import healpix_oracle as H

MP, LD = R.MP, R.LD


def _ring_theta(nside, ir):
    """Colatitude of ring ir from Gorski et al. 2005 eqs. 4 and 8, written out again here."""
    north = min(ir, 4 * nside - ir)
    z = 1 - MP.mpf(north) ** 2 / (3 * nside ** 2) if north < nside else MP.mpf(4) / 3 - MP.mpf(2 * north) / (3 * nside)
    return MP.acos(z) if ir <= 2 * nside else MP.pi - MP.acos(z)


def _ring_of_pixel(nside):
    """ring index (1-based) of every RING pixel, from the ring lengths alone"""
    lengths = [4 * min(ir, 4 * nside - ir, nside) for ir in range(1, 4 * nside)]
    assert sum(lengths) == 12 * nside * nside
    return NP.repeat(NP.arange(1, 4 * nside), lengths)


def _value(nside, theta, phi, hmap):
    pix, wgt = R.weights_at(nside, MP.mpf(theta), MP.mpf(phi))
    return sum(w * MP.mpf(float(hmap[p])) for p, w in zip(pix, wgt))


@pytest.mark.parametrize('nside', [1, 2, 3, 8])
def test_pixel_centres_return_the_pixel(nside):
    """Centres from the closed forms, to 38 digits: the interpolation returns the pixel's own value."""
    hmap = NP.random.default_rng(nside).uniform(-3.0, 0.0, 12 * nside * nside)
    p = 0
    for ir in range(1, 4 * nside):
        north = min(ir, 4 * nside - ir)
        nr = 4 * min(north, nside)
        shifted = north < nside or (north - nside) % 2 == 0
        for j in range(nr):
            phi = (j + (MP.mpf(1) / 2 if shifted else 0)) * 2 * MP.pi / nr
            assert abs(_value(nside, _ring_theta(nside, ir), phi, hmap) - MP.mpf(float(hmap[p]))) <= MP.mpf(10) ** -36, (ir, j)
            p += 1
    assert p == 12 * nside * nside


@pytest.mark.parametrize('nside', R.NSIDES)
def test_constant_map_returns_the_constant(nside):
    dc = R.random_directions(200, seed=nside)
    pix, wgt = R.interpol(nside, dc)
    c = LD(-1.2345678901234567)
    got = R.interpolate(pix, wgt, NP.full((12 * nside * nside, 1), c, dtype=LD))
    assert float(NP.max(NP.abs(got / c - 1))) <= 1e-18


@pytest.mark.parametrize('nside', [1, 2, 3, 8])
def test_ring_map_is_piecewise_linear_in_theta_and_the_ring_mean_in_a_cap(nside):
    rng = NP.random.default_rng(40 + nside)
    f = rng.uniform(-3.0, 0.0, 4 * nside)                      # f[ir]
    hmap = f[_ring_of_pixel(nside)]
    for ir in range(1, 4 * nside - 1):
        t0, t1 = _ring_theta(nside, ir), _ring_theta(nside, ir + 1)
        for frac in (MP.mpf(1) / 7, MP.mpf(1) / 2, MP.mpf(9) / 10):
            for phi in (0, MP.mpf('0.7'), MP.mpf('4.1'), 2 * MP.pi - MP.mpf(10) ** -30):
                want = MP.mpf(float(f[ir])) * (1 - frac) + MP.mpf(float(f[ir + 1])) * frac
                assert abs(_value(nside, t0 + frac * (t1 - t0), phi, hmap) - want) <= MP.mpf(10) ** -36
    for theta, fr in ((_ring_theta(nside, 1) / 3, f[1]), (MP.pi - _ring_theta(nside, 1) / 3, f[4 * nside - 1])):
        assert abs(_value(nside, theta, MP.mpf('2.2'), hmap) - MP.mpf(float(fr))) <= MP.mpf(10) ** -36
    # any map: at the poles themselves, the mean of the four pixels of the first / last ring
    anymap = rng.uniform(-3.0, 0.0, 12 * nside * nside)
    for theta, four in ((MP.zero, anymap[:4]), (+MP.pi, anymap[-4:])):
        want = sum(MP.mpf(float(v)) for v in four) / 4
        assert abs(_value(nside, theta, MP.mpf('1.3'), anymap) - want) <= MP.mpf(10) ** -36


@pytest.mark.parametrize('nside', R.NSIDES)
def test_values_are_continuous_across_ring_latitudes_and_azimuth_zero(nside):
    rng = NP.random.default_rng(60 + nside)
    hmap = rng.uniform(-3.0, 0.0, 12 * nside * nside)
    eps = MP.mpf(10) ** -30
    rings = R.RINGS_64 if nside == 64 else range(1, 4 * nside)
    z23 = MP.acos(MP.mpf(2) / 3)
    lats = [_ring_theta(nside, ir) for ir in rings] + [z23, MP.pi - z23]
    for t in lats:
        for phi in (0, MP.mpf('0.9'), MP.mpf('3.3'), 2 * MP.pi - eps):
            assert abs(_value(nside, t - eps, phi, hmap) - _value(nside, t + eps, phi, hmap)) <= MP.mpf(10) ** -17
    for t in lats + [eps, MP.pi - eps] + [(_ring_theta(nside, ir) + _ring_theta(nside, ir + 1)) / 2 for ir in list(rings)[:-1:3]]:
        assert abs(_value(nside, t, eps, hmap) - _value(nside, t, 2 * MP.pi - eps, hmap)) <= MP.mpf(10) ** -17


def test_midpoint_distance_and_the_rule():
    """finish() on values placed by hand: a float32 value itself is half an ulp from its midpoints; a midpoint is at distance 0 and only
    there does judge() allow the neighbour."""
    lo = NP.float32(0.5)
    up = NP.nextafter(lo, NP.float32(1))
    res = R.finish(NP.log10(NP.array([[LD(lo)], [(LD(lo) + LD(up)) / 2], [LD(up)]], dtype=LD)))      # all below 1: colmax = 0
    assert res['mid'][1, 0] <= 1e-18 and abs(res['mid'][0, 0] - 2.0 ** -25) <= 1e-12
    assert res['f32'][0, 0] == lo and res['f32'][2, 0] == up and res['f32'][1, 0] in (lo, up)
    f = res['f32'].astype(NP.float64)
    assert R.judge(f, res)[:2] == (0, 0)
    nudged = f.copy()
    nudged[1, 0] = float(up if res['f32'][1, 0] == lo else lo)
    assert R.judge(nudged, res)[:2] == (0, 1)
    nudged = f.copy()
    nudged[0, 0] = float(up)
    assert R.judge(nudged, res)[:2] == (1, 0)
    assert R.judge(f * (1 + 1e-12), res)[0] == f.size                       # not a float32 value at all


# ---- the fp64 restatement against the reference -------------------------------------------------------------------------------------
def _twin(dc, beam, m):
    """oracle/healpix_oracle.py fed what the device gets: theta = atan2(hypot(x, y), z), phi = atan2(x, y); 10 ** work in fp64."""
    theta = NP.arctan2(NP.hypot(dc[:, 0], dc[:, 1]), dc[:, 2])
    phi = NP.arctan2(dc[:, 0], dc[:, 1])
    work = H.get_interp_val(NP.log10(beam) @ m.T, theta, phi)
    return H.normalise_logbeam(work, quantise_f32=False)


def _cases():
    for nside in R.NSIDES:
        yield 'nside %d' % nside, R.case_nside(nside)
    yield 'wide', R.case_wide()
    yield 'many, last row', R.case_many(-1)[:4]
    yield 'many, row 16384', R.case_many(16384)[:4]


@pytest.fixture(scope='module')
def twin_runs():
    return [(name, c[3], _twin(c[0], c[1], c[2])) for name, c in _cases()]


def test_inputs_leave_no_float32_subnormals_and_take_every_branch():
    for name, (dc, beam, m, res) in _cases():
        assert float(NP.min(res['ref'])) >= 1e-30, name
    res = R.case_nside(8)[3]
    assert res['colmax'][1] > 0 and res['colmax'][0] == 0 and NP.all(res['ref'][:, 3] == 1.0)
    for row in (-1, 16384):
        dc, beam, m, res, target = R.case_many(row)
        assert dc.shape == (16384 + 37, 3) and target in (16384, 16384 + 36)
        assert int(NP.argmax(res['work'][:, 0])) == target and NP.sum(res['work'][:, 0] == res['work'][target, 0]) == 1
        assert res['ref'][target, 0] == 1.0 and NP.all(res['colmax'] > 0)


def test_restatement_against_the_reference(twin_runs):
    """Every element of the fp64 restatement, rounded to float32, is the reference's float32 bit for bit or excused by the rule; at most
    1e-3 of a case excused."""
    for name, res, pb in twin_runs:
        failed, excused, worst = R.judge(pb.astype(NP.float32).astype(NP.float64), res)
        print('%-16s %6d x %3d  failed %d  excused %d  worst fp64 deviation %.3e' % (name, pb.shape[0], pb.shape[1], failed, excused, worst))
        assert failed == 0, name
        assert excused <= R.EXCUSED_SHARE * pb.size, name


def test_floor_of_the_restatement(twin_runs):
    """The largest relative deviation of the restatement's 10 ** work from the reference: DELTA is 8 x this floor."""
    floor = 0.0
    for name, res, pb in twin_runs:
        dev = float(NP.max(NP.abs(pb.astype(LD) / res['ref_ld'] - 1)))
        print('%-16s floor %.3e' % (name, dev))
        floor = max(floor, dev)
    print('floor %.3e   DELTA %.3e' % (floor, R.DELTA))
    assert floor <= R.DELTA / 8
