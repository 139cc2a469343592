"""GPU (-m gpu): the wide tier of the fp32 leapfrog (step_bound.h: step_tier; skyvis_kernels.hip: the WIDE body of the packed fp32 kernel).
A baseline group of 256 whose step bound lies beyond 1/8 cycle but within the wide limit WIDE runs the leapfrog with sin_2pi_y_wide; the
strict flag (<= 1/8 cycle) keeps the present body and everything beyond WIDE the plain rotation.  All cases: 64-channel tiles, 128 channels,
64-300 sources, parity with the fp64 C oracle at the project's fp32 tolerance, 5e-6 of S_f = sum_s |pbflux[s, f]|, and the counts the library
reports (last_sum_lift_groups: tier 1, last_sum_wide_groups: tier 2).  The arrays are built as in test_gpu_step_bound.py: the longest
baseline of a group lies along the horizontal part of e = s - s_pc of the source with the largest horizontal offset (10 degrees altitude),
so that source's step sits AT the group's bound.

The limit itself was chosen by the single-source sweep of profiles/LOG.md 4.1.10 (half the tolerance, 2.5e-6, for ONE source carrying all
the flux); test_single_source_worst_case repeats that measurement at the limit and holds it to the project tolerance like every other case.
CPU-side checks of step_tier are in test_step_tier.py."""
import functools
import os
import subprocess
import sys

import numpy as NP
import pytest

from oracle import skyvis_oracle as O, c_oracle as CO
from prisim_amd import _abi, geometry as GEOM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL32 = 5e-6
C = 299792458.0
ZEN = NP.array([0.0, 0.0, 1.0])
F0, DF, NCHAN = 150e6, 1e5, 128
CH = F0 + DF * NP.arange(NCHAN)
ALT_MIN = 10.0
STRICT = 0.125 * (1.0 - 1e-9)
WIDE = 11.0 / 64.0 * (1.0 - 1e-9)                 # step_bound.h: step_wide_limit_cycles()


def relerr(v, ref, pb):
    return float(NP.max(NP.abs(v - ref) / O.abs_flux_sum(pb)[None, :]))


def sky_dircos(rng, nsrc, alt_min=ALT_MIN):
    """nsrc sources down to alt_min degrees altitude; source 0 at the zenith, source 1 AT alt_min (the largest horizontal offset)"""
    sin_alt = rng.uniform(NP.sin(NP.radians(alt_min + 2.0)), 1.0, nsrc)
    alt = NP.degrees(NP.arcsin(sin_alt))
    az = rng.uniform(0.0, 360.0, nsrc)
    alt[0], alt[1] = 90.0, alt_min
    return GEOM.altaz2dircos(NP.stack((alt, az), axis=1))


def pbflux(rng, nsrc):
    return rng.uniform(0.2, 2.0, (nsrc, NCHAN)) * (1.0 + 0.1 * NP.sin(NP.arange(NCHAN) / 7.0))[None, :]


def extreme_direction(dc, pc=ZEN):
    """(horizontal unit vector along e_xy of the source with the largest |e_xy|, that |e_xy|)"""
    e = dc - pc[None, :]
    hor = NP.hypot(e[:, 0], e[:, 1])
    s = int(NP.argmax(hor))
    return NP.array([e[s, 0], e[s, 1], 0.0]) / hor[s], float(hor[s])


def planar_group(rng, n, length, direction, rmin=0.05):
    """n horizontal baselines of rmin .. 0.99 `length` in random directions; the first is exactly `length` along `direction`"""
    a = rng.uniform(0.0, 2 * NP.pi, n)
    r = rng.uniform(rmin, 0.99, n) * length
    bl = NP.stack((r * NP.cos(a), r * NP.sin(a), NP.zeros(n)), axis=1)
    bl[0] = length * direction
    return bl


def planar_array(rng, dc, steps, n=256, sign=1.0):
    """one planar group per entry of `steps` whose step bound is steps[g] cycles, met by the source of the largest horizontal offset;
    sign = -1: every baseline reversed (that source's step is then -steps[g])"""
    direction, hor = extreme_direction(dc)
    return sign * NP.concatenate([planar_group(rng, n, st * C / (hor * DF), direction) for st in steps])


def aligned_group(rng, n, step, dc, sign=1.0):
    """n baselines ALONG the extreme direction, 0.98 .. 1 of the length whose step is `step`: every one of them is near the group's bound"""
    direction, hor = extreme_direction(dc)
    r = rng.uniform(0.98, 1.0, n)
    r[0] = 1.0
    return sign * (r * step * C / (hor * DF))[:, None] * direction[None, :]


def group_bounds(bl, dc, pc=ZEN):
    """per group of 256: (the step bound of step_bound.h, the brute-force largest step), in cycles"""
    e = dc - pc[None, :]
    h2, z2 = e[:, 0] ** 2 + e[:, 1] ** 2, e[:, 2] ** 2
    d, h, z = float(NP.sqrt((h2 + z2).max())), float(NP.sqrt(h2.max())), float(NP.sqrt(z2.max()))
    out = []
    for g in range((bl.shape[0] + 255) // 256):
        b = bl[g * 256:(g + 1) * 256]
        maxlen, maxh, maxz = NP.linalg.norm(b, axis=1).max(), NP.hypot(b[:, 0], b[:, 1]).max(), NP.abs(b[:, 2]).max()
        out.append((min(maxlen * d, maxh * h + maxz * z) * DF / C, NP.abs(b @ e.T).max() * DF / C))
    return NP.array(out)


def tiers(bl, dc, pc=ZEN):
    b = group_bounds(bl, dc, pc)[:, 0]
    return NP.where(b <= STRICT, 1, NP.where(b <= WIDE, 2, 0))


def run(ctx, bl, dc, pb, pc=ZEN, nsplit=1):
    ctx.set_array(bl, CH)
    ctx.set_tuning(64, 0, nsplit)
    try:
        out = ctx.skyvis(dc, pb, pc, precision=_abi.PRISIM_FP32, kernel=_abi.PRISIM_KERNEL_RECURRENCE)
        tm = ctx.timing()
        assert tm['last_chan_tile'] == 64 and tm['last_nsplit'] == nsplit, tm
        assert tm['wide_limit_cycles'] == WIDE, tm            # the library's limit is the one restated here
        return out, tm
    finally:
        ctx.set_tuning(0, 0, 0)


@functools.lru_cache(maxsize=None)
def three_tier_case(sign, nsrc=300, seed=31):
    """groups at 0.1249 cycle (tier 1), WIDE (1 - 1e-3) (tier 2) and WIDE (1 + 1e-3) (tier 0), and the oracle's V"""
    rng = NP.random.default_rng(seed)
    dc = sky_dircos(rng, nsrc)
    pb = pbflux(rng, nsrc)
    bl = planar_array(rng, dc, [0.1249, WIDE * (1.0 - 1e-3), WIDE * (1.0 + 1e-3)], sign=float(sign))
    ref = CO.skyvis(bl, CH, dc, pb, ZEN)
    for a in (dc, pb, bl, ref):
        a.setflags(write=False)
    return dc, pb, bl, ref


def test_three_tier_premise():
    """(no GPU work) the construction: the bounds are met by the brute-force step, and fall in tiers 1, 2, 0"""
    for sign in (1, -1):
        dc, _, bl, _ = three_tier_case(sign)
        b = group_bounds(bl, dc)
        assert NP.allclose(b[:, 0], [0.1249, WIDE * (1.0 - 1e-3), WIDE * (1.0 + 1e-3)], rtol=0, atol=1e-9), b
        assert NP.allclose(b[:, 0], b[:, 1], rtol=0, atol=1e-9), b
        assert tiers(bl, dc).tolist() == [1, 2, 0]
        e1 = dc[1] - ZEN
        assert NP.sign(bl[256] @ e1) == sign                  # the extreme source's step has the stated sign


@pytest.mark.parametrize('sign', [1, -1], ids=['positive', 'negative'])
@pytest.mark.parametrize('nsplit', [1, 3])
def test_three_tiers_in_one_launch(ctx, sign, nsplit):
    dc, pb, bl, ref = three_tier_case(sign)
    v, tm = run(ctx, bl, dc, pb, nsplit=nsplit)
    assert tm['last_sum_lift_groups'] == 1 and tm['last_sum_wide_groups'] == 1, tm
    errs = [relerr(v[g * 256:(g + 1) * 256], ref[g * 256:(g + 1) * 256], pb) for g in range(3)]
    print('three tiers, sign %+d, nsplit %d: err / S_f per group (strict, wide, plain) = %s' % (sign, nsplit, ' '.join('%.3e' % e for e in errs)))
    assert max(errs) <= TOL32, errs


def test_flush_every_64_sources(ctx, monkeypatch):
    """300 sources in segments of 64: five read-modify-write flushes of the fp32 partial sums into the fp64 cube"""
    dc, pb, bl, ref = three_tier_case(1)
    monkeypatch.setenv('PRISIM_HIP_FLUSH_SRC', '64')
    v, tm = run(ctx, bl, dc, pb)
    assert tm['last_sum_lift_groups'] == 1 and tm['last_sum_wide_groups'] == 1, tm
    err = relerr(v, ref, pb)
    print('flush every 64 sources: err / S_f = %.3e' % err)
    assert err <= TOL32, err


def test_single_source_worst_case(ctx):
    """One source carries all the flux, at the direction of the groups' largest step (10 degrees altitude; 63 more sources of zero flux
    keep the sky's extrema where they are); every baseline of both groups lies along that direction within 2 % of the bound, which is
    the wide limit; group 1 is group 0 reversed (negative steps).  The maximum is over baselines and channels."""
    rng = NP.random.default_rng(32)
    dc = sky_dircos(rng, 64)
    pb = NP.zeros((64, NCHAN))
    pb[1] = pbflux(rng, 1)[0]
    bound = WIDE * (1.0 - 1e-6)
    bl = NP.concatenate((aligned_group(rng, 256, bound, dc), aligned_group(rng, 256, bound, dc, sign=-1.0)))
    b = group_bounds(bl, dc)
    assert NP.allclose(b, bound, rtol=0, atol=1e-9) and tiers(bl, dc).tolist() == [2, 2], b
    v, tm = run(ctx, bl, dc, pb)
    assert tm['last_sum_lift_groups'] == 0 and tm['last_sum_wide_groups'] == 2, tm
    ref = CO.skyvis(bl, CH, dc, pb, ZEN)
    errs = [relerr(v[:256], ref[:256], pb), relerr(v[256:], ref[256:], pb)]
    print('single source at the wide limit: err / S_f = %.3e (positive steps) %.3e (negative steps)' % tuple(errs))
    assert max(errs) <= TOL32, errs


def test_folded_array_with_groups_in_different_tiers(ctx):
    """700 rows of 300 distinct vectors: the 256 + 44 summed rows form a strict group and a wide one"""
    rng = NP.random.default_rng(33)
    dc = sky_dircos(rng, 100)
    pb = pbflux(rng, 100)
    direction, hor = extreme_direction(dc)
    uniq = NP.concatenate((planar_group(rng, 256, 0.11 * C / (hor * DF), direction), planar_group(rng, 44, WIDE * (1.0 - 1e-3) * C / (hor * DF), direction)))
    rows = NP.concatenate((NP.arange(300), rng.integers(0, 300, 400)))      # (distinct vectors are listed in order of first appearance)
    bl = uniq[rows]
    assert tiers(uniq, dc).tolist() == [1, 2]
    v, tm = run(ctx, bl, dc, pb)
    assert tm['last_sum_baselines'] == 300, tm
    assert tm['last_sum_lift_groups'] == 1 and tm['last_sum_wide_groups'] == 1, tm
    vu = v[:300]
    assert NP.array_equal(v, vu[rows])
    err = relerr(vu, CO.skyvis(uniq, CH, dc, pb, ZEN), pb)
    print('folded 700 / 300: err / S_f = %.3e' % err)
    assert err <= TOL32, err


def test_zero_and_millimetre_baselines_beside_a_wide_group(ctx):
    """group 0: zero-length baselines (theta = 0 exactly) and millimetre ones; group 1 at the wide limit"""
    rng = NP.random.default_rng(34)
    dc = sky_dircos(rng, 64)
    pb = pbflux(rng, 64)
    g0 = planar_group(rng, 256, 3e-3, NP.array([1.0, 0.0, 0.0]))
    g0[::4] = 0.0
    bl = NP.concatenate((g0, planar_array(rng, dc, [WIDE * (1.0 - 1e-3)])))
    assert tiers(bl, dc).tolist() == [1, 2]
    v, tm = run(ctx, bl, dc, pb)
    assert tm['last_sum_lift_groups'] == 1 and tm['last_sum_wide_groups'] == 1, tm
    ref = CO.skyvis(bl, CH, dc, pb, ZEN)
    err = relerr(v, ref, pb)
    print('zero / millimetre group beside a wide one: err / S_f = %.3e' % err)
    assert err <= TOL32, err
    assert NP.allclose(v[0], pb.sum(axis=0), rtol=1e-6)      # a zero baseline sees the total flux


def test_cached_table_follows_the_sky(ctx):
    """Two skies on one resident array.  Under the first (sources down to 10 degrees altitude) group 0 is tier 2; the second reaches down
    to 5 degrees, its hmax is 1.2 % larger and the same group is tier 0.  The second result must be, bit for bit, what the second sky
    gives right after a fresh set_array (no cached table)."""
    rng = NP.random.default_rng(35)
    dc1 = sky_dircos(rng, 64)
    dc2 = dc1.copy()
    az = NP.degrees(NP.arctan2(dc1[1, 0], dc1[1, 1]))
    dc2[1] = GEOM.altaz2dircos(NP.array([[5.0, az]]))[0]
    pb = pbflux(rng, 64)
    bl = planar_array(rng, dc1, [WIDE * (1.0 - 1e-3), 0.05])
    assert tiers(bl, dc1).tolist() == [2, 1] and tiers(bl, dc2).tolist() == [0, 1]
    ctx.set_array(bl, CH)
    ctx.set_tuning(64, 0, 1)
    try:
        kw = dict(precision=_abi.PRISIM_FP32, kernel=_abi.PRISIM_KERNEL_RECURRENCE)
        v1 = ctx.skyvis(dc1, pb, ZEN, **kw)
        tm1 = ctx.timing()
        v2 = ctx.skyvis(dc2, pb, ZEN, **kw)
        tm2 = ctx.timing()
        ctx.set_array(bl, CH)
        v2_fresh = ctx.skyvis(dc2, pb, ZEN, **kw)
        v1_again = ctx.skyvis(dc1, pb, ZEN, **kw)
    finally:
        ctx.set_tuning(0, 0, 0)
    assert (tm1['last_sum_lift_groups'], tm1['last_sum_wide_groups']) == (1, 1), tm1
    assert (tm2['last_sum_lift_groups'], tm2['last_sum_wide_groups']) == (1, 0), tm2
    assert NP.array_equal(v2, v2_fresh) and NP.array_equal(v1, v1_again)
    errs = [relerr(v1, CO.skyvis(bl, CH, dc1, pb, ZEN), pb), relerr(v2, CO.skyvis(bl, CH, dc2, pb, ZEN), pb)]
    print('two skies on one array: err / S_f = %.3e (tier 2) %.3e (tier 0)' % tuple(errs))
    assert max(errs) <= TOL32, errs


_CHILD = r'''
import sys
import numpy as NP
from prisim_amd import _abi
d = NP.load(sys.argv[1])
with _abi.Context(0) as ctx:
    ctx.set_array(d['bl'], d['ch'])
    ctx.set_tuning(64, 0, 1)
    v = ctx.skyvis(d['dc'], d['pb'], d['pc'], precision=_abi.PRISIM_FP32, kernel=_abi.PRISIM_KERNEL_RECURRENCE)
    tm = ctx.timing()
NP.save(sys.argv[2], v)
print('TIERS %d %d %d' % (tm['last_chan_tile'], tm['last_sum_lift_groups'], tm['last_sum_wide_groups']))
'''


def test_hook_off_in_a_fresh_process(ctx, tmp_path):
    """PRISIM_HIP_WIDE_LEAPFROG=0 (read by set_array): no group is tier 2, the wide group runs the plain rotation -- within tolerance, and
    not the bits of the wide body"""
    dc, pb, bl, ref = three_tier_case(1)
    inp, outp = str(tmp_path / 'in.npz'), str(tmp_path / 'vis.npy')
    NP.savez(inp, bl=bl, ch=CH, dc=dc, pb=pb, pc=ZEN)
    env = dict(os.environ, PRISIM_HIP_WIDE_LEAPFROG='0', PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    res = subprocess.run([sys.executable, '-c', _CHILD, inp, outp], env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    line = [ln for ln in res.stdout.splitlines() if ln.startswith('TIERS')][-1].split()
    assert [int(x) for x in line[1:]] == [64, 1, 0], line
    off = NP.load(outp)
    err = relerr(off, ref, pb)
    print('hook off: err / S_f = %.3e' % err)
    assert err <= TOL32, err
    on, tm = run(ctx, bl, dc, pb)
    assert tm['last_sum_wide_groups'] == 1, tm
    assert NP.array_equal(on[:256], off[:256]) and NP.array_equal(on[512:], off[512:])      # tiers 1 and 0: the same bodies either way
    assert not NP.array_equal(on[256:512], off[256:512])
