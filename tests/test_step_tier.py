"""CPU: the second tier of the step flag (prisim_amd/csrc/step_bound.h: step_tier).  A baseline group of 256 whose step bound
    step = min(maxlen dmax, maxh hmax + maxz zmax) |df| / c   cycles
exceeds the leapfrog's 1/8-cycle limit but not the WIDE limit (11/64 cycle, times 1 - 1e-9; fp32 only) is tier 2 and runs the
leapfrog with a sine rounded once from fp64; tier 1 is exactly what step_flag says, tier 0 the plain rotation.  The header is host-only: a
stand-alone program around it is built with -fsanitize=address,undefined and run on every case (nothing loaded into Python is sanitised).
Checked on planar, tilted and vertical arrays: the tiers equal a numpy statement of the rule bit for bit, tier 1 holds exactly where
step_flag is true, tier 2 implies that the brute-force largest step max_{b, s} |b . e| |df| / c of the group is within the wide limit;
and the counts on the headline workload (config 3, folded): 39 groups of tier 1 and 3 of tier 2 of 43.

The geometry helpers are those of test_step_bound.py."""
import os
import shutil
import subprocess
import sys

import numpy as NP
import pytest

from prisim_amd import workloads as W

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_step_bound as SB                                   # noqa: E402

ROOT = SB.ROOT
C = SB.C
ZEN = SB.ZEN
WIDE_64THS = 11                                               # step_bound.h: kStepWideCycles, measured (profiles/LOG.md 4.1.10)
STRICT = 0.125 * (1.0 - 1e-9)
WIDE = WIDE_64THS / 64.0 * (1.0 - 1e-9)


@pytest.fixture(scope='module')
def tier_exe(tmp_path_factory):
    gxx = shutil.which('g++')
    assert gxx, 'g++ is needed to build the step-tier driver'
    exe = tmp_path_factory.mktemp('steptier') / 'step_tier_main'
    subprocess.check_call([gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-Wall', '-Werror',
                           '-I', os.path.join(ROOT, 'prisim_amd', 'csrc'), os.path.join(ROOT, 'tests', 'step_tier_main.cpp'),
                           '-o', str(exe)])
    return str(exe)


def numpy_tiers(tab, ext, df, f32):
    step, _ = SB.numpy_rule(tab, ext, df, f32)
    strict = step <= (0.125 if f32 else 0.25) * (1.0 - 1e-9)
    wide = (step <= WIDE) & f32
    return step, NP.where(strict, 1, NP.where(wide, 2, 0))


def run_tiers(exe, tab, ext, df, f32, tmp_path):
    path = tmp_path / 'groups.f64'
    NP.concatenate((NP.array([ext[0], ext[1], ext[2], df, 1.0 if f32 else 0.0]), NP.asarray(tab, dtype=NP.float64).ravel())).tofile(str(path))
    res = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and not res.stderr, (res.returncode, res.stderr[-2000:])
    words = res.stdout.split()
    assert float(words[0]) == WIDE, (words[0], WIDE)                      # the header's constant is the one restated here
    vals = NP.array(words[1:], dtype=NP.float64).reshape(-1, 3)
    assert vals.shape[0] == tab.shape[0]
    return vals[:, 0], vals[:, 1] != 0.0, vals[:, 2].astype(int)


def check(exe, bl, dc, pc, df, tmp_path):
    """the three properties, in both precisions; returns the fp32 tiers"""
    bl = NP.asarray(bl, dtype=NP.float64).reshape(-1, 3)
    tab, ext = SB.group_tables(bl), SB.sky_extrema(dc, pc)
    e = NP.asarray(dc) - NP.asarray(pc)[None, :]
    dots = NP.abs(bl @ e.T).max(axis=1)
    brute = NP.array([dots[g * 256:(g + 1) * 256].max() for g in range(tab.shape[0])]) * abs(df) / C
    out = None
    for f32 in (True, False):
        step, flags, tiers = run_tiers(exe, tab, ext, df, f32, tmp_path)
        step_np, tiers_np = numpy_tiers(tab, ext, df, f32)
        assert NP.array_equal(step, step_np)
        assert NP.array_equal(tiers, tiers_np), (tiers, tiers_np)
        assert NP.array_equal(tiers == 1, flags)                          # tier 1 exactly where step_flag is true
        assert NP.all(brute[tiers == 2] <= WIDE * (1.0 + SB.ROUNDING)), (brute, tiers)
        if f32:
            out = tiers
        else:
            assert not NP.any(tiers == 2)                                 # the wide tier exists in fp32 only
    return out


def uniform_array(rng, nbl, lmax, zscale=0.0):
    """baselines of lengths spread evenly up to lmax in random horizontal directions (heights ~ zscale), sorted by length: the groups'
    bounds climb steadily through both limits"""
    r = NP.sort(rng.uniform(0.0, lmax, nbl))
    a = rng.uniform(0.0, 2 * NP.pi, nbl)
    return NP.stack((r * NP.cos(a), r * NP.sin(a), rng.normal(0.0, 1.0, nbl) * zscale), axis=1)


@pytest.mark.parametrize('seed', [1, 2, 3])
def test_planar_arrays(tier_exe, tmp_path, seed):
    rng = NP.random.default_rng(seed)
    bl = uniform_array(rng, 1500, 700.0)
    tiers = check(tier_exe, bl, SB.random_sky(rng, 200), ZEN, 97656.25, tmp_path)
    assert set(tiers.tolist()) == {0, 1, 2}, tiers                        # the cases do straddle both limits


@pytest.mark.parametrize('seed', [4, 5])
def test_tilted_arrays(tier_exe, tmp_path, seed):
    rng = NP.random.default_rng(seed)
    t = NP.radians(20.0)
    rot = NP.array([[1.0, 0.0, 0.0], [0.0, NP.cos(t), -NP.sin(t)], [0.0, NP.sin(t), NP.cos(t)]])
    seen = set()
    for bl in (uniform_array(rng, 1500, 700.0) @ rot.T, SB.sorted_array(rng, 1100, 120.0, 120.0)):
        seen |= set(check(tier_exe, bl, SB.random_sky(rng, 150), ZEN, 97656.25, tmp_path).tolist())
    assert seen == {0, 1, 2}, seen


def test_purely_vertical_baselines(tier_exe, tmp_path):
    rng = NP.random.default_rng(6)
    bl = NP.zeros((2000, 3))
    bl[:, 2] = NP.sort(rng.uniform(0.0, 900.0, 2000))
    dc = SB.random_sky(rng, 120)
    tiers = check(tier_exe, bl, dc, ZEN, 97656.25, tmp_path)
    tab, ext = SB.group_tables(bl), SB.sky_extrema(dc, ZEN)
    step = tab[:, 2] * ext[2] * 97656.25 / C                             # the vertical term alone decides
    assert NP.array_equal(tiers, NP.where(step <= STRICT, 1, NP.where(step <= WIDE, 2, 0)))
    assert set(tiers.tolist()) == {0, 1, 2}, tiers


def test_descending_grid_off_the_zenith(tier_exe, tmp_path):
    rng = NP.random.default_rng(8)
    alt, az = NP.radians(55.0), NP.radians(240.0)
    pc = NP.array([NP.cos(alt) * NP.sin(az), NP.cos(alt) * NP.cos(az), NP.sin(alt)])
    tiers = check(tier_exe, SB.sorted_array(rng, 1300, 140.0, 2.0), SB.random_sky(rng, 180), pc, -97656.25, tmp_path)      # |df| enters
    assert (tiers == 1).any() and (tiers != 1).any()


def test_headline_counts(tier_exe, tmp_path):
    """config 3 as the benchmark runs it: 43 groups of distinct vectors; 39 of tier 1 (test_step_bound.py); the bounds of the last four are
    0.1256, 0.1292, 0.1338 and 0.1867 cycle, so three of them are tier 2 and the last stays tier 0"""
    cfg = W.config3()
    ch = cfg['channels']
    df = float(ch[1] - ch[0])
    bl = SB.fold_order(cfg['baselines'])
    dc = cfg['sky']['dircos']
    tab, ext = SB.group_tables(bl), SB.sky_extrema(dc, ZEN)
    assert tab.shape[0] == 43
    step, _ = SB.numpy_rule(tab, ext, df, True)
    assert NP.allclose(step[39:], [0.1256, 0.1292, 0.1338, 0.1867], atol=5e-5), step[39:]
    tiers = check(tier_exe, bl, dc, ZEN, df, tmp_path)
    assert NP.all(tiers[:39] == 1)
    assert 0.1338 <= WIDE < 0.1867                                       # the limit admits groups 39-41 and leaves the outriggers' group plain
    assert int(NP.sum(tiers == 1)) == 39 and int(NP.sum(tiers == 2)) == 3
    assert NP.all(tiers[39:42] == 2) and tiers[42] == 0, tiers
