"""CPU: the step-phase bound of prisim_amd/csrc/step_bound.h, which decides the baseline groups (of 256) that run the leapfrog rotation:
    step = min(maxlen dmax, maxh hmax + maxz zmax) |df| / c   cycles,   flagged when step <= 1/8 (fp32) or 1/4 (fp64), times 1 - 1e-9
with maxlen / maxh / maxz the group's largest |b|, |b_xy|, |b_z| and dmax / hmax / zmax the sky's largest |e|, |e_xy|, |e_z|, e = s - s_pc.
The header is host-only: a stand-alone program around it is built with -fsanitize=address,undefined and run on every case (nothing
loaded into Python is sanitised).  Checked: the bound is at least the brute-force largest step max_{b, s} |b . e| |df| / c of the group, at
most the whole-vector bound maxlen dmax |df| / c it replaces, and the flags equal a numpy statement of the rule; and the counts on the
headline workload (config 3, folded: 29 -> 39 of 43 groups)."""
import os
import shutil
import subprocess

import numpy as NP
import pytest

from prisim_amd import workloads as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = 299792458.0
# |b . e| is compared with a bound formed by two products, a sum, a product and a quotient in float64, each within 2^-53 relative, and with
# extrema that went through a square and a square root: a handful of ulps.  1e-13 relative covers them with room.
ROUNDING = 1e-13


@pytest.fixture(scope='module')
def bound_exe(tmp_path_factory):
    gxx = shutil.which('g++')
    assert gxx, 'g++ is needed to build the step-bound driver'
    exe = tmp_path_factory.mktemp('stepbound') / 'step_bound_main'
    subprocess.check_call([gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-Wall', '-Werror',
                           '-I', os.path.join(ROOT, 'prisim_amd', 'csrc'), os.path.join(ROOT, 'tests', 'step_bound_main.cpp'),
                           '-o', str(exe)])
    return str(exe)


def group_tables(bl):
    """(maxlen, maxh, maxz) per group of 256 rows, as prisim_hip_set_array forms them"""
    bl = NP.asarray(bl, dtype=NP.float64).reshape(-1, 3)
    ng = (bl.shape[0] + 255) // 256
    length = NP.sqrt(bl[:, 0] * bl[:, 0] + bl[:, 1] * bl[:, 1] + bl[:, 2] * bl[:, 2])
    hor = NP.sqrt(bl[:, 0] * bl[:, 0] + bl[:, 1] * bl[:, 1])
    az = NP.abs(bl[:, 2])
    return NP.array([[v[g * 256:(g + 1) * 256].max() for v in (length, hor, az)] for g in range(ng)])


def sky_extrema(dc, pc):
    """(dmax, hmax, zmax) as the library's upload loop forms them: square roots of the largest squares"""
    e = NP.asarray(dc, dtype=NP.float64) - NP.asarray(pc, dtype=NP.float64)[None, :]
    h2 = e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]
    z2 = e[:, 2] * e[:, 2]
    return float(NP.sqrt((h2 + z2).max())), float(NP.sqrt(h2.max())), float(NP.sqrt(z2.max()))


def numpy_rule(tab, ext, df, f32):
    whole = tab[:, 0] * ext[0]
    axes = tab[:, 1] * ext[1] + tab[:, 2] * ext[2]
    step = NP.minimum(whole, axes) * abs(df) / C
    return step, step <= (0.125 if f32 else 0.25) * (1.0 - 1e-9)


def run_bound(exe, tab, ext, df, f32, tmp_path):
    path = tmp_path / 'groups.f64'
    NP.concatenate((NP.array([ext[0], ext[1], ext[2], df, 1.0 if f32 else 0.0]), NP.asarray(tab, dtype=NP.float64).ravel())).tofile(str(path))
    res = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and not res.stderr, (res.returncode, res.stderr[-2000:])
    vals = NP.array(res.stdout.split(), dtype=NP.float64).reshape(-1, 2)
    assert vals.shape[0] == tab.shape[0]
    return vals[:, 0], vals[:, 1] != 0.0


def check(exe, bl, dc, pc, df, tmp_path):
    """the three properties, in both precisions; returns the fp32 flags"""
    bl = NP.asarray(bl, dtype=NP.float64).reshape(-1, 3)
    tab, ext = group_tables(bl), sky_extrema(dc, pc)
    e = NP.asarray(dc) - NP.asarray(pc)[None, :]
    dots = NP.abs(bl @ e.T).max(axis=1)
    brute = NP.array([dots[g * 256:(g + 1) * 256].max() for g in range(tab.shape[0])]) * abs(df) / C
    old = tab[:, 0] * ext[0] * abs(df) / C
    out = None
    for f32 in (True, False):
        step, flags = run_bound(exe, tab, ext, df, f32, tmp_path)
        step_np, flags_np = numpy_rule(tab, ext, df, f32)
        assert NP.array_equal(step, step_np), NP.max(NP.abs(step - step_np))
        assert NP.array_equal(flags, flags_np)
        assert NP.all(step * (1.0 + ROUNDING) >= brute), (step, brute)
        assert NP.all(step <= old * (1.0 + ROUNDING)), (step, old)
        if f32:
            out = flags
    return out


def random_sky(rng, nsrc, alt_min_deg=10.0):
    sin_alt = rng.uniform(NP.sin(NP.radians(alt_min_deg)), 1.0, nsrc)
    az = rng.uniform(0.0, 2 * NP.pi, nsrc)
    ca = NP.sqrt(1.0 - sin_alt * sin_alt)
    return NP.stack((ca * NP.sin(az), ca * NP.cos(az), sin_alt), axis=1)


def sorted_array(rng, nbl, scale, zscale):
    bl = rng.normal(0.0, 1.0, (nbl, 3)) * NP.array([scale, scale, zscale])
    return bl[NP.argsort(NP.linalg.norm(bl, axis=1))]


ZEN = NP.array([0.0, 0.0, 1.0])


@pytest.mark.parametrize('seed', [1, 2, 3])
def test_planar_arrays(bound_exe, tmp_path, seed):
    rng = NP.random.default_rng(seed)
    bl = sorted_array(rng, 1500, 150.0, 0.0)
    flags = check(bound_exe, bl, random_sky(rng, 200), ZEN, 97656.25, tmp_path)
    assert flags.any() and not flags.all()             # the cases do straddle the limit


@pytest.mark.parametrize('seed', [4, 5])
def test_tilted_arrays(bound_exe, tmp_path, seed):
    """a plane tilted by 20 degrees, and a cloud with as much height as width: the whole-vector bound is then often the smaller one"""
    rng = NP.random.default_rng(seed)
    t = NP.radians(20.0)
    rot = NP.array([[1.0, 0.0, 0.0], [0.0, NP.cos(t), -NP.sin(t)], [0.0, NP.sin(t), NP.cos(t)]])
    whole_wins = False
    for bl in (sorted_array(rng, 1100, 150.0, 0.0) @ rot.T, sorted_array(rng, 1100, 120.0, 120.0)):
        dc = random_sky(rng, 150)
        tab, ext = group_tables(bl), sky_extrema(dc, ZEN)
        check(bound_exe, bl, dc, ZEN, 97656.25, tmp_path)
        whole_wins = whole_wins or bool(NP.any(tab[:, 0] * ext[0] < tab[:, 1] * ext[1] + tab[:, 2] * ext[2]))
    assert whole_wins                                   # min() does pick the whole-vector term somewhere


def test_purely_vertical_baselines(bound_exe, tmp_path):
    rng = NP.random.default_rng(6)
    bl = NP.zeros((700, 3))
    bl[:, 2] = NP.sort(rng.uniform(0.0, 900.0, 700))
    dc = random_sky(rng, 120)
    flags = check(bound_exe, bl, dc, ZEN, 97656.25, tmp_path)
    tab, ext = group_tables(bl), sky_extrema(dc, ZEN)
    assert NP.all(tab[:, 1] == 0.0)
    assert NP.array_equal(flags, tab[:, 2] * ext[2] * 97656.25 / C <= 0.125 * (1.0 - 1e-9))     # the vertical term alone decides
    assert flags.any() and not flags.all()


def test_one_source_at_the_phase_centre(bound_exe, tmp_path):
    rng = NP.random.default_rng(7)
    pc = NP.array([0.3, -0.2, NP.sqrt(1.0 - 0.13)])
    bl = sorted_array(rng, 600, 5000.0, 300.0)
    flags = check(bound_exe, bl, pc[None, :], pc, 97656.25, tmp_path)
    assert flags.all()                                  # every step is zero


@pytest.mark.parametrize('seed', [8, 9])
def test_phase_centre_off_the_zenith(bound_exe, tmp_path, seed):
    rng = NP.random.default_rng(seed)
    alt, az = NP.radians(55.0), NP.radians(200.0 + 30.0 * seed)
    pc = NP.array([NP.cos(alt) * NP.sin(az), NP.cos(alt) * NP.cos(az), NP.sin(alt)])
    dc = random_sky(rng, 180)
    bl = sorted_array(rng, 1300, 140.0, 2.0)
    flags = check(bound_exe, bl, dc, pc, -97656.25, tmp_path)         # (a descending channel grid: |df| enters)
    assert flags.any() and not flags.all()
    # the extrema are taken about the phase centre: about the zenith they differ
    assert sky_extrema(dc, pc) != sky_extrema(dc, ZEN)


def fold_order(bl):
    """distinct baseline vectors in order of first appearance (-0.0 == +0.0), as baseline_fold.h lists them"""
    b = NP.asarray(bl, dtype=NP.float64).reshape(-1, 3) + 0.0
    _, first = NP.unique(b, axis=0, return_index=True)
    return b[NP.sort(first)]


def test_headline_counts(bound_exe, tmp_path):
    """config 3 as the benchmark runs it: 10 999 distinct vectors in 43 groups; 29 pass the whole-vector rule, 39 the per-axis rule,
    which is all the exact per-row maximum allows"""
    cfg = W.config3()
    ch = cfg['channels']
    df = float(ch[1] - ch[0])
    assert df == 97656.25
    bl = fold_order(cfg['baselines'])
    assert bl.shape[0] == 10999
    dc = cfg['sky']['dircos']
    tab, ext = group_tables(bl), sky_extrema(dc, ZEN)
    assert tab.shape[0] == 43 and NP.all(tab[:, 2] == 0.0)
    assert abs(ext[0] - 1.2856) < 1e-4 and abs(ext[1] - 0.9848) < 1e-4 and abs(ext[2] - 0.8263) < 1e-4, ext
    limit = 0.125 * (1.0 - 1e-9)
    assert int(NP.sum(tab[:, 0] * ext[0] * df / C <= limit)) == 29
    flags = check(bound_exe, bl, dc, ZEN, df, tmp_path)
    assert int(flags.sum()) == 39 and NP.all(flags[:39]) and not NP.any(flags[39:])
    e = dc - ZEN[None, :]
    exact = NP.array([NP.abs(bl[g * 256:(g + 1) * 256] @ e.T).max() for g in range(43)]) * df / C
    assert int(NP.sum(exact <= limit)) == 39
    # fp64: the 1/4-cycle limit admits every group under either rule
    _, flags64 = run_bound(bound_exe, tab, ext, df, False, tmp_path)
    assert flags64.all() and NP.all(tab[:, 0] * ext[0] * df / C <= 0.25 * (1.0 - 1e-9))
