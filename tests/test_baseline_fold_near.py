"""CPU: fold_baselines_near and choose_fold of prisim_amd/csrc/baseline_fold.h (rows whose baseline vectors are equal to rounding are
summed once, prisim_hip_set_array) against a numpy restatement of the rule:

    walk the rows in order; a row joins the earliest-founded cluster whose representative (the cluster's first row) is within tol of
    it in every component (|d| <= tol); otherwise it founds a cluster.  max_dev = the largest 2-norm |b - b_rep|.

The header is host-only: a stand-alone program around it is built with -fsanitize=address,undefined and run on every case (nothing loaded
into Python is sanitised).  The counts on the headline array (config 3 as the benchmark builds it) are those measured for it: 10 999
vectors distinct by IEEE value, 7 090 distinct to rounding, 28 groups of 256 of which 24 / 3 / 1 are step tiers 1 / 2 / 0."""
import math
import os
import shutil
import subprocess
import sys
import time

import numpy as NP
import pytest

from prisim_amd import layouts, sharding, workloads as W

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_step_bound as SB                                   # noqa: E402
import test_step_tier as ST                                    # noqa: E402
from test_step_tier import tier_exe                            # noqa: E402,F401  (the fixture that builds the step-tier driver)
from test_baseline_fold import numpy_fold                      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = 299792458.0
BUDGET = 1e-12                                                 # rad: a tenth of the fp64 tolerance of 1e-11
NONE, EXACT, NEAR = 0, 1, 2


@pytest.fixture(scope='module')
def near_exe(tmp_path_factory):
    gxx = shutil.which('g++')
    assert gxx, 'g++ is needed to build the fold-map driver'
    exe = tmp_path_factory.mktemp('foldnear') / 'baseline_fold_near_main'
    subprocess.check_call([gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-Wall', '-Werror',
                           '-I', os.path.join(ROOT, 'prisim_amd', 'csrc'), os.path.join(ROOT, 'tests', 'baseline_fold_near_main.cpp'),
                           '-o', str(exe)])
    return str(exe)


def run_near(exe, bl, tol, tmp_path, fmax=0.0, allow_near=True):
    """-> dict(rep, map, n_exact, kind, tol, max_dev, phase, seconds)"""
    bl = NP.ascontiguousarray(bl, dtype=NP.float64).reshape(-1, 3)
    path = tmp_path / 'bl.f64'
    bl.tofile(str(path))
    t0 = time.perf_counter()
    res = subprocess.run([exe, str(path), tol if isinstance(tol, str) else repr(float(tol)), repr(float(fmax)), '1' if allow_near else '0'],
                         capture_output=True, text=True, timeout=120)
    dt = time.perf_counter() - t0
    assert res.returncode == 0 and not res.stderr, (res.returncode, res.stderr[-2000:])
    words = res.stdout.split()
    nu, nbl, nx, kind = (int(w) for w in words[:4])
    vals = NP.array(words[7:], dtype=NP.int64)
    assert nbl == bl.shape[0] and vals.size == nu + nbl
    return {'rep': vals[:nu], 'map': vals[nu:], 'n_exact': nx, 'kind': kind, 'tol': float(words[4]), 'max_dev': float(words[5]),
            'phase': float(words[6]), 'seconds': dt}


def numpy_near(bl, tol):
    """the rule, restated -> (rep, map, max_dev)"""
    bl = NP.asarray(bl, dtype=NP.float64).reshape(-1, 3)
    reps = NP.empty((bl.shape[0], 3))
    rep, fmap, dev = [], NP.empty(bl.shape[0], dtype=NP.int64), 0.0
    for b in range(bl.shape[0]):
        v = bl[b]
        hit = NP.flatnonzero(NP.all(NP.abs(v[None, :] - reps[:len(rep)]) <= tol, axis=1))
        if hit.size:
            fmap[b] = hit[0]
            d = [float(x) for x in v - reps[hit[0]]]
            dev = max(dev, math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]))
        else:
            reps[len(rep)] = v
            fmap[b] = len(rep)
            rep.append(b)
    return NP.array(rep, dtype=NP.int64), fmap, dev


def numpy_tol(bl):
    return 16.0 * 2.0 ** -52 * float(NP.abs(bl).max())


def numpy_phase(dev, fmax):
    return 2.0 * math.pi * abs(fmax) / C * 2.0 * dev


def numpy_choose(nbl, n_exact, n_near, phase, allow_near=True):
    """the selection rule of prisim_hip_set_array, restated"""
    if allow_near and n_near < n_exact and n_near * 8 <= nbl * 7 and n_near > 256 and phase <= BUDGET:
        return NEAR
    if n_exact * 8 <= nbl * 7 and n_exact > 256:
        return EXACT
    return NONE


def invariants(bl, tol, rep, fmap):
    bl = NP.asarray(bl, dtype=NP.float64).reshape(-1, 3)
    assert NP.all(NP.abs(bl - bl[rep][fmap]) <= tol)                      # every row within tol of its representative, per component
    assert NP.all(NP.diff(rep) > 0) and NP.all(rep[fmap] <= NP.arange(bl.shape[0])) and NP.array_equal(fmap[rep], NP.arange(rep.size))
    r = bl[rep]
    if rep.size <= 3000:                                                  # representatives pairwise further apart than tol
        d = NP.abs(r[:, None, :] - r[None, :, :]).max(axis=2)
        d[NP.arange(rep.size), NP.arange(rep.size)] = NP.inf
        assert NP.all(d > tol)


def check(exe, bl, tol, tmp_path, expect_nu=None):
    got = run_near(exe, bl, tol, tmp_path)
    rep, fmap, dev = numpy_near(bl, tol)
    if expect_nu is not None:
        assert got['rep'].size == expect_nu, got['rep'].size
    assert NP.array_equal(got['rep'], rep) and NP.array_equal(got['map'], fmap)
    assert got['max_dev'] == dev, (got['max_dev'], dev)
    invariants(bl, tol, got['rep'], got['map'])
    return got


def lattice(rng, n, pitch, ulps, copies):
    """`copies` rows per point of an n x n lattice, each perturbed by 0 ... `ulps` ulp of its own value per component, shuffled"""
    i, j = NP.meshgrid(NP.arange(n) - n // 2, NP.arange(n) - n // 2, indexing='ij')
    pts = NP.stack((pitch * (i + 0.5 * j).ravel(), pitch * 0.75 ** 0.5 * j.ravel(), NP.full(n * n, 0.125)), axis=1)
    bl = NP.repeat(pts, copies, axis=0)
    bl = bl + rng.integers(-ulps, ulps + 1, bl.shape) * NP.spacing(NP.abs(bl))
    return bl[rng.permutation(bl.shape[0])]


# ---- exact duplicates, tol = 0, zeros ----
def test_exact_duplicates_only_is_the_exact_fold(near_exe, tmp_path):
    rng = NP.random.default_rng(9)
    vec = rng.normal(0.0, 300.0, (300, 3))
    mult = 1 + NP.arange(300) % 9
    bl = NP.repeat(vec, mult, axis=0)[rng.permutation(int(mult.sum()))]
    got = check(near_exe, bl, numpy_tol(bl), tmp_path, expect_nu=300)
    rep, fmap = numpy_fold(bl)
    assert NP.array_equal(got['rep'], rep) and NP.array_equal(got['map'], fmap) and got['max_dev'] == 0.0 and got['n_exact'] == 300


@pytest.mark.parametrize('name', ['HERA-19', 'HERA-61'])
def test_tol_zero_is_the_exact_fold(near_exe, tmp_path, name):
    bl = layouts.layout_baselines(name)[0]
    got = run_near(near_exe, bl, 0.0, tmp_path)                            # (the program compares with fold_baselines itself: status 5)
    rep, fmap = numpy_fold(bl)
    assert NP.array_equal(got['rep'], rep) and NP.array_equal(got['map'], fmap) and got['max_dev'] == 0.0


def test_zeros_of_both_signs_and_negative_coordinates(near_exe, tmp_path):
    bl = NP.array([[14.6, -0.0, 0.0], [14.6, 0.0, -0.0], [-0.0, -0.0, -0.0], [0.0, 0.0, 0.0], [14.6, 0.0, 1e-300], [-14.6, 0.0, 0.0],
                   [-14.6 - 1e-13, -1e-13, 1e-13], [-14.6 + 1e-13, 1e-13, -1e-13], [14.6, 0.0, -2e-12], [-1e-13, 1e-13, -0.0]])
    for tol in (0.0, 1e-12):
        got = check(near_exe, bl, tol, tmp_path)
        if tol == 0.0:
            assert list(got['rep']) == [0, 2, 4, 5, 6, 7, 8, 9] and list(got['map']) == [0, 0, 1, 1, 2, 3, 4, 5, 6, 7]
        else:
            assert list(got['rep']) == [0, 2, 5, 8] and list(got['map']) == [0, 0, 1, 1, 0, 2, 2, 2, 3, 1]


def test_single_row_and_no_rows(near_exe, tmp_path):
    got = check(near_exe, NP.array([[1.0, 2.0, 3.0]]), 1e-9, tmp_path, expect_nu=1)
    assert list(got['rep']) == [0] and list(got['map']) == [0] and got['max_dev'] == 0.0
    got = run_near(near_exe, NP.zeros((0, 3)), 1e-9, tmp_path)
    assert got['rep'].size == 0 and got['map'].size == 0 and got['kind'] == NONE


# ---- perturbed lattices, chains, cell boundaries ----
@pytest.mark.parametrize('ulps', [0, 1, 2, 4])
def test_lattice_with_perturbations(near_exe, tmp_path, ulps):
    rng = NP.random.default_rng(40 + ulps)
    bl = lattice(rng, 21, 14.6, ulps, 5)
    tol = numpy_tol(bl)
    assert 8 * NP.spacing(NP.abs(bl).max()) <= tol                        # twice the perturbation of any row is within tol
    got = check(near_exe, bl, tol, tmp_path, expect_nu=441)
    assert got['n_exact'] == (441 if ulps == 0 else numpy_fold(bl)[0].size) and (ulps == 0 or got['n_exact'] > 441)
    assert (got['max_dev'] == 0.0) == (ulps == 0)


def test_a_chain_does_not_join_its_first_row(near_exe, tmp_path):
    tol = 1e-9
    a = NP.array([100.0, -37.5, 2.0])
    for axis in range(3):
        e = NP.zeros(3)
        e[axis] = tol
        bl = NP.stack((a, a + 0.75 * e, a + 1.5 * e))
        got = check(near_exe, bl, tol, tmp_path, expect_nu=2)
        assert list(got['rep']) == [0, 2] and list(got['map']) == [0, 0, 1]
        # ... and a later row between them joins the earliest-founded cluster it is within tol of, not the nearest
        bl = NP.stack((a, a + 1.5 * e, a + 0.9 * e))
        got = check(near_exe, bl, tol, tmp_path, expect_nu=2)
        assert list(got['map']) == [0, 1, 0]


def test_cell_boundaries_and_exactly_tol(near_exe, tmp_path):
    tol = 0.25                                                            # cells of 0.5: boundaries at multiples of 0.5, all exact in binary
    for axis in range(3):
        for edge in (-1.0, 0.0, 0.5, 7.5):
            base = NP.full(3, 0.125 if axis != 1 else -3.0)
            lo, hi, at, past = base.copy(), base.copy(), base.copy(), base.copy()
            lo[axis], hi[axis] = edge - 0.0625, edge + 0.0625             # either side of a cell boundary, 0.125 apart
            at[axis] = edge - 0.0625 + tol                                # exactly tol from `lo`: joins it
            past[axis] = edge - 0.0625 + tol * (1.0 + 2.0 ** -40)            # a hair further: founds a cluster
            got = check(near_exe, NP.stack((lo, hi, at, past)), tol, tmp_path, expect_nu=2)
            assert list(got['map']) == [0, 0, 0, 1], (axis, edge, got['map'])
    # diagonal neighbours: within tol in every component across three cell boundaries at once, and just outside in one
    corner = NP.array([[0.49, 0.99, -0.51], [0.51, 1.01, -0.49], [0.51, 1.01, -0.51 + 0.2401]])
    got = check(near_exe, corner, tol, tmp_path, expect_nu=1)
    corner[2, 2] = -0.51 + NP.nextafter(tol, 1.0)
    got = check(near_exe, corner, tol, tmp_path, expect_nu=2)
    assert list(got['map']) == [0, 0, 1]


@pytest.mark.parametrize('seed', [1, 2, 3, 4])
def test_invariants_on_random_inputs(near_exe, tmp_path, seed):
    rng = NP.random.default_rng(seed)
    tol = float(10.0 ** rng.uniform(-12, -1))
    n = 2500
    # clumps about the size of tol (rows that chain and straddle cells), some exact copies, some far offsets
    centres = rng.normal(0.0, 50.0, (200, 3)) * NP.array([1.0, 1.0, 0.01])
    bl = centres[rng.integers(200, size=n)] + rng.uniform(-1.5, 1.5, (n, 3)) * tol * rng.integers(0, 2, (n, 1))
    bl[::97] += 1e6
    got = check(near_exe, bl, tol, tmp_path)
    assert 200 <= got['rep'].size < n


def test_large_offsets_and_tiny_tolerances_do_not_overflow_the_grid(near_exe, tmp_path):
    rng = NP.random.default_rng(11)
    bl = NP.concatenate((rng.normal(0.0, 1.0, (50, 3)), rng.normal(0.0, 1.0, (50, 3)) + 1e15, [[-1e300, 1e300, 0.0], [1e-300, -1e-300, 0.0]]))
    bl = NP.concatenate((bl, bl))
    got = check(near_exe, bl, 1e-30, tmp_path, expect_nu=102)
    assert got['max_dev'] == 0.0


# ---- the headline array, its shards, and the selection rule ----
@pytest.fixture(scope='module')
def headline(near_exe, tmp_path_factory):
    cfg = W.config3()
    fmax = float(NP.abs(cfg['channels']).max())
    got = run_near(near_exe, cfg['baselines'], 'auto', tmp_path_factory.mktemp('headline'), fmax=fmax)
    return cfg, fmax, got


def test_headline_array(headline):
    cfg, fmax, got = headline
    bl = cfg['baselines']
    assert bl.shape == (61075, 3)
    tol = numpy_tol(bl)
    assert got['tol'] == tol and abs(tol - 2.07e-12) < 5e-15
    rep, fmap, dev = numpy_near(bl, tol)
    assert NP.array_equal(got['rep'], rep) and NP.array_equal(got['map'], fmap) and got['max_dev'] == dev
    invariants(bl, tol, got['rep'], got['map'])
    assert got['n_exact'] == 10999 and got['rep'].size == 7090
    print('headline: %d exact, %d merged, tol %.3e m, max_dev %.3e m, phase bound %.3e rad, %.3f s'
          % (got['n_exact'], got['rep'].size, tol, got['max_dev'], got['phase'], got['seconds']))
    assert '%.1e' % got['max_dev'] == '6.4e-14'
    assert got['phase'] == numpy_phase(dev, fmax) and got['phase'] < BUDGET
    assert got['kind'] == NEAR == numpy_choose(61075, 10999, 7090, got['phase'])
    assert got['seconds'] < 1.0


def test_headline_groups_and_step_tiers(headline, tier_exe, tmp_path):
    cfg, _, got = headline
    ch = cfg['channels']
    df = float(ch[1] - ch[0])
    bl = cfg['baselines'][got['rep']]                                     # what the kernels see: the representatives, first-appearance order
    dc = cfg['sky']['dircos']
    tab, ext = SB.group_tables(bl), SB.sky_extrema(dc, SB.ZEN)
    assert tab.shape[0] == 28 and bl.shape[0] - 27 * 256 == 178
    step, _ = SB.numpy_rule(tab, ext, df, True)
    assert step[:24].max() < 0.1229 + 5e-5 and NP.allclose(step[24:], [0.1264, 0.1303, 0.1353, 0.1867], atol=5e-5), step[23:]
    tiers = ST.check(tier_exe, bl, dc, SB.ZEN, df, tmp_path)
    assert [int(NP.sum(tiers == t)) for t in (1, 2, 0)] == [24, 3, 1]
    assert NP.all(tiers[:24] == 1) and NP.all(tiers[24:27] == 2) and tiers[27] == 0, tiers


def test_shards_of_rank_0(near_exe, tmp_path):
    cfg = W.config3()
    fmax = float(NP.abs(cfg['channels']).max())
    counts = []
    for world in (2, 4, 8):
        bl = sharding.shard_rows(cfg['baselines'], world, 0)[0]
        got = run_near(near_exe, bl, 'auto', tmp_path, fmax=fmax)
        invariants(bl, got['tol'], got['rep'], got['map'])
        assert got['kind'] == NEAR
        counts.append((got['n_exact'], got['rep'].size))
    assert counts == [(6325, 3833), (3457, 2121), (1684, 1022)], counts


def test_selection_rule(near_exe, headline, tmp_path):
    fmax = 150e6 + 63 * 97656.25
    # HERA-61: the merged fold leaves 108 rows, at most one group -- the exact fold (477 rows) is kept; HERA-19: neither
    for name, nbl, nx, nn, kind in (('HERA-61', 1830, 477, 108, EXACT), ('HERA-19', 171, 67, 30, NONE)):
        bl = layouts.layout_baselines(name)[0]
        got = run_near(near_exe, bl, 'auto', tmp_path, fmax=fmax)
        rep, fmap, dev = numpy_near(bl, numpy_tol(bl))
        assert NP.array_equal(got['rep'], rep) and NP.array_equal(got['map'], fmap) and got['max_dev'] == dev
        assert (bl.shape[0], got['n_exact'], rep.size) == (nbl, nx, nn), (name, bl.shape[0], got['n_exact'], rep.size)
        assert got['kind'] == kind == numpy_choose(nbl, nx, nn, numpy_phase(dev, fmax)), (name, got['kind'])
    # HERA-350: merged; with the hook off, exact
    cfg, f350, got = headline
    assert got['kind'] == NEAR
    assert run_near(near_exe, cfg['baselines'], 'auto', tmp_path, fmax=f350, allow_near=False)['kind'] == EXACT
    # deviations within tol but over the budget: the exact fold.  1200 rows of 300 vectors, copies moved by up to 8 ulp of P.
    rng = NP.random.default_rng(8)
    vec = rng.uniform(-250.0, 250.0, (300, 3)) * NP.array([1.0, 1.0, 0.004])
    bl = NP.repeat(vec, 4, axis=0)
    bl[1::2] += rng.integers(-8, 9, (600, 3)) * NP.spacing(NP.abs(bl).max())      # (two exact copies, two moved ones per vector)
    tol = numpy_tol(bl)
    got = run_near(near_exe, bl, 'auto', tmp_path, fmax=fmax)
    rep, fmap, dev = numpy_near(bl, tol)
    assert NP.array_equal(got['rep'], rep) and NP.array_equal(got['map'], fmap) and got['max_dev'] == dev
    assert rep.size == 300 and 300 < got['n_exact'] <= 900 and got['n_exact'] * 8 <= 1200 * 7
    assert got['phase'] == numpy_phase(dev, fmax) and got['phase'] > BUDGET
    assert got['kind'] == EXACT == numpy_choose(1200, got['n_exact'], 300, got['phase'])
    # ... and the same array at a tenth of the frequency is within the budget: merged
    got = run_near(near_exe, bl, 'auto', tmp_path, fmax=fmax / 10.0)
    assert got['phase'] <= BUDGET and got['kind'] == NEAR
