"""CPU: the fold map of prisim_amd/csrc/baseline_fold.h (rows of equal baseline vectors are summed once, prisim_hip_set_array) against
numpy.unique(axis=0) in first-appearance order.  The header is host-only: a stand-alone program around it is built with
-fsanitize=address,undefined and run on every case (nothing loaded into Python is sanitised)."""
import os
import shutil
import subprocess

import numpy as NP
import pytest

from prisim_amd import layouts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def fold_exe(tmp_path_factory):
    gxx = shutil.which('g++')
    assert gxx, 'g++ is needed to build the fold-map driver'
    exe = tmp_path_factory.mktemp('fold') / 'baseline_fold_main'
    subprocess.check_call([gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-Wall', '-Werror',
                           '-I', os.path.join(ROOT, 'prisim_amd', 'csrc'), os.path.join(ROOT, 'tests', 'baseline_fold_main.cpp'),
                           '-o', str(exe)])
    return str(exe)


def run_fold(exe, bl, tmp_path):
    bl = NP.ascontiguousarray(bl, dtype=NP.float64).reshape(-1, 3)
    path = tmp_path / 'bl.f64'
    bl.tofile(str(path))
    res = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and not res.stderr, (res.returncode, res.stderr[-2000:])
    vals = NP.array(res.stdout.split(), dtype=NP.int64)
    nu, nbl = int(vals[0]), int(vals[1])
    assert nbl == bl.shape[0] and vals.size == 2 + nu + nbl
    return vals[2:2 + nu], vals[2 + nu:]


def numpy_fold(bl):
    """numpy.unique(axis=0) (IEEE value equality once -0.0 is +0.0) re-ordered by first appearance."""
    b = NP.asarray(bl, dtype=NP.float64).reshape(-1, 3) + 0.0          # -0.0 + 0.0 = +0.0
    _, first, inv = NP.unique(b, axis=0, return_index=True, return_inverse=True)
    order = NP.argsort(first)
    rank = NP.empty(order.size, dtype=NP.int64)
    rank[order] = NP.arange(order.size)
    return first[order], rank[NP.asarray(inv).ravel()]


def check(exe, bl, tmp_path, expect_nu=None):
    rep, fmap = run_fold(exe, bl, tmp_path)
    rep_ref, map_ref = numpy_fold(bl)
    if expect_nu is not None:
        assert rep.size == expect_nu
    assert NP.array_equal(rep, rep_ref)
    assert NP.array_equal(fmap, map_ref)
    bl = NP.asarray(bl, dtype=NP.float64).reshape(-1, 3)
    assert NP.array_equal(bl[rep][fmap], bl)                            # (-0.0 == +0.0 here too)
    assert NP.all(rep[fmap] <= NP.arange(bl.shape[0])) and NP.all(NP.diff(rep) > 0)
    return rep, fmap


def test_hera19(fold_exe, tmp_path):
    bl = layouts.layout_baselines('HERA-19')[0]
    assert bl.shape == (171, 3)
    rep, _ = check(fold_exe, bl, tmp_path)
    assert rep.size < 171                       # a hexagonal lattice is redundant


def test_hera350(fold_exe, tmp_path):
    bl = layouts.layout_baselines('HERA-350')[0]
    assert bl.shape == (61075, 3)
    assert NP.any(NP.signbit(bl) & (bl == 0.0))  # the layouts do contain negative zeros
    _, fmap = check(fold_exe, bl, tmp_path, expect_nu=10999)
    assert NP.bincount(fmap).max() == 182


def test_all_rows_distinct(fold_exe, tmp_path):
    bl = NP.random.default_rng(5).normal(0.0, 100.0, (1000, 3))
    rep, fmap = check(fold_exe, bl, tmp_path, expect_nu=1000)
    assert NP.array_equal(rep, NP.arange(1000)) and NP.array_equal(fmap, NP.arange(1000))


def test_all_rows_equal(fold_exe, tmp_path):
    rep, fmap = check(fold_exe, NP.tile(NP.array([14.6, -3.0, 0.25]), (777, 1)), tmp_path, expect_nu=1)
    assert rep[0] == 0 and not fmap.any()


def test_negative_and_positive_zero_are_one_class(fold_exe, tmp_path):
    bl = NP.array([[14.6, -0.0, 0.0], [14.6, 0.0, -0.0], [-0.0, -0.0, -0.0], [0.0, 0.0, 0.0], [14.6, 0.0, 1e-300]])
    rep, fmap = check(fold_exe, bl, tmp_path, expect_nu=3)
    assert list(rep) == [0, 2, 4] and list(fmap) == [0, 0, 1, 1, 2]


def test_single_row(fold_exe, tmp_path):
    rep, fmap = check(fold_exe, NP.array([[1.0, 2.0, 3.0]]), tmp_path, expect_nu=1)
    assert list(rep) == [0] and list(fmap) == [0]


def test_irregular_multiplicities_in_scrambled_order(fold_exe, tmp_path):
    rng = NP.random.default_rng(9)
    vec = rng.normal(0.0, 300.0, (300, 3))
    mult = 1 + NP.arange(300) % 9
    bl = NP.repeat(vec, mult, axis=0)[rng.permutation(int(mult.sum()))]
    check(fold_exe, bl, tmp_path, expect_nu=300)
