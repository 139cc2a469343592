"""CPU: the source-split count of prisim_amd/csrc/split_plan.h, which make_plan asks for every sky-sum whose split is not set by
set_tuning.  The header is host-only: a stand-alone program around it is built with -fsanitize=address,undefined and run on every case
(nothing loaded into Python is sanitised).  Checked: the header returns what the rule returned while it stood inside make_plan --
restated here, with the one repair the header makes: the floor of 32 sources per split is applied behind the deep branch too, which
alone could leave it (a sky of a few hundred sources on a grid of a few blocks; of the named grids only config 2 in fp32, 64 -> 47,
where make_plan's whole 64-source chunks allow 24 either way) --
    want = round(7.5 slots / (tiles groups)) for grids under 6 rounds of resident blocks, else 1
    want <= nsrc / 32                                              (at least 32 sources per split)
    want > 16: max(16, min(round(1.5 slots / (tiles groups)), cap))   (the partial-traffic cap, never under one round of blocks)
    1 <= nsplit <= 64
on the headline grid, rank 0's shard of 2, 4 and 8 ranks, config 2's grids and random cases; and the bounds on every case."""
import os
import shutil
import subprocess

import numpy as NP
import pytest

from prisim_amd import sharding, workloads as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUS = 256                       # MI355X


@pytest.fixture(scope='module')
def plan_exe(tmp_path_factory):
    gxx = shutil.which('g++')
    assert gxx, 'g++ is needed to build the split-plan driver'
    exe = tmp_path_factory.mktemp('splitplan') / 'split_plan_main'
    subprocess.check_call([gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-Wall', '-Werror',
                           '-I', os.path.join(ROOT, 'prisim_amd', 'csrc'), os.path.join(ROOT, 'tests', 'split_plan_main.cpp'),
                           '-o', str(exe)])
    return str(exe)


def parent_rule(tiles, groups, slots, nsrc, nbl, nchan, f32, taper, floor_behind_cap=True):
    """the rule as make_plan stated it before it moved into the header (integer arithmetic as in C++; int() truncates like the cast);
    floor_behind_cap: with the header's repair"""
    base = tiles * groups
    want = 1
    if base * 10 < slots * 60:
        want = (slots * 15 // 2 + base // 2) // base
    want = min(want, max(1, nsrc // 32))
    rate = (7.0e12 if taper else 1.0e13) if f32 else (2.8e12 if taper else 5.0e12)
    t_compute = float(nbl) * float(nchan) * float(nsrc) / rate
    t_split = 2.0 * float(nbl) * float(nchan) * (8.0 if f32 else 16.0) / 3.0e12
    cap = max((slots + base - 1) // max(base, 1), int(0.03 * t_compute / t_split))
    if want > 16:
        want = max(16, min((3 * slots // 2 + base // 2) // max(base, 1), cap))
        if floor_behind_cap:
            want = min(want, max(1, nsrc // 32))
    return max(1, min(want, 64))


def run_plan(exe, cases, tmp_path):
    path = tmp_path / 'cases.i64'
    NP.asarray(cases, dtype=NP.int64).reshape(-1, 8).tofile(str(path))
    res = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and not res.stderr, (res.returncode, res.stderr[-2000:])
    out = [int(v) for v in res.stdout.split()]
    assert len(out) == len(cases)
    return out


def distinct_vectors(bl):
    return int(NP.unique(NP.asarray(bl, dtype=NP.float64) + 0.0, axis=0).shape[0])


def packed_f32_grid(bl, nchan, nsrc):
    """the grid of the packed fp32 kernel on 64-channel tiles over the rows the sky-sum computes: the distinct vectors when the array
    folds (at most 7/8 of the rows distinct, more than one group of 256), two resident blocks per CU"""
    nu = distinct_vectors(bl)
    rows = nu if nu * 8 <= bl.shape[0] * 7 and nu > 256 else bl.shape[0]
    return [(nchan + 63) // 64, (rows + 255) // 256, 2 * CUS, nsrc, rows, nchan, 1, 0]


def named_cases():
    c3 = W.config3()
    bl, nchan, nsrc = c3['baselines'], c3['channels'].size, c3['sky']['dircos'].shape[0]
    cases = {'headline': packed_f32_grid(bl, nchan, nsrc)}
    for world in (2, 4, 8):
        cases['shard 0 of %d' % world] = packed_f32_grid(sharding.shard_rows(bl, world, 0)[0], nchan, nsrc)
    c2 = W.config2()
    nb2, nc2, ns2 = c2['baselines'].shape[0], c2['channels'].size, c2['sky']['dircos'].shape[0]
    # config 2 (171 baselines: one group): fp64 with the taper on 16-channel tiles, packed fp32 on 32-channel tiles; two blocks per CU both
    cases['config 2 fp64'] = [(nc2 + 15) // 16, 1, 2 * CUS, ns2, nb2, nc2, 0, 1]
    cases['config 2 fp32'] = [(nc2 + 31) // 32, 1, 2 * CUS, ns2, nb2, nc2, 1, 1]
    return cases


def test_named_grids(plan_exe, tmp_path):
    cases = named_cases()
    assert cases['headline'][:5] == [16, 43, 512, 10000, 10999]
    assert [cases['shard 0 of %d' % w][1] for w in (2, 4, 8)] == [25, 14, 7]
    got = dict(zip(cases, run_plan(plan_exe, list(cases.values()), tmp_path)))
    for name, case in cases.items():
        assert got[name] == parent_rule(*case), (name, case, got[name])
        if name != 'config 2 fp32':                                     # the rule as it stood, to the letter
            assert got[name] == parent_rule(*case, floor_behind_cap=False), (name, case, got[name])
    assert got['config 2 fp32'] == 47 and parent_rule(*cases['config 2 fp32'], floor_behind_cap=False) == 64
    print('split counts:', got)
    # 16 x 43 x 6 = 4128 blocks on 512 slots; the shards: 7.5 rounds asks for 10 at N = 2, and is held at 16 from N = 4 on
    assert got['headline'] == 6
    assert [got['shard 0 of %d' % w] for w in (2, 4, 8)] == [10, 16, 16]


def test_random_grids_and_bounds(plan_exe, tmp_path):
    rng = NP.random.default_rng(2024)
    cases = []
    for _ in range(4000):
        nchan = int(rng.integers(1, 4097))
        ct = int(rng.choice([8, 16, 32, 64]))
        nbl = int(rng.integers(1, 70000)) if rng.random() < 0.5 else int(rng.integers(1, 3000))
        f32 = int(rng.integers(2))
        slots = int(rng.choice([64, 104, 208, 304]) * rng.choice([2, 4])) if rng.random() < 0.3 else CUS * int(rng.choice([2, 4]))
        nsrc = int(rng.integers(1, 64)) if rng.random() < 0.2 else int(rng.integers(1, 200000))
        cases.append([(nchan + ct - 1) // ct, (nbl + 255) // 256, slots, nsrc, nbl, nchan, f32, int(rng.integers(2))])
    # the edges: one source, exactly 32 and 63 sources, a grid of exactly 6 rounds and one block short of it, one block in all
    cases += [[1, 1, 512, 1, 1, 1, 1, 0], [1, 1, 512, 32, 3, 8, 1, 0], [1, 1, 512, 63, 3, 8, 0, 1], [1, 1, 512, 64, 3, 8, 0, 1],
              [6, 512, 512, 10000, 512 * 256, 384, 1, 0], [3071, 1, 512, 10000, 256, 3071 * 8, 1, 0], [1, 1, 1, 10 ** 6, 256, 8, 0, 0]]
    got = run_plan(plan_exe, cases, tmp_path)
    split = repaired = 0
    for case, n in zip(cases, got):
        assert n == parent_rule(*case), (case, n)
        old = parent_rule(*case, floor_behind_cap=False)
        assert n == old or (old > 16 and case[3] // old < 32 and n == max(1, case[3] // 32)), (case, n, old)      # the repair and nothing else
        repaired += n != old
        assert 1 <= n <= 64, (case, n)
        assert n == 1 or case[3] // n >= 32, (case, n)                 # at least 32 sources per split
        if case[0] * case[1] * 10 >= case[2] * 60:
            assert n == 1, (case, n)                                    # grids of 6 rounds or more are left whole
        split += n > 1
    assert 200 < split < len(cases) - 200                               # the cases do lie on both sides of the rule
    assert 0 < repaired < len(cases) // 20, repaired
