"""CPU: the tail pieces of prisim_amd/csrc/tail_plan.h.  The packed fp32 sky-sum without the taper cuts the LAST of the plan's n0
source pieces, L sources long, into round_up(L / 2, chunk) and up to four of round_up(L / 8, chunk) (the last takes what is left), and
deals the slabs (piece, tile) round-robin to the 8 XCDs.  The header is host-only: a stand-alone program around it is built with
-fsanitize=address,undefined and run on every case (nothing loaded into Python is sanitised).  Checked on 4000 random grids and on
the named ones (the headline, rank 0's shard of 2 / 4 / 8, built as test_split_plan.named_cases builds them):
  pieces   tile [src_lo, src_hi) exactly and in order, none empty; every boundary but the last a multiple of the chunk from src_lo;
           the first n0 - 1 pieces are the plan's; n <= min(n0 + 4, 64); unchanged wherever a condition fails (tuned, n0 = 1, a grid
           shallower than three rounds, a tail piece under 64 sources); equal to a numpy restatement of the rule;
  table    holds every (piece, tile) once; piece sizes never increase along an XCD's row; per size class the XCDs differ by <= 1;
  headline n0 = 6 becomes 10 pieces (5 x 1728, 704, 3 x 192, 80), 10 + 2 + 8 slabs per XCD;
  model    a list-scheduling model of the launch (below) never gives the tail pieces a longer makespan than the plan's pieces on the
           named grids.  This tests the rule, not the GPU.

The model, per XCD: 32 CUs x 2 resident blocks; the XCD's items start in their order, the next one on the CU with the fewest resident
blocks; the elder block of a CU advances at 0.75, the younger at 0.25, a lone block at 0.75 (a lone wave per SIMD issues packed FMAs
at 3/4 rate: split_plan.h).  An item costs its piece's sources times 1 / 1.04 / 1.51 for a strict / wide / plain baseline group (the
VALU census of the three source loops, 154 / 160 / 232 per 64 wave-terms); the groups of a slab are walked last-first, and of G groups
the last is taken as plain and the round(3 G / 43) before it as wide, the headline's own tiers (39 / 3 / 1 of 43) scaled to the grid."""
import os
import shutil
import subprocess
import sys

import numpy as NP
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_split_plan as SP                                   # noqa: E402

ROOT = SP.ROOT
OFF, RULE, FORCE = 0, 1, 2


@pytest.fixture(scope='module')
def tail_exe(tmp_path_factory):
    gxx = shutil.which('g++')
    assert gxx, 'g++ is needed to build the tail-plan driver'
    exe = tmp_path_factory.mktemp('tailplan') / 'tail_plan_main'
    subprocess.check_call([gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-Wall', '-Werror',
                           '-I', os.path.join(ROOT, 'prisim_amd', 'csrc'), os.path.join(ROOT, 'tests', 'tail_plan_main.cpp'),
                           '-o', str(exe)])
    return str(exe)


def run_tail(exe, cases, tmp_path):
    """cases: (n0, src_per_split, chunk, src_lo, src_hi, ntiles, nbgroups, slots, mode, tuned) -> [(n, ntail, per, lo, tab[8][per][2])]"""
    path = tmp_path / 'cases.i64'
    NP.asarray(cases, dtype=NP.int64).reshape(-1, 10).tofile(str(path))
    res = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and not res.stderr, (res.returncode, res.stderr[-2000:])
    out = []
    for line in res.stdout.splitlines():
        v = [int(x) for x in line.split()]
        n, ntail, per = v[:3]
        lo = v[3:4 + n]
        tab = NP.asarray(v[4 + n:], dtype=NP.int64).reshape(8, per, 2)
        out.append((n, ntail, per, lo, tab))
    assert len(out) == len(cases)
    return out


def plan_pieces(nsrc, chunk, want):
    """make_plan's realisation of a split count in whole chunks: (n0, src_per_split)"""
    nchunks = (max(nsrc, 1) + chunk - 1) // chunk
    want = max(1, min(want, nchunks))
    cps = (nchunks + want - 1) // want
    return (nchunks + cps - 1) // cps, cps * chunk


def restated(n0, per, chunk, src_lo, src_hi, ntiles, nbgroups, slots, mode, tuned):
    """the rule in numpy: the boundaries and the number of tail pieces"""
    plan = [min(src_lo + i * per, src_hi) for i in range(n0)] + [src_hi]
    if mode == OFF or tuned or n0 < 2 or n0 + 1 > 64:
        return plan, 0
    if mode != FORCE and ntiles * nbgroups * n0 < 3 * slots:
        return plan, 0
    start = src_lo + (n0 - 1) * per
    L = src_hi - start
    if L < 8 * (1 if mode == FORCE else 64):
        return plan, 0
    up = lambda x: int(NP.ceil(NP.ceil(x) / chunk)) * chunk     # noqa: E731  (round_up of the real quotient)
    lens = [up(L / 2.0)] + [up(L / 8.0)] * 3
    cuts = NP.minimum(NP.cumsum(lens), L).tolist() + [L]
    cuts = [0] + sorted(set(cuts))                               # empty pieces are dropped
    sizes = NP.diff(cuts)
    if len(sizes) < 2 or n0 - 1 + len(sizes) > 64 or sizes.min() < (1 if mode == FORCE else 64):
        return plan, 0
    return plan[:n0 - 1] + [start + c for c in cuts], len(sizes)


def check_pieces(case, got):
    n0, per, chunk, src_lo, src_hi, ntiles, nbgroups, slots, mode, tuned = case
    n, ntail, _, lo, _ = got
    want_lo, want_ntail = restated(*case)
    assert lo == want_lo and ntail == want_ntail and n == len(want_lo) - 1, (case, lo, want_lo)
    assert lo[0] == src_lo and lo[-1] == src_hi and all(b > a for a, b in zip(lo, lo[1:])), (case, lo)      # tile the range, none empty
    assert all((b - src_lo) % chunk == 0 for b in lo[:-1]), (case, lo)
    assert lo[:n0] == [src_lo + i * per for i in range(n0)], (case, lo)                                      # the first n0 - 1 pieces are the plan's
    assert n <= min(n0 + 4, 64) and (ntail == 0) == (n == n0), (case, n, ntail)
    sizes = NP.diff(lo)
    assert NP.all(sizes[1:] <= sizes[:-1]), (case, lo)
    if mode == OFF or tuned or n0 == 1 or (mode == RULE and ntiles * nbgroups * n0 < 3 * slots):
        assert ntail == 0, case
    if mode == RULE and ntail:
        assert sizes[n0 - 1:].min() >= 64, (case, lo)
    if mode == RULE and (src_hi - src_lo - (n0 - 1) * per) < 8 * 64:
        assert ntail == 0, (case, lo)                            # L / 8 < 64


def check_table(case, got):
    ntiles = case[5]
    n, _, per, lo, tab = got
    sizes = NP.diff(lo)
    assert per == (n * ntiles + 7) // 8
    used = tab[tab[:, :, 0] >= 0]
    assert NP.all(tab[tab[:, :, 0] < 0] == -1)
    assert sorted(map(tuple, used.tolist())) == [(p, t) for p in range(n) for t in range(ntiles)]           # every slab exactly once
    for x in range(8):
        row = tab[x]
        k = int(NP.sum(row[:, 0] >= 0))
        assert NP.all(row[:k, 0] >= 0) and NP.all(row[k:, 0] < 0)                                          # the padding is behind the slabs
        sz = sizes[row[:k, 0]]
        assert NP.all(sz[1:] <= sz[:-1]), (case, x)                                                         # big ones first
    for s in NP.unique(sizes):
        cnt = [int(NP.sum(sizes[tab[x][tab[x][:, 0] >= 0][:, 0]] == s)) for x in range(8)]
        assert max(cnt) - min(cnt) <= 1, (case, int(s), cnt)


def named_cases():
    """(n0, src_per_split, chunk, ...) of the headline and of rank 0's shard of 2 / 4 / 8: the grids of test_split_plan with the
    planner's split count (checked there against the header) realised in whole 64-source chunks"""
    cases = {}
    for name, (tiles, groups, slots, nsrc, nbl, nchan, f32, taper) in SP.named_cases().items():
        if name.startswith('config 2'):
            continue
        n0, per = plan_pieces(nsrc, 64, SP.parent_rule(tiles, groups, slots, nsrc, nbl, nchan, f32, taper))
        cases[name] = [n0, per, 64, 0, nsrc, tiles, groups, slots, RULE, 0]
    return cases


def test_named_grids(tail_exe, tmp_path):
    cases = named_cases()
    got = dict(zip(cases, run_tail(tail_exe, list(cases.values()), tmp_path)))
    for name, case in cases.items():
        check_pieces(case, got[name])
        check_table(case, got[name])
    # the headline, restated: 6 pieces of 1728 (the last 1360 long) become 5 x 1728, 704, 3 x 192, 80
    assert cases['headline'][:2] == [6, 1728]
    n, ntail, per, lo, tab = got['headline']
    assert (n, ntail) == (10, 5) and NP.diff(lo).tolist() == [1728] * 5 + [704, 192, 192, 192, 80]
    sizes = NP.diff(lo)
    assert per == 20
    for x in range(8):
        sz = sizes[tab[x][:, 0]]
        assert (int(NP.sum(sz == 1728)), int(NP.sum(sz == 704)), int(NP.sum(sz < 704))) == (10, 2, 8)
    # the shards: 10 pieces of 1024 at N = 2 (the last 784 long: 448, 128, 128, 80); at N = 4 and 8 the planner's 16 pieces of 640 leave
    # L = 400, whose eighth is under 64 sources: the plan's pieces stand
    assert (got['shard 0 of 2'][0], got['shard 0 of 2'][1]) == (13, 4) and NP.diff(got['shard 0 of 2'][3]).tolist()[9:] == [448, 128, 128, 80]
    assert [got['shard 0 of %d' % w][:2] for w in (4, 8)] == [(16, 0), (16, 0)]


def test_random_grids(tail_exe, tmp_path):
    rng = NP.random.default_rng(2025)
    cases = []
    for _ in range(4000):
        chunk = int(rng.choice([16, 32, 64, 64, 64, 128]))
        nsrc = int(rng.integers(1, 3000)) if rng.random() < 0.3 else int(rng.integers(1, 200000))
        n0, per = plan_pieces(nsrc, chunk, int(rng.integers(1, 65)))
        src_lo = 0 if rng.random() < 0.7 else int(rng.integers(0, 1000)) * chunk
        ntiles = int(rng.integers(1, 65))
        nbgroups = int(rng.integers(1, 300))
        slots = int(rng.choice([128, 208, 512, 608, 1024]))
        mode = int(rng.choice([OFF, RULE, RULE, RULE, FORCE, FORCE]))
        cases.append([n0, per, chunk, src_lo, src_lo + nsrc, ntiles, nbgroups, slots, mode, int(rng.random() < 0.15)])
    # the edges: one piece; a forced last piece of 200 sources (128, 64, 8); the last piece exactly 8 x 64 and one source short of it; 64 pieces;
    # 60 pieces (n0 + 4 is the bound) and 61 (the rule would pass 64); a grid exactly three rounds deep and one item short of it
    cases += [[1, 6400, 64, 0, 6400, 16, 43, 512, RULE, 0], [2, 640, 64, 0, 840, 16, 43, 512, FORCE, 0],
              [6, 1024, 64, 0, 5 * 1024 + 512, 16, 43, 512, RULE, 0], [6, 1024, 64, 0, 5 * 1024 + 511, 16, 43, 512, RULE, 0],
              [64, 640, 64, 0, 64 * 640, 16, 43, 512, RULE, 0], [60, 1024, 64, 0, 60 * 1024, 16, 43, 512, RULE, 0],
              [61, 1024, 64, 0, 61 * 1024, 16, 43, 512, RULE, 0], [6, 1728, 64, 0, 10000, 16, 16, 512, RULE, 0],
              [6, 1728, 64, 0, 10000, 17, 15, 512, RULE, 0]]
    got = run_tail(tail_exe, cases, tmp_path)
    on = 0
    for case, g in zip(cases, got):
        check_pieces(case, g)
        check_table(case, g)
        on += g[1] > 0
    assert 400 < on < len(cases) - 400                                   # the cases do lie on both sides of the rule
    edge = got[4000:]
    assert [g[1] for g in edge] == [0, 3, 5, 0, 0, 5, 0, 5, 0], [g[1] for g in edge]
    assert edge[5][0] == 64 and edge[6][0] == 61


# ---- the list-scheduling model ---------------------------------------------------------------------------------------------------------

def group_costs(groups):
    wide = int(round(3.0 * groups / 43.0))
    cost = NP.ones(groups)
    cost[groups - 1 - wide:groups - 1] = 1.04
    cost[groups - 1] = 1.51
    return cost


def xcd_makespan(items):
    """items: the costs of one XCD's work items in start order -> the time its last block ends"""
    cus = [[] for _ in range(32)]                                 # per CU: the remaining work of its resident blocks, eldest first
    nxt, t = 0, 0.0
    items = list(items)
    while True:
        while nxt < len(items):                                   # the next item starts on the CU with the fewest resident blocks
            c = min(range(32), key=lambda i: len(cus[i]))
            if len(cus[c]) >= 2:
                break
            cus[c].append(items[nxt])
            nxt += 1
        busy = [c for c in cus if c]
        if not busy:
            return t
        # the elder block advances at 0.75 (also when alone), the younger at 0.25: the time to the first completion anywhere
        dt = min(min(c[0] / 0.75, c[1] / 0.25 if len(c) > 1 else NP.inf) for c in busy)
        t += dt
        for c in busy:
            c[0] -= 0.75 * dt
            if len(c) > 1:
                c[1] -= 0.25 * dt
            c[:] = [w for w in c if w > 1e-9]


def plan_makespan(sizes, ntiles, groups):
    """block_item's map: the slab-major items cut into 8 ranges by count; a slab's groups last-first"""
    gc = group_costs(groups)[::-1]
    items = NP.concatenate([NP.full(ntiles * groups, float(s)) for s in sizes]) * NP.tile(gc, len(sizes) * ntiles)
    per = (len(items) + 7) // 8
    return max(xcd_makespan(items[x * per:(x + 1) * per]) for x in range(8))


def table_makespan(sizes, tab, groups):
    gc = group_costs(groups)[::-1]
    return max(xcd_makespan(NP.concatenate([float(sizes[p]) * gc for p, _ in tab[x] if p >= 0])) for x in range(8))


def test_model_never_prefers_the_plans_pieces(tail_exe, tmp_path):
    cases = named_cases()
    tail = run_tail(tail_exe, list(cases.values()), tmp_path)
    plan = run_tail(tail_exe, [c[:8] + [OFF, 0] for c in cases.values()], tmp_path)
    for (name, case), gt, gp in zip(cases.items(), tail, plan):
        ntiles, groups = case[5], case[6]
        work = float(NP.sum(NP.diff(gp[3]))) * ntiles * float(NP.sum(group_costs(groups))) / (8 * 32 * 1.0)      # divisible work per CU at rate 1
        t_plan = plan_makespan(NP.diff(gp[3]), ntiles, groups)
        t_tail = table_makespan(NP.diff(gt[3]), gt[4], groups) if gt[1] else t_plan
        print('%-14s pieces %2d -> %2d   efficiency %.3f -> %.3f   makespan ratio %.4f' % (name, gp[0], gt[0], work / t_plan, work / t_tail, t_tail / t_plan))
        assert t_tail <= t_plan * (1.0 + 1e-12), (name, t_tail, t_plan)
    # (the dealt table alone, with the plan's equal pieces, is the same items in another order: the model's gain is the pieces')
