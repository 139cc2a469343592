"""GPU (-m gpu): tail pieces (csrc/tail_plan.h).  The packed fp32 sky-sum without the taper cuts the last of the plan's source pieces into
a half and up to four eighths, writes one partial cube per piece and maps its blocks through a per-XCD slab table.  The rule proper needs
a grid three rounds of resident blocks deep; PRISIM_HIP_TAIL_PIECES=force (read by set_array) drops that and the 64-source floor, so the
cases here are small.  Two child processes run every case once, one under `force` and one under `0` (the plan's pieces); a last test runs
the rule itself, in this process, on the smallest grid that is deep enough.

Checked against the fp64 C oracle at the project's fp32 tolerance, 5e-6 of S_f = sum_s |pbflux[s, f]| (on the large cases for 64 rows
spread over the baseline groups), the counts the library reports against a numpy restatement of planner and rule
(test_split_plan.parent_rule, test_tail_plan.restated), and the stated bit-equalities.  Every case: 64-channel tiles (set_tuning(64, 0, 0):
the split count and the chunk stay the planner's), baselines sorted by length so that the groups run different bodies.

The planner cuts a sky of 1100 sources on these small grids into single 64-source chunks, so the last piece (12 sources) cannot be cut and
the restatement gives no tail pieces for the three 1100-source cases: there the launch must simply be the plan's.  The cases where the
rule engages under `force`:
  e576   700 rows / 300 distinct x 576 channels (9 tiles) x 4000 sources: 21 pieces of 192, the last 160 -> 128 + 32 (a piece under 64
         sources: the warm-up is off inside it)
  e576b  the same array, 4100 sources: 22 pieces, the last 68 -> 64 + 4
  e64    300 rows x 64 channels (one tile) x 16500 sources: 52 pieces of 320, the last 180 -> 128 + 52; 53 slabs on 8 XCDs, so the table
         has padding entries (fewer than 8 slabs never reach the table: such a sky is cut into single chunks)
  e1500  1500 rows (6 groups) x 576 channels x 8150 sources, not a multiple of the chunk: 16 pieces of 512, the last 470 -> 256 + 3 x 64 + 22"""
import functools
import os
import subprocess
import sys

import numpy as NP
import pytest

from oracle import skyvis_oracle as O, c_oracle as CO
from prisim_amd import _abi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_split_plan as SP                                   # noqa: E402
import test_tail_plan as TP                                    # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL32 = 5e-6
ZEN = NP.array([0.0, 0.0, 1.0])
F32, F64, REC = _abi.PRISIM_FP32, _abi.PRISIM_FP64, _abi.PRISIM_KERNEL_RECURRENCE
#        name: (rows, distinct, channels, sources, seed)
CASES = {'a128': (700, 300, 128, 1100, 1), 'a576': (700, 300, 576, 1100, 2), 'a64': (700, 300, 64, 1100, 3),
         'e576': (700, 300, 576, 4000, 4), 'e576b': (700, 300, 576, 4100, 4), 'e64': (300, 300, 64, 16500, 5),
         'e1500': (1500, 1500, 576, 8150, 6)}
FAMILIES = ('taper', 'fp64', 'grad', 'two_runs', 'tuned3')


def channels(nchan):
    return 150e6 + 1e5 * NP.arange(nchan)


@functools.lru_cache(maxsize=None)
def case(name):
    """(baselines, distinct rows, fold map, direction cosines, pbflux) -- the same in this process and in the children"""
    nrows, nu, nchan, nsrc, seed = CASES[name]
    rng = NP.random.default_rng(7000 + seed)
    r = NP.sort(rng.uniform(5.0, 600.0, nu))                  # by length: the first groups leapfrog, the last take the plain rotation
    a = rng.uniform(0.0, 2 * NP.pi, nu)
    uniq = NP.stack((r * NP.cos(a), r * NP.sin(a), rng.uniform(-2.0, 2.0, nu)), axis=1)
    rows = NP.concatenate((NP.arange(nu), rng.integers(0, nu, nrows - nu)))      # (distinct vectors in order of first appearance)
    alt = NP.degrees(NP.arcsin(rng.uniform(NP.sin(NP.radians(10.0)), 1.0, nsrc)))
    dc = O.altaz2dircos(NP.stack((alt, rng.uniform(0, 360, nsrc)), axis=1))
    pb = rng.uniform(0.5, 10.0, size=(nsrc, 1)) * rng.uniform(0.5, 1.0, size=(nsrc, nchan))
    if name == 'e576b':                                        # the sky of e576 and 100 sources more
        dc[:4000], pb[:4000] = case('e576')[3], case('e576')[4]
    for arr in (uniq, rows, dc, pb):
        arr.setflags(write=False)
    return uniq[rows], uniq, rows, dc, pb


def two_run_fwhm(nsrc):
    f = NP.zeros(nsrc)
    f[nsrc // 2:] = 0.5
    return f


def one(ctx, name, precision=F32, **kw):
    bl, _, _, dc, pb = case(name)
    v = ctx.skyvis(dc, pb, ZEN, precision=precision, kernel=REC, **kw)
    tm = ctx.timing()
    return v, [tm['last_chan_tile'], tm['last_nsplit'], tm['last_sum_pieces'], tm['last_tail_pieces'], tm['last_sum_baselines']]


def child_main(out_path):
    """everything the parent compares, under the PRISIM_HIP_TAIL_PIECES of this process"""
    res = {}
    with _abi.Context(0) as ctx:
        res['cus'] = NP.array(ctx.device_info()['cu_count'])
        for name in CASES:
            ctx.set_array(case(name)[0], channels(CASES[name][2]))
            ctx.set_tuning(64, 0, 0)
            res['v_' + name], res['tm_' + name] = one(ctx, name)
        # the kernel families that keep the plan's pieces, on e576
        nsrc = CASES['e576'][3]
        ctx.set_array(case('e576')[0], channels(576))
        ctx.set_tuning(64, 0, 0)
        res['v_taper'], res['tm_taper'] = one(ctx, 'e576', fwhm_deg=NP.full(nsrc, 0.5))
        res['v_two_runs'], res['tm_two_runs'] = one(ctx, 'e576', fwhm_deg=two_run_fwhm(nsrc))
        res['v_fp64'], res['tm_fp64'] = one(ctx, 'e576', precision=F64)
        (res['v_grad'], res['g_grad']), res['tm_grad'] = one(ctx, 'e576', want_grad=True)
        ctx.set_tuning(64, 0, 3)
        res['v_tuned3'], res['tm_tuned3'] = one(ctx, 'e576')
        # deferred post-pass: four queued computes into alternating slots, then the same sequence waited for one by one
        ctx.set_array(case('e576')[0], channels(576), nt_max=2)
        ctx.set_tuning(64, 0, 0)
        seq = ('e576', 'e576b', 'e576', 'e576b')
        for t, name in enumerate(seq):
            ctx.set_sky(case(name)[3], case(name)[4], ZEN)
            ctx.compute(precision=F32, slot=t % 2)
        ctx.sync()
        res['queued'] = NP.stack([ctx.get_vis(slot=s) for s in range(2)])
        for t, name in enumerate(seq):
            ctx.set_sky(case(name)[3], case(name)[4], ZEN)
            ctx.compute(precision=F32, slot=t % 2)
            ctx.sync()
            res['synced_%d' % t] = ctx.get_vis(slot=t % 2)
        # stale tables: a second sky of another source count on the same array, then a second set_array
        res['stale_a'], _ = one(ctx, 'e576')
        res['stale_b'], res['tm_stale_b'] = one(ctx, 'e576b')
        ctx.set_array(case('e576')[0], channels(576))
        ctx.set_tuning(64, 0, 0)
        res['stale_b2'], _ = one(ctx, 'e576b')
        res['stale_a2'], res['tm_stale_a2'] = one(ctx, 'e576')
    for name in ('e576b', 'e576'):
        with _abi.Context(0) as ctx:
            ctx.set_array(case(name)[0], channels(576))
            ctx.set_tuning(64, 0, 0)
            res['fresh_' + name], _ = one(ctx, name)
    NP.savez(out_path, **res)


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    """{mode: results of child_main} for PRISIM_HIP_TAIL_PIECES = force and 0, one process each"""
    out = {}
    for mode in ('force', '0'):
        path = str(tmp_path_factory.mktemp('tail') / ('run_%s.npz' % mode))
        env = dict(os.environ, PRISIM_HIP_TAIL_PIECES=mode, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
        code = 'import sys; sys.path.insert(0, %r); import test_gpu_tail_pieces as T; T.child_main(sys.argv[1])' % os.path.join(ROOT, 'tests')
        res = subprocess.run([sys.executable, '-c', code, path], env=env, capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stderr[-3000:]
        out[mode] = dict(NP.load(path))
    return out


def expected(name, cus, mode):
    """(plan's count, partial cubes, tail pieces) by the numpy restatement of planner and rule"""
    _, nu, nchan, nsrc, _ = CASES[name]
    tiles, groups, slots = (nchan + 63) // 64, (nu + 255) // 256, 2 * cus
    n0, per = TP.plan_pieces(nsrc, 64, SP.parent_rule(tiles, groups, slots, nsrc, nu, nchan, 1, 0))
    lo, ntail = TP.restated(n0, per, 64, 0, nsrc, tiles, groups, slots, mode, 0)
    return n0, len(lo) - 1, ntail


def oracle_rows(name, nrows=64):
    """the oracle's V of `nrows` distinct vectors spread over the baseline groups (all of them on the small cases)"""
    _, uniq, _, dc, pb = case(name)
    _, nu, nchan, nsrc, _ = CASES[name]
    pick = NP.arange(nu) if nu * nchan * nsrc <= 2e8 else NP.unique(NP.linspace(0, nu - 1, nrows).astype(int))
    return pick, CO.skyvis(uniq[pick], channels(nchan), dc, pb, ZEN)


def relerr(v, ref, pb):
    return float(NP.max(NP.abs(v - ref) / O.abs_flux_sum(pb)[None, :]))


@pytest.mark.parametrize('name', list(CASES))
def test_pieces_counts_and_parity(runs, name):
    """under `force`: the reported pieces are the restatement's, last_nsplit stays the plan's, every row is its distinct vector's, the
    oracle is met, and the `0` run (the plan's pieces) differs by no more than the tolerance"""
    _, _, rows, _, pb = case(name)
    nu = CASES[name][1]
    cus = int(runs['force']['cus'])
    n0, pieces, ntail = expected(name, cus, TP.FORCE)
    v, tm = runs['force']['v_' + name], runs['force']['tm_' + name].tolist()
    v0, tm0 = runs['0']['v_' + name], runs['0']['tm_' + name].tolist()
    print('%s: plan %d pieces -> %d (%d of the last), reported %s' % (name, n0, pieces, ntail, tm))
    folded = nu < rows.size
    assert tm == [64, n0, pieces, ntail, nu if folded else rows.size], (tm, n0, pieces, ntail)
    assert tm0 == [64, n0, n0, 0, tm[4]], tm0
    if cus == 256:
        assert (ntail > 0) == name.startswith('e'), (name, ntail)        # the cases the docstring says engage, do
    vu = v[:nu]
    assert NP.array_equal(v, vu[rows])
    pick, ref = oracle_rows(name)
    err, err0, diff = relerr(vu[pick], ref, pb), relerr(v0[:nu][pick], ref, pb), relerr(v, v0, pb)
    print('%s: err / S_f = %.3e (force) %.3e (plan); |force - plan| / S_f = %.3e' % (name, err, err0, diff))
    assert err <= TOL32 and err0 <= TOL32 and diff <= TOL32, (err, err0, diff)
    if ntail == 0:
        assert NP.array_equal(v, v0)                                       # no tail pieces: the plan's launch, the plan's bits


def test_deferred_post_with_both_partial_sets(runs):
    """four queued computes (skies of 4000 and 4100 sources alternating: 22 and 23 partial cubes, the tables uploaded again each time)
    into slots 0, 1, 0, 1 leave what the same sequence leaves when every compute is waited for"""
    r = runs['force']
    assert r['tm_e576'].tolist()[3] == 2 and r['tm_e576b'].tolist()[3] == 2
    assert NP.array_equal(r['queued'][0], r['synced_2']) and NP.array_equal(r['queued'][1], r['synced_3'])
    assert NP.array_equal(r['synced_0'], r['synced_2']) and NP.array_equal(r['synced_1'], r['synced_3'])
    assert NP.array_equal(r['synced_2'], r['v_e576']) and NP.array_equal(r['synced_3'], r['v_e576b'])
    assert not NP.array_equal(r['synced_2'], r['synced_3'])


def test_tables_follow_the_sky_and_the_array(runs):
    """a second sky of another source count on the same array, then a second set_array: bit for bit a fresh context's results"""
    r = runs['force']
    assert r['tm_stale_b'].tolist()[2:4] == [23, 2] and r['tm_stale_a2'].tolist()[2:4] == [22, 2]
    for tag, name in (('a', 'e576'), ('b', 'e576b')):
        assert NP.array_equal(r['stale_' + tag], r['fresh_' + name])
        assert NP.array_equal(r['stale_%s2' % tag], r['fresh_' + name])


@pytest.mark.parametrize('family', FAMILIES)
def test_other_families_keep_the_plans_pieces(runs, family):
    """taper, a sky of two runs, fp64, the fused gradient and a tuned split count: no tail pieces under `force`, and the bits of the `0` run"""
    r, r0 = runs['force'], runs['0']
    tm = r['tm_' + family].tolist()
    print('%s: tile, nsplit, pieces, tail pieces, rows = %s' % (family, tm))
    assert tm[3] == 0, tm
    assert tm == r0['tm_' + family].tolist()
    assert NP.array_equal(r['v_' + family], r0['v_' + family])
    if family == 'grad':
        assert NP.array_equal(r['g_grad'], r0['g_grad'])
    if family == 'tuned3':
        assert tm[:4] == [64, 3, 3, 0], tm                                # set_tuning(64, 0, 3): exactly three partial cubes
        assert r['tm_e576'].tolist()[3] == 2                               # ... where the planner's own count is cut


def test_the_rule_itself_on_a_deep_grid(ctx):
    """No hook: 7424 rows (29 groups) x 576 channels (9 tiles) x 8630 sources.  The planner asks for 15 pieces of 576 on 261 x 15 = 3915
    items >= 3 x 512 slots, the last piece is 566 sources: 320 + 128 + 118, 17 partial cubes.  (On a device of another CU count the
    restatement decides what is expected.)"""
    nu, nchan, nsrc = 7424, 576, 8630
    rng = NP.random.default_rng(7100)
    r = NP.sort(rng.uniform(5.0, 600.0, nu))
    a = rng.uniform(0.0, 2 * NP.pi, nu)
    bl = NP.stack((r * NP.cos(a), r * NP.sin(a), rng.uniform(-2.0, 2.0, nu)), axis=1)
    alt = NP.degrees(NP.arcsin(rng.uniform(NP.sin(NP.radians(10.0)), 1.0, nsrc)))
    dc = O.altaz2dircos(NP.stack((alt, rng.uniform(0, 360, nsrc)), axis=1))
    pb = rng.uniform(0.5, 10.0, size=(nsrc, 1)) * rng.uniform(0.5, 1.0, size=(nsrc, nchan))
    cus = ctx.device_info()['cu_count']
    tiles, groups, slots = 9, 29, 2 * cus
    n0, per = TP.plan_pieces(nsrc, 64, SP.parent_rule(tiles, groups, slots, nsrc, nu, nchan, 1, 0))
    lo, ntail = TP.restated(n0, per, 64, 0, nsrc, tiles, groups, slots, TP.RULE, 0)
    if cus == 256:
        assert (n0, per, len(lo) - 1, ntail) == (15, 576, 17, 3)
    ctx.set_array(bl, channels(nchan))
    ctx.set_tuning(64, 0, 0)
    try:
        v = ctx.skyvis(dc, pb, ZEN, precision=F32, kernel=REC)
        tm = ctx.timing()
    finally:
        ctx.set_tuning(0, 0, 0)
    assert (tm['last_chan_tile'], tm['last_nsplit'], tm['last_sum_pieces'], tm['last_tail_pieces']) == (64, n0, len(lo) - 1, ntail), tm
    pick = NP.unique(NP.linspace(0, nu - 1, 48).astype(int))
    err = relerr(v[pick], CO.skyvis(bl[pick], channels(nchan), dc, pb, ZEN), pb)
    print('the rule on a deep grid: %d -> %d pieces, err / S_f = %.3e' % (n0, len(lo) - 1, err))
    assert err <= TOL32, err
