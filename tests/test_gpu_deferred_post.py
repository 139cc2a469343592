"""GPU (-m gpu): the deferred post-pass.  A folded compute() with a source split (recurrence kernel, no gradient) enqueues only pack /
prep and the sky-sum on the compute stream; k_reduce_partials and k_expand_rows run on the post stream behind an event, under the next
snapshot's sky-sum, on two alternating sets of partial cubes.  The kernels and the order of summation are those of the single-stream
order (PRISIM_HIP_DEFER_POST=0, read by set_array), so every result is the same bit for bit; what these tests check is the ordering:
queued snapshots, reuse of a partial set two computes later, readers and undeferred computes issued right behind a deferred one.

HERA-61 (1830 rows, 477 distinct vectors: folded) x 128 channels x 250 seeded point sources, fp32, set_tuning(64, 0, 3) so that partial
cubes exist.  The C oracle is held at the suite's fp32 tolerance, 5e-6 of S_f = sum_s |pbflux[s, f]| (1e-11 for the one fp64 case)."""
import os
import subprocess
import sys

import numpy as NP
import pytest

from oracle import skyvis_oracle as O, c_oracle as CO
from prisim_amd import _abi, layouts, workloads as W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = {_abi.PRISIM_FP64: 1e-11, _abi.PRISIM_FP32: 5e-6}
C = 299792458.0
ZEN = NP.array([0.0, 0.0, 1.0])
NCHAN = 128
CH = 150e6 + (NP.arange(NCHAN) - 64) * 97656.25
NSRC = 250
F32 = _abi.PRISIM_FP32
SLOTS = (0, 1, 2, 0, 1)           # where the five queued snapshots go
LANDED = {0: 3, 1: 4, 2: 2}       # slot -> the snapshot it holds at the end


def relerr(v, ref, pb):
    return float(NP.max(NP.abs(v - ref) / O.abs_flux_sum(pb)[None, :]))


def numpy_fold(bl):
    """(first row of every distinct vector in first-appearance order, entry of every row): numpy.unique(axis=0), -0.0 == +0.0."""
    b = NP.asarray(bl, dtype=NP.float64) + 0.0
    _, first, inv = NP.unique(b, axis=0, return_index=True, return_inverse=True)
    order = NP.argsort(first)
    rank = NP.empty(order.size, dtype=NP.int64)
    rank[order] = NP.arange(order.size)
    return first[order], rank[NP.asarray(inv).ravel()]


def point_sky(rng, nsrc, alt_lo=10.0):
    alt = NP.degrees(NP.arcsin(rng.uniform(NP.sin(NP.radians(alt_lo)), 1.0, nsrc)))
    dc = O.altaz2dircos(NP.stack((alt, rng.uniform(0, 360, nsrc)), axis=1))
    pb = rng.uniform(0.5, 10.0, size=(nsrc, 1)) * rng.uniform(0.5, 1.0, size=(nsrc, NCHAN))
    return dc, pb


@pytest.fixture(scope='module')
def hera61():
    """HERA-61 and five seeded skies; the oracle cube of the three that are still in a slot at the end, and the oracle gradient of
    sky 0, each computed once."""
    bl = layouts.layout_baselines('HERA-61')[0]
    rep, fmap = numpy_fold(bl)
    assert bl.shape[0] == 1830 and rep.size == 477
    skies = [point_sky(NP.random.default_rng(6100 + t), NSRC) for t in range(5)]
    ref = {t: CO.skyvis(bl, CH, skies[t][0], skies[t][1], ZEN) for t in sorted(set(LANDED.values()))}
    ref0, gref0 = CO.skyvis(bl, CH, skies[0][0], skies[0][1], ZEN, gradient=True)
    ref[0] = ref0
    return {'bl': bl, 'rep': rep, 'map': fmap, 'skies': skies, 'ref': ref, 'gref0': gref0}


@pytest.fixture()
def split3(ctx, hera61):
    """the context on HERA-61 with three slots and the tuning that makes partial cubes; the planner's own tuning again afterwards"""
    ctx.set_array(hera61['bl'], CH, nt_max=3)
    ctx.set_tuning(64, 0, 3)
    try:
        yield ctx
    finally:
        ctx.sync()
        ctx.set_tuning(0, 0, 0)


def deferred_shape(tm, nu):
    """what makes a compute() deferrable was in force: folded rows, more than one split, the 64-channel tile"""
    return tm['last_sum_baselines'] == nu and tm['last_nsplit'] > 1 and tm['last_chan_tile'] == 64


_CHILD = r'''
import sys
import numpy as NP
from prisim_amd import _abi
d = NP.load(sys.argv[1])
slots = [int(s) for s in d['slots']]
with _abi.Context(0) as ctx:
    ctx.set_array(d['bl'], d['ch'], nt_max=3)
    ctx.set_tuning(64, 0, 3)
    for t, slot in enumerate(slots):
        ctx.set_sky(d['dc'][t], d['pb'][t], d['pc'])
        ctx.compute(precision=_abi.PRISIM_FP32, slot=slot)
    ctx.sync()
    tm = ctx.timing()
    NP.save(sys.argv[2], NP.stack([ctx.get_vis(slot=s) for s in range(3)]))
print('PLAN %d %d' % (tm['last_sum_baselines'], tm['last_nsplit']))
'''


def test_queued_snapshots_equal_the_single_stream_order(split3, hera61, tmp_path):
    """Five snapshots into slots 0, 1, 2, 0, 1, a different sky before each, nothing waited for until the end: every slot holds, bit
    for bit, what the same sequence leaves in a fresh process with PRISIM_HIP_DEFER_POST=0, and every row is the oracle's."""
    ctx, h = split3, hera61
    for t, slot in enumerate(SLOTS):
        ctx.set_sky(h['skies'][t][0], h['skies'][t][1], ZEN)
        ctx.compute(precision=F32, slot=slot)
    ctx.sync()
    assert deferred_shape(ctx.timing(), h['rep'].size), ctx.timing()
    got = [ctx.get_vis(slot=s) for s in range(3)]
    inp, outp = str(tmp_path / 'in.npz'), str(tmp_path / 'vis.npy')
    NP.savez(inp, bl=h['bl'], ch=CH, dc=NP.stack([s[0] for s in h['skies']]), pb=NP.stack([s[1] for s in h['skies']]), pc=ZEN,
             slots=NP.array(SLOTS))
    env = dict(os.environ, PRISIM_HIP_DEFER_POST='0', PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    res = subprocess.run([sys.executable, '-c', _CHILD, inp, outp], env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    line = [ln for ln in res.stdout.splitlines() if ln.startswith('PLAN')][-1].split()
    assert int(line[1]) == h['rep'].size and int(line[2]) > 1
    serial = NP.load(outp)
    for slot, t in LANDED.items():
        assert NP.array_equal(got[slot], serial[slot]), 'slot %d differs from the single-stream order' % slot
        assert NP.array_equal(got[slot], got[slot][h['rep']][h['map']])
        err = relerr(got[slot], h['ref'][t], h['skies'][t][1])
        print('slot %d (snapshot %d): max err / S_f = %.3e' % (slot, t, err))
        assert err <= TOL[F32]


def test_partial_sets_are_reused_two_computes_later(split3, hera61):
    """four queued computes of one sky into one slot: the third writes the partial set the first one's reduction read"""
    ctx, h = split3, hera61
    dc, pb = h['skies'][0]
    ctx.set_sky(dc, pb, ZEN)
    ctx.compute(precision=F32, slot=0)
    ctx.sync()
    once = ctx.get_vis(slot=0)
    for _ in range(4):
        ctx.compute(precision=F32, slot=0)
    four = ctx.get_vis(slot=0)
    assert deferred_shape(ctx.timing(), h['rep'].size), ctx.timing()
    assert NP.array_equal(four, once)
    assert relerr(once, h['ref'][0], pb) <= TOL[F32]


def test_readers_right_behind_a_queued_compute(split3, hera61):
    """get_vis, phase_rotate and delay_transform_device issued with no sync behind a compute(): each gives what it gives behind a
    sync, bit for bit"""
    ctx, h = split3, hera61
    dc, pb = h['skies'][0]
    diff = (O.altaz2dircos(NP.array([[80.0, 30.0]]))[0] - ZEN)[None, :]

    def fresh(sync):
        ctx.set_vis(NP.zeros((1830, NCHAN), dtype=NP.complex128), slot=0)      # (no reader may see the previous round's slot)
        ctx.set_sky(dc, pb, ZEN)
        ctx.compute(precision=F32, slot=0)
        if sync:
            ctx.sync()

    out = {}
    for sync in (True, False):
        fresh(sync)
        vis = ctx.get_vis(slot=0)
        fresh(sync)
        ctx.phase_rotate(1, diff)
        rot = ctx.get_vis(slot=0)
        fresh(sync)
        ctx.delay_transform_device(1, want_lag=True)
        lag = ctx.get_lags(0, 1)
        out[sync] = (vis, rot, lag)
    for name, a, b in zip(('get_vis', 'phase_rotate', 'delay_transform_device'), out[True], out[False]):
        assert NP.array_equal(a, b), name
    assert relerr(out[False][0], h['ref'][0], pb) <= TOL[F32]
    want = h['ref'][0] * NP.exp(-2j * NP.pi * CH[None, :] * (h['bl'] @ diff[0])[:, None] / C)       # interferometry.py:7871-7877
    assert relerr(out[False][1], want, pb) <= TOL[F32]
    assert NP.max(NP.abs(out[False][2])) > 0.0


def repeated_array(rng, nvec, nrows, lengths):
    """nrows rows carrying nvec distinct vectors of the given lengths, multiplicities 1 ... 9, sorted by length up to a local shuffle"""
    mult = NP.ones(nvec, dtype=NP.int64)
    mult[:9] = NP.arange(1, 10)
    while mult.sum() < nrows:
        i = int(rng.integers(nvec))
        if mult[i] < 9:
            mult[i] += 1
    ang = rng.uniform(0, 2 * NP.pi, nvec)
    vec = NP.stack((lengths * NP.cos(ang), lengths * NP.sin(ang), 0.004 * lengths * rng.uniform(-1, 1, nvec)), axis=1)
    idx = NP.repeat(NP.arange(nvec), mult)
    idx = idx[NP.argsort(idx + rng.uniform(-3.0, 3.0, idx.size), kind='stable')]
    return vec[idx]


@pytest.fixture(scope='module')
def mixed():
    """the 700-row array of the fold tests (300 vectors, multiplicities 1 ... 9) under 300 point sources + the nside-8 diffuse half
    (two source runs, taper on), and its oracle cube"""
    rng = NP.random.default_rng(700)
    lengths = NP.concatenate((NP.sort(rng.uniform(5.0, 200.0, 264)), NP.sort(rng.uniform(700.0, 1500.0, 36))))
    bl = repeated_array(rng, 300, 700, lengths)
    rep, fmap = numpy_fold(bl)
    assert rep.size == 300
    dc_p, pb_p = point_sky(rng, 300, alt_lo=8.0)
    dif = W.diffuse_sky(8, 3)
    nd = dif['dircos'].shape[0]
    dc = NP.concatenate((dc_p, dif['dircos']))
    pb = NP.concatenate((pb_p, rng.uniform(0.5, 10.0, size=(nd, 1)) * rng.uniform(0.5, 1.0, size=(nd, NCHAN))))
    fw = NP.concatenate((NP.zeros(300), dif['fwhm_deg']))
    return {'bl': bl, 'rep': rep, 'map': fmap, 'dc': dc, 'pb': pb, 'fw': fw, 'ref': CO.skyvis(bl, CH, dc, pb, ZEN, fwhm_deg=fw)}


def test_undeferred_computes_right_behind_a_deferred_one(split3, hera61, mixed):
    """a deferred compute() followed directly -- no sync -- by a gradient compute, by an nsplit = 1 compute, and by a second set_array
    (the mixed 700-row array): results and last_sum_baselines as in the fold tests"""
    ctx, h, m = split3, hera61, mixed
    dc, pb = h['skies'][0]
    nu = h['rep'].size
    ctx.set_sky(dc, pb, ZEN)
    # the gradient (never deferred: it reduces nothing and expands four planes) into the slot the deferred post-pass is writing
    ctx.compute(precision=F32, slot=0)
    ctx.compute(precision=F32, slot=0, want_grad=True)
    tm = ctx.timing()
    assert tm['last_sum_baselines'] == nu, tm
    vis, grad = ctx.get_vis(slot=0, want_grad=True)
    assert NP.array_equal(vis, vis[h['rep']][h['map']]) and NP.array_equal(grad, grad[:, h['rep']][:, h['map']])
    errs = [relerr(vis, h['ref'][0], pb)] + [relerr(grad[c], h['gref0'][c], pb) for c in range(3)]
    print('gradient behind a deferred compute: max err / S_f = %.3e (V) %.3e %.3e %.3e (grad)' % tuple(errs))
    assert max(errs) <= TOL[F32], errs
    # one split: the sky-sum writes the compact buffer itself, which the deferred reduction before it also writes
    ctx.set_sky(h['skies'][2][0], h['skies'][2][1], ZEN)
    ctx.compute(precision=F32, slot=1)
    ctx.set_tuning(64, 0, 1)
    ctx.set_sky(h['skies'][3][0], h['skies'][3][1], ZEN)
    ctx.compute(precision=F32, slot=1)
    tm = ctx.timing()
    assert tm['last_sum_baselines'] == nu and tm['last_nsplit'] == 1, tm
    one = ctx.get_vis(slot=1)
    assert NP.array_equal(one, one[h['rep']][h['map']])
    assert relerr(one, h['ref'][3], h['skies'][3][1]) <= TOL[F32]
    # a second set_array behind a queued deferred compute: the map, the compact buffer and the cube are replaced under it
    ctx.set_tuning(64, 0, 3)
    ctx.set_sky(dc, pb, ZEN)
    ctx.compute(precision=F32, slot=2)
    ctx.set_array(m['bl'], CH)
    ctx.set_tuning(0, 0, 0)
    ctx.set_sky(m['dc'], m['pb'], ZEN, fwhm_deg=m['fw'])
    for prec in (F32, _abi.PRISIM_FP64):
        ctx.compute(precision=prec)
        tm = ctx.timing()
        assert tm['last_sum_baselines'] == 300 and tm['last_nsplit'] > 1, tm
        mv = ctx.get_vis()
        assert NP.array_equal(mv, mv[m['rep']][m['map']])
        err = relerr(mv, m['ref'], m['pb'])
        print('700 rows / 300 vectors behind a deferred compute, prec %d: max err / S_f = %.3e' % (prec, err))
        assert err <= TOL[prec]


def test_timing_spans_the_expansion_and_other_slots_keep_their_fill(split3, hera61):
    ctx, h = split3, hera61
    rng = NP.random.default_rng(3)
    fill = [rng.normal(size=(1830, NCHAN)) + 1j * rng.normal(size=(1830, NCHAN)) for _ in range(3)]
    for t in range(3):
        ctx.set_vis(fill[t], slot=t)
    dc, pb = h['skies'][0]
    ctx.set_sky(dc, pb, ZEN)
    ctx.compute(precision=F32, slot=1)
    ctx.compute(precision=F32, slot=1)
    ctx.sync()
    tm = ctx.timing()
    assert deferred_shape(tm, h['rep'].size), tm
    print('last_compute_ms %.4f, last_kernel_ms %.4f' % (tm['last_compute_ms'], tm['last_kernel_ms']))
    assert tm['last_compute_ms'] >= tm['last_kernel_ms'] > 0.0, tm
    assert NP.array_equal(ctx.get_vis(slot=0), fill[0]) and NP.array_equal(ctx.get_vis(slot=2), fill[2])
    assert relerr(ctx.get_vis(slot=1), h['ref'][0], pb) <= TOL[F32]
