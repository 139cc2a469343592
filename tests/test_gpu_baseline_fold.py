"""GPU (-m gpu): baseline folding.  prisim_hip_set_array maps rows of equal baseline vectors onto one entry (baseline_fold.h); compute()
sums every distinct vector once into a compact buffer and k_expand_rows copies compact row map[b] into cube row b (and into the three
gradient planes).  Every cube row is checked against the C oracle at the project's tolerances, relative to S_f = sum_s |pbflux[s, f]|:
5e-6 for fp32, 1e-11 for fp64."""
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


def repeated_array(rng, nvec, nrows, lengths):
    """nrows rows carrying nvec distinct vectors of the given lengths (one per vector, ascending) with multiplicities 1 ... 9, in an
    order that is sorted by length up to a local shuffle -- so the first-appearance order of the vectors stays near the length order."""
    mult = NP.ones(nvec, dtype=NP.int64)
    mult[:9] = NP.arange(1, 10)
    while mult.sum() < nrows:
        i = int(rng.integers(nvec))
        if mult[i] < 9:
            mult[i] += 1
    assert mult.sum() == nrows and mult.min() == 1 and mult.max() == 9
    ang = rng.uniform(0, 2 * NP.pi, nvec)
    vec = NP.stack((lengths * NP.cos(ang), lengths * NP.sin(ang), 0.004 * lengths * rng.uniform(-1, 1, nvec)), axis=1)
    idx = NP.repeat(NP.arange(nvec), mult)
    idx = idx[NP.argsort(idx + rng.uniform(-3.0, 3.0, idx.size), kind='stable')]
    return vec[idx], mult


@pytest.fixture(scope='module')
def hera61():
    """HERA-61 x 128 channels x 300 point sources and its oracle cube, computed once."""
    bl = layouts.layout_baselines('HERA-61')[0]
    rep, fmap = numpy_fold(bl)
    dc, pb = point_sky(NP.random.default_rng(61), 300)
    return {'bl': bl, 'rep': rep, 'map': fmap, 'dc': dc, 'pb': pb, 'ref': CO.skyvis(bl, CH, dc, pb, ZEN)}


def test_hera61_fp32_rows_counts_and_oracle(ctx, hera61):
    h = hera61
    nu = h['rep'].size
    assert h['bl'].shape[0] == 1830 and nu > 256 and nu % 64 != 0 and nu * 8 <= 1830 * 7          # folded; a ragged last wavefront
    ctx.set_array(h['bl'], CH)
    ctx.set_tuning(0, 0, 0)
    ctx.set_sky(h['dc'], h['pb'], ZEN)
    ctx.compute(precision=_abi.PRISIM_FP32)
    tm = ctx.timing()
    vis = ctx.get_vis()
    assert tm['last_sum_baselines'] == nu, tm
    assert tm['last_terms'] == 1830 * NCHAN * 300 and tm['last_terms_evaluated'] == nu * NCHAN * 300, tm
    # lifting groups: in groups of 256 cube rows for the caller, in groups of 256 summed rows as the kernel flags them (HERA-61's 117 m
    # under a sky down to 10 deg of altitude: 117 x 1.29 x 97.7 kHz / c = 0.05 cycle, every group lifts)
    assert tm['last_lift_groups'] == (1830 + 255) // 256 and tm['last_sum_lift_groups'] == (nu + 255) // 256, tm
    assert NP.array_equal(vis, vis[h['rep']][h['map']])              # rows that share a vector are equal element for element
    err = relerr(vis, h['ref'], h['pb'])
    print('HERA-61 fp32 folded (%d of 1830 rows summed): max err / S_f = %.3e' % (nu, err))
    assert err <= TOL[_abi.PRISIM_FP32]


_CHILD = r'''
import sys
import numpy as NP
from prisim_amd import _abi
d = NP.load(sys.argv[1])
with _abi.Context(0) as ctx:
    ctx.set_array(d['bl'], d['ch'])
    ctx.set_sky(d['dc'], d['pb'], d['pc'])
    ctx.compute(precision=_abi.PRISIM_FP32)
    tm = ctx.timing()
    NP.save(sys.argv[2], ctx.get_vis())
print('SUM_BASELINES %d %d' % (tm['last_sum_baselines'], tm['last_terms_evaluated']))
'''


def test_hera61_fold_off_in_a_fresh_process(ctx, hera61, tmp_path):
    """PRISIM_HIP_FOLD=0 (read by set_array): every row is summed.  The cubes agree within the tolerance, not bit for bit -- a vector's
    group of 256, and so the kernel body it runs, changes with the folding."""
    h = hera61
    ctx.set_array(h['bl'], CH)
    ctx.set_tuning(0, 0, 0)
    ctx.set_sky(h['dc'], h['pb'], ZEN)
    ctx.compute(precision=_abi.PRISIM_FP32)
    folded = ctx.get_vis()
    assert ctx.timing()['last_sum_baselines'] == h['rep'].size
    inp, outp = str(tmp_path / 'in.npz'), str(tmp_path / 'vis.npy')
    NP.savez(inp, bl=h['bl'], ch=CH, dc=h['dc'], pb=h['pb'], pc=ZEN)
    env = dict(os.environ, PRISIM_HIP_FOLD='0', PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    res = subprocess.run([sys.executable, '-c', _CHILD, inp, outp], env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    line = [ln for ln in res.stdout.splitlines() if ln.startswith('SUM_BASELINES')][-1].split()
    assert int(line[1]) == 1830 and int(line[2]) == 1830 * NCHAN * 300
    unfolded = NP.load(outp)
    assert relerr(unfolded, h['ref'], h['pb']) <= TOL[_abi.PRISIM_FP32]
    diff = relerr(folded, unfolded, h['pb'])
    print('HERA-61 fp32: folded vs PRISIM_HIP_FOLD=0: max diff / S_f = %.3e' % diff)
    assert diff <= TOL[_abi.PRISIM_FP32]


@pytest.fixture(scope='module')
def mixed():
    """700 rows from 300 vectors (multiplicities 1 ... 9) whose lengths lie on both sides of the lift limit of both precisions;
    300 point sources + the nside-8 diffuse half (two source runs, taper on); oracle V and gradient on every row, computed once."""
    rng = NP.random.default_rng(700)
    lengths = NP.concatenate((NP.sort(rng.uniform(5.0, 200.0, 264)), NP.sort(rng.uniform(700.0, 1500.0, 36))))
    bl, mult = repeated_array(rng, 300, 700, lengths)
    rep, fmap = numpy_fold(bl)
    assert rep.size == 300 and 300 * 8 <= 700 * 7
    dc_p, pb_p = point_sky(rng, 300, alt_lo=8.0)
    dif = W.diffuse_sky(8, 3)
    nd = dif['dircos'].shape[0]
    dc = NP.concatenate((dc_p, dif['dircos']))
    pb = NP.concatenate((pb_p, rng.uniform(0.5, 10.0, size=(nd, 1)) * rng.uniform(0.5, 1.0, size=(nd, NCHAN))))
    fw = NP.concatenate((NP.zeros(300), dif['fwhm_deg']))
    # the lift limit (max|b| of a group of 256 SUMMED rows x max|s - s_pc| x |df| / c against 1/8 cycle in fp32, 1/4 in fp64): the
    # first group of distinct vectors is under it, the ragged second group over it, in both precisions
    k = float(NP.linalg.norm(dc - ZEN[None, :], axis=1).max()) * 97656.25 / C
    ulen = NP.linalg.norm(bl[rep], axis=1)
    assert ulen[:256].max() * k < 0.125 and ulen[256:].max() * k > 0.25
    ref, gref = CO.skyvis(bl, CH, dc, pb, ZEN, fwhm_deg=fw, gradient=True)
    return {'bl': bl, 'rep': rep, 'map': fmap, 'dc': dc, 'pb': pb, 'fw': fw, 'ref': ref, 'gref': gref}


@pytest.mark.parametrize('prec', [_abi.PRISIM_FP32, _abi.PRISIM_FP64], ids=['fp32', 'fp64'])
def test_irregular_multiplicities_mixed_sky_with_gradient(ctx, mixed, prec):
    m = mixed
    ctx.set_array(m['bl'], CH)
    ctx.set_tuning(0, 0, 0)
    ctx.set_sky(m['dc'], m['pb'], ZEN, fwhm_deg=m['fw'])
    ctx.compute(precision=prec)                                       # the planner's source split: partial cubes of the compact size
    tm = ctx.timing()
    assert tm['last_sum_baselines'] == 300 and tm['last_nsplit'] > 1, tm
    vis = ctx.get_vis()
    assert NP.array_equal(vis, vis[m['rep']][m['map']])
    err = relerr(vis, m['ref'], m['pb'])
    ctx.compute(precision=prec, want_grad=True)
    assert ctx.timing()['last_sum_baselines'] == 300
    vis, grad = ctx.get_vis(want_grad=True)
    assert NP.array_equal(grad, grad[:, m['rep']][:, m['map']])
    errs = [relerr(vis, m['ref'], m['pb'])] + [relerr(grad[c], m['gref'][c], m['pb']) for c in range(3)]
    print('700 rows / 300 vectors, prec %d: max err / S_f = %.3e (split), %.3e (V) %.3e %.3e %.3e (grad)' % ((prec, err) + tuple(errs)))
    assert err <= TOL[prec]
    assert max(errs) <= TOL[prec], errs
    assert NP.max(NP.abs(m['gref'][2])) > 0.0


def test_flushes_and_accumulating_launches_land_in_the_compact_buffer(ctx, mixed, monkeypatch):
    """PRISIM_HIP_FLUSH_SRC=64: the fp32 accumulators are flushed by read-modify-write every 64 sources (the generic and the packed
    kernel; the sources split and in one piece).  fp64 on 32-channel tiles with one split (the grouped taper kernel) runs the sky run
    by run: the diffuse run's launch accumulates onto the point sources' -- all of it in the compact buffer, never in the slot."""
    m = mixed
    monkeypatch.setenv('PRISIM_HIP_FLUSH_SRC', '64')
    ctx.set_array(m['bl'], CH)
    ctx.set_sky(m['dc'], m['pb'], ZEN, fwhm_deg=m['fw'])
    try:
        for prec, ct, nsplit in ((_abi.PRISIM_FP32, 0, 0), (_abi.PRISIM_FP32, 0, 1), (_abi.PRISIM_FP32, 64, 1), (_abi.PRISIM_FP64, 32, 1)):
            ctx.set_tuning(ct, 0, nsplit)
            ctx.compute(precision=prec)
            tm = ctx.timing()
            assert tm['last_sum_baselines'] == 300 and (nsplit == 0 or tm['last_nsplit'] == 1) and (ct == 0 or tm['last_chan_tile'] == ct), tm
            vis = ctx.get_vis()
            assert NP.array_equal(vis, vis[m['rep']][m['map']])
            err = relerr(vis, m['ref'], m['pb'])
            print('700 rows / 300 vectors, prec %d, flush every 64 sources, tile %d, nsplit %d: max err / S_f = %.3e'
                  % (prec, tm['last_chan_tile'], tm['last_nsplit'], err))
            assert err <= TOL[prec]
    finally:
        ctx.set_tuning(0, 0, 0)


def test_expansion_writes_only_the_addressed_slot(ctx, mixed):
    m = mixed
    rng = NP.random.default_rng(3)
    ctx.set_array(m['bl'], CH, nt_max=3)
    ctx.set_tuning(0, 0, 0)
    fill = [rng.normal(size=(700, NCHAN)) + 1j * rng.normal(size=(700, NCHAN)) for _ in range(3)]
    for t in range(3):
        ctx.set_vis(fill[t], slot=t)
    ctx.set_sky(m['dc'], m['pb'], ZEN, fwhm_deg=m['fw'])
    ctx.compute(precision=_abi.PRISIM_FP32, slot=1)
    assert ctx.timing()['last_sum_baselines'] == 300
    assert NP.array_equal(ctx.get_vis(slot=0), fill[0]) and NP.array_equal(ctx.get_vis(slot=2), fill[2])
    assert relerr(ctx.get_vis(slot=1), m['ref'], m['pb']) <= TOL[_abi.PRISIM_FP32]


@pytest.mark.parametrize('nrows, nvec', [(600, 590), (400, 200)], ids=['more_than_7_8_distinct', 'at_most_256_distinct'])
def test_folding_stays_off(ctx, nrows, nvec):
    rng = NP.random.default_rng(nrows)
    vec = rng.uniform(-150.0, 150.0, (nvec, 3)) * NP.array([1.0, 1.0, 0.01])
    bl = NP.concatenate((vec, vec[rng.integers(nvec, size=nrows - nvec)]))
    assert numpy_fold(bl)[0].size == nvec
    dc, pb = point_sky(rng, 200)
    ctx.set_array(bl, CH)
    ctx.set_tuning(0, 0, 0)
    ctx.set_sky(dc, pb, ZEN)
    ctx.compute(precision=_abi.PRISIM_FP32)
    tm = ctx.timing()
    assert tm['last_sum_baselines'] == nrows and tm['last_terms_evaluated'] == tm['last_terms'] == nrows * NCHAN * 200, tm
    assert relerr(ctx.get_vis(), CO.skyvis(bl, CH, dc, pb, ZEN), pb) <= TOL[_abi.PRISIM_FP32]


def test_second_set_array_replaces_the_map(ctx, hera61, mixed):
    h, m = hera61, mixed
    ctx.set_tuning(0, 0, 0)
    ctx.set_array(m['bl'], CH)
    ctx.set_sky(h['dc'], h['pb'], ZEN)
    ctx.compute(precision=_abi.PRISIM_FP32)
    assert ctx.timing()['last_sum_baselines'] == 300
    ctx.set_array(h['bl'], CH)
    ctx.set_sky(h['dc'], h['pb'], ZEN)
    ctx.compute(precision=_abi.PRISIM_FP32)
    assert ctx.timing()['last_sum_baselines'] == h['rep'].size
    vis = ctx.get_vis()
    assert NP.array_equal(vis, vis[h['rep']][h['map']])
    assert relerr(vis, h['ref'], h['pb']) <= TOL[_abi.PRISIM_FP32]
    # ... and back to an array that does not fold at all
    bl = h['bl'][h['rep']]
    ctx.set_array(bl, CH)
    ctx.set_sky(h['dc'], h['pb'], ZEN)
    ctx.compute(precision=_abi.PRISIM_FP32)
    assert ctx.timing()['last_sum_baselines'] == bl.shape[0]
    assert relerr(ctx.get_vis(), h['ref'][h['rep']], h['pb']) <= TOL[_abi.PRISIM_FP32]


def test_phase_rotate_after_a_folded_compute(ctx, hera61):
    """phase_rotate reads the whole baseline arrays per cube row: after a folded compute() it gives what it gives on the unfolded rows
    (here: the distinct vectors as an array of their own, which does not fold), and the oracle's cube times the rotation."""
    h = hera61
    pc2 = O.altaz2dircos(NP.array([[80.0, 30.0]]))[0]
    diff = (pc2 - ZEN)[None, :]
    ctx.set_tuning(0, 0, 0)
    ctx.set_array(h['bl'], CH)
    ctx.set_sky(h['dc'], h['pb'], ZEN)
    ctx.compute(precision=_abi.PRISIM_FP64)
    assert ctx.timing()['last_sum_baselines'] == h['rep'].size
    ctx.phase_rotate(1, diff)
    rot = ctx.get_vis()
    ctx.set_array(h['bl'][h['rep']], CH)
    ctx.set_sky(h['dc'], h['pb'], ZEN)
    ctx.compute(precision=_abi.PRISIM_FP64)
    assert ctx.timing()['last_sum_baselines'] == h['rep'].size
    ctx.phase_rotate(1, diff)
    rot_u = ctx.get_vis()
    assert relerr(rot, rot_u[h['map']], h['pb']) <= TOL[_abi.PRISIM_FP64]
    want = h['ref'] * NP.exp(-2j * NP.pi * CH[None, :] * (h['bl'] @ diff[0])[:, None] / C)       # interferometry.py:7871-7877
    assert relerr(rot, want, h['pb']) <= 2 * TOL[_abi.PRISIM_FP64]                              # (the sum's error + the rotation's)
