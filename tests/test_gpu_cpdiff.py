"""GPU: the differences of day sub-samples (prisim_cphase_diff, prisim_amd.bispectrum_phase.ClosurePhase.subsample_differencing)
against the numpy.ma checker and tests/golden/golden_cpdiff.npz (the reference's statements executed), every case of the fixture;
the resident route; chunking over the triad axis; the refusals of the entry.

What is compared, and the bounds, in units of u = 2^-53 (tests/cpdiff_checker.py:compare_errinfo holds them).

- Masks: equal.  Values are compared only where the mask is False; under it the device writes 0 for the differences, which must be
  finite.
- Weights: the binned weights are sums of 0 / 1, so their squares and the sum of two squares are exact in fp64 and the only rounding
  is the square root's: 1 ulp, i.e. a relative 2 u, should the device's root not round as numpy's does.
- Differences with the same member phases on both sides (the entry fed the checker's own binned stack): a side takes one sincos per
  member, each component within 2 u of the true value (the two libraries' cos / sin differ by at most 4 u), subtracts component by
  component (1 u of a value <= 2 per side, 2 u between the sides after the halving, which is exact), so a component differs by
  0.5 (4 u + 4 u) + 2 u between the sides: DIFF_CONST = 6 u, taken for the complex number as well, as the phasor bounds below are.
- Differences against the fixture: the member phases themselves differ, by the per-element phasor bound B of
  tests/cphase_bins_checker.py:compare -- phasor_bound(nbin, |Z|), plus e1 / |Z| after two passes, e1 the largest bound of the
  first pass -- so a difference of members a, b moves by 0.5 (B_a + B_b) more.
- Elements of which one of the four members is ill-conditioned (|Z| < 0.05 in either pass) are left out of the comparison of the
  differences and must be finite; they may be 2 % of the unmasked elements at most (the fixture has none).
"""
import ctypes as C
import os
import sys
import warnings

import numpy as NP
import numpy.ma as MA
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cpdiff_checker as DK  # noqa: E402

from prisim_amd import _abi  # noqa: E402
from prisim_amd import bispectrum_phase as BSP  # noqa: E402

NAMES = [c[0] for c in DK.cases()]
pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    with _abi.Context(0) as c:
        yield c


@pytest.mark.parametrize('name', NAMES)
def test_entry_against_the_checker(ctx, name):
    """the checker's own binned stack through prisim_cphase_diff from host arrays, against the checker's differences"""
    err, detail = DK.reference(name)
    pairs = err['list_of_pair_of_pairs']
    res = ctx.cphase_diff(pairs, binned=detail['binned'])
    st = res['stats']
    n0, _, nt, nc = detail['binned'][0].shape
    assert st['chunks'] == 1 and not st['resident'] and st['ncomb'] == len(pairs) and st['elements'] == n0 * len(pairs) * nt * nc
    assert st['upload_bytes'] == len(pairs) * 16 + detail['binned'][0].size * 24
    assert st['download_bytes'] == st['elements'] * _abi.PRISIM_CPDIFF_OUT_BYTES
    for name_ in _abi.CPDIFF_OUTPUTS:
        want = NP.complex128 if name_.startswith('diff') else (NP.float64 if name_.startswith('wts') else NP.bool_)
        assert res[name_].dtype == want and res[name_].shape == (n0, len(pairs), nt, nc), name_
    ref = DK.diff_step(*detail['binned'], pairs)
    for g in range(2):
        assert NP.array_equal(res['mask%d' % g], ref['mask%d' % g])
        m = ref['mask%d' % g]
        for s in ('mean', 'median'):
            assert NP.all(res['diff%d_%s' % (g, s)][m] == 0)
        equal = NP.array_equal(res['wts%d' % g], ref['wts%d' % g])
        print('%s wts %d: device square root %s numpy' % (name, g, 'equals' if equal else 'DIFFERS FROM'))
    got = dict(DK.errinfo_of(res), list_of_pair_of_pairs=pairs)
    DK.compare_errinfo(got, err, detail, label=name + ' entry', exact_members=True)


def many_pairs(n1, count, step):
    """`count` valid rows (i != j, k != m, not necessarily disjoint: the entry takes any) out of all ordered pairs of pairs of n1
    indices, every step-th: neighbouring rows share some indices and change others, as the kernel's register cache expects"""
    ordered = [(i, j) for i in range(n1) for j in range(n1) if i != j]
    rows = [[p[0], p[1], q[0], q[1]] for p in ordered for q in ordered][::step][:count]
    assert len(rows) == count
    return rows


@pytest.mark.parametrize('name,count,step', [('nd5_lst', 41, 9), ('nd4_lst_67', 37, 3), ('onelst', 16, 5), ('onelst', 17, 5)])
def test_entry_with_more_pairs_than_one_run(ctx, name, count, step):
    """pair lists longer than one thread's run of 16 and no multiple of it (and exactly one run, and one more): several runs per row,
    a short last run, the members taken anew at every run's start.  From host arrays, against the checker's differences."""
    err, detail = DK.reference(name)
    binned = detail['binned']
    n0, n1, nt, nc = binned[0].shape
    pairs = many_pairs(n1, count, step)
    res = ctx.cphase_diff(pairs, binned=binned)
    assert res['stats']['ncomb'] == count and res['stats']['elements'] == n0 * count * nt * nc and res['stats']['chunks'] == 1
    ref = DK.diff_step(*binned, pairs)
    for g in range(2):
        assert NP.array_equal(res['mask%d' % g], ref['mask%d' % g])
        for s in ('mean', 'median'):
            assert NP.all(res['diff%d_%s' % (g, s)][ref['mask%d' % g]] == 0)
    got = dict(DK.errinfo_of(res), list_of_pair_of_pairs=pairs)
    want = dict(DK.errinfo_of(ref), list_of_pair_of_pairs=pairs)
    DK.compare_errinfo(got, want, detail, label='%s %d pairs' % (name, count), exact_members=True)


@pytest.mark.parametrize('name', NAMES)
def test_subsample_differencing_against_the_reference(ctx, name):
    raw, nchan, kw = DK.case(name)
    err, detail = DK.reference(name)
    cp = BSP.ClosurePhase({'raw': {k: v.copy() for k, v in raw.items()}}, 150e6 + 1e5 * NP.arange(nchan), ctx=ctx)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        cp.subsample_differencing(**kw)
    got = cp.cpinfo['errinfo']
    ref = DK.gold_errinfo(name)
    assert sorted(got.keys()) == sorted(DK.gold()[name + '_keys'].tolist())
    for key in ('daybins', 'diff_dbins', 'lstbins', 'dlstbins'):
        assert NP.shape(got[key]) == ref[key].shape and NP.array_equal(got[key], ref[key]), key
    DK.compare_errinfo(got, ref, detail, label=name)
    # the resident route: the passes before the difference step copy nothing back and upload only their CSR tables; the difference
    # step uploads the pair table and downloads the eight outputs
    stats = cp.binning_stats
    two = 'lst' in detail
    assert len(stats) == 2 + two and all(s['resident'] for s in stats)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        plans = [BSP.day_bins(raw['days'], kw.get('daybinsize'), kw.get('ndaybins', 4))[2:4]]
        if two:
            plans.append(BSP.lst_bins(BSP.unwrapped_lst(raw['lst']), kw['lstbinsize'], raw['lst'].shape[0])[2:4])
    for s, (off, mem) in zip(stats, plans):
        assert s['download_bytes'] == 0 and s['upload_bytes'] == off.size * 8 + mem.size * 4
    ncomb = len(ref['list_of_pair_of_pairs'])
    last = stats[-1]
    assert last['ncomb'] == ncomb and last['elements'] == ref['wts']['0'].size and last['upload_bytes'] == ncomb * 16
    assert last['download_bytes'] == last['elements'] * (4 * 16 + 2 * 8 + 2 * 1)
    print('%s difference step: %d elements, kernel %.4f ms, %.1f GB/s of %d kernel bytes' % (
        name, last['elements'], last['kernel_ms'], last['kernel_bytes'] / max(last['kernel_ms'], 1e-9) / 1e6, last['kernel_bytes']))
    cp._drop_stack()


@pytest.mark.parametrize('count', [3, 37])
def test_three_chunks_equal_one(ctx, count):
    """a budget that holds one triad: three chunks over the triad axis, outputs bit-identical to one chunk, from a resident stack
    and from host arrays; with the fixture's 3 pairs of pairs and with 37, three runs per row of which the last is short"""
    err, detail = DK.reference('nd4_lst_67')
    binned = detail['binned']
    n0, n1, nt, nc = binned[0].shape
    pairs = err['list_of_pair_of_pairs'] if count == 3 else many_pairs(n1, count, 3)
    one = ctx.cphase_diff(pairs, binned=binned)
    out_per_triad = n0 * len(pairs) * nc * _abi.PRISIM_CPDIFF_OUT_BYTES
    three = ctx.cphase_diff(pairs, binned=binned, budget_bytes=n0 * n1 * nc * 24 + out_per_triad + 100)
    assert one['stats']['chunks'] == 1 and three['stats']['chunks'] == 3 and three['stats']['chunk_triads'] == 1
    # a resident stack of the same values: one single-member LST pass over the host arrays, kept
    off, mem = NP.arange(n0 + 1, dtype=NP.int64), NP.arange(n0, dtype=NP.int32)
    kept = ctx.cphase_bin(0, off, mem, binned=binned, want=('wts', 'cp_mean', 'cp_median'), keep=True)
    try:
        again = (kept['cp_mean'], kept['cp_median'], kept['wts'])
        r_one = ctx.cphase_diff(pairs, stack=kept['stack'])
        r_three = ctx.cphase_diff(pairs, stack=kept['stack'], budget_bytes=out_per_triad + 100)
        h_one = ctx.cphase_diff(pairs, binned=again)
    finally:
        kept['stack'].close()
    assert r_one['stats']['resident'] and r_one['stats']['chunks'] == 1 and r_three['stats']['chunks'] == 3
    assert r_three['stats']['upload_bytes'] == len(pairs) * 16
    for q in _abi.CPDIFF_OUTPUTS:
        assert NP.array_equal(one[q], three[q]), q
        assert NP.array_equal(r_one[q], r_three[q]) and NP.array_equal(r_one[q], h_one[q]), q


def test_five_triads_in_chunks_of_two_equal_one_chunk(ctx):
    """Five triads in chunks of 2, 2 and 1: the eight outputs bit for bit those of one chunk."""
    rng = NP.random.default_rng(81)
    n0, n1, ntriads, nchan = 2, 4, 5, 8
    shape = (n0, n1, ntriads, nchan)
    binned = (rng.uniform(-NP.pi, NP.pi, shape), rng.uniform(-NP.pi, NP.pi, shape), rng.integers(0, 3, shape).astype(NP.float64))
    pairs = NP.array([[0, 1, 2, 3], [0, 2, 1, 3]])
    per_triad = n0 * n1 * nchan * 24 + n0 * len(pairs) * nchan * _abi.PRISIM_CPDIFF_OUT_BYTES
    one = ctx.cphase_diff(pairs, binned=binned)
    three = ctx.cphase_diff(pairs, binned=binned, budget_bytes=2 * per_triad)
    assert one['stats']['chunks'] == 1 and three['stats']['chunks'] == 3 and three['stats']['chunk_triads'] == 2
    for q in _abi.CPDIFF_OUTPUTS:
        assert NP.array_equal(one[q], three[q]), q


def test_refusals(ctx):
    """argument checks made before any launch: PRISIM_EINVAL through the raw entry with the outputs found unchanged, ValueError
    through the binding"""
    err, detail = DK.reference('nd4_lst')
    binned = tuple(NP.ascontiguousarray(a) for a in detail['binned'])
    n0, n1, nt, nc = binned[0].shape
    lib = ctx._lib
    native = ctx.cphase_upload(NP.zeros((n0, n1, nt, nc)), NP.zeros((n0, n1, nt, nc), dtype=bool))

    def raw_call(pairs, stack=None, drop_output=None):
        pr = NP.ascontiguousarray(pairs, dtype=NP.int32).reshape(-1, 4)
        ncomb = pr.shape[0]
        outs = [NP.full((n0, max(ncomb, 1), nt, nc) + ((2,) if i < 4 else ()), 7, dtype=NP.uint8 if i >= 6 else NP.float64) for i in range(8)]
        ptrs = [None if i == drop_output else _abi._ptr(o) for i, o in enumerate(outs)]
        rc = lib.prisim_cphase_diff(ctx._h, *[_abi._ptr(a) for a in binned], n0, n1, nt, nc, None if stack is None else stack.handle,
                                    ncomb, _abi._ptr(pr), 0, *ptrs, None)
        assert all(NP.all(o == 7) for o in outs)
        return rc, lib.prisim_hip_last_error(ctx._h).decode()

    try:
        for pairs, stack, drop, text in (([[0, 1, 2, n1]], None, None, 'not an index of axis 1'),
                                         ([[0, 1, 2, 3], [-1, 1, 2, 3]], None, None, 'not an index of axis 1'),
                                         ([[1, 1, 2, 3]], None, None, 'a pair of one index with itself'),
                                         ([[0, 1, 3, 3]], None, None, 'a pair of one index with itself'),
                                         (NP.zeros((0, 4)), None, None, 'need ncomb >= 1'),
                                         ([[0, 1, 2, 3]], native, None, 'not of kind BINNED'),
                                         ([[0, 1, 2, 3]], None, 5, 'an output is NULL')):
            rc, msg = raw_call(pairs, stack, drop)
            assert rc == _abi.PRISIM_EINVAL and text in msg, (pairs, rc, msg)
            if drop is None:
                with pytest.raises(ValueError, match=text):
                    ctx.cphase_diff(pairs, stack=stack, binned=None if stack is not None else binned)
        # a BINNED stack of another shape than stated
        kept = ctx.cphase_bin(0, [0, 1], [0], binned=binned, want=(), keep=True)['stack']
        try:
            rc, msg = raw_call([[0, 1, 2, 3]], kept)
            assert rc == _abi.PRISIM_EINVAL and 'another shape' in msg
        finally:
            kept.close()
    finally:
        native.close()
    with pytest.raises(ValueError, match='must all be'):
        ctx.cphase_diff([[0, 1, 2, 3]], binned=(binned[0], binned[1], binned[2][:1]))
    # and the entry still works
    res = ctx.cphase_diff([[0, 1, 2, 3]], binned=binned)
    assert NP.array_equal(res['mask0'], DK.diff_step(*binned, [[0, 1, 2, 3]])['mask0'])
