"""GPU: the day and LST binning of closure phases (prisim_cphase_bin, prisim_amd.bispectrum_phase.ClosurePhase.smooth_in_tbins)
against tests/golden/golden_cphase.npz (the reference's statements executed) and the numpy.ma checker, every case of the fixture;
chunking over the triad axis; the resident two-pass route; the refusal of a bin above PRISIM_CPBINS_MAX_BIN.

What is compared, and the bounds, in units of u = 2^-53 (tests/cphase_bins_checker.py:compare holds them).  n is the number of
members of the bin, |Z| the modulus of the checker's mean (or median) phasor before normalisation, i.e. |z| / n of the phasor sum z.

- Weights and masks: equal.  The weights are sums of 0 / 1 in fp64, exact in any order.  Values are compared only where the mask is
  False: under it the reference leaves unspecified values; the device writes eicp = 1 and 0 elsewhere, which must be finite.
- Phasors (eicp and cphase, mean and median), as |exp(ia) - exp(ib)|.  Both sides sum the same members in the same order; their
  cos / sin differ by the two libraries' errors, at most 4 u together, and each sequential sum of n terms of modulus <= 1 carries at
  most (n - 1) u of its mean, so a component of Z differs by at most 4 u + 2 (n - 1) u, and by 2 u more for the division: (2 n + 4) u,
  times sqrt 2 for the complex number, < (4 n + 8) u.  For the median phasor a component is a selected value (or half the sum of two):
  an error of 4 u in the values moves it by no more, also where it changes which member is selected.  atan2 is conditioned by the
  modulus: the angle moves by (4 n + 8) u / |Z|.  What follows -- atan2 itself (2 ulp of pi: 8 u), the sincos of the angle (4 u per
  component) and the second atan2 (8 u) on each side -- adds at most 32 u.  Bound: (4 n + 8) u / |Z| + 32 u.
- rms: both sides hold the same phases, |phase| <= pi.  The mean of n of them carries (n - 1) u pi per side, a deviation from it
  2 u pi more, and the root of the mean of n squares (n + 2) u / 2 of a value <= 2 pi; together < (4 n + 8) u pi per pair of sides.
  For n <= 64 this is 9.2e-14, and never looser than 1e-12.
- mad: |phase - median angle| moves by the error of the median angle, the phasor bound, and carries 2 u 2 pi of rounding and the
  mean of two: (4 n + 8) u pi + the median phasor bound.
- A second pass over device products (day then LST) reads phases that differ from the checker's by e1, the largest phasor bound of the
  first pass: its phasors then move by e1 / |Z|, its rms and mad by 2 e1; this is added where the device result of two passes is
  compared to the fixture.  Against the checker run on the device's own first-pass products nothing is added.
- Points with |Z| < 0.05 are left out of the phasor and mad comparisons and must be finite; they may be 2 % of the unmasked points
  at most (the fixture's generator refuses more; the fixture has none).
"""
import json
import os
import sys
import warnings

import numpy as NP
import numpy.ma as MA
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cphase_bins_checker as CK  # noqa: E402

from prisim_amd import _abi  # noqa: E402
from prisim_amd import bispectrum_phase as BSP  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = NP.load(os.path.join(HERE, 'golden', 'golden_cphase.npz'))
CASES = json.loads(str(GOLD['cases']))
NAMES = [c[0] for c in CASES]
BINNED = [n for n in NAMES if n != 'none']
pytestmark = pytest.mark.gpu
_REF = {}


@pytest.fixture(scope='module')
def ctx():
    with _abi.Context(0) as c:
        yield c


def case(name):
    nchan, kw = [(c[1], c[2]) for c in CASES if c[0] == name][0]
    raw = {k: GOLD['%s_in_%s' % (name, k)] for k in ('cphase', 'flags', 'lst', 'days')}
    return raw, nchan, kw


def reference(name):
    """the checker's run of a case, computed once: (prelim, detail, bins of the day pass, bins of the LST pass)"""
    if name not in _REF:
        raw, nchan, kw = case(name)
        detail = {}
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            prelim = CK.smooth_in_tbins({'raw': raw}, detail=detail, **kw)
            day = BSP.day_bins(raw['days'], kw.get('daybinsize'), kw.get('ndaybins')) if 'day' in detail else None
            lst = BSP.lst_bins(BSP.unwrapped_lst(raw['lst']), kw['lstbinsize'], raw['lst'].shape[0]) if 'lst' in detail else None
        _REF[name] = (prelim, detail, day, lst)
    return _REF[name]


def gold_quantities(name):
    out = {}
    for q, path in CK.PASS_TO_PRELIM.items():
        key = name + '_out_' + '_'.join(path)
        out[q] = MA.array(GOLD[key], mask=GOLD[key + '__mask'])
    return out


def first_pass_error(detail):
    d = detail['day']
    return float(NP.max(CK.phasor_bound(d['nbin'], NP.minimum(d['mod_mean'], d['mod_median']))[d['wts'] > 0.0]))


def as_masked(res):
    mask = res['wts'] <= 0.0
    return {q: MA.array(res[q], mask=mask) for q in CK.QUANTITIES}


@pytest.mark.parametrize('name', BINNED)
def test_entry_against_the_checker_and_the_reference(ctx, name):
    """every pass of the case through prisim_cphase_bin from host arrays: against the checker's pass on the same input, and the last
    pass against the fixture"""
    raw, nchan, kw = case(name)
    prelim, detail, day, lst = reference(name)
    res = None
    if day is not None:
        _, _, off, mem, mad_all = day
        res = ctx.cphase_bin(1, off, mem, phases=raw['cphase'], flags=raw['flags'], mad_ignores_flags=mad_all)
        assert res['stats']['chunks'] == 1 and not res['stats']['resident']
        CK.compare(res, detail['day'], detail['day'], label=name + ' day pass')
    if lst is not None:
        _, _, off, mem = lst
        if res is not None:
            first = res
            res = ctx.cphase_bin(0, off, mem, binned=(first['cp_mean'], first['cp_median'], first['wts']))
            own = CK.binned_pass(first['cp_mean'], first['cp_median'], first['wts'], 0, off, mem)
            CK.compare(res, own, own, label=name + ' lst pass on device products')
            e1 = first_pass_error(detail)
        else:
            res = ctx.cphase_bin(0, off, mem, phases=raw['cphase'], flags=raw['flags'])
            CK.compare(res, detail['lst'], detail['lst'], label=name + ' lst pass')
            e1 = 0.0
    else:
        e1 = 0.0
    aux = detail.get('lst', detail.get('day'))
    CK.compare(as_masked(res), gold_quantities(name), aux, in_err=e1, label=name + ' fixture')


@pytest.mark.parametrize('name', NAMES)
def test_smooth_in_tbins_against_the_reference(ctx, name):
    raw, nchan, kw = case(name)
    prelim, detail, day, lst = reference(name)
    cp = BSP.ClosurePhase({'raw': {k: v.copy() for k, v in raw.items()}}, 150e6 + 1e5 * NP.arange(nchan), ctx=ctx)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        cp.smooth_in_tbins(**kw)
    got = cp.cpinfo['processed']['prelim']
    assert sorted(got.keys()) == GOLD[name + '_keys'].tolist()
    for key in ('daybins', 'diff_dbins', 'lstbins', 'dlstbins'):
        if key in got:
            ref = GOLD[name + '_out_' + key]
            assert NP.shape(got[key]) == ref.shape and NP.array_equal(got[key], ref), key
    if name == 'none':
        assert cp.binning_stats == []
        return
    aux = detail.get('lst', detail.get('day'))
    two = 'lst' in detail and 'day' in detail
    CK.compare(CK.prelim_quantities(got), gold_quantities(name), aux, in_err=first_pass_error(detail) if two else 0.0, label=name)
    # the stack was uploaded once and read where it lies; with two passes only the CSR tables go up and only the last products come down
    assert all(s['resident'] for s in cp.binning_stats)
    for s, plan in zip(cp.binning_stats, [p for p in (day, lst) if p is not None]):
        off, mem = plan[2], plan[3]
        assert s['upload_bytes'] == off.size * 8 + mem.size * 4
    if two:
        assert cp.binning_stats[0]['download_bytes'] == 0
        assert cp.binning_stats[1]['download_bytes'] == prelim['wts'].size * 8 * 9
    cp._drop_stack()


def test_three_chunks_equal_one(ctx):
    """a budget that holds one triad: three chunks over the triad axis, results identical to one chunk, on both axes and input kinds"""
    raw, nchan, kw = case('day_lst_67')
    prelim, detail, day, lst = reference('day_lst_67')
    _, _, off, mem, mad_all = day
    one = ctx.cphase_bin(1, off, mem, phases=raw['cphase'], flags=raw['flags'], mad_ignores_flags=mad_all)
    per_triad = 7 * 6 * 67 * 9 + 7 * 2 * 67 * 8 * 9
    three = ctx.cphase_bin(1, off, mem, phases=raw['cphase'], flags=raw['flags'], mad_ignores_flags=mad_all, budget_bytes=per_triad + 100)
    assert three['stats']['chunks'] == 3 and three['stats']['chunk_triads'] == 1 and one['stats']['chunks'] == 1
    for q in CK.QUANTITIES:
        assert NP.array_equal(one[q], three[q]), q
    _, _, off, mem = lst
    b = (one['cp_mean'], one['cp_median'], one['wts'])
    one2 = ctx.cphase_bin(0, off, mem, binned=b)
    three2 = ctx.cphase_bin(0, off, mem, binned=b, budget_bytes=7 * 2 * 67 * 24 + 3 * 2 * 67 * 8 * 9 + 100)
    assert three2['stats']['chunks'] == 3
    for q in CK.QUANTITIES:
        assert NP.array_equal(one2[q], three2[q]), q


def test_five_triads_in_chunks_of_two_equal_one_chunk(ctx):
    """Five triads in chunks of 2, 2 and 1: every quantity bit for bit that of one chunk."""
    rng = NP.random.default_rng(80)
    n0, n1, ntriads, nchan = 2, 4, 5, 8
    ph = rng.uniform(-NP.pi, NP.pi, (n0, n1, ntriads, nchan))
    fl = rng.uniform(size=ph.shape) < 0.2
    off, mem = NP.array([0, 2, 4], dtype=NP.int64), NP.arange(4, dtype=NP.int32)
    per_triad = n0 * n1 * nchan * 9 + n0 * 2 * nchan * 8 * 9                    # phases and flags in; nine doubles per output point
    one = ctx.cphase_bin(1, off, mem, phases=ph, flags=fl)
    three = ctx.cphase_bin(1, off, mem, phases=ph, flags=fl, budget_bytes=2 * per_triad)
    assert one['stats']['chunks'] == 1 and three['stats']['chunks'] == 3 and three['stats']['chunk_triads'] == 2
    for q in _abi.CPBINS_WANT:
        assert NP.array_equal(one[q], three[q]), q


def test_resident_two_pass_equals_two_round_trips(ctx):
    raw, nchan, kw = case('day_lst_67')
    prelim, detail, day, lst = reference('day_lst_67')
    _, _, doff, dmem, mad_all = day
    _, _, loff, lmem = lst
    first = ctx.cphase_bin(1, doff, dmem, phases=raw['cphase'], flags=raw['flags'], mad_ignores_flags=mad_all)
    second = ctx.cphase_bin(0, loff, lmem, binned=(first['cp_mean'], first['cp_median'], first['wts']))
    stack = ctx.cphase_upload(raw['cphase'], raw['flags'])
    kept = ctx.cphase_bin(1, doff, dmem, stack=stack, want=(), mad_ignores_flags=mad_all, keep=True)
    assert kept['stats']['resident'] and kept['stats']['download_bytes'] == 0 and kept['stats']['upload_bytes'] == doff.size * 8 + dmem.size * 4
    assert kept['stack'].shape == first['wts'].shape and kept['stack'].kind == _abi.PRISIM_CPBINS_BINNED
    res = ctx.cphase_bin(0, loff, lmem, stack=kept['stack'])
    assert res['stats']['resident'] and res['stats']['upload_bytes'] == loff.size * 8 + lmem.size * 4
    for q in CK.QUANTITIES:
        assert NP.array_equal(res[q], second[q]), q
    # the kept products are the first pass's, and can be copied back together with being kept
    both = ctx.cphase_bin(1, doff, dmem, stack=stack, mad_ignores_flags=mad_all, keep=True)
    for q in CK.QUANTITIES:
        assert NP.array_equal(both[q], first[q]), q
    for s in (kept['stack'], both['stack'], stack):
        s.close()


def test_bin_above_the_supported_size_is_refused(ctx):
    """PRISIM_CPBINS_MAX_BIN + 1 members: PRISIM_EINVAL with the documented message, nothing written, no stack made; the largest
    supported bin is taken"""
    n = _abi.PRISIM_CPBINS_MAX_BIN + 1
    rng = NP.random.default_rng(5)
    ph = 0.5 + 0.4 * rng.standard_normal((n, 1, 1, 3))
    fl = rng.uniform(size=ph.shape) < 0.3
    lib = ctx._lib
    off = NP.asarray([0, n], dtype=NP.int64)
    mem = NP.arange(n, dtype=NP.int32)
    outs = [NP.full((1, 1, 1, 3) if i not in (1, 2) else (1, 1, 1, 6), -7.0) for i in range(7)]
    import ctypes as C
    keep = C.c_void_p()
    flu = fl.astype(NP.uint8)
    rc = lib.prisim_cphase_bin(ctx._h, _abi.PRISIM_CPBINS_PHASE_FLAGS, _abi._ptr(ph), None, None, _abi._ptr(flu), n, 1, 1, 3, 0, 1,
                               _abi._ptr(off), _abi._ptr(mem), _abi.PRISIM_CPBINS_ALL, 0, 0, None, C.byref(keep),
                               *[_abi._ptr(o) for o in outs], None)
    assert rc == _abi.PRISIM_EINVAL and not keep.value
    assert 'more than PRISIM_CPBINS_MAX_BIN (256)' in lib.prisim_hip_last_error(ctx._h).decode()
    assert all(NP.all(o == -7.0) for o in outs)
    with pytest.raises(ValueError, match='PRISIM_CPBINS_MAX_BIN'):
        ctx.cphase_bin(0, off, mem, phases=ph, flags=fl)
    with pytest.raises(ValueError, match='not an index of the binned axis'):
        ctx.cphase_bin(1, [0, 2], [0, 1], phases=ph, flags=fl)
    res = ctx.cphase_bin(0, [0, n - 1], mem[:-1], phases=ph, flags=fl)
    assert res['stats']['max_bin'] == _abi.PRISIM_CPBINS_MAX_BIN
    ref = CK.native_pass(ph, fl, 0, [0, n - 1], mem[:-1])
    CK.compare(res, ref, ref, label='largest bin')
