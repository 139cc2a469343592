"""CPU: the numpy.ma checker of ClosurePhase.subsample_differencing and ClosurePhase.subtract (tests/cpdiff_checker.py) against every
case of tests/golden/golden_cpdiff.npz (the reference's statements executed, tests/golden/make_golden_cpdiff.py); the host logic of
prisim_amd.bispectrum_phase.ClosurePhase on a stand-in context (tests/cpdiff_standin.py) against the same fixture; the enumeration of
the pairs of pairs; the ctypes mirror of prisim_cpdiff_stats against the compiled header; the kernel's register budget.

Values are compared only where the reference's mask is False (under it the reference leaves unspecified values); the masks themselves
must be equal.  The bounds are those of tests/test_gpu_cpdiff.py, which derives them."""
import json
import math
import os
import subprocess
import warnings

import numpy as NP
import numpy.ma as MA
import pytest

import cphase_bins_checker as CK
import cpdiff_checker as DK
import cpdiff_standin as SI
from prisim_amd import _abi
from prisim_amd import bispectrum_phase as BSP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [c[0] for c in DK.cases()]
FREQS = lambda nchan: 150e6 + 1e5 * NP.arange(nchan)  # noqa: E731


def closure_phase(raw, nchan, ctx):
    return BSP.ClosurePhase({'raw': {k: v.copy() for k, v in raw.items()}}, FREQS(nchan), ctx=ctx)


def check_bins(err, ref):
    for key in ('daybins', 'diff_dbins', 'lstbins', 'dlstbins'):
        assert NP.shape(err[key]) == ref[key].shape and NP.asarray(err[key]).dtype == ref[key].dtype, key
        assert NP.array_equal(err[key], ref[key]), key


def test_fixture_cases():
    assert NAMES == ['nd4_lst', 'nd5_lst', 'size_lst', 'below', 'onelst', 'onelst_size', 'nd4_lst_67']
    want = {'nd4_lst': (4, 3), 'nd5_lst': (4, 15), 'size_lst': (4, 15), 'below': (7, 3), 'onelst': (1, 3), 'onelst_size': (1, 3),
            'nd4_lst_67': (4, 3)}      # the last of the 4 LST bins is empty
    for name in NAMES:
        raw, nchan, kw = DK.case(name)
        ref = DK.gold_errinfo(name)
        assert ref['wts']['0'].shape == want[name] + (3, nchan), name
        assert raw['cphase'].shape == (1 if name.startswith('onelst') else 7, 6, 3, nchan)
        assert sorted(DK.gold()[name + '_keys'].tolist()) == sorted(ref.keys())
        for g in '01':       # masked and unmasked elements both occur, and the masks of a pair are shared by its four arrays
            m = MA.getmaskarray(ref['wts'][g])
            assert m.any() and not m.all(), name
    assert DK.gold_errinfo('onelst')['dlstbins'].tolist() == [0.0] and DK.gold_errinfo('onelst_size')['dlstbins'].tolist() == [800.0]
    # 5 uneven day bins from daybinsize = 1.5
    assert DK.reference('size_lst')[1]['day']['nbin'][0, :, 0, 0].tolist() == [2, 1, 1, 1, 1]


@pytest.mark.parametrize('name', NAMES)
def test_checker_equals_the_reference(name):
    err, detail = DK.reference(name)
    ref = DK.gold_errinfo(name)
    check_bins(err, ref)
    DK.compare_errinfo(err, ref, detail, label=name)


@pytest.mark.parametrize('n', [4, 5, 6, 7])
def test_pairs_of_pairs(n):
    pairs = BSP.pairs_of_day_bin_pairs(n)
    assert pairs == DK.pairs_of_pairs(n) and len(pairs) == 3 * math.comb(n, 4)
    assert all(isinstance(v, int) for row in pairs for v in row)
    keys = {frozenset((frozenset(r[:2]), frozenset(r[2:]))) for r in pairs}
    assert len(keys) == len(pairs) and all(len(set(r)) == 4 and r[0] < r[1] and r[2] < r[3] for r in pairs)
    for name in NAMES:
        ref = DK.gold_errinfo(name)['list_of_pair_of_pairs']
        if len(ref) == len(pairs):
            assert ref == pairs


@pytest.mark.parametrize('name', NAMES)
def test_host_logic_against_the_reference(name):
    """ClosurePhase.subsample_differencing on the stand-in context: bins, keys, shapes, dtypes and masks are the reference's; the
    stacks stay on the device and are closed"""
    raw, nchan, kw = DK.case(name)
    ctx = SI.StandinContext()
    cp = closure_phase(raw, nchan, ctx)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        cp.subsample_differencing(**kw)
    assert (len(caught) == 1 and 'smaller than the LST resolution' in str(caught[0].message)) == (name == 'below')
    err = cp.cpinfo['errinfo']
    ref = DK.gold_errinfo(name)
    assert sorted(err.keys()) == sorted(DK.gold()[name + '_keys'].tolist())
    check_bins(err, ref)
    assert isinstance(err['list_of_pair_of_pairs'], list) and set(err['wts']) == {'0', '1'} and set(err['eicp_diff']) == {'0', '1'}
    assert all(set(err['eicp_diff'][g]) == {'mean', 'median'} for g in '01')
    DK.compare_errinfo(err, ref, DK.reference(name)[1], label=name)
    two = 'lstbinsize' in kw and raw['lst'].shape[0] > 1
    assert [c.get('diff', False) for c in ctx.calls] == [False] * (1 + two) + [True] and ctx.uploads == 1
    assert all(c['source'] == 'stack' for c in ctx.calls)                   # nothing but tables is uploaded per call
    assert all(c['want'] == () and c['keep'] for c in ctx.calls[:-1])       # nothing but the differences is copied back
    assert ctx.calls[0]['axis'] == 1 and ctx.calls[0]['kind'] == 'native'
    if two:
        assert ctx.calls[1]['axis'] == 0 and ctx.calls[1]['kind'] == 'binned'
    assert ctx.calls[-1]['pairs'].tolist() == ref['list_of_pair_of_pairs']
    assert len(ctx.stacks) == 1 + two and all(s.closed for s in ctx.stacks)
    assert len(cp.binning_stats) == 2 + two


def test_several_lsts_without_lstbinsize_take_the_single_lst_route():
    raw, nchan, _ = DK.case('nd4_lst')
    ctx = SI.StandinContext()
    cp = closure_phase(raw, nchan, ctx)
    cp.subsample_differencing(ndaybins=4)
    detail = {}
    ref = DK.subsample_differencing({'raw': raw}, ndaybins=4, detail=detail)
    assert 'lst' not in detail and len(ctx.calls) == 2
    err = cp.cpinfo['errinfo']
    check_bins(err, ref)
    assert err['lstbins'].shape == (7,) and err['dlstbins'].tolist() == [0.0] and err['wts']['0'].shape == (7, 3, 3, nchan)
    DK.compare_errinfo(err, ref, detail, label='no lstbinsize')
    for g in '01':
        assert NP.array_equal(err['wts'][g].data, ref['wts'][g].data)
        for s in ('mean', 'median'):
            assert NP.array_equal(err['eicp_diff'][g][s].data, ref['eicp_diff'][g][s].data)


def test_errors_come_before_any_device_work():
    raw, nchan, _ = DK.case('nd4_lst')
    ctx = SI.StandinContext()
    cp = closure_phase(raw, nchan, ctx)
    for exc, match, kw in (
            (ValueError, 'Only one of daybinsize or ndaybins should be set', {'daybinsize': 2.0}),
            (ValueError, 'Input ndaybins must be greater than or equal to 4', {'ndaybins': 3}),
            (TypeError, 'Input ndaybins must be an integer', {'ndaybins': 4.0}),
            (ValueError, 'One of daybinsize or ndaybins must be set', {'ndaybins': None}),
            (TypeError, 'Input daybinsize must be a scalar', {'daybinsize': '2', 'ndaybins': None}),
            (ValueError, 'day resolution', {'daybinsize': 1.0, 'ndaybins': None}),
            (ValueError, 'Could not find at least 4 bins along repeating days. Adjust binning interval.', {'daybinsize': 2.5, 'ndaybins': None}),
            (TypeError, 'Input lstbinsize must be a scalar', {'lstbinsize': '800'})):
        with pytest.raises(exc, match=match):
            cp.subsample_differencing(**kw)
    assert not ctx.calls and ctx.uploads == 0 and cp.cpinfo['errinfo'] == {}
    with pytest.raises(ValueError, match='smooth_in_tbins must fill'):
        cp.subtract(NP.zeros((3, nchan)))


@pytest.mark.parametrize('fail_at', [1, 2])
def test_kept_stacks_are_closed_on_failure(fail_at):
    raw, nchan, kw = DK.case('nd4_lst')
    ctx = SI.StandinContext(fail_at=fail_at)
    cp = closure_phase(raw, nchan, ctx)
    with pytest.raises(RuntimeError, match='stand-in failure'):
        cp.subsample_differencing(**kw)
    assert len(ctx.stacks) == fail_at and all(s.closed for s in ctx.stacks)
    assert cp.cpinfo['errinfo'] == {}


def _subtract_instance():
    raw = {k: DK.gold()['subtract_in_' + k] for k in ('cphase', 'flags', 'lst', 'days')}
    cp = closure_phase(raw, raw['cphase'].shape[-1], SI.StandinContext())
    cp.smooth_in_tbins(**json.loads(str(DK.gold()['subtract_smooth'])))
    return cp


@pytest.mark.parametrize('model', ['triadchan', 'full_nan'])
def test_subtract_against_the_reference(model):
    """keys, shapes, dtypes and masks equal; data within 8 u where unmasked (exp, the subtraction or the division and the angle on
    phasors of modulus 1 that agree to a few u); 0 under the masks.  The checker is held to the same."""
    cphase, sub, res = DK.gold_subtract(model)
    cp = _subtract_instance()
    prelim = cp.cpinfo['processed']['prelim']
    cp.subtract(cphase.copy())
    proc = cp.cpinfo['processed']
    csub, cres = DK.subtract(prelim, cphase.copy())
    assert set(proc['submodel']) == {'cphase', 'eicp'} and set(proc['residual']) == {'eicp', 'cphase'}
    for gsub, gres in ((proc['submodel'], proc['residual']), (csub, cres)):
        pairs = [(gsub[k], sub[k]) for k in ('cphase', 'eicp')] + [(gres[q][s], res[q][s]) for q in ('eicp', 'cphase') for s in ('mean', 'median')]
        for got, ref in pairs:
            assert isinstance(got, MA.MaskedArray) and got.shape == ref.shape and got.dtype == ref.dtype
            mask = MA.getmaskarray(ref)
            assert NP.array_equal(MA.getmaskarray(got), mask)
            assert NP.all(got.data[mask] == 0)
            assert NP.all(NP.abs(got.data - ref.data)[~mask] <= 8.0 * CK.U)
    assert proc['submodel']['cphase'].shape == (1,) * (4 - cphase.ndim) + cphase.shape
    if model == 'full_nan':
        assert MA.getmaskarray(proc['submodel']['cphase']).sum() == 1 and MA.getmaskarray(proc['residual']['eicp']['mean'])[1, 0, 2, 3]
    assert MA.getmaskarray(res['eicp']['mean']).any()


def test_subtract_validation():
    cp = _subtract_instance()
    with pytest.raises(TypeError, match='Input cphase must be a numpy array'):
        cp.subtract([0.0])
    with pytest.raises(ValueError, match='shape incompatible'):
        cp.subtract(NP.zeros((4, 5)))
    with pytest.raises(ValueError, match='shape incompatible'):
        cp.subtract(NP.zeros((1, 1, 1, 3, 5)))
    assert 'submodel' not in cp.cpinfo['processed']


def test_output_bytes_and_where_the_entry_is_declared():
    assert _abi.PRISIM_CPDIFF_OUT_BYTES == 4 * 16 + 2 * 8 + 2
    # the new symbols live in the new header only
    assert 'cphase_diff' not in open(os.path.join(ROOT, 'include', 'prisim_hip.h')).read()
    assert 'cphase_diff' not in open(os.path.join(ROOT, 'include', 'prisim_cpbins.h')).read()


def test_kernel_uses_no_scratch(tmp_path):
    """hipcc -S of cpdiff.hip for gfx950: the kernel keeps everything in registers (tools/kernel_meta.py reads the metadata)."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_meta
    hipcc = '/opt/rocm/bin/hipcc'
    assert os.path.exists(hipcc), 'the library under test cannot be built without hipcc'
    asm = tmp_path / 'cpdiff.s'
    subprocess.check_call([hipcc, '-O3', '-std=c++17', '--offload-arch=gfx950', '-ffp-contract=off', '-I/opt/rocm/include',
                           '--cuda-device-only', '-S', os.path.join(ROOT, 'prisim_amd', 'csrc_closure', 'cpdiff.hip'), '-o', str(asm)])
    rows = [r for r in kernel_meta.kernel_meta(asm.read_text()) if 'k_cpdiff' in r['name']]
    assert len(rows) == 1
    print(rows[0])
    assert rows[0]['scratch'] == 0 and rows[0]['vgpr_spill'] == 0
