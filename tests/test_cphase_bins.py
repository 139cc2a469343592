"""CPU: the numpy.ma checker of the day and LST binning of closure phases (tests/cphase_bins_checker.py) against every case of
tests/golden/golden_cphase.npz (the reference's statements executed, tests/golden/make_golden_cphase.py); the host logic of
prisim_amd.bispectrum_phase.ClosurePhase on a stand-in context (tests/cphase_standin.py) against the same fixture; loadnpz, the
constructor's validation and the masks of expicp; the ctypes mirror of prisim_cpbins_stats against the compiled header.

Values are compared only where the reference's mask is False (under it the reference leaves unspecified values); the masks themselves
and the weights must be equal.  The bounds are those of tests/test_gpu_cphase_bins.py, which derives them."""
import json
import os
import subprocess
import warnings

import numpy as NP
import numpy.ma as MA
import pytest

import cphase_bins_checker as CK
import cphase_standin as SI
from prisim_amd import _abi
from prisim_amd import bispectrum_phase as BSP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = NP.load(os.path.join(ROOT, 'tests', 'golden', 'golden_cphase.npz'))
CASES = json.loads(str(GOLD['cases']))
NAMES = [c[0] for c in CASES]


def case(name):
    nchan, kw = [(c[1], c[2]) for c in CASES if c[0] == name][0]
    raw = {k: GOLD['%s_in_%s' % (name, k)] for k in ('cphase', 'flags', 'lst', 'days')}
    return raw, nchan, kw


def gold_prelim(name):
    """the fixture's prelim dictionary, masked arrays rebuilt"""
    pre = name + '_out_'
    out = {}
    for key in GOLD.files:
        if not key.startswith(pre) or key.endswith('__mask'):
            continue
        v = GOLD[key]
        if key + '__mask' in GOLD.files:
            v = MA.array(v, mask=GOLD[key + '__mask'])
        path = key[len(pre):].split('_')
        if path[0] in ('eicp', 'cphase'):
            out.setdefault(path[0], {})[path[1]] = v
        else:
            out[key[len(pre):]] = v
    return out


def checker_run(name):
    raw, nchan, kw = case(name)
    detail = {}
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        prelim = CK.smooth_in_tbins({'raw': raw}, detail=detail, **kw)
    return prelim, detail


def final_aux(detail):
    """(bin_pass result of the last pass, bound of the error of its input phases)"""
    if 'lst' in detail and 'day' in detail:
        d = detail['day']
        good = d['wts'] > 0.0
        e1 = float(NP.max(CK.phasor_bound(d['nbin'], NP.minimum(d['mod_mean'], d['mod_median']))[good]))
        return detail['lst'], e1
    return detail.get('lst', detail.get('day')), 0.0


def compare_prelim(prelim, name, detail, two_pass_on_device=False):
    ref = gold_prelim(name)
    assert sorted(prelim.keys()) == GOLD[name + '_keys'].tolist() == sorted(ref.keys())
    for key in ('daybins', 'diff_dbins', 'lstbins', 'dlstbins'):
        if key in ref:
            assert NP.shape(prelim[key]) == ref[key].shape and NP.asarray(prelim[key]).dtype == ref[key].dtype, key
            assert NP.array_equal(prelim[key], ref[key]), key
    if 'wts' not in ref:
        assert 'eicp' not in prelim and 'cphase' not in prelim
        return {}
    aux, e1 = final_aux(detail)
    got, want = CK.prelim_quantities(prelim), CK.prelim_quantities(ref)
    for q in CK.QUANTITIES:
        assert isinstance(got[q], MA.MaskedArray), q
        assert NP.array_equal(MA.getmaskarray(want[q]), MA.getdata(want['wts']) <= 0.0), q      # the fixture's own masks
    return CK.compare(got, want, aux, in_err=e1 if two_pass_on_device else 0.0, label=name)


@pytest.mark.parametrize('name', NAMES)
def test_checker_equals_the_reference(name):
    prelim, detail = checker_run(name)
    compare_prelim(prelim, name, detail)


def test_fixture_has_the_cases_the_bounds_need():
    """fully masked bins on both axes, a bin of exactly two unflagged members on both axes, wrapped phases, uneven bins"""
    raw, _, _ = case('daybinsize')
    assert NP.all(raw['flags'][3:5, :, 0, 1]) and raw['flags'][0, 0:3, 1, 2].tolist() == [False, True, False]
    assert raw['flags'][0:3, 0, 2, 3].tolist() == [False, True, False]
    assert NP.any(raw['cphase'] > 3.0) and NP.any(raw['cphase'] < -3.0) and NP.all(NP.abs(raw['cphase']) <= NP.pi)
    assert 0.25 < raw['flags'].mean() < 0.4
    d = checker_run('daybinsize')[1]['day']
    assert sorted(set(d['nbin'].ravel().tolist())) == [1, 2, 3] and NP.any(d['wts'] <= 0.0) and d['n'][0, 0, 1, 2] == 2
    d = checker_run('ndaybins')[1]['day']
    assert [int(d['nbin'][0, k, 0, 0]) for k in range(4)] == [2, 2, 1, 1]
    d = checker_run('lst')[1]['lst']
    assert [int(d['nbin'][k, 0, 0, 0]) for k in range(3)] == [3, 2, 2] and NP.all(d['wts'][1, :, 0, 1] <= 0.0) and d['n'][0, 0, 2, 3] == 2
    assert NP.any(raw['lst'][:, 0] > 23.0) and NP.any(raw['lst'][:, 0] < 1.0)                   # wraps through 24 h
    assert case('day_lst_67')[0]['cphase'].shape == (7, 6, 3, 67)
    # the ndaybins mad ignores the flags (:1834), the daybinsize mad does not (:1797): with the same bins they differ
    raw, _, _ = case('ndaybins')
    off, mem = CK.csr(NP.array_split(NP.arange(6), 4))
    a, b = (CK.native_pass(raw['cphase'], raw['flags'], 1, off, mem, f)['mad'] for f in (True, False))
    assert not NP.array_equal(a, b)


@pytest.mark.parametrize('name', NAMES)
def test_host_logic_against_the_reference(name):
    """ClosurePhase.smooth_in_tbins on the stand-in context: bins, axes, keys, shapes, dtypes and masks are the reference's"""
    raw, nchan, kw = case(name)
    ctx = SI.StandinContext()
    cp = BSP.ClosurePhase({'raw': {k: v.copy() for k, v in raw.items()}}, 150e6 + 1e5 * NP.arange(nchan), ctx=ctx)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        cp.smooth_in_tbins(**kw)
    assert (len(caught) == 1 and 'smaller than the LST resolution' in str(caught[0].message)) == (name == 'below')
    compare_prelim(cp.cpinfo['processed']['prelim'], name, checker_run(name)[1])
    n_day = int('daybinsize' in kw or 'ndaybins' in kw)
    n_lst = int('lstbinsize' in kw)
    assert len(ctx.calls) == n_day + n_lst and ctx.uploads == min(1, n_day + n_lst)
    assert all(c['source'] == 'stack' for c in ctx.calls)                   # nothing but the CSR tables is uploaded per call
    if n_day:
        assert ctx.calls[0]['axis'] == 1 and ctx.calls[0]['mad_ignores_flags'] == ('ndaybins' in kw)
    if n_day and n_lst:                                                     # the day-binned stack stays on the device
        assert ctx.calls[0]['keep'] and ctx.calls[0]['want'] == () and ctx.calls[1]['kind'] == 'binned' and ctx.calls[1]['axis'] == 0
    if name == 'below':
        assert ctx.calls[0]['offsets'].tolist() == list(range(8)) and ctx.calls[0]['members'].tolist() == list(range(7))
    # a second call reuses the resident native stack
    cp.smooth_in_tbins(ndaybins=3)
    assert ctx.uploads == 1


def test_lst_pass_over_the_products_of_an_earlier_call():
    """'wts' in prelim from an earlier call: the LST pass reads those products from the host (binned input), as the reference does"""
    raw, nchan, kw = case('day_lst')
    ctx = SI.StandinContext()
    cp = BSP.ClosurePhase({'raw': raw}, NP.arange(nchan) * 1.0, ctx=ctx)
    cp.smooth_in_tbins(ndaybins=2)
    cp.smooth_in_tbins(lstbinsize=800.0)
    assert [c['source'] for c in ctx.calls] == ['stack', 'binned']
    compare_prelim(cp.cpinfo['processed']['prelim'], 'day_lst', checker_run('day_lst')[1])


def test_binned_count_reading():
    x = NP.asarray([0.0, 1.0, 2.0, 3.0, 5.0, 6.0])
    for fn in (BSP.binned_count, CK.binned_count):
        counts, ri = fn(x, [0.0, 2.5, 5.0, 7.5])
        assert counts.tolist() == [3, 1, 2] and ri.tolist() == [4, 7, 8, 10, 0, 1, 2, 3, 4, 5]
        counts, ri = fn([5.0, -1.0, 2.5, 9.0], [0.0, 2.5, 5.0])             # the right edge is open, outliers fall in no bin
        assert counts.tolist() == [0, 1] and ri[ri[1]:ri[2]].tolist() == [2]


def test_loadnpz(tmp_path):
    raw, nchan, _ = case('lst')
    last = 58000.0 + 6713.0 + NP.arange(6)[None, :] + raw['lst'] / 24.0
    days = 2458000.5 + NP.arange(6.0)
    path = str(tmp_path / 'cp.npz')
    NP.savez(path, closures=raw['cphase'].astype(NP.float32), triads=NP.arange(9).reshape(3, 3), flags=raw['flags'].astype(NP.uint8),
             last=last, days=days)
    info = BSP.loadnpz(path, longitude=21.4, latitude=-30.7)
    assert set(info) == {'raw'} and set(info['raw']) == {'cphase', 'triads', 'flags', 'lst', 'lst-day', 'days'}
    r = info['raw']
    assert r['cphase'].dtype == NP.float64 and NP.array_equal(r['cphase'], raw['cphase'].astype(NP.float32).astype(NP.float64))
    assert r['flags'].dtype == bool and NP.array_equal(r['flags'], raw['flags'])
    assert NP.allclose(r['lst'], raw['lst'], atol=1e-6) and NP.array_equal(r['days'], days)
    assert NP.array_equal(r['lst-day'], NP.floor(last) - 6713.0 + 2400000.5) and r['lst-day'].shape == (7, 6)
    NP.savez(path, closures=raw['cphase'], triads=NP.arange(9).reshape(3, 3), flags=raw['flags'], last=raw['lst'], days=days)
    r = BSP.loadnpz(path, lst_format='HourAngle')['raw']
    assert NP.array_equal(r['lst'], raw['lst']) and NP.array_equal(r['lst-day'], NP.broadcast_to(days, (7, 6)))
    with pytest.raises(ValueError, match='lst_format invalid'):
        BSP.loadnpz(path, lst_format='degrees')
    # from a file, through the constructor
    cp = BSP.ClosurePhase(path, NP.arange(nchan) * 1e5, ctx=SI.StandinContext())
    assert cp.extfile == str(tmp_path / 'cp.hdf5') and cp.df == 1e5 and cp.cpinfo['errinfo'] == {} and cp.cpinfo['processed']['prelim'] == {}
    NP.savez(path, closures=raw['cphase'], triads=NP.arange(9).reshape(3, 3), flags=raw['flags'], last=raw['lst'], days=days,
             averaged_closures=raw['cphase'][:, 0])
    with pytest.raises(NotImplementedError):
        BSP.loadnpz(path)


def test_constructor_validation_and_expicp_masks():
    raw, nchan, _ = case('none')
    f = NP.arange(nchan) * 1e5
    with pytest.raises(TypeError, match='infile must be a string'):
        BSP.ClosurePhase(3, f)
    with pytest.raises(TypeError, match='freqs must be a numpy array'):
        BSP.ClosurePhase({'raw': raw}, list(f))
    with pytest.raises(TypeError, match='infmt must be a string'):
        BSP.ClosurePhase({'raw': raw}, f, infmt=1)
    with pytest.raises(ValueError, match='must be "npz" or "hdf5"'):
        BSP.ClosurePhase({'raw': raw}, f, infmt='fits')
    with pytest.raises(NotImplementedError):
        BSP.ClosurePhase('x.hdf5', f, infmt='hdf5')
    with pytest.raises(ValueError, match='do not match with dimensions'):
        BSP.ClosurePhase({'raw': raw}, f[:-1])
    cp = BSP.ClosurePhase({'raw': raw}, f, ctx=SI.StandinContext())
    native = cp.cpinfo['processed']['native']
    assert set(native) == {'cphase', 'eicp', 'wts'}
    for k in native:
        assert isinstance(native[k], MA.MaskedArray) and NP.array_equal(MA.getmaskarray(native[k]), raw['flags']), k
    assert native['eicp'].dtype == NP.complex128 and NP.array_equal(native['eicp'].data[~raw['flags']], NP.exp(1j * raw['cphase'])[~raw['flags']])
    assert NP.array_equal(native['wts'].data, (~raw['flags']).astype(float))
    with pytest.raises(ValueError, match='Only one of daybinsize or ndaybins'):
        cp.smooth_in_tbins(daybinsize=2.0, ndaybins=2)
    with pytest.raises(TypeError, match='ndaybins must be an integer'):
        cp.smooth_in_tbins(ndaybins=2.0)
    with pytest.raises(ValueError, match='ndaybins must be positive'):
        cp.smooth_in_tbins(ndaybins=0)
    with pytest.raises(TypeError, match='daybinsize must be a scalar'):
        cp.smooth_in_tbins(daybinsize='2')
    with pytest.raises(TypeError, match='lstbinsize must be a scalar'):
        cp.smooth_in_tbins(lstbinsize='2')
    with pytest.raises(ValueError, match='day resolution'):
        cp.smooth_in_tbins(daybinsize=0.5)
    assert not cp._ctx.calls


def test_want_bits_follow_the_quantities():
    bits = [_abi.PRISIM_CPBINS_WTS, _abi.PRISIM_CPBINS_EICP_MEAN, _abi.PRISIM_CPBINS_EICP_MEDIAN, _abi.PRISIM_CPBINS_CP_MEAN,
            _abi.PRISIM_CPBINS_CP_MEDIAN, _abi.PRISIM_CPBINS_RMS, _abi.PRISIM_CPBINS_MAD]
    assert [_abi.CPBINS_WANT[q] for q in CK.QUANTITIES] == bits and list(_abi.CPBINS_WANT) == list(CK.QUANTITIES)
    assert _abi.PRISIM_CPBINS_ALL == sum(bits)


def test_kernel_uses_no_scratch(tmp_path):
    """hipcc -S of cpbins.hip for gfx950: the kernel keeps everything in registers (tools/kernel_meta.py reads the metadata)."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_meta
    hipcc = '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    asm = tmp_path / 'cpbins.s'
    subprocess.check_call([hipcc, '-O3', '-std=c++17', '--offload-arch=gfx950', '-ffp-contract=off', '-I/opt/rocm/include',
                           '--cuda-device-only', '-S', os.path.join(ROOT, 'prisim_amd', 'csrc_closure', 'cpbins.hip'), '-o', str(asm)])
    rows = [r for r in kernel_meta.kernel_meta(asm.read_text()) if 'k_cpbins' in r['name']]
    assert len(rows) == 1
    print(rows[0])
    assert rows[0]['scratch'] == 0 and rows[0]['vgpr_spill'] == 0
