"""GPU: delay CLEAN (prisim_amd/csrc_clean/clean.hip) at ties, box edges and length edges.  Rows with ties (tests/clean_cases.py) against
the exact-arithmetic run (tests/clean_exact.py): iterations, flags, cc and res identical, rms within 2 ulp; rows whose kernel peak is
complex and off lag 0, the lengths about the LDS limit of the shared kernel, sixteen waves per workgroup, a rejected row among good
ones and the delayClean chain entry with per-row kernels and boxes over three cubes against the numpy checker (tests/clean_checker.py).
tests/test_clean_exact.py asserts on the CPU that no row of these inputs decides within a last bit, so no row is excused here.

What these tests found when they first ran: a row rejected for its threshold (flag 16) hung its wave (the compiler had threaded lane 0
past the row hand-out's shuffle; clean.hip now meets at a wave barrier there); inrms and outrms drifted 20 to 120 ulp from the checker
because the AXPY rounded four products where numpy fuses two; and a kernel whose peak is complex was normalised by a hypot one ulp off
the true modulus on one kernel in ten.  The device's hypot resolved every sign-symmetric tie as the exact run does."""
import os
import sys

import numpy as NP
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clean_cases as CC  # noqa: E402
import clean_checker as CK  # noqa: E402

from prisim_amd import _abi  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    with _abi.Context(0) as c:
        yield c


def _run(ctx, b):
    return ctx.clean_rows(b['inp'], b['kern'], b['box'], b['gain'], b['maxiter'], b['threshold'], absolute=b['absolute'], kidx=b['kidx'])


def _rms_off(got, want, ulps):
    """Rows whose (inrms, outrms) is not NaN where wanted and within ulps relative elsewhere."""
    nan = NP.isnan(want)
    with NP.errstate(invalid='ignore'):
        ok = NP.where(nan, NP.isnan(got), NP.abs(got - want) <= ulps * CK.ULP * NP.abs(want))
    return NP.flatnonzero(~ok.all(axis=1))


def _check_exact(got, want, ids):
    """Device results against the exact run: everything identical, rms within 2 ulp (one hypot, and the mean of two)."""
    cc, res, it, fl, rms = got[:5]
    wcc, wres, wit, wfl, wrms = want[:5]
    bad = NP.flatnonzero((it != wit) | (fl != wfl))
    assert bad.size == 0, [(ids[r], int(it[r]), int(wit[r]), int(fl[r]), int(wfl[r])) for r in bad[:8]]
    bad = NP.flatnonzero((cc != wcc).any(axis=1) | (res != wres).any(axis=1))
    assert bad.size == 0, [ids[r] for r in bad[:8]]
    bad = _rms_off(rms, wrms, 2)
    assert bad.size == 0, [(ids[r], rms[r].tolist(), wrms[r].tolist()) for r in bad[:8]]


def _check_checker(got, want, inp, what):
    """Device results against the checker: decisions equal, cc and res to 1e-12 of the row's peak, rms within 4 ulp (two hypots within
    an ulp each, the median selects an element, the mean of two adds a rounding)."""
    cc, res, it, fl, rms = got[:5]
    wcc, wres, wit, wfl, wrms = want[:5]
    bad = NP.flatnonzero((it != wit) | (fl != wfl))
    assert bad.size == 0, (what, [(int(r), int(it[r]), int(wit[r]), int(fl[r]), int(wfl[r])) for r in bad[:8]])
    scale = NP.abs(inp).max(axis=1)
    assert (NP.abs(cc - wcc).max(axis=1) <= 1e-12 * scale).all() and (NP.abs(res - wres).max(axis=1) <= 1e-12 * scale).all(), what
    with NP.errstate(invalid='ignore', divide='ignore'):
        print('%s: largest rms difference %.2f ulp' % (what, NP.nanmax(NP.abs(rms - wrms) / NP.abs(wrms)) / CK.ULP))
    bad = _rms_off(rms, wrms, 4)
    assert bad.size == 0, (what, [(int(r), rms[r].tolist(), wrms[r].tolist()) for r in bad[:8]])


@pytest.mark.parametrize('m,variant,repeats', CC.tie_batches())
def test_tie_rows_equal_the_exact_run(ctx, m, variant, repeats):
    b = CC.tie_batch(m, variant, repeats)
    got = _run(ctx, b)
    want = CC.tie_reference(m, variant, repeats)
    _check_exact(got, want, b['ids'])
    assert got[5]['rows'] == len(b['ids']) and got[5]['sum_iter'] == int(want[2].sum())


@pytest.mark.parametrize('m,nrows', CC.SHIFTED)
@pytest.mark.parametrize('per_row', [False, True])
def test_shifted_kernel_rows_against_the_checker(ctx, m, nrows, per_row):
    b = CC.shifted_batch(m, nrows, per_row)
    _check_checker(_run(ctx, b), CC.shifted_reference(m, nrows, per_row), b['inp'], 'm %d' % m)


def test_sixteen_waves_per_workgroup_one_row_and_no_row(ctx):
    """16 x (CU count) rows: every workgroup runs sixteen waves, each in its own slice of LDS.  The tie rows of m = 24, tiled and
    shuffled; the reference is computed once per distinct row."""
    key = (24, 0, 4)
    b, want = CC.tie_batch(*key), CC.tie_reference(*key)
    nrows = 16 * ctx.device_info()['cu_count']
    pick = NP.random.default_rng(CC.SEED).permutation(nrows) % len(b['ids'])
    tiled = dict(b, inp=b['inp'][pick], box=b['box'][pick], kidx=b['kidx'][pick])
    got = _run(ctx, tiled)
    assert got[5]['waves_per_block'] == 16 and got[5]['rows'] == nrows
    _check_exact(got, [a[pick] for a in want[:5]], [b['ids'][i] for i in pick])
    assert got[5]['sum_iter'] == int(want[2][pick].sum())
    one = dict(b, inp=b['inp'][7:8], box=b['box'][7:8], kidx=b['kidx'][7:8])
    got = _run(ctx, one)
    assert got[5]['waves_per_block'] == 1
    _check_exact(got, [a[7:8] for a in want[:5]], b['ids'][7:8])
    none = dict(b, inp=b['inp'][:0], box=b['box'][:0], kidx=b['kidx'][:0])
    cc, res, it, fl, rms, st = _run(ctx, none)
    assert cc.shape == res.shape == (0, 24) and it.size == fl.size == rms.size == 0 and st['rows'] == 0 and st['sum_iter'] == 0


@pytest.mark.parametrize('m', CC.LDS_EDGE)
def test_lengths_about_the_lds_limit_and_the_top(ctx, m):
    b = CC.shifted_batch(m, 2, False, CC.LDS_EDGE_MAXITER)
    got = _run(ctx, b)
    print('m %d: kernel_in_lds %s, %d B of LDS' % (m, got[5]['kernel_in_lds'], got[5]['lds_bytes']))
    if m == 2048:
        assert got[5]['kernel_in_lds'] is True
    if m == 4096:
        assert got[5]['kernel_in_lds'] is False
    _check_checker(got, CC.shifted_reference(m, 2, False, CC.LDS_EDGE_MAXITER), b['inp'], 'm %d' % m)


def test_a_rejected_row_among_good_ones(ctx):
    """An absolute threshold above one row's peak: that row comes back untouched with flag 16 and NaN rms, its neighbours in the same
    workgroup as if it were not there."""
    b, want = CC.tie_batch(*CC.BAD_THRESHOLD), CC.tie_reference(*CC.BAD_THRESHOLD)
    r = [i for i, name in enumerate(b['ids']) if '-but2-' in name][0]
    assert NP.abs(b['inp'][r]).max() > 0 and want[3][r] == _abi.PRISIM_CLEAN_BAD_THRESHOLD
    assert NP.count_nonzero(want[3] != _abi.PRISIM_CLEAN_BAD_THRESHOLD) >= 8
    nrows = 3 * ctx.device_info()['cu_count']                # three rows per workgroup
    pick = NP.random.default_rng(CC.SEED + 1).permutation(nrows) % len(b['ids'])
    cc, res, it, fl, rms, st = _run(ctx, dict(b, inp=b['inp'][pick], box=b['box'][pick], kidx=b['kidx'][pick]))
    assert st['waves_per_block'] == 3
    for i in NP.flatnonzero(pick == r):
        assert fl[i] == _abi.PRISIM_CLEAN_BAD_THRESHOLD and it[i] == 0
        assert NP.array_equal(res[i], b['inp'][r]) and not NP.any(cc[i]) and NP.isnan(rms[i]).all()
    _check_exact((cc, res, it, fl, rms), [a[pick] for a in want[:5]], [b['ids'][i] for i in pick])
    assert st['sum_iter'] == int(want[2][pick].sum())


@pytest.mark.parametrize('nchan,m', CC.DELAY_SHAPES)
def test_delay_chain_entry_with_per_row_kernels_and_boxes_over_three_cubes(ctx, nchan, m):
    """prisim_clean_delay maps CLEAN row r to box and kernel index r % nrows: every cube must meet its own rows' boxes and kernels."""
    c, want = CC.delay_case(nchan, m), CC.delay_reference(nchan, m)
    got = ctx.clean_delay(c['win'], c['kwin'], c['box'], m, c['lag_scale'], c['freq_scale1'], c['freq_scale2'], c['gain'], c['maxiter'],
                          c['threshold'], kidx=c['kidx'])
    assert NP.array_equal(got['iters'], want['iters']) and NP.array_equal(got['flags'], want['flags'])
    for name in ('lag', 'kern_lag', 'cc', 'res', 'cc_freq', 'res_freq'):
        assert got[name].shape == want[name].shape
        assert NP.max(NP.abs(got[name] - want[name])) <= 1e-10 * NP.max(NP.abs(want[name])), name
    nan = NP.isnan(want['rms'])
    assert NP.array_equal(NP.isnan(got['rms']), nan)
    assert NP.all(NP.abs(got['rms'][~nan] - want['rms'][~nan]) <= 1e-10 * NP.abs(want['rms'][~nan]).max())
    assert got['stats']['rows'] == want['iters'].size and got['stats']['sum_iter'] == int(want['iters'].sum())
