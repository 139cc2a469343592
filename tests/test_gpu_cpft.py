"""GPU: the closure-phasor delay spectra (prisim_cphase_ft, prisim_amd.bispectrum_phase.ClosurePhaseDelaySpectrum.FT) against
tests/golden/golden_cpft.npz (the reference's FT executed) and the numpy checker tests/cpft_checker.py.

The bound is the package's bound for its two FFT routes, 1e-12 (tests/test_gpu_cpdelay.py), relative to df * sum over the
channels of |x| per row and window, x from the checker: the largest value the spectrum can take.  Rows that are non-finite in the
reference (weights of mean 0) are compared with 0, exactly, and may be 10 % of the rows at most."""
import os
import sys
import warnings

import numpy as NP
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cpft_checker as FK  # noqa: E402
from test_cpft import check_result, closure_phase, ft_args  # noqa: E402

from prisim_amd import _abi  # noqa: E402
from prisim_amd import bispectrum_phase as BSP  # noqa: E402

NAMES = [c['name'] for c in FK.cases()]
pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    with _abi.Context(0) as c:
        yield c


def pow2(m):
    return m & (m - 1) == 0


@pytest.mark.parametrize('route', ['auto', 'fused', 'rocfft'])
@pytest.mark.parametrize('name', NAMES)
def test_entry_against_the_fixture(ctx, name, route):
    """the fixture's cpinfo through prisim_cphase_ft, one call per weight set, against the reference's spectra"""
    m = FK.setup(name)['m']
    if route == 'fused' and not pow2(m):
        with pytest.raises(ValueError, match='power-of-two'):
            FK.entry_results(ctx, name, route=route)
        return
    res, stats = FK.entry_results(ctx, name, route=route)
    for st in stats:
        assert st['route'] == ('rocfft' if route == 'rocfft' or not pow2(m) else 'fused') and st['chunks'] == 1
    for tag in res:
        FK.compare_spectra(res[tag], name, tag, label=route)


def synthetic(nchan, lead=(2, 3, 3), nwin=2, seed=5):
    """random stacks: a full one and three that broadcast, weights with a row of zeros and a flagged channel, two windows, a scale"""
    rng = NP.random.default_rng(seed + nchan)
    n0, n1, n2 = lead
    shapes = [lead, (1, 1, n2), (n0, 1, 1), (1, n1, 1)]
    inputs = [rng.standard_normal(s + (nchan,)) + 1j * rng.standard_normal(s + (nchan,)) for s in shapes]
    w = rng.integers(0, 4, lead + (nchan,)).astype(NP.float64)
    w[n0 - 1, n1 - 1, 0, :] = 0.0
    w[:, :, :, nchan // 3] = 0.0
    inputs[0][n0 - 1, n1 - 1, 0, 0] = NP.nan                                  # under a weight of 0: it must not reach the spectrum
    wts = NP.zeros((nwin, nchan))
    wts[0, :] = 0.5 + rng.uniform(size=nchan)
    wts[1, nchan // 4:nchan // 4 + max(nchan // 2, 1)] = rng.uniform(size=max(nchan // 2, 1))
    return inputs, w, wts, rng.uniform(0.5, 2.0, (nwin, n0))


def compare(out, ref, df, label):
    worst = 0.0
    for kind in ('over', 'res'):
        for i, xs in enumerate(ref['xsum']):
            worst = max(worst, FK.spectrum_error(out[kind][i], ref[kind][i], xs, df))
    worst = max(worst, FK.spectrum_error(out['lag_kernel'], ref['lag_kernel'], ref['lag_xsum'], df),
                FK.spectrum_error(out['lag_kernel_res'], ref['lag_kernel_res'], ref['lag_xsum'], df))
    print('%s: error %.3e of df sum |x|' % (label, worst))
    assert worst <= FK.BOUND, (label, worst)


# (nchan, m): the fixture's sizes; one row per workgroup (m = 2048); LDS beyond 64 KiB (m = 4096 with as many channels)
@pytest.mark.parametrize('nchan,m,lead', [(16, 32, (2, 3, 3)), (64, 128, (2, 3, 3)), (20, 30, (2, 3, 3)), (67, 134, (2, 3, 3)),
                                           (1000, 2048, (1, 2, 2)), (4096, 4096, (1, 1, 3))])
def test_chunks_and_broadcasting(ctx, nchan, m, lead):
    """random stacks against the checker; a budget of three chunks with a partial last one, bit-identical to one chunk; stride-0
    broadcasting bit-identical to the materialised stacks; rows of zero weight exactly 0"""
    inputs, w, wts, vs = synthetic(nchan, lead)
    df, nres = 1e5, max(m // 5, 1)
    rows = int(NP.prod(lead))
    one = ctx.cphase_ft(inputs, wts, m, df, weights=w, vscale=vs, nres=nres)
    st = one['stats']
    assert st['chunks'] == 1 and st['rows'] == rows and st['route'] == ('fused' if pow2(m) else 'rocfft')
    assert st['group_rows'] == max(1, min(64, 2048 // m))
    ref = FK.transform(inputs, wts, m, df, weights=w, vscale=vs, nres=nres)
    compare(one, ref, df, 'nchan %d m %d' % (nchan, m))
    for arr in one['over'] + one['res'] + [one['lag_kernel'], one['lag_kernel_res']]:
        assert NP.all(arr[:, lead[0] - 1, lead[1] - 1, 0] == 0)
    tc = max(1, (rows - 1) // 2 - (1 if rows > 6 else 0))          # three chunks or more, the last one partial where rows allow
    few = ctx.cphase_ft(inputs, wts, m, df, weights=w, vscale=vs, nres=nres, budget_bytes=2 * st['row_bytes'] * tc + 8)
    assert few['stats']['chunk_rows'] == tc and few['stats']['chunks'] == -(-rows // tc) >= 3 and few['stats']['streams'] == 2
    if rows > 6:
        assert rows % tc != 0
    full = [NP.ascontiguousarray(NP.broadcast_to(x, lead + (nchan,))) for x in inputs]
    mat = ctx.cphase_ft(full, wts, m, df, weights=w, vscale=vs, nres=nres)
    assert mat['stats']['upload_bytes'] > st['upload_bytes']
    for kind in ('over', 'res'):
        for i in range(len(inputs)):
            assert NP.array_equal(one[kind][i], few[kind][i], equal_nan=True), (kind, i)
            assert NP.array_equal(one[kind][i], mat[kind][i], equal_nan=True), (kind, i)
    for kind in ('lag_kernel', 'lag_kernel_res'):
        assert NP.array_equal(one[kind], few[kind]) and NP.array_equal(one[kind], mat[kind])
    if not pow2(m):
        return
    other = ctx.cphase_ft(inputs, wts, m, df, weights=w, vscale=vs, nres=nres, route='rocfft')
    assert other['stats']['route'] == 'rocfft'
    compare(other, ref, df, 'nchan %d m %d rocfft' % (nchan, m))


@pytest.mark.parametrize('m', [16, 12])
def test_five_rows_in_chunks_of_two_equal_one_chunk(ctx, m):
    """Five rows in chunks of 2, 2 and 1 on two streams, fused (m = 16) and through rocFFT (m = 12, whose plan for the last chunk has
    another batch): every output bit for bit that of one chunk."""
    inputs, w, wts, vs = synthetic(8, lead=(1, 1, 5))
    one = ctx.cphase_ft(inputs, wts, m, 1e5, weights=w, vscale=vs, nres=5)
    three = ctx.cphase_ft(inputs, wts, m, 1e5, weights=w, vscale=vs, nres=5, budget_bytes=2 * 2 * one['stats']['row_bytes'])
    st = three['stats']
    assert one['stats']['chunks'] == 1 and st['route'] == ('fused' if m == 16 else 'rocfft')
    assert st['chunks'] == 3 and st['chunk_rows'] == 2 and st['streams'] == 2
    for kind in ('over', 'res'):
        for i in range(len(inputs)):
            assert NP.array_equal(one[kind][i], three[kind][i], equal_nan=True), (kind, i)
    for kind in ('lag_kernel', 'lag_kernel_res'):
        assert NP.array_equal(one[kind], three[kind], equal_nan=True), kind


@pytest.mark.parametrize('m', [32, 30])
def test_without_weights(ctx, m):
    """no weights: the lag kernel has one row per window, [nwin][1][1][1][m]; no input at all gives the lag kernel alone"""
    nchan = 16
    inputs, _, wts, vs = synthetic(nchan)
    inputs[0][1, 2, 0, 0] = 0.5                               # no weights: nothing hides the NaN of synthetic()
    out = ctx.cphase_ft(inputs, wts, m, 1e5, vscale=vs, nres=7)
    assert out['lag_kernel'].shape == (2, 1, 1, 1, m) and out['lag_kernel_res'].shape == (2, 1, 1, 1, 7)
    assert out['over'][1].shape == (2, 2, 3, 3, m) and out['res'][3].shape == (2, 2, 3, 3, 7)
    compare(out, FK.transform(inputs, wts, m, 1e5, vscale=vs, nres=7), 1e5, 'no weights m %d' % m)
    alone = ctx.cphase_ft([], wts, m, 1e5, want=('lag_kernel',))
    assert alone['over'] is None and alone['res'] is None and alone['lag_kernel_res'] is None
    assert NP.array_equal(alone['lag_kernel'], out['lag_kernel'])


def test_refusals(ctx):
    inputs, w, wts, vs = synthetic(16)
    for kw, text in (({'m': 8}, 'lags'), ({'m': 8192}, 'lags'), ({'m': 32, 'nres': 5000}, 'resampled'), ({'m': 30, 'route': 'fused'}, 'power-of-two')):
        with pytest.raises(ValueError, match=text):
            ctx.cphase_ft(inputs, wts, kw.pop('m'), 1e5, weights=w, vscale=vs, **dict({'nres': 7}, **kw))
    with pytest.raises(ValueError, match='neither the full extent nor 1'):
        ctx.cphase_ft([inputs[0][:, :2]], wts, 32, 1e5, weights=w, nres=7)
    with pytest.raises(ValueError, match='input stacks'):
        ctx.cphase_ft([inputs[1]] * 9, wts, 32, 1e5, weights=w, nres=7)
    out = ctx.cphase_ft(inputs[1:2], wts, 32, 1e5, weights=w, nres=7)           # and the entry still works
    compare(out, FK.transform(inputs[1:2], wts, 32, 1e5, weights=w, nres=7), 1e5, 'after the refusals')


@pytest.mark.parametrize('name', NAMES)
def test_class_against_the_reference(ctx, name):
    """ClosurePhase from the fixture's raw inputs with the fixture's processed and errinfo; every array of FT's result against the
    reference's, oversampled and resampled"""
    cp = closure_phase(name, ctx)
    ds = BSP.ClosurePhaseDelaySpectrum(cp)
    bw, kw = ft_args(name)
    res = ds.FT(bw, **kw)
    check_result(ds.cPhaseDS, name, 'o', 'class')
    if kw['resample']:
        assert res is ds.cPhaseDS_resampled
        check_result(res, name, 'r', 'class')
    assert sorted(ds.ft_stats) == ['errinfo0', 'errinfo1', 'prelim']
    assert all(s['route'] == ('fused' if pow2(FK.setup(name)['m']) else 'rocfft') for s in ds.ft_stats.values())
    if FK.case(name)['vis_ones']:
        res = ds.FT(bw, **dict(kw, visscaleinfo=None))
        s = 1.0 / NP.sqrt(1.0 / 3.0)
        FK.compare_spectra(ds.cPhaseDS, name, 'o', label='no visscaleinfo', scale=s)
        FK.compare_spectra(res, name, 'r', label='no visscaleinfo', scale=s)


def test_end_to_end_from_raw_phases(ctx):
    """device smooth_in_tbins, subtract, subsample_differencing and FT from raw phases, against the checker applied to the cpinfo
    the device produced (FT is linear in its inputs, so the conditioning of the binning does not enter)"""
    name = 'noflags'
    cp = closure_phase(name, ctx, fill=False)
    S = FK.setup(name)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        cp.smooth_in_tbins(ndaybins=2, lstbinsize=1008.0)
        shape = cp.cpinfo['processed']['prelim']['wts'].shape
        cp.subtract(0.3 * NP.random.default_rng(3).standard_normal(shape[2:]))
        cp.subsample_differencing(ndaybins=4, lstbinsize=1008.0)
    ds = BSP.ClosurePhaseDelaySpectrum(cp)
    bw, kw = ft_args(name, apply_flags=True)
    res = ds.FT(bw, **kw)
    vs = FK.vis_scale(kw['visscaleinfo']['vis'], S['wts'], shape[0])
    nzero = nrows = 0
    for label, w, stacks in FK.ft_inputs(name, cp.cpinfo['processed'], cp.cpinfo['errinfo']):
        ref = FK.transform([s for _, s in stacks], S['wts'], S['m'], S['df'], weights=w, vscale=vs, nres=S['nres'])
        zero = NP.mean(w, axis=-1) == 0.0
        nzero, nrows = nzero + int(zero.sum()), nrows + zero.size
        for i, (p, _) in enumerate(stacks):
            for r, kind in ((ds.cPhaseDS, 'over'), (res, 'res')):
                got = FK.pool(r, p)
                assert NP.all(got[:, zero] == 0), (p, kind)
                e = FK.spectrum_error(got, ref[kind][i], ref['xsum'][i], S['df'])
                print('end to end %s %s: error %.3e of df sum |x|' % (p, kind, e))
                assert e <= FK.BOUND, (p, kind, e)
        if label == 'prelim':
            assert FK.spectrum_error(ds.cPhaseDS['lag_kernel'], ref['lag_kernel'], ref['lag_xsum'], S['df']) <= FK.BOUND
    assert 0 < nzero <= FK.MAX_ZERO_SHARE * nrows
    for label, st in sorted(ds.ft_stats.items()):
        print('FT %s: %d rows, kernel %.4f ms, %.2f GB/s of %d kernel bytes, wall %.3f ms, route %s, %d rows per workgroup, %d B of LDS' % (
            label, st['rows'], st['kernel_ms'], st['kernel_bytes'] / max(st['kernel_ms'], 1e-9) / 1e6, st['kernel_bytes'], st['wall_ms'],
            st['route'], st['group_rows'], st['lds_bytes']))
    cp._drop_stack()
