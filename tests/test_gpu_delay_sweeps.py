"""GPU (-m gpu): the delay transform where its kernels take another path than at the 74 rows of test_gpu_beams_delay_gather.py.

B1  the fused LDS FFT kernel (delay_kernels.hip) with more rows than one sweep of its persistent grid: second and third trips of
    `for (pass = blockIdx.x; pass < npass; pass += gridDim.x)`, the register prefetch of the next pass, the reuse of the LDS row buffer,
    dead rows past the end, every N and every window mode; against the numpy restatement, and bit for bit against launches of one
    snapshot each, in which every block makes a single pass.
B2  the fused kernel against the restatement in extended precision.
B3  the rocFFT pipeline (k_dt_prepare / k_dt_finish in aux_kernels.hip) at odd and non-smooth lengths, truncated padding, factors with
    interpolation, the clamp at the last sample, ragged batches, and more elements than one sweep of its grid.
B4  the output length the library reports against _abi.delay_nout.
B5  InterferometerArray.delay_transform and DelaySpectrum.delay_transform where len(arange(0, nfft, 1 + pad)) is one too many."""
from fractions import Fraction

import numpy as NP
import pytest

from oracle import delay_oracle as DO
from prisim_amd import _abi, workloads as W
from prisim_amd import delay_spectrum as DS, interferometry as RI, skymodel as SM

pytestmark = pytest.mark.gpu

DF = 97656.25
FUSED_N = (256, 512, 768, 1024, 2048, 4096)
WMODES = ('none', 'row', 'baseline')


def grid_blocks(ctx):
    """RESTATES launch_delay_fft_n (delay_kernels.hip): grid = min(2 * cu_count, npass), cu_count taken as 256 when the device reports
    none.  Whoever changes the launcher's grid changes this, or the totals below no longer reach a second and a third trip."""
    cu = ctx.device_info()['cu_count']
    return 2 * (cu if cu > 0 else 256)


def rows_per_pass(n):
    """RESTATES k_delay_fft: RPB = 256 / (N / 16) rows per block pass: 16, 8, 5, 4, 2, 1."""
    return 256 // (n // 16)


def exact_nout(nchan, pad):
    """The count of j >= 0 with j (1 + pad) < nfft, the pad taken as the decimal written (a string)."""
    nfft = nchan + int(nchan * float(pad))
    q = Fraction(nfft) / (1 + Fraction(pad))
    return nfft, -((-q.numerator) // q.denominator)


def load(ctx, nchan, nbl, nt, seed, df=DF):
    """A seeded complex normal cube (nt, nbl, nchan) in the context's slots."""
    rng = NP.random.default_rng(seed)
    ctx.set_array(rng.uniform(-100, 100, (nbl, 3)), 150e6 + NP.arange(nchan) * df, nt_max=nt)
    cube = rng.normal(size=(nt, nbl, nchan)) + 1j * rng.normal(size=(nt, nbl, nchan))
    for t in range(nt):
        ctx.set_vis(cube[t], slot=t)
    return rng, cube


def window(rng, mode, nbl, nchan):
    if mode == 'none':
        return None
    return rng.uniform(0.2, 1.0, nchan if mode == 'row' else (nbl, nchan))


def full(w, nbl, nchan):
    return None if w is None else NP.ascontiguousarray(NP.broadcast_to(w, (nbl, nchan)))


def restatement(cube, w, df, pad, real=NP.float64):
    """oracle.delay_oracle.delay_transform (zero padding, ifft, fftshift, interpolation at arange(0, nfft, 1 + pad)) snapshot by
    snapshot, (nt, nbl, n) like the library's output; real=NP.longdouble transforms in extended precision."""
    nt, nbl, nchan = cube.shape
    one = NP.ones((1, 1, 1), dtype=real)
    bp = one if w is None else NP.broadcast_to(NP.asarray(w, dtype=real), (nbl, nchan))[:, :, None]
    ctype = NP.result_type(real, NP.complex64)
    return NP.stack([DO.delay_transform(cube[t].astype(ctype)[:, :, None], bp, one, df, pad=pad)[0][:, :, 0] for t in range(nt)])


def check_rows(got, ref, tol, what, rpb=None, grid=None, fails=None):
    """max |got - ref| over every row <= tol; the worst row by where the fused kernel computed it.  With a list `fails` the finding
    is appended there, so that the caller can go on to its other checks and report them all."""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = NP.abs(got - ref).max(axis=2)
    worst = float(err.max())
    print('%s: max err %.3e, bound %.3e' % (what, worst, tol))
    if not worst <= tol:
        t, b = (int(i) for i in NP.unravel_index(int(NP.argmax(NP.where(NP.isnan(err), NP.inf, err))), err.shape))
        where = 'snapshot %d, baseline %d' % (t, b)
        if rpb is not None:
            p = (t * err.shape[1] + b) // rpb
            where += ', pass %d, block %d, trip %d' % (p, p % grid, p // grid)
        msg = '%s: max err %.3e > %.3e at %s' % (what, worst, tol, where)
        if fails is None:
            raise AssertionError(msg)
        fails.append(msg)


# ---- B1 --------------------------------------------------------------------------------------------------------------------------

def sweep_totals(grid, rpb):
    """(nt, nbl) just over one sweep of the grid (the second trip has one or two live rows, the rest of that pass is dead), and over two
    sweeps with a ragged tail (odd nbl, no multiple of 5: a pass straddles a snapshot boundary, row % nbl wraps inside a pass, some
    blocks make a third trip)."""
    small = grid * rpb // 2 + 1
    while 2 * small <= grid * rpb:
        small += 1
    need = 2 * grid * rpb + rpb + (rpb + 1) // 2
    large = -(-need // 3)
    while large % 2 == 0 or large % 5 == 0:
        large += 1
    return (2, small), (3, large)


@pytest.mark.parametrize('wmode', WMODES)
@pytest.mark.parametrize('nchan', FUSED_N)
def test_fused_delay_fft_beyond_one_sweep_of_the_grid(ctx, monkeypatch, nchan, wmode):
    grid, rpb = grid_blocks(ctx), rows_per_pass(nchan)
    monkeypatch.delenv('PRISIM_HIP_DT_BATCH_BYTES', raising=False)
    monkeypatch.delenv('PRISIM_HIP_DT_FUSED', raising=False)
    for nt, nbl in sweep_totals(grid, rpb):
        nrows = nt * nbl
        npass = -(-nrows // rpb)
        if nt == 2:
            assert 1 <= nrows - grid * rpb <= 2 and grid < npass <= grid + 2
        else:
            assert npass > 2 * grid and 3 * nbl >= 2 * grid * rpb + rpb + (rpb + 1) // 2
            assert rpb == 1 or nbl % rpb != 0
        assert nbl <= grid * rpb                                   # one snapshot alone is a single pass of every block
        rng, cube = load(ctx, nchan, nbl, nt, 1000 * nchan + nt)
        w = window(rng, wmode, nbl, nchan)
        if wmode == 'baseline':
            assert NP.unique(w, axis=0).shape[0] == nbl
        for pad in (1.0, 0.0) if (nt == 3 and wmode == 'none') else (1.0,):
            what = 'N %d %s rows %d x %d pad %.0f' % (nchan, wmode, nt, nbl, pad)
            fails = []
            _, nout = ctx.delay_transform_device(nt, bpwts=w, pad=pad, want_lag=True, want_power=True, power_scale=0.5)
            assert nout == nchan and ctx.timing()['last_delay_fused'] == 1
            lag, pw = ctx.get_lags(0, nt), ctx.get_delay_power(0, nt)
            ref = restatement(cube, w, DF, pad)
            top = float(NP.max(NP.abs(ref)))
            check_rows(lag, ref, 1e-12 * top, what + ' lags', rpb, grid, fails)
            check_rows(pw, DO.delay_power(ref, 0.5), 1e-11 * top ** 2, what + ' power', rpb, grid, fails)
            del ref
            # a row's arithmetic does not depend on which pass or block carries it: one launch per snapshot, one pass per block
            nfft = nchan + int(nchan * pad)
            monkeypatch.setenv('PRISIM_HIP_DT_BATCH_BYTES', str(nbl * nfft * 16))
            ctx.delay_transform_device(nt, bpwts=w, pad=pad, want_lag=True, want_power=True, power_scale=0.5)
            assert ctx.timing()['last_delay_fused'] == 1
            lag1, pw1 = ctx.get_lags(0, nt), ctx.get_delay_power(0, nt)
            monkeypatch.delenv('PRISIM_HIP_DT_BATCH_BYTES')
            check_rows(lag, lag1, 0.0, what + ' lags, one launch against one launch per snapshot', rpb, grid, fails)
            check_rows(pw, pw1, 0.0, what + ' power, one launch against one launch per snapshot', rpb, grid, fails)
            if not (NP.array_equal(lag, lag1) and NP.array_equal(pw, pw1)):
                fails.append(what + ': one launch and one launch per snapshot differ in bits')
            del lag1, pw1
            out, _, hpw = ctx.delay_transform(nt, bpwts=full(w, nbl, nchan), pad=pad, want_power=True, power_scale=0.5)
            check_rows(out, lag, 0.0, what + ' lags, host-output form against device form', rpb, grid, fails)
            check_rows(hpw, pw, 0.0, what + ' power, host-output form against device form', rpb, grid, fails)
            if not (NP.array_equal(out, lag) and NP.array_equal(hpw, pw)):
                fails.append(what + ': host-output form and device form differ in bits')
            assert not fails, '\n'.join(fails)
            del out, hpw
            if nt == 2 and wmode == 'row':                         # the out == nullptr and out_pow == nullptr stores, once per N
                ctx.delay_transform_device(nt, bpwts=w, pad=pad, want_lag=False, want_power=True, power_scale=0.5)
                assert NP.array_equal(ctx.get_delay_power(0, nt), pw), what + ' power only'
                with pytest.raises(RuntimeError):
                    ctx.get_lags(0, nt)
                ctx.delay_transform_device(nt, bpwts=w, pad=pad, want_lag=True, want_power=False)
                assert NP.array_equal(ctx.get_lags(0, nt), lag), what + ' lags only'
                with pytest.raises(RuntimeError):
                    ctx.get_delay_power(0, nt)


# ---- B2 --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('nchan', FUSED_N)
def test_fused_delay_fft_against_extended_precision(ctx, monkeypatch, nchan):
    """The same restatement fed long-double input, which numpy transforms in long double (x87: 64-bit mantissa), at the bound the
    float64 comparison uses, 1e-12 max|ref|."""
    if NP.fft.ifft(NP.ones(8, dtype=NP.clongdouble)).dtype != NP.clongdouble or NP.finfo(NP.longdouble).eps >= NP.finfo(NP.float64).eps:
        pytest.skip('numpy.fft does not transform clongdouble in extended precision here')
    monkeypatch.delenv('PRISIM_HIP_DT_BATCH_BYTES', raising=False)
    monkeypatch.delenv('PRISIM_HIP_DT_FUSED', raising=False)
    nbl, nt = 37, 2
    rng, cube = load(ctx, nchan, nbl, nt, 77 + nchan)
    w = window(rng, 'baseline', nbl, nchan)
    _, nout = ctx.delay_transform_device(nt, bpwts=w, pad=1.0, want_lag=True, want_power=True, power_scale=0.5)
    assert nout == nchan and ctx.timing()['last_delay_fused'] == 1
    ref = restatement(cube, w, DF, 1.0, real=NP.longdouble)
    assert ref.dtype == NP.clongdouble
    top = float(NP.max(NP.abs(ref)))
    lag = ctx.get_lags(0, nt)
    err = float(NP.max(NP.abs(lag.astype(NP.clongdouble) - ref)))
    perr = float(NP.max(NP.abs(ctx.get_delay_power(0, nt).astype(NP.longdouble) - NP.abs(ref) ** 2 * NP.longdouble(0.5))))
    print('B2 N %d: lags max err / max|ref| = %.3e, power max err / max|ref|^2 = %.3e' % (nchan, err / top, perr / top ** 2))
    assert err <= 1e-12 * top
    assert perr <= 1e-11 * top ** 2


# ---- B3 --------------------------------------------------------------------------------------------------------------------------

PIPELINE_SHAPES = ((33, '0.0'),       # odd nfft
                   (50, '0.33'),      # npad truncates to 16: nfft 66, nout 50
                   (203, '0.7'),      # nfft 345 = 3 * 5 * 23, odd and not smooth, with interpolation
                   (64, '2.5'),       # factor 3.5
                   (768, '0.5'),      # a channel count of the fused kernel with a factor that is no integer
                   (1000, '1.0'),     # an integer factor at a channel count the fused kernel does not have
                   (15, '0.4'), (120, '0.4'), (1000, '0.4'))      # len(arange(0, nfft, 1.4)) is one too many


def pipeline_reference(cube, w, df, nchan, pad):
    """The restatement, cut to the exact count of lags where numpy's arange has a position more; every position dropped is >= nfft."""
    nfft, nout = exact_nout(nchan, pad)
    ref = restatement(cube, w, df, float(pad))
    pos = NP.arange(0, nfft, 1 + float(pad)) if float(pad) > 0.0 else NP.arange(nfft, dtype=NP.float64)
    assert ref.shape[2] == pos.size and pos.size in (nout, nout + 1)
    assert NP.all(pos[nout:] >= nfft) and NP.all(pos[:nout] < nfft)
    return nfft, nout, ref[:, :, :nout]


@pytest.mark.parametrize('wmode', WMODES)
@pytest.mark.parametrize('nchan,pad', PIPELINE_SHAPES)
def test_rocfft_pipeline_at_odd_lengths_and_fractional_factors(ctx, monkeypatch, nchan, pad, wmode):
    monkeypatch.delenv('PRISIM_HIP_DT_BATCH_BYTES', raising=False)
    monkeypatch.delenv('PRISIM_HIP_DT_FUSED', raising=False)
    nbl, nt, df, scale = 13, 3, 1.0e5, 2.5
    rng, cube = load(ctx, nchan, nbl, nt, 31 * nchan + len(pad), df=df)
    w = window(rng, wmode, nbl, nchan)
    nfft, nout, ref = pipeline_reference(cube, w, df, nchan, pad)
    if (nchan, pad) == (50, '0.33'):
        assert (nfft, nout) == (66, 50)
    if (nchan, pad) == (203, '0.7'):
        assert nfft == 345
    top = float(NP.max(NP.abs(ref)))
    tol, ptol = 1e-10 * top, 1e-9 * top ** 2 * scale
    refp = DO.delay_power(ref, scale)
    what = 'nchan %d pad %s %s' % (nchan, pad, wmode)
    fpad = float(pad)
    _, n = ctx.delay_transform_device(nt, bpwts=w, pad=fpad, want_lag=True, want_power=True, power_scale=scale)
    assert ctx.timing()['last_delay_fused'] == 0
    assert n == nout == _abi.delay_nout(nchan, fpad)
    check_rows(ctx.get_lags(0, nt), ref, tol, what + ' device form lags')
    check_rows(ctx.get_delay_power(0, nt), refp, ptol, what + ' device form power')
    out, _, pw = ctx.delay_transform(nt, bpwts=full(w, nbl, nchan), pad=fpad, want_power=True, power_scale=scale)
    assert out.shape == pw.shape == (nt, nbl, nout)
    check_rows(out, ref, tol, what + ' host-output form lags')
    check_rows(pw, refp, ptol, what + ' host-output form power')
    # two snapshots per batch: the third is a ragged last batch (no bit identity asked: rocFFT may plan another batch count otherwise)
    monkeypatch.setenv('PRISIM_HIP_DT_BATCH_BYTES', str(2 * nbl * nfft * 16))
    ctx.delay_transform_device(nt, bpwts=w, pad=fpad, want_lag=True, want_power=True, power_scale=scale)
    assert ctx.timing()['last_delay_fused'] == 0
    check_rows(ctx.get_lags(0, nt), ref, tol, what + ' device form in batches, lags')
    check_rows(ctx.get_delay_power(0, nt), refp, ptol, what + ' device form in batches, power')
    out, _, pw = ctx.delay_transform(nt, bpwts=full(w, nbl, nchan), pad=fpad, want_power=True, power_scale=scale)
    check_rows(out, ref, tol, what + ' host-output form in batches, lags')
    check_rows(pw, refp, ptol, what + ' host-output form in batches, power')


def test_rocfft_pipeline_beyond_one_sweep_of_its_grid(ctx, monkeypatch):
    """RESTATES grid_for (aux_kernels.hip): at most 16384 blocks of 256 threads.  4197 rows of 1000 channels, pad 1: k_dt_finish has
    4 197 000 elements and loops, k_dt_prepare 8 394 000 and makes a third trip."""
    monkeypatch.delenv('PRISIM_HIP_DT_BATCH_BYTES', raising=False)
    monkeypatch.delenv('PRISIM_HIP_DT_FUSED', raising=False)
    nchan, nbl, nt, df, scale = 1000, 1399, 3, 1.0e5, 2.5
    sweep = 16384 * 256
    assert nt * nbl * nchan > sweep and nt * nbl * 2 * nchan > 2 * sweep
    rng, cube = load(ctx, nchan, nbl, nt, 4197, df=df)
    w = window(rng, 'row', nbl, nchan)
    _, nout = ctx.delay_transform_device(nt, bpwts=w, pad=1.0, want_lag=True, want_power=True, power_scale=scale)
    assert nout == nchan and ctx.timing()['last_delay_fused'] == 0
    ref = restatement(cube, w, df, 1.0)
    top = float(NP.max(NP.abs(ref)))
    check_rows(ctx.get_lags(0, nt), ref, 1e-10 * top, 'grid-stride lags')
    check_rows(ctx.get_delay_power(0, nt), DO.delay_power(ref, scale), 1e-9 * top ** 2 * scale, 'grid-stride power')


# ---- B4 --------------------------------------------------------------------------------------------------------------------------

def length_cases():
    """Every channel count below 300 at which len(arange(0, nfft, 1.4)) exceeds the exact count, and 1000; the multiples of 5 below 130
    at which it does not; the shapes of B3."""
    cases = []
    for nchan in list(range(5, 300, 5)) + [1000]:
        nfft, nout = exact_nout(nchan, '0.4')
        if NP.arange(0, nfft, 1.4).size != nout or nchan < 130:
            cases.append((nchan, '0.4'))
    return cases + [c for c in PIPELINE_SHAPES if c not in cases]


def test_library_output_length_is_delay_nout(ctx, monkeypatch):
    monkeypatch.delenv('PRISIM_HIP_DT_BATCH_BYTES', raising=False)
    cases = length_cases()
    longer = [n for n, p in cases if p == '0.4' and NP.arange(0, exact_nout(n, p)[0], 1.4).size != exact_nout(n, p)[1]]
    assert longer == [15, 30, 60, 115, 120, 125, 225, 230, 235, 240, 245, 250, 255, 1000] and 35 <= len(cases) <= 45
    for nchan, pad in cases:
        load(ctx, nchan, 1, 1, nchan, df=1.0e5)
        _, nout = ctx.delay_transform_device(1, pad=float(pad))
        assert nout == _abi.delay_nout(nchan, float(pad)) == exact_nout(nchan, pad)[1], (nchan, pad)
        assert ctx.get_lags(0, 1).shape == (1, 1, nout)


# ---- B5 --------------------------------------------------------------------------------------------------------------------------

def test_classes_at_120_channels_and_pad_0p4():
    """A host-assigned cube goes snapshot by snapshot through Context.delay_transform_host, whose arrays were one lag too long here."""
    cfg = W.config1()
    bl, sky = cfg['baselines'], cfg['sky']
    nchan, nt, pad = 120, 2, 0.4
    ch = 150e6 + 1.0e5 * NP.arange(nchan)
    skymod = SM.SkyModel(location=sky['altaz'], flux_ref=sky['flux_ref'], spindex=sky['spindex'], ref_freq=sky['ref_freq'],
                         src_shape=NP.stack((sky['fwhm_deg'], sky['fwhm_deg'], NP.zeros_like(sky['fwhm_deg'])), axis=1))
    ia = RI.InterferometerArray(['b%d' % i for i in range(bl.shape[0])], bl, ch, telescope={'id': 'hera'}, latitude=-30.7224,
                                skycoords='altaz', pointing_coords='altaz')
    bpass = 0.6 + 0.4 * NP.hanning(nchan + 2)[1:-1]
    for j in range(nt):
        ia.observe((2457000.5 + j, 30.0 + 2.0 * j), {'Tnet': 200.0}, bpass, [90.0, 270.0], skymod, 10.7)
    rng = NP.random.default_rng(120)
    nbl = bl.shape[0]
    cube = rng.normal(size=(nbl, nchan, nt)) + 1j * rng.normal(size=(nbl, nchan, nt))
    ia.skyvis_freq = cube
    ia.delay_transform(pad=pad, verbose=False)
    assert ia.skyvis_lag.shape == (nbl, nchan, nt)
    ref = DO.delay_transform(cube, NP.asarray(ia.bp), NP.asarray(ia.bp_wts), ia.freq_resolution, pad=pad)[0]
    assert ref.shape[1] == nchan + 1                               # numpy's count; its last position is nfft itself
    ref = ref[:, :nchan, :]
    assert NP.max(NP.abs(ia.skyvis_lag - ref)) <= 1e-10 * NP.max(NP.abs(ref))
    res = DS.DelaySpectrum(ia).delay_transform(pad=pad, downsample=True, verbose=False)
    assert res['skyvis_lag'].shape == (nbl, nchan, nt)
    assert res['lags'].shape == (res['skyvis_lag'].shape[1],)
    assert NP.max(NP.abs(res['skyvis_lag'] - ref)) <= 1e-10 * NP.max(NP.abs(ref))
