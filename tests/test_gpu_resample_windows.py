"""GPU: the resampled spectra of the four entries that share the resampling plan (prisim_amd/csrc_addon/addon_plan.h) --
subband_transform, runs_transform(mode='resample'), closure_delay_spectra(phases=...) and cphase_ft -- under four windows in one
call: all ones, zero edges, one interior zero channel, all zero.  The kept-bin rules differ between the entries (the support span for
runs, the channels a window does not zero for cpft and cpdelay; subband reads the span in its kernel), so the interior zero and the
zero edges take different lists through the same tables.  nchan = 10 < m, so bins of the zero padding are dropped; m = 16 runs fused
and m = 12 through rocFFT; nres = 16 from m = 12 resamples upwards.

Every result is held to its entry's own checker under that checker's bound (1e-12, DESIGN 4.7, with each checker's scale), and the
all-zero window's outputs are exactly 0."""
import os
import sys

import numpy as NP
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import allruns_checker as RK  # noqa: E402
import cpdelay_checker as CC  # noqa: E402
import cpft_checker as FK  # noqa: E402
import subband_checker as SK  # noqa: E402
from test_allruns import rel_err as runs_rel_err  # noqa: E402

from prisim_amd import dsp_readings as D  # noqa: E402

pytestmark = pytest.mark.gpu
NCHAN, NT, DF = 10, 3, 1e5
SHAPES = [(16, 5), (16, 8), (12, 5), (12, 8), (12, 16)]     # (m, nres)


def windows(rng):
    w = rng.uniform(0.5, 1.5, (4, NCHAN))
    w[0] = 1.0
    w[1, 0] = w[1, -1] = 0.0
    w[2, NCHAN // 2] = 0.0
    w[3] = 0.0
    return w


def route_of(m):
    return 'fused' if m == 16 else 'rocfft'


@pytest.mark.parametrize('m,nres', SHAPES)
def test_subband(ctx, m, nres):
    rng = NP.random.default_rng(1000 * m + nres)
    nbl, wts = 2, windows(rng)
    x = rng.normal(size=(nbl, NCHAN, NT)) + 1j * rng.normal(size=(nbl, NCHAN, NT))
    bp = 0.5 + rng.uniform(size=(nbl, NCHAN, 1))
    out = ctx.subband_transform(NP.transpose(x, (2, 0, 1))[NP.newaxis], bp[:, :, 0], wts, m, DF, nres=nres, want=('over', 'res'))
    assert out['stats']['route'] == route_of(m) and out['stats']['rows'] == nbl * NT
    over, res = (NP.transpose(out[k][0], (1, 2, 3, 0)) for k in ('over', 'res'))    # (nbl, nwin, lags, nt)
    want = SK.transform(x, bp, wts, m - NCHAN, DF)
    assert SK.rel_err(over, want) <= 1e-12
    assert SK.rel_err(res, D.resample(want, nres, axis=2), scale_of=want) <= 1e-12
    assert res.shape[2] == nres and not NP.any(over[:, 3]) and not NP.any(res[:, 3])


@pytest.mark.parametrize('m,nres', SHAPES)
def test_runs(ctx, m, nres):
    rng = NP.random.default_rng(2000 * m + nres)
    R, nbl, win = 2, 3, windows(rng)
    vis = rng.standard_normal((R, nbl, NCHAN, NT)) + 1j * rng.standard_normal((R, nbl, NCHAN, NT))
    kw = dict(bp=0.5 + rng.uniform(size=(nbl, NCHAN, NT)), wts=rng.uniform(0.5, 1.5, size=(nbl, NCHAN, NT)), win=win, m=m, scale=m * DF,
              mode='resample', nout=nres)
    got, st = ctx.runs_transform(vis, nbl, NCHAN, NT, **kw)
    want = RK.transform(vis, nbl, NCHAN, NT, **kw)
    assert st['route'] == 'direct' and got.shape == want.shape == (4, R, nbl, nres, NT)
    assert runs_rel_err(got, want) <= 1e-12
    assert not NP.any(got[3])


@pytest.mark.parametrize('m,nres', SHAPES)
def test_closure_delay_spectra(ctx, m, nres):
    rng = NP.random.default_rng(3000 * m + nres)
    nrows, wts = 5, windows(rng)
    ph = rng.uniform(-NP.pi, NP.pi, (nrows, NCHAN, NT))
    one = ctx.closure_delay_spectra(wts, m, DF, phases=ph, nres=nres, want=('over', 'res'))
    assert one['stats']['route'] == route_of(m) and one['stats']['chunks'] == 1
    want = dict(zip(('over', 'res'), CC.delay_spectra(ph, wts, m, DF, nres)))
    for k in ('over', 'res'):
        assert one[k].shape == want[k].shape
        assert CC.spectrum_error(one[k][:, :3], want[k][:, :3], wts[:3], DF) <= 1e-12, k    # the scale of the all-zero window is 0
        assert not NP.any(one[k][:, 3]), k
    # five rows in chunks of 2, 2 and 1 on two streams: the phases, both spectra and, through rocFFT, its rows per row
    per_row = NCHAN * NT * 8 + 4 * NT * (m * (16 if m == 16 else 32) + nres * 16)
    three = ctx.closure_delay_spectra(wts, m, DF, phases=ph, nres=nres, want=('over', 'res'), budget_bytes=2 * 2 * per_row)
    st = three['stats']
    assert st['chunks'] == 3 and st['chunk_rows'] == 2 and st['streams'] == 2
    assert all(NP.array_equal(one[k], three[k]) for k in ('over', 'res'))


@pytest.mark.parametrize('m,nres', SHAPES)
def test_cphase_ft(ctx, m, nres):
    rng = NP.random.default_rng(4000 * m + nres)
    lead, wts = (1, 2, 3), windows(rng)
    inputs = [rng.standard_normal(s + (NCHAN,)) + 1j * rng.standard_normal(s + (NCHAN,)) for s in (lead, (1, 1, 3))]
    w = rng.integers(1, 4, lead + (NCHAN,)).astype(NP.float64)
    vs = rng.uniform(0.5, 2.0, (4, lead[0]))
    out = ctx.cphase_ft(inputs, wts, m, DF, weights=w, vscale=vs, nres=nres)
    assert out['stats']['route'] == route_of(m)
    ref = FK.transform(inputs, wts, m, DF, weights=w, vscale=vs, nres=nres)
    for kind in ('over', 'res'):
        for i, xs in enumerate(ref['xsum']):
            assert FK.spectrum_error(out[kind][i], ref[kind][i], xs, DF) <= FK.BOUND, (kind, i)
            assert not NP.any(out[kind][i][3]), (kind, i)
    for kind in ('lag_kernel', 'lag_kernel_res'):
        assert FK.spectrum_error(out[kind], ref[kind], ref['lag_xsum'], DF) <= FK.BOUND, kind
        assert not NP.any(out[kind][3]), kind
