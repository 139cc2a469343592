"""GPU (-m gpu): the leapfrog step rotation of the packed fp32 sky-sum (k_skyvis_rec_f32pk, k_skyvis_grad_f32pk) at its edges, against
the fp64 C oracle at the fp32 tolerance (5e-6 of S_f = sum_s |pbflux[s, f]|).  The sky-sum cases run 64-channel tiles, i.e. the full 32-step (up, down)
chains (the fused gradient kernel always runs 16-channel tiles), on baseline groups (256 baselines each) whose lift flag the host sets when max|b| max|s - s_pc| df / c
<= 1/8 cycle.  The longest baseline of a group is laid along s - s_pc of one source, so that source's step sits AT the group's bound.

A CPU-side check of the same change (the packed-FMA census of the lifting loops) is in test_leapfrog_census.py.
"""
import numpy as NP
import pytest

from oracle import skyvis_oracle as O, c_oracle as CO
from prisim_amd import _abi

pytestmark = pytest.mark.gpu

TOL = 5e-6
C = 299792458.0
PC = NP.array([0.0, 0.0, 1.0])
F0 = 150e6
NCHAN = 128


def relerr(v, ref, pb):
    return float(NP.max(NP.abs(v - ref) / O.abs_flux_sum(pb)[None, :]))


def _sky(rng, nsrc, radius=0.6):
    """nsrc directions within `radius` of the zenith (the phase centre); source 0 sits AT the phase centre, source 1 at the largest
    offset (it sets max|s - s_pc|)."""
    r = NP.sqrt(rng.uniform(0.0, 1.0, nsrc)) * radius
    a = rng.uniform(0.0, 2 * NP.pi, nsrc)
    r[0], r[1] = 0.0, radius
    dc = NP.stack((r * NP.cos(a), r * NP.sin(a), NP.sqrt(1.0 - r * r)), axis=1)
    pb = rng.uniform(0.2, 2.0, (nsrc, NCHAN)) * (1.0 + 0.1 * NP.sin(NP.arange(NCHAN) / 7.0))[None, :]
    return dc, pb


def _group(rng, n, length, direction):
    """n baselines of at most `length` metres; the first is exactly `length` along `direction` (a unit vector)."""
    bl = rng.uniform(-1.0, 1.0, (n, 3)) * NP.array([1.0, 1.0, 0.05])
    bl *= (rng.uniform(0.05, 0.99, n) * length / NP.linalg.norm(bl, axis=1))[:, None]
    bl[0] = length * direction
    return bl


def _plan(dc, steps, rng, n=256):
    """One baseline group per entry of `steps`: the group's largest step phase, in cycles, is steps[g].  Returns (baselines, channels)."""
    off = dc[1] - PC
    dmax = float(NP.max(NP.linalg.norm(dc - PC, axis=1)))
    df = 1e5
    lmax = steps[0] * C / (dmax * df)
    bl = NP.concatenate([_group(rng, n, lmax * st / steps[0], off / NP.linalg.norm(off)) for st in steps])
    ch = F0 + df * NP.arange(NCHAN)
    return bl, ch


def _run(ctx, bl, ch, dc, pb, want_grad=False, fwhm=None, nsplit=1):
    ctx.set_array(bl, ch)
    ctx.set_tuning(64, 0, nsplit)
    try:
        out = ctx.skyvis(dc, pb, PC, fwhm_deg=fwhm, precision=_abi.PRISIM_FP32, kernel=_abi.PRISIM_KERNEL_RECURRENCE, want_grad=want_grad)
        return out, ctx.timing()
    finally:
        ctx.set_tuning(0, 0, 0)


def _check(v, bl, ch, dc, pb, fwhm=None, grad=None):
    if grad is None:
        ref = CO.skyvis(bl, ch, dc, pb, PC, fwhm_deg=fwhm)
    else:
        ref, gref = CO.skyvis(bl, ch, dc, pb, PC, fwhm_deg=fwhm, gradient=True)
        errs = [relerr(grad[k], gref[k], pb) for k in range(3)]
        assert max(errs) <= TOL, errs
    err = relerr(v, ref, pb)
    assert err <= TOL, err


def test_step_just_under_the_lift_limit(ctx):
    """One group whose largest step is 0.12499 cycle: the leapfrog coefficient 2 sin(alpha) is at its largest (|alpha| ~ pi/4)."""
    rng = NP.random.default_rng(11)
    dc, pb = _sky(rng, 48)
    bl, ch = _plan(dc, [0.12499], rng)
    v, tm = _run(ctx, bl, ch, dc, pb)
    assert tm['last_chan_tile'] == 64 and tm['last_lift_groups'] == 1, tm
    _check(v, bl, ch, dc, pb)


def test_zero_and_tiny_steps(ctx):
    """theta ~ 0: zero-length and millimetre baselines, sources at and next to the phase centre.  A chain whose step is exactly 1 must
    stay constant (z_{k+1} = z_{k-1} = z_k)."""
    rng = NP.random.default_rng(12)
    dc, pb = _sky(rng, 40, radius=1e-4)
    bl = rng.uniform(-1e-3, 1e-3, (256, 3))
    bl[:8] = 0.0
    ch = F0 + 1e5 * NP.arange(NCHAN)
    v, tm = _run(ctx, bl, ch, dc, pb)
    assert tm['last_chan_tile'] == 64 and tm['last_lift_groups'] == 1, tm
    _check(v, bl, ch, dc, pb)
    # zero baselines: V = sum_s pbflux exactly up to the fp32 accumulation
    assert NP.max(NP.abs(v[:8] - pb.sum(axis=0)[None, :]) / O.abs_flux_sum(pb)[None, :]) <= TOL


def test_groups_either_side_of_the_lift_limit(ctx):
    """Two groups, largest steps 0.1249 and 0.1251 cycle: the first takes the leapfrog body, the second the 4-instruction rotation,
    in one launch."""
    rng = NP.random.default_rng(13)
    dc, pb = _sky(rng, 48)
    bl, ch = _plan(dc, [0.1249, 0.1251], rng)
    v, tm = _run(ctx, bl, ch, dc, pb)
    assert tm['last_chan_tile'] == 64 and tm['last_lift_groups'] == 1, tm
    _check(v, bl, ch, dc, pb)


@pytest.mark.parametrize('nsplit', [1, 3])
def test_many_sources_across_flushes(ctx, nsplit, monkeypatch):
    """300 sources flushed every 16 (a ragged last segment) and split into partial cubes: the chains are re-seeded per source, the
    accumulators survive read-modify-write flushes."""
    monkeypatch.setenv('PRISIM_HIP_FLUSH_SRC', '16')
    rng = NP.random.default_rng(14)
    dc, pb = _sky(rng, 300)
    bl, ch = _plan(dc, [0.12, 0.05], rng)
    v, tm = _run(ctx, bl, ch, dc, pb, nsplit=nsplit)
    assert tm['last_chan_tile'] == 64 and tm['last_lift_groups'] == 2, tm
    _check(v, bl, ch, dc, pb)


@pytest.mark.parametrize('taper', [False, True])
def test_fp32_gradient_either_side_of_the_lift_limit(ctx, taper):
    """The fused fp32 gradient (k_skyvis_grad_f32pk): the pre-multiplied-row body on a leapfrog group and on a rotation group; with the
    source-shape taper, the taper gradient bodies beside them."""
    rng = NP.random.default_rng(15 + taper)
    dc, pb = _sky(rng, 64)
    bl, ch = _plan(dc, [0.12499, 0.1251], rng)
    fwhm = rng.uniform(0.2, 1.0, dc.shape[0]) if taper else None
    (v, g), tm = _run(ctx, bl, ch, dc, pb, want_grad=True, fwhm=fwhm)
    assert tm['last_chan_tile'] == 16, tm
    _check(v, bl, ch, dc, pb, fwhm=fwhm, grad=g)
