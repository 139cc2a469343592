"""GPU (-m gpu): the per-axis step bound that decides which baseline groups (of 256) run the leapfrog rotation (step_bound.h):
    step = min(maxlen dmax, maxh hmax + maxz zmax) |df| / c  <=  1/8 cycle (fp32), 1/4 (fp64),
with dmax / hmax / zmax the sky's largest |e|, |e_xy|, |e_z|, e = s - s_pc.  The arrays are two groups of 256 baselines over 128 channels;
the longest baseline of the group under test lies along the horizontal part of e of the source with the largest horizontal offset, so that
source's step sits AT the group's per-axis bound while the whole-vector rule maxlen dmax reads well above the limit.  Every case first
asserts its premise in numpy (the old rule, the new rule, the brute-force largest step), then the counts the library reports
(last_sum_lift_groups: the kernel's flags; last_lift_groups: the length rule) and parity with the fp64 C oracle at the project's
tolerances (5e-6 of S_f = sum_s |pbflux[s, f]| in fp32, 1e-11 in fp64).

CPU-side checks of the bound itself are in test_step_bound.py."""
import functools

import numpy as NP
import pytest

from oracle import skyvis_oracle as O, c_oracle as CO
from prisim_amd import _abi, geometry as GEOM

pytestmark = pytest.mark.gpu

TOL32, TOL64 = 5e-6, 1e-11
C = 299792458.0
ZEN = NP.array([0.0, 0.0, 1.0])
F0, DF, NCHAN = 150e6, 1e5, 128
CH = F0 + DF * NP.arange(NCHAN)
ALT_MIN = 10.0


def relerr(v, ref, pb):
    return float(NP.max(NP.abs(v - ref) / O.abs_flux_sum(pb)[None, :]))


def sky_altaz(rng, nsrc):
    """(alt, az) degrees of nsrc sources down to 10 degrees altitude; source 0 at the zenith, source 1 AT 10 degrees (the largest
    horizontal offset from the zenith, cos 10 = 0.9848, and the largest |e| = 1.2856)"""
    sin_alt = rng.uniform(NP.sin(NP.radians(ALT_MIN + 2.0)), 1.0, nsrc)
    alt = NP.degrees(NP.arcsin(sin_alt))
    az = rng.uniform(0.0, 360.0, nsrc)
    alt[0], alt[1] = 90.0, ALT_MIN
    return NP.stack((alt, az), axis=1)


def pbflux(rng, nsrc):
    return rng.uniform(0.2, 2.0, (nsrc, NCHAN)) * (1.0 + 0.1 * NP.sin(NP.arange(NCHAN) / 7.0))[None, :]


def extrema(dc, pc):
    e = dc - pc[None, :]
    h2 = e[:, 0] ** 2 + e[:, 1] ** 2
    z2 = e[:, 2] ** 2
    return float(NP.sqrt((h2 + z2).max())), float(NP.sqrt(h2.max())), float(NP.sqrt(z2.max()))


def group_steps(bl, dc, pc):
    """per group of 256: (old rule, new rule, brute-force largest step), in cycles"""
    d, h, z = extrema(dc, pc)
    e = dc - pc[None, :]
    out = []
    for g in range((bl.shape[0] + 255) // 256):
        b = bl[g * 256:(g + 1) * 256]
        maxlen, maxh, maxz = NP.linalg.norm(b, axis=1).max(), NP.hypot(b[:, 0], b[:, 1]).max(), NP.abs(b[:, 2]).max()
        old = maxlen * d * DF / C
        new = min(maxlen * d, maxh * h + maxz * z) * DF / C
        out.append((old, new, NP.abs(b @ e.T).max() * DF / C))
    return NP.array(out)


def planar_group(rng, n, length, direction):
    """n horizontal baselines of at most 0.99 `length`; the first is exactly `length` along `direction` (a horizontal unit vector)"""
    a = rng.uniform(0.0, 2 * NP.pi, n)
    r = rng.uniform(0.05, 0.99, n) * length
    bl = NP.stack((r * NP.cos(a), r * NP.sin(a), NP.zeros(n)), axis=1)
    bl[0] = length * direction
    return bl


def planar_array(rng, dc, pc, steps, n=256):
    """one planar group per entry of `steps`, whose per-axis bound is steps[g] cycles: its longest baseline lies along e_xy of the source
    with the largest |e_xy|"""
    e = dc - pc[None, :]
    hor = NP.hypot(e[:, 0], e[:, 1])
    s = int(NP.argmax(hor))
    direction = NP.array([e[s, 0], e[s, 1], 0.0]) / hor[s]
    return NP.concatenate([planar_group(rng, n, st * C / (hor[s] * DF), direction) for st in steps])


def limit(f32=True):
    return (0.125 if f32 else 0.25) * (1.0 - 1e-9)


def run(ctx, bl, dc, pb, pc=ZEN, ct=64, nsplit=1, precision=_abi.PRISIM_FP32, want_grad=False, fwhm=None):
    ctx.set_array(bl, CH)
    ctx.set_tuning(ct, 0, nsplit)
    try:
        out = ctx.skyvis(dc, pb, pc, fwhm_deg=fwhm, precision=precision, kernel=_abi.PRISIM_KERNEL_RECURRENCE, want_grad=want_grad)
        return out, ctx.timing()
    finally:
        ctx.set_tuning(0, 0, 0)


@functools.lru_cache(maxsize=None)
def planar_case(step, seed=21, nsrc=300, second=0.2):
    """group 0 at `step` cycles under the per-axis bound, group 1 at `second` (beyond the limit under either rule); the oracle's V and gradient"""
    rng = NP.random.default_rng(seed)
    dc = GEOM.altaz2dircos(sky_altaz(rng, nsrc))
    pb = pbflux(rng, nsrc)
    bl = planar_array(rng, dc, ZEN, [step, second])
    ref, gref = CO.skyvis(bl, CH, dc, pb, ZEN, gradient=True)
    for a in (dc, pb, bl, ref, gref):
        a.setflags(write=False)
    return dc, pb, bl, ref, gref


def test_planar_premise():
    """(no GPU work) the construction: the new bound is met by the brute-force step, the old rule reads above the limit"""
    for step, flagged in ((0.1249, True), (0.1251, False)):
        dc, _, bl, _, _ = planar_case(step)
        st = group_steps(bl, dc, ZEN)
        assert abs(st[0, 1] - step) < 1e-9 and abs(st[0, 2] - step) < 1e-9 and st[0, 0] > 0.16, st
        assert (st[0, 1] <= limit()) == flagged and st[0, 0] > limit()
        assert st[1, 1] > limit() and st[1, 0] > limit()
    d, h, z = extrema(planar_case(0.1249)[0], ZEN)
    assert abs(h - NP.cos(NP.radians(ALT_MIN))) < 1e-12 and abs(z - (1.0 - NP.sin(NP.radians(ALT_MIN)))) < 1e-12 and abs(d - NP.hypot(h, z)) < 1e-12


@pytest.mark.parametrize('nsplit', [1, 3])
def test_planar_newly_flagged(ctx, nsplit):
    """0.1249 cycle under the per-axis bound, 0.163 under the whole-vector rule: the group lifts now; |alpha| is AT pi/4 for source 1"""
    dc, pb, bl, ref, _ = planar_case(0.1249)
    v, tm = run(ctx, bl, dc, pb, nsplit=nsplit)
    assert tm['last_chan_tile'] == 64 and tm['last_nsplit'] == nsplit, tm
    assert tm['last_sum_lift_groups'] == 1 and tm['last_lift_groups'] == 0, tm
    err = relerr(v, ref, pb)
    print('planar 0.1249 nsplit %d: err / S_f = %.3e' % (nsplit, err))
    assert err <= TOL32, err


def test_planar_newly_flagged_gradient(ctx):
    """the fused fp32 gradient (16-channel tiles) on the newly flagged group"""
    dc, pb, bl, ref, gref = planar_case(0.1249)
    (v, g), tm = run(ctx, bl, dc, pb, ct=0, want_grad=True)
    assert tm['last_chan_tile'] == 16, tm
    assert tm['last_sum_lift_groups'] == 1 and tm['last_lift_groups'] == 0, tm
    errs = [relerr(v, ref, pb)] + [relerr(g[k], gref[k], pb) for k in range(3)]
    print('planar 0.1249 gradient: err / S_f = %s' % ' '.join('%.3e' % e for e in errs))
    assert max(errs) <= TOL32, errs


def test_planar_just_over(ctx):
    """0.1251 cycle under the per-axis bound: not flagged"""
    dc, pb, bl, ref, _ = planar_case(0.1251)
    v, tm = run(ctx, bl, dc, pb)
    assert tm['last_chan_tile'] == 64, tm
    assert tm['last_sum_lift_groups'] == 0 and tm['last_lift_groups'] == 0, tm
    err = relerr(v, ref, pb)
    print('planar 0.1251: err / S_f = %.3e' % err)
    assert err <= TOL32, err


def test_vertical_term(ctx):
    """group 0: its longest baseline is vertical, 0.13 cycle under the 10-degree source through |b_z| zmax alone, beside metre-long horizontal
    companions -- it must not lift (its brute-force step is 0.13); group 1 is short and lifts under either rule"""
    rng = NP.random.default_rng(22)
    dc = GEOM.altaz2dircos(sky_altaz(rng, 64))
    pb = pbflux(rng, 64)
    _, h, z = extrema(dc, ZEN)
    g0 = planar_group(rng, 256, 1.0, NP.array([1.0, 0.0, 0.0]))
    g0[0] = [0.0, 0.0, 0.13 * C / (z * DF)]
    g0[1:, 2] = rng.uniform(-0.5, 0.5, 255) * g0[0, 2]
    bl = NP.concatenate((g0, planar_array(rng, dc, ZEN, [0.05])))
    st = group_steps(bl, dc, ZEN)
    assert st[0, 1] > limit() and st[0, 2] > limit() and 1.0 * h * DF / C < 1e-3, st          # premise: the vertical term alone exceeds 1/8
    assert abs(st[0, 2] - 0.13) < 1e-9 and st[1, 0] <= limit() and st[1, 1] <= limit(), st
    v, tm = run(ctx, bl, dc, pb)
    assert tm['last_chan_tile'] == 64, tm
    assert tm['last_sum_lift_groups'] == 1 and tm['last_lift_groups'] == 1, tm
    err = relerr(v, CO.skyvis(bl, CH, dc, pb, ZEN), pb)
    print('vertical term: err / S_f = %.3e' % err)
    assert err <= TOL32, err


def test_phase_centre_off_the_zenith(ctx):
    """the extrema are taken about s_pc: about a phase centre at 60 degrees altitude the largest horizontal offset is larger than about
    the zenith.  Groups at 0.1249 and 0.1251 cycle under the per-axis bound about s_pc; extrema about the zenith would flag both."""
    rng = NP.random.default_rng(23)
    dc = GEOM.altaz2dircos(sky_altaz(rng, 64))
    pb = pbflux(rng, 64)
    pc = GEOM.altaz2dircos(NP.array([[60.0, 30.0]]))[0]
    bl = planar_array(rng, dc, pc, [0.1249, 0.1251])
    st = group_steps(bl, dc, pc)
    assert st[0, 1] <= limit() < st[1, 1] and NP.all(st[:, 0] > limit()), st
    assert abs(st[0, 2] - 0.1249) < 1e-9 and abs(st[1, 2] - 0.1251) < 1e-9, st
    assert NP.all(group_steps(bl, dc, ZEN)[:, 1] <= limit())                                   # premise: the zenith's extrema would flag both
    v, tm = run(ctx, bl, dc, pb, pc=pc)
    assert tm['last_chan_tile'] == 64, tm
    assert tm['last_sum_lift_groups'] == 1 and tm['last_lift_groups'] == 0, tm
    err = relerr(v, CO.skyvis(bl, CH, dc, pb, pc), pb)
    print('phase centre off the zenith: err / S_f = %.3e' % err)
    assert err <= TOL32, err


@pytest.mark.parametrize('form', ['packed', 'split'])
def test_taper_on_newly_flagged(ctx, form):
    """the source-shape taper on the newly flagged group, which now runs the non-re-anchored bodies: sizes that vary from source to source
    (the packed fp32 taper kernel), and one size for the whole sky (its split form).  Parity only."""
    dc, pb, bl, _, _ = planar_case(0.1249)
    rng = NP.random.default_rng(24)
    fwhm = rng.uniform(0.2, 1.0, dc.shape[0]) if form == 'packed' else NP.full(dc.shape[0], 0.6)
    v, tm = run(ctx, bl, dc, pb, fwhm=fwhm)
    assert tm['last_chan_tile'] == 64, tm
    err = relerr(v, CO.skyvis(bl, CH, dc, pb, ZEN, fwhm_deg=fwhm), pb)
    print('taper %s: err / S_f = %.3e (%s)' % (form, err, {k: tm[k] for k in ('last_taper_group', 'last_taper_split')}))
    assert err <= TOL32, err


def test_fp64_newly_flagged(ctx):
    """fp64: 0.2499 cycle under the per-axis bound, 0.326 under the whole-vector rule"""
    dc, pb, bl, ref, _ = planar_case(0.2499, second=0.4)
    st = group_steps(bl, dc, ZEN)
    assert st[0, 1] <= limit(False) < st[0, 0] and abs(st[0, 2] - 0.2499) < 1e-9 and NP.all(st[1, :2] > limit(False)), st
    v, tm = run(ctx, bl, dc, pb, ct=0, precision=_abi.PRISIM_FP64)
    assert tm['last_sum_lift_groups'] == 1 and tm['last_lift_groups'] == 0, tm
    err = relerr(v, ref, pb)
    print('fp64 0.2499: err / S_f = %.3e' % err)
    assert err <= TOL64, err


@pytest.mark.parametrize('path', ['three_pass', 'one_block'])
def test_device_extrema(ctx, path, monkeypatch):
    """the same planar sky as an alt-az catalogue through set_catalog / observe_catalog, where the device forms the extrema: the three
    passes (a catalogue above the small-catalogue limit of 16384 sources: the sky's 300 and 16400 more below the horizon, which the region
    of interest drops) and the one-block kernel (the 300 alone; it serves arrays of at most 256 baselines, so group 0 alone, through the
    per-snapshot chain).  The flag count equals the numpy prediction and V the set_sky result of the same sources."""
    dc, pb, bl, _, _ = planar_case(0.1249)
    rng = NP.random.default_rng(25)
    nsrc = dc.shape[0]
    altaz = GEOM.dircos2altaz(dc)
    assert NP.max(NP.abs(GEOM.altaz2dircos(altaz) - dc)) < 1e-12
    flux, spx = rng.uniform(1.0, 10.0, nsrc), rng.uniform(-1.0, -0.5, nsrc)
    if path == 'three_pass':
        nfill = 16400
        altaz = NP.concatenate((altaz, NP.stack((NP.full(nfill, -20.0), rng.uniform(0.0, 360.0, nfill)), axis=1)))
        flux, spx = NP.concatenate((flux, NP.ones(nfill))), NP.concatenate((spx, NP.zeros(nfill)))
        expect = (1, 0)
    else:
        bl = bl[:256]
        monkeypatch.setenv('PRISIM_HIP_WAVE_ITEMS', '0')          # the per-snapshot chain: small arrays otherwise share one fp64 launch
        expect = (1, 0)
    st = group_steps(bl, dc, ZEN)
    assert int(NP.sum(st[:, 1] <= limit())) == expect[0] and int(NP.sum(st[:, 0] <= limit())) == expect[1], st
    pbf = flux[:nsrc, None] * (CH[None, :] / F0) ** spx[:nsrc, None]
    v_sky, tm_sky = run(ctx, bl, dc, pbf)
    assert (tm_sky['last_sum_lift_groups'], tm_sky['last_lift_groups']) == expect, tm_sky
    ctx.set_array(bl, CH)
    ctx.set_tuning(64, 0, 1)
    try:
        ctx.set_catalog(altaz, 'altaz', flux_ref=flux, spindex=spx, ref_freq_hz=F0)
        counts = ctx.observe_catalog(ctx.make_obs(-30.7224), NP.array([0.0]), ZEN, precision=_abi.PRISIM_FP32)
        tm = ctx.timing()
        v = ctx.get_vis(slot=0)
    finally:
        ctx.set_tuning(0, 0, 0)
    assert int(counts[0]) == nsrc, counts
    assert tm['last_chan_tile'] == 64 and tm['last_batch_snapshots'] == 1, tm
    assert (tm['last_sum_lift_groups'], tm['last_lift_groups']) == expect, tm
    err = relerr(v, v_sky, pbf)
    print('device extrema %s: |V - V(set_sky)| / S_f = %.3e' % (path, err))
    assert err <= TOL32, err
