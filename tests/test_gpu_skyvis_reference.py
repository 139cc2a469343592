"""GPU (-m gpu): every kernel family of the sky-sum ("Kernel families of the sky-sum") against the 40-digit reference of
tests/skyvis_reference.py -- not against oracle/, whose own error passes 1e-11 of S_f beyond 30 km baselines -- on seeded sets out to
3000 km, under THE RULE stated there: fp32 within 5e-6 S_f, fp64 within (1e-11 + 2 pi r 2^-53 N') S_f, every element, V and G alike,
output finite everywhere.  After each compute() what ctx.timing() reports is held to what the family must report, so that a case that
silently took another family fails.  k_phase_rotate (aux_kernels.hip), which forms its phase the same way, rotates the reference
cube of each length decade to a second phase centre under the same rule.

Out of scope: the batched catalogue launch (observe_catalog), whose geometry is formed on the device -- these cases give the device
the direction cosines as doubles, which is what makes the reference exact on them.

The split form of the packed fp32 kernel exists only where its eligibility rule admits it (kappa (|b| f / c)^2 <= 30: up to the 30 km
decade with these source sizes); beyond, the same request must report the unsplit packed kernel, and is held all the same."""
import collections
import math

import numpy as NP
import pytest

import skyvis_reference as R
from prisim_amd import _abi

pytestmark = pytest.mark.gpu

F64, F32 = _abi.PRISIM_FP64, _abi.PRISIM_FP32
AUTO, REC, DIRECT = _abi.PRISIM_KERNEL_AUTO, _abi.PRISIM_KERNEL_RECURRENCE, _abi.PRISIM_KERNEL_DIRECT

# taper: True / False = cases with / without source sizes only; None = both
Fam = collections.namedtuple('Fam', 'name prec ct nsplit kernel grad env taper r')
FAMILIES = [
    Fam('direct', F64, 0, 0, DIRECT, False, {}, None, R.R_DIRECT),
    Fam('direct_four_pass_grad', F64, 0, 0, DIRECT, True, {}, None, R.R_DIRECT),
    Fam('rec_f64_ct8', F64, 8, 1, AUTO, False, {}, None, R.R_RECURRENCE),                      # with the taper: the exact form
    Fam('rec_f64_ct16_split3', F64, 16, 3, AUTO, False, {}, False, R.R_RECURRENCE),
    Fam('rec_f64_ct32', F64, 32, 1, AUTO, False, {}, False, R.R_RECURRENCE),
    Fam('rec_f32_ct8', F32, 8, 1, AUTO, False, {}, None, 0),
    Fam('rec_f32_ct16', F32, 16, 1, AUTO, False, {}, None, 0),
    Fam('packed_f32_ct32', F32, 32, 1, AUTO, False, {}, False, 0),
    Fam('packed_f32_ct64', F32, 64, 1, AUTO, False, {}, False, 0),
    Fam('packed_f32_ct32_taper_grouped', F32, 32, 1, AUTO, False, {'PRISIM_HIP_TAPER_GROUP': '1'}, True, 0),
    Fam('packed_f32_ct64_taper_grouped', F32, 64, 1, AUTO, False, {'PRISIM_HIP_TAPER_GROUP': '1', 'PRISIM_HIP_TAPER_SPLIT': '0'}, True, 0),
    Fam('packed_f32_ct32_taper_exact', F32, 32, 1, AUTO, False, {'PRISIM_HIP_TAPER_GROUP': '0'}, True, 0),
    Fam('packed_f32_ct64_taper_exact', F32, 64, 1, AUTO, False, {'PRISIM_HIP_TAPER_GROUP': '0'}, True, 0),
    Fam('packed_f32_ct64_split_form', F32, 64, 1, AUTO, False, {}, True, 0),
    Fam('taper_f64_block_ct16', F64, 16, 1, AUTO, False, {}, True, R.R_RECURRENCE),
    Fam('taper_f64_block_ct32', F64, 32, 1, AUTO, False, {}, True, R.R_RECURRENCE),
    Fam('taper_f64_block_ct32_split3', F64, 32, 3, AUTO, False, {'PRISIM_HIP_WAVE_ITEMS': '0'}, True, R.R_RECURRENCE),
    Fam('taper_f64_wave_ct16', F64, 16, 3, AUTO, False, {}, True, R.R_RECURRENCE),
    Fam('taper_f64_wave_ct32', F64, 32, 3, AUTO, False, {}, True, R.R_RECURRENCE),
    Fam('taper_f64_exact_ct16', F64, 16, 1, AUTO, False, {'PRISIM_HIP_TAPER_F64_GROUP': '0'}, True, R.R_RECURRENCE),
    Fam('taper_f64_exact_ct32', F64, 32, 1, AUTO, False, {'PRISIM_HIP_TAPER_F64_GROUP': '0'}, True, R.R_RECURRENCE),
    Fam('grad_fused_f32', F32, 0, 0, AUTO, True, {}, None, 0),
    Fam('grad_fused_f64', F64, 0, 0, AUTO, True, {}, False, R.R_RECURRENCE),
    Fam('grad_fused_f64_taper_grouped', F64, 0, 0, AUTO, True, {}, True, R.R_RECURRENCE),
    Fam('grad_fused_f64_taper_exact', F64, 0, 0, AUTO, True, {'PRISIM_HIP_GRAD_TAPER_GROUP': '0'}, True, R.R_RECURRENCE),
    Fam('grad_four_pass_f64', F64, 0, 0, AUTO, True, {'PRISIM_HIP_FUSED_GRAD': '0'}, None, R.R_RECURRENCE),
    Fam('grad_four_pass_f32', F32, 0, 0, AUTO, True, {'PRISIM_HIP_FUSED_GRAD': '0'}, None, 0),
]
FAM = {f.name: f for f in FAMILIES}


def _groups(fam):
    g = ['len', 'edges', 'ragged', 'grids']
    if fam.prec == F32:
        g.append('sources')
    if fam.taper is not False:
        g.append('taper')
    return g


def _names(fam, group):
    out = []
    for taper in ((False, True) if fam.taper is None else (fam.taper,)):
        sfx = '_taper' if taper else ''
        if group == 'len':
            out += ['len_%s%s' % (tag, sfx) for tag, _ in R.LENGTHS]
        elif group == 'edges':
            out += ['edges' + sfx] + ['edges%s_row%d' % (sfx, i) for i in range(11)]
        elif group == 'ragged':
            out += ['ragged' + sfx]
        elif group == 'grids':
            out += ['grids_descending' + sfx, 'grids_one_channel' + sfx]
            if fam.env.get('PRISIM_HIP_TAPER_GROUP') != '1':                       # (the grouped form is stated for fine grids only; the
                out += ['grids_coarse' + sfx]                                      # hook that forces it on a coarse one is not a use)
            if fam.kernel == DIRECT:
                out += ['grids_nonuniform' + sfx]                      # a non-uniform grid is the direct kernel's alone
        elif group == 'sources':
            out += ['sources_%d%s' % (n, sfx) for n in (1, 3, 4, 5, 63, 64, 65, 130)]
        elif group == 'taper' and taper:
            out += ['taper_%g' % f for f in R.TAPER_FWHM] + ['taper_mixed']
    return out


PARAMS = [(f.name, g) for f in FAMILIES for g in _groups(f)]


@pytest.fixture(scope='module')
def sctx():
    c = _abi.Context(0)
    yield c
    c.close()


# ---- what timing() must report ---------------------------------------------------------------------------------------------------------
def _fine_grid(ch):
    if ch.size < 2:
        return abs(ch[0]) > 0.0
    df = (ch[-1] - ch[0]) / (ch.size - 1)
    return abs(df) <= 3.4e-3 * min(abs(ch[0]), abs(ch[-1]))


def _runs(fw):
    """Runs of consecutive sources of one size, as the library counts them: more than 8, no runs."""
    if fw is None:
        return []
    runs, lo = [], 0
    for s in range(1, fw.size + 1):
        if s == fw.size or fw[s] != fw[lo]:
            runs.append(fw[lo])
            lo = s
    return runs if len(runs) <= 8 else []


def _split_eligible(c):
    runs = _runs(c.fw)
    if not runs or not _fine_grid(c.ch) or not any(f > 0.0 for f in runs):
        return 0
    kmax = max(math.log(2.0) * (2.0 * math.sin(math.radians(f) / 2.0)) ** 2 for f in runs)
    fmax, fmin = float(NP.abs(c.ch).max()), float(min(abs(c.ch[0]), abs(c.ch[-1])))
    df = abs(c.ch[1] - c.ch[0]) if c.ch.size > 1 else 0.0
    umax = kmax * (float(NP.sqrt(NP.sum(c.bl ** 2, axis=1)).max()) * fmax / R.C_LIGHT) ** 2
    return len(runs) if (umax <= 30.0 and 2.0 * umax * df <= 0.125 * fmin) else 0


def _expect(fam, c, tm, nsplit_req):
    taper = c.fw is not None
    fused = fam.grad and fam.kernel != DIRECT and fam.env.get('PRISIM_HIP_FUSED_GRAD') != '0'
    if fam.kernel == DIRECT:
        assert (tm['last_kernel_id'], tm['last_chan_tile'], tm['last_nsplit']) == (DIRECT, 1, 1), tm
        assert tm['last_taper_group'] == 0 and tm['last_taper_split'] == 0 and tm['last_lift_groups'] == 0, tm
        return
    assert tm['last_kernel_id'] == REC, tm
    tile = None
    if fused:
        tile = 16 if fam.prec == F32 else (16 if taper and fam.env.get('PRISIM_HIP_GRAD_TAPER_GROUP') == '0' else 32)
    elif fam.ct:
        tile = min(fam.ct, 32 if fam.prec == F64 else 64)
        if fam.prec == F32 and taper and not _fine_grid(c.ch):
            tile = min(tile, 32)                                                   # coarse grids: the 32-channel cap of the exact form
    if tile is not None:
        assert tm['last_chan_tile'] == tile, (tile, tm)
    pk = fam.prec == F32 and (fused or tile in (32, 64))
    nsrc = c.dc.shape[0]
    if fused or nsplit_req == 1:
        assert tm['last_nsplit'] == 1, tm
    elif nsplit_req > 1:
        wave_rule = (fam.prec == F64 and taper and tile in (16, 32) and c.bl.shape[0] <= 256 and
                     fam.env.get('PRISIM_HIP_TAPER_F64_GROUP') != '0')
        if wave_rule:                                                              # make_plan: pieces of whole groups of four sources
            per = -(-(-(-nsrc // nsplit_req)) // 4) * 4                            # ceil(ceil(nsrc / pieces) / 4) * 4
            assert tm['last_nsplit'] == max(1, -(-nsrc // per)), (per, tm)
        else:
            assert 1 <= tm['last_nsplit'] <= nsplit_req and (nsrc < 33 or tm['last_nsplit'] >= 2), tm
    if tile is not None:
        forced = fam.env.get('PRISIM_HIP_TAPER_GROUP')
        tg = taper and (forced == '1' if forced is not None else _fine_grid(c.ch))
        assert tm['last_taper_group'] == (1 if pk and tg else 0), tm
        want_split = 0
        if pk and tg and taper and tile == 64 and not fam.grad and fam.env.get('PRISIM_HIP_TAPER_SPLIT') != '0' and nsplit_req == 1:
            want_split = _split_eligible(c)
        if nsplit_req == 1:
            assert tm['last_taper_split'] == want_split, (want_split, tm)
        if c.name.startswith('len_') and not (taper and pk):                       # (the packed taper kernel never lifts: it reports 0)
            if c.name.startswith('len_3e2'):
                assert tm['last_lift_groups'] >= 1, tm
            elif not c.name.startswith('len_3e3'):
                assert tm['last_lift_groups'] == 0, tm


# ---- one compute, held to the rule ---------------------------------------------------------------------------------------------------
def _hold(fam, c, ref, v, g, what):
    single = c.dc.shape[0] == 1
    if fam.prec == F32:
        # one source on 64-channel tiles under the default hooks: the per-term figure of test_fp32_single_source_worst_case_per_term
        bar = 4e-6 if (single and fam.name in ('packed_f32_ct64', 'packed_f32_ct64_split_form')) else R.BAR_F32
        bound = bar * ref.S[None, :] * NP.ones_like(ref.N)
    else:
        bound = R.f64_bound(fam.r, ref.N) * ref.S[None, :]
    s = NP.where(ref.S > 0.0, ref.S, 1.0)[None, :]
    worst = 0.0
    for label, got, want in [('V', v, ref.V)] + ([('G%d' % k, g[k], ref.G[k]) for k in range(3)] if g is not None else []):
        assert NP.all(NP.isfinite(got.view(NP.float64))), (what, label)
        err = NP.abs(got - want)
        worst = max(worst, float(NP.max(err / s)))
        bad = err > bound
        assert not NP.any(bad), (what, label, int(bad.sum()), 'worst err / S_f', float(NP.max(err / s)), 'bound / S_f there',
                                 float((bound / s).ravel()[NP.argmax(err / s)]))
    return worst


def _run(ctx, fam, name, nsplit=None):
    c, ref = R.get(name)
    nsplit = fam.nsplit if nsplit is None else nsplit
    ctx.set_array(c.bl, c.ch)
    ctx.set_tuning(fam.ct, 0, nsplit)
    ctx.set_sky(c.dc, c.pb, c.pc, fwhm_deg=c.fw)
    ctx.compute(precision=fam.prec, kernel=fam.kernel, want_grad=fam.grad)
    tm = ctx.timing()
    out = ctx.get_vis(want_grad=fam.grad)
    v, g = out if fam.grad else (out, None)
    _expect(fam, c, tm, nsplit)
    return _hold(fam, c, ref, v, g, (fam.name, name, nsplit))


@pytest.mark.parametrize('family,group', PARAMS)
def test_family_against_the_40_digit_reference(sctx, monkeypatch, family, group):
    fam = FAM[family]
    for k, val in fam.env.items():
        monkeypatch.setenv(k, val)
    splits = (None,)
    if group == 'sources':
        # fp32 accumulators flushed every 16 sources: several read-modify-write flushes, the last one partial; source splits 1 and 3
        monkeypatch.setenv('PRISIM_HIP_FLUSH_SRC', '16')
        splits = (1, 3)
    worst = {}
    try:
        for name in _names(fam, group):
            for ns in splits:
                key = name.split('_row')[0] if group == 'edges' else name
                worst[key] = max(worst.get(key, 0.0), _run(sctx, fam, name, ns))
    finally:
        sctx.set_tuning(0, 0, 0)
    for key in sorted(worst):
        print('WORST %-34s %-26s %.2e' % (family, key, worst[key]))


# ---- k_phase_rotate ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag', [t for t, _ in R.LENGTHS])
def test_phase_rotate_against_the_reference_product(sctx, tag):
    """cube *= exp(-2 pi i f b.d / c), d = s_pc2 - s_pc as doubles: the reference cube of the decade, rotated on the device, against
    the product formed in longdouble from the exactly reduced phase, under (1e-11 + 2 pi R_ROTATE u N_d) S_f (N_d: the phase scale of d)."""
    c, ref = R.get('len_' + tag)
    d, (pre, pim), nd = R.rotation('len_' + tag)
    sctx.set_array(c.bl, c.ch)
    sctx.set_vis(ref.V, 0)
    sctx.phase_rotate(1, d[None, :])
    got = sctx.get_vis()
    vr, vi = ref.V.real.astype(R.LD), ref.V.imag.astype(R.LD)
    want = (vr * pre - vi * pim).astype(NP.float64) + 1j * (vr * pim + vi * pre).astype(NP.float64)
    assert NP.all(NP.isfinite(got.view(NP.float64)))
    err = NP.abs(got - want) / ref.S[None, :]
    print('WORST %-34s %-26s %.2e' % ('k_phase_rotate', 'len_' + tag, float(err.max())))
    assert NP.all(err <= R.f64_bound(R.R_ROTATE, nd)), float(NP.max(err / R.f64_bound(R.R_ROTATE, nd)))


# ---- the stated phase range ----------------------------------------------------------------------------------------------------------
def test_set_array_refuses_phases_at_the_quadrant_range_and_accepts_the_largest_below(sctx):
    """|4 phase| < 2^31 before (int)q in the kernels: prisim_hip_set_array refuses max|b| 2 max|f| / c >= 2^29 cycles (|s - s_pc| <= 2) on
    the host; no kernel runs.  With f = c Hz the figure is 2 |b| exactly."""
    f = NP.array([float(R.C_LIGHT)])
    with pytest.raises(ValueError, match='2\\^29'):
        sctx.set_array(NP.array([[2.0 ** 28, 0.0, 0.0], [1.0, 2.0, 3.0]]), f)
    with pytest.raises(ValueError, match='2\\^29'):
        sctx.set_array(NP.array([[0.0, -2.0 ** 28, 0.0]]), -f)
    sctx.set_array(NP.array([[NP.nextafter(2.0 ** 28, 0.0), 0.0, 0.0], [1.0, 2.0, 3.0]]), f)      # the largest accepted value
    c, _ = R.get('len_3e2')
    sctx.set_array(c.bl, c.ch)
