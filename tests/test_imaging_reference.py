"""CPU: the 40-digit reference of the dirty image (tests/imaging_reference.py) held to itself and to what it is for.

  * its two routes agree to 1e-17 of the scale on a seeded sub-sample of every set tests/test_gpu_imaging_reference.py runs;
  * exact properties: d = 0, the antipode, V(-b) against conj V(b), a point source, whole and half cycles;
  * the floor of tests/imaging_checker.py (dirty_image, stepped_image) per decade, asserted both ways: inside 1e-11 of the scale up to
    30 km, outside from 300 km on, and on the narrow field an error that follows N_b, not N';
  * a float64 numpy restatement of the device's own statement (k_img_dirs, img_rows direct and stepped, cycles_phasor with a correctly
    rounded sincospi) passes THE RULE on every set, and three wrong variants of it -- 1 / c rounded to float32, the normalisation left
    out, the third component of d dropped -- each fail it where the sets are meant to see them.

Measured 2026-10-21 on x86-64 (printed by the tests; the tables stand in the docstring of tests/imaging_reference.py):
    route gap over all sets 1.2e-19 of the scale (asserted <= 1e-17)
    wrong variants, the worst deviation over the bound:  1 / c in float32 1.6e6, no normalisation 6.2e8,
    d.z dropped 3.7e10 (4.2e9 and 3.8e8 on the narrow field at 300 m and 300 km)"""
import os
import sys

import numpy as NP
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import imaging_checker as IK  # noqa: E402
import imaging_reference as R  # noqa: E402
import skyvis_reference as SR  # noqa: E402

LD = NP.longdouble
BIG = (33, 33, 65, 2)
SETS = R.sets()


@pytest.fixture(scope='module')
def geos():
    """name -> (case, Geometry), each made once for the module."""
    made = {}

    def get(name):
        if name not in made:
            c = dict((n, t) for n, t, _ in SETS)[name]()
            made[name] = (c, R.geometry_case(c))
        return made[name]
    return get


# ---- the device's statement in float64 numpy ---------------------------------------------------------------------------------------------

def _round(x):
    return NP.asarray(x).astype(NP.float64)


def _phasor(x):
    """cycles_phasor: r = x - rint(x) exact, then sincospi(2 r) correctly rounded (through longdouble)."""
    r = x - NP.rint(x)
    ang = r.astype(LD) * (LD(2) * SR.to_ld(SR.MP.pi))
    return _round(NP.cos(ang)), _round(NP.sin(ang))


def device_image(c, weights, kind, route, chan_avg, variant=None):
    """k_img_dirs, img_tile_pass and k_img_sum operation by operation in float64 (numpy contracts nothing); the accumulation of a
    (pixel, channel) over (t, b), an FMA chain on the device (nt nbl u of the scale at most), and the recurrence's FMAs are formed in
    longdouble and rounded.  variant: None, or one of the three wrong statements."""
    u, rot, beta, pc = c['unitvec'], c['rot'], c['beta'], c['pc']
    bl, fq = c['baselines'], c['freqs']
    nt, nbl, nchan = rot.shape[0], bl.shape[0], fq.size
    t = u[None, :, :] + beta[:, None, :]
    v = NP.stack([(rot[:, i, 0, None] * t[..., 0] + rot[:, i, 1, None] * t[..., 1]) + rot[:, i, 2, None] * t[..., 2] for i in range(3)], axis=-1)
    nrm = NP.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])
    s = v if variant == 'no normalisation' else v / nrm[..., None]
    d = s - pc[:, None, :]
    inv_c = float(NP.float32(1.0 / 299792458.0)) if variant == '1/c in float32' else 1.0 / 299792458.0
    b = bl * inv_c
    tau = b[None, None, :, 0] * d[:, :, None, 0] + b[None, None, :, 1] * d[:, :, None, 1]
    if variant != 'd.z dropped':
        tau = tau + b[None, None, :, 2] * d[:, :, None, 2]              # (nt, npix, nbl)
    if route == 'direct':
        cs, sn = _phasor(fq * tau[..., None])
    else:
        df = R.grid_df(fq)
        cs, sn = NP.empty(tau.shape + (nchan,)), NP.empty(tau.shape + (nchan,))
        sc, ss = _phasor(df * tau)
        for k0 in range(0, nchan, R.TILE):
            ck, sk = _phasor(fq[k0] * tau)
            for k in range(k0, min(k0 + R.TILE, nchan)):
                cs[..., k], sn[..., k] = ck, sk
                p = sk * ss
                cn = _round(ck.astype(LD) * sc - p)
                sk = _round(ck.astype(LD) * ss + (sk * sc))
                ck = cn
    w = IK.full_weights(weights, nt, nbl, nchan)
    if kind == 'psf':
        wre, wim = NP.array(w, dtype=NP.float64), NP.zeros((nt, nbl, nchan))
    else:
        wre, wim = w * c['cube'].real, w * c['cube'].imag
    D = _round(NP.sum(wre[:, None].astype(LD) * cs - wim[:, None].astype(LD) * sn, axis=(0, 2)))
    W = NP.zeros(nchan)
    for tt in range(nt):
        for bb in range(nbl):
            W = W + w[tt, bb]
    if chan_avg:
        return NP.cumsum(D, axis=1)[:, -1] / NP.cumsum(W)[-1]
    return D / W


def ratio(got, ref, geo, freqs, route, chan_avg):
    """(the worst deviation in units of the scale, the worst in units of THE RULE's bound)"""
    want, scale = (ref.band_image, ref.band_scale) if chan_avg else (ref.image, ref.scale)
    dev = NP.abs(got - want) / scale
    bound = R.bound(geo, freqs, route, band=chan_avg)
    return float(dev.max()), float(NP.max(dev / (bound[0] if chan_avg else bound)))


# ---- the two routes ------------------------------------------------------------------------------------------------------------------

def test_the_two_routes_agree_on_every_set(geos):
    worst = 0.0
    for name, _, _ in SETS:
        c, geo = geos(name)
        for kind, weights in (('dirty', c['w_full']), ('psf', c['w_bl'])):
            ref = R.image(geo, c['cube'], weights, kind)
            gap = R.route_gap(c, weights, kind, ref, nsample=8)
            worst = max(worst, gap)
            assert gap <= R.ROUTE_GAP, (name, kind, gap)
    print('route gap over all sets: %.2e of the scale (bound %.0e)' % (worst, R.ROUTE_GAP))


# ---- exact properties ------------------------------------------------------------------------------------------------------------------

def test_zero_offset_antipode_and_exact_cycles(geos):
    c, geo = geos('edges x1000')
    assert NP.all(geo.d[0, 0] == 0.0) and all(v == 0 for v in geo.D[0, 0])
    assert NP.array_equal(geo.d[0, 1], [0.0, 0.0, -2.0]) and geo.D[0, 1, 2] == -2 << R.DIR_BITS and NP.sqrt(NP.sum(geo.d[0, 1] ** 2)) == 2.0
    for form in ('none', 'baseline', 'full'):
        w = R.weights_of(c, form)
        ref = R.image(geo, c['cube'], w, 'dirty')
        wl = IK.full_weights(w, 1, c['nbl'], c['nchan']).astype(LD)
        plain = NP.sum(wl * c['cube'].real.astype(LD), axis=(0, 1))                                  # D = sum w Re V at d = 0, to the order
        assert NP.all(NP.abs(ref.D_ld[0] - plain) <= c['nbl'] * NP.finfo(LD).eps * ref.num_ld)       # of the longdouble sum alone
        assert NP.all(R.image(geo, None, w, 'psf').image_ld[0] == 1)                                  # and the PSF is 1
    c, geo = geos('whole and half cycles')
    sign = NP.array([1, 1, 1, 1, -1])
    assert NP.all(geo.cos[0, 0, :, 0] == sign) and NP.all(geo.cos[0, 1, :, 0] == sign) and NP.all(geo.cos[0, 2] == 1) and NP.all(geo.sin == 0)
    ref = R.image(geo, c['cube'], c['w_bl'], 'dirty')
    assert NP.array_equal(ref.D_ld[0, 0], NP.sum(c['w_bl'].astype(LD) * c['cube'][0, :, 0].real.astype(LD) * sign))


def test_negated_baselines_image_the_conjugate_cube(geos):
    for name in ('%s x1000 sphere' % (BIG,), 'edges x1', 'whole and half cycles'):
        c, geo = geos(name)
        neg = R.geometry(c['unitvec'], c['rot'], c['beta'], c['pc'], -c['baselines'], c['freqs'])
        assert NP.array_equal(neg.cos, geo.cos) and NP.array_equal(neg.sin, -geo.sin)
        a = R.image(neg, c['cube'], c['w_full'], 'dirty')
        b = R.image(geo, c['cube'].conj(), c['w_full'], 'dirty')
        assert NP.array_equal(a.D_ld, b.D_ld) and NP.array_equal(a.image, b.image)


def test_a_point_source_images_to_its_flux(geos):
    c, geo = geos('%s x1000 sphere' % (BIG,))
    S, q = 3.25, 7
    v = S * (geo.cos[:, q].astype(NP.float64) - 1j * geo.sin[:, q].astype(NP.float64))      # S conj E of pixel q, rounded to complex128
    ref = R.image(geo, v, c['w_full'], 'dirty')
    assert NP.all(NP.abs(ref.image[q] - S) <= 4 * R.U * S) and NP.all(NP.abs(ref.image) <= S * (1 + 4 * R.U))
    assert NP.all(NP.abs(ref.scale - S) <= 4 * R.U * S)
    assert NP.all(NP.abs(ref.band_image[q] - S) <= 4 * R.U * S)


def test_grid_gap_and_the_bounds(geos):
    c, geo = geos('edge grid x1000')
    assert R.grid_gap(150e6 + 1e5 * NP.arange(70)) == 0.0 and R.grid_gap([150e6]) == 0.0
    assert R.grid_gap(c['freqs']) == 3 * NP.spacing(150e6)
    f = 150e6 + 1e5 * NP.arange(70)
    f[33] += 2e-8                                                          # off the line by one channel of the second tile alone
    assert R.grid_gap(f) == f[33] - (150e6 + 33e5)
    f[32] += 2e-8                                                          # the seed of that tile moves with it: the gap is the tile's own
    assert R.grid_gap(f) == f[32] - (150e6 + 32e5)
    for route in ('direct', 'stepped'):
        b, ub = R.bound(geo, c['freqs'], route), R.update_bound(geo, c['freqs'], route)
        assert NP.all(b > R.BAR) and NP.all(ub > b) and NP.all(ub < 2.2 * b)
        assert R.bound(geo, c['freqs'], route, band=True)[0] == b.max()
    assert NP.all(R.bound(geo, c['freqs'], 'stepped') > R.bound(geo, c['freqs'], 'direct'))
    assert NP.allclose(geo.tau_max * c['freqs'], geo.Np, rtol=1e-15)


def test_the_lines_the_rule_cites_say_what_it_counts():
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'prisim_amd')
    cited = {'csrc_imaging/imaging_kernels.h': ((29, 'kInvC = 1.0 / 299792458.0'), (45, 'u[0] + fr.beta[0]'), (46, 'fr.rot[0] * t0 + fr.rot[1] * t1) + fr.rot[2] * t2'),
                                                (49, 'sqrt((v0 * v0 + v1 * v1) + v2 * v2)'), (50, 'v0 / nrm'), (52, 'l - fr.pc[0]'), (73, 'x - rint(x)'),
                                                (74, 'sincospi(2.0 * r'), (90, '(sh_b[r * 3] * d.x + sh_b[r * 3 + 1] * d.y) + sh_b[r * 3 + 2] * d.z'),
                                                (94, 'f0 * tau'), (95, 'df * tau'), (109, 'sh_f[k] * tau'), (147, '* kInvC')),
             'csrc_imaging/clean_update.h': ((73, '((bl[0] * kInvC) * dq.x + (bl[1] * kInvC) * dq.y) + (bl[2] * kInvC) * dq.z'), (75, 'sh_f[c] * tau'),
                                             (77, 'wa * cq, -(wa * sq)')),
             'csrc_addon/imaging_plan.h': ((30, '(f[n - 1] - f[0]) / (double)(n - 1)'),)}
    for name, lines in cited.items():
        src = open(os.path.join(root, name)).read().splitlines()
        for number, text in lines:
            assert text in src[number - 1], (name, number, src[number - 1])
    mk = open(os.path.join(root, 'csrc', 'Makefile')).read()
    assert '-ffp-contract=off' in mk                                    # the count of the dot product stands on it


# ---- the checker's floor ---------------------------------------------------------------------------------------------------------------

def test_the_checkers_floor_per_decade_and_the_law_of_the_narrow_field(geos):
    for field in ('sphere', 'narrow'):
        for scale in R.SCALES:
            c, geo = geos('%s x%d %s' % (BIG, scale, field))
            ref = R.image(geo, c['cube'], c['w_full'], 'dirty')
            args = (c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'])
            chk = IK.dirty_image(*args, cube=c['cube'], weights=c['w_full'], aberr_beta=c['beta'])
            stp = IK.stepped_image(*args, c['cube'], weights=c['w_full'], aberr_beta=c['beta'])
            assert NP.allclose(chk['scale'], ref.scale, rtol=1e-14, atol=0)
            dev = {'dirty_image': float(NP.max(NP.abs(chk['image'] - ref.image) / ref.scale)),
                   'stepped_image': float(NP.max(NP.abs(stp - ref.image) / ref.scale))}
            for route in ('direct', 'stepped'):
                dev[route] = ratio(device_image(c, c['w_full'], 'dirty', route, False), ref, geo, c['freqs'], route, False)[0]
            unit = 2.0 * NP.pi * R.U * geo.Nb.max()
            print('%-6s x%-4d  dirty_image %.1e | stepped_image %.1e | restatement %.1e / %.1e   (N_b %.2e, N\' %.2e; restatement %.2f / %.2f of '
                  '2 pi u N_b)' % (field, scale, dev['dirty_image'], dev['stepped_image'], dev['direct'], dev['stepped'], geo.Nb.max(),
                                   geo.Np.max(), dev['direct'] / unit, dev['stepped'] / unit))
            for what in ('dirty_image', 'stepped_image'):
                if scale in R.CHECKER_KEEPS:
                    assert dev[what] <= R.BAR, (field, scale, what, dev[what])
                else:
                    assert scale in R.CHECKER_LOSES and dev[what] > R.BAR, (field, scale, what, dev[what])
                assert dev[what] <= float(R.bound(geo, c['freqs'], 'direct').max())      # the checker states the same chain, and more
            if field == 'narrow':
                assert geo.Nb.max() > 50.0 * geo.Np.max()
                if scale in R.SCALES[-2:]:
                    # the error follows N_b: it is past everything the sky-sum's rule (the phase roundings on N' alone) would allow
                    sky_rule = 2.0 * NP.pi * R.U * R.R_PH_DIRECT * geo.Np.max()
                    for what in ('dirty_image', 'direct', 'stepped'):
                        assert dev[what] > sky_rule, (scale, what, dev[what], sky_rule)


# ---- the device's statement passes, wrong ones fail ------------------------------------------------------------------------------------

def test_the_restatement_of_the_device_passes_the_rule_on_every_set(geos):
    worst = {'direct': 0.0, 'stepped': 0.0}
    for name, _, uniform in SETS:
        c, geo = geos(name)
        for kind in ('dirty', 'psf'):
            ref = R.image(geo, c['cube'], c['w_full'], kind)
            for route in (('direct', 'stepped') if uniform else ('direct',)):
                for chan_avg in (False, True):
                    got = device_image(c, c['w_full'], kind, route, chan_avg)
                    dev, rel = ratio(got, ref, geo, c['freqs'], route, chan_avg)
                    assert NP.all(NP.isfinite(got)) and rel <= 1.0, (name, kind, route, chan_avg, dev, rel)
                    worst[route] = max(worst[route], rel)
    print('restatement, the worst deviation over the bound: direct %.3f, stepped %.3f' % (worst['direct'], worst['stepped']))


@pytest.mark.parametrize('variant', ['1/c in float32', 'no normalisation', 'd.z dropped'])
def test_a_wrong_statement_fails_the_rule(geos, variant):
    seen = {}
    for name in ('%s x1 sphere' % (BIG,), '%s x1000 sphere' % (BIG,), '%s x1 narrow' % (BIG,), '%s x1000 narrow' % (BIG,)):
        c, geo = geos(name)
        ref = R.image(geo, c['cube'], c['w_full'], 'dirty')
        seen[name] = min(ratio(device_image(c, c['w_full'], 'dirty', route, False, variant=variant), ref, geo, c['freqs'], route, False)[1]
                         for route in ('direct', 'stepped'))
    print('%s: deviation over the bound %s' % (variant, ', '.join('%s %.2e' % (n, v) for n, v in seen.items())))
    assert max(seen.values()) > 1.0
    if variant == 'd.z dropped':
        assert seen['%s x1 narrow' % (BIG,)] > 1.0 and seen['%s x1000 narrow' % (BIG,)] > 1.0
