"""GPU (-m gpu): the mosaic (k_mos_sum of prisim_amd/csrc_imaging/mosaic_kernels.h, its fp32 route and prisim_dirty_image_f32), the
CLEAN of the mosaic (mosclean_kernels.h, clean_update.h) and the Cotton-Schwab CLEANs with their minor-cycle beam P (cycle_kernels.h,
csclean.hip, moscs.hip) through the C-ABI against the 40-digit reference of tests/mosaic_reference.py, from 300 m to 2400 km
baselines, under THE RULES stated in that module: every element of every output, finite wherever it is not masked, the NaN positions
the reference's, nothing excused.

Shapes (nbl, nchan, npix, nt): (1, 1, 1, 1); (33, 33, 65, 2): a second LDS pass of one row, a second channel tile of one channel, a
ragged block, two frames; (3, 65, 257, 1): three tiles, a second block of one pixel; the lattice (33, 33, 5, 13, 2), five rows of
thirteen pixels, as it is (scales 1 and 1000) and with both half-widths divided by the scale (1000 and 8000), where b . delta in
wavelengths stays what it is at 300 m while the whole baseline grows a thousandfold and more.

The replays of the CLEANs follow the device's lists on the reference's phasors E_ref, beams A_ref and lattice beam P_ref with the counted
bounds; that the reference's own Cotton-Schwab run is not vacuous is asserted on the reference's run, never on the device's."""
import os
import sys
import time

import numpy as NP
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import csclean_checker as CS  # noqa: E402
import imaging_reference as R  # noqa: E402
import imclean_checker as CK  # noqa: E402
import mosaic_cases as MC  # noqa: E402
import mosaic_checker as MK  # noqa: E402
import mosaic_reference as M  # noqa: E402
import mosclean_cases as QC  # noqa: E402
import mosclean_checker as QK  # noqa: E402
import moscs_cases as XC  # noqa: E402
import moscs_checker as XK  # noqa: E402

pytestmark = pytest.mark.gpu
SHAPE = (33, 33, 65, 2)
BEAMS = ('gaussian', 'airy', 'dipole_ground')
FORMS = ('none', 'baseline', 'full')
SETTING_A = dict(gain=0.3, maxiter=25, threshold=0.0, threshold_relative=False, cycle_depth=0.5, cycle_niter=4, max_major=10)   # test_gpu_csclean.py
_WORST = {}


def ident(v):
    return 'x'.join(str(x) for x in v) if isinstance(v, tuple) else str(v)


@pytest.fixture(scope='module', autouse=True)
def wall_time():
    t0 = time.time()
    yield
    print('\ntests/test_gpu_mosaic_reference.py: %.1f s wall; the largest share of each bound per decade:' % (time.time() - t0))
    for key in sorted(_WORST):
        print('    %-28s x%-5d %.3f' % (key[0], key[1], _WORST[key]))


def note(what, scale, share):
    _WORST[(what, scale)] = max(_WORST.get((what, scale), 0.0), share)


def share_of(dev, tol):
    """The largest dev / tol; an element with no tolerance must have no deviation."""
    with NP.errstate(invalid='ignore', divide='ignore'):
        return float(NP.max(NP.where(tol > 0.0, dev / tol, NP.where(dev > 0.0, NP.inf, 0.0))))


def call(ctx, c, name, weights=None, **kw):
    kind, dia, ext, _ = MC.beam_setups(c['rot'].shape[0])[name]
    return ctx.mosaic_image(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], kind, dia, ext=ext, cube=c['cube'], weights=weights,
                            aberr_beta=c['beta'], **kw)


def held(ctx, c, geo, ref, name, weights, route, scale, label, precision='double'):
    """One beam, both chan_avg, under THE RULES: num, den, wsum, the quotient and the mask."""
    nt, npix, nbl, nchan = geo.cos.shape
    tol_n, tol_q = M.tolerances(ref, M.snapshot_bounds(geo, c['baselines'], c['freqs'], route))
    if precision == 'single':
        tol_n = M.F32_BAR * ref.scale_N + M.BEAM_BAR * ref.absV.sum(axis=0)[None, :]
    for chan_avg in (False, True):
        mosaic, num, den, wsum, st = call(ctx, c, name, weights=weights, chan_avg=chan_avg, route=route, pbmin=M.PBMIN, precision=precision)
        assert st['route'] == route and st['precision'] == precision and st['terms'] == npix * nbl * nchan * nt
        assert num.shape == den.shape == (npix, nchan) and NP.all(NP.isfinite(num)) and NP.all(NP.isfinite(den)) and NP.all(NP.isfinite(wsum))
        sn, sq = share_of(NP.abs(num - ref.num), tol_n), share_of(NP.abs(den - ref.den), tol_q)
        print('%s %s %s chan_avg=%d %s: num %.3f of tol_N, den %.1e of tol_Q' % (label, name, precision, chan_avg, route, sn, sq))
        assert sn <= 1.0 and sq <= 1.0, (label, name, precision, chan_avg, route, sn, sq)
        note('mosaic num' if precision == 'double' else 'mosaic num fp32', scale, sn)
        note('mosaic den', scale, sq)
        assert NP.all(NP.abs(wsum - ref.wsum) <= nt * nbl * R.U * ref.wsum)
        want_mosaic, want_eff = MK.quotient(num, den, wsum, M.PBMIN, chan_avg)
        assert mosaic.shape == want_mosaic.shape and NP.array_equal(mosaic, want_mosaic, equal_nan=True), label
        assert NP.array_equal(st['pb_eff'], want_eff, equal_nan=True), label
        masked = M.mask_ratio(ref, M.PBMIN, chan_avg) < 1.0
        assert NP.array_equal(NP.isnan(mosaic), masked), (label, 'the NaN positions are the reference\'s')
        assert NP.all(NP.isfinite(mosaic[~masked])) and NP.all(NP.isfinite(st['pb_eff']))


# ---- the mosaic ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape, scale, field', [cfg for cfg in M.MOSAIC_CONFIGS if cfg[0] != SHAPE or cfg[1] != 10], ids=ident)
def test_s1_mosaic_every_element_under_the_rules(ctx, shape, scale, field):
    c, geo = R.case(shape, scale, field), R.geometry_of(shape, scale, field)
    forms = FORMS if (shape, scale) == (SHAPE, 1000) else ('full',)
    for name in BEAMS:
        for form in forms:
            ref = M.mosaic_of(shape, scale, field, name, form)
            for route in ('direct', 'stepped'):
                held(ctx, c, geo, ref, name, R.weights_of(c, form), route, scale, '%s x%d %s weights=%s' % (shape, scale, field, form))


def test_s1_a_flipped_snapshot_and_pixels_below_the_horizon(ctx):
    """mosaic_cases.up_case at 300 km: snapshot 1 turns the sky upside down, the last 20 pixels are down in the other."""
    c = M.scaled(MC.up_case(33, 33, 65, 2, flip=(1,), down=20), 1000)
    geo = R.geometry_case(c)
    up, margin = M.horizon(c['unitvec'], c['rot'], c['beta'], c['pc'])
    assert margin > 0.04 and NP.array_equal(up[0], NP.arange(65) < 45) and NP.array_equal(up[1], ~up[0])
    for name in ('gaussian', 'dipole_ground'):
        ref = M.mosaic(geo, M.beams(geo, up, M.SPECS[name], c['freqs']), c['cube'], c['w_full'])
        for route in ('direct', 'stepped'):
            held(ctx, c, geo, ref, name, c['w_full'], route, 1000, 'flipped x1000')


# ---- the fp32 entries -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape, scale, field', [cfg for cfg in M.MOSAIC_CONFIGS if cfg[1] in (1000, 8000)], ids=ident)
def test_s2_fp32_entries_at_long_baselines(ctx, shape, scale, field):
    """prisim_mosaic_image_f32 and prisim_dirty_image_f32 against the reference under their own bar, 5e-6 of the natural scale."""
    c, geo = R.case(shape, scale, field), R.geometry_of(shape, scale, field)
    for name in BEAMS:
        held(ctx, c, geo, M.mosaic_of(shape, scale, field, name), name, c['w_full'], 'stepped', scale, '%s x%d %s' % (shape, scale, field), precision='single')
    for kind in ('dirty', 'psf'):
        ref = R.image_of(shape, scale, field, True, 'full', kind)
        for chan_avg in (False, True):
            img, wsum, st = ctx.dirty_image(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], cube=c['cube'], weights=c['w_full'],
                                            aberr_beta=c['beta'], kind=kind, chan_avg=chan_avg, precision='single')
            want, scl = (ref.band_image, ref.band_scale) if chan_avg else (ref.image, ref.scale)
            assert st['precision'] == 'single' and img.shape == want.shape and NP.all(NP.isfinite(img))
            dev = float(NP.max(NP.abs(img - want) / scl)) / M.F32_BAR
            print('%s x%d %s fp32 %s chan_avg=%d: %.3f of 5e-6 of the scale' % (shape, scale, field, kind, chan_avg, dev))
            assert dev <= 1.0
            note('dirty image fp32', scale, dev)


# ---- CLEAN of the mosaic ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('scale', (1, 100, 1000, 8000))
def test_s3_clean_of_the_mosaic_replayed_on_the_reference(ctx, scale):
    """prisim_clean_mosaic on mosclean_cases.parity_case((33, 33, 65, 2)): gain 0.3, maxiter 8, absolute threshold 0, a window on every
    second pixel; the replay of tests/mosclean_checker.py on E_ref and A_ref with the counted bounds of both chains."""
    c = M.scaled(QC.parity_case(SHAPE), scale)
    geo = R.geometry_case(c)
    up, margin = M.horizon(c['unitvec'], c['rot'], c['beta'], c['pc'])
    assert margin >= M.HORIZON_MARGIN
    window = NP.arange(65) % 2 == 0
    pbmin = 0.2                      # of these 65 directions the mask keeps 0.20 (Gaussian) and 0.38 (Airy), none within 0.13 of its rim
    for beam in ('gaussian', 'airy'):
        sh = M.shared(geo, M.beams(geo, up, M.SPECS[beam], c['freqs'], pointing=c['bpc']))
        for chan_avg in (False, True):
            pb = QC.problem(c, beam, weights=c['w_full'], chan_avg=chan_avg, window=window, share=sh, pbmin=pbmin)
            QC.assert_mask_keeps_and_cuts(pb)
            for route in ('direct', 'stepped'):
                got = ctx.clean_mosaic(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], QC.BEAMS[beam], QC.DISH, beam_pc_dircos=c['bpc'],
                                       cube=c['cube'], weights=c['w_full'], aberr_beta=c['beta'], chan_avg=chan_avg, pbmin=pbmin, gain=0.3,
                                       maxiter=8, threshold=0.0, threshold_relative=False, window=window, route=route)
                assert got['stats']['route'] == route and NP.all(got['ncomp'] == 8) and NP.all(NP.isfinite(got['num']))
                bound = (M.snapshot_bounds(geo, c['baselines'], c['freqs'], route), M.snapshot_bounds(geo, c['baselines'], c['freqs'], route, update=True))
                worst = QK.replay(pb, got, 0.3, 8, 0.0, False, bound=bound)
                print('clean of the mosaic x%d %s chan_avg=%d %s: %.3f of the tolerance' % (scale, beam, chan_avg, route, worst))
                assert worst <= 1.0
                note('clean_mosaic replay', scale, worst)


# ---- Cotton-Schwab --------------------------------------------------------------------------------------------------------------------------------
def same_bits(a, b, names):
    return all((a[n] is None) == (b[n] is None) and (a[n] is None or NP.array_equal(a[n], b[n], equal_nan=True)) for n in names)


def psf_held(psf, lat, c, route, chan_avg, label, scale):
    ny, nx = c['ny'], c['nx']
    assert psf.shape == lat.P.shape and NP.all(NP.isfinite(psf))
    assert NP.array_equal(psf, psf[:, ::-1, ::-1]) and NP.all(psf[:, ny - 1, nx - 1] == 1.0)          # even bit for bit, 1 at the centre
    bound = M.p_bound(lat, c['freqs'], route, band=chan_avg)
    dev = NP.abs(psf - lat.P).max(axis=(1, 2))
    worst = float(NP.max(dev / bound))
    print('%s chan_avg=%d %s: |P - P_ref| %.2e, %.3f of its rule (N_delta %.3g, N_b %.3g)' % (label, chan_avg, route, dev.max(), worst, lat.Nd.max(), lat.Nb.max()))
    assert worst <= 1.0
    note('P', scale, worst)
    return bound


@pytest.mark.parametrize('scale, shrink', M.LATTICE_CONFIGS, ids=ident)
def test_s4_cotton_schwab_on_the_reference(ctx, scale, shrink):
    c, geo = M.lattice_case(scale, shrink), M.lattice_geometry(scale, shrink)
    ny, nx = c['ny'], c['nx']
    E = geo.cos.astype(NP.float64) + 1j * geo.sin.astype(NP.float64)
    args = tuple(SETTING_A[n] for n in M.CS_ARGS)
    label = 'cs x%d lattice / %d' % (scale, shrink)
    for chan_avg in (False, True):
        lat = M.lattice_of(scale, shrink, 'full', chan_avg)
        pb = CK.Problem(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], c['cube'], weights=c['w_full'], aberr_beta=c['beta'],
                        chan_avg=chan_avg, E=E)
        own = CS.clean(pb, lat.P, ny, nx, *args)
        M.assert_not_vacuous(own)                                        # on the reference's run
        for route in ('direct', 'stepped'):
            runs = [ctx.clean_image_cs(c['unitvec'], (ny, nx), c['rot'], c['pc'], c['baselines'], c['freqs'], cube=c['cube'], weights=c['w_full'],
                                       aberr_beta=c['beta'], chan_avg=chan_avg, route=route, minor_route=minor, want_psf=True, want_vis=True,
                                       **SETTING_A) for minor in ('lds', 'global')]
            got = runs[0]
            assert got['stats']['route'] == route and [r['stats']['minor_route'] for r in runs] == ['lds', 'global']
            assert same_bits(runs[0], runs[1], [n for n in runs[0] if n != 'stats']), (label, 'the LDS and GLOBAL minor routes give the same bits')
            psf_held(got['psf'], lat, c, route, chan_avg, label, scale)
            assert NP.all(NP.isfinite(got['residual'])) and NP.all(NP.isfinite(got['vres'].view(NP.float64)))
            bound = (R.bound(geo, c['freqs'], route, band=chan_avg), R.update_bound(geo, c['freqs'], route, band=chan_avg))
            assert NP.all(M.p_bound(lat, c['freqs'], route, band=chan_avg) <= bound[1])
            worst = CS.replay(pb, lat.P, ny, nx, got, *args, bound=bound)
            print('%s chan_avg=%d %s: %d to %d cycles, %d to %d components, statuses %s, the replay at %.3f of its tolerance'
                  % (label, chan_avg, route, got['ncycles'].min(), got['ncycles'].max(), got['ncomp'].min(), got['ncomp'].max(),
                     sorted(set(got['status'].tolist())), worst))
            assert worst <= 1.0
            note('clean_image_cs replay', scale, worst)


@pytest.mark.parametrize('scale, shrink', M.LATTICE_CONFIGS, ids=ident)
def test_s5_cotton_schwab_of_the_mosaic_on_the_reference(ctx, scale, shrink):
    """prisim_clean_mosaic_cs with the 6 m dishes of tests/moscs_cases.py, under its SETTINGS['A'] (one cycle to maxiter on most channels)
    and under SETTING_A of tests/test_gpu_csclean.py, whose cap of four components a cycle makes the major cycles do the work."""
    c, geo = M.lattice_case(scale, shrink), M.lattice_geometry(scale, shrink)
    ny, nx = c['ny'], c['nx']
    up, margin = M.horizon(c['unitvec'], c['rot'], c['beta'], c['pc'])
    assert margin >= M.HORIZON_MARGIN
    bpc = M.lattice_pointing(geo, ny, nx)
    cc = dict(c, bpc=bpc, dish=6.0, pbmin=0.3)
    for beam in ('gaussian', 'airy'):
        sh = M.shared(geo, M.beams(geo, up, M.SPECS[beam + '6'], c['freqs'], pointing=bpc))
        for chan_avg in (False, True):
            lat = M.lattice_of(scale, shrink, 'full', chan_avg)
            pb = XC.problem(cc, beam, weights=c['w_full'], chan_avg=chan_avg, share=sh)
            assert pb.search.any(axis=0).all()
            for sname, kw in (("SETTINGS['A']", XC.SETTINGS['A']), ('SETTING_A', SETTING_A)):
                label = 'moscs x%d lattice / %d %s %s' % (scale, shrink, sname, beam)
                own = XK.clean(pb, lat.P, ny, nx, *XC.replay_args(kw))                # the reference's run
                assert NP.all(own['ncomp'] >= 8), own['ncomp']
                if kw is SETTING_A:
                    M.assert_not_vacuous(own)
                for route in ('direct', 'stepped'):
                    runs = [ctx.clean_mosaic_cs(c['unitvec'], (ny, nx), c['rot'], c['pc'], c['baselines'], c['freqs'], XC.BEAMS[beam], 6.0,
                                                beam_pc_dircos=bpc, cube=c['cube'], weights=c['w_full'], aberr_beta=c['beta'], chan_avg=chan_avg,
                                                pbmin=0.3, route=route, minor_route=minor, want_psf=True, want_vis=True, **kw) for minor in ('lds', 'global')]
                    got = runs[0]
                    assert got['stats']['route'] == route
                    assert same_bits(runs[0], runs[1], [n for n in runs[0] if n != 'stats']), (label, 'the LDS and GLOBAL minor routes give the same bits')
                    pbound = psf_held(got['psf'], lat, c, route, chan_avg, label, scale)
                    bound = (M.snapshot_bounds(geo, c['baselines'], c['freqs'], route), M.snapshot_bounds(geo, c['baselines'], c['freqs'], route, update=True))
                    worst = XK.replay(pb, lat.P, ny, nx, got, *XC.replay_args(kw), bound=bound, psf_bound=pbound)
                    print('%s chan_avg=%d %s: %d to %d cycles, %d to %d components, statuses %s, the replay at %.3f of its tolerance'
                          % (label, chan_avg, route, got['ncycles'].min(), got['ncycles'].max(), got['ncomp'].min(), got['ncomp'].max(),
                             sorted(set(got['status'].tolist())), worst))
                    assert worst <= 1.0
                    note('clean_mosaic_cs replay', scale, worst)
