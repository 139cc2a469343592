"""CPU: tests/mosaic_reference.py held to itself and to the code it judges, before any device run.

  * its two routes agree within imaging_reference.ROUTE_GAP of the scale on a seeded sub-sample of every case set the GPU tests use,
    for N, Q and P;
  * the floor of the numpy checkers per decade (mosaic_checker for N, csclean_checker.beam for P), asserted both ways;
  * a float64 restatement of the device's chain, operation by operation from the lines THE RULES cite, passes the counted rules at
    every decade, and five deliberately wrong restatements fail them;
  * P loses accuracy on N_delta and not on N_b, asserted both ways;
  * the input conditions of the GPU tests, on the reference alone, at every scale;
  * the reference-side Cotton-Schwab runs are not vacuous.
Measured 2026-10-21 on x86-64: the figures this file prints are recorded in the docstring of tests/mosaic_reference.py."""
import os
import sys
import types

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
import skyvis_reference as SR  # noqa: E402

SHAPE = (33, 33, 65, 2)
K_INV_C = 1.0 / 299792458.0
BEAMS = ('gaussian', 'airy', 'dipole_ground')
SETTING_A = dict(gain=0.3, maxiter=25, threshold=0.0, threshold_relative=False, cycle_depth=0.5, cycle_niter=4, max_major=10)


# ---- the float64 restatement of the device's chain ----------------------------------------------------------------------------------------
def restated_directions(c):
    """k_img_dirs, imaging_kernels.h:45-52: (s, d), (nt, npix, 3)."""
    u, rot, beta, pc = c['unitvec'], c['rot'], c['beta'], c['pc']
    t = u[None, :, :] + beta[:, None, :]
    v = [(rot[:, None, i, 0] * t[..., 0] + rot[:, None, i, 1] * t[..., 1]) + rot[:, None, i, 2] * t[..., 2] for i in range(3)]
    nrm = NP.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    s = NP.stack([x / nrm for x in v], axis=-1)
    return s, s - pc[:, None, :]


def _phasor(x):
    r = 2.0 * (x - NP.rint(x))                                                        # cycles_phasor, imaging_kernels.h:73-74
    return NP.cos(NP.pi * r), NP.sin(NP.pi * r)


def restated_phasors(d, baselines, freqs, route='direct'):
    """img_rows (imaging_kernels.h:90; DIRECT :109; STEPPED :94-95 and the recurrence :101-103, a seed per 32-channel tile) on the offsets d
    (nt, n, 3): (cos, sin) (nt, n, nbl, nchan)."""
    b = baselines * K_INV_C                                                           # imaging_kernels.h:147
    tau = (b[None, None, :, 0] * d[:, :, None, 0] + b[None, None, :, 1] * d[:, :, None, 1]) + b[None, None, :, 2] * d[:, :, None, 2]
    if route == 'direct':
        return _phasor(freqs[None, None, None, :] * tau[..., None])
    cos, sin = NP.empty(tau.shape + (freqs.size,)), NP.empty(tau.shape + (freqs.size,))
    sc, ss = _phasor(R.grid_df(freqs) * tau)
    for k0 in range(0, freqs.size, R.TILE):
        c, s = _phasor(freqs[k0] * tau)
        for k in range(k0, min(k0 + R.TILE, freqs.size)):
            cos[..., k], sin[..., k] = c, s
            c, s = c * sc - s * ss, c * ss + s * sc
    return cos, sin


def restated_mosaic(c, A_ref, weights, wrong=None, route='direct'):
    """k_mos_sum (mosaic_kernels.h:68-82) in float64: (N, Q).  The beam values are the reference's rounded to doubles (the device's are
    held to 1e-12 of them elsewhere); the horizon is the restatement's own s_z >= 0."""
    nt, nbl, nchan = c['cube'].shape
    w = NP.ones((nt, nbl, nchan)) if weights is None else NP.broadcast_to(weights[None, :, None] if weights.ndim == 1 else weights, (nt, nbl, nchan))
    s, d = restated_directions(c)
    cos, sin = restated_phasors(d, c['baselines'], c['freqs'], route)
    wv = w * c['cube']
    D = NP.einsum('tbk,tpbk->tpk', wv.real, cos) - NP.einsum('tbk,tpbk->tpk', wv.imag, sin)
    Wt = w.sum(axis=1)
    A = NP.where((s[..., 2] >= 0.0)[..., None], A_ref, 0.0)
    if wrong == 'no horizon mask':
        A = M.beams(types.SimpleNamespace(s=s), NP.ones(s.shape[:2], dtype=bool), wrong_spec(c), c['freqs']).astype(NP.float64)
    N, Q = NP.zeros(D.shape[1:]), NP.zeros(D.shape[1:])
    for t in range(nt):
        N = A[t] * D[t] + N
        Q = (A[t] if wrong == 'A to the first power in Q' else A[t] * A[t]) * Wt[t][None, :] + Q
    return N, Q


def wrong_spec(c):
    return M.SPECS['dipole_ground']                          # the one beam that is not zero below the horizon by itself


def restated_P(c, weights, chan_avg, wrong=None, route='direct'):
    """cycle_kernels.h:283-284 (the steps), :70-74 (the offsets), the PSF of img_rows on them, the mirror of k_csclean_mirror."""
    ny, nx = c['ny'], c['nx']
    u = c['unitvec'].reshape(ny, nx, 3)
    rho = (u[ny - 1, nx // 2] - u[0, nx // 2]) / float(ny if wrong == 'rho over ny' else ny - 1)
    kappa = (u[ny // 2, nx - 1] - u[ny // 2, 0]) / float(nx - 1)
    hp = NP.array(M.half_plane(ny, nx), dtype=NP.float64)
    t = hp[:, :1] * rho[None, :] + hp[:, 1:] * kappa[None, :]                         # (h, 3)
    rot = c['rot'] if wrong != 'delta not rotated' else NP.broadcast_to(NP.eye(3), c['rot'].shape)
    dd = NP.stack([(rot[:, None, i, 0] * t[None, :, 0] + rot[:, None, i, 1] * t[None, :, 1]) + rot[:, None, i, 2] * t[None, :, 2] for i in range(3)],
                  axis=-1)
    cos, _ = restated_phasors(dd, c['baselines'], c['freqs'], route)
    nt, nbl, nchan = c['cube'].shape
    w = NP.ones((nt, nbl, nchan)) if weights is None else NP.broadcast_to(weights[None, :, None] if weights.ndim == 1 else weights, (nt, nbl, nchan))
    num = NP.einsum('tbk,thbk->kh', w, cos)
    W = w.sum(axis=(0, 1))
    half = num.sum(axis=0, keepdims=True) / W.sum() if chan_avg else num / W[:, None]
    P = NP.empty((half.shape[0], 2 * ny - 1, 2 * nx - 1))
    at = {o: h for h, o in enumerate(M.half_plane(ny, nx))}
    for (di, dj), h in at.items():
        P[:, ny - 1 + di, nx - 1 + dj] = half[:, h]
        P[:, ny - 1 - di, nx - 1 - dj] = half[:, at[(di, -dj)] if wrong == 'mirror at (di, -dj)' and di > 0 else h]
    return P


def share(dev, tol):
    """The largest dev / tol; an element with no tolerance must have no deviation."""
    with NP.errstate(invalid='ignore', divide='ignore'):
        return float(NP.max(NP.where(tol > 0.0, dev / tol, NP.where(dev > 0.0, NP.inf, 0.0))))


# ---- the two routes -----------------------------------------------------------------------------------------------------------------------
def test_the_two_routes_agree_on_every_case_set():
    worst = {'N': 0.0, 'Q': 0.0, 'P': 0.0}
    rounding = 0.0
    for shape, scale, field in M.MOSAIC_CONFIGS:
        c = R.case(shape, scale, field)
        nbl, nchan, npix, nt = shape
        names = BEAMS if shape == SHAPE and scale in (1, 1000) else ('airy',)
        for name in names:
            ref = M.mosaic_of(shape, scale, field, name)
            outs = M.sample((npix, nchan), 6 if shape == SHAPE else 3, seed=scale)
            if name != 'dipole_ground' and scale == 1:                                  # what rounding the directions is worth to a beam value
                for (p, k), (_, _, beam) in zip(outs, M.mosaic_terms_mp(c, M.SPECS[name], c['w_full'], outs, unrounded_beam=True)):
                    rounding = max(rounding, max(float(abs(SR.ld_to_mp(M.LD(ref.A[t, p, k])) - a)) - 0.5 * NP.spacing(ref.A[t, p, k]) for t, a in enumerate(beam)))
            for (p, k), (n, q, _) in zip(outs, M.mosaic_terms_mp(c, M.SPECS[name], c['w_full'], outs)):
                sn = SR.ld_to_mp(M.LD(ref.scale_N[p, k]) + M.LD(1e-12) * ref.absV[:, k].sum())
                sq = SR.ld_to_mp(M.LD(ref.wt[:, k].sum()))
                worst['N'] = max(worst['N'], float(abs(SR.ld_to_mp(ref.num_ld[p, k]) - n) / sn))
                worst['Q'] = max(worst['Q'], float(abs(SR.ld_to_mp(ref.den_ld[p, k]) - q) / sq))
    # the flipped case, the case of the CLEAN of the mosaic with its moving pointing, the lattice through the 6 m dishes
    lc, lg = M.lattice_case(1000, 1000), M.lattice_geometry(1000, 1000)
    for c, geo, names, pointing in ((M.scaled(MC.up_case(33, 33, 65, 2, flip=(1,), down=20), 1000), None, ('gaussian', 'dipole_ground'), None),
                                    (M.scaled(QC.parity_case(SHAPE), 1000), None, ('gaussian', 'airy'), 'bpc'),
                                    (lc, lg, ('gaussian6', 'airy6'), M.lattice_pointing(lg, lc['ny'], lc['nx']))):
        geo = R.geometry_case(c) if geo is None else geo
        pointing = c['bpc'] if isinstance(pointing, str) else pointing
        up, _ = M.horizon(c['unitvec'], c['rot'], c['beta'], c['pc'])
        for name in names:
            ref = M.mosaic(geo, M.beams(geo, up, M.SPECS[name], c['freqs'], pointing=pointing), c['cube'], c['w_full'])
            outs = M.sample(ref.num.shape, 4, seed=3)
            if name != 'dipole_ground':
                for (p, k), (_, _, beam) in zip(outs, M.mosaic_terms_mp(c, M.SPECS[name], c['w_full'], outs, unrounded_beam=True, pointing=pointing)):
                    rounding = max(rounding, max(float(abs(SR.ld_to_mp(M.LD(ref.A[t, p, k])) - a)) - 0.5 * NP.spacing(ref.A[t, p, k]) for t, a in enumerate(beam)))
            for (p, k), (n, q, _) in zip(outs, M.mosaic_terms_mp(c, M.SPECS[name], c['w_full'], outs, pointing=pointing)):
                sn = SR.ld_to_mp(M.LD(ref.scale_N[p, k]) + M.LD(1e-12) * ref.absV[:, k].sum())
                worst['N'] = max(worst['N'], float(abs(SR.ld_to_mp(ref.num_ld[p, k]) - n) / sn))
                worst['Q'] = max(worst['Q'], float(abs(SR.ld_to_mp(ref.den_ld[p, k]) - q) / SR.ld_to_mp(M.LD(ref.wt[:, k].sum()))))
    for scale, shrink in M.LATTICE_CONFIGS:
        c = M.lattice_case(scale, shrink)
        for chan_avg in (False, True):
            lat = M.lattice_of(scale, shrink, 'full', chan_avg)
            outs = M.sample(lat.P.shape, 3 if chan_avg else 8, seed=scale)
            want = M.lattice_terms_mp(c['unitvec'], c['rot'], c['baselines'], c['freqs'], c['ny'], c['nx'], c['w_full'], chan_avg, outs)
            worst['P'] = max(worst['P'], max(float(abs(SR.ld_to_mp(lat.P_ld[o]) - x)) for o, x in zip(outs, want)))
    print('route gap: N %.1e of sum_t A sum w|V| + 1e-12 sum w|V|, Q %.1e of Wtot, P %.1e' % (worst['N'], worst['Q'], worst['P']))
    print('the beams at unrounded directions: within %.1e of A_ref (less the rounding of A_ref to a double)' % rounding)
    assert max(worst.values()) <= M.ROUTE_GAP, worst
    assert rounding <= 1e-15


def test_the_lines_the_rules_cite_say_what_they_count():
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'prisim_amd', 'csrc_imaging')
    cited = {'cycle_kernels.h': ((71, 'di * L.rho[0] + dj * L.kappa[0]'), (73, '(fr.rot[0] * t0 + fr.rot[1] * t1) + fr.rot[2] * t2'),
                                 (74, '(fr.rot[6] * t0 + fr.rot[7] * t1) + fr.rot[8] * t2'), (84, 'f >= f0 ? f - f0 : f0 - f'),
                                 (255, 'M.bl[b * 3] * kInvC'), (263, 'point_phasor(b0, b1, b2, ddt[q], f, c, s)'),
                                 (283, '- u[(nx / 2) * 3 + i]) / (double)(ny - 1)'), (284, '- u[((ny / 2) * nx) * 3 + i]) / (double)(nx - 1)')),
             'mosaic_kernels.h': ((29, 's += row ? row[b * W.sb] : 1.0'), (68, 'img_tile_pass<STEPPED, false>(t, P.dd[pl]'), (75, 'P.s4[pl].z >= 0.0'),
                                  (81, 'fma(A, acc[k], t ? P.N[at + k] : 0.0)'), (82, 'fma(A * A, P.wt[k0 + k], t ? P.Q[at + k] : 0.0)')),
             'clean_update.h': ((89, 'my_a * P.A[(t * P.npix + sh_q[tid]) * P.nchan + k0 + tid]'), (96, 'fma(-Ap[k], acc[k], out[k])')),
             'imaging_kernels.h': ((79, '(b0 * d.x + b1 * d.y) + b2 * d.z'), (80, 'cycles_phasor(f * tau, c, s)'))}
    for name, lines in cited.items():
        src = open(os.path.join(root, name)).read().splitlines()
        for number, text in lines:
            assert text in src[number - 1], (name, number, src[number - 1])
    assert M.R_OFF == 2 + 1 + 1 + 3 and M.R_PH_P == R.R_PH_TAU - 1 + 1 == 6


# ---- the checkers' floor per decade -------------------------------------------------------------------------------------------------------
def test_the_floor_of_mosaic_checker_per_decade():
    """Worst |mosaic_checker N - N_ref| over its own bound_num (1e-11 sum_t A sum w|V| + 1e-12 sum w|V|), (33, 33, 65, 2), sphere | narrow,
    Airy 2 m, w_full; measured 2026-10-21 on x86-64:
        300 m 0.0022 | 0.0020    3 km 0.023 | 0.018    30 km 0.29 | 0.22    300 km 2.3 | 2.1    2400 km 17 | 13
    inside the bar up to the 30 km decade, outside it from the 300 km decade on, as imaging_checker itself (CHECKER_KEEPS / _LOSES)."""
    setup = MC.beam_setups(2)['airy'][3]
    for field in ('sphere', 'narrow'):
        for scale in M.SCALES:
            c = R.case(SHAPE, scale, field)
            ref = M.mosaic_of(SHAPE, scale, field, 'airy')
            chk = MK.mosaic(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], c['cube'], setup, weights=c['w_full'], aberr_beta=c['beta'])
            assert NP.max(NP.abs(chk['A'] - ref.A)) <= 1e-13                            # two independent beams, three orders inside 1e-12
            bar = R.BAR * ref.scale_N + M.BEAM_BAR * ref.absV.sum(axis=0)[None, :]
            floor, q = share(NP.abs(chk['num'] - ref.num), bar), share(NP.abs(chk['den'] - ref.den), M.tolerances(ref, M.snapshot_bounds(
                R.geometry_of(SHAPE, scale, field), c['baselines'], c['freqs'], 'direct'))[1])
            print('mosaic_checker %s x%d: N %.3g of its bar, Q %.3g of tol_Q' % (field, scale, floor, q))
            assert q <= 1.0
            assert (floor <= 1.0) if scale in M.CHECKER_KEEPS else (floor > 1.0), (field, scale, floor)


P_CHECKER_KEEPS, P_CHECKER_LOSES = (1, 10), (1000, 8000)


def test_the_floor_of_the_checkers_beam_per_decade():
    """Worst |csclean_checker.beam - P_ref| on the lattice as it is (N_delta 86 cycles at 300 m, growing with the baselines), w_full, per
    channel | band; measured 2026-10-21 on x86-64:
        300 m 8.6e-15 | 3.1e-15    3 km 8.3e-14 | 5.3e-15    30 km 1.0e-12 | 1.2e-13    300 km 9.9e-12 | 1.6e-12    2400 km 8.4e-11 | 7.2e-12
    0.14 to 0.17 of 2 pi u N_delta per channel: inside the 1e-12 of PSF_BOUND on the first two decades, ON it at 30 km (1.01e-12, which
    is asserted neither way), outside it from 300 km on."""
    for scale in M.SCALES:
        c = M.lattice_case(scale, 1)
        devs = []
        for chan_avg in (False, True):
            lat = M.lattice_of(scale, 1, 'full', chan_avg)
            pb = types.SimpleNamespace(w=NP.asarray(c['w_full']), W=NP.array([lat.W.sum()]) if chan_avg else lat.W, chan_avg=chan_avg)
            devs.append(float(NP.max(NP.abs(CS.beam(pb, c['unitvec'], c['rot'], c['baselines'], c['freqs'], c['ny'], c['nx']) - lat.P))))
        print('csclean_checker.beam x%d: %.2e per channel, %.2e band; N_delta %.3g, %.2f of 2 pi u N_delta'
              % (scale, devs[0], devs[1], lat.Nd.max(), devs[0] / (2 * NP.pi * M.U * lat.Nd.max())))
        assert scale not in P_CHECKER_KEEPS or devs[0] <= M.P_BAR, (scale, devs)
        assert scale not in P_CHECKER_LOSES or devs[0] > M.P_BAR, (scale, devs)


# ---- the restatement passes, wrong ones fail ----------------------------------------------------------------------------------------------
def test_the_restatement_of_the_mosaic_passes_the_rules_at_every_decade():
    worst = {}
    for field in ('sphere', 'narrow'):
        for scale in M.SCALES:
            c, geo = R.case(SHAPE, scale, field), R.geometry_of(SHAPE, scale, field)
            for route in ('direct', 'stepped'):
                bounds = M.snapshot_bounds(geo, c['baselines'], c['freqs'], route)
                for name in BEAMS:
                    ref = M.mosaic_of(SHAPE, scale, field, name)
                    tol_n, tol_q = M.tolerances(ref, bounds)
                    N, Q = restated_mosaic(c, ref.A, c['w_full'], route=route)
                    worst[(field, scale, name, route)] = (share(NP.abs(N - ref.num), tol_n), share(NP.abs(Q - ref.den), tol_q))
                print('restated mosaic %s x%d %s: N %s of tol_N, Q %s of tol_Q'
                      % (field, scale, route, ' '.join('%.3f' % worst[(field, scale, n, route)][0] for n in BEAMS),
                         ' '.join('%.1e' % worst[(field, scale, n, route)][1] for n in BEAMS)))
    assert max(max(v) for v in worst.values()) <= 1.0, worst


def test_the_restatement_of_P_passes_its_rule_and_follows_N_delta_not_N_b():
    for scale, shrink in ((1, 1), (10, 1), (100, 1), (1000, 1), (8000, 1), (1000, 1000), (8000, 8000)):
        c = M.lattice_case(scale, shrink)
        for chan_avg in (False, True):
            lat = M.lattice_of(scale, shrink, 'full', chan_avg)
            for route in ('stepped', 'direct'):
                dev = NP.abs(restated_P(c, c['w_full'], chan_avg, route=route) - lat.P).max(axis=(1, 2))
                bound = M.p_bound(lat, c['freqs'], route, band=chan_avg)
                assert NP.all(dev <= bound), (route, float(NP.max(dev / bound)))
            print('restated P x%d lattice / %d chan_avg=%d: %.2e, %.3f of its rule; N_delta %.3g (%.2f of it literal), N_b %.3g, %.1e of 2 pi u N_b'
                  % (scale, shrink, chan_avg, dev.max(), float(NP.max(dev / bound)), lat.Nd.max(), float(NP.min(lat.Nd_literal / lat.Nd)), lat.Nb.max(),
                     dev.max() / (2 * NP.pi * M.U * lat.Nb.max())))
            assert NP.all(dev <= bound)
            assert NP.all(lat.Nd <= 1.8 * lat.Nd_literal)
            assert NP.all(M.p_bound(lat, c['freqs'], 'stepped', band=chan_avg) <= R.update_bound(M.lattice_geometry(scale, shrink), c['freqs'], 'direct').min())
            if shrink > 1:
                # N_delta is what it is at 300 m and N_b a thousand times that and more: the error stays with N_delta ...
                assert lat.Nd.max() < 100.0 and lat.Nb.max() > 2e5 and dev.max() < 0.01 * 2 * NP.pi * M.U * lat.Nb.max()
    # ... where the image on its narrow field, whose directions are normalised unit vectors, follows N_b (imaging_reference, FLOOR)
    c, geo = R.case(SHAPE, 1000, 'narrow'), R.geometry_of(SHAPE, 1000, 'narrow')
    ref = R.image_of(SHAPE, 1000, 'narrow')
    _, d = restated_directions(c)
    cos, sin = restated_phasors(d, c['baselines'], c['freqs'])
    wv = c['w_full'] * c['cube']
    img = (NP.einsum('tbk,tpbk->pk', wv.real, cos) - NP.einsum('tbk,tpbk->pk', wv.imag, sin)) / c['w_full'].sum(axis=(0, 1))
    dev = float(NP.max(NP.abs(img - ref.image) / ref.scale))
    print('restated image, narrow field x1000: %.2e of the scale, %.2f of 2 pi u N_b, N\' %.3g' % (dev, dev / (2 * NP.pi * M.U * geo.Nb.max()), geo.Np.max()))
    assert dev > 0.05 * 2 * NP.pi * M.U * geo.Nb.max() and geo.Np.max() < 0.01 * geo.Nb.max()


@pytest.mark.parametrize('wrong', ['delta not rotated', 'rho over ny', 'mirror at (di, -dj)'])
def test_a_wrong_restatement_of_P_fails_its_rule(wrong):
    for scale, shrink in M.LATTICE_CONFIGS:
        c, lat = M.lattice_case(scale, shrink), M.lattice_of(scale, shrink)
        dev = NP.abs(restated_P(c, c['w_full'], False, wrong) - lat.P).max(axis=(1, 2))
        print('%s, x%d lattice / %d: %.2e, %.3g of the rule' % (wrong, scale, shrink, dev.max(), float(NP.max(dev / M.p_bound(lat, c['freqs'], 'direct')))))
        assert NP.all(dev > M.p_bound(lat, c['freqs'], 'direct'))


@pytest.mark.parametrize('wrong', ['A to the first power in Q', 'no horizon mask'])
def test_a_wrong_restatement_of_the_mosaic_fails_its_rule(wrong):
    for scale in (1, 1000):
        c, geo = R.case(SHAPE, scale, 'sphere'), R.geometry_of(SHAPE, scale, 'sphere')
        ref = M.mosaic_of(SHAPE, scale, 'sphere', 'dipole_ground')
        tol_n, tol_q = M.tolerances(ref, M.snapshot_bounds(geo, c['baselines'], c['freqs'], 'direct'))
        N, Q = restated_mosaic(c, ref.A, c['w_full'], wrong)
        n, q = share(NP.abs(N - ref.num), tol_n), share(NP.abs(Q - ref.den), tol_q)
        print('%s x%d: N %.3g of tol_N, Q %.3g of tol_Q' % (wrong, scale, n, q))
        assert q > 1.0 and (n > 1.0 or wrong != 'no horizon mask')


# ---- input conditions, on the reference alone -----------------------------------------------------------------------------------------------
def test_input_conditions_hold_at_every_scale():
    for shape, field in sorted({(sh, f) for sh, _, f in M.MOSAIC_CONFIGS}):
        scales = sorted({sc for sh, sc, f in M.MOSAIC_CONFIGS if (sh, f) == (shape, field)})
        up, margin = M.horizon_of(shape, scales[0], field)
        assert margin >= M.HORIZON_MARGIN and margin >= MK.HORIZON_MARGIN
        for name in BEAMS:
            first = M.mosaic_of(shape, scales[0], field, name)
            for scale in scales:
                ref = M.mosaic_of(shape, scale, field, name)
                assert NP.array_equal(R.geometry_of(shape, scale, field).s, R.geometry_of(shape, scales[0], field).s)
                # A, Q and W do not depend on the baselines: bit for bit the same at every scale
                assert NP.array_equal(ref.A, first.A) and NP.array_equal(ref.den_ld, first.den_ld) and NP.array_equal(ref.wt, first.wt)
                for chan_avg in (False, True):
                    ratio = M.mask_ratio(ref, M.PBMIN, chan_avg)
                    assert NP.min(NP.abs(ratio - 1.0)) > M.MASK_MARGIN
                    if (shape, field) == (SHAPE, 'sphere'):
                        masked = float(NP.mean(ratio < 1.0))
                        assert 0.1 <= masked <= 0.9, (name, chan_avg, masked)
            if (shape, field) == (SHAPE, 'sphere'):
                print('%s: the mask cuts %.2f of the elements' % (name, float(NP.mean(M.mask_ratio(first, M.PBMIN) < 1.0))))


def test_input_conditions_of_the_flipped_case():
    c = M.scaled(MC.up_case(33, 33, 65, 2, flip=(1,), down=20), 1000)
    up, margin = M.horizon(c['unitvec'], c['rot'], c['beta'], c['pc'])
    assert margin > 0.04 and NP.array_equal(up[0], NP.arange(65) < 45) and NP.array_equal(up[1], ~up[0])
    geo = R.geometry_case(c)
    for name in ('gaussian', 'dipole_ground'):
        A = M.beams(geo, up, M.SPECS[name], c['freqs'])
        assert NP.all(A[~up] == 0) and NP.any(A[1, 45:] > 0.01)          # what the flip puts up is seen, by that snapshot alone
        ref = M.mosaic(geo, A, c['cube'], c['w_full'])
        for chan_avg in (False, True):
            ratio = M.mask_ratio(ref, M.PBMIN, chan_avg)
            assert NP.min(NP.abs(ratio - 1.0)) > M.MASK_MARGIN and 0.1 <= float(NP.mean(ratio < 1.0)) <= 0.9


def test_input_conditions_of_the_clean_cases():
    """The case of prisim_clean_mosaic (pbmin 0.2) and the lattices of prisim_clean_mosaic_cs (6 m dishes, pbmin 0.3)."""
    c = M.scaled(QC.parity_case(SHAPE), 1000)
    geo = R.geometry_case(c)
    up, margin = M.horizon(c['unitvec'], c['rot'], c['beta'], c['pc'])
    assert margin >= M.HORIZON_MARGIN and up.all()
    for name in ('gaussian', 'airy'):
        ref = M.mosaic(geo, M.beams(geo, up, M.SPECS[name], c['freqs'], pointing=c['bpc']), c['cube'], c['w_full'])
        for chan_avg in (False, True):
            ratio = M.mask_ratio(ref, 0.2, chan_avg)
            print('clean of the mosaic, %s chan_avg=%d: the mask cuts %.2f, nothing within %.2f of its rim' % (name, chan_avg, float(NP.mean(ratio < 1.0)),
                                                                                                             float(NP.min(NP.abs(ratio - 1.0)))))
            assert NP.min(NP.abs(ratio - 1.0)) > 0.1 and 0.1 <= float(NP.mean(ratio < 1.0)) <= 0.9
    for scale, shrink in M.LATTICE_CONFIGS:
        c, geo = M.lattice_case(scale, shrink), M.lattice_geometry(scale, shrink)
        up, margin = M.horizon(c['unitvec'], c['rot'], c['beta'], c['pc'])
        assert margin >= M.HORIZON_MARGIN and not up[0].any() and up[1].all()        # snapshot 0 sees nothing of the lattice: its beam is 0
        for name in ('gaussian6', 'airy6'):
            ref = M.mosaic(geo, M.beams(geo, up, M.SPECS[name], c['freqs'], pointing=M.lattice_pointing(geo, c['ny'], c['nx'])), c['cube'], c['w_full'])
            for chan_avg in (False, True):
                ratio = M.mask_ratio(ref, 0.3, chan_avg)
                assert NP.min(NP.abs(ratio - 1.0)) > M.MASK_MARGIN and float(NP.mean(ratio >= 1.0)) >= 0.1
                assert shrink > 1 or float(NP.mean(ratio < 1.0)) >= 0.1


# ---- the Cotton-Schwab runs of the reference are not vacuous ----------------------------------------------------------------------------------
@pytest.mark.parametrize('scale, shrink', M.LATTICE_CONFIGS)
def test_the_reference_side_cotton_schwab_runs_are_not_vacuous(scale, shrink):
    c, geo = M.lattice_case(scale, shrink), M.lattice_geometry(scale, shrink)
    E = geo.cos.astype(NP.float64) + 1j * geo.sin.astype(NP.float64)
    pb = CK.Problem(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], c['cube'], weights=c['w_full'], aberr_beta=c['beta'], E=E)
    out = CS.clean(pb, M.lattice_of(scale, shrink).P, c['ny'], c['nx'], *(SETTING_A[n] for n in M.CS_ARGS))
    print('x%d lattice / %d: %d to %d cycles, %d to %d components, statuses %s'
          % (scale, shrink, out['ncycles'].min(), out['ncycles'].max(), out['ncomp'].min(), out['ncomp'].max(), sorted(set(out['status'].tolist()))))
    M.assert_not_vacuous(out)
