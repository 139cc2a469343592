"""numpy statement of include/prisim_moscs.h, TEST INFRASTRUCTURE, built on tests/mosclean_checker.py (its Problem: the phasors, the
beams, the sums and the bounds of the mosaic) and tests/csclean_checker.py (the minor-cycle beam P of a lattice and its shifts): an
independent Cotton-Schwab CLEAN of the mosaic with numpy's argmax, and a replay that follows the component lists and the cycle tables
of another CLEAN -- the device's -- and asserts every decision.

The replay follows the decisions it is given, so two pixels that tie to rounding cannot fail it; it asserts that each was a right one
to within the tolerance, so it cannot pass a wrong one either.  The exact numerator at the start of a cycle is the replay's own
mosaic numerator of V less the model so far, which is what the header defines it to be.

Tolerances.  No constant is new: BOUND = 1e-11 and BEAM_BOUND = 1e-12 of mosclean_checker, whose Problem.tolerances gives tol_N, tol_F
and tmax = the largest tol_F over the searched pixels from the reference's own N, Q and W, with spent_q = sum |a_c| A[t][q_c] and spent
= sum |a_c| over the components so far; 1e-12 for P, the bound of tests/test_gpu_csclean.py.
  Start of a cycle.  R_N is the mosaic's numerator of V - model: that is what tol_N bounds, and F = R_N / sqrt(Q W) what tol_F does.
    So Pc, a maximum over pixels, is within tmax of the replay's.
  Inside a minor cycle the working image is F' = F - sum_j c_j P[. - q_j].  F carries tol_F of the cycle's start.  Each subtraction
    rounds a product and a difference of magnitude at most |c_j| (|P| <= 1): a few 2^-53 |c_j|, where tol_F already grows by some
    1e-11 |a_j| A / sqrt(Q W) per component once |a_j| is added to spent -- so tF is tol_F of the cycle's start with the components
    of the running cycle added to spent as they are appended, and tmax its largest over the searched pixels.  Two peaks that both
    carry tmax are compared to 2 tmax: every pick within 2 tmax of the working peak, every continuation >= L - 2 tmax, every end
    <= L + 2 tmax or at a cap.
  The flux a = gain F'[q] sqrt(Wc / Qc[q]): to first order in F' +- tF and Q +- tol_Q, d sqrt(W / Q) = -sqrt(W / Q) dQ / (2 Q), so
      |a - gain r[q] sqrt(Wc / Qc[q])| <= gain sqrt(Wc / Qc[q]) tF[q] + |a| tol_Q[q] / (2 Qc[q])
  The end.  num within tol_N of the replay's numerator and of mosaic_checker's mosaic of V - model; den within tol_Q; the quotients,
    the mask and residual_flat recomputed from the returned num, den and wsum and compared exactly, NaN positions included.  The
    residual visibilities: a visibility loses sum_j (a_j A[t][q_j]) e^{-i phi_j}; each term carries the 1e-11 of a phasor at the
    scale of |a_j| (A <= 1) and the 1e-12 of a device beam value times |a_j|, so
      |vres - (V - model)| <= BOUND (max_{t,b} |V[:, :, k]| + spent_k) + BEAM_BOUND spent_k
Input conditions are those of mosclean_checker.Problem, asserted there.  Nothing is skipped."""
import types

import numpy as NP

import csclean_checker as CS
import mosaic_checker as MK
import mosclean_checker as QK

BOUND, BEAM_BOUND = QK.BOUND, QK.BEAM_BOUND
THRESHOLD, MAXITER, DEAD, MAJOR, DIVERGED = CS.THRESHOLD, CS.MAXITER, CS.DEAD, CS.MAJOR, CS.DIVERGED
PSF_BOUND = 1e-12


def beam(pb, ny, nx):
    """P (nc, 2 ny - 1, 2 nx - 1) of the mosaic Problem pb, by csclean_checker.beam: the weights over their sums, the band's with
    chan_avg; NaN in a channel without weight."""
    u, rot, _, bl, fq, _ = pb.geometry
    return CS.beam(types.SimpleNamespace(w=pb.w, W=pb.Wc, chan_avg=pb.chan_avg), u, rot, bl, fq, ny, nx)


def scale_of(pb):
    """s (npix, nc) = sqrt(Wc / Qc): what turns a flat amplitude into a true flux"""
    with NP.errstate(invalid='ignore', divide='ignore'):
        return NP.sqrt(pb.Wc[NP.newaxis, :] / pb.Qc)


def _peak1(pb, r, k):
    """(max over the window and the mask of |r|, its first pixel) of image channel k; (-1, -1) where there is none"""
    a = NP.where(pb.search[:, k] & ~NP.isnan(r), NP.abs(r), -1.0)
    q = int(NP.argmax(a))
    return (a[q], q) if a[q] >= 0.0 else (-1.0, -1)


def _spend(pb, spent_q, spent, k, q, a):
    ks = slice(None) if pb.chan_avg else slice(k, k + 1)
    spent_q[:, ks] += abs(a) * pb.A[:, q, ks]
    spent[ks] += abs(a)


def channel_tolerance(pb, RN, k, bound=None):
    """Problem.tolerances(RN, spent_q, spent) for image channel k alone, as a function of (spent_q, spent): (tol_F[:, k], tmax[k]).
    The same expressions on the channel's own columns, so that a minor cycle of many components does not form the bounds of every
    other channel once per component (tests/test_moscs.py holds the two against each other)."""
    if pb.chan_avg:
        def whole(spent_q, spent):
            _, tol_F, tmax = pb.tolerances(RN, spent_q, spent, bound)
            return tol_F[:, 0], tmax[0]
        return whole
    b_scale, b_spent = (b * NP.ones((pb.nt, pb.nchan)) for b in ((BOUND, BOUND) if bound is None else bound))
    Ak = NP.ascontiguousarray(pb.A[:, :, k])                                        # (nt, npix)
    AW = pb.Wt[:, k].dot(Ak)
    srch = pb.search[:, k]
    with NP.errstate(invalid='ignore', divide='ignore'):
        inv = 1.0 / NP.sqrt(pb.Qc[:, k] * pb.Wc[k])
        fterm = NP.abs(pb.flat(RN)[:, k]) * pb.tol_Q[:, k] / (2.0 * pb.Qc[:, k])

    def own(spent_q, spent):
        scale = pb.absV[:, k] + pb.Wt[:, k] * spent_q[:, k]
        sums = BOUND * scale.dot(Ak) if bound is None else (b_scale[:, k] * pb.absV[:, k] + b_spent[:, k] * (pb.Wt[:, k] * spent_q[:, k])).dot(Ak)
        tol_N = sums + BEAM_BOUND * (scale.sum() + AW * spent[k])
        with NP.errstate(invalid='ignore'):
            tol_F = tol_N * inv + fterm
        return tol_F, (float(NP.max(tol_F[srch])) if srch.any() else 0.0)
    return own


def clean(pb, P, ny, nx, gain, maxiter, threshold, relative, depth, cycle_niter, max_major):
    """The independent Cotton-Schwab CLEAN of the mosaic.  Returns the dict of the device's outputs ('vres' included, 'psf' is P)."""
    nc = pb.nc
    cap = cycle_niter if cycle_niter and cycle_niter > 0 else None
    s = scale_of(pb)
    vm = NP.zeros_like(pb.v)
    RN = pb.numerator(pb.v)
    status = NP.where(pb.dead, DEAD, 0).astype(NP.int32)
    pix, flux = [[] for _ in range(nc)], [[] for _ in range(nc)]
    cyc_n, cyc_p = [[] for _ in range(nc)], [[] for _ in range(nc)]
    peak0, thr, prev = NP.full(nc, NP.nan), NP.full(nc, NP.nan), NP.zeros(nc)
    for c in range(max_major + 1):
        F = pb.flat(RN)
        peak, _ = pb.peak(F)
        ran = False
        for k in NP.flatnonzero(status == 0):
            if c == 0:
                if peak[k] >= 0.0:
                    peak0[k] = peak[k]
                thr[k] = threshold * peak[k] if relative else threshold
            cyc_p[k].append(peak[k] if peak[k] >= 0.0 else NP.nan)
            if peak[k] < 0.0 or not peak[k] > thr[k]:
                status[k] = THRESHOLD
            elif len(pix[k]) >= maxiter:
                status[k] = MAXITER
            elif c > 0 and peak[k] > prev[k]:
                status[k] = DIVERGED
            elif c == max_major:
                status[k] = MAJOR
            else:
                ran = True
                prev[k] = peak[k]
                L = max(thr[k], depth * peak[k])
                r = F[:, k].copy()
                n = 0
                while (cap is None or n < cap) and len(pix[k]) < maxiter:
                    v, q = _peak1(pb, r, k)
                    if q < 0 or not v > L:
                        break
                    cflat = gain * r[q]
                    a = cflat * s[q, k]
                    pix[k].append(q), flux[k].append(a)
                    r -= cflat * CS.shifted(P[k], q, ny, nx)
                    vm += pb.component_vis(k, q, a)
                    n += 1
                cyc_n[k].append(len(pix[k]))
        if not ran:
            break
        RN = pb.numerator(pb.v - vm)
    count = NP.array([len(x) for x in pix], dtype=NP.int32)
    ncycles = NP.array([len(x) for x in cyc_n], dtype=NP.int32)
    longest, most = (int(count.max()), int(ncycles.max())) if nc else (0, 0)
    cp, cf = NP.full((nc, longest), -1, dtype=NP.int32), NP.zeros((nc, longest))
    cn, cpk = NP.full((nc, most), -1, dtype=NP.int32), NP.full((nc, most + 1), NP.nan)
    for k in range(nc):
        cp[k, :count[k]], cf[k, :count[k]] = pix[k], flux[k]
        cn[k, :ncycles[k]] = cyc_n[k]
        cpk[k, :len(cyc_p[k])] = cyc_p[k]
    out = pb.outputs(RN, cp, cf, count, status, peak0)
    out.update(ncycles=ncycles, cycle_ncomp=cn, cycle_peak=cpk, vres=pb.v - vm, psf=P)
    return out


def replay(pb, P, ny, nx, got, gain, maxiter, threshold, relative, depth, cycle_niter, max_major, bound=None, psf_bound=None):
    """Follows the lists and cycle tables of `got` (the dict of Context.clean_mosaic_cs, or of clean()) and asserts every decision
    and the results.  Returns the largest deviation met, as a fraction of its tolerance.  bound: what mosclean_checker's
    Problem.tolerances takes, its second factor (the largest over the snapshots) also for the residual visibilities; psf_bound: (nc,)
    in place of PSF_BOUND (tests/mosaic_reference.py derives both)."""
    nc, npix = pb.nc, pb.npix
    cap = cycle_niter if cycle_niter and cycle_niter > 0 else None
    cp, cf, count, status, ncyc, cn, cpk = (NP.asarray(got[n]) for n in ('comp_pixel', 'comp_flux', 'ncomp', 'status', 'ncycles', 'cycle_ncomp',
                                                                         'cycle_peak'))
    assert cp.shape == cf.shape and cp.shape[0] == nc and count.shape == status.shape == ncyc.shape == (nc,)
    assert cp.shape[1] == (int(count.max()) if nc else 0) and NP.all(count >= 0) and NP.all(count <= maxiter)
    most = int(ncyc.max()) if nc else 0
    assert cn.shape == (nc, most) and cpk.shape == (nc, most + 1) and NP.all(ncyc >= 0) and most <= max_major, 'the shapes of the cycle tables'
    assert NP.array_equal(status == DEAD, pb.dead) and NP.all(count[pb.dead] == 0) and NP.all(ncyc[pb.dead] == 0), 'the dead channels'
    assert NP.all(NP.isin(status, (THRESHOLD, MAXITER, DEAD, MAJOR, DIVERGED)))
    live = ~pb.dead
    empty = live & ~pb.search.any(axis=0)                             # nothing to search: THRESHOLD at once, a NaN P0, no cycle
    seen = live & ~empty
    s = scale_of(pb)
    tol_Qc = pb.band(pb.tol_Q)
    worst = 0.0

    def note(dev, t):
        nonlocal worst
        dev, t = NP.asarray(dev, dtype=NP.float64), NP.asarray(t, dtype=NP.float64)
        if dev.size:
            with NP.errstate(invalid='ignore', divide='ignore'):
                worst = max(worst, float(NP.max(NP.where(t > 0.0, dev / t, NP.where(dev > 0.0, NP.inf, 0.0)))))

    got0 = NP.asarray(got['peak0'], dtype=NP.float64)
    assert NP.all(NP.isnan(got0[~seen])), 'P0 of a channel that is dead or has nothing to search is NaN'
    assert NP.all(count[empty] == 0) and NP.all(status[empty] == THRESHOLD) and NP.all(ncyc[empty] == 0), \
        'a channel with nothing to search ends at the threshold at once'
    assert NP.all(NP.isnan(cpk[~seen])), 'no peak is recorded where nothing was searched'
    thr = threshold * got0 if relative else NP.full(nc, float(threshold))
    vm = NP.zeros_like(pb.v)
    RN = pb.numerator(pb.v)
    spent_q, spent = NP.zeros((pb.nt, pb.nchan)), NP.zeros(pb.nchan)
    for c in range(most + 1):
        F = pb.flat(RN)
        peak, _ = pb.peak(F)
        _, _, tmax = pb.tolerances(RN, spent_q, spent, bound)
        # the components of this cycle are added to these as they are appended; a channel's own columns alone bear on its tolerance
        run_q, run = spent_q.copy(), spent.copy()
        for k in NP.flatnonzero(seen & (ncyc >= c)):
            pc, t2 = cpk[k, c], 2 * tmax[k]
            assert peak[k] >= 0.0 and abs(pc - peak[k]) <= tmax[k], ('Pc', k, c, pc, peak[k], tmax[k])
            note(abs(pc - peak[k]), tmax[k])
            if c == 0:
                assert got0[k] == pc, ('P0 is the peak of cycle 0', k)
            held = int(cn[k, c - 1]) if c > 0 else 0
            over = peak[k] >= thr[k] - t2
            fell = c == 0 or peak[k] <= cpk[k, c - 1] + t2
            if ncyc[k] == c:                                                      # the channel ends at this test
                assert count[k] == held, ('components beyond the last cycle', k, count[k], held)
                if status[k] == THRESHOLD:
                    assert peak[k] <= thr[k] + t2, ('a stop at the threshold above it', k, c, peak[k], thr[k])
                elif status[k] == MAXITER:
                    assert over and held == maxiter, ('a stop at maxiter', k, c, held)
                elif status[k] == DIVERGED:
                    assert over and held < maxiter and c > 0 and peak[k] >= cpk[k, c - 1] - t2, ('a divergence that is none', k, c)
                else:
                    assert status[k] == MAJOR and over and held < maxiter and fell and c == max_major, ('a stop at max_major', k, c, status[k])
                continue
            assert over and held < maxiter and fell and c < max_major, ('a cycle that should not have started', k, c)
            n1 = int(cn[k, c])
            assert held < n1 <= min(maxiter, count[k]) and (cap is None or n1 - held <= cap), ('the components of a cycle', k, c, held, n1)
            L = max(thr[k], depth * pc)
            r = F[:, k].copy()
            tolerance = channel_tolerance(pb, RN, k, bound)
            for j in range(held, n1):
                tF, tm = tolerance(run_q, run)
                v, _ = _peak1(pb, r, k)
                q, a = int(cp[k, j]), cf[k, j]
                assert 0 <= q < npix and pb.window[q], ('a pick outside the window', k, j)
                assert pb.valid[q, k] and pb.search[q, k], ('a pick on a masked pixel', k, j, q)
                assert abs(r[q]) >= v - 2 * tm, ('a pick that is not the peak', k, j, abs(r[q]), v)
                assert v >= L - 2 * tm, ('a continuation below the limit of the cycle', k, c, j, v, L)
                want = gain * r[q] * s[q, k]
                ta = gain * s[q, k] * tF[q] + abs(a) * tol_Qc[q, k] / (2.0 * pb.Qc[q, k])
                assert abs(a - want) <= ta, ('a flux that is not gain * F[q] * sqrt(W / Q[q])', k, j, a, want, ta)
                note(v - abs(r[q]), 2 * tm)
                note(abs(a - want), ta)
                r -= (a / s[q, k]) * CS.shifted(P[k], q, ny, nx)                    # the flat amplitude the other CLEAN took
                vm += pb.component_vis(k, q, a)
                _spend(pb, run_q, run, k, q, a)
            if not ((cap is not None and n1 - held == cap) or n1 == maxiter):
                _, tm = tolerance(run_q, run)
                v, _ = _peak1(pb, r, k)
                assert v <= L + 2 * tm, ('a cycle ended early', k, c, v, L)
                note(max(v - L, 0.0), 2 * tm)
        spent_q, spent = run_q, run
        RN = pb.numerator(pb.v - vm)
    tol_N, _, _ = pb.tolerances(RN, spent_q, spent, bound)
    num, den, wsum = (NP.asarray(got[n], dtype=NP.float64) for n in ('num', 'den', 'wsum'))
    assert num.shape == den.shape == (npix, pb.nchan) and wsum.shape == (pb.nchan,)
    dev = NP.abs(num - RN)
    assert NP.all(dev <= tol_N), ('the numerator against the replay', float(NP.max(dev / tol_N)))
    note(dev, tol_N)
    # linearity, by the mosaic's own checker: R_N is the mosaic's numerator of the visibilities less those of the model
    u, rot, pc_, bl, fq, beta = pb.geometry
    sums = MK.snapshot_sums(u, rot, pc_, bl, fq, pb.v - vm, weights=pb.weights, aberr_beta=beta)
    ref = MK.combine(sums, pb.A, pbmin=pb.pbmin, chan_avg=pb.chan_avg)
    dev = NP.abs(num - ref['num'])
    assert NP.all(dev <= tol_N), ('the numerator against the mosaic of V - model', float(NP.max(dev / tol_N)))
    note(dev, tol_N)
    dev = NP.abs(den - pb.Q)
    assert NP.all(dev <= pb.tol_Q), ('Q', float(NP.max(dev / NP.where(pb.tol_Q > 0, pb.tol_Q, 1.0))))
    note(dev, pb.tol_Q)
    assert NP.allclose(wsum, pb.Wtot, rtol=1e-13, atol=0)
    # the quotients and the mask: exactly what the header's expressions make of the returned num, den and wsum
    residual, pb_eff = MK.quotient(num, den, wsum, pb.pbmin, pb.chan_avg)
    for name, want in (('residual', residual), ('pb_eff', pb_eff), ('residual_flat', QK.flat_of(num, den, wsum, pb.pbmin, pb.chan_avg))):
        have = NP.asarray(got[name], dtype=NP.float64)
        assert have.shape == want.shape and NP.array_equal(have, want, equal_nan=True), name
    masked = NP.isnan(NP.asarray(got['residual_flat'], dtype=NP.float64)).reshape(npix, nc)
    assert NP.array_equal(masked[:, live], (~pb.valid | (pb.Qc == 0.0))[:, live]) and NP.all(masked[:, pb.dead]), 'the mask is the reference\'s'
    if got.get('vres') is not None:
        vres = NP.asarray(got['vres'])
        assert vres.shape == pb.v.shape
        b_vis = BOUND if bound is None else NP.max(bound[1] * NP.ones((pb.nt, pb.nchan)), axis=0)
        vbound = b_vis * (NP.abs(pb.v).max(axis=(0, 1)) + spent) + BEAM_BOUND * spent
        dev = NP.abs(vres - (pb.v - vm)).max(axis=(0, 1))
        assert NP.all(dev <= vbound), ('the residual visibilities against V - model', float(NP.max(dev / vbound)))
        note(dev, vbound)
    if got.get('psf') is not None:
        psf = NP.asarray(got['psf'], dtype=NP.float64)
        assert psf.shape == P.shape
        pbound = NP.full(nc, PSF_BOUND) if psf_bound is None else NP.asarray(psf_bound, dtype=NP.float64) * NP.ones(nc)
        dev = NP.abs(psf - P)[live]
        assert NP.all(dev <= pbound[live, None, None]), ('P against the checker\'s', float(NP.max(dev / pbound[live, None, None])))
        note(dev, pbound[live, None, None])
    return worst
