"""numpy statement of include/prisim_csclean.h, TEST INFRASTRUCTURE, built on tests/imclean_checker.py (its Problem: the phasors, the
dirty image, the visibilities of a component): the minor-cycle beam P of a lattice, an independent Cotton-Schwab CLEAN with numpy's
argmax, and a replay that follows the component lists and the cycle tables of another CLEAN -- the device's -- and asserts every
decision.

The replay follows the decisions it is given, so two pixels that tie to rounding cannot fail it; it asserts that each was a right one
to within the tolerance of imclean_checker, per image channel
    tol_k = BOUND * (scale_k + sum over the components so far of |a|),  BOUND = 1e-11,
so it cannot pass a wrong one either: every Pc within tol; every pick in the window and within 2 tol of the peak of the working image;
|a - gain R'[q]| <= gain tol; every continuation of a minor cycle at or above L - 2 tol, every end at or below L + 2 tol or at a cap;
every status justified in the order of the header; the final residual within tol of the dirty image of V - model, and the residual
visibilities within BOUND (max |V| of the channel + sum |a|) of V - model.  The exact residual at the start of a cycle is the replay's own
dirty image of V less the model so far, which is what the header defines it to be."""
import numpy as NP

import imaging_checker as IK
import imclean_checker as CK

BOUND = CK.BOUND
THRESHOLD, MAXITER, DEAD, MAJOR, DIVERGED = 1, 2, 4, 8, 16


def lattice_steps(unitvec, ny, nx):
    u = NP.asarray(unitvec, dtype=NP.float64).reshape(ny, nx, 3)
    rho = (u[ny - 1, nx // 2] - u[0, nx // 2]) / (ny - 1) if ny > 1 else NP.zeros(3)
    kappa = (u[ny // 2, nx - 1] - u[ny // 2, 0]) / (nx - 1) if nx > 1 else NP.zeros(3)
    return rho, kappa


def beam(pb, unitvec, rot, baselines, freqs_hz, ny, nx):
    """P (nc, 2 ny - 1, 2 nx - 1) of the problem pb: sum_tb w cos(2 pi f b . rot_t (di rho + dj kappa) / c) / W, the band's with chan_avg."""
    rho, kappa = lattice_steps(unitvec, ny, nx)
    di, dj = NP.meshgrid(NP.arange(-(ny - 1), ny), NP.arange(-(nx - 1), nx), indexing='ij')
    delta = di[..., None] * rho + dj[..., None] * kappa                            # (2ny-1, 2nx-1, 3)
    rt = NP.asarray(rot, dtype=NP.float64).reshape(-1, 3, 3)
    bl = NP.asarray(baselines, dtype=NP.float64).reshape(-1, 3)
    fq = NP.asarray(freqs_hz, dtype=NP.float64).ravel()
    tau = NP.einsum('tij,yxj,bi->tyxb', rt, delta, bl) / IK.C_LIGHT
    num = NP.zeros((fq.size,) + di.shape)
    for k in range(fq.size):                                                      # a channel at a time keeps the phases small in memory
        num[k] = NP.einsum('tb,tyxb->yx', pb.w[:, :, k], NP.cos(2.0 * NP.pi * fq[k] * tau))
    with NP.errstate(invalid='ignore', divide='ignore'):
        return (num.sum(axis=0, keepdims=True) / pb.W[0]) if pb.chan_avg else num / pb.W[:, None, None]


def shifted(Pk, q, ny, nx):
    """P[i_p - i_q][j_p - j_q] for every pixel p, (npix,)"""
    iq, jq = divmod(int(q), nx)
    return Pk[ny - 1 - iq:2 * ny - 1 - iq, nx - 1 - jq:2 * nx - 1 - jq].ravel()


def _peak1(pb, r):
    """(max over the window of |r|, its first pixel) of one image channel; (-1, -1) where nothing is a number"""
    a = NP.where(pb.window & ~NP.isnan(r), NP.abs(r), -1.0)
    q = int(NP.argmax(a))
    return (a[q], q) if a[q] >= 0.0 else (-1.0, -1)


def clean(pb, P, ny, nx, gain, maxiter, threshold, relative, depth, cycle_niter, max_major):
    """The independent Cotton-Schwab CLEAN.  Returns the dict of the device's outputs ('vres' included)."""
    nc = pb.nc
    cap = cycle_niter if cycle_niter and cycle_niter > 0 else None
    vm = NP.zeros_like(pb.v)
    R = pb.dirty(pb.v)
    status = NP.where(pb.dead, DEAD, 0).astype(NP.int32)
    pix, flux = [[] for _ in range(nc)], [[] for _ in range(nc)]
    cyc_n, cyc_p = [[] for _ in range(nc)], [[] for _ in range(nc)]
    peak0, thr, prev = NP.full(nc, NP.nan), NP.full(nc, NP.nan), NP.zeros(nc)
    for c in range(max_major + 1):
        peak, _ = pb.window_peak(R)
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
                r = R[:, k].copy()
                n = 0
                while (cap is None or n < cap) and len(pix[k]) < maxiter:
                    v, q = _peak1(pb, r)
                    if q < 0 or not v > L:
                        break
                    a = gain * r[q]
                    pix[k].append(q), flux[k].append(a)
                    r -= a * shifted(P[k], q, ny, nx)
                    vm += pb.component_vis(k, q, a)
                    n += 1
                cyc_n[k].append(len(pix[k]))
        if not ran:
            break
        R = pb.dirty(pb.v - vm)
    count = NP.array([len(x) for x in pix], dtype=NP.int32)
    ncycles = NP.array([len(x) for x in cyc_n], dtype=NP.int32)
    longest, most = (int(count.max()), int(ncycles.max())) if nc else (0, 0)
    cp, cf = NP.full((nc, longest), -1, dtype=NP.int32), NP.zeros((nc, longest))
    cn, cpk = NP.full((nc, most), -1, dtype=NP.int32), NP.full((nc, most + 1), NP.nan)
    for k in range(nc):
        cp[k, :count[k]], cf[k, :count[k]] = pix[k], flux[k]
        cn[k, :ncycles[k]] = cyc_n[k]
        cpk[k, :len(cyc_p[k])] = cyc_p[k]
    return {'residual': R if not pb.chan_avg else R[:, 0], 'comp_pixel': cp, 'comp_flux': cf, 'ncomp': count, 'status': status, 'peak0': peak0,
            'ncycles': ncycles, 'cycle_ncomp': cn, 'cycle_peak': cpk, 'vres': pb.v - vm}


def replay(pb, P, ny, nx, got, gain, maxiter, threshold, relative, depth, cycle_niter, max_major, bound=None):
    """Follows the lists and cycle tables of `got` (the dict of Context.clean_image_cs, or of clean()) and asserts every decision and
    the results.  Returns the largest deviation met, as a fraction of its tolerance.  bound: None for BOUND, or a pair of (nc,) arrays,
    the factor of the scale and that of the sum of |a| in the tolerance, as imclean_checker.replay takes them (tests/mosaic_reference.py
    says which they are at long baselines); the second also holds the residual visibilities."""
    b_scale, b_spent = (BOUND, BOUND) if bound is None else bound
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
    scale = NP.where(live, pb.scale, 0.0)
    spent = NP.zeros(nc)
    worst = 0.0

    def tol():
        return BOUND * (scale + spent) if bound is None else b_scale * scale + b_spent * spent

    def note(dev, t):
        nonlocal worst
        worst = max(worst, float(NP.max(NP.asarray(dev) / NP.asarray(t))) if NP.size(dev) else 0.0)

    got0 = NP.asarray(got['peak0'], dtype=NP.float64)
    assert NP.all(NP.isnan(got0[pb.dead]))
    thr = threshold * got0 if relative else NP.full(nc, float(threshold))
    vm = NP.zeros_like(pb.v)
    R = pb.dirty(pb.v)
    for c in range(most + 1):
        peak, _ = pb.window_peak(R)
        t = tol()
        for k in NP.flatnonzero(live & (ncyc >= c)):
            pc = cpk[k, c]
            assert peak[k] >= 0.0 and abs(pc - peak[k]) <= t[k], ('Pc', k, c, pc, peak[k], t[k])
            note(abs(pc - peak[k]), t[k])
            if c == 0:
                assert got0[k] == pc, ('P0 is the peak of cycle 0', k)
            held = int(cn[k, c - 1]) if c > 0 else 0
            over = peak[k] >= thr[k] - 2 * t[k]
            fell = c == 0 or peak[k] <= cpk[k, c - 1] + 2 * t[k]
            if ncyc[k] == c:                                                      # the channel ends at this test
                assert count[k] == held, ('components beyond the last cycle', k, count[k], held)
                if status[k] == THRESHOLD:
                    assert peak[k] <= thr[k] + 2 * t[k], ('a stop at the threshold above it', k, c, peak[k], thr[k])
                elif status[k] == MAXITER:
                    assert over and held == maxiter, ('a stop at maxiter', k, c, held)
                elif status[k] == DIVERGED:
                    assert over and held < maxiter and c > 0 and peak[k] >= cpk[k, c - 1] - 2 * t[k], ('a divergence that is none', k, c)
                else:
                    assert status[k] == MAJOR and over and held < maxiter and fell and c == max_major, ('a stop at max_major', k, c, status[k])
                continue
            assert over and held < maxiter and fell and c < max_major, ('a cycle that should not have started', k, c)
            n1 = int(cn[k, c])
            assert held < n1 <= min(maxiter, count[k]) and (cap is None or n1 - held <= cap), ('the components of a cycle', k, c, held, n1)
            L = max(thr[k], depth * pc)
            r = R[:, k].copy()
            for j in range(held, n1):
                tk = tol()[k]
                v, _ = _peak1(pb, r)
                q, a = int(cp[k, j]), cf[k, j]
                assert 0 <= q < npix and pb.window[q], ('a pick outside the window', k, j)
                assert abs(r[q]) >= v - 2 * tk, ('a pick that is not the peak', k, j, abs(r[q]), v)
                assert v >= L - 2 * tk, ('a continuation below the limit of the cycle', k, c, j, v, L)
                assert abs(a - gain * r[q]) <= gain * tk, ('a flux that is not gain * R[q]', k, j, a, gain * r[q], tk)
                note(v - abs(r[q]), 2 * tk)
                note(abs(a - gain * r[q]), gain * tk)
                r -= a * shifted(P[k], q, ny, nx)
                vm += pb.component_vis(k, q, a)
                spent[k] += abs(a)
            if not ((cap is not None and n1 - held == cap) or n1 == maxiter):
                tk = tol()[k]
                v, _ = _peak1(pb, r)
                assert v <= L + 2 * tk, ('a cycle ended early', k, c, v, L)
                note(max(v - L, 0.0), 2 * tk)
        R = pb.dirty(pb.v - vm)
    t = tol()
    res = NP.asarray(got['residual'], dtype=NP.float64).reshape(npix, nc)
    assert NP.array_equal(NP.isnan(res), NP.broadcast_to(pb.dead, res.shape)), 'NaN in the dead channels and nowhere else'
    dev = NP.abs(res - R)[:, live]
    assert NP.all(dev <= t[live]), ('the residual against the dirty image of V - model', float(NP.max(dev / t[live])))
    note(dev, t[live])
    if got.get('vres') is not None:
        vres = NP.asarray(got['vres'])
        assert vres.shape == pb.v.shape
        bound = NP.max(b_spent) * (NP.abs(pb.v).max(axis=(0, 1)) + spent[0]) if pb.chan_avg else b_spent * (NP.abs(pb.v).max(axis=(0, 1)) + spent)
        dev = NP.abs(vres - (pb.v - vm)).max(axis=(0, 1))
        assert NP.all(dev <= bound), ('the residual visibilities against V - model', float(NP.max(dev / bound)))
        note(dev, bound)
    return worst
