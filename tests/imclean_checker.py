"""numpy statement of include/prisim_imclean.h, TEST INFRASTRUCTURE, built on tests/imaging_checker.py: an independent Hogbom CLEAN
with the exact beam (its own argmax), and a replay that follows the component lists of another CLEAN -- the device's -- and rebuilds
the sequence of residuals in complex128, every phase from the channel's own frequency.

The replay follows the decisions it is given, so two pixels that tie to rounding cannot fail it; it asserts that every decision was
a right one to within the tolerance, so it cannot pass a wrong pick either.  Tolerance per image channel:
    tol_k = BOUND * (scale_k + sum over the components so far of |a|),  BOUND = 1e-11 (the project's fp64 bound),
scale_k the natural scale of tests/imaging_checker.py (sum w|V| / sum w), and the second term the scale of the model visibilities
that the updates have imaged.  Nothing is skipped."""
import numpy as NP

import imaging_checker as IK

BOUND = 1e-11
THRESHOLD, MAXITER, DEAD = 1, 2, 4


class Problem(object):
    """The phasors and sums of one imaging problem.  E[t][p][b][k] = e^{+i phi}, phi = 2 pi f_k b . (s[p][t] - s0[t]) / c; w, v
    (nt, nbl, nchan); W (nchan,); nc image channels.  Everything in the image-channel layout (npix, nc)."""

    def __init__(self, unitvec, rot, pc_dircos, baselines, freqs_hz, cube, weights=None, aberr_beta=None, chan_avg=False, window=None,
                 nonzero=None, E=None):
        bl = NP.asarray(baselines, dtype=NP.float64).reshape(-1, 3)
        fq = NP.asarray(freqs_hz, dtype=NP.float64).ravel()
        s = IK.directions(unitvec, rot, aberr_beta)
        pc = NP.asarray(pc_dircos, dtype=NP.float64).reshape(-1, 3)
        self.nt, self.npix, self.nbl, self.nchan = s.shape[0], s.shape[1], bl.shape[0], fq.size
        tau = NP.einsum('tpi,bi->tpb', s - pc[:, NP.newaxis, :], bl) / IK.C_LIGHT
        self.E = NP.exp(2j * NP.pi * tau[..., NP.newaxis] * fq) if E is None else E      # E: that of another Problem of the same geometry
        assert self.E.shape == (self.nt, self.npix, self.nbl, self.nchan)
        self.w = NP.array(IK.full_weights(weights, self.nt, self.nbl, self.nchan), dtype=NP.float64)
        self.v = NP.asarray(cube, dtype=NP.complex128)
        assert self.v.shape == (self.nt, self.nbl, self.nchan)
        self.chan_avg = bool(chan_avg)
        self.nc = 1 if chan_avg else self.nchan
        W = NP.einsum('tbk->k', self.w)
        meant = NP.ones(self.nchan, dtype=bool) if nonzero is None else NP.asarray(nonzero, dtype=bool)
        assert NP.all(W[meant] >= 1.0) and NP.all(W[~meant] == 0.0)
        num = NP.einsum('tbk->k', self.w * NP.abs(self.v))
        with NP.errstate(invalid='ignore', divide='ignore'):
            self.W = NP.array([W.sum()]) if chan_avg else W
            self.scale = NP.array([num.sum() / W.sum()]) if chan_avg else num / W
        self.dead = self.W == 0.0
        self.window = NP.ones(self.npix, dtype=bool) if window is None else NP.asarray(window) != 0
        assert self.window.shape == (self.npix,) and self.window.any()

    def dirty(self, v):
        """The dirty image of the visibilities v, (npix, nc); NaN where the weight sum is 0."""
        D = NP.einsum('tbk,tpbk->pk', self.w * v, self.E).real
        with NP.errstate(invalid='ignore', divide='ignore'):
            return D.sum(axis=1, keepdims=True) / self.W if self.chan_avg else D / self.W

    def component_vis(self, k, q, a):
        """The visibilities of the component (q, a) of image channel k: a e^{-i phi_q}, (nt, nbl, nchan), zero outside the channel."""
        out = NP.zeros_like(self.v)
        if self.chan_avg:
            out[:] = a * self.E[:, q].conj()
        else:
            out[:, :, k] = a * self.E[:, q, :, k].conj()
        return out

    def beams(self, ks, qs, fluxes):
        """B[:, j] of the components (qs[j], fluxes[j]) of the image channels ks[j]: (npix, len(ks))."""
        if self.chan_avg:
            assert list(ks) == [0]
            x = self.w * self.E[:, qs[0]].conj()                                   # (nt, nbl, nchan)
            return (fluxes[0] * NP.einsum('tbk,tpbk->p', x, self.E).real / self.W[0])[:, NP.newaxis]
        ks, qs = NP.asarray(ks), NP.asarray(qs)
        Eq = NP.stack([self.E[:, q, :, k] for k, q in zip(ks, qs)], axis=-1)       # (nt, nbl, nk)
        x = self.w[:, :, ks] * Eq.conj()
        Ek = self.E if NP.array_equal(ks, NP.arange(self.nchan)) else self.E[:, :, :, ks]
        return NP.einsum('tbk,tpbk->pk', x, Ek).real * NP.asarray(fluxes) / self.W[ks]

    def window_peak(self, R):
        """(max over the window of |R|, its first pixel) per image channel; (-1, -1) where nothing in the window is a number."""
        a = NP.where(self.window[:, NP.newaxis] & ~NP.isnan(R), NP.abs(R), -1.0)
        q = NP.argmax(a, axis=0)                                                  # the first of equal values: the lowest pixel
        peak = a[q, NP.arange(self.nc)]
        return peak, NP.where(peak >= 0.0, q, -1)


def clean(pb, gain, maxiter, threshold, relative):
    """The independent CLEAN: every channel in step, numpy's own argmax.  Returns the dict of the device's outputs."""
    R = pb.dirty(pb.v)
    nc = pb.nc
    peak0, _ = pb.window_peak(R)
    peak0 = NP.where(peak0 >= 0.0, peak0, NP.nan)
    thr = threshold * peak0 if relative else NP.full(nc, float(threshold))
    status = NP.where(pb.dead, DEAD, 0).astype(NP.int32)
    pix, flux = [[] for _ in range(nc)], [[] for _ in range(nc)]
    while NP.any(status == 0):
        peak, q = pb.window_peak(R)
        ks, qs, fl = [], [], []
        for k in NP.flatnonzero(status == 0):
            if q[k] < 0 or not peak[k] > thr[k]:
                status[k] = THRESHOLD
            elif len(pix[k]) >= maxiter:
                status[k] = MAXITER
            else:
                a = gain * R[q[k], k]
                pix[k].append(int(q[k]))
                flux[k].append(a)
                ks.append(k), qs.append(int(q[k])), fl.append(a)
        if ks:
            R[:, ks] -= pb.beams(ks, qs, fl)
    count = NP.array([len(x) for x in pix], dtype=NP.int32)
    longest = int(count.max()) if nc else 0
    cp, cf = NP.full((nc, longest), -1, dtype=NP.int32), NP.zeros((nc, longest))
    for k in range(nc):
        cp[k, :count[k]], cf[k, :count[k]] = pix[k], flux[k]
    return {'residual': R if not pb.chan_avg else R[:, 0], 'comp_pixel': cp, 'comp_flux': cf, 'ncomp': count, 'status': status, 'peak0': peak0}


def replay(pb, got, gain, maxiter, threshold, relative, bound=None):
    """Follows the lists of `got` (the dict of Context.clean_image, or of clean()) and asserts every decision and the results.  Returns
    the largest deviation met, as a fraction of its tolerance.  bound: None for BOUND, or a pair of (nc,) arrays, the factor of the scale
    and that of the sum of |a| in the tolerance (tests/imaging_reference.py derives them for long baselines)."""
    b_scale, b_spent = (BOUND, BOUND) if bound is None else bound
    nc, npix = pb.nc, pb.npix
    cp, cf, count, status = (NP.asarray(got[n]) for n in ('comp_pixel', 'comp_flux', 'ncomp', 'status'))
    assert cp.shape == cf.shape and cp.shape[0] == nc and count.shape == (nc,) and status.shape == (nc,)
    assert cp.shape[1] == (int(count.max()) if nc else 0) and NP.all(count >= 0) and NP.all(count <= maxiter)
    assert NP.array_equal(status == DEAD, pb.dead) and NP.all(count[pb.dead] == 0), 'the channels without weight, and they alone, are dead'
    assert NP.all(NP.isin(status, (THRESHOLD, MAXITER, DEAD)))
    live = ~pb.dead
    R = pb.dirty(pb.v)
    scale = NP.where(live, pb.scale, 0.0)
    spent = NP.zeros(nc)                                                          # sum of |a| so far
    worst = 0.0

    def tol():
        return b_scale * scale + b_spent * spent

    def note(dev, t):
        nonlocal worst
        worst = max(worst, float(NP.max(NP.asarray(dev) / NP.asarray(t))) if NP.size(dev) else 0.0)

    peak0, _ = pb.window_peak(R)
    assert NP.all(peak0[live] >= 0.0)
    got0 = NP.asarray(got['peak0'], dtype=NP.float64)
    assert NP.all(NP.isnan(got0[pb.dead])) and NP.all(NP.abs(got0[live] - peak0[live]) <= tol()[live]), 'P0'
    note(NP.abs(got0[live] - peak0[live]), tol()[live])
    # the threshold the other CLEAN compared with came from its own P0
    thr = threshold * got0 if relative else NP.full(nc, float(threshold))
    vm = NP.zeros_like(pb.v)                                                      # the model visibilities
    for i in range(cp.shape[1] + 1):
        peak, _ = pb.window_peak(R)
        t = tol()
        going = NP.flatnonzero(live & (count > i))
        ending = NP.flatnonzero(live & (count == i))
        for k in ending:
            if status[k] == THRESHOLD:
                assert peak[k] <= thr[k] + 2 * t[k], ('a stop at the threshold above it', k, i, peak[k], thr[k], t[k])
                note(max(peak[k] - thr[k], 0.0), 2 * t[k])
            else:
                assert status[k] == MAXITER and count[k] == maxiter, ('a stop that is neither', k, i, status[k])
                assert peak[k] >= thr[k] - 2 * t[k], ('a stop at maxiter below the threshold', k, i, peak[k], thr[k], t[k])
        if not going.size:
            continue
        qs, fl = cp[going, i], cf[going, i]
        assert NP.all((qs >= 0) & (qs < npix)) and NP.all(pb.window[qs]), ('a pick outside the window', i)
        at = R[qs, going]
        assert NP.all(NP.abs(at) >= peak[going] - 2 * t[going]), ('a pick that is not the peak', i, going, NP.abs(at), peak[going])
        assert NP.all(peak[going] >= thr[going] - 2 * t[going]), ('a continuation below the threshold', i)
        assert NP.all(NP.abs(fl - gain * at) <= gain * t[going]), ('a flux that is not gain * R[q]', i, fl, gain * at, t[going])
        note(peak[going] - NP.abs(at), 2 * t[going])
        note(NP.abs(fl - gain * at), gain * t[going])
        R[:, going] -= pb.beams(going, qs, fl)
        for k, q, a in zip(going, qs, fl):
            vm += pb.component_vis(k, int(q), a)
        spent[going] += NP.abs(fl)
    t = tol()
    res = NP.asarray(got['residual'], dtype=NP.float64).reshape(npix, nc)
    assert NP.array_equal(NP.isnan(res), NP.broadcast_to(pb.dead, res.shape)), 'NaN in the dead channels and nowhere else'
    dev = NP.abs(res - R)[:, live]
    assert NP.all(dev <= t[live]), ('the residual against the replay', float(NP.max(dev / t[live])))
    note(dev, t[live])
    # linearity: the residual is the dirty image of the visibilities less those of the model
    dev = NP.abs(res - pb.dirty(pb.v - vm))[:, live]
    assert NP.all(dev <= t[live]), ('the residual against the dirty image of V - model', float(NP.max(dev / t[live])))
    note(dev, t[live])
    return worst


def restored(residual, unitvec, comp_pixel, comp_flux, ncomp, fwhm_rad):
    """R[p][k] + sum over the components (q, a) of k of a exp(-4 ln 2 theta^2 / fwhm_k^2), theta = 2 asin(min(1, |u_p - u_q| / 2))."""
    u = NP.asarray(unitvec, dtype=NP.float64).reshape(-1, 3)
    res = NP.asarray(residual, dtype=NP.float64)
    out = res.reshape(u.shape[0], -1).copy()
    for k in range(out.shape[1]):
        for q, a in zip(comp_pixel[k, :ncomp[k]], comp_flux[k, :ncomp[k]]):
            theta = 2.0 * NP.arcsin(NP.minimum(1.0, 0.5 * NP.sqrt(NP.sum((u - u[q]) ** 2, axis=1))))
            out[:, k] += a * NP.exp(-4.0 * NP.log(2.0) * theta ** 2 / fwhm_rad[k] ** 2)
    return out.reshape(res.shape)


def answer(unitvec, rot, pc_dircos, baselines, freqs_hz, cube, weights=None, chan_avg=False, aberr_beta=None, gain=0.1, maxiter=10000,
           threshold=5e-3, threshold_relative=True, window=None, fwhm_rad=None):
    """Context.clean_image by the independent CLEAN: its dict, less the statistics."""
    pb = Problem(unitvec, rot, pc_dircos, baselines, freqs_hz, cube, weights=weights, aberr_beta=aberr_beta, chan_avg=chan_avg, window=window)
    r = clean(pb, gain, maxiter, threshold, threshold_relative)
    r['wsum'] = pb.W.copy()
    r['restored'] = None
    if fwhm_rad is not None:
        fw = NP.broadcast_to(NP.asarray(fwhm_rad, dtype=NP.float64), (pb.nc,))
        r['restored'] = restored(r['residual'], unitvec, r['comp_pixel'], r['comp_flux'], r['ncomp'], fw)
    return r
