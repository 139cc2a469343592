"""numpy statement of include/prisim_mosclean.h, TEST INFRASTRUCTURE, built on tests/mosaic_checker.py (the sums and the quotient of
the mosaic, its bounds), tests/imclean_checker.py (the statuses, the restoring beam) and tests/antpower_checker.py (beam_of, by way
of mosaic_checker.beams): an independent CLEAN of the mosaic with its own argmax, and a replay that follows the component lists of
another CLEAN -- the device's -- and rebuilds the sequence of numerators R_N in complex128, every phase from the channel's own
frequency and every beam value from the oracle.

The replay follows the decisions it is given, so two pixels that tie to rounding cannot fail it; it asserts that every decision was
a right one to within the tolerance, so it cannot pass a wrong pick either.

Tolerances.  No constant is new: 1e-11 is the project's bound of an fp64 image sum against its natural scale and 1e-12 the absolute
bound of a device beam value against the oracle (tests/mosaic_checker.py, tests/test_gpu_antpower.py).
  R_N is the mosaic's N of the visibilities V - sum_c A[t][q_c] a_c e^{-i phi_qc}.  The natural scale of snapshot t grows by the
  model's: sum_b w |V_model| <= W_t sum_c |a_c| A[t][q_c], as tests/imclean_checker.py adds sum |a|.  So, per (pixel, channel),
      tol_N = 1e-11 sum_t A[t][p] (sum_b w|V| + W_t sum_c |a_c| A[t][q_c])                            the sums
            + 1e-12 sum_t (sum_b w|V| + W_t sum_c |a_c| (A[t][p] + A[t][q_c]))                        the beams
  the second line being the 1e-12 of a beam value through A[t][p] (times the scale of what it multiplies, as in mosaic_checker's
  bound_num) and through A[t][q_c] (times |a_c| W_t A[t][p] <= |a_c| W_t).  tol_Q is mosaic_checker's bound_den.
  F = N / sqrt(Q W): to first order dF = dN / sqrt(Q W) - N dQ / (2 Q sqrt(Q W)), so
      tol_F = tol_N / sqrt(Q W) + |F| tol_Q / (2 Q)
  and for a = gain N / Q, da = gain (dN / Q - N dQ / Q^2):
      tol_a = gain (tol_N + |N / Q| tol_Q) / Q
  all from the reference's own N, Q and W.  W itself differs between two orders of summation by some nbl 2^-53 of itself, five orders
  below the 1e-11 above, and is not given a term.  With chan_avg, N, Q, W and their tolerances are the sums over the band.
A peak is a maximum over pixels, so where peaks are compared the tolerance is the largest tol_F over the valid pixels of the window.

Input conditions, asserted on the reference alone (Problem.__init__): no direction within 1e-9 of the horizon (mosaic_checker.beams)
and no Q_ref / (pbmin^2 Wtot) within 1e-6 of 1, so that the device masks what the reference masks.  Nothing is skipped."""
import numpy as NP

import imaging_checker as IK
import imclean_checker as CK
import mosaic_checker as MK

BOUND = CK.BOUND                 # 1e-11
BEAM_BOUND = 1e-12               # a device beam value against the oracle, absolute
THRESHOLD, MAXITER, DEAD = CK.THRESHOLD, CK.MAXITER, CK.DEAD


def flat_of(num, den, wsum, pbmin, chan_avg=False):
    """F from N, Q (npix, nchan) and Wtot (nchan,) by the expressions of include/prisim_mosclean.h, the sums over k ascending one
    term at a time (mosaic_checker.quotient's)."""
    num, den, wsum = NP.asarray(num, dtype=NP.float64), NP.asarray(den, dtype=NP.float64), NP.asarray(wsum, dtype=NP.float64)
    if chan_avg:
        n, q, w = NP.zeros(num.shape[0]), NP.zeros(num.shape[0]), 0.0
        for k in range(num.shape[1]):
            n, q, w = n + num[:, k], q + den[:, k], w + wsum[k]
        num, den, wsum = n, q, w
    with NP.errstate(invalid='ignore', divide='ignore'):
        return NP.where(den >= (pbmin * pbmin) * wsum, num / NP.sqrt(den * wsum), NP.nan)


class Problem(object):
    """The phasors, beams and sums of one problem.  E[t][k][p][b] = e^{+i phi}; A (nt, npix, nchan); w, v (nt, nbl, nchan); Wt
    (nt, nchan); Q (npix, nchan).  setups: what mosaic_checker.beams takes.  Image-channel arrays are (npix, nc)."""

    def __init__(self, unitvec, rot, pc_dircos, baselines, freqs_hz, cube, setups, weights=None, aberr_beta=None, chan_avg=False, window=None,
                 pbmin=0.1, share=None):
        bl = NP.asarray(baselines, dtype=NP.float64).reshape(-1, 3)
        fq = NP.asarray(freqs_hz, dtype=NP.float64).ravel()
        self.geometry = (unitvec, rot, pc_dircos, baselines, freqs_hz, aberr_beta)
        if share is None:                                             # share: a Problem of the same geometry and beams
            s = IK.directions(unitvec, rot, aberr_beta)
            pc = NP.asarray(pc_dircos, dtype=NP.float64).reshape(-1, 3)
            tau = NP.einsum('tpi,bi->tpb', s - pc[:, NP.newaxis, :], bl) / IK.C_LIGHT
            self.E = NP.exp(2j * NP.pi * tau[:, NP.newaxis, :, :] * fq[NP.newaxis, :, NP.newaxis, NP.newaxis])      # (nt, nchan, npix, nbl)
            self.A = MK.beams(s, fq, setups)                          # asserts the horizon margin
        else:
            self.E, self.A = share.E, share.A
        self.setups = setups
        self.nt, self.nchan, self.npix, self.nbl = self.E.shape
        assert self.A.shape == (self.nt, self.npix, self.nchan)
        self.weights = weights
        self.w = NP.array(IK.full_weights(weights, self.nt, self.nbl, self.nchan), dtype=NP.float64)
        self.v = NP.asarray(cube, dtype=NP.complex128)
        assert self.v.shape == (self.nt, self.nbl, self.nchan)
        self.chan_avg, self.pbmin = bool(chan_avg), float(pbmin)
        self.nc = 1 if chan_avg else self.nchan
        self.Wt = NP.einsum('tbk->tk', self.w)
        self.Wtot = NP.zeros(self.nchan)
        for t in range(self.nt):
            self.Wtot = self.Wtot + self.Wt[t]
        self.absV = NP.einsum('tbk->tk', self.w * NP.abs(self.v))
        self.Q = NP.zeros((self.npix, self.nchan))
        for t in range(self.nt):
            self.Q = self.Q + self.A[t] * self.A[t] * self.Wt[t][NP.newaxis, :]
        self.tol_Q = BOUND * NP.einsum('tpk,tk->pk', self.A * self.A, self.Wt) + 2 * BEAM_BOUND * NP.einsum('tpk,tk->pk', self.A, self.Wt)
        self.Qc, self.Wc = self.band(self.Q), (NP.array([self.Wtot.sum()]) if chan_avg else self.Wtot)
        self.dead = self.Wc == 0.0
        live = ~self.dead
        with NP.errstate(invalid='ignore', divide='ignore'):
            ratio = self.Qc[:, live] / ((self.pbmin * self.pbmin) * self.Wc[live])[NP.newaxis, :]
        if self.pbmin > 0.0 and ratio.size:
            assert NP.min(NP.abs(ratio - 1.0)) > 1e-6, ('an element on the rim of the mask', float(NP.min(NP.abs(ratio - 1.0))))
        self.valid = NP.zeros((self.npix, self.nc), dtype=bool)
        self.valid[:, live] = self.Qc[:, live] >= ((self.pbmin * self.pbmin) * self.Wc[live])[NP.newaxis, :]
        self.window = NP.ones(self.npix, dtype=bool) if window is None else NP.asarray(window) != 0
        assert self.window.shape == (self.npix,) and self.window.any()
        self.search = self.valid & self.window[:, NP.newaxis] & (self.Qc > 0.0)      # Q == 0 passes pbmin = 0, and its F is 0 / 0

    def band(self, x):
        """(npix, nchan) -> (npix, nc): the sum over the band with chan_avg"""
        return x.sum(axis=1, keepdims=True) if self.chan_avg else x

    def numerator(self, v):
        """N (npix, nchan) of the visibilities v (nt, nbl, nchan): sum_t A_t Re sum_b w v e^{+i phi}"""
        x = NP.transpose(self.w * v, (0, 2, 1))[..., NP.newaxis]                      # (nt, nchan, nbl, 1)
        D = NP.matmul(self.E, x)[..., 0].real                                         # (nt, nchan, npix)
        return NP.einsum('tpk,tkp->pk', self.A, D)

    def component_vis(self, k, q, a):
        """The visibilities of the component (q, a) of image channel k, as the sky-sum simulates them: A[t][q] a e^{-i phi_q},
        (nt, nbl, nchan), zero outside the channel."""
        out = NP.zeros_like(self.v)
        ks = slice(None) if self.chan_avg else slice(k, k + 1)
        out[:, :, ks] = a * NP.transpose(self.A[:, q, ks][:, :, NP.newaxis] * self.E[:, ks, q, :].conj(), (0, 2, 1))
        return out

    def flat(self, RN):
        """F (npix, nc) of the numerator RN, NaN outside the mask"""
        with NP.errstate(invalid='ignore', divide='ignore'):
            return NP.where(self.valid, self.band(RN) / NP.sqrt(self.Qc * self.Wc), NP.nan)

    def peak(self, F):
        """(max over the window and the mask of |F|, its first pixel) per image channel; (-1, -1) where there is none"""
        a = NP.where(self.search & ~NP.isnan(F), NP.abs(F), -1.0)
        q = NP.argmax(a, axis=0)
        peak = a[q, NP.arange(self.nc)]
        return peak, NP.where(peak >= 0.0, q, -1)

    def cost(self, vm):
        """sum w |V - model|^2 per image channel"""
        c = NP.einsum('tbk->k', self.w * NP.abs(self.v - vm) ** 2)
        return NP.array([c.sum()]) if self.chan_avg else c

    def tolerances(self, RN, spent_q, spent, bound=None):
        """(tol_N (npix, nchan), tol_F (npix, nc), the largest tol_F over the searched pixels (nc,)).  spent_q (nt, nchan): the sum over
        the components so far of |a_c| A[t][q_c][k]; spent (nchan,): of |a_c|.  bound: None for BOUND, or a pair of (nt, nchan) arrays
        in its place, the factor of sum_b w|V| and that of the model's scale (tests/mosaic_reference.py derives them)."""
        scale = self.absV + self.Wt * spent_q                                          # (nt, nchan)
        sums = BOUND * NP.einsum('tpk,tk->pk', self.A, scale) if bound is None else \
            NP.einsum('tpk,tk->pk', self.A, bound[0] * self.absV + bound[1] * (self.Wt * spent_q))
        tol_N = sums + \
            BEAM_BOUND * (scale.sum(axis=0)[NP.newaxis, :] + NP.einsum('tpk,tk->pk', self.A, self.Wt * spent[NP.newaxis, :]))
        with NP.errstate(invalid='ignore', divide='ignore'):
            F = self.flat(RN)
            tol_F = self.band(tol_N) / NP.sqrt(self.Qc * self.Wc) + NP.abs(F) * self.band(self.tol_Q) / (2.0 * self.Qc)
        tmax = NP.array([NP.max(tol_F[self.search[:, k], k]) if self.search[:, k].any() else 0.0 for k in range(self.nc)])
        return tol_N, tol_F, tmax

    def tol_flux(self, RN, tol_N, q, k, gain):
        """The tolerance of a = gain N / Q at pixel q of image channel k"""
        n, tn, tq, qq = self.band(RN)[q, k], self.band(tol_N)[q, k], self.band(self.tol_Q)[q, k], self.Qc[q, k]
        return gain * (tn + abs(n / qq) * tq) / qq

    def outputs(self, RN, cp, cf, count, status, peak0):
        residual, pb_eff = MK.quotient(RN, self.Q, self.Wtot, self.pbmin, self.chan_avg)
        return {'residual': residual, 'residual_flat': flat_of(RN, self.Q, self.Wtot, self.pbmin, self.chan_avg), 'pb_eff': pb_eff,
                'num': RN, 'den': self.Q.copy(), 'wsum': self.Wtot.copy(), 'comp_pixel': cp, 'comp_flux': cf, 'ncomp': count,
                'status': status, 'peak0': peak0}


def _lists(nc, pix, flux):
    count = NP.array([len(x) for x in pix], dtype=NP.int32)
    longest = int(count.max()) if nc else 0
    cp, cf = NP.full((nc, longest), -1, dtype=NP.int32), NP.zeros((nc, longest))
    for k in range(nc):
        cp[k, :count[k]], cf[k, :count[k]] = pix[k], flux[k]
    return cp, cf, count


def clean(pb, gain, maxiter, threshold, relative, costs=None):
    """The independent CLEAN: every channel in step, numpy's own argmax.  Returns the dict of the device's outputs.  costs: a list
    that receives sum w |V - model|^2 per image channel before the first component and behind every iteration."""
    RN = pb.numerator(pb.v)
    nc = pb.nc
    peak0, _ = pb.peak(pb.flat(RN))
    peak0 = NP.where(peak0 >= 0.0, peak0, NP.nan)
    thr = threshold * peak0 if relative else NP.full(nc, float(threshold))
    status = NP.where(pb.dead, DEAD, 0).astype(NP.int32)
    pix, flux = [[] for _ in range(nc)], [[] for _ in range(nc)]
    vm = NP.zeros_like(pb.v)
    if costs is not None:
        costs.append(pb.cost(vm))
    while NP.any(status == 0):
        peak, q = pb.peak(pb.flat(RN))
        step = NP.zeros_like(pb.v)
        for k in NP.flatnonzero(status == 0):
            if q[k] < 0 or not peak[k] > thr[k]:
                status[k] = THRESHOLD
            elif len(pix[k]) >= maxiter:
                status[k] = MAXITER
            else:
                a = gain * (pb.band(RN)[q[k], k] / pb.Qc[q[k], k])
                pix[k].append(int(q[k]))
                flux[k].append(a)
                step += pb.component_vis(k, int(q[k]), a)
        if NP.any(step != 0.0):
            RN = RN - pb.numerator(step)
            vm += step
            if costs is not None:
                costs.append(pb.cost(vm))
    cp, cf, count = _lists(nc, pix, flux)
    return pb.outputs(RN, cp, cf, count, status, peak0)


def replay(pb, got, gain, maxiter, threshold, relative, bound=None):
    """Follows the lists of `got` (the dict of Context.clean_mosaic, or of clean()) and asserts every decision and the results.
    Returns the largest deviation met, as a fraction of its tolerance.  bound: what Problem.tolerances takes."""
    nc, npix = pb.nc, pb.npix
    cp, cf, count, status = (NP.asarray(got[n]) for n in ('comp_pixel', 'comp_flux', 'ncomp', 'status'))
    assert cp.shape == cf.shape and cp.shape[0] == nc and count.shape == (nc,) and status.shape == (nc,)
    assert cp.shape[1] == (int(count.max()) if nc else 0) and NP.all(count >= 0) and NP.all(count <= maxiter)
    assert NP.array_equal(status == DEAD, pb.dead) and NP.all(count[pb.dead] == 0), 'the channels without weight, and they alone, are dead'
    assert NP.all(NP.isin(status, (THRESHOLD, MAXITER, DEAD)))
    live = ~pb.dead
    empty = live & ~pb.search.any(axis=0)                             # nothing to search: THRESHOLD at once, a NaN P0
    RN = pb.numerator(pb.v)
    spent_q, spent = NP.zeros((pb.nt, pb.nchan)), NP.zeros(pb.nchan)
    worst = 0.0

    def note(dev, t):
        nonlocal worst
        dev, t = NP.asarray(dev, dtype=NP.float64), NP.asarray(t, dtype=NP.float64)
        if dev.size:
            with NP.errstate(invalid='ignore', divide='ignore'):
                worst = max(worst, float(NP.max(NP.where(t > 0.0, dev / t, NP.where(dev > 0.0, NP.inf, 0.0)))))

    tol_N, tol_F, tmax = pb.tolerances(RN, spent_q, spent, bound)
    peak0, _ = pb.peak(pb.flat(RN))
    got0 = NP.asarray(got['peak0'], dtype=NP.float64)
    seen = live & ~empty
    assert NP.all(NP.isnan(got0[~seen])) and NP.all(NP.abs(got0[seen] - peak0[seen]) <= tmax[seen]), ('P0', got0, peak0, tmax)
    note(NP.abs(got0[seen] - peak0[seen]), tmax[seen])
    assert NP.all(count[empty] == 0) and NP.all(status[empty] == THRESHOLD), 'a channel with nothing to search ends at the threshold at once'
    # the threshold the other CLEAN compared with came from its own P0
    thr = threshold * got0 if relative else NP.full(nc, float(threshold))
    vm = NP.zeros_like(pb.v)
    for i in range(cp.shape[1] + 1):
        F = pb.flat(RN)
        peak, _ = pb.peak(F)
        tol_N, tol_F, tmax = pb.tolerances(RN, spent_q, spent, bound)
        going = NP.flatnonzero(seen & (count > i))
        for k in NP.flatnonzero(seen & (count == i)):
            if status[k] == THRESHOLD:
                assert peak[k] <= thr[k] + 2 * tmax[k], ('a stop at the threshold above it', k, i, peak[k], thr[k], tmax[k])
                note(max(peak[k] - thr[k], 0.0), 2 * tmax[k])
            else:
                assert status[k] == MAXITER and count[k] == maxiter, ('a stop that is neither', k, i, status[k])
                assert peak[k] >= thr[k] - 2 * tmax[k], ('a stop at maxiter below the threshold', k, i, peak[k], thr[k], tmax[k])
        if not going.size:
            continue
        qs, fl = cp[going, i], cf[going, i]
        assert NP.all((qs >= 0) & (qs < npix)) and NP.all(pb.window[qs]), ('a pick outside the window', i)
        assert NP.all(pb.valid[qs, going]), ('a pick on a masked pixel', i, qs, going)
        at = F[qs, going]
        assert NP.all(NP.abs(at) >= peak[going] - 2 * tmax[going]), ('a pick that is not the peak', i, going, NP.abs(at), peak[going])
        assert NP.all(peak[going] >= thr[going] - 2 * tmax[going]), ('a continuation below the threshold', i)
        note(peak[going] - NP.abs(at), 2 * tmax[going])
        step = NP.zeros_like(pb.v)
        for k, q, a in zip(going, qs, fl):
            want = gain * (pb.band(RN)[q, k] / pb.Qc[q, k])
            ta = pb.tol_flux(RN, tol_N, q, k, gain)
            assert abs(a - want) <= ta, ('a flux that is not gain * R_N[q] / Q[q]', i, k, a, want, ta)
            note(abs(a - want), ta)
            step += pb.component_vis(k, int(q), a)
        RN = RN - pb.numerator(step)
        vm += step
        for k, q, a in zip(going, qs, fl):
            ks = slice(None) if pb.chan_avg else slice(k, k + 1)
            spent_q[:, ks] += abs(a) * pb.A[:, q, ks]
            spent[ks] += abs(a)
    tol_N, _, _ = pb.tolerances(RN, spent_q, spent, bound)
    num, den, wsum = (NP.asarray(got[n], dtype=NP.float64) for n in ('num', 'den', 'wsum'))
    assert num.shape == den.shape == (npix, pb.nchan) and wsum.shape == (pb.nchan,)
    dev = NP.abs(num - RN)
    assert NP.all(dev <= tol_N), ('the numerator against the replay', float(NP.max(dev / tol_N)))
    note(dev, tol_N)
    # linearity, by the mosaic's own checker: R_N is the mosaic's numerator of the visibilities less those of the model
    u, rot, pc, bl, fq, beta = pb.geometry
    sums = MK.snapshot_sums(u, rot, pc, bl, fq, pb.v - vm, weights=pb.weights, aberr_beta=beta)
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
    for name, want in (('residual', residual), ('pb_eff', pb_eff), ('residual_flat', flat_of(num, den, wsum, pb.pbmin, pb.chan_avg))):
        have = NP.asarray(got[name], dtype=NP.float64)
        assert have.shape == want.shape and NP.array_equal(have, want, equal_nan=True), name
    masked = NP.isnan(NP.asarray(got['residual_flat'], dtype=NP.float64)).reshape(npix, nc)
    assert NP.array_equal(masked[:, live], (~pb.valid | (pb.Qc == 0.0))[:, live]) and NP.all(masked[:, pb.dead]), 'the mask is the reference\'s'
    return worst


def response(pb, q, k=0):
    """A unit component at pixel q of image channel k: (N_c (npix, nc), its flat-noise response |F_c| (npix, nc) with the mask lifted,
    the normalised response |N_c[p]| / sqrt(Q[p] Q[q]) (npix, nc)) -- the last two in column k alone where nc > 1."""
    Nc = pb.band(pb.numerator(pb.component_vis(k, q, 1.0)))
    with NP.errstate(invalid='ignore', divide='ignore'):
        return Nc, NP.abs(Nc) / NP.sqrt(pb.Qc * pb.Wc), NP.abs(Nc) / NP.sqrt(pb.Qc * pb.Qc[q][NP.newaxis, :])


def answer(unitvec, rot, pc_dircos, baselines, freqs_hz, cube, setups, weights=None, chan_avg=False, aberr_beta=None, pbmin=0.1, gain=0.1,
           maxiter=10000, threshold=5e-3, threshold_relative=True, window=None, fwhm_rad=None):
    """Context.clean_mosaic by the independent CLEAN: its dict, less the statistics."""
    pb = Problem(unitvec, rot, pc_dircos, baselines, freqs_hz, cube, setups, weights=weights, aberr_beta=aberr_beta, chan_avg=chan_avg,
                 window=window, pbmin=pbmin)
    r = clean(pb, gain, maxiter, threshold, threshold_relative)
    r['restored'] = None
    if fwhm_rad is not None:
        fw = NP.broadcast_to(NP.asarray(fwhm_rad, dtype=NP.float64), (pb.nc,))
        r['restored'] = CK.restored(r['residual'], unitvec, r['comp_pixel'], r['comp_flux'], r['ncomp'], fw)
    return r
