"""40-digit reference of the beam-weighted mosaic and of the minor-cycle beam P of the Cotton-Schwab CLEANs (TEST INFRASTRUCTURE).

What include/prisim_mosaic.h and include/prisim_csclean.h state, for pixel p, channel k, snapshot t and baseline b:
    N[p][k] = sum_t A[t][p][k] D_t[p][k],   Q[p][k] = sum_t A[t][p][k]^2 W_t[k],   Wtot[k] = sum_t W_t[k],   mosaic = N / Q under the mask
    D_t = sum_b w (Re V cos phi - Im V sin phi) of tests/imaging_reference.py, one snapshot at a time;  A = 0 below the horizon
    rho = (u[ny-1][nx/2] - u[0][nx/2]) / (ny - 1),   kappa = (u[ny/2][nx-1] - u[ny/2][0]) / (nx - 1),   delta = di rho + dj kappa
    P[k][di][dj] = sum_{t,b} w cos(2 pi f_k b . (rot_t delta) / c) / W[k]       (the band's sums over the band's W with chan_avg)
This module shares no code with prisim_amd, oracle/ or the numpy checkers.  It builds on tests/imaging_reference.py (the 60-digit
directions, the exact reduction of every phase modulo one cycle through skyvis_reference.frac_cycles, the seeded cases) and on
tests/beam_reference.py (power, Spec, Ground), and like them it needs mpmath and an x87 long double.

Beams.  A_ref[t][p][k] = beam_reference.power(spec, geo.s[t], freqs): the 40-digit beam at the reference's own directions, the 60-digit
directions rounded to doubles.  That rounding is immaterial to a beam value: it moves a direction cosine by at most u = 2^-53 = 1.1e-16,
and the steepest beam here, the 6 m Gaussian at 153 MHz (sigma = 0.12 in direction cosines, power exp(-sin^2 / sigma^2)), changes by at
most 0.86 / 0.12 = 7 per unit of direction cosine, the 6 m Airy pattern by less: 8e-16, a thousandth of the 1e-12 the device's beam is
held to.  (mosaic_terms_mp(unrounded_beam=True) states the Gaussian and the Airy pattern on the UNROUNDED directions; the CPU test holds
A_ref to it within 1e-15.)  The horizon mask is the sign of the 60-digit s_z; no case may have |s_z| < 1e-9 (asserted), so no rounding
can decide it otherwise.
Dishes of 2 m and 6 m, Gaussian and Airy, and the 0.74 m dipole 0.3 m over a ground plane of tests/mosaic_cases.py (SPECS).

Sums.  D_t, W_t, sum_b w|V|, the products with A_ref and A_ref^2 and the sums over t are numpy.longdouble, rounded to float64 at the end.

Two routes, as in imaging_reference: the route above, and one that forms every term of a seeded sub-sample of the outputs in mpmath
from unrounded values (N, Q: mosaic_terms_mp; P: lattice_terms_mp).  tests/test_mosaic_reference.py holds the second to the first
within imaging_reference.ROUTE_GAP = 1e-17 of the scale.  Measured 2026-10-21 on x86-64: see MEASURED below.

THE RULES, u = 2^-53; every length term is COUNTED from the cited lines, none is fitted; the project's bars are kept as they are: 1e-11
of the natural scale for an fp64 image sum, 1e-12 absolute for a device beam value, 1e-12 for P (tests/moscs_checker.PSF_BOUND).

  tol_N[p][k] = sum_t bound_t[k] A_ref[t][p][k] sum_b w|V| + 1e-12 sum_{t,b} w|V|
  tol_Q[p][k] = 1e-11 sum_t A_ref^2 W_t + 2e-12 sum_t A_ref W_t
      the shape of mosaic_checker's bound_num and bound_den.  bound_t = imaging_reference.bound(geometry of snapshot t, freqs, route): the
      image's own rule (R_DIR on N_b, the phase chain on N' of that snapshot), because k_mos_sum (prisim_amd/csrc_imaging/
      mosaic_kernels.h:68) runs img_tile_pass on the dd of k_img_dirs as k_img_sum does.  The epilogue adds one FMA per snapshot
      (mosaic_kernels.h:81-82): nt u of the scale, inside the 1e-11.  Q has no phase in it: W_t is a sum of nbl weights
      (mosaic_kernels.h:29), A A one product, so its 1e-11 stays flat.  The beam is evaluated by the device at ITS directions, off the
      reference's by R_DIR u <= 1.5e-15: times the gradient above, 1e-14, inside the 1e-12 of a beam value.
  fp32 entries: |N - N_ref| <= 5e-6 sum_t A_ref sum_b w|V| + 1e-12 sum_{t,b} w|V|, and |image - ref| <= 5e-6 scale_k for the dirty image;
      den, wsum: the fp64 rule.

  P, direct:   |P - P_ref| <= 1e-12 + 2 pi u (R_OFF + R_PH_P) N_delta[k]
  P, stepped:  |P - P_ref| <= 1e-12 + 2 pi u ((R_OFF + R_PH_P) N_delta[k] + N_delta[k0]) + 2 pi grid_gap tau_max,  band: the largest factor
      N_delta[k] = f_k max_{t,b,di,dj} sum_i |b_i| sum_j |R_t,ij| (|di| |rho_j| + |dj| |kappa_j|) / c
      that is f_k max sum_i |b_i| |(rot_t delta)_i| / c with the absolute values taken term by term: the 1-norm bound of the partial
      sums the roundings act on (a rounding on di rho_j is u |di rho_j| whatever dj kappa_j cancels of it).  It is at most 1.8 times the
      literal expression on the lattices used (printed by the CPU test).
      R_OFF = 7, the offset chain:
        2   rho_j = (u_a - u_b) / (ny - 1): the difference and the division, each on its own term (kappa alike) cycle_kernels.h:283-284
        1   the products di rho_j and dj kappa_j, each rounds its own term                                           cycle_kernels.h:71
        1   their sum                                                                                               cycle_kernels.h:71
        3   (R_i0 t_0 + R_i1 t_1) + R_i2 t_2: the three products a term each, the two sums a partial sum each        cycle_kernels.h:73-74
      R_PH_P = 6, the phase chain after it: imaging_reference's R_PH_TAU without d = s - s0 (the offset IS d: cycle_kernels.h:303 hands dd
        to the dirty image's kernel, kind PSF), 5, and the product f_k tau, 1; stepped: the seed's product acts on N_delta[k0] and the step's
        product replaces f_k tau, as in imaging_reference.
  WHERE P LOSES ACCURACY.  On N_delta, NOT on the whole baseline N_b: nothing in the chain of P is ever as large as a unit vector.  The
      difference u_a - u_b is the first operation, on doubles the reference takes exactly, and it rounds relative to the DIFFERENCE (for a
      narrow lattice it is exact, Sterbenz); every later rounding is relative to an offset or to b . delta.  The image's directions go
      through a normalisation of a vector of length 1 and lose u N_b; P does not.  Asserted both ways on the lattice whose half-widths
      are divided by the scale (N_delta stays 90 cycles while N_b grows to 1.8e6): the float64 restatement of the device's chain stays
      inside the rule on N_delta, and BELOW a hundredth of 2 pi u N_b, where the image on its narrow field sits at 0.16 to 0.24 of it.

  CLEAN of the mosaic, per pick both chains count, as imaging_reference.update_bound: the factor of sum |a| is update_bound of the
      snapshot.  Cotton-Schwab replays (csclean_checker.replay(bound=...)): the factor of the scale is imaging_reference.bound, that of
      sum |a| imaging_reference.update_bound (the model visibilities carry the pick's chain, the residual image the pixel's), and the
      minor cycles run on P_ref, whose distance from the device's P (the P rule) is below update_bound on every lattice used (asserted).

MEASURED 2026-10-21 on x86-64 (tests/test_mosaic_reference.py prints them):
    route gap: N 7.7e-20 of its scale, Q 5.1e-20 of Wtot, P 3.1e-20; the 2 m and 6 m beams at unrounded directions within 3.8e-17 of A_ref.
    FLOOR of tests/mosaic_checker.py, worst |N - N_ref| over its own bound_num, (33, 33, 65, 2), Airy 2 m, w_full, sphere | narrow:
        300 m 0.0022 | 0.0020    3 km 0.023 | 0.018    30 km 0.29 | 0.22    300 km 2.3 | 2.1    2400 km 17 | 13       (Q: 3e-4 of tol_Q)
      inside its bar up to 30 km, outside from 300 km on (CHECKER_KEEPS / CHECKER_LOSES of imaging_reference, asserted both ways).
    FLOOR of csclean_checker.beam on the lattice as it is (N_delta 88 cycles at 300 m), per channel | band:
        300 m 8.6e-15 | 3.1e-15    3 km 8.3e-14 | 5.3e-15    30 km 1.0e-12 | 1.2e-13    300 km 9.9e-12 | 1.6e-12    2400 km 8.4e-11 | 7.2e-12
      0.14 to 0.17 of 2 pi u N_delta: inside 1e-12 to 3 km, on it at 30 km (asserted neither way), outside from 300 km (asserted).
    the float64 restatement of the device, both routes: N at most 0.018 of tol_N, Q 6e-5 of tol_Q on every decade; P at most 0.012 of its rule on
      the lattice as it is (9.9e-15 at 300 m ... 6.4e-11 at 2400 km, 0.05 to 0.06 of 2 pi u N_b because N_delta is 0.4 N_b there), and on
      the shrunk lattices 8.0e-15 at 300 km and 6.2e-15 at 2400 km: 5e-5 and 5e-6 of 2 pi u N_b, where the restated image on its narrow
      field is at 0.20 of it.  N_delta is 1.33 times its literal form on every lattice.
    wrong restatements: delta not rotated, rho over ny, the mirror at (di, -dj): 5e8 to 3e11 times the rule of P; A to the first power in
      Q: 5e11 times tol_Q; no horizon mask: 2e11 times tol_N.

ON THE MI355X (tests/test_gpu_mosaic_reference.py, 2026-10-21), the largest share of each bound per decade, 300 m | 30 km | 300 km | 2400 km:
    mosaic N (fp64)        0.009 | 0.018 | 0.086 | 0.014 of tol_N          Q below 1e-3 of tol_Q on every decade
    mosaic N, dirty image and PSF (fp32)      -- | -- | 0.173 | 0.041 of 5e-6 of the natural scale
    prisim_clean_mosaic, the replay           0.001 | 0.009 | 0.009 | 0.010 of its tolerance
    P                      9.9e-15, 0.006 of its rule at 300 m; 9.3e-12, 0.012 at 300 km on the lattice as it is; 7.9e-15, 0.004 and
                           6.3e-15, 0.003 on the shrunk lattices at 300 km and 2400 km: the device is the restatement to two digits
    prisim_clean_image_cs, the replay         0.002 | -- | 0.010 | 0.007        prisim_clean_mosaic_cs   0.006 | -- | 0.020 | 0.019
The 43 GPU tests of that file take 15 s together.  No kernel had to change.
"""
import collections
import functools
import types

import numpy as NP

import beam_reference as BR
import imaging_cases as IC
import imaging_reference as R
import skyvis_reference as SR

LD = NP.longdouble
MP = R.MP
U = R.U
C_LIGHT = R.C_LIGHT
BEAM_BAR = BR.BOUND                                        # 1e-12 absolute: a device beam value
P_BAR = 1e-12                                              # the flat term of P (tests/moscs_checker.PSF_BOUND, test_gpu_csclean.py)
F32_BAR = 5e-6
R_OFF = 7
R_PH_P = R.R_PH_TAU - 1 + 1
HORIZON_MARGIN = 1e-9
MASK_MARGIN = 1e-6
PBMIN = 0.1
ROUTE_GAP = R.ROUTE_GAP
SCALES = R.SCALES
CHECKER_KEEPS, CHECKER_LOSES = R.CHECKER_KEEPS, R.CHECKER_LOSES

SPECS = {'gaussian': BR.Spec('gaussian', 2.0), 'airy': BR.Spec('airy', 2.0), 'gaussian6': BR.Spec('gaussian', 6.0), 'airy6': BR.Spec('airy', 6.0),
         'dipole_ground': BR.Spec('dipole', 0.74, dipole_axis=(1.0, 0.0, 0.0), ground=BR.Ground(0.3))}

Mosaic = collections.namedtuple('Mosaic', 'num den wsum wt absV A up scale_N num_ld den_ld D_ld')
Lattice = collections.namedtuple('Lattice', 'P P_ld Nd Nd_literal Nb tau_max W')


def _weights(weights, nt, nbl, nchan):
    if weights is None:
        return NP.ones((nt, nbl, nchan), dtype=LD)
    w = NP.asarray(weights, dtype=NP.float64)
    return NP.broadcast_to(w[None, :, None] if w.shape == (nbl,) else w, (nt, nbl, nchan)).astype(LD)


# ---- the beams -------------------------------------------------------------------------------------------------------------------------
def horizon(unitvec, rot, beta, pc):
    """up (nt, npix) from the sign of the 60-digit s_z, and min |s_z|."""
    sd = R.directions_mp(unitvec, rot, beta, pc)
    z = [[row[0][2] for row in snap] for snap in sd]
    up = NP.array([[bool(v >= 0) for v in snap] for snap in z])
    return up, float(min(abs(v) for snap in z for v in snap))


def beams(geo, up, spec, freqs, pointing=None):
    """A_ref (nt, npix, nchan) longdouble: beam_reference.power at geo.s[t], 0 where the 60-digit direction is below the horizon.
    pointing: None for the spec's own, (3,) or (nt, 3)."""
    nt = geo.s.shape[0]
    A = []
    for t in range(nt):
        sp = spec
        if pointing is not None:
            sp = spec._replace(pointing=tuple(float(x) for x in NP.broadcast_to(NP.asarray(pointing, dtype=NP.float64).reshape(-1, 3), (nt, 3))[t]))
        pw, blank, _ = BR.power(sp, geo.s[t], freqs)
        assert NP.all(NP.isfinite(pw)) and NP.all(pw[blank] == 0)
        A.append(NP.where(up[t][:, None], pw, LD(0)))
    return NP.stack(A)


def mosaic(geo, A, cube, weights):
    """Mosaic of the cube (nt, nbl, nchan) through A (nt, npix, nchan): every sum in longdouble, rounded at the end."""
    nt, npix, nbl, nchan = geo.cos.shape
    w = _weights(weights, nt, nbl, nchan)
    v = NP.asarray(cube, dtype=NP.complex128).reshape(nt, nbl, nchan)
    re, im = v.real.astype(LD), v.imag.astype(LD)
    wre, wim = w * re, w * im
    D = NP.sum(wre[:, None] * geo.cos - wim[:, None] * geo.sin, axis=2)              # (nt, npix, nchan)
    Wt = NP.sum(w, axis=1)                                                            # (nt, nchan)
    absV = NP.sum(w * NP.sqrt(re * re + im * im), axis=1)
    num, den = NP.sum(A * D, axis=0), NP.sum(A * A * Wt[:, None, :], axis=0)
    f = lambda a: NP.asarray(a).astype(NP.float64)                      # noqa: E731
    return Mosaic(f(num), f(den), f(Wt.sum(axis=0)), f(Wt), f(absV), f(A), None, f(NP.sum(A * absV[:, None, :], axis=0)), num, den, D)


def snapshot_bounds(geo, baselines, freqs, route, update=False):
    """imaging_reference.bound -- update: update_bound -- of every snapshot's own geometry, (nt, nchan)."""
    bl = NP.asarray(baselines, dtype=NP.float64).reshape(-1, 3)
    fq = NP.asarray(freqs, dtype=NP.float64).ravel()
    out = []
    for t in range(geo.d.shape[0]):
        np1 = float(NP.max(NP.einsum('bi,pi->pb', NP.abs(bl), NP.abs(geo.d[t]))))
        g = R.Geometry(None, None, None, None, None, geo.Nb, fq * np1 / C_LIGHT, np1 / C_LIGHT)
        out.append(R.update_bound(g, fq, route) if update else R.bound(g, fq, route))
    return NP.stack(out)


def tolerances(ref, bounds):
    """(tol_N, tol_Q) (npix, nchan) of THE RULES from a Mosaic and snapshot_bounds()."""
    tol_n = NP.einsum('tk,tpk,tk->pk', bounds, ref.A, ref.absV) + BEAM_BAR * ref.absV.sum(axis=0)[None, :]
    tol_q = R.BAR * NP.einsum('tpk,tk->pk', ref.A * ref.A, ref.wt) + 2 * BEAM_BAR * NP.einsum('tpk,tk->pk', ref.A, ref.wt)
    return tol_n, tol_q


def mask_ratio(ref, pbmin, chan_avg=False):
    """Q_ref / (pbmin^2 Wtot) per element, of the band with chan_avg, from the longdouble sums."""
    den, w = ref.den_ld, ref.wt.astype(LD).sum(axis=0)
    if chan_avg:
        den, w = den.sum(axis=1), w.sum()
    return (den / (LD(pbmin) * LD(pbmin) * w)).astype(NP.float64)


def _beam_mp(spec, s, f):
    """The Gaussian or Airy power at the mpmath direction s (zenith pointing is not assumed) and frequency f, from unrounded values."""
    p = [MP.mpf(float(v)) for v in spec.pointing]
    cr = (s[1] * p[2] - s[2] * p[1], s[2] * p[0] - s[0] * p[2], s[0] * p[1] - s[1] * p[0])
    sinx = MP.sqrt(cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2])
    if s[0] * p[0] + s[1] * p[1] + s[2] * p[2] <= 0 or s[2] <= 0:
        return MP.mpf(0)
    f = MP.mpf(float(f))
    if spec.kind == 'gaussian':
        sigma = 1 / (2 * MP.pi * (MP.mpf(float(spec.size)) / (2 * MP.sqrt(2 * MP.log(2))) * f / C_LIGHT))
        return MP.exp(-(sinx / sigma) ** 2)
    half, tol = MP.pi * f / C_LIGHT * MP.mpf(float(spec.size)), MP.sin(MP.mpf(1e-10))
    airy = lambda a: 2 * MP.besselj(1, a) / a                          # noqa: E731
    return (airy(half * max(sinx, tol)) / airy(half * tol)) ** 2


def mosaic_terms_mp(c, spec, weights, outputs, unrounded_beam=False, pointing=None):
    """[(N, Q, [A_t])] in mpmath for the (p, k) of `outputs`: every phase, product and sum from the unrounded directions.  The beam is
    A_ref's own value, at the rounded directions as the reference is defined; unrounded_beam (the dishes): at the unrounded ones, by a
    statement of the Gaussian and the Airy pattern of its own, which measures what that rounding is worth.  pointing: as beams() takes it."""
    bl = NP.asarray(c['baselines'], dtype=NP.float64).reshape(-1, 3)
    fq = NP.asarray(c['freqs'], dtype=NP.float64).ravel()
    sd = R.directions_mp(c['unitvec'], c['rot'], c['beta'], c['pc'])
    nt, nbl, nchan = len(sd), bl.shape[0], fq.size
    w = _weights(weights, nt, nbl, nchan).astype(NP.float64)
    v = NP.asarray(c['cube'], dtype=NP.complex128)
    bm = [[MP.mpf(float(x)) for x in row] for row in bl]
    res = []
    for p, k in outputs:
        f, n, q, beam = MP.mpf(float(fq[k])), MP.mpf(0), MP.mpf(0), []
        for t in range(nt):
            s, d = sd[t][p]
            sp = spec if pointing is None else spec._replace(pointing=tuple(float(x) for x in NP.broadcast_to(NP.asarray(pointing, dtype=NP.float64).reshape(-1, 3), (nt, 3))[t]))
            if unrounded_beam:
                a = _beam_mp(sp, s, fq[k])
            else:
                a = SR.ld_to_mp(BR.power(sp, NP.array([[float(x) for x in s]]), fq[k:k + 1])[0][0, 0]) if s[2] >= 0 else MP.mpf(0)
            acc, wt = MP.mpf(0), MP.mpf(0)
            for b in range(nbl):
                x = 2 * f * (bm[b][0] * d[0] + bm[b][1] * d[1] + bm[b][2] * d[2]) / C_LIGHT
                wv = MP.mpf(float(w[t, b, k]))
                acc += wv * (MP.mpf(float(v[t, b, k].real)) * MP.cospi(x) - MP.mpf(float(v[t, b, k].imag)) * MP.sinpi(x))
                wt += wv
            n += a * acc
            q += a * a * wt
            beam.append(a)
        res.append((n, q, beam))
    return res


def sample(shape, nsample=12, seed=0):
    """A seeded sub-sample of the index tuples of `shape`, the corners always."""
    rng = NP.random.default_rng(seed)
    outs = {tuple(0 for _ in shape), tuple(n - 1 for n in shape)}
    while len(outs) < min(nsample, int(NP.prod(shape))):
        outs.add(tuple(int(rng.integers(n)) for n in shape))
    return sorted(outs)


# ---- the lattice beam --------------------------------------------------------------------------------------------------------------------
def lattice_steps_mp(unitvec, ny, nx):
    """(rho, kappa) as lists of three mpmath numbers: the unit vectors exactly as the doubles they are, the difference and the division
    at 60 digits."""
    u = NP.asarray(unitvec, dtype=NP.float64).reshape(ny, nx, 3)
    mp = lambda x: MP.mpf(float(x))                                     # noqa: E731
    rho = [(mp(u[ny - 1, nx // 2, i]) - mp(u[0, nx // 2, i])) / (ny - 1) if ny > 1 else MP.mpf(0) for i in range(3)]
    kappa = [(mp(u[ny // 2, nx - 1, i]) - mp(u[ny // 2, 0, i])) / (nx - 1) if nx > 1 else MP.mpf(0) for i in range(3)]
    return rho, kappa


def half_plane(ny, nx):
    return [(di, dj) for di in range(0, ny) for dj in range(-(nx - 1), nx) if di > 0 or dj >= 0]


def lattice_offsets_mp(unitvec, rot, ny, nx):
    """[t][h] -> rot_t (di rho + dj kappa) as three mpmath numbers, h over half_plane(ny, nx)."""
    rho, kappa = lattice_steps_mp(unitvec, ny, nx)
    rot = NP.asarray(rot, dtype=NP.float64).reshape(-1, 3, 3)
    out = []
    for t in range(rot.shape[0]):
        Rm = [[MP.mpf(float(rot[t, i, j])) for j in range(3)] for i in range(3)]
        row = []
        for di, dj in half_plane(ny, nx):
            dl = [di * rho[j] + dj * kappa[j] for j in range(3)]
            row.append([Rm[i][0] * dl[0] + Rm[i][1] * dl[1] + Rm[i][2] * dl[2] for i in range(3)])
        out.append(row)
    return out


def lattice_lengths(unitvec, rot, baselines, freqs, ny, nx):
    """(N_delta (nchan,), its literal form, N_b, tau_max): see THE RULES."""
    rho, kappa = (NP.array([float(x) for x in v]) for v in lattice_steps_mp(unitvec, ny, nx))
    rot = NP.asarray(rot, dtype=NP.float64).reshape(-1, 3, 3)
    bl = NP.abs(NP.asarray(baselines, dtype=NP.float64).reshape(-1, 3))
    fq = NP.asarray(freqs, dtype=NP.float64).ravel()
    hp = NP.array(half_plane(ny, nx), dtype=NP.float64)
    a = NP.abs(hp[:, :1]) * NP.abs(rho) + NP.abs(hp[:, 1:]) * NP.abs(kappa)                 # (h, 3)
    m = NP.einsum('tij,hj->thi', NP.abs(rot), a)
    lit = NP.abs(NP.einsum('tij,hj->thi', rot, hp[:, :1] * rho + hp[:, 1:] * kappa))
    n1, n0 = float(NP.max(NP.einsum('bi,thi->thb', bl, m))), float(NP.max(NP.einsum('bi,thi->thb', bl, lit)))
    return fq * n1 / C_LIGHT, fq * n0 / C_LIGHT, fq * float(NP.max(bl.sum(axis=1))) / C_LIGHT, n1 / C_LIGHT


def lattice_beam(unitvec, rot, baselines, freqs, ny, nx, weights=None, chan_avg=False):
    """Lattice: P (nc, 2 ny - 1, 2 nx - 1) rounded to float64 and in longdouble, N_delta, N_b, tau_max, W."""
    bl = NP.ascontiguousarray(baselines, dtype=NP.float64).reshape(-1, 3)
    fq = NP.ascontiguousarray(freqs, dtype=NP.float64).ravel()
    off = lattice_offsets_mp(unitvec, rot, ny, nx)
    nt, nh, nbl, nchan = len(off), len(off[0]), bl.shape[0], fq.size
    D = NP.empty((nt, nh, 3), dtype=object)
    for t in range(nt):
        for h in range(nh):
            for i in range(3):
                D[t, h, i] = int(MP.nint(MP.ldexp(off[t][h][i], R.DIR_BITS)))
    B, kb = SR.ints(bl)
    F, kf = SR.ints(fq)
    M = D[:, :, None, 0] * B[None, None, :, 0] + D[:, :, None, 1] * B[None, None, :, 1] + D[:, :, None, 2] * B[None, None, :, 2]
    w = _weights(weights, nt, nbl, nchan)
    num = NP.empty((nchan, nh), dtype=LD)
    for k in range(nchan):                                              # a channel at a time keeps the integers small in memory
        frac = SR.frac_cycles(M * F[k], kb + kf + R.DIR_BITS)          # (nt, nh, nbl)
        cos = NP.where(NP.abs(frac) == LD(0.25), LD(0), NP.cos(frac * R._two_pi()))
        num[k] = NP.sum(w[:, None, :, k] * cos, axis=(0, 2))
    W = NP.sum(w, axis=(0, 1))
    half = (num.sum(axis=0, keepdims=True) / W.sum()) if chan_avg else num / W[:, None]
    nc = half.shape[0]
    P = NP.empty((nc, 2 * ny - 1, 2 * nx - 1), dtype=LD)
    for h, (di, dj) in enumerate(half_plane(ny, nx)):
        P[:, ny - 1 + di, nx - 1 + dj] = half[:, h]
        P[:, ny - 1 - di, nx - 1 - dj] = half[:, h]
    nd, lit, nb, tau = lattice_lengths(unitvec, rot, bl, fq, ny, nx)
    return Lattice(P.astype(NP.float64), P, nd, lit, nb, tau, W.astype(NP.float64))


def lattice_terms_mp(unitvec, rot, baselines, freqs, ny, nx, weights, chan_avg, outputs):
    """[P[k][di][dj]] in mpmath for the (k, di + ny - 1, dj + nx - 1) of `outputs`, every term from unrounded values."""
    bl = NP.asarray(baselines, dtype=NP.float64).reshape(-1, 3)
    fq = NP.asarray(freqs, dtype=NP.float64).ravel()
    rho, kappa = lattice_steps_mp(unitvec, ny, nx)
    rot = NP.asarray(rot, dtype=NP.float64).reshape(-1, 3, 3)
    nt, nbl, nchan = rot.shape[0], bl.shape[0], fq.size
    w = _weights(weights, nt, nbl, nchan).astype(NP.float64)
    res = []
    for k, i, j in outputs:
        di, dj = i - (ny - 1), j - (nx - 1)
        dl = [di * rho[a] + dj * kappa[a] for a in range(3)]
        acc, wt = MP.mpf(0), MP.mpf(0)
        for kk in (range(nchan) if chan_avg else (k,)):
            f = MP.mpf(float(fq[kk]))
            for t in range(nt):
                rd = [sum(MP.mpf(float(rot[t, a, b])) * dl[b] for b in range(3)) for a in range(3)]
                for b in range(nbl):
                    x = 2 * f * sum(MP.mpf(float(bl[b, a])) * rd[a] for a in range(3)) / C_LIGHT
                    acc += MP.mpf(float(w[t, b, kk])) * MP.cospi(x)
                    wt += MP.mpf(float(w[t, b, kk]))
        res.append(acc / wt)
    return res


def p_bound(lat, freqs, route, band=False):
    """THE RULE of P per channel (nchan,), or the largest of them (1,) for the band's beam."""
    fq = NP.asarray(freqs, dtype=NP.float64).ravel()
    r = R_OFF + R_PH_P
    if route == 'direct':
        b = P_BAR + 2.0 * NP.pi * U * r * lat.Nd
    else:
        assert route == 'stepped' and (R.TILE - 1) * abs(R.grid_df(fq)) <= fq.min()
        nd0 = lat.Nd[(NP.arange(fq.size) // R.TILE) * R.TILE]
        b = P_BAR + 2.0 * NP.pi * U * (r * lat.Nd + nd0) + 2.0 * NP.pi * R.grid_gap(fq) * lat.tau_max
    return NP.array([b.max()]) if band else b


# ---- the case sets ---------------------------------------------------------------------------------------------------------------------
MOSAIC_CONFIGS = R.CONFIGS                                              # (shape, scale, field) of tests/test_gpu_imaging_reference.py
LATTICE_SHAPE = (33, 33, 5, 13, 2)                                      # (nbl, nchan, ny, nx, nt): five rows of thirteen pixels
LATTICE_CONFIGS = ((1, 1), (1000, 1), (1000, 1000), (8000, 8000))        # (scale of the baselines, divisor of the lattice's half-widths)


def lattice_grid(ny, nx, shrink=1.0):
    """The lattice of tests/csclean_cases.py, l = 0.1 +- 0.15 / shrink over nx and m = -0.05 +- 0.2 / shrink over ny, nx fastest."""
    l = NP.linspace(0.1 - 0.15 / shrink, 0.1 + 0.15 / shrink, nx) if nx > 1 else NP.array([0.1])
    m = NP.linspace(-0.05 - 0.2 / shrink, -0.05 + 0.2 / shrink, ny) if ny > 1 else NP.array([-0.05])
    mm, ll = NP.meshgrid(m, l, indexing='ij')
    ll, mm = ll.ravel(), mm.ravel()
    return NP.stack((ll, mm, NP.sqrt(1.0 - ll * ll - mm * mm)), axis=1)


def shared(geo, A):
    """What mosclean_checker.Problem takes as share=: the reference's phasors E (nt, nchan, npix, nbl) and beams A, as doubles."""
    E = geo.cos.astype(NP.float64) + 1j * geo.sin.astype(NP.float64)
    return types.SimpleNamespace(E=NP.ascontiguousarray(NP.transpose(E, (0, 3, 1, 2))), A=NP.asarray(A, dtype=NP.float64))


def lattice_pointing(geo, ny, nx):
    """The dish pointing of tests/moscs_cases.py from the reference's directions: unit(s[t][centre pixel] + (0.03 (t - 1), 0.02 t, 0))."""
    centre = (ny // 2) * nx + nx // 2
    return IC.unit(NP.stack([geo.s[t, centre] + NP.array([0.03 * (t - 1), 0.02 * t, 0.0]) for t in range(geo.s.shape[0])]))


def scaled(c, scale):
    """The case with its baselines scaled."""
    return dict(c, baselines=NP.asarray(c['baselines'], dtype=NP.float64) * float(scale))


CS_ARGS = ('gain', 'maxiter', 'threshold', 'threshold_relative', 'cycle_depth', 'cycle_niter', 'max_major')
MAXITER, DIVERGED = 2, 16                                               # PRISIM_IMCLEAN_MAXITER, PRISIM_CSCLEAN_DIVERGED of the headers


def assert_not_vacuous(out, live=None):
    """On the REFERENCE's own Cotton-Schwab run: at least two major cycles and eight components in every live channel, and no status
    but MAXITER and DIVERGED."""
    live = NP.ones(out['ncomp'].shape, dtype=bool) if live is None else live
    assert NP.all(out['ncycles'][live] >= 2) and NP.all(out['ncomp'][live] >= 8), (out['ncycles'], out['ncomp'])
    assert set(out['status'][live].tolist()) <= {MAXITER, DIVERGED}, out['status']


@functools.lru_cache(maxsize=None)
def lattice_case(scale, shrink, shape=LATTICE_SHAPE):
    nbl, nchan, ny, nx, nt = shape
    c = IC.case(nbl, nchan, ny * nx, nt)
    c['unitvec'] = lattice_grid(ny, nx, float(shrink))
    c['ny'], c['nx'] = ny, nx
    c['baselines'] = c['baselines'] * float(scale)
    for v in c.values():
        if isinstance(v, NP.ndarray):
            v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def lattice_of(scale, shrink, form='full', chan_avg=False, shape=LATTICE_SHAPE):
    c = lattice_case(scale, shrink, shape)
    return lattice_beam(c['unitvec'], c['rot'], c['baselines'], c['freqs'], c['ny'], c['nx'], R.weights_of(c, form), chan_avg)


@functools.lru_cache(maxsize=None)
def lattice_geometry(scale, shrink, shape=LATTICE_SHAPE):
    return R.geometry_case(lattice_case(scale, shrink, shape))


@functools.lru_cache(maxsize=None)
def horizon_of(shape, scale, field='sphere'):
    c = R.case(shape, scale, field)
    return horizon(c['unitvec'], c['rot'], c['beta'], c['pc'])


@functools.lru_cache(maxsize=None)
def beams_of(shape, field, name):
    """A_ref of a case set: it does not depend on the baselines, so one evaluation serves every scale."""
    c, geo = R.case(shape, 1, field), R.geometry_of(shape, 1, field)
    up, margin = horizon_of(shape, 1, field)
    assert margin >= HORIZON_MARGIN
    A = beams(geo, up, SPECS[name], c['freqs'])
    A.setflags(write=False)
    return A


@functools.lru_cache(maxsize=None)
def mosaic_of(shape, scale, field, name, form='full'):
    c = R.case(shape, scale, field)
    return mosaic(R.geometry_of(shape, scale, field), beams_of(shape, field, name), c['cube'], R.weights_of(c, form))

