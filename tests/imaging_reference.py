"""40-digit reference of the dirty image and the synthesized beam by the direct Fourier sum (TEST INFRASTRUCTURE).

What include/prisim_imaging.h states, for pixel p, channel k, the snapshots t and the baselines b:
    s[t][p]  = normalise(R_t (u_p + beta_t)),     d = s[t][p] - s0[t],     E[t][p][b][k] = e^{+2 pi i f_k b.d / c}
    D[p][k]  = sum_{t,b} w (Re V cos phi - Im V sin phi),   W[k] = sum_{t,b} w,   image = D / W,   band image = sum_k D / sum_k W
    scale_k  = sum_{t,b} w |V| / W[k]  (the scale of tests/imaging_checker.py; the PSF is V = 1 and its scale 1)
This module shares no code with prisim_amd, oracle/ or tests/imaging_checker.py; of tests/skyvis_reference.py it takes the integer
helpers alone, and like that module it needs mpmath and an x87 long double.  unitvec, rot, aberr_beta, pc_dircos, the baselines, the
frequencies, the cube and the weights are taken exactly as the doubles they are; c = 299792458 and pi are exact.

Two routes.
  * The directions are the same for both: s and d in mpmath at 60 digits, nt * npix evaluations, each component of d then kept as an
    integer times 2^-140 (2^-111 of a cycle at the 2^29 cycles the library accepts at most).
  * reference: the route the tests use.  f_k b.d / c is a ratio of integers; it is reduced modulo one cycle EXACTLY to [-1/2, 1/2) and
    only then divided (72 fractional bits, skyvis_reference.frac_cycles).  Cosine and sine are taken in numpy.longdouble; w Re V,
    w Im V, every product and every sum, W, sum w|V| and the two divisions are longdouble; the result is rounded to float64 at the end
    and the longdouble values are kept beside it.  An exact half cycle gives (-1, 0) and an exact quarter (0, +-1), not pi's rounding.
  * terms_mp: every term of a (pixel, channel) in mpmath at 60 digits from the unrounded d, summed there: a sub-sample.
  tests/test_imaging_reference.py holds the second to the first on a seeded sub-sample of every case set the GPU tests use: 1e-17 of
  the scale (skyvis_reference.ROUTE_GAP).  Measured 2026-10-21 on x86-64: the largest gap over all sets is 1.2e-19 of the scale.

THE RULE (tests/test_gpu_imaging_reference.py: every element, output finite everywhere, nothing excused), u = 2^-53:
    direct:    |got - ref| <= (1e-11 + 2 pi u (R_DIR N_b[k] + R_PH_DIRECT N'[k])) scale_k
    stepped:   |got - ref| <= (1e-11 + 2 pi u (R_DIR N_b[k] + (R_PH_TAU + 1) N'[k] + N'[k0]) + 2 pi grid_gap tau_max) scale_k
    band:      the largest per-channel factor times the band's scale
    N_b[k]  = f_k max_b sum_i |b_i| / c                      the whole baseline in wavelengths
    N'[k]   = f_k max_{t,p,b} sum_i |b_i| |d_i| / c          the phase scale;   tau_max = N'[k] / f_k;   k0 the first channel of k's tile
1e-11 is the project's bar: it holds sincospi's rounding, the FMAs of the accumulation (nt nbl u of the scale), the division by W
and, stepped, the 31 complex multiplies of the recurrence (a few tens of u).  The length terms are COUNTED FROM THE CODE, not fitted.
A rounding of relative size u on a partial sum of the phase moves the phase by at most u times the 1-norm bound of that partial sum.

The image is not given its directions as the sky-sum is: it computes them, and what rounds s acts on f b.s / c, the whole baseline in
wavelengths, whatever the field of view.  The sky-sum's rule (N' alone) would be wrong here: on a narrow field N' is 200 times below
N_b and the error follows N_b (FLOOR below, asserted in the tests).

  R_DIR = 13, k_img_dirs (prisim_amd/csrc_imaging/imaging_kernels.h:45-52), on N_b:
      4     v_i = (R_i0 t_0 + R_i1 t_1) + R_i2 t_2 with t = u + beta: the sum t (:45), a product, two sums (:46-48): |dv_i| <= 4 u
            sum_j |R_ij| |t_j| <= 4 u |v| (the rows of R are unit vectors to 1e-9)
      x 2.37  the normalisation maps dv to ds_i = (dv_i - s_i (s.dv)) / |v|: |ds_i| <= 4 u (1 + |s_i| sum_j |s_j|), and |s_i| sum_j |s_j|
            <= 1/2 + sqrt(3)/2 = 1.37 on the sphere: 9.46 u
      2.5   the norm given v (:49): a square and two sums under the square root (3 u / 2) and the root (1)
      1     the division (:50)
      sum   9.46 + 3.5 = 12.96, each on a component |s_i| <= 1, so on sum_i |b_i| f / c
  R_PH_TAU = 6, the delay b.d / c of img_rows, on N':
      1     d = s - s0, per component                          imaging_kernels.h:52
      1     kInvC = fl(1 / c), a rounded constant              imaging_kernels.h:29
      1     b * kInvC, per component                           imaging_kernels.h:147
      3     (b0 d.x + b1 d.y) + b2 d.z under -ffp-contract=off: the three products round a term each, u N' together, and the two sums
            a partial sum each                                 imaging_kernels.h:90
  R_PH_DIRECT = 7: R_PH_TAU and the product f_k tau (imaging_kernels.h:109); x - rint(x) and 2 r are exact (:73-74).
  stepped, R_PH_TAU + 2 = 8 roundings: the six of tau act on (f0 + j df) tau, channel k's phase; the seed's product f0 tau (:94) acts
      on N'[k0]; the step's product df tau (:95) is applied j <= 31 times, 31 |df| |tau| u <= N'[k] u since 31 |df| <= f on every
      grid used (asserted).  The stepped phase is (f0 + j df) tau, not f_k tau: grid_gap(freqs) is the largest |f_k - (f_k0 + (k - k0) df)|
      over the channels of every 32-channel tile, df as imaging_grid_uniform forms it (imaging_plan.h:30) and the gap evaluated
      exactly; it adds 2 pi grid_gap tau_max radians.
  (The ISSUE's own count of the phase was 9: it gives the three products of the dot product a rounding each on N', where each rounds
  its own term only.)

CLEAN updates (k_clean_update, prisim_amd/csrc_imaging/clean_update.h).  What an update subtracts from pixel p is the image of the
staged operand w a (cos phi_q, -sin phi_q) (:77), and phi_q is the pick's own chain: its direction from k_img_dirs (R_DIR on N_b), tau =
((b0 kInvC) d.x + (b1 kInvC) d.y) + (b2 kInvC) d.z (:73, the six roundings of R_PH_TAU) and f_k tau (:75), always from the channel's
own frequency.  The pixel's phasor multiplies it in the tile pass with its own chain, direct or stepped.  The term that multiplies
sum |a| in the replay's tolerance carries both:
    update, direct:   1e-11 + 2 pi u (2 R_DIR N_b[k] + 2 R_PH_DIRECT N'[k])
    update, stepped:  1e-11 + 2 pi u (2 R_DIR N_b[k] + (R_PH_DIRECT + R_PH_TAU + 1) N'[k] + N'[k0]) + 2 pi grid_gap tau_max
(update_bound below); the term on scale_k is the image's own rule.

FLOOR of tests/imaging_checker.py against this reference, the worst |checker - ref| / scale_k per decade on the shape (33, 33, 65, 2)
with w_full, as tests/test_imaging_reference.py prints it (measured 2026-10-21 on x86-64; dirty_image | stepped_image | the
float64 restatement of the device, direct / stepped):
    sphere  300 m    3.8e-14 | 3.1e-14 | 3.2e-14 / 3.5e-14 (N_b 2.2e2, N' 2.5e2)      narrow  300 m    2.6e-14 | 2.6e-14 | 2.9e-14 / 2.9e-14 (N_b 2.2e2, N' 1.1)
    sphere  3 km     4.0e-13 | 4.6e-13 | 2.9e-13 / 2.8e-13 (2.2e3, 2.5e3)              narrow  3 km     2.4e-13 | 2.4e-13 | 2.6e-13 / 2.6e-13 (2.2e3, 1.1e1)
    sphere  30 km    3.4e-12 | 3.0e-12 | 3.0e-12 / 3.0e-12 (2.2e4, 2.5e4)              narrow  30 km    2.8e-12 | 2.8e-12 | 3.8e-12 / 3.8e-12 (2.2e4, 1.1e2)
    sphere  300 km   3.3e-11 | 3.3e-11 | 2.6e-11 / 2.6e-11 (2.2e5, 2.5e5)              narrow  300 km   2.7e-11 | 2.7e-11 | 3.1e-11 / 3.1e-11 (2.2e5, 1.1e3)
    sphere  2400 km  2.8e-10 | 3.1e-10 | 2.0e-10 / 2.1e-10 (1.8e6, 2.0e6)              narrow  2400 km  1.7e-10 | 1.7e-10 | 2.3e-10 / 2.3e-10 (1.8e6, 9.1e3)
The error grows linearly with the baseline, 0.16 to 0.24 of 2 pi u N_b on BOTH fields: about a fifth of ONE rounding of the bound's
twenty.  On the narrow field N' is 200 times below N_b and the error is the same: 2 pi u R_PH_DIRECT N' is 5.5e-12 at 300 km and
4.4e-11 at 2400 km there, the error 3.1e-11 and 2.3e-10 (asserted).  The restatement's worst deviation over all sets is 0.086 of the
bound (direct) and 0.082 (stepped).
So the checker keeps 1e-11 of the scale up to the 30 km decade and loses it from the 300 km decade on (CHECKER_KEEPS / CHECKER_LOSES,
asserted both ways); the counted rule holds for the restatement on every set.

ON THE MI355X (tests/test_gpu_imaging_reference.py, 2026-10-21), the worst |device - ref| in units of the scale | of the bound:
    300 m   sphere  dirty 3.2e-14 | 0.002 direct, 3.5e-14 | 0.003 stepped    PSF 2.2e-14 | 0.002 direct, 2.1e-14 | 0.002 stepped
    300 m   narrow  dirty 2.9e-14 | 0.002 direct, 2.9e-14 | 0.002 stepped    PSF 4.1e-14 | 0.003 direct, 4.1e-14 | 0.003 stepped
    3 km    sphere  dirty 2.9e-13 | 0.007 direct, 2.8e-13 | 0.006 stepped    PSF 2.3e-13 | 0.006 direct, 2.4e-13 | 0.005 stepped
    3 km    narrow  dirty 2.6e-13 | 0.008 direct, 2.6e-13 | 0.008 stepped    PSF 3.0e-13 | 0.010 direct, 3.0e-13 | 0.010 stepped
    30 km   sphere  dirty 3.0e-12 | 0.009 direct, 3.0e-12 | 0.009 stepped    PSF 3.1e-12 | 0.009 direct, 3.3e-12 | 0.009 stepped
    30 km   narrow  dirty 3.8e-12 | 0.018 direct, 3.8e-12 | 0.018 stepped    PSF 3.0e-12 | 0.014 direct, 3.0e-12 | 0.014 stepped
    300 km  sphere  dirty 2.6e-11 | 0.008 direct, 2.6e-11 | 0.008 stepped    PSF 3.0e-11 | 0.009 direct, 2.7e-11 | 0.008 stepped
    300 km  narrow  dirty 3.1e-11 | 0.015 direct, 3.1e-11 | 0.015 stepped    PSF 4.3e-11 | 0.021 direct, 4.3e-11 | 0.021 stepped
    2400 km sphere  dirty 2.0e-10 | 0.008 direct, 2.1e-10 | 0.008 stepped    PSF 1.8e-10 | 0.007 direct, 1.7e-10 | 0.006 stepped
    2400 km narrow  dirty 2.3e-10 | 0.014 direct, 2.3e-10 | 0.014 stepped    PSF 2.2e-10 | 0.013 direct, 2.2e-10 | 0.013 stepped
The device is the restatement to two digits.  Elsewhere: the edge grid 1.5e-11 | 0.034 (30 km) and 1.3e-10 | 0.031 (300 km), its gap
term 9.2e-11 and 9.2e-10; the edges set at 300 km 5.1e-11 | 0.021; whole and half cycles 5.8e-17; the largest accepted range (2.7e8
wavelengths) 2.6e-7 | 0.055; the CLEAN replay at most 0.006 of its tolerance on every decade; the adjoint identity at 300 km 5.3e-4 of
its bound, 2.3e-12 of sum|x| sum w|V|.  The 35 GPU tests take 4.6 s.
"""
import collections
import fractions
import functools

import mpmath
import numpy as NP

import imaging_cases as IC
import skyvis_reference as SR

LD = NP.longdouble
MP = mpmath.mp.clone()
MP.dps = 60

C_LIGHT = 299792458
U = 2.0 ** -53
BAR = 1e-11
R_DIR = 13
R_PH_TAU = 6
R_PH_DIRECT = 7
ROUTE_GAP = SR.ROUTE_GAP
TILE = 32
DIR_BITS = 140

SCALES = (1, 10, 100, 1000, 8000)                          # the longest baseline: 300 m, 3 km, 30 km, 300 km, 2400 km
CHECKER_KEEPS = (1, 10, 100)                               # decades on which tests/imaging_checker.py is inside 1e-11 of the scale
CHECKER_LOSES = (1000, 8000)                               # ... and outside it
SHAPES = ((1, 1, 1, 1), (32, 32, 64, 1), (33, 33, 65, 2), (3, 65, 257, 1))      # (nbl, nchan, npix, nt)
MAX_TERMS = 200000

Geometry = collections.namedtuple('Geometry', 'D s d cos sin Nb Np tau_max')
Image = collections.namedtuple('Image', 'image wsum D scale band_image band_wsum band_scale image_ld wsum_ld D_ld num_ld')


# ---- the directions --------------------------------------------------------------------------------------------------------------------
def directions_mp(unitvec, rot, beta, pc):
    """[t][p] -> (s, d) as lists of three mpmath numbers: s = normalise(R_t (u_p + beta_t)), d = s - s0[t], at 60 digits."""
    u = NP.asarray(unitvec, dtype=NP.float64).reshape(-1, 3)
    rot = NP.asarray(rot, dtype=NP.float64).reshape(-1, 3, 3)
    nt = rot.shape[0]
    beta = NP.zeros((nt, 3)) if beta is None else NP.asarray(beta, dtype=NP.float64).reshape(nt, 3)
    pc = NP.asarray(pc, dtype=NP.float64).reshape(nt, 3)
    out = []
    for t in range(nt):
        R = [[MP.mpf(float(rot[t, i, j])) for j in range(3)] for i in range(3)]
        b = [MP.mpf(float(x)) for x in beta[t]]
        s0 = [MP.mpf(float(x)) for x in pc[t]]
        row = []
        for p in range(u.shape[0]):
            x = [MP.mpf(float(u[p, j])) + b[j] for j in range(3)]
            v = [R[i][0] * x[0] + R[i][1] * x[1] + R[i][2] * x[2] for i in range(3)]
            n = MP.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
            s = [vi / n for vi in v]
            row.append((s, [s[i] - s0[i] for i in range(3)]))
        out.append(row)
    return out


@functools.lru_cache(maxsize=None)
def _two_pi():
    return LD(2) * SR.to_ld(MP.pi)


def geometry(unitvec, rot, beta, pc, baselines, freqs):
    """Geometry: D (nt, npix, 3) the integers d 2^140; s and d rounded to doubles; cos and sin (nt, npix, nbl, nchan) of the phasors E in
    longdouble; N_b, N' and tau_max per channel."""
    bl = NP.ascontiguousarray(baselines, dtype=NP.float64).reshape(-1, 3)
    fq = NP.ascontiguousarray(freqs, dtype=NP.float64).ravel()
    sd = directions_mp(unitvec, rot, beta, pc)
    nt, npix = len(sd), len(sd[0])
    assert nt * npix * bl.shape[0] * fq.size <= MAX_TERMS
    D = NP.empty((nt, npix, 3), dtype=object)
    s, d = NP.empty((nt, npix, 3)), NP.empty((nt, npix, 3))
    for t in range(nt):
        for p in range(npix):
            for i in range(3):
                D[t, p, i] = int(MP.nint(MP.ldexp(sd[t][p][1][i], DIR_BITS)))
                s[t, p, i], d[t, p, i] = float(sd[t][p][0][i]), float(sd[t][p][1][i])
    B, kb = SR.ints(bl)
    F, kf = SR.ints(fq)
    M = D[:, :, None, 0] * B[None, None, :, 0] + D[:, :, None, 1] * B[None, None, :, 1] + D[:, :, None, 2] * B[None, None, :, 2]
    frac = SR.frac_cycles(M[..., None] * F, kb + kf + DIR_BITS)                      # (nt, npix, nbl, nchan), cycles in [-1/2, 1/2)
    ang = frac * _two_pi()
    cos = NP.where(NP.abs(frac) == LD(0.25), LD(0), NP.cos(ang))
    sin = NP.where(frac == LD(-0.5), LD(0), NP.where(NP.abs(frac) == LD(0.25), NP.sign(frac), NP.sin(ang)))
    nb1 = float(NP.max(NP.sum(NP.abs(bl), axis=1)))
    np1 = float(NP.max(NP.einsum('bi,tpi->tpb', NP.abs(bl), NP.abs(d))))
    for a in (s, d, cos, sin):
        a.setflags(write=False)
    return Geometry(D, s, d, cos, sin, fq * nb1 / C_LIGHT, fq * np1 / C_LIGHT, np1 / C_LIGHT)


def image(geo, cube=None, weights=None, kind='dirty'):
    """Image of the cube (nt, nbl, nchan) complex128, or of V = 1 (kind 'psf'), with weights None, (nbl,) or (nt, nbl, nchan)."""
    nt, npix, nbl, nchan = geo.cos.shape
    if weights is None:
        w = NP.ones((nt, nbl, nchan), dtype=LD)
    else:
        w = NP.asarray(weights, dtype=NP.float64)
        w = NP.broadcast_to(w[None, :, None] if w.shape == (nbl,) else w, (nt, nbl, nchan)).astype(LD)
    if kind == 'psf':
        re, im = NP.ones((nt, nbl, nchan), dtype=LD), NP.zeros((nt, nbl, nchan), dtype=LD)
    else:
        v = NP.asarray(cube, dtype=NP.complex128).reshape(nt, nbl, nchan)
        re, im = v.real.astype(LD), v.imag.astype(LD)
    wre, wim = w * re, w * im
    D = NP.sum(wre[:, None] * geo.cos - wim[:, None] * geo.sin, axis=(0, 2))        # (npix, nchan)
    W = NP.sum(w, axis=(0, 1))
    num = NP.sum(w * NP.sqrt(re * re + im * im), axis=(0, 1))
    assert NP.all(W > 0)
    img, band = D / W, D.sum(axis=1) / W.sum()
    f = lambda a: NP.asarray(a).astype(NP.float64)                      # noqa: E731
    return Image(f(img), f(W), f(D), f(num / W), f(band), f(W.sum()).reshape(1), float(num.sum() / W.sum()), img, W, D, num)


def terms_mp(unitvec, rot, beta, pc, baselines, freqs, cube, weights, kind, outputs):
    """[D[p][k]] in mpmath for the (p, k) of `outputs`: every term formed and summed at 60 digits, from the unrounded d."""
    bl = NP.ascontiguousarray(baselines, dtype=NP.float64).reshape(-1, 3)
    fq = NP.ascontiguousarray(freqs, dtype=NP.float64).ravel()
    sd = directions_mp(unitvec, rot, beta, pc)
    nt, nbl, nchan = len(sd), bl.shape[0], fq.size
    w = NP.ones((nt, nbl, nchan)) if weights is None else NP.asarray(weights, dtype=NP.float64)
    w = NP.broadcast_to(w[None, :, None] if w.shape == (nbl,) else w, (nt, nbl, nchan))
    v = NP.ones((nt, nbl, nchan), dtype=NP.complex128) if kind == 'psf' else NP.asarray(cube, dtype=NP.complex128)
    bm = [[MP.mpf(float(x)) for x in row] for row in bl]
    res = []
    for p, k in outputs:
        f, acc = MP.mpf(float(fq[k])), MP.mpf(0)
        for t in range(nt):
            d = sd[t][p][1]
            for b in range(nbl):
                x = 2 * f * (bm[b][0] * d[0] + bm[b][1] * d[1] + bm[b][2] * d[2]) / C_LIGHT
                acc += MP.mpf(float(w[t, b, k])) * (MP.mpf(float(v[t, b, k].real)) * MP.cospi(x) - MP.mpf(float(v[t, b, k].imag)) * MP.sinpi(x))
        res.append(acc)
    return res


def route_gap(c, weights, kind, ref, nsample=16, seed=0):
    """Largest |fast route - mpmath route| in units of the scale over a seeded sub-sample of the outputs (the corners always)."""
    npix, nchan = ref.D.shape
    rng = NP.random.default_rng(seed)
    outs = {(0, 0), (npix - 1, nchan - 1), (0, nchan - 1), (npix - 1, 0)}
    while len(outs) < min(nsample, npix * nchan):
        outs.add((int(rng.integers(npix)), int(rng.integers(nchan))))
    outs = sorted(outs)
    want = terms_mp(c['unitvec'], c['rot'], c['beta'], c['pc'], c['baselines'], c['freqs'], c['cube'], weights, kind, outs)
    worst = 0.0
    for (p, k), x in zip(outs, want):
        worst = max(worst, float(abs(SR.ld_to_mp(ref.D_ld[p, k]) - x) / SR.ld_to_mp(ref.num_ld[k])))
    return worst


# ---- the rule --------------------------------------------------------------------------------------------------------------------------
def grid_df(freqs):
    """df as imaging_grid_uniform forms it, in float64."""
    fq = NP.asarray(freqs, dtype=NP.float64).ravel()
    return float((fq[-1] - fq[0]) / float(fq.size - 1)) if fq.size > 1 else 0.0


def grid_gap(freqs):
    """The largest |f_k - (f_k0 + (k - k0) df)| over the channels of every 32-channel tile, evaluated exactly."""
    fq = NP.asarray(freqs, dtype=NP.float64).ravel()
    df = fractions.Fraction(grid_df(fq))
    gap = fractions.Fraction(0)
    for k in range(fq.size):
        k0 = k - k % TILE
        gap = max(gap, abs(fractions.Fraction(float(fq[k])) - (fractions.Fraction(float(fq[k0])) + (k - k0) * df)))
    return float(gap)


def _length_term(geo, freqs, route, r_dir, r_tau, r_prod):
    """2 pi u (r_dir N_b + r_tau N' + the products of the route) [+ the grid's gap], per channel."""
    fq = NP.asarray(freqs, dtype=NP.float64).ravel()
    if route == 'direct':
        return 2.0 * NP.pi * U * (r_dir * geo.Nb + (r_tau + r_prod + 1) * geo.Np)
    assert route == 'stepped' and (TILE - 1) * abs(grid_df(fq)) <= fq.min()
    np0 = geo.Np[(NP.arange(fq.size) // TILE) * TILE]
    return 2.0 * NP.pi * U * (r_dir * geo.Nb + (r_tau + r_prod + 1) * geo.Np + np0) + 2.0 * NP.pi * grid_gap(fq) * geo.tau_max


def bound(geo, freqs, route, band=False):
    """THE RULE's factor of scale_k per channel (nchan,), or the largest of them (1,) for the band's image."""
    b = BAR + _length_term(geo, freqs, route, R_DIR, R_PH_TAU, 0)
    return NP.array([b.max()]) if band else b


def update_bound(geo, freqs, route, band=False):
    """The factor of sum |a| in the tolerance of a CLEAN replay: the pick's chain (always direct) and the pixel's."""
    b = BAR + _length_term(geo, freqs, route, 2 * R_DIR, 2 * R_PH_TAU, 1)
    return NP.array([b.max()]) if band else b


# ---- the case sets ---------------------------------------------------------------------------------------------------------------------
def _narrow(c, radius=0.01, seed=5):
    """Snapshot 0 alone, its pixels redrawn within `radius` rad of its phase centre."""
    rng = NP.random.default_rng(seed)
    npix = c['npix']
    c = dict(c, nt=1, rot=c['rot'][:1].copy(), beta=c['beta'][:1].copy(), pc=c['pc'][:1].copy(), cube=c['cube'][:1].copy(),
             w_full=c['w_full'][:1].copy())
    off = rng.standard_normal((npix, 3))
    off = 0.9 * radius * rng.uniform(0.0, 1.0, (npix, 1)) ** 0.5 * off / NP.sqrt(NP.sum(off * off, axis=1, keepdims=True))
    target = IC.unit(c['pc'][0] + off)
    c['unitvec'] = IC.unit(target @ c['rot'][0] - c['beta'][0])                  # R^T s - beta, back on the sphere
    return c


@functools.lru_cache(maxsize=None)
def case(shape, scale, field='sphere', uniform=True):
    """imaging_cases.case of the shape with its baselines scaled; field 'narrow': see _narrow.  Not to be written to."""
    c = IC.case(*shape, uniform=uniform)
    if field == 'narrow':
        c = _narrow(c)
    c['baselines'] = c['baselines'] * float(scale)
    for v in c.values():
        if isinstance(v, NP.ndarray):
            v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def geometry_of(shape, scale, field='sphere', uniform=True):
    c = case(shape, scale, field, uniform)
    return geometry(c['unitvec'], c['rot'], c['beta'], c['pc'], c['baselines'], c['freqs'])


@functools.lru_cache(maxsize=None)
def image_of(shape, scale, field='sphere', uniform=True, form='full', kind='dirty'):
    c = case(shape, scale, field, uniform)
    r = image(geometry_of(shape, scale, field, uniform), c['cube'], weights_of(c, form), kind)
    for a in (r.image, r.wsum, r.D, r.scale, r.band_image):
        assert NP.all(NP.isfinite(a))
        a.setflags(write=False)
    return r


def weights_of(c, form):
    return {'none': None, 'baseline': c['w_bl'], 'full': c['w_full']}[form]


# the integer and half-integer phases: f = 2^27 Hz, baselines c 2^-k m along an axis, axis-aligned directions about the zenith
EXACT_F = 2.0 ** 27


def edges_case(scale):
    """R = I, beta = 0, the phase centre at the zenith: a pixel there exactly, its antipode, the six axes, seeded pixels; a zero
    baseline, baselines along one axis, seeded ones to 300 m times `scale`; 33 channels."""
    rng = NP.random.default_rng(977)
    axes = NP.array([[0, 0, 1], [0, 0, -1], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0]], dtype=NP.float64)
    u = NP.vstack((axes, IC.unit(rng.standard_normal((27, 3)))))
    bl = rng.uniform(-1.0, 1.0, (12, 3)) * NP.array([300.0, 300.0, 20.0]) / NP.sqrt(2.0)
    bl[0] = 0.0
    bl[1], bl[2], bl[3] = (250.0, 0.0, 0.0), (0.0, -170.0, 0.0), (0.0, 0.0, 19.0)
    bl = bl * float(scale)
    nt, nbl, nchan = 1, 12, 33
    cube = rng.standard_normal((nt, nbl, nchan)) + 1j * rng.standard_normal((nt, nbl, nchan))
    return {'nbl': nbl, 'nchan': nchan, 'npix': u.shape[0], 'nt': nt, 'unitvec': u, 'rot': NP.eye(3)[None].copy(), 'beta': NP.zeros((1, 3)),
            'pc': NP.array([[0.0, 0.0, 1.0]]), 'baselines': bl, 'freqs': 150e6 + 1e5 * NP.arange(nchan), 'cube': cube,
            'w_bl': rng.uniform(1.0, 2.0, nbl), 'w_full': rng.uniform(1.0, 2.0, (nt, nbl, nchan))}


def exact_case():
    """One channel at 2^27 Hz, the baselines c 2^-k m along East for k = 24 .. 28 (8, 4, 2, 1 and 1/2 cycles per unit of d_x) and the
    pixels East, West and the zenith about a phase centre at the zenith: d_x = +1, -1, 0, and every phase a whole or a half cycle."""
    ks = NP.arange(24, 29)
    bl = NP.zeros((ks.size, 3))
    bl[:, 0] = float(C_LIGHT) * 2.0 ** -ks
    rng = NP.random.default_rng(31)
    cube = rng.standard_normal((1, ks.size, 1)) + 1j * rng.standard_normal((1, ks.size, 1))
    return {'nbl': ks.size, 'nchan': 1, 'npix': 3, 'nt': 1, 'unitvec': NP.array([[1.0, 0, 0], [-1.0, 0, 0], [0, 0, 1.0]]),
            'rot': NP.eye(3)[None].copy(), 'beta': NP.zeros((1, 3)), 'pc': NP.array([[0.0, 0.0, 1.0]]), 'baselines': bl,
            'freqs': NP.array([EXACT_F]), 'cube': cube, 'w_bl': rng.uniform(1.0, 2.0, ks.size), 'w_full': rng.uniform(1.0, 2.0, (1, ks.size, 1))}


def edge_grid_case(scale):
    """The case (33, 33, 65, 2) with its inner channels three units in the last place (8.9e-8 Hz) either side of their line, in turn:
    inside the 1e-7 Hz rule of imaging_grid_uniform, so AUTO steps, and the stepped phase (f0 + j df) tau is off the true one."""
    c = dict(case((33, 33, 65, 2), scale))
    f = c['freqs'].copy()
    f[1:-1] += NP.where(NP.arange(1, f.size - 1) % 2 == 0, 3.0, -3.0) * NP.spacing(f[0])
    assert 0.85e-7 < NP.max(NP.abs(f - c['freqs'])) <= 1e-7 and 0.85e-7 < grid_gap(f) <= 1e-7 and grid_df(f) == 1e5
    c['freqs'] = f
    return c


def range_edge():
    """(the longest East baseline at 150 MHz with max|b| 2 max|f| / c < 2^29 cycles as the library forms it, the next double up)."""
    f = 150e6
    below = 2.0 ** 29 * C_LIGHT / (2.0 * f)
    while below * 2.0 * f / 299792458.0 >= 2.0 ** 29:
        below = float(NP.nextafter(below, 0.0))
    above = below
    while above * 2.0 * f / 299792458.0 < 2.0 ** 29:
        above = float(NP.nextafter(above, NP.inf))
    return below, above


def largest_case():
    """One baseline, one channel and five pixels at the largest phase range the library accepts."""
    c = dict(case((1, 1, 1, 1), 1))
    c.update(npix=5, unitvec=NP.array([[0.0, 0.0, 1.0], [0.0, 0.0, -1.0], [0.6, 0.0, 0.8], [0.0, -1.0, 0.0], [-0.28, 0.96, 0.0]]),
             baselines=NP.array([[range_edge()[0], 0.0, 0.0]]), freqs=NP.array([150e6]))
    return c


def geometry_case(c):
    return geometry(c['unitvec'], c['rot'], c['beta'], c['pc'], c['baselines'], c['freqs'])


# every set tests/test_gpu_imaging_reference.py runs: (name, thunk of the case, the grid is uniform)
CONFIGS = [(sh, sc, field) for sh in SHAPES for sc in (SCALES if sh == (33, 33, 65, 2) else (1, 1000)) for field in ('sphere', 'narrow')]


def sets():
    out = [('%s x%d %s' % (sh, sc, field), functools.partial(case, sh, sc, field), True) for sh, sc, field in CONFIGS]
    out += [('non-uniform x%d' % sc, functools.partial(case, (33, 33, 65, 2), sc, 'sphere', False), False) for sc in (1, 1000)]
    out += [('edge grid x%d' % sc, functools.partial(edge_grid_case, sc), True) for sc in (100, 1000)]
    out += [('edges x%d' % sc, functools.partial(edges_case, sc), True) for sc in (1, 1000)]
    return out + [('whole and half cycles', exact_case, True), ('largest range', largest_case, True)]
