"""Seeded inputs of the imaging tests (tests/test_imaging.py, tests/test_gpu_imaging.py), TEST INFRASTRUCTURE: directions in a frame
of their own, a different rotation, aberration vector and phase centre per snapshot, baselines to 300 m, a random cube and weights in
the three forms of include/prisim_imaging.h with every seventh baseline at 0."""
import numpy as NP


def rotation(rng):
    """A proper rotation, orthonormal to rounding."""
    q, r = NP.linalg.qr(rng.standard_normal((3, 3)))
    q = q * NP.sign(NP.diag(r))
    if NP.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def unit(v):
    v = NP.asarray(v, dtype=NP.float64)
    return v / NP.sqrt(NP.sum(v * v, axis=-1, keepdims=True))


def case(nbl, nchan, npix, nt, uniform=True, seed=20261019):
    rng = NP.random.default_rng([seed, nbl, nchan, npix, nt])
    c = {'nbl': nbl, 'nchan': nchan, 'npix': npix, 'nt': nt}
    c['unitvec'] = unit(rng.standard_normal((npix, 3)))
    c['rot'] = NP.stack([rotation(rng) for _ in range(nt)])
    c['beta'] = 1e-4 * rng.standard_normal((nt, 3))                   # |beta| well below 0.01, well above rounding
    c['pc'] = unit(rng.standard_normal((nt, 3)) + NP.array([0.0, 0.0, 2.0]))
    bl = rng.uniform(-1.0, 1.0, (nbl, 3)) * NP.array([300.0, 300.0, 20.0]) / NP.sqrt(2.0)
    bl[0] = [212.0, -211.0, 14.0]                                     # one baseline at the full 300 m
    c['baselines'] = bl
    freqs = 150e6 + 1e5 * NP.arange(nchan)
    if not uniform:
        freqs = freqs + 3e4 * NP.sin(NP.arange(nchan))                # tens of kHz off the line: no uniform grid by any rule
    c['freqs'] = freqs
    c['cube'] = rng.standard_normal((nt, nbl, nchan)) + 1j * rng.standard_normal((nt, nbl, nchan))
    seventh = NP.arange(nbl) % 7 == 6
    w_bl = rng.uniform(1.0, 2.0, nbl)
    w_bl[seventh] = 0.0
    w_full = rng.uniform(1.0, 2.0, (nt, nbl, nchan))
    w_full[:, seventh, :] = 0.0
    c['w_bl'], c['w_full'] = w_bl, w_full
    return c
