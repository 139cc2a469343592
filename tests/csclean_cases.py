"""Seeded inputs of the Cotton-Schwab CLEAN tests (tests/test_csclean.py, tests/test_gpu_csclean.py), TEST INFRASTRUCTURE: the case of
tests/imaging_cases.py -- rotations, aberration, phase centres, baselines, cube and weights -- with its directions replaced by a
regular ny x nx lattice of direction cosines in their own frame, row-major with nx fastest: l centred on 0.1 +- 0.15 over nx, m centred
on -0.05 +- 0.2 over ny (an axis of one pixel sits at its centre)."""
import numpy as NP

import imaging_cases as IC


def grid(ny, nx):
    """(ny * nx, 3) unit vectors of the lattice, nx fastest."""
    l = NP.linspace(0.1 - 0.15, 0.1 + 0.15, nx) if nx > 1 else NP.array([0.1])
    m = NP.linspace(-0.05 - 0.2, -0.05 + 0.2, ny) if ny > 1 else NP.array([-0.05])
    mm, ll = NP.meshgrid(m, l, indexing='ij')
    ll, mm = ll.ravel(), mm.ravel()
    return NP.stack((ll, mm, NP.sqrt(1.0 - ll * ll - mm * mm)), axis=1)


def case(nbl, nchan, ny, nx, nt, uniform=True):
    c = IC.case(nbl, nchan, ny * nx, nt, uniform=uniform)
    c['unitvec'] = grid(ny, nx)
    c['ny'], c['nx'] = ny, nx
    return c
