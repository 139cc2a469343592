"""Seeded inputs of the tests of the Cotton-Schwab CLEAN of the mosaic (tests/test_moscs.py, tests/test_gpu_moscs.py), TEST
INFRASTRUCTURE: the lattice case of tests/csclean_cases.py -- rotations, aberration, phase centres, baselines, cube and weights of
tests/imaging_cases.py on a regular ny x nx lattice -- seen through a dish that points near the lattice in every snapshot,
    bpc[t] = unit(s[t][centre pixel] + (0.03 (t - 1), 0.02 t, 0)),
s the directions of the snapshot (imaging_checker.directions) and the centre pixel (ny // 2, nx // 2).  Where a snapshot's rotation
puts the whole lattice below the horizon its beam is 0 everywhere: the last snapshot of the third shape is such a one.  What a GPU
test relies on in its inputs is asserted on the CPU from the checker alone (tests/test_moscs.py).  The two sources through a drifting
chromatic beam are those of tests/mosclean_cases.py, with the lattice 17 x 17."""
import numpy as NP

import csclean_cases as CC
import imaging_cases as IC
import imaging_checker as IK
import mosaic_checker as MK
import mosclean_cases as QC
import mosclean_checker as QK

K = QC.K
# (nbl, nchan, ny, nx, nt) and the dish: the smallest there is; 63 pixels of one ragged block, neither side a divisor of 256; 1000
# pixels in four blocks, wider than high, with a second channel tile of one channel and three snapshots, the last with everything down
SHAPES = [(1, 1, 1, 1, 1), (37, 5, 9, 7, 1), (37, K + 1, 25, 40, 3)]
DISH = {SHAPES[0]: 2.0, SHAPES[1]: 6.0, SHAPES[2]: 6.0}
PBMIN = {SHAPES[0]: 0.01, SHAPES[1]: 0.3, SHAPES[2]: 0.3}
FORMS = QC.FORMS
BEAMS = QC.BEAMS
# gain, maxiter, threshold (relative), cycle_depth, cycle_niter, max_major: the three settings whose statuses the prototype of the
# definition met
SETTINGS = {'A': dict(gain=0.1, maxiter=40, threshold=0.05, threshold_relative=True, cycle_depth=0.3, cycle_niter=0, max_major=3),
            'B': dict(gain=0.2, maxiter=1000, threshold=0.02, threshold_relative=True, cycle_depth=0.1, cycle_niter=7, max_major=6),
            'C': dict(gain=0.1, maxiter=1000, threshold=0.3, threshold_relative=True, cycle_depth=0.3, cycle_niter=0, max_major=32)}


def replay_args(kw):
    return tuple(kw[n] for n in ('gain', 'maxiter', 'threshold', 'threshold_relative', 'cycle_depth', 'cycle_niter', 'max_major'))


def case(shape, uniform=True):
    nbl, nchan, ny, nx, nt = shape
    c = CC.case(nbl, nchan, ny, nx, nt, uniform=uniform)
    s = IK.directions(c['unitvec'], c['rot'], c['beta'])              # (nt, npix, 3)
    centre = (ny // 2) * nx + nx // 2
    c['bpc'] = IC.unit(NP.stack([s[t, centre] + NP.array([0.03 * (t - 1), 0.02 * t, 0.0]) for t in range(nt)]))
    c['dish'] = DISH.get(shape, 6.0)                                  # another shape: the 6 m dish of the larger ones
    c['pbmin'] = PBMIN.get(shape, 0.3)
    return c


def weights_of(c, form):
    return QC.weights_of(c, form)


def problem(c, beam='gaussian', weights=None, chan_avg=False, window=None, pbmin=None, share=None, cube=None):
    setups = MK.setups_of(BEAMS[beam], c['dish'], c['bpc'], None, c['rot'].shape[0])
    return QK.Problem(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], c['cube'] if cube is None else cube, setups, weights=weights,
                      aberr_beta=c['beta'], chan_avg=chan_avg, window=window, pbmin=c['pbmin'] if pbmin is None else pbmin, share=share)


def two_sources():
    """mosclean_cases.two_sources() with its lattice named: (the case, the band's Problem)"""
    c, band = QC.two_sources()
    c['ny'], c['nx'], c['pbmin'] = 17, 17, 0.1
    return c, band
