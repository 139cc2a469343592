"""Seeded inputs of the mosaic CLEAN tests (tests/test_mosclean.py, tests/test_gpu_mosclean.py), TEST INFRASTRUCTURE: the parity
cases -- directions over the upper hemisphere through 2 m dishes whose pointing moves from snapshot to snapshot -- and the two
sources of the end-to-end case, seen in three snapshots through a chromatic Gaussian that drifts across them.  What a GPU test relies
on in its inputs is asserted on the CPU from the checker alone (tests/test_mosclean.py)."""
import numpy as NP

import imaging_cases as IC
import mosaic_cases as MC
import mosaic_checker as MK
import mosclean_checker as QK
from prisim_amd import _abi
from prisim_amd import interferometry as RI

K = 32
# (nbl, nchan, npix, nt): the smallest there is; 63 pixels of one ragged block; 1000 pixels in four blocks with a second channel tile of
# one channel
SHAPES = [(1, 1, 1, 1), (37, 5, 63, 1), (37, K + 1, 1000, 3)]
FORMS = ('none', 'baseline', 'full')
BEAMS = {'gaussian': _abi.PRISIM_BEAM_GAUSSIAN, 'airy': _abi.PRISIM_BEAM_AIRY}
DISH = 2.0
PBMIN = 0.45                     # of the 2 m dishes over the upper hemisphere: masks and keeps at least a tenth each (asserted)


def pointings(nt):
    """The element pointing of every snapshot: off the zenith, and moving"""
    return IC.unit(NP.array([[0.1 * (t + 1), -0.05 * t, 1.0] for t in range(nt)]))


def parity_case(shape, uniform=True):
    """mosaic_cases.up_case with the pointing of the dishes per snapshot"""
    nbl, nchan, npix, nt = shape
    c = MC.up_case(nbl, nchan, npix, nt)
    if not uniform:
        c['freqs'] = IC.case(nbl, nchan, npix, nt, uniform=False)['freqs']
    c['bpc'] = pointings(nt)
    return c


def weights_of(c, form):
    return {'none': None, 'baseline': c['w_bl'], 'full': c['w_full']}[form]


def problem(c, beam, weights=None, chan_avg=False, window=None, pbmin=PBMIN, share=None, cube=None):
    setups = MK.setups_of(BEAMS[beam], c.get('dish', DISH), c['bpc'], None, c['rot'].shape[0])
    return QK.Problem(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], c['cube'] if cube is None else cube, setups, weights=weights,
                      aberr_beta=c['beta'], chan_avg=chan_avg, window=window, pbmin=pbmin, share=share)


def assert_mask_keeps_and_cuts(pb):
    """Over the (pixel, image channel) elements of the channels that carry weight the reference masks at least a tenth and keeps at
    least a tenth (the distance of every element from the rim is asserted by the Problem itself)."""
    live = ~pb.dead
    masked = float(NP.mean(~pb.valid[:, live]))
    assert 0.1 <= masked <= 0.9, masked
    return masked


# ---- two sources through a drifting chromatic beam ------------------------------------------------------------------------------------

SRC = NP.array([5 * 17 + 3, 11 * 17 + 12])
FLUX = NP.array([1.0, 0.6])


def two_sources():
    """The geometry of the two-source case of tests/test_gpu_imclean.py -- 150 baselines to 300 m, 33 channels, a 17 x 17 grid of
    direction cosines to 0.2, identity frames, zenith phase centre, 1.0 Jy on pixel (row 5, column 3) and 0.6 Jy on (11, 12) -- seen
    in three snapshots through a 4 m Gaussian whose pointing drifts along the line between the two: the beam at the sources runs from
    0.33 to 0.84 and differs between them in every snapshot and from channel to channel.  The cube is what the sky-sum simulates:
    sum_src A[t][src][k] S e^{-i phi_src}, by the checker."""
    base = IC.case(150, K + 1, 289, 1)
    nt = 3
    c = {'unitvec': RI.ApertureSynthesis.dircos_grid(17, 0.2), 'rot': NP.repeat(NP.eye(3)[NP.newaxis], nt, axis=0), 'beta': None,
         'pc': NP.repeat(NP.array([[0.0, 0.0, 1.0]]), nt, axis=0), 'baselines': base['baselines'], 'freqs': base['freqs'], 'dish': 4.0,
         'bpc': IC.unit(NP.array([[-0.04, -0.025, 1.0], [0.0, 0.0, 1.0], [0.04, 0.025, 1.0]])), 'w_bl': None, 'w_full': None}
    c['bpc'][:, 2] = NP.sqrt(1.0 - c['bpc'][:, 0] ** 2 - c['bpc'][:, 1] ** 2)
    c['cube'] = NP.zeros((nt, 150, K + 1), dtype=NP.complex128)
    band = problem(c, 'gaussian', chan_avg=True, pbmin=0.1)
    c['cube'] = sum(band.component_vis(0, int(q), S) for q, S in zip(SRC, FLUX))
    return c, band
