"""Seeded inputs of the mosaic tests (tests/test_mosaic.py, tests/test_gpu_mosaic.py), TEST INFRASTRUCTURE: the beams of the parity
cases, directions that are up, the masked-pixel case and the drift scan of the end-to-end test.  What a GPU test relies on in its
inputs -- the masked fraction, the distance of every element from the mask's threshold, an apparent flux that is off by more than a
hundredth -- is asserted from here on the CPU (tests/test_mosaic.py), with the checker alone."""
import numpy as NP

import imaging_cases as IC
from prisim_amd import _abi, geometry as GEOM, primary_beams as PB

EAST = NP.array([1.0, 0.0, 0.0])
GROUND = {'height': 0.3, 'modifier': None}


def beamformers(nt, seed=7):
    """A 4 x 4 tile steered to another direction in every snapshot, two jitter realisations of delays and gains"""
    rng = NP.random.default_rng(seed)
    pos = PB.mwa_tile_element_locs()
    out = []
    for t in range(nt):
        pc = GEOM.altaz2dircos(NP.array([[60.0 + 5.0 * t, 40.0 * t]]), 'degrees')
        delays = (pos.dot(pc.T) / 299792458.0) + 2e-11 * rng.standard_normal((16, 2))
        gains = 1.0 + 0.05 * rng.standard_normal((16, 2))
        out.append({'positions': pos, 'delays': delays, 'gains': gains})
    return out


def beam_setups(nt):
    """name -> (beam_kind, diameter, ext of the entry, setup of the checker).  The dishes are 2 m wide, so that their beams (some 60
    degrees at 150 MHz) weigh a good part of directions spread over the whole sky."""
    bfs = beamformers(nt)
    return {
        'delta': (_abi.PRISIM_BEAM_DELTA, 0.0, None, {'element': 'delta'}),
        'gaussian': (_abi.PRISIM_BEAM_GAUSSIAN, 2.0, None, {'element': 'gaussian', 'size': 2.0}),
        'airy': (_abi.PRISIM_BEAM_AIRY, 2.0, None, {'element': 'dish', 'size': 2.0}),
        'dipole_ground': (_abi.PRISIM_BEAM_DIPOLE, 0.74, {'dipole_dircos': EAST, 'ground': GROUND},
                          {'element': 'dipole', 'size': 0.74, 'element_dircos': EAST, 'ground': GROUND}),
        'beamformer': (_abi.PRISIM_BEAM_DIPOLE, 0.74, [{'dipole_dircos': EAST, 'beamformer': bf} for bf in bfs],
                       {'element': 'dipole', 'size': 0.74, 'element_dircos': EAST, 'beamformers': bfs}),
    }


def rot_z(deg):
    c, s = NP.cos(NP.radians(deg)), NP.sin(NP.radians(deg))
    return NP.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


FLIP = NP.diag([1.0, -1.0, -1.0])          # a proper rotation that puts what is up below the horizon


def up_case(nbl, nchan, npix, nt, flip=(), down=0, seed=20261019):
    """imaging_cases.case with directions that are local: unit vectors at least 0.05 above the horizon, the last `down` of them as far
    below; rotations about the zenith (which keep them there) but for the snapshots of `flip`, which turn the sky upside down."""
    c = IC.case(nbl, nchan, npix, nt, seed=seed)
    u = c['unitvec'].copy()
    u[:, 2] = NP.abs(u[:, 2]) + 0.05
    u = IC.unit(u)
    if down:
        u[npix - down:, 2] *= -1.0
    c['unitvec'] = u
    c['rot'] = NP.stack([FLIP.dot(rot_z(17.0 * t)) if t in flip else rot_z(17.0 * t) for t in range(nt)])
    c['pc'] = IC.unit(NP.array([[0.02 * t, -0.03 * t, 1.0] for t in range(nt)]))
    return c


MASK_PBMIN = 0.1


def mask_case():
    """The masked-pixel case: 300 directions over the upper hemisphere through the 2 m Gaussian at the zenith, three snapshots."""
    return up_case(37, 33, 300, 3)


# ---- the end-to-end drift scan -------------------------------------------------------------------------------------------------------

LAT = -30.7224
CH = 150e6 + 1e5 * NP.arange(33)
GAUSS14 = {'id': 'custom', 'shape': 'gaussian', 'size': 14.0, 'ocoords': 'altaz', 'orientation': NP.array([[90.0, 270.0]]), 'groundplane': None}
LSTS = [30.0, 31.5, 34.0]
JD0 = 2457000.5
FLUX = 2.75
ZENITH = [90.0, 270.0]
# 2.5 degrees of declination and -3 to +1 degrees of hour angle off the beam centre of a 14 m Gaussian (8.5 degrees wide at 150 MHz);
# 3 degrees off the zenith for the sky that does not move
SOURCE_RADEC = NP.array([[33.0, LAT + 2.5]])
SOURCE_ALTAZ = NP.array([[87.0, 140.0]])


def e2e_baselines(nbl=37):
    rng = NP.random.default_rng(77)
    return rng.uniform(-1.0, 1.0, (nbl, 3)) * NP.array([200.0, 200.0, 5.0])
