"""numpy restatement of the two reference steps that prisim_closure_realizations fuses, on host arrays, given the noise cubes:
prisim/scriptUtils/replicatesim_util.py:94 (outarray = data_array + noise) and, per realisation, the no-filter branch of
prisim/interferometry.py:getClosurePhase (:7427-7485 the gather of the legs with their conjugations, :7625-7627 the bandpass weights,
:7647-7649 the phase of the product of the three legs), stacked as prisim/bispectrum_phase.py:225-244 stacks them:
(nlst, n_realize, ntriads, nchan).  The draw itself is not restated: the noise cubes are handed in (Context.noise on the device, or
any array).  Used by the CPU and the GPU suites; never by the package."""
import numpy as NP


def closure_realizations(cube, noise, bpwts, legs, conj, kind='noisy'):
    """cube: (nt, nrow, nchan) complex visibilities of the used rows; noise: (n_realize, nt, nrow, nchan) complex; bpwts: (nt, nrow,
    nchan) real, bp * bp_wts; legs, conj: (ntriads, 3) used rows and conjugation flags.  Returns (phases (nt, n_realize, ntriads, nchan),
    the bispectra of the same shape)."""
    legs, conj = NP.asarray(legs), NP.asarray(conj)
    vis = (cube[NP.newaxis] + noise) if kind == 'noisy' else noise                   # replicatesim_util.py:94
    triplets = []
    for l in range(3):
        v = vis[:, :, legs[:, l], :]                                                  # (n_realize, nt, ntriads, nchan), :7427-7485
        v = NP.where(conj[:, l].astype(bool)[NP.newaxis, NP.newaxis, :, NP.newaxis], v.conj(), v)
        triplets.append(v * bpwts[NP.newaxis][:, :, legs[:, l], :])                   # :7625-7627 (bpwts is real: its conjugate is itself)
    bispectrum = (triplets[0] * triplets[1]) * triplets[2]                            # :7647, NP.prod over the legs in order
    bispectrum = NP.transpose(bispectrum, (1, 0, 2, 3))                               # bispectrum_phase.py:244
    return NP.angle(bispectrum), bispectrum                                           # :7649


def phase_deviation(phi_a, phi_b):
    """|exp(i phi_a) - exp(i phi_b)|: the distance of two phases on the unit circle"""
    return NP.abs(NP.exp(1j * phi_a) - NP.exp(1j * phi_b))


def triplet_matches(vectors, bltriplet, blltol):
    """Whether a triad's three baseline vectors (3, 3) hold, for every row of bltriplet, a leg within blltol metres of the row or of
    its negative (bispectrum_phase.py:186-204 with both signs allowed)."""
    vectors, bltriplet = NP.asarray(vectors, dtype=NP.float64), NP.asarray(bltriplet, dtype=NP.float64)
    for row in bltriplet:
        d = NP.minimum(NP.sqrt(NP.sum((vectors - row) ** 2, axis=1)), NP.sqrt(NP.sum((vectors + row) ** 2, axis=1)))
        if not NP.any(d <= blltol):
            return False
    return True
