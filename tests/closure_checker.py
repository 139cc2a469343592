"""numpy restatement of InterferometerArray.getClosurePhase's numerics (prisim/interferometry.py:7411-7651) on host cubes, every branch:
the gather of the legs with their conjugations, the spectral weights, the delay filter with the FT1D reading of the delay CLEAN path
(tests/clean_checker.py: inverse=False is numpy.fft.fft, inverse=True is numpy.fft.ifft), the bandpass weights and the phase of the
product.  Used by the CPU and the GPU suites; never by the package."""
import numpy as NP

C_LIGHT = 299792458.0


def filter_unmask(fft_delays, filter_type, filter_mode, delay_min, delay_width, baseline_length=None):
    """:7536-7543 ('regular') / :7570-7587 ('horizon', one baseline) -- ones with zeros on the filtered delays"""
    unmask = NP.ones(fft_delays.size)
    if filter_type == 'regular':
        delay_max = delay_min + delay_width
        if filter_mode == 'discard':
            mask_ind = NP.logical_and(NP.abs(fft_delays) >= delay_min, NP.abs(fft_delays) <= delay_max)
        else:
            mask_ind = NP.logical_or(NP.abs(fft_delays) <= delay_min, NP.abs(fft_delays) >= delay_max)
    else:
        delay_max = baseline_length / C_LIGHT + delay_width
        mask_ind = NP.abs(fft_delays) <= delay_max if filter_mode == 'discard' else NP.abs(fft_delays) >= delay_max
    unmask[mask_ind] = 0.0
    return unmask


def closure_phase(cube, legs, conj, bp, bp_wts, freq_wts=None, delay_filter=None, baseline_lengths=None, df=None):
    """cube, bp, bp_wts: (nbl, nchan, nt); legs, conj: (ntriads, 3).  delay_filter: None or (type, mode, delay_min, delay_width) with
    the width already in seconds.  Returns (triplets (ntriads, 3, nchan, nt), phases (ntriads, nchan, nt))."""
    nbl, nchan, nt = cube.shape
    fw = NP.asarray(1.0).reshape(-1) if freq_wts is None else NP.asarray(freq_wts)
    fft_delays = None if delay_filter is None else NP.fft.fftfreq(nchan, df)
    triplets = []
    for T in range(len(legs)):
        row = []
        for l in range(3):
            ind = int(legs[T][l])
            if conj[T][l]:
                v, bpwts = cube[ind].conj(), bp[ind].conj() * bp_wts[ind].conj()
            else:
                v, bpwts = cube[ind], bp[ind] * bp_wts[ind]
            if delay_filter is not None:
                ftype, fmode, dmin, dwidth = delay_filter
                unmask = filter_unmask(fft_delays, ftype, fmode, dmin, dwidth, None if baseline_lengths is None else baseline_lengths[ind])
                v = NP.fft.ifft(unmask[:, NP.newaxis] * NP.fft.fft(fw.reshape(-1, 1) * v, axis=0), axis=0)
            else:
                v = fw.reshape(-1, 1) * v
            row += [v * bpwts]
        triplets += [row]
    triplets = NP.asarray(triplets)
    return triplets, NP.angle(NP.prod(triplets, axis=1))


def phase_deviation(phi_a, phi_b):
    """|exp(i phi_a) - exp(i phi_b)|: the distance of two phases on the unit circle"""
    return NP.abs(NP.exp(1j * phi_a) - NP.exp(1j * phi_b))
