"""numpy restatement of the reference's antenna_power (prisim/interferometry.py:2362-2408), TEST INFRASTRUCTURE: the sky turned into
alt-az per LST (hadec2altaz written out here), the sources with alt >= 0, the beams of oracle.beams_oracle on them, and
NP.sum(pb * spectrum, 0) / NP.sum(pb, 0).  It also returns what the tolerances of tests/test_gpu_antpower.py are made of."""
import numpy as NP

from oracle import beams_oracle as BO


def hadec2altaz(hadec, latitude):
    """(HA, Dec) degrees -> (alt, az) degrees, az from North through East (astroutils.geometry.hadec2altaz as the reference calls it)."""
    hadec = NP.asarray(hadec, dtype=NP.float64).reshape(-1, 2)
    ha, dec, lat = NP.radians(hadec[:, 0]), NP.radians(hadec[:, 1]), NP.radians(latitude)
    alt = NP.arcsin(NP.clip(NP.sin(dec) * NP.sin(lat) + NP.cos(dec) * NP.cos(lat) * NP.cos(ha), -1.0, 1.0))
    az = NP.arctan2(-NP.cos(dec) * NP.sin(ha), NP.sin(dec) * NP.cos(lat) - NP.cos(dec) * NP.sin(lat) * NP.cos(ha))
    return NP.degrees(NP.stack((alt, NP.where(az < 0.0, az + 2 * NP.pi, az)), axis=1))


def altaz2dircos(altaz):
    alt, az = NP.radians(altaz[:, 0]), NP.radians(altaz[:, 1])
    return NP.stack((NP.cos(alt) * NP.sin(az), NP.cos(alt) * NP.cos(az), NP.sin(alt)), axis=1)


def sky_dircos(location, coords, lst, latitude):
    """East-North-Up direction cosines (n_lst, nsrc, 3) of the sky at every LST, through alt-az as the reference goes (:2371-2385)."""
    loc = NP.asarray(location, dtype=NP.float64)
    out = []
    for l in NP.asarray(lst, dtype=NP.float64).ravel():
        if coords == 'radec':
            altaz = hadec2altaz(NP.stack((l - loc[:, 0], loc[:, 1]), axis=1), latitude)        # :2372-2379
        elif coords == 'hadec':
            altaz = hadec2altaz(loc, latitude)
        elif coords == 'altaz':
            altaz = loc
        else:
            out.append(loc.reshape(-1, 3))
            continue
        out.append(altaz2dircos(altaz))
    return NP.stack(out)


def frame_dircos(unitvec, rot, beta):
    """s = normalise(R (u + beta)) for every snapshot: (nsnap, nsrc, 3)."""
    u = NP.asarray(unitvec, dtype=NP.float64).reshape(-1, 3)
    rot = NP.asarray(rot, dtype=NP.float64).reshape(-1, 3, 3)
    beta = NP.zeros((rot.shape[0], 3)) if beta is None else NP.asarray(beta, dtype=NP.float64).reshape(-1, 3)
    v = NP.einsum('tij,tsj->tsi', rot, u[NP.newaxis] + beta[:, NP.newaxis, :])
    return v / NP.sqrt(NP.sum(v * v, axis=2, keepdims=True))


def beam_of(setup, freqs_hz, t=0):
    """A function dircos -> power pattern (nsrc, nchan) for a setup: dict(element, size, and optionally element_dircos, array, ground,
    beamformer or beamformers (one per snapshot)), the arguments of oracle.beams_oracle.composite_power_beam."""
    kw = {k: v for k, v in setup.items() if k not in ('beamformers',)}
    if 'beamformers' in setup:
        kw['beamformer'] = setup['beamformers'][t]
    return lambda dircos: BO.composite_power_beam(dircos, freqs_hz, **kw)


def antenna_power(dircos, spectrum, beam):
    """dircos (nsnap, nsrc, 3); spectrum (nsrc, nchan); beam(t, dircos_up) -> (n_up, nchan).  Returns a dict of (nsnap, nchan) arrays
    power, num, den, abs_num = sum |pb S| and abs_flux = sum |S| over the sources up, and n_up (nsnap,)."""
    spectrum = NP.asarray(spectrum, dtype=NP.float64)
    out = {k: [] for k in ('power', 'num', 'den', 'abs_num', 'abs_flux', 'n_up')}
    for t in range(dircos.shape[0]):
        up = dircos[t][:, 2] >= 0.0                                                    # alt >= 0.0 (:2398)
        spec = spectrum[up]
        if not NP.any(up):
            pb = NP.zeros((0, spectrum.shape[1]))
        else:
            pb = NP.asarray(beam(t, dircos[t][up]), dtype=NP.float64)
        num, den = NP.sum(pb * spec, axis=0), NP.sum(pb, axis=0)
        with NP.errstate(invalid='ignore', divide='ignore'):
            out['power'].append(num / den)                                             # :2403
        out['num'].append(num)
        out['den'].append(den)
        out['abs_num'].append(NP.sum(NP.abs(pb * spec), axis=0))
        out['abs_flux'].append(NP.sum(NP.abs(spec), axis=0))
        out['n_up'].append(int(NP.sum(up)))
    return {k: NP.asarray(v) for k, v in out.items()}


def tolerances(ref):
    """The bounds of the project's own beam parity (device beams agree with the oracle to 1e-12 absolute, beam x flux to 1e-11
    relative): |den - den_ref| <= 1e-12 n_up + 1e-11 sum pb; |num - num_ref| <= 1e-12 sum |S| + 1e-11 sum |pb S|; and the two combined
    through the quotient, over den_ref, for the power."""
    den_tol = 1e-12 * ref['n_up'][:, NP.newaxis] + 1e-11 * ref['den']
    num_tol = 1e-12 * ref['abs_flux'] + 1e-11 * ref['abs_num']
    with NP.errstate(invalid='ignore', divide='ignore'):
        power_tol = (num_tol + NP.abs(ref['power']) * den_tol) / ref['den']
    return num_tol, den_tol, power_tol
