"""numpy statement of include/prisim_imaging.h, TEST INFRASTRUCTURE: the dirty image and the synthesized beam by the direct Fourier sum
in complex128, einsum over (t, b), every phase from the channel's own frequency (no stepping), and the scale the tolerances of
tests/test_gpu_imaging.py are taken against."""
import numpy as NP

C_LIGHT = 299792458.0


def directions(unitvec, rot, beta=None):
    """s[t][p] = normalise(R_t (u_p + beta_t)): (nt, npix, 3)."""
    u = NP.asarray(unitvec, dtype=NP.float64).reshape(-1, 3)
    rot = NP.asarray(rot, dtype=NP.float64).reshape(-1, 3, 3)
    beta = NP.zeros((rot.shape[0], 3)) if beta is None else NP.asarray(beta, dtype=NP.float64).reshape(-1, 3)
    v = NP.einsum('tij,tpj->tpi', rot, u[NP.newaxis] + beta[:, NP.newaxis, :])
    return v / NP.sqrt(NP.sum(v * v, axis=2, keepdims=True))


def full_weights(weights, nt, nbl, nchan):
    """None, (nbl,) or (nt, nbl, nchan) as (nt, nbl, nchan)."""
    if weights is None:
        return NP.ones((nt, nbl, nchan))
    w = NP.asarray(weights, dtype=NP.float64)
    if w.shape == (nbl,):
        return NP.broadcast_to(w[NP.newaxis, :, NP.newaxis], (nt, nbl, nchan))
    assert w.shape == (nt, nbl, nchan), w.shape
    return w


def dirty_image(unitvec, rot, pc_dircos, baselines, freqs_hz, cube=None, weights=None, kind='dirty', chan_avg=False, aberr_beta=None,
                nonzero=None, dtype=NP.float64, pixel_chunk=64):
    """Returns {'image', 'wsum', 'D', 'scale'} and, with chan_avg = False, 'band': the same four of chan_avg = True.  image (npix,
    nchan) or (npix,); wsum (nchan,) or (1,); D (npix, nchan) the numerators;
    scale = sum_{t,b} w |V| / sum w per channel (chan_avg: of the band; the PSF: |V| = 1, so 1) -- NaN where the weight sum is 0.
    nonzero: the channels (boolean (nchan,)) whose weight sum is meant to be non-zero, all by default: each is asserted >= 1 before
    anything is divided.  dtype NP.longdouble evaluates the phases and the sums in extended precision."""
    bl = NP.asarray(baselines, dtype=dtype).reshape(-1, 3)
    fq = NP.asarray(freqs_hz, dtype=dtype).ravel()
    s = directions(unitvec, rot, aberr_beta).astype(dtype)
    pc = NP.asarray(pc_dircos, dtype=dtype).reshape(-1, 3)
    nt, npix, nbl, nchan = s.shape[0], s.shape[1], bl.shape[0], fq.size
    w = full_weights(weights, nt, nbl, nchan).astype(dtype)
    ctype = NP.clongdouble if dtype == NP.longdouble else NP.complex128
    v = NP.ones((nt, nbl, nchan), dtype=ctype) if kind == 'psf' else NP.asarray(cube).astype(ctype)
    assert v.shape == (nt, nbl, nchan), v.shape
    wv = w * v
    two_pi = 2 * NP.arccos(NP.asarray(-1.0, dtype=dtype))
    D = NP.empty((npix, nchan), dtype=dtype)
    for p0 in range(0, npix, pixel_chunk):
        d = s[:, p0:p0 + pixel_chunk] - pc[:, NP.newaxis, :]                         # (nt, np, 3)
        tau = NP.einsum('tpi,bi->tpb', d, bl) / dtype(C_LIGHT)
        ph = NP.exp(1j * (two_pi * tau[..., NP.newaxis] * fq))                      # (nt, np, nbl, nchan)
        D[p0:p0 + pixel_chunk] = NP.einsum('tbk,tpbk->pk', wv, ph).real
    W = NP.einsum('tbk->k', w)
    meant = NP.ones(nchan, dtype=bool) if nonzero is None else NP.asarray(nonzero, dtype=bool)
    assert NP.all(W[meant] >= 1.0), W[meant].min()
    assert NP.all(W[~meant] == 0.0)
    num = NP.einsum('tbk->k', w * NP.abs(v))
    with NP.errstate(invalid='ignore', divide='ignore'):
        band = {'image': D.sum(axis=1) / W.sum(), 'wsum': NP.array([W.sum()]), 'D': D, 'scale': num.sum() / W.sum()}
        if chan_avg:
            return band
        return {'image': D / W, 'wsum': W, 'D': D, 'scale': num / W, 'band': band}


def stepped_image(unitvec, rot, pc_dircos, baselines, freqs_hz, cube, weights=None, aberr_beta=None, reseed=32):
    """D / W with the phasor seeded every `reseed` channels from the true frequency and stepped by e^{2 pi i tau df} in between: what
    the stepped route of the device does, in numpy (uniform grids)."""
    bl = NP.asarray(baselines, dtype=NP.float64).reshape(-1, 3)
    fq = NP.asarray(freqs_hz, dtype=NP.float64).ravel()
    s = directions(unitvec, rot, aberr_beta)
    pc = NP.asarray(pc_dircos, dtype=NP.float64).reshape(-1, 3)
    nt, nbl, nchan = s.shape[0], bl.shape[0], fq.size
    w = full_weights(weights, nt, nbl, nchan)
    df = (fq[-1] - fq[0]) / (nchan - 1) if nchan > 1 else 0.0
    tau = NP.einsum('tpi,bi->tpb', s - pc[:, NP.newaxis, :], bl) / C_LIGHT
    step = NP.exp(2j * NP.pi * tau * df)
    D = NP.empty((s.shape[1], nchan))
    for k in range(nchan):
        z = NP.exp(2j * NP.pi * tau * fq[k]) if k % reseed == 0 else z * step
        D[:, k] = NP.einsum('tb,tpb->p', w[:, :, k] * NP.asarray(cube)[:, :, k], z).real
    return D / NP.einsum('tbk->k', w)


def point_source_cube(src_dircos, flux, pc_dircos, baselines, freqs_hz):
    """V[t][b][k] = S e^{-2 pi i f b . (s_src[t] - s0[t]) / c}: what the sky-sum gives for one source seen through a delta beam."""
    src = NP.asarray(src_dircos, dtype=NP.float64).reshape(-1, 3)
    pc = NP.asarray(pc_dircos, dtype=NP.float64).reshape(-1, 3)
    tau = NP.einsum('ti,bi->tb', src - pc, NP.asarray(baselines, dtype=NP.float64)) / C_LIGHT
    return flux * NP.exp(-2j * NP.pi * tau[..., NP.newaxis] * NP.asarray(freqs_hz, dtype=NP.float64))


def skysum(src_dircos, flux, pc_dircos, baselines, freqs_hz):
    """V[t][b][k] = sum_s x_s e^{-2 pi i f b . (s[t][s] - s0[t]) / c}; src_dircos (nt, nsrc, 3), flux (nsrc,)."""
    src = NP.asarray(src_dircos, dtype=NP.float64)
    pc = NP.asarray(pc_dircos, dtype=NP.float64).reshape(-1, 3)
    tau = NP.einsum('tsi,bi->tsb', src - pc[:, NP.newaxis, :], NP.asarray(baselines, dtype=NP.float64)) / C_LIGHT
    ph = NP.exp(-2j * NP.pi * tau[..., NP.newaxis] * NP.asarray(freqs_hz, dtype=NP.float64))
    return NP.einsum('s,tsbk->tbk', NP.asarray(flux, dtype=NP.float64), ph)
