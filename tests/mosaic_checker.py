"""numpy statement of include/prisim_mosaic.h, TEST INFRASTRUCTURE: the beam-weighted linear mosaic of the snapshots in complex128,
einsum over b, every phase from the channel's own frequency (no stepping), the beams from oracle.beams_oracle by way of
tests/antpower_checker.py, and the bounds the tolerances of tests/test_gpu_mosaic.py are made of:
    |N - N_ref| <= 1e-11 sum_t A_ref sum_b w|V| + 1e-12 sum_{t,b} w|V|          (the image sums to 1e-11 of their natural scale,
    |Q - Q_ref| <= 1e-11 sum_t A_ref^2 W_t  + 2e-12 sum_t A_ref W_t              the device beams to 1e-12 absolute)
The quotient, the mask and the effective beam are not compared to a bound: quotient() restates them from num, den and wsum with the
expressions of the header, and the device's outputs are held to it exactly."""
import numpy as NP

import antpower_checker as AK
import imaging_checker as IK
from prisim_amd import _abi

HORIZON_MARGIN = 1e-9            # min |s_z| asserted, so that the horizon test cannot differ between two roundings


def snapshot_sums(unitvec, rot, pc_dircos, baselines, freqs_hz, cube, weights=None, aberr_beta=None, pixel_chunk=64):
    """Per snapshot: D (nt, npix, nchan) = sum_b w Re(V e^{+i phi}), W (nt, nchan) = sum_b w, absV (nt, nchan) = sum_b w|V|, and the
    directions s (nt, npix, 3)."""
    bl = NP.asarray(baselines, dtype=NP.float64).reshape(-1, 3)
    fq = NP.asarray(freqs_hz, dtype=NP.float64).ravel()
    s = IK.directions(unitvec, rot, aberr_beta)
    pc = NP.asarray(pc_dircos, dtype=NP.float64).reshape(-1, 3)
    nt, npix, nbl, nchan = s.shape[0], s.shape[1], bl.shape[0], fq.size
    w = IK.full_weights(weights, nt, nbl, nchan)
    v = NP.asarray(cube).astype(NP.complex128)
    assert v.shape == (nt, nbl, nchan), v.shape
    wv = w * v
    D = NP.empty((nt, npix, nchan))
    for p0 in range(0, npix, pixel_chunk):
        d = s[:, p0:p0 + pixel_chunk] - pc[:, NP.newaxis, :]
        tau = NP.einsum('tpi,bi->tpb', d, bl) / IK.C_LIGHT
        ph = NP.exp(1j * (2 * NP.pi * tau[..., NP.newaxis] * fq))                  # (nt, np, nbl, nchan)
        D[:, p0:p0 + pixel_chunk] = NP.einsum('tbk,tpbk->tpk', wv, ph).real
    return {'D': D, 'W': NP.einsum('tbk->tk', w), 'absV': NP.einsum('tbk->tk', w * NP.abs(v)), 's': s}


def beams(s, freqs_hz, setup):
    """A (nt, npix, nchan): the power pattern of `setup` (antpower_checker.beam_of; one for all snapshots, or a list of one each) at
    the directions s (nt, npix, 3), 0 below the horizon.  No direction may graze the horizon."""
    assert NP.min(NP.abs(s[..., 2])) >= HORIZON_MARGIN, NP.min(NP.abs(s[..., 2]))
    per = setup if isinstance(setup, (list, tuple)) else [setup] * s.shape[0]
    A = NP.stack([NP.asarray(AK.beam_of(per[t], freqs_hz, t)(s[t]), dtype=NP.float64) for t in range(s.shape[0])])
    A[s[..., 2] < 0.0] = 0.0
    return A


def quotient(num, den, wsum, pbmin, chan_avg=False):
    """(mosaic, pb_eff) from N, Q (npix, nchan) and Wtot (nchan,) by the expressions of include/prisim_mosaic.h, the sums over k
    ascending one term at a time."""
    num, den, wsum = NP.asarray(num, dtype=NP.float64), NP.asarray(den, dtype=NP.float64), NP.asarray(wsum, dtype=NP.float64)
    if chan_avg:
        n, q, w = NP.zeros(num.shape[0]), NP.zeros(num.shape[0]), 0.0
        for k in range(num.shape[1]):
            n, q, w = n + num[:, k], q + den[:, k], w + wsum[k]
        num, den, wsum = n, q, w
    with NP.errstate(invalid='ignore', divide='ignore'):
        return NP.where(den >= (pbmin * pbmin) * wsum, num / den, NP.nan), NP.sqrt(den / wsum)


def combine(sums, A, pbmin=0.1, chan_avg=False):
    """The mosaic of snapshot_sums() and beams(): {'mosaic', 'pb_eff', 'num', 'den', 'wsum', 'wt', 'A', 'bound_num', 'bound_den'};
    num, den and the bounds (npix, nchan), wsum (nchan,), wt (nt, nchan)."""
    D, W, absV = sums['D'], sums['W'], sums['absV']
    num, den = NP.zeros(D.shape[1:]), NP.zeros(D.shape[1:])
    for t in range(D.shape[0]):
        num = num + A[t] * D[t]
        den = den + A[t] * A[t] * W[t][NP.newaxis, :]
    wsum = NP.zeros(W.shape[1])
    for t in range(W.shape[0]):
        wsum = wsum + W[t]
    mosaic, pb_eff = quotient(num, den, wsum, pbmin, chan_avg)
    return {'mosaic': mosaic, 'pb_eff': pb_eff, 'num': num, 'den': den, 'wsum': wsum, 'wt': W, 'A': A,
            'bound_num': 1e-11 * NP.einsum('tpk,tk->pk', A, absV) + 1e-12 * absV.sum(axis=0)[NP.newaxis, :],
            'bound_den': 1e-11 * NP.einsum('tpk,tk->pk', A * A, W) + 2e-12 * NP.einsum('tpk,tk->pk', A, W)}


def mosaic(unitvec, rot, pc_dircos, baselines, freqs_hz, cube, setup, weights=None, chan_avg=False, aberr_beta=None, pbmin=0.1):
    sums = snapshot_sums(unitvec, rot, pc_dircos, baselines, freqs_hz, cube, weights=weights, aberr_beta=aberr_beta)
    return combine(sums, beams(sums['s'], freqs_hz, setup), pbmin=pbmin, chan_avg=chan_avg)


def assert_mask_is_decided(ref, pbmin):
    """For a masked-pixel case, before anything is compared: over the (pixel, channel) elements of the channels that carry weight the
    reference masks at least a tenth and keeps at least a tenth, and no Q_ref / (pbmin^2 Wtot) lies within 1e-6 of 1 -- so that the
    device, whose Q differs from Q_ref by rounding, masks the same elements."""
    assert pbmin > 0.0
    live = ref['wsum'] > 0.0
    ratio = ref['den'][:, live] / ((pbmin * pbmin) * ref['wsum'][live])[NP.newaxis, :]
    masked = float(NP.mean(ratio < 1.0))
    assert masked >= 0.1, masked
    assert 1.0 - masked >= 0.1, masked
    assert NP.min(NP.abs(ratio - 1.0)) > 1e-6, NP.min(NP.abs(ratio - 1.0))
    return masked


def setups_of(beam_kind, diameter_m, beam_pc_dircos, ext, nt):
    """The checker's setups, one per snapshot (antpower_checker.beam_of), of a beam as Context.mosaic_image takes it: beam_pc_dircos
    (3,) or (nt, 3); ext None, a dict or one dict per snapshot."""
    element = {_abi.PRISIM_BEAM_DELTA: 'delta', _abi.PRISIM_BEAM_GAUSSIAN: 'gaussian', _abi.PRISIM_BEAM_AIRY: 'dish',
               _abi.PRISIM_BEAM_DIPOLE: 'dipole'}[beam_kind]
    bpc = NP.broadcast_to(NP.asarray(beam_pc_dircos, dtype=NP.float64).reshape(-1, 3), (nt, 3))
    exts = [ext] * nt if ext is None or isinstance(ext, dict) else list(ext)
    assert len(exts) == nt
    out = []
    for t in range(nt):
        x = exts[t] or {}
        setup = {'element': element, 'size': diameter_m, 'element_dircos': NP.asarray(x['dipole_dircos']) if element == 'dipole' else bpc[t]}
        for key in ('array', 'ground', 'beamformer'):
            if x.get(key) is not None:
                setup[key] = x[key]
        out.append(setup)
    return out
