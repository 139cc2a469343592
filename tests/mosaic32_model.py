"""numpy restatement of the chain of prisim_mosaic_image_f32 (include/prisim_mosaic32.h, prisim_amd/csrc_imaging/mosaic32_kernels.h),
TEST INFRASTRUCTURE and never the reference: it shows on the CPU, before any device run, what the chain can hold against
tests/mosaic_checker.py.

Per snapshot, D_t is the float32 chain of tests/imaging32_model.py on that snapshot alone: the seed at the tile's centre, the
recurrence with FMA rounding, the flush every 64 rows and at the snapshot's end.  That model returns D_t / W_t; it is multiplied back by
W_t here (two float64 roundings, 2e-16 of D_t, against a bound of 2.5e-6 -- one more reason this is a model and no bit oracle), and a
channel without weight, where every operand is zero, gets D_t = 0 as the device has it.  Then the float64 epilogue of the header in t
order, N = fma(A, D_t, N) and Q = fma(A A, W_t, Q), with the beams and the weight sums of the checker.  The fused multiply-add is
formed from error-free transformations (Dekker's product, Knuth's sum): a b + c = s + (t + e) exactly with s = fl(fl(a b) + c), and
fl(s + fl(t + e)) is the correctly rounded sum unless it lies within 2^-100 of a tie.  A long double would not do: its second
rounding changes one result in two thousand.  tests/test_mosaic32.py holds Q against the same statement in exact rationals."""
import numpy as NP

import imaging32_model as M
import imaging_checker as IK

SPLIT = 134217729.0                                                  # 2^27 + 1: Veltkamp's splitter for a 53-bit significand


def _split(a):
    c = SPLIT * a
    hi = c - (c - a)
    return hi, a - hi


def fma64(a, b, c):
    """float64(a b + c) with one rounding, elementwise; for finite operands far from overflow"""
    a, b, c = NP.broadcast_arrays(NP.asarray(a, dtype=NP.float64), NP.asarray(b, dtype=NP.float64), NP.asarray(c, dtype=NP.float64))
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl                 # p + e = a b exactly
    s = p + c
    v = s - p
    t = (p - (s - v)) + (c - v)                                       # s + t = p + c exactly
    return s + (t + e)


def snapshot_sum(t, unitvec, rot, pc_dircos, baselines, freqs_hz, cube, w, aberr_beta=None):
    """D_t (npix, nchan) float64 as the device's fp32 chain forms it; w (nt, nbl, nchan) the full weights"""
    beta = None if aberr_beta is None else NP.asarray(aberr_beta)[t:t + 1]
    img = M.dirty_image(unitvec, NP.asarray(rot)[t:t + 1], NP.asarray(pc_dircos).reshape(-1, 3)[t:t + 1], baselines, freqs_hz,
                        cube=NP.asarray(cube)[t:t + 1], weights=w[t:t + 1], aberr_beta=beta)
    Wt = NP.einsum('bk->k', w[t])
    return NP.where(Wt > 0.0, NP.nan_to_num(img) * Wt, 0.0)


def epilogue(D, A, W):
    """(N, Q) (npix, nchan) from D (nt, npix, nchan), A (nt, npix, nchan) and W (nt, nchan) by the header's statements, t ascending"""
    N, Q = NP.zeros(D.shape[1:]), NP.zeros(D.shape[1:])
    for t in range(D.shape[0]):
        N = fma64(A[t], D[t], N)
        Q = fma64(A[t] * A[t], NP.broadcast_to(W[t], Q.shape), Q)
    return N, Q


def mosaic_sums(unitvec, rot, pc_dircos, baselines, freqs_hz, cube, A, weights=None, aberr_beta=None):
    """{'num', 'den'} of the model for the beams A (nt, npix, nchan) of the checker"""
    nt, nbl, nchan = A.shape[0], NP.asarray(baselines).reshape(-1, 3).shape[0], NP.asarray(freqs_hz).size
    w = NP.asarray(IK.full_weights(weights, nt, nbl, nchan), dtype=NP.float64)
    D = NP.stack([snapshot_sum(t, unitvec, rot, pc_dircos, baselines, freqs_hz, cube, w, aberr_beta) for t in range(nt)])
    N, Q = epilogue(D, A, NP.einsum('tbk->tk', w))
    return {'num': N, 'den': Q, 'D': D}
