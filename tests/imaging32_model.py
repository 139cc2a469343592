"""numpy float32 restatement of the chain of prisim_dirty_image_f32 (include/prisim_imaging32.h, prisim_amd/csrc_imaging/
imaging32_kernels.h), TEST INFRASTRUCTURE and never the reference: it shows on the CPU, before any device run, what the chosen chain --
seed position, step, recurrence, flush interval, all read from the constants of prisim_amd/csrc_addon/imaging32_plan.h -- can hold
against tests/imaging_checker.py.

What it states as the device does: tau, f tau and df tau in float64; the quadrant reduction and the polynomials of sincos_qcycles
(prisim_amd/csrc_imaging/sincos_qcycles32.h) in float32; the operand formed in float64 and rounded once; the seed at the tile's centre channel
from f[k0] + 16 df, walked down over [0, 16) and up over [16, 32) by one complex multiply a channel (two rounded products, two fused
multiply-adds); float32 partial sums, one per row of a pair, added into float64 totals every `flush` rows, the even row's before the
odd row's.  A fused multiply-add is float32(float64(a) float64(b) + float64(c)): the product is exact in float64, and the sum is
rounded twice where the device rounds once -- a difference of an ulp in rare ties, which is why this is a model and no bit oracle.
The order of the terms is the device's; the weight sums are the checker's."""
import os
import re

import numpy as NP

import imaging_cases as IC
import imaging_checker as IK

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = NP.float32, NP.float64
KINVC = 1.0 / 299792458.0


def plan_constants():
    """{name: value} of the integer constants of imaging32_plan.h and the tile of imaging_plan.h, from their text."""
    out = {}
    for header in ('imaging_plan.h', 'imaging32_plan.h'):
        txt = open(os.path.join(ROOT, 'prisim_amd', 'csrc_addon', header)).read()
        out.update({n: int(v) for n, v in re.findall(r'constexpr int (kImaging\w+) = (\d+);', txt)})
    return out


PLAN = plan_constants()
TILE, ROWS, FLUSH, SEED = PLAN['kImagingTile'], PLAN['kImaging32Rows'], PLAN['kImaging32Flush'], PLAN['kImaging32Seed']


def fma(a, b, c):
    return (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(F32)


def sincos_qcycles(a4):
    """(cos, sin) of 2 pi a4 / 4 as float32: sincos_qcycles(double, float&, float&), operation by operation."""
    q = NP.rint(a4)
    y = ((a4 - q) * 0.25).astype(F32)
    qi = q.astype(NP.int64)
    y2 = y * y
    ps = NP.full_like(y, F32(42.058693944897655))
    for coef in (-76.70585975306136, 81.60524927607504, -41.341702240399755):
        ps = fma(ps, y2, NP.full_like(y, F32(coef)))
    sy = fma(y * y2, ps, y * F32(6.2831855))
    sy = fma(y, NP.full_like(y, F32(-1.7484555e-7)), sy)
    pc = NP.full_like(y, F32(-26.42625678337438))
    for coef in (60.24464137187666, -85.45681720669373, 64.93939402266829, -19.739208802178716, 1.0):
        pc = fma(pc, y2, NP.full_like(y, F32(coef)))
    swap = (qi & 1) != 0
    cc, ss = NP.where(swap, sy, pc), NP.where(swap, pc, sy)
    return NP.where(((qi + 1) & 2) != 0, -cc, cc), NP.where((qi & 2) != 0, -ss, ss)


def dirty_image(unitvec, rot, pc_dircos, baselines, freqs_hz, cube=None, weights=None, kind='dirty', chan_avg=False, aberr_beta=None,
                flush=FLUSH, seed=SEED):
    """The image as the device's chain forms it, (npix, nchan) or (npix,) float64.  flush: rows between two additions of the float32
    partial sums into the float64 totals, even and counted from the first baseline of every snapshot; 0: never within a snapshot."""
    bl = NP.asarray(baselines, dtype=F64).reshape(-1, 3)
    fq = NP.asarray(freqs_hz, dtype=F64).ravel()
    d = IK.directions(unitvec, rot, aberr_beta) - NP.asarray(pc_dircos, dtype=F64).reshape(-1, 1, 3)     # (nt, npix, 3), as k_img_dirs
    nt, npix, nbl, nchan = d.shape[0], d.shape[1], bl.shape[0], fq.size
    w = NP.asarray(IK.full_weights(weights, nt, nbl, nchan), dtype=F64)
    df = (fq[-1] - fq[0]) / (nchan - 1) if nchan > 1 else 0.0
    flush = int(flush) if flush else nbl + (nbl & 1)
    assert flush % 2 == 0 and seed * 2 == TILE
    ngroup = (nbl + flush - 1) // flush
    pad = ngroup * flush - nbl
    b = NP.concatenate((bl * KINVC, NP.zeros((pad, 3))))              # rows past the last baseline: a zero baseline and a zero operand
    D = NP.zeros((npix, nchan))
    for k0 in range(0, nchan, TILE):
        live = min(TILE, nchan - k0)
        fc, df4 = fq[k0] + float(seed) * df, 4.0 * df
        for t in range(nt):
            if kind == 'psf':
                x, y = w[t, :, k0:k0 + live].astype(F32), None
            else:
                v = NP.asarray(cube)[t, :, k0:k0 + live]
                x, y = (w[t, :, k0:k0 + live] * v.real).astype(F32), (w[t, :, k0:k0 + live] * v.imag).astype(F32)
            x = NP.concatenate((x, NP.zeros((pad, live), dtype=F32))).reshape(ngroup, flush // 2, 2, live)
            y = None if y is None else NP.concatenate((y, NP.zeros((pad, live), dtype=F32))).reshape(ngroup, flush // 2, 2, live)
            tau = ((b[:, NP.newaxis, 0] * d[t, :, 0] + b[:, NP.newaxis, 1] * d[t, :, 1]) + b[:, NP.newaxis, 2] * d[t, :, 2])
            tau = tau.reshape(ngroup, flush // 2, 2, npix)
            acc = NP.zeros((live, ngroup, 2, npix), dtype=F32)
            for j in range(flush // 2):
                turns = fc * tau[:, j]
                c, s = sincos_qcycles(4.0 * (turns - NP.rint(turns)))
                sc, ss = sincos_qcycles(df4 * tau[:, j])
                cu, su, cd, sd = c, s, c, s
                for i in range(seed):
                    cd, sd = fma(cd, sc, sd * ss), fma(sd, sc, -(cd * ss))
                    k = seed - 1 - i
                    if k < live:
                        acc[k] = fma(x[:, j, :, k, NP.newaxis], cd, acc[k])
                        if y is not None:
                            acc[k] = fma(-y[:, j, :, k, NP.newaxis], sd, acc[k])
                    k = seed + i
                    if k < live:
                        acc[k] = fma(x[:, j, :, k, NP.newaxis], cu, acc[k])
                        if y is not None:
                            acc[k] = fma(-y[:, j, :, k, NP.newaxis], su, acc[k])
                    if i + 1 < seed and seed + i + 1 < live:
                        cu, su = fma(cu, sc, -(su * ss)), fma(cu, ss, su * sc)
            for g in range(ngroup):
                D[:, k0:k0 + live] = (D[:, k0:k0 + live] + acc[:, g, 0].T.astype(F64)) + acc[:, g, 1].T.astype(F64)
    W = NP.einsum('tbk->k', w)
    with NP.errstate(invalid='ignore', divide='ignore'):
        return D.sum(axis=1) / W.sum() if chan_avg else D / W


def coherent_case(nbl=20000, npix=65):
    """The inputs of the coherent-accumulation test: imaging_cases.case(nbl, 2, npix, 1) seen in its own frame (the identity, no
    aberration) with the phase centre at the zenith and the first direction on it, so that there tau is 0 exactly and every term of the
    beam is the weight itself."""
    c = IC.case(nbl, 2, npix, 1)
    c['rot'], c['beta'], c['pc'] = NP.eye(3)[NP.newaxis], None, NP.array([[0.0, 0.0, 1.0]])
    c['unitvec'][0] = [0.0, 0.0, 1.0]
    return c
