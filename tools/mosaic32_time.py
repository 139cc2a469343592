"""The measurement of DESIGN 4.29: kernel_ms of the fp32 route of Context.mosaic_image (precision='single', prisim_mosaic_image_f32)
against kernel_ms of the fp64 stepped route on the same inputs in one process -- HERA-350's 61 075 baselines x 1024 channels of
97.656 kHz from 100 MHz x 4 snapshots of a seeded host cube, no weights, a 14 m Gaussian at the zenith, dircos_grid(64, 0.5); one small
warm-up call per entry, then --calls calls each, alternated; minimum, median and maximum.  The two mosaics are compared over every
unmasked element in units of the scale sum_t A_t sum_b |V| / Q, and den, wsum, pb_eff and the mask for equality.  Prints one JSON line
and, with --out, writes it there."""
import argparse
import json
import os
import sys

import numpy as NP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from prisim_amd import _abi, layouts as LAY  # noqa: E402
from prisim_amd import interferometry as RI  # noqa: E402
import mosaic_checker as MK  # noqa: E402

PRECISIONS = ('double', 'single')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=64)
    ap.add_argument('--nbl', type=int, default=0, help='the first nbl baselines only (0: all)')
    ap.add_argument('--nchan', type=int, default=1024)
    ap.add_argument('--nt', type=int, default=4)
    ap.add_argument('--calls', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    bl = LAY.layout_baselines('HERA-350')[0]
    bl = NP.ascontiguousarray(bl[:a.nbl] if a.nbl else bl, dtype=NP.float64)
    nbl, nchan, nt = bl.shape[0], a.nchan, a.nt
    freqs = 100e6 + 97656.25 * NP.arange(nchan)
    grid = RI.ApertureSynthesis.dircos_grid(a.n, 0.5)
    rng = NP.random.default_rng(20261021)
    cube = NP.empty((nt, nbl, nchan), dtype=NP.complex128)
    for t in range(nt):
        cube[t].real = rng.standard_normal((nbl, nchan))
        cube[t].imag = rng.standard_normal((nbl, nchan))
    # a drift of two degrees of hour angle per snapshot about the zenith (tools/mosaic_time.py): the pixels stay up
    ang = NP.radians(2.0 * NP.arange(nt))
    rot = NP.stack([NP.array([[NP.cos(x), -NP.sin(x), 0.0], [NP.sin(x), NP.cos(x), 0.0], [0.0, 0.0, 1.0]]) for x in ang])
    pc = NP.repeat(NP.array([[0.0, 0.0, 1.0]]), nt, axis=0)
    small = RI.ApertureSynthesis.dircos_grid(16, 0.5)
    terms = grid.shape[0] * nbl * nchan * nt
    out = {'nbl': nbl, 'nchan': nchan, 'nt': nt, 'npix': grid.shape[0], 'terms': terms, 'calls': a.calls, 'beam': 'gaussian 14 m'}

    with _abi.Context(0) as ctx:
        out['device'] = ctx.device_info()
        run = lambda g, precision: ctx.mosaic_image(g, rot, pc, bl, freqs, _abi.PRISIM_BEAM_GAUSSIAN, 14.0, cube=cube, route='stepped',
                                                    precision=precision)      # noqa: E731
        for precision in PRECISIONS:
            run(small, precision)
        rows, got = {p: [] for p in PRECISIONS}, {}
        for _ in range(a.calls):
            for precision in PRECISIONS:
                got[precision] = run(grid, precision)
                rows[precision].append(got[precision][4])
    for precision, sts in rows.items():
        ms = sorted(r['kernel_ms'] for r in sts)
        wall = sorted(r['wall_ms'] for r in sts)
        out[precision] = {'kernel_ms': [ms[0], ms[len(ms) // 2], ms[-1]], 'wall_ms': [wall[0], wall[-1]], 'chunks': sts[0]['chunks'],
                          'streams': sts[0]['streams'], 'route': sts[0]['route'], 'lds_bytes': sts[0]['lds_bytes'],
                          'kernel_bytes': sts[0]['kernel_bytes'], 'terms_per_s': terms / (ms[len(ms) // 2] * 1e-3)}
    out['ratio_of_medians_double_over_single'] = out['double']['kernel_ms'][1] / out['single']['kernel_ms'][1]
    m32, n32, q32, w32, s32 = got['single']
    m64, n64, q64, w64, s64 = got['double']
    out['den_wsum_pb_eff_and_mask_equal'] = bool(NP.array_equal(q32, q64) and NP.array_equal(w32, w64) and
                                                 NP.array_equal(s32['pb_eff'], s64['pb_eff'], equal_nan=True) and
                                                 NP.array_equal(NP.isnan(m32), NP.isnan(m64)))
    out['masked_fraction'] = float(NP.mean(NP.isnan(m64)))
    # the scale of the mosaic: sum_t A_t sum_b |V| / Q per element, with the beam of the numpy checker at the directions of every
    # snapshot (no weights: w = 1)
    s = NP.einsum('tij,pj->tpi', rot, grid)
    absv = NP.abs(cube).sum(axis=1)                                   # (nt, nchan)
    A = MK.beams(s, freqs, {'element': 'gaussian', 'size': 14.0})
    scale = NP.einsum('tpk,tk->pk', A, absv) / q64
    keep = ~NP.isnan(m64)
    out['single_minus_double_over_scale'] = float(NP.max(NP.abs(m32 - m64)[keep] / scale[keep]))
    out['num_single_minus_double_over_5e-6_scale'] = float(NP.max(NP.abs(n32 - n64)[keep] / (5e-6 * (scale * q64)[keep])))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
