"""The measurement of DESIGN 4.28: kernel_ms of the fp32 route of Context.dirty_image (precision='single', prisim_dirty_image_f32)
against kernel_ms of the fp64 stepped route on the same inputs in one process -- HERA-350's 61 075 baselines x 1024 channels of
97.656 kHz from 100 MHz x 1 snapshot of a seeded host cube, no weights, dircos_grid(64, 0.5); one small warm-up call per entry, then
--calls calls each, alternated; minimum, median and maximum.  The two images are compared over every element in units of the scale
sum|V| / (nt nbl).  Prints one JSON line and, with --out, writes it there."""
import argparse
import json
import os
import sys

import numpy as NP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from prisim_amd import _abi, layouts as LAY  # noqa: E402
from prisim_amd import interferometry as RI  # noqa: E402

FLOP_PER_TERM = 10                     # one complex multiply (two products, two FMAs) and two FMAs into the sum, in either precision
PEAK = {'double': 78.6e12, 'single': 157.3e12}      # datasheet vector peaks of the MI355X, flop/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=64)
    ap.add_argument('--nbl', type=int, default=0, help='the first nbl baselines only (0: all)')
    ap.add_argument('--nchan', type=int, default=1024)
    ap.add_argument('--calls', type=int, default=3)
    ap.add_argument('--kind', choices=('dirty', 'psf'), default='dirty')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    bl = LAY.layout_baselines('HERA-350')[0]
    bl = NP.ascontiguousarray(bl[:a.nbl] if a.nbl else bl, dtype=NP.float64)
    nbl, nchan, nt = bl.shape[0], a.nchan, 1
    freqs = 100e6 + 97656.25 * NP.arange(nchan)
    grid = RI.ApertureSynthesis.dircos_grid(a.n, 0.5)
    rng = NP.random.default_rng(20261021)
    cube = NP.empty((nt, nbl, nchan), dtype=NP.complex128)
    cube[0].real = rng.standard_normal((nbl, nchan))
    cube[0].imag = rng.standard_normal((nbl, nchan))
    rot, pc = NP.eye(3)[NP.newaxis], NP.array([[0.0, 0.0, 1.0]])
    small = RI.ApertureSynthesis.dircos_grid(16, 0.5)
    terms = grid.shape[0] * nbl * nchan * nt
    out = {'nbl': nbl, 'nchan': nchan, 'nt': nt, 'npix': grid.shape[0], 'terms': terms, 'calls': a.calls, 'kind': a.kind}

    with _abi.Context(0) as ctx:
        out['device'] = ctx.device_info()
        run = lambda g, precision: ctx.dirty_image(g, rot, pc, bl, freqs, cube=cube, kind=a.kind, route='stepped', precision=precision)  # noqa: E731
        for precision in PEAK:
            run(small, precision)
        rows, image = {p: [] for p in PEAK}, {}
        for _ in range(a.calls):
            for precision in PEAK:
                image[precision], _, st = run(grid, precision)
                rows[precision].append(st)
    for precision, sts in rows.items():
        ms = sorted(r['kernel_ms'] for r in sts)
        wall = sorted(r['wall_ms'] for r in sts)
        rate = terms / (ms[len(ms) // 2] * 1e-3)
        out[precision] = {'kernel_ms': [ms[0], ms[len(ms) // 2], ms[-1]], 'wall_ms': [wall[0], wall[-1]], 'chunks': sts[0]['chunks'],
                          'streams': sts[0]['streams'], 'route': sts[0]['route'], 'lds_bytes': sts[0]['lds_bytes'], 'terms_per_s': rate,
                          'of_vector_peak': rate * FLOP_PER_TERM / PEAK[precision]}
    out['ratio_of_medians_double_over_single'] = out['double']['kernel_ms'][1] / out['single']['kernel_ms'][1]
    scale = 1.0 if a.kind == 'psf' else NP.abs(cube).sum(axis=(0, 1)) / (nt * nbl)
    out['single_minus_double_over_scale'] = float(NP.max(NP.abs(image['single'] - image['double']) / scale))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
