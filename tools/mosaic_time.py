"""The measurement of DESIGN 4.22: kernel_ms of Context.mosaic_image against kernel_ms of Context.dirty_image on the same inputs in
one process -- HERA-350's 61 075 baselines x 1024 channels x 4 snapshots of a seeded host cube, dircos_grid(128, 0.5), an Airy 14 m
beam at the zenith, the stepped route; one small warm-up call each, then --calls calls each, minimum, median and maximum.  Two pixels
of the mosaic are compared with the numpy checker at the full size.  With --only mosaic the process runs the mosaic alone, for a
kernel trace that gives the share of every kernel.  Prints one JSON line and, with --out, writes it there."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=128)
    ap.add_argument('--nbl', type=int, default=0, help='the first nbl baselines only (0: all)')
    ap.add_argument('--nchan', type=int, default=1024)
    ap.add_argument('--nt', type=int, default=4)
    ap.add_argument('--calls', type=int, default=3)
    ap.add_argument('--budget', type=int, default=0, help='budget_bytes of the mosaic (0: the default 1 GiB)')
    ap.add_argument('--only', choices=('both', 'mosaic'), default='both')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    bl = LAY.layout_baselines('HERA-350')[0]
    bl = NP.ascontiguousarray(bl[:a.nbl] if a.nbl else bl, dtype=NP.float64)
    nbl, nchan, nt = bl.shape[0], a.nchan, a.nt
    freqs = 100e6 + 97656.25 * NP.arange(nchan)
    grid = RI.ApertureSynthesis.dircos_grid(a.n, 0.5)
    rng = NP.random.default_rng(20261019)
    cube = NP.empty((nt, nbl, nchan), dtype=NP.complex128)
    for t in range(nt):
        cube[t].real = rng.standard_normal((nbl, nchan))
        cube[t].imag = rng.standard_normal((nbl, nchan))
    # a drift of two degrees of hour angle per snapshot about the zenith, in the manner of rot_z: the pixels stay up
    ang = NP.radians(2.0 * NP.arange(nt))
    rot = NP.stack([NP.array([[NP.cos(x), -NP.sin(x), 0.0], [NP.sin(x), NP.cos(x), 0.0], [0.0, 0.0, 1.0]]) for x in ang])
    pc = NP.repeat(NP.array([[0.0, 0.0, 1.0]]), nt, axis=0)
    small = RI.ApertureSynthesis.dircos_grid(16, 0.5)
    out = {'nbl': nbl, 'nchan': nchan, 'nt': nt, 'npix': grid.shape[0], 'terms': grid.shape[0] * nbl * nchan * nt, 'calls': a.calls, 'budget': a.budget}

    def stats(rows):
        ms = sorted(r['kernel_ms'] for r in rows)
        wall = sorted(r['wall_ms'] for r in rows)
        return {'kernel_ms': [ms[0], ms[len(ms) // 2], ms[-1]], 'wall_ms': [wall[0], wall[-1]], 'chunks': rows[0]['chunks'],
                'streams': rows[0]['streams'], 'route': rows[0]['route'], 'kernel_bytes': rows[0]['kernel_bytes']}

    with _abi.Context(0) as ctx:
        out['device'] = ctx.device_info()
        mos = lambda g: ctx.mosaic_image(g, rot, pc, bl, freqs, _abi.PRISIM_BEAM_AIRY, 14.0, cube=cube, route='stepped',
                                           budget_bytes=a.budget)      # noqa: E731
        img = lambda g: ctx.dirty_image(g, rot, pc, bl, freqs, cube=cube, route='stepped')      # noqa: E731
        mos(small)
        rows = []
        for _ in range(a.calls):
            mosaic, num, den, wsum, st = mos(grid)
            rows.append(st)
        out['mosaic'] = stats(rows)
        if a.only == 'both':
            img(small)
            rows = [img(grid)[2] for _ in range(a.calls)]
            out['image'] = stats(rows)
            out['ratio_of_medians'] = out['mosaic']['kernel_ms'][1] / out['image']['kernel_ms'][1]
            import mosaic_checker as MK
            pix = NP.array([a.n * (a.n // 2) + a.n // 2 + 3, 5 * a.n + 7])          # one near the beam's centre, one far out
            # one (pixel, snapshot) at a time: the checker's phases of 61 075 x 1024 terms are 1 GB
            parts = [[MK.snapshot_sums(grid[p:p + 1], rot[t:t + 1], pc[t:t + 1], bl, freqs, cube[t:t + 1]) for p in pix] for t in range(nt)]
            sums = {'D': NP.stack([NP.concatenate([x['D'][0] for x in row]) for row in parts]),
                    's': NP.stack([NP.concatenate([x['s'][0] for x in row]) for row in parts]),
                    'W': NP.stack([row[0]['W'][0] for row in parts]), 'absV': NP.stack([row[0]['absV'][0] for row in parts])}
            ref = MK.combine(sums, MK.beams(sums['s'], freqs, {'element': 'dish', 'size': 14.0}))
            out['two_pixels'] = {'num_err_over_bound': float(NP.max(NP.abs(num[pix] - ref['num']) / ref['bound_num'])),
                                 'den_err_over_bound': float(NP.max(NP.abs(den[pix] - ref['den']) / ref['bound_den'])),
                                 'pb_eff': [float(st['pb_eff'][p].mean()) for p in pix]}
        out['masked_fraction'] = float(NP.mean(NP.isnan(mosaic)))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
