"""The measurement of DESIGN 4.27: kernel_ms of Context.clean_mosaic_cs, split by phase, against kernel_ms of Context.clean_mosaic on the
same inputs in one process -- the setting of DESIGN 4.23: HERA-350's 61 075 baselines x 1024 channels x 4 snapshots x
dircos_grid(64, 0.5) turning by 2 degrees about the zenith per snapshot, an Airy 14 m beam at the zenith, a seeded random host cube,
no weights, the stepped route, gain 0.1, absolute threshold 0, maxiter 100; the cycles with cycle_niter 25 and max_major 4 (so 4 cycles
of 25 components per channel, 5 mosaic passes).  budget_bytes is given: the call holds some 4.5 GB, 4.0 GB of them the residual
visibilities.  One small warm-up call each, then --calls calls each, alternated.  Prints one JSON line and, with --out, writes it
there."""
import argparse
import json
import os
import sys

import numpy as NP


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help='the tree whose package is imported')
    ap.add_argument('--n', type=int, default=64)
    ap.add_argument('--nbl', type=int, default=0, help='the first nbl baselines only (0: all)')
    ap.add_argument('--nchan', type=int, default=1024)
    ap.add_argument('--nt', type=int, default=4)
    ap.add_argument('--calls', type=int, default=2)
    ap.add_argument('--maxiter', type=int, default=100)
    ap.add_argument('--cycle-niter', type=int, default=25)
    ap.add_argument('--max-major', type=int, default=4)
    ap.add_argument('--budget', type=int, default=5 << 30, help='budget_bytes: the residual visibilities alone take 4.0e9 B')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    from prisim_amd import _abi, layouts as LAY
    from prisim_amd import interferometry as RI
    bl = LAY.layout_baselines('HERA-350')[0]
    bl = NP.ascontiguousarray(bl[:a.nbl] if a.nbl else bl, dtype=NP.float64)
    nbl, nchan, nt = bl.shape[0], a.nchan, a.nt
    freqs = 100e6 + 97656.25 * NP.arange(nchan)
    grid = RI.ApertureSynthesis.dircos_grid(a.n, 0.5)
    small = RI.ApertureSynthesis.dircos_grid(16, 0.5)
    rng = NP.random.default_rng(20261020)
    cube = NP.empty((nt, nbl, nchan), dtype=NP.complex128)
    for t in range(nt):
        cube[t].real = rng.standard_normal((nbl, nchan))
        cube[t].imag = rng.standard_normal((nbl, nchan))
    ang = NP.radians(2.0 * NP.arange(nt))
    rot = NP.stack([NP.array([[NP.cos(x), -NP.sin(x), 0.0], [NP.sin(x), NP.cos(x), 0.0], [0.0, 0.0, 1.0]]) for x in ang])
    pc = NP.repeat(NP.array([[0.0, 0.0, 1.0]]), nt, axis=0)
    kw = dict(cube=cube, route='stepped', gain=0.1, maxiter=a.maxiter, threshold=0.0, threshold_relative=False, budget_bytes=a.budget)
    out = {'root': os.path.abspath(a.root), 'nbl': nbl, 'nchan': nchan, 'nt': nt, 'npix': grid.shape[0], 'terms': grid.shape[0] * nbl * nchan * nt,
           'calls': a.calls, 'maxiter': a.maxiter, 'cycle_niter': a.cycle_niter, 'max_major': a.max_major, 'budget': a.budget}
    with _abi.Context(0) as ctx:
        out['device'] = ctx.device_info()
        hog = lambda g: ctx.clean_mosaic(g, rot, pc, bl, freqs, _abi.PRISIM_BEAM_AIRY, 14.0, **kw)      # noqa: E731
        cyc = lambda g, n: ctx.clean_mosaic_cs(g, (n, n), rot, pc, bl, freqs, _abi.PRISIM_BEAM_AIRY, 14.0, cycle_depth=0.3, cycle_niter=a.cycle_niter,
                                               max_major=a.max_major, **kw)      # noqa: E731
        hog(small)
        cyc(small, 16)
        hrows, crows = [], []
        for _ in range(a.calls):                                      # alternated
            crows.append(cyc(grid, a.n))
            hrows.append(hog(grid))
        keys = ('kernel_ms', 'psf_ms', 'beam_ms', 'mosaic_ms', 'peak_ms', 'minor_ms', 'model_ms', 'restore_ms', 'wall_ms', 'cycles', 'components', 'polls',
                'minor_route', 'minor_lds_bytes', 'device_bytes', 'psf_offsets')
        out['cycles'] = [{k: r['stats'][k] for k in keys} for r in crows]
        out['cycles_status'] = sorted(set(crows[0]['status'].tolist()))
        out['cycles_peak_over_peak0'] = float(NP.nanmax(crows[0]['cycle_peak'][:, -1] / crows[0]['peak0']))
        out['hogbom'] = [{k: r['stats'][k] for k in ('kernel_ms', 'mosaic_ms', 'peak_ms', 'update_ms', 'restore_ms', 'wall_ms', 'iterations', 'components')}
                         for r in hrows]
        out['hogbom_peak_over_peak0'] = float(NP.nanmax(NP.nanmax(NP.abs(hrows[0]['residual_flat']), axis=0) / hrows[0]['peak0']))
        out['masked_fraction'] = float(NP.mean(NP.isnan(crows[0]['residual'])))
        out['kernel_ms_ratio'] = max(c['kernel_ms'] for c in out['cycles']) / min(h['kernel_ms'] for h in out['hogbom'])
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
