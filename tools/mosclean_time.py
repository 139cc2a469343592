"""The measurement of DESIGN 4.23: per iteration, the update and the search (search image and peak) of Context.clean_mosaic against
kernel_ms of Context.mosaic_image on the same inputs in one process -- HERA-350's 61 075 baselines x 1024 channels x 4 snapshots of a
seeded cube held in the context's resident slots, dircos_grid(64, 0.5) turning by 2 degrees about the zenith per snapshot, an Airy
14 m beam at the zenith, no weights, the stepped route, gain 0.1, maxiter 10, absolute threshold 0; one small warm-up call each, then
--calls calls each, alternated; minimum, median and maximum.

With --entries the process runs Context.mosaic_image, clean_image (one snapshot, maxiter 3, restored), clean_mosaic (maxiter 3, restored,
every optional output) and clean_image_cs (one snapshot, cycle_niter 2, max_major 2, with the beam and the residual visibilities)
alone, once each behind a warm-up, and prints their kernel_ms, the phase times of the CLEANs and a SHA-1 over every array each
returns: run from two trees (--root), it shows that the entries whose kernels moved into shared headers give the same bits and take
the same time.  Prints one JSON line and, with --out, writes it there."""
import argparse
import hashlib
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
    ap.add_argument('--calls', type=int, default=3)
    ap.add_argument('--maxiter', type=int, default=10)
    ap.add_argument('--budget', type=int, default=2 << 30, help='budget_bytes: enough for one resident image')
    ap.add_argument('--entries', action='store_true', help='mosaic_image and the three CLEAN entries alone: their times and a hash of the outputs')
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
    ang = NP.radians(2.0 * NP.arange(nt))
    rot = NP.stack([NP.array([[NP.cos(x), -NP.sin(x), 0.0], [NP.sin(x), NP.cos(x), 0.0], [0.0, 0.0, 1.0]]) for x in ang])
    pc = NP.repeat(NP.array([[0.0, 0.0, 1.0]]), nt, axis=0)
    out = {'root': os.path.abspath(a.root), 'nbl': nbl, 'nchan': nchan, 'nt': nt, 'npix': grid.shape[0], 'terms': grid.shape[0] * nbl * nchan * nt,
           'calls': a.calls, 'maxiter': a.maxiter, 'budget': a.budget}

    def three(values):
        v = sorted(values)
        return [v[0], v[len(v) // 2], v[-1]]

    def digest(*arrays):
        h = hashlib.sha1()
        for x in arrays:
            h.update(NP.ascontiguousarray(x).tobytes())
        return h.hexdigest()

    def entry(r):
        """Of a CLEAN entry's dict: kernel_ms with the phase times, and the hash over every array it returned, by name"""
        row = {k: v for k, v in r['stats'].items() if k.endswith('_ms') and k != 'wall_ms'}
        row['sha1'] = digest(*[r[k] for k in sorted(r) if isinstance(r[k], NP.ndarray)])
        return row

    with _abi.Context(0) as ctx:
        out['device'] = ctx.device_info()
        ctx.set_array(bl, freqs, nt_max=nt)
        slot = NP.empty((nbl, nchan), dtype=NP.complex128)
        for t in range(nt):                                           # the cube goes up a snapshot at a time and stays there
            slot.real = rng.standard_normal((nbl, nchan))
            slot.imag = rng.standard_normal((nbl, nchan))
            ctx.set_vis(slot, slot=t)
        mos = lambda g: ctx.mosaic_image(g, rot, pc, bl, freqs, _abi.PRISIM_BEAM_AIRY, 14.0, route='stepped', budget_bytes=a.budget)      # noqa: E731
        if a.entries:
            img = lambda g: ctx.clean_image(g, rot[:1], pc[:1], bl, freqs, route='stepped', gain=0.1, maxiter=3, threshold=0.0,
                                            threshold_relative=False, fwhm_rad=0.01, budget_bytes=a.budget)      # noqa: E731
            mos(small)
            mosaic, num, den, wsum, st = mos(grid)
            out['mosaic_image'] = {'kernel_ms': st['kernel_ms'], 'sha1': digest(mosaic, num, den, wsum, st['pb_eff'])}
            img(small)
            r = img(grid)
            out['clean_image'] = entry(r)
            cln = lambda g: ctx.clean_mosaic(g, rot, pc, bl, freqs, _abi.PRISIM_BEAM_AIRY, 14.0, route='stepped', gain=0.1, maxiter=3, threshold=0.0,
                                             threshold_relative=False, fwhm_rad=0.01, budget_bytes=a.budget)      # noqa: E731
            cln(small)
            out['clean_mosaic'] = entry(cln(grid))
            ccs = lambda g, n: ctx.clean_image_cs(g, (n, n), rot[:1], pc[:1], bl, freqs, route='stepped', gain=0.1, maxiter=10, threshold=0.0,
                                                  threshold_relative=False, cycle_niter=2, max_major=2, fwhm_rad=0.01, budget_bytes=a.budget,
                                                  want_psf=True, want_vis=True)      # noqa: E731
            ccs(small, 16)
            out['clean_image_cs'] = entry(ccs(grid, a.n))
        else:
            cln = lambda g: ctx.clean_mosaic(g, rot, pc, bl, freqs, _abi.PRISIM_BEAM_AIRY, 14.0, route='stepped', gain=0.1, maxiter=a.maxiter,
                                             threshold=0.0, threshold_relative=False, budget_bytes=a.budget)      # noqa: E731
            mos(small)
            cln(small)
            mrows, crows = [], []
            for _ in range(a.calls):                                  # alternated
                mosaic, num, den, wsum, st = mos(grid)
                mrows.append(st)
                r = cln(grid)
                crows.append(r['stats'])
            its = [c['iterations'] for c in crows]
            out['mosaic_kernel_ms'] = three([m['kernel_ms'] for m in mrows])
            out['clean'] = {'iterations': its, 'components': crows[0]['components'], 'polls': crows[0]['polls'], 'route': crows[0]['route'],
                            'device_bytes': crows[0]['device_bytes'], 'lds_bytes': crows[0]['lds_bytes'],
                            'first_residual_ms': three([c['mosaic_ms'] for c in crows]),
                            'update_ms_per_iteration': three([c['update_ms'] / max(c['iterations'], 1) for c in crows]),
                            'search_ms_per_iteration': three([c['peak_ms'] / (c['iterations'] + 1) for c in crows]),
                            'restore_ms': three([c['restore_ms'] for c in crows]), 'wall_ms': three([c['wall_ms'] for c in crows])}
            out['update_over_mosaic'] = out['clean']['update_ms_per_iteration'][1] / out['mosaic_kernel_ms'][1]
            # with no iteration the call is the mosaic, bit for bit, at this size too
            zero = ctx.clean_mosaic(grid, rot, pc, bl, freqs, _abi.PRISIM_BEAM_AIRY, 14.0, route='stepped', maxiter=0, threshold=0.0,
                                    threshold_relative=False, budget_bytes=a.budget)
            out['maxiter_0_is_the_mosaic'] = bool(NP.array_equal(zero['num'], num) and NP.array_equal(zero['den'], den)
                                                  and NP.array_equal(zero['residual'], mosaic, equal_nan=True))
            out['masked_fraction'] = float(NP.mean(NP.isnan(mosaic)))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
