"""Time one prisim_cphase_ft call on the device and the numpy formulation it replaces on the CPU.

    python tools/cpft_time.py [--nlst 20 --ndays 4 --ntriads 30 --nchan 1024] [--pad 1.0] [--nwin 2] [--nin 2] [--reps 2] [--no-cpu]

Random stacks (nlst, ndays, ntriads, nchan): --nin inputs, integer weights with some rows of zeros, --nwin windows, a scale.  The
call is timed after one warm-up call; kernel_ms and kernel_bytes are the entry's own statistics (stream events; every input and every
output counted once).  The CPU time is tests/cpft_checker.py:transform on the same arrays.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as NP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import cpft_checker as FK  # noqa: E402
from prisim_amd import _abi  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nlst', type=int, default=20)
    ap.add_argument('--ndays', type=int, default=4)
    ap.add_argument('--ntriads', type=int, default=30)
    ap.add_argument('--nchan', type=int, default=1024)
    ap.add_argument('--pad', type=float, default=1.0)
    ap.add_argument('--nwin', type=int, default=2)
    ap.add_argument('--nin', type=int, default=2)
    ap.add_argument('--reps', type=int, default=2)
    ap.add_argument('--route', default='auto')
    ap.add_argument('--no-cpu', action='store_true')
    a = ap.parse_args()
    rng = NP.random.default_rng(1)
    lead = (a.nlst, a.ndays, a.ntriads)
    m = a.nchan + int(a.nchan * a.pad)
    nres = max(m // 8, 1)
    inputs = [rng.standard_normal(lead + (a.nchan,)) + 1j * rng.standard_normal(lead + (a.nchan,)) for _ in range(a.nin)]
    w = rng.integers(0, 5, lead + (a.nchan,)).astype(NP.float64)
    w[0, 0, :, :] = 0.0
    wts = rng.uniform(size=(a.nwin, a.nchan))
    vs = rng.uniform(0.5, 2.0, (a.nwin, a.nlst))
    out = {'shape': list(lead) + [a.nchan], 'm': m, 'nres': nres, 'nwin': a.nwin, 'nin': a.nin}
    with _abi.Context(0) as ctx:
        res = ctx.cphase_ft(inputs, wts, m, 1e5, weights=w, vscale=vs, nres=nres, route=a.route)
        best = None
        for _ in range(a.reps):
            t0 = time.perf_counter()
            res = ctx.cphase_ft(inputs, wts, m, 1e5, weights=w, vscale=vs, nres=nres, route=a.route)
            dt = (time.perf_counter() - t0) * 1e3
            if best is None or dt < best[0]:
                best = (dt, res['stats'])
    st = best[1]
    out.update({'call_ms': best[0], 'wall_ms': st['wall_ms'], 'kernel_ms': st['kernel_ms'], 'kernel_bytes': st['kernel_bytes'],
                'kernel_gbs': st['kernel_bytes'] / max(st['kernel_ms'], 1e-9) / 1e6, 'route': st['route'], 'chunks': st['chunks'],
                'group_rows': st['group_rows'], 'lds_bytes': st['lds_bytes'], 'upload_bytes': st['upload_bytes'],
                'download_bytes': st['download_bytes']})
    if not a.no_cpu:
        t0 = time.perf_counter()
        ref = FK.transform(inputs, wts, m, 1e5, weights=w, vscale=vs, nres=nres)
        out['checker_ms'] = (time.perf_counter() - t0) * 1e3
        out['error'] = max(FK.spectrum_error(res[k][i], ref[k][i], ref['xsum'][i], 1e5) for k in ('over', 'res') for i in range(a.nin))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
