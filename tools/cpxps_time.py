"""Time prisim_cphase_xpower calls on the device and the numpy formulation they replace on the CPU.

    python tools/cpxps_time.py [--nspw 2 --nlst 20 --ndays 1 --ntriads 60 --nlags 256] [--reps 2] [--no-cpu]

Random spectra (nspw, nlst, ndays, ntriads, nlags) crossed over LST (shifts 0 and 1) and triads -- xinfo axes [1, 3] -- and collapsed
over the triads ([3]), then over LST and triads ([1, 3]), for both statistics.  Each call is timed after one warm-up call; kernel_ms,
kernel_bytes and cross_bytes are the entry's own statistics (stream events; the inputs once, every buffer written once and read once
by the next kernel; the size of the uncollapsed product).  The CPU time is tests/cpxps_checker.py:xpower on the same arrays, on this
machine's host.  Prints one JSON line per call; no ratio is asserted."""
import argparse
import json
import os
import sys
import time

import numpy as NP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import cpxps_checker as XK  # noqa: E402
from prisim_amd import _abi  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nspw', type=int, default=2)
    ap.add_argument('--nlst', type=int, default=20)
    ap.add_argument('--ndays', type=int, default=1)
    ap.add_argument('--ntriads', type=int, default=60)
    ap.add_argument('--nlags', type=int, default=256)
    ap.add_argument('--reps', type=int, default=2)
    ap.add_argument('--no-cpu', action='store_true')
    a = ap.parse_args()
    rng = NP.random.default_rng(1)
    shape = (a.nspw, a.nlst, a.ndays, a.ntriads, a.nlags)
    x = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    factor = rng.uniform(0.5, 2.0, a.nspw)
    shifts = [0, 1]
    with _abi.Context(0) as ctx:
        for order in ([3], [1, 3]):
            modes = ('collapse' if 1 in order else 'full', 'none', 'collapse')
            for stat in ('mean', 'median'):
                kw = dict(factor=factor, modes=modes, shifts=shifts, collapse=order, stat=stat)
                res = ctx.cphase_xpower(x, **kw)
                best = None
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    res = ctx.cphase_xpower(x, **kw)
                    dt = (time.perf_counter() - t0) * 1e3
                    if best is None or dt < best[0]:
                        best = (dt, res['stats'])
                st = best[1]
                out = {'shape': list(shape), 'collapse': order, 'stat': stat, 'call_ms': best[0], 'wall_ms': st['wall_ms'],
                       'kernel_ms': st['kernel_ms'], 'kernel_bytes': st['kernel_bytes'],
                       'kernel_gbs': st['kernel_bytes'] / max(st['kernel_ms'], 1e-9) / 1e6, 'cross_bytes': st['cross_bytes'],
                       'chunks': st['chunks'], 'chunk_lags': st['chunk_lags'], 'upload_bytes': st['upload_bytes'],
                       'download_bytes': st['download_bytes']}
                if not a.no_cpu:
                    t0 = time.perf_counter()
                    ref = XK.xpower(x, None, factor, None, modes, shifts, order, stat)
                    out['checker_ms'] = (time.perf_counter() - t0) * 1e3
                    lim = XK.bound(x, None, factor, None, modes, shifts, order, stat)
                    ok = ~XK.cnan(ref)
                    assert NP.array_equal(XK.cnan(res['out']), ~ok)
                    out['error_of_bound'] = float(NP.max(NP.abs(res['out'] - ref)[ok] / lim[ok]))
                print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
