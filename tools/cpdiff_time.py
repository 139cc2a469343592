"""Time one ClosurePhase.subsample_differencing(ndaybins=..., lstbinsize=...) call on the device.

    python tools/cpdiff_time.py [--nlst 60 --ndays 18 --ntriads 30 --nchan 1024] [--ndaybins 6] [--reps 2] [--hbm-gbs 8000]

The stack is that of tools/cphase_bins_time.py.  The call is timed on the host clock after one warm-up call, the native stack already
resident; kernel_ms and kernel_bytes are the entries' own statistics (stream events; every input element counted once, every output
once), and their quotient is set against --hbm-gbs, the peak HBM bandwidth of the device in GB/s.  The weights of the difference step
are compared with numpy's square root on the downloaded arrays' own inputs.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as NP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from cphase_bins_time import make_raw  # noqa: E402
from prisim_amd import _abi  # noqa: E402
from prisim_amd import bispectrum_phase as BSP  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nlst', type=int, default=60)
    ap.add_argument('--ndays', type=int, default=18)
    ap.add_argument('--ntriads', type=int, default=30)
    ap.add_argument('--nchan', type=int, default=1024)
    ap.add_argument('--ndaybins', type=int, default=6)
    ap.add_argument('--lstbinsize', type=float, default=600.0)
    ap.add_argument('--reps', type=int, default=2)
    ap.add_argument('--hbm-gbs', type=float, default=8000.0)
    a = ap.parse_args()
    raw = make_raw(a.nlst, a.ndays, a.ntriads, a.nchan)
    kw = {'ndaybins': a.ndaybins, 'lstbinsize': a.lstbinsize}
    out = {'shape': [a.nlst, a.ndays, a.ntriads, a.nchan], 'ndaybins': a.ndaybins}
    with _abi.Context(0) as ctx:
        cp = BSP.ClosurePhase({'raw': raw}, 150e6 + 1e5 * NP.arange(a.nchan), ctx=ctx)
        cp._native_stack()
        cp.subsample_differencing(**kw)                                 # warm-up
        walls, kernels = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            cp.subsample_differencing(**kw)
            walls.append(time.perf_counter() - t0)
            kernels.append([s['kernel_ms'] for s in cp.binning_stats])
        out['device_call_s'] = min(walls)
        out['steps'] = []
        for i, s in enumerate(cp.binning_stats):
            ms = min(k[i] for k in kernels)
            out['steps'].append({'step': ('day', 'lst', 'diff')[i] if len(cp.binning_stats) == 3 else ('day', 'diff')[i], 'kernel_ms': ms,
                                 'kernel_bytes': s['kernel_bytes'], 'gbs': s['kernel_bytes'] / ms * 1e-6,
                                 'hbm_fraction': s['kernel_bytes'] / ms * 1e-6 / a.hbm_gbs, 'chunks': s['chunks'],
                                 'upload_bytes': s['upload_bytes'], 'download_bytes': s['download_bytes']})
        err = cp.cpinfo['errinfo']
        out['ncomb'] = len(err['list_of_pair_of_pairs'])
        out['lstbins'] = int(err['lstbins'].size)
        out['elements'] = int(err['wts']['0'].size)
        # sqrt(w_j^2 + w_i^2) of integers: the squares of the device's roots, rounded, give the integers back exactly, and numpy's root
        # of those is what the reference holds
        w = err['wts']['0'].data
        out['weights_equal_numpy_sqrt'] = bool(NP.array_equal(w, NP.sqrt(NP.rint(w * w))))
        cp._drop_stack()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
