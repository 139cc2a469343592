"""Measure the gain-table path (include/prisim_gains.h).

  python tools/gains_profile.py OUT.json
      apply: one config-3-sized snapshot (61 075 baselines x 1024 channels) resident in HBM, an antenna table of 350 rows, noise
             uploaded: best kernel ms of 5 and the algorithmic 48 B per element (sky, noise, output) against 8 TB/s;
      eval:  a HERA-350 table (350 antennas x 1024 channels x 120 times) evaluated at its own grid: kernel ms;
      add_noise: config 2 (HERA-19, 256 channels) at 64 snapshots with antenna and baseline tables, through the class (wall ms), against
             the numpy statement gains * skyvis + noise on the host with the gain cube given (wall ms, NumPy's own threads).
Run it under `rocprofv3 --kernel-trace --stats -- python tools/gains_profile.py OUT.json` for the kernel table.
"""
import json
import os
import sys
import tempfile
import time

import numpy as NP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def apply_cfg3():
    from prisim_amd import _abi
    nbl, nchan, nant = 61075, 1024, 350
    rng = NP.random.default_rng(1)
    out = {}
    with _abi.Context(0) as ctx:
        bl = NP.zeros((nbl, 3))
        bl[:, 0] = 14.6
        ctx.set_array(bl, NP.linspace(100e6, 200e6, nchan), nt_max=1)
        g = (1.0 + 0.1 * rng.standard_normal((nant, nchan, 1))) * (1 + 0.1j)
        tab, _ = ctx.gains_gather(g, NP.arange(nchan), NP.zeros(1, dtype=NP.int64))
        i1, i2 = rng.integers(0, nant, nbl), rng.integers(0, nant, nbl)
        noise = NP.zeros((1, nbl, nchan), dtype=complex)
        ms = []
        for _ in range(5):
            _, st = ctx.gains_apply(1, nbl, nchan, fa=(tab, _abi.PRISIM_GAINS_ANTENNA, i1, i2), noise=noise)
            ms.append(st['kernel_ms'])
        tab.close()
        best = min(ms)
        out = {'kernel_ms': ms, 'best_ms': best, 'algorithmic_bytes': 48 * nbl * nchan,
               'algorithmic_TBps': 48.0 * nbl * nchan / (best * 1e-3) / 1e12, 'frac_of_8TBps': 48.0 * nbl * nchan / (best * 1e-3) / 8e12}
    return out


def eval_hera():
    from prisim_amd import gains as G, hdf5io
    rng = NP.random.default_rng(5)
    nant, nchan, nt = 350, 1024, 120
    f = NP.linspace(100e6, 200e6, nchan)
    t = 2459000.0 + NP.arange(nt) / 720.0
    ga = (1.0 + 0.05 * NP.cos(NP.linspace(0, 20, nchan))[None, :, None] + 0.01 * rng.standard_normal((nant, 1, nt))) \
        * NP.exp(1j * rng.uniform(-1, 1, (nant, 1, 1)))
    path = os.path.join(tempfile.mkdtemp(), 'hera.hdf5')
    with hdf5io.File(path, 'w') as fo:
        fo.write('antenna-based/gains', ga)
        fo.write('antenna-based/ordering', NP.array(['label', 'frequency', 'time']))
        fo.write('antenna-based/label', NP.array([str(i) for i in range(nant)]))
        fo.write('antenna-based/frequency', f)
        fo.write('antenna-based/time', t)
    t0 = time.perf_counter()
    info = G.GainInfo(init_file=path)
    fit_s = time.perf_counter() - t0
    ctx = G._device()
    ms = []
    for _ in range(3):
        tab, st = ctx.gains_eval_spline(info.packed['antenna-based'], t, f)
        tab.close()
        ms.append(st['kernel_ms'])
    return {'kernel_ms': ms, 'best_ms': min(ms), 'scipy_fit_s': fit_s, 'table_bytes': nant * nchan * nt * 16}


def add_noise_cfg2(nacc=64):
    import test_gpu_gains as TG
    from prisim_amd import workloads as W
    rng = NP.random.default_rng(3)
    cfg = W.config2()
    ch, nbl = cfg['channels'], cfg['baselines'].shape[0]
    labels = [(str(i + 1), str(i // 2)) for i in range(nbl)]
    path = os.path.join(tempfile.mkdtemp(), 'g.hdf5')
    TG._gain_file(path, labels, ch, 2457000.5 + NP.arange(nacc) / 64.0, nbl + 1, rng)
    ia, _ = TG._config2_array(nacc, path)
    walls = []
    for _ in range(3):
        ia._device_in_step = True
        t0 = time.perf_counter()
        ia.add_noise()
        walls.append(1e3 * (time.perf_counter() - t0))
    gains = ia.gaininfo.spline_gains(ia.gain_labels(), freqs=ia.channels, times=NP.asarray(ia.timestamp))
    sky, noise = NP.asarray(ia.skyvis_freq), ia.vis_noise_freq
    np_ms = []
    for _ in range(3):
        t0 = time.perf_counter()
        ref = gains * sky + noise
        np_ms.append(1e3 * (time.perf_counter() - t0))
    err = float(NP.max(NP.abs(ia.vis_freq - ref) / (NP.abs(gains) * NP.abs(sky) + NP.abs(noise))))
    return {'nbl': nbl, 'nchan': int(ch.size), 'nacc': nacc, 'add_noise_wall_ms': walls, 'numpy_statement_ms': np_ms, 'max_rel_err': err}


def main():
    res = {'apply_cfg3': apply_cfg3(), 'eval_hera350': eval_hera(), 'add_noise_cfg2': add_noise_cfg2()}
    with open(sys.argv[1], 'w') as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == '__main__':
    main()
