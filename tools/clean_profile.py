"""Measure the delay CLEAN (include/prisim_clean.h) and the numpy checker beside it.

  python tools/clean_profile.py cfg2 OUT.json [--nacc 64] [--dump ROWS.npz]
      BASELINE config 2 (HERA-19, 256 channels, nside-16 diffuse sky, Airy 14 m) through observe() x n_acc, noise on, then
      DelaySpectrum.delayClean(pad=1.0): 171 x n_acc x 2 rows of M = 512 lags.  Reports the call's device ms, the CLEAN kernel's
      ms, the iterations summed over rows and ns per row-iteration; --dump keeps a sample of rows for the cpu mode.
  python tools/clean_profile.py cfg5 OUT.json [--nbl 2000]
      A config-5 slice: the first nbl HERA-350 baselines x 1024 channels, 40 point sources, pad 1.0 (M = 2048), sky and noisy cubes,
      through prisim_clean_delay directly.
  python tools/clean_profile.py cpu OUT.json --rows ROWS.npz [--procs 16]
      The checker (tests/clean_checker.py, the reference's statements in numpy) on the dumped rows, one row per task over a pool of
      --procs processes: wall time, iterations, ns per row-iteration, extrapolated to all rows of the GPU run.
"""
import argparse
import json
import os
import sys
import time

import numpy as NP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def cfg2(args):
    from prisim_amd import delay_spectrum as DS, interferometry as RI, skymodel as SM, workloads as W
    cfg = W.config2()
    bl, ch, sky = cfg['baselines'], cfg['channels'], cfg['sky']
    skymod = SM.SkyModel(location=sky['altaz'], flux_ref=sky['flux_ref'], spindex=sky['spindex'], ref_freq=sky['ref_freq'],
                         src_shape=NP.stack((sky['fwhm_deg'], sky['fwhm_deg'], NP.zeros_like(sky['fwhm_deg'])), axis=1))
    ia = RI.InterferometerArray(['b%d' % i for i in range(bl.shape[0])], bl, ch, telescope={'id': 'hera'}, latitude=-30.7224,
                                skycoords='altaz', pointing_coords='altaz')
    ia.reserve(args.nacc)
    bpass = NP.ones(ch.size)
    for j in range(args.nacc):
        ia.observe((2457000.5 + j * 10.7 / 86400.0, 30.0 + 0.045 * j), {'Tnet': 200.0}, bpass, [90.0, 270.0], skymod, 10.7)
    ia.generate_noise(seed=11)
    ia.add_noise()
    ds = DS.DelaySpectrum(ia)
    ds.delayClean(pad=1.0, freq_wts=NP.blackman(ch.size) + 0.01, verbose=False)          # warm-up: code objects, rocFFT plans
    t0 = time.perf_counter()
    ds.delayClean(pad=1.0, freq_wts=NP.blackman(ch.size) + 0.01, verbose=False)
    wall = time.perf_counter() - t0
    st = ds._clean_stats
    it = ds._clean_iters
    out = {'mode': 'cfg2', 'n_acc': args.nacc, 'rows': st['rows'], 'M': int(ds.lags.size), 'call_wall_s': wall, 'device_ms': st['device_ms'],
           'clean_kernel_ms': st['clean_ms'], 'sum_iter': st['sum_iter'], 'ns_per_row_iter': st['clean_ms'] * 1e6 / st['sum_iter'],
           'iter_median': float(NP.median(it)), 'iter_min': int(it.min()), 'iter_max': int(it.max())}
    if args.dump:
        rng = NP.random.default_rng(1)
        nbl, m, nt = ds.skyvis_lag.shape
        pick = rng.choice(nbl * nt, size=args.sample, replace=False)
        b, t = pick // nt, pick % nt
        lag = NP.fft.ifftshift(ds.vis_lag, axes=1)[b, :, t]
        kern = NP.fft.ifftshift(ds.lag_kernel, axes=1)[b, :, t]
        hdl = ds.horizon_delay_limits
        import clean_checker as CK
        box = NP.array([CK.clean_box(ds.lags, hdl[ti if hdl.shape[0] > 1 else 0, bi], 1.0, ds.df * ch.size) for bi, ti in zip(b, t)])
        NP.savez(args.dump, lag=lag, kern=kern, box=box, iters=it[1, b, t], total_rows=st['rows'], gpu_device_ms=st['device_ms'],
                 gpu_clean_ms=st['clean_ms'], gpu_sum_iter=st['sum_iter'])
    return out


def cfg5(args):
    from prisim_amd import _abi, layouts as LAY, workloads as W
    bl = LAY.layout_baselines('HERA-350')[0][:args.nbl]
    ch = W.channel_grid(150e6, 97656.25, 1024)
    df, nchan = ch[1] - ch[0], ch.size
    rng = NP.random.default_rng(5)
    n = bl.shape[0]
    dirs = rng.normal(size=(40, 3))
    dirs[:, 2] = NP.abs(dirs[:, 2]) + 0.5
    dirs /= NP.linalg.norm(dirs, axis=1, keepdims=True)
    flux = rng.uniform(0.5, 10.0, 40)
    tau = bl.dot(dirs.T) / 299792458.0                                                    # (nbl, nsrc)
    vis = NP.einsum('bs,bsf->bf', NP.broadcast_to(flux, tau.shape), NP.exp(-2j * NP.pi * tau[:, :, None] * ch[None, None, :]))
    noisy = vis + 0.5 * (rng.standard_normal(vis.shape) + 1j * rng.standard_normal(vis.shape))
    win = NP.blackman(nchan) + 0.01
    m = 2 * nchan
    lags = NP.fft.fftfreq(m, df)
    blen = NP.linalg.norm(bl, axis=1) / 299792458.0
    bw = df * nchan
    box = NP.logical_and(lags <= blen[:, None] + 1.0 / bw, lags >= -blen[:, None] - 1.0 / bw)
    x = NP.stack((vis * win, noisy * win))
    with _abi.Context(0) as ctx:
        kw = dict(m=m, lag_scale=df, freq_scale1=lags[1] - lags[0], freq_scale2=2.0, gain=0.1, maxiter=10000, threshold=5e-3)
        ctx.clean_delay(x[:, :64], win[None].astype(complex), box[:64], **kw)                 # warm-up
        out = ctx.clean_delay(x, win[None].astype(complex), box, **kw)
    st = out['stats']
    return {'mode': 'cfg5_slice', 'rows': st['rows'], 'M': m, 'device_ms': st['device_ms'], 'clean_kernel_ms': st['clean_ms'],
            'sum_iter': st['sum_iter'], 'ns_per_row_iter': st['clean_ms'] * 1e6 / st['sum_iter'], 'waves_per_block': st['waves_per_block'],
            'kernel_in_lds': st['kernel_in_lds'], 'lds_bytes': st['lds_bytes'], 'iter_median': float(NP.median(out['iters']))}


def _one(arg):
    import clean_checker as CK
    lag, kern, box = arg
    t0 = time.perf_counter()
    o = CK.clean_row(lag, kern, box)
    return time.perf_counter() - t0, o['iter']


def cpu(args):
    from multiprocessing import Pool
    d = NP.load(args.rows)
    tasks = [(d['lag'][i], d['kern'][i], d['box'][i]) for i in range(d['lag'].shape[0])]
    with Pool(args.procs) as pool:
        pool.map(_one, tasks[:args.procs])                                                # warm the workers
        t0 = time.perf_counter()
        res = pool.map(_one, tasks, chunksize=1)
        wall = time.perf_counter() - t0
    secs = NP.array([r[0] for r in res])
    iters = NP.array([r[1] for r in res])
    cpu_total_s = wall / iters.sum() * float(d['gpu_sum_iter'])                         # the GPU run's iterations at this rate
    return {'mode': 'cpu_checker', 'procs': args.procs, 'rows': len(tasks), 'wall_s': wall, 'row_s_median': float(NP.median(secs)),
            'row_s_max': float(secs.max()), 'sum_iter': int(iters.sum()), 'iter_mismatches_vs_device': int(NP.sum(iters != d['iters'])),
            'ns_per_row_iter_aggregate': wall * 1e9 / iters.sum(),
            'extrapolated_s_for_gpu_rows': cpu_total_s, 'gpu_device_s': float(d['gpu_device_ms']) / 1e3,
            'speedup_vs_gpu_call': cpu_total_s / (float(d['gpu_device_ms']) / 1e3),
            'speedup_vs_gpu_kernel': cpu_total_s / (float(d['gpu_clean_ms']) / 1e3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', choices=('cfg2', 'cfg5', 'cpu'))
    ap.add_argument('out')
    ap.add_argument('--nacc', type=int, default=64)
    ap.add_argument('--nbl', type=int, default=2000)
    ap.add_argument('--dump', default=None)
    ap.add_argument('--sample', type=int, default=320)
    ap.add_argument('--rows', default=None)
    ap.add_argument('--procs', type=int, default=16)
    args = ap.parse_args()
    res = {'cfg2': cfg2, 'cfg5': cfg5, 'cpu': cpu}[args.mode](args)
    print(json.dumps(res))
    with open(args.out, 'w') as fh:
        json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
