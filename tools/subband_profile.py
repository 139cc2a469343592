"""Measure the sub-band delay transform (include/prisim_subband.h) and the numpy checker beside it.

  python tools/subband_profile.py cfg2 OUT.json [--nacc 64]
      BASELINE config 2 (HERA-19, 256 channels) through observe() x nacc, noise on, delayClean(pad=1.0), then
      subband_delay_transform with both keys, three bhw / bnw windows, pad 1 (M = 512): the whole call's wall time, its device and
      kernel ms, and the numpy checker (tests/subband_checker.py) on the same inputs.
  python tools/subband_profile.py cfg5 OUT.json [--nt 8] [--per-call 1]
      A config-5 slice: the HERA-350 layout (61 075 baselines) x 1024 channels, nt snapshots of seeded visibilities resident in HBM,
      three bhw windows, pad 1 (M = 2048), power only (oversampled and resampled), per-call snapshots at a time: kernel ms, rows,
      and the algorithmic traffic (each input row read once, each output written once) against 8 TB/s.
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
    import subband_checker as CK
    cfg = W.config2()
    bl, ch, sky = cfg['baselines'], cfg['channels'], cfg['sky']
    skymod = SM.SkyModel(location=sky['altaz'], flux_ref=sky['flux_ref'], spindex=sky['spindex'], ref_freq=sky['ref_freq'],
                         src_shape=NP.stack((sky['fwhm_deg'], sky['fwhm_deg'], NP.zeros_like(sky['fwhm_deg'])), axis=1))
    ia = RI.InterferometerArray(['b%d' % i for i in range(bl.shape[0])], bl, ch, telescope={'id': 'hera'}, latitude=-30.7224,
                                skycoords='altaz', pointing_coords='altaz')
    ia.reserve(args.nacc)
    for j in range(args.nacc):
        ia.observe((2457000.5 + j * 10.7 / 86400.0, 30.0 + 0.045 * j), {'Tnet': 200.0}, NP.ones(ch.size), [90.0, 270.0], skymod, 10.7)
    ia.generate_noise(seed=11)
    ia.add_noise()
    ds = DS.DelaySpectrum(ia)
    ds.delayClean(pad=1.0, verbose=False)
    f, df, nchan = ds.f, ds.df, ds.f.size
    fc = {k: f[[nchan // 4, nchan // 2, 3 * nchan // 4]] for k in ('cc', 'sim')}
    bw = {k: nchan * df / 8 for k in ('cc', 'sim')}
    shape, pad = {'cc': 'bhw', 'sim': 'bnw'}, {'cc': 1.0, 'sim': 1.0}
    ds.subband_delay_transform(bw, freq_center=fc, shape=shape, pad=pad, verbose=False)            # warm-up
    t0 = time.perf_counter()
    ds.subband_delay_transform(bw, freq_center=fc, shape=shape, pad=pad, verbose=False)
    wall = time.perf_counter() - t0
    st = ds._subband_stats
    cubes = {'sim': {'skyvis': NP.asarray(ia.skyvis_freq), 'vis': NP.asarray(ia.vis_freq), 'vis_noise': NP.asarray(ia.vis_noise_freq)},
             'cc': {n: getattr(ds, 'cc_%s_freq' % n) for n in ('skyvis', 'vis', 'skyvis_res', 'vis_res', 'skyvis_net', 'vis_net')}}
    t0 = time.perf_counter()
    CK.subband(f, df, cubes, NP.asarray(ia.bp), {k: NP.repeat(v, 3) for k, v in bw.items()}, fc, shape, pad)
    cpu = time.perf_counter() - t0
    out = {'config': 'cfg2', 'nacc': args.nacc, 'rows': st['rows'], 'windows': 3, 'm': 2 * nchan, 'call_s': wall,
           'device_ms': st['device_ms'], 'kernel_ms': st['kernel_ms'], 'routes': st['routes'], 'calls': st['calls'],
           'checker_s': cpu, 'checker_threads': os.environ.get('OMP_NUM_THREADS')}
    return out


def cfg5(args):
    from prisim_amd import _abi, dsp_readings as D, layouts as LAY, workloads as W
    import subband_checker as CK
    bl, _ = LAY.layout_baselines('HERA-350')                       # config 5's array
    nbl, nchan, df = bl.shape[0], 1024, 97656.25
    f = W.channel_grid(150e6, df, nchan)
    m = 2 * nchan
    fc = f[[nchan // 4, nchan // 2, 3 * nchan // 4]]
    bw = NP.repeat(nchan * df / 8, 3)
    fw = CK.freq_wts(f, df, bw, fc, 'bhw')
    nres = D.fft_downsample_length(m, NP.min(m * df / bw))
    rng = NP.random.default_rng(1)
    vis = rng.standard_normal((nbl, nchan)) + 1j * rng.standard_normal((nbl, nchan))
    out = {'config': 'cfg5 slice', 'nbl': nbl, 'nt': args.nt, 'nchan': nchan, 'm': m, 'nres': nres, 'windows': 3, 'calls': []}
    with _abi.Context(0) as ctx:
        ctx.set_array(NP.asarray(bl, dtype=NP.float64), f, nt_max=args.nt)
        for t in range(args.nt):
            ctx.set_vis(vis * (1.0 + 0.01 * t), slot=t)
        for t0 in range(0, args.nt, args.per_call):
            _, _, st = ctx.subband_power_resident(t0, args.per_call, NP.ones((1, nchan)), fw, m, df, NP.ones(3), nres=nres)
            out['calls'].append(st)
    rows = nbl * args.nt
    kms = sum(c['kernel_ms'] for c in out['calls'])
    alg = rows * (nchan * 16 + 3 * (m + nres) * 8)
    out.update({'rows': rows, 'kernel_ms': kms, 'alg_bytes': alg, 'alg_TBps': alg / (kms * 1e-3) / 1e12,
                'frac_of_8TBps': alg / (kms * 1e-3) / 8e12})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', choices=('cfg2', 'cfg5'))
    ap.add_argument('out')
    ap.add_argument('--nacc', type=int, default=64)
    ap.add_argument('--nt', type=int, default=8)
    ap.add_argument('--per-call', type=int, default=1)
    args = ap.parse_args()
    res = cfg2(args) if args.mode == 'cfg2' else cfg5(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
