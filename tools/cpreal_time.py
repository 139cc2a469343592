"""Time InterferometerArray.closure_phase_realizations on both routes against the host loop it replaces, on one array.

    python tools/cpreal_time.py [--nt 16 --nreal 8 --nchan 256] [--every 1] [--rounds 3] [--out FILE]

HERA-19 (171 baselines) observing the config-2 sky for --nt snapshots of --nchan channels; every --every-th triad of
getThreePointCombinations.  Per round, alternating: the fused call on the staged route, on the direct route (the noisy stack only),
and the chain `generate_noise(seed + r); add_noise(); getClosurePhase(triplets)` for r < --nreal, whose phases must equal the fused
stack bit for bit.  One warm-up of each first.  wall_ms, kernel_ms and draws are the entry's own statistics; call_ms and chain_ms are
the host clock around the whole Python call.  Prints one JSON line per round and a summary line (minimum and median)."""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as NP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from prisim_amd import interferometry as RI, layouts as LAY, skymodel as SM, workloads as W  # noqa: E402


def hera19(nt, nchan):
    cfg = W.config2()
    pos = LAY.array_layout('HERA-19')
    bl, ids = LAY.fold_and_sort_baselines(*LAY.baseline_generator(pos))
    labels = [(str(int(a)), str(int(b))) for a, b in ids]
    ch = cfg['channels'][:nchan]
    sky = cfg['sky']
    shape = None if sky.get('fwhm_deg') is None else NP.stack((sky['fwhm_deg'], sky['fwhm_deg'], NP.zeros_like(sky['fwhm_deg'])), axis=1)
    skymod = SM.SkyModel(location=sky['altaz'], flux_ref=sky['flux_ref'], spindex=sky['spindex'], ref_freq=sky['ref_freq'], src_shape=shape)
    layout = {'positions': pos, 'labels': NP.array([str(i) for i in range(len(pos))]), 'ids': NP.arange(len(pos)), 'coords': 'ENU'}
    ia = RI.InterferometerArray(labels, bl, ch, telescope={'id': 'hera', 'shape': 'delta', 'size': 14.0, 'ocoords': 'altaz',
                                                           'orientation': NP.array([[90.0, 270.0]]), 'groundplane': None},
                                latitude=-30.7224, skycoords='altaz', pointing_coords='altaz', layout=layout)
    ia.reserve(nt)
    bpass = 0.6 + 0.4 * NP.hanning(ch.size + 2)[1:-1]
    for j in range(nt):
        ia.observe((2457000.5 + j / 64.0, 30.0 + 0.25 * j), {'Tnet': 200.0}, bpass, [90.0, 270.0], skymod, 10.7)
    return ia


def fused(ia, triplets, nreal, seed, route):
    t0 = time.perf_counter()
    res = ia.closure_phase_realizations(nreal, seed, antenna_triplets=triplets, route=route)
    return (time.perf_counter() - t0) * 1e3, res['closure_phase_vis'], ia.cpreal_stats['noisy']


def chain(ia, triplets, nreal, seed, check=None):
    t0 = time.perf_counter()
    same = True
    for r in range(nreal):
        ia.generate_noise(seed=seed + r)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            ia.add_noise()
        ph = ia.getClosurePhase(antenna_triplets=triplets)['closure_phase_vis']
        if check is not None:
            same = same and NP.array_equal(check[:, r], NP.transpose(ph, (2, 0, 1)))
    return (time.perf_counter() - t0) * 1e3, same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nt', type=int, default=16)
    ap.add_argument('--nreal', type=int, default=8)
    ap.add_argument('--nchan', type=int, default=256)
    ap.add_argument('--every', type=int, default=1)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    ia = hera19(a.nt, a.nchan)
    triplets = ia.getThreePointCombinations()[0][::a.every]
    used = NP.unique(ia.closure_leg_table(triplets)[0]).size
    head = {'array': 'HERA-19', 'nbl': int(ia.baselines.shape[0]), 'used_rows': int(used), 'ntriads': len(triplets), 'nchan': a.nchan, 'nt': a.nt,
            'n_realize': a.nreal, 'output_bytes': a.nt * a.nreal * len(triplets) * a.nchan * 8}
    lines = [json.dumps(head)]
    print(lines[-1], flush=True)
    _, ref, _ = fused(ia, triplets, a.nreal, 100, 'staged')                       # warm-ups
    _, other, _ = fused(ia, triplets, a.nreal, 100, 'direct')
    assert NP.array_equal(ref, other), 'the two routes differ'
    _, same = chain(ia, triplets, 1, 100, check=ref)
    assert same, 'the chain and the fused call differ'
    rows = []
    for k in range(a.rounds):
        row = {'round': k}
        for route in ('staged', 'direct'):
            ms, ph, st = fused(ia, triplets, a.nreal, 100, route)
            row[route] = {'call_ms': ms, 'wall_ms': st['wall_ms'], 'kernel_ms': st['kernel_ms'], 'draws': st['draws'], 'chunks': st['chunks'],
                          'chan_tile': st['chan_tile'], 'lds_bytes': st['lds_bytes'], 'kernel_bytes': st['kernel_bytes'],
                          'resident': st['resident'], 'equal_to_first': bool(NP.array_equal(ph, ref))}
        ms, same = chain(ia, triplets, a.nreal, 100, check=ref if k == 0 else None)
        row['chain'] = {'chain_ms': ms, 'equal_to_fused': bool(same)}
        rows.append(row)
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    def stat(get):
        v = sorted(get(r) for r in rows)
        return {'min': v[0], 'median': v[len(v) // 2], 'max': v[-1]}
    summary = {'summary': {'staged_kernel_ms': stat(lambda r: r['staged']['kernel_ms']), 'direct_kernel_ms': stat(lambda r: r['direct']['kernel_ms']),
                           'staged_call_ms': stat(lambda r: r['staged']['call_ms']), 'direct_call_ms': stat(lambda r: r['direct']['call_ms']),
                           'chain_ms': stat(lambda r: r['chain']['chain_ms']), 'staged_draws': rows[0]['staged']['draws'],
                           'direct_draws': rows[0]['direct']['draws']}}
    lines.append(json.dumps(summary))
    print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
