"""Time prisim_antenna_power (Context.antenna_power) against the host loop it replaces, and three sizes of its pb_tile.

    python tools/antpower_time.py [--shapes config5,config2] [--ways entry,...] [--rounds 3] [--host-bytes 268435456] [--out FILE]

Shapes.  config5: the positions of an nside-256 HEALPix sky (786 432 pixels, the whole sphere as RA-Dec) with a power law, 1024
channels, 8 LSTs, the Airy pattern of 14 m (HERA).  config2: nside 16 (3072 pixels), 256 channels, 64 LSTs, the same beam.

Ways, in one process, alternated over --rounds rounds after one warm-up each:
  entry          the call with the planner's pb_tile (64 MiB)
  tile16/tile256 the same call with pb_tile of 16 and 256 MiB (PRISIM_ANTPOWER_TILE_BYTES, a development hook of the library); the
                 three must give the same bits
  entry_reduced  the call on every k-th pixel, k the smallest stride at which one LST's beam array (sources up x channels x 8 B) fits in
                 --host-bytes
  host_reduced   the host loop on that reduced sky: per LST primary_beams.primary_beam_generator on the sources above the horizon (a
                 context, the beam on the GPU, the array downloaded), the power law with numpy and two numpy sums
wall_ms and kernel_ms are the entry's own statistics (host clock around the call, stream events around the kernels); call_ms and
host_ms are the host clock around the whole Python call.  kernel_ms adds up the two streams' event spans, which overlap, so it can
exceed wall_ms.  gbps = kernel_bytes / kernel_ms, the bytes counted from the algorithm.
Prints one JSON line per round and a summary (minimum, median, maximum) per shape."""
import argparse
import json
import os
import sys
import time

import numpy as NP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from prisim_amd import _abi, frames as FRAMES, geometry as GEOM, primary_beams as PB  # noqa: E402

LAT = -30.7224
SHAPES = {'config5': (256, 1024, 8, 97656.25), 'config2': (16, 256, 64, 390625.0)}
TILE_ENV = 'PRISIM_ANTPOWER_TILE_BYTES'


def sky_of(nside, nchan, nlst, df, seed=55):
    theta, phi = GEOM.healpix_pix2ang_ring(nside)
    rng = NP.random.default_rng(seed)
    radec = NP.stack((NP.degrees(phi), 90.0 - NP.degrees(theta)), axis=1)
    return {'radec': radec, 'unitvec': GEOM.catalog_unitvec(radec, 'radec'), 'flux_ref': rng.lognormal(mean=NP.log(300.0), sigma=0.5, size=theta.size),
            'spindex': NP.full(theta.size, -0.55), 'ref_freq': 150e6, 'freqs': 150e6 + (NP.arange(nchan) - 0.5 * nchan) * df,
            'lst': 360.0 * NP.arange(nlst) / nlst + 1.0}


def entry(ctx, sky, sel=slice(None), tile_bytes=None):
    if tile_bytes is None:
        os.environ.pop(TILE_ENV, None)
    else:
        os.environ[TILE_ENV] = str(int(tile_bytes))
    rot = NP.stack([FRAMES.equatorial_to_enu(l, LAT) for l in sky['lst']])
    t0 = time.perf_counter()
    power, _, _, st = ctx.antenna_power(sky['unitvec'][sel], sky['freqs'], rot, _abi.PRISIM_BEAM_AIRY, 14.0, flux_ref=sky['flux_ref'][sel],
                                        spindex=sky['spindex'][sel], ref_freq_hz=sky['ref_freq'], want_sums=False)
    ms = (time.perf_counter() - t0) * 1e3
    os.environ.pop(TILE_ENV, None)
    keys = ('wall_ms', 'kernel_ms', 'kernel_bytes', 'spans', 'span_sources', 'streams', 'sources_up', 'sources_evaluated')
    row = dict({k: st[k] for k in keys}, call_ms=ms)
    row['gbps'] = st['kernel_bytes'] / st['kernel_ms'] / 1e6 if st['kernel_ms'] > 0 else None
    return power, row


def host_loop(sky, sel):
    """The reference's loop (prisim/interferometry.py:2391-2403) on this project's pieces."""
    t0 = time.perf_counter()
    radec, out = sky['radec'][sel], []
    for l in sky['lst']:
        altaz = GEOM.hadec2altaz(NP.stack((l - radec[:, 0], radec[:, 1]), axis=1), LAT, units='degrees')
        up = altaz[:, 0] >= 0.0
        pb = PB.primary_beam_generator(altaz[up], sky['freqs'], {'id': 'hera'}, freq_scale='Hz', skyunits='altaz')
        spectrum = sky['flux_ref'][sel][up, None] * (sky['freqs'][None, :] / sky['ref_freq']) ** sky['spindex'][sel][up, None]
        out.append(NP.sum(pb * spectrum, axis=0) / NP.sum(pb, axis=0))
    return NP.asarray(out), {'host_ms': (time.perf_counter() - t0) * 1e3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='config5,config2')
    ap.add_argument('--ways', default='entry,tile16,tile256,entry_reduced,host_reduced', help='a subset, e.g. for a kernel trace of the entry alone')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--host-bytes', type=int, default=1 << 28)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    lines = []

    def emit(obj):
        lines.append(json.dumps(obj))
        print(lines[-1], flush=True)

    with _abi.Context(0) as ctx:
        for name in a.shapes.split(','):
            nside, nchan, nlst, df = SHAPES[name]
            sky = sky_of(nside, nchan, nlst, df)
            nsrc = sky['radec'].shape[0]
            stride = 1
            while (nsrc // stride) * nchan * 8 // 2 > a.host_bytes:
                stride *= 2
            red = slice(None, None, stride)
            ways = {'entry': lambda: entry(ctx, sky), 'tile16': lambda: entry(ctx, sky, tile_bytes=16 << 20),
                    'tile256': lambda: entry(ctx, sky, tile_bytes=256 << 20), 'entry_reduced': lambda: entry(ctx, sky, red),
                    'host_reduced': lambda: host_loop(sky, red)}
            ways = {w: fn for w, fn in ways.items() if w in a.ways.split(',')}
            emit({'shape': name, 'nside': nside, 'nsrc': nsrc, 'nchan': nchan, 'nlst': nlst, 'reduced_stride': stride, 'reduced_nsrc': len(range(nsrc)[red])})
            first = {w: fn()[0] for w, fn in ways.items()}                           # one warm-up each
            same_bits = host_diff = None
            if all(w in first for w in ('entry', 'tile16', 'tile256')):
                same_bits = bool(NP.array_equal(first['entry'], first['tile16']) and NP.array_equal(first['entry'], first['tile256']))
            if 'entry_reduced' in first and 'host_reduced' in first:
                with NP.errstate(invalid='ignore', divide='ignore'):
                    host_diff = float(NP.nanmax(NP.abs(first['entry_reduced'] - first['host_reduced']) / NP.abs(first['host_reduced'])))
            emit({'shape': name, 'tiles_same_bits': same_bits, 'entry_vs_host_max_rel': host_diff})
            rows = []
            for k in range(a.rounds):
                row = {'shape': name, 'round': k}
                for w, fn in ways.items():
                    row[w] = fn()[1]
                rows.append(row)
                emit(row)

            def stat(way, key):
                v = sorted(r[way][key] for r in rows)
                return {'min': v[0], 'median': v[len(v) // 2], 'max': v[-1]}
            summary = {w: {k: stat(w, k) for k in ('kernel_ms', 'wall_ms', 'call_ms', 'gbps')} for w in ways if w != 'host_reduced'}
            if 'host_reduced' in ways:
                summary['host_reduced'] = {'host_ms': stat('host_reduced', 'host_ms')}
            emit({'shape': name, 'summary': summary})
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
