"""Bits and times of the four delay add-ons (subband, runs, cpdelay, cpft) from one build of the library, for an A/B of two builds of
the same ABI in alternating fresh processes.

    python tools/delay_lines_ab.py <libprisim_hip.so> [--workload subband|runs|cpdelay|cpft|all]

Without --workload: seeded small cases over the transform lengths (1, 2, padded, fused, rocFFT with odd and even floor(m/2), once 4096
with dynamic LDS above 64 KiB), the snapshot counts (1, 3, 65), two windows of which one has leading, trailing and interior zeros,
nres of 1, 4 and 7, and every form of call of each entry.  Prints one JSON line: per case the SHA-1 of every output array and the
entry's stats without its times, or the message of a refusal.
With --workload: one call of workload size per entry after a warm-up call (the shapes of tools/subband_profile.py cfg5 and
tools/cpft_time.py; cpdelay and runs have no tool of their own); prints the entry's kernel_ms (runs has none: its kernels are timed
from outside, by a kernel trace of this process)."""
import argparse
import hashlib
import json
import os
import sys

import numpy as NP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from prisim_amd import _abi  # noqa: E402

DF = 1e5
SIZES = [(1, 1, 3), (2, 2, 1), (8, 5, 65), (64, 64, 3), (9, 7, 3), (12, 9, 65)]          # (m, nchan, nt)
BIG = (4096, 2048, 1)
NRES = (1, 4, 7)


def sha(a):
    return hashlib.sha1(NP.ascontiguousarray(a).tobytes()).hexdigest()


def record(out, name, call, arrays):
    """out[name]: the hashes of arrays(result) and the stats, or the refusal."""
    try:
        res = call()
    except (ValueError, RuntimeError) as e:              # a refusal of the entry or of the binding: its words are the record
        out[name] = {'refused': '%s: %s' % (type(e).__name__, e)}
        return
    got, st = arrays(res)
    out[name] = {'sha1': {k: sha(v) for k, v in got.items() if v is not None},
                 'stats': {k: v for k, v in st.items() if not k.endswith('_ms')}}


def windows(rng, nchan):
    """Two windows: one without zeros; one with a leading, a trailing and an interior zero where it has the channels for them."""
    w = rng.uniform(0.5, 1.5, (2, nchan))
    if nchan >= 5:
        w[1, [0, nchan // 2, nchan - 1]] = 0.0
    return w


def cx(rng, shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def subband_cases(ctx, out):
    rng = NP.random.default_rng(101)
    nbl = 3
    pick = lambda r: ({k: v for k, v in r.items() if k != 'stats'}, r['stats'])
    want = ('over', 'over_power', 'res', 'res_power')
    for i, (m, nchan, nt) in enumerate(SIZES + [BIG]):
        wts, ps = windows(rng, nchan), rng.uniform(0.5, 2.0, 2)
        cubes = cx(rng, (2, nt, nbl, nchan))
        nbp = (1, nbl, nt * nbl)[i % 3]
        bp = rng.uniform(0.5, 1.5, (nbp, nchan))
        for nres in (NRES if m in (8, 64, 9) else (NRES[i % 3],)):
            record(out, 'subband m%d nt%d nbp%d nres%d' % (m, nt, nbp, nres),
                   lambda: ctx.subband_transform(cubes, bp, wts, m, DF, nres=nres, pscale=ps, want=want), pick)
    m, nchan, nt = 64, 64, 3
    wts, ps, bp = windows(rng, nchan), rng.uniform(0.5, 2.0, 2), rng.uniform(0.5, 1.5, (nbl, nchan))
    cubes = cx(rng, (1, nt, nbl, nchan))
    for w in want:
        record(out, 'subband only ' + w, lambda: ctx.subband_transform(cubes, bp, wts, m, DF, nres=7, pscale=ps, want=(w,)), pick)
    ctx.set_array(rng.standard_normal((nbl, 3)), 150e6 + DF * NP.arange(nchan), nt_max=nt)
    for t in range(nt):
        ctx.set_vis(cubes[0, t], slot=t)
    for route in ('auto', 'rocfft'):
        record(out, 'subband resident ' + route,
               lambda: ctx.subband_transform(None, bp, wts, m, DF, nres=4, pscale=ps, want=want, route=route, t0=0, nt=nt), pick)
        record(out, 'subband uploaded ' + route,
               lambda: ctx.subband_transform(cubes, bp, wts, m, DF, nres=4, pscale=ps, want=want, route=route), pick)
    record(out, 'subband fused m12', lambda: ctx.subband_transform(cx(rng, (1, 1, nbl, 9)), NP.ones((1, 9)), windows(rng, 9), 12, DF,
                                                                      want=('over',), route='fused'), pick)


def runs_cases(ctx, out):
    rng = NP.random.default_rng(102)
    R, nbl = 1, 5
    pick = lambda r: ({'out': r[0]}, r[1])
    for i, (m, nchan, nt) in enumerate(SIZES + [BIG]):
        win = windows(rng, nchan)
        vis = cx(rng, (R, nbl, nchan, nt))
        bp, wts = rng.uniform(0.5, 1.5, (nbl, nchan, 1)), rng.uniform(0.5, 1.5, (1, nchan, nt))
        kw = dict(bp=bp, wts=wts, win=win, m=m, scale=0.37)
        record(out, 'runs all m%d nt%d' % (m, nt), lambda: ctx.runs_transform(vis, nbl, nchan, nt, **kw), pick)
        if m == BIG[0]:
            continue
        record(out, 'runs interp m%d nt%d' % (m, nt),
               lambda: ctx.runs_transform(vis, nbl, nchan, nt, mode='interp', nout=max(m // 2, 1), factor=1.75, **kw), pick)
        for nres in (NRES if m in (8, 64, 9) else (NRES[i % 3],)):
            record(out, 'runs resample m%d nt%d nres%d' % (m, nt, nres),
                   lambda: ctx.runs_transform(vis, nbl, nchan, nt, mode='resample', nout=nres, **kw), pick)
    m, nchan, nt = 8, 5, 3
    win, vis = windows(rng, nchan), cx(rng, (R, nbl, nchan, nt))
    record(out, 'runs complex64', lambda: ctx.runs_transform(vis.astype(NP.complex64), nbl, nchan, nt, win=win, m=m), pick)
    record(out, 'runs no windows', lambda: ctx.runs_transform(vis, nbl, nchan, nt, m=m, mode='resample', nout=4), pick)
    for mode, nout, mm in (('all', 8, 8), ('all', 12, 12), ('resample', 4, 8)):
        per_pair = nchan * nt * 16 + 2 * nout * nt * 16 + (2 * nt * mm * 16 if mm == 12 else 0)
        record(out, 'runs three chunks %s m%d' % (mode, mm),
               lambda: ctx.runs_transform(vis, nbl, nchan, nt, win=win, m=mm, mode=mode, nout=nout, budget_bytes=2 * 2 * per_pair), pick)
    record(out, 'runs fused m12', lambda: ctx.runs_transform(vis, nbl, nchan, nt, win=win, m=12, route='fused'), pick)


def cpdelay_cases(ctx, out):
    rng = NP.random.default_rng(103)
    rows = 5
    pick = lambda r: ({k: v for k, v in r.items() if k != 'stats'}, r['stats'])
    want = ('over', 'over_power', 'res', 'res_power')
    for i, (m, nchan, nt) in enumerate(SIZES + [BIG]):
        wts, ps = windows(rng, nchan), rng.uniform(0.5, 2.0, 2)
        ph = rng.uniform(-NP.pi, NP.pi, (rows, nchan, nt))
        for nres in (NRES if m in (8, 64, 9) else (NRES[i % 3],)):
            record(out, 'cpdelay phases m%d nt%d nres%d' % (m, nt, nres),
                   lambda: ctx.closure_delay_spectra(wts, m, DF, phases=ph, nres=nres, pscale=ps, want=want), pick)
    nbl, nchan, nt, nres = 5, 8, 3, 4
    x = cx(rng, (nbl, nchan, nt))
    bpw = rng.uniform(0.5, 1.5, (nbl, nchan, nt))
    legs = rng.integers(0, nbl, (rows, 3)).astype(NP.int32)
    conj = rng.integers(0, 2, (rows, 3)).astype(NP.int32)
    wts, ps = windows(rng, nchan), rng.uniform(0.5, 2.0, 2)
    for m in (16, 12):
        per_triad = nchan * nt * (3 * 16 + 8) + 2 * nt * (m * (24 + (16 if m == 12 else 0)) + nres * 24)
        for name, budget in (('one chunk', _abi.CLOSURE_BUDGET), ('three chunks', 2 * 2 * per_triad)):
            record(out, 'cpdelay cube m%d %s' % (m, name),
                   lambda: ctx.closure_delay_spectra(wts, m, DF, cube=x, legs=legs, conj=conj, bpwts=bpw, nres=nres, pscale=ps, want=want,
                                                     want_phase=True, budget_bytes=budget), pick)
        ph = rng.uniform(-NP.pi, NP.pi, (rows, nchan, nt))
        record(out, 'cpdelay phases three chunks m%d' % m,
               lambda: ctx.closure_delay_spectra(wts, m, DF, phases=ph, nres=nres, pscale=ps, want=want,
                                                 budget_bytes=2 * 2 * (per_triad - nchan * nt * 48)), pick)
    record(out, 'cpdelay fused m12', lambda: ctx.closure_delay_spectra(wts, 12, DF, phases=ph, want=('over',), route='fused'), pick)


def cpft_cases(ctx, out):
    rng = NP.random.default_rng(104)
    lead = (5, 1, 1)

    def pick(r):
        got = {'lag_kernel': r['lag_kernel'], 'lag_kernel_res': r['lag_kernel_res']}
        for key in ('over', 'res'):
            for j, a in enumerate(r[key] or []):
                got['%s%d' % (key, j)] = a
        return got, r['stats']

    for i, (m, nchan, nt) in enumerate(SIZES + [BIG]):
        wts = windows(rng, nchan)
        full, bcast = cx(rng, lead + (nchan,)), cx(rng, (1, 1, 1, nchan))
        w = rng.integers(0, 4, lead + (nchan,)).astype(NP.float64)
        w[1] = 0.0
        vs = rng.uniform(0.5, 2.0, (2, lead[0]))
        for nres in (NRES if m in (8, 64, 9) else (NRES[i % 3],)):
            record(out, 'cpft weights m%d nres%d' % (m, nres),
                   lambda: ctx.cphase_ft([full, bcast], wts, m, DF, weights=w, vscale=vs, nres=nres), pick)
        record(out, 'cpft no weights m%d' % m, lambda: ctx.cphase_ft([full, bcast], wts, m, DF, nres=NRES[i % 3], shape=lead), pick)
        record(out, 'cpft lone lag kernel m%d' % m, lambda: ctx.cphase_ft([], wts, m, DF, nres=NRES[i % 3], want=('lag_kernel', 'res')), pick)
        if m in (8, 12):                                 # five rows in chunks of two
            row = 1 * nchan * 16 + nchan * 8 + 2 * (3 * m * 16 * (1 if m == 8 else 2) + 3 * 4 * 16)
            record(out, 'cpft three chunks m%d' % m,
                   lambda: ctx.cphase_ft([full, bcast], wts, m, DF, weights=w, vscale=vs, nres=4, budget_bytes=2 * 2 * row), pick)
    record(out, 'cpft fused m12', lambda: ctx.cphase_ft([cx(rng, lead + (9,))], windows(rng, 9), 12, DF, want=('over',), route='fused'), pick)


def workload(ctx, entry):
    """kernel_ms of the better of two calls behind a warm-up call, and the shape."""
    rng = NP.random.default_rng(1)
    if entry == 'subband':
        import subband_checker as CK
        from prisim_amd import dsp_readings as D, layouts as LAY, workloads as W
        bl, _ = LAY.layout_baselines('HERA-350')
        nbl, nchan, df = bl.shape[0], 1024, 97656.25
        f = W.channel_grid(150e6, df, nchan)
        m = 2 * nchan
        bw = NP.repeat(nchan * df / 8, 3)
        fw = CK.freq_wts(f, df, bw, f[[nchan // 4, nchan // 2, 3 * nchan // 4]], 'bhw')
        nres = D.fft_downsample_length(m, NP.min(m * df / bw))
        ctx.set_array(NP.asarray(bl, dtype=NP.float64), f, nt_max=1)
        ctx.set_vis(cx(rng, (nbl, nchan)), slot=0)
        call = lambda: ctx.subband_power_resident(0, 1, NP.ones((1, nchan)), fw, m, df, NP.ones(3), nres=nres)[2]
        shape = {'nbl': nbl, 'nchan': nchan, 'm': m, 'nres': int(nres), 'windows': 3, 'outputs': 'powers, resident input'}
    elif entry == 'cpft':
        lead, nchan = (20, 4, 30), 1024
        m, nres = 2 * nchan, 2 * nchan // 8
        inputs = [cx(rng, lead + (nchan,)) for _ in range(2)]
        w = rng.integers(0, 5, lead + (nchan,)).astype(NP.float64)
        w[0, 0, :, :] = 0.0
        wts, vs = rng.uniform(size=(2, nchan)), rng.uniform(0.5, 2.0, (2, lead[0]))
        call = lambda: ctx.cphase_ft(inputs, wts, m, DF, weights=w, vscale=vs, nres=nres)['stats']
        shape = {'shape': list(lead) + [nchan], 'm': m, 'nres': nres, 'nwin': 2, 'nin': 2}
    elif entry == 'cpdelay':
        rows, nchan, nt = 512, 1024, 8
        m, nres = 2 * nchan, 2 * nchan // 8
        ph = rng.uniform(-NP.pi, NP.pi, (rows, nchan, nt))
        wts = rng.uniform(size=(2, nchan))
        call = lambda: ctx.closure_delay_spectra(wts, m, DF, phases=ph, nres=nres, pscale=NP.ones(2),
                                                 want=('over_power', 'res', 'res_power'))['stats']
        shape = {'rows': rows, 'nchan': nchan, 'nt': nt, 'm': m, 'nres': nres, 'nwin': 2}
    else:
        R, nbl, nchan, nt = 2, 256, 1024, 4
        vis = cx(rng, (R, nbl, nchan, nt))
        win = rng.uniform(size=(2, nchan))

        def call():
            ctx.runs_transform(vis, nbl, nchan, nt, win=win, m=nchan)
            return ctx.runs_transform(vis, nbl, nchan, nt, win=win, m=2 * nchan, mode='resample', nout=nchan // 4)[1]
        shape = {'runs': R, 'nbl': nbl, 'nchan': nchan, 'nt': nt, 'calls': 'all lags at m = nchan; resample m = 2 nchan to nchan / 4', 'nwin': 2}
    call()
    stats = [call() for _ in range(2)]
    return {'shape': shape, 'kernel_ms': min(s['kernel_ms'] for s in stats) if 'kernel_ms' in stats[0] else None, 'route': stats[0]['route']}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('library')
    ap.add_argument('--workload', choices=('subband', 'runs', 'cpdelay', 'cpft', 'all'))
    a = ap.parse_args()
    _abi.LIB_PATH = os.path.abspath(a.library)
    out = {'library': a.library}
    with _abi.Context(0) as ctx:
        if a.workload:
            out['workload'] = {e: workload(ctx, e) for e in (('subband', 'runs', 'cpdelay', 'cpft') if a.workload == 'all' else (a.workload,))}
        else:
            out['cases'] = {}
            for cases in (subband_cases, runs_cases, cpdelay_cases, cpft_cases):
                cases(ctx, out['cases'])
    print(json.dumps(out))


if __name__ == '__main__':
    main()
