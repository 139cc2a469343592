"""CPU: the sky-sum's planning header prisim_amd/csrc/skyvis_plan.h -- make_plan (tile, chunk, split), route (kernel family, row layout,
partial-cube sets, the ordered launches) and batch_plan (a chunk of snapshots in one launch).  The header is host-only: a stand-alone
program around it (tests/skyvis_plan_main.cpp) is built with -fsanitize=address,undefined and run on every case; nothing loaded into
Python is sanitised.  Checked: every field equals a restatement of the rules as they stood, spread over make_plan, fill_params,
taper_split_plan, run_pass, run_grad_pass, compute() and run_wave_batch, before they moved into the header (written here as they were
written there, branch by branch, with integer arithmetic as in C++); and on every case the agreements between plan and launches that the
launchers and the buffers rely on."""
import math
import os
import shutil
import subprocess

import numpy as NP
import pytest

from prisim_amd import sharding, workloads as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUS = 256                       # MI355X
C = 299792458.0
FP64, FP32 = 0, 1
AUTO, REC, DIRECT = 0, 1, 2
MAX_RUN_SETS = 8
(F_DIRECT, F_REC, F_PK, F_PK_SPLIT, F_T64_BLOCK, F_T64_WAVE, F_GRAD_F32, F_GRAD_F64, F_GRAD_F64_TGROUP, F_GRAD_F64_TEXACT,
 F_FOUR_PASS) = range(11)
FAMILY_NAMES = ['direct', 'recurrence', 'packed fp32', 'packed fp32 split', 'fp64 taper block items', 'fp64 taper wave items', 'grad fp32',
                'grad fp64', 'grad fp64 taper grouped', 'grad fp64 taper exact', 'four-pass gradient']
PAIRS, NATURAL, GRADROWS = 0, 1, 2
TOGGLES = ['taper_split', 'taper_f64_group', 'grad_taper_group', 'wave_items', 'fused_grad', 'wave_batch', 'wave_batch_grad',
           'wave_batch_single', 'batch_fp32_as_fp64']
HOOKS = ['PRISIM_HIP_FLUSH_SRC', 'PRISIM_HIP_TAPER_GROUP'] + ['PRISIM_HIP_' + n.upper() for n in TOGGLES]
NFIELDS = 72


@pytest.fixture(scope='module')
def plan_exe(tmp_path_factory):
    gxx = shutil.which('g++')
    assert gxx, 'g++ is needed to build the sky-sum plan driver'
    exe = tmp_path_factory.mktemp('skyvisplan') / 'skyvis_plan_main'
    subprocess.check_call([gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-Wall', '-Werror',
                           '-I', os.path.join(ROOT, 'prisim_amd', 'csrc'), os.path.join(ROOT, 'tests', 'skyvis_plan_main.cpp'),
                           '-o', str(exe)])
    return str(exe)


# ---- cases ---------------------------------------------------------------------------------------------------------------------------

def case(nbl, nchan, nsrc, nbl_sum=None, f0=150e6, df=80e3, uniform=True, taper=True, runs=(), lmax=300.0, precision=FP64, kernel=AUTO,
         want_grad=False, split_ready=True, kc=1, tune=(0, 0, 0), cu=CUS, ngroups=None, cull_any=(False, False), cull_staged=False,
         have_lift=True, flush_src=0, taper_group=-1, **toggles):
    nbl_sum = nbl if nbl_sum is None else nbl_sum
    c = dict(nbl=nbl, nbl_sum=nbl_sum, nchan=nchan, nsrc=nsrc, f0=float(f0), df=float(df), uniform=uniform, taper=taper,
             folded=nbl_sum != nbl, cu=cu, tune_ct=tune[0], tune_chunk=tune[1], tune_nsplit=tune[2],
             runs=[(int(lo), int(hi), float(k), int(row)) for lo, hi, k, row in runs],
             ngroups=(nbl_sum + 255) // 256 if ngroups is None else ngroups, lmax=float(lmax), cull_any=tuple(cull_any), cull_staged=cull_staged,
             have_lift=have_lift, flush_src=flush_src, taper_group=taper_group, precision=precision, kernel=kernel, want_grad=want_grad,
             split_ready=split_ready, kc=kc)
    for name in TOGGLES:
        c[name] = bool(toggles.pop(name, True))
    assert not toggles, toggles
    return c


def encode(c):
    row = [c['nbl'], c['nbl_sum'], c['nchan'], c['nsrc'], c['f0'], c['df'], c['uniform'], c['taper'], c['folded'], c['cu'], c['tune_ct'],
           c['tune_chunk'], c['tune_nsplit'], len(c['runs'])]
    for r in range(9):
        row += list(c['runs'][r]) if r < len(c['runs']) else [0, 0, 0.0, 0]
    row += [c['ngroups'], c['lmax'], c['cull_any'][0], c['cull_any'][1], c['cull_staged'], c['have_lift'], c['flush_src'], c['taper_group']]
    row += [c[name] for name in TOGGLES]
    row += [c['precision'], c['kernel'], c['want_grad'], c['split_ready'], c['kc']]
    assert len(row) == NFIELDS
    return [float(v) for v in row]


def run_driver(exe, cases, tmp_path):
    path = tmp_path / 'cases.f64'
    NP.asarray([encode(c) for c in cases], dtype=NP.float64).tofile(str(path))
    res = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and not res.stderr, (res.returncode, res.stderr[-2000:])
    lines = res.stdout.splitlines()
    assert len(lines) == len(cases)
    return [decode(line) for line in lines]


PLAN_KEYS = ['kernel', 'f32', 'ct', 'chunk', 'nsplit', 'src_per_split', 'nsrc_pad', 'ntiles', 'nbgroups', 'pk']
ROUTE_KEYS = ['layout', 'taper_group', 'cull', 'cull_prec', 'by_run', 'nsets', 'part_f32', 'alloc_sets', 'may_defer', 'last_taper_group',
              'zero_lift_counts', 'nlaunch']
LAUNCH_KEYS = ['family', 'src_lo', 'src_hi', 'src_per_split', 'accumulate', 'out_set', 'kappa0', 'cull_row', 'flags_row', 'taper', 'wave_nbw',
               'wave_nsplit', 'nbgroups', 'repack_pairs']
BATCH_KEYS = ['eligible', 'ct', 'ntiles', 'nbw', 'npad', 'nsplit']


def decode(line):
    v = [float(x) if ('.' in x or 'e' in x or 'n' in x) else int(x) for x in line.split()]
    out = {'base': dict(zip(PLAN_KEYS, v[:10])), 'family': v[10], 'sum_family': v[11], 'pl': dict(zip(PLAN_KEYS, v[12:22]))}
    out.update(zip(ROUTE_KEYS, v[22:34]))
    pos = 34
    out['launches'] = []
    for _ in range(out['nlaunch']):
        out['launches'].append(dict(zip(LAUNCH_KEYS, v[pos:pos + 14])))
        pos += 14
    out['split_eligible'] = v[pos]
    out['batch'] = dict(zip(BATCH_KEYS, v[pos + 1:pos + 7]))
    assert len(v) == pos + 7
    return out


# ---- the rules as the parent commit stated them ---------------------------------------------------------------------------------------

def round_up(v, m):
    return (v + m - 1) // m * m


def split_count(tiles, groups, slots, nsrc, nbl, nchan, f32, taper):
    """split_plan.h (tests/test_split_plan.py holds it to its own rule)"""
    base = max(tiles * groups, 1)
    slots = max(slots, 1)
    want = 1
    if base * 10 < slots * 60:
        want = (slots * 15 // 2 + base // 2) // base
    want = min(want, max(1, nsrc // 32))
    rate = (7.0e12 if taper else 1.0e13) if f32 else (2.8e12 if taper else 5.0e12)
    t_compute = float(nbl) * float(nchan) * float(nsrc) / rate
    t_split = 2.0 * float(nbl) * float(nchan) * (8.0 if f32 else 16.0) / 3.0e12
    cap = max((slots + base - 1) // base, int(0.03 * t_compute / t_split))
    if want > 16:
        want = max(16, min((3 * slots // 2 + base // 2) // base, cap))
    want = min(want, max(1, nsrc // 32))
    return max(1, min(want, 64))


def fmin_fmax(c):
    a, b = abs(c['f0']), abs(c['f0'] + c['df'] * float(c['nchan'] - 1))
    return min(a, b), max(a, b)


def parent_make_plan(c, precision, kernel):
    """make_plan (capi.cpp)"""
    pl = {}
    f32 = pl['f32'] = precision == FP32
    pl['kernel'] = kernel
    if kernel == AUTO:
        pl['kernel'] = REC if c['uniform'] else DIRECT
    nbl, nchan, nsrc = c['nbl_sum'], c['nchan'], c['nsrc']
    nbg = pl['nbgroups'] = (nbl + 255) // 256
    max_ct = 64 if f32 else 32
    fmin, _ = fmin_fmax(c)
    if f32 and c['taper'] and not (fmin > 0.0 and abs(c['df']) <= 3.4e-3 * fmin):
        max_ct = 32
    ct = c['tune_ct']
    if ct == 0:
        max_split = max(1, nsrc // 64)
        seed, per_term = (30.0, 2.5) if f32 else (48.0, 5.0)
        best, ct = 0.0, 8
        active = (nbg - 1) * 4 + min(4, (nbl - (nbg - 1) * 256 + 63) // 64)
        want_waves = 512 if f32 else 1024
        for cand in (64, 32, 16, 8):
            if cand > max_ct:
                continue
            tiles = (nchan + cand - 1) // cand
            if cand > 8 and tiles * nbg * max_split < 1024 and tiles * active * max_split < want_waves:
                continue
            cost = float(tiles) * (seed + per_term * cand)
            if best == 0.0 or cost < best * (1.0 - 1e-9):
                best, ct = cost, cand
    ct = min(ct, max_ct)
    pl['ct'] = ct
    pl['pk'] = f32 and ct in (32, 64) and pl['kernel'] == REC
    pl['ntiles'] = (nchan + ct - 1) // ct
    chunk = c['tune_chunk'] if c['tune_chunk'] else 64
    chunk = max(1, min(chunk, 16384 // (ct * (4 if f32 else 8)), 256))
    pl['chunk'] = chunk
    pl['nsrc_pad'] = round_up(max(nsrc, 1), chunk)
    nsplit = c['tune_nsplit']
    if nsplit == 0:
        per_cu = 2 if pl['pk'] else (4 if f32 else 2)
        nsplit = split_count(pl['ntiles'], nbg, max(c['cu'], 1) * per_cu, nsrc, nbl, nchan, f32, c['taper'])
    if (not f32 and c['taper'] and ct in (16, 32) and pl['kernel'] == REC and nbl <= 256 and not c['tune_chunk'] and c['taper_f64_group']):
        nbw = (nbl + 63) // 64
        if c['tune_nsplit']:
            s_want = c['tune_nsplit']
        else:
            s_want = max(1, 2 * 4 * max(c['cu'], 1) // (pl['ntiles'] * nbw))
            s_want = min(s_want, max(1, nsrc // 16))
        if s_want > 1:
            per = round_up((max(nsrc, 1) + s_want - 1) // max(s_want, 1), 4)
            pl.update(chunk=4, nsrc_pad=round_up(max(nsrc, 1), 16), src_per_split=per, nsplit=max(1, (nsrc + per - 1) // per))
            return pl
    if not c['tune_chunk'] and (not f32 or c['tune_nsplit']):
        def realised(ch):
            nch = round_up(max(nsrc, 1), ch) // ch
            per = (nch + nsplit - 1) // max(nsplit, 1)
            return (nch + per - 1) // max(per, 1)
        while chunk > 16 and realised(chunk) < nsplit:
            chunk //= 2
        pl['chunk'] = chunk
        pl['nsrc_pad'] = round_up(max(nsrc, 1), chunk)
    nchunks = pl['nsrc_pad'] // chunk
    nsplit = max(1, min(nsplit, nchunks))
    cps = (nchunks + nsplit - 1) // nsplit
    pl['src_per_split'] = cps * chunk
    pl['nsplit'] = (nchunks + cps - 1) // cps
    return pl


def launch(family, lo, hi, sps, acc=0, out_set=0, kappa0=0.0, cull_row=-1, flags_row=-1, taper=0, wave=(0, 0, 0), repack=0):
    return dict(zip(LAUNCH_KEYS, [family, lo, hi, sps, acc, out_set, kappa0, cull_row, flags_row, taper, wave[0], wave[1], wave[2], repack]))


def parent_route(c):
    """compute(), fill_params, taper_split_plan, run_pass and run_grad_pass (capi.cpp) for one sky-sum; c['split_ready']: whether the device
    half of taper_split_plan succeeds."""
    runs, nruns, taper, nsrc = c['runs'], len(c['runs']), c['taper'], c['nsrc']
    base = parent_make_plan(c, c['precision'], c['kernel'])
    pl = dict(base)
    f32 = pl['f32']
    fmin, fmax = fmin_fmax(c)
    # fill_params
    flush_src = c['flush_src'] if 0 < c['flush_src'] < (1 << 30) else 16384
    tgroup = 1 if (taper and fmin > 0.0 and abs(c['df']) <= 3.4e-3 * fmin) else 0
    if c['taper_group'] >= 0:
        tgroup = 1 if (c['taper_group'] != 0 and taper) else 0
    # compute()
    fused = c['want_grad'] and pl['kernel'] == REC and c['fused_grad']
    if fused:
        pl['ct'] = 16 if f32 else (16 if (taper and not c['grad_taper_group']) else 32)
        pl['pk'] = f32
        pl['ntiles'] = (c['nchan'] + pl['ct'] - 1) // pl['ct']
        pl['nsplit'] = 1
        pl['nsrc_pad'] = round_up(pl['nsrc_pad'], 4)
        pl['src_per_split'] = pl['nsrc_pad']
    ct, nsplit, chunk, pk = pl['ct'], pl['nsplit'], pl['chunk'], pl['pk']
    out = {'base': base, 'pl': pl, 'taper_group': tgroup, 'last_taper_group': 1 if (pk and tgroup) else 0}
    out['may_defer'] = int(not c['want_grad'] and pl['kernel'] == REC and nsplit > 1)
    rec = pl['kernel'] == REC
    out['alloc_sets'] = nruns if (rec and not fused and taper and 1 < nruns <= MAX_RUN_SETS) else 1
    out['zero_lift_counts'] = int(rec and taper and pk)
    out.update(cull=0, cull_prec=0, by_run=0, nsets=1, part_f32=0, layout=PAIRS)
    whole = dict(lo=0, hi=nsrc, taper=int(taper))
    # taper_split_plan: the eligibility half
    elig = bool(pk and taper and ct == 64 and tgroup and nruns > 0 and nruns <= MAX_RUN_SETS and c['taper_split'])
    if elig:
        kmax = max(r[2] for r in runs)
        umax = kmax * (c['lmax'] * fmax / C) * (c['lmax'] * fmax / C)
        elig = (kmax > 0.0 and umax <= 30.0 and 2.0 * umax * abs(c['df']) <= 0.125 * fmin and pl['nbgroups'] == c['ngroups'] and c['have_lift'])
    out['split_eligible'] = int(elig)
    if pl['kernel'] == DIRECT:
        out['sum_family'] = F_DIRECT
        out['launches'] = [launch(F_DIRECT, sps=pl['src_per_split'], **whole)]
    elif fused:
        # run_grad_pass
        if f32:
            fam = F_GRAD_F32
            out['layout'] = GRADROWS if not taper else PAIRS
            nbg = 0
        else:
            fam = F_GRAD_F64_TGROUP if (ct == 32 and taper) else (F_GRAD_F64 if ct == 32 else F_GRAD_F64_TEXACT)
            out['layout'] = NATURAL if (taper and ct == 32) else PAIRS
            nbg = (c['nbl_sum'] + 63) // 64
        out['sum_family'] = fam
        out['launches'] = [launch(fam, sps=pl['nsrc_pad'], wave=(0, 0, nbg), **whole)]
    else:
        # run_pass
        g64 = not f32 and taper and ct in (16, 32) and c['taper_f64_group']
        out['layout'] = NATURAL if g64 else PAIRS
        split = elig and c['split_ready']
        by_run = (split or g64) and 1 < nruns <= MAX_RUN_SETS
        nsets = nruns if (nsplit > 1 and by_run) else 1

        def run_per_split(r):
            return round_up(((r[1] - r[0]) + nsplit - 1) // nsplit, chunk)
        max_per = max(run_per_split(r) for r in runs) if nsets > 1 else pl['src_per_split']
        part_f32 = nsplit > 1 and f32 and max_per <= flush_src
        cpr = 1 if f32 else 0
        cull = bool((pk or g64) and taper and c['cull_any'][cpr] and c['cull_staged'] and nruns > 0 and pl['nbgroups'] == c['ngroups'])
        out.update(cull=int(cull), cull_prec=cpr, by_run=int(by_run), nsets=nsets, part_f32=int(part_f32))
        whole_cull = runs[0][3] if (cull and not split) else -1
        wave = (not f32 and taper and ct in (16, 32) and nsplit > 1 and c['nbl'] <= 256 and c['wave_items'])
        nbw = (c['nbl'] + 63) // 64
        wtriple = (nbw, nsplit, (nbw * nsplit + 3) // 4) if wave else (0, 0, 0)
        L = []
        if split:
            for r, (lo, hi, kappa, row) in enumerate(runs):
                sps = round_up(hi - lo, chunk) if nsplit == 1 else (run_per_split(runs[r]) if nsets > 1 else pl['src_per_split'])
                acc, oset = int(r > 0 and nsets == 1), (r if nsets > 1 else 0)
                if kappa > 0.0:
                    L.append(launch(F_PK_SPLIT, lo, hi, sps, acc, oset, kappa, row if cull else -1, r, 1))
                else:
                    L.append(launch(F_PK, lo, hi, sps, acc, oset, taper=0))
            out['sum_family'] = F_PK_SPLIT
        elif pk:
            L.append(launch(F_PK, sps=pl['src_per_split'], cull_row=whole_cull, **whole))
            out['sum_family'] = F_PK
        elif g64:
            fam = F_T64_WAVE if wave else F_T64_BLOCK
            if by_run:
                for r, (lo, hi, kappa, row) in enumerate(runs):
                    sps = round_up(hi - lo, chunk) if nsplit == 1 else run_per_split(runs[r])
                    acc, oset = int(r > 0 and nsets == 1), (r if nsets > 1 else 0)
                    if kappa > 0.0:
                        L.append(launch(fam, lo, hi, sps, acc, oset, cull_row=row if cull else -1, taper=1, wave=wtriple))
                    else:
                        L.append(launch(F_REC, lo, hi, sps, acc, oset, taper=0, repack=1))
            else:
                L.append(launch(fam, sps=pl['src_per_split'], cull_row=whole_cull, wave=wtriple, **whole))
            out['sum_family'] = fam
        else:
            L.append(launch(F_REC, sps=pl['src_per_split'], **whole))
            out['sum_family'] = F_REC
        out['launches'] = L
    out['nlaunch'] = len(out['launches'])
    out['family'] = F_FOUR_PASS if (c['want_grad'] and not fused) else out['sum_family']
    out['batch'] = parent_batch(c)
    return out


def parent_batch(c):
    """wave_batch_eligible's shape-and-hook part and run_wave_batch's plan (catalog.cpp); c['nsrc']: the catalogue's size"""
    kc, grad, nchan, nbl, n = c['kc'], c['want_grad'], c['nchan'], c['nbl'], c['nsrc']
    ok = c['wave_batch'] and c['wave_items'] and (c['precision'] == FP64 or c['batch_fp32_as_fp64'])
    ok = ok and not (kc < 1 or not c['uniform'] or nbl > 256 or nchan < 16)
    if grad:
        ok = ok and c['grad_taper_group'] and c['wave_batch_grad'] and c['fused_grad']
    if kc < 2:
        ok = ok and c['wave_batch_single']
    ok = ok and c['taper_f64_group'] and not c['tune_chunk']
    ct = c['tune_ct'] if c['tune_ct'] else (32 if (nchan >= 32 and kc > 1) else 16)
    if ct not in (16, 32):
        ct = 32
    if grad:
        ct = 32
    ntiles = (nchan + ct - 1) // ct
    nbw = (nbl + 15) // 16 if grad else (nbl + 63) // 64
    nsplit = c['tune_nsplit']
    if nsplit == 0:
        slots = 2 * 4 * max(c['cu'], 1)
        items0 = max(kc * nbw * ntiles, 1)                          # (kc >= 1 wherever the plan is used)
        lo = max(1, ((5 * slots // 2 if kc > 1 else slots) + items0 - 1) // items0)
        best, nsplit = 1e30, lo
        for m in range(lo, 2 * lo + 1):
            r = float(items0 * m) / float(slots)
            waste = math.ceil(r) / r + 0.002 * float(m - lo)
            if waste < best - 1e-12:
                best, nsplit = waste, m
        if kc == 1:
            nsplit = max(1, slots // items0)
        nsplit = min(nsplit, max(1, n // 32), 64)
    return dict(eligible=int(ok), ct=ct, ntiles=ntiles, nbw=nbw, npad=round_up(max(n, 1), 4), nsplit=nsplit)


def compare(c, got, want):
    for key in ('base', 'pl', 'batch'):
        assert {k: int(v) for k, v in got[key].items()} == {k: int(v) for k, v in want[key].items()}, (key, c, got[key], want[key])
    for key in ['family', 'sum_family', 'split_eligible'] + ROUTE_KEYS:
        assert got[key] == want[key], (key, FAMILY_NAMES[want['family']], c, got[key], want[key])
    for i, (g, w) in enumerate(zip(got['launches'], want['launches'])):
        assert g == w, (i, FAMILY_NAMES[want['family']], c, g, w)


def check_invariants(c, got):
    """what the launchers, the partial buffers and the reduction rely on, whatever the rules say"""
    pl, L, nsrc = got['pl'], got['launches'], c['nsrc']
    flush = c['flush_src'] if c['flush_src'] > 0 else 16384
    assert 1 <= len(L) <= MAX_RUN_SETS and got['alloc_sets'] >= got['nsets'] >= 1
    if len(L) > 1:
        assert L[0]['src_lo'] == 0 and L[-1]['src_hi'] == nsrc
        assert all(a['src_hi'] == b['src_lo'] for a, b in zip(L, L[1:])) and all(q['src_lo'] < q['src_hi'] for q in L)
    seen = set()
    for q in L:
        nsp = q['wave_nsplit'] if q['wave_nbw'] else pl['nsplit']
        if got['sum_family'] != F_DIRECT:
            assert q['src_per_split'] % pl['chunk'] == 0, (c, q)
            assert nsp * q['src_per_split'] >= q['src_hi'] - q['src_lo'], (c, q)
        assert 0 <= q['out_set'] < got['nsets']
        assert q['accumulate'] == int(q['out_set'] in seen), (c, q)
        seen.add(q['out_set'])
        if got['part_f32']:
            assert q['src_per_split'] <= flush, (c, q)
        nbg = q['nbgroups'] if q['nbgroups'] else pl['nbgroups']
        if q['family'] == F_T64_WAVE:
            assert c['nbl_sum'] <= 256 and 64 * q['wave_nbw'] >= c['nbl_sum'] and 4 * nbg >= q['wave_nbw'] * q['wave_nsplit'], (c, q)
            assert pl['ntiles'] * nbg <= 0x3fffffff
        else:
            assert q['wave_nbw'] == 0
            assert pl['ntiles'] * pl['nsplit'] * nbg <= 0x3fffffff
        assert q['family'] != F_FOUR_PASS
        if q['family'] == F_PK_SPLIT:
            assert pl['ct'] == 64 and q['flags_row'] >= 0 and q['kappa0'] > 0.0
        if q['family'] in (F_T64_BLOCK, F_T64_WAVE, F_PK_SPLIT):
            assert q['taper'] == 1 and pl['ct'] in ((64,) if q['family'] == F_PK_SPLIT else (16, 32))
    assert (got['layout'] == NATURAL) == (got['sum_family'] in (F_T64_BLOCK, F_T64_WAVE, F_GRAD_F64_TGROUP)), (c, got)
    if got['sum_family'] >= F_GRAD_F32:
        assert pl['nsplit'] == 1 and len(L) == 1 and pl['nsrc_pad'] % 4 == 0
    b = got['batch']
    if b['eligible']:
        per = 16 if c['want_grad'] else 64
        nbg = (c['kc'] * b['nbw'] * b['nsplit'] + 3) // 4                   # run_wave_batch's grid
        assert c['nbl'] <= 256 and per * b['nbw'] >= c['nbl'] and b['ct'] in (16, 32) and 1 <= b['nsplit']
        assert b['ntiles'] * nbg <= 0x3fffffff and b['npad'] % 4 == 0 and b['npad'] >= c['nsrc']


def check(exe, cases, tmp_path):
    got = run_driver(exe, cases, tmp_path)
    for c, g in zip(cases, got):
        compare(c, g, parent_route(c))
        check_invariants(c, g)
    return got


# ---- named shapes --------------------------------------------------------------------------------------------------------------------

def distinct_vectors(bl):
    return int(NP.unique(NP.asarray(bl, dtype=NP.float64) + 0.0, axis=0).shape[0])


def array_shape(bl, channels):
    """nbl, nbl_sum (set_array's fold rule), the channel grid and the longest baseline"""
    nu = distinct_vectors(bl)
    rows = nu if nu * 8 <= bl.shape[0] * 7 and nu > 256 else bl.shape[0]
    ch = NP.asarray(channels, dtype=NP.float64)
    return dict(nbl=int(bl.shape[0]), nbl_sum=int(rows), nchan=int(ch.size), f0=float(ch[0]), df=float((ch[-1] - ch[0]) / (ch.size - 1)),
                lmax=float(NP.sqrt((bl ** 2).sum(axis=1)).max()))


def kappa_of(fwhm_deg):
    return math.log(2.0) * (2.0 * math.sin(0.5 * fwhm_deg * math.pi / 180.0)) ** 2


def sky_runs(fwhm_deg):
    k = [kappa_of(float(v)) for v in NP.asarray(fwhm_deg)]
    runs, lo = [], 0
    for s in range(1, len(k) + 1):
        if s == len(k) or k[s] != k[lo]:
            runs.append((lo, s, k[lo], len(runs)))
            lo = s
    return runs


@pytest.fixture(scope='module')
def named_shapes():
    c2, c3 = W.config2(), W.config3()
    shapes = {'config 2': dict(array_shape(c2['baselines'], c2['channels']), nsrc=int(c2['sky']['dircos'].shape[0]),
                               runs=sky_runs(c2['sky']['fwhm_deg']))}
    bl3, n3 = c3['baselines'], int(c3['sky']['dircos'].shape[0])
    runs3 = [(0, n3, 0.0, 0)]                                              # point sources: one run of size 0
    shapes['headline'] = dict(array_shape(bl3, c3['channels']), nsrc=n3, runs=runs3)
    for world in (2, 4, 8):
        shapes['shard 0 of %d' % world] = dict(array_shape(sharding.shard_rows(bl3, world, 0)[0], c3['channels']), nsrc=n3, runs=runs3)
    kd = kappa_of(float(NP.degrees(W.GEOM.nside2resol(128))))              # config3(with_diffuse=True): nside 128 above the horizon
    nd = 12 * 128 * 128 // 2
    shapes['config 3 + diffuse'] = dict(shapes['shard 0 of 2'], nsrc=n3 + nd, runs=[(0, n3, 0.0, 0), (n3, n3 + nd, kd, 1)])
    small = dict(nbl=300, nbl_sum=300, nchan=72, f0=150e6, df=80e3, lmax=120.0)
    shapes['3 runs, points first'] = dict(small, nsrc=200, runs=[(0, 60, 0.0, 0), (60, 130, 2e-4, 1), (130, 200, 5e-4, 2)])
    for n in (MAX_RUN_SETS, MAX_RUN_SETS + 1):
        shapes['%d runs' % n] = dict(small, nsrc=40 * n, runs=[(40 * r, 40 * r + 40, 1e-4 * r, r) for r in range(n)])
    shapes['no runs'] = dict(small, nsrc=200, runs=[])
    shapes['non-uniform grid'] = dict(small, nsrc=200, runs=[(0, 200, 2e-4, 0)], uniform=False)
    for name, ratio in (('grid just above 3.4e-3', 3.4001e-3), ('grid just below 3.4e-3', 3.3999e-3)):
        shapes[name] = dict(small, nsrc=200, runs=[(0, 200, 2e-4, 0)], nchan=64, df=ratio * 150e6)
    for n in (0, 1, 15, 16, 17):
        shapes['nsrc %d' % n] = dict(small, nbl=171, nbl_sum=171, nsrc=n, runs=[(0, n, 2e-4, 0)] if n else [])
    for nb in (256, 257):
        shapes['nbl %d' % nb] = dict(small, nbl=nb, nbl_sum=nb, nsrc=1504, runs=[(0, 1504, 2e-4, 0)])
    shapes['folded, split'] = dict(small, nbl=600, nbl_sum=280, nsrc=4000, runs=[(0, 4000, 0.0, 0)])
    shapes['folded, no split'] = dict(small, nbl=100000, nbl_sum=61075, nchan=1024, nsrc=4000, runs=[(0, 4000, 0.0, 0)])
    return shapes


def variants(shape):
    """want_grad x precision x taper (without the taper: no runs), the split form's flags prepared or not"""
    out = []
    for grad in (False, True):
        for prec in (FP64, FP32):
            for taper in (True, False):
                for ready in (True, False):
                    s = dict(shape, taper=taper, runs=shape['runs'] if taper else [])
                    out.append(case(precision=prec, want_grad=grad, split_ready=ready, **s))
    return out


def test_named_shapes(plan_exe, named_shapes, tmp_path):
    cases, names = [], []
    for name, shape in named_shapes.items():
        v = variants(shape)
        cases += v
        names += [name] * len(v)
    # the batch plans of config 2's array: one snapshot and many
    c2 = named_shapes['config 2']
    assert c2['nbl'] == 171
    for kc in (1, 64, 256):
        for grad in (False, True):
            cases.append(case(kc=kc, want_grad=grad, **c2))
            names.append('batch of %d' % kc)
    # ... and on 16-channel tiles, where fp64 with the taper takes the grouped kernel whatever the array's size
    for name in ('3 runs, points first', '%d runs' % MAX_RUN_SETS, '%d runs' % (MAX_RUN_SETS + 1), 'no runs', 'nbl 256', 'nbl 257'):
        cases.append(case(tune=(16, 0, 0), **named_shapes[name]))
        names.append(name + ', 16-channel tiles')
    for name in ('grid just above 3.4e-3', 'grid just below 3.4e-3'):      # (a request for 64-channel tiles: the cap is what decides)
        cases.append(case(tune=(64, 0, 0), precision=FP32, **named_shapes[name]))
        names.append(name + ', 64-channel tiles')
    got = check(plan_exe, cases, tmp_path)
    by = {}
    for name, c, g in zip(names, cases, got):
        by.setdefault(name, []).append((c, g))

    def pick(name, **kw):
        (hit,) = [g for c, g in by[name] if all(c[k] == v for k, v in kw.items())]
        return hit
    plain = dict(want_grad=False, taper=True, split_ready=True)
    # config 2: 42 splits of 36 sources in wave items (fp64), 32-channel packed tiles (fp32); the batch of 64: 32-channel tiles, 4 splits
    g = pick('config 2', precision=FP64, **plain)
    assert (g['family'], g['pl']['ct'], g['pl']['nsplit'], g['pl']['src_per_split']) == (F_T64_WAVE, 16, 42, 36)
    g = pick('config 2', precision=FP32, **plain)
    assert (g['family'], g['pl']['ct']) == (F_PK, 32)
    assert [(g['batch']['ct'], g['batch']['nsplit']) for c, g in by['batch of 64'] if not c['want_grad']] == [(32, 4)]
    assert [(g['batch']['ct'], g['batch']['eligible']) for c, g in by['batch of 1'] if not c['want_grad']] == [(16, 1)]
    # the headline and its shards: packed fp32 on 64-channel tiles, split_plan.h's counts
    points = dict(want_grad=False, taper=False, split_ready=True)
    assert [pick(n, precision=FP32, **points)['pl']['nsplit'] for n in ('headline', 'shard 0 of 2', 'shard 0 of 4', 'shard 0 of 8')] == [6, 10, 16, 16]
    g = pick('headline', precision=FP32, **points)
    assert (g['family'], g['pl']['ct'], g['may_defer']) == (F_PK, 64, 1)
    # config 3 + diffuse on half the array: the split form, run by run, each run its own set of complex64 partial cubes
    g = pick('config 3 + diffuse', precision=FP32, **plain)
    assert (g['family'], g['nsets'], g['nlaunch'], g['by_run']) == (F_PK_SPLIT, 2, 2, 1)
    assert [q['family'] for q in g['launches']] == [F_PK, F_PK_SPLIT]
    assert pick('config 3 + diffuse', precision=FP32, want_grad=False, taper=True, split_ready=False)['family'] == F_PK
    # runs: three and eight go run by run, nine fall back to one launch over the whole sky
    assert pick('3 runs, points first, 16-channel tiles')['nlaunch'] == 3
    assert [q['family'] for q in pick('3 runs, points first, 16-channel tiles')['launches']] == [F_REC, F_T64_BLOCK, F_T64_BLOCK]
    assert pick('%d runs, 16-channel tiles' % MAX_RUN_SETS)['nlaunch'] == MAX_RUN_SETS
    assert pick('%d runs, 16-channel tiles' % (MAX_RUN_SETS + 1))['nlaunch'] == 1
    assert pick('no runs, 16-channel tiles')['nlaunch'] == 1
    assert pick('non-uniform grid', precision=FP64, **plain)['family'] == F_DIRECT
    assert pick('non-uniform grid', precision=FP64, want_grad=True, taper=True, split_ready=True)['family'] == F_FOUR_PASS
    # the channel-grid condition: the tile cap and the grouped recurrence move together
    above, below = pick('grid just above 3.4e-3, 64-channel tiles'), pick('grid just below 3.4e-3, 64-channel tiles')
    assert (above['pl']['ct'], above['taper_group']) == (32, 0) and (below['pl']['ct'], below['taper_group']) == (64, 1)
    # one baseline group goes in wave items, two do not
    assert pick('nbl 256, 16-channel tiles')['family'] == F_T64_WAVE
    assert pick('nbl 257, 16-channel tiles')['family'] == F_T64_BLOCK
    assert pick('folded, split', precision=FP32, **plain)['may_defer'] == 1 and pick('folded, no split', precision=FP32, **plain)['may_defer'] == 0
    # the gradients
    assert pick('config 2', precision=FP64, want_grad=True, taper=True, split_ready=True)['family'] == F_GRAD_F64_TGROUP
    assert pick('config 2', precision=FP64, want_grad=True, taper=False, split_ready=True)['family'] == F_GRAD_F64
    assert pick('config 2', precision=FP32, want_grad=True, taper=False, split_ready=True)['layout'] == GRADROWS


def test_every_toggle_off(plan_exe, named_shapes, tmp_path):
    """one hook at a time, on the named shape it decides"""
    c2, mixed = named_shapes['config 2'], named_shapes['config 3 + diffuse']
    fine = named_shapes['grid just below 3.4e-3']
    on = {'taper_split': case(precision=FP32, **mixed), 'taper_f64_group': case(**c2), 'grad_taper_group': case(want_grad=True, **c2),
          'wave_items': case(**c2), 'fused_grad': case(want_grad=True, **c2), 'wave_batch': case(kc=64, **c2),
          'wave_batch_grad': case(kc=64, want_grad=True, **c2), 'wave_batch_single': case(kc=1, **c2),
          'batch_fp32_as_fp64': case(kc=64, precision=FP32, **c2)}
    cases = list(on.values()) + [dict(c, **{name: False}) for name, c in on.items()]
    cases += [case(precision=FP32, taper_group=v, **fine) for v in (-1, 0, 1)]
    cases += [case(precision=FP32, taper_group=1, **named_shapes['grid just above 3.4e-3'])]
    cases += [case(precision=FP32, tune=(0, 0, 3), flush_src=v, **named_shapes['3 runs, points first']) for v in (0, 64)]
    got = check(plan_exe, cases, tmp_path)
    n = len(on)
    g_on, g_off = dict(zip(on, got[:n])), dict(zip(on, got[n:2 * n]))
    assert (g_on['taper_split']['family'], g_off['taper_split']['family']) == (F_PK_SPLIT, F_PK)
    assert (g_on['taper_f64_group']['family'], g_off['taper_f64_group']['family']) == (F_T64_WAVE, F_REC)
    assert (g_on['grad_taper_group']['family'], g_off['grad_taper_group']['family']) == (F_GRAD_F64_TGROUP, F_GRAD_F64_TEXACT)
    assert (g_on['wave_items']['family'], g_off['wave_items']['family']) == (F_T64_WAVE, F_T64_BLOCK)
    assert (g_on['fused_grad']['family'], g_off['fused_grad']['family']) == (F_GRAD_F64_TGROUP, F_FOUR_PASS)
    for name in ('wave_batch', 'wave_batch_grad', 'wave_batch_single', 'batch_fp32_as_fp64'):
        assert (g_on[name]['batch']['eligible'], g_off[name]['batch']['eligible']) == (1, 0), name
    # PRISIM_HIP_TAPER_GROUP forces the grouped form both ways
    assert [g['taper_group'] for g in got[2 * n:2 * n + 4]] == [1, 0, 1, 1]
    # PRISIM_HIP_FLUSH_SRC=64: pieces of more than 64 sources keep fp64 partial cubes
    assert [g['part_f32'] for g in got[2 * n + 4:]] == [1, 0]


def test_hooks_are_read_from_the_environment(plan_exe):
    def read(**env):
        e = {k: v for k, v in os.environ.items() if k not in HOOKS}
        e.update(env)
        res = subprocess.run([plan_exe, '--toggles'], capture_output=True, text=True, timeout=60, env=e)
        assert res.returncode == 0 and not res.stderr, res.stderr[-2000:]
        return [int(v) for v in res.stdout.split()]
    default = [0, -1] + [1] * len(TOGGLES)
    assert read() == default
    for i, hook in enumerate(HOOKS[2:]):
        off = list(default)
        off[2 + i] = 0
        assert read(**{hook: '0'}) == off, hook
        assert read(**{hook: '1'}) == default, hook              # these hooks can only switch off
    assert read(PRISIM_HIP_TAPER_GROUP='0')[1] == 0 and read(PRISIM_HIP_TAPER_GROUP='1')[1] == 1
    assert read(PRISIM_HIP_FLUSH_SRC='64')[0] == 64 and read(PRISIM_HIP_FLUSH_SRC='0')[0] == 0 and read(PRISIM_HIP_FLUSH_SRC='-3')[0] == 0


# ---- random cases --------------------------------------------------------------------------------------------------------------------

def random_case(rng):
    packed = rng.random() < 0.12      # a share of large packed fp32 taper skies on fine grids: where the split form can be reached at all
    small = rng.random() < 0.45 and not packed
    nbl = int(rng.integers(1, 400)) if small else int(rng.integers(257, 70000))
    nbl_sum = nbl
    if nbl > 600 and rng.random() < 0.3:
        nbl_sum = int(rng.integers(257, nbl * 7 // 8 + 1))
    nchan = int(rng.choice([1, 8, 15, 16, 17, 31, 32, 64, 72, 100, 256, 768, 1024])) if rng.random() < 0.8 else int(rng.integers(1, 2049))
    if packed:
        nchan = int(rng.choice([64, 72, 256, 1024]))
    nsrc = int(rng.integers(0, 40)) if rng.random() < 0.1 else int(rng.integers(1, 30000))
    f0 = float(rng.uniform(50e6, 250e6))
    df = float(rng.choice([-1.0, 1.0]) * rng.uniform(1e3, 4e-3 * f0)) if rng.random() < 0.8 else float(rng.uniform(4e-3, 4e-2) * f0)
    if packed:
        df = float(rng.uniform(1e3, 2e-3 * f0 / nchan * 64))
    if f0 + df * (nchan - 1) <= 1e6:
        df = abs(df)
    taper = bool(rng.random() < 0.7) or packed
    runs = []
    if taper and nsrc > 0 and (rng.random() < 0.8 or packed):
        nr = min(int(rng.choice([1, 1, 2, 2, 3, 5, 8, 9])), nsrc)
        cuts = [0] + sorted(rng.choice(NP.arange(1, nsrc), size=nr - 1, replace=False).tolist()) + [nsrc] if nr > 1 else [0, nsrc]
        kmax = float(10.0 ** rng.uniform(-6.0, -4.0 if packed else -2.0))
        runs = [(cuts[r], cuts[r + 1], 0.0 if rng.random() < 0.3 else kmax * float(rng.uniform(0.1, 1.0)), r) for r in range(nr)]
    tune = (int(rng.choice([0, 0, 0, 8, 16, 32, 64])), int(rng.choice([0, 0, 0, 0, 4, 16, 64, 256])), int(rng.choice([0, 0, 0, 1, 3, 7, 64, 4096])))
    if packed:
        tune = (int(rng.choice([0, 64])), 0, tune[2])
    tg = {name: bool(rng.random() >= 0.15) for name in TOGGLES}
    return case(nbl, nchan, nsrc, nbl_sum=nbl_sum, f0=f0, df=df, uniform=bool(rng.random() < 0.9) or packed, taper=taper, runs=runs,
                lmax=float(10.0 ** rng.uniform(0.5, 2.5 if packed else 3.5)), precision=FP32 if packed else int(rng.integers(2)),
                kernel=int(rng.choice([AUTO, AUTO, AUTO, REC, DIRECT])) if not packed else AUTO,
                want_grad=bool(rng.random() < 0.3) and not packed, split_ready=bool(rng.random() < 0.85), kc=int(rng.choice([1, 1, 2, 5, 64, 256])),
                tune=tune, cu=int(rng.choice([CUS, CUS, CUS, 104, 304, 0])), ngroups=None if rng.random() < 0.95 else 1 + (nbl_sum + 255) // 256,
                cull_any=(bool(rng.random() < 0.5), bool(rng.random() < 0.5)), cull_staged=bool(rng.random() < 0.8),
                have_lift=bool(rng.random() < 0.9), flush_src=int(rng.choice([0, 0, 64, 1000])), taper_group=int(rng.choice([-1, -1, -1, 0, 1])), **tg)


def test_random_cases(plan_exe, tmp_path):
    rng = NP.random.default_rng(2026)
    cases = []
    while len(cases) < 6000:
        c = random_case(rng)
        if c['kernel'] == REC and not c['uniform']:
            continue                                                # compute() refuses the recurrence on a non-uniform grid
        cases.append(c)
    got = check(plan_exe, cases, tmp_path)
    families = NP.zeros(len(FAMILY_NAMES), dtype=int)
    launched = NP.zeros(len(FAMILY_NAMES), dtype=int)
    for g in got:
        families[g['family']] += 1
        for q in g['launches']:
            launched[q['family']] += 1
    print('route families:', dict(zip(FAMILY_NAMES, families.tolist())))
    print('launch families:', dict(zip(FAMILY_NAMES, launched.tolist())))
    assert (families >= 50).all(), dict(zip(FAMILY_NAMES, families.tolist()))
    for name in TOGGLES:
        n_off = sum(not c[name] for c in cases)
        assert 50 <= n_off <= len(cases) - 50, name
    for v in (-1, 0, 1):
        assert sum(c['taper_group'] == v for c in cases) >= 50
    for v in (0, 64):
        assert sum(c['flush_src'] == v for c in cases) >= 50
    # both outcomes of what the toggles and the shape decide
    for key in ('cull', 'by_run', 'part_f32', 'may_defer', 'split_eligible'):
        n = sum(g[key] for g in got)
        assert 50 <= n <= len(got) - 50, (key, n)
    assert sum(g['nsets'] > 1 and g['pl']['nsplit'] > 1 for g in got) >= 50
    assert 50 <= sum(g['batch']['eligible'] for g in got) <= len(got) - 50
