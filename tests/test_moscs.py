"""CPU: Cotton-Schwab CLEAN of the beam-weighted mosaic (include/prisim_moscs.h) -- the export, both structs and the constants against
the compiled header, the planning header under ASan and UBSan in a host program of its own (tests/moscs_plan_main.cpp), what the GPU
tests rely on in their inputs (tests/moscs_cases.py), the numpy checker against itself (tests/moscs_checker.py: the independent CLEAN
against the replay, the replay against doctored records and against two pixels that tie), the two sources through a drifting
chromatic beam, and the class prisim_amd.interferometry.ApertureSynthesis.clean_mosaic_cotton_schwab against a stand-in context that
answers clean_mosaic_cs with the checker.

Bounds.  The replay's tolerances are those the device is held to (tests/test_gpu_moscs.py), derived in the checker's docstring.  The
checker's own CLEAN and its replay evaluate the same numpy expressions, so they agree far inside them (1e-2 is asserted); what this
file shows of the replay is that it fails where a record is wrong by more than the tolerance.  The two sources: the bound of
tests/test_gpu_mosclean.py::test_c3_two_sources_come_back_in_true_flux, 1.5 thresholds in the units of F."""
import ctypes as C
import inspect
import os
import subprocess
import sys

import numpy as NP
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import csclean_checker as CS  # noqa: E402
import imaging_cases as IC  # noqa: E402
import mosaic_cases as MC  # noqa: E402
import mosaic_checker as MK  # noqa: E402
import mosclean_checker as QK  # noqa: E402
import moscs_cases as XC  # noqa: E402
import moscs_checker as XK  # noqa: E402
import test_mosaic as TM  # noqa: E402  (the array, the sky and the stand-in context of the mosaic tests)

from prisim_amd import _abi  # noqa: E402
from prisim_amd import interferometry as RI  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = XC.K


# ---- the library and its headers ----------------------------------------------------------------------------------------------------

def test_export_is_in_the_library_and_outside_the_core_abi():
    lib = _abi.load_library()
    assert _abi.MOSCS_EXPORTS == ('prisim_clean_mosaic_cs',) == _abi.HEADER_EXPORTS['prisim_moscs.h'] and 'prisim_clean_mosaic_cs' not in _abi.EXPORTS
    assert lib.prisim_clean_mosaic_cs(*[None] * 20) == _abi.PRISIM_EINVAL      # a null context and null args are refused, not read
    assert not hasattr(_abi, 'PrisimMoscsStats')                      # the struct lives on the class
    cs = [n for n, _ in _abi.Context.PrisimCscleanStats._fields_]
    assert [n for n, _ in _abi.Context.PrisimMoscsStats._fields_] == [('mosaic_ms' if n == 'dirty_ms' else n) for n in cs] + ['beam_ms']
    # the arguments: those of prisim_mosclean_args less its polling, in their order, then those of the cycles
    names = [n for n, _ in _abi.Context.PrisimMoscsArgs._fields_]
    mos = [n for n, _ in _abi.Context.PrisimMoscleanArgs._fields_]
    assert mos[-1] == 'poll_every' and names[:len(mos) - 1] == mos[:-1]
    assert names[len(mos) - 1:] == ['ny', 'nx', 'cycle_depth', 'cycle_niter', 'max_major', 'minor_route']
    assert (XK.THRESHOLD, XK.MAXITER, XK.DEAD, XK.MAJOR, XK.DIVERGED) == (_abi.PRISIM_IMCLEAN_THRESHOLD, _abi.PRISIM_IMCLEAN_MAXITER,
                                                                          _abi.PRISIM_IMCLEAN_DEAD, _abi.PRISIM_CSCLEAN_MAJOR,
                                                                          _abi.PRISIM_CSCLEAN_DIVERGED)
    # what the entry joins is called, not restated: one new kernel, the cycles and the mosaic's CLEAN kernels from their headers
    folder = os.path.join(ROOT, 'prisim_amd', 'csrc_imaging')
    src = {name: open(os.path.join(folder, name)).read() for name in os.listdir(folder)}
    new = src['moscs.hip']
    assert new.count('__global__') == 1 and 'k_moscs_scale(' in new and '#include "cycle_kernels.h"' in new and '#include "mosclean_kernels.h"' in new
    for name in ('struct CycleState', 'struct Lattice', 'Peak workgroup_peak(', 'k_csclean_init(', 'k_csclean_offsets(', 'k_csclean_mirror(',
                 'k_csclean_decide(', 'k_csclean_minor(', 'k_csclean_model(', 'Lattice lattice_of(', 'struct PlainFlux', 'struct FlatFlux',
                 'struct NoBeam', 'struct TableBeam'):
        assert [f for f, txt in src.items() if name in txt.replace('launch(ctx, ' + name, '')] == ['cycle_kernels.h'], name
    for name in ('k_mosclean_horizon(', 'k_mosclean_flat(', 'k_mosclean_flat_band('):
        assert [f for f, txt in src.items() if '__global__' in txt and name in txt] == ['mosclean_kernels.h'], name
    for step in ('enqueue_mos_wsum(', 'enqueue_mos_beam(', 'enqueue_mosclean_horizon(', 'enqueue_mos_sum(', 'enqueue_mosclean_flat(', 'enqueue_mos_finish(',
                 'enqueue_dirty_sums(', 'enqueue_minor(', 'k_csclean_model<TableBeam>', 'k_csclean_decide', '.check_outputs(', '.check_inputs(',
                 '.open(', '.search(', '.close(', '.gather(', '.write(', '.common_stats(', 'clean_refusal(', 'check_mosaic_beam('):
        assert step in new, step
    assert 'img_tile_pass' not in new and 'double acc' not in new and 'fill_beam(' not in new and 'atomicAdd' not in new
    assert 'while' not in new and 'volatile' not in new               # nothing waits for another workgroup
    body = new[new.index('  CleanCall '):new.index('extern "C"')]
    assert 'std::vector<double>' not in body and 'std::vector<int32_t>' not in body and 'CycleTables ' not in body      # host buffers outlive the stream
    # with PlainFlux and NoBeam prisim_clean_image_cs is what it was
    assert 'PlainFlux' in src['csclean.hip'] and 'k_csclean_model<NoBeam>' in src['csclean.hip'] and 'FlatFlux' not in src['csclean.hip']
    # an add-on: one name in the Makefile, nothing under csrc/
    mk = open(os.path.join(ROOT, 'prisim_amd', 'csrc', 'Makefile')).read()
    assert mk.count('moscs') == 1 and not [f for f in os.listdir(os.path.join(ROOT, 'prisim_amd', 'csrc')) if 'moscs' in f]


def test_structs_and_constants_against_the_compiled_header(tmp_path):
    """sizeof and every offsetof of prisim_moscs_args and prisim_moscs_stats as gcc lays them out, against the ctypes mirrors"""
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "prisim_moscs.h"', 'int main(void) {']
    mirrors = {'prisim_moscs_args': _abi.Context.PrisimMoscsArgs, 'prisim_moscs_stats': _abi.Context.PrisimMoscsStats}
    for cname, cls in mirrors.items():
        lines.append('  printf("%zu\\n", sizeof({0}));'.format(cname))
        lines += ['  printf("%zu\\n", offsetof({0}, {1}));'.format(cname, f) for f, _ in cls._fields_]
    lines += ['  printf("%d %d %d %d %d %d %d %d %d\\n", PRISIM_IMCLEAN_THRESHOLD, PRISIM_IMCLEAN_MAXITER, PRISIM_IMCLEAN_DEAD, PRISIM_CSCLEAN_MAJOR, '
              'PRISIM_CSCLEAN_DIVERGED, PRISIM_CSCLEAN_AUTO, PRISIM_CSCLEAN_LDS, PRISIM_CSCLEAN_GLOBAL, PRISIM_CSCLEAN_MAX_MAJOR);', '  return 0;', '}']
    (tmp_path / 'm.c').write_text('\n'.join(lines))
    subprocess.check_call(['gcc', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), str(tmp_path / 'm.c'), '-o', str(tmp_path / 'm')])
    out = subprocess.check_output([str(tmp_path / 'm')]).decode().split('\n')
    want = []
    for cls in mirrors.values():
        want += [str(C.sizeof(cls))] + [str(getattr(cls, f).offset) for f, _ in cls._fields_]
    assert out[:len(want)] == want
    assert out[len(want)].split() == [str(v) for v in (_abi.PRISIM_IMCLEAN_THRESHOLD, _abi.PRISIM_IMCLEAN_MAXITER, _abi.PRISIM_IMCLEAN_DEAD,
                                                       _abi.PRISIM_CSCLEAN_MAJOR, _abi.PRISIM_CSCLEAN_DIVERGED, _abi.PRISIM_CSCLEAN_AUTO,
                                                       _abi.PRISIM_CSCLEAN_LDS, _abi.PRISIM_CSCLEAN_GLOBAL, _abi.PRISIM_CSCLEAN_MAX_MAJOR)]


def test_plan_header_under_the_sanitizers(tmp_path):
    exe = tmp_path / 'moscs_plan_main'
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-I',
                           os.path.join(ROOT, 'prisim_amd', 'csrc_addon'), os.path.join(ROOT, 'tests', 'moscs_plan_main.cpp'), '-o', str(exe)])
    res = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = res.stdout.decode()
    assert res.returncode == 0, out
    last = out.strip().splitlines()[-1].split()
    assert last[0] == 'checked' and int(last[1]) > 20000 and last[2:] == ['bad', '0'], out
    txt = open(os.path.join(ROOT, 'prisim_amd', 'csrc_addon', 'moscs_plan.h')).read()
    assert '#include <hip' not in txt and '__device__' not in txt and '#include "addon_internal.h"' not in txt
    # the parents are asked, not restated
    assert 'mosclean_plan(' in txt and 'csclean_plan(' in txt and 'kImagingBlock' not in txt and 'kImcleanMaxSlabs' not in txt and 'psf_half =' not in txt


# ---- what the GPU tests rely on in their inputs, from the reference alone ---------------------------------------------------------------

@pytest.fixture(scope='module')
def large():
    c = XC.case(XC.SHAPES[2])
    return c, XC.problem(c, weights=c['w_bl'])


@pytest.fixture(scope='module')
def small():
    """37 baselines, 5 channels, 9 x 7 pixels, one snapshot through the 6 m Gaussian, weights per visibility with every seventh
    baseline at 0"""
    c = XC.case(XC.SHAPES[1])
    return c, XC.problem(c, weights=c['w_full'])


def test_the_cases_are_what_the_gpu_tests_rely_on(small, large):
    for (c, pb), shape in ((small, XC.SHAPES[1]), (large, XC.SHAPES[2])):
        masked = float(NP.mean(~pb.valid))
        print('%s: %.0f %% masked, the beam per snapshot up to %s' % (shape, 100 * masked, [round(float(pb.A[t].max()), 3) for t in range(pb.nt)]))
        assert 0.1 <= masked <= 0.9                                   # the mask keeps and cuts at least a tenth each
        for beam in ('gaussian', 'airy'):
            for chan_avg in (False, True):
                other = XC.problem(c, beam=beam, weights=c['w_full'], chan_avg=chan_avg, share=pb if beam == 'gaussian' else None)
                assert 0.1 <= float(NP.mean(~other.valid)) <= 0.9     # (the rim of the mask is asserted by the Problem itself)
        assert NP.count_nonzero(NP.asarray(c['w_bl']) == 0.0) == 37 // 7
    c, pb = large
    # the last snapshot has every direction below the horizon: its beam is exactly 0, the others see the lattice near their axis
    assert NP.all(pb.A[2] == 0.0) and pb.A[0].max() > 0.9 and pb.A[1].max() > 0.9
    one = XC.problem(XC.case(XC.SHAPES[0]), weights=None)
    assert NP.all(one.valid) and one.A.min() > 0.9
    # the independent CLEAN meets every status over the three settings
    P = XK.beam(pb, 25, 40)
    seen = {}
    for name, kw in XC.SETTINGS.items():
        r = XK.clean(pb, P, 25, 40, *XC.replay_args(kw))
        seen[name] = set(r['status'].tolist())
        print('setting %s: statuses %s, %d components, %d cycles' % (name, sorted(seen[name]), r['ncomp'].sum(), r['ncycles'].max()))
    assert seen['A'] == {XK.MAXITER} and {XK.MAJOR, XK.DIVERGED} <= seen['B'] and {XK.THRESHOLD, XK.MAXITER, XK.DIVERGED} <= seen['C']
    c, pb = small
    r = XK.clean(pb, XK.beam(pb, 9, 7), 9, 7, *XC.replay_args(XC.SETTINGS['B']))
    assert XK.MAJOR in set(r['status'].tolist())


# ---- the checker against itself -------------------------------------------------------------------------------------------------------

def test_the_channel_tolerance_is_the_problems_own(small):
    c, pb = small
    RN = pb.numerator(pb.v)
    rng = NP.random.default_rng(3)
    spent_q, spent = rng.uniform(0.0, 2.0, (pb.nt, pb.nchan)), rng.uniform(0.0, 3.0, pb.nchan)
    _, tol_F, tmax = pb.tolerances(RN, spent_q, spent)
    for k in range(pb.nc):
        tF, tm = XK.channel_tolerance(pb, RN, k)(spent_q, spent)
        ok = pb.valid[:, k]
        assert NP.allclose(tF[ok], tol_F[ok, k], rtol=1e-12, atol=0) and abs(tm - tmax[k]) <= 1e-12 * tmax[k]


@pytest.mark.parametrize('chan_avg', [False, True])
def test_independent_clean_against_the_replay(small, chan_avg):
    c, pb0 = small
    window = NP.arange(63) % 3 != 1
    pb = XC.problem(c, weights=c['w_full'], chan_avg=chan_avg, window=window, share=pb0)
    P = XK.beam(pb, 9, 7)
    assert P.shape == (pb.nc, 17, 13) and NP.array_equal(P, P[:, ::-1, ::-1]) and NP.allclose(P[:, 8, 6], 1.0, rtol=0, atol=1e-14)
    s = XK.scale_of(pb)
    seen = set()
    settings = [XC.replay_args(kw) for kw in XC.SETTINGS.values()] + [(0.3, 25, 0.0, False, 0.5, 4, 10), (1.0, 3, 0.2, True, 0.5, 2, 3),
                                                                       (0.5, 0, 0.1, False, 0.3, 0, 4), (0.5, 5, 0.1, False, 0.3, 0, 0)]
    for args in settings:
        gain, maxiter, thr, rel, depth, niter, major = args
        r = XK.clean(pb, P, 9, 7, *args)
        worst = XK.replay(pb, P, 9, 7, r, *args)
        seen |= set(r['status'].tolist())
        print('%s: %d components in %d cycles, statuses %s, worst deviation %.2e of its tolerance'
              % (args, r['ncomp'].sum(), r['ncycles'].max(), sorted(set(r['status'].tolist())), worst))
        used = r['comp_pixel'][r['comp_pixel'] >= 0]
        assert worst <= 1e-2 and NP.all(window[used])
        assert NP.all(r['ncomp'] <= maxiter) and NP.all(r['ncycles'] <= major) and NP.all((r['status'] == XK.MAXITER) <= (r['ncomp'] == maxiter))
        for k in range(pb.nc):
            n = r['ncycles'][k]
            assert NP.all(pb.valid[r['comp_pixel'][k, :r['ncomp'][k]], k])
            held = NP.concatenate(([0], r['cycle_ncomp'][k, :n]))
            assert NP.all(NP.diff(held) >= 1) and held[-1] == r['ncomp'][k]      # a cycle that starts adds a component
            assert niter == 0 or NP.all(NP.diff(held) <= niter)
            assert NP.all(NP.isfinite(r['cycle_peak'][k, :n + 1])) and NP.all(NP.isnan(r['cycle_peak'][k, n + 1:]))
            if r['status'][k] == XK.DIVERGED:
                assert r['cycle_peak'][k, n] > r['cycle_peak'][k, n - 1]
        # the residual visibilities are V less the components through the beam, and num is their mosaic numerator
        vm = NP.zeros_like(pb.v)
        for k in range(pb.nc):
            for q, a in zip(r['comp_pixel'][k, :r['ncomp'][k]], r['comp_flux'][k, :r['ncomp'][k]]):
                vm += pb.component_vis(k, int(q), a)
        assert NP.allclose(r['vres'], pb.v - vm, rtol=0, atol=1e-13 * NP.abs(pb.v).max())
        assert NP.allclose(r['num'], pb.numerator(r['vres']), rtol=0, atol=1e-12 * NP.abs(r['num']).max())
        if maxiter == 0 or major == 0:                                # a mosaic
            assert NP.array_equal(r['num'], pb.numerator(pb.v)) and r['comp_pixel'].shape == (pb.nc, 0) and NP.array_equal(r['vres'], pb.v)
            assert NP.all(r['status'] == (XK.MAXITER if maxiter == 0 else XK.MAJOR)) and NP.all(r['ncycles'] == 0)
            assert NP.array_equal(r['residual'], MK.quotient(r['num'], r['den'], r['wsum'], c['pbmin'], chan_avg)[0], equal_nan=True)
    assert {XK.THRESHOLD, XK.MAXITER, XK.MAJOR} <= seen
    # the first component of a run is gain times the mosaic's value at the pick: F s = (N / sqrt(Q W)) sqrt(W / Q) = N / Q
    r = XK.clean(pb, P, 9, 7, 0.3, 1, 0.0, False, 0.5, 0, 4)
    RN = pb.numerator(pb.v)
    for k in range(pb.nc):
        q = r['comp_pixel'][k, 0]
        assert abs(r['comp_flux'][k, 0] - 0.3 * pb.band(RN)[q, k] / pb.Qc[q, k]) <= 1e-14 * abs(r['comp_flux'][k, 0]) and s[q, k] > 1.0


def test_replay_refuses_doctored_records(small):
    c, pb = small
    P = XK.beam(pb, 9, 7)
    args = (0.3, 60, 0.4, True, 0.8, 3, 16)
    r = XK.clean(pb, P, 9, 7, *args)
    assert NP.all(r['status'] == XK.THRESHOLD) and len(set(r['ncycles'].tolist())) > 2     # the channels end at different places
    XK.replay(pb, P, 9, 7, r, *args)

    def tampered(**kw):
        out = {k: NP.array(v) for k, v in r.items()}
        for name, (index, value) in kw.items():
            out[name][index] = value
        return out

    k = int(NP.argsort(r['ncycles'], kind='stable')[-2])             # not the longest: the shapes of the tables stand when it is cut short
    n, last = int(r['ncycles'][k]), int(r['ncomp'][k])
    assert 3 <= n < r['ncycles'].max() and last < r['ncomp'].max()
    s = XK.scale_of(pb)
    F0 = pb.flat(pb.numerator(pb.v))[:, k]
    second = NP.argsort(NP.where(pb.search[:, k], NP.abs(F0), -1.0))[-2]      # the second largest of the first search image
    masked = int(NP.flatnonzero(~pb.valid[:, k])[0])
    q1 = int(r['comp_pixel'][k, 1])
    # the model without the beam factor: every component's visibilities as a dirty-image CLEAN would take them out
    bare = NP.array(pb.v)
    for kk in range(pb.nc):
        for q, a in zip(r['comp_pixel'][kk, :r['ncomp'][kk]], r['comp_flux'][kk, :r['ncomp'][kk]]):
            bare[:, :, kk] -= (pb.component_vis(kk, int(q), a)[:, :, kk] / pb.A[:, int(q), kk][:, NP.newaxis])
    assert NP.max(NP.abs(bare - r['vres'])) > 1e-3
    cases = [('not the peak', tampered(comp_pixel=((k, 0), second))),                                  # a wrong pick
             ('a flux that is not', tampered(comp_flux=((k, 1), r['comp_flux'][k, 1] * (1 + 1e-9)))),   # a flux off by 1e-9 of itself
             ('a flux that is not', tampered(comp_flux=((k, 1), r['comp_flux'][k, 1] / s[q1, k]))),     # a flux left in flat units
             ('masked', tampered(comp_pixel=((k, 0), masked))),                                         # a pick on a masked pixel
             (None, tampered(status=(k, XK.MAXITER))), (None, tampered(status=(k, XK.MAJOR))), (None, tampered(status=(k, XK.DIVERGED))),
             (None, tampered(status=(k, XK.DEAD))),                                                      # wrong statuses
             ('components beyond the last cycle', tampered(ncycles=(k, n - 1))),                       # a wrong cycle count
             (None, tampered(ncycles=(k, n + 1))),                                                       # ... and a cycle without a record
             ('residual visibilities', tampered(vres=((0, 3, k), r['vres'][0, 3, k] + 1e-8))),           # a vres off by 1e-8
             ('residual visibilities', dict(tampered(), vres=bare)),                                     # a model without the beam factor
             ('P0', tampered(peak0=(k, r['peak0'][k] * (1 + 1e-9)))), ('Pc', tampered(cycle_peak=((k, 1), r['cycle_peak'][k, 1] * (1 + 1e-9)))),
             ('numerator', tampered(num=((5, k), r['num'][5, k] + 1e-9 * pb.absV[:, k].sum()))),
             ('residual', tampered(residual=((int(NP.flatnonzero(pb.valid[:, k])[0]), k), 0.0)))]      # a quotient that is not the header's
    # a minor cycle ended early: its last component moved to the cycle after it, while the working peak was still above the limit
    cyc = next(j for j in range(n - 1) if r['cycle_ncomp'][k, j] - (r['cycle_ncomp'][k, j - 1] if j else 0) in (2, 3))
    cases.append(('a cycle ended early', tampered(cycle_ncomp=((k, cyc), r['cycle_ncomp'][k, cyc] - 1))))
    # a channel stopped one cycle early at the threshold: its peak is still above it
    early = tampered(ncycles=(k, n - 1), status=(k, XK.THRESHOLD), ncomp=(k, r['cycle_ncomp'][k, n - 2]))
    early['comp_pixel'][k, r['cycle_ncomp'][k, n - 2]:], early['comp_flux'][k, r['cycle_ncomp'][k, n - 2]:] = -1, 0.0
    assert last > r['cycle_ncomp'][k, n - 2]
    cases.append(('a stop at the threshold above it', early))
    for i, (msg, bad) in enumerate(cases):
        with pytest.raises(AssertionError, match=msg):
            XK.replay(pb, P, 9, 7, bad, *args)
            print('doctored record %d passed' % i)
    # a pick outside the window
    win = NP.ones(63, dtype=bool)
    later = [q for q in r['comp_pixel'][k, :last] if q not in r['comp_pixel'][:, 0]]
    win[later[0]] = False                                             # not the first peak of any channel: every P0 stands
    pbw = XC.problem(c, weights=c['w_full'], window=win, share=pb)
    with pytest.raises(AssertionError, match='window|peak'):
        XK.replay(pbw, P, 9, 7, r, *args)


def test_replay_passes_either_of_two_pixels_that_tie_to_rounding(small):
    c, pb = small
    P = XK.beam(pb, 9, 7)
    one_args = (0.3, 1, 0.0, False, 0.5, 0, 4)
    one = XK.clean(pb, P, 9, 7, *one_args)
    k = 2
    q0 = int(one['comp_pixel'][k, 0])
    twin = (q0 + 7) % 63                                              # the next row: a copy of the peak's direction, a few units in the last place away
    assert twin not in (31, 59, 3, 28, 34) and q0 not in (31, 59, 3, 28, 34)      # not one of the pixels the lattice steps are taken from
    u2 = c['unitvec'].copy()
    u2[twin] = IC.unit(u2[q0] + 4e-16 * NP.array([1.0, -1.0, 1.0]))
    assert not NP.array_equal(u2[twin], u2[q0])
    ct = dict(c, unitvec=u2)
    pbt = XC.problem(ct, weights=c['w_full'])
    RN0 = pbt.numerator(pbt.v)
    F0 = pbt.flat(RN0)
    _, tol_F, tmax = pbt.tolerances(RN0, NP.zeros((pbt.nt, pbt.nchan)), NP.zeros(pbt.nchan))
    assert pbt.search[twin, k] and abs(abs(F0[twin, k]) - abs(F0[q0, k])) <= tmax[k]
    one = XK.clean(pbt, P, 9, 7, *one_args)
    assert one['comp_pixel'][k, 0] in (q0, twin) and one['status'][k] == XK.MAXITER and one['ncycles'][k] == 1
    other = twin if one['comp_pixel'][k, 0] == q0 else q0
    alt = {name: NP.array(v) for name, v in one.items()}
    a = 0.3 * F0[other, k] * XK.scale_of(pbt)[other, k]
    alt['comp_pixel'][k, 0], alt['comp_flux'][k, 0] = other, a
    vres = pbt.v - pbt.component_vis(k, other, a)
    alt['vres'][:, :, k] = vres[:, :, k]
    alt['num'][:, k] = pbt.numerator(vres)[:, k]
    alt['residual'], alt['pb_eff'] = MK.quotient(alt['num'], alt['den'], alt['wsum'], c['pbmin'])
    alt['residual_flat'] = QK.flat_of(alt['num'], alt['den'], alt['wsum'], c['pbmin'])
    alt['cycle_peak'][k, 1] = NP.nanmax(NP.abs(alt['residual_flat'][:, k]))
    XK.replay(pbt, P, 9, 7, one, *one_args)
    XK.replay(pbt, P, 9, 7, alt, *one_args)


def test_the_minor_beam_approximates_the_normalised_response_of_the_mosaic():
    """In F a unit component at q answers with |N_c[p]| / sqrt(Q[p] Q[q]): 1 at p = q, never above 1, and |P| to well within the
    largest sidelobe of P -- what makes the minor cycle of the dirty image serve the flat-noise image."""
    c, band = XC.two_sources()
    per = XC.problem(c, pbmin=0.1, share=band)
    P = XK.beam(per, 17, 17)
    side = 0.0
    worst = 0.0
    for k in (0, 16, K):
        centre = NP.abs(P[k]).copy()
        centre[16, 16] = 0.0
        side = max(side, float(centre.max()))
        for q in XC.QC.SRC:
            norm = QK.response(per, int(q), k)[2][:, k]
            assert abs(norm[q] - 1.0) <= 1e-12 and NP.all(norm <= 1.0 + 1e-12)
            worst = max(worst, float(NP.max(NP.abs(norm - NP.abs(CS.shifted(P[k], int(q), 17, 17))))))
    print('the normalised response against |P|: %.3f at most, the largest sidelobe of P %.3f' % (worst, side))
    assert worst < 0.5 * side


def test_two_sources_through_a_drifting_chromatic_beam_come_back_in_true_flux():
    c, band = XC.two_sources()
    per = XC.problem(c, pbmin=0.1, share=band)
    args = (0.1, 10000, 5e-3, True, 0.3, 0, 32)
    hogbom = QK.clean(per, 0.1, 10000, 5e-3, True)
    for pb in (per, XC.problem(c, chan_avg=True, pbmin=0.1, share=band)):      # (the case's own band Problem was made before its cube)
        P = XK.beam(pb, 17, 17)
        r = XK.clean(pb, P, 17, 17, *args)
        assert NP.all(r['status'] == XK.THRESHOLD) and r['ncycles'].max() <= 8, (r['status'], r['ncycles'])
        used = r['comp_pixel'][r['comp_pixel'] >= 0]
        assert NP.all(NP.isin(used, XC.QC.SRC)), NP.unique(used)     # no stray component
        dev = XK.replay(pb, P, 17, 17, r, *args)
        eff = r['pb_eff'].reshape(289, pb.nc)
        worst = 0.0
        for k in range(pb.nc):
            n = r['ncomp'][k]
            for q, S in zip(XC.QC.SRC, XC.QC.FLUX):
                total = r['comp_flux'][k, :n][r['comp_pixel'][k, :n] == q].sum()
                worst = max(worst, abs(S - total) * eff[q, k] / (5e-3 * r['peak0'][k]))
        print('nc = %d: %d to %d cycles, %d to %d components, fluxes to %.3f thresholds, replay %.1e of its tolerance'
              % (pb.nc, r['ncycles'].min(), r['ncycles'].max(), r['ncomp'].min(), r['ncomp'].max(), worst, dev))
        assert worst <= 1.5 and dev <= 1e-2
        if pb is per:
            assert NP.all(NP.abs(r['ncomp'] - hogbom['ncomp']) <= 3), (r['ncomp'], hogbom['ncomp'])
            assert NP.all(10 * r['ncycles'] < r['ncomp'])


# ---- the class against a stand-in context ---------------------------------------------------------------------------------------------

class MoscsOracleContext(TM.MosaicOracleContext):
    """MosaicOracleContext whose clean_mosaic_cs is the numpy checker; it records what it was handed."""
    cleans = []

    def clean_mosaic_cs(self, unitvec, grid_shape, rot, pc_dircos, baselines, freqs_hz, beam_kind, diameter_m, beam_pc_dircos=(0.0, 0.0, 1.0),
                        ext=None, cube=None, weights=None, chan_avg=False, aberr_beta=None, pbmin=0.1, gain=0.1, maxiter=10000, threshold=5e-3,
                        threshold_relative=True, cycle_depth=0.3, cycle_niter=0, max_major=32, window=None, fwhm_rad=None, route='auto',
                        minor_route='auto', budget_bytes=0, want_psf=False, want_vis=False):
        call = dict(unitvec=NP.array(unitvec), grid_shape=grid_shape, rot=NP.array(rot), pc=NP.array(pc_dircos), baselines=NP.array(baselines),
                    freqs=NP.array(freqs_hz), beam_kind=beam_kind, diameter=diameter_m, beam_pc=NP.array(beam_pc_dircos), ext=ext,
                    cube=None if cube is None else NP.array(cube), weights=None if weights is None else NP.array(weights), chan_avg=chan_avg,
                    beta=None if aberr_beta is None else NP.array(aberr_beta), pbmin=pbmin, gain=gain, maxiter=maxiter, threshold=threshold,
                    threshold_relative=threshold_relative, cycle_depth=cycle_depth, cycle_niter=cycle_niter, max_major=max_major,
                    window=None if window is None else NP.array(window), fwhm_rad=None if fwhm_rad is None else NP.array(fwhm_rad), route=route,
                    minor_route=minor_route, budget_bytes=budget_bytes, want_vis=want_vis)
        MoscsOracleContext.cleans.append(call)
        nt = call['rot'].reshape(-1, 9).shape[0]
        v = self.cube[:nt] if cube is None else cube
        ny, nx = grid_shape
        pb = QK.Problem(unitvec, rot, pc_dircos, baselines, freqs_hz, v, MK.setups_of(beam_kind, diameter_m, beam_pc_dircos, ext, nt), weights=weights,
                        aberr_beta=aberr_beta, chan_avg=chan_avg, window=window, pbmin=pbmin)
        r = XK.clean(pb, XK.beam(pb, ny, nx), ny, nx, gain, maxiter, threshold, threshold_relative, cycle_depth, cycle_niter, max_major)
        r['psf'], r['restored'] = None, None
        if fwhm_rad is not None:
            r['restored'] = QK.CK.restored(r['residual'], unitvec, r['comp_pixel'], r['comp_flux'], r['ncomp'], NP.broadcast_to(fwhm_rad, (pb.nc,)))
        if not want_vis:
            r['vres'] = None
        r['stats'] = {'route': 'stepped' if route == 'auto' else route, 'minor_route': 'lds' if minor_route == 'auto' else minor_route,
                      'cycles': int(r['ncycles'].max()), 'resident': cube is None}
        return r


def observed(monkeypatch, pointings, reserve=False):
    monkeypatch.setattr(TM, 'MosaicOracleContext', MoscsOracleContext)
    MoscsOracleContext.cleans = []
    return TM.observed(monkeypatch, MC.GAUSS14, pointings, reserve=reserve)


GRID = NP.concatenate((MC.SOURCE_RADEC, MC.SOURCE_RADEC + [[0.0, 1.5]], MC.SOURCE_RADEC + [[2.0, 0.0]], MC.SOURCE_RADEC + [[2.0, 1.5]]))      # 2 x 2


def test_argument_checks_signature_and_exception_types(monkeypatch):
    ia = observed(monkeypatch, [MC.ZENITH] * 3)
    aps = RI.ApertureSynthesis(ia)
    for kw, exc in ((dict(threshold_type='sigma'), ValueError), (dict(threshold=[0.1]), TypeError), (dict(threshold=0.0), ValueError),
                    (dict(threshold=1.0), ValueError), (dict(gain=1), TypeError), (dict(gain=0.0), TypeError), (dict(maxiter=10.0), TypeError),
                    (dict(maxiter=0), ValueError), (dict(coords='galactic'), ValueError), (dict(datakey='vis'), ValueError),
                    (dict(weights=NP.ones(3)), ValueError), (dict(route='fast'), ValueError), (dict(window=NP.ones(8)), ValueError),
                    (dict(window=NP.zeros(4)), ValueError), (dict(fwhm=0.0), ValueError), (dict(fwhm=NP.ones(5)), ValueError),
                    (dict(pbmin=-0.1), ValueError), (dict(pbmin=1.0), ValueError), (dict(pbmin=NP.nan), ValueError),
                    (dict(cycle_depth=0.0), ValueError), (dict(cycle_depth=1.0), ValueError), (dict(cycle_depth=1), ValueError),
                    (dict(cycle_depth=NP.nan), ValueError), (dict(cycle_niter=0), ValueError), (dict(cycle_niter=2.0), ValueError),
                    (dict(max_major=-1), ValueError), (dict(max_major=1.0), ValueError), (dict(max_major=65537), ValueError),
                    (dict(minor_route='fast'), ValueError),
                    (dict(telescope={'shape': 'rect', 'size': 14.0}), NotImplementedError),
                    (dict(telescope={'shape': 'square', 'size': 14.0}), NotImplementedError), (dict(pb_info=[None, None]), ValueError)):
        with pytest.raises(exc):
            aps.clean_mosaic_cotton_schwab(GRID, (2, 2), **dict(dict(coords='radec'), **kw))
    for shape in ((3, 2), (4,), 4, (0, 4), (2, 2, 1), None):
        with pytest.raises(ValueError, match='grid_shape'):
            aps.clean_mosaic_cotton_schwab(GRID, shape, coords='radec')
    ia._extbeam = (NP.ones((12, 2)), NP.eye(2))                       # what set_external_beam leaves
    with pytest.raises(NotImplementedError, match='external beam'):
        aps.clean_mosaic_cotton_schwab(GRID, (2, 2), coords='radec')
    ia._extbeam = None
    assert len(MoscsOracleContext.cleans) == 0                        # nothing reached the device
    p = inspect.signature(aps.clean_mosaic_cotton_schwab).parameters
    assert list(p) == ['directions', 'grid_shape', 'coords', 'datakey', 'weights', 'chan_avg', 'epoch', 'telescope', 'pb_info', 'pbmin', 'gain',
                       'maxiter', 'threshold', 'threshold_type', 'window', 'fwhm', 'restore', 'cycle_depth', 'cycle_niter', 'max_major', 'return_vis',
                       'route', 'minor_route', 'budget_bytes']
    assert [p[n].default for n in list(p)[2:]] == ['dircos', 'noiseless', None, False, None, None, None, 0.1, 0.1, 10000, 5e-3, 'relative', None, None,
                                                   True, 0.3, None, 32, False, 'auto', 'auto', None]
    # the existing entries keep their signatures
    assert list(inspect.signature(aps.clean_mosaic).parameters) == [
        'directions', 'coords', 'datakey', 'weights', 'chan_avg', 'epoch', 'telescope', 'pb_info', 'pbmin', 'gain', 'maxiter', 'threshold',
        'threshold_type', 'window', 'fwhm', 'restore', 'route', 'budget_bytes']
    assert list(inspect.signature(aps.clean_cotton_schwab).parameters) == [
        'directions', 'grid_shape', 'coords', 'datakey', 'weights', 'chan_avg', 'epoch', 'gain', 'maxiter', 'threshold', 'threshold_type',
        'cycle_depth', 'cycle_niter', 'max_major', 'window', 'fwhm', 'restore', 'return_vis', 'route', 'minor_route', 'budget_bytes']
    empty = RI.InterferometerArray(TM.LABELS, TM.BL, TM.CH, telescope=MC.GAUSS14, latitude=TM.LAT, skycoords='radec', pointing_coords='altaz')
    with pytest.raises(ValueError, match='observe'):
        RI.ApertureSynthesis(empty).clean_mosaic_cotton_schwab(GRID, (2, 2), coords='radec')


def test_marshals_as_clean_mosaic_does_and_returns_the_documented_dict(monkeypatch):
    ia = observed(monkeypatch, [MC.ZENITH] * 3)
    aps = RI.ApertureSynthesis(ia)
    cleans = MoscsOracleContext.cleans
    out = aps.clean_mosaic_cotton_schwab(GRID, (2, 2), coords='radec', gain=0.2, maxiter=50, threshold=0.05)
    c, st = cleans[-1], dict(aps.image_stats)
    # what mosaic() hands over, by the same code: the geometry, the cube and the beam of every snapshot
    aps.mosaic(GRID, coords='radec')
    m = TM.MosaicOracleContext.calls[-1]
    for name in ('unitvec', 'rot', 'pc', 'baselines', 'freqs', 'cube', 'beta', 'beam_pc'):
        assert NP.array_equal(c[name], m[name]), name
    assert c['beam_kind'] == m['beam_kind'] == _abi.PRISIM_BEAM_GAUSSIAN and c['diameter'] == m['diameter'] == 14.0 and c['ext'] is None
    assert c['grid_shape'] == (2, 2) and c['pbmin'] == 0.1 and c['weights'] is None and c['window'] is None and c['chan_avg'] is False
    assert (c['gain'], c['maxiter'], c['threshold'], c['threshold_relative'], c['budget_bytes']) == (0.2, 50, 0.05, True, 0)
    assert (c['cycle_depth'], c['cycle_niter'], c['max_major'], c['route'], c['minor_route'], c['want_vis']) == (0.3, 0, 32, 'auto', 'auto', False)
    longest = NP.sqrt((TM.BL ** 2).sum(axis=1)).max()
    assert NP.allclose(c['fwhm_rad'], RI.C_LIGHT / (TM.CH * longest), rtol=1e-15) and NP.allclose(out['fwhm'], NP.degrees(c['fwhm_rad']), rtol=1e-15)
    # the dict: clean_mosaic()'s keys and the two of the cycles; shapes, dtypes
    assert set(out) == {'residual', 'restored', 'residual_flat', 'model', 'components', 'status', 'peak0', 'threshold', 'fwhm', 'cycles', 'residual_vis'}
    assert set(out['components']) == {'pixel', 'flux', 'count'} and set(out['cycles']) == {'count', 'ncomp', 'peak'} and out['residual_vis'] is None
    for name in ('residual', 'restored', 'residual_flat', 'model'):
        assert out[name].shape == (4, 6) and out[name].dtype == NP.float64, name
    n, mc = int(out['components']['count'].max()), int(out['cycles']['count'].max())
    assert out['components']['pixel'].shape == out['components']['flux'].shape == (6, n) and 0 < n <= 50 and 0 < mc <= 32
    assert out['cycles']['count'].shape == (6,) and out['cycles']['ncomp'].shape == (6, mc) and out['cycles']['peak'].shape == (6, mc + 1)
    assert out['cycles']['count'].dtype == out['cycles']['ncomp'].dtype == NP.int32 and out['cycles']['peak'].dtype == NP.float64
    assert out['status'].shape == out['peak0'].shape == out['threshold'].shape == out['fwhm'].shape == (6,) and out['status'].dtype == NP.int32
    assert NP.array_equal(out['threshold'], 0.05 * out['peak0']) and NP.array_equal(out['cycles']['peak'][:, 0], out['peak0'])
    assert set(('num', 'den', 'wsum', 'pb_eff', 'route', 'minor_route', 'resident', 'cycles')) <= set(st)
    assert st['num'].shape == st['den'].shape == (4, 6) and st['wsum'].shape == (6,) and st['pb_eff'].shape == (4, 6) and st['resident'] is False
    assert NP.array_equal(out['residual'], MK.quotient(st['num'], st['den'], st['wsum'], 0.1)[0], equal_nan=True)
    # the one source of the drift scan comes back in true flux on its own pixel
    assert NP.all(out['components']['pixel'][out['components']['pixel'] >= 0] == 0)
    assert NP.all(NP.abs(out['model'][0] - MC.FLUX) <= 0.06 * MC.FLUX) and NP.all(out['model'][1:] == 0.0)
    # chan_avg, an absolute threshold, weights, a window, the cycle settings, no restoration, the residual visibilities
    full_w = NP.random.default_rng(1).uniform(0.5, 1.0, (4, 6, 3))
    window = NP.array([True, True, False, True])
    out = aps.clean_mosaic_cotton_schwab(GRID, (4, 1), coords='radec', weights=full_w, chan_avg=True, threshold=0.5, threshold_type='absolute',
                                         window=window, restore=False, cycle_depth=0.5, cycle_niter=3, max_major=7, return_vis=True, route='direct',
                                         minor_route='global', budget_bytes=1 << 20, pbmin=0.0, maxiter=5)
    c = cleans[-1]
    assert c['weights'].shape == (3, 4, 6) and NP.array_equal(c['weights'], NP.transpose(full_w, (2, 0, 1))) and c['chan_avg'] is True
    assert c['threshold_relative'] is False and c['threshold'] == 0.5 and c['fwhm_rad'] is None and c['route'] == 'direct'
    assert c['budget_bytes'] == 1 << 20 and c['pbmin'] == 0.0 and NP.array_equal(c['window'], window) and c['window'].dtype == bool
    assert (c['grid_shape'], c['cycle_depth'], c['cycle_niter'], c['max_major'], c['minor_route'], c['want_vis']) == ((4, 1), 0.5, 3, 7, 'global', True)
    assert out['residual'].shape == out['model'].shape == out['residual_flat'].shape == (4,) and out['restored'] is None and out['status'].shape == (1,)
    assert NP.array_equal(out['threshold'], [0.5]) and aps.image_stats['pb_eff'].shape == (4,)
    assert out['residual_vis'].shape == (4, 6, 3) and out['residual_vis'].dtype == NP.complex128 and out['residual_vis'].flags['C_CONTIGUOUS']
    # the residual is the mosaic of the residual visibilities
    ia.skyvis_freq, keep = out['residual_vis'], ia.skyvis_freq
    again = aps.mosaic(GRID, coords='radec', weights=full_w, chan_avg=True, pbmin=0.0)
    assert NP.allclose(again, out['residual'], rtol=0, atol=1e-12 * MC.FLUX)
    ia.skyvis_freq = keep


def test_reads_the_resident_cube_where_it_lies(monkeypatch):
    ia = observed(monkeypatch, [MC.ZENITH] * 3, reserve=True)
    aps = RI.ApertureSynthesis(ia)
    res = aps.clean_mosaic_cotton_schwab(GRID, (2, 2), coords='radec', maxiter=20)
    assert MoscsOracleContext.cleans[-1]['cube'] is None and aps.image_stats['resident'] is True
    ia.skyvis_freq = NP.array(ia.skyvis_freq)                         # replaced: the slots are out of step, the cube is handed over
    host = aps.clean_mosaic_cotton_schwab(GRID, (2, 2), coords='radec', maxiter=20)
    assert MoscsOracleContext.cleans[-1]['cube'] is not None and aps.image_stats['resident'] is False
    assert NP.array_equal(res['residual'], host['residual'], equal_nan=True) and NP.array_equal(res['model'], host['model'])
