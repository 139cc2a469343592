"""CPU: CLEAN of the beam-weighted mosaic (include/prisim_mosclean.h) -- the export, both structs and the constants against the compiled
header, the planning header under ASan and UBSan in a host program of its own (tests/mosclean_plan_main.cpp), the numpy checker
against itself (tests/mosclean_checker.py: the independent CLEAN against the replay, the monotone cost, the Cauchy-Schwarz property
of the search image, the replay against wrong decisions, the delta-beam case against tests/imclean_checker.py), the input conditions
of the GPU tests, and the class prisim_amd.interferometry.ApertureSynthesis.clean_mosaic against a stand-in context that answers
clean_mosaic with the checker.

Bounds.  The replay's tolerances are the ones the device is held to (tests/test_gpu_mosclean.py), derived in the checker's docstring.
The checker's own CLEAN and its replay evaluate the same numpy expressions, so they agree far inside them; what this file shows of
the replay is that it fails where a decision is wrong by more than the tolerance."""
import ctypes as C
import inspect
import os
import subprocess
import sys

import numpy as NP
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import imaging_cases as IC  # noqa: E402
import imclean_checker as CK  # noqa: E402
import mosaic_cases as MC  # noqa: E402
import mosaic_checker as MK  # noqa: E402
import mosclean_cases as QC  # noqa: E402
import mosclean_checker as QK  # noqa: E402
import test_mosaic as TM  # noqa: E402  (the arrays, the drift scan and the stand-in context of the mosaic tests)

from prisim_amd import _abi  # noqa: E402
from prisim_amd import interferometry as RI  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the library and its headers ----------------------------------------------------------------------------------------------------

def test_export_is_in_the_library_and_outside_the_core_abi():
    lib = _abi.load_library()
    assert _abi.MOSCLEAN_EXPORTS == ('prisim_clean_mosaic',) == _abi.HEADER_EXPORTS['prisim_mosclean.h'] and 'prisim_clean_mosaic' not in _abi.EXPORTS
    assert lib.prisim_clean_mosaic(*[None] * 15) == _abi.PRISIM_EINVAL          # a null context and null args are refused, not read
    assert not hasattr(_abi, 'PrisimMoscleanStats')                   # the struct lives on the class (tests/test_abi_helpers.py)
    assert set(_abi._stats_dict(_abi.Context.PrisimMoscleanStats())) == {
        'wall_ms', 'kernel_ms', 'mosaic_ms', 'peak_ms', 'update_ms', 'restore_ms', 'terms', 'beam_values', 'iterations', 'components', 'polls',
        'chunks', 'chunk_pixels', 'kernel_bytes', 'upload_bytes', 'download_bytes', 'device_bytes', 'route', 'streams', 'chan_tile', 'reseed',
        'lds_bytes', 'block_pixels'}
    # the arguments are those of the mosaic in their order, then those of the CLEAN
    names = [n for n, _ in _abi.Context.PrisimMoscleanArgs._fields_]
    mosaic = [n for n, _ in _abi.Context.PrisimMosaicArgs._fields_]
    assert names[:len(mosaic)] == mosaic and names[len(mosaic):] == ['gain', 'maxiter', 'threshold', 'threshold_relative', 'window', 'fwhm_rad',
                                                                      'poll_every']
    folder = os.path.join(ROOT, 'prisim_amd', 'csrc_imaging')
    src = {name: open(os.path.join(folder, name)).read() for name in os.listdir(folder)}
    new = src['mosclean.hip']
    # what the entry joins is called, not restated: the mosaic's kernels, the CLEAN's bookkeeping, the tile pass, the beam
    for name in ('k_mos_wsum', 'k_mos_sum', 'k_mos_finish', 'k_mos_finish_band', 'struct MosParams'):
        assert [f for f, txt in src.items() if '__global__' in txt and name + '(' in txt.replace('launch(ctx, ' + name, '')
                or name in txt and name.startswith('struct') and name + ' {' in txt] == ['mosaic_kernels.h'], name
    for name in ('struct Peak', 'struct CleanState', 'struct BatchEvents', 'bool peak_beats(', 'void __launch_bounds__(kThreads) k_imclean_init(',
                 'void __launch_bounds__(kThreads) k_imclean_peak1(', 'void __launch_bounds__(kThreads) k_imclean_peak2(',
                 'void __launch_bounds__(kThreads) k_imclean_restore(', 'hipMemcpyAsync(counts, S.counts'):
        assert [f for f, txt in src.items() if name in txt] == ['clean_kernels.h'], name
    # the update is one kernel for this entry and prisim_clean_image: its accumulators, its tile pass and its operand's phasor are
    # written in one file of the directory, besides the dirty image, the mosaic's sum and the model of the Cotton-Schwab cycles
    upd = src['clean_update.h']
    assert upd.count('double acc[CT];') == 1 and upd.count('img_tile_pass<STEPPED, false>(') == 1 and upd.count('cycles_phasor(') == 1       # one set of accumulators
    assert sorted(f for f, txt in src.items() if 'double acc[CT];' in txt) == ['clean_update.h', 'dirty_image.h', 'mosaic_kernels.h']
    assert sorted(f for f, txt in src.items() if 'img_tile_pass<STEPPED, false>(' in txt.replace('img_tile_pass<STEPPED, false>(...)', '')) == [
        'clean_update.h', 'mosaic_kernels.h']
    assert sorted(f for f, txt in src.items() if 'cycles_phasor(' in txt) == ['clean_update.h', 'csclean.hip', 'imaging_kernels.h']
    assert 'template <bool STEPPED, bool MOSAIC>' in upd and 'img_rows' not in upd
    for entry in (new, src['imclean.hip']):
        assert 'img_tile_pass' not in entry and 'sh_b[tid] =' not in entry and 'img_rows' not in entry and 'double acc' not in entry
    assert 'enqueue_clean_update<true>(' in new and 'enqueue_clean_update<false>(' in src['imclean.hip'] and 'enqueue_mos_sum(' in new
    # the frame of a call is one: its checks, the launches of the peak search, of the decision and of the restoration are written once
    assert 'enqueue_mos_beam(' in new and 'fill_beam(' not in new and 'check_mosaic_beam(' in new
    for name in ('check_clean_args(ctx', 'launch(ctx, k_imclean_init', 'launch(ctx, k_imclean_peak1', 'launch(ctx, k_imclean_peak2<', 'launch(ctx, k_imclean_restore',
                 'alloc_clean_state(ctx', 'DEV_UPLOAD(ctx, wk.dev, d_fwhm', 'lists.enqueue(', 'lists.write(', 'out_status or out_peak0 is NULL'):
        assert [f for f, txt in src.items() if name in txt.replace('inline int ' + name, '')] == ['clean_kernels.h'], name
    assert not [f for f, txt in src.items() if 'hipLaunchKernelGGL(k_imclean' in txt]
    shared = src['clean_kernels.h']
    for entry in (new, src['imclean.hip'], src['csclean.hip']):
        for step in ('.check_outputs(', '.check_inputs(', '.open(', '.search(', '.close(', '.gather(', '.write(', '.common_stats(', 'clean_refusal('):
            assert step in entry, step
        # the stream drains when the frame goes: the host buffers a copy may still be filling are declared before it, so they go after it
        body = entry[entry.index('  CleanCall '):entry.index('extern "C"')]
        for kind in ('std::vector<double>', 'std::vector<int32_t>', 'DirtyResidual ', 'CleanLoop '):
            assert kind not in body, kind
    frame = shared[shared.index('struct CleanCall {'):shared.index('  CleanCall(prisim_ctx*')]
    assert all(frame.index(member) < frame.index('Work wk;') for member in ('ImgTables T;', 'CleanLists lists;', 'h_res, h_rest;'))
    assert frame.rstrip().splitlines()[-1].lstrip().startswith('Work wk;')          # the last member
    assert 'struct MosaicFlux' in new and 'MosaicFlux' not in src['imclean.hip'] and 'ResidualFlux' in src['imclean.hip']
    assert '.decide(' in new and '.decide(' in src['imclean.hip'] and '.decide(' not in src['csclean.hip']
    assert (_abi.PRISIM_IMCLEAN_THRESHOLD, _abi.PRISIM_IMCLEAN_MAXITER, _abi.PRISIM_IMCLEAN_DEAD) == (QK.THRESHOLD, QK.MAXITER, QK.DEAD)
    # an add-on: one name in the Makefile, nothing under csrc/
    mk = open(os.path.join(ROOT, 'prisim_amd', 'csrc', 'Makefile')).read()
    assert mk.count('mosclean') == 1 and not [f for f in os.listdir(os.path.join(ROOT, 'prisim_amd', 'csrc')) if 'mosclean' in f]


def test_structs_and_constants_against_the_compiled_header(tmp_path):
    """sizeof and every offsetof of prisim_mosclean_args and prisim_mosclean_stats as gcc lays them out, against the ctypes mirrors"""
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "prisim_mosclean.h"', 'int main(void) {']
    mirrors = {'prisim_mosclean_args': _abi.Context.PrisimMoscleanArgs, 'prisim_mosclean_stats': _abi.Context.PrisimMoscleanStats}
    for cname, cls in mirrors.items():
        lines.append('  printf("%zu\\n", sizeof({0}));'.format(cname))
        lines += ['  printf("%zu\\n", offsetof({0}, {1}));'.format(cname, f) for f, _ in cls._fields_]
    lines += ['  printf("%d %d %d %d %d\\n", PRISIM_IMCLEAN_THRESHOLD, PRISIM_IMCLEAN_MAXITER, PRISIM_IMCLEAN_DEAD, PRISIM_IMCLEAN_POLL_DEFAULT, '
              'PRISIM_IMCLEAN_POLL_MAX);', '  return 0;', '}']
    (tmp_path / 'm.c').write_text('\n'.join(lines))
    subprocess.check_call(['gcc', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), str(tmp_path / 'm.c'), '-o', str(tmp_path / 'm')])
    out = subprocess.check_output([str(tmp_path / 'm')]).decode().split('\n')
    want = []
    for cls in mirrors.values():
        want += [str(C.sizeof(cls))] + [str(getattr(cls, f).offset) for f, _ in cls._fields_]
    assert out[:len(want)] == want
    assert out[len(want)].split() == [str(v) for v in (_abi.PRISIM_IMCLEAN_THRESHOLD, _abi.PRISIM_IMCLEAN_MAXITER, _abi.PRISIM_IMCLEAN_DEAD,
                                                       _abi.PRISIM_IMCLEAN_POLL_DEFAULT, _abi.PRISIM_IMCLEAN_POLL_MAX)]


def test_plan_header_under_the_sanitizers(tmp_path):
    exe = tmp_path / 'mosclean_plan_main'
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-I',
                           os.path.join(ROOT, 'prisim_amd', 'csrc_addon'), os.path.join(ROOT, 'tests', 'mosclean_plan_main.cpp'), '-o', str(exe)])
    res = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = res.stdout.decode()
    assert res.returncode == 0, out
    last = out.strip().splitlines()[-1].split()
    assert last[0] == 'checked' and int(last[1]) > 20000 and last[2:] == ['bad', '0'], out
    txt = open(os.path.join(ROOT, 'prisim_amd', 'csrc_addon', 'mosclean_plan.h')).read()
    assert '#include <hip' not in txt and '__device__' not in txt and '#include "addon_internal.h"' not in txt
    assert 'imclean_plan(' in txt and 'kImagingBlock' not in txt and 'kImcleanMaxSlabs' not in txt      # asked of imclean_plan, not restated


# ---- the checker against itself -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def small():
    """37 baselines, 5 channels, 63 pixels over the upper hemisphere, 3 snapshots, the 2 m Airy dish with a pointing that moves"""
    c = QC.parity_case((37, 5, 63, 3))
    return c, QC.problem(c, 'airy', weights=c['w_full'], pbmin=0.1)


@pytest.mark.parametrize('chan_avg', [False, True])
def test_independent_clean_against_the_replay_and_the_cost_never_grows(small, chan_avg):
    c, pb0 = small
    window = NP.arange(63) % 3 != 1
    pb = QC.problem(c, 'airy', weights=c['w_full'], chan_avg=chan_avg, window=window, pbmin=0.1, share=pb0)
    assert 0.1 <= QC.assert_mask_keeps_and_cuts(pb) <= 0.9
    # the first residual is the mosaic checker's
    want = MK.mosaic(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], c['cube'], pb.setups, weights=c['w_full'], aberr_beta=c['beta'])
    assert NP.all(NP.abs(pb.numerator(pb.v) - want['num']) <= 1e-2 * want['bound_num']) and NP.all(NP.abs(pb.Q - want['den']) <= 1e-2 * want['bound_den'])
    for gain, maxiter, thr, rel in ((0.3, 25, 0.0, False), (0.1, 40, 0.5, True), (1.0, 3, 0.2, True), (0.5, 0, 0.1, False)):
        costs = []
        r = QK.clean(pb, gain, maxiter, thr, rel, costs=costs)
        worst = QK.replay(pb, r, gain, maxiter, thr, rel)
        print('gain %.1f maxiter %d threshold %.1f: %d components, worst deviation %.2e of its tolerance' % (gain, maxiter, thr, r['ncomp'].sum(), worst))
        used = r['comp_pixel'][r['comp_pixel'] >= 0]
        assert worst <= 1e-2 and NP.all(window[used])
        assert NP.all(r['ncomp'] <= maxiter) and NP.all((r['status'] == QK.MAXITER) == ((r['ncomp'] == maxiter) & (r['status'] != QK.THRESHOLD)))
        # matching pursuit in the weighted visibility space: sum w |V - model|^2 does not grow from one iteration to the next, for any
        # drift and chromaticity of the beam, at gain 1 either
        assert len(costs) == int(r['ncomp'].max()) + 1
        for before, after in zip(costs[:-1], costs[1:]):
            assert NP.all(after <= before * (1 + 1e-12)), (gain, before, after)
        if maxiter == 0:
            assert NP.array_equal(r['num'], pb.numerator(pb.v)) and r['comp_pixel'].shape == (pb.nc, 0)
            assert NP.array_equal(r['residual'], MK.quotient(r['num'], r['den'], r['wsum'], 0.1, chan_avg)[0], equal_nan=True)
        else:
            assert costs[-1].sum() < costs[0].sum()


def test_the_search_image_never_answers_louder_off_the_components_own_pixel():
    """Cauchy-Schwarz, on the drifting chromatic case of the two sources: |F_c[p]| <= F_c[q] = sqrt(Q[q] / W) for a unit component at q,
    at every pixel, per channel and for the band; N_c / Q, which a search on the mosaic itself would see, grows towards the rim."""
    c, band = QC.two_sources()
    per = QC.problem(c, 'gaussian', pbmin=0.1, share=band)
    rng = NP.random.default_rng(5)
    louder = 0
    for pb, ks in ((per, (0, 16, 32)), (band, (0,))):
        for k in ks:
            for q in list(QC.SRC) + rng.integers(0, 289, 6).tolist():
                Nc, Fc, norm = QK.response(pb, int(q), k)
                own = NP.sqrt(pb.Qc[q, k] / pb.Wc[k])
                assert abs(Nc[q, k] - pb.Qc[q, k]) <= 1e-12 * pb.Qc[q, k] and abs(Fc[q, k] - own) <= 1e-12 * own
                assert NP.all(Fc[:, k] <= own * (1 + 1e-12)) and NP.all(norm[:, k] <= 1 + 1e-12)
                louder += int(NP.max(NP.abs(Nc[:, k]) / pb.Qc[:, k]) > 1 + 1e-6)
    assert louder > 0                                                 # the mosaic's own response does exceed 1 off the pixel somewhere


def test_the_two_sources_case_is_what_the_gpu_test_relies_on():
    c, band = QC.two_sources()
    A = band.A[:, QC.SRC, :]
    print('the beam at the two sources: %.3f .. %.3f' % (A.min(), A.max()))
    assert 0.3 <= A.min() and A.max() <= 0.9 and NP.all(NP.abs(A[:, 0] - A[:, 1]) > 0.05)
    assert NP.all(NP.abs(A[:, :, 0] - A[:, :, -1]) > 0.004)           # chromatic: the band's ends differ at both sources
    per = QC.problem(c, 'gaussian', pbmin=0.1, share=band)
    worst = 0.0
    for k in range(33):
        for q in QC.SRC:
            norm = QK.response(per, int(q), k)[2][:, k].copy()
            norm[q] = 0.0
            worst = max(worst, float(NP.max(norm)))
    print('worst normalised off-pixel response: %.3f' % worst)
    assert worst < 1.0 / 3.0
    # the mosaic of the cube returns the fluxes; the dirty image does not
    ref = MK.combine(MK.snapshot_sums(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], c['cube']), band.A, pbmin=0.1)
    img = CK.Problem(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], c['cube']).dirty(c['cube'])
    assert NP.all(NP.abs(img[QC.SRC[0]] - 1.0) > 0.3) and NP.all(NP.abs(ref['mosaic'][QC.SRC[0]] - 1.0) < 0.2)


def test_replay_refuses_wrong_decisions(small):
    c, pb = small
    args = (0.3, 25, 0.5, True)
    r = QK.clean(pb, *args)
    assert len(set(r['ncomp'].tolist())) > 1 and NP.any(r['status'] == QK.THRESHOLD)      # the channels end at different places
    QK.replay(pb, r, *args)

    def tampered(**kw):
        out = {k: NP.array(v) for k, v in r.items()}
        for name, (index, value) in kw.items():
            out[name][index] = value
        return out

    k = int(NP.argmax(r['ncomp']))
    assert r['ncomp'][k] >= 4
    F0 = pb.flat(pb.numerator(pb.v))[:, k]
    second = NP.argsort(NP.where(pb.search[:, k], NP.abs(F0), -1.0))[-2]      # the second largest of the first search image
    masked = int(NP.flatnonzero(~pb.valid[:, k])[0])
    wrong = [tampered(comp_pixel=((k, 0), second)),                   # a pick that is not the peak
             tampered(comp_pixel=((k, 0), masked)),                   # a pick on a masked pixel
             tampered(comp_flux=((k, 3), r['comp_flux'][k, 3] * (1 + 1e-9))),      # a flux off by 1e-9 of itself
             tampered(comp_flux=((k, 3), -r['comp_flux'][k, 3])),
             tampered(num=((5, k), r['num'][5, k] + 1e-9 * pb.absV[:, k].sum())),   # a numerator off by far more than the tolerance
             tampered(status=(k, QK.THRESHOLD if r['status'][k] == QK.MAXITER else QK.MAXITER)),      # a wrong status
             tampered(status=(k, QK.DEAD)), tampered(peak0=(k, r['peak0'][k] * (1 + 1e-9)))]
    with pytest.raises(AssertionError, match='masked'):
        QK.replay(pb, wrong[1], *args)
    # a stop one component early: the peak is still above the threshold
    early = tampered(ncomp=(k, r['ncomp'][k] - 1), status=(k, QK.THRESHOLD))
    early['comp_pixel'][k, r['ncomp'][k] - 1], early['comp_flux'][k, r['ncomp'][k] - 1] = -1, 0.0
    if NP.max(NP.delete(r['ncomp'], k)) < r['ncomp'][k]:
        early['comp_pixel'], early['comp_flux'] = early['comp_pixel'][:, :-1], early['comp_flux'][:, :-1]
    wrong.append(early)
    # a quotient that is not the header's expression of the returned sums
    wrong.append(tampered(residual=((int(NP.flatnonzero(pb.valid[:, k])[0]), k), 0.0)))
    for bad in wrong:
        with pytest.raises(AssertionError):
            QK.replay(pb, bad, *args)
    # a pick outside the window
    win = NP.ones(63, dtype=bool)
    later = [q for q in r['comp_pixel'][k, :r['ncomp'][k]] if q not in r['comp_pixel'][:, 0]]
    win[later[0]] = False                                             # not the first peak of any channel: every P0 stands
    pbw = QC.problem(c, 'airy', weights=c['w_full'], window=win, pbmin=0.1, share=pb)
    with pytest.raises(AssertionError, match='window'):
        QK.replay(pbw, r, *args)


def test_a_delta_beam_on_one_snapshot_is_the_clean_of_the_dirty_image():
    """A = 1 everywhere: N = D, Q = W, F = D / W and a = gain D / W, the quantities of tests/imclean_checker.py -- to tolerance, not bit
    for bit: the divisions come in another order (N / sqrt(Q W) against D / W, the update before the division against after it)."""
    c = MC.up_case(37, 5, 63, 1)
    setups = [{'element': 'delta'}]
    for chan_avg in (False, True):
        pb = QK.Problem(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], c['cube'], setups, weights=c['w_bl'], aberr_beta=c['beta'],
                        chan_avg=chan_avg, pbmin=0.1)
        assert NP.all(pb.A == 1.0) and NP.all(pb.valid)
        got = QK.clean(pb, 0.3, 25, 0.0, False)
        im = CK.Problem(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], c['cube'], weights=c['w_bl'], aberr_beta=c['beta'], chan_avg=chan_avg)
        # the replay of the dirty-image CLEAN accepts the mosaic CLEAN's decisions, residual and first peak
        as_image = dict(got, residual=got['residual'])
        worst = CK.replay(im, as_image, 0.3, 25, 0.0, False)
        print('chan_avg=%d: the mosaic CLEAN under the replay of the dirty-image CLEAN, worst deviation %.2e of its tolerance' % (chan_avg, worst))
        assert worst <= 1e-2
        assert NP.allclose(got['residual_flat'], got['residual'], rtol=1e-13, atol=0) and NP.all(got['pb_eff'] == 1.0)


# ---- the class against a stand-in context ---------------------------------------------------------------------------------------------

class MoscleanOracleContext(TM.MosaicOracleContext):
    """MosaicOracleContext whose clean_mosaic is the numpy checker; it records what it was handed."""
    cleans = []

    def clean_mosaic(self, unitvec, rot, pc_dircos, baselines, freqs_hz, beam_kind, diameter_m, beam_pc_dircos=(0.0, 0.0, 1.0), ext=None, cube=None,
                     weights=None, chan_avg=False, aberr_beta=None, pbmin=0.1, gain=0.1, maxiter=10000, threshold=5e-3, threshold_relative=True,
                     window=None, fwhm_rad=None, route='auto', budget_bytes=0, poll_every=0):
        call = dict(unitvec=NP.array(unitvec), rot=NP.array(rot), pc=NP.array(pc_dircos), baselines=NP.array(baselines), freqs=NP.array(freqs_hz),
                    beam_kind=beam_kind, diameter=diameter_m, beam_pc=NP.array(beam_pc_dircos), ext=ext,
                    cube=None if cube is None else NP.array(cube), weights=None if weights is None else NP.array(weights), chan_avg=chan_avg,
                    beta=None if aberr_beta is None else NP.array(aberr_beta), pbmin=pbmin, gain=gain, maxiter=maxiter, threshold=threshold,
                    threshold_relative=threshold_relative, window=None if window is None else NP.array(window),
                    fwhm_rad=None if fwhm_rad is None else NP.array(fwhm_rad), route=route, budget_bytes=budget_bytes)
        MoscleanOracleContext.cleans.append(call)
        nt = call['rot'].reshape(-1, 9).shape[0]
        v = self.cube[:nt] if cube is None else cube
        r = QK.answer(unitvec, rot, pc_dircos, baselines, freqs_hz, v, MK.setups_of(beam_kind, diameter_m, beam_pc_dircos, ext, nt), weights=weights,
                      chan_avg=chan_avg, aberr_beta=aberr_beta, pbmin=pbmin, gain=gain, maxiter=maxiter, threshold=threshold,
                      threshold_relative=threshold_relative, window=window, fwhm_rad=fwhm_rad)
        r['stats'] = {'route': 'stepped' if route == 'auto' else route, 'iterations': int(r['ncomp'].max()), 'resident': cube is None}
        return r


def observed(monkeypatch, pointings, reserve=False):
    monkeypatch.setattr(TM, 'MosaicOracleContext', MoscleanOracleContext)
    MoscleanOracleContext.cleans = []
    return TM.observed(monkeypatch, MC.GAUSS14, pointings, reserve=reserve)


def test_clean_mosaic_argument_checks_and_exception_types(monkeypatch):
    ia = observed(monkeypatch, [MC.ZENITH] * 3)
    aps = RI.ApertureSynthesis(ia)
    d = MC.SOURCE_RADEC
    for kw, exc in ((dict(threshold_type='sigma'), ValueError), (dict(threshold=[0.1]), TypeError), (dict(threshold=0.0), ValueError),
                    (dict(threshold=1.0), ValueError), (dict(gain=1), TypeError), (dict(gain=0.0), TypeError), (dict(maxiter=10.0), TypeError),
                    (dict(maxiter=0), ValueError), (dict(coords='galactic'), ValueError), (dict(datakey='vis'), ValueError),
                    (dict(weights=NP.ones(3)), ValueError), (dict(route='fast'), ValueError), (dict(window=NP.ones(8)), ValueError),
                    (dict(window=NP.zeros(1)), ValueError), (dict(fwhm=0.0), ValueError), (dict(fwhm=NP.ones(5)), ValueError),
                    (dict(pbmin=-0.1), ValueError), (dict(pbmin=1.0), ValueError), (dict(pbmin=NP.nan), ValueError),
                    (dict(telescope={'shape': 'rect', 'size': 14.0}), NotImplementedError),
                    (dict(telescope={'shape': 'square', 'size': 14.0}), NotImplementedError), (dict(pb_info=[None, None]), ValueError)):
        with pytest.raises(exc):
            aps.clean_mosaic(d, **dict(dict(coords='radec'), **kw))
    ia._extbeam = (NP.ones((12, 2)), NP.eye(2))                       # what set_external_beam leaves
    with pytest.raises(NotImplementedError, match='external beam'):
        aps.clean_mosaic(d, coords='radec')
    ia._extbeam = None
    assert len(MoscleanOracleContext.cleans) == 0                     # nothing reached the device
    assert list(inspect.signature(aps.clean_mosaic).parameters) == [
        'directions', 'coords', 'datakey', 'weights', 'chan_avg', 'epoch', 'telescope', 'pb_info', 'pbmin', 'gain', 'maxiter', 'threshold',
        'threshold_type', 'window', 'fwhm', 'restore', 'route', 'budget_bytes']
    p = inspect.signature(aps.clean_mosaic).parameters
    assert [p[n].default for n in ('coords', 'datakey', 'pbmin', 'gain', 'maxiter', 'threshold', 'threshold_type', 'restore', 'route')] == [
        'dircos', 'noiseless', 0.1, 0.1, 10000, 5e-3, 'relative', True, 'auto']
    # the existing entries keep their signatures
    assert list(inspect.signature(aps.mosaic).parameters) == ['directions', 'coords', 'datakey', 'weights', 'chan_avg', 'epoch', 'telescope',
                                                              'pb_info', 'pbmin', 'route', 'budget_bytes']
    assert list(inspect.signature(aps.clean).parameters) == ['directions', 'coords', 'datakey', 'weights', 'chan_avg', 'epoch', 'gain', 'maxiter',
                                                             'threshold', 'threshold_type', 'window', 'fwhm', 'restore', 'route', 'budget_bytes']


def test_clean_mosaic_marshals_as_mosaic_does_and_returns_the_documented_dict(monkeypatch):
    ia = observed(monkeypatch, [MC.ZENITH] * 3)
    aps = RI.ApertureSynthesis(ia)
    cleans = MoscleanOracleContext.cleans
    grid = NP.concatenate((MC.SOURCE_RADEC, MC.SOURCE_RADEC + [[0.0, 1.5]], MC.SOURCE_RADEC + [[2.0, -1.0]], MC.SOURCE_RADEC + [[-1.5, 0.5]]))
    out = aps.clean_mosaic(grid, coords='radec', gain=0.2, maxiter=50, threshold=0.05)
    c, st = cleans[-1], dict(aps.image_stats)
    # what mosaic() hands over, by the same code: the geometry, the cube and the beam of every snapshot
    aps.mosaic(grid, coords='radec')
    m = TM.MosaicOracleContext.calls[-1]
    for name in ('unitvec', 'rot', 'pc', 'baselines', 'freqs', 'cube', 'beta', 'beam_pc'):
        assert NP.array_equal(c[name], m[name]), name
    assert c['beam_kind'] == m['beam_kind'] == _abi.PRISIM_BEAM_GAUSSIAN and c['diameter'] == m['diameter'] == 14.0 and c['ext'] is None
    assert c['beam_pc'].shape == (3,) and c['pbmin'] == 0.1 and c['weights'] is None and c['window'] is None and c['route'] == 'auto'
    assert (c['gain'], c['maxiter'], c['threshold'], c['threshold_relative'], c['budget_bytes']) == (0.2, 50, 0.05, True, 0)
    longest = NP.sqrt((TM.BL ** 2).sum(axis=1)).max()
    assert NP.allclose(c['fwhm_rad'], RI.C_LIGHT / (TM.CH * longest), rtol=1e-15) and NP.allclose(out['fwhm'], NP.degrees(c['fwhm_rad']), rtol=1e-15)
    # the dict: keys, shapes, dtypes
    assert set(out) == {'residual', 'restored', 'residual_flat', 'model', 'components', 'status', 'peak0', 'threshold', 'fwhm'}
    assert set(out['components']) == {'pixel', 'flux', 'count'}
    for name in ('residual', 'restored', 'residual_flat', 'model'):
        assert out[name].shape == (4, 6) and out[name].dtype == NP.float64, name
    n = int(out['components']['count'].max())
    assert out['components']['pixel'].shape == out['components']['flux'].shape == (6, n) and 0 < n <= 50
    assert out['components']['pixel'].dtype == NP.int32 and out['components']['flux'].dtype == NP.float64 and out['components']['count'].dtype == NP.int32
    assert out['status'].shape == out['peak0'].shape == out['threshold'].shape == out['fwhm'].shape == (6,) and out['status'].dtype == NP.int32
    assert NP.array_equal(out['threshold'], 0.05 * out['peak0'])
    assert set(('num', 'den', 'wsum', 'pb_eff', 'route', 'resident', 'iterations')) <= set(st)
    assert st['num'].shape == st['den'].shape == (4, 6) and st['wsum'].shape == (6,) and st['pb_eff'].shape == (4, 6) and st['resident'] is False
    assert NP.array_equal(out['residual'], MK.quotient(st['num'], st['den'], st['wsum'], 0.1)[0], equal_nan=True)
    # the one source of the drift scan comes back in true flux on its own pixel
    assert NP.all(out['components']['pixel'][out['components']['pixel'] >= 0] == 0)
    assert NP.all(NP.abs(out['model'][0] - MC.FLUX) <= 0.06 * MC.FLUX) and NP.all(out['model'][1:] == 0.0)
    # chan_avg, an absolute threshold, weights, a window, no restoration, the other arguments handed on
    full_w = NP.random.default_rng(1).uniform(0.5, 1.0, (4, 6, 3))
    window = NP.array([True, True, False, True])
    out = aps.clean_mosaic(grid, coords='radec', weights=full_w, chan_avg=True, threshold=0.5, threshold_type='absolute', window=window,
                           restore=False, route='direct', budget_bytes=1 << 20, pbmin=0.0, maxiter=5)
    c = cleans[-1]
    assert c['weights'].shape == (3, 4, 6) and NP.array_equal(c['weights'], NP.transpose(full_w, (2, 0, 1))) and c['chan_avg'] is True
    assert c['threshold_relative'] is False and c['threshold'] == 0.5 and c['fwhm_rad'] is None and c['route'] == 'direct'
    assert c['budget_bytes'] == 1 << 20 and c['pbmin'] == 0.0 and NP.array_equal(c['window'], window) and c['window'].dtype == bool
    assert out['residual'].shape == out['model'].shape == out['residual_flat'].shape == (4,) and out['restored'] is None and out['status'].shape == (1,)
    assert NP.array_equal(out['threshold'], [0.5]) and aps.image_stats['pb_eff'].shape == (4,)
    # a pointing that moves: the element pointing of every snapshot, as mosaic() hands it over
    ia = observed(monkeypatch, [[90.0, 270.0], [88.0, 10.0], [87.0, 200.0]])
    aps = RI.ApertureSynthesis(ia)
    aps.clean_mosaic(grid, coords='radec', maxiter=3)
    aps.mosaic(grid, coords='radec')
    c, m = MoscleanOracleContext.cleans[-1], TM.MosaicOracleContext.calls[-1]
    assert c['beam_pc'].shape == (3, 3) and NP.array_equal(c['beam_pc'], m['beam_pc']) and c['ext'] is None and m['ext'] is None


def test_clean_mosaic_reads_the_resident_cube_where_it_lies(monkeypatch):
    ia = observed(monkeypatch, [MC.ZENITH] * 3, reserve=True)
    aps = RI.ApertureSynthesis(ia)
    res = aps.clean_mosaic(MC.SOURCE_RADEC, coords='radec', maxiter=20)
    assert MoscleanOracleContext.cleans[-1]['cube'] is None and aps.image_stats['resident'] is True
    ia.skyvis_freq = NP.array(ia.skyvis_freq)                         # replaced: the slots are out of step, the cube is handed over
    host = aps.clean_mosaic(MC.SOURCE_RADEC, coords='radec', maxiter=20)
    assert MoscleanOracleContext.cleans[-1]['cube'] is not None and aps.image_stats['resident'] is False
    assert NP.array_equal(res['residual'], host['residual']) and NP.array_equal(res['model'], host['model'])
