"""CPU: Hogbom CLEAN of dirty images with the exact beam (include/prisim_imclean.h) -- the export (tests/test_abi_headers.py holds the
ctypes mirrors, the constants and the prototype to the header), the planning header under ASan and UBSan in a host program of its
own (tests/imclean_plan_main.cpp), the numpy checker against itself (tests/imclean_checker.py: the independent CLEAN against the
replay, and the replay against wrong decisions), the linearity identity, and the class
prisim_amd.interferometry.ApertureSynthesis.clean against a stand-in context that answers clean_image with the checker.

Bounds.  The replay's tolerance is the one the device is held to (tests/test_gpu_imclean.py): 1e-11 of the natural scale plus the
sum of |a| so far.  The checker's own CLEAN and its replay evaluate the same numpy expressions, so they agree far inside it; what this
file shows of the replay is that it fails where a decision is wrong by more than the tolerance."""
import os
import subprocess
import sys

import numpy as NP
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import imaging_cases as IC  # noqa: E402
import imaging_checker as IK  # noqa: E402
import imclean_checker as CK  # noqa: E402
import test_imaging as TI  # noqa: E402  (the arrays, the sky and the stand-in context of the imaging tests)

from prisim_amd import _abi  # noqa: E402
from prisim_amd import interferometry as RI  # noqa: E402
from prisim_amd import skymodel as SM  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the library and its headers ----------------------------------------------------------------------------------------------------

def test_export_is_in_the_library_and_outside_the_core_abi():
    lib = _abi.load_library()
    assert _abi.IMCLEAN_EXPORTS == ('prisim_clean_image',) and 'prisim_clean_image' not in _abi.EXPORTS
    assert lib.prisim_clean_image(*[None] * 11) == _abi.PRISIM_EINVAL          # a null context and null args are refused, not read
    assert not hasattr(_abi, 'PrisimImcleanStats')                    # the struct lives on the class (tests/test_abi_helpers.py)
    assert set(_abi._stats_dict(_abi.Context.PrisimImcleanStats())) == {
        'wall_ms', 'kernel_ms', 'dirty_ms', 'peak_ms', 'update_ms', 'restore_ms', 'terms', 'iterations', 'components', 'polls', 'chunks',
        'chunk_pixels', 'kernel_bytes', 'upload_bytes', 'download_bytes', 'device_bytes', 'route', 'streams', 'chan_tile', 'reseed',
        'lds_bytes', 'block_pixels'}
    assert (_abi.PRISIM_IMCLEAN_THRESHOLD, _abi.PRISIM_IMCLEAN_MAXITER, _abi.PRISIM_IMCLEAN_DEAD) == (CK.THRESHOLD, CK.MAXITER, CK.DEAD) == (1, 2, 4)
    src = open(os.path.join(ROOT, 'prisim_amd', 'csrc_imaging', 'imclean.hip')).read()
    assert 'atomic' not in src.replace('No atomics', '') and '#include "dirty_image.h"' in src
    # the dirty image of both entries is one set of kernels, enqueued by one function; the update's hot loop is that of the dirty image
    assert '#include "dirty_image.h"' in open(os.path.join(ROOT, 'prisim_amd', 'csrc_imaging', 'imaging.hip')).read()
    assert 'enqueue_dirty(' in src and 'k_img_sum<' not in src and 'prisim_imaging_args ia' not in src
    # ... in the one update kernel that this entry and the mosaic's CLEAN launch, which is not restated here
    upd = open(os.path.join(ROOT, 'prisim_amd', 'csrc_imaging', 'clean_update.h')).read()
    assert 'img_tile_pass<STEPPED, false>(' in upd and 'img_rows' not in upd and 'sh_b[tid] =' not in upd and 'atomic' not in upd.replace('No atomics', '')
    assert '#include "clean_update.h"' in src and 'enqueue_clean_update<false>(' in src and 'k_imclean_avg_sub(' in src
    assert 'img_tile_pass' not in src and 'img_rows' not in src and 'sh_b[tid] =' not in src and 'double acc' not in src


def test_plan_header_under_the_sanitizers(tmp_path):
    exe = tmp_path / 'imclean_plan_main'
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-I',
                           os.path.join(ROOT, 'prisim_amd', 'csrc_addon'), os.path.join(ROOT, 'tests', 'imclean_plan_main.cpp'), '-o', str(exe)])
    res = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = res.stdout.decode()
    assert res.returncode == 0, out
    last = out.strip().splitlines()[-1].split()
    assert last[0] == 'checked' and int(last[1]) > 10000 and last[2:] == ['bad', '0'], out
    txt = open(os.path.join(ROOT, 'prisim_amd', 'csrc_addon', 'imclean_plan.h')).read()
    assert '#include <hip' not in txt and '__device__' not in txt and '#include "addon_internal.h"' not in txt


# ---- the checker against itself -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def small():
    """37 baselines, 5 channels, 63 pixels, 3 snapshots, weights per visibility with every seventh baseline at 0."""
    c = IC.case(37, 5, 63, 3)
    pb = CK.Problem(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], c['cube'], weights=c['w_full'], aberr_beta=c['beta'])
    return c, pb


@pytest.mark.parametrize('chan_avg', [False, True])
def test_independent_clean_against_the_replay(small, chan_avg):
    c, pb0 = small
    window = NP.arange(63) % 3 != 1
    pb = CK.Problem(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], c['cube'], weights=c['w_full'], aberr_beta=c['beta'],
                    chan_avg=chan_avg, window=window, E=pb0.E)
    # the dirty image of the problem is the imaging checker's
    want = IK.dirty_image(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], cube=c['cube'], weights=c['w_full'], aberr_beta=c['beta'],
                          chan_avg=chan_avg)
    assert NP.max(NP.abs(pb.dirty(pb.v) - want['image'].reshape(63, -1)) / want['scale']) <= 1e-13 and NP.allclose(pb.scale, want['scale'], rtol=1e-14)
    for gain, maxiter, thr, rel in ((0.3, 25, 0.0, False), (0.1, 40, 0.5, True), (1.0, 3, 0.2, True), (0.5, 0, 0.1, False)):
        r = CK.clean(pb, gain, maxiter, thr, rel)
        worst = CK.replay(pb, r, gain, maxiter, thr, rel)
        print('gain %.1f maxiter %d threshold %.1f: %d components, worst deviation %.2e of its tolerance' % (gain, maxiter, thr, r['ncomp'].sum(), worst))
        assert worst <= 1e-2 and NP.all(window[r['comp_pixel'][r['comp_pixel'] >= 0]])
        assert NP.all(r['ncomp'] <= maxiter) and NP.all((r['status'] == CK.MAXITER) == ((r['ncomp'] == maxiter) & (r['status'] != CK.THRESHOLD)))
        if maxiter == 0:
            assert NP.array_equal(r['residual'].reshape(63, -1), pb.dirty(pb.v)) and r['comp_pixel'].shape == (pb.nc, 0)
    # matching pursuit: sum w |V - model|^2 does not grow from one component to the next, at gain 1 either
    r = CK.clean(pb, 1.0, 12, 0.0, False)
    for k in range(pb.nc):
        vm, last = NP.zeros_like(pb.v), None
        for q, a in zip(r['comp_pixel'][k], r['comp_flux'][k]):
            chan = slice(None) if chan_avg else k
            cost = float(NP.sum(pb.w[:, :, chan] * NP.abs((pb.v - vm)[:, :, chan]) ** 2))
            assert last is None or cost <= last * (1 + 1e-12)
            last = cost
            vm += pb.component_vis(k, int(q), a)


def test_replay_refuses_wrong_decisions(small):
    c, pb = small
    args = (0.3, 25, 0.5, True)
    r = CK.clean(pb, *args)
    assert len(set(r['ncomp'].tolist())) > 1 and NP.any(r['status'] == CK.THRESHOLD)      # the channels end at different places
    CK.replay(pb, r, *args)

    def tampered(**kw):
        out = {k: NP.array(v) for k, v in r.items()}
        for name, (index, value) in kw.items():
            out[name][index] = value
        return out

    k = int(NP.argmax(r['ncomp']))
    second = NP.argsort(NP.abs(pb.dirty(pb.v)[:, k]))[-2]             # the second largest of the first residual
    wrong = [tampered(comp_pixel=((k, 0), second)),                   # a pick that is not the peak
             tampered(comp_flux=((k, 3), r['comp_flux'][k, 3] * (1 + 1e-9))),      # a flux off by 1e-9 of itself
             tampered(comp_flux=((k, 3), -r['comp_flux'][k, 3])),
             tampered(residual=((5, k), r['residual'][5, k] + 1e-9)),  # a residual pixel off by far more than the tolerance
             tampered(status=(k, CK.THRESHOLD if r['status'][k] == CK.MAXITER else CK.MAXITER)),
             tampered(status=(k, CK.DEAD)), tampered(peak0=(k, r['peak0'][k] * (1 + 1e-9)))]
    # a stop one component early: the peak is still above the threshold
    early = tampered(ncomp=(k, r['ncomp'][k] - 1), status=(k, CK.THRESHOLD))
    early['comp_pixel'][k, r['ncomp'][k] - 1], early['comp_flux'][k, r['ncomp'][k] - 1] = -1, 0.0
    if NP.max(NP.delete(r['ncomp'], k)) < r['ncomp'][k]:
        early['comp_pixel'], early['comp_flux'] = early['comp_pixel'][:, :-1], early['comp_flux'][:, :-1]
    wrong.append(early)
    for bad in wrong:
        with pytest.raises(AssertionError):
            CK.replay(pb, bad, *args)
    # a pick outside the window
    win = NP.ones(63, dtype=bool)
    later = [q for q in r['comp_pixel'][k, :r['ncomp'][k]] if q != r['comp_pixel'][k, 0]]
    win[later[0]] = False                                             # not the first peak: P0 stands
    pbw = CK.Problem(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], c['cube'], weights=c['w_full'], aberr_beta=c['beta'],
                     window=win, E=pb.E)
    with pytest.raises(AssertionError, match='window'):
        CK.replay(pbw, r, *args)
    # two pixels that tie to rounding -- the second a copy of the peak's direction, a few units in the last place away: either pick passes
    one = CK.clean(pb, 0.3, 1, 0.0, False)
    q0 = int(one['comp_pixel'][k, 0])
    twin = (q0 + 7) % 63
    u2 = c['unitvec'].copy()
    u2[twin] = IC.unit(u2[q0] + 4e-16 * NP.array([1.0, -1.0, 1.0]))
    assert not NP.array_equal(u2[twin], u2[q0])
    pbt = CK.Problem(u2, c['rot'], c['pc'], c['baselines'], c['freqs'], c['cube'], weights=c['w_full'], aberr_beta=c['beta'])
    R0 = pbt.dirty(pbt.v)
    assert abs(abs(R0[twin, k]) - abs(R0[q0, k])) <= CK.BOUND * pbt.scale[k]
    one = CK.clean(pbt, 0.3, 1, 0.0, False)
    assert one['comp_pixel'][k, 0] in (q0, twin)
    other = twin if one['comp_pixel'][k, 0] == q0 else q0
    alt = {name: NP.array(v) for name, v in one.items()}
    alt['comp_pixel'][k, 0], alt['comp_flux'][k, 0] = other, 0.3 * R0[other, k]
    alt['residual'][:, k] = R0[:, k] - pbt.beams([k], [other], [0.3 * R0[other, k]])[:, 0]
    CK.replay(pbt, one, 0.3, 1, 0.0, False)
    CK.replay(pbt, alt, 0.3, 1, 0.0, False)


def test_linearity_identity(small):
    """The residual is the dirty image of V less the components' visibilities, and a component's beam is the dirty image of its own
    visibilities: 1 times its flux at its own pixel."""
    c, pb = small
    r = CK.clean(pb, 0.2, 30, 0.0, False)
    vm = NP.zeros_like(pb.v)
    for k in range(pb.nc):
        for q, a in zip(r['comp_pixel'][k, :r['ncomp'][k]], r['comp_flux'][k, :r['ncomp'][k]]):
            vm += pb.component_vis(k, int(q), a)
    tol = CK.BOUND * (pb.scale + NP.abs(r['comp_flux']).sum(axis=1))
    assert NP.all(NP.abs(r['residual'] - pb.dirty(pb.v - vm)) <= tol)
    # ... by the imaging checker's own einsum too
    want = IK.dirty_image(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], cube=pb.v - vm, weights=c['w_full'], aberr_beta=c['beta'])
    assert NP.all(NP.abs(r['residual'] - want['image']) <= tol)
    b = pb.beams([2], [17], [1.5])
    assert abs(b[17, 0] - 1.5) <= 1e-14 and NP.all(NP.abs(b[:, 0]) <= 1.5 * (1 + 1e-14))
    assert NP.allclose(b[:, 0], pb.dirty(pb.component_vis(2, 17, 1.5))[:, 2], rtol=0, atol=1e-13)
    # the model of a restored image: the beam is 1 at the component's own pixel
    one = CK.restored(NP.zeros((63, 5)), c['unitvec'], NP.array([[9]] * 5, dtype=NP.int32), NP.full((5, 1), 2.0), NP.ones(5, dtype=NP.int32), NP.full(5, 0.3))
    assert NP.all(one[9] == 2.0) and NP.all(one <= 2.0) and NP.all(one > 0.0)
    far = 2.0 * NP.arcsin(min(1.0, 0.5 * NP.linalg.norm(c['unitvec'][10] - c['unitvec'][9])))
    assert NP.allclose(one[10], 2.0 * NP.exp(-4 * NP.log(2) * far ** 2 / 0.09), rtol=1e-14)


# ---- the class against a stand-in context ---------------------------------------------------------------------------------------------

class CleanOracleContext(TI.ImagingOracleContext):
    """ImagingOracleContext whose clean_image is the numpy checker; it records what it was handed."""
    cleans = []

    def clean_image(self, unitvec, rot, pc_dircos, baselines, freqs_hz, cube=None, weights=None, chan_avg=False, aberr_beta=None, gain=0.1,
                    maxiter=10000, threshold=5e-3, threshold_relative=True, window=None, fwhm_rad=None, route='auto', budget_bytes=0,
                    poll_every=0):
        call = dict(unitvec=NP.array(unitvec), rot=NP.array(rot), pc=NP.array(pc_dircos), baselines=NP.array(baselines), freqs=NP.array(freqs_hz),
                    cube=None if cube is None else NP.array(cube), weights=None if weights is None else NP.array(weights), chan_avg=chan_avg,
                    beta=None if aberr_beta is None else NP.array(aberr_beta), gain=gain, maxiter=maxiter, threshold=threshold,
                    threshold_relative=threshold_relative, window=None if window is None else NP.array(window),
                    fwhm_rad=None if fwhm_rad is None else NP.array(fwhm_rad), route=route, budget_bytes=budget_bytes)
        CleanOracleContext.cleans.append(call)
        nt = call['rot'].reshape(-1, 9).shape[0]
        v = self.cube[:nt] if cube is None else cube
        r = CK.answer(unitvec, rot, pc_dircos, baselines, freqs_hz, v, weights=weights, chan_avg=chan_avg, aberr_beta=aberr_beta, gain=gain,
                      maxiter=maxiter, threshold=threshold, threshold_relative=threshold_relative, window=window, fwhm_rad=fwhm_rad)
        r['stats'] = {'route': 'stepped' if route == 'auto' else route, 'iterations': int(r['ncomp'].max()), 'resident': cube is None}
        return r


def observed(monkeypatch, reserve=False):
    sky = SM.SkyModel(location=[[80.0, 100.0], [50.0, 10.0]], flux_ref=[1.0, 3.0], spindex=[0.0, 0.0], ref_freq=150e6)
    monkeypatch.setattr(TI, 'ImagingOracleContext', CleanOracleContext)
    CleanOracleContext.cleans = []
    return TI.observed(monkeypatch, 'altaz', [[90.0, 270.0]] * 3, reserve=reserve, sky=sky)


def test_clean_argument_checks_and_exception_types(monkeypatch):
    ia = observed(monkeypatch)
    aps = RI.ApertureSynthesis(ia)
    grid = aps.dircos_grid(3, 0.2)
    for kw, exc in ((dict(threshold_type='sigma'), ValueError), (dict(threshold=[0.1]), TypeError), (dict(threshold=0.0), ValueError),
                    (dict(threshold=-1.0), ValueError), (dict(threshold=1.0), ValueError), (dict(gain=1), TypeError), (dict(gain=0.0), TypeError),
                    (dict(gain=1.0), TypeError), (dict(maxiter=10.0), TypeError), (dict(maxiter=0), ValueError), (dict(coords='galactic'), ValueError),
                    (dict(datakey='vis'), ValueError), (dict(datakey='noisy'), ValueError), (dict(weights=NP.ones(3)), ValueError),
                    (dict(route='fast'), ValueError), (dict(window=NP.ones(8)), ValueError), (dict(window=NP.zeros(9)), ValueError),
                    (dict(fwhm=0.0), ValueError), (dict(fwhm=NP.ones(5)), ValueError), (dict(fwhm=NP.inf), ValueError),
                    (dict(fwhm=[1.0, 1.0, 1.0, 1.0, 1.0, -1.0]), ValueError), (dict(fwhm=NP.ones(6), chan_avg=True), ValueError)):
        with pytest.raises(exc):
            aps.clean(grid, **kw)
    assert aps.clean(grid, threshold=1.0, threshold_type='absolute')['status'].shape == (6,)      # an absolute threshold may exceed 1
    assert len(CleanOracleContext.cleans) == 1                        # nothing else reached the device
    empty = RI.InterferometerArray(TI.LABELS, TI.BL, TI.CH, telescope=TI.TELESCOPE, latitude=TI.LAT, skycoords='altaz', pointing_coords='altaz')
    with pytest.raises(ValueError, match='observe'):
        RI.ApertureSynthesis(empty).clean(grid)


def test_clean_marshals_and_returns_the_documented_dict(monkeypatch):
    ia = observed(monkeypatch)
    aps = RI.ApertureSynthesis(ia)
    cleans = CleanOracleContext.cleans
    aa = NP.array([[80.0, 100.0], [50.0, 10.0], [70.0, 200.0], [30.0, 300.0]])
    out = aps.clean(aa, coords='altaz', gain=0.2, maxiter=50, threshold=0.05)
    c = cleans[-1]
    # what image() hands over, by the same code
    aps.image(aa, coords='altaz')
    i = TI.ImagingOracleContext.calls[-1]
    for name in ('unitvec', 'rot', 'pc', 'baselines', 'freqs', 'cube'):
        assert NP.array_equal(c[name], i[name]), name
    assert c['beta'] is None and c['weights'] is None and c['window'] is None and c['chan_avg'] is False and c['route'] == 'auto'
    assert (c['gain'], c['maxiter'], c['threshold'], c['threshold_relative'], c['budget_bytes']) == (0.2, 50, 0.05, True, 0)
    # the default restoring beam: c / (f max|b|) radians per channel
    longest = NP.sqrt((TI.BL ** 2).sum(axis=1)).max()
    assert NP.allclose(c['fwhm_rad'], RI.C_LIGHT / (TI.CH * longest), rtol=1e-15) and NP.allclose(out['fwhm'], NP.degrees(c['fwhm_rad']), rtol=1e-15)
    # the dict: keys, shapes, dtypes
    assert set(out) == {'residual', 'restored', 'model', 'components', 'status', 'peak0', 'threshold', 'fwhm'}
    assert set(out['components']) == {'pixel', 'flux', 'count'}
    for name in ('residual', 'restored', 'model'):
        assert out[name].shape == (4, 6) and out[name].dtype == NP.float64, name
    n = int(out['components']['count'].max())
    assert out['components']['pixel'].shape == out['components']['flux'].shape == (6, n) and 0 < n <= 50
    assert out['components']['pixel'].dtype == NP.int32 and out['components']['flux'].dtype == NP.float64 and out['components']['count'].dtype == NP.int32
    assert out['status'].shape == out['peak0'].shape == out['threshold'].shape == out['fwhm'].shape == (6,) and out['status'].dtype == NP.int32
    assert NP.array_equal(out['threshold'], 0.05 * out['peak0'])
    model = NP.zeros((4, 6))
    for k in range(6):
        m = out['components']['count'][k]
        NP.add.at(model[:, k], out['components']['pixel'][k, :m], out['components']['flux'][k, :m])
    assert NP.array_equal(out['model'], model)
    assert aps.image_stats['route'] == 'stepped' and aps.image_stats['resident'] is False and aps.image_stats['wsum'].shape == (6,)
    # the restored image is the residual and the components through the beam
    assert NP.allclose(out['restored'], CK.restored(out['residual'], c['unitvec'], out['components']['pixel'], out['components']['flux'],
                                                    out['components']['count'], c['fwhm_rad']), rtol=0, atol=1e-14)

    # chan_avg: one image channel, the default beam at the mean frequency; absolute threshold; weights in both forms; a window; no restoration
    full_w = NP.random.default_rng(1).uniform(0.5, 1.0, (4, 6, 3))
    window = NP.array([True, True, False, True])
    out = aps.clean(aa, coords='altaz', weights=full_w, chan_avg=True, threshold=0.5, threshold_type='absolute', window=window, restore=False,
                    route='direct', budget_bytes=1 << 20)
    c = cleans[-1]
    assert c['weights'].shape == (3, 4, 6) and NP.array_equal(c['weights'], NP.transpose(full_w, (2, 0, 1))) and c['chan_avg'] is True
    assert c['threshold_relative'] is False and c['threshold'] == 0.5 and c['fwhm_rad'] is None and c['route'] == 'direct' and c['budget_bytes'] == 1 << 20
    assert NP.array_equal(c['window'], window) and c['window'].dtype == bool
    assert out['residual'].shape == out['model'].shape == (4,) and out['restored'] is None and out['status'].shape == (1,)
    assert NP.array_equal(out['threshold'], [0.5]) and NP.allclose(out['fwhm'], NP.degrees(RI.C_LIGHT / (TI.CH.mean() * longest)), rtol=1e-15)
    assert out['model'][2] == 0.0
    out = aps.clean(aa, coords='altaz', weights=NP.arange(1.0, 5.0), fwhm=2.5)
    assert NP.array_equal(cleans[-1]['weights'], NP.arange(1.0, 5.0)) and NP.allclose(cleans[-1]['fwhm_rad'], NP.radians(2.5)) and out['fwhm'].shape == (6,)
    out = aps.clean(aa, coords='altaz', fwhm=NP.linspace(1.0, 2.0, 6))
    assert NP.allclose(cleans[-1]['fwhm_rad'], NP.radians(NP.linspace(1.0, 2.0, 6))) and NP.allclose(out['fwhm'], NP.linspace(1.0, 2.0, 6))
    # 'radec' directions: the frames of image()
    rd = NP.array([[11.0, -29.0], [14.0, -20.0]])
    ia.frame_model = 'apparent'
    aps.clean(rd, coords='radec', epoch='J2000', maxiter=3)
    aps.image(rd, coords='radec', epoch='J2000')
    c, i = cleans[-1], TI.ImagingOracleContext.calls[-1]
    assert NP.array_equal(c['rot'], i['rot']) and NP.array_equal(c['beta'], i['beta']) and NP.any(c['beta'] != 0.0)


def test_clean_reads_the_resident_cube_where_it_lies(monkeypatch):
    ia = observed(monkeypatch, reserve=True)
    aps = RI.ApertureSynthesis(ia)
    aa = NP.array([[80.0, 100.0], [50.0, 10.0]])
    res = aps.clean(aa, coords='altaz', maxiter=20)
    assert CleanOracleContext.cleans[-1]['cube'] is None and aps.image_stats['resident'] is True
    ia.skyvis_freq = NP.array(ia.skyvis_freq)                         # replaced: the slots are out of step, the cube is handed over
    host = aps.clean(aa, coords='altaz', maxiter=20)
    assert CleanOracleContext.cleans[-1]['cube'] is not None and aps.image_stats['resident'] is False
    assert NP.array_equal(res['residual'], host['residual']) and NP.array_equal(res['model'], host['model'])
