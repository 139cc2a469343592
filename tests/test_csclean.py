"""CPU: Cotton-Schwab CLEAN of dirty images (include/prisim_csclean.h) -- the export (tests/test_abi_headers.py holds the ctypes
mirrors, the constants and the prototype to the header), the planning header under ASan and UBSan in a host program of its own
(tests/csclean_plan_main.cpp), the numpy checker against itself (tests/csclean_checker.py: the independent CLEAN against the replay,
and the replay against wrong decisions), and the class prisim_amd.interferometry.ApertureSynthesis.clean_cotton_schwab against a
stand-in context that answers clean_image_cs with the checker.

Bounds.  The replay's tolerance is the one the device is held to (tests/test_gpu_csclean.py): 1e-11 of the natural scale plus the sum
of |a| so far.  The checker's own CLEAN and its replay evaluate the same numpy expressions, so they agree far inside it; what this file
shows of the replay is that it fails where a decision is wrong by more than the tolerance."""
import os
import subprocess
import sys

import numpy as NP
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import csclean_cases as CC  # noqa: E402
import csclean_checker as CS  # noqa: E402
import imclean_checker as CK  # noqa: E402
import test_imaging as TI  # noqa: E402  (the arrays, the sky and the stand-in context of the imaging tests)

from prisim_amd import _abi  # noqa: E402
from prisim_amd import interferometry as RI  # noqa: E402
from prisim_amd import skymodel as SM  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the library and its headers ----------------------------------------------------------------------------------------------------

def test_export_is_in_the_library_and_outside_the_core_abi():
    lib = _abi.load_library()
    assert _abi.CSCLEAN_EXPORTS == ('prisim_clean_image_cs',) and 'prisim_clean_image_cs' not in _abi.EXPORTS
    assert lib.prisim_clean_image_cs(*[None] * 16) == _abi.PRISIM_EINVAL       # a null context and null args are refused, not read
    assert not hasattr(_abi, 'PrisimCscleanStats')                    # the struct lives on the class (tests/test_abi_helpers.py)
    assert set(_abi._stats_dict(_abi.Context.PrisimCscleanStats())) == {
        'wall_ms', 'kernel_ms', 'psf_ms', 'dirty_ms', 'peak_ms', 'minor_ms', 'model_ms', 'restore_ms', 'terms', 'cycles', 'components', 'polls',
        'psf_offsets', 'upload_bytes', 'download_bytes', 'device_bytes', 'route', 'minor_route', 'streams', 'chan_tile', 'reseed', 'lds_bytes',
        'minor_lds_bytes', 'block_pixels'}
    assert (_abi.PRISIM_CSCLEAN_MAJOR, _abi.PRISIM_CSCLEAN_DIVERGED) == (CS.MAJOR, CS.DIVERGED) == (8, 16)
    assert (_abi.PRISIM_CSCLEAN_AUTO, _abi.PRISIM_CSCLEAN_LDS, _abi.PRISIM_CSCLEAN_GLOBAL) == (-1, 0, 1)
    # the fields of prisim_imclean_args come first and in its order, so the helpers that fill the one fill the other
    mine, base = _abi.Context.PrisimCscleanArgs._fields_, _abi.Context.PrisimImcleanArgs._fields_
    assert mine[:len(base) - 2] == base[:-2] and [f for f, _ in mine[len(base) - 2:]] == ['ny', 'nx', 'cycle_depth', 'cycle_niter', 'max_major', 'minor_route']
    src = open(os.path.join(ROOT, 'prisim_amd', 'csrc_imaging', 'csclean.hip')).read()
    # the dirty images and the beam are those of prisim_dirty_image, called and not restated; the restoration and the peak search are shared
    assert '#include "dirty_image.h"' in src and '#include "clean_kernels.h"' in src and 'k_img_sum<' not in src and 'img_tile_pass' not in src
    assert src.count('enqueue_dirty(') == 2 and src.count('enqueue_dirty_sums(') == 1 and '.search(' in src and '.close(' in src
    # ... through the frame of clean_kernels.h: their launches are written there alone, and the decision kernel calls the pieces of its own
    folder = os.path.join(ROOT, 'prisim_amd', 'csrc_imaging')
    for name in ('k_imclean_peak1', 'k_imclean_restore', 'k_imclean_init'):
        assert [f for f in sorted(os.listdir(folder)) if 'launch(ctx, ' + name in open(os.path.join(folder, f)).read()] == ['clean_kernels.h'], name
        assert 'hipLaunchKernelGGL(' + name not in src
    shared = open(os.path.join(folder, 'clean_kernels.h')).read()
    for name in ('Peak best_partial(', 'void set_first_peak(', 'void publish_active('):
        assert shared.count('__device__ __forceinline__ ' + name) == 1 and src.count(name.split()[1]) == 1 and shared.count(name.split()[1]) == 2, name
    assert 'sh_n' not in src and 'S.counts[0] =' not in src and 'partial[s * nc + k]' not in src and 'DirtyResidual ' in src
    # a minor cycle waits for nobody: no flags, no spinning
    assert 'while' not in src and 'volatile' not in src


def test_plan_header_under_the_sanitizers(tmp_path):
    exe = tmp_path / 'csclean_plan_main'
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-I',
                           os.path.join(ROOT, 'prisim_amd', 'csrc_addon'), os.path.join(ROOT, 'tests', 'csclean_plan_main.cpp'), '-o', str(exe)])
    res = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = res.stdout.decode()
    assert res.returncode == 0, out
    last = out.strip().splitlines()[-1].split()
    assert last[0] == 'checked' and int(last[1]) > 10000 and last[2:] == ['bad', '0'], out
    txt = open(os.path.join(ROOT, 'prisim_amd', 'csrc_addon', 'csclean_plan.h')).read()
    assert '#include <hip' not in txt and '__device__' not in txt and '#include "addon_internal.h"' not in txt


# ---- the checker against itself -------------------------------------------------------------------------------------------------------

NY, NX = 9, 7
# (gain, maxiter, threshold, relative, cycle_depth, cycle_niter, max_major)
SETTINGS = ((0.3, 25, 0.0, False, 0.5, 4, 10), (0.3, 25, 0.0, False, 0.8, 0, 4), (0.1, 40, 0.5, True, 0.3, 0, 6), (1.0, 3, 0.2, True, 0.5, 2, 3),
            (0.5, 0, 0.1, False, 0.3, 0, 0))


@pytest.fixture(scope='module')
def small():
    """37 baselines, 5 channels, 9 x 7 pixels, 3 snapshots, weights per visibility with every seventh baseline at 0."""
    c = CC.case(37, 5, NY, NX, 3)
    pb = CK.Problem(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], c['cube'], weights=c['w_full'], aberr_beta=c['beta'])
    return c, pb


def beam_of(c, pb):
    return CS.beam(pb, c['unitvec'], c['rot'], c['baselines'], c['freqs'], c['ny'], c['nx'])


def test_the_beam_is_even_and_one_at_the_centre_and_exact_for_a_flat_array():
    c = CC.case(37, 5, NY, NX, 1)
    pb = CK.Problem(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], c['cube'], weights=c['w_bl'], aberr_beta=c['beta'])
    P = beam_of(c, pb)
    assert P.shape == (5, 2 * NY - 1, 2 * NX - 1) and NP.array_equal(P, P[:, ::-1, ::-1])
    assert NP.allclose(P[:, NY - 1, NX - 1], 1.0, rtol=0, atol=1e-14) and NP.all(NP.abs(P) <= 1.0 + 1e-14)
    rho, kappa = CS.lattice_steps(c['unitvec'], NY, NX)
    assert NP.allclose(rho[:2], [0.0, 0.4 / (NY - 1)], atol=1e-16) and NP.allclose(kappa[:2], [0.3 / (NX - 1), 0.0], atol=1e-16)
    # baselines in the plane of the lattice's (l, m), no rotation, no aberration: the phase depends on the offset alone and P is the exact beam
    bl = c['baselines'].copy()
    bl[:, 2] = 0.0
    flat = CK.Problem(c['unitvec'], NP.eye(3)[None], c['pc'], bl, c['freqs'], c['cube'], weights=c['w_bl'])
    Pf = CS.beam(flat, c['unitvec'], NP.eye(3)[None], bl, c['freqs'], NY, NX)
    for q in (0, 17, 62):
        exact = flat.beams(NP.arange(5), [q] * 5, NP.ones(5))
        got = NP.stack([CS.shifted(Pf[k], q, NY, NX) for k in range(5)], axis=1)
        assert NP.max(NP.abs(exact - got)) <= 1e-13
    # ... and not with the w-term: there the minor cycle's beam is an approximation, which the major cycles make good
    exact = pb.beams(NP.arange(5), [17] * 5, NP.ones(5))
    got = NP.stack([CS.shifted(P[k], 17, NY, NX) for k in range(5)], axis=1)
    assert 1e-3 < NP.max(NP.abs(exact - got)) < 0.5


@pytest.mark.parametrize('chan_avg', [False, True])
def test_independent_clean_against_the_replay(small, chan_avg):
    c, pb0 = small
    window = NP.arange(NY * NX) % 3 != 1
    pb = CK.Problem(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], c['cube'], weights=c['w_full'], aberr_beta=c['beta'],
                    chan_avg=chan_avg, window=window, E=pb0.E)
    P = beam_of(c, pb)
    assert P.shape == (pb.nc, 2 * NY - 1, 2 * NX - 1)
    seen = set()
    for args in SETTINGS:
        gain, maxiter, thr, rel, depth, niter, major = args
        r = CS.clean(pb, P, NY, NX, *args)
        worst = CS.replay(pb, P, NY, NX, r, *args)
        seen |= set(r['status'].tolist())
        print('%s: %d components in %d cycles, statuses %s, worst deviation %.2e of its tolerance'
              % (args, r['ncomp'].sum(), r['ncycles'].max(), sorted(set(r['status'].tolist())), worst))
        assert worst <= 1e-2 and NP.all(window[r['comp_pixel'][r['comp_pixel'] >= 0]])
        assert NP.all(r['ncomp'] <= maxiter) and NP.all(r['ncycles'] <= major) and NP.all((r['status'] == CS.MAXITER) <= (r['ncomp'] == maxiter))
        for k in range(pb.nc):
            n = r['ncycles'][k]
            held = NP.concatenate(([0], r['cycle_ncomp'][k, :n]))
            assert NP.all(NP.diff(held) >= 1) and held[-1] == r['ncomp'][k]      # a cycle that starts adds a component
            assert niter == 0 or NP.all(NP.diff(held) <= niter)
            assert NP.all(NP.isfinite(r['cycle_peak'][k, :n + 1])) and NP.all(NP.isnan(r['cycle_peak'][k, n + 1:]))
            if r['status'][k] == CS.DIVERGED:
                assert r['cycle_peak'][k, n] > r['cycle_peak'][k, n - 1]
            elif n > 1:
                assert NP.all(NP.diff(r['cycle_peak'][k, :n]) <= 0.0)
        if maxiter == 0:
            assert NP.array_equal(r['residual'].reshape(NY * NX, -1), pb.dirty(pb.v)) and r['comp_pixel'].shape == (pb.nc, 0)
            assert NP.all(r['status'] == CS.MAXITER) and NP.all(r['ncycles'] == 0) and NP.array_equal(r['vres'], pb.v)
    assert {CS.THRESHOLD, CS.MAXITER, CS.MAJOR} <= seen


def test_replay_refuses_wrong_decisions(small):
    c, pb = small
    P = beam_of(c, pb)
    args = (0.3, 40, 0.7, True, 0.85, 4, 12)
    r = CS.clean(pb, P, NY, NX, *args)
    assert NP.all(r['status'] == CS.THRESHOLD) and len(set(r['ncycles'].tolist())) > 2     # the channels end at different places
    CS.replay(pb, P, NY, NX, r, *args)

    def tampered(**kw):
        out = {k: NP.array(v) for k, v in r.items()}
        for name, (index, value) in kw.items():
            out[name][index] = value
        return out

    k = int(NP.argsort(r['ncycles'], kind='stable')[-2])             # not the longest: the shapes of the tables stand when it is cut short
    n, last = int(r['ncycles'][k]), int(r['ncomp'][k])
    assert 3 <= n < r['ncycles'].max() and last < r['ncomp'].max()
    second = NP.argsort(NP.abs(pb.dirty(pb.v)[:, k]))[-2]             # the second largest of the first residual
    wrong = [tampered(comp_pixel=((k, 0), second)),                   # a pick that is not the peak
             tampered(comp_flux=((k, 1), r['comp_flux'][k, 1] * (1 + 1e-9))),      # a flux off by 1e-9 of itself
             tampered(comp_flux=((k, 1), -r['comp_flux'][k, 1])),
             tampered(residual=((5, k), r['residual'][5, k] + 1e-9)),
             tampered(vres=((1, 3, k), r['vres'][1, 3, k] + 1e-8)),
             tampered(status=(k, CS.MAXITER if r['status'][k] != CS.MAXITER else CS.THRESHOLD)),    # a wrong status
             tampered(status=(k, CS.MAJOR)), tampered(status=(k, CS.DIVERGED)), tampered(status=(k, CS.DEAD)),
             tampered(peak0=(k, r['peak0'][k] * (1 + 1e-9))), tampered(cycle_peak=((k, 1), r['cycle_peak'][k, 1] * (1 + 1e-9))),
             tampered(ncycles=(k, n - 1)),                            # a wrong cycle count: components beyond the last cycle
             tampered(ncycles=(k, n + 1))]                            # ... and a cycle without a record
    # a minor cycle ended early: its last component moved to the cycle after it, while the working peak was still above the limit
    cyc = next(j for j in range(n - 1) if r['cycle_ncomp'][k, j] - (r['cycle_ncomp'][k, j - 1] if j else 0) in (2, 3))
    wrong.append(tampered(cycle_ncomp=((k, cyc), r['cycle_ncomp'][k, cyc] - 1)))
    # a channel stopped one cycle early at the threshold: its peak is still above it
    early = tampered(ncycles=(k, n - 1), status=(k, CS.THRESHOLD), ncomp=(k, r['cycle_ncomp'][k, n - 2]))
    early['comp_pixel'][k, r['cycle_ncomp'][k, n - 2]:], early['comp_flux'][k, r['cycle_ncomp'][k, n - 2]:] = -1, 0.0
    assert last > r['cycle_ncomp'][k, n - 2]
    wrong.append(early)
    for i, bad in enumerate(wrong):
        with pytest.raises(AssertionError):
            CS.replay(pb, P, NY, NX, bad, *args)
            print('wrong decision %d passed' % i)
    # a pick outside the window
    win = NP.ones(NY * NX, dtype=bool)
    later = [q for q in r['comp_pixel'][k, :last] if q != r['comp_pixel'][k, 0]]
    win[later[0]] = False
    pbw = CK.Problem(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], c['cube'], weights=c['w_full'], aberr_beta=c['beta'], window=win, E=pb.E)
    with pytest.raises(AssertionError, match='window|peak'):
        CS.replay(pbw, P, NY, NX, r, *args)
    # two pixels that tie to rounding -- the second a copy of the peak's direction, a few units in the last place away: either pick passes
    one_args = (0.3, 1, 0.0, False, 0.5, 0, 4)
    one = CS.clean(pb, P, NY, NX, *one_args)
    q0 = int(one['comp_pixel'][k, 0])
    twin = (q0 + 7) % (NY * NX)
    u2 = c['unitvec'].copy()
    u2[twin] = CC.IC.unit(u2[q0] + 4e-16 * NP.array([1.0, -1.0, 1.0]))
    assert not NP.array_equal(u2[twin], u2[q0])
    pbt = CK.Problem(u2, c['rot'], c['pc'], c['baselines'], c['freqs'], c['cube'], weights=c['w_full'], aberr_beta=c['beta'])
    R0 = pbt.dirty(pbt.v)
    assert abs(abs(R0[twin, k]) - abs(R0[q0, k])) <= CK.BOUND * pbt.scale[k]
    one = CS.clean(pbt, P, NY, NX, *one_args)
    assert one['comp_pixel'][k, 0] in (q0, twin) and one['status'][k] == CS.MAXITER and one['ncycles'][k] == 1
    other = twin if one['comp_pixel'][k, 0] == q0 else q0
    alt = {name: NP.array(v) for name, v in one.items()}
    alt['comp_pixel'][k, 0], alt['comp_flux'][k, 0] = other, 0.3 * R0[other, k]
    vm = pbt.component_vis(k, other, 0.3 * R0[other, k])
    alt['vres'][:, :, k] = (pbt.v - vm)[:, :, k]
    alt['residual'][:, k] = pbt.dirty(pbt.v - vm)[:, k]
    alt['cycle_peak'][k, 1] = NP.abs(alt['residual'][:, k]).max()
    CS.replay(pbt, P, NY, NX, one, *one_args)
    CS.replay(pbt, P, NY, NX, alt, *one_args)


# ---- the class against a stand-in context ---------------------------------------------------------------------------------------------

class CycleOracleContext(TI.ImagingOracleContext):
    """ImagingOracleContext whose clean_image_cs is the numpy checker; it records what it was handed."""
    cleans = []

    def clean_image_cs(self, unitvec, grid_shape, rot, pc_dircos, baselines, freqs_hz, cube=None, weights=None, chan_avg=False, aberr_beta=None,
                       gain=0.1, maxiter=10000, threshold=5e-3, threshold_relative=True, cycle_depth=0.3, cycle_niter=0, max_major=32,
                       window=None, fwhm_rad=None, route='auto', minor_route='auto', budget_bytes=0, want_psf=False, want_vis=False):
        call = dict(unitvec=NP.array(unitvec), grid_shape=grid_shape, rot=NP.array(rot), pc=NP.array(pc_dircos), baselines=NP.array(baselines),
                    freqs=NP.array(freqs_hz), cube=None if cube is None else NP.array(cube), weights=None if weights is None else NP.array(weights),
                    chan_avg=chan_avg, beta=None if aberr_beta is None else NP.array(aberr_beta), gain=gain, maxiter=maxiter, threshold=threshold,
                    threshold_relative=threshold_relative, cycle_depth=cycle_depth, cycle_niter=cycle_niter, max_major=max_major,
                    window=None if window is None else NP.array(window), fwhm_rad=None if fwhm_rad is None else NP.array(fwhm_rad), route=route,
                    minor_route=minor_route, budget_bytes=budget_bytes, want_vis=want_vis)
        CycleOracleContext.cleans.append(call)
        nt = call['rot'].reshape(-1, 9).shape[0]
        v = self.cube[:nt] if cube is None else cube
        ny, nx = grid_shape
        pb = CK.Problem(unitvec, rot, pc_dircos, baselines, freqs_hz, v, weights=weights, aberr_beta=aberr_beta, chan_avg=chan_avg, window=window)
        P = CS.beam(pb, unitvec, rot, baselines, freqs_hz, ny, nx)
        r = CS.clean(pb, P, ny, nx, gain, maxiter, threshold, threshold_relative, cycle_depth, cycle_niter, max_major)
        r['wsum'], r['psf'], r['restored'] = pb.W.copy(), None, None
        if fwhm_rad is not None:
            r['restored'] = CK.restored(r['residual'], unitvec, r['comp_pixel'], r['comp_flux'], r['ncomp'], NP.broadcast_to(fwhm_rad, (pb.nc,)))
        if not want_vis:
            r['vres'] = None
        r['stats'] = {'route': 'stepped' if route == 'auto' else route, 'minor_route': 'lds' if minor_route == 'auto' else minor_route,
                      'cycles': int(r['ncycles'].max()), 'resident': cube is None}
        return r


def observed(monkeypatch, reserve=False):
    sky = SM.SkyModel(location=[[80.0, 100.0], [50.0, 10.0]], flux_ref=[1.0, 3.0], spindex=[0.0, 0.0], ref_freq=150e6)
    monkeypatch.setattr(TI, 'ImagingOracleContext', CycleOracleContext)
    CycleOracleContext.cleans = []
    return TI.observed(monkeypatch, 'altaz', [[90.0, 270.0]] * 3, reserve=reserve, sky=sky)


def test_argument_checks_and_exception_types(monkeypatch):
    ia = observed(monkeypatch)
    aps = RI.ApertureSynthesis(ia)
    grid = aps.dircos_grid(3, 0.2)
    for kw, exc in ((dict(threshold_type='sigma'), ValueError), (dict(threshold=[0.1]), TypeError), (dict(threshold=0.0), ValueError),
                    (dict(threshold=1.0), ValueError), (dict(gain=1), TypeError), (dict(gain=1.0), TypeError), (dict(maxiter=10.0), TypeError),
                    (dict(maxiter=0), ValueError), (dict(coords='galactic'), ValueError), (dict(datakey='vis'), ValueError),
                    (dict(weights=NP.ones(3)), ValueError), (dict(route='fast'), ValueError), (dict(window=NP.ones(8)), ValueError),
                    (dict(window=NP.zeros(9)), ValueError), (dict(fwhm=0.0), ValueError), (dict(fwhm=NP.ones(5)), ValueError),
                    (dict(cycle_depth=0.0), ValueError), (dict(cycle_depth=1.0), ValueError), (dict(cycle_depth=1), ValueError),
                    (dict(cycle_depth=NP.nan), ValueError), (dict(cycle_niter=0), ValueError), (dict(cycle_niter=2.0), ValueError),
                    (dict(max_major=-1), ValueError), (dict(max_major=1.0), ValueError), (dict(max_major=65537), ValueError),
                    (dict(minor_route='fast'), ValueError)):
        with pytest.raises(exc):
            aps.clean_cotton_schwab(grid, (3, 3), **kw)
    for shape in ((3, 2), (9,), 9, (0, 9), (3, 3, 1), None):
        with pytest.raises(ValueError, match='grid_shape'):
            aps.clean_cotton_schwab(grid, shape)
    assert len(CycleOracleContext.cleans) == 0                        # nothing reached the device
    assert aps.clean_cotton_schwab(grid, (1, 9), threshold=1.0, threshold_type='absolute')['status'].shape == (6,)
    empty = RI.InterferometerArray(TI.LABELS, TI.BL, TI.CH, telescope=TI.TELESCOPE, latitude=TI.LAT, skycoords='altaz', pointing_coords='altaz')
    with pytest.raises(ValueError, match='observe'):
        RI.ApertureSynthesis(empty).clean_cotton_schwab(grid, (3, 3))


def test_marshals_and_returns_the_documented_dict(monkeypatch):
    ia = observed(monkeypatch)
    aps = RI.ApertureSynthesis(ia)
    cleans = CycleOracleContext.cleans
    grid = aps.dircos_grid(4, 0.3)[:12]                               # 3 rows of 4
    out = aps.clean_cotton_schwab(grid, (3, 4), gain=0.2, maxiter=50, threshold=0.05)
    c, stats = cleans[-1], aps.image_stats
    # what image() hands over, by the same code
    aps.image(grid)
    i = TI.ImagingOracleContext.calls[-1]
    for name in ('unitvec', 'rot', 'pc', 'baselines', 'freqs', 'cube'):
        assert NP.array_equal(c[name], i[name]), name
    assert c['grid_shape'] == (3, 4) and c['beta'] is None and c['weights'] is None and c['window'] is None and c['chan_avg'] is False
    assert (c['gain'], c['maxiter'], c['threshold'], c['threshold_relative'], c['budget_bytes']) == (0.2, 50, 0.05, True, 0)
    assert (c['cycle_depth'], c['cycle_niter'], c['max_major'], c['route'], c['minor_route'], c['want_vis']) == (0.3, 0, 32, 'auto', 'auto', False)
    longest = NP.sqrt((TI.BL ** 2).sum(axis=1)).max()
    assert NP.allclose(c['fwhm_rad'], RI.C_LIGHT / (TI.CH * longest), rtol=1e-15) and NP.allclose(out['fwhm'], NP.degrees(c['fwhm_rad']), rtol=1e-15)
    # the dict: clean()'s keys and the two new ones; shapes, dtypes
    assert set(out) == {'residual', 'restored', 'model', 'components', 'status', 'peak0', 'threshold', 'fwhm', 'cycles', 'residual_vis'}
    assert set(out['components']) == {'pixel', 'flux', 'count'} and set(out['cycles']) == {'count', 'ncomp', 'peak'} and out['residual_vis'] is None
    for name in ('residual', 'restored', 'model'):
        assert out[name].shape == (12, 6) and out[name].dtype == NP.float64, name
    n, m = int(out['components']['count'].max()), int(out['cycles']['count'].max())
    assert out['components']['pixel'].shape == out['components']['flux'].shape == (6, n) and 0 < n <= 50 and 0 < m <= 32
    assert out['cycles']['count'].shape == (6,) and out['cycles']['ncomp'].shape == (6, m) and out['cycles']['peak'].shape == (6, m + 1)
    assert out['cycles']['count'].dtype == out['cycles']['ncomp'].dtype == NP.int32 and out['cycles']['peak'].dtype == NP.float64
    assert out['status'].shape == out['peak0'].shape == out['threshold'].shape == out['fwhm'].shape == (6,) and out['status'].dtype == NP.int32
    assert NP.array_equal(out['threshold'], 0.05 * out['peak0']) and NP.array_equal(out['cycles']['peak'][:, 0], out['peak0'])
    model = NP.zeros((12, 6))
    for k in range(6):
        cnt = out['components']['count'][k]
        NP.add.at(model[:, k], out['components']['pixel'][k, :cnt], out['components']['flux'][k, :cnt])
        assert out['cycles']['ncomp'][k, out['cycles']['count'][k] - 1] == cnt
    assert NP.array_equal(out['model'], model)
    assert stats['route'] == 'stepped' and stats['minor_route'] == 'lds' and stats['resident'] is False and stats['wsum'].shape == (6,)
    # chan_avg, an absolute threshold, weights, a window, the cycle settings, no restoration, the residual visibilities
    full_w = NP.random.default_rng(1).uniform(0.5, 1.0, (4, 6, 3))
    window = NP.arange(12) != 5
    out = aps.clean_cotton_schwab(grid, (3, 4), weights=full_w, chan_avg=True, threshold=0.5, threshold_type='absolute', window=window, restore=False,
                                  cycle_depth=0.5, cycle_niter=3, max_major=7, return_vis=True, route='direct', minor_route='global', budget_bytes=1 << 20)
    c = cleans[-1]
    assert c['weights'].shape == (3, 4, 6) and NP.array_equal(c['weights'], NP.transpose(full_w, (2, 0, 1))) and c['chan_avg'] is True
    assert c['threshold_relative'] is False and c['threshold'] == 0.5 and c['fwhm_rad'] is None and c['route'] == 'direct' and c['budget_bytes'] == 1 << 20
    assert (c['cycle_depth'], c['cycle_niter'], c['max_major'], c['minor_route'], c['want_vis']) == (0.5, 3, 7, 'global', True)
    assert NP.array_equal(c['window'], window) and c['window'].dtype == bool
    assert out['residual'].shape == out['model'].shape == (12,) and out['restored'] is None and out['status'].shape == (1,) and out['model'][5] == 0.0
    assert out['residual_vis'].shape == (4, 6, 3) and out['residual_vis'].dtype == NP.complex128 and out['residual_vis'].flags['C_CONTIGUOUS']
    # the residual is the image of the residual visibilities
    ia.skyvis_freq, keep = out['residual_vis'], ia.skyvis_freq
    assert NP.allclose(aps.image(grid, weights=full_w, chan_avg=True), out['residual'], rtol=0, atol=1e-12)
    ia.skyvis_freq = keep


def test_reads_the_resident_cube_where_it_lies(monkeypatch):
    ia = observed(monkeypatch, reserve=True)
    aps = RI.ApertureSynthesis(ia)
    grid = aps.dircos_grid(3, 0.2)
    res = aps.clean_cotton_schwab(grid, (3, 3), maxiter=20)
    assert CycleOracleContext.cleans[-1]['cube'] is None and aps.image_stats['resident'] is True
    ia.skyvis_freq = NP.array(ia.skyvis_freq)                         # replaced: the slots are out of step, the cube is handed over
    host = aps.clean_cotton_schwab(grid, (3, 3), maxiter=20)
    assert CycleOracleContext.cleans[-1]['cube'] is not None and aps.image_stats['resident'] is False
    assert NP.array_equal(res['residual'], host['residual']) and NP.array_equal(res['model'], host['model'])
