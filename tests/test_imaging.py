"""CPU: dirty images and synthesized beams by the direct Fourier sum (include/prisim_imaging.h) -- the export (tests/test_abi_headers.py holds
the ctypes mirrors, the constants and the prototype to the header), the planning header compiled alone, the class
prisim_amd.interferometry.ApertureSynthesis against a stand-in context that answers dirty_image with the numpy checker
(tests/imaging_checker.py), and the checker itself against its own arithmetic in longdouble, a stepped phasor and two closed forms.

What the longdouble comparison covers.  It evaluates the phases and the sums of the checker in longdouble, from directions
normalise(R (u + beta)) that BOTH arms form in float64, on baselines to 300 m (250 cycles): it holds the checker's phase and sum
arithmetic at that length and nothing else.  It is not independent of the directions, whose rounding acts on the whole baseline in
wavelengths, and it says nothing beyond 300 m: tests/imaging_reference.py is the independent reference (directions at 60 digits,
phases reduced exactly), and tests/test_imaging_reference.py measures this checker against it per decade -- inside 1e-11 of the scale
up to 30 km, outside from 300 km on.

Bounds of the checker's self-tests.  A term of the sum carries the rounding of its phase: up to 1.3e3 rad here, formed by a handful
of fp64 operations of 1.1e-16 each, so at most some 1e-12 of the term and far less of the sum, where the roundings average out.
1e-12 of the natural scale sum w|V| / sum w is therefore asserted throughout (a tenth of the 1e-11 the device is held to); the
figures measured are printed."""
import os
import subprocess
import sys
import warnings

import numpy as NP
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fake_context  # noqa: E402
import imaging_cases as IC  # noqa: E402
import imaging_checker as IK  # noqa: E402

from prisim_amd import _abi  # noqa: E402
from prisim_amd import frames as FRAMES  # noqa: E402
from prisim_amd import geometry as GEOM  # noqa: E402
from prisim_amd import interferometry as RI  # noqa: E402
from prisim_amd import skymodel as SM  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECKER_BOUND = 1e-12


# ---- the library and its headers ----------------------------------------------------------------------------------------------------

def test_export_is_in_the_library_and_outside_the_core_abi():
    lib = _abi.load_library()
    assert 'prisim_dirty_image' not in _abi.EXPORTS
    assert lib.prisim_dirty_image(None, None, None, None, None) == _abi.PRISIM_EINVAL      # a null context and null args are refused, not read
    assert not hasattr(_abi, 'PrisimImagingStats')                    # the struct lives on the class (tests/test_abi_helpers.py)
    assert set(_abi._stats_dict(_abi.Context.PrisimImagingStats())) == {
        'wall_ms', 'kernel_ms', 'terms', 'chunks', 'chunk_pixels', 'kernel_bytes', 'upload_bytes', 'download_bytes', 'route', 'streams',
        'chan_tile', 'reseed', 'lds_bytes', 'block_pixels'}
    folder = os.path.join(ROOT, 'prisim_amd', 'csrc_imaging')
    srcs = {name: open(os.path.join(folder, name)).read() for name in os.listdir(folder)}
    assert all('atomic' not in txt.lower().replace('no atomics', '') for txt in srcs.values())
    # the hot loop of the three entries is stated once: the two barriers of the staging loop are in one file, which the others call
    assert [name for name, txt in srcs.items() if '__syncthreads();' in txt and 'sh_b[tid] =' in txt] == ['imaging_kernels.h']
    assert srcs['imaging_kernels.h'].count('__syncthreads();') == 2 and srcs['dirty_image.h'].count('img_tile_pass<STEPPED, PSF>(') == 1
    # ... and it has three callers, each with one set of accumulators: the dirty image, the mosaic's sum and the one update of the CLEANs
    assert sorted(name for name, txt in srcs.items() if 'double acc[CT];' in txt) == ['clean_update.h', 'dirty_image.h', 'mosaic_kernels.h']
    assert all(srcs[name].count('double acc[CT];') == 1 and srcs[name].count('img_tile_pass<STEPPED, ') == 1
               for name in ('clean_update.h', 'dirty_image.h', 'mosaic_kernels.h'))
    assert '#include "dirty_image.h"' in srcs['imaging.hip'] and 'enqueue_dirty(' in srcs['imaging.hip'] and '<<<' not in srcs['imaging.hip']
    header = open(os.path.join(ROOT, 'include', 'prisim_imaging.h')).read()
    for name in ('prisim_hip.h', 'prisim_hip_last_error', 'prisim_hip_set_array'):
        header = header.replace(name, '')
    assert 'prisim_hip_' not in header
    assert (_abi.PRISIM_IMAGE_DIRTY, _abi.PRISIM_IMAGE_PSF) == (0, 1)
    assert (_abi.PRISIM_IMAGE_AUTO, _abi.PRISIM_IMAGE_DIRECT, _abi.PRISIM_IMAGE_STEPPED) == (-1, 0, 1)
    assert (_abi.PRISIM_IMAGE_W_NONE, _abi.PRISIM_IMAGE_W_BASELINE, _abi.PRISIM_IMAGE_W_FULL) == (0, 1, 2)


PLAN_PROGRAM = r'''
#include "imaging_plan.h"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace pint;

int main() {
  long bad = 0, checked = 0;
  const int64_t K = kImagingReseed, lds950 = 160 * 1024;
  const int64_t pixs[] = {1, 63, 65, 1000, int64_t(1) << 20};
  const int64_t chans[] = {1, 5, K, K + 1, 1024};
  const int64_t snaps[] = {1, 3};
  for (int64_t npix : pixs)
    for (int64_t nchan : chans)
      for (int64_t nt : snaps)
        for (int form = 0; form < 3; ++form)
          for (int avg = 0; avg < 2; ++avg) {
            const int64_t per = imaging_pixel_bytes(nchan, nt, avg != 0), one = kImagingBlock * per;
            const int64_t budgets[] = {0, one, one + 1, 2 * one - 1, 2 * one, 3 * one + 12345, int64_t(1) << 24, int64_t(1) << 30};
            for (int64_t budget : budgets)
              for (int asked = -1; asked <= 1; ++asked)
                for (int uniform = 0; uniform < 2; ++uniform) {
                  const ImagingPlan p = imaging_plan(npix, 300, nchan, nt, form, avg != 0, budget, lds950, asked, uniform != 0, 2);
                  const int64_t have = budget_or_default(budget);
                  bool ok = true;
                  ++checked;
                  if (asked == kImagingStepped && !uniform) {          // an explicit STEPPED on a non-uniform grid is refused
                    if (!p.refusal || !std::strstr(p.refusal, "uniform")) { std::printf("stepped on a non-uniform grid accepted\n"); ++bad; }
                    continue;
                  }
                  ok = p.refusal == nullptr;
                  // AUTO is STEPPED exactly when the grid is uniform; an explicit route is itself
                  ok = ok && p.route == (asked >= 0 ? asked : uniform ? kImagingStepped : kImagingDirect);
                  ok = ok && p.reseed == (p.route == kImagingStepped ? K : 1);
                  // tile, block and LDS do not change with the budget
                  ok = ok && p.tile == kImagingTile && p.ntiles * p.tile >= nchan && (p.ntiles - 1) * p.tile < nchan && p.block == kImagingBlock &&
                       p.nblocks * p.block >= npix && (p.nblocks - 1) * p.block < npix && p.lds == kImagingLds && p.lds <= lds950 &&
                       p.pixel_bytes == per;
                  const Chunks& c = p.chunks;
                  // whole blocks per chunk, within the budget with every stream's buffers, no larger grid than allowed
                  ok = ok && c.size >= p.block && c.size % p.block == 0 && c.nstreams >= 1 && c.nstreams <= 2 && c.nstreams <= c.count &&
                       p.buffer_bytes == c.nstreams * c.size * per && p.buffer_bytes <= have && c.size / p.block <= kImagingMaxGrid;
                  // the chunks cover [0, npix) once and in order
                  int64_t next = 0;
                  for (int64_t k = 0; ok && k < c.count; ++k) {
                    const Span sp = c.span(k, npix);
                    ok = sp.first == next && sp.count >= 1 && (k == c.count - 1 || sp.count == c.size) && sp.first + sp.count <= npix;
                    next = sp.first + sp.count;
                  }
                  ok = ok && next == npix;
                  // the largest such chunk: one block more is past the pixels, the grid or the budget of as many streams
                  if (ok && c.size < p.nblocks * p.block && c.size / p.block < kImagingMaxGrid && c.count > 1)
                    ok = c.nstreams * (c.size + p.block) * per > have || c.nstreams == 1;
                  if (!ok) {
                    std::printf("plan(%lld, %lld, %lld, form %d, avg %d, budget %lld, asked %d, uniform %d): %s size %lld count %lld streams %d\n",
                                (long long)npix, (long long)nchan, (long long)nt, form, avg, (long long)budget, asked, uniform,
                                p.refusal ? p.refusal : "-", (long long)c.size, (long long)c.count, c.nstreams);
                    ++bad;
                  }
                }
            // one byte short of one block, and an LDS limit one byte short, are refused
            if (!imaging_plan(npix, 300, nchan, nt, form, avg != 0, one - 1, lds950, -1, true, 2).refusal) ++bad;
            if (!imaging_plan(npix, 300, nchan, nt, form, avg != 0, 0, kImagingLds - 1, -1, true, 2).refusal) ++bad;
            if (imaging_plan(npix, 300, nchan, nt, form, avg != 0, 0, kImagingLds, -1, true, 2).refusal) ++bad;
            checked += 3;
          }
  if (!imaging_plan(10, 10, 10, 1, 3, false, 0, lds950, -1, true, 2).refusal || !imaging_plan(10, 10, 10, 1, 0, false, 0, lds950, 2, true, 2).refusal ||
      !imaging_plan(0, 10, 10, 1, 0, false, 0, lds950, -1, true, 2).refusal)
    ++bad;
  // the uniform-grid rule: 1e-7 Hz about the line through the first and the last channel
  double df = 0.0;
  std::vector<double> f(64);
  for (int k = 0; k < 64; ++k) f[k] = 150e6 + 1e5 * k;
  if (!imaging_grid_uniform(f.data(), 64, df) || df != 1e5) ++bad;
  f[10] += 5e-8;
  if (!imaging_grid_uniform(f.data(), 64, df)) ++bad;
  f[10] += 1e-6;
  if (imaging_grid_uniform(f.data(), 64, df)) ++bad;
  if (!imaging_grid_uniform(f.data(), 1, df) || df != 0.0) ++bad;
  // the figures the documents quote: 128 x 128 directions of 1024 channels, one snapshot, in the default budget
  const ImagingPlan h = imaging_plan(16384, 61075, 1024, 1, 0, false, 0, lds950, -1, true, 2);
  if (h.refusal || h.route != kImagingStepped || h.ntiles != 32 || h.nblocks != 64 || h.chunks.count != 1 || h.lds != 17408) ++bad;
  // the smallest budget tests/test_gpu_imaging.py gives: 1000 pixels in four chunks of one block
  const ImagingPlan s = imaging_plan(1000, 37, 70, 3, 2, false, 256 * imaging_pixel_bytes(70, 3, false), lds950, -1, true, 2);
  if (s.refusal || s.chunks.size != 256 || s.chunks.count != 4 || s.chunks.nstreams != 1) ++bad;
  checked += 9;
  std::printf("checked %ld bad %ld\n", checked, bad);
  return bad ? 1 : 0;
}
'''


def test_plan_header_compiles_alone_and_plans_soundly(tmp_path):
    src = tmp_path / 'imaging_plan_check.cpp'
    src.write_text(PLAN_PROGRAM)
    exe = tmp_path / 'imaging_plan_check'
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-Wall', '-Werror', '-fsanitize=address,undefined', '-I',
                           os.path.join(ROOT, 'prisim_amd', 'csrc_addon'), str(src), '-o', str(exe)])
    res = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = res.stdout.decode()
    assert res.returncode == 0, out
    assert out.strip().splitlines()[-1] == 'checked %d bad 0' % (5 * 5 * 2 * 3 * 2 * (8 * 3 * 2 + 3) + 9), out
    txt = open(os.path.join(ROOT, 'prisim_amd', 'csrc_addon', 'imaging_plan.h')).read()
    assert '#include <hip' not in txt and '__device__' not in txt and '#include "addon_internal.h"' not in txt


# ---- the checker against itself -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def g1():
    """The shapes of the largest parity case of tests/test_gpu_imaging.py: 300 baselines to 300 m, 70 channels, 3 snapshots, 65 pixels."""
    c = IC.case(nbl=300, nchan=70, npix=65, nt=3)
    c['want'] = IK.dirty_image(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], cube=c['cube'], weights=c['w_full'],
                               aberr_beta=c['beta'])
    return c


def test_checker_against_extended_precision_and_a_stepped_phasor(g1):
    c, want = g1, g1['want']
    tau = NP.einsum('tpi,bi->tpb', IK.directions(c['unitvec'], c['rot'], c['beta']) - c['pc'][:, None, :], c['baselines']) / IK.C_LIGHT
    assert 1.0e3 < float(NP.abs(2 * NP.pi * tau * c['freqs'][-1]).max()) < 2.0e3          # phases beyond a thousand radians
    if NP.finfo(NP.longdouble).eps < 1e-18:
        ext = IK.dirty_image(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], cube=c['cube'], weights=c['w_full'],
                             aberr_beta=c['beta'], dtype=NP.longdouble)
        dev = float(NP.max(NP.abs(want['image'] - ext['image']) / want['scale']))
        print('checker against longdouble: %.3e of the scale (bound %.1e)' % (dev, CHECKER_BOUND))
        assert dev <= CHECKER_BOUND
    stepped = IK.stepped_image(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], c['cube'], weights=c['w_full'],
                               aberr_beta=c['beta'], reseed=32)
    dev = float(NP.max(NP.abs(want['image'] - stepped) / want['scale']))
    print('a phasor stepped over 32 channels: %.3e of the scale (bound %.1e)' % (dev, CHECKER_BOUND))
    assert dev <= CHECKER_BOUND


def test_checker_against_the_two_closed_forms(g1):
    c = g1
    nt, nbl, nchan = c['cube'].shape
    # a point source of flux S seen through a delta beam images to S at its own direction, whatever the weights; the PSF is 1 at the
    # phase centre
    s_dir = IK.directions(c['unitvec'][7:8], c['rot'], c['beta'])[:, 0, :]
    S = 3.25
    v = IK.point_source_cube(s_dir, S, c['pc'], c['baselines'], c['freqs'])
    got = IK.dirty_image(c['unitvec'][7:8], c['rot'], c['pc'], c['baselines'], c['freqs'], cube=v, weights=c['w_full'], aberr_beta=c['beta'])
    dev = float(NP.max(NP.abs(got['image'] - S)) / S)
    print('point source: %.3e of S' % dev)
    assert dev <= CHECKER_BOUND and NP.allclose(got['scale'], S, rtol=1e-14)
    psf = IK.dirty_image(c['pc'][0:1], NP.repeat(NP.eye(3)[None], 1, axis=0), c['pc'][0:1], c['baselines'], c['freqs'], kind='psf',
                         weights=c['w_bl'])
    assert NP.allclose(psf['image'], 1.0, rtol=0, atol=1e-15) and NP.allclose(psf['scale'], 1.0, rtol=0, atol=1e-15)
    # the dot-product identity: sum_p x_p D[p][k] = Re sum_{t,b} w V conj(V_sim), V_sim the sky-sum of the fluxes x at the pixels
    x = NP.random.default_rng(5).uniform(0.5, 2.0, c['unitvec'].shape[0])
    vsim = IK.skysum(IK.directions(c['unitvec'], c['rot'], c['beta']), x, c['pc'], c['baselines'], c['freqs'])
    lhs = NP.einsum('p,pk->k', x, g1['want']['D'])
    rhs = NP.einsum('tbk,tbk->k', c['w_full'] * c['cube'], vsim.conj()).real
    bound = NP.abs(x).sum() * NP.einsum('tbk->k', c['w_full'] * NP.abs(c['cube']))
    dev = float(NP.max(NP.abs(lhs - rhs) / bound))
    print('dot-product identity: %.3e of sum|x| sum w|V|' % dev)
    assert dev <= CHECKER_BOUND
    # chan_avg is the ratio of the sums, not the mean of the ratios; a channel without weight is NaN alone
    w0 = c['w_full'].copy()
    w0[:, :, 4] = 0.0
    flagged = NP.ones(nchan, dtype=bool)
    flagged[4] = False
    per = IK.dirty_image(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], cube=c['cube'], weights=w0, aberr_beta=c['beta'],
                         nonzero=flagged)
    band = IK.dirty_image(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], cube=c['cube'], weights=w0, aberr_beta=c['beta'],
                          nonzero=flagged, chan_avg=True)
    assert NP.all(NP.isnan(per['image'][:, 4])) and NP.all(NP.isfinite(NP.delete(per['image'], 4, axis=1))) and per['wsum'][4] == 0.0
    assert NP.all(NP.isfinite(band['image'])) and NP.allclose(band['image'], per['D'].sum(axis=1) / per['wsum'].sum(), rtol=1e-14)
    with pytest.raises(AssertionError):
        IK.dirty_image(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], cube=c['cube'], weights=w0, aberr_beta=c['beta'])


# ---- the class against a stand-in context ---------------------------------------------------------------------------------------------

class ImagingOracleContext(fake_context.OracleContext):
    """OracleContext whose dirty_image is the numpy checker; it records what it was handed."""
    calls = []

    def dirty_image(self, unitvec, rot, pc_dircos, baselines, freqs_hz, cube=None, weights=None, kind='dirty', chan_avg=False,
                    aberr_beta=None, route='auto', budget_bytes=0):
        call = dict(unitvec=NP.array(unitvec), rot=NP.array(rot), pc=NP.array(pc_dircos), baselines=NP.array(baselines),
                    freqs=NP.array(freqs_hz), cube=None if cube is None else NP.array(cube), weights=None if weights is None else NP.array(weights),
                    kind=kind, chan_avg=chan_avg, beta=None if aberr_beta is None else NP.array(aberr_beta), route=route, budget_bytes=budget_bytes)
        ImagingOracleContext.calls.append(call)
        nt = call['rot'].reshape(-1, 9).shape[0]
        resident = cube is None and kind == 'dirty'
        v = self.cube[:nt] if resident else cube
        r = IK.dirty_image(unitvec, rot, pc_dircos, baselines, freqs_hz, cube=v, weights=weights, kind=kind, chan_avg=chan_avg,
                           aberr_beta=aberr_beta)
        return r['image'], r['wsum'], {'route': 'stepped' if route == 'auto' else route, 'terms': r['D'].size * self.nbl * nt, 'resident': resident}


LAT = -30.7224
CH = 150e6 + 1e5 * NP.arange(6)
BL = NP.array([[14.6, 0.0, 0.0], [7.3, 12.6, 0.1], [-7.3, 12.6, -0.2], [29.2, 0.0, 0.3]])
LABELS = [('1', '0'), ('2', '0'), ('2', '1'), ('3', '0')]
TELESCOPE = {'id': 'custom', 'shape': 'delta', 'size': 14.0, 'ocoords': 'altaz', 'orientation': NP.array([[90.0, 270.0]]), 'groundplane': None}
LSTS = [10.0, 10.5, 11.25]


def observed(monkeypatch, coords, pointings, reserve=False, skycoords='altaz', sky=None):
    monkeypatch.setattr(_abi, 'Context', ImagingOracleContext)
    ImagingOracleContext.calls = []
    ia = RI.InterferometerArray(LABELS, BL, CH, telescope=TELESCOPE, latitude=LAT, skycoords=skycoords, pointing_coords=coords)
    ia.frame_model = 'date'
    if reserve:
        ia.reserve(len(LSTS))
    if sky is None:
        sky = SM.SkyModel(location=[[80.0, 100.0], [50.0, 10.0]], flux_ref=[1.0, 3.0], spindex=[0.0, -0.7], ref_freq=150e6)
    for j, lst in enumerate(LSTS):
        ia.observe((2457000.5 + j / 64.0, lst), {'Tnet': 200.0}, NP.ones(CH.size), pointings[j], sky, 10.7)
    return ia


def test_constructor_takes_the_reference_attributes_and_raises_its_exceptions(monkeypatch):
    with pytest.raises(NameError):
        RI.ApertureSynthesis()
    with pytest.raises(TypeError):
        RI.ApertureSynthesis('an array')
    ia = observed(monkeypatch, 'altaz', [[90.0, 270.0]] * 3)
    aps = RI.ApertureSynthesis(ia)
    assert aps.ia is ia and aps.f is ia.channels and aps.df == ia.freq_resolution and aps.n_acc == 3 and aps.lst is ia.lst
    assert aps.phase_center_coords == 'altaz' and aps.pointing_coords == 'altaz' and aps.latitude == LAT and aps.timestamp is ia.timestamp
    assert NP.array_equal(aps.blxyz, GEOM.enu2xyz(BL, LAT, units='degrees'))
    assert aps.uvw is None and aps.uvw_lambda is None and aps.grid_ready is False and aps.gridu is None
    assert not hasattr(aps, 'setUVWgrid')                             # not ported: its grid is not in the reference tree


@pytest.mark.parametrize('coords, pointings', [('hadec', [[5.0, -25.0], [5.0, -25.0], [7.5, -31.0]]),
                                               ('altaz', [[90.0, 270.0], [80.0, 10.0], [65.0, 200.0]]),
                                               ('radec', [[12.0, -28.0], [12.0, -28.0], [9.0, -35.0]])])
def test_genuvw_is_project_baselines_at_the_phase_centre(monkeypatch, coords, pointings):
    ia = observed(monkeypatch, coords, pointings)
    aps = RI.ApertureSynthesis(ia)
    aps.genUVW()
    ia.project_baselines({'location': NP.asarray(ia.phase_center), 'coords': coords})
    want = ia.projected_baselines
    assert aps.uvw_lambda.shape == (4, 3, 3) and aps.uvw.shape == (4, 3, 6, 3)
    assert NP.max(NP.abs(aps.uvw_lambda - want)) <= 1e-12 * NP.max(NP.abs(BL))
    assert NP.allclose(aps.uvw, want[:, :, None, :] * CH[None, None, :, None] / RI.C_LIGHT, rtol=1e-13, atol=1e-12)
    # w is the baseline along the phase centre; 'radec' follows the centre (HA = LST - RA), not the meridian
    pc = ia._pc_dircos(ia.phase_center, coords)
    assert NP.max(NP.abs(aps.uvw_lambda[:, 2, :] - BL.dot(pc.T))) <= 1e-12 * NP.max(NP.abs(BL))
    r = aps.reorderUVW()
    assert r.shape == (3, 4 * 6 * 3) and NP.array_equal(r[1].reshape(4, 6, 3), aps.uvw[:, 1]) and r[2, 1] == aps.uvw[0, 2, 0, 1]
    aps.phase_center_coords = 'dircos'
    with pytest.raises(ValueError):
        aps.genUVW()


def test_dircos_grid_values_and_refusal():
    g = RI.ApertureSynthesis.dircos_grid(5, 0.6)
    ax = NP.linspace(-0.6, 0.6, 5)
    assert g.shape == (25, 3) and NP.array_equal(g[:5, 0], ax) and NP.all(g[:5, 1] == -0.6) and NP.array_equal(g[::5, 1], ax)
    assert NP.allclose(NP.sum(g * g, axis=1), 1.0, rtol=0, atol=1e-15) and NP.all(g[:, 2] > 0) and NP.array_equal(g[12], [0.0, 0.0, 1.0])
    assert RI.ApertureSynthesis.dircos_grid(2, NP.sqrt(0.5)).shape == (4, 3)
    assert NP.array_equal(RI.ApertureSynthesis.dircos_grid(1, 0.3), [[0.0, 0.0, 1.0]])
    for bad in (0.7072, -0.1, NP.nan):
        with pytest.raises(ValueError):
            RI.ApertureSynthesis.dircos_grid(4, bad)
    with pytest.raises(ValueError):
        RI.ApertureSynthesis.dircos_grid(0, 0.1)


def test_image_and_psf_argument_checks(monkeypatch):
    ia = observed(monkeypatch, 'altaz', [[90.0, 270.0]] * 3)
    aps = RI.ApertureSynthesis(ia)
    grid = aps.dircos_grid(3, 0.2)
    with pytest.raises(ValueError, match='coords'):
        aps.image(grid, coords='galactic')
    with pytest.raises(ValueError, match='datakey'):
        aps.image(grid, datakey='vis')
    with pytest.raises(ValueError, match='vis_freq'):
        aps.image(grid, datakey='noisy')                              # no noise was added: there is no such cube
    with pytest.raises(ValueError, match='vis_noise_freq'):
        aps.image(grid, datakey='noise')
    for w in (NP.ones(3), NP.ones((4, 6)), NP.ones((3, 4, 6)), NP.ones((4, 6, 2))):
        with pytest.raises(ValueError, match='weights'):
            aps.image(grid, weights=w)
        with pytest.raises(ValueError, match='weights'):
            aps.psf(grid, weights=w)
    with pytest.raises(ValueError, match='route'):
        aps.image(grid, route='fast')
    with pytest.raises(ValueError):
        aps.image(NP.ones((3, 3)), coords='dircos')                   # beyond the unit sphere
    with pytest.raises(ValueError):
        aps.image(NP.ones((3, 4)) * 0.1, coords='dircos')
    with pytest.raises(ValueError):
        aps.image(grid, coords='altaz')                               # three columns of degrees
    assert not ImagingOracleContext.calls                             # nothing reached the device
    empty = RI.InterferometerArray(LABELS, BL, CH, telescope=TELESCOPE, latitude=LAT, skycoords='altaz', pointing_coords='altaz')
    with pytest.raises(ValueError, match='observe'):
        RI.ApertureSynthesis(empty).psf(grid)


def test_image_marshals_directions_frames_cube_and_weights(monkeypatch):
    pointings = [[12.0, -28.0], [12.0, -28.0], [9.0, -35.0]]
    ia = observed(monkeypatch, 'radec', pointings)
    aps = RI.ApertureSynthesis(ia)
    calls = ImagingOracleContext.calls
    pc = ia._pc_dircos(ia.phase_center, 'radec')
    vis_t = NP.transpose(ia.skyvis_freq, (2, 0, 1))

    # local direction cosines: the identity per snapshot, two columns completed on the sphere, the cube handed over snapshot-major
    lm = NP.array([[0.0, 0.0], [0.1, -0.2], [-0.3, 0.05]])
    img = aps.image(lm, coords='dircos')
    c = calls[-1]
    assert img.shape == (3, 6) and c['kind'] == 'dirty' and c['route'] == 'auto' and c['beta'] is None and c['weights'] is None
    assert NP.array_equal(c['rot'], NP.repeat(NP.eye(3)[None], 3, axis=0)) and NP.array_equal(c['pc'], pc)
    assert NP.array_equal(c['unitvec'][:, :2], lm) and NP.allclose(NP.sum(c['unitvec'] ** 2, axis=1), 1.0, atol=1e-15, rtol=0)
    assert NP.array_equal(c['baselines'], BL) and NP.array_equal(c['freqs'], CH)
    assert c['cube'].shape == (3, 4, 6) and c['cube'].dtype == NP.complex128 and NP.array_equal(c['cube'], vis_t)
    assert aps.image_stats['route'] == 'stepped' and aps.image_stats['resident'] is False and aps.image_stats['wsum'].shape == (6,)

    # alt-az and hour angle-declination: the catalogue's unit vectors, the identity and hadec_to_enu
    aa = NP.array([[80.0, 100.0], [50.0, 10.0]])
    aps.image(aa, coords='altaz', weights=NP.arange(1.0, 5.0), chan_avg=True, route='direct', budget_bytes=12345)
    c = calls[-1]
    assert NP.array_equal(c['unitvec'], GEOM.catalog_unitvec(aa, 'altaz')) and NP.array_equal(c['rot'][2], NP.eye(3))
    assert NP.array_equal(c['weights'], NP.arange(1.0, 5.0)) and c['chan_avg'] is True and c['route'] == 'direct' and c['budget_bytes'] == 12345
    aps.image(aa, coords='hadec')
    c = calls[-1]
    assert NP.array_equal(c['unitvec'], GEOM.catalog_unitvec(aa, 'hadec'))
    assert all(NP.array_equal(c['rot'][t], FRAMES.hadec_to_enu(LAT)) for t in range(3))

    # right ascension-declination: per snapshot, the frame observe() applies to a 'radec' sky; an epoch turns precession on
    rd = NP.array([[11.0, -29.0], [14.0, -20.0]])
    full_w = NP.random.default_rng(1).uniform(0.0, 1.0, (4, 6, 3))
    aps.image(rd, coords='radec', weights=full_w)
    c = calls[-1]
    for t in range(3):
        r, b = FRAMES.snapshot_frame('radec', LSTS[t], LAT, jd=ia.timestamp[t], epoch=None, model='date')
        assert NP.array_equal(c['rot'][t], r) and NP.array_equal(c['beta'][t], b)
    assert not NP.array_equal(c['rot'][0], c['rot'][2]) and NP.array_equal(c['unitvec'], GEOM.catalog_unitvec(rd, 'radec'))
    assert c['weights'].shape == (3, 4, 6) and NP.array_equal(c['weights'], NP.transpose(full_w, (2, 0, 1)))
    ia.frame_model = 'apparent'
    aps.image(rd, coords='radec', epoch='J2000')
    c = calls[-1]
    r, b = FRAMES.snapshot_frame('radec', LSTS[1], LAT, jd=ia.timestamp[1], epoch='J2000', model='apparent')
    assert NP.array_equal(c['rot'][1], r) and NP.array_equal(c['beta'][1], b) and NP.any(b != 0.0)
    seen = []
    ia.frame_provider = lambda jd, lst, skymodel: (seen.append((jd, lst, skymodel.epoch)) or (NP.eye(3), NP.full(3, 1e-5)))
    aps.image(rd, coords='radec', epoch='J1950')
    assert seen == [(ia.timestamp[t], LSTS[t], 'J1950') for t in range(3)] and NP.array_equal(calls[-1]['beta'], NP.full((3, 3), 1e-5))
    ia.frame_provider = None

    # the synthesized beam: no cube, and 1 at every snapshot's phase centre when that centre is one direction
    n0 = len(calls)
    psf = aps.psf(lm, coords='dircos', weights=NP.ones(4))
    assert len(calls) == n0 + 1 and calls[-1]['kind'] == 'psf' and calls[-1]['cube'] is None and psf.shape == (3, 6)
    # the other cubes, handed over
    ia.generate_noise(seed=3)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')                               # (no gain table: unity gains)
        ia.add_noise()
    aps.image(lm, datakey='noisy')
    assert NP.array_equal(calls[-1]['cube'], NP.transpose(ia.vis_freq, (2, 0, 1)))
    aps.image(lm, datakey='noise')
    assert NP.array_equal(calls[-1]['cube'], NP.transpose(ia.vis_noise_freq, (2, 0, 1)))


def test_image_reads_the_resident_cube_where_it_lies_and_finds_the_sources(monkeypatch):
    """An array observed after reserve(): the noiseless cube is not handed over.  Two sources through a delta beam with a flat
    spectrum, imaged at their own alt-az positions: each images to its flux plus the other's sidelobe, which the checker's PSF gives."""
    sky = SM.SkyModel(location=[[80.0, 100.0], [50.0, 10.0]], flux_ref=[1.0, 3.0], spindex=[0.0, 0.0], ref_freq=150e6)
    ia = observed(monkeypatch, 'altaz', [[90.0, 270.0]] * 3, reserve=True, sky=sky)
    aps = RI.ApertureSynthesis(ia)
    aa = NP.array([[80.0, 100.0], [50.0, 10.0]])
    img = aps.image(aa, coords='altaz')
    c = ImagingOracleContext.calls[-1]
    assert c['cube'] is None and aps.image_stats['resident'] is True
    dc = GEOM.catalog_unitvec(aa, 'altaz')
    pc = ia._pc_dircos(ia.phase_center, 'altaz')
    eye = NP.repeat(NP.eye(3)[None], 3, axis=0)
    side = IK.dirty_image(dc[1:2], eye, NP.repeat(dc[0:1], 3, axis=0), BL, CH, kind='psf')['image'][0]      # the beam centred on source 0, at source 1
    assert NP.allclose(img[0], 1.0 + 3.0 * side, rtol=0, atol=1e-9) and NP.allclose(img[1], 3.0 + 1.0 * side, rtol=0, atol=1e-9)
    assert NP.array_equal(c['pc'], pc)
    # once skyvis_freq is replaced the slots are out of step: the cube is handed over
    ia.skyvis_freq = NP.array(ia.skyvis_freq) * 2.0
    img2 = aps.image(aa, coords='altaz')
    assert ImagingOracleContext.calls[-1]['cube'] is not None and NP.allclose(img2, 2.0 * img, rtol=1e-13)
