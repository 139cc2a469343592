"""CPU: the beam-weighted mosaic of the snapshots (include/prisim_mosaic.h) -- the export and both structs against the compiled header
(tests/test_abi_headers.py holds every mirror to the headers as well), the planning header compiled alone, the numpy checker
(tests/mosaic_checker.py) against two closed forms, the inputs the GPU tests rely on (tests/mosaic_cases.py), and the method
prisim_amd.interferometry.ApertureSynthesis.mosaic against a stand-in context that answers mosaic_image with the checker.

Bounds of the checker's self-tests: 1e-12 of the natural scale, a tenth of what the device is held to, as in tests/test_imaging.py;
the figures measured are printed."""
import ctypes as C
import os
import subprocess
import sys

import numpy as NP
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fake_context  # noqa: E402
import imaging_cases as IC  # noqa: E402
import imaging_checker as IK  # noqa: E402
import mosaic_cases as MC  # noqa: E402
import mosaic_checker as MK  # noqa: E402

from prisim_amd import _abi  # noqa: E402
from prisim_amd import frames as FRAMES  # noqa: E402
from prisim_amd import geometry as GEOM  # noqa: E402
from prisim_amd import interferometry as RI  # noqa: E402
from prisim_amd import primary_beams as PB  # noqa: E402
from prisim_amd import skymodel as SM  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECKER_BOUND = 1e-12


# ---- the library and its headers ----------------------------------------------------------------------------------------------------

def test_export_is_in_the_library_and_outside_the_core_abi():
    lib = _abi.load_library()
    assert _abi.MOSAIC_EXPORTS == ('prisim_mosaic_image',) == _abi.HEADER_EXPORTS['prisim_mosaic.h']
    assert 'prisim_mosaic_image' not in _abi.EXPORTS and lib.prisim_hip_version().decode() == _abi.ABI_VERSION
    assert lib.prisim_mosaic_image(None, None, None, None, None, None, None, None) == _abi.PRISIM_EINVAL      # a null context: refused, nothing read
    assert not hasattr(_abi, 'PrisimMosaicStats')                     # the struct lives on the class (tests/test_abi_helpers.py)
    assert set(_abi._stats_dict(_abi.Context.PrisimMosaicStats())) == {
        'wall_ms', 'kernel_ms', 'terms', 'beam_values', 'chunks', 'chunk_pixels', 'pixel_bytes', 'kernel_bytes', 'upload_bytes',
        'download_bytes', 'route', 'streams', 'chan_tile', 'reseed', 'lds_bytes', 'block_pixels'}
    src = open(os.path.join(ROOT, 'prisim_amd', 'csrc_imaging', 'mosaic.hip')).read()
    assert 'atomic' not in src.replace('No atomics', '') and 'fma(' in src
    assert 'img_tile_pass<STEPPED, false>(' in src and 'launch_beam_flux(' in src and 'beam_flux_body' not in src      # called, not restated
    # ... by k_mos_sum, once, in the header that this entry and the mosaic's CLEAN include; the CLEAN's own call of it is the shared update's
    folder = os.path.join(ROOT, 'prisim_amd', 'csrc_imaging')
    assert open(os.path.join(folder, 'mosaic_kernels.h')).read().count('img_tile_pass<STEPPED, false>(') == 1 and '#include "mosaic_kernels.h"' in src
    assert 'img_tile_pass' not in open(os.path.join(folder, 'mosclean.hip')).read()
    assert 'img_rows' not in src and 'sh_b[tid] =' not in src and 'prisim_imaging_args ia' not in src and 'k_mos_dirs' not in src
    assert '#include "imaging_kernels.h"' in src and 'dirty_image.h"' not in src and 'Wunused' not in src      # it compiles what it launches
    ant = open(os.path.join(ROOT, 'prisim_amd', 'csrc_antpower', 'antpower.hip')).read()
    assert 'beam_setup.h' in ant and 'beam_setup.h' in src and 'void fill_beam' not in ant + src       # one statement of the beam's set-up
    header = open(os.path.join(ROOT, 'include', 'prisim_mosaic.h')).read()
    for name in ('prisim_hip.h', 'prisim_hip_last_error', 'prisim_hip_set_sky_analytic'):
        header = header.replace(name, '')
    assert 'prisim_hip_' not in header


def test_structs_and_constants_against_the_compiled_header(tmp_path):
    fields = {'prisim_mosaic_args': _abi.Context.PrisimMosaicArgs, 'prisim_mosaic_stats': _abi.Context.PrisimMosaicStats}
    consts = ('PRISIM_IMAGE_AUTO', 'PRISIM_IMAGE_DIRECT', 'PRISIM_IMAGE_STEPPED', 'PRISIM_IMAGE_W_NONE', 'PRISIM_IMAGE_W_BASELINE',
              'PRISIM_IMAGE_W_FULL', 'PRISIM_BEAM_DELTA', 'PRISIM_BEAM_GAUSSIAN', 'PRISIM_BEAM_AIRY', 'PRISIM_BEAM_DIPOLE', 'PRISIM_BEAM_POLY')
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "prisim_mosaic.h"', 'int main(void) {']
    for cname, cls in fields.items():
        lines.append('  printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        lines += ['  printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (cname, f, cname, f, cname, f) for f, _ in cls._fields_]
    lines += ['  printf("%s %%d\\n", (int)%s);' % (n, n) for n in consts] + ['  return 0;', '}']
    src, exe = tmp_path / 'mosaic_abi.c', tmp_path / 'mosaic_abi'
    src.write_text('\n'.join(lines))
    subprocess.check_call(['gcc', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])      # alone: it includes what it needs
    got = {ln.split()[0]: [int(x) for x in ln.split()[1:]] for ln in subprocess.check_output([str(exe)]).decode().splitlines()}
    for cname, cls in fields.items():
        assert got[cname] == [C.sizeof(cls)]
        for f, ftype in cls._fields_:
            assert got[cname + '.' + f] == [getattr(cls, f).offset, C.sizeof(ftype)], (cname, f)
    for n in consts:
        assert got[n] == [getattr(_abi, n)], n
    # the fields of prisim_imaging_args less `kind`, in their order, then the beam's, pbmin and the budget
    names = [f for f, _ in _abi.Context.PrisimMosaicArgs._fields_]
    shared = [f for f, _ in _abi.Context.PrisimImagingArgs._fields_ if f not in ('kind', 'budget_bytes')]
    assert names[:len(shared)] == shared
    assert names[len(shared):] == ['beam_kind', 'diameter_m', 'beam_pc_dircos', 'beam_pc_snap', 'ext', 'n_ext', 'pbmin', 'budget_bytes']


PLAN_PROGRAM = r'''
#include "mosaic_plan.h"

#include <cstdint>
#include <cstdio>
#include <cstring>

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
            const int64_t per = mosaic_pixel_bytes(nchan, nt, avg != 0), one = kImagingBlock * per;
            // the stated formula: two direction tables, the beam tile, N and Q, the two outputs
            if (per != 64 * nt + 8 * nchan + 16 * nchan + (avg ? 16 : 16 * nchan)) ++bad;
            const int64_t budgets[] = {0, one, one + 1, 2 * one - 1, 2 * one, 3 * one + 12345, int64_t(1) << 24, int64_t(1) << 30};
            for (int64_t budget : budgets)
              for (int asked = -1; asked <= 1; ++asked)
                for (int uniform = 0; uniform < 2; ++uniform) {
                  const MosaicPlan p = mosaic_plan(npix, 300, nchan, nt, form, avg != 0, budget, lds950, asked, uniform != 0, 2);
                  const int64_t have = budget_or_default(budget);
                  bool ok = true;
                  ++checked;
                  if (asked == kImagingStepped && !uniform) {          // an explicit STEPPED on a non-uniform grid is refused
                    if (!p.refusal || !std::strstr(p.refusal, "uniform")) { std::printf("stepped on a non-uniform grid accepted\n"); ++bad; }
                    continue;
                  }
                  if (budget > 0 && budget < one) {                    // (1 << 24 does not hold one block of 1024 channels)
                    if (!p.refusal || !std::strstr(p.refusal, "one block")) { std::printf("a budget below one block accepted\n"); ++bad; }
                    continue;
                  }
                  ok = p.refusal == nullptr;
                  // the route rules of prisim_dirty_image, unchanged
                  ok = ok && p.route == (asked >= 0 ? asked : uniform ? kImagingStepped : kImagingDirect);
                  ok = ok && p.reseed == (p.route == kImagingStepped ? K : 1);
                  // tile, block and LDS are those of k_img_sum and do not change with the budget
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
            if (!mosaic_plan(npix, 300, nchan, nt, form, avg != 0, one - 1, lds950, -1, true, 2).refusal) ++bad;
            if (!mosaic_plan(npix, 300, nchan, nt, form, avg != 0, 0, kImagingLds - 1, -1, true, 2).refusal) ++bad;
            if (mosaic_plan(npix, 300, nchan, nt, form, avg != 0, 0, kImagingLds, -1, true, 2).refusal) ++bad;
            checked += 3;
          }
  if (!mosaic_plan(10, 10, 10, 1, 3, false, 0, lds950, -1, true, 2).refusal || !mosaic_plan(10, 10, 10, 1, 0, false, 0, lds950, 2, true, 2).refusal ||
      !mosaic_plan(0, 10, 10, 1, 0, false, 0, lds950, -1, true, 2).refusal)
    ++bad;
  // the figures the documents quote: 128 x 128 directions of 1024 channels, four snapshots, in the default budget -- 41216 B a
  // pixel, 675 MB in all: two chunks of 50 and 14 blocks, one on each stream
  const MosaicPlan h = mosaic_plan(16384, 61075, 1024, 4, 0, false, 0, lds950, -1, true, 2);
  if (h.refusal || h.route != kImagingStepped || h.ntiles != 32 || h.nblocks != 64 || h.chunks.count != 2 || h.chunks.size != 12800 ||
      h.chunks.nstreams != 2 || h.lds != 17408 || h.pixel_bytes != 41216)
    ++bad;
  // the smallest budget tests/test_gpu_mosaic.py gives: 1000 pixels in four chunks of one block
  const MosaicPlan s = mosaic_plan(1000, 37, 33, 3, 2, false, 256 * mosaic_pixel_bytes(33, 3, false), lds950, -1, true, 2);
  if (s.refusal || s.chunks.size != 256 || s.chunks.count != 4 || s.chunks.nstreams != 1) ++bad;
  // the plan of prisim_dirty_image is what it was: the same arithmetic over its own bytes per pixel
  const ImagingPlan d = imaging_plan(1000, 37, 70, 3, 2, false, 256 * imaging_pixel_bytes(70, 3, false), lds950, -1, true, 2);
  if (d.refusal || d.pixel_bytes != 32 * 3 + 8 * 70 || d.chunks.size != 256 || d.chunks.count != 4) ++bad;
  checked += 6;
  std::printf("checked %ld bad %ld\n", checked, bad);
  return bad ? 1 : 0;
}
'''


def test_plan_header_compiles_alone_and_plans_soundly(tmp_path):
    src = tmp_path / 'mosaic_plan_check.cpp'
    src.write_text(PLAN_PROGRAM)
    exe = tmp_path / 'mosaic_plan_check'
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-Wall', '-Werror', '-fsanitize=address,undefined', '-I',
                           os.path.join(ROOT, 'prisim_amd', 'csrc_addon'), str(src), '-o', str(exe)])
    res = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = res.stdout.decode()
    assert res.returncode == 0, out
    assert out.strip().splitlines()[-1] == 'checked %d bad 0' % (5 * 5 * 2 * 3 * 2 * (8 * 3 * 2 + 3) + 6), out
    txt = open(os.path.join(ROOT, 'prisim_amd', 'csrc_addon', 'mosaic_plan.h')).read()
    assert '#include <hip' not in txt and '__device__' not in txt and '#include "addon_internal.h"' not in txt


# ---- the checker against itself, and the inputs of the GPU tests ---------------------------------------------------------------------

def chromatic_gaussian(size):
    return {'element': 'gaussian', 'size': size}


def test_checker_returns_the_flux_of_a_point_source_through_a_drifting_chromatic_beam():
    """D_t = A_t S W_t at the source's own pixel, so N / Q = S for any drift and chromaticity.  Three snapshots of a 'radec' source that
    drifts through a Gaussian beam at the zenith whose width changes by a third over the band."""
    lat, lsts = MC.LAT, [30.0, 33.0, 37.0]
    freqs = NP.linspace(120e6, 180e6, 5)
    src = GEOM.catalog_unitvec(NP.array([[34.0, lat + 3.0]]), 'radec')
    frames = [FRAMES.snapshot_frame('radec', l, lat, model='date') for l in lsts]
    rot, beta = NP.stack([f[0] for f in frames]), NP.stack([f[1] for f in frames])
    c = IC.case(37, 5, 1, 3)
    pc = NP.repeat(NP.array([[0.0, 0.0, 1.0]]), 3, axis=0)
    s = IK.directions(src, rot, beta)                                  # (3, 1, 3)
    setup = chromatic_gaussian(10.0)
    A = MK.beams(s, freqs, setup)[:, 0, :]                            # (3, 5)
    print('beam at the source, per snapshot and channel:\n', A)
    assert A.max() < 0.95 and A.min() > 0.01
    assert NP.max(A[:, 2]) > 1.5 * NP.min(A[:, 2])                    # drifting: the snapshots see the source through different beams
    assert NP.max(A[:, 0] / A[:, 4]) > 1.5                            # chromatic: so do the band's ends
    S = 3.25
    cube = A[:, NP.newaxis, :] * IK.point_source_cube(s[:, 0, :], S, pc, c['baselines'], freqs)
    for weights in (None, c['w_bl'], c['w_full']):
        ref = MK.mosaic(src, rot, pc, c['baselines'], freqs, cube, setup, weights=weights, aberr_beta=beta, pbmin=0.0)
        dev = float(NP.max(NP.abs(ref['mosaic'] - S)) / S)
        print('point source through a drifting chromatic beam: %.3e of S' % dev)
        assert dev <= CHECKER_BOUND
        band = MK.quotient(ref['num'], ref['den'], ref['wsum'], 0.0, chan_avg=True)[0]
        assert float(NP.max(NP.abs(band - S)) / S) <= CHECKER_BOUND
        # the dirty image of the same cube is an apparent flux: off by the beam
        img = IK.dirty_image(src, rot, pc, c['baselines'], freqs, cube=cube, weights=weights, aberr_beta=beta)['image']
        assert NP.all(NP.abs(img - S) > 0.05 * S)


def test_checker_with_a_delta_beam_on_one_snapshot_is_the_dirty_image():
    c = MC.up_case(37, 33, 65, 1)
    for weights in (None, c['w_bl'], c['w_full']):
        ref = MK.mosaic(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], c['cube'], {'element': 'delta'}, weights=weights,
                        aberr_beta=c['beta'])
        img = IK.dirty_image(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], cube=c['cube'], weights=weights, aberr_beta=c['beta'])
        assert NP.all(ref['A'] == 1.0) and NP.array_equal(ref['den'], NP.broadcast_to(ref['wsum'], ref['den'].shape))
        assert NP.array_equal(ref['num'], img['D']) and NP.array_equal(ref['mosaic'], img['image']) and NP.array_equal(ref['wsum'], img['wsum'])
        assert NP.all(ref['pb_eff'] == 1.0)
        band = MK.quotient(ref['num'], ref['den'], ref['wsum'], 0.1, chan_avg=True)[0]
        assert NP.max(NP.abs(band - img['band']['image'])) <= CHECKER_BOUND * img['band']['scale']      # (another order of the sum over k)
    # below the horizon the delta beam is 0 too: the mask is the checker's own, whatever the pattern
    d = MC.up_case(37, 33, 65, 1, down=20)
    ref = MK.mosaic(d['unitvec'], d['rot'], d['pc'], d['baselines'], d['freqs'], d['cube'], {'element': 'delta'}, aberr_beta=d['beta'], pbmin=0.0)
    assert NP.all(NP.isnan(ref['mosaic'][45:])) and NP.all(NP.isfinite(ref['mosaic'][:45])) and NP.all(ref['den'][45:] == 0.0)
    with pytest.raises(AssertionError):                               # a direction that grazes the horizon is no test input
        MK.beams(NP.array([[[1.0, 0.0, 1e-12]]]), d['freqs'], {'element': 'delta'})


def test_the_masked_pixel_case_is_decided_on_the_cpu():
    c = MC.mask_case()
    beam = MC.beam_setups(3)['gaussian']
    ref = MK.mosaic(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], c['cube'], beam[3], weights=c['w_full'], aberr_beta=c['beta'],
                    pbmin=MC.MASK_PBMIN)
    masked = MK.assert_mask_is_decided(ref, MC.MASK_PBMIN)
    print('masked at pbmin %.2f: %.3f of the elements' % (MC.MASK_PBMIN, masked))
    assert NP.array_equal(NP.isnan(ref['mosaic']), ref['den'] < MC.MASK_PBMIN ** 2 * ref['wsum'][NP.newaxis, :])
    # the conditions bite: a mask that keeps everything, and an element on the threshold, are turned away
    with pytest.raises(AssertionError):
        MK.assert_mask_is_decided(ref, 1e-6)
    edge = dict(ref, den=ref['den'].copy())
    edge['den'][0, 0] = MC.MASK_PBMIN ** 2 * ref['wsum'][0] * (1.0 + 1e-9)
    with pytest.raises(AssertionError):
        MK.assert_mask_is_decided(edge, MC.MASK_PBMIN)
    # the parity cases of the GPU suite weigh a good part of their sky: no beam of theirs is all zeros or all ones
    g = IC.case(37, 5, 63, 1)
    s = IK.directions(g['unitvec'], g['rot'], g['beta'])
    for name, (_, _, _, setup) in MC.beam_setups(1).items():
        if name != 'delta':
            A = MK.beams(s, g['freqs'], setup)
            assert NP.mean(A > 1e-3) > 0.2 and NP.mean(A == 0.0) > 0.2, name


@pytest.mark.parametrize('coords', ['radec', 'altaz'])
def test_the_drift_scan_of_the_end_to_end_test_shows_an_apparent_flux_that_is_off(coords):
    """The geometry tests/test_gpu_mosaic.py observes, here through the checker alone: the source sits where the 14 m Gaussian is
    between 0.2 and 0.9, the dirty image is off by far more than a hundredth, the mosaic returns the flux."""
    S, nt = MC.FLUX, 3
    src = MC.SOURCE_RADEC if coords == 'radec' else MC.SOURCE_ALTAZ
    uv = GEOM.catalog_unitvec(src, coords)
    if coords == 'radec':
        frames = [FRAMES.snapshot_frame('radec', MC.LSTS[t], MC.LAT, jd=MC.JD0 + t / 64.0, epoch=None, model='date') for t in range(nt)]
        rot, beta = NP.stack([f[0] for f in frames]), NP.stack([f[1] for f in frames])
    else:
        rot, beta = NP.repeat(NP.eye(3)[None], nt, axis=0), None
    pc = NP.repeat(GEOM.altaz2dircos(NP.array([MC.ZENITH]), 'degrees'), nt, axis=0)
    bl = MC.e2e_baselines()
    s = IK.directions(uv, rot, beta)
    setup = chromatic_gaussian(14.0)
    A = MK.beams(s, MC.CH, setup)[:, 0, :]
    assert 0.2 < A.min() and A.max() < 0.9 and (coords == 'altaz' or A[0].max() < 0.8 * A[2].min())
    cube = A[:, NP.newaxis, :] * IK.point_source_cube(s[:, 0, :], S, pc, bl, MC.CH)
    ref = MK.mosaic(uv, rot, pc, bl, MC.CH, cube, setup, aberr_beta=beta)
    img = IK.dirty_image(uv, rot, pc, bl, MC.CH, cube=cube, aberr_beta=beta)['image']
    assert NP.max(NP.abs(ref['mosaic'] - S)) <= CHECKER_BOUND * S and NP.all(NP.abs(img - S) > 0.01 * S)
    print('%s: beam at the source %.3f .. %.3f, the dirty image %.3f of S' % (coords, A.min(), A.max(), float(img.mean() / S)))


# ---- the class against a stand-in context ---------------------------------------------------------------------------------------------

class MosaicOracleContext(fake_context.OracleContext):
    """OracleContext whose mosaic_image is the numpy checker; it records what it was handed."""
    calls = []

    def mosaic_image(self, unitvec, rot, pc_dircos, baselines, freqs_hz, beam_kind, diameter_m, beam_pc_dircos=(0.0, 0.0, 1.0), ext=None,
                     cube=None, weights=None, chan_avg=False, aberr_beta=None, pbmin=0.1, route='auto', budget_bytes=0, want_sums=True):
        call = dict(unitvec=NP.array(unitvec), rot=NP.array(rot), pc=NP.array(pc_dircos), baselines=NP.array(baselines),
                    freqs=NP.array(freqs_hz), beam_kind=beam_kind, diameter=diameter_m, beam_pc=NP.array(beam_pc_dircos), ext=ext,
                    cube=None if cube is None else NP.array(cube), weights=None if weights is None else NP.array(weights), chan_avg=chan_avg,
                    beta=None if aberr_beta is None else NP.array(aberr_beta), pbmin=pbmin, route=route, budget_bytes=budget_bytes)
        MosaicOracleContext.calls.append(call)
        nt = call['rot'].reshape(-1, 9).shape[0]
        v = self.cube[:nt] if cube is None else cube
        r = MK.mosaic(unitvec, rot, pc_dircos, baselines, freqs_hz, v, MK.setups_of(beam_kind, diameter_m, beam_pc_dircos, ext, nt),
                      weights=weights, chan_avg=chan_avg, aberr_beta=aberr_beta, pbmin=pbmin)
        st = {'route': 'stepped' if route == 'auto' else route, 'terms': r['num'].size * self.nbl * nt, 'resident': cube is None,
              'pb_eff': r['pb_eff']}
        return r['mosaic'], r['num'], r['den'], r['wsum'], st


LAT = MC.LAT
CH = 150e6 + 1e5 * NP.arange(6)
BL = NP.array([[14.6, 0.0, 0.0], [7.3, 12.6, 0.1], [-7.3, 12.6, -0.2], [29.2, 0.0, 0.3]])
LABELS = [('1', '0'), ('2', '0'), ('2', '1'), ('3', '0')]
LSTS = MC.LSTS


def observed(monkeypatch, telescope, pointings, pointing_coords='altaz', skycoords='radec', reserve=False, sky=None):
    monkeypatch.setattr(_abi, 'Context', MosaicOracleContext)
    MosaicOracleContext.calls = []
    ia = RI.InterferometerArray(LABELS, BL, CH, telescope=telescope, latitude=LAT, skycoords=skycoords, pointing_coords=pointing_coords)
    ia.frame_model = 'date'
    if reserve:
        ia.reserve(len(LSTS))
    if sky is None:
        sky = SM.SkyModel(location=MC.SOURCE_RADEC if skycoords == 'radec' else MC.SOURCE_ALTAZ, flux_ref=[MC.FLUX], spindex=[0.0], ref_freq=150e6)
    for j, lst in enumerate(LSTS):
        ia.observe((MC.JD0 + j / 64.0, lst), {'Tnet': 200.0}, NP.ones(CH.size), pointings[j], sky, 10.7)
    return ia


def test_mosaic_of_a_drift_scan_through_the_class_returns_the_flux(monkeypatch):
    ia = observed(monkeypatch, MC.GAUSS14, [MC.ZENITH] * 3)
    aps = RI.ApertureSynthesis(ia)
    got = aps.mosaic(MC.SOURCE_RADEC, coords='radec')
    c = MosaicOracleContext.calls[-1]
    # the specs of the three snapshots are one: a single element pointing, no extension
    assert c['beam_kind'] == _abi.PRISIM_BEAM_GAUSSIAN and c['diameter'] == 14.0 and c['ext'] is None and c['beam_pc'].shape == (3,)
    assert NP.allclose(c['beam_pc'], [0.0, 0.0, 1.0], atol=1e-15, rtol=0) and c['pbmin'] == 0.1 and c['route'] == 'auto'
    assert NP.array_equal(c['cube'], NP.transpose(ia.skyvis_freq, (2, 0, 1))) and c['weights'] is None
    for t in range(3):
        r, b = FRAMES.snapshot_frame('radec', LSTS[t], LAT, jd=ia.timestamp[t], epoch=None, model='date')
        assert NP.array_equal(c['rot'][t], r) and NP.array_equal(c['beta'][t], b)
    assert NP.array_equal(c['pc'], ia._pc_dircos(ia.phase_center, ia.phase_center_coords)) and NP.array_equal(c['baselines'], BL)
    # what the stand-in's sky-sum simulated through its Gaussian comes back as the catalogue's flux; the dirty image would not
    assert got.shape == (1, 6) and NP.max(NP.abs(got - MC.FLUX)) <= 1e-9 * MC.FLUX
    st = aps.image_stats
    assert set(('num', 'den', 'wsum', 'pb_eff', 'route', 'resident', 'terms')) <= set(st)
    assert st['num'].shape == st['den'].shape == (1, 6) and st['wsum'].shape == (6,) and st['pb_eff'].shape == (1, 6) and st['resident'] is False
    assert NP.array_equal(st['wsum'], NP.full(6, 12.0)) and NP.all((st['pb_eff'] > 0.2) & (st['pb_eff'] < 0.9))
    assert NP.array_equal(got, MK.quotient(st['num'], st['den'], st['wsum'], 0.1)[0])
    # the other arguments, handed on
    full_w = NP.random.default_rng(1).uniform(0.5, 1.0, (4, 6, 3))
    band = aps.mosaic(MC.SOURCE_RADEC, coords='radec', weights=full_w, chan_avg=True, pbmin=0.0, route='direct', budget_bytes=12345)
    c = MosaicOracleContext.calls[-1]
    assert band.shape == (1,) and c['chan_avg'] is True and c['pbmin'] == 0.0 and c['route'] == 'direct' and c['budget_bytes'] == 12345
    assert NP.array_equal(c['weights'], NP.transpose(full_w, (2, 0, 1))) and aps.image_stats['pb_eff'].shape == (1,)
    assert abs(band[0] - MC.FLUX) <= 1e-9 * MC.FLUX


def test_mosaic_marshals_a_beam_per_snapshot_where_the_pointing_moves(monkeypatch):
    pointings = [[90.0, 270.0], [80.0, 10.0], [65.0, 200.0]]
    ia = observed(monkeypatch, MC.GAUSS14, pointings)
    aps = RI.ApertureSynthesis(ia)
    aps.mosaic(MC.SOURCE_RADEC, coords='radec')
    c = MosaicOracleContext.calls[-1]
    assert c['beam_pc'].shape == (3, 3) and c['ext'] is None and c['beam_kind'] == _abi.PRISIM_BEAM_GAUSSIAN
    assert NP.allclose(c['beam_pc'], GEOM.altaz2dircos(NP.array(pointings), 'degrees'), atol=1e-15, rtol=0)
    # a phased array: one pb_info for all is one extension, one per snapshot is one beamformer per snapshot -- with another telescope
    # than the array's own
    mwa = {'id': 'mwa', 'latitude': LAT}
    one = {'pointing_center': NP.array([60.0, 40.0]), 'pointing_coords': 'altaz'}
    aps.mosaic(MC.SOURCE_RADEC, coords='radec', telescope=mwa, pb_info=one)
    c = MosaicOracleContext.calls[-1]
    want = PB.device_beam_spec(mwa, pointing_info=one, pointing_center=NP.array(pointings[0]), first_frequency_hz=float(CH[0]))
    assert c['beam_kind'] == _abi.PRISIM_BEAM_DIPOLE == want[0] and c['diameter'] == 0.74 and c['beam_pc'].shape == (3,)
    assert isinstance(c['ext'], dict) and RI._same_beam_spec(c['ext'], want[3]) and c['ext']['beamformer']['delays'].shape == (16, 1)
    per = [{'pointing_center': NP.array([60.0 + 5.0 * t, 40.0 * t]), 'pointing_coords': 'altaz'} for t in range(3)]
    aps.mosaic(MC.SOURCE_RADEC, coords='radec', telescope=mwa, pb_info=per)
    c = MosaicOracleContext.calls[-1]
    assert isinstance(c['ext'], list) and len(c['ext']) == 3 and c['beam_pc'].shape == (3,)
    for t in range(3):
        want = PB.device_beam_spec(mwa, pointing_info=per[t], pointing_center=NP.array(pointings[t]), first_frequency_hz=float(CH[0]))
        assert RI._same_beam_spec(c['ext'][t], want[3])
    assert not RI._same_beam_spec(c['ext'][0], c['ext'][1])
    with pytest.raises(ValueError, match='pb_info'):
        aps.mosaic(MC.SOURCE_RADEC, coords='radec', telescope=mwa, pb_info=per[:2])


def test_mosaic_refusals_and_the_resident_cube(monkeypatch):
    ia = observed(monkeypatch, MC.GAUSS14, [MC.ZENITH] * 3, reserve=True)
    aps = RI.ApertureSynthesis(ia)
    aps.mosaic(MC.SOURCE_RADEC, coords='radec')
    assert MosaicOracleContext.calls[-1]['cube'] is None and aps.image_stats['resident'] is True      # read where it lies
    n0 = len(MosaicOracleContext.calls)
    for bad in (-0.1, 1.0, NP.nan):
        with pytest.raises(ValueError, match='pbmin'):
            aps.mosaic(MC.SOURCE_RADEC, coords='radec', pbmin=bad)
    for shape in ('rect', 'square'):
        with pytest.raises(NotImplementedError, match='accelerated path'):
            aps.mosaic(MC.SOURCE_RADEC, coords='radec', telescope={'shape': shape, 'size': 14.0})
    with pytest.raises(ValueError, match='route'):
        aps.mosaic(MC.SOURCE_RADEC, coords='radec', route='fast')
    with pytest.raises(ValueError, match='coords'):
        aps.mosaic(MC.SOURCE_RADEC, coords='galactic')
    with pytest.raises(ValueError, match='weights'):
        aps.mosaic(MC.SOURCE_RADEC, coords='radec', weights=NP.ones(3))
    ia._extbeam = (NP.ones((12, 2)), NP.eye(2))                       # what set_external_beam leaves
    with pytest.raises(NotImplementedError, match='external beam'):
        aps.mosaic(MC.SOURCE_RADEC, coords='radec')
    ia._extbeam = None
    assert len(MosaicOracleContext.calls) == n0                       # nothing reached the device
    # image(), psf() and clean() keep their signatures
    import inspect
    assert list(inspect.signature(aps.image).parameters) == ['directions', 'coords', 'datakey', 'weights', 'chan_avg', 'epoch', 'route', 'budget_bytes']
    assert list(inspect.signature(aps.mosaic).parameters) == ['directions', 'coords', 'datakey', 'weights', 'chan_avg', 'epoch', 'telescope',
                                                              'pb_info', 'pbmin', 'route', 'budget_bytes']
    assert inspect.signature(aps.mosaic).parameters['pbmin'].default == 0.1
