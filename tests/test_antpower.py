"""CPU: the power an antenna receives from the sky (include/prisim_antpower.h) -- the planning header compiled alone under the
sanitizers, the export (tests/test_abi_headers.py holds the ctypes mirrors and the prototype to the header), the Python
function prisim_amd.interferometry.antenna_power against a stub context (exceptions, pointings, rotations, units, the choice of n_ext),
and the numpy checker (tests/antpower_checker.py) on a uniform sky."""
import os
import subprocess

import numpy as NP
import pytest

import antpower_checker as AK
from prisim_amd import _abi
from prisim_amd import frames as FRAMES
from prisim_amd import geometry as GEOM
from prisim_amd import interferometry as RI
from prisim_amd import skymodel as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PLAN_PROGRAM = r'''
#include "antpower_plan.h"

#include <cstdint>
#include <cstdio>
#include <vector>

using namespace pint;

int main() {
  long bad = 0, checked = 0;
  const int64_t srcs[] = {1, 255, 256, 257, 1537, 4097, 786432};
  const int64_t chans[] = {1, 2, 37, 64, 65, 300, 1024};
  const int64_t snaps[] = {1, 2, 8};
  const int64_t tiles[] = {int64_t(16) << 20, int64_t(64) << 20, int64_t(256) << 20};
  for (int64_t nsrc : srcs)
    for (int64_t nchan : chans) {
      const AntpowerShape sh = antpower_shape(nsrc, nchan);
      bool ok = sh.block == kAntpowerBlock && (sh.tile & (sh.tile - 1)) == 0 && sh.tile <= kAntpowerMaxChanTile &&
                (sh.tile >= nchan || sh.tile == kAntpowerMaxChanTile) && (sh.tile == 1 || sh.tile / 2 < nchan) &&
                sh.lanes * sh.tile == kAntpowerThreads && sh.nblocks * sh.block >= nsrc && (sh.nblocks - 1) * sh.block < nsrc &&
                sh.ntiles * sh.tile >= nchan && (sh.ntiles - 1) * sh.tile < nchan && sh.lds == kAntpowerThreads * 16;
      if (!ok) { std::printf("shape(%lld, %lld)\n", (long long)nsrc, (long long)nchan); ++bad; }
      ++checked;
      const int64_t per = antpower_source_bytes(nchan), part = antpower_partial_bytes(sh, nchan);
      const int64_t one = sh.block * (per + kAntpowerUnitBytes) + part;      // one block on one stream
      const int64_t budgets[] = {0, -5, 1000, one - 1, one, one + 1, 2 * (2 * sh.block * per + part) + 2 * sh.block * kAntpowerUnitBytes,
                                 3 * one + 12345, int64_t(1) << 30, int64_t(1) << 34};
      for (int64_t nsnap : snaps)
        for (int64_t tile_bytes : tiles)
          for (int64_t budget : budgets) {
            const AntpowerPlan p = antpower_plan(nsrc, nchan, nsnap, budget, tile_bytes, 2);
            const int64_t have = budget_or_default(budget), span = p.spans.size;
            // block, tile and lanes do not change with the budget, the streams or the size of pb_tile
            ok = p.shape.block == sh.block && p.shape.tile == sh.tile && p.shape.lanes == sh.lanes && p.shape.nblocks == sh.nblocks &&
                 p.shape.ntiles == sh.ntiles;
            ok = ok && p.ok == (have >= one);                               // a budget too small for one block is an error, no other is
            if (ok && p.ok) {
              ok = span >= sh.block && span % sh.block == 0 && span <= sh.nblocks * sh.block && p.nstreams >= 1 && p.nstreams <= 2 &&
                   p.nstreams <= nsnap && span / sh.block <= kAntpowerMaxGrid;
              // the buffers stay within the budget, pb_tile within its size (one block at least)
              ok = ok && p.buffer_bytes == p.nstreams * (span * per + part) + span * kAntpowerUnitBytes && p.buffer_bytes <= have;
              ok = ok && (span == sh.block || span * 8 * nchan <= tile_bytes);
              // the spans cover every source once, each a whole number of blocks but the last
              std::vector<int> seen((size_t)nsrc, 0);
              int64_t next = 0;
              for (int64_t k = 0; ok && k < p.spans.count; ++k) {
                const Span sp = p.spans.span(k, nsrc);
                ok = sp.first == next && sp.first % sh.block == 0 && sp.count >= 1 && (k == p.spans.count - 1 || sp.count == span) &&
                     sp.first + sp.count <= nsrc;
                for (int64_t s = sp.first; ok && s < sp.first + sp.count; ++s) ++seen[(size_t)s];
                next = sp.first + sp.count;
              }
              ok = ok && next == nsrc;
              for (int64_t s = 0; ok && s < nsrc; ++s) ok = seen[(size_t)s] == 1;
              // the largest such span: one block more is past the catalogue, pb_tile or the budget
              if (ok && span < sh.nblocks * sh.block && (span + sh.block) * 8 * nchan <= tile_bytes)
                ok = p.nstreams * ((span + sh.block) * per + part) + (span + sh.block) * kAntpowerUnitBytes > have;
            }
            if (!ok) {
              std::printf("plan(%lld, %lld, %lld, %lld, %lld): span %lld count %lld streams %d bytes %lld ok %d\n", (long long)nsrc,
                          (long long)nchan, (long long)nsnap, (long long)budget, (long long)tile_bytes, (long long)span,
                          (long long)p.spans.count, p.nstreams, (long long)p.buffer_bytes, (int)p.ok);
              ++bad;
            }
            ++checked;
          }
    }
  // the figures the documents quote: an nside-256 sky of 1024 channels goes in 96 spans of 8192 sources, 3072 blocks, 4 lanes
  const AntpowerPlan c5 = antpower_plan(786432, 1024, 8, 0, kAntpowerPbTileBytes, 2);
  if (!c5.ok || c5.spans.size != 8192 || c5.spans.count != 96 || c5.shape.nblocks != 3072 || c5.shape.tile != 64 || c5.shape.lanes != 4 ||
      c5.nstreams != 2)
    ++bad;
  // the budgets tests/test_gpu_antpower.py gives: four spans of 512 on two streams, seven of one block on one
  const AntpowerPlan a = antpower_plan(1537, 37, 5, 2 * (512 * (32 + 8 * 37) + 7 * 2 * 37 * 8) + 512 * 16, kAntpowerPbTileBytes, 2);
  const AntpowerPlan b = antpower_plan(1537, 37, 5, 256 * (32 + 8 * 37) + 7 * 2 * 37 * 8 + 256 * 16, kAntpowerPbTileBytes, 2);
  if (a.spans.size != 512 || a.spans.count != 4 || a.nstreams != 2 || b.spans.size != 256 || b.spans.count != 7 || b.nstreams != 1) ++bad;
  checked += 2;
  std::printf("checked %ld bad %ld\n", checked, bad);
  return bad ? 1 : 0;
}
'''


def test_plan_header_compiles_alone_and_plans_soundly(tmp_path):
    src = tmp_path / 'antpower_plan_check.cpp'
    src.write_text(PLAN_PROGRAM)
    exe = tmp_path / 'antpower_plan_check'
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-Wall', '-Werror', '-fsanitize=address,undefined', '-I',
                           os.path.join(ROOT, 'prisim_amd', 'csrc_addon'), str(src), '-o', str(exe)])
    res = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = res.stdout.decode()
    assert res.returncode == 0, out
    assert out.strip().splitlines()[-1] == 'checked %d bad 0' % (7 * 7 * (1 + 3 * 3 * 10) + 2), out
    txt = open(os.path.join(ROOT, 'prisim_amd', 'csrc_addon', 'antpower_plan.h')).read()
    assert '#include <hip' not in txt and '__device__' not in txt and '#include "addon_internal.h"' not in txt


def test_export_is_in_the_library_and_outside_the_core_abi():
    lib = _abi.load_library()
    assert 'prisim_antenna_power' not in _abi.EXPORTS
    assert lib.prisim_antenna_power(None, None, None, None, None, None) == _abi.PRISIM_EINVAL       # a null context is refused, not read
    # the struct lives on the class: the module's Prisim*Stats names are pinned by tests/test_abi_helpers.py
    assert not hasattr(_abi, 'PrisimAntpowerStats') and 'reserved_' not in _abi._stats_dict(_abi.Context.PrisimAntpowerStats())
    src = open(os.path.join(ROOT, 'prisim_amd', 'csrc_antpower', 'antpower.hip')).read()
    assert 'atomic' not in src.replace('No atomics', '').replace('no atomic', '')
    header = open(os.path.join(ROOT, 'include', 'prisim_antpower.h')).read()
    assert 'prisim_hip_' not in header.replace('prisim_hip.h', '').replace('prisim_hip_last_error', '').replace('prisim_hip_set_sky_analytic', '')


# ---- the Python function against a stub context -------------------------------------------------------------------------------------

class StubContext(object):
    """Context.antenna_power on the host: records what it was handed and returns a power that names the snapshot and the channel."""
    calls = []

    def __init__(self, device=0):
        self.device = device

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def antenna_power(self, unitvec, freqs_hz, cel2enu, beam_kind, diameter_m, **kw):
        call = dict(kw, unitvec=NP.array(unitvec), freqs_hz=NP.array(freqs_hz), cel2enu=NP.array(cel2enu), beam_kind=beam_kind,
                    diameter_m=diameter_m, device=self.device)
        StubContext.calls.append(call)
        nsnap, nchan = call['cel2enu'].reshape(-1, 9).shape[0], call['freqs_hz'].size
        power = 100.0 * NP.arange(nsnap)[:, None] + NP.arange(nchan)[None, :]
        return power, None, None, {'spans': 1, 'streams': 1}


@pytest.fixture
def stub(monkeypatch):
    StubContext.calls = []
    monkeypatch.setattr(RI._abi, 'Context', StubContext)
    return StubContext


LAT = -30.7215
RADEC = NP.array([[10.0, -30.0], [200.0, 15.0], [359.0, -80.0]])
FREQS = NP.array([100e6, 150e6, 200e6])


def spectrum_model(location=RADEC):
    return SM.SkyModel(location=location, frequency=FREQS, spectrum=NP.arange(9.0).reshape(3, 3) + 1.0)


def func_model():
    return SM.SkyModel(location=RADEC, flux_ref=[1.0, 2.0, 3.0], spindex=[-0.7, -0.8, 0.0], ref_freq=150.0)


def test_python_argument_checks(stub):
    sky, tel = spectrum_model(), {'id': 'hera'}
    with pytest.raises(TypeError, match='telescope_info must be a dictionary'):
        RI.antenna_power(sky, ['hera'], {'lst': [0.0]})
    with pytest.raises(TypeError, match='pointing_info must be a dictionary'):
        RI.antenna_power(sky, tel, [0.0])
    with pytest.raises(TypeError, match='SkyModel'):
        RI.antenna_power(RADEC, tel, {'lst': [0.0]})
    with pytest.raises(KeyError, match='lst'):
        RI.antenna_power(sky, tel, {})
    with pytest.raises(KeyError, match='pointing_coords'):
        RI.antenna_power(sky, tel, {'lst': [0.0], 'pointing_center': NP.array([[90.0, 270.0]])})
    with pytest.raises(TypeError, match='must be a numpy array'):
        RI.antenna_power(sky, tel, {'lst': [0.0], 'pointing_center': [[90.0, 270.0]], 'pointing_coords': 'altaz'})
    with pytest.raises(ValueError, match='cannot exceed two dimensions'):
        RI.antenna_power(sky, tel, {'lst': [0.0], 'pointing_center': NP.zeros((1, 1, 2)), 'pointing_coords': 'altaz'})
    with pytest.raises(ValueError, match='3-column array'):
        RI.antenna_power(sky, tel, {'lst': [0.0], 'pointing_center': NP.array([[0.0, 1.0]]), 'pointing_coords': 'dircos'})
    for pc_coords in ('radec', 'hadec', 'altaz'):
        with pytest.raises(ValueError, match='2-column array'):
            RI.antenna_power(sky, tel, {'lst': [0.0], 'pointing_center': NP.array([[0.0, 0.0, 1.0]]), 'pointing_coords': pc_coords})
    with pytest.raises(ValueError, match='must match'):
        RI.antenna_power(sky, tel, {'lst': [0.0, 1.0, 2.0], 'pointing_center': NP.array([[80.0, 0.0], [70.0, 0.0]]), 'pointing_coords': 'altaz'})
    with pytest.raises(ValueError, match='frequency='):
        RI.antenna_power(func_model(), tel, {'lst': [0.0]})
    with pytest.raises(ValueError, match='coords must be'):
        RI.antenna_power(sky, tel, {'lst': [0.0]}, coords='galactic')
    with pytest.raises(ValueError, match='one .* per LST'):
        RI.antenna_power(sky, tel, {'lst': [0.0, 1.0]}, frames=[(NP.eye(3), NP.zeros(3))])
    with pytest.raises(NotImplementedError):
        RI.antenna_power(sky, {'shape': 'rect', 'size': [3.0, 4.0]}, {'lst': [0.0]})
    assert stub.calls == []                                           # nothing reached the device


def test_python_defaults_and_what_reaches_the_entry(stub):
    lst = NP.array([0.0, 73.1, 146.2])
    st = {}
    out = RI.antenna_power(spectrum_model(), {'id': 'hera'}, {'lst': lst}, device=3, budget_bytes=12345, stats=st)
    assert out.shape == (3, 3) and NP.array_equal(out, 100.0 * NP.arange(3)[:, None] + NP.arange(3)[None, :]) and st == {'spans': 1, 'streams': 1}
    (call,) = stub.calls
    assert call['device'] == 3 and call['budget_bytes'] == 12345 and call['want_sums'] is False
    assert call['beam_kind'] == _abi.PRISIM_BEAM_AIRY and call['diameter_m'] == 14.0 and call['ext'] is None
    assert NP.array_equal(call['beam_pc_dircos'], [0.0, 0.0, 1.0]) and call['aberr_beta'] is None
    assert NP.array_equal(call['freqs_hz'], FREQS)                  # no freq_scale: Hz
    assert NP.array_equal(call['flux_spectrum'], NP.arange(9.0).reshape(3, 3) + 1.0) and 'flux_ref' not in call
    assert NP.array_equal(call['unitvec'], GEOM.catalog_unitvec(RADEC, 'radec'))
    # the default latitude is the MWA's, and the rotations are hadec2altaz of (LST - RA, Dec) on three directions to 1e-15
    assert call['cel2enu'].shape == (3, 3, 3)
    for t, l in enumerate(lst):
        want = AK.altaz2dircos(AK.hadec2altaz(NP.stack((l - RADEC[:, 0], RADEC[:, 1]), axis=1), -26.701))
        assert NP.max(NP.abs(call['cel2enu'][t].dot(call['unitvec'].T).T - want)) <= 1e-15
    RI.antenna_power(spectrum_model(), {'id': 'hera', 'latitude': LAT}, {'lst': lst})
    want = AK.altaz2dircos(AK.hadec2altaz(NP.stack((lst[1] - RADEC[:, 0], RADEC[:, 1]), axis=1), LAT))
    assert NP.max(NP.abs(stub.calls[-1]['cel2enu'][1].dot(stub.calls[-1]['unitvec'].T).T - want)) <= 1e-15


def test_python_sky_frames(stub):
    tel, pinfo = {'id': 'hera', 'latitude': LAT}, {'lst': [5.0, 50.0]}
    RI.antenna_power(spectrum_model(), tel, pinfo, coords='hadec')
    call = stub.calls[-1]
    want = AK.altaz2dircos(AK.hadec2altaz(RADEC, LAT))
    for t in range(2):
        assert NP.max(NP.abs(call['cel2enu'][t].dot(call['unitvec'].T).T - want)) <= 1e-15
    altaz = NP.array([[10.0, 20.0], [80.0, 300.0], [45.0, 45.0]])
    RI.antenna_power(spectrum_model(altaz), tel, pinfo, coords='altaz')
    call = stub.calls[-1]
    assert NP.array_equal(call['cel2enu'], NP.stack([NP.eye(3)] * 2)) and NP.array_equal(call['unitvec'], GEOM.altaz2dircos(altaz))

    class Dircos(object):                                            # a model whose locations are direction cosines, and which says so
        coords, spec_type, frequency = 'dircos', 'spectrum', FREQS
        location = GEOM.altaz2dircos(altaz)

        def generate_spectrum(self, frequency=None, interp_method=None):
            return NP.ones((3, 3))

    RI.antenna_power(Dircos(), tel, pinfo)
    call = stub.calls[-1]
    assert NP.array_equal(call['cel2enu'], NP.stack([NP.eye(3)] * 2)) and NP.array_equal(call['unitvec'], GEOM.altaz2dircos(altaz))
    frames = [FRAMES.snapshot_frame('radec', l, LAT, jd=2461333.5, epoch='J2000', model='apparent') for l in pinfo['lst']]
    RI.antenna_power(spectrum_model(), tel, pinfo, frames=frames)
    call = stub.calls[-1]
    assert NP.array_equal(call['cel2enu'], NP.stack([f[0] for f in frames])) and NP.array_equal(call['aberr_beta'], NP.stack([f[1] for f in frames]))
    assert NP.max(NP.abs(call['aberr_beta'])) > 1e-5


def test_python_units_and_power_laws(stub):
    tel, pinfo = {'shape': 'dish', 'size': 14.0}, {'lst': [0.0]}
    RI.antenna_power(func_model(), tel, pinfo, freq_scale='MHz', frequency=[100.0, 150.0, 200.0])
    call = stub.calls[-1]
    assert NP.array_equal(call['freqs_hz'], FREQS) and call['ref_freq_hz'] == 150e6 and 'flux_spectrum' not in call
    assert NP.array_equal(call['flux_ref'], [1.0, 2.0, 3.0]) and NP.array_equal(call['spindex'], [-0.7, -0.8, 0.0])
    assert call['beam_kind'] == _abi.PRISIM_BEAM_AIRY and call['diameter_m'] == 14.0
    for scale, factor in (('GHz', 1e9), ('kHz', 1e3), ('Hz', 1.0), (None, 1.0)):
        RI.antenna_power(func_model(), tel, pinfo, freq_scale=scale, frequency=[0.1, 0.15, 0.2])
        assert NP.array_equal(stub.calls[-1]['freqs_hz'], NP.array([0.1, 0.15, 0.2]) * factor)
        assert stub.calls[-1]['ref_freq_hz'] == 150.0 * factor
    # the polynomial beams take their band from the first frequency in Hz
    RI.antenna_power(func_model(), {'id': 'vla'}, pinfo, freq_scale='GHz', frequency=[1.4, 1.5])
    assert stub.calls[-1]['beam_kind'] == _abi.PRISIM_BEAM_POLY and NP.array_equal(stub.calls[-1]['ext']['poly'][:3], [-1.343, 6.579, -1.186])


def test_python_pointings_and_the_choice_of_n_ext(stub):
    lst = NP.array([20.0, 95.0, 170.0])
    tel = {'id': 'mwa', 'latitude': LAT}
    sky = spectrum_model()
    pos = RI.PB.mwa_tile_element_locs()

    def delays_for(altaz):
        return pos.dot(GEOM.altaz2dircos(NP.asarray(altaz, dtype=NP.float64).reshape(1, 2)).T) / 299792458.0

    # no pointing centre: the zenith, alt-az [90, 270], at every LST -- one shared ext, a beamformer with the zenith's (zero) delays
    RI.antenna_power(sky, tel, {'lst': lst})
    ext = stub.calls[-1]['ext']
    assert isinstance(ext, dict) and NP.allclose(ext['beamformer']['delays'], delays_for([90.0, 270.0]), rtol=0, atol=1e-25)
    assert NP.max(NP.abs(ext['beamformer']['delays'])) < 1e-23
    # one alt-az row is repeated: still one ext
    RI.antenna_power(sky, tel, {'lst': lst, 'pointing_center': NP.array([60.0, 130.0]), 'pointing_coords': 'altaz'})
    ext = stub.calls[-1]['ext']
    assert isinstance(ext, dict) and NP.array_equal(ext['beamformer']['delays'], delays_for([60.0, 130.0]))
    # a tracked (RA, Dec): converted with LST - RA, other delays at every LST, one ext per LST
    RI.antenna_power(sky, tel, {'lst': lst, 'pointing_center': NP.array([[95.0, LAT + 5.0]]), 'pointing_coords': 'radec'})
    ext = stub.calls[-1]['ext']
    assert isinstance(ext, list) and len(ext) == 3
    altaz = AK.hadec2altaz(NP.stack((lst - 95.0, NP.full(3, LAT + 5.0)), axis=1), LAT)
    for t in range(3):
        assert NP.allclose(ext[t]['beamformer']['delays'], delays_for(altaz[t]), rtol=0, atol=1e-22)
    assert not NP.array_equal(ext[0]['beamformer']['delays'], ext[1]['beamformer']['delays'])
    # (HA, Dec) and direction cosines, one row per LST
    hadec = NP.array([[-20.0, -25.0], [0.0, -30.0], [30.0, -40.0]])
    RI.antenna_power(sky, tel, {'lst': lst, 'pointing_center': hadec, 'pointing_coords': 'hadec'})
    ext = stub.calls[-1]['ext']
    for t in range(3):
        assert NP.allclose(ext[t]['beamformer']['delays'], delays_for(AK.hadec2altaz(hadec[t:t + 1], LAT)[0]), rtol=0, atol=1e-22)
    dircos = GEOM.altaz2dircos(NP.array([[80.0, 10.0], [70.0, 100.0], [60.0, 190.0]]))
    RI.antenna_power(sky, tel, {'lst': lst, 'pointing_center': dircos, 'pointing_coords': 'dircos'})
    ext = stub.calls[-1]['ext']
    for t in range(3):
        assert NP.allclose(ext[t]['beamformer']['delays'], pos.dot(dircos[t:t + 1].T) / 299792458.0, rtol=0, atol=1e-22)
    # dishes do not follow the pointing: one shared description, pointed where telescope_info says
    RI.antenna_power(sky, {'id': 'hera'}, {'lst': lst, 'pointing_center': hadec, 'pointing_coords': 'hadec'})
    assert stub.calls[-1]['ext'] is None and NP.array_equal(stub.calls[-1]['beam_pc_dircos'], [0.0, 0.0, 1.0])


# ---- the checker itself ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('setup', [{'element': 'delta'}, {'element': 'gaussian', 'size': 14.0}, {'element': 'dish', 'size': 14.0},
                                   {'element': 'dipole', 'size': 0.74, 'element_dircos': (1.0, 0.0, 0.0), 'ground': {'height': 0.3, 'modifier': None}}])
def test_checker_returns_the_temperature_of_a_uniform_sky(setup):
    rng = NP.random.default_rng(3)
    n, T = 800, 3.0e2 / 7.0
    radec = NP.stack((rng.uniform(0.0, 360.0, n), NP.degrees(NP.arcsin(rng.uniform(-1.0, 1.0, n)))), axis=1)
    freqs = NP.linspace(100e6, 200e6, 9)
    dircos = AK.sky_dircos(radec, 'radec', [0.0, 120.0], LAT)
    ref = AK.antenna_power(dircos, NP.full((n, 9), T), lambda t, dc: AK.beam_of(setup, freqs)(dc))
    assert NP.all(ref['den'] > 0.0) and NP.all(ref['n_up'] > 300)
    assert NP.all(NP.abs(ref['power'] - T) <= ref['n_up'][:, None] * 2.0 ** -53 * T)
    assert NP.allclose(ref['abs_flux'], ref['n_up'][:, None] * T) and NP.allclose(ref['abs_num'], ref['num'])
    # the frames' route gives the same directions as the route through alt-az, whose arcsin and arctan2 in degrees cost a few more
    # roundings (each component is of order one: 45 units in the last place)
    rot = NP.stack([FRAMES.equatorial_to_enu(l, LAT) for l in (0.0, 120.0)])
    assert NP.max(NP.abs(AK.frame_dircos(GEOM.catalog_unitvec(radec, 'radec'), rot, None) - dircos)) <= 1e-14
    empty = AK.antenna_power(dircos[:, :1] * NP.array([1.0, 1.0, -1.0]) * NP.sign(dircos[:, :1, 2:3]), NP.ones((1, 9)), lambda t, dc: AK.beam_of(setup, freqs)(dc))
    assert NP.all(NP.isnan(empty['power'])) and NP.all(empty['num'] == 0.0) and NP.all(empty['n_up'] == 0)
