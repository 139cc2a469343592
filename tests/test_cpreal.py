"""CPU: closure phases of noise realisations (include/prisim_cpreal.h) -- the planning header compiled alone, the ctypes mirror of
prisim_cpreal_stats against the compiled header, the selection of triads by a baseline triplet on the HERA-19 layout, the class
surface (InterferometerArray.closure_phase_realizations, bispectrum_phase.simulate_closure_phases) against a stub context that closes
known noise cubes with the numpy checker (tests/cpreal_checker.py), and the refusals of the Python layer."""
import os
import subprocess
import types

import numpy as NP
import pytest

import closure_checker as CK
import cpreal_checker as RK
from prisim_amd import _abi
from prisim_amd import bispectrum_phase as BP
from prisim_amd import interferometry as RI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = NP.load(os.path.join(ROOT, 'tests', 'golden', 'golden_closure.npz'))

PLAN_PROGRAM = r'''
#include "cpreal_plan.h"

#include <cstdint>
#include <cstdio>
#include <vector>

using namespace pint;

int main() {
  long bad = 0, checked = 0;
  const int64_t limits[] = {65536, 163840, 1000, 127, 128};
  const int64_t rows[] = {1, 7, 8, 9, 62, 63, 64, 640, 641, 1280, 1281, 4095, 4096, 4097, 10240, 10241, 12000};
  const int64_t chans[] = {1, 4, 7, 8, 9, 16, 37, 63, 64, 65, 1024};
  for (int64_t lds_max : limits)
    for (int64_t nrow : rows) {
      const bool fits = nrow * 16 * kCprealMinTile <= lds_max;
      // AUTO is STAGED exactly when the narrowest tile fits; an explicit STAGED that does not fit is refused
      if (cpreal_route(-1, nrow, lds_max) != (fits ? kCprealStaged : kCprealDirect)) { std::printf("auto %lld %lld\n", (long long)nrow, (long long)lds_max); ++bad; }
      if (cpreal_route(kCprealStaged, nrow, lds_max) != (fits ? kCprealStaged : -1)) ++bad;
      if (cpreal_route(kCprealDirect, nrow, lds_max) != kCprealDirect) ++bad;
      checked += 3;
      for (int64_t nchan : chans) {
        const CprealTile t = cpreal_tile(nrow, nchan, lds_max);
        bool ok;
        if (!fits) ok = t.tile == 0 && t.lds == 0;
        else
          ok = t.tile >= kCprealMinTile && t.tile <= kCprealMaxTile && (t.tile & (t.tile - 1)) == 0 && t.lds == nrow * 16 * t.tile &&
               t.lds <= lds_max && t.ntiles * t.tile >= nchan && (t.ntiles - 1) * t.tile < nchan &&
               (t.tile == kCprealMinTile || (t.tile <= nchan && t.lds <= kTileLds)) &&
               // the widest such tile: the next one is past the band, the maximum or the LDS
               (t.tile == kCprealMaxTile || 2 * t.tile > nchan || 2 * t.lds > std::min<int64_t>(lds_max, kTileLds)) &&
               (t.threads == 256 || t.threads == 512 || t.threads == 1024) && (163840 / t.lds) * (int64_t)t.threads >= 1024;
        if (!ok) {
          std::printf("tile(%lld, %lld, %lld): {%lld, %lld, %lld, %d}\n", (long long)nrow, (long long)nchan, (long long)lds_max,
                      (long long)t.tile, (long long)t.ntiles, (long long)t.lds, t.threads);
          ++bad;
        }
        ++checked;
      }
    }
  // the chunks of (snapshot, realisation) pairs cover every pair exactly once, within the budget and the grid
  const int64_t pairs[] = {1, 2, 5, 15, 97, 2048, 100000};
  const int64_t bytes[] = {8, 2072, int64_t(1) << 20, int64_t(3) << 30};
  const int64_t budgets[] = {0, 1, 2 * 2072, 2 * 5 * 2072 + 17, int64_t(1) << 30};
  const int64_t blocks[] = {0, 1, 5, 1000, int64_t(1) << 17};
  for (int64_t n : pairs)
    for (int64_t per : bytes)
      for (int64_t budget : budgets)
        for (int64_t bpp : blocks) {
          const int64_t max_blocks = int64_t(1) << 20;
          const Chunks c = cpreal_chunks(n, per, budget, bpp, max_blocks, 2);
          std::vector<int> seen((size_t)n, 0);
          bool ok = c.count >= 1 && c.size >= 1 && c.nstreams >= 1 && c.nstreams <= 2 && c.nstreams <= c.count;
          int64_t next = 0;
          for (int64_t k = 0; ok && k < c.count; ++k) {
            const Span sp = c.span(k, n);
            ok = sp.first == next && sp.count >= 1 && sp.count <= c.size && sp.first + sp.count <= n && (k == c.count - 1 || sp.count == c.size);
            for (int64_t p = sp.first; ok && p < sp.first + sp.count; ++p) ++seen[(size_t)p];
            next = sp.first + sp.count;
          }
          ok = ok && next == n && c.last == n - (c.count - 1) * c.size;
          for (int64_t p = 0; ok && p < n; ++p) ok = seen[(size_t)p] == 1;
          // one pair is always taken; beyond that the buffers of both streams stay within the budget and the grid within max_blocks
          if (ok && c.size > 1) ok = 2 * c.size * per <= budget_or_default(budget) && c.size * bpp <= max_blocks;
          if (!ok) {
            std::printf("chunks(%lld, %lld, %lld, %lld): {%lld, %lld, %lld, %d}\n", (long long)n, (long long)per, (long long)budget,
                        (long long)bpp, (long long)c.size, (long long)c.count, (long long)c.last, c.nstreams);
            ++bad;
          }
          ++checked;
        }
  // the figures the documents quote: 8 channels of 1280 rows fill the 160 KiB of gfx950, one row more goes direct
  const CprealTile full = cpreal_tile(1280, 1024, 163840);
  if (full.tile != 8 || full.lds != 163840 || full.threads != 1024 || cpreal_route(-1, 1281, 163840) != kCprealDirect) ++bad;
  const CprealTile small = cpreal_tile(9, 37, 163840);
  if (small.tile != 32 || small.ntiles != 2 || small.lds != 9 * 16 * 32 || small.threads != 256) ++bad;
  checked += 2;
  std::printf("checked %ld bad %ld\n", checked, bad);
  return bad ? 1 : 0;
}
'''


def test_plan_header_compiles_alone_and_plans_soundly(tmp_path):
    src = tmp_path / 'cpreal_plan_check.cpp'
    src.write_text(PLAN_PROGRAM)
    exe = tmp_path / 'cpreal_plan_check'
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-Wall', '-Werror', '-fsanitize=address,undefined', '-I',
                           os.path.join(ROOT, 'prisim_amd', 'csrc_addon'), str(src), '-o', str(exe)])
    res = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = res.stdout.decode()
    assert res.returncode == 0, out
    assert out.strip().splitlines()[-1] == 'checked %d bad 0' % (5 * 17 * (3 + 11) + 7 * 4 * 5 * 5 + 2), out
    txt = open(os.path.join(ROOT, 'prisim_amd', 'csrc_addon', 'cpreal_plan.h')).read()
    assert '#include <hip' not in txt and '__device__' not in txt and '#include "addon_internal.h"' not in txt


def test_kinds_are_the_enumerators():
    assert _abi.CPREAL_KINDS == {'noisy': _abi.PRISIM_CPREAL_NOISY, 'noise': _abi.PRISIM_CPREAL_NOISE}


# ---- the selection of triads by a baseline triplet ------------------------------------------------------------------------------

def layout_of(pos):
    return {'positions': pos, 'labels': NP.array([str(i) for i in range(len(pos))]), 'ids': NP.arange(len(pos)), 'coords': 'ENU'}


def hera19_standin(**attrs):
    s = types.SimpleNamespace(layout=layout_of(GOLD['hera19_pos']), baselines=GOLD['hera19_bl'],
                              labels=[tuple(x) for x in GOLD['hera19_labels'].tolist()], bl_reversemap=None, **attrs)
    for name in ('getThreePointCombinations', 'closure_leg_table', 'getClosurePhase', 'closure_phase_realizations', '_thermal_rms'):
        setattr(s, name, types.MethodType(getattr(RI.InterferometerArray, name), s))
    return s


EQUILATERAL = 14.6 * NP.array([[1.0, 0.0, 0.0], [-0.5, NP.sqrt(0.75), 0.0], [-0.5, -NP.sqrt(0.75), 0.0]])


def test_triads_of_bltriplet_on_hera19():
    s = hera19_standin()
    all_ant, all_vec = s.getThreePointCombinations(unique=False)
    matches = NP.array([RK.triplet_matches(v, EQUILATERAL, 0.1) for v in all_vec])
    assert 0 < matches.sum() < len(all_ant)
    for triplet in (EQUILATERAL, -EQUILATERAL, EQUILATERAL * NP.array([[1.0], [-1.0], [1.0]]), EQUILATERAL[[2, 0, 1]]):
        triads, vec = BP.triads_of_bltriplet(s, triplet, blltol=0.1)
        assert triads.shape == (vec.shape[0], 3) and vec.shape[1:] == (3, 3)
        want = [tuple(str(a) for a in t) for t, m in zip(all_ant, matches) if m]
        assert [tuple(t) for t in triads.tolist()] == want             # only triads whose three vectors match, in either sign, and all of them
        assert NP.array_equal(vec, NP.asarray(all_vec, dtype=NP.float64)[matches])
        assert NP.allclose(NP.sqrt(NP.sum(vec ** 2, axis=2)), 14.6, atol=0.1)
    with pytest.raises(ValueError, match='not found in the model triads'):
        BP.triads_of_bltriplet(s, NP.array([[100.0, 0.0, 0.0], [0.0, 100.0, 0.0], [-100.0, -100.0, 0.0]]))
    # every row is a baseline of the array, and no triad holds all three
    with pytest.raises(ValueError, match='Specified triad not found'):
        BP.triads_of_bltriplet(s, NP.array([[14.6, 0.0, 0.0], [29.2, 0.0, 0.0], [58.4, 0.0, 0.0]]))
    with pytest.raises(TypeError):
        BP.triads_of_bltriplet(s, EQUILATERAL.tolist())
    with pytest.raises(ValueError, match='three baseline vectors'):
        BP.triads_of_bltriplet(s, EQUILATERAL[:2])


# ---- the class surface against a stub context -------------------------------------------------------------------------------------

class StubContext(object):
    """closure_realizations and closure_phase on the host: the noise of realisation r is a numpy draw keyed on its seed and on the
    global baseline of each row, closed by the checkers.  Records what it was handed."""

    def __init__(self):
        self.calls = []

    @staticmethod
    def noise(seed, glob, nt, nchan, rms):
        out = NP.empty((nt, len(glob), nchan), dtype=NP.complex128)
        for i, g in enumerate(glob):
            rng = NP.random.default_rng([int(seed), int(g)])
            out[:, i, :] = rng.standard_normal((nt, nchan)) + 1j * rng.standard_normal((nt, nchan))
        return out * rms * NP.sqrt(0.5)

    def closure_realizations(self, cube, cube_row, bl_global, rms, bpwts, legs, conj, seed, n_realize, first=0, kind='noisy', nt=None,
                             route='auto', budget_bytes=None):
        self.calls.append({'cube': cube, 'cube_row': cube_row, 'bl_global': NP.asarray(bl_global), 'rms': rms, 'bpwts': bpwts, 'legs': legs,
                           'conj': conj, 'seed': seed, 'first': first, 'kind': kind, 'nt': nt, 'route': route})
        nt, nrow, nchan = rms.shape
        noise = NP.stack([self.noise(seed + first + r, bl_global, nt, nchan, rms) for r in range(n_realize)])
        phases, _ = RK.closure_realizations(cube, noise, bpwts, legs, conj, kind=kind)
        return phases, {'route': 'stub', 'pairs': nt * n_realize}

    def closure_phase(self, cube, legs, conj, bpwts, freq_wts=None, masks=None, mask_index=None, nt=None, route='auto'):
        trip, ph = CK.closure_phase(cube, legs, conj, bpwts, NP.ones_like(bpwts))
        return trip, ph, {'route': 'stub'}


NT, NCHAN = 3, 6


def simulated_standin(ctx):
    rng = NP.random.default_rng(3)
    nbl = GOLD['hera19_bl'].shape[0]
    sky = rng.standard_normal((nbl, NCHAN, NT)) + 1j * rng.standard_normal((nbl, NCHAN, NT))
    return hera19_standin(channels=150e6 + 1e5 * NP.arange(NCHAN), freq_resolution=1e5, gaininfo=None, skyvis_freq=sky, vis_freq=None,
                          vis_noise_freq=None, vis_rms_freq=None, _cube=[sky[:, :, t] for t in range(NT)], _device_in_step=False, _reserved=0,
                          bp=rng.uniform(0.5, 1.0, (nbl, NCHAN, NT)), bp_wts=NP.ones((nbl, NCHAN, 1)), baseline_lengths=None,
                          timestamp=[2457000.5 + 0.01 * t for t in range(NT)], lst=NP.array([30.0, 30.25, 30.5]),
                          eff_Q=NP.ones((nbl, NCHAN)), A_eff=NP.full((nbl, NCHAN), 150.0), t_acc=[10.7] * NT,
                          Tsys=rng.uniform(150.0, 250.0, (nbl, NCHAN, NT)), flux_unit='JY', _ctx=ctx)


def test_class_method_compacts_the_rows_and_returns_the_stack():
    ctx = StubContext()
    s = simulated_standin(ctx)
    triads, _ = BP.triads_of_bltriplet(s, EQUILATERAL)
    few = [tuple(t) for t in triads[::9].tolist()]
    res = s.closure_phase_realizations(4, 10, antenna_triplets=few, datakey=['noisy', 'noise'], n_avg=4, first=2)
    assert set(res) == {'closure_phase_vis', 'closure_phase_noise', 'antenna_triplets', 'baseline_triplets', 'seeds'}
    assert res['seeds'].dtype == NP.uint64 and res['seeds'].tolist() == [12, 13, 14, 15]
    assert set(s.cpreal_stats) == {'noisy', 'noise'} and [c['kind'] for c in ctx.calls] == ['noisy', 'noise']
    assert s.vis_freq is None and s.vis_noise_freq is None and s.vis_rms_freq is None       # untouched
    legs, conj, vec = s.closure_leg_table(few)
    assert NP.array_equal(NP.asarray(vec), NP.asarray(res['baseline_triplets']))
    used = NP.unique(legs)
    call = ctx.calls[0]
    assert 3 <= used.size < 3 * len(few) and NP.array_equal(call['bl_global'], used) and call['cube_row'] is None
    assert NP.array_equal(used[call['legs']], legs) and NP.array_equal(call['conj'], conj)
    rms = s._thermal_rms()
    assert NP.array_equal(call['rms'], NP.transpose(rms[used] / 2.0, (2, 0, 1)))           # sqrt(n_avg) = 2
    assert NP.array_equal(call['cube'], NP.transpose(s.skyvis_freq[used], (2, 0, 1)))
    assert NP.array_equal(call['bpwts'], NP.transpose((s.bp * s.bp_wts)[used], (2, 0, 1)))
    # the stack is what the per-realisation chain gives on full cubes: noise of every baseline, then the closure phases
    nbl = s.baselines.shape[0]
    full_rms = NP.transpose(NP.broadcast_to(rms, (nbl, NCHAN, NT)) / 2.0, (2, 0, 1))
    for r in range(4):
        noise = NP.transpose(StubContext.noise(12 + r, NP.arange(nbl), NT, NCHAN, full_rms), (1, 2, 0))
        for key, cube in (('closure_phase_vis', s.skyvis_freq + noise), ('closure_phase_noise', noise)):
            _, ph = CK.closure_phase(cube, legs, conj, s.bp, s.bp_wts)
            assert res[key].shape == (NT, 4, len(few), NCHAN)
            assert RK.phase_deviation(res[key][:, r], NP.transpose(ph, (2, 0, 1))).max() <= 32 * 2.0 ** -53
    # a sharded run: the draws are keyed on the global index
    glob = 1000 + 3 * NP.arange(nbl)
    s.closure_phase_realizations(1, 10, antenna_triplets=few, bl_index=glob)
    assert NP.array_equal(ctx.calls[-1]['bl_global'], glob[used])


def test_simulate_closure_phases_gives_loadnpz_dictionaries(tmp_path):
    ctx = StubContext()
    s = simulated_standin(ctx)
    nreal = 5
    prefix = str(tmp_path / 'model')
    out = BP.simulate_closure_phases(s, nreal, 21, bltriplet=EQUILATERAL, datakey=['noiseless', 'noisy', 'noise'], outfile_prefix=prefix)
    triads, _ = BP.triads_of_bltriplet(s, EQUILATERAL)
    ntriads = len(triads)
    assert list(out) == ['noiseless', 'noisy', 'noise']
    for key, d in out.items():
        raw = d['raw']
        assert list(d) == ['raw'] and set(raw) == {'cphase', 'triads', 'flags', 'lst', 'lst-day', 'days'}
        assert raw['cphase'].shape == raw['flags'].shape == (NT, nreal, ntriads, NCHAN)
        assert raw['cphase'].dtype == NP.float64 and raw['flags'].dtype == bool and not raw['flags'].any()
        assert raw['triads'].shape == (ntriads, 3) and NP.array_equal(raw['triads'], triads.astype(str))
        assert raw['lst'].shape == raw['lst-day'].shape == (NT, nreal) and raw['days'].shape == (nreal,) and raw['days'].dtype == NP.float64
        assert NP.allclose(raw['lst'], (s.lst / 15.0).reshape(-1, 1), rtol=0, atol=1e-12)
        assert NP.array_equal(raw['days'], s.timestamp[0] + NP.arange(nreal))
        # the file holds the reference's five arrays, and loadnpz reads it back to the returned dictionary
        fname = '%s_%s.npz' % (prefix, key)
        with NP.load(fname) as f:
            assert set(f.files) == {'closures', 'flags', 'triads', 'last', 'days'}
            assert f['closures'].shape == f['flags'].shape == (NT, nreal, ntriads, NCHAN) and f['last'].shape == (NT, nreal)
            assert NP.array_equal(f['last'], (s.lst / 15.0 / 24.0).reshape(-1, 1) + NP.zeros((1, nreal)))
        back = BP.loadnpz(fname)['raw']
        assert set(back) == set(raw)
        for k in raw:
            assert back[k].dtype == raw[k].dtype and NP.array_equal(back[k], raw[k]), (key, k)
    # noiseless: one getClosurePhase call, repeated along the realisation axis
    sky = out['noiseless']['raw']['cphase']
    assert all(NP.array_equal(sky[:, r], sky[:, 0]) for r in range(nreal))
    legs, conj, _ = s.closure_leg_table([tuple(t) for t in triads.tolist()])
    _, ph = CK.closure_phase(s.skyvis_freq, legs, conj, s.bp, s.bp_wts)
    assert NP.array_equal(sky[:, 0], NP.transpose(ph, (2, 0, 1)))
    assert not NP.array_equal(out['noisy']['raw']['cphase'][:, 0], out['noisy']['raw']['cphase'][:, 1])
    # ClosurePhase takes the dictionary as it is
    cp = BP.ClosurePhase(out['noisy'], s.channels)
    assert cp.cpinfo['raw']['cphase'].shape == (NT, nreal, ntriads, NCHAN)
    assert NP.array_equal(cp.cpinfo['processed']['native']['eicp'].data, NP.exp(1j * out['noisy']['raw']['cphase']))
    # without a prefix nothing is written; explicit triads skip the selection
    few = triads[:4]
    one = BP.simulate_closure_phases(s, 2, 21, triads=few.tolist())
    assert list(one) == ['noisy'] and one['noisy']['raw']['cphase'].shape == (NT, 2, 4, NCHAN)
    assert NP.array_equal(one['noisy']['raw']['cphase'], out['noisy']['raw']['cphase'][:, :2, :4])
    assert sorted(os.listdir(str(tmp_path))) == sorted(['model_noiseless.npz', 'model_noise.npz', 'model_noisy.npz'])


def test_python_layer_refusals():
    s = simulated_standin(StubContext())
    few = [('0', '1', '5')]
    with pytest.raises(ValueError, match='n_realize must be at least 1'):
        s.closure_phase_realizations(0, 1, antenna_triplets=few)
    with pytest.raises(TypeError, match='n_realize'):
        s.closure_phase_realizations(2.0, 1, antenna_triplets=few)
    with pytest.raises(ValueError, match='datakey'):
        s.closure_phase_realizations(2, 1, antenna_triplets=few, datakey='noiseless')
    with pytest.raises(ValueError, match='datakey'):
        s.closure_phase_realizations(2, 1, antenna_triplets=few, datakey=['noisy', 'vis'])
    with pytest.raises(TypeError, match='datakey'):
        s.closure_phase_realizations(2, 1, antenna_triplets=few, datakey=('noisy',))
    with pytest.raises(ValueError, match='n_avg'):
        s.closure_phase_realizations(2, 1, antenna_triplets=few, n_avg=0)
    with pytest.raises(TypeError, match='list of triplet tuples'):
        s.closure_phase_realizations(2, 1, antenna_triplets=tuple(few))
    with pytest.raises(ValueError, match='bl_index'):
        s.closure_phase_realizations(2, 1, antenna_triplets=few, bl_index=NP.arange(3))
    s.gaininfo = object()
    with pytest.raises(NotImplementedError, match='gains'):
        s.closure_phase_realizations(2, 1, antenna_triplets=few)
    s.gaininfo = None
    assert not s._ctx.calls                                          # every refusal came before any device call
    with pytest.raises(ValueError, match='One of triads or bltriplet'):
        BP.simulate_closure_phases(s, 2, 1)
    with pytest.raises(ValueError, match='Invalid input found in datakey'):
        BP.simulate_closure_phases(s, 2, 1, triads=few, datakey='vis')
    with pytest.raises(TypeError, match='datakey must be a list'):
        BP.simulate_closure_phases(s, 2, 1, triads=few, datakey=('noisy',))
    with pytest.raises(ValueError, match='n_realize must be at least 1'):
        BP.simulate_closure_phases(s, 0, 1, triads=few)
    with pytest.raises(TypeError, match='triads must be a list or numpy array'):
        BP.simulate_closure_phases(s, 2, 1, triads='0,1,5')
    with pytest.raises(TypeError, match='outfile_prefix'):
        BP.simulate_closure_phases(s, 2, 1, triads=few, outfile_prefix=3)
    assert not s._ctx.calls
