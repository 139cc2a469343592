"""CPU: the fp32 route of the beam-weighted mosaic (include/prisim_mosaic32.h) -- the export, the sources that share one host body, the
planner compiled alone under the sanitizers, a numpy model of the device's chain against the checker, and the attribute `precision` of
prisim_amd.interferometry.ApertureSynthesis against a stand-in context.

Bounds.  BOUND = 5e-6 is the project's bar for its float32 mode and what tests/test_gpu_imaging32.py holds every D_t to;
A_t <= 1 and the triangle inequality carry it to |N_32 - N_64| <= BOUND sum_t A_t sum_b w|V| per element, which is what
tests/test_gpu_mosaic32.py holds the device to.  The model (tests/mosaic32_model.py: the chain of tests/imaging32_model.py per snapshot,
then the fp64 epilogue of the header in t order) is held to half of it, 2.5e-6, against tests/mosaic_checker.py on the shapes the
device is run on, and its Q to the bits of the header's statement evaluated in exact rationals.  Measured here (x86-64), worst over the
four beams as a share of 2.5e-6: 1 x 33 x 1000 x 1 0.50; 37 x 5 x 63 x 1 0.06; 65 x 33 x 257 x 2 0.05; 300 x 70 x 65 x 3 0.03;
37 x 33 x 1000 x 3 0.08."""
import inspect
import os
import subprocess
import sys
from fractions import Fraction

import numpy as NP
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import imaging_cases as IC  # noqa: E402
import mosaic32_model as M32  # noqa: E402
import mosaic_cases as MC  # noqa: E402
import mosaic_checker as MK  # noqa: E402
import test_mosaic as TM  # noqa: E402  (the array, the drift scan and the stand-in context of the mosaic tests)
import test_mosclean as TQ  # noqa: E402  (the stand-in context of clean_mosaic)
import test_moscs as TX  # noqa: E402  (the stand-in context of clean_mosaic_cotton_schwab)

from prisim_amd import _abi  # noqa: E402
from prisim_amd import interferometry as RI  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 5e-6
MODEL_BOUND = BOUND / 2
K = 32
# (nbl, nchan, npix, nt) of tests/test_gpu_mosaic32.py
SHAPES = [(1, 1, 1, 1), (1, K + 1, 1000, 1), (37, 5, 63, 1), (65, K + 1, 257, 2), (300, 70, 65, 3), (37, K + 1, 1000, 3)]
BEAMS = ['gaussian', 'airy', 'dipole_ground', 'beamformer']
REAL_CONTEXT = _abi.Context                                          # the tests of the class put a stand-in in its place


# ---- the library, its sources and the planner -----------------------------------------------------------------------------------------

def test_export_is_in_the_library_and_outside_the_core_abi():
    lib = _abi.load_library()
    assert _abi.MOSAIC32_EXPORTS == ('prisim_mosaic_image_f32',) == _abi.HEADER_EXPORTS['prisim_mosaic32.h']
    assert 'prisim_mosaic_image_f32' not in _abi.EXPORTS and lib.prisim_hip_version().decode() == _abi.ABI_VERSION
    assert _abi.FUNCTIONS['prisim_mosaic_image_f32'] == _abi.FUNCTIONS['prisim_mosaic_image']      # the same arguments, the same structs
    assert lib.prisim_mosaic_image_f32(None, None, None, None, None, None, None, None) == _abi.PRISIM_EINVAL     # a null context: refused, not read
    assert _abi.MOSAIC_PRECISIONS == {'double': 'prisim_mosaic_image', 'single': 'prisim_mosaic_image_f32'}
    p = inspect.signature(_abi.Context.mosaic_image).parameters
    assert p['precision'].default == 'double' and list(p)[-1] == 'precision'
    header = open(os.path.join(ROOT, 'include', 'prisim_mosaic32.h')).read()
    assert '#include "prisim_mosaic.h"' in header and 'typedef struct' not in header and 'enum' not in header.split('*/', 1)[1]


def test_the_two_entries_share_one_host_body_and_each_compiles_its_own_sum():
    folder = os.path.join(ROOT, 'prisim_amd', 'csrc_imaging')
    src = {name: open(os.path.join(folder, name)).read() for name in ('mosaic.hip', 'mosaic32.hip', 'mosaic_frame.h', 'mosaic32_kernels.h',
                                                                      'mosaic_kernels.h', 'imaging32_kernels.h')}
    frame = src['mosaic_frame.h']
    # the checks, the tables, the beam, the chunk loop and the host buffers are written once, in the frame both entries call
    for name in ('check_args(ctx, v)', 'check_mosaic_beam(ctx, *a)', 'imaging_preamble(ctx, v, su)', 'upload_tables(ctx, wk.dev, v, s0, T)',
                 'upload_beamformers(', 'enqueue_mos_wsum(', 'enqueue_mos_beam(', 'enqueue_mos_finish(', 'chunk_loop(', 'poly_beam_verdict(',
                 'std::vector<double> h_mos', 'plan_stats('):
        assert frame.count(name) == 1, name
        assert name not in src['mosaic.hip'] and name not in src['mosaic32.hip'], name
    for entry, plan, enqueue in (('mosaic.hip', 'mosaic_plan,', 'enqueue_mos_sum('), ('mosaic32.hip', 'mosaic32_plan,', 'enqueue_mos32_sum(')):
        assert src[entry].count('mosaic_frame(') == 1 and '#include "mosaic_frame.h"' in src[entry] and plan in src[entry] and enqueue in src[entry]
    assert 'enqueue_mos_sum(' not in frame and 'enqueue_mos32_sum(' not in frame and 'mosaic_plan(' not in frame and 'mosaic32_plan(' not in frame
    # the fp32 sum calls the tile pass of the dirty image's fp32 route and restates nothing of it
    k = src['mosaic32_kernels.h']
    assert k.count('img32_tile_pass<false>(') == 1 and '#include "imaging32_kernels.h"' in k and '#include "mosaic_kernels.h"' in k
    assert k.count('__global__') == 1 and 'k_mos32_sum(MosParams P)' in k and 'kImaging32Lds' in k and 'static_assert' in k
    for name in ('sincos_qcycles(', 'pk_fma(', '__syncthreads', 'sh_f[', 'double acc'):
        assert name not in k, name
    assert 'fma(A, tot[k], t ? P.N[at + k] : 0.0)' in k and 'fma(A * A, P.wt[k0 + k], t ? P.Q[at + k] : 0.0)' in k and 'double tot[CT];' in k
    assert src['imaging32_kernels.h'].count('void img32_tile_pass(') == 1 and src['mosaic_kernels.h'].count('struct MosParams {') == 1
    plan = open(os.path.join(ROOT, 'prisim_amd', 'csrc_addon', 'mosaic32_plan.h')).read()
    assert 'mosaic_plan(' in plan and 'kImaging32Lds' in plan and 'kImaging32Reseed' in plan and '17920' not in plan
    assert not [ln for ln in plan.splitlines() if ln.lstrip().startswith('constexpr')]           # no constant of its own
    # an add-on: one name in the Makefile, nothing under csrc/
    mk = open(os.path.join(ROOT, 'prisim_amd', 'csrc', 'Makefile')).read()
    assert mk.count('mosaic32') == 1 and not [f for f in os.listdir(os.path.join(ROOT, 'prisim_amd', 'csrc')) if 'mosaic32' in f]


def test_plan_header_compiles_alone_and_plans_as_the_fp64_entry(tmp_path):
    exe = tmp_path / 'mosaic32_plan_check'
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-Wall', '-Werror', '-fsanitize=address,undefined', '-I',
                           os.path.join(ROOT, 'prisim_amd', 'csrc_addon'), os.path.join(ROOT, 'tests', 'mosaic32_plan_main.cpp'), '-o', str(exe)])
    res = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = res.stdout.decode()
    assert res.returncode == 0, out
    lines = out.strip().splitlines()
    assert lines[-1] == 'checked %d bad 0' % (5 * 5 * 2 * 3 * 2 * (8 * 3 * 2 + 4) + 3), out
    got = {name: int(value) for name, value in (ln.split() for ln in lines[:-1])}
    # the constants of imaging32_plan.h, and what the plan reports of them
    assert got == {'reseed': 32, 'lds': 17920, 'tile': 32, 'block': 256, 'reported_reseed': 32, 'reported_lds': 17920, 'reported_tile': 32,
                   'reported_block': 256}
    txt = open(os.path.join(ROOT, 'prisim_amd', 'csrc_addon', 'mosaic32_plan.h')).read()
    assert '#include <hip' not in txt and '__device__' not in txt and '#include "addon_internal.h"' not in txt


# ---- the model of the chain against the checker ---------------------------------------------------------------------------------------

def exact_fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))             # float() of a Fraction rounds once, to nearest even


def q_statement(A, W):
    """Q of include/prisim_mosaic.h, Q = fma(A * A, W_t, Q) from 0 with t ascending, every fma in exact rationals rounded once"""
    fma = NP.frompyfunc(exact_fma, 3, 1)
    Q = NP.zeros(A.shape[1:])
    for t in range(A.shape[0]):
        Q = fma(A[t] * A[t], NP.broadcast_to(W[t], Q.shape), Q).astype(NP.float64)
    return Q


def test_model_fma_rounds_once():
    rng = NP.random.default_rng(11)
    a, b = rng.uniform(0.0, 1.0, 20000), rng.uniform(0.5, 600.0, 20000)
    c = NP.where(rng.uniform(size=20000) < 0.5, rng.uniform(0.0, 2000.0, 20000), -a * b * (1.0 + 1e-9 * rng.standard_normal(20000)))
    want = NP.frompyfunc(exact_fma, 3, 1)(a, b, c).astype(NP.float64)
    assert NP.array_equal(M32.fma64(a, b, c), want)
    assert NP.count_nonzero(a * b + c != want) > 100                  # and two roundings are seen to differ: the comparison bites


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(str(v) for v in s))
def test_model_of_the_chain_holds_half_the_contract(shape):
    nbl, nchan, npix, nt = shape
    c = IC.case(nbl, nchan, npix, nt)
    beams = MC.beam_setups(nt)
    weights = c['w_full'] if nbl >= 7 else None
    sums = MK.snapshot_sums(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], c['cube'], weights=weights, aberr_beta=c['beta'])
    model = None
    worst = 0.0
    for name in BEAMS:
        A = MK.beams(sums['s'], c['freqs'], beams[name][3])
        ref = MK.combine(sums, A)
        if model is None:                                             # the chain of every snapshot once per shape; the beams share it
            model = M32.mosaic_sums(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], c['cube'], A, weights=weights, aberr_beta=c['beta'])
            D = model['D']
        N, Q = M32.epilogue(D, A, sums['W'])
        bound = MODEL_BOUND * NP.einsum('tpk,tk->pk', A, sums['absV'])
        err = NP.abs(N - ref['num'])
        with NP.errstate(invalid='ignore', divide='ignore'):
            share = float(NP.nanmax(NP.where(bound > 0.0, err / bound, NP.where(err > 0.0, NP.inf, 0.0))))
        print('%s %s: model |N - N_ref| at most %.3f of the bound %.1e sum_t A sum_b w|V|' % (shape, name, share, MODEL_BOUND))
        assert N.dtype == NP.float64 and N.shape == (npix, nchan) and NP.all(err <= bound), (shape, name, share)
        assert NP.array_equal(Q, q_statement(A, sums['W'])), (shape, name)
        assert NP.allclose(Q, ref['den'], rtol=1e-15, atol=0)         # the checker's Q, which rounds the product and the sum apart
        worst = max(worst, share)
    print('%s: worst %.3f of the model bound' % (shape, worst))


# ---- the precision through the class, against a stand-in context --------------------------------------------------------------------------

class Precision32Context(TQ.MoscleanOracleContext, TX.MoscsOracleContext):
    """The stand-in contexts of the mosaic tests in one, with a mosaic_image that takes `precision` as Context.mosaic_image does and
    records whether it was handed one; clean_mosaic and clean_mosaic_cs are the stand-ins as they are, and take no such keyword."""

    def mosaic_image(self, *args, **kw):
        handed = 'precision' in kw
        precision = kw.pop('precision', 'double')
        out = super().mosaic_image(*args, **kw)
        TM.MosaicOracleContext.calls[-1].update(precision=precision, handed=handed)
        return out[:4] + (dict(out[4], precision=precision),)


def observed(monkeypatch, channels=None):
    monkeypatch.setattr(TM, 'MosaicOracleContext', Precision32Context)
    TQ.MoscleanOracleContext.cleans = []
    TX.MoscsOracleContext.cleans = []
    if channels is not None:
        monkeypatch.setattr(TM, 'CH', channels)
    return TM.observed(monkeypatch, MC.GAUSS14, [MC.ZENITH] * 3)


def test_precision_reaches_the_context_and_the_default_call_is_the_old_one(monkeypatch):
    ia = observed(monkeypatch)
    calls = TM.MosaicOracleContext.calls
    aps = RI.ApertureSynthesis(ia)
    assert aps.precision == 'double'
    plain = aps.mosaic(MC.SOURCE_RADEC, coords='radec')
    assert len(calls) == 1 and calls[0]['handed'] is False and aps.image_stats['precision'] == 'double'      # no new keyword: the call of before
    aps.precision = 'single'
    for route in ('auto', 'stepped'):
        one = aps.mosaic(MC.SOURCE_RADEC, coords='radec', route=route, pbmin=0.05, budget_bytes=777)
        c = calls[-1]
        assert c['handed'] is True and c['precision'] == 'single' and c['route'] == route and c['pbmin'] == 0.05 and c['budget_bytes'] == 777
        assert aps.image_stats['precision'] == 'single' and NP.array_equal(one, plain)          # the stand-in answers with the checker
        assert set(('num', 'den', 'wsum', 'pb_eff')) <= set(aps.image_stats)
    # refused before any device work: nothing reaches the context
    n = len(calls)
    with pytest.raises(ValueError, match='direct'):
        aps.mosaic(MC.SOURCE_RADEC, coords='radec', route='direct')
    aps.precision = 'half'
    with pytest.raises(ValueError, match='precision'):
        aps.mosaic(MC.SOURCE_RADEC, coords='radec')
    assert len(calls) == n
    aps.precision = 'double'
    aps.mosaic(MC.SOURCE_RADEC, coords='radec', route='direct')       # the fp64 route takes it as before
    assert calls[-1]['handed'] is False and calls[-1]['route'] == 'direct' and aps.image_stats['precision'] == 'double'
    # the parameter list is the one tests/test_mosaic.py pins: the precision is an attribute
    assert list(inspect.signature(aps.mosaic).parameters) == ['directions', 'coords', 'datakey', 'weights', 'chan_avg', 'epoch', 'telescope',
                                                              'pb_info', 'pbmin', 'route', 'budget_bytes']
    # Context.mosaic_image itself turns any other value away before it touches its arguments
    with pytest.raises(ValueError, match='precision'):
        REAL_CONTEXT.mosaic_image(None, None, None, None, None, None, 0, 0.0, precision='half')


def test_single_precision_refuses_a_non_uniform_grid_before_any_device_work(monkeypatch):
    ia = observed(monkeypatch, channels=150e6 + 1e5 * NP.arange(6) + 3e4 * NP.sin(NP.arange(6)))
    calls = TM.MosaicOracleContext.calls
    aps = RI.ApertureSynthesis(ia)
    aps.precision = 'single'
    for route in ('auto', 'stepped'):
        with pytest.raises(ValueError, match='uniform'):
            aps.mosaic(MC.SOURCE_RADEC, coords='radec', route=route)
    assert calls == []
    aps.precision = 'double'
    aps.mosaic(MC.SOURCE_RADEC, coords='radec')
    assert len(calls) == 1 and calls[0]['handed'] is False


def test_the_cleans_of_the_mosaic_do_not_read_the_attribute(monkeypatch):
    ia = observed(monkeypatch)
    aps = RI.ApertureSynthesis(ia)
    aps.precision = 'single'
    # the stand-ins' clean_mosaic and clean_mosaic_cs take no `precision`: a keyword handed on would be a TypeError here
    out = aps.clean_mosaic(TX.GRID, coords='radec', gain=0.2, maxiter=20, threshold=0.05)
    assert len(TQ.MoscleanOracleContext.cleans) == 1 and 'residual' in out
    out = aps.clean_mosaic_cotton_schwab(TX.GRID, (2, 2), coords='radec', gain=0.2, maxiter=20, threshold=0.05)
    assert len(TX.MoscsOracleContext.cleans) == 1 and 'residual' in out
    assert TM.MosaicOracleContext.calls == []                         # neither went through mosaic_image
    for method in (RI.ApertureSynthesis.clean, RI.ApertureSynthesis.clean_mosaic, RI.ApertureSynthesis.clean_cotton_schwab,
                   RI.ApertureSynthesis.clean_mosaic_cotton_schwab):
        assert 'precision' not in inspect.getsource(method).split('"""')[2], method.__name__
