"""CPU: the fp32 route of dirty images and synthesized beams (include/prisim_imaging32.h) -- the planner compiled alone under the
sanitizers, a numpy float32 model of the device's chain against the checker, the coherent sum with and without the flush, the export
and the attribute `precision` of prisim_amd.interferometry.ApertureSynthesis against a stand-in context.

Bounds.  BOUND = 5e-6 of the natural scale (sum w|V| / sum w, 1 for the beam) is the project's bar for its float32 mode and what
tests/test_gpu_imaging32.py holds the device to.  The model (tests/imaging32_model.py: the device's seed position, step, recurrence and
flush interval, read from prisim_amd/csrc_addon/imaging32_plan.h) is held to half of it, 2.5e-6, on the shapes the device is run on and
on one baseline x 33 channels x 3000 pixels, where nothing averages the error of a chain: the chosen chain has a factor of two in hand
before any device run.  Measured here (x86-64): 1 x 33 x 3000 1.5e-6, the same at 90 km; 1 x 33 x 1000 1.4e-6; the multi-baseline
shapes <= 1.5e-7; the coherent beam of 20000 baselines 1.5e-7 (w = 0.7) and 2.8e-7 (0.1) with the plan's flush and 8.7e-5 with none.
The device gives these figures to three digits (tests/test_gpu_imaging32.py)."""
import inspect
import os
import re
import subprocess
import sys

import numpy as NP
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import imaging32_model as M  # noqa: E402
import imaging_cases as IC  # noqa: E402
import imaging_checker as IK  # noqa: E402
import test_imaging as TI  # noqa: E402  (the arrays and the stand-in context of the imaging tests)

from prisim_amd import _abi  # noqa: E402
from prisim_amd import interferometry as RI  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 5e-6
MODEL_BOUND = BOUND / 2
# (nbl, nchan, npix, nt) of tests/test_gpu_imaging32.py
SHAPES = [(1, 1, 1, 1), (1, 33, 1000, 1), (37, 5, 63, 1), (300, 70, 65, 3), (37, 33, 1000, 3)]


# ---- the library, its sources and the planner -----------------------------------------------------------------------------------------

def test_export_is_in_the_library_and_outside_the_core_abi():
    lib = _abi.load_library()
    assert _abi.IMAGING32_EXPORTS == ('prisim_dirty_image_f32',) and 'prisim_dirty_image_f32' not in _abi.EXPORTS
    assert _abi.HEADER_EXPORTS['prisim_imaging32.h'] == _abi.IMAGING32_EXPORTS
    assert _abi.FUNCTIONS['prisim_dirty_image_f32'] == _abi.FUNCTIONS['prisim_dirty_image']      # the same arguments, the same structs
    assert lib.prisim_dirty_image_f32(None, None, None, None, None) == _abi.PRISIM_EINVAL       # a null context is refused, not read
    assert _abi.IMAGING_PRECISIONS == {'double': 'prisim_dirty_image', 'single': 'prisim_dirty_image_f32'}
    assert inspect.signature(_abi.Context.dirty_image).parameters['precision'].default == 'double'
    header = open(os.path.join(ROOT, 'include', 'prisim_imaging32.h')).read()
    assert '#include "prisim_imaging.h"' in header and 'typedef struct' not in header and 'enum' not in header.split('*/', 1)[1]


def test_sources_compile_what_they_launch_and_restate_the_trig_to_the_letter():
    folder = os.path.join(ROOT, 'prisim_amd', 'csrc_imaging')
    src = {name: open(os.path.join(folder, name)).read() for name in ('imaging32.hip', 'imaging32_kernels.h', 'dirty_frame.h', 'sincos_qcycles32.h')}
    # the fp32 entry includes the frame of the dirty image, not the fp64 sum; the fp64 sum is not in the frame
    assert all('dirty_image.h"' not in txt and 'k_img_sum<' not in txt for txt in src.values())
    assert '#include "dirty_frame.h"' in src['imaging32_kernels.h'] and '#include "dirty_frame.h"' in open(os.path.join(folder, 'dirty_image.h')).read()
    # the shared host set-up is called, not restated
    for name in ('check_args(ctx, v)', 'imaging_preamble(ctx, v, su)', 'upload_tables(ctx, wk.dev, v, s0, T)', 'enqueue_weight_sums(ctx, job, s0)'):
        assert src['imaging32.hip'].count(name) == 1, name
    assert 'imaging32_plan(' in src['imaging32.hip'] and 'pixel_plan(' in open(os.path.join(ROOT, 'prisim_amd', 'csrc_addon', 'imaging32_plan.h')).read()
    # packed FMAs written out, no hardware sine or cosine, builtins for every fused operation
    k = src['imaging32_kernels.h']
    assert 'ext_vector_type(2)' in k and '__builtin_elementwise_fma' in k and 'sinf' not in k and 'cosf' not in k and '__sinf' not in k

    def body(txt):
        return re.search(r'__device__ __forceinline__ void sincos_qcycles\(double a4, float& c, float& s\) \{.*?\n\}', txt, flags=re.S).group(0)

    original = open(os.path.join(ROOT, 'prisim_amd', 'csrc', 'skyvis_kernels.hip')).read()
    assert body(src['sincos_qcycles32.h']) == body(original)
    mk = open(os.path.join(ROOT, 'prisim_amd', 'csrc', 'Makefile')).read()
    assert mk.count('imaging32') == 1 and not [f for f in os.listdir(os.path.join(ROOT, 'prisim_amd', 'csrc')) if 'imaging32' in f]


def test_plan_header_compiles_alone_and_plans_as_the_fp64_entry(tmp_path):
    exe = tmp_path / 'imaging32_plan_check'
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-Wall', '-Werror', '-fsanitize=address,undefined', '-I',
                           os.path.join(ROOT, 'prisim_amd', 'csrc_addon'), os.path.join(ROOT, 'tests', 'imaging32_plan_main.cpp'), '-o', str(exe)])
    res = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = res.stdout.decode()
    assert res.returncode == 0, out
    lines = out.strip().splitlines()
    assert lines[-1] == 'checked %d bad 0' % (5 * 5 * 2 * 3 * 2 * (8 * 3 * 2 + 4) + 3), out
    got = {name: int(value) for name, value in (ln.split() for ln in lines[:-1])}
    # the constants the model reads from the text are the compiled ones
    assert got == {'rows': M.ROWS, 'flush': M.FLUSH, 'seed': M.SEED, 'reseed': M.PLAN['kImaging32Reseed'], 'lds': 17920, 'tile': M.TILE, 'block': 256}
    assert (M.ROWS, M.FLUSH, M.SEED, M.TILE) == (64, 64, 16, 32)
    txt = open(os.path.join(ROOT, 'prisim_amd', 'csrc_addon', 'imaging32_plan.h')).read()
    assert '#include <hip' not in txt and '__device__' not in txt and '#include "addon_internal.h"' not in txt


# ---- the model of the chain against the checker ---------------------------------------------------------------------------------------

def deviation(got, want):
    return float(NP.max(NP.abs(got - want['image']) / want['scale']))


def test_model_trig_is_good_to_an_ulp():
    x = NP.random.default_rng(5).uniform(-3e8, 3e8, 200000)           # cycles, out to the 2^29 of the domain
    c, s = M.sincos_qcycles(4.0 * x)
    r = x - NP.rint(x)
    err = max(float(NP.max(NP.abs(c - NP.cos(2 * NP.pi * r)))), float(NP.max(NP.abs(s - NP.sin(2 * NP.pi * r)))))
    print('model sincos_qcycles: %.3e absolute (2^-23 = %.3e)' % (err, 2.0 ** -23))
    assert c.dtype == NP.float32 and err <= 2.0 ** -23


@pytest.mark.parametrize('shape', SHAPES + [(1, 33, 3000, 1)], ids=lambda s: 'x'.join(str(v) for v in s))
def test_model_of_the_chain_holds_half_the_contract(shape):
    nbl, nchan, npix, nt = shape
    c = IC.case(nbl, nchan, npix, nt)
    worst = 0.0
    for kind, weights in (('dirty', c['w_full'] if nbl >= 7 else None), ('psf', c['w_bl'] if nbl >= 7 else None)):
        want = IK.dirty_image(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], cube=c['cube'], weights=weights, kind=kind,
                              aberr_beta=c['beta'])
        got = M.dirty_image(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], cube=c['cube'], weights=weights, kind=kind,
                            aberr_beta=c['beta'])
        dev = deviation(got, want)
        band = deviation(NP.einsum('pk,k->p', got, want['wsum']) / want['band']['wsum'][0], want['band'])
        print('%s %s: model %.3e, band %.3e of the scale (bound %.2e)' % (shape, kind, dev, band, MODEL_BOUND))
        assert got.dtype == NP.float64 and got.shape == (npix, nchan)
        worst = max(worst, dev, band)
    assert worst <= MODEL_BOUND, (shape, worst)


def test_model_long_baselines_cost_nothing():
    c = IC.case(1, 33, 3000, 1)
    bl = c['baselines'] * 300.0                                       # 90 km
    want = IK.dirty_image(c['unitvec'], c['rot'], c['pc'], bl, c['freqs'], cube=c['cube'], aberr_beta=c['beta'])
    dev = deviation(M.dirty_image(c['unitvec'], c['rot'], c['pc'], bl, c['freqs'], cube=c['cube'], aberr_beta=c['beta']), want)
    print('1 x 33 x 3000 at 90 km: model %.3e of the scale (bound %.2e)' % (dev, MODEL_BOUND))
    assert dev <= MODEL_BOUND


def test_model_coherent_sum_needs_the_flush_and_the_plans_interval_holds_it():
    c = M.coherent_case()
    nbl = c['nbl']
    for weight in (0.7, 0.1):
        w = NP.full(nbl, weight)
        want = IK.dirty_image(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], weights=w, kind='psf')
        got = M.dirty_image(c['unitvec'], c['rot'], c['pc'], c['baselines'], c['freqs'], weights=w, kind='psf')
        centre, dev = float(NP.max(NP.abs(got[0] - 1.0))), deviation(got, want)
        print('coherent beam, w = %.1f, flush every %d rows: %.3e at the phase centre, %.3e over all (bound %.1e)' % (weight, M.FLUSH, centre, dev, BOUND))
        assert centre <= BOUND and dev <= BOUND
    # the same chain with no flush inside a snapshot: the float32 partial sums of 10000 equal terms drift past the bound
    w = NP.full(nbl, 0.7)
    none = M.dirty_image(c['unitvec'][:3], c['rot'], c['pc'], c['baselines'], c['freqs'], weights=w, kind='psf', flush=0)
    drift = float(NP.max(NP.abs(none[0] - 1.0)))
    print('coherent beam, w = 0.7, no flush: %.3e at the phase centre' % drift)
    assert drift > BOUND


# ---- the precision through the class, against a stand-in context --------------------------------------------------------------------------

class Precision32Context(TI.ImagingOracleContext):
    """ImagingOracleContext that takes `precision` as Context.dirty_image does and records it."""

    def dirty_image(self, *args, precision='double', **kw):
        image, wsum, st = super().dirty_image(*args, **kw)
        TI.ImagingOracleContext.calls[-1]['precision'] = precision
        return image, wsum, dict(st, precision=precision)


def observed(monkeypatch, channels=None):
    monkeypatch.setattr(TI, 'ImagingOracleContext', Precision32Context)
    if channels is not None:
        monkeypatch.setattr(TI, 'CH', channels)
    ia = TI.observed(monkeypatch, 'altaz', [[90.0, 270.0]] * 3)
    return ia, Precision32Context.calls


def test_precision_reaches_the_context_and_the_default_is_double(monkeypatch):
    ia, calls = observed(monkeypatch)
    aps = RI.ApertureSynthesis(ia)
    grid = aps.dircos_grid(3, 0.2)
    del calls[:]
    assert aps.precision == 'double'
    img = aps.image(grid)
    assert len(calls) == 1 and calls[0]['precision'] == 'double' and aps.image_stats['precision'] == 'double'
    aps.precision = 'single'
    for route in ('auto', 'stepped'):
        one = aps.image(grid, route=route)
        assert calls[-1]['precision'] == 'single' and calls[-1]['route'] == route and calls[-1]['kind'] == 'dirty'
        assert aps.image_stats['precision'] == 'single' and NP.array_equal(one, img)              # the stand-in answers with the checker
    beam = aps.psf(grid, chan_avg=True)
    assert calls[-1]['precision'] == 'single' and calls[-1]['kind'] == 'psf' and calls[-1]['chan_avg'] is True and beam.shape == (9,)
    assert aps.image_stats['precision'] == 'single'
    # refused before any device work: nothing reaches the context
    n = len(calls)
    for fn in (aps.image, aps.psf):
        with pytest.raises(ValueError, match='direct'):
            fn(grid, route='direct')
    aps.precision = 'half'
    for fn in (aps.image, aps.psf):
        with pytest.raises(ValueError, match='precision'):
            fn(grid)
    assert len(calls) == n
    aps.precision = 'double'
    aps.psf(grid)
    assert calls[-1]['precision'] == 'double' and aps.image_stats['precision'] == 'double'
    aps.image(grid, route='direct')                                   # the fp64 route takes it as before
    assert calls[-1]['precision'] == 'double' and calls[-1]['route'] == 'direct'
    # the parameter lists of image() and psf() are the ones tests/test_mosaic.py pins: the precision is an attribute
    assert 'precision' not in inspect.signature(aps.image).parameters and 'precision' not in inspect.signature(aps.psf).parameters


def test_single_precision_refuses_a_non_uniform_grid_before_any_device_work(monkeypatch):
    ia, calls = observed(monkeypatch, channels=150e6 + 1e5 * NP.arange(6) + 3e4 * NP.sin(NP.arange(6)))
    aps = RI.ApertureSynthesis(ia)
    grid = aps.dircos_grid(3, 0.2)
    del calls[:]
    aps.precision = 'single'
    for route in ('auto', 'stepped'):
        for fn in (aps.image, aps.psf):
            with pytest.raises(ValueError, match='uniform'):
                fn(grid, route=route)
    assert calls == []
    aps.precision = 'double'
    aps.image(grid)
    assert len(calls) == 1 and calls[0]['precision'] == 'double'
