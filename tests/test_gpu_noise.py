"""The device's thermal-noise draw (csrc/noise_draw.h through k_noise, prisim_hip_noise and prisim_hip_noise_indexed) held to
tests/noise_checker.py: Philox-4x32-10 as published on the counter (f, g low, t, g high) under the key (seed low, seed high), two 52-bit
uniforms, Box-Muller through cospi / sinpi.  tests/test_noise_checker.py holds the checker itself to the published known-answer vectors
and shows that the comparison used here rejects a 9-round Philox, exchanged multipliers or counter words, a dropped high word, a wrong
shift, a missing + 1, a wrong scale, exchanged parts and an angle rounded before the cosine.

The bound.  Against the exact (mpmath) reference, over the small case and its five seeds (3885 elements), the largest componentwise
relative deviation of the device measured on an MI355X is 4.07 u (u = 2^-53; per seed 3.85, 4.07, 3.97, 3.73, 3.62; profiles/LOG.md
section 4.12).  K = 2 x that, rounded up, = 9 u: the factor of 2 is room for a math library that moves log or sincospi by an ulp.
K <= 32 whatever is measured.  Cases too large for mpmath go against the numpy reference, within K + noise_checker.FAST_SLACK of the
element's magnitude rms rad / sqrt(2)."""
import os
import sys

import numpy as NP
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import noise_checker as RK  # noqa: E402

from prisim_amd import sharding as SH  # noqa: E402

pytestmark = pytest.mark.gpu

K = 9
assert K <= RK.K_CEILING

# element (t = 0, b = 0, f = 0) of seed 0, bl_offset 0, rms 1: the published vector 6627e8d5 e169c58d bc57ac4c 9b00dbd8 of the all-zero
# counter and key through Box-Muller -- u1 = (0x6627e8d5e169c + 1) / 2^52, u2 = 0xbc57ac4c9b00d / 2^52 -- by the exact reference
FIRST = complex(-0.08592618483248862, -0.9546172486086594)


def _set(ctx, nbl, nchan):
    ctx.set_array(NP.random.default_rng(nbl).uniform(-100.0, 100.0, (nbl, 3)), 150e6 + NP.arange(nchan) * 1e5, nt_max=1)


@pytest.fixture(scope='module')
def small_rms():
    return RK.small_rms()


def test_known_answer_through_the_abi(ctx):
    _set(ctx, 1, 1)
    got = ctx.noise(NP.ones((1, 1, 1)), seed=0)[0, 0, 0]
    print('first element', repr(got))
    assert RK.deviation(got, FIRST) <= K
    assert RK.draw(0, 0, 0, 0, 1.0, exact=True) == FIRST


@pytest.mark.parametrize('seed', RK.SEEDS, ids=[hex(s) for s in RK.SEEDS])
def test_small_exact_case(ctx, small_rms, seed):
    nt, nbl, nchan = RK.SMALL_SHAPE
    _set(ctx, nbl, nchan)
    got = ctx.noise(small_rms, seed=seed)
    assert got.shape == small_rms.shape and NP.all(got[small_rms == 0.0] == 0.0)
    ref = RK.reference(small_rms, seed, exact=True)
    print('seed %#x: %.2f u' % (seed, RK.deviation(got, ref[0])))
    RK.assert_matches(got, small_rms, seed, K=K, ref=ref)


@pytest.mark.parametrize('bl_offset', RK.HIGH_OFFSETS, ids=['across 2^32', '2^40 + 3'])
def test_high_word_of_the_baseline_and_its_carry(ctx, small_rms, bl_offset):
    nt, nbl, nchan = RK.SMALL_SHAPE
    seed = RK.SEEDS[3]
    _set(ctx, nbl, nchan)
    got = ctx.noise(small_rms, seed=seed, bl_offset=bl_offset)
    print('offset %#x: %.2f u' % (bl_offset, RK.assert_matches(got, small_rms, seed, bl_offset=bl_offset, K=K)))
    # rows g and g + 2^32 differ: the same low word under another high word
    one = NP.ones(small_rms.shape)
    base, high = ctx.noise(one, seed=seed, bl_offset=bl_offset), ctx.noise(one, seed=seed, bl_offset=bl_offset + 2 ** 32)
    assert not NP.any(base.real == high.real) and not NP.any(base.imag == high.imag)
    RK.assert_matches(high, one, seed, bl_offset=bl_offset + 2 ** 32, K=K)


def test_indexed_path_splits_runs(ctx):
    index = [5, 6, 7, 3, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 100, 100, 0]
    nt, nchan, seed = 2, 37, RK.SEEDS[3]
    _set(ctx, len(index), nchan)
    rms = NP.random.default_rng(4).uniform(0.5, 2.0, (nt, len(index), nchan))
    rms[:, 8] = rms[:, 7]
    got = ctx.noise(rms, seed=seed, bl_index=index)
    print('indexed: %.2f u' % RK.assert_matches(got, rms, seed, bl_index=index, K=K))
    assert NP.array_equal(got[:, 7], got[:, 8])                                    # the two rows of global baseline 100
    _set(ctx, 3, nchan)                                                            # and a run is what the contiguous entry draws
    assert NP.array_equal(ctx.noise(rms[:, 4:7], seed=seed, bl_offset=2 ** 32 - 1), got[:, 4:7])


@pytest.mark.parametrize('nbl,nchan', [(1, 1), (3, 255), (3, 257)])
def test_shapes_about_a_workgroup(ctx, nbl, nchan):
    nt, seed = 2, RK.SEEDS[4]
    _set(ctx, nbl, nchan)
    rms = NP.random.default_rng(nchan).uniform(0.5, 2.0, (nt, nbl, nchan))
    print('%d x %d: %.2f u' % (nbl, nchan, RK.assert_matches(ctx.noise(rms, seed=seed, bl_offset=11), rms, seed, bl_offset=11, K=K)))


def test_grid_stride_second_trip(ctx):
    """grid_for caps a launch at 16 384 workgroups of 256 = 4 194 304 threads; 4100 x 1024 = 4 198 400 elements send 4096 threads round again."""
    nbl, nchan, seed = 4100, 1024, RK.SEEDS[3]
    assert 16384 * 256 < nbl * nchan < 2 * 16384 * 256
    _set(ctx, nbl, nchan)
    rms = NP.random.default_rng(6).uniform(0.5, 2.0, (1, nbl, nchan))
    got = ctx.noise(rms, seed=seed)
    print('4100 x 1024: %.2f u of the magnitude' % RK.assert_matches(got, rms, seed, K=K, exact=False))
    g, f = NP.array([4095, 4096, 4099])[:, NP.newaxis], NP.array([0, 1, 1023])[NP.newaxis, :]     # about the second trip, exactly
    assert RK.deviation(got[0][g, f], RK.draw(f, g, 0, seed, rms[0][g, f], exact=True)) <= K


def test_shard_deal_draws_what_the_whole_array_draws(ctx):
    nbl, nchan, nt, world, seed = 701, 5, 2, 3, RK.SEEDS[2]
    bl = NP.random.default_rng(8).uniform(-100.0, 100.0, (nbl, 3))
    ch = 150e6 + NP.arange(nchan) * 1e5
    rms = NP.random.default_rng(9).uniform(0.5, 2.0, (nt, nbl, nchan))
    ctx.set_array(bl, ch, nt_max=1)
    whole = ctx.noise(rms, seed=seed)
    dealt = NP.full(whole.shape, NP.nan, dtype=NP.complex128)
    seen = NP.zeros(nbl, dtype=int)
    for rank in range(world):
        idx = SH.shard_index(nbl, world, rank)
        assert NP.any(NP.diff(idx) > 1)                                            # not one contiguous range: the indexed entry is needed
        ctx.set_array(bl[idx], ch, nt_max=1)
        dealt[:, idx] = ctx.noise(rms[:, idx], seed=seed, bl_index=idx)
        seen[idx] += 1
    assert NP.all(seen == 1) and NP.array_equal(dealt, whole)
    print('dealt: %.2f u of the magnitude' % RK.assert_matches(dealt, rms, seed, K=K, exact=False))


def test_interferometer_array_generate_noise():
    """The class: rms (nbl, nchan, nt) goes to the device as (nt, nbl, nchan) and the noise comes back transposed; the seed is taken mod 2^64;
    row b is global baseline bl_offset + b."""
    from prisim_amd import interferometry as RI, skymodel as SM
    nbl, nchan, nt = 5, 16, 3
    ch = 150e6 + NP.arange(nchan) * 1e5
    bl = NP.random.default_rng(10).uniform(-50.0, 50.0, (nbl, 3))
    area = NP.random.default_rng(13).uniform(100.0, 200.0, (nbl, nchan))            # rms differs along every axis
    skymod = SM.SkyModel(location=[[80.0, 100.0]], flux_ref=[1.0], spindex=[0.0], ref_freq=150e6)
    ia = RI.InterferometerArray(['b%d' % b for b in range(nbl)], bl, ch, telescope={'shape': 'delta'}, skycoords='altaz',
                                pointing_coords='altaz', A_eff=area, eff_Q=0.96)
    for j in range(nt):
        ia.observe((2457000.5 + j, 0.0), {'Tnet': 300.0 + 40.0 * j}, NP.ones(nchan), [90.0, 270.0], skymod, 60.0)
    seed = 2 ** 64 + 0xa4093822299f31d0
    ia.generate_noise(seed=seed, bl_offset=2 ** 32 - 2)
    assert ia.vis_noise_freq.shape == (nbl, nchan, nt)
    rms_bft = NP.broadcast_to(ia.vis_rms_freq, (nbl, nchan, nt))
    assert NP.unique(rms_bft).size == nbl * nchan * nt
    rms_tbf = NP.transpose(rms_bft, (2, 0, 1))
    got = NP.transpose(ia.vis_noise_freq, (2, 0, 1))
    print('class: %.2f u' % RK.assert_matches(got, rms_tbf, seed - 2 ** 64, bl_offset=2 ** 32 - 2, K=K))
    ia.generate_noise(seed=seed - 2 ** 64, bl_index=NP.arange(nbl) + 2 ** 32 - 2)
    assert NP.array_equal(NP.transpose(ia.vis_noise_freq, (2, 0, 1)), got)
