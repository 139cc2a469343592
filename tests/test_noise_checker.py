"""tests/noise_checker.py held to the published known-answer vectors of Philox-4x32-10 (Random123, kat_vectors), its two evaluations held
to each other, and the comparison that the GPU suite calls (assert_matches) shown to reject every mutated restatement of the draw on the
GPU suite's own cases.  No GPU."""
import math
import os
import sys

import numpy as NP
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import noise_checker as RK  # noqa: E402

KAT = (((0x00000000,) * 4, (0x00000000,) * 2, (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)))

# element (t = 0, b = 0, f = 0) of seed 0, bl_offset 0, rms 1: the first vector through Box-Muller, by the exact evaluation
FIRST = complex(-0.08592618483248862, -0.9546172486086594)


def test_published_known_answer_vectors():
    for counter, key, want in KAT:
        assert RK.philox4x32_int(counter, key) == want
        assert RK.philox4x32_10(counter, key) == want
        got = RK.philox4x32_np([NP.array([c], dtype=NP.uint64) for c in counter], [NP.array([k], dtype=NP.uint64) for k in key])
        assert tuple(int(w[0]) for w in got) == want and all(w.dtype == NP.uint64 for w in got)
    # all three at once, as the vectorised form is used
    got = RK.philox4x32_10([NP.array([k[0][i] for k in KAT]) for i in range(4)], [NP.array([k[1][i] for k in KAT]) for i in range(2)])
    assert [tuple(int(w[j]) for w in got) for j in range(3)] == [k[2] for k in KAT]


def test_scalar_and_vectorised_forms_agree():
    rng = NP.random.default_rng(7)
    words = rng.integers(0, 2 ** 32, (6, 10000), dtype=NP.uint64)
    vec = NP.stack(RK.philox4x32_np(words[:4], words[4:]))
    for j in range(words.shape[1]):
        w = [int(x) for x in words[:, j]]
        assert RK.philox4x32_int(w[:4], w[4:]) == tuple(int(x) for x in vec[:, j])


def test_counter_and_key_words():
    g, seed = (0x12 << 32) | 0x89abcdef, (0xfeed << 32) | 0xbeef
    assert RK.counter_key(5, g, 7, seed) == ((5, 0x89abcdef, 7, 0x12), (0xbeef, 0xfeed))
    assert RK.counter_key(5, g, 7, seed + 2 ** 64) == RK.counter_key(5, g, 7, seed)            # the seed is taken mod 2^64
    c, k = RK.counter_key(NP.array([5]), NP.array([g], dtype=NP.uint64), NP.array([7]), seed)
    assert [int(w[0]) for w in c] == [5, 0x89abcdef, 7, 0x12] and [int(w) for w in k] == [0xbeef, 0xfeed]


@pytest.mark.parametrize('form', ['int', 'numpy'])
def test_edges_of_the_uniforms(form):
    def uni(r):
        if form == 'int':
            return RK.uniforms(r)
        u1, u2 = RK.uniforms([NP.array([w], dtype=NP.uint64) for w in r])
        return float(u1[0]), float(u2[0])
    u1, u2 = uni((0, 0, 0, 0))
    assert u1 == 2.0 ** -52 and u2 == 0.0
    for exact in (True, False):
        v = complex((RK.box_muller_exact if exact else RK.box_muller_fast)(u1, u2, 1.5)[0])
        assert v.imag == 0.0 and math.isfinite(v.real)                                          # real and finite: the largest draw there is
        assert abs(v.real / (1.5 * math.sqrt(52.0 * math.log(2.0))) - 1.0) < 1e-15              # rms / sqrt(2) * sqrt(2 * 52 ln 2)
    u1, u2 = uni((0xffffffff,) * 4)
    assert u1 == 1.0 and u2 == 1.0 - 2.0 ** -52
    for exact in (True, False):
        assert complex((RK.box_muller_exact if exact else RK.box_muller_fast)(u1, u2, 1.5)[0]) == 0.0
    u1, u2 = uni((0, 0xfff, 0x80000000, 0))                                                     # the low 12 bits of r1 and r3 are not used
    assert u1 == 2.0 ** -52 and u2 == 0.5


def test_first_element_is_the_first_vector_through_box_muller():
    u1, u2 = RK.uniforms(KAT[0][2])
    assert u1 == ((0x6627e8d5 << 20 | 0xe169c58d >> 12) + 1) / 2.0 ** 52 and u2 == (0xbc57ac4c << 20 | 0x9b00dbd8 >> 12) / 2.0 ** 52
    assert RK.draw(0, 0, 0, 0, 1.0, exact=True) == FIRST
    assert RK.noise(NP.ones((1, 1, 1)), 0, exact=True)[0, 0, 0] == FIRST
    # the same number from the definition, without the checker's Box-Muller: cos and sin of 2 pi u2 in mpmath
    import mpmath
    with mpmath.workprec(200):
        a = mpmath.sqrt(-mpmath.log(mpmath.mpf(u1)))                                            # sqrt(-2 ln u1) / sqrt(2)
        ang = 2 * mpmath.pi * mpmath.mpf(u2)
        assert abs(float(a * mpmath.cos(ang)) - FIRST.real) <= 2.0 ** -53 * abs(FIRST.real)     # INV_SQRT2 is 1/sqrt(2) to 21 digits
        assert abs(float(a * mpmath.sin(ang)) - FIRST.imag) <= 2.0 ** -53 * abs(FIRST.imag)


def test_layout_offset_and_index():
    rms = NP.random.default_rng(3).uniform(0.5, 2.0, (2, 4, 5))
    a = RK.noise(rms, 77, bl_offset=9)
    assert a.shape == rms.shape and a.dtype == NP.complex128
    for t, b, f in ((0, 0, 0), (1, 3, 4), (0, 2, 1)):
        assert a[t, b, f] == RK.draw(f, 9 + b, t, 77, float(rms[t, b, f]))
    assert NP.array_equal(a, RK.noise(rms, 77, bl_index=[9, 10, 11, 12]))
    one = NP.ones(rms.shape)
    a, b = RK.noise(one, 77, bl_offset=9), RK.noise(one, 77, bl_index=[12, 2 ** 40, 9, 9])
    assert NP.array_equal(b[:, 0], a[:, 3]) and NP.array_equal(b[:, 2], a[:, 0]) and NP.array_equal(b[:, 3], a[:, 0])
    assert not NP.array_equal(b[:, 1], b[:, 0])
    with pytest.raises(ValueError):
        RK.noise(rms, 77, bl_index=[1, 2, 3])


@pytest.fixture(scope='module')
def big_uniforms():
    """The uniforms of a 4100 x 1024 draw (the GPU suite's largest case), flattened."""
    f, g, t = RK.indices((1, 4100, 1024), 0, None)
    u1, u2 = RK.uniforms(RK.philox4x32_np(*RK.counter_key(f, g, t, RK.SEEDS[3])))
    return u1.ravel(), u2.ravel()


def test_fast_evaluation_against_exact(big_uniforms):
    """The numpy evaluation against mpmath on 2000 elements of a 4.2 M-element draw: the 200 with u2 nearest each of 0, 1/4, 1/2 and 3/4
    (the zeros of the components), the 200 smallest and the 200 largest u1 (the largest radii, and the radii that cancel in ln u1) and 800
    more.  Largest componentwise relative deviation measured: 3.97 u (u = 2^-53; 3.97 u near the zeros too); RK.FAST_SLACK = 8 u is held here with its margin of 2."""
    u1, u2 = big_uniforms
    assert u1.size == 4100 * 1024 and u1.min() > 0.0 and u1.max() <= 1.0 and u2.min() >= 0.0 and u2.max() < 1.0
    pick = [NP.argpartition(NP.abs(u2 - z), 200)[:200] for z in (0.0, 0.25, 0.5, 0.75)]
    pick[0] = NP.concatenate((pick[0][:100], NP.argpartition(1.0 - u2, 100)[:100]))             # the zero at 0 from both sides
    pick += [NP.argpartition(u1, 200)[:200], NP.argpartition(-u1, 200)[:200], NP.random.default_rng(11).choice(u1.size, 800, replace=False)]
    idx = NP.concatenate(pick)
    assert idx.size == 2000
    rms = NP.random.default_rng(12).uniform(0.5, 2.0, idx.size)
    exact = RK.box_muller_exact(u1[idx], u2[idx], rms)[0]
    fast = RK.box_muller_fast(u1[idx], u2[idx], rms)[0]
    dev = RK.deviation(fast, exact)
    near = RK.deviation(fast[:800], exact[:800])
    print('fast against exact: %.2f u over all, %.2f u near the zeros' % (dev, near))
    assert 2.0 * dev <= RK.FAST_SLACK


# ---- the comparison must be able to fail ----------------------------------------------------------------------------------------
def _rounded_angle(u1, u2, rms):
    """cos and sin of fl(fl(2 pi) * u2): everything else exact"""
    import mpmath
    out = NP.empty(u1.shape, dtype=NP.complex128)
    with mpmath.workprec(160):
        for i in NP.ndindex(u1.shape):
            a = mpmath.mpf(float(rms[i])) * mpmath.mpf(RK.INV_SQRT2) * mpmath.sqrt(-2 * mpmath.log(mpmath.mpf(float(u1[i]))))
            ang = mpmath.mpf((2.0 * math.pi) * float(u2[i]))
            out[i] = complex(float(a * mpmath.cos(ang)), float(a * mpmath.sin(ang)))
    return out


def restate(rms, seed, bl_offset=0, bl_index=None, rounds=10, mult=(RK.PHILOX_M0, RK.PHILOX_M1), weyl=(RK.PHILOX_W0, RK.PHILOX_W1),
            swap_ft=False, g_mask=2 ** 64 - 1, seed_mask=2 ** 64 - 1, shift=12, plus=1, factor=1.0, swap_parts=False, rounded_angle=False):
    """The draw put together from the checker's pieces, with one knob per way of getting it wrong."""
    f, g, t = RK.indices(rms.shape, bl_offset, bl_index)
    if swap_ft:
        f, t = t, f
    counter, key = RK.counter_key(f, g & NP.uint64(g_mask), t, (int(seed) & 0xFFFFFFFFFFFFFFFF) & seed_mask)
    u1, u2 = RK.uniforms(RK.philox4x32_np(counter, key, rounds=rounds, mult=mult, weyl=weyl), shift=shift, plus=plus)
    u1 = NP.maximum(u1, 2.0 ** -60)                                                             # plus = 0 can give 0: keep the log finite
    out = _rounded_angle(u1, u2, rms) if rounded_angle else RK.box_muller_fast(u1, u2, rms)[0]
    out = out * factor
    return out.imag + 1j * out.real if swap_parts else out


MUTANTS = {
    'nine rounds': dict(rounds=9),
    'multipliers exchanged': dict(mult=(RK.PHILOX_M1, RK.PHILOX_M0)),
    'key increment off by one bit': dict(weyl=(RK.PHILOX_W0 ^ 1, RK.PHILOX_W1)),
    'second key increment off by one bit': dict(weyl=(RK.PHILOX_W0, RK.PHILOX_W1 ^ (1 << 31))),
    'f and t exchanged': dict(swap_ft=True),
    'high word of g dropped': dict(g_mask=0xFFFFFFFF),
    'seed >> 32 unused': dict(seed_mask=0xFFFFFFFF),
    '>> 11': dict(shift=11),
    'no + 1 in u1': dict(plus=0),
    'rms / 2': dict(factor=math.sqrt(0.5)),
    'real and imaginary parts exchanged': dict(swap_parts=True),
    'product rounded before the cosine': dict(rounded_angle=True),
}
# where a mutant cannot show: a seed below 2^32 has no high word, a baseline below 2^32 neither
BLIND = {'seed >> 32 unused': lambda seed, off: seed < 2 ** 32, 'high word of g dropped': lambda seed, off: off + RK.SMALL_SHAPE[1] <= 2 ** 32}


@pytest.fixture(scope='module')
def small_refs():
    """The exact references of the GPU suite's small case: every seed at offset 0, and the offsets that reach the counter's high word."""
    rms = RK.small_rms()
    cases = [(seed, 0) for seed in RK.SEEDS] + [(RK.SEEDS[3], off) for off in RK.HIGH_OFFSETS]
    return rms, {c: RK.reference(rms, c[0], bl_offset=c[1], exact=True) for c in cases}


def test_small_case_shape_and_edges(small_refs):
    rms, refs = small_refs
    assert rms.shape == (3, 7, 37) and (rms == 0.0).sum() == 1 and (rms == 1e300).sum() == 1
    rest = rms[(rms != 0.0) & (rms != 1e300)]
    assert rest.min() >= 0.5 and rest.max() <= 2.0
    val = refs[(0, 0)][0]
    assert val[0, 0, 0] == RK.draw(0, 0, 0, 0, float(rms[0, 0, 0]), exact=True)
    assert NP.all(val[rms == 0.0] == 0.0) and NP.all(NP.isfinite(_parts(val)))
    assert not NP.array_equal(refs[(RK.SEEDS[3], RK.HIGH_OFFSETS[0])][0][:, :3], refs[(RK.SEEDS[3], RK.HIGH_OFFSETS[1])][0][:, :3])


def _parts(z):
    return NP.stack((z.real, z.imag), axis=-1)


def test_unmutated_restatement_is_accepted(small_refs):
    rms, refs = small_refs
    for (seed, off), ref in refs.items():
        assert NP.array_equal(restate(rms, seed, bl_offset=off), RK.noise(rms, seed, bl_offset=off))
        RK.assert_matches(restate(rms, seed, bl_offset=off), rms, seed, bl_offset=off, K=RK.FAST_SLACK, ref=ref)
        RK.assert_matches(ref[0], rms, seed, bl_offset=off, K=0, exact=False)                  # and the exact one passes the numpy comparison


@pytest.mark.parametrize('name', sorted(MUTANTS))
def test_every_mutant_is_rejected(small_refs, name):
    """At the ceiling K = 32 u, the widest bound the GPU suite may ever use: what is rejected here is rejected at any measured K."""
    rms, refs = small_refs
    seen = 0
    for (seed, off), ref in refs.items():
        if name in BLIND and BLIND[name](seed, off):
            continue
        if name == 'product rounded before the cosine' and seen:
            break                                                                               # mpmath throughout: one case is enough
        got = restate(rms, seed, bl_offset=off, **MUTANTS[name])
        with pytest.raises(AssertionError):
            RK.assert_matches(got, rms, seed, bl_offset=off, K=RK.K_CEILING, ref=ref)
        if name != 'product rounded before the cosine':
            with pytest.raises(AssertionError):                                                 # gross: the numpy comparison sees it too
                RK.assert_matches(got, rms, seed, bl_offset=off, K=RK.K_CEILING, exact=False)
        seen += 1
    assert seen >= 1


def test_rounded_angle_shows_only_near_the_zeros(small_refs):
    """fl(2 pi) u2, rounded, is off by up to 6e-16 rad: relative to the element's magnitude that is a few u and inside any bound; relative
    to a component that is a small part of that magnitude it is not.  So the exact, componentwise comparison tells it apart on the 777 elements of the
    small case, and only on components near a zero."""
    rms, refs = small_refs
    seed = RK.SEEDS[0]
    val, scale = refs[(seed, 0)]
    got = restate(rms, seed, rounded_angle=True)
    assert RK.deviation(got, val) > RK.K_CEILING
    assert RK.deviation(got, val, scale) <= 8.0                                                 # 6e-16 rad is 5.4 u
    with NP.errstate(divide='ignore', invalid='ignore'):
        rel = NP.abs(_parts(got) - _parts(val)) / NP.abs(_parts(val)) / RK.U
        frac = NP.abs(_parts(val)) / scale[..., NP.newaxis]
    big = NP.nan_to_num(rel) > RK.K_CEILING
    assert big.sum() >= 3 and NP.all(frac[big] < 0.25)                                          # 8 u of the magnitude is 32 u of a quarter of it


def test_comparison_rejects_nan_shape_and_nonzero_at_zero_rms(small_refs):
    rms, refs = small_refs
    ref = refs[(0, 0)]
    bad = ref[0].copy()
    bad[rms == 0.0] = 1e-300
    with pytest.raises(AssertionError):
        RK.assert_matches(bad, rms, 0, ref=ref)
    bad = ref[0].copy()
    bad[0, 0, 0] = complex(NP.nan, 0.0)
    for exact in (True, False):
        with pytest.raises(AssertionError):
            RK.assert_matches(bad, rms, 0, ref=ref, exact=exact)
    with pytest.raises(AssertionError):
        RK.assert_matches(ref[0][:, :6], rms, 0, ref=ref)
    one = ref[0].copy()
    one.real[2, 2, 2] *= 1.0 + 40 * 2.0 ** -53                                                  # one component 40 u off
    with pytest.raises(AssertionError):
        RK.assert_matches(one, rms, 0, ref=ref)
    assert RK.assert_matches(ref[0], rms, 0, ref=ref) == 0.0
