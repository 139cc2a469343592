"""CPU: the 40-digit sky-sum reference (tests/skyvis_reference.py) held to its own exact properties and to its second route, and the
floor of the two fp64 restatements (oracle/skyvis_oracle.py, oracle/skyvis_oracle.c) against it on every case set the GPU tests use."""
import numpy as NP
import pytest

import skyvis_reference as R
from oracle import skyvis_oracle as O, c_oracle as CO


def _families():
    fam = {}
    for name in R.CASES:
        key = name if name.startswith('len_') else name.split('_')[0] + ('_taper' if name.endswith('_taper') or '_taper_' in name else '')
        if name.startswith('taper_'):
            key = 'taper'
        fam.setdefault(key, []).append(name)
    return fam


FAMILIES = _families()


# ---- the two routes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', sorted(FAMILIES))
def test_integer_reduced_longdouble_route_agrees_with_mpmath(family):
    """Every case: the route the tests use against every term in mpmath at 40 digits, on a seeded sub-sample of the outputs, V and G."""
    worst = 0.0
    for name in FAMILIES[family]:
        c, r = R.get(name)
        worst = max(worst, R.route_gap(c, r, nsample=6 if c.dc.shape[0] > 60 else 12, seed=len(name)))
    print('route gap %-24s %.2e of S_f' % (family, worst))
    assert worst <= R.ROUTE_GAP


# ---- exact properties ----------------------------------------------------------------------------------------------------------------
def test_single_source_at_the_phase_centre_gives_pbflux_exactly():
    c, _ = R.get('edges')
    pb = c.pb[:1]
    for fw in (None, NP.array([0.7])):
        r = R.reference(c.bl, c.ch, R.PC[None, :], pb, R.PC, fw)
        if fw is None:
            assert NP.array_equal(r.V, NP.broadcast_to(pb.astype(NP.complex128), r.V.shape))      # every baseline, the zero vector too
        assert NP.array_equal(r.V[0], pb[0].astype(NP.complex128))                                # b = 0: w = 1 under any taper
        assert NP.all(r.V.imag == 0.0)


def test_negated_baselines_give_the_conjugate_bit_for_bit():
    for name in ('len_3e6_taper', 'edges_taper', 'ragged'):
        c, r = R.get(name)
        m = R.reference(-c.bl[:9], c.ch, c.dc, c.pb, c.pc, c.fw)
        assert NP.array_equal(m.V, NP.conj(r.V[:9])) and NP.array_equal(m.G, NP.conj(r.G[:, :9])), name
    c, r = R.get('edges')
    assert NP.array_equal(r.V[3], NP.conj(r.V[7]))                                                # the set's own negated row


def test_a_zero_flux_source_changes_nothing():
    c, r = R.get('edges_taper')
    keep = NP.arange(c.dc.shape[0]) != 8
    assert not NP.any(c.pb[8])
    m = R.reference(c.bl, c.ch, c.dc[keep], c.pb[keep], c.pc, c.fw[keep])
    assert NP.array_equal(m.V, r.V) and NP.array_equal(m.G, r.G) and NP.array_equal(m.S, r.S)


def test_taper_tends_to_one_as_fwhm_tends_to_zero():
    c, r = R.get('taper_0')
    assert NP.array_equal(r.V, R.reference(c.bl, c.ch, c.dc, c.pb, c.pc, None).V)                 # fwhm = 0: w = 1 exactly
    gaps = []
    for fw in (1e-3, 1e-5, 1e-7):
        m = R.reference(c.bl, c.ch, c.dc, c.pb, c.pc, NP.full(c.dc.shape[0], fw))
        gaps.append(float(NP.max(NP.abs(m.V - r.V) / r.S)))
    # 1 - w <= kappa (|b| f / c)^2 = ln 2 (fwhm |b| f / c)^2: 1.2 km at 203 MHz is 813 wavelengths
    for fw, gap in zip((1e-3, 1e-5, 1e-7), gaps):
        assert gap <= NP.log(2.0) * (NP.radians(fw) * 813.0) ** 2 * 1.01 + 2e-16, (fw, gap)
    assert gaps[0] > gaps[1] > gaps[2] and gaps[2] < 2e-12


def test_clamp_holds_where_the_exact_expression_is_negative():
    """A source exactly along a baseline whose doubles are longer than a unit vector: |b|^2 - (b.s)^2 < 0, w = 1 by the clamp."""
    b = NP.array([[3.0, 4.0, 0.0]])
    s = NP.array([[0.6000000000000001, 0.8000000000000002, 0.0]])
    p = NP.ones((1, 3))
    ch = R.CH33[:3]
    assert NP.array_equal(R.reference(b, ch, s, p, R.PC, NP.array([30.0])).V, R.reference(b, ch, s, p, R.PC, None).V)


# ---- the floor of both oracles -------------------------------------------------------------------------------------------------------
def _oracle_errors(name):
    c, r = R.get(name)
    out = {}
    with NP.errstate(all='ignore'):
        got = {'numpy': O.skyvis(c.bl, c.ch, c.dc, c.pb, c.pc, fwhm_deg=c.fw, gradient=True),
               'C': CO.skyvis(c.bl, c.ch, c.dc, c.pb, c.pc, fwhm_deg=c.fw, gradient=True)}
    s = NP.where(r.S > 0.0, r.S, 1.0)[None, :]
    for which, (v, g) in got.items():
        err = NP.maximum(NP.abs(v - r.V), NP.max(NP.abs(g - r.G), axis=0)) / s
        out[which] = err
    return r, out


@pytest.mark.parametrize('family', sorted(FAMILIES))
def test_oracle_floor_and_derived_bound(family):
    """Both oracles against the reference on every set: inside (1e-11 + 2 pi R_ORACLE u N_abs) S_f everywhere -- the rule of
    skyvis_reference.py with the oracle's own rounding count and scale -- and inside the plain 1e-11 up to the 30 km decade only.
    The numpy restatement keeps the upstream NaN where |b|^2 - (c tau)^2 rounds below zero (a source along a baseline): those terms are
    the C oracle's alone."""
    worst = {'numpy': 0.0, 'C': 0.0}
    for name in FAMILIES[family]:
        r, errs = _oracle_errors(name)
        bound = R.f64_bound(R.R_ORACLE, r.Nabs)
        for which, err in errs.items():
            if which == 'numpy' and NP.any(NP.isnan(err)):
                assert 'edges_taper' in name, name
                continue
            assert NP.all(NP.isfinite(err)), (name, which)
            assert NP.all(err <= bound), (name, which, float(NP.max(err / bound)))
            worst[which] = max(worst[which], float(err.max()))
    print('oracle floor %-24s numpy %.1e | C %.1e' % (family, worst['numpy'], worst['C']))
    if family in R.ORACLE_KEEPS or family[:-6] in R.ORACLE_KEEPS:
        assert max(worst.values()) <= R.BAR_F64
    elif family in R.ORACLE_LOSES:
        assert min(worst.values()) > R.BAR_F64           # the oracle is no reference at this length: what the device is held to is above


def test_case_sets_are_built_as_stated():
    for name in R.CASES:
        c, r = R.get(name)
        assert r.V.shape == (c.bl.shape[0], c.ch.size) and r.G.shape == (3,) + r.V.shape
    c, _ = R.get('len_3e2')
    assert c.bl.shape == (70, 3) and c.ch.size == 33 and c.dc.shape[0] == 21
    c, _ = R.get('ragged')
    assert (c.bl.shape[0], c.ch.size, c.dc.shape[0]) == (257, 65, 5)
    c, _ = R.get('edges')
    assert (c.bl.shape[0], c.ch.size) == (12, 17) and NP.signbit(c.dc[3, 2]) and not NP.signbit(c.dc[2, 2]) and c.dc[4, 2] < 0.0
    c, _ = R.get('taper_mixed')
    x = NP.log(2.0) * (2.0 * NP.sin(NP.radians(NP.asarray(R.TAPER_FWHM)) / 2.0)) ** 2 * (1200.0 * c.ch.max() / R.C_LIGHT) ** 2
    assert x[2] < 18.0 < x[3] < 28.0 < x[4] and x[-1] > 800.0         # the cull thresholds are straddled, exp_tab_front's clamp is passed
