"""The external HEALPix beam on the device (k_extbeam_table, k_extbeam_gather, k_colmax_partial, k_colmax_final, k_extbeam_finish) against
the 40-digit reference of tests/extbeam_reference.py, with sources placed on the edges: poles, the |z| = 2/3 change of zone, ring and
pixel boundaries, the azimuth wrap, a channel past 256 and a source past the gather's 16384-block grid.

The rule (extbeam_reference.judge): every element is float32(reference) bit for bit, except where the reference lies within DELTA
(relative; 8 x the measured floor of the fp64 restatement) of a float32 rounding midpoint -- there one float32 ulp either way is allowed,
for at most 1e-3 of the elements of a case."""
import numpy as NP
import pytest

import extbeam_reference as R
from prisim_amd import _abi

pytestmark = pytest.mark.gpu

ZEN = NP.array([0.0, 0.0, 1.0])
LD = R.LD


def _device(dc, beam, m, res, fluxes=None, law=None):
    """set_array (one baseline), set_external_beam, set_sky_external (unit fluxes unless given) at a zenith phase centre, get_pbflux.
    Beforehand, on the reference: no expected value is a float32 subnormal."""
    assert float(NP.min(res['ref'])) >= 1e-30
    nchan = m.shape[0]
    ch = 150e6 + 1e5 * NP.arange(nchan)
    with _abi.Context(0) as ctx:
        ctx.set_array(NP.array([[14.6, 0.0, 0.0]]), ch, nt_max=1)
        ctx.set_external_beam(beam, m)
        if law is not None:
            ctx.set_sky_external_analytic(dc, law[0], law[1], law[2], ZEN)
        else:
            ctx.set_sky_external(dc, NP.ones((dc.shape[0], nchan)) if fluxes is None else fluxes, ZEN)
        return ctx.get_pbflux(), ch


def _hold(name, got, res):
    assert got.shape == res['f32'].shape
    failed, excused, worst = R.judge(got, res)
    print('%-18s %6d x %3d  failed %d  excused %d  worst |got / reference - 1| %.3e (float32 storage: up to 6e-8 when right)'
          % (name, got.shape[0], got.shape[1], failed, excused, worst))
    if failed:
        bad = NP.argwhere(got.astype(NP.float32) != res['f32'])
        print('first rows off:', [(int(s), int(c), float(got[s, c]), float(res['ref'][s, c])) for s, c in bad[:8]])
    assert failed == 0, name
    assert excused <= R.EXCUSED_SHARE * got.size, name


@pytest.mark.parametrize('nside', R.NSIDES)
def test_edges(nside):
    dc, beam, m, res = R.case_nside(nside)
    got, _ = _device(dc, beam, m, res)
    _hold('nside %d' % nside, got, res)
    assert NP.all(got[:, 3] == 1.0)                                 # the all-zero row of M


def test_wide_257_channels():
    """The gather's channel loop runs a second time for one channel; k_colmax_final gets eight full 32-channel tiles and a ragged one."""
    dc, beam, m, res = R.case_wide()
    got, _ = _device(dc, beam, m, res)
    _hold('wide', got, res)


@pytest.mark.parametrize('target_row', [-1, 16384], ids=['last_row', 'first_row_of_the_second_pass'])
def test_many_sources_past_the_gather_grid(target_row):
    """16384 + 37 sources, so the gather's 16384 blocks take a second grid pass (rows 16384 ..): every row of both passes is held to the
    reference.  The column maximum sits on one row only -- the last, or the first of the second pass -- and has to reach every row
    through the 256 strided partial blocks.  (One run does not show that the loop's barriers are sufficient; that is read in the code.)"""
    dc, beam, m, res, target = R.case_many(target_row)
    got, _ = _device(dc, beam, m, res)
    _hold('many, row %d' % target, got, res)
    assert got[target, 0] == 1.0 and NP.all(NP.delete(got[:, 0], target) < 1.0)


@pytest.mark.parametrize('form', ['table', 'power_law'])
def test_flux_forms(form):
    """Where the beam is float32(reference), beam x flux equals float32(reference) x flux (formed in longdouble) to 1e-12 relative."""
    dc, beam, m, res = R.case_nside(3)
    rng = NP.random.default_rng(303)
    unit, ch = _device(dc, beam, m, res)
    match = unit.astype(NP.float32) == res['f32']
    assert NP.count_nonzero(~match) <= R.EXCUSED_SHARE * match.size
    if form == 'table':
        fl = rng.uniform(0.1, 10.0, unit.shape)
        got, _ = _device(dc, beam, m, res, fluxes=fl)
        flux = fl.astype(LD)
    else:
        flux_ref, spindex, ref_freq = rng.uniform(0.1, 10.0, dc.shape[0]), rng.uniform(-1.5, 0.5, dc.shape[0]), 150.3e6
        got, _ = _device(dc, beam, m, res, law=(flux_ref, spindex, ref_freq))
        flux = flux_ref.astype(LD)[:, None] * NP.power((ch.astype(LD) / LD(ref_freq))[None, :], spindex.astype(LD)[:, None])
    want = res['f32'].astype(LD) * flux
    dev = NP.abs(got.astype(LD) - want) / want
    print('%-10s worst deviation of beam x flux where the beam matches: %.3e' % (form, float(NP.max(dev[match]))))
    assert float(NP.max(dev[match])) <= 1e-12
