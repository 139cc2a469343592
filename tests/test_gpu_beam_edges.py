"""The analytic primary beams on the device (k_beam_flux<KIND>, k_beam_flux_plain<KIND>; prisim_amd/csrc/aux_kernels.hip) against the
40-digit reference of tests/beam_reference.py, with sources placed on the edges:
  dishes (Airy and Gaussian; D = 0.5, 14, 300 m; zenith and alt 70 / az 200 pointing): the pointing itself, offsets either side of the
    small-angle floor sin 1e-10, the first three zeros of J1 at the middle channel and the next double, 1 rad off axis, z = 5e-324,
    z = +-0.0, alt 1e-14, 1e-7 and -1e-9 degrees, seeded directions -- plain, and under an array factor and a ground plane;
  dipoles (three lengths, two axes, three modes): the axis and its opposite, rotations off it either side of 1 - |dot| = 1e-10;
  array factors (4 x 4, 4 x 3, 5 x 2): |phi| either side of 1e-10, the grating lobes and displacements of 1e-14 ... 1e-3 from them;
  ground planes with and without the modifier, down to the horizon;
  the flux factor as a power law and as a table; and two launches whose grid-stride loop takes a second and a sixteenth step.

The rule (beam_reference: THE RULE): |got - reference| <= 1e-12 on every power value, |got - reference x flux| <= 1e-12 x flux with a
flux, output finite everywhere, blank elements exactly 0.0, nothing excused."""
import math

import numpy as NP
import pytest

import beam_reference as R
from prisim_amd import _abi

pytestmark = pytest.mark.gpu

ZEN = NP.array([0.0, 0.0, 1.0])
LD = R.LD
KINDS = {'delta': _abi.PRISIM_BEAM_DELTA, 'gaussian': _abi.PRISIM_BEAM_GAUSSIAN, 'airy': _abi.PRISIM_BEAM_AIRY, 'dipole': _abi.PRISIM_BEAM_DIPOLE}
MODES = {'short': _abi.PRISIM_DIPOLE_SHORT, 'halfwave': _abi.PRISIM_DIPOLE_HALFWAVE, 'general': _abi.PRISIM_DIPOLE_GENERAL}


def _ext(spec):
    ext = {}
    if spec.kind == 'dipole':
        ext.update(dipole_dircos=list(spec.dipole_axis), dipole_mode=MODES[spec.dipole_mode])
    if spec.array is not None:
        a = spec.array
        ext['array'] = dict(nax1=a.nax1, nax2=a.nax2, sep1=a.sep1, sep2=a.sep2, east2ax1=a.east2ax1, pointing_dircos=list(a.pointing))
    if spec.ground is not None:
        g = spec.ground
        ext['ground'] = dict(height=g.height, modifier=None if g.scale is None else dict(scale=g.scale, max=g.max))
    return ext or None


def _device(spec, dircos, freqs, flux_ref=None, spindex=None, ref_freq=150e6, flux_spectrum=None):
    """set_array (one baseline), set_sky_analytic (unit flux, spindex 0 unless given), get_pbflux; in a context of its own."""
    n = dircos.shape[0]
    with _abi.Context(0) as ctx:
        ctx.set_array(NP.array([[14.6, 0.0, 0.0]]), freqs, nt_max=1)
        ctx.set_sky_analytic(dircos, NP.ones(n) if flux_ref is None else flux_ref, NP.zeros(n) if spindex is None else spindex, ref_freq,
                             KINDS[spec.kind], spec.size, NP.asarray(spec.pointing), ZEN, flux_spectrum=flux_spectrum, ext=_ext(spec))
        return ctx.get_pbflux()


def _hold(case, got, rows=None):
    """The rule on a unit-flux run.  rows: print these rows' deviations apart."""
    assert got.shape == case.ref.shape
    assert NP.all(NP.isfinite(got)), case.name
    dev = R.deviation(got, case.ref)
    i, j = NP.unravel_index(int(NP.argmax(dev)), dev.shape)
    print('%-44s %2d x %d  worst |got - reference| %.3e at row %d (%s), channel %d' % (case.name, got.shape[0], got.shape[1], dev[i, j], i, case.labels[i], j))
    for r in NP.flatnonzero(rows) if rows is not None else ():
        print('    %-36s %.3e' % (case.labels[r], dev[r].max()))
    assert NP.all(got[case.blank] == 0.0), case.name
    assert dev.max() <= R.BOUND, (case.name, case.labels[i], float(dev[i, j]))


@pytest.mark.parametrize('extras', [False, True], ids=['plain', 'array_ground'])
@pytest.mark.parametrize('kind,diameter,pointing', R.DISH_CASES, ids=['%s-%g-%s' % c for c in R.DISH_CASES])
def test_dish(kind, diameter, pointing, extras):
    """plain: k_beam_flux_plain<AIRY | GAUSSIAN>; array_ground: k_beam_flux<KIND> under a 4 x 4, 1.1 m array factor pointed at the
    beam's pointing and a 0.3 m ground plane."""
    case = R.dish_case(kind, diameter, pointing, extras)
    _hold(case, _device(case.spec, case.dircos, case.freqs))


@pytest.mark.parametrize('length,axis,mode', R.DIPOLE_CASES, ids=['%g-%s-%s' % c for c in R.DIPOLE_CASES])
def test_dipole(length, axis, mode):
    case = R.dipole_case(length, axis, mode)
    _hold(case, _device(case.spec, case.dircos, case.freqs))


@pytest.mark.parametrize('arr', R.ARRAYS, ids=lambda a: '%dx%d' % a[:2])
def test_array_factor(arr):
    """The grating-lobe rows of an axis with nax 3 or 5 are where sin(n phi/2) / sin(phi/2), taken literally, is noise in fp64
    (test_beam_reference.py::test_oracle_array_factor): the kernel reduces the phase to cycles first, and is held there like anywhere."""
    case = R.array_case(*arr)
    _hold(case, _device(case.spec, case.dircos, case.freqs), rows=R.noisy_lobe_rows(case)[0])


@pytest.mark.parametrize('height,modifier', R.GROUND_CASES, ids=['%g-%s' % (h, 'modified' if m else 'bare') for h, m in R.GROUND_CASES])
def test_ground_plane(height, modifier):
    case = R.ground_case(height, modifier)
    _hold(case, _device(case.spec, case.dircos, case.freqs))


def _hold_flux(name, got, ref, flux, blank):
    assert NP.all(NP.isfinite(got)), name
    dev = (NP.abs(got.astype(LD) - ref * flux) / flux).astype(NP.float64)
    i, j = NP.unravel_index(int(NP.argmax(dev)), dev.shape)
    print('%-44s %6d x %2d  worst |got - reference x flux| / flux %.3e at row %d, channel %d' % (name, got.shape[0], got.shape[1], dev[i, j], i, j))
    assert NP.all(got[blank] == 0.0), name
    assert dev.max() <= R.BOUND, (name, int(i), int(j), float(dev[i, j]))
    return dev


@pytest.mark.parametrize('form', ['power_law', 'table'])
def test_flux(form):
    """Airy D = 14 m off zenith, seeded flux_ref in [0.1, 10] and spindex in [-3, 1] (every fifth row 0), ref_freq the middle channel:
    every element to the flux bound; the middle channel -- and every channel of a spindex-0 row -- is beam x flux_ref exactly, `beam`
    being the device's own unit-flux value.  table: the same fluxes handed over as flux_spectrum, every element exactly beam x table."""
    case = R.dish_case('airy', 14.0, 'offzenith')
    n = len(case.labels)
    rng = NP.random.default_rng(14)
    flux_ref, spindex, ref_freq = rng.uniform(0.1, 10.0, n), rng.uniform(-3.0, 1.0, n), float(case.freqs[R.MID])
    spindex[::5] = 0.0
    unit = _device(case.spec, case.dircos, case.freqs)
    _hold(case, unit)
    assert NP.count_nonzero(~case.blank) >= n - 4
    if form == 'power_law':
        got = _device(case.spec, case.dircos, case.freqs, flux_ref, spindex, ref_freq)
        _hold_flux('power law', got, case.ref, R.flux(flux_ref, spindex, ref_freq, case.freqs), case.blank)
        assert NP.array_equal(got[:, R.MID], unit[:, R.MID] * flux_ref)
        assert NP.array_equal(got[::5], unit[::5] * flux_ref[::5, None])
    else:
        table = flux_ref[:, None] * (case.freqs[None, :] / ref_freq) ** spindex[:, None]
        got = _device(case.spec, case.dircos, case.freqs, flux_spectrum=table, ref_freq=None)
        _hold_flux('table', got, case.ref, table.astype(LD), case.blank)
        assert NP.array_equal(got, unit * table)


@pytest.mark.parametrize('nsrc,nchan', R.LAUNCH_SHAPES, ids=['20011x17', '70001x61'])
def test_launch_geometry(nsrc, nchan):
    """20011 x 17 = 340187 elements on 1037 blocks (1024 rounded up to whole periods of 17): the first 74715 threads take a second step.
    70001 x 61 = 4270061 elements on 1098 blocks: 15 to 16 steps a thread.  Every element of every step is held to the flux bound; the
    rows are a seeded draw, with repeats, from the Airy D = 14 m set, the reference computed on the distinct directions."""
    case, rows, flux_ref, spindex, ref_freq = R.launch_case(nsrc, nchan)
    total = nsrc * nchan
    g = (total + 255) // 256
    period = nchan // math.gcd(nchan, 256)
    blocks = -(-min(max((g + 15) // 16, min(g, 1024)), 16384) // period) * period               # beam_grid(total, nchan, 16384, 1)
    assert blocks == {(20011, 17): 1037, (70001, 61): 1098}[(nsrc, nchan)] and (blocks * 256) % nchan == 0
    assert (total - 1) // (blocks * 256) == {(20011, 17): 1, (70001, 61): 15}[(nsrc, nchan)]     # the last thread's extra steps
    got = _device(case.spec, NP.ascontiguousarray(case.dircos[rows]), case.freqs, flux_ref, spindex, ref_freq)
    assert got.shape == (nsrc, nchan)
    dev = _hold_flux(case.name, got, case.ref[rows], R.flux(flux_ref, spindex, ref_freq, case.freqs), case.blank[rows])
    first = blocks * 256 // nchan
    for lab, r in (('first row of the second pass', first), ('last row', nsrc - 1)):
        print('    %-30s row %5d (%s)  %.3e' % (lab, r, case.labels[rows[r]], dev[r].max()))
