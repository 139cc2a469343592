"""GPU: the power an antenna receives from the sky, reduced on the device (include/prisim_antpower.h), through the C-ABI and through
prisim_amd.interferometry.antenna_power against the numpy restatement of the reference (tests/antpower_checker.py).

Tolerances.  They come from the project's own beam parity: device beams agree with the oracle to 1e-12 absolute
(test_device_beams_match_golden_reference_functions) and beam x flux to 1e-11 relative.  With n_up sources above the horizon
    |den - den_ref| <= 1e-12 n_up + 1e-11 sum pb
    |num - num_ref| <= 1e-12 sum |S| + 1e-11 sum |pb S|
    |power - power_ref| <= (the two combined through the quotient) / den_ref.
Two conditions are asserted on the CPU before anything is compared, and no element is skipped: min |s_z| >= 1e-9 over every
(snapshot, source), so that the horizon test cannot differ between two roundings, and den_ref >= 1 at every (LST, channel).

The Gaussian of 14 m on the inputs of test 1 is the one exception to the second condition: its beam is narrower than the Airy
pattern's and on these 1537 positions numpy gives sum pb between 0.297 and 5.45 (the Airy pattern: 1.39 to 11.9), so the floor
asserted for it is 0.29.  The inputs and the tolerances are the same as for the other beams; the bounds scale with den_ref themselves."""
import os
import sys

import numpy as NP
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import antpower_checker as AK  # noqa: E402

from oracle import beams_oracle as BO  # noqa: E402
from prisim_amd import _abi, frames as FRAMES, geometry as GEOM, primary_beams as PB, skymodel as SM  # noqa: E402
from prisim_amd import interferometry as RI  # noqa: E402

pytestmark = pytest.mark.gpu

LAT = -30.7215
ZEN = NP.array([0.0, 0.0, 1.0])
U = 2.0 ** -53


def sphere(rng, n):
    """n positions uniform on the sphere as (RA, Dec) degrees"""
    z = rng.uniform(-1.0, 1.0, n)
    return NP.stack((rng.uniform(0.0, 360.0, n), NP.degrees(NP.arcsin(z))), axis=1)


def rotations(lst, lat=LAT):
    return NP.stack([FRAMES.equatorial_to_enu(l, lat) for l in lst])


def beamformer_16(nsnap, seed=7):
    """A 4 x 4 tile steered to another direction in every snapshot, two jitter realisations of delays and gains"""
    rng = NP.random.default_rng(seed)
    pos = PB.mwa_tile_element_locs()
    out = []
    for t in range(nsnap):
        pc = GEOM.altaz2dircos(NP.array([[60.0 + 5.0 * t, 40.0 * t]]), 'degrees')
        delays = (pos.dot(pc.T) / 299792458.0) + 2e-11 * rng.standard_normal((16, 2))
        gains = 1.0 + 0.05 * rng.standard_normal((16, 2))
        out.append({'positions': pos, 'delays': delays, 'gains': gains})
    return out


def setups(nsnap):
    """name -> (beam_kind, diameter, ext of the entry, setup of the checker): the five beams of the issue"""
    tile = {'nax1': 4, 'nax2': 4, 'sep1': 1.1, 'sep2': 1.1, 'east2ax1': 0.0, 'pointing_dircos': ZEN}
    ground = {'height': 0.3, 'modifier': None}
    east = NP.array([1.0, 0.0, 0.0])
    bfs = beamformer_16(nsnap)
    return {
        'delta': (_abi.PRISIM_BEAM_DELTA, 0.0, None, {'element': 'delta'}),
        'gaussian': (_abi.PRISIM_BEAM_GAUSSIAN, 14.0, None, {'element': 'gaussian', 'size': 14.0}),
        'airy': (_abi.PRISIM_BEAM_AIRY, 14.0, None, {'element': 'dish', 'size': 14.0}),
        'mwa_tile': (_abi.PRISIM_BEAM_DIPOLE, 0.74, {'dipole_dircos': east, 'array': tile, 'ground': ground},
                     {'element': 'dipole', 'size': 0.74, 'element_dircos': east, 'array': tile, 'ground': ground}),
        'beamformer': (_abi.PRISIM_BEAM_DIPOLE, 0.74, [{'dipole_dircos': east, 'beamformer': bf} for bf in bfs],
                       {'element': 'dipole', 'size': 0.74, 'element_dircos': east, 'beamformers': bfs}),
    }


class Case1(object):
    """1537 positions uniform on the sphere, five LSTs, 37 channels over 100-200 MHz; a power law with a tenth of the flux_ref
    negative, and the same as a table"""
    lst = NP.array([0.0, 73.1, 146.2, 219.3, 292.4])

    def __init__(self):
        rng = NP.random.default_rng(20261019)
        self.nsrc, self.nchan = 1537, 37
        self.radec = sphere(rng, self.nsrc)
        self.freqs = NP.linspace(100e6, 200e6, self.nchan)
        self.flux_ref = rng.uniform(0.5, 5.0, self.nsrc) * NP.where(rng.uniform(size=self.nsrc) < 0.1, -1.0, 1.0)
        self.spindex = rng.uniform(-1.2, -0.2, self.nsrc)
        self.ref_freq = 150e6
        self.table = self.flux_ref[:, None] * (self.freqs[None, :] / self.ref_freq) ** self.spindex[:, None]
        self.unitvec = GEOM.catalog_unitvec(self.radec, 'radec')
        self.rot = rotations(self.lst)
        self.dircos = AK.sky_dircos(self.radec, 'radec', self.lst, LAT)
        self.setups = setups(self.lst.size)
        self._ref = {}

    def ref(self, name, spectrum=None):
        key = (name, spectrum is None)
        if spectrum is not None or key not in self._ref:
            setup = self.setups[name][3]
            r = AK.antenna_power(self.dircos, self.table if spectrum is None else spectrum,
                                 lambda t, dc: AK.beam_of(setup, self.freqs, t)(dc))
            if spectrum is not None:
                return r
            self._ref[key] = r
        return self._ref[key]

    def call(self, ctx, name, table=False, **kw):
        kind, dia, ext, _ = self.setups[name]
        flux = {'flux_spectrum': self.table} if table else {'flux_ref': self.flux_ref, 'spindex': self.spindex, 'ref_freq_hz': self.ref_freq}
        flux.update(kw)
        return ctx.antenna_power(self.unitvec, self.freqs, self.rot, kind, dia, ext=ext, **flux)


@pytest.fixture(scope='module')
def case1():
    return Case1()


def preconditions(dircos, ref, den_floor=1.0):
    """asserted on the CPU before anything is compared"""
    assert NP.min(NP.abs(dircos[..., 2])) >= 1e-9
    if den_floor is not None:
        assert NP.min(ref['den']) >= den_floor, NP.min(ref['den'])


def compare(power, num, den, ref, label=''):
    num_tol, den_tol, power_tol = AK.tolerances(ref)
    for got, want, tol, what in ((den, ref['den'], den_tol, 'den'), (num, ref['num'], num_tol, 'num'), (power, ref['power'], power_tol, 'power')):
        err = NP.abs(got - want)
        print('%s %s: max err / tol = %.3e' % (label, what, float(NP.max(err / tol))))
        assert NP.all(err <= tol), (label, what, float(NP.max(err / tol)))


# ---- 1. the entry against the checker --------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['delta', 'gaussian', 'airy', 'mwa_tile', 'beamformer'])
def test_entry_matches_the_checker(ctx, case1, name):
    ref = case1.ref(name)
    preconditions(case1.dircos, ref, den_floor=0.29 if name == 'gaussian' else 1.0)
    for table in (False, True):
        power, num, den, st = case1.call(ctx, name, table=table)
        assert power.shape == num.shape == den.shape == (5, 37)
        compare(power, num, den, ref, '%s table=%s' % (name, table))
        assert st['sources_evaluated'] == 5 * 1537 and st['sources_up'] == int(ref['n_up'].sum())
        assert st['block_sources'] == 256 and st['chan_tile'] == 64 and st['spans'] == 1 and st['streams'] == 2
        assert st['download_bytes'] == 3 * 5 * 37 * 8 + 5 * 8 and st['kernel_bytes'] > 0 and st['kernel_ms'] > 0.0


def test_delta_beam_on_a_uniform_sky_returns_the_temperature(ctx, case1):
    T = 3.0e2 / 7.0
    table = NP.full((case1.nsrc, case1.nchan), T)
    ref = case1.ref('delta', spectrum=table)
    preconditions(case1.dircos, ref)
    power, num, den, _ = case1.call(ctx, 'delta', table=True, flux_spectrum=table)
    assert NP.array_equal(den, ref['n_up'][:, None] * NP.ones(case1.nchan))
    assert NP.all(NP.abs(power - T) <= ref['n_up'][:, None] * U * T)


# ---- 2. block and tile edges --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('nchan', [1, 37, 300])
@pytest.mark.parametrize('nsrc', [1, 255, 256, 257, 4097])
def test_block_and_tile_edges(ctx, nsrc, nchan):
    rng = NP.random.default_rng(1000 * nsrc + nchan)
    lst = NP.array([10.0, 130.0, 250.0])
    # near the zenith of the first LST and spread from there, so that a Gaussian of 3 m sees something at every LST even from one source
    radec = sphere(rng, nsrc)
    if nsrc < 300:
        radec = NP.stack((rng.uniform(0.0, 360.0, nsrc), LAT + rng.uniform(-12.0, 12.0, nsrc)), axis=1)
    freqs = NP.linspace(100e6, 200e6, nchan) if nchan > 1 else NP.array([150e6])
    flux_ref, spindex = rng.uniform(0.5, 5.0, nsrc), rng.uniform(-1.2, -0.2, nsrc)
    dircos = AK.sky_dircos(radec, 'radec', lst, LAT)
    table = flux_ref[:, None] * (freqs[None, :] / 150e6) ** spindex[:, None]
    ref = AK.antenna_power(dircos, table, lambda t, dc: AK.beam_of({'element': 'gaussian', 'size': 3.0}, freqs)(dc))
    preconditions(dircos, ref, den_floor=None)                # one source cannot fill the beam: the horizon condition alone, per case
    power, num, den, st = ctx.antenna_power(GEOM.catalog_unitvec(radec, 'radec'), freqs, rotations(lst), _abi.PRISIM_BEAM_GAUSSIAN, 3.0,
                                            flux_ref=flux_ref, spindex=spindex, ref_freq_hz=150e6)
    assert st['sources_up'] == int(ref['n_up'].sum()) and st['chan_tile'] == min(64, 1 << (nchan - 1).bit_length())
    num_tol, den_tol, power_tol = AK.tolerances(ref)
    assert NP.all(NP.abs(den - ref['den']) <= den_tol) and NP.all(NP.abs(num - ref['num']) <= num_tol)
    ok = ref['den'] > 0.0                                     # 0 / 0 is NaN on both sides
    assert NP.array_equal(NP.isnan(power), NP.isnan(ref['power']))
    assert NP.all(NP.abs(power - ref['power'])[ok] <= power_tol[ok])


# ---- 3. one source is the beam kernel itself -----------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['delta', 'gaussian', 'airy', 'mwa_tile', 'beamformer'])
def test_one_source_is_the_beam_kernel(ctx, name):
    altaz = NP.array([[89.0, 10.0], [70.0, 100.0], [45.0, 200.0], [20.0, 300.0], [3.0, 33.0]])
    freqs = NP.linspace(100e6, 200e6, 37)
    kind, dia, ext, _ = setups(1)[name]
    ext = ext[0] if isinstance(ext, list) else ext
    ctx.set_array(NP.zeros((1, 3)), freqs, nt_max=1)
    for i in range(altaz.shape[0]):
        u = GEOM.altaz2dircos(altaz[i:i + 1], 'degrees')
        s = GEOM.frame_dircos(u, NP.eye(3), NP.zeros(3))     # what the entry's own normalisation makes of it, to the bit
        table = NP.linspace(-2.0, 3.0, 37).reshape(1, 37) + 0.1 * i
        fr, sp = NP.array([1.7 + i]), NP.array([-0.8])
        ctx.set_sky_analytic(s, NP.ones(1), NP.zeros(1), 1.0, kind, dia, ZEN, ZEN, ext=ext)
        pb = ctx.get_pbflux()
        ctx.set_sky_analytic(s, None, None, None, kind, dia, ZEN, ZEN, flux_spectrum=table, ext=ext)
        pb_table = ctx.get_pbflux()
        ctx.set_sky_analytic(s, fr, sp, 150e6, kind, dia, ZEN, ZEN, ext=ext)
        pb_law = ctx.get_pbflux()
        _, num, den, _ = ctx.antenna_power(u, freqs, NP.eye(3), kind, dia, flux_spectrum=table, ext=ext)
        assert NP.array_equal(den, pb) and NP.array_equal(num, pb_table)
        _, num, den, _ = ctx.antenna_power(u, freqs, NP.eye(3), kind, dia, flux_ref=fr, spindex=sp, ref_freq_hz=150e6, ext=ext)
        assert NP.array_equal(den, pb)
        assert NP.all(NP.abs(num - pb_law) <= 4 * U * NP.abs(pb_law))


# ---- 4. empty sky ---------------------------------------------------------------------------------------------------------------------

def test_empty_sky_is_nan(ctx):
    rng = NP.random.default_rng(4)
    radec = NP.stack((rng.uniform(-10.0, 10.0, 200), LAT + rng.uniform(-10.0, 10.0, 200)), axis=1)
    lst = NP.array([0.0, 180.0])
    freqs = NP.linspace(100e6, 200e6, 37)
    dircos = AK.sky_dircos(radec, 'radec', lst, LAT)
    assert NP.min(dircos[0][:, 2]) >= 0.97 and NP.max(dircos[1][:, 2]) <= -0.31
    flux_ref, spindex = rng.uniform(0.5, 5.0, 200), rng.uniform(-1.2, -0.2, 200)
    table = flux_ref[:, None] * (freqs[None, :] / 150e6) ** spindex[:, None]
    ref = AK.antenna_power(dircos, table, lambda t, dc: AK.beam_of({'element': 'dish', 'size': 14.0}, freqs)(dc))
    assert NP.min(ref['den'][0]) >= 1.0
    power, num, den, st = ctx.antenna_power(GEOM.catalog_unitvec(radec, 'radec'), freqs, rotations(lst), _abi.PRISIM_BEAM_AIRY, 14.0,
                                            flux_ref=flux_ref, spindex=spindex, ref_freq_hz=150e6)
    num_tol, den_tol, power_tol = AK.tolerances(ref)
    assert NP.all(NP.isfinite(power[0])) and NP.all(NP.abs(power[0] - ref['power'][0]) <= power_tol[0])
    assert NP.all(NP.abs(num[0] - ref['num'][0]) <= num_tol[0]) and NP.all(NP.abs(den[0] - ref['den'][0]) <= den_tol[0])
    assert NP.all(NP.isnan(power[1])) and NP.all(num[1] == 0.0) and NP.all(den[1] == 0.0)
    assert st['sources_up'] == 200 and st['sources_evaluated'] == 400


# ---- 5. same bits however it is streamed ----------------------------------------------------------------------------------------------

def test_same_bits_however_it_is_streamed(ctx, case1):
    power, num, den, st = case1.call(ctx, 'airy')
    # two streams, each: spans of 512 sources (dirs 32 B, pb_tile 8 B x 37 channels) and the partial sums of 7 blocks; 16 B of unit flux
    budget = 2 * (512 * (32 + 8 * 37) + 7 * 2 * 37 * 8) + 512 * 16
    p2, n2, d2, st2 = case1.call(ctx, 'airy', budget_bytes=budget)
    assert st2['spans'] == 4 and st2['span_sources'] == 512 and 1537 % 512 != 0 and st['spans'] == 1
    assert NP.array_equal(p2, power) and NP.array_equal(n2, num) and NP.array_equal(d2, den)
    p3, n3, d3, st3 = case1.call(ctx, 'airy', budget_bytes=256 * (32 + 8 * 37) + 7 * 2 * 37 * 8 + 256 * 16)      # one block, one stream
    assert st3['spans'] == 7 and st3['streams'] == 1
    assert NP.array_equal(p3, power) and NP.array_equal(n3, num) and NP.array_equal(d3, den)
    # one shared ext against five copies of it
    kind, dia, ext, _ = case1.setups['mwa_tile']
    flux = {'flux_ref': case1.flux_ref, 'spindex': case1.spindex, 'ref_freq_hz': case1.ref_freq}
    one = ctx.antenna_power(case1.unitvec, case1.freqs, case1.rot, kind, dia, ext=ext, **flux)
    five = ctx.antenna_power(case1.unitvec, case1.freqs, case1.rot, kind, dia, ext=[ext] * 5, **flux)
    assert all(NP.array_equal(a, b) for a, b in zip(one[:3], five[:3]))
    # without the sums
    p4, n4, d4, st4 = ctx.antenna_power(case1.unitvec, case1.freqs, case1.rot, _abi.PRISIM_BEAM_AIRY, 14.0, want_sums=False, **flux)
    assert n4 is None and d4 is None and NP.array_equal(p4, power) and st4['download_bytes'] == 5 * 37 * 8 + 5 * 8


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------

def test_refusals_write_nothing(ctx, case1):
    lib = _abi.load_library()
    import ctypes as C
    nsrc, nchan, nsnap = 300, 5, 2
    uv = NP.ascontiguousarray(case1.unitvec[:nsrc])
    fr, sp = NP.ascontiguousarray(case1.flux_ref[:nsrc]), NP.ascontiguousarray(case1.spindex[:nsrc])
    fq = NP.linspace(100e6, 200e6, nchan)
    rot = NP.ascontiguousarray(case1.rot[:nsnap].reshape(nsnap, 9))
    good_ext = _abi.make_beam_ext({'dipole_dircos': [1.0, 0.0, 0.0]})
    sentinel = -12345.0
    outs = [NP.full((nsnap, nchan), sentinel) for _ in range(3)]

    def args(**kw):
        a = ctx.PrisimAntpowerArgs()
        a.nsrc, a.nchan, a.nsnap = nsrc, nchan, nsnap
        a.unitvec, a.flux_ref, a.spindex, a.freqs_hz, a.cel2enu = (_abi._ptr(x) for x in (uv, fr, sp, fq, rot))
        a.ref_freq_hz = 150e6
        a.beam_kind, a.diameter_m = _abi.PRISIM_BEAM_AIRY, 14.0
        a.beam_pc_dircos[:] = [0.0, 0.0, 1.0]
        keep = []
        for k, v in kw.items():
            if isinstance(v, NP.ndarray):
                keep.append(v)
                v = _abi._ptr(v)
            setattr(a, k, v)
        a._keep = keep
        return a

    def call(a, power=True):
        rc = lib.prisim_antenna_power(ctx._h, None if a is None else C.byref(a), _abi._ptr(outs[0]) if power else None, _abi._ptr(outs[1]),
                                      _abi._ptr(outs[2]), None)
        return rc, lib.prisim_hip_last_error(ctx._h).decode()

    def bad(vec, i, v):
        out = NP.array(vec, dtype=NP.float64, copy=True)
        out.flat[i] = v
        return out

    long7 = uv.copy()
    long7[7] *= 1.00001
    skew = rot.copy()
    skew[1, 0] += 1e-8
    bad_ext = _abi.make_beam_ext({'dipole_dircos': [1.0, 0.0, 0.0]})
    bad_ext.dipole_mode = 17
    bf_ext = _abi.make_beam_ext({'dipole_dircos': [1.0, 0.0, 0.0], 'beamformer': {'positions': NP.zeros((2, 3))}})
    bf_ext.bf_nrand = 0
    cases = [
        (None, 'argument struct is NULL'), (args(unitvec=None), 'unitvec is NULL'), (args(freqs_hz=None), 'freqs_hz is NULL'),
        (args(cel2enu=None), 'cel2enu is NULL'), (args(nsrc=0), '>= 1'), (args(nchan=0), '>= 1'), (args(nsnap=0), '>= 1'),
        (args(nchan=(1 << 20) + 1), 'nchan must be at most 2^20'), (args(nsrc=1 << 45, nchan=4), 'nsrc * nchan'),
        (args(flux_ref=None), 'neither a power law'), (args(spindex=None), 'neither a power law'), (args(ref_freq_hz=0.0), 'ref_freq_hz'),
        (args(freqs_hz=bad(fq, 2, 0.0)), 'freqs_hz[2]'), (args(freqs_hz=bad(fq, 4, NP.inf)), 'freqs_hz[4]'),
        (args(freqs_hz=bad(fq, 1, NP.nan)), 'freqs_hz[1]'), (args(unitvec=long7), 'unitvec[7]'),
        (args(cel2enu=skew), 'cel2enu of snapshot 1'), (args(aberr_beta=NP.array([[0.0, 0.0, 0.0], [0.01, 0.0, 0.0]])), 'aberr_beta of snapshot 1'),
        (args(n_ext=3, ext=C.cast(C.pointer(good_ext), C.c_void_p)), 'n_ext must be 0, 1 or nsnap'), (args(n_ext=1), 'ext is NULL'),
        (args(beam_kind=9), 'unknown beam_kind'), (args(diameter_m=0.0), 'diameter_m must be positive'),
        (args(beam_kind=_abi.PRISIM_BEAM_DIPOLE), 'PRISIM_BEAM_DIPOLE needs'),
        (args(n_ext=1, ext=C.cast(C.pointer(bad_ext), C.c_void_p)), 'unknown dipole_mode'),
        (args(n_ext=1, ext=C.cast(C.pointer(bf_ext), C.c_void_p)), 'bf_nrand'),
        (args(budget_bytes=1000), 'cannot hold one block'),
    ]
    for a, text in cases:
        rc, msg = call(a)
        assert rc == _abi.PRISIM_EINVAL and text in msg, (text, rc, msg)
        assert all(NP.all(o == sentinel) for o in outs), text
    rc, msg = call(args(), power=False)
    assert rc == _abi.PRISIM_EINVAL and 'out_power is NULL' in msg and all(NP.all(o == sentinel) for o in outs)
    # the validity messages of the polynomial beams: coefficients that push the value past 1.01, and a NaN
    for coef, text in (([5.0, 0.0, 0.0, 0.0], 'exceeds unity'), ([NP.nan, 0.0, 0.0, 0.0], 'found to be NaN')):
        x = _abi.make_beam_ext({'poly': coef})
        rc, msg = call(args(beam_kind=_abi.PRISIM_BEAM_POLY, n_ext=1, ext=C.cast(C.pointer(x), C.c_void_p)))
        assert rc == _abi.PRISIM_EINVAL and text in msg and all(NP.all(o == sentinel) for o in outs), (text, msg)
    rc, msg = call(args())
    assert rc == _abi.PRISIM_OK, msg
    want = ctx.antenna_power(uv, fq, rot, _abi.PRISIM_BEAM_AIRY, 14.0, flux_ref=fr, spindex=sp, ref_freq_hz=150e6)
    assert all(NP.array_equal(o, w) for o, w in zip(outs, want[:3])) and NP.all(NP.isfinite(outs[0]))


# ---- 7. the Python function ---------------------------------------------------------------------------------------------------------

class Sky7(object):
    lst = NP.array([20.0, 95.0, 170.0, 245.0])

    def __init__(self):
        rng = NP.random.default_rng(7)
        self.nsrc = 3001
        self.radec = sphere(rng, self.nsrc)
        self.freqs = NP.linspace(110e6, 190e6, 21)
        self.flux_ref = rng.uniform(0.5, 5.0, self.nsrc)
        self.spindex = rng.uniform(-1.2, -0.2, self.nsrc)
        self.table = self.flux_ref[:, None] * (self.freqs[None, :] / 150e6) ** self.spindex[:, None]
        self.func_mhz = SM.SkyModel(location=self.radec, flux_ref=self.flux_ref, spindex=self.spindex, ref_freq=150.0)
        self.spectrum = SM.SkyModel(location=self.radec, frequency=self.freqs, spectrum=self.table)
        self.pinfo = {'lst': self.lst}


@pytest.fixture(scope='module')
def sky7():
    return Sky7()


def check_python(got, dircos, table, beam, n_lst, nchan, den_floor=1.0):
    ref = AK.antenna_power(dircos, table, beam)
    preconditions(dircos, ref, den_floor)
    assert got.shape == (n_lst, nchan) and got.dtype == NP.float64
    _, _, power_tol = AK.tolerances(ref)
    assert NP.all(NP.abs(got - ref['power']) <= power_tol), float(NP.max(NP.abs(got - ref['power']) / power_tol))


def test_python_hera_on_a_spectrum_model(sky7):
    tel = {'id': 'hera', 'latitude': LAT}
    st = {}
    got = RI.antenna_power(sky7.spectrum, tel, sky7.pinfo, stats=st)
    dircos = AK.sky_dircos(sky7.radec, 'radec', sky7.lst, LAT)
    check_python(got, dircos, sky7.table, lambda t, dc: BO.primary_beam_generator(GEOM.dircos2altaz(dc), sky7.freqs, tel), 4, 21)
    assert st['sources_evaluated'] == 4 * sky7.nsrc and st['spans'] == 1


def test_python_dish_on_a_power_law_in_mhz(sky7):
    tel = {'shape': 'dish', 'size': 14.0, 'latitude': LAT}
    got = RI.antenna_power(sky7.func_mhz, tel, sky7.pinfo, freq_scale='MHz', frequency=sky7.freqs / 1e6)
    dircos = AK.sky_dircos(sky7.radec, 'radec', sky7.lst, LAT)
    check_python(got, dircos, sky7.table, lambda t, dc: BO.primary_beam_generator(GEOM.dircos2altaz(dc), sky7.freqs, tel), 4, 21)


def test_python_mwa_tracking_a_radec_pointing(sky7):
    tel = {'id': 'mwa', 'latitude': LAT}
    pc = NP.array([[95.0, LAT + 5.0]])                          # (RA, Dec): the tile follows it, other delays at every LST
    pinfo = {'lst': sky7.lst[:3], 'pointing_center': pc, 'pointing_coords': 'radec'}
    st = {}
    got = RI.antenna_power(sky7.spectrum, tel, pinfo, stats=st)
    altaz = AK.hadec2altaz(NP.stack((sky7.lst[:3] - 95.0, NP.full(3, LAT + 5.0)), axis=1), LAT)
    assert NP.all(altaz[:, 0] > 0.0)
    pos = PB.mwa_tile_element_locs()
    bfs = []
    for t in range(3):
        delays, gains = BO.beamformer_settings(pos, {'pointing_center': AK.altaz2dircos(altaz[t:t + 1]).ravel()})
        bfs.append({'positions': pos, 'delays': delays, 'gains': gains})
    assert not NP.array_equal(bfs[0]['delays'], bfs[1]['delays'])
    setup = {'element': 'dipole', 'size': 0.74, 'element_dircos': NP.array([1.0, 0.0, 0.0]), 'beamformers': bfs}
    dircos = AK.sky_dircos(sky7.radec, 'radec', sky7.lst[:3], LAT)
    check_python(got, dircos, sky7.table, lambda t, dc: AK.beam_of(setup, sky7.freqs, t)(dc), 3, 21)


@pytest.mark.parametrize('coords', ['hadec', 'altaz'])
def test_python_other_sky_frames(sky7, coords):
    tel = {'id': 'hera', 'latitude': LAT}
    if coords == 'hadec':
        loc = sky7.radec                                            # read as (HA, Dec): the same sky at every LST
    else:
        loc = GEOM.dircos2altaz(AK.sky_dircos(sky7.radec, 'radec', [33.0], LAT)[0])
    model = SM.SkyModel(location=loc, frequency=sky7.freqs, spectrum=sky7.table)
    got = RI.antenna_power(model, tel, {'lst': sky7.lst[:2]}, coords=coords)
    dircos = AK.sky_dircos(loc, coords, sky7.lst[:2], LAT)
    check_python(got, dircos, sky7.table, lambda t, dc: BO.primary_beam_generator(GEOM.dircos2altaz(dc), sky7.freqs, tel), 2, 21)
    assert NP.array_equal(got[0], got[1])


def test_python_true_place_through_frames(sky7):
    tel = {'id': 'hera', 'latitude': LAT}
    jd0 = 2461333.5                                                 # 2026 October 19
    frames = [FRAMES.snapshot_frame('radec', l, LAT, jd=jd0 + 0.01 * i, epoch='J2000', model='apparent') for i, l in enumerate(sky7.lst)]
    got = RI.antenna_power(sky7.spectrum, tel, sky7.pinfo, frames=frames)
    dircos = AK.frame_dircos(GEOM.catalog_unitvec(sky7.radec, 'radec'), NP.stack([f[0] for f in frames]), NP.stack([f[1] for f in frames]))
    plain = AK.sky_dircos(sky7.radec, 'radec', sky7.lst, LAT)
    assert NP.max(NP.abs(dircos - plain)) > 1e-3                    # a quarter of a century of precession: not the default's place
    check_python(got, dircos, sky7.table, lambda t, dc: BO.primary_beam_generator(GEOM.dircos2altaz(dc), sky7.freqs, tel), 4, 21)
