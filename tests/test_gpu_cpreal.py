"""GPU: closure phases of noise realisations, drawn and closed on the device (include/prisim_cpreal.h), through the C-ABI against the
numpy checker (tests/cpreal_checker.py) on the noise cubes of Context.noise, the bit equalities between the routes, chunkings and
row subsets, and InterferometerArray.closure_phase_realizations against the chain it replaces (generate_noise, add_noise,
getClosurePhase).

Bound.  Phases are compared as |exp(i a) - exp(i b)| <= 32 u, u = 2^-53: the bound derived at the head of tests/test_gpu_closure.py
(two complex products and an atan2 per side).  The extra sum cube + n is one IEEE addition, identical on both sides.  Points whose
bispectrum is exactly zero are left out of the comparison and must be finite.  Against the chain the comparison is array_equal: both
sides run the same device statements."""
import os
import sys
import warnings

import numpy as NP
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cpreal_checker as RK  # noqa: E402

from prisim_amd import _abi, layouts as LAY, skymodel as SM, workloads as W  # noqa: E402
from prisim_amd import bispectrum_phase as BP  # noqa: E402
from prisim_amd import interferometry as RI  # noqa: E402

pytestmark = pytest.mark.gpu
PHASE_BOUND = 32 * 2.0 ** -53
SEED, NREAL = 0xFFFFFFFFFFFFFFFE, 5            # the keys of realisations 2.. wrap past 2^64


class Case(object):
    """12 baselines of which 9 are used, 37 channels (no multiple of a tile), 3 snapshots; 7 triads that share rows, with mixed
    conjugation; a global baseline map that is not the identity and holds one index >= 2^32 (the counter's high word); positive
    bpwts except one (row, channel), zero in every snapshot."""
    nbl, nchan, nt = 12, 37, 3
    used = NP.array([0, 1, 3, 4, 6, 7, 8, 10, 11])
    legs = NP.array([[0, 1, 2], [2, 3, 4], [4, 5, 6], [6, 7, 8], [8, 0, 4], [1, 3, 5], [7, 2, 0]], dtype=NP.int32)     # rows of `used`
    conj = NP.array([[0, 0, 1], [1, 0, 0], [0, 1, 0], [1, 1, 0], [0, 0, 0], [1, 1, 1], [0, 1, 1]], dtype=NP.int32)
    zero_row, zero_chan = 4, 20                # of `used`

    def __init__(self):
        rng = NP.random.default_rng(20250101)
        self.glob = NP.array([5, 3, 40, 41, 7, (1 << 32) + 9, 100, 2, 77, 1000, 12, 6], dtype=NP.int64)
        self.baselines = rng.uniform(-100.0, 100.0, (self.nbl, 3))
        self.channels = 150e6 + 1e5 * NP.arange(self.nchan)
        self.cube = rng.standard_normal((self.nt, self.nbl, self.nchan)) + 1j * rng.standard_normal((self.nt, self.nbl, self.nchan))
        self.rms = rng.uniform(0.5, 2.0, (self.nt, self.nbl, self.nchan))
        self.bpwts = rng.uniform(0.5, 1.5, (self.nt, self.nbl, self.nchan))
        self.bpwts[:, self.used[self.zero_row], self.zero_chan] = 0.0

    def resident(self, ctx):
        ctx.set_array(self.baselines, self.channels, nt_max=self.nt)
        for t in range(self.nt):
            ctx.set_vis(NP.ascontiguousarray(self.cube[t]), slot=t)

    def noise(self, ctx, nreal=NREAL, first=0):
        """(nreal, nt, 9, nchan): Context.noise over all twelve baselines under the key of every realisation, the used rows of it"""
        return NP.stack([ctx.noise(self.rms, (SEED + first + r) % (1 << 64), bl_index=self.glob)[:, self.used] for r in range(nreal)])

    def call(self, ctx, resident=False, rows=None, legs=None, conj=None, **kw):
        rows = self.used if rows is None else rows
        cube, cube_row = (None, rows) if resident else (self.cube[:, rows], None)
        return ctx.closure_realizations(cube, cube_row, self.glob[rows], self.rms[:, rows], self.bpwts[:, rows],
                                        self.legs if legs is None else legs, self.conj if conj is None else conj, SEED,
                                        kw.pop('n_realize', NREAL), nt=self.nt, **kw)


@pytest.fixture(scope='module')
def case(ctx):
    c = Case()
    c.resident(ctx)
    c.noise_cubes = c.noise(ctx)
    c.want = {kind: RK.closure_realizations(c.cube[:, c.used], c.noise_cubes, c.bpwts[:, c.used], c.legs, c.conj, kind=kind)
              for kind in ('noisy', 'noise')}
    c.full = {kind: c.call(ctx, kind=kind)[0] for kind in ('noisy', 'noise')}
    return c


def _check(ph, want, bispectrum, zero_expected, what):
    zero = bispectrum == 0
    assert NP.array_equal(zero, zero_expected), what                # the zeroed bpwts entry and nothing more
    assert NP.all(NP.isfinite(ph)), what
    dev = float(RK.phase_deviation(ph, want)[~zero].max())
    print(what, 'largest phase deviation %.3e (bound %.3e)' % (dev, PHASE_BOUND))
    assert dev <= PHASE_BOUND, (what, dev)


@pytest.mark.parametrize('kind', ['noisy', 'noise'])
@pytest.mark.parametrize('resident', [False, True], ids=['host', 'resident'])
def test_entry_against_the_checker(ctx, case, kind, resident):
    want_ph, want_b = case.want[kind]
    assert want_ph.shape == (case.nt, NREAL, len(case.legs), case.nchan)
    # the share of exact zeros the zeroed bpwts entry implies: the triads that use that row, at that channel
    uses = NP.any(case.legs == case.zero_row, axis=1)
    zero_expected = NP.zeros(want_ph.shape, dtype=bool)
    zero_expected[:, :, uses, case.zero_chan] = True
    assert 0 < uses.sum() < len(case.legs) and zero_expected.sum() == case.nt * NREAL * uses.sum()
    ph, st = case.call(ctx, resident=resident, kind=kind)
    assert ph.shape == want_ph.shape and ph.dtype == NP.float64
    assert st['resident'] == resident and st['pairs'] == case.nt * NREAL and st['chunks'] == 1 and st['download_bytes'] == ph.nbytes
    _check(ph, want_ph, want_b, zero_expected, '%s %s' % (kind, 'resident' if resident else 'host'))
    assert NP.array_equal(ph, case.full[kind])


def test_routes_chunks_offsets_and_row_subsets_give_the_same_bits(ctx, case):
    ntriads, nchan, nt = len(case.legs), case.nchan, case.nt
    for kind in ('noisy', 'noise'):
        full = case.full[kind]
        outs = {}
        for route in ('staged', 'direct'):
            outs[route], st = case.call(ctx, kind=kind, route=route)
            assert st['route'] == route
            assert st['draws'] == nt * NREAL * nchan * (len(case.used) if route == 'staged' else 3 * ntriads)
        assert NP.array_equal(outs['staged'], outs['direct']) and NP.array_equal(outs['staged'], full)
        # 15 pairs in chunks of 4, 4, 4 and 3 on two streams, both routes
        for route in ('staged', 'direct'):
            ph, st = case.call(ctx, kind=kind, route=route, budget_bytes=2 * 4 * ntriads * nchan * 8 + 100)
            assert st['chunks'] == 4 and st['chunk_pairs'] == 4 and st['streams'] == 2 and st['chunks'] >= 3
            assert NP.array_equal(ph, full), (kind, route)
        # realisations 2..4 alone
        ph, _ = case.call(ctx, kind=kind, first=2, n_realize=3)
        assert ph.shape == (nt, 3, ntriads, nchan) and NP.array_equal(ph, full[:, 2:5])
        # a subset of the rows with their global indices: the triads that use only those rows
        rows_sub = NP.array([0, 2, 3, 4, 6, 7, 8])                       # of `used`
        remap = -NP.ones(len(case.used), dtype=NP.int64)
        remap[rows_sub] = NP.arange(rows_sub.size)
        keep = NP.all(NP.isin(case.legs, rows_sub), axis=1)
        assert keep.sum() >= 2
        for cube_resident in (False, True):
            ph, _ = case.call(ctx, resident=cube_resident, kind=kind, rows=case.used[rows_sub], legs=remap[case.legs[keep]].astype(NP.int32),
                              conj=case.conj[keep])
            assert NP.array_equal(ph, full[:, :, keep]), (kind, cube_resident)


def test_auto_route_follows_the_lds(ctx, case):
    _, st = case.call(ctx)
    assert st['route'] == 'staged' and st['chan_tile'] == 32 and st['lds_bytes'] == 9 * 16 * 32      # cpreal_plan.h: tests/test_cpreal.py
    # 12 000 used rows of 4 channels: 16 B x 8 channels x 12 000 rows is past every LDS, so AUTO goes direct
    rng = NP.random.default_rng(12000)
    nrow, nchan, ntriads = 12000, 4, 300
    ctx.set_array(rng.uniform(-100.0, 100.0, (nrow, 3)), 150e6 + 1e5 * NP.arange(nchan), nt_max=1)
    cube = rng.standard_normal((1, nrow, nchan)) + 1j * rng.standard_normal((1, nrow, nchan))
    rms = rng.uniform(0.5, 2.0, (1, nrow, nchan))
    bpwts = rng.uniform(0.5, 1.5, (1, nrow, nchan))
    legs = rng.integers(0, nrow, (ntriads, 3)).astype(NP.int32)
    legs[0] = (0, nrow - 1, nrow // 2)
    conj = rng.integers(0, 2, (ntriads, 3)).astype(NP.int32)
    glob = NP.arange(nrow, dtype=NP.int64)[::-1].copy()
    try:
        ph, st = ctx.closure_realizations(cube, None, glob, rms, bpwts, legs, conj, 7, 1)
        assert st['route'] == 'direct' and st['chan_tile'] == 0 and st['lds_bytes'] == 0 and st['draws'] == 3 * ntriads * nchan
        noise = ctx.noise(rms, 7, bl_index=glob)[NP.newaxis]
        want_ph, want_b = RK.closure_realizations(cube, noise, bpwts, legs, conj)
        _check(ph, want_ph, want_b, NP.zeros(want_ph.shape, dtype=bool), '12 000 rows, direct')
        with pytest.raises(ValueError, match='do not fit'):
            ctx.closure_realizations(cube, None, glob, rms, bpwts, legs, conj, 7, 1, route='staged')
    finally:
        case.resident(ctx)                                             # the module's array again


def test_entry_refusals_leave_the_context_usable(ctx, case):
    lib, h = ctx._lib, ctx._h
    u = case.used
    cube = NP.ascontiguousarray(case.cube[:, u])
    rms, bpw = NP.ascontiguousarray(case.rms[:, u]), NP.ascontiguousarray(case.bpwts[:, u])
    glob, crow = NP.ascontiguousarray(case.glob[u]), NP.ascontiguousarray(u, dtype=NP.int32)
    out = NP.empty((case.nt, 2, len(case.legs), case.nchan))
    p = _abi._ptr

    def entry(**kw):
        a = dict(cube=cube, cube_row=None, glob=glob, nt=case.nt, nrow=len(u), nchan=case.nchan, rms=rms, bpw=bpw, legs=case.legs, conj=case.conj,
                 ntriads=len(case.legs), n_realize=2, kind=0, route=-1, out=out)
        a.update(kw)
        rc = lib.prisim_closure_realizations(h, p(a['cube']), p(a['cube_row']), p(a['glob']), a['nt'], a['nrow'], a['nchan'], p(a['rms']),
                                             p(a['bpw']), p(a['legs']), p(a['conj']), a['ntriads'], 5, 0, a['n_realize'], a['kind'],
                                             a['route'], 0, p(a['out']), None)
        return rc, lib.prisim_hip_last_error(h).decode()

    bad_leg = case.legs.copy()
    bad_leg[3, 1] = 9
    neg_leg = case.legs.copy()
    neg_leg[0, 0] = -1
    bad_glob = glob.copy()
    bad_glob[2] = -1
    bad_rms = rms.copy()
    bad_rms[1, 2, 3] = NP.nan
    bad_crow = crow.copy()
    bad_crow[4] = case.nbl
    refusals = [({'glob': None}, 'null'), ({'rms': None}, 'null'), ({'bpw': None}, 'null'), ({'legs': None}, 'null'), ({'conj': None}, 'null'),
                ({'out': None}, 'null'), ({'cube': None, 'cube_row': None}, 'cube_row'),
                ({'nt': 0}, '>= 1'), ({'nrow': 0}, '>= 1'), ({'nchan': -1}, '>= 1'), ({'ntriads': 0}, '>= 1'), ({'n_realize': 0}, '>= 1'),
                ({'legs': bad_leg}, 'leg 1 of triad 3 is row 9 of 9 used rows'), ({'legs': neg_leg}, 'leg 0 of triad 0 is row -1'),
                ({'glob': bad_glob}, 'negative global baseline'), ({'rms': bad_rms}, 'finite and non-negative'),
                ({'kind': 2}, 'unknown kind'), ({'kind': -1}, 'unknown kind'), ({'route': 2}, 'unknown route'), ({'route': -2}, 'unknown route'),
                ({'cube': None, 'cube_row': crow, 'nt': case.nt + 1}, 'resident cube has 3 slots'),
                ({'cube': None, 'cube_row': bad_crow}, 'cube_row 4 is row 12 of a resident cube of 12 baselines')]
    for kw, msg in refusals:
        rc, err = entry(**kw)
        assert rc == _abi.PRISIM_EINVAL and msg in err, (kw.keys(), rc, err)
    rc, err = entry()
    assert rc == _abi.PRISIM_OK, err
    ph, _ = case.call(ctx)
    assert NP.array_equal(ph, case.full['noisy'])                   # and the context computes what it computed before


# ---- the class against the chain it replaces ------------------------------------------------------------------------------------

def _hera19_array(nt):
    cfg = W.config2()
    pos = LAY.array_layout('HERA-19')
    bl, ids = LAY.fold_and_sort_baselines(*LAY.baseline_generator(pos))
    labels = [(str(int(a)), str(int(b))) for a, b in ids]
    ch = cfg['channels'][:32]
    sky = cfg['sky']
    shape = None if sky.get('fwhm_deg') is None else NP.stack((sky['fwhm_deg'], sky['fwhm_deg'], NP.zeros_like(sky['fwhm_deg'])), axis=1)
    skymod = SM.SkyModel(location=sky['altaz'], flux_ref=sky['flux_ref'], spindex=sky['spindex'], ref_freq=sky['ref_freq'], src_shape=shape)
    layout = {'positions': pos, 'labels': NP.array([str(i) for i in range(len(pos))]), 'ids': NP.arange(len(pos)), 'coords': 'ENU'}
    ia = RI.InterferometerArray(labels, bl, ch, telescope={'id': 'hera', 'shape': 'delta', 'size': 14.0, 'ocoords': 'altaz',
                                                           'orientation': NP.array([[90.0, 270.0]]), 'groundplane': None},
                                latitude=-30.7224, skycoords='altaz', pointing_coords='altaz', layout=layout)
    ia.reserve(nt)
    bpass = 0.6 + 0.4 * NP.hanning(ch.size + 2)[1:-1]
    for j in range(nt):
        ia.observe((2457000.5 + j / 64.0, 30.0 + 0.25 * j), {'Tnet': 200.0 + 10.0 * j}, bpass, [90.0, 270.0], skymod, 10.7)
    return ia


def test_class_equals_the_chain_it_replaces():
    """HERA-19 (171 baselines), 32 channels, 2 snapshots, 3 realisations, all 14.6 m equilateral triads: bit for bit the phases of
    generate_noise(seed + r); add_noise(); getClosurePhase(triplets), for the noisy visibilities and for the noise alone."""
    nt, nreal, seed = 2, 3, 41
    ia = _hera19_array(nt)
    assert ia.baselines.shape[0] == 171 and ia.channels.size == 32
    equilateral = 14.6 * NP.array([[1.0, 0.0, 0.0], [-0.5, NP.sqrt(0.75), 0.0], [-0.5, -NP.sqrt(0.75), 0.0]])
    triads, _ = BP.triads_of_bltriplet(ia, equilateral)
    triplets = [tuple(t) for t in triads.tolist()]
    assert len(triplets) == 144
    res = ia.closure_phase_realizations(nreal, seed, antenna_triplets=triplets, datakey=['noisy', 'noise'])
    assert ia.vis_freq is None and ia.vis_noise_freq is None
    st = ia.cpreal_stats
    assert set(st) == {'noisy', 'noise'} and all(v['resident'] and v['route'] == 'staged' and v['pairs'] == nt * nreal for v in st.values())
    assert res['seeds'].tolist() == [41, 42, 43]
    for key in ('closure_phase_vis', 'closure_phase_noise'):
        assert res[key].shape == (nt, nreal, 144, 32)
    direct = ia.closure_phase_realizations(nreal, seed, antenna_triplets=triplets, datakey=['noisy', 'noise'], route='direct')
    for r in range(nreal):
        ia.generate_noise(seed=seed + r)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            ia.add_noise()
        chain = ia.getClosurePhase(antenna_triplets=triplets)
        for key in ('closure_phase_vis', 'closure_phase_noise'):
            want = NP.transpose(chain[key], (2, 0, 1))
            assert NP.array_equal(res[key][:, r], want), (key, r)
            assert NP.array_equal(direct[key][:, r], want), (key, r)
