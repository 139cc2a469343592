"""GPU: visibility triplets and closure phases of antenna triads (include/prisim_closure.h), through the C-ABI and through
InterferometerArray.getClosurePhase, against tests/golden/golden_closure.npz (the reference's statements executed) and the numpy
checker (tests/closure_checker.py).

Bounds.  Triplets without a filter: equal value for value (two real products, each rounded once).  Phases: |exp(i a) - exp(i b)| <=
32 u, u = 2^-53 -- a complex product, fused or not, errs by at most sqrt(5) u |a||b| (Brent, Percival, Zimmermann 2007), so two
products on each side move B by at most 4 sqrt(5) u ~ 9 u of |B|, and an atan2 good to 2 ulp of a value up to pi adds 8 u per side:
25 u, rounded up to 32 u.  Points whose bispectrum is exactly zero (a flagged channel) are left out of the phase comparison and must be
finite.  Filtered triplets: 1e-12 of the row maximum (the bound of tests/test_gpu_subband.py for the same two FFT routes); their phases
are compared with numpy's angle of the product of the device's own triplets."""
import os
import sys
import warnings

import numpy as NP
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import closure_checker as CK  # noqa: E402

from prisim_amd import _abi, layouts as LAY, skymodel as SM, workloads as W  # noqa: E402
from prisim_amd import interferometry as RI  # noqa: E402

GOLD = NP.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'golden_closure.npz'))
pytestmark = pytest.mark.gpu
PHASE_BOUND = 32 * 2.0 ** -53
CUBES = (('skyvis', 'skyvis_freq', 'skyvis'), ('vis', 'vis_freq', 'vis'), ('noise', 'vis_noise_freq', 'noisevis'))


def _gold_legs():
    import types
    labels = [tuple(x) for x in GOLD['cp_labels'].tolist()]
    s = types.SimpleNamespace(labels=labels, baselines=GOLD['cp_baselines'], bl_reversemap=None)
    return RI.InterferometerArray.closure_leg_table(s, [tuple(t) for t in GOLD['cp_triplets'].tolist()])[:2]


def _check_phases(ph, ref_ph, bispectrum, what, expect_zero=None):
    zero = bispectrum == 0
    if expect_zero is None:
        assert not zero.any(), what
    else:
        assert NP.array_equal(zero, expect_zero), what
    assert NP.all(NP.isfinite(ph)), what
    dev = float(CK.phase_deviation(ph, ref_ph)[~zero].max())
    print(what, 'largest phase deviation %.3e (bound %.3e)' % (dev, PHASE_BOUND))
    assert dev <= PHASE_BOUND, (what, dev)
    return dev


def test_no_filter_branch_against_the_reference(ctx):
    legs, conj = _gold_legs()
    bpw = GOLD['cp_bp'] * GOLD['cp_bp_wts']
    nchan = GOLD['cp_channels'].size
    for name, cube, key in CUBES:
        x = GOLD['cp_' + cube]
        ref_t, ref_ph = GOLD['cp_out_' + key], GOLD['cp_out_closure_phase_' + name]
        flagged = NP.zeros(ref_ph.shape, dtype=bool)
        flagged[:, 7, :] = True
        assert flagged.mean() == 1.0 / nchan
        trip, ph, st = ctx.closure_phase(x, legs, conj, bpw)
        assert st['route'] == 'direct' and st['chunks'] == 1 and st['triads'] == len(legs)
        assert NP.array_equal(trip, ref_t), name
        _check_phases(ph, ref_ph, NP.prod(ref_t, axis=1), 'fixture ' + name, expect_zero=flagged)
        # the same cube resident on the device ([nt][nbl][nchan]): the other read path
        nbl, _, nt = x.shape
        ctx.set_array(GOLD['cp_baselines'], GOLD['cp_channels'], nt_max=nt)
        for t in range(nt):
            ctx.set_vis(NP.ascontiguousarray(x[:, :, t]), slot=t)
        trip2, ph2, _ = ctx.closure_phase(None, legs, conj, bpw, nt=nt)
        assert NP.array_equal(trip2, ref_t) and NP.array_equal(ph2, ph), name


def test_many_to_one_reversemap_against_the_reference(ctx):
    """HERA-19 with redundant folding: the leg table goes through a reversemap that maps 171 pairs onto 30 simulated baselines."""
    import types
    labels = [tuple(x) for x in GOLD['hera19red_labels'].tolist()]
    rev = {tuple(k): tuple(v) for k, v in zip(GOLD['hera19red_rev_keys'].tolist(), GOLD['hera19red_rev_vals'].tolist())}
    s = types.SimpleNamespace(labels=labels, baselines=GOLD['hera19red_bl'], bl_reversemap=rev)
    legs, conj, vec = RI.InterferometerArray.closure_leg_table(s, [tuple(t) for t in GOLD['redcp_triplets'].tolist()])
    assert NP.array_equal(NP.asarray(vec), GOLD['redcp_out_baseline_triplets'])
    for name, cube, key in CUBES:
        trip, ph, _ = ctx.closure_phase(GOLD['redcp_' + cube], legs, conj, GOLD['redcp_bp'] * GOLD['redcp_bp_wts'])
        assert NP.array_equal(trip, GOLD['redcp_out_' + key]), name
        _check_phases(ph, GOLD['redcp_out_closure_phase_' + name], NP.prod(GOLD['redcp_out_' + key], axis=1), 'folded ' + name)


@pytest.mark.parametrize('nchan', [2048, 4096])
def test_fused_filter_on_the_longest_rows(ctx, nchan):
    """One snapshot per workgroup; nchan = 4096 takes 96 KiB of dynamic LDS, above the 64 KiB a kernel gets without asking."""
    rng = NP.random.default_rng(nchan)
    nbl, nt, ntriads, df = 4, 3, 5, 1e5
    x, bp, wts, legs, conj = _random_case(rng, nbl, nchan, nt, ntriads)
    lengths = rng.uniform(10.0, 900.0, nbl)
    tau = NP.fft.fftfreq(nchan, df)
    dwidth = 3.0 * (tau[1] - tau[0])
    want_t, _ = CK.closure_phase(x, legs, conj, bp, wts, delay_filter=('horizon', 'discard', 0.0, dwidth), baseline_lengths=lengths, df=df)
    masks, idx = RI.closure_filter_masks(tau, 'horizon', 'discard', 0.0, dwidth, lengths)
    for route in ('auto', 'rocfft'):
        trip, ph, st = ctx.closure_phase(x, legs, conj, bp * wts, masks=masks, mask_index=idx, route=route)
        assert st['route'] == ('fused' if route == 'auto' else 'rocfft')
        if route == 'auto':
            assert st['tile'] == 1 and st['lds_bytes'] == 16 * (nchan + 1) + 8 * nchan and (nchan < 4096 or st['lds_bytes'] > 65536)
        err = float(NP.max(NP.abs(trip - want_t) / NP.max(NP.abs(want_t), axis=2, keepdims=True)))
        print(nchan, route, 'triplet error %.3e of the row maximum' % err)
        assert err <= 1e-12
        own = NP.prod(trip, axis=1)
        _check_phases(ph, NP.angle(own), own, 'filter %d %s' % (nchan, route))


def _random_case(rng, nbl, nchan, nt, ntriads):
    x = rng.standard_normal((nbl, nchan, nt)) + 1j * rng.standard_normal((nbl, nchan, nt))
    bp = 1.0 + 0.2 * rng.standard_normal((nbl, nchan, nt))
    wts = rng.uniform(0.5, 1.5, (nbl, nchan, nt))
    legs = rng.integers(0, nbl, (ntriads, 3)).astype(NP.int32)
    conj = rng.integers(0, 2, (ntriads, 3)).astype(NP.int32)
    return x, bp, wts, legs, conj


def test_resident_tiled_path_and_streaming(ctx):
    """nt large enough for the LDS-tile kernel, sizes that are no multiples of the tile; a budget that forces several chunks with a
    partial last one gives the output of one chunk."""
    rng = NP.random.default_rng(5)
    nbl, nchan, nt, ntriads = 9, 70, 37, 23
    x, bp, wts, legs, conj = _random_case(rng, nbl, nchan, nt, ntriads)
    fw = rng.uniform(0.2, 1.0, nchan)
    want_t, want_ph = CK.closure_phase(x, legs, conj, bp, wts, freq_wts=fw)
    ctx.set_array(rng.standard_normal((nbl, 3)), 150e6 + 1e5 * NP.arange(nchan), nt_max=nt)
    for t in range(nt):
        ctx.set_vis(NP.ascontiguousarray(x[:, :, t]), slot=t)
    per_triad = nchan * nt * (3 * 16 + 8)
    outs = []
    for cube, kw in ((None, {'nt': nt}), (x, {})):
        for budget in (_abi.CLOSURE_BUDGET, 2 * 5 * per_triad):
            trip, ph, st = ctx.closure_phase(cube, legs, conj, bp * wts, freq_wts=fw, budget_bytes=budget, **kw)
            assert st['tile'] == (1 if cube is None else 0)
            if budget != _abi.CLOSURE_BUDGET:
                assert st['chunks'] == 5 and st['chunk_triads'] == 5 and st['streams'] == 2
            assert NP.array_equal(trip, want_t)
            _check_phases(ph, want_ph, NP.prod(want_t, axis=1), 'tiled' if cube is None else 'plain')
            outs.append((trip, ph))
    for trip, ph in outs[1:]:
        assert NP.array_equal(trip, outs[0][0]) and NP.array_equal(ph, outs[0][1])


@pytest.mark.parametrize('nchan', [64, 48])
@pytest.mark.parametrize('ftype', ['regular', 'horizon'])
@pytest.mark.parametrize('fmode', ['discard', 'retain'])
@pytest.mark.parametrize('window', [False, True])
def test_filter_branches_against_the_checker(ctx, nchan, ftype, fmode, window):
    rng = NP.random.default_rng(nchan + 7 * window)
    nbl, nt, ntriads, df = 7, 5, 11, 1e5
    x, bp, wts, legs, conj = _random_case(rng, nbl, nchan, nt, ntriads)
    lengths = rng.uniform(10.0, 900.0, nbl)
    tau = NP.fft.fftfreq(nchan, df)
    dtau = tau[1] - tau[0]
    dmin, dwidth = (2 * dtau, 5 * dtau) if ftype == 'regular' else (0.0, 1.0 * dtau)
    fw = (0.3 + NP.hanning(nchan + 2)[1:-1]) if window else None
    want_t, _ = CK.closure_phase(x, legs, conj, bp, wts, freq_wts=fw, delay_filter=(ftype, fmode, dmin, dwidth),
                                 baseline_lengths=lengths, df=df)
    masks, idx = RI.closure_filter_masks(tau, ftype, fmode, dmin, dwidth, lengths)
    routes = ('fused', 'rocfft') if nchan & (nchan - 1) == 0 else ('rocfft',)
    ctx.set_array(rng.standard_normal((nbl, 3)), 150e6 + df * NP.arange(nchan), nt_max=nt)
    for t in range(nt):
        ctx.set_vis(NP.ascontiguousarray(x[:, :, t]), slot=t)
    for route in routes + ('auto',):
        for cube, kw in ((x, {}), (None, {'nt': nt})):
            trip, ph, st = ctx.closure_phase(cube, legs, conj, bp * wts, freq_wts=fw, masks=masks, mask_index=idx, route=route,
                                             budget_bytes=2 * 4 * nchan * nt * (6 * 16 + 8), **kw)
            assert st['route'] == (route if route != 'auto' else routes[0]) and st['chunks'] == (3 if st['route'] == 'rocfft' else 2)
            rowmax = NP.max(NP.abs(want_t), axis=2, keepdims=True)
            err = float(NP.max(NP.abs(trip - want_t) / rowmax))
            print(nchan, ftype, fmode, window, route, 'triplet error %.3e of the row maximum' % err)
            assert err <= 1e-12
            own = NP.prod(trip, axis=1)
            _check_phases(ph, NP.angle(own), own, 'filter %s' % route)
    if nchan & (nchan - 1):
        with pytest.raises(ValueError, match='power-of-two'):
            ctx.closure_phase(x, legs, conj, bp * wts, masks=masks, mask_index=idx, route='fused')


@pytest.mark.parametrize('nchan,nt,route', [(1, 3, 'fused'), (2, 3, 'fused'), (8, 65, 'fused'), (12, 5, 'rocfft')])
def test_filter_on_the_shortest_rows_and_one_snapshot_past_the_tile(ctx, nchan, nt, route):
    """Rows of 1 and 2 channels (no bit to reverse, one butterfly), 65 snapshots of 8 channels (a full tile of 64 and one more), and 12
    channels through rocFFT; three chunks of 3, 3 and 1 triads on two streams."""
    rng = NP.random.default_rng(1000 + nchan)
    nbl, ntriads, df = 5, 7, 1e5
    x, bp, wts, legs, conj = _random_case(rng, nbl, nchan, nt, ntriads)
    tau, dtau = NP.fft.fftfreq(nchan, df), 1.0 / (nchan * df)
    fw = rng.uniform(0.3, 1.3, nchan)
    want_t, _ = CK.closure_phase(x, legs, conj, bp, wts, freq_wts=fw, delay_filter=('regular', 'discard', 2 * dtau, 5 * dtau), df=df)
    masks, idx = RI.closure_filter_masks(tau, 'regular', 'discard', 2 * dtau, 5 * dtau, None)
    per_triad = nchan * nt * (3 * 16 + 8 + (3 * 16 if route == 'rocfft' else 0))
    trip, ph, st = ctx.closure_phase(x, legs, conj, bp * wts, freq_wts=fw, masks=masks, mask_index=idx, route=route,
                                     budget_bytes=2 * 3 * per_triad)
    assert st['route'] == route and st['chunk_triads'] == 3 and st['chunks'] == 3 and st['streams'] == 2
    if route == 'fused':
        assert st['tile'] == min(nt, 64)
    err = float(NP.max(NP.abs(trip - want_t) / NP.max(NP.abs(want_t), axis=2, keepdims=True)))
    print(nchan, nt, route, 'triplet error %.3e of the row maximum' % err)
    assert err <= 1e-12
    own = NP.prod(trip, axis=1)
    _check_phases(ph, NP.angle(own), own, 'short rows %s' % route)


def test_three_chunks_are_the_one_chunk_output(ctx):
    """Five triads in chunks of 2, 2 and 1 on two streams: triplets and phases bit for bit those of one chunk."""
    rng = NP.random.default_rng(77)
    nbl, nchan, nt, ntriads = 5, 8, 4, 5
    x, bp, wts, legs, conj = _random_case(rng, nbl, nchan, nt, ntriads)
    trip1, ph1, st1 = ctx.closure_phase(x, legs, conj, bp * wts)
    trip3, ph3, st3 = ctx.closure_phase(x, legs, conj, bp * wts, budget_bytes=2 * 2 * nchan * nt * (3 * 16 + 8))
    assert st1['chunks'] == 1 and st3['chunks'] == 3 and st3['chunk_triads'] == 2 and st3['streams'] == 2
    assert NP.array_equal(trip1, trip3) and NP.array_equal(ph1, ph3)


def test_entry_rejects_bad_input(ctx):
    rng = NP.random.default_rng(1)
    x, bp, wts, legs, conj = _random_case(rng, 4, 8, 2, 3)
    bad = legs.copy()
    bad[1, 2] = 4
    with pytest.raises(ValueError, match='is row 4 of a cube of 4 baselines'):
        ctx.closure_phase(x, bad, conj, bp)
    with pytest.raises(ValueError, match='no masks were given'):
        ctx.closure_phase(x, legs, conj, bp, route='fused')
    with pytest.raises(ValueError, match='takes no delay filter'):
        ctx.closure_phase(x, legs, conj, bp, masks=NP.ones((1, 8)), route='direct')
    with pytest.raises(ValueError, match='mask_index out of range'):
        ctx.closure_phase(x, legs, conj, bp, masks=NP.ones((1, 8)), mask_index=NP.array([0, 0, 1, 0]))


def _hera19_array(nt, sky=None):
    cfg = W.config2()
    pos = LAY.array_layout('HERA-19')
    bl, ids = LAY.fold_and_sort_baselines(*LAY.baseline_generator(pos))
    assert NP.array_equal(bl, cfg['baselines'])
    labels = [(str(int(a)), str(int(b))) for a, b in ids]
    ch = cfg['channels']
    sky = cfg['sky'] if sky is None else sky
    shape = None if sky.get('fwhm_deg') is None else NP.stack((sky['fwhm_deg'], sky['fwhm_deg'], NP.zeros_like(sky['fwhm_deg'])), axis=1)
    skymod = SM.SkyModel(location=sky['altaz'], flux_ref=sky['flux_ref'], spindex=sky['spindex'], ref_freq=sky['ref_freq'], src_shape=shape)
    layout = {'positions': pos, 'labels': NP.array([str(i) for i in range(len(pos))]), 'ids': NP.arange(len(pos)), 'coords': 'ENU'}
    ia = RI.InterferometerArray(labels, bl, ch, telescope={'id': 'hera', 'shape': 'delta', 'size': 14.0, 'ocoords': 'altaz',
                                                           'orientation': NP.array([[90.0, 270.0]]), 'groundplane': None},
                                latitude=-30.7224, skycoords='altaz', pointing_coords='altaz', layout=layout)
    ia.reserve(nt)
    bpass = 0.6 + 0.4 * NP.hanning(ch.size + 2)[1:-1]
    for j in range(nt):
        ia.observe((2457000.5 + j / 64.0, 30.0 + 0.25 * j), {'Tnet': 200.0}, bpass, [90.0, 270.0], skymod, 10.7)
    return ia


def _check_class_result(ia, res, what, **filt):
    legs, conj, vec = ia.closure_leg_table(res['antenna_triplets'])
    assert NP.array_equal(NP.asarray(vec), NP.asarray(res['baseline_triplets']))
    bp, wts = NP.asarray(ia.bp), NP.asarray(ia.bp_wts)
    for name, cube, key in CUBES:
        x = NP.asarray(getattr(ia, cube))
        fw = res['spectral_weights']
        want_t, want_ph = CK.closure_phase(x, legs, conj, bp, wts, freq_wts=fw, **filt)
        trip, ph = res[key], res['closure_phase_' + name]
        assert trip.shape == (len(legs), 3) + x.shape[1:] and ph.shape == (len(legs),) + x.shape[1:]
        if not filt:
            assert NP.array_equal(trip, want_t), (what, name)
            _check_phases(ph, want_ph, NP.prod(want_t, axis=1), '%s %s' % (what, name))
        else:
            assert NP.max(NP.abs(trip - want_t) / NP.max(NP.abs(want_t), axis=2, keepdims=True)) <= 1e-12, (what, name)
            own = NP.prod(trip, axis=1)
            _check_phases(ph, NP.angle(own), own, '%s %s' % (what, name))


def test_class_level_hera19(tmp_path):
    nt = 3
    ia = _hera19_array(nt)
    ia.generate_noise(seed=11)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        ia.add_noise()
    res = ia.getClosurePhase()
    assert len(res['antenna_triplets']) == 5814 and res['spectral_weights'].shape == (1,)
    st = ia.closure_stats
    assert set(st) == {'skyvis', 'vis', 'noisevis'} and all(v['route'] == 'direct' for v in st.values())
    assert st['skyvis']['resident'] and not st['vis']['resident'] and not st['noisevis']['resident']      # read where it lies
    _check_class_result(ia, res, 'observed')
    # delay filter and spectral window on a few triads, against the checker
    few = res['antenna_triplets'][::400]
    nchan, df = ia.channels.size, ia.freq_resolution
    dtau = 1.0 / (nchan * df)
    r2 = ia.getClosurePhase(antenna_triplets=few, delay_filter_info={'type': 'horizon', 'mode': 'discard', 'width': 2.0},
                            spectral_window_info={'freq_center': None, 'bw_eff': None, 'shape': 'bhw', 'fftpow': None})
    assert r2['spectral_weights'].shape == (nchan,) and all(v['route'] == 'fused' for v in ia.closure_stats.values())
    _check_class_result(ia, r2, 'filtered', delay_filter=('horizon', 'discard', 0.0, 2.0 * dtau), baseline_lengths=ia.baseline_lengths, df=df)


def _noisy(ia, seed):
    ia.generate_noise(seed=seed)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        ia.add_noise()
    return ia


def test_class_level_round_trip_through_init_file(tmp_path):
    """save() -> init_file: the loaded array (its cube uploaded into the device slots again) gives over all triads what the observed
    one gave, and that matches the checker."""
    from prisim_amd import hdf5io
    from prisim_amd.dsp_readings import _key
    try:
        hdf5io._load()
    except hdf5io.HDF5Unavailable as exc:
        pytest.skip('no HDF5 library: %s' % exc)
    ia = _noisy(_hera19_array(3), 12)
    res = ia.getClosurePhase()
    fname = ia.save(str(tmp_path / 'sim'), fmt='HDF5', npz=False, overwrite=True, verbose=False)
    ib = RI.InterferometerArray(None, None, None, init_file=fname)
    assert ib.bl_reversemap is None and ib.blgroups is None          # none was given, none is invented
    rb = ib.getClosurePhase()
    assert ib.closure_stats['skyvis']['resident'] and len(rb['antenna_triplets']) == 5814
    assert [_key(t) for t in rb['antenna_triplets']] == [_key(t) for t in res['antenna_triplets']]
    _check_class_result(ib, rb, 'loaded')
    for key in ('skyvis', 'vis', 'noisevis', 'closure_phase_skyvis', 'closure_phase_vis', 'closure_phase_noise'):
        assert NP.array_equal(rb[key], res[key]), key


def test_class_level_resident_cube_through_the_tile_kernel():
    """16 snapshots: the noiseless cube is read where it lies and goes through the LDS-tile kernel; every 40th triad."""
    ia = _noisy(_hera19_array(16), 13)
    few = ia.getThreePointCombinations()[0][::40]
    res = ia.getClosurePhase(antenna_triplets=few)
    st = ia.closure_stats
    assert st['skyvis']['resident'] and st['skyvis']['tile'] == 1 and not st['vis']['resident'] and st['vis']['tile'] == 0
    _check_class_result(ia, res, 'observed, 16 snapshots')


def test_point_source_at_the_phase_centre_has_zero_closure_phase():
    """Physical check, independent of the checker: every leg of a noiseless point source at the phase centre is real to the suite's
    fp64 sky-sum tolerance of 1e-11, so the closure phase of three legs is at most 3e-11 in modulus on every triad."""
    sky = {'altaz': NP.array([[90.0, 270.0]]), 'flux_ref': NP.array([1.0]), 'spindex': NP.array([0.0]), 'ref_freq': 150e6, 'fwhm_deg': None}
    ia = _hera19_array(2, sky=sky)
    res = ia.getClosurePhase()
    assert res['closure_phase_vis'] is None and res['vis'] is None and res['noisevis'] is None
    assert len(res['antenna_triplets']) == 5814
    assert NP.min(NP.abs(res['skyvis'])) > 0.5                 # unit flux under a unit delta beam, bandpass >= 0.6: no leg is empty
    worst = float(NP.max(NP.abs(res['closure_phase_skyvis'])))
    print('largest |closure phase| of a point source at the phase centre %.3e' % worst)
    assert worst <= 3e-11
