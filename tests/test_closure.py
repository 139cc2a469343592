"""CPU: antenna triads, the leg table and the numpy restatement of the closure phases against tests/golden/golden_closure.npz (the
reference's getThreePointCombinations and getClosurePhase executed, tests/golden/make_golden_closure.py); argument validation of
getClosurePhase; the ctypes mirror of prisim_closure_stats against the compiled header."""
import os
import types
import warnings

import numpy as NP
import pytest

import closure_checker as CK
from prisim_amd import _abi
from prisim_amd import interferometry as RI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = NP.load(os.path.join(ROOT, 'tests', 'golden', 'golden_closure.npz'))
PHASE_BOUND = 32 * 2.0 ** -53            # |exp(i a) - exp(i b)|: two complex products per side (4 sqrt(5) u) and an atan2 of 2 ulp per side


def standin(**attrs):
    """the attributes the host methods read, with InterferometerArray's methods bound"""
    s = types.SimpleNamespace(**attrs)
    for name in ('getThreePointCombinations', 'closure_leg_table', 'getClosurePhase'):
        setattr(s, name, types.MethodType(getattr(RI.InterferometerArray, name), s))
    return s


def layout_of(pos):
    return {'positions': pos, 'labels': NP.array([str(i) for i in range(len(pos))]), 'ids': NP.arange(len(pos)), 'coords': 'ENU'}


def cp_standin():
    labels = [tuple(x) for x in GOLD['cp_labels'].tolist()]
    return standin(labels=labels, baselines=GOLD['cp_baselines'], bl_reversemap={lab: lab for lab in labels})


@pytest.mark.parametrize('tag', ['hera19', 'hera19red', 'irr'])
@pytest.mark.parametrize('unique', [False, True])
def test_triads_equal_the_reference(tag, unique):
    s = standin(layout=layout_of(GOLD[tag + '_pos']), baselines=GOLD[tag + '_bl'])
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        ant, vec = s.getThreePointCombinations(unique=unique)
    key = '%s_%s' % (tag, 'unique' if unique else 'all')
    assert [tuple(str(a) for a in t) for t in ant] == [tuple(t) for t in GOLD[key + '_ant'].tolist()]
    assert NP.array_equal(NP.asarray(vec, dtype=NP.float64).reshape(-1, 3, 3), GOLD[key + '_vec'])
    assert len(w) == int(GOLD[key + '_nwarn'])
    if tag == 'irr':
        assert len(w) > 0 and all('not found in the simulated reference baselines' in str(x.message) for x in w)


def test_triads_reject_a_non_boolean_unique():
    s = standin(layout=layout_of(GOLD['irr_pos']), baselines=GOLD['irr_bl'])
    with pytest.raises(TypeError, match='unique must be boolean'):
        s.getThreePointCombinations(unique=1)


def test_leg_table_equals_the_reference_and_covers_every_conjugation_pattern():
    s = cp_standin()
    trip = [tuple(t) for t in GOLD['cp_triplets'].tolist()]
    legs, conj, vec = s.closure_leg_table(trip)
    assert legs.shape == conj.shape == (len(trip), 3) and legs.dtype == conj.dtype == NP.int32
    assert len(set(map(tuple, conj.tolist()))) == 8
    assert NP.array_equal(NP.asarray(vec), GOLD['cp_out_baseline_triplets'])
    # the rows themselves: the reference's gather, redone from the table, gives its triplets
    for name, cube in (('skyvis', 'skyvis_freq'), ('vis', 'vis_freq'), ('noisevis', 'vis_noise_freq')):
        t, _ = CK.closure_phase(GOLD['cp_' + cube], legs, conj, GOLD['cp_bp'], GOLD['cp_bp_wts'])
        assert NP.array_equal(t, GOLD['cp_out_' + name])


def red_standin():
    """HERA-19 with redundant folding: 171 antenna pairs mapped onto the 30 simulated baselines"""
    labels = [tuple(x) for x in GOLD['hera19red_labels'].tolist()]
    rev = {tuple(k): tuple(v) for k, v in zip(GOLD['hera19red_rev_keys'].tolist(), GOLD['hera19red_rev_vals'].tolist())}
    return standin(labels=labels, baselines=GOLD['hera19red_bl'], bl_reversemap=rev)


def test_leg_table_through_a_many_to_one_reversemap_equals_the_reference():
    s = red_standin()
    assert len(s.bl_reversemap) == 171 and len(set(s.bl_reversemap.values())) == len(s.labels) < 171
    legs, conj, vec = s.closure_leg_table([tuple(t) for t in GOLD['redcp_triplets'].tolist()])
    assert NP.array_equal(NP.asarray(vec), GOLD['redcp_out_baseline_triplets'])
    for name, cube, key in (('skyvis', 'skyvis_freq', 'skyvis'), ('vis', 'vis_freq', 'vis'), ('noise', 'vis_noise_freq', 'noisevis')):
        t, ph = CK.closure_phase(GOLD['redcp_' + cube], legs, conj, GOLD['redcp_bp'], GOLD['redcp_bp_wts'])
        assert NP.array_equal(t, GOLD['redcp_out_' + key])
        assert not NP.any(NP.prod(t, axis=1) == 0)
        assert CK.phase_deviation(ph, GOLD['redcp_out_closure_phase_' + name]).max() <= PHASE_BOUND
    s.bl_reversemap[('1', '0')] = ('99', '98')               # a value that is no simulated baseline
    with pytest.raises(ValueError, match='not found in simulated baselines'):
        s.closure_leg_table([('0', '1', '2')])


def test_leg_table_identity_map_and_missing_baseline():
    s = cp_standin()
    s.bl_reversemap = None                                   # no blgroupinfo: the identity map of the labels
    trip = [tuple(t) for t in GOLD['cp_triplets'].tolist()]
    legs, conj, _ = s.closure_leg_table(trip)
    s2 = cp_standin()
    legs2, conj2, _ = s2.closure_leg_table(trip)
    assert NP.array_equal(legs, legs2) and NP.array_equal(conj, conj2) and s.bl_reversemap is None
    with pytest.raises(ValueError, match='not found in simulated baselines'):
        s.closure_leg_table([('0', '4', '1')])             # the pair (0, 4) was not simulated


def test_checker_equals_the_reference_on_the_no_filter_branch():
    s = cp_standin()
    legs, conj, _ = s.closure_leg_table([tuple(t) for t in GOLD['cp_triplets'].tolist()])
    nchan = GOLD['cp_channels'].size
    for name, cube in (('skyvis', 'skyvis_freq'), ('vis', 'vis_freq'), ('noise', 'vis_noise_freq')):
        t, ph = CK.closure_phase(GOLD['cp_' + cube], legs, conj, GOLD['cp_bp'], GOLD['cp_bp_wts'])
        ref_t = GOLD['cp_out_' + ('noisevis' if name == 'noise' else name)]
        ref_ph = GOLD['cp_out_closure_phase_' + name]
        assert NP.array_equal(t, ref_t)
        zero = NP.prod(ref_t, axis=1) == 0
        flagged = NP.zeros_like(zero)
        flagged[:, 7, :] = True
        assert NP.array_equal(zero, flagged) and zero.mean() == 1.0 / nchan
        dev = CK.phase_deviation(ph, ref_ph)[~zero]
        print(name, 'largest phase deviation', dev.max())
        assert dev.max() <= PHASE_BOUND
        assert NP.all(NP.isfinite(ph))


def test_filter_masks_equal_the_checker():
    nchan, df = 32, 1e5
    tau = NP.fft.fftfreq(nchan, df)
    dtau = tau[1] - tau[0]
    lengths = NP.array([14.6, 14.6, 29.2, 250.0])
    for mode in ('discard', 'retain'):
        m, idx = RI.closure_filter_masks(tau, 'regular', mode, 2 * dtau, 3 * dtau, lengths)
        assert idx is None and NP.array_equal(m[0], CK.filter_unmask(tau, 'regular', mode, 2 * dtau, 3 * dtau))
        m, idx = RI.closure_filter_masks(tau, 'horizon', mode, 0.0, 1.5 * dtau, lengths)
        assert idx.dtype == NP.int32 and m.shape[0] <= lengths.size
        for b, length in enumerate(lengths):
            assert NP.array_equal(m[idx[b]], CK.filter_unmask(tau, 'horizon', mode, 0.0, 1.5 * dtau, length))


def test_argument_validation_and_refusals():
    s = cp_standin()
    s.channels, s.freq_resolution = GOLD['cp_channels'], 1e5
    trip = [tuple(t) for t in GOLD['cp_triplets'].tolist()]
    with pytest.raises(TypeError, match='list of triplet tuples'):
        s.getClosurePhase(antenna_triplets=tuple(trip))
    with pytest.raises(NotImplementedError, match='specsmooth_info'):
        s.getClosurePhase(antenna_triplets=trip, specsmooth_info={'op_type': 'median', 'window_size': 3})
    with pytest.raises(NotImplementedError):
        s.getClosurePhase(antenna_triplets=trip, spectral_window_info={'freq_center': None, 'bw_eff': None, 'shape': 'bhw', 'fftpow': 2.0})
    with pytest.raises(ValueError, match='fftpow must be positive'):
        s.getClosurePhase(antenna_triplets=trip, spectral_window_info={'freq_center': None, 'bw_eff': None, 'shape': None, 'fftpow': -1.0})
    with pytest.raises(ValueError, match='window shape not currently supported'):
        s.getClosurePhase(antenna_triplets=trip, spectral_window_info={'freq_center': None, 'bw_eff': None, 'shape': 'bnw', 'fftpow': None})
    with pytest.raises(TypeError, match='must be specified as a dictionary'):
        s.getClosurePhase(antenna_triplets=trip, delay_filter_info=[1])
    with pytest.raises(ValueError, match='Invalid delay filter mode'):
        s.getClosurePhase(antenna_triplets=trip, delay_filter_info={'mode': 'keep'})
    with pytest.raises(ValueError, match='Invalid delay filter type'):
        s.getClosurePhase(antenna_triplets=trip, delay_filter_info={'type': 'wedge'})
    with pytest.raises(KeyError):
        s.getClosurePhase(antenna_triplets=trip, delay_filter_info={'type': 'regular', 'min': 0.0})
    with pytest.raises(ValueError, match='width must be positive'):
        s.getClosurePhase(antenna_triplets=trip, delay_filter_info={'type': 'regular', 'min': 0.0, 'width': 0.0})
    with pytest.raises(TypeError, match='Minimum delay'):
        s.getClosurePhase(antenna_triplets=trip, delay_filter_info={'type': 'regular', 'min': '0', 'width': 1.0})
    with pytest.raises(TypeError, match='Delay width'):
        s.getClosurePhase(antenna_triplets=trip, delay_filter_info={'type': 'horizon', 'width': '1'})


def test_init_file_reads_blgroupinfo_back(tmp_path, monkeypatch):
    """save() writes blgroupinfo/groups and blgroupinfo/reversemap; the init_file loader reads them back (interferometry.py:5390-5397)."""
    import fake_context
    from prisim_amd import hdf5io
    try:
        hdf5io.File(str(tmp_path / 'probe.hdf5'), 'w').close()
    except hdf5io.HDF5Unavailable:
        pytest.skip('no HDF5 library')
    from prisim_amd import skymodel as SM
    monkeypatch.setattr(_abi, 'Context', fake_context.OracleContext)
    ch = 150e6 + 1e5 * NP.arange(4)
    bl = NP.array([[14.6, 0.0, 0.0], [7.3, 12.6, 0.0], [-7.3, 12.6, 0.0]])
    labels = [('1', '0'), ('2', '0'), ('2', '1')]
    layout = layout_of(NP.array([[0.0, 0, 0], [14.6, 0, 0], [7.3, 12.6, 0]]))
    groups = {('1', '0'): [('1', '0')], ('2', '0'): [('2', '0')], ('2', '1'): [('2', '1')]}
    rev = {m: k for k, v in groups.items() for m in v}
    ia = RI.InterferometerArray(labels, bl, ch, telescope={'id': 'hera', 'shape': 'delta', 'size': 14.0, 'ocoords': 'altaz',
                                                           'orientation': NP.array([[90.0, 270.0]]), 'groundplane': None},
                                latitude=-30.7, skycoords='altaz', layout=layout, blgroupinfo={'groups': groups, 'reversemap': rev})
    skymod = SM.SkyModel(location=[[80.0, 100.0], [50.0, 10.0]], flux_ref=[1.0, 3.0], spindex=[0.0, -0.7], ref_freq=150e6)
    tsys = {'Trx': 100.0, 'Tant': {'f0': 150e6, 'T0': 200.0, 'spindex': -2.5}, 'Tnet': None}
    ia.observe((2457000.5, 10.0), tsys, NP.ones(4), [0.0, -30.7], skymod, 10.7)
    fname = ia.save(str(tmp_path / 'sim'), fmt='HDF5', npz=False, overwrite=True, verbose=False)
    ib = RI.InterferometerArray(None, None, None, init_file=fname)
    assert ib.bl_reversemap == rev and ib.blgroups == groups
    ant, _ = ib.getThreePointCombinations()
    legs, conj, _ = ib.closure_leg_table(ant)
    legs0, conj0, _ = ia.closure_leg_table(ant)
    assert len(ant) == 6 and NP.array_equal(legs, legs0) and NP.array_equal(conj, conj0)
