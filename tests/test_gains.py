"""Gain tables on the host (prisim_amd/gains.py): file round trips through hdf5io (gzip included), argument checks, label resolution,
the find_list_in_list reading, the packed splines against scipy and the reference's fixtures, and the class surface.  No GPU."""
import os
import warnings

import numpy as NP
import pytest

from prisim_amd import dsp_readings as R
from prisim_amd import gains as G
from prisim_amd import hdf5io

import gains_checker as GC


@pytest.fixture(scope='module')
def golden():
    return GC.load_golden()


def _info(golden, name, tmp_path):
    z, recs = golden
    path = str(tmp_path / (name + '.hdf5'))
    GC.write_case(z, recs[name], path)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return G.GainInfo(init_file=path, axes_order=['label', 'frequency', 'time'])


def test_find_list_in_list_known_answers():
    ind = R.find_list_in_list(['label', 'frequency', 'time'], ['time', 'label', 'frequency'])
    assert ind.tolist() == [2, 0, 1] and not NP.any(ind.mask)
    ind = R.find_list_in_list(NP.array(['a', 'b', 'a']), ['a', 'c', b'b'])
    assert ind.data[0] == 0 and bool(ind.mask[1]) and ind.data[1] == -1 and ind.data[2] == 1
    bl = NP.array([('1', '0'), ('2', '1')], dtype=[('A2', 'U2'), ('A1', 'U2')])
    q = NP.array([('2', '1'), ('0', '1'), ('1', '0')], dtype=[('A2', 'S2'), ('A1', 'S2')])
    ind = R.find_list_in_list(bl, q)
    assert ind.tolist() == [1, None, 0]
    with pytest.raises(TypeError):
        R.find_list_in_list(None, ['a'])


def test_label_forms_resolve_alike():
    want = [('1', '0'), ('HH3', 'HH2')]
    a = G.bl_label_array([('1', '0'), ('HH3', 'HH2')])
    b = G.bl_label_array(NP.array([(b'1', b'0'), (b'HH3', b'HH2')], dtype=[('A2', 'S3'), ('A1', 'S3')]))
    c = G.bl_label_array(['1-0', 'HH3-HH2'])
    for arr in (a, b, c):
        assert [tuple(x) for x in arr.tolist()] == want
    assert G._split_label('X-1-X-12') == ('X-1', 'X-12')
    with pytest.raises(TypeError):
        G.bl_label_array([3.5])


def test_table_round_trip_with_gzip(tmp_path, golden):
    info = _info(golden, 'both2d', tmp_path)
    out = str(tmp_path / 'rt.hdf5')
    info.write_gaintable(out)
    with hdf5io.File(out, 'r') as f:
        assert f.nfilters('antenna-based/gains') == (1 if f.deflate_available() else 0)
    back = G.GainInfo(init_file=out)
    for key in G.GAINKEYS:
        for sub in ('gains', 'frequency', 'time'):
            assert NP.array_equal(back.gaintable[key][sub], info.gaintable[key][sub])
        assert [tuple(x) if isinstance(x, tuple) else x for x in back.gaintable[key]['label'].tolist()] == \
            [tuple(x) if isinstance(x, tuple) else x for x in info.gaintable[key]['label'].tolist()]
    info.write_gaintable(str(tmp_path / 'plain.hdf5'), compress=False)
    with hdf5io.File(str(tmp_path / 'plain.hdf5'), 'r') as f:
        assert f.nfilters('antenna-based/gains') == 0


def test_argument_checks(tmp_path, golden):
    with pytest.raises(TypeError):
        G.read_gaintable('x.hdf5', axes_order='label')
    with pytest.raises(ValueError):
        G.read_gaintable('x.hdf5', axes_order=['label', 'frequency'])
    with pytest.raises(ValueError):
        G.read_gaintable('x.hdf5', axes_order=['label', 'frequency', 'lst'])
    with pytest.warns(UserWarning, match='Invalid file'):
        assert G.read_gaintable(str(tmp_path / 'absent.hdf5')) is None
    info = _info(golden, 'ant2d', tmp_path)
    with pytest.raises(TypeError):
        info.splinator(smoothness='a')
    with pytest.raises(ValueError):
        info.splinator(smoothness=-1.0)
    with pytest.raises(ValueError):
        info.read_gaintable('x', action='keep')
    assert isinstance(info.read_gaintable('x', action=3), TypeError)          # returned, not raised (:3040)
    with pytest.raises(NotImplementedError, match='interp2d'):
        info.interpolator()
    with pytest.raises(NotImplementedError, match='spline_gains'):
        info.interpolate_gains(GC.bl_struct([('1', '0')]))
    with pytest.raises(TypeError):
        info.write_gaintable(str(tmp_path / 'o.hdf5'), compress='yes')
    with pytest.raises(ValueError):
        info.write_gaintable(str(tmp_path / 'o.hdf5'), compress_fmt='bz2')


def test_packed_splines_match_scipy_and_the_fixtures(tmp_path, golden):
    z, recs = golden
    for name in ('ant2d', 'both2d', 'retry_offset', 'both_blfreq'):
        info = _info(golden, name, tmp_path)
        qf, qt = z[name + '/qf'], z[name + '/qt']
        ev = {}
        for key in G.GAINKEYS:
            pk = info.packed[key]
            if pk is None:
                continue
            dims = pk['dims']
            tt = qt if 'time' in dims else NP.zeros(1)
            ff = qf if 'frequency' in dims else NP.zeros(1)
            ev[key] = GC.eval_packed(pk, tt, ff)
            interp = info.splinefuncs[key]['interp']
            for r in range(interp.shape[0]):
                for part, sign in (('real', 1.0), ('imag', 1.0)):
                    spl = interp[part][r]
                    if dims.size == 2:
                        T, F = NP.meshgrid(tt, ff, indexing='ij')
                        ref = spl.ev(T, F)                                  # (nt, nf)
                    elif dims[0] == 'time':
                        ref = spl(tt)[:, None]
                    else:
                        ref = spl(ff)[None, :]
                    got = ev[key][:, r, :].real if part == 'real' else ev[key][:, r, :].imag
                    assert NP.max(NP.abs(got - ref)) <= 1e-13 * max(1.0, NP.max(NP.abs(ref)))
        if recs[name]['results']['spline'] != 'ok':
            continue
        # the reference's product from the checker's tables: conj(g[A1]) g[A2] g_bl, (nbl, nchan, nt)
        query = GC.bl_struct(z['query'].tolist())
        g = NP.ones((query.size, qf.size, qt.size if 'antenna-based' in ev and ev['antenna-based'].shape[0] > 1 else 1), dtype=complex)
        if 'antenna-based' in ev:
            lab = list(info.gaintable['antenna-based']['label'])
            i1 = [lab.index(a) for a in query['A1']]
            i2 = [lab.index(a) for a in query['A2']]
            T = NP.transpose(ev['antenna-based'], (1, 2, 0))
            g = NP.conj(T[i1]) * T[i2]
        if 'baseline-based' in ev:
            rows, cj = G.GainInfo._bl_rows(info.gaintable['baseline-based']['label'], query)
            T = NP.transpose(ev['baseline-based'], (1, 2, 0))
            gb = NP.ones((query.size,) + T.shape[1:], dtype=complex)
            for b in range(query.size):
                if rows[b] >= 0:
                    gb[b] = NP.conj(T[rows[b]]) if cj[b] else T[rows[b]]
            g = g * gb
        want = z[name + '/spline']
        assert NP.max(NP.abs(g - want)) <= 1e-13 * NP.max(NP.abs(want))


def test_first_smoothness_is_kept_for_later_tables():
    """An antenna table of 10 x 7 samples sets s = 70; the baseline table after it has 6 x 5 samples and rough data, so its fit under
    the kept s = 70 differs from a fit under its own sample count (30) -- the reference keeps 70."""
    from scipy import interpolate
    rng = NP.random.default_rng(11)
    fa, ta = NP.linspace(1e8, 1.1e8, 10), NP.arange(7.0)
    fb, tb = NP.linspace(1e8, 1.1e8, 6), NP.arange(5.0)
    info = G.GainInfo()
    info.gaintable = {
        'antenna-based': {'gains': rng.standard_normal((2, 10, 7)) + 1j, 'label': NP.array(['0', '1']), 'frequency': fa, 'time': ta,
                          'ordering': ['label', 'frequency', 'time']},
        'baseline-based': {'gains': 3.0 * rng.standard_normal((1, 6, 5)) + 0j, 'label': None, 'frequency': fb, 'time': tb,
                           'ordering': ['label', 'frequency', 'time']}}
    info.splinator()
    z = info.gaintable['baseline-based']['gains'][0].real.T
    bbox = [tb.min(), tb.max(), fb.min(), fb.max()]
    kept = interpolate.RectBivariateSpline(tb, fb, z, bbox=bbox, s=70)
    own = interpolate.RectBivariateSpline(tb, fb, z, bbox=bbox, s=30)
    got = info.splinefuncs['baseline-based']['interp']['real'][0]
    assert all(NP.array_equal(x, y) for x, y in zip(got.tck, kept.tck))
    T, F = NP.meshgrid(tb, fb, indexing='ij')
    assert NP.max(NP.abs(kept.ev(T, F) - own.ev(T, F))) > 1e-3 * NP.max(NP.abs(z))      # the kept s changes the fit


def test_driver_gains_key(tmp_path, golden):
    from prisim_amd import driver
    p = driver.deep_merge(driver.DEFAULTS, {})
    assert driver.build_gaininfo(p) is None
    p['gains'] = {'file': 'hera.hdf5', 'filepathtype': 'default'}
    with pytest.raises(NotImplementedError, match='prisim/data/gains'):
        driver.build_gaininfo(p)
    p['gains'] = {'file': 3, 'filepathtype': 'custom'}
    with pytest.raises(TypeError):
        driver.build_gaininfo(p)
    z, recs = golden
    path = str(tmp_path / 'g.hdf5')
    GC.write_case(z, recs['both2d'], path)
    p['gains'] = {'file': path, 'filepathtype': 'custom'}
    gi = driver.build_gaininfo(p)
    assert isinstance(gi, G.GainInfo) and gi.gaintable['antenna-based']['ordering'] == ['label', 'frequency', 'time']


def test_driver_labels_resolve_against_a_table(tmp_path):
    """The driver's '{A2}-{A1}' strings resolve to the antennas of a table written for them; padding rows are left out."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import dist_worker
    import test_gpu_gains_driver as TD
    from prisim_amd import driver
    parms = dist_worker.parms_for_test()
    path = str(tmp_path / 'g.hdf5')
    TD.write_gains_for(parms, path)
    gi = G.GainInfo(init_file=path)
    _, labels, _, _ = driver.baseline_info(parms)
    lab = G.bl_label_array(labels)
    jd = NP.asarray(driver.schedule(parms)[0])
    from prisim_amd import workloads as W
    bp = parms['bandpass']
    ch = W.channel_grid(float(bp['freq']), float(bp['freq_resolution']), int(bp['nchan']))
    plan = gi.spline_plan(lab, freqs=ch, times=jd)
    assert plan.shape == (len(labels), ch.size, jd.size) and len(plan.factors) == 2
    rows, cj = G.GainInfo._bl_rows(gi.gaintable['baseline-based']['label'], lab)
    assert NP.sum(rows >= 0) == gi.gaintable['baseline-based']['gains'].shape[0]


def test_constant_table_has_no_splines(tmp_path, golden):
    info = _info(golden, 'const', tmp_path)
    assert info.splinefuncs['antenna-based'] is None
    z, recs = golden
    plan = info.spline_plan(GC.bl_struct(z['query'].tolist()), freqs=z['const/qf'], times=z['const/qt'])
    assert plan.factors == [] and plan.shape == (1, 1, 1)
    assert recs['const']['results']['spline'] == 'ok' and z['const/spline'].shape == (1, 1, 1)


def test_plans_raise_what_the_reference_raises(tmp_path, golden):
    z, recs = golden
    query = GC.bl_struct(z['query'].tolist())
    for name, rec in recs.items():
        info = _info(golden, name, tmp_path)
        qf, qt = z[name + '/qf'], z[name + '/qt']
        calls = {'spline': lambda: info.spline_plan(query, freqs=qf, times=qt),
                 'spline_ordered': lambda: info.spline_plan(query, freqs=qf, times=qt, axes_order=['label', 'frequency', 'time']),
                 'nearest': lambda: info.nearest_plan(query, freqs=qf, times=qt)}
        for cname, fn in calls.items():
            want = rec['results'][cname]
            if want == 'ok':
                plan = fn()
                n0, nf, nt = plan.shape
                assert tuple(plan.shape[p] for p in plan.perm) == z[name + '/' + cname].shape, (name, cname)
            else:
                with pytest.raises(Exception) as exc:
                    fn()
                assert type(exc.value).__name__ == want, (name, cname)


def test_interferometer_array_takes_a_gaininfo(tmp_path, golden):
    from prisim_amd import interferometry as RI
    assert RI.GainInfo is G.GainInfo and RI.read_gaintable is G.read_gaintable and RI.extract_gains is G.extract_gains
    with pytest.raises(TypeError, match='GainInfo'):
        RI.InterferometerArray(['1-0'], NP.array([[14.6, 0.0, 0.0]]), NP.array([150e6]), gaininfo={'gains': 1})


def test_extract_gains_is_the_reference_statement(tmp_path, golden):
    z, recs = golden
    query = GC.bl_struct(z['query'].tolist())
    for name, rec in recs.items():
        info = _info(golden, name, tmp_path)
        if rec['results']['eval'] == 'ok':
            assert NP.array_equal(G.extract_gains(info.gaintable, query), z[name + '/eval'])
        else:
            with pytest.raises(Exception) as exc:
                G.extract_gains(info.gaintable, query)
            assert type(exc.value).__name__ == rec['results']['eval']
