"""GPU: gain tables (include/prisim_gains.h) -- the device evaluation against the reference's fixtures (tests/golden/golden_gains.npz),
a HERA-350-sized table against scipy, and add_noise through the class (host, resident and memsave skies, the fallback chain) against
the host statement gains * skyvis + noise."""
import os
import sys
import warnings

import numpy as NP
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gains_checker as GC  # noqa: E402

from prisim_amd import gains as G, skymodel as SM, workloads as W  # noqa: E402

pytestmark = pytest.mark.gpu


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


def test_device_evaluation_against_every_fixture(tmp_path, golden):
    z, recs = golden
    query = GC.bl_struct(z['query'].tolist())
    for name, rec in recs.items():
        info = _info(golden, name, tmp_path)
        qf, qt = z[name + '/qf'], z[name + '/qt']
        calls = {'spline': lambda: info.spline_gains(query, freqs=qf, times=qt),
                 'spline_ordered': lambda: info.spline_gains(query, freqs=qf, times=qt, axes_order=['label', 'frequency', 'time']),
                 'nearest': lambda: info.nearest_gains(query, freqs=qf, times=qt),
                 'eval': lambda: info.eval_gains(query, freq_index=[0], time_index=[0])}      # indices ignored, as there
        for cname, fn in calls.items():
            want = rec['results'][cname]
            if want == 'ok':
                got, ref = fn(), z[name + '/' + cname]
                assert got.shape == ref.shape, (name, cname)
                assert NP.max(NP.abs(got - ref)) <= 1e-13 * max(NP.max(NP.abs(ref)), 1e-300), (name, cname)
            else:
                with pytest.raises(Exception) as exc:
                    fn()
                assert type(exc.value).__name__ == want, (name, cname)


def test_hera350_table_against_scipy(tmp_path):
    from scipy import interpolate
    rng = NP.random.default_rng(5)
    nant, nchan, nt = 350, 1024, 120
    f = NP.linspace(100e6, 200e6, nchan)
    t = 2459000.0 + NP.arange(nt) / 720.0
    ga = (1.0 + 0.05 * NP.cos(NP.linspace(0, 20, nchan))[None, :, None] + 0.01 * rng.standard_normal((nant, 1, nt))) \
        * NP.exp(1j * rng.uniform(-1, 1, (nant, 1, 1)))
    from prisim_amd import hdf5io
    path = str(tmp_path / 'hera.hdf5')
    with hdf5io.File(path, 'w') as fo:
        fo.write('antenna-based/gains', ga)
        fo.write('antenna-based/ordering', NP.array(['label', 'frequency', 'time']))
        fo.write('antenna-based/label', NP.array([str(i) for i in range(nant)]))
        fo.write('antenna-based/frequency', f)
        fo.write('antenna-based/time', t)
    info = G.GainInfo(init_file=path)
    pk = info.packed['antenna-based']
    ctx = G._device()
    tab, st = ctx.gains_eval_spline(pk, t, f)
    got = tab.get()
    tab.close()
    print('HERA-350 x 1024 x 120 evaluation: {0:.3f} ms kernels, {1:.3f} ms with transfers'.format(st['kernel_ms'], st['device_ms']))
    T, F = NP.meshgrid(t, f, indexing='ij')
    for r in rng.choice(nant, 12, replace=False):
        sr, si = info.splinefuncs['antenna-based']['interp'][r]
        ref = sr.ev(T, F) + 1j * si.ev(T, F)
        assert NP.max(NP.abs(got[:, r, :] - ref)) <= 1e-13 * NP.max(NP.abs(ref))


def _gain_file(path, labels, ch, times, nant, rng, with_bl=True):
    from prisim_amd import hdf5io
    ga = (1.0 + 0.05 * NP.cos(NP.linspace(0, 6, ch.size))[None, :, None] + 0.02 * NP.linspace(-1, 1, times.size)[None, None, :]) \
        * NP.exp(1j * rng.uniform(-1, 1, (nant, 1, 1)))
    with hdf5io.File(path, 'w') as fo:
        fo.write('antenna-based/gains', ga)
        fo.write('antenna-based/ordering', NP.array(['label', 'frequency', 'time']))
        fo.write('antenna-based/label', NP.array([str(i) for i in range(nant)]))
        fo.write('antenna-based/frequency', ch)
        fo.write('antenna-based/time', times)
        if with_bl:
            bl = labels[::3]
            gb = 1.0 + 0.1 * rng.standard_normal((len(bl), 1, 1)) + 0.05j * NP.sin(NP.linspace(0, 3, ch.size))[None, :, None] \
                + 0.01 * NP.linspace(-1, 1, times.size)[None, None, :]
            fo.write('baseline-based/gains', gb)
            fo.write('baseline-based/ordering', NP.array(['label', 'frequency', 'time']))
            fo.write('baseline-based/label', GC.bl_struct([tuple(reversed(x)) if i % 2 else x for i, x in enumerate(bl)]))
            fo.write('baseline-based/frequency', ch)
            fo.write('baseline-based/time', times)


def _config2_array(nt, gaininfo_path=None, memsave=False):
    from prisim_amd import interferometry as RI
    cfg = W.config2()
    bl, ch, sky = cfg['baselines'], cfg['channels'], cfg['sky']
    skymod = SM.SkyModel(location=sky['altaz'], flux_ref=sky['flux_ref'], spindex=sky['spindex'], ref_freq=sky['ref_freq'],
                         src_shape=NP.stack((sky['fwhm_deg'], sky['fwhm_deg'], NP.zeros_like(sky['fwhm_deg'])), axis=1))
    labels = [(str(i + 1), str(i // 2)) for i in range(bl.shape[0])]
    gi = None if gaininfo_path is None else G.GainInfo(init_file=gaininfo_path)
    ia = RI.InterferometerArray(labels, bl, ch, telescope={'id': 'hera'}, latitude=-30.7224, skycoords='altaz',
                                pointing_coords='altaz', gaininfo=gi)
    ia.reserve(nt)
    bpass = 0.6 + 0.4 * NP.hanning(ch.size + 2)[1:-1]
    for j in range(nt):
        ia.observe((2457000.5 + j / 64.0, 30.0 + 0.25 * j), {'Tnet': 200.0}, bpass, [90.0, 270.0], skymod, 10.7, memsave=memsave)
    ia.generate_noise(seed=11)
    return ia, labels


def _host_statement(ia, gains):
    return gains * ia.skyvis_freq + ia.vis_noise_freq


@pytest.mark.parametrize('memsave', [False, True])
def test_add_noise_resident_and_overridden_sky(tmp_path, memsave):
    nt = 64
    rng = NP.random.default_rng(3)
    cfg = W.config2()
    ch, nbl = cfg['channels'], cfg['baselines'].shape[0]
    labels = [(str(i + 1), str(i // 2)) for i in range(nbl)]
    times = 2457000.5 + NP.arange(nt) / 64.0
    path = str(tmp_path / 'g.hdf5')
    _gain_file(path, labels, ch, times, nbl + 1, rng)
    ia, labels = _config2_array(nt, path, memsave=memsave)
    assert ia._device_in_step
    ia.add_noise()                                           # resident sky
    vis_res = ia.vis_freq
    gains = ia.gaininfo.spline_gains(ia.gain_labels(), freqs=ia.channels, times=NP.asarray(ia.timestamp))
    want = _host_statement(ia, gains)
    scale = NP.abs(gains) * NP.abs(ia.skyvis_freq) + NP.abs(ia.vis_noise_freq)
    assert NP.max(NP.abs(vis_res - want) / scale) <= 1e-13
    # an overridden sky and a replaced noise cube are used as they stand
    ia.skyvis_freq = NP.asarray(ia.skyvis_freq) * (1.0 + 0.5j)
    ia.vis_noise_freq = ia.vis_noise_freq * 0.5
    ia.add_noise()
    want = _host_statement(ia, gains)
    scale = NP.abs(gains) * NP.abs(ia.skyvis_freq) + NP.abs(ia.vis_noise_freq)
    assert NP.max(NP.abs(ia.vis_freq - want) / scale) <= 1e-13


def test_add_noise_fallback_chain_against_the_fixtures(tmp_path, golden):
    from prisim_amd import interferometry as RI
    z, recs = golden
    query = [tuple(x) for x in z['query'].tolist()]
    for name, rec in recs.items():
        path = str(tmp_path / (name + '.hdf5'))
        GC.write_case(z, rec, path)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            gi = G.GainInfo(init_file=path, axes_order=['label', 'frequency', 'time'])
        qf = z[name + '/qf']
        ia = RI.InterferometerArray(query, NP.tile([[14.6, 0.0, 0.0]], (len(query), 1)), qf, gaininfo=gi)
        ia.timestamp = [float(x) for x in z[name + '/stamps']]
        ia.skyvis_freq = z[name + '/sky']
        ia.vis_noise_freq = z[name + '/noise']
        with warnings.catch_warnings(record=True) as wl:
            warnings.simplefilter('always')
            if rec['results']['add_noise'] == 'ok':
                ia.add_noise()
                ref = z[name + '/add_noise']
                assert NP.max(NP.abs(ia.vis_freq - ref)) <= 1e-13 * NP.max(NP.abs(ref)), name
            else:
                with pytest.raises(Exception) as exc:
                    ia.add_noise()
                assert type(exc.value).__name__ == rec['results']['add_noise'], name
        assert any('neighbour logic failed' in str(w.message) for w in wl) == rec['add_noise_warned'], name


def test_save_and_init_file_restore_the_gaininfo(tmp_path):
    from prisim_amd import interferometry as RI
    nt = 4
    rng = NP.random.default_rng(9)
    cfg = W.config2()
    ch, nbl = cfg['channels'], cfg['baselines'].shape[0]
    labels = [(str(i + 1), str(i // 2)) for i in range(nbl)]
    path = str(tmp_path / 'g.hdf5')
    _gain_file(path, labels, ch, 2457000.5 + NP.arange(nt) / 64.0, nbl + 1, rng)
    ia, _ = _config2_array(nt, path)
    ia.add_noise()
    out = str(tmp_path / 'sim')
    ia.save(out, verbose=False, npz=False)
    assert os.path.exists(out + '.gains.hdf5')
    back = RI.InterferometerArray(None, None, None, init_file=out)
    assert isinstance(back.gaininfo, G.GainInfo)
    for key in G.GAINKEYS:
        assert NP.array_equal(back.gaininfo.gaintable[key]['gains'], ia.gaininfo.gaintable[key]['gains'])


def test_apply_kernel_rate_on_a_config3_snapshot():
    """Apply on device-resident sky of a config-3-sized snapshot (61075 baselines x 1024 channels), antenna table of 350 rows."""
    from prisim_amd import _abi
    nbl, nchan, nant = 61075, 1024, 350
    rng = NP.random.default_rng(1)
    ctx = _abi.Context(0)
    bl = NP.zeros((nbl, 3))
    bl[:, 0] = 14.6
    ctx.set_array(bl, NP.linspace(100e6, 200e6, nchan), nt_max=1)
    tab, _ = ctx.gains_gather(NP.ones((nant, 1, 1), dtype=complex) * (1 + 0.1j), NP.zeros(nchan, dtype=NP.int64), NP.zeros(1, dtype=NP.int64))
    i1 = rng.integers(0, nant, nbl)
    i2 = rng.integers(0, nant, nbl)
    noise = NP.zeros((1, nbl, nchan), dtype=complex)
    best = None
    for _ in range(3):
        vis, st = ctx.gains_apply(1, nbl, nchan, fa=(tab, _abi.PRISIM_GAINS_ANTENNA, i1, i2), sky=None, noise=noise)
        best = st['kernel_ms'] if best is None else min(best, st['kernel_ms'])
    tb = 48.0 * nbl * nchan / (best * 1e-3) / 1e12
    print('apply config-3 snapshot: {0:.3f} ms, {1:.2f} TB/s algorithmic ({2:.2f} of 8 TB/s)'.format(best, tb, tb / 8.0))
    tab.close()
    ctx.close()
    assert NP.all(NP.isfinite(vis))


def _span_points(k, lo, hi):
    """every knot, every span's midpoint, and one point on each side outside [lo, hi]"""
    return NP.unique(NP.concatenate((k, 0.5 * (k[:-1] + k[1:]), [lo - 0.3 * (hi - lo), hi + 0.2 * (hi - lo)])))


def test_interior_knots_against_scipy():
    """Rough data of magnitude 100 with s = the sample count: fits with many interior knots, so the device's span search, clamp and
    multi-span coefficient offsets are all exercised -- 2-D (RectBivariateSpline.ev) and both 1-D forms (splev, clamped like fpbisp)."""
    from scipy import interpolate
    rng = NP.random.default_rng(2)
    f = NP.linspace(100e6, 120e6, 40)
    t = 2459000.0 + NP.arange(30) * 0.01
    ctx = G._device()
    bbox = [t.min(), t.max(), f.min(), f.max()]
    re2 = interpolate.RectBivariateSpline(t, f, 100 * rng.standard_normal((30, 40)), bbox=bbox, s=1200)
    im2 = interpolate.RectBivariateSpline(t, f, 100 * rng.standard_normal((30, 40)), bbox=bbox, s=1200)
    assert min(len(re2.tck[0]), len(re2.tck[1])) > 2 * 3 + 2 + 10           # well beyond the 2k + 2 knots of a single span
    interp = NP.empty(2, dtype=[('real', object), ('imag', object)])
    interp[0], interp[1] = (re2, im2), (im2, re2)
    tq, fq = _span_points(re2.tck[0], t.min(), t.max()), _span_points(re2.tck[1], f.min(), f.max())
    tq = NP.unique(NP.concatenate((tq, _span_points(im2.tck[0], t.min(), t.max()))))
    fq = NP.unique(NP.concatenate((fq, _span_points(im2.tck[1], f.min(), f.max()))))
    tab, _ = ctx.gains_eval_spline(G.pack_splines(interp, NP.array(['frequency', 'time'])), tq, fq)
    got = tab.get()
    tab.close()
    T, F = NP.meshgrid(tq, fq, indexing='ij')
    for r, (a, b) in enumerate(((re2, im2), (im2, re2))):
        ref = a.ev(T, F) + 1j * b.ev(T, F)
        assert NP.max(NP.abs(got[:, r, :] - ref)) <= 1e-13 * NP.max(NP.abs(ref))
    for dim, x in (('frequency', f), ('time', t)):
        sr = interpolate.UnivariateSpline(x, 100 * rng.standard_normal(x.size), s=x.size, ext='raise')
        si = interpolate.UnivariateSpline(x, 100 * rng.standard_normal(x.size), s=x.size, ext='raise')
        assert len(sr._eval_args[0]) > 2 * 3 + 2 + 10
        interp = NP.empty(1, dtype=[('real', object), ('imag', object)])
        interp[0] = (sr, si)
        q = NP.unique(NP.concatenate((_span_points(sr._eval_args[0], x.min(), x.max()), _span_points(si._eval_args[0], x.min(), x.max()))))
        pk = G.pack_splines(interp, NP.array([dim]))
        tab, _ = ctx.gains_eval_spline(pk, q if dim == 'time' else NP.zeros(1), NP.zeros(1) if dim == 'time' else q)
        got = tab.get()[:, 0, 0] if dim == 'time' else tab.get()[0, 0, :]
        tab.close()
        ref = interpolate.splev(q, sr._eval_args, ext=3) + 1j * interpolate.splev(q, si._eval_args, ext=3)
        assert NP.max(NP.abs(got - ref)) <= 1e-13 * NP.max(NP.abs(ref))


def test_apply_streams_over_snapshot_chunks_and_padding_rows_get_unity():
    """More snapshots than one 512 MiB chunk holds: the per-snapshot table rows follow each chunk; rows marked -1 get unity gains."""
    from prisim_amd import _abi
    rng = NP.random.default_rng(4)
    nt, nbl, nchan, nant = 9, 4096, 2048, 8                  # 128 MiB per snapshot: chunks of 4 snapshots
    ctx = G._device()
    g = rng.standard_normal((nant, nchan, nt)) + 1j * rng.standard_normal((nant, nchan, nt))
    tab, _ = ctx.gains_gather(g, NP.arange(nchan), NP.arange(nt))
    a, c = rng.integers(0, nant, nbl), rng.integers(0, nant, nbl)
    a[-3:] = -1
    sky = rng.standard_normal((nt, nbl, nchan)) + 1j * rng.standard_normal((nt, nbl, nchan))
    vis, _ = ctx.gains_apply(nt, nbl, nchan, fa=(tab, _abi.PRISIM_GAINS_ANTENNA, a, c), sky=sky)
    tab.close()
    gt = NP.transpose(g, (2, 0, 1))                          # [t][ant][f]
    want = NP.conj(gt[:, a[:-3], :]) * gt[:, c[:-3], :] * sky[:, :-3, :]
    assert NP.max(NP.abs(vis[:, :-3, :] - want)) <= 1e-13 * NP.max(NP.abs(want))
    assert NP.array_equal(vis[:, -3:, :], sky[:, -3:, :])
