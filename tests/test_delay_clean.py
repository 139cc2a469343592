"""CPU: delay CLEAN.  The numpy checker (tests/clean_checker.py) against the reference's fixtures (tests/golden/golden_clean.npz);
DelaySpectrum.delayClean's host logic and complex1dClean's surface through a stand-in context whose CLEAN entries are the checker; the
argument checks; DelayPowerSpectrum's cc keys; and the C-ABI of prisim_amd/csrc_clean (guards, header, binding, library exports)."""
import os
import re

import numpy as NP
import pytest

import clean_checker as CK
import fake_context
from prisim_amd import _abi, delay_spectrum as DS, skymodel as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'golden_clean.npz')


class CleanOracleContext(fake_context.OracleContext):
    """The oracle seam plus the two CLEAN entries of include/prisim_clean.h, computed by the checker."""

    def clean_rows(self, inp, kern, cbox, gain, maxiter, threshold, absolute=False, kidx=None):
        inp = NP.asarray(inp, dtype=NP.complex128)
        if inp.shape[1] > _abi.PRISIM_CLEAN_MAX_LEN:
            raise ValueError('delay CLEAN takes rows of 1 to 4096 lags')
        cc, res, iters, flags, rms = CK.clean_rows(inp, kern, cbox, gain, maxiter, threshold, absolute, kidx)
        return cc, res, iters, flags, rms, {'rows': inp.shape[0], 'sum_iter': int(iters.sum()), 'device_ms': 0.0, 'clean_ms': 0.0}

    def clean_delay(self, win, kwin, cbox, m, lag_scale, freq_scale1, freq_scale2, gain, maxiter, threshold, absolute=False, kidx=None):
        win = NP.asarray(win, dtype=NP.complex128)
        ncubes, nrows, nchan = win.shape

        def to_lag(x):
            xp = NP.zeros(x.shape[:-1] + (m,), dtype=NP.complex128)
            xp[..., :nchan] = x
            return NP.fft.ifft(xp, axis=-1) * m * lag_scale

        out = {'lag': to_lag(win), 'kern_lag': to_lag(NP.asarray(kwin, dtype=NP.complex128))}
        for name in ('cc', 'res', 'cc_freq', 'res_freq'):
            out[name] = NP.empty_like(out['lag'])
        out['iters'] = NP.empty((ncubes, nrows), NP.int32)
        out['flags'] = NP.empty((ncubes, nrows), NP.int32)
        out['rms'] = NP.empty((ncubes, nrows, 2))
        for c in range(ncubes):
            cc, res, it, fl, rms = CK.clean_rows(out['lag'][c], out['kern_lag'], cbox, gain, maxiter, threshold, absolute, kidx)
            out['cc'][c], out['res'][c], out['iters'][c], out['flags'][c], out['rms'][c] = cc, res, it, fl, rms
            out['cc_freq'][c] = NP.fft.fft(cc, axis=1) * freq_scale1 * freq_scale2
            out['res_freq'][c] = NP.fft.fft(res, axis=1) * freq_scale1 * freq_scale2
        out['stats'] = {'rows': ncubes * nrows, 'sum_iter': int(out['iters'].sum()), 'device_ms': 0.0, 'clean_ms': 0.0}
        return out


def test_checker_reproduces_the_reference_fixtures():
    g = NP.load(GOLD)
    n = int(g['n'])
    stops = NP.zeros(3, dtype=int)
    for i in range(n):
        gain, maxiter, thr, absolute = g['params_%d' % i]
        inp = g['inp_%d' % i]
        o = CK.clean_row(inp, g['kernel_%d' % i], g['cbox_%d' % i], gain, int(maxiter), thr, 'absolute' if absolute else 'relative')
        assert o['iter'] == int(g['iter_%d' % i]), i
        assert [o['cond1'], o['cond2'], o['cond3']] == list(g['cond_%d' % i]), i
        scale = max(NP.abs(inp).max(), 1e-300)
        assert NP.max(NP.abs(o['cc'] - g['cc_%d' % i])) <= 1e-13 * scale, i
        assert NP.max(NP.abs(o['res'] - g['res_%d' % i])) <= 1e-13 * scale, i
        assert NP.array_equal([o['inrms'], o['outrms']], g['rms_%d' % i], equal_nan=True), i
        stops += NP.asarray(g['cond_%d' % i], dtype=int)
    assert stops.min() > 0                                  # every termination condition occurs
    ms = {g['inp_%d' % i].size for i in range(n)}
    assert any(m % 2 for m in ms) and any(m % 2 == 0 for m in ms)
    assert not NP.any(g['inp_%d' % (n - 1)])                # the all-zero row


def test_checker_reproduces_the_reference_box_and_post_processing():
    g = NP.load(GOLD)
    nchan, pad, df = int(g['dc_nchan']), float(g['dc_pad']), float(g['dc_df'])
    npad = int(nchan * pad)
    m = nchan + npad
    lags = NP.fft.fftfreq(m, df)
    assert NP.array_equal(lags, g['dc_lags']) and NP.array_equal(NP.fft.fftshift(lags), g['dc_cc_lags'])
    hdl, boxes = g['dc_hdl'], g['dc_boxes']
    deta, pf = lags[1] - lags[0], 1.0 + 1.0 * npad / nchan
    for name in ('skyvis', 'vis'):
        lag_in = g['dc_%s_lag_in' % name]
        nbl, _, nt = lag_in.shape
        assert NP.array_equal(g['dc_%s_lag' % name], NP.fft.fftshift(lag_in, axes=1))
        for b in range(nbl):
            for t in range(nt):
                box = CK.clean_box(lags, hdl[t, b], 1.0, df * nchan)
                assert NP.array_equal(box, boxes[t, b] > 0)
                o = CK.clean_row(lag_in[b, :, t], g['dc_kernel'], box)
                for key, want in (('lag', NP.fft.fftshift(o['cc'])), ('res_lag', NP.fft.fftshift(o['res'])),
                                  ('freq', NP.fft.fft(o['cc']) * deta * pf), ('res_freq', NP.fft.fft(o['res']) * deta * pf)):
                    ref = g['dc_cc_%s_%s' % (name, key)]
                    assert NP.max(NP.abs(ref[b, :, t] - want)) <= 1e-13 * NP.max(NP.abs(ref)), (name, key, b, t)
        assert NP.array_equal(g['dc_cc_%s_net_lag' % name], g['dc_cc_%s_lag' % name] + g['dc_cc_%s_res_lag' % name])


def _array(monkeypatch, bl_order=None, noise=True, nbl=6, nchan=24, nt=3, seed=3):
    from prisim_amd import interferometry as RI
    monkeypatch.setattr(_abi, 'Context', CleanOracleContext)
    rng = NP.random.default_rng(seed)
    ch = 150e6 + 3e5 * (NP.arange(nchan) - nchan // 2)
    bl = rng.uniform(-60.0, 60.0, size=(nbl, 3)) * NP.array([1.0, 1.0, 0.02])
    labels = ['b%d' % i for i in range(nbl)]
    if bl_order is not None:
        bl, labels = bl[bl_order], [labels[i] for i in bl_order]
    alt, az = rng.uniform(20.0, 89.0, 40), rng.uniform(0.0, 360.0, 40)
    skymod = SM.SkyModel(location=NP.stack((alt, az), axis=1), flux_ref=rng.uniform(0.5, 5.0, 40), spindex=rng.uniform(-1.0, 0.0, 40),
                         ref_freq=150e6)
    ia = RI.InterferometerArray(labels, bl, ch, telescope={'id': 'hera'}, latitude=-30.7, skycoords='altaz', pointing_coords='hadec')
    bpass = 0.5 + 0.5 * NP.hanning(nchan + 2)[1:-1]
    for j in range(nt):
        ia.observe((2457000.5 + j, 10.0 + 3 * j), {'Tnet': 300.0}, bpass, [0.0, -30.7], skymod, 10.0)
    if noise:
        ia.generate_noise(seed=5)
        ia.add_noise()
    return ia


_CC = ('cc_lag_kernel', 'cc_skyvis_lag', 'cc_skyvis_res_lag', 'cc_vis_lag', 'cc_vis_res_lag', 'cc_skyvis_net_lag', 'cc_vis_net_lag',
       'cc_skyvis_freq', 'cc_skyvis_res_freq', 'cc_vis_freq', 'cc_vis_res_freq', 'cc_skyvis_net_freq', 'cc_vis_net_freq')


@pytest.mark.parametrize('pad,window', [(1.0, None), (0.5, 'blackman'), (0.0, 'per-snapshot')])
def test_delay_clean_host_logic_on_the_seam(monkeypatch, pad, window):
    ia = _array(monkeypatch)
    nbl, nchan, nt = ia.baselines.shape[0], ia.channels.size, ia.n_acc
    fw = None if window is None else (NP.blackman(nchan) + 0.05 if window == 'blackman' else
                                      NP.outer(NP.blackman(nchan) + 0.05, NP.linspace(1.0, 1.4, nt)))
    ds = DS.DelaySpectrum(ia)
    assert ds.horizon_delay_limits.shape[0] == nt
    if window == 'per-snapshot':
        ds.horizon_delay_limits = ds.horizon_delay_limits[1:2]          # departure 4: one row of limits serves every snapshot
    ds.delayClean(pad=pad, freq_wts=fw, gain=0.1, verbose=False)
    bp = NP.asarray(ia.bp)
    w = NP.ones_like(bp) if fw is None else (NP.broadcast_to(fw.reshape(1, -1, 1), bp.shape) if fw.ndim == 1 else
                                             NP.broadcast_to(fw[None], bp.shape))
    want = CK.delay_clean(NP.asarray(ia.skyvis_freq), NP.asarray(ia.vis_freq), bp, w, ds.horizon_delay_limits, ia.channels, ds.df, pad=pad)
    m = nchan + int(nchan * pad)
    assert NP.array_equal(ds.lags, want['lags']) and NP.array_equal(ds.cc_lags, want['cc_lags'])
    for name in ('skyvis_lag', 'vis_lag', 'lag_kernel') + _CC:
        got = getattr(ds, name)
        assert got.shape == (nbl, m, nt), name
        assert NP.max(NP.abs(got - want[name])) <= 1e-12 * NP.max(NP.abs(want[name])), name
    assert NP.array_equal(ds._clean_iters[0], want['iters']['skyvis']) and NP.array_equal(ds._clean_iters[1], want['iters']['vis'])
    if fw is not None:
        assert NP.array_equal(NP.asarray(ds.bp_wts), w)
    assert ds.clean_window_buffer == 1.0


def test_permuting_baselines_permutes_the_outputs(monkeypatch):
    """One box per (baseline, snapshot): the serial branch's box, never reset, would give each row the union of all earlier rows'
    boxes and make the result depend on row order."""
    order = NP.array([5, 2, 0, 4, 1, 3])
    ds_a = DS.DelaySpectrum(_array(monkeypatch, noise=False))
    ds_b = DS.DelaySpectrum(_array(monkeypatch, bl_order=order, noise=False))
    for ds in (ds_a, ds_b):
        ds.delayClean(pad=1.0, verbose=False)
    for name in ('cc_skyvis_lag', 'cc_skyvis_res_lag', 'cc_skyvis_freq'):
        a, b = getattr(ds_a, name), getattr(ds_b, name)
        assert NP.max(NP.abs(a[order] - b)) <= 1e-12 * NP.max(NP.abs(a)), name
    # the boxes do differ between baselines: the union box would have changed the later rows
    bw = ds_a.df * ds_a.f.size
    boxes = [CK.clean_box(ds_a.lags, ds_a.horizon_delay_limits[0, b], 1.0, bw) for b in range(6)]
    assert len({bx.tobytes() for bx in boxes}) > 1
    # departure 3: no noisy cube -> no cc_vis_*, vis_lag None
    assert ds_a.vis_lag is None and all(getattr(ds_a, n) is None for n in _CC if n.startswith('cc_vis'))
    assert ds_a.cc_skyvis_lag is not None


def test_failed_calls_change_no_attributes(monkeypatch):
    ia = _array(monkeypatch)
    ds = DS.DelaySpectrum(ia)
    before = dict(vars(ds))
    bad = [({'threshold_type': 'rel'}, ValueError, 'invalid specification for threshold_type'),
           ({'threshold': 'x'}, TypeError, 'input threshold must be a scalar'),
           ({'threshold': -1.0}, ValueError, 'input threshold must be positive'),
           ({'threshold': 1.0}, ValueError, 'incompatible value specified for threshold'),
           ({'threshold': 1e9, 'threshold_type': 'absolute'}, ValueError, 'incompatible value specified for threshold'),
           ({'gain': 1}, TypeError, 'gain must be a floating point number'),
           ({'gain': 1.5}, TypeError, 'gain must lie between 0 and 1'),
           ({'maxiter': 10.0}, TypeError, 'maxiter must be an integer'),
           ({'maxiter': 0}, ValueError, 'maxiter must be positive'),
           ({'pad': '1'}, TypeError, 'pad fraction must be a scalar value.'),
           ({'freq_wts': NP.ones(5)}, ValueError, 'window shape dimensions')]
    for kw, exc, msg in bad:
        with pytest.raises(exc, match=re.escape(msg)):
            ds.delayClean(verbose=False, freq_wts=kw.pop('freq_wts', None), **kw)
        after = vars(ds)
        assert after.keys() == before.keys()
        for k, v in before.items():
            assert after[k] is v, (kw, k)


def test_power_spectrum_gains_the_cc_keys_only_after_delay_clean(monkeypatch):
    ia = _array(monkeypatch)
    ds = DS.DelaySpectrum(ia)
    ds.delay_transform(pad=1.0, action='store', verbose=False)
    dps = DS.DelayPowerSpectrum(ds)
    dps.compute_power_spectrum()
    assert not any(k.startswith('cc_') for k in dps.dps)
    ds.delayClean(pad=1.0, verbose=False)
    dps = DS.DelayPowerSpectrum(ds)
    assert dps.cc_lags is ds.cc_lags
    dps.compute_power_spectrum()
    factor = dps.jacobian1 * dps.jacobian2 * dps.Jy2K ** 2
    for key in ('cc_skyvis', 'cc_vis', 'cc_skyvis_res', 'cc_vis_res', 'cc_skyvis_net', 'cc_vis_net'):
        assert NP.array_equal(dps.dps[key], NP.abs(getattr(ds, key + '_lag')) ** 2 * factor), key


def test_complex1dclean_surface_and_departures(monkeypatch):
    monkeypatch.setattr(_abi, 'Context', CleanOracleContext)
    g = NP.load(GOLD)
    inp, kern, box = g['inp_0'], g['kernel_0'], g['cbox_0']
    o = DS.complex1dClean(inp, kern, cbox=box, gain=0.1, maxiter=10000, threshold=5e-3)
    assert o['iter'] == int(g['iter_0']) and o['rms'] is None
    assert [o['termination'][k] for k in ('threshold', 'maxiter', 'inrms<outrms')] == list(g['cond_0'])
    assert NP.max(NP.abs(o['cc'] - g['cc_0'])) <= 1e-13 * NP.abs(inp).max()
    assert o['inrms'] == g['rms_0'][0] and o['outrms'] == g['rms_0'][1]
    # rows (extension): one call, per-row results equal to the 1-D calls
    rows = NP.stack([g['inp_%d' % i] for i in range(4)])
    r = DS.complex1dClean(rows, kern, cbox=box, gain=0.1, threshold=5e-3)
    for i in range(4):
        one = DS.complex1dClean(rows[i], kern, cbox=box, gain=0.1, threshold=5e-3)
        assert r['iter'][i] == one['iter'] and NP.array_equal(r['cc'][i], one['cc'])
    # departure 2: <= 2 entries outside the box: cond3 False and outrms None (the reference raises UnboundLocalError)
    full = NP.ones(inp.size)
    full[:2] = 0
    o = DS.complex1dClean(inp, kern, cbox=full, gain=0.5, maxiter=50)
    assert o['outrms'] is None and o['termination']['inrms<outrms'] is False and o['inrms'] == o['inrms']
    # argument checks, in the reference's order and words
    for kw, exc, msg in (({'inp': list(inp)}, TypeError, 'inp must be a numpy array'),
                         ({'kernel': 3}, TypeError, 'kernel must be a numpy array'),
                         ({'threshold_type': 'abs'}, ValueError, 'invalid specification for threshold_type'),
                         ({'threshold': 0.0}, ValueError, 'input threshold must be positive'),
                         ({'kernel': kern[:-1]}, ValueError, 'inp and kernel must have same size'),
                         ({'cbox': box[:-1]}, ValueError, 'Clean box must be of same size as input'),
                         ({'cbox': [1, 0]}, TypeError, 'cbox must be a numpy array'),
                         ({'threshold': 1e9, 'threshold_type': 'absolute', 'gain': 2}, ValueError, 'incompatible value specified'),
                         ({'gain': 1}, TypeError, 'gain must be a floating point number'),
                         ({'gain': 0.0}, TypeError, 'gain must lie between 0 and 1'),
                         ({'maxiter': 5.0}, TypeError, 'maxiter must be an integer'),
                         ({'maxiter': -1}, ValueError, 'maxiter must be positive')):
        args = {'inp': inp, 'kernel': kern}
        args.update(kw)
        with pytest.raises(exc, match=re.escape(msg)):
            DS.complex1dClean(args.pop('inp'), args.pop('kernel'), **args)


def test_complex1dclean_has_no_cpu_fallback(monkeypatch, tmp_path):
    monkeypatch.setattr(_abi, '_lib', None)
    monkeypatch.setattr(_abi, 'LIB_PATH', str(tmp_path / 'missing.so'))
    g = NP.load(GOLD)
    with pytest.raises(_abi.PrisimHipError):
        DS.complex1dClean(g['inp_0'], g['kernel_0'], cbox=g['cbox_0'])


def test_clean_entries_are_guarded_and_header_binding_library_agree():
    src_dir = os.path.join(ROOT, 'prisim_amd', 'csrc_clean')
    src = ''.join(open(os.path.join(src_dir, f)).read() for f in sorted(os.listdir(src_dir)))
    entries = re.findall(r'^int (prisim_clean_\w+)\(', src, flags=re.M)
    assert sorted(entries) == sorted(_abi.CLEAN_EXPORTS)
    for name in entries:
        body = src[src.index('int %s(' % name):]
        assert 'return guarded(' in body[:body.index('{') + 200], name
    hdr = open(os.path.join(ROOT, 'include', 'prisim_clean.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    assert sorted(set(re.findall(r'\b(prisim_clean_\w+)\s*\(', hdr))) == sorted(_abi.CLEAN_EXPORTS)
    assert not set(_abi.CLEAN_EXPORTS) & set(_abi.EXPORTS)
    lib = _abi.load_library()
    for name in _abi.CLEAN_EXPORTS:
        assert hasattr(lib, name)
    assert re.search(r'#define PRISIM_CLEAN_MAX_LEN (\d+)', open(os.path.join(ROOT, 'include', 'prisim_clean.h')).read()).group(1) == \
        str(_abi.PRISIM_CLEAN_MAX_LEN)
    # no argument checks reach the device with a null context
    assert lib.prisim_clean_rows(None, 0, 8, None, 1, None, None, None, 0.1, 10, 5e-3, 0, None, None, None, None, None, None) == \
        _abi.PRISIM_EINVAL
