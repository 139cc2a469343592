"""numpy statement of include/prisim_cpft.h: the delay spectra of stacks of complex numbers (n0, n1, n2, nchan) under flag weights
divided by their mean over the channels, frequency windows and a visibility scale, oversampled and FFT-resampled, and the lag kernel --
the transforms of prisim/bispectrum_phase.py:ClosurePhaseDelaySpectrum.FT (:2719-2757, :2770-2779).  The checker of prisim_cphase_ft
and of prisim_amd.bispectrum_phase.ClosurePhaseDelaySpectrum; tests/test_cpft.py pins it to tests/golden/golden_cpft.npz, the
reference's own statements executed (tests/golden/make_golden_cpft.py).

Where the reference divides 0 by 0 (a row whose weights average to 0) the checker, like the device, gives 0.
"""
import json
import os

import numpy as NP
import numpy.ma as MA

from prisim_amd import dsp_readings as DSP

BOUND = 1e-12          # the package's bound for its two FFT routes (tests/test_gpu_cpdelay.py), relative to df sum |x|
MAX_ZERO_SHARE = 0.10  # rows of zero mean weight (non-finite in the reference) among the rows compared, at most


def flag_weights(weights):
    """fw = w / mean over the channels of w; 0 for the whole row where the mean is 0"""
    w = NP.asarray(weights, dtype=NP.float64)
    mu = NP.mean(w, axis=-1, keepdims=True)
    with NP.errstate(divide='ignore', invalid='ignore'):
        return NP.where(mu == 0.0, 0.0, w / mu)


def padded(inp, wts, m, weights=None, vscale=None, lead=None):
    """x (nwin, n0, n1, n2, m): inp * fw * wts * vscale, zero-padded; inp None: the lag kernel's fw * wts.  A real factor of exactly 0
    gives 0 whatever the input holds.  lead: the full (n0, n1, n2) where neither the weights nor the input show it."""
    wts = NP.asarray(wts, dtype=NP.float64)
    nwin, nchan = wts.shape
    fac = wts[:, None, None, None, :]
    if weights is not None:
        fac = flag_weights(weights)[None] * fac
    if inp is None:
        x = fac.astype(NP.complex128)
    else:
        inp = NP.asarray(inp, dtype=NP.complex128)
        if lead is None:
            lead = NP.asarray(weights).shape[:3] if weights is not None else inp.shape[:3]
        if vscale is not None:
            fac = fac * NP.asarray(vscale, dtype=NP.float64)[:, :, None, None, None]
        fac = NP.broadcast_to(fac, (nwin,) + tuple(lead) + (nchan,))
        with NP.errstate(invalid='ignore'):
            x = NP.where(fac == 0.0, 0.0, NP.broadcast_to(inp, tuple(lead) + (nchan,))[None] * fac)
    return NP.pad(x, [(0, 0)] * 4 + [(0, m - nchan)], mode='constant')


def transform(inputs, wts, m, df, weights=None, vscale=None, nres=None):
    """The outputs of prisim_cphase_ft: 'over' and 'res' (lists, one array per input; 'res' None without nres), 'lag_kernel',
    'lag_kernel_res', and 'xsum' / 'lag_xsum': sum over the channels of |x| per (window, row), what spectrum_error scales by."""
    out = {'over': [], 'res': None if nres is None else [], 'xsum': []}

    def one(x):
        over = NP.fft.fftshift(NP.fft.ifft(x, axis=-1), axes=-1) * m * df
        return over, (None if nres is None else DSP.resample(over, nres, axis=-1))

    lead = NP.shape(weights)[:3] if weights is not None else (NP.broadcast_shapes(*[NP.shape(i)[:3] for i in inputs]) if len(inputs) else None)
    for inp in inputs:
        x = padded(inp, wts, m, weights, vscale, lead)
        over, res = one(x)
        out['over'].append(over)
        if nres is not None:
            out['res'].append(res)
        out['xsum'].append(NP.sum(NP.abs(x), axis=-1))
    x = padded(None, wts, m, weights)
    out['lag_kernel'], out['lag_kernel_res'] = one(x)
    out['lag_xsum'] = NP.sum(NP.abs(x), axis=-1)
    return out


def spectrum_error(got, want, x_abs_sum, df):
    """The largest |got - want| of a (window, row), relative to df * sum over the channels of |x| of that window and row -- the
    largest value its spectrum can take (a row's own maximum would reward rows that cancel).  A row with x = 0 must agree exactly."""
    got, want = NP.asarray(got), NP.asarray(want)
    assert got.shape == want.shape and got.shape[:-1] == NP.shape(x_abs_sum), (got.shape, want.shape, NP.shape(x_abs_sum))
    dev = NP.max(NP.abs(got - want), axis=-1)
    scale = df * NP.asarray(x_abs_sum)
    if NP.any((scale == 0.0) & ~(dev == 0.0)) or not NP.all(NP.isfinite(dev)):
        return NP.inf
    ok = scale > 0.0
    return float(NP.max(dev[ok] / scale[ok])) if NP.any(ok) else 0.0


# ---- the fixture ------------------------------------------------------------------------------------------------------------------

_GOLD = {}
POOLS = (('whole', 'mean'), ('whole', 'median'), ('submodel', None), ('residual', 'mean'), ('residual', 'median'),
         ('errinfo', 'dspec0', 'mean'), ('errinfo', 'dspec0', 'median'), ('errinfo', 'dspec1', 'mean'), ('errinfo', 'dspec1', 'median'))


def gold():
    if not _GOLD:
        _GOLD['npz'] = NP.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'golden_cpft.npz'))
    return _GOLD['npz']


def cases():
    """[{'name', 'nchan', 'pad', 'shape', 'bw_eff', 'freq_center', 'apply_flags', 'resample', 'model', 'vis_ones', ...}, ...]"""
    return json.loads(str(gold()['cases']))


def case(name):
    return [c for c in cases() if c['name'] == name][0]


def _masked(key):
    g = gold()
    return MA.array(g[key], mask=g[key + '__mask']) if key + '__mask' in g.files else g[key]


def raw(name):
    return {k: gold()['%s_in_%s' % (name, k)] for k in ('cphase', 'flags', 'lst', 'days')}


def freqs(name):
    return gold()[name + '_f']


def visscaleinfo(name):
    return {'vis': gold()[name + '_vis'].copy(), 'lst': gold()[name + '_vis_lst'].copy()}


def cpinfo(name):
    """(processed, errinfo) of a case: what the reference's smooth_in_tbins, subtract and subsample_differencing left, with this
    package's values under the masks, as masked arrays"""
    g, pre = gold(), name + '_cp_'
    prelim = {'wts': _masked(pre + 'prelim_wts'), 'lstbins': g[pre + 'prelim_lstbins'],
              'eicp': {s: _masked(pre + 'prelim_eicp_' + s) for s in ('mean', 'median')}}
    proc = {'prelim': prelim}
    if pre + 'submodel_eicp' in g.files:
        proc['submodel'] = {'eicp': _masked(pre + 'submodel_eicp')}
        proc['residual'] = {'eicp': {s: _masked(pre + 'residual_eicp_' + s) for s in ('mean', 'median')}}
    err = {'wts': {q: _masked(pre + 'errinfo_wts_' + q) for q in ('0', '1')},
           'eicp_diff': {q: {s: _masked(pre + 'errinfo_eicp_diff_%s_%s' % (q, s)) for s in ('mean', 'median')} for q in ('0', '1')}}
    return proc, err


def pool(result, name):
    """the spectra of POOLS entry `name` in a result dictionary of FT, or None"""
    d = result.get(name[0], {})
    if name[0] == 'errinfo':
        return d[name[1]].get(name[2])
    if name[0] == 'submodel':
        return d.get('dspec')
    return d.get('dspec', {}).get(name[1])


def gold_result(name, tag):
    """the reference's result dictionary of a case: tag 'o' oversampled (cPhaseDS), 'r' resampled (None where the case did not resample)"""
    g, pre = gold(), '%s_%s_' % (name, tag)
    if pre + 'lags' not in g.files:
        return None
    res = {k: g[pre + k] for k in ('freq_center', 'freq_wts', 'bw_eff', 'lags', 'lag_corr_length', 'lag_kernel')}
    res['shape'], res['fftpow'], res['npad'] = str(g[pre + 'shape']), float(g[pre + 'fftpow']), int(g[pre + 'npad'])
    res.update({'whole': {'dspec': {}}, 'residual': {'dspec': {}}, 'submodel': {}, 'errinfo': {'dspec0': {}, 'dspec1': {}}})
    for p in POOLS:
        key = pre + '_'.join(x for x in p if x)
        if key in g.files:
            if p[0] == 'errinfo':
                res['errinfo'][p[1]][p[2]] = g[key]
            elif p[0] == 'submodel':
                res['submodel']['dspec'] = g[key]
            else:
                res[p[0]]['dspec'][p[1]] = g[key]
    return res


def ft_inputs(name, proc=None, err=None):
    """The three device calls of FT on a case: [(label, weights, [(pool name, stack)])], stacks with this package's values under the
    masks, from the fixture's cpinfo or from (proc, err)."""
    if proc is None:
        proc, err = cpinfo(name)

    def data(x, fill):
        x = MA.array(x)
        d = NP.where(MA.getmaskarray(x), fill, MA.getdata(x)).astype(NP.complex128)
        return d.reshape((1,) * (4 - d.ndim) + d.shape)

    pre = proc['prelim']
    stacks = [(('whole', s), data(pre['eicp'][s], 1.0)) for s in ('mean', 'median')]
    if 'submodel' in proc:
        stacks.append((('submodel', None), data(proc['submodel']['eicp'], 0.0)))
        stacks += [(('residual', s), data(proc['residual']['eicp'][s], 0.0)) for s in ('mean', 'median')]
    calls = [('prelim', MA.getdata(pre['wts']), stacks)]
    for q in ('0', '1'):
        calls.append(('errinfo' + q, MA.getdata(err['wts'][q]),
                      [(('errinfo', 'dspec' + q, s), data(err['eicp_diff'][q][s], 0.0)) for s in ('mean', 'median')]))
    return calls


def vis_scale(vis, freq_wts, nlst):
    """visscale (nwin, nlst) of :2716-2717 from one reference LST's visibilities (3, 1, nchan)"""
    v = NP.asarray(vis)[:, 0, :]
    avg = NP.sum(v[None, :, :] * freq_wts[:, None, :], axis=-1) / NP.sum(freq_wts, axis=-1)[:, None]      # nwin x 3
    return NP.repeat(NP.sqrt(1.0 / NP.sum(1.0 / NP.abs(avg) ** 2, axis=-1))[:, None], nlst, axis=1)


# ---- a case of the fixture through an implementation of cphase_ft -----------------------------------------------------------------

def setup(name):
    """what FT derives from a case's arguments: f, df, bw_eff, freq_center, wts, m, npad, factor, nres"""
    from prisim_amd.delay_spectrum import subband_freq_wts
    c, f = case(name), freqs(name)
    df = f[1] - f[0]
    bw, fc = NP.asarray(c['bw_eff']) * df, f[0] + NP.asarray(c['freq_center']) * df
    npad = int(f.size * c['pad'])
    m = f.size + npad
    factor = NP.min(m * df / bw)
    return {'f': f, 'df': df, 'bw_eff': bw, 'freq_center': fc, 'wts': subband_freq_wts(f, df, bw, fc, c['shape'], 1.0), 'm': m, 'npad': npad,
            'factor': factor, 'nres': DSP.fft_downsample_length(m, factor)}


class CheckerContext(object):
    """cphase_ft of prisim_amd._abi.Context computed by this module: the stand-in context of the CPU tests"""

    def __init__(self):
        self.calls = 0

    def cphase_ft(self, inputs, wts, m, df, weights=None, vscale=None, nres=None, want=('over', 'res', 'lag_kernel'), route='auto',
                  budget_bytes=0, shape=None):
        self.calls += 1
        t = transform(inputs, wts, m, df, weights=weights, vscale=vscale, nres=nres if 'res' in want else None)
        return {'over': t['over'] if 'over' in want else None, 'res': t['res'] if 'res' in want else None,
                'lag_kernel': t['lag_kernel'] if 'lag_kernel' in want else None,
                'lag_kernel_res': t['lag_kernel_res'] if 'lag_kernel' in want and 'res' in want else None, 'stats': {}}


def entry_results(ctx, name, vscale='case', **kw):
    """{'o': ..., 'r': ...}: the spectra and the lag kernel of a case's result dictionaries from three calls of ctx.cphase_ft on the
    fixture's cpinfo, one per weight set; and the list of the calls' stats"""
    c, S = case(name), setup(name)
    vs = None
    if vscale == 'case':
        vs = vis_scale(gold()[name + '_vis'], S['wts'], NP.asarray(gold()[name + '_cp_prelim_lstbins']).size)
    res = {t: {'whole': {'dspec': {}}, 'residual': {'dspec': {}}, 'submodel': {}, 'errinfo': {'dspec0': {}, 'dspec1': {}}}
           for t in (('o', 'r') if c['resample'] else ('o',))}

    def put(r, p, v):
        if p[0] == 'errinfo':
            r['errinfo'][p[1]][p[2]] = v
        elif p[0] == 'submodel':
            r['submodel']['dspec'] = v
        else:
            r[p[0]]['dspec'][p[1]] = v

    stats = []
    for label, w, stacks in ft_inputs(name):
        lagk = label == 'prelim'
        want = ('over',) + (('res',) if c['resample'] else ()) + (('lag_kernel',) if lagk else ())
        out = ctx.cphase_ft([s for _, s in stacks], S['wts'], S['m'], S['df'], weights=w if c['apply_flags'] else None, vscale=vs,
                            nres=S['nres'] if c['resample'] else None, want=want, shape=w.shape[:3], **kw)
        stats.append(out['stats'])
        for i, (p, _) in enumerate(stacks):
            put(res['o'], p, out['over'][i])
            if c['resample']:
                put(res['r'], p, out['res'][i])
        if lagk:
            res['o']['lag_kernel'] = out['lag_kernel']
            if c['resample']:
                res['r']['lag_kernel'] = DSP.downsampler(out['lag_kernel'], S['factor'], axis=-1, method='interp', kind='linear')
    return res, stats


def compare_spectra(got, name, tag, label='', scale=1.0, verbose=True):
    """Every spectrum and the lag kernel of `got` (a result dictionary of FT, or of entry_results) against the fixture's reference
    result `tag` ('o' / 'r') times `scale`: spectrum_error <= BOUND, relative to df sum |x| with x from this checker.  Rows that are
    non-finite in the reference (zero mean weight) are compared with 0, exactly; they may be MAX_ZERO_SHARE of the rows at most.
    Returns the largest error."""
    c, S, ref = case(name), setup(name), gold_result(name, tag)
    vs = vis_scale(gold()[name + '_vis'], S['wts'], NP.asarray(gold()[name + '_cp_prelim_lstbins']).size)
    worst, nbad, nrows = 0.0, 0, 0
    items = []
    for _, w, stacks in ft_inputs(name):
        wt = w if c['apply_flags'] else None
        for p, stack in stacks:
            items.append((p, pool(got, p), pool(ref, p), NP.sum(NP.abs(padded(stack, S['wts'], S['m'], wt, vs)), axis=-1)))
    prelim_w = ft_inputs(name)[0][1] if c['apply_flags'] else None
    items.append(('lag_kernel', got['lag_kernel'], ref['lag_kernel'] / scale, NP.sum(NP.abs(padded(None, S['wts'], S['m'], prelim_w)), axis=-1)))
    for p, g, r, xsum in items:
        assert g is not None and r is not None, (label, name, tag, p)
        assert g.shape == r.shape and g.dtype == r.dtype == NP.complex128, (label, name, tag, p, g.shape, r.shape)
        bad = ~NP.all(NP.isfinite(r), axis=-1)
        assert NP.all(g[bad] == 0), (label, name, tag, p, 'rows of zero mean weight must be exactly 0')
        e = spectrum_error(g, NP.where(bad[..., None], 0.0, r * scale), NP.abs(scale) * xsum, S['df'])
        if verbose:
            print('%s %s %s %s: error %.3e of df sum |x| (%d of %d rows of zero mean weight)' % (label, name, tag, p, e, bad.sum(), bad.size))
        assert e <= BOUND, (label, name, tag, p, e)
        worst = max(worst, e)
        if p != 'lag_kernel':
            nbad += int(bad.sum())
            nrows += bad.size
    assert nbad <= MAX_ZERO_SHARE * nrows, (label, name, tag, nbad, nrows)
    return worst
