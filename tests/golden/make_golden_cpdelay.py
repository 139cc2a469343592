"""Regenerate tests/golden/golden_cpdelay.npz from the reference's own closure-phase delay statements.

At generation time this reads the bodies of DelaySpectrum.subband_delay_transform_closure_phase (prisim/delay_spectrum.py:2850-2972),
DelayPowerSpectrum.compute_individual_closure_phase_power_spectrum (:4308-4348) and compute_averaged_closure_phase_power_spectrum
(:4488-4540) from a PRISim checkout and executes them under Python 3 on stand-in ``self`` objects with seeded inputs, with the stand-in
DSP / LKP modules of make_golden_subband.py (prisim_amd/dsp_readings.py; FT1D read as fftshift(ifft(.))).  The stand-in ``self`` of the
power spectra carries this package's k_parallel / k_perp / comoving_los_depth (the reference's call astropy).  For the cube case
``self.ia.getClosurePhase`` is the numpy checker of tests/closure_checker.py (itself pinned to the reference by golden_closure.npz) on the
golden closure case's cubes with channel 7 given a non-zero bandpass, so that no bispectrum is exactly zero.  No reference text is
stored: only inputs and outputs.

    python tests/golden/make_golden_cpdelay.py /path/to/PRISim
"""
import json
import os
import sys
import textwrap
import types

import numpy as NP
import scipy.constants as FCNST

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import closure_checker as CK  # noqa: E402
from make_golden_subband import _lines, _namespace  # noqa: E402
from prisim_amd import delay_spectrum as DS  # noqa: E402
from prisim_amd import interferometry as RI  # noqa: E402

KEYS = ('closure_phase_skyvis', 'closure_phase_vis', 'closure_phase_noise')


def _functions(ref_root):
    src = os.path.join(ref_root, 'prisim', 'delay_spectrum.py')
    ns = _namespace()
    ns['FCNST'] = FCNST
    ns['CNST'] = types.SimpleNamespace(rest_freq_HI=DS.REST_FREQ_HI)
    body = textwrap.indent(textwrap.dedent(_lines(src, 2850, 2972)), '    ')
    exec('def cpdelay(self, bw_eff, cpinfo, antenna_triplets, specsmooth_info, delay_filter_info, spectral_window_info, freq_center, '
         'shape, fftpow, pad, action, verbose):\n' + body, ns)
    for name, a, b in (('individual', 4308, 4348), ('averaged', 4488, 4540)):
        body = textwrap.indent(textwrap.dedent(_lines(src, a, b)), '    ')
        exec('def %s(self, closure_phase_delay_spectra):\n' % name + body, ns)
    return ns['cpdelay'], ns['individual'], ns['averaged']


def _dps_standin(f, nt):
    s = types.SimpleNamespace(cosmo=DS.cosmo100, wl0=FCNST.c / f[int(f.size / 2)], ds=types.SimpleNamespace(n_acc=nt))
    for name in ('k_parallel', 'k_perp', 'comoving_los_depth', 'comoving_transverse_distance'):
        setattr(s, name, types.MethodType(getattr(DS.DelayPowerSpectrum, name), s))
    return s


def _store(out, pre, d):
    for field, v in d.items():
        if isinstance(v, dict):
            _store(out, pre + field + '_', v)
        elif isinstance(v, (NP.ndarray, float, int, str)) and not isinstance(v, bool):
            out[pre + field] = NP.asarray(v)


def main(ref_root):
    cpdelay, individual, averaged = _functions(ref_root)
    rng = NP.random.default_rng(20261016)
    df = 97.65625e3
    out = {}
    # (nchan, leading shape of the phases, nt, window shape, pad, freq_center in channels, bw_eff in channels)
    specs = [
        (32, (3,), 2, 'rect', 1.0, [16.0], [8.0]),                       # M = 64, a power of two
        (33, (3, 2), 3, 'bhw', 0.5, [25.0, 6.0], [2.6, 3.4]),            # M = 49; two windows given out of channel order; a middle axis
        (40, (4,), 5, 'bhw', 0.6, [11.0], [4.0]),                        # a non-integer pad giving M = 64
    ]
    for i, (nchan, lead, nt, shape, pad, fc, bw) in enumerate(specs):
        f = 150e6 + df * NP.arange(nchan)
        ntrip = lead[0]
        cpinfo = {key: rng.uniform(-NP.pi, NP.pi, lead + (nchan, nt)) for key in KEYS}
        cpinfo['antenna_triplets'] = [(str(a), str(a + 1), str(a + 2)) for a in range(ntrip)]
        cpinfo['baseline_triplets'] = [rng.normal(size=(3, 3)) * 30.0 for _ in range(ntrip)]
        self = types.SimpleNamespace(f=f, df=df, ia=None)
        bw_eff, freq_center = NP.asarray(bw) * df, f[0] + NP.asarray(fc) * df
        pre = 'c%d_' % i
        out[pre + 'params'] = NP.array(json.dumps({'nchan': nchan, 'lead': list(lead), 'nt': nt, 'df': df, 'shape': shape, 'pad': pad,
                                                   'bw_eff': bw_eff.tolist(), 'freq_center': freq_center.tolist()}))
        for key in KEYS:
            out[pre + 'in_' + key] = cpinfo[key]
        out[pre + 'in_baseline_triplets'] = NP.asarray(cpinfo['baseline_triplets'])
        for tag, action in (('o', 'return_oversampled'), ('r', 'return_resampled')):
            d = cpdelay(self, bw_eff.copy(), cpinfo, None, None, None, None, freq_center.copy(), shape, 1.0, pad, action, False)
            out[pre + tag + '_keys'] = NP.array(sorted(d.keys()))
            _store(out, pre + tag + '_', {k: v for k, v in d.items() if k not in ('antenna_triplets', 'baseline_triplets')})
            if tag == 'r' and len(lead) == 1:
                _store(out, pre + 'pi_', individual(_dps_standin(f, nt), d))
            if tag == 'r':
                _store(out, pre + 'pa_', averaged(_dps_standin(f, nt), d))

    # the cube path: the golden closure case without its flagged channel
    G = NP.load(os.path.join(HERE, 'golden_closure.npz'))
    labels = [tuple(x) for x in G['cp_labels'].tolist()]
    trip = [tuple(t) for t in G['cp_triplets'].tolist()]
    s = types.SimpleNamespace(labels=labels, baselines=G['cp_baselines'], bl_reversemap=None)
    legs, conj, vec = RI.InterferometerArray.closure_leg_table(s, trip)
    bp = G['cp_bp'].copy()
    bp[:, 7, :] = 0.8
    f = G['cp_channels']
    nchan = f.size
    df = float(f[1] - f[0])
    cubes = {'skyvis': G['cp_skyvis_freq'], 'vis': G['cp_vis_freq'], 'noise': G['cp_vis_noise_freq']}
    nt = cubes['skyvis'].shape[2]

    def get_closure_phase(antenna_triplets=None, specsmooth_info=None, delay_filter_info=None, spectral_window_info=None):
        info = {'antenna_triplets': trip, 'baseline_triplets': vec}
        for name, cube in cubes.items():
            t, ph = CK.closure_phase(cube, legs, conj, bp, G['cp_bp_wts'])
            assert not NP.any(NP.prod(t, axis=1) == 0), 'a bispectrum of the cube case is exactly zero'
            info['closure_phase_' + name] = ph
        return info

    self = types.SimpleNamespace(f=f, df=df, ia=types.SimpleNamespace(getClosurePhase=get_closure_phase))
    fc, bw, shape, pad = [nchan * 0.5 + 0.2, 5.0], [nchan / 4.0], 'bhw', 1.0
    bw_eff, freq_center = NP.asarray(bw) * df, f[0] + NP.asarray(fc) * df
    out['cube_params'] = NP.array(json.dumps({'nchan': int(nchan), 'nt': int(nt), 'df': df, 'shape': shape, 'pad': pad,
                                              'bw_eff': bw_eff.tolist(), 'freq_center': freq_center.tolist()}))
    out['cube_bp'] = bp
    for tag, action in (('o', 'return_oversampled'), ('r', None)):
        d = cpdelay(self, bw_eff.copy(), None, trip, None, None, None, freq_center.copy(), shape, 1.0, pad, action, False)
        out['cube_' + tag + '_keys'] = NP.array(sorted(d.keys()))
        _store(out, 'cube_' + tag + '_', {k: v for k, v in d.items() if k not in ('antenna_triplets', 'baseline_triplets')})
    NP.savez_compressed(os.path.join(HERE, 'golden_cpdelay.npz'), **out)
    print('golden_cpdelay.npz: %d bytes, %d arrays' % (os.path.getsize(os.path.join(HERE, 'golden_cpdelay.npz')), len(out)))


if __name__ == '__main__':
    main(sys.argv[1])
