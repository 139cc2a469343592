"""Regenerate tests/golden/golden_gains.npz from the reference's own gain-table statements.

At generation time this reads read_gaintable (prisim/interferometry.py:333-631), extract_gains (:635-853) and GainInfo's splinator
(:3107-3166), spline_gains (:3382-3595) and nearest_gains (:3599-3721), and InterferometerArray.add_noise (:6697-6722) from a PRISim
checkout and executes them under Python 3 on a stand-in ``self``: NMO.find_list_in_list and LKP.find_1NN are the readings of
prisim_amd/dsp_readings.py, h5py is a small ``.value`` shim over prisim_amd/hdf5io.py (prisim_amd/gains.py:H5File), ``xrange`` and the
numpy aliases the reference uses (NP.bool, NP.complex, NP.object) are restored.  No reference text is stored: only inputs and
outputs, and the class name of the exception where a statement raises.

    python tests/golden/make_golden_gains.py /path/to/PRISim
"""
import copy
import json
import os
import sys
import tempfile
import textwrap
import types
import warnings

import numpy as NP

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from prisim_amd import dsp_readings as R  # noqa: E402
from prisim_amd import gains as G  # noqa: E402
from prisim_amd import hdf5io  # noqa: E402


def _lines(path, a, b):
    with open(path) as fh:
        return ''.join(fh.readlines()[a - 1:b])


def _namespace():
    from scipy import interpolate
    np_ns = types.SimpleNamespace(**{k: getattr(NP, k) for k in dir(NP) if not k.startswith('__')})
    np_ns.bool, np_ns.complex, np_ns.object, np_ns.int, np_ns.float = bool, complex, object, int, float
    h5py = types.SimpleNamespace(File=lambda path, mode='r': G.H5File(path))
    return {'NP': np_ns, 'NMO': types.SimpleNamespace(find_list_in_list=R.find_list_in_list),
            'LKP': types.SimpleNamespace(find_1NN=R.find_1NN), 'h5py': h5py, 'interpolate': interpolate, 'xrange': range,
            'warnings': warnings, 'copy': copy}


def _load(ref_root):
    src = os.path.join(ref_root, 'prisim', 'interferometry.py')
    ns = _namespace()
    exec(_lines(src, 333, 631), ns)
    exec(_lines(src, 635, 853), ns)
    for a, b in ((3107, 3166), (3382, 3595), (3599, 3721), (6697, 6722)):
        exec(textwrap.dedent(_lines(src, a, b)), ns)
    return ns


class _Info(object):
    """stand-in GainInfo: the reference's methods bound to a plain object"""

    def __init__(self, ns, path, axes_order=None):
        self.gaintable = ns['read_gaintable'](path, axes_order=axes_order)
        self.splinefuncs = {key: None for key in ['antenna-based', 'baseline-based']}
        self.splinator = types.MethodType(ns['splinator'], self)
        self.spline_gains = types.MethodType(ns['spline_gains'], self)
        self.nearest_gains = types.MethodType(ns['nearest_gains'], self)
        self.splinator(smoothness=None)


def _gain(rng, shape, amp=0.2):
    return (1.0 + amp * rng.standard_normal(shape)) * NP.exp(1j * amp * rng.standard_normal(shape))


def _smooth(rng, nl, f, t):
    """gains smooth in frequency and time (ripple + drift), one row per label"""
    fr = (f - f.mean()) / (f.max() - f.min() + 1e-30)
    tr = (t - t.mean()) / (t.max() - t.min() + 1e-30)
    a = 1.0 + 0.1 * rng.standard_normal((nl, 1, 1))
    return a * (1.0 + 0.05 * NP.cos(6.0 * fr[None, :, None] + rng.uniform(0, 6, (nl, 1, 1))) + 0.03 * tr[None, None, :]) \
        * NP.exp(1j * (0.3 * fr[None, :, None] * rng.standard_normal((nl, 1, 1)) + 0.2 * tr[None, None, :] + rng.uniform(-1, 1, (nl, 1, 1))))


def _write(path, groups):
    with hdf5io.File(path, 'w') as fo:
        for key, g in groups.items():
            order = g['ordering']
            perm = [['label', 'frequency', 'time'].index(ax) for ax in order]
            fo.write(key + '/gains', NP.ascontiguousarray(NP.transpose(g['gains'], perm)))
            fo.write(key + '/ordering', NP.asarray(order))
            for sub in ('label', 'frequency', 'time'):
                fo.write(key + '/' + sub, NP.asarray(g[sub]))


def _bl_dtype(n=8):
    return [('A2', 'U%d' % n), ('A1', 'U%d' % n)]


def main(ref_root):
    ns = _load(ref_root)
    rng = NP.random.default_rng(20261016)
    f = NP.linspace(150e6, 160e6, 14)
    jd = 2459000.25 + NP.arange(9) * 0.004
    toff = jd - jd[0]
    ants = [str(i) for i in range(6)]
    bls_tab = NP.asarray([('1', '0'), ('2', '0'), ('3', '1'), ('4', '2'), ('5', '3')], dtype=_bl_dtype())
    # queried baselines (A2, A1): direct labels, a reversed one ('0','2' is the reverse of ('2','0')) and one absent from the table
    query = NP.asarray([('1', '0'), ('0', '2'), ('3', '1'), ('5', '4'), ('4', '2')], dtype=_bl_dtype())
    qf = NP.concatenate((f[1:-1:3], 0.5 * (f[2:5] + f[3:6])))
    qt = NP.concatenate((jd[::2], jd[1:3] + 0.001))
    mk = lambda shape: _smooth(rng, *shape)   # noqa: E731
    cases = {
        # name: (groups {key: (labels, ordering, (nf, nt) varying, times-as)}, query freqs, query times, add_noise timestamps)
        'ant2d': ({'antenna-based': (ants, ['time', 'label', 'frequency'], 'ft', jd)}, qf, qt, jd),
        'bl2d': ({'baseline-based': (bls_tab, ['frequency', 'time', 'label'], 'ft', jd)}, qf, qt, jd),
        'both2d': ({'antenna-based': (ants, ['label', 'frequency', 'time'], 'ft', jd),
                    'baseline-based': (bls_tab, ['label', 'time', 'frequency'], 'ft', jd)}, qf, qt, jd),
        'ant_freq': ({'antenna-based': (ants, ['label', 'frequency', 'time'], 'f', jd)}, qf, qt[:1], jd[:1]),
        'ant_time': ({'antenna-based': (ants, ['frequency', 'label', 'time'], 't', jd)}, qf[:1], qt, jd),
        'both_blfreq': ({'antenna-based': (ants, ['label', 'frequency', 'time'], 'ft', jd),
                         'baseline-based': (bls_tab, ['label', 'frequency', 'time'], 'f', jd)}, qf, qt[:1], jd[:1]),
        'const': ({'antenna-based': (ants, ['label', 'frequency', 'time'], '', jd)}, qf, qt, jd),
        'retry_offset': ({'antenna-based': (ants, ['label', 'frequency', 'time'], 'ft', toff)}, qf, qt - jd[0], jd),
        'fall_nearest': ({'antenna-based': (ants, ['label', 'frequency', 'time'], 'ft', jd[2:6])}, qf, qt, jd),
        'missing_ant': ({'antenna-based': (ants[:5], ['label', 'frequency', 'time'], 'ft', jd)}, qf, qt, jd),
    }
    out = {'cases': []}
    arrays = {}
    tmp = tempfile.mkdtemp()
    for name, (groups, cf, ct, stamps) in cases.items():
        spec = {}
        for key, (labels, order, vary, times) in groups.items():
            nl = len(labels)
            nf = f.size if 'f' in vary else 1
            nt = times.size if 't' in vary else 1
            g = mk((nl, f[:nf] if nf > 1 else f[:1], times[:nt] if nt > 1 else times[:1]))
            spec[key] = {'gains': g, 'ordering': order, 'label': labels, 'frequency': f[:nf], 'time': times[:nt]}
        path = os.path.join(tmp, name + '.hdf5')
        _write(path, spec)
        for key, g in spec.items():
            k = key.split('-')[0]
            arrays['%s/%s/gains' % (name, k)] = g['gains']
            arrays['%s/%s/frequency' % (name, k)] = g['frequency']
            arrays['%s/%s/time' % (name, k)] = g['time']
            arrays['%s/%s/label' % (name, k)] = NP.asarray([tuple(x) for x in g['label']] if key == 'baseline-based' else g['label'])
        rec = {'name': name, 'orderings': {k: v['ordering'] for k, v in spec.items()}, 'results': {}}
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            info = _Info(ns, path, axes_order=['label', 'frequency', 'time'])
            calls = {
                'spline': lambda: info.spline_gains(query, freqs=cf, times=ct),
                'spline_ordered': lambda: info.spline_gains(query, freqs=cf, times=ct, axes_order=['label', 'frequency', 'time']),
                'nearest': lambda: info.nearest_gains(query, freqs=cf, times=ct),
                'eval': lambda: ns['extract_gains'](info.gaintable, query),
            }
            for cname, fn in calls.items():
                try:
                    arrays['%s/%s' % (name, cname)] = NP.asarray(fn())
                    rec['results'][cname] = 'ok'
                except Exception as exc:      # the reference raises here: the class name is the fixture
                    rec['results'][cname] = type(exc).__name__
            # add_noise on a stand-in array: sky (nbl, nchan, nt) at the queried channels and timestamps
            nbl = query.size
            sky = _gain(rng, (nbl, cf.size, stamps.size), 1.0) * 3.0
            noise = 0.1 * (rng.standard_normal(sky.shape) + 1j * rng.standard_normal(sky.shape))
            arr = types.SimpleNamespace(gaininfo=info, labels=query, channels=cf, timestamp=list(stamps), skyvis_freq=sky,
                                        vis_noise_freq=noise)
            with warnings.catch_warnings(record=True) as wl:
                warnings.simplefilter('always')
                try:
                    ns['add_noise'](arr)
                    arrays['%s/add_noise' % name] = arr.vis_freq
                    rec['results']['add_noise'] = 'ok'
                except Exception as exc:
                    rec['results']['add_noise'] = type(exc).__name__
            rec['add_noise_warned'] = any('neighbour logic failed' in str(w.message) for w in wl)
            arrays['%s/sky' % name] = sky
            arrays['%s/noise' % name] = noise
            arrays['%s/stamps' % name] = NP.asarray(stamps)
            arrays['%s/qf' % name] = cf
            arrays['%s/qt' % name] = ct
        out['cases'].append(rec)
    arrays['query'] = NP.asarray([tuple(x) for x in query])
    arrays['meta'] = NP.asarray(json.dumps(out))
    dst = os.path.join(HERE, 'golden_gains.npz')
    NP.savez_compressed(dst, **arrays)
    print(dst, os.path.getsize(dst), 'bytes')
    for rec in out['cases']:
        print(rec['name'], rec['results'], 'warned' if rec['add_noise_warned'] else '')


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get('PRISIM_REF', '../PRISim'))
