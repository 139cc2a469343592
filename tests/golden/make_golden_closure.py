"""Regenerate tests/golden/golden_closure.npz from the reference's own triad and closure-phase statements.

At generation time this reads InterferometerArray.getThreePointCombinations (prisim/interferometry.py:6989-7085) and getClosurePhase
(:7087-7651) from a PRISim checkout and executes them under Python 3 on a stand-in ``self`` that holds the attributes they read
(layout, baselines, labels, bl_reversemap, channels, freq_resolution, the three cubes, bp, bp_wts), with the numpy aliases the
reference uses (NP.bool, NP.float_, NP.int) restored and a progress bar that does nothing.  getClosurePhase is executed without a
delay filter and without a spectral window: those branches call DSP / LKP, which are not in the reference tree.  No reference text is
stored: only inputs and outputs.

    python tests/golden/make_golden_closure.py /path/to/PRISim
"""
import os
import sys
import textwrap
import types
import warnings

import numpy as NP

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from prisim_amd import layouts as LAY  # noqa: E402


def _lines(path, a, b):
    with open(path) as fh:
        return ''.join(fh.readlines()[a - 1:b])


class _Bar(object):
    def __init__(self, *a, **k):
        pass

    def start(self):
        return self

    def update(self, *a):
        pass

    def finish(self):
        pass


def _load(ref_root):
    src = os.path.join(ref_root, 'prisim', 'interferometry.py')
    np_ns = types.SimpleNamespace(**{k: getattr(NP, k) for k in dir(NP) if not k.startswith('__')})
    np_ns.bool, np_ns.float_, np_ns.int = bool, NP.float64, int
    pgb = types.SimpleNamespace(ProgressBar=_Bar, Percentage=_Bar, Bar=_Bar, Counter=_Bar, ETA=_Bar)
    ns = {'NP': np_ns, 'warnings': warnings, 'PGB': pgb}
    exec(textwrap.dedent(_lines(src, 6989, 7085)), ns)
    exec(textwrap.dedent(_lines(src, 7087, 7651)), ns)
    return ns


def _array(pos, redundant):
    """Antenna labels '0'..'n-1', all pairs j > i folded and sorted (layout_baselines' construction); redundant=True keeps one
    baseline per distinct vector and maps every pair onto it (the array.redundant folding of the simulator's driver)."""
    bl, ids = LAY.baseline_generator(pos)
    bl, ids = LAY.fold_and_sort_baselines(bl, ids)
    labels = [(str(int(a)), str(int(b))) for a, b in NP.asarray(ids).reshape(-1, 2)]
    revmap = {lab: lab for lab in labels}
    if redundant:
        keys = ['{0[0]:.2f}_{0[1]:.2f}_{0[2]:.2f}'.format(v + 0.0) for v in bl]
        first = {}
        keep = []
        for i, k in enumerate(keys):
            if k not in first:
                first[k] = i
                keep.append(i)
        revmap = {labels[i]: labels[first[k]] for i, k in enumerate(keys)}
        bl, labels = bl[keep], [labels[i] for i in keep]
    return bl, labels, revmap


def _standin(ns, pos, bl, labels, revmap):
    s = types.SimpleNamespace()
    s.layout = {'positions': NP.array(pos, dtype=NP.float64), 'labels': NP.array([str(i) for i in range(len(pos))]),
                'ids': NP.arange(len(pos)), 'coords': 'ENU'}
    s.baselines = NP.array(bl, dtype=NP.float64)
    s.labels = NP.array(labels, dtype=[('A2', 'U8'), ('A1', 'U8')])
    s.bl_reversemap = revmap
    s.getThreePointCombinations = types.MethodType(ns['getThreePointCombinations'], s)
    s.getClosurePhase = types.MethodType(ns['getClosurePhase'], s)
    return s


def _triads(s, tag, out, counts):
    for unique in (False, True):
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter('always')
            ant, vec = s.getThreePointCombinations(unique=unique)
        key = '%s_%s' % (tag, 'unique' if unique else 'all')
        out[key + '_ant'] = NP.array(ant, dtype='U8').reshape(-1, 3)
        out[key + '_vec'] = NP.array(vec, dtype=NP.float64).reshape(-1, 3, 3)
        out[key + '_nwarn'] = NP.array(len(w))
        counts[key] = len(ant)


def main(ref_root):
    ns = _load(ref_root)
    out, counts = {}, {}
    hera = LAY.array_layout('HERA-19')
    for tag, red in (('hera19', False), ('hera19red', True)):
        bl, labels, revmap = _array(hera, red)
        s = _standin(ns, hera, bl, labels, revmap)
        out[tag + '_pos'], out[tag + '_bl'] = hera, bl
        out[tag + '_labels'] = NP.array(labels, dtype='U8')
        out[tag + '_rev_keys'] = NP.array(list(revmap.keys()), dtype='U8')
        out[tag + '_rev_vals'] = NP.array(list(revmap.values()), dtype='U8')
        _triads(s, tag, out, counts)
        if red:
            # getClosurePhase through a many-to-one bl_reversemap (every pair folded onto the one simulated baseline of its vector):
            # every 97th triad, a small seeded cube
            rng = NP.random.default_rng(20261017)
            shape = (len(labels), 6, 2)
            s.bl_reversemap = {k: s.labels[labels.index(v)] for k, v in revmap.items()}      # records, as below
            s.channels, s.freq_resolution = 150e6 + 1e5 * NP.arange(shape[1]), 1e5
            s.skyvis_freq = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
            s.vis_noise_freq = 0.3 * (rng.standard_normal(shape) + 1j * rng.standard_normal(shape))
            s.vis_freq = s.skyvis_freq + s.vis_noise_freq
            s.bp, s.bp_wts = 1.0 + 0.2 * rng.standard_normal(shape), rng.uniform(0.5, 1.5, shape)
            trip = [tuple(t) for t in out[tag + '_all_ant'][::97].tolist()]
            res = s.getClosurePhase(antenna_triplets=list(trip))
            out['redcp_triplets'] = NP.array(trip, dtype='U8')
            for name in ('skyvis_freq', 'vis_freq', 'vis_noise_freq', 'bp', 'bp_wts'):
                out['redcp_' + name] = getattr(s, name)
            for key in ('closure_phase_skyvis', 'closure_phase_vis', 'closure_phase_noise', 'skyvis', 'vis', 'noisevis'):
                out['redcp_out_' + key] = NP.asarray(res[key])
            out['redcp_out_baseline_triplets'] = NP.asarray(res['baseline_triplets'])
    # irregular layout: the pair (0, 4) has no simulated baseline
    pos = NP.array([[0.0, 0.0, 0.0], [14.6, 0.0, 0.0], [3.1, 17.2, 0.0], [-9.4, 6.3, 0.5], [21.7, -11.9, 0.0]])
    bl, labels, revmap = _array(pos, False)
    drop = labels.index(('4', '0'))
    bl = NP.delete(bl, drop, axis=0)
    labels = [lab for i, lab in enumerate(labels) if i != drop]
    revmap = {lab: lab for lab in labels}
    s = _standin(ns, pos, bl, labels, revmap)
    out['irr_pos'], out['irr_bl'], out['irr_labels'] = pos, bl, NP.array(labels, dtype='U8')
    _triads(s, 'irr', out, counts)

    # getClosurePhase, no filter, no window: seeded cubes, non-trivial bp and bp_wts, one flagged channel, all 8 conjugation patterns
    rng = NP.random.default_rng(20261016)
    nbl, nchan, nt = len(labels), 24, 5
    shape = (nbl, nchan, nt)
    s.channels = 150e6 + 1e5 * NP.arange(nchan)
    s.freq_resolution = 1e5
    s.skyvis_freq = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    s.vis_noise_freq = 0.3 * (rng.standard_normal(shape) + 1j * rng.standard_normal(shape))
    s.vis_freq = s.skyvis_freq + s.vis_noise_freq
    s.bp = 1.0 + 0.2 * rng.standard_normal(shape)
    s.bp[:, 7, :] = 0.0                                                  # a flagged channel
    s.bp_wts = rng.uniform(0.5, 1.5, shape)
    # the folded labels point either way, so the ordered triplets of the antennas cover every conjugation pattern: the first triplet
    # of each of the 8 patterns (by the rule of :7418-7473), then a few more
    import itertools
    # (folded baselines lie in one half-plane and never close a cycle, which the patterns (0, 0, 0) and (1, 1, 1) need: one baseline
    # of this case is entered the other way round, label and vector)
    lab2 = list(labels)
    flip = lab2.index(('1', '3'))
    lab2[flip] = ('3', '1')
    s.labels = NP.array(lab2, dtype=[('A2', 'U8'), ('A1', 'U8')])
    s.bl_reversemap = {lab: s.labels[i] for i, lab in enumerate(lab2)}     # records: numpy 2 compares a structured array with those only
    s.baselines = s.baselines.copy()
    s.baselines[flip] *= -1
    have = set(lab2)
    first = {}
    for trip in itertools.permutations([str(i) for i in range(len(pos))], 3):
        ids = ((trip[1], trip[0]), (trip[2], trip[1]), (trip[0], trip[2]))
        if any(i not in have and i[::-1] not in have for i in ids):
            continue
        first.setdefault(tuple(int(i not in have) for i in ids), trip)
    assert len(first) == 8, sorted(first)
    triplets = [first[k] for k in sorted(first)] + [('0', '1', '2'), ('3', '4', '1'), ('2', '4', '3'), ('1', '3', '0')]
    res = s.getClosurePhase(antenna_triplets=list(triplets))
    out['cp_labels'] = NP.array(lab2, dtype='U8')
    out['cp_baselines'] = s.baselines
    out['cp_triplets'] = NP.array(triplets, dtype='U8')
    for name in ('skyvis_freq', 'vis_freq', 'vis_noise_freq', 'bp', 'bp_wts', 'channels'):
        out['cp_' + name] = getattr(s, name)
    for key in ('closure_phase_skyvis', 'closure_phase_vis', 'closure_phase_noise', 'skyvis', 'vis', 'noisevis', 'spectral_weights'):
        out['cp_out_' + key] = NP.asarray(res[key])
    out['cp_out_baseline_triplets'] = NP.asarray(res['baseline_triplets'])
    NP.savez_compressed(os.path.join(HERE, 'golden_closure.npz'), **out)
    print('golden_closure.npz: triad counts', counts)
    print({k: v.shape for k, v in out.items() if k.startswith('cp_out')})


if __name__ == '__main__':
    main(sys.argv[1])
