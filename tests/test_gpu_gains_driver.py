"""GPU: the YAML driver with gains.file -- a one-rank run from a YAML file in tmp_path against the host statement gains * skyvis + noise,
and a two-rank run on one GPU (tests/dist_worker_gains.py) against world 1."""
import os
import subprocess
import sys

import numpy as NP
import pytest
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import dist_worker  # noqa: E402
import gains_checker as GC  # noqa: E402

from prisim_amd import driver, gains as G, hdf5io, workloads as W  # noqa: E402

pytestmark = pytest.mark.gpu


def write_gains_for(parms, path, seed=8):
    """antenna gains for every antenna of the run and a few baseline gains, over (a little more than) its channels and times"""
    rng = NP.random.default_rng(seed)
    bp = parms['bandpass']
    ch = W.channel_grid(float(bp['freq']), float(bp['freq_resolution']), int(bp['nchan']))
    jd = NP.asarray(driver.schedule(parms)[0], dtype=float)
    _, labels, _, _ = driver.baseline_info(parms)
    lab = G.bl_label_array(labels)
    ants = sorted(set(lab['A1']) | set(lab['A2']))
    f = NP.linspace(ch.min() - 1e3, ch.max() + 1e3, 12)
    span = max(jd.max() - jd.min(), 0.01)
    t = NP.linspace(jd.min() - 0.1 * span, jd.max() + 0.1 * span, 6)
    ga = (1.0 + 0.05 * NP.cos(NP.linspace(0, 4, f.size))[None, :, None] + 0.02 * NP.linspace(-1, 1, t.size)[None, None, :]) \
        * NP.exp(1j * rng.uniform(-1, 1, (len(ants), 1, 1)))
    bl = [tuple(x) for x in lab[::5].tolist()]
    gb = 1.0 + 0.1 * rng.standard_normal((len(bl), 1, 1)) + 0.05j * NP.sin(NP.linspace(0, 3, f.size))[None, :, None] \
        + 0.0 * t[None, None, :]
    with hdf5io.File(path, 'w') as fo:
        for key, g, labs in (('antenna-based', ga, NP.asarray(ants)), ('baseline-based', gb, GC.bl_struct(bl))):
            fo.write(key + '/gains', NP.ascontiguousarray(g))
            fo.write(key + '/ordering', NP.array(['label', 'frequency', 'time']))
            fo.write(key + '/label', labs)
            fo.write(key + '/frequency', f)
            fo.write(key + '/time', t)


def test_yaml_run_with_a_gains_file(tmp_path):
    gpath = str(tmp_path / 'gains.hdf5')
    over = {'array': {'layout': 'HERA-19', 'redundant': False}, 'telescope': {'id': 'custom', 'latitude': -30.7224},
            'antenna': {'shape': 'delta', 'size': 1.0}, 'bandpass': {'freq': 150e6, 'freq_resolution': 1e6, 'nchan': 16},
            'obsparm': {'n_acc': 3, 't_acc': 600.0, 'obs_mode': 'drift'},
            'pointing': {'lst_init': 1.0, 'drift_init': {'ha': 0.0, 'dec': -30.7224}},
            'skyparm': {'model': 'ptsrc_random', 'n_src': 40, 'seed': 7, 'custom_reffreq': 0.150, 'spindex': -0.8},
            'processing': {'add_noise': True, 'noise_seed': 5}, 'gains': {'file': gpath, 'filepathtype': 'custom'}}
    yml = tmp_path / 'run.yaml'
    yml.write_text(yaml.safe_dump(over))
    parms = driver.load_parms(str(yml))
    write_gains_for(parms, gpath)
    out = driver.run(parms, infile_dir=str(tmp_path), verbose=False)
    ia = out['ia']
    assert isinstance(ia.gaininfo, G.GainInfo)
    gains = ia.gaininfo.spline_gains(G.bl_label_array(out['labels']), freqs=out['freq'], times=out['timestamp'])
    want = gains * out['skyvis_freq'] + out['vis_noise_freq']
    scale = NP.abs(gains) * NP.abs(out['skyvis_freq']) + NP.abs(out['vis_noise_freq'])
    assert NP.max(NP.abs(out['vis_freq'] - want) / scale) <= 1e-13
    assert NP.max(NP.abs(out['vis_freq'] - out['skyvis_freq'] - out['vis_noise_freq'])) > 1e-3 * NP.max(NP.abs(out['vis_freq']))


def test_two_ranks_with_gains_on_one_gpu(tmp_path):
    gpath = str(tmp_path / 'gains.hdf5')
    write_gains_for(dist_worker.parms_for_test(), gpath)
    env = dict(os.environ, OMP_NUM_THREADS='2')
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'PRISIM_RDZV_FILE'):
        env.pop(k, None)
    cmd = [sys.executable, '-m', 'prisim_amd.launch', '-n', '2', os.path.join(ROOT, 'tests', 'dist_worker_gains.py'), gpath]
    res = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    out = res.stdout + res.stderr
    assert res.returncode == 0, out[-3000:]
    for r in range(2):
        assert 'RANK %d OK' % r in out, out[-3000:]
