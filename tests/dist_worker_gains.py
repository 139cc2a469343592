"""Worker for tests/test_gpu_gains_driver.py: one process per rank, started by prisim_amd.launch.  Two ranks on device 0 (the real HIP
context, the exchange through tests/fake_context.py's host stand-in, as tests/dist_worker.py's 'gpu' mode) run the YAML driver with a
gains file; the gathered vis_freq must equal the world-1 run's, and the padding rows of the last shard must not trip the table's
"antenna not found" fallback (no warning)."""
import os
import sys
import warnings

import numpy as NP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from prisim_amd import _abi, driver, rendezvous  # noqa: E402
import dist_worker  # noqa: E402
import fake_context  # noqa: E402


def main():
    gains_file = sys.argv[1]
    rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
    rdzv = rendezvous.Rendezvous(rank, world)
    uid = rdzv.broadcast_bytes(bytes(range(128)) if rank == 0 else b'')
    fake_context.RDZV = rdzv
    _abi.Context = fake_context.HostCommContext
    parms = driver.deep_merge(dist_worker.parms_for_test(), {'gains': {'file': gains_file, 'filepathtype': 'custom'},
                                                             'processing': {'add_noise': True, 'delay_transform': False}})
    with warnings.catch_warnings(record=True) as wl:
        warnings.simplefilter('always')
        out = driver.run(parms, rank=rank, world=world, device=0, comm_uid=uid, verbose=False)
    fell_back = any('neighbour logic failed' in str(w.message) for w in wl)
    ref = driver.run(parms, rank=0, world=1, device=0, verbose=False)
    scale = float(NP.max(NP.abs(ref['vis_freq'])))
    err = float(NP.max(NP.abs(out['vis_freq'] - ref['vis_freq'])))
    sky_err = float(NP.max(NP.abs(out['skyvis_freq'] - ref['skyvis_freq'])))
    # the gains did act: vis_freq is not skyvis + noise
    acted = float(NP.max(NP.abs(ref['vis_freq'] - ref['skyvis_freq'] - ref['vis_noise_freq']))) > 1e-3 * scale
    ok = (not fell_back) and acted and err <= 1e-11 * scale and sky_err <= 1e-11 * scale
    all_ok = all(rdzv.allgather(bool(ok)))
    rdzv.barrier()
    rdzv.close()
    if not all_ok:
        print('RANK %d MISMATCH err %g sky %g fell_back %s acted %s' % (rank, err, sky_err, fell_back, acted))
        sys.exit(1)
    print('RANK %d OK err_vis=%.2e' % (rank, err))


if __name__ == '__main__':
    main()
