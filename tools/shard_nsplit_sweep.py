"""Development helper: step time of the bench workload (world 1) and of rank 0's 1/N baseline shard of it against the source-split
count, queued as the benchmark queues its steps (no sync between them, so a folded grid's reduce / expand pass runs deferred under the
next sky-sum).  Candidates alternate, round by round, so that clock / temperature drift of the box cancels; 0 is the planner's own count
(csrc/split_plan.h), printed as it was realised.
    python tools/shard_nsplit_sweep.py [worlds, default 1,2,4,8] [candidates, default 0,4,5,6,7,8,9,10,12,16] [queued steps, 10] [rounds, 4]
One line per grid: median ms per step by candidate, with the spread (max - min over the rounds) behind it."""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as NP
from prisim_amd import _abi, workloads as W
from bench import shard_baselines
argv = sys.argv[1:]
worlds = [int(v) for v in (argv[0] if len(argv) > 0 else '1,2,4,8').split(',')]
cands = [int(v) for v in (argv[1] if len(argv) > 1 else '0,4,5,6,7,8,9,10,12,16').split(',')]
nq = int(argv[2]) if len(argv) > 2 else 10
rounds = int(argv[3]) if len(argv) > 3 else 4
cfg = W.config3(); bl, ch, sky = cfg['baselines'], cfg['channels'], cfg['sky']
zen = NP.array([0.0, 0.0, 1.0])
for world in worlds:
    mine = shard_baselines(bl, world, 0)[0] if world > 1 else bl
    ctx = _abi.Context(0)
    ctx.set_array(mine, ch, nt_max=1)
    ctx.set_sky_analytic(sky['dircos'], sky['flux_ref'], sky['spindex'], sky['ref_freq'], _abi.PRISIM_BEAM_AIRY, 14.0, zen, zen)
    acc = {c: [] for c in cands}
    real = {}
    for rnd in range(rounds + 1):                    # round 0 warms up (allocations of every candidate's partial cubes)
        for c in cands:
            ctx.set_tuning(0, 0, c)
            ctx.compute(precision=_abi.PRISIM_FP32)
            ctx.sync(); t0 = time.perf_counter()
            for _ in range(nq):
                ctx.compute(precision=_abi.PRISIM_FP32)
            ctx.sync()
            if rnd:
                acc[c].append((time.perf_counter() - t0) * 1e3 / nq)
            tm = ctx.timing()
            real[c] = (tm['last_nsplit'], tm['last_sum_baselines'])
    print('world=%d rows=%d summed=%d  ms per step (spread) by nsplit  ' % (world, mine.shape[0], real[cands[0]][1]) +
          '  '.join('%s:%.3f(%.3f)' % ('plan=%d' % real[c][0] if c == 0 else str(c), NP.median(acc[c]), max(acc[c]) - min(acc[c])) for c in cands), flush=True)
    ctx.close()
