"""The stand-in context of tests/cphase_standin.py with cphase_diff added, computed by tests/cpdiff_checker.py: for the CPU tests of
ClosurePhase.subsample_differencing.  It keeps every stack it hands out, so that a test can see them closed, and can be told to fail
at its n-th device call."""
import numpy as NP

import cpdiff_checker as DK
import cphase_standin as SI
from prisim_amd import _abi


class StandinContext(SI.StandinContext):
    def __init__(self, fail_at=None):
        SI.StandinContext.__init__(self)
        self.stacks = []
        self.fail_at = fail_at

    def _count(self):
        if self.fail_at is not None and len(self.calls) == self.fail_at:
            raise RuntimeError('stand-in failure')

    def cphase_bin(self, *args, **kwargs):
        self._count()
        out = SI.StandinContext.cphase_bin(self, *args, **kwargs)
        if 'stack' in out:
            self.stacks.append(out['stack'])
        return out

    def cphase_diff(self, pairs, stack=None, binned=None, budget_bytes=0):
        self._count()
        src = 'stack' if stack is not None else 'binned'
        if stack is not None:
            assert not stack.closed and stack.kind == _abi.PRISIM_CPBINS_BINNED
            binned = stack.arrays
        out = DK.diff_step(binned[0], binned[1], binned[2], pairs)
        self.calls.append({'diff': True, 'source': src, 'pairs': NP.asarray(pairs).copy()})
        out['stats'] = {'resident': stack is not None, 'ncomb': len(pairs)}
        return out
