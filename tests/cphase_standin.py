"""A stand-in for the device context of prisim_amd.bispectrum_phase.ClosurePhase on machines without a GPU: cphase_upload and
cphase_bin with the signatures of prisim_amd._abi.Context, computed by tests/cphase_bins_checker.py.  It records its calls, so that the
CPU tests can check what the host logic asks of the device (axes, bins, what stays resident, what is copied back)."""
import numpy as NP

import cphase_bins_checker as CK
from prisim_amd import _abi


class StandinStack(object):
    def __init__(self, kind, arrays):
        self.kind, self.arrays, self.shape, self.closed = kind, arrays, arrays[0].shape, False

    def close(self):
        self.closed = True


class StandinContext(object):
    def __init__(self):
        self.calls = []
        self.uploads = 0

    def cphase_upload(self, phases, flags):
        self.uploads += 1
        return StandinStack(_abi.PRISIM_CPBINS_PHASE_FLAGS, (NP.array(phases, dtype=NP.float64), NP.array(flags, dtype=bool)))

    def cphase_bin(self, axis, offsets, members, phases=None, flags=None, binned=None, stack=None, want=tuple(_abi.CPBINS_WANT),
                   mad_ignores_flags=False, keep=False, budget_bytes=0):
        src = 'stack' if stack is not None else ('binned' if binned is not None else 'host')
        if stack is not None:
            assert not stack.closed
            if stack.kind == _abi.PRISIM_CPBINS_BINNED:
                binned = stack.arrays
            else:
                phases, flags = stack.arrays
        if binned is not None:
            res = CK.binned_pass(binned[0], binned[1], binned[2], axis, offsets, members)
            kind = 'binned'
        else:
            res = CK.native_pass(phases, flags, axis, offsets, members, mad_ignores_flags)
            kind = 'native'
        self.calls.append({'axis': axis, 'source': src, 'kind': kind, 'want': tuple(want), 'keep': keep, 'mad_ignores_flags': mad_ignores_flags,
                           'offsets': NP.asarray(offsets).copy(), 'members': NP.asarray(members).copy()})
        out = {q: res[q] for q in want}
        if keep:
            out['stack'] = StandinStack(_abi.PRISIM_CPBINS_BINNED, (res['cp_mean'], res['cp_median'], res['wts']))
        out['stats'] = {'resident': stack is not None}
        return out
