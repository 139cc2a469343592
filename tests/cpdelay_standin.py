"""Stand-ins for the host logic of the closure-phase delay spectra (pattern of tests/subband_standin.py): a context whose
closure_delay_spectra / closure_power compute the device entries' contracts in numpy (tests/cpdelay_checker.py), a DelaySpectrum over a
stand-in array built from the golden closure case, and a DelayPowerSpectrum without a device."""
import os
import types

import numpy as NP
import scipy.constants as FCNST

import cpdelay_checker as CC
from prisim_amd import delay_spectrum as DS, interferometry as RI

GOLD_CLOSURE = NP.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'golden_closure.npz'))


def phases_of(cube, legs, conj, bpwts, freq_wts, masks=None, mask_index=None):
    """prisim_closure_phase's phases in numpy: cube (nbl, nchan, nt) -> (ntriads, nchan, nt)"""
    v = NP.asarray(cube)[legs]                                               # (T, 3, nchan, nt)
    v = NP.where(NP.asarray(conj, dtype=bool)[:, :, None, None], v.conj(), v)
    v = NP.asarray(freq_wts, dtype=NP.float64).reshape(1, 1, -1, 1) * v
    if masks is not None:
        mk = masks[mask_index[legs]] if mask_index is not None else NP.broadcast_to(masks[0], legs.shape + (masks.shape[1],))
        v = NP.fft.ifft(mk[..., None] * NP.fft.fft(v, axis=2), axis=2)
    v = v * NP.asarray(bpwts)[legs]
    return NP.angle((v[:, 0] * v[:, 1]) * v[:, 2])


class StandinContext(object):
    """closure_delay_spectra / closure_power with the device calls' contracts, restated in numpy; ``calls`` records (entry, form, want)."""

    def __init__(self):
        self.calls = []
        self.phases = []

    def closure_delay_spectra(self, wts, m, df, phases=None, cube=None, legs=None, conj=None, bpwts=None, freq_wts=None, masks=None,
                              mask_index=None, nt=None, nres=0, want=('res',), **kw):
        self.calls.append(('spectra', 'phases' if phases is not None else 'cube', tuple(want)))
        wts = NP.asarray(wts)
        if phases is None:
            if cube is None:
                raise AssertionError('the stand-in has no resident cube')
            nchan = wts.shape[-1]
            fw = NP.ones(nchan) if freq_wts is None else NP.broadcast_to(NP.asarray(freq_wts, dtype=NP.float64).ravel(), (nchan,))
            phases = phases_of(cube, NP.asarray(legs), conj, NP.broadcast_to(bpwts, NP.shape(cube)), fw, masks, mask_index)
        self.phases.append(phases)
        over, res = CC.delay_spectra(phases, wts, m, df, nres if 'res' in want else None)
        out = {'stats': {'route': 'standin', 'rows': int(NP.prod(NP.shape(phases)[:-2]))}}
        if 'over' in want:
            out['over'] = over
        if 'res' in want:
            out['res'] = res
        return out

    def closure_power(self, spectra, scale, want=('individual',), **kw):
        self.calls.append(('power', None, tuple(want)))
        out = {'stats': {}}
        if 'individual' in want:
            out['individual'] = CC.power_individual(spectra, scale)
        if 'auto' in want or 'cross' in want:
            out['auto'], out['cross'] = CC.power_averaged(spectra, scale)
        return out


def make_ds(bp=None, noise=True, ctx=None):
    """A DelaySpectrum over a stand-in array holding the golden closure case's cubes (9 baselines, 24 channels, 5 snapshots)."""
    G = GOLD_CLOSURE
    labels = [tuple(x) for x in G['cp_labels'].tolist()]
    f = G['cp_channels']
    nt = G['cp_skyvis_freq'].shape[2]
    bl = G['cp_baselines']
    ia = types.SimpleNamespace(labels=labels, baselines=bl, bl_reversemap=None, channels=f, freq_resolution=float(f[1] - f[0]), n_acc=nt,
                               baseline_lengths=NP.sqrt(NP.sum(bl ** 2, axis=1)), skyvis_freq=G['cp_skyvis_freq'],
                               vis_freq=G['cp_vis_freq'] if noise else None, vis_noise_freq=G['cp_vis_noise_freq'] if noise else None,
                               bp=G['cp_bp'] if bp is None else bp, bp_wts=G['cp_bp_wts'], _cube=[None] * nt, _device_in_step=False,
                               _reserved=0, _ctx=ctx if ctx is not None else StandinContext())
    for name in ('getThreePointCombinations', 'closure_leg_table'):
        setattr(ia, name, types.MethodType(getattr(RI.InterferometerArray, name), ia))
    ds = DS.DelaySpectrum.__new__(DS.DelaySpectrum)
    ds.ia, ds.f, ds.df, ds.n_acc = ia, f, ia.freq_resolution, nt
    return ds


def gold_triplets():
    return [tuple(t) for t in GOLD_CLOSURE['cp_triplets'].tolist()]


def make_dps(f, nt, ctx=None):
    """A DelayPowerSpectrum with the attributes the closure-phase power spectra read"""
    dps = DS.DelayPowerSpectrum.__new__(DS.DelayPowerSpectrum)
    dps.cosmo = DS.cosmo100
    dps.wl0 = FCNST.c / f[int(f.size / 2)]
    dps.ds = types.SimpleNamespace(n_acc=nt, ia=types.SimpleNamespace(_ctx=ctx if ctx is not None else StandinContext()))
    return dps
