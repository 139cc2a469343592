"""Host-side mirror of the reference's ``InterferometerArray`` for the sky-sum path.

Same class / method / keyword names, argument meaning and exception types as
prisim/interferometry.py of nithyanandan/PRISim (constructor :5140-5145, 5665-5870; observe
:5874-6410; observing_run :6414-6657; delay_transform :8052-8137) so that a PRISim user can switch
to ``prisim_amd.interferometry.InterferometerArray`` for this path.  Everything numerical on the
path -- tau, the source-shape taper, the DFT sum, the baseline gradient, pb*flux, the analytic
beams in scope, the delay transform -- runs in HIP kernels behind include/prisim_hip.h.  There is
NO CPU fallback: without libprisim_hip.so or a GPU the constructor raises ``PrisimHipError``.

Differences kept on purpose:
  Q1  ``timeobj`` may be an astropy-``Time``-like object (``.jd``, ``.sidereal_time('apparent').deg``),
      or a ``(jd, lst_deg)`` tuple, or a float jd with the ``lst`` keyword; astropy is not required.
  Q2  ``observing_run`` works (the reference's passes a str as timeobj and cannot run).
  Q4  baseline gradients work for shapeless sky models too.
  Q5  ``memsave`` reduces the phase in fp64 before the fp32 recurrence (more accurate than the reference's
      all-fp32 phase); results are complex64 like the reference's.  On arrays of at most 256 baselines observed from the resident
      catalogue the arithmetic of a ``memsave`` snapshot is fp64 (the batched launch of include/prisim_hip.h serves it: faster than any
      fp32 launch chain at that size); the stored type stays complex64.
  Q7  the visibility cube is grown without O(nt^2) recopy; same logical shape (nbl, nchan, n_acc).
  Q20 delay_transform transforms whichever of the three cubes exist.
  sky coordinates 'radec': the reference's astropy chain FK5(skymodel.epoch) -> FK5(obstime) -> AltAz (:6174-6180) is ONE rotation and
      ONE aberration vector per snapshot, applied on the device (prisim_snapshot.cel2enu / aberr_beta).  Without astropy they come from
      prisim_amd/frames.py: IAU 2006 precession + truncated IAU 1980 nutation + annual aberration + rotation by the apparent LST
      (``frame_model = 'apparent'``, the default; 'mean' = precession only; 'date' = none, HA = LST - RA).  Not modelled: frame bias,
      light deflection, diurnal aberration, polar motion (< 1 arcsec together; parity with astropy unpinned).  A caller with astropy sets
      ``frame_provider`` and reproduces the reference's frame exactly.
Out of scope here: gain tables, FITS persistence, uvfits / uvh5.
"""
import contextlib
import os
import warnings
import weakref

import numpy as NP

from . import _abi
from . import baseline_delay_horizon as DLY
from . import frames as FRAMES
from . import geometry as GEOM
from .gains import GainInfo, extract_gains, read_gaintable  # noqa: F401  (the reference's names in prisim.interferometry)
from . import primary_beams as PB

C_LIGHT = 299792458.0
SIDEREAL_RATE = 1.00273790935    # sidereal seconds per solar second
_CATALOG_OOM = 'device memory exhausted on the resident-catalogue path; this sky model continues on the per-snapshot upload path'


class _DeviceSlot(object):
    """Placeholder in InterferometerArray._cube for a snapshot that so far lives only in slot `slot` of the device cube (after
    reserve()); the host copy is fetched the first time skyvis_freq is read.  Runs that gather on the device never fetch it."""
    __slots__ = ('slot', 'dtype', 'staged')

    def __init__(self, slot, dtype, staged=False):
        self.slot, self.dtype = slot, NP.dtype(dtype)
        self.staged = staged           # an asynchronous download into the pinned host cube is in flight or done (reserve(host_staging=True))


class _ResidentLags(object):
    """Delay spectra of slots [0, nt) that one delay_transform_device call left in the context's single resident buffer, fetched when
    read (config 5: 120 GB that a sharded run exchanges GPU -> GPU instead).  Any later transform on that context (another window or pad,
    the other class's delay_transform, a power-spectrum fetch) overwrites the buffer: the transform is then simply run again
    (milliseconds) before the read -- a stored result never changes, as in the reference, whose store is a host copy."""
    __slots__ = ('ctx', 'nt', 'nout', 'window', 'pad', 'lags', 'generation')

    def __init__(self, ctx, nt, window, pad):
        self.ctx, self.nt, self.window, self.pad = ctx, nt, NP.array(window, dtype=NP.float64), pad
        self.lags, self.nout = ctx.delay_transform_device(nt, bpwts=self.window, pad=pad, want_lag=True)
        self.generation = getattr(ctx, '_dt_generation', None)

    def _refresh(self):
        if getattr(self.ctx, '_dt_generation', None) != self.generation:
            self.ctx.delay_transform_device(self.nt, bpwts=self.window, pad=self.pad, want_lag=True)
            self.generation = getattr(self.ctx, '_dt_generation', None)

    def spectra(self, rows=None):
        """(nbl | len(rows), nout, nt) lag spectra."""
        self._refresh()
        lags = self.ctx.get_lags(0, self.nt) if rows is None else self.ctx.get_lags(0, self.nt, rows=rows)
        return NP.transpose(lags, (1, 2, 0))

    def power(self, power_scale):
        """(nbl, nout, nt) abs(spectra)**2 * power_scale: the same spectra transformed again, with their power beside them."""
        self.ctx.delay_transform_device(self.nt, bpwts=self.window, pad=self.pad, want_lag=True, want_power=True, power_scale=power_scale)
        self.generation = getattr(self.ctx, '_dt_generation', None)
        return NP.transpose(self.ctx.get_delay_power(0, self.nt), (1, 2, 0))

    def allgather(self, nranks, download=True):
        """RCCL all-gather of the spectra, GPU -> GPU; the gathered [t][rank][b][lag] | [t][bl][lag] cube, or None with download=False."""
        self._refresh()
        self.ctx.allgather_lags(self.nt)
        return self.ctx.get_gathered(self.nt, nranks, row=self.nout) if download else None


@contextlib.contextmanager
def _through_slot0(ctx, keep):
    """Host-side transforms run through device slot 0; with keep (the slot holds a resident snapshot) it is saved and put back."""
    saved = ctx.get_vis(slot=0) if keep else None
    try:
        yield
    finally:
        if saved is not None:
            ctx.set_vis(saved, slot=0)


def _all_same(layers):
    """Whether every (1 | nbl, nchan) layer of a list equals the first, in shape and values."""
    return all(l.shape == layers[0].shape and NP.array_equal(l, layers[0]) for l in layers[1:])


def _distinct_layers(layers, nbl):
    """The distinct (1 | nbl, nchan) layers of a list concatenated along the rows (complex128), and each (layer, baseline)'s row index
    into them, (len(layers), nbl) int64."""
    distinct, idx = [], NP.empty((len(layers), nbl), dtype=NP.int64)
    for t, l in enumerate(layers):
        hit = next((i for i, d in enumerate(distinct) if d.shape == l.shape and NP.array_equal(d, l)), None)
        if hit is None:
            hit = len(distinct)
            distinct.append(l)
        base = sum(d.shape[0] for d in distinct[:hit])
        idx[t] = base + (NP.arange(nbl) if l.shape[0] == nbl else 0)
    return NP.concatenate(distinct, axis=0).astype(NP.complex128), idx


class _LayerStack(object):
    """The per-snapshot layers of a (nbl, nchan, n_acc) attribute (bp, bp_wts, Tsys) in the broadcastable form they were given in
    -- (1 | nbl, 1 | nchan) -- instead of the dense arrays the reference grows by NP.dstack at every observe()
    (interferometry.py:6019-6024, 6082-6086: 0.5 GB per snapshot and attribute at HERA-350 x 1024 channels, O(n_acc^2) copies).
    The dense array with the reference's shape is formed when the attribute is read."""

    def __init__(self, nbl, nchan, initial):
        self.nbl, self.nchan = nbl, nchan
        self.initial = NP.asarray(initial, dtype=NP.float64)         # value before the first snapshot, broadcastable to (nbl, nchan)
        self.layers = []

    def append(self, layer):
        layer = NP.asarray(layer, dtype=NP.float64)
        if layer.ndim == 3:
            layer = layer[:, :, 0]
        self.layers.append(layer.reshape((layer.shape[0] if layer.ndim == 2 else 1), -1) if layer.ndim else layer.reshape(1, 1))

    def dense(self):
        if not self.layers:
            return NP.array(NP.broadcast_to(self.initial, (self.nbl, self.nchan)))
        return NP.stack([NP.broadcast_to(l, (self.nbl, self.nchan)) for l in self.layers], axis=2)

    _ONE = NP.ones((1, 1))

    def ones_like(self):
        # (observe() resets bp_wts to ones of the shape of bp at EVERY snapshot (:6024): a stack that simply follows this one's length --
        # a fresh array per existing layer made that O(n_acc^2) allocations over a run, 0.5 ms of a 0.76 ms config-2 snapshot after 300
        # snapshots; a fresh list per snapshot still O(n_acc))
        return _OnesStack(self)


class _OnesStack(_LayerStack):
    """bp_wts after observe(): ones with as many layers as the bandpass stack it follows."""

    def __init__(self, parent):
        self.nbl, self.nchan = parent.nbl, parent.nchan
        self.initial = self._ONE
        self.parent = parent

    @property
    def layers(self):
        return [self._ONE] * len(self.parent.layers)

    def append(self, layer):
        raise TypeError('bp_wts follows the bandpass stack; assign an array to replace it')


class _SameObject(object):
    """Equal only to a wrapper of the very same object (which it keeps alive: its identity cannot be handed to another object)."""
    __slots__ = ('obj',)

    def __init__(self, obj):
        self.obj = obj

    def __eq__(self, other):
        return isinstance(other, _SameObject) and other.obj is self.obj

    def __ne__(self, other):
        return not self.__eq__(other)

    __hash__ = None


class _LazyGradients(dict):
    """InterferometerArray.gradient: {gradient_mode: (3, nbl, nchan, n_acc)} like the reference's, but the per-snapshot gradient blocks that
    observe() left in the device gradient cube (reserve()) are only fetched -- and stacked, once, instead of the reference's per-snapshot
    dstack (interferometry.py:6385-6393) -- when the entry is read.  Sharded runs that gather the gradients on the device never fetch them."""

    def __init__(self, owner):
        dict.__init__(self)
        self._owner = owner

    def _materialise(self, key):
        ia = self._owner
        if key == ia.gradient_mode and ia._grad and not dict.__contains__(self, key):
            blocks = []
            for i, g in enumerate(ia._grad):
                if isinstance(g, _DeviceSlot):
                    g = ia._ctx.get_vis(slot=g.slot, want_grad=True, complex64=(g.dtype == NP.complex64))[1]
                    ia._grad[i] = g
                blocks.append(g)
            dict.__setitem__(self, key, NP.stack(blocks, axis=3))

    def invalidate(self, key):
        dict.pop(self, key, None)

    def __getitem__(self, key):
        self._materialise(key)
        return dict.__getitem__(self, key)

    def get(self, key, default=None):
        self._materialise(key)
        return dict.get(self, key, default)

    def __contains__(self, key):
        return dict.__contains__(self, key) or (key == self._owner.gradient_mode and bool(self._owner._grad))

    def __bool__(self):
        return dict.__len__(self) > 0 or bool(self._owner._grad)

    def keys(self):
        ks = list(dict.keys(self))
        if self._owner.gradient_mode is not None and self._owner._grad and self._owner.gradient_mode not in ks:
            ks.append(self._owner.gradient_mode)
        return ks

    def items(self):
        return [(k, self[k]) for k in self.keys()]

    def values(self):
        return [self[k] for k in self.keys()]

    def __iter__(self):
        return iter(self.keys())

    def __len__(self):
        return len(self.keys())


class _CatalogROI(object):
    """Entry of ``InterferometerArray.obs_catalog_indices`` (interferometry.py:6377) for a snapshot whose sky was formed on the device
    from the resident catalogue: the integer index list -- and the direction cosines behind ``geometric_delays`` -- are fetched when
    they are read (prisim_hip_catalog_roi forms that snapshot's region of interest again; it is deterministic).  ``size`` / ``len``
    are known from the snapshot's own read-back.  Behaves like the int64 array the reference stores."""

    def __init__(self, owner, obs, lst, pc_dircos, size, frame=None):
        self._owner, self._obs, self._lst, self._pc = owner, obs, float(lst), NP.array(pc_dircos, dtype=NP.float64)
        self._frame = frame
        self.size = int(size)
        self.shape = (self.size,)
        self.ndim = 1
        self.dtype = NP.dtype(NP.int64)
        self._idx = self._dc = None

    def fetch(self):
        if self._idx is None:
            self._idx, self._dc = self._owner._ctx.catalog_roi(self._obs, self._lst, self._pc, frame=self._frame)
            self._owner = self._obs = None
        return self._idx

    def dircos(self):
        self.fetch()
        return self._dc

    def __array__(self, dtype=None, copy=None):
        out = self.fetch()
        return out if dtype is None else out.astype(dtype)

    def __len__(self):
        return self.size

    def __getitem__(self, key):
        return self.fetch()[key]

    def __iter__(self):
        return iter(self.fetch())


class LazyGeometricDelays(object):
    """Stand-in for one entry of ``InterferometerArray.geometric_delays`` (the reference stores the full
    nsrc x nbl matrix per snapshot, interferometry.py:6287-6291 -- 4.9 GB at HERA-350 x 1e4 sources).
    Materialised on demand by ``numpy.asarray(obj)``: tau = dc . bl^T / c.  `dircos`: the (nsrc, 3) array, or the snapshot's
    _CatalogROI (the direction cosines then come from the device when first needed)."""

    def __init__(self, baselines, dircos, dtype):
        self._bl, self._dc, self._dtype = baselines, dircos, dtype
        self.shape = ((dircos.size if isinstance(dircos, _CatalogROI) else dircos.shape[0]), baselines.shape[0])

    def __array__(self, dtype=None, copy=None):
        dc = self._dc.dircos() if isinstance(self._dc, _CatalogROI) else self._dc
        out = DLY.geometric_delay(self._bl, dc, altaz=False, hadec=False, dircos=True).astype(self._dtype)
        return out if dtype is None else out.astype(dtype)


def _available_host_bytes():
    """Host memory that can be claimed without swapping: MemAvailable of /proc/meminfo (free pages + reclaimable cache), else the strictly
    free pages (SC_AVPHYS_PAGES), else None."""
    try:
        with open('/proc/meminfo') as f:
            for line in f:
                if line.startswith('MemAvailable:'):
                    return int(line.split()[1]) * 1024
    except (OSError, ValueError, IndexError):
        pass
    try:
        return os.sysconf('SC_AVPHYS_PAGES') * os.sysconf('SC_PAGE_SIZE')
    except (ValueError, OSError, AttributeError):
        return None


def _lst_and_jd(timeobj, lst):
    """Resolve (jd, lst_deg) from the accepted forms of ``timeobj`` (interferometry.py:6113, 6395)."""
    if hasattr(timeobj, 'sidereal_time'):
        st = timeobj.sidereal_time('apparent')
        lst_deg = float(getattr(st, 'deg', st))
        return float(timeobj.jd), lst_deg       # the lst kwarg is overwritten, as in the reference (:6113)
    if isinstance(timeobj, (tuple, list)) and len(timeobj) == 2:
        return float(timeobj[0]), float(timeobj[1])
    if isinstance(timeobj, dict) and 'jd' in timeobj and 'lst' in timeobj:
        return float(timeobj['jd']), float(timeobj['lst'])
    if isinstance(timeobj, (int, float, NP.floating, NP.integer)):
        if lst is None:
            raise ValueError('LST must be provided when timeobj is a bare Julian date.')
        return float(timeobj), float(lst)
    raise TypeError('timeobj must be a Time-like object, a (jd, lst_deg) pair, or a Julian date with lst given.')


def _closure_prepare(self, antenna_triplets, delay_filter_info, specsmooth_info, spectral_window_info, unique):
    """What getClosurePhase prepares before its device calls (interferometry.py:7296-7485), for it and for
    DelaySpectrum.subband_delay_transform_closure_phase: the argument checks in the reference's order, the spectral window, the filter
    masks, the leg table, bp * bp_wts, and whether the noiseless cube can be read where it lies on the device.  `self` is the array (or a
    stand-in with the attributes read)."""
    from . import delay_spectrum as DS
    from . import dsp_readings as DSP
    if antenna_triplets is None:
        antenna_triplets, _ = self.getThreePointCombinations(unique=unique)
    if not isinstance(antenna_triplets, list):
        raise TypeError('Input antenna triplets must be a list of triplet tuples')
    if specsmooth_info is not None:
        raise NotImplementedError("specsmooth_info is not supported: the reference's 'median' branch indexes specsmooth_info["
                                  "specsmooth_info['window_size']] and cannot run, and 'interp' redraws noise from numpy's global "
                                  "generator")
    nchan = self.channels.size
    if spectral_window_info is not None:                                       # :7296-7344
        freq_center, bw_eff = spectral_window_info['freq_center'], spectral_window_info['bw_eff']
        shape, fftpow = spectral_window_info['shape'], spectral_window_info['fftpow']
        if freq_center is None:
            freq_center = self.channels[nchan // 2]
        shape = 'rect' if shape is None else shape.lower()
        if bw_eff is None:
            if shape == 'rect':
                bw_eff = nchan * self.freq_resolution
            elif shape == 'bhw':
                bw_eff = 0.5 * nchan * self.freq_resolution
            else:
                raise ValueError('Specified window shape not currently supported')
        if fftpow is None:
            fftpow = 1.0
        elif isinstance(fftpow, (int, float)):
            if fftpow <= 0.0:
                raise ValueError('Value fftpow must be positive')
        else:
            raise ValueError('Value fftpow must be a scalar (int or float)')
        wts = DS.subband_freq_wts(self.channels, self.freq_resolution, NP.asarray(bw_eff, dtype=NP.float64).reshape(-1),
                                  NP.asarray(freq_center, dtype=NP.float64).reshape(-1), shape, fftpow)
        if wts.shape[0] != 1:
            raise ValueError('freq_center is outside the band')
        freq_wts = wts[0]
    else:
        freq_wts = NP.asarray(1.0).reshape(-1)

    masks = mask_index = None
    if delay_filter_info is not None:                                          # :7350-7399
        fft_delays = DSP.spectral_axis(nchan, delx=self.freq_resolution, shift=False, use_real=False)
        dtau = fft_delays[1] - fft_delays[0]
        if not isinstance(delay_filter_info, dict):
            raise TypeError('Delay filter info must be specified as a dictionary')
        filter_mode = delay_filter_info.get('mode', 'discard')
        if filter_mode.lower() not in ['discard', 'retain']:
            raise ValueError('Invalid delay filter mode specified')
        filter_type = delay_filter_info.get('type', 'horizon')
        if filter_type.lower() not in ['horizon', 'regular']:
            raise ValueError('Invalid delay filter type specified')
        if filter_type.lower() == 'regular':
            if ('min' not in delay_filter_info) or ('width' not in delay_filter_info):
                raise KeyError('Keys "min" and "width" must be specified in input delay_filter_info')
            delay_min, delay_width = delay_filter_info['min'], delay_filter_info['width']
            if delay_min is None:
                delay_min = 0.0
            elif isinstance(delay_min, (int, float)):
                delay_min = max([0.0, delay_min])
            else:
                raise TypeError('Minimum delay in the filter must be a scalar value (int or float)')
            if isinstance(delay_width, (int, float)):
                if delay_width <= 0.0:
                    raise ValueError('Delay filter width must be positive')
            else:
                raise TypeError('Delay width in the filter must be a scalar value (int or float)')
        else:
            delay_width = delay_filter_info.get('width', 0.0)
            if delay_width is None:
                delay_width = 0.0
            elif isinstance(delay_width, (int, float)):
                if delay_width <= 0.0:
                    raise ValueError('Delay filter width must be positive')
            else:
                raise TypeError('Delay width in the filter must be a scalar value (int or float)')
        delay_width = delay_width * dtau
        masks, mask_index = closure_filter_masks(fft_delays, filter_type.lower(), filter_mode.lower(),
                                                 delay_min if filter_type.lower() == 'regular' else 0.0, delay_width,
                                                 self.baseline_lengths)

    legs, conj, blvecttriplets = self.closure_leg_table(antenna_triplets)
    nbl = self.baselines.shape[0]
    if self.skyvis_freq is None and not getattr(self, '_cube', None):
        raise ValueError('no visibilities: call observe() first')
    nt = len(self._cube)
    # the noiseless cube is read where it lies when the device slots [0, nt) hold skyvis_freq itself, in fp64 (the rule of add_noise)
    resident = bool(self._device_in_step) and nt <= self._reserved and all(
        sn.dtype == NP.complex128 and (not isinstance(sn, _DeviceSlot) or sn.slot == i) for i, sn in enumerate(self._cube))
    bpwts = NP.asarray(self.bp * self.bp_wts, dtype=NP.float64).reshape(nbl, nchan, -1)      # :7433, formed once for the call
    return {'antenna_triplets': antenna_triplets, 'freq_wts': freq_wts, 'masks': masks, 'mask_index': mask_index, 'legs': legs,
            'conj': conj, 'baseline_triplets': blvecttriplets, 'nbl': nbl, 'nchan': nchan, 'nt': nt, 'resident': resident, 'bpwts': bpwts}


def closure_filter_masks(fft_delays, filter_type, filter_mode, delay_min, delay_width, baseline_lengths):
    """The filter_unmask vectors of getClosurePhase's delay filter (interferometry.py:7536-7543 'regular', :7570-7587 'horizon') on the
    unshifted FFT delay axis: ones with zeros on the filtered delays.  'regular': one mask, zero where delay_min <= |tau| <= delay_min +
    delay_width ('discard') or where |tau| <= delay_min or |tau| >= delay_min + delay_width ('retain').  'horizon': one mask per
    baseline with delay_max = |b| / c + delay_width, zero where |tau| <= delay_max ('discard') or |tau| >= delay_max ('retain').
    Returns (masks (nmask, nchan), mask_index (nbl,) int32 or None: mask 0 for every baseline)."""
    tau = NP.abs(NP.asarray(fft_delays, dtype=NP.float64))
    if filter_type == 'regular':
        delay_max = delay_min + delay_width
        if filter_mode == 'discard':
            zero = NP.logical_and(tau >= delay_min, tau <= delay_max)
        else:
            zero = NP.logical_or(tau <= delay_min, tau >= delay_max)
        return NP.where(zero, 0.0, 1.0).reshape(1, -1), None
    delay_max = NP.asarray(baseline_lengths, dtype=NP.float64) / C_LIGHT + delay_width
    zero = tau[NP.newaxis, :] <= delay_max[:, NP.newaxis] if filter_mode == 'discard' else tau[NP.newaxis, :] >= delay_max[:, NP.newaxis]
    rows, mask_index = NP.unique(zero, axis=0, return_inverse=True)
    return NP.where(rows, 0.0, 1.0), NP.asarray(mask_index, dtype=NP.int32).ravel()


def _same_beam_spec(a, b):
    """Whether two values of primary_beams.device_beam_spec (nested tuples and dicts of scalars and arrays) are equal."""
    if isinstance(a, dict) or isinstance(b, dict):
        return (isinstance(a, dict) and isinstance(b, dict) and sorted(a) == sorted(b)
                and all(_same_beam_spec(a[k], b[k]) for k in a))
    if isinstance(a, (tuple, list)) or isinstance(b, (tuple, list)):
        return (isinstance(a, (tuple, list)) and isinstance(b, (tuple, list)) and len(a) == len(b)
                and all(_same_beam_spec(x, y) for x, y in zip(a, b)))
    if a is None or b is None:
        return a is None and b is None
    return NP.array_equal(NP.asarray(a), NP.asarray(b))


def _antenna_power_pointings(pointing_info, lst, latitude):
    """The pointing centres of antenna_power as (n_lst, 2) alt-az degrees, with the reference's checks (interferometry.py:2332-2369)."""
    n_lst = lst.size
    if 'pointing_center' not in pointing_info:
        return NP.repeat(NP.asarray([90.0, 270.0]).reshape(1, -1), n_lst, axis=0)
    if 'pointing_coords' not in pointing_info:
        raise KeyError('key "pointing_coords" not found in input parameter pointing_info')
    pointing_coords = pointing_info['pointing_coords']
    if not isinstance(pointing_info['pointing_center'], NP.ndarray):
        raise TypeError('Value in key "pointing_center" in input parameter pointing_info must be a numpy array')
    pointing_center = pointing_info['pointing_center']
    if pointing_center.ndim > 2:
        raise ValueError('Value under key "pointing_center" in input parameter pointing_info cannot exceed two dimensions')
    if pointing_center.ndim < 2:
        pointing_center = pointing_center.reshape(1, -1)
    if pointing_coords == 'dircos':
        if pointing_center.shape[1] != 3:
            raise ValueError('Value under key "pointing_center" in input parameter pointing_info must be a 3-column array for direction '
                             'cosine coordinate system')
    elif pointing_center.shape[1] != 2:
        raise ValueError('Value under key "pointing_center" in input parameter pointing_info must be a 2-column array for RA-Dec, HA-Dec '
                         'and Alt-Az coordinate systems')
    n_pointings = pointing_center.shape[0]
    if (n_pointings != n_lst) and (n_pointings != 1):
        raise ValueError('Number of pointing centers and number of LST must match')
    if n_pointings < n_lst:
        pointing_center = NP.repeat(pointing_center, n_lst, axis=0)
    pointing_center = NP.asarray(pointing_center, dtype=NP.float64)
    if pointing_coords == 'dircos':
        return GEOM.dircos2altaz(pointing_center, units='degrees')
    if pointing_coords == 'hadec':
        return GEOM.hadec2altaz(pointing_center, latitude, units='degrees')
    if pointing_coords == 'radec':
        return GEOM.hadec2altaz(NP.stack((lst - pointing_center[:, 0], pointing_center[:, 1]), axis=1), latitude, units='degrees')
    return NP.copy(pointing_center)


def antenna_power(skymodel, telescope_info, pointing_info, freq_scale=None, frequency=None, coords=None, frames=None, device=0,
                  budget_bytes=None, stats=None):
    """Antenna power received from the sky for a sky model, a telescope and pointings: for every LST and channel
    sum_s pb(s, f) S_s(f) / sum_s pb(s, f) over the sources above the horizon (alt >= 0), the reference's antenna_power
    (prisim/interferometry.py:2169-2408), with its signature, argument meaning and exceptions.  With a diffuse model in kelvin this is
    the antenna temperature, with point sources the beam-weighted flux.  The rotation into the local frame, the beam and both sums run
    on the device (include/prisim_antpower.h); only the (n_lst, nchan) result comes back.

    skymodel        a SkyModel.  A 'spectrum' model is used on its own grid: skymodel.frequency is the channel axis, as in the reference.
                    A 'func' (power-law) model has no grid here and needs frequency=; its ref_freq is in the units of that axis, and the
                    power law is evaluated on the device.
    telescope_info  the reference's dictionary: 'latitude' (default -26.701), 'id' or 'shape' / 'size' / 'orientation' / 'ocoords',
                    'element_locs', 'groundplane', 'ground_modify' (prisim_amd.primary_beams.device_beam_spec; rect / square apertures
                    raise its NotImplementedError).
    pointing_info   'lst' (degrees, one per pointing); optionally 'pointing_center' with 'pointing_coords' ('radec', 'hadec', 'altaz':
                    M x 2; 'dircos': M x 3; M = n_lst, or 1 for all; default alt-az [90, 270]).  As in the reference (:2392-2400) the
                    pointing reaches the beam only as the pointing_info of a phased array's beamformer; dishes and Gaussians point
                    where telescope_info says, the zenith by default.
    freq_scale      units of the frequencies: 'GHz', 'MHz', 'kHz' or 'Hz'; None is Hz (how primary_beams.py:212-217 reads it).
    coords          frame of skymodel.location: 'radec', 'hadec', 'altaz' or 'dircos'; default skymodel.coords, else 'radec'.
    frames          one (cel2enu (3, 3), aberr_beta (3,)) per LST, as prisim_amd.frames.snapshot_frame returns.  The default for
                    'radec' is the plain hour-angle rotation HA = LST - RA, which is what the reference computes (:2372-2379) and right
                    for coordinates of date; frames= gives the true place of a catalogue of another epoch (precession, nutation and
                    aberration, some degrees over decades for a narrow beam).
    device, budget_bytes, stats    the GPU, the device bytes of the streamed buffers, and a dict that receives the entry's statistics.

    Returns (n_lst, nchan) float64.  A pointing with no source above the horizon is a row of NaN.

    Departures from the reference: no progress bar; a 'dircos' pointing is accepted (the reference's elif at :2350 rejects every
    3-column array); frequency=, coords=, frames=, device=, budget_bytes= and stats= are additions; NaN rows come back without a
    numpy warning."""
    if not hasattr(skymodel, 'location'):
        raise TypeError('Input parameter skymodel must be an instance of class SkyModel')
    if not isinstance(telescope_info, dict):
        raise TypeError('Input parameter telescope_info must be a dictionary')
    if not isinstance(pointing_info, dict):
        raise TypeError('Input parameter pointing_info must be a dictionary')
    latitude = telescope_info['latitude'] if 'latitude' in telescope_info else -26.701
    if 'lst' not in pointing_info:
        raise KeyError('Key "lst" not provided in input parameter pointing_info')
    lst = NP.asarray(pointing_info['lst'], dtype=NP.float64).ravel()
    n_lst = lst.size
    pointings_altaz = _antenna_power_pointings(pointing_info, lst, latitude)

    # channels and spectra
    scale = {'ghz': 1.0e9, 'mhz': 1.0e6, 'khz': 1.0e3}.get(freq_scale.lower() if isinstance(freq_scale, str) else None, 1.0)
    flux = {}
    if getattr(skymodel, 'spec_type', 'func') == 'spectrum':
        chans = NP.asarray(skymodel.frequency if frequency is None else frequency, dtype=NP.float64).ravel()
        flux['flux_spectrum'] = skymodel.generate_spectrum(frequency=chans, interp_method='pchip')
    else:
        if frequency is None:
            raise ValueError('a power-law sky model has no frequency grid: give frequency=')
        chans = NP.asarray(frequency, dtype=NP.float64).ravel()
        flux.update(flux_ref=skymodel.flux_ref, spindex=skymodel.spindex, ref_freq_hz=float(skymodel.ref_freq) * scale)
    freqs_hz = chans * scale

    # the sky in its own frame, and one rotation per LST
    coords = coords or getattr(skymodel, 'coords', None) or 'radec'
    if coords in ('radec', 'hadec', 'altaz'):
        unitvec = GEOM.catalog_unitvec(skymodel.location, coords)
    elif coords == 'dircos':
        unitvec = NP.asarray(skymodel.location, dtype=NP.float64).reshape(-1, 3)
    else:
        raise ValueError('coords must be "radec", "hadec", "altaz" or "dircos"')
    beta = None
    if frames is not None:
        frames = list(frames)
        if len(frames) != n_lst:
            raise ValueError('frames must hold one (cel2enu, aberr_beta) per LST')
        rot = NP.stack([NP.asarray(f[0], dtype=NP.float64).reshape(3, 3) for f in frames])
        beta = NP.stack([NP.asarray(f[1], dtype=NP.float64).reshape(3) for f in frames])
    elif coords == 'radec':
        rot = NP.stack([FRAMES.equatorial_to_enu(l, latitude) for l in lst])
    elif coords == 'hadec':
        rot = NP.repeat(FRAMES.hadec_to_enu(latitude)[NP.newaxis], n_lst, axis=0)
    else:
        rot = NP.repeat(NP.eye(3)[NP.newaxis], n_lst, axis=0)

    # the beam of every LST: one shared description unless a beamformer's delays follow the pointing
    specs = [PB.device_beam_spec(telescope_info, pointing_info={'pointing_center': pointings_altaz[i, :], 'pointing_coords': 'altaz'},
                                 first_frequency_hz=float(freqs_hz[0])) for i in range(n_lst)]
    kind, dia, bpc, ext0 = specs[0]
    if all(_same_beam_spec(specs[0], sp) for sp in specs[1:]):
        ext = ext0
    else:
        ext = [sp[3] for sp in specs]
    with _abi.Context(device) as ctx:
        power, _, _, st = ctx.antenna_power(unitvec, freqs_hz, rot, kind, dia, beam_pc_dircos=bpc, aberr_beta=beta, ext=ext,
                                            budget_bytes=int(budget_bytes or 0), want_sums=False, **flux)
    if stats is not None:
        stats.update(st)
    return power


def _label_from_text(s):
    """A baseline label back from the text save() wrote for it (str(label), '/' written as '|' in dataset names): the tuple of
    strings that ast.literal_eval gives (interferometry.py:5394-5397), or, for a text that is no literal (numpy scalars inside the
    tuple), its quoted fields; any other text stays a string."""
    import ast
    import re
    try:
        v = ast.literal_eval(s)
    except (ValueError, SyntaxError):
        fields = re.findall(r"'([^']*)'", s)
        return tuple(fields) if fields else s
    return tuple(str(x) for x in v) if isinstance(v, (tuple, list)) else v


class InterferometerArray(object):
    """Interferometer array whose snapshots are simulated on one MI355X (see module docstring).

    Attributes touched by observe() keep the reference's names and shapes:
    bp, bp_wts, Tsys, Tsysinfo, pointing_center, phase_center, geometric_delays, obs_catalog_indices,
    skyvis_freq, gradient, gradient_mode, timestamp, t_acc, t_obs, n_acc, lst.
    """

    # Astrometric model of skycoords 'radec' (module docstring; prisim_amd/frames.py): 'apparent' | 'mean' | 'date', and an optional
    # callable (jd, lst_deg, skymodel) -> (R (3, 3), beta (3,)) that replaces it (e.g. filled from astropy)
    frame_model = os.environ.get('PRISIM_FRAME_MODEL', 'apparent')
    frame_provider = None

    def __init__(self, labels, baselines, channels, telescope=None, eff_Q=0.89,
                 latitude=34.0790, longitude=0.0, altitude=0.0, skycoords='radec',
                 A_eff=NP.pi * (25.0 / 2) ** 2, pointing_coords='hadec', layout=None,
                 blgroupinfo=None, baseline_coords='localenu', freq_scale=None,
                 gaininfo=None, init_file=None, simparms_file=None, device=0):
        if init_file is not None:
            # interferometry.py:5184-5658: initialise from <init_file>.hdf5; if it cannot be opened, fall back to the arguments
            try:
                self._init_from_hdf5(init_file, device)
                return
            except (IOError, OSError) as exc:
                warnings.warn('\tinit_file provided but could not open the initialization file ({0}). Attempting to initialize '
                              'with input parameters...'.format(exc))
        if gaininfo is not None and not isinstance(gaininfo, GainInfo):                 # :5773-5777
            raise TypeError('Input gaininfo must be an instance of class GainInfo')

        self.baselines = NP.asarray(baselines, dtype=NP.float64)                      # :5668-5682
        if self.baselines.ndim == 1:
            if self.baselines.size == 2:
                self.baselines = NP.hstack((self.baselines.reshape(1, -1), NP.zeros((1, 1))))
            elif self.baselines.size == 3:
                self.baselines = self.baselines.reshape(1, -1)
            else:
                raise ValueError('Baseline(s) must be a 2- or 3-column array.')
        elif self.baselines.ndim == 2:
            if self.baselines.shape[1] == 2:
                self.baselines = NP.hstack((self.baselines, NP.zeros((self.baselines.shape[0], 1))))
            elif self.baselines.shape[1] != 3:
                raise ValueError('Baseline(s) must be a 2- or 3-column array')
        else:
            raise ValueError('Baseline(s) array contains more than 2 dimensions.')
        self.baseline_lengths = NP.sqrt(NP.sum(self.baselines ** 2, axis=1))         # :5684
        self.baseline_orientations = NP.angle(self.baselines[:, 0] + 1j * self.baselines[:, 1])
        self.projected_baselines = None

        if not isinstance(labels, (list, tuple, NP.ndarray)):                         # :5688-5693
            raise TypeError('Interferometer array labels must be a list or tuple of unique identifiers')
        elif len(labels) != self.baselines.shape[0]:
            raise ValueError('Number of labels do not match the number of baselines specified.')
        self.labels = labels
        self.simparms_file = simparms_file if isinstance(simparms_file, str) else None

        if isinstance(telescope, dict):                                               # :5701-5710
            self.telescope = telescope
        else:
            self.telescope = {'id': 'vla', 'shape': 'dish', 'size': 25.0, 'ocoords': 'altaz',
                              'orientation': NP.asarray([90.0, 270.0]).reshape(1, -1), 'groundplane': None}
        self.layout = {}
        if isinstance(layout, dict):                                                  # :5713-5751
            for key in ('positions', 'coords', 'labels', 'ids'):
                if key not in layout:
                    raise KeyError('Array layout {0} missing'.format(key))
            self.layout = dict(layout)
        self.blgroups = None
        self.bl_reversemap = None
        if blgroupinfo is not None:
            if not isinstance(blgroupinfo, dict):
                raise TypeError('Input blgroupinfo must be a dictionary')
            self.blgroups = blgroupinfo['groups']
            self.bl_reversemap = blgroupinfo['reversemap']

        self.latitude, self.longitude, self.altitude = latitude, longitude, altitude
        self.vis_freq = None
        self.skyvis_freq = None
        self.vis_noise_freq = None
        self.gradient_mode = None
        self.gradient = {}
        self.gaininfo = gaininfo
        self.gain_padding = None      # bool (nbl,): rows that get unity gains whatever the table holds (the padding rows of a shard)

        ch = NP.asarray(channels, dtype=NP.float64).ravel()                           # :5779-5788
        if (freq_scale is None) or (freq_scale in ('Hz', 'hz')):
            self.channels = ch
        elif freq_scale in ('GHz', 'ghz'):
            self.channels = ch * 1.0e9
        elif freq_scale in ('MHz', 'mhz'):
            self.channels = ch * 1.0e6
        elif freq_scale in ('kHz', 'khz'):
            self.channels = ch * 1.0e3
        else:
            raise ValueError('Frequency units must be "GHz", "MHz", "kHz" or "Hz". If not set, it defaults to "Hz"')

        nbl, nchan = self.baselines.shape[0], self.channels.size
        self._stacks = {'bp': _LayerStack(nbl, nchan, NP.ones((1, 1))), 'bp_wts': _LayerStack(nbl, nchan, NP.ones((1, 1))),
                        'Tsys': _LayerStack(nbl, nchan, NP.zeros((1, 1)))}                # :5790-5793, read through the properties below
        self._dense = {}
        self.lag_kernel = None
        self.Tsysinfo = []
        self.flux_unit = 'JY'
        self.timestamp = []
        self.t_acc = []
        self.t_obs = 0.0
        self.n_acc = 0
        self.pointing_center = NP.empty([1, 2])
        self.phase_center = NP.empty([1, 2])
        self.lst = []

        self.eff_Q = self._broadcast_bl_chan(eff_Q, 'Efficiency', lo=0.0, hi=1.0)      # :5806-5824
        self.A_eff = self._broadcast_bl_chan(A_eff, 'Effective area', lo=0.0, hi=None)  # :5826-5844

        self.vis_rms_freq = None
        self.freq_resolution = self.channels[1] - self.channels[0] if nchan > 1 else 0.0   # :5847
        self.lags = None
        self.skyvis_lag = None
        self.vis_noise_lag = None
        self.vis_lag = None
        self.obs_catalog_indices = []
        self.geometric_delays = []

        if pointing_coords in ('radec', 'hadec', 'altaz'):                            # :5856-5860
            self.pointing_coords = pointing_coords
            self.phase_center_coords = pointing_coords
        else:
            raise ValueError('Pointing center of the interferometer must be "radec", "hadec" or "altaz". Check inputs.')
        if skycoords in ('radec', 'hadec', 'altaz'):                                  # :5862-5865
            self.skycoords = skycoords
        else:
            raise ValueError('Sky coordinates must be "radec", "hadec" or "altaz". Check inputs.')
        if baseline_coords in ('equatorial', 'localenu'):                             # :5867-5870
            self.baseline_coords = baseline_coords
        else:
            raise ValueError('Baseline coordinates must be "equatorial" or "local". Check inputs.')

        # GPU context: fails loudly when the HIP library or a device is missing
        self._ctx = _abi.Context(device)
        self._ctx.set_array(self._baselines_local(), self.channels, nt_max=1)
        self._cube = []        # per-snapshot (nbl, nchan) visibilities, stacked lazily into skyvis_freq
        self._grad = []
        self._reserved = 1     # snapshot slots of the device cube (reserve())
        self._stage, self._host_cube = False, None      # reserve(host_staging=True): snapshots are copied to a pinned host cube as they finish
        self._device_in_step = False                    # device slots [0, n_acc) hold the current skyvis_freq

    def _init_from_hdf5(self, init_file, device):
        """Attributes from a file written by save() / by PRISim (interferometry.py:5186-5657; same group and dataset names,
        same KeyErrors for what is mandatory there).  The visibility cube goes back onto the device, snapshot t in slot t."""
        from . import hdf5io
        fname = init_file if init_file.endswith('.hdf5') else init_file + '.hdf5'
        if not os.path.exists(fname):
            raise IOError('no such file: ' + fname)
        try:
            f = hdf5io.File(fname, 'r')
        except hdf5io.HDF5Unavailable as exc:
            raise IOError(str(exc))
        def text(v):
            return v.decode() if isinstance(v, bytes) else str(v)
        with f:
            def get(path, default=None, required=None):
                if f.exists(path):
                    return f.read(path)
                if required:
                    raise KeyError(required)
                return default
            for key in ('header', 'telescope_parms', 'spectral_info', 'antenna_element', 'timing', 'skyparms', 'array', 'instrument',
                        'visibilities'):
                if not f.exists(key):
                    raise KeyError('Key {0} not found in init_file'.format(key))
            self.simparms_file = get('simparms/simfile')
            self.flux_unit = text(get('header/flux_unit', 'JY'))
            self.latitude = float(get('telescope_parms/latitude', 0.0))
            self.longitude = float(get('telescope_parms/longitude', 0.0))
            self.altitude = float(get('telescope_parms/altitude', 0.0))
            self.telescope = {'shape': 'delta', 'size': 1.0, 'groundplane': None}
            if f.exists('telescope_parms/id'):
                self.telescope['id'] = text(f.read('telescope_parms/id'))
            if f.exists('antenna_element/shape'):
                self.telescope['shape'] = text(f.read('antenna_element/shape'))
            if f.exists('antenna_element/size'):
                size = NP.asarray(f.read('antenna_element/size'), dtype=NP.float64)
                self.telescope['size'] = float(size) if size.ndim == 0 else size
            self.telescope['ocoords'] = text(get('antenna_element/ocoords', required='Keyword "ocoords" not found in init_file'))
            self.telescope['orientation'] = NP.asarray(get('antenna_element/orientation', required='Key "orientation" not found in init_file'),
                                                       dtype=NP.float64).reshape(1, -1)
            if f.exists('antenna_element/groundplane'):
                self.telescope['groundplane'] = float(f.read('antenna_element/groundplane'))
            self.layout = {}
            if f.exists('layout'):
                self.layout = {'positions': get('layout/positions', required='Antenna layout positions is missing'),
                               'coords': text(f.read_attr('layout/positions', 'coords')),
                               'labels': get('layout/labels', required='Layout antenna labels is missing'),
                               'ids': get('layout/ids', required='Layout antenna ids is missing')}
            self.freq_resolution = float(f.read('spectral_info/freq_resolution'))
            self.channels = NP.asarray(f.read('spectral_info/freqs'), dtype=NP.float64)
            self.lags = get('spectral_info/lags')
            self.bp = NP.asarray(get('spectral_info/bp', required='Key "bp" not found in init_file'))
            self.bp_wts = NP.asarray(get('spectral_info/bp_wts', NP.ones_like(self.bp)))
            self.pointing_coords = text(get('skyparms/pointing_coords', 'hadec'))
            self.phase_center_coords = text(get('skyparms/phase_center_coords', self.pointing_coords))
            self.skycoords = text(get('skyparms/skycoords', 'radec'))
            self.lst = NP.asarray(f.read('skyparms/LST')).ravel().tolist()
            self.pointing_center = NP.asarray(f.read('skyparms/pointing_center'))
            self.phase_center = NP.asarray(f.read('skyparms/phase_center'))
            self.timestamp = NP.asarray(get('timing/timestamps', required='Key "timestamps" not found in init_file')).tolist()
            self.t_acc = NP.asarray(get('timing/t_acc', required='Key "t_acc" not found in init_file')).ravel().tolist()
            self.t_obs = float(f.read('timing/t_obs'))
            self.n_acc = int(f.read('timing/n_acc'))
            labels = get('array/labels', required='Key "labels" not found in init_file')
            if labels.dtype.names:
                self.labels = [tuple(text(x) for x in rec) for rec in labels.tolist()]
            else:
                self.labels = [text(x) for x in labels.tolist()]
            self.baselines = NP.asarray(get('array/baselines', required='Key "baselines" not found in init_file'), dtype=NP.float64)
            self.baseline_coords = text(get('array/baseline_coords', 'localenu'))
            self.projected_baselines = get('array/projected_baselines')
            self.baseline_lengths = NP.sqrt(NP.sum(self.baselines ** 2, axis=1))
            self.baseline_orientations = NP.angle(self.baselines[:, 0] + 1j * self.baselines[:, 1])
            self.A_eff = NP.asarray(f.read('instrument/effective_area'))
            self.eff_Q = NP.asarray(f.read('instrument/efficiency'))
            self.Tsysinfo = []
            if f.exists('instrument/Trx'):
                trx, t0, f0, sp = (NP.asarray(f.read('instrument/' + k)).ravel() for k in ('Trx', 'Tant0', 'f0', 'spindex'))
                tnet = NP.asarray(get('instrument/Tnet', NP.full(trx.size, -999.0))).ravel()
                for i in range(trx.size):
                    self.Tsysinfo += [{'Trx': float(trx[i]), 'Tant': {'T0': float(t0[i]), 'f0': float(f0[i]), 'spindex': float(sp[i])},
                                       'Tnet': float(tnet[i]) if tnet[i] > 0 else None}]
            self.Tsys = NP.asarray(get('instrument/Tsys', NP.zeros((self.baselines.shape[0], self.channels.size))))
            self.vis_rms_freq = get('visibilities/freq_spectrum/rms')
            self.vis_freq = get('visibilities/freq_spectrum/vis')
            skyvis = get('visibilities/freq_spectrum/skyvis', required='Key "skyvis" not found in init_file')
            self.vis_noise_freq = get('visibilities/freq_spectrum/noise')
            self.vis_lag = get('visibilities/delay_spectrum/vis')
            self.skyvis_lag = get('visibilities/delay_spectrum/skyvis')
            self.vis_noise_lag = get('visibilities/delay_spectrum/noise')
            self.gradient_mode, self.gradient = None, {}
            if f.exists('gradients/baseline'):
                self.gradient_mode = 'baseline'
                self.gradient = {'baseline': f.read('gradients/baseline')}
            gainsfile = get('gaininfo/gainsfile')                                      # :5387-5389
            blgroups = bl_reversemap = None                                            # :5390-5397
            if f.exists('blgroupinfo'):
                blgroups, bl_reversemap = {}, {}
                for name in (f.list('blgroupinfo/groups') if f.exists('blgroupinfo/groups') else []):
                    blgroups[_label_from_text(name.replace('|', '/'))] = [_label_from_text(text(m)) for m in
                                                                          NP.asarray(f.read('blgroupinfo/groups/' + name)).ravel()]
                for name in (f.list('blgroupinfo/reversemap') if f.exists('blgroupinfo/reversemap') else []):
                    bl_reversemap[_label_from_text(name.replace('|', '/'))] = _label_from_text(
                        text(NP.asarray(f.read('blgroupinfo/reversemap/' + name)).ravel()[0]))
        self.gaininfo = None if gainsfile is None else GainInfo(init_file=text(gainsfile))
        self.gain_padding = None
        self.blgroups, self.bl_reversemap = blgroups, bl_reversemap
        self.lag_kernel = None
        self.obs_catalog_indices = []
        self.geometric_delays = []
        self._cube, self._grad = [], []
        self._reserved = max(int(self.n_acc), 1)
        self._ctx = _abi.Context(device)
        self._ctx.set_array(self._baselines_local(), self.channels, nt_max=self._reserved)
        self._stage, self._host_cube = False, None
        self.skyvis_freq = skyvis
        self._upload_cube()

    def _baselines_local(self):
        """The baselines in the local East-North-Up frame the sky-sum works in: as given, or rotated from the equatorial frame at the
        array's latitude (baseline_coords='equatorial'; interferometry.py:6151-6153 does this at every observe())."""
        if getattr(self, 'baseline_coords', 'localenu') == 'equatorial':
            return GEOM.xyz2enu(self.baselines, self.latitude, 'degrees')
        return self.baselines

    def reserve(self, n_acc, host_staging=False):
        """Allocate `n_acc` snapshot slots in the device visibility cube so that every observe() also leaves its result
        resident on the GPU (slot = snapshot index) for a later allgather() / device-side delay transform.  Not in the
        reference (its cube is a host array grown by dstack, interferometry.py:6384-6393).

        host_staging=True: the reference's product is skyvis_freq ON THE HOST (:6384-6393).  Every observe() then also enqueues the
        download of its snapshot into a page-locked host cube on a copy stream, behind its own sky-sum and beside the next one's
        (prisim_hip_get_vis_async): reading skyvis_freq afterwards only waits for the last copy instead of pulling the whole cube
        over PCIe in one serial tail.  Falls back to the lazy download when the pinned cube cannot be allocated."""
        n_acc = int(n_acc)
        if n_acc < 1:
            raise ValueError('n_acc must be positive')
        if self.n_acc > 0:
            raise RuntimeError('reserve() must be called before the first observe()')
        self._ctx.set_array(self._baselines_local(), self.channels, nt_max=n_acc)
        self._reserved = n_acc
        self._stage, self._host_cube = bool(host_staging), None
        self._restore_external_beam()
        self._catalog_key = None                       # (set_array drops the resident catalogue)

    def _reset_device_array(self):
        """set_array of the (changed) baselines after snapshots have been observed: what lives only on the device is fetched first --
        the catalogue-resident index lists and the gradient blocks observe() left in the device gradient cube (prisim_hip_set_array
        releases that cube) -- and the catalogue is uploaded again by the next observe()."""
        self._materialise_catalog_state()
        if self.gradient_mode is not None and isinstance(self.gradient, _LazyGradients):
            self.gradient.get(self.gradient_mode)
        self._ctx.set_array(self._baselines_local(), self.channels, nt_max=self._reserved)
        self._restore_external_beam()
        self._catalog_key = None

    def _cull_order(self, alt_deg, fwhm_deg):
        """Permutation that lists every run of sources of one size by decreasing altitude, or None when nothing could be culled
        (no source sizes, short baselines, more than 8 runs, or the sources already are in that order)."""
        if fwhm_deg is None or fwhm_deg.size < 2:
            return None
        kmax = NP.log(2.0) * (2.0 * NP.sin(0.5 * NP.radians(float(NP.max(fwhm_deg))))) ** 2
        lmax = float(NP.max(self.baseline_lengths)) if self.baseline_lengths.size else 0.0
        fmin = float(NP.min(NP.abs(self.channels)))
        if not kmax * (lmax * fmin / C_LIGHT) ** 2 >= 18.0:
            return None
        cuts = NP.flatnonzero(fwhm_deg[1:] != fwhm_deg[:-1]) + 1
        if cuts.size >= 8:
            return None
        order = NP.arange(fwhm_deg.size)
        bounds = NP.concatenate(([0], cuts, [fwhm_deg.size]))
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            order[lo:hi] = lo + NP.argsort(-alt_deg[lo:hi], kind='stable')
        return None if NP.array_equal(order, NP.arange(order.size)) else order

    def _ensure_host_cube(self, dtype):
        """The page-locked host cube of reserve(host_staging=True) (allocated on first use), or None when staging is off, unavailable,
        or the cube holds another dtype."""
        if not getattr(self, '_stage', False):
            return None
        if self._host_cube is None:
            need = self._reserved * self.baselines.shape[0] * self.channels.size * NP.dtype(dtype).itemsize
            avail = _available_host_bytes()
            # Page-locked memory cannot be swapped or reclaimed, and reading skyvis_freq afterwards stacks the snapshots into a second
            # (pageable) cube of the same size beside it: the budget is 2 x need, against what the kernel says can be made available
            # (MemAvailable: free + reclaimable page cache -- a box that has just read a large catalog is not short of memory)
            if avail is not None and 2 * need > avail:
                warnings.warn('host staging switched off: the pinned host cube and its (nbl, nchan, n_acc) copy would need {0:.1f} GiB of '
                              '{1:.1f} GiB available'.format(2 * need / 2.0 ** 30, avail / 2.0 ** 30))
                self._stage = False
                return None
            try:
                self._host_cube = _abi.host_empty((self._reserved, self.baselines.shape[0], self.channels.size), dtype)
            except (MemoryError, _abi.PrisimHipError, OSError) as exc:
                warnings.warn('host staging switched off: the pinned host cube could not be allocated ({0})'.format(exc))
                self._stage = False
                return None
        if self._host_cube.dtype != NP.dtype(dtype):
            return None                      # a run that mixes memsave and full precision: this snapshot takes the lazy path
        return self._host_cube

    def _stage_download(self, slot, dtype):
        """Enqueue the asynchronous download of device slot `slot` into the pinned host cube; False when staging is off / unavailable."""
        hc = self._ensure_host_cube(dtype)
        if hc is None:
            return False
        self._ctx.get_vis_async(slot, hc[slot])
        return True

    def set_external_beam(self, beam, beam_freqs_hz, spec_interp='cubic', chromatic=True, select_freq=None):
        """Use a tabulated HEALPix (RING, local zenith-angle/azimuth frame) power beam [npix, nfreq] for all following
        observe() calls that do not pass roi_info (scripts/run_prisim.py:489-494, 2091-2103: interpolation of log10(beam) in
        frequency and on the sphere, per-channel peak normalisation, float32 storage) -- evaluated on the GPU per snapshot."""
        m = PB.spectral_interp_matrix(beam_freqs_hz, self.channels, kind=spec_interp, chromatic=chromatic, select_freq=select_freq)
        self._ctx.set_external_beam(beam, m)
        self._extbeam = (NP.asarray(beam), m)

    def _restore_external_beam(self):
        if getattr(self, '_extbeam', None) is not None:
            self._ctx.set_external_beam(*self._extbeam)

    def comm_setup(self, comm_uid, nranks, rank, selftest=True):
        """Build the RCCL communicator of this array's context (once) and run its self-test: a 1 MiB all-gather of a rank-dependent
        pattern verified on the host of every rank (prisim_hip_comm_selftest), so that a communicator that cannot move data raises HERE
        (PrisimHipError) and not as a silently wrong cube on disk.  Returns True; callers that can talk to the other ranks combine the
        outcomes of the SELF-TEST (driver.run does, over the rendezvous: selftest=False here, then comm_selftest()) so that every rank
        stops when one fails.  comm_init itself is a collective (ncclCommInitRank): a rank whose init fails must END -- its peers are
        inside that collective and only the launcher, seeing the exit, can stop them -- so its error is never swallowed into a vote."""
        if not getattr(self, '_comm_ready', False):
            self._ctx.comm_init(comm_uid, nranks, rank)
            if selftest:
                self._ctx.comm_selftest()
            self._comm_ready = True
        self._apply_shard_map()
        return True

    def set_shard_map(self, bl_index, nbl_total):
        """This array is one baseline shard of a larger array: bl_index (nranks, nbl_shard) = global baseline of every (padded) local row of
        every rank, negative = padding.  With it every gather (allgather, allgather_lags, allgather_gradient, allgather_cube) leaves -- and
        returns -- the cube in the GLOBAL baseline order of the unsharded array, padding dropped, put in order by a copy kernel on the
        receiving GPU (prisim_hip_set_shard_map): the order of the reference's rank-0 concatenate (scripts/run_prisim.py:2233-2242).
        Without it the gathered cubes are rank-major (nranks * nbl_shard rows)."""
        if bl_index is None:
            self._shard_map = None
        else:
            m = NP.ascontiguousarray(bl_index, dtype=NP.int64)
            if m.ndim != 2 or m.shape[1] != self.baselines.shape[0]:
                raise ValueError('bl_index must have shape (nranks, nbl_shard)')
            self._shard_map = (m, int(nbl_total))
        self._shard_map_applied = False
        if getattr(self, '_comm_ready', False):
            self._apply_shard_map()

    def _apply_shard_map(self):
        if getattr(self, '_shard_map_applied', True):
            return
        sm = getattr(self, '_shard_map', None)
        if sm is None:
            self._ctx.set_shard_map(None, 0)
        else:
            self._ctx.set_shard_map(sm[0], sm[1])
        self._shard_map_applied = True

    def _gathered_cube(self, g, nranks, row):
        """The host copy of a gathered cube, baseline axis first like every cube of the class: (rows, row, nt) with rows = nbl_total in
        global order when a shard map is set, nranks * nbl_shard (rank-major) otherwise."""
        nt = g.shape[0]
        if getattr(self, '_shard_map', None) is not None:
            return NP.transpose(g, (1, 2, 0))                         # [t][global baseline][row]
        return NP.transpose(g.reshape(nt, nranks * self.baselines.shape[0], row), (1, 2, 0))

    def comm_selftest(self):
        self._ctx.comm_selftest()

    def allgather(self, comm_uid, nranks, rank, download=True, root=None):
        """One RCCL all-gather of the baseline shards of all ranks (equal shard sizes; replaces the reference's per-rank
        part files + rank-0 concatenate, scripts/run_prisim.py:2207, 2233-2242).  Returns (nranks*nbl, nchan, n_acc) rank-major -- or, with
        set_shard_map(), (nbl_total, nchan, n_acc) in the global baseline order, put in order on the device --, or None with
        download=False (the gathered cube then stays in HBM only: a rank that writes nothing need not pull it over PCIe).
        root = r: this and every later gather of this array (lags, gradients, noise) deliver to rank r ONLY -- the other GPUs keep no
        copy of the whole cube (SURVEY 8(e) gather_to_root); download must then be False everywhere else."""
        if self._reserved < self.n_acc:
            raise RuntimeError('reserve(n_acc) must be called before observing to keep the cube on the device')
        if root is not None and download and rank != root:
            raise ValueError('with root = {0} only that rank can download the gathered cube'.format(root))
        self.comm_setup(comm_uid, nranks, rank)
        self._ctx.set_gather_root(root)
        # complex64 on the wire only when EVERY snapshot was observed with memsave (host arrays and _DeviceSlot placeholders both
        # carry their dtype); a run that mixes precisions, or has no snapshot yet, gathers complex128
        c64 = bool(self._cube) and all(NP.dtype(sn.dtype) == NP.complex64 for sn in self._cube)
        self._ctx.allgather(self.n_acc, complex64=c64)
        if not download:
            return None
        return self._gathered_cube(self._ctx.get_gathered(self.n_acc, nranks), nranks, self.channels.size)      # [t][rank][b][f] | [t][bl][f]

    def allgather_lags(self, nranks, download=True):
        """All-gather of the delay spectra of the baseline shards (the FFT is along frequency, so every rank transforms
        its own shard and the spectra are exchanged like the visibilities).  Call after allgather() and delay_transform().  Spectra
        that delay_transform() left resident on the device go GPU -> GPU (prisim_hip_allgather_lags); host-side spectra take the
        place of the visibilities in the device cube slots for the exchange.  Returns (nranks*nbl, nlag, n_acc)."""
        if not getattr(self, '_comm_ready', False):
            raise RuntimeError('allgather() must be called first (it sets up the communicator)')
        if getattr(self, '_lag_resident', None) is not None:
            g = self._lag_resident.allgather(nranks, download)
            return None if g is None else self._gathered_cube(g, nranks, self._lag_resident.nout)
        if self.skyvis_lag is None:
            raise RuntimeError('delay_transform() must be called first')
        if self.skyvis_lag.shape != (self.baselines.shape[0], self.channels.size, self.n_acc):
            raise NotImplementedError('host-side delay spectra are exchanged through the visibility slots: this needs nlag == nchan (pad = 0, 1, 2, ...)')
        return self.allgather_cube(self.skyvis_lag, nranks, download=download)

    def allgather_gradient(self, nranks, download=True):
        """All-gather of the baseline-gradient cubes of the shards (gradient_mode='baseline'): the reference concatenates them over the
        baseline chunks (interferometry.py:8349-8350).  The gradient blocks observe() left in the device gradient cube go GPU -> GPU
        (prisim_hip_allgather_grad).  Call after allgather().  Returns (3, nranks*nbl, nchan, n_acc), or None with download=False."""
        if not getattr(self, '_comm_ready', False):
            raise RuntimeError('allgather() must be called first (it sets up the communicator)')
        if self.gradient_mode is None or len(self._grad) != self.n_acc:
            raise RuntimeError('every snapshot must have been observed with gradient_mode set')
        if self._reserved < self.n_acc:
            raise RuntimeError('reserve(n_acc) must be called before observing to keep the gradient cube on the device')
        c64 = all(NP.dtype(g.dtype) == NP.complex64 for g in self._grad)
        self._ctx.allgather_grad(self.n_acc, complex64=c64)
        if not download:
            return None
        g = self._ctx.get_gathered_grad(self.n_acc, nranks)             # [t][rank][k][b][f], or [t][k][global baseline][f] with a shard map
        if getattr(self, '_shard_map', None) is not None:
            return NP.transpose(g, (1, 2, 3, 0))
        nbl, nchan = self.baselines.shape[0], self.channels.size
        return NP.transpose(g, (2, 1, 3, 4, 0)).reshape(3, nranks * nbl, nchan, self.n_acc)

    def allgather_cube(self, cube, nranks, download=True):
        """All-gather of a host-side (nbl, nchan, n_acc) cube of this shard that has no device copy (the thermal noise, host-side delay
        spectra): it takes the place of the visibilities in the device cube slots for the exchange, and the visibilities go back afterwards.
        Call after allgather().  Returns (nranks*nbl, nchan, n_acc), or None with download=False."""
        if not getattr(self, '_comm_ready', False):
            raise RuntimeError('allgather() must be called first (it sets up the communicator)')
        cube = NP.asarray(cube)
        if cube.shape != (self.baselines.shape[0], self.channels.size, self.n_acc):
            raise ValueError('cube must have the shape of the visibility cube (nbl, nchan, n_acc)')
        _ = self.skyvis_freq                                           # make sure the host owns the visibilities before their slots are reused
        for t in range(self.n_acc):
            self._ctx.set_vis(NP.ascontiguousarray(cube[:, :, t], dtype=NP.complex128), slot=t)
        self._ctx.allgather(self.n_acc, complex64=False)
        g = self._ctx.get_gathered(self.n_acc, nranks) if download else None
        for t in range(self.n_acc):                                    # and the visibilities go back into their slots
            self._ctx.set_vis(NP.asarray(self.skyvis_freq[:, :, t], dtype=NP.complex128), slot=t)
        if g is None:
            return None
        return self._gathered_cube(g, nranks, self.channels.size)

    # ------------------------------------------------------------------------------------------
    def _broadcast_bl_chan(self, value, what, lo, hi):
        nbl, nchan = self.baselines.shape[0], self.channels.size
        if isinstance(value, (int, float)):
            if value < lo or (hi is not None and value > hi):
                raise ValueError('{0} value of interferometer is invalid.'.format(what))
            return value * NP.ones((nbl, nchan))
        elif isinstance(value, (list, tuple, NP.ndarray)):
            value = NP.asarray(value)
            if NP.any(value < lo) or (hi is not None and NP.any(value > hi)):
                raise ValueError('One or more values of {0} found to be outside the valid range.'.format(what))
            if value.size == nbl:
                return NP.repeat(value.reshape(-1, 1), nchan, axis=1)
            elif value.size == nchan:
                return NP.repeat(value.reshape(1, -1), nbl, axis=0)
            elif value.size == nbl * nchan:
                return value.reshape(-1, nchan)
            raise ValueError('{0} values of interferometers incompatible with the number of interferometers and/or '
                             'frequency channels.'.format(what))
        raise TypeError('{0} values of interferometers must be provided as a scalar, list, tuple or numpy array.'.format(what))

    # ------------------------------------------------------------------------------------------
    def _bandpass_layer(self, bandpass):
        """The bandpass layer of one snapshot, checked (interferometry.py:5993-6018)."""
        bandpass = NP.asarray(bandpass)
        nbl, nchan = self.baselines.shape[0], self.channels.size
        if bandpass.ndim == 1:
            if bandpass.size != nchan:
                raise ValueError('Specified bandpass incompatible with the number of frequency channels')
            layer = bandpass.reshape(1, -1)                                # one row for every baseline (dense on read)
        elif bandpass.ndim == 2:
            if bandpass.shape[1] != nchan:
                raise ValueError('Specified bandpass incompatible with the number of frequency channels')
            elif bandpass.shape[0] != nbl:
                raise ValueError('Specified bandpass incompatible with the number of interferometers')
            layer = bandpass
        elif bandpass.ndim == 3:
            if bandpass.shape[1] != nchan:
                raise ValueError('Specified bandpass incompatible with the number of frequency channels')
            elif bandpass.shape[0] != nbl:
                raise ValueError('Specified bandpass incompatible with the number of interferometers')
            elif bandpass.shape[2] != 1:
                raise ValueError('Bandpass can have only one layer for this instance of accumulation.')
            layer = bandpass
        else:
            raise ValueError('Specified bandpass has too many dimensions')
        return layer

    def _tsys_layer(self, Tsysinfo, bpcorrect):
        """The system-temperature layer of one snapshot, checked (interferometry.py:6026-6081)."""
        nbl, nchan = self.baselines.shape[0], self.channels.size
        if not isinstance(Tsysinfo, dict):
            raise TypeError('Input Tsysinfo must be a dictionary')
        Tsys = None
        if Tsysinfo.get('Tnet', None) is not None:
            Tsys = Tsysinfo['Tnet']
        else:
            try:
                Tsys = Tsysinfo['Trx'] + Tsysinfo['Tant']['T0'] * (self.channels / Tsysinfo['Tant']['f0']) ** Tsysinfo['Tant']['spindex']
            except KeyError:
                raise KeyError('One or more keys not found in input Tsysinfo')
            Tsys = Tsys.reshape(1, -1)                                     # one row for every baseline (:6046; dense on read)
        if bpcorrect is not None:
            if not isinstance(bpcorrect, NP.ndarray):
                raise TypeError('Input specifying bandpass correction must be a numpy array')
            if bpcorrect.size == nchan:
                bpcorrect = bpcorrect.reshape(1, -1)
            elif bpcorrect.size == nbl:
                bpcorrect = bpcorrect.reshape(-1, 1)
            elif bpcorrect.size == nbl * nchan:
                bpcorrect = bpcorrect.reshape(-1, nchan)
            else:
                raise ValueError('Input bpcorrect has dimensions incompatible with the number of baselines and frequencies')
            Tsys = Tsys * bpcorrect
        if isinstance(Tsys, (int, float)):
            if Tsys < 0.0:
                raise ValueError('Tsys found to be negative.')
            layer = NP.full((1, 1), float(Tsys))
        elif isinstance(Tsys, (list, tuple, NP.ndarray)):
            Tsys = NP.asarray(Tsys)
            if NP.any(Tsys < 0.0):
                raise ValueError('Tsys should be non-negative.')
            if Tsys.size == 1:
                layer = NP.full((1, 1), float(Tsys.ravel()[0]))
            elif Tsys.shape == (1, nchan) or (Tsys.size == nchan and Tsys.size != nbl):
                layer = Tsys.reshape(1, -1)
            elif Tsys.size == nbl:                                        # (as in the reference, nbl wins when nbl == nchan)
                layer = Tsys.reshape(-1, 1)
            elif Tsys.size == nchan:
                layer = Tsys.reshape(1, -1)
            elif Tsys.size == nbl * nchan:
                layer = Tsys.reshape(-1, nchan)
            else:
                raise ValueError('Specified Tsys has incompatible dimensions with the number of baselines and/or number of frequency channels.')
        else:
            raise TypeError('Tsys should be a scalar, list, tuple, or numpy array')
        return layer

    # ------------------------------------------------------------------------------------------
    # ------------------------------------------------------------------------------------------
    # Device-resident catalogue (prisim_hip_set_catalog, ABI 0.4).  The reference re-derives the sky at every observe() from a sky
    # model that does not change over a run (scripts/run_prisim.py:2165-2207; interferometry.py:6223-6247 store_prev_skymodel_file
    # exists because that is expensive).  Here the model is uploaded the first time it is seen and every later snapshot's
    # hadec -> altaz -> dircos, region of interest, flux spectra and beam x flux are formed on the GPU.

    def _catalog_fingerprint(self, skymodel):
        """What decides whether the catalogue resident on the device still IS this sky model: identity of the object and the CONTENT of
        everything that was uploaded (an in-place edit -- ``skymodel.flux_ref *= 2`` between two observe() calls, a Monte-Carlo loop over
        realisations -- must be seen; the reference re-reads the sky model at every call).  One pass of sums over the nsrc-sized vectors
        (a microsecond or two per 1e4 sources each) and over a strided sample of a spectrum table."""
        def digest(a, sample=False):
            # ONE integer reduction over the BIT PATTERNS (a wrapping 64-bit sum: any edit that is not an exchange of values moves it): exact, NaN-safe, and a plain numpy
            # loop -- NOT a BLAS dot product: OpenBLAS answers a 1e5-element dot with every core it sees (64 threads on a box whose cgroup
            # grants 16), and the scheduler then throttles the whole process for tens of milliseconds at a time -- measured: a config-4 shard
            # through observe_batch went from 1.04 to 1.2-1.8 x the kernel-only time with a dot product here.
            if a is None:
                return None
            if type(a) is not NP.ndarray:
                a = NP.asarray(a)
            if a.dtype != NP.float64:
                if a.dtype.kind not in 'fiu':
                    return (a.shape, str(a.dtype))
                a = a.astype(NP.float64)
            flat = a.reshape(-1)
            if sample and flat.size > (1 << 20):          # a spectrum table: 65536 evenly spaced samples (plus the shape) instead of gigabytes
                flat = flat[::flat.size // (1 << 16)]
            if not flat.flags.c_contiguous:
                flat = NP.ascontiguousarray(flat)
            u = flat.view(NP.uint64)
            return (a.shape, int(NP.add.reduce(u)))
        def g(k):
            return getattr(skymodel, k, None)      # (attributes, class-level defaults and properties alike)
        ref_freq = g('ref_freq')
        frozen = getattr(skymodel, '_frozen', None)
        if frozen is not None:
            # prisim_amd.skymodel.SkyModel.freeze(): the arrays are private read-only copies -- their identity stands for their content (the key
            # holds them, so no identity can be reused); anything assigned or made writeable since falls through to the content pass
            cur = (g('location'), g('flux_ref'), g('spindex'), g('spectrum'), g('frequency'), g('src_shape'))
            if len(frozen) == len(cur) and all(c is f and (c is None or not c.flags.writeable) for c, f in zip(cur, frozen)):
                return (id(skymodel), self.skycoords, g('spec_type'), _SameObject(frozen), None if ref_freq is None else float(NP.sum(ref_freq)),
                        self.channels.size, float(self.channels[0]), float(self.channels[-1]), self._reserved)
        return (id(skymodel), self.skycoords, g('spec_type'), digest(skymodel.location), digest(g('flux_ref')), digest(g('spindex')),
                None if ref_freq is None else float(NP.sum(ref_freq)), digest(g('spectrum'), sample=True), digest(g('frequency')),
                digest(g('src_shape')), self.channels.size, float(self.channels[0]), float(self.channels[-1]), self._reserved)

    def close(self):
        """Release the GPU context.  Class state that still lives on the device is fetched first: obs_catalog_indices / geometric_delays of
        snapshots formed from the resident catalogue, snapshots and gradient blocks parked in device slots."""
        if getattr(self, '_ctx', None) is None:
            return
        self._materialise_catalog_state()
        if getattr(self, '_cube', None):
            self.skyvis_freq
        if isinstance(self.gradient, _LazyGradients) and self.gradient_mode is not None:
            self.gradient.get(self.gradient_mode)
        self._ctx.close()

    def invalidate_catalog(self):
        """Forget the sky model resident on the device: the next observe() uploads it again (for edits the fingerprint cannot see,
        e.g. a custom generate_spectrum whose parameters changed), and try again one that was refused for want of device memory."""
        self._materialise_catalog_state()
        self._catalog_key = None
        self._catalog_refused = None

    def _refuse_catalog(self, skymodel, message):
        """`skymodel` does not fit on the device as a resident catalogue: it takes the per-snapshot upload path (ROI rows only) until
        invalidate_catalog() or until it is collected.  (An object that cannot be referenced weakly is tried again at its next call.)"""
        warnings.warn(message)
        try:
            self._catalog_refused = weakref.ref(skymodel)
        except TypeError:
            self._catalog_refused = None
        self._materialise_catalog_state()

    def _catalog_ready(self, skymodel):
        """True when `skymodel` is (now) the catalogue resident on the device.  PRISIM_CATALOG=0 switches the path off (A/B: every
        snapshot's sky is then formed on the host and uploaded, as before round 5)."""
        if os.environ.get('PRISIM_CATALOG', '1') == '0' or not hasattr(self._ctx, 'set_catalog'):
            return False
        key = self._catalog_fingerprint(skymodel)
        if getattr(self, '_catalog_key', None) == key:
            return True
        refused = getattr(self, '_catalog_refused', None)
        if refused is not None and refused() is skymodel:
            return False                               # this sky model ran out of device memory on the resident path
        self._materialise_catalog_state()              # lazy class state of the previous catalogue is fetched while it is still there
        location = NP.asarray(skymodel.location, dtype=NP.float64).reshape(-1, 2)
        nsrc, nchan = location.shape[0], self.channels.size
        fwhm = None
        src_shape = getattr(skymodel, 'src_shape', None)
        if src_shape is not None:                                                      # :6258, 6267
            src_shape = NP.asarray(src_shape, dtype=NP.float64)
            fwhm = NP.sqrt(src_shape[:, 0] * src_shape[:, 1])
        powerlaw = (getattr(skymodel, 'spec_type', None) == 'func' and all(hasattr(skymodel, a) for a in ('flux_ref', 'spindex', 'ref_freq')))
        try:
            if powerlaw:
                self._ctx.set_catalog(location, self.skycoords, flux_ref=skymodel.flux_ref, spindex=skymodel.spindex,
                                      ref_freq_hz=float(skymodel.ref_freq), fwhm_deg=fwhm)
            else:
                if nsrc * nchan * 8 > (16 << 30):
                    return False                       # a spectrum table this large stays on the per-snapshot path (ROI rows only)
                spectra = NP.asarray(skymodel.generate_spectrum(ind=NP.arange(nsrc), frequency=self.channels, interp_method='pchip'),
                                     dtype=NP.float64).reshape(-1, nchan)              # :6249, once for the whole catalogue
                self._ctx.set_catalog(location, self.skycoords, flux_spectrum=spectra, fwhm_deg=fwhm)
        except MemoryError:
            self._refuse_catalog(skymodel, 'the sky model does not fit on the device as a resident catalogue; it takes the per-snapshot '
                                           'upload path')
            return False
        self._catalog_key = key
        self._catalog_obs_cache = None
        return True

    def _catalog_obs(self, pb_info, pc_altaz, roi_radius, roi_center):
        """(prisim_obs, beam pointing direction cosines) of a snapshot.  The struct is cached while nothing it depends on changes."""
        if getattr(self, '_extbeam', None) is not None:
            key = ('ext', roi_radius, roi_center, self.latitude)
            cache = getattr(self, '_catalog_obs_cache', None)
            if cache is None or cache[0] != key:
                cache = (key, self._ctx.make_obs(self.latitude, roi_radius, roi_center, use_external_beam=True))
                self._catalog_obs_cache = cache
            return cache[1], None
        if pb_info is None:
            skey = (id(self.telescope), float(pc_altaz[0]), float(pc_altaz[1]))
            spec = getattr(self, '_beam_spec_cache', None)
            if spec is None or spec[0] != skey:
                spec = (skey, PB.device_beam_spec(self.telescope, pointing_info=None, pointing_center=pc_altaz,
                                                  first_frequency_hz=float(self.channels[0])))                  # :6252
                self._beam_spec_cache = spec
            kind, dia, bpc, ext = spec[1]
        else:
            kind, dia, bpc, ext = PB.device_beam_spec(self.telescope, pointing_info=pb_info, pointing_center=pc_altaz,
                                                      first_frequency_hz=float(self.channels[0]))
        if pb_info is not None or (ext is not None and 'beamformer' in ext):
            return self._ctx.make_obs(self.latitude, roi_radius, roi_center, beam_kind=kind, diameter_m=dia, ext=ext), bpc
        key = (kind, dia, id(self.telescope), roi_radius, roi_center, self.latitude)
        cache = getattr(self, '_catalog_obs_cache', None)
        if cache is None or cache[0] != key:
            cache = (key, self._ctx.make_obs(self.latitude, roi_radius, roi_center, beam_kind=kind, diameter_m=dia, ext=ext))
            self._catalog_obs_cache = cache
        return cache[1], bpc

    def _materialise_catalog_state(self):
        """Fetch the lazy per-snapshot class state that lives in the device-resident catalogue (obs_catalog_indices, the direction
        cosines behind geometric_delays) before the catalogue goes away: a new sky model, or set_array (reserve, conjugate ...)."""
        for entry in getattr(self, 'obs_catalog_indices', []):
            if isinstance(entry, _CatalogROI):
                entry.fetch()
        self._catalog_key = None

    def _snapshot_frame(self, jd, lst, skymodel):
        """(R, beta) of one snapshot: catalogue frame of `skymodel` -> local East, North, Up (interferometry.py:6174-6180; prisim_amd/frames.py).
        The same pair goes to the device (prisim_snapshot.cel2enu / aberr_beta) and to the host path (geometry.frame_dircos)."""
        if self.frame_provider is not None and self.skycoords == 'radec':
            rot, beta = self.frame_provider(jd, lst, skymodel)
            return NP.asarray(rot, dtype=NP.float64).reshape(3, 3), NP.asarray(beta, dtype=NP.float64).reshape(3)
        key = (self.skycoords, float(lst), float(self.latitude), float(jd), getattr(skymodel, 'epoch', None), self.frame_model)
        cache = getattr(self, '_frame_cache', None)
        if cache is None or cache[0] != key:
            cache = (key, FRAMES.snapshot_frame(self.skycoords, lst, self.latitude, jd=jd, epoch=getattr(skymodel, 'epoch', None),
                                                model=self.frame_model))
            self._frame_cache = cache
        return cache[1]

    @staticmethod
    def _check_gradient_mode(gradient_mode):
        if gradient_mode is not None:                                                 # :6306-6311
            if not isinstance(gradient_mode, str):
                raise TypeError('Input gradient_mode must be a string')
            if gradient_mode.lower() not in ['baseline', 'skypos', 'frequency']:
                raise ValueError('Invalid value specified in input gradient_mode')
            if gradient_mode.lower() != 'baseline':
                raise NotImplementedError('only gradient_mode="baseline" is computed (as in the reference)')
        return gradient_mode is not None

    @staticmethod
    def _check_skymodel(skymodel):
        for attr in ('location', 'generate_spectrum'):                                 # :6171 (duck-typed SkyModel)
            if not hasattr(skymodel, attr):
                raise TypeError('skymodel should be an instance of class SkyModel.')

    def _pointing(self, pointing_center, lst):
        """Pointing = phase centre of one snapshot (:6103-6108, 6155-6164): (its row of pointing_center, alt-az degrees, ENU direction
        cosines)."""
        pc = NP.asarray(pointing_center, dtype=NP.float64).reshape(-1)
        if pc.size != 2:
            raise ValueError('pointing_center must be a 2-element vector')
        # (a drift scan points at one (HA, Dec) for hours: the conversion of the previous snapshot is kept while nothing it depends on changes)
        key = (self.pointing_coords, float(pc[0]), float(pc[1]), lst if self.pointing_coords == 'radec' else None, self.latitude)
        cache = getattr(self, '_pointing_cache', None)
        if cache is not None and cache[0] == key:
            return pc, cache[1], cache[2]
        pc_altaz = pc                                                                 # :6155-6162
        if self.pointing_coords == 'hadec':
            pc_altaz = GEOM.hadec2altaz(pc, self.latitude, units='degrees')
        elif self.pointing_coords == 'radec':
            pc_altaz = GEOM.hadec2altaz(NP.asarray([lst - pc[0], pc[1]]), self.latitude, units='degrees')
        pc_altaz = NP.array(pc_altaz, dtype=NP.float64)
        pc_dircos = GEOM.altaz2dircos(pc_altaz, 'degrees').ravel()                    # :6164
        self._pointing_cache = (key, pc_altaz, pc_dircos)
        return pc, pc_altaz, pc_dircos

    def _snapshot_inputs(self, timeobj, Tsysinfo, bandpass, pointing_center, bpcorrect, lst=None):
        """One snapshot's inputs, checked in the reference's order and appended nowhere: (bandpass layer, Tsysinfo, Tsys layer, jd, lst,
        pointing row, pointing alt-az, pointing direction cosines)."""
        bp = self._bandpass_layer(bandpass)
        tsys = self._tsys_layer(Tsysinfo, bpcorrect)
        jd, lst = _lst_and_jd(timeobj, lst)                                           # :6113
        return (bp, Tsysinfo, tsys, jd, lst) + self._pointing(pointing_center, lst)

    def _commit(self, snaps, t_acc, sels, vis, grads, slot0, gradient_mode, memsave):
        """Append observed snapshots to every per-snapshot attribute -- the only place observe() and observe_batch() change them, after
        the device has answered, so that a call that fails leaves the instance as it was.  snaps: _snapshot_inputs() of each; sels: the
        (index list, direction cosines) of each snapshot's region of interest, or None when it was empty on the upload path (the
        reference then appends no index list and no delays, :6377-6382); vis / grads: host arrays or _DeviceSlot; slot0: the device
        slot of the first."""
        for sel in sels:
            if sel is None or len(sel[0]) == 0:                                      # :6378-6382 (the device slot holds zeros)
                warnings.warn('No sources found in the catalog within matching radius. Simply populating the observed visibilities and/or gradients with noise.')
        n, k = self.n_acc, len(snaps)
        self._device_in_step = slot0 == n and (n == 0 or getattr(self, '_device_in_step', False))
        base_bl = self._baselines_local()
        for (bp, tsysinfo, tsys, jd, lst, _, _, _), tacc, sel in zip(snaps, t_acc, sels):
            self._append_layer('bp', bp)                                              # :6019-6022
            self._append_layer('Tsys', tsys)                                          # :6082-6086
            self.Tsysinfo.append(tsysinfo)
            if sel is not None:
                self.geometric_delays.append(LazyGeometricDelays(base_bl, sel[1], NP.float32 if memsave else NP.float64))   # :6287-6291
                self.obs_catalog_indices.append(sel[0])                               # :6377
            self.timestamp.append(jd)                                                 # :6395-6399
            self.t_acc.append(tacc)
            self.t_obs += tacc
            self.lst.append(lst)
        if self._stacks.get('bp') is not None:                                        # :6024
            cur = self._stacks.get('bp_wts')
            if not (isinstance(cur, _OnesStack) and cur.parent is self._stacks['bp']):
                self._stacks['bp_wts'] = self._stacks['bp'].ones_like()
            self._dense.pop('bp_wts', None)
        else:
            self.bp_wts = NP.ones_like(self.bp)
        # pointing_center / phase_center are (n_acc, 2) arrays like the reference's (:6103-6108, grown there by NP.vstack: O(n) per
        # snapshot); here both are views of buffers that grow by doubling
        for name in ('pointing_center', 'phase_center'):
            cur = getattr(self, name)
            buf = self.__dict__.get('_buf_' + name)
            if n == 0 or buf is None or cur.base is not buf or cur.shape[0] != n or buf.shape[0] < n + k:
                newbuf = NP.empty((max(16, 2 * (n + k)), 2))
                if n > 0:
                    newbuf[:n] = NP.asarray(cur, dtype=NP.float64).reshape(-1, 2)[:n]
                buf = self.__dict__['_buf_' + name] = newbuf
            buf[n:n + k] = [s[5] for s in snaps]
            setattr(self, name, buf[:n + k])
        self._cube.extend(vis)                                                        # :6384-6393
        self._skyvis_cache = None
        if gradient_mode is not None:
            self._grad.extend(grads)
            if self.gradient_mode is None:
                self.gradient_mode = gradient_mode
            if not isinstance(self.gradient, _LazyGradients):
                self.gradient = _LazyGradients(self)
            self.gradient.invalidate(gradient_mode)                                   # stacked again when it is next read
        self.n_acc += k

    def _unpark(self, slot):
        """Fetch whatever snapshot (and gradient block) still lives only in device slot `slot` before the slot is overwritten."""
        for i, snap in enumerate(self._cube):
            if isinstance(snap, _DeviceSlot) and snap.slot == slot:
                self._cube[i] = self._ctx.get_vis(slot=slot, complex64=(snap.dtype == NP.complex64))
        for i, g in enumerate(self._grad):
            if isinstance(g, _DeviceSlot) and g.slot == slot:
                self._grad[i] = self._ctx.get_vis(slot=slot, want_grad=True, complex64=(g.dtype == NP.complex64))[1]

    @staticmethod
    def _roi_defaults(roi_radius, roi_center):
        if roi_radius is None:                                                        # :6204-6216
            roi_radius = 90.0
        if roi_center is None:
            roi_center = 'zenith'
        elif (roi_center != 'zenith') and (roi_center != 'pointing_center'):
            raise ValueError('Center of region of interest, roi_center, must be set to "zenith" or "pointing_center".')
        return roi_radius, roi_center

    def observe(self, timeobj, Tsysinfo, bandpass, pointing_center, skymodel,
                t_acc, pb_info=None, brightness_units=None, bpcorrect=None,
                roi_info=None, roi_radius=None, roi_center=None, lst=None,
                gradient_mode=None, memsave=False, vmemavail=None,
                store_prev_skymodel_file=None):
        """Simulate one snapshot (interferometry.py:5874-6410).  See the reference docstring for the
        argument meaning; vmemavail is accepted and ignored (the GPU kernel never materialises the nsrc x nbl x nchan matrix, so there
        is no memory-shortage path).  store_prev_skymodel_file (:6223-6247: the previous call's sky on disk, so that an unchanged sky
        is not re-derived) is accepted too: what it buys is had without a file -- the sky model handed in stays resident on the GPU
        from the first call that sees it, and every later snapshot's geometry, region of interest and beam x flux are formed there
        (prisim_hip_set_catalog / prisim_hip_observe_catalog)."""
        snap = self._snapshot_inputs(timeobj, Tsysinfo, bandpass, pointing_center, bpcorrect, lst)
        self._check_skymodel(skymodel)
        self._check_gradient_mode(gradient_mode)
        self._observe_snapshot(snap, skymodel, t_acc, pb_info, roi_info, roi_radius, roi_center, gradient_mode, memsave)

    def _observe_snapshot(self, snap, skymodel, t_acc, pb_info, roi_info, roi_radius, roi_center, gradient_mode, memsave):
        """One snapshot of checked inputs through the device -- from the resident catalogue, else formed on the host and uploaded --
        and committed."""
        jd, lst, pc_altaz, pc_dircos = snap[3], snap[4], snap[6], snap[7]
        nbl, nchan = self.baselines.shape[0], self.channels.size
        datatype = NP.complex64 if memsave else NP.complex128                         # :6182-6185
        want_grad = gradient_mode is not None
        prec = _abi.PRISIM_FP32 if memsave else _abi.PRISIM_FP64
        slot = self.n_acc if self.n_acc < self._reserved else 0

        frame = self._snapshot_frame(jd, lst, skymodel)                               # :6174-6180 as one rotation + aberration vector
        sel = None
        if roi_info is None and self._catalog_ready(skymodel):
            # ---- the sky model is resident on the device: geometry, ROI, spectra, beam x flux and the sky-sum in ONE call ----
            roi_radius, roi_center = self._roi_defaults(roi_radius, roi_center)
            obs, bpc = self._catalog_obs(pb_info, pc_altaz, roi_radius, roi_center)
            if slot != self.n_acc:
                self._unpark(slot)
            try:
                nroi = int(self._ctx.observe_catalog(obs, [lst], pc_dircos, bpc, precision=prec, want_grad=want_grad, slot0=slot,
                                                     frames=[frame])[0])
            except MemoryError:
                # the resident path sizes its beam x flux for a whole chunk of snapshots; a catalogue that ran through the per-snapshot
                # upload before must still run: drop the resident copy and take that path (ROI rows only)
                self._refuse_catalog(skymodel, _CATALOG_OOM)
            else:
                roi = _CatalogROI(self, obs, lst, pc_dircos, nroi, frame)
                sel = (roi, roi)
        if sel is None:
            sel = self._upload_snapshot_sky(skymodel, frame, pc_altaz, pc_dircos, pb_info, roi_info, roi_radius, roi_center)
            if sel is not None:
                if slot != self.n_acc:                                   # (a fresh reserved slot holds nothing: no O(n_acc) scan per snapshot)
                    self._unpark(slot)
                self._ctx.compute(precision=prec, want_grad=want_grad, slot=slot)

        if sel is None:                                                               # :6378-6382
            skyvis = NP.zeros((nbl, nchan), dtype=datatype)
            skyvis_gradient = NP.zeros((3, nbl, nchan), dtype=datatype) if want_grad else None
            if slot == self.n_acc:                                                    # the snapshot's device slot says the same
                self._ctx.set_vis(NP.zeros((nbl, nchan), dtype=NP.complex128), slot=slot)
        elif slot == self.n_acc:
            # the snapshot stays in its own slot of the device cube: no synchronous download (1 GB and 20 ms per HERA-350
            # snapshot; 4 GB with the gradient blocks); with host staging its copy to the pinned host cube is queued behind the
            # sky-sum, on the copy stream.  The gradient blocks stay in the device gradient cube until `gradient` is read.
            skyvis = _DeviceSlot(slot, datatype, staged=self._stage_download(slot, datatype))
            skyvis_gradient = _DeviceSlot(slot, datatype) if want_grad else None
        else:
            res = self._ctx.get_vis(slot=slot, want_grad=want_grad, complex64=memsave)
            skyvis, skyvis_gradient = res if want_grad else (res, None)
        self._commit([snap], [t_acc], [sel], [skyvis], [skyvis_gradient], slot, gradient_mode, memsave)

    def observe_batch(self, timeobjs, Tsysinfo, bandpass, pointing_centers, skymodel, t_acc, pb_info=None, bpcorrect=None,
                      roi_radius=None, roi_center=None, gradient_mode=None, memsave=False):
        """K snapshots of ONE sky model in one call -- what the reference's callers write as a loop over observe()
        (scripts/run_prisim.py:2165-2207, interferometry.py:6641-6647).  Not in the reference.  With the sky model resident on the
        device the geometry of all K snapshots is formed first (one small read-back for the lot) and their skies and sky-sums are then
        queued back to back without a host synchronisation; arrays of at most 256 baselines put the K sky-sums into ONE launch
        (prisim_hip_observe_catalog).  The class state afterwards is what K calls of observe() leave.

        timeobjs          K time objects as observe() takes them ((jd, lst_deg) pairs, Time-likes ...)
        Tsysinfo          one dictionary for every snapshot, or a list of K
        bandpass          (nchan,) / (nbl, nchan) for every snapshot, or a list of K
        pointing_centers  (2,) for every snapshot or (K, 2)
        t_acc             scalar or K values
        The inputs of all K snapshots are checked before anything runs.  Falls back to one snapshot after the other, as observe() runs
        them, when the catalogue path is not available (PRISIM_CATALOG=0, no free device slots)."""
        k = len(timeobjs)
        if k == 0:
            return
        tsys_l = Tsysinfo if isinstance(Tsysinfo, (list, tuple)) else [Tsysinfo] * k
        bp_l = bandpass if isinstance(bandpass, (list, tuple)) else [bandpass] * k
        pcs = NP.broadcast_to(NP.asarray(pointing_centers, dtype=NP.float64).reshape(-1, 2), (k, 2))
        tacc_l = [float(v) for v in NP.broadcast_to(NP.asarray(t_acc, dtype=NP.float64).ravel(), (k,))]
        if len(tsys_l) != k or len(bp_l) != k:
            raise ValueError('Tsysinfo / bandpass lists must have one entry per snapshot')
        self._check_skymodel(skymodel)
        snaps = [self._snapshot_inputs(timeobjs[t], tsys_l[t], bp_l[t], pcs[t], bpcorrect) for t in range(k)]
        want_grad = self._check_gradient_mode(gradient_mode)
        if self.n_acc == 0 and self._reserved < k:
            self.reserve(k, host_staging=getattr(self, '_stage', False))
        if self.n_acc + k <= self._reserved and (pb_info is None) and self._catalog_ready(skymodel):
            roi_radius, roi_center = self._roi_defaults(roi_radius, roi_center)
            datatype = NP.complex64 if memsave else NP.complex128
            bpcs, frames, obs = [], [], None
            for s in snaps:
                o, bpc = self._catalog_obs(None, s[6], roi_radius, roi_center)
                obs = o if obs is None else obs
                if o is not obs:
                    raise RuntimeError('the beam specification changed inside a batch')
                bpcs.append(s[7] if bpc is None else bpc)
                frames.append(self._snapshot_frame(s[3], s[4], skymodel))
            slot0 = self.n_acc
            host_cube = self._ensure_host_cube(datatype) if getattr(self, '_stage', False) else None
            try:
                counts = self._ctx.observe_catalog(obs, [s[4] for s in snaps], NP.asarray([s[7] for s in snaps]), NP.asarray(bpcs),
                                                   precision=_abi.PRISIM_FP32 if memsave else _abi.PRISIM_FP64, want_grad=want_grad,
                                                   slot0=slot0, host_cube=host_cube, frames=frames)
            except MemoryError:
                self._refuse_catalog(skymodel, _CATALOG_OOM)      # the snapshots below take the per-snapshot upload path (ROI rows only)
            else:
                rois = [_CatalogROI(self, obs, s[4], s[7], int(c), f) for s, c, f in zip(snaps, counts, frames)]
                self._commit(snaps, tacc_l, [(r, r) for r in rois], [_DeviceSlot(slot0 + t, datatype, host_cube is not None) for t in range(k)],
                             [_DeviceSlot(slot0 + t, datatype) for t in range(k)], slot0, gradient_mode, memsave)
                return
        for t in range(k):
            self._observe_snapshot(snaps[t], skymodel, tacc_l[t], pb_info, None, roi_radius, roi_center, gradient_mode, memsave)

    def _upload_snapshot_sky(self, skymodel, frame, pc_altaz, pc_dircos, pb_info, roi_info, roi_radius, roi_center):
        """The snapshot's sky formed on the HOST and uploaded (roi_info given, PRISIM_CATALOG=0, or a spectrum table too large to keep
        resident): interferometry.py:6171-6283 statement by statement, with the astropy / GEOM coordinate chain of :6174-6180 as the
        snapshot's frame (R, beta) applied by geometry.frame_dircos -- the host statement of the device's cat_source().  Returns the region
        of interest as (catalogue indices, direction cosines), or None when it is empty."""
        nchan = self.channels.size
        location = NP.asarray(skymodel.location, dtype=NP.float64).reshape(-1, 2)
        dc_all = GEOM.frame_dircos(GEOM.catalog_unitvec(location, self.skycoords), frame[0], frame[1])     # :6174-6180, 6263
        pb = None
        if roi_info is not None:                                                      # :6189-6202
            if ('ind' not in roi_info) or ('pbeam' not in roi_info):
                raise KeyError('Both "ind" and "pbeam" keys must be present in dictionary roi_info')
            m2 = NP.arange(0)
            if (roi_info['ind'] is not None) and (roi_info['pbeam'] is not None):
                m2 = NP.asarray(roi_info['ind']).ravel()
                if m2.size > 0:
                    try:
                        pb = NP.asarray(roi_info['pbeam']).reshape(-1, nchan)
                    except ValueError:
                        raise ValueError('Number of columns of primary beam in key "pbeam" of dictionary roi_info must be equal to number of frequency channels.')
                    if m2.size != pb.shape[0]:
                        raise ValueError('Values in keys ind and pbeam in must carry same number of elements.')
        else:                                                                         # :6204-6216
            roi_radius, roi_center = self._roi_defaults(roi_radius, roi_center)
            m2 = GEOM.roi_select(dc_all, roi_center, roi_radius, pc_dircos)       # :6210-6216 on the direction cosines
        if len(m2) == 0:
            return None
        dircos_roi = dc_all[m2, :]                                                # :6219, 6263 (unconditional, Q4)
        # flux spectra (:6249).  A power-law sky model (spec_type 'func') is described to the device by its nsrc-sized
        # flux_ref / spindex vectors and S = flux_ref (f / ref_freq)^spindex is formed there; anything else goes through
        # generate_spectrum on the host, as in the reference.
        powerlaw = (getattr(skymodel, 'spec_type', None) == 'func' and pb is None
                    and all(hasattr(skymodel, a) for a in ('flux_ref', 'spindex', 'ref_freq')))
        if powerlaw:
            fluxes = None
            flux_ref = NP.asarray(skymodel.flux_ref, dtype=NP.float64)[m2]
            spindex = NP.asarray(skymodel.spindex, dtype=NP.float64)[m2]
            ref_freq = float(skymodel.ref_freq)
        else:
            fluxes = NP.asarray(skymodel.generate_spectrum(ind=m2, frequency=self.channels, interp_method='pchip'),
                                dtype=NP.float64).reshape(-1, nchan)
            flux_ref = spindex = ref_freq = None
        fwhm = None
        src_shape = getattr(skymodel, 'src_shape', None)
        if src_shape is not None:                                                 # :6258, 6267
            src_shape = NP.asarray(src_shape, dtype=NP.float64)
            fwhm = NP.sqrt(src_shape[m2, 0] * src_shape[m2, 1])
        # Upload order.  The sum over sources does not care about their order, the taper culling of the library does: for every
        # baseline group it skips the LEADING sources of a run of one source size whose weight is provably below the tolerance,
        # and those are the sources nearest the zenith (long baselines resolve them out: b_perp ~ |b|).  So when anything can be
        # culled at all -- kappa_max (|b|_max f_min / c)^2 >= 18 -- each run is listed by decreasing altitude.  Class state
        # (obs_catalog_indices, geometric_delays) keeps the catalog order.
        up = self._cull_order(dircos_roi[:, 2], fwhm)                             # (n = sin(altitude): the same order)
        dircos_up = dircos_roi
        if up is not None:
            dircos_up, fwhm = dircos_roi[up], fwhm[up]
            flux_ref, spindex = (flux_ref[up], spindex[up]) if flux_ref is not None else (None, None)
            fluxes = fluxes[up] if fluxes is not None else None
            pb = pb[up] if pb is not None else None
        if pb is not None:
            # supplied beam (ROI_parameters path): pbfluxes = pb * fluxes on the device (:6254)
            self._ctx.set_sky(dircos_up, pb, pc_dircos, fwhm_deg=fwhm, fluxes=fluxes)
        elif getattr(self, '_extbeam', None) is not None:
            self._ctx.set_sky_external_analytic(dircos_up, flux_ref, spindex, ref_freq, pc_dircos, fwhm_deg=fwhm, flux_spectrum=fluxes)
        else:
            kind, dia, bpc, ext = PB.device_beam_spec(self.telescope, pointing_info=pb_info, pointing_center=pc_altaz,
                                                      first_frequency_hz=float(self.channels[0]))                   # :6252
            self._ctx.set_sky_analytic(dircos_up, flux_ref, spindex, ref_freq, kind, dia, bpc, pc_dircos, fwhm_deg=fwhm,
                                       flux_spectrum=fluxes, ext=ext)
        return m2, dircos_roi

    # skyvis_freq: (nbl, nchan, n_acc), time fastest, like the reference (:6385-6390)
    @property
    def skyvis_freq(self):
        if not getattr(self, '_cube', None):
            return self._skyvis_override
        if getattr(self, '_skyvis_cache', None) is None:
            staged = [isinstance(sn, _DeviceSlot) and sn.staged for sn in self._cube]
            if any(staged):
                self._ctx.wait_downloads()                              # the copies ran under the later snapshots' sky-sums
            for i, snap in enumerate(self._cube):
                if isinstance(snap, _DeviceSlot):                       # first read: fetch the device-resident snapshots
                    if snap.staged:
                        self._cube[i] = self._host_cube[snap.slot]
                    else:
                        self._cube[i] = self._ctx.get_vis(slot=snap.slot, complex64=(snap.dtype == NP.complex64))
            # the reference's layout: (nbl, nchan, n_acc) C-contiguous, time fastest (:6385-6390) -- a host-side transpose of the
            # per-snapshot arrays; skyvis_freq_snapshots() hands out the snapshot-major cube without it
            self._skyvis_cache = NP.stack(self._cube, axis=2)
        return self._skyvis_cache

    def skyvis_freq_snapshots(self):
        """The visibilities snapshot-major, (n_acc, nbl, nchan) -- the layout they are computed and downloaded in.  With
        reserve(host_staging=True) this is the page-locked host cube itself (no copy: the downloads already ran under the later
        snapshots' sky-sums and only the last one is waited for); otherwise the snapshots are fetched and stacked."""
        if not getattr(self, '_cube', None):
            return None if self._skyvis_override is None else NP.moveaxis(NP.asarray(self._skyvis_override), 2, 0)
        hc = getattr(self, '_host_cube', None)
        if hc is not None and all(isinstance(sn, _DeviceSlot) and sn.staged and sn.slot == i for i, sn in enumerate(self._cube)):
            self._ctx.wait_downloads()
            return hc[:len(self._cube)]
        return NP.moveaxis(self.skyvis_freq, 2, 0)

    @skyvis_freq.setter
    def skyvis_freq(self, value):
        self._skyvis_override = value
        self._device_in_step = False      # the device slots no longer hold this cube (callers that re-upload set the flag again)
        if value is not None:
            value = NP.asarray(value)
            self._cube = [value[:, :, i] for i in range(value.shape[2])]
            self._skyvis_cache = value

    def _upload_cube(self):
        """Put the host visibility cube into the device slots (needs reserve(n_acc) slots) and mark the two as in step."""
        cube = self.skyvis_freq
        for t in range(cube.shape[2]):
            self._ctx.set_vis(NP.ascontiguousarray(cube[:, :, t], dtype=NP.complex128), slot=t)
        self._device_in_step = True

    # bp, bp_wts, Tsys: (nbl, nchan) before the first snapshot, (nbl, nchan, n_acc) afterwards, like the reference's; kept as
    # per-snapshot layers (_LayerStack) and materialised on read.  Assigning an array replaces the layers.
    def _get_stacked(self, name):
        if name not in getattr(self, '_dense', {}):
            self.__dict__.setdefault('_dense', {})[name] = self._stacks[name].dense()
        return self._dense[name]

    def _set_stacked(self, name, value):
        self.__dict__.setdefault('_dense', {})[name] = NP.asarray(value)
        self.__dict__.setdefault('_stacks', {})[name] = None

    bp = property(lambda self: self._get_stacked('bp'), lambda self, v: self._set_stacked('bp', v))
    bp_wts = property(lambda self: self._get_stacked('bp_wts'), lambda self, v: self._set_stacked('bp_wts', v))
    Tsys = property(lambda self: self._get_stacked('Tsys'), lambda self, v: self._set_stacked('Tsys', v))

    def _append_layer(self, name, layer):
        """One more snapshot layer ((nbl | 1, nchan | 1), or (nbl, nchan, 1)) of a stacked attribute."""
        st = self._stacks.get(name)
        if st is not None:
            st.append(layer)
            self._dense.pop(name, None)
            return
        cur = self._dense[name]                                          # the attribute was assigned a dense array: grow that
        nbl, nchan = self.baselines.shape[0], self.channels.size
        layer = NP.asarray(layer)
        layer = NP.array(NP.broadcast_to(layer if layer.ndim == 3 else layer.reshape(layer.shape[0] if layer.ndim == 2 else 1, -1)[:, :, NP.newaxis],
                                         (nbl, nchan, 1)))
        self._dense[name] = layer if cur.ndim == 2 else NP.dstack((cur, layer))

    def _window_layers(self):
        """bp * bp_wts (:8116) per snapshot as a list of (1 | nbl, nchan) arrays: compact layers while both attributes are layer stacks,
        else the snapshots of the dense product."""
        a, b = self._stacks.get('bp'), self._stacks.get('bp_wts')
        if a is not None and b is not None and len(a.layers) == len(b.layers) and a.layers:
            return [x * y for x, y in zip(a.layers, b.layers)]
        wall = (self.bp * self.bp_wts).reshape(self.baselines.shape[0], self.channels.size, -1)
        return [wall[:, :, t] for t in range(wall.shape[2])]

    # skyvis_lag / lag_kernel: computed on the GPU by delay_transform(); when the visibility cube is resident on the device the
    # spectra stay there too (a _ResidentLags) and are fetched on first read
    @property
    def skyvis_lag(self):
        if getattr(self, '_lag_resident', None) is not None and getattr(self, '_skyvis_lag', None) is None:
            self._skyvis_lag = self._lag_resident.spectra()
        return getattr(self, '_skyvis_lag', None)

    @skyvis_lag.setter
    def skyvis_lag(self, value):
        self._skyvis_lag = value
        self._lag_resident = None

    def skyvis_lag_rows(self, rows):
        """Delay spectra (len(rows), nlag, n_acc) of selected baselines without fetching the whole cube from the device."""
        if getattr(self, '_lag_resident', None) is not None and getattr(self, '_skyvis_lag', None) is None:
            return self._lag_resident.spectra(rows)
        if self.skyvis_lag is None:
            raise RuntimeError('delay_transform() must be called first')
        return self.skyvis_lag[NP.asarray(rows), :, :]

    @property
    def lag_kernel(self):
        if getattr(self, '_lag_kernel', None) is None and getattr(self, '_lag_kernel_maker', None) is not None:
            self._lag_kernel = self._lag_kernel_maker()
            self._lag_kernel_maker = None
        return getattr(self, '_lag_kernel', None)

    @lag_kernel.setter
    def lag_kernel(self, value):
        self._lag_kernel = value
        self._lag_kernel_maker = None

    # ------------------------------------------------------------------------------------------
    def observing_run(self, pointing_init, skymodel, t_acc, duration, channels,
                      bpass, Tsys, lst_init, roi_radius=None, roi_center=None,
                      mode='track', pointing_coords=None, freq_scale=None,
                      brightness_units=None, verbose=True, memsave=False):
        """Extended observing run in 'track' or 'drift' mode built from snapshots
        (interferometry.py:6414-6657; argument checks :6510-6601, LST ramp :6607, pointing :6611-6633).
        lst_init is in HOURS, as the reference's LST ramp (:6607) treats it."""
        if isinstance(pointing_init, list):
            pointing_init = NP.asarray(pointing_init)
        elif not isinstance(pointing_init, NP.ndarray):
            raise TypeError('pointing_init must be a list or numpy array.')
        if pointing_init.size != 2:
            raise ValueError('pointing_init must be a 2-element vector.')
        pointing_init = pointing_init.ravel().astype(NP.float64)
        if not isinstance(t_acc, (int, float)):
            raise TypeError('t_acc must be a scalar integer or float.')
        if t_acc <= 0.0:
            raise ValueError('t_acc must be positive.')
        if not isinstance(duration, (int, float)):
            raise TypeError('duration must be a scalar integer or float.')
        if duration <= t_acc:
            if verbose:
                warnings.warn('\t\tDuration specified to be shorter than t_acc. Will set it equal to t_acc')
            duration = t_acc
        n_acc = int(duration / t_acc)                                                  # :6536
        nbl, nchan = self.baselines.shape[0], self.channels.size
        if not isinstance(bpass, (list, tuple, NP.ndarray)):
            raise TypeError('bpass must be a list, tuple or numpy array')
        bpass = NP.asarray(bpass)
        if bpass.size == nchan:                                                        # :6561-6572
            bpass = NP.expand_dims(NP.repeat(bpass.reshape(1, -1), nbl, axis=0), axis=2)
        elif bpass.size == nbl * nchan:
            bpass = NP.expand_dims(bpass.reshape(-1, nchan), axis=2)
        elif bpass.size == nbl * nchan * n_acc:
            bpass = bpass.reshape(-1, nchan, n_acc)
        else:
            raise ValueError('Dimensions of bpass incompatible with the number of frequency channels, baselines and number of accumulations.')
        if not isinstance(Tsys, (int, float, list, tuple, NP.ndarray)):
            raise TypeError('Tsys must be a scalar, list, tuple or numpy array')
        Tsys = NP.asarray(Tsys, dtype=NP.float64).reshape(-1)                          # :6574-6598
        if Tsys.size == 1:
            Tsys = Tsys + NP.zeros((nbl, nchan, 1))
        elif Tsys.size == nchan:
            Tsys = NP.expand_dims(NP.repeat(Tsys.reshape(1, -1), nbl, axis=0), axis=2)
        elif Tsys.size == nbl:
            Tsys = NP.expand_dims(NP.repeat(Tsys.reshape(-1, 1), nchan, axis=1), axis=2)
        elif Tsys.size == nbl * nchan:
            Tsys = NP.expand_dims(Tsys.reshape(-1, nchan), axis=2)
        elif Tsys.size == nbl * nchan * n_acc:
            Tsys = Tsys.reshape(-1, nchan, n_acc)
        else:
            raise ValueError('Dimensions of Tsys incompatible with the number of frequency channels, baselines and number of accumulations.')
        if not isinstance(lst_init, (int, float)):
            raise TypeError('Starting LST should be a scalar')

        lst = (lst_init + (t_acc / 3.6e3) * NP.arange(n_acc)) * 15.0                   # :6607 (degrees)
        lst_init_deg = lst_init * 15.0
        if mode == 'track':                                                            # :6611-6622
            if pointing_coords == 'hadec':
                pointing = NP.asarray([lst_init_deg - pointing_init[0], pointing_init[1]])
            elif (pointing_coords == 'radec') or (pointing_coords is None):
                pointing = pointing_init
            elif pointing_coords == 'altaz':
                hadec = GEOM.altaz2hadec(pointing_init, self.latitude, units='degrees')
                pointing = NP.asarray([lst_init_deg - hadec[0], hadec[1]])
            else:
                raise ValueError('pointing_coords can only be set to "hadec", "radec" or "altaz".')
            self.pointing_coords = 'radec'
            self.phase_center_coords = 'radec'
        elif mode == 'drift':                                                          # :6623-6633
            if pointing_coords == 'radec':
                pointing = NP.asarray([lst_init_deg - pointing_init[0], pointing_init[1]])
            elif (pointing_coords == 'hadec') or (pointing_coords is None):
                pointing = pointing_init
            elif pointing_coords == 'altaz':
                pointing = GEOM.altaz2hadec(pointing_init, self.latitude, units='degrees')
            else:
                raise ValueError('pointing_coords can only be set to "hadec", "radec" or "altaz".')
            self.pointing_coords = 'hadec'
            self.phase_center_coords = 'hadec'
        else:
            raise ValueError('mode must be "track" or "drift"')

        jd0 = 2451545.0
        # :6641-6647 loops observe(); here the snapshots go to the device as ONE batch (observe_batch): the sky model stays resident,
        # the geometry of all snapshots is formed there first, and arrays of at most 256 baselines sum all of them in one launch
        times = [(jd0 + i * t_acc / 86400.0, float(lst[i])) for i in range(n_acc)]
        self.observe_batch(times, [{'Tnet': Tsys[:, :, i % Tsys.shape[2]]} for i in range(n_acc)],
                           [bpass[:, :, i % bpass.shape[2]] for i in range(n_acc)], pointing, skymodel, t_acc,
                           roi_radius=roi_radius, roi_center=roi_center, memsave=memsave)
        self.t_obs = duration                                                          # :6654-6655
        self.n_acc = n_acc

    # ------------------------------------------------------------------------------------------
    def _thermal_rms(self):
        """vis_rms_freq from the system parameters (interferometry.py:6661-6687), broadcastable to (nbl, nchan, nt): the statement of
        generate_noise, also read by closure_phase_realizations.  No attribute is changed."""
        if not self.timestamp:
            raise ValueError('no snapshots: call observe() first')
        eff_Q = self.eff_Q if self.eff_Q.ndim == 3 else self.eff_Q[:, :, NP.newaxis]
        A_eff = self.A_eff if self.A_eff.ndim == 3 else self.A_eff[:, :, NP.newaxis]
        t_acc = NP.asarray(self.t_acc, dtype=NP.float64)[NP.newaxis, NP.newaxis, :]
        Tsys = self.Tsys if self.Tsys.ndim == 3 else self.Tsys[:, :, NP.newaxis]
        if self.flux_unit in ('JY', 'jy', 'Jy'):
            return 2.0 * 1.380649e-23 / NP.sqrt(t_acc * self.freq_resolution) * (Tsys / A_eff / eff_Q) / 1.0e-26   # :6685
        if self.flux_unit in ('K', 'k'):
            return 1.0 / NP.sqrt(t_acc * self.freq_resolution) * Tsys / eff_Q                                  # :6687
        raise ValueError('Flux density units can only be in Jy or K.')

    def generate_noise(self, seed=None, bl_offset=0, bl_index=None):
        """Thermal noise for every (baseline, channel, snapshot) from the system parameters (interferometry.py:6661-6693):
        vis_rms_freq = 2 k / sqrt(t_acc df) * Tsys / (A_eff eff_Q) / Jy (flux_unit 'JY') or Tsys / eff_Q / sqrt(t_acc df) ('K');
        vis_noise_freq = vis_rms_freq / sqrt(2) * (randn + 1j randn).  The normals are drawn on the GPU (counter-based Philox),
        reproducibly for a given `seed` (None: a fresh random seed, like the reference's global numpy RNG)."""
        self.vis_rms_freq = self._thermal_rms()
        if seed is None:
            seed = int(NP.random.SeedSequence().generate_state(2, dtype=NP.uint32).astype(NP.uint64) @ NP.array([1, 1 << 32], dtype=NP.uint64))
        rms_tbf = NP.ascontiguousarray(NP.transpose(NP.broadcast_to(self.vis_rms_freq, (self.baselines.shape[0], self.channels.size,
                                                                                          len(self.timestamp))), (2, 0, 1)))
        # bl_offset / bl_index: this array's baselines inside the WHOLE array of a sharded run (the draws are keyed on the global index)
        noise = self._ctx.noise(rms_tbf, seed, bl_offset=bl_offset, bl_index=bl_index)   # (nt, nbl, nchan)
        self.vis_noise_freq = NP.transpose(noise, (1, 2, 0))                             # :6692
        self.noise_seed = seed

    def add_noise(self):
        """vis_freq = gains * skyvis_freq + vis_noise_freq (interferometry.py:6697-6722).  With a GainInfo the gains come from
        spline_gains at (channels, timestamps); on IndexError from spline_gains at timestamps - timestamps[0]; on IndexError again
        from nearest_gains; if that fails too, unity gains with a warning.  The gains are applied on the device from their per-kind
        tables (prisim_amd/gains.py) -- no gain cube is formed.  The sky is the device-resident cube when it is in step with
        skyvis_freq, otherwise skyvis_freq itself; the noise is vis_noise_freq as it stands."""
        if self.vis_noise_freq is None:
            raise ValueError('generate_noise() must be called first')
        plan = None
        if self.gaininfo is not None:
            labels = self.gain_labels()[self._gain_rows()]
            times = NP.asarray(self.timestamp)
            try:
                plan = self.gaininfo.spline_plan(labels, freqs=self.channels, times=times)
            except IndexError:
                try:
                    plan = self.gaininfo.spline_plan(labels, freqs=self.channels, times=times - self.timestamp[0])
                except IndexError:
                    try:
                        plan = self.gaininfo.nearest_plan(labels, freqs=self.channels, times=times)
                    except Exception:
                        warnings.warn('Interpolation and nearest neighbour logic failed. Proceeding with default unity gains')
        else:
            warnings.warn('Gain table absent. Proceeding with default unity gains')
        if plan is None:
            self.vis_freq = self.skyvis_freq + self.vis_noise_freq
            return
        self.vis_freq = self._apply_gains(plan)

    def gain_labels(self):
        """The baselines' labels as the reference's gain methods take them: a structured array with fields 'A2', 'A1' (from (A2, A1)
        tuples, such a structured array, or the driver's '{prefix}{A2}-{prefix}{A1}' strings).  Rows marked in gain_padding get an
        empty label: they take no part in the gain evaluation."""
        from .gains import bl_label_array
        keep = self._gain_rows()
        labels = bl_label_array([self.labels[i] if keep[i] else ('', '') for i in range(len(self.labels))])
        return labels

    def _gain_rows(self):
        """bool (nbl,): the rows whose gains come from the gain table (every row but those of gain_padding)."""
        nbl = self.baselines.shape[0]
        if self.gain_padding is None:
            return NP.ones(nbl, dtype=bool)
        pad = NP.asarray(self.gain_padding, dtype=bool).ravel()
        if pad.size != nbl:
            raise ValueError('gain_padding must have one entry per baseline')
        return ~pad

    def _apply_gains(self, plan):
        """gains * skyvis_freq + vis_noise_freq on the device for a GainPlan, with numpy's broadcasting of the three shapes."""
        nbl, nchan, nt = self.baselines.shape[0], self.channels.size, len(self.timestamp)
        keep = self._gain_rows()
        nval = int(NP.sum(keep))
        gshape = tuple(plan.shape[p] for p in plan.perm)
        noise = NP.asarray(self.vis_noise_freq)
        out_shape = tuple(int(n) for n in NP.broadcast_shapes(gshape, (nval, nchan, nt), noise[keep].shape))   # numpy's ValueError
        if out_shape != (nval, nchan, nt) or noise.shape != (nbl, nchan, nt) or (plan.perm != [0, 1, 2] and gshape != (1, 1, 1)):
            raise NotImplementedError('gains of shape {0} (axes {1}) against visibilities {2} and noise {3}: only gains that broadcast '
                                      'along (label, frequency, time) are applied'.format(gshape, plan.perm, (nbl, nchan, nt), noise.shape))
        cube = getattr(self, '_cube', None) or []
        resident = bool(getattr(self, '_device_in_step', False)) and len(cube) == nt and \
            all(isinstance(sn, _DeviceSlot) and sn.slot == i for i, sn in enumerate(cube))
        sky, c64 = None, False
        if resident:
            c64 = any(sn.dtype == NP.complex64 for sn in cube)
            if not all((sn.dtype == NP.complex64) == c64 for sn in cube):
                resident = False
        if not resident:
            sky = NP.ascontiguousarray(NP.moveaxis(NP.asarray(self.skyvis_freq), 2, 0), dtype=NP.complex128)     # complex64 promoted
            c64 = False
        noise_tbf = NP.ascontiguousarray(NP.moveaxis(noise, 2, 0), dtype=NP.complex128)
        facs, tabs = plan.device_factors(self._ctx, nval)
        full = []
        for tab, mode, a, c in facs:                  # rows of gain_padding: row -1, unity gains
            fa, fc = NP.full(nbl, -1, dtype=NP.int64), NP.zeros(nbl, dtype=NP.int64)
            fa[keep], fc[keep] = a, c
            full.append((tab, mode, fa, fc))
        try:
            vis, _ = self._ctx.gains_apply(nt, nbl, nchan, fa=full[0] if full else None, fb=full[1] if len(full) > 1 else None,
                                           sky=sky, t0=0, sky_c64=c64, noise=noise_tbf)
        finally:
            for tab in tabs:
                tab.close()
        return NP.ascontiguousarray(NP.moveaxis(vis, 0, 2))

    # ------------------------------------------------------------------------------------------
    def _pc_dircos(self, pc, coords):
        """Phase centres (n_acc, 2|3) in `coords` -> ENU direction cosines, per snapshot (uses self.lst)."""
        pc = NP.asarray(pc, dtype=NP.float64)
        lst = NP.asarray(self.lst, dtype=NP.float64)
        if coords == 'dircos':
            if (pc.shape[1] < 2) or (pc.shape[1] > 3):
                raise ValueError('Dimensions incompatible for direction cosine positions')
            if NP.any(NP.sqrt(NP.sum(pc ** 2, axis=1)) > 1.0 + 1e-12):
                raise ValueError('direction cosines found to be exceeding unit magnitude.')
            if pc.shape[1] == 2:
                pc = NP.hstack((pc, NP.sqrt(NP.maximum(0.0, 1.0 - NP.sum(pc ** 2, axis=1))).reshape(-1, 1)))
            return pc
        if coords == 'altaz':
            return GEOM.altaz2dircos(pc, 'degrees')
        if coords == 'hadec':
            return GEOM.altaz2dircos(GEOM.hadec2altaz(pc, self.latitude, units='degrees'), 'degrees')
        if coords == 'radec':
            hadec = NP.stack((lst - pc[:, 0], pc[:, 1]), axis=1)
            return GEOM.altaz2dircos(GEOM.hadec2altaz(hadec, self.latitude, units='degrees'), 'degrees')
        raise ValueError('Invalid phase center coordinate system specified')

    def _convert_pc(self, dircos, coords):
        """ENU direction cosines -> phase-centre coordinates in `coords` (for the phase_center attribute)."""
        if coords == 'dircos':
            return dircos
        altaz = GEOM.dircos2altaz(dircos, units='degrees')
        if coords == 'altaz':
            return altaz
        hadec = GEOM.altaz2hadec(altaz, self.latitude, units='degrees')
        if coords == 'hadec':
            return hadec
        return NP.stack((NP.asarray(self.lst) - hadec[:, 0], hadec[:, 1]), axis=1)

    def phase_centering(self, phase_center=None, phase_center_coords=None, do_delay_transform=False, verbose=True):
        """Re-centre the visibility phases on new phase centre(s): V *= exp(-2 pi i f b.(s_cur - s_new)/c)
        (interferometry.py:7735-7886; arithmetic :7871-7877) on the GPU.  phase_center: (1|n_acc, 2|3) array in
        phase_center_coords ('radec', 'hadec', 'altaz', 'dircos'); None uses the pointing centres."""
        if phase_center is None:
            phase_center = self.pointing_center
            phase_center_coords = self.pointing_coords
        elif not isinstance(phase_center, NP.ndarray):
            raise TypeError('Phase center must be a numpy array')
        if phase_center_coords is None:
            raise NameError('Coordinates of phase center not provided.')
        phase_center = NP.asarray(phase_center, dtype=NP.float64)
        if phase_center.ndim == 1:
            phase_center = phase_center.reshape(1, -1)
        if phase_center.ndim != 2:
            raise ValueError('Phase center has invalid dimensions')
        n_acc = len(self.lst)
        if phase_center.shape[0] == 1:
            phase_center = NP.repeat(phase_center, n_acc, axis=0)
        elif phase_center.shape[0] != n_acc:
            raise ValueError('One phase center must be provided for every timestamp.')
        if not getattr(self, '_cube', None) and getattr(self, '_skyvis_override', None) is None:
            raise ValueError('no visibilities to rotate: call observe() first')
        cur = self._pc_dircos(self.phase_center, self.phase_center_coords)
        new = self._pc_dircos(phase_center, phase_center_coords)
        diff = cur - new                                                               # :7871

        def rotate(cube):
            cube = NP.asarray(cube, dtype=NP.complex128)
            out = NP.empty_like(cube)
            for t in range(cube.shape[2]):                 # through device cube slot 0 (host-resident cubes)
                self._ctx.set_vis(cube[:, :, t], slot=0)
                self._ctx.phase_rotate(1, diff[[t]])
                out[:, :, t] = self._ctx.get_vis(slot=0)
            return out

        resident = self._reserved >= n_acc and len(self._cube) == n_acc and all(isinstance(sn, _DeviceSlot) for sn in self._cube)
        if resident and self.vis_freq is None and self.vis_noise_freq is None:
            # the whole cube lives on the device (reserve()) and was never read: rotate it where it is, one kernel over all snapshots
            self._ctx.phase_rotate(n_acc, diff)                                         # :7877
            self._skyvis_cache = None
            for sn in self._cube:                              # host copies staged before the rotation are stale: queue them again
                if sn.staged:
                    sn.staged = self._stage_download(sn.slot, sn.dtype)
        else:
            dtype = self.skyvis_freq.dtype
            self.skyvis_freq = rotate(self.skyvis_freq).astype(dtype)                  # :7877
            if self.vis_freq is not None:
                self.vis_freq = rotate(self.vis_freq)
            if self.vis_noise_freq is not None:
                self.vis_noise_freq = rotate(self.vis_noise_freq)
            if self._reserved >= n_acc:                        # keep the device-resident cube in step
                self._upload_cube()
        self.phase_center = self._convert_pc(new, self.phase_center_coords)            # :7874-7875
        if do_delay_transform:
            self.delay_transform(verbose=verbose)

    def project_baselines(self, ref_point):
        """Baselines projected on the (u, v, w) frame of a reference direction per snapshot
        (interferometry.py:7890-7985; rotation matrix :7979-7981).  Host side: O(nbl * n_acc)."""
        if not isinstance(ref_point, dict):
            raise TypeError('Input ref_point must be a dictionary')
        if ('location' not in ref_point) or ('coords' not in ref_point):
            raise KeyError('Both keys "location" and "coords" must be specified in input dictionary ref_point')
        pc, coords = ref_point['location'], ref_point['coords']
        if not isinstance(pc, NP.ndarray):
            raise TypeError('The specified reference point must be a numpy array')
        if not isinstance(coords, str):
            raise TypeError('The specified coordinates of the reference point must be a string')
        if coords not in ['radec', 'hadec', 'altaz', 'dircos']:
            raise ValueError('Specified coordinates of reference point invalid')
        pc = pc.reshape(1, -1) if pc.ndim == 1 else pc
        if pc.ndim > 2:
            raise ValueError('Reference point has invalid dimensions')
        if (pc.shape[0] != self.n_acc) and (pc.shape[0] != 1):
            raise ValueError('Reference point has dimensions incompatible with the number of timestamps')
        if pc.shape[0] == 1:
            pc = NP.repeat(pc, self.n_acc, axis=0)
        dc = self._pc_dircos(pc, coords)
        hadec = GEOM.altaz2hadec(GEOM.dircos2altaz(dc, units='degrees'), self.latitude, units='degrees')
        ha, dec = NP.radians(hadec[:, 0]), NP.radians(hadec[:, 1])
        lat = NP.radians(self.latitude)
        e, n, u = self.baselines[:, 0], self.baselines[:, 1], self.baselines[:, 2]
        eq = NP.stack((-NP.sin(lat) * n + NP.cos(lat) * u, e, NP.cos(lat) * n + NP.sin(lat) * u), axis=1)   # GEOM.enu2xyz (:7977)
        rot = NP.asarray([[NP.sin(ha), NP.cos(ha), NP.zeros(ha.size)],
                          [-NP.sin(dec) * NP.cos(ha), NP.sin(dec) * NP.sin(ha), NP.cos(dec)],
                          [NP.cos(dec) * NP.cos(ha), -NP.cos(dec) * NP.sin(ha), NP.sin(dec)]])            # :7979-7981
        self.projected_baselines = NP.einsum('bk,jkt->bjt', eq, rot)                                      # :7985 (nbl, 3, n_acc)

    def rotate_visibilities(self, ref_point, do_delay_transform=False, verbose=True):
        """phase_centering + project_baselines about one reference point (interferometry.py:7655-7733)."""
        if not isinstance(ref_point, dict):
            raise TypeError('Input ref_point must be a dictionary')
        if ('location' not in ref_point) or ('coords' not in ref_point):
            raise KeyError('Both keys "location" and "coords" must be specified in input dictionary ref_point')
        self.phase_centering(phase_center=ref_point['location'], phase_center_coords=ref_point['coords'],
                             do_delay_transform=do_delay_transform, verbose=verbose)
        self.project_baselines(ref_point)

    def conjugate(self, ind=None, verbose=True):
        """Flip the selected baselines and conjugate their visibilities (interferometry.py:7989-8048)."""
        if ind is None:
            return
        if isinstance(ind, str):
            if ind != 'all':
                raise ValueError('Value of ind must be "all" if set to string')
            ind = NP.arange(self.baselines.shape[0])
        elif isinstance(ind, (int, NP.integer)):
            ind = [ind]
        elif not isinstance(ind, (list, NP.ndarray)):
            raise TypeError('ind must be string "all", scalar interger, list or numpy array')
        ind = NP.asarray(ind)
        if NP.any(ind >= self.baselines.shape[0]):
            raise IndexError('Out of range indices found.')
        self.labels = [tuple(reversed(self.labels[i])) if (i in ind and isinstance(self.labels[i], tuple)) else self.labels[i]
                       for i in range(len(self.labels))]
        self.baselines[ind, :] = -self.baselines[ind, :]
        self.baseline_orientations = NP.angle(self.baselines[:, 0] + 1j * self.baselines[:, 1])
        if self.skyvis_freq is not None:
            cube = NP.array(self.skyvis_freq)
            cube[ind, :, :] = cube[ind, :, :].conj()
            self.skyvis_freq = cube
        for name in ('vis_freq', 'vis_noise_freq'):
            arr = getattr(self, name)
            if arr is not None:
                arr[ind, :, :] = arr[ind, :, :].conj()
        if self.projected_baselines is not None:
            self.projected_baselines[ind, :, :] = -self.projected_baselines[ind, :, :]
        self._reset_device_array()                                                 # the resident array follows the flip
        if self._reserved >= self.n_acc and self.skyvis_freq is not None:
            self._upload_cube()

    def adopt_observation(self, shard):
        """Make this (so far unobserved) array stand for the WHOLE array of an observation of which `shard` -- another InterferometerArray, one
        rank's baseline shard -- was a part: take over everything that does not depend on the baseline (snapshots, pointings, phase centres,
        system-temperature records, the bandpass / weights / Tsys layers).  What the reference gets by concatenating the per-rank part files
        along the baseline axis (scripts/run_prisim.py:2233-2242, interferometry.py `concatenate`); here the visibility cubes arrive through
        the all-gather and are assigned by the caller (skyvis_freq, vis_freq, vis_noise_freq, skyvis_lag ...).  Per-baseline layers of a
        shard cannot stand for the other shards' baselines and are refused."""
        if self.timestamp:
            raise ValueError('adopt_observation() is for an array that has not observed anything itself')
        if not NP.array_equal(self.channels, shard.channels):
            raise ValueError('the shard was observed on another channel grid')
        nbl, nchan = self.baselines.shape[0], self.channels.size
        for name in ('bp', 'bp_wts', 'Tsys'):
            st = shard._stacks.get(name)
            if st is not None:
                if any(l.shape[0] != 1 for l in st.layers) or (NP.ndim(st.initial) == 2 and st.initial.shape[0] not in (1,)):
                    raise ValueError('{0} of the shard varies with the baseline: not enough to describe the whole array'.format(name))
                new = _LayerStack(nbl, nchan, st.initial)
                new.layers = list(st.layers)
                self._stacks[name] = new
                self.__dict__.setdefault('_dense', {}).pop(name, None)
            else:
                dense = NP.asarray(shard._dense[name])
                if dense.shape[0] > 1 and not NP.array_equal(dense, NP.broadcast_to(dense[:1], dense.shape)):
                    raise ValueError('{0} of the shard varies with the baseline: not enough to describe the whole array'.format(name))
                self._set_stacked(name, NP.array(NP.broadcast_to(dense[:1], (nbl,) + dense.shape[1:])))
        if shard.vis_rms_freq is not None:
            rms = NP.asarray(shard.vis_rms_freq)
            if rms.shape[0] > 1 and not NP.array_equal(rms, NP.broadcast_to(rms[:1], rms.shape)):
                raise ValueError('vis_rms_freq of the shard varies with the baseline: not enough to describe the whole array')
            self.vis_rms_freq = NP.array(NP.broadcast_to(rms[:1], (nbl,) + rms.shape[1:]))
        self.timestamp, self.t_acc, self.lst = list(shard.timestamp), list(shard.t_acc), list(shard.lst)
        self.t_obs, self.n_acc = shard.t_obs, shard.n_acc
        self.Tsysinfo = list(shard.Tsysinfo)
        self.pointing_center = NP.array(shard.pointing_center)
        self.phase_center = NP.array(shard.phase_center)
        self.phase_center_coords = shard.phase_center_coords
        self.obs_catalog_indices = list(shard.obs_catalog_indices)
        self.flux_unit = shard.flux_unit
        self.lags = None if shard.lags is None else NP.array(shard.lags)
        self.noise_seed = getattr(shard, 'noise_seed', None)

    def apply_gradients(self, gradient_mode=None, perturbations=None):
        """First-order change of the sky visibilities under small baseline displacements, from the gradient cube observe()
        accumulated with gradient_mode='baseline' (interferometry.py:6726-6819; arithmetic :6810-6812):

            delta V[..., b, f, t] = -2 pi i / lambda_f * sum_k db[..., k, b] * G[k, b, f, t]

        perturbations   {'baseline': array of shape (3, nbl), (nseed, 3, nbl) or (n1, n2, ..., 3, nbl)} in the units of
                        `baselines`.  Fewer than three coordinate rows are completed with zeros and more than three are cut
                        to the first three, each with a warning, as in the reference.  The caller's dictionary is left as
                        given (the reference reshapes the array inside it in place).
        Returns an (n1, ..., nbl, nchan, n_acc) complex array; a plain (3, nbl) input gives a leading axis of 1.
        """
        if gradient_mode is None:
            gradient_mode = self.gradient_mode
        if perturbations is None:
            perturbations = {gradient_mode: NP.zeros((1, 1, 1))}
        if self.gradient_mode is None or not self.gradient:
            raise AttributeError('No gradient attribute found')
        if not isinstance(perturbations, dict):
            raise TypeError('Input perturbations must be a dictionary')
        if not isinstance(gradient_mode, str):
            raise TypeError('Input gradient_mode must be a string')
        if gradient_mode not in ['baseline']:
            raise KeyError('Specified gradient mode {0} not currently supported'.format(gradient_mode))
        if gradient_mode not in perturbations:
            raise KeyError('{0} key not found in input perturbations'.format(gradient_mode))
        if gradient_mode != self.gradient_mode:
            raise ValueError('Specified gradient mode {0} not found in attribute'.format(gradient_mode))
        pert = perturbations[gradient_mode]
        if not isinstance(pert, NP.ndarray):
            raise TypeError('Perturbations must be specified as a numpy array')
        if pert.ndim < 2:
            raise ValueError('Perturbations must be two--dimensions or higher')
        if pert.ndim == 2:
            pert = pert[NP.newaxis, ...]
        lead = pert.shape[:-2]
        pert = pert.reshape(-1, pert.shape[-2], pert.shape[-1])                      # nseed x ncoord x nbl
        grad = self.gradient[gradient_mode]                                          # 3 x nbl x nchan x n_acc
        if pert.shape[2] != grad.shape[1]:
            raise ValueError('Number of {0} perturbations not equal to that in the gradient attribute'.format(gradient_mode))
        ncoord = pert.shape[1]
        if ncoord < 3:
            warnings.warn('Only {0}-dimensional coordinates specified. Proceeding with zero perturbations in other coordinate axes.'.format(ncoord))
        elif ncoord > 3:
            warnings.warn('{0}-dimensional coordinates specified. Proceeding with only the first three dimensions of coordinate axes.'.format(3))
        ncoord = min(ncoord, 3)                                                      # absent rows contribute nothing
        wavenumber = 2.0 * NP.pi * self.channels / C_LIGHT                           # 2 pi / lambda
        delta = NP.einsum('skb,kbft->sbft', pert[:, :ncoord, :], grad[:ncoord])
        delta = -1j * wavenumber.reshape(1, 1, -1, 1) * delta
        return delta.reshape(lead + grad.shape[1:])

    # ------------------------------------------------------------------------------------------
    def save(self, outfile, fmt='HDF5', tabtype='BinTableHDU', npz=True, overwrite=False, uvfits_parms=None, verbose=True):
        """Write the object to disk in PRISim's HDF5 layout (interferometry.py:8393-8863; groups and dataset names of
        :8723-8846) and, with npz, the reference's NPZ summary (:8854-8857).  HDF5 goes through the HDF5 C library
        (prisim_amd/hdf5io.py; no h5py here); FITS and UVFITS need astropy / pyuvdata and are not written."""
        if not isinstance(outfile, str):
            raise TypeError('outfile must be a string')
        if fmt.lower() not in ('hdf5', 'fits'):
            raise ValueError('Invalid output file format specified')
        if fmt.lower() == 'fits':
            raise NotImplementedError('FITS output needs astropy, which this build does not carry; use fmt="HDF5"')
        if uvfits_parms is not None:
            raise NotImplementedError('UVFITS output needs pyuvdata / astropy, which this build does not carry')
        from . import hdf5io
        filename = outfile + '.hdf5'
        if verbose:
            print('\nSaving information about interferometer...')
        tel = self.telescope
        with hdf5io.File(filename, 'w' if overwrite else 'w-') as f:
            f.create_group('header')
            f.write('header/AstroUtils#', 'none (prisim_amd)')
            f.write('header/PRISim#', 'prisim_amd')
            f.write('header/flux_unit', self.flux_unit)
            f.write('telescope_parms/latitude', float(self.latitude), attrs={'units': 'deg'})
            f.write('telescope_parms/longitude', float(self.longitude), attrs={'units': 'deg'})
            f.write('telescope_parms/altitude', float(self.altitude), attrs={'units': 'm'})
            if 'id' in tel:
                f.write('telescope_parms/id', str(tel['id']))
            f.write('spectral_info/freq_resolution', float(self.freq_resolution), attrs={'units': 'Hz'})
            f.write('spectral_info/freqs', self.channels, attrs={'units': 'Hz'})
            if self.lags is not None:
                f.write('spectral_info/lags', self.lags, attrs={'units': 's'})
            f.write('spectral_info/bp', self.bp)
            f.write('spectral_info/bp_wts', self.bp_wts)
            if self.simparms_file is not None:
                f.write('simparms/simfile', self.simparms_file)
            f.create_group('antenna_element')
            # the reference's reader insists on ocoords and orientation (:5261-5266): defaults of its constructor (:5703-5709)
            ocoords = str(tel.get('ocoords', 'altaz'))
            f.write('antenna_element/shape', str(tel.get('shape', 'delta')))
            f.write('antenna_element/ocoords', ocoords)
            f.write('antenna_element/size', NP.asarray(tel.get('size', 1.0), dtype=NP.float64), attrs={'units': 'm'})
            f.write('antenna_element/orientation', NP.asarray(tel.get('orientation', [[90.0, 270.0]]), dtype=NP.float64),      # as held (:8766)
                    attrs=({'units': 'deg'} if ocoords != 'dircos' else None))
            if tel.get('groundplane') is not None:
                f.write('antenna_element/groundplane', float(tel['groundplane']))
            if self.layout:
                f.write('layout/positions', NP.asarray(self.layout['positions'], dtype=NP.float64),
                        attrs={'units': 'm', 'coords': str(self.layout['coords'])})
                f.write('layout/labels', NP.asarray(self.layout['labels']))
                f.write('layout/ids', NP.asarray(self.layout['ids']))
            f.write('timing/t_obs', float(self.t_obs))
            f.write('timing/n_acc', int(self.n_acc))
            if self.t_acc:
                f.write('timing/t_acc', NP.asarray(self.t_acc, dtype=NP.float64))
            f.write('timing/timestamps', NP.asarray(self.timestamp))
            f.write('skyparms/pointing_coords', str(self.pointing_coords))
            f.write('skyparms/phase_center_coords', str(self.phase_center_coords))
            f.write('skyparms/skycoords', str(self.skycoords))
            f.write('skyparms/LST', NP.asarray(self.lst, dtype=NP.float64).ravel(), attrs={'units': 'deg'})
            f.write('skyparms/pointing_center', NP.asarray(self.pointing_center, dtype=NP.float64))
            f.write('skyparms/phase_center', NP.asarray(self.phase_center, dtype=NP.float64))
            labels = self.labels
            if len(labels) and isinstance(labels[0], (tuple, list)):                    # (A2, A1) antenna-pair records like the reference's
                width = max(max(len(str(a)), len(str(b))) for a, b in labels)
                labels = NP.asarray([(str(a).encode(), str(b).encode()) for a, b in labels], dtype=[('A2', 'S%d' % width), ('A1', 'S%d' % width)])
            else:
                labels = NP.asarray([str(l) for l in labels])
            f.write('array/labels', labels)
            # (the reference labels the dataset 'local-ENU' whatever baseline_coords says, :8794; an equatorial array is labelled as what it holds)
            f.write('array/baselines', self.baselines, attrs={'coords': 'equatorial-XYZ' if self.baseline_coords == 'equatorial' else 'local-ENU', 'units': 'm'})
            f.write('array/baseline_coords', str(self.baseline_coords))
            if self.projected_baselines is not None:
                f.write('array/projected_baselines', self.projected_baselines, attrs={'coords': 'eq-XYZ', 'units': 'm'})
            f.write('instrument/effective_area', self.A_eff, attrs={'units': 'm^2'})
            f.write('instrument/efficiency', self.eff_Q)
            if self.Tsysinfo:
                def col(get):
                    return NP.asarray([get(elem) for elem in self.Tsysinfo], dtype=NP.float64)
                nan = float('nan')
                f.write('instrument/Trx', col(lambda e: e.get('Trx') if e.get('Trx') is not None else nan), attrs={'units': 'K'})
                f.write('instrument/Tant0', col(lambda e: (e.get('Tant') or {}).get('T0', nan)), attrs={'units': 'K'})
                f.write('instrument/f0', col(lambda e: (e.get('Tant') or {}).get('f0', nan)), attrs={'units': 'Hz'})
                f.write('instrument/spindex', col(lambda e: (e.get('Tant') or {}).get('spindex', nan)))
                f.write('instrument/Tnet', col(lambda e: e['Tnet'] if e.get('Tnet') is not None else -999), attrs={'units': 'K'})
            f.write('instrument/Tsys', self.Tsys, attrs={'units': 'K'})
            f.create_group('visibilities/freq_spectrum')
            for name, arr in (('rms', self.vis_rms_freq), ('vis', self.vis_freq), ('skyvis', self.skyvis_freq), ('noise', self.vis_noise_freq)):
                if arr is not None:
                    f.write('visibilities/freq_spectrum/' + name, arr, attrs={'units': 'Jy'})
            f.create_group('visibilities/delay_spectrum')
            for name, arr in (('vis', self.vis_lag), ('skyvis', self.skyvis_lag), ('noise', self.vis_noise_lag)):
                if arr is not None:
                    f.write('visibilities/delay_spectrum/' + name, arr, attrs={'units': 'Jy Hz'})
            if self.gradient_mode is not None:
                for key, arr in self.gradient.items():
                    f.write('gradients/' + str(key), arr)
            if self.gaininfo is not None:                                                       # :8843-8846
                f.write('gaininfo/gainsfile', outfile + '.gains.hdf5')
                self.gaininfo.write_gaintable(outfile + '.gains.hdf5')
            if self.blgroups is not None:
                f.create_group('blgroupinfo/groups')
                f.create_group('blgroupinfo/reversemap')
                for key, members in self.blgroups.items():
                    f.write('blgroupinfo/groups/' + str(key).replace('/', '|'), NP.asarray([str(m) for m in members]))
                for key, val in (self.bl_reversemap or {}).items():
                    f.write('blgroupinfo/reversemap/' + str(key).replace('/', '|'), NP.asarray([str(val)]))
        if verbose:
            print('\tInterferometer array information written successfully to file on disk:\n\t\t{0}\n'.format(filename))
        if npz:
            keys = {'skyvis_freq': self.skyvis_freq, 'lst': self.lst, 'freq': self.channels, 'timestamp': self.timestamp,
                    'bl': self.baselines, 'bl_length': self.baseline_lengths}                              # :8857
            if (self.vis_freq is not None) and (self.vis_noise_freq is not None):                         # :8855
                keys.update({'vis_freq': self.vis_freq, 'vis_noise_freq': self.vis_noise_freq})
            NP.savez_compressed(outfile + '.npz', **keys)
        return filename

    # ------------------------------------------------------------------------------------------
    def duplicate_measurements(self, blgroups=None):
        """Re-create the redundant baselines from the simulated unique ones (interferometry.py:6823-6906): every baseline whose
        label is a key of `blgroups` is repeated once per member of its group (visibilities, gradient, baselines, per-baseline
        system parameters), labels become the members' labels, then noise is regenerated for the expanded set.  The GPU computes
        the unique baselines only; this is a host-side repeat."""
        if blgroups is None:
            blgroups = self.blgroups
        if not isinstance(blgroups, dict):
            raise TypeError('Input blgroups must be a dictionary')
        nbl = sum(len(v) for v in blgroups.values()) if self.bl_reversemap is None else len(self.bl_reversemap)
        if len(self.labels) >= nbl:
            return
        labels = [tuple(l) if isinstance(l, (list, NP.ndarray)) else l for l in self.labels]
        groups = {}
        for key, members in blgroups.items():
            members = [tuple(m) if isinstance(m, (list, NP.ndarray)) else m for m in members]
            if key not in labels:
                rkey = tuple(reversed(key)) if isinstance(key, tuple) else key
                if rkey not in labels:
                    raise KeyError('Input label {0} not found in attribute labels'.format(key))
                key = rkey
            if key not in members:
                members = [key] + members
            groups[key] = members
        new_labels, num_list = [], []
        for label in labels:
            members = groups.get(label, [label])
            num_list.append(len(members))
            for m in members:
                if m in new_labels:
                    raise ValueError('Label {0} repeated in more than one baseline group'.format(m))
                new_labels.append(m)
        if self.skyvis_freq is not None:
            self.skyvis_freq = NP.repeat(self.skyvis_freq, num_list, axis=0)
        if self.gradient_mode is not None and self.gradient.get(self.gradient_mode) is not None:
            self.gradient[self.gradient_mode] = NP.repeat(self.gradient[self.gradient_mode], num_list, axis=1)
        self.labels = new_labels
        self.baselines = NP.repeat(self.baselines, num_list, axis=0)
        if self.projected_baselines is not None:
            self.projected_baselines = NP.repeat(self.projected_baselines, num_list, axis=0)
        self.baseline_lengths = NP.repeat(self.baseline_lengths, num_list)
        self.baseline_orientations = NP.repeat(self.baseline_orientations, num_list)
        for name in ('Tsys', 'eff_Q', 'A_eff', 'bp', 'bp_wts'):
            arr = getattr(self, name, None)
            if isinstance(arr, NP.ndarray) and arr.ndim >= 1 and arr.shape[0] > 1:
                setattr(self, name, NP.repeat(arr, num_list, axis=0))
        # the resident device array follows the expanded baseline list (slots are re-uploaded on demand)
        self._reset_device_array()
        if self._reserved >= self.n_acc and self.skyvis_freq is not None:
            self._upload_cube()
        self.generate_noise()                                                          # :6905-6906
        self.add_noise()

    # ------------------------------------------------------------------------------------------
    def getThreePointCombinations(self, unique=False):
        """All (unique=False, the default) or only the unique triads of the antenna layout whose three baselines were simulated
        (interferometry.py:6989-7085): the triple loop over layout['labels'] in the reference's order, baselines matched through
        their '%.2f_%.2f_%.2f' strings with one sign flip, a warning (not an error) for a pair that was not simulated, and with
        unique=True only the first triad of every set of three baseline strings.  Returns what the reference returns: the list of
        antenna-label triplets and the list of [bl12, bl23, bl31] baseline vectors as matched (flipped legs flipped).  Host code;
        needs `layout` and `baselines` only."""
        if not isinstance(unique, bool):
            raise TypeError('Input unique must be boolean')

        def blstring(v):
            return '{0[0]:.2f}_{0[1]:.2f}_{0[2]:.2f}'.format(v)

        def match(v):
            """v cleaned as :7020-7028; (vector, string) of the simulated baseline it is, or of its negative; string None: neither"""
            v = v + 0.0
            v[NP.abs(v) < 1e-10] = 0.0
            if not NP.sqrt(NP.sum(v ** 2)) > 0.0:
                return v, False
            s = blstring(v)
            if s not in blstr:
                v = -1 * v + 0.0
                s = blstring(v)
            return v, (s if s in blstr else None)

        blstr = set(blstring(lo) for lo in (self.baselines + 0.0))
        pos = NP.asarray(self.layout['positions'], dtype=NP.float64)
        labels = self.layout['labels']
        missing = 'A baseline not found in the simulated reference baselines. Proceeding with the rest'
        anttriplets, blvecttriplets, seen = [], [], set()
        for aind1, albl1 in enumerate(labels):
            for aind2, albl2 in enumerate(labels):
                bl12, s12 = match(pos[aind2] - pos[aind1])
                if s12 is False:
                    continue
                if s12 is None:
                    warnings.warn(missing)
                    continue
                for aind3, albl3 in enumerate(labels):
                    bl23, s23 = match(pos[aind3] - pos[aind2])
                    bl31, s31 = match(pos[aind1] - pos[aind3])
                    if s23 is False or s31 is False:
                        continue
                    if s23 is None or s31 is None:                 # (the reference looks at 31 only once 23 is found: one warning)
                        warnings.warn(missing)
                        continue
                    if unique:
                        key = frozenset((s12, s23, s31))          # setdiff1d(new, old).size == 0 with three strings each
                        if any(key <= old for old in seen) if len(key) < 3 else key in seen:
                            continue
                        seen.add(key)
                    blvecttriplets += [[bl12, bl23, bl31]]
                    anttriplets += [(albl1, albl2, albl3)]
        return (anttriplets, blvecttriplets)

    def closure_leg_table(self, antenna_triplets):
        """The legs of antenna triplets as rows of the visibility cube (interferometry.py:7412-7485): for each (a1, a2, a3) the
        baseline ids (a2, a1), (a3, a2), (a1, a3) are looked up in bl_reversemap; an id found reversed is a conjugated leg; one
        found neither way raises the reference's ValueError.  Returns (legs (ntriads, 3) int32 rows ind12, ind23, ind31,
        conj (ntriads, 3) int32 flags, blvecttriplets: a list of (3, 3) arrays of the legs' baseline vectors, negated on conjugated
        legs).  An array built without blgroupinfo has no bl_reversemap (the reference then fails on `in None`): the identity map
        {label: label} of `labels` is used for the call; no attribute is changed.  A reversemap value that is not among `labels`
        raises the same ValueError (the reference: IndexError from NP.where(...)[0][0])."""
        from .dsp_readings import _key
        row_of = {}
        for i, lab in enumerate(self.labels):
            row_of.setdefault(_key(lab), i)
        if self.bl_reversemap is None:
            revmap = {k: k for k in row_of}
        else:
            revmap = {_key(k): _key(v) for k, v in self.bl_reversemap.items()}
        n = len(antenna_triplets)
        legs, conj = NP.zeros((n, 3), dtype=NP.int32), NP.zeros((n, 3), dtype=NP.int32)
        blvecttriplets = []
        for ti, anttriplet in enumerate(antenna_triplets):
            a1, a2, a3 = (str(_key(a)) for a in anttriplet)
            vec = NP.zeros((3, 3))
            for li, bl_id in enumerate(((a2, a1), (a3, a2), (a1, a3))):
                if bl_id in revmap:
                    ref = revmap[bl_id]
                elif tuple(reversed(bl_id)) in revmap:
                    ref = revmap[tuple(reversed(bl_id))]
                    conj[ti, li] = 1
                else:
                    raise ValueError('Baseline ({0[0]}, {0[1]}) not found in simulated baselines'.format(bl_id))
                if ref not in row_of:
                    raise ValueError('Baseline ({0[0]}, {0[1]}) not found in simulated baselines'.format(ref))
                legs[ti, li] = row_of[ref]
                vec[li, :] = -self.baselines[legs[ti, li], :] if conj[ti, li] else self.baselines[legs[ti, li], :]
            blvecttriplets += [vec]
        return legs, conj, blvecttriplets

    def getClosurePhase(self, antenna_triplets=None, delay_filter_info=None, specsmooth_info=None, spectral_window_info=None,
                        unique=False):
        """Closure phases (bispectrum phases) of the visibilities on triads of antennas, on the GPU (interferometry.py:7087-7651;
        include/prisim_closure.h).  Arguments and the returned dictionary are the reference's:

        antenna_triplets      list of antenna-label triplets; None: getThreePointCombinations(unique=unique)
        delay_filter_info     None, or {'type': 'horizon' (default) | 'regular', 'mode': 'discard' (default) | 'retain',
                              'min': seconds, 'width': in units of the delay resolution}: every leg is filtered as
                              ifft(mask * fft(freq_wts * v)) before the closure phase (:7348-7399, :7536-7599)
        spectral_window_info  None, or {'freq_center', 'bw_eff', 'shape', 'fftpow'} (each may be None): one spectral window, built
                              by delay_spectrum.subband_freq_wts (:7296-7344); default centre channels[nchan // 2]
        specsmooth_info       must be None (below)

        Returns {'closure_phase_skyvis', 'closure_phase_vis', 'closure_phase_noise': (ntriads, nchan, nt) radians;
        'antenna_triplets'; 'baseline_triplets': list of (3, 3) arrays; 'skyvis', 'vis', 'noisevis': (ntriads, 3, nchan, nt) the
        visibilities that went into the phases; 'spectral_weights': (1,) ones, or (nchan,)}.

        Departures, all stated: the noisy and noise entries are None when the array holds no vis_freq / vis_noise_freq (the
        reference fails there); specsmooth_info raises NotImplementedError (the reference's 'median' branch indexes
        specsmooth_info[specsmooth_info['window_size']] and cannot run, and 'interp' redraws noise from numpy's global generator);
        fftpow other than 1 raises NotImplementedError as everywhere in this package (DSP.window_fftpow is unread); without
        blgroupinfo the identity bl_reversemap is used (closure_leg_table).  DSP.FT1D is read as numpy's fft / ifft
        (prisim_amd/dsp_readings.py).  The noiseless cube is read where it lies on the device when the device slots are in step
        with skyvis_freq; the other cubes are uploaded once each.  bp * bp_wts is handed over dense, (nbl, nchan, nt) float64, also when
        it is constant in time; it and an uploaded cube lie on the device for the call, outside the chunk budget.  The stats of the
        device calls are left in closure_stats, per cube.  There is no CPU path."""
        p = _closure_prepare(self, antenna_triplets, delay_filter_info, specsmooth_info, spectral_window_info, unique)
        antenna_triplets, freq_wts, masks, mask_index = p['antenna_triplets'], p['freq_wts'], p['masks'], p['mask_index']
        legs, conj, blvecttriplets, nchan, nt, resident, bpwts = (p['legs'], p['conj'], p['baseline_triplets'], p['nchan'], p['nt'],
                                                                  p['resident'], p['bpwts'])
        out = {}
        self.closure_stats = {}                    # the device call's stats per cube: 'skyvis', 'vis', 'noisevis'
        for name, key in (('skyvis', 'skyvis'), ('vis', 'vis'), ('noise', 'noisevis')):
            if name == 'skyvis':
                cube = None if resident else self.skyvis_freq
            else:
                cube = self.vis_freq if name == 'vis' else self.vis_noise_freq
                if cube is None:
                    out[key], out['closure_phase_' + name] = None, None
                    continue
            if not legs.shape[0]:
                out[key] = NP.zeros((0, 3, nchan, nt), dtype=NP.complex128)
                out['closure_phase_' + name] = NP.zeros((0, nchan, nt))
                continue
            trip, phase, stats = self._ctx.closure_phase(cube, legs, conj, bpwts, freq_wts=freq_wts, masks=masks, mask_index=mask_index,
                                                         nt=nt)
            out[key], out['closure_phase_' + name] = trip, phase
            self.closure_stats[key] = stats
        out.update({'antenna_triplets': antenna_triplets, 'baseline_triplets': blvecttriplets, 'spectral_weights': freq_wts})
        return out

    def closure_phase_realizations(self, n_realize, seed, antenna_triplets=None, unique=False, datakey='noisy', n_avg=1, first=0,
                                   bl_index=None, route='auto', budget_bytes=None):
        """Closure phases of n_realize thermal-noise realisations of this noiseless run on triads of antennas, drawn and closed on
        the GPU (include/prisim_cpreal.h): the realisations of prisim/scriptUtils/replicatesim_util.py:replicate (:82-95) and their
        closure phases as prisim/bispectrum_phase.py:write_PRISim_bispectrum_phase_to_npz stacks them (:211-249).

        Realisation r is by definition what generate_noise(seed=seed + first + r, bl_index=bl_index); add_noise();
        getClosurePhase(antenna_triplets) gives in 'closure_phase_vis' ('noisy') and 'closure_phase_noise' ('noise'), bit for bit,
        with the rms divided by sqrt(n_avg) (replicate :90): the draws are keyed on (channel, global baseline, snapshot) and that seed.
        No noise cube is formed and nothing but the baselines of the triads is drawn or copied; vis_freq, vis_noise_freq and
        vis_rms_freq are left as they are.

        n_realize          number of realisations, >= 1
        seed, first        realisation r uses the key seed + first + r (mod 2^64)
        antenna_triplets   list of antenna-label triplets; None: getThreePointCombinations(unique=unique)
        datakey            'noisy', 'noise' or a list of them
        n_avg              averages per realisation: the rms is divided by sqrt(n_avg)
        bl_index           global index of every baseline of this array inside the whole array of a sharded run (None: its own rows)
        route              'auto', 'direct' or 'staged' (include/prisim_cpreal.h); budget_bytes: device bytes of the chunk buffers

        Returns {'closure_phase_vis' and / or 'closure_phase_noise': (nt, n_realize, ntriads, nchan) radians, 'antenna_triplets',
        'baseline_triplets', 'seeds': (n_realize,) uint64} and leaves the stats of the device calls in cpreal_stats, per datakey.  The
        noiseless cube is read where it lies on the device when the device slots are in step with skyvis_freq; otherwise the used rows
        of skyvis_freq are handed over.  A gaininfo raises NotImplementedError: gains are not part of the fused route.  There is no
        CPU path."""
        if isinstance(n_realize, bool) or not isinstance(n_realize, (int, NP.integer)):
            raise TypeError('n_realize must be an integer')
        if n_realize < 1:
            raise ValueError('n_realize must be at least 1')
        if not (n_avg > 0):
            raise ValueError('n_avg must be positive')
        keys = [datakey] if isinstance(datakey, str) else datakey
        if not isinstance(keys, list) or not keys:
            raise TypeError('datakey must be a string or a list of strings')
        for k in keys:
            if k not in ('noisy', 'noise'):
                raise ValueError("datakey can only hold 'noisy' and 'noise'")
        if self.gaininfo is not None:
            raise NotImplementedError('closure_phase_realizations does not apply gains: use generate_noise, add_noise and getClosurePhase')
        p = _closure_prepare(self, antenna_triplets, None, None, None, unique)
        legs, nbl, nchan, nt = p['legs'], p['nbl'], p['nchan'], p['nt']
        seeds = ((int(seed) + int(first) + NP.arange(n_realize, dtype=object)) % (1 << 64)).astype(NP.uint64)
        out = {'antenna_triplets': p['antenna_triplets'], 'baseline_triplets': p['baseline_triplets'], 'seeds': seeds}
        self.cpreal_stats = {}
        names = {'noisy': 'closure_phase_vis', 'noise': 'closure_phase_noise'}
        if not legs.shape[0]:
            for k in keys:
                out[names[k]] = NP.zeros((nt, n_realize, 0, nchan))
            return out
        used, inv = NP.unique(legs, return_inverse=True)                 # the distinct rows of the legs, and the legs as rows of those
        legs_used = NP.asarray(inv, dtype=NP.int32).reshape(legs.shape)
        if bl_index is not None and NP.asarray(bl_index).size != nbl:
            raise ValueError('bl_index must have one entry per baseline')
        glob = used if bl_index is None else NP.asarray(bl_index, dtype=NP.int64).ravel()[used]

        def rows_tbf(a):                                                 # (nbl | 1, nchan | 1, nt | 1) -> the used rows as (nt, nrow, nchan)
            a = NP.broadcast_to(a, (nbl, nchan, nt))[used]
            return NP.ascontiguousarray(NP.transpose(a, (2, 0, 1)))
        rms = rows_tbf(self._thermal_rms() / NP.sqrt(float(n_avg)))
        bpwts = rows_tbf(p['bpwts'])
        cube = None if p['resident'] else rows_tbf(NP.asarray(self.skyvis_freq, dtype=NP.complex128))
        kw = {} if budget_bytes is None else {'budget_bytes': budget_bytes}
        for k in keys:
            out[names[k]], self.cpreal_stats[k] = self._ctx.closure_realizations(
                cube, used if cube is None else None, glob, rms, bpwts, legs_used, p['conj'], seed, n_realize, first=first, kind=k, nt=nt,
                route=route, **kw)
        return out

    # ------------------------------------------------------------------------------------------
    def delay_transform(self, pad=1.0, freq_wts=None, verbose=True):
        """Frequency -> delay transform on the GPU (rocFFT) of whichever visibility cubes exist
        (interferometry.py:8052-8137; Q20).  Sets lags, skyvis_lag (vis_lag, vis_noise_lag when their
        frequency cubes exist) and lag_kernel."""
        if not isinstance(pad, (int, float)):
            raise TypeError('pad fraction must be a scalar value.')
        if pad < 0.0:
            pad = 0.0
            if verbose:
                warnings.warn('\tPad fraction found to be negative. Resetting to 0.0 (no padding will be applied).')
        nbl, nchan = self.baselines.shape[0], self.channels.size
        if freq_wts is not None:                                                       # :8096-8107
            freq_wts = NP.asarray(freq_wts)
            if freq_wts.size == nchan and self._stacks.get('bp') is not None and len(self._stacks['bp'].layers) == self.n_acc:
                # one window for every baseline and snapshot: kept as n_acc (1, nchan) layers (dense (nbl, nchan, n_acc) on read)
                st = _LayerStack(nbl, nchan, NP.ones((1, 1)))
                st.layers = [NP.asarray(freq_wts, dtype=NP.float64).reshape(1, -1)] * self.n_acc
                self._stacks['bp_wts'] = st
                self._dense.pop('bp_wts', None)
            else:
                if freq_wts.size == nchan:
                    freq_wts = NP.repeat(NP.expand_dims(NP.repeat(freq_wts.reshape(1, -1), nbl, axis=0), axis=2), self.n_acc, axis=2)
                elif freq_wts.size == nchan * self.n_acc:
                    freq_wts = NP.repeat(NP.expand_dims(freq_wts.reshape(nchan, -1), axis=0), nbl, axis=0)
                elif freq_wts.size == nchan * nbl:
                    freq_wts = NP.repeat(NP.expand_dims(freq_wts.reshape(-1, nchan), axis=2), self.n_acc, axis=2)
                elif freq_wts.size == nchan * nbl * self.n_acc:
                    freq_wts = freq_wts.reshape(nbl, nchan, self.n_acc)
                else:
                    raise ValueError('window shape dimensions incompatible with number of channels and/or number of tiemstamps.')
                self.bp_wts = freq_wts
        if not self._cube and self._skyvis_override is None:
            raise ValueError('no visibilities to transform: call observe() first')
        sky, lags, vis_lag, vis_noise_lag, make_kernel = self._transform_cubes(self._window_layers(), pad)
        self._skyvis_lag, self._lag_resident = (None, sky) if isinstance(sky, _ResidentLags) else (sky, None)
        self.lags = lags
        if vis_lag is not None:
            self.vis_lag = vis_lag
        if vis_noise_lag is not None:
            self.vis_noise_lag = vis_noise_lag
        self._lag_kernel, self._lag_kernel_maker = None, make_kernel      # formed on first read of lag_kernel

    def _transform_cubes(self, layers, pad, decimate=True):
        """The delay transform of the visibility cubes that exist, for delay_transform() and DelaySpectrum.delay_transform().  layers:
        the per-snapshot windows bp * bp_wts, each (1 | nbl, nchan).  Returns (sky, lags, vis_lag, vis_noise_lag, make_kernel): sky is a
        _ResidentLags when the cube is resident on the device (reserve()) and one window serves every snapshot -- all snapshots are
        transformed where they are and the spectra stay in HBM until read (the device cube is complex128 for memsave runs too: nothing is
        rounded on the way) --, else the host array (nbl, nlag, nt), transformed snapshot by snapshot through device slot 0; lags are the
        context's; vis_lag / vis_noise_lag are None where the cube does not exist; make_kernel() forms lag_kernel.
        decimate=False (DelaySpectrum's downsample=False with pad > 0): every snapshot goes through the host, the zero-padded product
        uploaded as the single snapshot of a temporary context whose channel grid is the padded one and transformed there with pad = 0 --
        same FFT length, same (npad + N) df scale (:1316-1321)."""
        ctx, nbl, nchan = self._ctx, self.baselines.shape[0], self.channels.size
        same = _all_same(layers)

        def transform(cube):
            outs, lags = [], None
            for t in range(cube.shape[2]):
                window = NP.broadcast_to(layers[t if (not same and t < len(layers)) else 0], (nbl, nchan))
                if decimate:
                    out, lags, _ = ctx.delay_transform_host(cube[:, :, t], window, pad)
                else:
                    npad = int(nchan * pad)
                    x = NP.zeros((nbl, nchan + npad), dtype=NP.complex128)
                    x[:, :nchan] = cube[:, :, t] * window
                    grid = self.channels[0] + self.freq_resolution * NP.arange(nchan + npad)
                    with _abi.Context(getattr(ctx, 'device', 0)) as tmp:
                        tmp.set_array(NP.asarray(self.baselines, dtype=NP.float64), grid, nt_max=1)
                        out, lags, _ = tmp.delay_transform_host(x, None, 0.0)
                outs.append(out)
            return NP.stack(outs, axis=2), lags

        # number of snapshots without forcing device-resident ones onto the host (_DeviceSlot placeholders)
        nt = len(self._cube) if self._cube else self._skyvis_override.shape[2]
        # Are the device slots holding THIS cube?  observe() into reserved slots leaves them in step; assigning skyvis_freq (the setter,
        # adopt_observation + assignment, assemble_full_array) does not -- then the cube is uploaded first when the slots exist,
        # otherwise the transform goes snapshot by snapshot through slot 0.
        if bool(self._cube) and self._reserved >= nt and self.n_acc == nt and not getattr(self, '_device_in_step', False) \
                and not any(isinstance(sn, _DeviceSlot) for sn in self._cube):
            self._upload_cube()
        resident = self._reserved >= self.n_acc and bool(self._cube) and getattr(self, '_device_in_step', False)   # slot 0 must survive
        if resident and self._reserved >= nt and self.n_acc == nt and same and decimate:
            w0 = layers[0][0] if layers[0].shape[0] == 1 else layers[0]          # (nchan,): one window for every baseline
            sky = _ResidentLags(ctx, nt, w0, pad)
            lags = sky.lags
        else:
            cube = NP.asarray(self.skyvis_freq, dtype=NP.complex128)
            with _through_slot0(ctx, resident):
                sky, lags = transform(cube)

        # (the reference multiplies vis_freq / vis_noise_freq unconditionally and fails on a noiseless object, SURVEY Q20: here the
        # cubes that exist are transformed)
        vis_lag = vis_noise_lag = None
        if self.vis_freq is not None:
            with _through_slot0(ctx, resident):
                vis_lag = transform(NP.asarray(self.vis_freq, dtype=NP.complex128))[0]
        if self.vis_noise_freq is not None:
            with _through_slot0(ctx, resident):
                vis_noise_lag = transform(NP.asarray(self.vis_noise_freq, dtype=NP.complex128))[0]

        def make_kernel():
            with _through_slot0(ctx, resident):
                if same:
                    # the transform of bp * bp_wts (:8119 / :8127) is the same for every snapshot then: one FFT batch, repeated
                    return NP.repeat(transform(NP.ones((nbl, nchan, 1), dtype=NP.complex128))[0], nt, axis=2)
                return transform(NP.ones((nbl, nchan, nt), dtype=NP.complex128))[0]
        return sky, lags, vis_lag, vis_noise_lag, make_kernel


class _Epoch(object):
    """What a frame_provider reads of a sky model: its epoch."""

    def __init__(self, epoch):
        self.epoch = epoch


class ApertureSynthesis(object):
    """Aperture synthesis of the visibilities of an InterferometerArray: the reference's ApertureSynthesis (prisim/interferometry.py
    :8990-9255) -- constructor, genUVW, reorderUVW, with its attributes and exceptions -- and what its docstring promises and its body
    does not reach: the dirty image and the synthesized beam of a run, by the direct Fourier sum on the GPU (include/prisim_imaging.h),
    the exact adjoint of the sky-sum with the same phase, phase centres and frames as observe().

    Attributes as in the reference (:9136-9163): ia, f, df, n_acc, lst, phase_center, phase_center_coords, pointing_center,
    pointing_coords, baselines, timestamp, latitude, blxyz, uvw_lambda, uvw, blc, trc, grid_blc, grid_trc, gridu, gridv, gridw,
    grid_ready; and image_stats, the statistics of the last image(), psf(), clean(), mosaic(), clean_mosaic() or
    clean_cotton_schwab(); and precision, 'double' or 'single', the arithmetic of image(), psf() and mosaic() (see image()); the
    clean*() methods do not read it and stay fp64.

    Departures from the reference: setUVWgrid is not ported -- its grid comes from GRD.grid_3d, whose source is not part of the
    reference tree, and the direct transform needs no grid; grid_ready stays False.  genUVW with a 'radec' phase centre takes
    HA = LST - RA and the centre's declination, as _pc_dircos and project_baselines do (the reference puts HA = LST and Dec = 0, :9180).
    image(), psf(), clean() (Hogbom's CLEAN of image() with the exact beam, include/prisim_imclean.h), mosaic() (the beam-weighted
    mosaic of the snapshots, horizon mask included: true fluxes where image() gives apparent ones, include/prisim_mosaic.h),
    clean_mosaic() (CLEAN of that mosaic, include/prisim_mosclean.h), clean_cotton_schwab() (clean() in major and minor cycles,
    include/prisim_csclean.h) and dircos_grid() are additions.
    There is no CPU path."""

    def __init__(self, interferometer_array=None):
        if interferometer_array is None:
            raise NameError('No input interferometer_array provided')
        if not isinstance(interferometer_array, InterferometerArray):
            raise TypeError('Input interferometer_array must be an instance of class InterferometerArray')
        ia = self.ia = interferometer_array
        self.f = ia.channels
        self.df = ia.freq_resolution
        self.n_acc = ia.n_acc
        self.lst = ia.lst
        self.phase_center = ia.phase_center
        self.pointing_center = ia.pointing_center
        self.phase_center_coords = ia.phase_center_coords
        self.pointing_coords = ia.pointing_coords
        self.baselines = ia.baselines
        self.timestamp = ia.timestamp
        self.latitude = ia.latitude
        self.blxyz = GEOM.enu2xyz(self.baselines, self.latitude, units='degrees')
        self.uvw_lambda = None
        self.uvw = None
        self.blc, self.trc = NP.zeros(2), NP.zeros(2)
        self.grid_blc, self.grid_trc = NP.zeros(2), NP.zeros(2)
        self.gridu, self.gridv, self.gridw = None, None, None
        self.grid_ready = False
        self.image_stats = None
        self.precision = 'double'                                     # of image(), psf() and mosaic(): 'double', or 'single' for the fp32 routes

    def genUVW(self):
        """(u, v, w) of every baseline phased to the phase centre of every snapshot: uvw_lambda (nbl, 3, n_acc) in metres and uvw
        (nbl, 3, nchan, n_acc) in wavelengths (:9167-9195), with the rotation project_baselines carries (:7979-7981)."""
        pc = NP.asarray(self.phase_center, dtype=NP.float64).reshape(-1, 2)
        if self.phase_center_coords == 'hadec':
            hadec = pc
        elif self.phase_center_coords == 'radec':
            hadec = NP.stack((NP.asarray(self.lst, dtype=NP.float64) - pc[:, 0], pc[:, 1]), axis=1)
        elif self.phase_center_coords == 'altaz':
            hadec = GEOM.altaz2hadec(pc, self.latitude, units='degrees')
        else:
            raise ValueError('Attribute phase_center_coords must be set to one of "hadec", "radec" or "altaz"')
        ha, dec = NP.radians(hadec[:, 0]), NP.radians(hadec[:, 1])
        rot = NP.asarray([[NP.sin(ha), NP.cos(ha), NP.zeros(ha.size)],
                          [-NP.sin(dec) * NP.cos(ha), NP.sin(dec) * NP.sin(ha), NP.cos(dec)],
                          [NP.cos(dec) * NP.cos(ha), -NP.cos(dec) * NP.sin(ha), NP.sin(dec)]])
        self.uvw_lambda = NP.einsum('bk,jkt->bjt', self.blxyz, rot)
        wl = C_LIGHT / NP.asarray(self.f, dtype=NP.float64)
        self.uvw = self.uvw_lambda[:, :, NP.newaxis, :] / wl.reshape(1, 1, -1, 1)

    def reorderUVW(self):
        """uvw (nbl, 3, nchan, n_acc) as (3, nbl * nchan * n_acc) (:9208-9210)."""
        return NP.swapaxes(self.uvw, 0, 1).reshape(3, -1)

    @staticmethod
    def dircos_grid(n, half_width):
        """The (n * n, 3) East-North-Up direction cosines of a regular n x n grid in (l, m) over [-half_width, half_width]^2, row-major
        in m then l (l fastest), the third from sqrt(1 - l^2 - m^2).  half_width <= 1 / sqrt(2) keeps every corner on the sphere."""
        n = int(n)
        if n < 1:
            raise ValueError('n must be at least 1')
        if not (0.0 <= half_width <= NP.sqrt(0.5)):
            raise ValueError('half_width must lie in [0, 1/sqrt(2)]')
        ax = NP.linspace(-float(half_width), float(half_width), n) if n > 1 else NP.zeros(1)
        m, l = NP.meshgrid(ax, ax, indexing='ij')
        l, m = l.ravel(), m.ravel()
        return NP.stack((l, m, NP.sqrt(NP.maximum(0.0, 1.0 - l * l - m * m))), axis=1)

    def _directions(self, directions, coords, epoch):
        """(unit vectors (npix, 3) in their own frame, rotations (nt, 3, 3), aberration (nt, 3) or None)"""
        ia, nt = self.ia, len(self.ia.lst)
        d = NP.asarray(directions, dtype=NP.float64)
        if d.ndim == 1:
            d = d.reshape(1, -1)
        if d.ndim != 2 or d.shape[0] < 1:
            raise ValueError('directions must be a (npix, 2) or (npix, 3) array')
        if coords == 'dircos':
            if d.shape[1] not in (2, 3):
                raise ValueError('Dimensions incompatible for direction cosine positions')
            if NP.any(NP.sqrt(NP.sum(d ** 2, axis=1)) > 1.0 + 1e-12):
                raise ValueError('direction cosines found to be exceeding unit magnitude.')
            if d.shape[1] == 2:
                d = NP.hstack((d, NP.sqrt(NP.maximum(0.0, 1.0 - NP.sum(d ** 2, axis=1))).reshape(-1, 1)))
            return d, NP.repeat(NP.eye(3)[NP.newaxis], nt, axis=0), None
        if coords not in ('altaz', 'hadec', 'radec'):
            raise ValueError('coords must be "altaz", "hadec", "radec" or "dircos"')
        if d.shape[1] != 2:
            raise ValueError('directions in {0} must be a (npix, 2) array of degrees'.format(coords))
        uv = GEOM.catalog_unitvec(d, coords)
        if coords == 'altaz':
            return uv, NP.repeat(NP.eye(3)[NP.newaxis], nt, axis=0), None
        if coords == 'hadec':
            return uv, NP.repeat(FRAMES.hadec_to_enu(ia.latitude)[NP.newaxis], nt, axis=0), None
        rot, beta = [], []
        for t in range(nt):                                            # what observe() applies to a 'radec' sky (_snapshot_frame)
            if ia.frame_provider is not None:
                r, b = ia.frame_provider(ia.timestamp[t], ia.lst[t], _Epoch(epoch))
            else:
                r, b = FRAMES.snapshot_frame('radec', ia.lst[t], ia.latitude, jd=ia.timestamp[t], epoch=epoch, model=ia.frame_model)
            rot.append(NP.asarray(r, dtype=NP.float64).reshape(3, 3))
            beta.append(NP.asarray(b, dtype=NP.float64).reshape(3))
        return uv, NP.stack(rot), NP.stack(beta)

    def _prepare(self, kind, directions, coords, datakey, weights, epoch, route):
        """What image(), psf() and clean() hand to the context: (unit vectors, rotations, aberration or None, phase centres, weights
        snapshot-major or None, cube snapshot-major or None for the resident one -- and for the beam, which reads none)."""
        ia = self.ia
        nt = len(ia.lst)
        if nt < 1:
            raise ValueError('no snapshots: call observe() first')
        if route not in ('auto', 'direct', 'stepped'):
            raise ValueError("route must be 'auto', 'direct' or 'stepped'")
        uv, rot, beta = self._directions(directions, coords, epoch)
        nbl, nchan = ia.baselines.shape[0], ia.channels.size
        w = None
        if weights is not None:
            w = NP.asarray(weights, dtype=NP.float64)
            if w.shape == (nbl, nchan, nt):
                w = NP.ascontiguousarray(NP.transpose(w, (2, 0, 1)))
            elif w.shape != (nbl,):
                raise ValueError('weights must be None, (nbl,) or (nbl, nchan, n_acc)')
        cube = None
        if kind == 'dirty':
            names = {'noiseless': 'skyvis_freq', 'noisy': 'vis_freq', 'noise': 'vis_noise_freq'}
            if datakey not in names:
                raise ValueError("datakey must be 'noiseless', 'noisy' or 'noise'")
            # the noiseless cube is read where it lies when the device slots [0, nt) hold skyvis_freq itself, in fp64 (_closure_prepare)
            snaps = getattr(ia, '_cube', None) or []
            resident = datakey == 'noiseless' and len(snaps) == nt and bool(ia._device_in_step) and nt <= ia._reserved and all(
                sn.dtype == NP.complex128 and (not isinstance(sn, _DeviceSlot) or sn.slot == i) for i, sn in enumerate(snaps))
            if not resident:
                vis = getattr(ia, names[datakey])
                if vis is None:
                    raise ValueError('no {0}: the array holds no such visibilities'.format(names[datakey]))
                vis = NP.asarray(vis)
                if vis.shape != (nbl, nchan, nt):
                    raise ValueError('{0} must have shape (nbl, nchan, n_acc)'.format(names[datakey]))
                cube = NP.ascontiguousarray(NP.transpose(vis, (2, 0, 1)), dtype=NP.complex128)
        pc = ia._pc_dircos(ia.phase_center, ia.phase_center_coords)
        return uv, rot, beta, pc, w, cube

    def _precision_keyword(self, route):
        """(the attribute `precision`, the keyword that selects it at the context) for image(), psf() and mosaic(): {} for 'double',
        which calls the context as ever; for 'single' what the fp32 entries refuse is refused here, before any device work."""
        precision = self.precision
        if precision not in ('double', 'single'):
            raise ValueError("precision must be 'double' or 'single'")
        if precision == 'double':
            return precision, {}
        if route == 'direct':
            raise ValueError("precision='single' has no direct route: use route='auto' or 'stepped', or precision='double'")
        f = NP.asarray(self.ia.channels, dtype=NP.float64).ravel()
        line = f[0] + NP.arange(f.size) * ((f[-1] - f[0]) / (f.size - 1) if f.size > 1 else 0.0)
        if not NP.all(NP.abs(f - line) <= 1e-7):                      # the uniform-grid rule of include/prisim_imaging.h
            raise ValueError("precision='single' needs a uniform channel grid: use precision='double'")
        return precision, {'precision': 'single'}

    def _synthesize(self, kind, directions, coords, datakey, weights, chan_avg, epoch, route, budget_bytes):
        ia = self.ia
        uv, rot, beta, pc, w, cube = self._prepare(kind, directions, coords, datakey, weights, epoch, route)
        precision, single = self._precision_keyword(route)
        image, wsum, st = ia._ctx.dirty_image(uv, rot, pc, ia._baselines_local(), ia.channels, cube=cube, weights=w, kind=kind,
                                              chan_avg=bool(chan_avg), aberr_beta=beta, route=route, budget_bytes=int(budget_bytes or 0),
                                              **single)
        self.image_stats = dict(st, wsum=wsum, precision=precision)
        return image

    def image(self, directions, coords='dircos', datakey='noiseless', weights=None, chan_avg=False, epoch=None, route='auto',
              budget_bytes=None):
        """The dirty image of the array's visibilities at the given directions, (npix, nchan) float64 or (npix,) with chan_avg: per
        channel sum_{t,b} w Re(V e^{+i phi}) / sum_{t,b} w with phi = 2 pi f b . (s - s0) / c, s0 the array's phase centre of the
        snapshot.  In the units of the visibilities per beam: a point source of flux S seen through a delta beam images to S at its own
        direction.  No horizon test is made, and a channel whose weights are all zero is NaN.

        directions   (npix, 2) degrees for coords 'altaz' (alt, az), 'hadec' and 'radec'; (npix, 2 | 3) for 'dircos' (East-North-Up).
                     'radec' directions go through the frame observe() applies to a 'radec' sky (frame_model, or frame_provider when
                     set) at every snapshot's LST and timestamp, with epoch= the epoch of the coordinates (None: of date): an image of
                     a simulated catalogue shows its sources at the catalogue's positions.
        datakey      'noiseless' (skyvis_freq), 'noisy' (vis_freq) or 'noise' (vis_noise_freq).  The noiseless cube is read where it
                     lies on the device when the device slots are in step with skyvis_freq (reserve()); otherwise the cube is handed over.
        weights      None, (nbl,) or (nbl, nchan, n_acc): finite and non-negative.
        route        'auto', 'direct' or 'stepped' (include/prisim_imaging.h); budget_bytes: device bytes of the streamed buffers.
        The attribute `precision` of the object, 'double' by default, selects the arithmetic of image() and psf(): set to 'single' they
        take the fp32 route (include/prisim_imaging32.h): every element within 5e-6 of sum w|V| / sum w of the fp64 image, the phases
        still fp64 so that long baselines cost nothing.  It takes a uniform channel grid and route 'auto' or 'stepped'; anything else
        is a ValueError before any device work.  It is an attribute and no keyword: the parameter lists of these methods are pinned.
        The entry's statistics, 'wsum' and 'precision' are left in image_stats."""
        return self._synthesize('dirty', directions, coords, datakey, weights, chan_avg, epoch, route, budget_bytes)

    def psf(self, directions, coords='dircos', weights=None, chan_avg=False, epoch=None, route='auto', budget_bytes=None):
        """The synthesized beam at the given directions: image() of V = 1, centred on every snapshot's phase centre, where it is 1.
        The attribute `precision` selects the arithmetic as it does for image()."""
        return self._synthesize('psf', directions, coords, None, weights, chan_avg, epoch, route, budget_bytes)

    def mosaic(self, directions, coords='dircos', datakey='noiseless', weights=None, chan_avg=False, epoch=None, telescope=None,
               pb_info=None, pbmin=0.1, route='auto', budget_bytes=None):
        """The beam-weighted linear mosaic of the snapshots at the given directions, on the GPU (include/prisim_mosaic.h), (npix, nchan)
        float64 or (npix,) with chan_avg: sum_t A_t D_t / sum_t A_t^2 W_t, with D_t the unnormalised image() of snapshot t alone, W_t
        its weight sum and A_t the power pattern of the primary beam at the direction in that snapshot, 0 below the horizon.  Where
        image() gives apparent fluxes, this gives true ones: a source of flux S simulated through the beam comes back as S at its own
        direction for any number of snapshots, any drift of the beam across the sky and any chromaticity of the beam.

        directions, coords, datakey, weights, chan_avg, epoch, route, budget_bytes as image() takes them; the noiseless cube is read
        where it lies on the device under the same condition.
        telescope    the dictionary of the beam; None: the array's own (ia.telescope), the beam the visibilities were simulated with.
        pb_info      the pointing_info of a phased array's beamformer, as observe() takes it: None, one dictionary, or a sequence of one
                     per snapshot (observe() takes one per call).  The beam of snapshot t is primary_beams.device_beam_spec at the
                     pointing observe() used; what differs between the snapshots -- the element's pointing, the beamformer's delays --
                     goes to the device per snapshot.
        pbmin        in [0, 1): where the effective beam pb_eff = sqrt(sum_t A_t^2 W_t / sum_t W_t) is below it the mosaic is NaN (the
                     usual 'pblimit'; 0.1 is a convention, not a measured value).  0 masks only what no snapshot saw at all.
        The noise of the mosaic goes as 1 / pb_eff.  num, den (npix, nchan), wsum (nchan,), pb_eff (the mosaic's shape), 'precision'
        and the entry's statistics are left in image_stats.
        The attribute `precision` of the object selects the arithmetic as it does for image(): set to 'single', every snapshot's sum
        D_t takes the fp32 route (include/prisim_mosaic32.h) while the beam, the weight sums and the sums over t stay fp64, so den,
        wsum, pb_eff and the mask have the bits of 'double' and num is within 5e-6 sum_t A_t sum_b w|V| of it.  It takes a uniform
        channel grid and route 'auto' or 'stepped'; anything else is a ValueError before any device work.

        Raises NotImplementedError for an array with an external beam (set_external_beam) and for the apertures device_beam_spec
        does not carry (rect, square)."""
        ia = self.ia
        if getattr(ia, '_extbeam', None) is not None:
            raise NotImplementedError('mosaic() evaluates the analytic beams; the array has an external beam (set_external_beam)')
        pbmin = float(pbmin)
        if not (0.0 <= pbmin < 1.0):
            raise ValueError('pbmin must lie in [0, 1)')
        uv, rot, beta, pc, w, cube = self._prepare('dirty', directions, coords, datakey, weights, epoch, route)
        precision, single = self._precision_keyword(route)
        kind, dia, bpc, ext = self._beam_specs(telescope, pb_info)
        image, num, den, wsum, st = ia._ctx.mosaic_image(uv, rot, pc, ia._baselines_local(), ia.channels, kind, dia, beam_pc_dircos=bpc,
                                                         ext=ext, cube=cube, weights=w, chan_avg=bool(chan_avg), aberr_beta=beta,
                                                         pbmin=pbmin, route=route, budget_bytes=int(budget_bytes or 0), **single)
        self.image_stats = dict(st, num=num, den=den, wsum=wsum, precision=precision)
        return image

    def _beam_specs(self, telescope, pb_info):
        """The beam of the snapshots as mosaic_image and clean_mosaic take it: (kind, size, beam_pc_dircos (3,) or (nt, 3), ext None, a
        dict or one dict per snapshot), from primary_beams.device_beam_spec at the pointing observe() used in every snapshot."""
        ia = self.ia
        tel = ia.telescope if telescope is None else telescope
        nt = len(ia.lst)
        infos = list(pb_info) if isinstance(pb_info, (list, tuple)) else [pb_info] * nt
        if len(infos) != nt:
            raise ValueError('pb_info must be None, one dictionary or one per snapshot')
        specs = []
        for t in range(nt):
            pc_altaz = ia._pointing(ia.pointing_center[t], ia.lst[t])[1]
            specs.append(PB.device_beam_spec(tel, pointing_info=infos[t], pointing_center=pc_altaz, first_frequency_hz=float(ia.channels[0])))
        # one shared description unless the pointing moves: then the element's pointing, a beamformer's delays, or both go per snapshot
        kind, dia, bpc, ext = specs[0]
        if not all(_same_beam_spec(specs[0][:2], sp[:2]) for sp in specs[1:]):
            raise ValueError('the snapshots must share one kind and size of beam')
        if not all(_same_beam_spec(bpc, sp[2]) for sp in specs[1:]):
            bpc = NP.stack([NP.asarray(sp[2], dtype=NP.float64).ravel() for sp in specs])
        if not all(_same_beam_spec(ext, sp[3]) for sp in specs[1:]):
            ext = [sp[3] for sp in specs]
        return kind, dia, bpc, ext

    def clean(self, directions, coords='dircos', datakey='noiseless', weights=None, chan_avg=False, epoch=None, gain=0.1, maxiter=10000,
              threshold=5e-3, threshold_type='relative', window=None, fwhm=None, restore=True, route='auto', budget_bytes=None):
        """Hogbom CLEAN of image() with the exact beam, on the GPU (include/prisim_imclean.h): per channel (or for the band's image with
        chan_avg) and iteration, the pixel of the largest |residual| inside the window becomes a component of gain times its value,
        and the dirty image of that component's own visibilities -- the synthesized beam at that very place, w-term and frames
        included, no shift invariance assumed -- is subtracted from every pixel.  The residual therefore always is the dirty image
        of the visibilities less those of the components.  A channel ends when its peak is at or below the threshold or when it
        holds maxiter components; a channel whose weights are all zero is NaN and holds none.

        directions, coords, datakey, weights, chan_avg, epoch, route as image() takes them; the noiseless cube is read where it lies
        on the device under the same condition.
        gain, maxiter, threshold, threshold_type   as complex1dClean takes them, with its checks and exceptions: gain a float in
                     (0, 1), maxiter a positive int, threshold a positive scalar, below 1 when threshold_type is 'relative' (a
                     fraction of the channel's first peak) rather than 'absolute'.
        window       None, or (npix,) booleans: the pixels that may hold components.  Every pixel is updated all the same.
        fwhm         the restoring beam in degrees, a scalar or (nc,).  None: c / (f max|b|) radians per channel, at the mean frequency
                     with chan_avg -- a convention (the diffraction scale of the longest baseline), not a fit to the synthesized beam.
        restore      False: no restored image.
        budget_bytes device bytes the resident image may take (None: 1 GiB); an image that does not fit is refused, not streamed.
        Returns a dict: 'residual' and 'restored' (None without restore) (npix, nchan) or (npix,); 'model', of the same shape, the
        component fluxes summed per pixel; 'components' {'pixel' int32, 'flux' (nc, longest list; -1 and 0 past a channel's own),
        'count' (nc,)}; 'status' (nc,) of _abi.PRISIM_IMCLEAN_THRESHOLD, _MAXITER or _DEAD; 'peak0' and 'threshold' (nc,) the first peak
        and the level the channel was cleaned to; 'fwhm' (nc,) degrees.  The entry's statistics, and 'wsum', are left in image_stats."""
        from . import delay_spectrum as DS                            # (imports this module)
        threshold = DS._check_clean_args(threshold_type, threshold, gain, maxiter)
        DS._check_gain_maxiter(gain, maxiter)
        ia = self.ia
        uv, rot, beta, pc, w, cube = self._prepare('dirty', directions, coords, datakey, weights, epoch, route)
        npix, nchan = uv.shape[0], ia.channels.size
        nc = 1 if chan_avg else nchan
        bl = ia._baselines_local()
        win, fwhm_rad = self._window_and_fwhm(window, fwhm, npix, nc, chan_avg, bl)
        r = ia._ctx.clean_image(uv, rot, pc, bl, ia.channels, cube=cube, weights=w, chan_avg=bool(chan_avg), aberr_beta=beta,
                                gain=gain, maxiter=maxiter, threshold=threshold, threshold_relative=threshold_type == 'relative',
                                window=win, fwhm_rad=fwhm_rad if restore else None, route=route, budget_bytes=int(budget_bytes or 0))
        self.image_stats = dict(r['stats'], wsum=r['wsum'])
        return self._clean_dict(r, npix, nc, chan_avg, restore, threshold, threshold_type, fwhm_rad)

    def clean_cotton_schwab(self, directions, grid_shape, coords='dircos', datakey='noiseless', weights=None, chan_avg=False, epoch=None,
                            gain=0.1, maxiter=10000, threshold=5e-3, threshold_type='relative', cycle_depth=0.3, cycle_niter=None,
                            max_major=32, window=None, fwhm=None, restore=True, return_vis=False, route='auto', minor_route='auto',
                            budget_bytes=None):
        """Cotton-Schwab CLEAN of image(), on the GPU (include/prisim_csclean.h): clean() pays a full direct Fourier pass for every
        component; this pays one per major cycle.  A minor cycle cleans one channel's residual in image space with a shift-invariant
        beam -- the synthesized beam at the offsets of the lattice grid_shape, without the curvature of the grid or aberration -- down
        to cycle_depth of the cycle's first peak; the major cycle then takes the new components out of the residual visibilities
        with their exact phases and images those again.  So after every major cycle, and at the end, the residual is the dirty image
        of the visibilities less those of the components, as clean()'s is.

        directions, coords, datakey, weights, chan_avg, epoch, gain, maxiter, threshold, threshold_type, window, fwhm, restore, route
        and budget_bytes as clean() takes them.
        grid_shape   (ny, nx) with ny * nx = npix: the directions as ny rows of nx, nx fastest, as dircos_grid(n, hw) lays them out
                     with ny = nx = n.  Any list of directions is accepted, because the major cycle is exact for all of them; only
                     the speed of convergence depends on the list being a lattice, for which the minor cycle's beam is a good one.
        cycle_depth  in (0, 1): 0.3 is a convention.  A deeper cycle (a smaller value) saves major cycles and trusts the approximate
                     beam further; with a beam that is several per cent off, 0.1 picks stray pixels where 0.3 does not.
        cycle_niter  None, or components per channel and minor cycle at most (a positive int).
        max_major    major cycles at most, 0 .. 65536.  A channel that wants more ends with _abi.PRISIM_CSCLEAN_MAJOR; one whose peak
                     grew from one cycle to the next with PRISIM_CSCLEAN_DIVERGED, its components kept and its residual still exact.
        return_vis   True: the residual visibilities are returned.
        minor_route  'auto', 'lds' or 'global': where the working image of a minor cycle lives; no result depends on it.
        Returns the dict of clean() and 'cycles': {'count' (nc,) the minor cycles a channel ran, 'ncomp' (nc, most cycles; -1 past a
        channel's own) the components it held at the end of each, 'peak' (nc, most cycles + 1; NaN past a channel's own) its peak at the
        start of each and at the test that ended it}, and 'residual_vis' (nbl, nchan, n_acc) complex128 or None.  The entry's
        statistics, and 'wsum', are left in image_stats."""
        from . import delay_spectrum as DS                            # (imports this module)
        threshold = DS._check_clean_args(threshold_type, threshold, gain, maxiter)
        DS._check_gain_maxiter(gain, maxiter)
        if not isinstance(cycle_depth, float) or not (0.0 < cycle_depth < 1.0):
            raise ValueError('cycle_depth must be a float in (0, 1)')
        if cycle_niter is not None and (not isinstance(cycle_niter, (int, NP.integer)) or isinstance(cycle_niter, bool) or cycle_niter < 1):
            raise ValueError('cycle_niter must be None or a positive int')
        if not isinstance(max_major, (int, NP.integer)) or isinstance(max_major, bool) or not (0 <= max_major <= 65536):
            raise ValueError('max_major must be an int in [0, 65536]')
        if minor_route not in ('auto', 'lds', 'global'):
            raise ValueError("minor_route must be 'auto', 'lds' or 'global'")
        ia = self.ia
        uv, rot, beta, pc, w, cube = self._prepare('dirty', directions, coords, datakey, weights, epoch, route)
        npix, nchan = uv.shape[0], ia.channels.size
        try:
            ny, nx = (int(n) for n in grid_shape)
        except (TypeError, ValueError):
            raise ValueError('grid_shape must be (ny, nx)')
        if ny < 1 or nx < 1 or ny * nx != npix:
            raise ValueError('grid_shape must be (ny, nx) with ny * nx the number of directions')
        nc = 1 if chan_avg else nchan
        bl = ia._baselines_local()
        win, fwhm_rad = self._window_and_fwhm(window, fwhm, npix, nc, chan_avg, bl)
        r = ia._ctx.clean_image_cs(uv, (ny, nx), rot, pc, bl, ia.channels, cube=cube, weights=w, chan_avg=bool(chan_avg), aberr_beta=beta,
                                   gain=gain, maxiter=maxiter, threshold=threshold, threshold_relative=threshold_type == 'relative',
                                   cycle_depth=cycle_depth, cycle_niter=int(cycle_niter or 0), max_major=int(max_major), window=win,
                                   fwhm_rad=fwhm_rad if restore else None, route=route, minor_route=minor_route,
                                   budget_bytes=int(budget_bytes or 0), want_vis=bool(return_vis))
        self.image_stats = dict(r['stats'], wsum=r['wsum'])
        out = self._clean_dict(r, npix, nc, chan_avg, restore, threshold, threshold_type, fwhm_rad)
        out['cycles'] = {'count': NP.asarray(r['ncycles']), 'ncomp': r['cycle_ncomp'], 'peak': r['cycle_peak']}
        out['residual_vis'] = NP.ascontiguousarray(NP.transpose(r['vres'], (1, 2, 0))) if return_vis else None
        return out

    def _window_and_fwhm(self, window, fwhm, npix, nc, chan_avg, bl):
        """(the window as booleans or None, the restoring beam (nc,) in radians) of clean() and clean_mosaic(), with their checks"""
        win = None
        if window is not None:
            win = NP.asarray(window)
            if win.shape != (npix,):
                raise ValueError('window must be None or (npix,)')
            win = win != 0
            if not win.any():
                raise ValueError('window holds no pixel')
        if fwhm is None:
            f = NP.asarray(self.ia.channels, dtype=NP.float64)
            longest = float(NP.sqrt(NP.max(NP.sum(NP.asarray(bl, dtype=NP.float64) ** 2, axis=1))))
            if not longest > 0.0:
                raise ValueError('the default fwhm needs a baseline of non-zero length')
            fwhm_rad = C_LIGHT / ((NP.array([f.mean()]) if chan_avg else f) * longest)
        else:
            fwhm_rad = NP.radians(NP.asarray(fwhm, dtype=NP.float64))
            if fwhm_rad.ndim == 0:
                fwhm_rad = NP.full(nc, float(fwhm_rad))
            if fwhm_rad.shape != (nc,):
                raise ValueError('fwhm must be None, a scalar or ({0},)'.format(nc))
            if not NP.all(NP.isfinite(fwhm_rad) & (fwhm_rad > 0.0)):
                raise ValueError('fwhm must be positive and finite')
        return win, fwhm_rad

    @staticmethod
    def _clean_dict(r, npix, nc, chan_avg, restore, threshold, threshold_type, fwhm_rad):
        """What clean() and clean_mosaic() return alike, from the context's dict r"""
        count = NP.asarray(r['ncomp'])
        model = NP.zeros((npix, nc), dtype=NP.float64)
        for k in range(nc):
            NP.add.at(model[:, k], r['comp_pixel'][k, :count[k]], r['comp_flux'][k, :count[k]])
        peak0 = NP.asarray(r['peak0'])
        return {'residual': r['residual'], 'restored': r['restored'] if restore else None, 'model': model[:, 0] if chan_avg else model,
                'components': {'pixel': r['comp_pixel'], 'flux': r['comp_flux'], 'count': count}, 'status': r['status'], 'peak0': peak0,
                'threshold': threshold * peak0 if threshold_type == 'relative' else NP.full(nc, threshold), 'fwhm': NP.degrees(fwhm_rad)}

    def clean_mosaic(self, directions, coords='dircos', datakey='noiseless', weights=None, chan_avg=False, epoch=None, telescope=None,
                     pb_info=None, pbmin=0.1, gain=0.1, maxiter=10000, threshold=5e-3, threshold_type='relative', window=None, fwhm=None,
                     restore=True, route='auto', budget_bytes=None):
        """CLEAN of mosaic(), on the GPU (include/prisim_mosclean.h): a deconvolved sky in true fluxes for a drift scan through a
        chromatic beam, where clean() returns apparent fluxes and mosaic() leaves every source the sidelobes of every other one.  Per
        channel (or for the band with chan_avg) and iteration, the pixel of the largest |F| inside the window and the pbmin mask
        becomes a component of gain times the mosaic's value there -- F = num / sqrt(den wsum) is the flat-noise image, in the units
        and at the noise level of image(), so the search does not run to the rim of the beam --, and what the beam-weighted snapshots
        show of that component's own visibilities, as observe() would simulate them, is subtracted from the numerator of every pixel.
        The mosaic's value is the least-squares flux of a component at that pixel, so a step is one of matching pursuit: the weighted
        sum of |V - model|^2 cannot grow.

        directions, coords, datakey, weights, chan_avg, epoch, telescope, pb_info, pbmin, route as mosaic() takes them; gain, maxiter,
        threshold, threshold_type, window, fwhm, restore, budget_bytes as clean() takes them, the threshold in the units of F.
        Returns the dict of clean() -- 'residual' and 'restored' in true fluxes, NaN where the mosaic is masked; 'model' and the
        components' fluxes true fluxes; 'peak0' and 'threshold' in the units of F -- and 'residual_flat', F of the final residual.
        num (the final numerator), den, wsum, pb_eff and the entry's statistics are left in image_stats.

        Raises NotImplementedError for an array with an external beam (set_external_beam) and for the apertures device_beam_spec
        does not carry (rect, square)."""
        from . import delay_spectrum as DS                            # (imports this module)
        ia = self.ia
        if getattr(ia, '_extbeam', None) is not None:
            raise NotImplementedError('clean_mosaic() evaluates the analytic beams; the array has an external beam (set_external_beam)')
        threshold = DS._check_clean_args(threshold_type, threshold, gain, maxiter)
        DS._check_gain_maxiter(gain, maxiter)
        pbmin = float(pbmin)
        if not (0.0 <= pbmin < 1.0):
            raise ValueError('pbmin must lie in [0, 1)')
        uv, rot, beta, pc, w, cube = self._prepare('dirty', directions, coords, datakey, weights, epoch, route)
        kind, dia, bpc, ext = self._beam_specs(telescope, pb_info)
        npix, nchan = uv.shape[0], ia.channels.size
        nc = 1 if chan_avg else nchan
        bl = ia._baselines_local()
        win, fwhm_rad = self._window_and_fwhm(window, fwhm, npix, nc, chan_avg, bl)
        r = ia._ctx.clean_mosaic(uv, rot, pc, bl, ia.channels, kind, dia, beam_pc_dircos=bpc, ext=ext, cube=cube, weights=w,
                                 chan_avg=bool(chan_avg), aberr_beta=beta, pbmin=pbmin, gain=gain, maxiter=maxiter, threshold=threshold,
                                 threshold_relative=threshold_type == 'relative', window=win, fwhm_rad=fwhm_rad if restore else None,
                                 route=route, budget_bytes=int(budget_bytes or 0))
        self.image_stats = dict(r['stats'], num=r['num'], den=r['den'], wsum=r['wsum'], pb_eff=r['pb_eff'])
        return dict(self._clean_dict(r, npix, nc, chan_avg, restore, threshold, threshold_type, fwhm_rad), residual_flat=r['residual_flat'])

    def clean_mosaic_cotton_schwab(self, directions, grid_shape, coords='dircos', datakey='noiseless', weights=None, chan_avg=False, epoch=None,
                                   telescope=None, pb_info=None, pbmin=0.1, gain=0.1, maxiter=10000, threshold=5e-3, threshold_type='relative',
                                   window=None, fwhm=None, restore=True, cycle_depth=0.3, cycle_niter=None, max_major=32, return_vis=False,
                                   route='auto', minor_route='auto', budget_bytes=None):
        """Cotton-Schwab CLEAN of mosaic(), on the GPU (include/prisim_moscs.h): clean_mosaic() pays a full mosaic pass over all
        snapshots for every component; this pays one per major cycle, as clean_cotton_schwab() does for clean().  A minor cycle cleans
        the flat-noise image F = num / sqrt(den wsum) of one channel with the shift-invariant beam of the lattice grid_shape: in F a
        component answers with at most its own amplitude anywhere, and near its pixel with the synthesized beam, so the step of
        clean_cotton_schwab() serves; each component is listed with its true flux.  The major cycle then takes the new components out
        of the residual visibilities through the beam of every snapshot, as observe() would simulate them, and forms the mosaic's
        numerator of those again: what the minor cycle's beam leaves out -- the drift and chromaticity of the beam, the curvature of
        the grid, aberration, the w-term -- is corrected there, and after every major cycle, and at the end, the residual is the
        mosaic of the visibilities less those of the components, as clean_mosaic()'s is.

        directions, coords, datakey, weights, chan_avg, epoch, telescope, pb_info, pbmin, gain, maxiter, threshold, threshold_type,
        window, fwhm, restore, route and budget_bytes as clean_mosaic() takes them; grid_shape, cycle_depth, cycle_niter, max_major,
        return_vis and minor_route as clean_cotton_schwab() takes them.
        Returns the dict of clean_mosaic() -- 'status' may also hold _abi.PRISIM_CSCLEAN_MAJOR or _DIVERGED -- and 'cycles': {'count'
        (nc,), 'ncomp' (nc, most cycles; -1 past a channel's own), 'peak' (nc, most cycles + 1; NaN past a channel's own, in the units
        of F)}, and 'residual_vis' (nbl, nchan, n_acc) complex128 or None.  num (the mosaic's numerator of the residual visibilities),
        den, wsum, pb_eff and the entry's statistics are left in image_stats.

        Raises NotImplementedError for an array with an external beam (set_external_beam) and for the apertures device_beam_spec
        does not carry (rect, square)."""
        from . import delay_spectrum as DS                            # (imports this module)
        ia = self.ia
        if getattr(ia, '_extbeam', None) is not None:
            raise NotImplementedError('clean_mosaic_cotton_schwab() evaluates the analytic beams; the array has an external beam '
                                      '(set_external_beam)')
        threshold = DS._check_clean_args(threshold_type, threshold, gain, maxiter)
        DS._check_gain_maxiter(gain, maxiter)
        pbmin = float(pbmin)
        if not (0.0 <= pbmin < 1.0):
            raise ValueError('pbmin must lie in [0, 1)')
        if not isinstance(cycle_depth, float) or not (0.0 < cycle_depth < 1.0):
            raise ValueError('cycle_depth must be a float in (0, 1)')
        if cycle_niter is not None and (not isinstance(cycle_niter, (int, NP.integer)) or isinstance(cycle_niter, bool) or cycle_niter < 1):
            raise ValueError('cycle_niter must be None or a positive int')
        if not isinstance(max_major, (int, NP.integer)) or isinstance(max_major, bool) or not (0 <= max_major <= 65536):
            raise ValueError('max_major must be an int in [0, 65536]')
        if minor_route not in ('auto', 'lds', 'global'):
            raise ValueError("minor_route must be 'auto', 'lds' or 'global'")
        uv, rot, beta, pc, w, cube = self._prepare('dirty', directions, coords, datakey, weights, epoch, route)
        kind, dia, bpc, ext = self._beam_specs(telescope, pb_info)
        npix, nchan = uv.shape[0], ia.channels.size
        try:
            ny, nx = (int(n) for n in grid_shape)
        except (TypeError, ValueError):
            raise ValueError('grid_shape must be (ny, nx)')
        if ny < 1 or nx < 1 or ny * nx != npix:
            raise ValueError('grid_shape must be (ny, nx) with ny * nx the number of directions')
        nc = 1 if chan_avg else nchan
        bl = ia._baselines_local()
        win, fwhm_rad = self._window_and_fwhm(window, fwhm, npix, nc, chan_avg, bl)
        r = ia._ctx.clean_mosaic_cs(uv, (ny, nx), rot, pc, bl, ia.channels, kind, dia, beam_pc_dircos=bpc, ext=ext, cube=cube, weights=w,
                                    chan_avg=bool(chan_avg), aberr_beta=beta, pbmin=pbmin, gain=gain, maxiter=maxiter, threshold=threshold,
                                    threshold_relative=threshold_type == 'relative', cycle_depth=cycle_depth,
                                    cycle_niter=int(cycle_niter or 0), max_major=int(max_major), window=win,
                                    fwhm_rad=fwhm_rad if restore else None, route=route, minor_route=minor_route,
                                    budget_bytes=int(budget_bytes or 0), want_vis=bool(return_vis))
        self.image_stats = dict(r['stats'], num=r['num'], den=r['den'], wsum=r['wsum'], pb_eff=r['pb_eff'])
        out = dict(self._clean_dict(r, npix, nc, chan_avg, restore, threshold, threshold_type, fwhm_rad), residual_flat=r['residual_flat'])
        out['cycles'] = {'count': NP.asarray(r['ncycles']), 'ncomp': r['cycle_ncomp'], 'peak': r['cycle_peak']}
        out['residual_vis'] = NP.ascontiguousarray(NP.transpose(r['vres'], (1, 2, 0))) if return_vis else None
        return out
