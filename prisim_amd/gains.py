"""Instrument gain tables: read_gaintable, extract_gains and GainInfo of prisim/interferometry.py (:333-632, :635-898, :2412-3860).

The host side keeps the reference's statements -- its argument checks, exceptions, label matching, broadcasting and axis orders --
and hands the evaluation to the device (include/prisim_gains.h): ``splinator`` fits scipy's splines exactly as the reference does and
packs their knots, coefficients and degrees; ``spline_gains`` evaluates them with FITPACK's B-spline recursion on the GPU,
``nearest_gains`` and ``eval_gains`` gather on the GPU from index maps the host forms with the readings of LKP.find_1NN and
NMO.find_list_in_list (prisim_amd/dsp_readings.py).  A gain is built from at most two device tables, one per gain kind, each
[nt][rows][nchan]; ``InterferometerArray.add_noise`` applies them to the visibility cube without forming a gain cube
(GainPlan), the standalone methods return the reference's (nbl, nchan, nt) arrays.

h5py is not used: files go through prisim_amd/hdf5io.py, read with h5py's conventions (complex compounds, strings as text).
Departure: ``interpolator`` / ``interpolate_gains`` are built on scipy.interpolate.interp2d, which scipy >= 1.14 removed; they raise
NotImplementedError and GainInfo() does not call ``interpolator``.
"""
import copy
import warnings

import numpy as NP

from . import _abi
from . import dsp_readings as R
from . import hdf5io

GAINKEYS = ('antenna-based', 'baseline-based')
AXES = ['label', 'frequency', 'time']


# ---- h5py-flavoured reading over hdf5io ----------------------------------------------------------------------------------------
def _text(v):
    """h5py under Python 2 (the reference's setting) hands out text: bytes, byte-string arrays and byte-string fields become str."""
    if isinstance(v, bytes):
        return v.decode()
    if isinstance(v, NP.ndarray):
        if v.dtype.kind == 'S':
            return NP.char.decode(v, 'utf-8')
        if v.dtype.kind == 'O':
            return NP.asarray([_text(x) for x in v.ravel()]).reshape(v.shape)
        if v.dtype.names:
            fields = [(n, 'U{0}'.format(max(v.dtype[n].itemsize, 1)) if v.dtype[n].kind == 'S' else v.dtype[n]) for n in v.dtype.names]
            out = NP.empty(v.shape, dtype=fields)
            for n in v.dtype.names:
                out[n] = _text(v[n])
            return out
    return v


class _Dataset(object):
    def __init__(self, f, path):
        self._f, self._path = f, path

    @property
    def value(self):
        return _text(self._f.read(self._path))


class _Group(object):
    def __init__(self, f, path):
        self._f, self._path = f, path

    def __getitem__(self, name):
        path = self._path + '/' + name
        if not self._f.exists(path):
            raise KeyError("Unable to open object (object '{0}' doesn't exist)".format(name))
        return _Dataset(self._f, path)

    def __contains__(self, name):
        return self._f.exists(self._path + '/' + name)

    def __iter__(self):
        return iter(self._f.list(self._path))


class H5File(object):
    """The read side of h5py.File that read_gaintable needs: iteration over the root's groups, grp[name].value, `name in grp`."""

    def __init__(self, path):
        if not isinstance(path, str):
            raise IOError('gains file name must be a string')
        try:
            self._f = hdf5io.File(path, 'r')
        except ValueError as exc:
            raise IOError(str(exc))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self._f.close()

    def __iter__(self):
        return iter(self._f.list('/'))

    def __getitem__(self, name):
        if not self._f.exists(name):
            raise KeyError(name)
        return _Group(self._f, name)


def _check_axes_order(axes_order):
    if not isinstance(axes_order, (list, NP.ndarray)):
        raise TypeError('axes_order must be a list')
    if len(axes_order) != 3:
        raise ValueError('axes_order must be a three element list')
    for orderkey in AXES:
        if orderkey not in axes_order:
            raise ValueError('axes_order does not contain key "{0}"'.format(orderkey))


# ---- module functions ---------------------------------------------------------------------------------------------------------
def read_gaintable(gainsfile, axes_order=None):
    """interferometry.py:333-632.  The gain table of an HDF5 file: {'antenna-based' | 'baseline-based': {'gains' (3-D, axes in
    axes_order, default ['label', 'frequency', 'time']), 'label', 'frequency', 'time' (None where the axis has length 1), 'ordering'}},
    or None (unity gains) when the file cannot be read or holds no group."""
    if axes_order is None:
        axes_order = list(AXES)
    else:
        _check_axes_order(axes_order)
    gaintable = {}
    try:
        with H5File(gainsfile) as fileobj:
            for gainkey in fileobj:
                try:
                    gaintable[gainkey] = {}
                    grp = fileobj[gainkey]
                    gval = grp['gains'].value
                    if isinstance(gval, (NP.float32, NP.float64, NP.complex64, NP.complex128)):
                        gaintable[gainkey]['gains'] = NP.asarray(gval).reshape(1, 1, 1)
                    elif isinstance(gval, NP.ndarray):
                        if 'ordering' in grp:
                            ordering = list(grp['ordering'].value)
                        else:
                            raise KeyError('Axes ordering for gains not specified')
                        if len(ordering) != 3:
                            raise ValueError('Ordering must contain three elements')
                        elif ('time' not in ordering) or ('label' not in ordering) or ('frequency' not in ordering):
                            raise ValueError('Required elements not found in ordering of instrument gains')
                        else:
                            if gval.ndim == 3:
                                transpose_order = R.find_list_in_list(ordering, axes_order)
                                gaintable[gainkey]['gains'] = NP.transpose(gval, axes=transpose_order)
                                for subkey in ['time', 'label', 'frequency']:
                                    gaintable[gainkey][subkey] = None
                                    sval = grp[subkey].value
                                    if isinstance(sval, NP.ndarray):
                                        if gaintable[gainkey]['gains'].shape[axes_order.index(subkey)] > 1:
                                            gaintable[gainkey][subkey] = NP.asarray(sval).ravel()
                                            if gaintable[gainkey][subkey].size != gaintable[gainkey]['gains'].shape[axes_order.index(subkey)]:
                                                raise ValueError('List of labels and the gains do not match in dimensions')
                                    else:
                                        raise TypeError('Value of key "{0}" in {1} gains must be a numpy array'.format(subkey, gainkey))
                            else:
                                raise ValueError('Gains array must be three-dimensional. Use fake dimension if there is no variation '
                                                 'along any particular axis.')
                    else:
                        warnings.warn('Invalid data type specified for {0} instrument gains. Proceeding with defaults (unity '
                                      'gains)'.format(gainkey))
                    gaintable[gainkey]['ordering'] = axes_order
                except KeyError:
                    warnings.warn('No info found on {0} instrument gains. Proceeding with defaults (unity gains)'.format(gainkey))
    except IOError:
        warnings.warn('Invalid file specified for instrument gains. Proceeding with defaults (unity gains)')
        gaintable = None
    if not gaintable:
        gaintable = None
    return gaintable


def _to_label_order(entry):
    """The table's gains with axes (label, frequency, time) (:841-846)."""
    inp_order = entry['ordering']
    if NP.all(inp_order == AXES):
        return NP.copy(entry['gains'])
    return NP.transpose(NP.copy(entry['gains']), axes=R.find_list_in_list(inp_order, AXES))


def extract_gains(gaintable, bl_labels, freq_index=None, time_index=None, axes_order=None):
    """interferometry.py:635-898 on the host: the gains of baselines bl_labels (structured, fields 'A2' and 'A1') at table indices.
    GainInfo.eval_gains does the same on the device."""
    blgains = NP.asarray(1.0).reshape(1, 1, 1)
    if gaintable is not None:
        a1_labels = bl_labels['A1']
        a2_labels = bl_labels['A2']
        for gainkey in GAINKEYS:
            if gainkey in gaintable:
                inp_order = gaintable[gainkey]['ordering']
                gains = _to_label_order(gaintable[gainkey])
                freq_index, time_index = _table_index(freq_index, gains.shape[1], 'freq_index', 'frequency'), \
                    _table_index(time_index, gains.shape[2], 'time_index', 'time')
                if gains.shape[0] == 1:
                    blgains = blgains * gains[:, freq_index, time_index].reshape(1, freq_index.size, time_index.size)
                else:
                    labels = gaintable[gainkey]['label']
                    if gainkey == 'antenna-based':
                        ind1 = R.find_list_in_list(labels, a1_labels)
                        ind2 = R.find_list_in_list(labels, a2_labels)
                        if NP.sum(ind1.mask) > 0 or NP.sum(ind2.mask) > 0:
                            raise IndexError('Some antenna gains could not be found')
                        blgains = blgains * gains[NP.ix_(ind2, freq_index, time_index)].reshape(ind2.size, freq_index.size, time_index.size) \
                            * gains[NP.ix_(ind1, freq_index, time_index)].conj().reshape(ind1.size, freq_index.size, time_index.size)
                    else:
                        ind = _bl_index_appended(labels, bl_labels)
                        selected = NP.concatenate((gains, gains.conj()), axis=0)[NP.ix_(ind.compressed(), freq_index, time_index)]
                        blgains[~ind.mask, ...] = blgains[~ind.mask, ...] * selected
                if axes_order is None:
                    axes_order = inp_order
                else:
                    _check_axes_order(axes_order)
                blgains = NP.transpose(blgains, axes=R.find_list_in_list(inp_order, axes_order))
    return blgains


def _table_index(index, n, name, what):
    if index is None:
        index = NP.arange(n)
    elif isinstance(index, (int, list, NP.ndarray)):
        index = NP.asarray(index).ravel()
    if NP.any(index >= n):
        raise IndexError('Input {0} cannot exceed the {1} dimensions in the gain table'.format(name, what))
    return index


def _bl_index_appended(labels, bl_labels):
    """Rows of bl_labels in [labels, reversed labels] (:866-870): i < nlabels direct, i >= nlabels the conjugate of row i - nlabels."""
    labels_conj = NP.asarray([tuple(reversed(tuple(label))) for label in labels], dtype=labels.dtype)
    return R.find_list_in_list(NP.concatenate((labels, labels_conj), axis=0), bl_labels)


def bl_label_array(labels):
    """Baseline labels as the structured array the reference's gain methods take (fields 'A2', 'A1', text), from (A2, A1) tuples,
    a structured array with those fields, or strings '{prefix}{A2}-{prefix}{A1}' (prisim_amd/driver.py:baseline_info)."""
    if isinstance(labels, NP.ndarray) and labels.dtype.names and 'A2' in labels.dtype.names and 'A1' in labels.dtype.names:
        pairs = [(str(_text(r['A2'])), str(_text(r['A1']))) for r in labels]
    else:
        pairs = []
        for lab in labels:
            if isinstance(lab, (tuple, list, NP.ndarray, NP.void)) and len(lab) == 2:
                pairs.append((str(_text(lab[0])), str(_text(lab[1]))))
            elif isinstance(lab, (str, bytes, NP.str_, NP.bytes_)):
                pairs.append(_split_label(str(_text(lab))))
            else:
                raise TypeError('baseline label {0!r} is neither an (A2, A1) pair nor a string "A2-A1"'.format(lab))
    n = max([len(a) for p in pairs for a in p] + [1])
    return NP.asarray(pairs, dtype=[('A2', 'U{0}'.format(n)), ('A1', 'U{0}'.format(n))]).reshape(-1)


def _split_label(s):
    """'{prefix}{A2}-{prefix}{A1}' -> (A2, A1) with the prefix kept on both (the antenna labels a gain table holds): the '-' whose two
    sides share everything but their trailing digits; a plain 'A2-A1' splits at its only '-'."""
    import re
    cands = [i for i, ch in enumerate(s) if ch == '-']
    for i in cands:
        left, right = s[:i], s[i + 1:]
        ml, mr = re.match(r'^(.*?)(\d+)$', left), re.match(r'^(.*?)(\d+)$', right)
        if ml and mr and ml.group(1) == mr.group(1):
            return left, right
    if len(cands) == 1:
        return s[:cands[0]], s[cands[0] + 1:]
    raise ValueError('cannot split baseline label {0!r} into its two antennas'.format(s))


# ---- packing of fitted splines for the device ----------------------------------------------------------------------------------
_DUMMY_KNOTS = NP.array([0.0, 1.0])        # an axis a 1-D spline does not vary along: degree 0, one coefficient


def pack_splines(interp, dims):
    """Knots, coefficients and degrees of a table's fitted splines (GainInfo.splinefuncs[key]) in the layout of
    prisim_gains_eval_spline: spline 2 r + part (0 real, 1 imaginary) of row r; x = time, y = frequency."""
    nx, ny, kxo, kyo, co, knots, coefs = [], [], [], [], [], [], []
    kx = ky = None
    nk = nc = 0
    for r in range(interp.shape[0]):
        for part in ('real', 'imag'):
            spl = interp[part][r]
            if dims.size == 1:
                t, c, k = spl._eval_args
                t, c = NP.asarray(t, dtype=NP.float64), NP.asarray(c, dtype=NP.float64)[:t.size - k - 1]
                if dims[0] == 'time':
                    tx, ty, sk = t, _DUMMY_KNOTS, (k, 0)
                else:
                    tx, ty, sk = _DUMMY_KNOTS, t, (0, k)
            else:
                tx, ty, c = (NP.asarray(a, dtype=NP.float64) for a in spl.tck)
                sk = tuple(int(d) for d in spl.degrees)
            if kx is None:
                kx, ky = sk
            elif (kx, ky) != sk:
                raise ValueError('the splines of one gain table must share their degrees')
            nx.append(tx.size)
            ny.append(ty.size)
            kxo.append(nk)
            kyo.append(nk + tx.size)
            nk += tx.size + ty.size
            knots += [tx, ty]
            co.append(nc)
            c = c[:(tx.size - kx - 1) * (ty.size - ky - 1)]
            nc += c.size
            coefs.append(c)
    return {'kx': kx, 'ky': ky, 'nx': NP.asarray(nx, dtype=NP.int64), 'ny': NP.asarray(ny, dtype=NP.int64),
            'kx_off': NP.asarray(kxo, dtype=NP.int64), 'ky_off': NP.asarray(kyo, dtype=NP.int64), 'c_off': NP.asarray(co, dtype=NP.int64),
            'knots': NP.concatenate(knots), 'coefs': NP.concatenate(coefs), 'dims': NP.asarray(dims)}


_default_ctx = {}


def _device(ctx=None, device=0):
    """The context a standalone evaluation runs on: the caller's, else one shared context per device (made on first use).
    InterferometerArray.add_noise always uses the array's own context."""
    if ctx is not None:
        return ctx
    device = int(device)
    if device not in _default_ctx:
        _default_ctx[device] = _abi.Context(device)
    return _default_ctx[device]


class _Factor(object):
    """One gain kind's contribution: a device table source and, per baseline, its rows (prisim_gains_apply's factor)."""

    def __init__(self, source, mode, a, c, shape):
        self.source, self.mode, self.a, self.c, self.shape = source, mode, a, c, shape

    def table(self, ctx):
        kind = self.source[0]
        if kind == 'spline':
            return ctx.gains_eval_spline(self.source[1], self.source[2], self.source[3])[0]
        return ctx.gains_gather(self.source[1], self.source[2], self.source[3])[0]


class GainPlan(object):
    """What a gain evaluation resolved to: up to two factors, the shape of the reference's blgains (label, frequency, time) and the
    transposition it ends with.  cube() forms the gains on the device; add_noise applies the factors without forming them."""

    def __init__(self, factors, shape, perm):
        self.factors, self.shape, self.perm = factors, tuple(shape), [int(p) for p in perm]

    def device_factors(self, ctx, nbl):
        out, keep = [], []
        for fac in self.factors:
            tab = fac.table(ctx)
            keep.append(tab)
            a, c = fac.a, fac.c
            if a.size == 1 and nbl != 1:
                a, c = NP.repeat(a, nbl), NP.repeat(c, nbl)
            out.append((tab, fac.mode, a, c))
        return out, keep

    def cube(self, ctx=None, device=0):
        n0, nf, nt = self.shape
        if not self.factors:
            blg = NP.ones(self.shape, dtype=NP.float64)
        else:
            ctx = _device(ctx, device)
            facs, keep = self.device_factors(ctx, n0)
            g, _ = ctx.gains_apply(nt, n0, nf, fa=facs[0], fb=facs[1] if len(facs) > 1 else None, want_gain=True)
            for tab in keep:
                tab.close()
            blg = NP.ascontiguousarray(NP.transpose(g, (1, 2, 0)))
        return NP.transpose(blg, axes=self.perm)


def _bcast(*shapes):
    """numpy's broadcasting of the reference's products, shapes only (its ValueError where the arrays would not broadcast)."""
    return tuple(int(n) for n in NP.broadcast_shapes(*shapes))


class GainInfo(object):
    """interferometry.py:2412-3860.  gaintable: read_gaintable's dictionary or None; splinefuncs[key]: {'interp': (real, imag)
    scipy splines per label, 'dims': the varying axes} or None; packed[key]: their knots and coefficients for the device."""

    def __init__(self, init_file=None, axes_order=None):
        self.gaintable = None
        self.interpfuncs = {key: None for key in GAINKEYS}
        self.splinefuncs = {key: None for key in GAINKEYS}
        self.packed = {key: None for key in GAINKEYS}
        if init_file is not None:
            self.gaintable = self.read_gaintable(init_file, axes_order=axes_order, action='return')
        # interferometry.py:2770 calls self.interpolator() here: built on scipy's removed interp2d, it is not offered
        self.splinator(smoothness=None)

    def read_gaintable(self, gainsfile, axes_order=None, action='return'):
        """:2775-3048."""
        if not isinstance(action, str):
            return TypeError('Input parameter action must be a string')       # returned, not raised, as at :3040
        action = action.lower()
        if action not in ['store', 'return']:
            raise ValueError('Invalid value specified for input parameter action')
        gaintable = read_gaintable(gainsfile, axes_order=axes_order)
        if action == 'store':
            self.gaintable = gaintable
        return gaintable

    def interpolator(self, kind='linear'):
        """:3052-3103 fits scipy.interpolate.interp2d, which scipy >= 1.14 removed."""
        raise NotImplementedError('GainInfo.interpolator is built on scipy.interpolate.interp2d, which scipy removed in 1.14; '
                                  'use splinator / spline_gains')

    def interpolate_gains(self, bl_labels, freqs=None, times=None, axes_order=None):
        """:3169-3378, built on interpolator()."""
        raise NotImplementedError('GainInfo.interpolate_gains is built on scipy.interpolate.interp2d, which scipy removed in 1.14; '
                                  'use spline_gains')

    def splinator(self, smoothness=None):
        """:3107-3166: scipy UnivariateSpline (one varying axis) or RectBivariateSpline over (time, frequency) per label, real and
        imaginary parts apart, smoothing s = the number of samples -- the FIRST value derived is kept for every later label and gain
        kind, as there.  The fits are packed for the device (self.packed)."""
        from scipy import interpolate
        if smoothness is not None:
            if not isinstance(smoothness, (int, float)):
                raise TypeError('Input smoothness must be a scalar')
            if smoothness <= 0.0:
                raise ValueError('Input smoothness must be a positive number')
        if self.gaintable is not None:
            for gainkey in self.gaintable:
                if self.gaintable[gainkey] is not None:
                    self.splinefuncs[gainkey] = None
                    self.packed[gainkey] = None
                    if self.gaintable[gainkey]['gains'] is not None:
                        if isinstance(self.gaintable[gainkey]['gains'], NP.ndarray):
                            entry = self.gaintable[gainkey]
                            if entry['gains'].ndim != 3:
                                raise ValueError('Gains must be a 3D numpy array')
                            if (entry['gains'].shape[entry['ordering'].index('frequency')] > 1) or \
                                    (entry['gains'].shape[entry['ordering'].index('time')] > 1):
                                gains = _to_label_order(entry)
                                dims = NP.asarray([AXES[ax] for ax in (1, 2) if gains.shape[ax] > 1])
                                interpf = []
                                for labelind in range(gains.shape[0]):
                                    if dims.size == 1:
                                        if smoothness is None:
                                            smoothness = entry[dims[0]].size
                                        fr = interpolate.UnivariateSpline(entry[dims[0]], gains[labelind, :, :].real.ravel(), s=smoothness, ext='raise')
                                        fi = interpolate.UnivariateSpline(entry[dims[0]], gains[labelind, :, :].imag.ravel(), s=smoothness, ext='raise')
                                    else:
                                        if smoothness is None:
                                            smoothness = gains.shape[1] * gains.shape[2]
                                        bbox = [entry['time'].min(), entry['time'].max(), entry['frequency'].min(), entry['frequency'].max()]
                                        fr = interpolate.RectBivariateSpline(entry['time'], entry['frequency'], gains[labelind, :, :].real.T,
                                                                             bbox=bbox, s=smoothness)
                                        fi = interpolate.RectBivariateSpline(entry['time'], entry['frequency'], gains[labelind, :, :].imag.T,
                                                                             bbox=bbox, s=smoothness)
                                    interpf += [(copy.copy(fr), copy.copy(fi))]
                                interp = NP.empty(len(interpf), dtype=[('real', object), ('imag', object)])
                                for i, (fr, fi) in enumerate(interpf):
                                    interp[i] = (fr, fi)
                                self.splinefuncs[gainkey] = {'interp': interp, 'dims': dims}
                                self.packed[gainkey] = pack_splines(interp, dims)

    # ---- evaluation plans (the reference's statements with the arrays left on the device) ----
    @staticmethod
    def _range_index(vals, table_vals, what):
        if table_vals is not None:
            ib = NP.logical_and(vals <= NP.amax(table_vals), vals >= NP.amin(table_vals))
            if NP.any(NP.logical_not(ib)):
                raise IndexError('One or more of the {0} outside interpolation range'.format(what))
            return ib
        if vals is not None:
            return NP.ones(vals.size, dtype=bool)
        return None

    def spline_plan(self, bl_labels, freqs=None, times=None, axes_order=None):
        """spline_gains (:3382-3597) up to the arrays: a GainPlan.  Raises what the reference raises where it raises."""
        blshape = (1, 1, 1)
        factors = []
        inp_times = inp_freqs = None
        if self.gaintable is not None:
            a1_labels = bl_labels['A1']
            a2_labels = bl_labels['A2']
            for key in GAINKEYS:
                if self.splinefuncs[key] is not None:
                    labels = self.gaintable[key]['label']
                    if freqs is None:
                        if self.gaintable[key]['frequency'] is not None:
                            freqs = self.gaintable[key]['frequency']
                    elif isinstance(freqs, (int, list, NP.ndarray)):
                        freqs = NP.asarray(freqs).ravel()
                    else:
                        raise TypeError('Input freqs must be a scalar, list or numpy array')
                    if times is None:
                        if self.gaintable[key]['time'] is not None:
                            times = self.gaintable[key]['time']
                    elif isinstance(times, (int, list, NP.ndarray)):
                        times = NP.asarray(times).ravel()
                    else:
                        raise TypeError('Input times must be a scalar, list or numpy array')
                    ib_freq_index = self._range_index(freqs, self.gaintable[key]['frequency'], 'frequencies')
                    ib_time_index = self._range_index(times, self.gaintable[key]['time'], 'times')
                    sf = self.splinefuncs[key]
                    if not isinstance(sf, dict):
                        continue
                    if 'dims' not in sf:
                        raise KeyError('Key "dims" not found in attribute splinefuncs[{0}]'.format(key))
                    if not isinstance(sf['dims'], NP.ndarray):
                        raise TypeError('Key "dims" in attribute splinefuncs[{0}] must contain a numpy array'.format(key))
                    if sf['dims'].size == 1:
                        if sf['dims'][0] == 'time':
                            ntimes = ib_time_index.size
                            nchan = 1 if freqs is None else ib_freq_index.size
                            inp = times[ib_time_index]
                        else:
                            nchan = ib_freq_index.size
                            ntimes = 1 if times is None else ib_time_index.size
                            inp = freqs[ib_freq_index]
                    else:
                        inp_times = times[ib_time_index]
                        inp_freqs = freqs[ib_freq_index]
                        ntimes = ib_time_index.size
                        nchan = ib_freq_index.size
                    if inp_times is None:
                        # :3516 forms NP.meshgrid(inp_times, inp_freqs) for every table; before any 2-D table there is no inp_times
                        raise UnboundLocalError("local variable 'inp_times' referenced before assignment")
                    if sf['dims'].size == 1:
                        if sf['dims'][0] == 'time':
                            src = ('spline', self.packed[key], inp, NP.zeros(1))
                        else:
                            src = ('spline', self.packed[key], NP.zeros(1), inp)
                    else:
                        src = ('spline', self.packed[key], inp_times, inp_freqs)
                    if key == 'antenna-based':
                        ind1 = R.find_list_in_list(labels, a1_labels)
                        ind2 = R.find_list_in_list(labels, a2_labels)
                        if NP.sum(ind1.mask) > 0 or NP.sum(ind2.mask) > 0:
                            raise IndexError('Some antenna gains could not be found')
                        fac = _Factor(src, _abi.PRISIM_GAINS_ANTENNA, NP.asarray(ind1.data), NP.asarray(ind2.data), (ind1.size, nchan, ntimes))
                        evaluated = ind1.size > 0
                    else:
                        row, cj = self._bl_rows(labels, bl_labels)
                        fac = _Factor(src, _abi.PRISIM_GAINS_BASELINE, row, cj, (row.size, nchan, ntimes))
                        evaluated = bool(NP.any(row >= 0))
                    if sf['dims'].size == 1 and evaluated and inp.size != nchan * ntimes:     # (...)(inp).reshape(1, nchan, ntimes)
                        raise ValueError('cannot reshape array of size {0} into shape (1,{1},{2})'.format(inp.size, nchan, ntimes))
                    blshape = _bcast(blshape, fac.shape, (1, nchan, ntimes))
                    factors.append(fac)
        if axes_order is None:
            axes_order = self.gaintable['antenna-based']['ordering']
        else:
            _check_axes_order(axes_order)
        return GainPlan(factors, blshape, R.find_list_in_list(list(AXES), axes_order))

    @staticmethod
    def _bl_rows(labels, bl_labels):
        """Per baseline: the table row of its label, else of its reversed label (conjugated), else -1 (unity) (:3548-3577)."""
        ind = _bl_index_appended(labels, bl_labels)
        n = len(labels)
        data = NP.asarray(ind.data)
        row = NP.where(ind.mask, -1, NP.where(data >= n, data - n, data)).astype(NP.int64)
        cj = (~ind.mask & (data >= n)).astype(NP.int64)
        return row, cj

    def spline_gains(self, bl_labels, freqs=None, times=None, axes_order=None, ctx=None, device=0):
        """:3382-3597: gains of baselines bl_labels (structured, 'A2' / 'A1') from the fitted splines at freqs and times, axes in
        axes_order (default: the table's ordering) -- evaluated on the device: the context ctx, else a shared one on `device`."""
        return self.spline_plan(bl_labels, freqs=freqs, times=times, axes_order=axes_order).cube(ctx, device)

    def _indexed_plan(self, bl_labels, index_maps, axes_order):
        """nearest_gains / eval_gains up to the arrays: per gain kind the table rows at index_maps(gainkey, gains) -> (fidx, tidx)."""
        blshape = (1, 1, 1)
        factors = []
        perm = NP.arange(3)
        if self.gaintable is not None:
            a1_labels = bl_labels['A1']
            a2_labels = bl_labels['A2']
            for gainkey in GAINKEYS:
                if gainkey in self.gaintable:
                    inp_order = self.gaintable[gainkey]['ordering']
                    gains = _to_label_order(self.gaintable[gainkey])
                    rf, rt = index_maps(gainkey, gains)
                    nf, nt = rf.size, rt.size
                    if gains.shape[0] == 1:
                        if nf > 1 and nt > 1:          # gains[:, rf, rt]: the two index arrays broadcast against each other
                            if nf == nt:
                                raise ValueError('cannot reshape array of size {0} into shape (1,{0},{0})'.format(nf))
                            raise IndexError('shape mismatch: indexing arrays could not be broadcast together with shapes ({0},) '
                                             '({1},)'.format(nf, nt))
                        fac = _Factor(('gather', gains, rf, rt), _abi.PRISIM_GAINS_BASELINE, NP.zeros(1, dtype=NP.int64),
                                      NP.zeros(1, dtype=NP.int64), (1, nf, nt))
                        blshape = _bcast(blshape, fac.shape)
                    else:
                        labels = self.gaintable[gainkey]['label']
                        if gainkey == 'antenna-based':
                            ind1 = R.find_list_in_list(labels, a1_labels)
                            ind2 = R.find_list_in_list(labels, a2_labels)
                            if NP.sum(ind1.mask) > 0 or NP.sum(ind2.mask) > 0:
                                raise IndexError('Some antenna gains could not be found')
                            fac = _Factor(('gather', gains, rf, rt), _abi.PRISIM_GAINS_ANTENNA, NP.asarray(ind1.data), NP.asarray(ind2.data),
                                          (ind1.size, nf, nt))
                            blshape = _bcast(blshape, fac.shape)
                        else:
                            row, cj = self._bl_rows(labels, bl_labels)
                            nbl = row.size
                            if blshape[0] != nbl:      # blgains[~ind.mask, ...]
                                raise IndexError('boolean index did not match indexed array along dimension 0; dimension is {0} but '
                                                 'corresponding boolean dimension is {1}'.format(blshape[0], nbl))
                            sel = int(NP.sum(row >= 0))
                            if _bcast((sel,) + blshape[1:], (sel, nf, nt)) != (sel,) + blshape[1:]:
                                raise ValueError('could not broadcast the selected baseline gains into blgains')
                            if len(factors) == 0:      # blgains is still the real 1.0: the assignment would drop the imaginary parts
                                raise NotImplementedError('baseline-based nearest gains of a one-baseline array without antenna gains '
                                                          'are not offered')
                            fac = _Factor(('gather', gains, rf, rt), _abi.PRISIM_GAINS_BASELINE, row, cj, (nbl, nf, nt))
                    if factors and not NP.array_equal(perm, NP.arange(3)):
                        raise NotImplementedError('a second gain kind after a transposing axes_order is not offered')
                    factors.append(fac)
                    if axes_order is None:
                        axes_order = inp_order
                    else:
                        _check_axes_order(axes_order)
                    perm = NP.asarray(perm)[NP.asarray(R.find_list_in_list(inp_order, axes_order))]     # transposes compose
        return GainPlan(factors, blshape, perm)

    def nearest_plan(self, bl_labels, freqs=None, times=None, axes_order=None):
        """nearest_gains (:3599-3723) up to the arrays: the nearest table channel and time of every requested one
        (LKP.find_1NN, prisim_amd/dsp_readings.py), out-of-range points dropped as remove_oob=True does."""
        def maps(gainkey, gains):
            entry = self.gaintable[gainkey]
            refind_freqs = refind_times = None
            fs = copy.copy(freqs) if freqs is not None else copy.copy(entry['frequency'])
            if fs is not None and entry['frequency'] is not None:
                _, refind_freqs, _ = R.find_1NN(entry['frequency'].reshape(-1, 1), NP.asarray(fs).reshape(-1, 1), remove_oob=True)
            if refind_freqs is None:
                refind_freqs = NP.arange(gains.shape[1])
            ts = copy.copy(times) if times is not None else copy.copy(entry['time'])
            if ts is not None and entry['time'] is not None:
                _, refind_times, _ = R.find_1NN(entry['time'].reshape(-1, 1), NP.asarray(ts).reshape(-1, 1), remove_oob=True)
            if refind_times is None:
                refind_times = NP.arange(gains.shape[2])
            return NP.asarray(refind_freqs, dtype=NP.int64), NP.asarray(refind_times, dtype=NP.int64)
        return self._indexed_plan(bl_labels, maps, axes_order)

    def nearest_gains(self, bl_labels, freqs=None, times=None, axes_order=None, ctx=None, device=0):
        """:3599-3723 with the gather on the device (ctx, else a shared context on `device`)."""
        return self.nearest_plan(bl_labels, freqs=freqs, times=times, axes_order=axes_order).cube(ctx, device)

    def eval_gains(self, bl_labels, freq_index=None, time_index=None, axes_order=None, ctx=None, device=0):
        """:3725-3763: the table's gains of bl_labels at every table frequency and time.  The reference passes freq_index=None,
        time_index=None and axes_order=None to extract_gains whatever it was given; so does this."""
        held = {}

        def maps(gainkey, gains):          # extract_gains sets its indices from the FIRST table and keeps them for the second (:811-826)
            fi = held.setdefault('f', NP.arange(gains.shape[1], dtype=NP.int64))
            ti = held.setdefault('t', NP.arange(gains.shape[2], dtype=NP.int64))
            if NP.any(fi >= gains.shape[1]):
                raise IndexError('Input freq_index cannot exceed the frequency dimensions in the gain table')
            if NP.any(ti >= gains.shape[2]):
                raise IndexError('Input time_index cannot exceed the time dimensions in the gain table')
            return fi, ti
        return self._indexed_plan(bl_labels, maps, None).cube(ctx, device)

    def write_gaintable(self, outfile, axes_order=None, compress=True, compress_fmt='gzip', compress_opts=9):
        """:3767-3860 through prisim_amd/hdf5io.py: one group per gain kind with 'gains' (chunked along frequency, gzip), 'ordering'
        and the label / frequency / time arrays that are arrays.  compress_fmt 'lzf' is h5py's own filter, absent from libhdf5."""
        if axes_order is not None:
            _check_axes_order(axes_order)
        if not isinstance(compress, bool):
            raise TypeError('Input parameter compress must be boolean')
        if compress:
            if not isinstance(compress_fmt, str):
                raise TypeError('Input parameter compress_fmt must be a string')
            compress_fmt = compress_fmt.lower()
            if compress_fmt not in ['gzip', 'lzf']:
                raise ValueError('Input parameter compress_fmt invalid')
            if compress_fmt == 'lzf':
                raise NotImplementedError('lzf compression is an h5py filter that the HDF5 library does not carry; use gzip')
            if not isinstance(compress_opts, int):
                raise TypeError('Input parameter compress_opts must be an integer')
            compress_opts = int(NP.clip(compress_opts, 0, 9))
        with hdf5io.File(outfile, 'w') as fileobj:
            for gainkey in self.gaintable:
                if self.gaintable[gainkey] is not None:
                    if axes_order is not None:
                        transpose_order = R.find_list_in_list(self.gaintable[gainkey]['ordering'], axes_order)
                    else:
                        axes_order = self.gaintable[gainkey]['ordering']
                    if NP.all(self.gaintable[gainkey]['ordering'] == axes_order):
                        gains = NP.copy(self.gaintable[gainkey]['gains'])
                    else:
                        gains = NP.transpose(NP.copy(self.gaintable[gainkey]['gains']), axes=transpose_order)
                    fileobj.create_group(gainkey)
                    for subkey in self.gaintable[gainkey]:
                        path = gainkey + '/' + subkey
                        if subkey == 'gains':
                            chunkshape = tuple(gains.shape[ind] if axis == 'frequency' else 1 for ind, axis in enumerate(axes_order))
                            if gains.ndim != 3:
                                fileobj.write(path, gains)
                            elif compress:
                                fileobj.write(path, gains, chunks=chunkshape, gzip=compress_opts)
                            else:
                                fileobj.write(path, gains, chunks=chunkshape)
                        elif subkey == 'ordering':
                            fileobj.write(path, NP.asarray(axes_order))
                        elif isinstance(self.gaintable[gainkey][subkey], NP.ndarray):
                            fileobj.write(path, self.gaintable[gainkey][subkey])
