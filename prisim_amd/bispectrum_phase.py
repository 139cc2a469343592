"""Closure (bispectrum) phases of observed data: prisim/bispectrum_phase.py's loadnpz and the first steps of its ClosurePhase class,
with the day and LST binning of smooth_in_tbins and of subsample_differencing on the GPU (include/prisim_cpbins.h,
prisim_amd/csrc_closure/cpbins.hip) and the differences of the day sub-samples there too (include/prisim_cpdiff.h,
prisim_amd/csrc_closure/cpdiff.hip).

Readings and departures
- astropy is not a dependency.  The reference uses astropy.time.Time only to carry Julian dates, so loadnpz does that arithmetic
  itself; longitude and latitude are accepted and unused.
- OPS.binned_statistic(x, statistic='count', bins=edges) (astroutils is not a dependency) is read as: bin k holds the indices i with
  edges[k] <= x[i] < edges[k+1], in increasing i; its fourth result ri is IDL's reverse-index vector, ri[ri[k]:ri[k+1]] the members
  of bin k (binned_count below).
- Both binning modes (edges with reverse indices, numpy.array_split) reduce to a CSR pair (offsets, members) that the host builds;
  the device reduces every bin (prisim_cphase_bin).  There is no host fall-back.
- Where every member of a bin is flagged the reference assigns masked values into plain arrays and what lands under its mask is not
  specified.  Here the data under the mask are eicp = 1 + 0i and 0 for everything else; the masks are the reference's (wts <= 0).
- The reference's quirks are kept: in the ndaybins branch the mad is the median over all days of the bin, flagged ones included
  (:1834); |cphase - angle(median)| is never wrapped; the LST pass over a day-binned stack takes its mean over exp(i cphase['mean']),
  its median over cos / sin of cphase['median'], its rms of cphase['mean'] and its mad of cphase['median'] (:1930-1933), all with
  the masks of the day pass; only column 0 of the unwrapped LST sets the LST bins.
- A daybinsize that does not exceed the day resolution ends the reference in an UnboundLocalError (:1841); here it is a ValueError.
- ClosurePhase takes, besides an NPZ file name, a ready cpinfo dictionary ({'raw': {...}}), so that simulated phases can be wrapped
  without a file; and a keyword ctx, the device context to use (default: a new one on device 0 at the first binning).
- subsample_differencing bins in days, then in LST, then differences, all on the device: the day-binned and the LST-binned stack
  never reach the host, and cpinfo['errinfo'] receives the reference's keys.  The reference computes the rms and the mad of both
  passes there and stores neither; they are not requested.  Under the masks of 'eicp_diff' the reference leaves unspecified values
  (MA.empty); here the data are 0 + 0i, the reading of the commented-out .filled(0.0) of its delay transform (:2728).  'wts' holds
  sqrt(w_j^2 + w_i^2) everywhere, as the reference's .data does.
- Several LSTs with lstbinsize=None end the reference's subsample_differencing in a NameError (eicp_tmean is never bound, :2231);
  here that case takes the single-LST route: the differences of the day-binned stack.  ndaybins=None with daybinsize=None and a
  daybinsize that does not exceed the day resolution end the reference in an UnboundLocalError (wts_daybins, :2119); here each is a
  ValueError.  These, the reference's own ValueError for a daybinsize that gives fewer than 4 bins, and every other type and value
  error are raised before any device work.
- subtract is host numpy, like expicp: it is elementwise on arrays the host already holds.  Under the masks of 'residual' (the mask of
  prelim or of the model; NaN in the model is masked) the data are 0.
- infmt='hdf5' and save() are not implemented.
"""
import warnings

import numpy as NP
import numpy.ma as MA

from . import _abi


def loadnpz(npzfile, longitude=0.0, latitude=0.0, lst_format='fracday'):
    """Read an NPZ file of closure phases as written from CASA ('closures' (nlst, ndays, ntriads, nchan) radians, 'triads' (ntriads, 3),
    'flags' of the closures' shape, 'last' (nlst, ndays), 'days' (ndays,)) and return {'raw': {'cphase' float64, 'triads', 'flags'
    bool, 'lst' hours, 'lst-day' Julian date, 'days' Julian date}}.

    lst_format: 'fracday' -- 'last' is MJD + 6713 (CASA), its fraction the LST in days; 'hourangle' -- 'last' is the LST in hours.
    longitude, latitude: accepted for the reference's signature and unused (the reference attaches them to astropy Time objects it
    only reads Julian dates from).  The optional 'averaged_closures' / 'std_dev_*' entries, which the reference cannot read either
    (undefined names), raise NotImplementedError when present."""
    npzdata = NP.load(npzfile)
    names = set(npzdata.files)
    for key in ('averaged_closures', 'std_dev_triad', 'std_dev_lst'):
        if key in names:
            raise NotImplementedError('{0} in the NPZ file is not supported (the reference fails on it)'.format(key))
    days = npzdata['days'].astype(NP.float64)
    if lst_format.lower() == 'hourangle':
        lst = npzdata['last']
        lstday = days.reshape(1, -1) + NP.zeros(lst.shape[0]).reshape(-1, 1)
    elif lst_format.lower() == 'fracday':
        lstfrac, lstint = NP.modf(npzdata['last'])
        lstday = lstint.astype(NP.float64) - 6713.0 + 2400000.5           # MJD -> JD
        lst = lstfrac * 24.0
    else:
        raise ValueError('Input lst_format invalid')
    return {'raw': {'cphase': npzdata['closures'].astype(NP.float64), 'triads': NP.copy(npzdata['triads']),
                    'flags': npzdata['flags'].astype(bool), 'lst': NP.copy(lst), 'lst-day': NP.copy(lstday), 'days': NP.copy(days)}}


def binned_count(x, edges):
    """(counts, ri) of the module docstring's reading of OPS.binned_statistic(x, statistic='count', bins=edges)."""
    x = NP.asarray(x, dtype=NP.float64).ravel()
    edges = NP.asarray(edges, dtype=NP.float64).ravel()
    nbins = edges.size - 1
    which = NP.searchsorted(edges, x, side='right') - 1                  # edges[k] <= x < edges[k+1]
    members = [NP.nonzero(which == k)[0] for k in range(nbins)]
    counts = NP.asarray([m.size for m in members], dtype=NP.int64)
    ri = NP.concatenate([nbins + 1 + NP.concatenate(([0], NP.cumsum(counts)))] + members).astype(NP.int64)
    return counts, ri


def _csr(lists):
    offsets = NP.zeros(len(lists) + 1, dtype=NP.int64)
    offsets[1:] = NP.cumsum([len(m) for m in lists])
    members = NP.asarray([i for m in lists for i in m], dtype=NP.int32)
    return offsets, members


def _bin_edges(lo, hi, res, size):
    """edges, centres and widths of bins of `size` from lo to hi + res (:1766-1775, :1869-1878)"""
    eps = 1e-10
    edges = NP.arange(lo, hi + res + eps, size)
    nbins = edges.size
    edges = NP.concatenate((edges, [edges[-1] + size + eps]))
    if nbins > 1:
        widths = edges[1:] - edges[:-1]
        centers = edges[:-1] + 0.5 * widths
    else:
        widths = NP.asarray(size).reshape(-1)
        centers = edges[0] + 0.5 * widths
    return edges, centers, widths


def day_bins(days, daybinsize=None, ndaybins=None):
    """The day bins of smooth_in_tbins: (centres, widths, offsets, members, mad_ignores_flags)."""
    days = NP.asarray(days)
    if daybinsize is not None:
        if not isinstance(daybinsize, (int, float)):
            raise TypeError('Input daybinsize must be a scalar')
        dres = NP.diff(days).min()
        dextent = days.max() - days.min() + dres
        if not daybinsize > dres:
            raise ValueError('Input daybinsize must exceed the day resolution of the data')
        daybinsize = NP.clip(daybinsize, dres, dextent)
        edges, centers, widths = _bin_edges(days.min(), days.max(), dres, daybinsize)
        counts, ri = binned_count(days, edges)
        lists = [ri[ri[k]:ri[k + 1]] for k in range(counts.size)]
        return (centers, widths) + _csr(lists) + (False,)
    if not isinstance(ndaybins, int):
        raise TypeError('Input ndaybins must be an integer')
    if ndaybins <= 0:
        raise ValueError('Input ndaybins must be positive')
    split = NP.array_split(days, ndaybins)
    centers = NP.asarray([NP.mean(d) for d in split])
    widths = NP.asarray([d.max() - d.min() for d in split])
    return (centers, widths) + _csr(NP.array_split(NP.arange(days.size), ndaybins)) + (True,)


def unwrapped_lst(lst):
    """raw['lst'] (hours) unwrapped along axis 0 and, if any value exceeds 24, shifted as a whole by -24 (:1853-1855)"""
    rawlst = NP.degrees(NP.unwrap(NP.radians(NP.asarray(lst) * 15.0), discont=NP.pi, axis=0)) / 15.0
    if NP.any(rawlst > 24.0):
        rawlst -= 24.0
    return rawlst


def lst_bins(rawlst, lstbinsize, nrows):
    """The LST bins of smooth_in_tbins from column 0 of the unwrapped LST: (lstbins, dlstbins, offsets, members).  nrows: entries on
    axis 0 of the stack that is binned."""
    if not isinstance(lstbinsize, (int, float)):
        raise TypeError('Input lstbinsize must be a scalar')
    lstbinsize = lstbinsize / 3.6e3                                      # hours
    col = rawlst[:, 0]
    tres = NP.diff(col).min()
    textent = col.max() - col.min() + tres
    eps = 1e-10
    if lstbinsize > tres:
        lstbinsize = NP.clip(lstbinsize, tres, textent)
        edges, centers, widths = _bin_edges(col.min(), col.max(), tres, lstbinsize)
        counts, ri = binned_count(col, edges)
        lists = [ri[ri[k]:ri[k + 1]] for k in range(counts.size)]
    else:
        warnings.warn('LST bin size found to be smaller than the LST resolution in the data. No LST binning/averaging will be performed.')
        edges = NP.arange(col.min(), col.max() + tres + eps, tres)
        nbins = edges.size - 1
        widths = edges[1:] - edges[:-1] if nbins > 1 else NP.asarray(tres).reshape(-1)
        centers = edges[:-1]
        centers[0] += eps
        centers[-1] -= eps
        lists = [[k] for k in range(nbins)]
    for m in lists:
        if len(m) and NP.max(m) >= nrows:
            raise IndexError('LST bin member {0} is out of bounds for axis 0 with size {1}'.format(int(NP.max(m)), nrows))
    return (centers, widths) + _csr(lists)


def pairs_of_day_bin_pairs(ndaybins):
    """[[i, j, k, m], ...]: every unordered pair of disjoint pairs {i, j}, {k, m} of day bins once, 3 C(ndaybins, 4) of them, in the
    order of the reference's enumeration (:2218-2228): (i, j) ascending, then (k, m) ascending among the pairs disjoint from it, a
    pair of pairs left out where it was listed before with its halves exchanged."""
    seen = set()
    out = []
    for i in range(ndaybins - 1):
        for j in range(i + 1, ndaybins):
            for k in range(ndaybins - 1):
                if k in (i, j):
                    continue
                for m in range(k + 1, ndaybins):
                    if m in (i, j) or ((k, m), (i, j)) in seen:
                        continue
                    seen.add(((i, j), (k, m)))
                    out.append([i, j, k, m])
    return out


class ClosurePhase(object):
    """Closure phases of a data set, (nlst, ndays, ntriads, nchan), their flags, and their binning in days and LST.

    Attributes: cpinfo (the reference's dictionary: 'raw', 'processed' -> 'native' / 'prelim', 'errinfo'), f (Hz), df, extfile.
    binning_stats: the device statistics of the passes of the last smooth_in_tbins call."""

    def __init__(self, infile, freqs, infmt='npz', ctx=None):
        if not isinstance(infile, (str, dict)):
            raise TypeError('Input infile must be a string')
        if not isinstance(freqs, NP.ndarray):
            raise TypeError('Input freqs must be a numpy array')
        freqs = freqs.ravel()
        if not isinstance(infmt, str):
            raise TypeError('Input infmt must be a string')
        if infmt.lower() not in ['npz', 'hdf5']:
            raise ValueError('Input infmt must be "npz" or "hdf5"')
        if isinstance(infile, dict):
            if 'raw' not in infile:
                raise KeyError('a cpinfo dictionary needs the key "raw"')
            self.cpinfo = infile
            self.extfile = None
        elif infmt.lower() == 'npz':
            self.cpinfo = loadnpz(infile)
            self.extfile = infile.split('.npz')[0] + '.hdf5'
        else:
            raise NotImplementedError('infmt="hdf5" is not implemented')
        if freqs.size != self.cpinfo['raw']['cphase'].shape[-1]:
            raise ValueError('Input frequencies do not match with dimensions of the closure phase data')
        self.f = freqs
        self.df = freqs[1] - freqs[0]
        self._ctx = ctx
        self._stack = None
        self.binning_stats = []
        force_expicp = 'processed' not in self.cpinfo or 'native' not in self.cpinfo['processed']
        self.expicp(force_action=force_expicp)
        if 'prelim' not in self.cpinfo['processed']:
            self.cpinfo['processed']['prelim'] = {}
        self.cpinfo['errinfo'] = {}

    def expicp(self, force_action=False):
        """cpinfo['processed']['native']: 'cphase', 'eicp' = exp(i cphase) and 'wts' (1 where unflagged) as masked arrays with the
        flags as masks; formed only where missing unless force_action.  The device copy of the stack is dropped when they are formed
        anew; it is uploaded once, at the next binning."""
        raw = self.cpinfo['raw']
        proc = self.cpinfo.setdefault('processed', {})
        if 'native' not in proc:
            proc['native'] = {}
            force_action = True
        native = proc['native']
        if 'cphase' not in native:
            native['cphase'] = MA.array(raw['cphase'].astype(NP.float64), mask=raw['flags'])
            force_action = True
        if force_action or 'eicp' not in native:
            native['eicp'] = NP.exp(1j * native['cphase'])
            native['wts'] = MA.array(NP.logical_not(raw['flags']).astype(NP.float64), mask=raw['flags'])
            self._drop_stack()

    def _drop_stack(self):
        if getattr(self, '_stack', None) is not None:
            self._stack.close()
        self._stack = None

    def _context(self):
        if self._ctx is None:
            self._ctx = _abi.Context(0)
        return self._ctx

    def _native_stack(self):
        if self._stack is None:
            raw = self.cpinfo['raw']
            self._stack = self._context().cphase_upload(raw['cphase'], raw['flags'])
        return self._stack

    def _store(self, res):
        prelim = self.cpinfo['processed']['prelim']
        mask = res['wts'] <= 0.0
        prelim['wts'] = MA.array(res['wts'], mask=mask)
        prelim['eicp'] = {'mean': MA.array(res['eicp_mean'], mask=mask), 'median': MA.array(res['eicp_median'], mask=mask)}
        prelim['cphase'] = {'mean': MA.array(res['cp_mean'], mask=mask), 'median': MA.array(res['cp_median'], mask=mask),
                            'rms': MA.array(res['rms'], mask=mask), 'mad': MA.array(res['mad'], mask=mask)}

    def smooth_in_tbins(self, daybinsize=None, ndaybins=None, lstbinsize=None):
        """Bin the closure phases in days (daybinsize in days, or ndaybins bins of roughly equal numbers of days) and / or in LST
        (lstbinsize in seconds), on the device.  Fills cpinfo['processed']['prelim'] with 'daybins', 'diff_dbins', 'lstbins', 'dlstbins',
        'wts', 'eicp' ('mean', 'median') and 'cphase' ('mean', 'median', 'rms', 'mad'), masked where wts <= 0, as the reference does.
        With both a day and an LST binning the day-binned stack stays on the device and only the LST-binned products are copied back."""
        if (ndaybins is not None) and (daybinsize is not None):
            raise ValueError('Only one of daybinsize or ndaybins should be set')
        raw = self.cpinfo['raw']
        proc = self.cpinfo['processed']
        if 'prelim' not in proc:
            proc['prelim'] = {}
        prelim = proc['prelim']
        self.binning_stats = []
        rawlst = unwrapped_lst(raw['lst'])
        day = (daybinsize is not None) or (ndaybins is not None)
        lst = rawlst.shape[0] > 1 and lstbinsize is not None
        day_plan = day_bins(raw['days'], daybinsize, ndaybins) if day else None
        kept = None
        if day:
            centers, widths, off, mem, mad_all = day_plan
            if lst:
                # checked before any device work: the LST pass reads this pass's output
                lst_plan = lst_bins(rawlst, lstbinsize, rawlst.shape[0])
                res = self._context().cphase_bin(1, off, mem, stack=self._native_stack(), want=(), mad_ignores_flags=mad_all, keep=True)
                kept = res['stack']
            else:
                res = self._context().cphase_bin(1, off, mem, stack=self._native_stack(), mad_ignores_flags=mad_all)
                self._store(res)
            prelim['daybins'], prelim['diff_dbins'] = centers, widths
            self.binning_stats.append(res['stats'])
        if lst:
            try:
                if kept is not None:
                    centers, widths, off, mem = lst_plan
                    res = self._context().cphase_bin(0, off, mem, stack=kept)
                elif 'wts' in prelim:
                    # products of an earlier call: uploaded from the host, masked where their weights are <= 0
                    centers, widths, off, mem = lst_bins(rawlst, lstbinsize, prelim['wts'].shape[0])
                    res = self._context().cphase_bin(0, off, mem, binned=(MA.getdata(prelim['cphase']['mean']),
                                                                         MA.getdata(prelim['cphase']['median']),
                                                                         MA.getdata(prelim['wts'])))
                else:
                    centers, widths, off, mem = lst_bins(rawlst, lstbinsize, rawlst.shape[0])
                    res = self._context().cphase_bin(0, off, mem, stack=self._native_stack())
            finally:
                if kept is not None:
                    kept.close()
            prelim['lstbins'], prelim['dlstbins'] = centers, widths
            self._store(res)
            self.binning_stats.append(res['stats'])
        else:
            prelim['lstbins'] = NP.mean(rawlst, axis=1)
            prelim['dlstbins'] = NP.asarray(lstbinsize).reshape(-1) if lstbinsize is not None else NP.zeros(1)

    def subtract(self, cphase):
        """Subtract a model of the closure phase (radians; an array that broadcasts against the binned phases, NaN or a mask where
        there is no model) from the binned phasors of smooth_in_tbins, on the host.  Fills cpinfo['processed']['submodel'] = {'cphase',
        'eicp'} at the model's shape with leading axes of length 1, and cpinfo['processed']['residual'] = {'eicp': {'mean', 'median'},
        'cphase': {'mean', 'median'}} with eicp = prelim - model and cphase = angle(prelim / model), masked where prelim or the model
        is; under the mask the data are 0."""
        if not isinstance(cphase, NP.ndarray):
            raise TypeError('Input cphase must be a numpy array')
        if not isinstance(cphase, MA.MaskedArray):
            cphase = MA.array(cphase, mask=NP.isnan(cphase))
        proc = self.cpinfo['processed']
        prelim = proc.get('prelim', {})
        if 'eicp' not in prelim or 'cphase' not in prelim:
            raise ValueError('smooth_in_tbins must fill the binned closure phases before a model can be subtracted')
        shape = prelim['cphase']['median'].shape
        try:
            ok = cphase.ndim <= len(shape) and NP.broadcast_shapes(cphase.shape, shape) is not None
        except ValueError:
            ok = False
        if not ok:
            raise ValueError('Input cphase has shape incompatible with that in instance attribute')
        cphase = cphase.reshape((1,) * (len(shape) - cphase.ndim) + cphase.shape)
        mmask = MA.getmaskarray(cphase)
        cphase = MA.array(NP.where(mmask, 0.0, MA.getdata(cphase)), mask=mmask)
        eicp = MA.array(NP.where(mmask, 0.0, NP.exp(1j * cphase.data)), mask=mmask)
        proc['submodel'] = {'cphase': cphase, 'eicp': eicp}
        proc['residual'] = {'eicp': {}, 'cphase': {}}
        model = NP.exp(1j * cphase.data)                                  # of modulus 1 everywhere, so that the ratio is finite
        for key in ('mean', 'median'):
            pre = prelim['eicp'][key]
            mask = MA.getmaskarray(pre) | mmask
            proc['residual']['eicp'][key] = MA.array(NP.where(mask, 0.0, MA.getdata(pre) - model), mask=mask)
            proc['residual']['cphase'][key] = MA.array(NP.where(mask, 0.0, NP.angle(MA.getdata(pre) / model)), mask=mask)

    def subsample_differencing(self, daybinsize=None, ndaybins=4, lstbinsize=None):
        """Noise estimate from differences of day sub-samples: bin the closure phases in at least 4 day bins (daybinsize in days, or
        ndaybins bins of roughly equal numbers of days), bin those in LST (lstbinsize in seconds; only with several LSTs), and take
        0.5 (e_j - e_i) and 0.5 (e_m - e_k) of the binned unit phasors for every pair of disjoint pairs {i, j}, {k, m} of day bins,
        all on the device.  Fills cpinfo['errinfo'] with 'daybins', 'diff_dbins', 'lstbins', 'dlstbins', 'list_of_pair_of_pairs',
        'wts' {'0', '1'} and 'eicp_diff' {'0', '1'} -> {'mean', 'median'}, (nlstbins, 3 C(ndaybins, 4), ntriads, nchan) masked
        arrays, as the reference does.  Only the bin tables and the list of pairs go to the device and only those arrays come back."""
        if (ndaybins is not None) and (daybinsize is not None):
            raise ValueError('Only one of daybinsize or ndaybins should be set')
        if ndaybins is None and daybinsize is None:
            raise ValueError('One of daybinsize or ndaybins must be set')
        if daybinsize is None:
            if not isinstance(ndaybins, int):
                raise TypeError('Input ndaybins must be an integer')
            if ndaybins < 4:
                raise ValueError('Input ndaybins must be greater than or equal to 4')
        raw = self.cpinfo['raw']
        centers, widths, doff, dmem, mad_all = day_bins(raw['days'], daybinsize, ndaybins)
        ndaybins = doff.size - 1
        if ndaybins < 4:
            raise ValueError('Could not find at least 4 bins along repeating days. Adjust binning interval.')
        rawlst = unwrapped_lst(raw['lst'])
        lst = rawlst.shape[0] > 1 and lstbinsize is not None
        if lst:
            lstcenters, lstwidths, loff, lmem = lst_bins(rawlst, lstbinsize, rawlst.shape[0])
        pairs = pairs_of_day_bin_pairs(ndaybins)
        self.binning_stats = []
        ctx = self._context()
        kept = []
        try:
            res = ctx.cphase_bin(1, doff, dmem, stack=self._native_stack(), want=(), mad_ignores_flags=mad_all, keep=True)
            kept.append(res['stack'])
            self.binning_stats.append(res['stats'])
            if lst:
                res = ctx.cphase_bin(0, loff, lmem, stack=kept[-1], want=(), keep=True)
                kept.append(res['stack'])
                self.binning_stats.append(res['stats'])
            res = ctx.cphase_diff(pairs, stack=kept[-1])
            self.binning_stats.append(res['stats'])
        finally:
            for stack in kept:
                stack.close()
        err = self.cpinfo['errinfo']
        err['daybins'], err['diff_dbins'] = centers, widths
        if lst:
            err['lstbins'], err['dlstbins'] = lstcenters, lstwidths
        else:
            err['lstbins'] = NP.mean(rawlst, axis=1)
            err['dlstbins'] = NP.asarray(lstbinsize).reshape(-1) if lstbinsize is not None else NP.zeros(1)
        err['list_of_pair_of_pairs'] = pairs
        err['wts'] = {str(g): MA.array(res['wts%d' % g], mask=res['mask%d' % g]) for g in range(2)}
        err['eicp_diff'] = {str(g): {stat: MA.array(res['diff%d_%s' % (g, stat)], mask=res['mask%d' % g]) for stat in ('mean', 'median')}
                            for g in range(2)}
