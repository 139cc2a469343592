"""Closure (bispectrum) phases of observed data: prisim/bispectrum_phase.py's loadnpz and the first steps of its ClosurePhase class,
with the day and LST binning of smooth_in_tbins and of subsample_differencing on the GPU (include/prisim_cpbins.h,
prisim_amd/csrc_closure/cpbins.hip) and the differences of the day sub-samples there too (include/prisim_cpdiff.h,
prisim_amd/csrc_closure/cpdiff.hip); and ClosurePhaseDelaySpectrum with its FT, the delay spectra of the binned phasors, of the
residuals, of the sub-model and of the half differences on the GPU (include/prisim_cpft.h, prisim_amd/csrc_closure/cpft.hip), and with
subset, compute_power_spectrum, compute_power_spectrum_uncertainty and beam3Dvol: the cross products of those spectra over pairs of LST
bins, day bins and triads and their collapses on the GPU (include/prisim_cpxps.h, prisim_amd/csrc_closure/cpxps.hip); and the
module-level incoherent_cross_power_spectrum_average and incoherent_kbin_averaging: the weighted averages of those power spectra over
data sets, diagonals and bins of |k_parallel| on the GPU (include/prisim_cpavg.h, prisim_amd/csrc_closure/cpavg.hip).  In front of all
that, simulate_closure_phases and triads_of_bltriplet: the model stack of write_PRISim_bispectrum_phase_to_npz, closure phases of noise
realisations of a simulated array drawn and closed on the GPU (include/prisim_cpreal.h, prisim_amd/csrc_closure/cpreal.hip).

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
- write_PRISim_bispectrum_phase_to_npz (:40-249) reads files of noisy cubes that replicatesim_util.py wrote.  Here
  simulate_closure_phases takes the InterferometerArray itself and has the realisations drawn and closed on the GPU
  (include/prisim_cpreal.h), n_realize of them under the keys seed + r, with the rms divided by sqrt(n_avg): the draws are the
  counter-based ones of generate_noise, not numpy's RandomState, so the stack is the reference's in distribution and not in value.  It
  returns loadnpz's dictionary per key and writes the reference's NPZ files only when a prefix is given; the file-prefix and HDF5 front
  end (:137-176) is not implemented.  The selection of triads by a baseline triplet (:178-209) is triads_of_bltriplet; LKP.find_NN,
  which is not in the tree, is read as: the legs within a Euclidean distance of blltol.

Readings and departures of ClosurePhaseDelaySpectrum.FT (:2573-2784).  Every error is raised before any device work.
- visscaleinfo=None ends the reference in an AttributeError (visscale = 1.0 is a float and :2732 calls .filled); here the scale is 1.
- freq_center=None is read as f[f.size // 2] (the reference's / is Python 2).
- pad < 0 becomes 0 silently (the reference raises a NameError on `verbose`).
- method='nufft' raises NotImplementedError (the reference falls through to an UnboundLocalError).
- datapool: only 'prelim' is accepted, as in the reference.
- Missing inputs raise a ValueError that names the step to run (the reference raises a KeyError at :2713): smooth_in_tbins where
  cpinfo['processed']['prelim'] lacks 'eicp' or 'wts', subsample_differencing where cpinfo['errinfo'] lacks 'wts' or 'eicp_diff'.
- The reference transforms the .data under masks (:2727, :2741, :2749), whose content it leaves unspecified.  Here the data under a
  mask are what this module documents above: 1 + 0i for prelim 'eicp', 0 for the residual, the sub-model and 'eicp_diff'.  They matter
  only with apply_flags=False: a weight of 0 zeroes the term whatever the data hold.
- A row (LST bin, day bin, triad) whose weights average to 0 is NaN in the reference (0 / 0, :2725, :2738); here its spectra and its
  lag kernel are 0.
- Kept quirks: the residual and the sub-model use the prelim weights; 'lag_kernel' uses the weights of the last pool processed
  (prelim's) and has the shape (nspw, 1, 1, 1, nlags) with apply_flags=False; 'residual' always carries 'twts'; 'submodel' is {}
  unless subtract ran; 'freq_center' and 'bw_eff' are returned as given while the rows of 'freq_wts' are in channel order.
- The frequency windows are those of delay_spectrum.subband_freq_wts (the statements of :2688-2709 in the readings of
  dsp_readings.py; fftpow other than 1 has no reading there).
- visscaleinfo: 'vis' as a numpy or masked array (3, nlst_vis, nchan) with 'lst' and nlst_vis == 1 (:2669-2670, :2716-2717, on the
  host: the scale is one number per window and LST bin).  Several reference LSTs need OPS.interpolate_masked_array_1D and an
  InterferometerArray under 'vis' needs its baseline search; both raise NotImplementedError.
- The spectra are copied to the host and do not stay on the device.  save, rescale_power_spectrum and
  average_rescaled_power_spectrum are not implemented.

Readings and departures of subset, compute_power_spectrum (:2888-3601), compute_power_spectrum_uncertainty (:3605-4357) and beam3Dvol
(:4638-4879).  Every error is raised, and every departure decided, before any device work.
- On the host, as O(input) work on arrays it already holds: the normalisation of the arguments, subset, the LST shifts of dlst_range,
  z, kprll and the factor (power_factor), the selection and the coherent average over autoinfo['axes'] (the twts awts weighted mean
  with twts at the channel of largest total weight, NP.median for 'median').  On the device: one prisim_cphase_xpower call per pool,
  statistic and sampling -- the cross product under the preX weights and its collapses, in the order of xinfo['collapse_axes'].  Back
  on the host, on the collapsed result: postX, postXnorm, avgcov, diagoffsets, diagweights, axesmap and the sample counts.
- For days and triads the reference puts the first spectrum at the second index of a pair and the second spectrum at the first
  (:3482, :3509); the entry puts a at the first.  The host swaps the two axes of a full pair and reverses the offsets of a collapsed
  one, so the results have the reference's layout.
- astropy is not a dependency: cosmo is delay_spectrum.cosmo100 by default (h = 1: lengths are Mpc/h) and the results are plain
  complex128 arrays in Jy^2 Mpc/h or K^2 (Mpc/h)^3 for both statistics; the reference converts the units of the last one only.
  OPS.array_trace is read in dsp_readings.array_trace.
- No collapsed axis (xinfo['collapse_axes'] empty) and no incoherent axis (xinfo['axes'] absent, or all of length 1) end the reference
  in an UnboundLocalError on diagweights / diagoffsets (:3594-3595).  Here diagoffsets = {} and diagweights = {} and the full
  cross-power matrix, or factor |dspec|^2 (formed on the host), is returned.
- autoinfo=None, xinfo=None and xinfo={'axes': None} end the reference in TypeErrors (dtpye, :3262, :3291, :3298); here they mean no
  coherent and no incoherent axes.
- A selection together with coherent axes indexes the selected array a second time in the reference (:3465, IndexError); here it is
  indexed once.
- avgcov=True without a collapsed axis fails in the reference; here it is a ValueError.  preXnorm=True calls an undefined logical_or
  (:3518); here it is NotImplementedError.  collapse_axes that are not among xinfo['axes'] (a KeyError in the reference), axes outside
  1..3 and weights of a length that is neither 1 nor the axis' are ValueErrors.
- An LST shift that leaves no LST bin (the default shifts 0 and 1 on a single selected LST bin) fills the reference's row with NaN;
  here it is a ValueError.
- A cpds argument leaves the reference's `sampling` unbound; here the samplings are those present in cpds, and a sampling that FT did
  not produce (resample=False) is skipped.  A pool without spectra ('submodel' and 'residual' unless subtract ran) is skipped.
- The caller's dictionaries (selection, autoinfo, xinfo, beamparms, cpds) are not modified.
- Uncertainty: the days axis 2 is dropped from the coherent, incoherent and collapsed axes, as in the reference; avgcov is the plain
  nanmean over the collapsed axes (:4327; the reference's weighted average behind it multiplies and divides by the same sum); the
  coherent average follows the intent of :4196-4210, which raises a KeyError in the reference ('dspec'); the weights of both halves are
  taken at the channel where those of 'dspec0' total most.  No incoherent axis left is a ValueError (:4340 reads an unbound name).
- beam3Dvol: delay_spectrum.beam3Dvol of delay_spectrum.healpix_power_pattern(freqs, telescope, nside) (the analytic pattern on the
  device), nside 64 and chromatic True by default; chromatic=False takes the pattern at select_freq, by default the mean of the
  frequencies.  A beamfile raises NotImplementedError: its formats need astropy or pyuvdata.

Readings and departures of incoherent_cross_power_spectrum_average (:806-1231) and incoherent_kbin_averaging (:1235-1493).  Every error
is raised before any device work, and the callers' dictionaries are not modified.
- On the host, as O(input) bookkeeping: the broadcast weight arrays from 'diagweights' and 'axesmap', the masks of the selected
  offsets, the bin edges and the CSR of the bins.  On the device: every sum -- one prisim_cphase_xavg call per sampling, pool and
  statistic, one prisim_cphase_kbin call per sampling, pool, statistic and combination.  The results are plain numpy arrays without
  units, never masked arrays.
- excpdps=None: the reference raises a TypeError (:1124 indexes excpdps[0]); here the second result is None.
- 'diagweights' is a dictionary, as compute_power_spectrum returns, or an ndarray, as this function returns, as in the reference; the
  array must have the axes of the spectra, every extent 1 or the spectra's and 1 on the lags.  Axes of a dictionary that are absent
  from that pool's 'diagoffsets' (the avgcov=True case) have weight 1; the reference would broadcast the averaged axis back to 2n - 1.
  'diagoffsets' and 'axesmap' of the result are those of the first data set, as in the reference.
- Each of these is a ValueError where the reference fails otherwise or returns masked values: an axis in diagoffsets that is not a
  collapsed axis of the input (not a key of its 'diagoffsets'); a selection that matches no offset; diagoffsets for an axis whose
  'diagweights' are missing (an empty 'diagweights' together with diagoffsets); data sets of different shapes.
- Axis 2 of a combination is skipped for excpdps, as in the reference; a combination left with no axis returns the stage-1 array and
  its weights (the reference multiplies and divides it by the weights).
- Kept quirk of stage 1 (:1118): a NaN element contributes nothing to the weighted sum while its weight still counts in the
  divisor, so it becomes 0 / weights.  The structural NaN of an LST axis that is crossed and not collapsed therefore come out as 0.
  Stage 2 (MA.sum over the unmasked entries) propagates NaN.
- 'lstXoffsets', which the reference drops, is carried into both results when the first data set has it.
- incoherent_kbin_averaging: a statistic that is a bare array, because diagoffsets=None was used before, is taken as a list of one (the
  reference iterates over its first axis).  kprll.shape[1] / 2 + 1 is read as //, as in Python 2.  With kbintype='log' and
  num_kbins=None, num_kbins is 10.  -eps is inserted in front of the generated edges, so that bin 0 holds k = 0.  Explicit kbins are
  used as given (at least two increasing edges, else a ValueError) and lags outside every bin are dropped.  Kept quirk: num_kbins is
  overwritten with the number of bins of the sampling just binned (:1448), which counts the bin of k = 0, so with 'log' the resampled
  spectra get one bin more than the oversampled ones.
- 'kbininfo' carries 'counts', 'kbin_edges', 'kbinnum' and 'ri' exactly as binned_statistic_count reads OPS.binned_statistic: kbinnum
  is 1 + the bin, 0 below the first edge and nbins + 1 from the last edge on.  Per bin the device walks the members in increasing lag:
  the mean of the members that are not NaN, the mean of |k|^3 P over 2 pi^2 with |k|^3 = (|k| |k|) |k|, and sum |k| |P| / sum |P| with
  each sum dropping its own NaN terms; an empty bin is NaN in all three.  The progress bar and the print are dropped.
"""
import warnings

import copy

import numpy as NP
import numpy.ma as MA

from . import _abi
from . import dsp_readings as DSP


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
    return _cpinfo_of(npzdata, lst_format)


def _cpinfo_of(npzdata, lst_format='fracday'):
    """loadnpz's dictionary from the five arrays of the file ('closures', 'triads', 'flags', 'last', 'days'), given as a mapping."""
    days = NP.asarray(npzdata['days']).astype(NP.float64)
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


def triads_of_bltriplet(simvis, bltriplet, blltol=0.1):
    """The antenna triads of a simulated array whose three baseline vectors are those of bltriplet (3, 3) (legs by ENU metres): the
    selection of write_PRISim_bispectrum_phase_to_npz (:178-209).  The triads are those of simvis.getThreePointCombinations(
    unique=False); leg l of a triad matches row l of bltriplet when some leg of that triad lies within blltol metres of the row
    (LKP.find_NN is not in the tree: it is read as Euclidean distance <= blltol); the rows that match no leg of any triad are
    reversed in sign and all rows searched again, and a triad is selected when every row found one of its legs.  The reference's two
    ValueErrors are kept.  Returns (triads (n, 3) array of antenna labels, their baseline vectors (n, 3, 3)), in the order of
    getThreePointCombinations."""
    if not isinstance(bltriplet, NP.ndarray):
        raise TypeError('Input bltriplet must be a numpy array')
    if isinstance(blltol, bool) or not isinstance(blltol, (int, float)):
        raise TypeError('Input blltol must be a scalar')
    if bltriplet.ndim != 2:
        raise ValueError('Input bltriplet must be a 2D numpy array')
    if bltriplet.shape[0] != 3:
        raise ValueError('Input bltriplet must contain three baseline vectors')
    if bltriplet.shape[1] != 3:
        raise ValueError('Input bltriplet must contain baseline vectors along three corrdinates in the ENU frame')
    triads, bltriplets = simvis.getThreePointCombinations(unique=False)
    triads = NP.asarray(triads).reshape(-1, 3)
    bltriplets = NP.asarray(bltriplets, dtype=NP.float64).reshape(-1, 3, 3)
    flat = bltriplets.reshape(-1, 3)

    def find(rows):                                                        # per row: the flat indices of the legs within blltol
        return [NP.nonzero(NP.sqrt(NP.sum((flat - row) ** 2, axis=1)) <= blltol)[0] for row in rows]
    match = find(bltriplet)
    revind = [i for i in range(3) if match[i].size == 0]
    if revind:                                                             # :191-198
        flip = NP.ones(3)
        flip[revind] = -1.0
        match = find(bltriplet * flip.reshape(-1, 1))
        if any(m.size == 0 for m in match):
            raise ValueError('Some baselines in the triplet are not found in the model triads')
    triadinds = [NP.unravel_index(m, bltriplets.shape[:2])[0] for m in match]
    both = NP.intersect1d(triadinds[0], NP.intersect1d(triadinds[1], triadinds[2]))
    if both.size == 0:
        raise ValueError('Specified triad not found in the PRISim model. Try other permutations of the baseline vectors and/or reverse '
                         'individual baseline vectors in the triad before giving up.')
    return triads[both, :], bltriplets[both, :, :]


def simulate_closure_phases(simvis, n_realize, seed, triads=None, bltriplet=None, blltol=0.1, datakey='noisy', n_avg=1, outfile_prefix=None):
    """Closure phases of n_realize noise realisations of a simulated array in the form loadnpz reads: the body of
    write_PRISim_bispectrum_phase_to_npz (:211-249) for an InterferometerArray that is at hand, with the realisations of
    scriptUtils/replicatesim_util.py:replicate (:82-95) drawn and closed on the GPU (InterferometerArray.closure_phase_realizations)
    in place of its file of noisy cubes.

    triads       list or array (ntriads, 3) of antenna labels; None: triads_of_bltriplet(simvis, bltriplet, blltol)
    datakey      'noiseless', 'noisy' (default), 'noise' or a list of them.  'noiseless' is one getClosurePhase call, repeated along
                 the realisation axis, as the reference repeats it
    seed, n_avg  realisation r is generate_noise(seed=seed + r) with the rms divided by sqrt(n_avg)
    Returns {key: {'raw': {'cphase' (nt, n_realize, ntriads, nchan) float64, 'triads' (ntriads, 3), 'flags' all False, 'lst' hours,
    'lst-day', 'days'}}}: per key what loadnpz gives for the reference's file, so that ClosurePhase(result['noisy'], freqs) works
    directly.  'last' = lst / 15 / 24 broadcast to (nt, n_realize) and 'days' = timestamp[0] + arange(n_realize), as in the reference.
    With outfile_prefix, <prefix>_<key>.npz is written too, with the reference's five arrays ('closures', 'flags', 'triads', 'last',
    'days'); loadnpz reads it back to the same dictionary."""
    if (triads is None) and (bltriplet is None):
        raise ValueError('One of triads or bltriplet must be set')
    if outfile_prefix is not None and not isinstance(outfile_prefix, str):
        raise TypeError('Input outfile_prefix must be a string')
    if isinstance(datakey, str):
        datakey = [datakey]
    elif not isinstance(datakey, list):
        raise TypeError('Input datakey must be a list')
    datakey = [k.lower() for k in datakey]
    for dkey in datakey:
        if dkey not in ['noiseless', 'noisy', 'noise']:
            raise ValueError('Invalid input found in datakey')
    if isinstance(n_realize, bool) or not isinstance(n_realize, (int, NP.integer)):
        raise TypeError('n_realize must be an integer')
    if n_realize < 1:
        raise ValueError('n_realize must be at least 1')
    if triads is None:
        triads, _ = triads_of_bltriplet(simvis, bltriplet, blltol)
    elif not isinstance(triads, (list, NP.ndarray)):
        raise TypeError('Input triads must be a list or numpy array')
    triads = NP.asarray(triads).astype(str).reshape(-1, 3)
    triplets = [tuple(t) for t in triads.tolist()]
    last = (NP.asarray(simvis.lst, dtype=NP.float64) / 15.0 / 24.0).reshape(-1, 1) + NP.zeros((1, n_realize))     # :156-157, :248
    days = NP.asarray(simvis.timestamp[0]).ravel() + NP.arange(n_realize)                                        # :158, :249
    cpdata = {}
    drawn = [k for k in datakey if k != 'noiseless']
    if drawn:
        res = simvis.closure_phase_realizations(n_realize, seed, antenna_triplets=triplets, datakey=drawn, n_avg=n_avg)
        for k in drawn:
            cpdata[k] = res['closure_phase_vis' if k == 'noisy' else 'closure_phase_noise']
    if 'noiseless' in datakey:
        sky = simvis.getClosurePhase(antenna_triplets=triplets)['closure_phase_skyvis']                          # (ntriads, nchan, nt)
        cpdata['noiseless'] = NP.repeat(NP.transpose(sky, (2, 0, 1))[:, NP.newaxis, :, :], n_realize, axis=1)
    out = {}
    for k in datakey:
        arrays = {'closures': cpdata[k], 'flags': NP.zeros(cpdata[k].shape, dtype=bool), 'triads': triads, 'last': last, 'days': days}
        if outfile_prefix is not None:
            NP.savez_compressed(outfile_prefix + '_{0}.npz'.format(k), **arrays)
        out[k] = _cpinfo_of(arrays)
    return out


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


def binned_statistic_count(x, edges):
    """(counts, edges, binnum, ri) as OPS.binned_statistic(x, statistic='count', bins=edges) returns them, in binned_count's reading:
    binnum[i] is 1 + the bin of x[i], 0 below the first edge and nbins + 1 from the last edge on."""
    x = NP.asarray(x, dtype=NP.float64).ravel()
    edges = NP.asarray(edges, dtype=NP.float64).ravel()
    counts, ri = binned_count(x, edges)
    return counts, edges, NP.searchsorted(edges, x, side='right').astype(NP.int64), ri


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


_TOP_KEYS = ('triads', 'triads_ind', 'lst', 'lst_ind', 'dlst', 'days', 'day_ind', 'dday')
_SAMPLING_KEYS = ('z', 'kprll', 'lags', 'freq_center', 'bw_eff', 'shape', 'freq_wts', 'lag_corr_length')


def _diag_weights(pool, stat, where):
    """The diagweights of one data set of a pool at a shape that broadcasts against its spectra: from the dictionary that
    compute_power_spectrum returns (axes absent from the pool's diagoffsets have weight 1) or from the array that
    incoherent_cross_power_spectrum_average returns"""
    arr = NP.asarray(pool[stat])
    dw = pool['diagweights']
    if isinstance(dw, dict):
        w = NP.ones((1,) * arr.ndim, dtype=NP.float64)
        for ax in dw:
            if ax not in pool.get('diagoffsets', {}):
                continue
            v = NP.asarray(dw[ax], dtype=NP.float64).reshape(-1)
            pos = int(NP.asarray(pool['axesmap'][ax]).reshape(-1)[0])
            if not 0 < pos < arr.ndim - 1 or v.size != arr.shape[pos]:
                raise ValueError('{0}: the diagweights of axis {1} do not match the spectra'.format(where, ax))
            shp = [1] * arr.ndim
            shp[pos] = v.size
            w = w * v.reshape(shp)
        return w
    if isinstance(dw, NP.ndarray):
        w = NP.asarray(dw, dtype=NP.float64)
        if w.ndim != arr.ndim or w.shape[-1] != 1 or any(b not in (1, n) for b, n in zip(w.shape, arr.shape)):
            raise ValueError('{0}: diagweights of shape {1} do not broadcast against spectra of shape {2}'.format(where, w.shape, arr.shape))
        return w
    raise TypeError('Diagonal weights in input must be a dictionary or a numpy array')


def incoherent_cross_power_spectrum_average(xcpdps, excpdps=None, diagoffsets=None, ctx=None):
    """Incoherent average of cross-power spectra (:806-1231).  xcpdps: a result of compute_power_spectrum or a list of them, one per
    data set; excpdps: None, or as many results of compute_power_spectrum_uncertainty.  Stage 1 averages the data sets of every
    sampling, pool and statistic under their diagweights: sum(a w) / sum(w), a NaN product counted as 0.  Stage 2, with diagoffsets (a
    dictionary {axis: offsets} with the axes 1 LST, 2 days, 3 triads, or a list of them): per combination the diagweights-weighted
    average over the selected offsets of its axes; the statistics are then lists with one array per combination, the reduced axes
    kept at length 1, and 'diagweights' is the list of the summed weights.  Axis 2 does not apply to excpdps.  Every sum runs on the
    device (prisim_cphase_xavg), one call per sampling, pool and statistic.  Returns (out_xcpdps, out_excpdps), plain arrays;
    out_excpdps is None without excpdps.  ctx: the device context (default: a new one on device 0).  See the module docstring for the
    departures."""
    if isinstance(xcpdps, dict):
        xcpdps = [xcpdps]
    if not isinstance(xcpdps, list):
        raise TypeError('Invalid data type provided for input xcpdps')
    if len(xcpdps) < 1:
        raise ValueError('Input xcpdps is empty')
    if excpdps is not None:
        if isinstance(excpdps, dict):
            excpdps = [excpdps]
        if not isinstance(excpdps, list):
            raise TypeError('Invalid data type provided for input excpdps')
        if len(xcpdps) != len(excpdps):
            raise ValueError('Inputs xcpdps and excpdps found to have unequal number of values')
    combos = None
    if diagoffsets is not None:
        if isinstance(diagoffsets, dict):
            diagoffsets = [diagoffsets]
        if not isinstance(diagoffsets, list):
            raise TypeError('Input diagoffsets must be a list of dictionaries')
        combos = []
        for item in diagoffsets:
            if not isinstance(item, dict):
                raise TypeError('Input diagoffsets must be a list of dictionaries')
            for ax in item:
                if not isinstance(item[ax], (list, NP.ndarray)):
                    raise TypeError('Values in input dictionary diagoffsets must be a list or numpy array')
            combos.append({ax: NP.asarray(item[ax]).reshape(-1) for ax in item})

    # the plan: per output, sampling, pool and statistic the arrays, their weights and the masks of every combination
    plan = []
    outs = []
    for sets, pools, skip in ((xcpdps, ('whole', 'submodel', 'residual'), ()), (excpdps, ('errinfo',), (2,))):
        if sets is None:
            outs.append(None)
            continue
        first = sets[0]
        out = {key: first[key] for key in _TOP_KEYS}
        if 'lstXoffsets' in first:
            out['lstXoffsets'] = first['lstXoffsets']
        for smplng in ('oversampled', 'resampled'):
            if smplng not in first:
                continue
            out[smplng] = {key: first[smplng][key] for key in _SAMPLING_KEYS}
            for dpool in pools:
                if dpool not in first[smplng]:
                    continue
                pool0 = first[smplng][dpool]
                out[smplng][dpool] = {'diagoffsets': pool0['diagoffsets'], 'axesmap': pool0['axesmap']}
                for stat in ('mean', 'median'):
                    if stat not in pool0:
                        continue
                    where = '{0} {1} {2}'.format(smplng, dpool, stat)
                    arrays = [NP.asarray(d[smplng][dpool][stat]) for d in sets]
                    if any(a.shape != arrays[0].shape for a in arrays) or not 5 <= arrays[0].ndim <= 8:
                        raise ValueError('{0}: the data sets must have one shape of 5 to 8 axes'.format(where))
                    weights = [_diag_weights(d[smplng][dpool], stat, where) for d in sets]
                    masks = None
                    if combos is not None:
                        masks = []
                        for combo in combos:
                            mask = {}
                            for ax in combo:
                                if ax in skip:
                                    continue
                                if ax not in pool0['diagoffsets']:
                                    raise ValueError('{0}: axis {1} in diagoffsets is not a collapsed axis of the input'.format(where, ax))
                                for d in sets:
                                    dw = d[smplng][dpool]['diagweights']
                                    if isinstance(dw, dict) and ax not in dw:
                                        raise ValueError('{0}: the diagoffsets of axis {1} need its diagweights, and there are none'.format(where, ax))
                                sel = NP.isin(NP.asarray(pool0['diagoffsets'][ax]).reshape(-1), combo[ax])
                                if not NP.any(sel):
                                    raise ValueError('{0}: no offset of axis {1} is among {2}'.format(where, ax, combo[ax].tolist()))
                                pos = int(NP.asarray(pool0['axesmap'][ax]).reshape(-1)[0])
                                if not 0 < pos < arrays[0].ndim - 1 or sel.size != arrays[0].shape[pos]:
                                    raise ValueError('{0}: the diagoffsets of axis {1} do not match the spectra'.format(where, ax))
                                mask[pos] = sel
                            masks.append(mask)
                    plan.append((out[smplng][dpool], stat, arrays, weights, masks))
        outs.append(out)

    if plan and ctx is None:
        ctx = _abi.Context(0)
    for pool, stat, arrays, weights, masks in plan:
        if masks is None:
            res = ctx.cphase_xavg(arrays, weights)
            pool[stat], pool['diagweights'] = res['avg'], res['wsum']
            continue
        res = ctx.cphase_xavg(arrays, weights, combos=[m for m in masks if m], want_avg=not all(masks))
        reduced, wreduced = iter(res['out']), iter(res['wout'])
        # a combination left with no axis: the average itself
        pool[stat] = [next(reduced) if m else res['avg'] for m in masks]
        pool['diagweights'] = [next(wreduced) if m else res['wsum'] for m in masks]
    return tuple(outs)


def incoherent_kbin_averaging(xcpdps, kbins=None, num_kbins=None, kbintype='log', ctx=None):
    """Power spectra in bins of |k_parallel| (:1235-1493).  xcpdps: a result of incoherent_cross_power_spectrum_average.  kbins: the
    bin edges, or None: edges from eps to max |kprll| + eps, linear (kprll.shape[1] // 2 + 1 of them, folding -k on +k) or logarithmic
    (num_kbins + 1 of them, num_kbins 10 by default), behind an edge at -eps so that bin 0 holds k = 0.  Returns the reference's
    dictionary: the top-level keys, and per sampling its keys, 'kbininfo' ('counts', 'kbin_edges', 'kbinnum', 'ri', one entry per
    window, and per pool and statistic the list of the |P|-weighted bin centres) and per pool 'diagoffsets', 'diagweights', 'axesmap'
    and per statistic {'PS': [...], 'Del2': [...]}, one array per combination with nkbins in the place of the lags; an empty bin is
    NaN.  Every sum runs on the device (prisim_cphase_kbin), one call per sampling, pool, statistic and combination.  ctx: the device
    context (default: a new one on device 0).  See the module docstring for the departures."""
    if not isinstance(xcpdps, dict):
        raise TypeError('Input xcpdps must be a dictionary')
    if kbins is not None:
        if not isinstance(kbins, (list, NP.ndarray)):
            raise TypeError('Input kbins must be a list or numpy array')
        edges_given = NP.asarray(kbins, dtype=NP.float64).reshape(-1)
        if edges_given.size < 2 or NP.any(NP.diff(edges_given) <= 0):
            raise ValueError('Input kbins must hold at least two increasing edges')
    else:
        if not isinstance(kbintype, str):
            raise TypeError('Input kbintype must be a string')
        if kbintype.lower() not in ['linear', 'log']:
            raise ValueError('Input kbintype must be set to "linear" or "log"')
        if kbintype.lower() == 'log':
            if num_kbins is None:
                num_kbins = 10
            if isinstance(num_kbins, bool) or not isinstance(num_kbins, (int, NP.integer)):
                raise TypeError('Input num_kbins must be an integer')
            if num_kbins < 1:
                raise ValueError('Input num_kbins must be positive')
    psinfo = {key: xcpdps[key] for key in _TOP_KEYS}
    if 'lstXoffsets' in xcpdps:
        psinfo['lstXoffsets'] = xcpdps['lstXoffsets']
    eps = 1e-10
    plan = []
    for smplng in ('oversampled', 'resampled'):
        if smplng not in xcpdps:
            continue
        psinfo[smplng] = {key: xcpdps[smplng][key] for key in _SAMPLING_KEYS if key not in ('kprll', 'lags')}
        kprll = NP.asarray(xcpdps[smplng]['kprll'], dtype=NP.float64)
        if kprll.ndim != 2:
            raise ValueError('{0}: kprll must be (nspw, nlags)'.format(smplng))
        if kbins is None:
            if kbintype.lower() == 'linear':
                bins_kprll = NP.linspace(eps, NP.abs(kprll).max() + eps, num=kprll.shape[1] // 2 + 1, endpoint=True)
            else:
                bins_kprll = NP.geomspace(eps, NP.abs(kprll).max() + eps, num=num_kbins + 1, endpoint=True)
            bins_kprll = NP.insert(bins_kprll, 0, -eps)
        else:
            bins_kprll = edges_given
        num_kbins = bins_kprll.size - 1                # carried to the next sampling, as in the reference
        info = {'counts': [], 'kbin_edges': [], 'kbinnum': [], 'ri': []}
        psinfo[smplng]['kbininfo'] = info
        lists = []
        for spw in range(kprll.shape[0]):
            counts, kbin_edges, kbinnum, ri = binned_statistic_count(NP.abs(kprll[spw, :]), bins_kprll)
            info['counts'].append(counts)
            info['kbin_edges'].append(NP.copy(kbin_edges))
            info['kbinnum'].append(kbinnum)
            info['ri'].append(ri)
            lists.append([ri[ri[k]:ri[k + 1]] for k in range(num_kbins)])
        offsets = NP.asarray([_csr(l)[0] for l in lists], dtype=NP.int64)
        members = [_csr(l)[1] for l in lists]
        for dpool in ('whole', 'submodel', 'residual', 'errinfo'):
            if dpool not in xcpdps[smplng]:
                continue
            pool = xcpdps[smplng][dpool]
            psinfo[smplng][dpool] = {key: pool[key] for key in ('diagoffsets', 'diagweights', 'axesmap')}
            info[dpool] = {}
            for stat in ('mean', 'median'):
                if stat not in pool:
                    continue
                arrays = pool[stat] if isinstance(pool[stat], (list, tuple)) else [pool[stat]]
                arrays = [NP.asarray(a) for a in arrays]
                for a in arrays:
                    if a.ndim < 2 or a.shape[0] != kprll.shape[0] or a.shape[-1] != kprll.shape[1]:
                        raise ValueError('{0} {1} {2}: spectra of shape {3} do not have the windows and lags of kprll {4}'.format(
                            smplng, dpool, stat, a.shape, kprll.shape))
                psinfo[smplng][dpool][stat] = {'PS': [], 'Del2': []}
                info[dpool][stat] = []
                plan.append((psinfo[smplng][dpool][stat], info[dpool][stat], arrays, kprll, offsets, members))
    if plan and ctx is None:
        ctx = _abi.Context(0)
    for ps, centres, arrays, kprll, offsets, members in plan:
        for a in arrays:
            res = ctx.cphase_kbin(a, kprll, offsets, members)
            ps['PS'].append(res['ps'])
            ps['Del2'].append(res['del2'])
            centres.append(res['kc'])
    return psinfo


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


def _vis_scale(visscaleinfo, freq_wts, nlst):
    """visscale (nspw, nlst) of :2631-2672 and :2716-2717 for one reference LST, or None"""
    if visscaleinfo is None:
        return None
    if not isinstance(visscaleinfo, dict):
        raise TypeError('Input visscaleinfo must be a dictionary')
    if 'vis' not in visscaleinfo:
        raise KeyError('Input visscaleinfo does not contain key "vis"')
    vis = visscaleinfo['vis']
    if not isinstance(vis, NP.ndarray):
        if hasattr(vis, 'skyvis_freq'):
            raise NotImplementedError('an InterferometerArray under visscaleinfo["vis"] is not supported: pass the (3, nlst_vis, nchan) array')
        raise TypeError('Input visibilities must be a numpy or a masked array')
    if 'lst' not in visscaleinfo:
        raise KeyError('Input visscaleinfo does not contain key "lst"')
    lst_vis = NP.asarray(visscaleinfo['lst']) * 15.0
    if vis.ndim != 3 or vis.shape[0] != 3 or vis.shape[2] != freq_wts.shape[1]:
        raise ValueError('Input visibilities must have the shape (3, nlst_vis, nchan)')
    if lst_vis.size != 1 or vis.shape[1] != 1:
        raise NotImplementedError('several reference LSTs in visscaleinfo need OPS.interpolate_masked_array_1D, which is not available')
    if not isinstance(vis, MA.MaskedArray):
        vis = MA.array(vis, mask=NP.isnan(vis))
    vis_ref = MA.copy(vis) * NP.ones(nlst).reshape(1, -1, 1)                                    # (3, nlst, nchan)
    fw = freq_wts[:, NP.newaxis, NP.newaxis, NP.newaxis, :]
    visscale = NP.nansum(NP.transpose(vis_ref[NP.newaxis, NP.newaxis, :, :, :], axes=(0, 3, 1, 2, 4)) * fw, axis=-1, keepdims=True) \
        / NP.nansum(fw, axis=-1, keepdims=True)                                                # nspw x nlst x 1 x 3 x 1
    visscale = NP.sqrt(1.0 / NP.nansum(1 / NP.abs(visscale) ** 2, axis=-2, keepdims=True))
    return NP.ascontiguousarray(MA.filled(visscale, NP.nan).reshape(freq_wts.shape[0], nlst), dtype=NP.float64)


class ClosurePhaseDelaySpectrum(object):
    """Delay spectra of the binned closure phasors of a ClosurePhase.

    Attributes: cPhase, f (Hz), df, cPhaseDS (the oversampled result of the last FT), cPhaseDS_resampled (its resampled result, set
    with resample=True).  ft_stats: the device statistics of the calls of the last FT, by weight set."""

    def __init__(self, cPhase):
        if not isinstance(cPhase, ClosurePhase):
            raise TypeError('Input cPhase must be an instance of class ClosurePhase')
        self.cPhase = cPhase
        self.f = self.cPhase.f
        self.df = self.cPhase.df
        self.cPhaseDS = None
        self.cPhaseDS_resampled = None
        self.ft_stats = {}
        self.xps_stats = {}

    def FT(self, bw_eff, freq_center=None, shape=None, fftpow=None, pad=None, datapool='prelim', visscaleinfo=None, method='fft',
           resample=True, apply_flags=True):
        """Delay transform of the binned phasors (cpinfo['processed']['prelim']), of the residuals and the sub-model where subtract
        ran, and of the half differences of subsample_differencing (cpinfo['errinfo']), in the frequency windows (bw_eff, freq_center,
        shape, fftpow), zero-padded by pad * nchan channels, under the flag weights divided by their mean over the channels
        (apply_flags) and scaled to visibilities (visscaleinfo), on the device.  Returns the reference's dictionary: 'freq_center',
        'shape', 'freq_wts', 'bw_eff', 'fftpow', 'npad', 'lags', 'lag_corr_length', 'lag_kernel', 'whole' / 'residual' -> 'dspec' ->
        'twts', 'mean', 'median', 'submodel' -> 'dspec', 'errinfo' -> 'dspec0' / 'dspec1' -> 'twts', 'mean', 'median'; spectra are
        (nspw, nlst, ndays, ntriads, nlags).  With resample the spectra are FFT-resampled to round(nlags / min((nchan + npad) df /
        bw_eff)) lags and 'lags' and 'lag_kernel' interpolated; the oversampled result stays in cPhaseDS.  See the module docstring for
        the departures."""
        from .delay_spectrum import subband_freq_wts
        if not isinstance(bw_eff, (int, float, list, NP.ndarray)):
            raise TypeError('Value of effective bandwidth must be a scalar, list or numpy array')
        bw_eff = NP.asarray(bw_eff).reshape(-1)
        if NP.any(bw_eff <= 0.0):
            raise ValueError('All values in effective bandwidth must be strictly positive')
        if freq_center is None:
            freq_center = NP.asarray(self.f[self.f.size // 2]).reshape(-1)
        elif isinstance(freq_center, (int, float, list, NP.ndarray)):
            freq_center = NP.asarray(freq_center).reshape(-1)
            if NP.any((freq_center <= self.f.min()) | (freq_center >= self.f.max())):
                raise ValueError('Value(s) of frequency center(s) must lie strictly inside the observing band')
        else:
            raise TypeError('Values(s) of frequency center must be scalar, list or numpy array')
        if (bw_eff.size == 1) and (freq_center.size > 1):
            bw_eff = NP.repeat(bw_eff, freq_center.size)
        elif (bw_eff.size > 1) and (freq_center.size == 1):
            freq_center = NP.repeat(freq_center, bw_eff.size)
        elif bw_eff.size != freq_center.size:
            raise ValueError('Effective bandwidth(s) and frequency center(s) must have same number of elements')
        if shape is not None:
            if not isinstance(shape, str):
                raise TypeError('Window shape must be a string')
            if shape not in ['rect', 'bhw', 'bnw', 'RECT', 'BHW', 'BNW']:
                raise ValueError('Invalid value for window shape specified.')
        else:
            shape = 'rect'
        if fftpow is None:
            fftpow = 1.0
        else:
            if not isinstance(fftpow, (int, float)):
                raise TypeError('Power to raise window FFT by must be a scalar value.')
            if fftpow < 0.0:
                raise ValueError('Power for raising FFT of window by must be positive.')
        if pad is None:
            pad = 1.0
        else:
            if not isinstance(pad, (int, float)):
                raise TypeError('pad fraction must be a scalar value.')
            if pad < 0.0:
                pad = 0.0
        if not isinstance(datapool, str):
            raise TypeError('Input datapool must be a string')
        if datapool.lower() not in ['prelim']:
            raise ValueError('Specified datapool not supported')
        if not isinstance(method, str):
            raise TypeError('Input method must be a string')
        if method.lower() not in ['fft', 'nufft']:
            raise ValueError('Specified FFT method not supported')
        if method.lower() == 'nufft':
            raise NotImplementedError('method="nufft" is not implemented')
        if not isinstance(apply_flags, bool):
            raise TypeError('Input apply_flags must be boolean')
        cpinfo = self.cPhase.cpinfo
        proc = cpinfo.get('processed', {})
        prelim = proc.get('prelim', {})
        if 'eicp' not in prelim or 'wts' not in prelim:
            raise ValueError('smooth_in_tbins must fill the binned closure phases before they can be transformed')
        err = cpinfo.get('errinfo', {})
        if 'wts' not in err or 'eicp_diff' not in err:
            raise ValueError('subsample_differencing must fill the sub-sample differences before they can be transformed')
        nchan = self.f.size
        freq_wts = subband_freq_wts(self.f, self.df, bw_eff, freq_center, shape, fftpow)        # nspw x nchan
        nlst = NP.asarray(prelim['lstbins']).size
        vscale = _vis_scale(visscaleinfo, freq_wts, nlst)
        npad = int(nchan * pad)
        m = nchan + npad
        if m > _abi.PRISIM_CPFT_MAX_LEN:
            raise ValueError('nchan + npad = {0} exceeds the {1} lags of the device transform'.format(m, _abi.PRISIM_CPFT_MAX_LEN))
        lags = DSP.spectral_axis(m, delx=self.df, use_real=False, shift=True)
        downsample_factor = NP.min(m * self.df / bw_eff)
        nres = DSP.fft_downsample_length(m, downsample_factor) if resample else None
        if resample and not 1 <= nres <= _abi.PRISIM_CPFT_MAX_LEN:
            raise ValueError('the resampled spectra would have {0} lags'.format(nres))

        def data(x, fill):
            """the data of a masked array with `fill` under its mask, at its stored shape with leading axes of length 1 added"""
            x = MA.array(x)
            d = NP.where(MA.getmaskarray(x), fill, MA.getdata(x)).astype(NP.complex128)
            return d.reshape((1,) * (4 - d.ndim) + d.shape)

        # one call per weight set: (weights, names, input stacks)
        names = [('whole', key) for key in prelim['eicp']]
        stacks = [data(prelim['eicp'][key], 1.0) for key in prelim['eicp']]
        if 'submodel' in proc:
            names.append(('submodel', None))
            stacks.append(data(proc['submodel']['eicp'], 0.0))
        if 'residual' in proc:
            names += [('residual', key) for key in proc['residual']['eicp']]
            stacks += [data(proc['residual']['eicp'][key], 0.0) for key in proc['residual']['eicp']]
        calls = [('prelim', MA.getdata(prelim['wts']), names, stacks)]
        for g in ('0', '1'):
            calls.append(('errinfo' + g, MA.getdata(err['wts'][g]), [('errinfo', 'dspec' + g, stat) for stat in err['eicp_diff'][g]],
                          [data(err['eicp_diff'][g][stat], 0.0) for stat in err['eicp_diff'][g]]))
        for label, wts, _, stk in calls:
            for x in stk:
                if x.ndim != 4 or x.shape[-1] != nchan or any(b not in (n, 1) for b, n in zip(x.shape[:3], wts.shape[:3])):
                    raise ValueError('a stack of {0} does not broadcast against its weights'.format(label))
            if vscale is not None and wts.shape[0] != nlst:
                raise ValueError('the weights of {0} do not have the LST bins of prelim'.format(label))

        result = {'freq_center': freq_center, 'shape': shape, 'freq_wts': freq_wts, 'bw_eff': bw_eff, 'fftpow': fftpow, 'npad': npad,
                  'lags': lags, 'lag_corr_length': nchan / NP.sum(freq_wts, axis=-1),
                  'whole': {'dspec': {'twts': prelim['wts']}}, 'residual': {'dspec': {'twts': prelim['wts']}},
                  'errinfo': {'dspec0': {'twts': err['wts']['0']}, 'dspec1': {'twts': err['wts']['1']}}, 'submodel': {}}
        resampled = None
        if resample:
            resampled = copy.deepcopy(result)

        def put(res, name, value):
            if name[0] == 'errinfo':
                res['errinfo'][name[1]][name[2]] = value
            elif name[0] == 'submodel':
                res['submodel']['dspec'] = value
            else:
                res[name[0]]['dspec'][name[1]] = value

        ctx = self.cPhase._context()
        self.ft_stats = {}
        want = ('over', 'res') if resample else ('over',)
        for label, wts, names, stk in calls:
            lagk = label == 'prelim'
            out = ctx.cphase_ft(stk, freq_wts, m, self.df, weights=wts if apply_flags else None, vscale=vscale, nres=nres,
                                want=want + (('lag_kernel',) if lagk else ()), shape=wts.shape[:3])
            self.ft_stats[label] = out['stats']
            for i, name in enumerate(names):
                put(result, name, out['over'][i])
                if resample:
                    put(resampled, name, out['res'][i])
            if lagk:
                result['lag_kernel'] = out['lag_kernel']
        self.cPhaseDS = result
        if not resample:
            return result
        resampled['lags'] = DSP.downsampler(result['lags'], downsample_factor, axis=-1, method='interp', kind='linear')
        resampled['lag_kernel'] = DSP.downsampler(result['lag_kernel'], downsample_factor, axis=-1, method='interp', kind='linear')
        self.cPhaseDS_resampled = resampled
        return resampled

    def subset(self, selection=None):
        """(triad_ind, lst_ind, day_ind, day_ind_eicpdiff): the indices that `selection` ({'triads': list of 3-tuples, 'lst': indices,
        'days': indices}; a missing key, None or selection=None: all) picks of the triads, of the LST and day bins of
        cpinfo['processed']['prelim'] and of the pairs of day-bin pairs of cpinfo['errinfo'] (those made of selected day bins only).
        The caller's dictionary is not modified."""
        if selection is None:
            selection = {}
        elif not isinstance(selection, dict):
            raise TypeError('Input selection must be a dictionary')
        cpinfo = self.cPhase.cpinfo
        triads = [tuple(t) for t in NP.asarray(cpinfo['raw']['triads']).tolist()]
        seltriads = selection.get('triads')
        if seltriads is None:
            seltriads = triads
        triad_ind = NP.asarray([triads.index(tuple(NP.asarray(triad).tolist())) for triad in seltriads], dtype=int)
        prelim = cpinfo['processed'].get('prelim', {})
        shape = prelim['wts'].shape if 'wts' in prelim else None

        def indices(key, axis, what):
            sel = selection.get(key)
            if shape is None:
                return None
            if sel is None:
                return NP.arange(shape[axis])
            if not isinstance(sel, (list, NP.ndarray)):
                raise TypeError('Wrong type for processed {0} indices'.format(what))
            sel = NP.asarray(sel, dtype=int).reshape(-1)
            if NP.any((sel < 0) | (sel >= shape[axis])):
                raise ValueError('Input processed {0} indices out of bounds'.format(what))
            return sel

        lst_ind = indices('lst', 0, 'lst')
        if lst_ind is None:
            raise ValueError('LST index selection could not be performed')
        day_ind = indices('days', 1, 'day')
        if day_ind is None:
            raise ValueError('Day index selection could not be performed')
        day_ind_eicpdiff = None
        pairs = cpinfo.get('errinfo', {}).get('list_of_pair_of_pairs')
        if pairs is not None:
            if selection.get('days') is None:
                day_ind_eicpdiff = NP.arange(len(pairs))
            else:
                chosen = set(day_ind.tolist())
                day_ind_eicpdiff = NP.asarray([i for i, item in enumerate(pairs) if len(set(NP.asarray(item).ravel().tolist()) - chosen) == 0],
                                              dtype=int)
        return (triad_ind, lst_ind, day_ind, day_ind_eicpdiff)

    def beam3Dvol(self, beamparms, freq_wts=None):
        """Integral of the squared power pattern over solid angle and frequency, in Sr Hz, per window of freq_wts (nwin, nchan):
        delay_spectrum.beam3Dvol of the analytic power pattern of beamparms['telescope'] at beamparms['freqs'] on a HEALPix grid of
        beamparms['nside'] (64), evaluated on the device; with 'chromatic' False (default True) the pattern at 'select_freq' (the mean
        of the frequencies) at every channel.  A 'beamfile' raises NotImplementedError.  The caller's dictionary is not modified."""
        from . import delay_spectrum as DS
        if not isinstance(beamparms, dict):
            raise TypeError('Input beamparms must be a dictionary')
        if ('beamfile' not in beamparms) and ('telescope' not in beamparms):
            raise KeyError('Input beamparms does not contain either "beamfile" or "telescope" keys')
        if 'freqs' not in beamparms:
            raise KeyError('Key "freqs" not found in input beamparms')
        freqs = beamparms['freqs']
        if not isinstance(freqs, NP.ndarray):
            raise TypeError('Key "freqs" in input beamparms must contain a numpy array')
        nside = beamparms.get('nside', 64)
        if not isinstance(nside, int):
            raise TypeError('"nside" parameter in input beamparms must be an integer')
        chromatic = beamparms.get('chromatic', True)
        if not isinstance(chromatic, bool):
            raise TypeError('Beam chromaticity parameter in input beamparms must be a boolean')
        if beamparms.get('beamfile') is not None:
            raise NotImplementedError('a beamfile is not supported (its formats need astropy or pyuvdata): give the "telescope"')
        if 'telescope' not in beamparms:
            raise KeyError('Input beamparms does not contain the key "telescope"')
        device = getattr(self.cPhase._ctx, 'device', 0)
        if chromatic:
            beam = DS.healpix_power_pattern(freqs, beamparms['telescope'], nside=nside, device=device)
        else:
            select_freq = beamparms.get('select_freq')
            if select_freq is None:
                select_freq = NP.mean(freqs)
            beam = DS.healpix_power_pattern(NP.asarray([select_freq], dtype=NP.float64), beamparms['telescope'], nside=nside, device=device)
        return DS.beam3Dvol(beam, freqs, freq_wts=freq_wts, hemisphere=True)

    def power_factor(self, cpds, units='K', beamparms=None, cosmo=None):
        """(z, kprll, factor) of one sampling of FT's result (:3395-3416): the redshifts of the windows, k_parallel (nspw, nlags) in
        h/Mpc and the factor that turns (Jy Hz)^2 into Jy^2 Mpc/h, drz_los / bw_eff^2, or into K^2 (Mpc/h)^3,
        rz_los^2 drz_los / bw_eff / omega_bw (wl^2 Jy / 2 k_B)^2."""
        from . import delay_spectrum as DS
        import scipy.constants as FCNST
        cosmo = DS.cosmo100 if cosmo is None else cosmo
        fc, bw = NP.asarray(cpds['freq_center'], dtype=NP.float64).reshape(-1), NP.asarray(cpds['bw_eff'], dtype=NP.float64).reshape(-1)
        wl = FCNST.c / fc
        z = DS.REST_FREQ_HI / fc - 1
        kprll = DS.dkprll_deta(z, cosmo=cosmo).reshape(-1, 1) * NP.asarray(cpds['lags'])
        drz_los = (FCNST.c / 1e3) * bw * (1 + z) ** 2 / DS.REST_FREQ_HI / cosmo.H0.value / cosmo.efunc(z)                 # Mpc/h
        if units == 'Jy':
            factor = (1 / bw) * (drz_los / bw)
        elif units == 'K':
            rz_los = NP.asarray(cosmo.comoving_distance(z).to('Mpc').value, dtype=NP.float64).reshape(-1)
            omega_bw = self.beam3Dvol(beamparms, freq_wts=cpds['freq_wts'])
            factor = (1 / omega_bw) * (rz_los ** 2 * drz_los / bw) * (wl ** 2 * DS.JY / (2 * FCNST.k)) ** 2
        else:
            raise ValueError('Input value for units invalid')
        return z, kprll, NP.ascontiguousarray(factor, dtype=NP.float64)

    def compute_power_spectrum(self, cpds=None, selection=None, autoinfo=None, xinfo=None, cosmo=None, units='K', beamparms=None):
        """Delay power spectra of the closure phases (:2888-3601): the spectra of FT (cpds, by default those of the last FT) of the
        pools 'whole', 'submodel' and 'residual', averaged coherently over autoinfo['axes'] on the host, are cross-multiplied over the
        pairs of xinfo['axes'] (1 LST with the shifts of xinfo['dlst_range'], 2 days, 3 triads) under xinfo['wts']['preX'] and
        collapsed over xinfo['collapse_axes'] on the device (prisim_cphase_xpower), then weighted by xinfo['wts']['postX'], normalised
        ('postXnorm') and averaged ('avgcov') on the host.  Returns the reference's dictionary: 'triads', 'triads_ind', 'lst',
        'lst_ind', 'dlst', 'days', 'day_ind', 'dday', 'lstXoffsets' and per sampling ('oversampled', 'resampled') 'z', 'kprll', 'lags',
        'freq_center', 'bw_eff', 'shape', 'freq_wts', 'lag_corr_length' and per pool 'mean', 'median' (complex128, Jy^2 Mpc/h or
        K^2 (Mpc/h)^3), 'diagoffsets', 'diagweights', 'axesmap', 'nsamples_incoh', 'nsamples_coh'.  xps_stats holds the device
        statistics of the calls.  See the module docstring for the departures."""
        return self._power_spectrum(False, cpds, selection, autoinfo, xinfo, cosmo, units, beamparms)

    def compute_power_spectrum_uncertainty(self, cpds=None, selection=None, autoinfo=None, xinfo=None, cosmo=None, units='K',
                                           beamparms=None):
        """Uncertainty of the delay power spectra from the sub-sample differences (:3605-4357): as compute_power_spectrum on the pool
        'errinfo', dspec0 conj(dspec1) over the pairs of xinfo['axes'], with the reference's keys (top level from cpinfo['errinfo'],
        'day_ind' the pairs of day-bin pairs).  The days axis 2 is dropped from every list of axes."""
        return self._power_spectrum(True, cpds, selection, autoinfo, xinfo, cosmo, units, beamparms)

    @staticmethod
    def _xps_arguments(autoinfo, xinfo, uncertainty):
        """The normalised arguments of the power spectra (:3261-3356) as a dictionary, from copies of the caller's"""
        def axes_of(info, name):
            axes = info.get('axes')
            if axes is None:
                return None
            if isinstance(axes, bool) or not isinstance(axes, (list, tuple, NP.ndarray, int, NP.integer)):
                raise TypeError('Value under key axes in input {0} must be an integer, list, tuple or numpy array'.format(name))
            axes = NP.asarray(axes).reshape(-1)
            if axes.size and (not NP.issubdtype(axes.dtype, NP.integer) or NP.any((axes < 1) | (axes > 3)) or NP.unique(axes).size != axes.size):
                raise ValueError('axes in input {0} must be distinct and among 1 (LST), 2 (days) and 3 (triads)'.format(name))
            return [int(ax) for ax in axes]

        one = [NP.ones(1, dtype=NP.float64)]
        if autoinfo is None:
            autoinfo = {}
        elif not isinstance(autoinfo, dict):
            raise TypeError('Input autoinfo must be a dictionary')
        cohax = axes_of(autoinfo, 'autoinfo')
        awts = autoinfo.get('wts')
        if cohax is None or awts is None:
            awts = one * (1 if cohax is None else len(cohax))
        else:
            if not isinstance(awts, list):
                raise TypeError('wts in input autoinfo must be a list of numpy arrays')
            if len(awts) != len(cohax):
                raise ValueError('Input list of wts must be same as length of autoinfo axes')
        if xinfo is None:
            xinfo = {}
        elif not isinstance(xinfo, dict):
            raise TypeError('Input xinfo must be a dictionary')
        incohax = axes_of(xinfo, 'xinfo')
        nax = 1 if incohax is None else len(incohax)
        wts = xinfo.get('wts')
        X = {'preX': one * nax, 'postX': one * nax, 'preXnorm': False, 'postXnorm': False}
        if wts is not None:
            if incohax is not None:
                if not isinstance(wts, dict):
                    raise TypeError('wts in input xinfo must be a dictionary')
                for xkey in ('preX', 'postX'):
                    if xkey not in wts:
                        raise KeyError('wts in input xinfo lacks the key {0}'.format(xkey))
                    if not isinstance(wts[xkey], list):
                        raise TypeError('{0} wts in input xinfo must be a list of numpy arrays'.format(xkey))
                    if len(wts[xkey]) != len(incohax):
                        raise ValueError('Input list of {0} wts must be same as length of xinfo axes'.format(xkey))
                    X[xkey] = list(wts[xkey])
            if isinstance(wts, dict):
                for nkey in ('preXnorm', 'postXnorm'):
                    if not isinstance(wts.get(nkey, False), (bool, NP.bool_)):
                        raise TypeError('{0} in input xinfo must be a boolean'.format(nkey))
                    X[nkey] = bool(wts.get(nkey, False))
        avgcov = xinfo.get('avgcov', False)
        if not isinstance(avgcov, (bool, NP.bool_)):
            raise TypeError('avgcov under input xinfo must be boolean')
        colax = xinfo.get('collapse_axes', [])
        if isinstance(colax, bool) or not isinstance(colax, (int, NP.integer, list, tuple, NP.ndarray)):
            raise TypeError('collapse_axes under input xinfo must be an integer, tuple, list or numpy array')
        colax = [int(ax) for ax in NP.asarray(colax).reshape(-1)]
        cohax = [] if cohax is None else cohax
        incohax = [] if incohax is None else incohax
        if set(cohax) & set(incohax):
            raise ValueError("Inputs autoinfo['axes'] and xinfo['axes'] must have no intersection")
        if X['preXnorm']:
            raise NotImplementedError('preXnorm is not implemented (the reference calls an undefined logical_or there)')
        preX = dict(zip(incohax, X['preX']))
        if uncertainty:                                   # the days axis is that of the pairs of day-bin pairs: never averaged or crossed
            awts = [w for ax, w in zip(cohax, awts) if ax != 2]
            cohax = [ax for ax in cohax if ax != 2]
            incohax = [ax for ax in incohax if ax != 2]
            colax = [ax for ax in colax if ax != 2]
        if len(set(colax)) != len(colax) or not set(colax) <= set(incohax):
            raise ValueError("xinfo['collapse_axes'] must be distinct axes of xinfo['axes']")
        if len(colax) > len(X['postX']):
            raise ValueError('Input list of postX wts is shorter than the collapsed axes')
        return {'cohax': cohax, 'awts': [NP.asarray(w) for w in awts], 'incohax': incohax, 'preX': {ax: NP.asarray(preX[ax]) for ax in incohax},
                'postX': [NP.asarray(w) for w in X['postX']], 'postXnorm': X['postXnorm'], 'avgcov': bool(avgcov), 'colax': colax,
                'dlst_range': xinfo.get('dlst_range')}

    def _power_spectrum(self, uncertainty, cpds, selection, autoinfo, xinfo, cosmo, units, beamparms):
        from . import delay_spectrum as DS
        if not isinstance(units, str):
            raise TypeError('Input parameter units must be a string')
        if units not in ('Jy', 'K'):
            raise ValueError('Input value for units invalid')
        if units == 'K':
            if not isinstance(beamparms, dict):
                raise TypeError('Input beamparms must be a dictionary')
            beamparms = dict(beamparms)
            if 'freqs' not in beamparms:
                beamparms['freqs'] = self.f
        cosmo = DS.cosmo100 if cosmo is None else cosmo
        A = self._xps_arguments(autoinfo, xinfo, uncertainty)
        cohax, incohax, colax = A['cohax'], A['incohax'], A['colax']
        if selection is not None and not isinstance(selection, dict):
            raise TypeError('Input selection must be a dictionary')
        if cpds is None:
            cpds = {'oversampled': self.cPhaseDS, 'resampled': self.cPhaseDS_resampled}
        elif not isinstance(cpds, dict):
            raise TypeError('Input cpds must be a dictionary')
        sampling = [s for s in ('oversampled', 'resampled') if cpds.get(s) is not None]
        if not sampling:
            raise ValueError('FT must compute the delay spectra before their power spectra')
        triad_ind, lst_ind, day_ind, day_ind_eicpdiff = self.subset(selection=selection)
        cpinfo = self.cPhase.cpinfo
        if uncertainty:
            if day_ind_eicpdiff is None:
                raise ValueError('subsample_differencing must fill the sub-sample differences before their power spectra')
            bins, mid_ind = cpinfo['errinfo'], day_ind_eicpdiff
        else:
            bins, mid_ind = cpinfo['processed']['prelim'], day_ind
        dlst = NP.asarray(bins['dlstbins']).reshape(-1)
        result = {'triads': NP.asarray(cpinfo['raw']['triads'])[triad_ind], 'triads_ind': triad_ind, 'lst': NP.asarray(bins['lstbins'])[lst_ind],
                  'lst_ind': lst_ind, 'dlst': dlst[lst_ind] if dlst.size > 1 else dlst,
                  'days': NP.asarray(bins['daybins'])[day_ind], 'day_ind': mid_ind, 'dday': NP.asarray(bins['diff_dbins'])[day_ind]}
        dlstbin = NP.mean(bins['dlstbins'])
        if A['dlst_range'] is None:
            lstshifts = NP.arange(2)                      # LST index offsets of 0 and 1 only
        else:
            dlst_range = NP.asarray(A['dlst_range'], dtype=NP.float64).ravel() / 60.0
            if dlst_range.size == 1:
                dlst_range = NP.insert(dlst_range, 0, 0.0)
            if not dlstbin > 0.0:
                raise ValueError('dlst_range needs LST bins of a non-zero width')
            lstshifts = NP.arange(max(0, int(NP.ceil(dlst_range.min() / dlstbin))), min(int(NP.ceil(dlst_range.max() / dlstbin)), lst_ind.size))
        result['lstXoffsets'] = lstshifts * dlstbin
        sizes = {1: lst_ind.size, 2: mid_ind.size, 3: triad_ind.size}
        nsamples_coh = int(NP.prod([sizes[ax] for ax in cohax])) if cohax else 1
        nsamples = int(NP.prod([sizes[ax] for ax in incohax])) if incohax else 1
        nsamples_incoh = nsamples * (nsamples - 1) if incohax else 1
        crossed = nsamples_incoh > 1
        collapsing = crossed and len(colax) > 0
        if A['avgcov'] and not collapsing:
            raise ValueError('avgcov needs collapsed axes to average over')
        if uncertainty and not crossed:
            raise ValueError('the uncertainty needs an axis of xinfo to cross the sub-sample differences over')
        modes = tuple(('collapse' if ax in colax else 'full') if (crossed and ax in incohax) else 'none' for ax in (1, 2, 3))
        if crossed and 1 in incohax:
            if lstshifts.size < 1 or NP.any(lstshifts >= lst_ind.size):
                raise ValueError('the LST shifts {0} do not lie inside the {1} selected LST bins'.format(lstshifts.tolist(), lst_ind.size))
        weights = [None, None, None]
        for ax in incohax:
            w = A['preX'][ax].astype(NP.complex128).reshape(-1)
            if w.size not in (1, sizes[ax]):
                raise ValueError('the preX weights of axis {0} must have 1 or {1} entries'.format(ax, sizes[ax]))
            weights[ax - 1] = NP.ascontiguousarray(NP.broadcast_to(w, (sizes[ax],)))
        # the output axes of every input axis: (shift, LST) or (i, j) where crossed, one where collapsed or not crossed
        width = {ax: 2 if modes[ax - 1] == 'full' else 1 for ax in (1, 2, 3)}
        pos = {ax: 1 + sum(width[y] for y in range(1, ax)) for ax in (1, 2, 3)}
        outlen = {1: lstshifts.size, 2: 2 * sizes[2] - 1, 3: 2 * sizes[3] - 1}
        ndim_out = 2 + sum(width.values())
        postX = NP.ones((1,) * ndim_out, dtype=NP.complex128)
        for colaxind, ax in enumerate(colax if collapsing else []):
            w = A['postX'][colaxind].astype(NP.complex128).reshape(-1)
            if w.size not in (1, outlen[ax]):
                raise ValueError('the postX weights of axis {0} must have 1 or {1} entries'.format(ax, outlen[ax]))
            shp = [1] * ndim_out
            shp[pos[ax]] = -1
            postX = postX * w.reshape(shp)
        axes_to_sum = tuple(pos[ax] for ax in colax)

        # the pools: (name, statistic or None) -> the spectra a (and b) and the weights of their coherent average
        def pools_of(ds):
            if uncertainty:
                err = ds.get('errinfo', {})
                if 'dspec0' not in err or 'dspec1' not in err:
                    return []
                return [('errinfo', stat, err['dspec0'][stat], err['dspec1'][stat], err['dspec0']['twts'], err['dspec1']['twts'])
                        for stat in ('mean', 'median') if stat in err['dspec0'] and stat in err['dspec1']]
            out = []
            twts = ds['whole']['dspec']['twts']
            for dpool in ('whole', 'submodel', 'residual'):
                spec = ds.get(dpool, {}).get('dspec')
                if spec is None:
                    continue
                for stat in ('mean', 'median'):
                    x = spec if dpool == 'submodel' else spec.get(stat)
                    if x is not None:
                        out.append((dpool, stat, x, None, twts, None))
            return out

        def coherent(x, twts, stat, chan_twts):
            """the selected spectra averaged over the coherent axes (:3445-3467), the weights at the channel where chan_twts total most"""
            x = NP.asarray(x)[NP.ix_(NP.arange(NP.shape(x)[0]), lst_ind, mid_ind, triad_ind, NP.arange(NP.shape(x)[4]))]
            if nsamples_coh > 1:
                if stat == 'median':
                    return NP.median(x, axis=tuple(cohax), keepdims=True)
                tw = MA.getdata(twts)
                tw = tw[..., [int(NP.argmax(NP.sum(MA.getdata(chan_twts), axis=(0, 1, 2))))]][NP.ix_(lst_ind, mid_ind, triad_ind, NP.arange(1))][NP.newaxis, ...]
                aw = NP.ones((1,) * 5, dtype=NP.complex128)
                for caxind, ax in enumerate(cohax):
                    w = A['awts'][caxind].reshape(-1)
                    if w.size not in (1, sizes[ax]):
                        raise ValueError('the wts of autoinfo axis {0} must have 1 or {1} entries'.format(ax, sizes[ax]))
                    shp = [1] * 5
                    shp[ax] = -1
                    aw = aw * w.reshape(shp)
                return NP.sum(tw * aw * x, axis=tuple(cohax), keepdims=True) / NP.sum(tw * aw, axis=tuple(cohax), keepdims=True)
            return x

        work = []
        for smplng in sampling:
            ds = cpds[smplng]
            z, kprll, factor = self.power_factor(ds, units=units, beamparms=beamparms, cosmo=cosmo)
            result[smplng] = {'z': z, 'kprll': kprll, 'lags': NP.copy(ds['lags']), 'freq_center': ds['freq_center'], 'bw_eff': ds['bw_eff'],
                              'shape': ds['shape'], 'freq_wts': ds['freq_wts'], 'lag_corr_length': ds['lag_corr_length']}
            for dpool, stat, xa, xb, ta, tb in pools_of(ds):
                a = NP.ascontiguousarray(coherent(xa, ta, stat, ta), dtype=NP.complex128)
                b = None if xb is None else NP.ascontiguousarray(coherent(xb, tb, stat, ta), dtype=NP.complex128)
                work.append((smplng, dpool, stat, factor, a, b))

        ctx = self.cPhase._context() if crossed and work else None
        self.xps_stats = {}
        for smplng, dpool, stat, factor, a, b in work:
            out = result[smplng].setdefault(dpool, {})
            diagoffsets, diagweights, axesmap = {}, {}, {}
            if not crossed:
                f5 = factor.reshape(-1, 1, 1, 1, 1)
                p = (f5 * NP.abs(a) ** 2).astype(NP.complex128)
            else:
                res = ctx.cphase_xpower(a, b=b, factor=factor, weights=weights, modes=modes, shifts=lstshifts if 1 in incohax else None,
                                        collapse=colax, stat=stat)
                self.xps_stats[(smplng, dpool, stat)] = res['stats']
                p = res['out']
                for ax in (2, 3):                           # the reference has a at the second and b at the first index of a pair
                    if modes[ax - 1] == 'full':
                        p = NP.swapaxes(p, pos[ax], pos[ax] + 1)
                    elif modes[ax - 1] == 'collapse':
                        p = NP.flip(p, axis=pos[ax])
                axesmap = {ax: (pos[ax] + NP.arange(2) if modes[ax - 1] == 'full' else NP.asarray([pos[ax]])) for ax in incohax}
                if collapsing:
                    for ax in colax:
                        if ax == 1:
                            diagweights[ax] = int(NP.sum(NP.logical_not(NP.isnan(a[0, :, 0, 0, 0])))) - lstshifts
                            diagoffsets[ax] = lstshifts
                        else:
                            diagoffsets[ax] = NP.arange(-(sizes[ax] - 1), sizes[ax])
                            diagweights[ax] = sizes[ax] - NP.abs(diagoffsets[ax])
                    p = p * postX
                    if A['postXnorm']:
                        p = p / NP.nansum(postX, axis=axes_to_sum, keepdims=True)
                    if A['avgcov']:
                        if uncertainty:
                            with warnings.catch_warnings():
                                warnings.simplefilter('ignore', RuntimeWarning)
                                p = NP.nanmean(p, axis=axes_to_sum, keepdims=True)
                        else:
                            dw = NP.ones((1,) * p.ndim)
                            for ax in colax:
                                shp = [1] * p.ndim
                                shp[pos[ax]] = -1
                                dw = dw * NP.asarray(diagweights[ax], dtype=NP.float64).reshape(shp)
                            p = NP.nansum(p * dw, axis=axes_to_sum, keepdims=True) / NP.nansum(dw, axis=axes_to_sum, keepdims=True)
                        for ax in colax:
                            del diagoffsets[ax]
            out[stat] = p
            out.update({'diagoffsets': diagoffsets, 'diagweights': diagweights, 'axesmap': axesmap, 'nsamples_incoh': nsamples_incoh,
                        'nsamples_coh': nsamples_coh})
        return result
