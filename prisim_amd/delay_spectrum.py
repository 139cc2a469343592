"""Delay spectra and delay power spectra of simulated visibilities on the GPU.

Mirrors the part of prisim/delay_spectrum.py that follows the sky-sum in a run: ``DelaySpectrum(ia).delay_transform(pad, freq_wts,
downsample, action)`` (:1224-1342) and ``DelayPowerSpectrum(ds).compute_power_spectrum()`` (:3605-3678, 3982-3995) with the same names,
keywords, attributes and exception types.  The transform itself (window, zero-pad, inverse FFT, shift, decimate) and
``abs(.)**2 * jacobian1 * jacobian2 * Jy2K**2`` run in libprisim_hip.so (prisim_hip_delay_transform*, one HBM-bound kernel for
power-of-two channel counts); the host computes the scalars: redshift, comoving distances, the beam volume, the Jy -> K factor.

Delay CLEAN: ``complex1dClean`` (:133-352) and ``DelaySpectrum.delayClean`` (:1622-1838) run on the GPU (include/prisim_clean.h,
prisim_amd/csrc_clean/clean.hip): one wave64 per (baseline, snapshot) row CLEANs all rows of a chunk in one launch, between rocFFT's
padded inverse transform to lags and the forward transforms of the clean components and residuals; DelayPowerSpectrum then forms the
dps['cc_*'] spectra (:3996-4002).  Departures from the reference are listed in each docstring.

Sub-band delay spectra: ``DelaySpectrum.subband_delay_transform`` (:1842-2250) windows the band around one or more centre frequencies and
transforms every window of every (baseline, snapshot) row in one device call (include/prisim_subband.h, prisim_amd/csrc_subband/);
the astroutils functions it calls are read once in prisim_amd/dsp_readings.py.  ``compute_power_spectrum`` fills the sub-band power
spectra (:4004-4063).

Stacks of runs: ``delay_transform_allruns`` (:1475-1618), ``subband_delay_transform_allruns`` (:2252-2513) and
``DelayPowerSpectrum.compute_power_spectrum_allruns`` (:4067-4195) take the caller's (..., nbl, nchan, n_acc) visibilities, whose leading
axes are runs, and stream them through include/prisim_runs.h (prisim_amd/csrc_runs/) in the reference's layout, with no host transpose.

Closure phases: ``DelaySpectrum.subband_delay_transform_closure_phase`` (:2518-2972) transforms exp(-i closure phase) of every antenna
triad in sub-bands, the phases formed on the device by InterferometerArray.getClosurePhase's code and consumed there
(include/prisim_cpdelay.h, prisim_amd/csrc_closure/cpdelay.hip); ``DelayPowerSpectrum.compute_individual_closure_phase_power_spectrum``
(:4199-4348) and ``compute_averaged_closure_phase_power_spectrum`` (:4352-4540) form their power spectra there.

Not here (out of scope): FITS persistence.

Cosmology.  The reference takes ``astropy.cosmology.Planck15.clone(H0=100)`` (:34-35); astropy is not in this image, so ``cosmo100`` here
is this module's own flat LambdaCDM with Planck15's Om0 = 0.3075, Tcmb0 = 2.7255 K, Neff = 3.046 (photons + massless neutrinos in the
radiation term; Planck15's single 0.06 eV neutrino is not modelled: E(z) differs by ~1e-3 at z ~ 8) -- PARITY UNPINNED against astropy.
Any object with astropy's interface (``H0.value``, ``efunc(z)``, ``comoving_distance(z).to('Mpc').value``,
``comoving_transverse_distance(z)``) is accepted in its place.
"""

import numpy as NP
import scipy.constants as FCNST

from . import _abi
from . import dsp_readings as DSP
from . import geometry as GEOM
from . import interferometry as RI
from . import primary_beams as PB

REST_FREQ_HI = 1420405751.77      # Hz (astroutils.constants.rest_freq_HI, used at :3642, 3707)
JY = 1.0e-26                      # W m^-2 Hz^-1 (astroutils.constants.Jy, :3663)


class _Quantity(object):
    """The two accessors of an astropy Quantity the reference uses: ``.value`` and ``.to('Mpc').value``."""

    def __init__(self, value):
        self.value = value

    def to(self, unit):
        if unit != 'Mpc':
            raise ValueError('only Mpc is supported')
        return self


class FlatLambdaCDM(object):
    """Flat LambdaCDM with radiation: E(z)^2 = Om0 (1+z)^3 + Or0 (1+z)^4 + (1 - Om0 - Or0); comoving distances by quadrature."""

    def __init__(self, H0=100.0, Om0=0.3075, Tcmb0=2.7255, Neff=3.046, name=None):
        self.name = name
        self.H0 = _Quantity(float(H0))
        self.Om0 = float(Om0)
        self.Tcmb0, self.Neff = float(Tcmb0), float(Neff)
        h100 = float(H0) * 1e3 / (1e6 * FCNST.parsec)                              # s^-1
        rho_crit = 3.0 * h100 ** 2 / (8.0 * NP.pi * FCNST.G)                       # kg m^-3
        rho_gamma = 4.0 * FCNST.Stefan_Boltzmann * self.Tcmb0 ** 4 / FCNST.c ** 3  # kg m^-3
        self.Ogamma0 = rho_gamma / rho_crit
        self.Or0 = self.Ogamma0 * (1.0 + 0.22710731766 * self.Neff)                # 7/8 (4/11)^(4/3) per massless species
        self.Ode0 = 1.0 - self.Om0 - self.Or0

    def efunc(self, z):
        zp1 = 1.0 + NP.asarray(z, dtype=NP.float64)
        return NP.sqrt(self.Om0 * zp1 ** 3 + self.Or0 * zp1 ** 4 + self.Ode0)

    def comoving_distance(self, z):
        from scipy.integrate import quad
        dh = FCNST.c / 1e3 / self.H0.value                                         # Mpc
        zs = NP.atleast_1d(NP.asarray(z, dtype=NP.float64))
        out = NP.array([quad(lambda x: 1.0 / float(self.efunc(x)), 0.0, zi, epsabs=0.0, epsrel=1e-12)[0] for zi in zs]) * dh
        return _Quantity(out.reshape(NP.shape(z)) if NP.ndim(z) else float(out[0]))

    def comoving_transverse_distance(self, z):
        return self.comoving_distance(z)                                           # flat


cosmo100 = FlatLambdaCDM(H0=100.0, Om0=0.3075, name='flat LambdaCDM, Planck 2015 Om0, h = 1.0 (:34-35)')


def _is_cosmology(c):
    return hasattr(c, 'H0') and hasattr(c, 'efunc') and hasattr(c, 'comoving_distance') and hasattr(c, 'comoving_transverse_distance')


def dkprll_deta(redshift, cosmo=cosmo100):
    """Jacobian delay -> k_parallel (h/Mpc per second), :357-391."""
    if not isinstance(redshift, (int, float, list, NP.ndarray)):
        raise TypeError('redshift must be a scalar, list or numpy array')
    redshift = NP.asarray(redshift)
    if NP.any(redshift < 0.0):
        raise ValueError('redshift(s) must be non-negative')
    if not _is_cosmology(cosmo):
        raise TypeError('Input cosmology must be a cosmology class defined in Astropy')
    return 2 * NP.pi * cosmo.H0.value * REST_FREQ_HI * cosmo.efunc(redshift) / FCNST.c / (1 + redshift) ** 2 * 1e3      # :389


def beam3Dvol(beam, freqs, freq_wts=None, hemisphere=True):
    """Integral of the squared power pattern over solid angle and frequency, in Sr Hz (:395-489).  beam (npix, nchan | 1) on a
    HEALPix RING grid in the local frame (theta = zenith angle), peak-normalised."""
    if not isinstance(beam, NP.ndarray):
        raise TypeError('Input beam must be a numpy array')
    if not isinstance(freqs, (list, NP.ndarray)):
        raise TypeError('Input freqs must be a list or numpy array')
    freqs = NP.asarray(freqs).astype(NP.float64).reshape(-1)
    if freqs.size < 2:
        raise ValueError('Input freqs does not have enough elements to determine frequency resolution')
    if beam.ndim > 2:
        raise ValueError('Invalid dimensions for beam')
    elif beam.ndim == 2:
        if beam.shape[1] != 1 and beam.shape[1] != freqs.size:
            raise ValueError('Dimensions of beam do not match the number of frequency channels')
    elif beam.ndim == 1:
        beam = beam.reshape(-1, 1)
    else:
        raise ValueError('Invalid dimensions for beam')
    if freq_wts is not None:
        if not isinstance(freq_wts, NP.ndarray):
            raise TypeError('Input freq_wts must be a numpy array')
        if freq_wts.ndim > 2:
            raise ValueError('Input freq_wts must be of shape nwin x nchan')
        freq_wts = NP.asarray(freq_wts).astype(NP.float64).reshape(-1, freqs.size)
    else:
        freq_wts = NP.ones(freqs.size, dtype=NP.float64).reshape(1, -1)
    eps = 1e-10
    if beam.max() > 1.0 + eps:
        raise ValueError('Input beam maximum exceeds unity. Input beam should be normalized to peak of unity')
    npix = beam.shape[0]
    nside = int(round(NP.sqrt(npix / 12.0)))
    if 12 * nside * nside != npix:
        raise ValueError('beam does not have a HEALPix number of pixels')
    domega = 4.0 * NP.pi / npix
    df = freqs[1] - freqs[0]
    bw = df * freqs.size
    theta, _ = GEOM.healpix_pix2ang_ring(nside)
    ind = NP.where(theta <= NP.pi / 2)[0] if hemisphere else NP.arange(npix)
    b2 = beam[ind, :] ** 2                                                               # (npix', nchan | 1)
    # sum over pixels and channels of (beam * wts)^2 for every window (:484), without the (npix, nwin, nchan) temporary
    if b2.shape[1] == 1:
        omega_bw = domega * df * NP.nansum(b2) * NP.sum(freq_wts ** 2, axis=1)
    else:
        omega_bw = domega * df * (freq_wts ** 2).dot(NP.nansum(b2, axis=0))
    if NP.any(omega_bw > 4 * NP.pi * bw):
        raise ValueError('3D volume estimated from beam exceeds the upper limit. Check normalization of the input beam')
    return omega_bw


def healpix_power_pattern(channels, telescope, nside=32, extbeam=None, device=0):
    """(npix, nchan) power pattern at the pixel centres of a HEALPix RING grid in the local frame (theta = zenith angle, phi = azimuth;
    zero below the horizon), evaluated on the GPU: the analytic beam of ``telescope`` (:3956-3963), or an external beam
    ``extbeam = (table (npix_beam, nfreq), spectral interpolation matrix (nchan, nfreq))`` log-interpolated and peak-normalised per channel
    as in a run (:3934-3953; the grid is then no finer than the table's, :3931-3932)."""
    f = NP.asarray(channels, dtype=NP.float64)
    if extbeam is not None:
        beam_nside = int(round(NP.sqrt(extbeam[0].shape[0] / 12.0)))
        if beam_nside < nside:
            nside = beam_nside
    theta, phi = GEOM.healpix_pix2ang_ring(nside)
    up = theta <= NP.pi / 2
    altaz_up = NP.hstack(((90.0 - NP.degrees(theta[up])).reshape(-1, 1), NP.degrees(phi[up]).reshape(-1, 1)))
    beam = NP.zeros((theta.size, f.size))
    if extbeam is not None:
        dc = GEOM.altaz2dircos(altaz_up, 'degrees')
        n = dc.shape[0]
        with _abi.Context(device) as ctx:
            ctx.set_array(NP.zeros((1, 3)), f, nt_max=1)
            ctx.set_external_beam(*extbeam)
            ctx.set_sky_external_analytic(dc, NP.ones(n), NP.zeros(n), 1.0, NP.array([0.0, 0.0, 1.0]))
            beam[up] = ctx.get_pbflux()
    else:
        beam[up] = PB.primary_beam_generator(altaz_up, f, telescope, freq_scale='Hz', skyunits='altaz', east2ax1=0.0, pointing_info=None,
                                             pointing_center=None, device=device)
    return beam


def power_constants(channels, telescope, freq_wts=None, cosmo=cosmo100, nside=32, extbeam=None, device=0):
    """The scalars of DelayPowerSpectrum.__init__ (:3640-3663) for callers that hold a device cube but no InterferometerArray
    (bench.py, tools/): f0, wl0, z, bw, drz_los, rz_los, omega_bw, jacobian1, jacobian2, Jy2K and factor = jacobian1 jacobian2 Jy2K^2
    (a float when freq_wts is one window)."""
    f = NP.asarray(channels, dtype=NP.float64)
    df = f[1] - f[0]
    f0 = f[int(f.size / 2)]
    wl0 = FCNST.c / f0
    z = REST_FREQ_HI / f0 - 1
    bw = df * f.size
    drz_los = (FCNST.c / 1e3) * bw * (1 + z) ** 2 / REST_FREQ_HI / cosmo.H0.value / float(cosmo.efunc(z))
    rz_los = cosmo.comoving_distance(z).to('Mpc').value
    omega_bw = beam3Dvol(healpix_power_pattern(f, telescope, nside=nside, extbeam=extbeam, device=device), f,
                         freq_wts=None if freq_wts is None else NP.asarray(freq_wts, dtype=NP.float64))
    jacobian1 = 1 / omega_bw
    jacobian2 = rz_los ** 2 * drz_los / bw
    Jy2K = wl0 ** 2 * JY / (2 * FCNST.k)
    factor = jacobian1 * jacobian2 * Jy2K ** 2
    return {'f0': f0, 'wl0': wl0, 'z': z, 'bw': bw, 'drz_los': drz_los, 'rz_los': rz_los, 'omega_bw': omega_bw, 'jacobian1': jacobian1,
            'jacobian2': jacobian2, 'Jy2K': Jy2K, 'factor': float(factor[0]) if factor.size == 1 else factor,
            'cosmology': getattr(cosmo, 'name', None) or type(cosmo).__name__}


def _check_clean_args(threshold_type, threshold, gain, maxiter):
    """The argument checks of complex1dClean that do not depend on the rows (:195-203, 246-256), with the reference's exception types and
    messages; returns threshold as a float."""
    if threshold_type not in ['relative', 'absolute']:
        raise ValueError('invalid specification for threshold_type')
    if not isinstance(threshold, (int, float)):
        raise TypeError('input threshold must be a scalar')
    threshold = float(threshold)
    if threshold <= 0.0:
        raise ValueError('input threshold must be positive')
    if threshold_type == 'relative' and threshold >= 1.0:
        raise ValueError('incompatible value specified for threshold')
    return threshold


def _check_gain_maxiter(gain, maxiter):
    if not isinstance(gain, float):
        raise TypeError('gain must be a floating point number')
    if (gain <= 0.0) or (gain >= 1.0):
        raise TypeError('gain must lie between 0 and 1')
    if not isinstance(maxiter, int):
        raise TypeError('maxiter must be an integer')
    if maxiter <= 0:
        raise ValueError('maxiter must be positive')


def complex1dClean(inp, kernel, cbox=None, gain=0.1, maxiter=10000, threshold=5e-3, threshold_type='relative', verbose=False,
                   progressbar=False, pid=None, progressbar_yloc=0, device=0):
    """Hogbom CLEAN of a complex 1-D array on the GPU (prisim/delay_spectrum.py:133-352, prisim_clean_rows).

    As the reference: the kernel is divided by its max modulus; each iteration takes the first argmax of |res * cbox|, adds
    gain * res there to the clean components and subtracts that times the kernel rolled onto it; it stops when |maxres| <=
    lolim * max|inp| (cond1), after maxiter iterations (cond2), or when the median absolute deviation of the residuals inside the
    box is <= that outside it (cond3).  Returns {'termination': {'threshold', 'maxiter', 'inrms<outrms'}, 'iter', 'rms', 'inrms',
    'outrms', 'res', 'cc'}.

    Extension: a 2-D ``inp`` (nrows, m) cleans every row in one launch (kernel (m,) or (nrows, m), cbox (m,) or (nrows, m)); the
    entries are then arrays over the rows (outrms NaN where undefined) and 'stats' holds the device timing and iteration sum.
    Departures (one test each in tests/test_delay_clean.py):
      - with <= 2 entries outside the box the reference raises UnboundLocalError (cond3 is never assigned): here cond3 is False and
        outrms None;
      - 'inrms' / 'outrms' are the final values, not per-iteration histories; 'rms' (the MAD of the whole array) decides nothing and
        is None.
    verbose, progressbar, pid and progressbar_yloc are accepted and ignored.  Rows are complex128 on the device; up to 4096 entries."""
    if not isinstance(inp, NP.ndarray):
        raise TypeError('inp must be a numpy array')
    if not isinstance(kernel, NP.ndarray):
        raise TypeError('kernel must be a numpy array')
    if threshold_type not in ['relative', 'absolute']:
        raise ValueError('invalid specification for threshold_type')
    if not isinstance(threshold, (int, float)):
        raise TypeError('input threshold must be a scalar')
    threshold = float(threshold)
    if threshold <= 0.0:
        raise ValueError('input threshold must be positive')
    rows = inp.ndim == 2
    x = NP.ascontiguousarray(inp if rows else inp.reshape(1, -1), dtype=NP.complex128)
    nrows, m = x.shape
    k = NP.asarray(kernel, dtype=NP.complex128)
    if rows and k.ndim == 2 and k.shape[0] == nrows and k.shape[0] > 1:
        kidx = NP.arange(nrows, dtype=NP.int32)
    else:
        k, kidx = k.reshape(1, -1), None
    if k.shape[1] != m:
        raise ValueError('inp and kernel must have same size')
    if cbox is None:
        box = NP.ones((nrows, m), dtype=bool)
    elif isinstance(cbox, NP.ndarray):
        if cbox.size not in (m, nrows * m):
            raise ValueError('Clean box must be of same size as input')
        box = NP.broadcast_to(NP.where(cbox > 0.0, True, False).reshape(-1, m), (nrows, m))
    else:
        raise TypeError('cbox must be a numpy array')
    if threshold_type == 'relative':
        lolim = NP.full(nrows, threshold)
    else:
        with NP.errstate(divide='ignore'):
            lolim = threshold / NP.abs(x).max(axis=1)
    if NP.any(lolim >= 1.0):
        raise ValueError('incompatible value specified for threshold')
    _check_gain_maxiter(gain, maxiter)
    with _abi.Context(device) as ctx:
        cc, res, iters, flags, rms, stats = ctx.clean_rows(x, k, box, gain, maxiter, threshold, absolute=threshold_type == 'absolute',
                                                           kidx=kidx)
    if NP.any(flags & _abi.PRISIM_CLEAN_BAD_THRESHOLD):
        raise ValueError('incompatible value specified for threshold')
    term = {'threshold': (flags & _abi.PRISIM_CLEAN_THRESHOLD) != 0, 'maxiter': (flags & _abi.PRISIM_CLEAN_MAXITER) != 0,
            'inrms<outrms': (flags & _abi.PRISIM_CLEAN_INRMS) != 0}
    if rows:
        return {'termination': term, 'iter': iters, 'rms': None, 'inrms': rms[:, 0], 'outrms': rms[:, 1], 'cc': cc, 'res': res,
                'stats': stats}
    no_out = bool(flags[0] & _abi.PRISIM_CLEAN_NO_OUTRMS)
    return {'termination': {key: bool(v[0]) for key, v in term.items()}, 'iter': int(iters[0]), 'rms': None, 'inrms': float(rms[0, 0]),
            'outrms': None if no_out else float(rms[0, 1]), 'cc': cc[0], 'res': res[0]}


class DelaySpectrum(object):
    """Delay spectra of an InterferometerArray's visibilities (prisim/delay_spectrum.py:493-1342, the argument path of __init__ and
    delay_transform()).  Attributes as in the reference: ia, f, df, n_acc, bp, bp_wts, pad, lags, lag_kernel, skyvis_lag, vis_lag,
    vis_noise_lag, horizon_delay_limits; the CLEAN attributes after delayClean(), the sub-band ones after subband_delay_transform()."""

    def __init__(self, interferometer_array=None, init_file=None):
        if init_file is not None:
            raise NotImplementedError('DelaySpectrum(init_file=...): FITS persistence is out of scope (SURVEY.md 2.1 row 17)')
        if not isinstance(interferometer_array, RI.InterferometerArray):
            raise TypeError('Input interferometer_array must be an instance of class InterferometerArray')
        self.ia = interferometer_array
        self.f = interferometer_array.channels
        self.df = interferometer_array.freq_resolution
        self.n_acc = interferometer_array.n_acc
        self.horizon_delay_limits = self.get_horizon_delay_limits()
        self.pad = 0.0
        self.lags = NP.fft.fftshift(NP.fft.fftfreq(self.f.size, self.df))               # DSP.spectral_axis(N, delx=df, shift=True), :1191
        self._bp_wts_override = None
        self._lag_kernel, self._lag_kernel_maker = None, None
        self._skyvis_lag, self._lag_resident = None, None
        self.vis_lag = None
        self.vis_noise_lag = None
        self.clean_window_buffer = 1.0
        for name in ('cc_lags', 'cc_freq', 'cc_lag_kernel', 'cc_skyvis_lag', 'cc_skyvis_res_lag', 'cc_vis_lag', 'cc_vis_res_lag',
                     'cc_skyvis_net_lag', 'cc_vis_net_lag', 'cc_skyvis_freq', 'cc_skyvis_res_freq', 'cc_vis_freq', 'cc_vis_res_freq',
                     'cc_skyvis_net_freq', 'cc_vis_net_freq'):
            setattr(self, name, None)
        self.subband_delay_spectra = {}
        self.subband_delay_spectra_resampled = {}

    # bp / bp_wts: the array's own attributes (dense (nbl, nchan, n_acc) on read, as in the reference) unless delay_transform(action='store')
    # replaced the weights
    @property
    def bp(self):
        return self.ia.bp

    @property
    def bp_wts(self):
        return self._bp_wts_override if self._bp_wts_override is not None else self.ia.bp_wts

    @bp_wts.setter
    def bp_wts(self, value):
        self._bp_wts_override = value

    # skyvis_lag: a stored result the transform left resident on the device (an interferometry._ResidentLags) is fetched when read
    @property
    def skyvis_lag(self):
        if self._lag_resident is not None and self._skyvis_lag is None:
            self._skyvis_lag = self._lag_resident.spectra()
        return self._skyvis_lag

    @skyvis_lag.setter
    def skyvis_lag(self, value):
        self._skyvis_lag, self._lag_resident = value, None

    @property
    def lag_kernel(self):
        if self._lag_kernel is None and self._lag_kernel_maker is not None:
            self._lag_kernel = self._lag_kernel_maker()
            self._lag_kernel_maker = None
        return self._lag_kernel

    @lag_kernel.setter
    def lag_kernel(self, value):
        self._lag_kernel, self._lag_kernel_maker = value, None

    def get_horizon_delay_limits(self, phase_center=None, phase_center_coords=None):
        """(n_phase_centres, nbl, 2): min / max delay of the horizon for every baseline, shifted by the phase centre (:2976-3030 and
        baseline_delay_horizon.py:100-129)."""
        if phase_center is None:
            phase_center = self.ia.phase_center
            phase_center_coords = self.ia.phase_center_coords
        if phase_center_coords not in ['hadec', 'altaz', 'dircos']:
            raise ValueError('Phase center coordinates must be "altaz", "hadec" or "dircos"')
        pc = NP.asarray(phase_center, dtype=NP.float64)
        pc = pc.reshape(-1, 3 if phase_center_coords == 'dircos' else 2)
        if phase_center_coords == 'hadec':
            pc_dircos = GEOM.altaz2dircos(GEOM.hadec2altaz(pc, self.ia.latitude, units='degrees'), units='degrees')
        elif phase_center_coords == 'altaz':
            pc_dircos = GEOM.altaz2dircos(pc, units='degrees')
        else:
            pc_dircos = pc
        bl = NP.asarray(self.ia.baselines, dtype=NP.float64)
        dmax = NP.sqrt(NP.sum(bl ** 2, axis=1)).reshape(1, -1) / FCNST.c                # baseline_delay_horizon.py:94
        shift = pc_dircos.dot(bl.T) / FCNST.c                                            # :95
        return NP.dstack((-dmax - shift, dmax - shift))                                  # :127-128

    def set_horizon_delay_limits(self):
        self.horizon_delay_limits = self.get_horizon_delay_limits()

    # ------------------------------------------------------------------------------------------
    def _window_factors(self, freq_wts):
        """Per-snapshot bandpass and window layers, each of shape (1 | nbl, nchan), as two lists of n_acc entries; plus the freq_wts
        to report (a zero-copy broadcast view when one window serves every baseline and snapshot)."""
        ia = self.ia
        nbl, nchan, nt = ia.baselines.shape[0], self.f.size, self.n_acc
        stacks = getattr(ia, '_stacks', {})

        def layers_of(name):
            st = stacks.get(name)
            if st is not None and len(st.layers) == nt and nt > 0:
                return list(st.layers)
            dense = NP.asarray(getattr(ia, name))
            if dense.ndim == 2:
                return [dense] * max(nt, 1)
            return [dense[:, :, t] for t in range(dense.shape[2])]

        bp_layers = layers_of('bp')
        if freq_wts is not None:
            if freq_wts.size == nchan:                                                   # :1275-1276
                w = NP.asarray(freq_wts, dtype=NP.float64).reshape(1, -1)
                w_layers = [w] * max(nt, 1)
                report = NP.broadcast_to(w.reshape(1, -1, 1), (nbl, nchan, nt))
            elif freq_wts.size == nchan * nt:                                            # :1277-1278
                w2 = NP.asarray(freq_wts, dtype=NP.float64).reshape(nchan, -1)
                w_layers = [w2[:, t].reshape(1, -1) for t in range(nt)]
                report = NP.broadcast_to(w2[NP.newaxis, :, :], (nbl, nchan, nt))
            elif freq_wts.size == nchan * nbl:                                           # :1279-1280
                w2 = NP.asarray(freq_wts, dtype=NP.float64).reshape(-1, nchan)
                w_layers = [w2] * max(nt, 1)
                report = NP.broadcast_to(w2[:, :, NP.newaxis], (nbl, nchan, nt))
            elif freq_wts.size == nchan * nbl * nt:                                      # :1281-1282
                report = NP.asarray(freq_wts, dtype=NP.float64).reshape(nbl, nchan, nt)
                w_layers = [report[:, :, t] for t in range(nt)]
            else:
                raise ValueError('window shape dimensions incompatible with number of channels and/or number of tiemstamps.')
        else:
            if self._bp_wts_override is not None:
                report = NP.asarray(self._bp_wts_override)
                w_layers = [report[:, :, t] for t in range(report.shape[2])] if report.ndim == 3 else [report] * max(nt, 1)
            else:
                w_layers = layers_of('bp_wts')
                report = None                                                            # the array's own (dense on read)
        n = min(len(bp_layers), len(w_layers))
        return [NP.asarray(l) for l in bp_layers[:n]], [NP.asarray(l) for l in w_layers[:n]], report

    def delay_transform(self, pad=1.0, freq_wts=None, downsample=True, action=None, verbose=True):
        """IFFT of visibilities * bandpass * window along frequency on the GPU (:1224-1342): skyvis_lag, vis_lag, vis_noise_lag (for
        the cubes that exist), lag_kernel, lags, freq_wts, pad.  With the visibility cube resident in HBM (InterferometerArray.reserve)
        and one window for every snapshot, the spectra stay on the device until ``skyvis_lag`` is read."""
        if verbose:
            print('Preparing to compute delay transform...\n\tChecking input parameters for compatibility...')
        if not isinstance(pad, (int, float)):
            raise TypeError('pad fraction must be a scalar value.')
        if pad < 0.0:
            pad = 0.0
            if verbose:
                print('\tPad fraction found to be negative. Resetting to 0.0 (no padding will be applied).')
        if freq_wts is not None:
            freq_wts = NP.asarray(freq_wts)
        bp_layers, w_layers, report = self._window_factors(freq_wts)
        if verbose:
            print('\tFrequency window weights assigned.')
        if not isinstance(downsample, bool):
            raise TypeError('Input downsample must be of boolean type')
        nchan = self.f.size
        if self.n_acc == 0:
            raise ValueError('no visibilities to transform: call observe() first')
        result = {'freq_wts': report if report is not None else self.bp_wts, 'pad': pad}
        nfft = int(nchan * (1 + pad))
        result['lags'] = NP.fft.fftshift(NP.fft.fftfreq(nfft, self.df))                 # :1303
        decimate = downsample or pad == 0.0
        sky, _, vis_lag, vis_noise_lag, make_kernel = self.ia._transform_cubes([b * w for b, w in zip(bp_layers, w_layers)], pad, decimate)
        resident = isinstance(sky, RI._ResidentLags)

        if decimate and pad > 0.0:
            result['lags'] = result['lags'][NP.arange(0, nfft, 1 + pad).astype(int)] if float(1 + pad).is_integer() else \
                NP.interp(NP.arange(0, nfft, 1 + pad), NP.arange(nfft), result['lags'])    # DSP.downsampler(lags, 1 + pad), :1329
            # as many as the spectra have (arange has one position more, nfft itself, where nfft / (1 + pad) rounds up past an integer)
            result['lags'] = result['lags'].flatten()[:_abi.delay_nout(nchan, pad)]
            if verbose:
                print('\tDelay transform products downsampled by factor of {0:.1f}'.format(1 + pad))
                print('delay_transform() completed successfully.')

        if action == 'store':
            self.pad = pad
            self.lags = result['lags']
            if report is not None:
                self._bp_wts_override = report
            self._skyvis_lag, self._lag_resident = (None, sky) if resident else (sky, None)   # (only a STORED result keeps resident spectra)
            self.vis_lag = vis_lag
            self.vis_noise_lag = vis_noise_lag
            self._lag_kernel, self._lag_kernel_maker = None, make_kernel
        if resident:
            result['skyvis_lag'] = sky.spectra() if action != 'store' else _Deferred(lambda: self.skyvis_lag)
        else:
            result['skyvis_lag'] = sky
        result['vis_lag'] = vis_lag
        result['vis_noise_lag'] = vis_noise_lag
        result['lag_kernel'] = _Deferred(make_kernel) if action == 'store' else make_kernel()
        return _LazyDict(result)


    def delayClean(self, pad=1.0, freq_wts=None, clean_window_buffer=1.0, gain=0.1, maxiter=10000, threshold=5e-3,
                   threshold_type='relative', parallel=False, nproc=None, verbose=True):
        """Delay transform and CLEAN of the sky and noisy visibilities on the GPU (:1622-1838, prisim_clean_delay): the windowed rows
        vis * bp * bp_wts are zero-padded to M = nchan + int(nchan * pad) lags and inverse-transformed (M df ifft, :1738-1740), every
        (baseline, snapshot) row is CLEANed with the lag kernel of bp * bp_wts inside the box of lags within the horizon limits widened by
        clean_window_buffer / bw (:1764), and the clean components and residuals are transformed back, times deta * pad_factor
        (:1808-1815).  Assigns lags (unshifted), skyvis_lag, vis_lag, lag_kernel, cc_lag_kernel (full length, shifted), cc_lags (shifted)
        and the cc_skyvis_* / cc_vis_* lag and frequency products (:1816-1838); bp_wts when freq_wts is given.  The whole call is
        validated and computed before any attribute changes.

        Departures (one test each in tests/test_delay_clean.py):
          - the box is made per (baseline, snapshot) whatever ``parallel`` says (the parallel branch, :1763-1764; the serial branch
            never resets its box, so each row would get the union of all earlier rows' boxes); ``parallel`` and ``nproc`` have no effect;
          - with <= 2 lags outside the box cond3 is False (the reference raises UnboundLocalError);
          - on a noiseless array (vis_freq None) vis_lag and the cc_vis_* attributes stay None;
          - a one-row horizon_delay_limits serves every snapshot (the reference indexes it by snapshot and raises IndexError);
          - complex1dClean's per-iteration rms histories are not formed."""
        if not isinstance(pad, (int, float)):
            raise TypeError('pad fraction must be a scalar value.')
        if pad < 0.0:
            pad = 0.0
            if verbose:
                print('\tPad fraction found to be negative. Resetting to 0.0 (no padding will be applied).')
        if freq_wts is not None:
            freq_wts = NP.asarray(freq_wts)
        bp_layers, w_layers, report = self._window_factors(freq_wts)
        threshold = _check_clean_args(threshold_type, threshold, gain, maxiter)
        _check_gain_maxiter(gain, maxiter)
        ia = self.ia
        nbl, nchan, nt = ia.baselines.shape[0], self.f.size, self.n_acc
        if nt == 0:
            raise ValueError('no visibilities to clean: call observe() first')
        hdl = NP.asarray(self.horizon_delay_limits, dtype=NP.float64)
        if hdl.ndim != 3 or hdl.shape[1:] != (nbl, 2) or hdl.shape[0] not in (1, nt):
            raise ValueError('horizon_delay_limits must have shape (1 or n_acc, n_baselines, 2)')
        bw = self.df * nchan
        npad = int(nchan * pad)
        m = nchan + npad
        lags = NP.fft.fftfreq(m, self.df)                                               # DSP.spectral_axis(..., shift=False), :1736
        # :1764, one box per (baseline, snapshot)
        boxes = NP.logical_and(lags <= hdl[:, :, 1:2] + clean_window_buffer / bw, lags >= hdl[:, :, 0:1] - clean_window_buffer / bw)
        deta = lags[1] - lags[0]
        pad_factor = (1.0 + 1.0 * npad / nchan)
        cubes = [NP.asarray(ia.skyvis_freq, dtype=NP.complex128)]
        if ia.vis_freq is not None:
            cubes.append(NP.asarray(ia.vis_freq, dtype=NP.complex128))
        ncubes = len(cubes)
        wins = [bp_layers[t] * w_layers[t] for t in range(nt)]                          # self.bp * self.bp_wts (:1740)
        ctx = ia._ctx
        chunk = max(1, min(nt, (1 << 30) // max(1, ncubes * nbl * m * 16)))
        names = ('lag', 'cc', 'res', 'cc_freq', 'res_freq')
        full = {name: NP.empty((ncubes, nt, nbl, m), dtype=NP.complex128) for name in names}
        kern_full = NP.empty((nt, nbl, m), dtype=NP.complex128)
        iters = NP.empty((ncubes, nt, nbl), dtype=NP.int32)
        flags = NP.empty((ncubes, nt, nbl), dtype=NP.int32)
        stats = []
        for t0 in range(0, nt, chunk):
            t1 = min(nt, t0 + chunk)
            kwin, kidx = RI._distinct_layers(wins[t0:t1], nbl)                         # the distinct windows of the chunk, rows' indices
            win = NP.empty((ncubes, t1 - t0, nbl, nchan), dtype=NP.complex128)
            for c, cube in enumerate(cubes):
                for t in range(t0, t1):
                    win[c, t - t0] = (cube[:, :, t] * bp_layers[t]) * w_layers[t]         # skyvis_freq * bp * bp_wts (:1738-1739)
            box = boxes[NP.arange(t0, t1) if hdl.shape[0] > 1 else NP.zeros(t1 - t0, dtype=int)]
            out = ctx.clean_delay(win.reshape(ncubes, -1, nchan), kwin, box.reshape(-1, m), m, self.df, deta, pad_factor, gain, maxiter,
                                  threshold, absolute=threshold_type == 'absolute', kidx=None if kwin.shape[0] == 1 else kidx.ravel())
            for name in names:
                full[name][:, t0:t1] = out[name].reshape(ncubes, t1 - t0, nbl, m)
            kern_full[t0:t1] = out['kern_lag'][kidx.ravel()].reshape(t1 - t0, nbl, m) if kwin.shape[0] > 1 else out['kern_lag'][0]
            iters[:, t0:t1] = out['iters'].reshape(ncubes, t1 - t0, nbl)
            flags[:, t0:t1] = out['flags'].reshape(ncubes, t1 - t0, nbl)
            stats.append(out['stats'])
        if NP.any(flags & _abi.PRISIM_CLEAN_BAD_THRESHOLD):
            raise ValueError('incompatible value specified for threshold')

        def cube(c, name, shift):
            x = NP.transpose(full[name][c], (1, 2, 0))                                  # (nt, nbl, M) -> (nbl, M, nt)
            return NP.fft.fftshift(x, axes=1) if shift else NP.ascontiguousarray(x)

        # commit (:1816-1838)
        if report is not None:
            self._bp_wts_override = report
        self.lags = lags
        self.skyvis_lag = cube(0, 'lag', True)
        self.vis_lag = cube(1, 'lag', True) if ncubes > 1 else None
        self.lag_kernel = NP.fft.fftshift(NP.transpose(kern_full, (1, 2, 0)), axes=1)
        self.cc_lag_kernel = self.lag_kernel
        for c, name in enumerate(('skyvis', 'vis')):
            have = c < ncubes
            lag_cc, lag_res = (cube(c, 'cc', True), cube(c, 'res', True)) if have else (None, None)
            f_cc, f_res = (cube(c, 'cc_freq', False), cube(c, 'res_freq', False)) if have else (None, None)
            setattr(self, 'cc_%s_lag' % name, lag_cc)
            setattr(self, 'cc_%s_res_lag' % name, lag_res)
            setattr(self, 'cc_%s_net_lag' % name, lag_cc + lag_res if have else None)
            setattr(self, 'cc_%s_freq' % name, f_cc)
            setattr(self, 'cc_%s_res_freq' % name, f_res)
            setattr(self, 'cc_%s_net_freq' % name, f_cc + f_res if have else None)
        self.cc_lags = NP.fft.fftshift(lags)
        self.clean_window_buffer = clean_window_buffer
        self._clean_iters = NP.transpose(iters, (0, 2, 1))                               # (cube, baseline, snapshot)
        self._clean_stats = {'device_ms': sum(s['device_ms'] for s in stats), 'clean_ms': sum(s['clean_ms'] for s in stats),
                             'sum_iter': int(sum(s['sum_iter'] for s in stats)), 'rows': int(sum(s['rows'] for s in stats)),
                             'calls': len(stats)}
        if verbose:
            print('delayClean() completed: {0} rows, {1} iterations'.format(self._clean_stats['rows'], self._clean_stats['sum_iter']))

    def subband_delay_transform(self, bw_eff, freq_center=None, shape=None, fftpow=None, pad=None, bpcorrect=False, action=None,
                                verbose=True):
        """Delay spectra of frequency sub-bands on the GPU (:1842-2250, prisim_subband_transform).  For key 'sim' the cubes skyvis_freq,
        vis_freq and vis_noise_freq, for key 'cc' (only after delayClean) cc_{skyvis,vis}{,_res,_net}_freq[:, :nchan, :], times self.bp
        times every window of subband_freq_wts, zero-padded to M = nchan + int(nchan pad) and transformed, M df fftshift(ifft(.))
        (:2196-2206).  subband_delay_spectra[key] holds freq_center, shape, freq_wts, bw_eff, npad, lags, lag_kernel, lag_corr_length and
        the spectra, each (nbl, n_win, M, n_acc); subband_delay_spectra_resampled[key] the same FFT-resampled (DSP.downsampler, read in
        prisim_amd/dsp_readings.py) to round(M / factor) lags, lags and lag_kernel linearly interpolated (:2220-2236).  action None,
        'return_oversampled' or 'return_resampled'; the attributes are always updated, and only after the whole call succeeded.

        Reproduced literally: windows sorted by channel while freq_center / bw_eff keep the given order; windows truncated at the band
        edges; the resampling factor of every key uses the npad of the last key processed (:2225); 'interp' lags (ceil(M / factor)) and
        'FFT' spectra (round(M / factor)) may differ in length; bpcorrect is recorded and has no effect (:2190 computes the factor and
        never applies it).
        Departures (one test each in tests/test_subband.py): the default freq_center is f[int(nchan / 2)]; on a noiseless array vis_lag /
        vis_noise_lag (and the cc_vis_* spectra) are None; fftpow other than 1 raises NotImplementedError
        (dsp_readings.window_fftpow); the caller's dictionaries are not modified."""
        f, df, ia = self.f, self.df, self.ia
        nchan = f.size
        bw_eff, freq_center, shape, fftpow, pad = _check_subband_args(f, df, bw_eff, freq_center, shape, fftpow, pad, bpcorrect, verbose)
        nbl, nt = ia.baselines.shape[0], self.n_acc
        keys = [key for key in SUBBAND_KEYS if key == 'sim' or self.cc_lags is not None]
        if nt == 0:
            raise ValueError('no visibilities to transform: call observe() first')
        # the inputs of every key, checked before anything is computed
        plan = {}
        for key in keys:
            freq_wts = subband_freq_wts(f, df, bw_eff[key], freq_center[key], shape[key], fftpow[key])
            npad = int(nchan * pad[key])
            m = nchan + npad
            if m > _abi.PRISIM_SUBBAND_MAX_LEN:
                raise ValueError('sub-band spectra of %d lags exceed PRISIM_SUBBAND_MAX_LEN = %d' % (m, _abi.PRISIM_SUBBAND_MAX_LEN))
            if key == 'cc':
                names = ('skyvis', 'vis', 'skyvis_res', 'vis_res', 'skyvis_net', 'vis_net')
                srcs = [getattr(self, 'cc_%s_freq' % name) for name in names]
                srcs = [None if x is None else x[:, :nchan, :] for x in srcs]
            else:
                names = ('skyvis', 'vis', 'vis_noise')
                srcs = [ia.skyvis_freq, ia.vis_freq, ia.vis_noise_freq]
            plan[key] = {'freq_wts': freq_wts, 'npad': npad, 'm': m, 'names': names, 'srcs': srcs}
        # :2225 -- the factor of every key takes the npad left over from the last key of the loop above
        last_npad = plan[keys[-1]]['npad']
        for key in keys:
            p = plan[key]
            p['factor'] = NP.min((nchan + last_npad) * df / bw_eff[key])
            p['nres'] = DSP.fft_downsample_length(p['m'], p['factor'])
            if p['nres'] > _abi.PRISIM_SUBBAND_MAX_LEN:
                raise ValueError('resampled sub-band spectra of %d lags exceed PRISIM_SUBBAND_MAX_LEN = %d'
                                 % (p['nres'], _abi.PRISIM_SUBBAND_MAX_LEN))
        bp_layers, _, _ = self._window_factors(None)
        bp_same = RI._all_same(bp_layers)
        # the lag kernel: one transform per row of each distinct bandpass layer, gathered to (nbl, n_win, M, n_acc)
        kern_rows, kidx = RI._distinct_layers(bp_layers[:nt], nbl)
        ctx = ia._ctx

        result, result_resampled, stats = {}, {}, []
        for key in keys:
            p = plan[key]
            m, nres, nwin = p['m'], p['nres'], p['freq_wts'].shape[0]
            have = [i for i, x in enumerate(p['srcs']) if x is not None]
            cubes = [NP.asarray(p['srcs'][i]) for i in have]
            over = [NP.empty((nbl, nwin, m, nt), dtype=NP.complex128) for _ in have]
            res = [NP.empty((nbl, nwin, nres, nt), dtype=NP.complex128) for _ in have]
            chunk = max(1, min(nt, (1 << 30) // max(1, len(have) * nbl * nwin * (m + nres) * 16)))
            for t0 in range(0, nt, chunk):
                t1 = min(nt, t0 + chunk)
                x = NP.empty((len(have), t1 - t0, nbl, nchan), dtype=NP.complex128)
                for c, cube in enumerate(cubes):
                    x[c] = NP.transpose(cube[:, :, t0:t1], (2, 0, 1))
                if bp_same:
                    bp = bp_layers[0]
                else:
                    bp = NP.concatenate([NP.broadcast_to(bp_layers[t], (nbl, nchan)) for t in range(t0, t1)], axis=0)
                out = ctx.subband_transform(x, bp, p['freq_wts'], m, df, nres=nres, want=('over', 'res'))
                stats.append(out['stats'])
                for c in range(len(have)):
                    over[c][..., t0:t1] = NP.transpose(out['over'][c], (1, 2, 3, 0))
                    res[c][..., t0:t1] = NP.transpose(out['res'][c], (1, 2, 3, 0))
            k = ctx.subband_transform(kern_rows.reshape(1, 1, -1, nchan), NP.ones((1, nchan)), p['freq_wts'], m, df, want=('over',))
            k = k['over'][0, 0]                                                              # (distinct rows, n_win, M)
            lag_kernel = NP.ascontiguousarray(NP.transpose(k[kidx], (1, 2, 3, 0)))
            lags = DSP.spectral_axis(m, delx=df, use_real=False, shift=True)
            r = {'freq_center': freq_center[key], 'shape': shape[key], 'freq_wts': p['freq_wts'], 'bw_eff': bw_eff[key], 'npad': p['npad'],
                 'lags': lags, 'lag_kernel': lag_kernel, 'lag_corr_length': nchan / NP.sum(p['freq_wts'], axis=1)}
            rr = {'freq_center': freq_center[key], 'bw_eff': bw_eff[key]}
            rr['lags'] = DSP.downsampler(lags, p['factor'], axis=-1, method='interp', kind='linear')
            rr['lag_kernel'] = DSP.downsampler(lag_kernel, p['factor'], axis=2, method='interp', kind='linear')
            for i, name in enumerate(p['names']):
                c = have.index(i) if i in have else None
                r[name + '_lag'] = over[c] if c is not None else None
                rr[name + '_lag'] = res[c] if c is not None else None
            dlag = rr['lags'][1] - rr['lags'][0]
            rr['lag_corr_length'] = (1 / bw_eff[key]) / dlag
            if key == 'cc':
                r['bpcorrect'] = bpcorrect
            result[key], result_resampled[key] = r, rr
        if verbose:
            print('\tSub-band(s) delay transform computed')
            print('\tDownsampled Sub-band(s) delay transform computed')
        # commit
        self.subband_delay_spectra = result
        self.subband_delay_spectra_resampled = result_resampled
        self._subband_stats = {'device_ms': sum(st['device_ms'] for st in stats), 'kernel_ms': sum(st['kernel_ms'] for st in stats),
                               'rows': sum(st['rows'] for st in stats), 'routes': sorted(set(st['route'] for st in stats)),
                               'calls': len(stats)}
        if action == 'return_oversampled':
            return result
        if action == 'return_resampled':
            return result_resampled


    # ------------------------------------------------------------------------------------------
    # stacks of runs: the caller's visibilities (..., nbl, nchan, n_acc), prisim_runs_transform (include/prisim_runs.h)
    def _check_runs_vis(self, vis):
        """The vis checks of :1543-1556 / :2393-2406.  Returns vis with at least one leading axis (a view) and (nbl, nchan, nt)."""
        nbl, nchan, nt = self.ia.baselines.shape[0], self.f.size, self.n_acc
        if not isinstance(vis, NP.ndarray):
            raise TypeError('Input vis must be a numpy array')
        elif vis.ndim < 3:
            raise ValueError('Input vis must be at least 3-dimensional')
        elif vis.shape[-3:] == (nbl, nchan, nt):
            vis = vis.reshape((1,) + vis.shape if vis.ndim == 3 else vis.shape)
        else:
            raise ValueError('Input vis does not have compatible shape')
        return vis, nbl, nchan, nt

    def delay_transform_allruns(self, vis, pad=1.0, freq_wts=None, downsample=True, verbose=True):
        """Delay spectra of a stack of runs on the GPU (:1475-1618, prisim_runs_transform): vis (..., nbl, nchan, n_acc), the leading
        axes being runs, times self.bp times the weights, zero-padded to M = nchan + int(nchan pad) lags and transformed,
        M df fftshift(ifft(.)) along the channel axis (nchan df without padding); with downsample every (1 + pad)-th lag, linearly
        interpolated for a non-integer factor (the reading DelaySpectrum.delay_transform takes).  Returns freq_wts (reshaped as the
        reference does), pad, lags, vis_lag (..., nbl, nlags, n_acc) and lag_kernel (1, ..., nbl, nlags, n_acc), the transform of
        bp * freq_wts, computed once for all runs.  freq_wts: (nchan,), (nchan, n_acc), (nbl, nchan) or (nbl, nchan, n_acc); None: bp_wts.
        Nothing is set on self and the caller's arrays are not modified; the spectra are written by the device in the reference's layout.

        Reproduced literally: a freq_wts of vis's own shape raises ValueError (:1583, ``elif not freq_wts.shape != vis.shape``); the lags
        are the int(nchan (1 + pad)) of :1600, downsampled like the spectra.
        Departures (one test each in tests/test_allruns.py): other freq_wts shapes, which the reference leaves to numpy broadcasting,
        are taken when they broadcast over the trailing (nbl, nchan, n_acc) axes only, and weights that vary from run to run raise
        NotImplementedError; spectra longer than PRISIM_SUBBAND_MAX_LEN lags raise ValueError before any device work."""
        if verbose:
            print('Preparing to compute delay transform...\n\tChecking input parameters for compatibility...')
        vis, nbl, nchan, nt = self._check_runs_vis(vis)
        if not isinstance(pad, (int, float)):
            raise TypeError('pad fraction must be a scalar value.')
        if pad < 0.0:
            pad = 0.0
            if verbose:
                print('\tPad fraction found to be negative. Resetting to 0.0 (no padding will be applied).')
        ones = (1,) * (vis.ndim - 3)
        if freq_wts is not None:
            shp = NP.shape(freq_wts)
            fw = NP.asarray(freq_wts)
            if shp == self.f.shape:
                report = fw.reshape(ones + (1, -1, 1))
            elif shp == (nchan, nt):
                report = fw.reshape(ones + (1, nchan, nt))
            elif shp == (nbl, nchan):
                report = fw.reshape(ones + (nbl, nchan, 1))
            elif shp == (nbl, nchan, nt):
                report = fw.reshape(ones + (nbl, nchan, nt))
            elif not shp != vis.shape:
                raise ValueError('window shape dimensions incompatible with number of channels and/or number of tiemstamps.')
            else:
                report = fw                                                              # left to numpy broadcasting in the reference
                try:
                    full = NP.broadcast_shapes(shp, vis.shape)
                except ValueError:
                    raise ValueError('window shape dimensions incompatible with number of channels and/or number of tiemstamps.')
                if full != vis.shape or any(d != 1 for d in shp[:-3]):
                    raise NotImplementedError('freq_wts that vary from run to run (shape %s) are not supported; weights must broadcast '
                                              'over the trailing (nbl, nchan, n_acc) axes' % (shp,))
            wts3 = report.reshape(report.shape[-3:]) if report.ndim > 3 else report
        else:
            wts3 = NP.asarray(self.bp_wts)
            report = wts3.reshape(ones + wts3.shape)
        if verbose:
            print('\tFrequency window weights assigned.')
        if not isinstance(downsample, bool):
            raise TypeError('Input downsample must be of boolean type')
        npad = int(nchan * pad) if pad != 0.0 else 0
        m = nchan + npad
        if m > _abi.PRISIM_SUBBAND_MAX_LEN:
            raise ValueError('delay spectra of %d lags exceed PRISIM_SUBBAND_MAX_LEN = %d' % (m, _abi.PRISIM_SUBBAND_MAX_LEN))
        if verbose:
            print('\tInput parameters have been verified to be compatible.\n\tProceeding to compute delay transform.')
        lags = DSP.spectral_axis(int(nchan * (1 + pad)), delx=self.df, use_real=False, shift=True)         # :1600
        kw = {'m': m, 'scale': m * self.df, 'mode': 'all'}
        if downsample:
            kw.update(mode='interp', factor=1 + pad, nout=NP.arange(0, m, 1 + pad).size)
            lags = DSP.downsampler(lags, 1 + pad, method='interp').flatten()
        bp = NP.asarray(self.bp)
        ctx = self.ia._ctx
        vis_lag, _ = ctx.runs_transform(vis, nbl, nchan, nt, bp=bp, wts=wts3, **kw)
        kernel, _ = ctx.runs_transform(None, nbl, nchan, nt, bp=bp, wts=wts3, **kw)
        nlags = vis_lag.shape[-2]
        if verbose:
            print('\tDelay transform computed ' + ('without padding.' if pad == 0.0 else 'with padding fraction {0:.1f}'.format(pad)))
            if downsample:
                print('\tDelay transform products downsampled by factor of {0:.1f}'.format(1 + pad))
                print('delay_transform() completed successfully.')
        return {'freq_wts': report, 'pad': pad, 'lags': lags, 'vis_lag': vis_lag.reshape(vis.shape[:-3] + (nbl, nlags, nt)),
                'lag_kernel': kernel.reshape(ones + (nbl, nlags, nt))}

    def subband_delay_transform_allruns(self, vis, bw_eff, freq_center=None, shape=None, fftpow=None, pad=None, bpcorrect=False,
                                        action=None, verbose=True):
        """Sub-band delay spectra of a stack of runs on the GPU (:2252-2513, prisim_runs_transform): vis (..., nbl, nchan, n_acc) times
        self.bp times every window of subband_freq_wts, zero-padded to M = nchan + int(nchan pad) lags; returned FFT-resampled
        (DSP.downsampler 'FFT', read in prisim_amd/dsp_readings.py) to round(M / factor) lags with factor = min(M df / bw_eff), the
        spectra formed on the device from the windowed channels directly (the M-lag spectra are never formed).  Returns freq_center,
        shape, freq_wts (n_win, 1, ..., 1, nchan, 1), bw_eff, npad, lags and lag_kernel (n_win, 1, ..., nbl, nlags, n_acc) linearly
        interpolated at arange(0, M, factor), vis_lag (n_win, ..., nbl, nres, n_acc) and lag_corr_length.  Nothing is set on self.

        Reproduced literally: any action other than None returns the resampled dictionary (:2490, ``action = 'return_resampled'``);
        windows sorted by channel while freq_center / bw_eff keep the given order; 'interp' lags (ceil(M / factor)) and 'FFT' spectra
        (round(M / factor)) may differ in length; bpcorrect has no effect.
        Departures (one test each in tests/test_allruns.py): action=None raises its ValueError before anything is computed (the
        reference computes first); the default freq_center is f[int(nchan / 2)]; fftpow other than 1 raises NotImplementedError
        (dsp_readings.window_fftpow)."""
        vis, nbl, nchan, nt = self._check_runs_vis(vis)
        f, df = self.f, self.df
        if not isinstance(bw_eff, (int, float, list, NP.ndarray)):
            raise TypeError('Value of effective bandwidth must be a scalar, list or numpy array')
        # the checks of :2408-2447 are those of subband_delay_transform for one key (both keys given the caller's value), but for the
        # window shape, which is compared case-insensitively here (shape.lower())
        if shape is not None:
            if not isinstance(shape, str):
                raise TypeError('Window shape must be a string')
            if shape.lower() not in ['rect', 'bhw', 'bnw']:
                raise ValueError('Invalid value for window shape specified.')
        else:
            shape = 'rect'
        both = lambda v: None if v is None else {'sim': v, 'cc': v}
        bw, fc, _, fpow, pd = _check_subband_args(f, df, both(bw_eff), both(freq_center), None, both(fftpow), both(pad), False, verbose)
        bw_eff, freq_center, fftpow, pad = bw['sim'], fc['sim'], fpow['sim'], pd['sim']
        if action is None:
            raise ValueError('Invalid value specified for keyword input action')
        freq_wts = subband_freq_wts(f, df, bw_eff, freq_center, shape, fftpow)
        nwin = freq_wts.shape[0]
        npad = int(nchan * pad)
        m = nchan + npad
        if m > _abi.PRISIM_SUBBAND_MAX_LEN:
            raise ValueError('sub-band spectra of %d lags exceed PRISIM_SUBBAND_MAX_LEN = %d' % (m, _abi.PRISIM_SUBBAND_MAX_LEN))
        factor = NP.min((nchan + npad) * df / bw_eff)
        nres = DSP.fft_downsample_length(m, factor)
        if not 1 <= nres <= _abi.PRISIM_SUBBAND_MAX_LEN:
            raise ValueError('resampled sub-band spectra of %d lags must lie in 1 .. PRISIM_SUBBAND_MAX_LEN = %d'
                             % (nres, _abi.PRISIM_SUBBAND_MAX_LEN))
        lags = DSP.downsampler(DSP.spectral_axis(m, delx=df, use_real=False, shift=True), factor, axis=-1, method='interp', kind='linear')
        bp = NP.asarray(self.bp)
        ctx = self.ia._ctx
        vis_lag, _ = ctx.runs_transform(vis, nbl, nchan, nt, bp=bp, win=freq_wts, m=m, scale=m * df, mode='resample', nout=nres)
        kernel, _ = ctx.runs_transform(None, nbl, nchan, nt, bp=bp, win=freq_wts, m=m, scale=m * df, mode='interp', factor=factor,
                                       nout=NP.arange(0, m, factor).size)
        if verbose:
            print('\tSub-band(s) delay transform computed')
        ones = (1,) * (vis.ndim - 3)
        dlag = lags[1] - lags[0]
        return {'freq_center': freq_center, 'shape': shape, 'freq_wts': freq_wts.reshape((nwin,) + ones + (1, nchan, 1)), 'bw_eff': bw_eff,
                'npad': npad, 'lags': lags, 'vis_lag': vis_lag.reshape((nwin,) + vis.shape[:-3] + (nbl, nres, nt)),
                'lag_kernel': kernel.reshape((nwin,) + ones + (nbl, kernel.shape[-2], nt)), 'lag_corr_length': (1 / bw_eff) / dlag}

    def subband_delay_transform_closure_phase(self, bw_eff, cpinfo=None, antenna_triplets=None, specsmooth_info=None,
                                              delay_filter_info=None, spectral_window_info=None, freq_center=None, shape=None,
                                              fftpow=None, pad=None, action=None, verbose=True):
        """Sub-band delay spectra of closure phases on the GPU (:2518-2972, prisim_closure_delay_spectra): for every antenna triad,
        snapshot and window of subband_freq_wts, exp(-1j closure phase) times the window, zero-padded to M = nchan + int(nchan pad) lags
        and transformed, M df fftshift(ifft(.)) (:2943), and that FFT-resampled (DSP.downsampler 'FFT', read in
        prisim_amd/dsp_readings.py) to round(M / factor) lags, factor = min(M df / bw_eff) (:2955-2962).

        cpinfo None: the closure phases are those InterferometerArray.getClosurePhase(antenna_triplets, specsmooth_info,
        delay_filter_info, spectral_window_info) gives, formed on the device by the same code and transformed where they lie -- neither
        the triplets nor the phases are downloaded -- for skyvis, and for vis / noise when those cubes exist.  cpinfo given: its
        'closure_phase_skyvis' / '_vis' / '_noise' arrays (ntriplets, ..., nchan, nt), any number of middle axes, are uploaded and
        transformed; antenna_triplets and the three *_info arguments are then unused, as in the reference.

        Returns, for action None or 'return_resampled': antenna_triplets, baseline_triplets, freq_center, bw_eff, freq_wts, lags and
        lag_kernel (linearly interpolated at arange(0, M, factor)), lag_corr_length = (1 / bw_eff) / dlag, and the spectra
        (ntriplets, ..., n_win, nres, nt); the M-lag spectra are then not downloaded.  For 'return_oversampled': freq_center, shape,
        freq_wts, bw_eff, npad, lags, lag_kernel, lag_corr_length = nchan / sum(freq_wts) and the spectra (ntriplets, ..., n_win, M, nt).
        No attribute of self is set; the stats of the device calls are left in ia.closure_delay_stats, per key.

        Reproduced literally (one test each in tests/test_cpdelay.py):
          - the oversampled dictionary carries no antenna_triplets / baseline_triplets (:2937 rebinds the result);
          - windows are sorted by channel while freq_center / bw_eff keep the given order;
          - lag_kernel is the transform of the windows alone, of shape (1, ..., n_win, M, 1);
          - lag_corr_length of the resampled result is (1 / bw_eff) / dlag.
        Departures (one test each):
          - the default freq_center is f[int(nchan / 2)] (the reference indexes with a float);
          - fftpow other than 1 raises NotImplementedError (dsp_readings.window_fftpow), and so does specsmooth_info when cpinfo is None
            (getClosurePhase);
          - a closure_phase_* entry that is None (a noiseless array) is skipped and comes back as None;
          - a cpinfo with none of the three keys raises ValueError (the reference: NameError on available_CP_key);
          - M or the resampled length above PRISIM_CPDELAY_MAX_LEN, and an action other than None, 'return_resampled' or
            'return_oversampled', raise ValueError before any device work (the reference computes first)."""
        f, df, ia = self.f, self.df, self.ia
        nchan = f.size
        if not isinstance(bw_eff, (int, float, list, NP.ndarray)):
            raise TypeError('Value of effective bandwidth must be a scalar, list or numpy array')
        # the checks of :2855-2900 are those of subband_delay_transform for one key (both keys given the caller's value)
        both = lambda v: None if v is None else {'sim': v, 'cc': v}
        if freq_center is not None and not isinstance(freq_center, (int, float, list, NP.ndarray)):
            raise TypeError('Values(s) of frequency center must be scalar, list or numpy array')
        bw, fc, shp, fpow, pd = _check_subband_args(f, df, both(bw_eff), both(freq_center), both(shape), both(fftpow), both(pad), False,
                                                    verbose)
        bw_eff, freq_center, shape, fftpow, pad = bw['sim'], fc['sim'], shp['sim'], fpow['sim'], pd['sim']
        if cpinfo is not None and not isinstance(cpinfo, dict):
            raise TypeError('Input cpinfo must be a dictionary')
        if action is not None and (not isinstance(action, str) or action.lower() not in ('return_resampled', 'return_oversampled')):
            raise ValueError('Invalid action specified')
        oversampled = action is not None and action.lower() == 'return_oversampled'
        freq_wts = subband_freq_wts(f, df, bw_eff, freq_center, shape, fftpow)
        nwin = freq_wts.shape[0]
        npad = int(nchan * pad)
        m = nchan + npad
        if m > _abi.PRISIM_CPDELAY_MAX_LEN:
            raise ValueError('closure-phase delay spectra of %d lags exceed PRISIM_CPDELAY_MAX_LEN = %d' % (m, _abi.PRISIM_CPDELAY_MAX_LEN))
        factor = NP.min(m * df / bw_eff)
        nres = DSP.fft_downsample_length(m, factor)
        if not 1 <= nres <= _abi.PRISIM_CPDELAY_MAX_LEN:
            raise ValueError('resampled closure-phase delay spectra of %d lags must lie in 1 .. PRISIM_CPDELAY_MAX_LEN = %d'
                             % (nres, _abi.PRISIM_CPDELAY_MAX_LEN))
        keys = ('closure_phase_skyvis', 'closure_phase_vis', 'closure_phase_noise')
        want = ('over',) if oversampled else ('res',)
        kw = {'nres': 0 if oversampled else nres, 'want': want}
        spectra, stats, nlead = {}, {}, 1
        if cpinfo is not None:
            triplets = {'antenna_triplets': cpinfo['antenna_triplets'], 'baseline_triplets': cpinfo['baseline_triplets']}     # :2907
            have = [key for key in cpinfo if key in keys]
            if not have:
                raise ValueError('Input cpinfo holds none of closure_phase_skyvis, closure_phase_vis, closure_phase_noise')
            arrays = {}
            for key in have:
                if cpinfo[key] is None:
                    continue
                arr = NP.asarray(cpinfo[key], dtype=NP.float64)
                if arr.ndim < 3 or arr.shape[-2] != nchan:
                    raise ValueError('%s must have shape ntriplets x ... x nchan x ntimes' % key)
                arrays[key] = arr
                nlead = arr.ndim - 2                                                      # (:2945 takes the last key found)
            ctx = ia._ctx
            for key in have:
                if key not in arrays:
                    spectra[key] = None
                    continue
                out = ctx.closure_delay_spectra(freq_wts, m, df, phases=arrays[key], **kw)
                spectra[key], stats[key] = out[want[0]], out['stats']
        else:
            p = RI._closure_prepare(ia, antenna_triplets, delay_filter_info, specsmooth_info, spectral_window_info, False)
            triplets = {'antenna_triplets': p['antenna_triplets'], 'baseline_triplets': p['baseline_triplets']}
            ntriads, nt = p['legs'].shape[0], p['nt']
            for key, cube in ((keys[0], None if p['resident'] else ia.skyvis_freq), (keys[1], ia.vis_freq), (keys[2], ia.vis_noise_freq)):
                if key != keys[0] and cube is None:
                    spectra[key] = None
                    continue
                if not ntriads:
                    spectra[key] = NP.zeros((0, nwin, m if oversampled else nres, nt), dtype=NP.complex128)
                    continue
                out = ia._ctx.closure_delay_spectra(freq_wts, m, df, cube=cube, legs=p['legs'], conj=p['conj'], bpwts=p['bpwts'],
                                                    freq_wts=p['freq_wts'], masks=p['masks'], mask_index=p['mask_index'], nt=nt, **kw)
                spectra[key], stats[key] = out[want[0]], out['stats']
        ia.closure_delay_stats = stats
        lags = DSP.spectral_axis(m, delx=df, use_real=False, shift=True)
        padded = NP.zeros((nwin, m), dtype=NP.float64)
        padded[:, :nchan] = freq_wts
        lag_kernel = (NP.fft.fftshift(NP.fft.ifft(padded, axis=-1), axes=-1) * m * df).reshape((1,) * nlead + (nwin, m, 1))      # :2945
        if verbose:
            print('\tSub-band(s) delay transform computed')
        if oversampled:
            result = {'freq_center': freq_center, 'shape': shape, 'freq_wts': freq_wts, 'bw_eff': bw_eff, 'npad': npad, 'lags': lags,
                      'lag_corr_length': nchan / NP.sum(freq_wts, axis=-1)}
            result.update(spectra)
            result['lag_kernel'] = lag_kernel
            return result
        result = dict(triplets)
        result.update({'freq_center': freq_center, 'bw_eff': bw_eff, 'freq_wts': freq_wts})
        result['lags'] = DSP.downsampler(lags, factor, axis=-1, method='interp', kind='linear')
        result['lag_kernel'] = DSP.downsampler(lag_kernel, factor, axis=-2, method='interp', kind='linear')
        dlag = result['lags'][1] - result['lags'][0]
        result['lag_corr_length'] = (1 / bw_eff) / dlag
        result.update(spectra)
        if verbose:
            print('\tDownsampled Sub-band(s) delay transform computed')
        return result



SUBBAND_KEYS = ('cc', 'sim')


def subband_freq_wts(f, df, bw_eff, freq_center, shape, fftpow):
    """The (n_win, nchan) windows of subband_delay_transform (:2159-2177): a window of n_window = round(bw_eff / df / frac_width) channels
    scaled by sqrt(frac_width n_window), its peak on the channel nearest each centre, truncated at the band edges; rows in channel order
    (sortind), not in the order the centres were given."""
    f = NP.asarray(f, dtype=NP.float64)
    nchan = f.size
    frac_width = DSP.window_N2width(n_window=None, shape=shape, fftpow=fftpow, area_normalize=False, power_normalize=True)
    window_loss_factor = 1 / frac_width
    n_window = NP.round(window_loss_factor * bw_eff / df).astype(int)
    ind_freq_center, ind_channels, dfrequency = DSP.find_1NN(f.reshape(-1, 1), freq_center.reshape(-1, 1), distance_ULIM=0.5 * df,
                                                             remove_oob=True)
    sortind = NP.argsort(ind_channels)
    ind_channels = ind_channels[sortind]
    n_window = n_window[sortind]
    freq_wts = NP.empty((bw_eff.size, nchan), dtype=NP.float64)
    for i, ind_chan in enumerate(ind_channels):
        window = NP.sqrt(frac_width * n_window[i]) * DSP.window_fftpow(n_window[i], shape=shape, fftpow=fftpow, centering=True, peak=None,
                                                                       area_normalize=False, power_normalize=True)
        window_chans = f[ind_chan] + df * (NP.arange(n_window[i]) - int(n_window[i] / 2))
        ind_window_chans, ind_chans, dfreq = DSP.find_1NN(f.reshape(-1, 1), window_chans.reshape(-1, 1), distance_ULIM=0.5 * df,
                                                          remove_oob=True)
        sind = NP.argsort(ind_window_chans)
        ind_window_chans = ind_window_chans[sind]
        ind_chans = ind_chans[sind]
        window = window[ind_window_chans]
        window = NP.pad(window, ((ind_chans.min(), nchan - 1 - ind_chans.max())), mode='constant', constant_values=((0.0, 0.0)))
        freq_wts[i, :] = window
    return freq_wts


def _check_subband_args(f, df, bw_eff, freq_center, shape, fftpow, pad, bpcorrect, verbose):
    """The argument checks of :2073-2147 with the reference's exception types, on copies of the caller's dictionaries (the reference
    writes its normalised values back into them).  Returns the normalised (bw_eff, freq_center, shape, fftpow, pad)."""
    if not isinstance(bw_eff, dict):
        raise TypeError('Effective bandwidth must be specified as a dictionary')
    bw_eff = dict(bw_eff)
    for key in SUBBAND_KEYS:
        if key in bw_eff:
            if not isinstance(bw_eff[key], (int, float, list, NP.ndarray)):
                raise TypeError('Value of effective bandwidth must be a scalar, list or numpy array')
            bw_eff[key] = NP.asarray(bw_eff[key]).reshape(-1)
            if NP.any(bw_eff[key] <= 0.0):
                raise ValueError('All values in effective bandwidth must be strictly positive')
    if freq_center is None:
        # the reference's self.f[self.f.size/2] is a float index under `from __future__ import division` (departure: int(nchan / 2))
        freq_center = {key: NP.asarray(f[int(f.size / 2)]).reshape(-1) for key in SUBBAND_KEYS}
    elif isinstance(freq_center, dict):
        freq_center = dict(freq_center)
        for key in SUBBAND_KEYS:
            if isinstance(freq_center[key], (int, float, list, NP.ndarray)):
                freq_center[key] = NP.asarray(freq_center[key]).reshape(-1)
                if NP.any((freq_center[key] <= f.min()) | (freq_center[key] >= f.max())):
                    raise ValueError('Value(s) of frequency center(s) must lie strictly inside the observing band')
            else:
                raise TypeError('Values(s) of frequency center must be scalar, list or numpy array')
    else:
        raise TypeError('Input frequency center must be specified as a dictionary')
    for key in SUBBAND_KEYS:
        if (bw_eff[key].size == 1) and (freq_center[key].size > 1):
            bw_eff[key] = NP.repeat(bw_eff[key], freq_center[key].size)
        elif (bw_eff[key].size > 1) and (freq_center[key].size == 1):
            freq_center[key] = NP.repeat(freq_center[key], bw_eff[key].size)
        elif bw_eff[key].size != freq_center[key].size:
            raise ValueError('Effective bandwidth(s) and frequency center(s) must have same number of elements')
    if shape is not None:
        if not isinstance(shape, dict):
            raise TypeError('Window shape must be specified as a dictionary')
        for key in SUBBAND_KEYS:
            if not isinstance(shape[key], str):
                raise TypeError('Window shape must be a string')
            if shape[key] not in ['rect', 'bhw', 'bnw', 'RECT', 'BHW', 'BNW']:
                raise ValueError('Invalid value for window shape specified.')
    else:
        shape = {key: 'rect' for key in SUBBAND_KEYS}
    if fftpow is None:
        fftpow = {key: 1.0 for key in SUBBAND_KEYS}
    else:
        if not isinstance(fftpow, dict):
            raise TypeError('Power to raise FFT of window by must be specified as a dictionary')
        for key in SUBBAND_KEYS:
            if not isinstance(fftpow[key], (int, float)):
                raise TypeError('Power to raise window FFT by must be a scalar value.')
            if fftpow[key] < 0.0:
                raise ValueError('Power for raising FFT of window by must be positive.')
    if pad is None:
        pad = {key: 1.0 for key in SUBBAND_KEYS}
    else:
        if not isinstance(pad, dict):
            raise TypeError('Padding for delay transform must be specified as a dictionary')
        pad = dict(pad)
        for key in SUBBAND_KEYS:
            if not isinstance(pad[key], (int, float)):
                raise TypeError('pad fraction must be a scalar value.')
            if pad[key] < 0.0:
                pad[key] = 0.0
                if verbose:
                    print('\tPad fraction found to be negative. Resetting to 0.0 (no padding will be applied).')
    if not isinstance(bpcorrect, bool):
        raise TypeError('Input keyword bpcorrect must be of boolean type')
    return bw_eff, freq_center, shape, fftpow, pad


class _Deferred(object):
    def __init__(self, fn):
        self.fn = fn


class _LazyDict(dict):
    """dict whose _Deferred values are materialised on first access (a 120 GB spectrum cube is only pulled over PCIe when read)."""

    def __getitem__(self, key):
        v = dict.__getitem__(self, key)
        if isinstance(v, _Deferred):
            v = v.fn()
            dict.__setitem__(self, key, v)
        return v

    def get(self, key, default=None):
        return self[key] if key in self else default

    def items(self):
        return [(k, self[k]) for k in self.keys()]

    def values(self):
        return [self[k] for k in self.keys()]


class DelayPowerSpectrum(object):
    """Delay power spectra in K^2 (Mpc/h)^3 from delay spectra in Jy Hz (prisim/delay_spectrum.py:3355-3678, 3982-3995)."""

    def __init__(self, dspec, cosmo=cosmo100):
        if not isinstance(dspec, DelaySpectrum):
            raise TypeError('Input dspec must be an instance of class DelaySpectrum')
        if not _is_cosmology(cosmo):
            raise TypeError('Input cosmology must be a cosmology class defined in Astropy')
        self.cosmo = cosmo
        self.ds = dspec
        self.f = self.ds.f
        self.lags = self.ds.lags
        self.cc_lags = self.ds.cc_lags
        self.bl = self.ds.ia.baselines
        self.bl_length = self.ds.ia.baseline_lengths
        self.df = self.ds.df
        self.f0 = self.f[int(self.f.size / 2)]                                          # :3640
        self.wl0 = FCNST.c / self.f0
        self.z = REST_FREQ_HI / self.f0 - 1                                             # :3642
        self.bw = self.df * self.f.size
        self.kprll = self.k_parallel(self.lags, redshift=self.z, action='return')       # h/Mpc
        self.kperp = self.k_perp(self.bl_length, redshift=self.z, action='return')      # h/Mpc
        self.horizon_kprll_limits = self.k_parallel(self.ds.horizon_delay_limits, redshift=self.z, action='return')
        self.drz_los = self.comoving_los_depth(self.bw, self.z, action='return')        # Mpc/h
        self.rz_transverse = self.comoving_transverse_distance(self.z, action='return')
        self.rz_los = self.comoving_los_distance(self.z, action='return')
        omega_bw = self.beam3Dvol(freq_wts=self._first_window())                        # :3655 freq_wts = ds.bp_wts[0,:,0]
        self.jacobian1 = 1 / omega_bw                                                   # :3656
        self.jacobian2 = self.rz_los ** 2 * self.drz_los / self.bw                      # :3658
        self.Jy2K = self.wl0 ** 2 * JY / (2 * FCNST.k)                                  # :3659
        self.K2Jy = 1 / self.Jy2K
        self.dps = {}
        for key in ('skyvis', 'vis', 'noise', 'cc_skyvis', 'cc_vis', 'cc_skyvis_res', 'cc_vis_res', 'cc_skyvis_net', 'cc_vis_net'):
            self.dps[key] = None
        self.subband_delay_power_spectra = {}
        self.subband_delay_power_spectra_resampled = {}

    def _first_window(self):
        """ds.bp_wts[0, :, 0] without forming the dense (nbl, nchan, n_acc) array."""
        ds = self.ds
        if ds._bp_wts_override is not None:
            w = NP.asarray(ds._bp_wts_override)
            return NP.array(w[0, :, 0] if w.ndim == 3 else w[0, :], dtype=NP.float64)
        st = getattr(ds.ia, '_stacks', {}).get('bp_wts')
        if st is not None and st.layers:
            return NP.array(NP.broadcast_to(st.layers[0], (st.layers[0].shape[0], self.f.size))[0], dtype=NP.float64)
        w = NP.asarray(ds.ia.bp_wts)
        return NP.array(w[0, :, 0] if w.ndim == 3 else w[0, :], dtype=NP.float64)

    def comoving_los_depth(self, bw, redshift, action=None):
        drz_los = (FCNST.c / 1e3) * bw * (1 + redshift) ** 2 / REST_FREQ_HI / self.cosmo.H0.value / self.cosmo.efunc(redshift)   # :3707
        if action is None:
            self.z = redshift
            self.drz_los = drz_los
            return
        return drz_los

    def comoving_transverse_distance(self, redshift, action=None):
        rz_transverse = self.cosmo.comoving_transverse_distance(redshift).to('Mpc').value        # :3741
        if action is None:
            self.z = redshift
            self.rz_transverse = rz_transverse
            return
        return rz_transverse

    def comoving_los_distance(self, redshift, action=None):
        rz_los = self.cosmo.comoving_distance(redshift).to('Mpc').value                          # :3775
        if action is None:
            self.z = redshift
            self.rz_los = rz_los
            return
        return rz_los

    def k_parallel(self, lags, redshift, action=None):
        kprll = dkprll_deta(redshift, cosmo=self.cosmo) * lags                                   # :3813-3814
        if action is None:
            self.z = redshift
            self.kprll = kprll
            return
        return kprll

    def k_perp(self, baseline_length, redshift, action=None):
        kperp = 2 * NP.pi * (baseline_length / self.wl0) / self.comoving_transverse_distance(redshift, action='return')   # :3853
        if action is None:
            self.z = redshift
            self.kperp = kperp
            return
        return kperp

    def beam3Dvol(self, freq_wts=None, nside=32):
        """Omega x bandwidth of the array's power pattern (:3864-3978): the pattern is evaluated on the GPU at the pixel centres of a
        HEALPix grid in the local frame -- the analytic beam of ia.telescope, or the external beam the array was given
        (InterferometerArray.set_external_beam: log-interpolated in frequency, peak-normalised per channel) -- and squared and summed
        over the upper hemisphere and the band."""
        ia = self.ds.ia
        beam = healpix_power_pattern(self.f, ia.telescope, nside=nside, extbeam=getattr(ia, '_extbeam', None),
                                     device=getattr(ia._ctx, 'device', 0))
        return beam3Dvol(beam, self.f, freq_wts=freq_wts, hemisphere=True)

    def power_scale(self):
        """jacobian1 * jacobian2 * Jy2K**2 (:3992) as a scalar (one spectral window)."""
        return float(NP.ravel(self.jacobian1 * self.jacobian2 * self.Jy2K ** 2)[0])

    def compute_power_spectrum(self):
        """dps['skyvis' | 'vis' | 'noise'] = abs(lag spectrum)**2 * jacobian1 * jacobian2 * Jy2K**2 (:3982-3995), and after
        DelaySpectrum.delayClean the six dps['cc_*'] of the clean components, residuals and their sums (:3996-4002).  When the delay
        spectra are resident on the device the product is formed there (prisim_hip_delay_transform_device with power_scale = the factor)
        and fetched when dps['skyvis'] is read.  After DelaySpectrum.subband_delay_transform it fills subband_delay_power_spectra[key]
        (z, dz, kprll, kperp, horizon_kprll_limits, rz_los, rz_transverse, drz_los, jacobian1 = 1 / beam3Dvol(freq_wts), jacobian2,
        Jy2K, factor per window, and abs(spectrum)**2 * factor of every product) and subband_delay_power_spectra_resampled[key] (kprll,
        kperp, horizon_kprll_limits, the resampled products times the same factor), as :4004-4063."""
        ds = self.ds
        factor = self.jacobian1 * self.jacobian2 * self.Jy2K ** 2
        dps = _LazyDict()
        if ds._lag_resident is not None and ds._skyvis_lag is None:
            resident, k = ds._lag_resident, self.power_scale()
            dps['skyvis'] = _Deferred(lambda: resident.power(k))
        elif ds.skyvis_lag is not None:
            dps['skyvis'] = NP.abs(ds.skyvis_lag) ** 2 * factor
        if ds.vis_lag is not None:
            dps['vis'] = NP.abs(ds.vis_lag) ** 2 * factor
        if ds.vis_noise_lag is not None:
            dps['noise'] = NP.abs(ds.vis_noise_lag) ** 2 * factor
        if ds.cc_lags is not None:                                                       # :3996-4002
            for key in ('cc_skyvis', 'cc_vis', 'cc_skyvis_res', 'cc_vis_res', 'cc_skyvis_net', 'cc_vis_net'):
                lag = getattr(ds, key + '_lag')
                if lag is not None:
                    dps[key] = NP.abs(lag) ** 2 * factor
        self.dps = dps
        if ds.subband_delay_spectra:                                                     # :4004-4040
            for key in ds.subband_delay_spectra:
                sb = ds.subband_delay_spectra[key]
                out = self.subband_delay_power_spectra[key] = {}
                wl = FCNST.c / sb['freq_center']
                out['z'] = REST_FREQ_HI / sb['freq_center'] - 1
                out['dz'] = REST_FREQ_HI / sb['freq_center'] ** 2 * sb['bw_eff']
                out['kprll'], out['kperp'], out['horizon_kprll_limits'] = self._subband_k(sb['lags'], out['z'])
                out['rz_los'] = self.cosmo.comoving_distance(out['z']).to('Mpc').value
                out['rz_transverse'] = self.comoving_transverse_distance(out['z'], action='return')
                out['drz_los'] = self.comoving_los_depth(sb['bw_eff'], out['z'], action='return')
                omega_bw = self.beam3Dvol(freq_wts=sb['freq_wts'])
                out['jacobian1'] = 1 / omega_bw
                out['jacobian2'] = out['rz_los'] ** 2 * out['drz_los'] / sb['bw_eff']
                out['Jy2K'] = wl ** 2 * JY / (2 * FCNST.k)
                out['factor'] = out['jacobian1'] * out['jacobian2'] * out['Jy2K'] ** 2
                self._subband_power(sb, out, out['factor'].reshape(1, -1, 1, 1))
        if ds.subband_delay_spectra_resampled:                                           # :4042-4063
            for key in ds.subband_delay_spectra_resampled:
                sb = ds.subband_delay_spectra_resampled[key]
                out = self.subband_delay_power_spectra_resampled[key] = {}
                out['kprll'], out['kperp'], out['horizon_kprll_limits'] = self._subband_k(sb['lags'], self.subband_delay_power_spectra[key]['z'])
                self._subband_power(sb, out, self.subband_delay_power_spectra[key]['factor'].reshape(1, -1, 1, 1))

    def compute_power_spectrum_allruns(self, dspec, subband=False):
        """Delay power spectra of stacks of runs on the GPU (:4067-4195, prisim_runs_power): dspec['vislag1'] * dspec['vislag2'].conj()
        * factor, its real part, times 2 for cross power (mode 'cross' iff 'vislag2' is given; auto power reads vislag1 twice without
        copying it), rounded as numpy rounds that statement.  Full band (subband=False): factor = jacobian1 jacobian2 Jy2K**2, key
        'fullband'.  Sub-bands: per window 1 / beam3Dvol(squeeze(freq_wts)) * rz_los**2 drz_los / bw_eff * Jy2K**2 at the redshift of
        each raveled freq_center, key 'subband' (the reference's unused kprll / kperp are not formed).  complex64 spectra are multiplied
        in fp32, as numpy does.
        Departure (one test in tests/test_allruns.py): the reference writes vislag2, freq_center and bw_eff back into the caller's
        dspec; this port leaves dspec as it was."""
        if not isinstance(dspec, dict):
            raise TypeError('Input dspec must be a dictionary')
        mode = 'auto'
        if 'vislag1' not in dspec:
            raise KeyError('Key "vislag1" not found in input dspec')
        v1 = dspec['vislag1']
        if not isinstance(v1, NP.ndarray):
            raise TypeError('Value under key "vislag1" must be a numpy array')
        v2 = None
        if 'vislag2' in dspec:
            mode = 'cross'
            v2 = dspec['vislag2']
            if not isinstance(v2, NP.ndarray):
                raise TypeError('Value under key "vislag2" must be a numpy array')
            if v1.shape != v2.shape:
                raise ValueError('Value under keys "vislag1" and "vislag2" must have same shape')
        if not isinstance(subband, bool):
            raise TypeError('Input subband must be boolean')
        if not subband:
            factor = NP.ravel(self.jacobian1 * self.jacobian2 * self.Jy2K ** 2)
            key = 'fullband'
        else:
            freq_center = NP.asarray(dspec['freq_center']).ravel()
            bw_eff = NP.asarray(dspec['bw_eff']).ravel()
            wl = FCNST.c / freq_center
            redshift = REST_FREQ_HI / freq_center - 1
            rz_los = self.cosmo.comoving_distance(redshift).to('Mpc').value
            drz_los = self.comoving_los_depth(bw_eff, redshift, action='return')
            omega_bw = self.beam3Dvol(freq_wts=NP.squeeze(dspec['freq_wts']))
            jacobian1 = 1 / omega_bw
            jacobian2 = rz_los ** 2 * drz_los / bw_eff
            Jy2K = wl ** 2 * JY / (2 * FCNST.k)
            factor = NP.ravel(jacobian1 * jacobian2 * Jy2K ** 2)
            key = 'subband'
        power, _ = self.ds.ia._ctx.runs_power(v1, v2, factor, cross=(mode == 'cross'))
        return {key: power}

    # ------------------------------------------------------------------------------------------
    # power spectra of closure-phase delay spectra (prisim_closure_power, include/prisim_cpdelay.h)
    CP_KEYS = ('closure_phase_skyvis', 'closure_phase_vis', 'closure_phase_noise')

    def _closure_phase_k(self, cpds):
        """z, kprll (n_win, nlags), kperp (n_win, ntriplets, 3), horizon_kprll_limits (n_acc, n_win, ntriplets, 3, 2) and
        factor = (1 / bw_eff) (drz_los / bw_eff) of a closure-phase delay spectrum dictionary (:4314-4342, :4494-4522)."""
        fc = NP.asarray(cpds['freq_center'])
        bw_eff = NP.asarray(cpds['bw_eff'])
        z = REST_FREQ_HI / fc - 1
        ntrip = len(cpds['antenna_triplets'])
        kprll = NP.empty((fc.size, cpds['lags'].size))
        kperp = NP.empty((fc.size, ntrip, 3))
        horizon_kprll_limits = NP.empty((self.ds.n_acc, fc.size, ntrip, 3, 2))
        bl_lengths = [NP.sqrt(NP.sum(NP.asarray(cpds['baseline_triplets'][i]) ** 2, axis=1)) for i in range(ntrip)]
        for zind, redshift in enumerate(z):
            kprll[zind, :] = self.k_parallel(cpds['lags'], redshift, action='return')
            for ti in range(ntrip):
                kperp[zind, ti, :] = self.k_perp(bl_lengths[ti], redshift, action='return')
                hdl = bl_lengths[ti].reshape(1, -1, 1) / FCNST.c
                hdl = NP.concatenate((hdl, -hdl), axis=2)                                    # (1, 3, 2): upper and lower limit
                horizon_kprll_limits[:, zind, ti, :, :] = self.k_parallel(hdl, redshift, action='return')
        drz_los = self.comoving_los_depth(bw_eff, z, action='return')
        factor = (1 / bw_eff) * (drz_los / bw_eff)                                           # jacobian1 * jacobian2, :4340-4342
        return {'z': z, 'kprll': kprll, 'kperp': kperp, 'horizon_kprll_limits': horizon_kprll_limits}, NP.ravel(factor)

    def compute_individual_closure_phase_power_spectrum(self, closure_phase_delay_spectra):
        """Power spectra of closure-phase delay spectra, triad by triad, on the GPU (:4199-4348, prisim_closure_power):
        abs(spectrum)**2 * factor with factor = drz_los / bw_eff**2 per window.  Takes a dictionary of
        DelaySpectrum.subband_delay_transform_closure_phase; returns z, kprll (n_win, nlags), kperp (n_win, ntriplets, 3),
        horizon_kprll_limits (n_acc, n_win, ntriplets, 3, 2) and the power of every closure_phase_* key present (None stays None).
        Reproduced literally: the factor is reshaped to (1, -1, 1, 1), so the spectra must be 4-D (ntriplets, n_win, nlags, nt) --
        anything else raises ValueError here (the reference broadcasts or fails in numpy).  The caller's dictionary is not modified."""
        cpds = closure_phase_delay_spectra
        out, factor = self._closure_phase_k(cpds)
        todo = [key for key in self.CP_KEYS if key in cpds]
        for key in todo:
            if cpds[key] is not None and (NP.ndim(cpds[key]) != 4 or NP.shape(cpds[key])[1] != factor.size):
                raise ValueError('%s must have shape ntriplets x n_win x nlags x nt' % key)
        for key in todo:
            if cpds[key] is None:
                out[key] = None
            elif NP.size(cpds[key]) == 0:
                out[key] = NP.zeros(NP.shape(cpds[key]))
            else:
                out[key] = self.ds.ia._ctx.closure_power(cpds[key], factor, want=('individual',))['individual']
        return out

    def compute_averaged_closure_phase_power_spectrum(self, closure_phase_delay_spectra):
        """Power spectra of closure-phase delay spectra averaged over axis 0 on the GPU (:4352-4540, prisim_closure_power).  Returns z,
        kprll, kperp, horizon_kprll_limits and {'auto': {key: mean over axis 0 of abs(spectrum)**2, times factor}, 'cross': {key:
        (factor abs(sum over axis 0 of spectrum)**2 - n0 auto) / (n0 (n0 - 1))}}, each (1, ..., n_win, nlags, nt); factor =
        drz_los / bw_eff**2 sits on axis -3 and axis 0 is averaged whatever it holds, as in the reference.  None stays None.
        Departures: one entry on axis 0 raises ValueError before any device work (the reference: ZeroDivisionError in the cross term,
        after the auto term was computed); spectra of fewer than four axes, where axis 0 is the window axis itself, raise ValueError.
        The caller's dictionary is not modified."""
        cpds = closure_phase_delay_spectra
        out, factor = self._closure_phase_k(cpds)
        todo = [key for key in self.CP_KEYS if key in cpds]
        for key in todo:
            if cpds[key] is None:
                continue
            shp = NP.shape(cpds[key])
            if len(shp) < 4 or shp[-3] != factor.size:
                raise ValueError('%s must have shape n0 x ... x n_win x nlags x nt' % key)
            if shp[0] < 2:
                raise ValueError('%s has %d entry on axis 0: the cross power divides by n0 (n0 - 1)' % (key, shp[0]))
        out['auto'], out['cross'] = {}, {}
        for key in todo:
            if cpds[key] is None:
                out['auto'][key] = out['cross'][key] = None
                continue
            x = NP.asarray(cpds[key])
            nmid = int(NP.prod(x.shape[1:-3], dtype=NP.int64))
            r = self.ds.ia._ctx.closure_power(x.reshape(x.shape[0], nmid * factor.size, -1), NP.tile(factor, nmid), want=('auto', 'cross'))
            for mode in ('auto', 'cross'):
                out[mode][key] = r[mode].reshape((1,) + x.shape[1:])
        return out

    def _subband_k(self, lags, zs):
        """kprll (n_win, nlags), kperp (n_win, nbl) and horizon_kprll_limits (n_acc, n_win, nbl, 2) at the redshifts zs (:4011-4018)."""
        kprll = NP.empty((zs.size, lags.size))
        kperp = NP.empty((zs.size, self.bl_length.size))
        horizon_kprll_limits = NP.empty((self.ds.n_acc, zs.size, self.bl_length.size, 2))
        for zind, z in enumerate(zs):
            kprll[zind, :] = self.k_parallel(lags, z, action='return')
            kperp[zind, :] = self.k_perp(self.bl_length, z, action='return')
            horizon_kprll_limits[:, zind, :, :] = self.k_parallel(self.ds.horizon_delay_limits, z, action='return')
        return kprll, kperp, horizon_kprll_limits

    @staticmethod
    def _subband_power(sb, out, conversion_factor):
        """abs(spectrum)**2 * factor of every product the sub-band dictionary holds (:4031-4040); None where the spectrum is None."""
        for name in ('skyvis_lag', 'vis_lag', 'vis_noise_lag', 'skyvis_res_lag', 'vis_res_lag', 'skyvis_net_lag', 'vis_net_lag'):
            if name in sb:
                out[name] = None if sb[name] is None else NP.abs(sb[name]) ** 2 * conversion_factor
