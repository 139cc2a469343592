"""ctypes binding of libprisim_hip.so (include/prisim_hip.h) -- numpy + ctypes only, no torch.

The product path FAILS LOUDLY when the HIP library or a GPU is missing: there is no CPU
fallback anywhere in ``prisim_amd``.
"""
import ctypes as C
import math
import os
import re

import numpy as NP

from . import dsp_readings

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('PRISIM_HIP_LIB') or os.path.join(_HERE, 'lib', 'libprisim_hip.so')      # PRISIM_HIP_LIB: A/B another build of the same ABI
ABI_VERSION = 'prisim_hip 0.5 gfx950'       # prisim_hip_version(): bumped whenever a struct or a signature of include/prisim_hip.h changes

# the enumerators and macros of include/*.h, each under its own name (tests/test_abi_headers.py holds names and values to the headers)
PRISIM_OK = 0
PRISIM_EINVAL, PRISIM_ENODEV, PRISIM_ENOMEM, PRISIM_ESTATE, PRISIM_ELIB, PRISIM_EINTERNAL = -1, -2, -3, -4, -5, -6
PRISIM_FP64, PRISIM_FP32 = 0, 1
PRISIM_KERNEL_AUTO, PRISIM_KERNEL_RECURRENCE, PRISIM_KERNEL_DIRECT = 0, 1, 2
PRISIM_BEAM_DELTA, PRISIM_BEAM_GAUSSIAN, PRISIM_BEAM_AIRY, PRISIM_BEAM_DIPOLE, PRISIM_BEAM_POLY = 0, 1, 2, 3, 4
PRISIM_DIPOLE_GENERAL, PRISIM_DIPOLE_SHORT, PRISIM_DIPOLE_HALFWAVE = 0, 1, 2
PRISIM_COORDS_RADEC, PRISIM_COORDS_HADEC, PRISIM_COORDS_ALTAZ = 0, 1, 2
PRISIM_COORDS = {'radec': PRISIM_COORDS_RADEC, 'hadec': PRISIM_COORDS_HADEC, 'altaz': PRISIM_COORDS_ALTAZ}

# delay CLEAN (include/prisim_clean.h, prisim_amd/csrc_clean/)
PRISIM_CLEAN_MAX_LEN = 4096
PRISIM_CLEAN_THRESHOLD, PRISIM_CLEAN_MAXITER, PRISIM_CLEAN_INRMS, PRISIM_CLEAN_NO_OUTRMS, PRISIM_CLEAN_BAD_THRESHOLD = 1, 2, 4, 8, 16

# sub-band delay spectra (include/prisim_subband.h, prisim_amd/csrc_subband/)
PRISIM_SUBBAND_MAX_LEN = 4096
PRISIM_SUBBAND_OVER, PRISIM_SUBBAND_OVER_POWER, PRISIM_SUBBAND_RES, PRISIM_SUBBAND_RES_POWER = 1, 2, 4, 8
PRISIM_SUBBAND_AUTO, PRISIM_SUBBAND_FUSED, PRISIM_SUBBAND_ROCFFT = -1, 0, 1
SUBBAND_ROUTES = {PRISIM_SUBBAND_FUSED: 'fused', PRISIM_SUBBAND_ROCFFT: 'rocfft'}

# delay spectra and power spectra of runs (include/prisim_runs.h, prisim_amd/csrc_runs/)
PRISIM_RUNS_MAX_LEN = PRISIM_SUBBAND_MAX_LEN
PRISIM_RUNS_ALL, PRISIM_RUNS_INTERP, PRISIM_RUNS_RESAMPLE = 1, 2, 3
PRISIM_RUNS_AUTO, PRISIM_RUNS_FUSED, PRISIM_RUNS_ROCFFT, PRISIM_RUNS_DIRECT = -1, 0, 1, 2
RUNS_ROUTES = {PRISIM_RUNS_FUSED: 'fused', PRISIM_RUNS_ROCFFT: 'rocfft', PRISIM_RUNS_DIRECT: 'direct'}
RUNS_BUDGET = 1 << 30               # device bytes one call of the runs entries streams through by default

# closure phases of antenna triads (include/prisim_closure.h, prisim_amd/csrc_closure/)
PRISIM_CLOSURE_MAX_LEN = PRISIM_SUBBAND_MAX_LEN
PRISIM_CLOSURE_AUTO, PRISIM_CLOSURE_DIRECT, PRISIM_CLOSURE_FUSED, PRISIM_CLOSURE_ROCFFT = -1, 0, 1, 2
CLOSURE_ROUTES = {PRISIM_CLOSURE_DIRECT: 'direct', PRISIM_CLOSURE_FUSED: 'fused', PRISIM_CLOSURE_ROCFFT: 'rocfft'}
CLOSURE_BUDGET = 1 << 30            # device bytes the chunk buffers of one closure-phase call take by default

# delay spectra of closure phases and their power spectra (include/prisim_cpdelay.h, prisim_amd/csrc_closure/cpdelay.hip)
PRISIM_CPDELAY_MAX_LEN = PRISIM_SUBBAND_MAX_LEN
PRISIM_CPDELAY_OVER, PRISIM_CPDELAY_OVER_POWER, PRISIM_CPDELAY_RES, PRISIM_CPDELAY_RES_POWER = 1, 2, 4, 8
PRISIM_CPDELAY_AUTO, PRISIM_CPDELAY_FUSED, PRISIM_CPDELAY_ROCFFT = -1, 0, 1
CPDELAY_ROUTES = {PRISIM_CPDELAY_FUSED: 'fused', PRISIM_CPDELAY_ROCFFT: 'rocfft'}
PRISIM_CPPOWER_INDIVIDUAL, PRISIM_CPPOWER_AUTO, PRISIM_CPPOWER_CROSS = 1, 2, 4

# day and LST binning of closure phases (include/prisim_cpbins.h, prisim_amd/csrc_closure/cpbins.hip)
PRISIM_CPBINS_MAX_BIN = 256
PRISIM_CPBINS_PHASE_FLAGS, PRISIM_CPBINS_BINNED = 0, 1
PRISIM_CPBINS_WTS, PRISIM_CPBINS_EICP_MEAN, PRISIM_CPBINS_EICP_MEDIAN, PRISIM_CPBINS_CP_MEAN = 1, 2, 4, 8
PRISIM_CPBINS_CP_MEDIAN, PRISIM_CPBINS_RMS, PRISIM_CPBINS_MAD, PRISIM_CPBINS_ALL = 16, 32, 64, 127
CPBINS_WANT = {'wts': PRISIM_CPBINS_WTS, 'eicp_mean': PRISIM_CPBINS_EICP_MEAN, 'eicp_median': PRISIM_CPBINS_EICP_MEDIAN,
               'cp_mean': PRISIM_CPBINS_CP_MEAN, 'cp_median': PRISIM_CPBINS_CP_MEDIAN, 'rms': PRISIM_CPBINS_RMS, 'mad': PRISIM_CPBINS_MAD}

# differences of day sub-samples of binned closure phases (include/prisim_cpdiff.h, prisim_amd/csrc_closure/cpdiff.hip)
CPDIFF_OUTPUTS = ('diff0_mean', 'diff0_median', 'diff1_mean', 'diff1_median', 'wts0', 'wts1', 'mask0', 'mask1')
PRISIM_CPDIFF_OUT_BYTES = 82

# delay spectra of binned closure phasors (include/prisim_cpft.h, prisim_amd/csrc_closure/cpft.hip)
PRISIM_CPFT_MAX_LEN, PRISIM_CPFT_MAX_IN = PRISIM_SUBBAND_MAX_LEN, 8
PRISIM_CPFT_OVER, PRISIM_CPFT_RES, PRISIM_CPFT_LAG = 1, 2, 4
PRISIM_CPFT_AUTO, PRISIM_CPFT_FUSED, PRISIM_CPFT_ROCFFT = -1, 0, 1
CPFT_ROUTES = {PRISIM_CPFT_FUSED: 'fused', PRISIM_CPFT_ROCFFT: 'rocfft'}

# cross power of closure-phase delay spectra (include/prisim_cpxps.h, prisim_amd/csrc_closure/cpxps.hip)
PRISIM_CPXPS_MAX_MEDIAN = 256
PRISIM_CPXPS_NONE, PRISIM_CPXPS_FULL, PRISIM_CPXPS_COLLAPSE = 0, 1, 2
PRISIM_CPXPS_MEAN, PRISIM_CPXPS_MEDIAN = 0, 1
CPXPS_MODES = {'none': PRISIM_CPXPS_NONE, 'full': PRISIM_CPXPS_FULL, 'collapse': PRISIM_CPXPS_COLLAPSE}
CPXPS_STATS = {'mean': PRISIM_CPXPS_MEAN, 'median': PRISIM_CPXPS_MEDIAN}

# incoherent averages of closure-phase power spectra (include/prisim_cpavg.h, prisim_amd/csrc_closure/cpavg.hip)
PRISIM_CPAVG_MIN_DIM, PRISIM_CPAVG_MAX_DIM = 5, 8
PRISIM_CPAVG_AUTO, PRISIM_CPAVG_LDS, PRISIM_CPAVG_GLOBAL = -1, 0, 1
CPAVG_ROUTES = {PRISIM_CPAVG_LDS: 'lds', PRISIM_CPAVG_GLOBAL: 'global'}

# closure phases of noise realisations (include/prisim_cpreal.h, prisim_amd/csrc_closure/cpreal.hip)
PRISIM_CPREAL_AUTO, PRISIM_CPREAL_DIRECT, PRISIM_CPREAL_STAGED = -1, 0, 1
PRISIM_CPREAL_NOISY, PRISIM_CPREAL_NOISE = 0, 1
CPREAL_ROUTES = {PRISIM_CPREAL_DIRECT: 'direct', PRISIM_CPREAL_STAGED: 'staged'}
CPREAL_KINDS = {'noisy': PRISIM_CPREAL_NOISY, 'noise': PRISIM_CPREAL_NOISE}

# dirty images and synthesized beams by the direct Fourier sum (include/prisim_imaging.h, prisim_amd/csrc_imaging/imaging.hip)
PRISIM_IMAGE_DIRTY, PRISIM_IMAGE_PSF = 0, 1
PRISIM_IMAGE_AUTO, PRISIM_IMAGE_DIRECT, PRISIM_IMAGE_STEPPED = -1, 0, 1
PRISIM_IMAGE_W_NONE, PRISIM_IMAGE_W_BASELINE, PRISIM_IMAGE_W_FULL = 0, 1, 2
IMAGING_ROUTES = {PRISIM_IMAGE_DIRECT: 'direct', PRISIM_IMAGE_STEPPED: 'stepped'}
IMAGING_KINDS = {'dirty': PRISIM_IMAGE_DIRTY, 'psf': PRISIM_IMAGE_PSF}
# ... and their fp32 route (include/prisim_imaging32.h, prisim_amd/csrc_imaging/imaging32.hip): the entry of each precision
IMAGING_PRECISIONS = {'double': 'prisim_dirty_image', 'single': 'prisim_dirty_image_f32'}
# ... and the two entries of the beam-weighted mosaic (include/prisim_mosaic.h, include/prisim_mosaic32.h)
MOSAIC_PRECISIONS = {'double': 'prisim_mosaic_image', 'single': 'prisim_mosaic_image_f32'}

# Hogbom CLEAN of dirty images with the exact beam (include/prisim_imclean.h, prisim_amd/csrc_imaging/imclean.hip)
PRISIM_IMCLEAN_THRESHOLD, PRISIM_IMCLEAN_MAXITER, PRISIM_IMCLEAN_DEAD = 1, 2, 4
PRISIM_IMCLEAN_POLL_DEFAULT, PRISIM_IMCLEAN_POLL_MAX = 32, 1024

# Cotton-Schwab CLEAN of dirty images (include/prisim_csclean.h, prisim_amd/csrc_imaging/csclean.hip)
PRISIM_CSCLEAN_MAJOR, PRISIM_CSCLEAN_DIVERGED = 8, 16
PRISIM_CSCLEAN_AUTO, PRISIM_CSCLEAN_LDS, PRISIM_CSCLEAN_GLOBAL = -1, 0, 1
PRISIM_CSCLEAN_MAX_MAJOR = 65536
CSCLEAN_ROUTES = {PRISIM_CSCLEAN_LDS: 'lds', PRISIM_CSCLEAN_GLOBAL: 'global'}

# instrument gain tables (include/prisim_gains.h, prisim_amd/csrc_gains/)
PRISIM_GAINS_MAX_DEGREE = 5
PRISIM_GAINS_ANTENNA, PRISIM_GAINS_BASELINE = 0, 1


class PrisimSky(C.Structure):
    _fields_ = [('nsrc', C.c_int64), ('dircos', C.c_void_p), ('pbflux', C.c_void_p),
                ('pbflux_is_f32', C.c_int32), ('pc_dircos', C.c_void_p), ('fwhm_deg', C.c_void_p), ('fluxes', C.c_void_p)]


class PrisimBeamExt(C.Structure):
    _fields_ = [('dipole_dircos', C.c_double * 3), ('dipole_mode', C.c_int32), ('array_nax1', C.c_int32),
                ('array_nax2', C.c_int32), ('ground_modify', C.c_int32), ('array_sep1', C.c_double), ('array_sep2', C.c_double),
                ('array_east2ax1_deg', C.c_double), ('array_pc_dircos', C.c_double * 3), ('ground_height', C.c_double),
                ('ground_scale', C.c_double), ('ground_max', C.c_double), ('bf_nelem', C.c_int32), ('bf_nrand', C.c_int32),
                ('bf_pos', C.c_void_p), ('bf_delays', C.c_void_p), ('bf_gains', C.c_void_p), ('poly_coef', C.c_double * 4)]


def make_beam_ext(ext):
    """dict -> PrisimBeamExt.  Keys: dipole_dircos, dipole_mode, array (dict nax1, nax2, sep1, sep2, east2ax1, pointing_dircos),
    ground (dict height, modifier{scale,max}), beamformer (dict positions [n,3], delays [n] or [n,nrand], gains likewise).
    The returned struct keeps the beamformer arrays alive (attribute _keep)."""
    if ext is None:
        return None
    x = PrisimBeamExt()
    dd = NP.asarray(ext.get('dipole_dircos', (1.0, 0.0, 0.0)), dtype=NP.float64).ravel()
    if dd.size != 3:
        raise ValueError('dipole_dircos must have 3 elements')
    x.dipole_dircos[:] = dd.tolist()
    x.dipole_mode = int(ext.get('dipole_mode', PRISIM_DIPOLE_GENERAL))
    arr = ext.get('array', None)
    if arr is not None:
        x.array_nax1, x.array_nax2 = int(arr['nax1']), int(arr['nax2'])
        x.array_sep1, x.array_sep2 = float(arr['sep1']), float(arr['sep2'])
        x.array_east2ax1_deg = float(arr.get('east2ax1', 0.0) or 0.0)
        pc = NP.asarray(arr.get('pointing_dircos', (0.0, 0.0, 1.0)), dtype=NP.float64).ravel()
        if pc.size != 3:
            raise ValueError('array pointing_dircos must have 3 elements')
        x.array_pc_dircos[:] = pc.tolist()
    gnd = ext.get('ground', None)
    if gnd is not None:
        x.ground_height = float(gnd['height'])
        mod = gnd.get('modifier', None)
        if isinstance(mod, dict):
            x.ground_modify = 1
            if 'scale' in mod:
                x.ground_modify |= 2
                x.ground_scale = float(mod['scale'])
            if 'max' in mod:
                x.ground_modify |= 4
                x.ground_max = float(mod['max'])
    bf = ext.get('beamformer', None)
    if bf is not None:
        pos = NP.ascontiguousarray(bf['positions'], dtype=NP.float64)
        if pos.ndim != 2 or pos.shape[1] != 3:
            raise ValueError('beamformer positions must have shape (nelem, 3)')
        nel = pos.shape[0]
        delays = NP.asarray(bf.get('delays', NP.zeros(nel)), dtype=NP.float64).reshape(nel, -1)
        gains = NP.asarray(bf.get('gains', NP.ones(nel)), dtype=NP.float64).reshape(nel, -1)
        nrand = max(delays.shape[1], gains.shape[1])
        delays = NP.ascontiguousarray(NP.broadcast_to(delays, (nel, nrand)))
        gains = NP.ascontiguousarray(NP.broadcast_to(gains, (nel, nrand)))
        x.bf_nelem, x.bf_nrand = nel, nrand
        x.bf_pos, x.bf_delays, x.bf_gains = pos.ctypes.data, delays.ctypes.data, gains.ctypes.data
        x._keep = (pos, delays, gains)
    poly = ext.get('poly', None)
    if poly is not None:
        c = NP.zeros(4)
        pc = NP.asarray(poly, dtype=NP.float64).ravel()
        if pc.size < 1 or pc.size > 4:
            raise ValueError('poly must have 1 to 4 coefficients')
        c[:pc.size] = pc
        x.poly_coef[:] = c.tolist()
    return x


class PrisimBeamSky(C.Structure):
    _fields_ = [('nsrc', C.c_int64), ('dircos', C.c_void_p), ('flux_ref', C.c_void_p), ('spindex', C.c_void_p),
                ('flux_spectrum', C.c_void_p), ('ref_freq_hz', C.c_double), ('beam_kind', C.c_int32), ('diameter_m', C.c_double),
                ('beam_pc_dircos', C.c_void_p), ('pc_dircos', C.c_void_p), ('fwhm_deg', C.c_void_p), ('ext', C.c_void_p)]


class PrisimCatalog(C.Structure):
    _fields_ = [('nsrc', C.c_int64), ('coords', C.c_int32), ('reserved_', C.c_int32), ('location', C.c_void_p), ('flux_ref', C.c_void_p),
                ('spindex', C.c_void_p), ('ref_freq_hz', C.c_double), ('flux_spectrum', C.c_void_p), ('fwhm_deg', C.c_void_p),
                ('unitvec', C.c_void_p)]


class PrisimObs(C.Structure):
    _fields_ = [('latitude_deg', C.c_double), ('roi_radius_deg', C.c_double), ('roi_center', C.c_int32), ('use_external_beam', C.c_int32),
                ('beam_kind', C.c_int32), ('reserved_', C.c_int32), ('diameter_m', C.c_double), ('ext', C.c_void_p)]


class PrisimSnapshot(C.Structure):
    _fields_ = [('lst_deg', C.c_double), ('pc_dircos', C.c_double * 3), ('beam_pc_dircos', C.c_double * 3), ('frame_given', C.c_int32),
                ('reserved_', C.c_int32), ('cel2enu', C.c_double * 9), ('aberr_beta', C.c_double * 3)]


class PrisimPost(C.Structure):
    _fields_ = [('host_vis', C.c_void_p), ('host_is_c64', C.c_int32), ('gather', C.c_int32), ('gather_as_c64', C.c_int32), ('reserved_', C.c_int32)]


class PrisimTiming(C.Structure):
    _fields_ = [('last_kernel_ms', C.c_double), ('last_compute_ms', C.c_double), ('sum_kernel_ms', C.c_double),
                ('n_kernel', C.c_int64), ('last_terms', C.c_int64), ('last_kernel_id', C.c_int32),
                ('last_chan_tile', C.c_int32), ('last_nsplit', C.c_int32), ('last_lift_groups', C.c_int32),
                ('last_taper_group', C.c_int32), ('last_delay_fused', C.c_int32), ('last_delay_ms', C.c_double),
                ('last_taper_split', C.c_int32), ('last_split_uncorrected_groups', C.c_int32), ('last_culled_fraction', C.c_double),
                ('last_batch_snapshots', C.c_int32), ('reserved_', C.c_int32)]


class PrisimCommStats(C.Structure):
    _fields_ = [('n_gathers', C.c_int64), ('bytes_per_peer', C.c_int64), ('sum_gather_ms', C.c_double), ('last_gather_ms', C.c_double),
                ('max_gather_ms', C.c_double), ('last_gather_after_compute_ms', C.c_double), ('stream_priority', C.c_int32),
                ('stream_priority_lowest', C.c_int32), ('nranks', C.c_int32), ('reserved_', C.c_int32), ('sum_undeal_ms', C.c_double),
                ('last_undeal_ms', C.c_double)]


class PrisimCleanStats(C.Structure):
    _fields_ = [('device_ms', C.c_double), ('clean_ms', C.c_double), ('sum_iter', C.c_int64), ('rows', C.c_int64),
                ('waves_per_block', C.c_int32), ('kernel_in_lds', C.c_int32), ('lds_bytes', C.c_int64)]


class PrisimSubbandStats(C.Structure):
    _fields_ = [('device_ms', C.c_double), ('kernel_ms', C.c_double), ('rows', C.c_int64), ('route', C.c_int32),
                ('lds_bytes', C.c_int32)]


class PrisimRunsStats(C.Structure):
    _fields_ = [('wall_ms', C.c_double), ('pairs', C.c_int64), ('chunks', C.c_int64), ('chunk_pairs', C.c_int64), ('route', C.c_int32),
                ('streams', C.c_int32), ('tile', C.c_int32), ('lds_bytes', C.c_int32)]


class PrisimClosureStats(C.Structure):
    _fields_ = [('wall_ms', C.c_double), ('kernel_ms', C.c_double), ('triads', C.c_int64), ('chunks', C.c_int64),
                ('chunk_triads', C.c_int64), ('kernel_bytes', C.c_int64), ('download_bytes', C.c_int64), ('route', C.c_int32),
                ('streams', C.c_int32), ('tile', C.c_int32), ('lds_bytes', C.c_int32)]


class PrisimCpdelayStats(C.Structure):
    _fields_ = [('wall_ms', C.c_double), ('kernel_ms', C.c_double), ('rows', C.c_int64), ('chunks', C.c_int64), ('chunk_rows', C.c_int64),
                ('upload_bytes', C.c_int64), ('download_bytes', C.c_int64), ('route', C.c_int32), ('phase_route', C.c_int32),
                ('streams', C.c_int32), ('tile', C.c_int32), ('lds_bytes', C.c_int32), ('reserved_', C.c_int32)]


class PrisimCpbinsStats(C.Structure):
    _fields_ = [('wall_ms', C.c_double), ('kernel_ms', C.c_double), ('elements', C.c_int64), ('chunks', C.c_int64),
                ('chunk_triads', C.c_int64), ('kernel_bytes', C.c_int64), ('upload_bytes', C.c_int64), ('download_bytes', C.c_int64),
                ('max_bin', C.c_int32), ('resident_in', C.c_int32)]


class PrisimCpdiffStats(C.Structure):
    _fields_ = [('wall_ms', C.c_double), ('kernel_ms', C.c_double), ('elements', C.c_int64), ('chunks', C.c_int64),
                ('chunk_triads', C.c_int64), ('kernel_bytes', C.c_int64), ('upload_bytes', C.c_int64), ('download_bytes', C.c_int64),
                ('resident_in', C.c_int32), ('ncomb', C.c_int32)]


class PrisimCpftStats(C.Structure):
    _fields_ = [('wall_ms', C.c_double), ('kernel_ms', C.c_double), ('rows', C.c_int64), ('chunks', C.c_int64), ('chunk_rows', C.c_int64),
                ('row_bytes', C.c_int64), ('kernel_bytes', C.c_int64), ('upload_bytes', C.c_int64), ('download_bytes', C.c_int64),
                ('route', C.c_int32), ('streams', C.c_int32), ('group_rows', C.c_int32), ('lds_bytes', C.c_int32)]


class _PrisimCpxpsStats(C.Structure):
    """prisim_cpxps_stats, public as Context.PrisimCpxpsStats: tests/test_abi_helpers.py pins the Prisim*Stats names of this module's
    namespace; like every mirror it is listed in STRUCTS, which tests/test_abi_headers.py holds to the headers."""
    _fields_ = [('wall_ms', C.c_double), ('kernel_ms', C.c_double), ('chunks', C.c_int64), ('chunk_lags', C.c_int64),
                ('kernel_bytes', C.c_int64), ('upload_bytes', C.c_int64), ('download_bytes', C.c_int64), ('cross_bytes', C.c_int64)]


class _PrisimCpavgStats(C.Structure):
    """prisim_cpavg_stats of both entries of include/prisim_cpavg.h, public as Context.PrisimCpavgStats (see _PrisimCpxpsStats)."""
    _fields_ = [('wall_ms', C.c_double), ('kernel_ms', C.c_double), ('chunks', C.c_int64), ('kernel_bytes', C.c_int64),
                ('upload_bytes', C.c_int64), ('download_bytes', C.c_int64), ('route', C.c_int32), ('lds_limit', C.c_int32)]


class _PrisimCprealStats(C.Structure):
    """prisim_cpreal_stats of include/prisim_cpreal.h, public as Context.PrisimCprealStats (see _PrisimCpxpsStats)."""
    _fields_ = [('wall_ms', C.c_double), ('kernel_ms', C.c_double), ('pairs', C.c_int64), ('chunks', C.c_int64),
                ('chunk_pairs', C.c_int64), ('draws', C.c_int64), ('kernel_bytes', C.c_int64), ('download_bytes', C.c_int64),
                ('route', C.c_int32), ('streams', C.c_int32), ('chan_tile', C.c_int32), ('lds_bytes', C.c_int32)]


class _PrisimAntpowerStats(C.Structure):
    """prisim_antpower_stats of include/prisim_antpower.h, public as Context.PrisimAntpowerStats (see _PrisimCpxpsStats)."""
    _fields_ = [('wall_ms', C.c_double), ('kernel_ms', C.c_double), ('sources_evaluated', C.c_int64), ('sources_up', C.c_int64),
                ('spans', C.c_int64), ('span_sources', C.c_int64), ('block_sources', C.c_int64), ('kernel_bytes', C.c_int64),
                ('upload_bytes', C.c_int64), ('download_bytes', C.c_int64), ('streams', C.c_int32), ('chan_tile', C.c_int32),
                ('lds_bytes', C.c_int32), ('reserved_', C.c_int32)]


class _PrisimAntpowerArgs(C.Structure):
    """prisim_antpower_args of include/prisim_antpower.h, public as Context.PrisimAntpowerArgs."""
    _fields_ = [('nsrc', C.c_int64), ('nchan', C.c_int64), ('nsnap', C.c_int64), ('unitvec', C.c_void_p), ('flux_ref', C.c_void_p),
                ('spindex', C.c_void_p), ('ref_freq_hz', C.c_double), ('flux_spectrum', C.c_void_p), ('freqs_hz', C.c_void_p),
                ('cel2enu', C.c_void_p), ('aberr_beta', C.c_void_p), ('beam_kind', C.c_int32), ('reserved_', C.c_int32),
                ('diameter_m', C.c_double), ('beam_pc_dircos', C.c_double * 3), ('ext', C.c_void_p), ('n_ext', C.c_int64),
                ('budget_bytes', C.c_int64)]


class _PrisimImagingStats(C.Structure):
    """prisim_imaging_stats of include/prisim_imaging.h, public as Context.PrisimImagingStats (see _PrisimCpxpsStats)."""
    _fields_ = [('wall_ms', C.c_double), ('kernel_ms', C.c_double), ('terms', C.c_int64), ('chunks', C.c_int64), ('chunk_pixels', C.c_int64),
                ('kernel_bytes', C.c_int64), ('upload_bytes', C.c_int64), ('download_bytes', C.c_int64), ('route', C.c_int32),
                ('streams', C.c_int32), ('chan_tile', C.c_int32), ('reseed', C.c_int32), ('lds_bytes', C.c_int32), ('block_pixels', C.c_int32)]


class _PrisimImagingArgs(C.Structure):
    """prisim_imaging_args of include/prisim_imaging.h, public as Context.PrisimImagingArgs."""
    _fields_ = [('npix', C.c_int64), ('nbl', C.c_int64), ('nchan', C.c_int64), ('nt', C.c_int64), ('unitvec', C.c_void_p), ('rot', C.c_void_p),
                ('aberr_beta', C.c_void_p), ('pc_dircos', C.c_void_p), ('baselines', C.c_void_p), ('freqs_hz', C.c_void_p), ('cube', C.c_void_p),
                ('weights', C.c_void_p), ('kind', C.c_int32), ('weight_form', C.c_int32), ('chan_avg', C.c_int32), ('route', C.c_int32),
                ('budget_bytes', C.c_int64)]


class _PrisimImcleanStats(C.Structure):
    """prisim_imclean_stats of include/prisim_imclean.h, public as Context.PrisimImcleanStats (see _PrisimCpxpsStats)."""
    _fields_ = [('wall_ms', C.c_double), ('kernel_ms', C.c_double), ('dirty_ms', C.c_double), ('peak_ms', C.c_double),
                ('update_ms', C.c_double), ('restore_ms', C.c_double), ('terms', C.c_int64), ('iterations', C.c_int64),
                ('components', C.c_int64), ('polls', C.c_int64), ('chunks', C.c_int64), ('chunk_pixels', C.c_int64),
                ('kernel_bytes', C.c_int64), ('upload_bytes', C.c_int64), ('download_bytes', C.c_int64), ('device_bytes', C.c_int64),
                ('route', C.c_int32), ('streams', C.c_int32), ('chan_tile', C.c_int32), ('reseed', C.c_int32), ('lds_bytes', C.c_int32),
                ('block_pixels', C.c_int32)]


class _PrisimImcleanArgs(C.Structure):
    """prisim_imclean_args of include/prisim_imclean.h, public as Context.PrisimImcleanArgs."""
    _fields_ = [('npix', C.c_int64), ('nbl', C.c_int64), ('nchan', C.c_int64), ('nt', C.c_int64), ('unitvec', C.c_void_p), ('rot', C.c_void_p),
                ('aberr_beta', C.c_void_p), ('pc_dircos', C.c_void_p), ('baselines', C.c_void_p), ('freqs_hz', C.c_void_p), ('cube', C.c_void_p),
                ('weights', C.c_void_p), ('window', C.c_void_p), ('fwhm_rad', C.c_void_p), ('gain', C.c_double), ('threshold', C.c_double),
                ('maxiter', C.c_int64), ('budget_bytes', C.c_int64), ('weight_form', C.c_int32), ('chan_avg', C.c_int32), ('route', C.c_int32),
                ('threshold_relative', C.c_int32), ('poll_every', C.c_int32), ('reserved_', C.c_int32)]


class _PrisimCscleanStats(C.Structure):
    """prisim_csclean_stats of include/prisim_csclean.h, public as Context.PrisimCscleanStats (see _PrisimCpxpsStats)."""
    _fields_ = [('wall_ms', C.c_double), ('kernel_ms', C.c_double), ('psf_ms', C.c_double), ('dirty_ms', C.c_double), ('peak_ms', C.c_double),
                ('minor_ms', C.c_double), ('model_ms', C.c_double), ('restore_ms', C.c_double), ('terms', C.c_int64), ('cycles', C.c_int64),
                ('components', C.c_int64), ('polls', C.c_int64), ('psf_offsets', C.c_int64), ('upload_bytes', C.c_int64),
                ('download_bytes', C.c_int64), ('device_bytes', C.c_int64), ('route', C.c_int32), ('minor_route', C.c_int32),
                ('streams', C.c_int32), ('chan_tile', C.c_int32), ('reseed', C.c_int32), ('lds_bytes', C.c_int32),
                ('minor_lds_bytes', C.c_int32), ('block_pixels', C.c_int32)]


class _PrisimCscleanArgs(C.Structure):
    """prisim_csclean_args of include/prisim_csclean.h, public as Context.PrisimCscleanArgs: the fields of prisim_imclean_args less its
    polling, then those of the cycles."""
    _fields_ = [f for f in _PrisimImcleanArgs._fields_ if f[0] not in ('poll_every', 'reserved_')] + [
        ('ny', C.c_int64), ('nx', C.c_int64), ('cycle_depth', C.c_double), ('cycle_niter', C.c_int64), ('max_major', C.c_int32),
        ('minor_route', C.c_int32)]


class _PrisimMosaicStats(C.Structure):
    """prisim_mosaic_stats of include/prisim_mosaic.h, public as Context.PrisimMosaicStats (see _PrisimCpxpsStats)."""
    _fields_ = [('wall_ms', C.c_double), ('kernel_ms', C.c_double), ('terms', C.c_int64), ('beam_values', C.c_int64), ('chunks', C.c_int64),
                ('chunk_pixels', C.c_int64), ('pixel_bytes', C.c_int64), ('kernel_bytes', C.c_int64), ('upload_bytes', C.c_int64),
                ('download_bytes', C.c_int64), ('route', C.c_int32), ('streams', C.c_int32), ('chan_tile', C.c_int32), ('reseed', C.c_int32),
                ('lds_bytes', C.c_int32), ('block_pixels', C.c_int32)]


class _PrisimMosaicArgs(C.Structure):
    """prisim_mosaic_args of include/prisim_mosaic.h, public as Context.PrisimMosaicArgs."""
    _fields_ = [('npix', C.c_int64), ('nbl', C.c_int64), ('nchan', C.c_int64), ('nt', C.c_int64), ('unitvec', C.c_void_p), ('rot', C.c_void_p),
                ('aberr_beta', C.c_void_p), ('pc_dircos', C.c_void_p), ('baselines', C.c_void_p), ('freqs_hz', C.c_void_p), ('cube', C.c_void_p),
                ('weights', C.c_void_p), ('weight_form', C.c_int32), ('chan_avg', C.c_int32), ('route', C.c_int32), ('beam_kind', C.c_int32),
                ('diameter_m', C.c_double), ('beam_pc_dircos', C.c_double * 3), ('beam_pc_snap', C.c_void_p), ('ext', C.c_void_p),
                ('n_ext', C.c_int64), ('pbmin', C.c_double), ('budget_bytes', C.c_int64)]


class _PrisimMoscleanStats(C.Structure):
    """prisim_mosclean_stats of include/prisim_mosclean.h, public as Context.PrisimMoscleanStats (see _PrisimCpxpsStats)."""
    _fields_ = [('wall_ms', C.c_double), ('kernel_ms', C.c_double), ('mosaic_ms', C.c_double), ('peak_ms', C.c_double),
                ('update_ms', C.c_double), ('restore_ms', C.c_double), ('terms', C.c_int64), ('beam_values', C.c_int64),
                ('iterations', C.c_int64), ('components', C.c_int64), ('polls', C.c_int64), ('chunks', C.c_int64),
                ('chunk_pixels', C.c_int64), ('kernel_bytes', C.c_int64), ('upload_bytes', C.c_int64), ('download_bytes', C.c_int64),
                ('device_bytes', C.c_int64), ('route', C.c_int32), ('streams', C.c_int32), ('chan_tile', C.c_int32), ('reseed', C.c_int32),
                ('lds_bytes', C.c_int32), ('block_pixels', C.c_int32)]


class _PrisimMoscleanArgs(C.Structure):
    """prisim_mosclean_args of include/prisim_mosclean.h, public as Context.PrisimMoscleanArgs: the fields of prisim_mosaic_args in their
    order, then those of the CLEAN."""
    _fields_ = _PrisimMosaicArgs._fields_ + [('gain', C.c_double), ('maxiter', C.c_int64), ('threshold', C.c_double),
                                             ('threshold_relative', C.c_int32), ('window', C.c_void_p), ('fwhm_rad', C.c_void_p),
                                             ('poll_every', C.c_int32)]


class _PrisimMoscsStats(C.Structure):
    """prisim_moscs_stats of include/prisim_moscs.h, public as Context.PrisimMoscsStats (see _PrisimCpxpsStats): prisim_csclean_stats
    with mosaic_ms for dirty_ms, then beam_ms."""
    _fields_ = [(('mosaic_ms' if n == 'dirty_ms' else n), t) for n, t in _PrisimCscleanStats._fields_] + [('beam_ms', C.c_double)]


class _PrisimMoscsArgs(C.Structure):
    """prisim_moscs_args of include/prisim_moscs.h, public as Context.PrisimMoscsArgs: the fields of prisim_mosclean_args less its
    polling, then those of the cycles."""
    _fields_ = [f for f in _PrisimMoscleanArgs._fields_ if f[0] != 'poll_every'] + [
        ('ny', C.c_int64), ('nx', C.c_int64), ('cycle_depth', C.c_double), ('cycle_niter', C.c_int64), ('max_major', C.c_int32),
        ('minor_route', C.c_int32)]


def numpy_fuses_complex_product(dtype):
    """Whether numpy rounds the real part of a * conj(b) as fma(ar, br, ai bi) (its SIMD complex loop on FMA hardware) rather than
    ar br + ai bi, for complex128 or complex64: probed on a product whose two readings differ (ar br is a tie -- (1 + 2^-26)(1 + 2^-27)
    in fp64, (1 + 2^-12)^2 in fp32 -- that the tiny ai bi breaks only when the sum is fused)."""
    dtype = NP.dtype(dtype)
    e1, e2, g = (2.0 ** -26, 2.0 ** -27, 2.0 ** -60) if dtype == NP.complex128 else (2.0 ** -12, 2.0 ** -12, 2.0 ** -30)
    a = NP.full(64, complex(1.0 + e1, g), dtype=dtype)
    b = NP.full(64, complex(1.0 + e2, g), dtype=dtype)
    return bool(NP.all((a * b.conj()).real != (a.real * b.real + a.imag * b.imag)))


class PrisimGainsStats(C.Structure):
    _fields_ = [('device_ms', C.c_double), ('kernel_ms', C.c_double), ('elements', C.c_int64)]


def _stats_dict(st, rename=None, **maps):
    """A stats struct as a dict of its fields without reserved_, each value as ctypes hands it over: a Python int for the integer
    fields, a float for the doubles (tests/test_abi_helpers.py pins the type per key).  maps: per field, a table of names (a value it
    lacks stays as it is) or a function of the value; rename: the keys that differ from the field names ('resident_in')."""
    out = {}
    for name, _ in st._fields_:
        if name == 'reserved_':
            continue
        v, f = getattr(st, name), maps.get(name)
        if f is not None:
            v = f.get(v, v) if isinstance(f, dict) else f(v)
        out[(rename or {}).get(name, name)] = v
    return out


def delay_nout(nchan, pad):
    """Lags per row of the delay transform of nchan channels padded by the fraction pad: the library's rule, delay_geom in
    csrc/capi.cpp (stated for callers in include/prisim_hip.h), restated so that the host sizes its arrays as the library fills them:
    change both together, tests/test_gpu_delay_sweeps.py holds one against the other.  It is the exact count of positions
    j (1 + pad) < nfft, j >= 0.  len(arange(0, nfft, 1 + pad)) is NOT: where nfft / (1 + pad) rounds up past an integer (1400 / 1.4 =
    1000.0000000000001) arange has one position more, and that position is nfft itself."""
    pad = max(float(pad), 0.0)
    nchan = int(nchan)
    npad = int(nchan * pad)
    nfft = nchan + npad
    return int(math.ceil(nfft / (1.0 + pad) - 1e-12))


def _resample_map(wanted, m, nout):
    """(nmap, map_out, map_in, map_w) of dsp_readings.resample_map(m, nout), the one reading of the resampling, as the library takes
    them; (0, None, None, None) when not wanted (no resampled output, or lengths that the library is left to refuse)."""
    if not wanted:
        return 0, None, None, None
    mo, mi, mw = (NP.ascontiguousarray(a) for a in dsp_readings.resample_map(m, nout))
    return mo.size, mo, mi, mw


def _closure_inputs(legs, conj, bpwts, freq_wts, masks, mask_index, nbl, nchan, nt):
    """The closure-phase inputs as the library takes them, C-contiguous: legs, conj (ntriads, 3) int32; bpwts (nbl, nchan, nt), freq_wts
    (nchan,) (None: ones), masks (nmask, nchan) or None: float64; mask_index (nbl,) int32 or None."""
    lg = NP.ascontiguousarray(legs, dtype=NP.int32).reshape(-1, 3)
    cj = NP.ascontiguousarray(conj, dtype=NP.int32).reshape(-1, 3)
    if cj.shape != lg.shape:
        raise ValueError('legs and conj must both be (ntriads, 3)')
    bw = NP.ascontiguousarray(NP.broadcast_to(NP.asarray(bpwts, dtype=NP.float64), (nbl, nchan, nt)))
    fw = NP.ones(nchan) if freq_wts is None else NP.ascontiguousarray(NP.broadcast_to(NP.asarray(freq_wts, dtype=NP.float64).ravel(), (nchan,)))
    mk = mi = None
    if masks is not None:
        mk = NP.ascontiguousarray(masks, dtype=NP.float64).reshape(-1, nchan)
        if mask_index is not None:
            mi = NP.ascontiguousarray(mask_index, dtype=NP.int32).ravel()
            if mi.size != nbl:
                raise ValueError('mask_index must have one entry per cube row')
    return lg, cj, bw, fw, mk, mi


def _imaging_inputs(a, unitvec, rot, pc_dircos, baselines, freqs_hz, cube, weights, chan_avg, aberr_beta, route, budget_bytes):
    """The inputs dirty_image, mosaic_image and clean_image take alike, checked and put into the fields that their argument structs
    have under the same names: unitvec (npix, 3), rot (nt, 3, 3), pc_dircos (nt, 3), baselines (nbl, 3), freqs_hz (nchan,), aberr_beta
    (nt, 3) or None: float64; cube (nt, nbl, nchan) complex128 or None; weights None, (nbl,) or (nt, nbl, nchan), which decides
    weight_form; chan_avg, route and budget_bytes.  Returns (npix, nbl, nchan, nt, resident, keep): resident, the cube is None; keep,
    the arrays the struct points into, to be held until the call is over."""
    uv = NP.ascontiguousarray(unitvec, dtype=NP.float64).reshape(-1, 3)
    rt = NP.ascontiguousarray(rot, dtype=NP.float64).reshape(-1, 9)
    pc = NP.ascontiguousarray(pc_dircos, dtype=NP.float64).reshape(-1, 3)
    bl = NP.ascontiguousarray(baselines, dtype=NP.float64).reshape(-1, 3)
    fq = NP.ascontiguousarray(freqs_hz, dtype=NP.float64).ravel()
    npix, nt, nbl, nchan = uv.shape[0], rt.shape[0], bl.shape[0], fq.size
    if pc.shape[0] != nt:
        raise ValueError('pc_dircos must have one row per snapshot')
    ab = None
    if aberr_beta is not None:
        ab = NP.ascontiguousarray(aberr_beta, dtype=NP.float64).reshape(-1, 3)
        if ab.shape[0] != nt:
            raise ValueError('aberr_beta must have one row per snapshot')
    if route != 'auto' and route not in IMAGING_ROUTES.values():
        raise ValueError("route must be 'auto', 'direct' or 'stepped'")
    x = None
    if cube is not None:
        x = NP.ascontiguousarray(cube, dtype=NP.complex128)
        if x.shape != (nt, nbl, nchan):
            raise ValueError('cube must be (nt, nbl, nchan)')
    w, form = None, PRISIM_IMAGE_W_NONE
    if weights is not None:
        w = NP.ascontiguousarray(weights, dtype=NP.float64)
        if w.shape == (nbl,):
            form = PRISIM_IMAGE_W_BASELINE
        elif w.shape == (nt, nbl, nchan):
            form = PRISIM_IMAGE_W_FULL
        else:
            raise ValueError('weights must be None, (nbl,) or (nt, nbl, nchan)')
    a.npix, a.nbl, a.nchan, a.nt = npix, nbl, nchan, nt
    a.unitvec, a.rot, a.aberr_beta, a.pc_dircos = _ptr(uv), _ptr(rt), _ptr(ab), _ptr(pc)
    a.baselines, a.freqs_hz, a.cube, a.weights = _ptr(bl), _ptr(fq), _ptr(x), _ptr(w)
    a.weight_form, a.chan_avg, a.route = form, 1 if chan_avg else 0, _route_code(route, IMAGING_ROUTES)
    a.budget_bytes = int(budget_bytes or 0)
    return npix, nbl, nchan, nt, x is None, (uv, rt, pc, bl, fq, ab, x, w)


def _mosaic_beam_fields(a, nt, beam_kind, diameter_m, beam_pc_dircos, ext, pbmin):
    """The beam of mosaic_image and clean_mosaic put into the fields their argument structs have alike: beam_pc_dircos (3,) or (nt, 3);
    ext None, a dict or one dict per snapshot; pbmin.  Returns what the struct points into, to be held until the call is over."""
    bpc = NP.ascontiguousarray(beam_pc_dircos, dtype=NP.float64)
    if bpc.shape not in ((3,), (nt, 3)):
        raise ValueError('beam_pc_dircos must be (3,) or one row per snapshot (nt, 3)')
    exts, xs, keep_ext = _beam_ext_array(ext)
    a.beam_kind, a.diameter_m = int(beam_kind), float(diameter_m)
    a.beam_pc_dircos[:] = bpc.reshape(-1, 3)[0].tolist()
    a.beam_pc_snap = _ptr(bpc) if bpc.ndim == 2 else None
    a.ext = C.cast(xs, C.c_void_p) if exts else None
    a.n_ext = len(exts)
    a.pbmin = float(pbmin)
    return bpc, xs, keep_ext


def _clean_fields(a, npix, nc, gain, maxiter, threshold, threshold_relative, window, fwhm_rad, poll_every):
    """The CLEAN arguments of clean_image and clean_mosaic put into the fields their argument structs have alike.  Returns (maxiter,
    the window as uint8 or None, fwhm_rad (nc,) or None): the arrays the struct points into."""
    win = None
    if window is not None:
        win = NP.ascontiguousarray(NP.asarray(window) != 0, dtype=NP.uint8)
        if win.shape != (npix,):
            raise ValueError('window must be (npix,)')
    fw = None
    if fwhm_rad is not None:
        fw = NP.ascontiguousarray(NP.broadcast_to(NP.asarray(fwhm_rad, dtype=NP.float64), (nc,)))
    maxiter = int(maxiter)
    a.window, a.fwhm_rad = _ptr(win), _ptr(fw)
    a.gain, a.threshold, a.maxiter = float(gain), float(threshold), maxiter
    a.threshold_relative, a.poll_every = 1 if threshold_relative else 0, int(poll_every or 0)
    return maxiter, win, fw


def _clean_outputs(npix, nchan, nc, maxiter, chan_avg, restore):
    """The arrays every CLEAN entry fills, under the names of its out_* arguments: the residual and (with restore) the restored image,
    (npix,) with chan_avg else (npix, nchan); the lists (nc, maxiter), their unused tail -1 and 0; ncomp, status and peak0 (nc,)."""
    shape = (npix,) if chan_avg else (npix, nchan)
    rows = max(maxiter, 0)
    return {'out_residual': NP.empty(shape, dtype=NP.float64), 'out_restored': NP.empty(shape, dtype=NP.float64) if restore else None,
            'out_comp_pixel': NP.full((nc, rows), -1, dtype=NP.int32), 'out_comp_flux': NP.zeros((nc, rows), dtype=NP.float64),
            'out_ncomp': NP.empty(nc, dtype=NP.int32), 'out_status': NP.empty(nc, dtype=NP.int32), 'out_peak0': NP.empty(nc, dtype=NP.float64)}


def _clean_result(out):
    """What every CLEAN entry returns of _clean_outputs: the lists trimmed to the longest."""
    longest = int(out['out_ncomp'].max()) if out['out_ncomp'].size else 0
    return {'residual': out['out_residual'], 'restored': out['out_restored'],
            'comp_pixel': NP.ascontiguousarray(out['out_comp_pixel'][:, :longest]),
            'comp_flux': NP.ascontiguousarray(out['out_comp_flux'][:, :longest]), 'ncomp': out['out_ncomp'], 'status': out['out_status'],
            'peak0': out['out_peak0']}


def _want_bits(want, bits):
    """The OR of bits[name] over the names of want; KeyError on an unknown name."""
    flag = 0
    for name in want:
        flag |= bits[name]
    return flag


def _beam_ext_array(ext):
    """The beam extensions of a call as the library takes them: ext is None, a dict (make_beam_ext) or a sequence of one dict per
    snapshot.  Returns (the dicts, a contiguous PrisimBeamExt array of at least one element, the structs that keep the beamformer
    arrays alive while the array is in use)."""
    exts = [] if ext is None else ([ext] if isinstance(ext, dict) else list(ext))
    xs = (PrisimBeamExt * max(len(exts), 1))()
    keep = []
    for i, e in enumerate(exts):
        x = make_beam_ext(e)
        keep.append(x)
        C.memmove(C.byref(xs, i * C.sizeof(PrisimBeamExt)), C.byref(x), C.sizeof(PrisimBeamExt))
    return exts, xs, keep


def _route_code(name, routes):
    """The library's code of a route: 'auto' (-1 in every header) or a name of the table routes (code: name); KeyError on another."""
    return -1 if name == 'auto' else {v: k for k, v in routes.items()}[name]


# every struct the headers typedef -> its ctypes mirror
STRUCTS = {
    'prisim_sky': PrisimSky, 'prisim_beam_ext': PrisimBeamExt, 'prisim_beam_sky': PrisimBeamSky, 'prisim_catalog': PrisimCatalog,
    'prisim_obs': PrisimObs, 'prisim_snapshot': PrisimSnapshot, 'prisim_post': PrisimPost, 'prisim_timing': PrisimTiming,
    'prisim_comm_stats': PrisimCommStats, 'prisim_clean_stats': PrisimCleanStats, 'prisim_subband_stats': PrisimSubbandStats,
    'prisim_runs_stats': PrisimRunsStats, 'prisim_closure_stats': PrisimClosureStats, 'prisim_cpdelay_stats': PrisimCpdelayStats,
    'prisim_cpbins_stats': PrisimCpbinsStats, 'prisim_cpdiff_stats': PrisimCpdiffStats, 'prisim_cpft_stats': PrisimCpftStats,
    'prisim_cpxps_stats': _PrisimCpxpsStats, 'prisim_cpavg_stats': _PrisimCpavgStats, 'prisim_cpreal_stats': _PrisimCprealStats,
    'prisim_antpower_stats': _PrisimAntpowerStats, 'prisim_antpower_args': _PrisimAntpowerArgs,
    'prisim_imaging_stats': _PrisimImagingStats, 'prisim_imaging_args': _PrisimImagingArgs, 'prisim_gains_stats': PrisimGainsStats,
    'prisim_imclean_stats': _PrisimImcleanStats, 'prisim_imclean_args': _PrisimImcleanArgs,
    'prisim_mosaic_stats': _PrisimMosaicStats, 'prisim_mosaic_args': _PrisimMosaicArgs,
    'prisim_mosclean_stats': _PrisimMoscleanStats, 'prisim_mosclean_args': _PrisimMoscleanArgs,
    'prisim_csclean_stats': _PrisimCscleanStats, 'prisim_csclean_args': _PrisimCscleanArgs,
    'prisim_moscs_stats': _PrisimMoscsStats, 'prisim_moscs_args': _PrisimMoscsArgs,
}

# The C ABI, declared once: per header of include/, its functions in the header's order, each as
#   <return> <function>(<class> <parameter name>, ...);
# with the header's parameter names.  Return: int (an error code), void, or str (const char*).  Classes: p pointer (void*, arrays and
# opaque handles), i int32, q int64, Q uint64, d double, s char*; *<struct> a pointer to a mirrored struct of STRUCTS, *<class> a
# pointer to one such scalar (an output).  tests/test_abi_headers.py holds every row to the text of its header.
_PROTOTYPES = {
    'prisim_hip.h': '''
        int prisim_hip_create(i device, *p out);
        void prisim_hip_destroy(p ctx);
        str prisim_hip_last_error(p ctx);
        str prisim_hip_version();
        int prisim_hip_set_array(p ctx, p bl_enu, q nbl, p freqs_hz, q nchan, q nt_max);
        int prisim_hip_set_sky(p ctx, *prisim_sky sky);
        int prisim_hip_compute(p ctx, i precision, i kernel, i want_grad, q slot);
        int prisim_hip_get_vis(p ctx, q slot, p vis, p grad, i out_is_c64);
        int prisim_hip_set_vis(p ctx, q slot, p vis);
        int prisim_hip_skyvis(p ctx, *prisim_sky sky, i precision, i kernel, p vis, p grad, i out_is_c64);
        int prisim_hip_set_sky_analytic(p ctx, *prisim_beam_sky sky);
        int prisim_hip_set_external_beam(p ctx, p beam, q npix, q nfreq, p interp_matrix);
        int prisim_hip_set_sky_external(p ctx, *prisim_sky sky);
        int prisim_hip_set_sky_external_analytic(p ctx, *prisim_beam_sky sky);
        int prisim_hip_get_pbflux(p ctx, p out);
        int prisim_hip_set_catalog(p ctx, *prisim_catalog cat);
        int prisim_hip_set_sky_from_catalog(p ctx, *prisim_obs obs, *prisim_snapshot snap, *q nsrc_roi);
        int prisim_hip_catalog_roi(p ctx, *prisim_obs obs, *prisim_snapshot snap, *q nsrc_roi, p indices, p dircos, q cap);
        int prisim_hip_observe_catalog(p ctx, *prisim_obs obs, *prisim_snapshot snaps, q nsnap, i precision, i want_grad, q slot0, p nsrc_roi,
            *prisim_post post);
        int prisim_hip_delay_transform(p ctx, q nt, p bpwts, d pad, p out, p lags_out, p out_power, d power_scale);
        int prisim_hip_delay_transform_device(p ctx, q nt, p bpwts, q wts_rows, d pad, i want_lag, i want_power, d power_scale, p lags_out,
            *q nout_out);
        int prisim_hip_get_lags(p ctx, q t0, q nt, p rows, q nrows, p out);
        int prisim_hip_get_delay_power(p ctx, q t0, q nt, p rows, q nrows, p out);
        int prisim_hip_phase_rotate(p ctx, q nt, p diff_dircos);
        int prisim_hip_noise(p ctx, q nt, p rms, Q seed, q bl_offset, p out);
        int prisim_hip_noise_indexed(p ctx, q nt, p rms, Q seed, p bl_index, p out);
        int prisim_hip_comm_unique_id(s id);
        int prisim_hip_comm_version(s out);
        int prisim_hip_comm_init(p ctx, s id, i nranks, i rank);
        int prisim_hip_device_pci(i device, s out);
        int prisim_hip_comm_last_error(s out);
        int prisim_hip_allgather(p ctx, q nt, i as_c64);
        int prisim_hip_allgather_slot_async(p ctx, q slot, i as_c64);
        int prisim_hip_get_gathered(p ctx, q nt, p out);
        int prisim_hip_allgather_lags(p ctx, q nt);
        int prisim_hip_gathered_checksum(p ctx, q nt, *d out);
        int prisim_hip_allgather_grad(p ctx, q nt, i as_c64);
        int prisim_hip_set_shard_map(p ctx, p bl_index, q nbl_total);
        int prisim_hip_set_gather_root(p ctx, i root);
        int prisim_hip_comm_selftest(p ctx, q bytes);
        int prisim_hip_get_comm_stats(p ctx, *prisim_comm_stats out, i reset);
        int prisim_hip_host_alloc(q bytes, *p out);
        int prisim_hip_host_free(p p);
        int prisim_hip_get_vis_async(p ctx, q slot, p vis, p grad, i out_is_c64);
        int prisim_hip_wait_downloads(p ctx);
        int prisim_hip_sync(p ctx);
        int prisim_hip_get_timing(p ctx, *prisim_timing out, i reset);
        int prisim_hip_get_fold_info(p ctx, *q last_sum_baselines, *q last_terms_evaluated, *q last_sum_lift_groups);
        int prisim_hip_get_fold_near(p ctx, *q exact_baselines, *q near_baselines, *d max_dev_m, *d phase_bound_rad, *i used);
        int prisim_hip_get_step_tiers(p ctx, *q last_sum_wide_groups, *d wide_limit_cycles);
        int prisim_hip_get_tail_pieces(p ctx, *q pieces, *q tail_pieces);
        int prisim_hip_device_info(p ctx, *i cu_count, *i clock_khz, s name);
        int prisim_hip_set_tuning(p ctx, i chan_tile, i src_chunk, i nsplit);
    ''',
    'prisim_clean.h': '''
        int prisim_clean_rows(p ctx, q nrows, q m, p inp, q nkern, p kern, p kidx, p cbox, d gain, q maxiter, d threshold, i threshold_absolute,
            p cc, p res, p iters, p flags, p rms, *prisim_clean_stats stats);
        int prisim_clean_delay(p ctx, i ncubes, q nrows, q nchan, q m, p win, q nkern, p kwin, p kidx, p cbox, d lag_scale, d freq_scale1,
            d freq_scale2, d gain, q maxiter, d threshold, i threshold_absolute, p lag, p kern_lag, p cc, p res, p cc_freq, p res_freq, p iters,
            p flags, p rms, *prisim_clean_stats stats);
    ''',
    'prisim_subband.h': '''
        int prisim_subband_transform(p ctx, i ncubes, q nt, q nbl, q nchan, p cubes, q t0, p bp, q nbp, i nwin, p wts, q m, d df, q nres, q nmap,
            p map_out, p map_in, p map_w, p pscale, i want, i route, p over, p over_pow, p res, p res_pow, *prisim_subband_stats stats);
    ''',
    'prisim_runs.h': '''
        int prisim_runs_transform(p ctx, q R, q nbl, q nchan, q nt, p vis, i vis_is_c64, p bp, p bp_strides, p wts, p wts_strides, i nwin, p win,
            q m, d scale, i out_mode, q nout, d factor, q nmap, p map_out, p map_in, p map_w, i route, q budget_bytes, p out,
            *prisim_runs_stats stats);
        int prisim_runs_power(p ctx, q nf, q inner, p v1, p v2, i is_c64, p factor, i cross, i fused_product, q budget_bytes, p out,
            *prisim_runs_stats stats);
    ''',
    'prisim_closure.h': '''
        int prisim_closure_phase(p ctx, p cube, q nt, q nbl, q nchan, p legs, p conj, q ntriads, p freq_wts, p bpwts, p masks, q nmask,
            p mask_index, i route, q budget_bytes, p out_triplets, p out_phase, *prisim_closure_stats stats);
    ''',
    'prisim_cpdelay.h': '''
        int prisim_closure_delay_spectra(p ctx, p phases, q nrows, p cube, q nt, q nbl, q nchan, p legs, p conj, p freq_wts, p bpwts, p masks,
            q nmask, p mask_index, i phase_route, i nwin, p wts, q m, d df, q nres, q nmap, p map_out, p map_in, p map_w, p pscale, i want,
            i route, q budget_bytes, p out_phase, p over, p over_pow, p res, p res_pow, *prisim_cpdelay_stats stats);
        int prisim_closure_power(p ctx, q n0, q nwin, q inner, p spectra, p scale, i want, q budget_bytes, p out_individual, p out_auto,
            p out_cross, *prisim_cpdelay_stats stats);
    ''',
    'prisim_cpbins.h': '''
        int prisim_cphase_bin(p ctx, i kind, p in_mean, p in_median, p in_wts, p in_flags, q n0, q n1, q ntriads, q nchan, i axis, q nbins,
            p offsets, p members, i want, i mad_ignores_flags, q budget_bytes, *p resident_in, *p keep_out, p out_wts, p out_eicp_mean,
            p out_eicp_median, p out_cp_mean, p out_cp_median, p out_rms, p out_mad, *prisim_cpbins_stats stats);
        void prisim_cphase_stack_free(p stack);
    ''',
    'prisim_cpdiff.h': '''
        int prisim_cphase_diff(p ctx, p in_mean, p in_median, p in_wts, q n0, q n1, q ntriads, q nchan, p resident, q ncomb, p pairs,
            q budget_bytes, p out_diff0_mean, p out_diff0_median, p out_diff1_mean, p out_diff1_median, p out_wts0, p out_wts1, p out_mask0,
            p out_mask1, *prisim_cpdiff_stats stats);
    ''',
    'prisim_cpft.h': '''
        int prisim_cphase_ft(p ctx, q n0, q n1, q n2, q nchan, i nin, p inputs, p in_shape, p w, i nwin, p wts, p vscale, q m, d df, q nres,
            q nmap, p map_out, p map_in, p map_w, i want, i route, q budget_bytes, p over, p res, p lag_kernel, p lag_kernel_res,
            *prisim_cpft_stats stats);
    ''',
    'prisim_cpxps.h': '''
        int prisim_cphase_xpower(p ctx, q nspw, q n1, q n2, q n3, q nlags, p a, p b, p factor, p weights, p modes, q nshift, p shifts,
            i ncollapse, p order, i stat, q budget_bytes, p out, *prisim_cpxps_stats stats);
    ''',
    'prisim_cpavg.h': '''
        int prisim_cphase_xavg(p ctx, i ndim, p shape, q nsets, p arrays, p weights, p wshapes, i ncombo, p reduce, p masks, q budget_bytes,
            p avg, p wsum, p out, p wout, *prisim_cpavg_stats stats);
        int prisim_cphase_kbin(p ctx, q nspw, q m, q nlags, q nk, p p, p kprll, p offsets, p members, i route, q budget_bytes, p ps, p del2, p kc,
            *prisim_cpavg_stats stats);
    ''',
    'prisim_cpreal.h': '''
        int prisim_closure_realizations(p ctx, p cube, p cube_row, p bl_global, q nt, q nrow, q nchan, p rms, p bpwts, p legs, p conj, q ntriads,
            Q seed, q first, q n_realize, i kind, i route, q budget_bytes, p out_phase, *prisim_cpreal_stats stats);
    ''',
    'prisim_antpower.h': '''
        int prisim_antenna_power(p ctx, *prisim_antpower_args a, p out_power, p out_num, p out_den, *prisim_antpower_stats stats);
    ''',
    'prisim_imaging.h': '''
        int prisim_dirty_image(p ctx, *prisim_imaging_args a, p out_image, p out_wsum, *prisim_imaging_stats stats);
    ''',
    'prisim_imaging32.h': '''
        int prisim_dirty_image_f32(p ctx, *prisim_imaging_args a, p out_image, p out_wsum, *prisim_imaging_stats stats);
    ''',
    'prisim_imclean.h': '''
        int prisim_clean_image(p ctx, *prisim_imclean_args a, p out_residual, p out_restored, p out_comp_pixel, p out_comp_flux, p out_ncomp,
            p out_status, p out_peak0, p out_wsum, *prisim_imclean_stats stats);
    ''',
    'prisim_mosaic.h': '''
        int prisim_mosaic_image(p ctx, *prisim_mosaic_args a, p out_mosaic, p out_pb_eff, p out_num, p out_den, p out_wsum,
            *prisim_mosaic_stats stats);
    ''',
    'prisim_mosaic32.h': '''
        int prisim_mosaic_image_f32(p ctx, *prisim_mosaic_args a, p out_mosaic, p out_pb_eff, p out_num, p out_den, p out_wsum,
            *prisim_mosaic_stats stats);
    ''',
    'prisim_mosclean.h': '''
        int prisim_clean_mosaic(p ctx, *prisim_mosclean_args a, p out_residual, p out_restored, p out_residual_flat, p out_pb_eff, p out_num,
            p out_den, p out_wsum, p out_comp_pixel, p out_comp_flux, p out_ncomp, p out_status, p out_peak0, *prisim_mosclean_stats stats);
    ''',
    'prisim_csclean.h': '''
        int prisim_clean_image_cs(p ctx, *prisim_csclean_args a, p out_residual, p out_restored, p out_comp_pixel, p out_comp_flux,
            p out_ncomp, p out_status, p out_peak0, p out_wsum, p out_ncycles, p out_cycle_ncomp, p out_cycle_peak, p out_psf, p out_vres,
            *prisim_csclean_stats stats);
    ''',
    'prisim_moscs.h': '''
        int prisim_clean_mosaic_cs(p ctx, *prisim_moscs_args a, p out_residual, p out_restored, p out_residual_flat, p out_pb_eff, p out_num,
            p out_den, p out_wsum, p out_comp_pixel, p out_comp_flux, p out_ncomp, p out_status, p out_peak0, p out_ncycles,
            p out_cycle_ncomp, p out_cycle_peak, p out_psf, p out_vres, *prisim_moscs_stats stats);
    ''',
    'prisim_gains.h': '''
        int prisim_gains_eval_spline(p ctx, q nrows, i kx, i ky, p nx, p ny, p kx_off, p ky_off, p c_off, q nknots, p knots, q ncoefs, p coefs,
            q nt, p times, q nchan, p freqs, *p out, *prisim_gains_stats stats);
        int prisim_gains_gather(p ctx, q nrows, q ngf, q ngt, p gains, q nchan, p fidx, q nt, p tidx, *p out, *prisim_gains_stats stats);
        int prisim_gains_table_shape(p tab, *q nt, *q nrows, *q nchan);
        int prisim_gains_table_get(p ctx, p tab, p out);
        void prisim_gains_table_free(p tab);
        int prisim_gains_apply(p ctx, q nt, q nbl, q nchan, p ta, i mode_a, p a_a, p c_a, p tb, i mode_b, p a_b, p c_b, p sky, q t0, i sky_c64,
            p noise, i want_gain, p vis, *prisim_gains_stats stats);
    ''',
}
_CLASSES = {'p': C.c_void_p, 'i': C.c_int32, 'q': C.c_int64, 'Q': C.c_uint64, 'd': C.c_double, 's': C.c_char_p}
_RETURNS = {'int': C.c_int, 'void': None, 'str': C.c_char_p}


def _parse_prototypes(table):
    """(FUNCTIONS, HEADER_EXPORTS) of a table like _PROTOTYPES: function -> (restype, ((parameter name, ctypes class), ...)), and
    header -> the names of its functions in order."""
    functions, exports = {}, {}
    for header, text in table.items():
        names = []
        for row in text.split(';')[:-1]:
            ret, name, params = re.match(r'\s*(\w+) (\w+)\((.*)\)$', row, flags=re.S).groups()
            pairs = []
            for code, pname in (p.split() for p in params.split(',') if p.strip()):
                inner = code.lstrip('*')
                ctype = STRUCTS[inner] if inner in STRUCTS else _CLASSES[inner]
                pairs.append((pname, C.POINTER(ctype) if code.startswith('*') else ctype))
            functions[name] = (_RETURNS[ret], tuple(pairs))
            names.append(name)
        exports[header] = tuple(names)
    return functions, exports


FUNCTIONS, HEADER_EXPORTS = _parse_prototypes(_PROTOTYPES)
# the functions of each header (tests and tools import these names)
(EXPORTS, CLEAN_EXPORTS, SUBBAND_EXPORTS, RUNS_EXPORTS, CLOSURE_EXPORTS, CPDELAY_EXPORTS, CPBINS_EXPORTS, CPDIFF_EXPORTS, CPFT_EXPORTS,
 CPXPS_EXPORTS, CPAVG_EXPORTS, CPREAL_EXPORTS, ANTPOWER_EXPORTS, IMAGING_EXPORTS, IMAGING32_EXPORTS, IMCLEAN_EXPORTS, MOSAIC_EXPORTS, MOSAIC32_EXPORTS,
 MOSCLEAN_EXPORTS, CSCLEAN_EXPORTS, MOSCS_EXPORTS, GAINS_EXPORTS) = (
    HEADER_EXPORTS['prisim_%s.h' % h] for h in ('hip', 'clean', 'subband', 'runs', 'closure', 'cpdelay', 'cpbins', 'cpdiff', 'cpft', 'cpxps',
                                                'cpavg', 'cpreal', 'antpower', 'imaging', 'imaging32', 'imclean', 'mosaic', 'mosaic32', 'mosclean',
                                                'csclean', 'moscs', 'gains'))


class PrisimHipError(RuntimeError):
    """Raised when libprisim_hip.so is missing/unloadable or no GPU is usable."""


_lib = None


def load_library():
    """Load libprisim_hip.so and declare the prototypes.  Raises PrisimHipError if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PrisimHipError('HIP extension not built: {0} is missing. Run `python -c "import __graft_entry__ as g; '
                             'g.build()"` (or make -C prisim_amd/csrc). There is no CPU fallback.'.format(LIB_PATH))
    try:
        lib = C.CDLL(LIB_PATH)
    except OSError as exc:
        raise PrisimHipError('cannot load {0}: {1}'.format(LIB_PATH, exc))
    lib.prisim_hip_version.restype, lib.prisim_hip_version.argtypes = C.c_char_p, []
    have = (lib.prisim_hip_version() or b'').decode()
    if have != ABI_VERSION:
        # a library of another round next to this binding: the structs below (prisim_timing, prisim_beam_sky ...) would be read wrongly
        raise PrisimHipError('{0} reports {1!r}, this binding is written for {2!r}: rebuild it (python -c "import __graft_entry__ as g; '
                             'g.build()")'.format(LIB_PATH, have, ABI_VERSION))
    for name, (restype, params) in FUNCTIONS.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, [ctype for _, ctype in params]
    _lib = lib
    return lib


def _ptr(arr):
    return None if arr is None else arr.ctypes.data_as(C.c_void_p)


def _call_declared(fn, name, params, kw):
    """fn(*args), the arguments taken by name from kw, put into the declared order params ((name, class), ...) and marshalled by
    class.  Integers go through int(), doubles through float().  To a pointer class, None is NULL; a numpy array goes as its data
    pointer and must be C-contiguous (ValueError); a ctypes struct, or an instance of the class a scalar pointer points to, goes by
    reference; any other ctypes object (a handle, an array of pointers) as it is.  TypeError, before anything is called, when kw
    lacks a declared name or holds another."""
    if len(kw) != len(params) or any(pname not in kw for pname, _ in params):
        declared = set(pname for pname, _ in params)
        raise TypeError('{0}: missing {1}, unknown {2}'.format(name, sorted(declared - set(kw)), sorted(set(kw) - declared)))
    args = []
    for pname, ctype in params:
        v = kw[pname]
        if ctype in (C.c_int32, C.c_int64, C.c_uint64):
            v = int(v)
        elif ctype is C.c_double:
            v = float(v)
        elif isinstance(v, NP.ndarray):
            if not v.flags.c_contiguous:
                raise ValueError('{0}: {1} must be a C-contiguous array'.format(name, pname))
            v = v.ctypes.data
        elif isinstance(v, C.Structure) or (ctype not in (C.c_void_p, C.c_char_p) and isinstance(v, ctype._type_)):
            v = C.byref(v)
        args.append(v)
    return fn(*args)


def _raise(code, msg):
    """Map the C-ABI error codes onto the exception types the reference raises inline."""
    if code == PRISIM_EINVAL:
        raise ValueError(msg)
    if code == PRISIM_ENOMEM:
        raise MemoryError(msg)
    if code == PRISIM_ESTATE:
        raise RuntimeError(msg)
    raise PrisimHipError(msg)


def host_empty(shape, dtype):
    """numpy array over page-locked host memory (prisim_hip_host_alloc): the destination of asynchronous downloads.  Freed when the
    last view of it is garbage-collected."""
    import weakref
    lib = load_library()
    dtype = NP.dtype(dtype)
    nbytes = int(NP.prod(shape, dtype=NP.int64)) * dtype.itemsize
    p = C.c_void_p()
    rc = lib.prisim_hip_host_alloc(max(nbytes, 1), C.byref(p))
    if rc != PRISIM_OK:
        _raise(rc, 'prisim_hip_host_alloc({0} B) failed: {1}'.format(nbytes, lib.prisim_hip_last_error(None).decode()))
    buf = (C.c_char * max(nbytes, 1)).from_address(p.value)
    weakref.finalize(buf, lib.prisim_hip_host_free, C.c_void_p(p.value))
    return NP.frombuffer(buf, dtype=dtype, count=int(NP.prod(shape, dtype=NP.int64))).reshape(shape)


class Context(object):
    """One GPU <-> one context <-> one HIP stream (include/prisim_hip.h)."""

    def __init__(self, device=0):
        self._lib = load_library()
        h = C.c_void_p()
        rc = self._lib.prisim_hip_create(int(device), C.byref(h))
        if rc != PRISIM_OK:
            msg = self._lib.prisim_hip_last_error(None).decode()
            _raise(rc, 'prisim_hip_create(device={0}) failed: {1}'.format(device, msg))
        self._h = h
        self.device = int(device)
        self.nbl = self.nchan = self.nt_max = 0
        self.nsrc = 0

    def close(self):
        if getattr(self, '_h', None):
            self._lib.prisim_hip_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc, what):
        if rc != PRISIM_OK:
            msg = self._lib.prisim_hip_last_error(self._h).decode()
            _raise(rc, '{0} failed: {1}'.format(what, msg))

    def _call(self, entry, **kw):
        """An add-on entry by parameter name: one keyword per name the table declares for it (`ctx` is this context unless given),
        marshalled by _call_declared, and the returned code checked."""
        restype, params = FUNCTIONS[entry]
        if params[0][0] == 'ctx':
            kw.setdefault('ctx', self._h)
        rc = _call_declared(getattr(self._lib, entry), entry, params, kw)
        if restype is not None:
            self._check(rc, entry)

    # ---- array ----
    def set_array(self, baselines, freqs_hz, nt_max=1):
        bl = NP.ascontiguousarray(baselines, dtype=NP.float64).reshape(-1, 3)
        fr = NP.ascontiguousarray(freqs_hz, dtype=NP.float64).ravel()
        self._check(self._lib.prisim_hip_set_array(self._h, _ptr(bl), bl.shape[0], _ptr(fr), fr.size, int(nt_max)),
                    'prisim_hip_set_array')
        if getattr(self, 'nbl_total', 0) and bl.shape[0] != self.nbl:
            self.nbl_total = 0                       # (the library drops a shard map made for another shard size)
        self.nbl, self.nchan, self.nt_max = bl.shape[0], fr.size, int(nt_max)

    # ---- sky ----
    def _sky_struct(self, dircos, pbflux, pc_dircos, fwhm_deg, fluxes=None):
        dc = NP.ascontiguousarray(dircos, dtype=NP.float64).reshape(-1, 3)
        nsrc = dc.shape[0]
        pbflux = NP.asarray(pbflux)
        is_f32 = pbflux.dtype == NP.float32
        pb = NP.ascontiguousarray(pbflux, dtype=NP.float32 if is_f32 else NP.float64)
        if nsrc > 0 and pb.size != nsrc * self.nchan:
            raise ValueError('pbflux must have shape (nsrc, nchan) = ({0}, {1}), got {2}'.format(nsrc, self.nchan, pb.shape))
        pc = NP.ascontiguousarray(pc_dircos, dtype=NP.float64).ravel()
        if pc.size != 3:
            raise ValueError('pc_dircos must have 3 elements')
        fw = None
        if fwhm_deg is not None:
            fw = NP.ascontiguousarray(fwhm_deg, dtype=NP.float64).ravel()
            if fw.size != nsrc:
                raise ValueError('fwhm_deg must have nsrc elements')
        fl = None
        if fluxes is not None:
            fl = NP.ascontiguousarray(fluxes, dtype=NP.float64)
            if fl.size != nsrc * self.nchan:
                raise ValueError('fluxes must have shape (nsrc, nchan)')
        sky = PrisimSky(nsrc, _ptr(dc), _ptr(pb), 1 if is_f32 else 0, _ptr(pc), _ptr(fw), _ptr(fl))
        return sky, (dc, pb, pc, fw, fl)

    def set_sky(self, dircos, pbflux, pc_dircos, fwhm_deg=None, fluxes=None):
        """pbflux: beam x flux (nsrc, nchan); or, with `fluxes` given, the beam alone (product formed on the device)."""
        sky, keep = self._sky_struct(dircos, pbflux, pc_dircos, fwhm_deg, fluxes)
        self._check(self._lib.prisim_hip_set_sky(self._h, C.byref(sky)), 'prisim_hip_set_sky')
        self.nsrc = sky.nsrc

    def set_sky_analytic(self, dircos, flux_ref, spindex, ref_freq_hz, beam_kind, diameter_m, beam_pc_dircos,
                         pc_dircos, fwhm_deg=None, flux_spectrum=None, ext=None):
        """Fused beam x flux on the device.  Flux is the power law flux_ref*(f/ref)^spindex, or, when
        flux_spectrum (nsrc, nchan) is given, that tabulated spectrum."""
        dc = NP.ascontiguousarray(dircos, dtype=NP.float64).reshape(-1, 3)
        nsrc = dc.shape[0]
        fs = fr = sp = None
        if flux_spectrum is not None:
            fs = NP.ascontiguousarray(flux_spectrum, dtype=NP.float64)
            if fs.size != nsrc * self.nchan:
                raise ValueError('flux_spectrum must have shape (nsrc, nchan)')
            ref_freq_hz = 1.0 if ref_freq_hz is None else ref_freq_hz
        else:
            fr = NP.ascontiguousarray(flux_ref, dtype=NP.float64).ravel()
            sp = NP.ascontiguousarray(spindex, dtype=NP.float64).ravel()
            if fr.size != nsrc or sp.size != nsrc:
                raise ValueError('flux_ref and spindex must have nsrc elements')
        bpc = NP.ascontiguousarray(beam_pc_dircos, dtype=NP.float64).ravel()
        pc = NP.ascontiguousarray(pc_dircos, dtype=NP.float64).ravel()
        fw = None
        if fwhm_deg is not None:
            fw = NP.ascontiguousarray(fwhm_deg, dtype=NP.float64).ravel()
            if fw.size != nsrc:
                raise ValueError('fwhm_deg must have nsrc elements')
        xs = make_beam_ext(ext)
        sky = PrisimBeamSky(nsrc, _ptr(dc), _ptr(fr), _ptr(sp), _ptr(fs), float(ref_freq_hz), int(beam_kind), float(diameter_m),
                            _ptr(bpc), _ptr(pc), _ptr(fw), None if xs is None else C.cast(C.pointer(xs), C.c_void_p))
        self._check(self._lib.prisim_hip_set_sky_analytic(self._h, C.byref(sky)), 'prisim_hip_set_sky_analytic')
        self.nsrc = nsrc

    def set_external_beam(self, beam, interp_matrix):
        """beam (npix, nfreq) HEALPix RING, local frame; interp_matrix (nchan, nfreq) spectral interpolation operator."""
        b = NP.ascontiguousarray(beam, dtype=NP.float64)
        if b.ndim != 2:
            raise ValueError('beam must be a (npix, nfreq) array')
        m = NP.ascontiguousarray(interp_matrix, dtype=NP.float64)
        if m.shape != (self.nchan, b.shape[1]):
            raise ValueError('interp_matrix must have shape (nchan, nfreq) = ({0}, {1})'.format(self.nchan, b.shape[1]))
        self._check(self._lib.prisim_hip_set_external_beam(self._h, _ptr(b), b.shape[0], b.shape[1], _ptr(m)),
                    'prisim_hip_set_external_beam')

    def set_sky_external(self, dircos, fluxes, pc_dircos, fwhm_deg=None):
        dc = NP.ascontiguousarray(dircos, dtype=NP.float64).reshape(-1, 3)
        nsrc = dc.shape[0]
        fl = NP.ascontiguousarray(fluxes, dtype=NP.float64)
        if fl.size != nsrc * self.nchan:
            raise ValueError('fluxes must have shape (nsrc, nchan)')
        pc = NP.ascontiguousarray(pc_dircos, dtype=NP.float64).ravel()
        if pc.size != 3:
            raise ValueError('pc_dircos must have 3 elements')
        fw = None
        if fwhm_deg is not None:
            fw = NP.ascontiguousarray(fwhm_deg, dtype=NP.float64).ravel()
            if fw.size != nsrc:
                raise ValueError('fwhm_deg must have nsrc elements')
        sky = PrisimSky(nsrc, _ptr(dc), None, 0, _ptr(pc), _ptr(fw), _ptr(fl))
        self._check(self._lib.prisim_hip_set_sky_external(self._h, C.byref(sky)), 'prisim_hip_set_sky_external')
        self.nsrc = nsrc

    def set_sky_external_analytic(self, dircos, flux_ref, spindex, ref_freq_hz, pc_dircos, fwhm_deg=None, flux_spectrum=None):
        """External-beam sky whose flux spectra are formed on the device from the power law flux_ref*(f/ref)^spindex (only nsrc-sized
        vectors are uploaded per snapshot), or from flux_spectrum (nsrc, nchan) when given."""
        dc = NP.ascontiguousarray(dircos, dtype=NP.float64).reshape(-1, 3)
        nsrc = dc.shape[0]
        fs = fr = sp = None
        if flux_spectrum is not None:
            fs = NP.ascontiguousarray(flux_spectrum, dtype=NP.float64)
            if fs.size != nsrc * self.nchan:
                raise ValueError('flux_spectrum must have shape (nsrc, nchan)')
            ref_freq_hz = 1.0 if ref_freq_hz is None else ref_freq_hz
        else:
            fr = NP.ascontiguousarray(flux_ref, dtype=NP.float64).ravel()
            sp = NP.ascontiguousarray(spindex, dtype=NP.float64).ravel()
            if fr.size != nsrc or sp.size != nsrc:
                raise ValueError('flux_ref and spindex must have nsrc elements')
        pc = NP.ascontiguousarray(pc_dircos, dtype=NP.float64).ravel()
        if pc.size != 3:
            raise ValueError('pc_dircos must have 3 elements')
        fw = None
        if fwhm_deg is not None:
            fw = NP.ascontiguousarray(fwhm_deg, dtype=NP.float64).ravel()
            if fw.size != nsrc:
                raise ValueError('fwhm_deg must have nsrc elements')
        sky = PrisimBeamSky(nsrc, _ptr(dc), _ptr(fr), _ptr(sp), _ptr(fs), float(ref_freq_hz), PRISIM_BEAM_DELTA, 1.0,
                            _ptr(pc), _ptr(pc), _ptr(fw), None)
        self._check(self._lib.prisim_hip_set_sky_external_analytic(self._h, C.byref(sky)), 'prisim_hip_set_sky_external_analytic')
        self.nsrc = nsrc

    # ---- device-resident catalogue ----
    def set_catalog(self, location, coords, flux_ref=None, spindex=None, ref_freq_hz=None, flux_spectrum=None, fwhm_deg=None, unitvec='host'):
        """Upload a run's sky model once (prisim_hip_set_catalog): location (nsrc, 2) degrees in `coords` ('radec' | 'hadec' | 'altaz'),
        the power law flux_ref (f / ref_freq_hz)^spindex or flux_spectrum (nsrc, nchan), source sizes fwhm_deg (or None).
        unitvec: 'host' (default) -- the catalogue's unit vectors are formed here (geometry.catalog_unitvec) and uploaded, so that the host
        mirror of the snapshot geometry (geometry.frame_dircos) and the device select the same sources bit for bit; 'device' -- only
        `location` crosses and the device forms them; or an (nsrc, 3) array."""
        loc = NP.ascontiguousarray(location, dtype=NP.float64).reshape(-1, 2)
        nsrc = loc.shape[0]
        if coords not in PRISIM_COORDS:
            raise ValueError('coords must be "radec", "hadec" or "altaz"')
        uv = None
        if isinstance(unitvec, str):
            if unitvec == 'host':
                from . import geometry as _G
                uv = NP.ascontiguousarray(_G.catalog_unitvec(loc, coords))
            elif unitvec != 'device':
                raise ValueError("unitvec must be 'host', 'device' or an (nsrc, 3) array")
        elif unitvec is not None:
            uv = NP.ascontiguousarray(unitvec, dtype=NP.float64).reshape(-1, 3)
            if uv.shape[0] != nsrc:
                raise ValueError('unitvec must have shape (nsrc, 3)')
        fs = fr = sp = fw = None
        if flux_spectrum is not None:
            fs = NP.ascontiguousarray(flux_spectrum, dtype=NP.float64)
            if fs.size != nsrc * self.nchan:
                raise ValueError('flux_spectrum must have shape (nsrc, nchan)')
            ref_freq_hz = 1.0
        else:
            fr = NP.ascontiguousarray(flux_ref, dtype=NP.float64).ravel()
            sp = NP.ascontiguousarray(spindex, dtype=NP.float64).ravel()
            if fr.size != nsrc or sp.size != nsrc:
                raise ValueError('flux_ref and spindex must have nsrc elements')
        if fwhm_deg is not None:
            fw = NP.ascontiguousarray(fwhm_deg, dtype=NP.float64).ravel()
            if fw.size != nsrc:
                raise ValueError('fwhm_deg must have nsrc elements')
        cat = PrisimCatalog(nsrc, PRISIM_COORDS[coords], 0, _ptr(loc), _ptr(fr), _ptr(sp), float(ref_freq_hz), _ptr(fs), _ptr(fw), _ptr(uv))
        self._check(self._lib.prisim_hip_set_catalog(self._h, C.byref(cat)), 'prisim_hip_set_catalog')
        self.ncat = nsrc
        self.cat_coords = coords

    @staticmethod
    def make_obs(latitude_deg, roi_radius_deg=90.0, roi_center='zenith', beam_kind=PRISIM_BEAM_DELTA, diameter_m=1.0, ext=None,
                 use_external_beam=False):
        """prisim_obs of a run (keeps the beam extension alive as attribute _keep)."""
        xs = make_beam_ext(ext)
        obs = PrisimObs(float(latitude_deg), float(roi_radius_deg), 1 if roi_center == 'pointing_center' else 0, 1 if use_external_beam else 0,
                        int(beam_kind), 0, float(diameter_m), None if xs is None else C.cast(C.pointer(xs), C.c_void_p))
        obs._keep = xs
        return obs

    @staticmethod
    def _fill_snapshot(sn, lst_deg, pc_dircos, beam_pc_dircos, frame=None):
        """frame: None -- the library's fall-back rotation from lst and latitude (hour angle = LST - RA); or (R (3, 3), beta (3,)), the
        snapshot's catalogue-frame -> East-North-Up rotation and aberration vector (prisim_amd/frames.py snapshot_frame)."""
        sn.lst_deg = float(lst_deg)
        sn.pc_dircos[0], sn.pc_dircos[1], sn.pc_dircos[2] = float(pc_dircos[0]), float(pc_dircos[1]), float(pc_dircos[2])
        b = pc_dircos if beam_pc_dircos is None else beam_pc_dircos
        sn.beam_pc_dircos[0], sn.beam_pc_dircos[1], sn.beam_pc_dircos[2] = float(b[0]), float(b[1]), float(b[2])
        if frame is None:
            sn.frame_given = 0
        else:
            rot, beta = frame
            sn.frame_given = 1
            sn.cel2enu[:] = NP.asarray(rot, dtype=NP.float64).reshape(9).tolist()
            sn.aberr_beta[:] = NP.asarray(beta, dtype=NP.float64).reshape(3).tolist()
        return sn

    @classmethod
    def _snapshot(cls, lst_deg, pc_dircos, beam_pc_dircos, frame=None):
        return cls._fill_snapshot(PrisimSnapshot(), lst_deg, pc_dircos, beam_pc_dircos, frame)

    def set_sky_from_catalog(self, obs, lst_deg, pc_dircos, beam_pc_dircos=None, frame=None):
        """Snapshot geometry, region of interest, beam x flux of the resident catalogue on the device; returns the ROI source count."""
        sn = self._snapshot(lst_deg, pc_dircos, beam_pc_dircos, frame)
        n = C.c_int64()
        self._check(self._lib.prisim_hip_set_sky_from_catalog(self._h, C.byref(obs), C.byref(sn), C.byref(n)), 'prisim_hip_set_sky_from_catalog')
        self.nsrc = int(n.value)
        return self.nsrc

    def catalog_roi(self, obs, lst_deg, pc_dircos, want_indices=True, want_dircos=True, frame=None):
        """(indices int64 [n], dircos [n, 3]) of the region of interest of one snapshot, catalogue order (prisim_hip_catalog_roi)."""
        sn = self._snapshot(lst_deg, pc_dircos, None, frame)
        n = C.c_int64()
        self._check(self._lib.prisim_hip_catalog_roi(self._h, C.byref(obs), C.byref(sn), C.byref(n), None, None, 0), 'prisim_hip_catalog_roi')
        cnt = int(n.value)
        idx = NP.empty(cnt, dtype=NP.int64) if want_indices else None
        dc = NP.empty((cnt, 3), dtype=NP.float64) if want_dircos else None
        if cnt > 0 and (want_indices or want_dircos):
            self._check(self._lib.prisim_hip_catalog_roi(self._h, C.byref(obs), C.byref(sn), C.byref(n), _ptr(idx), _ptr(dc), cnt),
                        'prisim_hip_catalog_roi')
        return idx, dc

    def observe_catalog(self, obs, lst_deg, pc_dircos, beam_pc_dircos=None, precision=PRISIM_FP64, want_grad=False, slot0=0,
                        host_cube=None, gather=None, frames=None):
        """K snapshots of the resident catalogue in one call (prisim_hip_observe_catalog): lst_deg (K,), pc_dircos (K, 3) or (3,),
        beam_pc_dircos likewise (default: pc_dircos).  Results land in cube slots slot0 ... slot0 + K - 1; returns the ROI counts (K,).
        host_cube: page-locked (nt_max, nbl, nchan) complex128 / complex64 array (host_empty) every finished slot is downloaded into,
        behind its sky-sum; gather: None, or 'c128' / 'c64' -- every finished slot is all-gathered on the communication stream.
        frames: None (the library's fall-back rotation from lst and latitude), or K pairs (R (3, 3), beta (3,)) -- see _fill_snapshot.
        Arrays of at most 256 baselines take ONE launch per chunk of up to 256 snapshots in every mode (fp64, want_grad, and
        precision=PRISIM_FP32, whose arithmetic is then the fp64 launch's)."""
        lst = NP.asarray(lst_deg, dtype=NP.float64).ravel()
        k = lst.size
        if frames is not None and len(frames) != k:
            raise ValueError('frames must hold one (R, beta) pair per snapshot')
        # the K prisim_snapshot structs are filled through numpy views of their memory (20 doubles each: lst, pc[3], beam_pc[3],
        # {frame_given, reserved}, cel2enu[9], aberr_beta[3]) -- a per-field ctypes fill costs more than the C call of a small array
        cache = self.__dict__.get('_snap_cache')
        if cache is None or cache[0] != k:
            snaps = (PrisimSnapshot * k)()
            cache = self.__dict__['_snap_cache'] = (k, snaps, NP.frombuffer(snaps, dtype=NP.float64).reshape(k, 20),
                                                    NP.frombuffer(snaps, dtype=NP.int32).reshape(k, 40))
        _, snaps, fv, iv = cache
        fv[:, 0] = lst
        fv[:, 1:4] = NP.asarray(pc_dircos, dtype=NP.float64).reshape(-1, 3)
        fv[:, 4:7] = fv[:, 1:4] if beam_pc_dircos is None else NP.asarray(beam_pc_dircos, dtype=NP.float64).reshape(-1, 3)
        if frames is None:
            iv[:, 14] = 0
        else:
            iv[:, 14] = 1
            for t in range(k):
                fv[t, 8:17] = NP.asarray(frames[t][0], dtype=NP.float64).reshape(9)
                fv[t, 17:20] = frames[t][1]
        counts = NP.zeros(k, dtype=NP.int64)
        post = None
        if host_cube is not None or gather is not None:
            post = PrisimPost()
            if host_cube is not None:
                if host_cube.shape[1:] != (self.nbl, self.nchan) or host_cube.dtype not in (NP.complex128, NP.complex64) or not host_cube.flags['C_CONTIGUOUS']:
                    raise ValueError('host_cube must be a C-contiguous (nt, nbl, nchan) complex128 / complex64 array')
                if host_cube.shape[0] < slot0 + k:
                    raise ValueError('host_cube has fewer snapshots than slot0 + K')
                post.host_vis = host_cube.ctypes.data
                post.host_is_c64 = 1 if host_cube.dtype == NP.complex64 else 0
            if gather is not None:
                post.gather, post.gather_as_c64 = 1, (1 if gather == 'c64' else 0)
                self._gathered_c64 = gather == 'c64'
        self._check(self._lib.prisim_hip_observe_catalog(self._h, C.byref(obs), snaps, k, int(precision), 1 if want_grad else 0, int(slot0),
                                                         _ptr(counts), None if post is None else C.byref(post)), 'prisim_hip_observe_catalog')
        self.nsrc = int(counts[-1]) if k else 0
        return counts

    def get_pbflux(self):
        out = NP.empty((self.nsrc, self.nchan), dtype=NP.float64)
        self._check(self._lib.prisim_hip_get_pbflux(self._h, _ptr(out)), 'prisim_hip_get_pbflux')
        return out

    # ---- compute ----
    def compute(self, precision=PRISIM_FP64, kernel=PRISIM_KERNEL_AUTO, want_grad=False, slot=0):
        self._check(self._lib.prisim_hip_compute(self._h, int(precision), int(kernel), 1 if want_grad else 0, int(slot)),
                    'prisim_hip_compute')

    def get_vis(self, slot=0, want_grad=False, complex64=False):
        ctype = NP.complex64 if complex64 else NP.complex128
        vis = NP.empty((self.nbl, self.nchan), dtype=ctype)
        grad = NP.empty((3, self.nbl, self.nchan), dtype=ctype) if want_grad else None
        self._check(self._lib.prisim_hip_get_vis(self._h, int(slot), _ptr(vis), _ptr(grad), 1 if complex64 else 0),
                    'prisim_hip_get_vis')
        return (vis, grad) if want_grad else vis

    def skyvis(self, dircos, pbflux, pc_dircos, fwhm_deg=None, precision=PRISIM_FP64, kernel=PRISIM_KERNEL_AUTO,
               want_grad=False, complex64=False, fluxes=None):
        """One-shot drop-in for interferometry.py:6255-6376."""
        sky, keep = self._sky_struct(dircos, pbflux, pc_dircos, fwhm_deg, fluxes)
        ctype = NP.complex64 if complex64 else NP.complex128
        vis = NP.empty((self.nbl, self.nchan), dtype=ctype)
        grad = NP.empty((3, self.nbl, self.nchan), dtype=ctype) if want_grad else None
        self._check(self._lib.prisim_hip_skyvis(self._h, C.byref(sky), int(precision), int(kernel), _ptr(vis), _ptr(grad),
                                                1 if complex64 else 0), 'prisim_hip_skyvis')
        self.nsrc = sky.nsrc
        return (vis, grad) if want_grad else vis

    # ---- delay transform ----
    def delay_transform(self, nt, bpwts=None, pad=1.0, want_power=False, power_scale=1.0, want_lag=True):
        pad = max(float(pad), 0.0)
        nchan = self.nchan
        nout = delay_nout(nchan, pad)                     # the library writes nt * nbl rows of exactly this many lags back to back
        w = None
        if bpwts is not None:
            w = NP.ascontiguousarray(bpwts, dtype=NP.float64).reshape(self.nbl, nchan)
        out = NP.empty((nt, self.nbl, nout), dtype=NP.complex128) if want_lag else None
        pw = NP.empty((nt, self.nbl, nout), dtype=NP.float64) if want_power else None
        lags = NP.empty(nchan, dtype=NP.float64)
        self._check(self._lib.prisim_hip_delay_transform(self._h, int(nt), _ptr(w), pad, _ptr(out), _ptr(lags), _ptr(pw),
                                                         float(power_scale)), 'prisim_hip_delay_transform')
        return out, lags, pw

    def delay_transform_device(self, nt, bpwts=None, pad=1.0, want_lag=True, want_power=False, power_scale=1.0):
        """Delay-transform slots [0, nt) and leave the spectra in HBM (prisim_hip_delay_transform_device).  Returns (lags, nout);
        read the results with get_lags / get_delay_power or exchange them with allgather_lags."""
        pad = max(float(pad), 0.0)
        w, wrows = None, 0
        if bpwts is not None:
            w = NP.ascontiguousarray(bpwts, dtype=NP.float64)
            if w.size == self.nchan:
                w, wrows = w.reshape(1, self.nchan), 1                   # one window for every baseline
            else:
                w, wrows = w.reshape(self.nbl, self.nchan), self.nbl
                if self.nbl > 1 and NP.array_equal(w, NP.broadcast_to(w[:1], w.shape)):
                    w, wrows = NP.ascontiguousarray(w[:1]), 1
        lags = NP.empty(self.nchan, dtype=NP.float64)
        nout = C.c_int64()
        self._check(self._lib.prisim_hip_delay_transform_device(self._h, int(nt), _ptr(w), wrows, pad, 1 if want_lag else 0, 1 if want_power else 0,
                                                                float(power_scale), _ptr(lags), C.byref(nout)),
                    'prisim_hip_delay_transform_device')
        self._dt_nout = int(nout.value)
        # every transform overwrites the context's ONE resident spectrum buffer: holders of a lazily fetched result (DelaySpectrum with
        # action='store', InterferometerArray.skyvis_lag) remember the generation they produced and transform again when it has moved on
        self._dt_generation = getattr(self, '_dt_generation', 0) + 1
        return lags, self._dt_nout

    def _get_resident(self, fn, what, dtype, t0, nt, rows):
        r = None
        nrow = self.nbl
        if rows is not None:
            r = NP.ascontiguousarray(rows, dtype=NP.int64).ravel()
            nrow = r.size
        out = NP.empty((nt, nrow, self._dt_nout), dtype=dtype)
        self._check(fn(self._h, int(t0), int(nt), _ptr(r), 0 if r is None else r.size, _ptr(out)), what)
        return out

    def get_lags(self, t0, nt, rows=None):
        """(nt, nrows | nbl, nout) complex128 lag spectra of snapshots [t0, t0 + nt) from the device-resident result."""
        return self._get_resident(self._lib.prisim_hip_get_lags, 'prisim_hip_get_lags', NP.complex128, t0, nt, rows)

    def get_delay_power(self, t0, nt, rows=None):
        return self._get_resident(self._lib.prisim_hip_get_delay_power, 'prisim_hip_get_delay_power', NP.float64, t0, nt, rows)

    def allgather_lags(self, nt):
        """RCCL all-gather of the resident lag spectra, device to device; read with get_gathered(nt, nranks, row=nout)."""
        self._check(self._lib.prisim_hip_allgather_lags(self._h, int(nt)), 'prisim_hip_allgather_lags')
        self._gathered_c64 = False

    def set_vis(self, vis, slot=0):
        v = NP.ascontiguousarray(vis, dtype=NP.complex128)
        if v.shape != (self.nbl, self.nchan):
            raise ValueError('vis must have shape (nbl, nchan)')
        self._check(self._lib.prisim_hip_set_vis(self._h, int(slot), _ptr(v)), 'prisim_hip_set_vis')

    def delay_transform_host(self, vis, bpwts, pad):
        """Delay-transform one host snapshot (nbl, nchan): upload into slot 0, transform, download."""
        self.set_vis(vis, 0)
        out, lags, pw = self.delay_transform(1, bpwts=bpwts, pad=pad)
        return out[0], lags, pw

    def phase_rotate(self, nt, diff_dircos):
        """cube[t] *= exp(-2 pi i f (b . diff[t])/c) for t < nt, in place on the device (interferometry.py:7871-7877)."""
        d = NP.ascontiguousarray(diff_dircos, dtype=NP.float64).reshape(-1, 3)
        if d.shape[0] != nt:
            raise ValueError('diff_dircos must have one row per snapshot')
        self._check(self._lib.prisim_hip_phase_rotate(self._h, int(nt), _ptr(d)), 'prisim_hip_phase_rotate')

    def noise(self, rms, seed, bl_offset=0, bl_index=None):
        """Complex Gaussian noise (nt, nbl, nchan) with per-element rms (interferometry.py:6692), Philox counter-based draws
        on the device: identical for sharded and unsharded runs when bl_offset is the shard's first global baseline -- or, for
        shards that are not one contiguous range, bl_index holds the global index of every local baseline."""
        r = NP.ascontiguousarray(rms, dtype=NP.float64)
        if r.ndim != 3 or r.shape[1:] != (self.nbl, self.nchan):
            raise ValueError('rms must have shape (nt, nbl, nchan)')
        out = NP.empty(r.shape, dtype=NP.complex128)
        if bl_index is not None:
            ix = NP.ascontiguousarray(bl_index, dtype=NP.int64).ravel()
            if ix.size != self.nbl:
                raise ValueError('bl_index must have one entry per baseline')
            self._check(self._lib.prisim_hip_noise_indexed(self._h, r.shape[0], _ptr(r), int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(ix), _ptr(out)),
                        'prisim_hip_noise_indexed')
            return out
        self._check(self._lib.prisim_hip_noise(self._h, r.shape[0], _ptr(r), int(seed) & 0xFFFFFFFFFFFFFFFF, int(bl_offset), _ptr(out)),
                    'prisim_hip_noise')
        return out

    # ---- delay CLEAN (include/prisim_clean.h) ----
    @staticmethod
    def _clean_kernels(kern, kidx, nrows, n):
        k = NP.ascontiguousarray(kern, dtype=NP.complex128).reshape(-1, n)
        if kidx is None:
            if k.shape[0] != 1:
                raise ValueError('kidx is required with more than one kernel')
            return k, None
        ix = NP.ascontiguousarray(kidx, dtype=NP.int32).ravel()
        if ix.size != nrows:
            raise ValueError('kidx must have one entry per row')
        return k, ix

    def clean_rows(self, inp, kern, cbox, gain, maxiter, threshold, absolute=False, kidx=None):
        """Hogbom CLEAN of every row of inp (nrows, m) on the device (prisim_clean_rows).  kern: (nkern, m) kernels, row r uses
        kern[kidx[r]] (kidx None: one kernel).  Returns cc, res (nrows, m), iters, flags (nrows,), rms (nrows, 2), stats."""
        x = NP.ascontiguousarray(inp, dtype=NP.complex128)
        nrows, m = x.shape
        k, ix = self._clean_kernels(kern, kidx, nrows, m)
        box = NP.ascontiguousarray(cbox, dtype=NP.uint8).reshape(nrows, m)
        cc, res = NP.empty_like(x), NP.empty_like(x)
        iters, flags = NP.empty(nrows, dtype=NP.int32), NP.empty(nrows, dtype=NP.int32)
        rms = NP.empty((nrows, 2))
        st = PrisimCleanStats()
        self._call('prisim_clean_rows', nrows=nrows, m=m, inp=x, nkern=k.shape[0], kern=k, kidx=ix, cbox=box, gain=gain, maxiter=maxiter,
                   threshold=threshold, threshold_absolute=bool(absolute), cc=cc, res=res, iters=iters, flags=flags, rms=rms, stats=st)
        return cc, res, iters, flags, rms, _stats_dict(st, kernel_in_lds=bool)

    def clean_delay(self, win, kwin, cbox, m, lag_scale, freq_scale1, freq_scale2, gain, maxiter, threshold, absolute=False, kidx=None):
        """The delayClean chain (prisim_clean_delay) for win (ncubes, nrows, nchan) windowed rows zero-padded to m lags, kernels
        kwin (nkern, nchan), boxes cbox (nrows, m).  Returns a dict of lag, kern_lag, cc, res, cc_freq, res_freq (unshifted),
        iters, flags, rms and stats."""
        w = NP.ascontiguousarray(win, dtype=NP.complex128)
        ncubes, nrows, nchan = w.shape
        k, ix = self._clean_kernels(kwin, kidx, nrows, nchan)
        box = NP.ascontiguousarray(cbox, dtype=NP.uint8).reshape(nrows, m)
        out = {name: NP.empty((ncubes, nrows, m), dtype=NP.complex128) for name in ('lag', 'cc', 'res', 'cc_freq', 'res_freq')}
        out['kern_lag'] = NP.empty((k.shape[0], m), dtype=NP.complex128)
        out['iters'] = NP.empty((ncubes, nrows), dtype=NP.int32)
        out['flags'] = NP.empty((ncubes, nrows), dtype=NP.int32)
        out['rms'] = NP.empty((ncubes, nrows, 2))
        st = PrisimCleanStats()
        self._call('prisim_clean_delay', ncubes=ncubes, nrows=nrows, nchan=nchan, m=m, win=w, nkern=k.shape[0], kwin=k, kidx=ix, cbox=box,
                   lag_scale=lag_scale, freq_scale1=freq_scale1, freq_scale2=freq_scale2, gain=gain, maxiter=maxiter, threshold=threshold,
                   threshold_absolute=bool(absolute), stats=st, **out)
        out['stats'] = _stats_dict(st, kernel_in_lds=bool)
        return out

    # ---- sub-band delay spectra (include/prisim_subband.h) ----
    def subband_transform(self, cubes, bp, wts, m, df, nres=0, pscale=None, want=('over', 'res'), route='auto', nbl=None, t0=0, nt=None):
        """Sub-band delay spectra on the device (prisim_subband_transform).  cubes: (ncubes, nt, nbl, nchan) complex128 on the host, or
        None for the resident visibility slots [t0, t0 + nt) of this context; bp: (nbp, nchan) bandpass rows, nbp in (1, nbl, nt nbl);
        wts: (nwin, nchan) windows; m lags (zero padding), nres resampled lags; pscale (nwin,) for the power products.  want: any of
        'over', 'over_power', 'res', 'res_power'.  Returns a dict of the wanted outputs, shaped (ncubes, nt, nbl, nwin, m | nres), and
        'stats' (device_ms, kernel_ms, rows, route 'fused' | 'rocfft', lds_bytes)."""
        w = NP.ascontiguousarray(wts, dtype=NP.float64)
        w = w.reshape(-1, w.shape[-1])
        nwin, nchan = w.shape
        if cubes is None:
            x, ncubes, nbl = None, 1, self.nbl if nbl is None else int(nbl)
            if nt is None:
                raise ValueError('nt is required with resident input')
        else:
            x = NP.ascontiguousarray(cubes, dtype=NP.complex128)
            ncubes, nt, nbl = x.shape[0], x.shape[1], x.shape[2]
            if x.shape[3] != nchan:
                raise ValueError('cubes and wts must have the same channel count')
        b = NP.ascontiguousarray(bp, dtype=NP.float64).reshape(-1, nchan)
        flag = _want_bits(want, {'over': PRISIM_SUBBAND_OVER, 'over_power': PRISIM_SUBBAND_OVER_POWER, 'res': PRISIM_SUBBAND_RES,
                                 'res_power': PRISIM_SUBBAND_RES_POWER})
        ps = None if pscale is None else NP.ascontiguousarray(NP.broadcast_to(NP.asarray(pscale, dtype=NP.float64).ravel(), (nwin,)))
        out = {}
        for name in want:
            n = m if name.startswith('over') else max(int(nres), 1)
            out[name] = NP.empty((ncubes, nt, nbl, nwin, n), dtype=NP.complex128 if name in ('over', 'res') else NP.float64)
        nmap, mo, mi, mw = _resample_map(flag & (PRISIM_SUBBAND_RES | PRISIM_SUBBAND_RES_POWER) and 1 <= int(nres) <= PRISIM_SUBBAND_MAX_LEN,
                                         m, nres)
        st = PrisimSubbandStats()
        r = _route_code(route, SUBBAND_ROUTES)
        self._call('prisim_subband_transform', ncubes=ncubes, nt=nt, nbl=nbl, nchan=nchan, cubes=x, t0=t0, bp=b, nbp=b.shape[0], nwin=nwin,
                   wts=w, m=m, df=df, nres=nres, nmap=nmap, map_out=mo, map_in=mi, map_w=mw, pscale=ps, want=flag, route=r,
                   over=out.get('over'), over_pow=out.get('over_power'), res=out.get('res'), res_pow=out.get('res_power'), stats=st)
        out['stats'] = _stats_dict(st, route=SUBBAND_ROUTES)
        return out

    def subband_power_resident(self, t0, nt, bp, wts, m, df, pscale, nres=0, route='auto'):
        """Power-only sub-band spectra of the resident snapshots [t0, t0 + nt): |.|^2 * pscale[w] of the oversampled (and, with nres > 0,
        the resampled) spectra of the visibilities already in HBM.  No complex spectrum leaves the device and no visibility is uploaded.
        Returns (over_power (nt, nbl, nwin, m), res_power (nt, nbl, nwin, nres) or None, stats)."""
        want = ('over_power', 'res_power') if nres > 0 else ('over_power',)
        out = self.subband_transform(None, bp, wts, m, df, nres=nres, pscale=pscale, want=want, route=route, t0=t0, nt=nt)
        return out['over_power'][0], (out['res_power'][0] if nres > 0 else None), out['stats']

    # ---- delay spectra and power spectra of runs (include/prisim_runs.h) ----
    def runs_transform(self, vis, nbl, nchan, nt, bp=None, wts=None, win=None, m=None, scale=1.0, mode='all', nout=None, factor=1.0,
                       route='auto', budget_bytes=RUNS_BUDGET):
        """Delay spectra of a stack of runs on the device (prisim_runs_transform).  vis: (R, nbl, nchan, nt) complex128 or complex64 on
        the host (any leading shape whose product is R; not copied when C-contiguous), or None for unit visibilities (R = 1, the lag
        kernel); bp, wts: None or float64 arrays broadcastable to (nbl, nchan, nt), passed with their broadcast strides (nothing dense
        is formed); win: None or (nwin, nchan) windows.  spectrum = scale fftshift(ifft(((vis bp) wts) win, m)); mode 'all' (m lags),
        'interp' (nout positions j * factor, linearly interpolated) or 'resample' (scipy.signal.resample to nout lags).  The call is
        streamed in chunks of (run, baseline) pairs within budget_bytes of device memory.  Returns (out (nwin, R, nbl, nout, nt)
        complex128, stats)."""
        nbl, nchan, nt = int(nbl), int(nchan), int(nt)
        m = nchan if m is None else int(m)
        if vis is None:
            x, R, c64 = None, 1, 0
        else:
            x = NP.asarray(vis)
            if x.dtype not in (NP.complex128, NP.complex64):
                x = x.astype(NP.complex128)
            x = NP.ascontiguousarray(x)
            if x.ndim < 3 or x.shape[-3:] != (nbl, nchan, nt):
                raise ValueError('vis must be (..., nbl, nchan, nt) = (..., %d, %d, %d)' % (nbl, nchan, nt))
            R, c64 = int(NP.prod(x.shape[:-3], dtype=NP.int64)), int(x.dtype == NP.complex64)
        weights = []
        for w in (bp, wts):                     # the broadcast view's strides over the contiguous array's own memory (0: broadcast)
            if w is None:
                weights.append((None, None))
                continue
            src = NP.ascontiguousarray(w, dtype=NP.float64)
            if src.ndim > 3:
                raise ValueError('weights broadcast over (nbl, nchan, nt) only')
            view = NP.broadcast_to(src, (nbl, nchan, nt))
            weights.append((src, NP.array([s // 8 for s in view.strides], dtype=NP.int64)))
        if win is not None:
            wn = NP.ascontiguousarray(win, dtype=NP.float64).reshape(-1, nchan)
            nwin = wn.shape[0]
        else:
            wn, nwin = None, 1
        modes = {'all': PRISIM_RUNS_ALL, 'interp': PRISIM_RUNS_INTERP, 'resample': PRISIM_RUNS_RESAMPLE}
        md = modes[mode]
        nout = m if md == PRISIM_RUNS_ALL else int(nout)
        nmap, mo, mi, mw = _resample_map(md == PRISIM_RUNS_RESAMPLE and 1 <= nout <= PRISIM_RUNS_MAX_LEN and 1 <= m <= PRISIM_RUNS_MAX_LEN,
                                         m, nout)
        out = NP.empty((nwin, R, nbl, max(nout, 1), nt), dtype=NP.complex128)
        st = PrisimRunsStats()
        r = {'auto': PRISIM_RUNS_AUTO, 'fused': PRISIM_RUNS_FUSED, 'rocfft': PRISIM_RUNS_ROCFFT}[route]      # 'direct' is not the caller's to ask for
        (bpa, bps), (wa, wss) = weights
        self._call('prisim_runs_transform', R=R, nbl=nbl, nchan=nchan, nt=nt, vis=x, vis_is_c64=c64, bp=bpa, bp_strides=bps, wts=wa,
                   wts_strides=wss, nwin=nwin, win=wn, m=m, scale=scale, out_mode=md, nout=nout, factor=factor, nmap=nmap, map_out=mo,
                   map_in=mi, map_w=mw, route=r, budget_bytes=budget_bytes, out=out, stats=st)
        return out, _stats_dict(st, route=RUNS_ROUTES)

    def runs_power(self, vislag1, vislag2=None, factor=1.0, cross=False, budget_bytes=RUNS_BUDGET):
        """(vislag1 * vislag2.conj() * factor).real (* 2 when cross) on the device (prisim_runs_power), rounded as numpy rounds it on
        this host.  vislag1 / vislag2: same-shape complex128 or complex64 host arrays (vislag2 None: vislag1); factor: a scalar or one
        value per index of the leading axis.  Returns (power float64 of vislag1's shape, stats)."""
        v1 = NP.asarray(vislag1)
        dt = NP.result_type(v1, NP.asarray(vislag2) if vislag2 is not None else v1)
        if dt not in (NP.complex128, NP.complex64):
            dt = NP.complex128
        v1 = NP.ascontiguousarray(v1, dtype=dt)
        v2 = None if vislag2 is None else NP.ascontiguousarray(vislag2, dtype=dt)
        if v2 is not None and v2.shape != v1.shape:
            raise ValueError('vislag1 and vislag2 must have the same shape')
        f = NP.ascontiguousarray(NP.asarray(factor, dtype=NP.float64).ravel())
        n = int(v1.size)
        if f.size == 1:
            nf, inner = 1, max(n, 1)
        elif v1.ndim >= 1 and f.size == v1.shape[0]:
            nf, inner = f.size, max(n // max(f.size, 1), 1)
        else:
            raise ValueError('factor must be a scalar or have one value per index of the leading axis')
        out = NP.empty(v1.shape, dtype=NP.float64)
        st = PrisimRunsStats()
        if n == 0:
            return out, _stats_dict(st, route=RUNS_ROUTES)
        self._call('prisim_runs_power', nf=nf, inner=inner, v1=v1, v2=v2, is_c64=dt == NP.complex64, factor=f, cross=bool(cross),
                   fused_product=numpy_fuses_complex_product(dt), budget_bytes=budget_bytes, out=out, stats=st)
        return out, _stats_dict(st, route=RUNS_ROUTES)

    # ---- closure phases of antenna triads (include/prisim_closure.h) ----
    def closure_phase(self, cube, legs, conj, bpwts, freq_wts=None, masks=None, mask_index=None, nt=None, route='auto',
                      budget_bytes=CLOSURE_BUDGET):
        """Visibility triplets and closure phases of antenna triads on the device (prisim_closure_phase).  cube: (nbl, nchan, nt)
        complex128 on the host, or None for the resident visibility slots [0, nt) of this context; legs, conj: (ntriads, 3) cube rows
        and conjugation flags of the legs 12, 23, 31; bpwts: bp * bp_wts, broadcastable to (nbl, nchan, nt); freq_wts: (nchan,) or a
        scalar (None: ones); masks: None (no delay filter) or (nmask, nchan) filter_unmask vectors on the unshifted FFT delay axis, with
        mask_index (nbl,) the mask of each cube row (None: mask 0).  The outputs are streamed in chunks of triads within budget_bytes
        of device memory; an uploaded cube (16 B per element) and the dense bpwts (8 B per element of (nbl, nchan, nt), also when bp is
        constant in time) lie on the device for the call on top of that budget.  Returns (triplets (ntriads, 3, nchan, nt) complex128, phases (ntriads, nchan, nt) float64, stats); stats['resident']: the resident cube was read."""
        if cube is None:
            if nt is None:
                raise ValueError('nt is required with resident input')
            x, nbl, nchan, nt = None, self.nbl, self.nchan, int(nt)
        else:
            x = NP.ascontiguousarray(cube, dtype=NP.complex128)
            if x.ndim != 3:
                raise ValueError('cube must be (nbl, nchan, nt)')
            nbl, nchan, nt = x.shape
        lg, cj, bw, fw, mk, mi = _closure_inputs(legs, conj, bpwts, freq_wts, masks, mask_index, nbl, nchan, nt)
        ntriads = lg.shape[0]
        trip = NP.empty((ntriads, 3, nchan, nt), dtype=NP.complex128)
        phase = NP.empty((ntriads, nchan, nt), dtype=NP.float64)
        st = PrisimClosureStats()
        r = _route_code(route, CLOSURE_ROUTES)
        self._call('prisim_closure_phase', cube=x, nt=nt, nbl=nbl, nchan=nchan, legs=lg, conj=cj, ntriads=ntriads, freq_wts=fw, bpwts=bw,
                   masks=mk, nmask=0 if mk is None else mk.shape[0], mask_index=mi, route=r, budget_bytes=budget_bytes,
                   out_triplets=trip, out_phase=phase, stats=st)
        return trip, phase, dict(_stats_dict(st, route=CLOSURE_ROUTES), resident=x is None)

    # ---- closure phases of noise realisations (include/prisim_cpreal.h) ----
    PrisimCprealStats = _PrisimCprealStats

    def closure_realizations(self, cube, cube_row, bl_global, rms, bpwts, legs, conj, seed, n_realize, first=0, kind='noisy', nt=None,
                             route='auto', budget_bytes=CLOSURE_BUDGET):
        """Closure phases of n_realize thermal-noise realisations, drawn and closed on the device (prisim_closure_realizations).
        cube: (nt, nrow, nchan) complex128 on the host, the visibilities of the used rows; or None for the resident visibility slots
        [0, nt) of this context, of which cube_row (nrow,) names the rows.  bl_global: (nrow,) the global baseline index of each used
        row, the counter of the draw as in noise(bl_index=...); rms: the noise rms and bpwts: bp * bp_wts, each broadcastable to (nt,
        nrow, nchan); legs, conj: (ntriads, 3) used rows and conjugation flags of the legs 12, 23, 31.  Realisation r is drawn under
        the key seed + first + r; kind: 'noisy' (the visibilities with the noise added) or 'noise'; route: 'auto', 'direct' or
        'staged'.  The output is streamed in chunks of (snapshot, realisation) pairs within budget_bytes of device memory; the
        uploaded rows lie on the device for the call on top of that budget.  Returns (phases (nt, n_realize, ntriads, nchan) float64,
        stats); stats['resident']: the resident cube was read."""
        ix = NP.ascontiguousarray(bl_global, dtype=NP.int64).ravel()
        nrow = ix.size
        if cube is None:
            if nt is None or cube_row is None:
                raise ValueError('nt and cube_row are required with resident input')
            x, nchan, nt = None, self.nchan, int(nt)
            cr = NP.ascontiguousarray(cube_row, dtype=NP.int32).ravel()
            if cr.size != nrow:
                raise ValueError('cube_row and bl_global must have one entry per used row')
        else:
            x = NP.ascontiguousarray(cube, dtype=NP.complex128)
            if x.ndim != 3 or x.shape[1] != nrow:
                raise ValueError('cube must be (nt, nrow, nchan) with one row per entry of bl_global')
            nt, _, nchan = x.shape
            cr = None
        lg = NP.ascontiguousarray(legs, dtype=NP.int32).reshape(-1, 3)
        cj = NP.ascontiguousarray(conj, dtype=NP.int32).reshape(-1, 3)
        if cj.shape != lg.shape:
            raise ValueError('legs and conj must both be (ntriads, 3)')
        rm = NP.ascontiguousarray(NP.broadcast_to(NP.asarray(rms, dtype=NP.float64), (nt, nrow, nchan)))
        bw = NP.ascontiguousarray(NP.broadcast_to(NP.asarray(bpwts, dtype=NP.float64), (nt, nrow, nchan)))
        if kind not in CPREAL_KINDS:
            raise ValueError("kind must be 'noisy' or 'noise'")
        n_realize, ntriads = int(n_realize), lg.shape[0]
        out = NP.empty((nt, max(n_realize, 0), ntriads, nchan), dtype=NP.float64)
        st = self.PrisimCprealStats()
        self._call('prisim_closure_realizations', cube=x, cube_row=cr, bl_global=ix, nt=nt, nrow=nrow, nchan=nchan, rms=rm, bpwts=bw, legs=lg,
                   conj=cj, ntriads=ntriads, seed=int(seed) & 0xFFFFFFFFFFFFFFFF, first=first, n_realize=n_realize, kind=CPREAL_KINDS[kind],
                   route=_route_code(route, CPREAL_ROUTES), budget_bytes=budget_bytes, out_phase=out, stats=st)
        return out, dict(_stats_dict(st, route=CPREAL_ROUTES), resident=x is None)

    # ---- beam-weighted sky power per snapshot (include/prisim_antpower.h) ----
    PrisimAntpowerStats = _PrisimAntpowerStats
    PrisimAntpowerArgs = _PrisimAntpowerArgs

    def antenna_power(self, unitvec, freqs_hz, cel2enu, beam_kind, diameter_m, beam_pc_dircos=(0.0, 0.0, 1.0), flux_ref=None, spindex=None,
                      ref_freq_hz=None, flux_spectrum=None, aberr_beta=None, ext=None, budget_bytes=0, want_sums=True):
        """The power an antenna receives from the sky, sum_s pb S / sum_s pb over the sources above the horizon, per snapshot and
        channel on the device (prisim_antenna_power).  unitvec: (nsrc, 3) unit vectors in the catalogue's frame
        (geometry.catalog_unitvec); freqs_hz: (nchan,); cel2enu: (nsnap, 3, 3) rotations catalogue frame -> East-North-Up and
        aberr_beta: (nsnap, 3) or None, as prisim_amd.frames.snapshot_frame gives them.  The flux is the power law flux_ref (f /
        ref_freq_hz)^spindex, evaluated on the device, or the table flux_spectrum (nsrc, nchan).  The beam is that of set_sky_analytic:
        beam_kind, diameter_m, beam_pc_dircos and ext, a dict (make_beam_ext), None, or a sequence of one dict per snapshot.
        budget_bytes: device bytes of the streamed buffers (0: 1 GiB); the result does not depend on it.  Returns (power, num, den,
        stats), each array (nsnap, nchan) float64; num and den are None without want_sums.  A snapshot with nothing above the horizon
        is NaN in power."""
        uv = NP.ascontiguousarray(unitvec, dtype=NP.float64).reshape(-1, 3)
        fq = NP.ascontiguousarray(freqs_hz, dtype=NP.float64).ravel()
        rot = NP.ascontiguousarray(cel2enu, dtype=NP.float64).reshape(-1, 9)
        nsrc, nchan, nsnap = uv.shape[0], fq.size, rot.shape[0]
        ab = None
        if aberr_beta is not None:
            ab = NP.ascontiguousarray(aberr_beta, dtype=NP.float64).reshape(-1, 3)
            if ab.shape[0] != nsnap:
                raise ValueError('aberr_beta must have one row per snapshot')
        fs = fr = sp = None
        if flux_spectrum is not None:
            fs = NP.ascontiguousarray(flux_spectrum, dtype=NP.float64)
            if fs.shape != (nsrc, nchan):
                raise ValueError('flux_spectrum must have shape (nsrc, nchan)')
        elif flux_ref is not None and spindex is not None:
            fr = NP.ascontiguousarray(flux_ref, dtype=NP.float64).ravel()
            sp = NP.ascontiguousarray(spindex, dtype=NP.float64).ravel()
            if fr.size != nsrc or sp.size != nsrc:
                raise ValueError('flux_ref and spindex must have nsrc elements')
        exts, xs, keep = _beam_ext_array(ext)
        a = self.PrisimAntpowerArgs()
        a.nsrc, a.nchan, a.nsnap = nsrc, nchan, nsnap
        a.unitvec, a.flux_ref, a.spindex, a.flux_spectrum = _ptr(uv), _ptr(fr), _ptr(sp), _ptr(fs)
        a.ref_freq_hz = 0.0 if ref_freq_hz is None else float(ref_freq_hz)
        a.freqs_hz, a.cel2enu, a.aberr_beta = _ptr(fq), _ptr(rot), _ptr(ab)
        a.beam_kind, a.diameter_m = int(beam_kind), float(diameter_m)
        bpc = NP.asarray(beam_pc_dircos, dtype=NP.float64).ravel()
        if bpc.size != 3:
            raise ValueError('beam_pc_dircos must have 3 elements')
        a.beam_pc_dircos[:] = bpc.tolist()
        a.ext = C.cast(xs, C.c_void_p) if exts else None
        a.n_ext = len(exts)
        a.budget_bytes = int(budget_bytes or 0)
        power = NP.empty((nsnap, nchan), dtype=NP.float64)
        num = NP.empty((nsnap, nchan), dtype=NP.float64) if want_sums else None
        den = NP.empty((nsnap, nchan), dtype=NP.float64) if want_sums else None
        st = self.PrisimAntpowerStats()
        self._call('prisim_antenna_power', a=a, out_power=power, out_num=num, out_den=den, stats=st)
        return power, num, den, _stats_dict(st)

    # ---- dirty images and synthesized beams by the direct Fourier sum (include/prisim_imaging.h) ----
    PrisimImagingStats = _PrisimImagingStats
    PrisimImagingArgs = _PrisimImagingArgs

    def dirty_image(self, unitvec, rot, pc_dircos, baselines, freqs_hz, cube=None, weights=None, kind='dirty', chan_avg=False,
                    aberr_beta=None, route='auto', budget_bytes=0, precision='double'):
        """The dirty image (kind 'dirty') or the synthesized beam ('psf') at the given directions by the direct Fourier sum on the
        device (prisim_dirty_image): D[p][k] = sum_t sum_b w Re(V e^{+i phi}), phi = 2 pi f_k b . (s - s0) / c, over W[k] = sum w.
        unitvec: (npix, 3) unit vectors of the directions in their own frame (geometry.catalog_unitvec); rot: (nt, 3, 3) rotations of
        that frame into East-North-Up and aberr_beta: (nt, 3) or None, as prisim_amd.frames.snapshot_frame gives them; pc_dircos:
        (nt, 3) East-North-Up phase centres; baselines: (nbl, 3) metres; freqs_hz: (nchan,).  cube: (nt, nbl, nchan) complex128 on the
        host, or None for the resident visibility slots [0, nt) of this context; not read for the PSF.  weights: None, (nbl,) or (nt,
        nbl, nchan), finite and non-negative.  chan_avg: one image of the band instead of one per channel.  route: 'auto', 'direct'
        or 'stepped'; budget_bytes: device bytes of the streamed buffers (0: 1 GiB), which the result does not depend on.  Returns
        (image (npix, nchan) or (npix,), wsum (nchan,) or (1,), stats); a zero weight sum is NaN in the image; stats['resident']: the
        resident cube was read.  precision: 'double', or 'single' for the fp32 route (prisim_dirty_image_f32,
        include/prisim_imaging32.h): the phases fp64, the phasors and partial sums fp32, within 5e-6 of the scale; it takes a uniform
        grid and route 'auto' or 'stepped'.  stats['precision'] says which ran."""
        if kind not in IMAGING_KINDS:
            raise ValueError("kind must be 'dirty' or 'psf'")
        if precision not in IMAGING_PRECISIONS:
            raise ValueError("precision must be 'double' or 'single'")
        a = self.PrisimImagingArgs()
        npix, _, nchan, _, resident, keep = _imaging_inputs(a, unitvec, rot, pc_dircos, baselines, freqs_hz, cube if kind == 'dirty' else None,
                                                            weights, chan_avg, aberr_beta, route, budget_bytes)
        a.kind = IMAGING_KINDS[kind]
        image = NP.empty((npix,) if chan_avg else (npix, nchan), dtype=NP.float64)
        wsum = NP.empty(1 if chan_avg else nchan, dtype=NP.float64)
        st = self.PrisimImagingStats()
        self._call(IMAGING_PRECISIONS[precision], a=a, out_image=image, out_wsum=wsum, stats=st)
        del keep
        return image, wsum, dict(_stats_dict(st, route=IMAGING_ROUTES), resident=resident and kind == 'dirty', precision=precision)

    # ---- beam-weighted mosaics of the snapshots (include/prisim_mosaic.h) ----
    PrisimMosaicStats = _PrisimMosaicStats
    PrisimMosaicArgs = _PrisimMosaicArgs

    def mosaic_image(self, unitvec, rot, pc_dircos, baselines, freqs_hz, beam_kind, diameter_m, beam_pc_dircos=(0.0, 0.0, 1.0), ext=None,
                     cube=None, weights=None, chan_avg=False, aberr_beta=None, pbmin=0.1, route='auto', budget_bytes=0, want_sums=True,
                     precision='double'):
        """The beam-weighted linear mosaic of the snapshots at the given directions on the device (prisim_mosaic_image):
        sum_t A_t D_t / sum_t A_t^2 W_t with D_t the direct Fourier sum of snapshot t (dirty_image), W_t its weight sum and A_t the
        power pattern of the primary beam at the direction in that snapshot, 0 below the horizon.  The geometry, cube, weights,
        chan_avg, route and budget_bytes as dirty_image takes them; the beam as antenna_power takes it: beam_kind, diameter_m,
        beam_pc_dircos -- (3,), or (nt, 3) for an element pointing that moves from snapshot to snapshot -- and ext, a dict
        (make_beam_ext), None, or a sequence of one dict per snapshot.  pbmin in [0, 1): a pixel whose
        effective beam sqrt(Q / Wtot) is below it is NaN; 0 masks only Q == 0.  Returns (mosaic (npix, nchan) or (npix,), num, den
        (npix, nchan) -- None without want_sums --, wsum (nchan,), stats); stats['pb_eff'] is the effective beam in the shape of the
        mosaic and stats['resident'] whether the resident cube was read.  precision: 'double', or 'single' for the fp32 route
        (prisim_mosaic_image_f32, include/prisim_mosaic32.h): every D_t formed as dirty_image forms it with precision='single', the
        beam, the weight sums and the sums over t still fp64, so that den, wsum, pb_eff and the NaN positions have the bits of
        'double' and num is within 5e-6 sum_t A_t sum_b w|V| of it; it takes a uniform grid and route 'auto' or 'stepped'.
        stats['precision'] says which ran."""
        if precision not in MOSAIC_PRECISIONS:
            raise ValueError("precision must be 'double' or 'single'")
        a = self.PrisimMosaicArgs()
        npix, _, nchan, nt, resident, keep = _imaging_inputs(a, unitvec, rot, pc_dircos, baselines, freqs_hz, cube, weights, chan_avg, aberr_beta,
                                                             route, budget_bytes)
        keep_ext = _mosaic_beam_fields(a, nt, beam_kind, diameter_m, beam_pc_dircos, ext, pbmin)
        shape = (npix,) if chan_avg else (npix, nchan)
        mosaic, pb_eff = NP.empty(shape, dtype=NP.float64), NP.empty(shape, dtype=NP.float64)
        num = NP.empty((npix, nchan), dtype=NP.float64) if want_sums else None
        den = NP.empty((npix, nchan), dtype=NP.float64) if want_sums else None
        wsum = NP.empty(nchan, dtype=NP.float64)
        st = self.PrisimMosaicStats()
        self._call(MOSAIC_PRECISIONS[precision], a=a, out_mosaic=mosaic, out_pb_eff=pb_eff, out_num=num, out_den=den, out_wsum=wsum, stats=st)
        del keep, keep_ext
        return mosaic, num, den, wsum, dict(_stats_dict(st, route=IMAGING_ROUTES), resident=resident, pb_eff=pb_eff, precision=precision)

    # ---- Hogbom CLEAN of dirty images with the exact beam (include/prisim_imclean.h) ----
    PrisimImcleanStats = _PrisimImcleanStats
    PrisimImcleanArgs = _PrisimImcleanArgs

    def clean_image(self, unitvec, rot, pc_dircos, baselines, freqs_hz, cube=None, weights=None, chan_avg=False, aberr_beta=None,
                    gain=0.1, maxiter=10000, threshold=5e-3, threshold_relative=True, window=None, fwhm_rad=None, route='auto',
                    budget_bytes=0, poll_every=0):
        """Hogbom CLEAN of the dirty image of dirty_image(kind='dirty') with the exact beam on the device (prisim_clean_image): per
        image channel (one for the band with chan_avg) and iteration, the largest |residual| inside the window becomes a component of
        gain times its value, and the dirty image of that component's own visibilities is subtracted from every pixel.  The
        geometry, cube and weights as dirty_image takes them.  gain in (0, 1]; maxiter >= 0 components per channel at most; threshold
        finite and >= 0, a fraction (< 1) of the first peak with threshold_relative; window: (npix,) of pixels that may hold
        components, or None for all; fwhm_rad: a scalar or (nc,) restoring beam in radians, or None for no restoration; budget_bytes:
        device bytes the resident image may take (0: 1 GiB); poll_every: iterations between two reads of the active count (0: 32),
        which no result depends on.  Returns a dict: 'residual' and 'restored' (or None) (npix, nchan) or (npix,); 'comp_pixel' int32
        and 'comp_flux' (nc, longest list), the unused tail of a row -1 and 0; 'ncomp', 'status' (PRISIM_IMCLEAN_* bits) int32 and
        'peak0', 'wsum' (nc,); and the stats dict."""
        a = self.PrisimImcleanArgs()
        npix, _, nchan, _, resident, keep = _imaging_inputs(a, unitvec, rot, pc_dircos, baselines, freqs_hz, cube, weights, chan_avg, aberr_beta,
                                                            route, budget_bytes)
        nc = 1 if chan_avg else nchan
        maxiter, win, fw = _clean_fields(a, npix, nc, gain, maxiter, threshold, threshold_relative, window, fwhm_rad, poll_every)
        out = _clean_outputs(npix, nchan, nc, maxiter, chan_avg, fw is not None)
        wsum = NP.empty(nc, dtype=NP.float64)
        st = self.PrisimImcleanStats()
        self._call('prisim_clean_image', a=a, out_wsum=wsum, stats=st, **out)
        del keep, win, fw
        return dict(_clean_result(out), wsum=wsum, stats=dict(_stats_dict(st, route=IMAGING_ROUTES), resident=resident))

    # ---- Cotton-Schwab CLEAN of dirty images (include/prisim_csclean.h) ----
    PrisimCscleanStats = _PrisimCscleanStats
    PrisimCscleanArgs = _PrisimCscleanArgs

    def clean_image_cs(self, unitvec, grid_shape, rot, pc_dircos, baselines, freqs_hz, cube=None, weights=None, chan_avg=False, aberr_beta=None,
                       gain=0.1, maxiter=10000, threshold=5e-3, threshold_relative=True, cycle_depth=0.3, cycle_niter=0, max_major=32,
                       window=None, fwhm_rad=None, route='auto', minor_route='auto', budget_bytes=0, want_psf=False, want_vis=False):
        """Cotton-Schwab CLEAN of the dirty image of dirty_image(kind='dirty') on the device (prisim_clean_image_cs): minor cycles on
        one image channel with the shift-invariant beam P of the lattice grid_shape = (ny, nx) (ny * nx = npix, nx fastest), each
        down to cycle_depth of its first peak or cycle_niter components (0: no cap), and after each a major cycle that takes the new
        components out of the residual visibilities and images those again, max_major at most.  The geometry, cube, weights, gain,
        maxiter, threshold, threshold_relative, window, fwhm_rad, route and budget_bytes as clean_image takes them; minor_route:
        'auto', 'lds' or 'global', where the working image of a minor cycle lives, which no result depends on.  Returns the dict of
        clean_image -- 'status' may also hold PRISIM_CSCLEAN_MAJOR or _DIVERGED -- with 'ncycles' (nc,) int32, 'cycle_ncomp' int32
        (nc, most cycles; -1 past a channel's own), 'cycle_peak' (nc, most cycles + 1; NaN past a channel's own), 'psf' (nc, 2 ny - 1,
        2 nx - 1) with want_psf and 'vres' (nt, nbl, nchan) complex128 with want_vis, else None."""
        a = self.PrisimCscleanArgs()
        npix, nbl, nchan, nt, resident, keep = _imaging_inputs(a, unitvec, rot, pc_dircos, baselines, freqs_hz, cube, weights, chan_avg,
                                                               aberr_beta, route, budget_bytes)
        nc = 1 if chan_avg else nchan
        maxiter, win, fw = _clean_fields(a, npix, nc, gain, maxiter, threshold, threshold_relative, window, fwhm_rad, None)
        ny, nx = (int(n) for n in grid_shape)
        a.ny, a.nx, a.cycle_depth, a.cycle_niter, a.max_major = ny, nx, float(cycle_depth), int(cycle_niter or 0), int(max_major)
        a.minor_route = _route_code(minor_route, CSCLEAN_ROUTES)
        out = _clean_outputs(npix, nchan, nc, maxiter, chan_avg, fw is not None)
        cyc = max(int(max_major), 0)
        ncycles, wsum = NP.empty(nc, dtype=NP.int32), NP.empty(nc, dtype=NP.float64)
        cycle_ncomp = NP.full((nc, cyc), -1, dtype=NP.int32)
        cycle_peak = NP.full((nc, cyc + 1), NP.nan, dtype=NP.float64)
        psf = NP.empty((nc, max(2 * ny - 1, 0), max(2 * nx - 1, 0)), dtype=NP.float64) if want_psf else None
        vres = NP.empty((nt, nbl, nchan), dtype=NP.complex128) if want_vis else None
        st = self.PrisimCscleanStats()
        self._call('prisim_clean_image_cs', a=a, out_wsum=wsum, out_ncycles=ncycles, out_cycle_ncomp=cycle_ncomp, out_cycle_peak=cycle_peak,
                   out_psf=psf, out_vres=vres, stats=st, **out)
        del keep, win, fw
        most = int(ncycles.max()) if nc else 0
        return dict(_clean_result(out), wsum=wsum, ncycles=ncycles, cycle_ncomp=NP.ascontiguousarray(cycle_ncomp[:, :most]),
                    cycle_peak=NP.ascontiguousarray(cycle_peak[:, :most + 1]), psf=psf, vres=vres,
                    stats=dict(_stats_dict(st, route=IMAGING_ROUTES, minor_route=CSCLEAN_ROUTES), resident=resident))

    # ---- CLEAN of the beam-weighted mosaic (include/prisim_mosclean.h) ----
    PrisimMoscleanStats = _PrisimMoscleanStats
    PrisimMoscleanArgs = _PrisimMoscleanArgs

    def clean_mosaic(self, unitvec, rot, pc_dircos, baselines, freqs_hz, beam_kind, diameter_m, beam_pc_dircos=(0.0, 0.0, 1.0), ext=None,
                     cube=None, weights=None, chan_avg=False, aberr_beta=None, pbmin=0.1, gain=0.1, maxiter=10000, threshold=5e-3,
                     threshold_relative=True, window=None, fwhm_rad=None, route='auto', budget_bytes=0, poll_every=0):
        """CLEAN of the beam-weighted mosaic of mosaic_image on the device (prisim_clean_mosaic): per image channel (one for the band
        with chan_avg) and iteration, the pixel of the largest |F| inside the window and the mask, F = R_N / sqrt(Q Wtot) the flat-noise
        image, becomes a component of the true flux gain * R_N / Q there, and what the beam-weighted snapshots show of that component's
        own visibilities is subtracted from the numerator R_N of every pixel.  The geometry, cube, weights and the beam as mosaic_image
        takes them; gain, maxiter, threshold (in the units of F), threshold_relative, window, fwhm_rad, budget_bytes and poll_every as
        clean_image takes them.  Returns a dict: 'residual' (R_N / Q under the mask, true fluxes), 'restored' (or None),
        'residual_flat' (F) and 'pb_eff', (npix, nchan) or (npix,); 'num' (the final R_N) and 'den' (Q) (npix, nchan); 'wsum'
        (nchan,); 'comp_pixel' int32 and 'comp_flux' (nc, longest list), the unused tail of a row -1 and 0; 'ncomp', 'status'
        (PRISIM_IMCLEAN_* bits) int32 and 'peak0' (nc,); and the stats dict."""
        a = self.PrisimMoscleanArgs()
        npix, _, nchan, nt, resident, keep = _imaging_inputs(a, unitvec, rot, pc_dircos, baselines, freqs_hz, cube, weights, chan_avg, aberr_beta,
                                                             route, budget_bytes)
        keep_ext = _mosaic_beam_fields(a, nt, beam_kind, diameter_m, beam_pc_dircos, ext, pbmin)
        nc = 1 if chan_avg else nchan
        maxiter, win, fw = _clean_fields(a, npix, nc, gain, maxiter, threshold, threshold_relative, window, fwhm_rad, poll_every)
        out = _clean_outputs(npix, nchan, nc, maxiter, chan_avg, fw is not None)
        flat, pb_eff = NP.empty_like(out['out_residual']), NP.empty_like(out['out_residual'])
        num, den = NP.empty((npix, nchan), dtype=NP.float64), NP.empty((npix, nchan), dtype=NP.float64)
        wsum = NP.empty(nchan, dtype=NP.float64)
        st = self.PrisimMoscleanStats()
        self._call('prisim_clean_mosaic', a=a, out_residual_flat=flat, out_pb_eff=pb_eff, out_num=num, out_den=den, out_wsum=wsum, stats=st, **out)
        del keep, keep_ext, win, fw
        return dict(_clean_result(out), residual_flat=flat, pb_eff=pb_eff, num=num, den=den, wsum=wsum,
                    stats=dict(_stats_dict(st, route=IMAGING_ROUTES), resident=resident))

    # ---- Cotton-Schwab CLEAN of the beam-weighted mosaic (include/prisim_moscs.h) ----
    PrisimMoscsStats = _PrisimMoscsStats
    PrisimMoscsArgs = _PrisimMoscsArgs

    def clean_mosaic_cs(self, unitvec, grid_shape, rot, pc_dircos, baselines, freqs_hz, beam_kind, diameter_m, beam_pc_dircos=(0.0, 0.0, 1.0),
                        ext=None, cube=None, weights=None, chan_avg=False, aberr_beta=None, pbmin=0.1, gain=0.1, maxiter=10000, threshold=5e-3,
                        threshold_relative=True, cycle_depth=0.3, cycle_niter=0, max_major=32, window=None, fwhm_rad=None, route='auto',
                        minor_route='auto', budget_bytes=0, want_psf=False, want_vis=False):
        """Cotton-Schwab CLEAN of the beam-weighted mosaic of mosaic_image on the device (prisim_clean_mosaic_cs): where clean_mosaic
        pays a mosaic pass per component, this pays one per major cycle.  A minor cycle cleans the flat-noise image F of one image
        channel with the shift-invariant beam P of the lattice grid_shape = (ny, nx) (ny * nx = npix, nx fastest), down to cycle_depth
        of its first peak or cycle_niter components (0: no cap), each component listed with its true flux; the major cycle then takes
        the new components out of the residual visibilities through the beam of every snapshot and forms the mosaic's numerator of
        those again, max_major times at most.  The geometry, cube, weights and the beam as mosaic_image takes them; pbmin, gain,
        maxiter, threshold (in the units of F), threshold_relative, window, fwhm_rad, route and budget_bytes as clean_mosaic takes
        them; cycle_depth, cycle_niter, max_major and minor_route as clean_image_cs takes them.  Returns the dict of clean_mosaic --
        'status' may also hold PRISIM_CSCLEAN_MAJOR or _DIVERGED -- with 'ncycles' (nc,) int32, 'cycle_ncomp' int32 (nc, most cycles;
        -1 past a channel's own), 'cycle_peak' (nc, most cycles + 1; NaN past a channel's own), 'psf' (nc, 2 ny - 1, 2 nx - 1) with
        want_psf and 'vres' (nt, nbl, nchan) complex128 with want_vis, else None; 'num' is the mosaic's numerator of 'vres'."""
        a = self.PrisimMoscsArgs()
        npix, nbl, nchan, nt, resident, keep = _imaging_inputs(a, unitvec, rot, pc_dircos, baselines, freqs_hz, cube, weights, chan_avg,
                                                               aberr_beta, route, budget_bytes)
        keep_ext = _mosaic_beam_fields(a, nt, beam_kind, diameter_m, beam_pc_dircos, ext, pbmin)
        nc = 1 if chan_avg else nchan
        maxiter, win, fw = _clean_fields(a, npix, nc, gain, maxiter, threshold, threshold_relative, window, fwhm_rad, None)
        ny, nx = (int(n) for n in grid_shape)
        a.ny, a.nx, a.cycle_depth, a.cycle_niter, a.max_major = ny, nx, float(cycle_depth), int(cycle_niter or 0), int(max_major)
        a.minor_route = _route_code(minor_route, CSCLEAN_ROUTES)
        out = _clean_outputs(npix, nchan, nc, maxiter, chan_avg, fw is not None)
        flat, pb_eff = NP.empty_like(out['out_residual']), NP.empty_like(out['out_residual'])
        num, den = NP.empty((npix, nchan), dtype=NP.float64), NP.empty((npix, nchan), dtype=NP.float64)
        wsum = NP.empty(nchan, dtype=NP.float64)
        cyc = max(int(max_major), 0)
        ncycles = NP.empty(nc, dtype=NP.int32)
        cycle_ncomp = NP.full((nc, cyc), -1, dtype=NP.int32)
        cycle_peak = NP.full((nc, cyc + 1), NP.nan, dtype=NP.float64)
        psf = NP.empty((nc, max(2 * ny - 1, 0), max(2 * nx - 1, 0)), dtype=NP.float64) if want_psf else None
        vres = NP.empty((nt, nbl, nchan), dtype=NP.complex128) if want_vis else None
        st = self.PrisimMoscsStats()
        self._call('prisim_clean_mosaic_cs', a=a, out_residual_flat=flat, out_pb_eff=pb_eff, out_num=num, out_den=den, out_wsum=wsum,
                   out_ncycles=ncycles, out_cycle_ncomp=cycle_ncomp, out_cycle_peak=cycle_peak, out_psf=psf, out_vres=vres, stats=st, **out)
        del keep, keep_ext, win, fw
        most = int(ncycles.max()) if nc else 0
        return dict(_clean_result(out), residual_flat=flat, pb_eff=pb_eff, num=num, den=den, wsum=wsum, ncycles=ncycles,
                    cycle_ncomp=NP.ascontiguousarray(cycle_ncomp[:, :most]), cycle_peak=NP.ascontiguousarray(cycle_peak[:, :most + 1]),
                    psf=psf, vres=vres, stats=dict(_stats_dict(st, route=IMAGING_ROUTES, minor_route=CSCLEAN_ROUTES), resident=resident))

    # ---- delay spectra of closure phases and their power spectra (include/prisim_cpdelay.h) ----
    def closure_delay_spectra(self, wts, m, df, phases=None, cube=None, legs=None, conj=None, bpwts=None, freq_wts=None, masks=None,
                              mask_index=None, nt=None, phase_route='auto', nres=0, pscale=None, want=('res',), route='auto',
                              want_phase=False, budget_bytes=CLOSURE_BUDGET):
        """Delay spectra of closure phases on the device (prisim_closure_delay_spectra).  Either phases (..., nchan, nt) float64 --
        every leading axis is a row --, or the arguments of closure_phase (cube (nbl, nchan, nt) or None for the resident slots [0, nt),
        legs, conj, bpwts, freq_wts, masks, mask_index, phase_route): the phases are then formed on the device and transformed there, no
        triplet is downloaded, and the phases come back only with want_phase.  wts (nwin, nchan) windows, m lags, nres resampled
        lags, pscale (nwin,) for the power products; want: any of 'over', 'over_power', 'res', 'res_power'.  Returns a dict of the
        wanted outputs, (rows..., nwin, m | nres, nt), 'phase' (ntriads, nchan, nt) with want_phase, and 'stats'."""
        w = NP.ascontiguousarray(wts, dtype=NP.float64)
        w = w.reshape(-1, w.shape[-1])
        nwin, nchan = w.shape
        m, nres = int(m), int(nres)
        lg = cj = bw = fw = mk = mi = x = ph = None
        nbl = 0
        if phases is not None:
            ph = NP.ascontiguousarray(phases, dtype=NP.float64)
            if ph.ndim < 2 or ph.shape[-2] != nchan:
                raise ValueError('phases must be (..., nchan, nt) with the channel count of wts')
            lead, nt = ph.shape[:-2], ph.shape[-1]
            nrows = int(NP.prod(lead, dtype=NP.int64))
        else:
            if legs is None or conj is None or bpwts is None:
                raise ValueError('without phases, legs, conj and bpwts are required')
            if cube is None:
                if nt is None:
                    raise ValueError('nt is required with resident input')
                nbl, nt = self.nbl, int(nt)
                if self.nchan != nchan:
                    raise ValueError('wts must have the channel count of the resident cube')
            else:
                x = NP.ascontiguousarray(cube, dtype=NP.complex128)
                if x.ndim != 3 or x.shape[1] != nchan:
                    raise ValueError('cube must be (nbl, nchan, nt) with the channel count of wts')
                nbl, _, nt = x.shape
            lg, cj, bw, fw, mk, mi = _closure_inputs(legs, conj, bpwts, freq_wts, masks, mask_index, nbl, nchan, nt)
            nrows, lead = lg.shape[0], (lg.shape[0],)
        flag = _want_bits(want, {'over': PRISIM_CPDELAY_OVER, 'over_power': PRISIM_CPDELAY_OVER_POWER, 'res': PRISIM_CPDELAY_RES,
                                 'res_power': PRISIM_CPDELAY_RES_POWER})
        ps = None if pscale is None else NP.ascontiguousarray(NP.broadcast_to(NP.asarray(pscale, dtype=NP.float64).ravel(), (nwin,)))
        out = {}
        for name in want:
            n = m if name.startswith('over') else max(nres, 1)
            out[name] = NP.empty(tuple(lead) + (nwin, n, nt), dtype=NP.complex128 if name in ('over', 'res') else NP.float64)
        if want_phase and phases is None:
            out['phase'] = NP.empty((nrows, nchan, nt), dtype=NP.float64)
        nmap, mo, mi_, mw = _resample_map(flag & (PRISIM_CPDELAY_RES | PRISIM_CPDELAY_RES_POWER) and 1 <= nres <= PRISIM_CPDELAY_MAX_LEN
                                          and 1 <= m <= PRISIM_CPDELAY_MAX_LEN, m, nres)
        st = PrisimCpdelayStats()
        r, pr = _route_code(route, CPDELAY_ROUTES), _route_code(phase_route, CLOSURE_ROUTES)
        self._call('prisim_closure_delay_spectra', phases=ph, nrows=nrows, cube=x, nt=nt, nbl=nbl, nchan=nchan, legs=lg, conj=cj, freq_wts=fw,
                   bpwts=bw, masks=mk, nmask=0 if mk is None else mk.shape[0], mask_index=mi, phase_route=pr, nwin=nwin, wts=w, m=m, df=df,
                   nres=nres, nmap=nmap, map_out=mo, map_in=mi_, map_w=mw, pscale=ps, want=flag, route=r, budget_bytes=budget_bytes,
                   out_phase=out.get('phase'), over=out.get('over'), over_pow=out.get('over_power'), res=out.get('res'),
                   res_pow=out.get('res_power'), stats=st)
        out['stats'] = _stats_dict(st, route=CPDELAY_ROUTES, phase_route=CLOSURE_ROUTES.get)   # phase_route: None where no phases were formed
        out['stats']['resident'] = phases is None and x is None
        return out

    def closure_power(self, spectra, scale, want=('individual',), budget_bytes=CLOSURE_BUDGET):
        """Power spectra of closure-phase delay spectra on the device (prisim_closure_power).  spectra (n0, nwin, ...) complex128, scale
        (nwin,); want: any of 'individual' (|x|^2 scale, spectra's shape), 'auto' (mean over axis 0 of |x|^2, times scale; axis 0 kept
        with one entry) and 'cross' ((scale |sum over axis 0 of x|^2 - n0 auto) / (n0 (n0 - 1)); n0 >= 2).  Returns a dict of the wanted
        outputs and 'stats'."""
        x = NP.ascontiguousarray(spectra, dtype=NP.complex128)
        if x.ndim < 2:
            raise ValueError('spectra must be (n0, nwin, ...)')
        n0, nwin = x.shape[0], x.shape[1]
        inner = int(NP.prod(x.shape[2:], dtype=NP.int64))
        sc = NP.ascontiguousarray(NP.broadcast_to(NP.asarray(scale, dtype=NP.float64).ravel(), (nwin,)))
        flag = _want_bits(want, {'individual': PRISIM_CPPOWER_INDIVIDUAL, 'auto': PRISIM_CPPOWER_AUTO, 'cross': PRISIM_CPPOWER_CROSS})
        out = {name: NP.empty(x.shape if name == 'individual' else (1,) + x.shape[1:], dtype=NP.float64) for name in want}
        st = PrisimCpdelayStats()
        self._call('prisim_closure_power', n0=n0, nwin=nwin, inner=inner, spectra=x, scale=sc, want=flag, budget_bytes=budget_bytes,
                   out_individual=out.get('individual'), out_auto=out.get('auto'), out_cross=out.get('cross'), stats=st)
        out['stats'] = _stats_dict(st, route=CPDELAY_ROUTES, phase_route=CLOSURE_ROUTES.get)   # phase_route: None where no phases were formed
        return out

    # ---- day and LST binning of closure phases (include/prisim_cpbins.h) ----
    def cphase_upload(self, phases, flags):
        """Upload a (n0, n1, ntriads, nchan) stack of closure phases and its flags once; returns the resident CphaseStack."""
        ph = NP.ascontiguousarray(phases, dtype=NP.float64)
        fl = NP.ascontiguousarray(NP.asarray(flags) != 0, dtype=NP.uint8)
        if ph.ndim != 4 or fl.shape != ph.shape:
            raise ValueError('phases and flags must both be (n0, n1, ntriads, nchan)')
        h = C.c_void_p()
        st = PrisimCpbinsStats()
        n0, n1, ntriads, nchan = ph.shape
        self._call('prisim_cphase_bin', kind=PRISIM_CPBINS_PHASE_FLAGS, in_mean=ph, in_median=None, in_wts=None, in_flags=fl, n0=n0, n1=n1,
                   ntriads=ntriads, nchan=nchan, axis=0, nbins=0, offsets=None, members=None, want=0, mad_ignores_flags=0, budget_bytes=0,
                   resident_in=h, keep_out=None, out_wts=None, out_eicp_mean=None, out_eicp_median=None, out_cp_mean=None,
                   out_cp_median=None, out_rms=None, out_mad=None, stats=st)
        return CphaseStack(self, h, PRISIM_CPBINS_PHASE_FLAGS, ph.shape)

    def cphase_bin(self, axis, offsets, members, phases=None, flags=None, binned=None, stack=None, want=tuple(CPBINS_WANT),
                   mad_ignores_flags=False, keep=False, budget_bytes=CLOSURE_BUDGET):
        """Flagged binning of one axis (0 or 1) of a (n0, n1, ntriads, nchan) stack of closure phases on the device
        (prisim_cphase_bin).  The bins are the CSR pair offsets (nbins + 1,), members (indices on the axis).  The input is one of:
        phases and flags (the native stack); binned = (mean phases, median phases, weights) of an earlier pass, masked where the weight
        is <= 0; or stack, a resident CphaseStack of either kind (cphase_upload, or a call with keep=True).  want: any of 'wts',
        'eicp_mean', 'eicp_median', 'cp_mean', 'cp_median', 'rms', 'mad', the outputs copied back; keep: the (mean phase, median phase,
        weights) of this call stay on the device and come back as out['stack'].  Under the mask (no unmasked member) the device writes
        eicp = 1, everything else 0.  Returns a dict of the wanted outputs and 'stats'."""
        a = b = w = f = None
        if stack is not None:
            kind, shape = stack.kind, stack.shape
        elif binned is not None:
            kind = PRISIM_CPBINS_BINNED
            a, b, w = (NP.ascontiguousarray(x, dtype=NP.float64) for x in binned)
            shape = a.shape
            if a.ndim != 4 or b.shape != shape or w.shape != shape:
                raise ValueError('the binned arrays must all be (n0, n1, ntriads, nchan)')
        else:
            kind = PRISIM_CPBINS_PHASE_FLAGS
            a = NP.ascontiguousarray(phases, dtype=NP.float64)
            f = NP.ascontiguousarray(NP.asarray(flags) != 0, dtype=NP.uint8)
            shape = a.shape
            if a.ndim != 4 or f.shape != shape:
                raise ValueError('phases and flags must both be (n0, n1, ntriads, nchan)')
        if axis not in (0, 1):
            raise ValueError('axis must be 0 or 1')
        off = NP.ascontiguousarray(offsets, dtype=NP.int64).ravel()
        mem = NP.ascontiguousarray(members, dtype=NP.int32).ravel()
        nbins = off.size - 1
        if nbins < 1 or off[0] != 0 or off[-1] != mem.size:
            raise ValueError('offsets must be (nbins + 1,), from 0 to the number of members')
        oshape = tuple(nbins if i == axis else n for i, n in enumerate(shape))
        flag = _want_bits(want, CPBINS_WANT)
        out = {name: NP.empty(oshape, dtype=NP.complex128 if name.startswith('eicp') else NP.float64) for name in want}
        st = PrisimCpbinsStats()
        hin = C.c_void_p(stack.handle.value) if stack is not None else None
        hout = C.c_void_p()
        n0, n1, ntriads, nchan = shape
        self._call('prisim_cphase_bin', kind=kind, in_mean=a, in_median=b, in_wts=w, in_flags=f, n0=n0, n1=n1, ntriads=ntriads, nchan=nchan,
                   axis=axis, nbins=nbins, offsets=off, members=mem, want=flag, mad_ignores_flags=bool(mad_ignores_flags),
                   budget_bytes=budget_bytes, resident_in=hin, keep_out=hout if keep else None, stats=st,
                   **{'out_' + name: out.get(name) for name in CPBINS_WANT})
        if keep:
            out['stack'] = CphaseStack(self, hout, PRISIM_CPBINS_BINNED, oshape)
        out['stats'] = _stats_dict(st, rename={'resident_in': 'resident'}, resident_in=bool)
        return out

    # ---- differences of day sub-samples of binned closure phases (include/prisim_cpdiff.h) ----
    def cphase_diff(self, pairs, stack=None, binned=None, budget_bytes=0):
        """Half differences of the unit phasors of pairs of day bins of a binned (n0, n1, ntriads, nchan) stack on the device
        (prisim_cphase_diff).  pairs: (ncomb, 4) integers (i, j, k, m), indices on axis 1 with i != j and k != m.  The input is one of:
        stack, a resident CphaseStack of kind BINNED (a cphase_bin call with keep=True), or binned = (mean phases, median phases,
        weights) on the host.  Returns a dict of 'diff0_mean', 'diff0_median' (0.5 (e_j - e_i)), 'diff1_mean', 'diff1_median'
        (0.5 (e_m - e_k)) complex128, 'wts0', 'wts1' (the root of the sum of the squared weights) float64 and 'mask0', 'mask1' bool (a
        member's weight is not > 0), each (n0, ncomb, ntriads, nchan), and 'stats'.  Under the mask the differences are 0; the weights
        are written everywhere."""
        a = b = w = None
        if stack is not None:
            if stack.kind != PRISIM_CPBINS_BINNED:
                raise ValueError('the resident stack is not of kind BINNED, or of another shape or device')
            shape = stack.shape
        elif binned is not None:
            a, b, w = (NP.ascontiguousarray(x, dtype=NP.float64) for x in binned)
            shape = a.shape
            if a.ndim != 4 or b.shape != shape or w.shape != shape:
                raise ValueError('the binned arrays must all be (n0, n1, ntriads, nchan)')
        else:
            raise ValueError('need a resident stack or the binned arrays')
        pr = NP.asarray(pairs)
        if pr.size and not NP.issubdtype(pr.dtype, NP.integer):
            raise ValueError('pairs must be integers')
        if pr.ndim != 2 or pr.shape[1] != 4 or pr.shape[0] < 1:
            raise ValueError('need ncomb >= 1 pairs of pairs')
        for q, row in enumerate(pr.tolist()):
            for v in row:
                if v < 0 or v >= shape[1]:
                    raise ValueError('pair of pairs {0} holds {1}, not an index of axis 1'.format(q, v))
            if row[0] == row[1] or row[2] == row[3]:
                raise ValueError('pair of pairs {0} holds a pair of one index with itself'.format(q))
        pr = NP.ascontiguousarray(pr, dtype=NP.int32)
        oshape = (shape[0], pr.shape[0], shape[2], shape[3])
        out = {name: NP.empty(oshape, dtype=NP.complex128 if name.startswith('diff') else (NP.float64 if name.startswith('wts') else NP.uint8))
               for name in CPDIFF_OUTPUTS}
        st = PrisimCpdiffStats()
        n0, n1, ntriads, nchan = shape
        self._call('prisim_cphase_diff', in_mean=a, in_median=b, in_wts=w, n0=n0, n1=n1, ntriads=ntriads, nchan=nchan,
                   resident=None if stack is None else stack.handle, ncomb=pr.shape[0], pairs=pr, budget_bytes=budget_bytes, stats=st,
                   **{'out_' + name: out[name] for name in CPDIFF_OUTPUTS})
        for name in ('mask0', 'mask1'):
            out[name] = out[name].view(NP.bool_)
        out['stats'] = _stats_dict(st, rename={'resident_in': 'resident'}, resident_in=bool)
        return out

    # ---- delay spectra of binned closure phasors (include/prisim_cpft.h) ----
    def cphase_ft(self, inputs, wts, m, df, weights=None, vscale=None, nres=None, want=('over', 'res', 'lag_kernel'), route='auto',
                  budget_bytes=0, shape=None):
        """Delay spectra of stacks of complex numbers (n0, n1, n2, nchan) on the device (prisim_cphase_ft).  inputs: up to 8 complex
        arrays, each (b0, b1, b2, nchan) with every b the full extent or 1 (read with stride 0 on the device, never materialised);
        the full shape is that of weights, else `shape` (n0, n1, n2), else the broadcast of the inputs' shapes.  wts (nwin, nchan)
        frequency windows, m lags, df; weights (n0, n1, n2, nchan) float64 flag weights shared by all inputs, divided by their mean
        over the channels on the device (None: no weights); vscale (nwin, n0) (None: 1); nres resampled lags.  want: any of 'over',
        'res' and 'lag_kernel'.  Returns a dict of 'over' and 'res' (lists, one (nwin, n0, n1, n2, m | nres) array per input),
        'lag_kernel' and 'lag_kernel_res' ((nwin, n0, n1, n2, m | nres) with weights, (nwin, 1, 1, 1, m | nres) without) -- None
        where not wanted -- and 'stats'."""
        fw = NP.ascontiguousarray(wts, dtype=NP.float64)
        fw = fw.reshape(-1, fw.shape[-1])
        nwin, nchan = fw.shape
        xs = [NP.asarray(x) for x in inputs]
        if len(xs) > PRISIM_CPFT_MAX_IN:
            raise ValueError('need 0 <= nin <= {0} input stacks'.format(PRISIM_CPFT_MAX_IN))
        for x in xs:
            if x.ndim != 4 or x.shape[-1] != nchan:
                raise ValueError('every input must be (b0, b1, b2, nchan) with the channel count of wts')
        w = None
        if weights is not None:
            w = NP.ascontiguousarray(weights, dtype=NP.float64)
            if w.ndim != 4 or w.shape[-1] != nchan:
                raise ValueError('weights must be (n0, n1, n2, nchan) with the channel count of wts')
            lead = w.shape[:3]
        elif shape is not None:
            lead = tuple(int(n) for n in shape)
        elif xs:
            lead = NP.broadcast_shapes(*[x.shape[:3] for x in xs])
        else:
            lead = (1, 1, 1)
        for i, x in enumerate(xs):
            for a in range(3):
                if x.shape[a] not in (lead[a], 1):
                    raise ValueError('input {0}: axis {1} has {2} entries, neither the full extent nor 1'.format(i, a, x.shape[a]))
        xs = [NP.ascontiguousarray(x, dtype=NP.complex128) for x in xs]
        vs = None
        if vscale is not None:
            vs = NP.ascontiguousarray(NP.broadcast_to(NP.asarray(vscale, dtype=NP.float64), (nwin, lead[0])))
        m = int(m)
        flag = _want_bits(want, {'over': PRISIM_CPFT_OVER, 'res': PRISIM_CPFT_RES, 'lag_kernel': PRISIM_CPFT_LAG})
        nres = 0 if nres is None else int(nres)
        if flag & PRISIM_CPFT_RES and nres < 1:
            raise ValueError('the resampled spectra need nres >= 1')
        nmap, mo, mi, mw = _resample_map(flag & PRISIM_CPFT_RES and nres <= PRISIM_CPFT_MAX_LEN and 1 <= m <= PRISIM_CPFT_MAX_LEN, m, nres)
        nin = len(xs)
        out = {'over': None, 'res': None, 'lag_kernel': None, 'lag_kernel_res': None}
        if flag & PRISIM_CPFT_OVER:
            out['over'] = [NP.empty((nwin,) + tuple(lead) + (m,), dtype=NP.complex128) for _ in xs]
        if flag & PRISIM_CPFT_RES:
            out['res'] = [NP.empty((nwin,) + tuple(lead) + (nres,), dtype=NP.complex128) for _ in xs]
        if flag & PRISIM_CPFT_LAG:
            klead = tuple(lead) if w is not None else (1, 1, 1)
            out['lag_kernel'] = NP.empty((nwin,) + klead + (m,), dtype=NP.complex128)
            if flag & PRISIM_CPFT_RES:
                out['lag_kernel_res'] = NP.empty((nwin,) + klead + (nres,), dtype=NP.complex128)

        def pointers(arrays):
            if not arrays:
                return None
            return (C.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])

        shapes = NP.ascontiguousarray([x.shape[:3] for x in xs], dtype=NP.int64).reshape(-1, 3)
        st = PrisimCpftStats()
        r = _route_code(route, CPFT_ROUTES)
        self._call('prisim_cphase_ft', n0=lead[0], n1=lead[1], n2=lead[2], nchan=nchan, nin=nin, inputs=pointers(xs),
                   in_shape=shapes if nin else None, w=w, nwin=nwin, wts=fw, vscale=vs, m=m, df=df, nres=nres, nmap=nmap, map_out=mo, map_in=mi,
                   map_w=mw, want=flag, route=r, budget_bytes=budget_bytes, over=pointers(out['over']), res=pointers(out['res']),
                   lag_kernel=out['lag_kernel'], lag_kernel_res=out['lag_kernel_res'], stats=st)
        out['stats'] = _stats_dict(st, route=CPFT_ROUTES)
        return out

    # ---- cross power of closure-phase delay spectra (include/prisim_cpxps.h) ----
    PrisimCpxpsStats = _PrisimCpxpsStats

    @staticmethod
    def cphase_xpower_shape(shape, modes, nshift):
        """The shape of cphase_xpower's result for inputs of `shape` (nspw, n1, n2, n3, nlags)"""
        out = [int(shape[0])]
        for ax, mode in enumerate(modes):
            n = int(shape[ax + 1])
            if mode == 'none':
                out.append(n)
            elif mode == 'full':
                out += [int(nshift), n] if ax == 0 else [n, n]
            else:
                out.append(int(nshift) if ax == 0 else 2 * n - 1)
        return tuple(out) + (int(shape[4]),)

    def cphase_xpower(self, a, b=None, factor=None, weights=None, modes=('none', 'none', 'none'), shifts=None, collapse=(), stat='mean',
                      budget_bytes=0):
        """Cross power of delay spectra on the device (prisim_cphase_xpower): P = (factor (a wa)) conj(b wb) over pairs of LST bins, day
        bins and triads, and its collapses.  a, b (None: a): complex (nspw, n1, n2, n3, nlags); factor (nspw,) (None: 1); weights: None
        or three entries, per axis a complex vector of the axis' length or None; modes: per axis 'none', 'full' or 'collapse'; shifts:
        the LST shifts, needed where axis 1 is crossed; collapse: the collapsed axes (1, 2, 3) in the order of their collapse; stat:
        'mean' or 'median' of the LST collapse.  Returns {'out': complex (nspw, per axis n | nshift, n1 | n, n | nshift | 2n-1, nlags),
        'stats'}."""
        a = NP.ascontiguousarray(a, dtype=NP.complex128)
        if a.ndim != 5:
            raise ValueError('a must be (nspw, n1, n2, n3, nlags)')
        if b is not None:
            b = NP.ascontiguousarray(b, dtype=NP.complex128)
            if b.shape != a.shape:
                raise ValueError('b must have the shape of a')
        nspw = a.shape[0]
        f = NP.ones(nspw) if factor is None else NP.ascontiguousarray(factor, dtype=NP.float64).reshape(-1)
        if f.size != nspw:
            raise ValueError('factor must have one entry per window')
        modes = tuple(modes)
        if len(modes) != 3:
            raise ValueError('modes must have three entries')
        mcodes = NP.ascontiguousarray([CPXPS_MODES[m] for m in modes], dtype=NP.int32)
        ws = [None] * 3
        if weights is not None:
            if len(weights) != 3:
                raise ValueError('weights must have three entries')
            for ax, w in enumerate(weights):
                if w is not None:
                    ws[ax] = NP.ascontiguousarray(w, dtype=NP.complex128).reshape(-1)
                    if ws[ax].size != a.shape[ax + 1]:
                        raise ValueError('the weights of axis {0} must have {1} entries'.format(ax + 1, a.shape[ax + 1]))
        wptr = (C.c_void_p * 3)(*[None if w is None else w.ctypes.data for w in ws])
        sh = None
        if modes[0] != 'none':
            if shifts is None:
                raise ValueError('a crossed LST axis needs its shifts')
            sh = NP.ascontiguousarray(shifts, dtype=NP.int64).reshape(-1)
        nshift = 0 if sh is None else sh.size
        order = NP.ascontiguousarray(collapse, dtype=NP.int32).reshape(-1)
        scode = CPXPS_STATS[stat]
        if nshift < 1 and sh is not None:
            raise ValueError('a crossed LST axis needs 1 to 2^20 shifts')
        out = NP.empty(self.cphase_xpower_shape(a.shape, modes, nshift), dtype=NP.complex128)
        st = self.PrisimCpxpsStats()
        self._call('prisim_cphase_xpower', nspw=nspw, n1=a.shape[1], n2=a.shape[2], n3=a.shape[3], nlags=a.shape[4], a=a, b=b, factor=f,
                   weights=wptr, modes=mcodes, nshift=nshift, shifts=sh, ncollapse=order.size, order=order, stat=scode,
                   budget_bytes=budget_bytes, out=out, stats=st)
        return {'out': out, 'stats': _stats_dict(st)}

    # ---- incoherent averages of closure-phase power spectra (include/prisim_cpavg.h) ----
    PrisimCpavgStats = _PrisimCpavgStats

    @staticmethod
    def cphase_xavg_arguments(arrays, weights, combos=()):
        """The checked arguments of cphase_xavg: (arrays complex128, weights float64, masks), masks a list of {axis: uint8 mask}.
        ValueError where the header would refuse them."""
        arrays = [NP.ascontiguousarray(a, dtype=NP.complex128) for a in arrays]
        weights = [NP.ascontiguousarray(w, dtype=NP.float64) for w in weights]
        if len(arrays) < 1 or len(weights) != len(arrays):
            raise ValueError('need at least one array and one weight array per array')
        shape = arrays[0].shape
        ndim = len(shape)
        if not PRISIM_CPAVG_MIN_DIM <= ndim <= PRISIM_CPAVG_MAX_DIM:
            raise ValueError('the arrays must have {0} to {1} axes'.format(PRISIM_CPAVG_MIN_DIM, PRISIM_CPAVG_MAX_DIM))
        if min(shape) < 1:
            raise ValueError('every axis needs at least one entry')
        for a, w in zip(arrays, weights):
            if a.shape != shape:
                raise ValueError('the arrays must have one shape')
            if w.ndim != ndim or w.shape[-1] != 1 or any(b not in (1, n) for b, n in zip(w.shape, shape)):
                raise ValueError('weights of shape {0} do not broadcast against {1} with 1 on the lags'.format(w.shape, shape))
        masks = []
        for combo in combos:
            if len(combo) < 1:
                raise ValueError('a combination must reduce at least one axis')
            mk = {}
            for ax, sel in combo.items():
                ax = int(ax)
                if not 0 < ax < ndim - 1:
                    raise ValueError('a combination cannot reduce axis {0}: neither the windows nor the lags'.format(ax))
                sel = NP.ascontiguousarray(NP.asarray(sel).astype(bool).reshape(-1), dtype=NP.uint8)
                if sel.size != shape[ax] or not sel.any():
                    raise ValueError('the mask of axis {0} must have {1} entries and select at least one'.format(ax, shape[ax]))
                mk[ax] = sel
            masks.append(mk)
        return arrays, weights, masks

    @staticmethod
    def cphase_xavg_shapes(shape, wshapes, masks):
        """(U, [shape of out], [shape of wout]) of cphase_xavg: the common shape of the weights and the results per combination"""
        u = tuple(int(max(ws[x] for ws in wshapes)) for x in range(len(shape)))
        oshapes = [tuple(1 if x in mk else int(n) for x, n in enumerate(shape)) for mk in masks]
        woshapes = [tuple(1 if x in mk else n for x, n in enumerate(u)) for mk in masks]
        return u, oshapes, woshapes

    def cphase_xavg(self, arrays, weights, combos=(), want_avg=True, budget_bytes=0):
        """The weighted average of several arrays and averages of it over selected positions, on the device (prisim_cphase_xavg).
        arrays: complex, one shape of 5 to 8 axes, axis 0 the windows and the last the lags; weights: per array a float array with
        every extent 1 or the array's and 1 on the lags; combos: dictionaries {axis: boolean mask of the selected positions}.
        Returns {'avg': sum(a w) / sum(w) with NaN products counted as 0 (None unless want_avg), 'wsum': sum(w) at the common shape
        of the weights, 'out': per combination (sum of avg wsum) / (sum of wsum) over its positions, the reduced axes kept at 1,
        'wout': those sums of wsum, 'stats'}."""
        arrays, weights, masks = self.cphase_xavg_arguments(arrays, weights, combos)
        shape = arrays[0].shape
        ndim, nsets, ncombo = len(shape), len(arrays), len(masks)
        wshapes = NP.ascontiguousarray([w.shape for w in weights], dtype=NP.int64)
        u, oshapes, woshapes = self.cphase_xavg_shapes(shape, wshapes, masks)
        avg = NP.empty(shape, dtype=NP.complex128) if want_avg else None
        wsum = NP.empty(u, dtype=NP.float64)
        out = [NP.empty(s, dtype=NP.complex128) for s in oshapes]
        wout = [NP.empty(s, dtype=NP.float64) for s in woshapes]
        reduce = NP.zeros((max(ncombo, 1), ndim), dtype=NP.int32)
        mptr = (C.c_void_p * max(ncombo * ndim, 1))()
        for c, mk in enumerate(masks):
            for ax, sel in mk.items():
                reduce[c, ax] = 1
                mptr[c * ndim + ax] = sel.ctypes.data

        def pointers(xs):
            return (C.c_void_p * max(len(xs), 1))(*[x.ctypes.data for x in xs])

        st = self.PrisimCpavgStats()
        self._call('prisim_cphase_xavg', ndim=ndim, shape=NP.ascontiguousarray(shape, dtype=NP.int64), nsets=nsets, arrays=pointers(arrays),
                   weights=pointers(weights), wshapes=wshapes, ncombo=ncombo, reduce=reduce, masks=mptr, budget_bytes=budget_bytes, avg=avg,
                   wsum=wsum, out=pointers(out), wout=pointers(wout), stats=st)
        return {'avg': avg, 'wsum': wsum, 'out': out, 'wout': wout, 'stats': _stats_dict(st, route=CPAVG_ROUTES)}

    @staticmethod
    def cphase_kbin_arguments(p, kprll, offsets, members):
        """The checked arguments of cphase_kbin: (p complex128 (nspw, m, nlags), kprll, offsets int64 (nspw, nk + 1), the members of all
        windows int32, the leading shape of p).  ValueError where the header would refuse them."""
        p = NP.asarray(p)
        k = NP.ascontiguousarray(kprll, dtype=NP.float64)
        if k.ndim != 2 or p.ndim < 2 or p.shape[0] != k.shape[0] or p.shape[-1] != k.shape[1] or p.size < 1:
            raise ValueError('p must be (nspw, ..., nlags) and kprll (nspw, nlags), none of them empty')
        lead = p.shape[:-1]
        p = NP.ascontiguousarray(p, dtype=NP.complex128).reshape(k.shape[0], -1, k.shape[1])
        off = NP.ascontiguousarray(offsets, dtype=NP.int64)
        if off.ndim != 2 or off.shape[0] != k.shape[0] or off.shape[1] < 2:
            raise ValueError('offsets must be (nspw, nk + 1) with nk >= 1')
        if len(members) != k.shape[0]:
            raise ValueError('members must hold one array per window')
        mem = [NP.asarray(m).reshape(-1) for m in members]
        for w, m in enumerate(mem):
            o = off[w]
            if o[0] != 0 or NP.any(NP.diff(o) < 0) or o[-1] != m.size:
                raise ValueError('window {0}: the offsets must start at 0, not decrease and end at the number of members'.format(w))
            if m.size and (m.min() < 0 or m.max() >= k.shape[1]):
                raise ValueError('window {0}: a member is not a lag in [0, {1})'.format(w, k.shape[1]))
            for b in range(o.size - 1):
                if NP.any(NP.diff(m[o[b]:o[b + 1]]) <= 0):
                    raise ValueError('window {0}, bin {1}: the members must increase'.format(w, b))
        allmem = NP.ascontiguousarray(NP.concatenate(mem) if mem else NP.zeros(0), dtype=NP.int32)
        return p, k, off, allmem, lead

    def cphase_kbin(self, p, kprll, offsets, members, route='auto', budget_bytes=0):
        """Averages of a power spectrum in bins of |k_parallel| on the device (prisim_cphase_kbin).  p: complex (nspw, ..., nlags);
        kprll (nspw, nlags); offsets (nspw, nk + 1) and members (one array of lag indices per window): per window the CSR pair of its
        bins, the members of a bin increasing; route: 'auto', 'lds' or 'global'.  Returns {'ps': the mean of the members that are not
        NaN, 'del2': the mean of |k|^3 p over 2 pi^2, 'kc': sum |k| |p| / sum |p|, each (nspw, ..., nk), NaN for an empty bin,
        'stats'}."""
        r = _route_code(route, CPAVG_ROUTES)
        p, k, off, mem, lead = self.cphase_kbin_arguments(p, kprll, offsets, members)
        nk = off.shape[1] - 1
        ps = NP.empty(lead + (nk,), dtype=NP.complex128)
        del2 = NP.empty(lead + (nk,), dtype=NP.complex128)
        kc = NP.empty(lead + (nk,), dtype=NP.float64)
        st = self.PrisimCpavgStats()
        self._call('prisim_cphase_kbin', nspw=p.shape[0], m=p.shape[1], nlags=p.shape[2], nk=nk, p=p, kprll=k, offsets=off, members=mem,
                   route=r, budget_bytes=budget_bytes, ps=ps, del2=del2, kc=kc, stats=st)
        return {'ps': ps, 'del2': del2, 'kc': kc, 'stats': _stats_dict(st, route=CPAVG_ROUTES)}

    # ---- instrument gain tables (include/prisim_gains.h) ----
    def gains_eval_spline(self, packed, times, freqs):
        """Evaluate a packed spline table (prisim_amd/gains.py:pack_splines) at every (time, channel) on the device: a GainTable
        [nt][nrows][nchan] and the stats."""
        t = NP.ascontiguousarray(NP.asarray(times, dtype=NP.float64).ravel())
        f = NP.ascontiguousarray(NP.asarray(freqs, dtype=NP.float64).ravel())
        arr = {k: NP.ascontiguousarray(packed[k], dtype=NP.int64) for k in ('nx', 'ny', 'kx_off', 'ky_off', 'c_off')}
        kn = NP.ascontiguousarray(packed['knots'], dtype=NP.float64)
        co = NP.ascontiguousarray(packed['coefs'], dtype=NP.float64)
        nrows = arr['nx'].size // 2
        h, st = C.c_void_p(), PrisimGainsStats()
        self._call('prisim_gains_eval_spline', nrows=nrows, kx=packed['kx'], ky=packed['ky'], nknots=kn.size, knots=kn, ncoefs=co.size,
                   coefs=co, nt=t.size, times=t, nchan=f.size, freqs=f, out=h, stats=st, **arr)
        return GainTable(self, h), _stats_dict(st)

    def gains_gather(self, gains, fidx, tidx):
        """Nearest-neighbour table on the device: table[t][r][f] = gains[r][fidx[f]][tidx[t]] for gains (nrows, ngf, ngt)."""
        g = NP.ascontiguousarray(gains, dtype=NP.complex128)
        if g.ndim != 3:
            raise ValueError('gains must be (nrows, nfreq, ntime)')
        fi = NP.ascontiguousarray(NP.asarray(fidx).ravel(), dtype=NP.int64)
        ti = NP.ascontiguousarray(NP.asarray(tidx).ravel(), dtype=NP.int64)
        h, st = C.c_void_p(), PrisimGainsStats()
        self._call('prisim_gains_gather', nrows=g.shape[0], ngf=g.shape[1], ngt=g.shape[2], gains=g, nchan=fi.size, fidx=fi, nt=ti.size,
                   tidx=ti, out=h, stats=st)
        return GainTable(self, h), _stats_dict(st)

    def gains_apply(self, nt, nbl, nchan, fa=None, fb=None, sky=None, t0=0, sky_c64=False, noise=None, want_gain=False):
        """vis [nt][nbl][nchan] = (fa * fb) * sky + noise on the device (prisim_gains_apply).  fa / fb: None or (GainTable, mode, a, c)
        with mode PRISIM_GAINS_ANTENNA | PRISIM_GAINS_BASELINE and a, c (nbl,) rows; sky: (nt, nbl, nchan) complex128 or None for the
        resident slots [t0, t0 + nt); want_gain: the gain cube itself.  Returns (vis, stats)."""
        def fac(x):
            if x is None:
                return None, 0, None, None
            tab, mode, a, c = x
            return (tab._h, int(mode), NP.ascontiguousarray(NP.asarray(a).ravel(), dtype=NP.int64),
                    NP.ascontiguousarray(NP.asarray(c).ravel(), dtype=NP.int64))
        ta, ma, aa, ca = fac(fa)
        tb, mb, ab, cb = fac(fb)
        for arr in (aa, ca, ab, cb):
            if arr is not None and arr.size != nbl:
                raise ValueError('factor rows must have one entry per baseline')
        s = None if (sky is None or want_gain) else NP.ascontiguousarray(sky, dtype=NP.complex128)
        n = None if (noise is None or want_gain) else NP.ascontiguousarray(noise, dtype=NP.complex128)
        for arr in (s, n):
            if arr is not None and arr.shape != (nt, nbl, nchan):
                raise ValueError('sky and noise must be (nt, nbl, nchan)')
        out = NP.empty((nt, nbl, nchan), dtype=NP.complex128)
        st = PrisimGainsStats()
        self._call('prisim_gains_apply', nt=nt, nbl=nbl, nchan=nchan, ta=ta, mode_a=ma, a_a=aa, c_a=ca, tb=tb, mode_b=mb, a_b=ab, c_b=cb, sky=s,
                   t0=t0, sky_c64=bool(sky_c64), noise=n, want_gain=bool(want_gain), vis=out, stats=st)
        return out, _stats_dict(st)

    # ---- multi-GPU ----
    @staticmethod
    def comm_unique_id():
        lib = load_library()
        buf = C.create_string_buffer(128)
        rc = lib.prisim_hip_comm_unique_id(buf)
        if rc != PRISIM_OK:
            _raise(rc, 'prisim_hip_comm_unique_id failed: ' + lib.prisim_hip_last_error(None).decode())
        return buf.raw

    @staticmethod
    def comm_version():
        """'librccl <version> (<path>)' of the RCCL the library loads."""
        lib = load_library()
        buf = C.create_string_buffer(128)
        rc = lib.prisim_hip_comm_version(buf)
        if rc != PRISIM_OK:
            _raise(rc, 'prisim_hip_comm_version failed: ' + lib.prisim_hip_last_error(None).decode())
        return buf.value.decode()

    @staticmethod
    def device_pci(device):
        lib = load_library()
        buf = C.create_string_buffer(64)
        lib.prisim_hip_device_pci(int(device), buf)
        return buf.value.decode()

    @staticmethod
    def comm_last_error():
        """Text of librccl's last error / warning; safe to call from a watchdog thread while comm_init blocks in another."""
        lib = load_library()
        buf = C.create_string_buffer(512)
        lib.prisim_hip_comm_last_error(buf)
        return buf.value.decode()

    def comm_init(self, uid, nranks, rank):
        if len(uid) != 128:
            raise ValueError('unique id must be 128 bytes')
        self._check(self._lib.prisim_hip_comm_init(self._h, uid, int(nranks), int(rank)), 'prisim_hip_comm_init')
        if getattr(self, 'nranks', 1) != int(nranks):
            self.nbl_total = 0                       # (the library drops a shard map made for another communicator size)
        self.nranks = int(nranks)

    def allgather(self, nt, complex64=False):
        self._check(self._lib.prisim_hip_allgather(self._h, int(nt), 1 if complex64 else 0), 'prisim_hip_allgather')
        self._gathered_c64 = bool(complex64)

    def allgather_slot_async(self, slot, complex64=False):
        """Gather one snapshot on the communication stream, overlapping later compute() calls."""
        self._check(self._lib.prisim_hip_allgather_slot_async(self._h, int(slot), 1 if complex64 else 0),
                    'prisim_hip_allgather_slot_async')
        self._gathered_c64 = bool(complex64)

    def set_shard_map(self, bl_index, nbl_total):
        """bl_index (nranks, nbl_shard): global baseline of every local row of every rank (negative = padding), or None to go back to the
        rank-major layout.  Afterwards every gather leaves the gathered cube in the global baseline order of the unsharded array,
        (nt, nbl_total, row), on the device (prisim_hip_set_shard_map)."""
        if bl_index is None:
            self._check(self._lib.prisim_hip_set_shard_map(self._h, None, 0), 'prisim_hip_set_shard_map')
            self.nbl_total = 0
            return
        m = NP.ascontiguousarray(bl_index, dtype=NP.int64)
        if m.size != getattr(self, 'nranks', 1) * self.nbl:
            raise ValueError('bl_index must have shape (nranks, nbl_shard)')
        self._check(self._lib.prisim_hip_set_shard_map(self._h, _ptr(m), int(nbl_total)), 'prisim_hip_set_shard_map')
        self.nbl_total = int(nbl_total)

    def get_gathered(self, nt, nranks=None, row=None):
        """(nt, nranks, nbl_shard, row): snapshot-major, rank blocks in rank order; row = nchan (visibilities) or nout (delay spectra).
        With a shard map set: (nt, nbl_total, row) in global baseline order."""
        nranks = getattr(self, 'nranks', 1) if nranks is None else nranks
        row = self.nchan if row is None else int(row)
        dtype = NP.complex64 if getattr(self, '_gathered_c64', False) else NP.complex128
        if getattr(self, 'nbl_total', 0) > 0:
            out = NP.empty((nt, self.nbl_total, row), dtype=dtype)
            self._check(self._lib.prisim_hip_get_gathered(self._h, int(nt), _ptr(out)), 'prisim_hip_get_gathered')
            return out
        out = NP.empty((nt, nranks, self.nbl, row), dtype=dtype)
        self._check(self._lib.prisim_hip_get_gathered(self._h, int(nt), _ptr(out)), 'prisim_hip_get_gathered')
        return out

    def allgather_grad(self, nt, complex64=False):
        """Gather the baseline-gradient cube of nt snapshots; read with get_gathered_grad(nt, nranks)."""
        self._check(self._lib.prisim_hip_allgather_grad(self._h, int(nt), 1 if complex64 else 0), 'prisim_hip_allgather_grad')
        self._gathered_c64 = bool(complex64)

    def get_gathered_grad(self, nt, nranks=None):
        """(nt, nranks, 3, nbl_shard, nchan) after allgather_grad; with a shard map set (nt, 3, nbl_total, nchan) in global order."""
        nranks = getattr(self, 'nranks', 1) if nranks is None else nranks
        if getattr(self, 'nbl_total', 0) > 0:
            return self.get_gathered(nt, nranks, row=3 * self.nchan).reshape(nt, 3, self.nbl_total, self.nchan)
        g = self.get_gathered(nt, nranks, row=3 * self.nchan)                  # rows of 3*nchan: the block is [3][nbl][nchan] per rank
        return g.reshape(nt, nranks, 3, self.nbl, self.nchan)

    def set_gather_root(self, root=None):
        """Later gathers deliver to rank `root` only (None: to every rank); the other ranks then hold no gathered cube."""
        self._check(self._lib.prisim_hip_set_gather_root(self._h, -1 if root is None else int(root)), 'prisim_hip_set_gather_root')

    def comm_selftest(self, nbytes=1 << 20):
        """All-gather of a rank-dependent pattern, verified on the host; raises PrisimHipError when the communicator cannot move data."""
        self._check(self._lib.prisim_hip_comm_selftest(self._h, int(nbytes)), 'prisim_hip_comm_selftest')

    def comm_stats(self, reset=False):
        st = PrisimCommStats()
        self._check(self._lib.prisim_hip_get_comm_stats(self._h, C.byref(st), 1 if reset else 0), 'prisim_hip_get_comm_stats')
        return {k: getattr(st, k) for k, _ in PrisimCommStats._fields_ if k != 'reserved_'}

    # ---- asynchronous downloads ----
    def get_vis_async(self, slot, out, grad_out=None):
        """Enqueue the download of slot `slot` into `out` (nbl, nchan) complex128 / complex64 -- ideally an array from host_empty() --
        on the copy stream, behind the compute issued so far.  The arrays must stay alive until wait_downloads() / sync()."""
        if out.shape != (self.nbl, self.nchan) or out.dtype not in (NP.complex128, NP.complex64) or not out.flags['C_CONTIGUOUS']:
            raise ValueError('out must be a C-contiguous (nbl, nchan) complex128 / complex64 array')
        c64 = out.dtype == NP.complex64
        if grad_out is not None and (grad_out.shape != (3, self.nbl, self.nchan) or grad_out.dtype != out.dtype or not grad_out.flags['C_CONTIGUOUS']):
            raise ValueError('grad_out must be a C-contiguous (3, nbl, nchan) array of the dtype of out')
        self._check(self._lib.prisim_hip_get_vis_async(self._h, int(slot), _ptr(out), _ptr(grad_out), 1 if c64 else 0), 'prisim_hip_get_vis_async')

    def wait_downloads(self):
        self._check(self._lib.prisim_hip_wait_downloads(self._h), 'prisim_hip_wait_downloads')

    def gathered_checksum(self, nt, complex64=None):
        v = C.c_double()
        self._check(self._lib.prisim_hip_gathered_checksum(self._h, int(nt), C.byref(v)), 'prisim_hip_gathered_checksum')
        return v.value

    # ---- misc ----
    def sync(self):
        self._check(self._lib.prisim_hip_sync(self._h), 'prisim_hip_sync')

    def timing(self, reset=False):
        t = PrisimTiming()
        self._check(self._lib.prisim_hip_get_timing(self._h, C.byref(t), 1 if reset else 0), 'prisim_hip_get_timing')
        out = {k: getattr(t, k) for k, _ in PrisimTiming._fields_ if k != 'reserved_'}
        # baseline folding: rows the last compute() summed (distinct baseline vectors of a folded array) and the terms its kernels
        # evaluated, and the groups of 256 summed rows that lifted (last_sum_lift_groups: the kernel's own flags, by the per-axis step
        # bound of csrc/step_bound.h -- what the kernel ran); last_terms stays the delivered count, and last_lift_groups stays the
        # length-rule count max|b| max|s - s_pc| |df| / c <= limit in groups of 256 cube rows, a lower bound of what lifts
        nsum, nterms, nlift = C.c_int64(), C.c_int64(), C.c_int64()
        self._check(self._lib.prisim_hip_get_fold_info(self._h, C.byref(nsum), C.byref(nterms), C.byref(nlift)), 'prisim_hip_get_fold_info')
        out['last_sum_lift_groups'] = nlift.value
        out['last_sum_baselines'] = nsum.value
        out['last_terms_evaluated'] = nterms.value
        # vectors equal to rounding (csrc/baseline_fold.h): the rows the exact and the merged fold of the last set_array() would sum, the
        # largest |b - b_rep| of the merged one (m), the phase it bounds (rad), and whether the kernels see the merged clusters
        nexact, nnear, dev, phase, used = C.c_int64(), C.c_int64(), C.c_double(), C.c_double(), C.c_int()
        self._check(self._lib.prisim_hip_get_fold_near(self._h, C.byref(nexact), C.byref(nnear), C.byref(dev), C.byref(phase), C.byref(used)),
                    'prisim_hip_get_fold_near')
        out['fold_exact_baselines'] = nexact.value
        out['fold_near_baselines'] = nnear.value
        out['fold_near_max_dev_m'] = dev.value
        out['fold_near_phase_bound'] = phase.value
        out['fold_near_used'] = used.value
        # the second tier of the fp32 step flag: groups of 256 summed rows that ran the wide leapfrog body, and its limit in cycles
        nwide, wlim = C.c_int64(), C.c_double()
        self._check(self._lib.prisim_hip_get_step_tiers(self._h, C.byref(nwide), C.byref(wlim)), 'prisim_hip_get_step_tiers')
        out['last_sum_wide_groups'] = nwide.value
        out['wide_limit_cycles'] = wlim.value
        # tail pieces (csrc/tail_plan.h): partial cubes the last compute() summed, and how many of them the plan's last source piece was
        # cut into (0: the plan's pieces; last_nsplit stays the plan's count either way)
        npieces, ntail = C.c_int64(), C.c_int64()
        self._check(self._lib.prisim_hip_get_tail_pieces(self._h, C.byref(npieces), C.byref(ntail)), 'prisim_hip_get_tail_pieces')
        out['last_sum_pieces'] = npieces.value
        out['last_tail_pieces'] = ntail.value
        return out

    def device_info(self):
        cu, clk = C.c_int(), C.c_int()
        name = C.create_string_buffer(64)
        self._check(self._lib.prisim_hip_device_info(self._h, C.byref(cu), C.byref(clk), name), 'prisim_hip_device_info')
        return {'name': name.value.decode(), 'cu_count': cu.value, 'clock_khz': clk.value}

    def set_tuning(self, chan_tile=0, src_chunk=0, nsplit=0):
        self._check(self._lib.prisim_hip_set_tuning(self._h, int(chan_tile), int(src_chunk), int(nsplit)),
                    'prisim_hip_set_tuning')


class CphaseStack(object):
    """A stack of closure phases resident on the device (prisim_cphase_stack).  Freed by close() or with the last reference; it must not
    outlive its context."""

    def __init__(self, ctx, handle, kind, shape):
        self._ctx = ctx                    # keeps the context alive
        self.handle = handle
        self.kind = kind
        self.shape = tuple(int(n) for n in shape)

    def close(self):
        if getattr(self, 'handle', None) is not None and self.handle.value:
            self._ctx._call('prisim_cphase_stack_free', stack=self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GainTable(object):
    """A gain table on the device ([nt][nrows][nchan] complex128, include/prisim_gains.h), freed with close() or when collected.
    It keeps its context alive."""

    def __init__(self, ctx, handle):
        self._ctx, self._h = ctx, handle
        nt, nr, nf = C.c_int64(), C.c_int64(), C.c_int64()
        ctx._call('prisim_gains_table_shape', tab=handle, nt=nt, nrows=nr, nchan=nf)
        self.shape = (int(nt.value), int(nr.value), int(nf.value))

    def get(self):
        out = NP.empty(self.shape, dtype=NP.complex128)
        self._ctx._call('prisim_gains_table_get', tab=self._h, out=out)
        return out

    def close(self):
        if getattr(self, '_h', None) and getattr(self._ctx, '_h', None):
            self._ctx._call('prisim_gains_table_free', tab=self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
