"""ctypes host layer over the C-ABI (include/dpe_hip.h).

Mirrors the reference's operator interface for the hot path -- BatchCorrScores.Start/Update/
Stop and BatchCorrManifold.Start/Update/Stop (cudarecv/modules/src/batchcorrscores.cu:710-1208,
batchcorrmanifold.cu:2315-2635) -- with the reference's port names as keyword arguments.
There is NO CPU fallback: if libdpe_hip.so is missing or no GPU is present, calls fail loudly.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DPE_LIB_PATH") or os.path.join(_HERE, "libdpe_hip.so")   # DPE_LIB_PATH: A/B builds of the library (experiments)
_lib = None

EXPORTS = [
    "dpe_abi_version", "dpe_last_error", "dpe_device_info", "dpe_gen_ca_code", "dpe_sampleblock_upload",
    "dpe_host_alloc_pinned", "dpe_host_free_pinned", "dpe_device_alloc", "dpe_device_free", "dpe_memcpy_h2d",
    "dpe_memcpy_d2h", "dpe_stream_create", "dpe_stream_destroy", "dpe_stream_synchronize",
    "dpe_bcs_create", "dpe_bcs_destroy", "dpe_bcs_update", "dpe_bcs_outputs", "dpe_bcs_read_info",
    "dpe_bcs_export_dense", "dpe_bcm_create", "dpe_bcm_create_axes", "dpe_bcm_destroy", "dpe_bcm_update", "dpe_bcm_results",
    "dpe_bcm_scores", "dpe_bcm_scores_pitch", "dpe_bcm_keys", "dpe_bcm_results_from_keys", "dpe_event_create", "dpe_event_record",
    "dpe_event_elapsed_ms", "dpe_event_destroy", "dpe_chm_create", "dpe_chm_destroy", "dpe_chm_start",
    "dpe_chm_update", "dpe_chm_outputs", "dpe_bcs_profile", "dpe_bcm_profile", "dpe_acq_create", "dpe_acq_destroy",
    "dpe_acq_search", "dpe_acq_results", "dpe_acq_surface", "dpe_bcs_set_graph", "dpe_bcm_set_graph",
    "dpe_acq_fine", "dpe_acq_scalar_acquisition",
    "dpe_ekf_create", "dpe_ekf_destroy", "dpe_ekf_step_update", "dpe_ekf_step_predict", "dpe_ekf_state", "dpe_ekf_load",
    "dpe_hbm_ceiling", "dpe_bcs_stage1_kernel",
    "dpe_set_device", "dpe_comm_create", "dpe_comm_wrap_nccl", "dpe_comm_destroy", "dpe_comm_rank", "dpe_comm_allreduce_max_u64",
    "dpe_comm_allgather", "dpe_bcm_exchange_keys", "dpe_bcs_allgather_banks",
    "dpe_bcs_update_dev", "dpe_bcs_dev_status", "dpe_bcm_update_dev", "dpe_bcm_export_scores_f64",
    "dpe_chm_dev_create", "dpe_chm_dev_destroy", "dpe_chm_dev_attach", "dpe_chm_dev_ports", "dpe_chm_dev_start", "dpe_chm_dev_update",
    "dpe_chm_dev_step", "dpe_chm_dev_fix", "dpe_chm_dev_read", "dpe_bcs_update_prepared", "dpe_bcm_update_prepared", "dpe_bcs_set_dev_hint",
    "dpe_chm_dev_set_shard", "dpe_chm_dev_set_ekf", "dpe_chm_dev_ekf_state", "dpe_chm_dev_ekf_load",
    "dpe_pipe_create", "dpe_pipe_create_axes", "dpe_pipe_destroy", "dpe_pipe_in_flight", "dpe_pipe_submit", "dpe_pipe_acquire", "dpe_pipe_mark_stage1",
    "dpe_pipe_commit", "dpe_pipe_lane", "dpe_pipe_set_in_flight", "dpe_pipe_lane_at", "dpe_pipe_results", "dpe_pipe_samples_consumed", "dpe_pipe_join", "dpe_pipe_synchronize",
    "dpe_trk_create", "dpe_trk_destroy", "dpe_trk_set_params", "dpe_trk_track", "dpe_trk_correlate", "dpe_trk_read_log",
    "dpe_trk_read_cp_signs", "dpe_trk_state", "dpe_trk_dev_status",
    "dpe_bcm_create_joint", "dpe_bcm_update_joint", "dpe_bcm_results_joint", "dpe_bcm_joint_set_own_keys",
    "dpe_bcm_create_epochs", "dpe_bcm_update_epochs", "dpe_bcm_results_epochs", "dpe_bcm_last_split",
    "dpe_bcm_create_subsets", "dpe_bcm_update_subsets", "dpe_bcm_results_subsets",
    "dpe_bcm_create_refine", "dpe_bcm_update_refine", "dpe_bcm_results_refine", "dpe_bcm_refine_scores", "dpe_bcm_refine_keys",
    "dpe_bcm_moments", "dpe_bcm_moments_results", "dpe_bcm_moments_dev", "dpe_bcm_moments_from_sums",
    "dpe_bcm_moments_rval", "dpe_chm_dev_set_measurement_cov", "dpe_chm_dev_rval",
    "dpe_nav_create", "dpe_nav_destroy", "dpe_nav_decode", "dpe_nav_set_ephemerides", "dpe_nav_solve", "dpe_nav_solve_log", "dpe_nav_status", "dpe_nav_load_log",
    "dpe_vt_create", "dpe_vt_destroy", "dpe_vt_set_ephemerides", "dpe_vt_init", "dpe_vt_init_from_trk", "dpe_vt_track", "dpe_vt_read_log",
    "dpe_vt_read_corr", "dpe_vt_state", "dpe_vt_dev_status", "dpe_vt_filter_step_host",
    "dpe_syn_create", "dpe_syn_destroy", "dpe_syn_set_nav_bits", "dpe_syn_windows", "dpe_syn_record",
    "dpe_cd_create", "dpe_cd_destroy", "dpe_cd_predict", "dpe_cd_update", "dpe_cd_results", "dpe_cd_map",
    "dpe_fe_create", "dpe_fe_destroy", "dpe_fe_info", "dpe_fe_convert", "dpe_fe_clipped",
    "dpe_ix_create", "dpe_ix_destroy", "dpe_ix_info", "dpe_ix_process", "dpe_ix_stats", "dpe_ix_analyse",
    "dpe_arr_create", "dpe_arr_destroy", "dpe_arr_info", "dpe_arr_process", "dpe_arr_stats", "dpe_arr_analyse",
]


class DpeError(RuntimeError):
    pass


class BcsConfig(C.Structure):
    _fields_ = [("samplesPerWindow", C.c_int32), ("lagHalfWidth", C.c_int32), ("binHalfWidth", C.c_int32),
                ("maxWindows", C.c_int32), ("maxChannels", C.c_int32), ("reserved", C.c_int32),
                ("samplingFrequency", C.c_double)]


class BcsPortsDev(C.Structure):     # dpe_bcs_ports_dev: device pointers to the reference's port arrays
    _fields_ = [(n, C.c_void_p) for n in ("codePhaseStart", "carrierPhaseStart", "codeFrequency", "carrierFrequency",
                                          "cpElapsedStart", "cpReference", "validPRNs")]


class BcmPortsDev(C.Structure):     # dpe_bcm_ports_dev
    _fields_ = [(n, C.c_void_p) for n in ("xCurrkk1", "enu2ecef", "satStates", "codePhaseEnd", "codeFrequency",
                                          "carrierFrequency", "cpRefTOW", "cpElapsedEnd", "cpRef", "dopplerSign")] + \
               [("dimT", C.c_int32), ("reserved", C.c_int32)]


class ChanStart(C.Structure):
    _fields_ = [("codePhaseStart", C.c_double), ("carrierPhaseStart", C.c_double), ("codeFrequency", C.c_double),
                ("carrierFrequency", C.c_double), ("cpElapsedStart", C.c_int32), ("cpReference", C.c_int32),
                ("prn", C.c_int32), ("reserved", C.c_int32)]


class BcmConfig(C.Structure):
    _fields_ = [("samplesPerWindow", C.c_int32), ("lagHalfWidth", C.c_int32), ("binHalfWidth", C.c_int32),
                ("lPower", C.c_int32), ("maxWindows", C.c_int32), ("maxChannels", C.c_int32),
                ("numFFTPoints", C.c_int64), ("samplingFrequency", C.c_double),
                ("posGrid", C.POINTER(C.c_double)), ("velGrid", C.POINTER(C.c_double)),
                ("posGridSize", C.c_int64), ("velGridSize", C.c_int64),
                ("posGridIndexOffset", C.c_int64), ("velGridIndexOffset", C.c_int64),
                ("writeScores", C.c_int32), ("weightedMean", C.c_int32), ("referencePair", C.c_int32), ("reserved", C.c_int32)]


class BcmWindow(C.Structure):
    _fields_ = [("xCurrkk1", C.c_double * 8), ("enu2ecef", C.c_double * 9), ("rxTime", C.c_double),
                ("dopplerSign", C.c_int32), ("reserved", C.c_int32)]


class ChanEnd(C.Structure):
    _fields_ = [("satState", C.c_double * 8), ("codePhaseEnd", C.c_double), ("codeFrequency", C.c_double),
                ("carrierFrequency", C.c_double), ("cpRefTOW", C.c_int32), ("cpElapsedEnd", C.c_int32),
                ("cpRef", C.c_int32), ("reserved", C.c_int32)]


class BcmResult(C.Structure):
    _fields_ = [("zVal", C.c_double * 8), ("posIndex", C.c_int64), ("velIndex", C.c_int64),
                ("posScore", C.c_float), ("velScore", C.c_float), ("posOutOfWindow", C.c_int64),
                ("velOutOfWindow", C.c_int64), ("zValMean", C.c_double * 8), ("weightedSums", (C.c_double * 5) * 2)]


class BcmJointRx(C.Structure):      # dpe_bcm_joint_rx
    _fields_ = [("codeBank_dev", C.c_void_p), ("carrBank_dev", C.c_void_p), ("chan_host", C.POINTER(ChanEnd)), ("win", BcmWindow),
                ("nChan", C.c_int32), ("reserved", C.c_int32)]


class BcmJointResult(C.Structure):  # dpe_bcm_joint_result
    _fields_ = [("posIndex", C.c_int64), ("velIndex", C.c_int64), ("posScore", C.c_float), ("velScore", C.c_float),
                ("offset", C.c_double * 8), ("posOutOfWindow", C.c_int64), ("velOutOfWindow", C.c_int64)]


class BcmJointRxResult(C.Structure):  # dpe_bcm_joint_rx_result
    _fields_ = [("zVal", C.c_double * 8), ("posIndex", C.c_int64), ("velIndex", C.c_int64), ("posScore", C.c_float),
                ("velScore", C.c_float), ("posOutOfWindow", C.c_int64), ("velOutOfWindow", C.c_int64)]


class BcmEpochsResult(C.Structure):  # dpe_bcm_epochs_result
    _fields_ = [("zVal", C.c_double * 8), ("offset", C.c_double * 8), ("posIndex", C.c_int64), ("velIndex", C.c_int64),
                ("posScore", C.c_float), ("velScore", C.c_float), ("posOutOfWindow", C.c_int64), ("velOutOfWindow", C.c_int64),
                ("nPasses", C.c_int32), ("reserved", C.c_int32)]


class BcmSubsetResult(C.Structure):  # dpe_bcm_subset_result
    _fields_ = [("zVal", C.c_double * 8), ("offset", C.c_double * 8), ("posIndex", C.c_int64), ("velIndex", C.c_int64),
                ("posScore", C.c_float), ("velScore", C.c_float), ("posOutOfWindow", C.c_int64), ("velOutOfWindow", C.c_int64)]


REFINE_MAX_LEVELS = 4    # DPE_REFINE_MAX_LEVELS


class BcmRefineResult(C.Structure):  # dpe_bcm_refine_result
    _fields_ = [("zVal", C.c_double * 8), ("offset", C.c_double * 8), ("posIndex", C.c_int64 * REFINE_MAX_LEVELS),
                ("velIndex", C.c_int64 * REFINE_MAX_LEVELS), ("posScore", C.c_float * REFINE_MAX_LEVELS),
                ("velScore", C.c_float * REFINE_MAX_LEVELS), ("posOutOfWindow", C.c_int64 * REFINE_MAX_LEVELS),
                ("velOutOfWindow", C.c_int64 * REFINE_MAX_LEVELS)]


class BcmMomentsConfig(C.Structure):  # dpe_bcm_moments_config
    _fields_ = [("rho", C.c_double * 2), ("keys_dev", C.c_void_p), ("posScores_dev", C.c_void_p), ("velScores_dev", C.c_void_p),
                ("posPitch", C.c_int64), ("velPitch", C.c_int64), ("nWindows", C.c_int32), ("reserved", C.c_int32)]


class BcmMomentsResult(C.Structure):  # dpe_bcm_moments_result
    _fields_ = [("sums", (C.c_double * 15) * 2), ("nAbove", C.c_int64 * 2), ("threshold", C.c_float * 2),
                ("zValMom", C.c_double * 8), ("RValMom", C.c_double * 64)]


MOMENT_NAMES = ("1", "x", "y", "z", "t", "xx", "xy", "xz", "xt", "yy", "yz", "yt", "zz", "zt", "tt")   # the order of sums[m]


CHAN_START_DTYPE = np.dtype([("codePhaseStart", "<f8"), ("carrierPhaseStart", "<f8"), ("codeFrequency", "<f8"),
                             ("carrierFrequency", "<f8"), ("cpElapsedStart", "<i4"), ("cpReference", "<i4"),
                             ("prn", "<i4"), ("reserved", "<i4")])
CHAN_END_DTYPE = np.dtype([("satState", "<f8", (8,)), ("codePhaseEnd", "<f8"), ("codeFrequency", "<f8"),
                           ("carrierFrequency", "<f8"), ("cpRefTOW", "<i4"), ("cpElapsedEnd", "<i4"),
                           ("cpRef", "<i4"), ("reserved", "<i4")])
BCM_WINDOW_DTYPE = np.dtype([("xCurrkk1", "<f8", (8,)), ("enu2ecef", "<f8", (9,)), ("rxTime", "<f8"),
                             ("dopplerSign", "<i4"), ("reserved", "<i4")])
assert CHAN_START_DTYPE.itemsize == C.sizeof(ChanStart)
assert CHAN_END_DTYPE.itemsize == C.sizeof(ChanEnd)
assert BCM_WINDOW_DTYPE.itemsize == C.sizeof(BcmWindow)


def lib():
    """Load libdpe_hip.so (built in-tree by __graft_entry__.build()).  No fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise DpeError("HIP extension %s is missing: run `python -c 'import __graft_entry__ as g; g.build()'`"
                           % LIB_PATH)
        # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64 with the same SONAME as the system one
        # this library links against.  Whichever is loaded first serves both; loading the system runtime first leaves
        # torch with "No HIP GPUs are available".  So torch (when present) goes first.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        _lib = C.CDLL(LIB_PATH)
        _lib.dpe_last_error.restype = C.c_char_p
        _lib.dpe_bcs_stage1_kernel.restype = C.c_char_p
        for name in EXPORTS:
            getattr(_lib, name)  # AttributeError if the ABI is incomplete
    return _lib


def _check(rc):
    if rc != 0:
        raise DpeError(lib().dpe_last_error().decode("utf-8", "replace"))


def _ptr(x):
    """torch tensor / int -> raw device pointer."""
    if hasattr(x, "data_ptr"):
        return C.c_void_p(x.data_ptr())
    return C.c_void_p(int(x))


def _grids(pos_grid, vel_grid, pos_index_offset, vel_index_offset):
    """The two manifold grids as the C-ABI takes them: [G, 4] point lists, or GridAxes (whose slice sets size and index
    offset).  Returns (pos, vel, pos_offset, vel_offset, axes?)."""
    from .grid_axes import GridAxes
    pa, va = isinstance(pos_grid, GridAxes), isinstance(vel_grid, GridAxes)
    if pa != va:
        raise DpeError("[BatchCorrManifold] grids: give both manifolds as GridAxes or both as point lists")
    if pa:
        if pos_index_offset or vel_index_offset:
            raise DpeError("[BatchCorrManifold] grids: a GridAxes slice carries its own index offset (GridAxes.shard)")
        return pos_grid, vel_grid, pos_grid.begin, vel_grid.begin, True
    return (np.ascontiguousarray(pos_grid, dtype=np.float64), np.ascontiguousarray(vel_grid, dtype=np.float64),
            int(pos_index_offset), int(vel_index_offset), False)


def _bcm_config(S, L, B, LPower, W, K, Cf, fs, pos, vel, pos_off, vel_off, axes, write_scores, weighted_mean, reference_pair):
    dp = C.POINTER(C.c_double)
    return BcmConfig(S, L, B, LPower, W, K, Cf, fs, None if axes else pos.ctypes.data_as(dp), None if axes else vel.ctypes.data_as(dp),
                     pos.shape[0], vel.shape[0], pos_off, vel_off, 1 if write_scores else 0, 1 if weighted_mean else 0,
                     1 if reference_pair else 0, 0)


STREAM_NONE = "none"      # Pipe.submit / acquire: the samples are already resident (DPE_STREAM_NONE: no cross-stream wait)


def _stream(stream):
    if isinstance(stream, str) and stream == STREAM_NONE:
        return C.c_void_p(-1)
    if stream is None:
        import torch
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if hasattr(stream, "cuda_stream"):
        return C.c_void_p(stream.cuda_stream)
    return C.c_void_p(int(stream))


class Stream:
    """A HIP stream owned by the library (dpe_stream_create); pass it as ``stream=`` to the modules."""

    def __init__(self):
        self._s = C.c_void_p(None)
        _check(lib().dpe_stream_create(C.byref(self._s)))
        self.cuda_stream = self._s.value

    def synchronize(self):
        _check(lib().dpe_stream_synchronize(self._s))

    def close(self):
        if self._s:
            lib().dpe_stream_destroy(self._s)
            self._s = C.c_void_p(None)
            self.cuda_stream = 0


def carr_fft_len(S):
    p = 1
    while p < S:
        p <<= 1
    return 8 * p


def gen_ca_code():
    out = np.zeros((37, 1023), dtype=np.int8)
    _check(lib().dpe_gen_ca_code(out.ctypes.data_as(C.POINTER(C.c_int8))))
    return out


def device_info():
    name = C.create_string_buffer(128)
    cu, mem = C.c_int(0), C.c_int64(0)
    _check(lib().dpe_device_info(name, 128, C.byref(cu), C.byref(mem)))
    return name.value.decode(), cu.value, mem.value


def hbm_ceiling(bytes_per_array=1 << 30, iters=10, stream=None):
    """Measured stream-copy and triad bandwidth of this device in GB/s (diagnostic; see dpe_hbm_ceiling)."""
    cp, tr = C.c_double(0), C.c_double(0)
    _check(lib().dpe_hbm_ceiling(C.c_int64(bytes_per_array), C.c_int(iters), _stream(stream), C.byref(cp), C.byref(tr)))
    return cp.value, tr.value


def d2h(ptr, nbytes, dtype, stream=None):
    out = np.empty(nbytes // np.dtype(dtype).itemsize, dtype=dtype)
    _check(lib().dpe_memcpy_d2h(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), C.c_int64(nbytes), _stream(stream)))
    return out


def chan_start_array(prn, rc, ri, fc, fi, cp_ela, cp_ref):
    """Pack start-referenced channel params (arrays of shape [W,K] or [K]) for BatchCorrScores."""
    rc = np.asarray(rc, dtype=np.float64)
    a = np.zeros(rc.shape, dtype=CHAN_START_DTYPE)
    a["codePhaseStart"], a["carrierPhaseStart"] = rc, ri
    a["codeFrequency"], a["carrierFrequency"] = fc, fi
    a["cpElapsedStart"], a["cpReference"], a["prn"] = cp_ela, cp_ref, prn
    return a


def chan_end_array(sat, rc_end, fc, fi, cp_ref_tow, cp_ela_end, cp_ref):
    rc_end = np.asarray(rc_end, dtype=np.float64)
    a = np.zeros(rc_end.shape, dtype=CHAN_END_DTYPE)
    a["satState"] = sat
    a["codePhaseEnd"], a["codeFrequency"], a["carrierFrequency"] = rc_end, fc, fi
    a["cpRefTOW"], a["cpElapsedEnd"], a["cpRef"] = cp_ref_tow, cp_ela_end, cp_ref
    return a


def bcm_window_array(x_kk1, enu2ecef, rx_time, doppler_sign=1):
    rx_time = np.atleast_1d(np.asarray(rx_time, dtype=np.float64))
    a = np.zeros(rx_time.shape, dtype=BCM_WINDOW_DTYPE)
    a["xCurrkk1"] = x_kk1
    a["enu2ecef"] = np.asarray(enu2ecef).reshape(rx_time.shape + (9,))
    a["rxTime"] = rx_time
    a["dopplerSign"] = doppler_sign
    return a


class BatchCorrScores:
    """Module "BatchCorrScores" (batchcorrscores.cu:674-700): Start/Update/Stop + output ports."""

    def __init__(self, SamplingFrequency, SampleLength=None, samples_per_window=None, lag_half_width=8,
                 bin_half_width=48, max_windows=1, max_channels=8):
        S = int(samples_per_window) if samples_per_window is not None else int(round(SamplingFrequency * SampleLength))
        self.S, self.fs = S, float(SamplingFrequency)
        self.L, self.B = int(lag_half_width), int(bin_half_width)
        self.max_windows, self.max_channels = int(max_windows), int(max_channels)
        self._h = C.c_void_p(None)
        self.Started = False

    def Start(self):
        if self.Started:
            return 0
        cfg = BcsConfig(self.S, self.L, self.B, self.max_windows, self.max_channels, 0, self.fs)
        _check(lib().dpe_bcs_create(C.byref(cfg), C.byref(self._h)))
        code, carr = C.c_void_p(), C.c_void_p()
        nlag, nbin, nfft = C.c_int32(), C.c_int32(), C.c_int64()
        _check(lib().dpe_bcs_outputs(self._h, C.byref(code), C.byref(carr), C.byref(nlag), C.byref(nbin), C.byref(nfft)))
        self.CodeScores, self.CarrScores = code.value, carr.value     # device pointers (float2 banks)
        self.nLag, self.nBin, self.NumFFTPoints = nlag.value, nbin.value, nfft.value
        self.Started = True
        self._W = self._K = 0
        return 0

    def Update(self, Samples, chan, window_stride=None, stream=None):
        """Samples: device int16 [W, 2*S] (torch tensor or raw pointer); chan: CHAN_START_DTYPE [W,K]."""
        if not self.Started:
            raise DpeError("[BatchCorrScores] Error: Update() Failed due to batch correlator not initialized")
        chan = np.ascontiguousarray(chan)
        if chan.ndim == 1:
            chan = chan[None, :]
        W, K = chan.shape
        stride = self.S if window_stride is None else int(window_stride)
        _check(lib().dpe_bcs_update(self._h, _ptr(Samples), C.c_int64(stride), C.c_int32(W), C.c_int32(K),
                                    chan.ctypes.data_as(C.POINTER(ChanStart)), _stream(stream)))
        self._W, self._K = W, K
        return 0

    def UpdateDev(self, Samples, n_chan, ports, stream=None):
        """One window with the channel parameters in DEVICE arrays (dpe_bcs_update_dev): ports = {field: device pointer}
        with the fields of dpe_bcs_ports_dev."""
        if not self.Started:
            raise DpeError("[BatchCorrScores] Error: Update() Failed due to batch correlator not initialized")
        p = BcsPortsDev(**{k: _ptr(v).value for k, v in ports.items()})
        _check(lib().dpe_bcs_update_dev(self._h, _ptr(Samples), C.c_int32(n_chan), C.byref(p), _stream(stream)))
        self._W, self._K = 1, int(n_chan)
        return 0

    def UpdatePrepared(self, Samples, n_chan, stream=None):
        """One window whose channel block an attached ChanMgrDev has already written on the device."""
        _check(lib().dpe_bcs_update_prepared(self._h, _ptr(Samples), C.c_int32(n_chan), _stream(stream)))
        self._W, self._K = 1, int(n_chan)
        return 0

    def allgather_banks(self, comm, code_all, carr_all, stream=None):
        """Stage 1 sharded by window: this rank's banks of the last Update into code_all / carr_all (device pointers,
        [nRanks * W_local][maxChannels][2L+1 | 2B+1] float2), rank-major (dpe_bcs_allgather_banks)."""
        _check(lib().dpe_bcs_allgather_banks(self._h, comm._h, _ptr(code_all), _ptr(carr_all), _stream(stream)))

    def set_dev_hint(self, flags=1):
        """dpe_bcs_set_dev_hint: flags bit 0 = the chip kernels' conditions hold for every channel (no readback in UpdateDev)."""
        _check(lib().dpe_bcs_set_dev_hint(self._h, C.c_int32(flags)))

    def dev_status(self, stream=None):
        st = C.c_int32()
        _check(lib().dpe_bcs_dev_status(self._h, C.byref(st), _stream(stream)))
        return st.value

    def set_graph(self, enable=True):
        """Replay repeated Updates as one hipGraph launch (needs a created stream, see dpe_hip.h)."""
        _check(lib().dpe_bcs_set_graph(self._h, C.c_int32(1 if enable else 0)))

    PROFILE_SLOTS = ("bcs_sum", "bcs_bank", "bcs_finalize")

    def profile(self, enable=True):
        """-> {kernel: (total_ms, launches)} since the previous call; sets the enable flag.
        enable: False / True (every kernel) / one of PROFILE_SLOTS (events around that kernel only)."""
        ms, cnt = (C.c_float * 3)(), (C.c_int32 * 3)()
        code = 2 << self.PROFILE_SLOTS.index(enable) if isinstance(enable, str) else (1 if enable else 0)
        _check(lib().dpe_bcs_profile(self._h, C.c_int32(code), ms, cnt))
        return {n: (ms[i], cnt[i]) for i, n in enumerate(self.PROFILE_SLOTS)}

    @property
    def stage1_kernel(self):
        return lib().dpe_bcs_stage1_kernel(self._h).decode()

    def Stop(self):
        if self.Started:
            if getattr(self, "_owned", True):      # (a lane of a Pipe is destroyed by the pipe)
                _check(lib().dpe_bcs_destroy(self._h))
            self._h = C.c_void_p(None)
            self.Started = False
        return 0

    @classmethod
    def _adopt(cls, handle, fs, S, L, B, max_windows, max_channels):
        """Python face of a handle that a dpe_pipe owns."""
        self = cls(fs, samples_per_window=S, lag_half_width=L, bin_half_width=B, max_windows=max_windows, max_channels=max_channels)
        self._h, self._owned = C.c_void_p(handle), False
        code, carr = C.c_void_p(), C.c_void_p()
        nlag, nbin, nfft = C.c_int32(), C.c_int32(), C.c_int64()
        _check(lib().dpe_bcs_outputs(self._h, C.byref(code), C.byref(carr), C.byref(nlag), C.byref(nbin), C.byref(nfft)))
        self.CodeScores, self.CarrScores = code.value, carr.value
        self.nLag, self.nBin, self.NumFFTPoints = nlag.value, nbin.value, nfft.value
        self.Started = True
        self._W = self._K = 0
        return self

    def __del__(self):
        try:            # at interpreter shutdown module globals may already be gone
            self.Stop()
        except Exception:
            pass

    # ---- host-side readers (tests / diagnostics)
    def read_banks(self, stream=None):
        W, K = self._W, self._K
        code = d2h(self.CodeScores, self.max_windows * self.max_channels * self.nLag * 8, np.complex64, stream)
        carr = d2h(self.CarrScores, self.max_windows * self.max_channels * self.nBin * 8, np.complex64, stream)
        code = code.reshape(self.max_windows, self.max_channels, self.nLag)[:W, :K]
        carr = carr.reshape(self.max_windows, self.max_channels, self.nBin)[:W, :K]
        return code, carr

    def read_info(self, stream=None):
        n = self._W * self._K
        idx = np.zeros(n, dtype=np.int32)
        nfl = np.zeros(n, dtype=np.int32)
        mean = np.zeros(2 * self._W)
        _check(lib().dpe_bcs_read_info(self._h, idx.ctypes.data_as(C.POINTER(C.c_int32)),
                                       nfl.ctypes.data_as(C.POINTER(C.c_int32)),
                                       mean.ctypes.data_as(C.POINTER(C.c_double)), _stream(stream)))
        return (idx.reshape(self._W, self._K), nfl.reshape(self._W, self._K).astype(bool),
                mean.reshape(self._W, 2).view(np.complex128).ravel())

    def export_dense(self, window, code_dev, carr_dev, stream=None):
        _check(lib().dpe_bcs_export_dense(self._h, C.c_int32(window), _ptr(code_dev) if code_dev is not None else None,
                                          _ptr(carr_dev) if carr_dev is not None else None, _stream(stream)))


class Comm:
    """dpe_comm: the multi-GPU exchange behind the C-ABI (RCCL, or host files for one-GPU functional tests)."""
    RCCL, HOSTFILES = 0, 1

    def __init__(self, rank, n_ranks, rendezvous="", backend=0):
        self._h = C.c_void_p(None)
        _check(lib().dpe_comm_create(C.c_int32(rank), C.c_int32(n_ranks), rendezvous.encode(), C.c_int32(backend), C.byref(self._h)))
        self.rank, self.n_ranks = rank, n_ranks

    def allreduce_max_u64(self, dev_ptr, count, stream=None):
        _check(lib().dpe_comm_allreduce_max_u64(self._h, C.c_void_p(dev_ptr), C.c_int64(count), _stream(stream)))

    def close(self):
        if self._h:
            lib().dpe_comm_destroy(self._h)
            self._h = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _win_chan(win, chan):
    """The win / chan arguments of a manifold's Update as contiguous arrays [W] and [W, K] -> (win, chan, W, K)."""
    win = np.ascontiguousarray(np.atleast_1d(win))
    chan = np.ascontiguousarray(chan)
    if chan.ndim == 1:
        chan = chan[None, :]
    return (win, chan) + chan.shape


def moments_from_sums(sums, centre, enu2ecef):
    """dpe_bcm_moments_from_sums (host only): sums [2, 15] -- one handle's, or the all-reduced sums of shards -- to
    (zValMom [8], RValMom [8, 8]) about `centre` [8] in the frame of zVal (enu2ecef: the window's 3x3 matrix, row-major)."""
    s = np.ascontiguousarray(sums, dtype=np.float64).reshape(2, 15)
    c = np.ascontiguousarray(centre, dtype=np.float64).reshape(8)
    R = np.ascontiguousarray(enu2ecef, dtype=np.float64).reshape(9)
    z, Rv = np.zeros(8), np.zeros(64)
    dp = C.POINTER(C.c_double)
    _check(lib().dpe_bcm_moments_from_sums(s.ctypes.data_as(dp), c.ctypes.data_as(dp), R.ctypes.data_as(dp), z.ctypes.data_as(dp),
                                           Rv.ctypes.data_as(dp)))
    return z, Rv.reshape(8, 8)


def moments_rval(sums, enu2ecef, floor_var):
    """dpe_bcm_moments_rval (host only): the measurement covariance a filter takes from a window's sums [2, 15] in the frame given
    by enu2ecef: per manifold RValMom's block plus the grid's quantisation floor J diag(floor_var[m]) J^T (floor_var [2, 4]:
    pipeline.quantisation_floor of the position and the velocity grid).  A block that is not finite (no point above the threshold)
    becomes the identity.  Returns (R [8, 8], fallback: bit m set where block m is the identity).  The device-resident loop forms
    its R with the same function (ChanMgrDev.set_measurement_cov)."""
    s = np.ascontiguousarray(sums, dtype=np.float64).reshape(2, 15)
    R = np.ascontiguousarray(enu2ecef, dtype=np.float64).reshape(9)
    f = np.ascontiguousarray(floor_var, dtype=np.float64).reshape(2, 4)
    out, fb = np.zeros(64), C.c_int32(0)
    dp = C.POINTER(C.c_double)
    _check(lib().dpe_bcm_moments_rval(s.ctypes.data_as(dp), R.ctypes.data_as(dp), f.ctypes.data_as(dp), out.ctypes.data_as(dp), C.byref(fb)))
    return out.reshape(8, 8), int(fb.value)


class BatchCorrManifold:
    """Module "BatchCorrManifold" (batchcorrmanifold.cu:2247-2303): params PosGrid/VelGrid (host
    [G,4] ENU offsets, i.e. the LoadPosGrid path :2422-2448 generalised to both manifolds), LPower."""

    def __init__(self, SamplingFrequency, samples_per_window, NumFFTPoints, pos_grid, vel_grid, LPower=1,
                 lag_half_width=8, bin_half_width=48, max_windows=1, max_channels=8, write_scores=True,
                 pos_index_offset=0, vel_index_offset=0, weighted_mean=False, reference_pair=False):
        self.fs, self.S, self.C = float(SamplingFrequency), int(samples_per_window), int(NumFFTPoints)
        # [G, 4] point lists, or GridAxes (grid_axes.py): then the handle never holds a per-point copy of the grid
        self.pos_grid, self.vel_grid, pos_index_offset, vel_index_offset, self.axes = _grids(pos_grid, vel_grid, pos_index_offset,
                                                                                            vel_index_offset)
        self.LPower, self.L, self.B = int(LPower), int(lag_half_width), int(bin_half_width)
        self.max_windows, self.max_channels = int(max_windows), int(max_channels)
        self.write_scores = bool(write_scores)
        self.weighted_mean = bool(weighted_mean)
        self.reference_pair = bool(reference_pair)
        self.pos_off, self.vel_off = int(pos_index_offset), int(vel_index_offset)
        self._h = C.c_void_p(None)
        self.Started = False

    def Start(self):
        if self.Started:
            return 0
        cfg = _bcm_config(self.S, self.L, self.B, self.LPower, self.max_windows, self.max_channels, self.C, self.fs, self.pos_grid,
                          self.vel_grid, self.pos_off, self.vel_off, self.axes, self.write_scores, self.weighted_mean, self.reference_pair)
        if self.axes:
            pa, va = self.pos_grid.c_struct(), self.vel_grid.c_struct()
            _check(lib().dpe_bcm_create_axes(C.byref(cfg), C.byref(pa), C.byref(va), C.byref(self._h)))
        else:
            _check(lib().dpe_bcm_create(C.byref(cfg), C.byref(self._h)))
        self._bind_outputs()
        return 0

    def Update(self, CodeScores, CarrScores, win, chan, stream=None):
        """win: BCM_WINDOW_DTYPE [W]; chan: CHAN_END_DTYPE [W,K]; banks: device pointers from BCS."""
        if not self.Started:
            raise DpeError("[BatchCorrManifold] Error: Update() Failed due to module not initialized")
        win, chan, W, K = _win_chan(win, chan)
        assert win.shape[0] == W
        _check(lib().dpe_bcm_update(self._h, _ptr(CodeScores), _ptr(CarrScores), C.c_int32(W), C.c_int32(K),
                                    win.ctypes.data_as(C.POINTER(BcmWindow)),
                                    chan.ctypes.data_as(C.POINTER(ChanEnd)), _stream(stream)))
        self._W = W
        self._refresh_keys()
        return 0

    def UpdateDev(self, CodeScores, CarrScores, n_chan, ports, dim_t, rx_time, stream=None):
        """One window with the inputs in DEVICE arrays (dpe_bcm_update_dev): ports = {field: device pointer} with the
        pointer fields of dpe_bcm_ports_dev."""
        if not self.Started:
            raise DpeError("[BatchCorrManifold] Error: Update() Failed due to module not initialized")
        p = BcmPortsDev(dimT=int(dim_t), reserved=0, **{k: _ptr(v).value for k, v in ports.items()})
        _check(lib().dpe_bcm_update_dev(self._h, _ptr(CodeScores), _ptr(CarrScores), C.c_int32(n_chan), C.byref(p),
                                        C.c_double(rx_time), _stream(stream)))
        self._W = 1
        self._refresh_keys()
        return 0

    def UpdatePrepared(self, CodeScores, CarrScores, n_chan, stream=None):
        """One window whose coefficient blocks an attached ChanMgrDev has already written on the device."""
        _check(lib().dpe_bcm_update_prepared(self._h, _ptr(CodeScores), _ptr(CarrScores), C.c_int32(n_chan), _stream(stream)))
        self._W = 1
        return 0

    def results(self, stream=None):
        res = (BcmResult * self._W)()
        _check(lib().dpe_bcm_results(self._h, res, _stream(stream)))
        return [dict(zVal=np.array(r.zVal), RVal=np.eye(8), posIndex=r.posIndex, velIndex=r.velIndex,
                     posScore=r.posScore, velScore=r.velScore, posOutOfWindow=r.posOutOfWindow,
                     velOutOfWindow=r.velOutOfWindow, zValMean=np.array(r.zValMean),
                     weightedSums=np.array([list(r.weightedSums[0]), list(r.weightedSums[1])])) for r in res]

    def exchange_keys(self, comm, stream=None, to_host=True):
        """All-reduce(MAX) of the last Update's packed keys across the ranks of `comm` (dpe_bcm_exchange_keys);
        returns the reduced host keys [W, 2] for results_from_keys (to_host=False: in place on the device only, asynchronous)."""
        if not to_host:
            _check(lib().dpe_bcm_exchange_keys(self._h, comm._h, None, _stream(stream)))
            return None
        keys = np.zeros((self._W, 2), dtype=np.uint64)
        _check(lib().dpe_bcm_exchange_keys(self._h, comm._h, keys.ctypes.data_as(C.POINTER(C.c_uint64)), _stream(stream)))
        return keys

    def results_from_keys(self, keys_host, pos_grid_global=None, vel_grid_global=None):
        """Measurement from reduced keys.  The global grids may be None (or GridAxes) for a handle made from GridAxes: it then
        decodes from its own axes, which are the global ones."""
        from .grid_axes import GridAxes
        keys_host = np.ascontiguousarray(keys_host, dtype=np.uint64)
        W = keys_host.shape[0]
        dp = C.POINTER(C.c_double)
        if pos_grid_global is None or isinstance(pos_grid_global, GridAxes):
            if not (vel_grid_global is None or isinstance(vel_grid_global, GridAxes)):
                raise DpeError("[BatchCorrManifold] results_from_keys: both global grids as point lists, or neither")
            args = (None, C.c_int64(0), None, C.c_int64(0))
        else:
            pg = np.ascontiguousarray(pos_grid_global, dtype=np.float64)
            vg = np.ascontiguousarray(vel_grid_global, dtype=np.float64)
            args = (pg.ctypes.data_as(dp), C.c_int64(pg.shape[0]), vg.ctypes.data_as(dp), C.c_int64(vg.shape[0]))
        res = (BcmResult * W)()
        _check(lib().dpe_bcm_results_from_keys(self._h, keys_host.ctypes.data_as(C.POINTER(C.c_uint64)), C.c_int32(W), *args, res))
        return [dict(zVal=np.array(r.zVal), posIndex=r.posIndex, velIndex=r.velIndex, posScore=r.posScore,
                     velScore=r.velScore) for r in res]

    def last_split(self):
        """(position, velocity) blocks per window or group of the last Update (dpe_bcm_last_split): with fewer blocks than
        1024-point tiles a block walks several tiles."""
        split = (C.c_int32 * 2)()
        _check(lib().dpe_bcm_last_split(self._h, split))
        return (int(split[0]), int(split[1]))

    def moments(self, rho, keys=None, pos_scores=None, vel_scores=None, n_windows=None, stream=None):
        """Thresholded moments of the last Update's score rows (dpe_bcm_moments + dpe_bcm_moments_results): weights
        max(score - rho * max, 0) per manifold, rho = (rho_pos, rho_vel) or one value for both.  keys: device uint64 [W, 2] to take
        the rows' maxima from (default: the last Update's own, exchanged if exchange_keys ran); pos_scores / vel_scores: rows to
        read instead of the handle's own -- a 2-D float32 device tensor (pitch = its row stride) or (device pointer, pitch).
        Returns one dict per window: sums [2, 15] (order MOMENT_NAMES), nAbove [2], threshold [2], zValMom [8], RValMom [8, 8]."""
        if not self.Started:
            raise DpeError("[BatchCorrManifold] Error: moments() Failed due to module not initialized")
        rp, rv = (rho, rho) if np.isscalar(rho) else rho

        def rows(x):
            if x is None:
                return None, 0
            if hasattr(x, "data_ptr"):
                if x.dim() != 2 or x.stride(1) != 1 or x.element_size() != 4:
                    raise DpeError("[BatchCorrManifold] moments: override rows must be a 2-D float32 tensor with contiguous rows")
                return x.data_ptr(), x.stride(0)
            return _ptr(x[0]).value, int(x[1])
        (pp, ppitch), (vp, vpitch) = rows(pos_scores), rows(vel_scores)
        cfg = BcmMomentsConfig((C.c_double * 2)(float(rp), float(rv)), None if keys is None else _ptr(keys).value, pp, vp, ppitch, vpitch,
                               0 if n_windows is None else int(n_windows), 0)
        _check(lib().dpe_bcm_moments(self._h, C.byref(cfg), _stream(stream)))
        W = self._W if n_windows is None else int(n_windows)
        res = (BcmMomentsResult * W)()
        _check(lib().dpe_bcm_moments_results(self._h, res, _stream(stream)))
        return [dict(sums=np.array([list(r.sums[0]), list(r.sums[1])]), nAbove=np.array(r.nAbove, dtype=np.int64),
                     threshold=np.array(r.threshold, dtype=np.float32), zValMom=np.array(r.zValMom),
                     RValMom=np.array(r.RValMom).reshape(8, 8)) for r in res]

    def moments_dev(self):
        """Device pointers of the last moments call's sums (double [max_windows, 2, 15]) and counts (int64 [max_windows, 2])."""
        s, n = C.c_void_p(), C.c_void_p()
        _check(lib().dpe_bcm_moments_dev(self._h, C.byref(s), C.byref(n)))
        return s.value, n.value

    def read_scores(self, stream=None):
        Gp, Gv = self.pos_grid.shape[0], self.vel_grid.shape[0]
        ps = d2h(self.PosScores, self._W * self.PosScoresPitch * 4, np.float32, stream).reshape(self._W, self.PosScoresPitch)[:, :Gp]
        vs = d2h(self.VelScores, self._W * self.VelScoresPitch * 4, np.float32, stream).reshape(self._W, self.VelScoresPitch)[:, :Gv]
        return np.ascontiguousarray(ps), np.ascontiguousarray(vs)

    def export_scores_f64(self, window, pos_dev, vel_dev, stream=None):
        """PosScores / its velocity twin as the reference's dense fp64 rows (dpe_bcm_export_scores_f64)."""
        _check(lib().dpe_bcm_export_scores_f64(self._h, C.c_int32(window), _ptr(pos_dev) if pos_dev is not None else None,
                                               _ptr(vel_dev) if vel_dev is not None else None, _stream(stream)))

    def set_graph(self, enable=True):
        """Replay repeated Updates as one hipGraph launch (needs a created stream, see dpe_hip.h)."""
        _check(lib().dpe_bcm_set_graph(self._h, C.c_int32(1 if enable else 0)))

    def profile(self, enable=True):
        ms, cnt = (C.c_float * 2)(), (C.c_int32 * 2)()
        _check(lib().dpe_bcm_profile(self._h, C.c_int32(1 if enable else 0), ms, cnt))
        return {"bcm_scan": (ms[0], cnt[0])}   # one fused launch scores both manifolds

    def Stop(self):
        if self.Started:
            if getattr(self, "_owned", True):      # (a lane of a Pipe is destroyed by the pipe)
                _check(lib().dpe_bcm_destroy(self._h))
            self._h = C.c_void_p(None)
            self.Started = False
        return 0

    def _refresh_keys(self):
        keys = C.c_void_p()   # the key sets alternate between Updates: refresh the device pointer
        _check(lib().dpe_bcm_keys(self._h, C.byref(keys)))
        self.Keys = keys.value

    def _bind_outputs(self):
        self.PosScores = self.VelScores = None
        if self.write_scores:
            ps, vs = C.c_void_p(), C.c_void_p()
            _check(lib().dpe_bcm_scores(self._h, C.byref(ps), C.byref(vs)))
            self.PosScores, self.VelScores = ps.value, vs.value
        pp, vp = C.c_int64(), C.c_int64()
        _check(lib().dpe_bcm_scores_pitch(self._h, C.byref(pp), C.byref(vp)))
        self.PosScoresPitch, self.VelScoresPitch = pp.value, vp.value     # floats between the rows of consecutive windows
        self._refresh_keys()
        self.Started = True
        self._W = 0

    @classmethod
    def _adopt(cls, handle, *args, **kw):
        """Python face of a handle that a dpe_pipe owns."""
        self = cls(*args, **kw)
        self._h, self._owned = C.c_void_p(handle), False
        self._bind_outputs()
        return self

    def __del__(self):
        try:            # at interpreter shutdown module globals may already be gone
            self.Stop()
        except Exception:
            pass


class JointManifold(BatchCorrManifold):
    """Several receivers over one pair of grids (dpe_bcm_create_joint): PyGNSS' multi receiver mode
    (receiver.py:266-274,337-345,385-388) as one launch.  max_channels bounds one receiver, max_channels_total the
    (receiver, SV) pairs of a window.  PosScores / VelScores / Keys are the JOINT rows and keys."""

    def __init__(self, SamplingFrequency, samples_per_window, NumFFTPoints, pos_grid, vel_grid, max_rx, max_channels_total, LPower=1,
                 lag_half_width=8, bin_half_width=48, max_windows=1, max_channels=8, write_scores=True, own_keys=True):
        super().__init__(SamplingFrequency, samples_per_window, NumFFTPoints, pos_grid, vel_grid, LPower=LPower,
                         lag_half_width=lag_half_width, bin_half_width=bin_half_width, max_windows=max_windows,
                         max_channels=max_channels, write_scores=write_scores)
        if self.axes:
            raise DpeError("[BatchCorrManifold] create_joint: point-list grids only (GridAxes are not supported)")
        self.max_rx, self.max_channels_total, self.own_keys = int(max_rx), int(max_channels_total), bool(own_keys)
        self._nRx = 0

    def Start(self):
        if self.Started:
            return 0
        cfg = _bcm_config(self.S, self.L, self.B, self.LPower, self.max_windows, self.max_channels, self.C, self.fs, self.pos_grid,
                          self.vel_grid, 0, 0, False, self.write_scores, False, False)
        _check(lib().dpe_bcm_create_joint(C.byref(cfg), C.c_int32(self.max_rx), C.c_int32(self.max_channels_total), C.byref(self._h)))
        self._bind_outputs()
        self.set_own_keys(self.own_keys)
        return 0

    def set_own_keys(self, enable=True):
        """Keep (default) or drop the per-receiver arg-max of the following Updates; the joint bits are the same either way."""
        _check(lib().dpe_bcm_joint_set_own_keys(self._h, C.c_int32(1 if enable else 0)))
        self.own_keys = bool(enable)

    @staticmethod
    def pack(rx):
        """rx: [W][nRx] (or [nRx] for one window) of dicts {code, carr: device pointers to that receiver's bank rows of the
        window, win: BCM_WINDOW_DTYPE scalar / [1], chan: CHAN_END_DTYPE [K_r]} -> the dpe_bcm_joint_rx array Update takes
        (a caller that repeats an Update packs once)."""
        if rx and isinstance(rx[0], dict):
            rx = [rx]
        W, nRx = len(rx), len(rx[0])
        arr = (BcmJointRx * (W * nRx))()
        keep = []
        for w, row in enumerate(rx):
            if len(row) != nRx:
                raise DpeError("[BatchCorrManifold] update_joint: every window needs the same number of receivers")
            for r, d in enumerate(row):
                chan = np.ascontiguousarray(d["chan"], dtype=CHAN_END_DTYPE).reshape(-1)
                win = np.ascontiguousarray(np.atleast_1d(d["win"]), dtype=BCM_WINDOW_DTYPE)
                keep += [chan, win]
                a = arr[w * nRx + r]
                a.codeBank_dev, a.carrBank_dev = _ptr(d["code"]).value, _ptr(d["carr"]).value
                a.chan_host = chan.ctypes.data_as(C.POINTER(ChanEnd))
                C.memmove(C.byref(a.win), win.ctypes.data, C.sizeof(BcmWindow))
                a.nChan, a.reserved = chan.shape[0], 0
        return (arr, keep, W, nRx)

    def Update(self, rx, stream=None):
        """rx: what pack() takes, or its result."""
        if not self.Started:
            raise DpeError("[BatchCorrManifold] Error: Update() Failed due to module not initialized")
        arr, _keep, W, nRx = rx if isinstance(rx, tuple) else self.pack(rx)
        _check(lib().dpe_bcm_update_joint(self._h, C.c_int32(W), C.c_int32(nRx), arr, _stream(stream)))
        self._W, self._nRx = W, nRx
        self._refresh_keys()
        return 0

    def results(self, stream=None):
        """-> per window a dict: the joint arg-max (posIndex, velIndex, posScore, velScore, offset[8], out-of-window counts) and
        rx = [per receiver: zVal (its centre moved by the joint offset), its own arg-max and out-of-window counts]."""
        jr = (BcmJointResult * self._W)()
        pr = (BcmJointRxResult * (self._W * self._nRx))()
        _check(lib().dpe_bcm_results_joint(self._h, jr, pr, _stream(stream)))
        out = []
        for w, j in enumerate(jr):
            rxs = [dict(zVal=np.array(o.zVal), RVal=np.eye(8), posIndex=o.posIndex, velIndex=o.velIndex, posScore=o.posScore,
                        velScore=o.velScore, posOutOfWindow=o.posOutOfWindow, velOutOfWindow=o.velOutOfWindow)
                   for o in pr[w * self._nRx:(w + 1) * self._nRx]]
            out.append(dict(posIndex=j.posIndex, velIndex=j.velIndex, posScore=j.posScore, velScore=j.velScore,
                            offset=np.array(j.offset), posOutOfWindow=j.posOutOfWindow, velOutOfWindow=j.velOutOfWindow, rx=rxs))
        return out

    def read_keys(self, stream=None):
        """The joint packed keys of the last Update, uint64 [W, 2] (dpe_bcm_keys)."""
        return d2h(self.Keys, self._W * 2 * 8, np.uint64, stream).reshape(self._W, 2)

    def UpdateDev(self, *a, **k):
        raise DpeError("[BatchCorrManifold] a joint handle takes its inputs through Update(rx) only")

    UpdatePrepared = exchange_keys = results_from_keys = UpdateDev


class EpochManifold(BatchCorrManifold):
    """N consecutive windows summed into one score row and one arg-max (dpe_bcm_create_epochs): non-coherent accumulation
    over epochs along the predicted trajectory.  max_windows bounds the windows of a launch (groups x epochs), max_epochs the
    windows of a group; pairs_per_pass = 0 lets a pass hold as many whole windows as the LDS budget allows, a positive value caps
    the (window, SV) pairs of a pass.  PosScores / VelScores / Keys are the GROUP rows and keys."""

    def __init__(self, SamplingFrequency, samples_per_window, NumFFTPoints, pos_grid, vel_grid, max_epochs, pairs_per_pass=0, LPower=1,
                 lag_half_width=8, bin_half_width=48, max_windows=None, max_channels=8):
        super().__init__(SamplingFrequency, samples_per_window, NumFFTPoints, pos_grid, vel_grid, LPower=LPower,
                         lag_half_width=lag_half_width, bin_half_width=bin_half_width,
                         max_windows=max_epochs if max_windows is None else max_windows, max_channels=max_channels, write_scores=True)
        if self.axes:
            raise DpeError("[BatchCorrManifold] create_epochs: point-list grids only (GridAxes are not supported)")
        self.max_epochs, self.pairs_per_pass = int(max_epochs), int(pairs_per_pass)
        self.n_epochs = 0

    def Start(self):
        if self.Started:
            return 0
        cfg = _bcm_config(self.S, self.L, self.B, self.LPower, self.max_windows, self.max_channels, self.C, self.fs, self.pos_grid,
                          self.vel_grid, 0, 0, False, True, False, False)
        _check(lib().dpe_bcm_create_epochs(C.byref(cfg), C.c_int32(self.max_epochs), C.c_int32(self.pairs_per_pass), C.byref(self._h)))
        self._bind_outputs()
        return 0

    def Update(self, CodeScores, CarrScores, win, chan, n_epochs, stream=None):
        """win: BCM_WINDOW_DTYPE [G * n_epochs]; chan: CHAN_END_DTYPE [G * n_epochs, K], group-major; banks: the device pointers
        of a BatchCorrScores updated with the same windows."""
        if not self.Started:
            raise DpeError("[BatchCorrManifold] Error: Update() Failed due to module not initialized")
        win, chan, W, K = _win_chan(win, chan)
        n_epochs = int(n_epochs)
        if win.shape[0] != W or n_epochs < 1 or W % n_epochs:
            raise DpeError("[BatchCorrManifold] update_epochs: %d windows are not whole groups of %d" % (W, n_epochs))
        _check(lib().dpe_bcm_update_epochs(self._h, _ptr(CodeScores), _ptr(CarrScores), C.c_int32(W // n_epochs), C.c_int32(n_epochs),
                                           C.c_int32(K), win.ctypes.data_as(C.POINTER(BcmWindow)),
                                           chan.ctypes.data_as(C.POINTER(ChanEnd)), _stream(stream)))
        self._W, self.n_epochs = W // n_epochs, n_epochs          # rows, keys and results are per GROUP
        self._refresh_keys()
        return 0

    def results(self, stream=None):
        """-> per group a dict: zVal (the last window's centre moved by the ML offset), the arg-max of the summed rows, offset[8],
        the summed out-of-window counts and nPasses."""
        res = (BcmEpochsResult * self._W)()
        _check(lib().dpe_bcm_results_epochs(self._h, res, _stream(stream)))
        return [dict(zVal=np.array(r.zVal), RVal=np.eye(8), offset=np.array(r.offset), posIndex=r.posIndex, velIndex=r.velIndex,
                     posScore=r.posScore, velScore=r.velScore, posOutOfWindow=r.posOutOfWindow, velOutOfWindow=r.velOutOfWindow,
                     nPasses=r.nPasses) for r in res]

    def read_keys(self, stream=None):
        """The groups' packed keys of the last Update, uint64 [G, 2] (dpe_bcm_keys)."""
        return d2h(self.Keys, self._W * 2 * 8, np.uint64, stream).reshape(self._W, 2)

    def UpdateDev(self, *a, **k):
        raise DpeError("[BatchCorrManifold] an epochs handle takes its inputs through Update(..., n_epochs) only")

    UpdatePrepared = exchange_keys = results_from_keys = UpdateDev


SUBSET_MAX = 16      # kSubsetMax: subsets per window of one scan


def leave_one_out_masks(K):
    """The K single-SV exclusions of K channels as uint64 masks [K]: mask j holds every channel but j."""
    K = int(K)
    if not 2 <= K <= 64:
        raise DpeError("[BatchCorrManifold] leave_one_out_masks: K %d out of range (2 .. 64)" % K)
    full = (1 << K) - 1
    return np.array([full & ~(1 << j) for j in range(K)], dtype=np.uint64)


class SubsetManifold(BatchCorrManifold):
    """The arg-max of every SV subset of a window from one scan (dpe_bcm_create_subsets): solution separation / fault exclusion.
    A subset is a uint64 mask over the window's channels; its key, fix and out-of-window count carry the bits of an Update on those
    channels alone.  PosScores / VelScores / Keys are the FULL set's rows and keys; subset rows are not written."""

    def __init__(self, SamplingFrequency, samples_per_window, NumFFTPoints, pos_grid, vel_grid, max_subsets, LPower=1,
                 lag_half_width=8, bin_half_width=48, max_windows=1, max_channels=8, write_scores=True):
        super().__init__(SamplingFrequency, samples_per_window, NumFFTPoints, pos_grid, vel_grid, LPower=LPower,
                         lag_half_width=lag_half_width, bin_half_width=bin_half_width, max_windows=max_windows,
                         max_channels=max_channels, write_scores=write_scores)
        if self.axes:
            raise DpeError("[BatchCorrManifold] create_subsets: point-list grids only (GridAxes are not supported)")
        self.max_subsets = int(max_subsets)
        self._M = self._K = 0

    def Start(self):
        if self.Started:
            return 0
        cfg = _bcm_config(self.S, self.L, self.B, self.LPower, self.max_windows, self.max_channels, self.C, self.fs, self.pos_grid,
                          self.vel_grid, 0, 0, False, self.write_scores, False, False)
        _check(lib().dpe_bcm_create_subsets(C.byref(cfg), C.c_int32(self.max_subsets), C.byref(self._h)))
        self._bind_outputs()
        return 0

    def Update(self, CodeScores, CarrScores, win, chan, masks=None, stream=None):
        """win, chan, banks as for BatchCorrManifold.Update; masks: uint64 [M] (the same subsets for every window) or [W, M];
        None or empty: the plain scan."""
        if not self.Started:
            raise DpeError("[BatchCorrManifold] Error: Update() Failed due to module not initialized")
        win, chan, W, K = _win_chan(win, chan)
        assert win.shape[0] == W
        masks = np.zeros((W, 0), dtype=np.uint64) if masks is None else np.asarray(masks, dtype=np.uint64)
        if masks.ndim == 1:
            masks = np.broadcast_to(masks, (W, masks.shape[0]))
        if masks.ndim != 2 or masks.shape[0] != W:
            raise DpeError("[BatchCorrManifold] update_subsets: masks must be [M] or [%d, M]" % W)
        masks = np.ascontiguousarray(masks)
        M = masks.shape[1]
        _check(lib().dpe_bcm_update_subsets(self._h, _ptr(CodeScores), _ptr(CarrScores), C.c_int32(W), C.c_int32(K),
                                            win.ctypes.data_as(C.POINTER(BcmWindow)), chan.ctypes.data_as(C.POINTER(ChanEnd)),
                                            C.c_int32(M), masks.ctypes.data_as(C.POINTER(C.c_uint64)) if M else None, _stream(stream)))
        self._W, self._M, self._K = W, M, K
        self._refresh_keys()
        return 0

    @staticmethod
    def _dict(r):
        return dict(zVal=np.array(r.zVal), RVal=np.eye(8), offset=np.array(r.offset), posIndex=r.posIndex, velIndex=r.velIndex,
                    posScore=r.posScore, velScore=r.velScore, posOutOfWindow=r.posOutOfWindow, velOutOfWindow=r.velOutOfWindow)

    def results(self, stream=None):
        """-> per window a dict: the full set's fix (zVal, offset[8], arg-max, counts), subs = [per subset: the same fields] and
        oobPerSv int64 [2, K] (position, velocity)."""
        full = (BcmSubsetResult * self._W)()
        subs = (BcmSubsetResult * max(self._W * self._M, 1))()
        oob = np.zeros((self._W, 2, self._K), dtype=np.int64)
        _check(lib().dpe_bcm_results_subsets(self._h, full, subs if self._M else None, oob.ctypes.data_as(C.POINTER(C.c_int64)),
                                             _stream(stream)))
        out = []
        for w, f in enumerate(full):
            d = self._dict(f)
            d["subs"] = [self._dict(r) for r in subs[w * self._M:(w + 1) * self._M]] if self._M else []
            d["oobPerSv"] = oob[w]
            out.append(d)
        return out

    def read_keys(self, stream=None):
        """The full set's packed keys of the last Update, uint64 [W, 2] (dpe_bcm_keys)."""
        return d2h(self.Keys, self._W * 2 * 8, np.uint64, stream).reshape(self._W, 2)


class RefineManifold:
    """Coarse-to-fine scan (dpe_bcm_create_refine): levels = [(GridAxes pos, GridAxes vel), ...], level l >= 1 scored around the
    fp32 point level l - 1 peaked at, per window and manifold, one launch per level and nothing read back in between.  Every
    level's rows, keys and counts carry the bits of an axes handle on the fp32 values centre + axis.  The span
    of a level is the caller's choice: it has to cover the distance between the previous level's arg-max and the true peak."""

    def __init__(self, SamplingFrequency, samples_per_window, NumFFTPoints, levels, LPower=1, lag_half_width=8, bin_half_width=48,
                 max_windows=1, max_channels=8, write_scores=True):
        from .grid_axes import GridAxes
        self.fs, self.S, self.C = float(SamplingFrequency), int(samples_per_window), int(NumFFTPoints)
        self.levels = [tuple(lv) for lv in levels]
        for lv in self.levels:
            if len(lv) != 2 or not all(isinstance(a, GridAxes) and a.size == a.global_size for a in lv):
                raise DpeError("[BatchCorrManifold] create_refine: every level is a pair of whole GridAxes (position, velocity)")
        self.LPower, self.L, self.B = int(LPower), int(lag_half_width), int(bin_half_width)
        self.max_windows, self.max_channels = int(max_windows), int(max_channels)
        self.write_scores = bool(write_scores)
        self._h = C.c_void_p(None)
        self.Started = False
        self._W = 0

    def Start(self):
        if self.Started:
            return 0
        from .grid_axes import GridAxesC
        n = len(self.levels)
        cfg = BcmConfig(self.S, self.L, self.B, self.LPower, self.max_windows, self.max_channels, self.C, self.fs, None, None,
                        0, 0, 0, 0, 1 if self.write_scores else 0, 0, 0, 0)
        pa, va = (GridAxesC * max(n, 1))(), (GridAxesC * max(n, 1))()
        for i, (p, v) in enumerate(self.levels):
            pa[i], va[i] = p.c_struct(), v.c_struct()
        _check(lib().dpe_bcm_create_refine(C.byref(cfg), C.c_int32(n), pa, va, C.byref(self._h)))
        self.Started = True
        return 0

    def Update(self, CodeScores, CarrScores, win, chan, stream=None):
        """win: BCM_WINDOW_DTYPE [W]; chan: CHAN_END_DTYPE [W, K]; banks: device pointers from BatchCorrScores."""
        if not self.Started:
            raise DpeError("[BatchCorrManifold] Error: Update() Failed due to module not initialized")
        win, chan, W, K = _win_chan(win, chan)
        assert win.shape[0] == W
        _check(lib().dpe_bcm_update_refine(self._h, _ptr(CodeScores), _ptr(CarrScores), C.c_int32(W), C.c_int32(K),
                                           win.ctypes.data_as(C.POINTER(BcmWindow)), chan.ctypes.data_as(C.POINTER(ChanEnd)),
                                           _stream(stream)))
        self._W = W
        return 0

    def results(self, stream=None):
        """-> per window a dict: zVal, offset[8] (the fp32 points of the last level's maxima) and, per level, posIndex / velIndex
        (-1: not scanned), posScore / velScore, posOutOfWindow / velOutOfWindow as arrays [levels]."""
        res = (BcmRefineResult * self._W)()
        _check(lib().dpe_bcm_results_refine(self._h, res, _stream(stream)))
        n = len(self.levels)
        return [dict(zVal=np.array(r.zVal), RVal=np.eye(8), offset=np.array(r.offset),
                     posIndex=np.array(r.posIndex[:n], dtype=np.int64), velIndex=np.array(r.velIndex[:n], dtype=np.int64),
                     posScore=np.array(r.posScore[:n], dtype=np.float32), velScore=np.array(r.velScore[:n], dtype=np.float32),
                     posOutOfWindow=np.array(r.posOutOfWindow[:n], dtype=np.int64),
                     velOutOfWindow=np.array(r.velOutOfWindow[:n], dtype=np.int64)) for r in res]

    def read_scores(self, level, stream=None):
        """Level `level`'s position and velocity rows of the last Update, float32 [W, G_level] each."""
        ps, vs, pp, vp = C.c_void_p(), C.c_void_p(), C.c_int64(), C.c_int64()
        _check(lib().dpe_bcm_refine_scores(self._h, C.c_int32(level), C.byref(ps), C.byref(vs), C.byref(pp), C.byref(vp)))
        Gp, Gv = (a.global_size for a in self.levels[level])
        p = d2h(ps.value, self._W * pp.value * 4, np.float32, stream).reshape(self._W, pp.value)[:, :Gp]
        v = d2h(vs.value, self._W * vp.value * 4, np.float32, stream).reshape(self._W, vp.value)[:, :Gv]
        return np.ascontiguousarray(p), np.ascontiguousarray(v)

    def read_keys(self, level, stream=None, all_windows=False):
        """Level `level`'s packed keys of the last Update, uint64 [W, 2]; all_windows: the whole set, [max_windows, 2]."""
        keys = C.c_void_p()
        _check(lib().dpe_bcm_refine_keys(self._h, C.c_int32(level), C.byref(keys)))
        n = self.max_windows if all_windows else self._W
        return d2h(keys.value, n * 2 * 8, np.uint64, stream).reshape(n, 2)

    def last_split(self):
        """(position, velocity) blocks per window of the LAST level's launch (dpe_bcm_last_split)."""
        split = (C.c_int32 * 2)()
        _check(lib().dpe_bcm_last_split(self._h, split))
        return (int(split[0]), int(split[1]))

    def profile(self, enable=True):
        ms, cnt = (C.c_float * 2)(), (C.c_int32 * 2)()
        _check(lib().dpe_bcm_profile(self._h, C.c_int32(1 if enable else 0), ms, cnt))
        return {"bcm_scan": (ms[0], cnt[0])}   # the levels' launches of an Update together

    def Stop(self):
        if self.Started:
            _check(lib().dpe_bcm_destroy(self._h))
            self._h = C.c_void_p(None)
            self.Started = False
        return 0

    def __del__(self):
        try:
            self.Stop()
        except Exception:
            pass


def bank_rows(bcs, window=0):
    """Device pointers to window `window` of a BatchCorrScores' code and carrier banks (JointManifold.Update's code / carr)."""
    return (bcs.CodeScores + window * bcs.max_channels * (2 * bcs.L + 1) * 8,
            bcs.CarrScores + window * bcs.max_channels * (2 * bcs.B + 1) * 8)


class Pipe:
    """dpe_pipe: `in_flight` batches of the BatchCorrScores -> BatchCorrManifold path on the device at once (the reference's
    overlap of ingest and compute: sampleblock.cu:327-447, batchcorrscores.h:60-64).  submit() deals a batch to the next lane and
    returns its ticket; results(ticket) waits for that batch only.  lane(ticket) -> (BatchCorrScores, BatchCorrManifold, stream)
    of the batch (banks, scores, keys), valid until `in_flight` later batches have been issued."""

    def __init__(self, SamplingFrequency, samples_per_window, pos_grid, vel_grid, lag_half_width=8, bin_half_width=48,
                 max_windows=1, max_channels=8, in_flight=2, LPower=1, write_scores=True, pos_index_offset=0, vel_index_offset=0,
                 bcm_max_windows=None, weighted_mean=False):
        self.fs, self.S = float(SamplingFrequency), int(samples_per_window)
        self.L, self.B = int(lag_half_width), int(bin_half_width)
        self.max_windows, self.max_channels = int(max_windows), int(max_channels)
        self.bcm_max_windows = int(bcm_max_windows) if bcm_max_windows else self.max_windows   # (stage 1 sharded by window: the scan sees all)
        self.pos_grid, self.vel_grid, po, vo, axes = _grids(pos_grid, vel_grid, pos_index_offset, vel_index_offset)
        self._bcm_kw = dict(LPower=int(LPower), lag_half_width=self.L, bin_half_width=self.B, max_windows=self.bcm_max_windows,
                            max_channels=self.max_channels, write_scores=bool(write_scores),
                            pos_index_offset=0 if axes else po, vel_index_offset=0 if axes else vo, weighted_mean=bool(weighted_mean))
        bcs = BcsConfig(self.S, self.L, self.B, self.max_windows, self.max_channels, 0, self.fs)
        bcm = _bcm_config(self.S, self.L, self.B, int(LPower), self.bcm_max_windows, self.max_channels, carr_fft_len(self.S), self.fs,
                          self.pos_grid, self.vel_grid, po, vo, axes, write_scores, weighted_mean, False)
        self._h = C.c_void_p(None)
        if axes:
            pa, va = self.pos_grid.c_struct(), self.vel_grid.c_struct()
            _check(lib().dpe_pipe_create_axes(C.byref(bcs), C.byref(bcm), C.byref(pa), C.byref(va), C.c_int32(in_flight),
                                              C.byref(self._h)))
        else:
            _check(lib().dpe_pipe_create(C.byref(bcs), C.byref(bcm), C.c_int32(in_flight), C.byref(self._h)))
        self.lanes = self.in_flight = int(in_flight)
        self._faces = {}      # handle pair -> (BatchCorrScores, BatchCorrManifold) faces of a lane
        self._nw = {}         # ticket -> (windows, channels) of the batches the lanes hold

    def set_in_flight(self, n):
        """Deal to the first n lanes only (1: one stream)."""
        _check(lib().dpe_pipe_set_in_flight(self._h, C.c_int32(n)))
        self.in_flight = int(n)

    def lane_at(self, i):
        """(BatchCorrScores, BatchCorrManifold, stream) of lane i, for set-up calls (profile, set_graph)."""
        b, m, st = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(lib().dpe_pipe_lane_at(self._h, C.c_int32(i), C.byref(b), C.byref(m), C.byref(st)))
        return self._lane_faces(b, m, st)

    def _note(self, ticket, W, K):
        self._nw[ticket] = (W, K)
        for t in [t for t in self._nw if t <= ticket - self.lanes]:
            del self._nw[t]

    def _lane_faces(self, bcs_h, bcm_h, st):
        key = (bcs_h.value, bcm_h.value)
        if key not in self._faces:
            b = BatchCorrScores._adopt(bcs_h.value, self.fs, self.S, self.L, self.B, self.max_windows, self.max_channels)
            m = BatchCorrManifold._adopt(bcm_h.value, self.fs, self.S, b.NumFFTPoints, self.pos_grid, self.vel_grid, **self._bcm_kw)
            self._faces[key] = (b, m)
        b, m = self._faces[key]
        return b, m, st.value

    def submit(self, Samples, chan_start, win, chan_end, window_stride=None, stream=None):
        """One batch: Samples device int16 [W, 2 S]; chan_start CHAN_START_DTYPE [W, K]; win BCM_WINDOW_DTYPE [W]; chan_end
        CHAN_END_DTYPE [W, K].  `stream`: the stream that produced Samples (the lane waits for it on the device).  -> ticket"""
        cs = np.ascontiguousarray(chan_start)
        ce = np.ascontiguousarray(chan_end)
        win = np.ascontiguousarray(np.atleast_1d(win))
        if cs.ndim == 1:
            cs, ce = cs[None, :], ce[None, :]
        W, K = cs.shape
        assert ce.shape == (W, K) and win.shape[0] == W
        t = C.c_int64(-1)
        stride = self.S if window_stride is None else int(window_stride)
        _check(lib().dpe_pipe_submit(self._h, _ptr(Samples), C.c_int64(stride), C.c_int32(W), C.c_int32(K),
                                     cs.ctypes.data_as(C.POINTER(ChanStart)), win.ctypes.data_as(C.POINTER(BcmWindow)),
                                     ce.ctypes.data_as(C.POINTER(ChanEnd)), _stream(stream), C.byref(t)))
        self._note(t.value, W, K)
        return t.value

    def acquire(self, stream=None):
        """The next lane for a host that drives the two stages itself (multi-GPU exchanges in between):
        -> (ticket, BatchCorrScores, BatchCorrManifold, lane stream); finish with commit(ticket, n_windows)."""
        t, b, m, st = C.c_int64(-1), C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(lib().dpe_pipe_acquire(self._h, _stream(stream), C.byref(t), C.byref(b), C.byref(m), C.byref(st)))
        return (t.value,) + self._lane_faces(b, m, st)

    def mark_stage1(self, ticket):
        _check(lib().dpe_pipe_mark_stage1(self._h, C.c_int64(ticket)))

    def commit(self, ticket, n_windows, n_chan=None):
        _check(lib().dpe_pipe_commit(self._h, C.c_int64(ticket), C.c_int32(n_windows)))
        self._note(ticket, int(n_windows), n_chan)

    def lane(self, ticket):
        b, m, st = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(lib().dpe_pipe_lane(self._h, C.c_int64(ticket), C.byref(b), C.byref(m), C.byref(st)))
        fb, fm, s = self._lane_faces(b, m, st)
        held = self._nw.get(ticket)
        if held:
            fm._W = held[0]
            fb._W, fb._K = min(held[0], self.max_windows), held[1] or fb._K
        return fb, fm, s

    def results(self, ticket):
        held = self._nw.get(ticket)
        W = held[0] if held else self.bcm_max_windows
        res = (BcmResult * W)()
        _check(lib().dpe_pipe_results(self._h, C.c_int64(ticket), res))
        return [dict(zVal=np.array(r.zVal), RVal=np.eye(8), posIndex=r.posIndex, velIndex=r.velIndex,
                     posScore=r.posScore, velScore=r.velScore, posOutOfWindow=r.posOutOfWindow,
                     velOutOfWindow=r.velOutOfWindow, zValMean=np.array(r.zValMean),
                     weightedSums=np.array([list(r.weightedSums[0]), list(r.weightedSums[1])])) for r in res]

    def samples_consumed(self, ticket, stream=None):
        _check(lib().dpe_pipe_samples_consumed(self._h, C.c_int64(ticket), _stream(stream)))

    def join(self, stream=None):
        _check(lib().dpe_pipe_join(self._h, _stream(stream)))

    def synchronize(self):
        _check(lib().dpe_pipe_synchronize(self._h))

    def close(self):
        if self._h:
            for b, m in self._faces.values():
                b.Stop(); m.Stop()          # (faces only: the pipe owns the handles)
            self._faces = {}
            _check(lib().dpe_pipe_destroy(self._h))
            self._h = C.c_void_p(None)

    Stop = close

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ChmConfig(C.Structure):
    _fields_ = [("nChan", C.c_int32), ("dopplerSign", C.c_int32), ("sampleLength", C.c_double), ("rxTime", C.c_double)]


CHM_INIT_DTYPE = np.dtype([("prn", "<i4"), ("cpElapsed", "<i4"), ("cpReference", "<i4"), ("cpRefTOW", "<i4"),
                           ("codePhase", "<f8"), ("carrierPhase", "<f8"), ("codeFrequency", "<f8"),
                           ("carrierFrequency", "<f8"), ("eph", "<f8", (21,))])


class ChanMgr:
    """Module "cuChanMgr" (cuchanmgr.cu:930-1268), host fp64.  Start()/Update() then outputs()
    returns (chan_start[K], chan_end[K], bcm_window[1]) ready for BatchCorrScores / BatchCorrManifold."""

    def __init__(self, prn, rc, ri, fc, fi, cp, cp_ref, cp_ref_tow, eph, rx_time, T, DopplerSign=1):
        K = len(prn)
        init = np.zeros(K, dtype=CHM_INIT_DTYPE)
        init["prn"], init["cpElapsed"], init["cpReference"], init["cpRefTOW"] = prn, cp, cp_ref, cp_ref_tow
        init["codePhase"], init["carrierPhase"], init["codeFrequency"], init["carrierFrequency"] = rc, ri, fc, fi
        init["eph"] = eph
        self.K = K
        self._h = C.c_void_p(None)
        cfg = ChmConfig(K, int(DopplerSign), float(T), float(rx_time))
        _check(lib().dpe_chm_create(C.byref(cfg), init.ctypes.data_as(C.c_void_p), C.byref(self._h)))

    @classmethod
    def from_handoff(cls, ho, T, K=None, DopplerSign=1):
        """The handoff carries no sign of the front end's spectrum: the caller states it (fi is then the -1 receiver's own)."""
        sl = slice(0, K)
        return cls(ho["prn_list"][sl], ho["rc"][sl], ho["ri"][sl], ho["fc"][sl], ho["fi"][sl], ho["cp"][sl],
                   ho["cp_timestamp"][sl], ho["TOW"][sl], ho["eph"][sl], ho["rxTime"], T, DopplerSign=DopplerSign)

    def _step(self, fn, x_k1k1, x_kk1, time_grid):
        a = np.ascontiguousarray(x_k1k1, dtype=np.float64)
        b = np.ascontiguousarray(x_kk1, dtype=np.float64)
        tg = np.ascontiguousarray(time_grid, dtype=np.float64)
        dp = C.POINTER(C.c_double)
        _check(fn(self._h, a.ctypes.data_as(dp), b.ctypes.data_as(dp), tg.ctypes.data_as(dp), C.c_int32(tg.size)))
        self._dimT = tg.size

    def Start(self, x_k1k1, x_kk1, time_grid=(0.0,)):
        self._step(lib().dpe_chm_start, x_k1k1, x_kk1, time_grid)
        return 0

    def Update(self, x_k1k1, x_kk1, time_grid=(0.0,)):
        self._step(lib().dpe_chm_update, x_k1k1, x_kk1, time_grid)
        return 0

    def outputs(self, with_batch=False):
        start = np.zeros(self.K, dtype=CHAN_START_DTYPE)
        end = np.zeros(self.K, dtype=CHAN_END_DTYPE)
        win = np.zeros(1, dtype=BCM_WINDOW_DTYPE)
        batch = np.zeros((self.K, self._dimT, 8)) if with_batch else None
        _check(lib().dpe_chm_outputs(self._h, start.ctypes.data_as(C.c_void_p), end.ctypes.data_as(C.c_void_p),
                                     win.ctypes.data_as(C.c_void_p),
                                     batch.ctypes.data_as(C.c_void_p) if with_batch else None))
        return (start, end, win, batch) if with_batch else (start, end, win)

    def Stop(self):
        if self._h:
            lib().dpe_chm_destroy(self._h)
            self._h = C.c_void_p(None)
        return 0

    def __del__(self):
        try:            # at interpreter shutdown module globals may already be gone
            self.Stop()
        except Exception:
            pass


class FixRecord(C.Structure):     # dpe_fix_record
    _fields_ = [("seq", C.c_uint64), ("zVal", C.c_double * 8), ("rxTime", C.c_double), ("posIndex", C.c_int64), ("velIndex", C.c_int64),
                ("posOutOfWindow", C.c_int64), ("velOutOfWindow", C.c_int64), ("posScore", C.c_float), ("velScore", C.c_float),
                ("status", C.c_int32), ("reserved", C.c_int32)]


class RvalRecord(C.Structure):    # dpe_rval_record
    _fields_ = [("seq", C.c_uint64), ("R", C.c_double * 64), ("sums", (C.c_double * 15) * 2), ("nAbove", C.c_int64 * 2),
                ("threshold", C.c_float * 2), ("fallback", C.c_int32), ("reserved", C.c_int32)]


class ChanMgrDev:
    """Module "cuChanMgr" as the reference has it: state and port arrays in DEVICE memory, one small kernel per window
    (dpe_chm_dev_*; cuchanmgr.cu:1100-1132,1237-1264).  attach(bcs, bcm) makes it write their parameter blocks and form the
    measurement from the scan's keys: the closed loop is then bcs.UpdatePrepared -> bcm.UpdatePrepared -> step()."""

    def __init__(self, prn, rc, ri, fc, fi, cp, cp_ref, cp_ref_tow, eph, rx_time, T, time_grid=(0.0,), DopplerSign=1):
        K = len(prn)
        init = np.zeros(K, dtype=CHM_INIT_DTYPE)
        init["prn"], init["cpElapsed"], init["cpReference"], init["cpRefTOW"] = prn, cp, cp_ref, cp_ref_tow
        init["codePhase"], init["carrierPhase"], init["codeFrequency"], init["carrierFrequency"] = rc, ri, fc, fi
        init["eph"] = eph
        self.K = K
        tg = np.ascontiguousarray(time_grid, dtype=np.float64)
        self._dimT = tg.size
        self._h = C.c_void_p(None)
        cfg = ChmConfig(K, int(DopplerSign), float(T), float(rx_time))
        _check(lib().dpe_chm_dev_create(C.byref(cfg), init.ctypes.data_as(C.c_void_p), tg.ctypes.data_as(C.c_void_p),
                                        C.c_int32(tg.size), C.byref(self._h)))

    @classmethod
    def from_handoff(cls, ho, T, K=None, time_grid=(0.0,), DopplerSign=1):
        sl = slice(0, K)
        return cls(ho["prn_list"][sl], ho["rc"][sl], ho["ri"][sl], ho["fc"][sl], ho["fi"][sl], ho["cp"][sl],
                   ho["cp_timestamp"][sl], ho["TOW"][sl], ho["eph"][sl], ho["rxTime"], T, time_grid, DopplerSign=DopplerSign)

    def attach(self, bcs=None, bcm=None, ring_depth=64):
        _check(lib().dpe_chm_dev_attach(self._h, bcs._h if bcs is not None else None, bcm._h if bcm is not None else None,
                                        C.c_int32(ring_depth)))

    def set_shard(self, comm, pos_grid_global, vel_grid_global):
        """dpe_chm_dev_set_shard: the attached BatchCorrManifold scans a shard; step() all-reduces the keys over `comm` before the
        measurement kernel, which decodes them against these GLOBAL grids ([G, 4] each; None, or GridAxes, for a BatchCorrManifold
        made from GridAxes: its axes are the global ones)."""
        from .grid_axes import GridAxes
        if pos_grid_global is None or isinstance(pos_grid_global, GridAxes):
            if not (vel_grid_global is None or isinstance(vel_grid_global, GridAxes)):
                raise DpeError("[cuChanMgr] set_shard: both global grids as point lists, or neither")
            _check(lib().dpe_chm_dev_set_shard(self._h, comm._h, None, C.c_int64(0), None, C.c_int64(0)))
            return
        p = np.ascontiguousarray(pos_grid_global, dtype=np.float64)
        v = np.ascontiguousarray(vel_grid_global, dtype=np.float64)
        _check(lib().dpe_chm_dev_set_shard(self._h, comm._h, p.ctypes.data_as(C.c_void_p), C.c_int64(p.shape[0]),
                                           v.ctypes.data_as(C.c_void_p), C.c_int64(v.shape[0])))

    def set_ekf(self, T, x0, P0=None, couple_velocity=True):
        """dpe_chm_dev_set_ekf: cuEKF's filter (EnableEKF = true) inside the measurement kernel instead of the pass-through."""
        cfg = EkfConfig(float(T), 1 if couple_velocity else 0, 0)
        cfg.x0[:] = [float(v) for v in np.asarray(x0, dtype=np.float64)]
        cfg.P0[:] = [float(v) for v in (np.eye(8) if P0 is None else np.asarray(P0, dtype=np.float64)).reshape(64)]
        _check(lib().dpe_chm_dev_set_ekf(self._h, C.byref(cfg)))

    def set_measurement_cov(self, rho, pos_floor, vel_floor):
        """dpe_chm_dev_set_measurement_cov: the device filter takes R from the window's manifold moments (thresholds rho =
        (rho_pos, rho_vel) or one value for both) plus the grids' quantisation floors (pipeline.quantisation_floor of each grid)
        instead of the identity.  After set_ekf, before Start."""
        rp, rv = (rho, rho) if np.isscalar(rho) else rho
        pf = np.ascontiguousarray(pos_floor, dtype=np.float64).reshape(4)
        vf = np.ascontiguousarray(vel_floor, dtype=np.float64).reshape(4)
        dp = C.POINTER(C.c_double)
        _check(lib().dpe_chm_dev_set_measurement_cov(self._h, (C.c_double * 2)(float(rp), float(rv)), pf.ctypes.data_as(dp),
                                                     vf.ctypes.data_as(dp)))

    def rval(self, window, stream=None):
        """dpe_chm_dev_rval: window's R [8, 8] as the device filter took it, with the sums [2, 15], nAbove [2] and threshold [2] it
        was made from and `fallback` (bit m: block m is the identity).  Synchronises `stream`."""
        r = RvalRecord()
        _check(lib().dpe_chm_dev_rval(self._h, C.c_int64(window), C.byref(r), _stream(stream)))
        return dict(R=np.array(r.R[:]).reshape(8, 8), sums=np.array([list(r.sums[0]), list(r.sums[1])]),
                    nAbove=np.array(r.nAbove, dtype=np.int64), threshold=np.array(r.threshold, dtype=np.float32), fallback=int(r.fallback))

    def ekf_state(self, stream=None):
        """dpe_chm_dev_ekf_state: the device filter's members in the form of cuEKF.state()."""
        a = {k: np.zeros(n) for k, n in (("xk1k1", 8), ("xkk1", 8), ("Pk1k1", 64), ("Pkk1", 64), ("Q", 64), ("K", 64))}
        dp = C.POINTER(C.c_double)
        _check(lib().dpe_chm_dev_ekf_state(self._h, *[a[k].ctypes.data_as(dp) for k in ("xk1k1", "xkk1", "Pk1k1", "Pkk1", "Q", "K")],
                                           _stream(stream)))
        return {k: (v if v.size == 8 else v.reshape(8, 8)) for k, v in a.items()}

    def ekf_load(self, xkk1=None, Pkk1=None, stream=None):
        """dpe_chm_dev_ekf_load: x_k|k-1 / P_k|k-1 of the device filter overwritten (None: left as it is).  Between windows only:
        after fix(w) of the last step() has returned."""
        x = None if xkk1 is None else np.ascontiguousarray(xkk1, dtype=np.float64).reshape(8)
        P = None if Pkk1 is None else np.ascontiguousarray(Pkk1, dtype=np.float64).reshape(64)
        dp = C.POINTER(C.c_double)
        _check(lib().dpe_chm_dev_ekf_load(self._h, None if x is None else x.ctypes.data_as(dp), None if P is None else P.ctypes.data_as(dp),
                                          _stream(stream)))

    def ports(self):
        """-> (BcsPortsDev, BcmPortsDev, rxTime_dev, xk1k1_dev, xkk1_dev, zVal_dev): raw device pointers."""
        b, m = BcsPortsDev(), BcmPortsDev()
        rx, x1, xk, z = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(lib().dpe_chm_dev_ports(self._h, C.byref(b), C.byref(m), C.byref(rx), C.byref(x1), C.byref(xk), C.byref(z)))
        return b, m, rx.value, x1.value, xk.value, z.value

    def Start(self, x0, stream=None):
        a = np.ascontiguousarray(x0, dtype=np.float64)
        _check(lib().dpe_chm_dev_start(self._h, a.ctypes.data_as(C.c_void_p), _stream(stream)))
        return 0

    def Update(self, x_k1k1_dev, x_kk1_dev, stream=None):
        _check(lib().dpe_chm_dev_update(self._h, _ptr(x_k1k1_dev), _ptr(x_kk1_dev), _stream(stream)))
        return 0

    def step(self, stream=None):
        _check(lib().dpe_chm_dev_step(self._h, _stream(stream)))
        return 0

    def fix(self, window, timeout_us=-1):
        """-> dict of the window's fix, or None when it has not arrived within timeout_us (>= 0)."""
        r = FixRecord()
        rc = lib().dpe_chm_dev_fix(self._h, C.c_int64(window), C.byref(r), C.c_int32(timeout_us))
        if rc == 1:
            return None
        _check(rc)
        return dict(zVal=np.array(r.zVal[:]), rxTime=r.rxTime, posIndex=r.posIndex, velIndex=r.velIndex, posScore=r.posScore,
                    velScore=r.velScore, posOutOfWindow=r.posOutOfWindow, velOutOfWindow=r.velOutOfWindow, status=r.status)

    def outputs(self, with_batch=False, stream=None):
        start = np.zeros(self.K, dtype=CHAN_START_DTYPE)
        end = np.zeros(self.K, dtype=CHAN_END_DTYPE)
        win = np.zeros(1, dtype=BCM_WINDOW_DTYPE)
        batch = np.zeros((self.K, self._dimT, 8))
        status = C.c_int32(0)
        _check(lib().dpe_chm_dev_read(self._h, start.ctypes.data_as(C.c_void_p), end.ctypes.data_as(C.c_void_p),
                                      win.ctypes.data_as(C.c_void_p), batch.ctypes.data_as(C.c_void_p), C.byref(status), _stream(stream)))
        self.status = status.value
        return (start, end, win, batch) if with_batch else (start, end, win)

    def Stop(self):
        if self._h:
            lib().dpe_chm_dev_destroy(self._h)
            self._h = C.c_void_p(None)
        return 0

    def __del__(self):
        try:
            self.Stop()
        except Exception:
            pass


class AcqConfig(C.Structure):
    _fields_ = [("samplesPerWindow", C.c_int32), ("nCodePeriods", C.c_int32), ("nBins", C.c_int32), ("nPrn", C.c_int32),
                ("mode", C.c_int32), ("prnChunk", C.c_int32), ("samplingFrequency", C.c_double),
                ("binStartHz", C.c_double), ("binStepHz", C.c_double), ("dopplerSign", C.c_double),
                ("prn", C.c_int32 * 37), ("reserved", C.c_int32)]


class AcqResult(C.Structure):
    _fields_ = [("prn", C.c_int32), ("found", C.c_int32), ("maxCodeIdx", C.c_int32), ("maxDoppIdx", C.c_int32),
                ("rc", C.c_double), ("fc", C.c_double), ("fi", C.c_double), ("cppr", C.c_double), ("cppm", C.c_double),
                ("peak", C.c_double)]


class AcqFineResult(C.Structure):
    _fields_ = [("prn", C.c_int32), ("maxCarrIdx", C.c_int32), ("rc", C.c_double), ("ri", C.c_double), ("fc", C.c_double),
                ("fi", C.c_double), ("peakRe", C.c_double), ("peakIm", C.c_double)]


class AcqTrackInit(C.Structure):
    _fields_ = [("prn", C.c_int32), ("found", C.c_int32), ("fromSecondWindow", C.c_int32), ("reserved", C.c_int32),
                ("rc", C.c_double), ("ri", C.c_double), ("fc", C.c_double), ("fi", C.c_double), ("cppr", C.c_double),
                ("cppm", C.c_double), ("cppmWindow", C.c_double * 2)]


class Acquisition:
    """Coarse acquisition over `prns` x Doppler bins x all code delays of one window.
    mode: "coherent" / "noncoherent" = Correlator.coarse_acquisition(coherent=True/False)
    (correlator.py:53-103); "textbook" = 1 ms coherent x N non-coherent (not in the reference)."""
    MODES = {"coherent": 0, "noncoherent": 1, "textbook": 2}

    def __init__(self, SamplingFrequency, samples_per_window, prns, bins_hz, mode="coherent", prn_chunk=0, ds=1.0):
        bins_hz = np.asarray(bins_hz, dtype=np.float64)
        step = float(bins_hz[1] - bins_hz[0]) if bins_hz.size > 1 else 0.0
        assert bins_hz.size == 1 or np.allclose(np.diff(bins_hz), step), "bins must be equally spaced"
        self.S, self.fs = int(samples_per_window), float(SamplingFrequency)
        self.N = int(round(self.S / self.fs / 1e-3))
        self.M = self.S // self.N
        self.prns, self.bins, self.ds = [int(p) for p in prns], bins_hz, float(ds)
        cfg = AcqConfig(self.S, self.N, bins_hz.size, len(self.prns), self.MODES[mode], int(prn_chunk), self.fs,
                        float(bins_hz[0]), step, float(ds), (C.c_int32 * 37)(*self.prns), 0)
        self._h = C.c_void_p(None)
        _check(lib().dpe_acq_create(C.byref(cfg), C.byref(self._h)))
        surf, mp = C.c_void_p(), C.c_void_p()
        _check(lib().dpe_acq_surface(self._h, C.byref(surf), C.byref(mp)))
        self.Surface, self.MaxPerCode = surf.value, mp.value

    def search(self, Samples, stream=None):
        _check(lib().dpe_acq_search(self._h, _ptr(Samples), _stream(stream)))

    def results(self, stream=None):
        res = (AcqResult * len(self.prns))()
        _check(lib().dpe_acq_results(self._h, res, _stream(stream)))
        return [dict(prn=r.prn, found=bool(r.found), max_code_idx=r.maxCodeIdx, max_dopp_idx=r.maxDoppIdx, rc=r.rc, fc=r.fc,
                     fi=r.fi, cppr=r.cppr, cppm=r.cppm, peak=r.peak) for r in res]

    def fine(self, Samples, coarse, stream=None):
        """Correlator.fine_frequency_acquisition (correlator.py:105-133) for every PRN, from `coarse` = results()."""
        res = (AcqResult * len(self.prns))()
        for r, c in zip(res, coarse):
            r.prn, r.rc, r.fc, r.fi = c["prn"], c["rc"], c["fc"], c["fi"]
        out = (AcqFineResult * len(self.prns))()
        _check(lib().dpe_acq_fine(self._h, _ptr(Samples), res, out, _stream(stream)))
        return [dict(prn=r.prn, max_carr_idx=r.maxCarrIdx, rc=r.rc, ri=r.ri, fc=r.fc, fi=r.fi,
                     peak=complex(r.peakRe, r.peakIm)) for r in out]

    def search_signal(self, Samples, stream=None):
        """Correlator.search_signal (correlator.py:38-51): coarse then fine; one dict per PRN."""
        self.search(Samples, stream)
        coarse = self.results(stream)
        fine = self.fine(Samples, coarse, stream)
        return [dict(found=c["found"], rc=f["rc"], ri=f["ri"], fc=f["fc"], fi=f["fi"], cppr=c["cppr"], cppm=c["cppm"],
                     max_carr_idx=f["max_carr_idx"], max_code_idx=c["max_code_idx"], max_dopp_idx=c["max_dopp_idx"])
                for c, f in zip(coarse, fine)]

    def scalar_acquisition(self, Window0, Window1, stream=None):
        """Receiver.scalar_acquisition (receiver.py:452-520) on two consecutive windows (device buffers)."""
        out = (AcqTrackInit * len(self.prns))()
        _check(lib().dpe_acq_scalar_acquisition(self._h, _ptr(Window0), _ptr(Window1), out, _stream(stream)))
        return [dict(prn=r.prn, found=bool(r.found), from_second_window=bool(r.fromSecondWindow), rc=r.rc, ri=r.ri, fc=r.fc,
                     fi=r.fi, cppr=r.cppr, cppm=r.cppm, cppm_window=(r.cppmWindow[0], r.cppmWindow[1])) for r in out]

    def read_surface(self, stream=None):
        n = len(self.prns) * self.bins.size * self.M
        return d2h(self.Surface, n * 4, np.float32, stream).reshape(len(self.prns), self.bins.size, self.M)

    def close(self):
        if self._h:
            lib().dpe_acq_destroy(self._h)
            self._h = C.c_void_p(None)

    def __del__(self):
        try:            # at interpreter shutdown module globals may already be gone
            self.close()
        except Exception:
            pass


class TrkConfig(C.Structure):
    _fields_ = [("samplingFrequency", C.c_double), ("T", C.c_double), ("nChan", C.c_int32), ("order", C.c_int32),
                ("codeBnp", C.c_double), ("carrBnp", C.c_double), ("dopplerSign", C.c_double), ("logCapacityWindows", C.c_int64),
                ("prn", C.c_int32 * 37), ("reserved", C.c_int32)]


class TrkChanState(C.Structure):
    _fields_ = [("prn", C.c_int32), ("lock", C.c_int32), ("frozen", C.c_int32), ("reserved", C.c_int32),
                ("cp", C.c_int64), ("nWindows", C.c_int64), ("nSigns", C.c_int64),
                ("rc", C.c_double), ("ri", C.c_double), ("fc", C.c_double), ("fi", C.c_double), ("fc_bias", C.c_double),
                ("fi_bias", C.c_double), ("paRe", C.c_double), ("paIm", C.c_double)]


class ScalarTracker:
    """Receiver.scalar_track (receiver.py:522-542) for `prns`: every channel's early / prompt / late loop over all windows
    of a call in one kernel launch (dpe_trk_*).  Loop bandwidths default to the twin's (channel.py:57-58)."""
    LOG_NAMES = ("cp", "rc", "ri", "fc", "fi", "iE", "qE", "iP", "qP", "iL", "qL", "dc", "di", "efc", "efi", "dpc", "dpi",
                 "fc_bias", "fi_bias", "lock", "lockval", "snr", "case", "cp_compl")
    CORR_WIDTH = 32

    def __init__(self, SamplingFrequency, prns, T=1e-3, log_capacity_windows=4096, code_bnp=0.0, carr_bnp=0.0, ds=1.0):
        self.fs, self.T = float(SamplingFrequency), float(T)
        self.S = int(round(self.T * self.fs))
        self.prns = [int(p) for p in prns]
        cfg = TrkConfig(self.fs, self.T, len(self.prns), 2, float(code_bnp), float(carr_bnp), float(ds), int(log_capacity_windows),
                        (C.c_int32 * 37)(*self.prns), 0)
        self._h = C.c_void_p(None)
        _check(lib().dpe_trk_create(C.byref(cfg), C.byref(self._h)))
        self.n_windows = 0

    def set_params(self, init, stream=None):
        """init: one dict per channel with prn, rc, ri, fc, fi -- as Acquisition.scalar_acquisition returns them
        (Channel.set_scalar_params, channel.py:82-102)."""
        a = (AcqTrackInit * len(self.prns))()
        for r, c in zip(a, init):
            r.prn, r.found, r.rc, r.ri, r.fc, r.fi = int(c["prn"]), int(bool(c.get("found", True))), c["rc"], c["ri"], c["fc"], c["fi"]
        _check(lib().dpe_trk_set_params(self._h, a, _stream(stream)))
        self.n_windows = 0

    def track(self, Samples, n_windows, stream=None):
        """Samples: device int16 [n_windows, 2*S], consecutive windows.  Asynchronous; successive calls continue the record."""
        _check(lib().dpe_trk_track(self._h, _ptr(Samples), C.c_int32(n_windows), _stream(stream)))
        self.n_windows += int(n_windows)

    def correlate(self, Samples, params, stream=None):
        """Teacher-forced correlator: params [M, K, 4] = rc, ri, fc, fi per window and channel, carried p_a = 0.  Returns
        dict(seg [M, K, 3 segments, 3 taps E P L] complex, epl [M, K, 3] complex, case, cp_compl, idxs1, idxs2, signs [M, K, 2])."""
        p = np.ascontiguousarray(params, dtype=np.float64)
        M, K = p.shape[0], p.shape[1]
        assert p.shape == (M, len(self.prns), 4)
        out = np.empty((M, K, self.CORR_WIDTH), dtype=np.float64)
        dp = C.POINTER(C.c_double)
        _check(lib().dpe_trk_correlate(self._h, _ptr(Samples), C.c_int32(M), p.ctypes.data_as(dp), out.ctypes.data_as(dp), _stream(stream)))
        seg = (out[..., 0:18:2] + 1j * out[..., 1:18:2]).reshape(M, K, 3, 3)
        return dict(seg=seg, epl=out[..., 18:24:2] + 1j * out[..., 19:24:2], case=out[..., 24].astype(np.int64),
                    cp_compl=out[..., 25].astype(np.int64), idxs1=out[..., 26], idxs2=out[..., 27], signs=out[..., 28:30].astype(np.int8))

    def read_log(self, first=0, n=None, stream=None):
        """{name: [n, K]} for the windows [first, first + n) since set_params, names as the twin's logs (LOG_NAMES)."""
        n = self.n_windows - first if n is None else int(n)
        out = np.empty((n, len(self.prns), len(self.LOG_NAMES)), dtype=np.float64)
        _check(lib().dpe_trk_read_log(self._h, C.c_int64(first), C.c_int32(n), out.ctypes.data_as(C.POINTER(C.c_double)), _stream(stream)))
        return {name: out[:, :, j].copy() for j, name in enumerate(self.LOG_NAMES)}

    def load_log(self, rows, stream=None):
        """A saved log back onto the device (Receiver.load_measurement_logs, the log alone): rows {name: [n, K]} with any of
        LOG_NAMES (the others NaN) become windows [0, n).  Tracking continues only after set_params."""
        n = len(next(iter(rows.values())))
        a = np.full((n, len(self.prns), len(self.LOG_NAMES)), np.nan)
        for name, v in rows.items():
            a[:, :, self.LOG_NAMES.index(name)] = v
        _check(lib().dpe_nav_load_log(self._h, C.c_int32(n), a.ctypes.data_as(C.POINTER(C.c_double)), _stream(stream)))
        self.n_windows = n

    def state(self, stream=None):
        st = (TrkChanState * len(self.prns))()
        _check(lib().dpe_trk_state(self._h, st, _stream(stream)))
        return [{f[0]: getattr(r, f[0]) for f in TrkChanState._fields_ if f[0] != "reserved"} for r in st]

    def read_cp_signs(self, chan, first=0, n=None, stream=None):
        """Channel `chan`'s cp_sign stream (int8), entries [first, first + n); n = None: up to the last one written."""
        if n is None:
            n = self.state(stream)[chan]["nSigns"] - first
        out = np.empty(int(n), dtype=np.int8)
        _check(lib().dpe_trk_read_cp_signs(self._h, C.c_int32(chan), C.c_int64(first), C.c_int32(int(n)),
                                           out.ctypes.data_as(C.POINTER(C.c_int8)), _stream(stream)))
        return out

    def dev_status(self, stream=None):
        st = C.c_int32()
        _check(lib().dpe_trk_dev_status(self._h, C.byref(st), _stream(stream)))
        return st.value

    def close(self):
        if self._h:
            lib().dpe_trk_destroy(self._h)
            self._h = C.c_void_p(None)

    def __del__(self):
        try:            # at interpreter shutdown module globals may already be gone
            self.close()
        except Exception:
            pass


class NavDecoded(C.Structure):      # dpe_nav_decoded
    _fields_ = [("eph", C.c_double * 21), ("week", C.c_int32), ("accuracy", C.c_int32), ("health", C.c_int32), ("iode", C.c_int32),
                ("iodc", C.c_int32), ("tow", C.c_int32), ("cp", C.c_int64), ("status", C.c_int32), ("nPreambleHits", C.c_int32),
                ("subframeId", C.c_int32 * 5), ("polarity", C.c_int32 * 5), ("parity", C.c_int32 * 50), ("subframeCp", C.c_int64 * 5)]


class NavFix(C.Structure):          # dpe_nav_fix
    _fields_ = [("X_ECEF", C.c_double * 8), ("rxTime", C.c_double), ("rxTime_a", C.c_double), ("lastUpdate", C.c_double),
                ("iterations", C.c_int32), ("status", C.c_int32)]


NAV_FIX_DTYPE = np.dtype([("X_ECEF", "<f8", (8,)), ("rxTime", "<f8"), ("rxTime_a", "<f8"), ("lastUpdate", "<f8"),
                          ("iterations", "<i4"), ("status", "<i4")])
assert NAV_FIX_DTYPE.itemsize == C.sizeof(NavFix)


class ScalarNavigator:
    """The twin's scalar navigation stage for `prns` (dpe_nav_*): nav-message decode of a channel's cp_sign stream
    (dataparser.py:10-70, ephemeris.py:16-297), the per-epoch fix (naveng.py:10-224) on the host or, for every logged epoch
    of a ScalarTracker, in one device launch, and the handoff dict the DPE loop starts from (receiver.py:804-875)."""
    FULL, ASSISTED = 0, 1
    DEC_FEW_PREAMBLES, DEC_PARITY, DEC_IODE, DEC_POLARITY_FLIP, DEC_CP_SLIP, DEC_NO_HISTORY, DEC_POLARITY_D30, DEC_INCOMPLETE = \
        1, 2, 4, 8, 16, 32, 64, 128
    SOL_RANK_POS, SOL_NOT_CONVERGED, SOL_KEPLER, SOL_RANK_VEL = 1, 2, 4, 8

    def __init__(self, prns, ds=1.0):
        self.prns = [int(p) for p in prns]
        self._h = C.c_void_p(None)
        _check(lib().dpe_nav_create(C.c_int32(len(self.prns)), C.c_double(ds), C.byref(self._h)))
        K = len(self.prns)
        self.eph = np.full((K, 21), np.nan)
        self.tow = np.full(K, -1, dtype=np.int32)
        self.cp_timestamp = np.full(K, -1, dtype=np.int64)

    def decode(self, chan, signs, cp_first=0, mode="full", cp_log=None):
        """signs: channel `chan`'s cp_sign entries (ScalarTracker.read_cp_signs), the first one of code period cp_first.
        Returns the decode as a dict; what it found (ephemerides in full mode, the timestamp in both) stays in the navigator."""
        from .handoff import EPH_FIELDS
        s = np.ascontiguousarray(signs, dtype=np.int8)
        out = NavDecoded()
        cl, ncl = None, 0
        if cp_log is not None:
            cl = np.ascontiguousarray(cp_log, dtype=np.float64)
            ncl = cl.size
        _check(lib().dpe_nav_decode(self._h, C.c_int32(chan), s.ctypes.data_as(C.POINTER(C.c_int8)), C.c_int64(s.size), C.c_int64(int(cp_first)),
                                    C.c_int32(self.ASSISTED if mode in ("assisted", self.ASSISTED) else self.FULL),
                                    cl.ctypes.data_as(C.POINTER(C.c_double)) if cl is not None else None, C.c_int64(ncl), C.byref(out)))
        eph = np.array(out.eph)
        d = {name: float(eph[j]) for j, name in enumerate(EPH_FIELDS)}
        d.update(weeknumber=out.week, accuracy=out.accuracy, health=out.health, IODE=out.iode, IODC=out.iodc,
                 timestamp=dict(TOW=out.tow, cp=out.cp) if out.cp >= 0 else None, status=out.status, n_preamble_hits=out.nPreambleHits,
                 subframe_id=np.array(out.subframeId), polarity=np.array(out.polarity), parity=np.array(out.parity).reshape(5, 10),
                 subframe_cp=np.array(out.subframeCp), eph=eph)
        complete = mode in ("full", self.FULL) and not out.status & (self.DEC_INCOMPLETE | self.DEC_FEW_PREAMBLES | self.DEC_NO_HISTORY)
        if complete:
            self.eph[chan] = eph
        if out.cp >= 0:
            self.tow[chan], self.cp_timestamp[chan] = out.tow, out.cp
        return d

    def set_ephemerides(self, eph=None, tow=None, cp=None):
        """Caller-supplied ephemerides [K, 21] in handoff.EPH_FIELDS order and / or timestamps (tow [K], cp [K])."""
        K = len(self.prns)
        e = t = c = None
        if eph is not None:
            e = np.ascontiguousarray(eph, dtype=np.float64)
            assert e.shape == (K, 21)
            self.eph[:] = e
        if tow is not None:
            t, c = np.ascontiguousarray(tow, dtype=np.int32), np.ascontiguousarray(cp, dtype=np.int64)
            assert t.shape == (K,) and c.shape == (K,)
            self.tow[:], self.cp_timestamp[:] = t, c
        _check(lib().dpe_nav_set_ephemerides(self._h, e.ctypes.data_as(C.POINTER(C.c_double)) if e is not None else None,
                                             t.ctypes.data_as(C.POINTER(C.c_int32)) if t is not None else None,
                                             c.ctypes.data_as(C.POINTER(C.c_int64)) if c is not None else None))

    @staticmethod
    def _mask(chans):
        m = 0
        for k in chans or ():
            m |= 1 << int(k)
        return C.c_uint64(m)

    @staticmethod
    def _fix(r):
        return dict(X_ECEF=np.array(r["X_ECEF"], dtype=np.float64), rxTime=float(r["rxTime"]), rxTime_a=float(r["rxTime_a"]),
                    last_update=float(r["lastUpdate"]), iterations=int(r["iterations"]), status=int(r["status"]))

    def solve(self, cp, rc, fi, chans=None, rx_time0=None):
        """One epoch on the host: cp, rc, fi [K] (a row of the tracker's log); chans: the channels to use (None: all)."""
        dp = C.POINTER(C.c_double)
        a = [np.ascontiguousarray(v, dtype=np.float64) for v in (cp, rc, fi)]
        assert all(v.shape == (len(self.prns),) for v in a)
        out = np.zeros(1, dtype=NAV_FIX_DTYPE)
        _check(lib().dpe_nav_solve(self._h, a[0].ctypes.data_as(dp), a[1].ctypes.data_as(dp), a[2].ctypes.data_as(dp), self._mask(chans),
                                   C.c_double(np.nan if rx_time0 is None else rx_time0), out.ctypes.data_as(C.c_void_p)))
        return self._fix(out[0])

    def solve_log(self, tracker, first=0, n_epochs=None, stride=1, chans=None, rx_time0=None, rx_time_step=0.0, stream=None):
        """Every epoch first + i * stride, i < n_epochs, of `tracker`'s device-resident log in one launch.  Returns the
        dpe_nav_fix records as a structured array (NAV_FIX_DTYPE)."""
        if n_epochs is None:
            n_epochs = (tracker.n_windows - first + stride - 1) // stride
        out = np.zeros(int(n_epochs), dtype=NAV_FIX_DTYPE)
        _check(lib().dpe_nav_solve_log(self._h, tracker._h, C.c_int64(first), C.c_int32(int(n_epochs)), C.c_int32(stride), self._mask(chans),
                                       C.c_double(np.nan if rx_time0 is None else rx_time0), C.c_double(rx_time_step),
                                       out.ctypes.data_as(C.c_void_p), _stream(stream)))
        return out

    def status(self):
        st = C.c_int32()
        _check(lib().dpe_nav_status(self._h, C.byref(st)))
        return st.value

    def handoff(self, fix, rc, ri, fc, fi, cp, bytes_read=0):
        """The handoff dict (handoff.read_handoff's form) at one epoch: `fix` from solve / one record of solve_log, the
        channels' rc, ri, fc, fi, cp there (a row of the tracker's log, or its state), the file offset of that window."""
        f = self._fix(fix) if not isinstance(fix, dict) else fix
        assert np.all(self.cp_timestamp >= 0) and not np.isnan(self.eph).any(), "a channel has no timestamp or no ephemerides"
        return dict(rxTime=f["rxTime"], rxTime_a=f["rxTime_a"], X_ECEF=np.array(f["X_ECEF"], dtype=np.float64), bytes_read=int(bytes_read),
                    prn_list=np.array(self.prns, dtype=np.int32), rc=np.array(rc, dtype=np.float64), ri=np.array(ri, dtype=np.float64),
                    fc=np.array(fc, dtype=np.float64), fi=np.array(fi, dtype=np.float64), cp=np.array(cp).astype(np.int32),
                    cp_timestamp=self.cp_timestamp.astype(np.int32), TOW=self.tow.astype(np.int32), eph=self.eph.copy())

    def close(self):
        if self._h:
            lib().dpe_nav_destroy(self._h)
            self._h = C.c_void_p(None)

    def __del__(self):
        try:            # at interpreter shutdown module globals may already be gone
            self.close()
        except Exception:
            pass


class VtConfig(C.Structure):        # dpe_vt_config
    _fields_ = [("samplingFrequency", C.c_double), ("T", C.c_double), ("N", C.c_int32), ("nChan", C.c_int32), ("prn", C.c_int32 * 16),
                ("dopplerSign", C.c_double), ("numPrev", C.c_int32), ("reserved", C.c_int32), ("initVarRange", C.c_double),
                ("initVarRate", C.c_double), ("minVarRange", C.c_double), ("minVarRate", C.c_double), ("qDiag", C.c_double * 8),
                ("initSigmaDiag", C.c_double * 8), ("lockThreshold", C.c_double), ("logCapacityEpochs", C.c_int64)]


class VtChan(C.Structure):          # dpe_vt_chan
    _fields_ = [("rc", C.c_double), ("ri", C.c_double), ("fc", C.c_double), ("fi", C.c_double), ("cp", C.c_double), ("sat", C.c_double * 8),
                ("histRange", C.c_double * 32), ("histRate", C.c_double * 32), ("histN", C.c_int32), ("histPos", C.c_int32)]


class VtStateRec(C.Structure):      # dpe_vt_state_rec
    _fields_ = [("X", C.c_double * 8), ("Sigma", C.c_double * 64), ("rxTime0", C.c_double), ("rxBase", C.c_double), ("epochs", C.c_int64),
                ("status", C.c_int32), ("satValid", C.c_int32), ("chan", VtChan * 16)]


class VectorTracker:
    """Vector tracking for `prns` (dpe_vt_*): no channel has a loop filter of its own; every epoch of N windows the
    early / prompt / late correlations of all channels become range and range-rate residuals of one 8-state filter, and every
    channel's code and carrier NCO is back-computed from the filtered state.  Two kernel launches per epoch, no host synchronisation
    between epochs."""
    BAD_WINDOW, NO_UPDATE, PIVOT = 1, 2, 4
    LOG_HEAD, LOG_CHAN, MAX_CHAN = 20, 12, 16
    CHAN_NAMES = ("rc", "ri", "fc", "fi", "cp", "eR", "eV", "wR", "wV", "lock", "dpc", "dfi")

    @staticmethod
    def config(SamplingFrequency, prns, T=1e-3, N=20, ds=1.0, num_prev=20, init_var=(0.0, 0.0), min_var=(0.0, 0.0), q_diag=None,
               init_sigma_diag=None, lock_threshold=0.0, log_capacity_epochs=4096):
        prns = [int(p) for p in prns]
        return VtConfig(float(SamplingFrequency), float(T), int(N), len(prns), (C.c_int32 * 16)(*prns[:16]), float(ds), int(num_prev), 0,
                        float(init_var[0]), float(init_var[1]), float(min_var[0]), float(min_var[1]),
                        (C.c_double * 8)(*([0.0] * 8 if q_diag is None else q_diag)),
                        (C.c_double * 8)(*([0.0] * 8 if init_sigma_diag is None else init_sigma_diag)), float(lock_threshold), int(log_capacity_epochs))

    def __init__(self, SamplingFrequency, prns, **kw):
        self.prns = [int(p) for p in prns]
        self.cfg = self.config(SamplingFrequency, prns, **kw)
        self.fs, self.T, self.N = self.cfg.samplingFrequency, self.cfg.T, self.cfg.N or 20
        self.S = int(round(self.T * self.fs))
        self._h = C.c_void_p(None)
        _check(lib().dpe_vt_create(C.byref(self.cfg), C.byref(self._h)))
        self.n_epochs = 0
        self.eph = self.tow = self.cp_timestamp = None

    def set_ephemerides(self, eph, tow, cp):
        """eph [K, 21] in handoff.EPH_FIELDS order with their timestamps (TOW [K] at code-period count cp [K])."""
        K = len(self.prns)
        e, t, c = np.ascontiguousarray(eph, dtype=np.float64), np.ascontiguousarray(tow, dtype=np.int32), np.ascontiguousarray(cp, dtype=np.int64)
        assert e.shape == (K, 21) and t.shape == (K,) and c.shape == (K,)
        self.eph, self.tow, self.cp_timestamp = e.copy(), t.copy(), c.copy()
        _check(lib().dpe_vt_set_ephemerides(self._h, e.ctypes.data_as(C.POINTER(C.c_double)), t.ctypes.data_as(C.POINTER(C.c_int32)),
                                            c.ctypes.data_as(C.POINTER(C.c_int64))))

    def init(self, X, Sigma, rx_time0, chan, stream=None):
        """X [8], Sigma [8, 8], the receive time of the first sample and chan [K, 5] = rc ri fc fi cp there."""
        dp = C.POINTER(C.c_double)
        x, s, c = (np.ascontiguousarray(v, dtype=np.float64) for v in (X, Sigma, chan))
        assert x.shape == (8,) and s.size == 64 and c.shape == (len(self.prns), 5)
        _check(lib().dpe_vt_init(self._h, x.ctypes.data_as(dp), s.ctypes.data_as(dp), C.c_double(rx_time0), c.ctypes.data_as(dp), _stream(stream)))
        self.n_epochs = 0

    def init_from_tracker(self, tracker, fix, stream=None):
        """The vt_init hand-over: channel states from `tracker`'s device state (after its last window), X and rxTime0 from `fix`,
        the solution of the tracker's last tracked window (ScalarNavigator.solve_log(tracker, first=n_windows - 1, n_epochs=1)[0]),
        advanced by that one window."""
        f = NavFix((C.c_double * 8)(*np.asarray(fix["X_ECEF"], dtype=np.float64)), float(fix["rxTime"]), float(fix["rxTime_a"]), 0.0, 0, 0)
        _check(lib().dpe_vt_init_from_trk(self._h, tracker._h, C.byref(f), _stream(stream)))
        self.n_epochs = 0

    def track(self, Samples, n_epochs, stream=None):
        """Samples: device int16, n_epochs * N consecutive windows of 2 * S values.  Asynchronous; successive calls continue."""
        _check(lib().dpe_vt_track(self._h, _ptr(Samples), C.c_int32(n_epochs), _stream(stream)))
        self.n_epochs += int(n_epochs)

    def read_log(self, first=0, n=None, stream=None):
        """{X [n, 8], diag [n, 8], rxTime0, mask, status, n_incl [n], and per channel CHAN_NAMES [n, K]} for epochs [first, first + n)."""
        return self.unpack_log(self.read_log_rows(first, n, stream), len(self.prns))

    def read_log_rows(self, first=0, n=None, stream=None):
        """The raw log rows [n, LOG_HEAD + MAX_CHAN * LOG_CHAN] of epochs [first, first + n), channels K .. MAX_CHAN - 1 included."""
        n = self.n_epochs - first if n is None else int(n)
        out = np.empty((n, self.LOG_HEAD + self.MAX_CHAN * self.LOG_CHAN), dtype=np.float64)
        _check(lib().dpe_vt_read_log(self._h, C.c_int64(first), C.c_int32(n), out.ctypes.data_as(C.POINTER(C.c_double)), _stream(stream)))
        return out

    @classmethod
    def unpack_log(cls, out, K):
        d = dict(X=out[:, 0:8].copy(), diag=out[:, 8:16].copy(), rxTime0=out[:, 16].copy(), mask=out[:, 17].astype(np.int64),
                 status=out[:, 18].astype(np.int64), n_incl=out[:, 19].astype(np.int64))
        ch = out[:, cls.LOG_HEAD:].reshape(out.shape[0], cls.MAX_CHAN, cls.LOG_CHAN)
        for j, name in enumerate(cls.CHAN_NAMES):
            d[name] = ch[:, :K, j].copy()
        return d

    def read_corr(self, stream=None):
        """The last epoch's correlations [N, K, 8]: iE qE iP qP iL qL, boundary case, completed code periods."""
        out = np.empty((self.N, len(self.prns), 8), dtype=np.float64)
        _check(lib().dpe_vt_read_corr(self._h, out.ctypes.data_as(C.POINTER(C.c_double)), _stream(stream)))
        return out

    def state_rec(self, stream=None):
        """The whole device state as the raw VtStateRec: beside what state() gives, every channel's satellite cache and residual
        history, satValid and rxBase -- what filter_step_host takes as its `st`."""
        st = VtStateRec()
        _check(lib().dpe_vt_state(self._h, C.byref(st), _stream(stream)))
        return st

    def state(self, stream=None):
        return self.unpack_state(self.state_rec(stream), len(self.prns))

    @staticmethod
    def unpack_state(st, K):
        d = dict(X=np.array(st.X), Sigma=np.array(st.Sigma).reshape(8, 8), rxTime0=st.rxTime0, epochs=st.epochs, status=st.status)
        for n in ("rc", "ri", "fc", "fi", "cp"):
            d[n] = np.array([getattr(st.chan[k], n) for k in range(K)])
        return d

    def dev_status(self, stream=None):
        st = C.c_int32()
        _check(lib().dpe_vt_dev_status(self._h, C.byref(st), _stream(stream)))
        return st.value

    def handoff(self, bytes_read=0, stream=None):
        """The state after the last epoch as a handoff dict (handoff.read_handoff's form): what ChanMgr.from_handoff and
        pipeline.run_closed_loop start from, as ScalarNavigator.handoff's."""
        s = self.state(stream)
        return dict(rxTime=s["rxTime0"], rxTime_a=s["rxTime0"] - s["X"][3] / 299792458.0, X_ECEF=s["X"].copy(), bytes_read=int(bytes_read),
                    prn_list=np.array(self.prns, dtype=np.int32), rc=s["rc"], ri=s["ri"], fc=s["fc"], fi=s["fi"], cp=s["cp"].astype(np.int32),
                    cp_timestamp=self.cp_timestamp.astype(np.int32), TOW=self.tow.astype(np.int32), eph=self.eph.copy())

    @classmethod
    def filter_step_host(cls, cfg, eph, tow, cp, st, sums):
        """dpe_vt_filter_step_host: one epoch's discriminators, gate, W, update, predict and steering on the host.  cfg: config(...);
        st: a VtStateRec (updated in place); sums [N, K, 8].  Returns the epoch's log record, unpacked."""
        e, t, c = np.ascontiguousarray(eph, dtype=np.float64), np.ascontiguousarray(tow, dtype=np.int32), np.ascontiguousarray(cp, dtype=np.int64)
        s = np.ascontiguousarray(sums, dtype=np.float64)
        assert s.shape == ((cfg.N or 20), cfg.nChan, 8)
        rec = np.zeros((1, cls.LOG_HEAD + cls.MAX_CHAN * cls.LOG_CHAN))
        dp = C.POINTER(C.c_double)
        _check(lib().dpe_vt_filter_step_host(C.byref(cfg), e.ctypes.data_as(dp), t.ctypes.data_as(C.POINTER(C.c_int32)), c.ctypes.data_as(C.POINTER(C.c_int64)),
                                             C.byref(st), s.ctypes.data_as(dp), rec.ctypes.data_as(dp)))
        return {k: v[0] for k, v in cls.unpack_log(rec, cfg.nChan).items()}

    def close(self):
        if self._h:
            lib().dpe_vt_destroy(self._h)
            self._h = C.c_void_p(None)

    def __del__(self):
        try:            # at interpreter shutdown module globals may already be gone
            self.close()
        except Exception:
            pass


class EkfConfig(C.Structure):
    _fields_ = [("sampleLength", C.c_double), ("coupleVelocity", C.c_int32), ("reserved", C.c_int32),
                ("x0", C.c_double * 8), ("P0", C.c_double * 64)]


class cuEKF:
    """Module "cuEKF" (cudarecv/modules/src/cuekf.cu): EnableEKF=False passes zVal through (EKF_PassMeas :147-159,
    the shipped flow); EnableEKF=True runs StepUpdate then StepPredict per Update (:560-599), host fp64."""

    def __init__(self, InitX, InitP=None, SampleLength=0.02, EnableEKF=False, couple_velocity=True):
        self.EnableEKF = bool(EnableEKF)
        self.xCurrk1k1 = np.array(InitX, dtype=np.float64).copy()
        self.xCurrkk1 = self.xCurrk1k1.copy()
        self._h = C.c_void_p(None)
        if self.EnableEKF:
            cfg = EkfConfig()
            cfg.sampleLength = float(SampleLength)
            cfg.coupleVelocity = 1 if couple_velocity else 0
            P0 = np.eye(8) if InitP is None else np.asarray(InitP, dtype=np.float64).reshape(8, 8)
            for i in range(8):
                cfg.x0[i] = float(self.xCurrk1k1[i])
            for i in range(64):
                cfg.P0[i] = float(P0.ravel()[i])
            _check(lib().dpe_ekf_create(C.byref(cfg), C.byref(self._h)))

    def Update(self, zVal, RVal=None):
        z = np.ascontiguousarray(zVal, dtype=np.float64)
        if not self.EnableEKF:
            self.xCurrk1k1 = z.copy(); self.xCurrkk1 = z.copy()
            return 0
        R = np.ascontiguousarray(np.eye(8) if RVal is None else RVal, dtype=np.float64)
        dp = C.POINTER(C.c_double)
        _check(lib().dpe_ekf_step_update(self._h, z.ctypes.data_as(dp), R.ctypes.data_as(dp)))
        _check(lib().dpe_ekf_step_predict(self._h))
        st = self.state()
        self.xCurrk1k1, self.xCurrkk1 = st["xk1k1"], st["xkk1"]
        return 0

    def step_update(self, zVal, RVal):
        z = np.ascontiguousarray(zVal, dtype=np.float64); R = np.ascontiguousarray(RVal, dtype=np.float64)
        dp = C.POINTER(C.c_double)
        _check(lib().dpe_ekf_step_update(self._h, z.ctypes.data_as(dp), R.ctypes.data_as(dp)))

    def step_predict(self):
        _check(lib().dpe_ekf_step_predict(self._h))

    def state(self):
        a = {k: np.zeros(n) for k, n in (("xk1k1", 8), ("xkk1", 8), ("Pk1k1", 64), ("Pkk1", 64), ("Q", 64), ("K", 64))}
        dp = C.POINTER(C.c_double)
        _check(lib().dpe_ekf_state(self._h, *[a[k].ctypes.data_as(dp) for k in ("xk1k1", "xkk1", "Pk1k1", "Pkk1", "Q", "K")]))
        return {k: (v if v.size == 8 else v.reshape(8, 8)) for k, v in a.items()}

    def load(self, xkk1=None, Pkk1=None):
        """dpe_ekf_load: x_k|k-1 / P_k|k-1 overwritten between two steps (None: left as it is)."""
        x = None if xkk1 is None else np.ascontiguousarray(xkk1, dtype=np.float64).reshape(8)
        P = None if Pkk1 is None else np.ascontiguousarray(Pkk1, dtype=np.float64).reshape(64)
        dp = C.POINTER(C.c_double)
        _check(lib().dpe_ekf_load(self._h, None if x is None else x.ctypes.data_as(dp), None if P is None else P.ctypes.data_as(dp)))
        if x is not None:
            self.xCurrkk1 = x.copy()

    def Stop(self):
        if self._h:
            lib().dpe_ekf_destroy(self._h)
            self._h = C.c_void_p(None)

    def __del__(self):
        try:            # at interpreter shutdown module globals may already be gone
            self.Stop()
        except Exception:
            pass


class SynConfig(C.Structure):       # dpe_syn_config
    _fields_ = [("samplingFrequency", C.c_double), ("maxSegments", C.c_int32), ("maxChannels", C.c_int32), ("maxNavBits", C.c_int32),
                ("reserved", C.c_int32)]


class SynSignal(C.Structure):       # dpe_syn_signal
    _fields_ = [("sigma", C.c_double), ("dcI", C.c_double), ("dcQ", C.c_double), ("seed", C.c_uint64)]


class Synthesizer:
    """Seeded int16 I/Q made on the device from channel parameters (dpe_syn_*, csrc/dpe_syn.hip): synth.gen_iq's
    model for windows and synth.gen_iq_record's for a continuous record, with counter-based noise -- a sample depends on
    (seed, stream, sample index) alone.  Both calls are asynchronous and return torch int16 tensors on the device that
    BatchCorrScores.Update, Pipe.submit, Acquisition.search, ScalarTracker.track and VectorTracker.track take as they are."""

    def __init__(self, SamplingFrequency, max_segments=1, max_channels=8, max_nav_bits=0):
        self.fs = float(SamplingFrequency)
        self.max_segments, self.max_channels, self.max_nav_bits = int(max_segments), int(max_channels), int(max_nav_bits)
        cfg = SynConfig(self.fs, self.max_segments, self.max_channels, self.max_nav_bits, 0)
        self._h = C.c_void_p(None)
        _check(lib().dpe_syn_create(C.byref(cfg), C.byref(self._h)))

    @staticmethod
    def _chan(chan):
        """CHAN_START_DTYPE array, or a dict with synth.random_channels' keys (prn, rc, ri, fc, fi and optionally cp, cp_ref)."""
        if isinstance(chan, dict):
            z = np.zeros(np.shape(chan["rc"]), dtype=np.int32)
            chan = chan_start_array(chan["prn"], chan["rc"], chan["ri"], chan["fc"], chan["fi"], chan.get("cp", z), chan.get("cp_ref", z))
        return np.ascontiguousarray(chan, dtype=CHAN_START_DTYPE)

    @staticmethod
    def _signal(K, amp, sigma, dc, seed):
        amp = np.ascontiguousarray(np.broadcast_to(np.asarray(amp, dtype=np.float64), (K,)))
        return amp, SynSignal(float(sigma), float(dc[0]), float(dc[1]), int(seed) & 0xFFFFFFFFFFFFFFFF)

    def set_nav_bits(self, nav_bits, stream=None):
        """nav_bits[k]: +-1 per bit of channel slot k (gen_iq_record's convention)."""
        for k, b in enumerate(nav_bits):
            b = np.ascontiguousarray(b, dtype=np.int8)
            _check(lib().dpe_syn_set_nav_bits(self._h, C.c_int32(k), b.ctypes.data_as(C.POINTER(C.c_int8)), C.c_int32(b.size), _stream(stream)))

    def windows(self, S, chan, amp=48.0, sigma=300.0, dc=(3.0, -2.0), flip=None, seed=0, first_stream=0, stride=None, out=None,
                stream=None):
        """W windows of S samples from chan[W][K] (or [K]: one window): the device form of the loop body of
        workload.build_windows.  stride: int16 values between windows (even, >= 2 S; default 2 S).  Window w draws its noise
        from stream first_stream + w.  Returns int16 [W, stride] (`out`, when given, is written in place: what lies between
        windows is not touched)."""
        import torch
        chan = self._chan(chan)
        if chan.ndim == 1:
            chan = chan[None, :]
        W, K = chan.shape
        stride = 2 * int(S) if stride is None else int(stride)
        amp, sig = self._signal(K, amp, sigma, dc, seed)
        fl = None
        if flip is not None:
            fl = np.ascontiguousarray(np.broadcast_to(np.asarray(flip, dtype=bool), (W, K)), dtype=np.uint8)
        if out is None:
            out = torch.empty((W, max(stride, 2 * int(S))), dtype=torch.int16, device="cuda")
        _check(lib().dpe_syn_windows(self._h, _ptr(out), C.c_int64(stride), C.c_int32(W), C.c_int32(int(S)), C.c_int32(K),
                                     chan.ctypes.data_as(C.POINTER(ChanStart)), amp.ctypes.data_as(C.POINTER(C.c_double)), C.byref(sig),
                                     None if fl is None else fl.ctypes.data_as(C.POINTER(C.c_uint8)), C.c_uint64(int(first_stream)),
                                     _stream(stream)))
        return out

    def record(self, first_sample, n_samples, chan, amp=48.0, sigma=300.0, dc=(0.0, 0.0), seed=0, stream_id=0, out=None, stream=None):
        """Samples [first_sample, first_sample + n_samples) of the continuous record of chan[K] (referred to sample 0), nav bits
        as set_nav_bits left them.  Any split of a range into calls gives the bytes of one call.  Returns int16 [2 n_samples]."""
        import torch
        chan = self._chan(chan)
        K = chan.shape[0]
        amp, sig = self._signal(K, amp, sigma, dc, seed)
        if out is None:
            out = torch.empty(2 * int(n_samples), dtype=torch.int16, device="cuda")
        _check(lib().dpe_syn_record(self._h, _ptr(out), C.c_int64(int(first_sample)), C.c_int64(int(n_samples)), C.c_int32(K),
                                    chan.ctypes.data_as(C.POINTER(ChanStart)), amp.ctypes.data_as(C.POINTER(C.c_double)), C.byref(sig),
                                    C.c_uint64(int(stream_id)), _stream(stream)))
        return out

    def close(self):
        if self._h:
            lib().dpe_syn_destroy(self._h)
            self._h = C.c_void_p(None)

    def __del__(self):
        try:            # at interpreter shutdown module globals may already be gone
            self.close()
        except Exception:
            pass


class CdConfig(C.Structure):        # dpe_cd_config
    _fields_ = [("M", C.c_int32), ("nBins", C.c_int32), ("maxSv", C.c_int32), ("driftHalfWidth", C.c_int32), ("nPoints", C.c_int32),
                ("reserved", C.c_int32), ("enuGrid", C.POINTER(C.c_double)), ("samplingFrequency", C.c_double),
                ("binStartHz", C.c_double), ("binStepHz", C.c_double), ("dopplerSign", C.c_double)]


class CdSv(C.Structure):            # dpe_cd_sv
    _fields_ = [("prn", C.c_int32), ("row", C.c_int32), ("sat", C.c_double * 3), ("delay0", C.c_double), ("bin0", C.c_double),
                ("range0", C.c_double), ("dopplerHz", C.c_double)]


class CdResult(C.Structure):        # dpe_cd_result
    _fields_ = [("point", C.c_int32), ("m", C.c_int32), ("j", C.c_int32), ("binsOutOfRange", C.c_int32), ("nSv", C.c_int32),
                ("reserved", C.c_int32), ("score", C.c_double), ("fixEcef", C.c_double * 3), ("clockBiasM", C.c_double),
                ("clockDriftMps", C.c_double)]


class CdSvResult(C.Structure):      # dpe_cd_sv_result
    _fields_ = [("prn", C.c_int32), ("found", C.c_int32), ("maxCodeIdx", C.c_int32), ("maxDoppIdx", C.c_int32),
                ("rc", C.c_double), ("fc", C.c_double), ("fi", C.c_double), ("peak", C.c_double)]


def cd_predict(SamplingFrequency, M, bins_hz, eph, prns, rows, p0, rx_time, ds=1.0):
    """Host, fp64, no device (dpe_cd_predict): per SV the delay and the fractional Doppler bin at p0 (ECEF) for the coarse GPS time
    rx_time of the window's first sample, from ephemerides [K, 21] (handoff.EPH_FIELDS' order).  One dict per SV (prn, row, sat,
    delay0, bin0, range0, doppler_hz), as CollectiveDetector.update takes them."""
    bins_hz = np.asarray(bins_hz, dtype=np.float64)
    step = float(bins_hz[1] - bins_hz[0]) if bins_hz.size > 1 else 0.0
    cfg = CdConfig(int(M), bins_hz.size, 1, 0, 1, 0, None, float(SamplingFrequency), float(bins_hz[0]), step, float(ds))
    eph = np.ascontiguousarray(eph, dtype=np.float64).reshape(-1, 21)
    prns, rows = np.ascontiguousarray(prns, dtype=np.int32), np.ascontiguousarray(rows, dtype=np.int32)
    p0 = np.ascontiguousarray(np.asarray(p0, dtype=np.float64)[:3])
    K = prns.size
    assert eph.shape[0] == K == rows.size
    out = (CdSv * max(K, 1))()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    _check(lib().dpe_cd_predict(C.byref(cfg), C.c_int32(K), eph.ctypes.data_as(dp), prns.ctypes.data_as(ip), rows.ctypes.data_as(ip),
                                p0.ctypes.data_as(dp), C.c_double(float(rx_time)), out))
    return [dict(prn=r.prn, row=r.row, sat=np.array(r.sat[:]), delay0=r.delay0, bin0=r.bin0, range0=r.range0,
                 doppler_hz=r.dopplerHz) for r in out[:K]]


class CollectiveDetector:
    """Collective detection (dpe_cd_*, csrc/dpe_cd.hip): the delay x Doppler surfaces of all SVs, as an
    Acquisition leaves them on the device, summed over position offset x clock bias x clock drift, one arg-max over the sum.
    enu_grid: [P, 3] position offsets in ENU metres about the p0 of an update; bins_hz: the surfaces' Doppler raster."""
    MAX_SV, MAX_DRIFT = 16, 32

    def __init__(self, SamplingFrequency, M, bins_hz, enu_grid, drift_half_width=0, max_sv=16, ds=1.0):
        bins_hz = np.asarray(bins_hz, dtype=np.float64)
        step = float(bins_hz[1] - bins_hz[0]) if bins_hz.size > 1 else 0.0
        assert bins_hz.size == 1 or np.allclose(np.diff(bins_hz), step), "bins must be equally spaced"
        self.fs, self.M, self.bins, self.J = float(SamplingFrequency), int(M), bins_hz, int(drift_half_width)
        self.grid = np.ascontiguousarray(enu_grid, dtype=np.float64).reshape(-1, 3)
        self.P, self.max_sv, self.n_sv, self.ds = self.grid.shape[0], int(max_sv), 0, float(ds)
        cfg = CdConfig(self.M, bins_hz.size, self.max_sv, self.J, self.P, 0, self.grid.ctypes.data_as(C.POINTER(C.c_double)), self.fs,
                       float(bins_hz[0]), step, float(ds))
        self._h = C.c_void_p(None)
        _check(lib().dpe_cd_create(C.byref(cfg), C.byref(self._h)))
        score, jm = C.c_void_p(), C.c_void_p()
        _check(lib().dpe_cd_map(self._h, C.byref(score), C.byref(jm)))
        self.MapScore, self.MapJM = score.value, jm.value

    @staticmethod
    def sv_array(sv):
        """List of dicts (prn, row, sat, delay0, bin0) -> the C array; a C array passes through."""
        if not isinstance(sv, (list, tuple)):
            return sv
        a = (CdSv * len(sv))()
        for r, c in zip(a, sv):
            r.prn, r.row, r.delay0, r.bin0 = int(c["prn"]), int(c["row"]), float(c["delay0"]), float(c["bin0"])
            r.sat[0], r.sat[1], r.sat[2] = (float(v) for v in c["sat"])
            r.range0, r.dopplerHz = float(c.get("range0", 0.0)), float(c.get("doppler_hz", 0.0))
        return a

    def predict(self, eph, prns, rows, p0, rx_time):
        """cd_predict with the handle's sampling frequency, M, bin raster and Doppler sign."""
        return cd_predict(self.fs, self.M, self.bins, eph, prns, rows, p0, rx_time, ds=self.ds)

    def update(self, acq_or_surface, sv, p0, enu2ecef, n_rows=None, stream=None):
        """One scan, asynchronous.  acq_or_surface: an Acquisition after search (its surface and row count are taken), or a
        device float32 array [n_rows, nBins, M] (torch tensor, or a raw pointer with n_rows given)."""
        if isinstance(acq_or_surface, Acquisition):
            surf, n_rows = acq_or_surface.Surface, len(acq_or_surface.prns)
        else:
            surf = acq_or_surface
            if n_rows is None:
                n_rows = int(acq_or_surface.shape[0])
        a = self.sv_array(sv)
        p0 = np.ascontiguousarray(np.asarray(p0, dtype=np.float64)[:3])
        R = np.ascontiguousarray(enu2ecef, dtype=np.float64).reshape(9)
        dp = C.POINTER(C.c_double)
        _check(lib().dpe_cd_update(self._h, _ptr(surf), C.c_int32(int(n_rows)), p0.ctypes.data_as(dp), R.ctypes.data_as(dp),
                                   C.c_int32(len(a)), a, _stream(stream)))
        self.n_sv = len(a)

    def results(self):
        """Synchronises.  -> (fix dict, per-SV list in Acquisition.results()' shape: Acquisition.fine takes it as it is)."""
        res, sv = CdResult(), (CdSvResult * max(self.n_sv, 1))()
        _check(lib().dpe_cd_results(self._h, C.byref(res), sv))
        fix = dict(point=res.point, m=res.m, j=res.j, score=res.score, bins_out_of_range=res.binsOutOfRange,
                   fix_ecef=np.array(res.fixEcef[:]), clock_bias_m=res.clockBiasM, clock_drift_mps=res.clockDriftMps)
        return fix, [dict(prn=r.prn, found=bool(r.found), max_code_idx=r.maxCodeIdx, max_dopp_idx=r.maxDoppIdx, rc=r.rc, fc=r.fc,
                          fi=r.fi, peak=r.peak) for r in sv[:self.n_sv]]

    def read_map(self, stream=None):
        """The position-domain map of the last update: (score float32 [P], jm int32 [P, 2]) -- per point the best score over
        (j, m) and that (j, m)."""
        return (d2h(self.MapScore, self.P * 4, np.float32, stream), d2h(self.MapJM, self.P * 8, np.int32, stream).reshape(self.P, 2))

    def close(self):
        if self._h:
            lib().dpe_cd_destroy(self._h)
            self._h = C.c_void_p(None)

    def __del__(self):
        try:            # at interpreter shutdown module globals may already be gone
            self.close()
        except Exception:
            pass


class FeConfig(C.Structure):        # dpe_fe_config
    _fields_ = [("samplingFrequency", C.c_double), ("intermediateFrequency", C.c_double), ("gain", C.c_double), ("levels", C.c_double * 4),
                ("format", C.c_int32), ("outputFormat", C.c_int32), ("decimation", C.c_int32), ("nTaps", C.c_int32)]


class FeInfo(C.Structure):          # dpe_fe_info_t
    _fields_ = [("realisedIF", C.c_double), ("outputFrequency", C.c_double), ("delta", C.c_int64), ("groupDelay", C.c_int32),
                ("bytesNum", C.c_int32), ("bytesDen", C.c_int32), ("tileOutputs", C.c_int32), ("ldsBytes", C.c_int32), ("reserved", C.c_int32)]


FE_FORMATS = {"I16C": 0, "I8C": 1, "I16R": 2, "I8R": 3, "ARGPI4": 4, "P2R": 5, "P2C": 6}      # DPE_FE_*


class _StreamStage:
    """What FrontEnd, Excisor and ArrayCombiner share (csrc/dpe_stream_plan.h): the end of the handle, the output tensors, the record
    length as the C ABI takes it, and the record cut that ends needed().  A subclass names its destroy symbol and sets out_f32."""
    _destroy = None

    def _new_out(self, out_count):
        import torch
        return torch.empty(2 * int(out_count), dtype=torch.float32 if self.out_f32 else torch.int16, device="cuda")

    @staticmethod
    def _record(record_length):
        return C.c_int64(-1 if record_length is None else int(record_length))

    @staticmethod
    def _cut(lo, hi, record_length):
        if record_length is not None:
            hi = min(hi, int(record_length))
        lo = max(lo, 0)
        return lo, max(hi, lo)

    def close(self):
        if self._h:
            getattr(lib(), self._destroy)(self._h)
            self._h = C.c_void_p(None)

    def __del__(self):
        try:            # at interpreter shutdown module globals may already be gone
            self.close()
        except Exception:
            pass


class FrontEnd(_StreamStage):
    """Raw record bytes on the device to interleaved int16 I/Q at zero IF and fs_in / D (dpe_fe_*, csrc/dpe_fe.hip):
    unpack, mix by the integer phase word, low-pass with the caller's odd-length taps, decimate.  The output is a torch int16
    tensor on the device that Acquisition.search, the trackers and every scan take as it is (out_f32: float pairs before
    rounding).  The handle keeps nothing of the record: any split of an output range into calls gives the bytes of one call."""
    _destroy = "dpe_fe_destroy"

    def __init__(self, fs_in, fmt, D, taps, gain=1.0, f_if=0.0, levels=(-3.0, -1.0, 1.0, 3.0), out_f32=False):
        if isinstance(fmt, str):
            if fmt.upper() not in FE_FORMATS:
                raise DpeError("[FrontEnd] create: input format %r is none of %s" % (fmt, ", ".join(FE_FORMATS)))
            fmt = FE_FORMATS[fmt.upper()]
        self.taps = np.ascontiguousarray(taps, dtype=np.float64).ravel()
        self.fs_in, self.D, self.T, self.out_f32 = float(fs_in), int(D), int(self.taps.size), bool(out_f32)
        cfg = FeConfig(self.fs_in, float(f_if), float(gain), (C.c_double * 4)(*[float(v) for v in levels]), int(fmt), 1 if out_f32 else 0,
                       self.D, self.T)
        self._h = C.c_void_p(None)
        _check(lib().dpe_fe_create(C.byref(cfg), self.taps.ctypes.data_as(C.POINTER(C.c_double)), C.byref(self._h)))
        info = FeInfo()
        _check(lib().dpe_fe_info(self._h, C.byref(info)))
        self.delta, self.realised_if, self.fs_out, self.T0 = int(info.delta), info.realisedIF, info.outputFrequency, int(info.groupDelay)
        self.bytes_num, self.bytes_den, self.tile_outputs, self.lds_bytes = int(info.bytesNum), int(info.bytesDen), int(info.tileOutputs), int(info.ldsBytes)

    def needed(self, out_first, out_count, record_length=None):
        """[lo, hi): the input samples the outputs [out_first, out_first + out_count) read, cut to the record."""
        return self._cut(int(out_first) * self.D - self.T0, (int(out_first) + int(out_count) - 1) * self.D + self.T - self.T0, record_length)

    def convert(self, raw, raw_first, out_first, out_count, record_length=None, raw_count=None, out=None, stream=None):
        """Outputs [out_first, out_first + out_count) from `raw`, a device tensor holding the record's input samples from
        raw_first on (raw_count of them; default: all its bytes hold).  Asynchronous.  Returns int16 [2 out_count], or float32
        [2 out_count] for out_f32."""
        if raw_count is None:
            raw_count = raw.numel() * raw.element_size() * self.bytes_den // self.bytes_num
        if out is None:
            out = self._new_out(out_count)
        _check(lib().dpe_fe_convert(self._h, _ptr(raw), C.c_int64(int(raw_first)), C.c_int64(int(raw_count)),
                                    self._record(record_length), _ptr(out), C.c_int64(int(out_first)),
                                    C.c_int64(int(out_count)), _stream(stream)))
        return out

    def clipped(self):
        """Output components the last int16 convert clipped to a rail.  Synchronises."""
        n = C.c_int64(0)
        _check(lib().dpe_fe_clipped(self._h, C.byref(n)))
        return int(n.value)


class IxConfig(C.Structure):        # dpe_ix_config
    _fields_ = [("threshold", C.c_double), ("blankPower", C.c_double), ("gain", C.c_double), ("frameLength", C.c_int32), ("guard", C.c_int32),
                ("inputFormat", C.c_int32), ("outputFormat", C.c_int32)]


class IxInfo(C.Structure):          # dpe_ix_info_t
    _fields_ = [("hop", C.c_int32), ("hopsPerBlock", C.c_int32), ("ldsBytes", C.c_int32), ("leadHops", C.c_int32), ("tailHops", C.c_int32),
                ("reserved", C.c_int32)]


class IxStats(C.Structure):         # dpe_ix_stats_t
    _fields_ = [("frames", C.c_int64), ("excisedBins", C.c_int64), ("blanked", C.c_int64), ("clipped", C.c_int64)]


class Excisor(_StreamStage):
    """Interference excision on complex baseband samples on the device (dpe_ix_*, csrc/dpe_ix.hip): a pulse blanker,
    then frames of N samples at a hop of N / 2 whose bins above `threshold` times the frame's lower median power (widened by
    `guard`, plus the always-excised `static_mask`) are set to zero before the frame is put back.  Takes and gives interleaved
    int16 I/Q (in_f32 / out_f32: float pairs) at the same rate, so it sits between FrontEnd.convert and every other stage.  The
    handle keeps nothing of the record: any split of an output range into calls gives the bytes of one call."""
    _destroy = "dpe_ix_destroy"

    def __init__(self, N, threshold, guard=1, blank_power=0.0, gain=1.0, static_mask=None, in_f32=False, out_f32=False):
        self.N, self.in_f32, self.out_f32 = int(N), bool(in_f32), bool(out_f32)
        cfg = IxConfig(float(threshold), float(blank_power), float(gain), self.N, int(guard), 1 if in_f32 else 0, 1 if out_f32 else 0)
        mask = None
        if static_mask is not None:
            mask = np.ascontiguousarray(np.asarray(static_mask) != 0, dtype=np.uint8).ravel()
            if mask.size != self.N:
                raise DpeError("[Excisor] create: the static mask holds %d bins, the frame %d" % (mask.size, self.N))
        self._h = C.c_void_p(None)
        _check(lib().dpe_ix_create(C.byref(cfg), None if mask is None else mask.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(self._h)))
        info = IxInfo()
        _check(lib().dpe_ix_info(self._h, C.byref(info)))
        self.hop, self.hops_per_block, self.lds_bytes = int(info.hop), int(info.hopsPerBlock), int(info.ldsBytes)
        self.lead_hops, self.tail_hops = int(info.leadHops), int(info.tailHops)

    def needed(self, out_first, out_count, record_length=None):
        """[lo, hi): the input samples the outputs [out_first, out_first + out_count) read, cut to the record."""
        H = self.N // 2
        return self._cut((int(out_first) // H - 1) * H, ((int(out_first) + int(out_count) - 1) // H + 2) * H, record_length)

    def _count(self, x, x_count):
        return x.numel() // 2 if x_count is None else int(x_count)

    def process(self, x, x_first, out_first, out_count, record_length=None, x_count=None, out=None, stream=None):
        """Outputs [out_first, out_first + out_count) from `x`, a device tensor (int16 or float32 [2 n]) holding the record's samples
        from x_first on.  Asynchronous.  Returns int16 [2 out_count], or float32 [2 out_count] for out_f32."""
        if out is None:
            out = self._new_out(out_count)
        _check(lib().dpe_ix_process(self._h, _ptr(x), C.c_int64(int(x_first)), C.c_int64(self._count(x, x_count)),
                                    self._record(record_length), _ptr(out), C.c_int64(int(out_first)),
                                    C.c_int64(int(out_count)), _stream(stream)))
        return out

    def stats(self):
        """The last process call's counters: frames, excisedBins, blanked, clipped, and excisedPerBin (int64 [N]).  Synchronises."""
        st = IxStats()
        per = np.zeros(self.N, dtype=np.int64)
        _check(lib().dpe_ix_stats(self._h, C.byref(st), per.ctypes.data_as(C.POINTER(C.c_int64))))
        return dict(frames=int(st.frames), excisedBins=int(st.excisedBins), blanked=int(st.blanked), clipped=int(st.clipped), excisedPerBin=per)

    def analyse(self, x, x_first, frame_first, frame_count, record_length=None, x_count=None, stream=None):
        """The device's own detection for the frames [frame_first, frame_first + frame_count): (P float32 [frames, N], m float32
        [frames], e uint8 [frames, N]) as device tensors -- the spectrogram of the record, and what process excises."""
        import torch
        n = max(int(frame_count), 0)
        P = torch.empty((n, self.N), dtype=torch.float32, device="cuda")
        m = torch.empty(n, dtype=torch.float32, device="cuda")
        e = torch.empty((n, self.N), dtype=torch.uint8, device="cuda")
        _check(lib().dpe_ix_analyse(self._h, _ptr(x), C.c_int64(int(x_first)), C.c_int64(self._count(x, x_count)),
                                    self._record(record_length), C.c_int64(int(frame_first)),
                                    C.c_int64(int(frame_count)), _ptr(P), _ptr(m), _ptr(e), _stream(stream)))
        return P, m, e


class ArrConfig(C.Structure):       # dpe_arr_config
    _fields_ = [("loading", C.c_double), ("gain", C.c_double), ("nElements", C.c_int32), ("blockLength", C.c_int32), ("nConstraints", C.c_int32),
                ("reference", C.c_int32), ("outputFormat", C.c_int32), ("reserved", C.c_int32)]


class ArrInfo(C.Structure):         # dpe_arr_info_t
    _fields_ = [("blockLength", C.c_int32), ("blocksPerUnit", C.c_int32), ("ldsBytes", C.c_int32), ("minSamples", C.c_int32)]


class ArrStats(C.Structure):        # dpe_arr_stats_t
    _fields_ = [("blocks", C.c_int64), ("fallbackBlocks", C.c_int64), ("clipped", C.c_int64)]


L1_WAVELENGTH = 299792458.0 / 1575.42e6


def steering_vectors(element_pos_m, los_unit, wavelength=L1_WAVELENGTH):
    """exp(2 pi j pos . los / wavelength) as complex128 [B, M]: the phase of a plane wave from the unit vectors los_unit [B, 3]
    (receiver to source) at the elements element_pos_m [M, 3] relative to the array's origin -- the constraints of ArrayCombiner for
    MVDR beams toward the line-of-sight vectors the channel manager holds."""
    pos = np.asarray(element_pos_m, dtype=np.float64).reshape(-1, 3)
    los = np.asarray(los_unit, dtype=np.float64).reshape(-1, 3)
    return np.exp(2j * np.pi * (los @ pos.T) / float(wavelength))


class ArrayCombiner(_StreamStage):
    """Antenna array combiner on the device (dpe_arr_*, csrc/dpe_arr.hip): n_elements streams of interleaved int16 I/Q
    to one stream per constraint, with weights adapted per block of block_length samples from the block's exact covariance, loaded
    by `loading` times its mean diagonal.  constraints=None is power inversion: the `reference` element passes with unit weight and
    whatever dominates the covariance is nulled; complex constraints [B, M] (steering_vectors) give B MVDR beams.  The output
    ("i16", or "f32" for float pairs before rounding) is what Acquisition.search, the trackers and every scan take.  The handle
    keeps nothing of the record: any split of an output range into calls gives the bytes of one call."""
    _destroy = "dpe_arr_destroy"

    def __init__(self, n_elements, block_length, constraints=None, reference=0, loading=1e-3, gain=1.0, output="i16"):
        if output not in ("i16", "f32"):
            raise DpeError("[ArrayCombiner] create: output %r is neither 'i16' nor 'f32'" % (output,))
        self.M, self.L, self.out_f32 = int(n_elements), int(block_length), output == "f32"
        cons = None
        self.B = 1
        if constraints is not None:
            cons = np.ascontiguousarray(np.atleast_2d(np.asarray(constraints, dtype=np.complex128)))
            if cons.ndim != 2 or cons.shape[1] != self.M:
                raise DpeError("[ArrayCombiner] create: constraints of shape %s, not [B, %d]" % (tuple(cons.shape), self.M))
            self.B = int(cons.shape[0])
        cfg = ArrConfig(float(loading), float(gain), self.M, self.L, self.B, int(reference), 1 if self.out_f32 else 0, 0)
        self._h = C.c_void_p(None)
        _check(lib().dpe_arr_create(C.byref(cfg), None if cons is None else cons.ctypes.data_as(C.POINTER(C.c_double)), C.byref(self._h)))
        info = ArrInfo()
        _check(lib().dpe_arr_info(self._h, C.byref(info)))
        self.blocks_per_unit, self.lds_bytes, self.min_samples = int(info.blocksPerUnit), int(info.ldsBytes), int(info.minSamples)

    def info(self):
        """dict(block_length, blocks_per_unit, lds_bytes, min_samples) of the handle"""
        return dict(block_length=self.L, blocks_per_unit=self.blocks_per_unit, lds_bytes=self.lds_bytes, min_samples=self.min_samples)

    def needed(self, first, count, record_length=None):
        """[lo, hi): the input samples of every element the outputs [first, first + count) read, cut to the record."""
        return self._cut(int(first) // self.L * self.L, ((int(first) + int(count) - 1) // self.L + 1) * self.L, record_length)

    def _elements(self, x, x_count):
        """-> (the host array of M device pointers, the samples each buffer holds)"""
        xs = list(x)
        if len(xs) != self.M:
            raise DpeError("[ArrayCombiner] %d input buffers for %d elements" % (len(xs), self.M))
        if x_count is None:
            x_count = xs[0].numel() // 2
        return (C.c_void_p * self.M)(*[_ptr(t) for t in xs]), int(x_count)

    def process(self, x, x_first, out_first, out_count, record_length=None, x_count=None, out=None, stream=None):
        """Outputs [out_first, out_first + out_count) of every constraint from `x`, a sequence of M device tensors (int16 [2 n], or
        the rows of one [M, 2 n] tensor), each holding its element's samples from x_first on.  Asynchronous.  Returns a list of B
        device tensors, int16 [2 out_count] or float32 [2 out_count] for "f32" (`out`: B tensors to write into)."""
        ptrs, n = self._elements(x, x_count)
        if out is None:
            out = [self._new_out(out_count) for _ in range(self.B)]
        outs = list(out)
        if len(outs) != self.B:
            raise DpeError("[ArrayCombiner] %d output buffers for %d constraints" % (len(outs), self.B))
        optrs = (C.c_void_p * self.B)(*[_ptr(t) for t in outs])
        _check(lib().dpe_arr_process(self._h, ptrs, C.c_int64(int(x_first)), C.c_int64(n), self._record(record_length),
                                     optrs, C.c_int64(int(out_first)), C.c_int64(int(out_count)), _stream(stream)))
        return outs

    def stats(self):
        """The last process call's counters: blocks, fallbackBlocks, clipped.  Synchronises."""
        st = ArrStats()
        _check(lib().dpe_arr_stats(self._h, C.byref(st)))
        return dict(blocks=int(st.blocks), fallbackBlocks=int(st.fallbackBlocks), clipped=int(st.clipped))

    def analyse(self, x, x_first, block_first, block_count, record_length=None, x_count=None, stream=None):
        """The device's own (S int64 [blocks, M, M, 2], w float64 [blocks, B, M, 2], v float32 [blocks, B, M, 2]) for the blocks
        [block_first, block_first + block_count) as device tensors: the covariances, the weights and what process applies."""
        import torch
        ptrs, n = self._elements(x, x_count)
        k = max(int(block_count), 0)
        S = torch.empty((k, self.M, self.M, 2), dtype=torch.int64, device="cuda")
        w = torch.empty((k, self.B, self.M, 2), dtype=torch.float64, device="cuda")
        v = torch.empty((k, self.B, self.M, 2), dtype=torch.float32, device="cuda")
        _check(lib().dpe_arr_analyse(self._h, ptrs, C.c_int64(int(x_first)), C.c_int64(n), self._record(record_length),
                                     C.c_int64(int(block_first)), C.c_int64(int(block_count)), _ptr(S), _ptr(w), _ptr(v), _stream(stream)))
        return S, w, v


class HipEventTimer:
    """HIP events recorded on the stream the kernels are launched on (bench.py roofline leg)."""

    def __init__(self):
        self.a, self.b = C.c_void_p(), C.c_void_p()
        _check(lib().dpe_event_create(C.byref(self.a)))
        _check(lib().dpe_event_create(C.byref(self.b)))

    def start(self, stream=None):
        _check(lib().dpe_event_record(self.a, _stream(stream)))

    def stop(self, stream=None):
        _check(lib().dpe_event_record(self.b, _stream(stream)))

    def elapsed_ms(self):
        ms = C.c_float()
        _check(lib().dpe_event_elapsed_ms(self.a, self.b, C.byref(ms)))
        return ms.value
