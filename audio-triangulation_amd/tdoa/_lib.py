"""ctypes binding of libtdoa.so (include/tdoa.h, include/tdoa_reference_abi.h).

This is the Python host side of the product: it only marshals device
pointers (torch tensors on the GPU) into the C ABI.  Every computation runs in
libtdoa's gfx950 kernels; if the library or a gfx950 device is missing the
calls raise -- there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TDOA_LIB") or os.path.join(HERE, "libtdoa.so")

ENGINE_DIRECT = 0
ENGINE_GCC_PHAT = 1
ENGINES = {"direct": ENGINE_DIRECT, "gcc_phat": ENGINE_GCC_PHAT}
SAMPLE_FORMATS = {"adc8": 0, "pcm16": 1}  # tdoa_sample_format
STREAM_TRIGGER_VAR_PCM16 = 131072  # TDOA_STREAM_TRIGGER_VAR_PCM16: 2 * 256^2 counts^2

STATUS = {0: "TDOA_OK", -1: "TDOA_ERR_INVALID", -2: "TDOA_ERR_HIP",
          -3: "TDOA_ERR_NO_DEVICE", -4: "TDOA_ERR_NOMEM"}

# Every symbol include/*.h declares (tests check the library exports them).
EXPORTED_SYMBOLS = [
    # tdoa.h
    "tdoa_config_default", "tdoa_create", "tdoa_destroy", "tdoa_get_dims",
    "tdoa_localize_batch", "tdoa_correlate_prepared", "tdoa_average_batch",
    "tdoa_decay_us", "tdoa_get_window", "tdoa_get_mics", "tdoa_get_lut",
    "tdoa_get_prior", "tdoa_dpss_q15", "tdoa_last_error", "tdoa_abi_version", "tdoa_batch_kernel",
    "tdoa_batch_grid_fused", "tdoa_gpu_clock_mhz",
    "tdoa_heatmap", "tdoa_peaks", "tdoa_stream_create", "tdoa_stream_step", "tdoa_stream_reset", "tdoa_stream_state",
    "tdoa_stream_destroy", "tdoa_stream_step_f", "tdoa_stream_state_f", "tdoa_stream_create_pcm16",
    "tdoa_stream_create_continuous", "tdoa_stream_peaks", "tdoa_stream_est_device",
    "tdoa_stream_kernel",
    "tdoa_track_batch", "tdoa_track_host", "tdoa_stream_track", "tdoa_stream_tracks_device",
    "tdoa_beam_fir", "tdoa_beam_geometry_of", "tdoa_beam_latency_of", "tdoa_beam_latency", "tdoa_get_beam_geometry",
    "tdoa_beam_batch", "tdoa_beam_host", "tdoa_stream_beam",
    "tdoa_sep_window", "tdoa_sep_check_of", "tdoa_sep_set_block", "tdoa_sep_get_block", "tdoa_sep_batch", "tdoa_stream_sep",
    "tdoa_band_weights", "tdoa_set_bin_weights", "tdoa_set_band_hz", "tdoa_get_bin_weights",
    "tdoa_set_sample_format", "tdoa_get_sample_format",
    # tdoa_reference_abi.h
    "microphones_init", "rolling_buffer_init", "rolling_buffer_push",
    "rolling_buffer_write_out", "rolling_buffer_get_incoming_power",
    "rolling_buffer_get_outgoing_power", "buffer_window",
    "buffer_normalize_range", "correlations_init", "correlations_average",
    "tdoa_ref_set_clock", "tdoa_ref_set_device",
    "mic_a_location", "mic_b_location", "mic_c_location",
]

SEP_MAX_TARGETS = 4   # TDOA_SEP_MAX_TARGETS
SEP_LOADING = 1e-2    # TDOA_SEP_LOADING


class TdoaError(RuntimeError):
    def __init__(self, code: int, where: str, msg: str):
        super().__init__(f"{where}: {STATUS.get(code, code)}: {msg}")
        self.code = code


class Config(C.Structure):
    """struct tdoa_config (include/tdoa.h)."""
    _fields_ = [
        ("num_mics", C.c_int32), ("frame_len", C.c_int32),
        ("sample_rate_hz", C.c_int32), ("max_shift", C.c_int32),
        ("speed_of_sound", C.c_float), ("engine", C.c_int32),
        ("mic_xy", C.POINTER(C.c_float)),
        ("grid_half_w", C.c_int32), ("grid_half_h", C.c_int32),
        ("grid_scale", C.c_float), ("height_offset", C.c_float),
        ("window_q15", C.POINTER(C.c_int32)), ("phat_eps", C.c_float),
    ]


class Outputs(C.Structure):
    """struct tdoa_outputs (include/tdoa.h): device pointers."""
    _fields_ = [(n, C.c_void_p) for n in (
        "lags", "gate", "cell", "xy", "max_L", "max_Lf", "scores", "weighted",
        "scores_f", "weighted_f", "xy_ls", "ls_rms")]


MAX_PEAKS = 8  # TDOA_MAX_PEAKS


class PeaksParams(C.Structure):
    """struct tdoa_peaks_params (include/tdoa.h)."""
    _fields_ = [("num_peaks", C.c_int32), ("radius", C.c_int32), ("min_rel", C.c_float)]


class PeaksOutputs(C.Structure):
    """struct tdoa_peaks_outputs (include/tdoa.h): device pointers."""
    _fields_ = [(n, C.c_void_p) for n in (
        "count", "cell", "xy", "L", "Lf", "lags", "xy_ls", "ls_rms")]


MAX_TRACKS = 8  # TDOA_MAX_TRACKS


class Track(C.Structure):
    """struct tdoa_track (include/tdoa.h): one 64-byte track record."""
    _fields_ = [("id", C.c_int32), ("status", C.c_int32), ("hits", C.c_int32), ("misses", C.c_int32),
                ("x", C.c_float), ("y", C.c_float), ("vx", C.c_float), ("vy", C.c_float),
                ("p00", C.c_float), ("p01", C.c_float), ("p11", C.c_float), ("peak", C.c_int32),
                ("t_us", C.c_int64), ("upd_us", C.c_int64)]


# the same record as a numpy structured dtype (the fields are naturally aligned: no padding)
TRACK_FIELDS = [("id", "<i4"), ("status", "<i4"), ("hits", "<i4"), ("misses", "<i4"),
                ("x", "<f4"), ("y", "<f4"), ("vx", "<f4"), ("vy", "<f4"),
                ("p00", "<f4"), ("p01", "<f4"), ("p11", "<f4"), ("peak", "<i4"),
                ("t_us", "<i8"), ("upd_us", "<i8")]
TRACK_STATUS = {0: "free", 1: "tentative", 2: "confirmed"}


class TrackParams(C.Structure):
    """struct tdoa_track_params (include/tdoa.h).  Lengths in metres, times in
    seconds (max_coast_us in microseconds): meas_var r is the variance of a peak
    position (m^2), accel_psd q the power spectral density of the unmodelled
    acceleration (m^2/s^3), init_vel_var the velocity variance of a newborn
    track (m^2/s^2), gate_d2 the largest accepted |z - x|^2 / (p00 + r)."""
    _fields_ = [("max_tracks", C.c_int32), ("confirm_hits", C.c_int32), ("max_misses", C.c_int32),
                ("max_coast_us", C.c_int64), ("gate_d2", C.c_float), ("meas_var", C.c_float),
                ("accel_psd", C.c_float), ("init_vel_var", C.c_float)]


# defaults of the Python faces: a grid cell at the default scale is 1/24 m, so
# r = 0.01 m^2 is a 10 cm (2.4-cell) standard deviation; a gate of 9 is 3 sigma
TRACK_DEFAULTS = dict(max_tracks=8, confirm_hits=3, max_misses=5, max_coast_us=2_000_000, gate_d2=9.0,
                      meas_var=0.01, accel_psd=1.0, init_vel_var=4.0)


def track_params(**kw) -> TrackParams:
    """TrackParams from TRACK_DEFAULTS overridden by keywords."""
    bad = set(kw) - set(TRACK_DEFAULTS)
    if bad:
        raise TypeError(f"unknown track parameter(s) {sorted(bad)}")
    v = {**TRACK_DEFAULTS, **kw}
    return TrackParams(int(v["max_tracks"]), int(v["confirm_hits"]), int(v["max_misses"]), int(v["max_coast_us"]),
                       float(v["gate_d2"]), float(v["meas_var"]), float(v["accel_psd"]), float(v["init_vel_var"]))


class TrackOutputs(C.Structure):
    """struct tdoa_track_outputs (include/tdoa.h): any may be NULL, not all."""
    _fields_ = [(n, C.c_void_p) for n in ("tracks", "assigned", "num_confirmed")]


BEAM_HALF, BEAM_PHASES, BEAM_MAX_TARGETS = 8, 32, 8  # TDOA_BEAM_HALF, TDOA_BEAM_PHASES, TDOA_BEAM_MAX_TARGETS


class BeamGeometry(C.Structure):
    """struct tdoa_beam_geometry (include/tdoa.h): what steering reads of a context."""
    _fields_ = [("num_mics", C.c_int32), ("sample_rate_hz", C.c_int32), ("speed_of_sound", C.c_float),
                ("height_offset", C.c_float), ("mic_xy", C.c_float * 16)]


class BeamOutputs(C.Structure):
    """struct tdoa_beam_outputs (include/tdoa.h): audio is required."""
    _fields_ = [(n, C.c_void_p) for n in ("audio", "delays", "active", "block_start")]


class StreamOutputs(C.Structure):
    """struct tdoa_stream_outputs (include/tdoa.h): device pointers."""
    _fields_ = [(n, C.c_void_p) for n in (
        "count", "stream_id", "end", "lags", "gate", "ema_best", "cell", "xy", "max_L")]


class StreamOutputsF(C.Structure):
    """struct tdoa_stream_outputs_f (a GCC_PHAT pipeline): device pointers."""
    _fields_ = [(n, C.c_void_p) for n in (
        "count", "stream_id", "end", "lags", "gate", "ema_best", "cell", "xy", "max_Lf")]


# reference structs (include/tdoa_reference_abi.h, reference buffer.h:8-12,
# rolling_buffer.h:13-25, correlations.h:10-16, point.h:3-6)
class Buffer(C.Structure):
    _fields_ = [("buffer", C.c_int16 * 1024), ("power", C.c_int64)]


class RollingBuffer(C.Structure):
    _fields_ = [("head", C.c_int), ("incoming_power", C.c_int64),
                ("incoming_total", C.c_int64), ("outgoing_power", C.c_int64),
                ("outgoing_total", C.c_int64), ("is_full", C.c_bool),
                ("buffer", C.c_int16 * 1024)]


class Correlations(C.Structure):
    _fields_ = [("correlations", C.c_int64 * 93), ("best_shift", C.c_int),
                ("last_update", C.c_uint64)]


class Point2d(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float)]


CLOCK_FN = C.CFUNCTYPE(C.c_uint64)

_lib = None


def load() -> C.CDLL:
    """Load libtdoa.so (built in-tree by __graft_entry__.build / make)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise TdoaError(-3, "load", f"{LIB_PATH} missing: run `make -C audio-triangulation_amd`")
    L = C.CDLL(LIB_PATH)
    P, I32, I64 = C.c_void_p, C.c_int32, C.c_int64
    L.tdoa_config_default.argtypes = [C.POINTER(Config)]
    L.tdoa_create.argtypes = [C.POINTER(Config), C.c_int, C.POINTER(P)]
    L.tdoa_destroy.argtypes = [P]
    L.tdoa_get_dims.argtypes = [P] + [C.POINTER(I32)] * 5
    L.tdoa_localize_batch.argtypes = [P, P, I64, C.POINTER(Outputs), P]
    L.tdoa_correlate_prepared.argtypes = [P, P, I64, C.POINTER(Outputs), P]
    L.tdoa_average_batch.argtypes = [P, I64, P, P, P, P, C.POINTER(Outputs), P]
    L.tdoa_decay_us.argtypes = [C.c_uint64, C.c_uint64]
    L.tdoa_decay_us.restype = C.c_float
    L.tdoa_get_window.argtypes = [P, P]
    L.tdoa_get_mics.argtypes = [P, P]
    L.tdoa_get_lut.argtypes = [P, P]
    L.tdoa_get_prior.argtypes = [P, P]
    L.tdoa_dpss_q15.argtypes = [I32, C.c_double, P]
    L.tdoa_last_error.restype = C.c_char_p
    L.tdoa_abi_version.restype = C.c_int
    L.tdoa_batch_kernel.argtypes = [P]
    L.tdoa_batch_kernel.restype = C.c_char_p
    L.tdoa_batch_grid_fused.argtypes = [P]
    L.tdoa_batch_grid_fused.restype = C.c_int
    L.tdoa_gpu_clock_mhz.argtypes = [C.c_int, P, C.c_double, C.POINTER(C.c_double)]
    L.tdoa_heatmap.argtypes = [P, P, P, C.c_int, I64, P, P]
    L.tdoa_peaks.argtypes = [P, P, C.c_int, I64, C.POINTER(PeaksParams), C.POINTER(PeaksOutputs), P]
    L.tdoa_stream_create.argtypes = [P, I32, I32, P, I64, C.c_int, C.POINTER(P)]
    L.tdoa_stream_create_pcm16.argtypes = [P, I32, I32, P, I64, I64, C.c_int, C.POINTER(P)]
    L.tdoa_stream_create_continuous.argtypes = [P, I32, I32, P, I64, I64, C.c_int, C.POINTER(P)]
    L.tdoa_stream_step.argtypes = [P, C.POINTER(StreamOutputs), P]
    L.tdoa_stream_reset.argtypes = [P, P]
    L.tdoa_stream_state.argtypes = [P, P, P, P, P]
    L.tdoa_stream_step_f.argtypes = [P, C.POINTER(StreamOutputsF), P]
    L.tdoa_stream_state_f.argtypes = [P, P, P, P, P]
    L.tdoa_stream_destroy.argtypes = [P]
    L.tdoa_stream_peaks.argtypes = [P, C.POINTER(PeaksParams), P, C.POINTER(PeaksOutputs), P]
    L.tdoa_stream_est_device.argtypes = [P, C.POINTER(P), C.POINTER(C.c_int)]
    L.tdoa_stream_kernel.argtypes = [P]
    L.tdoa_stream_kernel.restype = C.c_char_p
    track_tail = [P, I32, C.POINTER(TrackParams), C.POINTER(TrackOutputs)]  # xy, Kp, prm, out
    L.tdoa_track_batch.argtypes = [C.c_int, P, P, I64, P, P, P] + track_tail + [P]
    L.tdoa_track_host.argtypes = [P, P, I64, P, P, P] + track_tail
    L.tdoa_stream_track.argtypes = [P, C.POINTER(TrackParams), P] + track_tail[:2] + [C.POINTER(TrackOutputs), P]
    L.tdoa_stream_tracks_device.argtypes = [P, C.POINTER(P), C.POINTER(P)]
    L.tdoa_beam_fir.argtypes = [P]
    L.tdoa_beam_geometry_of.argtypes = [C.POINTER(Config), C.POINTER(BeamGeometry)]
    L.tdoa_beam_latency_of.argtypes = [C.POINTER(BeamGeometry), C.POINTER(I32), C.POINTER(I32)]
    L.tdoa_beam_latency.argtypes = [P, C.POINTER(I32), C.POINTER(I32)]
    L.tdoa_get_beam_geometry.argtypes = [P, C.POINTER(BeamGeometry)]
    L.tdoa_beam_batch.argtypes = [P, P, I64, P, P, I32, C.POINTER(BeamOutputs), P]
    L.tdoa_beam_host.argtypes = [C.POINTER(BeamGeometry), I32, P, I64, P, P, I32, C.POINTER(BeamOutputs)]
    L.tdoa_stream_beam.argtypes = [P, P, P, I32, I32, C.POINTER(BeamOutputs), P]
    L.tdoa_sep_window.argtypes = [I32, P]
    L.tdoa_sep_check_of.argtypes = [C.POINTER(BeamGeometry), I32, I32, C.c_float]
    L.tdoa_sep_set_block.argtypes = [P, I32]
    L.tdoa_sep_get_block.argtypes = [P, C.POINTER(I32)]
    L.tdoa_sep_batch.argtypes = [P, P, I64, P, P, I32, C.c_float, C.POINTER(BeamOutputs), P]
    L.tdoa_stream_sep.argtypes = [P, P, P, I32, I32, C.c_float, C.POINTER(BeamOutputs), P]
    L.tdoa_band_weights.argtypes = [I32, I32, C.c_double, C.c_double, C.c_double, P]
    L.tdoa_set_bin_weights.argtypes = [P, P]
    L.tdoa_set_band_hz.argtypes = [P, C.c_double, C.c_double, C.c_double]
    L.tdoa_get_bin_weights.argtypes = [P, P]
    L.tdoa_set_sample_format.argtypes = [P, C.c_int]
    L.tdoa_get_sample_format.argtypes = [P, C.POINTER(C.c_int)]
    # reference-named per-frame symbols
    L.microphones_init.argtypes = []
    L.rolling_buffer_init.argtypes = [C.POINTER(RollingBuffer)]
    L.rolling_buffer_push.argtypes = [C.POINTER(RollingBuffer), C.c_int16]
    L.rolling_buffer_write_out.argtypes = [C.POINTER(RollingBuffer), C.POINTER(Buffer)]
    L.rolling_buffer_get_incoming_power.argtypes = [C.POINTER(RollingBuffer)]
    L.rolling_buffer_get_incoming_power.restype = C.c_int64
    L.rolling_buffer_get_outgoing_power.argtypes = [C.POINTER(RollingBuffer)]
    L.rolling_buffer_get_outgoing_power.restype = C.c_int64
    L.buffer_window.argtypes = [C.POINTER(Buffer)]
    L.buffer_normalize_range.argtypes = [C.POINTER(Buffer)]
    L.correlations_init.argtypes = [C.POINTER(Correlations), C.POINTER(Buffer), C.POINTER(Buffer)]
    L.correlations_average.argtypes = [C.POINTER(Correlations), C.POINTER(Correlations)]
    L.tdoa_ref_set_clock.argtypes = [CLOCK_FN]
    L.tdoa_ref_set_device.argtypes = [C.c_int]
    _lib = L
    return L


def check(rc: int, where: str) -> None:
    if rc != 0:
        msg = load().tdoa_last_error()
        raise TdoaError(rc, where, msg.decode() if msg else "")


def dpss_q15(n: int, nw: float = 2.0):
    """DPSS(n, nw) Q15 window from libtdoa's host generator."""
    import numpy as np
    out = np.zeros(n, np.int32)
    check(load().tdoa_dpss_q15(n, nw, out.ctypes.data_as(C.c_void_p)), "tdoa_dpss_q15")
    return out


def band_weights(N: int, fs: int, lo: float, hi: float, taper: float = 0.0):
    """Band mask float32 [N + 1] over the bins k * fs / 2N of the 2N-point
    spectrum (tdoa_band_weights): 1 in [lo, hi] Hz, raised-cosine edges of
    `taper` Hz outside, 0 elsewhere.  Host only."""
    import numpy as np
    w = np.zeros(max(int(N), 0) + 1, np.float32)
    check(load().tdoa_band_weights(int(N), int(fs), float(lo), float(hi), float(taper),
                                   w.ctypes.data_as(C.c_void_p)), "tdoa_band_weights")
    return w


def decay_us(now_us: int, last_us: int) -> float:
    return float(load().tdoa_decay_us(int(now_us), int(last_us)))


def track_host(tracks, next_id, t_us, count, xy, stream_of_row=None, **params) -> dict:
    """tdoa_track_host: the tracker's rule (include/tdoa.h, "Tracking") on numpy
    arrays, no device.  tracks [S][8] TRACK_DTYPE and next_id [S] int32 are the
    state, updated in place; t_us [rows] int64, count [rows] int32 and
    xy [rows][Kp][2] float32 are the rows, row i being stream stream_of_row[i]
    (None: stream i).  Returns tracks [rows][T], assigned [rows][Kp] and
    num_confirmed [rows]."""
    import numpy as np
    dt = np.dtype(TRACK_FIELDS)
    if not (isinstance(tracks, np.ndarray) and tracks.dtype == dt and tracks.ndim == 2
            and tracks.shape[1] == MAX_TRACKS and tracks.flags.c_contiguous and tracks.flags.writeable):
        raise ValueError(f"tracks must be a writable C-contiguous [S][{MAX_TRACKS}] array of TRACK_DTYPE")
    S = tracks.shape[0]
    if not (isinstance(next_id, np.ndarray) and next_id.dtype == np.int32 and next_id.shape == (S,)
            and next_id.flags.c_contiguous and next_id.flags.writeable):
        raise ValueError("next_id must be a writable int32 [S] array")
    xy = np.ascontiguousarray(xy, np.float32)
    if xy.ndim != 3 or xy.shape[2] != 2:
        raise ValueError("xy must be [rows][Kp][2]")
    rows, Kp = xy.shape[0], xy.shape[1]
    t_us = np.ascontiguousarray(t_us, np.int64)
    count = np.ascontiguousarray(count, np.int32)
    if t_us.shape != (rows,) or count.shape != (rows,):
        raise ValueError("t_us and count must be [rows]")
    sor = None
    if stream_of_row is not None:
        sor = np.ascontiguousarray(stream_of_row, np.int32)
        if sor.shape != (rows,) or (rows and (sor.min() < 0 or sor.max() >= S)):
            raise ValueError("stream_of_row must be [rows] with entries in [0, S)")
    elif rows > S:
        raise ValueError("more rows than streams")
    prm = track_params(**params)
    T = min(max(prm.max_tracks, 1), MAX_TRACKS)
    o = {"tracks": np.zeros((rows, T), dt), "assigned": np.zeros((rows, Kp), np.int32),
         "num_confirmed": np.zeros(rows, np.int32)}
    stub = np.zeros(1, np.int64)  # rows = 0: an empty array's address may be NULL, and nothing is read

    def ptr(a):
        return (a if a.size else stub).ctypes.data_as(C.c_void_p)
    out = TrackOutputs(*[ptr(o[n]) for n, _ in TrackOutputs._fields_])
    check(load().tdoa_track_host(ptr(tracks), ptr(next_id), rows, None if sor is None else ptr(sor), ptr(t_us),
                                 ptr(count), ptr(xy), Kp, C.byref(prm), C.byref(out)), "tdoa_track_host")
    return o


def beam_fir():
    """The beamformer's fractional-delay FIR table (tdoa_beam_fir): float32
    [32][16], phase q, tap k = -7..8 at [q][k + 7].  Host only."""
    import numpy as np
    h = np.zeros((BEAM_PHASES, 2 * BEAM_HALF), np.float32)
    check(load().tdoa_beam_fir(h.ctypes.data_as(C.c_void_p)), "tdoa_beam_fir")
    return h


def beam_geometry(mic_xy=None, num_mics: int = 3, sample_rate_hz: int = 50000, speed_of_sound: float = 343.0,
                  height_offset: float = 1.2) -> BeamGeometry:
    """BeamGeometry of the context these config fields would make
    (tdoa_beam_geometry_of): mic_xy [M][2] metres, None with 3 mics for the
    reference triangle.  Host only."""
    import numpy as np
    cfg = Config()
    check(load().tdoa_config_default(C.byref(cfg)), "tdoa_config_default")
    mics = None
    if mic_xy is not None:
        mics = np.ascontiguousarray(mic_xy, np.float32)
        if mics.ndim != 2 or mics.shape[1] != 2:
            raise ValueError("mic_xy must be [M][2]")
        num_mics = mics.shape[0]
        cfg.mic_xy = mics.ctypes.data_as(C.POINTER(C.c_float))
    cfg.num_mics, cfg.sample_rate_hz = int(num_mics), int(sample_rate_hz)
    cfg.speed_of_sound, cfg.height_offset = float(speed_of_sound), float(height_offset)
    g = BeamGeometry()
    check(load().tdoa_beam_geometry_of(C.byref(cfg), C.byref(g)), "tdoa_beam_geometry_of")
    return g


def beam_latency(geometry: BeamGeometry):
    """(A, Dmax) of a geometry in samples (tdoa_beam_latency_of): output sample
    n needs the input up to n + A; no delay code exceeds 32 Dmax."""
    a, d = C.c_int32(), C.c_int32()
    check(load().tdoa_beam_latency_of(C.byref(geometry), C.byref(a), C.byref(d)), "tdoa_beam_latency_of")
    return a.value, d.value


def beam_host(geometry: BeamGeometry, frames, xy, count=None) -> dict:
    """tdoa_beam_host: the beamformer's rule (include/tdoa.h, "Listening") on
    numpy arrays, no device.  frames int16 [B][M][N] (any N >= 1), xy float32
    [B][Kt][2] plane coordinates, count int32 [B] (None: all Kt).  Returns audio
    float32 [B][Kt][N], delays int32 [B][Kt][M] (the codes, -1 invalid) and
    active uint8 [B][Kt]."""
    import numpy as np
    frames = np.ascontiguousarray(frames, np.int16)
    xy = np.ascontiguousarray(xy, np.float32)
    M = geometry.num_mics
    if frames.ndim != 3 or frames.shape[1] != M:
        raise ValueError(f"frames must be int16 [B][{M}][N]")
    B, _, N = frames.shape
    if xy.ndim != 3 or xy.shape[0] != B or xy.shape[2] != 2:
        raise ValueError("xy must be [B][Kt][2]")
    Kt = xy.shape[1]
    if count is not None:
        count = np.ascontiguousarray(count, np.int32)
        if count.shape != (B,):
            raise ValueError("count must be [B]")
    o = {"audio": np.zeros((B, Kt, N), np.float32), "delays": np.zeros((B, Kt, M), np.int32),
         "active": np.zeros((B, Kt), np.uint8)}
    stub = np.zeros(1, np.int64)  # B = 0: an empty array's address may be NULL, and nothing is read

    def ptr(a):
        return (a if a.size else stub).ctypes.data_as(C.c_void_p)
    out = BeamOutputs(ptr(o["audio"]), ptr(o["delays"]), ptr(o["active"]), None)
    check(load().tdoa_beam_host(C.byref(geometry), N, ptr(frames), B, None if count is None else ptr(count), ptr(xy),
                                Kt, C.byref(out)), "tdoa_beam_host")
    return o


def sep_window(L: int):
    """The separator's analysis / synthesis window (tdoa_sep_window): float32
    [L], periodic sqrt-Hann, L a power of two in 128..2048.  Host only."""
    import numpy as np
    g = np.zeros(max(int(L), 1), np.float32)
    check(load().tdoa_sep_window(int(L), g.ctypes.data_as(C.c_void_p)), "tdoa_sep_window")
    return g


def sep_check(geometry: BeamGeometry, L: int, num_targets: int = 1, loading: float = SEP_LOADING) -> None:
    """Raises TdoaError unless a geometry, a block length L, a target count
    and a loading make a block the separator takes (tdoa_sep_check_of: L a
    power of two in 128..2048, L >= 8 Dmax, 1..4 targets, loading in
    [1e-4, 1e4]).  Host only."""
    check(load().tdoa_sep_check_of(C.byref(geometry), int(L), int(num_targets), float(loading)), "tdoa_sep_check_of")
