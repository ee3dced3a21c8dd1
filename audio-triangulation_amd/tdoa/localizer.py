"""Batched localizer: the Python face of include/tdoa.h.

`Localizer.localize(frames)` is the batched form of the reference's per-frame
hot path (sample_compute.h:105-134 -> vga_heatmap.h:99-108).  Inputs and
outputs are torch tensors on the context's GPU; torch only provides device
memory and the stream -- the work is libtdoa's kernels.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np
import torch

from . import _lib
from ._lib import (BeamGeometry, BeamOutputs, Config, Outputs, PeaksOutputs, PeaksParams, TrackOutputs, check, load,
                   track_params)


def _ptr(t: torch.Tensor | None):
    return None if t is None else C.c_void_p(t.data_ptr())


@dataclass
class Geometry:
    """Derived sizes of a context: M mics, N samples, P pairs, K lags, G cells."""
    M: int
    N: int
    P: int
    K: int
    G: int
    S: int = field(init=False)

    def __post_init__(self):
        self.S = (self.K - 1) // 2


class Localizer:
    """One libtdoa context bound to one GPU (not thread-safe).

    engine: "direct" (exact int64, the reference's semantics bit-for-bit) or
    "gcc_phat" (fp32 FFT cross-spectrum with PHAT weighting).
    sample_format: "adc8" (the reference's 8-bit ADC front end: the low byte of
    every sample) or "pcm16" (full-range int16 frames, GCC_PHAT only; see
    set_sample_format).
    """

    def __init__(self, num_mics: int = 3, frame_len: int = 1024,
                 sample_rate_hz: int = 50000, max_shift: int = 0,
                 engine: str = "direct", mic_xy=None, grid_half_w: int = 50,
                 grid_half_h: int = 50, grid_scale: float = 24.0,
                 height_offset: float = 1.2, speed_of_sound: float = 343.0,
                 window_q15=None, phat_eps: float = 1e-12, device: int = 0,
                 band_hz=None, band_taper_hz: float = 0.0, sample_format: str = "adc8"):
        L = load()
        cfg = Config()
        L.tdoa_config_default(C.byref(cfg))
        cfg.num_mics = num_mics
        cfg.frame_len = frame_len
        cfg.sample_rate_hz = sample_rate_hz
        cfg.max_shift = max_shift
        cfg.speed_of_sound = speed_of_sound
        cfg.engine = _lib.ENGINES[engine]
        cfg.grid_half_w = grid_half_w
        cfg.grid_half_h = grid_half_h
        cfg.grid_scale = grid_scale
        cfg.height_offset = height_offset
        cfg.phat_eps = phat_eps
        self._keep = []
        if mic_xy is not None:
            a = np.ascontiguousarray(mic_xy, dtype=np.float32).reshape(-1)
            assert a.size == 2 * num_mics, "mic_xy must be [num_mics][2]"
            self._keep.append(a)
            cfg.mic_xy = a.ctypes.data_as(C.POINTER(C.c_float))
        if window_q15 is not None:
            w = np.ascontiguousarray(window_q15, dtype=np.int32)
            assert w.size == frame_len
            self._keep.append(w)
            cfg.window_q15 = w.ctypes.data_as(C.POINTER(C.c_int32))
        self.engine = engine
        self.device = device
        self.torch_device = torch.device("cuda", device)
        ctx = C.c_void_p()
        check(L.tdoa_create(C.byref(cfg), device, C.byref(ctx)), "tdoa_create")
        self._ctx = ctx
        d = [C.c_int32() for _ in range(5)]
        check(L.tdoa_get_dims(ctx, *[C.byref(x) for x in d]), "tdoa_get_dims")
        self.dims = Geometry(*[x.value for x in d])
        self.grid_W = 2 * grid_half_w + 1
        self.grid_half_w, self.grid_half_h, self.grid_scale = grid_half_w, grid_half_h, grid_scale
        try:
            if band_hz is not None:
                self.set_band(band_hz[0], band_hz[1], band_taper_hz)
            if sample_format != "adc8":
                self.set_sample_format(sample_format)
        except Exception:
            self.close()
            raise

    # ---------------------------------------------------------- lifetime
    def close(self):
        if getattr(self, "_ctx", None):
            load().tdoa_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---------------------------------------------------------- tables
    def batch_kernel(self) -> str:
        """Name of the kernel a batch of this context runs first (tdoa_batch_kernel)."""
        return (load().tdoa_batch_kernel(self._ctx) or b"").decode()

    def batch_grid_fused(self) -> bool:
        """A grid-requesting batch solves the grid inside its first kernel (tdoa_batch_grid_fused)."""
        return bool(load().tdoa_batch_grid_fused(self._ctx))

    def window(self) -> np.ndarray:
        w = np.zeros(self.dims.N, np.int32)
        check(load().tdoa_get_window(self._ctx, w.ctypes.data_as(C.c_void_p)), "tdoa_get_window")
        return w

    def mics(self) -> np.ndarray:
        m = np.zeros((self.dims.M, 2), np.float32)
        check(load().tdoa_get_mics(self._ctx, m.ctypes.data_as(C.c_void_p)), "tdoa_get_mics")
        return m

    def lut(self) -> np.ndarray:
        lut = np.zeros((self.dims.P, self.dims.G), np.uint8)
        check(load().tdoa_get_lut(self._ctx, lut.ctypes.data_as(C.c_void_p)), "tdoa_get_lut")
        return lut

    def prior(self) -> np.ndarray:
        p = np.zeros(self.dims.K, np.float32)
        check(load().tdoa_get_prior(self._ctx, p.ctypes.data_as(C.c_void_p)), "tdoa_get_prior")
        return p

    # ---------------------------------------------------------- band limiting
    def set_band(self, lo: float, hi: float, taper: float = 0.0) -> None:
        """Band-limited GCC-PHAT (tdoa_set_band_hz): only the bins in [lo, hi] Hz,
        with raised-cosine edges of `taper` Hz, vote.  Synchronous; not while
        a call of this context is in flight."""
        check(load().tdoa_set_band_hz(self._ctx, float(lo), float(hi), float(taper)), "tdoa_set_band_hz")

    def set_bin_weights(self, w) -> None:
        """Per-bin weights float [N + 1] on the cross spectrum, finite and >= 0
        (tdoa_set_bin_weights); None clears the table and the context runs its
        unweighted kernels again.  Synchronous; not while a call is in flight."""
        if w is None:
            check(load().tdoa_set_bin_weights(self._ctx, None), "tdoa_set_bin_weights")
            return
        a = np.ascontiguousarray(w, dtype=np.float32).reshape(-1)
        if a.size != self.dims.N + 1:
            raise ValueError(f"bin weights must be [{self.dims.N + 1}], got {a.size}")
        check(load().tdoa_set_bin_weights(self._ctx, a.ctypes.data_as(C.c_void_p)), "tdoa_set_bin_weights")

    def bin_weights(self) -> np.ndarray:
        """The table in force, float32 [N + 1]; all ones when none is set."""
        w = np.zeros(self.dims.N + 1, np.float32)
        check(load().tdoa_get_bin_weights(self._ctx, w.ctypes.data_as(C.c_void_p)), "tdoa_get_bin_weights")
        return w

    # ---------------------------------------------------------- 16-bit input
    def set_sample_format(self, fmt: str) -> None:
        """"adc8": the 8-bit ADC front end ((x - off) << 8 in int16, the low
        byte of every sample), every kernel and bit as before.  "pcm16":
        full-range int16 frames, s = ((x - floor mean) * W) >> 15 without the
        wrap (tdoa_set_sample_format; GCC_PHAT only).  Synchronous; not while
        a call of this context is in flight."""
        if fmt not in _lib.SAMPLE_FORMATS:
            raise ValueError(f"sample_format must be one of {sorted(_lib.SAMPLE_FORMATS)}, got {fmt!r}")
        check(load().tdoa_set_sample_format(self._ctx, _lib.SAMPLE_FORMATS[fmt]), "tdoa_set_sample_format")

    @property
    def sample_format(self) -> str:
        """The format in force: "adc8" or "pcm16"."""
        v = C.c_int()
        check(load().tdoa_get_sample_format(self._ctx, C.byref(v)), "tdoa_get_sample_format")
        return {n: k for k, n in _lib.SAMPLE_FORMATS.items()}[v.value]

    # ---------------------------------------------------------- compute
    def alloc_outputs(self, B: int, scores: bool = False, grid: bool = True,
                      ls: bool = False, engine: str | None = None) -> dict:
        """Output tensors for a batch of B frames; `engine` overrides the
        context's (the prepared path always fills the DIRECT int64 set)."""
        dev, P, K = self.torch_device, self.dims.P, self.dims.K
        direct = (engine or self.engine) == "direct"
        o = {"lags": torch.empty((B, P), dtype=torch.int32, device=dev),
             "gate": torch.empty(B, dtype=torch.uint8, device=dev)}
        if grid:
            o["cell"] = torch.empty(B, dtype=torch.int32, device=dev)
            o["xy"] = torch.empty((B, 2), dtype=torch.float32, device=dev)
            if direct:
                o["max_L"] = torch.empty(B, dtype=torch.int64, device=dev)
            else:
                o["max_Lf"] = torch.empty(B, dtype=torch.float32, device=dev)
        if ls:
            o["xy_ls"] = torch.empty((B, 2), dtype=torch.float32, device=dev)
            o["ls_rms"] = torch.empty(B, dtype=torch.float32, device=dev)
        if scores:
            if direct:
                o["scores"] = torch.empty((B, P, K), dtype=torch.int64, device=dev)
                o["weighted"] = torch.empty((B, P, K), dtype=torch.int64, device=dev)
            else:
                o["scores_f"] = torch.empty((B, P, K), dtype=torch.float32, device=dev)
                o["weighted_f"] = torch.empty((B, P, K), dtype=torch.float32, device=dev)
        return o

    @staticmethod
    def _outputs_struct(o: dict) -> Outputs:
        s = Outputs()
        for name, _ in Outputs._fields_:
            t = o.get(name)
            setattr(s, name, None if t is None else t.data_ptr())
        return s

    def _check_frames(self, frames: torch.Tensor) -> int:
        M, N = self.dims.M, self.dims.N
        if frames.dtype != torch.int16 or frames.dim() != 3 or tuple(frames.shape[1:]) != (M, N):
            raise ValueError(f"frames must be int16 [B][{M}][{N}], got {tuple(frames.shape)} {frames.dtype}")
        if frames.device != self.torch_device:
            raise ValueError(f"frames must live on {self.torch_device}")
        if not frames.is_contiguous():
            raise ValueError("frames must be contiguous")
        return frames.shape[0]

    def localize_into(self, frames: torch.Tensor, out: dict, stream=None) -> dict:
        """Asynchronous batched localization into preallocated outputs."""
        B = self._check_frames(frames)
        st = stream if stream is not None else torch.cuda.current_stream(self.torch_device)
        s = self._outputs_struct(out)
        check(load().tdoa_localize_batch(self._ctx, C.c_void_p(frames.data_ptr()), B,
                                         C.byref(s), C.c_void_p(st.cuda_stream)),
              "tdoa_localize_batch")
        return out

    def prepare(self, frames: torch.Tensor, out: dict, stream=None):
        """A prebuilt localize_into(frames, out, stream): the argument checks and
        the ctypes output struct are done once, and each call of the returned
        function enqueues the same tdoa_localize_batch (frames and outputs must
        stay allocated; they are kept referenced).  For launch loops whose
        host-side Python would otherwise be on the critical path."""
        B = self._check_frames(frames)
        st = stream if stream is not None else torch.cuda.current_stream(self.torch_device)
        s = self._outputs_struct(out)
        fn = load().tdoa_localize_batch
        args = (self._ctx, C.c_void_p(frames.data_ptr()), B, C.byref(s), C.c_void_p(st.cuda_stream))

        def launch():
            rc = fn(*args)
            if rc != 0:
                check(rc, "tdoa_localize_batch")
            return out

        launch.keep = (frames, out, s, st)
        return launch

    def localize(self, frames: torch.Tensor, scores: bool = False, grid: bool = True,
                 stream=None, ls: bool = False) -> dict:
        out = self.alloc_outputs(self._check_frames(frames), scores=scores, grid=grid, ls=ls)
        return self.localize_into(frames, out, stream)

    def correlate_prepared(self, prepared: torch.Tensor, scores: bool = True,
                           grid: bool = True) -> dict:
        """Frames already DC-removed, normalised and windowed (correlations_init
        inputs).  Runs the reference's integer path (DIRECT) on any context, so
        the int64 outputs are returned whatever the context's engine."""
        B = self._check_frames(prepared)
        out = self.alloc_outputs(B, scores=scores, grid=grid, engine="direct")
        s = self._outputs_struct(out)
        st = torch.cuda.current_stream(self.torch_device)
        check(load().tdoa_correlate_prepared(self._ctx, C.c_void_p(prepared.data_ptr()), B,
                                             C.byref(s), C.c_void_p(st.cuda_stream)),
              "tdoa_correlate_prepared")
        return out

    def average(self, est: torch.Tensor, fresh: torch.Tensor, decay: torch.Tensor,
                best: torch.Tensor, solve: dict | None = None) -> None:
        """EMA of correlations.c:38-63 over S streams, in place on `est`/`best`."""
        S = est.shape[0]
        P, K = self.dims.P, self.dims.K
        assert est.dtype == torch.int64 and tuple(est.shape) == (S, P, K) and est.is_contiguous()
        assert fresh.dtype == torch.int64 and tuple(fresh.shape) == (S, P, K) and fresh.is_contiguous()
        assert decay.dtype == torch.float32 and decay.numel() == S
        assert best.dtype == torch.int32 and tuple(best.shape) == (S, P)
        st = torch.cuda.current_stream(self.torch_device)
        sol = C.byref(self._outputs_struct(solve)) if solve is not None else None
        check(load().tdoa_average_batch(self._ctx, S, _ptr(est), _ptr(fresh), _ptr(decay),
                                        _ptr(best), sol, C.c_void_p(st.cuda_stream)),
              "tdoa_average_batch")

    def heatmap(self, weighted: torch.Tensor, max_L: torch.Tensor) -> torch.Tensor:
        """vga_heatmap.h:110-130 colour classes [B][H][W] (4 white .. 0 black)."""
        B = weighted.shape[0]
        is_float = weighted.dtype == torch.float32
        assert weighted.dtype in (torch.int64, torch.float32) and max_L.dtype == weighted.dtype
        assert tuple(weighted.shape[1:]) == (self.dims.P, self.dims.K) and weighted.is_contiguous()
        H = self.dims.G // self.grid_W
        out = torch.empty((B, H, self.grid_W), dtype=torch.uint8, device=self.torch_device)
        st = torch.cuda.current_stream(self.torch_device)
        check(load().tdoa_heatmap(self._ctx, _ptr(weighted), _ptr(max_L), int(is_float), B,
                                  _ptr(out), C.c_void_p(st.cuda_stream)), "tdoa_heatmap")
        return out

    def peaks(self, scores: torch.Tensor, num_peaks: int = 2, radius: int = 8,
              min_rel: float = 0.0, ls: bool = False, stream=None) -> dict:
        """Up to `num_peaks` maxima of L = sum_p scores_p[LUT_p] per frame, a
        square of `radius` cells suppressed around each (tdoa_peaks).

        scores: [B][P][K] int64 or float32 on the context's GPU -- raw scores
        (`scores` / `scores_f`) to find several simultaneous sources, weighted
        scores for the map the reference displays, or EMA scores.  Returns
        count [B], cell [B][Kp] (-1 in empty slots), xy [B][Kp][2], L (int64)
        or Lf (float32) [B][Kp], lags [B][Kp][P] and, with ls, xy_ls / ls_rms.
        Asynchronous on `stream` (default: the current stream)."""
        P, K, dev = self.dims.P, self.dims.K, self.torch_device
        if scores.dtype not in (torch.int64, torch.float32):
            raise ValueError(f"scores must be int64 or float32, got {scores.dtype}")
        if scores.dim() != 3 or tuple(scores.shape[1:]) != (P, K):
            raise ValueError(f"scores must be [B][{P}][{K}], got {tuple(scores.shape)}")
        if scores.device != dev:
            raise ValueError(f"scores must live on {dev}")
        if not scores.is_contiguous():
            raise ValueError("scores must be contiguous")
        B, Kp = scores.shape[0], int(num_peaks)
        is_float = scores.dtype == torch.float32
        st = stream if stream is not None else torch.cuda.current_stream(dev)
        n = max(Kp, 0)
        with torch.cuda.stream(st):
            o = {"count": torch.empty(B, dtype=torch.int32, device=dev),
                 "cell": torch.empty((B, n), dtype=torch.int32, device=dev),
                 "xy": torch.empty((B, n, 2), dtype=torch.float32, device=dev),
                 "Lf" if is_float else "L": torch.empty((B, n), dtype=scores.dtype, device=dev),
                 "lags": torch.empty((B, n, P), dtype=torch.int32, device=dev)}
            if ls:
                o["xy_ls"] = torch.empty((B, n, 2), dtype=torch.float32, device=dev)
                o["ls_rms"] = torch.empty((B, n), dtype=torch.float32, device=dev)
        if B == 0:  # nothing to launch (and empty tensors have no address to pass)
            return o
        prm = PeaksParams(Kp, int(radius), float(min_rel))
        s = PeaksOutputs()
        for name, _ in PeaksOutputs._fields_:
            t = o.get(name)
            setattr(s, name, None if t is None else t.data_ptr())
        check(load().tdoa_peaks(self._ctx, _ptr(scores), int(is_float), B, C.byref(prm),
                                C.byref(s), C.c_void_p(st.cuda_stream)), "tdoa_peaks")
        return o

    def track_batch(self, tracks: torch.Tensor, next_id: torch.Tensor, t_us: torch.Tensor, count: torch.Tensor,
                    xy: torch.Tensor, stream_of_row: torch.Tensor | None = None, outputs=None, stream=None,
                    **params) -> dict:
        """One tracker update of caller-owned state from a block of measurements
        (tdoa_track_batch, kernel k_track; the rule is in include/tdoa.h,
        "Tracking").

        tracks: uint8 [S][8][64] (tdoa_track records, all zero at start; view
        its host copy with TRACK_DTYPE) and next_id: int32 [S], updated in
        place.  Row i is stream stream_of_row[i] (int32 [rows]; None: stream
        i) at time t_us[i] (int64, microseconds) with count[i] (int32)
        measurements xy[i, :count[i]] (float32 [rows][Kp][2], metres, e.g. a
        peaks() call's xy or xy_ls).  params: the tdoa_track_params fields
        (_lib.TRACK_DEFAULTS).  outputs: a dict of tensors to write (tracks
        uint8 [rows][T][64], assigned int32 [rows][Kp], num_confirmed int32
        [rows]; a missing key is not written) -- fresh ones by default.
        Asynchronous on `stream` (default: the current stream)."""
        dev = self.torch_device
        prm = track_params(**params)
        S = tracks.shape[0] if tracks.dim() else 0
        if tracks.dtype != torch.uint8 or tuple(tracks.shape) != (S, _lib.MAX_TRACKS, 64):
            raise ValueError(f"tracks must be uint8 [S][{_lib.MAX_TRACKS}][64]")
        if next_id.dtype != torch.int32 or tuple(next_id.shape) != (S,):
            raise ValueError("next_id must be int32 [S]")
        if xy.dtype != torch.float32 or xy.dim() != 3 or xy.shape[2] != 2:
            raise ValueError("xy must be float32 [rows][Kp][2]")
        rows, Kp = xy.shape[0], xy.shape[1]
        if t_us.dtype != torch.int64 or tuple(t_us.shape) != (rows,):
            raise ValueError("t_us must be int64 [rows]")
        if count.dtype != torch.int32 or tuple(count.shape) != (rows,):
            raise ValueError("count must be int32 [rows]")
        if stream_of_row is None:
            if rows > S:
                raise ValueError("more rows than streams")
        elif stream_of_row.dtype != torch.int32 or tuple(stream_of_row.shape) != (rows,):
            raise ValueError("stream_of_row must be int32 [rows]")
        T = min(max(prm.max_tracks, 1), _lib.MAX_TRACKS)
        st = stream if stream is not None else torch.cuda.current_stream(dev)
        if outputs is None:
            with torch.cuda.stream(st):
                outputs = {"tracks": torch.empty((rows, T, 64), dtype=torch.uint8, device=dev),
                           "assigned": torch.empty((rows, Kp), dtype=torch.int32, device=dev),
                           "num_confirmed": torch.empty(rows, dtype=torch.int32, device=dev)}
        want = {"tracks": (torch.uint8, (rows, T, 64)), "assigned": (torch.int32, (rows, Kp)),
                "num_confirmed": (torch.int32, (rows,))}
        for name, t in outputs.items():
            if name not in want or t.dtype != want[name][0] or tuple(t.shape) != want[name][1]:
                raise ValueError(f"outputs[{name!r}] must be {want.get(name)}")
        for t in (tracks, next_id, t_us, count, xy, stream_of_row, *outputs.values()):
            if t is not None and (t.device != dev or not t.is_contiguous()):
                raise ValueError(f"every tensor must be contiguous on {dev}")
        if rows == 0:  # nothing to launch (and empty tensors have no address to pass)
            return outputs
        o = TrackOutputs(*[None if outputs.get(n) is None else outputs[n].data_ptr() for n, _ in TrackOutputs._fields_])
        check(load().tdoa_track_batch(self.device, _ptr(tracks), _ptr(next_id), rows, _ptr(stream_of_row), _ptr(t_us),
                                      _ptr(count), _ptr(xy), Kp, C.byref(prm), C.byref(o),
                                      C.c_void_p(st.cuda_stream)), "tdoa_track_batch")
        return outputs

    def _steered_batch(self, frames, N, xy, count, outputs, stream, name: str, call) -> dict:
        """What beam_batch() and sep_batch() share: frames int16 [B][M][N] (N an
        int, or None: any length), xy, count and the outputs validated, the
        outputs made where none were given, then -- B > 0 -- call(Kt,
        BeamOutputs pointer, stream pointer) -> the library's return code."""
        dev = self.torch_device
        M = self.dims.M
        if frames.dtype != torch.int16 or frames.dim() != 3 or tuple(frames.shape[1:]) != (M, N or frames.shape[2]):
            raise ValueError(f"frames must be int16 [B][{M}][{N or 'L'}]")
        B, N = frames.shape[0], frames.shape[2]
        if xy.dtype != torch.float32 or xy.dim() != 3 or xy.shape[0] != B or xy.shape[2] != 2:
            raise ValueError("xy must be float32 [B][Kt][2]")
        Kt = xy.shape[1]
        if count is not None and (count.dtype != torch.int32 or tuple(count.shape) != (B,)):
            raise ValueError("count must be int32 [B]")
        st = stream if stream is not None else torch.cuda.current_stream(dev)
        want = {"audio": (torch.float32, (B, Kt, N)), "delays": (torch.int32, (B, Kt, M)),
                "active": (torch.uint8, (B, Kt))}
        if outputs is None:
            with torch.cuda.stream(st):
                outputs = {k: torch.empty(shp, dtype=dt, device=dev) for k, (dt, shp) in want.items()}
        if "audio" not in outputs:
            raise ValueError("outputs[\"audio\"] is required")
        for name, t in outputs.items():
            if name not in want or t.dtype != want[name][0] or tuple(t.shape) != want[name][1]:
                raise ValueError(f"outputs[{name!r}] must be {want.get(name)}")
        for t in (frames, xy, count, *outputs.values()):
            if t is not None and (t.device != dev or not t.is_contiguous()):
                raise ValueError(f"every tensor must be contiguous on {dev}")
        if B == 0:  # nothing to launch (and empty tensors have no address to pass)
            return outputs
        o = BeamOutputs(*[None if outputs.get(n) is None else outputs[n].data_ptr() for n, _ in BeamOutputs._fields_])
        check(call(Kt, C.byref(o), C.c_void_p(st.cuda_stream)), name)
        return outputs

    def beam_batch(self, frames: torch.Tensor, xy: torch.Tensor, count: torch.Tensor | None = None,
                   outputs=None, stream=None) -> dict:
        """Beamformed audio of up to 8 targets per frame (tdoa_beam_batch, kernel
        k_beam; the rule is in include/tdoa.h, "Listening").

        frames: int16 [B][M][N] as localize() takes them; xy: float32
        [B][Kt][2] plane coordinates (a localize() xy / xy_ls, a peaks() row);
        count: int32 [B], target k of frame b valid for k < count[b] (None: all
        Kt) and finite coordinates.  outputs: a dict of tensors to write (audio
        float32 [B][Kt][N], required; delays int32 [B][Kt][M]; active uint8
        [B][Kt]) -- fresh ones by default.  Asynchronous on `stream` (default:
        the current stream)."""
        return self._steered_batch(frames, self.dims.N, xy, count, outputs, stream, "tdoa_beam_batch",
                                   lambda Kt, out, st: load().tdoa_beam_batch(
                                       self._ctx, _ptr(frames), frames.shape[0], _ptr(count),
                                       _ptr(xy) if xy.numel() else None, Kt, out, st))

    def sep_batch(self, frames: torch.Tensor, xy: torch.Tensor, count: torch.Tensor | None = None,
                  loading: float = _lib.SEP_LOADING, outputs=None, stream=None) -> dict:
        """One null-steered STFT block per frame and target (tdoa_sep_batch,
        kernel k_sep; the rule is in include/tdoa.h, "Separating"): channel k
        has unit gain on target k and nulls on the frame's other valid targets.

        frames: int16 [B][M][L], L a power of two in 128..2048 with L >= 8 Dmax
        -- frame_len or any other block length: a call whose L differs from the
        context's (sep_block()) sets it first (tdoa_sep_set_block: an upload and
        a device synchronisation, once per change); xy: float32 [B][Kt][2]
        plane coordinates, Kt <= 4; count:
        int32 [B] (None: all Kt); loading: the diagonal loading delta in
        [1e-4, 1e4].  outputs: a dict of tensors to write (audio float32
        [B][Kt][L], required -- the synthesis-windowed block, to be
        overlap-added with its half-overlapped neighbours; delays int32
        [B][Kt][M]; active uint8 [B][Kt]) -- fresh ones by default.
        Asynchronous on `stream` (default: the current stream)."""
        def call(Kt, out, st):
            if frames.shape[2] != self.sep_block():
                check(load().tdoa_sep_set_block(self._ctx, frames.shape[2]), "tdoa_sep_set_block")
            return load().tdoa_sep_batch(self._ctx, _ptr(frames), frames.shape[0], _ptr(count),
                                         _ptr(xy) if xy.numel() else None, Kt, float(loading), out, st)
        return self._steered_batch(frames, None, xy, count, outputs, stream, "tdoa_sep_batch", call)

    def sep_block(self) -> int:
        """The block length sep_batch() runs at (tdoa_sep_get_block; 0: none yet)."""
        n = C.c_int32()
        check(load().tdoa_sep_get_block(self._ctx, C.byref(n)), "tdoa_sep_get_block")
        return n.value

    def beam_geometry(self) -> BeamGeometry:
        """What steering reads of this context (tdoa_get_beam_geometry)."""
        g = BeamGeometry()
        check(load().tdoa_get_beam_geometry(self._ctx, C.byref(g)), "tdoa_get_beam_geometry")
        return g

    def beam_latency(self):
        """(A, Dmax) in samples (tdoa_beam_latency): the beam's output sample n
        needs the input up to n + A; no delay code exceeds 32 Dmax."""
        a, d = C.c_int32(), C.c_int32()
        check(load().tdoa_beam_latency(self._ctx, C.byref(a), C.byref(d)), "tdoa_beam_latency")
        return a.value, d.value

    def cell_xy(self, cell: np.ndarray) -> np.ndarray:
        """((x - half_w)/scale, (half_h - y)/scale) of row-major cells, float32 as on device."""
        cell = np.asarray(cell)
        x = (cell % self.grid_W - self.grid_half_w).astype(np.float32)
        y = (self.grid_half_h - cell // self.grid_W).astype(np.float32)
        return np.stack([x / np.float32(self.grid_scale), y / np.float32(self.grid_scale)], -1)
