"""Streaming pipeline: the Python face of tdoa_stream_* (include/tdoa.h).

The batched form of the reference's sample loop (sample_compute.h:53-146)
for S independent streams: every `step()` consumes one hop of H samples per
stream from a device capture ring of 8-bit ADC bytes [S][capture_len][M]
(dma_sampler.c:17-23), runs the trigger scan, the DIRECT path on the
triggered frames, the EMA (correlations.c:38-63) and the grid solve on the
EMA scores -- all libtdoa kernels, launched on the pipeline's stream (or, with
use_graph, replayed as one hipGraph per step).

A `gcc_phat` Localizer streams the GCC-PHAT engine instead (k_stream_phat):
float scores under the localizer's weight table (set_band / set_bin_weights,
read at every step), a float32 EMA, `out["max_Lf"]` in place of
`out["max_L"]` and float32 `est` from state().

A `gcc_phat` Localizer whose sample_format is "pcm16" streams an int16 capture
ring [S][capture_len][M] (tdoa_stream_create_pcm16: k_stream_trigger16, then
k_stream_phat_pcm16): the trigger of include/tdoa.h on int16 samples with the
threshold `trigger_var` (counts^2, default 131072 = 2 * 256^2, the 8-bit
trigger for samples scaled by 256).  The pipeline keeps the format it was
created in.

peaks() / peak_records() report, per hop and without a host synchronisation,
up to `num_peaks` maxima of the EMA map of every frame the step listed
(tdoa_stream_peaks: k_stream_peaks, with ls the per-peak least-squares
refinement k_ls_stream); peaks_all() runs tdoa_peaks over the whole device
state, est_ptr() hands that state out as a device address.

mode="continuous" (a `gcc_phat` Localizer; tdoa_stream_create_continuous:
k_stream_active in place of a trigger) chooses frames for continuous audio
instead of clicks.  The ring is uint8 or int16 according to loc.sample_format.
With pos the samples consumed before the hop there is one candidate per stream
and hop, e = pos + hop, eligible iff e >= N; its frame is F = [e - N, e);
pw(m) = N * sum_F x_m^2 - (sum_F x_m)^2 on the ring's own sample values, exact
in int64; the stream is listed iff sum_m pw(m) >= activity_var * N^2.  The
comparison is >=, so activity_var = 0 (the default) lists every eligible
stream; activity_var is in counts^2 summed over mics, in [0, 2^30].  Listed
frames go through what triggered frames do, the gate sum lag^2 > 4 included.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from ._lib import (STREAM_TRIGGER_VAR_PCM16, PeaksOutputs, PeaksParams, StreamOutputs, StreamOutputsF, check,
                   load)
from .localizer import Localizer


class StreamPipeline:
    # use_graph: each hop replayed as a captured hipGraph of its two kernels.
    # Plain stream launches are the default: 67.0 vs 71.8 us per config-5 hop
    # (tools/diag_stream_launch.py, same box; the graph's launch adds ~5 us)
    def __init__(self, loc: Localizer, capture: torch.Tensor, hop: int = 512,
                 use_graph: bool = False, trigger_var: int | None = None, mode: str = "triggered",
                 activity_var: int | None = None):
        if loc.engine not in ("direct", "gcc_phat"):
            raise ValueError("the streaming pipeline runs the DIRECT or the GCC_PHAT engine")
        if mode not in ("triggered", "continuous"):
            raise ValueError(f"mode must be \"triggered\" or \"continuous\", not {mode!r}")
        self.mode = mode
        self.activity_var = None
        self.phat = loc.engine == "gcc_phat"
        if mode == "continuous":
            if not self.phat:
                raise ValueError("continuous mode needs a gcc_phat localizer (DIRECT reproduces the firmware)")
            if trigger_var is not None:
                raise ValueError("trigger_var applies to triggered mode; continuous mode takes activity_var")
            want = torch.int16 if loc.sample_format == "pcm16" else torch.uint8
            if capture.dtype != want:
                raise ValueError(f"continuous mode on a {loc.sample_format} localizer takes a {want} capture")
        elif activity_var is not None:
            raise ValueError("activity_var applies to mode=\"continuous\"")
        # an int16 ring on a PCM16 localizer; a uint8 ring goes to tdoa_stream_create
        # whatever the format (the library rejects it on a PCM16 context)
        self.pcm16 = capture.dtype == torch.int16
        if self.pcm16 and loc.sample_format != "pcm16":
            raise ValueError("an int16 capture needs a localizer whose sample_format is \"pcm16\"")
        if not self.pcm16 and trigger_var is not None:
            raise ValueError("trigger_var applies to an int16 capture (the 8-bit trigger's threshold is fixed)")
        if capture.dtype not in (torch.uint8, torch.int16) or capture.dim() != 3 or capture.shape[2] != loc.dims.M:
            raise ValueError(f"capture must be uint8 (or, in pcm16 format, int16) [S][T][{loc.dims.M}]")
        if capture.device != loc.torch_device or not capture.is_contiguous():
            raise ValueError("capture must be contiguous on the localizer's device")
        self.loc, self.capture, self.hop = loc, capture, hop
        self.S, self.capture_len = capture.shape[0], capture.shape[1]
        P = loc.dims.P
        dev = loc.torch_device
        S = self.S
        self.out = {
            "count": torch.zeros(1, dtype=torch.int32, device=dev),
            "stream_id": torch.zeros(S, dtype=torch.int32, device=dev),
            "end": torch.zeros(S, dtype=torch.int64, device=dev),
            "lags": torch.zeros((S, P), dtype=torch.int32, device=dev),
            "gate": torch.zeros(S, dtype=torch.uint8, device=dev),
            "ema_best": torch.zeros((S, P), dtype=torch.int32, device=dev),
            "cell": torch.zeros(S, dtype=torch.int32, device=dev),
            "xy": torch.zeros((S, 2), dtype=torch.float32, device=dev),
        }
        if self.phat:
            self.out["max_Lf"] = torch.zeros(S, dtype=torch.float32, device=dev)
        else:
            self.out["max_L"] = torch.zeros(S, dtype=torch.int64, device=dev)
        struct = StreamOutputsF if self.phat else StreamOutputs
        self._s = struct(*[self.out[n].data_ptr() for n, _ in struct._fields_])
        # graph capture needs a real (non-default) stream
        self.stream = torch.cuda.Stream(device=dev)
        h = C.c_void_p()
        if mode == "continuous":
            self.activity_var = 0 if activity_var is None else int(activity_var)
            if not -2 ** 63 <= self.activity_var < 2 ** 63:
                raise ValueError("activity_var does not fit int64")
            check(load().tdoa_stream_create_continuous(loc._ctx, S, hop, C.c_void_p(capture.data_ptr()),
                                                       self.capture_len, self.activity_var, int(use_graph),
                                                       C.byref(h)), "tdoa_stream_create_continuous")
        elif self.pcm16:
            self.trigger_var = STREAM_TRIGGER_VAR_PCM16 if trigger_var is None else int(trigger_var)
            if not -2 ** 63 <= self.trigger_var < 2 ** 63:
                raise ValueError("trigger_var does not fit int64")
            check(load().tdoa_stream_create_pcm16(loc._ctx, S, hop, C.c_void_p(capture.data_ptr()),
                                                  self.capture_len, self.trigger_var, int(use_graph),
                                                  C.byref(h)), "tdoa_stream_create_pcm16")
        else:
            check(load().tdoa_stream_create(loc._ctx, S, hop, C.c_void_p(capture.data_ptr()),
                                            self.capture_len, int(use_graph), C.byref(h)),
                  "tdoa_stream_create")
        self._h = h
        self._peaks = {}  # (Kp, ls) -> the output tensors of peaks()
        self._peaks_last = None

    def step(self) -> dict:
        """One hop for every stream (asynchronous on self.stream)."""
        step = load().tdoa_stream_step_f if self.phat else load().tdoa_stream_step
        check(step(self._h, C.byref(self._s), C.c_void_p(self.stream.cuda_stream)), "tdoa_stream_step")
        return self.out

    def records(self) -> dict:
        """Synchronously fetch this step's triggered slots, sorted by stream."""
        self.stream.synchronize()
        n = int(self.out["count"].item())
        r = {k: v[:n].cpu().numpy() for k, v in self.out.items() if k != "count"}
        order = np.argsort(r["stream_id"], kind="stable")
        return {k: v[order] for k, v in r.items()}

    def peaks(self, num_peaks: int = 2, radius: int = 8, min_rel: float = 0.0, ls: bool = False,
              gated_only: bool = True) -> dict:
        """Up to `num_peaks` maxima of the EMA map of every frame the last step
        listed (tdoa_stream_peaks), asynchronous on self.stream: call it after
        step() and before the next one.

        Returns device tensors indexed by the step's slots, rows < out["count"]
        written: count [S], cell [S][Kp] (-1 in empty slots), xy [S][Kp][2], L
        (DIRECT, int64) or Lf (GCC_PHAT, float32) [S][Kp], lags [S][Kp][P] and,
        with ls, xy_ls [S][Kp][2] / ls_rms [S][Kp].  They are allocated once per
        (num_peaks, ls) and reused by later calls.  gated_only: slots whose frame
        did not pass the gate (out["gate"] == 0) get the empty record; otherwise
        every listed slot's map is searched, as its last gated frame left it."""
        Kp, ls = int(num_peaks), bool(ls)
        o = self._peaks.get((Kp, ls))
        if o is None:
            S, n, P, dev = self.S, max(Kp, 0), self.loc.dims.P, self.loc.torch_device
            o = {"count": torch.zeros(S, dtype=torch.int32, device=dev),
                 "cell": torch.zeros((S, n), dtype=torch.int32, device=dev),
                 "xy": torch.zeros((S, n, 2), dtype=torch.float32, device=dev),
                 "Lf" if self.phat else "L": torch.zeros((S, n), dtype=torch.float32 if self.phat else torch.int64,
                                                         device=dev),
                 "lags": torch.zeros((S, n, P), dtype=torch.int32, device=dev)}
            if ls:
                o["xy_ls"] = torch.zeros((S, n, 2), dtype=torch.float32, device=dev)
                o["ls_rms"] = torch.zeros((S, n), dtype=torch.float32, device=dev)
            # the allocator's fills ran on the current stream: they precede the kernels on self.stream
            self.stream.wait_stream(torch.cuda.current_stream(dev))
        prm = PeaksParams(Kp, int(radius), float(min_rel))
        s = PeaksOutputs()
        for name, _ in PeaksOutputs._fields_:
            t = o.get(name)
            setattr(s, name, t.data_ptr() if t is not None and t.numel() else None)
        gate = C.c_void_p(self.out["gate"].data_ptr()) if gated_only else None
        check(load().tdoa_stream_peaks(self._h, C.byref(prm), gate, C.byref(s), C.c_void_p(self.stream.cuda_stream)),
              "tdoa_stream_peaks")
        self._peaks[(Kp, ls)] = o  # kept only once the library accepted the arguments
        self._peaks_last = o
        return o

    def peak_records(self) -> dict:
        """Synchronously fetch the last peaks() call's rows of this step's slots,
        sorted by stream, with the slots' stream_id attached."""
        if self._peaks_last is None:
            raise RuntimeError("peak_records() reads the result of a peaks() call")
        self.stream.synchronize()
        n = int(self.out["count"].item())
        r = {k: v[:n].cpu().numpy() for k, v in self._peaks_last.items()}
        r["stream_id"] = self.out["stream_id"][:n].cpu().numpy()
        order = np.argsort(r["stream_id"], kind="stable")
        return {k: v[order] for k, v in r.items()}

    def est_ptr(self):
        """(device address, is_float) of the EMA state: int64 [S][P][K] (DIRECT)
        or float32 [S][P][K] (GCC_PHAT); valid until close().  Calls that read
        it are stream-ordered with the steps (tdoa_stream_est_device)."""
        ptr, flt = C.c_void_p(), C.c_int()
        check(load().tdoa_stream_est_device(self._h, C.byref(ptr), C.byref(flt)), "tdoa_stream_est_device")
        return int(ptr.value), bool(flt.value)

    def peaks_all(self, num_peaks: int = 2, radius: int = 8, min_rel: float = 0.0, ls: bool = False) -> dict:
        """tdoa_peaks over the whole device state, one row per stream (B = S),
        listed or not, asynchronous on self.stream; fresh tensors as
        Localizer.peaks returns them."""
        S, Kp, P, dev = self.S, int(num_peaks), self.loc.dims.P, self.loc.torch_device
        n = max(Kp, 0)
        with torch.cuda.stream(self.stream):
            o = {"count": torch.empty(S, dtype=torch.int32, device=dev),
                 "cell": torch.empty((S, n), dtype=torch.int32, device=dev),
                 "xy": torch.empty((S, n, 2), dtype=torch.float32, device=dev),
                 "Lf" if self.phat else "L": torch.empty((S, n), dtype=torch.float32 if self.phat else torch.int64,
                                                         device=dev),
                 "lags": torch.empty((S, n, P), dtype=torch.int32, device=dev)}
            if ls:
                o["xy_ls"] = torch.empty((S, n, 2), dtype=torch.float32, device=dev)
                o["ls_rms"] = torch.empty((S, n), dtype=torch.float32, device=dev)
        ptr, flt = self.est_ptr()
        prm = PeaksParams(Kp, int(radius), float(min_rel))
        s = PeaksOutputs()
        for name, _ in PeaksOutputs._fields_:
            t = o.get(name)
            setattr(s, name, t.data_ptr() if t is not None and t.numel() else None)
        check(load().tdoa_peaks(self.loc._ctx, C.c_void_p(ptr), int(flt), S, C.byref(prm), C.byref(s),
                                C.c_void_p(self.stream.cuda_stream)), "tdoa_peaks")
        return o

    def reset(self) -> None:
        check(load().tdoa_stream_reset(self._h, C.c_void_p(self.stream.cuda_stream)),
              "tdoa_stream_reset")

    def state(self):
        P, K = self.loc.dims.P, self.loc.dims.K
        pos = np.zeros(1, np.int64)
        est = np.zeros((self.S, P, K), np.float32 if self.phat else np.int64)
        last = np.zeros(self.S, np.uint64)
        state = load().tdoa_stream_state_f if self.phat else load().tdoa_stream_state
        check(state(self._h, pos.ctypes.data_as(C.c_void_p), est.ctypes.data_as(C.c_void_p),
                    last.ctypes.data_as(C.c_void_p), None), "tdoa_stream_state")
        return int(pos[0]), est, last

    def totals(self):
        """(samples consumed per stream, triggered frames, gated frames) so far."""
        pos = np.zeros(1, np.int64)
        st = np.zeros(2, np.int64)
        check(load().tdoa_stream_state(self._h, pos.ctypes.data_as(C.c_void_p), None, None,
                                       st.ctypes.data_as(C.c_void_p)), "tdoa_stream_state")
        return int(pos[0]), int(st[0]), int(st[1])

    def close(self) -> None:
        if getattr(self, "_h", None):
            load().tdoa_stream_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
