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

The shapes k_stream_phat's LDS cannot hold but the batch engine's long-frame
kernel can -- 8 mics x 2048 and 4 mics x 4096 -- stream through k_f16_ring
(that kernel's body over the step's listed frames, staged from the rings) and
k_stream_ema_grid, in every mode and ring format below; `kernel` names the
route.  Records, state, peaks() and track() are the same.

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

track() / track_records() / tracks_all() follow sources across hops
(tdoa_stream_track: k_track).  Per hop the order is step -> peaks -> track.
Each stream owns a table of 8 track records (TRACK_DTYPE: id, status, hits,
misses, x, y, vx, vy, p00, p01, p11, peak, t_us, upd_us), all zero at start,
and a counter next_id, 0 at start (the first id is 1).  A listed slot is a row:
its stream s, its time t = end * 1e6 / fs (int64 us, the EMA's clock), n = its
peak count clamped to [0, Kp], measurements z_k = (zx, zy), k < n.  With
T = max_tracks, r = meas_var, q = accel_psd, all float arithmetic fp32 with
every operation rounded on its own and IEEE division, in exactly this order:
  0. n <= 0: the row is not evaluated (state untouched: no miss is counted, no
     time advances; the outputs are the unchanged table, assigned all 0).  A
     measurement with a non-finite coordinate is invalid: neither associated
     nor born.
  1. coast-out: each live slot j < T, in slot order, with
     t - upd_us > max_coast_us is zeroed (freed).
  2. predict every live track: dt = (float)max(t - t_us, 0) / 1e6f;
     x = x + vx*dt; y = y + vy*dt; a = dt*p11; c = (p01 + p01) + a; d = dt*c;
     dt2 = dt*dt; dt3 = dt2*dt; p00 = (p00 + d) + (q*dt3)/3.0f;
     p01 = (p01 + a) + (q*dt2)*0.5f; p11 = p11 + q*dt; t_us = t.
  3. cost for live j, valid k: dx = zx - x; dy = zy - y; s = p00 + r;
     c_jk = (dx*dx + dy*dy) / s; eligible iff c_jk <= gate_d2 (NaN: false).
  4. greedy association: the eligible pair of minimum c_jk among tracks and
     measurements both unassigned, ties to the lowest j, then the lowest k;
     repeat until no eligible pair remains.
  5. assigned track, from the old values: k0 = p00/s; k1 = p01/s;
     x = x + k0*dx; y = y + k0*dy; vx = vx + k1*dx; vy = vy + k1*dy;
     p11 = p11 - k1*p01; p01 = p01 - k0*p01; p00 = p00 - k0*p00; hits += 1;
     misses = 0; upd_us = t; peak = k; status 1 with hits >= confirm_hits
     becomes 2.
  6. unassigned live track: misses += 1; peak = -1; freed when
     misses >= max_misses.
  7. births: each unassigned valid measurement, ascending k, takes the lowest
     free slot < T (slots freed in 1 and 6 count) or is dropped:
     id = ++next_id[s], status = confirm_hits <= 1 ? 2 : 1, hits = 1,
     misses = 0, (x, y) = z, vx = vy = 0, p00 = r, p01 = 0,
     p11 = init_vel_var, t_us = upd_us = t, peak = k.
With gated_only=False peaks, a stream never updated reports cell 0 with L = 0
and a track is born there: track gated peaks (the default) or use min_rel.

beam() listens to the sources (tdoa_stream_beam: k_beam_ring; the rule is in
include/tdoa.h, "Listening"): per hop and stream one block of delay-and-sum
audio per target -- the track table's slots (step -> peaks -> track -> beam) or
explicit plane coordinates -- read from the capture rings behind the device
clock, for every stream whether the step listed it or not, A = Dmax + 8
samples behind the clock (Localizer.beam_latency()); consecutive blocks abut.

sep() separates them (tdoa_stream_sep: k_sep; include/tdoa.h, "Separating"):
the same targets, at most 4, but channel k nulls the stream's other valid
targets -- a frequency-domain, diagonally loaded null-steering beamformer over
half-overlapped blocks of L = 2 hop samples, overlap-added on the device; its
audio runs L samples behind the clock.  It needs L >= 8 Dmax.

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

from ._lib import (BEAM_MAX_TARGETS, MAX_TRACKS, SEP_LOADING, SEP_MAX_TARGETS, STREAM_TRIGGER_VAR_PCM16, TRACK_FIELDS,
                   BeamOutputs, PeaksOutputs, PeaksParams, StreamOutputs, StreamOutputsF, TrackOutputs, check, load, track_params)
from .localizer import Localizer, _ptr


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
        self._tracks = {}  # (T, Kp) -> the output tensors of track()
        self._tracks_last = None
        self._beams = {}  # Kt -> the output tensors of beam()
        self._seps = {}  # Kt -> the output tensors of sep()

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

    def track(self, peaks: dict | None = None, use_ls: bool | None = None, **params) -> dict:
        """One tracker update per listed stream from a peaks() result
        (tdoa_stream_track, kernel k_track), asynchronous on self.stream: call
        it after step() and peaks(), before the next step().

        peaks: a dict with count [S] int32 and xy / xy_ls [S][Kp][2] float32 as
        peaks() returns them (default: the last peaks() result; any tensors of
        that layout do, the call does not depend on peaks()).  use_ls: take
        xy_ls (None: when the result has it).  params: the tdoa_track_params
        fields (_lib.TRACK_DEFAULTS).  Returns device tensors indexed by the
        step's slots, rows < out["count"] written: tracks uint8 [S][T][64] (a
        stream's slots 0..T-1 after the update; track_records() views them as
        TRACK_DTYPE), assigned int32 [S][Kp] (the track id each peak went to or
        was born as, 0 otherwise) and num_confirmed int32 [S].  They are
        allocated once per (T, Kp) and reused by later calls."""
        pk = self._peaks_last if peaks is None else peaks
        if pk is None:
            raise RuntimeError("track() reads the result of a peaks() call (or takes one as `peaks`)")
        ls = ("xy_ls" in pk) if use_ls is None else bool(use_ls)
        xy, count = pk["xy_ls" if ls else "xy"], pk["count"]
        dev = self.loc.torch_device
        if xy.dtype != torch.float32 or xy.dim() != 3 or xy.shape[0] != self.S or xy.shape[2] != 2:
            raise ValueError("the measurements must be float32 [S][Kp][2]")
        if count.dtype != torch.int32 or tuple(count.shape) != (self.S,):
            raise ValueError("count must be int32 [S]")
        if xy.device != dev or count.device != dev or not xy.is_contiguous() or not count.is_contiguous():
            raise ValueError("count and the measurements must be contiguous on the localizer's device")
        prm = track_params(**params)
        Kp, T = xy.shape[1], min(max(prm.max_tracks, 1), MAX_TRACKS)
        o = self._tracks.get((T, Kp))
        if o is None:
            S = self.S
            o = {"tracks": torch.zeros((S, T, 64), dtype=torch.uint8, device=dev),
                 "assigned": torch.zeros((S, max(Kp, 0)), dtype=torch.int32, device=dev),
                 "num_confirmed": torch.zeros(S, dtype=torch.int32, device=dev)}
            # the allocator's fills ran on the current stream: they precede the kernel on self.stream
            self.stream.wait_stream(torch.cuda.current_stream(dev))
        s = TrackOutputs(*[o[n].data_ptr() if o[n].numel() else None for n, _ in TrackOutputs._fields_])
        check(load().tdoa_stream_track(self._h, C.byref(prm), C.c_void_p(count.data_ptr()),
                                       C.c_void_p(xy.data_ptr()) if xy.numel() else None, Kp, C.byref(s),
                                       C.c_void_p(self.stream.cuda_stream)), "tdoa_stream_track")
        self._tracks[(T, Kp)] = o  # kept only once the library accepted the arguments
        self._tracks_last = o
        return o

    def track_records(self) -> dict:
        """Synchronously fetch the last track() call's rows of this step's slots,
        sorted by stream, with the slots' stream_id attached; tracks is a
        structured array [n][T] of TRACK_DTYPE."""
        if self._tracks_last is None:
            raise RuntimeError("track_records() reads the result of a track() call")
        self.stream.synchronize()
        n = int(self.out["count"].item())
        r = {k: v[:n].cpu().numpy() for k, v in self._tracks_last.items()}
        r["tracks"] = np.ascontiguousarray(r["tracks"]).view(np.dtype(TRACK_FIELDS))[..., 0]
        r["stream_id"] = self.out["stream_id"][:n].cpu().numpy()
        order = np.argsort(r["stream_id"], kind="stable")
        return {k: v[order] for k, v in r.items()}

    def tracks_all(self):
        """Host snapshot of the whole track state, listed or not (synchronises):
        (tracks [S][8] of TRACK_DTYPE, next_id [S] int32); all zero before the
        first track() call (tdoa_stream_tracks_device)."""
        tr, nid = C.c_void_p(), C.c_void_p()
        check(load().tdoa_stream_tracks_device(self._h, C.byref(tr), C.byref(nid)), "tdoa_stream_tracks_device")
        tracks = np.zeros((self.S, MAX_TRACKS), np.dtype(TRACK_FIELDS))
        next_id = np.zeros(self.S, np.int32)
        if tr.value:
            self.stream.synchronize()
            hip = load()  # the HIP runtime's symbols resolve through libtdoa.so, which is linked to it
            hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            for dst, src in ((tracks, tr.value), (next_id, nid.value)):
                rc = hip.hipMemcpy(dst.ctypes.data_as(C.c_void_p), C.c_void_p(src), dst.nbytes, 2)  # device to host
                if rc != 0:
                    raise RuntimeError(f"copying the track state failed: hipError {rc}")
        return tracks, next_id

    @property
    def kernel(self) -> str:
        """Name of the kernel that computes the hop's scores (tdoa_stream_kernel):
        k_stream_phat / k_stream_phat_pcm16, k_f16_ring for the long-frame
        shapes (8 mics x 2048, 4 x 4096), k_direct_mfma / k_direct."""
        return (load().tdoa_stream_kernel(self._h) or b"").decode()

    def _target_count(self, xy, count, num_targets, default: int) -> int:
        """Kt of a beam() / sep() call, its xy / count / num_targets validated."""
        if xy is None:
            if count is not None:
                raise ValueError("count goes with xy; the track table's targets are chosen by min_status")
            return default if num_targets is None else int(num_targets)
        if xy.dtype != torch.float32 or xy.dim() != 3 or xy.shape[0] != self.S or xy.shape[2] != 2:
            raise ValueError("xy must be float32 [S][Kt][2]")
        if num_targets is not None and int(num_targets) != xy.shape[1]:
            raise ValueError("num_targets differs from xy's Kt")
        if count is not None and (count.dtype != torch.int32 or tuple(count.shape) != (self.S,)):
            raise ValueError("count must be int32 [S]")
        for t in (xy, count):
            if t is not None and (t.device != self.loc.torch_device or not t.is_contiguous()):
                raise ValueError("xy and count must be contiguous on the localizer's device")
        return xy.shape[1]

    def _steered(self, cache: dict, Kt: int, name: str, call) -> dict:
        """The output tensors of `cache` for Kt (made at first use), filled by
        call(BeamOutputs pointer, stream pointer) -> the library's return code."""
        dev = self.loc.torch_device
        o = cache.get(Kt)
        if o is None:
            S, n, M = self.S, max(Kt, 0), self.loc.dims.M
            o = {"audio": torch.zeros((S, n, self.hop), dtype=torch.float32, device=dev),
                 "delays": torch.zeros((S, n, M), dtype=torch.int32, device=dev),
                 "active": torch.zeros((S, n), dtype=torch.uint8, device=dev),
                 "block_start": torch.zeros(1, dtype=torch.int64, device=dev)}
            # the allocator's fills ran on the current stream: they precede the kernel on self.stream
            self.stream.wait_stream(torch.cuda.current_stream(dev))
        s = BeamOutputs(*[o[n].data_ptr() if o[n].numel() else None for n, _ in BeamOutputs._fields_])
        check(call(C.byref(s), C.c_void_p(self.stream.cuda_stream)), name)
        cache[Kt] = o  # kept only once the library accepted the arguments
        return o

    def beam(self, xy: torch.Tensor | None = None, count: torch.Tensor | None = None,
             num_targets: int | None = None, min_status: int = 2) -> dict:
        """One block of beamformed audio per stream and target
        (tdoa_stream_beam, kernel k_beam_ring; the rule is in include/tdoa.h,
        "Listening"), asynchronous on self.stream: call it after step() -- and
        after peaks() / track() when it listens to their results -- before the
        producer overwrites the ring rows of the last hop + A + 7 samples.

        xy: float32 [S][Kt][2] plane coordinates indexed by STREAM (scatter a
        step's peaks by out["stream_id"]), target k of stream s valid for
        k < count[s] (int32 [S]; None: all Kt) and finite coordinates.  xy None:
        the pipeline's own track table, channel k = track slot k (k <
        num_targets, default 8), valid iff its status >= min_status (2:
        confirmed tracks only); a channel stays with its track's id.  Returns
        device tensors allocated once per Kt and reused: audio float32
        [S][Kt][hop] (zeros for an invalid target), delays int32 [S][Kt][M]
        (the codes, -1 invalid), active uint8 [S][Kt] and block_start int64 [1],
        the absolute sample of audio[..., 0] = clock - hop - A; consecutive
        hops' blocks abut.  Every stream is written, listed by the step or not."""
        Kt = self._target_count(xy, count, num_targets, BEAM_MAX_TARGETS)
        return self._steered(self._beams, Kt, "tdoa_stream_beam", lambda out, st: load().tdoa_stream_beam(
            self._h, _ptr(count), _ptr(xy), Kt, int(min_status), out, st))

    def sep(self, xy: torch.Tensor | None = None, count: torch.Tensor | None = None,
            num_targets: int | None = None, min_status: int = 2, loading: float = SEP_LOADING) -> dict:
        """One block of null-steered audio per stream and target
        (tdoa_stream_sep, kernel k_sep; the rule is in include/tdoa.h,
        "Separating"): channel k has unit gain on target k and nulls on the
        stream's other valid targets.  Asynchronous on self.stream: call it once
        per hop after step() -- and after peaks() / track() when it separates
        their results -- before the producer overwrites the ring rows of the
        last 2 hop samples.

        Targets as beam() takes them, at most 4: xy float32 [S][Kt][2] with
        count int32 [S], or -- xy None -- the track table's slots k <
        num_targets (default 4), valid iff status >= min_status.  loading: the
        diagonal loading delta in [1e-4, 1e4].  Returns device tensors
        allocated once per Kt and reused: audio float32 [S][Kt][hop], the
        overlap-added block whose first sample is block_start int64 [1] =
        clock - 2 hop; delays int32 [S][Kt][M]; active uint8 [S][Kt].
        Consecutive hops' blocks abut; a call with another Kt starts the
        overlap-add afresh, and so does reset()."""
        Kt = self._target_count(xy, count, num_targets, SEP_MAX_TARGETS)
        return self._steered(self._seps, Kt, "tdoa_stream_sep", lambda out, st: load().tdoa_stream_sep(
            self._h, _ptr(count), _ptr(xy), Kt, int(min_status), float(loading), out, st))

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
