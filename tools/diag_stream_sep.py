#!/usr/bin/env python3
"""Config-5 cost of the per-hop null-steering beamformer (tdoa_stream_sep:
k_sep) next to the delay-and-sum (k_beam_ring) for the same targets, next to
k_stream_phat -- this project's own yardstick for an LDS-FFT kernel -- and next
to the hop itself: 16,384 streams, hop 512 (L = 1024), frame_len 1024, 3 mics,
the bench's capture generator and seed, everything in one process on one box.

Pipelines: u8 (the DIRECT triggered hop on the 8-bit ring), int16 (a continuous
GCC_PHAT pipeline on an int16 ring, activity_var 2^30: nothing is listed, the
hop is the lister alone) and, for the yardstick, int16-all (the same ring with
activity_var 0: every stream is listed, the hop is the lister plus
k_stream_phat_pcm16 over 16,384 frames of 3 x 1024).

Three alternated rounds of `hop` per pipeline (--hops steps, host clock around
them, one synchronise at the end): the hop without the call.  --hop-only stops
there and uses nothing this file's commit added, so with --pkg DIR it measures
another build of the project (the parent commit) on the same box in the same
job.

Then device events around --reps back-to-back launches on the block the last
step left, five alternated rounds: k_sep and k_beam_ring per Kt = 1, 2, 4 and
ring; and around --reps steps of int16-all and of int16, whose difference is
k_stream_phat_pcm16 per 16,384 frames.  The rings stay in the last-level cache
between launches: these are the kernels' floors, not cold-ring times.

Appends to profiles/stream_sep_hop.txt.  Diagnostic only.

    python tools/diag_stream_sep.py [--streams S] [--hops K] [--reps R] [--hop-only]
                                    [--pkg DIR] [--label TEXT] [--out FILE]
"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--streams", type=int, default=16384)
ap.add_argument("--hops", type=int, default=200)
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--hop-only", action="store_true")
ap.add_argument("--pkg", default=os.path.join(ROOT, "audio-triangulation_amd"))
ap.add_argument("--label", default="")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_sep_hop.txt"))
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.pkg))
import torch  # noqa: E402

import tdoa  # noqa: E402
from tdoa import shard, synth  # noqa: E402
from tdoa.localizer import Localizer  # noqa: E402
from tdoa.stream import StreamPipeline  # noqa: E402

S, K, H, N, M = a.streams, a.hops, 512, 1024, 3
KTS = (1, 2, 4)
locs = {"u8": Localizer(sample_rate_hz=48000, engine="direct"),
        "int16": Localizer(sample_rate_hz=48000, engine="gcc_phat", sample_format="pcm16")}
lut = locs["u8"].lut()
adc = synth.adc_stream(S, 64 * H, M, lut, locs["u8"].dims.S, shard.frame_seed(synth.SEEDS[5], 0), device="cuda")
pcm = ((adc[:, :8 * H].to(torch.int16) - 128) * 64).contiguous()  # an int16 ring of 8 hops
torch.cuda.synchronize()
pipes = {"u8": StreamPipeline(locs["u8"], adc, hop=H),
         "int16": StreamPipeline(locs["int16"], pcm, hop=H, mode="continuous", activity_var=1 << 30)}
lines = [f"{a.label or os.path.abspath(a.pkg)}: {S} streams, hop {H}, frame_len {N}, {M} mics, {K} hops per round"]


def hops(p):
    """us per hop over K hops."""
    for _ in range(20):
        p.step()
    p.stream.synchronize()
    t0 = time.perf_counter()
    for _ in range(K):
        p.step()
    p.stream.synchronize()
    return (time.perf_counter() - t0) / K * 1e6


hop_t = {n: [] for n in pipes}
for rnd in range(3):
    for n, p in pipes.items():
        hop_t[n].append(hops(p))
        lines.append(f"  round {rnd} {n} hop: {hop_t[n][-1]:.2f} us per hop")
for n in pipes:
    lines.append(f"  best of three {n}: hop {min(hop_t[n]):.2f} us (spread {max(hop_t[n]) - min(hop_t[n]):.2f})")


def events(fn, stream, reps):
    """us per call of `reps` back-to-back calls on `stream` (device events)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(5):
        fn()
    with torch.cuda.stream(stream):
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


if not a.hop_only:
    from tdoa._lib import BeamOutputs
    L = tdoa.load()
    rng = torch.Generator(device="cuda")
    rng.manual_seed(5)
    xy = {kt: (torch.rand((S, kt, 2), device="cuda", generator=rng) * 4 - 2).contiguous() for kt in KTS}
    pipes["int16-all"] = StreamPipeline(locs["int16"], pcm, hop=H, mode="continuous", activity_var=0)
    for _ in range(8):
        pipes["int16-all"].step()
    pipes["int16-all"].stream.synchronize()
    listed = int(pipes["int16-all"].out["count"].item())
    calls, t = {}, {}
    for n in ("u8", "int16"):
        p = pipes[n]
        st = C.c_void_p(p.stream.cuda_stream)
        for kt in KTS:
            xp = C.c_void_p(xy[kt].data_ptr())
            ob, osp = p.beam(xy[kt]), p.sep(xy[kt])
            bb = BeamOutputs(*[ob[k].data_ptr() for k, _ in BeamOutputs._fields_])
            bs = BeamOutputs(*[osp[k].data_ptr() for k, _ in BeamOutputs._fields_])

            def beam(p=p, bb=bb, xp=xp, kt=kt, st=st):
                assert L.tdoa_stream_beam(p._h, None, xp, kt, 2, C.byref(bb), st) == 0

            def sep(p=p, bs=bs, xp=xp, kt=kt, st=st):
                assert L.tdoa_stream_sep(p._h, None, xp, kt, 2, C.c_float(1e-2), C.byref(bs), st) == 0
            # (every timed series keeps one Kt: the tails are cleared once, in the warm-up)
            calls[(n, "k_beam_ring", kt)] = (beam, p.stream)
            calls[(n, "k_sep", kt)] = (sep, p.stream)
        p.stream.synchronize()
    for n in ("int16", "int16-all"):
        calls[(n, "step", 0)] = (pipes[n].step, pipes[n].stream)
    for key in calls:
        t[key] = []
    for rnd in range(5):
        for key, (fn, stream) in calls.items():
            t[key].append(events(fn, stream, a.reps))
    phat = min(t[("int16-all", "step", 0)]) - min(t[("int16", "step", 0)])
    lines.append(f"  int16-all step {min(t[('int16-all', 'step', 0)]):.2f} us (spread "
                 f"{max(t[('int16-all', 'step', 0)]) - min(t[('int16-all', 'step', 0)]):.2f}), {listed} frames listed; "
                 f"int16 step (lister alone) {min(t[('int16', 'step', 0)]):.2f} us: k_stream_phat_pcm16 {phat:.2f} us "
                 f"per {listed} frames of {M} x {N}")
    for n in ("u8", "int16"):
        A, D = locs[n].beam_latency()
        for kt in KTS:
            sp, bm = t[(n, "k_sep", kt)], t[(n, "k_beam_ring", kt)]
            lines.append(f"  {n} ring, Kt {kt} (L {2 * H}, Dmax {D}): k_sep {min(sp):.2f} us (spread over 5 rounds "
                         f"{max(sp) - min(sp):.2f}) = {min(sp) / S * 1e3:.2f} ns per stream; k_beam_ring {min(bm):.2f} us "
                         f"(spread {max(bm) - min(bm):.2f}): k_sep / k_beam_ring {min(sp) / min(bm):.2f}; "
                         f"k_sep / k_stream_phat_pcm16 {min(sp) / phat * listed / S:.2f} per row")

mhz = C.c_double(0.0)
rc = tdoa.load().tdoa_gpu_clock_mhz(0, C.c_void_p(pipes["u8"].stream.cuda_stream), 2.0, C.byref(mhz))
lines.append(f"  gpu_clock_mhz: {mhz.value:.1f}" if rc == 0 else "  gpu_clock_mhz: probe failed")
for p in pipes.values():
    p.close()
print("\n".join(lines))
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "a") as f:
    f.write("\n".join(lines) + "\n")
