#!/usr/bin/env python3
"""Config-5 cost of the per-hop beamformer (tdoa_stream_beam: k_beam_ring) next
to its traffic floor and next to the hop itself: 16,384 streams, hop 512,
frame_len 1024, 3 mics, the bench's capture generator and seed, plain stream
launches, everything in one process on one box.

Pipelines: u8 (the DIRECT triggered hop on the 8-bit ring) and int16 (a
continuous GCC_PHAT pipeline on an int16 ring, activity_var 2^30: nothing is
listed, the hop is the lister alone -- the ring type is what matters here).

Per pipeline, three alternated rounds of
    hop            --hops steps, host clock around them, one synchronise at the end
    hop+beamK      the same with beam(xy, Kt = K) after every step, K = 1, 2, 4
then device events around --reps back-to-back k_beam_ring launches on the block
the last step left (the same 25 / 50 MB every time: they stay in the last-level
cache, so this is the kernel's floor, not its cold-ring time; the per-hop
difference above is the figure with the hop's own traffic in between), five
alternated rounds per Kt.  Bytes moved: S M (hop + Dmax + 15) sizeof(T) read,
S Kt hop 4 written; the share is of --sweep-tbs, the 16-byte read sweep of
profiles/r05_hbm_calibration.json that profiles/stream_cont_hop.txt refers to.

--hop-only times the hops alone and uses nothing this file's commit added, so
with --pkg DIR it measures another build of the project (the parent commit) on
the same box in the same job.

Appends to profiles/stream_beam_hop.txt.  Diagnostic only.

    python tools/diag_stream_beam.py [--streams S] [--hops K] [--reps R] [--hop-only]
                                     [--pkg DIR] [--label TEXT] [--out FILE] [--sweep-tbs X]
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
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--hop-only", action="store_true")
ap.add_argument("--pkg", default=os.path.join(ROOT, "audio-triangulation_amd"))
ap.add_argument("--label", default="")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_beam_hop.txt"))
ap.add_argument("--sweep-tbs", type=float, default=6.86)
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
lines = [f"{a.label or os.path.abspath(a.pkg)}: {S} streams, hop {H}, frame_len {N}, {M} mics, {K} hops per round, "
         f"stream launches"]
rng = torch.Generator(device="cuda")
rng.manual_seed(5)
xy = {kt: (torch.rand((S, kt, 2), device="cuda", generator=rng) * 4 - 2).contiguous() for kt in KTS}


def hops(p, kt):
    """us per hop over K hops, beam(xy[kt]) after every step if kt."""
    def one():
        p.step()
        if kt:
            p.beam(xy[kt])
    for _ in range(20):
        one()
    p.stream.synchronize()
    t0 = time.perf_counter()
    for _ in range(K):
        one()
    p.stream.synchronize()
    return (time.perf_counter() - t0) / K * 1e6


def name(kt):
    return "hop" if not kt else f"hop+beam{kt}"


forms = (0,) if a.hop_only else (0,) + KTS
hop_t = {(n, kt): [] for n in pipes for kt in forms}
for rnd in range(3):
    for n, p in pipes.items():
        for kt in forms:
            hop_t[(n, kt)].append(hops(p, kt))
            lines.append(f"  round {rnd} {n} {name(kt)}: {hop_t[(n, kt)][-1]:.2f} us per hop")
for n in pipes:
    base = min(hop_t[(n, 0)])
    lines.append(f"  best of three {n}: " + ", ".join(
        f"{name(kt)} {min(hop_t[(n, kt)]):.2f} us (spread "
        f"{max(hop_t[(n, kt)]) - min(hop_t[(n, kt)]):.2f}" + (f", +{min(hop_t[(n, kt)]) - base:.2f}" if kt else "") + ")"
        for kt in forms))


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
    for n, p in pipes.items():
        A, D = locs[n].beam_latency()
        size = 1 if n == "u8" else 2
        st = C.c_void_p(p.stream.cuda_stream)
        t = {kt: [] for kt in KTS}
        calls = {}
        for kt in KTS:
            o = p.beam(xy[kt])
            bo = BeamOutputs(*[o[k].data_ptr() for k, _ in BeamOutputs._fields_])
            xp = C.c_void_p(xy[kt].data_ptr())

            def call(bo=bo, xp=xp, kt=kt):
                assert L.tdoa_stream_beam(p._h, None, xp, kt, 2, C.byref(bo), st) == 0
            calls[kt] = call
        p.stream.synchronize()
        for rnd in range(5):
            for kt in KTS:
                t[kt].append(events(calls[kt], p.stream, a.reps))
        for kt in KTS:
            rd, wr = S * M * (H + D + 15) * size, S * kt * H * 4
            us = min(t[kt])
            tbs = (rd + wr) / us / 1e6
            lines.append(f"  {n} ring, Kt {kt} (A {A}, Dmax {D}): k_beam_ring {us:.2f} us (spread over 5 rounds "
                         f"{max(t[kt]) - us:.2f}), {rd / 1e6:.1f} MB read + {wr / 1e6:.1f} MB written = {tbs:.2f} TB/s, "
                         f"{100 * tbs / a.sweep_tbs:.0f} % of the {a.sweep_tbs} TB/s read sweep; the bytes alone would "
                         f"take {(rd + wr) / a.sweep_tbs / 1e6:.1f} us")

mhz = C.c_double(0.0)
rc = tdoa.load().tdoa_gpu_clock_mhz(0, C.c_void_p(pipes["u8"].stream.cuda_stream), 2.0, C.byref(mhz))
lines.append(f"  gpu_clock_mhz: {mhz.value:.1f}" if rc == 0 else "  gpu_clock_mhz: probe failed")
for p in pipes.values():
    p.close()
print("\n".join(lines))
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "a") as f:
    f.write("\n".join(lines) + "\n")
