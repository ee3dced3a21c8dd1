#!/usr/bin/env python3
"""Config-5 hop time of the GCC_PHAT streaming pipeline on an 8-bit capture ring
and on the int16 ring holding (u8 - 128) * 256 of the same capture (so both
trigger the same frames at every hop): 16,384 streams, hop 512, frame_len 1024,
3 mics, the bench's capture generator and seed, plain stream launches, the
pipelines interleaved in three rounds.  Appends the hop times and the shader
clock to profiles/stream_pcm16_hop.txt.  Diagnostic only.

    python tools/diag_stream_pcm16.py [--streams S] [--hops K] [--formats adc8,pcm16]
                                      [--pkg DIR] [--label TEXT] [--out FILE]

--pkg DIR: the directory holding the `tdoa` package to measure (default: this
tree's); with --formats adc8 it measures another build of the project, e.g.
the commit before the int16 pipeline, on the same box in the same job.
"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--streams", type=int, default=16384)
ap.add_argument("--hops", type=int, default=400)
ap.add_argument("--formats", default="adc8,pcm16")
ap.add_argument("--pkg", default=os.path.join(ROOT, "audio-triangulation_amd"))
ap.add_argument("--label", default="")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_pcm16_hop.txt"))
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.pkg))
import torch  # noqa: E402

import tdoa  # noqa: E402
from tdoa import shard, synth  # noqa: E402
from tdoa.localizer import Localizer  # noqa: E402
from tdoa.stream import StreamPipeline  # noqa: E402

S, K, H = a.streams, a.hops, 512
formats = a.formats.split(",")
locs = {f: Localizer(sample_rate_hz=48000, engine="gcc_phat") for f in formats}
first = locs[formats[0]]
adc = synth.adc_stream(S, 64 * H, 3, first.lut(), first.dims.S, shard.frame_seed(synth.SEEDS[5], 0), device="cuda")
caps = {"adc8": adc}
if "pcm16" in formats:
    locs["pcm16"].set_sample_format("pcm16")
    caps["pcm16"] = ((adc.to(torch.int16) - 128) * 256).contiguous()
torch.cuda.synchronize()
pipes = {f: StreamPipeline(locs[f], caps[f], hop=H, use_graph=False) for f in formats}
lines = [f"{a.label or os.path.abspath(a.pkg)}: {S} streams, hop {H}, frame_len 1024, 3 mics, {K} hops per round, "
         f"stream launches, GCC_PHAT"]
times = {f: [] for f in formats}
for rnd in range(3):
    for f, p in pipes.items():
        for _ in range(20):
            p.step()
        p.stream.synchronize()
        _, trig0, gated0 = p.totals()
        t0 = time.perf_counter()
        for _ in range(K):
            p.step()
        p.stream.synchronize()
        dt = (time.perf_counter() - t0) / K * 1e6
        _, trig1, gated1 = p.totals()
        times[f].append(dt)
        lines.append(f"  round {rnd} {f}: {dt:.2f} us per hop, {(trig1 - trig0) / K:.0f} triggered and "
                     f"{(gated1 - gated0) / K:.0f} gated frames per hop")
mhz = C.c_double(0.0)
rc = tdoa.load().tdoa_gpu_clock_mhz(0, C.c_void_p(pipes[formats[0]].stream.cuda_stream), 2.0, C.byref(mhz))
lines.append("  best of three: " + ", ".join(f"{f} {min(t):.2f} us (spread {max(t) - min(t):.2f})"
                                             for f, t in times.items()) +
             (f"; pcm16 / adc8 = {min(times['pcm16']) / min(times['adc8']):.3f}" if len(formats) == 2 else ""))
lines.append(f"  gpu_clock_mhz: {mhz.value:.1f}" if rc == 0 else "  gpu_clock_mhz: probe failed")
for p in pipes.values():
    p.close()
print("\n".join(lines))
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "a") as f:
    f.write("\n".join(lines) + "\n")
