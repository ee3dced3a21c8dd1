#!/usr/bin/env python3
"""Config-5 hop time of the GCC_PHAT streaming pipeline in triggered and in
continuous mode, on an 8-bit capture ring and on the int16 ring holding
(u8 - 128) * 256 of the same capture: 16,384 streams, hop 512, frame_len 1024,
3 mics, the bench's capture generator and seed, plain stream launches, all
pipelines in one process, interleaved in three rounds.

Pipelines ("mode/format"):
    trig/adc8   trig/pcm16     the click trigger (k_stream_trigger_p, k_stream_trigger_lds<int16_t>)
    cont0/*                    continuous, activity_var = 0: every stream, every hop
    contT/*                    continuous at the threshold that lists about the share
                               of streams the trigger lists (the matching quantile of
                               sum_m pw / N^2 over the capture's frames; times 65536
                               on the int16 ring)
Appends the hop times, the listed and gated frames per hop and the shader clock
to profiles/stream_cont_hop.txt.  Diagnostic only.  For the per-kernel split run
it under a kernel-trace profiler with a smaller --hops.

    python tools/diag_stream_cont.py [--streams S] [--hops K] [--pipes LIST] [--activity-var V]
                                     [--pkg DIR] [--label TEXT] [--out FILE]

--activity-var V: contT's threshold in u8 counts^2, instead of deriving it (a
profiled run then launches no kernels but those of the pipelines it names).

--pkg DIR: the directory holding the `tdoa` package to measure (default: this
tree's); with --pipes trig/adc8,trig/pcm16 it measures another build of the
project, e.g. the commit before continuous mode, on the same box in the same job.
"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = "trig/adc8,trig/pcm16,cont0/adc8,contT/adc8,cont0/pcm16,contT/pcm16"
ap = argparse.ArgumentParser()
ap.add_argument("--streams", type=int, default=16384)
ap.add_argument("--hops", type=int, default=200)
ap.add_argument("--pipes", default=ALL)
ap.add_argument("--activity-var", type=int, default=None)
ap.add_argument("--pkg", default=os.path.join(ROOT, "audio-triangulation_amd"))
ap.add_argument("--label", default="")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_cont_hop.txt"))
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.pkg))
import torch  # noqa: E402

import tdoa  # noqa: E402
from tdoa import shard, synth  # noqa: E402
from tdoa.localizer import Localizer  # noqa: E402
from tdoa.stream import StreamPipeline  # noqa: E402

S, K, H, N = a.streams, a.hops, 512, 1024
names = a.pipes.split(",")
formats = sorted({n.split("/")[1] for n in names})
locs = {f: Localizer(sample_rate_hz=48000, engine="gcc_phat") for f in formats}
first = locs[formats[0]]
adc = synth.adc_stream(S, 64 * H, 3, first.lut(), first.dims.S, shard.frame_seed(synth.SEEDS[5], 0), device="cuda")
caps = {"adc8": adc}
if "pcm16" in formats:
    locs["pcm16"].set_sample_format("pcm16")
    caps["pcm16"] = ((adc.to(torch.int16) - 128) * 256).contiguous()
torch.cuda.synchronize()

# the trigger's share of streams per hop, then the activity threshold with the same share
thr, share = a.activity_var, None
if thr is None and any(n.startswith("contT") for n in names):
    p = StreamPipeline(locs[formats[0]], caps[formats[0]], hop=H)
    for _ in range(64):
        p.step()
    share = p.totals()[1] / (64 * S)
    p.close()
    tot = []
    for h in range(2, 64, 4):  # sum_m (N sum x^2 - (sum x)^2) of the frames ending at (h + 1) H
        x = adc[:, (h + 1) * H - N:(h + 1) * H].to(torch.int64)
        tot.append((N * (x * x).sum(1) - x.sum(1) ** 2).sum(1))
    tot = torch.cat(tot).sort().values
    thr = int(tot[int((1.0 - share) * (tot.numel() - 1))].item()) // (N * N)


def make(name):
    mode, f = name.split("/")
    if mode == "trig":
        return StreamPipeline(locs[f], caps[f], hop=H, use_graph=False)
    var = 0 if mode == "cont0" else thr * (65536 if f == "pcm16" else 1)
    return StreamPipeline(locs[f], caps[f], hop=H, use_graph=False, mode="continuous", activity_var=var)


pipes = {n: make(n) for n in names}
lines = [f"{a.label or os.path.abspath(a.pkg)}: {S} streams, hop {H}, frame_len {N}, 3 mics, {K} hops per round, "
         f"stream launches, GCC_PHAT" + (f"; contT: activity_var {thr} (u8 counts^2; x 65536 on int16)" if thr is not None else "") +
         (f", the trigger lists {share:.1%} of the streams per hop" if share is not None else "")]
times = {n: [] for n in names}
for rnd in range(3):
    for n, p in pipes.items():
        for _ in range(20):
            p.step()
        p.stream.synchronize()
        _, l0, g0 = p.totals()
        t0 = time.perf_counter()
        for _ in range(K):
            p.step()
        p.stream.synchronize()
        dt = (time.perf_counter() - t0) / K * 1e6
        _, l1, g1 = p.totals()
        times[n].append(dt)
        lines.append(f"  round {rnd} {n}: {dt:.2f} us per hop, {(l1 - l0) / K:.0f} listed and "
                     f"{(g1 - g0) / K:.0f} gated frames per hop")
mhz = C.c_double(0.0)
rc = tdoa.load().tdoa_gpu_clock_mhz(0, C.c_void_p(pipes[names[0]].stream.cuda_stream), 2.0, C.byref(mhz))
lines.append("  best of three: " + ", ".join(f"{n} {min(t):.2f} us (spread {max(t) - min(t):.2f})"
                                             for n, t in times.items()))
lines.append(f"  gpu_clock_mhz: {mhz.value:.1f}" if rc == 0 else "  gpu_clock_mhz: probe failed")
for p in pipes.values():
    p.close()
print("\n".join(lines))
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "a") as f:
    f.write("\n".join(lines) + "\n")
