#!/usr/bin/env python3
"""Hop time and per-kernel times of the long-frame streaming route (selector ->
k_f16_ring -> k_stream_ema_grid) at 8 mics x 2048 (hop 1024) and 4 mics x 4096
(hop 2048): 4096 streams, continuous mode at activity_var = 0 (every stream
listed every hop), on a uint8 ring and on the int16 ring holding
(u8 - 128) * 256 of it, plain stream launches.  Next to them, in the same
process, the batch engine on 4096 contiguous frames holding the same samples
(k_frame16 / k_f16_pcm16 + k_grid_bb).

One process per shape.  Each shape runs twice: plain, for the wall-clock time
per hop and per batch call, and (unless --no-profile) under
`rocprofv3 --kernel-trace --stats` with fewer hops, for the kernels' average
durations.  Appends everything and the shader clock to
profiles/stream_long_hop.txt.  Diagnostic only.

    python tools/diag_stream_long.py [--streams S] [--hops K] [--no-profile] [--label TEXT] [--out FILE]
"""
import argparse
import csv
import glob
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(8, 2048, 1024), (4, 4096, 2048)]
KERNELS = ("k_stream_active", "k_f16_ring", "k_stream_ema_grid", "k_frame16", "k_f16_pcm16", "k_grid_bb")
ap = argparse.ArgumentParser()
ap.add_argument("--streams", type=int, default=4096)
ap.add_argument("--hops", type=int, default=60)
ap.add_argument("--no-profile", action="store_true")
ap.add_argument("--label", default="")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_long_hop.txt"))
ap.add_argument("--child", nargs=3, type=int, metavar=("M", "N", "HOP"), help=argparse.SUPPRESS)
a = ap.parse_args()


def child(M, N, H):
    import ctypes as C

    sys.path.insert(0, os.path.join(ROOT, "audio-triangulation_amd"))
    import torch

    import tdoa
    from tdoa import synth
    from tdoa.localizer import Localizer
    from tdoa.stream import StreamPipeline

    S, K = a.streams, a.hops
    mics = {8: synth.circle_mics(), 4: synth.square_mics(0.15)}[M]
    locs = {f: Localizer(engine="gcc_phat", num_mics=M, frame_len=N, sample_rate_hz=48000, mic_xy=mics, sample_format=f)
            for f in ("adc8", "pcm16")}
    L = N + 2 * H  # the smallest ring
    adc = synth.adc_stream(S, L, M, locs["adc8"].lut(), locs["adc8"].dims.S, 910, device="cuda")
    caps = {"adc8": adc, "pcm16": ((adc.to(torch.int16) - 128) * 256).contiguous()}
    # the batch frames: every stream's ring samples [0, N) -- the frame the hop ending at N lists
    frames = {f: c[:, :N].permute(0, 2, 1).to(torch.int16).contiguous() for f, c in caps.items()}
    outs = {f: locs[f].alloc_outputs(S, scores=False, grid=True) for f in caps}
    pipes = {f: StreamPipeline(locs[f], caps[f], hop=H, mode="continuous", activity_var=0) for f in caps}
    torch.cuda.synchronize()
    print(f"  {M} mics x {N}, hop {H}, {S} streams, ring {L} samples, {K} hops per round: stream kernel "
          f"{pipes['adc8'].kernel}, batch kernel {locs['adc8'].batch_kernel()}")
    hop_t, bat_t = {f: [] for f in caps}, {f: [] for f in caps}
    for rnd in range(3):
        for f, p in pipes.items():
            for _ in range(6):
                p.step()
            p.stream.synchronize()
            _, l0, g0 = p.totals()
            t0 = time.perf_counter()
            for _ in range(K):
                p.step()
            p.stream.synchronize()
            hop_t[f].append((time.perf_counter() - t0) / K * 1e6)
            _, l1, g1 = p.totals()
            launch = locs[f].prepare(frames[f], outs[f])
            for _ in range(3):
                launch()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(K):
                launch()
            torch.cuda.synchronize()
            bat_t[f].append((time.perf_counter() - t0) / K * 1e6)
            print(f"  round {rnd} {f}: hop {hop_t[f][-1]:.1f} us ({(l1 - l0) / K:.0f} listed, {(g1 - g0) / K:.0f} gated "
                  f"per hop), batch of {S} frames {bat_t[f][-1]:.1f} us")
    for f in caps:
        print(f"  best of three {f}: hop {min(hop_t[f]):.1f} us (spread {max(hop_t[f]) - min(hop_t[f]):.1f}), "
              f"{min(hop_t[f]) * 1e3 / S:.1f} ns per frame; batch {min(bat_t[f]):.1f} us "
              f"(spread {max(bat_t[f]) - min(bat_t[f]):.1f}), {min(bat_t[f]) * 1e3 / S:.1f} ns per frame")
    mhz = C.c_double(0.0)
    rc = tdoa.load().tdoa_gpu_clock_mhz(0, C.c_void_p(pipes["adc8"].stream.cuda_stream), 2.0, C.byref(mhz))
    print(f"  gpu_clock_mhz: {mhz.value:.1f}" if rc == 0 else "  gpu_clock_mhz: probe failed")
    for p in pipes.values():
        p.close()


def kernel_rows(d):
    rows = []
    for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            n = r["Name"].replace("void ", "").replace("(anonymous namespace)::", "").split("(")[0]
            if any(k in n for k in KERNELS):
                rows.append(f"    {n[:56]:56s} calls {int(r['Calls']):5d}  avg {float(r['AverageNs']) / 1e3:9.2f} us")
    return sorted(rows)


if a.child:
    child(*a.child)
    sys.exit(0)

lines = [f"{a.label or 'long-frame streaming'}: continuous, activity_var 0, stream launches, GCC_PHAT"]
me = os.path.abspath(__file__)
for M, N, H in SHAPES:
    base = [sys.executable, me, "--streams", str(a.streams), "--child", str(M), str(N), str(H)]
    r = subprocess.run(base + ["--hops", str(a.hops)], capture_output=True, text=True, timeout=400)
    if r.returncode != 0:
        sys.exit(f"{M} x {N}: the measuring process failed\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    lines += r.stdout.rstrip().splitlines()
    if not a.no_profile and shutil.which("rocprofv3"):
        with tempfile.TemporaryDirectory() as td:
            r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", td, "-o", "run", "--output-format", "csv",
                                "--"] + base + ["--hops", "10"], capture_output=True, text=True, timeout=400)
            if r.returncode != 0:
                sys.exit(f"{M} x {N}: the profiled process failed\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
            rows = kernel_rows(td)
        lines.append(f"  per kernel ({M} x {N}, kernel trace; template arguments <C, M, int16 ring, weight table>):")
        lines += rows or ["    (no kernel statistics found)"]
print("\n".join(lines))
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "a") as f:
    f.write("\n".join(lines) + "\n")
