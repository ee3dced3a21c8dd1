#!/usr/bin/env python3
"""Config-5 hop time of the DIRECT and the GCC_PHAT streaming pipelines on the
same box: 16,384 streams, hop 512, the bench's capture generator and seed,
plain stream launches, the two pipelines interleaved in three rounds.  Writes
both hop times and the shader clock to profiles/stream_phat_hop.txt.
Diagnostic only.

    python tools/diag_stream_phat.py [S] [hops] [out.txt]

TDOA_STREAM_PHAT_GRID=n caps k_stream_phat's launch size (A/B runs).
"""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "audio-triangulation_amd"))
import torch  # noqa: E402

import tdoa  # noqa: E402
from tdoa import shard, synth  # noqa: E402
from tdoa.localizer import Localizer  # noqa: E402
from tdoa.stream import StreamPipeline  # noqa: E402

S = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
K = int(sys.argv[2]) if len(sys.argv) > 2 else 400
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "stream_phat_hop.txt")
H = 512
locs = {e: Localizer(sample_rate_hz=48000, engine=e) for e in ("direct", "gcc_phat")}
lut = locs["direct"].lut()
cap = synth.adc_stream(S, 64 * H, 3, lut, locs["direct"].dims.S, shard.frame_seed(synth.SEEDS[5], 0), device="cuda")
torch.cuda.synchronize()
pipes = {e: StreamPipeline(loc, cap, hop=H, use_graph=False) for e, loc in locs.items()}
lines = [f"config-5 shape: {S} streams, hop {H}, frame_len 1024, 3 mics, {K} hops per round, stream launches"]
best = {}
for rnd in range(3):
    for e, p in pipes.items():
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
        best[e] = min(best.get(e, dt), dt)
        lines.append(f"round {rnd} {e}: {dt:.2f} us per hop, {(trig1 - trig0) / K:.0f} triggered and "
                     f"{(gated1 - gated0) / K:.0f} gated frames per hop")
mhz = C.c_double(0.0)
st = pipes["direct"].stream
rc = tdoa.load().tdoa_gpu_clock_mhz(0, C.c_void_p(st.cuda_stream), 2.0, C.byref(mhz))
lines.append(f"best of three: direct {best['direct']:.2f} us, gcc_phat {best['gcc_phat']:.2f} us per hop "
             f"(ratio {best['gcc_phat'] / best['direct']:.2f})")
lines.append(f"gpu_clock_mhz: {mhz.value:.1f}" if rc == 0 else "gpu_clock_mhz: probe failed")
if hasattr(tdoa.load(), "tdoa_diag_fetch_stream_phat"):
    # the diagnostic library (TDOA_LIB=.../libtdoa_diag.so): k_stream_phat's phase
    # stamps of the last hop, summed over the workgroups that had slots
    import numpy as np
    d = np.zeros(4096 * 8, np.uint64)
    if tdoa.load().tdoa_diag_fetch_stream_phat(d.ctypes.data_as(C.c_void_p), d.size) == 0:
        d = d.reshape(-1, 8)
        d = d[d[:, 4] > 0].astype(np.float64)
        tot = d[:, :4].sum()
        names = ("staging", "front ends + forward FFTs", "pairs", "EMA + grid")
        lines.append(f"k_stream_phat phases, last hop, {len(d)} workgroups, {int(d[:, 4].sum())} slots: " +
                     ", ".join(f"{n} {d[:, k].sum() / tot:.1%}" for k, n in enumerate(names)))
cap_env = os.environ.get("TDOA_STREAM_PHAT_GRID")
if cap_env:
    lines.append(f"TDOA_STREAM_PHAT_GRID={cap_env}")
for p in pipes.values():
    p.close()
print("\n".join(lines))
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    f.write("\n".join(lines) + "\n")
