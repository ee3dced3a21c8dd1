#!/usr/bin/env python3
"""Config 5 hop time by launch form: the per-hop hipGraph (the bench's form)
against plain stream launches of the same two kernels, interleaved, same box.
Diagnostic only.  The optional shape arguments measure other pipelines the
same way, e.g. the LDS trigger's shapes: 1024 384 3, or 1024 512 8.

    python tools/diag_stream_launch.py [S] [hops] [frame_len] [hop] [mics] [direct|gcc_phat]
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "audio-triangulation_amd"))
import torch  # noqa: E402

from tdoa import synth  # noqa: E402
from tdoa.localizer import Localizer  # noqa: E402
from tdoa.stream import StreamPipeline  # noqa: E402

S = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
K = int(sys.argv[2]) if len(sys.argv) > 2 else 400
N = int(sys.argv[3]) if len(sys.argv) > 3 else 1024
H = int(sys.argv[4]) if len(sys.argv) > 4 else 512
M = int(sys.argv[5]) if len(sys.argv) > 5 else 3
ENGINE = sys.argv[6] if len(sys.argv) > 6 else "direct"
MICS = {2: [[-0.066, 0], [0.066, 0]], 3: None, 4: synth.square_mics(0.15), 8: synth.circle_mics()}
loc = Localizer(sample_rate_hz=48000, frame_len=N, num_mics=M, mic_xy=MICS[M], engine=ENGINE)
cap = synth.adc_stream(S, 64 * H, M, loc.lut(), loc.dims.S, synth.SEEDS[5], device="cuda")
torch.cuda.synchronize()
pipes = {g: StreamPipeline(loc, cap, hop=H, use_graph=g) for g in (True, False)}
for rnd in range(3):
    for g, p in pipes.items():
        for _ in range(20):
            p.step()
        p.stream.synchronize()
        t0 = time.perf_counter()
        for _ in range(K):
            p.step()
        p.stream.synchronize()
        dt = (time.perf_counter() - t0) / K
        print(f"round {rnd} graph={int(g)}: {dt * 1e6:.2f} us per hop")
for p in pipes.values():
    p.close()
