#!/usr/bin/env python3
"""Price the 16-bit PCM routes of GCC_PHAT (tdoa_set_sample_format) against the
8-bit route of the same context and against PCM16 on the two-pass kernels.

One context per shape, its variants alternated round by round in one process:
  adc8         the 8-bit front end on synth.adc_frames (the bench's frames);
  pcm16        the format's own route (k_p1k_pcm16 / k_f16_pcm16 where the shape
               has one, else the two-pass kernels) on synth.pcm16_frames;
  pcm16_2pass  PCM16 forced onto the two-pass route by an all-ones weight
               table (k_phat_spectra_pcm16, k_phat_pairs<true>, then the grid).
Each round: set the variant, two warm launches, then K launches between two
HIP events on the launch stream (the bench's lags + grid outputs; protocol of
tools/time_band.py).  The PCM16 batch is 512 distinct scenario frames tiled to
B.  Prints one JSON line per shape: per variant the median, minimum and maximum
ms per launch over the rounds, the kernel and grid_fused a batch reports, and
the shader clock probed after each variant's last round (tdoa_gpu_clock_mhz).
Diagnostic only.

    python tools/time_pcm16.py [shape ...]
        shapes: M x N x B, default 3x1024x4096 4x4096x16384 8x2048x16384
                4x1024x16384 3x4096x16384 4x2048x16384
"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "audio-triangulation_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import tdoa  # noqa: E402
from tdoa import synth  # noqa: E402
from tdoa.localizer import Localizer  # noqa: E402

ROUNDS, FS = 9, 50000
MICS = {3: None, 4: synth.square_mics(0.15), 8: synth.circle_mics(8, 0.15)}
DELAYS = [0, 7, -12, 20, 3, -5, 9, -17]
DC = [12000, -9000, 5000, -12000, 800, -3000, 10000, -7000]


def clock_mhz(stream):
    mhz = C.c_double(0.0)
    rc = tdoa.load().tdoa_gpu_clock_mhz(0, C.c_void_p(stream.cuda_stream), 2.0, C.byref(mhz))
    return round(mhz.value, 1) if rc == 0 else None


def run(M, N, B):
    loc = Localizer(engine="gcc_phat", num_mics=M, frame_len=N, sample_rate_hz=FS, mic_xy=MICS[M])
    S = loc.dims.S
    fr8, _, _ = synth.adc_frames(B, M, N, loc.lut(), S, 7, device="cuda")
    tile, _ = synth.pcm16_frames(min(B, 512), M, N, S, 7, DELAYS, dc=DC, device="cuda")
    fr16 = tile.repeat((B + len(tile) - 1) // len(tile), 1, 1)[:B].contiguous()
    out = loc.alloc_outputs(B)
    ones = np.ones(N + 1, np.float32)
    variants = {"adc8": ("adc8", None, fr8), "pcm16": ("pcm16", None, fr16), "pcm16_2pass": ("pcm16", ones, fr16)}
    st = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = {k: [] for k in variants}
    info = {}
    # launches per timed window: about 60 ms of the 8-bit route, 20..400
    for _ in range(3):
        loc.localize_into(fr8, out)
    e0.record()
    for _ in range(5):
        loc.localize_into(fr8, out)
    e1.record()
    torch.cuda.synchronize()
    K = int(min(400, max(20, 60.0 / max(e0.elapsed_time(e1) / 5, 1e-3))))
    for r in range(ROUNDS):
        for name, (fmt, w, fr) in variants.items():
            torch.cuda.synchronize()  # nothing of the context in flight when the setters run
            loc.set_sample_format(fmt)
            loc.set_bin_weights(w)
            for _ in range(2):
                loc.localize_into(fr, out)
            e0.record()
            for _ in range(K):
                loc.localize_into(fr, out)
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / K)
            if r == ROUNDS - 1:
                info[name] = {"kernel": loc.batch_kernel(), "grid_fused": loc.batch_grid_fused(),
                              "gpu_clock_mhz": clock_mhz(st)}
    res = {"shape": f"{M}x{N}", "B": B, "rounds": ROUNDS, "launches_per_round": K}
    for name, v in ms.items():
        v = sorted(v)
        res[name] = {"ms_median": round(v[len(v) // 2], 4), "ms_min": round(v[0], 4), "ms_max": round(v[-1], 4),
                     **info[name]}
    med = {k: res[k]["ms_median"] for k in variants}
    res["pcm16_over_adc8"] = round(med["pcm16"] / med["adc8"], 4)
    res["two_pass_over_pcm16"] = round(med["pcm16_2pass"] / med["pcm16"], 4)
    loc.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    for s in sys.argv[1:] or ["3x1024x4096", "4x4096x16384", "8x2048x16384", "4x1024x16384", "3x4096x16384",
                              "4x2048x16384"]:
        run(*[int(x) for x in s.lower().split("x")])
