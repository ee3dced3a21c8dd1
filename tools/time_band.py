#!/usr/bin/env python3
"""Price the band-limited GCC-PHAT route (tdoa_set_bin_weights: k_phat_spectra,
then k_phat_pairs<true>) against the route a context takes without a table.

One context per shape, its variants alternated round by round in one process
(none / all-ones table / 1-6 kHz band), each round: set the table, two warm
launches, then K launches between two HIP events on the launch stream (the
bench's lags + grid outputs; protocol of tools/time_launch.py).  Prints one
JSON line per shape: per variant the median, minimum and maximum ms per launch
over the rounds, the kernel and grid_fused a batch reports, and the shader
clock probed after each variant's last round (tdoa_gpu_clock_mhz).
Diagnostic only.

    python tools/time_band.py [--variants=none,ones,band_1_6k] [shape ...]
        shapes: M x N x B, default 4x1024x16384 3x1024x4096 8x2048x16384
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


def clock_mhz(stream):
    mhz = C.c_double(0.0)
    rc = tdoa.load().tdoa_gpu_clock_mhz(0, C.c_void_p(stream.cuda_stream), 2.0, C.byref(mhz))
    return round(mhz.value, 1) if rc == 0 else None


def run(M, N, B, only=None):
    loc = Localizer(engine="gcc_phat", num_mics=M, frame_len=N, sample_rate_hz=FS, mic_xy=MICS[M])
    fr, _, _ = synth.adc_frames(B, M, N, loc.lut(), loc.dims.S, 7, device="cuda")
    out = loc.alloc_outputs(B)
    tables = {"none": None, "ones": np.ones(N + 1, np.float32), "band_1_6k": tdoa.band_weights(N, FS, 1000, 6000)}
    if only:  # e.g. under a kernel trace, where one kernel name must mean one table
        tables = {k: tables[k] for k in only}
    st = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = {k: [] for k in tables}
    info = {}
    # launches per timed window: about 60 ms of the unweighted route, 20..400
    for _ in range(3):
        loc.localize_into(fr, out)
    e0.record()
    for _ in range(5):
        loc.localize_into(fr, out)
    e1.record()
    torch.cuda.synchronize()
    K = int(min(400, max(20, 60.0 / max(e0.elapsed_time(e1) / 5, 1e-3))))
    for r in range(ROUNDS):
        for name, w in tables.items():
            torch.cuda.synchronize()  # nothing of the context in flight when the table changes
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
    res = {"shape": f"{M}x{N}", "B": B, "rounds": ROUNDS, "launches_per_round": K,
           "nonzero_bins": {k: (N + 1 if w is None else int((w != 0).sum())) for k, w in tables.items()}}
    for name, v in ms.items():
        v = sorted(v)
        res[name] = {"ms_median": round(v[len(v) // 2], 4), "ms_min": round(v[0], 4), "ms_max": round(v[-1], 4),
                     **info[name]}
    med = {k: res[k]["ms_median"] for k in tables}
    if "ones" in med and "none" in med:
        res["ones_over_none"] = round(med["ones"] / med["none"], 4)
    if "ones" in med and "band_1_6k" in med:
        res["band_over_ones"] = round(med["band_1_6k"] / med["ones"], 4)
    loc.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--variants=")]
    only = [a.split("=", 1)[1].split(",") for a in sys.argv[1:] if a.startswith("--variants=")]
    for s in args or ["4x1024x16384", "3x1024x4096", "8x2048x16384"]:
        run(*[int(x) for x in s.lower().split("x")], only=only[0] if only else None)
