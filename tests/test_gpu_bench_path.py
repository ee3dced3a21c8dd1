"""The exact outputs bench.py times, checked against the checked path, bit for bit.

bench.py's timed launches never request scores (tdoa_localize_batch with only
lags / gate / cell / xy / max_Lf, plus xy_ls / ls_rms at config 4).  Without
weighted scores the library takes its lean paths:
  config 2   k_p1k_lean's no-debug-output branch (grid fused in the kernel)
  config 3/4 k_frame16 writes only the grid-used lags into a compact scratch
             (kp.wc_*), which k_grid_bb expands in LDS (tdoa_capi.cpp run_batch)
Every fp64 / exhaustive-grid test requests scores, i.e. the full-scratch
layout.  So, per shape and input kind, this asserts:
  1. localize(fr) == localize(fr, scores=True): lags, gate, cell, xy, max_Lf
     (and xy_ls, ls_rms at config 4) bit for bit;
  2. the no-scores cell / max_Lf == the exhaustive float32 scan
     (vga_heatmap.h:99-108, first row-major max) of the scores run's weighted_f;
  3. the same no-scores outputs from a child process run with
     TDOA_NO_COMPACT=1 (the full weighted-score scratch) are bit-equal.
Inputs: ADC-like integer-delay frames (the bench's generator), noise-only
frames (flat scores, weak grid bounds) and a ragged batch (a partly filled last
workgroup / wave).  Reference: correlations.c:20-33, vga_heatmap.h:99-108.
  4. configs 3/4 with TDOA_F16_CHUNK=512 (the compact scratch of one chunk of
     frames at a time, reused; read once per process, so a child process): whole
     chunks (B = 2048) and a last chunk of 5 frames (B = 2053) bit-equal to the
     unchunked run, the least squares over the full batch included.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tdoa import synth  # noqa: E402
from tdoa.localizer import Localizer  # noqa: E402
from test_gpu_gcc_phat import _grid_f32, _np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# BASELINE configs 2-4 at test sizes: (M, N, mics, B, ragged B, least squares)
SHAPES = {
    "cfg2": (3, 1024, None, 4096, 4093, False),
    "cfg3": (4, 4096, "square", 2048, 2053, False),
    "cfg4": (8, 2048, "circle", 2048, 2053, True),
}
KINDS = ("adc", "noise_only", "ragged")
OUT_KEYS = ("lags", "gate", "cell", "xy", "max_Lf", "xy_ls", "ls_rms")


def _mics(kind):
    return {None: None, "square": synth.square_mics(0.15), "circle": synth.circle_mics(8, 0.15)}[kind]


def _localizer(shape):
    M, N, mics, *_ = SHAPES[shape]
    return Localizer(engine="gcc_phat", num_mics=M, frame_len=N, mic_xy=_mics(mics))


def _frames(shape, kind, loc):
    M, N, _, B, Br, _ = SHAPES[shape]
    P, S = loc.dims.P, loc.dims.S
    seed = synth.SEEDS[int(shape[-1])]
    if kind == "noise_only":
        g = torch.Generator(device="cpu").manual_seed(seed & 0xFFFF)
        return torch.randint(0, 256, (B, M, N), generator=g, dtype=torch.int16).cuda()
    n = Br if kind == "ragged" else B
    fr, _, _ = synth.adc_frames(n, M, N, loc.lut().reshape(P, 101, 101), S, seed + (kind == "ragged"),
                                device="cuda")
    return fr.contiguous()


def _bench_outputs(loc, fr, ls):
    """What bench.py's prepared launch writes (no scores requested)."""
    out = loc.alloc_outputs(fr.shape[0], ls=ls)
    loc.localize_into(fr, out)
    torch.cuda.synchronize()
    return _np(out)


CHILD = r"""
import sys
sys.path[:0] = [{pkg!r}, {tests!r}]
import numpy as np, torch
from test_gpu_bench_path import SHAPES, _localizer, _bench_outputs
shape = {shape!r}
loc = _localizer(shape)
res = {{}}
for kind in {kinds!r}:
    fr = torch.from_numpy(np.load({tmp!r} + "/" + kind + ".npy")).cuda()
    for k, v in _bench_outputs(loc, fr, SHAPES[shape][5]).items():
        res[kind + "." + k] = v
np.savez({tmp!r} + "/child.npz", **res)
print("child ok", loc.batch_kernel())
"""


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_bench_path_equals_checked_path(shape, tmp_path):
    ls = SHAPES[shape][5]
    loc = _localizer(shape)
    lut = loc.lut()
    mine = {}
    for kind in KINDS:
        fr = _frames(shape, kind, loc)
        np.save(tmp_path / f"{kind}.npy", fr.cpu().numpy())
        bench = _bench_outputs(loc, fr, ls)
        checked = _np(loc.localize(fr, scores=True, ls=ls))
        mine[kind] = bench
        # 1. the lean (no-scores) path equals the scores-requested path
        for k in OUT_KEYS:
            if k in bench:
                assert k in checked, k
                assert np.array_equal(bench[k], checked[k]), (shape, kind, k)
        # 2. its grid answer equals the exhaustive f32 scan of the engine's own scores
        cell, mx = _grid_f32(checked["weighted_f"], lut)
        assert np.array_equal(bench["cell"], cell), (shape, kind)
        assert np.array_equal(bench["max_Lf"], mx), (shape, kind)
        if ls:
            assert np.isfinite(bench["xy_ls"]).all()
    kernel = loc.batch_kernel()
    loc.close()
    # 3. the full weighted-score scratch (TDOA_NO_COMPACT=1) in a child process
    code = CHILD.format(pkg=os.path.join(ROOT, "audio-triangulation_amd"), tests=os.path.join(ROOT, "tests"),
                        shape=shape, kinds=KINDS, tmp=str(tmp_path))
    env = dict(os.environ, TDOA_NO_COMPACT="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "child ok " + kernel in r.stdout
    child = np.load(tmp_path / "child.npz")
    for kind in KINDS:
        for k, v in mine[kind].items():
            assert np.array_equal(child[f"{kind}.{k}"], v), (shape, kind, k)


@pytest.mark.parametrize("shape", ["cfg3", "cfg4"])
def test_chunked_compact_path_equals_unchunked(shape, tmp_path):
    ls = SHAPES[shape][5]
    kinds = ("adc", "ragged")
    loc = _localizer(shape)
    mine = {}
    for kind in kinds:
        fr = _frames(shape, kind, loc)
        assert fr.shape[0] > 4 * 512 - 1
        np.save(tmp_path / f"{kind}.npy", fr.cpu().numpy())
        mine[kind] = _bench_outputs(loc, fr, ls)
        assert set(mine[kind]) == set(OUT_KEYS) - (set() if ls else {"xy_ls", "ls_rms"})
    kernel = loc.batch_kernel()
    loc.close()
    code = CHILD.format(pkg=os.path.join(ROOT, "audio-triangulation_amd"), tests=os.path.join(ROOT, "tests"),
                        shape=shape, kinds=kinds, tmp=str(tmp_path))
    env = dict(os.environ, TDOA_F16_CHUNK="512")
    env.pop("TDOA_NO_COMPACT", None)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "child ok " + kernel in r.stdout
    child = np.load(tmp_path / "child.npz")
    for kind in kinds:
        for k, v in mine[kind].items():
            assert np.array_equal(child[f"{kind}.{k}"], v), (shape, kind, k)
