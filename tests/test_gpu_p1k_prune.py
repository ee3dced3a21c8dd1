"""k_p1k_lean's pruned grid scan on the GPU (DESIGN.md "k_p1k_lean": the 4-wave
workgroup scans only the rows of 64 tuples whose exact bound reaches the best
L).  With Localizer(engine="gcc_phat"), cell and max_Lf must equal an
exhaustive float32 ((w0 + w1) + w2) scan of the kernel's own weighted_f bit
for bit (ties to the first row-major cell), on

  * 64 ADC frames (a few rows survive) and 64 uncorrelated-noise frames (nearly
    every row survives: the wave falls back to the exhaustive scan);
  * 16 constant frames (every tuple ties: cell 0's tuple), all-zero frames,
    known-answer click frames;
  * waves that mix a peaked frame 2w with a constant or a noisy frame 2w + 1;
  * batches of 1, 2, 15 and 17 frames (the ragged last wave and workgroup),

once with the debug score outputs and once without (the benchmark's branch of
the kernel), whose cell, xy and max_Lf must be the first launch's bytes.  The
A/B library's 8-wave shape (TDOA_P1K=lean8) keeps the exhaustive scan: every
output of both launches must be the same bytes as the product's.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import known_answer as KA

pytestmark = pytest.mark.gpu

from tdoa import synth  # noqa: E402
from tdoa.localizer import Localizer  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AB_LIB = os.path.join(ROOT, "audio-triangulation_amd", "tdoa", "libtdoa_ab.so")
PATHS = [os.path.join(ROOT, "audio-triangulation_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
KINDS = ("adc", "noise", "constant", "zero", "click", "mixed_constant", "mixed_noise", "b1", "b2", "b15", "b17")


def _grid_f32(weighted, lut):
    """vga_heatmap.h:99-108 on the engine's own float weighted scores, in float32
    with the kernel's association ((w0 + w1) + w2): the first cell of max L, and max L."""
    w = np.asarray(weighted, np.float32)
    lut2 = np.asarray(lut).reshape(w.shape[1], -1).astype(np.int64)
    L = w[:, 0][:, lut2[0]]
    for p in range(1, w.shape[1]):
        L = (L + w[:, p][:, lut2[p]]).astype(np.float32)
    return L.argmax(-1).astype(np.int32), L.max(-1)


def inputs(lut):
    """kind -> int16 [B][3][1024] frames (CPU tensors), from seeds."""
    lut3 = np.asarray(lut).reshape(3, 101, 101)
    adc = synth.adc_frames(64, 3, 1024, lut3, 46, 0x9A)[0]
    noise = torch.randint(0, 256, (64, 3, 1024), generator=torch.Generator().manual_seed(7), dtype=torch.int16)
    click = torch.from_numpy(KA.click_frames([[0, 5, 9], [0, -3, 4], [7, 0, -6], [0, 0, 0], [0, 40, -40], [0, None, 3]],
                                             3, 1024))
    mixc, mixn = adc.clone(), adc.clone()
    mixc[1::2] = 77
    mixn[1::2] = noise[1::2]
    d = {"adc": adc, "noise": noise, "constant": torch.full((16, 3, 1024), 77, dtype=torch.int16),
         "zero": torch.zeros((4, 3, 1024), dtype=torch.int16), "click": click, "mixed_constant": mixc,
         "mixed_noise": mixn}
    for b in (1, 2, 15, 17):
        d[f"b{b}"] = synth.adc_frames(b, 3, 1024, lut3, 46, 0x9B + b)[0]
    assert tuple(d) == KINDS
    return {k: v.contiguous() for k, v in d.items()}


def run_all(ph):
    """kind/launch/output -> array: both launches of every kind."""
    res = {}
    for kind, fr in inputs(ph.lut()).items():
        fr = fr.cuda()
        for scores in (True, False):
            out = ph.localize(fr, scores=scores)
            torch.cuda.synchronize()
            for k, v in out.items():
                res[f"{kind}/{int(scores)}/{k}"] = v.cpu().numpy()
    return res


@pytest.fixture(scope="module")
def product():
    ph = Localizer(engine="gcc_phat")
    assert ph.batch_kernel() == "k_p1k_lean", ph.batch_kernel()
    res = run_all(ph)
    lut = ph.lut()
    ph.close()
    for v in res.values():
        v.flags.writeable = False
    return res, lut


@pytest.mark.parametrize("kind", KINDS)
def test_cell_and_max_equal_the_exhaustive_scan_of_own_scores(product, kind):
    res, lut = product
    w = res[f"{kind}/1/weighted_f"]
    cell, mx = _grid_f32(w, lut)
    got_cell, got_mx = res[f"{kind}/1/cell"], res[f"{kind}/1/max_Lf"]
    assert got_cell.tolist() == cell.tolist()
    assert got_mx.tobytes() == mx.astype(np.float32).tobytes()
    for k in ("cell", "xy", "max_Lf"):  # the launch without score outputs: the same bytes
        assert res[f"{kind}/0/{k}"].tobytes() == res[f"{kind}/1/{k}"].tobytes(), k
    if kind in ("constant", "zero"):  # every tuple ties: cell 0's tuple
        assert (got_cell == 0).all() and (w == w[0, 0, 0]).all()
    if kind == "mixed_constant":
        assert (got_cell[1::2] == 0).all() and (got_cell[0::2] != 0).any()
    if kind == "click":  # a one-hot per live pair: L = 3 peaks where the lags form a grid tuple
        assert np.abs(res["click/1/lags"][0]).tolist() == [5, 9, 4]


CHILD = r"""
import sys
sys.path[:0] = {paths!r}
import numpy as np
from tdoa.localizer import Localizer
from test_gpu_p1k_prune import run_all
ph = Localizer(engine="gcc_phat")
assert ph.batch_kernel() == "k_p1k_lean", ph.batch_kernel()
np.savez({dump!r}, **run_all(ph))
ph.close()
print("exhaustive ok")
"""


@pytest.mark.skipif(not os.path.exists(AB_LIB), reason="tdoa/libtdoa_ab.so not built (make ab)")
def test_exhaustive_build_gives_the_same_bytes(product, tmp_path):
    """The 8-wave shape of the A/B library scans every tuple (a fresh child:
    the library reads TDOA_P1K once per process)."""
    dump = str(tmp_path / "lean8.npz")
    r = subprocess.run([sys.executable, "-c", CHILD.format(paths=PATHS, dump=dump)],
                       env=dict(os.environ, TDOA_LIB=AB_LIB, TDOA_P1K="lean8"), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "exhaustive ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    res, other = product[0], np.load(dump)
    assert sorted(res) == sorted(other.files)
    for name in res:
        assert res[name].dtype == other[name].dtype and res[name].tobytes() == other[name].tobytes(), name
