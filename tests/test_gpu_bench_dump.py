"""bench.py --dump-outputs: the files hold what the last timed step computed.

A plain config-2 run (no --full) with 6 timed steps over 2 rotating batches and
2 step streams: the last step launches batch 1 into the second stream's output
buffers.  The dumped arrays must equal, bit for bit, what Localizer.localize
returns for that batch regenerated from its seed, each as float32 (float
outputs) or float64 (integer outputs), one file per output and no others.
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import ROOT  # noqa: E402
from tdoa import shard  # noqa: E402
from tdoa.localizer import Localizer  # noqa: E402

sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_dump_is_the_last_timed_steps_outputs(tmp_path):
    old = sys.argv
    sys.argv = ["bench.py", "--steps", "6", "--warmup", "2", "--rotate-mib", "32", "--preflight-s", "0",
                "--dump-outputs", str(tmp_path / "dump")]
    try:
        args = bench.parse()
    finally:
        sys.argv = old
    dev = torch.device("cuda", 0)
    res = bench.time_engine("gcc_phat", args, dev, shard.rank_info(), {})
    assert (res["rotate_batches"], res["streams"]) == (2, 2)
    assert res["ms_per_step"] > 0 and "parity" not in res and res["gpu_clock_mhz"] is None

    loc = Localizer(engine="gcc_phat", device=0)
    # step 5 of 6 launches entry 5 % 4 = 1 of the 4 prepared launches: batch 1
    fr, _ = bench.make_frames(4096, 3, 1024, loc.lut().reshape(loc.dims.P, -1), loc.dims.S,
                              shard.frame_seed(0x5EED0002, 0, 1), dev)
    exp = {k: v.cpu().numpy() for k, v in loc.localize(fr).items()}
    loc.close()
    assert sorted(os.listdir(tmp_path / "dump")) == sorted(k + ".npy" for k in exp)
    for k, v in exp.items():
        got = np.load(tmp_path / "dump" / f"{k}.npy")
        assert got.dtype == (np.float32 if v.dtype == np.float32 else np.float64), k
        assert got.shape == v.shape and np.array_equal(got, v), k
