"""k_p1k_lean and k_p1k_pcm16 against the bytes their parent commit wrote
(tests/golden/p1k_parent_bytes.npz, recorded by tools/p1k_parent_bytes.py from
the library before the kernels' LDS reads were moved: DESIGN.md "k_p1k_lean").

Moving when a table or tile value is requested, and how it is waited for,
changes no float operation, operand order or association, so every output of
every case is the same bytes: lags, gate, cell, xy, max_Lf compared whole,
scores_f and weighted_f by the SHA-256 of their bytes.  Cases (the tool's):
both sample formats, two PHAT floors, batches of 1, 2, 7, 8, 9 and 17 frames
of ADC-like, full-range, all-zero and click frames.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import p1k_parent_bytes as PB  # noqa: E402


@pytest.fixture(scope="module")
def now():
    return PB.run()


def test_the_golden_file_is_small_and_complete():
    assert os.path.getsize(PB.GOLDEN) < 100 * 1024
    g = np.load(PB.GOLDEN)
    want = {f"{e}/{f}/{B}/{k}" for e in PB.FLOORS for f in PB.FORMATS for B in PB.BATCHES for k in PB.KEYS}
    assert set(g.files) == want


@pytest.mark.parametrize("fmt", sorted(PB.FORMATS))
@pytest.mark.parametrize("eps", PB.FLOORS)
def test_every_output_byte_is_the_parents(now, eps, fmt):
    g = np.load(PB.GOLDEN)
    for B in PB.BATCHES:
        for k in PB.KEYS:
            name = f"{eps}/{fmt}/{B}/{k}"
            x, y = g[name], now[name]
            assert x.dtype == y.dtype and x.shape == y.shape, name
            assert x.tobytes() == y.tobytes(), (name, np.argwhere(x != y)[:4].tolist())
    # the cases are live: the first click frame (pool index 3) answers its
    # delay differences, and the all-zero frame (index 2) has the zero lag row
    # the prior's centre picks (every score 0)
    assert np.abs(now[f"{eps}/{fmt}/7/lags"][3]).tolist() == [5, 9, 4]
    assert now[f"{eps}/{fmt}/7/max_Lf"][2] == 0
