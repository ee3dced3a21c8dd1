"""Multi-source peak extraction, CPU side: the numpy restatement of tdoa_peaks
(tests/peaks_ref.py) on hand-made maps with known answers, the frame
generator synth.multi_source_frames, and the two-source premise of the GPU
test on the float64 GCC-PHAT oracle."""
import numpy as np
import pytest

import peaks_ref as R

INT64_MIN = np.iinfo(np.int64).min


def _one_pair(Lmap, dtype=np.int64):
    """A [1][1][K] score block and a [1][G] LUT whose L map is Lmap: cell c reads lag c."""
    Lmap = np.asarray(Lmap, dtype).reshape(-1)
    return Lmap.reshape(1, 1, -1).copy(), np.arange(Lmap.size, dtype=np.uint8).reshape(1, -1)


def _ref(Lmap, W, H, dtype=np.int64, **kw):
    sc, lut = _one_pair(Lmap, dtype)
    S = (sc.shape[2] - 1) // 2
    return R.peaks_ref(sc, lut, W, (W - 1) // 2, (H - 1) // 2, 2.0, S, **kw), S


@pytest.mark.parametrize("dtype", [np.int64, np.float32])
def test_two_separated_maxima_on_3x5(dtype):
    m = np.array([[1, 2, 1, 0, 3],
                  [9, 2, 1, 4, 7],
                  [1, 2, 1, 0, 3]])
    r, S = _ref(m, 5, 3, dtype, num_peaks=2, radius=1)
    assert r["count"].tolist() == [2]
    assert r["cell"].tolist() == [[5, 9]]
    assert r["L" if dtype == np.int64 else "Lf"].tolist() == [[9, 7]]
    # xy = ((cx - half_w) / scale, (half_h - cy) / scale), scale 2
    assert r["xy"].tolist() == [[[-1.0, 0.0], [1.0, 0.0]]]
    assert r["lags"].tolist() == [[[5 - S], [9 - S]]]
    # a third peak: what is left outside both squares is column 2; its maximum 1
    # first occurs in row 0
    r3, _ = _ref(m, 5, 3, dtype, num_peaks=3, radius=1)
    assert r3["cell"].tolist() == [[5, 9, 2]] and r3["count"].tolist() == [3]
    # radius 0 suppresses the peak's own cell only: the next two largest follow
    r0, _ = _ref(m, 5, 3, dtype, num_peaks=3, radius=0)
    assert r0["cell"].tolist() == [[5, 9, 8]]


def test_all_equal_map_walks_the_squares():
    # 7 x 7, radius 1: peak 0 is cell 0 and clears x, y <= 1; the first row-major
    # cell left is (2, 0); its square clears x in 1..3, y <= 1; then (4, 0), (6, 0),
    # and with row 0 and 1 gone, (0, 2)
    r, _ = _ref(np.full(49, 5), 7, 7, num_peaks=5, radius=1)
    assert r["cell"].tolist() == [[0, 2, 4, 6, 14]]
    assert r["count"].tolist() == [5]
    assert r["L"].tolist() == [[5] * 5]


def test_radius_covering_the_grid_leaves_one_peak():
    m = np.arange(15)[::-1].copy()
    r, _ = _ref(m, 5, 3, num_peaks=4, radius=4)
    assert r["count"].tolist() == [1]
    assert r["cell"].tolist() == [[0, -1, -1, -1]]
    assert r["L"].tolist() == [[14, INT64_MIN, INT64_MIN, INT64_MIN]]
    assert np.isnan(r["xy"][0, 1:]).all() and not np.isnan(r["xy"][0, 0]).any()
    assert (r["lags"][0, 1:] == 0).all()
    rf, _ = _ref(m, 5, 3, np.float32, num_peaks=2, radius=4)
    assert rf["Lf"][0, 1] == -np.inf and rf["cell"].tolist() == [[0, -1]]


def test_min_rel_cuts_at_the_second_peak():
    m = np.array([[100, 0, 0, 0, 60],
                  [0, 0, 0, 0, 0],
                  [0, 0, 49, 0, 0]])
    keep, _ = _ref(m, 5, 3, num_peaks=3, radius=0, min_rel=0.5)
    assert keep["count"].tolist() == [2] and keep["cell"].tolist() == [[0, 4, -1]]
    cut, _ = _ref(m, 5, 3, num_peaks=3, radius=0, min_rel=0.7)
    assert cut["count"].tolist() == [1] and cut["cell"].tolist() == [[0, -1, -1]]
    # the first rejected peak ends the search, and <= 0 means no threshold
    none, _ = _ref(m, 5, 3, num_peaks=3, radius=0, min_rel=0.0)
    assert none["cell"].tolist() == [[0, 4, 12]]
    # equality passes: 0.5 * 100 <= 50
    m[0, 4] = 50
    eq, _ = _ref(m, 5, 3, num_peaks=2, radius=0, min_rel=0.5)
    assert eq["count"].tolist() == [2]


def test_float_map_adds_pairs_in_order():
    """Two or more pairs: float32 L is ((0 + s0) + s1) + s2, one rounding per add."""
    s = np.array([[[1e8, 0.0]], [[3.0, 0.0]], [[-1e8, 0.0]]], np.float32).reshape(1, 3, 2)
    lut = np.zeros((3, 4), np.uint8)
    L = R.l_map(s, lut)
    assert L.dtype == np.float32 and (L == np.float32(np.float32(1e8) + np.float32(3.0)) - np.float32(1e8)).all()


def test_multi_source_frames_contract(oracle):
    from tdoa import synth
    mics = synth.circle_mics(8, 0.15)
    lut = oracle.build_lut(mics, max_shift=46)  # [P][H][W]
    fr, cells, tau = synth.multi_source_frames(12, 8, 512, lut, 46, 7, num_sources=3, min_sep=20)
    assert fr.dtype.is_floating_point is False and tuple(fr.shape) == (12, 8, 512)
    assert tuple(cells.shape) == (12, 3) and tuple(tau.shape) == (12, 3, 8)
    assert int(fr.min()) >= 0 and int(fr.max()) <= 255
    c = cells.numpy()
    for a in range(3):
        for b in range(a + 1, 3):
            assert (R.cheb(c[:, a], c[:, b], 101) >= 20).all()
    l2 = lut.reshape(28, -1).astype(np.int64)
    assert (tau.numpy()[:, :, 0] == 0).all()
    for m in range(1, 8):
        assert (tau.numpy()[:, :, m] == l2[m - 1][c] - 46).all()
    again = synth.multi_source_frames(12, 8, 512, lut, 46, 7, num_sources=3, min_sep=20)
    assert (again[0] == fr).all() and (again[1] == cells).all()
    # a single source placed like adc_frames' is found by cross-correlating the mics
    one, c1, t1 = synth.multi_source_frames(2, 8, 512, lut, 46, 9, num_sources=1, noise_std=0.5)
    x = one.numpy().astype(np.float64) - 128.0
    for f in range(2):
        d = int(t1[f, 0, 3])
        lags = np.arange(-46, 47)
        cc = [np.dot(x[f, 0, 46:-46], np.roll(x[f, 3], -s)[46:-46]) for s in lags]
        assert lags[int(np.argmax(cc))] == d


def test_two_source_premise_on_the_oracle(oracle):
    """Raw GCC-PHAT scores keep both sources: the top two peaks (radius 8) lie
    within 8 cells of the two true cells on every one of the 16 frames.  The
    weighted scores (the Gaussian lag prior around each pair's best lag) do
    not -- by design of the reference's display."""
    import gcc_phat_oracle as G
    fr, cells, lut, win, _ = R.two_source_case()
    assert fr.shape == (16, 8, 2048) and (R.cheb(cells[:, 0], cells[:, 1], 101) >= 25).all()
    o = G.gcc_phat_batch(fr, 46, win)
    pk = R.peaks_ref(o["scores_f"].astype(np.float32), lut, 101, 50, 50, 24.0, 46, num_peaks=2, radius=8)
    assert (pk["count"] == 2).all()
    found = R.both_found(cells, pk["cell"], 101, within=8)
    assert found.all(), np.flatnonzero(~found).tolist()
    pw = R.peaks_ref(o["weighted_f"].astype(np.float32), lut, 101, 50, 50, 24.0, 46, num_peaks=2, radius=8)
    assert not R.both_found(cells, pw["cell"], 101, within=8).all()
