"""Numpy restatement of tdoa_peaks (include/tdoa.h), shared by the CPU and GPU
peak tests.  A helper module, not a conftest.

Per frame:
  1. L[c] = sum_p scores[p][lut[p][c]] in the block's own type (int64, or
     float32 with one rounded add per pair in ascending p, starting from 0);
  2. up to num_peaks times: the maximum L among the cells not yet suppressed,
     ties to the lowest cell.  Peak 0 is always reported; peak k >= 1 only if a
     cell remains and, for min_rel > 0, double(L_k) >= double(float32(min_rel))
     * double(L_0); the first peak not reported ends the search.  Then every
     cell within `radius` (Chebyshev) of the peak is suppressed.
Empty slots: cell -1, xy NaN, L INT64_MIN / Lf -inf, lags 0.
"""
import numpy as np

INT64_MIN = np.iinfo(np.int64).min


def l_map(scores: np.ndarray, lut: np.ndarray) -> np.ndarray:
    """[B][P][K] scores, [P][G] lut -> L [B][G] in the scores' dtype."""
    s = np.ascontiguousarray(scores)
    assert s.dtype in (np.int64, np.float32)
    B, P, _ = s.shape
    lut2 = np.asarray(lut).reshape(P, -1).astype(np.int64)
    L = np.zeros((B, lut2.shape[1]), s.dtype)
    for p in range(P):
        L += s[:, p][:, lut2[p]]  # stays in dtype: one add per pair
    return L


def peaks_from_map(L: np.ndarray, lut: np.ndarray, grid_W: int, half_w: int, half_h: int,
                   grid_scale: float, S: int, num_peaks: int, radius: int,
                   min_rel: float = 0.0) -> dict:
    B, G = L.shape
    P = lut.shape[0]
    lut2 = np.asarray(lut).reshape(P, -1).astype(np.int64)
    is_float = L.dtype == np.float32
    Kp = num_peaks
    out = {"count": np.zeros(B, np.int32),
           "cell": np.full((B, Kp), -1, np.int32),
           "xy": np.full((B, Kp, 2), np.nan, np.float32),
           "lags": np.zeros((B, Kp, P), np.int32)}
    val = np.full((B, Kp), -np.inf if is_float else INT64_MIN, L.dtype)
    cx_all, cy_all = np.arange(G) % grid_W, np.arange(G) // grid_W
    thr = float(np.float32(min_rel))
    sc = np.float32(grid_scale)
    for f in range(B):
        alive = np.ones(G, bool)
        for k in range(Kp):
            idx = np.flatnonzero(alive)
            if idx.size == 0:
                break
            c = int(idx[np.argmax(L[f, idx])])  # first maximum = lowest cell
            v = L[f, c]
            if k > 0 and thr > 0.0 and not (float(v) >= thr * float(L[f, out["cell"][f, 0]])):
                break
            out["cell"][f, k] = c
            val[f, k] = v
            cx, cy = c % grid_W, c // grid_W
            out["xy"][f, k] = (np.float32(cx - half_w) / sc, np.float32(half_h - cy) / sc)
            out["lags"][f, k] = lut2[:, c] - S
            out["count"][f] = k + 1
            alive &= ~((np.abs(cx_all - cx) <= radius) & (np.abs(cy_all - cy) <= radius))
    out["Lf" if is_float else "L"] = val
    return out


def peaks_ref(scores, lut, grid_W, half_w, half_h, grid_scale, S, num_peaks=2, radius=8,
              min_rel=0.0) -> dict:
    return peaks_from_map(l_map(scores, lut), lut, grid_W, half_w, half_h, grid_scale, S,
                          num_peaks, radius, min_rel)


def cheb(cell_a, cell_b, grid_W):
    """Chebyshev distance in cells between row-major cells (broadcasting)."""
    a, b = np.asarray(cell_a, np.int64), np.asarray(cell_b, np.int64)
    return np.maximum(np.abs(a % grid_W - b % grid_W), np.abs(a // grid_W - b // grid_W))


def both_found(true_cells, peak_cells, grid_W, within=8):
    """[B][ns] true cells, [B][Kp] reported cells (-1 = empty) -> bool [B]: every
    true cell has a reported peak within `within` cells."""
    t, pk = np.asarray(true_cells), np.asarray(peak_cells)
    d = cheb(t[:, :, None], np.maximum(pk, 0)[:, None, :], grid_W)
    d = np.where(pk[:, None, :] >= 0, d, np.iinfo(np.int64).max)
    return (d.min(-1) <= within).all(-1)


def assert_equal(got: dict, exp: dict, where=""):
    """Every field of exp equals got's bit for bit (NaN fills equal NaN)."""
    for k, e in exp.items():
        g = np.asarray(got[k])
        assert g.shape == e.shape and g.dtype == e.dtype, (where, k, g.shape, e.shape, g.dtype, e.dtype)
        same = (g == e) | ((g != g) & (e != e)) if e.dtype.kind == "f" else (g == e)
        assert same.all(), (where, k, np.argwhere(~same)[:4].tolist())


def two_source_case():
    """The two-source premise shared by the CPU and the GPU test: 8-mic circle,
    N = 2048, S = 46, 16 frames of two independent sources at least 25 cells
    apart, and the explicit Q15 window both tests use.
    Returns (frames int16 [16][8][2048], cells [16][2], lut [28][101*101], window int32 [2048], mics)."""
    import oracle as O
    from tdoa import synth
    mics = synth.circle_mics(8, 0.15)
    lut = O.build_lut(mics, max_shift=46).reshape(28, -1)
    fr, cells, _ = synth.multi_source_frames(16, 8, 2048, lut, 46, TWO_SOURCE_SEED, grid_W=101)
    return fr.numpy(), cells.numpy(), lut, two_source_window(2048), mics


TWO_SOURCE_SEED = 0x5EED0201


def two_source_window(N: int) -> np.ndarray:
    """The explicit Q15 window [N] of the two-source tests: the DPSS(NW=2) table
    a context of this frame length uses by default (tests/golden), passed to
    the oracle and, as window_q15=, to the GPU context."""
    import os
    here = os.path.dirname(os.path.abspath(__file__))
    w = np.load(os.path.join(here, "golden", "window_q15.npz"), allow_pickle=False)[f"n{N}"]
    return np.ascontiguousarray(w, dtype=np.int32)
