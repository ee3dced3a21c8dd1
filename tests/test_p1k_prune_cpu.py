"""k_p1k_lean's pruned grid scan on the CPU (DESIGN.md "k_p1k_lean", tests/prune_ref.py).

  * the row table the library builds (tdoa_p1k_prune_section, read back through
    tools/tables_dump: the host-only build of csrc/tdoa_tables.cpp) equals the
    documented rule restated in numpy from the LUT, is a permutation of the
    distinct tuples with their first cells, and every row's [lo, hi] covers its
    tuples; a table of more than 64 rows has none;
  * the as-built search in numpy (same table, bound, order, tie rule, float32)
    gives the exhaustive float32 scan's cell and max L bit for bit on synthetic
    scores: peaked, flat noise, all equal, all negative (the max(., 0) term),
    exact ties planted in two different rows, +-inf, NaN in one pair, and waves
    that mix a peaked frame with a constant or a noisy one;
  * the bound is never below the L of a tuple in its row;
  * a condition on pruning power: on the benchmark's frames at most 6 rows on
    average keep a bound >= the final best (union over a wave's two frames).
"""
import os

import numpy as np
import pytest

import prune_ref as R
from conftest import GOLDEN
from test_tables_cpu import CONFIGS, TOOL, run_tool, tools  # noqa: F401  (tools: the fixture that builds the tool)

F32 = np.float32
K = 93  # the default config: S = 46


@pytest.fixture(scope="module")
def dumped(tools, tmp_path_factory):  # noqa: F811
    """name -> (lut, tuples [3][U], first cells, the library's section words), never modified."""
    tmp = str(tmp_path_factory.mktemp("prune"))
    res = {}
    for name in ("default", "near_wide", "triangle2_s63"):
        _, out, r = run_tool(tools[0], tmp, name, CONFIGS[name])
        assert r.returncode == 0, r.stdout + r.stderr
        rd = lambda f, dt: np.fromfile(os.path.join(out, f + ".bin"), dt)  # noqa: E731
        lut, tup, cell = rd("lut", np.uint8), rd("tuples", np.uint32), rd("tuple_cell", np.int32)
        T = np.stack([(tup >> (8 * p)) & 0xFF for p in range(3)]).astype(np.int64)
        res[name] = (lut, T, cell.astype(np.int64), rd("p1k_prune", np.uint32))
    return res


@pytest.fixture(scope="module")
def tab(dumped):
    t = R.parse_section(dumped["default"][3])
    for v in t.values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return t


@pytest.mark.parametrize("name", ["default", "near_wide"])
def test_row_table_is_the_documented_rule(dumped, name):
    lut, T, cell, words = dumped[name]
    T2, cell2 = R.distinct_tuples(lut)
    assert np.array_equal(T, T2) and np.array_equal(cell, cell2)
    got, want = R.parse_section(words), R.row_table(T, cell)
    assert sorted(got) == sorted(want)
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    U, rows, p = T.shape[1], got["rows"], got["pair"]
    assert rows == -(-U // 64) and got["U"] == U and got["cell0"] == cell[0] == 0
    # a permutation of the distinct tuples, each with its own first cell
    key = lambda t: (t[0] << 16) | (t[1] << 8) | t[2]  # noqa: E731
    cell_of = dict(zip(key(T).tolist(), cell.tolist()))
    real = got["cells"] != R.INT_MAX
    assert real.sum() == U and real[:U].all()
    assert sorted(key(got["tuples"][:, :U]).tolist()) == sorted(cell_of)
    assert [cell_of[k] for k in key(got["tuples"][:, :U]).tolist()] == got["cells"][:U].tolist()
    assert (got["tuples"][:, U:] == 127).all()
    # sorted by the pair's slot, ties in first-cell order; rows covered by [lo, hi]
    s = got["tuples"][p, :U]
    assert (np.diff(s) >= 0).all()
    assert (np.diff(got["cells"][:U])[np.diff(s) == 0] > 0).all()
    for r in range(rows):
        sr = s[64 * r:64 * r + 64]
        assert got["lo"][r] == sr.min() and got["hi"][r] == sr.max()
    assert got["width"] == (got["hi"] - got["lo"] + 1).max()
    if name == "default":
        assert (U, rows) == (2469, 39) and got["width"] <= 4


def test_more_than_64_rows_have_no_table(dumped):
    _, T, _, words = dumped["triangle2_s63"]
    assert T.shape[1] == 6510 and words.size == 0 and R.row_table(T, np.arange(6510)) is None


def _peaked(rng, n, T, K=K):
    """n frames of [3][K] scores: a bump of the lag prior's shape around a grid tuple, plus noise."""
    k = np.arange(K)
    c = T[:, rng.integers(0, T.shape[1], n)].T + rng.integers(-1, 2, (n, 3))
    amp = rng.uniform(0.05, 0.4, (n, 3, 1))
    return (amp * np.exp(-(k - c[..., None]) ** 2 / 36.0) + rng.normal(0, 4e-3, (n, 3, K))).astype(F32)


def _cases(T, tab, K=K):
    """kind -> [48][3][K] float32 scores for the table `tab` of the tuples T.  K: the lag
    slots per pair (the module's 93 by default); the planted +-inf / NaN slots keep
    their share of the range, 19..73 at K = 93.  A one-row table has no "planted_ties"."""
    rng = np.random.default_rng(0x9121)
    n = 48
    lo, hi = K * 19 // 93, K * 74 // 93
    noise = lambda m=n: rng.normal(0, 5e-3, (m, 3, K)).astype(F32)  # noqa: E731
    peaked = _peaked(rng, n, T, K)
    const = np.full((n, 3, K), 0.25, F32)
    c = {"peaked": peaked, "flat_noise": noise(), "all_equal": const,
         "all_negative": (-rng.uniform(0.01, 1.0, (n, 3, K))).astype(F32),
         "all_negative_peaked": (peaked - F32(1.0)).astype(F32)}
    # exact ties: every score -1 but the slots of two tuples from different rows (0: sums are exact)
    ties = np.full((n, 3, K), -1.0, F32)
    for f in range(n if tab["rows"] >= 2 else 0):
        ra, rb = rng.choice(tab["rows"], 2, replace=False)
        for r in (ra, rb):
            u = 64 * r + rng.integers(0, min(64, tab["U"] - 64 * r))
            ties[f, np.arange(3), tab["tuples"][:, u]] = 0.0
    if tab["rows"] >= 2:
        c["planted_ties"] = ties
    inf = peaked.copy()
    for f in range(n):
        inf[f, rng.integers(0, 3), rng.integers(lo, hi, 3)] = np.inf if f % 3 else -np.inf
        if f % 4 == 0:
            inf[f, rng.integers(0, 3), rng.integers(lo, hi, 2)] = -np.inf
    c["inf"] = inf
    nan = peaked.copy()
    for f in range(n):
        q = rng.integers(0, 3)
        if f % 4 == 3:
            nan[f, q] = np.nan  # every L is NaN: tuple 0, -inf
        else:
            nan[f, q, rng.integers(lo, hi, 1 + f % 6)] = np.nan
    c["nan_one_pair"] = nan
    mixed = peaked.copy()
    mixed[1::4] = const[1::4]
    mixed[3::4] = noise()[3::4]
    c["mixed_waves"] = mixed
    return c


@pytest.fixture(scope="module")
def cases(dumped, tab):
    return _cases(dumped["default"][1], tab)


NAMES = ["peaked", "flat_noise", "all_equal", "all_negative", "all_negative_peaked", "planted_ties", "inf",
         "nan_one_pair", "mixed_waves"]


@pytest.mark.parametrize("name", NAMES)
def test_model_equals_the_exhaustive_scan(dumped, tab, cases, name):
    _, T, cell, _ = dumped["default"]
    w = cases[name]
    ecell, emx = R.exhaustive(w, T, cell)
    scanned = []
    for v in range(0, len(w), 2):
        c, mx, nrow = R.pruned_wave(w[v:v + 2], tab)
        assert c.tolist() == ecell[v:v + 2].tolist(), (name, v)
        assert mx.tobytes() == emx[v:v + 2].tobytes(), (name, v, mx, emx[v:v + 2])
        scanned.append(nrow)
    print(f"{name}: rows scanned per wave mean {np.mean(scanned):.2f} max {max(scanned)} of {tab['rows']}")
    if name == "all_equal":  # every tuple ties: cell 0's tuple, and nothing is pruned (the exhaustive fallback)
        assert (ecell == 0).all() and min(scanned) == tab["rows"]
    if name == "peaked":  # both passes run on some wave, without the fallback
        assert 2 < max(scanned) < tab["rows"]
    if name == "all_negative":  # the bound's other terms are 0, not the (negative) maxima
        assert (R.bound_terms(w) == 0).all() and (emx < 0).all()
    if name == "planted_ties":  # several tuples reach 0, in different rows; the first cell wins
        L = R._L(R._table128(w), tab["tuples"])
        rows_at_max = [len(set((np.nonzero(L[f] == 0)[0] // 64).tolist())) for f in range(len(w))]
        assert (emx == 0).all() and min(rows_at_max) >= 2
        assert all(ecell[f] == tab["cells"][L[f] == 0].min() for f in range(len(w)))
    if name == "nan_one_pair":
        assert (ecell[3::4] == 0).all() and np.isneginf(emx[3::4]).all() and np.isfinite(emx[0::4]).all()


@pytest.mark.parametrize("name", NAMES)
def test_bound_is_not_below_any_tuple_of_its_row(tab, cases, name):
    w = cases[name]
    b = R.row_bounds(w, tab)
    L = R._L(R._table128(w), tab["tuples"]).reshape(len(w), tab["rows"], 64)
    with np.errstate(invalid="ignore"):
        below = b[:, :, None] < L  # NaN on either side: False, and such a row is never skipped
    assert not below.any()


def test_pruning_power_on_the_benchmark_frames(dumped, tab):
    """A condition, not a measurement: rows whose bound is >= the final best,
    as the union over the frame pairs (2w, 2w+1), on 1024 of bench.py's
    config-2 frames with the float64 oracle's weighted scores cast to float32."""
    import gcc_phat_oracle as G
    from tdoa import synth
    lut, T, cell, _ = dumped["default"]
    z = np.load(os.path.join(GOLDEN, "window_q15.npz"))
    win = [z[k] for k in z.files if z[k].shape == (1024,)][0]
    fr = synth.adc_frames(1024, 3, 1024, lut.reshape(3, 101, 101), 46, 0x5EED0002)[0].numpy()
    exp = G.gcc_phat_batch(fr, 46, win, lut.reshape(3, 101, 101))
    w = exp["weighted_f"].astype(F32)
    M = np.fmax(exp["scores_f"].astype(F32).max(-1), F32(0))  # the kernel's term: max(raw maximum, 0)
    assert (M >= w.max(-1)).all()
    best = R.exhaustive(w, T, cell)[1]
    alive = R.row_bounds(w, tab, M) >= best[:, None]
    kept = alive.reshape(-1, 2, tab["rows"]).any(1).sum(1)
    scanned = [R.pruned_wave(w[v:v + 2], tab, M[v:v + 2])[2] for v in range(0, 1024, 2)]
    print(f"sort pair {tab['pair']}, {tab['rows']} rows: bound >= final best in {kept.mean():.2f} rows per wave "
          f"(p99 {np.percentile(kept, 99):.0f}, max {kept.max()}); as built {np.mean(scanned):.2f} rows scanned "
          f"(p99 {np.percentile(scanned, 99):.0f}, max {max(scanned)})")
    assert kept.mean() <= 6
