"""The geometry sweep on the CPU (tests/grid_geometry_cases.py; the GPU half is
tests/test_gpu_grid_geometry.py).

  * every case's host tables, through tools/tables_dump (the host-only build of
    csrc/tdoa_tables.cpp): W, H, S, K, U, NT, the wide flag and the parsed
    p1k_prune section (rows, sort pair, widest row) equal the case table, so a
    drift in the table builder fails here and does not silently move a GPU case
    onto another branch of a kernel;
  * across the set, the branches the cases were chosen for are present;
  * the numpy model of k_p1k_lean's pruned search (tests/prune_ref.py) on every
    3 x 1024 case's own row table equals the exhaustive float32 scan bit for
    bit, on the score kinds of tests/test_p1k_prune_cpu.py, and no row's bound
    is below the L of one of its tuples;
  * the GPU module's inputs on the references alone: the float64 oracle's
    margins exclude nothing, the mirror cells are a known answer on both
    oracles, the two-trip frames defeat a one-trip bound in the numpy model, and
    the streaming captures drop no stream and skip no cell;
  * the LUT of every case is the oracle's at the case's geometry, and the
    sanitized tools/tables_dump_san (nothing preloaded) is clean on the cases
    and gives the same scalars.
"""
import json
import os

import numpy as np
import pytest

import band_ref
import grid_geometry_cases as GC
import prune_ref as R
from test_p1k_prune_cpu import _cases
from test_tables_cpu import run_tool, tools  # noqa: F401  (tools: the fixture that builds the tool)


@pytest.fixture(scope="module")
def dumped(tools, tmp_path_factory):  # noqa: F811
    """name -> (scalars, lut, tuples [3][U] or None, first cells, parsed prune section or None), never modified."""
    tmp = str(tmp_path_factory.mktemp("geometry"))
    res = {}
    for name in GC.CASES:
        _, out, r = run_tool(tools[0], tmp, name, GC.config_overrides(name))
        assert r.returncode == 0, (name, r.stdout + r.stderr)
        meta = json.loads(r.stdout)
        rd = lambda f, dt: np.fromfile(os.path.join(out, f + ".bin"), dt)  # noqa: E731
        lut, tup, cell = rd("lut", np.uint8), rd("tuples", np.uint32), rd("tuple_cell", np.int32)
        T = tab = None
        if name in GC.P1K_SHAPED:
            T = np.stack([(tup >> (8 * p)) & 0xFF for p in range(3)]).astype(np.int64)
            tab = R.parse_section(rd("p1k_prune", np.uint32))
        for a in (lut, T, cell) + tuple(v for v in (tab or {}).values() if isinstance(v, np.ndarray)):
            if a is not None:
                a.flags.writeable = False
        res[name] = (meta, lut, T, cell.astype(np.int64), tab)
    return res


@pytest.mark.parametrize("name", list(GC.CASES))
def test_case_tables_are_as_recorded(dumped, oracle, name):
    c = GC.CASES[name]
    m, lut, T, cell, tab = dumped[name]
    hw, hh, scale, height, speed, fs = GC.geometry(name)
    assert (m["W"], m["H"], m["S"], m["K"], m["U"]) == (c["W"], c["H"], c["S"], c["K"], c["U"])
    assert (m["W"], m["H"], m["G"]) == (2 * hw + 1, 2 * hh + 1, c["W"] * c["H"]) and m["NT"] > 0
    assert m["K"] == 2 * m["S"] + 1 and m["S"] == (c["kw"].get("max_shift") or fs * 32 // 34300)
    if c["wide"] is not None:
        assert m["wide"] == c["wide"]
    if c["rows"] is not None:
        assert tab is not None and (tab["rows"], tab["U"]) == (c["rows"], c["U"]) and c["rows"] == -(-c["U"] // 64)
    if c["pair"] is not None:
        assert (tab["pair"], tab["width"]) == (c["pair"], c["width"])
        assert tab["width"] == (tab["hi"] - tab["lo"] + 1).max()
        # the rule of the row table, restated from the tuples alone (tests/prune_ref.py row_table)
        want = R.row_table(T, cell)
        for k in want:
            assert np.array_equal(tab[k], want[k]), k
    # the LUT is the oracle's at this geometry
    mics = c["kw"].get("mic_xy")
    exp = oracle.build_lut(oracle.microphones_ref() if mics is None else mics, hw, hh, scale, height, speed, fs, m["S"])
    assert lut.tobytes() == np.ascontiguousarray(exp, np.uint8).tobytes()


def test_the_cases_reach_the_intended_branches(dumped):
    tabs = {n: dumped[n][4] for n in GC.LEAN_CASES}
    assert all(t is not None for t in tabs.values())
    # the bound loop of k_p1k_lean steps 4 lags per trip: 2 trips, and 4
    assert any(4 < t["width"] <= 8 for t in tabs.values()) and any(t["width"] > 12 for t in tabs.values())
    assert any(t["pair"] != 0 for t in tabs.values()) and any(t["pair"] == 0 for t in tabs.values())
    assert any(t["rows"] == 1 for t in tabs.values())
    assert any(t["U"] % 64 == 0 for t in tabs.values())
    for n in ("s63_65", "s63_141x45"):
        # 40 rows, the most that k_p1k_lean stages, at K = 127: the score table's slot 126 lies beside
        # the -inf padding slot 127
        assert tabs[n]["rows"] == 40 and dumped[n][0]["K"] == 127 == R.KPAD - 1
    assert tabs["s63_141x45"]["U"] == 40 * 64 and (tabs["s63_141x45"]["cells"] != R.INT_MAX).all()
    # tdoa_phat1024_fits (GC.p1k_fits has the byte arithmetic): 8 x 16896 B of tiles + 16896 + 4 Upad + 64
    # <= 160 KiB, so Upad <= 2560.  40 rows: 135168 + 16896 + 10240 + 64 = 162368, fits; 41 rows
    # (Upad 3072): 164416 > 163840, and every larger table of the set: no k_p1k_lean.  A section exists
    # for each of them (<= 64 rows); it is the LDS rule that sends them to the generic fused kernel
    assert GC.p1k_fits(2560) and not GC.p1k_fits(2561) and GC.p1k_fits(1) and not GC.p1k_fits(3771)
    for n in GC.P1K_SHAPED:
        assert dumped[n][4] is not None and dumped[n][4]["rows"] <= 64
        assert (GC.CASES[n]["kernel"] == GC.LEAN) == GC.p1k_fits(dumped[n][0]["U"]), n
        assert GC.CASES[n]["kernel"] in (GC.LEAN, GC.FUSED_1024) and GC.CASES[n]["fused"]
    assert dumped["s63_143x45"][4]["rows"] == 41 and dumped["s63_full"][4]["rows"] == 59
    assert dumped["s63_full"][0]["U"] != 6510
    # k_grid_bb: partial 8 x 8 blocks in both directions, one lone partial tile, and the wide fallback
    for n in ("sq4_wide", "sq4_tall", "c8_wide"):
        m = dumped[n][0]
        assert m["W"] != m["H"] and m["W"] % 8 and m["H"] % 8 and m["wide"] == 0 and m["NT"] > 1
    assert dumped["sq4_wide"][0]["NT"] == 77 and dumped["c8_wide"][0]["P"] == 28
    assert dumped["c8_7x3"][0]["NT"] == 1 and dumped["c8_7x3"][0]["U"] < 64
    assert dumped["sq4_rect18"][0]["wide"] == 1 and dumped["n512_tall18"][0]["N"] == 512


@pytest.fixture(scope="module")
def scores(dumped):
    """name -> kind -> [48][3][K] float32 scores for the case's own table (test_p1k_prune_cpu._cases)."""
    res = {}
    for n in GC.P1K_SHAPED:
        m, _, T, _, tab = dumped[n]
        res[n] = _cases(T, tab, m["K"])
        for v in res[n].values():
            v.flags.writeable = False
    return res


@pytest.mark.parametrize("name", GC.P1K_SHAPED)
def test_model_equals_the_exhaustive_scan_on_the_case_table(dumped, scores, name):
    m, _, T, cell, tab = dumped[name]
    kinds = scores[name]
    assert ("planted_ties" in kinds) == (tab["rows"] >= 2) and len(kinds) == 8 + (tab["rows"] >= 2)
    for kind, w in kinds.items():
        assert w.shape == (48, 3, m["K"])
        ecell, emx = R.exhaustive(w, T, cell)
        scanned = []
        for v in range(0, len(w), 2):
            c, mx, nrow = R.pruned_wave(w[v:v + 2], tab)
            assert c.tolist() == ecell[v:v + 2].tolist(), (name, kind, v)
            assert mx.tobytes() == emx[v:v + 2].tobytes(), (name, kind, v, mx, emx[v:v + 2])
            scanned.append(nrow)
        if kind == "all_equal":  # every tuple ties: cell 0's tuple
            assert (ecell == 0).all()
        if kind == "planted_ties":
            assert (emx == 0).all()
        # the bound is never below the L of a tuple of its row
        b = R.row_bounds(w, tab)
        L = R._L(R._table128(w), tab["tuples"]).reshape(len(w), tab["rows"], 64)
        with np.errstate(invalid="ignore"):
            below = b[:, :, None] < L  # NaN on either side: False, and such a row is never skipped
        assert not below.any(), (name, kind)
    print(f"{name}: {tab['rows']} rows, pair {tab['pair']}, width {tab['width']}: model == exhaustive on "
          f"{len(kinds)} kinds")


def test_two_trip_frames_need_the_second_trip(dumped):
    """GC.TWO_TRIPS on the float64 oracle and the numpy model: the answer is the cell whose sort-pair
    slot lies at lo + 4 of its row, by a wide margin; the as-built search finds it, and the same
    search with a bound over the first four lags of a row only answers the decoy cell, every time."""
    import gcc_phat_oracle as G
    sp = GC.TWO_TRIPS
    name, c = sp["case"], GC.CASES[sp["case"]]
    hw, hh, scale = GC.geometry(name)[:3]
    m, flat, T, cell, tab = dumped[name]
    lut = _lut(dumped, name)
    l3 = flat.reshape(3, -1).astype(np.int64)
    assert tuple(l3[:, sp["cell"]]) == sp["tuple"] and tuple(l3[:, sp["decoy"]]) == sp["decoy_tuple"]
    p, at = tab["pair"], {int(cl): i for i, cl in enumerate(tab["cells"][:tab["U"]])}
    ra, rb = at[sp["cell"]] // 64, at[sp["decoy"]] // 64
    assert ra != rb and sp["tuple"][p] >= tab["lo"][ra] + 4 and tab["width"] <= 8
    assert [q for q in range(3) if sp["tuple"][q] != sp["decoy_tuple"][q]] == [p]
    fr = GC.two_trip_frames()
    exp = G.gcc_phat_batch(fr, c["S"], band_ref.window_q15(1024), lut, half_w=hw, half_h=hh, grid_scale=scale)
    srt = np.sort(exp["scores_f"], -1)
    top = exp["L"].max(-1)
    second = np.where(exp["L"] >= top[:, None] - 1e-12, -np.inf, exp["L"]).max(-1)
    assert (exp["cell"] == sp["cell"]).all() and (exp["lags"] == np.array(sp["tuple"]) - c["S"]).all()
    assert (srt[..., -1] - srt[..., -2]).min() > 0.05 and (top - second).min() > 0.05
    w = exp["weighted_f"].astype(np.float32)
    M = np.fmax(exp["scores_f"].astype(np.float32).max(-1), np.float32(0))  # the kernel's term: max(raw maximum, 0)
    one_trip = dict(tab, hi=np.minimum(tab["hi"], tab["lo"] + 3))
    for v in range(0, len(fr), 2):
        assert R.pruned_wave(w[v:v + 2], tab, M[v:v + 2])[0].tolist() == [sp["cell"]] * 2
        assert R.pruned_wave(w[v:v + 2], one_trip, M[v:v + 2])[0].tolist() == [sp["decoy"]] * 2


def _lut(dumped, name):
    c = GC.CASES[name]
    return dumped[name][1].reshape(-1, c["H"], c["W"])


@pytest.mark.parametrize("name", list(GC.CASES))
def test_the_oracle_alone_excludes_nothing(dumped, name):
    """The GPU test's frames on the float64 oracle alone: every (frame, pair) has a top-2 score
    margin above 2e-4, every frame a cell margin above 1e-3, and the frames use >= 4 cells."""
    import gcc_phat_oracle as G
    c = GC.CASES[name]
    hw, hh, scale = GC.geometry(name)[:3]
    lut = _lut(dumped, name)
    fr = GC.adc_batch(name, lut).numpy()
    exp = G.gcc_phat_batch(fr, c["S"], band_ref.window_q15(fr.shape[2]), lut, half_w=hw, half_h=hh, grid_scale=scale)
    srt = np.sort(exp["scores_f"], -1)
    top = exp["L"].max(-1)
    second = np.where(exp["L"] >= top[:, None] - 1e-12, -np.inf, exp["L"]).max(-1)
    assert (srt[..., -1] - srt[..., -2]).min() > 2e-4 and (top - second).min() > 1e-3
    assert len(set(exp["cell"].tolist())) >= (4 if lut[0].size > 1 else 1)
    assert (exp["xy"] == GC.closed_form_xy(exp["cell"], hw, hh, scale)).all()


@pytest.mark.parametrize("name", list(GC.MIRROR))
def test_mirror_cells_are_a_known_answer(dumped, oracle, name):
    """The preconditions of the asymmetric known answer, and the answer itself on both oracles."""
    import gcc_phat_oracle as G
    import known_answer as KA
    c = GC.CASES[name]
    hw, hh, scale = GC.geometry(name)[:3]
    S, lut = c["S"], _lut(dumped, name)
    l3 = lut.reshape(3, -1).astype(np.int64)
    cells, xy = GC.mirror_cells(name)
    assert c["W"] != c["H"] and (cells >= 0).all() and (cells < l3.shape[1]).all() and cells[0] != cells[1]
    assert (GC.closed_form_xy(cells, hw, hh, scale) == xy).all() and (xy[0] == xy[1][::-1]).all()
    assert (l3[:, cells[0]] != l3[:, cells[1]]).any()
    for cell in cells:
        same = (l3 == l3[:, cell:cell + 1]).all(0)
        assert same.argmax() == cell  # the first cell of its tuple
        assert l3[2][cell] - S == (l3[1][cell] - S) - (l3[0][cell] - S)
    fr = KA.click_frames(GC.mirror_delays(name, lut), 3, 1024)
    win = band_ref.window_q15(1024)
    e = G.gcc_phat_batch(fr, S, win, lut, half_w=hw, half_h=hh, grid_scale=scale)
    d = oracle.localize_batch(fr, S, win, lut, half_w=hw, half_h=hh, grid_scale=scale)
    for r in (e, d):
        assert r["cell"].tolist() == cells.tolist() and (r["xy"] == xy).all()


def test_stream_captures_stay_within_the_caps_on_the_references(dumped, oracle):
    """No stream dropped and no cell skipped on the float64 references alone, with their geometry arguments."""
    import stream_cont_cases as Cs
    import stream_cont_ref
    import stream_phat_ref
    win = band_ref.window_q15(1024)
    sp = GC.STREAM_PHAT
    hw, hh, scale, _, _, fs = GC.geometry(sp["case"])
    lut = _lut(dumped, sp["case"])
    r = stream_phat_ref.run(oracle, GC.stream_capture(sp, lut), sp["N"], fs, GC.CASES[sp["case"]]["S"], win, lut,
                            half_w=hw, half_h=hh, grid_scale=scale)
    records, gated, dropped, skipped, gap = stream_phat_ref.stats(r)
    print(f"triggered {sp['case']}: {records} records, {gated} gated, {dropped} dropped, {skipped} skipped, gap {gap:.2e}")
    assert gated > 10 and dropped == 0 and skipped == 0
    sd = GC.STREAM_DIRECT
    e = oracle.stream_run(GC.stream_capture(sd, lut), sd["N"], fs, GC.CASES[sd["case"]]["S"], win, lut, half_w=hw,
                          half_h=hh)
    assert e["gate"].sum() > 10
    sc = GC.STREAM_CONT
    hw, hh, scale, _, _, fs = GC.geometry(sc["case"])
    lut = _lut(dumped, sc["case"])
    r = stream_cont_ref.run(oracle, GC.stream_capture(sc, lut, **Cs.BURST), sc["N"], fs, GC.CASES[sc["case"]]["S"], win,
                            lut, sc["hop"], sc["activity_var"], half_w=hw, half_h=hh, grid_scale=scale)
    records, gated, dropped, skipped, gap = stream_cont_ref.stats(r)
    print(f"continuous {sc['case']}: {records} records, {gated} gated, {dropped} dropped, {skipped} skipped, gap {gap:.2e}")
    assert records >= 90 and dropped == 0 and skipped <= Cs.max_skip(3) * gated


def test_sanitized_build_is_clean_on_the_cases(tools, dumped, tmp_path):  # noqa: F811
    for name in GC.CASES:
        _, _, r = run_tool(tools[1], str(tmp_path), name, GC.config_overrides(name))
        assert r.returncode == 0, (name, r.stdout[-500:], r.stderr[-3000:])
        assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr
        assert json.loads(r.stdout) == dumped[name][0]
