"""Every grid-solve route on non-square, non-default geometries
(tests/grid_geometry_cases.py; tests/test_grid_geometry_cpu.py pins the cases'
host tables and checks the inputs below on the references alone).

Every other GPU test of a grid solve runs a square grid at grid_scale 24,
height_offset 1.2 and speed_of_sound 343, where a swapped half_w / half_h, a
wrong grid_W in cell -> (x, y) or a constant baked into k_ls changes no byte.
Per case this module checks

  * the route: batch_kernel() and batch_grid_fused();
  * GCC_PHAT against the float64 oracle at the case's geometry, with
    tests/test_gpu_gcc_phat.py's check_phat and tolerances (scores 3e-5, lags
    where the margin exceeds 2e-4, cell where it exceeds 1e-3, max_Lf 1e-3),
    xy == the closed form of W = 2 half_w + 1, half_w, half_h and scale; the
    margins may exclude at most 5 % of the pairs and 5 % of the frames (the
    oracle alone excludes none), and the frames use >= 4 cells;
  * cell / max_Lf bit for bit against the exhaustive float32 scan of the
    kernel's own weighted scores on ADC, noise and constant frames; on the
    k_p1k_lean cases also batches of 1 and 17 and the launch without scores;
  * frames whose maximum only the second trip of k_p1k_lean's bound loop can see
    (adc and noise frames do not expose a one-trip loop: the other pairs' terms
    keep the understated bound above every L that is found first);
  * an asymmetric known answer: two cells that are mirror images under x <-> y;
  * tdoa_peaks' own (x, y), and the two grid solves that only the A/B library
    holds (k_p1k_w64, the grid fused into k_frame16), in a child process;
  * 16-bit PCM input, DIRECT bit for bit (with tdoa_average_batch's solve),
    least squares with non-default physics and its clamp, and the three
    streaming pipelines, each against its reference at the case's geometry.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AB_LIB = os.path.join(ROOT, "audio-triangulation_amd", "tdoa", "libtdoa_ab.so")
PATHS = [os.path.join(ROOT, "audio-triangulation_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

import gcc_phat_oracle as G  # noqa: E402
import grid_geometry_cases as GC  # noqa: E402
import known_answer as KA  # noqa: E402
import pcm16_ref  # noqa: E402
import stream_cont_cases as Cs  # noqa: E402
import stream_cont_ref  # noqa: E402
import stream_phat_ref  # noqa: E402
import test_gpu_pcm16 as PCM  # noqa: E402  (the route names; its CPU module's batches and cap)
import test_gpu_stream as DS  # noqa: E402
import test_gpu_stream_cont as SC  # noqa: E402
import test_gpu_stream_phat as SP  # noqa: E402
from tdoa import synth  # noqa: E402
from tdoa.localizer import Localizer  # noqa: E402
from test_gpu_gcc_phat import TOL_CELL_MARGIN, TOL_LAG_MARGIN, _grid_f32, check_phat  # noqa: E402
from test_gpu_parity import _cmp  # noqa: E402
from test_ls import TOL as LS_TOL  # noqa: E402

MAX_EXCLUDED = 0.05  # share of (frame, pair) entries, and of frames, that the margins may exclude


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


@pytest.fixture(scope="module")
def ctx():
    """(case name or Localizer kwargs key, engine, sample_format) -> the one Localizer of it, closed at the end."""
    made = {}

    def get(name, engine="gcc_phat", sample_format="adc8"):
        key = (name, engine, sample_format)
        if key not in made:
            kw = GC.TWO_MICS_WIDE if name == "two_mics_wide" else GC.CASES[name]["kw"]
            made[key] = Localizer(engine=engine, sample_format=sample_format, **kw)
        return made[key]

    yield get
    torch.cuda.synchronize()
    for loc in made.values():
        loc.close()


def _geo(name):
    return GC.geometry(GC.TWO_MICS_WIDE if name == "two_mics_wide" else name)


def _assert_xy(loc, name, got):
    """xy is loc.cell_xy(cell) and the closed form, bit for bit."""
    hw, hh, scale = _geo(name)[:3]
    assert loc.grid_W == 2 * hw + 1
    assert got["xy"].tobytes() == loc.cell_xy(got["cell"]).tobytes()
    assert got["xy"].tobytes() == GC.closed_form_xy(got["cell"], hw, hh, scale).tobytes()


# ---- the route
@pytest.mark.parametrize("name", list(GC.CASES))
def test_route(ctx, name):
    c, loc = GC.CASES[name], ctx(name)
    assert (loc.dims.S, loc.dims.K, loc.dims.G) == (c["S"], c["K"], c["W"] * c["H"])
    assert loc.batch_kernel() == c["kernel"], (name, loc.batch_kernel())
    assert loc.batch_grid_fused() == c["fused"], name


# ---- GCC_PHAT against float64, geometry-aware
@pytest.mark.parametrize("name", list(GC.CASES))
def test_phat_vs_fp64(ctx, name):
    c, loc = GC.CASES[name], ctx(name)
    hw, hh, scale = _geo(name)[:3]
    lut = loc.lut().reshape(-1, c["H"], c["W"])
    fr = GC.adc_batch(name, lut)
    got = _np(loc.localize(fr.cuda(), scores=True))
    exp = G.gcc_phat_batch(fr.numpy(), c["S"], loc.window(), lut, half_w=hw, half_h=hh, grid_scale=scale)
    err = np.abs(got["scores_f"] - exp["scores_f"]).max()
    srt = np.sort(exp["scores_f"], axis=-1)
    pairs_out = 1.0 - ((srt[..., -1] - srt[..., -2]) > TOL_LAG_MARGIN).mean()
    top = exp["L"].max(-1)
    second = np.where(exp["L"] >= top[:, None] - 1e-12, -np.inf, exp["L"]).max(-1)
    frames_out = 1.0 - ((top - second > TOL_CELL_MARGIN) & (got["lags"] == exp["lags"]).all(-1)).mean()
    used = len(set(got["cell"].tolist()))
    print(f"{name}: {loc.batch_kernel()}, grid fused {loc.batch_grid_fused()}: max |score err| {err:.2e}, "
          f"pairs excluded {pairs_out:.3f}, frames excluded {frames_out:.3f}, {used} distinct cells")
    check_phat(got, exp, True, hw, hh, scale)
    assert pairs_out <= MAX_EXCLUDED and frames_out <= MAX_EXCLUDED
    assert used >= (4 if loc.dims.G > 1 else 1)
    _assert_xy(loc, name, got)


# ---- the grid, exact on the kernel's own scores
def _own_scores_frames(name, lut):
    M, N, B = GC.shape(name)
    g = torch.Generator(device="cpu").manual_seed(5)
    return {"adc": GC.adc_batch(name, lut),
            "noise": torch.randint(0, 256, (B, M, N), generator=g, dtype=torch.int16),
            "constant": torch.full((8, M, N), 77, dtype=torch.int16)}


def _assert_own_scores(loc, name, fr, tag):
    got = _np(loc.localize(fr.cuda().contiguous(), scores=True))
    cell, mx = _grid_f32(got["weighted_f"], loc.lut())
    assert got["cell"].tolist() == cell.tolist(), tag
    assert got["max_Lf"].tobytes() == mx.astype(np.float32).tobytes(), tag
    _assert_xy(loc, name, got)
    return got


@pytest.mark.parametrize("name", list(GC.CASES))
def test_grid_exact_on_own_scores(ctx, name):
    c, loc = GC.CASES[name], ctx(name)
    lut = loc.lut().reshape(-1, c["H"], c["W"])
    frames = _own_scores_frames(name, lut)
    if c["kernel"] == GC.LEAN:  # the ragged wave and workgroup
        M, N, _ = GC.shape(name)
        for b in (1, 17):
            frames[f"b{b}"] = synth.adc_frames(b, M, N, lut, c["S"], 0x9B + b)[0]
    for kind, fr in frames.items():
        got = _assert_own_scores(loc, name, fr, (name, kind))
        if kind == "constant":  # every tuple ties: the first cell
            assert (got["cell"] == 0).all()
        if c["kernel"] == GC.LEAN:  # the launch without score outputs: the same bytes
            lean = _np(loc.localize(fr.cuda().contiguous()))
            for k in ("cell", "xy", "max_Lf"):
                assert lean[k].tobytes() == got[k].tobytes(), (name, kind, k)


def test_second_trip_of_the_bound_loop(ctx):
    """Frames whose maximum sits on the one lag slot of its row that only the bound loop's second
    trip reads (GC.TWO_TRIPS): a loop of one trip prunes that row and answers the decoy cell, on
    every frame (tests/test_grid_geometry_cpu.py shows both on the numpy model)."""
    sp = GC.TWO_TRIPS
    loc = ctx(sp["case"])
    assert loc.batch_kernel() == GC.LEAN
    l3 = loc.lut().astype(np.int64)
    assert tuple(l3[:, sp["cell"]]) == sp["tuple"] and tuple(l3[:, sp["decoy"]]) == sp["decoy_tuple"]
    fr = torch.from_numpy(GC.two_trip_frames())
    got = _assert_own_scores(loc, sp["case"], fr, "two trips")
    assert (got["lags"] == np.array(sp["tuple"]) - loc.dims.S).all()
    assert (got["cell"] == sp["cell"]).all(), got["cell"].tolist()
    lean = _np(loc.localize(fr.cuda()))
    for k in ("cell", "xy", "max_Lf"):
        assert lean[k].tobytes() == got[k].tobytes(), k


# ---- the peak search's own cell -> (x, y)
@pytest.mark.parametrize("name,engine", [("g1x9", "gcc_phat"), ("tall", "gcc_phat"), ("wide48k", "gcc_phat"),
                                         ("sq4_wide", "gcc_phat"), ("wide48k", "direct"), ("c8_wide", "direct")])
def test_one_peak_is_the_grid_solve(ctx, name, engine):
    """tdoa_peaks with one peak on the weighted scores: the grid solve's cell and max, and its own
    (x, y) the closed form (as smoke() holds it on the default grid)."""
    c, loc = GC.CASES[name], ctx(name, engine)
    hw, hh, scale = _geo(name)[:3]
    fr = GC.adc_batch(name, loc.lut().reshape(-1, c["H"], c["W"])).cuda()
    out = loc.localize(fr, scores=True)
    direct = engine == "direct"
    pk = _np(loc.peaks(out["weighted" if direct else "weighted_f"], num_peaks=1))
    got = _np(out)
    assert (pk["count"] == 1).all() and pk["cell"][:, 0].tolist() == got["cell"].tolist()
    assert pk["L" if direct else "Lf"][:, 0].tobytes() == got["max_L" if direct else "max_Lf"].tobytes()
    assert pk["xy"][:, 0].tobytes() == GC.closed_form_xy(got["cell"], hw, hh, scale).tobytes()
    assert (pk["lags"][:, 0] == loc.lut().astype(np.int64)[:, got["cell"]].T - c["S"]).all()


# ---- the A/B library's grid solves (k_p1k_w64; the grid fused into k_frame16)
AB_CHILD = r"""
import sys
sys.path[:0] = {paths!r}
import numpy as np
import gcc_phat_oracle as G
import grid_geometry_cases as GC
from tdoa.localizer import Localizer
from test_gpu_gcc_phat import check_phat, _np, _grid_f32
for name, kernel in {cases!r}:
    c = GC.CASES[name]
    hw, hh, scale = GC.geometry(name)[:3]
    loc = Localizer(engine="gcc_phat", **c["kw"])
    assert loc.batch_kernel() == kernel and loc.batch_grid_fused(), (name, loc.batch_kernel(), loc.batch_grid_fused())
    lut = loc.lut().reshape(-1, c["H"], c["W"])
    fr = GC.adc_batch(name, lut)
    got = _np(loc.localize(fr.cuda(), scores=True))
    exp = G.gcc_phat_batch(fr.numpy(), c["S"], loc.window(), lut, half_w=hw, half_h=hh, grid_scale=scale)
    check_phat(got, exp, True, hw, hh, scale)
    cell, mx = _grid_f32(got["weighted_f"], loc.lut())
    assert got["cell"].tolist() == cell.tolist() and got["max_Lf"].tobytes() == mx.astype(np.float32).tobytes(), name
    assert got["xy"].tobytes() == GC.closed_form_xy(got["cell"], hw, hh, scale).tobytes(), name
    assert len(set(got["cell"].tolist())) >= 4
    lean = _np(loc.localize(fr.cuda()))  # no scores requested: the kernels' other store site
    for k in lean:
        assert lean[k].tobytes() == got[k].tobytes(), (name, k)
    loc.close()
print("geometry ok")
"""


def test_ab_library_grid_solves():
    """The two grid solves that only the A/B library holds, on non-square grids (a fresh child: the
    library reads TDOA_P1K / TDOA_F16_FG once per process): fp64, own scores, the closed form."""
    assert os.path.exists(AB_LIB), "build with `make -C audio-triangulation_amd ab`"
    # (8 x 2048 is a shape whose last pair round leaves waves idle for the fused grid; 4 x 2048 is not)
    cases = [("tall", "k_p1k_w64"), ("wide48k", "k_p1k_w64"), ("c8_wide", GC.FRAME16), ("c8_7x3", GC.FRAME16)]
    r = subprocess.run([sys.executable, "-c", AB_CHILD.format(paths=PATHS, cases=cases)],
                       env=dict(os.environ, TDOA_LIB=AB_LIB, TDOA_P1K="w64", TDOA_F16_FG="1"), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "geometry ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---- an asymmetric known answer
@pytest.mark.parametrize("engine", ["gcc_phat", "direct"])
@pytest.mark.parametrize("name", list(GC.MIRROR))
def test_mirror_cells_known_answer(ctx, name, engine):
    """Two cells that are mirror images under x <-> y, each the only answer of its integer-delay
    click frame: a transposed solve cannot return both, whatever the oracle does."""
    c, loc = GC.CASES[name], ctx(name, engine)
    cells, xy = GC.mirror_cells(name)
    l3 = loc.lut().astype(np.int64)
    assert c["W"] != c["H"] and (l3[:, cells[0]] != l3[:, cells[1]]).any()
    fr = torch.from_numpy(KA.click_frames(GC.mirror_delays(name, l3), 3, 1024)).cuda()
    got = _np(loc.localize(fr))
    assert (got["lags"] == l3[:, cells].T - c["S"]).all()
    assert got["cell"].tolist() == cells.tolist()
    assert got["xy"].tobytes() == xy.tobytes()


# ---- 16-bit PCM input
# s63_141x45: K = 127 on the largest table that k_p1k_pcm16 stages; s63_121x75's 55 rows exceed it
# (GC.p1k_fits), and a PCM16 context then takes the two-pass route with the exhaustive k_grid behind it
PCM16_CASES = [("g15x9", PCM.P1K, True), ("near", PCM.P1K, True), ("s63_141x45", PCM.P1K, True),
               ("s63_121x75", PCM.TWO_PASS, False), ("sq4_wide", PCM.F16, False)]


@pytest.mark.parametrize("name,kernel,fused", PCM16_CASES)
def test_pcm16(ctx, name, kernel, fused):
    c, loc = GC.CASES[name], ctx(name, sample_format="pcm16")
    hw, hh, scale = _geo(name)[:3]
    M, N, _ = GC.shape(name)
    assert loc.sample_format == "pcm16"
    assert loc.batch_kernel() == kernel and loc.batch_grid_fused() == fused
    fr, silent = PCM.CPU.batch(M, N, 33)
    got = _np(loc.localize(torch.from_numpy(fr).cuda(), scores=True))
    exp = pcm16_ref.gcc_phat_pcm16(fr, c["S"], loc.window(), loc.lut(), half_w=hw, half_h=hh, grid_scale=scale)
    left_out = PCM.CPU.unsure_share(exp, M, silent)
    print(f"{name} pcm16: {loc.batch_kernel()}: max |score err| {np.abs(got['scores_f'] - exp['scores_f']).max():.2e}, "
          f"pairs left out by the margin {left_out:.3f}")
    check_phat(got, exp, True, hw, hh, scale)
    assert left_out <= PCM.CPU.MAX_UNSURE
    for k in ("scores_f", "weighted_f", "max_Lf", "xy"):
        assert np.isfinite(got[k]).all(), k
    assert np.abs(got["lags"]).max() <= c["S"] and got["cell"].min() >= 0 and got["cell"].max() < loc.dims.G
    sp = PCM.CPU.silent_pairs(M)
    assert np.abs(got["scores_f"][silent][sp]).max() <= PCM.T.TOL_SCORE
    # (these frames' sources lie off the small grids, so the 1e-3 cell margin leaves most of their
    # cells to the own-scores rule: exact against the exhaustive float32 scan, and the closed form)
    cell, mx = _grid_f32(got["weighted_f"], loc.lut())
    assert got["cell"].tolist() == cell.tolist() and got["max_Lf"].tobytes() == mx.astype(np.float32).tobytes()
    _assert_xy(loc, name, got)


# ---- DIRECT, bit for bit
DIRECT_CASES = ["g1x9", "g15x9", "tall", "wide48k", "rect18", "sq4_wide", "c8_wide", "c8_7x3", "two_mics_wide"]


def _direct_lut(oracle, loc, name):
    """The oracle's LUT at the case's geometry, after comparing the context's with it."""
    hw, hh, scale, height, speed, fs = _geo(name)
    exp = oracle.build_lut(loc.mics(), hw, hh, scale, height, speed, fs, loc.dims.S)
    assert exp.shape[1:] == (2 * hh + 1, 2 * hw + 1) and (loc.lut() == exp.reshape(loc.dims.P, -1)).all()
    return exp


@pytest.mark.parametrize("name", DIRECT_CASES)
def test_direct_vs_oracle(ctx, oracle, name):
    loc = ctx(name, "direct")
    hw, hh, scale = _geo(name)[:3]
    M, N, S = loc.dims.M, loc.dims.N, loc.dims.S
    lut = _direct_lut(oracle, loc, name)
    B = 24 if M == 8 or N > 2048 else 48
    fr = torch.cat([synth.adc_frames(B, M, N, lut, S, 77 + M + N)[0], synth.full_range_frames(8, M, N, 99 + N)])
    got = _np(loc.localize(fr.cuda().contiguous(), scores=True))
    exp = oracle.localize_batch(fr.numpy(), S, loc.window(), lut, half_w=hw, half_h=hh, grid_scale=scale)
    _cmp(got, exp)
    _assert_xy(loc, name, got)
    assert len(set(got["cell"].tolist())) >= 4


@pytest.mark.parametrize("name", ["wide48k", "c8_wide"])
def test_average_batch_solve(ctx, oracle, name):
    """tdoa_average_batch's grid solve: random EMA scores (weak bounds) and one stream held all-equal (ties)."""
    loc = ctx(name, "direct")
    P, K = loc.dims.P, loc.dims.K
    lut = _direct_lut(oracle, loc, name)
    Sn, steps = 8, 4
    rng = np.random.default_rng(28)
    est = torch.zeros((Sn, P, K), dtype=torch.int64, device="cuda")
    best = torch.zeros((Sn, P), dtype=torch.int32, device="cuda")
    est_ref = np.zeros((Sn, P, K), np.int64)
    cells = set()
    for t in range(steps):
        fresh = rng.integers(-(1 << 40), 1 << 40, (Sn, P, K)).astype(np.int64)
        fresh[0] = 12345  # every tuple ties: the first cell
        dec = rng.uniform(0.05, 1.0, Sn).astype(np.float32)
        solve = {"cell": torch.empty(Sn, dtype=torch.int32, device="cuda"),
                 "max_L": torch.empty(Sn, dtype=torch.int64, device="cuda"),
                 "xy": torch.empty((Sn, 2), dtype=torch.float32, device="cuda")}
        loc.average(est, torch.from_numpy(fresh).cuda(), torch.from_numpy(dec).cuda(), best, solve)
        got = _np(solve)
        for s in range(Sn):
            for p in range(P):
                est_ref[s, p], _ = oracle.average(est_ref[s, p], fresh[s, p], float(dec[s]))
            mL, cell = oracle.grid_solve(est_ref[s], lut)
            assert got["cell"][s] == cell and got["max_L"][s] == mL, (t, s)
        assert (est.cpu().numpy() == est_ref).all()
        assert got["cell"][0] == 0
        _assert_xy(loc, name, got)
        cells.update(got["cell"].tolist())
    assert len(cells) >= 4


# ---- least squares with non-default physics
def _assert_ls(oracle, loc, name, got):
    hw, hh, scale, height, speed, fs = _geo(name)
    raw = got["scores"] if loc.engine == "direct" else got["scores_f"]
    uv, rms = oracle.ls_refine(raw, got["lags"], loc.mics(), got["cell"], hw, hh, scale, height, float(fs), speed)
    err = np.abs(got["xy_ls"] - uv) / np.maximum(1.0, np.abs(uv))
    assert err.max() <= LS_TOL, (name, loc.engine, err.max())
    assert np.abs(got["ls_rms"] - rms).max() <= 1e-4 * max(1.0, rms.max())
    return uv


@pytest.mark.parametrize("engine", ["direct", "gcc_phat"])
@pytest.mark.parametrize("name", ["wide48k", "sos280", "sos400", "rect18", "sq4_rect18", "c8_wide"])
def test_ls_vs_oracle(ctx, oracle, name, engine):
    c, loc = GC.CASES[name], ctx(name, engine)
    fr = GC.adc_batch(name, loc.lut().reshape(-1, c["H"], c["W"])).cuda()
    got = _np(loc.localize(fr, scores=True, ls=True))
    uv = _assert_ls(oracle, loc, name, got)
    # the refinement moves: a kernel that returned the cell's own coordinates would not pass
    assert np.abs(uv - got["xy"]).max() > 10 * LS_TOL
    # without scores / cell requested (k_frame16's peak scores where it writes them): the same answer
    lean = loc.localize(fr, grid=False, ls=True)
    assert lean["xy_ls"].cpu().numpy().tobytes() == got["xy_ls"].tobytes()


@pytest.mark.parametrize("engine", ["direct", "gcc_phat"])
@pytest.mark.parametrize("name", ["g15x9", "g1x9"])
def test_ls_clamp(ctx, oracle, name, engine):
    """Sources at the four corners of a 101 x 101 grid, far outside the case's box (+-7/24 x +-4/24 m;
    g1x9: lu = 0): the refinement runs into the clamp, per axis with the axis' own half extent."""
    c, loc = GC.CASES[name], ctx(name, engine)
    hw, hh, scale = _geo(name)[:3]
    big = oracle.build_lut(loc.mics(), 50, 50, 24.0, 1.2, 343.0, 50000, c["S"]).reshape(3, -1)
    corners = np.ascontiguousarray(big[:, [0, 100, 101 * 100, 101 * 101 - 1]])
    fr = synth.adc_frames(48, 3, 1024, corners, c["S"], 0xC1A + hw)[0].cuda()
    got = _np(loc.localize(fr, scores=True, ls=True))
    uv = _assert_ls(oracle, loc, name, got)
    lu, lv = hw / scale, hh / scale  # the clamp's bounds in double, as k_ls and the oracle form them
    assert (np.abs(got["xy_ls"][:, 0]) <= np.float32(lu)).all() and (np.abs(got["xy_ls"][:, 1]) <= np.float32(lv)).all()
    reached = 0
    for axis, lim in ((0, lu), (1, lv)):
        for sign in (-1.0, 1.0):
            on = uv[:, axis] == sign * lim
            reached += int(on.any())
            assert (got["xy_ls"][on, axis] == np.float32(sign * lim)).all(), (axis, sign)
    print(f"{name} {engine}: the oracle's clamp engages on {reached} of 4 bounds; "
          f"x on a bound {np.mean(np.abs(uv[:, 0]) == lu):.2f}, y {np.mean(np.abs(uv[:, 1]) == lv):.2f} of the frames")
    assert (np.abs(uv[:, 1]) == lv).any() and (np.abs(uv[:, 0]) == lu).any()
    if hw != hh and lu > 0:  # the two bounds differ, and each axis meets its own
        assert lu != lv and not (np.abs(got["xy_ls"][:, 0]) == np.float32(lv)).any()


# ---- streaming
def test_stream_phat_triggered(ctx, oracle):
    sp = GC.STREAM_PHAT
    loc = ctx(sp["case"])
    hw, hh, scale, _, _, fs = _geo(sp["case"])
    lut = loc.lut()
    adc = GC.stream_capture(sp, lut)
    ref = stream_phat_ref.run(oracle, adc, sp["N"], fs, loc.dims.S, loc.window(), lut, half_w=hw, half_h=hh,
                              grid_scale=scale)
    assert ref["gate"].sum() > 10
    for use_graph in (False, True):
        got = SP.run_pipeline(loc, adc, sp["hop"], use_graph=use_graph)
        SP.compare(got, ref, max_dropped=0, max_skip=0.0)
        for lst in got[0].values():
            for g in lst:
                if g["gate"]:
                    assert g["xy"].tobytes() == loc.cell_xy(g["cell"]).tobytes()


def test_stream_phat_continuous(ctx, oracle):
    sc = GC.STREAM_CONT
    loc = ctx(sc["case"])
    hw, hh, scale, _, _, fs = _geo(sc["case"])
    lut = loc.lut()
    cap = GC.stream_capture(sc, lut, **Cs.BURST)
    ref = stream_cont_ref.run(oracle, cap, sc["N"], fs, loc.dims.S, loc.window(), lut, sc["hop"], sc["activity_var"],
                              half_w=hw, half_h=hh, grid_scale=scale)
    assert ref["n_trig"].sum() >= 90
    got = SC.run_pipeline(loc, cap, sc["hop"], sc["activity_var"])
    SP.compare(got, ref, max_dropped=0, max_skip=Cs.max_skip(3))
    for lst in got[0].values():
        for g in lst:
            if g["gate"]:
                assert g["xy"].tobytes() == loc.cell_xy(g["cell"]).tobytes()


def test_stream_direct(ctx, oracle):
    sd = GC.STREAM_DIRECT
    loc = ctx(sd["case"], "direct")
    hw, hh, _, _, _, fs = _geo(sd["case"])
    lut = loc.lut()
    adc = GC.stream_capture(sd, lut)
    exp = oracle.stream_run(adc, sd["N"], fs, loc.dims.S, loc.window(), lut, half_w=hw, half_h=hh)
    assert exp["gate"].sum() > 10
    recs, est, last = DS.run_pipeline(loc, adc, sd["hop"])
    DS.compare(recs, est, last, exp, loc.dims.P)
    gated = [r for lst in recs.values() for r in lst if r["gate"]]
    for r in gated:
        assert r["xy"].tobytes() == loc.cell_xy(r["cell"]).tobytes()
    assert len({int(r["cell"]) for r in gated}) >= 4
