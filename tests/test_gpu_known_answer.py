"""Known-answer click frames (tests/known_answer.py) through every GCC-PHAT
dispatch route, the least-squares refinement and DIRECT.

A click frame preps to one nonzero sample per mic, so the PHAT score of pair
(i, j) is a one-hot at lag d_j - d_i whose height is the closed form
a_i a_j / sqrt((a_i^2 + eps)(a_j^2 + eps)) (include/tdoa.h phat_eps); the fp64
oracle meets that within 1e-9 with a top-2 margin > 0.99
(test_known_answer_oracle.py), which is why nothing here filters by margin:
every in-range live pair is asserted, dead-mic pairs are exactly zero with
lag -S, and out-of-range pairs are within tolerance of zero (their lag is
roundoff).  Tolerances are the project's: TOL_SCORE = 3e-5 absolute on scores
(test_gpu_gcc_phat.py), 1e-5 relative on xy_ls (test_ls.py); DIRECT is bit-exact.

Each case asserts the kernel its shape dispatches to (ROUTES), so the route
coverage cannot drift silently.  Every case prints the worst errors it measured
before asserting.  Measured on an MI355X (worst over a route's shapes, bound 3e-5):

  route            eps 1e-12 clicks          eps 1e-4 clicks      eps 1e-6 ADC
                   |gpu-onehot| |gpu-fp64|   |gpu-fp64| = |peak-closed form|
  k_p1k_lean       1.2e-7       1.2e-7       1.2e-7               1.3e-7
  k_gcc_phat_1024  6.0e-8       6.0e-8       9.5e-8               2.2e-7
  k_gcc_phat       1.2e-7       1.2e-7       7.1e-8               1.3e-7
  k_phat_spectra   1.2e-7       1.2e-7       1.4e-7               1.3e-7
  k_spec16         1.2e-7       1.2e-7       1.4e-7               1.7e-7
  k_frame16        1.6e-7       1.6e-7       1.5e-7               2.8e-7

Before the floor had one definition, the eps = 1e-4 peak of the h = 1 click was
0.6056 (per-pair clamp) on k_gcc_phat, k_gcc_phat_1024 and k_phat_spectra
against the contract's 0.3772; and k_p1k_lean, which floored bin N/2 at 4 eps,
gave 0.37694 (3.2e-4 from the fp64 oracle at h = 2).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gcc_phat_oracle as G  # noqa: E402
import known_answer as KA  # noqa: E402
from tdoa import synth  # noqa: E402
from tdoa.localizer import Localizer  # noqa: E402
from test_gpu_gcc_phat import PHAT_CONFIGS, TOL_SCORE, TWO, _grid_f32, _np, check_phat  # noqa: E402
from test_gpu_parity import _cmp  # noqa: E402
from test_ls import TOL as TOL_LS  # noqa: E402

DOUBLED = PHAT_CONFIGS[-1][3]  # the reference triangle doubled (S = 63)
assert PHAT_CONFIGS[-1][:3] == (3, 1024, 67600)
SQUARE = synth.square_mics(0.15)

# (expected kernel, M, N, fs, mics)
ROUTES = [
    ("k_p1k_lean", 3, 1024, 50000, None),
    ("k_gcc_phat_1024", 3, 1024, 67600, DOUBLED),
    ("k_gcc_phat", 2, 1024, 50000, TWO),
    ("k_gcc_phat", 3, 512, 48000, None),
    ("k_phat_spectra", 5, 1024, 50000, synth.circle_mics(5, 0.15)),
    ("k_phat_spectra", 4, 256, 50000, SQUARE),
    ("k_spec16", 2, 4096, 50000, TWO),
    ("k_spec16", 5, 2048, 50000, synth.circle_mics(5, 0.15)),
    ("k_frame16", 4, 4096, 50000, SQUARE),
    ("k_frame16", 3, 4096, 48000, None),
    ("k_frame16", 8, 2048, 50000, synth.circle_mics(8, 0.15)),
    ("k_frame16", 4, 2048, 50000, SQUARE),
]
ROUTE_IDS = [f"{r[0]}-{r[1]}x{r[2]}" for r in ROUTES]
GRID_KEYS = ("lags", "gate", "cell", "xy", "max_Lf")


def _phat(route, **kw):
    name, M, N, fs, mics = route
    loc = Localizer(engine="gcc_phat", num_mics=M, frame_len=N, sample_rate_hz=fs, mic_xy=mics, **kw)
    assert loc.batch_kernel() == name, (loc.batch_kernel(), name)
    return loc


class _Run:
    """One route's click set at the default floor: frames, closed forms, the
    scores-requested GPU run and the fp64 oracle, computed once per module."""

    def __init__(self, route):
        self.route = route
        _, M, N, _, _ = route
        self.loc = loc = _phat(route)
        self.S, self.lut, self.win = loc.dims.S, loc.lut(), loc.window()
        self.cases = KA.build_cases(M, self.S, self.lut)
        self.fr_np, self.delays = KA.case_frames(self.cases, M, N)
        assert len(self.cases) <= 64
        self.fr = torch.from_numpy(self.fr_np).cuda()
        self.exp = KA.expected(self.fr_np, self.delays, self.S, self.win)
        self.got = _np(loc.localize(self.fr, scores=True))
        self.f64 = G.gcc_phat_batch(self.fr_np, self.S, self.win, self.lut)


_RUNS = {}


@pytest.fixture(scope="module")
def runs():
    def get(i):
        if i not in _RUNS:
            _RUNS[i] = _Run(ROUTES[i])
        return _RUNS[i]
    yield get
    for r in _RUNS.values():
        r.loc.close()
    _RUNS.clear()


# ---------------------------------------------------------------- a
@pytest.mark.parametrize("i", range(len(ROUTES)), ids=ROUTE_IDS)
def test_clicks_vs_closed_form_and_fp64(runs, i):
    r = runs(i)
    got, exp, S = r.got, r.exp, r.S
    inr, live = exp["inr"], exp["live"]
    sc = got["scores_f"].astype(np.float64)
    oh = KA.onehot(exp, S)
    e_oh = np.abs(sc - oh)[inr].max()
    e_64 = np.abs(sc - r.f64["scores_f"]).max()
    e_oor = np.abs(sc[live & ~inr]).max(initial=0)
    print(f"\nKA eps=1e-12 {ROUTE_IDS[i]}: |gpu-onehot| {e_oh:.3e}  |gpu-fp64| {e_64:.3e}  "
          f"|out-of-range| {e_oor:.3e}  (bound {TOL_SCORE:.0e}; {int(inr.sum())} in-range pairs)")
    assert (got["lags"][inr] == exp["lag"][inr]).all(), np.argwhere(got["lags"] != exp["lag"])[:4].tolist()
    assert e_oh <= TOL_SCORE
    assert e_oor <= TOL_SCORE
    assert (got["scores_f"][~live] == 0.0).all() and (got["lags"][~live] == -S).all()
    assert (~live).any() and (live & ~inr).any()
    gate, known = KA.expected_gate(exp, S)
    assert (got["gate"][known] == gate[known]).all()
    assert (got["gate"][~known] == ((got["lags"][~known].astype(np.int64) ** 2).sum(-1) > 4)).all()
    check_phat(got, r.f64)
    # the grid: the exhaustive float32 scan of the run's own weighted scores ...
    cell, mx = _grid_f32(got["weighted_f"], r.lut)
    assert (got["cell"] == cell).all(), np.argwhere(got["cell"] != cell).ravel()[:4].tolist()
    assert (got["max_Lf"] == mx).all()
    # ... and the known answer: L of a cell counts the one-hot pairs whose LUT
    # entry is the click lag (dead and out-of-range pairs add nothing), so the
    # chosen cell has the largest such count (which cell among equal counts is
    # float roundoff) and max L is that count
    lut2 = r.lut.reshape(r.lut.shape[0], -1).astype(np.int64)
    hit = (lut2[None] == (exp["lag"] + S)[:, :, None]) & inr[:, :, None]  # [B][P][G]
    count = hit.sum(1)
    at = count[np.arange(len(cell)), got["cell"]]
    assert (at == count.max(-1)).all()
    assert np.abs(got["max_Lf"] - at).max() <= 1e-3


# ---------------------------------------------------------------- b
@pytest.mark.parametrize("i", range(len(ROUTES)), ids=ROUTE_IDS)
def test_lean_path_and_neighbour_independence(runs, i):
    r = runs(i)
    lean = _np(r.loc.localize(r.fr))
    assert "scores_f" not in lean
    for k in GRID_KEYS:
        assert np.array_equal(lean[k], r.got[k]), k
    rev = _np(r.loc.localize(r.fr.flip(0).contiguous()))
    for k in GRID_KEYS:
        assert np.array_equal(rev[k][::-1], r.got[k]), ("reversed", k)
    for b in range(3):  # B = 1: no neighbour in the wave or workgroup
        one = _np(r.loc.localize(r.fr[b:b + 1].contiguous()))
        for k in GRID_KEYS:
            assert np.array_equal(one[k][0], r.got[k][b]), ("alone", b, k)


# ---------------------------------------------------------------- c
FLOOR_DELAYS = (0, 5, 9, 2, 7, 11, 4, 13)


@pytest.mark.parametrize("i", range(len(ROUTES)), ids=ROUTE_IDS)
def test_raised_floor(i):
    """phat_eps = 1e-4 on clicks of height 1, 2, 100: every route computes the
    per-mic floor (0.3772 at h = 1 where the per-pair clamp gave 0.6056); and
    phat_eps = 1e-6 on ADC frames, where the two forms differ by 1e-4."""
    route = ROUTES[i]
    _, M, N, _, _ = route
    eps = 1e-4
    loc = _phat(route, phat_eps=eps)
    S, win, lut = loc.dims.S, loc.window(), loc.lut()
    rows = [list(FLOOR_DELAYS[:M])]
    fr = np.concatenate([KA.click_frames(rows, M, N, h=h) for h in (1, 2, 100)])
    delays = np.array(rows * 3, float)
    exp = KA.expected(fr, delays, S, win, eps=eps)
    assert exp["inr"].all()
    got = _np(loc.localize(torch.from_numpy(fr).cuda(), scores=True))
    f64 = G.gcc_phat_batch(fr, S, win, lut, eps=eps)
    sc = got["scores_f"].astype(np.float64)
    e_64 = np.abs(sc - f64["scores_f"]).max()
    e_cf = np.abs(sc.max(-1) - exp["peak"]).max()
    e_oh = np.abs(sc - KA.onehot(exp, S)).max()
    print(f"\nKA eps=1e-4 {ROUTE_IDS[i]}: |gpu-fp64| {e_64:.3e}  |peak-closed form| {e_cf:.3e}  "
          f"|gpu-onehot| {e_oh:.3e}  peaks h=1,2,100 (pair 0): {sc[:, 0].max(-1).round(5).tolist()} "
          f"closed {exp['peak'][:, 0].round(5).tolist()}  (bound {TOL_SCORE:.0e})")
    assert e_64 <= TOL_SCORE
    assert e_cf <= TOL_SCORE
    assert (got["lags"] == exp["lag"]).all()
    loc.close()
    eps = 1e-6
    loc = _phat(route, phat_eps=eps)
    fa, _, _ = synth.adc_frames(32, M, N, lut, S, 0xF1 + N + M, device="cuda")
    got = _np(loc.localize(fa, scores=True))
    f64 = G.gcc_phat_batch(fa.cpu().numpy(), S, win, lut, eps=eps)
    print(f"KA eps=1e-6 {ROUTE_IDS[i]} adc: |gpu-fp64| {np.abs(got['scores_f'] - f64['scores_f']).max():.3e}")
    check_phat(got, f64)
    loc.close()


# ---------------------------------------------------------------- d
def _ls_mics(M):
    return {3: None, 4: SQUARE, 8: synth.circle_mics(8, 0.15)}[M]


@pytest.mark.parametrize("engine,M,N", [("gcc_phat", 3, 1024), ("direct", 3, 1024),
                                        ("gcc_phat", 4, 4096), ("direct", 4, 4096),
                                        ("gcc_phat", 8, 2048), ("direct", 8, 2048)])
def test_ls_on_clicks_and_noise(oracle, engine, M, N):
    """xy_ls / ls_rms against the double oracle on the click set -- the +-S frames
    take the `inside == false` branch of the parabolic vertex, the dead pairs a
    flat parabola -- and on 64 noise-only frames, whose peaks land anywhere."""
    loc = Localizer(engine=engine, num_mics=M, frame_len=N, mic_xy=_ls_mics(M))
    S, lut = loc.dims.S, loc.lut()
    fr_np, _ = KA.case_frames(KA.build_cases(M, S, lut), M, N)
    g = torch.Generator(device="cpu").manual_seed(0xD0 + M)
    noise = torch.randint(0, 256, (64, M, N), generator=g, dtype=torch.int16)
    fr = torch.cat([torch.from_numpy(fr_np), noise]).contiguous().cuda()
    got = _np(loc.localize(fr, scores=True, ls=True))
    raw = got["scores"] if engine == "direct" else got["scores_f"]
    edge = np.abs(got["lags"]) == S
    assert edge.any()
    uv, rms = oracle.ls_refine(raw, got["lags"], loc.mics(), got["cell"])
    err = np.abs(got["xy_ls"] - uv) / np.maximum(1.0, np.abs(uv))
    e_rms = np.abs(got["ls_rms"] - rms).max()
    print(f"\nKA ls {engine} {M}x{N}: xy_ls rel err {err.max():.3e} (bound {TOL_LS:.0e})  "
          f"ls_rms err {e_rms:.3e} (bound {1e-4 * max(1.0, rms.max()):.3e})  edge peaks {int(edge.sum())}")
    assert err.max() <= TOL_LS
    assert e_rms <= 1e-4 * max(1.0, rms.max())
    lean = loc.localize(fr, grid=False, ls=True)
    assert (lean["xy_ls"].cpu().numpy() == got["xy_ls"]).all()
    loc.close()


# ---------------------------------------------------------------- e
DIRECT_SHAPES = [
    (3, 1024, 0, None), (3, 1024, 45, None), (8, 2048, 0, synth.circle_mics(8, 0.15)),
    (4, 4096, 0, SQUARE), (2, 4096, 0, TWO),
]


@pytest.mark.parametrize("M,N,max_shift,mics", DIRECT_SHAPES,
                         ids=[f"{s[0]}x{s[1]}-S{s[2]}" for s in DIRECT_SHAPES])
def test_direct_on_clicks(oracle, M, N, max_shift, mics):
    loc = Localizer(engine="direct", num_mics=M, frame_len=N, max_shift=max_shift, mic_xy=mics)
    S, lut, win = loc.dims.S, loc.lut(), loc.window()
    assert max_shift in (0, S)
    fr_np, delays = KA.case_frames(KA.build_cases(M, S, lut), M, N)
    got = _np(loc.localize(torch.from_numpy(fr_np).cuda(), scores=True))
    ref = oracle.localize_batch(fr_np, S, win, lut.reshape(lut.shape[0], 101, 101))
    _cmp(got, ref)
    # the closed form: the product of the two prepped samples at the click lag, 0 elsewhere
    exp = KA.expected(fr_np, delays, S, win)
    want = np.zeros(got["scores"].shape, np.int64)
    b, p = np.nonzero(exp["inr"])
    want[b, p, exp["lag"][b, p] + S] = exp["prod"][b, p]
    assert (exp["prod"][exp["inr"]] > 0).all()
    assert (got["scores"] == want).all()
    assert (got["lags"][exp["inr"]] == exp["lag"][exp["inr"]]).all()
    assert (got["lags"][~exp["inr"]] == -S).all()  # all-zero scores: the first maximum
    loc.close()


@pytest.mark.parametrize("M,N,mics", [(3, 1024, None), (8, 2048, synth.circle_mics(8, 0.15))])
def test_prepared_path_extremes(oracle, M, N, mics):
    """correlate_prepared on the largest int16 products, in the three-mic tile
    layout and at 8 mics: every pair bit-exact with the reference's integer
    cross-correlation and lag prior."""
    loc = Localizer(engine="direct", num_mics=M, frame_len=N, mic_xy=mics)
    S = loc.dims.S
    fr = np.full((3, M, N), -32768, np.int16)
    fr[1, 0, :] = 32767
    fr[2, :, 0::2] = 32767
    fr[2, :, 1::2] = -32767
    out = _np(loc.correlate_prepared(torch.from_numpy(fr).cuda(), scores=True, grid=False))
    for b in range(3):
        for p, (i, j) in enumerate(KA.pairs(M)):
            sc, best = oracle.xcorr(fr[b, i], fr[b, j], S)
            assert (out["scores"][b, p] == sc).all(), (b, p)
            assert out["lags"][b, p] == best, (b, p)
            assert (out["weighted"][b, p] == oracle.prior(sc, best)).all(), (b, p)
    loc.close()
