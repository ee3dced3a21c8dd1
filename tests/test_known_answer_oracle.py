"""The fp64 GCC-PHAT oracle on known-answer click frames (tests/known_answer.py).

These conditions are what lets test_gpu_known_answer.py assert every in-range
pair of a click frame against a closed form without a margin filter:
  in-range live pair   lag == d_j - d_i, peak == the per-mic closed form within
                       1e-9, off-peak magnitude <= 1e-9, top-2 margin > 0.99
  dead-mic pair        scores exactly 0, lag == -S (the first maximum)
  gate                 sum of squared lags > 4 of those lags
The peak is "within 1e-9 of 1" only in the limit of no floor: under the
definition U_m = X_m / sqrt(|X_m|^2 + eps) a click of prepped amplitude a peaks
at a^2 / (a^2 + eps), i.e. 1 - 1.7e-8 for the quiet click (h = 1) at the default
eps = 1e-12.  So the default-eps run is held to the closed form within 1e-9
(and to 1 within 1e-9 wherever the closed form itself is that close), and a run
at eps = 1e-300 is held to 1 within 1e-9 on every case.
"""
import numpy as np
import pytest

from conftest import golden

import gcc_phat_oracle as G
import known_answer as KA
from tdoa import synth

TOL = 1e-9


def _geometry(oracle, name):
    if name == "3x1024":
        M, N, S = 3, 1024, 46
        lut = golden("pipeline_cfg2.npz")["lut"]
    else:
        M, N, S = 4, 2048, 32
        lut = oracle.build_lut(synth.square_mics(0.15), max_shift=S)
    return M, N, S, np.asarray(lut).reshape(M * (M - 1) // 2, -1), golden("window_q15.npz")[f"n{N}"]


def _check_set(fr, delays, S, win, lut, eps, peak_is_one):
    exp = KA.expected(fr, delays, S, win, eps=eps)
    res = G.gcc_phat_batch(fr, S, win, lut, eps=eps)
    sc = res["scores_f"]
    inr, live = exp["inr"], exp["live"]
    assert inr.sum() > 0
    assert (res["lags"][inr] == exp["lag"][inr]).all()
    oh = KA.onehot(exp, S)
    assert np.abs(sc - oh)[inr].max() <= TOL  # peak and every off-peak lag
    srt = np.sort(sc, -1)
    assert (srt[..., -1] - srt[..., -2])[inr].min() > 0.99
    if peak_is_one:
        assert np.abs(sc.max(-1) - 1.0)[inr].max() <= TOL
    else:
        near = inr & (1.0 - exp["peak"] <= 1e-10)
        assert near.sum() > inr.sum() // 2
        assert np.abs(sc.max(-1) - 1.0)[near].max() <= TOL
    # out of range: nothing in -S..S
    assert np.abs(sc[live & ~inr]).max(initial=0) <= TOL
    # dead mic: an exactly zero spectrum, the first-maximum rule
    assert (sc[~live] == 0).all() and (res["lags"][~live] == -S).all()
    gate, known = KA.expected_gate(exp, S)
    assert known.sum() >= len(gate) - 2
    assert (res["gate"][known] == gate[known]).all()
    assert set(gate[known].tolist()) == {0, 1}
    return exp, res


@pytest.mark.parametrize("name", ["3x1024", "4x2048"])
@pytest.mark.parametrize("eps", [1e-12, 1e-300])
def test_oracle_on_click_cases(oracle, name, eps):
    M, N, S, lut, win = _geometry(oracle, name)
    cases = KA.build_cases(M, S, lut)
    names = [c.name for c in cases]
    assert len(names) == len(set(names)) and 20 <= len(cases) <= 64
    fr, delays = KA.case_frames(cases, M, N)
    exp, _ = _check_set(fr, delays, S, win, lut, eps, peak_is_one=eps < 1e-100)
    # the cases meant to fall out of range do, and only pairs of their mics
    for b, c in enumerate(cases):
        if c.name == "d1=S+1":
            assert [bool(v) for v in exp["inr"][b]] == [1 not in ij for ij in KA.pairs(M)]
        if c.name == "d1=S-1,d2=-(S-1)":
            assert [bool(v) for v in exp["inr"][b]] == [ij != (1, 2) for ij in KA.pairs(M)]
        if c.name in ("d1=+S", "d1=-S"):
            assert exp["inr"][b].all() and np.abs(exp["lag"][b]).max() == S


@pytest.mark.parametrize("N", [256, 512, 1024, 2048, 4096])
@pytest.mark.parametrize("n0", [None, 3, 10, 40, -50])
def test_oracle_click_positions_every_window(N, n0):
    """Every golden window and click position: lags 0, +-1, +-(S-1), +-S."""
    win = golden("window_q15.npz")[f"n{N}"]
    S = 30
    n0 = None if n0 is None else (n0 if n0 > 0 else N + n0)
    rows = [[0, 0, 0], [0, 1, 0], [0, 0, S - 1], [0, S, 0], [0, 0, S], [0, 1, S]]
    if n0 is None or n0 >= S:  # a click cannot sit before sample 0
        rows += [[0, -1, 0], [0, -(S - 1), 0], [0, -S, 0], [0, -S, 1]]
    fr = KA.click_frames(rows, 3, N, n0=n0)
    exp = KA.expected(fr, np.array(rows, float), S, win)
    res = G.gcc_phat_batch(fr, S, win)
    assert exp["inr"].sum() >= 3 * len(rows) - 2
    assert (res["lags"][exp["inr"]] == exp["lag"][exp["inr"]]).all()
    assert np.abs(res["scores_f"] - KA.onehot(exp, S))[exp["inr"]].max() <= TOL
    assert np.abs(res["scores_f"][exp["live"] & ~exp["inr"]]).max(initial=0) <= TOL


@pytest.mark.parametrize("name", ["3x1024", "4x2048"])
@pytest.mark.parametrize("base", [-32768, 0, 255, 32767 - 100])
def test_oracle_click_bases(oracle, name, base):
    M, N, S, lut, win = _geometry(oracle, name)
    rows = [[0] * M, [0, S] + [0] * (M - 2), [0, -S] + [1] * (M - 2), [0, 1] + [0] * (M - 2)]
    fr = KA.click_frames(rows, M, N, base=base)
    _check_set(fr, np.array(rows, float), S, win, lut, 1e-12, peak_is_one=False)


@pytest.mark.parametrize("name", ["3x1024", "4x2048"])
def test_oracle_raised_floor_is_per_mic(oracle, name):
    """eps = 1e-4: the peak is a_i a_j / sqrt((a_i^2 + eps)(a_j^2 + eps)), a one-hot still."""
    M, N, S, lut, win = _geometry(oracle, name)
    rows = [[0, 5, 9, 2][:M]]
    for h in (1, 2, 100):
        fr = KA.click_frames(rows, M, N, h=h)
        exp = KA.expected(fr, np.array(rows, float), S, win, eps=1e-4)
        res = G.gcc_phat_batch(fr, S, win, lut, eps=1e-4)
        assert exp["inr"].all()
        assert (res["lags"] == exp["lag"]).all()
        assert np.abs(res["scores_f"] - KA.onehot(exp, S)).max() <= TOL
        a = exp["amp"][0]
        mine = a[0] * a[1] / np.sqrt((a[0] ** 2 + 1e-4) * (a[1] ** 2 + 1e-4))
        assert abs(res["scores_f"][0, 0].max() - mine) <= TOL


def test_floor_definition_is_pinned():
    """h = 1 at 3 x 1024, eps = 1e-4: 0.37718 per mic (the contract); the per-pair
    clamp R / max(|X_i* X_j|, eps) that three routes used to compute gives 0.6056."""
    win = golden("window_q15.npz")["n1024"]
    fr = KA.click_frames([[0, 5, 9]], 3, 1024, h=1)
    res = G.gcc_phat_batch(fr, 46, win, eps=1e-4)
    peak = res["scores_f"][0, 0].max()
    assert abs(peak - 0.37718) <= 1e-4
    a = KA.expected(fr, np.array([[0.0, 5.0, 9.0]]), 46, win)["amp"][0]
    assert abs(min(1.0, a[0] * a[1] / 1e-4) - 0.6056) <= 1e-4  # what the old form gave
    assert abs(peak - 0.6056) > 0.2
