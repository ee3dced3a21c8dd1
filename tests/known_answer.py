"""Known-answer "click" frames for the GCC-PHAT and DIRECT routes (a plain
helper module, imported by test_known_answer_oracle.py and
test_gpu_known_answer.py).

A click frame is a constant `base` plus one sample of height `h` at position
n0 + d_m in mic m.  The integer front end (floor-mean DC removal, <<8, Q15
window) leaves exactly one nonzero sample a_m * 2^15 per live mic, so every
spectrum is flat, |X_m[k]| = a_m, and with the PHAT floor of include/tdoa.h
(U_m = X_m / sqrt(|X_m|^2 + eps)) the score of pair (i, j) is

    peak(i, j) = a_i a_j / sqrt((a_i^2 + eps) (a_j^2 + eps))

at lag d_j - d_i and 0 at every other lag: a one-hot when |d_j - d_i| <= S, all
zero in range when it is not, and exactly zero when a mic is dead (constant).
DIRECT's raw score at the click lag is the product of the two prepped samples.
"""
import functools
import itertools

import numpy as np

import gcc_phat_oracle as G


def click_frames(delays, M, N, h=100, base=128, n0=None):
    """int16 [B][M][N]: mic m of frame b is `base` with base + h at n0 + delays[b][m];
    a delay of None is a dead mic (constant at base).  n0 defaults to N / 2."""
    n0 = N // 2 if n0 is None else n0
    B = len(delays)
    fr = np.full((B, M, N), base, np.int64)
    for b, row in enumerate(delays):
        assert len(row) == M
        for m, d in enumerate(row):
            if d is None:
                continue
            assert 0 <= n0 + d < N, (n0, d)
            fr[b, m, n0 + d] = base + h
    assert fr.min() >= -32768 and fr.max() <= 32767
    return fr.astype(np.int16)


def pairs(M):
    return [(i, j) for i in range(M) for j in range(i + 1, M)]


@functools.lru_cache(maxsize=None)
def _gate_boundary(M):
    """Delay rows (d_0 = 0) with the largest sum of squared pair lags <= 4 and the
    smallest > 4 reachable at M mics (M = 2: lags 2 and 3; M = 3: 2 and 6)."""
    best = {}
    for d in itertools.product(range(-1, 4), repeat=M - 1):
        row = (0,) + d
        tot = M * sum(x * x for x in row) - sum(row) ** 2  # = sum over pairs of (d_j - d_i)^2
        key = "le" if tot <= 4 else "gt"
        if key not in best or (tot > best[key][0] if key == "le" else tot < best[key][0]):
            best[key] = (tot, list(row))
    return best["le"], best["gt"]


class Case:
    """One click frame: its name, delays (None = dead mic), and generator arguments."""

    def __init__(self, name, delays, h=100, base=128, n0=None, override=None):
        self.name, self.delays, self.h, self.base, self.n0 = name, list(delays), h, base, n0
        self.override = override or {}  # mic -> constant level (a dead, saturated mic)


def build_cases(M, S, lut, seed=0x5EED):
    """The click set of one geometry.  lut: uint8 [P][G] (or [P][H][W]), pair order
    (0,1), (0,2), ..."""
    lut2 = np.asarray(lut).reshape(M * (M - 1) // 2, -1).astype(np.int64)
    Gc = lut2.shape[1]

    def one(v):
        return [0, v] + [0] * (M - 2)

    def lut_delays(cell):
        return [0] + [int(lut2[m - 1][cell]) - S for m in range(1, M)]

    cases = [Case("zero", [0] * M)]
    (tle, dle), (tgt, dgt) = _gate_boundary(M)
    cases += [Case(f"gate_sum{tle}", dle), Case(f"gate_sum{tgt}", dgt)]
    cases += [Case("d1=+S", one(S)), Case("d1=-S", one(-S)), Case("d1=S-1", one(S - 1)),
              Case("d1=S+1", one(S + 1))]
    if M >= 3:
        cases.append(Case("d1=S-1,d2=-(S-1)", [0, S - 1, -(S - 1)] + [0] * (M - 3)))
    rng = np.random.default_rng(seed + M)
    cells = [0, Gc - 1, Gc // 2] + [int(c) for c in rng.integers(0, Gc, 5)]
    cases += [Case(f"lut_cell{c}", lut_delays(c)) for c in cells]
    dead1 = [0] * M
    dead1[1] = None
    cases.append(Case("mic1_dead", dead1, base=128))
    dead0 = [None] + [0] * (M - 1)
    cases.append(Case("mic0_dead_255", dead0, base=128, override={0: 255}))
    h = 100
    for i, base in enumerate((-32768, 0, 255, 32767 - h)):
        cases.append(Case(f"base{base}", lut_delays(cells[3 + i]), h=h, base=base))
    cases.append(Case("quiet_h1", lut_delays(cells[7]), h=1))
    cases.append(Case("n0=3", [m % 3 for m in range(M)], h=100, n0=3))
    return cases


def case_frames(cases, M, N):
    """int16 [len(cases)][M][N] and the delays as a float array (nan = dead)."""
    fr = np.concatenate([click_frames([c.delays], M, N, h=c.h, base=c.base, n0=c.n0) for c in cases])
    for b, c in enumerate(cases):
        for m, level in c.override.items():
            fr[b, m, :] = level
    d = np.array([[np.nan if x is None else float(x) for x in c.delays] for c in cases])
    return fr, d


def expected(frames, delays, S, window, eps=1e-12):
    """Closed forms of a click batch.  Returns a dict of [B][P] arrays:
      lag    d_j - d_i (0 where not live)
      live   both mics have a click
      inr    live and |lag| <= S  (the one-hot pairs)
      peak   the per-mic closed form at `eps`
      prod   the product of the two prepped int16 samples (DIRECT's raw peak)
    and `amp` [B][M], the prepped amplitude / 2^15 (0 for a dead mic)."""
    x = G.prep(frames, window).astype(np.int64)
    B, M, N = x.shape
    nz = (x != 0).sum(-1)
    alive = ~np.isnan(delays)
    assert (nz[alive] == 1).all() and (nz[~alive] == 0).all(), "a click must prep to one nonzero sample"
    samp = x.sum(-1)  # the one nonzero sample (0 for a dead mic)
    pos = np.abs(x).argmax(-1)
    amp = samp / 32768.0
    pr = pairs(M)
    P = len(pr)
    out = {k: np.zeros((B, P), t) for k, t in (("lag", np.int64), ("live", bool), ("inr", bool),
                                                 ("peak", np.float64), ("prod", np.int64))}
    for p, (i, j) in enumerate(pr):
        live = alive[:, i] & alive[:, j]
        lag = np.where(live, pos[:, j] - pos[:, i], 0)
        dl = np.where(live, np.nan_to_num(delays[:, j]) - np.nan_to_num(delays[:, i]), 0)
        assert (lag == dl).all()
        out["lag"][:, p] = lag
        out["live"][:, p] = live
        out["inr"][:, p] = live & (np.abs(lag) <= S)
        ai, aj = amp[:, i], amp[:, j]
        out["peak"][:, p] = ai * aj / np.sqrt((ai * ai + eps) * (aj * aj + eps))
        out["prod"][:, p] = samp[:, i] * samp[:, j]
    out["amp"] = amp
    return out


def onehot(exp, S):
    """float64 [B][P][K]: exp['peak'] at the click lag of every in-range pair, else 0."""
    B, P = exp["lag"].shape
    oh = np.zeros((B, P, 2 * S + 1))
    b, p = np.nonzero(exp["inr"])
    oh[b, p, exp["lag"][b, p] + S] = exp["peak"][b, p]
    return oh


def expected_gate(exp, S):
    """(gate uint8 [B], known bool [B]): sum of squared lags > 4 with a dead pair at
    lag -S; known only where no live pair is out of range (those lags are roundoff)."""
    lag = np.where(exp["live"], exp["lag"], -S)
    known = (exp["inr"] | ~exp["live"]).all(-1)
    return ((lag ** 2).sum(-1) > 4).astype(np.uint8), known
