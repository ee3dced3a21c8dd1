"""Float64 reference of the streaming GCC_PHAT pipeline (TEST INFRASTRUCTURE ONLY).

No product code: the trigger positions are oracle.stream_run's (the trigger
does not depend on the engine), each triggered frame is adc[s, end - N:end].T
widened to int16, its scores, lags and gate are band_ref.gcc_phat_band's (all
ones when no weight table is given), the EMA is

    est <- est + (w - est) * oracle.decay(now, last)     now = end * 10^6 // fs

in float64 on gated frames only (EMA scores and clocks start at 0), and the
grid is L[cell] = sum_p est[p][lut[p][cell]] with its first argmax.

Besides the records it returns what the comparisons need to know where fp32
may legitimately differ: per record the float64 top-2 margin of every pair's
raw scores, the top-2 margin of every pair's EMA row, the gap between the two
highest distinct values of the EMA map, and the EMA scores after the record
(`est_at`, from which `map_at` rebuilds the map's value at any cell).
"""
import numpy as np

import band_ref


def _top2(a):
    s = np.sort(a, axis=-1)
    return s[..., -1] - s[..., -2]


def run(oracle, adc, N, fs, S, window, lut, w=None, max_trig=64, half_w=50, half_h=50, grid_scale=24.0):
    adc = np.ascontiguousarray(adc, dtype=np.uint8)
    ns, T, M = adc.shape
    P, K = M * (M - 1) // 2, 2 * S + 1
    lut2 = np.asarray(lut).reshape(P, -1).astype(np.int64)
    trig = oracle.stream_run(adc, N, fs, S, window, np.asarray(lut).reshape(P, -1), max_trig=max_trig)
    n_trig, end = trig["n_trig"], trig["end"]
    assert n_trig.max() < max_trig
    if w is None:
        w = np.ones(N + 1)
    idx = [(s, i) for s in range(ns) for i in range(n_trig[s])]
    frames = np.stack([adc[s, end[s, i] - N:end[s, i], :].T.astype(np.int16) for s, i in idx])
    fr = band_ref.gcc_phat_band(frames, S, window, w)
    r = {"n_trig": n_trig, "end": end,
         "lags": np.zeros((ns, max_trig, P), np.int32), "gate": np.zeros((ns, max_trig), np.uint8),
         "ema_best": np.zeros((ns, max_trig, P), np.int32), "cell": np.full((ns, max_trig), -1, np.int32),
         "xy": np.zeros((ns, max_trig, 2), np.float32), "max_Lf": np.zeros((ns, max_trig)),
         "weighted": np.zeros((ns, max_trig, P, K)),
         "raw_margin": np.zeros((ns, max_trig, P)), "ema_margin": np.zeros((ns, max_trig, P)),
         "map_gap": np.zeros((ns, max_trig)), "est_at": np.zeros((ns, max_trig, P, K)),
         "est": np.zeros((ns, P, K)), "last": np.zeros(ns, np.uint64), "lut2": lut2}
    W = 2 * half_w + 1
    for b, (s, i) in enumerate(idx):
        r["lags"][s, i] = fr["lags"][b]
        r["gate"][s, i] = fr["gate"][b]
        r["weighted"][s, i] = fr["weighted_f"][b]
        r["raw_margin"][s, i] = _top2(fr["scores_f"][b])
        if not fr["gate"][b]:
            continue
        now = int(end[s, i]) * 1000000 // fs
        est = r["est"][s]
        est += (fr["weighted_f"][b] - est) * oracle.decay(now, int(r["last"][s]))
        r["last"][s] = now
        r["est_at"][s, i] = est
        r["ema_best"][s, i] = np.argmax(est, axis=-1) - S
        r["ema_margin"][s, i] = _top2(est)
        Lg = np.zeros(lut2.shape[1])
        for p in range(P):
            Lg += est[p][lut2[p]]
        cell = int(np.argmax(Lg))
        r["cell"][s, i] = cell
        r["max_Lf"][s, i] = Lg[cell]
        u = np.unique(Lg)
        r["map_gap"][s, i] = u[-1] - u[-2] if u.size > 1 else 0.0
        r["xy"][s, i] = (np.float32(cell % W - half_w) / np.float32(grid_scale),
                         np.float32(half_h - cell // W) / np.float32(grid_scale))
    return r


def map_at(r, s, i, cell):
    """The float64 EMA map of record (s, i) at `cell`."""
    est, lut2 = r["est_at"][s, i], r["lut2"]
    return float(sum(est[p][lut2[p][cell]] for p in range(est.shape[0])))


# the project's GCC-PHAT tolerances (tests/test_gpu_gcc_phat.py) and the EMA state's
TOL_LAG_MARGIN = 2e-4
TOL_CELL_MARGIN = 1e-3
TOL_MAXL = 1e-3
TOL_EST = 5e-5  # the 3e-5 score tolerance, kept by a convex combination, plus <= 64 fp32 roundings of values <= 1


def dropped_streams(r):
    """Per stream the index of its first record whose raw margin is <= 2e-4
    (its gate history may differ from then on); n_trig if none."""
    ns = r["n_trig"].size
    first = r["n_trig"].copy()
    for s in range(ns):
        for i in range(r["n_trig"][s]):
            if r["raw_margin"][s, i].min() <= TOL_LAG_MARGIN:
                first[s] = i
                break
    return first


def stats(r):
    """(records, gated, streams dropped, gated records whose cell is skipped,
    minimum map gap over the compared gated records)."""
    first = dropped_streams(r)
    n = g = skipped = 0
    gap = np.inf
    for s in range(r["n_trig"].size):
        n += int(r["n_trig"][s])
        g += int(r["gate"][s, :r["n_trig"][s]].sum())
        for i in range(first[s]):
            if r["gate"][s, i]:
                gap = min(gap, r["map_gap"][s, i])
                skipped += r["map_gap"][s, i] <= TOL_CELL_MARGIN
    return n, g, int((first < r["n_trig"]).sum()), int(skipped), float(gap)
