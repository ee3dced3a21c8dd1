"""Float64 reference of the continuous streaming pipeline (TEST INFRASTRUCTURE
ONLY; tdoa_stream_create_continuous, include/tdoa.h).

No product code.  `active` restates the header's frame rule: with pos the
samples consumed before a hop there is one candidate per stream and hop,
e = pos + hop, eligible iff e >= N; its frame is F = [e - N, e);

    pw(m) = N * sum_F x_m^2 - (sum_F x_m)^2

on the ring's own sample values (uint8 counts 0..255 or int16 counts), and the
stream is listed iff sum_m pw(m) >= activity_var * N^2.  The sums are int64
(the header's bounds: every value stays within 2^57), or with python_int=True
Python ints, which have no width to overflow; the CPU tests hold the two equal
on a full-scale capture.

`run` has the shape of stream_phat_ref.run / stream16_ref.run: the frames are
`active`'s, each frame cap[s, end - N:end].T goes through
band_ref.gcc_phat_band (uint8 rings, widened to int16) or
pcm16_ref.gcc_phat_pcm16 (int16 rings) with the weight table w, and the EMA,
grid, margins, est_at and map_at are stream_phat_ref's.  max_trig is the hop
count: a stream is listed at most once per hop.
"""
import numpy as np

import band_ref
import pcm16_ref
from stream_phat_ref import (TOL_CELL_MARGIN, TOL_EST, TOL_LAG_MARGIN, TOL_MAXL, _top2,  # noqa: F401
                             dropped_streams, map_at, stats)


def active(cap, N, hop, activity_var, python_int=False):
    """cap uint8 or int16 [S][T][M] -> {"n_trig": int32 [S], "end": int64
    [S][hops], "total": sum_m pw(m) of every hop's candidate [S][hops] (0 where
    it is not eligible)} over the first T // hop hops."""
    cap = np.asarray(cap)
    assert cap.dtype in (np.uint8, np.int16) and cap.ndim == 3
    ns, T, M = cap.shape
    hops = T // hop
    thr = int(activity_var) * N * N
    T_ = object if python_int else np.int64
    n_trig = np.zeros(ns, np.int32)
    end = np.zeros((ns, max(hops, 1)), np.int64)
    total = np.zeros((ns, max(hops, 1)), T_)
    for h in range(hops):
        e = (h + 1) * hop  # pos = h * hop
        if e < N:
            continue
        x = cap[:, e - N:e, :].astype(T_)
        s1, s2 = x.sum(1), (x * x).sum(1)
        tot = (N * s2 - s1 * s1).sum(1)
        total[:, h] = tot
        for s in range(ns):
            if tot[s] >= thr:
                end[s, n_trig[s]] = e
                n_trig[s] += 1
    return {"n_trig": n_trig, "end": end, "total": total}


def run(oracle, cap, N, fs, S, window, lut, hop, activity_var, w=None, half_w=50, half_h=50, grid_scale=24.0):
    """oracle: tests' oracle module (its decay() is the EMA's clock rule)."""
    cap = np.ascontiguousarray(cap)
    pcm16 = cap.dtype == np.int16
    ns, T, M = cap.shape
    P, K = M * (M - 1) // 2, 2 * S + 1
    lut2 = np.asarray(lut).reshape(P, -1).astype(np.int64)
    act = active(cap, N, hop, activity_var)
    n_trig, end = act["n_trig"], act["end"]
    max_trig = end.shape[1]
    idx = [(s, i) for s in range(ns) for i in range(n_trig[s])]
    r = {"n_trig": n_trig, "end": end,
         "lags": np.zeros((ns, max_trig, P), np.int32), "gate": np.zeros((ns, max_trig), np.uint8),
         "ema_best": np.zeros((ns, max_trig, P), np.int32), "cell": np.full((ns, max_trig), -1, np.int32),
         "xy": np.zeros((ns, max_trig, 2), np.float32), "max_Lf": np.zeros((ns, max_trig)),
         "weighted": np.zeros((ns, max_trig, P, K)),
         "raw_margin": np.zeros((ns, max_trig, P)), "ema_margin": np.zeros((ns, max_trig, P)),
         "map_gap": np.zeros((ns, max_trig)), "est_at": np.zeros((ns, max_trig, P, K)),
         "est": np.zeros((ns, P, K)), "last": np.zeros(ns, np.uint64), "lut2": lut2}
    if not idx:
        return r
    frames = np.stack([np.ascontiguousarray(cap[s, end[s, i] - N:end[s, i], :].T).astype(np.int16) for s, i in idx])
    if pcm16:
        fr = pcm16_ref.gcc_phat_pcm16(frames, S, window, w=w)
    else:
        fr = band_ref.gcc_phat_band(frames, S, window, np.ones(N + 1) if w is None else w)
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
