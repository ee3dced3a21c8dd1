"""Float64 reference of the streaming GCC_PHAT pipeline on int16 capture rings
(TEST INFRASTRUCTURE ONLY; tdoa_stream_create_pcm16, include/tdoa.h).

No product code.  `trigger16` restates the header's trigger on int16 samples:
for a stream with samples x_m[t] (zero for t < 0), h = N/2 and the candidate
end e, with O = [e - N, e - h), I = [e - h, e) and

    pw(m, R) = h * sum_R x_m^2 - (sum_R x_m)^2

the stream fires at the first e with e - ring_start >= N and

    sum_m pw(m, O) > trigger_var * h^2 + sum_m pw(m, I)

and ring_start = e from then on (0 at the start).  At most one candidate of a
hop can fire (the next eligible one is N >= hop later), so the positions do
not depend on the hop; a hop only limits the samples consumed to whole hops.
The sums are int64 (the header's bounds: every value stays below 2^56), or
with python_int=True Python ints, which have no width to overflow; the CPU
tests hold the two equal on a full-scale capture.

`run` has the shape of stream_phat_ref.run: the trigger is `trigger16`, each
triggered frame cap[s, end - N:end].T goes through pcm16_ref.gcc_phat_pcm16
(with the weight table w), and the EMA, grid, margins, est_at and map_at are
stream_phat_ref's.
"""
import numpy as np

import pcm16_ref
from stream_phat_ref import (TOL_CELL_MARGIN, TOL_EST, TOL_LAG_MARGIN, TOL_MAXL, _top2,  # noqa: F401
                             dropped_streams, map_at, stats)


def trigger16(cap, N, hop, trigger_var, max_trig=64, python_int=False):
    """cap int16 [S][T][M] -> {"n_trig": int32 [S], "end": int64 [S][max_trig]}.
    hop None: every sample is a candidate end; else the first (T // hop) * hop."""
    cap = np.asarray(cap)
    assert cap.dtype == np.int16 and cap.ndim == 3
    ns, T, M = cap.shape
    Tc = T if hop is None else (T // hop) * hop
    h = N // 2
    thr = int(trigger_var) * h * h
    n_trig = np.zeros(ns, np.int32)
    end = np.zeros((ns, max_trig), np.int64)
    T_ = object if python_int else np.int64
    for s in range(ns):
        # samples t = -N .. Tc - 1 (zeros before the stream starts) and their prefix sums
        x = np.concatenate([np.zeros((N, M), T_), cap[s, :Tc].astype(T_)])
        q1 = np.concatenate([np.zeros((1, M), T_), np.cumsum(x, 0)])
        q2 = np.concatenate([np.zeros((1, M), T_), np.cumsum(x * x, 0)])
        e = np.arange(1, Tc + 1)            # candidate ends; prefix index of time t is t + N
        a, b, c = e, e + h, e + N           # prefix indices of e - N, e - h, e

        def pw(lo, hi):
            s1, s2 = q1[hi] - q1[lo], q2[hi] - q2[lo]
            return (h * s2 - s1 * s1).sum(1)

        fire = np.array(pw(a, b) > thr + pw(b, c), dtype=bool)
        ring_start = 0
        for ei in np.nonzero(fire)[0]:
            ee = int(e[ei])
            if ee - ring_start >= N:
                assert n_trig[s] < max_trig
                end[s, n_trig[s]] = ee
                n_trig[s] += 1
                ring_start = ee
    return {"n_trig": n_trig, "end": end}


def run(oracle, cap, N, fs, S, window, lut, w=None, hop=None, trigger_var=131072, max_trig=64,
        half_w=50, half_h=50, grid_scale=24.0):
    """oracle: tests' oracle module (its decay() is the EMA's clock rule)."""
    cap = np.ascontiguousarray(cap, dtype=np.int16)
    ns, T, M = cap.shape
    P, K = M * (M - 1) // 2, 2 * S + 1
    lut2 = np.asarray(lut).reshape(P, -1).astype(np.int64)
    trig = trigger16(cap, N, hop, trigger_var, max_trig=max_trig)
    n_trig, end = trig["n_trig"], trig["end"]
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
    frames = np.stack([np.ascontiguousarray(cap[s, end[s, i] - N:end[s, i], :].T) for s, i in idx])
    fr = pcm16_ref.gcc_phat_pcm16(frames, S, window, w=w)
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


def full_scale_capture(ns, T, N, M, seed):
    """Streams alternating N/2-sample blocks of near-silence (uniform in
    [-2, 2]) and full scale, each stream starting at a random phase of the
    2-block period.  Even streams: the loud samples are +-32767 with equal
    probability (the largest sum of squares, hence the largest pw); odd
    streams: uniform over [-32767, 32767]."""
    rng = np.random.default_rng(seed)
    h = N // 2
    cap = np.zeros((ns, T, M), np.int16)
    for s in range(ns):
        ph = int(rng.integers(0, 2 * h))
        loud = ((np.arange(T) + ph) // h) % 2 == 1
        full = rng.choice(np.array([-32767, 32767]), (T, M)) if s % 2 == 0 else rng.integers(-32767, 32768, (T, M))
        cap[s] = np.where(loud[:, None], full, rng.integers(-2, 3, (T, M)))
    return cap
