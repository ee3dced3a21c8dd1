"""Float64 reference of GCC-PHAT on 16-bit PCM input (TEST INFRASTRUCTURE ONLY).

oracle/gcc_phat_oracle.py with the front end of TDOA_SAMPLES_PCM16
(include/tdoa.h) in place of the 8-bit ADC one.  Per mic row x[0..N) of int16:

    off  = floor(sum(x) / N)          arithmetic shift; off in [-32768, 32767]
    y[n] = x[n] - off                 no wrap; |y| <= 65535
    s[n] = (y[n] * W[n]) >> 15        arithmetic shift (floor); W the Q15 window

and x = s / 2^15 enters the 2N-point rfft as the oracle's prepared sample does.
Everything downstream -- PHAT with the per-mic floor, the optional bin-weight
table of tests/band_ref.py, lags, prior, gate, grid -- is the oracle's.
"""
import numpy as np

import gcc_phat_oracle as G


def prep16(frames, window):
    """int16 [..][N] raw -> int64 s, the definition above."""
    fr = np.asarray(frames)
    assert fr.dtype == np.int16
    N = fr.shape[-1]
    bits = int(np.log2(N))
    assert 1 << bits == N
    x = fr.astype(np.int64)
    off = x.sum(-1, keepdims=True) >> bits
    return ((x - off) * np.asarray(window, np.int64)) >> 15


def gcc_phat_pcm16(frames, S, window, lut=None, eps=1e-12, w=None, half_w=50, half_h=50, grid_scale=24.0):
    """gcc_phat_oracle.gcc_phat_batch on prep16's samples, R_ij[k] scaled by
    w[k] (float [N + 1]) when a table is given; same keys."""
    x = prep16(frames, window).astype(np.float64) / 32768.0
    B, M, N = x.shape
    L = 2 * N
    wk = np.ones(N + 1) if w is None else np.asarray(w, np.float64)
    assert wk.shape == (N + 1,)
    X = np.fft.rfft(x, L, axis=-1)
    U = X / np.sqrt(X.real ** 2 + X.imag ** 2 + eps)
    pairs = [(i, j) for i in range(M) for j in range(i + 1, M)]
    P, K = len(pairs), 2 * S + 1
    s_idx = np.arange(-S, S + 1) % L
    scores = np.zeros((B, P, K))
    for p, (i, j) in enumerate(pairs):
        r = np.fft.irfft(wk * (np.conj(U[:, i]) * U[:, j]), L, axis=-1)
        scores[:, p] = r[:, s_idx]
    best = np.argmax(scores, axis=-1)  # first max
    lags = (best - S).astype(np.int32)
    pr = G.prior_table(K).astype(np.float64)
    d = np.abs(np.arange(K)[None, None, :] - best[..., None])
    weighted = scores * pr[d]
    res = {"scores_f": scores, "weighted_f": weighted, "lags": lags,
           "gate": ((lags.astype(np.int64) ** 2).sum(-1) > 4).astype(np.uint8)}
    if lut is not None:
        lut2 = np.asarray(lut).reshape(P, -1).astype(np.int64)
        Lg = np.zeros((B, lut2.shape[1]))
        for p in range(P):
            Lg += weighted[:, p][:, lut2[p]]
        cell = np.argmax(Lg, axis=-1)
        W = 2 * half_w + 1
        res["cell"] = cell.astype(np.int32)
        res["max_Lf"] = Lg.max(-1)
        res["L"] = Lg
        res["xy"] = np.stack([(cell % W - half_w).astype(np.float32) / np.float32(grid_scale),
                              (half_h - cell // W).astype(np.float32) / np.float32(grid_scale)], -1)
    return res


def fixture17(N, window):
    """One mic row that needs 17 bits: -32768 everywhere except 32767 at the
    window's maximum (y = 65535 - floor(65535 / N) there, times the largest tap)."""
    row = np.full(N, -32768, np.int16)
    row[int(np.argmax(window))] = 32767
    return row
