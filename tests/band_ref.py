"""Float64 reference of band-limited GCC-PHAT (TEST INFRASTRUCTURE ONLY).

oracle/gcc_phat_oracle.py with one more factor: a real table w[0..N] over the
bins f_k = k fs / 2N of the 2N-point rfft,

    R_ij[k] = w[k] conj(U_i[k]) U_j[k],   r_ij = irfft(R_ij, 2N),

no renormalisation; lags, prior, gate and grid on these scores as the oracle
defines them.  band_weights is the mask of tdoa_band_weights (include/tdoa.h).
"""
import numpy as np

import gcc_phat_oracle as G


def band_weights(N, fs, lo, hi, taper=0.0):
    """w[k] = 1 for lo <= f_k <= hi, raised-cosine edges of width taper outside,
    0 elsewhere; float64 (the library rounds the same expressions to float)."""
    f = np.arange(N + 1, dtype=np.float64) * float(fs) / (2.0 * N)
    w = np.zeros(N + 1)
    w[(f >= lo) & (f <= hi)] = 1.0
    if taper > 0:
        up = (f > lo - taper) & (f < lo)
        w[up] = 0.5 * (1.0 - np.cos(np.pi * (f[up] - (lo - taper)) / taper))
        dn = (f > hi) & (f < hi + taper)
        w[dn] = 0.5 * (1.0 + np.cos(np.pi * (f[dn] - hi) / taper))
    return w


def gcc_phat_band(frames, S, window, w, lut=None, eps=1e-12, half_w=50, half_h=50, grid_scale=24.0):
    """gcc_phat_oracle.gcc_phat_batch with R_ij[k] scaled by w[k]; same keys."""
    x = G.prep(frames, window).astype(np.float64) / 32768.0
    B, M, N = x.shape
    L = 2 * N
    w = np.asarray(w, np.float64)
    assert w.shape == (N + 1,)
    X = np.fft.rfft(x, L, axis=-1)
    U = X / np.sqrt(X.real ** 2 + X.imag ** 2 + eps)
    pairs = [(i, j) for i in range(M) for j in range(i + 1, M)]
    P, K = len(pairs), 2 * S + 1
    s_idx = np.arange(-S, S + 1) % L
    scores = np.zeros((B, P, K))
    for p, (i, j) in enumerate(pairs):
        r = np.fft.irfft(w * (np.conj(U[:, i]) * U[:, j]), L, axis=-1)
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


def window_q15(N):
    """The context's default Q15 window (tdoa_create): the 1024-point DPSS(NW=2)
    table subsampled for N <= 1024, DPSS(N, 2) beyond."""
    import tdoa
    if N <= 1024:
        return tdoa.dpss_q15(1024)[:: 1024 // N].copy()
    return tdoa.dpss_q15(N)
