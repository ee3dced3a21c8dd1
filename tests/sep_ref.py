"""The null-steering beamformer's rule (include/tdoa.h, "Separating") restated
in float64 numpy: the reference k_sep is tested against.

Per row (a block-form frame, a stream's last L samples), block length L, M
mics, Kt targets of which J are valid:
  1. steering: the delay codes of every target are beam_ref.steer's (the
     delay-and-sum rule's, compared exactly); tau = code / 32 samples;
  2. analysis: X_m[k] = sum_n g[n] x_m[n] e^{-2 pi i k n / L}, k = 0..L/2, with
     g the periodic sqrt-Hann window rounded to float32;
  3. steering vectors a_{j,m}[k] = exp(-2 pi i ((k code_{j,m}) mod 32 L) / (32 L));
  4. weights per bin: A [M][J] over the valid targets, G = A^H A + delta M I,
     W = (1 + delta) A G^-1, Y_j[k] = sum_m conj(W[m][j]) X_m[k];
  5. synthesis: y_j[n] = g[n] irfft(Y_j)[n] (the imaginary parts of bins 0 and
     L/2 are dropped, as numpy's irfft drops them); an invalid target's block
     is zeros, its codes -1, its active byte 0.
The streaming form overlap-adds: with L = 2 hop and e the clock, the block is
[e - L, e); audio = tail + y[:hop], tail = y[hop:].
"""
import numpy as np

import beam_ref as R

MAX_TARGETS = 4
LOADING = 1e-2


def window(L):
    """g[n] = sqrt(0.5 - 0.5 cos(2 pi n / L)) in double, rounded to float32."""
    n = np.arange(L, dtype=np.float64)
    return np.sqrt(0.5 - 0.5 * np.cos(2.0 * np.pi * n / L)).astype(np.float32)


def block_ok(L, D):
    """The circular-delay guard: L a power of two in 128..2048 and L >= 8 Dmax."""
    return 128 <= L <= 2048 and (L & (L - 1)) == 0 and L >= 8 * D


def steering_vectors(codes, L):
    """a [L/2 + 1][M][J] of codes int [J][M]: the phase reduced in integers."""
    k = np.arange(L // 2 + 1, dtype=np.int64)[:, None, None]
    p = (k * np.asarray(codes, np.int64).T[None, :, :]) % (32 * L)
    return np.exp(-2j * np.pi * p.astype(np.float64) / (32 * L))


def weights(codes, L, loading=LOADING):
    """W [L/2 + 1][M][J] = (1 + delta) A (A^H A + delta M I)^-1."""
    A = steering_vectors(codes, L)
    M, J = A.shape[1], A.shape[2]
    AH = np.conj(np.transpose(A, (0, 2, 1)))
    G = AH @ A + loading * M * np.eye(J)[None]
    return (1.0 + loading) * (A @ np.linalg.inv(G))


def spectra(x, L):
    """X [M][L/2 + 1] of x [M][L] (float64 samples): windowed rfft."""
    return np.fft.rfft(window(L).astype(np.float64)[None, :] * np.asarray(x, np.float64), axis=1)


def synth(Y, L):
    """y [J][L] of Y [J][L/2 + 1]."""
    return window(L).astype(np.float64)[None, :] * np.fft.irfft(Y, n=L, axis=1)


def block(x, codes, valid, loading=LOADING):
    """One row: x [M][L], codes int [Kt][M], valid bool [Kt] -> y float64 [Kt][L]."""
    x = np.asarray(x, np.float64)
    M, L = x.shape
    Kt = len(valid)
    y = np.zeros((Kt, L))
    idx = np.flatnonzero(valid)
    if idx.size:
        W = weights(np.asarray(codes)[idx], L, loading)          # [K][M][J]
        X = spectra(x, L).T                                       # [K][M]
        Y = np.einsum("kmj,km->jk", np.conj(W), X)
        y[idx] = synth(Y, L)
    return y


def das_block(x, codes):
    """The frequency-domain delay-and-sum of one target: (1/M) sum_m conj(a_m) X_m, synthesised."""
    x = np.asarray(x, np.float64)
    M, L = x.shape
    a = steering_vectors(np.asarray(codes)[None, :], L)[:, :, 0]  # [K][M]
    Y = (np.conj(a) * spectra(x, L).T).sum(axis=1) / M
    return synth(Y[None, :], L)[0]


def targets(mics, fs, c, h, xy, count=None, valid=None):
    """codes int32 [..., Kt, M] (-1 invalid) and valid bool [..., Kt] of xy [..., Kt, 2]."""
    xy = np.asarray(xy, np.float32)
    codes, ok = R.steer(mics, fs, c, h, xy)
    if count is not None:
        ok = ok & (np.arange(xy.shape[-2])[None, :] < np.asarray(count)[:, None])
    if valid is not None:
        ok = ok & np.asarray(valid, bool)
    codes[~ok] = -1
    return codes, ok


def sep(mics, fs, c, h, frames, xy, count=None, loading=LOADING):
    """The block form on frames [B][M][L]: audio float64 [B][Kt][L], delays
    int32 [B][Kt][M], active uint8 [B][Kt]."""
    frames = np.asarray(frames)
    B, M, L = frames.shape
    assert block_ok(L, R.dmax(mics, fs, c))
    codes, ok = targets(mics, fs, c, h, xy, count)
    audio = np.stack([block(frames[b], codes[b], ok[b], loading) for b in range(B)]) if B else np.zeros(
        (0, codes.shape[1], L))
    return {"audio": audio, "delays": codes, "active": ok.astype(np.uint8)}


class Stream:
    """The streaming form over a capture history hist [S][T][M] (what the
    ring held): hop h = 1, 2, .. reads [e - L, e), e = h hop, L = 2 hop."""

    def __init__(self, mics, fs, c, h, hist, hop, Kt, loading=LOADING, block_fn=None, dtype=np.float64):
        """block_fn / dtype: another evaluation of one block (the tests' complex64
        restatement, with float32 tails) in place of block()."""
        self.geo = (mics, fs, c, h)
        self.hist, self.hop, self.Kt, self.loading = np.asarray(hist), hop, Kt, loading
        self.block_fn, self.dtype = block if block_fn is None else block_fn, dtype
        assert block_ok(2 * hop, R.dmax(mics, fs, c))
        self.reset()

    def reset(self):
        self.tail = np.zeros((self.hist.shape[0], self.Kt, self.hop), self.dtype)

    def step(self, e, xy, count=None, valid=None):
        """The hop whose clock is e: (block_start, audio float64 [S][Kt][hop], delays, active)."""
        S, T, M = self.hist.shape
        hop, L = self.hop, 2 * self.hop
        codes, ok = targets(*self.geo, xy, count, valid)
        audio = np.zeros((S, self.Kt, hop), self.dtype)
        for s in range(S):
            x = np.zeros((M, L))
            lo = max(e - L, 0)
            x[:, lo - (e - L):] = self.hist[s, lo:e].T
            y = self.block_fn(x, codes[s], ok[s], self.loading)
            audio[s] = self.tail[s] + y[:, :hop]
            self.tail[s] = y[:, hop:]
        return e - L, audio, codes, ok.astype(np.uint8)


def rel_l2(got, ref):
    """|got - ref|_2 / |ref|_2 over the last axis (0 where both are zero)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    num = np.sqrt(((got - ref) ** 2).sum(axis=-1))
    den = np.sqrt((ref ** 2).sum(axis=-1))
    return np.where(den > 0, num / np.where(den > 0, den, 1.0), np.where(num > 0, np.inf, 0.0))


# ---------------------------------------------------------------- the two-source scene
SCENE_FS, SCENE_L = 16000, 256
SCENE_POINTS = ((-1.5, 0.4), (1.2, -0.9))  # plane coordinates of talkers A and B


def band_noise(rng, T, lo, hi):
    """White noise band-limited to [lo, hi) cycles per sample, unit power."""
    X = np.fft.rfft(rng.normal(0, 1, T))
    f = np.arange(X.size) / T
    X[(f < lo) | (f >= hi)] = 0
    s = np.fft.irfft(X, n=T)
    return s / np.sqrt((s ** 2).mean())


def delayed(s, tau):
    """s delayed by tau samples (fractional; circular over the whole signal)."""
    T = s.size
    k = np.arange(T // 2 + 1)
    return np.fft.irfft(np.fft.rfft(s) * np.exp(-2j * np.pi * k * tau / T), n=T)


def true_delays(mics, fs, c, h, point):
    m64 = np.asarray(mics, np.float64)
    u, v = point
    k = h / np.sqrt(h * h + u * u + v * v)
    p = np.array([u * k, v * k, h * k])
    d = np.sqrt(p[2] ** 2 + (p[0] - m64[:, 0]) ** 2 + (p[1] - m64[:, 1]) ** 2)
    return (d - d.min()) / c * fs


def scene(mics, fs, c, h, nblocks, L, seed=5, amp=6000.0, band=(0.04, 0.45)):
    """Two independent band-limited noise sources at SCENE_POINTS, each heard
    by every mic at its true fractional delay: per source the int16-scaled mic
    signals alone, float64 [2][M][T], T = (nblocks + 1) L / 2.  The mix is
    their sum; a linear beamformer's output of the mix is the sum of its
    outputs of the parts, which is how the interferer-to-target ratios are
    measured."""
    rng = np.random.default_rng(seed)
    T = (nblocks + 1) * L // 2
    parts = []
    for point in SCENE_POINTS:
        s = amp * band_noise(rng, T, *band)
        tau = true_delays(mics, fs, c, h, point)
        parts.append(np.stack([delayed(s, t) for t in tau]))
    return np.stack(parts)


def scene_frames(parts, L):
    """Half-overlapped blocks [2][nblocks][M][L] of the parts, rounded to int16 counts."""
    T = parts.shape[-1]
    nb = 2 * T // L - 1
    fr = np.stack([parts[:, :, i * L // 2:i * L // 2 + L] for i in range(nb)], axis=1)
    return np.rint(fr).astype(np.int16)


def ola(blocks):
    """Overlap-add of half-overlapped blocks [nb][..., L] -> [..., (nb + 1) L / 2]."""
    nb, L = blocks.shape[0], blocks.shape[-1]
    out = np.zeros(blocks.shape[1:-1] + ((nb + 1) * L // 2,))
    for i in range(nb):
        out[..., i * L // 2:i * L // 2 + L] += blocks[i]
    return out


def ratio_db(p_interferer, p_target):
    return 10.0 * np.log10(p_interferer / p_target)
