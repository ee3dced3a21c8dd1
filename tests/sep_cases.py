"""Shared pieces of the separator's tests (test_sep_cpu.py, test_gpu_sep.py):
the geometries whose Dmax fits the block lengths, the block cases, and the
complex64 restatement of the rule whose own error against float64 sets the
audio tolerance.

The tolerance.  The error of an fp32 evaluation of the rule grows with the
conditioning of G = A^H A + delta M I, which depends on the targets and the
bin: no closed form.  So the same rule is evaluated in float32 / complex64
numpy (restate()) -- float32 window product, a complex64 radix-2 FFT written
out here (numpy's own FFT may run in double), steering vectors rounded to
complex64, np.linalg.solve in complex64, a complex64 inverse FFT -- and its
relative L2 error against the float64 reference, per (row, target), times
MARGIN = 8, is what k_sep's output may differ by: the margin covers a different
but equally valid fp32 operation order in the FFT and the solve.  The bound
never looks at the kernel's output.
"""
import numpy as np

import beam_ref as R
import sep_ref as S

H = 1.2
MARGIN = 8.0
GRID = 50 / 24.0
FS = 16000
C = 343.0


def circle(M, r):
    a = 2 * np.pi * np.arange(M) / M
    return np.stack([r * np.cos(a), r * np.sin(a)], axis=1).astype(np.float32)


# M -> mics (None: the reference triangle).  At 16 kHz the widest, the 8-mic
# circle of radius 0.15 m, has Dmax = 15: 8 Dmax <= 128.
MICS = {2: np.array([[-0.1, 0.0], [0.1, 0.0]], np.float32), 3: None, 5: circle(5, 0.12), 6: circle(6, 0.13),
        7: circle(7, 0.14), 8: circle(8, 0.15)}

# (M, L, Kt): the smallest shapes that reach each path -- one mic pair / an odd
# mic / more target pairs than mic pairs (2, 128, 2 has one of each; 3, 256, 4
# has two target pairs over two mic pairs, the second with an odd mic), an odd
# Kt, four full pairs, a radix-2 tail (128) and none (256), and the LDS maximum.
# From L = 512 on a thread owns several bins (k, k + 256, ..) and the FFT's
# butterflies fill (1024: n / 4 = 256 threads exactly) or exceed (2048) one pass
# of the workgroup; log2 L is odd at 512 and 2048 (radix-2 tail), even at 1024.
# Each of those lengths with an invalid target (the counts of block_case), an
# odd mic, an odd Kt, one target, more target pairs than mic pairs, and above
# 64 KiB of LDS with an odd mic (7, 2048, 4).
BLOCK_SHAPES = [(2, 128, 2), (3, 128, 2), (3, 256, 4), (5, 256, 3), (8, 256, 4),
                (2, 512, 4), (5, 512, 3), (7, 512, 4), (6, 1024, 3), (8, 1024, 4), (2, 1024, 1), (7, 2048, 4),
                (5, 2048, 3)]
LDS_MAX_SHAPE = (8, 2048, 4)


def block_case(mics, B, L, Kt, seed):
    """frames int16 [B][M][L], xy float32 [B][Kt][2], count int32 [B]: random
    targets over the grid; count = 0, 1, 3 and 4 (clipped to Kt) across the
    first rows where B allows, all Kt elsewhere."""
    rng = np.random.default_rng(seed)
    M = mics.shape[0]
    frames = rng.integers(-20000, 20001, (B, M, L)).astype(np.int16)
    xy = rng.uniform(-GRID, GRID, (B, Kt, 2)).astype(np.float32)
    count = np.full(B, Kt, np.int32)
    for b, cnt in zip(range(B), (0, 1, 3, 4)):
        if B >= 4:
            count[b] = min(cnt, Kt)
    return frames, xy, count


# ---------------------------------------------------------------- the complex64 restatement
def fft_c64(x, inverse=False):
    """Radix-2 decimation-in-time FFT over the last axis in complex64 (no 1/L)."""
    x = np.asarray(x, np.complex64)
    L = x.shape[-1]
    bits = L.bit_length() - 1
    rev = np.array([int(format(i, f"0{bits}b")[::-1], 2) for i in range(L)])
    y = x[..., rev].copy()
    sign = 2.0 if inverse else -2.0
    h = 1
    while h < L:
        w = np.exp(sign * 1j * np.pi * np.arange(h) / (2 * h)).astype(np.complex64)
        y = y.reshape(y.shape[:-1] + (L // (2 * h), 2, h))
        t = (y[..., 1, :] * w).astype(np.complex64)
        y = np.stack([y[..., 0, :] + t, y[..., 0, :] - t], axis=-2).astype(np.complex64)
        y = y.reshape(y.shape[:-3] + (L,))
        h *= 2
    return y


def restate(x, codes, valid, loading):
    """sep_ref.block in float32 / complex64: x [M][L], codes [Kt][M], valid [Kt] -> float32 [Kt][L]."""
    x = np.asarray(x, np.float32)
    M, L = x.shape
    Kt = len(valid)
    y = np.zeros((Kt, L), np.float32)
    idx = np.flatnonzero(valid)
    if not idx.size:
        return y
    g = S.window(L)
    X = fft_c64(g[None, :] * x)[:, :L // 2 + 1].T                                  # [K][M]
    A = S.steering_vectors(np.asarray(codes)[idx], L).astype(np.complex64)          # [K][M][J]
    J = idx.size
    AH = np.conj(np.transpose(A, (0, 2, 1)))
    G = (AH @ A + (np.float32(loading) * np.float32(M)) * np.eye(J, dtype=np.complex64)[None]).astype(np.complex64)
    b = (AH @ X[:, :, None]).astype(np.complex64)
    assert G.dtype == np.complex64 and b.dtype == np.complex64
    Y = ((np.float32(1.0) + np.float32(loading)) * np.linalg.solve(G, b)[:, :, 0]).astype(np.complex64)  # [K][J]
    Y[0].imag = 0
    Y[L // 2].imag = 0
    full = np.concatenate([Y, np.conj(Y[L // 2 - 1:0:-1])], axis=0).T              # [J][L], Hermitian
    z = fft_c64(full, inverse=True)
    y[idx] = g[None, :] * (z.real.astype(np.float32) * np.float32(1.0 / L))
    return y


def tolerance(frames, codes, valid, ref_audio, loading):
    """MARGIN times the restatement's relative L2 error per (row, target), [B][Kt]."""
    B = frames.shape[0]
    err = np.stack([S.rel_l2(restate(frames[b], codes[b], valid[b], loading), ref_audio[b]) for b in range(B)])
    return MARGIN * err, err
