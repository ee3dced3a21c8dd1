"""Synthetic multi-mic frames of the BASELINE shapes.

ADC-like frames: int16 holding u8 samples around 128 (dma_sampler.c:17-20,
sample_compute.h:67-69 read 8-bit ADC bytes into sample_t).  A broadband
N(0, src_std) source reaches mic m delayed by an integer tau_m taken from the
grid LUT of a random cell (tau_0 = 0, tau_m = LUT_(0,m)[cell] - S), plus
N(0, noise_std) noise, rounded and clipped to [0, 255].

`full_range` frames are uniform over all of int16 and exercise the
reference's int16 wrap paths (rolling_buffer.c:65-66, buffer.c:16).
"""
from __future__ import annotations

import numpy as np
import torch

SEEDS = {1: 0x5EED0001, 2: 0x5EED0002, 3: 0x5EED0003, 4: 0x5EED0004, 5: 0x5EED0005}


def adc_frames(B: int, M: int, N: int, lut: np.ndarray, S: int, seed: int,
               device: str | torch.device = "cpu", src_std: float = 40.0,
               noise_std: float = 8.0, mean: float = 128.0):
    """Returns (frames int16 [B][M][N], cells int64 [B], tau int64 [B][M])."""
    dev = torch.device(device)
    g = torch.Generator(device=dev)
    g.manual_seed(int(seed))
    P, G = lut.shape[0], lut.reshape(lut.shape[0], -1).shape[1]
    lut_t = torch.as_tensor(lut.reshape(P, -1).astype(np.int64), device=dev)
    cells = torch.randint(0, G, (B,), generator=g, device=dev)
    tau = torch.zeros((B, M), dtype=torch.int64, device=dev)
    for m in range(1, M):
        tau[:, m] = lut_t[m - 1][cells] - S  # pair (0, m) is index m-1
    pad = S + 1
    src = torch.randn((B, N + 2 * pad), generator=g, device=dev) * src_std
    idx = torch.arange(N, device=dev).view(1, 1, N) + pad - tau.view(B, M, 1)
    x = torch.gather(src.view(B, 1, -1).expand(B, M, -1), 2, idx)
    x = x + torch.randn((B, M, N), generator=g, device=dev) * noise_std + mean
    frames = torch.clamp(torch.round(x), 0, 255).to(torch.int16)
    return frames.contiguous(), cells, tau


def multi_source_frames(B: int, M: int, N: int, lut: np.ndarray, S: int, seed: int,
                        num_sources: int = 2, min_sep: int = 25, src_std=(40.0, 32.0),
                        noise_std: float = 4.0, mean: float = 128.0,
                        device: str | torch.device = "cpu", grid_W: int | None = None):
    """Frames with `num_sources` simultaneous independent broadband sources,
    built like adc_frames: source k sits at a random grid cell, at least
    `min_sep` cells (Chebyshev) from every other source of its frame, and
    reaches mic m delayed by the integer tau taken from the LUT; the sources
    add, plus N(0, noise_std) noise, rounded and clipped to [0, 255].
    src_std[k] is source k's level (the last entry repeats).  grid_W: the
    grid's width in cells (default: lut's last axis if it is [P][H][W], else
    a square grid).
    Returns (frames int16 [B][M][N], cells int64 [B][num_sources],
    tau int64 [B][num_sources][M])."""
    dev = torch.device(device)
    g = torch.Generator(device=dev)
    g.manual_seed(int(seed))
    P = lut.shape[0]
    G = lut.reshape(P, -1).shape[1]
    if grid_W is None:
        grid_W = lut.shape[2] if lut.ndim == 3 else int(round(G ** 0.5))
    assert G % grid_W == 0, "grid_W does not divide the LUT's cells"
    lut_t = torch.as_tensor(lut.reshape(P, -1).astype(np.int64), device=dev)
    cells = torch.zeros((B, num_sources), dtype=torch.int64, device=dev)
    for k in range(num_sources):
        todo = torch.ones(B, dtype=torch.bool, device=dev)
        for _ in range(1000):
            draw = torch.randint(0, G, (B,), generator=g, device=dev)
            cells[:, k] = torch.where(todo, draw, cells[:, k])
            todo = torch.zeros(B, dtype=torch.bool, device=dev)
            for j in range(k):
                dx = (cells[:, k] % grid_W - cells[:, j] % grid_W).abs()
                dy = (cells[:, k] // grid_W - cells[:, j] // grid_W).abs()
                todo |= torch.maximum(dx, dy) < min_sep
            if not bool(todo.any()):
                break
        else:
            raise ValueError("min_sep leaves no room for the sources on this grid")
    tau = torch.zeros((B, num_sources, M), dtype=torch.int64, device=dev)
    for m in range(1, M):
        tau[:, :, m] = lut_t[m - 1][cells] - S  # pair (0, m) is index m-1
    std = [float(src_std[min(k, len(src_std) - 1)]) for k in range(num_sources)]
    pad = S + 1
    x = torch.zeros((B, M, N), device=dev)
    for k in range(num_sources):
        src = torch.randn((B, N + 2 * pad), generator=g, device=dev) * std[k]
        idx = torch.arange(N, device=dev).view(1, 1, N) + pad - tau[:, k].reshape(B, M, 1)
        x = x + torch.gather(src.view(B, 1, -1).expand(B, M, -1), 2, idx)
    x = x + torch.randn((B, M, N), generator=g, device=dev) * noise_std + mean
    frames = torch.clamp(torch.round(x), 0, 255).to(torch.int16)
    return frames.contiguous(), cells, tau


def interferer_frames(B: int, M: int, N: int, fs: int, S: int, seed: int, target_lags,
                      interferer_lags, target_band=(1500, 5500), interferer_band=(12000, 24000),
                      amp: float = 40, noise: float = 2, device: str | torch.device = "cpu"):
    """A band-limited target under a band-limited interferer of the same level
    (the band-limited GCC-PHAT scenario).  Per frame two independent Gaussian
    noise signals of N + 4S samples are band-limited in the frequency domain
    (bins of the (N + 4S)-point rfft outside the band zeroed) and scaled to unit
    variance; mic m reads the target delayed by the integer target_lags[m] and
    the interferer by interferer_lags[m] (|lag| <= 2S), each times `amp`, plus
    N(0, noise) white noise, offset by 128, rounded and clipped to [0, 255].
    Draw order (numpy default_rng(seed)): target [B][N + 4S], interferer
    [B][N + 4S], white noise [B][M][N].
    Returns (frames int16 [B][M][N] on `device`, target pair lags int32 [P],
    interferer pair lags int32 [P]); pair (i, j) in lexicographic order has lag
    lags[j] - lags[i], the sign of the engines' best lags."""
    rng = np.random.default_rng(int(seed))
    T, pad = N + 4 * S, 2 * S
    f = np.arange(T // 2 + 1) * (float(fs) / T)

    def band_noise(band):
        X = np.fft.rfft(rng.standard_normal((B, T)), axis=-1)
        X[:, (f < band[0]) | (f > band[1])] = 0.0
        x = np.fft.irfft(X, T, axis=-1)
        return x / x.std(axis=-1, keepdims=True)

    sig = [band_noise(target_band), band_noise(interferer_band)]
    lags = [np.asarray(target_lags, np.int64)[:M], np.asarray(interferer_lags, np.int64)[:M]]
    x = rng.standard_normal((B, M, N)) * float(noise) + 128.0
    n = np.arange(N)
    for s, lag in zip(sig, lags):
        assert lag.size == M and np.abs(lag).max() <= pad, "one lag per mic, |lag| <= 2S"
        for m in range(M):
            x[:, m] += float(amp) * s[:, pad + n - lag[m]]
    frames = torch.from_numpy(np.clip(np.rint(x), 0, 255).astype(np.int16)).to(torch.device(device))
    pair = [np.array([lag[j] - lag[i] for i in range(M) for j in range(i + 1, M)], np.int32) for lag in lags]
    return frames.contiguous(), pair[0], pair[1]


def pcm16_frames(B: int, M: int, N: int, S: int, seed: int, delays, src_std: float = 3000.0,
                 noise_std: float = 600.0, dc=None, device: str | torch.device = "cpu"):
    """Full-range 16-bit frames of one white source (the 16-bit PCM scenario).
    Per frame a Gaussian source of N + 4S samples and standard deviation
    `src_std` counts; mic m reads it delayed by the integer delays[m]
    (|delay| <= 2S), plus N(0, noise_std) white noise, plus the offset dc[m]
    (default 0), rounded and clipped to int16.
    Draw order (numpy default_rng(seed)): source [B][N + 4S], noise [B][M][N].
    Returns (frames int16 [B][M][N] on `device`, pair lags int32 [P]); pair
    (i, j) in lexicographic order has lag delays[j] - delays[i], the sign of the
    engines' best lags."""
    rng = np.random.default_rng(int(seed))
    T, pad = N + 4 * S, 2 * S
    src = rng.standard_normal((B, T)) * float(src_std)
    x = rng.standard_normal((B, M, N)) * float(noise_std)
    lag = np.asarray(delays, np.int64)[:M]
    assert lag.size == M and np.abs(lag).max() <= pad, "one delay per mic, |delay| <= 2S"
    off = np.zeros(M) if dc is None else np.asarray(dc, np.float64)[:M]
    assert off.size == M, "one offset per mic"
    n = np.arange(N)
    for m in range(M):
        x[:, m] += src[:, pad + n - lag[m]] + off[m]
    frames = torch.from_numpy(np.clip(np.rint(x), -32768, 32767).astype(np.int16)).to(torch.device(device))
    pair = np.array([lag[j] - lag[i] for i in range(M) for j in range(i + 1, M)], np.int32)
    return frames.contiguous(), pair


def full_range_frames(B: int, M: int, N: int, seed: int, device="cpu") -> torch.Tensor:
    dev = torch.device(device)
    g = torch.Generator(device=dev)
    g.manual_seed(int(seed))
    return torch.randint(-32768, 32768, (B, M, N), generator=g, device=dev,
                         dtype=torch.int32).to(torch.int16).contiguous()


def adc_stream(S: int, T: int, M: int, lut: np.ndarray, max_shift: int, seed: int,
               device: str | torch.device = "cpu", burst_len: int = 700,
               gap: tuple = (1500, 3500), src_std: float = 40.0, noise_std: float = 0.5,
               mean: float = 128.0) -> torch.Tensor:
    """Config 5 capture bytes u8 [S][T][M] (round-robin per sample, dma_sampler.c:17-23).

    Each stream has a stationary source at a random grid cell emitting
    broadband bursts of `burst_len` samples separated by random gaps; mic m
    hears it delayed by tau_m (the cell's LUT lags), over a quiet noise floor.
    The reference triggers as a burst leaves the newer half of the ring."""
    dev = torch.device(device)
    g = torch.Generator(device=dev)
    g.manual_seed(int(seed))
    P, G = lut.shape[0], lut.reshape(lut.shape[0], -1).shape[1]
    lut_t = torch.as_tensor(lut.reshape(P, -1).astype(np.int64), device=dev)
    cells = torch.randint(0, G, (S,), generator=g, device=dev)
    tau = torch.zeros((S, M), dtype=torch.int64, device=dev)
    for m in range(1, M):
        tau[:, m] = lut_t[m - 1][cells] - max_shift
    pad = max_shift + 1
    TT = T + 2 * pad
    nb = TT // gap[0] + 2
    gaps = torch.randint(gap[0], gap[1], (S, nb), generator=g, device=dev)
    starts = torch.cumsum(gaps, 1) - gaps[:, :1] + torch.randint(0, gap[0], (S, 1), generator=g,
                                                                 device=dev)
    edge = torch.zeros((S, TT + burst_len + 1), dtype=torch.int32, device=dev)
    ok = starts < TT
    st = torch.where(ok, starts, torch.full_like(starts, TT))
    edge.scatter_add_(1, st, ok.to(torch.int32))
    edge.scatter_add_(1, st + burst_len, -ok.to(torch.int32))
    env = (torch.cumsum(edge, 1)[:, :TT] > 0).to(torch.float32)
    y = torch.randn((S, TT), generator=g, device=dev) * src_std * env
    idx = torch.arange(T, device=dev).view(1, 1, T) + pad - tau.view(S, M, 1)
    x = torch.gather(y.view(S, 1, -1).expand(S, M, -1), 2, idx)
    x = x + torch.randn((S, M, T), generator=g, device=dev) * noise_std + mean
    b = torch.clamp(torch.round(x), 0, 255).to(torch.uint8)
    return b.permute(0, 2, 1).contiguous()


def pcm16_stream(S: int, T: int, M: int, lut: np.ndarray, max_shift: int, seed: int,
                 device: str | torch.device = "cpu", burst_len: int = 700,
                 gap: tuple = (1500, 3500), src_std: float = 3000.0, noise_std: float = 30.0,
                 dc=None) -> torch.Tensor:
    """adc_stream's burst scenario as 16-bit PCM: int16 [S][T][M] on `device`.

    Each stream has a stationary source at a random grid cell emitting
    N(0, src_std) bursts of `burst_len` samples separated by random gaps; mic m
    hears it delayed by tau_m (tau_0 = 0, tau_m = LUT_(0,m)[cell] - max_shift)
    over N(0, noise_std) noise, plus the offset dc[m] counts (default 0; one
    per mic, shared by the streams), rounded and clipped to int16.
    Draw order (numpy default_rng(seed)): cells [S]; gaps [S][nb] uniform over
    [gap[0], gap[1]) with nb = (T + 2 pad) // gap[0] + 2 and pad = max_shift + 1;
    the first burst's start [S] uniform over [0, gap[0]); source [S][T + 2 pad];
    noise [S][M][T].  Burst b of a stream starts at first + gaps[:b].sum() on
    the source's own time axis, which is the capture's shifted by pad."""
    rng = np.random.default_rng(int(seed))
    P = lut.shape[0]
    lut2 = np.asarray(lut).reshape(P, -1).astype(np.int64)
    cells = rng.integers(0, lut2.shape[1], S)
    tau = np.zeros((S, M), np.int64)
    for m in range(1, M):
        tau[:, m] = lut2[m - 1][cells] - max_shift  # pair (0, m) is index m-1
    pad = max_shift + 1
    TT = T + 2 * pad
    nb = TT // gap[0] + 2
    gaps = rng.integers(gap[0], gap[1], (S, nb))
    first = rng.integers(0, gap[0], S)
    starts = first[:, None] + np.cumsum(gaps, 1) - gaps
    env = np.zeros((S, TT + 1), np.int32)
    for s in range(S):
        st = starts[s][starts[s] < TT]
        np.add.at(env[s], st, 1)
        np.add.at(env[s], np.minimum(st + burst_len, TT), -1)
    env = np.cumsum(env, 1)[:, :TT] > 0
    y = rng.standard_normal((S, TT)) * float(src_std) * env
    x = rng.standard_normal((S, M, T)) * float(noise_std)
    off = np.zeros(M) if dc is None else np.asarray(dc, np.float64)[:M]
    assert off.size == M, "one offset per mic"
    t = np.arange(T)
    for m in range(M):
        x[:, m] += np.take_along_axis(y, pad + t[None, :] - tau[:, m:m + 1], 1) + off[m]
    cap = np.clip(np.rint(x), -32768, 32767).astype(np.int16).transpose(0, 2, 1)
    return torch.from_numpy(np.ascontiguousarray(cap)).to(torch.device(device))


def square_mics(side: float = 0.15) -> np.ndarray:
    """Config 3: 4-mic square centred on the origin."""
    h = side / 2
    return np.array([[-h, -h], [h, -h], [h, h], [-h, h]], np.float32)


def circle_mics(M: int = 8, radius: float = 0.15) -> np.ndarray:
    """Config 4: M-mic circle centred on the origin."""
    a = 2 * np.pi * np.arange(M) / M
    return np.stack([radius * np.cos(a), radius * np.sin(a)], -1).astype(np.float32)
