"""Shared shapes and generators of the beamformer tests (test_beam_cpu.py,
test_gpu_beam.py): three geometries, block cases that contain every kind of
target the rule distinguishes, the known-answer scene and the capture
histories of the streaming runs.
"""
import numpy as np

import beam_ref as R

H = 1.2  # height_offset (the default)
GRID = 50 / 24.0  # the default grid's corner, metres

# The 4-mic square has its corners on the axes, 0.25 m across, and fs / c chosen
# so that the diagonal is exactly 30 samples (0.25 * 40800 / 340): Dmax = 31, and
# a target on the horizon along a diagonal reaches the code 960 = 32 Dmax - 32.
GEOMS = {
    "triangle": dict(mics=None, M=3, fs=50000, c=343.0),
    "square": dict(mics=np.array([[0.125, 0], [0, 0.125], [-0.125, 0], [0, -0.125]], np.float32), M=4, fs=40800,
                   c=340.0),
    "circle": dict(mics=np.stack([0.15 * np.cos(2 * np.pi * np.arange(8) / 8),
                                  0.15 * np.sin(2 * np.pi * np.arange(8) / 8)], axis=1).astype(np.float32), M=8,
                   fs=50000, c=343.0),
}


def geometry(name):
    """(tdoa BeamGeometry, mics float32 [M][2], fs, c) of a named geometry."""
    import tdoa
    g = GEOMS[name]
    bg = tdoa.beam_geometry(mic_xy=g["mics"], num_mics=g["M"], sample_rate_hz=g["fs"], speed_of_sound=g["c"],
                            height_offset=H)
    mics = np.array(list(bg.mic_xy), np.float32).reshape(8, 2)[:g["M"]].copy()
    return bg, mics, g["fs"], g["c"]


def block_case(mics, B, N, Kt, seed, horizon=False):
    """frames int16 [B][M][N], xy float32 [B][Kt][2], count int32 [B] (B >= 5):
    random targets over the grid, and on fixed rows a target above mic 0, one
    at the grid's corner, a NaN, a count of 0, a short count, full-scale frames
    and -- horizon -- a target on the horizon along the first mic's axis."""
    rng = np.random.default_rng(seed)
    M = mics.shape[0]
    frames = rng.integers(-20000, 20001, (B, M, N)).astype(np.int16)
    frames[1] = rng.choice(np.array([-32767, 32767], np.int16), (M, N))
    xy = rng.uniform(-GRID, GRID, (B, Kt, 2)).astype(np.float32)
    count = np.full(B, Kt, np.int32)
    xy[0, 0] = mics[0]
    xy[1, 0] = (-GRID, GRID)
    xy[2, Kt - 1] = (np.nan, 0.5)
    count[3] = 0
    count[4] = Kt - 1
    if horizon:
        xy[4, 0] = (1e6, 0.0)
    return frames, xy, count


# ---------------------------------------------------------------- known answer
def scene(mics, fs, c, N, point, seed, amp=8000.0):
    """A source at plane point `point` heard by every mic at its true fractional
    delay, plus white noise of the signal's power per mic: (frames int16
    [M][N], clean float64 [N] -- the source as the nearest mic hears it).  The
    signal is three sinusoids below fs / 8 whose amplitudes sum to amp."""
    rng = np.random.default_rng(seed)
    m64 = np.asarray(mics, np.float64)
    u, v = point
    k = H / np.sqrt(H * H + u * u + v * v)
    p = np.array([u * k, v * k, H * k])
    d = np.sqrt(p[2] ** 2 + (p[0] - m64[:, 0]) ** 2 + (p[1] - m64[:, 1]) ** 2)
    tau = (d - d.min()) / c * fs  # samples
    freqs = np.array([1 / 9.0, 1 / 13.0, 1 / 21.0])  # cycles per sample
    phases = rng.uniform(0, 2 * np.pi, 3)
    a = amp / 3

    def s(t):
        return sum(a * np.sin(2 * np.pi * f * t + ph) for f, ph in zip(freqs, phases))
    t = np.arange(N, dtype=np.float64)
    power = 3 * a * a / 2
    frames = np.stack([s(t - tau[m]) + rng.normal(0, np.sqrt(power), N) for m in range(len(tau))])
    return np.rint(frames).astype(np.int16), s(t)


# ---------------------------------------------------------------- streaming
def history(S, T, M, dtype, seed):
    """Capture history [S][T][M]: per stream a few sinusoids per mic plus noise,
    uint8 around 128 or int16."""
    rng = np.random.default_rng(seed)
    t = np.arange(T)[None, :, None]
    f = rng.uniform(0.01, 0.1, (S, 1, M))
    ph = rng.uniform(0, 2 * np.pi, (S, 1, M))
    x = np.sin(2 * np.pi * f * t + ph) + 0.3 * rng.normal(0, 1, (S, T, M))
    if np.dtype(dtype) == np.uint8:
        return np.clip(np.rint(128 + 60 * x), 0, 255).astype(np.uint8)
    return np.clip(np.rint(9000 * x), -32767, 32767).astype(np.int16)


def stream_ref(mics, fs, c, hist, xy, valid, hop, h):
    """Hop h (1-based) of the streaming form on the whole history hist
    [S][T][M] with targets xy [S][Kt][2] / valid [S][Kt]: block_start and, per
    stream and target, the block's float64 audio, magnitude sums, codes."""
    S, T, M = hist.shape
    Kt = xy.shape[1]
    A, D = R.latency(mics, fs, c)
    e = h * hop
    n0 = e - hop - A
    codes, fin = R.steer(mics, fs, c, H, xy)
    ok = fin & valid
    codes[~ok] = -1
    audio, mag = np.zeros((S, Kt, hop)), np.zeros((S, Kt, hop))
    table = R.fir()
    for s in range(S):
        x = hist[s, :e].T  # what the ring holds of the stream at this hop
        for k in range(Kt):
            if ok[s, k]:
                audio[s, k], mag[s, k] = R.beam_signal(x, 0, codes[s, k], n0, n0 + hop, D, table)
    return n0, {"audio": audio, "mag": mag, "delays": codes, "active": ok.astype(np.uint8)}
