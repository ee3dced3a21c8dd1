"""The beamformer's rule (include/tdoa.h, "Listening") restated in numpy: the
reference tdoa_beam_host and the kernels are tested against.

Steering is np.float32 arithmetic, one operation per line in the order the
header states, and gives the delay codes (compared exactly).  The audio is the
same sum in float64 over the library's own float32 FIR values, with the
per-sample magnitude sum the tolerance is a multiple of:
    |audio - ref| <= gamma(M) * (1/M) sum_m sum_k |h| |x|,  gamma = (16 M + 2) 2^-24
-- the first-order bound of an fp32 sum of 16 M fused multiply-adds, one
rounding each, then the rounded 1/M and its product.  The FIR table is built
from np.sinc and np.i0; phase 0 is the exact unit tap the rule states (np.sinc
leaves 4e-17 at the other integers, which a zero-padded block would show).
"""
import numpy as np

HALF, PHASES, MAX_TARGETS = 8, 32, 8
TAPS = 2 * HALF
f32 = np.float32


def fir64():
    """h[32][16] in float64: tap k = -7..8 of phase q at [q][k + 7], each phase normalised to sum 1."""
    q = np.arange(PHASES, dtype=np.float64)[:, None]
    k = np.arange(-(HALF - 1), HALF + 1, dtype=np.float64)[None, :]
    x = k - q / PHASES
    sinc = np.sinc(x)
    sinc[0] = k[0] == 0  # at phase 0 x is an integer: the unit tap itself, without np.sinc's sin(pi k) residue
    w = sinc * np.i0(HALF * np.sqrt(np.maximum(1.0 - (x / HALF) ** 2, 0.0))) / np.i0(float(HALF))
    w[np.abs(x) > HALF] = 0.0
    return w / w.sum(axis=1, keepdims=True)


def fir():
    return fir64().astype(np.float32)


def gamma(M):
    return (16 * M + 2) * 2.0 ** -24


def dmax(mics, fs, c):
    """ceil(max |mic_i - mic_j| fs / c) + 1, in double from the float32 positions and speed."""
    m = np.asarray(mics, np.float32).astype(np.float64)
    d = m[:, None, :] - m[None, :, :]
    sep = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]).max()
    return int(np.ceil(sep * float(fs) / float(f32(c)))) + 1


def latency(mics, fs, c):
    D = dmax(mics, fs, c)
    return D + HALF, D


def _hypot3(x, y, z):
    xx = x * x
    yy = y * y
    zz = z * z
    s = xx + yy
    return np.sqrt(s + zz)


def steer(mics, fs, c, h, xy):
    """codes int32 [..., M] of targets xy [..., 2] (float32); a non-finite target gives -1s.
    Also returns valid bool [...]."""
    mics = np.asarray(mics, np.float32)
    xy = np.asarray(xy, np.float32)
    M, D = mics.shape[0], dmax(mics, fs, c)
    u, v = xy[..., 0], xy[..., 1]
    valid = np.isfinite(u) & np.isfinite(v)
    h, c, fsf = f32(h), f32(c), f32(fs)
    with np.errstate(all="ignore"):
        k = h / _hypot3(np.full_like(u, h), u, v)
        xs = u * k
        ys = v * k
        zs = h * k
        d = []
        for m in range(M):
            dx = xs - mics[m, 0]
            dy = ys - mics[m, 1]
            d.append(_hypot3(zs, dx, dy))
        dmin = d[0]
        for m in range(1, M):
            dmin = np.where(d[m] < dmin, d[m], dmin)
        codes = []
        for m in range(M):
            dd = d[m] - dmin
            ts = dd / c
            t = ts * fsf
            t32 = t * f32(32.0)
            r = np.floor(t32 + f32(0.5))
            assert r.dtype == np.float32
            top = f32(32 * D)
            # r >= 0 ? (r > top ? top : r) : 0, a NaN giving 0
            codes.append(np.nan_to_num(np.clip(r, f32(0), top), nan=0.0).astype(np.int64))
    codes = np.stack(codes, axis=-1).astype(np.int32)
    codes[~valid] = -1
    return codes, valid


def beam_signal(x, t_first, codes, n0, n1, D, table=None):
    """y[n], n in [n0, n1), of one valid target in float64, and the magnitude
    sum (1/M) sum sum |h| |x|: x [M][T] holds samples t_first .. t_first + T - 1
    of every mic (zero elsewhere), codes [M]."""
    h = (fir() if table is None else table).astype(np.float64)
    x = np.asarray(x, np.float64)
    M, T = x.shape
    n = n1 - n0
    L = n + D + TAPS - 1
    # pad[m][i] = x_m[n0 - 7 + i]
    pad = np.zeros((M, L))
    lo = n0 - (HALF - 1)
    a, b = max(lo, t_first), min(lo + L, t_first + T)
    if b > a:
        pad[:, a - lo:b - lo] = x[:, a - t_first:b - t_first]
    y, mag = np.zeros(n), np.zeros(n)
    for m in range(M):
        Dm, q = int(codes[m]) >> 5, int(codes[m]) & 31
        for kk in range(TAPS):
            seg = pad[m, Dm + kk:Dm + kk + n]
            y += h[q, kk] * seg
            mag += abs(h[q, kk]) * np.abs(seg)
    return y / M, mag / M


def beam(mics, fs, c, h, frames, xy, count=None):
    """The block form on frames [B][M][N]: audio float64 [B][Kt][N], its
    magnitude sums, delays int32 [B][Kt][M], active uint8 [B][Kt]."""
    frames = np.asarray(frames)
    xy = np.asarray(xy, np.float32)
    B, M, N = frames.shape
    Kt = xy.shape[1]
    D = dmax(mics, fs, c)
    codes, valid = steer(mics, fs, c, h, xy)
    if count is not None:
        valid = valid & (np.arange(Kt)[None, :] < np.asarray(count)[:, None])
        codes[~valid] = -1
    audio, mag = np.zeros((B, Kt, N)), np.zeros((B, Kt, N))
    table = fir()
    for b in range(B):
        for k in range(Kt):
            if valid[b, k]:
                audio[b, k], mag[b, k] = beam_signal(frames[b], 0, codes[b, k], 0, N, D, table)
    return {"audio": audio, "mag": mag, "delays": codes, "active": valid.astype(np.uint8)}


def close(got, ref, M):
    """got float32 within gamma(M) * mag of ref["audio"], everywhere."""
    return bool((np.abs(got.astype(np.float64) - ref["audio"]) <= gamma(M) * ref["mag"]).all())


def worst(got, ref, M):
    """Where got exceeds the bound by most, for an assertion's message."""
    err = np.abs(got.astype(np.float64) - ref["audio"]) - gamma(M) * ref["mag"]
    i = np.unravel_index(np.argmax(err), err.shape)
    return (f"{int((err > 0).sum())} samples beyond the bound; worst at {i}: got {got[i]!r}, reference "
            f"{ref['audio'][i]!r}, bound {gamma(M) * ref['mag'][i]!r}")
