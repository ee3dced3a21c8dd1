"""Band-limited GCC-PHAT, the host side (no kernel runs here): the band mask of
tdoa_band_weights against the float64 formula (tests/band_ref.py), its
argument checks, and the scenario the feature exists for -- a band-limited
target under a louder-per-bin interferer elsewhere in the band -- on the
float64 reference alone."""
import ctypes as C

import numpy as np
import pytest

import band_ref
import gcc_phat_oracle as G
import tdoa
from tdoa import synth

TOL_W = 2.0 ** -23  # one float ulp at 1: libm cos against numpy cos

BANDS = [
    # (lo, hi, taper) in Hz
    (1000.0, 6000.0, 0.0),       # hard edges
    (1000.0, 6000.0, 500.0),     # tapered
    (0.0, 6000.0, 0.0),          # lo = 0
    (0.0, 3000.0, 750.0),        # lo = 0: the lower taper lies below bin 0
    (5000.0, None, 0.0),         # hi = fs/2
    (5000.0, None, 1000.0),      # hi = fs/2: the upper taper lies past bin N
    ("bin", "bin", 0.0),         # both edges exactly on a bin
    ("bin", "bin", "bins"),      # ... and the taper ends exactly on bins
    (1234.5, 1300.25, 2000.0),   # a band narrower than its tapers
]


def _band(N, fs, lo, hi, taper):
    df = fs / (2.0 * N)
    lo = 37 * df if lo == "bin" else lo
    hi = (fs / 2.0 if hi is None else (N // 3) * df if hi == "bin" else hi)
    taper = 16 * df if taper == "bins" else taper
    return lo, hi, taper


@pytest.mark.parametrize("band", BANDS)
@pytest.mark.parametrize("fs", [48000, 50000])
@pytest.mark.parametrize("N", [256, 1024, 4096])
def test_band_weights_match_the_formula(N, fs, band):
    lo, hi, taper = _band(N, fs, *band)
    got = tdoa.band_weights(N, fs, lo, hi, taper)
    exp = band_ref.band_weights(N, fs, lo, hi, taper)
    assert got.dtype == np.float32 and got.shape == (N + 1,)
    assert np.abs(got.astype(np.float64) - exp).max() <= TOL_W
    exact = (exp == 0.0) | (exp == 1.0)
    assert (got[exact] == exp[exact]).all()
    f = np.arange(N + 1) * fs / (2.0 * N)
    assert (got[(f >= lo) & (f <= hi)] == 1.0).all()
    assert (got[(f < lo - taper) | (f > hi + taper)] == 0.0).all()
    assert got.min() >= 0.0 and got.max() <= 1.0


def test_band_weights_edge_on_a_bin_is_inside():
    # f_37 = 37 * 50000 / 2048 is exact in double: the bin belongs to the band
    N, fs = 1024, 50000
    f37, f300 = 37 * fs / 2048.0, 300 * fs / 2048.0
    w = tdoa.band_weights(N, fs, f37, f300)
    assert w[36] == 0 and w[37] == 1 and w[300] == 1 and w[301] == 0
    assert w.sum() == 300 - 37 + 1


@pytest.mark.parametrize("args", [
    (1024, 50000, -1.0, 6000.0, 0.0),            # lo < 0
    (1024, 50000, 6000.0, 6000.0, 0.0),          # lo == hi
    (1024, 50000, 7000.0, 6000.0, 0.0),          # lo > hi
    (1024, 50000, 1000.0, 25000.5, 0.0),         # hi > fs/2
    (1024, 50000, 1000.0, 6000.0, -1.0),         # taper < 0
    (1024, 50000, float("nan"), 6000.0, 0.0),
    (1024, 50000, 1000.0, float("nan"), 0.0),
    (1024, 50000, 1000.0, 6000.0, float("nan")),
    (1000, 50000, 1000.0, 6000.0, 0.0),          # N not a power of two
    (128, 50000, 1000.0, 6000.0, 0.0),           # N < 256
    (8192, 50000, 1000.0, 6000.0, 0.0),          # N > 4096
    (1024, 0, 0.0, 0.0, 0.0),                    # fs <= 0
    (1024, 50000, 1001.0, 1002.0, 0.0),          # no bin inside: all zero
])
def test_band_weights_rejects(args):
    L = tdoa.load()
    w = np.full(8193, 7.0, np.float32)
    assert L.tdoa_band_weights(*args, w.ctypes.data_as(C.c_void_p)) == -1
    assert (w == 7.0).all()  # nothing written
    assert L.tdoa_last_error()
    with pytest.raises(tdoa.TdoaError):
        tdoa.band_weights(*args)


def test_band_weights_rejects_null_table():
    assert tdoa.load().tdoa_band_weights(1024, 50000, 1000.0, 6000.0, 0.0, None) == -1


def test_setters_reject_null_context():
    L = tdoa.load()
    w = np.ones(1025, np.float32)
    assert L.tdoa_set_bin_weights(None, w.ctypes.data_as(C.c_void_p)) == -1
    assert L.tdoa_set_band_hz(None, 1000.0, 6000.0, 0.0) == -1
    assert L.tdoa_get_bin_weights(None, w.ctypes.data_as(C.c_void_p)) == -1


# ---- the scenario (issue: "the test that fails without this feature"), on the
# float64 reference alone.  8-bit ADC-style frames at 50 kHz: a 1.5-5.5 kHz
# target with integer mic delays under a 12-24 kHz interferer of the same
# amplitude with other delays.
FS, S = 50000, 46
TARGET_DELAYS = [0, 7, -12, 20, 3, -5, 9, -17]
INTERFERER_DELAYS = [0, -15, 9, -6, 11, 22, -8, 4]
# seed of synth.interferer_frames (numpy default_rng; draw order in its
# docstring): the first seed tried; both conditions below hold at it for the
# three shapes
SCENARIO_SEED = 0xBA2D


def scenario(M, N, B=16, device="cpu"):
    return synth.interferer_frames(B, M, N, FS, S, SCENARIO_SEED + 16 * M + N, TARGET_DELAYS,
                                   INTERFERER_DELAYS, device=device)


@pytest.mark.parametrize("M,N", [(3, 2048), (4, 2048), (4, 4096)])
def test_scenario_on_the_reference(M, N):
    fr, tgt, itf = scenario(M, N)
    assert fr.dtype.is_floating_point is False and tuple(fr.shape) == (16, M, N)
    assert int(fr.min()) >= 0 and int(fr.max()) <= 255
    assert np.abs(tgt).max() <= S and np.abs(itf).max() <= S and (tgt != itf).any()
    fr = fr.numpy()
    win = band_ref.window_q15(N)
    plain = band_ref.gcc_phat_band(fr, S, win, np.ones(N + 1))
    hit_t = (plain["lags"] == tgt).all(-1)
    hit_i = (plain["lags"] == itf).all(-1)
    print(f"({M}, {N}) unweighted: target tuple on {hit_t.mean():.0%}, interferer's on {hit_i.mean():.0%}")
    assert not hit_t.any()
    band = band_ref.gcc_phat_band(fr, S, win, band_ref.band_weights(N, FS, 1000, 6000))
    hit_b = (band["lags"] == tgt).all(-1)
    print(f"({M}, {N}) 1-6 kHz: target tuple on {hit_b.mean():.0%}")
    assert hit_b.all()


def test_all_ones_reference_is_the_oracle():
    fr, _, _ = scenario(3, 1024, B=6)
    full = synth.full_range_frames(2, 3, 1024, 5)
    fr = np.concatenate([fr.numpy(), full.numpy()])
    win = band_ref.window_q15(1024)
    rng = np.random.default_rng(3)
    lut = rng.integers(0, 2 * S + 1, (3, 101 * 101)).astype(np.uint8)
    a = band_ref.gcc_phat_band(fr, S, win, np.ones(1025), lut)
    b = G.gcc_phat_batch(fr, S, win, lut)
    assert set(a) == set(b)
    for k in b:
        assert np.abs(a[k].astype(np.float64) - b[k].astype(np.float64)).max() <= 1e-12, k
