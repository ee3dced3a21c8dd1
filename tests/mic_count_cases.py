"""The shapes, seeds and inputs of the 6- and 7-microphone tests (TEST
INFRASTRUCTURE ONLY): one definition for tests/test_gpu_mic_counts.py, which
runs them on the GPU, and tests/test_mic_counts_cpu.py, which checks on the
references alone that no tolerance-gated comparison passes empty.

Geometry: synth.circle_mics(M, 0.15) for every M here (5..8), the default
grid.  Batches: 50 kHz, max_shift 46.  Streams: 48 kHz, max_shift 44.  Every
input is generated on the CPU (the GPU tests upload it), so both sides see the
same bytes.
"""
import numpy as np

from stream16_cases import DC  # per-mic offsets in counts, up to +-12000
from tdoa import synth

FS_BATCH, S_BATCH = 50000, 46
FS_STREAM, S_STREAM = 48000, 44
RADIUS = 0.15


def mics(M):
    return synth.circle_mics(M, RADIUS)


def lut_cpu(oracle, M, fs=FS_BATCH, S=S_BATCH):
    """The context's LUT [P][H][W] built by the oracle (no GPU)."""
    return oracle.build_lut(mics(M), fs=fs, max_shift=S)


# ---------------------------------------------------------------- batches
def batch_size(N):
    return 24 if N <= 1024 else (16 if N == 2048 else 12)


def batch_seed(M, N):
    return 10000 * M + N


# GCC_PHAT (M, N): the smallest shapes that take each route.  Reference-alone
# figures (float64 oracle on adc_frames(batch_size(N), seed batch_seed(M, N))):
# the minimum top-2 margin over every pair of every frame is 0.42 (6 x 256) to
# 0.84 (7 x 4096), and every cell's map margin exceeds 1e-3 but for one frame of
# 16 at (7, 2048).  pcm16_batch: margins 0.54 to 0.88, every cell sure.  Under
# the band table: 0.012 at (6, 256) with 23 of 24 cells sure, 0.063 at (7, 2048).
PHAT_SHAPES = [(6, 256), (7, 256), (7, 1024), (6, 2048), (7, 2048), (7, 4096), (8, 4096)]
# the band table (lo, hi, taper in Hz) of one 6-mic and one 7-mic shape
BAND = (2000, 9000, 1500)
BAND_SHAPES = [(6, 256), (7, 2048)]
MIN_SURE_CELLS = 0.9


def phat_route(N, fmt="adc8", band=False):
    """The first kernel of the batch: neither mic count is a k_frame16 shape."""
    if fmt == "pcm16":
        return "k_phat_spectra_pcm16"
    return "k_phat_spectra" if band or N <= 1024 else "k_spec16"


def adc_batch(lut, M, N, B=None, seed=None):
    """int16 [B][M][N] of synth.adc_frames on the CPU generator."""
    B = batch_size(N) if B is None else B
    seed = batch_seed(M, N) if seed is None else seed
    return synth.adc_frames(B, M, N, lut, S_BATCH, seed)[0].numpy()


def pcm16_batch(lut, M, N, B=None, seed=None, S=S_BATCH):
    """Full-range 16-bit frames in the manner of synth.adc_frames: per frame a
    white source of 3000 counts rms at a random cell, mic m delayed by the
    cell's integer LUT lag of pair (0, m), 600 counts of noise and the offsets
    DC; int16 [B][M][N]."""
    B = batch_size(N) if B is None else B
    rng = np.random.default_rng(0x16000000 + (batch_seed(M, N) if seed is None else seed))
    lut2 = np.asarray(lut).reshape(lut.shape[0], -1).astype(np.int64)
    cells = rng.integers(0, lut2.shape[1], B)
    tau = np.zeros((B, M), np.int64)
    for m in range(1, M):
        tau[:, m] = lut2[m - 1][cells] - S
    pad = S + 1
    src = rng.standard_normal((B, N + 2 * pad)) * 3000.0
    idx = np.arange(N)[None, None, :] + pad - tau[:, :, None]
    x = np.take_along_axis(np.broadcast_to(src[:, None, :], (B, M, src.shape[1])), idx, 2)
    x = x + rng.standard_normal((B, M, N)) * 600.0 + np.asarray(DC[:M], np.float64)[None, :, None]
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


# DIRECT (M, N, max_shift, batch): 0 is the rate's own 46; 63 is the widest lag
# range, 45 an odd one (the lag tiles then start at -S - 1).  Each batch gets
# eight full-range frames appended (the int16 wrap paths).
DIRECT_SHAPES = [(6, 256, 0, 24), (7, 256, 45, 24), (6, 2048, 63, 16), (7, 4096, 0, 12)]


def direct_batch(lut, M, N, S, B):
    adc = synth.adc_frames(B, M, N, lut, S, 77 + batch_seed(M, N))[0]
    full = synth.full_range_frames(8, M, N, 99 + batch_seed(M, N))
    return np.ascontiguousarray(np.concatenate([adc.numpy(), full.numpy()]))


# ---------------------------------------------------------------- streams
STREAMS, HOPS = 6, 24

# Triggered: (N, hop, M, seed) of synth.adc_stream(6, hop * 24, ...).  The
# float64 reference alone (tests/stream_phat_ref.py):
#   6 x 1024 / 512, seed 602: 0 streams dropped, 0 cells skipped, min map gap >= 4e-2
#   7 x  512 / 256, seed 702: 29 gated records, 0 dropped, 0 skipped, min map gap 3.8e-2
# (Seeds 601, 604, 701, 703 and 705 skip 2 to 6 records, 700 and 704 drop a stream.)
TRIGGERED = [(1024, 512, 6, 602), (512, 256, 7, 702)]
# the DIRECT route of each: k_direct_mfma runs the EMA itself when
# F * P * K <= 3 * threads at 8 waves (1536): 15 * 89 = 1335 fits, 21 * 89 = 1869 does not
DIRECT_STREAM_KERNEL = {6: "k_direct_mfma", 7: "k_direct"}


def triggered_capture(lut, N, hop, M, seed):
    return synth.adc_stream(STREAMS, hop * HOPS, M, lut, S_STREAM, seed).numpy()


# Continuous: (fmt, N, hop, M, hops, seed, activity_var, capture_len): bursts of
# 3000 samples 6000 to 9000 apart as in tests/stream_cont_cases.py, thresholds a
# third of a burst's variance summed over the mics.  capture_len is odd: 2049 * 5
# and 2049 * 7 bytes put every uint8 ring but the first on an odd address, 1283 *
# 7 likewise; 2049 * 6 int16 samples put every other ring 4 bytes off a 16-byte
# boundary.  Every ring is shorter than the capture, so frames wrap.
# The float64 reference alone (tests/stream_cont_ref.py), cap max_skip(M) = 25 %:
#   pcm16 6 x 1024 / 512 seed 62:  61 records, all gated, 0 dropped, 0 skipped, min map gap 1.0e-1
#   adc8  5 x 1024 / 512 seed 56:  60 records, all gated, 0 dropped, 0 skipped, min map gap 1.6e-1
#   adc8  7 x  512 / 256 seed 72: 136 records, all gated, 0 dropped, 0 skipped, min map gap 8.9e-2
# (of the seeds 61..66, 51..56 and 71..76 about half skip 1 to 24 cells; none drops a stream)
CONTINUOUS = [("pcm16", 1024, 512, 6, 24, 62, 6000000, 2049),
              ("adc8", 1024, 512, 5, 24, 56, 1000, 2049),
              ("adc8", 512, 256, 7, 48, 72, 1400, 1283)]
BURST = dict(burst_len=3000, gap=(6000, 9000))


def continuous_capture(fmt, lut, N, hop, M, hops, seed):
    if fmt == "pcm16":
        return synth.pcm16_stream(STREAMS, hop * hops, M, lut, S_STREAM, seed, dc=DC, **BURST).numpy()
    return synth.adc_stream(STREAMS, hop * hops, M, lut, S_STREAM, seed, **BURST).numpy()
