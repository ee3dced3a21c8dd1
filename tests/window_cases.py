"""Caller-supplied windows (tdoa_config.window_q15) and the batches that carry
them (TEST INFRASTRUCTURE ONLY): one definition for tests/test_gpu_window.py,
which runs them on the GPU, and tests/test_window_cpu.py, which checks on the
references alone that every lag and at least 90 % of the cells are compared.

Two tables per frame length:
  "asym"  zeros over the first N / 8 samples, a linear ramp to 32767 at N / 2, a
          plateau of 32767, then 1, 0, 1, ... over the last 16: nothing about it
          is symmetric, so a reversed, shifted or per-mic-misplaced table shows;
  "rect"  all 32767.
Neither is the default DPSS table or close to it.
"""
import numpy as np

from tdoa import synth

WINDOWS = ("asym", "rect")
TWO = np.array([[-0.066, 0.0], [0.066, 0.0]], np.float32)
# the reference triangle doubled: with S = 63 more lag tuples than k_p1k_lean holds
DOUBLED = np.array([[-0.132, -0.076], [0.132, -0.076], [0.0, 0.152]], np.float32)
MICS = {2: TWO, 3: None, 4: synth.square_mics(0.15), 5: synth.circle_mics(5, 0.15), 8: synth.circle_mics(8, 0.15)}


def window(kind, N):
    """int32 [N], every value in [0, 32767]."""
    if kind == "rect":
        return np.full(N, 32767, np.int32)
    assert kind == "asym"
    w = np.full(N, 32767, np.int32)
    w[:N // 8] = 0
    ramp = np.arange(N // 8, N // 2)
    w[ramp] = (32767 * (ramp - N // 8)) // (N // 2 - N // 8)
    w[N - 16:] = np.arange(16) % 2 == 0
    return w


def batch_size(N):
    return 12 if N == 4096 else 24


# (M, N, fs, mics, first kernel of the batch); the lag range is the rate's own
DIRECT = [(3, 1024, 50000, None, "k_direct_mfma"),
          (8, 2048, 50000, None, "k_direct_mfma"),
          (2, 4096, 50000, None, "k_direct")]       # frames beyond the MFMA kernel's staging registers
PHAT = [(3, 1024, 50000, None, "k_p1k_lean"),
        (3, 1024, 67600, DOUBLED, "k_gcc_phat_1024"),
        (3, 512, 50000, None, "k_gcc_phat"),
        (5, 512, 50000, None, "k_phat_spectra"),
        (4, 2048, 50000, None, "k_frame16"),
        (5, 2048, 50000, None, "k_spec16")]
PCM16 = [(3, 1024, 50000, None, "k_p1k_pcm16"), (4, 2048, 50000, None, "k_f16_pcm16")]


def mic_xy(M, mics):
    return MICS[M] if mics is None else mics


def max_shift(fs):
    return fs * 32 // 34300  # the library's default lag range, at most 63


def lut_cpu(oracle, M, fs, mics):
    xy = mic_xy(M, mics)
    return oracle.build_lut(oracle.microphones_ref() if xy is None else xy, fs=fs, max_shift=max_shift(fs))


def seed(M, N, fs):
    return 0x3100 + 100 * M + N + fs // 100


def adc_batch(lut, M, N, fs):
    """int16 [B][M][N] of synth.adc_frames on the CPU generator.  Reference-alone
    figures under both tables over PHAT's shapes: the minimum float64 top-2
    margin is 0.58 (5 x 512, "asym") or more, and every cell's map margin exceeds
    1e-3 but for one frame of 24 at 4 x 2048 under "rect"."""
    return synth.adc_frames(batch_size(N), M, N, lut, max_shift(fs), seed(M, N, fs))[0].numpy()


def pcm16_batch(lut, M, N, fs):
    """The same frames over the 16-bit range: (x - 128) * 256."""
    return ((adc_batch(lut, M, N, fs).astype(np.int32) - 128) * 256).astype(np.int16)


# Streams: eight streams x 24 hops of 3 x 1024 / hop 512 at 48 kHz (S = 44).
# The float64 reference alone (tests/stream_phat_ref.py) at this seed, under
# "asym" / "rect": 42 records, all gated, no stream dropped, no cell skipped,
# minimum map gap 4.2e-2 under either table.
STREAM = dict(streams=8, hops=24, N=1024, hop=512, M=3, fs=48000, S=44, seed=0x3157)


def stream_capture(lut):
    c = STREAM
    return synth.adc_stream(c["streams"], c["hop"] * c["hops"], c["M"], lut, c["S"], c["seed"]).numpy()
