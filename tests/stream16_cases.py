"""The captures of the int16 streaming tests (TEST INFRASTRUCTURE ONLY): one
definition for tests/test_gpu_stream16.py, which runs them on the GPU, and
tests/test_stream16_cpu.py, which checks on the float64 reference alone that
every seed used here drops no stream and stays within its cell-skip cap.

All contexts: 48 kHz, max_shift 44 (48000 * 32 // 34300), the default grid.
"""
import numpy as np

from tdoa import synth

FS, S_LAG = 48000, 44
MICS = {2: np.array([[-0.066, 0], [0.066, 0]], np.float32), 3: None, 4: synth.square_mics(0.15),
        8: synth.circle_mics()}
# per-mic DC offsets in counts, up to +-12000 (a 16-bit front end's; 8 bits cannot hold them)
DC = (12000.0, -9000.0, 4000.0, -12000.0, 700.0, -3100.0, 8000.0, -50.0)


def lut_cpu(oracle, M):
    """The context's LUT [P][H][W] built by the oracle (no GPU)."""
    mics = oracle.microphones_ref() if MICS[M] is None else MICS[M]
    return oracle.build_lut(mics, fs=FS, max_shift=S_LAG)


def scaled8(lut):
    """Case 1: the 8-bit config-5 test capture and (u8 - 128) * 256 of it."""
    adc = synth.adc_stream(40, 512 * 40, 3, lut, S_LAG, 0x5EED0005).numpy()
    return adc, scale8(adc)


def scale8(adc):
    return ((adc.astype(np.int16) - 128) * 256).astype(np.int16)


# Case 2: a quiet source (30 counts rms, 0.12 LSB of an 8-bit converter with
# the same full scale) over 4 counts of noise on large offsets, with a trigger
# threshold to match (the bursts' variance over three mics is about 2700)
TRUE16_SEED, TRUE16_VAR = 0x16B0001, 800


def true16(lut):
    return synth.pcm16_stream(40, 512 * 40, 3, lut, S_LAG, TRUE16_SEED, src_std=30.0, noise_std=4.0,
                              dc=DC).numpy()


def truncated8(cap):
    """What an 8-bit converter of the same full scale keeps: (x >> 8) << 8."""
    return ((cap >> 8) << 8).astype(np.int16)


# Case 4: (N, hop, M, hops, seed, share of gated records whose cell may be
# skipped) -- the shapes and caps of test_gpu_stream_phat.SHAPES
SHAPES = [(2048, 1024, 4, 24, 2122, 0.25),
          (512, 256, 2, 24, 584, 0.0),
          (1024, 384, 3, 24, 424, 0.0),
          (256, 256, 3, 40, 77, 0.0),
          (1024, 512, 8, 24, 808, 0.25)]


def shape_capture(lut, N, hop, M, hops, seed):
    return synth.pcm16_stream(6, hop * hops, M, lut, S_LAG, seed, dc=DC).numpy()


# Cases 5, 6, 8, 9: six or eight streams of the default scenario
WRAP_SEED, VAR_SEED, BAND_SEED, API_SEED = 23, 61, 102, 7
# Case 6: thresholds.  The bursts' variance is about 3000^2 = 9e6 counts^2 per
# mic, 2.7e7 over three mics: at 2.8e7 only a burst whose sample variance over
# the older half runs above nominal fires, under half of them
TRIGGER_VARS = (0, 131072, 28000000)


def small_capture(lut, seed, streams=6, hops=24, hop=512, M=3):
    return synth.pcm16_stream(streams, hop * hops, M, lut, S_LAG, seed, dc=DC).numpy()


# Case 7
FULL_SCALE = dict(ns=6, T=1024 * 16, N=2048, M=4, seed=0xF5)
