"""The captures of the continuous-mode streaming tests (TEST INFRASTRUCTURE
ONLY): one definition for tests/test_gpu_stream_cont.py, which runs them on the
GPU, and tests/test_stream_cont_cpu.py, which checks on the float64 reference
alone that every case drops no stream and stays within its cell-skip cap.

All contexts: 48 kHz, max_shift 44, stream16_cases' MICS / DC / lut_cpu, six
streams of 3000-sample bursts whose starts lie 6000 to 9000 samples apart
(silences of 3000 to 6000 samples).
"""
import numpy as np

from stream16_cases import DC, FS, MICS, S_LAG, lut_cpu  # noqa: F401
from tdoa import synth

STREAMS = 6
BURST = dict(burst_len=3000, gap=(6000, 9000))

# (N, hop, M, hops, seed, activity_var): activity_var in counts^2 summed over
# the mics, about a third of a burst's variance there (3000^2 per mic on int16
# rings, 40^2 on uint8 rings), far above the floor's (30^2 and 0.5^2)
PCM16_CASES = [(1024, 512, 3, 48, 31, 3000000),
               (1024, 256, 3, 96, 32, 3000000),
               (2048, 1024, 4, 36, 2122, 4000000),
               (512, 128, 2, 96, 584, 2000000),
               (1024, 512, 8, 36, 808, 8000000)]
ADC8_CASES = [(1024, 512, 3, 48, 31, 600),
              (1024, 384, 3, 64, 424, 600),   # hop != N / 2: the first frame ends at 1152
              (2048, 1024, 4, 36, 2122, 800),
              (512, 128, 2, 96, 584, 400),
              (1024, 512, 8, 36, 808, 1600)]
CASES = {"pcm16": PCM16_CASES, "adc8": ADC8_CASES}


def max_skip(M):
    """The suite's caps on gated records whose cell may be skipped: none for 2
    and 3 mics, 25 % for 4 and 8 (the 4-mic square's maps have near-ties)."""
    return 0.0 if M <= 3 else 0.25


def capture(fmt, lut, N, hop, M, hops, seed):
    """The case's capture [6][hop * hops][M]: int16 ("pcm16") or uint8 ("adc8")."""
    if fmt == "pcm16":
        return synth.pcm16_stream(STREAMS, hop * hops, M, lut, S_LAG, seed, dc=DC, **BURST).numpy()
    return synth.adc_stream(STREAMS, hop * hops, M, lut, S_LAG, seed, **BURST).numpy()


# the small shape of the ring tests: N 256 (4 samples per lane), hop 256, 3 mics
SMALL = dict(N=256, hop=256, M=3, hops=40)
SMALL_SEED = {"pcm16": 77, "adc8": 78}
SMALL_VAR = {"pcm16": 3000000, "adc8": 600}

# full scale on int16 rings: (N, M, hop, streams, samples, seed), activity_var 2^30
FULL_SCALE = [(4096, 2, 2048, 6, 4096 * 8, 0xF6), (2048, 4, 1024, 6, 2048 * 8, 0xF5)]


def alternating(T, M, amp=100):
    """+amp, -amp, ... on every mic: sum x = 0 and sum x^2 = N amp^2 over any
    even-length frame, so sum_m pw(m) = M amp^2 N^2 exactly."""
    x = np.where(np.arange(T) % 2 == 0, amp, -amp).astype(np.int16)
    return np.repeat(x[:, None], M, axis=1)
