"""The captures of the long-frame streaming tests (TEST INFRASTRUCTURE ONLY):
one definition for tests/test_gpu_stream_long.py, which runs them on the GPU
(k_f16_ring -> k_stream_ema_grid at 8 mics x 2048 and 4 mics x 4096), and
tests/test_stream_long_cpu.py, which checks on the float64 references alone
that at every seed used here no stream is dropped and no cell is skipped, so
the GPU comparisons run with max_dropped = 0 and max_skip = 0.

All contexts: 48 kHz, max_shift 44, six streams, stream16_cases' MICS / DC.
"""
import stream16_cases
import stream_cont_cases
from stream16_cases import FS, MICS, S_LAG, lut_cpu  # noqa: F401
from tdoa import synth

STREAMS = 6
FMTS = ("adc8", "pcm16")

# triggered: (N, hop, M, hops, seed)
TRIGGERED = [(2048, 1024, 8, 16, 910),
             (4096, 2048, 4, 12, 420)]
# the band of the triggered uint8 cases: (lo Hz, hi Hz, taper Hz)
BAND = (1000, 6000, 500)
# continuous: (N, hop, M, hops, seed, activity_var)
CONTINUOUS = {"adc8": [(2048, 1024, 8, 24, 910, 1600),
                       (4096, 2048, 4, 16, 400, 800)],
              "pcm16": [(2048, 1024, 8, 24, 910, 8000000),
                        (4096, 2048, 4, 16, 402, 4000000)]}

# what every reference must show before the GPU is compared against it
MIN_GAP = 2e-3
MIN_GATED = 25


def triggered_capture(fmt, lut, N, hop, M, hops, seed):
    """uint8 ("adc8": synth.adc_stream) or int16 ("pcm16": stream16_cases.shape_capture) [6][hop * hops][M]."""
    if fmt == "pcm16":
        return stream16_cases.shape_capture(lut, N, hop, M, hops, seed)
    return synth.adc_stream(STREAMS, hop * hops, M, lut, S_LAG, seed).numpy()


def continuous_capture(fmt, lut, N, hop, M, hops, seed):
    return stream_cont_cases.capture(fmt, lut, N, hop, M, hops, seed)
