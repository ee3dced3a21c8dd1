"""The streaming GCC_PHAT reference (tests/stream_phat_ref.py) pinned on the
CPU, on the config-5 capture the GPU tests use (test_gpu_stream_phat.py)."""
import numpy as np
import pytest

import band_ref
import stream_phat_ref as R
from conftest import golden
from tdoa import synth

FS, N, S = 48000, 1024, 44


@pytest.fixture(scope="module")
def case(oracle):
    mics = oracle.microphones_ref()
    lut = oracle.build_lut(mics, fs=FS, max_shift=S)
    win = golden("window_q15.npz")["n1024"]
    adc = synth.adc_stream(40, 512 * 40, 3, lut, S, 0x5EED0005).numpy()
    direct = oracle.stream_run(adc, N, FS, S, win, lut.reshape(3, -1), max_trig=64)
    return adc, win, lut, direct, R.run(oracle, adc, N, FS, S, win, lut)


def test_reference_lags_equal_the_direct_oracle(case):
    _, _, _, direct, ref = case
    n = 0
    for s in range(40):
        k = direct["n_trig"][s]
        assert ref["n_trig"][s] == k
        assert (ref["end"][s, :k] == direct["end"][s, :k]).all()
        assert (ref["lags"][s, :k] == direct["lags"][s, :k]).all()
        assert (ref["gate"][s, :k] == direct["gate"][s, :k]).all()
        n += k
    assert n > 200


def test_every_raw_margin_is_clear(case):
    _, _, _, _, ref = case
    worst = min(ref["raw_margin"][s, :ref["n_trig"][s]].min() for s in range(40))
    records, gated, dropped, skipped, gap = R.stats(ref)
    print(f"{records} frames, {gated} gated, min raw margin {worst:.3e}, {dropped} streams dropped, "
          f"{skipped} cells skipped, min map gap {gap:.3e}")
    assert worst > R.TOL_LAG_MARGIN
    assert dropped == 0 and skipped == 0


def test_one_gated_frame_from_zero_state(oracle, case):
    """est = 0 + (w - 0) * decay(now, 0): the first gated frame of a stream
    alone, run as a capture that ends with it."""
    adc, win, lut, _, ref = case
    s = 3
    i = int(np.argmax(ref["gate"][s, :ref["n_trig"][s]]))
    assert ref["gate"][s, i]
    end = int(ref["end"][s, i])
    one = R.run(oracle, adc[s:s + 1, :end], N, FS, S, win, lut)
    assert one["n_trig"][0] == i + 1 and one["end"][0, i] == end
    frame = adc[s, end - N:end, :].T.astype(np.int16)[None]
    w = band_ref.gcc_phat_band(frame, S, win, np.ones(N + 1))["weighted_f"][0]
    dec = oracle.decay(end * 1000000 // FS, 0)
    assert 0.0 < dec < 1.0
    assert np.array_equal(one["est"][0], w * dec)
    assert one["last"][0] == end * 1000000 // FS
