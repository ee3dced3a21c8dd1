"""The inputs of tests/test_gpu_window.py (tests/window_cases.py) on the
references alone: under both caller windows every pair's float64 top-2 margin
exceeds 2e-4 (every lag is compared), at least 90 % of the cells have a map
margin above 1e-3, and the streaming reference drops no stream and skips no
cell.  No kernel runs here."""
import numpy as np
import pytest

import band_ref
import gcc_phat_oracle as G
import pcm16_ref
import stream_phat_ref as RP
import window_cases as WC
from test_mic_counts_cpu import assert_batch_caps


@pytest.mark.parametrize("kind", WC.WINDOWS)
@pytest.mark.parametrize("N", [512, 1024, 2048, 4096])
def test_tables_are_what_the_docstring_says(kind, N):
    w = WC.window(kind, N)
    assert w.dtype == np.int32 and w.shape == (N,) and w.min() >= 0 and w.max() == 32767
    assert not np.array_equal(w, band_ref.window_q15(N))
    if kind == "rect":
        assert (w == 32767).all()
        return
    assert (w[:N // 8] == 0).all() and (np.diff(w[N // 8:N // 2]) > 0).all()
    assert (w[N // 2:N - 16] == 32767).all() and list(w[N - 16:]) == [1, 0] * 8
    assert not np.array_equal(w, w[::-1])


@pytest.mark.parametrize("kind", WC.WINDOWS)
@pytest.mark.parametrize("M,N,fs,mics,kernel", WC.PHAT)
def test_batch_references_compare_every_lag(oracle, kind, M, N, fs, mics, kernel):
    lut, win = WC.lut_cpu(oracle, M, fs, mics), WC.window(kind, N)
    fr = WC.adc_batch(lut, M, N, fs)
    exp = G.gcc_phat_batch(fr, WC.max_shift(fs), win, lut)
    assert_batch_caps(exp, (kind, M, N, fs))
    # the table matters: the default window gives other scores
    dflt = G.gcc_phat_batch(fr, WC.max_shift(fs), band_ref.window_q15(N), lut)
    assert np.abs(dflt["scores_f"] - exp["scores_f"]).max() > 1e-2


@pytest.mark.parametrize("kind", WC.WINDOWS)
@pytest.mark.parametrize("M,N,fs,mics,kernel", WC.PCM16)
def test_pcm16_references_compare_every_lag(oracle, kind, M, N, fs, mics, kernel):
    lut = WC.lut_cpu(oracle, M, fs, mics)
    exp = pcm16_ref.gcc_phat_pcm16(WC.pcm16_batch(lut, M, N, fs), WC.max_shift(fs), WC.window(kind, N), lut)
    assert_batch_caps(exp, (kind, "pcm16", M, N))


@pytest.mark.parametrize("kind", WC.WINDOWS)
def test_stream_reference_drops_and_skips_nothing(oracle, kind):
    c = WC.STREAM
    lut = WC.lut_cpu(oracle, c["M"], c["fs"], None)
    adc = WC.stream_capture(lut)
    win = WC.window(kind, c["N"])
    ref = RP.run(oracle, adc, c["N"], c["fs"], c["S"], win, lut)
    records, gated, dropped, skipped, gap = RP.stats(ref)
    print(f"{kind}: {records} records, {gated} gated, {dropped} dropped, {skipped} skipped, min map gap {gap:.3e}")
    assert dropped == 0 and skipped == 0 and gated >= 20
    exp = oracle.stream_run(adc, c["N"], c["fs"], c["S"], win, lut)
    assert exp["n_trig"].sum() == records and exp["gate"].sum() >= 20
    dflt = oracle.stream_run(adc, c["N"], c["fs"], c["S"], band_ref.window_q15(c["N"]), lut)
    assert not np.array_equal(dflt["est"], exp["est"])  # the table matters
