"""The inputs of tests/test_gpu_mic_counts.py (tests/mic_count_cases.py) on the
references alone: every condition that keeps a tolerance-gated GPU comparison
from passing empty.  No kernel runs here.

  batches   every pair's float64 top-2 margin exceeds 2e-4 (every lag is
            compared) and at least 90 % of the cells have a map margin above
            1e-3 (the cell is compared) -- 8-bit, 16-bit and band-limited;
  triggered 0 streams dropped, 0 cells skipped;
  continuous 0 streams dropped, cells skipped within stream_cont_cases.max_skip(M).
"""
import numpy as np
import pytest

import band_ref
import gcc_phat_oracle as G
import mic_count_cases as MC
import pcm16_ref
import stream_cont_cases as Cs
import stream_cont_ref as RC
import stream_phat_ref as RP
import tdoa

TOL_LAG_MARGIN, TOL_CELL_MARGIN = 2e-4, 1e-3  # tests/test_gpu_gcc_phat.py


def batch_caps(exp):
    """(minimum top-2 margin over every pair of every frame, share of frames
    whose float64 map maximum beats every other value by more than 1e-3)."""
    srt = np.sort(exp["scores_f"], axis=-1)
    Lg = exp["L"]
    top = Lg.max(-1)
    second = np.where(Lg >= top[:, None] - 1e-12, -np.inf, Lg).max(-1)
    return float((srt[..., -1] - srt[..., -2]).min()), float((top - second > TOL_CELL_MARGIN).mean())


def assert_batch_caps(exp, where):
    margin, sure = batch_caps(exp)
    print(f"{where}: min top-2 margin {margin:.3f}, cells sure {sure:.1%}")
    assert margin > TOL_LAG_MARGIN, where
    assert sure >= MC.MIN_SURE_CELLS, where


@pytest.mark.parametrize("M,N", MC.PHAT_SHAPES)
def test_batch_references_compare_every_lag(oracle, M, N):
    lut, win = MC.lut_cpu(oracle, M), band_ref.window_q15(N)
    fr = MC.adc_batch(lut, M, N)
    assert fr.shape == (MC.batch_size(N), M, N) and len(np.unique(fr.reshape(len(fr), -1), axis=0)) == len(fr)
    assert_batch_caps(G.gcc_phat_batch(fr, MC.S_BATCH, win, lut), ("adc8", M, N))
    fr16 = MC.pcm16_batch(lut, M, N)
    assert fr16.dtype == np.int16 and np.abs(fr16.astype(np.int32)).max() > 12000  # not 8-bit frames
    assert_batch_caps(pcm16_ref.gcc_phat_pcm16(fr16, MC.S_BATCH, win, lut), ("pcm16", M, N))


@pytest.mark.parametrize("M,N", MC.BAND_SHAPES)
def test_band_references_compare_every_lag(oracle, M, N):
    lut, win = MC.lut_cpu(oracle, M), band_ref.window_q15(N)
    w = tdoa.band_weights(N, MC.FS_BATCH, *MC.BAND)
    assert w.max() <= 1.0 and 0 < (w > 0).mean() < 0.5
    exp = band_ref.gcc_phat_band(MC.adc_batch(lut, M, N), MC.S_BATCH, win, w.astype(np.float64), lut)
    assert_batch_caps(exp, ("band", M, N))


def test_shapes_cover_both_mic_counts_and_every_route():
    for shapes in (MC.PHAT_SHAPES, [s[:2] for s in MC.DIRECT_SHAPES], MC.BAND_SHAPES):
        assert {6, 7} <= {M for M, _ in shapes}
    assert {MC.phat_route(N) for _, N in MC.PHAT_SHAPES} == {"k_phat_spectra", "k_spec16"}
    assert (8, 4096) in MC.PHAT_SHAPES
    assert {s for _, _, s, _ in MC.DIRECT_SHAPES} >= {0, 45, 63}
    # the tuple words of the generic grid solve: P = 15 leaves 3 pairs in the last word, P = 21 one
    assert [(M * (M - 1) // 2 + 3) // 4 for M in (6, 7)] == [4, 6]
    assert [M * (M - 1) // 2 % 4 for M in (6, 7)] == [3, 1]
    # the fused-EMA boundary of the DIRECT stream: 3 elements per thread at 8 waves
    K = 2 * MC.S_STREAM + 1
    assert 2 * 512 < 15 * K <= 3 * 512 < 21 * K


@pytest.mark.parametrize("N,hop,M,seed", MC.TRIGGERED)
def test_triggered_references_drop_and_skip_nothing(oracle, N, hop, M, seed):
    lut = MC.lut_cpu(oracle, M, MC.FS_STREAM, MC.S_STREAM)
    adc = MC.triggered_capture(lut, N, hop, M, seed)
    assert adc.shape == (MC.STREAMS, hop * MC.HOPS, M) and adc.dtype == np.uint8
    ref = RP.run(oracle, adc, N, MC.FS_STREAM, MC.S_STREAM, band_ref.window_q15(N), lut)
    records, gated, dropped, skipped, gap = RP.stats(ref)
    print(f"{M} x {N} / {hop} seed {seed}: {records} records, {gated} gated, {dropped} dropped, {skipped} skipped, "
          f"min map gap {gap:.3e}")
    assert dropped == 0 and skipped == 0 and gated >= 20
    # the DIRECT run of the same capture has the same triggers, gated too
    exp = oracle.stream_run(adc, N, MC.FS_STREAM, MC.S_STREAM, band_ref.window_q15(N), lut)
    assert exp["n_trig"].sum() == records and exp["gate"].sum() >= 20


@pytest.mark.parametrize("fmt,N,hop,M,hops,seed,var,capture_len", MC.CONTINUOUS)
def test_continuous_references_stay_within_their_caps(oracle, fmt, N, hop, M, hops, seed, var, capture_len):
    lut = MC.lut_cpu(oracle, M, MC.FS_STREAM, MC.S_STREAM)
    cap = MC.continuous_capture(fmt, lut, N, hop, M, hops, seed)
    assert cap.shape == (MC.STREAMS, hop * hops, M) and cap.dtype == (np.int16 if fmt == "pcm16" else np.uint8)
    assert N + 2 * hop <= capture_len < hop * hops and capture_len % 2 == 1
    ref = RC.run(oracle, cap, N, MC.FS_STREAM, MC.S_STREAM, band_ref.window_q15(N), lut, hop, var)
    records, gated, dropped, skipped, gap = RC.stats(ref)
    eligible = MC.STREAMS * sum((h + 1) * hop >= N for h in range(hops))
    print(f"{fmt} {M} x {N} / {hop} seed {seed}: {records} of {eligible} eligible frames listed, {gated} gated, "
          f"{dropped} dropped, {skipped} skipped, min map gap {gap:.3e}")
    assert dropped == 0 and skipped <= Cs.max_skip(M) * max(gated, 1)
    assert 50 <= records < eligible  # the gate holds the silences back
