"""Caller-supplied windows (tdoa_config.window_q15) through every front end.

The table is uploaded to each front end in a form of its own: floats / 128 in
the k_p1k_lean image, LDS window words in k_frame16, uint4 chunks in DIRECT,
the PCM16 variants' copies.  Two tables per frame length, neither the default
(tests/window_cases.py): an asymmetric one -- leading zeros, a ramp, a plateau
and 1, 0, 1, ... at the end, so a reversed or misplaced table shows -- and the
rectangular one.  The references take the same table.

Tolerances are the project's own: DIRECT bit for bit (tests/test_gpu_parity.py),
GCC_PHAT by test_gpu_gcc_phat.check_phat, the streams by test_gpu_stream.compare
and test_gpu_stream_phat.compare.  tests/test_window_cpu.py checks on the
references alone that every lag and at least 90 % of the cells are compared and
that the streaming reference drops and skips nothing.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gcc_phat_oracle as G  # noqa: E402
import pcm16_ref  # noqa: E402
import stream_phat_ref  # noqa: E402
import test_gpu_gcc_phat as T  # noqa: E402  (check_phat, _grid_f32)
import test_gpu_stream as TS  # noqa: E402  (run_pipeline, compare)
import test_gpu_stream_phat as TSF  # noqa: E402  (run_pipeline, compare, assert_bitwise)
import test_mic_counts_cpu as CPU  # noqa: E402  (assert_batch_caps)
import window_cases as WC  # noqa: E402
from test_gpu_parity import _cmp  # noqa: E402
from tdoa import synth  # noqa: E402
from tdoa.localizer import Localizer  # noqa: E402
from tdoa.stream import StreamPipeline  # noqa: E402


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _loc(engine, kind, M, N, fs, mics, **kw):
    win = WC.window(kind, N)
    loc = Localizer(engine=engine, num_mics=M, frame_len=N, sample_rate_hz=fs, mic_xy=WC.mic_xy(M, mics),
                    window_q15=win, **kw)
    assert loc.dims.S == WC.max_shift(fs)
    assert loc.window().dtype == win.dtype and (loc.window() == win).all()
    return loc, win


@pytest.mark.parametrize("kind", WC.WINDOWS)
@pytest.mark.parametrize("M,N,fs,mics,kernel", WC.DIRECT)
def test_direct_batch_bit_for_bit(oracle, kind, M, N, fs, mics, kernel):
    loc, win = _loc("direct", kind, M, N, fs, mics)
    assert loc.batch_kernel() == kernel
    S = loc.dims.S
    lut = WC.lut_cpu(oracle, M, fs, mics)
    assert (loc.lut() == lut.reshape(loc.lut().shape)).all()
    fr_np = np.concatenate([WC.adc_batch(lut, M, N, fs),
                            synth.full_range_frames(4, M, N, WC.seed(M, N, fs)).numpy()])
    got = _np(loc.localize(torch.from_numpy(fr_np).cuda(), scores=True))
    exp = oracle.localize_batch(fr_np, S, win, lut, threads=8)
    _cmp(got, exp)
    loc.close()


def _check_phat_run(loc, fr_np, exp, where):
    fr = torch.from_numpy(fr_np).cuda()
    got = _np(loc.localize(fr, scores=True))
    CPU.assert_batch_caps(exp, where)  # every lag and >= 90 % of the cells are compared below
    print(f"{where} {loc.batch_kernel()}: max |score err| {np.abs(got['scores_f'] - exp['scores_f']).max():.2e}")
    assert T.check_phat(got, exp) == 1.0
    assert (got["lags"] == exp["lags"]).all()
    lean = _np(loc.localize(fr))
    for k in lean:
        assert np.array_equal(lean[k].view(np.uint8), got[k].view(np.uint8)), k
    cell, mx = T._grid_f32(got["weighted_f"], loc.lut())
    assert (got["cell"] == cell).all() and (got["max_Lf"] == mx).all()


@pytest.mark.parametrize("kind", WC.WINDOWS)
@pytest.mark.parametrize("M,N,fs,mics,kernel", WC.PHAT)
def test_phat_batch_against_float64(oracle, kind, M, N, fs, mics, kernel):
    loc, win = _loc("gcc_phat", kind, M, N, fs, mics)
    assert loc.batch_kernel() == kernel
    lut = WC.lut_cpu(oracle, M, fs, mics)
    assert (loc.lut() == lut.reshape(loc.lut().shape)).all()
    fr_np = WC.adc_batch(lut, M, N, fs)
    _check_phat_run(loc, fr_np, G.gcc_phat_batch(fr_np, loc.dims.S, win, lut), (kind, M, N, fs))
    loc.close()


@pytest.mark.parametrize("kind", WC.WINDOWS)
@pytest.mark.parametrize("M,N,fs,mics,kernel", WC.PCM16)
def test_pcm16_batch_against_float64(oracle, kind, M, N, fs, mics, kernel):
    loc, win = _loc("gcc_phat", kind, M, N, fs, mics, sample_format="pcm16")
    assert loc.batch_kernel() == kernel
    lut = WC.lut_cpu(oracle, M, fs, mics)
    fr_np = WC.pcm16_batch(lut, M, N, fs)
    _check_phat_run(loc, fr_np, pcm16_ref.gcc_phat_pcm16(fr_np, loc.dims.S, win, lut), (kind, "pcm16", M, N))
    loc.close()


@pytest.mark.parametrize("kind", WC.WINDOWS)
def test_direct_stream_bit_for_bit(oracle, kind):
    c = WC.STREAM
    loc, win = _loc("direct", kind, c["M"], c["N"], c["fs"], None)
    lut = loc.lut()
    adc = WC.stream_capture(lut)
    pipe = StreamPipeline(loc, torch.from_numpy(adc[:, :2048]).cuda().contiguous(), hop=c["hop"])
    assert pipe.kernel == "k_direct_mfma"  # staged from the rings, the EMA inside
    pipe.close()
    exp = oracle.stream_run(adc, c["N"], c["fs"], c["S"], win, lut)
    assert exp["gate"].sum() >= 20
    for use_graph in (False, True):
        recs, est, last = TS.run_pipeline(loc, adc, c["hop"], use_graph=use_graph)
        TS.compare(recs, est, last, exp, loc.dims.P)
    loc.close()


@pytest.mark.parametrize("kind", WC.WINDOWS)
def test_phat_stream_against_float64(oracle, kind):
    c = WC.STREAM
    loc, win = _loc("gcc_phat", kind, c["M"], c["N"], c["fs"], None)
    lut = loc.lut()
    adc = WC.stream_capture(lut)
    pipe = StreamPipeline(loc, torch.from_numpy(adc[:, :2048]).cuda().contiguous(), hop=c["hop"])
    assert pipe.kernel == "k_stream_phat"
    pipe.close()
    ref = stream_phat_ref.run(oracle, adc, c["N"], c["fs"], c["S"], win, lut)
    assert ref["gate"].sum() >= 20
    runs = []
    for use_graph in (False, True):
        runs.append(TSF.run_pipeline(loc, adc, c["hop"], use_graph=use_graph))
        assert TSF.compare(runs[-1], ref, max_dropped=0, max_skip=0.0) == (0, 0)
    TSF.assert_bitwise(runs[1], runs[0])
    loc.close()
