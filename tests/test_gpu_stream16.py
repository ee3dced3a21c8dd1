"""Streaming GCC_PHAT on int16 capture rings (tdoa_stream_create_pcm16:
k_stream_trigger_lds<int16_t>, k_stream_phat_pcm16) against the float64 reference of
tests/stream16_ref.py.

Comparison rules: those of tests/test_gpu_stream_phat.py (its feed, compare
and assert_bitwise are used as they are): end, stream_id, count and totals()
exact; lags and gate exact while the stream is not dropped; ema_best exact
where the EMA row's margin exceeds TOL_LAG_MARGIN; cell exact where the map gap
exceeds TOL_CELL_MARGIN, else within that margin of the maximum; max_Lf within
TOL_MAXL; est within TOL_EST.  tests/test_stream16_cpu.py checks on the CPU
that the reference alone drops no stream and stays within each case's
cell-skip cap for every seed used here (tests/stream16_cases.py).
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import band_ref  # noqa: E402
import stream16_cases as Cs  # noqa: E402
import stream16_ref as R  # noqa: E402
import tdoa  # noqa: E402
from tdoa import _lib  # noqa: E402
from tdoa.localizer import Localizer  # noqa: E402
from tdoa.stream import StreamPipeline  # noqa: E402
from test_gpu_stream_phat import assert_bitwise, compare, feed  # noqa: E402

FS = Cs.FS


def _loc(M=3, N=1024, fmt="pcm16", engine="gcc_phat"):
    return Localizer(engine=engine, num_mics=M, frame_len=N, sample_rate_hz=FS, mic_xy=Cs.MICS[M],
                     sample_format=fmt)


def run_pipeline(loc, cap, hop, use_graph=False, capture_len=None, trigger_var=None):
    """Every full hop of the int16 capture `cap` through a new pipeline."""
    S, _, M = cap.shape
    src = None
    if capture_len is None:
        ring = torch.from_numpy(cap).cuda()
    else:  # a producer-fed ring
        ring = torch.zeros((S, capture_len, M), dtype=torch.int16, device="cuda")
        src = torch.from_numpy(cap).cuda()
    pipe = StreamPipeline(loc, ring, hop=hop, use_graph=use_graph, trigger_var=trigger_var)
    got = feed(pipe, cap, hop, capture_len, src)
    pipe.close()
    return got


def assert_trigger(got, trig):
    """count, stream_id and end exact against trigger positions n_trig / end."""
    recs, _, _, totals = got
    for s, lst in recs.items():
        assert len(lst) == trig["n_trig"][s], (s, len(lst), trig["n_trig"][s])
        assert [int(g["end"]) for g in lst] == [int(e) for e in trig["end"][s, :len(lst)]], s
    assert totals[1] == int(trig["n_trig"].sum())


@pytest.fixture(scope="module")
def loc3():
    loc = _loc()
    assert loc.dims.S == Cs.S_LAG
    yield loc
    loc.close()


@pytest.fixture(scope="module")
def scaled(oracle, loc3):
    """Case 1's captures, the reference and the eager run (shared, not modified)."""
    lut = loc3.lut()
    assert np.array_equal(np.asarray(lut).reshape(3, -1), Cs.lut_cpu(oracle, 3).reshape(3, -1))
    adc, cap = Cs.scaled8(lut)
    ref = R.run(oracle, cap, 1024, FS, loc3.dims.S, loc3.window(), lut)
    return adc, cap, ref, run_pipeline(loc3, cap, 512)


def test_scaled_8bit_capture(oracle, loc3, scaled):
    """(u8 - 128) * 256 of the 8-bit config-5 test capture at the default
    trigger_var: the trigger positions are the pinned 8-bit oracle's.  The
    reference alone: 323 frames, all gated, no stream dropped, no cell skipped,
    minimum map gap 4.1e-2."""
    adc, cap, ref, got = scaled
    lut = loc3.lut()
    direct = oracle.stream_run(adc, 1024, FS, loc3.dims.S, loc3.window(), np.asarray(lut).reshape(3, -1), max_trig=64)
    assert np.array_equal(ref["n_trig"], direct["n_trig"]) and np.array_equal(ref["end"], direct["end"])
    assert_trigger(got, direct)
    assert ref["n_trig"].sum() > 200 and ref["gate"].sum() > 100
    compare(got, ref)


def test_true_16bit_capture(oracle, loc3):
    """A 30-count source over 4 counts of noise on offsets up to +-12000.  The
    reference alone: 328 frames, all gated, none dropped or skipped (minimum
    map gap 3.9e-2); truncated to the 8 bits of a converter with the same full
    scale, 321 of the 328 frames get other lags (tests/test_stream16_cpu.py)."""
    lut = loc3.lut()
    cap = Cs.true16(lut)
    assert np.abs(cap.astype(np.int64).mean((0, 1))).max() > 11000
    ref = R.run(oracle, cap, 1024, FS, loc3.dims.S, loc3.window(), lut, trigger_var=Cs.TRUE16_VAR)
    assert ref["n_trig"].sum() > 200 and ref["gate"].sum() > 100
    # 8 bits are not enough here: the reference on the truncated frames finds other lags
    import pcm16_ref
    idx = [(s, i) for s in range(40) for i in range(ref["n_trig"][s])][::8]
    tr = Cs.truncated8(cap)
    fr = np.stack([np.ascontiguousarray(tr[s, ref["end"][s, i] - 1024:ref["end"][s, i]].T) for s, i in idx])
    lt = pcm16_ref.gcc_phat_pcm16(fr, loc3.dims.S, loc3.window())["lags"]
    assert sum(bool((lt[b] != ref["lags"][s, i]).any()) for b, (s, i) in enumerate(idx)) > len(idx) // 2
    compare(run_pipeline(loc3, cap, 512, trigger_var=Cs.TRUE16_VAR), ref)


def test_graph_equals_eager(loc3, scaled, monkeypatch):
    _, cap, ref, eager = scaled
    graph = run_pipeline(loc3, cap, 512, use_graph=True)
    compare(graph, ref)
    assert_bitwise(graph, eager)
    # two workgroups walk up to 40 slots: records and state as the uncapped run's
    monkeypatch.setenv("TDOA_STREAM_PHAT_GRID", "2")
    assert_bitwise(run_pipeline(loc3, cap, 512), eager)


@pytest.mark.parametrize("N,hop,M,hops,seed,max_skip", Cs.SHAPES)
def test_other_shapes(oracle, N, hop, M, hops, seed, max_skip):
    """Six streams each, graph and eager.  The float64 reference alone drops no
    stream at these seeds; it skips 16.9 % of the 59 gated records of
    (2048, 1024, 4 mics) (the square array's maps have near-ties; cap 25 %) and
    none elsewhere: 26, 21, 73 and 30 gated records, minimum map gaps 3.0e-2,
    4.1e-2, 1.0e-2 and 1.6e-3 (8 mics)."""
    loc = _loc(M, N)
    lut, S = loc.lut(), loc.dims.S
    cap = Cs.shape_capture(lut, N, hop, M, hops, seed)
    ref = R.run(oracle, cap, N, FS, S, loc.window(), lut, hop=hop)
    assert ref["gate"].sum() > 10
    for use_graph in (False, True):
        compare(run_pipeline(loc, cap, hop, use_graph=use_graph), ref, max_skip=max_skip)
    loc.close()


@pytest.mark.parametrize("capture_len", [2048, 2049])
def test_capture_ring_wraps(oracle, loc3, capture_len):
    """A producer-fed ring; with the odd length every other stream's ring starts
    2-byte aligned only (stride capture_len * 3 * 2 bytes).  The reference
    alone: 30 frames, all gated, none dropped or skipped."""
    lut = loc3.lut()
    cap = Cs.small_capture(lut, Cs.WRAP_SEED)
    ref = R.run(oracle, cap, 1024, FS, loc3.dims.S, loc3.window(), lut)
    for use_graph in (False, True):
        compare(run_pipeline(loc3, cap, 512, use_graph=use_graph, capture_len=capture_len), ref)


@pytest.mark.parametrize("trigger_var", Cs.TRIGGER_VARS)
def test_trigger_var(loc3, trigger_var):
    """0 (any excess of the older half's power fires: 51 triggers, most of them
    on the noise floor), the default (29: every burst) and 2.8e7 (7: under half
    the bursts).  Counts and positions exact; the scores of noise-floor frames
    have no clear maximum and are not compared."""
    cap = Cs.small_capture(loc3.lut(), Cs.VAR_SEED)
    trig = R.trigger16(cap, 1024, 512, trigger_var)
    if trigger_var == Cs.TRIGGER_VARS[2]:
        assert 0 < trig["n_trig"].sum() < R.trigger16(cap, 1024, 512, 131072)["n_trig"].sum() / 2
    assert_trigger(run_pipeline(loc3, cap, 512, trigger_var=trigger_var), trig)


def test_full_scale_trigger():
    """Alternating N/2-sample blocks of near-silence and +-32767 at N = 2048,
    4 mics: pw near 2^49 per mic.  Trigger exact; the scores only finite and
    in range (fp32 on 96 dB coloured input is outside the score tolerance)."""
    c = Cs.FULL_SCALE
    loc = _loc(c["M"], c["N"])
    cap = R.full_scale_capture(c["ns"], c["T"], c["N"], c["M"], c["seed"])
    trig = R.trigger16(cap, c["N"], 1024, 131072, python_int=True)
    assert (trig["n_trig"] >= 3).all()
    for use_graph in (False, True):
        got = run_pipeline(loc, cap, 1024, use_graph=use_graph)
        assert_trigger(got, trig)
        recs, est, _, _ = got
        assert np.isfinite(est).all()
        for lst in recs.values():
            for g in lst:
                assert np.abs(g["lags"]).max() <= loc.dims.S
                if g["gate"]:
                    assert np.isfinite(g["max_Lf"]) and 0 <= g["cell"] < 101 * 101
    loc.close()


@pytest.mark.parametrize("use_graph", [False, True])
def test_band_table_read_per_step(oracle, use_graph):
    """set_band, run, clear, reset, run: both runs match the reference.  The
    reference alone: 64 frames, all gated, none dropped or skipped (minimum map
    gaps 1.4e-3 banded, 4.1e-2 plain)."""
    loc = _loc()
    lut, win, S = loc.lut(), loc.window(), loc.dims.S
    cap = Cs.small_capture(lut, Cs.BAND_SEED, streams=8, hops=40)
    loc.set_band(1000, 6000, 500)
    pipe = StreamPipeline(loc, torch.from_numpy(cap).cuda(), hop=512, use_graph=use_graph)
    band = R.run(oracle, cap, 1024, FS, S, win, lut, w=band_ref.band_weights(1024, FS, 1000, 6000, 500))
    compare(feed(pipe, cap, 512), band)
    torch.cuda.synchronize()  # the setters want no step in flight
    loc.set_bin_weights(None)
    pipe.reset()
    plain = R.run(oracle, cap, 1024, FS, S, win, lut)
    assert not np.array_equal(plain["est"], band["est"])
    compare(feed(pipe, cap, 512), plain)
    pipe.close()
    loc.close()


def _create16(ctx, cap, S=2, hop=512, capture_len=4096, trigger_var=131072):
    h = C.c_void_p()
    rc = tdoa.load().tdoa_stream_create_pcm16(ctx, S, hop, C.c_void_p(cap.data_ptr()), capture_len, trigger_var,
                                              0, C.byref(h))
    msg = tdoa.load().tdoa_last_error() or b""
    if rc == 0:
        tdoa.load().tdoa_stream_destroy(h)
    return rc, msg.decode()


def test_api_contract(oracle, loc3):
    cap16 = torch.zeros((2, 4096, 3), dtype=torch.int16, device="cuda")
    cap8 = torch.zeros((2, 4096, 3), dtype=torch.uint8, device="cuda")
    # ---- the C entry point's rejections: code -1 and a message naming the cause
    assert _create16(loc3._ctx, cap16)[0] == 0
    direct = _loc(fmt="adc8", engine="direct")
    rc, msg = _create16(direct._ctx, cap16)
    assert rc == -1 and "GCC_PHAT" in msg
    adc8 = _loc(fmt="adc8")
    rc, msg = _create16(adc8._ctx, cap16)
    assert rc == -1 and "ADC8" in msg
    for tv in (-1, (1 << 30) + 1):
        rc, msg = _create16(loc3._ctx, cap16, trigger_var=tv)
        assert rc == -1 and "trigger_var" in msg
    assert _create16(loc3._ctx, cap16, trigger_var=0)[0] == 0 and _create16(loc3._ctx, cap16, trigger_var=1 << 30)[0] == 0
    rc, msg = _create16(loc3._ctx, cap16, hop=1025)
    assert rc == -1 and "hop" in msg
    rc, msg = _create16(loc3._ctx, cap16, capture_len=1024 + 2 * 512 - 1)
    assert rc == -1 and "capture_len" in msg
    big = _loc(8, 4096)  # outside the k_stream_phat LDS rule
    rc, msg = _create16(big._ctx, torch.zeros((1, 8192, 8), dtype=torch.int16, device="cuda"), S=1, hop=2048,
                        capture_len=8192)
    assert rc == -1 and "8 mics" in msg and "4096" in msg
    big.close()
    wide = _loc(8, 1024)  # fits k_stream_phat (80 KiB); its trigger at hop 1024 fits too
    assert _create16(wide._ctx, torch.zeros((1, 4096, 8), dtype=torch.int16, device="cuda"), S=1, hop=1024)[0] == 0
    wide.close()

    # ---- Python
    with pytest.raises(tdoa.TdoaError) as e:  # a uint8 ring on a PCM16 localizer reaches tdoa_stream_create
        StreamPipeline(loc3, cap8, hop=512)
    assert e.value.code == -1
    for bad in (adc8, direct):
        with pytest.raises(ValueError):
            StreamPipeline(bad, cap16, hop=512)
    with pytest.raises(ValueError):
        StreamPipeline(adc8, cap8, hop=512, trigger_var=131072)
    with pytest.raises(tdoa.TdoaError) as e:
        StreamPipeline(loc3, cap16, hop=512, trigger_var=-5)
    assert e.value.code == -1
    direct.close()
    adc8.close()

    pipe = StreamPipeline(loc3, cap16, hop=512)
    assert pipe.trigger_var == 131072
    assert "max_Lf" in pipe.out and "max_L" not in pipe.out and pipe.out["max_Lf"].dtype == torch.float32
    L = tdoa.load()
    assert L.tdoa_stream_step(pipe._h, C.byref(_lib.StreamOutputs()), None) == -1
    est = np.zeros((2, 3, loc3.dims.K), np.int64)
    assert L.tdoa_stream_state(pipe._h, None, est.ctypes.data_as(C.c_void_p), None, None) == -1
    assert pipe.totals() == (0, 0, 0)
    assert pipe.state()[1].dtype == np.float32
    pipe.close()


def test_pipeline_keeps_its_format_and_reset_reproduces(oracle):
    """A pipeline created in PCM16 keeps stepping 16-bit after the localizer
    returns to adc8; reset() reproduces the first run bitwise.  The reference
    alone: 18 frames, all gated, none dropped or skipped."""
    loc = _loc()
    lut, win, S = loc.lut(), loc.window(), loc.dims.S
    cap = Cs.small_capture(lut, Cs.API_SEED, hops=16)
    ref = R.run(oracle, cap, 1024, FS, S, win, lut)
    assert ref["gate"].sum() > 10
    pipe = StreamPipeline(loc, torch.from_numpy(cap).cuda(), hop=512)
    loc.set_sample_format("adc8")
    assert loc.sample_format == "adc8"
    first = feed(pipe, cap, 512)
    compare(first, ref)
    pipe.reset()
    assert_bitwise(feed(pipe, cap, 512), first)
    pipe.close()
    loc.close()
