"""Continuous streaming (tdoa_stream_create_continuous: k_stream_active in place
of a trigger, then k_stream_phat / k_stream_phat_pcm16) against the float64
reference of tests/stream_cont_ref.py.

Comparison rules: those of tests/test_gpu_stream_phat.py (its feed, compare and
assert_bitwise are used as they are): end, stream_id, count and totals() exact;
lags and gate exact while the stream is not dropped; ema_best exact where the
EMA row's margin exceeds TOL_LAG_MARGIN; cell exact where the map gap exceeds
TOL_CELL_MARGIN, else within that margin of the maximum; max_Lf within
TOL_MAXL; est within TOL_EST.  tests/test_stream_cont_cpu.py checks on the CPU
that the reference alone drops no stream and stays within each case's cell-skip
cap (tests/stream_cont_cases.py).  Runs at activity_var = 0 list noise-only
frames, whose scores have no clear maximum: they are compared on the list only.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import band_ref  # noqa: E402
import stream16_ref  # noqa: E402
import stream_cont_cases as Cs  # noqa: E402
import stream_cont_ref as R  # noqa: E402
import stream_phat_ref  # noqa: E402
import tdoa  # noqa: E402
from tdoa import _lib, synth  # noqa: E402
from tdoa.localizer import Localizer  # noqa: E402
from tdoa.stream import StreamPipeline  # noqa: E402
from test_gpu_stream_phat import assert_bitwise, compare, feed  # noqa: E402

FS = Cs.FS
ALL = [(fmt, *c) for fmt in ("pcm16", "adc8") for c in Cs.CASES[fmt]]
BAND = (1000, 6000, 500)


def _loc(M=3, N=1024, fmt="pcm16", engine="gcc_phat"):
    return Localizer(engine=engine, num_mics=M, frame_len=N, sample_rate_hz=FS, mic_xy=Cs.MICS[M],
                     sample_format=fmt)


def run_pipeline(loc, cap, hop, activity_var=None, use_graph=False, capture_len=None):
    """Every full hop of `cap` (uint8 or int16) through a new continuous pipeline."""
    S, _, M = cap.shape
    src = None
    if capture_len is None:
        ring = torch.from_numpy(cap).cuda()
    else:  # a producer-fed ring; + 4 spare bytes behind a uint8 one, as the triggered tests keep them
        dt = torch.from_numpy(cap[:0]).dtype
        flat = torch.zeros(S * capture_len * M + (4 if dt == torch.uint8 else 0), dtype=dt, device="cuda")
        ring = flat[:S * capture_len * M].view(S, capture_len, M)
        src = torch.from_numpy(cap).cuda()
    pipe = StreamPipeline(loc, ring, hop=hop, use_graph=use_graph, mode="continuous", activity_var=activity_var)
    got = feed(pipe, cap, hop, capture_len, src)
    pipe.close()
    return got


def assert_list(got, act):
    """count, stream_id and end exact against the listed frames n_trig / end."""
    recs, _, _, totals = got
    for s, lst in recs.items():
        assert [int(g["end"]) for g in lst] == [int(e) for e in act["end"][s, :act["n_trig"][s]]], s
    assert totals[1] == int(act["n_trig"].sum())


_refs = {}


def case_ref(oracle, loc, fmt, N, hop, M, hops, seed, var, band=None):
    """The case's capture and float64 reference, computed once and not modified."""
    key = (fmt, N, hop, M, hops, seed, var, band)
    if key not in _refs:
        lut = loc.lut()
        cap = Cs.capture(fmt, lut, N, hop, M, hops, seed)
        w = None if band is None else band_ref.band_weights(N, FS, *band)
        _refs[key] = cap, R.run(oracle, cap, N, FS, loc.dims.S, loc.window(), lut, hop, var, w=w)
    return _refs[key]


@pytest.mark.parametrize("fmt,N,hop,M,hops,seed,var", ALL)
def test_cases(oracle, monkeypatch, fmt, N, hop, M, hops, seed, var):
    """The ten cases, eager and graph-captured, each against the reference; the
    graph's records and state are the eager run's bit for bit, and so are those
    of two workgroups walking the list (TDOA_STREAM_PHAT_GRID=2)."""
    loc = _loc(M, N, "pcm16" if fmt == "pcm16" else "adc8")
    assert loc.dims.S == Cs.S_LAG
    cap, ref = case_ref(oracle, loc, fmt, N, hop, M, hops, seed, var)
    assert ref["n_trig"].sum() >= 90
    eager = run_pipeline(loc, cap, hop, var)
    compare(eager, ref, max_skip=Cs.max_skip(M))
    graph = run_pipeline(loc, cap, hop, var, use_graph=True)
    compare(graph, ref, max_skip=Cs.max_skip(M))
    assert_bitwise(graph, eager)
    monkeypatch.setenv("TDOA_STREAM_PHAT_GRID", "2")
    assert_bitwise(run_pipeline(loc, cap, hop, var), eager)
    loc.close()


@pytest.mark.parametrize("fmt,case,var", [("pcm16", 0, 0), ("pcm16", 0, 20000000), ("pcm16", 3, 0),
                                          ("adc8", 1, 0), ("adc8", 1, 1200), ("adc8", 4, 0)])
def test_list_only(fmt, case, var):
    """activity_var = 0 lists every stream at every hop with e >= N and none
    before (hop 384 at N = 1024: the first frame ends at 1152); a threshold
    above the cases' lists fewer.  Counts and ends exact."""
    N, hop, M, hops, seed, _ = Cs.CASES[fmt][case]
    loc = _loc(M, N, fmt)
    cap = Cs.capture(fmt, loc.lut(), N, hop, M, hops, seed)
    act = R.active(cap, N, hop, var)
    first = -(-N // hop) * hop
    if var == 0:
        assert (act["n_trig"] == hops - first // hop + 1).all() and (act["end"][:, 0] == first).all()
    else:
        assert 0 < act["n_trig"].sum() < R.active(cap, N, hop, Cs.CASES[fmt][case][5])["n_trig"].sum()
    for use_graph in (False, True):
        assert_list(run_pipeline(loc, cap, hop, var, use_graph=use_graph), act)
    # the hops before the first full frame report a count of 0
    pipe = StreamPipeline(loc, torch.from_numpy(cap).cuda(), hop=hop, mode="continuous", activity_var=0)
    for h in range(first // hop):
        pipe.step()
        pipe.stream.synchronize()
        assert int(pipe.out["count"].item()) == (Cs.STREAMS if (h + 1) * hop >= N else 0), h
    assert pipe.totals() == (first, Cs.STREAMS, pipe.totals()[2])
    pipe.close()
    loc.close()


@pytest.mark.parametrize("fmt", ["pcm16", "adc8"])
def test_exact_boundary(fmt):
    """+100, -100, ... on every mic of 3 (around 128 on a uint8 ring): sum_m pw
    = 3 * 100^2 * N^2, so activity_var 30000 lists every eligible hop and 30001
    none; a constant ring has pw = 0, listed at 0 and never at 1."""
    loc = _loc(3, 1024, fmt)
    alt = Cs.alternating(512 * 8, 3)
    if fmt == "adc8":
        alt = (alt + 128).astype(np.uint8)
    const = np.full_like(alt, 77)
    cap = np.stack([alt, const, alt])
    want = {30000: [7, 0, 7], 30001: [0, 0, 0], 0: [7, 7, 7], 1: [7, 0, 7]}
    for var, n in want.items():
        act = R.active(cap, 1024, 512, var)
        assert list(act["n_trig"]) == n
        assert int(act["total"][0, 1]) == 3 * 100 * 100 * 1024 * 1024 and int(act["total"][1, 1]) == 0
        assert_list(run_pipeline(loc, cap, 512, var), act)
    loc.close()


@pytest.mark.parametrize("fmt", ["pcm16", "adc8"])
@pytest.mark.parametrize("capture_len", [2048, 2049])
@pytest.mark.parametrize("shape", ["small", "case0"])
def test_capture_ring_wraps(oracle, fmt, capture_len, shape):
    """Producer-fed rings.  With the odd length the rings start 1-byte (uint8)
    or 2-byte (int16) aligned only and a frame wraps anywhere, so the element
    loads serve; with the even one the frames of N = 1024, hop 512 wrap between
    two 16-byte vectors.  small: N = 256, hop 256, 3 mics (4 samples per lane)."""
    if shape == "small":
        c = Cs.SMALL
        case = (c["N"], c["hop"], c["M"], c["hops"], Cs.SMALL_SEED[fmt], Cs.SMALL_VAR[fmt])
    else:
        case = Cs.CASES[fmt][0]
    N, hop, M, hops, seed, var = case
    loc = _loc(M, N, fmt)
    cap, ref = case_ref(oracle, loc, fmt, *case)
    assert ref["gate"].sum() > 10
    for use_graph in (False, True):
        compare(run_pipeline(loc, cap, hop, var, use_graph=use_graph, capture_len=capture_len), ref)
    loc.close()


@pytest.mark.parametrize("N,M,hop,ns,T,seed", Cs.FULL_SCALE)
def test_full_scale(N, M, hop, ns, T, seed):
    """Alternating N/2-sample blocks of near-silence and full scale on int16
    rings: sum x^2 near N 2^29 per mic.  Lists exact against the Python-int
    rule at 2^30 (and at 2^20, which every frame passes); the scores only finite
    and in range (fp32 on 96 dB coloured input is outside the score tolerance)."""
    loc = _loc(M, N)
    cap = stream16_ref.full_scale_capture(ns, T, N, M, seed)
    for var, use_graph in ((1 << 30, False), (1 << 30, True), (1 << 20, False)):
        act = R.active(cap, N, hop, var, python_int=True)
        if var == 1 << 20:
            assert (act["n_trig"] == T // hop - N // hop + 1).all()
        got = run_pipeline(loc, cap, hop, var, use_graph=use_graph)
        assert_list(got, act)
        recs, est, _, _ = got
        assert np.isfinite(est).all()
        for lst in recs.values():
            for g in lst:
                assert np.abs(g["lags"]).max() <= loc.dims.S
                if g["gate"]:
                    assert np.isfinite(g["max_Lf"]) and 0 <= g["cell"] < 101 * 101
    loc.close()


@pytest.mark.parametrize("fmt,use_graph", [("pcm16", True), ("adc8", False)])
def test_band_table_read_per_step(oracle, fmt, use_graph):
    """set_band, run, clear, reset, run: both runs match the reference, and a
    second reset reproduces the plain run bitwise."""
    case = Cs.CASES[fmt][0]
    N, hop, M, hops, seed, var = case
    loc = _loc(M, N, fmt)
    cap, plain = case_ref(oracle, loc, fmt, *case)
    _, band = case_ref(oracle, loc, fmt, *case, band=BAND)
    assert not np.array_equal(plain["est"], band["est"])
    loc.set_band(*BAND)
    pipe = StreamPipeline(loc, torch.from_numpy(cap).cuda(), hop=hop, use_graph=use_graph, mode="continuous",
                          activity_var=var)
    compare(feed(pipe, cap, hop), band)
    torch.cuda.synchronize()  # the setters want no step in flight
    loc.set_bin_weights(None)
    pipe.reset()
    first = feed(pipe, cap, hop)
    compare(first, plain)
    pipe.reset()
    assert_bitwise(feed(pipe, cap, hop), first)
    pipe.close()
    loc.close()


def _create(ctx, cap, S=2, hop=512, capture_len=4096, activity_var=0, out=True):
    h = C.c_void_p()
    ptr = C.c_void_p(cap if isinstance(cap, int) else cap.data_ptr()) if cap is not None else None
    rc = tdoa.load().tdoa_stream_create_continuous(ctx, S, hop, ptr, capture_len, activity_var, 0,
                                                   C.byref(h) if out else None)
    msg = tdoa.load().tdoa_last_error() or b""
    if rc == 0:
        tdoa.load().tdoa_stream_destroy(h)
    return rc, msg.decode()


def test_api_contract(oracle):
    loc16, loc8, direct = _loc(), _loc(fmt="adc8"), _loc(fmt="adc8", engine="direct")
    cap16 = torch.zeros((2, 4096, 3), dtype=torch.int16, device="cuda")
    cap8 = torch.zeros((2, 4096, 3), dtype=torch.uint8, device="cuda")
    # ---- the C entry point: the ring's type is the context's format; rejections by code and cause
    assert _create(loc16._ctx, cap16)[0] == 0 and _create(loc8._ctx, cap8)[0] == 0
    for rc, msg in (_create(None, cap16), _create(loc16._ctx, None), _create(loc16._ctx, cap16, out=False)):
        assert rc == -1 and "NULL" in msg
    rc, msg = _create(direct._ctx, cap8)
    assert rc == -1 and "GCC_PHAT" in msg
    for av in (-1, (1 << 30) + 1):
        rc, msg = _create(loc16._ctx, cap16, activity_var=av)
        assert rc == -1 and "activity_var" in msg
    assert _create(loc16._ctx, cap16, activity_var=1 << 30)[0] == 0
    for hop in (0, 1025):
        rc, msg = _create(loc16._ctx, cap16, hop=hop)
        assert rc == -1 and "hop" in msg
    assert _create(loc16._ctx, cap16, hop=1024, capture_len=3072)[0] == 0
    rc, msg = _create(loc16._ctx, cap16, capture_len=1024 + 2 * 512 - 1)
    assert rc == -1 and "capture_len" in msg
    rc, msg = _create(loc16._ctx, cap16.data_ptr() + 1, capture_len=2048)
    assert rc == -1 and "2-byte" in msg
    assert _create(loc8._ctx, cap8.data_ptr() + 1, capture_len=2048)[0] == 0  # bytes need no alignment
    big = _loc(8, 4096)  # outside the k_stream_phat LDS rule
    rc, msg = _create(big._ctx, torch.zeros((1, 8192, 8), dtype=torch.int16, device="cuda"), S=1, hop=2048,
                      capture_len=8192)
    assert rc == -1 and "8 mics" in msg and "4096" in msg
    big.close()

    # ---- Python
    with pytest.raises(ValueError):
        StreamPipeline(loc16, cap16, hop=512, activity_var=0)  # triggered mode takes no activity_var
    with pytest.raises(ValueError):
        StreamPipeline(loc16, cap16, hop=512, mode="continuous", trigger_var=131072)
    with pytest.raises(ValueError):
        StreamPipeline(loc16, cap16, hop=512, mode="always")
    with pytest.raises(ValueError):
        StreamPipeline(direct, cap8, hop=512, mode="continuous")
    for loc, cap in ((loc16, cap8), (loc8, cap16)):  # the ring's type follows loc.sample_format
        with pytest.raises(ValueError):
            StreamPipeline(loc, cap, hop=512, mode="continuous")
    with pytest.raises(tdoa.TdoaError) as e:
        StreamPipeline(loc16, cap16, hop=512, mode="continuous", activity_var=-5)
    assert e.value.code == -1
    trig = StreamPipeline(loc16, cap16, hop=512)
    assert trig.mode == "triggered" and trig.activity_var is None and trig.trigger_var == 131072
    trig.close()

    for loc, cap in ((loc16, cap16), (loc8, cap8)):
        pipe = StreamPipeline(loc, cap, hop=512, mode="continuous")
        assert pipe.mode == "continuous" and pipe.activity_var == 0
        assert "max_Lf" in pipe.out and "max_L" not in pipe.out and pipe.out["max_Lf"].dtype == torch.float32
        L = tdoa.load()
        assert L.tdoa_stream_step(pipe._h, C.byref(_lib.StreamOutputs()), None) == -1
        assert b"tdoa_stream_step_f" in L.tdoa_last_error()
        est = np.zeros((2, 3, loc.dims.K), np.int64)
        assert L.tdoa_stream_state(pipe._h, None, est.ctypes.data_as(C.c_void_p), None, None) == -1
        assert pipe.totals() == (0, 0, 0)
        assert pipe.state()[1].dtype == np.float32
        pipe.step()
        pipe.step()  # e = 1024: both all-zero streams are listed at activity_var 0
        assert pipe.totals()[:2] == (1024, 2)
        pipe.close()
    assert StreamPipeline(loc16, cap16, hop=512, mode="continuous", activity_var=9).activity_var == 9

    # ---- a PCM16 pipeline keeps stepping int16 after the localizer returns to adc8
    case = Cs.PCM16_CASES[0]
    N, hop, M, hops, seed, var = case
    cap, ref = case_ref(oracle, loc16, "pcm16", *case)
    pipe = StreamPipeline(loc16, torch.from_numpy(cap).cuda(), hop=hop, mode="continuous", activity_var=var)
    loc16.set_sample_format("adc8")
    assert loc16.sample_format == "adc8"
    compare(feed(pipe, cap, hop), ref)
    pipe.close()
    for loc in (loc16, loc8, direct):
        loc.close()


def test_triggered_default_path_is_untouched(oracle):
    """A triggered StreamPipeline with default arguments on a uint8 ring, as
    tests/test_gpu_stream_phat.py compares it: the click trigger's frames."""
    loc = _loc(fmt="adc8")
    lut = loc.lut()
    adc = synth.adc_stream(6, 512 * 24, 3, lut, loc.dims.S, 23).numpy()
    ref = stream_phat_ref.run(oracle, adc, 1024, FS, loc.dims.S, loc.window(), lut)
    assert ref["gate"].sum() > 10
    pipe = StreamPipeline(loc, torch.from_numpy(adc).cuda(), hop=512)
    assert pipe.mode == "triggered"
    compare(feed(pipe, adc, 512), ref)
    pipe.close()
    loc.close()
