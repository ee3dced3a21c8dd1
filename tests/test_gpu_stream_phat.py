"""Streaming GCC_PHAT (k_stream_phat behind tdoa_stream_step_f) against the
float64 reference of tests/stream_phat_ref.py.

Comparison rules (the project's GCC-PHAT tolerances, stream_phat_ref.TOL_*):
end, stream_id, count and totals() exact; lags (and with them gate) equal where
the frame's float64 raw top-2 margin exceeds 2e-4; ema_best equal where the EMA
row's margin exceeds 2e-4; cell and xy equal where the gap between the EMA
map's two highest distinct values exceeds 1e-3, elsewhere ("skipped") the
float64 map at the GPU's cell within 1e-3 of its maximum; max_Lf within 1e-3;
final est within 5e-5 (the 3e-5 score tolerance, kept by a convex combination,
plus at most 64 fp32 update roundings of values <= 1); last exact.  A stream is
dropped from its first frame whose raw margin is <= 2e-4 (its gate history may
differ from there on); every case caps the streams dropped and cells skipped.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import band_ref  # noqa: E402
import stream_phat_ref as R  # noqa: E402
import tdoa  # noqa: E402
from tdoa import _lib, synth  # noqa: E402
from tdoa.localizer import Localizer  # noqa: E402
from tdoa.stream import StreamPipeline  # noqa: E402

FS = 48000
MICS = {2: np.array([[-0.066, 0], [0.066, 0]], np.float32), 3: None, 4: synth.square_mics(0.15),
        8: synth.circle_mics()}


def _loc(M=3, N=1024, engine="gcc_phat"):
    return Localizer(engine=engine, num_mics=M, frame_len=N, sample_rate_hz=FS, mic_xy=MICS[M])


def feed(pipe, adc, hop, capture_len=None, src=None):
    """Every full hop through `pipe`; per-stream record lists, state, totals."""
    S, T, _ = adc.shape
    recs = {s: [] for s in range(S)}
    for h in range(T // hop):
        if capture_len is not None:  # producer-fed capture ring
            with torch.cuda.stream(pipe.stream):
                idx = torch.arange(h * hop, (h + 1) * hop, device="cuda") % capture_len
                pipe.capture[:, idx] = src[:, h * hop:(h + 1) * hop]
        pipe.step()
        r = pipe.records()
        for i, s in enumerate(r["stream_id"]):
            recs[int(s)].append({k: v[i] for k, v in r.items()})
    pos, est, last = pipe.state()
    assert pos == (T // hop) * hop
    return recs, est, last, pipe.totals()


def run_pipeline(loc, adc, hop, use_graph=False, capture_len=None):
    S, _, M = adc.shape
    src = None
    if capture_len is None:
        cap = torch.from_numpy(adc).cuda()
    else:
        # + 4 spare bytes: an unaligned last ring may be read word-wise by the trigger
        flat = torch.zeros(S * capture_len * M + 4, dtype=torch.uint8, device="cuda")
        cap = flat[:S * capture_len * M].view(S, capture_len, M)
        src = torch.from_numpy(adc).cuda()
    pipe = StreamPipeline(loc, cap, hop=hop, use_graph=use_graph)
    got = feed(pipe, adc, hop, capture_len, src)
    pipe.close()
    return got


def compare(got, ref, max_dropped=0, max_skip=0.0):
    recs, est, last, totals = got
    assert est.dtype == np.float32
    n_trig = ref["n_trig"]
    first = R.dropped_streams(ref)
    dropped = int((first < n_trig).sum())
    gated = skipped = 0
    worst_est = worst_L = 0.0
    for s, lst in recs.items():
        assert len(lst) == n_trig[s], (s, len(lst), n_trig[s])  # the trigger does not depend on the engine
        for i, g in enumerate(lst):
            assert g["end"] == ref["end"][s, i]
            assert "max_L" not in g
            if i >= first[s]:
                continue
            assert (g["lags"] == ref["lags"][s, i]).all(), (s, i)
            assert g["gate"] == ref["gate"][s, i]
            if not g["gate"]:
                assert g["cell"] == -1
                continue
            gated += 1
            sure = ref["ema_margin"][s, i] > R.TOL_LAG_MARGIN
            assert (g["ema_best"][sure] == ref["ema_best"][s, i][sure]).all(), (s, i)
            if ref["map_gap"][s, i] > R.TOL_CELL_MARGIN:
                assert g["cell"] == ref["cell"][s, i], (s, i)
                assert (g["xy"] == ref["xy"][s, i]).all()
            else:
                skipped += 1
                assert R.map_at(ref, s, i, int(g["cell"])) >= ref["max_Lf"][s, i] - R.TOL_CELL_MARGIN, (s, i)
            worst_L = max(worst_L, abs(float(g["max_Lf"]) - ref["max_Lf"][s, i]))
        if first[s] == n_trig[s]:
            worst_est = max(worst_est, float(np.abs(est[s] - ref["est"][s]).max()))
            assert last[s] == ref["last"][s]
    print(f"gated {gated}, dropped {dropped}, skipped {skipped}, max |est err| {worst_est:.2e}, "
          f"max |max_Lf err| {worst_L:.2e}")
    assert worst_L <= R.TOL_MAXL
    assert worst_est <= R.TOL_EST
    assert dropped <= max_dropped
    assert skipped <= max_skip * max(gated, 1)
    assert totals[1] == int(n_trig.sum())
    if dropped == 0:
        assert totals[2] == int(sum(ref["gate"][s, :n_trig[s]].sum() for s in range(n_trig.size)))
    return dropped, skipped


def assert_bitwise(a, b):
    assert a[3] == b[3]
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and np.array_equal(a[2], b[2])
    for s in a[0]:
        assert len(a[0][s]) == len(b[0][s])
        for x, y in zip(a[0][s], b[0][s]):
            for k in x:
                if x["gate"] or k in ("end", "stream_id", "lags", "gate", "cell"):
                    assert np.array_equal(np.atleast_1d(x[k]).view(np.uint8), np.atleast_1d(y[k]).view(np.uint8)), (s, k)


@pytest.fixture(scope="module")
def loc3():
    loc = _loc()
    yield loc
    loc.close()


@pytest.fixture(scope="module")
def config5(oracle, loc3):
    """Case 1's capture, its reference and the eager run (shared, not modified)."""
    lut = loc3.lut()
    adc = synth.adc_stream(40, 512 * 40, 3, lut, loc3.dims.S, 0x5EED0005).numpy()
    ref = R.run(oracle, adc, 1024, FS, loc3.dims.S, loc3.window(), lut)
    return adc, ref, run_pipeline(loc3, adc, 512)


def test_config5_shape(config5):
    _, ref, got = config5
    assert ref["n_trig"].sum() > 200 and ref["gate"].sum() > 100
    compare(got, ref)


def test_graph_equals_eager(loc3, config5):
    adc, ref, eager = config5
    graph = run_pipeline(loc3, adc, 512, use_graph=True)
    compare(graph, ref)
    assert_bitwise(graph, eager)


def test_persistent_loop_wraps(loc3, config5, monkeypatch):
    """Two workgroups walk up to 40 slots: records and state as the uncapped run's."""
    adc, _, eager = config5
    monkeypatch.setenv("TDOA_STREAM_PHAT_GRID", "2")
    assert_bitwise(run_pipeline(loc3, adc, 512), eager)


@pytest.mark.parametrize("use_graph", [False, True])
def test_ungated_frames(oracle, loc3, use_graph):
    lut = loc3.lut()
    adc = synth.adc_stream(8, 512 * 40, 3, lut, loc3.dims.S, 101).numpy().copy()
    adc[0] = adc[0][:, :1]  # one signal on all three mics: every lag 0
    ref = R.run(oracle, adc, 1024, FS, loc3.dims.S, loc3.window(), lut)
    n0 = ref["n_trig"][0]
    assert n0 > 0 and not ref["gate"][0, :n0].any() and not ref["lags"][0, :n0].any()
    assert ref["n_trig"].sum() == 64 and ref["gate"].sum() == 57
    got = run_pipeline(loc3, adc, 512, use_graph=use_graph)
    compare(got, ref)
    recs, est, last, _ = got
    assert all(r["cell"] == -1 and not r["gate"] for r in recs[0])
    assert not est[0].any() and last[0] == 0


@pytest.mark.parametrize("use_graph", [False, True])
def test_band_limited_and_table_read_per_step(oracle, use_graph):
    loc = _loc()
    lut, win, S = loc.lut(), loc.window(), loc.dims.S
    adc = synth.adc_stream(8, 512 * 40, 3, lut, S, 102).numpy()
    loc.set_band(1000, 6000, 500)
    pipe = StreamPipeline(loc, torch.from_numpy(adc).cuda(), hop=512, use_graph=use_graph)
    band = R.run(oracle, adc, 1024, FS, S, win, lut, w=band_ref.band_weights(1024, FS, 1000, 6000, 500))
    compare(feed(pipe, adc, 512), band)
    torch.cuda.synchronize()  # the setters want no step in flight
    loc.set_bin_weights(None)
    pipe.reset()
    plain = R.run(oracle, adc, 1024, FS, S, win, lut)
    assert not np.array_equal(plain["est"], band["est"])
    compare(feed(pipe, adc, 512), plain)
    pipe.close()
    loc.close()


# (N, hop, M, hops, seed, share of gated records whose cell may be skipped)
SHAPES = [(2048, 1024, 4, 24, 2122, 0.25),  # the TW = 2 / P = 6 solve; the reference alone skips 16.9 %
          (512, 256, 2, 24, 584, 0.0),
          (1024, 384, 3, 24, 424, 0.0),      # hop != N / 2: the LDS trigger (k_stream_trigger_lds)
          (256, 256, 3, 40, 77, 0.0),
          (1024, 512, 8, 24, 808, 0.25)]     # the largest LDS shape; 8 mics take the LDS trigger too


@pytest.mark.parametrize("N,hop,M,hops,seed,max_skip", SHAPES)
def test_other_shapes(oracle, N, hop, M, hops, seed, max_skip):
    """Six streams each.  (1024, 512, 8 mics): seed 808 of 800..811, at which
    the float64 reference alone skips 0 % of its 29 gated records (minimum map
    gap 8.8e-2) and drops no stream; over those twelve seeds it skips 0 % to
    17.9 % (28-pair maps have many near-ties), always under the 25 % cap."""
    loc = _loc(M, N)
    lut, S = loc.lut(), loc.dims.S
    adc = synth.adc_stream(6, hop * hops, M, lut, S, seed).numpy()
    ref = R.run(oracle, adc, N, FS, S, loc.window(), lut)
    assert ref["gate"].sum() > 10
    for use_graph in (False, True):
        compare(run_pipeline(loc, adc, hop, use_graph=use_graph), ref, max_skip=max_skip)
    loc.close()


@pytest.mark.parametrize("capture_len", [2048, 2049])
def test_capture_ring_wraps(oracle, loc3, capture_len):
    """A producer-fed ring; the odd length makes every stream's ring start
    unaligned (stride capture_len * 3 bytes)."""
    lut = loc3.lut()
    adc = synth.adc_stream(6, 512 * 24, 3, lut, loc3.dims.S, 23).numpy()
    ref = R.run(oracle, adc, 1024, FS, loc3.dims.S, loc3.window(), lut)
    for use_graph in (False, True):
        compare(run_pipeline(loc3, adc, 512, use_graph=use_graph, capture_len=capture_len), ref)


def test_api_contract(loc3):
    L = tdoa.load()
    cap = torch.zeros((2, 4096, 3), dtype=torch.uint8, device="cuda")
    pipe = StreamPipeline(loc3, cap, hop=512)
    assert "max_Lf" in pipe.out and "max_L" not in pipe.out
    assert pipe.out["max_Lf"].dtype == torch.float32
    assert L.tdoa_stream_step(pipe._h, C.byref(_lib.StreamOutputs()), None) == -1
    assert b"tdoa_stream_step_f" in L.tdoa_last_error()
    est = np.zeros((2, 3, loc3.dims.K), np.int64)
    assert L.tdoa_stream_state(pipe._h, None, est.ctypes.data_as(C.c_void_p), None, None) == -1
    assert pipe.totals() == (0, 0, 0)  # tdoa_stream_state without est serves both
    assert pipe.state()[1].dtype == np.float32
    pipe.close()

    direct = _loc(engine="direct")
    dp = StreamPipeline(direct, cap, hop=512)
    assert "max_L" in dp.out and "max_Lf" not in dp.out and dp.out["max_L"].dtype == torch.int64
    assert dp.state()[1].dtype == np.int64
    assert L.tdoa_stream_step_f(dp._h, C.byref(_lib.StreamOutputsF()), None) == -1
    estf = np.zeros((2, 3, direct.dims.K), np.float32)
    assert L.tdoa_stream_state_f(dp._h, None, estf.ctypes.data_as(C.c_void_p), None, None) == -1
    dp.step()
    assert dp.totals()[0] == 512
    dp.close()
    direct.close()

    big = _loc(8, 4096)
    with pytest.raises(tdoa.TdoaError) as e:
        StreamPipeline(big, torch.zeros((1, 8192, 8), dtype=torch.uint8, device="cuda"), hop=2048)
    assert e.value.code == -1
    assert "8 mics" in str(e.value) and "4096" in str(e.value)
    big.close()
