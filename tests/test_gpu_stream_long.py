"""Streaming GCC_PHAT at the long-frame shapes, 8 mics x 2048 and 4 mics x 4096
(selector -> k_f16_ring -> k_stream_ema_grid), against the float64 references
of tests/stream_phat_ref.py, tests/stream16_ref.py and tests/stream_cont_ref.py
on the cases of tests/stream_long_cases.py.

Comparison rules: those of tests/test_gpu_stream_phat.py, restated here (feed,
compare, assert_bitwise) with its tolerances (stream_phat_ref.TOL_*): end,
stream_id, count and totals() exact; lags and gate exact; ema_best exact where
the EMA row's margin exceeds TOL_LAG_MARGIN; cell and xy exact; max_Lf within
TOL_MAXL; est within TOL_EST; last exact.  tests/test_stream_long_cpu.py shows
on the references alone that no stream is dropped and no cell is skipped at
these seeds, so every comparison runs with max_dropped = 0 and max_skip = 0.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import band_ref  # noqa: E402
import stream16_ref  # noqa: E402
import stream_cont_ref  # noqa: E402
import stream_long_cases as Cs  # noqa: E402
import stream_phat_ref as R  # noqa: E402
import tdoa  # noqa: E402
import track_ref  # noqa: E402
from tdoa.localizer import Localizer  # noqa: E402
from tdoa.stream import StreamPipeline  # noqa: E402
from test_gpu_stream_peaks import _check_rows, _fill as _fill_peaks  # noqa: E402
from test_gpu_track import _check_hop, _fill as _fill_tracks  # noqa: E402

FS = Cs.FS
TRIG = [(fmt, *c) for fmt in Cs.FMTS for c in Cs.TRIGGERED]
CONT = [(fmt, *c) for fmt in Cs.FMTS for c in Cs.CONTINUOUS[fmt]]


def _loc(M, N, fmt="adc8"):
    loc = Localizer(engine="gcc_phat", num_mics=M, frame_len=N, sample_rate_hz=FS, mic_xy=Cs.MICS[M],
                    sample_format=fmt)
    assert loc.dims.S == Cs.S_LAG
    return loc


# ---- feed / compare / assert_bitwise of tests/test_gpu_stream_phat.py, restated
def feed(pipe, cap, hop, capture_len=None, src=None):
    """Every full hop through `pipe`; per-stream record lists, state, totals."""
    S, T, _ = cap.shape
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


def compare(got, ref, max_dropped=0, max_skip=0.0):
    recs, est, last, totals = got
    assert est.dtype == np.float32
    n_trig = ref["n_trig"]
    first = R.dropped_streams(ref)
    dropped = int((first < n_trig).sum())
    gated = skipped = 0
    worst_est = worst_L = 0.0
    for s, lst in recs.items():
        assert len(lst) == n_trig[s], (s, len(lst), n_trig[s])  # the selector does not depend on the engine
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
    assert gated >= Cs.MIN_GATED
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


def make_pipe(loc, cap, hop, use_graph=False, capture_len=None, activity_var=None):
    """(pipeline, producer source or None): the whole capture as the ring, or a
    producer-fed ring of capture_len samples (+ 4 spare bytes behind a uint8 one,
    as the triggered tests keep them: its trigger may read word-wise)."""
    S, _, M = cap.shape
    src = None
    if capture_len is None:
        ring = torch.from_numpy(cap).cuda()
    else:
        dt = torch.from_numpy(cap[:0]).dtype
        flat = torch.zeros(S * capture_len * M + (4 if dt == torch.uint8 else 0), dtype=dt, device="cuda")
        ring = flat[:S * capture_len * M].view(S, capture_len, M)
        src = torch.from_numpy(cap).cuda()
    kw = {} if activity_var is None else dict(mode="continuous", activity_var=activity_var)
    pipe = StreamPipeline(loc, ring, hop=hop, use_graph=use_graph, **kw)
    assert pipe.kernel == "k_f16_ring"
    return pipe, src


def run_pipeline(loc, cap, hop, use_graph=False, capture_len=None, activity_var=None):
    pipe, src = make_pipe(loc, cap, hop, use_graph, capture_len, activity_var)
    got = feed(pipe, cap, hop, capture_len, src)
    pipe.close()
    return got


# ---- the cases' captures, references and eager runs: computed once, shared, not modified
_cache = {}


def trig_case(oracle, fmt, N, hop, M, hops, seed, band=None):
    key = ("trig", fmt, N, M, seed, band)
    if key not in _cache:
        loc = _loc(M, N, fmt)
        lut, win = loc.lut(), loc.window()
        cap = Cs.triggered_capture(fmt, lut, N, hop, M, hops, seed)
        w = None if band is None else band_ref.band_weights(N, FS, *band)
        if fmt == "pcm16":
            ref = stream16_ref.run(oracle, cap, N, FS, loc.dims.S, win, lut, w=w, hop=hop)
        else:
            ref = R.run(oracle, cap, N, FS, loc.dims.S, win, lut, w=w)
        eager = None if band is not None else run_pipeline(loc, cap, hop)
        loc.close()
        _cache[key] = cap, ref, eager
    return _cache[key]


def cont_case(oracle, fmt, N, hop, M, hops, seed, var):
    key = ("cont", fmt, N, M, seed, var)
    if key not in _cache:
        loc = _loc(M, N, fmt)
        lut = loc.lut()
        cap = Cs.continuous_capture(fmt, lut, N, hop, M, hops, seed)
        ref = stream_cont_ref.run(oracle, cap, N, FS, loc.dims.S, loc.window(), lut, hop, var)
        eager = run_pipeline(loc, cap, hop, activity_var=var)
        loc.close()
        _cache[key] = cap, ref, eager
    return _cache[key]


# ---- creation
def test_creation_and_kernel_names():
    """Both long-frame shapes in all three creators run k_f16_ring; what fits
    k_stream_phat stays there; 8 x 4096 is refused as before."""
    for M, N, hop in ((8, 2048, 1024), (4, 4096, 2048)):
        for fmt, dt in (("adc8", torch.uint8), ("pcm16", torch.int16)):
            loc = _loc(M, N, fmt)
            ring = torch.zeros((2, N + 2 * hop, M), dtype=dt, device="cuda")
            for kw in ({}, dict(mode="continuous"), dict(use_graph=True)):
                pipe = StreamPipeline(loc, ring, hop=hop, **kw)
                assert pipe.kernel == "k_f16_ring", (M, N, fmt, kw)
                pipe.step()
                pipe.stream.synchronize()
                assert pipe.totals()[0] == hop
                pipe.close()
            loc.close()
    small = Localizer(engine="gcc_phat", sample_rate_hz=FS)
    pipe = StreamPipeline(small, torch.zeros((2, 4096, 3), dtype=torch.uint8, device="cuda"), hop=512)
    assert pipe.kernel == "k_stream_phat"
    pipe.close()
    small.close()
    for M, N in ((4, 2048), (3, 4096)):  # the product's routing of what fits does not change
        loc = _loc(M, N) if M == 4 else Localizer(engine="gcc_phat", num_mics=3, frame_len=N, sample_rate_hz=FS)
        pipe = StreamPipeline(loc, torch.zeros((1, 2 * N, M), dtype=torch.uint8, device="cuda"), hop=N // 2)
        assert pipe.kernel == "k_stream_phat", (M, N)
        pipe.close()
        loc.close()
    big = _loc(8, 4096)
    for kw in ({}, dict(mode="continuous")):
        with pytest.raises(tdoa.TdoaError) as e:
            StreamPipeline(big, torch.zeros((1, 8192, 8), dtype=torch.uint8, device="cuda"), hop=2048, **kw)
        assert e.value.code == -1
        assert "8 mics" in str(e.value) and "4096" in str(e.value)
    big.close()


# ---- references
@pytest.mark.parametrize("fmt,N,hop,M,hops,seed", TRIG)
def test_triggered_cases(oracle, monkeypatch, fmt, N, hop, M, hops, seed):
    """Eager and graph-captured against the reference; the graph's records and
    state are the eager run's bit for bit, and so are those of two workgroups
    walking the list in both kernels (TDOA_STREAM_PHAT_GRID=2)."""
    cap, ref, eager = trig_case(oracle, fmt, N, hop, M, hops, seed)
    compare(eager, ref)
    loc = _loc(M, N, fmt)
    graph = run_pipeline(loc, cap, hop, use_graph=True)
    compare(graph, ref)
    assert_bitwise(graph, eager)
    monkeypatch.setenv("TDOA_STREAM_PHAT_GRID", "2")
    assert_bitwise(run_pipeline(loc, cap, hop), eager)
    loc.close()


@pytest.mark.parametrize("fmt,N,hop,M,hops,seed,var", CONT)
def test_continuous_cases(oracle, fmt, N, hop, M, hops, seed, var):
    cap, ref, eager = cont_case(oracle, fmt, N, hop, M, hops, seed, var)
    compare(eager, ref)
    loc = _loc(M, N, fmt)
    graph = run_pipeline(loc, cap, hop, use_graph=True, activity_var=var)
    compare(graph, ref)
    assert_bitwise(graph, eager)
    loc.close()


@pytest.mark.parametrize("N,hop,M,hops,seed", Cs.TRIGGERED)
def test_band_limited_and_table_read_per_step(oracle, N, hop, M, hops, seed):
    """Triggered uint8 under the band table, eager and graph (bitwise equal);
    then, on the eager pipeline, the table cleared and the state reset: the
    plain reference.  The step picks the kernel's instantiation from the table."""
    cap, band, _ = trig_case(oracle, "adc8", N, hop, M, hops, seed, band=Cs.BAND)
    _, plain, _ = trig_case(oracle, "adc8", N, hop, M, hops, seed)
    assert not np.array_equal(plain["est"], band["est"])
    loc = _loc(M, N)
    loc.set_band(*Cs.BAND)
    graph = run_pipeline(loc, cap, hop, use_graph=True)
    compare(graph, band)
    pipe, _ = make_pipe(loc, cap, hop)
    first = feed(pipe, cap, hop)
    compare(first, band)
    assert_bitwise(graph, first)
    torch.cuda.synchronize()  # the setters want no step in flight
    loc.set_bin_weights(None)
    pipe.reset()
    compare(feed(pipe, cap, hop), plain)
    pipe.close()
    loc.close()


# ---- the batch engine's kernel on the same frames
@pytest.mark.parametrize("fmt,N,hop,M,hops,seed", TRIG)
def test_batch_equality(oracle, fmt, N, hop, M, hops, seed):
    """Every record's lags and gate equal Localizer.localize of the same frame
    cut from the capture; and after the hop that holds a stream's first gated
    frame (the capture ends with it for that stream's state: no earlier update),
    est == float32(batch weighted_f) * float32(decay), bit for bit (zeros
    compared without their sign)."""
    cap, ref, eager = trig_case(oracle, fmt, N, hop, M, hops, seed)
    recs = eager[0]
    idx = [(s, i) for s in recs for i in range(len(recs[s]))]
    frames = np.stack([np.ascontiguousarray(cap[s, int(recs[s][i]["end"]) - N:int(recs[s][i]["end"])].T).astype(np.int16)
                       for s, i in idx])
    loc = _loc(M, N, fmt)
    assert loc.batch_kernel() == ("k_f16_pcm16" if fmt == "pcm16" else "k_frame16")
    out = {k: v.cpu().numpy() for k, v in loc.localize(torch.from_numpy(frames).cuda(), scores=True).items()}
    for b, (s, i) in enumerate(idx):
        assert (recs[s][i]["lags"] == out["lags"][b]).all(), (s, i)
        assert recs[s][i]["gate"] == out["gate"][b], (s, i)
    # the first gated frame of every stream: the state right after its hop
    first = {}
    for b, (s, i) in enumerate(idx):
        if out["gate"][b] and s not in first:
            first[s] = (b, int(recs[s][i]["end"]))
    assert len(first) == cap.shape[0]
    pipe, _ = make_pipe(loc, cap, hop)
    worst, checked = 0.0, 0
    for h in range(cap.shape[1] // hop):
        pipe.step()
        due = [s for s, (_, e) in first.items() if h * hop < e <= (h + 1) * hop]
        if not due:
            continue
        est = pipe.state()[1]
        for s in due:
            b, e = first[s]
            dec = np.float32(tdoa.decay_us(e * 1000000 // FS, 0))
            # the first EMA step from est = +0, in float32.  A zero's sign is
            # the step's own (+0 + (-0) = +0, a fused step keeps an underflowed
            # -0), not the kernels': -0 and +0 compare as one value, x + 0
            want = out["weighted_f"][b] * dec + np.float32(0.0)
            assert want.dtype == np.float32
            got_s = est[s] + np.float32(0.0)
            worst = max(worst, float(np.abs(got_s - want).max()))
            bad = np.argwhere(got_s.view(np.uint32) != want.view(np.uint32))
            assert not bad.size, (s, worst, len(bad), [(tuple(i), est[s][tuple(i)], want[tuple(i)],
                                                         out["weighted_f"][b][tuple(i)]) for i in bad[:6]])
            checked += 1
    print(f"{checked} first gated frames, max |est - batch weighted_f * decay| {worst:.2e}")
    assert checked == cap.shape[0]
    pipe.close()
    loc.close()


# ---- rings
@pytest.mark.parametrize("fmt", Cs.FMTS)
def test_capture_ring_wraps_unaligned(oracle, fmt):
    """8 x 2048 on a producer-fed ring of N + 2 hop + 1 samples: the odd length
    makes every stream's ring start unaligned and the frames wrap anywhere.
    Records and state are the whole-capture run's bit for bit."""
    N, hop, M, hops, seed = Cs.TRIGGERED[0]
    cap, ref, eager = trig_case(oracle, fmt, N, hop, M, hops, seed)
    loc = _loc(M, N, fmt)
    got = run_pipeline(loc, cap, hop, capture_len=N + 2 * hop + 1)
    compare(got, ref)
    assert_bitwise(got, eager)
    loc.close()


# ---- end to end
def test_step_peaks_track_8x2048(oracle):
    """step -> peaks(num_peaks = 2, refined) -> track over the triggered uint8
    case: the peaks equal peaks_ref on the pipeline's own est, the tracks
    track_ref on those peaks (the helpers of the stream-peaks and track tests)."""
    N, hop, M, hops, seed = Cs.TRIGGERED[0]
    cap, _, _ = trig_case(oracle, "adc8", N, hop, M, hops, seed)
    loc = _loc(M, N)
    lut = loc.lut()
    pipe, _ = make_pipe(loc, cap, hop)
    prm = dict(track_ref.DEFAULTS, max_tracks=4, confirm_hits=2, max_misses=2)
    tr, nid = track_ref.new_state(pipe.S)
    pk = pipe.peaks(num_peaks=2, ls=True)  # no step yet: only allocates
    o = pipe.track(**prm)
    listed = evaluated = 0
    for h in range(hops):
        pipe.step()
        _fill_peaks(pipe, pk)
        assert pipe.peaks(num_peaks=2, ls=True) is pk
        _fill_tracks(pipe, o)
        assert pipe.track(**prm) is o  # the last peaks() result, xy_ls
        n, ids, gate, est = _check_rows(pipe, pk, lut, 2, 8, gated_only=True, where=("long", h))
        tr, nid, n2, _ = _check_hop(pipe, o, pk["count"], pk["xy_ls"], tr, nid, prm, ("long", h))
        assert n2 == n
        cnt = pk["count"][:n].cpu().numpy()
        assert ((cnt == 0) == (gate == 0)).all()
        xy_ls = pk["xy_ls"][:n].cpu().numpy()
        assert np.isfinite(xy_ls[cnt > 0, 0]).all()
        listed, evaluated = listed + n, evaluated + int((cnt > 0).sum())
    assert listed >= 30 and evaluated >= Cs.MIN_GATED, (listed, evaluated)
    assert (tr["status"] == 2).any() and nid.max() >= 1
    pipe.close()
    loc.close()
