"""The tracker on the device (k_track: tdoa_track_batch, tdoa_stream_track;
Localizer.track_batch, StreamPipeline.track / track_records / tracks_all).

No tolerance anywhere: the state and every output must equal the numpy
restatement of the rule (tests/track_ref.py) and the host twin
(tdoa_track_host) byte for byte.  Outputs are pre-filled with a sentinel; what
a call must not write must still hold it.  Only the scenario test, whose chain
goes through the least-squares refinement (compared within a bound elsewhere),
checks properties instead of bytes -- the ones its CPU oracle chain shows.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import track_cases as TC  # noqa: E402
import track_ref as R  # noqa: E402
import track_scenario as SC  # noqa: E402
import tdoa  # noqa: E402
from tdoa import _lib, synth  # noqa: E402
from tdoa.localizer import Localizer  # noqa: E402
from tdoa.stream import StreamPipeline  # noqa: E402

FS = 48000
SENT = 0x5A
OUTS = ("tracks", "assigned", "num_confirmed")


def same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def loc():
    lc = Localizer(engine="direct", sample_rate_hz=FS)
    yield lc
    lc.close()


def start_state(S, T):
    """All zero, but slots >= T hold a sentinel: the rule never reads or writes them."""
    tr, nid = R.new_state(S)
    tr.view(np.uint8).reshape(S, 8, 64)[:, T:] = SENT
    return tr, nid


# (rows, S, evaluations): one row; a partial workgroup; several workgroups with
# the rows a fresh permutation of 257 of 300 streams in every call
BATCHES = [(1, 6, 60), (5, 6, 60), (257, 300, 8)]
_expected = {}


def expected(T, Kp, rows, S, evals):
    """The sequence and, per call, the reference's state and outputs; computed
    once per case and never modified.  The host twin runs alongside."""
    key = (T, Kp, rows)
    if key not in _expected:
        calls = TC.make_sequence(TC.SEEDS[0], T, Kp, S=S, rows=rows, evals=evals)
        tr, nid = start_state(S, T)
        htr, hnid = start_state(S, T)
        steps = []
        for sor, t, cnt, xy in calls:
            tr, nid, out, _ = R.track_rows(tr, nid, t, cnt, xy, stream_of_row=sor, **TC.params(T))
            ho = tdoa.track_host(htr, hnid, t, cnt, xy, stream_of_row=sor, **TC.params(T))
            assert same(tr, htr) and same(nid, hnid) and all(same(out[k], ho[k]) for k in OUTS)
            steps.append((tr.copy(), nid.copy(), out))
        _expected[key] = (calls, steps)
    return _expected[key]


@pytest.mark.parametrize("rows,S,evals", BATCHES)
@pytest.mark.parametrize("T,Kp", TC.SHAPES)
def test_batch_equals_reference_and_host(loc, T, Kp, rows, S, evals):
    calls, steps = expected(T, Kp, rows, S, evals)
    tr0, nid0 = start_state(S, T)
    d_tr = torch.from_numpy(tr0.view(np.uint8).reshape(S, 8, 64).copy()).cuda()
    d_nid = torch.from_numpy(nid0).cuda()
    outs = {"tracks": torch.empty((rows, T, 64), dtype=torch.uint8, device="cuda"),
            "assigned": torch.empty((rows, Kp), dtype=torch.int32, device="cuda"),
            "num_confirmed": torch.empty(rows, dtype=torch.int32, device="cuda")}
    # which outputs a call passes: all of them, then each alone (the others' pointers are NULL)
    subsets = [OUTS, ("tracks",), ("assigned",), ("num_confirmed",)]
    for c, ((sor, t, cnt, xy), (e_tr, e_nid, e_out)) in enumerate(zip(calls, steps)):
        for v in outs.values():
            v.view(torch.uint8).fill_(SENT)
        use = subsets[c % 4]
        got = loc.track_batch(d_tr, d_nid, torch.from_numpy(t).cuda(), torch.from_numpy(cnt).cuda(),
                              torch.from_numpy(xy).cuda(), stream_of_row=torch.from_numpy(sor).cuda(),
                              outputs={k: outs[k] for k in use}, **TC.params(T))
        assert set(got) == set(use)
        torch.cuda.synchronize()
        assert d_tr.cpu().numpy().tobytes() == e_tr.tobytes(), f"state differs after call {c}"
        assert same(d_nid.cpu().numpy(), e_nid), f"next_id differs after call {c}"
        for k in OUTS:
            g = outs[k].cpu().numpy()
            if k in use:
                assert g.tobytes() == e_out[k].tobytes(), f"{k} differs in call {c}"
            else:
                assert (g.view(np.uint8) == SENT).all(), f"{k} written in call {c} without being passed"
    assert steps[-1][1].max() > 1


def test_batch_without_stream_of_row_and_with_zero_rows(loc):
    T, Kp, S = 4, 3, 7
    calls = TC.make_sequence(5, T, Kp, S=S, rows=S, evals=10)
    tr, nid = R.new_state(S)
    d_tr = torch.zeros((S, 8, 64), dtype=torch.uint8, device="cuda")
    d_nid = torch.zeros(S, dtype=torch.int32, device="cuda")
    for sor, t, cnt, xy in calls:  # row i is stream i: the sequence's streams are ignored
        tr, nid, out, _ = R.track_rows(tr, nid, t, cnt, xy, **TC.params(T))
        got = loc.track_batch(d_tr, d_nid, torch.from_numpy(t).cuda(), torch.from_numpy(cnt).cuda(),
                              torch.from_numpy(xy).cuda(), **TC.params(T))
        torch.cuda.synchronize()
        assert d_tr.cpu().numpy().tobytes() == tr.tobytes() and same(d_nid.cpu().numpy(), nid)
        assert all(got[k].cpu().numpy().tobytes() == out[k].tobytes() for k in OUTS)
    # rows = 0 through the C entry point: TDOA_OK, nothing launched, nothing written
    before = d_tr.clone()
    prm = _lib.track_params(**TC.params(T))
    o = _lib.TrackOutputs(None, d_nid.data_ptr(), None)
    p = lambda x: C.c_void_p(x.data_ptr())
    assert _lib.load().tdoa_track_batch(0, p(d_tr), p(d_nid), 0, None, p(d_nid), p(d_nid), p(d_tr), Kp,
                                        C.byref(prm), C.byref(o), None) == 0
    torch.cuda.synchronize()
    assert torch.equal(before, d_tr) and same(d_nid.cpu().numpy(), nid)


# ---------------------------------------------------------------- the streaming form
def _adc(lc, S, T, seed, quiet=(), **kw):
    adc = synth.adc_stream(S, T, lc.dims.M, lc.lut(), lc.dims.S, seed, **kw).numpy()
    for s in quiet:
        adc[s] = 128  # never triggers
    return adc


def _fill(pipe, tensors):
    with torch.cuda.stream(pipe.stream):
        for t in tensors.values():
            t.view(torch.uint8).fill_(SENT)


def _check_hop(pipe, o, count, xy, tr, nid, prm, where):
    """Synchronise; rows < the step's count and the whole state against the
    reference fed this hop's own count / xy / end / stream_id; rows >= count
    must hold the sentinel.  Returns the new reference state and the slots."""
    pipe.stream.synchronize()
    n = int(pipe.out["count"].item())
    ids = pipe.out["stream_id"][:n].cpu().numpy()
    end = pipe.out["end"][:n].cpu().numpy()
    t_us = (end.astype(np.uint64) * np.uint64(1000000) // np.uint64(FS)).astype(np.int64)
    assert len(set(ids.tolist())) == n
    tr, nid, exp, _ = R.track_rows(tr, nid, t_us, count.cpu().numpy()[:n], xy.cpu().numpy()[:n], stream_of_row=ids,
                                   **prm)
    for k in OUTS:
        g = o[k].cpu().numpy()
        assert g[:n].tobytes() == exp[k].tobytes(), (where, k)
        assert (g[n:].view(np.uint8) == SENT).all(), (where, k, "rows >= count written")
    g_tr, g_nid = pipe.tracks_all()
    assert same(g_tr, tr) and same(g_nid, nid), (where, "state")
    return tr, nid, n, ids


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("engine", ["direct", "gcc_phat"])
def test_stream_track_equals_reference(engine, use_graph):
    lc = Localizer(engine=engine, sample_rate_hz=FS)
    S, hops = 64, 12
    adc = _adc(lc, S, 512 * hops, 29, quiet=(0, 1, 17, 40), burst_len=500, gap=(1100, 1600))
    adc[5, :, 1] = adc[5, :, 0]  # one signal on all mics: lags 0, triggers but is never gated
    adc[5, :, 2] = adc[5, :, 0]
    pipe = StreamPipeline(lc, torch.from_numpy(adc).cuda(), hop=512, use_graph=use_graph)
    prm = dict(R.DEFAULTS, max_tracks=4, confirm_hits=2, max_misses=2)
    tr, nid = R.new_state(S)
    # before any step: nothing is launched, whatever the measurements
    cnt0 = torch.ones(S, dtype=torch.int32, device="cuda")
    xy0 = torch.zeros((S, 3, 2), dtype=torch.float32, device="cuda")
    o = pipe.track(peaks={"count": cnt0, "xy": xy0}, **prm)
    assert o["tracks"].shape == (S, 4, 64) and o["assigned"].shape == (S, 3) and o["num_confirmed"].shape == (S,)
    _fill(pipe, o)
    assert pipe.track(peaks={"count": cnt0, "xy": xy0}, **prm) is o
    pipe.stream.synchronize()
    assert all((v.cpu().numpy().view(np.uint8) == SENT).all() for v in o.values())
    g_tr, g_nid = pipe.tracks_all()
    assert same(g_tr, tr) and same(g_nid, nid)
    listed = ungated = evaluated = 0
    for h in range(hops):
        pipe.step()
        pk = pipe.peaks(num_peaks=3, ls=True)
        _fill(pipe, o)
        assert pipe.track(**prm) is o  # the last peaks() result, xy_ls
        before = tr
        tr, nid, n, ids = _check_hop(pipe, o, pk["count"], pk["xy_ls"], tr, nid, prm, (engine, use_graph, h))
        gate = pipe.out["gate"][:n].cpu().numpy()
        cnt = pk["count"][:n].cpu().numpy()
        assert ((cnt == 0) == (gate == 0)).all()  # gated_only peaks: an ungated slot has no peak
        off = ids[gate == 0]
        assert same(before[off], tr[off])  # ... and its stream's state is untouched
        listed, ungated, evaluated = listed + n, ungated + len(off), evaluated + int((cnt > 0).sum())
    assert listed >= 100 and evaluated >= 60 and ungated >= 1, (listed, evaluated, ungated)
    assert (tr[[0, 1, 17, 40]]["id"] == 0).all() and (tr["status"] == 2).any() and nid.max() >= 2
    r = pipe.track_records()  # the last hop, sorted by stream
    assert list(r["stream_id"]) == sorted(r["stream_id"]) and r["tracks"].dtype == tdoa.TRACK_DTYPE
    assert same(r["tracks"], tr[r["stream_id"], :4])
    # reset: no tracks, ids from 1 again; nothing is launched until the next step
    pipe.reset()
    _fill(pipe, o)
    pipe.track(**prm)
    pipe.stream.synchronize()
    assert all((v.cpu().numpy().view(np.uint8) == SENT).all() for v in o.values())
    tr, nid = R.new_state(S)
    g_tr, g_nid = pipe.tracks_all()
    assert same(g_tr, tr) and same(g_nid, nid)
    # step -> track with measurements of the caller's: no peaks() call involved
    rng = np.random.default_rng(3)
    born = 0
    o2 = pipe.track(peaks={"count": cnt0[:S], "xy": xy0[:, :2].contiguous()}, **prm)  # no step yet: only allocates
    assert o2 is not o and o2["assigned"].shape == (S, 2)
    for h in range(4):
        pipe.step()
        cnt = torch.from_numpy(rng.integers(0, 4, S).astype(np.int32)).cuda()
        xy = torch.from_numpy(rng.uniform(-1, 1, (S, 2, 2)).astype(np.float32)).cuda()  # Kp = 2 < some counts
        _fill(pipe, o2)
        pipe.stream.wait_stream(torch.cuda.current_stream())  # the uploads precede the kernel
        assert pipe.track(peaks={"count": cnt, "xy": xy}, **prm) is o2
        tr, nid, n, _ = _check_hop(pipe, o2, cnt, xy, tr, nid, prm, (engine, use_graph, "own", h))
        born += n
    assert born >= 10 and nid.max() >= 1 and set(tr["id"][tr["id"] != 0].tolist()) <= set(range(1, int(nid.max()) + 1))
    pipe.close()
    lc.close()


def test_stream_track_errors_leave_outputs_untouched():
    lc = Localizer(engine="gcc_phat", sample_rate_hz=FS)
    adc = _adc(lc, 4, 512 * 4, 23)
    pipe = StreamPipeline(lc, torch.from_numpy(adc).cuda(), hop=512)
    pipe.step()
    cnt = torch.ones(4, dtype=torch.int32, device="cuda")
    xy = torch.zeros((4, 2, 2), dtype=torch.float32, device="cuda")
    o = pipe.track(peaks={"count": cnt, "xy": xy})
    _fill(pipe, o)
    pipe.stream.synchronize()
    state = pipe.tracks_all()
    for bad in (dict(max_tracks=0), dict(gate_d2=float("nan")), dict(meas_var=0.0), dict(max_coast_us=0)):
        with pytest.raises(tdoa.TdoaError, match="tdoa_stream_track"):
            pipe.track(peaks={"count": cnt, "xy": xy}, **bad)
    L, prm = _lib.load(), _lib.track_params()
    none = _lib.TrackOutputs()
    st = C.c_void_p(pipe.stream.cuda_stream)
    assert L.tdoa_stream_track(pipe._h, C.byref(prm), C.c_void_p(cnt.data_ptr()), C.c_void_p(xy.data_ptr()), 2,
                               C.byref(none), st) == -1
    assert b"output" in L.tdoa_last_error()
    full = _lib.TrackOutputs(*[o[k].data_ptr() for k in OUTS])
    assert L.tdoa_stream_track(pipe._h, C.byref(prm), C.c_void_p(cnt.data_ptr()), C.c_void_p(xy.data_ptr()), 9,
                               C.byref(full), st) == -1
    assert b"Kp" in L.tdoa_last_error()
    pipe.stream.synchronize()
    assert all((v.cpu().numpy().view(np.uint8) == SENT).all() for v in o.values())
    after = pipe.tracks_all()
    assert same(state[0], after[0]) and same(state[1], after[1])
    pipe.close()
    lc.close()


def test_scenario_one_fixed_source_per_stream(oracle):
    """tests/track_scenario.py through the DIRECT pipeline: what its CPU oracle
    chain shows, the device must show -- from its confirmation on exactly one
    confirmed track per stream, the same id, assigned at every gated hop -- and
    the tables end with the chain's ids, statuses and hit counts."""
    adc, lut, win, mics = SC.capture(oracle)
    want, e_tr, e_nid = SC.oracle_tracks(SC.oracle_hops(oracle, adc, lut, win, mics))
    want.done()
    lc = Localizer(engine="direct", sample_rate_hz=SC.FS)
    assert lc.dims.S == SC.MAX_SHIFT and (lc.lut() == lut).all() and (lc.mics() == mics).all()
    pipe = StreamPipeline(lc, torch.from_numpy(adc).cuda(), hop=SC.HOP)
    got = SC.Follow()
    for h in range(SC.HOPS):
        pipe.step()
        pipe.peaks(num_peaks=SC.KP, radius=SC.RADIUS, min_rel=SC.MIN_REL, ls=True)
        pipe.track(**SC.PRM)
        r = pipe.track_records()
        n = len(r["stream_id"])
        gate = pipe.out["gate"][:n].cpu().numpy()[np.argsort(pipe.out["stream_id"][:n].cpu().numpy(), kind="stable")]
        got.hop(r["stream_id"], gate, r["tracks"], r["assigned"], ("device", h))
    got.done()
    assert got.conf_id == want.conf_id and got.gated_after == want.gated_after
    tr, nid = pipe.tracks_all()
    assert (nid == e_nid).all()
    for f in ("id", "status", "hits", "misses", "peak", "t_us", "upd_us"):
        assert (tr[f] == e_tr[f]).all(), f
    pipe.close()
    lc.close()
