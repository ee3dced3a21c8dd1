"""Peaks and least-squares refinement of the streaming EMA map per hop
(tdoa_stream_peaks: k_stream_peaks / k_ls_stream; StreamPipeline.peaks,
peak_records, peaks_all, est_ptr).

The expected value needs no tolerance: after a step and peaks() the state is
read back (state()) and row i of every output must equal tests/peaks_ref.py on
the single block est[stream_id[i]], bit for bit.  Outputs are pre-filled with a
sentinel; rows >= the step's count must still hold it.  Only the refinement is
compared within a bound: the xy_ls rule of tests/test_gpu_peaks.py (_check_ls,
1e-5 relative) against oracle.ls_refine on the state snapshot.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import peaks_ref as R  # noqa: E402
from tdoa import _lib, synth  # noqa: E402
from tdoa.localizer import Localizer  # noqa: E402
from tdoa.stream import StreamPipeline  # noqa: E402
from test_gpu_peaks import _check_ls  # noqa: E402

FS = 48000
SENT = -7
FIELDS = {"count": torch.int32, "cell": torch.int32, "xy": torch.float32, "lags": torch.int32,
          "xy_ls": torch.float32, "ls_rms": torch.float32}


def _ref_args(loc):
    return (loc.grid_W, loc.grid_half_w, loc.grid_half_h, loc.grid_scale, loc.dims.S)


def _loc(engine, **cfg):
    return Localizer(engine=engine, sample_rate_hz=FS, **cfg)


def _fill(pipe, tensors):
    """The sentinel into every output, ordered before the pipeline's next kernels."""
    with torch.cuda.stream(pipe.stream):
        for t in tensors.values():
            t.fill_(SENT)


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _outs(pipe, Kp, ls=False, lags=True):
    """A sentinel-filled output set of its own (the raw entry point's)."""
    S, P, phat = pipe.S, pipe.loc.dims.P, pipe.phat
    shapes = {"count": (S,), "cell": (S, Kp), "xy": (S, Kp, 2), "lags": (S, Kp, P)}
    if ls:
        shapes.update({"xy_ls": (S, Kp, 2), "ls_rms": (S, Kp)})
    if not lags:
        del shapes["lags"]
    o = {k: torch.full(s, SENT, dtype=FIELDS[k], device="cuda") for k, s in shapes.items()}
    o["Lf" if phat else "L"] = torch.full((S, Kp), SENT, dtype=torch.float32 if phat else torch.int64, device="cuda")
    torch.cuda.synchronize()
    return o


def _raw(pipe, o, Kp, radius=8, min_rel=0.0, gate=None, st=True, prm=True, out=True):
    """tdoa_stream_peaks through ctypes with exactly the tensors of `o`."""
    p = _lib.PeaksParams(Kp, radius, min_rel)
    s = _lib.PeaksOutputs()
    for k, t in o.items():
        setattr(s, k, t.data_ptr())
    return _lib.load().tdoa_stream_peaks(pipe._h if st else None, C.byref(p) if prm else None,
                                         None if gate is None else C.c_void_p(gate.data_ptr()),
                                         C.byref(s) if out else None, C.c_void_p(pipe.stream.cuda_stream))


def _empty(exp):
    """The empty record in the shape of a one-frame peaks_ref result."""
    e = {k: np.zeros_like(v) for k, v in exp.items()}
    e["cell"][:] = -1
    e["xy"][:] = np.nan
    if "L" in e:
        e["L"][:] = R.INT64_MIN
    else:
        e["Lf"][:] = -np.inf
    return e


def _check_rows(pipe, got, lut, Kp, radius, min_rel=0.0, gated_only=False, where=""):
    """Synchronise, then every row < count against peaks_ref on the state
    snapshot (the empty record where gated_only and the slot is not gated) and
    the sentinel in every row >= count.  Returns (count, stream_id, gate, est)."""
    loc = pipe.loc
    pipe.stream.synchronize()
    n = int(pipe.out["count"].item())
    ids = pipe.out["stream_id"][:n].cpu().numpy()
    gate = pipe.out["gate"][:n].cpu().numpy()
    est = pipe.state()[1]
    g = _np(got)
    assert len(set(ids.tolist())) == n and ((0 <= ids) & (ids < pipe.S)).all()
    for i in range(n):
        exp = R.peaks_ref(est[ids[i]][None], lut, *_ref_args(loc), Kp, radius, min_rel)
        if gated_only and not gate[i]:
            exp = _empty(exp)
        row = {k: g[k][i:i + 1] for k in exp}
        R.assert_equal(row, exp, (where, i, int(ids[i])))
    for k, v in g.items():
        assert (v[n:] == SENT).all(), (where, k, "rows >= count written")
    return n, ids, gate, est


def _adc(loc, S, T, seed, quiet=(), **kw):
    adc = synth.adc_stream(S, T, loc.dims.M, loc.lut(), loc.dims.S, seed, **kw).numpy()
    for s in quiet:
        adc[s] = 128  # never triggers
    return adc


def _run_hops(pipe, lut, hops, Kp, radius, gated_only=False, ls=False, where="", after=None):
    """step + peaks() for `hops` hops, each checked; the per-hop (count, ids, gate, est, got).
    after(n, got): called once the hop is checked, before the next step."""
    o = pipe.peaks(Kp, radius, ls=ls, gated_only=gated_only)  # no step yet: nothing launched
    seen = []
    for h in range(hops):
        pipe.step()
        _fill(pipe, o)
        assert pipe.peaks(Kp, radius, ls=ls, gated_only=gated_only) is o
        n, ids, gate, est = _check_rows(pipe, o, lut, Kp, radius, gated_only=gated_only, where=(where, h))
        seen.append((n, ids, gate, est, _np(o)))
        if after:
            after(n, seen[-1][4])
    return seen


def test_indirection_and_device_count_float():
    """GCC_PHAT 3 x 1024, hop 512: streams 0 and 1 never trigger, so whenever a
    frame is listed slot != stream; gate = NULL."""
    loc = _loc("gcc_phat")
    lut = loc.lut()
    S = 6
    adc = _adc(loc, S, 512 * 12, 23, quiet=(0, 1))
    pipe = StreamPipeline(loc, torch.from_numpy(adc).cuda(), hop=512)
    o = pipe.peaks(3, 8, gated_only=False)
    torch.cuda.synchronize()
    assert all((t == 0).all() for t in o.values())  # no step yet: nothing written
    seen = _run_hops(pipe, lut, 12, 3, 8, where="phat3")
    counts = [n for n, *_ in seen]
    assert any(0 < n < S for n in counts) and 0 in counts, counts
    for n, ids, *_ in seen:
        assert n == 0 or ids.min() >= 2  # slot 0's stream is not stream 0
    r = pipe.peak_records()  # the last hop, sorted by stream
    assert list(r["stream_id"]) == sorted(r["stream_id"]) and r["cell"].shape == (seen[-1][0], 3)
    pipe.close()
    loc.close()


def test_int64_direct_3x1024():
    loc = _loc("direct")
    adc = _adc(loc, 6, 512 * 12, 23, quiet=(0, 1))
    pipe = StreamPipeline(loc, torch.from_numpy(adc).cuda(), hop=512)
    seen = _run_hops(pipe, loc.lut(), 12, 3, 8, where="direct3")
    assert any(0 < n < 6 for n, *_ in seen)
    assert any(g["L"][:n].max() > 0 for n, _, _, _, g in seen if n)
    pipe.close()
    loc.close()


def test_int64_second_route_clipped_squares():
    """DIRECT 4 mics x 256, hop 100, max_shift 20 (the LDS trigger, k_direct ->
    k_stream_update) on a 15 x 9 grid with Kp = 8, radius 3: squares clipped at
    the border, and the search ends with count < Kp because no cell remains."""
    loc = _loc("direct", num_mics=4, frame_len=256, max_shift=20, mic_xy=synth.square_mics(0.15),
               grid_half_w=7, grid_half_h=4)
    assert loc.dims.G == 15 * 9
    adc = _adc(loc, 6, 100 * 12, 31, burst_len=150, gap=(200, 400))
    pipe = StreamPipeline(loc, torch.from_numpy(adc).cuda(), hop=100)
    seen = _run_hops(pipe, loc.lut(), 12, 8, 3, where="direct4")
    assert sum(n for n, *_ in seen) >= 6
    short = [g["count"][:n] for n, _, _, _, g in seen if n]
    assert any(((c >= 1) & (c < 8)).any() for c in short), short
    pipe.close()
    loc.close()


def test_continuous_pcm16_gate():
    """Continuous mode on an int16 ring at activity_var = 0: every stream is
    listed from the first full frame.  Stream 0 carries one signal on all mics
    (lags 0: never gated), the others bursts from off-centre cells."""
    loc = _loc("gcc_phat", sample_format="pcm16")
    lut = loc.lut()
    S = 5
    cap = synth.pcm16_stream(S, 512 * 10, 3, lut, loc.dims.S, 77).numpy()
    cap[0, :, 1] = cap[0, :, 0]
    cap[0, :, 2] = cap[0, :, 0]
    mixed = 0
    for gated_only in (True, False):
        pipe = StreamPipeline(loc, torch.from_numpy(cap).cuda(), hop=512, mode="continuous", activity_var=0)
        seen = _run_hops(pipe, lut, 10, 2, 8, gated_only=gated_only, where=("cont", gated_only))
        assert [n for n, *_ in seen] == [0] + [S] * 9
        for n, ids, gate, est, g in seen:
            if n and gate.any() and not gate.all():
                mixed += 1
                off = gate == 0
                if gated_only:
                    assert (g["count"][:n][off] == 0).all() and (g["cell"][:n][off] == -1).all()
                else:
                    assert (g["count"][:n][off] >= 1).all() and (g["cell"][:n][off, 0] >= 0).all()
                assert (g["count"][:n][~off] >= 1).all()
        pipe.close()
    assert mixed >= 2  # the premise, in both runs: a hop with gated and ungated slots
    loc.close()


@pytest.mark.parametrize("engine", ["direct", "gcc_phat"])
def test_one_peak_is_the_steps_own_solve(engine):
    loc = _loc(engine)
    adc = _adc(loc, 6, 512 * 12, 23)
    pipe = StreamPipeline(loc, torch.from_numpy(adc).cuda(), hop=512)
    o = pipe.peaks(1, 8)
    gated = 0
    for h in range(12):
        pipe.step()
        _fill(pipe, o)
        pipe.peaks(1, 8, gated_only=True)
        pipe.stream.synchronize()
        n = int(pipe.out["count"].item())
        on = pipe.out["gate"][:n].bool()
        gated += int(on.sum())
        assert torch.equal(o["cell"][:n, 0][on], pipe.out["cell"][:n][on])
        assert torch.equal(o["xy"][:n, 0][on], pipe.out["xy"][:n][on])
        L, mL = ("L", "max_L") if engine == "direct" else ("Lf", "max_Lf")
        assert torch.equal(o[L][:n, 0][on], pipe.out[mL][:n][on])
        assert (o["count"][:n][on] == 1).all() and (o["count"][:n][~on] == 0).all()
    assert gated >= 4
    pipe.close()
    loc.close()


@pytest.mark.parametrize("engine,M", [("direct", 4), ("gcc_phat", 8)])
def test_refinement_vs_oracle(oracle, engine, M):
    cfg = (dict(num_mics=4, mic_xy=synth.square_mics(0.15), max_shift=20) if M == 4 else
           dict(num_mics=8, frame_len=512, mic_xy=synth.circle_mics(8, 0.15)))
    loc = _loc(engine, **cfg)
    N = loc.dims.N
    hop = N // 2
    lut = loc.lut()
    adc = _adc(loc, 6, hop * 14, 13 + M)
    pipe = StreamPipeline(loc, torch.from_numpy(adc).cuda(), hop=hop)
    raw = _outs(pipe, 3, ls=True, lags=False)
    compared = []

    def without_lags(n, g):
        # the same step again without out->lags: the lag tuples go through the pipeline's scratch
        _fill(pipe, raw)
        assert _raw(pipe, raw, 3, gate=pipe.out["gate"]) == 0
        pipe.stream.synchronize()
        r = _np(raw)
        assert (r["cell"] == g["cell"]).all() and (r["xy_ls"][n:] == SENT).all()
        assert ((r["xy_ls"] == g["xy_ls"]) | np.isnan(g["xy_ls"]))[:n].all()
        assert (np.isnan(r["xy_ls"]) == np.isnan(g["xy_ls"])).all()
        compared.append(int((r["cell"][:n] >= 0).sum()))

    seen = _run_hops(pipe, lut, 14, 3, 8, gated_only=True, ls=True, where=("ls", engine), after=without_lags)
    refined = 0
    for n, ids, gate, est, g in seen:
        if not n:
            continue
        pk = {k: v[:n] for k, v in g.items()}
        empty = _check_ls(oracle, loc, torch.from_numpy(est[ids]), pk, fs=float(FS))
        assert (empty.all(1) == (gate == 0)).all()
        refined += int((~empty).sum())
    assert refined >= 9 and sum(compared) == refined
    pipe.close()
    loc.close()


def test_ordering_without_synchronisation():
    """Graph replay: step, peaks into a set of its own, step, peaks, ... with no
    synchronisation in between equals the run that synchronises after every call."""
    loc = _loc("gcc_phat")
    adc = _adc(loc, 6, 512 * 10, 23)
    runs = []
    for sync in (False, True):
        pipe = StreamPipeline(loc, torch.from_numpy(adc).cuda(), hop=512, use_graph=True)
        sets = [_outs(pipe, 3, ls=True) for _ in range(10)]
        counts = [torch.zeros(1, dtype=torch.int32, device="cuda") for _ in range(10)]
        slots = [torch.zeros(6, dtype=torch.int32, device="cuda") for _ in range(10)]
        torch.cuda.synchronize()
        for o, cnt, ids in zip(sets, counts, slots):
            pipe.step()
            if sync:
                pipe.stream.synchronize()
            assert _raw(pipe, o, 3, radius=5) == 0
            with torch.cuda.stream(pipe.stream):
                cnt.copy_(pipe.out["count"])
                ids.copy_(pipe.out["stream_id"])
            if sync:
                pipe.stream.synchronize()
        pipe.stream.synchronize()
        runs.append(([_np(o) for o in sets], [int(c.item()) for c in counts], [i.cpu().numpy() for i in slots]))
        pipe.close()
    (a, ca, ia), (b, cb, ib) = runs
    assert ca == cb and sum(ca) >= 6 and sum(1 for c in ca if c) >= 2
    for h, (x, y) in enumerate(zip(a, b)):
        n = ca[h]
        # slot order is arbitrary (the selector's atomic counter): rows by stream
        oa, ob = np.argsort(ia[h][:n]), np.argsort(ib[h][:n])
        assert (ia[h][:n][oa] == ib[h][:n][ob]).all()
        R.assert_equal({k: v[:n][oa] for k, v in x.items()}, {k: v[:n][ob] for k, v in y.items()}, ("order", h))
        for k in x:
            assert (x[k][n:] == SENT).all() and (y[k][n:] == SENT).all(), (h, k)
        assert n == 0 or ((x["cell"][:n, 0] >= 0).all() and not np.isnan(x["xy_ls"][:n, 0]).any())
    loc.close()


@pytest.mark.parametrize("engine", ["direct", "gcc_phat"])
def test_whole_state(engine):
    loc = _loc(engine)
    lut, d = loc.lut(), loc.dims
    S = 6
    adc = _adc(loc, S, 512 * 12, 23, quiet=(1,))
    pipe = StreamPipeline(loc, torch.from_numpy(adc).cuda(), hop=512)
    compared = 0
    for h in range(12):
        pipe.step()
        listed = pipe.peaks(2, 8)
        everything = pipe.peaks_all(2, 8)
        pipe.stream.synchronize()
        n = int(pipe.out["count"].item())
        ids = pipe.out["stream_id"][:n].cpu().numpy()
        on = pipe.out["gate"][:n].cpu().numpy() != 0
        lst, g = _np(listed), _np(everything)
        for k in g:  # on listed gated slots peaks() is peaks_all()'s row of that stream
            x, y = lst[k][:n][on], g[k][ids[on]]
            assert ((x == y) | ((x != x) & (y != y))).all(), (h, k)
        compared += int(on.sum())
    assert compared >= 3
    _, est, _ = pipe.state()
    ptr, is_float = pipe.est_ptr()
    assert is_float == (engine == "gcc_phat") and ptr
    host = np.zeros_like(est)
    L = _lib.load()
    L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert L.hipMemcpy(host.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), host.nbytes, 2) == 0  # device to host
    assert host.tobytes() == est.tobytes() and est.shape == (S, d.P, d.K)
    assert (est[1] == 0).all() and np.abs(est).max() > 0
    R.assert_equal(g, R.peaks_ref(est, lut, *_ref_args(loc), 2, 8), engine)
    assert g["cell"][1, 0] == 0 and g["L" if engine == "direct" else "Lf"][1, 0] == 0  # never updated: cell 0, L = 0
    pipe.close()
    loc.close()


def test_errors_leave_outputs_untouched():
    loc = _loc("gcc_phat")
    adc = _adc(loc, 4, 512 * 4, 23)
    pipe = StreamPipeline(loc, torch.from_numpy(adc).cuda(), hop=512, mode="continuous", activity_var=0)
    for _ in range(4):
        pipe.step()
    o = _outs(pipe, 8)
    no_cell = {k: v for k, v in o.items() if k != "cell"}
    L = _lib.load()
    bad = [
        (dict(st=False), "NULL"), (dict(prm=False), "NULL"), (dict(out=False), "NULL"),
        (dict(o=no_cell), "cell"),
        (dict(Kp=0), "num_peaks"), (dict(Kp=9), "num_peaks"), (dict(radius=-1), "radius"),
    ]
    for kw, word in bad:
        kw = dict(kw)
        assert _raw(pipe, kw.pop("o", o), kw.pop("Kp", 2), **kw) == -1, kw
        assert word in L.tdoa_last_error().decode(), (kw, L.tdoa_last_error())
    # a 201 x 201 grid: the L map alone is past the kernel's LDS budget
    big = _loc("gcc_phat", grid_half_w=100, grid_half_h=100)
    bp = StreamPipeline(big, torch.from_numpy(adc).cuda(), hop=512, mode="continuous", activity_var=0)
    for _ in range(3):
        bp.step()
    assert _raw(bp, o, 2) == -1 and "LDS" in L.tdoa_last_error().decode()
    with pytest.raises(_lib.TdoaError):
        bp.peaks(2, 8)
    with pytest.raises(_lib.TdoaError):
        pipe.peaks(9, 8)
    torch.cuda.synchronize()
    for k, t in o.items():
        assert (t == SENT).all(), k
    # ... and the same set is written by a valid call (4 listed streams)
    assert _raw(pipe, o, 8) == 0
    pipe.stream.synchronize()
    assert int(pipe.out["count"].item()) == 4 and (o["cell"][:4, 0] >= 0).all() and (o["count"][:4] >= 1).all()
    # the state pointer's own NULL checks
    p, f = C.c_void_p(), C.c_int()
    for args in ((None, C.byref(p), C.byref(f)), (pipe._h, None, C.byref(f)), (pipe._h, C.byref(p), None)):
        assert L.tdoa_stream_est_device(*args) == -1 and b"NULL" in L.tdoa_last_error()
    # after a reset there is no last step: nothing is launched
    pipe.reset()
    _fill(pipe, o)
    assert _raw(pipe, o, 8) == 0
    pipe.stream.synchronize()
    assert all((t == SENT).all() for t in o.values())
    bp.close()
    big.close()
    pipe.close()
    loc.close()
