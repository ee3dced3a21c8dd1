"""The tracker without a GPU: tdoa_track_host (the host twin, compiled from the
inline functions k_track runs) against the numpy restatement of the rule
(tests/track_ref.py) bit for bit, hand-made cases with known answers, every
TDOA_ERR_INVALID case of the three entry points that needs no device, the
record's layout, and a program of its own under ASan + UBSan."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT

import tdoa
from tdoa import _lib

import track_cases as TC
import track_ref as R

F = np.float32
NAN = float("nan")


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def run_both(calls, S, T, tally=None):
    """The sequence through the reference and the host twin; every byte compared after every call."""
    tr, nid = R.new_state(S)
    htr, hnid = R.new_state(S)
    tally = R.new_tally() if tally is None else tally
    for c, (sor, t, cnt, xy) in enumerate(calls):
        tr, nid, out, tally = R.track_rows(tr, nid, t, cnt, xy, stream_of_row=sor, tally=tally, **TC.params(T))
        ho = tdoa.track_host(htr, hnid, t, cnt, xy, stream_of_row=sor, **TC.params(T))
        assert same(tr, htr) and same(nid, hnid), f"state differs after call {c}"
        for k in ("tracks", "assigned", "num_confirmed"):
            assert same(out[k], ho[k]), f"{k} differs in call {c}"
    return tr, nid, tally


@pytest.mark.parametrize("seed", TC.SEEDS)
@pytest.mark.parametrize("T,Kp", TC.SHAPES)
def test_host_equals_reference_bit_for_bit(T, Kp, seed):
    tr, nid, tally = run_both(TC.make_sequence(seed, T, Kp), 6, T)
    assert nid.max() > 1 and tally["births"] > 0
    assert (tr[:, T:]["id"] == 0).all()  # slots >= T are never used


def test_the_sequences_contain_every_event_kind():
    """The condition on the seeds: over the sequences the reference's tally
    shows every event kind, and the shapes with room for the scripted ties
    (T >= 2, Kp >= 2) show them."""
    total = R.new_tally()
    for T, Kp in TC.SHAPES:
        for seed in TC.SEEDS:
            tr, nid = R.new_state(6)
            tally = R.new_tally()
            for sor, t, cnt, xy in TC.make_sequence(seed, T, Kp):
                tr, nid, _, tally = R.track_rows(tr, nid, t, cnt, xy, stream_of_row=sor, tally=tally, **TC.params(T))
            for e in R.EVENTS:
                total[e] += tally[e]
            if T >= 2 and Kp >= 2:
                assert tally["tie_breaks"] >= 2, (T, Kp, seed, tally)
            for e in ("births", "confirmations", "miss_outs", "coast_outs", "gate_rejections", "rows_skipped"):
                assert tally[e] > 0, (T, Kp, seed, e)
    print(total)
    assert all(total[e] > 0 for e in R.EVENTS), total


def test_permuted_and_partial_rows_touch_only_their_streams():
    S = 9
    tr, nid = R.new_state(S)
    rng = np.random.default_rng(5)
    for e in range(12):
        sor = rng.permutation(S)[:4].astype(np.int32)
        before, nbefore = tr.copy(), nid.copy()
        xy = rng.uniform(-1, 1, (4, 3, 2)).astype(np.float32)
        cnt = rng.integers(0, 4, 4).astype(np.int32)
        t = np.full(4, 1000 + e * TC.HOP_US, np.int64)
        rtr, rnid, out, _ = R.track_rows(tr, nid, t, cnt, xy, stream_of_row=sor, **TC.params(4))
        ho = tdoa.track_host(tr, nid, t, cnt, xy, stream_of_row=sor, **TC.params(4))
        assert same(rtr, tr) and same(rnid, nid) and all(same(out[k], ho[k]) for k in out)
        others = np.setdiff1d(np.arange(S), sor)
        assert same(before[others], tr[others]) and (nbefore[others] == nid[others]).all()


# ---------------------------------------------------------------- hand-made cases
def one(tracks, next_id, t, zs, Kp=None, **params):
    """One row on stream 0 through both implementations (state updated in place)."""
    Kp = max(len(zs), 1) if Kp is None else Kp
    xy = np.zeros((1, Kp, 2), np.float32)
    for k, z in enumerate(zs):
        xy[0, k] = z
    t_us, cnt = np.array([t], np.int64), np.array([len(zs)], np.int32)
    rtr, rnid, rout, _ = R.track_rows(tracks, next_id, t_us, cnt, xy, **params)
    out = tdoa.track_host(tracks, next_id, t_us, cnt, xy, **params)
    assert same(rtr, tracks) and same(rnid, next_id) and all(same(rout[k], out[k]) for k in out)
    return out


def test_tie_of_two_tracks_for_one_measurement_goes_to_the_lower_slot():
    tr, nid = R.new_state(1)
    o = one(tr, nid, 0, [(-0.125, 0.0), (0.125, 0.0)])
    assert o["assigned"].tolist() == [[1, 2]] and tr[0, :2]["id"].tolist() == [1, 2]
    o = one(tr, nid, 10240, [(0.0, 0.0)])
    assert o["assigned"].tolist() == [[1]]
    assert tr[0, 0]["hits"] == 2 and tr[0, 0]["peak"] == 0 and tr[0, 0]["misses"] == 0
    assert tr[0, 1]["hits"] == 1 and tr[0, 1]["peak"] == -1 and tr[0, 1]["misses"] == 1


def test_tie_of_two_measurements_for_one_track_goes_to_the_lower_index():
    tr, nid = R.new_state(1)
    one(tr, nid, 0, [(2.0, 2.0)])
    o = one(tr, nid, 10240, [(2.125, 2.0), (1.875, 2.0)])
    assert o["assigned"].tolist() == [[1, 2]]  # k = 0 updates track 1, k = 1 is born as 2
    assert tr[0, 0]["peak"] == 0 and tr[0, 0]["hits"] == 2 and tr[0, 0]["x"] > 2.0
    assert tr[0, 1]["id"] == 2 and tr[0, 1]["x"] == F(1.875) and tr[0, 1]["peak"] == 1


def test_a_stationary_measurement_repeated_keeps_the_state_on_it():
    tr, nid = R.new_state(1)
    z = (F(0.3), F(-0.7))
    for e in range(10):
        o = one(tr, nid, e * 10240, [z])
        a = tr[0, 0]
        assert o["assigned"].tolist() == [[1]] and nid[0] == 1
        assert a["x"] == z[0] and a["y"] == z[1] and a["vx"] == 0 and a["vy"] == 0  # the innovation is 0
        assert a["hits"] == e + 1 and a["t_us"] == a["upd_us"] == e * 10240
    assert tr[0, 0]["status"] == 2 and 0 < tr[0, 0]["p00"] < F(0.01)


def test_a_nan_measurement_is_ignored():
    tr, nid = R.new_state(1)
    o = one(tr, nid, 0, [(NAN, 0.0), (0.5, 0.5), (0.1, float("inf"))])
    assert o["assigned"].tolist() == [[0, 1, 0]] and nid[0] == 1
    assert tr[0, 0]["peak"] == 1 and (tr[0, 1:]["id"] == 0).all()
    # only invalid measurements: the row is evaluated, the track misses, nothing is born
    o = one(tr, nid, 10240, [(NAN, NAN)])
    assert o["assigned"].tolist() == [[0]] and tr[0, 0]["misses"] == 1 and tr[0, 0]["t_us"] == 10240 and nid[0] == 1


def test_a_row_without_measurements_is_not_evaluated():
    tr, nid = R.new_state(1)
    one(tr, nid, 0, [(0.5, 0.5)])
    before = tr.copy()
    o = one(tr, nid, 10_000_000, [], Kp=2)  # past max_coast_us: still untouched
    assert same(before, tr) and o["assigned"].tolist() == [[0, 0]] and same(o["tracks"][0], tr[0])


def test_time_running_backwards_gives_dt_zero():
    tr, nid = R.new_state(1)
    one(tr, nid, 50_000, [(0.5, 0.5)])
    p = tr[0, 0].copy()
    one(tr, nid, 20_000, [(0.5, 0.5)])
    a = tr[0, 0]
    # predict with dt = 0 leaves p00 = r, so k0 = r / (r + r) = 0.5 exactly
    assert a["t_us"] == 20_000 and a["upd_us"] == 20_000 and a["hits"] == 2
    assert a["p00"] == p["p00"] - F(0.5) * p["p00"] and a["p11"] == p["p11"] and a["x"] == F(0.5)


def test_confirm_hits_one_is_born_confirmed():
    tr, nid = R.new_state(1)
    o = one(tr, nid, 0, [(0.0, 0.0)], confirm_hits=1)
    assert tr[0, 0]["status"] == 2 and o["num_confirmed"].tolist() == [1]
    tr, nid = R.new_state(1)
    o = one(tr, nid, 0, [(0.0, 0.0)], confirm_hits=2)
    assert tr[0, 0]["status"] == 1 and o["num_confirmed"].tolist() == [0]
    o = one(tr, nid, 10240, [(0.0, 0.0)], confirm_hits=2)
    assert tr[0, 0]["status"] == 2 and o["num_confirmed"].tolist() == [1]


def test_ids_never_repeat_within_a_stream():
    for T, Kp in TC.SHAPES:
        tr, nid = R.new_state(6)
        seen = [set() for _ in range(6)]
        for sor, t, cnt, xy in TC.make_sequence(TC.SEEDS[0], T, Kp):
            before = tr["id"].copy()
            tdoa.track_host(tr, nid, t, cnt, xy, stream_of_row=sor, **TC.params(T))
            for s in range(6):
                new = set(tr[s]["id"][tr[s]["id"] != 0].tolist()) - set(before[s].tolist())
                assert not (new & seen[s]) and all(i > max(seen[s], default=0) for i in new)
                seen[s] |= new
        assert all(len(seen[s]) == nid[s] for s in range(6))  # ids 1..next_id, each given once


# ---------------------------------------------------------------- argument checks
GOOD = dict(TC.PARAMS, max_tracks=4)
BAD_PARAMS = [("max_tracks", 0), ("max_tracks", 9), ("confirm_hits", 0), ("max_misses", 0), ("max_coast_us", 0),
              ("max_coast_us", -5), ("gate_d2", 0.0), ("gate_d2", NAN), ("gate_d2", float("inf")),
              ("meas_var", 0.0), ("meas_var", -1.0), ("meas_var", NAN), ("meas_var", float("inf")),
              ("accel_psd", -1.0), ("accel_psd", NAN), ("accel_psd", float("inf")),
              ("init_vel_var", 0.0), ("init_vel_var", NAN), ("init_vel_var", float("inf"))]


class Args:
    """Host buffers for a 2-row call, the outputs pre-filled with a sentinel."""

    def __init__(self):
        self.tracks, self.next_id = R.new_state(2)
        self.tracks["id"][:] = 7
        self.t = np.array([5, 5], np.int64)
        self.count = np.array([1, 1], np.int32)
        self.xy = np.zeros((2, 2, 2), np.float32)
        self.o_tracks = np.full((2, 4, 64), 0xA5, np.uint8)
        self.o_asg = np.full((2, 2), -77, np.int32)
        self.o_conf = np.full(2, -77, np.int32)
        self.prm = _lib.track_params(**GOOD)
        self.out = _lib.TrackOutputs(self.o_tracks.ctypes.data, self.o_asg.ctypes.data, self.o_conf.ctypes.data)
        self.snap = self.snapshot()

    def snapshot(self):
        return [a.tobytes() for a in (self.tracks, self.next_id, self.o_tracks, self.o_asg, self.o_conf)]

    def call(self, entry, **over):
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        v = dict(tracks=p(self.tracks), next_id=p(self.next_id), rows=2, sor=None, t=p(self.t), count=p(self.count),
                 xy=p(self.xy), Kp=2, prm=C.byref(self.prm), out=C.byref(self.out))
        v.update(over)
        L = tdoa.load()
        if entry == "tdoa_track_host":
            rc = L.tdoa_track_host(v["tracks"], v["next_id"], v["rows"], v["sor"], v["t"], v["count"], v["xy"],
                                   v["Kp"], v["prm"], v["out"])
        else:  # the "device" pointers are never read: the checks come before any device call
            rc = L.tdoa_track_batch(0, v["tracks"], v["next_id"], v["rows"], v["sor"], v["t"], v["count"], v["xy"],
                                    v["Kp"], v["prm"], v["out"], None)
        return rc, (L.tdoa_last_error() or b"").decode()

    def untouched(self):
        return self.snapshot() == self.snap


@pytest.mark.parametrize("entry", ["tdoa_track_host", "tdoa_track_batch"])
def test_invalid_arguments_are_named_and_nothing_is_touched(entry):
    a = Args()
    for name in ("tracks", "next_id", "t", "count", "xy", "prm", "out"):
        rc, msg = a.call(entry, **{name: None})
        assert rc == -1 and entry in msg and "NULL" in msg, (name, msg)
    empty = _lib.TrackOutputs()
    rc, msg = a.call(entry, out=C.byref(empty))
    assert rc == -1 and entry in msg and "output" in msg
    for Kp in (0, -1, 9):
        rc, msg = a.call(entry, Kp=Kp)
        assert rc == -1 and entry in msg and "Kp" in msg
    for rows in (-1, 2 ** 31, 2 ** 40):
        rc, msg = a.call(entry, rows=rows)
        assert rc == -1 and entry in msg and "rows" in msg
    for field, val in BAD_PARAMS:
        prm = _lib.track_params(**dict(GOOD, **{field: val}))
        rc, msg = a.call(entry, prm=C.byref(prm))
        assert rc == -1 and entry in msg and field in msg, (field, val, msg)
    assert a.untouched()
    # rows = 0 is TDOA_OK and touches nothing (the device form returns before any device call)
    rc, _ = a.call(entry, rows=0)
    assert rc == 0 and a.untouched()
    if entry == "tdoa_track_host":  # and the same arguments, valid, do run
        rc, _ = a.call(entry)
        assert rc == 0 and not a.untouched()


def test_stream_entry_points_reject_null_without_a_device():
    L = tdoa.load()
    a = Args()
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    rc = L.tdoa_stream_track(None, C.byref(a.prm), p(a.count), p(a.xy), 2, C.byref(a.out), None)
    msg = L.tdoa_last_error()
    assert rc == -1 and b"tdoa_stream_track" in msg and b"NULL" in msg and a.untouched()
    tr, nid = C.c_void_p(5), C.c_void_p(5)
    assert L.tdoa_stream_tracks_device(None, C.byref(tr), C.byref(nid)) == -1
    msg = L.tdoa_last_error()
    assert b"tdoa_stream_tracks_device" in msg and b"NULL" in msg and tr.value == 5 and nid.value == 5


def test_python_faces_exist():
    for name in ("tdoa_track_batch", "tdoa_track_host", "tdoa_stream_track", "tdoa_stream_tracks_device"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(tdoa.load(), name)
    from tdoa.localizer import Localizer
    from tdoa.stream import StreamPipeline
    assert callable(Localizer.track_batch)
    for m in ("track", "track_records", "tracks_all"):
        assert callable(getattr(StreamPipeline, m))
    with pytest.raises(TypeError):
        _lib.track_params(gate=3.0)


# ---------------------------------------------------------------- layout, and the program of its own
@pytest.fixture(scope="module")
def san_tool():
    r = subprocess.run(["make", "-C", PKG, "track_host_san"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return os.path.join(ROOT, "tools", "track_host_san")


def run_tool(tool, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    return subprocess.run([tool, *args], capture_output=True, text=True, timeout=300, env=env)


def test_record_layout(san_tool):
    dt = tdoa.TRACK_DTYPE
    assert dt == R.TRACK_DTYPE and dt.itemsize == 64 and C.sizeof(_lib.Track) == 64
    assert C.sizeof(_lib.TrackParams) == 40 and C.sizeof(_lib.TrackOutputs) == 24
    r = run_tool(san_tool)
    assert r.returncode == 0, r.stderr[-2000:]
    w = r.stdout.split()
    c_layout = dict(zip(w[0::2], map(int, w[1::2])))
    assert c_layout.pop("sizeof") == 64
    assert list(c_layout) == list(dt.names)  # the header's field order
    for name in dt.names:
        assert c_layout[name] == dt.fields[name][1] == getattr(_lib.Track, name).offset, name
        assert dt.fields[name][0].itemsize == getattr(_lib.Track, name).size, name


@pytest.mark.parametrize("T,Kp", [(8, 8), (3, 5)])
def test_program_of_its_own_under_asan_and_ubsan(san_tool, tmp_path, T, Kp):
    S, rows = 6, 5
    calls = TC.make_sequence(TC.SEEDS[1], T, Kp, S=S, rows=rows)
    prm = _lib.track_params(**TC.params(T))
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([S, T, Kp, len(calls), rows], np.int32).tobytes())
        f.write(bytes(prm))
        for sor, t, cnt, xy in calls:
            f.write(sor.tobytes() + t.tobytes() + cnt.tobytes() + xy.tobytes())
    r = run_tool(san_tool, str(tmp_path / "in.bin"), str(tmp_path / "out.bin"))
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    want = b""
    tr, nid = R.new_state(S)
    for sor, t, cnt, xy in calls:
        tr, nid, out, _ = R.track_rows(tr, nid, t, cnt, xy, stream_of_row=sor, **TC.params(T))
        want += out["tracks"].tobytes() + out["assigned"].tobytes() + out["num_confirmed"].tobytes()
    want += tr.tobytes() + nid.tobytes()
    assert open(tmp_path / "out.bin", "rb").read() == want


def test_scenario_premise_holds_for_the_oracle_chain(oracle):
    """tests/track_scenario.py: the CPU chain alone (oracle streaming run ->
    peaks_ref -> oracle.ls_refine -> track_ref) follows every stream's fixed
    source with one confirmed track of unchanging id, assigned at every gated
    hop.  tests/test_gpu_track.py asks the same of the device."""
    import track_scenario as SC
    adc, lut, win, mics = SC.capture(oracle)
    hops = SC.oracle_hops(oracle, adc, lut, win, mics)
    f, tr, nid = SC.oracle_tracks(hops)
    f.done()
    assert (nid == 1).all() and (tr[:, 0]["status"] == 2).all() and (tr[:, 1:]["id"] == 0).all()
