"""The tracker's scenario through the DIRECT streaming pipeline, and its CPU
oracle chain: the oracle's streaming run -> peaks_ref -> oracle.ls_refine ->
track_ref.  Chosen here, on the CPU, such that the chain alone shows, on every
stream (each has one fixed source): from the track's confirmation on there is
exactly one confirmed track, its id never changes, and it is assigned a peak at
every gated hop.  tests/test_track_cpu.py checks that premise; the GPU test
must then show the same on the device.
"""
import numpy as np

import peaks_ref as PR
import track_ref as R

FS, MAX_SHIFT, N, HOP, HOPS, S, SEED = 48000, 44, 1024, 512, 32, 4, 0x7AC5
# the map of one source over three pairs has stable side maxima (where two of the
# three pairs still agree); in this capture they stay below 0.67 of the main
# peak, and min_rel = 0.8 keeps them out: left in, they become confirmed tracks
KP, RADIUS, MIN_REL = 2, 8, 0.8
# a grid cell is 1/24 m: r = (3 cells)^2; a fixed source needs no agility
PRM = dict(R.DEFAULTS, max_tracks=4, confirm_hits=3, max_misses=3, max_coast_us=2_000_000, gate_d2=9.0,
           meas_var=0.015625, accel_psd=0.01, init_vel_var=0.25)
GRID = dict(grid_W=101, half_w=50, half_h=50, grid_scale=24.0)


def capture(oracle):
    """(adc u8 [S][HOP * HOPS][3], lut [3][101 * 101], window, mics)."""
    import ctypes as C

    from tdoa import synth
    mics = np.zeros((3, 2), np.float32)
    oracle.lib().orc_microphones_ref(mics.ctypes.data_as(C.c_void_p))
    lut = oracle.build_lut(mics, fs=FS, max_shift=MAX_SHIFT).reshape(3, -1)
    adc = synth.adc_stream(S, HOP * HOPS, 3, lut, MAX_SHIFT, SEED).numpy()
    return adc, lut, PR.two_source_window(N), mics


def oracle_hops(oracle, adc, lut, win, mics):
    """Per hop, what the pipeline lists, from the oracle alone: a list of
    (stream_id [n], end [n], gate [n], count [n], xy_ls [n][KP][2] float32),
    streams ascending.  The EMA state after hop h is the oracle's final state
    on the capture's first (h + 1) * HOP samples."""
    hops = []
    for h in range(HOPS):
        r = oracle.stream_run(adc[:, :(h + 1) * HOP], N, FS, MAX_SHIFT, win, lut)
        ids, end, gate, count, xy = [], [], [], [], []
        for s in range(S):
            for i in range(r["n_trig"][s]):
                e = int(r["end"][s, i])
                if not h * HOP < e <= (h + 1) * HOP:
                    continue
                ids.append(s)
                end.append(e)
                gate.append(int(r["gate"][s, i]))
                z = np.full((KP, 2), np.nan, np.float32)
                n = 0
                if gate[-1]:
                    pk = PR.peaks_ref(r["est"][s][None], lut, GRID["grid_W"], GRID["half_w"], GRID["half_h"],
                                      GRID["grid_scale"], MAX_SHIFT, KP, RADIUS, MIN_REL)
                    n = int(pk["count"][0])
                    for k in range(n):
                        uv, _ = oracle.ls_refine(r["est"][s][None], pk["lags"][:, k], mics, pk["cell"][:, k],
                                                 half_w=GRID["half_w"], half_h=GRID["half_h"],
                                                 grid_scale=GRID["grid_scale"], fs=float(FS))
                        z[k] = uv[0].astype(np.float32)
                count.append(n)
                xy.append(z)
        hops.append((np.array(ids, np.int32), np.array(end, np.int64), np.array(gate, np.uint8),
                     np.array(count, np.int32), np.array(xy, np.float32).reshape(len(ids), KP, 2)))
    return hops


def times(end):
    return (np.asarray(end).astype(np.uint64) * np.uint64(1000000) // np.uint64(FS)).astype(np.int64)


class Follow:
    """The scenario's properties, fed one hop at a time with what a tracker
    reported for the listed slots: per stream, from the hop its first track is
    confirmed, exactly one confirmed track, the same id, assigned at every gated hop."""

    def __init__(self):
        self.conf_id = {}
        self.gated_after = {s: 0 for s in range(S)}

    def hop(self, ids, gate, tracks, assigned, where=""):
        for i, s in enumerate(np.asarray(ids).tolist()):
            conf = tracks[i][tracks[i]["status"] == 2]
            if s not in self.conf_id:
                if len(conf):
                    assert len(conf) == 1, (where, s, "two tracks confirmed at once")
                    self.conf_id[s] = int(conf[0]["id"])
                continue
            assert len(conf) == 1 and int(conf[0]["id"]) == self.conf_id[s], (where, s, conf["id"].tolist())
            if gate[i]:
                assert self.conf_id[s] in assigned[i].tolist() and conf[0]["peak"] >= 0, (where, s, "not assigned")
                self.gated_after[s] += 1

    def done(self):
        """Every stream confirmed a track and went on to be followed."""
        assert sorted(self.conf_id) == list(range(S)), self.conf_id
        assert all(v >= 2 for v in self.gated_after.values()), self.gated_after


def oracle_tracks(hops):
    """track_ref over the oracle's hops: the Follow of the chain, and its final state."""
    tr, nid = R.new_state(S)
    f = Follow()
    for h, (ids, end, gate, count, xy) in enumerate(hops):
        tr, nid, out, _ = R.track_rows(tr, nid, times(end), count, xy, stream_of_row=ids, **PRM)
        f.hop(ids, gate, out["tracks"], out["assigned"], ("oracle", h))
    return f, tr, nid
