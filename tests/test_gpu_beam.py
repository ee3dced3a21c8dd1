"""The beamformer on the device (k_beam: tdoa_beam_batch, Localizer.beam_batch;
k_beam_ring<T>: tdoa_stream_beam, StreamPipeline.beam).

The delay codes, the active bytes and block_start must equal the numpy
restatement of the rule (tests/beam_ref.py) and the host twin exactly; the
audio must lie within the reference's own per-sample bound, gamma(M) times the
magnitude sum of the taps (an fp32 sum of 16 M fused multiply-adds), of the
float64 reference -- and of the host twin, which runs the same inline
functions.  Outputs are pre-filled with a sentinel; what a call must not write
must still hold it.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import beam_cases as BC  # noqa: E402
import beam_ref as R  # noqa: E402
import stream_cont_cases as Cs  # noqa: E402
import tdoa  # noqa: E402
from tdoa import _lib, synth  # noqa: E402
from tdoa.localizer import Localizer  # noqa: E402
from tdoa.stream import StreamPipeline  # noqa: E402

FS = 48000
SENT = 0x5A
MICS = {2: np.array([[-0.066, 0], [0.066, 0]], np.float32), 3: None, 4: synth.square_mics(0.15),
        **{M: synth.circle_mics(M, 0.15) for M in (5, 6, 7, 8)}}


def _loc(M, N, engine="gcc_phat", fmt="adc8", mics=None):
    return Localizer(engine=engine, num_mics=M, frame_len=N, sample_rate_hz=FS,
                     mic_xy=MICS[M] if mics is None else mics, sample_format=fmt)


def _geom(lc):
    """(BeamGeometry, mics, fs, c) of a localizer, and its latency checked against the reference's."""
    bg = lc.beam_geometry()
    M = lc.dims.M
    mics = np.array(list(bg.mic_xy), np.float32).reshape(8, 2)[:M].copy()
    assert bg.num_mics == M and (mics == lc.mics().reshape(M, 2)).all()
    assert lc.beam_latency() == R.latency(mics, bg.sample_rate_hz, bg.speed_of_sound) == tdoa.beam_latency(bg)
    return bg, mics, bg.sample_rate_hz, bg.speed_of_sound


def near(got, ref, other, M):
    """got within gamma(M) mag of the float64 reference and of `other` (the host twin's float32)."""
    g = got.astype(np.float64)
    tol = R.gamma(M) * ref["mag"]
    return bool((np.abs(g - ref["audio"]) <= tol).all() and (np.abs(g - other.astype(np.float64)) <= tol).all())


# ---------------------------------------------------------------- the block form
_locs = {}


@pytest.fixture(scope="module")
def locs():
    yield lambda M, N: _locs.setdefault((M, N), _loc(M, N))
    for lc in _locs.values():
        lc.close()
    _locs.clear()


@pytest.mark.parametrize("Kt", [1, 3, 8])
@pytest.mark.parametrize("M,N", [(3, 256), (4, 2048), (8, 1024)])
def test_batch_equals_host_and_reference(locs, M, N, Kt):
    lc = locs(M, N)
    bg, mics, fs, c = _geom(lc)
    B = 7
    frames, xy, count = BC.block_case(mics, B, N, Kt, 100 + 10 * M + Kt)
    ref = R.beam(mics, fs, c, BC.H, frames, xy, count)
    host = tdoa.beam_host(bg, frames, xy, count)
    assert host["delays"].tobytes() == ref["delays"].tobytes() and ref["active"].any() and not ref["active"].all()
    d_fr, d_xy, d_cnt = (torch.from_numpy(a).cuda() for a in (frames, xy, count))
    outs = {"audio": torch.empty((B, Kt, N), dtype=torch.float32, device="cuda"),
            "delays": torch.empty((B, Kt, M), dtype=torch.int32, device="cuda"),
            "active": torch.empty((B, Kt), dtype=torch.uint8, device="cuda")}
    for use in (("audio", "delays", "active"), ("audio",), ("audio", "active")):
        for v in outs.values():
            v.view(torch.uint8).fill_(SENT)
        got = lc.beam_batch(d_fr, d_xy, d_cnt, outputs={k: outs[k] for k in use})
        torch.cuda.synchronize()
        assert set(got) == set(use)
        g = {k: v.cpu().numpy() for k, v in outs.items()}
        assert near(g["audio"], ref, host["audio"], M)
        assert (g["audio"][ref["active"] == 0] == 0).all()
        for k in ("delays", "active"):
            if k in use:
                assert g[k].tobytes() == ref[k].tobytes() == host[k].tobytes(), k
            else:
                assert (g[k].view(np.uint8) == SENT).all(), f"{k} written without being passed"
    # count = None: every finite target; fresh outputs
    full = R.beam(mics, fs, c, BC.H, frames, xy, None)
    got = lc.beam_batch(d_fr, d_xy)
    torch.cuda.synchronize()
    assert got["delays"].cpu().numpy().tobytes() == full["delays"].tobytes()
    assert near(got["audio"].cpu().numpy(), full, tdoa.beam_host(bg, frames, xy)["audio"], M)


def test_batch_errors_leave_outputs_untouched(locs):
    lc = locs(3, 256)
    L = _lib.load()
    fr = torch.zeros((2, 3, 256), dtype=torch.int16, device="cuda")
    xy = torch.zeros((2, 2, 2), dtype=torch.float32, device="cuda")
    audio = torch.full((2, 2, 256), 7.0, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    out, none = _lib.BeamOutputs(audio.data_ptr(), None, None, None), _lib.BeamOutputs()
    for args, word in (((lc._ctx, None, 2, None, p(xy), 2, C.byref(out), None), b"NULL"),
                       ((lc._ctx, p(fr), 2, None, None, 2, C.byref(out), None), b"NULL"),
                       ((lc._ctx, p(fr), 2, None, p(xy), 2, None, None), b"NULL"),
                       ((lc._ctx, p(fr), 2, None, p(xy), 2, C.byref(none), None), b"audio"),
                       ((lc._ctx, p(fr), 2, None, p(xy), 0, C.byref(out), None), b"Kt"),
                       ((lc._ctx, p(fr), 2, None, p(xy), 9, C.byref(out), None), b"Kt"),
                       ((lc._ctx, p(fr), -1, None, p(xy), 2, C.byref(out), None), b"B")):
        assert L.tdoa_beam_batch(*args) == -1 and word in L.tdoa_last_error(), word
    assert L.tdoa_beam_batch(lc._ctx, p(fr), 0, None, p(xy), 2, C.byref(out), None) == 0  # B = 0: no launch
    torch.cuda.synchronize()
    assert (audio == 7.0).all()
    # eight mics 20 m apart at N = 2048: the staged block exceeds the LDS limit
    wide = _loc(8, 2048, mics=synth.circle_mics(8, 10.0))
    A, D = wide.beam_latency()
    assert (8 * (2048 + D + 15) + 512) * 4 > 150 * 1024
    with pytest.raises(tdoa.TdoaError, match="LDS"):
        wide.beam_batch(torch.zeros((1, 8, 2048), dtype=torch.int16, device="cuda"),
                        torch.zeros((1, 1, 2), dtype=torch.float32, device="cuda"))
    wide.close()


# ---------------------------------------------------------------- the streaming form
S, HOPS, KT = 5, 8, 3

# (engine, mode, ring type, M, N, hop, capture_len).  Of the first six,
# capture_len * M is odd in some cases (a stream's ring is then 1- or 2-byte
# aligned only: element loads) and a multiple of 8 in others (16-byte vectors
# in every stream or every other one; RING_16 below says which), and every ring
# is shorter than the 8 hops: the staged runs wrap it -- from hop 4 at the
# latest where hop >= 200, at hops 7 and 8 where hop = 64 (capture_len >= N +
# 2 hop = 384 samples there, and six hops are 384).
STREAM_CASES = [
    ("direct", "triggered", np.uint8, 3, 256, 64, 385),
    ("direct", "triggered", np.uint8, 3, 1024, 512, 2051),
    ("gcc_phat", "triggered", np.uint8, 4, 1024, 512, 2050),
    ("gcc_phat", "triggered", np.int16, 3, 256, 200, 657),
    ("gcc_phat", "continuous", np.int16, 4, 1024, 512, 2048),
    ("gcc_phat", "continuous", np.uint8, 3, 256, 200, 664),
    # Every other mic count, on pipelines the streaming tests of those counts create (tests/test_gpu_stream.py,
    # tests/mic_count_cases.py, tests/stream16_cases.py, tests/stream_long_cases.py).  ring_stage walks a 16-byte
    # vector's elements over (sample row, mic): 2 mics put eight rows into a uint8 vector; 5, 6 and 7 turn the
    # row inside a vector at a different place in each; 8 mics are two rows per uint8 vector and one per int16
    # vector, on the 8 x 2048 pipeline at its hop of 1024 and on 8 x 1024.  The last is the 4 x 4096 pipeline.
    ("direct", "triggered", np.uint8, 2, 1024, 512, 2049),
    ("gcc_phat", "continuous", np.int16, 5, 1024, 512, 2056),
    ("gcc_phat", "continuous", np.int16, 6, 1024, 512, 2049),
    ("gcc_phat", "continuous", np.uint8, 7, 512, 256, 1040),
    ("gcc_phat", "triggered", np.uint8, 8, 2048, 1024, 4098),
    ("gcc_phat", "triggered", np.int16, 8, 1024, 512, 2049),
    ("gcc_phat", "continuous", np.int16, 4, 4096, 2048, 8195),
]
# (ring type, M, capture_len) of the cases whose rings are multiples of 16 bytes each: every stream's ring then
# starts as the first does, 16-byte aligned, and the vectors carry its runs up to the seam at the ring's end.
# In every other case the streams' alignments differ, down to element loads alone.  Both classes in both types.
RING_16 = {(np.int16, 4, 2048), (np.int16, 5, 2056), (np.uint8, 7, 1040), (np.uint8, 8, 4098), (np.int16, 8, 2049)}
LONG_FRAME = {(8, 2048): 1024, (4, 4096): 2048}  # the k_f16_ring pipelines and the hop each is run at here


def test_stream_cases_reach_every_ring_walk():
    """What the streaming cases cover together, on their parameters alone."""
    assert {c[3] for c in STREAM_CASES} == {2, 3, 4, 5, 6, 7, 8}
    for dtype in (np.uint8, np.int16):
        mine = [c for c in STREAM_CASES if c[2] == dtype]
        assert {(c[2], c[3], c[6]) in RING_16 for c in mine} == {False, True}
        assert any(c[3] == 8 for c in mine)
        assert any(c[3] in (2, 8) for c in mine) and any(c[3] in (5, 6, 7) for c in mine)
    for (M, N), hop in LONG_FRAME.items():
        assert any(c[0] == "gcc_phat" and c[3:6] == (M, N, hop) for c in STREAM_CASES)


def _pipe(lc, cap_len, dtype, hop, mode, use_graph):
    M = lc.dims.M
    dt = torch.uint8 if dtype == np.uint8 else torch.int16
    # + 4 spare bytes behind a uint8 ring, as the triggered tests keep them
    flat = torch.zeros(S * cap_len * M + (4 if dt == torch.uint8 else 0), dtype=dt, device="cuda")
    ring = flat[:S * cap_len * M].view(S, cap_len, M)
    kw = dict(mode="continuous", activity_var=0) if mode == "continuous" else {}
    return StreamPipeline(lc, ring, hop=hop, use_graph=use_graph, **kw)


def _produce(pipe, src, h, hop):
    """The producer: hop h's samples (0-based) into the ring's rows t mod capture_len."""
    with torch.cuda.stream(pipe.stream):
        idx = torch.arange(h * hop, (h + 1) * hop, device="cuda") % pipe.capture_len
        pipe.capture[:, idx] = src[:, h * hop:(h + 1) * hop]


def _targets(mics, seed):
    """xy [S][KT][2] and count [S]: a NaN, a short count and a count of 0 among random targets."""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-BC.GRID, BC.GRID, (S, KT, 2)).astype(np.float32)
    xy[0, 0] = mics[0]
    xy[1, 1] = (0.3, np.nan)
    count = np.array([KT, KT, KT - 1, 0, KT], np.int32)
    return xy, count


def _fill(pipe, o):
    with torch.cuda.stream(pipe.stream):
        for t in o.values():
            t.view(torch.uint8).fill_(SENT)


@pytest.mark.parametrize("engine,mode,dtype,M,N,hop,cap_len", STREAM_CASES)
def test_stream_beam_equals_reference(engine, mode, dtype, M, N, hop, cap_len):
    lc = _loc(M, N, engine, "pcm16" if dtype == np.int16 else "adc8")
    bg, mics, fs, c = _geom(lc)
    A, D = R.latency(mics, fs, c)
    assert cap_len >= 2 * hop + A + D + 16 and cap_len < HOPS * hop
    # the alignment class the case claims: a stream's ring is a multiple of 16 bytes, or it is not
    assert ((cap_len * M * np.dtype(dtype).itemsize) % 16 == 0) == ((dtype, M, cap_len) in RING_16)
    hist = BC.history(S, HOPS * hop, M, dtype, 7 * M + hop)
    src = torch.from_numpy(hist).cuda()
    xy, count = _targets(mics, hop)
    valid = np.arange(KT)[None, :] < count[:, None]
    d_xy, d_cnt = torch.from_numpy(xy).cuda(), torch.from_numpy(count).cuda()
    # one long reference run: the block form on the whole history, from n = -A on
    long_ref = R.beam(mics, fs, c, BC.H, np.concatenate([np.zeros((S, M, A), hist.dtype),
                                                         hist.transpose(0, 2, 1)], axis=2), xy, count)
    runs = {}
    for use_graph in (False, True):
        pipe = _pipe(lc, cap_len, dtype, hop, mode, use_graph)
        if (M, N) in LONG_FRAME:
            assert hop == LONG_FRAME[(M, N)] and pipe.kernel == "k_f16_ring"
        # before any step: TDOA_OK, nothing is launched
        o = pipe.beam(d_xy, d_cnt)
        assert o["audio"].shape == (S, KT, hop) and o["delays"].shape == (S, KT, M) and o["active"].shape == (S, KT)
        _fill(pipe, o)
        assert pipe.beam(d_xy, d_cnt) is o
        pipe.stream.synchronize()
        assert all((v.cpu().numpy().view(np.uint8) == SENT).all() for v in o.values())
        blocks = []
        wrapped = 0
        for h in range(1, HOPS + 1):
            _produce(pipe, src, h - 1, hop)
            pipe.step()
            _fill(pipe, o)
            assert pipe.beam(d_xy, d_cnt) is o
            pipe.stream.synchronize()
            g = {k: v.cpu().numpy() for k, v in o.items()}
            n0, ref = BC.stream_ref(mics, fs, c, hist, xy, valid, hop, h)
            assert int(g["block_start"][0]) == n0 == h * hop - hop - A, (h, g["block_start"])
            assert g["delays"].tobytes() == ref["delays"].tobytes() and g["active"].tobytes() == ref["active"].tobytes()
            assert R.close(g["audio"], ref, M), (h, R.worst(g["audio"], ref, M))
            assert (g["audio"][ref["active"] == 0] == 0).all()
            blocks.append(g["audio"])
            lo = (n0 - 7) % cap_len
            wrapped += lo + hop + D + 15 > cap_len and n0 - 7 >= 0
        assert wrapped >= 1  # a staged run crossed the ring's end
        assert np.abs(blocks[0]).max() > 0  # hop 1's block, which starts at -A, already carries signal
        # the blocks abut: their concatenation is the long run
        cat = np.concatenate(blocks, axis=2)
        sl = slice(0, HOPS * hop)
        long_cut = {k: long_ref[k][:, :, sl] for k in ("audio", "mag")}
        assert R.close(cat, long_cut, M), R.worst(cat, long_cut, M)
        runs[use_graph] = cat
        pipe.close()
    assert runs[False].tobytes() == runs[True].tobytes()  # graph and stream launches: the same bits
    lc.close()


@pytest.mark.parametrize("engine,mode,fmt", [("direct", "triggered", "adc8"), ("gcc_phat", "continuous", "pcm16")])
def test_stream_beam_follows_the_track_table(engine, mode, fmt):
    """step -> peaks -> track -> beam(): channel k is track slot k, steered at
    the position tracks_all() reports, silent below min_status."""
    N, hop, M = 1024, 512, 3
    lc = _loc(M, N, engine, fmt)
    bg, mics, fs, c = _geom(lc)
    lut = lc.lut()
    if fmt == "pcm16":
        hist = synth.pcm16_stream(S, hop * HOPS, M, lut, lc.dims.S, 41, burst_len=3000, gap=(3500, 4500)).numpy()
    else:
        hist = synth.adc_stream(S, hop * HOPS, M, lut, lc.dims.S, 29, burst_len=500, gap=(1100, 1600)).numpy()
    kw = dict(mode="continuous", activity_var=Cs.SMALL_VAR["pcm16"]) if mode == "continuous" else {}
    pipe = StreamPipeline(lc, torch.from_numpy(hist).cuda(), hop=hop, **kw)
    with pytest.raises(tdoa.TdoaError, match="track table"):
        pipe.beam()  # no tdoa_stream_track yet
    prm = dict(max_tracks=4, confirm_hits=2, max_misses=3)
    seen = {1: 0, 2: 0}
    silent = 0
    for h in range(1, HOPS + 1):
        pipe.step()
        pipe.peaks(num_peaks=3, ls=True)
        pipe.track(**prm)
        tr, _ = pipe.tracks_all()
        for min_status, Kt in ((1, 4), (2, 8)):
            o = pipe.beam(num_targets=Kt, min_status=min_status)
            _fill(pipe, o)
            assert pipe.beam(num_targets=Kt, min_status=min_status) is o
            pipe.stream.synchronize()
            g = {k: v.cpu().numpy() for k, v in o.items()}
            txy = np.stack([tr["x"][:, :Kt], tr["y"][:, :Kt]], axis=-1).astype(np.float32)
            n0, ref = BC.stream_ref(mics, fs, c, hist, txy, tr["status"][:, :Kt] >= min_status, hop, h)
            assert int(g["block_start"][0]) == n0
            assert g["delays"].tobytes() == ref["delays"].tobytes() and g["active"].tobytes() == ref["active"].tobytes()
            assert R.close(g["audio"], ref, M), (h, R.worst(g["audio"], ref, M))
            assert (g["audio"][ref["active"] == 0] == 0).all()
            seen[min_status] += int(ref["active"].sum())
            silent += int(((tr["status"][:, :Kt] > 0) & (tr["status"][:, :Kt] < min_status)).sum())
    # the run shows every kind: tentative and confirmed tracks heard, and a tentative one silent at min_status 2
    assert seen[1] > seen[2] >= 1 and silent >= 1, (seen, silent)
    pipe.close()
    lc.close()


def test_hop_outputs_are_the_same_with_and_without_beam():
    """The call changes no existing output: every hop's records and the final
    state of two runs on one capture, one of them calling beam() per hop."""
    N, hop, M = 1024, 512, 3
    lc = _loc(M, N, "gcc_phat")
    hist = synth.adc_stream(S, hop * HOPS, M, lc.lut(), lc.dims.S, 29, burst_len=500, gap=(1100, 1600)).numpy()
    xy = torch.zeros((S, 2, 2), dtype=torch.float32, device="cuda")
    got = {}
    for with_beam in (False, True):
        pipe = StreamPipeline(lc, torch.from_numpy(hist).cuda(), hop=hop)
        recs = []
        for h in range(HOPS):
            pipe.step()
            pipe.peaks(num_peaks=2, ls=True)
            pipe.track()
            if with_beam:
                pipe.beam(xy)
                pipe.beam(min_status=1)
            # (slot order is arbitrary: the records sorted by stream)
            for r in (pipe.records(), pipe.peak_records(), pipe.track_records()):
                recs.append(b"".join(np.ascontiguousarray(r[k]).tobytes() for k in sorted(r)))
        pos, est, last = pipe.state()
        tr, nid = pipe.tracks_all()
        got[with_beam] = (recs, pos, est.tobytes(), last.tobytes(), pipe.totals(), tr.tobytes(), nid.tobytes())
        pipe.close()
    assert got[False] == got[True] and got[True][4][1] >= 5
    lc.close()


def test_stream_beam_errors():
    L = _lib.load()
    # two mics a metre apart: Dmax = 141, so a 256-sample frame's smallest ring is too short for the beam
    lc = _loc(2, 256, mics=np.array([[-0.5, 0], [0.5, 0]], np.float32))
    A, D = lc.beam_latency()
    hop, cap_len = 64, 256 + 2 * 64
    assert cap_len < 2 * hop + A + D + 16
    ring = torch.zeros((S, cap_len, 2), dtype=torch.uint8, device="cuda")
    pipe = StreamPipeline(lc, ring, hop=hop)
    xy = torch.zeros((S, 2, 2), dtype=torch.float32, device="cuda")
    with pytest.raises(tdoa.TdoaError, match="capture_len"):
        pipe.beam(xy)
    pipe.close()
    lc.close()
    lc = _loc(3, 256)
    pipe = StreamPipeline(lc, torch.zeros((S, 1024, 3), dtype=torch.uint8, device="cuda"), hop=64)
    pipe.step()
    audio = torch.full((S, 2, 64), 7.0, device="cuda")
    out, none = _lib.BeamOutputs(audio.data_ptr(), None, None, None), _lib.BeamOutputs()
    st = C.c_void_p(pipe.stream.cuda_stream)
    p = C.c_void_p(xy.data_ptr())
    for args, word in (((pipe._h, None, p, 2, 2, None, st), b"NULL"), ((pipe._h, None, p, 2, 2, C.byref(none), st), b"audio"),
                       ((pipe._h, None, p, 0, 2, C.byref(out), st), b"Kt"), ((pipe._h, None, p, 9, 2, C.byref(out), st), b"Kt"),
                       ((pipe._h, None, None, 2, 2, C.byref(out), st), b"track table")):
        assert L.tdoa_stream_beam(*args) == -1 and word in L.tdoa_last_error(), word
    pipe.stream.synchronize()
    assert (audio == 7.0).all()
    pipe.close()
    lc.close()
