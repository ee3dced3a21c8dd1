"""The null-steering beamformer on the device (k_sep: tdoa_sep_batch,
Localizer.sep_batch; over the capture rings: tdoa_stream_sep,
StreamPipeline.sep).

The delay codes, the active bytes and block_start must equal the float64
restatement of the rule (tests/sep_ref.py) exactly.  The audio is compared per
(row, target) by relative L2 error against that reference; the bound is 8 times
the error of a complex64 numpy restatement of the same rule on the same row
(tests/sep_cases.py says why, and never reads the kernel's output).  Every
figure is printed before it is asserted.  Outputs are pre-filled with a
sentinel; what a call must not write must still hold it.

The streaming runs are rows of STREAM_CASES / TRACK_CASES: each names the
paths of k_sep it is there for (PATHS) and asserts the arithmetic that puts it
on them; test_stream_cases_reach_every_path asserts what the rows cover
together.  No run skips a stream, a target or a hop.
"""
import ctypes as C
from typing import NamedTuple

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import beam_ref as R  # noqa: E402
import mic_count_cases as MicCs  # noqa: E402
import sep_cases as SC  # noqa: E402
import sep_ref as S  # noqa: E402
import stream_long_cases as LongCs  # noqa: E402
import tdoa  # noqa: E402
from tdoa import _lib  # noqa: E402
from tdoa.localizer import Localizer  # noqa: E402
from tdoa.stream import StreamPipeline  # noqa: E402

SENT = 0x5A
FS, H = SC.FS, SC.H


def _loc(M, N=256, engine="gcc_phat", fmt="adc8", fs=FS, mics=None):
    return Localizer(engine=engine, num_mics=M, frame_len=N, sample_rate_hz=fs,
                     mic_xy=SC.MICS[M] if mics is None else mics, sample_format=fmt)


def _geom(lc):
    bg = lc.beam_geometry()
    M = lc.dims.M
    mics = np.array(list(bg.mic_xy), np.float32).reshape(8, 2)[:M].copy()
    return mics, bg.sample_rate_hz, bg.speed_of_sound


_locs = {}


@pytest.fixture(scope="module")
def locs():
    yield lambda M: _locs.setdefault(M, _loc(M))
    for lc in _locs.values():
        lc.close()
    _locs.clear()


def _run_block(lc, frames, xy, count, loading=S.LOADING, use=("audio", "delays", "active")):
    B, M, L = frames.shape
    Kt = xy.shape[1]
    outs = {"audio": torch.empty((B, Kt, L), dtype=torch.float32, device="cuda"),
            "delays": torch.empty((B, Kt, M), dtype=torch.int32, device="cuda"),
            "active": torch.empty((B, Kt), dtype=torch.uint8, device="cuda")}
    for v in outs.values():
        v.view(torch.uint8).fill_(SENT)
    d = [torch.from_numpy(a).cuda() for a in (frames, xy)]
    d_cnt = None if count is None else torch.from_numpy(count).cuda()
    got = lc.sep_batch(d[0], d[1], d_cnt, loading=loading, outputs={k: outs[k] for k in use})
    torch.cuda.synchronize()
    assert set(got) == set(use) and lc.sep_block() == L
    return {k: v.cpu().numpy() for k, v in outs.items()}


def _check_block(lc, frames, xy, count, loading=S.LOADING, use=("audio", "delays", "active"), label=""):
    mics, fs, c = _geom(lc)
    ref = S.sep(mics, fs, c, H, frames, xy, count, loading)
    ok = ref["active"] != 0
    tol, rerr = SC.tolerance(frames, ref["delays"], ok, ref["audio"], loading)
    g = _run_block(lc, frames, xy, count, loading, use)
    err = S.rel_l2(g["audio"], ref["audio"])
    print(f"{label} M {frames.shape[1]} L {frames.shape[2]} Kt {xy.shape[1]}: restatement's worst error "
          f"{rerr.max():.3g}, k_sep's worst error {err.max():.3g}, worst error / bound {np.max(err / np.maximum(tol, 1e-300)):.3g}")
    for k in ("delays", "active"):
        if k in use:
            assert g[k].tobytes() == ref[k].tobytes(), k
        else:
            assert (g[k].view(np.uint8) == SENT).all(), f"{k} written without being passed"
    assert np.isfinite(g["audio"]).all()
    assert (g["audio"][~ok] == 0).all()
    assert (err <= tol).all(), (err, tol)
    return ref, g


# ---------------------------------------------------------------- the block form
@pytest.mark.parametrize("M,L,Kt", SC.BLOCK_SHAPES)
def test_block_form_equals_the_reference(locs, M, L, Kt):
    lc = locs(M)
    mics, fs, c = _geom(lc)
    assert S.block_ok(L, R.dmax(mics, fs, c))
    frames, xy, count = SC.block_case(mics, 5, L, Kt, 1000 + M + L + Kt)
    if (M, L, Kt) == (3, 256, 4):
        assert count.tolist() == [0, 1, 3, 4, 4]
    ref, _ = _check_block(lc, frames, xy, count, label="count")
    assert ref["active"].any() and not ref["active"].all()
    _check_block(lc, frames, xy, None, use=("audio",), label="all  ")
    _check_block(lc, frames, xy, count, loading=1e-4, use=("audio", "active"), label="d1e-4")
    _check_block(lc, frames, xy, count, loading=1e4, label="d1e4 ")


def test_block_form_one_row_and_the_lds_maximum(locs):
    lc = locs(3)
    mics, _, _ = _geom(lc)
    frames, xy, _ = SC.block_case(mics, 1, 128, 2, 77)
    _check_block(lc, frames, xy, None, label="B = 1")
    lc = locs(8)
    mics, _, _ = _geom(lc)
    M, L, Kt = SC.LDS_MAX_SHAPE
    frames, xy, _ = SC.block_case(mics, 1, L, Kt, 78)
    _check_block(lc, frames, xy, None, label="LDS max")
    # and B = 0: nothing is launched, nothing is needed
    out = lc.sep_batch(torch.zeros((0, 8, L), dtype=torch.int16, device="cuda"),
                       torch.zeros((0, Kt, 2), dtype=torch.float32, device="cuda"))
    assert out["audio"].shape == (0, Kt, L)


def test_block_form_non_finite_and_coincident_targets(locs):
    lc = locs(3)
    mics, _, _ = _geom(lc)
    frames, xy, _ = SC.block_case(mics, 3, 256, 3, 79)
    xy[0, 1] = (np.nan, 0.5)
    xy[1, 0] = (0.2, np.inf)
    xy[2] = np.nan
    ref, g = _check_block(lc, frames, xy, None, label="non-finite")
    assert ref["active"].tolist() == [[1, 0, 1], [0, 1, 1], [0, 0, 0]] and (g["delays"][2] == -1).all()
    # two targets at one point: the loading alone keeps G definite; compared at loading = 1
    xy2 = np.array([[[0.4, 0.6], [0.4, 0.6], [-1.0, 0.3]]] * 2, np.float32)
    xy2[1, 2] = xy2[1, 0]
    _check_block(lc, frames[:2], xy2, None, loading=1.0, label="coincident")
    # at the default loading the result stays finite (no comparison: the issue sets it at loading = 1)
    g = _run_block(lc, frames[:2], xy2, None)
    assert np.isfinite(g["audio"]).all()


# ---------------------------------------------------------------- the streaming form
NS, HOP, HOPS, KT = 5, 64, 10, 3  # of the first four cases, and the defaults of the others


class Case(NamedTuple):
    """One streaming run: the pipeline (engine, mode, ring type, mics, frame_len
    N, sample rate, geometry), the ring (capture_len samples per stream, ns
    streams), the separator's call (hop, Kt) over `hops` hops, whether a
    stream's ring is a multiple of 16 bytes, and the paths of k_sep the case is
    there for (PATHS below: each is asserted of the case that names it)."""
    engine: str
    mode: str
    dtype: type
    M: int
    cap_len: int
    aligned: bool
    N: int = 256
    hop: int = HOP
    ns: int = NS
    hops: int = HOPS
    kt: int = KT
    fs: int = FS
    mics: object = None  # None: SC.MICS[M]
    paths: tuple = ()

    @property
    def L(self):
        return 2 * self.hop

    @property
    def ring_bytes(self):
        return self.cap_len * self.M * np.dtype(self.dtype).itemsize

    @property
    def lds(self):
        """k_sep's dynamic LDS: the 256-byte head and max(ceil(M / 2), ceil(Kt / 2)) buffers of L complex points."""
        return 256 + (max(self.M, self.kt) + 1) // 2 * self.L * 8

    def loc(self):
        return _loc(self.M, self.N, self.engine, "pcm16" if self.dtype == np.int16 else "adc8", self.fs,
                    SC.MICS[self.M] if self.mics is None else self.mics)


TPB = 256  # k_sep's workgroup
# what a case forces k_sep through, as arithmetic on the case alone
PATHS = {
    # a thread owns bins k, k + 256, .. of [0, hop] and their mirrors
    "bins in several passes": lambda c: c.hop >= TPB,
    # the overlap-add's items i = tid, tid + 256, .. < Kt hop end inside a pass
    "overlap-add in several passes, the last partial": lambda c: c.kt * c.hop > TPB and c.kt * c.hop % TPB != 0,
    # launch<ring_loader<T>, KT> raises its own instantiation's dynamic LDS limit
    "LDS above 64 KiB": lambda c: c.lds > 64 * 1024 and c.M in (7, 8) and c.hop == 1024 and c.kt == 4,
    # the 8 x 2048 GCC_PHAT pipeline (k_f16_ring), the only one of 8 mics whose hop may be 1024
    "long-frame pipeline": lambda c: (c.engine, c.M, c.N, c.hop) == ("gcc_phat", 8, 2048, 1024),
    # a 16-byte vector of the ring holds a whole number of sample rows: eight (u8) or four (int16) of 2 mics,
    # two or one of 8
    "whole rows per vector": lambda c: 16 // np.dtype(c.dtype).itemsize % c.M == 0,
    # ... or no whole number: the walk over (l, m) turns inside a vector at a different place in each
    "rows turn inside a vector": lambda c: 16 // np.dtype(c.dtype).itemsize % c.M != 0,
}

MICS4 = SC.circle(4, 0.1)  # Dmax = 11 at 16 kHz: L = 128 >= 8 Dmax
# The first four: hop 64, capture_len >= frame_len + 2 hop = 384 and shorter than the 10 hops.  385 * 3 elements
# per stream are no multiple of 16 bytes in either type: most streams' rows take element loads alone.  392 * 4
# elements are 1568 and 3136 bytes: every stream's ring starts 16-byte aligned and the 16-byte vectors carry the
# block, up to the seam at the ring's end.
# The others: every other block length (hop 128 .. 1024), the mic counts 2, 5, 7 and 8, each ring type with
# rings that are and are not multiples of 16 bytes, and the smallest streams x hops that still wrap the ring
# and see the count change.  The 5-, 7- and 8-mic pipelines are those of tests/mic_count_cases.py and
# tests/stream_long_cases.py (48 kHz, circles of radius 0.15 m: Dmax = 41 .. 43, 8 Dmax <= 512).
CAP_LEN = 385
LONG8 = dict(N=2048, hop=1024, ns=3, hops=5, kt=4, fs=LongCs.FS, mics=LongCs.MICS[8],
             paths=("bins in several passes", "LDS above 64 KiB", "long-frame pipeline", "whole rows per vector"))
STREAM_CASES = [
    pytest.param(Case("direct", "triggered", np.uint8, 3, CAP_LEN, False, paths=("rows turn inside a vector",)),
                 id="direct-triggered-uint8"),
    pytest.param(Case("gcc_phat", "continuous", np.int16, 3, CAP_LEN, False), id="gcc_phat-continuous-int16"),
    pytest.param(Case("direct", "triggered", np.uint8, 4, 392, True, mics=MICS4, paths=("whole rows per vector",)),
                 id="direct-triggered-uint8-392x4"),
    pytest.param(Case("gcc_phat", "continuous", np.int16, 4, 392, True, mics=MICS4),
                 id="gcc_phat-continuous-int16-392x4"),
    # 515 * 3 = 1545 bytes
    pytest.param(Case("direct", "triggered", np.uint8, 3, 515, False, hop=128, hops=8,
                      paths=("overlap-add in several passes, the last partial",)), id="uint8-3x515-hop128"),
    # 1544 * 5 * 2 = 15440 = 965 * 16 bytes
    pytest.param(Case("gcc_phat", "continuous", np.int16, 5, 1544, True, N=1024, hop=256, ns=4, hops=8, kt=4,
                      fs=MicCs.FS_STREAM, mics=MicCs.mics(5),
                      paths=("bins in several passes", "rows turn inside a vector")), id="int16-5x1544-hop256"),
    # 2051 * 7 * 2 = 28714 = 1794 * 16 + 10 bytes
    pytest.param(Case("gcc_phat", "continuous", np.int16, 7, 2051, False, N=1024, hop=512, ns=3, hops=6, kt=2,
                      fs=MicCs.FS_STREAM, mics=MicCs.mics(7),
                      paths=("bins in several passes", "rows turn inside a vector")), id="int16-7x2051-hop512"),
    # 4098 * 8 = 2049 * 16 bytes, and twice that
    pytest.param(Case("gcc_phat", "triggered", np.uint8, 8, 4098, True, **LONG8), id="uint8-8x4098-hop1024"),
    pytest.param(Case("gcc_phat", "continuous", np.int16, 8, 4098, True, **LONG8), id="int16-8x4098-hop1024"),
    # 392 * 2 = 784 = 49 * 16 bytes
    pytest.param(Case("direct", "triggered", np.uint8, 2, 392, True, kt=4, paths=("whole rows per vector",)),
                 id="uint8-2x392-hop64"),
]


def test_stream_cases_reach_every_path():
    """What the streaming cases cover together, on their parameters alone."""
    cases = [p.values[0] for p in STREAM_CASES]
    assert {c.hop for c in cases} == {64, 128, 256, 512, 1024}
    assert {c.M for c in cases} >= {2, 5, 7, 8}
    for name in PATHS:
        assert any(name in c.paths for c in cases), name
    for dtype in (np.uint8, np.int16):
        mine = [c for c in cases if c.dtype == dtype]
        assert {c.aligned for c in mine} == {False, True}
        assert any("LDS above 64 KiB" in c.paths for c in mine)  # one instantiation per ring type
    for c in cases:
        assert (c.ring_bytes % 16 == 0) == c.aligned
        assert c.hops * c.hop > c.cap_len >= max(c.N + 2 * c.hop, 3 * c.hop)
        assert c.ns >= 3 and c.kt >= 2  # the streams with the count change, the NaN and the short count


def _history(ns, T, M, dtype, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(T)[None, :, None]
    f = rng.uniform(0.01, 0.2, (ns, 1, M))
    ph = rng.uniform(0, 2 * np.pi, (ns, 1, M))
    x = np.sin(2 * np.pi * f * t + ph) + 0.5 * rng.normal(0, 1, (ns, T, M))
    if np.dtype(dtype) == np.uint8:
        return np.clip(np.rint(128 + 50 * x), 0, 255).astype(np.uint8)
    return np.clip(np.rint(8000 * x), -32767, 32767).astype(np.int16)


def _pipe(lc, dtype, mode, use_graph=True, cap_len=CAP_LEN, ns=NS, hop=HOP):
    M = lc.dims.M
    dt = torch.uint8 if dtype == np.uint8 else torch.int16
    flat = torch.zeros(ns * cap_len * M + (4 if dt == torch.uint8 else 0), dtype=dt, device="cuda")
    ring = flat[:ns * cap_len * M].view(ns, cap_len, M)
    kw = dict(mode="continuous", activity_var=0) if mode == "continuous" else {}
    return StreamPipeline(lc, ring, hop=hop, use_graph=use_graph, **kw)


def _produce(pipe, src, h):
    """Hop h's samples (0-based) into the ring's rows t mod capture_len."""
    hop = pipe.hop
    with torch.cuda.stream(pipe.stream):
        idx = torch.arange(h * hop, (h + 1) * hop, device="cuda") % pipe.capture_len
        pipe.capture[:, idx] = src[:, h * hop:(h + 1) * hop]


def _fill(pipe, o):
    with torch.cuda.stream(pipe.stream):
        for t in o.values():
            t.view(torch.uint8).fill_(SENT)


def _refs(mics, fs, c, hist, Kt, loading=S.LOADING, hop=HOP):
    """The float64 reference stream and the complex64 restatement of it."""
    return (S.Stream(mics, fs, c, H, hist, hop, Kt, loading),
            S.Stream(mics, fs, c, H, hist, hop, Kt, loading, block_fn=SC.restate, dtype=np.float32))


def _check_hop(g, want, restated, label, worst=None):
    """One hop against the reference; `worst` gathers the run's three figures:
    the restatement's worst error, k_sep's, and k_sep's worst error over its bound."""
    n0, audio, codes, ok = want
    assert int(g["block_start"][0]) == n0, (label, g["block_start"])
    assert g["delays"].tobytes() == codes.tobytes() and g["active"].tobytes() == ok.tobytes(), label
    tol = SC.MARGIN * S.rel_l2(restated[1], audio)
    err = S.rel_l2(g["audio"], audio)
    ratio = np.max(err / np.maximum(tol, 1e-300))
    print(f"{label}: restatement's worst error {tol.max() / SC.MARGIN:.3g}, k_sep's {err.max():.3g}, "
          f"worst error / bound {ratio:.3g}")
    if worst is not None:
        worst[:] = np.maximum(worst, [tol.max() / SC.MARGIN, err.max(), ratio])
    assert np.isfinite(g["audio"]).all() and (err <= tol).all(), (label, err, tol)
    return tol


def _assert_paths(case, mics, fs, c):
    """The case is what its row of STREAM_CASES claims: the ring's alignment class and every path it names."""
    assert S.block_ok(case.L, R.dmax(mics, fs, c))
    assert (case.ring_bytes % 16 == 0) == case.aligned
    assert case.cap_len < case.hops * case.hop and case.cap_len >= 3 * case.hop
    for name in case.paths:
        assert PATHS[name](case), name


@pytest.mark.parametrize("case", STREAM_CASES)
def test_stream_sep_with_explicit_targets(case):
    dtype, M, cap_len, ns, hop, hops, Kt = case.dtype, case.M, case.cap_len, case.ns, case.hop, case.hops, case.kt
    lc = case.loc()
    mics, fs, c = _geom(lc)
    _assert_paths(case, mics, fs, c)
    hist = _history(ns, hops * hop, M, dtype, 5 + np.dtype(dtype).itemsize)
    src = torch.from_numpy(hist).cuda()
    rng = np.random.default_rng(17)
    xy = rng.uniform(-SC.GRID, SC.GRID, (ns, Kt, 2)).astype(np.float32)
    xy[1, 1] = (0.3, np.nan)
    # stream 0: full, then one target (below); 1: a NaN; 2: a short count; 3: none; 4: full
    count = np.array([Kt, Kt, Kt - 1, 0, Kt][:ns], np.int32)
    d_xy, d_cnt = torch.from_numpy(xy).cuda(), torch.from_numpy(count).cuda()
    ref, c64 = _refs(mics, fs, c, hist, Kt, hop=hop)
    pipe = _pipe(lc, dtype, case.mode, cap_len=cap_len, ns=ns, hop=hop)
    if "long-frame pipeline" in case.paths:
        assert pipe.kernel == "k_f16_ring"
    assert pipe.capture.data_ptr() % 16 == 0  # (with the stride, what lets the aligned rings take vectors)
    # before any step: TDOA_OK, nothing is launched
    o = pipe.sep(d_xy, d_cnt)
    assert o["audio"].shape == (ns, Kt, hop) and o["delays"].shape == (ns, Kt, M) and o["active"].shape == (ns, Kt)
    _fill(pipe, o)
    assert pipe.sep(d_xy, d_cnt) is o
    pipe.stream.synchronize()
    assert all((v.cpu().numpy().view(np.uint8) == SENT).all() for v in o.values())
    blocks, tols, wrapped = [], [], 0
    worst = np.zeros(3)
    change = hops // 2 + 1  # (hop 6 of 10)
    assert change + 1 <= hops
    for h in range(1, hops + 1):
        if h == change:  # stream 0's slots from 1 on turn invalid: zeros from this block on
            count[0] = 1
            d_cnt = torch.from_numpy(count).cuda()
        _produce(pipe, src, h - 1)
        pipe.step()
        _fill(pipe, o)
        assert pipe.sep(d_xy, d_cnt) is o
        pipe.stream.synchronize()
        g = {k: v.cpu().numpy() for k, v in o.items()}
        want, rest = ref.step(h * hop, xy, count), c64.step(h * hop, xy, count)
        assert want[0] == h * hop - 2 * hop
        tols.append(_check_hop(g, want, rest, f"hop {h}", worst))
        if ns > 3:
            assert (g["audio"][3] == 0).all()  # count 0 from the start: no tail either
        if h == change:
            assert np.abs(g["audio"][0, 1:]).max() > 0  # the block is zeros: what is heard is the old tail
        if h > change:
            assert (g["audio"][0, 1:] == 0).all()  # invalid for two blocks: block and tail are zeros
        blocks.append(g["audio"])
        lo = (h * hop - 2 * hop) % cap_len
        wrapped += h >= 2 and lo + 2 * hop > cap_len
    assert wrapped >= 1  # a staged block crossed the ring's end
    # the blocks abut: their concatenation is the overlap-add of the block form over the history.  Where
    # every block has both its neighbours, [hop, T - 2 hop), its relative error is at most the largest of
    # the hops' bounds (the squared errors add, each below its hop's bound times that hop's reference).
    cat = np.concatenate(blocks, axis=2)[:, :, hop:]  # from sample 0 on (the first block starts at -hop)
    T = hops * hop
    cut = slice(hop, T - 2 * hop)
    for s in [s for s in (1, 4) if s < ns]:  # the streams whose targets never change
        codes, ok = S.targets(mics, fs, c, H, xy[s][None], count[s:s + 1])
        fr = np.stack([hist[s, i * hop:i * hop + 2 * hop].T for i in range(hops - 1)])
        whole = S.ola(np.stack([S.block(fr[b], codes[0], ok[0]) for b in range(hops - 1)]))
        err = S.rel_l2(cat[s][ok[0]][:, cut], whole[ok[0]][:, cut])
        bound = np.max([t[s] for t in tols], axis=0)[ok[0]]
        print(f"stream {s}: the concatenated blocks against the overlap-added block form: {err}, bound {bound}")
        assert (err <= bound).all()
    # a call with another Kt starts the overlap-add afresh: its first block has no tail
    K2 = Kt - 1
    o2 = pipe.sep(d_xy[:, :K2].contiguous(), None)
    pipe.stream.synchronize()
    fresh = S.Stream(mics, fs, c, H, hist, hop, K2)
    f64 = fresh.step(hops * hop, xy[:, :K2])
    f32 = S.Stream(mics, fs, c, H, hist, hop, K2, block_fn=SC.restate, dtype=np.float32).step(hops * hop, xy[:, :K2])
    _check_hop({k: v.cpu().numpy() for k, v in o2.items()}, f64, f32, f"Kt {Kt} -> {K2}", worst)
    print(f"stream case M {M} L {2 * hop} Kt {Kt} {np.dtype(dtype).name}: restatement's worst error {worst[0]:.3g}, "
          f"k_sep's worst error {worst[1]:.3g}, worst error / bound {worst[2]:.3g}")
    pipe.close()
    lc.close()


@pytest.mark.parametrize("case", STREAM_CASES)
def test_reset_zeroes_the_tails(case):
    dtype, M, cap_len, ns, hop = case.dtype, case.M, case.cap_len, case.ns, case.hop
    lc = case.loc()
    _assert_paths(case, *_geom(lc))
    hist = _history(ns, 4 * hop, M, dtype, 31)
    src = torch.from_numpy(hist).cuda()
    xy = torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, (ns, 2, 2)).astype(np.float32)).cuda()
    first = {}
    for warm in (0, 3):
        pipe = _pipe(lc, dtype, case.mode, cap_len=cap_len, ns=ns, hop=hop)
        for h in range(warm):
            _produce(pipe, src, h + 1)
            pipe.step()
            pipe.sep(xy)
        if warm:
            pipe.reset()
        for h in range(2):
            _produce(pipe, src, h)
            pipe.step()
            o = pipe.sep(xy)
            pipe.stream.synchronize()
            first[(warm, h)] = {k: v.cpu().numpy().copy() for k, v in o.items()}
        pipe.close()
    for h in range(2):
        for k in ("audio", "delays", "active", "block_start"):
            assert first[(0, h)][k].tobytes() == first[(3, h)][k].tobytes(), (h, k)
    assert np.abs(first[(0, 0)]["audio"]).max() > 0 and int(first[(3, 0)]["block_start"][0]) == -hop
    lc.close()


# the third: seven mics' int16 rings (1283 * 7 * 2 bytes, no multiple of 16; the 7 x 512 / 256 pipeline of
# tests/mic_count_cases.py) with the bins in two passes
TRACK_CASES = [
    pytest.param(Case("gcc_phat", "continuous", np.uint8, 3, CAP_LEN, False, kt=4), id="uint8"),
    pytest.param(Case("gcc_phat", "continuous", np.int16, 3, CAP_LEN, False, kt=4), id="int16"),
    pytest.param(Case("gcc_phat", "continuous", np.int16, 7, 1283, False, N=512, hop=256, ns=3, kt=4,
                      fs=MicCs.FS_STREAM, mics=MicCs.mics(7),
                      paths=("bins in several passes", "rows turn inside a vector")), id="int16-7x1283-hop256"),
]


@pytest.mark.parametrize("case", TRACK_CASES)
def test_stream_sep_follows_the_track_table(case):
    """step -> track -> sep(): channel k is track slot k, steered at the
    position tracks_all() reports, silent below min_status; a track that dies
    leaves its channel the old tail, then zeros."""
    dtype, M, ns, hop, hops = case.dtype, case.M, case.ns, case.hop, case.hops
    assert hops == HOPS and case.kt == 4
    lc = case.loc()
    mics, fs, c = _geom(lc)
    _assert_paths(case, mics, fs, c)
    hist = _history(ns, hops * hop, M, dtype, 41)
    src = torch.from_numpy(hist).cuda()
    pipe = _pipe(lc, dtype, "continuous", cap_len=case.cap_len, ns=ns, hop=hop)
    with pytest.raises(tdoa.TdoaError, match="track table"):
        pipe.sep()  # no tdoa_stream_track yet
    ref, c64 = _refs(mics, fs, c, hist, 4, hop=hop)
    z = np.array([[0.9, -0.4], [-1.2, 0.8]], np.float32)
    meas = {"xy": torch.from_numpy(np.broadcast_to(z, (ns, 2, 2)).copy()).cuda(),
            "count": torch.full((ns,), 2, dtype=torch.int32, device="cuda")}
    seen = died = 0
    was = np.zeros((ns, 4), bool)
    worst = np.zeros(3)
    for h in range(1, hops + 1):
        if h == 7:  # the second source falls silent: its track misses, then dies
            meas["count"] = torch.full((ns,), 1, dtype=torch.int32, device="cuda")
        _produce(pipe, src, h - 1)
        pipe.step()
        pipe.track(peaks=meas, use_ls=False, max_tracks=4, confirm_hits=2, max_misses=2)
        tr, _ = pipe.tracks_all()
        o = pipe.sep(min_status=2)
        pipe.stream.synchronize()
        assert o["audio"].shape == (ns, 4, hop)
        txy = np.stack([tr["x"][:, :4], tr["y"][:, :4]], axis=-1).astype(np.float32)
        valid = tr["status"][:, :4] >= 2
        want, rest = ref.step(h * hop, txy, valid=valid), c64.step(h * hop, txy, valid=valid)
        _check_hop({k: v.cpu().numpy() for k, v in o.items()}, want, rest, f"hop {h}", worst)
        seen += int(valid.sum())
        died += int((was & ~valid).sum())
        was = valid
    assert seen >= 2 * ns and died >= 1, (seen, died)
    print(f"track case M {M} L {2 * hop} Kt 4 {np.dtype(dtype).name}: restatement's worst error {worst[0]:.3g}, "
          f"k_sep's worst error {worst[1]:.3g}, worst error / bound {worst[2]:.3g}")
    pipe.close()
    lc.close()


# ---------------------------------------------------------------- capability
def test_capability_on_the_device():
    """The two-source scene of test_sep_cpu.py through sep_batch and beam_batch:
    the interferer-to-target ratios are the two references' within 0.5 dB."""
    import test_sep_cpu as TC
    lc = _loc(3, 256, fs=S.SCENE_FS)
    mics, fs, c = _geom(lc)
    L, nb = S.SCENE_L, 40
    parts = S.scene(mics, fs, c, H, nb, L)
    fr = S.scene_frames(parts, L)  # [2][nb][M][L]
    xy = np.broadcast_to(np.array(S.SCENE_POINTS, np.float32), (nb, 2, 2)).copy()
    sep_p, das_p, ref_p = np.zeros((2, 2)), np.zeros((2, 2)), np.zeros((2, 2))
    flat = np.rint(parts).astype(np.int16)[:, :, :nb // 2 * L].reshape(2, 3, nb // 2, L).transpose(0, 2, 1, 3).copy()
    for src in range(2):
        y = lc.sep_batch(torch.from_numpy(fr[src]).cuda(), torch.from_numpy(xy).cuda())["audio"].cpu().numpy()
        y = S.ola(y.astype(np.float64))  # [2][T]
        sep_p[:, src] = (y[:, L:-L] ** 2).mean(axis=1)
        # the delay-and-sum on abutting frames, against its float64 reference on the same frames
        d = lc.beam_batch(torch.from_numpy(flat[src]).cuda(), torch.from_numpy(xy[:nb // 2]).cuda())["audio"]
        das_p[:, src] = (d.cpu().numpy().astype(np.float64) ** 2).mean(axis=(0, 2))
        ref_p[:, src] = (R.beam(mics, fs, c, H, flat[src], xy[:nb // 2])["audio"] ** 2).mean(axis=(0, 2))
    torch.cuda.synchronize()
    sep = [S.ratio_db(sep_p[0, 1], sep_p[0, 0]), S.ratio_db(sep_p[1, 0], sep_p[1, 1])]
    das = [S.ratio_db(das_p[0, 1], das_p[0, 0]), S.ratio_db(das_p[1, 0], das_p[1, 1])]
    dref = [S.ratio_db(ref_p[0, 1], ref_p[0, 0]), S.ratio_db(ref_p[1, 0], ref_p[1, 1])]
    print("interferer-to-target, dB: k_sep", sep, "reference", TC.MEASURED_SEP_DB, "| k_beam", das, "reference", dref,
          "(whole-signal reference", TC.MEASURED_DAS_DB, ")")
    for ch in range(2):
        assert abs(sep[ch] - TC.MEASURED_SEP_DB[ch]) <= 0.5
        assert abs(das[ch] - dref[ch]) <= 0.5
        assert das[ch] - sep[ch] >= 0.5 * (TC.MEASURED_DAS_DB[ch] - TC.MEASURED_SEP_DB[ch])
    lc.close()


# ---------------------------------------------------------------- error paths (host only)
def test_block_form_errors_leave_outputs_untouched(locs):
    lc = locs(3)
    L = _lib.load()
    assert L.tdoa_sep_set_block(lc._ctx, 256) == 0
    fr = torch.zeros((2, 3, 256), dtype=torch.int16, device="cuda")
    xy = torch.zeros((2, 2, 2), dtype=torch.float32, device="cuda")
    audio = torch.full((2, 2, 256), 7.0, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    out, none = _lib.BeamOutputs(audio.data_ptr(), None, None, None), _lib.BeamOutputs()
    d = C.c_float(1e-2)
    for args, word in (((None, p(fr), 2, None, p(xy), 2, d, C.byref(out), None), b"NULL"),
                       ((lc._ctx, None, 2, None, p(xy), 2, d, C.byref(out), None), b"NULL"),
                       ((lc._ctx, p(fr), 2, None, None, 2, d, C.byref(out), None), b"NULL"),
                       ((lc._ctx, p(fr), 2, None, p(xy), 2, d, None, None), b"NULL"),
                       ((lc._ctx, p(fr), 2, None, p(xy), 2, d, C.byref(none), None), b"audio"),
                       ((lc._ctx, p(fr), 2, None, p(xy), 0, d, C.byref(out), None), b"Kt"),
                       ((lc._ctx, p(fr), 2, None, p(xy), 5, d, C.byref(out), None), b"Kt"),
                       ((lc._ctx, p(fr), -1, None, p(xy), 2, d, C.byref(out), None), b"B"),
                       ((lc._ctx, p(fr), 1 << 31, None, p(xy), 2, d, C.byref(out), None), b"B"),
                       ((lc._ctx, p(fr), 2, None, p(xy), 2, C.c_float(0.5e-4), C.byref(out), None), b"loading"),
                       ((lc._ctx, p(fr), 2, None, p(xy), 2, C.c_float(2e4), C.byref(out), None), b"loading"),
                       ((lc._ctx, p(fr), 2, None, p(xy), 2, C.c_float(float("nan")), C.byref(out), None), b"loading")):
        assert L.tdoa_sep_batch(*args) == -1 and word in L.tdoa_last_error(), word
    assert L.tdoa_sep_batch(lc._ctx, p(fr), 0, None, p(xy), 2, d, C.byref(out), None) == 0  # B = 0: no launch
    for bad in (64, 100, 384, 4096):
        assert L.tdoa_sep_set_block(lc._ctx, bad) == -1 and b"power of two" in L.tdoa_last_error()
    assert lc.sep_block() == 256
    torch.cuda.synchronize()
    assert (audio == 7.0).all()
    # the reference triangle at 48 kHz: Dmax = 29, a block of 128 is too short, frame_len 256 is not
    wide = _loc(3, 256, fs=48000)
    assert wide.beam_latency()[1] == 29 and wide.sep_block() == 256
    assert L.tdoa_sep_set_block(wide._ctx, 128) == -1 and b"8 Dmax" in L.tdoa_last_error()
    with pytest.raises(tdoa.TdoaError, match="8 Dmax"):
        wide.sep_batch(torch.zeros((1, 3, 128), dtype=torch.int16, device="cuda"),
                       torch.zeros((1, 1, 2), dtype=torch.float32, device="cuda"))
    wide.close()
    # eight mics on a 0.3 m circle at 48 kHz: Dmax = 43, frame_len 256 is no block length
    none_ctx = _loc(8, 256, fs=48000)
    assert none_ctx.sep_block() == 0
    fr8 = torch.zeros((1, 8, 256), dtype=torch.int16, device="cuda")
    assert L.tdoa_sep_batch(none_ctx._ctx, p(fr8), 1, None, p(xy), 2, d, C.byref(out), None) == -1
    assert b"block length" in L.tdoa_last_error()
    none_ctx.close()
    torch.cuda.synchronize()
    assert (audio == 7.0).all()


def test_stream_sep_errors():
    """Every refusal comes before a device call.  (capture_len < 3 hop cannot
    be reached through the public interface: a pipeline has hop <= frame_len
    and capture_len >= frame_len + 2 hop.)"""
    L = _lib.load()
    xy = torch.zeros((NS, 2, 2), dtype=torch.float32, device="cuda")
    audio = torch.full((NS, 2, 64), 7.0, device="cuda")
    out, none = _lib.BeamOutputs(audio.data_ptr(), None, None, None), _lib.BeamOutputs()
    p = C.c_void_p(xy.data_ptr())
    d = C.c_float(1e-2)
    lc = _loc(3)
    pipe = StreamPipeline(lc, torch.zeros((NS, 1024, 3), dtype=torch.uint8, device="cuda"), hop=64)
    pipe.step()
    st = C.c_void_p(pipe.stream.cuda_stream)
    for args, word in (((None, None, p, 2, 2, d, C.byref(out), st), b"NULL"),
                       ((pipe._h, None, p, 2, 2, d, None, st), b"NULL"),
                       ((pipe._h, None, p, 2, 2, d, C.byref(none), st), b"audio"),
                       ((pipe._h, None, p, 0, 2, d, C.byref(out), st), b"Kt"),
                       ((pipe._h, None, p, 5, 2, d, C.byref(out), st), b"Kt"),
                       ((pipe._h, None, p, 2, 2, C.c_float(1e5), C.byref(out), st), b"loading"),
                       ((pipe._h, None, None, 2, 2, d, C.byref(out), st), b"track table")):
        assert L.tdoa_stream_sep(*args) == -1 and word in L.tdoa_last_error(), word
    with pytest.raises(tdoa.TdoaError, match="Kt"):
        pipe.sep(num_targets=8)
    pipe.close()
    # hop 32: L = 64 is no block length
    pipe = StreamPipeline(lc, torch.zeros((NS, 1024, 3), dtype=torch.uint8, device="cuda"), hop=32)
    pipe.step()
    with pytest.raises(tdoa.TdoaError, match="power of two"):
        pipe.sep(xy)
    pipe.close()
    lc.close()
    # the triangle at 48 kHz: Dmax = 29 and L = 128 < 8 Dmax
    lc = _loc(3, 256, fs=48000)
    pipe = StreamPipeline(lc, torch.zeros((NS, 1024, 3), dtype=torch.uint8, device="cuda"), hop=64)
    pipe.step()
    with pytest.raises(tdoa.TdoaError, match="8 Dmax"):
        pipe.sep(xy)
    pipe.stream.synchronize()
    pipe.close()
    lc.close()
    assert (audio == 7.0).all()
