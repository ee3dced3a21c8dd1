"""Six and seven microphones through every kernel family, against the oracles.

Every layer is dispatched on M or on P = M (M - 1) / 2, and 6 and 7 mics are
where the M-dependent code differs from what the other GPU modules run: the
tuple words of the generic grid solve (P = 15: TW = 4 with 3 pairs in the last
word; P = 21: TW = 6 with 1), k_direct_mfma's 15- and 16-wave workgroups, the
fused-EMA boundary of the DIRECT stream (15 * 89 = 1335 of 1536 slots fits,
21 * 89 = 1869 does not), k_ls / k_ls_stream / k_stream_active at 5, 6 and 7
mics, and k_spec16 / k_pair16 beyond 2 x 4096 and 5 x 2048.

No tolerance is new: DIRECT bit for bit (tests/test_gpu_parity.py), GCC_PHAT
by test_gpu_gcc_phat.check_phat (scores 3e-5, lags where the float64 top-2
margin exceeds 2e-4, cells where the map margin exceeds 1e-3, max_Lf 1e-3),
streams by test_gpu_stream.compare / test_gpu_stream_phat.compare, the
refinement to 1e-5 relative (tests/test_ls.py), the beam within (16 M + 2) 2^-24
of the magnitude sum with equal delay codes (tests/beam_ref.py).  The shapes,
seeds and inputs are tests/mic_count_cases.py; tests/test_mic_counts_cpu.py
checks on the references alone that every lag and at least 90 % of the cells
are compared and that no stream is dropped.  Each route is asserted by name.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import band_ref  # noqa: E402
import beam_cases as BC  # noqa: E402
import beam_ref  # noqa: E402
import gcc_phat_oracle as G  # noqa: E402
import mic_count_cases as MC  # noqa: E402
import pcm16_ref  # noqa: E402
import peaks_ref  # noqa: E402
import stream_cont_cases as Cs  # noqa: E402
import stream_cont_ref  # noqa: E402
import stream_phat_ref  # noqa: E402
import tdoa  # noqa: E402
import test_gpu_beam as TB  # noqa: E402  (near, _geom, _pipe, _produce, _targets, _fill)
import test_gpu_gcc_phat as T  # noqa: E402  (check_phat, _grid_f32)
import test_gpu_peaks as TPK  # noqa: E402  (_check_ls, _ref_args)
import test_gpu_stream as TS  # noqa: E402  (run_pipeline, compare)
import test_gpu_stream_cont as TSC  # noqa: E402  (run_pipeline)
import test_gpu_stream_peaks as TSP  # noqa: E402  (_check_rows, _fill)
import test_gpu_stream_phat as TSF  # noqa: E402  (run_pipeline, compare, assert_bitwise)
import test_gpu_track as TT  # noqa: E402  (_check_hop, _fill)
import test_mic_counts_cpu as CPU  # noqa: E402  (assert_batch_caps)
import track_ref  # noqa: E402
from test_gpu_parity import _cmp  # noqa: E402
from test_ls import TOL as TOL_LS  # noqa: E402
from tdoa.localizer import Localizer  # noqa: E402
from tdoa.stream import StreamPipeline  # noqa: E402

LEAN_KEYS = ("lags", "gate", "cell", "xy", "max_Lf")


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _loc(engine, M, N, fs=MC.FS_BATCH, **kw):
    return Localizer(engine=engine, num_mics=M, frame_len=N, sample_rate_hz=fs, mic_xy=MC.mics(M), **kw)


def _check_ls(oracle, run, raw_key, fs):
    """xy_ls / ls_rms of a scores run against oracle.ls_refine on the run's own raw
    scores, lags and cells (tests/test_ls.py), and the grid=False path bit for bit."""
    got = run["got"]
    uv, rms = oracle.ls_refine(got[raw_key], got["lags"], run["mics"], got["cell"], fs=float(fs))
    err = np.abs(got["xy_ls"] - uv) / np.maximum(1.0, np.abs(uv))
    assert err.max() <= TOL_LS, err.max()
    assert np.abs(got["ls_rms"] - rms).max() <= 1e-4 * max(1.0, rms.max())
    assert (run["ls_only"]["xy_ls"] == got["xy_ls"]).all() and (run["ls_only"]["ls_rms"] == got["ls_rms"]).all()
    assert np.array_equal(run["ls_only"]["lags"], got["lags"])


# ---------------------------------------------------------------- 1. GCC_PHAT batches
PHAT_CASES = ([(M, N, "adc8", False) for M, N in MC.PHAT_SHAPES] + [(M, N, "pcm16", False) for M, N in MC.PHAT_SHAPES]
              + [(M, N, "adc8", True) for M, N in MC.BAND_SHAPES])


@pytest.fixture(scope="module")
def phat_runs(oracle):
    """case -> the context, its batch, the scores / lean / refinement-only runs and
    the float64 reference; made once per case, shared and not modified."""
    made = {}

    def get(M, N, fmt, band):
        key = (M, N, fmt, band)
        if key in made:
            return made[key]
        loc = _loc("gcc_phat", M, N, sample_format=fmt)
        assert loc.dims.S == MC.S_BATCH and loc.dims.P == M * (M - 1) // 2
        lut, win = loc.lut(), loc.window()
        assert (lut == MC.lut_cpu(oracle, M).reshape(lut.shape)).all()
        assert (win == band_ref.window_q15(N)).all()
        if band:
            loc.set_band(*MC.BAND)
            w = loc.bin_weights()
            assert (w == tdoa.band_weights(N, MC.FS_BATCH, *MC.BAND)).all()
        fr_np = (MC.pcm16_batch if fmt == "pcm16" else MC.adc_batch)(lut, M, N)
        fr = torch.from_numpy(fr_np).cuda()
        run = {"loc": loc, "lut": lut, "mics": loc.mics(), "kernel": loc.batch_kernel(), "frames": fr,
               "got": _np(loc.localize(fr, scores=True, ls=True)), "lean": _np(loc.localize(fr)),
               "ls_only": _np(loc.localize(fr, grid=False, ls=True))}
        if band:
            run["exp"] = band_ref.gcc_phat_band(fr_np, MC.S_BATCH, win, w.astype(np.float64), lut)
        elif fmt == "pcm16":
            run["exp"] = pcm16_ref.gcc_phat_pcm16(fr_np, MC.S_BATCH, win, lut)
        else:
            run["exp"] = G.gcc_phat_batch(fr_np, MC.S_BATCH, win, lut)
        made[key] = run
        return run

    yield get
    for run in made.values():
        run["loc"].close()


@pytest.mark.parametrize("M,N,fmt,band", PHAT_CASES)
def test_phat_batch_against_float64(phat_runs, M, N, fmt, band):
    run = phat_runs(M, N, fmt, band)
    assert run["kernel"] == MC.phat_route(N, fmt, band), run["kernel"]
    got, exp = run["got"], run["exp"]
    CPU.assert_batch_caps(exp, (M, N, fmt, band))  # every lag and >= 90 % of the cells are compared below
    print(f"({M}, {N}, {fmt}, band={band}) {run['kernel']}: max |score err| "
          f"{np.abs(got['scores_f'] - exp['scores_f']).max():.2e}, max |max_Lf err| "
          f"{np.abs(got['max_Lf'] - exp['max_Lf']).max():.2e}")
    assert T.check_phat(got, exp) == 1.0
    assert (got["lags"] == exp["lags"]).all() and (got["gate"] == exp["gate"]).all()
    assert np.abs(got["lags"]).max() <= MC.S_BATCH


@pytest.mark.parametrize("M,N,fmt,band", PHAT_CASES)
def test_phat_lean_call_equals_the_scores_call(phat_runs, M, N, fmt, band):
    run = phat_runs(M, N, fmt, band)
    for k in LEAN_KEYS:
        assert np.array_equal(run["lean"][k].view(np.uint8), run["got"][k].view(np.uint8)), k


@pytest.mark.parametrize("M,N,fmt,band", PHAT_CASES)
def test_phat_cell_is_the_exhaustive_scan_of_own_scores(phat_runs, M, N, fmt, band):
    """k_grid_bb / k_grid on P = 15, 21 (and 28) pairs: the cell and max L equal the
    exhaustive float32 scan of the run's own weighted scores bit for bit."""
    run = phat_runs(M, N, fmt, band)
    cell, mx = T._grid_f32(run["got"]["weighted_f"], run["lut"])
    assert (run["got"]["cell"] == cell).all()
    assert (run["got"]["max_Lf"] == mx).all()


@pytest.mark.parametrize("M,N,fmt,band", PHAT_CASES)
def test_phat_least_squares(oracle, phat_runs, M, N, fmt, band):
    _check_ls(oracle, phat_runs(M, N, fmt, band), "scores_f", MC.FS_BATCH)


# ---------------------------------------------------------------- 2. DIRECT batches
@pytest.fixture(scope="module")
def direct_runs(oracle):
    made = {}

    def get(M, N, S_cfg, B):
        key = (M, N, S_cfg, B)
        if key in made:
            return made[key]
        loc = _loc("direct", M, N, max_shift=S_cfg)
        S = loc.dims.S
        assert S == (S_cfg or MC.S_BATCH)
        lut = loc.lut()
        exp_lut = oracle.build_lut(loc.mics(), fs=MC.FS_BATCH, max_shift=S)
        assert (lut == exp_lut.reshape(lut.shape)).all()
        fr_np = MC.direct_batch(exp_lut, M, N, S, B)
        fr = torch.from_numpy(fr_np).cuda()
        made[key] = {"loc": loc, "lut": lut, "mics": loc.mics(), "kernel": loc.batch_kernel(),
                     "got": _np(loc.localize(fr, scores=True, ls=True)), "lean": _np(loc.localize(fr)),
                     "ls_only": _np(loc.localize(fr, grid=False, ls=True)),
                     "exp": oracle.localize_batch(fr_np, S, loc.window(), exp_lut, threads=8)}
        return made[key]

    yield get
    for run in made.values():
        run["loc"].close()


@pytest.mark.parametrize("M,N,S_cfg,B", MC.DIRECT_SHAPES)
def test_direct_batch_bit_for_bit(direct_runs, M, N, S_cfg, B):
    """k_direct_mfma at 15 waves (6 mics) and at 16 waves looping over 21 pairs (7
    mics), its generic grid solve on 4 and 6 tuple words; the full-range tail."""
    run = direct_runs(M, N, S_cfg, B)
    assert run["kernel"] == "k_direct_mfma"
    assert len(run["got"]["lags"]) == B + 8
    _cmp(run["got"], run["exp"])
    _cmp(run["lean"], run["exp"], keys=("lags", "gate", "cell", "max_L", "xy"))


@pytest.mark.parametrize("M,N,S_cfg,B", MC.DIRECT_SHAPES)
def test_direct_least_squares(oracle, direct_runs, M, N, S_cfg, B):
    _check_ls(oracle, direct_runs(M, N, S_cfg, B), "scores", MC.FS_BATCH)


@pytest.mark.parametrize("M", [6, 7])
def test_ema_solve_at_15_and_21_pairs(oracle, M):
    """tdoa_average_batch's grid solve (the int64 k_grid_bb, grouped running maxima
    of the P > 8 bound pass) against the oracle's exhaustive scan, bit for bit:
    random EMA scores (weak bounds) and one stream of all-equal scores (ties)."""
    loc = _loc("direct", M, 256)
    P, K = loc.dims.P, loc.dims.K
    lut = loc.lut().reshape(P, 101, 101)
    Sn, steps = 12, 4
    rng = np.random.default_rng(100 + P)
    est = torch.zeros((Sn, P, K), dtype=torch.int64, device="cuda")
    best = torch.zeros((Sn, P), dtype=torch.int32, device="cuda")
    est_ref = np.zeros((Sn, P, K), np.int64)
    for t in range(steps):
        fresh = rng.integers(-(1 << 40), 1 << 40, (Sn, P, K)).astype(np.int64)
        fresh[0] = 12345  # every tuple ties: the first cell
        dec = rng.uniform(0.05, 1.0, Sn).astype(np.float32)
        solve = {"cell": torch.empty(Sn, dtype=torch.int32, device="cuda"),
                 "max_L": torch.empty(Sn, dtype=torch.int64, device="cuda"),
                 "xy": torch.empty((Sn, 2), dtype=torch.float32, device="cuda")}
        loc.average(est, torch.from_numpy(fresh).cuda(), torch.from_numpy(dec).cuda(), best, solve)
        got_best = best.cpu().numpy()
        for s in range(Sn):
            for p in range(P):
                est_ref[s, p], b = oracle.average(est_ref[s, p], fresh[s, p], float(dec[s]))
                assert got_best[s, p] == b, (t, s, p)
            mL, cell = oracle.grid_solve(est_ref[s], lut)
            assert solve["cell"][s].item() == cell and solve["max_L"][s].item() == mL, (t, s)
        assert solve["cell"][0].item() == 0
        assert (solve["xy"].cpu().numpy() == loc.cell_xy(solve["cell"].cpu().numpy())).all()
        assert (est.cpu().numpy() == est_ref).all()
    loc.close()


# ---------------------------------------------------------------- 3. peaks
@pytest.mark.parametrize("engine,shape", [("direct", MC.DIRECT_SHAPES[0]), ("gcc_phat", (7, 1024, "adc8", False))])
def test_four_peaks_with_refinement(oracle, direct_runs, phat_runs, engine, shape):
    """Localizer.peaks on a run's own raw score block: 6 mics int64, 7 mics float32."""
    run = direct_runs(*shape) if engine == "direct" else phat_runs(*shape)
    loc = run["loc"]
    assert loc.dims.M == (6 if engine == "direct" else 7)
    blk = torch.from_numpy(run["got"]["scores" if engine == "direct" else "scores_f"]).cuda()
    pk = _np(loc.peaks(blk, 4, 8, ls=True))
    exp = peaks_ref.peaks_ref(blk.cpu().numpy(), run["lut"], *TPK._ref_args(loc), 4, 8)
    peaks_ref.assert_equal(pk, exp, (engine, shape))
    assert (pk["count"] == 4).all()
    assert not TPK._check_ls(oracle, loc, blk, pk, fs=float(MC.FS_BATCH)).any()


# ---------------------------------------------------------------- 4. streams
def _stream_loc(engine, M, N, fmt="adc8"):
    loc = _loc(engine, M, N, fs=MC.FS_STREAM, sample_format=fmt)
    assert loc.dims.S == MC.S_STREAM
    return loc


def _kernel(loc, cap, hop, **kw):
    pipe = StreamPipeline(loc, torch.from_numpy(cap[:, :loc.dims.N + 2 * hop]).cuda().contiguous(), hop=hop, **kw)
    name = pipe.kernel
    pipe.close()
    return name


@pytest.mark.parametrize("N,hop,M,seed", MC.TRIGGERED)
def test_direct_stream_bit_for_bit(oracle, N, hop, M, seed):
    """6 mics: the EMA and the grid inside k_direct_mfma (1335 of 1536 slots, a
    partly filled third element per thread); 7 mics: 1869 slots do not fit, the
    fresh scores go through k_stream_update.  Eager and graph."""
    loc = _stream_loc("direct", M, N)
    lut = loc.lut()
    assert (lut == MC.lut_cpu(oracle, M, MC.FS_STREAM, MC.S_STREAM).reshape(lut.shape)).all()
    adc = MC.triggered_capture(lut, N, hop, M, seed)
    assert _kernel(loc, adc, hop) == MC.DIRECT_STREAM_KERNEL[M]
    exp = oracle.stream_run(adc, N, MC.FS_STREAM, MC.S_STREAM, loc.window(), lut)
    assert exp["n_trig"].sum() >= 20 and exp["gate"].sum() >= 20
    for use_graph in (False, True):
        recs, est, last = TS.run_pipeline(loc, adc, hop, use_graph=use_graph)
        TS.compare(recs, est, last, exp, loc.dims.P)
    loc.close()


@pytest.mark.parametrize("N,hop,M,seed", MC.TRIGGERED)
def test_phat_stream_triggered(oracle, N, hop, M, seed):
    """k_stream_phat and its EMA grid solve on 4 and 6 tuple words: no stream dropped, no cell skipped."""
    loc = _stream_loc("gcc_phat", M, N)
    lut = loc.lut()
    adc = MC.triggered_capture(lut, N, hop, M, seed)
    assert _kernel(loc, adc, hop) == "k_stream_phat"
    ref = stream_phat_ref.run(oracle, adc, N, MC.FS_STREAM, MC.S_STREAM, loc.window(), lut)
    assert ref["gate"].sum() >= 20
    runs = []
    for use_graph in (False, True):
        runs.append(TSF.run_pipeline(loc, adc, hop, use_graph=use_graph))
        assert TSF.compare(runs[-1], ref, max_dropped=0, max_skip=0.0) == (0, 0)
    TSF.assert_bitwise(runs[1], runs[0])
    loc.close()


@pytest.mark.parametrize("fmt,N,hop,M,hops,seed,var,capture_len", MC.CONTINUOUS)
def test_phat_stream_continuous(oracle, fmt, N, hop, M, hops, seed, var, capture_len):
    """k_stream_active at 5, 6 and 7 mics on producer-fed rings of odd length."""
    loc = _stream_loc("gcc_phat", M, N, fmt)
    lut = loc.lut()
    cap = MC.continuous_capture(fmt, lut, N, hop, M, hops, seed)
    assert _kernel(loc, cap, hop, mode="continuous", activity_var=var) == (
        "k_stream_phat_pcm16" if fmt == "pcm16" else "k_stream_phat")
    ref = stream_cont_ref.run(oracle, cap, N, MC.FS_STREAM, MC.S_STREAM, loc.window(), lut, hop, var)
    assert ref["gate"].sum() >= 50
    runs = []
    for use_graph in (False, True):
        runs.append(TSC.run_pipeline(loc, cap, hop, var, use_graph=use_graph, capture_len=capture_len))
        TSF.compare(runs[-1], ref, max_dropped=0, max_skip=Cs.max_skip(M))
    TSF.assert_bitwise(runs[1], runs[0])
    loc.close()


def test_stream_peaks_then_track_at_6_mics(oracle):
    """step -> peaks -> track on the 6-mic DIRECT stream: k_stream_peaks and
    k_ls_stream<int64, 6> against tests/peaks_ref.py and oracle.ls_refine on the
    state snapshot, k_track against tests/track_ref.py on the hop's own peaks."""
    N, hop, M, seed = MC.TRIGGERED[0]
    loc = _stream_loc("direct", M, N)
    lut = loc.lut()
    adc = MC.triggered_capture(lut, N, hop, M, seed)
    pipe = StreamPipeline(loc, torch.from_numpy(adc).cuda(), hop=hop)
    prm = dict(track_ref.DEFAULTS, max_tracks=4, confirm_hits=2, max_misses=2)
    tr, nid = track_ref.new_state(MC.STREAMS)
    pk = pipe.peaks(3, 8, ls=True)  # no step yet: nothing is launched
    ot = pipe.track(**prm)
    listed = refined = 0
    for h in range(MC.HOPS):
        pipe.step()
        TSP._fill(pipe, pk)
        assert pipe.peaks(3, 8, ls=True) is pk
        n, ids, gate, est = TSP._check_rows(pipe, pk, lut, 3, 8, gated_only=True, where=("6 mics", h))
        if n:
            rows = {k: v[:n] for k, v in _np(pk).items()}
            empty = TPK._check_ls(oracle, loc, torch.from_numpy(est[ids]), rows, fs=float(MC.FS_STREAM))
            assert (empty.all(1) == (gate == 0)).all()
            refined += int((~empty).sum())
        TT._fill(pipe, ot)
        assert pipe.track(**prm) is ot
        tr, nid, n2, _ = TT._check_hop(pipe, ot, pk["count"], pk["xy_ls"], tr, nid, prm, ("6 mics", h))
        assert n2 == n
        listed += n
    assert listed >= 20 and refined >= 40, (listed, refined)
    assert (tr["status"] == 2).any() and nid.max() >= 1
    pipe.close()
    loc.close()


# ---------------------------------------------------------------- 5. beam
@pytest.mark.parametrize("M", [5, 6, 7])
def test_beam_batch(M):
    N, Kt, B = 256, 3, 7
    lc = _loc("gcc_phat", M, N, fs=MC.FS_STREAM)
    bg, mics, fs, c = TB._geom(lc)
    frames, xy, count = BC.block_case(mics, B, N, Kt, 100 + 10 * M + Kt)
    ref = beam_ref.beam(mics, fs, c, BC.H, frames, xy, count)
    host = tdoa.beam_host(bg, frames, xy, count)
    assert host["delays"].tobytes() == ref["delays"].tobytes() and ref["active"].any() and not ref["active"].all()
    got = _np(lc.beam_batch(*(torch.from_numpy(a).cuda() for a in (frames, xy, count))))
    assert got["delays"].tobytes() == ref["delays"].tobytes() and got["active"].tobytes() == ref["active"].tobytes()
    assert TB.near(got["audio"], ref, host["audio"], M), beam_ref.worst(got["audio"], ref, M)
    assert (got["audio"][ref["active"] == 0] == 0).all()
    lc.close()


# (engine, mode, ring type, M, N, hop, capture_len): 657 * 7 bytes is odd (every
# other ring on an odd address); 657 * 6 int16 samples leave the rings 4-byte
# aligned only.  Both rings are shorter than the 8 hops: the staged runs wrap.
BEAM_RINGS = [("gcc_phat", "triggered", np.uint8, 7, 256, 200, 657),
              ("gcc_phat", "continuous", np.int16, 6, 256, 200, 657)]


@pytest.mark.parametrize("engine,mode,dtype,M,N,hop,cap_len", BEAM_RINGS)
def test_beam_ring(engine, mode, dtype, M, N, hop, cap_len):
    S, HOPS, KT = TB.S, TB.HOPS, TB.KT
    lc = _loc(engine, M, N, fs=MC.FS_STREAM, sample_format="pcm16" if dtype == np.int16 else "adc8")
    bg, mics, fs, c = TB._geom(lc)
    A, D = beam_ref.latency(mics, fs, c)
    assert N + 2 * hop <= cap_len < HOPS * hop and cap_len >= 2 * hop + A + D + 16
    assert (cap_len * M * np.dtype(dtype).itemsize) % 16 != 0
    hist = BC.history(S, HOPS * hop, M, dtype, 7 * M + hop)
    src = torch.from_numpy(hist).cuda()
    xy, count = TB._targets(mics, hop)
    valid = np.arange(KT)[None, :] < count[:, None]
    d_xy, d_cnt = torch.from_numpy(xy).cuda(), torch.from_numpy(count).cuda()
    runs = {}
    for use_graph in (False, True):
        pipe = TB._pipe(lc, cap_len, dtype, hop, mode, use_graph)
        o = pipe.beam(d_xy, d_cnt)
        blocks, wrapped = [], 0
        for h in range(1, HOPS + 1):
            TB._produce(pipe, src, h - 1, hop)
            pipe.step()
            TB._fill(pipe, o)
            assert pipe.beam(d_xy, d_cnt) is o
            pipe.stream.synchronize()
            g = _np(o)
            n0, ref = BC.stream_ref(mics, fs, c, hist, xy, valid, hop, h)
            assert int(g["block_start"][0]) == n0 == h * hop - hop - A
            assert g["delays"].tobytes() == ref["delays"].tobytes() and g["active"].tobytes() == ref["active"].tobytes()
            assert beam_ref.close(g["audio"], ref, M), (h, beam_ref.worst(g["audio"], ref, M))
            assert (g["audio"][ref["active"] == 0] == 0).all()
            blocks.append(g["audio"])
            wrapped += ((n0 - 7) % cap_len) + hop + D + 15 > cap_len and n0 - 7 >= 0
        assert wrapped >= 1  # a staged run crossed the ring's end
        runs[use_graph] = np.concatenate(blocks, axis=2)
        pipe.close()
    assert np.abs(runs[False]).max() > 0
    assert runs[False].tobytes() == runs[True].tobytes()
    lc.close()
