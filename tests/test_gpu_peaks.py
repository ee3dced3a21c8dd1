"""Multi-source peak extraction on the GPU (tdoa_peaks / k_peaks,
Localizer.peaks) against its numpy restatement tests/peaks_ref.py, bit for
bit on the run's own score blocks; the Kp = 1 identity with the grid solve;
the two-source premise end to end; the per-peak least-squares refinement
against the double-precision oracle; argument errors; stream order."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import peaks_ref as R
from test_ls import TOL

from tdoa import synth

pytestmark = pytest.mark.gpu

KPS, RADII = (1, 3, 8), (0, 3, 60)

SHAPES = {
    "m2": (dict(num_mics=2, mic_xy=np.array([[-0.1, 0.0], [0.1, 0.0]], np.float32)), 9),
    "m3_ragged": (dict(), 33),
    "m8_n256": (dict(num_mics=8, frame_len=256, mic_xy=synth.circle_mics(8, 0.15)), 5),
    "small_15x9": (dict(grid_half_w=7, grid_half_h=4), 6),       # G = 135 < the workgroup
    "g475": (dict(num_mics=4, mic_xy=synth.square_mics(0.15), grid_half_w=12, grid_half_h=9), 7),  # 25 x 19
}


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _ref_args(loc):
    return (loc.grid_W, loc.grid_half_w, loc.grid_half_h, loc.grid_scale, loc.dims.S)


def _loc(engine, cfg):
    from tdoa.localizer import Localizer
    return Localizer(engine=engine, **cfg)


@pytest.mark.parametrize("engine", ["direct", "gcc_phat"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_peaks_bit_exact_on_own_scores(shape, engine):
    cfg, B = SHAPES[shape]
    loc = _loc(engine, cfg)
    d, lut = loc.dims, loc.lut()
    assert shape != "g475" or d.G % 64 != 0
    fr, _, _ = synth.adc_frames(B, d.M, d.N, lut, d.S, 31 + B, device="cuda")
    out = loc.localize(fr, scores=True)
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    if engine == "direct":
        blocks = {"scores": out["scores"], "weighted": out["weighted"],
                  "all_equal": torch.full((B, d.P, d.K), 7, dtype=torch.int64, device="cuda"),
                  "random": torch.randint(-(1 << 40), (1 << 40) + 1, (B, d.P, d.K), generator=g,
                                          device="cuda", dtype=torch.int64)}
    else:
        blocks = {"scores_f": out["scores_f"], "weighted_f": out["weighted_f"],
                  "all_equal": torch.full((B, d.P, d.K), 0.25, dtype=torch.float32, device="cuda")}
    for name, blk in blocks.items():
        Lm = R.l_map(blk.cpu().numpy(), lut)
        for Kp, radius in itertools.product(KPS, RADII):
            got = _np(loc.peaks(blk, Kp, radius))
            exp = R.peaks_from_map(Lm, lut, *_ref_args(loc), Kp, radius)
            assert set(got) == set(exp)
            R.assert_equal(got, exp, (shape, engine, name, Kp, radius))
            assert (got["count"] >= 1).all() and (got["cell"] < d.G).all()
    loc.close()


@pytest.mark.parametrize("engine,cfg", [
    ("direct", dict()), ("gcc_phat", dict()),
    ("direct", dict(num_mics=8, frame_len=2048, mic_xy=synth.circle_mics(8, 0.15))),
    ("gcc_phat", dict(num_mics=8, frame_len=2048, mic_xy=synth.circle_mics(8, 0.15))),
    ("gcc_phat", dict(num_mics=4, frame_len=4096, mic_xy=synth.square_mics(0.15))),
], ids=["direct3", "phat3", "direct8", "phat8", "phat4"])
def test_one_peak_on_weighted_is_the_grid_solve(engine, cfg):
    loc = _loc(engine, cfg)
    d = loc.dims
    fr, _, _ = synth.adc_frames(40, d.M, d.N, loc.lut(), d.S, 3, device="cuda")
    out = loc.localize(fr, scores=True)
    direct = engine == "direct"
    pk = loc.peaks(out["weighted" if direct else "weighted_f"], 1, 8)
    assert (pk["count"] == 1).all()
    assert torch.equal(pk["cell"][:, 0], out["cell"])
    assert torch.equal(pk["xy"][:, 0], out["xy"])
    assert torch.equal(pk["L" if direct else "Lf"][:, 0], out["max_L" if direct else "max_Lf"])
    loc.close()


@pytest.mark.parametrize("engine", ["direct", "gcc_phat"])
def test_min_rel_cuts_some_frames(engine):
    loc = _loc(engine, dict())
    d, lut = loc.dims, loc.lut()
    fr, _, _ = synth.adc_frames(33, d.M, d.N, lut, d.S, 21, device="cuda")
    blk = loc.localize(fr, scores=True)["scores" if engine == "direct" else "scores_f"]
    Lm = R.l_map(blk.cpu().numpy(), lut)
    free = R.peaks_from_map(Lm, lut, *_ref_args(loc), 3, 8)
    v = free["L" if engine == "direct" else "Lf"].astype(np.float64)
    assert (free["count"] == 3).all() and (v[:, 0] > 0).all()
    thr = float(np.float32(np.median(v[:, 1] / v[:, 0])))  # about half the frames lose peak 1
    exp = R.peaks_from_map(Lm, lut, *_ref_args(loc), 3, 8, thr)
    assert (exp["count"] == 1).any() and (exp["count"] > 1).any()
    got = _np(loc.peaks(blk, 3, 8, min_rel=thr))
    R.assert_equal(got, exp, engine)
    loc.close()


def test_two_sources_end_to_end():
    from tdoa.localizer import Localizer
    fr, cells, lut, win, mics = R.two_source_case()
    loc = Localizer(engine="gcc_phat", num_mics=8, frame_len=2048, mic_xy=mics, window_q15=win)
    assert (loc.lut() == lut).all() and (loc.window() == win).all()
    out = loc.localize(torch.from_numpy(fr).cuda(), scores=True)
    pk = _np(loc.peaks(out["scores_f"], 2, 8))
    found = R.both_found(cells, pk["cell"], 101, within=8)
    assert found.all(), np.flatnonzero(~found).tolist()
    one = loc.peaks(out["weighted_f"], 1, 8)
    assert torch.equal(one["cell"][:, 0], out["cell"])
    loc.close()


def _raw_peaks(loc, scores, Kp, radius, min_rel, **tensors):
    """tdoa_peaks through ctypes with exactly the given output tensors."""
    from tdoa import _lib
    prm = _lib.PeaksParams(Kp, radius, min_rel)
    o = _lib.PeaksOutputs()
    for k, t in tensors.items():
        setattr(o, k, t.data_ptr())
    st = torch.cuda.current_stream()
    return _lib.load().tdoa_peaks(loc._ctx, C.c_void_p(scores.data_ptr()), int(scores.dtype == torch.float32),
                                  scores.shape[0], C.byref(prm), C.byref(o), C.c_void_p(st.cuda_stream))


def _check_ls(oracle, loc, blk, pk, fs=50000.0):
    """xy_ls / ls_rms of every non-empty slot against oracle.ls_refine started at
    the peak with the peak's lags; NaN in the empty slots.  Returns the slots' emptiness."""
    sc = blk.cpu().numpy()
    empty = pk["cell"] < 0
    for k in range(pk["cell"].shape[1]):
        on = ~empty[:, k]
        if on.any():
            uv, rms = oracle.ls_refine(sc[on], pk["lags"][on, k], loc.mics(), pk["cell"][on, k],
                                       half_w=loc.grid_half_w, half_h=loc.grid_half_h,
                                       grid_scale=loc.grid_scale, fs=fs)
            err = np.abs(pk["xy_ls"][on, k] - uv) / np.maximum(1.0, np.abs(uv))
            assert err.max() <= TOL, (k, err.max())
            assert np.abs(pk["ls_rms"][on, k] - rms).max() <= 1e-4 * max(1.0, rms.max())
    assert np.isnan(pk["xy_ls"][empty]).all() and np.isnan(pk["ls_rms"][empty]).all()
    assert not np.isnan(pk["xy_ls"][~empty]).any()
    return empty


@pytest.mark.parametrize("engine,M", [("direct", 4), ("gcc_phat", 8)])
def test_ls_per_peak_vs_oracle(oracle, engine, M):
    cfg = (dict(num_mics=4, mic_xy=synth.square_mics(0.15), max_shift=20) if M == 4 else
           dict(num_mics=8, frame_len=512, mic_xy=synth.circle_mics(8, 0.15)))
    loc = _loc(engine, cfg)
    d, lut = loc.dims, loc.lut()
    fr, _, _ = synth.adc_frames(24, d.M, d.N, lut, d.S, 13, device="cuda")
    blk = loc.localize(fr, scores=True)["scores" if engine == "direct" else "scores_f"]
    pk = _np(loc.peaks(blk, 3, 8, ls=True))
    assert not _check_ls(oracle, loc, blk, pk).any()
    # a threshold that leaves empty slots: they are NaN, the others unchanged
    cut = _np(loc.peaks(blk, 3, 8, min_rel=0.97, ls=True))
    assert _check_ls(oracle, loc, blk, cut).any()
    # without lags requested the lag tuples go through the context's scratch
    cell = torch.empty((24, 3), dtype=torch.int32, device="cuda")
    xy_ls = torch.empty((24, 3, 2), dtype=torch.float32, device="cuda")
    assert _raw_peaks(loc, blk, 3, 8, 0.0, cell=cell, xy_ls=xy_ls) == 0
    assert (cell.cpu().numpy() == pk["cell"]).all() and (xy_ls.cpu().numpy() == pk["xy_ls"]).all()
    if M == 4:
        # a peak whose lag tuple sits at the end of the lag range (the corner cell's
        # clamped LUT lags): no parabolic vertex there (inside == false)
        S = d.S
        assert (np.abs(lut[:, 0].astype(np.int64) - S) == S).any()
        for dtype in (torch.float32, torch.int64):
            edge = torch.zeros((2, d.P, d.K), dtype=dtype, device="cuda")
            edge[:, :, 1:-1] = 1
            for p in range(d.P):
                edge[:, p, int(lut[p, 0])] = 1000 + p
            pe = _np(loc.peaks(edge, 2, 8, ls=True))
            assert (pe["cell"][:, 0] == 0).all() and (np.abs(pe["lags"][:, 0]) == S).any()
            _check_ls(oracle, loc, edge, pe)
    loc.close()


def test_argument_errors_leave_outputs_untouched():
    from tdoa import _lib
    from tdoa.localizer import Localizer
    L = _lib.load()
    loc = Localizer(engine="gcc_phat")
    d = loc.dims
    sc = torch.rand((4, d.P, d.K), device="cuda")
    cell = torch.full((4, 8), 77, dtype=torch.int32, device="cuda")
    count = torch.full((4,), 77, dtype=torch.int32, device="cuda")
    prm = _lib.PeaksParams(2, 8, 0.0)
    o = _lib.PeaksOutputs()
    o.cell, o.count = cell.data_ptr(), count.data_ptr()
    no_cell = _lib.PeaksOutputs()
    no_cell.count = count.data_ptr()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    scp = C.c_void_p(sc.data_ptr())
    bad = [
        (None, scp, 4, C.byref(prm), C.byref(o)),
        (loc._ctx, None, 4, C.byref(prm), C.byref(o)),
        (loc._ctx, scp, 4, None, C.byref(o)),
        (loc._ctx, scp, 4, C.byref(prm), None),
        (loc._ctx, scp, 4, C.byref(prm), C.byref(no_cell)),
        (loc._ctx, scp, -1, C.byref(prm), C.byref(o)),
        (loc._ctx, scp, 4, C.byref(_lib.PeaksParams(0, 8, 0.0)), C.byref(o)),
        (loc._ctx, scp, 4, C.byref(_lib.PeaksParams(9, 8, 0.0)), C.byref(o)),
        (loc._ctx, scp, 4, C.byref(_lib.PeaksParams(2, -1, 0.0)), C.byref(o)),
    ]
    for ctx, s, B, p, out in bad:
        assert L.tdoa_peaks(ctx, s, 1, B, p, out, st) == -1
        assert L.tdoa_last_error()
    with pytest.raises(_lib.TdoaError):
        loc.peaks(sc, 9, 8)
    with pytest.raises(ValueError):
        loc.peaks(sc[:, :, :-1].contiguous(), 2, 8)
    with pytest.raises(ValueError):
        loc.peaks(sc.double(), 2, 8)
    with pytest.raises(ValueError):
        loc.peaks(sc.transpose(1, 2).contiguous().transpose(1, 2), 2, 8)
    with pytest.raises(ValueError):
        loc.peaks(sc.cpu(), 2, 8)
    # B = 0 is fine and launches nothing
    assert L.tdoa_peaks(loc._ctx, scp, 1, 0, C.byref(prm), C.byref(o), st) == 0
    assert tuple(loc.peaks(sc[:0], 2, 8)["cell"].shape) == (0, 2)
    # a 201 x 201 grid: the L map alone is past the kernel's LDS budget
    big = Localizer(engine="gcc_phat", grid_half_w=100, grid_half_h=100)
    scb = torch.rand((4, big.dims.P, big.dims.K), device="cuda")
    assert L.tdoa_peaks(big._ctx, C.c_void_p(scb.data_ptr()), 1, 4, C.byref(prm), C.byref(o), st) == -1
    assert b"LDS" in L.tdoa_last_error()
    big.close()
    torch.cuda.synchronize()
    assert (cell == 77).all() and (count == 77).all()
    loc.close()


def test_two_calls_on_one_stream_without_sync():
    loc = _loc("gcc_phat", dict())
    d, lut = loc.dims, loc.lut()
    g = torch.Generator(device="cuda")
    g.manual_seed(11)
    a = torch.rand((64, d.P, d.K), generator=g, device="cuda")
    b = torch.rand((64, d.P, d.K), generator=g, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    ra = loc.peaks(a, 3, 5, ls=True, stream=s)
    rb = loc.peaks(b, 3, 5, ls=True, stream=s)
    s.synchronize()
    for blk, got in ((a, ra), (b, rb)):
        exp = R.peaks_ref(blk.cpu().numpy(), lut, *_ref_args(loc), 3, 5)
        R.assert_equal(_np(got), exp)
    assert not torch.equal(ra["cell"], rb["cell"])
    assert torch.equal(ra["xy_ls"], loc.peaks(a, 3, 5, ls=True)["xy_ls"])
    loc.close()
