"""Band-limited GCC-PHAT on the GPU (tdoa_set_bin_weights: k_phat_spectra, then
k_phat_pairs_w) against the float64 reference of tests/band_ref.py.

Tolerances: those of tests/test_gpu_gcc_phat.py unchanged (its check_phat) --
scores 3e-5 absolute, lags and gate equal where the float64 top-2 margin exceeds
2e-4, cell where the float64 grid margin exceeds 1e-3, max_Lf to 1e-3.  They
carry over because every table here has w <= 1: a weighted score is a sum of
the same per-bin terms, each scaled down, so the unweighted engine's error
bound holds.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import band_ref  # noqa: E402
import gcc_phat_oracle as G  # noqa: E402
import test_band_cpu as CPU  # noqa: E402  (the scenario's frames, delays and seed)
import test_gpu_gcc_phat as T  # noqa: E402  (check_phat, _grid_f32 and the tolerances)
import tdoa  # noqa: E402
from tdoa import synth  # noqa: E402
from tdoa.localizer import Localizer  # noqa: E402

FS, S = CPU.FS, CPU.S
MICS = {2: T.TWO, 3: None, 4: synth.square_mics(0.15), 5: synth.circle_mics(5, 0.15),
        8: synth.circle_mics(8, 0.15)}
MAX_UNSURE = 0.05  # share of pairs the 2e-4 margin may leave out


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _loc(M, N, **kw):
    return Localizer(engine="gcc_phat", num_mics=M, frame_len=N, sample_rate_hz=FS, mic_xy=MICS[M], **kw)


def _frames(M, N, B, seed=5):
    """B frames: B - 4 of the interferer scenario plus four full-range ones.
    The full-range frames' band-limited scores are noise, a few 1e-3 high, so a
    tenth of their pairs fall inside the 2e-4 lag margin; of the seeds 0..7,
    5 is the one at which the float64 reference alone leaves out the fewest
    pairs over the parity test's shapes and tables (worst case 4.2 %)."""
    fr, tgt, itf = synth.interferer_frames(B - 4, M, N, FS, S, 0xF00 + seed + 16 * M + N, CPU.TARGET_DELAYS,
                                           CPU.INTERFERER_DELAYS, device="cuda")
    full = synth.full_range_frames(4, M, N, 7 + N + seed).cuda()  # the CPU generator's draws
    return torch.cat([fr, full]).contiguous(), tgt, itf


def _tables(N):
    """A hard band low in the spectrum (only the bins k <= N/2 of a pair (k,
    N - k) carry weight), a tapered band high in it (only the bins N - k do),
    and uniform random weights (no wave of k_phat_pairs_w skips anything)."""
    rng = np.random.default_rng(N)
    return {"hard": tdoa.band_weights(N, FS, 1000, 6000),
            "taper": tdoa.band_weights(N, FS, 14000, 22000, 1500),
            "random": rng.uniform(0.0, 1.0, N + 1).astype(np.float32)}


# one shape per unweighted route, plus ragged ones; B * P a multiple of 8 (the
# XCD block remap) at (3, 1024, 8), (5, 512, 8) and (4, 4096, 8) only
SHAPES = [(2, 256, 33), (3, 1024, 33), (3, 1024, 8), (5, 512, 8), (4, 2048, 33), (4, 4096, 8), (8, 2048, 9)]


@pytest.mark.parametrize("M,N,B", SHAPES)
def test_parity_against_the_band_reference(M, N, B):
    loc = _loc(M, N)
    assert loc.dims.S == S
    lut, win = loc.lut(), loc.window()
    fr, _, _ = _frames(M, N, B)
    fr_np = fr.cpu().numpy()
    for name, w in _tables(N).items():
        assert w.max() <= 1.0
        loc.set_bin_weights(w)
        assert (loc.bin_weights() == w).all()
        assert loc.batch_kernel() == "k_phat_spectra" and not loc.batch_grid_fused()
        got = _np(loc.localize(fr, scores=True))
        exp = band_ref.gcc_phat_band(fr_np, S, win, w.astype(np.float64), lut)
        sure = T.check_phat(got, exp)
        print(f"({M}, {N}, B={B}) {name}: max |score err| {np.abs(got['scores_f'] - exp['scores_f']).max():.2e}, "
              f"pairs left out by the margin {1 - sure:.3f}")
        assert 1 - sure <= MAX_UNSURE, (name, sure)
    loc.close()


@pytest.mark.parametrize("M,N", [(3, 2048), (4, 4096)])
def test_scenario_band_finds_the_target(M, N):
    """Fails at the parent commit: unweighted GCC-PHAT reports the interferer."""
    fr, tgt, itf = CPU.scenario(M, N, device="cuda")
    loc = _loc(M, N)
    plain = _np(loc.localize(fr))
    hit_i = (plain["lags"] == itf).all(-1)
    print(f"({M}, {N}) unweighted: interferer's tuple on {hit_i.mean():.0%}")
    assert hit_i.mean() > 0.5
    assert not (plain["lags"] == tgt).all(-1).any()
    loc.set_band(1000, 6000)
    got = _np(loc.localize(fr))
    exp = band_ref.gcc_phat_band(fr.cpu().numpy(), S, loc.window(), band_ref.band_weights(N, FS, 1000, 6000))
    srt = np.sort(exp["scores_f"], axis=-1)
    sure = ((srt[..., -1] - srt[..., -2]) > T.TOL_LAG_MARGIN).all(-1)
    assert sure.any()
    hit = (got["lags"] == tgt).all(-1)
    print(f"({M}, {N}) 1-6 kHz: target tuple on {hit.mean():.0%}, {sure.mean():.0%} of frames sure")
    assert hit[sure].all()
    loc.close()


@pytest.mark.parametrize("M,N", [(3, 1024), (8, 2048)])
def test_clearing_restores_the_context(M, N):
    loc = _loc(M, N)
    kernel, fused = loc.batch_kernel(), loc.batch_grid_fused()
    assert kernel != "k_phat_spectra"
    if M == 3:
        assert kernel == "k_p1k_lean" and fused  # the fused lean kernel
    assert (loc.bin_weights() == 1.0).all()
    fr, _, _ = _frames(M, N, 24)
    before = loc.localize(fr, scores=True, ls=True)
    lean_before = loc.localize(fr)
    torch.cuda.synchronize()  # the setters want no call of the context in flight
    loc.set_band(1000, 6000, 500)
    assert not loc.batch_grid_fused() and loc.batch_kernel() == "k_phat_spectra"
    band = loc.localize(fr, scores=True, ls=True)
    assert not torch.equal(band["scores_f"], before["scores_f"])  # (synchronises)
    loc.set_bin_weights(None)
    assert (loc.bin_weights() == 1.0).all()
    assert loc.batch_kernel() == kernel and loc.batch_grid_fused() == fused
    after = loc.localize(fr, scores=True, ls=True)
    lean_after = loc.localize(fr)
    for a, b in ((before, after), (lean_before, lean_after)):
        for k in a:
            assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), k
    loc.close()


@pytest.mark.parametrize("M,N", [(3, 1024), (4, 2048)])
def test_all_ones_table_against_no_table(M, N):
    """Two engines, each within 3e-5 of the same float64 scores."""
    loc = _loc(M, N)
    fr, _, _ = _frames(M, N, 20)
    plain = _np(loc.localize(fr, scores=True))
    loc.set_bin_weights(np.ones(N + 1, np.float32))
    ones = _np(loc.localize(fr, scores=True))
    err = np.abs(ones["scores_f"] - plain["scores_f"]).max()
    print(f"({M}, {N}) all-ones table vs none: max |score diff| {err:.2e}")
    assert err <= 2 * T.TOL_SCORE
    exp = G.gcc_phat_batch(fr.cpu().numpy(), S, loc.window(), loc.lut())
    T.check_phat(ones, exp)
    srt = np.sort(exp["scores_f"], axis=-1)
    sure = (srt[..., -1] - srt[..., -2]) > T.TOL_LAG_MARGIN
    assert (ones["lags"][sure] == plain["lags"][sure]).all()
    loc.close()


@pytest.mark.parametrize("M,N", [(3, 1024), (4, 2048)])
def test_downstream_on_a_band_context(oracle, M, N):
    """Grid, least squares, peaks and heat map on the band route's own scores,
    all requested in one call: (3, 1024) solves the grid in its first kernel
    and (4, 2048) takes the refinement's peak scores from it when unweighted."""
    loc = _loc(M, N, band_hz=(2000, 9000), band_taper_hz=1500)
    assert (loc.bin_weights() == tdoa.band_weights(N, FS, 2000, 9000, 1500)).all()
    fr, _, _ = _frames(M, N, 20, seed=1)
    out = loc.localize(fr, scores=True, grid=True, ls=True)
    got = _np(out)
    cell, mx = T._grid_f32(got["weighted_f"], loc.lut())
    assert (got["cell"] == cell).all()
    assert (got["max_Lf"] == mx).all()
    uv, rms = oracle.ls_refine(got["scores_f"], got["lags"], loc.mics(), got["cell"])
    err = np.abs(got["xy_ls"] - uv) / np.maximum(1.0, np.abs(uv))
    assert err.max() <= 1e-5  # tests/test_ls.py TOL
    assert np.abs(got["ls_rms"] - rms).max() <= 1e-4 * max(1.0, rms.max())
    # without scores / cell requested: the context's scratch gives the same answer
    lean = loc.localize(fr, grid=False, ls=True)
    assert (lean["xy_ls"].cpu().numpy() == got["xy_ls"]).all()
    pk = loc.peaks(out["weighted_f"], num_peaks=1)
    assert torch.equal(pk["cell"][:, 0], out["cell"]) and torch.equal(pk["Lf"][:, 0], out["max_Lf"])
    hm = loc.heatmap(out["weighted_f"], out["max_Lf"]).cpu().numpy()
    assert hm.shape == (20, 101, 101) and hm.max() <= 4
    pos = got["max_Lf"] > 0  # the argmax cell is white (L >= max * 63 / 64)
    assert (hm.reshape(20, -1)[np.arange(20), got["cell"]][pos] == 4).all()
    loc.close()


def test_chunking_matches_one_chunk():
    """(8, 2048): 128 MiB of scratch hold 1024 frames' spectra, so 1030 frames
    run in two chunks; rows past the first chunk equal a 10-frame call."""
    M, N = 8, 2048
    loc = _loc(M, N, band_hz=(1000, 6000))
    fr, _, _ = synth.adc_frames(1030, M, N, loc.lut(), S, 5, device="cuda")
    big = loc.localize(fr, scores=True)
    part = loc.localize(fr[1020:1030].contiguous(), scores=True)
    for k in part:
        assert torch.equal(big[k][1020:1030].view(torch.uint8), part[k].view(torch.uint8)), k
    loc.close()


def test_setter_errors_leave_the_table_in_force():
    direct = Localizer(engine="direct")
    with pytest.raises(tdoa.TdoaError) as e:
        direct.set_band(1000, 6000)
    assert e.value.code == -1
    with pytest.raises(tdoa.TdoaError) as e:
        direct.set_bin_weights(np.ones(1025, np.float32))
    assert e.value.code == -1
    assert (direct.bin_weights() == 1.0).all()
    direct.close()

    loc = _loc(3, 1024, band_hz=(1000, 6000))
    w0 = loc.bin_weights()
    fr, _, _ = _frames(3, 1024, 12)
    before = loc.localize(fr, scores=True)
    torch.cuda.synchronize()
    bad = {"nan": w0.copy(), "inf": w0.copy(), "negative": w0.copy(), "zero": np.zeros_like(w0)}
    bad["nan"][700] = np.nan
    bad["inf"][3] = np.inf
    bad["negative"][100] = -1e-3
    for name, w in bad.items():
        with pytest.raises(tdoa.TdoaError) as e:
            loc.set_bin_weights(w)
        assert e.value.code == -1, name
        assert (loc.bin_weights() == w0).all(), name
        assert loc.batch_kernel() == "k_phat_spectra"
    with pytest.raises(tdoa.TdoaError):
        loc.set_band(6000, 1000)
    with pytest.raises(ValueError):
        loc.set_bin_weights(np.ones(1024, np.float32))
    after = loc.localize(fr, scores=True)
    for k in before:
        assert torch.equal(before[k].view(torch.uint8), after[k].view(torch.uint8)), k
    loc.close()


def test_empty_batch_and_one_frame():
    loc = _loc(3, 1024, band_hz=(1000, 6000))
    out = loc.localize(torch.empty((0, 3, 1024), dtype=torch.int16, device="cuda"))
    assert out["lags"].shape == (0, 3)
    fr, _, _ = _frames(3, 1024, 5)
    one = fr[:1].contiguous()
    got = _np(loc.localize(one, scores=True))
    exp = band_ref.gcc_phat_band(one.cpu().numpy(), S, loc.window(), loc.bin_weights().astype(np.float64), loc.lut())
    T.check_phat(got, exp)
    loc.close()
