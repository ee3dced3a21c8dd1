"""16-bit PCM input to GCC_PHAT on the GPU (tdoa_set_sample_format: k_p1k_pcm16,
k_f16_pcm16, k_phat_spectra_pcm16) against the float64 reference of
tests/pcm16_ref.py.

Tolerances: those of tests/test_gpu_gcc_phat.py unchanged (its check_phat) --
scores 3e-5 absolute, lags and gate equal where the float64 top-2 margin exceeds
2e-4, cell where the float64 grid margin exceeds 1e-3, max_Lf to 1e-3.  They
carry over because the prepared samples enter the same transforms in the same
units and the fixtures are white: the engine's conditioning is that of the
8-bit format (DESIGN.md "16-bit input" has the coloured-frame caveat).  The
2e-4 margin may leave out at most 5 % of a batch's pairs; the batches and
their seeds are those of tests/test_pcm16_cpu.py, chosen on the float64
reference alone.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gcc_phat_oracle as G  # noqa: E402
import pcm16_ref  # noqa: E402
import test_gpu_gcc_phat as T  # noqa: E402  (check_phat, _grid_f32 and the tolerances)
import test_pcm16_cpu as CPU  # noqa: E402  (the scenario, the batches and their seeds)
import tdoa  # noqa: E402
from tdoa import synth  # noqa: E402
from tdoa.localizer import Localizer  # noqa: E402
from tdoa.stream import StreamPipeline  # noqa: E402

FS, S = CPU.FS, CPU.S
MICS = {2: T.TWO, 3: None, 4: synth.square_mics(0.15), 5: synth.circle_mics(5, 0.15),
        8: synth.circle_mics(8, 0.15)}
P1K, F16, TWO_PASS = "k_p1k_pcm16", "k_f16_pcm16", "k_phat_spectra_pcm16"


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _loc(M, N, **kw):
    return Localizer(engine="gcc_phat", num_mics=M, frame_len=N, sample_rate_hz=FS, mic_xy=MICS[M], **kw)


def _check_batch(loc, fr_np, silent, w=None):
    """One batch through the context against the float64 reference: check_phat,
    the margin cap, and the silent mic's frame."""
    M = loc.dims.M
    got = _np(loc.localize(torch.from_numpy(fr_np).cuda(), scores=True))
    exp = pcm16_ref.gcc_phat_pcm16(fr_np, S, loc.window(), loc.lut(), w=w)
    err = np.abs(got["scores_f"] - exp["scores_f"]).max()
    left_out = CPU.unsure_share(exp, M, silent)
    print(f"({M}, {loc.dims.N}, B={len(fr_np)}) {loc.batch_kernel()}: max |score err| {err:.2e}, "
          f"pairs left out by the margin {left_out:.3f}")
    T.check_phat(got, exp)
    assert left_out <= CPU.MAX_UNSURE
    for k in ("scores_f", "weighted_f", "max_Lf", "xy"):
        assert np.isfinite(got[k]).all(), k
    assert np.abs(got["lags"]).max() <= S
    assert got["cell"].min() >= 0 and got["cell"].max() < loc.dims.G
    if silent is not None:
        sp = CPU.silent_pairs(M)
        assert np.abs(got["scores_f"][silent][sp]).max() <= T.TOL_SCORE
        assert np.abs(got["weighted_f"][silent][sp]).max() <= T.TOL_SCORE
    return got, exp


# ---- parity, per route
ROUTES = [
    # the fused config-2 variant: a lone half-wave, one full workgroup plus one frame, several workgroups
    (3, 1024, 1, P1K, True), (3, 1024, 9, P1K, True), (3, 1024, 33, P1K, True),
    # the long-frame variant; 300 frames: the persistent loop takes more than one frame per workgroup
    (4, 2048, 33, F16, False), (8, 2048, 9, F16, False), (4, 4096, 8, F16, False), (3, 4096, 5, F16, False),
    (4, 2048, 300, F16, False),
    # the two-pass route
    (2, 256, 33, TWO_PASS, False), (5, 512, 8, TWO_PASS, False), (4, 1024, 33, TWO_PASS, False),
    (3, 2048, 8, TWO_PASS, False), (5, 2048, 9, TWO_PASS, False),
]


@pytest.mark.parametrize("M,N,B,kernel,fused", ROUTES)
def test_parity_per_route(M, N, B, kernel, fused):
    loc = _loc(M, N, sample_format="pcm16")
    assert loc.dims.S == S and loc.sample_format == "pcm16"
    assert loc.batch_kernel() == kernel and loc.batch_grid_fused() == fused
    fr, silent = CPU.batch(M, N, B)
    _check_batch(loc, fr, silent)
    loc.close()


# ---- the scenario
@pytest.mark.parametrize("M,N", [(3, 1024), (8, 2048)])
def test_scenario_pcm16_finds_the_source(M, N):
    """Fails at the parent commit: the 8-bit front end keeps the low byte of
    every sample, and there is no other."""
    fr, lags = CPU.scenario(M, N, device="cuda")
    loc = _loc(M, N)
    assert loc.sample_format == "adc8"
    adc8 = _np(loc.localize(fr))
    hit8 = (adc8["lags"] == lags).all(-1)
    print(f"({M}, {N}) adc8: true tuple on {hit8.sum()} of {len(hit8)}")
    assert not hit8.any()
    torch.cuda.synchronize()  # the setters want no call of the context in flight
    loc.set_sample_format("pcm16")
    got = _np(loc.localize(fr))
    exp = pcm16_ref.gcc_phat_pcm16(fr.cpu().numpy(), S, loc.window())
    srt = np.sort(exp["scores_f"], axis=-1)
    sure = ((srt[..., -1] - srt[..., -2]) > T.TOL_LAG_MARGIN).all(-1)
    hit = (got["lags"] == lags).all(-1)
    print(f"({M}, {N}) pcm16: true tuple on {hit.sum()} of {len(hit)}, {sure.sum()} frames sure")
    assert sure.all() and hit[sure].all()
    loc.close()


# ---- identity end to end: x in 8 bits, 256 x in 16
def _small_frames(M, N, B):
    """8-bit-sized frames whose rows sum to multiples of N with |x - mean| < 128:
    prep16(256 x) == prep(x) exactly (tests/test_pcm16_cpu.py)."""
    fr, _ = synth.pcm16_frames(B, M, N, S, 0x1D + 16 * M + N, CPU.TARGET_DELAYS, src_std=30.0, noise_std=6.0)
    x = np.clip(fr.numpy().astype(np.int64), -100, 100)
    r = x.sum(-1) % N
    x -= np.arange(N) < r[..., None]
    assert (x.sum(-1) % N == 0).all() and np.abs(x - x.sum(-1, keepdims=True) // N).max() < 128
    return x.astype(np.int16)


@pytest.mark.parametrize("M,N,kernels", [(3, 1024, ("k_p1k_lean", P1K)), (8, 2048, ("k_frame16", F16)),
                                          (5, 512, ("k_phat_spectra", TWO_PASS))])
def test_identity_end_to_end(M, N, kernels):
    x = _small_frames(M, N, 12)
    x256 = (256 * x.astype(np.int32)).astype(np.int16)
    a, b = _loc(M, N), _loc(M, N, sample_format="pcm16")
    assert (a.batch_kernel(), b.batch_kernel()) == kernels
    assert (pcm16_ref.prep16(x256, a.window()) == G.prep(x, a.window())).all()
    exp = G.gcc_phat_batch(x, S, a.window(), a.lut())  # the one reference of both runs
    ga = _np(a.localize(torch.from_numpy(x).cuda(), scores=True))
    gb = _np(b.localize(torch.from_numpy(x256).cuda(), scores=True))
    T.check_phat(ga, exp)
    T.check_phat(gb, exp)
    print(f"({M}, {N}) adc8 on x vs pcm16 on 256 x: max |score diff| "
          f"{np.abs(ga['scores_f'] - gb['scores_f']).max():.2e}")
    for k in ("lags", "gate", "cell"):
        assert (ga[k] == gb[k]).all(), k
    a.close()
    b.close()


# ---- switching back
@pytest.mark.parametrize("M,N", [(3, 1024), (8, 2048)])
def test_switching_back_restores_the_context(M, N):
    loc = _loc(M, N)
    kernel, fused = loc.batch_kernel(), loc.batch_grid_fused()
    assert kernel == ("k_p1k_lean" if M == 3 else "k_frame16")
    fr = torch.from_numpy(CPU.batch(M, N, 12)[0]).cuda()
    before = loc.localize(fr, scores=True, ls=True)
    torch.cuda.synchronize()
    loc.set_sample_format("pcm16")
    assert loc.sample_format == "pcm16" and loc.batch_kernel() == (P1K if M == 3 else F16)
    assert loc.batch_grid_fused() == (M == 3)
    mid = loc.localize(fr, scores=True, ls=True)
    assert not torch.equal(mid["scores_f"], before["scores_f"])  # (synchronises)
    loc.set_sample_format("adc8")
    assert loc.sample_format == "adc8"
    assert loc.batch_kernel() == kernel and loc.batch_grid_fused() == fused
    after = loc.localize(fr, scores=True, ls=True)
    for k in ("scores_f", "lags", "cell", "xy_ls"):
        assert torch.equal(before[k].view(torch.uint8), after[k].view(torch.uint8)), k
    loc.close()


# ---- band limiting with 16-bit input
@pytest.mark.parametrize("M,N", [(3, 1024), (4, 2048)])
def test_band_with_pcm16(M, N):
    loc = _loc(M, N, sample_format="pcm16", band_hz=(1000, 6000))
    assert loc.batch_kernel() == TWO_PASS and not loc.batch_grid_fused()
    w = loc.bin_weights()
    assert (w == tdoa.band_weights(N, FS, 1000, 6000)).all()
    fr, silent = CPU.batch(M, N, 24)
    # (the margin cap is the white batches': a band keeps a quarter of the bins
    # and the full-range frames' scores shrink with it, so the cap is checked on
    # the source frames here)
    got = _np(loc.localize(torch.from_numpy(fr).cuda(), scores=True))
    exp = pcm16_ref.gcc_phat_pcm16(fr, S, loc.window(), loc.lut(), w=w.astype(np.float64))
    T.check_phat(got, exp)
    srt = np.sort(exp["scores_f"][:20], axis=-1)
    assert ((srt[..., -1] - srt[..., -2]) > T.TOL_LAG_MARGIN).mean() >= 1 - CPU.MAX_UNSURE
    assert np.abs(got["scores_f"][silent][CPU.silent_pairs(M)]).max() <= T.TOL_SCORE
    torch.cuda.synchronize()
    loc.set_bin_weights(None)  # back to the format's own route
    assert loc.batch_kernel() == (P1K if M == 3 else F16)
    loc.close()


# ---- least squares
def test_least_squares_at_8x2048(oracle):
    M, N = 8, 2048
    loc = _loc(M, N, sample_format="pcm16")
    fr = torch.from_numpy(CPU.batch(M, N, 12)[0][:8].copy()).cuda()  # the source frames
    got = _np(loc.localize(fr, scores=True, grid=True, ls=True))
    uv, rms = oracle.ls_refine(got["scores_f"], got["lags"], loc.mics(), got["cell"])
    err = np.abs(got["xy_ls"] - uv) / np.maximum(1.0, np.abs(uv))
    print(f"(8, 2048) pcm16 least squares: max relative error {err.max():.2e}")
    assert err.max() <= 1e-5  # tests/test_ls.py TOL
    assert np.abs(got["ls_rms"] - rms).max() <= 1e-4 * max(1.0, rms.max())
    # without scores / cell requested: the kernel's peak scores give the same answer
    lean = loc.localize(fr, grid=False, ls=True)
    assert (lean["xy_ls"].cpu().numpy() == got["xy_ls"]).all()
    loc.close()


# ---- two HIP streams on the grid-fused route
def test_two_streams_equal_one():
    loc = _loc(3, 1024, sample_format="pcm16")
    assert loc.batch_grid_fused()
    batches = [synth.pcm16_frames(512, 3, 1024, S, 0x5151 + i, CPU.TARGET_DELAYS, dc=CPU.DC, device="cuda")[0]
               for i in range(4)]
    streams = [torch.cuda.current_stream(), torch.cuda.Stream()]
    outs = [[loc.alloc_outputs(512) for _ in range(2)] for _ in range(2)]
    torch.cuda.synchronize()
    for rep in range(3):  # the same launches several times over: no state carried between them
        for i, fr in enumerate(batches):
            loc.prepare(fr, outs[i % 2][i // 2], streams[i % 2])()
    torch.cuda.synchronize()
    for i, fr in enumerate(batches):
        got = _np(outs[i % 2][i // 2])
        exp = _np(loc.localize(fr))
        for k in exp:
            assert np.array_equal(got[k], exp[k]), (i, k)
    loc.close()


# ---- rejections
def test_rejections():
    direct = Localizer(engine="direct")
    with pytest.raises(tdoa.TdoaError) as e:
        direct.set_sample_format("pcm16")
    assert e.value.code == -1 and direct.sample_format == "adc8"
    direct.set_sample_format("adc8")  # accepted on any context
    with pytest.raises(tdoa.TdoaError):
        Localizer(engine="direct", sample_format="pcm16")
    direct.close()

    loc = _loc(3, 1024)
    with pytest.raises(ValueError):
        loc.set_sample_format("float32")
    assert tdoa.load().tdoa_set_sample_format(loc._ctx, 2) == -1
    assert tdoa.load().tdoa_set_sample_format(loc._ctx, -1) == -1
    assert loc.sample_format == "adc8" and loc.batch_kernel() == "k_p1k_lean"

    # a pipeline created before the switch keeps its 8-bit parameters and steps
    cap = synth.adc_stream(4, 6144, 3, loc.lut(), S, 0xC0, device="cuda")
    pipe = StreamPipeline(loc, cap, hop=512)
    loc.set_sample_format("pcm16")
    with pytest.raises(tdoa.TdoaError) as e:
        StreamPipeline(loc, cap, hop=512)
    assert e.value.code == -1
    for _ in range(4):
        pipe.step()
    rec = pipe.records()
    assert np.isfinite(rec["max_Lf"]).all() and np.abs(rec["lags"]).max(initial=0) <= S
    assert pipe.totals()[0] == 4 * 512
    pipe.close()
    loc.close()
