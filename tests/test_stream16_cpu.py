"""The int16 streaming reference (tests/stream16_ref.py) and synth.pcm16_stream
pinned on the CPU, on the captures the GPU tests use (tests/stream16_cases.py,
tests/test_gpu_stream16.py)."""
import numpy as np
import pytest

import band_ref
import pcm16_ref
import stream16_cases as Cs
import stream16_ref as R
from tdoa import synth

FS, S = Cs.FS, Cs.S_LAG


@pytest.fixture(scope="module")
def lut3(oracle):
    return Cs.lut_cpu(oracle, 3)


# ---- the trigger: anchored to the pinned 8-bit one

@pytest.mark.parametrize("N,hop,M,seed", [(1024, 512, 3, 0x5EED0005), (1024, 384, 3, 424), (256, 256, 3, 77)])
def test_scaled_8bit_capture_fires_where_the_8bit_trigger_does(oracle, lut3, N, hop, M, seed):
    """(u8 - 128) * 256 with trigger_var 2 * 256^2: both sides of the inequality
    scale by 65536 and the shift cancels in pw.  A constant added per mic
    cancels too, and a hop only cuts the capture to whole hops."""
    adc = synth.adc_stream(8, hop * 40, M, lut3, S, seed).numpy()
    direct = oracle.stream_run(adc, N, FS, S, band_ref.window_q15(N), lut3.reshape(3, -1), max_trig=128)
    assert direct["n_trig"].sum() > 30
    cap = Cs.scale8(adc)
    got = R.trigger16(cap, N, None, 131072, max_trig=128)
    assert np.array_equal(got["n_trig"], direct["n_trig"]) and np.array_equal(got["end"], direct["end"])
    hopped = R.trigger16(cap, N, hop, 131072, max_trig=128)  # hop * 40 samples: all of them
    assert np.array_equal(hopped["n_trig"], got["n_trig"]) and np.array_equal(hopped["end"], got["end"])
    # cap lies in [-32768, 32512]: offsets in [0, 255] stay inside int16
    shifted = (cap.astype(np.int32) + np.array([200, 17, 255], np.int32)).astype(np.int16)
    assert np.array_equal(shifted.astype(np.int32) - cap, np.broadcast_to([200, 17, 255], cap.shape))
    sh = R.trigger16(shifted, N, None, 131072, max_trig=128)
    assert np.array_equal(sh["n_trig"], got["n_trig"]) and np.array_equal(sh["end"], got["end"])


def test_a_larger_threshold_never_fires_earlier(lut3):
    """Within a ring period (from one ring start to the next trigger) the
    candidates that fire under a larger trigger_var are a subset of those that
    fire under a smaller one: run from the same ring start, the larger
    threshold's first trigger is not earlier.  Over a whole capture it gives
    fewer or equal triggers."""
    cap = Cs.small_capture(lut3, Cs.VAR_SEED)
    runs = [R.trigger16(cap, 1024, None, v, max_trig=128) for v in (0, 2, 131072, 1 << 20, 1 << 24, 28000000, 1 << 30)]
    for lo, hi in zip(runs, runs[1:]):
        assert (hi["n_trig"] <= lo["n_trig"]).all()
        assert (hi["end"][:, 0][hi["n_trig"] > 0] >= lo["end"][:, 0][hi["n_trig"] > 0]).all()  # both rings start at 0
    assert runs[0]["n_trig"].sum() > runs[2]["n_trig"].sum() > runs[5]["n_trig"].sum() > 0
    assert runs[6]["n_trig"].sum() == 0  # these bursts' variance, 2.7e7 over three mics, is far below 2^30


def test_full_scale_matches_python_int_arithmetic():
    """N/2-sample blocks of near-silence and full scale at N = 2048, M = 4: the
    largest pw an int16 ring of that frame length can hold.  int64 equals
    unbounded integers, and the values come close to the header's bounds
    (h^2 2^30 per mic: 2^50 at h = 1024) without passing them."""
    c = Cs.FULL_SCALE
    cap = R.full_scale_capture(c["ns"], c["T"], c["N"], c["M"], c["seed"])
    assert cap.min() == -32767 and cap.max() == 32767
    a = R.trigger16(cap, c["N"], None, 131072)
    b = R.trigger16(cap, c["N"], None, 131072, python_int=True)
    assert np.array_equal(a["n_trig"], b["n_trig"]) and np.array_equal(a["end"], b["end"])
    assert (a["n_trig"] >= 3).all()
    big = R.trigger16(cap, c["N"], None, 1 << 30, python_int=True)
    assert np.array_equal(big["end"], R.trigger16(cap, c["N"], None, 1 << 30)["end"])
    # the header's bounds on this capture: a fully loud half of a +-32767 stream
    h = c["N"] // 2
    x = cap[0].astype(object)
    e = int(a["end"][0, 1])
    s1, s2 = x[e - c["N"]:e - h].sum(0), (x[e - c["N"]:e - h] ** 2).sum(0)
    pw = [h * int(q) - int(p) ** 2 for p, q in zip(s1, s2)]
    assert all(0 <= v <= (h * h) << 30 for v in pw) and sum(pw) > 1 << 50  # 4 mics, each near 2^49
    assert (1 << 30) * h * h == 1 << 50  # the largest threshold at this frame length


# ---- synth.pcm16_stream

def test_pcm16_stream_is_deterministic_and_honours_dc(lut3):
    a = synth.pcm16_stream(4, 6000, 3, lut3, S, 11, dc=Cs.DC)
    b = synth.pcm16_stream(4, 6000, 3, lut3, S, 11, dc=Cs.DC)
    c = synth.pcm16_stream(4, 6000, 3, lut3, S, 12, dc=Cs.DC)
    z = synth.pcm16_stream(4, 6000, 3, lut3, S, 11)
    assert a.dtype == z.dtype and str(a.dtype) == "torch.int16" and tuple(a.shape) == (4, 6000, 3)
    assert a.is_contiguous()
    assert (a == b).all() and not (a == c).all()
    a, z = a.numpy().astype(np.int64), z.numpy().astype(np.int64)
    # the same draws plus the offset, before rounding: within one count where nothing clips
    ok = (np.abs(a) < 32767).all(-1) & (np.abs(z) < 32767).all(-1)
    assert ok.mean() > 0.9
    assert np.abs((a - z)[ok] - np.array(Cs.DC[:3])).max() <= 1
    assert np.abs(a.mean((0, 1)) - np.array(Cs.DC[:3])).max() < 100
    # bursts over a quiet floor: loud and quiet stretches both exist
    sd = z[0, :, 0].reshape(-1, 100).std(1)
    assert (sd > 1500).any() and (sd < 100).any()
    # a source that would leave int16 is clipped, not wrapped
    loud = synth.pcm16_stream(2, 6000, 3, lut3, S, 11, src_std=30000.0, dc=Cs.DC).numpy()
    assert loud.max() == 32767 and loud.min() == -32768


# ---- the GPU tests' seeds, on the float64 reference alone

def _report(name, ref, max_skip):
    records, gated, dropped, skipped, gap = R.stats(ref)
    print(f"{name}: {records} frames, {gated} gated, {dropped} streams dropped, {skipped} cells skipped "
          f"({skipped / max(gated, 1):.1%}), min map gap {gap:.3e}")
    assert dropped == 0
    assert skipped <= max_skip * max(gated, 1)
    return records, gated


def test_case1_and_case2_references_are_clear(oracle, lut3):
    win = band_ref.window_q15(1024)
    adc, cap = Cs.scaled8(lut3)
    records, gated = _report("scaled 8-bit", R.run(oracle, cap, 1024, FS, S, win, lut3), 0.0)
    assert records > 200 and gated > 100
    c2 = Cs.true16(lut3)
    assert np.abs(c2.astype(np.int64).mean((0, 1)) - np.array(Cs.DC[:3])).max() < 10
    r2 = R.run(oracle, c2, 1024, FS, S, win, lut3, trigger_var=Cs.TRUE16_VAR)
    records, gated = _report("true 16-bit", r2, 0.0)
    assert records > 200 and gated > 100
    # 8 bits of the same full scale lose these lags: the same frames truncated
    idx = [(s, i) for s in range(40) for i in range(r2["n_trig"][s])]
    tr = Cs.truncated8(c2)
    fr = np.stack([np.ascontiguousarray(tr[s, r2["end"][s, i] - 1024:r2["end"][s, i]].T) for s, i in idx])
    lt = pcm16_ref.gcc_phat_pcm16(fr, S, win)["lags"]
    differ = sum(bool((lt[b] != r2["lags"][s, i]).any()) for b, (s, i) in enumerate(idx))
    print(f"true 16-bit: truncation to 8 bits changes the lags of {differ} of {len(idx)} frames")
    assert differ > len(idx) // 2


@pytest.mark.parametrize("N,hop,M,hops,seed,max_skip", Cs.SHAPES)
def test_other_shapes_references_stay_within_their_caps(oracle, N, hop, M, hops, seed, max_skip):
    lut = Cs.lut_cpu(oracle, M)
    cap = Cs.shape_capture(lut, N, hop, M, hops, seed)
    _, gated = _report(f"{N} x {M} hop {hop} seed {seed}",
                       R.run(oracle, cap, N, FS, S, band_ref.window_q15(N), lut, hop=hop), max_skip)
    assert gated > 10


def test_small_case_references_are_clear(oracle, lut3):
    win = band_ref.window_q15(1024)
    w = band_ref.band_weights(1024, FS, 1000, 6000, 500)
    _report("ring wrap", R.run(oracle, Cs.small_capture(lut3, Cs.WRAP_SEED), 1024, FS, S, win, lut3), 0.0)
    band = Cs.small_capture(lut3, Cs.BAND_SEED, streams=8, hops=40)
    _report("band table", R.run(oracle, band, 1024, FS, S, win, lut3, w=w), 0.0)
    _report("band table cleared", R.run(oracle, band, 1024, FS, S, win, lut3), 0.0)
    _report("api", R.run(oracle, Cs.small_capture(lut3, Cs.API_SEED, hops=16), 1024, FS, S, win, lut3), 0.0)
    # the thresholds of the trigger_var test: the high one fires on under half the bursts
    cap = Cs.small_capture(lut3, Cs.VAR_SEED)
    n = [int(R.trigger16(cap, 1024, 512, v)["n_trig"].sum()) for v in Cs.TRIGGER_VARS]
    print(f"trigger_var {Cs.TRIGGER_VARS}: {n} triggers")
    assert n[0] > n[1] and 0 < n[2] < n[1] / 2
