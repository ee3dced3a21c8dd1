"""The continuous-mode reference (tests/stream_cont_ref.py) pinned on the CPU,
on the captures the GPU tests use (tests/stream_cont_cases.py,
tests/test_gpu_stream_cont.py), and the ABI's new entry point."""
import os
import re

import numpy as np
import pytest

import band_ref
import stream16_ref
import stream_cont_cases as Cs
import stream_cont_ref as R
from conftest import ROOT

FS, S = Cs.FS, Cs.S_LAG
ALL = [(fmt, *c) for fmt in ("pcm16", "adc8") for c in Cs.CASES[fmt]]


# ---- the GPU tests' cases, on the float64 reference alone

@pytest.mark.parametrize("fmt,N,hop,M,hops,seed,var", ALL)
def test_case_references_stay_within_their_caps(oracle, fmt, N, hop, M, hops, seed, var):
    lut = Cs.lut_cpu(oracle, M)
    cap = Cs.capture(fmt, lut, N, hop, M, hops, seed)
    assert cap.shape == (Cs.STREAMS, hop * hops, M) and cap.dtype == (np.int16 if fmt == "pcm16" else np.uint8)
    ref = R.run(oracle, cap, N, FS, S, band_ref.window_q15(N), lut, hop, var)
    records, gated, dropped, skipped, gap = R.stats(ref)
    eligible = Cs.STREAMS * sum((h + 1) * hop >= N for h in range(hops))
    print(f"{fmt} {N} x {M} hop {hop} seed {seed}: {records} of {eligible} eligible frames listed, {gated} gated, "
          f"{dropped} streams dropped, {skipped} cells skipped ({skipped / max(gated, 1):.1%}), min map gap {gap:.3e}")
    assert dropped == 0
    assert skipped <= Cs.max_skip(M) * max(gated, 1)
    assert records >= 90
    assert records < eligible  # the gate holds the silences back


@pytest.mark.parametrize("fmt", ["pcm16", "adc8"])
def test_small_ring_case_reference_is_clear(oracle, fmt):
    c = Cs.SMALL
    lut = Cs.lut_cpu(oracle, c["M"])
    cap = Cs.capture(fmt, lut, c["N"], c["hop"], c["M"], c["hops"], Cs.SMALL_SEED[fmt])
    ref = R.run(oracle, cap, c["N"], FS, S, band_ref.window_q15(c["N"]), lut, c["hop"], Cs.SMALL_VAR[fmt])
    records, gated, dropped, skipped, gap = R.stats(ref)
    print(f"small {fmt}: {records} frames, {gated} gated, {dropped} dropped, {skipped} skipped, min map gap {gap:.3e}")
    assert dropped == 0 and skipped == 0 and gated > 10


@pytest.mark.parametrize("fmt", ["pcm16", "adc8"])
def test_band_case_reference_is_clear(oracle, fmt):
    """The first case of each ring type under the band table of the GPU test."""
    N, hop, M, hops, seed, var = Cs.CASES[fmt][0]
    lut = Cs.lut_cpu(oracle, M)
    cap = Cs.capture(fmt, lut, N, hop, M, hops, seed)
    w = band_ref.band_weights(N, FS, 1000, 6000, 500)
    records, gated, dropped, skipped, gap = R.stats(R.run(oracle, cap, N, FS, S, band_ref.window_q15(N), lut, hop, var, w=w))
    print(f"band {fmt}: {records} frames, {gated} gated, {dropped} dropped, {skipped} skipped, min map gap {gap:.3e}")
    assert dropped == 0 and skipped == 0 and gated > 100


def test_list_only_thresholds_list_fewer(oracle):
    """The thresholds of the GPU list-only test lie above the cases' own."""
    for fmt, case, var in (("pcm16", 0, 20000000), ("adc8", 1, 1200)):
        N, hop, M, hops, seed, v0 = Cs.CASES[fmt][case]
        cap = Cs.capture(fmt, Cs.lut_cpu(oracle, M), N, hop, M, hops, seed)
        assert 0 < R.active(cap, N, hop, var)["n_trig"].sum() < R.active(cap, N, hop, v0)["n_trig"].sum()


# ---- the rule itself

@pytest.mark.parametrize("N,M,hop,ns,T,seed", Cs.FULL_SCALE)
def test_full_scale_matches_python_int_arithmetic(N, M, hop, ns, T, seed):
    """N/2-sample blocks of near-silence and full scale: int64 equals unbounded
    integers at every threshold and the totals stay within the header's bound
    (M 2^54 <= 2^57 < 2^63)."""
    cap = stream16_ref.full_scale_capture(ns, T, N, M, seed)
    assert cap.min() == -32767 and cap.max() == 32767
    for var in (0, 1 << 20, 1 << 30):
        a = R.active(cap, N, hop, var)
        b = R.active(cap, N, hop, var, python_int=True)
        assert np.array_equal(a["n_trig"], b["n_trig"]) and np.array_equal(a["end"], b["end"])
        assert all(int(x) == int(y) for x, y in zip(a["total"].ravel(), b["total"].ravel()))
        assert all(0 <= int(t) <= M << 54 and int(t) < 1 << 63 for t in b["total"].ravel())
    assert max(int(t) for t in b["total"].ravel()) > 1 << (2 * int(np.log2(N)) + 28)  # near N^2 2^30 / 2 per mic
    assert var * N * N <= 1 << 54
    # 2^30 is half of full scale squared per mic pair: the +-32767 streams' frames (half loud, variance just
    # under 2^29 per mic) pass it with 4 mics and miss it with 2; the uniform streams never reach it
    assert b["n_trig"].sum() == (0 if M == 2 else R.active(cap, N, hop, 0)["n_trig"][0::2].sum())


def test_a_larger_threshold_lists_a_subset(oracle):
    lut = Cs.lut_cpu(oracle, 3)
    cap = Cs.capture("pcm16", lut, *Cs.PCM16_CASES[0][:5])
    runs = [R.active(cap, 1024, 512, v) for v in (0, 1000, 3000000, 20000000, 1 << 30)]
    for lo, hi in zip(runs, runs[1:]):
        for s in range(cap.shape[0]):
            assert set(hi["end"][s, :hi["n_trig"][s]]) <= set(lo["end"][s, :lo["n_trig"][s]])
    n = [int(r["n_trig"].sum()) for r in runs]
    assert n[0] > n[2] > n[3] > 0 and n[4] == 0


@pytest.mark.parametrize("N,hop,hops", [(1024, 512, 8), (1024, 384, 8), (256, 256, 4), (512, 128, 12)])
def test_zero_lists_exactly_the_hops_with_a_full_frame(N, hop, hops):
    """activity_var = 0: pw >= 0 always, so every hop with e >= N is listed --
    on noise, on a constant ring and on zeros alike -- and none before."""
    rng = np.random.default_rng(5)
    cap = rng.integers(0, 256, (3, hop * hops, 3)).astype(np.uint8)
    cap[1] = 200
    cap[2] = 0
    a = R.active(cap, N, hop, 0)
    want = [(h + 1) * hop for h in range(hops) if (h + 1) * hop >= N]
    assert want[0] == -(-N // hop) * hop
    for s in range(3):
        assert list(a["end"][s, :a["n_trig"][s]]) == want
    assert (a["total"][1] == 0).all() and R.active(cap, N, hop, 1)["n_trig"][1] == 0


def test_alternating_ring_sits_on_the_boundary():
    cap = Cs.alternating(4096, 3)[None]
    a = R.active(cap, 1024, 512, 30000)
    assert (a["total"][0, 1:] == 3 * 100 * 100 * 1024 * 1024).all()
    assert a["n_trig"][0] == 7 and R.active(cap, 1024, 512, 30001)["n_trig"][0] == 0


# ---- the ABI

def test_header_declares_and_library_exports_the_continuous_entry():
    import tdoa
    from tdoa import _lib
    txt = open(os.path.join(ROOT, "include", "tdoa.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+tdoa_stream_create_continuous\s*\(([^;]*)\)\s*;", code)
    assert m, "include/tdoa.h does not declare tdoa_stream_create_continuous"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 8 and "activity_var" in args[5] and "const void" in args[3]
    assert "tdoa_stream_create_continuous" in _lib.EXPORTED_SYMBOLS
    assert hasattr(tdoa.load(), "tdoa_stream_create_continuous")
    assert "sum_m pw(m) >= activity_var * N^2" in txt
