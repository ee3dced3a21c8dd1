"""The long-frame streaming cases (tests/stream_long_cases.py) on the float64
references alone: at every seed tests/test_gpu_stream_long.py uses, no stream
is dropped, no cell is skipped, the minimum map gap is above 2e-3 and at least
25 records are gated -- so the GPU comparisons run with max_dropped = 0 and
max_skip = 0 and cannot hide a failure.  And the ABI's new entry point."""
import os
import re

import numpy as np
import pytest

import band_ref
import stream16_ref
import stream_cont_ref
import stream_long_cases as Cs
import stream_phat_ref
from conftest import ROOT

FS, S = Cs.FS, Cs.S_LAG
TRIG = [(fmt, *c) for fmt in Cs.FMTS for c in Cs.TRIGGERED]
CONT = [(fmt, *c) for fmt in Cs.FMTS for c in Cs.CONTINUOUS[fmt]]


def _clear(ref, what):
    records, gated, dropped, skipped, gap = stream_phat_ref.stats(ref)
    print(f"{what}: {records} records, {gated} gated, {dropped} streams dropped, {skipped} cells skipped, "
          f"min map gap {gap:.3e}")
    assert dropped == 0
    assert skipped == 0
    assert gap > Cs.MIN_GAP
    assert gated >= Cs.MIN_GATED
    return gated, gap


def _triggered_ref(oracle, fmt, N, hop, M, hops, seed, w=None):
    lut = Cs.lut_cpu(oracle, M)
    cap = Cs.triggered_capture(fmt, lut, N, hop, M, hops, seed)
    assert cap.shape == (Cs.STREAMS, hop * hops, M) and cap.dtype == (np.int16 if fmt == "pcm16" else np.uint8)
    if fmt == "pcm16":
        return stream16_ref.run(oracle, cap, N, FS, S, band_ref.window_q15(N), lut, w=w, hop=hop)
    return stream_phat_ref.run(oracle, cap, N, FS, S, band_ref.window_q15(N), lut, w=w)


@pytest.mark.parametrize("fmt,N,hop,M,hops,seed", TRIG)
def test_triggered_references_are_clear(oracle, fmt, N, hop, M, hops, seed):
    """8 x 2048 seed 910: 36 / 36 gated (uint8 / int16), gaps 8.8e-2 / 8.2e-2;
    4 x 4096 seed 420: 29 / 28 gated, gap 1.56e-1 both."""
    _clear(_triggered_ref(oracle, fmt, N, hop, M, hops, seed), f"triggered {fmt} {M} x {N} seed {seed}")


@pytest.mark.parametrize("N,hop,M,hops,seed", Cs.TRIGGERED)
def test_band_references_are_clear(oracle, N, hop, M, hops, seed):
    """The triggered uint8 cases under the band 1000-6000 Hz, taper 500: gaps
    2.9e-3 (8 x 2048) and 5.1e-3 (4 x 4096)."""
    w = band_ref.band_weights(N, FS, *Cs.BAND)
    _clear(_triggered_ref(oracle, "adc8", N, hop, M, hops, seed, w=w), f"band {M} x {N} seed {seed}")


@pytest.mark.parametrize("fmt,N,hop,M,hops,seed,var", CONT)
def test_continuous_references_are_clear(oracle, fmt, N, hop, M, hops, seed, var):
    """8 x 2048 seed 910: 80 / 85 gated, gaps 1.2e-1 / 7.6e-2; 4 x 4096 seeds
    400 / 402: 70 / 70 gated, gap 1.56e-1 both."""
    lut = Cs.lut_cpu(oracle, M)
    cap = Cs.continuous_capture(fmt, lut, N, hop, M, hops, seed)
    assert cap.shape == (Cs.STREAMS, hop * hops, M) and cap.dtype == (np.int16 if fmt == "pcm16" else np.uint8)
    ref = stream_cont_ref.run(oracle, cap, N, FS, S, band_ref.window_q15(N), lut, hop, var)
    _clear(ref, f"continuous {fmt} {M} x {N} seed {seed}")


def test_header_declares_and_library_exports_the_kernel_name():
    import tdoa
    from tdoa import _lib
    txt = open(os.path.join(ROOT, "include", "tdoa.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"\bconst\s+char\s*\*\s*tdoa_stream_kernel\s*\(\s*const\s+tdoa_stream\s*\*\s*\w*\s*\)\s*;", code), \
        "include/tdoa.h does not declare tdoa_stream_kernel"
    assert "tdoa_stream_kernel" in _lib.EXPORTED_SYMBOLS
    L = tdoa.load()
    assert hasattr(L, "tdoa_stream_kernel") and L.tdoa_stream_kernel(None) is None
    assert L.tdoa_abi_version() == 1
    assert "k_f16_ring" in txt and "k_stream_ema_grid" in txt
