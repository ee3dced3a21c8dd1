"""Code-object guard (CPU suite) for the delay-and-sum beamformer's kernels:
k_beam and both k_beam_ring instantiations inside the built libtdoa.so, as
tests/test_sep_code_object.py holds k_sep (DESIGN.md "Code-object guard";
tools/co_audit.py): no private segment, no spills, no calls, no flat accesses,
one wait state behind a transcendental, no split-index scalar load.  The ring
kernels stage through a templated walk with a sink struct (tdoa_beam_dev.h); a
sink that fell out of line, or a per-thread array the compiler could not
resolve, would show here and in no numerical test.
"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import co_audit as A  # noqa: E402

LIB = os.path.join(ROOT, "audio-triangulation_amd", "tdoa", "libtdoa.so")

pytestmark = pytest.mark.skipif(not os.path.exists(f"{A.LLVM}/llvm-objdump"), reason="ROCm LLVM tools missing")


def _clean(r):
    return {k: r[k] for k in ("private_segment", "dynamic_stack", "vgpr_spill", "calls", "flat", "scratch")
            if r[k]} | {k: r[k][:2] for k in ("trans_use", "smem_split") if r[k]}


@pytest.fixture(scope="module")
def prod():
    assert os.path.exists(LIB), "build libtdoa.so first (__graft_entry__.build)"
    return A.audit(LIB)


def test_every_k_beam_is_there_and_clean(prod):
    names = [n for n in prod if "k_beam" in n]
    # k_beam, k_beam_ring<uint8_t>, k_beam_ring<int16_t>
    for part in ("k_beamE", "k_beam_ringIhE", "k_beam_ringIsE"):
        assert len([n for n in names if part in n]) == 1, (part, names)
    assert len(names) == 3
    for n in names:
        assert not _clean(prod[n]), (n, _clean(prod[n]))
        assert prod[n]["instructions"] > 500, n
        # 64 registers: 512 / 64 = 8 waves per SIMD, the next occupancy step on gfx950
        assert prod[n]["vgprs"] + prod[n]["agprs"] <= 64, (n, prod[n]["vgprs"])
