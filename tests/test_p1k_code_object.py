"""Code-object checks of k_p1k_lean's launched shape (CPU suite, tools/co_audit.py).

The product library holds exactly one instantiation of k_p1k_lean<NW> -- the
one it launches; the other workgroup shape is in tdoa/libtdoa_ab.so only.  Two
workgroups per CU (NW = 4) or two waves per SIMD of one workgroup (NW = 8)
both need the kernel within 256 VGPRs per lane: no AGPR use (they come out of
the same 512-register file on gfx950), no scratch.
"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import co_audit as A  # noqa: E402

LIB = os.path.join(ROOT, "audio-triangulation_amd", "tdoa", "libtdoa.so")
AB_LIB = os.path.join(ROOT, "audio-triangulation_amd", "tdoa", "libtdoa_ab.so")

pytestmark = pytest.mark.skipif(not os.path.exists(f"{A.LLVM}/llvm-objdump"), reason="ROCm LLVM tools missing")


def _lean(lib):
    return {n: r for n, r in A.audit(lib).items() if "k_p1k_lean" in n}


def _within_budget(name, r):
    assert 0 < r["vgprs"] <= 256, (name, r["vgprs"])
    assert r["agprs"] == 0, (name, r["agprs"])
    assert r["private_segment"] == 0 and r["vgpr_spill"] == 0 and r["scratch"] == 0 and not r["dynamic_stack"], (name, r)


def test_product_holds_one_lean_instantiation_within_256_vgprs():
    assert os.path.exists(LIB), "build libtdoa.so first (__graft_entry__.build)"
    lean = _lean(LIB)
    assert len(lean) == 1, sorted(lean)
    for n, r in lean.items():
        _within_budget(n, r)
        # the 4-wave shape has no static LDS (no progress words): its 80 KiB
        # budget is the dynamic size alone
        if "k_p1k_leanILi4E" in n:
            assert r["lds_static"] == 0, r["lds_static"]


@pytest.mark.skipif(not os.path.exists(AB_LIB), reason="tdoa/libtdoa_ab.so not built (make ab)")
def test_ab_library_holds_both_shapes_within_256_vgprs():
    lean = _lean(AB_LIB)
    assert sorted(n[:len("_Z10k_p1k_leanILi4E")] for n in lean) == ["_Z10k_p1k_leanILi4E", "_Z10k_p1k_leanILi8E"], sorted(lean)
    for n, r in lean.items():
        _within_budget(n, r)
