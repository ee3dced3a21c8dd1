"""k_p1k_pcm16's code object within k_p1k_lean's budget (CPU suite, tools/co_audit.py).

The 16-bit kernel shares k_p1k_lean<4>'s body (csrc/tdoa_p1k_frames.inc), its
launch shape and its two workgroups per CU, and sits nearest the limit: 256
VGPRs per lane in the lean forms.  A deeper LDS read depth (P1K_TWM_* ...,
tdoa_phat1024.hip) that fits the 8-bit kernel may not fit this one, so it is
held to the same budget as tests/test_p1k_code_object.py holds k_p1k_lean:
at most 256 VGPRs, no AGPRs, no spill, no scratch.
"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import co_audit as A  # noqa: E402

LIB = os.path.join(ROOT, "audio-triangulation_amd", "tdoa", "libtdoa.so")

pytestmark = pytest.mark.skipif(not os.path.exists(f"{A.LLVM}/llvm-objdump"), reason="ROCm LLVM tools missing")


def test_product_pcm16_kernel_within_256_vgprs():
    assert os.path.exists(LIB), "build libtdoa.so first (__graft_entry__.build)"
    pcm = {n: r for n, r in A.audit(LIB).items() if "k_p1k_pcm16" in n}
    assert len(pcm) == 1, sorted(pcm)
    for n, r in pcm.items():
        assert 0 < r["vgprs"] <= 256, (n, r["vgprs"])
        assert r["agprs"] == 0, (n, r["agprs"])
        assert r["private_segment"] == 0 and r["vgpr_spill"] == 0 and r["scratch"] == 0 and not r["dynamic_stack"], (n, r)
        assert r["lds_static"] == 0, r["lds_static"]  # the 80 KiB budget is the dynamic size alone
