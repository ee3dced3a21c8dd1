"""A batch longer than one chunk of the spectrum scratch, on every chunked route.

Both two-pass launchers (tdoa_launch_gcc_phat_split, launch_r16) cut a batch
into chunks of the TDOA_SPEC_BYTES scratch and carry the chunk's first frame c0
into pass 1's row offset, pass 2's first frame and every output offset.  Each
case here is chunk + 3 frames of 8 mics, so the last three frames run in a
second chunk with c0 = chunk.  The per-frame arithmetic does not depend on the
batch position (tests/test_gpu_bench_sizes.py relies on the same property), so
rows [0, 8) and [chunk - 8, chunk + 3) of every output must equal a separate
launch of just those 19 frames bit for bit, with scores and lean; the 19-frame
launch passes test_gpu_gcc_phat.check_phat against float64, and every lag of the
big batch lies within +-S.  The chunk length comes from the header's define, so
a changed constant cannot leave a case on one chunk unnoticed.
"""
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gcc_phat_oracle as G  # noqa: E402
import pcm16_ref  # noqa: E402
import test_gpu_gcc_phat as T  # noqa: E402  (check_phat)
from conftest import PKG  # noqa: E402
from tdoa import synth  # noqa: E402
from tdoa.localizer import Localizer  # noqa: E402

M = 8
OUT_KEYS = ("lags", "gate", "cell", "xy", "max_Lf", "scores_f", "weighted_f", "xy_ls", "ls_rms")


def spec_bytes():
    txt = open(os.path.join(PKG, "csrc", "tdoa_shared.h")).read()
    m = re.search(r"^#define\s+TDOA_SPEC_BYTES\s+\(\(size_t\)\s*(\d+)\s*<<\s*(\d+)\)\s*$", txt, flags=re.M)
    assert m, "csrc/tdoa_shared.h: TDOA_SPEC_BYTES is not ((size_t)A << B) any more; teach this test the new form"
    return int(m.group(1)) << int(m.group(2))


# (N, variant, first kernel, bytes of scratch per mic row, frames per chunk at 128 MiB, with the refinement)
CASES = [(4096, "plain", "k_spec16", (4096 + 32) * 8, 508, True),          # launch_r16: k_spec16 / k_pair16
         (4096, "ones", "k_phat_spectra", 4096 * 8, 512, False),           # an all-ones table: k_phat_pairs<true>
         (4096, "pcm16", "k_phat_spectra_pcm16", 4096 * 8, 512, False),
         (1024, "plain", "k_phat_spectra", 1024 * 8, 2048, False)]         # k_phat_pairs<false>


@pytest.mark.parametrize("N,variant,kernel,row_bytes,chunk_128,ls", CASES)
def test_rows_around_the_chunk_seam(N, variant, kernel, row_bytes, chunk_128, ls):
    spec = spec_bytes()
    chunk = spec // (M * row_bytes)
    assert spec != 128 << 20 or chunk == chunk_128
    B = chunk + 3
    assert chunk >= 16 and B > chunk  # two chunks: c0 = 0 and c0 = chunk
    loc = Localizer(engine="gcc_phat", num_mics=M, frame_len=N, mic_xy=synth.circle_mics(M, 0.15),
                    sample_format="pcm16" if variant == "pcm16" else "adc8")
    if variant == "ones":
        loc.set_bin_weights(np.ones(N + 1, np.float32))
    assert loc.batch_kernel() == kernel and not loc.batch_grid_fused()
    S, lut = loc.dims.S, loc.lut()
    fr, cells, _ = synth.adc_frames(B, M, N, lut, S, 0xC0 + N + len(variant), device="cuda")
    if variant == "pcm16":
        fr = ((fr - 128) * 256).contiguous()  # the same signal over the 16-bit range
    assert fr.numel() * 2 > 33e6
    rows = torch.cat([torch.arange(0, 8), torch.arange(chunk - 8, chunk + 3)]).cuda()
    sub = fr[rows].contiguous()
    assert len(torch.unique(sub.view(19, -1), dim=0)) == 19 and len(torch.unique(cells)) > B // 2  # no two rows alike

    big = loc.localize(fr, scores=True, ls=ls)
    big_lean = loc.localize(fr, ls=ls)
    small = loc.localize(sub, scores=True, ls=ls)
    small_lean = loc.localize(sub, ls=ls)
    assert int(big["lags"].abs().max()) <= S and int(big_lean["lags"].abs().max()) <= S
    assert set(small) == {k for k in OUT_KEYS if ls or k not in ("xy_ls", "ls_rms")}
    for k in small:
        assert torch.equal(big[k][rows].contiguous().view(torch.uint8), small[k].view(torch.uint8)), (k, "scores call")
    for k in small_lean:
        assert torch.equal(big_lean[k][rows].contiguous().view(torch.uint8), small_lean[k].view(torch.uint8)), (k, "lean")
        assert torch.equal(small_lean[k].view(torch.uint8), small[k].view(torch.uint8)), (k, "lean vs scores")

    sub_np = sub.cpu().numpy()
    ref = pcm16_ref.gcc_phat_pcm16 if variant == "pcm16" else G.gcc_phat_batch
    exp = ref(sub_np, S, loc.window(), lut)
    got = {k: v.cpu().numpy() for k, v in small.items()}
    print(f"(8, {N}, {variant}) chunk {chunk}, B {B}: max |score err| {np.abs(got['scores_f'] - exp['scores_f']).max():.2e}")
    assert T.check_phat(got, exp) > 0.95
    loc.close()
