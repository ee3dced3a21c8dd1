#!/usr/bin/env python3
"""Every output byte of the config-2 kernels (k_p1k_lean, k_p1k_pcm16) on a fixed
set of small batches: recorded once from the parent commit's library, compared
byte for byte by tests/test_gpu_p1k_parent_bytes.py.

    TDOA_LIB=/path/to/parent/libtdoa.so python tools/p1k_parent_bytes.py [out.npz]
        (default out: tests/golden/p1k_parent_bytes.npz; TDOA_LIB as tools/ab_libs.sh)

A change that only moves loads and waits leaves every float operation, operand
order and association as it was, so every output is the same bytes: the file
is the parent's answer, not an oracle's.

Cases: 3 x 1024 GCC_PHAT; both sample formats (adc8 -> k_p1k_lean, pcm16 ->
k_p1k_pcm16); the default PHAT floor and phat_eps = 1e-4; batches of 1, 2, 7, 8,
9 and 17 frames (one half-wave, one wave, a partial workgroup of the 4-wave
shape, a full one, one frame past one and past two workgroups).  A batch is
the first B frames of one pool of 17: ADC-like, full-range int16, all-zero
and single-click frames in turn, so each kind meets every place in a wave.
A band (tdoa_set_band_hz) sends a context to the two-pass kernels, not to
these: run() asserts that, and the file holds no banded case.

Stored per case: lags, gate, cell, xy, max_Lf whole; scores_f and weighted_f
(2 x 44 frames x 3 x 93 floats per format and floor: 390 KB in all) as the
SHA-256 of their bytes, which keeps the file within a few KB and the check a
check of every byte.
"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "audio-triangulation_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

BATCHES = (1, 2, 7, 8, 9, 17)
FLOORS = (None, 1e-4)
FORMATS = {"adc8": "k_p1k_lean", "pcm16": "k_p1k_pcm16"}
WHOLE = ("lags", "gate", "cell", "xy", "max_Lf")
DIGEST = ("scores_f", "weighted_f")
KEYS = WHOLE + DIGEST
GOLDEN = os.path.join(ROOT, "tests", "golden", "p1k_parent_bytes.npz")


def pool(lut):
    """The 17 frames, int16 [17][3][1024] (CPU tensor)."""
    import torch
    import known_answer as KA
    from tdoa import synth
    adc = synth.adc_frames(8, 3, 1024, lut.reshape(3, 101, 101), 46, 0x5EED17)[0]
    full = synth.full_range_frames(5, 3, 1024, 0xBEE)
    zero = torch.zeros((1, 3, 1024), dtype=torch.int16)
    click = torch.from_numpy(KA.click_frames([[0, 5, 9], [12, 0, 3]], 3, 1024))
    kinds = [adc[0:1], full[0:1], zero, click[0:1], adc[1:2], full[1:2], adc[2:3], click[1:2], full[2:3],
             adc[3:4], zero, adc[4:5], full[3:4], adc[5:6], adc[6:7], full[4:5], adc[7:8]]
    fr = torch.cat(kinds).contiguous()
    assert fr.shape == (17, 3, 1024)
    return fr


def run():
    """name -> array for every case, from the library in force (TDOA_LIB or the product)."""
    import torch
    from tdoa.localizer import Localizer
    res = {}
    for eps in FLOORS:
        kw = {} if eps is None else {"phat_eps": eps}
        for fmt, kernel in FORMATS.items():
            ph = Localizer(engine="gcc_phat", sample_format=fmt, **kw)
            assert ph.batch_kernel() == kernel, (fmt, ph.batch_kernel())
            fr = pool(ph.lut()).cuda()
            for B in BATCHES:
                out = ph.localize(fr[:B].contiguous(), scores=True)
                torch.cuda.synchronize()
                assert set(out) == set(KEYS), sorted(out)
                for k in WHOLE:
                    res[f"{eps}/{fmt}/{B}/{k}"] = out[k].cpu().numpy()
                for k in DIGEST:
                    a = np.ascontiguousarray(out[k].cpu().numpy())
                    assert a.dtype == np.float32 and a.shape == (B, 3, ph.dims.K), (k, a.dtype, a.shape)
                    res[f"{eps}/{fmt}/{B}/{k}"] = np.frombuffer(hashlib.sha256(a.tobytes()).digest(), np.uint8)
            ph.close()
    # a band takes a context off these kernels: nothing to record for it
    ph = Localizer(engine="gcc_phat", band_hz=(300.0, 8000.0))
    assert not ph.batch_kernel().startswith("k_p1k"), ph.batch_kernel()
    ph.close()
    return res


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    r = run()
    np.savez_compressed(path, **r)
    print(f"wrote {path}: {len(r)} arrays, {os.path.getsize(path)} bytes, library {os.environ.get('TDOA_LIB', '(product)')}")
