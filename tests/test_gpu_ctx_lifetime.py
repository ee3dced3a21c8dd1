"""Contexts and streaming pipelines give back what they allocate (-m gpu).

A context is created and destroyed 12 times; every third round also sets and
clears a band table (the on-demand 128 MiB spectrum scratch) and runs one batch
of 8 frames that asks only for the least-squares position, so the weighted-,
raw- / peak-score and cell scratch all grow.  The same for a 4-stream pipeline
on a DIRECT context, its steps replayed as captured graphs.

Afterwards the device's free memory (torch.cuda.mem_get_info after a
synchronise) must not be lower than before by 64 MiB or more: one leaked
split-shape context holds at least its 128 MiB spectrum scratch, so the bound
is half of the smallest leak that matters.  The last round's outputs equal the
first round's bit for bit.
"""
import pytest
import torch

from tdoa import synth
from tdoa.localizer import Localizer
from tdoa.stream import StreamPipeline

pytestmark = pytest.mark.gpu

ROUNDS = 12
LEAK_BOUND = 64 << 20


def free_bytes():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


@pytest.mark.parametrize("M,N,kernel", [(3, 1024, "k_p1k_lean"), (4, 4096, "k_frame16")])
def test_context_rounds_leak_nothing(M, N, kernel):
    mics = None if M == 3 else synth.square_mics(0.15)
    make = lambda: Localizer(engine="gcc_phat", num_mics=M, frame_len=N, mic_xy=mics)
    # outside the measurement: the frames, the output tensors (torch keeps their
    # blocks cached) and the first load of the kernels
    loc = make()
    assert loc.batch_kernel().startswith(kernel)
    fr, _, _ = synth.adc_frames(8, M, N, loc.lut(), loc.dims.S, synth.SEEDS[1], device="cuda")
    out = loc.alloc_outputs(8, grid=False, ls=True)
    loc.localize_into(fr, out)
    loc.close()
    before = free_bytes()
    first = last = None
    for r in range(ROUNDS):
        loc = make()
        if r % 3 == 0:
            loc.set_band(2000.0, 12000.0, 500.0)
            assert loc.batch_kernel() == "k_phat_spectra"
            loc.set_bin_weights(None)
            assert loc.batch_kernel().startswith(kernel)
            for t in out.values():
                t.zero_()
            loc.localize_into(fr, out)
            torch.cuda.synchronize()
            last = {k: v.cpu().numpy().copy() for k, v in out.items()}
            first = first or last
        loc.close()
    after = free_bytes()
    print(f"free before {before} after {after} lost {before - after}")
    assert before - after < LEAK_BOUND
    assert first is not last and set(first) == {"lags", "gate", "xy_ls", "ls_rms"}
    for k in first:
        assert first[k].tobytes() == last[k].tobytes(), k


def test_stream_rounds_leak_nothing():
    S, hop, hops = 4, 512, 16
    loc = Localizer(engine="direct")
    cap = synth.adc_stream(S, hop * hops, 3, loc.lut(), loc.dims.S, 17).cuda().contiguous()
    loc.close()

    def run(steps):
        loc = Localizer(engine="direct")
        pipe = StreamPipeline(loc, cap, hop=hop, use_graph=True)
        rec = []
        for _ in range(steps):
            pipe.step()
            rec.append(pipe.records())
        state = pipe.state() if steps else None
        pipe.close()
        loc.close()
        return rec, state

    run(hops)  # outside the measurement, as above
    before = free_bytes()
    first = last = None
    for r in range(ROUNDS):
        res = run(hops if r % 3 == 0 else 0)
        if r % 3 == 0:
            last = res
            first = first or res
    after = free_bytes()
    print(f"free before {before} after {after} lost {before - after}")
    assert before - after < LEAK_BOUND
    assert first is not last
    assert sum(len(h["stream_id"]) for h in first[0]) > 0  # something triggered
    for a, b in zip(first[0], last[0]):
        assert set(a) == set(b)
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), k
    assert first[1][0] == last[1][0]
    assert first[1][1].tobytes() == last[1][1].tobytes() and first[1][2].tobytes() == last[1][2].tobytes()
