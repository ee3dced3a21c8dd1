"""The beamformer without a GPU: the FIR table, tdoa_beam_host (the host twin,
compiled from the inline functions k_beam and k_beam_ring run) against the
numpy restatement of the rule (tests/beam_ref.py) -- codes exactly, audio
within the fp32 summation bound the reference computes per sample -- a scene
with a known answer, every TDOA_ERR_INVALID case that needs no device, and a
program of its own under ASan + UBSan."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT

import tdoa
from tdoa import _lib

import beam_cases as BC
import beam_ref as R

# (geometry, N, B, Kt, seed)
CASES = [("triangle", 256, 7, 3, 11), ("square", 512, 6, 8, 12), ("circle", 256, 5, 1, 13)]
_cache = {}


def case(name, N, B, Kt, seed):
    """(geometry, mics, fs, c, frames, xy, count, reference): computed once, never modified."""
    key = (name, N, B, Kt, seed)
    if key not in _cache:
        bg, mics, fs, c = BC.geometry(name)
        frames, xy, count = BC.block_case(mics, B, N, Kt, seed, horizon=name == "square")
        _cache[key] = (bg, mics, fs, c, frames, xy, count, R.beam(mics, fs, c, BC.H, frames, xy, count))
    return _cache[key]


def test_fir_table():
    h, ref = tdoa.beam_fir(), R.fir64()
    assert h.dtype == np.float32 and h.shape == (32, 16) and (R.PHASES, R.TAPS) == h.shape
    assert np.abs(h.astype(np.float64) - ref).max() <= 2.0 ** -24  # one float rounding of a value <= 1
    unit = np.zeros(16, np.float32)
    unit[7] = 1.0
    assert h[0].tobytes() == unit.tobytes()  # phase 0: exactly the unit tap at k = 0
    assert np.abs(h.astype(np.float64).sum(axis=1) - 1.0).max() <= 16 * 2.0 ** -24
    assert np.abs(ref).max() <= 1.0
    # the phases delay: the centroid of phase q sits q / 32 after the unit tap, within the window's skew
    k = np.arange(-7, 9)
    assert np.abs((ref * k).sum(axis=1) - np.arange(32) / 32.0).max() < 0.02


def test_latency_is_the_mic_separation():
    for name in BC.GEOMS:
        bg, mics, fs, c = BC.geometry(name)
        A, D = tdoa.beam_latency(bg)
        assert (A, D) == R.latency(mics, fs, c) and A == D + 8
    bg, mics, fs, c = BC.geometry("square")
    assert tdoa.beam_latency(bg) == (39, 31)  # the diagonal is exactly 30 samples
    bg, mics, _, _ = BC.geometry("triangle")  # the reference triangle, centred on its centroid
    assert mics.shape == (3, 2) and np.abs(mics.sum(axis=0)).max() < 1e-6 and np.abs(mics).max() > 0.05


@pytest.mark.parametrize("name,N,B,Kt,seed", CASES)
def test_host_twin_equals_reference(name, N, B, Kt, seed):
    bg, mics, fs, c, frames, xy, count, ref = case(name, N, B, Kt, seed)
    got = tdoa.beam_host(bg, frames, xy, count)
    assert got["delays"].tobytes() == ref["delays"].tobytes()
    assert got["active"].tobytes() == ref["active"].tobytes()
    assert R.close(got["audio"], ref, mics.shape[0])
    assert (got["audio"][ref["active"] == 0] == 0).all()  # invalid targets are silent
    # count = NULL: every finite target is valid
    full = R.beam(mics, fs, c, BC.H, frames[:3], xy[:3], None)
    g2 = tdoa.beam_host(bg, frames[:3], xy[:3])
    assert g2["delays"].tobytes() == full["delays"].tobytes() and R.close(g2["audio"], full, mics.shape[0])
    assert full["active"].sum() == 3 * Kt - 1  # all but the NaN


def test_cases_contain_every_kind():
    """Asserted on the reference: a NaN target, count = 0, a target above a mic,
    one at the grid's corner, full-scale frames, and codes at both ends."""
    kinds = set()
    for name, N, B, Kt, seed in CASES:
        bg, mics, fs, c, frames, xy, count, ref = case(name, N, B, Kt, seed)
        _, D = R.latency(mics, fs, c)
        act, codes = ref["active"], ref["delays"]
        if np.isnan(xy[..., 0]).any() and (act[np.isnan(xy[..., 0])] == 0).all():
            kinds.add("nan")
        if (count == 0).any() and (act[count == 0] == 0).all() and (codes[count == 0] == -1).all():
            kinds.add("count0")
        if ((count > 0) & (count < Kt)).any():
            kinds.add("short")
        if (xy[0, 0] == mics[0]).all() and act[0, 0] and codes[0, 0, 0] == 0 and (codes[0, 0, 1:] > 0).all():
            kinds.add("above a mic")
        if abs(xy[1, 0, 0]) == np.float32(BC.GRID) and abs(xy[1, 0, 1]) == np.float32(BC.GRID) and act[1, 0]:
            kinds.add("corner")
        if (np.abs(frames[1].astype(np.int32)) == 32767).all():
            kinds.add("full scale")
            assert np.abs(ref["audio"][1][act[1] == 1]).max() > 10000
        valid = codes[act == 1]
        assert (valid.min(axis=-1) == 0).all() and valid.max() <= 32 * D  # the nearest mic has code 0
        if valid.max() >= 32 * D - 32:
            kinds.add("top code")
        if len(np.unique(valid & 31)) == 32:
            kinds.add("every phase")
    assert kinds == {"nan", "count0", "short", "above a mic", "corner", "full scale", "top code", "every phase"}


# ---------------------------------------------------------------- known answer
# beam error power / single-mic error power of the float64 reference at the
# true point over the interior n in [A, N - A) of the scene below: uncorrelated
# noise averages to 1 / M, the fractional-delay FIR passes a little less noise
# than a unit tap, and 2000 samples leave a few per cent of scatter.  The
# reference measures 0.295 (M = 3), 0.261 (M = 4) and 0.123 (M = 8), that is
# 0.88, 1.04 and 0.99 of 1 / M: it meets 1.25 / M for every M, so that bound holds.
KNOWN = [("triangle", (0.9, -0.4), (-1.2, 1.0)), ("square", (1.1, 0.3), (-1.5, -0.4)),
         ("circle", (-0.7, 1.3), (1.4, -1.1))]
KN = 2048


def known(name):
    key = ("known", name)
    if key not in _cache:
        bg, mics, fs, c = BC.geometry(name)
        true, other = dict((k, (t, o)) for k, t, o in KNOWN)[name]
        frames, clean = BC.scene(mics, fs, c, KN, true, seed=5)
        xy = np.array([[true, other]], np.float32)
        _cache[key] = (bg, mics, fs, c, frames, clean, xy, R.beam(mics, fs, c, BC.H, frames[None], xy))
    return _cache[key]


def _ratios(audio, frames, clean, A, near):
    sl = slice(A, KN - A)
    e_beam = np.mean((audio[0, 0, sl] - clean[sl]) ** 2)
    e_mic = np.mean((frames[near, sl].astype(np.float64) - clean[sl]) ** 2)
    return e_beam / e_mic, np.mean(audio[0, 0, sl] ** 2), np.mean(audio[0, 1, sl] ** 2)


@pytest.mark.parametrize("name", [k[0] for k in KNOWN])
def test_known_answer(name):
    bg, mics, fs, c, frames, clean, xy, ref = known(name)
    M = mics.shape[0]
    A, D = R.latency(mics, fs, c)
    codes = ref["delays"][0]
    near = int(np.argmin(codes[0]))
    assert codes[0, near] == 0 and np.abs(codes[0] - codes[1]).max() >= 64  # >= 2 samples apart on some mic
    # the reference first, then the host twin
    for what, audio in (("reference", ref["audio"]), ("host", tdoa.beam_host(bg, frames[None], xy)["audio"])):
        ratio, p_true, p_other = _ratios(audio.astype(np.float64), frames, clean, A, near)
        print(f"{name} {what}: error power ratio {ratio:.4f} (1/M = {1 / M:.4f}), "
              f"output power {p_true:.0f} at the source, {p_other:.0f} beside it")
        assert ratio <= 1.25 / M, (what, ratio)
        assert p_true > p_other, (what, p_true, p_other)


# ---------------------------------------------------------------- errors that need no device
def _host_args(Kt=2, N=64):
    bg, mics, _, _ = BC.geometry("triangle")
    frames = np.zeros((1, 3, N), np.int16)
    xy = np.zeros((1, Kt, 2), np.float32)
    audio = np.full((1, max(Kt, 1), N), 7.0, np.float32)
    return bg, frames, xy, audio


def test_invalid_arguments_need_no_device():
    L = tdoa.load()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    bg, frames, xy, audio = _host_args()
    out = _lib.BeamOutputs(p(audio), None, None, None)

    def fails(rc, *words):
        msg = L.tdoa_last_error()
        assert rc == -1 and all(w in msg for w in words), (rc, msg)
    fails(L.tdoa_beam_host(None, 64, p(frames), 1, None, p(xy), 2, C.byref(out)), b"tdoa_beam_host", b"NULL")
    fails(L.tdoa_beam_host(C.byref(bg), 64, None, 1, None, p(xy), 2, C.byref(out)), b"NULL")
    fails(L.tdoa_beam_host(C.byref(bg), 64, p(frames), 1, None, None, 2, C.byref(out)), b"NULL")
    fails(L.tdoa_beam_host(C.byref(bg), 64, p(frames), 1, None, p(xy), 2, None), b"NULL")
    none = _lib.BeamOutputs()
    fails(L.tdoa_beam_host(C.byref(bg), 64, p(frames), 1, None, p(xy), 2, C.byref(none)), b"audio")
    for Kt in (0, 9, -1):
        fails(L.tdoa_beam_host(C.byref(bg), 64, p(frames), 1, None, p(xy), Kt, C.byref(out)), b"Kt")
    fails(L.tdoa_beam_host(C.byref(bg), 0, p(frames), 1, None, p(xy), 2, C.byref(out)), b"block length")
    fails(L.tdoa_beam_host(C.byref(bg), 64, p(frames), -1, None, p(xy), 2, C.byref(out)), b"B")
    assert (audio == 7.0).all()  # nothing was written
    # geometries the beamformer refuses
    for field, bad in (("num_mics", 1), ("num_mics", 9), ("sample_rate_hz", 0), ("speed_of_sound", 0.0),
                       ("speed_of_sound", float("nan")), ("height_offset", -1.0)):
        g = _lib.BeamGeometry.from_buffer_copy(bytes(bg))
        setattr(g, field, bad)
        fails(L.tdoa_beam_host(C.byref(g), 64, p(frames), 1, None, p(xy), 2, C.byref(out)), b"beam geometry")
        fails(L.tdoa_beam_latency_of(C.byref(g), None, None), b"beam geometry")
    g = _lib.BeamGeometry.from_buffer_copy(bytes(bg))
    g.mic_xy[2] = float("inf")
    fails(L.tdoa_beam_latency_of(C.byref(g), None, None), b"mic 1")
    g = _lib.BeamGeometry.from_buffer_copy(bytes(bg))
    g.mic_xy[0] = 1000.0  # 1 km at 50 kHz: more than 65535 samples
    fails(L.tdoa_beam_latency_of(C.byref(g), None, None), b"separation")
    # the entry points that take a context or a pipeline: NULL is refused before any device call
    fails(L.tdoa_beam_latency(None, None, None), b"tdoa_beam_latency")
    fails(L.tdoa_get_beam_geometry(None, C.byref(g)), b"NULL")
    fails(L.tdoa_beam_batch(None, p(frames), 1, None, p(xy), 2, C.byref(out), None), b"tdoa_beam_batch", b"NULL")
    fails(L.tdoa_stream_beam(None, None, p(xy), 2, 2, C.byref(out), None), b"tdoa_stream_beam", b"NULL")
    fails(L.tdoa_beam_fir(None), b"tdoa_beam_fir")
    fails(L.tdoa_beam_geometry_of(None, C.byref(g)), b"NULL")
    cfg = _lib.Config()
    L.tdoa_config_default(C.byref(cfg))
    cfg.num_mics = 4  # no mic_xy
    fails(L.tdoa_beam_geometry_of(C.byref(cfg), C.byref(g)), b"mic_xy")


def test_python_faces_exist():
    names = ("tdoa_beam_fir", "tdoa_beam_geometry_of", "tdoa_beam_latency_of", "tdoa_beam_latency",
             "tdoa_get_beam_geometry", "tdoa_beam_batch", "tdoa_beam_host", "tdoa_stream_beam")
    hdr = open(os.path.join(ROOT, "include", "tdoa.h")).read()
    for name in names:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(tdoa.load(), name) and f"int {name}(" in hdr, name
    for macro in ("TDOA_BEAM_HALF 8", "TDOA_BEAM_PHASES 32", "TDOA_BEAM_MAX_TARGETS 8"):
        assert f"#define {macro}" in hdr
    assert "out of scope" in hdr  # moving targets inside a block
    assert C.sizeof(_lib.BeamGeometry) == 80 and C.sizeof(_lib.BeamOutputs) == 32
    from tdoa.localizer import Localizer
    from tdoa.stream import StreamPipeline
    assert callable(Localizer.beam_batch) and callable(StreamPipeline.beam)
    assert callable(tdoa.beam_host) and callable(tdoa.beam_fir)
    with pytest.raises(ValueError):
        tdoa.beam_host(BC.geometry("triangle")[0], np.zeros((1, 4, 16), np.int16), np.zeros((1, 1, 2), np.float32))


# ---------------------------------------------------------------- the program of its own
@pytest.fixture(scope="module")
def san_tool():
    r = subprocess.run(["make", "-C", PKG, "beam_host_san"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return os.path.join(ROOT, "tools", "beam_host_san")


@pytest.mark.parametrize("name,N,B,Kt,seed", CASES)
def test_program_of_its_own_under_asan_and_ubsan(san_tool, tmp_path, name, N, B, Kt, seed):
    bg, mics, fs, c, frames, xy, count, ref = case(name, N, B, Kt, seed)
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(bytes(bg) + np.array([N, B, Kt, 1], np.int32).tobytes())
        f.write(frames.tobytes() + count.tobytes() + xy.tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([san_tool, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True,
                       text=True, timeout=300, env=env)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.stdout.split() == ["sizeof", "80"]
    M = mics.shape[0]
    raw = open(tmp_path / "out.bin", "rb").read()
    na, nd, nc = B * Kt * N * 4, B * Kt * M * 4, B * Kt
    assert len(raw) == na + nd + nc + 8 + 32 * 16 * 4
    audio = np.frombuffer(raw[:na], np.float32).reshape(B, Kt, N)
    # the same functions as the library's build of the host twin: the same bits
    lib = tdoa.beam_host(bg, frames, xy, count)
    assert audio.tobytes() == lib["audio"].tobytes() and R.close(audio, ref, M)
    assert raw[na:na + nd] == ref["delays"].tobytes() and raw[na + nd:na + nd + nc] == ref["active"].tobytes()
    assert tuple(np.frombuffer(raw[na + nd + nc:na + nd + nc + 8], np.int32)) == R.latency(mics, fs, c)
    assert raw[na + nd + nc + 8:] == tdoa.beam_fir().tobytes()
