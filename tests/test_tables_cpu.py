"""The host tables of a context, on the CPU (csrc/tdoa_tables.cpp through tools/tables_dump).

tools/tables_dump links the host-only table builder alone (no HIP runtime) and
writes every table of one config to files.  For six configs this module checks

  * each table's sha256 and every scalar against tests/golden/context_tables.json,
    recorded from the commit before the builder was split out of tdoa_create
    (so the split moved the code and changed no bit);
  * independently of the golden: the LUT against the C oracle, the tuples
    against the LUT, and the k_grid_bb / compact-layout tables against the
    properties the kernels rely on;
  * the same program built with ASan + UBSan (every report fatal, nothing
    preloaded) on the six configs and on rejected configs.
"""
import hashlib
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, PKG, ROOT
from tdoa import synth

TOOL = os.path.join(ROOT, "tools", "tables_dump")
TOOL_SAN = os.path.join(ROOT, "tools", "tables_dump_san")

DEFAULTS = dict(num_mics=3, frame_len=1024, sample_rate_hz=50000, max_shift=0, speed_of_sound=343.0, engine=0,
                grid_half_w=50, grid_half_h=50, grid_scale=24.0, height_offset=1.2, phat_eps=1e-12, mic_xy=None)
FLOATS = ("speed_of_sound", "grid_scale", "height_offset", "phat_eps")

CONFIGS = {
    # the default: 3 mics, N = 1024, fs 50000 (S = 46), 101 x 101 grid
    "default": {},
    "square4_2048": dict(num_mics=4, frame_len=2048, engine=1, mic_xy=synth.square_mics(0.15)),
    # bench config 4's geometry; P = 28: the P > 8 branches of bb_query and the compact layout
    "circle8_2048": dict(num_mics=8, frame_len=2048, engine=1, mic_xy=synth.circle_mics(8, 0.15)),
    # the reference triangle doubled, S = 63 (tests/test_gpu_gcc_phat.py): 6510 tuples
    "triangle2_s63": dict(sample_rate_hz=67600, engine=1,
                          mic_xy=np.array([[-0.132, -0.076], [0.132, -0.076], [0.0, 0.152]], np.float32)),
    # subsampled window, one partial 8 x 8 tile
    "n256_grid5": dict(frame_len=256, grid_half_w=2, grid_half_h=2),
    # 21 x 13 cells (no multiple of 8) close over the microphones: a tile's lags span more
    # than 15, so bb_wide is 1
    "near_wide": dict(grid_half_w=10, grid_half_h=6, grid_scale=12.0, height_offset=0.05),
}

# tests/test_abi.py::test_create_rejects_bad_config, and the window check that moved with them
REJECTED = {
    "frame_len_1000": (dict(frame_len=1000), "power of two"),
    "four_mics_no_xy": (dict(num_mics=4), "mic_xy is required"),
    "window_out_of_range": (dict(frame_len=256, window_q15=[40000] * 256), "window_q15[0] outside"),
}


def f32_hex(x):
    return "%08x" % struct.unpack("<I", struct.pack("<f", float(x)))[0]


def write_config(path, overrides):
    cfg = dict(DEFAULTS, **overrides)
    with open(path, "w") as f:
        for k, v in cfg.items():
            if v is None:
                continue
            if k == "mic_xy":
                f.write("mic_xy " + " ".join(f32_hex(x) for x in np.asarray(v, np.float32).ravel()) + "\n")
            elif k == "window_q15":
                f.write("window_q15 " + " ".join(str(int(x)) for x in v) + "\n")
            elif k in FLOATS:
                f.write(f"{k} {f32_hex(np.float32(v))}\n")
            else:
                f.write(f"{k} {int(v)}\n")
    return cfg


def run_tool(tool, tmp, name, overrides):
    out = os.path.join(tmp, name)
    os.makedirs(out, exist_ok=True)
    cfg = write_config(out + ".cfg", overrides)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([tool, out + ".cfg", out], capture_output=True, text=True, timeout=300, env=env)
    return cfg, out, r


FILES = {"win": np.int32, "prior": np.float32, "mic": np.float32, "lut": np.uint8, "tuples": np.uint32,
         "tuple_cell": np.int32, "tw": np.float32, "bb_img": np.uint8, "wc_chunks": np.uint32, "wc_lo": np.uint8,
         "wc_w": np.uint8, "wc_off": np.uint16, "pair_i": np.uint8, "pair_j": np.uint8, "fg": np.uint16}


@pytest.fixture(scope="module")
def tools():
    r = subprocess.run(["make", "-C", PKG, "tables_dump"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return TOOL, TOOL_SAN


@pytest.fixture(scope="module")
def dumps(tools, tmp_path_factory):
    """name -> (config, scalars, {table: array}, {table: sha256}), computed once and never modified."""
    tmp = str(tmp_path_factory.mktemp("tables"))
    res = {}
    for name, over in CONFIGS.items():
        cfg, out, r = run_tool(tools[0], tmp, name, over)
        assert r.returncode == 0, r.stdout + r.stderr
        meta = json.loads(r.stdout)
        arrs, sha = {}, {}
        for f, dt in FILES.items():
            raw = open(os.path.join(out, f + ".bin"), "rb").read()
            sha[f] = hashlib.sha256(raw).hexdigest()
            arrs[f] = np.frombuffer(raw, dt)
            arrs[f].flags.writeable = False
        res[name] = (cfg, meta, arrs, sha)
    return res


@pytest.mark.parametrize("name", list(CONFIGS))
def test_tables_equal_the_recorded_parent(dumps, name):
    want = json.load(open(os.path.join(GOLDEN, "context_tables.json")))["configs"][name]
    _, meta, _, sha = dumps[name]
    assert meta == want["scalars"]
    assert sha == want["sha256"]


def test_the_configs_reach_the_intended_branches(dumps):
    m = {k: v[1] for k, v in dumps.items()}
    assert m["default"]["S"] == 46 and m["default"]["G"] == 101 * 101
    assert m["circle8_2048"]["P"] == 28
    assert m["triangle2_s63"]["S"] == 63 and m["triangle2_s63"]["U"] == 6510
    assert m["n256_grid5"]["NT"] == 1 and m["n256_grid5"]["G"] == 25
    assert m["near_wide"]["wide"] == 1 and m["near_wide"]["W"] % 8 and m["near_wide"]["H"] % 8
    assert all(m[k]["wide"] == 0 for k in ("default", "square4_2048", "circle8_2048", "n256_grid5"))


def lags_of(tuples, U, TW, P):
    """[U][P] lag indices out of the packed tuple words (byte p & 3 of word p / 4)."""
    t = tuples.reshape(U, TW)
    return np.stack([(t[:, p // 4] >> (8 * (p & 3))) & 0xFF for p in range(P)], 1).astype(np.int64)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_lut_is_the_oracles_and_tuples_are_its_distinct_columns(dumps, oracle, name):
    cfg, m, a, _ = dumps[name]
    M, P, G, U, TW = m["M"], m["P"], m["G"], m["U"], m["TW"]
    mic = a["mic"].reshape(M, 2)
    if cfg["mic_xy"] is None:
        assert (mic == oracle.microphones_ref()).all()
    else:
        assert mic.tobytes() == np.asarray(cfg["mic_xy"], np.float32).tobytes()
    lut = oracle.build_lut(mic, cfg["grid_half_w"], cfg["grid_half_h"], cfg["grid_scale"], cfg["height_offset"],
                           cfg["speed_of_sound"], cfg["sample_rate_hz"], m["S"])
    assert a["lut"].tobytes() == np.ascontiguousarray(lut, np.uint8).tobytes()
    cols = a["lut"].reshape(P, G).T  # [G][P]
    seen, first = {}, []
    for cell in range(G):
        if seen.setdefault(cols[cell].tobytes(), cell) == cell:
            first.append(cell)
    assert U == len(first) and (a["tuple_cell"] == np.array(first, np.int32)).all()
    assert (lags_of(a["tuples"], U, TW, P) == cols[first]).all()
    # bytes past pair P - 1 of the last word are zero
    if P % 4:
        assert (a["tuples"].reshape(U, TW)[:, -1] >> (8 * (P % 4)) == 0).all()


def bb_sections(m, a):
    img, at = a["bb_img"], m["bb_at"]
    NT, P, U, TW = m["NT"], m["P"], m["U"], m["TW"]
    assert all(x % 16 == 0 for x in at) and at[0] == 0 and sorted(at) == at and len(img) % 16 == 0

    def sec(i, dt, n):
        b = img[at[i]:at[i] + n * np.dtype(dt).itemsize]
        assert len(b) == n * np.dtype(dt).itemsize
        return np.frombuffer(b.tobytes(), dt)
    return (sec(0, np.int32, 2 * NT).reshape(NT, 2), sec(1, np.uint16, NT * P).reshape(NT, P),
            sec(2, np.uint32, U * TW), sec(3, np.int32, U), sec(4, np.uint16, NT * P).reshape(NT, P))


def bb_layout(P, K):
    """tdoa_bb_layout.h restated: score row stride, scores per wave, grouped-level row stride."""
    ks = (K + 3) & ~3 if P > 8 else K
    return ks, (P * ks + 3) & ~3, (96 if K <= 96 else 128)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_tile_image(dumps, name):
    _, m, a, _ = dumps[name]
    NT, P, U, TW, K, W = m["NT"], m["P"], m["U"], m["TW"], m["K"], m["W"]
    tile, rng, tup, uidx, qry = bb_sections(m, a)
    assert sorted(uidx.tolist()) == list(range(U))
    assert (tup.reshape(U, TW) == a["tuples"].reshape(U, TW)[uidx]).all()
    # entries tile the regrouped order, at most 64 tuples each, all of one 8 x 8 block of cells
    assert tile[0, 0] == 0 and (tile[1:, 0] == tile[:-1, 0] + tile[:-1, 1]).all() and tile[-1].sum() == U
    assert tile[:, 1].min() >= 1 and tile[:, 1].max() <= 64
    lags = lags_of(tup, U, TW, P)
    cells = a["tuple_cell"][uidx]
    ks, pk, row = bb_layout(P, K)
    wide = 0
    for t in range(NT):
        s = slice(tile[t, 0], tile[t, 0] + tile[t, 1])
        blk = (cells[s] // W // 8) * 100000 + cells[s] % W // 8
        assert (blk == blk[0]).all()
        lo, hi = lags[s].min(0), lags[s].max(0)
        assert ((rng[t] & 0xFF) == lo).all() and ((rng[t] >> 8) == hi).all()
        for p in range(P):
            q, n = int(qry[t, p]), int(hi[p] - lo[p] + 1)
            if (q & 0x1FFF) == 0x1FFF:
                wide = 1
                assert n > 15  # lags never leave [0, K): only the width makes a query wide here
                continue
            # the query decodes to two windows of 2^lv lags inside [lo, hi] that cover it
            o1, d = q & 0x1FFF, q >> 13
            lv = n.bit_length() - 1
            assert 1 <= n <= 15 and d == n - (1 << lv)
            if lv == 0:
                base = p * ks
            elif P <= 8:
                base = lv * pk + p * K
            else:
                base = pk + (lv - 1) * 4 * row + (p & 3) * row
            w1 = o1 - base
            w2 = w1 + d
            assert w1 == lo[p] and w2 + (1 << lv) - 1 == hi[p] and w2 <= w1 + (1 << lv)
    assert wide == m["wide"] == m["kp"]["bb_wide"] and NT == m["kp"]["bb_NT"]


@pytest.mark.parametrize("name", list(CONFIGS))
def test_compact_layout(dumps, name):
    _, m, a, _ = dumps[name]
    P, U, TW, K = m["P"], m["U"], m["TW"], m["K"]
    assert m["wc_ok"] == 1
    lo, w, off = a["wc_lo"].astype(int), a["wc_w"].astype(int), a["wc_off"].astype(int)
    lags = lags_of(a["tuples"], U, TW, P)
    assert (lags >= lo).all() and (lags < lo + w).all() and (lo + w <= K).all()
    assert (off % 4 == 0).all() and off[0] == 0 and (np.diff(off) > 0).all()
    assert (np.diff(off) == (w[:-1] + 3) // 4 * 4).all() and m["wc_CK"] == off[-1] + (w[-1] + 3) // 4 * 4
    if P > 8:
        assert (lo % 4 == 0).all()
    # the chunks: every pair's range in steps of 4 lags, addressed in k_grid_bb's score rows
    ks = bb_layout(P, K)[0]
    want = [(p * ks + lo[p] + j) | (min(4, w[p] - j) << 16) for p in range(P) for j in range(0, w[p], 4)]
    assert a["wc_chunks"].tolist() == want and m["wc_nch"] == len(want)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_scalars_and_small_tables(dumps, oracle, name):
    cfg, m, a, _ = dumps[name]
    M, N, S, K = m["M"], m["N"], m["S"], m["K"]
    assert (m["P"], K, m["TW"]) == (M * (M - 1) // 2, 2 * S + 1, (m["P"] + 3) // 4)
    assert (m["W"], m["H"]) == (2 * cfg["grid_half_w"] + 1, 2 * cfg["grid_half_h"] + 1) and m["G"] == m["W"] * m["H"]
    pairs = [(i, j) for i in range(M) for j in range(i + 1, M)]
    assert list(zip(a["pair_i"].tolist(), a["pair_j"].tolist())) == pairs
    assert a["prior"].tolist() == [np.float32(oracle.prior_scale(d * d)) for d in range(K)]
    assert len(a["win"]) == N and a["win"].min() >= 0 and a["win"].max() == 32767
    kp = m["kp"]
    assert kp["sbase"] % 2 == 0 and kp["sbase"] <= -S and kp["sbase"] + 16 * kp["T"] > S
    assert kp["NSEG"] * 64 == N // 2 and kp["RS"] == N // 2 + 2 * kp["PADW"] and kp["PADW"] % 4 == 0
    assert 1 << kp["log2N"] == N
    k = np.arange(N)
    tw = a["tw"].astype(np.float64)
    assert np.abs(tw[0:2 * N:2] - np.cos(2 * np.pi * k / N)).max() < 1e-7
    assert np.abs(tw[1:2 * N:2] + np.sin(2 * np.pi * k / N)).max() < 1e-7
    assert m["tw2_at"] == 2 * N and m["r16_at"] == 4 * N + 2 and len(tw) == m["r16_at"] + 1536


def test_sanitized_build_is_clean_and_rejects_bad_configs(tools, dumps, tmp_path):
    for name, over in CONFIGS.items():
        _, out, r = run_tool(tools[1], str(tmp_path), name, over)
        assert r.returncode == 0, (name, r.stdout[-500:], r.stderr[-3000:])
        assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr
        assert json.loads(r.stdout) == dumps[name][1]
        for f in FILES:
            assert hashlib.sha256(open(os.path.join(out, f + ".bin"), "rb").read()).hexdigest() == dumps[name][3][f]
    for name, (over, msg) in REJECTED.items():
        _, _, r = run_tool(tools[1], str(tmp_path), name, over)
        assert r.returncode == 1, (name, r.stdout[-500:], r.stderr[-3000:])
        assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr
        err = json.loads(r.stdout)
        assert err["error"] == -1 and msg in err["message"]
