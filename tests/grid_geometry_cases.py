"""The geometry sweep's cases (TEST INFRASTRUCTURE ONLY): one table for
tests/test_grid_geometry_cpu.py, which pins each case's host tables through
tools/tables_dump, and tests/test_gpu_grid_geometry.py, which runs every grid
route on them.

Every other GPU test of a grid solve uses a square grid at grid_scale 24,
height_offset 1.2 and speed_of_sound 343, where half_w == half_h and W == H:
there a swapped half_w / half_h, a /H in place of a /W or a baked-in constant
leaves every byte as it is.  The cases below are non-square, degenerate (1 x 1,
1 x 9), off the default physics, and chosen to reach the branches of
k_p1k_lean's pruned scan that the default table (2469 tuples, 39 rows, sort
pair 0, rows of <= 4 lags, K = 93) never takes.

Unless `kw` says otherwise a case is 3 mics x 1024 samples on the reference
triangle at 50 kHz with max_shift 0 (S = fs * 32 / 34300).  `rows`, `pair` and
`width` are those of the p1k_prune section (None: no section is looked at);
`wide` is the branch-and-bound table's wide flag; `kernel` / `fused` are
Localizer.batch_kernel() / batch_grid_fused() of the GCC_PHAT engine.
"""
import numpy as np

from tdoa import synth

SQ4 = dict(num_mics=4, frame_len=2048, mic_xy=synth.square_mics(0.15))
C8 = dict(num_mics=8, frame_len=2048, mic_xy=synth.circle_mics(8, 0.15))
LEAN, FRAME16, FUSED_1024 = "k_p1k_lean", "k_frame16", "k_gcc_phat_1024"


def _case(kw, WH, SK, U, rows, pair, width, wide, kernel, fused):
    return dict(kw=kw, W=WH[0], H=WH[1], S=SK[0], K=SK[1], U=U, rows=rows, pair=pair, width=width, wide=wide,
                kernel=kernel, fused=fused)


CASES = {
    # one tuple, one row (the grid of tdoa_reference_abi.cpp)
    "g1x1": _case(dict(grid_half_w=0, grid_half_h=0), (1, 1), (46, 93), 1, 1, 0, 1, 0, LEAN, True),
    # W = 1: cell % W = 0, all position in y
    "g1x9": _case(dict(grid_half_w=0, grid_half_h=4), (1, 9), (46, 93), 9, 1, 0, 1, 0, LEAN, True),
    # two trips of the bound loop, sort pair 2
    "g15x9": _case(dict(grid_half_w=7, grid_half_h=4), (15, 9), (46, 93), 101, 2, 2, 5, 0, LEAN, True),
    # four trips of the bound loop
    "near": _case(dict(grid_half_w=10, grid_half_h=6, grid_scale=12.0, height_offset=0.05), (21, 13), (46, 93),
                  111, 2, 0, 14, 1, LEAN, True),
    # U = 3 * 64: the last row is full
    "g25x11": _case(dict(grid_half_w=12, grid_half_h=5), (25, 11), (46, 93), 192, 3, 2, 4, None, LEAN, True),
    # a tall grid, full last row
    "g13x29": _case(dict(grid_half_w=6, grid_half_h=14), (13, 29), (46, 93), 256, 4, 0, 3, None, LEAN, True),
    "tall": _case(dict(grid_half_w=25, grid_half_h=40), (51, 81), (46, 93), 1659, 26, 0, 3, 0, LEAN, True),
    "wide48k": _case(dict(sample_rate_hz=48000, grid_half_w=40, grid_half_h=25), (81, 51), (44, 89), 1592, 25, 2, 3,
                     0, LEAN, True),
    # K = 17: the LUT clamps most cells
    "ms8": _case(dict(max_shift=8), (101, 101), (8, 17), 538, 9, 0, 4, 0, LEAN, True),
    # non-default c.  3272 tuples are more than k_p1k_lean stages (p1k_fits below): the generic fused kernel
    "sos280": _case(dict(speed_of_sound=280.0), (101, 101), (46, 93), 3272, 52, 0, 3, 0, FUSED_1024, True),
    # non-default c on k_p1k_lean
    "sos400": _case(dict(speed_of_sound=400.0), (101, 101), (46, 93), 1991, 32, 0, 2, 0, LEAN, True),
    # K = 127 (lag slot 126 beside the -inf slot 127) and 40 rows, the largest table k_p1k_lean stages
    "s63_65": _case(dict(sample_rate_hz=67600, grid_half_w=32, grid_half_h=32), (65, 65), (63, 127), 2512, 40, 0, 3,
                    0, LEAN, True),
    # the same edge, non-square, pair 2, and U = 2560 exactly: 40 full rows, no padding tuple in the image
    "s63_141x45": _case(dict(sample_rate_hz=67600, grid_half_w=70, grid_half_h=22), (141, 45), (63, 127), 2560, 40,
                        2, 3, 0, LEAN, True),
    # two more columns: 2562 tuples, 41 rows, one row past the edge -> the generic fused kernel
    "s63_143x45": _case(dict(sample_rate_hz=67600, grid_half_w=71, grid_half_h=22), (143, 45), (63, 127), 2562, 41,
                        2, 3, 0, FUSED_1024, True),
    # K = 127 on tables of 55 rows: the generic fused kernel, square and non-square (sort pair 2)
    "s63_91": _case(dict(sample_rate_hz=67600, grid_half_w=45, grid_half_h=45), (91, 91), (63, 127), 3512, 55, 0, 2,
                    0, FUSED_1024, True),
    "s63_121x75": _case(dict(sample_rate_hz=67600, grid_half_w=60, grid_half_h=37), (121, 75), (63, 127), 3491, 55,
                        2, 3, 0, FUSED_1024, True),
    # the generic fused kernel at a U other than 6510 (a prune section of 59 rows exists)
    "s63_full": _case(dict(sample_rate_hz=67600), (101, 101), (63, 127), 3771, 59, None, None, 0, FUSED_1024, True),
    "rect18": _case(dict(grid_half_w=30, grid_half_h=18, grid_scale=18.0, height_offset=0.9), (61, 37), (46, 93),
                    1324, 21, 2, 3, 1, LEAN, True),
    # k_grid_bb's tiles (NT 77) with W != H, W % 8 = 1, H % 8 = 3, and the transpose
    "sq4_wide": _case(dict(SQ4, grid_half_w=40, grid_half_h=25), (81, 51), (46, 93), 3029, None, None, None, 0,
                      FRAME16, False),
    "sq4_tall": _case(dict(SQ4, grid_half_w=25, grid_half_h=40), (51, 81), (46, 93), 3029, None, None, None, 0,
                      FRAME16, False),
    # the wide fallback (the exhaustive k_grid) on W != H
    "sq4_rect18": _case(dict(SQ4, grid_half_w=30, grid_half_h=18, grid_scale=18.0, height_offset=0.9), (61, 37),
                        (46, 93), 1835, None, None, None, 1, FRAME16, False),
    # P = 28: the grouped P > 8 bound pass
    "c8_wide": _case(dict(C8, grid_half_w=40, grid_half_h=25), (81, 51), (46, 93), 4117, None, None, None, 0,
                     FRAME16, False),
    # one partial tile (NT = 1), U < a wave
    "c8_7x3": _case(dict(C8, grid_half_w=3, grid_half_h=1), (7, 3), (46, 93), 21, None, None, None, 0, FRAME16,
                    False),
    # the generic kernel, then the exhaustive k_grid
    "n512_tall18": _case(dict(frame_len=512, grid_half_w=18, grid_half_h=30, grid_scale=18.0, height_offset=0.9),
                         (37, 61), (46, 93), 1346, None, None, None, 1, "k_gcc_phat", False),
}

LEAN_CASES = [n for n, c in CASES.items() if c["kernel"] == LEAN]
P1K_SHAPED = [n for n, c in CASES.items() if c["kw"].get("num_mics", 3) == 3 and c["kw"].get("frame_len", 1024) == 1024]
# the 2 x 4096 DIRECT case: frames exceed k_direct_mfma's staging registers -> the VALU k_direct and the int64 k_grid_bb
TWO_MICS_WIDE = dict(num_mics=2, frame_len=4096, mic_xy=np.array([[-0.066, 0.0], [0.066, 0.0]], np.float32),
                     grid_half_w=40, grid_half_h=25)


# The asymmetric known answer: offsets (dx, dy) from the grid's centre, in cells.  The cell at
# (dx, dy) lies at (dx, dy) / scale metres and its mirror image under x <-> y at (dy, dx) / scale;
# both lie inside the grid, each is the first cell of its lag tuple, the tuples differ, and each
# tuple is consistent (lag_12 = lag_02 - lag_01), so integer-delay click frames have exactly
# that cell as their answer (tests/test_grid_geometry_cpu.py checks all of this on the oracles).
MIRROR = {"tall": (17, 7), "wide48k": (20, 3)}

# The streaming captures: six streams, the sizes of the smallest 3-mic cases of
# tests/test_gpu_stream_phat.py (24 hops of 512) and tests/stream_cont_cases.py (ADC8_CASES[0]).
# On the float64 references alone no stream is dropped and no cell skipped at these seeds
# (tests/test_grid_geometry_cpu.py), so the caps of those modules' smallest cases (0 and 0) hold.
STREAM_PHAT = dict(case="wide48k", N=1024, hop=512, hops=24, seed=424)
STREAM_DIRECT = dict(case="wide48k", N=1024, hop=512, hops=24, seed=23)
STREAM_CONT = dict(case="rect18", N=1024, hop=512, hops=48, seed=31, activity_var=600)


def shape(name):
    """(M, N, B): mics, samples, and the frames of a batch (48, or 24 for 8 mics)."""
    kw = CASES[name]["kw"]
    M = kw.get("num_mics", 3)
    return M, kw.get("frame_len", 1024), 24 if M == 8 else 48


def adc_batch(name, lut, device="cpu"):
    """The case's integer-delay ADC frames (synth.adc_frames on the case's own LUT), int16 [B][M][N]."""
    M, N, B = shape(name)
    return synth.adc_frames(B, M, N, lut, CASES[name]["S"], 40 + N + M, device=device)[0]


def mirror_cells(name):
    """The two cells of MIRROR[name] (row-major) and their coordinates from the closed form, float32 [2][2]."""
    hw, hh, scale = geometry(name)[:3]
    dx, dy = MIRROR[name]
    assert dx != dy and max(abs(dx), abs(dy)) <= min(hw, hh)
    W = 2 * hw + 1
    cells = np.array([(hh - dy) * W + hw + dx, (hh - dx) * W + hw + dy])
    return cells, np.array([[dx, dy], [dy, dx]], np.float32) / np.float32(scale)


def mirror_delays(name, lut):
    """Per mirror cell the integer mic delays [0, lag_01, lag_02] of the LUT's lags at that cell."""
    S = CASES[name]["S"]
    l3 = np.asarray(lut).reshape(3, -1).astype(np.int64)
    return [[0, int(l3[0][c]) - S, int(l3[1][c]) - S] for c in mirror_cells(name)[0]]


# Frames whose answer needs the second trip of k_p1k_lean's bound loop (g15x9: rows sorted by
# pair 2's lag slot, row 0 = slots 43..47, row 1 = slots 47..49).  Cell 51's tuple (46, 48, 47) is
# the last of row 0, its pair-2 slot 47 = lo + 4 is read by the second trip only; cell 36's tuple
# (46, 48, 48) shares the other two lags and lies in row 1.  A source s with mic delays (0, 0, 2)
# puts pairs (0,1), (0,2) on slots 46, 48 and pair (1,2) on slot 48; a stronger source u that only
# mics 1 and 2 hear, one sample apart, puts pair (1,2)'s best on slot 47.  The maximum is cell 51
# (M0 + M1 + M2); cell 36 has M0 + M1 + (s's lower peak).  A bound that misses slot 47 ranks row 0
# at noise level, scans row 1 first and prunes row 0 against cell 36's L.
TWO_TRIPS = dict(case="g15x9", cell=51, tuple=(46, 48, 47), decoy=36, decoy_tuple=(46, 48, 48), frames=16, seed=0x2B1D)


def two_trip_frames(spec=TWO_TRIPS, N=1024, std_s=20.0, std_u=30.0, noise_std=3.0):
    """int16 [frames][3][N] (numpy): s on all mics with the tuple's delays, u on mics 1 and 2 only."""
    S = CASES[spec["case"]]["S"]
    l01, l02, l12 = (int(x) - S for x in spec["tuple"])
    assert (l01, l02, l12 + 1) == tuple(int(x) - S for x in spec["decoy_tuple"]) and l02 - l01 == l12 + 1
    rng = np.random.default_rng(spec["seed"])
    B, pad = spec["frames"], S + 1
    s = rng.standard_normal((B, N + 2 * pad)) * std_s
    u = rng.standard_normal((B, N + 2 * pad)) * std_u
    n = np.arange(N) + pad
    x = rng.standard_normal((B, 3, N)) * noise_std + 128.0
    for m, d in enumerate((0, l01, l02)):
        x[:, m] += s[:, n - d]
    for m, d in ((1, 0), (2, l12)):
        x[:, m] += u[:, n - d]
    return np.clip(np.rint(x), 0, 255).astype(np.int16)


def stream_capture(spec, lut, **burst):
    """uint8 [6][hop * hops][3] capture of a streaming spec on the case's LUT."""
    return synth.adc_stream(6, spec["hop"] * spec["hops"], 3, lut, CASES[spec["case"]]["S"], spec["seed"],
                            **burst).numpy()


def p1k_fits(U):
    """tdoa_phat1024_fits restated for a 3 x 1024 context with a prune section: k_p1k_lean's image is
    P1K_IMG_FIXED + 4 * Upad bytes, P1K_IMG_FIXED = 32 * 32 * 8 + 16 * 32 * 8 + 128 * 4 + 512 * 8 = 16896
    and Upad = U rounded up to 512 tuples.  It must load as 4 units of 16 B per thread of 8 waves
    (<= 32768) and, beside the 8 waves' tiles of 2 * 8448 B each and 64 B of progress words, fit the
    CU's 160 KiB of LDS: 135168 + 16896 + 4 * Upad + 64 <= 163840, so Upad <= 2560: at most 40 rows
    of 64 tuples.  (The second rule binds; the first alone would admit 56 rows.)"""
    img = 16896 + 4 * (-(-U // 512) * 512)
    return img <= 4 * 8 * 64 * 16 and 8 * 2 * 8448 + img + 64 <= 160 * 1024


def geometry(name_or_kw):
    """(half_w, half_h, grid_scale, height_offset, speed_of_sound, sample_rate_hz) of a case or of Localizer kwargs."""
    kw = CASES[name_or_kw]["kw"] if isinstance(name_or_kw, str) else name_or_kw
    return (kw.get("grid_half_w", 50), kw.get("grid_half_h", 50), kw.get("grid_scale", 24.0),
            kw.get("height_offset", 1.2), kw.get("speed_of_sound", 343.0), kw.get("sample_rate_hz", 50000))


def config_overrides(name):
    """The case as a config of tools/tables_dump (tests/test_tables_cpu.py write_config): engine GCC_PHAT."""
    return dict(CASES[name]["kw"], engine=1)


def closed_form_xy(cell, half_w, half_h, scale):
    """((cx - half_w) / scale, (half_h - cy) / scale) with W = 2 half_w + 1, in float32 as on the device."""
    cell = np.asarray(cell).astype(np.int64)
    W = 2 * half_w + 1
    return np.stack([(cell % W - half_w).astype(np.float32) / np.float32(scale),
                     (half_h - cell // W).astype(np.float32) / np.float32(scale)], -1)
