// tdoa_tables.h -- everything a context computes before it touches the GPU
// (tdoa_tables.cpp).  Host only: no HIP header, so the builder also compiles
// with a plain host compiler and runs on a machine without a GPU
// (tools/tables_dump.cpp, tests/test_tables_cpu.py).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/tdoa.h"
#include "tdoa_shared.h"

struct tdoa_tables {
    tdoa_config cfg;  // as given, its pointers cleared and max_shift resolved
    int M, N, P, K, S, G, W, H, U, TW;
    std::vector<float> mic;           // [M][2]
    std::vector<int32_t> win;         // [N] Q15
    std::vector<float> prior;         // [K]
    std::vector<uint8_t> lut;         // [P][G]
    std::vector<uint32_t> tuples;     // [U][TW] distinct lag tuples, first-cell order
    std::vector<int32_t> tuple_cell;  // [U]
    // GCC_PHAT twiddles (re, im): [N] e^{-2 pi i k/N} at 0, [N + 1]
    // e^{-2 pi i k/2N} at tw2_at, the long-frame kernels' [3][16][16] at r16_at
    std::vector<float> tw;
    size_t tw2_at, r16_at;  // in floats
    // k_grid_bb's table image, 16-B padded sections at these byte offsets
    enum { BB_TILE, BB_RNG, BB_TUPLES, BB_UIDX, BB_Q, BB_SECTIONS };
    std::vector<uint8_t> bb_img;
    size_t bb_at[BB_SECTIONS];
    int bb_NT = 0;
    int bb_wide = 0;  // a range wider than the queries encode: no k_grid_bb
    // compact weighted-score layout (kp.wc_lo / wc_w / wc_off / wc_CK / wc_nch)
    bool wc_ok = false;
    std::vector<uint32_t> wc_chunks;
#if TDOA_AB
    // the fused k_frame16 grid's tables (A/B library only): kp.fg_q [NT][32],
    // then kp.fg_tup [U][32] at fg_tup_at
    bool fg_ok = false;
    std::vector<uint16_t> fg;
    size_t fg_tup_at = 0;  // in bytes
#endif
    // every field of the kernel parameters that is no device pointer; the
    // pointers are null until the context has uploaded what they point to
    tdoa_kparams kp;
};

// Validate cfg and fill *t.  TDOA_OK, or the TDOA_ERR_* code with the message
// left for tdoa_last_error.
int tdoa_build_tables(const tdoa_config *cfg, tdoa_tables *t);

// The pruned grid scan of k_p1k_lean (tdoa_phat1024.hip, three pairs, one
// tuple word per tuple): the distinct tuples sorted by the lag slot of one
// pair -- ties in first-cell order -- and cut into rows of 64, as 32-bit words:
//   [0] rows  [1] the sort pair  [2] the widest row's span in lags  [3] tuple 0's first cell
//   [4 .. 68)       per row lo | hi << 8: the sort pair's lag slots its tuples use
//   [68 .. + 64 rows) the tuples as LDS byte offsets (slot << 3 in bits 0-9, 10-19, 20-29)
//   [.. + 64 rows)    their first cells
// The last row is padded with the tuple (127, 127, 127), cell INT_MAX.  Empty
// when the tuples make more than 64 rows.
#define TDOA_P1K_PRUNE_HDR 4
void tdoa_p1k_prune_section(int U, const uint32_t *tuples, const int32_t *tuple_cell, std::vector<uint32_t> &sec);
