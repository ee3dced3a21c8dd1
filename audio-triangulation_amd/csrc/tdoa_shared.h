// tdoa_shared.h -- what the host-only table builder (tdoa_tables.cpp) and the
// HIP translation units both see: the tiling constants, the kernel parameter
// block and the error store.  No HIP header: a plain host compiler reads it.
#pragma once

#include <stddef.h>
#include <stdint.h>

#define TDOA_MAX_PAIRS 28  // 8 mics
#define TDOA_MAX_MICS_K 8
#define TDOA_LS_ITERS 10   // least-squares refinement steps (tdoa_ls.hip)

// Lag tiling of the DIRECT kernel: each work item owns TDOA_LT consecutive
// lags (an even start lag, so even lags read word-aligned sample pairs and odd
// lags read the one-sample-shifted pairs) over a TDOA_SEGW-word (2*SEGW
// sample) segment of the frame.  SEGW <= 128 keeps every int32 partial of the
// hi/lo byte-split products exact (256 * 32768 * 255 < 2^31).
#define TDOA_LT 16
#define TDOA_LT2 (TDOA_LT / 2)
#define TDOA_SEGW 64

// GCC_PHAT spectrum scratch of the two-pass shapes and of a band-limited
// context: a fixed chunk of frames' spectra that stays in L2 / MALL between passes
#define TDOA_SPEC_BYTES ((size_t)128 << 20)

struct tdoa_kparams {
    // shape
    int32_t M, N, log2N, P, K, S;  // S = max_shift, K = 2S+1
    int32_t G, U;                  // grid cells, unique lag tuples
    int32_t grid_W, half_w, half_h;
    float grid_scale;
    // DIRECT tiling
    int32_t sbase;   // first (even) lag of tile 0
    int32_t T;       // lag tiles per pair
    int32_t NSEG;    // segments per frame row (N/2 / SEGW)
    int32_t PADW;    // zero words left/right of every staged row
    int32_t RS;      // staged row stride in words = N/2 + 2*PADW
    int32_t F;       // frames per workgroup
    int32_t TW;      // tuple words per lag tuple = ceil(P/4)
    int32_t xc3;     // k_direct_mfma, three mics: a workgroup's xcorr units are (frame, first mic), the
                     // partners' lag columns side by side in one MFMA tile (0: one unit per pair)
    uint8_t pair_i[TDOA_MAX_PAIRS];
    uint8_t pair_j[TDOA_MAX_PAIRS];
    // device tables
    const int16_t *window;     // [N] Q15
    const float *prior;        // [K] scale by |s - best|
    const uint32_t *tuples;    // [U][TW] packed lag indices (byte p = pair p)
    const int32_t *tuple_cell; // [U] first row-major cell of each tuple
    const float *tw;           // GCC_PHAT: e^{-2 pi i k/N}, k < N   (re, im)
    const float *tw2;          // GCC_PHAT: e^{-2 pi i k/2N}, k <= N (re, im)
    const float *r16_tw;       // GCC_PHAT long frames: [3][16][16] W_N^{(N/256) r k}, W_N^{r l}, W_N^{16 r h}
    const uint8_t *lut;        // [P][G] lag index per cell (heat map)
    const void *p1k_img;       // config-2 GCC-PHAT kernel: its LDS table image (16-B units)
    int32_t p1k_img_bytes;
    const void *w64_img;       // ... and of its one-frame-per-wave form (k_p1k_w64)
    int32_t w64_img_bytes;
    // exact branch-and-bound grid (k_grid_bb): the distinct tuples regrouped
    // by the 8 x 8-cell tile of their first cell (<= 64 tuples per entry);
    // per entry and pair the lag range [lo, hi] of its tuples
    int32_t bb_NT;             // tile entries (0: no table, k_grid only)
    const int32_t *bb_tile;    // [NT][2] first tuple (regrouped order), count
    const uint16_t *bb_rng;    // [NT][P] lo | hi << 8
    const uint32_t *bb_tuples; // [U][TW] regrouped tuples
    const int32_t *bb_uidx;    // [U] their index in first-cell order
    const uint16_t *bb_q;      // [NT][P] the ranges as sparse-table queries (bb_query)
    int32_t bb_wide;           // some range is wider than a query encodes (k_grid instead)
    // compact weighted-score scratch (k_frame16 -> k_grid_bb): per frame only
    // the lags some grid tuple uses, pair p's lags [wc_lo, wc_lo + wc_w) at
    // wc_off[p] (a multiple of 4 floats), wc_CK floats per frame; k_grid_bb
    // expands it in LDS by 16-B chunks: wc_chunks[c] = LDS element of the
    // chunk's first lag (p * K + lag) | valid floats << 16
    int32_t wc_CK, wc_nch;
    uint16_t wc_off[TDOA_MAX_PAIRS];
    uint8_t wc_lo[TDOA_MAX_PAIRS], wc_w[TDOA_MAX_PAIRS];
    const uint32_t *wc_chunks;
    // the grid solve fused into k_frame16 (tdoa_phat_r16.hip, "FG"): every
    // (entry, pair) range of the k_grid_bb tables as a query into sparse-table
    // levels of the compact layout above: e | lv << 11 | d << 13 with e =
    // wc_off[p] + lo - wc_lo[p] the first window's element of level lv
    // (2^lv <= n = hi - lo + 1 < 2^(lv+1); level 0 = the scores) and d = n - 2^lv
    // the second window's distance; rows of 32 (P <= 28 used)
    const uint16_t *fg_q;      // [bb_NT][32]
    const uint16_t *fg_tup;    // [U][32] the regrouped tuples as compact element indices (wc_off + lag - wc_lo)
    int32_t fg_ok;             // the tables exist (n <= 15, wc_CK <= 2048, bb_NT <= 256, P <= 32)
    // DIRECT on the streaming batch read straight from the capture ring (the
    // triggers list the firing streams and copy nothing): frame f
    // of the batch is stream frame_ids[f]'s samples from ring index
    // frame_ring_at[f] (absolute sample frame_end[f] - N; earlier than the
    // stream's first sample reads as 0); frame_ring null: frame f is frames[f]
    const int32_t *frame_ids;
    const uint8_t *frame_ring;     // [S][ring_len][M] 8-bit ADC bytes, round-robin
    int64_t ring_len;
    const int64_t *frame_end;      // [B] samples consumed at the trigger
    const int64_t *frame_ring_at;  // [B] ring index of the frame's first sample
    // reserved, always 0 (once the flag of a compact 8-bit frame batch): the
    // four bytes stay so that no other field moves
    int32_t reserved0;
    // sample format of a GCC_PHAT batch (tdoa_set_sample_format): 0 the 8-bit
    // ADC front end, 1 full-range int16 (TDOA_SAMPLES_PCM16).  It picks the
    // launch's kernels on the host; no kernel reads it.  It fills the four
    // bytes between reserved0 and mic_xy, so no other field moves and every
    // kernel's argument offsets stay as they were
    int32_t pcm16;
    // least-squares refinement (tdoa_ls.hip)
    const float *mic_xy;       // [M][2] metres
    float fs, c, height;
    // band-limited GCC-PHAT (tdoa_set_bin_weights): R_ij[k] *= bin_w[k], k = 0..N
    // bins of the 2N-point spectrum; null: no weighting, the shape's own route.
    // bin_lo / bin_hi: the first / last bin with a non-zero weight
    const float *bin_w;        // [N + 1]
    int32_t bin_lo, bin_hi;
};
// passed to every kernel by value: host and device must agree on it
static_assert(sizeof(tdoa_kparams) == 520, "tdoa_kparams layout (x86-64 host, gfx950 device)");

// The thread's last error (tdoa_last_error): store the message, return the
// code.  Defined in tdoa_tables.cpp, the one TU every build of the library and
// every host-only tool links.
int tdoa_set_error(int code, const char *msg);
#if defined(__GNUC__)
__attribute__((format(printf, 2, 3)))
#endif
int tdoa_fail(int code, const char *fmt, ...);
