// tdoa_phat1024.hip -- GCC-PHAT metric kernel for BASELINE config 2
// (3 mics x 1024-sample frames, L = 2048), see DESIGN.md "k_phat1024".
//
// One frame per 32-lane half-wave (two frames per wave); the three mics of the
// frame run in the same lanes, so no spectrum ever crosses a wave and the
// kernel has no workgroup barrier after the table staging.  A frame is one FFT
// stream through the half-wave's own transpose tile; two waves per SIMD hide
// each other's LDS round trips (k_p1k_lean<NW> below: NW waves per workgroup).
//
// Per mic m (rolling_buffer.c:64-66, buffer.c:13-16, buffer.c:4-11 front end):
//   z[n] = x[2n] + i x[2n+1]  (n < 512; the upper half is the zero padding)
//   Z = FFT_1024(z) as 32 x 32: DFT-32 over n1 in registers (lane = residue
//       column n2 = res(lane)), twiddle W_1024^{n2 k1}, transpose through a
//       private padded LDS tile (row stride 264 B, residues 16 and 24 in
//       swapped slots: b64 writes and reads bank-conflict free), DFT-32 over n2.
//       Lane l then holds Z[res + 32 k2], k2 = 0..31.
//   Real-FFT split X[b] (b <-> N - b): lanes l, l^1 hold the partner residues
//       res, 32 - res; they swap their upper 16 registers by DPP so that the
//       partner of register k is register 31 - k in the same lane (lane 0 --
//       residue 0, self-paired with two fixed points 0 and 512 -- rotates its
//       upper half instead and keeps bin 512 in a 33rd register; lane 1 --
//       residue 16, self-paired -- keeps its registers).
//   PHAT factored per mic: U_m = X_m / sqrt(|X_m|^2 + e) (c_unit), so
//       R_ij = conj(U_i) U_j is the unit cross-spectrum: the definition of
//       include/tdoa.h and the oracle (an all-zero bin gives 0).
// Per pair (0,1), (0,2), (1,2) (sample_compute.h:120-122 order):
//   Y[b] = (R[b] + R*[N-b]) + i (R[b] - R*[N-b]) W_2048^{-b}   (in-lane pairs)
//   swap back to residue columns, y = IFFT_1024(Y) pruned to the outputs
//   n = n1 (+992) that hold lags -S..S, argmax + lag prior (correlations.c:20-33
//   semantics on float scores), gate (sample_compute.h:124-134).
// Per wave: the grid solve of vga_heatmap.h:99-108 for its two frames at once
// (lanes split the distinct lag tuples, one b64 gather per pair reads the two
// frames' weighted scores from an [p][k] float2 table in the wave's tiles).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <type_traits>
#include <vector>

#include "tdoa_cplx.h"
#include "tdoa_internal.h"
#include "tdoa_tables.h"  // the pruned scan's row table (tdoa_p1k_prune_section)

// TDOA_AB=1: the A/B build (tdoa/libtdoa_ab.so) holds both workgroup shapes of
// k_p1k_lean; the product holds the one it launches
#ifndef TDOA_AB
#define TDOA_AB 0
#endif

namespace {

constexpr int P1K_ROW = 264;              // tile row stride, bytes (32 complex + 8 B pad)
constexpr int P1K_TILE = 32 * P1K_ROW;    // 8448 B: one transpose of one half-wave
constexpr int P1K_KPAD = 128;             // lag slots per pair in the grid score table
constexpr int P1K_WAVE_LDS = 2 * P1K_TILE;  // a wave's two transpose tiles (one per half-wave)
[[maybe_unused]] constexpr int P1K_GB = 8;               // grid tuples per lane per batch
// Table image: twm [32][32] f2 | tw2 [16][32] f2 | prior [128] | win [512] f2 | tuples.
// The first P1K_IMG_LDS4 bytes are all that the 4-wave workgroup keeps in LDS.
constexpr int P1K_IMG_LDS4 = 32 * 32 * 8 + 16 * 32 * 8 + 128 * 4;
constexpr int P1K_IMG_FIXED = P1K_IMG_LDS4 + 512 * 8;
// tuple words of the exhaustive scan: U padded to whole double steps of 256.
// With P1K_GRID_PRUNE the pruned scan's row table follows them in the image
// (global memory only: no workgroup stages it)
__host__ __device__ constexpr int p1k_upad(int U) { return (U + P1K_GB * 64 - 1) / (P1K_GB * 64) * (P1K_GB * 64); }

// Tile row / column and table column of residue (or DFT index) x: 16 and 24
// swap places, so the residues of every 16-lane group of a half-wave --
// {0, 16, 1, 31, .., 7, 25} and {8, 24, 9, 23, .., 15, 17} -- fall on distinct
// 8-B bank slots mod 16: the transposes' ds_write_b64 / ds_read2_b64 and the
// table reads (bank = dword mod 32) are conflict-free (plain order: 2-way).
__host__ __device__ constexpr int slot(int x) { return x == 16 ? 24 : (x == 24 ? 16 : x); }

// residue column held by lane l of a half-wave: lanes (2j, 2j+1) hold the
// partner residues (j, 32 - j); lanes 0, 1 the self-paired residues 0, 16
__device__ __forceinline__ int lane_res(int l)
{
    return l < 2 ? l * 16 : ((l & 1) ? 32 - (l >> 1) : (l >> 1));
}

__device__ __forceinline__ float dpp_xor1(float v)
{
    return __builtin_bit_cast(
        float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, false));
}
__device__ __forceinline__ f2 dpp_xor1(f2 v) { return f2{dpp_xor1(v.x), dpp_xor1(v.y)}; }
typedef short v2s_t __attribute__((ext_vector_type(2)));

// Partner swap of the upper 16 bins (registers 16..31), exec-masked instead of
// two selects per dword: lanes other than 0, 1 (of each half-wave) take their
// DPP partner's register in place (one instruction per dword); lane 0 then
// shifts its own upper half by one register (FWD: V[j] <- V[j+1], V[31] <- V[0];
// !FWD: V[j] <- V[j-1], V[16] <- E) in 64-bit moves; lane 1 keeps its registers.
// Wait states inside the strings: 2 before a DPP reads a VGPR a VALU wrote
// (s_nop 1; the compiler pads only its own boundary), and a conservative
// s_nop 4 after each EXEC write ahead of a DPP / VALU.
#define P1K_X(i) "%" #i
#define P1K_DPP(i) "v_mov_b32_dpp " P1K_X(i) ", " P1K_X(i) " quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
#define P1K_MOV(d, s) "v_mov_b64 " P1K_X(d) ", " P1K_X(s) "\n\t"
template <bool FWD, int NV>
__device__ __forceinline__ void swap_upper_exec(f2 (&V)[NV], f2 E)
{
    float x[32];
#pragma unroll
    for (int j = 0; j < 16; j++) {
        x[2 * j] = V[16 + j].x;
        x[2 * j + 1] = V[16 + j].y;
    }
    uint64_t sv;
    asm volatile("s_mov_b64 %[sv], exec\n\t"
                 "s_and_b64 exec, exec, %[m1]\n\t"
                 "s_nop 4\n\t" P1K_DPP(0) P1K_DPP(1) P1K_DPP(2) P1K_DPP(3) P1K_DPP(4) P1K_DPP(5)
                     P1K_DPP(6) P1K_DPP(7) P1K_DPP(8) P1K_DPP(9) P1K_DPP(10) P1K_DPP(11) P1K_DPP(12)
                         P1K_DPP(13) P1K_DPP(14) P1K_DPP(15) P1K_DPP(16) P1K_DPP(17) P1K_DPP(18)
                             P1K_DPP(19) P1K_DPP(20) P1K_DPP(21) P1K_DPP(22) P1K_DPP(23) P1K_DPP(24)
                                 P1K_DPP(25) P1K_DPP(26) P1K_DPP(27) P1K_DPP(28) P1K_DPP(29)
                                     P1K_DPP(30) P1K_DPP(31) "s_mov_b64 exec, %[sv]\n\t"
                 "s_nop 4"
                 : "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3]), "+v"(x[4]), "+v"(x[5]),
                   "+v"(x[6]), "+v"(x[7]), "+v"(x[8]), "+v"(x[9]), "+v"(x[10]), "+v"(x[11]),
                   "+v"(x[12]), "+v"(x[13]), "+v"(x[14]), "+v"(x[15]), "+v"(x[16]), "+v"(x[17]),
                   "+v"(x[18]), "+v"(x[19]), "+v"(x[20]), "+v"(x[21]), "+v"(x[22]), "+v"(x[23]),
                   "+v"(x[24]), "+v"(x[25]), "+v"(x[26]), "+v"(x[27]), "+v"(x[28]), "+v"(x[29]),
                   "+v"(x[30]), "+v"(x[31]), [sv] "=&s"(sv)
                 : [m1] "s"(0xFFFFFFFCFFFFFFFCull));
    f2 y[16];
#pragma unroll
    for (int j = 0; j < 16; j++)
        y[j] = f2{x[2 * j], x[2 * j + 1]};
    const f2 e = FWD ? V[0] : E;
#define P1K_ROT_ASM(ROT)                                                                            \
    asm volatile("s_mov_b64 %[sv], exec\n\t"                                                        \
                 "s_and_b64 exec, exec, %[m2]\n\t"                                                  \
                 "s_nop 4\n\t" ROT "s_mov_b64 exec, %[sv]\n\t"                                     \
                 "s_nop 4"                                                                           \
                 : "+v"(y[0]), "+v"(y[1]), "+v"(y[2]), "+v"(y[3]), "+v"(y[4]), "+v"(y[5]),           \
                   "+v"(y[6]), "+v"(y[7]), "+v"(y[8]), "+v"(y[9]), "+v"(y[10]), "+v"(y[11]),         \
                   "+v"(y[12]), "+v"(y[13]), "+v"(y[14]), "+v"(y[15]), [sv] "=&s"(sv)                \
                 : [m2] "s"(0x0000000100000001ull), [e] "v"(e))
    if constexpr (FWD)
        P1K_ROT_ASM(P1K_MOV(0, 1) P1K_MOV(1, 2) P1K_MOV(2, 3) P1K_MOV(3, 4) P1K_MOV(4, 5) P1K_MOV(5, 6)
                        P1K_MOV(6, 7) P1K_MOV(7, 8) P1K_MOV(8, 9) P1K_MOV(9, 10) P1K_MOV(10, 11)
                            P1K_MOV(11, 12) P1K_MOV(12, 13) P1K_MOV(13, 14) P1K_MOV(14, 15)
                                "v_mov_b64 %15, %[e]\n\t");
    else
        P1K_ROT_ASM(P1K_MOV(15, 14) P1K_MOV(14, 13) P1K_MOV(13, 12) P1K_MOV(12, 11) P1K_MOV(11, 10)
                        P1K_MOV(10, 9) P1K_MOV(9, 8) P1K_MOV(8, 7) P1K_MOV(7, 6) P1K_MOV(6, 5)
                            P1K_MOV(5, 4) P1K_MOV(4, 3) P1K_MOV(3, 2) P1K_MOV(2, 1) P1K_MOV(1, 0)
                                "v_mov_b64 %0, %[e]\n\t");
#undef P1K_ROT_ASM
#pragma unroll
    for (int j = 0; j < 16; j++)
        V[16 + j] = y[j];
}

// sum over the 32 lanes of each half-wave, VALU only (no LDS queue): row
// all-reduce by DPP, row_bcast:15 into rows 1 and 3, then lanes 31 / 63
__device__ __forceinline__ int hsum32(int s, int hw)
{
    s += __builtin_amdgcn_mov_dpp(s, 0xB1, 0xF, 0xF, false);   // xor 1
    s += __builtin_amdgcn_mov_dpp(s, 0x4E, 0xF, 0xF, false);   // xor 2
    s += __builtin_amdgcn_mov_dpp(s, 0x141, 0xF, 0xF, false);  // half-row mirror
    s += __builtin_amdgcn_mov_dpp(s, 0x140, 0xF, 0xF, false);  // row mirror
    s += __builtin_amdgcn_update_dpp(0, s, 0x142, 0xA, 0xF, false);  // row_bcast:15
    const int s0 = __builtin_amdgcn_readlane(s, 31), s1 = __builtin_amdgcn_readlane(s, 63);
    return hw ? s1 : s0;
}

// LDS reads: volatile ds_read_b64 unless P1K_VLDS=0 (the backend otherwise
// merges neighbours into ds_read2_b64, twice the LDS cycles of two b64 reads)
#ifndef P1K_VLDS
#define P1K_VLDS 1
#endif
__device__ __forceinline__ f2 lds_f2(const char *base, int off)
{
#if P1K_VLDS
    return lds_rd(reinterpret_cast<const f2 *>(base + off));
#else
    return *reinterpret_cast<const f2 *>(base + off);
#endif
}
// the grid over tuples grouped by their first two lags (see the grid solve;
// A/B variant, not the default: 25 % fewer LDS instructions per wave, but the
// phase is latency-bound and the group's cell resolution adds ~1.9 k cycles,
// 31.0 vs 30.4 us per 4096 frames -- DESIGN.md "Measured negative results")
#ifndef P1K_GROUPS
#define P1K_GROUPS 0
#endif
// the winner's first cell from LDS (tuple words carry it; see the grid end).
// A/B variant, not the default: neutral (30.3 vs 30.35 us per 4096 frames) once
// the lag / gate stores moved behind the grid, and it needs every 32-tuple row
// to span < 2048 cells
#ifndef P1K_CELL_LDS
#define P1K_CELL_LDS 0
#endif
// the SIMD issue balance (s_setprio by phase progress; see the kernel).
// Without it (P1K_BALANCE=0): 31.8 vs 29.1 us per 4096 frames
#ifndef P1K_BALANCE
#define P1K_BALANCE 1
#endif
// mic 2's words requested inside mic 1's forward (as mic 1's inside mic 0's).
// A/B variant, not the default: 29.9 vs 29.1 us (the column pass of pair
// (0,1) then runs with 16 more live registers)
#ifndef P1K_W2_EARLY
#define P1K_W2_EARLY 0
#endif
// the frame's lag / gate stores after the grid (see store_frame)
#ifndef P1K_LATE_STORES
#define P1K_LATE_STORES 1
#endif
// The 4-wave workgroup's knobs (k_p1k_lean<4>; A/B variants, DESIGN.md has the figures):
// P1K_WG4_PRIO=1: s_setprio 3 in the latency-bound phases (staging, grid), 0 in
//   the transforms, instead of the default priority throughout
#ifndef P1K_WG4_PRIO
#define P1K_WG4_PRIO 0
#endif
// P1K_WG4_WQ_LATE=1: mic 2's window taps requested after pair (0,1)'s maximum
//   instead of with the row's words (16 fewer live registers across it)
#ifndef P1K_WG4_WQ_LATE
#define P1K_WG4_WQ_LATE 0
#endif
// P1K_WG4_TUPS_ALL=1: every tuple word of the lane requested at the grid's
//   start (the scan unrolled over at most 14 steps) instead of two steps ahead
#ifndef P1K_WG4_TUPS_ALL
#define P1K_WG4_TUPS_ALL 0
#endif
// P1K_GRID_PRUNE=1: the 4-wave workgroup scans only the rows of 64 tuples whose
// exact upper bound is not below the best L found so far (see the grid solve;
// the table image carries the rows after the tuple words).  0: the exhaustive
// scan of every tuple, as the 8-wave workgroup's always is; same outputs.
// Not with the scan variants that lay the image's tail out differently
#ifndef P1K_GRID_PRUNE
#define P1K_GRID_PRUNE 1
#endif
#if P1K_GROUPS || P1K_CELL_LDS
#undef P1K_GRID_PRUNE
#define P1K_GRID_PRUNE 0
#endif
// the image's bytes up to the pruned scan's row table: what the 8-wave
// workgroup keeps in LDS
__host__ __device__ inline int p1k_img_lds8(const tdoa_kparams &kp)
{
    return P1K_GRID_PRUNE ? P1K_IMG_FIXED + 4 * p1k_upad(kp.U) : kp.p1k_img_bytes;
}
// plain LDS read (the grid's gathers: data-dependent addresses, never merged,
// and free to be scheduled around the other reads of the software pipeline)
__device__ __forceinline__ f2 lds_f2_plain(const char *base, int off)
{
    return *reinterpret_cast<const f2 *>(base + off);
}
// LDS read at a 32-bit LDS byte address
__device__ __forceinline__ f2 lds_at(uint32_t addr)
{
    return *(const __attribute__((address_space(3))) f2 *)(uintptr_t)addr;
}
__device__ __forceinline__ void sts_f2(char *base, int off, f2 v)
{
    *reinterpret_cast<f2 *>(base + off) = v;
}

// an empty asm that needs the value: it must be computed here (keeps IR
// passes from sinking a finished partial sum past later phases)
__device__ __forceinline__ void pin(f2 &x) { asm volatile("" : "+v"(x)); }


struct Lane {
    int hw;           // half-wave of the wave
    int lane;         // 0..31 within the half-wave
    int res;          // residue column
    int cs;           // its tile / table slot, slot(res)
    bool is0, is1;    // the self-paired lanes
    char *tileA;      // this half-wave's transpose tile
    const char *twm;  // [k][r] W_1024^{r k}
    const char *tw2;  // [k][r] W_2048^{r + 32 k}, k < 16
    const char *win;  // [w] (W[2w], W[2w+1]) / 128
};

// How far ahead of their use the transforms request table and tile values from
// LDS, per call site: the kernel's register peak (pair (0,1), and mic 2 + cross:
// two unit spectra and a working column live) keeps the lean forms, the four
// other transforms (mic 0, mic 1, pairs (0,2) and (1,2): "roomy", 100+ free
// registers) may take the deep ones.  Loads and waits only: no floating-point
// operation, operand or association differs between the forms, so neither does
// any output byte (tests/test_gpu_p1k_parent_bytes.py).  A/B variants; the
// defaults are the forms that won on their own (DESIGN.md "k_p1k_lean" and
// "Measured negative results (LDS read depths)", profiles/c2_lds_inflight_ab.txt;
// us per 4096 frames on two step streams against 25.13 with every knob off).
// P1K_TWM_ROOMY / P1K_TWM_TIGHT: fft_col_lds's W_1024 twiddles.
//   8: groups of 8 after the DFT-32, each read next to its multiplies;
//   4: groups of 4 in two register sets, group g + 1 requested ahead of group
//      g's multiplies (the registers of 8);
//  32: all of them requested ahead of the DFT-32 (62 more live registers).
// Neither moved the step time: ROOMY=32 25.15, TIGHT=4 25.15
#ifndef P1K_TWM_ROOMY
#define P1K_TWM_ROOMY 8
#endif
#ifndef P1K_TWM_TIGHT
#define P1K_TWM_TIGHT 8
#endif
// P1K_TW2_ROOMY / P1K_TW2_TIGHT: the W_2048 twiddles of a split or pre-twiddle.
//   1: requested one bin pair ahead in the source (P1K_TWPF) -- the scheduler
//      sinks each read to the end of that pair's arithmetic, a few
//      instructions ahead of its use;
//   2: the same, the read held ahead of that pair's arithmetic (the pair's
//      first operand passes through an empty volatile asm behind the read),
//      so the wait ahead of a pair leaves the next pair's read in flight
//      (same registers);
//  16: (roomy only) all requested at once -- a split's with its row reads, a
//      pre-twiddle's ahead of its first pair (32 more live registers).
// ROOMY=16: 24.67, every round a win; ROOMY=2 (with TIGHT=2) 24.89; TIGHT=2 alone 25.02
#ifndef P1K_TW2_ROOMY
#define P1K_TW2_ROOMY 16
#endif
#ifndef P1K_TW2_TIGHT
#define P1K_TW2_TIGHT 1
#endif
// P1K_PRIOR_AHEAD=1: finish_pair requests its four lag-prior values at once,
//   unconditionally (a clamped index), instead of one round trip each inside
//   the candidates' exec-masked branches (24.74 against 25.13)
#ifndef P1K_PRIOR_AHEAD
#define P1K_PRIOR_AHEAD 1
#endif
// P1K_ROW_ROOMY: lean_row_inv's tile row.  16: two groups of 16 values; 32:
//   the whole row requested at once, summed in the same two groups
//   (24.97: inside the runs' spread of 0.30)
#ifndef P1K_ROW_ROOMY
#define P1K_ROW_ROOMY 16
#endif
// k_p1k_pcm16 (at 256 registers in the lean forms) may take smaller depths
#ifndef P1K_TWM_ROOMY_PCM16
#define P1K_TWM_ROOMY_PCM16 P1K_TWM_ROOMY
#endif
#ifndef P1K_TWM_TIGHT_PCM16
#define P1K_TWM_TIGHT_PCM16 P1K_TWM_TIGHT
#endif
#ifndef P1K_TW2_ROOMY_PCM16
#define P1K_TW2_ROOMY_PCM16 P1K_TW2_ROOMY
#endif
#ifndef P1K_TW2_TIGHT_PCM16
#define P1K_TW2_TIGHT_PCM16 P1K_TW2_TIGHT
#endif
#ifndef P1K_ROW_ROOMY_PCM16
#define P1K_ROW_ROOMY_PCM16 P1K_ROW_ROOMY
#endif

// first half of a 32 x 32 FFT_1024 on a residue column: DFT-32 in registers,
// twiddle W_1024^{-+res k}, column write into the tile
// ... with the twiddles read from LDS ahead of their writes, DEPTH at a time
// (P1K_TWM_*; 8 is the register-lean form for two waves per SIMD)
template <bool INV, bool HALF_ZERO, int DEPTH>
__device__ __forceinline__ void fft_col_lds(const Lane &L, f2 (&v)[32], char *tile)
{
    static_assert(DEPTH == 4 || DEPTH == 8 || DEPTH == 32, "fft_col_lds: twiddles 4, 8 or 32 ahead");
    auto put = [&](int wo, int k, f2 w) {
        f2 x = v[k];
        if (k)
            x = INV ? c_mulconj(x, w) : c_mul(x, w);
        sts_f2(tile, wo + P1K_ROW * slot(k), x);
    };
    if constexpr (DEPTH == 32) {
        // the table depends on the lane alone: requested here, its round trip
        // passes under the DFT-32 (k = 0 is W = 1: not read)
        const int wo = 8 * L.cs;
        f2 tw[32];
#pragma unroll
        for (int k = 1; k < 32; k++)
            tw[k] = lds_f2(L.twm, wo + 256 * k);
        __builtin_amdgcn_sched_barrier(0);  // (the scheduler would sink the reads to their uses)
        fft32d<INV, HALF_ZERO>(v);
        wave_lds_sync();  // after the previous pass's row reads of this tile
#pragma unroll
        for (int k = 0; k < 32; k++)
            put(wo, k, tw[k]);
    } else if constexpr (DEPTH == 4) {
        fft32d<INV, HALF_ZERO>(v);
        wave_lds_sync();  // after the previous pass's row reads of this tile
        const int wo = 8 * L.cs;
        f2 tw[2][4];
#pragma unroll
        for (int i = 0; i < 4; i++)
            tw[0][i] = lds_f2(L.twm, wo + 256 * i);
#pragma unroll
        for (int g = 0; g < 8; g++) {
            if (g < 7) {
#pragma unroll
                for (int i = 0; i < 4; i++)
                    tw[(g + 1) & 1][i] = lds_f2(L.twm, wo + 256 * (4 * g + 4 + i));
            }
#pragma unroll
            for (int i = 0; i < 4; i++)
                put(wo, 4 * g + i, tw[g & 1][i]);
        }
    } else {
        fft32d<INV, HALF_ZERO>(v);
        wave_lds_sync();  // after the previous pass's row reads of this tile
        const int wo = 8 * L.cs;
#pragma unroll
        for (int k0 = 0; k0 < 32; k0 += 8) {
            f2 tw[8];
#pragma unroll
            for (int i = 0; i < 8; i++)
                tw[i] = lds_f2(L.twm, wo + 256 * (k0 + i));
#pragma unroll
            for (int i = 0; i < 8; i++)
                put(wo, k0 + i, tw[i]);
        }
    }
    wave_lds_sync();  // before the row reads of other lanes' columns
}
struct NoHook {
    __device__ void operator()() const {}
};
// second half: row read (row res) + forward DFT-32 -> V[k2] = Z[res + 32 k2]
// (after_rows: further reads to request behind the row's, ahead of the DFT-32)
template <typename Hook = NoHook>
__device__ __forceinline__ void fft_row_fwd(const Lane &L, const char *tile, f2 (&V)[33], Hook after_rows = Hook())
{
    f2 v[32];
    const int ro = P1K_ROW * L.cs;
#pragma unroll
    for (int n = 0; n < 32; n++)
        v[n] = lds_f2(tile, ro + 8 * slot(n));
    after_rows();
    fft32d<false, false>(v);
#pragma unroll
    for (int k = 0; k < 32; k++)
        V[k] = v[k];
}
}  // namespace

#ifdef TDOA_DIAG
// diagnostic build only: per-wave phase stamps of k_p1k_lean
__device__ unsigned long long g_diag_p1k[1 << 16];
#endif

// ---------------------------------------------------------------------------
// k_p1k_lean: the same per-frame algorithm at TWO waves per SIMD (8 waves per
// workgroup, one workgroup per CU, <= 256 registers per lane).  One frame per
// half-wave and one FFT stream; the register plan keeps at most two unit
// spectra plus one working column live:
//   mic 0 -> U0, mic 1 -> U1, pair (0,1) built straight into the inverse's
//   column (no third spectrum), mic 2 -> V, U0 <- conj(U0) V, U1 <- conj(U1) V,
//   pairs (0,2), (1,2).
// Table values (window, twiddles) are read from LDS next to their use instead
// of as whole per-phase arrays.  The grid solve runs per iteration on the
// wave's two frames (b64 gathers of an [p][k] f2 score table).  The partner
// wave of the SIMD hides the LDS round trips that bound the one-wave kernel.
namespace {

// front end + forward FFT_1024 of one mic row, then the partner swap: V[k],
// V[31 - k] hold Z[b], Z[N - b] (paired layout); V[32] = unit X[512] (lane 0)
// A row's words: the frame words w, and -- where the window is not in LDS
// (WQ, the 4-wave workgroup) -- the window's Q15 tap pairs q from kp.window:
// dword res + 32 t of either array covers samples 2 (res + 32 t), + 1.
// PCM16 (TDOA_SAMPLES_PCM16, include/tdoa.h; the 4-wave workgroup only, whose
// Q15 taps are at hand as integers): the same DC sum, then per sample the
// sign-extended half-word minus off (no wrap, |y| <= 65535), one 24-bit
// integer multiply by the tap (|y W| < 2^31), an arithmetic shift by 15 and a
// convert (|s| <= 65535, exact) -- the units of the 8-bit form's floor(s W / 128).
// TWM: fft_col_lds's depth at this call site; after_rows: fft_row_fwd's hook
template <bool PCM16, int TWM, int NQ, typename Hook = NoHook, typename Hook2 = NoHook>
__device__ __forceinline__ void lean_spectrum(const Lane &L, const uint32_t (&w)[16], const uint32_t (&wq)[NQ],
                                              f2 (&V)[33], float e2, Hook after_front = Hook(),
                                              Hook2 after_rows = Hook2())
{
    constexpr bool WQ = NQ == 16;
    static_assert(!PCM16 || WQ, "the PCM16 front end reads the Q15 taps");
    f2 v[32];
    if constexpr (PCM16) {
        int s = 0;
#pragma unroll
        for (int t = 0; t < 16; t++)
            s = __builtin_amdgcn_sdot2(__builtin_bit_cast(v2s_t, w[t]), v2s_t{1, 1}, s, false);
        s = hsum32(s, L.hw);
        const int off = s >> 10;
#pragma unroll
        for (int t = 0; t < 16; t++) {
            const int x0 = (int)(int16_t)(w[t] & 0xFFFFu) - off, x1 = ((int)w[t] >> 16) - off;
            const uint32_t q = wq[NQ == 16 ? t : 0];
            const int p0 = __mul24(x0, (int)(q & 0xFFFFu)) >> 15, p1 = __mul24(x1, (int)(q >> 16)) >> 15;
            v[t] = f2{(float)p0, (float)p1};
        }
    } else {
        int s = 0;
#pragma unroll
        for (int t = 0; t < 16; t++)
            s = __builtin_amdgcn_sdot2(__builtin_bit_cast(v2s_t, w[t]), v2s_t{1, 1}, s, false);
        s = hsum32(s, L.hw);
        const uint32_t off = (uint32_t)(s >> 10) & 0xFFu;
        const uint32_t off2 = off | (off << 16);
#pragma unroll
        for (int t = 0; t < 16; t++) {
            const uint32_t d = (w[t] | 0x01000100u) - off2;
            f2 wf;
            if constexpr (WQ) {  // the image's (float)W / 128, formed here (exact: W < 2^15)
                const uint32_t q = wq[t];
                wf = f2{(float)(int16_t)(q & 0xFFFFu), (float)(int16_t)(q >> 16)} * f2{1.0f / 128.0f, 1.0f / 128.0f};
            } else
                wf = lds_f2(L.win, 8 * L.cs + 256 * t);
            const float s0 = (float)(int8_t)(d & 0xFFu);
            const float s1 = (float)(int8_t)((d >> 16) & 0xFFu);
            const f2 pr = f2{s0, s1} * wf;  // one packed multiply
            v[t] = f2{floorf(pr.x), floorf(pr.y)};
        }
    }
    after_front();  // the row's words are consumed
    fft_col_lds<false, true, TWM>(L, v, L.tileA);
    // X[512] = conj(Z[512]) is in units of X where every other bin holds 2 X
    // (the split's e, od), so its floor is e2 / 4.  One v_ldexp per row, issued
    // here under the transpose's LDS round trip (volatile: computed once per
    // kernel instead, the value costs a register the kernel does not have and
    // spills; config 2 measured 26.96 us per step here, 27.24 next to its use,
    // 27.01 without it)
    float e2q;
    asm volatile("v_ldexp_f32 %0, %1, -2" : "=v"(e2q) : "s"(e2));
    fft_row_fwd(L, L.tileA, V, after_rows);
    V[32] = c_unit(conjf2(V[16]), e2q);
    swap_upper_exec<true>(V, f2{0.0f, 0.0f});
}

// real-FFT split of the partner pair k + unit normalisation: the unit
// spectrum at bins b and N - b (the W_2048^b twiddle read next to its use)
__device__ __forceinline__ void lean_split_w(f2 A, f2 Bv, f2 wk, float e2, f2 &ub, f2 &un)
{
    const f2 e = c_addconj(A, Bv);
    const f2 od = c_mul(c_subconj(A, Bv), wk);
    ub = c_unit(c_add_mi(e, od), e2);
    un = c_unit(c_conj_add_i(e, od), e2);
}
// the W_2048^b twiddle of pair k (P1K_TWPF: requested one pair ahead of its
// use, so its LDS round trip overlaps the previous pair's arithmetic; read
// next to its use, each was a round trip of its own -- the inline-asm packed
// operations keep the backend from hoisting it)
#ifndef P1K_TWPF
#define P1K_TWPF 5  // bit 0: lean_forward, 1: lean_forward_cross, 2: lean_pretwiddle
#endif
__device__ __forceinline__ f2 lean_tw2(const Lane &L, int k) { return lds_f2(L.tw2, 8 * L.cs + 256 * k); }
// ... the next pair's, requested here and (TW2 = 2) kept here: `first`, an
// operand of everything the current pair computes, is pinned behind the read
// (volatile accesses and volatile asm keep their order; the packed operations
// are plain asm, which the instruction selection otherwise places ahead of it)
template <int TW2>
__device__ __forceinline__ f2 lean_tw2_next(const Lane &L, int k, f2 &first)
{
    const f2 w = lean_tw2(L, k);
    if constexpr (TW2 == 2)
        pin(first);
    return w;
}
__device__ __forceinline__ void lean_split(const Lane &L, f2 A, f2 Bv, int k, float e2, f2 &ub,
                                           f2 &un)
{
    lean_split_w(A, Bv, lean_tw2(L, k), e2, ub, un);
}

// unit spectrum of one mic row, in place (paired layout)
// (TWM, TW2: the depths of the column pass's and the split's twiddle reads)
template <bool PCM16, int TWM, int TW2, int NQ, typename Hook = NoHook>
__device__ __forceinline__ void lean_forward(const Lane &L, const uint32_t (&w)[16], const uint32_t (&wq)[NQ],
                                             f2 (&U)[33], float e2, Hook after_front = Hook())
{
    static_assert(TW2 == 1 || TW2 == 2 || TW2 == 16, "lean_forward: split twiddles one pair ahead or all 16");
    if constexpr (TW2 == 16) {
        // the split's 16 twiddles requested behind the row reads: their round
        // trip passes under the row's DFT-32
        f2 t2[16];
        lean_spectrum<PCM16, TWM>(L, w, wq, U, e2, after_front, [&] {
#pragma unroll
            for (int k = 0; k < 16; k++)
                t2[k] = lean_tw2(L, k);
        });
#pragma unroll
        for (int k = 0; k < 16; k++)
            lean_split_w(U[k], U[31 - k], t2[k], e2, U[k], U[31 - k]);
        return;
    }
    lean_spectrum<PCM16, TWM>(L, w, wq, U, e2, after_front);
#if P1K_TWPF & 1
    f2 wn = lean_tw2(L, 0);
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const f2 wk = wn;
        if (k < 15)
            wn = lean_tw2_next<TW2>(L, k + 1, U[k]);
        lean_split_w(U[k], U[31 - k], wk, e2, U[k], U[31 - k]);
    }
#else
#pragma unroll
    for (int k = 0; k < 16; k++)
        lean_split(L, U[k], U[31 - k], k, e2, U[k], U[31 - k]);
#endif
}

// unit spectrum V of one mic row consumed bin pair by bin pair as it is
// produced: A <- conj(A) V, B <- conj(B) V (V is never whole after the split)
template <bool PCM16, int TWM, int TW2, int NQ>
__device__ __forceinline__ void lean_forward_cross(const Lane &L, const uint32_t (&w)[16], const uint32_t (&wq)[NQ],
                                                   f2 (&A)[33], f2 (&Bs)[33], float e2)
{
    f2 V[33];
    lean_spectrum<PCM16, TWM>(L, w, wq, V, e2);
    A[32] = c_conjmul(A[32], V[32]);
    Bs[32] = c_conjmul(Bs[32], V[32]);
    // (TW2 = 2 requests one pair ahead here whatever P1K_TWPF says)
    constexpr bool AHEAD = (P1K_TWPF & 2) || TW2 == 2;
    [[maybe_unused]] f2 wn;
    if constexpr (AHEAD)
        wn = lean_tw2(L, 0);
#pragma unroll
    for (int k = 0; k < 16; k++) {
        f2 ub, un;
        if constexpr (AHEAD) {
            const f2 wk = wn;
            if (k < 15)
                wn = lean_tw2_next<TW2>(L, k + 1, V[k]);
            lean_split_w(V[k], V[31 - k], wk, e2, ub, un);
        } else
            lean_split(L, V[k], V[31 - k], k, e2, ub, un);
        A[k] = c_conjmul(A[k], ub);
        A[31 - k] = c_conjmul(A[31 - k], un);
        Bs[k] = c_conjmul(Bs[k], ub);
        Bs[31 - k] = c_conjmul(Bs[31 - k], un);
    }
}

// acc + d W_32^k (forward W), k compile-time after unrolling: two chained
// packed FMAs (one packed add for W = 1, -i)
__device__ __forceinline__ f2 cmac_fwd(f2 acc, f2 d, int k)
{
    if (k == 0)
        return acc + d;
    if (k == 8)
        return c_add_mi(acc, d);
    const f2 w = f2{(float)COS32D[k], -(float)COS32D[k < 8 ? 8 - k : k - 8]};
    return v_fma(v_yy(d), f2{-w.y, w.x}, v_fma(v_xx(d), w, acc));
}

// second half of the pruned inverse (fft_row_inv) in two groups of 8 residue
// pairs, so at most half a row of tile values is in registers at a time:
// y0 = sum of the row, y31 = sum_i (v_i - v_{i+16}) W_32^i accumulated by
// FMA in two chains per group
// (DEPTH 32, P1K_ROW_ROOMY: both groups' tile values requested at once -- one
// LDS round trip instead of two; the groups' sums are the same)
template <int DEPTH>
__device__ __forceinline__ void lean_row_inv(const Lane &L, const char *tile, f2 &y0, f2 &y31)
{
    static_assert(DEPTH == 16 || DEPTH == 32, "lean_row_inv: half a row or the whole row at once");
    const int ro = P1K_ROW * L.cs;
    f2 ga[2], gd[2];
    [[maybe_unused]] f2 rv[2][8], ru[2][8];
    if constexpr (DEPTH == 32) {
#pragma unroll
        for (int g = 0; g < 2; g++)
#pragma unroll
            for (int i = 0; i < 8; i++) {
                rv[g][i] = lds_f2(tile, ro + 8 * slot(8 * g + i));
                ru[g][i] = lds_f2(tile, ro + 8 * slot(8 * g + i + 16));
            }
    }
#pragma unroll
    for (int g = 0; g < 2; g++) {
        f2 a[8], c[2];
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const f2 v = DEPTH == 32 ? rv[g][i] : lds_f2(tile, ro + 8 * slot(8 * g + i));
            const f2 u = DEPTH == 32 ? ru[g][i] : lds_f2(tile, ro + 8 * slot(8 * g + i + 16));
            a[i] = v + u;
            const f2 d = v - u;
            c[i & 1] = i < 2 ? tw_only<false>(d, 8 * g + i) : cmac_fwd(c[i & 1], d, 8 * g + i);
        }
#pragma unroll
        for (int h = 4; h >= 1; h >>= 1)
#pragma unroll
            for (int r = 0; r < h; r++)
                a[r] = a[r] + a[r + h];
        ga[g] = a[0];
        gd[g] = c[0] + c[1];
        pin(ga[g]);
        pin(gd[g]);
    }
    y0 = ga[0] + ga[1];
    y31 = gd[0] + gd[1];
}

// residue of lane l (lane_res) in plain arithmetic (no divergent branch)
__device__ __forceinline__ int lane_res_sel(int l)
{
    const int h = l >> 1, o = l & 1;
    return h + o * (32 - 2 * h) - ((l == 1) << 4);
}


// the lane id through an opaque move: lane-dependent values derived from it
// are computed where they are used instead of being hoisted to the kernel's
// start and held in registers across every phase
__device__ __forceinline__ int fresh_tid()
{
    int t = (int)threadIdx.x;
    asm volatile("" : "+v"(t));
    return t;
}

// packed inverse input of the cross spectrum R (paired layout; R[k] =
// conj(A[k]) B[k] when B is given, else R = A), back in residue columns
// (TW2 16, P1K_TW2_ROOMY: the 16 twiddles requested at once ahead of the first pair)
template <bool CROSS, int TW2>
__device__ __forceinline__ void lean_pretwiddle(const Lane &L, const f2 (&A)[33], const f2 (&Bs)[33],
                                                f2 (&v)[32])
{
    static_assert(TW2 == 1 || TW2 == 2 || TW2 == 16, "lean_pretwiddle: twiddles one pair ahead or all 16");
    [[maybe_unused]] f2 t2[16];
    if constexpr (TW2 == 16) {
#pragma unroll
        for (int k = 0; k < 16; k++)
            t2[k] = lean_tw2(L, k);
    }
#if P1K_TWPF & 4
    [[maybe_unused]] f2 wn;
    if constexpr (TW2 != 16)
        wn = lean_tw2(L, 0);
#endif
#pragma unroll
    for (int k = 0; k < 16; k++) {
        f2 Rk = CROSS ? c_conjmul(A[k], Bs[k]) : A[k];
        const f2 Rn = CROSS ? c_conjmul(A[31 - k], Bs[31 - k]) : A[31 - k];
        f2 wk;
        if constexpr (TW2 == 16)
            wk = t2[k];
        else {
#if P1K_TWPF & 4
            wk = wn;
            if (k < 15)
                wn = lean_tw2_next<TW2>(L, k + 1, Rk);
#else
            wk = lean_tw2(L, k);
#endif
        }
        const f2 s = c_addconj(Rk, Rn);
        const f2 q = c_mulconj(c_subconj(Rk, Rn), wk);
        v[k] = c_add_i(s, q);
        v[31 - k] = c_conj_add_mi(s, q);
    }
    const f2 R32 = CROSS ? c_conjmul(A[32], Bs[32]) : A[32];
    const f2 Ye = f2{2.0f * R32.x, -2.0f * R32.y};  // Y[512] = 2 conj(R[512])
    swap_upper_exec<false>(v, Ye);
}

}  // namespace

// NW waves per workgroup, 2 NW frames:
//   NW = 8  (A/B: TDOA_P1K=lean8) one workgroup per CU, the whole table image in LDS, and the two
//           waves of a SIMD (w, w ^ 4) kept in step by balance();
//   NW = 4  (the product) two independent workgroups per CU (80 KiB of LDS each), usually of
//           consecutive launches and so at different phases: one's staging and
//           grid scan issue under the other's VALU-bound transforms.  LDS holds
//           the tiles and the image's prefix twm | tw2 | prior; the window
//           comes from kp.window with the row's words and the grid's tuple
//           words from the image in global memory (L2), two steps ahead.
//           Its grid solve scans only the rows of tuples whose upper bound
//           reaches the best L (P1K_GRID_PRUNE); NW = 8 scans every tuple.
// The per-frame arithmetic and its order are the same, and the pruned scan
// is exact, so all outputs are the same bytes.
// The body is tdoa_p1k_frames.inc, shared with k_p1k_pcm16 below.
template <int NW>
__global__ void __launch_bounds__(NW * 64, 2) k_p1k_lean(tdoa_kparams kp, tdoa_kout out,
                                                         const int16_t *__restrict__ frames, int64_t B,
                                                         float e2)
{
    constexpr bool PCM16 = false;
#include "tdoa_p1k_frames.inc"
}
// full-range int16 frames (TDOA_SAMPLES_PCM16): the product's 4-wave workgroup,
// launch shape, LDS budget, pruned grid scan and outputs of k_p1k_lean<4>
__global__ void __launch_bounds__(4 * 64, 2) k_p1k_pcm16(tdoa_kparams kp, tdoa_kout out,
                                                         const int16_t *__restrict__ frames, int64_t B,
                                                         float e2)
{
    constexpr int NW = 4;
    constexpr bool PCM16 = true;
#include "tdoa_p1k_frames.inc"
}

#ifdef TDOA_DIAG
extern "C" int tdoa_diag_fetch_p1k(unsigned long long *host, int n)
{
    if (n > (1 << 16))
        n = 1 << 16;
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_diag_p1k), sizeof(unsigned long long) * n, 0,
                               hipMemcpyDeviceToHost) == hipSuccess
               ? 0
               : -2;
}
#endif

// --------------------------------------------------------------- host side
namespace {
// waves per workgroup of the product's launch (the other shape is built into
// the A/B library only: TDOA_P1K=lean8 | lean4).  The 4-wave shape won every
// two-stream A/B pair against the parent's kernel, by ~0.55 us of 27.3; on one
// stream it is 12 % slower (profiles/c2_wg4_ab.txt).  Only the
// 4-wave shape prunes its grid scan (P1K_GRID_PRUNE: 1.46 us of 26.7 on two
// streams, profiles/c2_grid_prune_ab.txt); lean8 is the exhaustive scan's A/B build
#ifndef P1K_DEFAULT_NW
#define P1K_DEFAULT_NW 4
#endif

// dynamic LDS of a launch: the waves' tiles and the whole table image (8 waves)
// or the image's prefix twm | tw2 | prior (4 waves)
constexpr size_t p1k_lds(int nw, int img_bytes)
{
    return (size_t)nw * P1K_WAVE_LDS + (size_t)(nw == 4 ? P1K_IMG_LDS4 : img_bytes);
}

// the launched shape: P1K_DEFAULT_NW; in the A/B build TDOA_P1K=lean8 | lean4
int p1k_nw()
{
#if TDOA_AB
    static const int pick = [] {
        const char *e = getenv("TDOA_P1K");
        return e && !strcmp(e, "lean8") ? 8 : (e && !strcmp(e, "lean4") ? 4 : P1K_DEFAULT_NW);
    }();
    return pick;
#else
    return P1K_DEFAULT_NW;
#endif
}

template <int NW>
int p1k_launch(const tdoa_kparams &kp, const tdoa_kout &out, const int16_t *frames, int64_t B, float e2,
               hipStream_t stream)
{
    // one workgroup of 2 NW frames (one frame per half-wave)
    const int64_t grid = (B + 2 * NW - 1) / (2 * NW);
    if (grid > 0x7FFFFFFF)
        return tdoa_set_error(-1, "k_p1k_lean: batch too large for one launch");
    if (NW == 4 && kp.pcm16)
        hipLaunchKernelGGL(k_p1k_pcm16, dim3((unsigned)grid), dim3(NW * 64), p1k_lds(NW, p1k_img_lds8(kp)), stream, kp,
                           out, frames, B, e2);
    else
        hipLaunchKernelGGL(k_p1k_lean<NW>, dim3((unsigned)grid), dim3(NW * 64), p1k_lds(NW, p1k_img_lds8(kp)), stream,
                           kp, out, frames, B, e2);
    return 0;
}
}  // namespace

#ifdef TDOA_DIAG
// diagnostic build only: workgroups of the launched shape resident per CU
// (hipOccupancyMaxActiveBlocksPerMultiprocessor with its block and LDS size)
extern "C" int tdoa_diag_p1k_occupancy(int img_bytes, int *nw)
{
    int n = -1;
    *nw = p1k_nw();
    const hipError_t e = *nw == 4 ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_p1k_lean<4>, 4 * 64, p1k_lds(4, img_bytes))
                                  : hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_p1k_lean<8>, 8 * 64, p1k_lds(8, img_bytes));
    return e == hipSuccess ? n : -1;
}
#endif

// LDS table image of k_phat1024 (layout of the kernel's shared memory from twm on)
void tdoa_phat1024_image(int M, int N, int K, int U, const float *tw, const int32_t *win,
                         const float *prior, const uint32_t *tuples, const int32_t *tuple_cell,
                         std::vector<uint8_t> &img)
{
    img.clear();
    if (M != 3 || N != 1024 || K > P1K_KPAD - 1)
        return;
#if P1K_GROUPS
    // groups: tuples of equal (l0, l1) whose l2 are consecutive, at most 3 per
    // group (config 2: 1121 groups of 3 / 2 / 1 for 2469 tuples), bucketed by
    // size, each bucket in the order of its groups' first tuples (neighbouring
    // lanes, neighbouring cells and lag slots) and padded to whole waves
    struct Grp {
        int l0, l1, l2, n, u0;
        int cell[3];
    };
    std::map<std::pair<int, int>, std::vector<std::pair<int, int>>> by;  // (l0, l1) -> (l2, u)
    for (int u = 0; u < U; u++)
        by[{(int)(tuples[u] & 0xFFu), (int)((tuples[u] >> 8) & 0xFFu)}].push_back({(int)((tuples[u] >> 16) & 0xFFu), u});
    std::vector<Grp> bk[4];
    for (auto &kv : by) {
        auto &v = kv.second;
        std::sort(v.begin(), v.end());
        for (size_t i = 0; i < v.size();) {
            Grp g{kv.first.first, kv.first.second, v[i].first, 0, INT_MAX, {0, 0, 0}};
            while (i < v.size() && g.n < 3 && v[i].first == g.l2 + g.n) {
                if (tuple_cell[v[i].second] < 0 || tuple_cell[v[i].second] >= 0xFFFF)
                    return;  // cells are 16-bit in the table
                g.cell[g.n++] = tuple_cell[v[i].second];
                g.u0 = std::min(g.u0, v[i].second);
                i++;
            }
            bk[g.n].push_back(g);
        }
    }
    int nslot[4];
    for (int n = 1; n <= 3; n++) {
        std::sort(bk[n].begin(), bk[n].end(), [](const Grp &x, const Grp &y) { return x.u0 < y.u0; });
        nslot[n] = ((int)bk[n].size() + 127) / 128 * 128;  // whole pairs of 64-slot steps
    }
    const int ncell = 3 * nslot[3] + 2 * nslot[2] + nslot[1];
    const size_t bytes = (size_t)P1K_IMG_FIXED + 16 + 4 * (size_t)(nslot[3] + nslot[2] + nslot[1]) + 2 * (size_t)ncell;
    img.resize((bytes + 15) / 16 * 16);
#else
    const int Upad = p1k_upad(U);
#if P1K_CELL_LDS
    img.resize((size_t)P1K_IMG_FIXED + (size_t)Upad * 4 + (size_t)(Upad / 32) * 4);  // + the row cells
#else
    (void)tuple_cell;
    img.resize((size_t)P1K_IMG_FIXED + (size_t)Upad * 4);
#endif
#endif
    float *f = (float *)img.data();
    const float *tw2 = tw + 2 * N;
    for (int k = 0; k < 32; k++)  // twm [k][r] = W_1024^{r k}
        for (int r = 0; r < 32; r++) {
            const int i = (k * r) & (N - 1);
            f[2 * (32 * k + slot(r))] = tw[2 * i];
            f[2 * (32 * k + slot(r)) + 1] = tw[2 * i + 1];
        }
    f += 2 * 1024;
    for (int k = 0; k < 16; k++)  // tw2 [k][r] = W_2048^{r + 32 k}
        for (int r = 0; r < 32; r++) {
            const int b = r + 32 * k;
            f[2 * (32 * k + slot(r))] = tw2[2 * b];
            f[2 * (32 * k + slot(r)) + 1] = tw2[2 * b + 1];
        }
    f += 2 * 512;
    for (int k = 0; k < 128; k++)
        f[k] = k < K ? prior[k] : 0.0f;
    f += 128;  // (the 4-wave workgroup's LDS prefix ends here: P1K_IMG_LDS4)
    for (int e = 0; e < 512; e++) {  // (W[2e], W[2e+1]) / 128, word e = 32 t + r at slot(r)
        const int d = (e & ~31) + slot(e & 31);
        f[2 * d] = (float)win[2 * e] * (1.0f / 128.0f);
        f[2 * d + 1] = (float)win[2 * e + 1] * (1.0f / 128.0f);
    }
    uint32_t *t = (uint32_t *)(f + 2 * 512);
#if P1K_GROUPS
    // header: slots per bucket (n = 3, 2, 1), tuple 0's cell; then the group
    // words (LDS byte offsets of l0, l1 and the first l2 in a wave's [p][KPAD]
    // f2 score table, 10 bits each; padding groups start at slot 127 of every
    // pair, -inf) and the member cells (u16, bucket n: [slot][n])
    int32_t *hdr = (int32_t *)t;
    hdr[0] = nslot[3];
    hdr[1] = nslot[2];
    hdr[2] = nslot[1];
    hdr[3] = U > 0 ? tuple_cell[0] : 0;
    t += 4;
    uint16_t *cl = (uint16_t *)(t + nslot[3] + nslot[2] + nslot[1]);
    for (int n = 3; n >= 1; n--) {
        for (int e = 0; e < nslot[n]; e++) {
            const bool real = e < (int)bk[n].size();
            const Grp g = real ? bk[n][e] : Grp{127, 127, 128 - n, n, 0, {0xFFFF, 0xFFFF, 0xFFFF}};
            *t++ = ((uint32_t)g.l0 << 3) | ((uint32_t)g.l1 << 13) | ((uint32_t)g.l2 << 23);
            for (int j = 0; j < n; j++)
                *cl++ = (uint16_t)g.cell[j];
        }
    }
#else
    // tuples as LDS byte offsets into a wave's [p][KPAD] f2 score table, 10 bits
    // per pair; padding tuple (127, 127, 127) scores -inf
#if P1K_CELL_LDS
    // (lag slots 7 bits each, then the first cell minus its 32-tuple row's
    // first cell in 11 bits; a table with a row that spans more has no image:
    // the generic kernel runs it)
    int32_t *rowcell = (int32_t *)(t + Upad);
    for (int r = 0; r < Upad / 32; r++) {
        const int e0 = 32 * r, e1 = std::min(U, e0 + 32) - 1;
        rowcell[r] = e0 >= U ? 0 : tuple_cell[e0];
        if (e0 < U && tuple_cell[e1] - tuple_cell[e0] >= 2048) {
            img.clear();
            return;
        }
    }
    for (int e = 0; e < Upad; e++) {
        const uint32_t wd = e < U ? tuples[e] : 0x007F7F7Fu;
        const uint32_t dc = e < U ? (uint32_t)(tuple_cell[e] - rowcell[e >> 5]) : 0u;
        t[e] = ((wd & 0x7Fu) << 3) | (((wd >> 8) & 0x7Fu) << 10) | (((wd >> 16) & 0x7Fu) << 17) |
               ((dc & 0xFFu) << 24) | (dc >> 8);
    }
#else
    for (int e = 0; e < Upad; e++) {
        const uint32_t wd = e < U ? tuples[e] : 0x007F7F7Fu;
        t[e] = ((wd & 0xFFu) << 3) | (((wd >> 8) & 0xFFu) << 13) | (((wd >> 16) & 0xFFu) << 23);
    }
#if P1K_GRID_PRUNE
    // the pruned scan's row table, appended (16-B aligned: Upad is a multiple
    // of 512); a table of more than 64 rows has no image: the generic kernel
    // runs it, as it does every table the 8-wave workgroup cannot stage
    std::vector<uint32_t> sec;
    tdoa_p1k_prune_section(U, tuples, tuple_cell, sec);
    if (sec.empty()) {
        img.clear();
        return;
    }
    sec.resize((sec.size() + 3) / 4 * 4);
    const uint8_t *sb = (const uint8_t *)sec.data();
    img.insert(img.end(), sb, sb + sec.size() * 4);
#endif
#endif
#endif
}

// config-2 shape (M = 3, N = 1024, S <= 63) with a tuple table that fits the tail
bool tdoa_phat1024_fits(const tdoa_kparams &kp)
{
    if (kp.M != 3 || kp.N != 1024 || kp.S > 63 || kp.TW != 1 || !kp.p1k_img)
        return false;
    // grid scores of a wave's two frames live in its tiles: [3][KPAD] float2 = 3 KiB
    static_assert(3 * P1K_KPAD * 8 <= P1K_WAVE_LDS, "grid scores exceed the wave's tiles");
    // the image loads as at most 4 units of 16 B per thread (k_p1k_lean's staging)
    // and, with 8 waves' tiles and the static progress words, fits the CU's LDS.
    // The 4-wave shape stages a fixed prefix only, so the same contexts fit it.
    // (The pruned scan's row table after the staged bytes stays in global
    // memory; a staged part within 32 KiB has at most 56 rows of 64 tuples.)
    const int lds8 = p1k_img_lds8(kp);
    return lds8 <= kp.p1k_img_bytes && lds8 <= 4 * 8 * 64 * 16 && p1k_lds(8, lds8) + 64 <= 160 * 1024;
}

int tdoa_launch_phat1024(const tdoa_kparams &kp, const tdoa_kout &out, const int16_t *frames,
                         int64_t B, float phat_eps, void *stream)
{
    // per-mic floor: |X_m|^2 + eps in the oracle's units (x / 2^15, X / 2),
    // i.e. |X|^2 + eps * 2^32 in the kernel's int16 units with the split's factor 2
    float e2 = phat_eps * 4294967296.0f;
    if (!(e2 >= 1e-30f))
        e2 = 1e-30f;
    if (B <= 0)
        return 0;
    int rc;
#if TDOA_AB
    // (a PCM16 context ignores TDOA_P1K: its kernel has the 4-wave shape only)
    rc = p1k_nw() == 4 || kp.pcm16 ? p1k_launch<4>(kp, out, frames, B, e2, (hipStream_t)stream)
                                   : p1k_launch<8>(kp, out, frames, B, e2, (hipStream_t)stream);
#else
    rc = p1k_launch<P1K_DEFAULT_NW>(kp, out, frames, B, e2, (hipStream_t)stream);
#endif
    if (rc)
        return rc;
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        char buf[256];
        snprintf(buf, sizeof buf, "k_p1k_lean launch: %s", hipGetErrorString(e));
        return tdoa_set_error(-2, buf);
    }
    return 0;
}
