// tdoa_internal.h -- layout contract between the host side (tdoa_capi.cpp,
// tdoa_stream.cpp) and the gfx950 kernels (the .hip files beside it), and the
// one set of declarations of every function that crosses a translation unit.
// Not part of the public ABI.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include <hip/hip_runtime.h>

#include "tdoa_shared.h"  // constants, tdoa_kparams, tdoa_set_error / tdoa_fail

// Lanes of one wave exchanging data through LDS (transpose tiles, score
// tables, staging rows): the wave's DS instructions execute in issue order,
// but the compiler models each lane as a thread of its own and may move one
// lane's LDS write past a later read it cannot prove disjoint.  The wavefront-
// scope release/acquire fences order the memory operations at the IR level
// (they emit no instruction for LDS); the wave barrier between them keeps the
// lanes together (rocPRIM's wave-sync pattern).
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The least-squares refinement's sub-sample lag (tdoa_ls.hip, oracle
// orc_ls_refine): the argmax plus the parabolic vertex of the raw scores
// y0, y1, y2 at lags best - 1, best, best + 1, clamped to +-0.5; none at the
// lag range's ends (inside = false) or without a maximum (den >= 0).  One
// definition for k_ls and the kernels that keep the scores on chip, rounded
// as the C oracle (no contraction whatever the TU's flags).
__device__ __forceinline__ double ls_tau3(double y0, double y1, double y2, int best, bool inside)
{
#pragma clang fp contract(off)
    double d = 0.0;
    if (inside) {
        const double den = y0 - 2.0 * y1 + y2;
        if (den < 0.0) {
            d = 0.5 * (y0 - y2) / den;
            d = d < -0.5 ? -0.5 : (d > 0.5 ? 0.5 : d);
        }
    }
    return (double)best + d;
}

// correlations.c:40-43: the EMA decay from the stream clock, in the
// reference's float / double steps (no contraction whatever the TU's flags)
__device__ __forceinline__ float tdoa_decay_dev(uint64_t now, uint64_t last)
{
#pragma clang fp contract(off)
    const float dt = (float)(now - last) / 1e6f;
    const float arg = -dt / 0.5f;
    return (float)(1.0 - exp((double)arg));
}

struct tdoa_kout {
    int32_t *lags;
    uint8_t *gate;
    int32_t *cell;
    float *xy;
    int64_t *max_L;
    float *max_Lf;
    int64_t *scores;
    int64_t *weighted;
    float *scores_f;
    float *weighted_f;
    // per pair the raw scores at lags best - 1, best, best + 1 (the least-
    // squares refinement's parabolic vertex, tdoa_ls.hip): [B][P][3]; written by
    // the kernels that keep the scores on chip (k_frame16) instead of scores_f
    // (slots outside the lag range are not written and not read)
    float *peak3;
    // the compact weighted-score scratch ([B][kp.wc_CK], see tdoa_kparams),
    // written by k_frame16 and read by k_grid_bb in place of weighted_f
    float *weighted_c;
};

// Outputs of k_peaks (tdoa_peaks.hip): tdoa_peaks_outputs without the
// refinement's fields; cell is never null (scratch if the caller passed none).
struct tdoa_peaks_kout {
    int32_t *count;
    int32_t *cell;
    float *xy;
    int64_t *L;
    float *Lf;
    int32_t *lags;
};

// Streaming state of one pipeline (tdoa_stream.hip); all device pointers.
struct tdoa_stream_params {
    int32_t M, N, H, log2N, fs;
    int64_t capture_len;      // samples per stream in the capture ring
    const uint8_t *capture;   // [S][capture_len][M] 8-bit ADC bytes, round-robin; of a PCM16
                              // pipeline int16 samples (its kernels cast it)
    int64_t *pos;             // [1] samples consumed (device clock)
    int64_t *ring_start;      // [S] sample index of the last trigger (rings restart there)
    int32_t *count;           // [1] frames triggered this step
    int32_t *count_next;      // [1] the next step's counter: zeroed by this step's trigger
                              // (two counters alternate by hop parity: no memset node)
    // the hop's listed frames, written by its selector (a trigger or
    // k_stream_active) and staged from the capture ring by the hop kernel
    int32_t *ids;             // [S] compact slot -> stream
    int64_t *end;             // [S] samples consumed at the frame's end (always >= N)
    int64_t *ring_at;         // [S] ring index of the slot's first frame sample
    int64_t *fresh;           // [S][P][K] their weighted scores (k_direct)
    int32_t *fresh_lags;      // [S][P]
    uint8_t *fresh_gate;      // [S]
    int64_t *est;             // [S][P][K] EMA scores per stream
    uint64_t *last;           // [S] EMA clock per stream (us)
    int64_t *stats;           // [2] running totals: triggered frames, gated frames
};

struct tdoa_stream_kout {
    int32_t *count;
    int32_t *stream_id;
    int64_t *end;
    int32_t *lags;
    uint8_t *gate;
    int32_t *ema_best;
    int32_t *cell;
    float *xy;
    int64_t *max_L;
};

// Resident workgroups of `kernel` (threads, dynamic LDS) on the current device:
// blocks per CU from the occupancy query x CUs, cached per (device, kernel,
// threads, LDS) under a mutex (contexts on different host threads / devices).
int tdoa_resident_blocks(const void *kernel, int threads, size_t lds);

// A failed launch or runtime call: "<what>: <HIP's text>" as the thread's last
// error, returns TDOA_ERR_HIP (tdoa_capi.cpp).
int tdoa_hip_fail(hipError_t e, const char *what);

// The per-mic PHAT floor of U = X / sqrt(|X|^2 + eps) (include/tdoa.h) for x
// scaled by 2^-15, kept a normal float (v_rsq_f32 flushes denormals, and a zero
// bin must stay 0); and the same for kernels whose samples stay in int16 units,
// where |X|^2 is 2^30 times as large.
inline float tdoa_phat_floor(float phat_eps) { return phat_eps >= 1e-30f ? phat_eps : 1e-30f; }
inline float tdoa_phat_floor_int16(float phat_eps) { return tdoa_phat_floor(phat_eps) * 1073741824.0f; }

// Shapes the LDS Stockham kernels hold (tdoa_phat_lds.h: the two-pass route and
// the streaming hop): N a power of two in [256, 4096], K = 2S + 1 <= 127 (two
// argmax candidates per lane of one wave).
inline bool tdoa_phat_lds_shape(int N, int K) { return N >= 256 && N <= 4096 && !(N & (N - 1)) && K <= 127; }

// Host-side launchers implemented in the .hip files.
// count_dev (optional): device int32 batch size, B then only bounds the grid.
// ema (optional, streaming): the launch also runs the EMA of the gated frames
// and the grid on the EMA scores (k_direct_mfma only: tdoa_direct_fused_grid)
struct tdoa_stream_fuse {
    tdoa_stream_params sp;
    tdoa_stream_kout so;
};
int tdoa_launch_direct(const tdoa_kparams &kp, const tdoa_kout &out,
                       const int16_t *frames, int64_t B, bool prepared,
                       void *stream, int *lds_bytes_out,
                       const int32_t *count_dev = nullptr, const tdoa_stream_fuse *ema = nullptr);
// the DIRECT launch for this shape also solves the grid (k_direct_mfma)
bool tdoa_direct_fused_grid(const tdoa_kparams &kp);
// ... and can also run the streaming EMA (tdoa_stream_fuse)
bool tdoa_direct_ema_fits(const tdoa_kparams &kp);
int tdoa_launch_heatmap(const tdoa_kparams &kp, const void *weighted, const void *max_L,
                        bool is_float, int64_t B, uint8_t *classes, void *stream);
// per_frame > 0 (tdoa_peaks): the B rows are per_frame peaks of each of
// B / per_frame score frames -- row f reads the scores of frame f / per_frame,
// and a row whose cell is negative (an empty slot) gets NaN instead of the clamp
int tdoa_launch_ls(const tdoa_kparams &kp, const void *scores, bool is_float, const float *peak3,
                   const int32_t *lags, const int32_t *cells, float *xy_ls, float *rms,
                   int64_t B, void *stream, int per_frame = 0);
// k_peaks (tdoa_peaks.hip): its dynamic LDS for this context and score type,
// and whether that fits the budget
size_t tdoa_peaks_lds(const tdoa_kparams &kp, bool is_float);
bool tdoa_peaks_fits(const tdoa_kparams &kp, bool is_float);
int tdoa_launch_peaks(const tdoa_kparams &kp, const tdoa_peaks_kout &out, const void *scores,
                      bool is_float, int64_t B, int num_peaks, int radius, float min_rel,
                      void *stream);
// k_stream_peaks / k_ls_stream (tdoa_stream_peaks): k_peaks and the per-peak
// refinement over the frames a streaming step listed -- the batch size is
// *count (device, clamped to [0, S]), slot i's score block is
// est + ids[i] * P * K, output row i; gate (optional, device [S]): a slot whose
// byte is 0 gets the empty record
int tdoa_launch_stream_peaks(const tdoa_kparams &kp, const tdoa_peaks_kout &out, const void *est,
                             bool is_float, const int32_t *ids, const int32_t *count, const uint8_t *gate,
                             int64_t S, int num_peaks, int radius, float min_rel, void *stream);
int tdoa_launch_ls_stream(const tdoa_kparams &kp, const void *est, bool is_float, const int32_t *ids,
                          const int32_t *count, int64_t S, const int32_t *lags, const int32_t *cells,
                          float *xy_ls, float *rms, int per_frame, void *stream);
size_t tdoa_stream_trigger_lds(int M, int N, int H);
// The hop's frame selectors.  Each lists the frames it chooses as sp.ids[slot],
// sp.end[slot] (>= N: no frame reaches before its stream's start) and
// sp.ring_at[slot], counts them in *sp.count and zeroes *sp.count_next; the hop
// kernel (DIRECT or k_stream_phat*) stages each frame from its stream's ring.
// The trigger: k_stream_trigger_p where it applies (8-bit rings, N = 2 hop,
// M <= 4, aligned capture), else k_stream_trigger_lds<T> (T = int16_t for pcm16
// else uint8_t); thr = trigger_var * (N/2)^2, POWER_THRESHOLD = 2 for 8-bit
int tdoa_launch_stream_trigger(const tdoa_stream_params &sp, int64_t S, int64_t thr, bool pcm16, void *stream);
// continuous mode's frame lister in place of a trigger (k_stream_active<T, M>):
// every stream whose frame [e - N, e), e = pos + H >= N, has
// sum_m (N sum x_m^2 - (sum x_m)^2) >= thr, with thr = activity_var * N^2;
// ring_start is not touched
int tdoa_launch_stream_active(const tdoa_stream_params &sp, int64_t S, int64_t thr, bool pcm16, void *stream);
int tdoa_launch_stream_update(const tdoa_stream_params &sp, const tdoa_kparams &kp,
                              const tdoa_stream_kout &out, int64_t S, void *stream);
// the GCC_PHAT hop after the selector (tdoa_stream_phat.hip, k_stream_phat):
// its dynamic LDS, whether the shape fits, the launch size for S streams
// (resident workgroups, capped by `cap` > 0), and the launch -- est is the
// float EMA state [S][P][K] (sp.est, sp.fresh* are not read); pcm16: the
// int16-ring kernel (k_stream_phat_pcm16)
size_t tdoa_stream_phat_lds(const tdoa_kparams &kp);
bool tdoa_stream_phat_fits(const tdoa_kparams &kp);
int tdoa_stream_phat_grid(const tdoa_kparams &kp, int64_t S, int cap, bool pcm16 = false);
int tdoa_launch_stream_phat(const tdoa_stream_params &sp, const tdoa_kparams &kp, const tdoa_stream_kout &out,
                            float *est, float *max_Lf, int64_t S, float phat_eps, int grid, void *stream,
                            bool pcm16 = false);
// the GCC_PHAT hop of the long-frame shapes k_stream_phat's LDS cannot hold
// (8 mics x 2048, 4 x 4096): k_f16_ring (tdoa_phat_r16.hip: k_frame16's body
// over the step's listed frames, staged from the capture rings; kp.bin_w picks
// the weighted instantiation) writes by slot lags [S][P], gate [S] and the
// weighted scores [S][P][K], and k_stream_ema_grid (tdoa_stream_phat.hip) runs
// record, EMA and grid scan on them and the step's bookkeeping.  A stream's
// ring must stay under 2^31 bytes (32-bit sample offsets in the kernel).
bool tdoa_f16_ring_shape(const tdoa_kparams &kp);
// (its launch size for S streams, capped by `cap` > 0; 0: no workgroup fits)
int tdoa_f16_ring_grid(const tdoa_kparams &kp, int64_t S, int cap, bool pcm16);
int tdoa_launch_f16_ring(const tdoa_stream_params &sp, const tdoa_kparams &kp, int32_t *lags, uint8_t *gate,
                         float *weighted, int64_t S, float phat_eps, int grid, void *stream, bool pcm16);
int tdoa_stream_ema_grid_size(const tdoa_kparams &kp, int64_t S, int cap);
int tdoa_launch_stream_ema_grid(const tdoa_stream_params &sp, const tdoa_kparams &kp, const tdoa_stream_kout &out,
                                float *est, float *max_Lf, const float *weighted, const int32_t *lags,
                                const uint8_t *gate, int64_t S, int grid, void *stream);
int tdoa_launch_average(const tdoa_kparams &kp, int64_t S, int64_t *est,
                        const int64_t *fresh, const float *decay, int32_t *best,
                        const tdoa_kout *solve, void *stream);
int tdoa_launch_grid(const tdoa_kparams &kp, const tdoa_kout &out, const void *weighted,
                     bool is_float, int64_t B, void *stream);
int tdoa_launch_gcc_phat(const tdoa_kparams &kp, const tdoa_kout &out,
                         const int16_t *frames, int64_t B, float phat_eps,
                         void *spec_scratch, size_t spec_bytes, void *stream);
// GCC-PHAT shapes the fused kernels cannot hold (M > 3 or N > 2048): two
// passes per chunk of frames through a spectrum scratch (tdoa_phat_split.hip)
bool tdoa_gcc_phat_needs_split(int M, int N);
// config-2 GCC-PHAT kernel (tdoa_phat1024.hip): host-built LDS table image
// from the twiddles ([N] e^{-2 pi i k/N} then [N+1] e^{-2 pi i k/2N}),
// Q15 window, lag prior and distinct lag tuples with their first cells; empty
// if the shape differs
void tdoa_phat1024_image(int M, int N, int K, int U, const float *tw, const int32_t *win,
                         const float *prior, const uint32_t *tuples, const int32_t *tuple_cell,
                         std::vector<uint8_t> &img);
// the one-frame-per-wave config-2 kernel (tdoa_p1k_w64.hip): its image
void tdoa_p1k_w64_image(int M, int N, int K, int U, const int32_t *win, const float *prior,
                        const uint32_t *tuples, std::vector<uint8_t> &img);
bool tdoa_gcc_phat_fused_grid(const tdoa_kparams &kp);
// the kernels tdoa_launch_gcc_phat chooses between (tdoa_gcc_phat.hip), each
// with the predicate that says whether it holds the shape:
// the N = 1024, 3-mic kernel, which runs the grid solve itself (tdoa_phat1024.hip)
bool tdoa_phat1024_fits(const tdoa_kparams &kp);
int tdoa_launch_phat1024(const tdoa_kparams &kp, const tdoa_kout &out, const int16_t *frames,
                         int64_t B, float phat_eps, void *stream);
// one frame per 64-lane wave (tdoa_p1k_w64.hip, A/B build only)
bool tdoa_p1k_w64_fits(const tdoa_kparams &kp);
int tdoa_launch_p1k_w64(const tdoa_kparams &kp, const tdoa_kout &out, const int16_t *frames, int64_t B,
                        float phat_eps, void *stream);
// the register-pass long-frame kernels (tdoa_phat_r16.hip): the shape fits,
// the per-frame kernel (k_frame16) runs it, under which name, whether it
// writes kout.peak3, and whether it solves the grid too
bool tdoa_phat_r16_fits(int M, int N, int S);
bool frame16_shape(const tdoa_kparams &kp);
const char *frame16_kernel_name(const tdoa_kparams &kp);
bool tdoa_phat_r16_peak3(const tdoa_kparams &kp);
bool tdoa_frame16_fused_grid(const tdoa_kparams &kp);
int tdoa_launch_phat_r16(const tdoa_kparams &kp, const tdoa_kout &out, const int16_t *frames, int64_t B,
                         float phat_eps, void *scratch, size_t scratch_bytes, void *stream);
// the first kernel a GCC-PHAT batch runs for this shape (tdoa_batch_kernel)
const char *tdoa_gcc_phat_kernel_name(const tdoa_kparams &kp);
// the float grid runs k_grid_bb and can read the compact scratch (tdoa_grid.hip)
bool tdoa_grid_bb_compact(const tdoa_kparams &kp);
bool tdoa_gcc_phat_grid_in_kernel(const tdoa_kparams &kp);
bool tdoa_gcc_phat_peak3(const tdoa_kparams &kp);
int tdoa_launch_gcc_phat_split(const tdoa_kparams &kp, const tdoa_kout &out,
                               const int16_t *frames, int64_t B, float eps_int16,
                               void *scratch, size_t scratch_bytes, void *stream);
// the reference ABI's per-buffer steps on the device (tdoa_direct.hip)
int tdoa_launch_ref_buffer(int op, int16_t *buf, const int16_t *ring, int head, int64_t *power,
                           const int16_t *window, int n, void *stream, int16_t *s1, int16_t *s2);

// what the streaming pipeline and the reference ABI read of a context
// (tdoa_capi.cpp)
struct tdoa_ctx;
const tdoa_kparams *tdoa_ctx_kparams(const tdoa_ctx *c);
int tdoa_ctx_device(const tdoa_ctx *c);
int tdoa_ctx_engine(const tdoa_ctx *c);
int tdoa_ctx_rate(const tdoa_ctx *c);
float tdoa_ctx_phat_eps(const tdoa_ctx *c);
