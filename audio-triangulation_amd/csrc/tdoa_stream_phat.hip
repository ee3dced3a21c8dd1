// tdoa_stream_phat.hip -- the streaming hop of a GCC_PHAT pipeline after the
// trigger (tdoa_stream.hip): what k_direct_mfma's fused EMA form does for
// DIRECT, as one kernel.
//
//   k_stream_phat  one 256-thread workgroup per triggered slot, persistent over
//                  the device-side count.  Per slot: the frame's 8-bit samples
//                  from its stream's capture ring (the selectors list frames,
//                  none copies one) -- or, as k_stream_phat_pcm16, its int16
//                  samples from an int16 ring and the 16-bit front end
//                  (TDOA_SAMPLES_PCM16); per mic
//                  the integer front end, the complex FFT_N of z[n] = x[2n] +
//                  i x[2n+1] in LDS, the real-FFT split and the PHAT unit
//                  spectrum U_m = X_m / sqrt(|X_m|^2 + eps), kept in LDS for
//                  all M mics; per pair R = conj(U_i) U_j (times the context's
//                  per-bin weights when a table is in force), the inverse FFT
//                  in one work buffer, lags -S..S, first maximum, lag prior;
//                  gate; for gated frames the float EMA on the stream's scores
//                      est <- est + (fresh - est) * decay(now, last[s])
//                  (fp32, no contraction; now = end * 1e6 / fs), the EMA rows'
//                  first maxima and the grid solve on the EMA scores over the
//                  distinct lag tuples (float L, first tuple on ties).
//   k_stream_ema_grid  the part after the lag prior alone, for the long-frame
//                  shapes whose scores k_f16_ring (tdoa_phat_r16.hip) computes:
//                  it reads each slot's lags, gate and weighted scores from a
//                  scratch in place of LDS.  One text: tdoa_stream_ema_grid.inc.
//
// Every stage from the front end to the lag prior is a function of
// tdoa_phat_lds.h, the one k_phat_spectra and k_phat_pairs call, so a frame's
// scores are those of the two-pass route.  What is this file's own: the slot
// staging, the gate and the record, the float EMA, the EMA rows' maxima, the
// grid scan and the diagnostic stamps.  Samples stay in int16 units (eps x 2^30).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <climits>

#include "tdoa_internal.h"
#include "tdoa_phat_lds.h"


namespace {

// diagnostic build only (libtdoa_diag.so): s_memtime cycles per phase summed by
// each workgroup's thread 0 over its slots of the last hop -- [0] staging,
// [1] front ends and forward FFTs, [2] pairs, [3] EMA and grid, [4] slots
#ifdef TDOA_DIAG
#define SP_DIAG_WG 4096
__device__ unsigned long long g_diag_sp[SP_DIAG_WG * 8];
#define SP_T0() unsigned long long sp_t_ = __builtin_amdgcn_s_memtime(), sp_acc_[5] = {0, 0, 0, 0, 0}
#define SP_MARK(k)                                                  \
    do {                                                            \
        const unsigned long long n_ = __builtin_amdgcn_s_memtime(); \
        sp_acc_[k] += n_ - sp_t_;                                   \
        sp_t_ = n_;                                                 \
    } while (0)
#define SP_FLUSH()                                                           \
    do {                                                                     \
        if (threadIdx.x == 0 && blockIdx.x < SP_DIAG_WG)                     \
            for (int k_ = 0; k_ < 5; k_++)                                   \
                g_diag_sp[(size_t)blockIdx.x * 8 + k_] = sp_acc_[k_];        \
    } while (0)
#else
#define SP_T0() \
    do {        \
    } while (0)
#define SP_MARK(k) \
    do {           \
    } while (0)
#define SP_FLUSH() \
    do {           \
    } while (0)
#endif

// correlations.c:44-47 on float scores: one EMA step, rounded step by step
__device__ __forceinline__ float ema_step(float est, float fresh, float dec)
{
#pragma clang fp contract(off)
    const float delta = (fresh - est) * dec;
    return est + delta;
}

__global__ void __launch_bounds__(TPB) k_stream_phat(tdoa_stream_params sp, tdoa_kparams kp, tdoa_stream_kout out,
                                                     float *__restrict__ est_all, float *__restrict__ max_Lf,
                                                     int nstreams, float e2)
{
    constexpr bool PCM16 = false, SCRATCH = false;
    constexpr const int32_t *lags_in = nullptr;  // (SCRATCH only)
    constexpr const uint8_t *gate_in = nullptr;
#include "tdoa_stream_phat_hop.inc"
}

// int16 capture rings (tdoa_stream_create_pcm16)
__global__ void __launch_bounds__(TPB) k_stream_phat_pcm16(tdoa_stream_params sp, tdoa_kparams kp,
                                                           tdoa_stream_kout out, float *__restrict__ est_all,
                                                           float *__restrict__ max_Lf, int nstreams, float e2)
{
    constexpr bool PCM16 = true, SCRATCH = false;
    constexpr const int32_t *lags_in = nullptr;  // (SCRATCH only)
    constexpr const uint8_t *gate_in = nullptr;
#include "tdoa_stream_phat_hop.inc"
}

// The hop's second half for the long-frame shapes, after k_f16_ring
// (tdoa_phat_r16.hip) left every listed slot's lags, gate and weighted scores
// [S][P][K] in global memory: one 256-thread workgroup per slot, persistent over
// the device-side count; record, float EMA, EMA rows' maxima and the grid scan
// are tdoa_stream_ema_grid.inc, the text k_stream_phat runs.  Workgroup 0 does
// the step's bookkeeping as k_stream_phat does.
__global__ void __launch_bounds__(TPB) k_stream_ema_grid(tdoa_stream_params sp, tdoa_kparams kp, tdoa_stream_kout out,
                                                         float *__restrict__ est_all, float *__restrict__ max_Lf,
                                                         const float *__restrict__ weighted,
                                                         const int32_t *__restrict__ lags_in,
                                                         const uint8_t *__restrict__ gate_in, int nstreams)
{
    constexpr bool SCRATCH = true;
    constexpr const int *lag_s = nullptr;  // (LDS kernels only)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int P = kp.P, K = kp.K, S = kp.S, tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6, nwaves = TPB / 64;
    float *E = (float *)smem;  // [P][K] the stream's EMA scores
    __shared__ float redv[TPB / 64];
    __shared__ int redi[TPB / 64];
    // at most one slot per stream: a corrupted counter cannot index past [S]
    const int cnt_raw = *sp.count;
    const int cnt = cnt_raw < 0 ? 0 : (cnt_raw > nstreams ? nstreams : cnt_raw);
    if (blockIdx.x == 0 && tid == 0) {
        *sp.pos += sp.H;  // the selector has read it
        sp.stats[0] += cnt;
        if (out.count)
            *out.count = cnt;
    }
    int ngated = 0;  // this workgroup's gated frames
    for (int slot = blockIdx.x; slot < cnt; slot += gridDim.x) {
        __syncthreads();  // the previous slot's scores and reductions are consumed
        int s = sp.ids[slot];
        s = s < 0 ? 0 : (s >= nstreams ? nstreams - 1 : s);  // k_f16_ring's clamp
        const int64_t end = sp.end[slot];
        const float *Wf = weighted + (size_t)slot * P * K;
#include "tdoa_stream_ema_grid.inc"
    }
    // gated frames of this hop: one atomic per workgroup that had any
    if (tid == 0 && ngated)
        atomicAdd(reinterpret_cast<unsigned long long *>(sp.stats + 1), (unsigned long long)ngated);
}

}  // namespace

#ifdef TDOA_DIAG
extern "C" int tdoa_diag_fetch_stream_phat(unsigned long long *host, int n)
{
    if (n > SP_DIAG_WG * 8)
        n = SP_DIAG_WG * 8;
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_diag_sp), sizeof(unsigned long long) * n, 0,
                               hipMemcpyDeviceToHost) == hipSuccess
               ? 0
               : -2;
}
#endif

size_t tdoa_stream_phat_lds(const tdoa_kparams &kp)
{
    return (size_t)kp.M * kp.N * 8 + (size_t)kp.N * 8 + 2 * (size_t)kp.P * kp.K * 4;
}

// 160 KiB per workgroup, less the kernel's static tables (under 1 KiB)
static constexpr size_t LDS_BUDGET = 160 * 1024 - 1024;

bool tdoa_stream_phat_fits(const tdoa_kparams &kp)
{
    return tdoa_phat_lds_shape(kp.N, kp.K) && tdoa_stream_phat_lds(kp) <= LDS_BUDGET;
}

int tdoa_stream_phat_grid(const tdoa_kparams &kp, int64_t S, int cap, bool pcm16)
{
    const int res = tdoa_resident_blocks(pcm16 ? (const void *)k_stream_phat_pcm16 : (const void *)k_stream_phat, TPB,
                                         tdoa_stream_phat_lds(kp));
    int64_t grid = S;
    if (res > 0 && grid > res)
        grid = res;
    if (cap > 0 && grid > cap)
        grid = cap;
    return (int)(grid > 0 ? grid : 1);
}

int tdoa_stream_ema_grid_size(const tdoa_kparams &kp, int64_t S, int cap)
{
    const int res = tdoa_resident_blocks((const void *)k_stream_ema_grid, TPB, (size_t)kp.P * kp.K * sizeof(float));
    int64_t grid = S;
    if (res > 0 && grid > res)
        grid = res;
    if (cap > 0 && grid > cap)
        grid = cap;
    return (int)(grid > 0 ? grid : 1);
}

int tdoa_launch_stream_ema_grid(const tdoa_stream_params &sp, const tdoa_kparams &kp, const tdoa_stream_kout &out,
                                float *est, float *max_Lf, const float *weighted, const int32_t *lags,
                                const uint8_t *gate, int64_t S, int grid, void *stream)
{
    hipLaunchKernelGGL(k_stream_ema_grid, dim3((unsigned)(grid > 0 ? grid : 1)), dim3(TPB),
                       (size_t)kp.P * kp.K * sizeof(float), (hipStream_t)stream, sp, kp, out, est, max_Lf, weighted,
                       lags, gate, (int)S);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : tdoa_hip_fail(e, "k_stream_ema_grid launch");
}

int tdoa_launch_stream_phat(const tdoa_stream_params &sp, const tdoa_kparams &kp, const tdoa_stream_kout &out,
                            float *est, float *max_Lf, int64_t S, float phat_eps, int grid, void *stream,
                            bool pcm16)
{
    if (!tdoa_stream_phat_fits(kp))
        return tdoa_set_error(-1, "stream GCC_PHAT: shape exceeds the LDS budget");
    if (pcm16) {
        // the floor of the two-pass PCM16 route (tdoa_launch_gcc_phat): s is in int16 units too
        hipLaunchKernelGGL(k_stream_phat_pcm16, dim3((unsigned)(grid > 0 ? grid : 1)), dim3(TPB),
                           tdoa_stream_phat_lds(kp), (hipStream_t)stream, sp, kp, out, est, max_Lf, (int)S,
                           tdoa_phat_floor_int16(phat_eps));
        hipError_t e = hipGetLastError();
        return e == hipSuccess ? 0 : tdoa_hip_fail(e, "k_stream_phat_pcm16 launch");
    }
    hipLaunchKernelGGL(k_stream_phat, dim3((unsigned)(grid > 0 ? grid : 1)), dim3(TPB), tdoa_stream_phat_lds(kp),
                       (hipStream_t)stream, sp, kp, out, est, max_Lf, (int)S, tdoa_phat_floor_int16(phat_eps));
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : tdoa_hip_fail(e, "k_stream_phat launch");
}
