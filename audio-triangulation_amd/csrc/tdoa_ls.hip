// tdoa_ls.hip -- least-squares refinement of the grid argmax (north-star
// extension a15, absent in the reference; definition in oracle/tdoa_oracle.h):
// one thread per frame, double precision (MI355X FP64 vector is 1/2 the FP32
// rate and this is a few thousand flops per frame).
//   tau_p  = best_p + parabolic vertex of the raw scores around best_p
//   pred_p = (d_j - d_i) fs / c on the LUT's hemisphere geometry
//            (vga_heatmap.h:55-65), (u, v) in grid metres
//   10 Levenberg-Marquardt steps from the argmax cell, clamped to the grid.
// Built with -ffp-contract=off so it rounds like the C oracle.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "tdoa_internal.h"


namespace {

template <typename T>
__device__ __forceinline__ double ls_tau(const T *s, int K, int best)
{
    const int S = K / 2, kb = best + S;
    const bool inside = kb > 0 && kb < K - 1;
    return inside ? ls_tau3((double)s[kb - 1], (double)s[kb], (double)s[kb + 1], best, true)
                  : ls_tau3(0.0, 0.0, 0.0, best, false);
}

// MM: the mic count at compile time, so the per-frame arrays (P sub-sample
// lags, M distances and their derivatives) are registers, not scratch.
// PEAKS (tdoa_peaks): row f is one of per_frame peaks of score frame
// f / per_frame, its lags the peak's lag tuple; an empty slot (cell < 0) gets
// NaN.
template <typename T, int MM, bool PEAKS>
__global__ void __launch_bounds__(128) k_ls(tdoa_kparams kp, const T *__restrict__ scores,
                                            const float *__restrict__ peak3,
                                            const int32_t *__restrict__ lags,
                                            const int32_t *__restrict__ cells,
                                            float *__restrict__ xy_ls, float *__restrict__ rms_out,
                                            int64_t B, int iters, int per_frame)
{
    const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= B)
        return;
    constexpr int M = MM, P = MM * (MM - 1) / 2;
    const int K = kp.K;
    double tau[P];
    if constexpr (PEAKS) {
        if (cells[f] < 0) {
            if (xy_ls) {
                xy_ls[2 * f] = NAN;
                xy_ls[2 * f + 1] = NAN;
            }
            if (rms_out)
                rms_out[f] = NAN;
            return;
        }
        const T *sf = scores + (size_t)(f / per_frame) * P * K;
#pragma unroll
        for (int p = 0; p < P; p++)
            tau[p] = ls_tau(sf + (size_t)p * K, K, lags[f * P + p]);
    } else if (peak3) {
        // the sub-sample lags from the peaks' scores: every lag and peak word
        // loaded before the first use (the branch inside the loop made each
        // pair's loads a round trip of their own)
        int best[P];
        float y[3 * P];
#pragma unroll
        for (int p = 0; p < P; p++)
            best[p] = lags[f * P + p];
#pragma unroll
        for (int e = 0; e < 3 * P; e++)
            y[e] = peak3[(size_t)f * P * 3 + e];
#pragma unroll
        for (int p = 0; p < P; p++) {
            const bool inside = best[p] + K / 2 > 0 && best[p] + K / 2 < K - 1;
            tau[p] = inside ? ls_tau3((double)y[3 * p], (double)y[3 * p + 1], (double)y[3 * p + 2], best[p], true)
                            : ls_tau3(0.0, 0.0, 0.0, best[p], false);
        }
    } else {
#pragma unroll
        for (int p = 0; p < P; p++)  // ... or from the raw scores
            tau[p] = ls_tau(scores + ((size_t)f * P + p) * K, K, lags[f * P + p]);
    }
#include "tdoa_ls_solve.inc"
}

// tdoa_stream_peaks: row f is peak f % per_frame of the step's slot
// f / per_frame, whose score block is est + ids[slot] * P * K; rows of slots
// >= the step's count (read here, clamped as k_stream_peaks clamps it) are
// not written.  An empty slot (cell < 0) gets NaN.
template <typename T, int MM>
__global__ void __launch_bounds__(128) k_ls_stream(tdoa_kparams kp, const T *__restrict__ est,
                                                   const int32_t *__restrict__ ids,
                                                   const int32_t *__restrict__ count, int nstreams,
                                                   const int32_t *__restrict__ lags,
                                                   const int32_t *__restrict__ cells,
                                                   float *__restrict__ xy_ls, float *__restrict__ rms_out,
                                                   int iters, int per_frame)
{
    const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int cnt_raw = *count;
    const int cnt = cnt_raw < 0 ? 0 : (cnt_raw > nstreams ? nstreams : cnt_raw);
    if (f >= (int64_t)cnt * per_frame)
        return;
    constexpr int M = MM, P = MM * (MM - 1) / 2;
    const int K = kp.K;
    if (cells[f] < 0) {
        if (xy_ls) {
            xy_ls[2 * f] = NAN;
            xy_ls[2 * f + 1] = NAN;
        }
        if (rms_out)
            rms_out[f] = NAN;
        return;
    }
    double tau[P];
    const T *sf = est + (size_t)ids[f / per_frame] * P * K;
#pragma unroll
    for (int p = 0; p < P; p++)
        tau[p] = ls_tau(sf + (size_t)p * K, K, lags[f * P + p]);
#include "tdoa_ls_solve.inc"
}

}  // namespace

int tdoa_launch_ls(const tdoa_kparams &kp, const void *scores, bool is_float, const float *peak3,
                   const int32_t *lags, const int32_t *cells, float *xy_ls, float *rms,
                   int64_t B, void *stream, int per_frame)
{
    if (B <= 0)
        return 0;
    const int64_t grid = (B + 127) / 128;
    if (grid > 0x7fffffff)
        return tdoa_set_error(-1, "ls: batch too large for one launch");
    if (!peak3 && !scores)
        return tdoa_set_error(-1, "ls: neither peak scores nor raw scores");
    if (per_frame > 0 && (peak3 || !scores))
        return tdoa_set_error(-1, "ls: per-peak rows read the score block");
    hipStream_t st = (hipStream_t)stream;
    const bool flt = is_float || peak3;
#define TDOA_LS_K(TT, MM, PK)                                                                           \
    hipLaunchKernelGGL((k_ls<TT, MM, PK>), dim3((unsigned)grid), dim3(128), 0, st, kp, (const TT *)scores, \
                       peak3, lags, cells, xy_ls, rms, B, TDOA_LS_ITERS, per_frame)
#define TDOA_LS_M(MM)                                                                                   \
    case MM:                                                                                            \
        if (per_frame > 0 && flt)                                                                       \
            TDOA_LS_K(float, MM, true);                                                                 \
        else if (per_frame > 0)                                                                         \
            TDOA_LS_K(int64_t, MM, true);                                                               \
        else if (flt)                                                                                   \
            TDOA_LS_K(float, MM, false);                                                                \
        else                                                                                            \
            TDOA_LS_K(int64_t, MM, false);                                                              \
        break
    switch (kp.M) {
        TDOA_LS_M(2);
        TDOA_LS_M(3);
        TDOA_LS_M(4);
        TDOA_LS_M(5);
        TDOA_LS_M(6);
        TDOA_LS_M(7);
        TDOA_LS_M(8);
    default:
        return tdoa_set_error(-1, "ls: num_mics outside 2..8");
    }
#undef TDOA_LS_M
#undef TDOA_LS_K
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        char buf[256];
        snprintf(buf, sizeof buf, "k_ls launch: %s", hipGetErrorString(e));
        return tdoa_set_error(-2, buf);
    }
    return 0;
}

int tdoa_launch_ls_stream(const tdoa_kparams &kp, const void *est, bool is_float, const int32_t *ids,
                          const int32_t *count, int64_t S, const int32_t *lags, const int32_t *cells,
                          float *xy_ls, float *rms, int per_frame, void *stream)
{
    if (S <= 0 || per_frame <= 0)
        return 0;
    // one thread per row of every slot the step can list; those past its count return
    const int64_t grid = (S * per_frame + 127) / 128;
    if (S > 0x7fffffff || grid > 0x7fffffff)
        return tdoa_set_error(-1, "ls: too many streams for one launch");
    if (!est || !ids || !count || !lags || !cells)
        return tdoa_set_error(-1, "ls: per-slot rows read the state, the step's list and the peaks");
    hipStream_t st = (hipStream_t)stream;
#define TDOA_LS_S(TT, MM)                                                                              \
    hipLaunchKernelGGL((k_ls_stream<TT, MM>), dim3((unsigned)grid), dim3(128), 0, st, kp, (const TT *)est, \
                       ids, count, (int)S, lags, cells, xy_ls, rms, TDOA_LS_ITERS, per_frame)
#define TDOA_LS_M(MM)                \
    case MM:                         \
        if (is_float)                \
            TDOA_LS_S(float, MM);    \
        else                         \
            TDOA_LS_S(int64_t, MM);  \
        break
    switch (kp.M) {
        TDOA_LS_M(2);
        TDOA_LS_M(3);
        TDOA_LS_M(4);
        TDOA_LS_M(5);
        TDOA_LS_M(6);
        TDOA_LS_M(7);
        TDOA_LS_M(8);
    default:
        return tdoa_set_error(-1, "ls: num_mics outside 2..8");
    }
#undef TDOA_LS_M
#undef TDOA_LS_S
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        char buf[256];
        snprintf(buf, sizeof buf, "k_ls_stream launch: %s", hipGetErrorString(e));
        return tdoa_set_error(-2, buf);
    }
    return 0;
}
