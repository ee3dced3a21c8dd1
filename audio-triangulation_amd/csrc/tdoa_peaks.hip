// tdoa_peaks.hip -- multi-source peak extraction (tdoa_peaks, include/tdoa.h):
// the top-Kp maxima of the likelihood map
//   L(cell) = sum_p score_p[LUT_p(cell)]
// of one [P][K] score block per frame, with a Chebyshev square of `radius`
// cells suppressed around every reported peak (greedy non-maximum
// suppression).  The reference shows the whole map (vga_heatmap.h:110-130) and
// leaves the search for further hot spots to the viewer; this is that search.
//
// One workgroup per frame.  The frame's scores, its L map (in T, pairs added in
// ascending p as k_heatmap adds them) and a suppression bit per cell sit in
// LDS, so every round after the evaluation costs one scan of the LDS map:
//   per-thread strided scan -> wave64 shuffle reduction -> cross-wave through
//   LDS -> every thread folds the per-wave results (all agree on the peak) ->
//   all threads set the bits of the peak's square -> barrier.
// A bit, not the lowest value of T, marks a suppressed cell, so a map that
// holds the lowest value (-inf, INT64_MIN) still counts its cells as present.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <climits>
#include <cmath>
#include <cstdio>

#include "tdoa_internal.h"


namespace {

constexpr int PEAKS_MAX_THREADS = 1024;
constexpr int PEAKS_SCAN = 8;  // cells per thread whose LDS reads are in flight together
constexpr size_t PEAKS_LDS_BUDGET = 150 * 1024;  // k_grid's launcher budget

template <typename T> __device__ __forceinline__ T lowest_t();
template <> __device__ __forceinline__ int64_t lowest_t<int64_t>() { return INT64_MIN; }
template <> __device__ __forceinline__ float lowest_t<float>() { return -INFINITY; }

// (value descending, cell ascending); cell INT_MAX = nothing found yet, which
// loses against any cell of the same value
template <typename T>
__device__ __forceinline__ void better_t(T &bv, int &bu, T ov, int ou)
{
    if (ov > bv || (ov == bv && ou < bu)) {
        bv = ov;
        bu = ou;
    }
}

template <typename T>
__device__ __forceinline__ void store_L(const tdoa_peaks_kout &o, int64_t i, T v);
template <>
__device__ __forceinline__ void store_L<int64_t>(const tdoa_peaks_kout &o, int64_t i, int64_t v)
{
    if (o.L)
        o.L[i] = v;
}
template <>
__device__ __forceinline__ void store_L<float>(const tdoa_peaks_kout &o, int64_t i, float v)
{
    if (o.Lf)
        o.Lf[i] = v;
}

// LDS: W [P][K] T | Lmap [G] T | redv [waves] T | redi [waves] int | sup [ceil(G/32)] u32
template <typename T>
__global__ void __launch_bounds__(PEAKS_MAX_THREADS) k_peaks(tdoa_kparams kp, tdoa_peaks_kout out,
                                                         const T *__restrict__ scores, int Kp,
                                                         int radius, float min_rel)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int64_t f = blockIdx.x;
    const uint8_t *const lut = kp.lut;
#define PEAKS_FRAME_SRC (scores + f * PK)
#include "tdoa_peaks_frame.inc"
#undef PEAKS_FRAME_SRC
}

// tdoa_stream_peaks: the peaks of the EMA map of every frame a streaming step
// listed.  The batch is the step's: `count_dev` is its counter slot (clamped to
// [0, nstreams] as the hop kernels clamp it), ids[slot] the stream of slot
// `slot`, whose score block is est + ids[slot] * P * K; output row = slot.
// Workgroups are persistent over the slots.  A slot whose gate byte is 0 gets
// the empty record without its map being evaluated (gate may be null: every
// slot is evaluated).  The LUT is read from global memory as k_peaks reads it:
// staged once per workgroup in LDS it measured slower at 3 mics float, the one
// shape where it fits beside the map with two workgroups per CU (48.0 vs
// 40.7 ns per frame at num_peaks 4, 20.9 vs 18.9 at 1; DESIGN.md, k_stream_peaks).
template <typename T>
__global__ void __launch_bounds__(PEAKS_MAX_THREADS) k_stream_peaks(
    tdoa_kparams kp, tdoa_peaks_kout out, const T *__restrict__ est, const int32_t *__restrict__ ids,
    const int32_t *__restrict__ count_dev, const uint8_t *__restrict__ gate, int nstreams, int Kp, int radius,
    float min_rel)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int P = kp.P, tid = threadIdx.x;
    const int cnt_raw = *count_dev;
    const int cnt = cnt_raw < 0 ? 0 : (cnt_raw > nstreams ? nstreams : cnt_raw);
    if ((int)blockIdx.x >= cnt)
        return;
    const uint8_t *const lut = kp.lut;
    int s = ids[blockIdx.x];
    for (int slot = blockIdx.x; slot < cnt; slot += gridDim.x) {
        // the next slot's stream now: its load is off the next frame's path to the scores
        const int stream = s, nxt = slot + (int)gridDim.x;
        s = nxt < cnt ? ids[nxt] : 0;
        if (gate && !gate[slot]) {  // the same byte for every thread
            if (tid < Kp) {
                const int64_t i = (int64_t)slot * Kp + tid;
                out.cell[i] = -1;
                store_L<T>(out, i, lowest_t<T>());
                if (out.xy) {
                    out.xy[2 * i] = NAN;
                    out.xy[2 * i + 1] = NAN;
                }
                if (out.lags)
                    for (int p = 0; p < P; p++)
                        out.lags[i * P + p] = 0;
            }
            if (tid == 0 && out.count)
                out.count[slot] = 0;
            continue;
        }
        const int64_t f = slot;
#define PEAKS_FRAME_SRC (est + (int64_t)stream * PK)
#include "tdoa_peaks_frame.inc"
#undef PEAKS_FRAME_SRC
    }
}

template <typename T>
int launch(const tdoa_kparams &kp, const tdoa_peaks_kout &out, const T *scores, int64_t B, int Kp,
           int radius, float min_rel, int threads, size_t lds, hipStream_t st)
{
    hipLaunchKernelGGL(k_peaks<T>, dim3((unsigned)B), dim3(threads), lds, st, kp, out, scores,
                       Kp, radius, min_rel);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        char buf[256];
        snprintf(buf, sizeof buf, "k_peaks launch: %s", hipGetErrorString(e));
        return tdoa_set_error(-2, buf);
    }
    return 0;
}

}  // namespace

size_t tdoa_peaks_lds(const tdoa_kparams &kp, bool is_float)
{
    const size_t sz = is_float ? sizeof(float) : sizeof(int64_t);
    const size_t nw = PEAKS_MAX_THREADS / 64;  // the reduction area of the largest workgroup
    return ((size_t)kp.P * kp.K + (size_t)kp.G) * sz + nw * (sz + sizeof(int)) +
           (((size_t)kp.G + 31) / 32) * sizeof(uint32_t);
}

bool tdoa_peaks_fits(const tdoa_kparams &kp, bool is_float)
{
    return tdoa_peaks_lds(kp, is_float) <= PEAKS_LDS_BUDGET;
}

int tdoa_launch_peaks(const tdoa_kparams &kp, const tdoa_peaks_kout &out, const void *scores,
                      bool is_float, int64_t B, int num_peaks, int radius, float min_rel,
                      void *stream)
{
    if (B <= 0)
        return 0;
    if (B > INT_MAX)
        return tdoa_set_error(-1, "peaks: batch too large for one launch");
    if (!tdoa_peaks_fits(kp, is_float))
        return tdoa_set_error(-1, "peaks: the L map and one frame's scores exceed the LDS budget");
    // a radius past the grid suppresses all of it: clamp so px + radius cannot wrap
    const int span = kp.grid_W > kp.G / kp.grid_W ? kp.grid_W : kp.G / kp.grid_W;
    if (radius > span)
        radius = span;
    const size_t lds = tdoa_peaks_lds(kp, is_float);
    hipStream_t st = (hipStream_t)stream;
    // threads per workgroup, measured at B = 32768, Kp = 4 (k_peaks):
    // where several workgroups share a CU (float, 8 mics: three) 512 threads
    // beat 256 and 1024 (2.31 vs 3.39 and 4.08 ms); where the LDS leaves one
    // workgroup per CU (int64, 8 mics) 1024 beat 512 and 256 (4.80 vs 5.95 and 9.67 ms)
    const int th = lds > 80 * 1024 ? 1024 : 512;
    return is_float ? launch<float>(kp, out, (const float *)scores, B, num_peaks, radius, min_rel, th, lds, st)
                    : launch<int64_t>(kp, out, (const int64_t *)scores, B, num_peaks, radius, min_rel, th, lds, st);
}

namespace {

template <typename T>
void launch_stream(const tdoa_kparams &kp, const tdoa_peaks_kout &out, const T *est, const int32_t *ids,
                   const int32_t *count, const uint8_t *gate, int64_t S, int Kp, int radius, float min_rel,
                   int threads, size_t lds, hipStream_t st)
{
    // as many workgroups as are resident at this LDS, at most one per stream
    const int res = tdoa_resident_blocks((const void *)k_stream_peaks<T>, threads, lds);
    const unsigned grid = (unsigned)(S < res ? S : res);
    hipLaunchKernelGGL(k_stream_peaks<T>, dim3(grid), dim3(threads), lds, st, kp, out, est, ids, count, gate,
                       (int)S, Kp, radius, min_rel);
}

}  // namespace

int tdoa_launch_stream_peaks(const tdoa_kparams &kp, const tdoa_peaks_kout &out, const void *est,
                             bool is_float, const int32_t *ids, const int32_t *count, const uint8_t *gate,
                             int64_t S, int num_peaks, int radius, float min_rel, void *stream)
{
    if (S <= 0)
        return 0;
    if (S > INT_MAX)
        return tdoa_set_error(-1, "stream peaks: too many streams for one launch");
    if (!tdoa_peaks_fits(kp, is_float))
        return tdoa_set_error(-1, "stream peaks: the L map and one frame's scores exceed the LDS budget");
    const int span = kp.grid_W > kp.G / kp.grid_W ? kp.grid_W : kp.G / kp.grid_W;
    if (radius > span)  // as tdoa_launch_peaks
        radius = span;
    const size_t lds = tdoa_peaks_lds(kp, is_float);
    const int th = lds > 80 * 1024 ? 1024 : 512;  // tdoa_launch_peaks' rule
    hipStream_t st = (hipStream_t)stream;
    if (is_float)
        launch_stream<float>(kp, out, (const float *)est, ids, count, gate, S, num_peaks, radius, min_rel, th, lds, st);
    else
        launch_stream<int64_t>(kp, out, (const int64_t *)est, ids, count, gate, S, num_peaks, radius, min_rel, th,
                               lds, st);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        char buf[256];
        snprintf(buf, sizeof buf, "k_stream_peaks launch: %s", hipGetErrorString(e));
        return tdoa_set_error(-2, buf);
    }
    return 0;
}
