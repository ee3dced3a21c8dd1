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
    const int P = kp.P, K = kp.K, G = kp.G, GW = kp.grid_W, GH = G / GW, PK = P * K;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nth = blockDim.x;
    const int nwaves = nth >> 6, NS = (G + 31) >> 5;
    T *W = (T *)smem;
    T *Lmap = W + PK;
    T *redv = Lmap + G;
    int *redi = (int *)(redv + nwaves);
    uint32_t *sup = (uint32_t *)(redi + nwaves);
    const int64_t f = blockIdx.x;

    const T *src = scores + f * PK;
    for (int e = tid; e < PK; e += nth)
        W[e] = src[e];
    for (int e = tid; e < NS; e += nth)
        sup[e] = 0u;
    __syncthreads();
    // the L map: LUT bytes from global memory (coalesced over c), scores gathered
    // from LDS; one add per pair in ascending p, no reassociation
    for (int c = tid; c < G; c += nth) {
        T L = 0;
        for (int p = 0; p < P; p++) {
            int k = kp.lut[(size_t)p * G + c];
            k = k < K ? k : K - 1;  // the context's LUT never exceeds it
            L += W[p * K + k];
        }
        Lmap[c] = L;
    }
    __syncthreads();

    int count = 0;
    int my_cell = -1;         // thread k keeps peak k
    T my_val = lowest_t<T>();
    T v0 = lowest_t<T>();
    for (int k = 0; k < Kp; k++) {
        T bv = lowest_t<T>();
        int bu = INT_MAX;
        // increasing c per thread: strict '>' keeps the first; the first
        // unsuppressed cell is taken whatever its value.  PEAKS_SCAN cells'
        // reads (clamped, so unconditional) are issued before the first compare:
        // one cell at a time waited for the bit, then for the value.
        for (int c0 = tid; c0 < G; c0 += PEAKS_SCAN * nth) {
            T v[PEAKS_SCAN];
            uint32_t s[PEAKS_SCAN];
#pragma unroll
            for (int i = 0; i < PEAKS_SCAN; i++) {
                const int c = c0 + i * nth, cc = c < G ? c : G - 1;
                v[i] = Lmap[cc];
                s[i] = sup[cc >> 5];
            }
#pragma unroll
            for (int i = 0; i < PEAKS_SCAN; i++) {
                const int c = c0 + i * nth;
                const bool here = c < G && !((s[i] >> (c & 31)) & 1u);
                if (here && (v[i] > bv || bu == INT_MAX)) {
                    bv = v[i];
                    bu = c;
                }
            }
        }
        for (int m = 32; m >= 1; m >>= 1)
            better_t(bv, bu, __shfl_xor(bv, m, 64), __shfl_xor(bu, m, 64));
        if (lane == 0) {
            redv[wave] = bv;
            redi[wave] = bu;
        }
        __syncthreads();
        bv = redv[0];
        bu = redi[0];
        for (int w = 1; w < nwaves; w++)
            better_t(bv, bu, redv[w], redi[w]);
        // every thread holds the same (bv, bu): the decisions below are uniform
        if (bu < 0 || bu >= G)  // no cell remains
            break;
        if (k == 0)
            v0 = bv;
        else if (min_rel > 0.0f && !((double)bv >= (double)min_rel * (double)v0))
            break;
        if (tid == k) {
            my_cell = bu;
            my_val = bv;
        }
        count = k + 1;
        if (k + 1 == Kp)
            break;
        // suppress the peak's square, clipped to the grid
        const int px = bu % GW, py = bu / GW;
        const int x0 = px - radius > 0 ? px - radius : 0;
        const int x1 = px + radius < GW - 1 ? px + radius : GW - 1;
        const int y0 = py - radius > 0 ? py - radius : 0;
        const int y1 = py + radius < GH - 1 ? py + radius : GH - 1;
        const int sw = x1 - x0 + 1, n = sw * (y1 - y0 + 1);
        for (int e = tid; e < n; e += nth) {
            const int dy = e / sw, dx = e - dy * sw;
            const int c = (y0 + dy) * GW + x0 + dx;
            atomicOr(&sup[c >> 5], 1u << (c & 31));
        }
        __syncthreads();  // the bits are set, and redv / redi are free again
    }

    // one thread per slot writes the peak, or the empty slot's fills
    if (tid < Kp) {
        const int64_t i = f * Kp + tid;
        const bool have = tid < count;
        const int cell = have ? my_cell : -1;
        out.cell[i] = cell;
        store_L<T>(out, i, have ? my_val : lowest_t<T>());
        if (out.xy) {
            const int cx = have ? cell % GW : 0, cy = have ? cell / GW : 0;
            out.xy[2 * i] = have ? (float)(cx - kp.half_w) / kp.grid_scale : NAN;
            out.xy[2 * i + 1] = have ? (float)(kp.half_h - cy) / kp.grid_scale : NAN;
        }
        if (out.lags)
            for (int p = 0; p < P; p++)
                out.lags[i * P + p] = have ? (int)kp.lut[(size_t)p * G + cell] - kp.S : 0;
    }
    if (tid == 0 && out.count)
        out.count[f] = count;
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
