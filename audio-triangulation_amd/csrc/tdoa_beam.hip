// tdoa_beam.hip -- the steered delay-and-sum beamformer on the device
// (include/tdoa.h, "Listening"): k_beam_ring<T> over the capture rings of a
// streaming pipeline (T = uint8_t or int16_t), k_beam over int16 [B][M][N]
// frames, and their launcher.  The arithmetic is tdoa_beam_rule.h's, shared
// with the host twin (tdoa_beam_host.cpp).
//
// One workgroup of 256 threads per row (a stream, a frame), blocks of n outputs
// (the hop, the frame length).  With L = n + Dmax + 15:
//   1. the row's samples [t0 - 7, t0 - 7 + L) of all M mics go to LDS as planar
//      float xs[M][L], t0 the block's first output sample; the FIR table
//      (2 KB) and the geometry follow them.  A ring's run is L M contiguous
//      elements modulo the ring's capture_len M: 16-byte vectors where the
//      address is 16-byte aligned and the vector lies inside the ring (after a
//      partial head vector that brings the run to alignment), element loads
//      for the head, the tail, a vector that straddles the ring's end and --
//      when the wrap changes the alignment, capture_len M sizeof(T) being no
//      multiple of 16 -- everything after the wrap.  Samples before the
//      stream's start are staged as zeros.
//   2. thread (k, m) steers target k to mic m's delay code (8 threads per
//      target, each the whole expression: identical operations, identical bits).
//   3. an item is four consecutive outputs of one target: per mic the phase's 16
//      coefficients (four 16-byte LDS reads) and 19 samples are held in
//      registers for 64 fused multiply-adds; m ascending, then k ascending, as
//      the rule states.  Stores are float4 where n is a multiple of 4.
// No per-thread array is indexed at run time: no private segment.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "tdoa_beam_rule.h"
#include "tdoa_internal.h"

namespace {

constexpr int BEAM_TPB = 256;
constexpr int BEAM_GEO_WORDS = sizeof(tdoa_beam_geometry) / 4;

struct beam_kargs {
    tdoa_beam_geometry g;
    const void *src;           // ring: T [rows][cl][M]; block: int16 [rows][M][n]
    int64_t cl;                // ring: samples per stream
    const int64_t *pos;        // ring: the device clock (samples consumed)
    const int32_t *count;      // [rows], or null: all Kt
    const float *xy;           // [rows][Kt][2], or null:
    const tdoa_track *tracks;  // ... [rows][TDOA_MAX_TRACKS], target k = slot k
    const float *fir;          // [32][16]
    float *audio;              // [rows][Kt][n]
    int32_t *delays;           // [rows][Kt][M]
    uint8_t *active;           // [rows][Kt]
    int64_t *block_start;      // [1]
    int32_t Dmax, n, Kt, min_status;
};

// element v of a 16-byte vector of T
template <typename T> __device__ __forceinline__ float vec_elem(const uint4 &x, int v)
{
    const uint32_t w[4] = {x.x, x.y, x.z, x.w};
    if constexpr (sizeof(T) == 1)
        return (float)((w[v >> 2] >> (8 * (v & 3))) & 0xFFu);
    else
        return (float)(int16_t)(w[v >> 1] >> (16 * (v & 1)));
}

// step 1 for a ring: run element i (< L M) is sample tl + i / M of mic i % M
template <typename T>
__device__ __forceinline__ void stage_ring(const beam_kargs &a, float *xs, int64_t row, int64_t tl, int L, int M)
{
    constexpr int V = 16 / sizeof(T);
    const int64_t cl = a.cl, R = cl * M;
    const T *ring = static_cast<const T *>(a.src) + (size_t)row * R;
    int64_t j0 = tl % cl;
    if (j0 < 0)
        j0 += cl;  // (rows of samples before the start are read, inside the ring, and zeroed below)
    const int64_t b0 = j0 * M;  // < R; b0 + tot < 2 R: L <= cl
    const int tot = L * M;
    const int nz = tl < 0 ? (tl < -(int64_t)L ? L : (int)-tl) : 0;  // samples before the stream's start
    // vector j covers run elements [head + (j - 1) V, head + j V): j = 0 is the partial head
    const int head = (int)((V - (int)(((uintptr_t)(ring + b0) / sizeof(T)) % V)) % V);
    const int NV = (tot - head + V - 1) / V + 1;
    for (int j = threadIdx.x; j < NV; j += BEAM_TPB) {
        const int i0 = head + (j - 1) * V;
        int64_t r = b0 + i0;
        if (r >= R)
            r -= R;
        const bool whole = i0 >= 0 && i0 + V <= tot && r + V <= R && ((uintptr_t)(ring + r) & 15u) == 0;
        uint4 x = {0u, 0u, 0u, 0u};
        if (whole)
            x = *reinterpret_cast<const uint4 *>(ring + r);
        const int ia = i0 < 0 ? 0 : i0;
        int l = ia / M, m = ia - l * M;
#pragma unroll
        for (int v = 0; v < V; v++) {
            const int i = i0 + v;
            if (i < 0 || i >= tot)
                continue;
            float f;
            if (whole) {
                f = vec_elem<T>(x, v);
            } else {
                int64_t e = b0 + i;  // in [0, 2 R)
                if (e >= R)
                    e -= R;
                f = (float)ring[e];
            }
            xs[m * L + l] = l < nz ? 0.0f : f;
            if (++m == M) {
                m = 0;
                l++;
            }
        }
    }
}

template <typename T, bool RING> __device__ __forceinline__ void beam_block(const beam_kargs &a)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ tdoa_beam_geometry sg;
    __shared__ int32_t s_code[TDOA_BEAM_MAX_TARGETS][TDOA_MAX_MICS];
    __shared__ int32_t s_valid[TDOA_BEAM_MAX_TARGETS];
    const int tid = threadIdx.x, M = a.g.num_mics, n = a.n, Dmax = a.Dmax, Kt = a.Kt;
    const int L = n + Dmax + TDOA_BEAM_REACH;
    float *xs = smem;                              // [M][L]
    float *fir = smem + ((M * L + 3) & ~3);        // [32][16], 16-byte aligned
    const int64_t row = blockIdx.x;

    if (tid < BEAM_GEO_WORDS)
        reinterpret_cast<uint32_t *>(&sg)[tid] = reinterpret_cast<const uint32_t *>(&a.g)[tid];
    for (int i = tid; i < TDOA_BEAM_PHASES * TDOA_BEAM_TAPS; i += BEAM_TPB)
        fir[i] = a.fir[i];
    if constexpr (RING) {
        const int64_t e = *a.pos;                          // the position after the last step
        const int64_t t0 = e - n - (Dmax + TDOA_BEAM_HALF);  // e - hop - A
        if (row == 0 && tid == 0 && a.block_start)
            *a.block_start = t0;
        stage_ring<T>(a, xs, row, t0 - (TDOA_BEAM_HALF - 1), L, M);
    } else {
        // frame sample t at index t + 7 of its mic's row, zeros around the frame
        const int16_t *fr = static_cast<const int16_t *>(a.src) + (size_t)row * M * n;
        for (int i = tid; i < M * L; i += BEAM_TPB) {
            const int m = i / L, t = i - m * L - (TDOA_BEAM_HALF - 1);
            xs[i] = t >= 0 && t < n ? (float)fr[m * n + t] : 0.0f;
        }
    }
    __syncthreads();

    // step 2
    if (tid < Kt * TDOA_MAX_MICS) {
        const int kt = tid >> 3, m = tid & 7;
        const int64_t tg = row * Kt + kt;
        float u, v;
        bool valid;
        if (a.xy) {
            const int cnt = a.count ? a.count[row] : Kt;
            u = a.xy[tg * 2];
            v = a.xy[tg * 2 + 1];
            valid = kt < cnt;
        } else {
            const tdoa_track *tr = a.tracks + row * TDOA_MAX_TRACKS + kt;
            u = tr->x;
            v = tr->y;
            valid = tr->status >= a.min_status;
        }
        valid = valid && beam_finite(u) && beam_finite(v);
        if (m < M) {
            const int32_t code = valid ? beam_code(sg, Dmax, u, v, m) : -1;
            s_code[kt][m] = code;
            if (a.delays)
                a.delays[tg * M + m] = code;
        }
        if (m == 0) {
            s_valid[kt] = valid ? 1 : 0;
            if (a.active)
                a.active[tg] = valid ? 1 : 0;
        }
    }
    __syncthreads();

    // step 3.  With n no multiple of 4 the last item of a target reads up to 3
    // floats past its 19-sample reach -- the next mic's row, or past the last
    // row the padding and the FIR table -- into outputs that are not stored.
    const int G4 = (n + 3) >> 2;
    const bool vec = (n & 3) == 0 && ((uintptr_t)a.audio & 15u) == 0;
    for (int item = tid; item < Kt * G4; item += BEAM_TPB) {
        const int kt = item / G4, n0 = (item - kt * G4) * 4;
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (s_valid[kt]) {
            for (int m = 0; m < M; m++) {
                const int code = s_code[kt][m];
                const float4 *hp = reinterpret_cast<const float4 *>(fir + (code & 31) * TDOA_BEAM_TAPS);
                float h[TDOA_BEAM_TAPS], x[TDOA_BEAM_TAPS + 3];
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const float4 hv = hp[q];
                    h[4 * q] = hv.x;
                    h[4 * q + 1] = hv.y;
                    h[4 * q + 2] = hv.z;
                    h[4 * q + 3] = hv.w;
                }
                const float *xp = xs + m * L + n0 + (code >> 5);
#pragma unroll
                for (int j = 0; j < TDOA_BEAM_TAPS + 3; j++)
                    x[j] = xp[j];
#pragma unroll
                for (int j = 0; j < 4; j++)
                    acc[j] = beam_taps(h, x + j, acc[j]);
            }
#pragma unroll
            for (int j = 0; j < 4; j++)
                acc[j] = beam_scale(acc[j], M);
        }
        float *o = a.audio + ((size_t)row * Kt + kt) * n + n0;
        if (vec) {
            *reinterpret_cast<float4 *>(o) = float4{acc[0], acc[1], acc[2], acc[3]};
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (n0 + j < n)
                    o[j] = acc[j];
        }
    }
}

template <typename T> __global__ void __launch_bounds__(BEAM_TPB) k_beam_ring(beam_kargs a) { beam_block<T, true>(a); }

__global__ void __launch_bounds__(BEAM_TPB) k_beam(beam_kargs a) { beam_block<int16_t, false>(a); }

}  // namespace

int tdoa_launch_beam(const tdoa_beam_geometry &g, int Dmax, const void *src, bool pcm16, int64_t capture_len,
                     const int64_t *pos, int64_t rows, int n, const int32_t *count, const float *xy,
                     const tdoa_track *tracks, int32_t min_status, int32_t Kt, const float *fir,
                     const tdoa_beam_outputs &out, void *stream)
{
    if (rows <= 0)
        return 0;
    const size_t lds = tdoa_beam_lds(g.num_mics, n, Dmax);
    if (lds > 150 * 1024)
        return tdoa_set_error(TDOA_ERR_INVALID, "beam: the staged block exceeds the LDS budget");
    beam_kargs a{};
    a.g = g;
    a.src = src;
    a.cl = capture_len;
    a.pos = pos;
    a.count = count;
    a.xy = xy;
    a.tracks = tracks;
    a.fir = fir;
    a.audio = out.audio;
    a.delays = out.delays;
    a.active = out.active;
    a.block_start = pos ? out.block_start : nullptr;
    a.Dmax = Dmax;
    a.n = n;
    a.Kt = Kt;
    a.min_status = min_status;
    const dim3 grid((unsigned)rows), block(BEAM_TPB);
    hipStream_t st = (hipStream_t)stream;
    if (!pos)
        hipLaunchKernelGGL(k_beam, grid, block, lds, st, a);
    else if (pcm16)
        hipLaunchKernelGGL(k_beam_ring<int16_t>, grid, block, lds, st, a);
    else
        hipLaunchKernelGGL(k_beam_ring<uint8_t>, grid, block, lds, st, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return tdoa_hip_fail(e, pos ? "k_beam_ring launch" : "k_beam launch");
    return 0;
}
