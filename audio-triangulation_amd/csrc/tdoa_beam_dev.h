// tdoa_beam_dev.h -- the device code the two beamformers' kernels share
// (tdoa_beam.hip: k_beam, k_beam_ring; tdoa_sep.hip: k_sep): the geometry's
// copy to LDS, the fetch of a block from a capture ring and the steering of the
// targets to their delay codes.  No float arithmetic outside tdoa_beam_rule.h,
// which turns contraction off itself: a TU's -ffp-contract does not reach it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tdoa_beam_rule.h"

// the kernel argument's geometry to LDS (published by the caller's next barrier)
__device__ __forceinline__ void beam_geometry_to_lds(tdoa_beam_geometry *sg, const tdoa_beam_geometry &g)
{
    if (threadIdx.x < sizeof(tdoa_beam_geometry) / 4)
        reinterpret_cast<uint32_t *>(sg)[threadIdx.x] = reinterpret_cast<const uint32_t *>(&g)[threadIdx.x];
}

// element v of a 16-byte vector of T
template <typename T> __device__ __forceinline__ float ring_vec_elem(const uint4 &x, int v)
{
    const uint32_t w[4] = {x.x, x.y, x.z, x.w};
    if constexpr (sizeof(T) == 1)
        return (float)((w[v >> 2] >> (8 * (v & 3))) & 0xFFu);
    else
        return (float)(int16_t)(w[v >> 1] >> (16 * (v & 1)));
}

// The samples [tl, tl + L) of all M mics of stream `row`, from the capture
// rings T [rows][cl][M] at `src`, by a workgroup of NT threads: sink(m, l, x)
// receives sample tl + l of mic m once, as a float.  The run is L M contiguous
// elements modulo the ring's cl M (run element i is sample tl + i / M of mic
// i % M): 16-byte vectors where the address is 16-byte aligned and the vector
// lies inside the ring (after a partial head vector that brings the run to
// alignment), element loads for the head, the tail, a vector that straddles the
// ring's end and -- when the wrap changes the alignment, cl M sizeof(T) being
// no multiple of 16 -- everything after the wrap.  Samples before the stream's
// start are delivered as zeros.  L <= cl.  The sink is a small struct of
// pointers and ints taken by value, its call operator always_inline (DESIGN.md,
// "The stall of the out-of-line lag hook").
template <typename T, int NT, typename Sink>
__device__ __forceinline__ void ring_stage(const void *src, int64_t cl, int64_t row, int64_t tl, int L, int M,
                                           Sink sink)
{
    constexpr int V = 16 / sizeof(T);
    const int64_t R = cl * M;
    const T *ring = static_cast<const T *>(src) + (size_t)row * R;
    int64_t j0 = tl % cl;
    if (j0 < 0)
        j0 += cl;  // (rows of samples before the start are read, inside the ring, and zeroed below)
    const int64_t b0 = j0 * M;  // < R; b0 + tot < 2 R: L <= cl
    const int tot = L * M;
    const int nz = tl < 0 ? (tl < -(int64_t)L ? L : (int)-tl) : 0;  // samples before the stream's start
    // vector j covers run elements [head + (j - 1) V, head + j V): j = 0 is the partial head
    const int head = (int)((V - (int)(((uintptr_t)(ring + b0) / sizeof(T)) % V)) % V);
    const int NV = (tot - head + V - 1) / V + 1;
    for (int j = threadIdx.x; j < NV; j += NT) {
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
                f = ring_vec_elem<T>(x, v);
            } else {
                int64_t e = b0 + i;  // in [0, 2 R)
                if (e >= R)
                    e -= R;
                f = (float)ring[e];
            }
            sink(m, l, l < nz ? 0.0f : f);
            if (++m == M) {
                m = 0;
                l++;
            }
        }
    }
}

// Thread (k, m) = (tid / 8, tid % 8), tid < 8 Kt, steers target k of `row` to
// mic m's delay code (8 threads per target, each the whole expression:
// identical operations, identical bits): s_code [Kt][8] and s_valid [Kt] in
// LDS, delays [rows][Kt][M] and active [rows][Kt] where they are not null.  sg
// is the geometry in LDS; the caller's barriers publish the step.
__device__ __forceinline__ void beam_steer(const tdoa_beam_targets &t, const tdoa_beam_geometry &sg, int Dmax,
                                           int64_t row, int Kt, int M, int32_t (*s_code)[TDOA_MAX_MICS],
                                           int32_t *s_valid, int32_t *delays, uint8_t *active)
{
    const int tid = threadIdx.x;
    if (tid >= Kt * TDOA_MAX_MICS)
        return;
    const int kt = tid >> 3, m = tid & 7;
    const int64_t tg = row * Kt + kt;
    float u, v;
    const bool valid = beam_target(t, row, kt, Kt, &u, &v);
    if (m < M) {
        const int32_t code = valid ? beam_code(sg, Dmax, u, v, m) : -1;
        s_code[kt][m] = code;
        if (delays)
            delays[tg * M + m] = code;
    }
    if (m == 0) {
        s_valid[kt] = valid ? 1 : 0;
        if (active)
            active[tg] = valid ? 1 : 0;
    }
}
