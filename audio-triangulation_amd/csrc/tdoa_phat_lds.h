// tdoa_phat_lds.h -- the LDS pieces of GCC-PHAT that the two-pass kernels
// (tdoa_phat_split.hip) and the streaming kernel (tdoa_stream_phat.hip) share:
// the complex helpers, the in-place Stockham FFT of one 256-thread workgroup
// and the integer front end of one packed sample pair.  Internal linkage per TU.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr int TPB = 256;  // threads per workgroup
constexpr int BPT = 4;    // radix-4 butterflies per thread: N/4 <= 1024

typedef float f2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ f2 cmul(f2 a, f2 b)
{
    return f2{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x};
}
__device__ __forceinline__ f2 conj2(f2 a) { return f2{a.x, -a.y}; }
__device__ __forceinline__ f2 mul_i(f2 a) { return f2{-a.y, a.x}; }
__device__ __forceinline__ f2 mul_mi(f2 a) { return f2{a.y, -a.x}; }
__device__ __forceinline__ f2 ldtw(const float *tw, int k) { return f2{tw[2 * k], tw[2 * k + 1]}; }

// In-place complex FFT of length n (256 <= n <= 4096, power of two) held in
// LDS: Stockham radix-4 passes (one radix-2 pass last when log2 n is odd),
// each pass staged through registers so one buffer suffices.  tw = W_n^k.
template <bool INV>
__device__ void fft_inplace(f2 *buf, int n, const float *__restrict__ tw)
{
    const int tid = threadIdx.x, q = n >> 2;
    int Ns = 1;
    for (; Ns * 4 <= n; Ns *= 4) {
        const int tstep = n / (4 * Ns);
        f2 v[BPT][4];
#pragma unroll
        for (int b = 0; b < BPT; b++) {
            const int j = tid + TPB * b;
            if (j < q) {
#pragma unroll
                for (int r = 0; r < 4; r++)
                    v[b][r] = buf[j + r * q];
            }
        }
        __syncthreads();
#pragma unroll
        for (int b = 0; b < BPT; b++) {
            const int j = tid + TPB * b;
            if (j < q) {
                const int k = j & (Ns - 1);
                f2 w1 = ldtw(tw, k * tstep), w2 = ldtw(tw, 2 * k * tstep),
                   w3 = ldtw(tw, 3 * k * tstep);
                if (INV) {
                    w1 = conj2(w1);
                    w2 = conj2(w2);
                    w3 = conj2(w3);
                }
                const f2 x0 = v[b][0], x1 = cmul(v[b][1], w1), x2 = cmul(v[b][2], w2),
                         x3 = cmul(v[b][3], w3);
                const f2 a = x0 + x2, c = x0 - x2, s = x1 + x3;
                const f2 d = INV ? mul_i(x1 - x3) : mul_mi(x1 - x3);
                const int o = (j / Ns) * Ns * 4 + k;
                buf[o] = a + s;
                buf[o + Ns] = c + d;
                buf[o + 2 * Ns] = a - s;
                buf[o + 3 * Ns] = c - d;
            }
        }
        __syncthreads();
    }
    if (Ns < n) {  // radix-2, Ns = n/2: butterflies j < n/2 = 2q
        const int half = n >> 1;
        f2 v[BPT][2];
#pragma unroll
        for (int b = 0; b < BPT; b++) {
            const int j = tid + TPB * b;
            if (j < half) {
                v[b][0] = buf[j];
                v[b][1] = buf[j + half];
            }
        }
        __syncthreads();
#pragma unroll
        for (int b = 0; b < BPT; b++) {
            const int j = tid + TPB * b;
            if (j < half) {
                f2 w = ldtw(tw, j);
                if (INV)
                    w = conj2(w);
                const f2 c = cmul(v[b][1], w);
                buf[j] = v[b][0] + c;
                buf[j + half] = v[b][0] - c;
            }
        }
        __syncthreads();
    }
}

__device__ __forceinline__ uint32_t prep_word(uint32_t v, uint32_t off16, uint32_t wv)
{
    // (int16)(x - off), then <<= 8 keeps the low byte, then (x * W) >> 15
    uint32_t r = 0;
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const uint32_t x = (v >> (16 * h)) & 0xFFFFu;
        const int32_t w = (int32_t)(int16_t)((wv >> (16 * h)) & 0xFFFFu);
        const int32_t z = (int32_t)(int16_t)(uint16_t)((((x - off16) & 0xFFFFu) << 8) & 0xFFFFu);
        r |= ((uint32_t)((z * w) >> 15) & 0xFFFFu) << (16 * h);
    }
    return r;
}

}  // namespace
