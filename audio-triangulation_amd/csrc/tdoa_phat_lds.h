// tdoa_phat_lds.h -- every LDS stage of GCC-PHAT that the two-pass kernels
// (tdoa_phat_split.hip) and the streaming kernel (tdoa_stream_phat.hip) share,
// one definition each, collective over one 256-thread workgroup:
//
//   phat_front_end  DC floor mean, prep_word (or pcm16_sample), z[n] = x[2n] + i x[2n+1] zero
//                   padded into the FFT buffer
//   fft_inplace     the in-place Stockham FFT_N
//   phat_split      real-FFT split to X[0..N] (slot 0 packs X[0], X[N]), raw
//                   or as the PHAT unit spectrum U = X / sqrt(|X|^2 + e2)
//   phat_fold       Hermitian fold and inverse pre-twiddle of bins k, N - k
//   phat_lags       lags -S..S of the inverse, times 1 / 2N
//   wave_first_max  first maximum of a score row, NaN clamp and tie rule
//   prior_weighted  the lag prior on a lane's two candidates
//
// so a streamed frame's scores are the two-pass route's by construction.
// Internal linkage per TU.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <climits>

#include "tdoa_prep.h"  // prep_word, pcm16_sample, sum_word

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

// In-place complex FFT of length n (128 <= n <= 4096, power of two; the
// separator, tdoa_sep.hip, is the caller below 256) held in LDS: Stockham
// radix-4 passes (one radix-2 pass last when log2 n is odd), each pass staged
// through registers so one buffer suffices.  tw = W_n^k, n entries.  Nothing in
// it depends on n >= 256: a thread takes the butterflies j = tid + 256 b < n / 4
// (n / 2 in the radix-2 pass), none at all where tid is past them, and still
// reaches every barrier; the twiddle indices stay below 3 n / 4.  The caller's
// data must be published (a barrier) before the call; it ends with one.
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

// Integer front end of one mic row x (N int16 samples as N/2 packed words, in
// global memory or LDS): floor-mean DC removal (rolling_buffer.c:64-66), << 8
// wrap and Q15 window (buffer.c:13-16, buffer.c:4-11), then z[n] = x[2n] +
// i x[2n+1] into buf[0..N/2) and zeros into buf[N/2..N).  red: [TPB/64] in LDS.
// Ends with a barrier: buf is ready for fft_inplace.
// PCM16 (TDOA_SAMPLES_PCM16, include/tdoa.h): the same DC reduction, then
// y = x - off in int32 without the wrap (|y| <= 65535) and s = (y W) >> 15
// (|y W| < 2^31; |s| <= 65535, exact in fp32) straight to f2 -- no packed int16
// intermediate holds 17 bits.
template <bool PCM16 = false>
__device__ __forceinline__ void phat_front_end(const uint32_t *x, const uint32_t *win, int N, int log2N, int *red,
                                               f2 *buf)
{
    const int NW = N / 2, tid = threadIdx.x;
    int s = 0;
    for (int w = tid; w < NW; w += TPB)
        s += sum_word(x[w]);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1)
        s += __shfl_xor(s, o, 64);
    if ((tid & 63) == 0)
        red[tid >> 6] = s;
    __syncthreads();
    int tot = 0;
#pragma unroll
    for (int w = 0; w < TPB / 64; w++)
        tot += red[w];
    const int off = tot >> log2N;                          // floor mean
    const uint32_t off16 = (uint32_t)off & 0xFFFFu;        // ... as (int16)
    for (int w = tid; w < N; w += TPB) {
        f2 z = f2{0.0f, 0.0f};
        if (w < NW) {
            if constexpr (PCM16) {
                const uint32_t v = x[w], wv = win[w];
                z = f2{(float)pcm16_sample((int16_t)(v & 0xFFFFu), off, (int16_t)(wv & 0xFFFFu)),
                       (float)pcm16_sample((int16_t)(v >> 16), off, (int16_t)(wv >> 16))};
            } else {
                const uint32_t p = prep_word(x[w], off16, win[w]);
                z = f2{(float)(int16_t)(p & 0xFFFFu), (float)(int16_t)(p >> 16)};
            }
        }
        buf[w] = z;
    }
    __syncthreads();
}

// a bin as the split stores it: raw, or divided by sqrt(|X|^2 + e2) (UNIT)
template <bool UNIT>
__device__ __forceinline__ float phat_bin(float x, float e2)
{
    return UNIT ? x * __builtin_amdgcn_rsqf(x * x + e2) : x;
}
template <bool UNIT>
__device__ __forceinline__ f2 phat_bin(f2 x, float e2)
{
    if (UNIT)
        x *= __builtin_amdgcn_rsqf(x.x * x.x + x.y * x.y + e2);
    return x;
}

// Real-FFT split of buf = FFT_N(z) to the 2N-point spectrum of the row:
// X[k] = (Z[k] + Z*[N-k])/2 - i/2 W_2N^k (Z[k] - Z*[N-k]), N complex to o (slot
// 0 packs the two real bins X[0], X[N]).  tw2 = W_2N^k.  No barrier at the end.
template <bool UNIT>
__device__ __forceinline__ void phat_split(const f2 *buf, f2 *o, int N, const float *__restrict__ tw2, float e2)
{
    for (int k = threadIdx.x; k <= N / 2; k += TPB) {
        const int kn = (N - k) & (N - 1);
        const f2 a = buf[k], b = buf[kn];
        if (k == 0) {
            o[0] = f2{phat_bin<UNIT>(a.x + a.y, e2), phat_bin<UNIT>(a.x - a.y, e2)};  // X[0], X[N]: both real
            continue;
        }
        const f2 w2k = ldtw(tw2, k), w2n = ldtw(tw2, N - k);
        const f2 e = a + conj2(b), d = cmul(w2k, a - conj2(b));
        o[k] = phat_bin<UNIT>(0.5f * f2{e.x + d.y, e.y - d.x}, e2);
        if (k != N / 2) {
            const f2 ee = b + conj2(a), dd = cmul(w2n, b - conj2(a));
            o[kn] = phat_bin<UNIT>(0.5f * f2{ee.x + dd.y, ee.y - dd.x}, e2);
        }
    }
}

// Hermitian fold and inverse pre-twiddle of the cross spectrum's bins k and
// N - k (k <= N/2): Y[k] = (R[k] + R*[N-k]) + i (R[k] - R*[N-k]) conj(W_2N^k)
// into buf[k], and its mirror into buf[N-k]
__device__ __forceinline__ void phat_fold(f2 *buf, int N, int k, f2 Rk, f2 Rn, const float *__restrict__ tw2)
{
    const int kn = (N - k) & (N - 1);
    const f2 w2k = ldtw(tw2, k), w2n = ldtw(tw2, N - k);
    buf[k] = (Rk + conj2(Rn)) + mul_i(cmul(Rk - conj2(Rn), conj2(w2k)));
    if (k != 0 && k != N / 2)
        buf[kn] = (Rn + conj2(Rk)) + mul_i(cmul(Rn - conj2(Rk), conj2(w2n)));
}

// Lags -S..S of buf = inverse FFT_N(Y) into sc[0..K): r[s] = y / 2N at s mod
// 2N, r[2u] = Re y[u], r[2u+1] = Im y[u].  Ends with a barrier.
__device__ __forceinline__ void phat_lags(const f2 *buf, float *sc, int N, int K, int S)
{
    const float invL = 1.0f / (float)(2 * N);
    for (int i = threadIdx.x; i < K; i += TPB) {
        const int s = i - S;
        const int m = s < 0 ? s + 2 * N : s;
        const f2 y = buf[m >> 1];
        sc[i] = ((m & 1) ? y.y : y.x) * invL;
    }
    __syncthreads();
}

// first maximum of row[0..K) (K <= 127) over one wave: two candidates per lane
// in ascending order (v1 = row[lane], v2 = row[lane + 64], -inf past K),
// strict '>' keeps the first; the same index in every lane
__device__ __forceinline__ int wave_first_max(float v1, float v2, int lane, int K)
{
    const int k1 = lane, k2 = lane + 64;
    float bv = v1;
    int bk = k1 < K ? k1 : INT_MAX;
    if (k2 < K && (v2 > bv || bk == INT_MAX)) {
        bv = v2;
        bk = k2;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int ok = __shfl_xor(bk, o, 64);
        if (ov > bv || (ov == bv && ok < bk) || (bk == INT_MAX && ok != INT_MAX)) {
            bv = ov;
            bk = ok;
        }
    }
    bk = __shfl(bk, 0, 64);
    return bk < 0 ? 0 : (bk >= K ? K - 1 : bk);  // NaN scores: keep the index in range
}

// the lag prior on a lane's two candidates (correlations.c:20-33 on float
// scores): w[k] = v[k] * prior[|k - bk|] for k = lane, lane + 64 below K
__device__ __forceinline__ void prior_weighted(float *w, const float *__restrict__ prior, float v1, float v2,
                                               int lane, int K, int bk)
{
    const int k1 = lane, k2 = lane + 64;
    if (k1 < K)
        w[k1] = v1 * prior[k1 > bk ? k1 - bk : bk - k1];
    if (k2 < K)
        w[k2] = v2 * prior[k2 > bk ? k2 - bk : bk - k2];
}

}  // namespace
