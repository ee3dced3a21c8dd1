// tdoa_phat_split.hip -- GCC-PHAT for the shapes whose spectra do not fit one
// workgroup's LDS next to each other (M > 3 or N > 2048: BASELINE configs 3
// and 4).  Same definition as the fused kernels (oracle/gcc_phat_oracle.py),
// split in two passes over chunks of frames:
//
//   k_phat_spectra  one workgroup per (frame, mic) row: the integer front end
//                   (rolling_buffer.c:64-66, buffer.c:13-16, buffer.c:4-11),
//                   complex FFT_N of z[n] = x[2n] + i x[2n+1] in LDS and the
//                   split to X[0..N] of the real FFT_2N, stored N complex per
//                   row (slot 0 packs the two real bins X[0], X[N]) to a
//                   scratch sized to stay in L2 / MALL between the passes;
//   k_phat_pairs    one workgroup per (frame, pair): PHAT cross spectrum and
//                   inverse pre-twiddle straight from the scratch, inverse
//                   FFT_N in LDS, lags -S..S, first argmax, lag prior
//                   (correlations.c:20-33 semantics on float scores);
//   k_phat_pairs_w  the same with per-bin weights on the cross spectrum: pass 2
//                   of every shape while a context has a weight table
//                   (tdoa_set_bin_weights, band-limited GCC-PHAT);
//   k_phat_gate    sum of squared best lags > 4 (sample_compute.h:124-134).
//
// Samples stay in int16 units; the launcher scales the per-mic floor eps by
// 2^30 to match (|X|^2 here is 2^30 times that of x / 2^15).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <climits>

#include "tdoa_internal.h"
#include "tdoa_phat_lds.h"  // TPB, f2 helpers, fft_inplace, prep_word


namespace {

// ---------------------------------------------------------------- pass 1
__global__ void __launch_bounds__(TPB) k_phat_spectra(tdoa_kparams kp,
                                                      const int16_t *__restrict__ frames,
                                                      int64_t row0, f2 *__restrict__ spec)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    f2 *buf = (f2 *)smem;  // [N]
    __shared__ int red[TPB / 64];
    const int N = kp.N, NW = N / 2, tid = threadIdx.x;
    const int64_t row = row0 + blockIdx.x;
    const uint32_t *x = reinterpret_cast<const uint32_t *>(frames + row * (int64_t)N);
    const uint32_t *win = reinterpret_cast<const uint32_t *>(kp.window);

    int s = 0;
    for (int w = tid; w < NW; w += TPB) {
        const uint32_t v = x[w];
        s += (int)(int16_t)(v & 0xFFFFu) + (int)(int16_t)(v >> 16);
    }
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
    const uint32_t off16 = (uint32_t)(tot >> kp.log2N) & 0xFFFFu;  // floor mean, (int16)
    for (int w = tid; w < N; w += TPB) {
        f2 z = f2{0.0f, 0.0f};
        if (w < NW) {
            const uint32_t p = prep_word(x[w], off16, win[w]);
            z = f2{(float)(int16_t)(p & 0xFFFFu), (float)(int16_t)(p >> 16)};
        }
        buf[w] = z;
    }
    __syncthreads();
    fft_inplace<false>(buf, N, kp.tw);

    // X[k] = (Z[k] + Z*[N-k])/2 - i/2 W_2N^k (Z[k] - Z*[N-k])
    f2 *o = spec + (size_t)blockIdx.x * N;
    for (int k = tid; k <= N / 2; k += TPB) {
        const int kn = (N - k) & (N - 1);
        const f2 a = buf[k], b = buf[kn];
        if (k == 0) {
            o[0] = f2{a.x + a.y, a.x - a.y};  // X[0], X[N]: both real
            continue;
        }
        const f2 w2k = ldtw(kp.tw2, k), w2n = ldtw(kp.tw2, N - k);
        const f2 e = a + conj2(b), d = cmul(w2k, a - conj2(b));
        o[k] = 0.5f * f2{e.x + d.y, e.y - d.x};
        if (k != N / 2) {
            const f2 e2 = b + conj2(a), d2 = cmul(w2n, b - conj2(a));
            o[kn] = 0.5f * f2{e2.x + d2.y, e2.y - d2.x};
        }
    }
}

// ---------------------------------------------------------------- pass 2
__device__ __forceinline__ void load_bins(const f2 *X, int k, int kn, f2 &xk, f2 &xn)
{
    if (k == 0) {
        const f2 s = X[0];
        xk = f2{s.x, 0.0f};
        xn = f2{s.y, 0.0f};
    } else {
        xk = X[k];
        xn = X[kn];
    }
}

__global__ void __launch_bounds__(TPB) k_phat_pairs(tdoa_kparams kp, tdoa_kout out,
                                                    const f2 *__restrict__ spec, int64_t f_begin,
                                                    int64_t nblocks, float e2)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    f2 *buf = (f2 *)smem;                    // [N]
    float *sc = (float *)(buf + kp.N);       // [K]
    const int N = kp.N, P = kp.P, M = kp.M, K = kp.K, S = kp.S, tid = threadIdx.x;
    // XCD-aware order: consecutive dispatch slots go to different XCDs, so give
    // each XCD a contiguous run of (frame, pair) items -- the P pairs of a frame
    // then read its spectra through one L2
    int64_t b = blockIdx.x;
    if ((nblocks & 7) == 0)
        b = (b & 7) * (nblocks >> 3) + (b >> 3);
    const int64_t fl = b / P;
    const int p = (int)(b - fl * P);
    const f2 *Xi = spec + (size_t)(fl * M + kp.pair_i[p]) * N;
    const f2 *Xj = spec + (size_t)(fl * M + kp.pair_j[p]) * N;

    // U = X / sqrt(|X|^2 + e2), R = conj(U_i) U_j;  Y[k] = (R[k] + R*[N-k]) + i (R[k] - R*[N-k]) conj(W_2N^k)
    for (int k = tid; k <= N / 2; k += TPB) {
        const int kn = (N - k) & (N - 1);
        f2 ik, in, jk, jn;
        load_bins(Xi, k, kn, ik, in);
        load_bins(Xj, k, kn, jk, jn);
        ik *= __builtin_amdgcn_rsqf(ik.x * ik.x + ik.y * ik.y + e2);
        in *= __builtin_amdgcn_rsqf(in.x * in.x + in.y * in.y + e2);
        jk *= __builtin_amdgcn_rsqf(jk.x * jk.x + jk.y * jk.y + e2);
        jn *= __builtin_amdgcn_rsqf(jn.x * jn.x + jn.y * jn.y + e2);
        const f2 Rk = cmul(conj2(ik), jk), Rn = cmul(conj2(in), jn);
        const f2 w2k = ldtw(kp.tw2, k), w2n = ldtw(kp.tw2, N - k);
        buf[k] = (Rk + conj2(Rn)) + mul_i(cmul(Rk - conj2(Rn), conj2(w2k)));
        if (k != 0 && k != N / 2)
            buf[kn] = (Rn + conj2(Rk)) + mul_i(cmul(Rn - conj2(Rk), conj2(w2n)));
    }
    __syncthreads();
    fft_inplace<true>(buf, N, kp.tw);

    // r[s] = y / 2N at s mod 2N:  r[2u] = Re y[u], r[2u+1] = Im y[u]
    const float invL = 1.0f / (float)(2 * N);
    for (int i = tid; i < K; i += TPB) {
        const int s = i - S;
        const int m = s < 0 ? s + 2 * N : s;
        const f2 y = buf[m >> 1];
        sc[i] = ((m & 1) ? y.y : y.x) * invL;
    }
    __syncthreads();
    if (tid < 64) {  // K <= 127: two candidates per lane, ascending lag order
        const int lane = tid, k1 = lane, k2 = lane + 64;
        const float v1 = k1 < K ? sc[k1] : -INFINITY, v2 = k2 < K ? sc[k2] : -INFINITY;
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
        bk = bk < 0 ? 0 : (bk >= K ? K - 1 : bk);  // NaN scores: keep the index in range
        const int64_t fg = f_begin + fl;
        const size_t gb = (size_t)(fg * P + p) * K;
        if (k1 < K) {
            const int d = k1 > bk ? k1 - bk : bk - k1;
            if (out.scores_f)
                out.scores_f[gb + k1] = v1;
            if (out.weighted_f)
                out.weighted_f[gb + k1] = v1 * kp.prior[d];
        }
        if (k2 < K) {
            const int d = k2 > bk ? k2 - bk : bk - k2;
            if (out.scores_f)
                out.scores_f[gb + k2] = v2;
            if (out.weighted_f)
                out.weighted_f[gb + k2] = v2 * kp.prior[d];
        }
        if (lane == 0)
            out.lags[fg * P + p] = bk - S;
    }
}

// Band-limited pass 2 (tdoa_set_bin_weights): k_phat_pairs with R[k] scaled by
// kp.bin_w[k] before the Hermitian fold -- bin k by w[k], bin N-k by w[N-k];
// slot 0 of a spectrum row packs bins 0 and N.  Every non-zero weight lies in
// bins [kp.bin_lo, kp.bin_hi], so a wave whose 64 bins k (or N-k) all fall
// outside that range takes them as zero without reading the scratch, and
// writes plain zeros when both sides do: the branches are uniform per wave.
// The block order, the argmax with its NaN clamp and tie rule, the prior and
// the stores are k_phat_pairs' (a copy: that kernel's code stays as measured).
__global__ void __launch_bounds__(TPB) k_phat_pairs_w(tdoa_kparams kp, tdoa_kout out,
                                                      const f2 *__restrict__ spec, int64_t f_begin,
                                                      int64_t nblocks, float e2)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    f2 *buf = (f2 *)smem;                    // [N]
    float *sc = (float *)(buf + kp.N);       // [K]
    const int N = kp.N, P = kp.P, M = kp.M, K = kp.K, S = kp.S, tid = threadIdx.x;
    const int lo = kp.bin_lo, hi = kp.bin_hi;
    int64_t b = blockIdx.x;  // XCD-aware order
    if ((nblocks & 7) == 0)
        b = (b & 7) * (nblocks >> 3) + (b >> 3);
    const int64_t fl = b / P;
    const int p = (int)(b - fl * P);
    const f2 *Xi = spec + (size_t)(fl * M + kp.pair_i[p]) * N;
    const f2 *Xj = spec + (size_t)(fl * M + kp.pair_j[p]) * N;

    for (int k = tid; k <= N / 2; k += TPB) {
        const int kn = (N - k) & (N - 1);
        // this wave's bins: k in [kw, kw + 63], N - k in [N - kw - 63, N - kw]
        const int kw = __builtin_amdgcn_readfirstlane(k - (tid & 63));
        const bool live_k = kw <= hi && kw + 63 >= lo;
        const bool live_n = N - kw - 63 <= hi && N - kw >= lo;
        if (!live_k && !live_n) {
            buf[k] = f2{0.0f, 0.0f};
            buf[kn] = f2{0.0f, 0.0f};
            continue;
        }
        f2 ik = f2{0.0f, 0.0f}, in = ik, jk = ik, jn = ik;
        if (live_k) {
            ik = Xi[k];
            jk = Xj[k];
        }
        if (live_n) {  // kn = 0 at k = 0: slot 0 again
            in = Xi[kn];
            jn = Xj[kn];
        }
        if (k == 0) {  // slot 0 = (X[0], X[N]), both real
            ik = f2{ik.x, 0.0f};
            jk = f2{jk.x, 0.0f};
            in = f2{in.y, 0.0f};
            jn = f2{jn.y, 0.0f};
        }
        ik *= __builtin_amdgcn_rsqf(ik.x * ik.x + ik.y * ik.y + e2);
        in *= __builtin_amdgcn_rsqf(in.x * in.x + in.y * in.y + e2);
        jk *= __builtin_amdgcn_rsqf(jk.x * jk.x + jk.y * jk.y + e2);
        jn *= __builtin_amdgcn_rsqf(jn.x * jn.x + jn.y * jn.y + e2);
        const f2 Rk = kp.bin_w[k] * cmul(conj2(ik), jk), Rn = kp.bin_w[N - k] * cmul(conj2(in), jn);
        const f2 w2k = ldtw(kp.tw2, k), w2n = ldtw(kp.tw2, N - k);
        buf[k] = (Rk + conj2(Rn)) + mul_i(cmul(Rk - conj2(Rn), conj2(w2k)));
        if (k != 0 && k != N / 2)
            buf[kn] = (Rn + conj2(Rk)) + mul_i(cmul(Rn - conj2(Rk), conj2(w2n)));
    }
    __syncthreads();
    fft_inplace<true>(buf, N, kp.tw);

    // r[s] = y / 2N at s mod 2N:  r[2u] = Re y[u], r[2u+1] = Im y[u]
    const float invL = 1.0f / (float)(2 * N);
    for (int i = tid; i < K; i += TPB) {
        const int s = i - S;
        const int m = s < 0 ? s + 2 * N : s;
        const f2 y = buf[m >> 1];
        sc[i] = ((m & 1) ? y.y : y.x) * invL;
    }
    __syncthreads();
    if (tid < 64) {  // K <= 127: two candidates per lane, ascending lag order
        const int lane = tid, k1 = lane, k2 = lane + 64;
        const float v1 = k1 < K ? sc[k1] : -INFINITY, v2 = k2 < K ? sc[k2] : -INFINITY;
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
        bk = bk < 0 ? 0 : (bk >= K ? K - 1 : bk);  // NaN scores: keep the index in range
        const int64_t fg = f_begin + fl;
        const size_t gb = (size_t)(fg * P + p) * K;
        if (k1 < K) {
            const int d = k1 > bk ? k1 - bk : bk - k1;
            if (out.scores_f)
                out.scores_f[gb + k1] = v1;
            if (out.weighted_f)
                out.weighted_f[gb + k1] = v1 * kp.prior[d];
        }
        if (k2 < K) {
            const int d = k2 > bk ? k2 - bk : bk - k2;
            if (out.scores_f)
                out.scores_f[gb + k2] = v2;
            if (out.weighted_f)
                out.weighted_f[gb + k2] = v2 * kp.prior[d];
        }
        if (lane == 0)
            out.lags[fg * P + p] = bk - S;
    }
}

__global__ void k_phat_gate(const int32_t *__restrict__ lags, uint8_t *__restrict__ gate, int64_t B,
                            int P)
{
    const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= B)
        return;
    int tot = 0;
    for (int p = 0; p < P; p++) {
        const int b = lags[f * P + p];
        tot += b * b;
    }
    gate[f] = tot > 4 ? 1 : 0;
}

int fail_hip(hipError_t e, const char *what)
{
    char buf[256];
    snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
    return tdoa_set_error(-2, buf);
}

}  // namespace

int64_t tdoa_phat_split_row_bytes(int N) { return (int64_t)N * 8; }

int tdoa_launch_gcc_phat_split(const tdoa_kparams &kp, const tdoa_kout &out,
                               const int16_t *frames, int64_t B, float eps_int16,
                               void *scratch, size_t scratch_bytes, void *stream)
{
    const int N = kp.N, M = kp.M, P = kp.P;
    if (N < 256 || N > 4096 || (N & (N - 1)))
        return tdoa_set_error(-1, "GCC_PHAT: frame_len must be a power of two in [256, 4096]");
    if (kp.K > 127)
        return tdoa_set_error(-1, "GCC_PHAT: max_shift > 63 not supported");
    if (!scratch)
        return tdoa_set_error(-1, "GCC_PHAT: context has no spectrum scratch");
    const size_t per_frame = (size_t)M * N * sizeof(f2);
    const int64_t chunk = (int64_t)(scratch_bytes / per_frame);
    if (chunk < 1)
        return tdoa_set_error(-1, "GCC_PHAT: spectrum scratch smaller than one frame");
    hipStream_t st = (hipStream_t)stream;
    const size_t lds1 = (size_t)N * sizeof(f2);
    const size_t lds2 = (size_t)N * sizeof(f2) + 128 * sizeof(float);
    for (int64_t c0 = 0; c0 < B; c0 += chunk) {
        const int64_t nf = (B - c0) < chunk ? (B - c0) : chunk;
        if (nf * P > INT_MAX)
            return tdoa_set_error(-1, "GCC_PHAT: chunk too large for one launch");
        hipLaunchKernelGGL(k_phat_spectra, dim3((unsigned)(nf * M)), dim3(TPB), lds1, st, kp, frames,
                           c0 * M, (f2 *)scratch);
        if (kp.bin_w)
            hipLaunchKernelGGL(k_phat_pairs_w, dim3((unsigned)(nf * P)), dim3(TPB), lds2, st, kp, out,
                               (const f2 *)scratch, c0, nf * P, eps_int16);
        else
            hipLaunchKernelGGL(k_phat_pairs, dim3((unsigned)(nf * P)), dim3(TPB), lds2, st, kp, out,
                               (const f2 *)scratch, c0, nf * P, eps_int16);
    }
    if (out.gate) {
        const int64_t g = (B + 255) / 256;
        hipLaunchKernelGGL(k_phat_gate, dim3((unsigned)g), dim3(256), 0, st, out.lags, out.gate, B, P);
    }
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : fail_hip(e, "GCC_PHAT split launch");
}
