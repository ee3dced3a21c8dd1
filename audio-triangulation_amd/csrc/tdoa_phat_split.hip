// tdoa_phat_split.hip -- GCC-PHAT for the shapes whose spectra do not fit one
// workgroup's LDS next to each other (M > 3 or N > 2048: BASELINE configs 3
// and 4).  Same definition as the fused kernels (oracle/gcc_phat_oracle.py),
// split in two passes over chunks of frames:
//
//   k_phat_spectra  one workgroup per (frame, mic) row: the integer front end
//                   (rolling_buffer.c:64-66, buffer.c:13-16, buffer.c:4-11;
//                   k_phat_spectra_pcm16: the 16-bit one, TDOA_SAMPLES_PCM16),
//                   complex FFT_N of z[n] = x[2n] + i x[2n+1] in LDS and the
//                   split to X[0..N] of the real FFT_2N, stored N complex per
//                   row (slot 0 packs the two real bins X[0], X[N]) to a
//                   scratch sized to stay in L2 / MALL between the passes;
//   k_phat_pairs<BAND>  one workgroup per (frame, pair): PHAT cross spectrum
//                   and inverse pre-twiddle straight from the scratch, inverse
//                   FFT_N in LDS, lags -S..S, first argmax, lag prior
//                   (correlations.c:20-33 semantics on float scores); <true>
//                   with per-bin weights on the cross spectrum: pass 2 of every
//                   shape while a context has a weight table
//                   (tdoa_set_bin_weights, band-limited GCC-PHAT);
//   k_phat_gate    sum of squared best lags > 4 (sample_compute.h:124-134).
//
// Samples stay in int16 units; the launcher scales the per-mic floor eps by
// 2^30 to match (|X|^2 here is 2^30 times that of x / 2^15).  Every stage is
// a function of tdoa_phat_lds.h, shared with the streaming kernel.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <climits>

#include "tdoa_internal.h"
#include "tdoa_phat_lds.h"

namespace {

// ---------------------------------------------------------------- pass 1
// one definition for both sample formats: k_phat_spectra (8-bit ADC front end)
// and k_phat_spectra_pcm16 (TDOA_SAMPLES_PCM16) differ in phat_front_end alone
#define PHAT_SPECTRA_KERNEL(NAME, PCM16)                                                                      \
    __global__ void __launch_bounds__(TPB) NAME(tdoa_kparams kp, const int16_t *__restrict__ frames,         \
                                                int64_t row0, f2 *__restrict__ spec)                          \
    {                                                                                                         \
        extern __shared__ __attribute__((aligned(16))) char smem[];                                           \
        f2 *buf = (f2 *)smem; /* [N] */                                                                       \
        __shared__ int red[TPB / 64];                                                                         \
        const int N = kp.N;                                                                                   \
        const int64_t row = row0 + blockIdx.x;                                                                \
        phat_front_end<PCM16>(reinterpret_cast<const uint32_t *>(frames + row * (int64_t)N),                  \
                              reinterpret_cast<const uint32_t *>(kp.window), N, kp.log2N, red, buf);          \
        fft_inplace<false>(buf, N, kp.tw);                                                                    \
        phat_split<false>(buf, spec + (size_t)blockIdx.x * N, N, kp.tw2, 0.0f);                               \
    }
PHAT_SPECTRA_KERNEL(k_phat_spectra, false)
PHAT_SPECTRA_KERNEL(k_phat_spectra_pcm16, true)
#undef PHAT_SPECTRA_KERNEL

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

// U = X / sqrt(|X|^2 + e2) on bins k and N-k of both mics of a pair
__device__ __forceinline__ void phat_unit4(f2 &ik, f2 &in, f2 &jk, f2 &jn, float e2)
{
    ik = phat_bin<true>(ik, e2);
    in = phat_bin<true>(in, e2);
    jk = phat_bin<true>(jk, e2);
    jn = phat_bin<true>(jn, e2);
}

// BAND (tdoa_set_bin_weights): R[k] is scaled by kp.bin_w[k] before the
// Hermitian fold -- bin k by w[k], bin N-k by w[N-k].  Every non-zero weight
// lies in bins [kp.bin_lo, kp.bin_hi], so a wave whose 64 bins k (or N-k) all
// fall outside that range takes them as zero without reading the scratch, and
// writes plain zeros when both sides do: the branches are uniform per wave.
// The flag selects the loads and the weights; each side of it runs to its own
// phat_fold call (joined before the fold, the band kernel's loop compiled to 21
// more instructions, nine s_waitcnt among them).
template <bool BAND>
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

    // U = X / sqrt(|X|^2 + e2), R = conj(U_i) U_j
    for (int k = tid; k <= N / 2; k += TPB) {
        const int kn = (N - k) & (N - 1);
        f2 ik, in, jk, jn;
        if (BAND) {
            // this wave's bins: k in [kw, kw + 63], N - k in [N - kw - 63, N - kw]
            const int kw = __builtin_amdgcn_readfirstlane(k - (tid & 63));
            const bool live_k = kw <= kp.bin_hi && kw + 63 >= kp.bin_lo;
            const bool live_n = N - kw - 63 <= kp.bin_hi && N - kw >= kp.bin_lo;
            if (!live_k && !live_n) {
                buf[k] = f2{0.0f, 0.0f};
                buf[kn] = f2{0.0f, 0.0f};
                continue;
            }
            ik = in = jk = jn = f2{0.0f, 0.0f};
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
            phat_unit4(ik, in, jk, jn, e2);
            const f2 Rk = kp.bin_w[k] * cmul(conj2(ik), jk), Rn = kp.bin_w[N - k] * cmul(conj2(in), jn);
            phat_fold(buf, N, k, Rk, Rn, kp.tw2);
        } else {
            load_bins(Xi, k, kn, ik, in);
            load_bins(Xj, k, kn, jk, jn);
            phat_unit4(ik, in, jk, jn, e2);
            const f2 Rk = cmul(conj2(ik), jk), Rn = cmul(conj2(in), jn);
            phat_fold(buf, N, k, Rk, Rn, kp.tw2);
        }
    }
    __syncthreads();
    fft_inplace<true>(buf, N, kp.tw);
    phat_lags(buf, sc, N, K, S);
    if (tid < 64) {  // K <= 127: two candidates per lane, ascending lag order
        const int lane = tid, k1 = lane, k2 = lane + 64;
        const float v1 = k1 < K ? sc[k1] : -INFINITY, v2 = k2 < K ? sc[k2] : -INFINITY;
        const int bk = wave_first_max(v1, v2, lane, K);
        const int64_t fg = f_begin + fl;
        const size_t gb = (size_t)(fg * P + p) * K;
        if (out.scores_f) {
            if (k1 < K)
                out.scores_f[gb + k1] = v1;
            if (k2 < K)
                out.scores_f[gb + k2] = v2;
        }
        if (out.weighted_f)
            prior_weighted(out.weighted_f + gb, kp.prior, v1, v2, lane, K, bk);
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

}  // namespace

int64_t tdoa_phat_split_row_bytes(int N) { return (int64_t)N * 8; }

int tdoa_launch_gcc_phat_split(const tdoa_kparams &kp, const tdoa_kout &out,
                               const int16_t *frames, int64_t B, float eps_int16,
                               void *scratch, size_t scratch_bytes, void *stream)
{
    const int N = kp.N, M = kp.M, P = kp.P;
    if (!tdoa_phat_lds_shape(N, kp.K))
        return tdoa_set_error(-1, tdoa_phat_lds_shape(N, 0) ? "GCC_PHAT: max_shift > 63 not supported"
                                                            : "GCC_PHAT: frame_len must be a power of two in [256, 4096]");
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
        hipLaunchKernelGGL(kp.pcm16 ? k_phat_spectra_pcm16 : k_phat_spectra, dim3((unsigned)(nf * M)), dim3(TPB),
                           lds1, st, kp, frames, c0 * M, (f2 *)scratch);
        if (kp.bin_w)
            hipLaunchKernelGGL(k_phat_pairs<true>, dim3((unsigned)(nf * P)), dim3(TPB), lds2, st, kp, out,
                               (const f2 *)scratch, c0, nf * P, eps_int16);
        else
            hipLaunchKernelGGL(k_phat_pairs<false>, dim3((unsigned)(nf * P)), dim3(TPB), lds2, st, kp, out,
                               (const f2 *)scratch, c0, nf * P, eps_int16);
    }
    if (out.gate) {
        const int64_t g = (B + 255) / 256;
        hipLaunchKernelGGL(k_phat_gate, dim3((unsigned)g), dim3(256), 0, st, out.lags, out.gate, B, P);
    }
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : tdoa_hip_fail(e, "GCC_PHAT split launch");
}
