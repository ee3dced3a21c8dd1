// tdoa_sep.hip -- the null-steering beamformer on the device (include/tdoa.h,
// "Separating"): k_sep<Loader, KT>, one body, over int16 [B][M][L] frames
// (frame_loader) or the capture rings of a streaming pipeline
// (ring_loader<uint8_t | int16_t>), and its launcher.  The steering is
// tdoa_beam_rule.h's, the FFT the LDS Stockham stages of tdoa_phat_lds.h.
//
// One workgroup of 256 threads per row (a frame, a stream), one block of L
// samples.  LDS: 256 bytes of geometry, codes and validity, then
// max(ceil(M/2), ceil(KT/2)) complex buffers of L points:
//   1. the row's M x L samples, times the window, go to LDS two mics to a
//      complex buffer, z_p[n] = g[n] x_{2p}[n] + i g[n] x_{2p+1}[n].  A ring's
//      run is fetched by ring_stage (tdoa_beam_dev.h, shared with k_beam_ring),
//      which says how.
//   2. thread (k, m) of the first wave steers target k to mic m's delay code
//      (beam_steer, in the same header).
//   3. one forward FFT_L per mic pair, in place.
//   4. thread k owns bins k and L - k of every buffer: it splits the pairs'
//      transforms into X_m[k], accumulates b = A^H X and the lower triangle of
//      G = A^H A + delta M I over the mics, solves G y = b by Cholesky in
//      registers (KT x KT, in double, an invalid target a zero column), and writes
//      Y_{2q} + i Y_{2q+1} (Hermitian-extended) for every target pair q over
//      the slots it has just read: no other thread touches them.
//   5. one inverse FFT_L per target pair; y_j[n] = g[n] Re / Im z_q[n] / L.  The
//      block form stores y_j; the ring form adds its first half to the saved
//      tail (one coalesced read), stores that as the hop's audio and the second
//      half as the new tail (one coalesced write).
// Every per-thread array is indexed by unrolled constants: no private segment.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tdoa_beam_dev.h"
#include "tdoa_internal.h"
#include "tdoa_phat_lds.h"
#include "tdoa_sep_rule.h"

namespace {

constexpr int SEP_HEAD_BYTES = 256;  // geometry (80), codes [4][8] (128), validity [4] (16), padded

static_assert(sizeof(tdoa_beam_geometry) + TDOA_SEP_MAX_TARGETS * (TDOA_MAX_MICS + 1) * 4 <= SEP_HEAD_BYTES,
              "k_sep's LDS head");

struct sep_kargs {
    tdoa_beam_geometry g;
    tdoa_beam_source in;    // ring: T [rows][capture_len][M]; block: int16 [rows][M][L]
    tdoa_beam_targets tg;
    const float *tab;       // window [L], twiddles [2 L]
    float *tail;            // ring: [rows][TDOA_SEP_MAX_TARGETS][L/2]
    tdoa_beam_outputs out;  // audio: ring [rows][Kt][L/2], block [rows][Kt][L]; delays, active, block_start
    float loading;
    int32_t Dmax, L;
};

// where sample l of mic m is staged: mic pair m / 2's buffer, real or imaginary part
__device__ __forceinline__ void stage_put(float *zf, int L, int M, int m, int l, float v)
{
    const int at = (((m >> 1) * L + l) << 1) + (m & 1);
    zf[at] = v;
    if ((M & 1) && m == M - 1)
        zf[at + 1] = 0.0f;  // the odd mic's partner
}

struct frame_loader {
    static constexpr bool RING = false;
    // frame sample n of mic m is frames[row][m][n]
    static __device__ __forceinline__ void stage(const sep_kargs &a, float *zf, int64_t row, int64_t, int L, int M)
    {
        const int16_t *fr = static_cast<const int16_t *>(a.in.src) + (size_t)row * M * L;
        for (int i = threadIdx.x; i < M * L; i += TPB) {
            const int m = i / L, l = i - m * L;
            stage_put(zf, L, M, m, l, a.tab[l] * (float)fr[i]);
        }
    }
};

// ring_stage's sample l of mic m, times the window (finite and not negative: a
// zeroed sample stays +0), to its place
struct sep_sink {
    float *zf;
    const float *win;
    int L, M;
    __device__ __attribute__((always_inline)) void operator()(int m, int l, float x) const
    {
        stage_put(zf, L, M, m, l, win[l] * x);
    }
};

template <typename T> struct ring_loader {
    static constexpr bool RING = true;
    static __device__ __forceinline__ void stage(const sep_kargs &a, float *zf, int64_t row, int64_t tl, int L, int M)
    {
        ring_stage<T, TPB>(a.in.src, a.in.capture_len, row, tl, L, M, sep_sink{zf, a.tab, L, M});
    }
};

// e^{i pi x}
__device__ __forceinline__ f2 expipi(float x) { return f2{cospif(x), sinpif(x)}; }

// The per-bin system is accumulated and solved in double: the fp32 inputs (the
// spectra, the steering vectors) are exact in it, and the factorisation's
// cancellation -- a pivot of G is delta M after (1 + delta) M minus nearly as
// much, 1 / delta times the rounding error of either -- stays below the error
// the fp32 FFTs leave.  A few hundred fp64 operations per bin, beside 2 M KT
// sine / cosine pairs.
typedef double d2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ d2 dmul(d2 a, d2 b) { return d2{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
__device__ __forceinline__ d2 dconj(d2 a) { return d2{a.x, -a.y}; }
__device__ __forceinline__ d2 to_d2(f2 a) { return d2{(double)a.x, (double)a.y}; }

// G y = b for the KT x KT Hermitian positive definite G, given by its real
// diagonal gd and its lower triangle go[i][j], j < i: Cholesky G = C C^H, then
// C z = b and C^H y = z.  y replaces b.
template <int KT> __device__ __forceinline__ void sep_solve(const double (&gd)[KT], const d2 (&go)[KT][KT], d2 (&b)[KT])
{
    d2 c[KT][KT];
    double ci[KT];  // 1 / C[j][j]
#pragma unroll
    for (int j = 0; j < KT; j++) {
        double d = gd[j];
#pragma unroll
        for (int k = 0; k < j; k++)
            d -= c[j][k].x * c[j][k].x + c[j][k].y * c[j][k].y;
        ci[j] = 1.0 / __builtin_sqrt(d);
#pragma unroll
        for (int i = j + 1; i < KT; i++) {
            d2 s = go[i][j];
#pragma unroll
            for (int k = 0; k < j; k++)
                s -= dmul(c[i][k], dconj(c[j][k]));
            c[i][j] = s * ci[j];
        }
    }
#pragma unroll
    for (int i = 0; i < KT; i++) {
        d2 s = b[i];
#pragma unroll
        for (int k = 0; k < i; k++)
            s -= dmul(c[i][k], b[k]);
        b[i] = s * ci[i];
    }
#pragma unroll
    for (int i = KT - 1; i >= 0; i--) {
        d2 s = b[i];
#pragma unroll
        for (int k = i + 1; k < KT; k++)
            s -= dmul(dconj(c[k][i]), b[k]);
        b[i] = s * ci[i];
    }
}

template <typename Loader, int KT> __global__ void __launch_bounds__(TPB) k_sep(sep_kargs a)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    tdoa_beam_geometry &sg = *reinterpret_cast<tdoa_beam_geometry *>(smem);
    int32_t(*s_code)[TDOA_MAX_MICS] = reinterpret_cast<int32_t(*)[TDOA_MAX_MICS]>(smem + sizeof(tdoa_beam_geometry));
    int32_t *s_valid = reinterpret_cast<int32_t *>(smem + sizeof(tdoa_beam_geometry) +
                                                   TDOA_SEP_MAX_TARGETS * TDOA_MAX_MICS * 4);
    f2 *zb = reinterpret_cast<f2 *>(smem + SEP_HEAD_BYTES);
    const int tid = threadIdx.x, M = a.g.num_mics, L = a.L, Dmax = a.Dmax, hop = L >> 1;
    const float *win = a.tab, *tw = a.tab + L;
    const int64_t row = blockIdx.x;

    beam_geometry_to_lds(&sg, a.g);
    // step 1
    int64_t tl = 0;
    if constexpr (Loader::RING) {
        tl = *a.in.pos - L;  // the position after the last step, less the block
        if (row == 0 && tid == 0 && a.out.block_start)
            *a.out.block_start = tl;
    }
    Loader::stage(a, reinterpret_cast<float *>(zb), row, tl, L, M);
    __syncthreads();

    // step 2 (the FFT's barriers publish it)
    beam_steer(a.tg, sg, Dmax, row, KT, M, s_code, s_valid, a.out.delays, a.out.active);

    // step 3
    const int NP = (M + 1) >> 1;
    for (int p = 0; p < NP; p++)
        fft_inplace<false>(zb + p * L, L, tw);

    // step 4
    const double dM = (double)a.loading * (double)M, scale = 1.0 + (double)a.loading;
    const float inv_ph = -1.0f / (float)(16 * L);  // pi x = -2 pi p / (32 L)
    const int pmask = 32 * L - 1;
    for (int k = tid; k <= hop; k += TPB) {
        const int kn = (L - k) & (L - 1);
        double gd[KT];
        d2 go[KT][KT], b[KT];
        int ok[KT];
#pragma unroll
        for (int j = 0; j < KT; j++) {
            ok[j] = s_valid[j];
            gd[j] = (ok[j] ? (double)M : 0.0) + dM;
            b[j] = d2{0.0, 0.0};
#pragma unroll
            for (int i = 0; i < KT; i++)
                go[j][i] = d2{0.0, 0.0};
        }
        for (int p = 0; p < NP; p++) {
            const f2 za = zb[p * L + k], zn = conj2(zb[p * L + kn]);
            const f2 e = za + zn, d = za - zn;
            const f2 x0 = 0.5f * e, x1 = 0.5f * mul_mi(d);
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const int m = 2 * p + h;
                if (m < M) {
                    const d2 x = to_d2(h ? x1 : x0);
                    d2 s[KT];
#pragma unroll
                    for (int j = 0; j < KT; j++) {
                        const int ph = (k * s_code[j][m]) & pmask;  // 32 L is a power of two
                        s[j] = ok[j] ? to_d2(expipi((float)ph * inv_ph)) : d2{0.0, 0.0};
                        b[j] += dmul(dconj(s[j]), x);
#pragma unroll
                        for (int i = 0; i < j; i++)
                            go[j][i] += dmul(dconj(s[j]), s[i]);
                    }
                }
            }
        }
        sep_solve<KT>(gd, go, b);
        const bool real_bin = k == 0 || k == hop;
        f2 y[KT];
#pragma unroll
        for (int j = 0; j < KT; j++) {
            y[j] = ok[j] ? f2{(float)(scale * b[j].x), (float)(scale * b[j].y)} : f2{0.0f, 0.0f};
            if (real_bin)
                y[j].y = 0.0f;
        }
#pragma unroll
        for (int q = 0; q < (KT + 1) / 2; q++) {
            const f2 ya = y[2 * q], yb = 2 * q + 1 < KT ? y[2 * q + 1] : f2{0.0f, 0.0f};
            zb[q * L + k] = f2{ya.x - yb.y, ya.y + yb.x};
            zb[q * L + kn] = f2{ya.x + yb.y, yb.x - ya.y};  // conj(ya) + i conj(yb)
        }
    }
    __syncthreads();

    // step 5
    for (int q = 0; q < (KT + 1) / 2; q++)
        fft_inplace<true>(zb + q * L, L, tw);
    const float invL = 1.0f / (float)L;
    if constexpr (Loader::RING) {
        for (int i = tid; i < KT * hop; i += TPB) {
            const int j = i / hop, n = i - j * hop;
            const f2 lo = zb[(j >> 1) * L + n], hi = zb[(j >> 1) * L + n + hop];
            const bool on = s_valid[j] != 0;
            const float y0 = on ? win[n] * (((j & 1) ? lo.y : lo.x) * invL) : 0.0f;
            const float y1 = on ? win[n + hop] * (((j & 1) ? hi.y : hi.x) * invL) : 0.0f;
            float *t = a.tail + ((size_t)row * TDOA_SEP_MAX_TARGETS + j) * hop + n;
            a.out.audio[((size_t)row * KT + j) * hop + n] = *t + y0;
            *t = y1;
        }
    } else {
        for (int i = tid; i < KT * L; i += TPB) {
            const int j = i / L, n = i - j * L;
            const f2 z = zb[(j >> 1) * L + n];
            a.out.audio[((size_t)row * KT + j) * L + n] = s_valid[j] ? win[n] * (((j & 1) ? z.y : z.x) * invL) : 0.0f;
        }
    }
}

template <typename Loader, int KT> int launch(const sep_kargs &a, int64_t rows, size_t lds, hipStream_t st)
{
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_sep<Loader, KT>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess)
            return tdoa_hip_fail(e, "k_sep LDS size");
    }
    hipLaunchKernelGGL((k_sep<Loader, KT>), dim3((unsigned)rows), dim3(TPB), lds, st, a);
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? tdoa_hip_fail(e, "k_sep launch") : 0;
}

template <typename Loader> int launch_kt(const sep_kargs &a, int64_t rows, int Kt, size_t lds, hipStream_t st)
{
    switch (Kt) {
    case 1:
        return launch<Loader, 1>(a, rows, lds, st);
    case 2:
        return launch<Loader, 2>(a, rows, lds, st);
    case 3:
        return launch<Loader, 3>(a, rows, lds, st);
    default:
        return launch<Loader, 4>(a, rows, lds, st);
    }
}

}  // namespace

int tdoa_launch_sep(const tdoa_beam_geometry &g, int Dmax, const tdoa_beam_source &source, int L,
                    const tdoa_beam_targets &targets, float loading, const float *tab, float *tail,
                    const tdoa_beam_outputs &out, void *stream)
{
    const int64_t rows = source.rows;
    const int Kt = targets.Kt;
    if (rows <= 0)
        return 0;
    if (Kt < 1 || Kt > TDOA_SEP_MAX_TARGETS || !tab || (source.pos && !tail))
        return tdoa_set_error(TDOA_ERR_INVALID, "sep: launch arguments");
    const size_t lds = SEP_HEAD_BYTES + tdoa_sep_lds(g.num_mics, L, Kt);
    const sep_kargs a{g, source, targets, tab, tail, out, loading, Dmax, L};
    hipStream_t st = (hipStream_t)stream;
    if (!source.pos)
        return launch_kt<frame_loader>(a, rows, Kt, lds, st);
    return source.pcm16 ? launch_kt<ring_loader<int16_t>>(a, rows, Kt, lds, st)
                        : launch_kt<ring_loader<uint8_t>>(a, rows, Kt, lds, st);
}
