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
//      (2 KB) and the geometry follow them.  A ring's run is fetched by
//      ring_stage (tdoa_beam_dev.h, shared with k_sep), which says how.
//   2. thread (k, m) steers target k to mic m's delay code (beam_steer, in the
//      same header).
//   3. an item is four consecutive outputs of one target: per mic the phase's 16
//      coefficients (four 16-byte LDS reads) and 19 samples are held in
//      registers for 64 fused multiply-adds; m ascending, then k ascending, as
//      the rule states.  Stores are float4 where n is a multiple of 4.
// No per-thread array is indexed at run time: no private segment.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "tdoa_beam_dev.h"
#include "tdoa_internal.h"

namespace {

constexpr int BEAM_TPB = 256;

struct beam_kargs {
    tdoa_beam_geometry g;
    tdoa_beam_source in;    // ring: T [rows][capture_len][M]; block: int16 [rows][M][n]
    tdoa_beam_targets tg;
    const float *fir;       // [32][16]
    tdoa_beam_outputs out;  // audio [rows][Kt][n], delays [rows][Kt][M], active [rows][Kt], block_start [1]
    int32_t Dmax, n;
};

// where ring_stage's sample l of mic m goes: planar xs[M][L]
struct beam_sink {
    float *xs;
    int L;
    __device__ __attribute__((always_inline)) void operator()(int m, int l, float x) const { xs[m * L + l] = x; }
};

template <typename T, bool RING> __device__ __forceinline__ void beam_block(const beam_kargs &a)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ tdoa_beam_geometry sg;
    __shared__ int32_t s_code[TDOA_BEAM_MAX_TARGETS][TDOA_MAX_MICS];
    __shared__ int32_t s_valid[TDOA_BEAM_MAX_TARGETS];
    const int tid = threadIdx.x, M = a.g.num_mics, n = a.n, Dmax = a.Dmax, Kt = a.tg.Kt;
    const int L = n + Dmax + TDOA_BEAM_REACH;
    float *xs = smem;                              // [M][L]
    float *fir = smem + ((M * L + 3) & ~3);        // [32][16], 16-byte aligned
    const int64_t row = blockIdx.x;

    beam_geometry_to_lds(&sg, a.g);
    for (int i = tid; i < TDOA_BEAM_PHASES * TDOA_BEAM_TAPS; i += BEAM_TPB)
        fir[i] = a.fir[i];
    if constexpr (RING) {
        const int64_t e = *a.in.pos;                         // the position after the last step
        const int64_t t0 = e - n - (Dmax + TDOA_BEAM_HALF);  // e - hop - A
        if (row == 0 && tid == 0 && a.out.block_start)
            *a.out.block_start = t0;
        ring_stage<T, BEAM_TPB>(a.in.src, a.in.capture_len, row, t0 - (TDOA_BEAM_HALF - 1), L, M, beam_sink{xs, L});
    } else {
        // frame sample t at index t + 7 of its mic's row, zeros around the frame
        const int16_t *fr = static_cast<const int16_t *>(a.in.src) + (size_t)row * M * n;
        for (int i = tid; i < M * L; i += BEAM_TPB) {
            const int m = i / L, t = i - m * L - (TDOA_BEAM_HALF - 1);
            xs[i] = t >= 0 && t < n ? (float)fr[m * n + t] : 0.0f;
        }
    }
    __syncthreads();

    // step 2
    beam_steer(a.tg, sg, Dmax, row, Kt, M, s_code, s_valid, a.out.delays, a.out.active);
    __syncthreads();

    // step 3.  With n no multiple of 4 the last item of a target reads up to 3
    // floats past its 19-sample reach -- the next mic's row, or past the last
    // row the padding and the FIR table -- into outputs that are not stored.
    const int G4 = (n + 3) >> 2;
    const bool vec = (n & 3) == 0 && ((uintptr_t)a.out.audio & 15u) == 0;
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
        float *o = a.out.audio + ((size_t)row * Kt + kt) * n + n0;
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

int tdoa_launch_beam(const tdoa_beam_geometry &g, int Dmax, const tdoa_beam_source &source, int n,
                     const tdoa_beam_targets &targets, const float *fir, const tdoa_beam_outputs &out, void *stream)
{
    if (source.rows <= 0)
        return 0;
    const size_t lds = tdoa_beam_lds(g.num_mics, n, Dmax);
    if (lds > 150 * 1024)
        return tdoa_set_error(TDOA_ERR_INVALID, "beam: the staged block exceeds the LDS budget");
    const beam_kargs a{g, source, targets, fir, out, Dmax, n};
    const dim3 grid((unsigned)source.rows), block(BEAM_TPB);
    hipStream_t st = (hipStream_t)stream;
    if (!source.pos)
        hipLaunchKernelGGL(k_beam, grid, block, lds, st, a);
    else if (source.pcm16)
        hipLaunchKernelGGL(k_beam_ring<int16_t>, grid, block, lds, st, a);
    else
        hipLaunchKernelGGL(k_beam_ring<uint8_t>, grid, block, lds, st, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return tdoa_hip_fail(e, source.pos ? "k_beam_ring launch" : "k_beam launch");
    return 0;
}
