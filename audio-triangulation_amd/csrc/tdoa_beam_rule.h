// tdoa_beam_rule.h -- the beamformer's arithmetic (include/tdoa.h,
// "Listening"), one definition for the gfx950 kernels (tdoa_beam.hip, k_beam
// and k_beam_ring) and the host twin (tdoa_beam_host.cpp, tdoa_beam_host): the
// steering of a target to its per-mic delay codes and the 16-tap sum of one
// mic.  Every float operation of the steering is written on its own and
// contraction is off inside it whatever the TU's flags; the tap sum is one
// fused multiply-add per tap on both sides.  Also what a launch of either
// beamformer (k_sep too, tdoa_sep.hip) reads and steers at, tdoa_beam_source
// and tdoa_beam_targets, and the rule that makes a target valid (beam_target).
// No HIP header: a plain host compiler reads it; the device code the kernels
// share is in tdoa_beam_dev.h.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/tdoa.h"

#if defined(__HIPCC__)
#define TDOA_BEAM_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define TDOA_BEAM_HD inline
#endif

#define TDOA_BEAM_TAPS (2 * TDOA_BEAM_HALF)
// samples a block of n outputs reads of every mic: n + Dmax + 15, from 7 before
// its first output
#define TDOA_BEAM_REACH (TDOA_BEAM_TAPS - 1)

static_assert(sizeof(tdoa_beam_geometry) == 16 + 8 * TDOA_MAX_MICS, "tdoa_beam_geometry layout");

TDOA_BEAM_HD bool beam_finite(float v)
{
    // exponent field not all ones
    union {
        float f;
        uint32_t u;
    } b;
    b.f = v;
    return (b.u & 0x7f800000u) != 0x7f800000u;
}

TDOA_BEAM_HD float beam_hypot3(float x, float y, float z)
{
#pragma clang fp contract(off)
    const float xx = x * x;
    const float yy = y * y;
    const float zz = z * z;
    const float s = xx + yy;
    return __builtin_sqrtf(s + zz);
}

// distance of mic m from the hemisphere point (xs, ys, zs)
TDOA_BEAM_HD float beam_dist(const tdoa_beam_geometry &g, int m, float xs, float ys, float zs)
{
#pragma clang fp contract(off)
    const float dx = xs - g.mic_xy[m][0];
    const float dy = ys - g.mic_xy[m][1];
    return beam_hypot3(zs, dx, dy);
}

// the delay code of mic m for the finite target (u, v)
TDOA_BEAM_HD int32_t beam_code(const tdoa_beam_geometry &g, int32_t Dmax, float u, float v, int m)
{
#pragma clang fp contract(off)
    const float h = g.height_offset;
    const float k = h / beam_hypot3(h, u, v);
    const float xs = u * k;
    const float ys = v * k;
    const float zs = h * k;
    float dmin = beam_dist(g, 0, xs, ys, zs);
    for (int i = 1; i < g.num_mics; i++) {
        const float d = beam_dist(g, i, xs, ys, zs);
        dmin = d < dmin ? d : dmin;
    }
    const float dd = beam_dist(g, m, xs, ys, zs) - dmin;
    const float ts = dd / g.speed_of_sound;
    const float t = ts * (float)g.sample_rate_hz;
    const float t32 = t * 32.0f;
    const float r = __builtin_floorf(t32 + 0.5f);
    const float top = (float)(32 * Dmax);  // exact: Dmax <= 65536
    if (!(r >= 0.0f))
        return 0;  // (a NaN too)
    return r > top ? 32 * Dmax : (int32_t)r;
}

// acc + sum_k h[k] x[k] over the 16 taps of one mic, k ascending: x points at
// x_m[n + D_m - 7], h at h[q_m]
TDOA_BEAM_HD float beam_taps(const float *h, const float *x, float acc)
{
#pragma unroll
    for (int k = 0; k < TDOA_BEAM_TAPS; k++)
        acc = __builtin_fmaf(h[k], x[k], acc);
    return acc;
}

TDOA_BEAM_HD float beam_scale(float acc, int M)
{
#pragma clang fp contract(off)
    const float inv = 1.0f / (float)M;
    return acc * inv;
}

// a launch's input.  A ring launch (pos set) reads T [rows][capture_len][M]
// samples at `src` (T = int16_t for pcm16, else uint8_t) behind the device clock
// *pos; a block launch (pos null) reads int16 [rows][M][n] frames.
struct tdoa_beam_source {
    const void *src;
    bool pcm16;
    int64_t capture_len;  // ring: samples per stream
    const int64_t *pos;   // ring: the device clock (samples consumed)
    int64_t rows;         // streams, frames
};

// a launch's targets: xy [rows][Kt][2] with count [rows] (null: all Kt), or --
// xy null -- slot k of tracks [rows][TDOA_MAX_TRACKS], valid iff its status >=
// min_status
struct tdoa_beam_targets {
    const int32_t *count;
    const float *xy;
    const tdoa_track *tracks;
    int32_t min_status, Kt;
};

// target k (< Kt) of a row: its plane coordinates, and whether it is valid --
// listed (k < count, or the slot's status) and finite
TDOA_BEAM_HD bool beam_target(const tdoa_beam_targets &t, int64_t row, int k, int Kt, float *u, float *v)
{
    bool listed;
    if (t.xy) {
        const float *p = t.xy + (row * Kt + k) * 2;
        *u = p[0];
        *v = p[1];
        listed = k < (t.count ? t.count[row] : Kt);
    } else {
        const tdoa_track *tr = t.tracks + row * TDOA_MAX_TRACKS + k;
        *u = tr->x;
        *v = tr->y;
        listed = tr->status >= t.min_status;
    }
    return listed && beam_finite(*u) && beam_finite(*v);
}

// the launcher of k_beam / k_beam_ring (tdoa_beam.hip): one workgroup per row,
// blocks of n outputs.  fir: the device copy of tdoa_beam_fir's table.
int tdoa_launch_beam(const tdoa_beam_geometry &g, int Dmax, const tdoa_beam_source &source, int n,
                     const tdoa_beam_targets &targets, const float *fir, const tdoa_beam_outputs &out, void *stream);

// a context's geometry, largest delay and device FIR table (tdoa_capi.cpp);
// TDOA_ERR_INVALID with the cause stored for a geometry the beamformer refuses
struct tdoa_ctx;
int tdoa_ctx_beam(const tdoa_ctx *c, const char *fn, tdoa_beam_geometry *g, int *Dmax, const float **fir);

// what the entry points share (tdoa_beam_host.cpp; host only)
int tdoa_beam_dmax(const tdoa_beam_geometry &g, int *Dmax);  // validates g too
size_t tdoa_beam_lds(int M, int n, int Dmax);     // a workgroup's dynamic LDS for blocks of n outputs
// out and audio not null, Kt in 1..Kt_max: how tdoa_beam_check and tdoa_sep_check open
int tdoa_beam_check_outputs(const char *fn, int32_t Kt, int Kt_max, const void *out, const void *audio);
int tdoa_beam_check(const char *fn, const tdoa_beam_geometry &g, int Dmax, int n, int32_t Kt, const void *out,
                    const void *audio, bool device /* the LDS limit applies */);
