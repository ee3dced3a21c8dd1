// tdoa_track_rule.h -- the tracker's arithmetic (include/tdoa.h, "Tracking"),
// one definition for the gfx950 kernel (tdoa_track.hip, k_track) and the host
// twin (tdoa_track_host.cpp, tdoa_track_host): the steps of the rule that
// touch one track record.  Every float operation is written on its own and
// contraction is off inside each function whatever the TU's flags, so both
// sides round as the header states.  No HIP header: a plain host compiler
// reads it.
#pragma once

#include <stdint.h>

#include "../../include/tdoa.h"

#if defined(__HIPCC__)
#define TDOA_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define TDOA_HD inline
#endif

static_assert(sizeof(tdoa_track) == 64, "tdoa_track is 64 bytes");
static_assert(sizeof(tdoa_track_params) == 40, "tdoa_track_params layout");

// t - u for times that may be anything: wraps instead of overflowing
TDOA_HD int64_t track_elapsed(int64_t t, int64_t u) { return (int64_t)((uint64_t)t - (uint64_t)u); }

TDOA_HD bool track_finite(float v)
{
    // exponent field not all ones
    union {
        float f;
        uint32_t u;
    } b;
    b.f = v;
    return (b.u & 0x7f800000u) != 0x7f800000u;
}

TDOA_HD void track_free(tdoa_track &tr) { tr = tdoa_track{}; }

// step 1: true if the track coasted out
TDOA_HD bool track_coasted(const tdoa_track &tr, int64_t t, int64_t max_coast_us)
{
    return track_elapsed(t, tr.upd_us) > max_coast_us;
}

// step 2
TDOA_HD void track_predict(tdoa_track &tr, int64_t t, float q)
{
#pragma clang fp contract(off)
    const int64_t el = track_elapsed(t, tr.t_us);
    const float dt = (float)(el > 0 ? el : (int64_t)0) / 1e6f;
    const float mx = tr.vx * dt;
    const float my = tr.vy * dt;
    tr.x = tr.x + mx;
    tr.y = tr.y + my;
    const float a = dt * tr.p11;
    const float p2 = tr.p01 + tr.p01;
    const float c = p2 + a;
    const float d = dt * c;
    const float dt2 = dt * dt;
    const float dt3 = dt2 * dt;
    const float q3 = q * dt3;
    const float q2 = q * dt2;
    const float q1 = q * dt;
    const float e0 = tr.p00 + d;
    const float e1 = tr.p01 + a;
    tr.p00 = e0 + q3 / 3.0f;
    tr.p01 = e1 + q2 * 0.5f;
    tr.p11 = tr.p11 + q1;
    tr.t_us = t;
}

// step 3: the innovation (dx, dy), its variance s, and the cost
TDOA_HD float track_cost(const tdoa_track &tr, float zx, float zy, float r, float &dx, float &dy, float &s)
{
#pragma clang fp contract(off)
    dx = zx - tr.x;
    dy = zy - tr.y;
    s = tr.p00 + r;
    const float xx = dx * dx;
    const float yy = dy * dy;
    const float d2 = xx + yy;
    return d2 / s;
}

// step 5
TDOA_HD void track_update(tdoa_track &tr, float dx, float dy, float s, int32_t k, int64_t t, int32_t confirm_hits)
{
#pragma clang fp contract(off)
    const float k0 = tr.p00 / s;
    const float k1 = tr.p01 / s;
    const float ax = k0 * dx, ay = k0 * dy, bx = k1 * dx, by = k1 * dy;
    tr.x = tr.x + ax;
    tr.y = tr.y + ay;
    tr.vx = tr.vx + bx;
    tr.vy = tr.vy + by;
    const float m11 = k1 * tr.p01, m01 = k0 * tr.p01, m00 = k0 * tr.p00;
    tr.p11 = tr.p11 - m11;
    tr.p01 = tr.p01 - m01;
    tr.p00 = tr.p00 - m00;
    tr.hits += 1;
    tr.misses = 0;
    tr.upd_us = t;
    tr.peak = k;
    if (tr.status == 1 && tr.hits >= confirm_hits)
        tr.status = 2;
}

// step 6
TDOA_HD void track_miss(tdoa_track &tr, int32_t max_misses)
{
    tr.misses += 1;
    tr.peak = -1;
    if (tr.misses >= max_misses)
        track_free(tr);
}

// step 7
TDOA_HD void track_birth(tdoa_track &tr, int32_t id, float zx, float zy, int32_t k, int64_t t,
                         const tdoa_track_params &p)
{
    tr.id = id;
    tr.status = p.confirm_hits <= 1 ? 2 : 1;
    tr.hits = 1;
    tr.misses = 0;
    tr.x = zx;
    tr.y = zy;
    tr.vx = 0.0f;
    tr.vy = 0.0f;
    tr.p00 = p.meas_var;
    tr.p01 = 0.0f;
    tr.p11 = p.init_vel_var;
    tr.peak = k;
    tr.t_us = t;
    tr.upd_us = t;
}

// The argument checks of tdoa_track_batch / tdoa_track_host / tdoa_stream_track
// that need no device (tdoa_track_host.cpp): 0, or TDOA_ERR_INVALID with the
// thread's last error set, `fn` first in the message.
int tdoa_track_check(const char *fn, const tdoa_track_params *prm, const tdoa_track_outputs *out,
                     const void *count, const void *xy, int32_t Kp, int64_t rows);

// k_track (tdoa_track.hip) on `rows` rows, all device pointers.  rows_dev
// (optional): the batch size on the device, clamped to [0, rows] (a streaming
// step's counter slot); a row's time is t_us[row] or, with t_us null,
// (uint64)end[row] * 1000000 / fs.  Asynchronous on `stream` (a hipStream_t).
int tdoa_launch_track(tdoa_track *tracks, int32_t *next_id, int64_t rows, const int32_t *rows_dev,
                      const int32_t *stream_of_row, const int64_t *t_us, const int64_t *end, int32_t fs,
                      const int32_t *count, const float *xy, int32_t Kp, const tdoa_track_params &prm,
                      const tdoa_track_outputs &out, void *stream);
