// tdoa_beam_host.cpp -- the beamformer on the host (tdoa_beam_host,
// include/tdoa.h, "Listening"), the latency of a geometry and the argument
// checks its entry points share.  The steering and the tap sum are
// tdoa_beam_rule.h's, the functions k_beam and k_beam_ring run; here a frame's
// mics are staged as zero-padded float rows and the targets walked in order.
// No HIP call: a plain host compiler builds this file (with tdoa_tables.cpp for
// the FIR table and the error store).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/tdoa.h"
#include "tdoa_beam_rule.h"
#include "tdoa_shared.h"

int tdoa_beam_dmax(const tdoa_beam_geometry &g, int *Dmax)
{
    const int M = g.num_mics;
    if (M < 2 || M > TDOA_MAX_MICS)
        return tdoa_fail(TDOA_ERR_INVALID, "beam geometry: num_mics %d outside [2,%d]", M, TDOA_MAX_MICS);
    // (the negated comparisons are also true for a NaN)
    if (g.sample_rate_hz <= 0 || !(g.speed_of_sound > 0.0f) || !std::isfinite(g.speed_of_sound) ||
        !(g.height_offset > 0.0f) || !std::isfinite(g.height_offset))
        return tdoa_fail(TDOA_ERR_INVALID, "beam geometry: sample_rate_hz, speed_of_sound and height_offset must be "
                                           "finite and positive");
    double sep = 0.0;
    for (int i = 0; i < M; i++) {
        if (!std::isfinite(g.mic_xy[i][0]) || !std::isfinite(g.mic_xy[i][1]))
            return tdoa_fail(TDOA_ERR_INVALID, "beam geometry: mic %d has a non-finite coordinate", i);
        for (int j = i + 1; j < M; j++) {
            const double dx = (double)g.mic_xy[i][0] - (double)g.mic_xy[j][0];
            const double dy = (double)g.mic_xy[i][1] - (double)g.mic_xy[j][1];
            sep = std::max(sep, std::sqrt(dx * dx + dy * dy));
        }
    }
    const double d = std::ceil(sep * (double)g.sample_rate_hz / (double)g.speed_of_sound) + 1.0;
    if (!(d <= 65536.0))
        return tdoa_fail(TDOA_ERR_INVALID, "beam geometry: the mic separation is %g samples (limit 65535)", d - 1.0);
    *Dmax = (int)d;
    return TDOA_OK;
}

size_t tdoa_beam_lds(int M, int n, int Dmax)
{
    // the staged rows [M][n + Dmax + 15], padded to whole float4s, then the FIR table
    const size_t rows = ((size_t)M * ((size_t)n + Dmax + TDOA_BEAM_REACH) + 3) & ~(size_t)3;
    return (rows + TDOA_BEAM_PHASES * TDOA_BEAM_TAPS) * sizeof(float);
}

int tdoa_beam_check_outputs(const char *fn, int32_t Kt, int Kt_max, const void *out, const void *audio)
{
    if (!out || !audio)
        return tdoa_fail(TDOA_ERR_INVALID, "%s: NULL argument (outputs.audio is required)", fn);
    if (Kt < 1 || Kt > Kt_max)
        return tdoa_fail(TDOA_ERR_INVALID, "%s: Kt %d outside 1..%d", fn, (int)Kt, Kt_max);
    return TDOA_OK;
}

int tdoa_beam_check(const char *fn, const tdoa_beam_geometry &g, int Dmax, int n, int32_t Kt, const void *out,
                    const void *audio, bool device)
{
    if (const int rc = tdoa_beam_check_outputs(fn, Kt, TDOA_BEAM_MAX_TARGETS, out, audio))
        return rc;
    if (n < 1)
        return tdoa_fail(TDOA_ERR_INVALID, "%s: block length %d < 1", fn, n);
    const size_t lds = tdoa_beam_lds(g.num_mics, n, Dmax);
    if (device && lds > 150 * 1024)
        return tdoa_fail(TDOA_ERR_INVALID, "%s: %d mics x (block %d + max delay %d + 15) samples need %zu bytes of "
                                           "LDS per workgroup (limit 150 KiB)", fn, g.num_mics, n, Dmax, lds);
    return TDOA_OK;
}

extern "C" int tdoa_beam_latency_of(const tdoa_beam_geometry *g, int32_t *A, int32_t *Dmax)
{
    if (!g)
        return tdoa_fail(TDOA_ERR_INVALID, "tdoa_beam_latency_of: NULL geometry");
    int d = 0;
    if (const int rc = tdoa_beam_dmax(*g, &d))
        return rc;
    if (A)
        *A = d + TDOA_BEAM_HALF;
    if (Dmax)
        *Dmax = d;
    return TDOA_OK;
}

extern "C" int tdoa_beam_host(const tdoa_beam_geometry *g, int32_t N, const int16_t *frames, int64_t B,
                              const int32_t *count, const float *xy, int32_t Kt, const tdoa_beam_outputs *out)
{
    if (!g || !frames || !xy || !out)
        return tdoa_fail(TDOA_ERR_INVALID, "tdoa_beam_host: NULL argument");
    int Dmax = 0;
    if (const int rc = tdoa_beam_dmax(*g, &Dmax))
        return rc;
    if (const int rc = tdoa_beam_check("tdoa_beam_host", *g, Dmax, N, Kt, out, out->audio, false))
        return rc;
    if (B < 0 || B >= ((int64_t)1 << 31))
        return tdoa_fail(TDOA_ERR_INVALID, "tdoa_beam_host: B %lld outside [0, 2^31)", (long long)B);
    const int M = g->num_mics;
    const tdoa_beam_targets targets{count, xy, nullptr, 0, Kt};
    float fir[TDOA_BEAM_PHASES][TDOA_BEAM_TAPS];
    tdoa_beam_fir(&fir[0][0]);
    // row m: x_m[t] at index t + 7, zero outside [0, N)
    const size_t L = (size_t)N + Dmax + TDOA_BEAM_REACH;
    std::vector<float> xs((size_t)M * L);
    for (int64_t b = 0; b < B; b++) {
        std::fill(xs.begin(), xs.end(), 0.0f);
        for (int m = 0; m < M; m++)
            for (int t = 0; t < N; t++)
                xs[m * L + t + (TDOA_BEAM_HALF - 1)] = (float)frames[((size_t)b * M + m) * N + t];
        for (int k = 0; k < Kt; k++) {
            const size_t row = (size_t)b * Kt + k;
            float u, v;
            const bool valid = beam_target(targets, b, k, Kt, &u, &v);
            int32_t code[TDOA_MAX_MICS];
            for (int m = 0; m < M; m++)
                code[m] = valid ? beam_code(*g, Dmax, u, v, m) : -1;
            if (out->delays)
                std::memcpy(out->delays + row * M, code, (size_t)M * sizeof(int32_t));
            if (out->active)
                out->active[row] = valid ? 1 : 0;
            float *y = out->audio + row * N;
            for (int n = 0; n < N; n++) {
                float acc = 0.0f;
                if (valid) {
                    for (int m = 0; m < M; m++)
                        acc = beam_taps(fir[code[m] & 31], &xs[m * L + n + (code[m] >> 5)], acc);
                    acc = beam_scale(acc, M);
                }
                y[n] = acc;
            }
        }
    }
    return TDOA_OK;
}
