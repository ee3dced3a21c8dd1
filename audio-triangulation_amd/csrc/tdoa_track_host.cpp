// tdoa_track_host.cpp -- the tracker on the host (tdoa_track_host, include/tdoa.h)
// and the argument checks its three entry points share.  The rule's arithmetic
// is tdoa_track_rule.h's, the functions k_track runs; here the rows are walked
// in order and the 8 x 8 association is a plain scan.  No HIP call: a plain
// host compiler builds this file (with tdoa_tables.cpp for the error store).
#include <cmath>
#include <cstring>

#include "../../include/tdoa.h"
#include "tdoa_shared.h"
#include "tdoa_track_rule.h"

int tdoa_track_check(const char *fn, const tdoa_track_params *prm, const tdoa_track_outputs *out,
                     const void *count, const void *xy, int32_t Kp, int64_t rows)
{
    if (!prm || !out || !count || !xy)
        return tdoa_fail(TDOA_ERR_INVALID, "%s: NULL argument", fn);
    if (!out->tracks && !out->assigned && !out->num_confirmed)
        return tdoa_fail(TDOA_ERR_INVALID, "%s: every output is NULL", fn);
    if (Kp < 1 || Kp > TDOA_MAX_PEAKS)
        return tdoa_fail(TDOA_ERR_INVALID, "%s: Kp %d outside 1..%d", fn, (int)Kp, TDOA_MAX_PEAKS);
    if (rows < 0 || rows >= ((int64_t)1 << 31))
        return tdoa_fail(TDOA_ERR_INVALID, "%s: rows %lld outside [0, 2^31)", fn, (long long)rows);
    if (prm->max_tracks < 1 || prm->max_tracks > TDOA_MAX_TRACKS)
        return tdoa_fail(TDOA_ERR_INVALID, "%s: max_tracks %d outside 1..%d", fn, (int)prm->max_tracks,
                         TDOA_MAX_TRACKS);
    if (prm->confirm_hits < 1)
        return tdoa_fail(TDOA_ERR_INVALID, "%s: confirm_hits %d < 1", fn, (int)prm->confirm_hits);
    if (prm->max_misses < 1)
        return tdoa_fail(TDOA_ERR_INVALID, "%s: max_misses %d < 1", fn, (int)prm->max_misses);
    if (prm->max_coast_us <= 0)
        return tdoa_fail(TDOA_ERR_INVALID, "%s: max_coast_us %lld <= 0", fn, (long long)prm->max_coast_us);
    // (the negated comparisons are also true for a NaN)
    if (!(prm->gate_d2 > 0.0f) || !std::isfinite(prm->gate_d2))
        return tdoa_fail(TDOA_ERR_INVALID, "%s: gate_d2 %g is not a finite value > 0", fn, (double)prm->gate_d2);
    if (!(prm->meas_var > 0.0f) || !std::isfinite(prm->meas_var))
        return tdoa_fail(TDOA_ERR_INVALID, "%s: meas_var %g is not a finite value > 0", fn, (double)prm->meas_var);
    if (!(prm->accel_psd >= 0.0f) || !std::isfinite(prm->accel_psd))
        return tdoa_fail(TDOA_ERR_INVALID, "%s: accel_psd %g is not a finite value >= 0", fn,
                         (double)prm->accel_psd);
    if (!(prm->init_vel_var > 0.0f) || !std::isfinite(prm->init_vel_var))
        return tdoa_fail(TDOA_ERR_INVALID, "%s: init_vel_var %g is not a finite value > 0", fn,
                         (double)prm->init_vel_var);
    return TDOA_OK;
}

namespace {

// one evaluated row (n > 0) on the stream's table; asg[k] gets measurement k's track id
void track_row(tdoa_track *tr, int32_t &next_id, int64_t t, int n, const float *z, const tdoa_track_params &p,
               int32_t *asg)
{
    const int T = p.max_tracks;
    bool valid[TDOA_MAX_PEAKS], m_used[TDOA_MAX_PEAKS] = {};
    for (int k = 0; k < n; k++)
        valid[k] = track_finite(z[2 * k]) && track_finite(z[2 * k + 1]);
    for (int j = 0; j < T; j++)
        if (tr[j].id != 0 && track_coasted(tr[j], t, p.max_coast_us))
            track_free(tr[j]);
    float c[TDOA_MAX_TRACKS][TDOA_MAX_PEAKS], dx[TDOA_MAX_TRACKS][TDOA_MAX_PEAKS], dy[TDOA_MAX_TRACKS][TDOA_MAX_PEAKS],
        s[TDOA_MAX_TRACKS];
    bool elig[TDOA_MAX_TRACKS][TDOA_MAX_PEAKS] = {}, live[TDOA_MAX_TRACKS] = {};
    int got[TDOA_MAX_TRACKS];
    for (int j = 0; j < T; j++) {
        got[j] = -1;
        live[j] = tr[j].id != 0;
        if (!live[j])
            continue;
        track_predict(tr[j], t, p.accel_psd);
        for (int k = 0; k < n; k++) {
            if (!valid[k])
                continue;
            c[j][k] = track_cost(tr[j], z[2 * k], z[2 * k + 1], p.meas_var, dx[j][k], dy[j][k], s[j]);
            elig[j][k] = c[j][k] <= p.gate_d2;
        }
    }
    for (;;) {
        int bj = -1, bk = -1;
        for (int j = 0; j < T; j++) {
            if (!live[j] || got[j] >= 0)
                continue;
            for (int k = 0; k < n; k++)
                if (elig[j][k] && !m_used[k] && (bj < 0 || c[j][k] < c[bj][bk])) {
                    bj = j;
                    bk = k;
                }
        }
        if (bj < 0)
            break;
        got[bj] = bk;
        m_used[bk] = true;
    }
    for (int j = 0; j < T; j++) {
        if (!live[j])
            continue;
        if (got[j] >= 0) {
            const int k = got[j];
            track_update(tr[j], dx[j][k], dy[j][k], s[j], k, t, p.confirm_hits);
            asg[k] = tr[j].id;
        } else {
            track_miss(tr[j], p.max_misses);
        }
    }
    int slot = 0;
    for (int k = 0; k < n; k++) {
        if (!valid[k] || m_used[k])
            continue;
        while (slot < T && tr[slot].id != 0)
            slot++;
        if (slot >= T)
            break;  // no free slot: this and every later measurement is dropped
        track_birth(tr[slot], ++next_id, z[2 * k], z[2 * k + 1], k, t, p);
        asg[k] = tr[slot].id;
    }
}

}  // namespace

extern "C" int tdoa_track_host(tdoa_track *tracks, int32_t *next_id, int64_t rows, const int32_t *stream_of_row,
                               const int64_t *t_us, const int32_t *count, const float *xy, int32_t Kp,
                               const tdoa_track_params *prm, const tdoa_track_outputs *out)
{
    if (!tracks || !next_id || !t_us)
        return tdoa_fail(TDOA_ERR_INVALID, "tdoa_track_host: NULL argument");
    const int rc = tdoa_track_check("tdoa_track_host", prm, out, count, xy, Kp, rows);
    if (rc)
        return rc;
    const tdoa_track_params p = *prm;
    const int T = p.max_tracks;
    for (int64_t i = 0; i < rows; i++) {
        const int64_t s = stream_of_row ? stream_of_row[i] : i;
        tdoa_track *tr = tracks + s * TDOA_MAX_TRACKS;
        const int n = count[i] < 0 ? 0 : (count[i] > Kp ? Kp : count[i]);
        int32_t asg[TDOA_MAX_PEAKS] = {};
        if (n > 0)
            track_row(tr, next_id[s], t_us[i], n, xy + i * Kp * 2, p, asg);
        if (out->tracks)
            std::memcpy(out->tracks + i * T, tr, (size_t)T * sizeof(tdoa_track));
        if (out->assigned)
            std::memcpy(out->assigned + i * Kp, asg, (size_t)Kp * sizeof(int32_t));
        if (out->num_confirmed) {
            int nc = 0;
            for (int j = 0; j < T; j++)
                nc += tr[j].status == 2;
            out->num_confirmed[i] = nc;
        }
    }
    return TDOA_OK;
}
