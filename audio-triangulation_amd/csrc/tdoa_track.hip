// tdoa_track.hip -- the multi-target tracker on the device (include/tdoa.h,
// "Tracking"): k_track, tdoa_track_batch and the launcher tdoa_stream_track
// uses.  The rule's arithmetic is tdoa_track_rule.h's, shared with the host
// twin (tdoa_track_host.cpp).
//
// One wave64 per row, four rows per workgroup.  Lane l = 8 j + k stands for
// the pair (track slot j, measurement k) of the 8 x 8 cost matrix.  The row's
// table moves as 8-byte words, lane l carrying word k of record j (one 64-byte
// access per record, 512 contiguous bytes per wave), through a 512-byte LDS
// tile per wave; from there every lane of group j reads record j whole and the
// eight lanes of a group carry the same track through predict, update, miss
// and birth in registers (identical operations, identical bits).  The greedy
// association is at most 8 rounds of a wave-wide minimum over (c, lane) --
// lane order is (j, k) order, so the lowest lane among equal costs is the
// rule's tie-break -- with the assigned-track and assigned-measurement masks
// in uniform registers.  Births rank the unassigned measurements against the
// free slots by popcounts of the two masks.  No per-thread array is indexed at
// run time: no private segment.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdio>

#include "tdoa_internal.h"
#include "tdoa_track_rule.h"

namespace {

constexpr int TRACK_ROWS = 4;  // waves (rows) per workgroup

struct track_kargs {
    tdoa_track *tracks;             // [S][TDOA_MAX_TRACKS] state
    int32_t *next_id;               // [S]
    const int32_t *rows_dev;        // streaming: the step's counter slot (clamped to [0, rows]); null: rows
    const int32_t *stream_of_row;   // null: row i is stream i
    const int64_t *t_us;            // [rows] row times, or null:
    const int64_t *end;             // ... [rows] samples consumed at the frame's end, t = end * 1e6 / fs
    const int32_t *count;           // [rows]
    const float *xy;                // [rows][Kp][2]
    tdoa_track *o_tracks;           // [rows][T]
    int32_t *o_assigned;            // [rows][Kp]
    int32_t *o_confirmed;           // [rows]
    tdoa_track_params p;
    int32_t rows, Kp, fs;
};

__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

// bit 8 j of a wave ballot -> bit j
__device__ __forceinline__ uint32_t every8th(uint64_t b)
{
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < 8; j++)
        m |= (uint32_t)((b >> (8 * j)) & 1u) << j;
    return m;
}

// index of the r-th set bit of an 8-bit mask (r < popcount)
__device__ __forceinline__ int nth_bit(uint32_t m, int r)
{
    int at = 0;
#pragma unroll
    for (int b = 0; b < 8; b++) {
        const bool set = (m >> b) & 1u;
        if (set && r == 0)
            at = b;
        r -= set ? 1 : 0;
    }
    return at;
}

__global__ void __launch_bounds__(64 * TRACK_ROWS) k_track(track_kargs a)
{
    __shared__ __attribute__((aligned(16))) tdoa_track tile[TRACK_ROWS][TDOA_MAX_TRACKS];
    const int lane = threadIdx.x & 63, wave = uni(threadIdx.x >> 6);
    const int j = lane >> 3, k = lane & 7;
    int rows = a.rows;
    if (a.rows_dev) {
        const int c = *a.rows_dev;
        rows = c < 0 ? 0 : (c > a.rows ? a.rows : c);
    }
    const int64_t row = (int64_t)blockIdx.x * TRACK_ROWS + wave;
    if (row >= rows)
        return;
    const tdoa_track_params p = a.p;
    const int T = p.max_tracks, Kp = a.Kp;
    const int64_t s = a.stream_of_row ? a.stream_of_row[row] : row;
    const int64_t t = a.t_us ? a.t_us[row] : (int64_t)((uint64_t)a.end[row] * 1000000u / (uint64_t)a.fs);
    const int cnt = uni(a.count[row]);
    const int n = cnt < 0 ? 0 : (cnt > Kp ? Kp : cnt);
    const bool used = j < T;  // the slot belongs to the table

    // the table: word k of record j per lane, then record j whole per lane
    uint64_t *const st_w = reinterpret_cast<uint64_t *>(a.tracks + s * TDOA_MAX_TRACKS);
    uint64_t *const tile_w = reinterpret_cast<uint64_t *>(&tile[wave][0]);
    tile_w[lane] = used ? st_w[lane] : 0;
    wave_lds_sync();
    tdoa_track tr = tile[wave][j];
    wave_lds_sync();

    int32_t asg_id = 0;  // of measurement k (the same in every group)
    if (n > 0) {
        float zx = 0.0f, zy = 0.0f;
        if (k < n) {
            const float2 z = *reinterpret_cast<const float2 *>(a.xy + (row * Kp + k) * 2);
            zx = z.x;
            zy = z.y;
        }
        const bool valid = k < n && track_finite(zx) && track_finite(zy);
        // 1, 2
        if (tr.id != 0 && track_coasted(tr, t, p.max_coast_us))
            track_free(tr);
        const bool live = used && tr.id != 0;
        if (live)
            track_predict(tr, t, p.accel_psd);
        // 3
        float dx, dy, sv;
        const float c = track_cost(tr, zx, zy, p.meas_var, dx, dy, sv);
        const bool elig = live && valid && c <= p.gate_d2;
        // 4
        uint32_t tmask = 0, mmask = 0;
        int my_k = -1;  // the measurement of track j
        int my_j = -1;  // the track of measurement k
        for (int round = 0; round < TDOA_MAX_TRACKS; round++) {
            const bool cand = elig && !((tmask >> j) & 1u) && !((mmask >> k) & 1u);
            float bc = cand ? c : 0.0f;
            int bl = cand ? lane : 64;
#pragma unroll
            for (int m = 1; m < 64; m <<= 1) {
                const float oc = __shfl_xor(bc, m);
                const int ol = __shfl_xor(bl, m);
                if (ol < 64 && (bl >= 64 || oc < bc || (oc == bc && ol < bl))) {
                    bc = oc;
                    bl = ol;
                }
            }
            const int w = uni(bl);
            if (w >= 64)
                break;
            const int wj = w >> 3, wk = w & 7;
            tmask |= 1u << wj;
            mmask |= 1u << wk;
            if (j == wj)
                my_k = wk;
            if (k == wk)
                my_j = wj;
        }
        // 5, 6: the innovation of the pair (j, my_k) sits in lane 8 j + my_k
        const int src = my_k >= 0 ? (j << 3) + my_k : lane;
        const float adx = __shfl(dx, src), ady = __shfl(dy, src);
        if (live) {
            if (my_k >= 0)
                track_update(tr, adx, ady, sv, my_k, t, p.confirm_hits);
            else
                track_miss(tr, p.max_misses);
        }
        const int id_j = __shfl(tr.id, (my_j >= 0 ? my_j : 0) << 3);
        if (my_j >= 0)
            asg_id = id_j;
        // 7: the r-th unassigned valid measurement takes the r-th free slot
        const uint32_t fmask = every8th(__ballot(used && tr.id == 0));
        const uint32_t umask = (uint32_t)(__ballot(valid && j == 0) & 0xffu) & ~mmask;
        const int nf = __popc(fmask), nu = __popc(umask);
        const int32_t base = a.next_id[s];
        const int rj = __popc(fmask & ((1u << j) - 1u));
        const bool born = ((fmask >> j) & 1u) && rj < nu;
        const int bk = nth_bit(umask, rj);  // lane bk is (slot 0, measurement bk)
        const float bzx = __shfl(zx, bk), bzy = __shfl(zy, bk);
        if (born)
            track_birth(tr, base + rj + 1, bzx, bzy, bk, t, p);
        const int rk = __popc(umask & ((1u << k) - 1u));
        if (((umask >> k) & 1u) && rk < nf)
            asg_id = base + rk + 1;
        const int births = nu < nf ? nu : nf;
        if (lane == 0 && births > 0)
            a.next_id[s] = base + births;
        // the table back: record j from lane 8 j, then word k of record j per lane
        if (k == 0)
            tile[wave][j] = tr;
        wave_lds_sync();
        if (used)
            st_w[lane] = tile_w[lane];
    }
    // (a row that was not evaluated: the tile still holds the table as loaded)
    if (a.o_tracks && used)
        reinterpret_cast<uint64_t *>(a.o_tracks + row * T)[lane] = tile_w[lane];
    if (a.o_assigned && j == 0 && k < Kp)
        a.o_assigned[row * Kp + k] = asg_id;
    const uint64_t conf = __ballot(used && k == 0 && tr.status == 2);
    if (a.o_confirmed && lane == 0)
        a.o_confirmed[row] = __popcll(conf);
}

}  // namespace

int tdoa_launch_track(tdoa_track *tracks, int32_t *next_id, int64_t rows, const int32_t *rows_dev,
                      const int32_t *stream_of_row, const int64_t *t_us, const int64_t *end, int32_t fs,
                      const int32_t *count, const float *xy, int32_t Kp, const tdoa_track_params &prm,
                      const tdoa_track_outputs &out, void *stream)
{
    if (rows <= 0)
        return 0;
    track_kargs a{};
    a.tracks = tracks;
    a.next_id = next_id;
    a.rows_dev = rows_dev;
    a.stream_of_row = stream_of_row;
    a.t_us = t_us;
    a.end = end;
    a.count = count;
    a.xy = xy;
    a.o_tracks = out.tracks;
    a.o_assigned = out.assigned;
    a.o_confirmed = out.num_confirmed;
    a.p = prm;
    a.rows = (int32_t)rows;
    a.Kp = Kp;
    a.fs = fs;
    const unsigned grid = (unsigned)((rows + TRACK_ROWS - 1) / TRACK_ROWS);
    hipLaunchKernelGGL(k_track, dim3(grid), dim3(64 * TRACK_ROWS), 0, (hipStream_t)stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return tdoa_hip_fail(e, "k_track launch");
    return 0;
}

extern "C" int tdoa_track_batch(int device, tdoa_track *tracks, int32_t *next_id, int64_t rows,
                                const int32_t *stream_of_row, const int64_t *t_us, const int32_t *count,
                                const float *xy, int32_t Kp, const tdoa_track_params *prm,
                                const tdoa_track_outputs *out, void *stream)
{
    if (!tracks || !next_id || !t_us)
        return tdoa_fail(TDOA_ERR_INVALID, "tdoa_track_batch: NULL argument");
    const int rc = tdoa_track_check("tdoa_track_batch", prm, out, count, xy, Kp, rows);
    if (rc)
        return rc;
    if (rows == 0)
        return TDOA_OK;
    const hipError_t e = hipSetDevice(device);
    if (e != hipSuccess)
        return tdoa_hip_fail(e, "tdoa_track_batch: hipSetDevice");
    return tdoa_launch_track(tracks, next_id, rows, nullptr, stream_of_row, t_us, nullptr, 0, count, xy, Kp, *prm,
                             *out, stream);
}
