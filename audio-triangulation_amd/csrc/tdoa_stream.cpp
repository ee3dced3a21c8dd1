// tdoa_stream.cpp -- host side of the streaming pipeline (include/tdoa.h,
// kernels in tdoa_stream.hip): device state, the per-hop kernel sequence
//   selector -> hop kernel
// and its hipGraph capture / replay.  The selector is the trigger
// (k_stream_trigger_p, or k_stream_trigger_lds<T> for the other hop shapes and
// int16 rings) or, in a continuous pipeline (tdoa_stream_create_continuous),
// k_stream_active -- one candidate frame per stream and hop behind an activity
// threshold.  Every selector lists the frames it chooses (stream, end, ring
// index), none copies a frame; every hop kernel stages its frames from the
// capture ring.  The hop kernel of a DIRECT pipeline is k_direct_mfma
// (device-sized batch, EMA + grid on the EMA scores fused) -- or, for shapes
// that kernel does not solve, k_direct -> k_stream_update; of a GCC_PHAT
// pipeline k_stream_phat (tdoa_stream_phat.hip: float scores, float EMA state,
// max_Lf), k_stream_phat_pcm16 on an int16 ring (tdoa_stream_create_pcm16) --
// or, for the long-frame shapes its LDS cannot hold (8 mics x 2048, 4 x 4096),
//   selector -> k_f16_ring -> k_stream_ema_grid
// (tdoa_phat_r16.hip: the batch engine's long-frame kernel over the listed
// frames; then the EMA and grid half of k_stream_phat on its scores).
// The hop's frame counter alternates between two slots by hop parity: the
// selector zeroes the other slot for the next hop (a memset node cost 3.9 us
// per hop), so the two parities are two captured graphs.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <memory>

#include "../../include/tdoa.h"
#include "tdoa_beam_rule.h"
#include "tdoa_devmem.h"
#include "tdoa_internal.h"
#include "tdoa_sep_rule.h"
#include "tdoa_track_rule.h"

// a step's outputs, either engine's: tdoa_stream_outputs with max_L null and
// max_Lf set for a GCC_PHAT pipeline (tdoa_stream_outputs_f)
struct step_out {
    tdoa_stream_outputs o{};
    float *max_Lf = nullptr;
};

// a captured step graph and what it was captured for
struct step_graph {
    hipGraphExec_t exec = nullptr;
    hipGraph_t graph = nullptr;
    step_out out{};
    const float *bin_w = nullptr;  // GCC_PHAT: the context's weight table at capture
    hipStream_t stream = nullptr;
    step_graph() = default;
    step_graph(const step_graph &) = delete;
    step_graph &operator=(const step_graph &) = delete;
    ~step_graph() { drop(); }
    void drop()
    {
        if (exec)
            (void)hipGraphExecDestroy(exec);
        if (graph)
            (void)hipGraphDestroy(graph);
        exec = nullptr;
        graph = nullptr;
    }
};

struct tdoa_stream {
    tdoa_ctx *ctx;
    int device;
    int64_t S;
    tdoa_kparams kp;
    tdoa_stream_params sp;
    tdoa_devmem mem;  // one allocation for all state
    tdoa_devmem peak_lags;  // tdoa_stream_peaks: [S][TDOA_MAX_PEAKS][P] lag tuples when only the refinement reads them
    tdoa_devmem track_mem;  // tdoa_stream_track: tracks [S][TDOA_MAX_TRACKS], then next_id [S]
    // tdoa_stream_sep: the window and twiddles of L = 2 hop, then the tails [S][4][hop]; made at its first call
    tdoa_devmem sep_mem;
    int32_t sep_kt = 0;     // ... the Kt of its last call: another Kt zeroes the tails
    int use_graph;
    int64_t hop = 0;  // steps enqueued since create / reset: the counter slot's parity
    step_graph g[2];  // one per counter parity; released before mem
    bool phat = false;      // GCC_PHAT pipeline: k_stream_phat after the selector
    float *est_f = nullptr; // ... its EMA state [S][P][K] (sp.est is null)
    float phat_eps = 0.0f;
    int phat_grid = 1;      // k_stream_phat's launch size (f16: k_stream_ema_grid's)
    // the long-frame route (k_f16_ring -> k_stream_ema_grid) and its per-slot
    // scratch, carved from mem: weighted scores [S][P][K], lags [S][P], gate [S]
    bool f16 = false;
    int f16_grid = 1;       // k_f16_ring's launch size
    float *f16_w = nullptr;
    int32_t *f16_lags = nullptr;
    uint8_t *f16_gate = nullptr;
    bool pcm16 = false;     // int16 capture ring (tdoa_stream_create_pcm16): k_stream_trigger_lds<int16_t>,
                            // k_stream_phat_pcm16; the format is the pipeline's from creation on
    bool continuous = false;  // tdoa_stream_create_continuous: k_stream_active lists the frames, no trigger
    int64_t thr = 0;        // the selector's threshold: trigger_var * (N/2)^2 (POWER_THRESHOLD = 2,
                            // sample_compute.h:21, for 8-bit rings), continuous: activity_var * N^2
};

namespace {

tdoa_stream_kout to_kout(const step_out &so)
{
    const tdoa_stream_outputs *o = &so.o;
    tdoa_stream_kout k{};
    k.count = o->count;
    k.stream_id = o->stream_id;
    k.end = o->end;
    k.lags = o->lags;
    k.gate = o->gate;
    k.ema_best = o->ema_best;
    k.cell = o->cell;
    k.xy = o->xy;
    k.max_L = o->max_L;
    return k;
}

// the per-hop kernel sequence; par: the hop's counter slot
int enqueue_step(tdoa_stream *st, const step_out &out, hipStream_t s, int par)
{
    tdoa_stream_params sp = st->sp;
    sp.count = st->sp.count + par;
    sp.count_next = st->sp.count + (1 - par);
    int rc = st->continuous ? tdoa_launch_stream_active(sp, st->S, st->thr, st->pcm16, s)
                            : tdoa_launch_stream_trigger(sp, st->S, st->thr, st->pcm16, s);
    if (rc)
        return rc;
    if (st->phat) {
        // the weight table in force on the context now (tdoa_set_bin_weights)
        tdoa_kparams kp = st->kp;
        const tdoa_kparams *ck = tdoa_ctx_kparams(st->ctx);
        kp.bin_w = ck->bin_w;
        kp.bin_lo = ck->bin_lo;
        kp.bin_hi = ck->bin_hi;
        if (st->f16) {
            const tdoa_stream_kout ko = to_kout(out);
            int32_t *lags = ko.lags ? ko.lags : st->f16_lags;
            rc = tdoa_launch_f16_ring(sp, kp, lags, st->f16_gate, st->f16_w, st->S, st->phat_eps, st->f16_grid, s,
                                      st->pcm16);
            if (rc)
                return rc;
            return tdoa_launch_stream_ema_grid(sp, kp, ko, st->est_f, out.max_Lf, st->f16_w, lags, st->f16_gate,
                                               st->S, st->phat_grid, s);
        }
        return tdoa_launch_stream_phat(sp, kp, to_kout(out), st->est_f, out.max_Lf, st->S, st->phat_eps,
                                       st->phat_grid, s, st->pcm16);
    }
    // DIRECT stages each listed frame from its stream's ring: no frame pointer
    tdoa_kparams kp = st->kp;
    kp.frame_ids = sp.ids;
    kp.frame_ring = sp.capture;
    kp.ring_len = sp.capture_len;
    kp.frame_end = sp.end;
    kp.frame_ring_at = sp.ring_at;
    if (tdoa_direct_ema_fits(kp)) {
        // k_direct_mfma runs the EMA and the grid on the EMA scores itself:
        // results straight into the caller's slots, no fresh-score round trip
        tdoa_stream_fuse ef{};
        ef.sp = sp;
        ef.so = to_kout(out);
        tdoa_kout ko{};
        ko.lags = ef.so.lags ? ef.so.lags : sp.fresh_lags;
        ko.gate = ef.so.gate;
        ko.cell = ef.so.cell;
        ko.xy = ef.so.xy;
        ko.max_L = ef.so.max_L;
        return tdoa_launch_direct(kp, ko, nullptr, st->S, false, s, nullptr, sp.count, &ef);
    }
    tdoa_kout ko{};
    ko.lags = sp.fresh_lags;
    ko.gate = sp.fresh_gate;
    ko.weighted = sp.fresh;
    rc = tdoa_launch_direct(kp, ko, nullptr, st->S, false, s, nullptr, sp.count);
    if (rc)
        return rc;
    return tdoa_launch_stream_update(sp, st->kp, to_kout(out), st->S, s);
}

// tdoa_stream_create (pcm16 false: `capture` holds bytes),
// tdoa_stream_create_pcm16 (int16 samples, GCC_PHAT in PCM16 format only) and
// tdoa_stream_create_continuous (GCC_PHAT only; the ring's type is the
// context's sample format, `pcm16` is not read; `var` is activity_var)
int stream_create(const char *fn, tdoa_ctx *ctx, int32_t num_streams, int32_t hop, const void *capture,
                  int64_t capture_len, bool pcm16, int64_t var, int use_graph, tdoa_stream **out,
                  bool continuous = false)
{
    if (!ctx || !out || !capture)
        return tdoa_fail(TDOA_ERR_INVALID, "%s: NULL argument", fn);
    *out = nullptr;
    const int engine = tdoa_ctx_engine(ctx);
    if (continuous && engine != TDOA_ENGINE_GCC_PHAT)
        return tdoa_fail(TDOA_ERR_INVALID, "%s: continuous mode needs a GCC_PHAT context (DIRECT reproduces the "
                                           "firmware, which has no such mode)", fn);
    if (engine != TDOA_ENGINE_DIRECT && engine != TDOA_ENGINE_GCC_PHAT)
        return tdoa_fail(TDOA_ERR_INVALID, "%s: needs a DIRECT or GCC_PHAT context", fn);
    const bool phat = engine == TDOA_ENGINE_GCC_PHAT;
    const tdoa_kparams &kp = *tdoa_ctx_kparams(ctx);
    const int M = kp.M, N = kp.N, P = kp.P, K = kp.K;
    const int64_t trigger_var = var;
    if (continuous) {
        pcm16 = kp.pcm16 != 0;
        if (var < 0 || var > ((int64_t)1 << 30))
            return tdoa_fail(TDOA_ERR_INVALID, "%s: activity_var %lld outside [0, 2^30]", fn, (long long)var);
        if (pcm16 && ((uintptr_t)capture & 1) != 0)
            return tdoa_fail(TDOA_ERR_INVALID, "%s: capture is not 2-byte aligned", fn);
    } else if (pcm16) {
        if (!phat)
            return tdoa_fail(TDOA_ERR_INVALID, "%s: an int16 capture ring needs a GCC_PHAT context (DIRECT stays 8-bit)",
                             fn);
        if (!kp.pcm16)
            return tdoa_fail(TDOA_ERR_INVALID, "%s: the context's sample format is ADC8; set TDOA_SAMPLES_PCM16 first "
                                               "(tdoa_set_sample_format)", fn);
        if (trigger_var < 0 || trigger_var > ((int64_t)1 << 30))
            return tdoa_fail(TDOA_ERR_INVALID, "%s: trigger_var %lld outside [0, 2^30]", fn, (long long)trigger_var);
        if (((uintptr_t)capture & 1) != 0)
            return tdoa_fail(TDOA_ERR_INVALID, "%s: capture is not 2-byte aligned", fn);
    } else if (kp.pcm16) {
        return tdoa_fail(TDOA_ERR_INVALID, "%s: this capture ring is 8-bit and the context's sample format is PCM16 "
                                           "(tdoa_set_sample_format): tdoa_stream_create_pcm16 takes int16 rings", fn);
    }
    // the long-frame route: the two shapes k_stream_phat's LDS cannot hold
    const bool f16 = phat && tdoa_f16_ring_shape(kp) && !tdoa_stream_phat_fits(kp);
    if (f16 && capture_len > (((int64_t)1 << 31) - 1) / (M * (pcm16 ? 2 : 1)))
        return tdoa_fail(TDOA_ERR_INVALID, "%s: capture_len %lld: a stream's ring of %d mics x frame_len %d must stay "
                                           "under 2^31 bytes", fn, (long long)capture_len, M, N);
    if (phat && !f16 && !tdoa_stream_phat_fits(kp))
        return tdoa_fail(TDOA_ERR_INVALID,
                         "%s: GCC_PHAT with %d mics x frame_len %d needs %zu bytes of LDS per "
                         "workgroup (limit 160 KiB)",
                         fn, M, N, tdoa_stream_phat_lds(kp));
    if (num_streams < 1)
        return tdoa_fail(TDOA_ERR_INVALID, "%s: num_streams %d < 1", fn, num_streams);
    if (hop < 1 || hop > N || hop > 4096)
        return tdoa_fail(TDOA_ERR_INVALID, "%s: hop %d outside [1, frame_len]", fn, hop);
    if (capture_len < (int64_t)N + 2 * hop)
        return tdoa_fail(TDOA_ERR_INVALID, "%s: capture_len %lld < frame_len + 2 hop", fn, (long long)capture_len);
    if (!continuous && tdoa_stream_trigger_lds(M, N, hop) > 150 * 1024)  // no trigger runs in continuous mode
        return tdoa_fail(TDOA_ERR_INVALID, "%s: (frame_len + hop) x mics too large", fn);
    const int dev = tdoa_ctx_device(ctx);
    HIP_TRY(hipSetDevice(dev));

    auto st = std::make_unique<tdoa_stream>();
    st->ctx = ctx;
    st->device = dev;
    st->S = num_streams;
    st->kp = kp;
    st->use_graph = use_graph;
    st->phat = phat;
    st->pcm16 = pcm16;
    st->continuous = continuous;
    st->f16 = f16;
    // <= 2^30 * 2^24; an 8-bit trigger's variance is the firmware's POWER_THRESHOLD (sample_compute.h:21)
    st->thr = continuous ? var * (int64_t)N * N : (pcm16 ? trigger_var : 2) * (int64_t)(N / 2) * (N / 2);
    if (phat) {
        st->phat_eps = tdoa_ctx_phat_eps(ctx);
        // TDOA_STREAM_PHAT_GRID=n caps k_stream_phat's launch size (A/B runs)
        // (of the long-frame route: both its launches)
        const char *cap = std::getenv("TDOA_STREAM_PHAT_GRID");
        const int gcap = cap ? std::atoi(cap) : 0;
        st->phat_grid = f16 ? tdoa_stream_ema_grid_size(kp, num_streams, gcap)
                            : tdoa_stream_phat_grid(kp, num_streams, gcap, pcm16);
        if (f16) {
            st->f16_grid = tdoa_f16_ring_grid(kp, num_streams, gcap, pcm16);
            if (st->f16_grid < 1)
                return tdoa_fail(TDOA_ERR_HIP, "%s: k_f16_ring: no resident workgroup (LDS / registers)", fn);
        }
    }
    const size_t S = (size_t)num_streams;
    // carve: 256-B aligned sub-buffers of one allocation
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t o = off;
        off = (off + bytes + 255) & ~(size_t)255;
        return o;
    };
    // (a GCC_PHAT pipeline keeps the frame's scores on chip: no fresh* buffers, float EMA state)
    const size_t o_pos = take(8), o_count = take(8), o_rs = take(S * 8), o_ids = take(S * 4),
                 o_end = take(S * 8), o_at = take(S * 8),
                 o_fresh = take(phat ? 0 : S * P * K * 8), o_fl = take(phat ? 0 : S * P * 4),
                 o_fg = take(phat ? 0 : S), o_est = take(S * P * K * (phat ? 4 : 8)), o_last = take(S * 8),
                 o_stats = take(16), o_fw = take(f16 ? S * P * K * 4 : 0), o_fll = take(f16 ? S * P * 4 : 0),
                 o_fgt = take(f16 ? S : 0);
    if (st->mem.alloc(off) != hipSuccess)
        return tdoa_fail(TDOA_ERR_NOMEM, "%s: %zu bytes of stream state", fn, off);
    char *b = st->mem.get<char>();
    tdoa_stream_params &sp = st->sp;
    sp.M = M;
    sp.N = N;
    sp.H = hop;
    sp.log2N = kp.log2N;
    sp.fs = tdoa_ctx_rate(ctx);
    sp.capture_len = capture_len;
    sp.capture = static_cast<const uint8_t *>(capture);
    sp.pos = (int64_t *)(b + o_pos);
    sp.count = (int32_t *)(b + o_count);
    sp.ring_start = (int64_t *)(b + o_rs);
    sp.ids = (int32_t *)(b + o_ids);
    sp.end = (int64_t *)(b + o_end);
    sp.ring_at = (int64_t *)(b + o_at);
    sp.fresh = phat ? nullptr : (int64_t *)(b + o_fresh);
    sp.fresh_lags = phat ? nullptr : (int32_t *)(b + o_fl);
    sp.fresh_gate = phat ? nullptr : (uint8_t *)(b + o_fg);
    sp.est = phat ? nullptr : (int64_t *)(b + o_est);
    st->est_f = phat ? (float *)(b + o_est) : nullptr;
    sp.last = (uint64_t *)(b + o_last);
    sp.stats = (int64_t *)(b + o_stats);
    if (f16) {
        st->f16_w = (float *)(b + o_fw);
        st->f16_lags = (int32_t *)(b + o_fll);
        st->f16_gate = (uint8_t *)(b + o_fgt);
    }
    if (hipMemset(st->mem.get<void>(), 0, off) != hipSuccess || hipDeviceSynchronize() != hipSuccess)
        return tdoa_fail(TDOA_ERR_HIP, "%s: clearing state failed", fn);
    *out = st.release();
    return TDOA_OK;
}

}  // namespace

extern "C" int tdoa_stream_create(tdoa_ctx *ctx, int32_t num_streams, int32_t hop,
                                  const uint8_t *capture, int64_t capture_len, int use_graph,
                                  tdoa_stream **out)
{
    return stream_create("tdoa_stream_create", ctx, num_streams, hop, capture, capture_len, false, 0, use_graph, out);
}

extern "C" int tdoa_stream_create_pcm16(tdoa_ctx *ctx, int32_t num_streams, int32_t hop,
                                        const int16_t *capture, int64_t capture_len, int64_t trigger_var,
                                        int use_graph, tdoa_stream **out)
{
    return stream_create("tdoa_stream_create_pcm16", ctx, num_streams, hop, capture, capture_len, true, trigger_var,
                         use_graph, out);
}

extern "C" int tdoa_stream_create_continuous(tdoa_ctx *ctx, int32_t num_streams, int32_t hop, const void *capture,
                                             int64_t capture_len, int64_t activity_var, int use_graph,
                                             tdoa_stream **out)
{
    return stream_create("tdoa_stream_create_continuous", ctx, num_streams, hop, capture, capture_len, false,
                         activity_var, use_graph, out, true);
}

namespace {

int stream_step(tdoa_stream *st, const step_out &out, void *stream)
{
    HIP_TRY(hipSetDevice(st->device));
    hipStream_t s = (hipStream_t)stream;
    const int par = (int)(st->hop & 1);
    if (!st->use_graph || !s) {
        const int rc = enqueue_step(st, out, s, par);
        if (!rc) {
            st->hop++;
        } else {
            // a launch after the trigger failed: the trigger may have counted
            // into this hop's slot without the hop advancing; both slots are
            // zeroed so the next hop's slot base starts at 0 again
            (void)hipMemsetAsync(st->sp.count, 0, 2 * sizeof(int32_t), s);
        }
        return rc;
    }
    const step_out &want = out;
    // the weight table is a kernel argument: a graph captured under another one is stale
    const float *bin_w = st->phat ? tdoa_ctx_kparams(st->ctx)->bin_w : nullptr;
    step_graph &sg = st->g[par];
    if (!sg.exec || sg.stream != s || sg.bin_w != bin_w || std::memcmp(&want.o, &sg.out.o, sizeof want.o) != 0 ||
        want.max_Lf != sg.out.max_Lf) {
        sg.drop();
        HIP_TRY(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
        const int rc = enqueue_step(st, out, s, par);
        hipGraph_t g = nullptr;
        const hipError_t ec = hipStreamEndCapture(s, &g);
        if (rc) {
            if (g)
                (void)hipGraphDestroy(g);
            return rc;
        }
        if (ec != hipSuccess)
            return tdoa_fail(TDOA_ERR_HIP, "hipStreamEndCapture: %s", hipGetErrorString(ec));
        sg.graph = g;
        HIP_TRY(hipGraphInstantiate(&sg.exec, g, nullptr, nullptr, 0));
        sg.out = want;
        sg.bin_w = bin_w;
        sg.stream = s;
    }
    const hipError_t el = hipGraphLaunch(sg.exec, s);
    if (el != hipSuccess) {
        // as in the eager path: a partly run hop may have counted into its
        // slot; both slots are zeroed so the next hop starts from slot 0
        (void)hipMemsetAsync(st->sp.count, 0, 2 * sizeof(int32_t), s);
        return tdoa_fail(TDOA_ERR_HIP, "hipGraphLaunch: %s", hipGetErrorString(el));
    }
    st->hop++;
    return TDOA_OK;
}

}  // namespace

extern "C" int tdoa_stream_step(tdoa_stream *st, const tdoa_stream_outputs *out, void *stream)
{
    if (!st)
        return tdoa_fail(TDOA_ERR_INVALID, "tdoa_stream_step: NULL stream");
    if (st->phat)
        return tdoa_fail(TDOA_ERR_INVALID, "tdoa_stream_step: a GCC_PHAT pipeline steps with tdoa_stream_step_f");
    step_out so;
    if (out)
        so.o = *out;
    return stream_step(st, so, stream);
}

extern "C" int tdoa_stream_step_f(tdoa_stream *st, const tdoa_stream_outputs_f *out, void *stream)
{
    if (!st)
        return tdoa_fail(TDOA_ERR_INVALID, "tdoa_stream_step_f: NULL stream");
    if (!st->phat)
        return tdoa_fail(TDOA_ERR_INVALID, "tdoa_stream_step_f: a DIRECT pipeline steps with tdoa_stream_step");
    step_out so;
    if (out) {
        so.o.count = out->count;
        so.o.stream_id = out->stream_id;
        so.o.end = out->end;
        so.o.lags = out->lags;
        so.o.gate = out->gate;
        so.o.ema_best = out->ema_best;
        so.o.cell = out->cell;
        so.o.xy = out->xy;
        so.max_Lf = out->max_Lf;
    }
    return stream_step(st, so, stream);
}

extern "C" int tdoa_stream_reset(tdoa_stream *st, void *stream)
{
    if (!st)
        return tdoa_fail(TDOA_ERR_INVALID, "tdoa_stream_reset: NULL stream");
    HIP_TRY(hipSetDevice(st->device));
    HIP_TRY(hipMemsetAsync(st->mem.get<void>(), 0, st->mem.bytes(), (hipStream_t)stream));
    if (st->track_mem)  // no tracks, ids from 1 again
        HIP_TRY(hipMemsetAsync(st->track_mem.get<void>(), 0, st->track_mem.bytes(), (hipStream_t)stream));
    if (st->sep_mem) {  // the tails behind the table
        const size_t tab = tdoa_sep_table_floats(2 * st->sp.H) * sizeof(float);
        HIP_TRY(hipMemsetAsync(st->sep_mem.get<char>() + tab, 0, st->sep_mem.bytes() - tab, (hipStream_t)stream));
    }
    st->hop = 0;  // both counter slots are zero again
    return TDOA_OK;
}

namespace {

// est: int64 [S][P][K] of a DIRECT pipeline or float of a GCC_PHAT one
int stream_state(tdoa_stream *st, int64_t *pos, void *est, uint64_t *last, int64_t *stats)
{
    HIP_TRY(hipSetDevice(st->device));
    HIP_TRY(hipDeviceSynchronize());
    const size_t S = (size_t)st->S;
    if (pos)
        HIP_TRY(hipMemcpy(pos, st->sp.pos, sizeof(int64_t), hipMemcpyDeviceToHost));
    if (est)
        HIP_TRY(hipMemcpy(est, st->phat ? (const void *)st->est_f : (const void *)st->sp.est,
                          S * st->kp.P * st->kp.K * (st->phat ? sizeof(float) : sizeof(int64_t)),
                          hipMemcpyDeviceToHost));
    if (last)
        HIP_TRY(hipMemcpy(last, st->sp.last, S * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (stats)
        HIP_TRY(hipMemcpy(stats, st->sp.stats, 2 * sizeof(int64_t), hipMemcpyDeviceToHost));
    return TDOA_OK;
}

}  // namespace

extern "C" int tdoa_stream_state(tdoa_stream *st, int64_t *pos, int64_t *est, uint64_t *last,
                                 int64_t *stats)
{
    if (!st)
        return tdoa_fail(TDOA_ERR_INVALID, "tdoa_stream_state: NULL stream");
    if (st->phat && est)
        return tdoa_fail(TDOA_ERR_INVALID, "tdoa_stream_state: a GCC_PHAT pipeline's scores are float "
                                           "(tdoa_stream_state_f)");
    return stream_state(st, pos, est, last, stats);
}

extern "C" int tdoa_stream_state_f(tdoa_stream *st, int64_t *pos, float *est, uint64_t *last,
                                   int64_t *stats)
{
    if (!st)
        return tdoa_fail(TDOA_ERR_INVALID, "tdoa_stream_state_f: NULL stream");
    if (!st->phat)
        return tdoa_fail(TDOA_ERR_INVALID, "tdoa_stream_state_f: a DIRECT pipeline's scores are int64 "
                                           "(tdoa_stream_state)");
    return stream_state(st, pos, est, last, stats);
}

extern "C" int tdoa_stream_peaks(tdoa_stream *st, const tdoa_peaks_params *prm, const uint8_t *gate,
                                 const tdoa_peaks_outputs *out, void *stream)
{
    if (!st || !prm || !out)
        return tdoa_fail(TDOA_ERR_INVALID, "tdoa_stream_peaks: NULL argument");
    if (!out->cell)
        return tdoa_fail(TDOA_ERR_INVALID, "tdoa_stream_peaks: outputs.cell is required");
    if (prm->num_peaks < 1 || prm->num_peaks > TDOA_MAX_PEAKS)
        return tdoa_fail(TDOA_ERR_INVALID, "tdoa_stream_peaks: num_peaks %d outside 1..%d", (int)prm->num_peaks,
                         TDOA_MAX_PEAKS);
    if (prm->radius < 0)
        return tdoa_fail(TDOA_ERR_INVALID, "tdoa_stream_peaks: negative radius");
    if (!tdoa_peaks_fits(st->kp, st->phat))
        return tdoa_fail(TDOA_ERR_INVALID,
                         "tdoa_stream_peaks: the L map and one stream's scores (%zu bytes) exceed the LDS budget",
                         tdoa_peaks_lds(st->kp, st->phat));
    if (st->hop == 0)  // no step since creation or reset: no list to read
        return TDOA_OK;
    HIP_TRY(hipSetDevice(st->device));
    const int Kp = prm->num_peaks, P = st->kp.P;
    const bool ls = out->xy_ls || out->ls_rms;
    tdoa_peaks_kout k;
    k.count = out->count;
    k.cell = out->cell;
    k.xy = out->xy;
    k.L = st->phat ? nullptr : out->L;  // the pipeline's type decides which is written
    k.Lf = st->phat ? out->Lf : nullptr;
    k.lags = out->lags;
    if (ls && !k.lags) {
        // the refinement reads each peak's lag tuple: one scratch for every Kp, made once
        const size_t need = (size_t)st->S * TDOA_MAX_PEAKS * P * sizeof(int32_t);
        if (!st->peak_lags && st->peak_lags.alloc(need) != hipSuccess)
            return tdoa_fail(TDOA_ERR_NOMEM, "tdoa_stream_peaks: peak-lag scratch of %zu bytes", need);
        k.lags = st->peak_lags.get<int32_t>();
    }
    // the last step's counter slot and list: both hold until the next step,
    // whose selector zeroes that slot (its count_next) and writes a new list
    const int32_t *count = st->sp.count + (int)((st->hop - 1) & 1);
    const void *est = st->phat ? (const void *)st->est_f : (const void *)st->sp.est;
    int rc = tdoa_launch_stream_peaks(st->kp, k, est, st->phat, st->sp.ids, count, gate, st->S, Kp, prm->radius,
                                      prm->min_rel, stream);
    if (rc != 0 || !ls)
        return rc;
    return tdoa_launch_ls_stream(st->kp, est, st->phat, st->sp.ids, count, st->S, k.lags, k.cell, out->xy_ls,
                                 out->ls_rms, Kp, stream);
}

extern "C" const char *tdoa_stream_kernel(const tdoa_stream *st)
{
    if (!st)
        return nullptr;
    if (st->phat)
        return st->f16 ? "k_f16_ring" : (st->pcm16 ? "k_stream_phat_pcm16" : "k_stream_phat");
    tdoa_kparams kp = st->kp;  // as enqueue_step launches DIRECT: frames staged from the rings
    kp.frame_ids = st->sp.ids;
    kp.frame_ring = st->sp.capture;
    kp.ring_len = st->sp.capture_len;
    kp.frame_end = st->sp.end;
    kp.frame_ring_at = st->sp.ring_at;
    return tdoa_direct_ema_fits(kp) ? "k_direct_mfma" : "k_direct";
}

extern "C" int tdoa_stream_est_device(tdoa_stream *st, const void **est, int *is_float)
{
    if (!st || !est || !is_float)
        return tdoa_fail(TDOA_ERR_INVALID, "tdoa_stream_est_device: NULL argument");
    *est = st->phat ? (const void *)st->est_f : (const void *)st->sp.est;
    *is_float = st->phat ? 1 : 0;
    return TDOA_OK;
}

extern "C" int tdoa_stream_track(tdoa_stream *st, const tdoa_track_params *prm, const int32_t *count,
                                 const float *xy, int32_t Kp, const tdoa_track_outputs *out, void *stream)
{
    if (!st)
        return tdoa_fail(TDOA_ERR_INVALID, "tdoa_stream_track: NULL argument");
    const int rc = tdoa_track_check("tdoa_stream_track", prm, out, count, xy, Kp, st->S);
    if (rc)
        return rc;
    HIP_TRY(hipSetDevice(st->device));
    const size_t S = (size_t)st->S;
    if (!st->track_mem) {
        // the one allocation, zeroed before anything else on `stream` reads it
        const size_t need = S * (TDOA_MAX_TRACKS * sizeof(tdoa_track) + sizeof(int32_t));
        if (st->track_mem.alloc(need) != hipSuccess)
            return tdoa_fail(TDOA_ERR_NOMEM, "tdoa_stream_track: %zu bytes of track state", need);
        if (hipMemsetAsync(st->track_mem.get<void>(), 0, need, (hipStream_t)stream) != hipSuccess) {
            st->track_mem.release();
            return tdoa_fail(TDOA_ERR_HIP, "tdoa_stream_track: clearing the track state failed");
        }
    }
    if (st->hop == 0)  // no step since creation or reset: no list to read
        return TDOA_OK;
    tdoa_track *tracks = st->track_mem.get<tdoa_track>();
    int32_t *next_id = reinterpret_cast<int32_t *>(tracks + S * TDOA_MAX_TRACKS);
    // the last step's counter slot and lists, as tdoa_stream_peaks reads them
    const int32_t *rows_dev = st->sp.count + (int)((st->hop - 1) & 1);
    return tdoa_launch_track(tracks, next_id, st->S, rows_dev, st->sp.ids, nullptr, st->sp.end, st->sp.fs, count, xy,
                             Kp, *prm, *out, stream);
}

extern "C" int tdoa_stream_tracks_device(tdoa_stream *st, const tdoa_track **tracks, const int32_t **next_id)
{
    if (!st || !tracks || !next_id)
        return tdoa_fail(TDOA_ERR_INVALID, "tdoa_stream_tracks_device: NULL argument");
    const tdoa_track *t = st->track_mem ? st->track_mem.get<tdoa_track>() : nullptr;
    *tracks = t;
    *next_id = t ? reinterpret_cast<const int32_t *>(t + (size_t)st->S * TDOA_MAX_TRACKS) : nullptr;
    return TDOA_OK;
}

// What tdoa_stream_beam and tdoa_stream_sep share, before and after their own
// argument checks: the pipeline's beamformer geometry ...
static int stream_beam_open(tdoa_stream *st, const char *fn, const tdoa_beam_outputs *out, tdoa_beam_geometry *g,
                            int *Dmax, const float **fir)
{
    if (!st || !out)
        return tdoa_fail(TDOA_ERR_INVALID, "%s: NULL argument", fn);
    return tdoa_ctx_beam(st->ctx, fn, g, Dmax, fir);
}

// ... and its capture rings as a launch's source, the caller's xy -- or, xy
// null, the track table -- as its targets
static int stream_beam_io(tdoa_stream *st, const char *fn, const int32_t *count, const float *xy, int32_t Kt,
                          int32_t min_status, tdoa_beam_source *source, tdoa_beam_targets *targets)
{
    if (!xy && !st->track_mem)
        return tdoa_fail(TDOA_ERR_INVALID, "%s: no xy and no track table yet (tdoa_stream_track makes it)", fn);
    *source = tdoa_beam_source{st->sp.capture, st->pcm16, st->sp.capture_len, st->sp.pos, st->S};
    *targets = tdoa_beam_targets{count, xy, xy ? nullptr : st->track_mem.get<tdoa_track>(), min_status, Kt};
    return TDOA_OK;
}

extern "C" int tdoa_stream_beam(tdoa_stream *st, const int32_t *count, const float *xy, int32_t Kt,
                                int32_t min_status, const tdoa_beam_outputs *out, void *stream)
{
    tdoa_beam_geometry g;
    int Dmax = 0;
    const float *fir = nullptr;
    tdoa_beam_source source;
    tdoa_beam_targets targets;
    if (const int rc = stream_beam_open(st, "tdoa_stream_beam", out, &g, &Dmax, &fir))
        return rc;
    const int hop = st->sp.H, A = Dmax + TDOA_BEAM_HALF;
    if (const int rc = tdoa_beam_check("tdoa_stream_beam", g, Dmax, hop, Kt, out, out->audio, true))
        return rc;
    if (const int rc = stream_beam_io(st, "tdoa_stream_beam", count, xy, Kt, min_status, &source, &targets))
        return rc;
    // a block reaches hop + A + 7 samples back from the clock and Dmax + 8 past
    // its last output; one more hop is the producer's margin
    const int64_t need = 2 * (int64_t)hop + A + Dmax + 16;
    if (st->sp.capture_len < need)
        return tdoa_fail(TDOA_ERR_INVALID, "tdoa_stream_beam: capture_len %lld < 2 hop + A + Dmax + 16 = %lld",
                         (long long)st->sp.capture_len, (long long)need);
    if (st->hop == 0)  // no step since creation or reset: the clock has not moved
        return TDOA_OK;
    HIP_TRY(hipSetDevice(st->device));
    return tdoa_launch_beam(g, Dmax, source, hop, targets, fir, *out, stream);
}

extern "C" int tdoa_stream_sep(tdoa_stream *st, const int32_t *count, const float *xy, int32_t Kt, int32_t min_status,
                               float loading, const tdoa_beam_outputs *out, void *stream)
{
    tdoa_beam_geometry g;
    int Dmax = 0;
    const float *fir = nullptr;
    tdoa_beam_source source;
    tdoa_beam_targets targets;
    if (const int rc = stream_beam_open(st, "tdoa_stream_sep", out, &g, &Dmax, &fir))
        return rc;
    const int hop = st->sp.H, L = 2 * hop;
    if (const int rc = tdoa_sep_check("tdoa_stream_sep", Dmax, L, Kt, loading, out, out->audio))
        return rc;
    if (const int rc = stream_beam_io(st, "tdoa_stream_sep", count, xy, Kt, min_status, &source, &targets))
        return rc;
    // a block reaches L = 2 hop samples back from the clock; one more hop is the producer's margin
    if (st->sp.capture_len < 3 * (int64_t)hop)
        return tdoa_fail(TDOA_ERR_INVALID, "tdoa_stream_sep: capture_len %lld < 3 hop = %lld",
                         (long long)st->sp.capture_len, (long long)(3 * (int64_t)hop));
    if (st->hop == 0)  // no step since creation or reset: the clock has not moved
        return TDOA_OK;
    HIP_TRY(hipSetDevice(st->device));
    const size_t tab_floats = tdoa_sep_table_floats(L);
    const size_t tail_bytes = (size_t)st->S * TDOA_SEP_MAX_TARGETS * hop * sizeof(float);
    bool clear = Kt != st->sep_kt;
    if (!st->sep_mem) {
        std::unique_ptr<float[]> tab(new float[tab_floats]);
        if (const int rc = tdoa_sep_table(L, tab.get()))
            return rc;
        if (st->sep_mem.alloc(tab_floats * sizeof(float) + tail_bytes) != hipSuccess)
            return tdoa_fail(TDOA_ERR_NOMEM, "tdoa_stream_sep: %zu bytes of table and tail state",
                             tab_floats * sizeof(float) + tail_bytes);
        if (hipMemcpy(st->sep_mem.get<void>(), tab.get(), tab_floats * sizeof(float), hipMemcpyHostToDevice) !=
            hipSuccess) {
            st->sep_mem.release();
            return tdoa_fail(TDOA_ERR_HIP, "tdoa_stream_sep: uploading the window and twiddles failed");
        }
        clear = true;
    }
    float *tail = st->sep_mem.get<float>() + tab_floats;
    if (clear && hipMemsetAsync(tail, 0, tail_bytes, (hipStream_t)stream) != hipSuccess)
        return tdoa_fail(TDOA_ERR_HIP, "tdoa_stream_sep: clearing the tails failed");
    st->sep_kt = Kt;
    return tdoa_launch_sep(g, Dmax, source, L, targets, loading, st->sep_mem.get<float>(), tail, *out, stream);
}

extern "C" int tdoa_stream_destroy(tdoa_stream *st)
{
    if (!st)
        return TDOA_OK;
    (void)hipSetDevice(st->device);
    (void)hipDeviceSynchronize();
    delete st;  // the graphs, then the state
    return TDOA_OK;
}
