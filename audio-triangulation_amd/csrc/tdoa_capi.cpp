// tdoa_capi.cpp -- host side of libtdoa: the context (its device memory and
// kernel parameters) and the batched entry points declared in include/tdoa.h.
//
// Everything a context computes before it touches the GPU -- window, prior,
// LUT, lag tuples, the k_grid_bb tables, twiddles -- is built by
// tdoa_build_tables (tdoa_tables.cpp, host only); tdoa_create uploads it.
// Everything per frame runs in the gfx950 kernels (the .hip files beside this
// one, reached through the launchers of tdoa_internal.h).

#include "../../include/tdoa.h"
#include "tdoa_beam_rule.h"
#include "tdoa_devmem.h"
#include "tdoa_internal.h"
#include "tdoa_sep_rule.h"
#include "tdoa_tables.h"

#include <hip/hip_runtime.h>

#include <cstdlib>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <tuple>
#include <vector>

// ------------------------------------------------------------ context
struct tdoa_ctx {
    tdoa_tables t;  // the host tables (tdoa_tables.h)
    int device;
    // their device copies
    tdoa_devmem window, prior, tuples, tuple_cell, mic, lut;
    tdoa_devmem tw;       // GCC_PHAT twiddles (tdoa_tables::tw)
    tdoa_devmem p1k_img;  // LDS table image of the config-2 GCC_PHAT kernel
    tdoa_devmem w64_img;  // ... and of its one-frame-per-wave form
    tdoa_devmem bb;       // k_grid_bb tables: tiles | ranges | tuples | uidx | queries
    tdoa_devmem wc;       // compact weighted-score chunk table (kp.wc_chunks)
    tdoa_devmem fgq;      // kp.fg_q, kp.fg_tup
    // scratch that grows on demand:
    // weighted scores for the grid kernel when the caller did not ask for them
    // ([B][P][K] int64 or float, or the compact layout)
    tdoa_devmem wscratch;
    // raw scores, cells and [B][P][3] float peak scores for the least-squares refinement
    tdoa_devmem rscratch, cscratch, tscratch;
    tdoa_devmem pscratch;  // tdoa_peaks: [B][Kp][P] lag tuples when only the refinement reads them
    // GCC_PHAT spectrum scratch (TDOA_SPEC_BYTES) of the two-pass shapes (M > 3
    // or N > 2048) and, on demand, of a band-limited or 16-bit (PCM16) context
    tdoa_devmem spec;
    // band-limited GCC_PHAT (tdoa_set_bin_weights): the table in force (empty:
    // none) and its device copy, [N + 1] floats, kept once allocated
    std::vector<float> bin_w;
    tdoa_devmem d_bin_w;
    // the beamformer (tdoa_beam_batch, tdoa_stream_beam): what steering reads of
    // the config, the largest inter-mic delay, the FIR table's device copy
    tdoa_beam_geometry beam_g;
    int beam_dmax = 0;
    tdoa_devmem beam_fir;
    // the null-steering beamformer (tdoa_sep_batch): the window and twiddles of
    // its block length L (0: none; frame_len at creation where that is a block it
    // takes, tdoa_sep_set_block chooses another)
    tdoa_devmem sep_tab;
    int sep_L = 0;
    tdoa_kparams kp;
};

extern "C" int tdoa_config_default(tdoa_config *cfg)
{
    if (!cfg)
        return tdoa_fail(TDOA_ERR_INVALID, "tdoa_config_default: NULL");
    std::memset(cfg, 0, sizeof *cfg);
    cfg->num_mics = 3;
    cfg->frame_len = 1024;
    cfg->sample_rate_hz = 50000;
    cfg->max_shift = 0;
    cfg->speed_of_sound = 343.0f;
    cfg->engine = TDOA_ENGINE_DIRECT;
    cfg->mic_xy = nullptr;
    cfg->grid_half_w = 50;
    cfg->grid_half_h = 50;
    cfg->grid_scale = 24.0f;
    cfg->height_offset = 1.2f;
    cfg->window_q15 = nullptr;
    cfg->phat_eps = 1e-12f;
    return TDOA_OK;
}

namespace {

int check_device(int device)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return tdoa_fail(TDOA_ERR_NO_DEVICE, "no HIP device visible (libtdoa has no CPU path)");
    if (device < 0 || device >= ndev)
        return tdoa_fail(TDOA_ERR_INVALID, "device %d out of range (%d visible)", device, ndev);
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return tdoa_fail(TDOA_ERR_NO_DEVICE, "device %d is %s; libtdoa is built for gfx950 only",
                         device, prop.gcnArchName);
    return TDOA_OK;
}

template <typename T> size_t vbytes(const std::vector<T> &v) { return v.size() * sizeof(T); }

// window, prior, tuples, their first cells, microphones, LUT
int upload_tables(tdoa_ctx *c)
{
    const tdoa_tables &t = c->t;
    std::vector<int16_t> w16(t.N);
    for (int i = 0; i < t.N; i++)
        w16[i] = (int16_t)t.win[i];
    if (c->window.alloc(vbytes(w16)) != hipSuccess || c->prior.alloc(vbytes(t.prior)) != hipSuccess ||
        c->tuples.alloc(vbytes(t.tuples)) != hipSuccess || c->tuple_cell.alloc(vbytes(t.tuple_cell)) != hipSuccess ||
        c->mic.alloc(vbytes(t.mic)) != hipSuccess || c->lut.alloc(vbytes(t.lut)) != hipSuccess)
        return tdoa_fail(TDOA_ERR_NOMEM, "hipMalloc of context tables failed");
    hipError_t e = c->window.upload(w16.data(), vbytes(w16));
    if (e == hipSuccess)
        e = c->mic.upload(t.mic.data(), vbytes(t.mic));
    if (e == hipSuccess)
        e = c->lut.upload(t.lut.data(), vbytes(t.lut));
    if (e == hipSuccess)
        e = c->prior.upload(t.prior.data(), vbytes(t.prior));
    if (e == hipSuccess)
        e = c->tuples.upload(t.tuples.data(), vbytes(t.tuples));
    if (e == hipSuccess)
        e = c->tuple_cell.upload(t.tuple_cell.data(), vbytes(t.tuple_cell));
    if (e != hipSuccess)
        return tdoa_fail(TDOA_ERR_HIP, "uploading context tables: %s", hipGetErrorString(e));
    return TDOA_OK;
}

// GCC_PHAT: twiddles, the config-2 kernels' LDS images, the spectrum scratch
int upload_gcc_phat(tdoa_ctx *c)
{
    const tdoa_tables &t = c->t;
    if (c->tw.upload(t.tw.data(), vbytes(t.tw)) != hipSuccess)
        return tdoa_fail(TDOA_ERR_NOMEM, "uploading twiddle tables failed");
    std::vector<uint8_t> img;
    tdoa_phat1024_image(t.M, t.N, t.K, t.U, t.tw.data(), t.win.data(), t.prior.data(), t.tuples.data(),
                        t.tuple_cell.data(), img);
    if (!img.empty() && c->p1k_img.upload(img.data(), img.size()) != hipSuccess)
        return tdoa_fail(TDOA_ERR_NOMEM, "uploading the GCC_PHAT table image failed");
#if TDOA_AB
    // the one-frame-per-wave A/B kernel's image (tdoa/libtdoa_ab.so only)
    tdoa_p1k_w64_image(t.M, t.N, t.K, t.U, t.win.data(), t.prior.data(), t.tuples.data(), img);
    if (!img.empty() && c->w64_img.upload(img.data(), img.size()) != hipSuccess)
        return tdoa_fail(TDOA_ERR_NOMEM, "uploading the GCC_PHAT (w64) table image failed");
#endif
    if (tdoa_gcc_phat_needs_split(t.M, t.N) && c->spec.alloc(TDOA_SPEC_BYTES) != hipSuccess)
        return tdoa_fail(TDOA_ERR_NOMEM, "GCC_PHAT spectrum scratch of %zu bytes", TDOA_SPEC_BYTES);
    return TDOA_OK;
}

// k_grid_bb's tables; the compact chunk table and the fused k_frame16 grid's
// tables are optional: without them the kernels that read them are not chosen
int upload_grid(tdoa_ctx *c)
{
    const tdoa_tables &t = c->t;
    if (t.bb_NT <= 0)
        return TDOA_OK;
    if (c->bb.upload(t.bb_img.data(), t.bb_img.size()) != hipSuccess)
        return tdoa_fail(TDOA_ERR_NOMEM, "uploading the grid tile tables failed");
    if (!t.wc_ok || c->wc.upload(t.wc_chunks.data(), vbytes(t.wc_chunks)) != hipSuccess) {
        c->wc.release();
        return TDOA_OK;
    }
#if TDOA_AB
    if (t.fg_ok && c->fgq.upload(t.fg.data(), vbytes(t.fg)) != hipSuccess)
        c->fgq.release();
#endif
    return TDOA_OK;
}

// the beamformer's geometry (the tables' mics and the config's scalars), its
// largest delay, and the FIR table
int upload_beam(tdoa_ctx *c)
{
    const tdoa_tables &t = c->t;
    tdoa_beam_geometry &g = c->beam_g;
    std::memset(&g, 0, sizeof g);
    g.num_mics = t.M;
    g.sample_rate_hz = t.cfg.sample_rate_hz;
    g.speed_of_sound = t.cfg.speed_of_sound;
    g.height_offset = t.cfg.height_offset;
    std::memcpy(&g.mic_xy[0][0], t.mic.data(), vbytes(t.mic));
    // a geometry the beamformer cannot take (mics further apart than 65535
    // samples, a non-finite coordinate) leaves beam_dmax 0: its calls say why
    if (tdoa_beam_dmax(g, &c->beam_dmax) != TDOA_OK)
        c->beam_dmax = 0;
    float fir[TDOA_BEAM_PHASES * TDOA_BEAM_TAPS];
    tdoa_beam_fir(fir);
    if (c->beam_fir.upload(fir, sizeof fir) != hipSuccess)
        return tdoa_fail(TDOA_ERR_NOMEM, "uploading the beamformer's FIR table failed");
    return TDOA_OK;
}

// the separator's block length and its table: L = frame_len at creation where
// that is a block it takes (tdoa_sep_set_block chooses another)
int upload_sep(tdoa_ctx *c, int L)
{
    std::vector<float> tab(tdoa_sep_table_floats(L));
    if (const int rc = tdoa_sep_table(L, tab.data()))
        return rc;
    tdoa_devmem mem;
    if (mem.upload(tab.data(), vbytes(tab)) != hipSuccess)
        return tdoa_fail(TDOA_ERR_NOMEM, "uploading the separator's window and twiddles failed");
    c->sep_tab = std::move(mem);  // (the table it held goes with mem)
    c->sep_L = L;
    return TDOA_OK;
}

// the kernel parameters: the tables' scalars, then every device pointer
void wire_kparams(tdoa_ctx *c)
{
    const tdoa_tables &t = c->t;
    tdoa_kparams &kp = c->kp;
    kp = t.kp;
    kp.window = c->window.get<int16_t>();
    kp.prior = c->prior.get<float>();
    kp.mic_xy = c->mic.get<float>();
    kp.lut = c->lut.get<uint8_t>();
    kp.tuples = c->tuples.get<uint32_t>();
    kp.tuple_cell = c->tuple_cell.get<int32_t>();
    kp.tw = c->tw.get<float>();
    kp.tw2 = kp.tw + t.tw2_at;
    kp.r16_tw = kp.tw + t.r16_at;
    kp.p1k_img = c->p1k_img.get<void>();
    kp.p1k_img_bytes = (int32_t)c->p1k_img.bytes();
    kp.w64_img = c->w64_img.get<void>();
    kp.w64_img_bytes = (int32_t)c->w64_img.bytes();
    if (c->bb) {
        const char *b = c->bb.get<char>();
        kp.bb_tile = (const int32_t *)(b + t.bb_at[tdoa_tables::BB_TILE]);
        kp.bb_rng = (const uint16_t *)(b + t.bb_at[tdoa_tables::BB_RNG]);
        kp.bb_tuples = (const uint32_t *)(b + t.bb_at[tdoa_tables::BB_TUPLES]);
        kp.bb_uidx = (const int32_t *)(b + t.bb_at[tdoa_tables::BB_UIDX]);
        kp.bb_q = (const uint16_t *)(b + t.bb_at[tdoa_tables::BB_Q]);
    }
    kp.wc_chunks = c->wc.get<uint32_t>();
    if (!c->wc)
        kp.wc_CK = kp.wc_nch = 0;  // no compact mode (tdoa_grid_bb_compact)
#if TDOA_AB
    if (c->fgq) {
        kp.fg_q = c->fgq.get<uint16_t>();
        kp.fg_tup = (const uint16_t *)(c->fgq.get<char>() + t.fg_tup_at);
        kp.fg_ok = 1;
    }
#endif
}

}  // namespace

extern "C" int tdoa_create(const tdoa_config *cfg, int device, tdoa_ctx **out)
{
    if (!cfg || !out)
        return tdoa_fail(TDOA_ERR_INVALID, "tdoa_create: NULL argument");
    *out = nullptr;
    auto c = std::make_unique<tdoa_ctx>();
    if (const int rc = tdoa_build_tables(cfg, &c->t))
        return rc;
    if (const int rc = check_device(device))
        return rc;
    c->device = device;
    HIP_TRY(hipSetDevice(device));
    if (const int rc = upload_tables(c.get()))
        return rc;
    if (const int rc = upload_gcc_phat(c.get()))
        return rc;
    if (const int rc = upload_grid(c.get()))
        return rc;
    if (const int rc = upload_beam(c.get()))
        return rc;
    // (asked without tdoa_sep_check: a frame_len the separator does not take is no error here)
    const int N = c->t.N;
    if (c->beam_dmax > 0 && N >= 128 && N <= 2048 && (N & (N - 1)) == 0 && N >= 8 * (int64_t)c->beam_dmax) {
        if (const int rc = upload_sep(c.get(), N))
            return rc;
    }
    wire_kparams(c.get());
    *out = c.release();
    return TDOA_OK;
}

extern "C" int tdoa_destroy(tdoa_ctx *ctx)
{
    if (!ctx)
        return TDOA_OK;
    (void)hipSetDevice(ctx->device);
    std::unique_ptr<tdoa_ctx> released(ctx);  // its device memory goes with the device selected
    return TDOA_OK;
}

extern "C" int tdoa_get_dims(const tdoa_ctx *c, int32_t *M, int32_t *N, int32_t *P,
                             int32_t *K, int32_t *G)
{
    if (!c)
        return tdoa_fail(TDOA_ERR_INVALID, "tdoa_get_dims: NULL ctx");
    if (M)
        *M = c->t.M;
    if (N)
        *N = c->t.N;
    if (P)
        *P = c->t.P;
    if (K)
        *K = c->t.K;
    if (G)
        *G = c->t.G;
    return TDOA_OK;
}

static tdoa_kout to_kout(const tdoa_outputs *o)
{
    tdoa_kout k{};
    k.lags = o->lags;
    k.gate = o->gate;
    k.cell = o->cell;
    k.xy = o->xy;
    k.max_L = o->max_L;
    k.max_Lf = o->max_Lf;
    k.scores = o->scores;
    k.weighted = o->weighted;
    k.scores_f = o->scores_f;
    k.weighted_f = o->weighted_f;
    return k;
}

int tdoa_hip_fail(hipError_t e, const char *what)
{
    return tdoa_fail(TDOA_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
}

int tdoa_resident_blocks(const void *kernel, int threads, size_t lds)
{
    static std::mutex mu;
    static std::map<std::tuple<int, const void *, int, size_t>, int> cache;
    int dev = 0;
    (void)hipGetDevice(&dev);
    const auto key = std::make_tuple(dev, kernel, threads, lds);
    std::lock_guard<std::mutex> lk(mu);
    auto it = cache.find(key);
    if (it != cache.end())
        return it->second;
    int per_cu = 0, cus = 0;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, lds);
    const int r = (per_cu > 0 ? per_cu : 1) * (cus > 0 ? cus : 256);
    cache[key] = r;
    return r;
}

// A/B switch of the environment: set and not "0"
static bool env_flag(const char *name)
{
    const char *e = getenv(name);
    return e && *e && strcmp(e, "0") != 0;
}

// frames per k_frame16 -> k_grid_bb chunk in the compact mode: TDOA_F16_CHUNK
// (A/B switch; default 0, the whole batch in one launch pair).  Measured at
// config 4 (same box, ms per 1e6 frames): chunks of 16384 / 32768 frames 87.4 /
// 86.5 vs 85.8 unchunked -- and the counter traffic does not drop: the compact
// scores still leave and re-enter the L2 (k_frame16 writes 7.5 GB, k_grid_bb
// reads 7.1 GB per 1e6 frames, FETCH_SIZE / WRITE_SIZE count L2 <-> fabric
// requests whether the MALL serves them or HBM does), and each chunk adds two
// launch tails (DESIGN.md, round-6 negative results)
static int64_t compact_chunk(int64_t B)
{
    static const int64_t chunk = [] {
        const char *e = getenv("TDOA_F16_CHUNK");
        return e ? (int64_t)atoll(e) : (int64_t)0;
    }();
    return chunk > 0 && chunk < B ? chunk : B;
}

// the outputs of frames [c0, ...) of a batch (per-frame arrays advanced; the
// compact scratch, reused per chunk, is not)
static tdoa_kout offset_kout(const tdoa_kout &k, int64_t c0, int P, int K)
{
    tdoa_kout o = k;
    auto adv = [&](auto *&ptr, int64_t per) {
        if (ptr)
            ptr += c0 * per;
    };
    adv(o.lags, P);
    adv(o.gate, 1);
    adv(o.cell, 1);
    adv(o.xy, 2);
    adv(o.max_L, 1);
    adv(o.max_Lf, 1);
    adv(o.scores, (int64_t)P * K);
    adv(o.weighted, (int64_t)P * K);
    adv(o.scores_f, (int64_t)P * K);
    adv(o.weighted_f, (int64_t)P * K);
    adv(o.peak3, (int64_t)P * 3);
    return o;
}

// (TDOA_F16_CHUNK, A/B) the compact scratch of one chunk of frames at a time,
// reused: k_frame16 writes it and k_grid_bb reads it back while it can still
// sit in the 256 MB MALL (16384 x 7.3 KB at config 4)
static int run_compact_chunks(tdoa_ctx *ctx, const tdoa_kout &k, const int16_t *frames, int64_t B, int64_t chunk,
                              const void *weighted, void *stream)
{
    const int64_t M = ctx->kp.M, N = ctx->kp.N;
    int rc = 0;
    for (int64_t c0 = 0; rc == 0 && c0 < B; c0 += chunk) {
        const int64_t n = B - c0 < chunk ? B - c0 : chunk;
        const tdoa_kout kc = offset_kout(k, c0, ctx->t.P, ctx->t.K);
        rc = tdoa_launch_gcc_phat(ctx->kp, kc, frames + c0 * M * N, n, ctx->t.cfg.phat_eps, ctx->spec.get<void>(),
                                  ctx->spec.bytes(), stream);
        if (rc == 0)
            rc = tdoa_launch_grid(ctx->kp, kc, weighted, true, n, stream);
    }
    return rc;
}

static int run_batch(tdoa_ctx *ctx, const int16_t *frames, int64_t B, const tdoa_outputs *out,
                     void *stream, bool prepared)
{
    if (!ctx || !out)
        return tdoa_fail(TDOA_ERR_INVALID, "localize: NULL argument");
    if (B < 0)
        return tdoa_fail(TDOA_ERR_INVALID, "localize: negative batch");
    if (B == 0)
        return TDOA_OK;
    if (!frames)
        return tdoa_fail(TDOA_ERR_INVALID, "localize: NULL frames");
    if (!out->lags)
        return tdoa_fail(TDOA_ERR_INVALID, "localize: outputs.lags is required");
    HIP_TRY(hipSetDevice(ctx->device));
    const bool phat = ctx->t.cfg.engine == TDOA_ENGINE_GCC_PHAT && !prepared;
    tdoa_kout k = to_kout(out);
    const bool ls = out->xy_ls || out->ls_rms;
    const bool grid =
        ls || out->cell || out->xy || (phat ? out->max_Lf != nullptr : out->max_L != nullptr);
    const size_t sz = phat ? sizeof(float) : sizeof(int64_t);
    const size_t pk = (size_t)B * ctx->t.P * ctx->t.K * sz;
    const void *weighted = phat ? (const void *)out->weighted_f : (const void *)out->weighted;
    const bool fused_grid = phat ? tdoa_gcc_phat_grid_in_kernel(ctx->kp) : tdoa_direct_fused_grid(ctx->kp);
    // the per-frame long-frame kernel (k_frame16) can write only the lags the
    // grid reads, compacted, when k_grid_bb solves the grid (configs 3, 4)
    const bool compact = grid && !weighted && !fused_grid && phat && tdoa_gcc_phat_peak3(ctx->kp) &&
                         tdoa_grid_bb_compact(ctx->kp) && !env_flag("TDOA_NO_COMPACT");
    const int64_t chunk = compact ? compact_chunk(B) : B;
    if (compact) {
        if (const int rc = ctx->wscratch.grow((size_t)chunk * ctx->kp.wc_CK * sizeof(float), stream,
                                                    "weighted-score"))
            return rc;
        k.weighted_c = ctx->wscratch.get<float>();
        weighted = k.weighted_c;
    } else if (grid && !weighted && !fused_grid) {
        // the grid kernel reads the weighted scores back: keep them in scratch
        if (const int rc = ctx->wscratch.grow(pk, stream, "weighted-score"))
            return rc;
        weighted = ctx->wscratch.get<void>();
        if (phat)
            k.weighted_f = ctx->wscratch.get<float>();
        else
            k.weighted = ctx->wscratch.get<int64_t>();
    }
    const void *raw = phat ? (const void *)out->scores_f : (const void *)out->scores;
    // the refinement's peak scores: from the kernel (it keeps the scores on
    // chip) or from the raw scores around each peak
    const bool peak_k = ls && phat && tdoa_gcc_phat_peak3(ctx->kp);
    if (peak_k) {
        if (const int rc = ctx->tscratch.grow((size_t)B * ctx->t.P * 3 * sizeof(float), stream,
                                                    "peak-score"))
            return rc;
        k.peak3 = ctx->tscratch.get<float>();
    }
    if (ls && !raw && !peak_k) {  // the refinement reads the raw scores around each peak
        if (const int rc = ctx->rscratch.grow(pk, stream, "raw-score"))
            return rc;
        raw = ctx->rscratch.get<void>();
        if (phat)
            k.scores_f = ctx->rscratch.get<float>();
        else
            k.scores = ctx->rscratch.get<int64_t>();
    }
    if (ls && !out->cell) {
        if (const int rc = ctx->cscratch.grow((size_t)B * 4, stream, "cell"))
            return rc;
        k.cell = ctx->cscratch.get<int32_t>();
    }
    int rc = 0;
    if (compact && chunk < B) {
        rc = run_compact_chunks(ctx, k, frames, B, chunk, weighted, stream);
    } else {
        rc = phat ? tdoa_launch_gcc_phat(ctx->kp, k, frames, B, ctx->t.cfg.phat_eps, ctx->spec.get<void>(),
                                         ctx->spec.bytes(), stream)
                  : tdoa_launch_direct(ctx->kp, k, frames, B, prepared, stream, nullptr);
        if (rc != 0 || !grid)
            return rc;
        if (!fused_grid)
            rc = tdoa_launch_grid(ctx->kp, k, weighted, phat, B, stream);
    }
    if (rc != 0 || !ls)
        return rc;
    return tdoa_launch_ls(ctx->kp, raw, phat, k.peak3, k.lags, k.cell, out->xy_ls, out->ls_rms, B, stream);
}

extern "C" int tdoa_heatmap(tdoa_ctx *ctx, const void *weighted, const void *max_L, int is_float,
                            int64_t B, uint8_t *classes, void *stream)
{
    if (!ctx || !weighted || !max_L || !classes)
        return tdoa_fail(TDOA_ERR_INVALID, "tdoa_heatmap: NULL argument");
    if (B < 0)
        return tdoa_fail(TDOA_ERR_INVALID, "tdoa_heatmap: negative batch");
    HIP_TRY(hipSetDevice(ctx->device));
    return tdoa_launch_heatmap(ctx->kp, weighted, max_L, is_float != 0, B, classes, stream);
}

extern "C" int tdoa_peaks(tdoa_ctx *ctx, const void *scores, int is_float, int64_t B,
                          const tdoa_peaks_params *prm, const tdoa_peaks_outputs *out, void *stream)
{
    if (!ctx || !scores || !prm || !out)
        return tdoa_fail(TDOA_ERR_INVALID, "tdoa_peaks: NULL argument");
    if (!out->cell)
        return tdoa_fail(TDOA_ERR_INVALID, "tdoa_peaks: outputs.cell is required");
    if (B < 0)
        return tdoa_fail(TDOA_ERR_INVALID, "tdoa_peaks: negative batch");
    if (B > INT32_MAX)
        return tdoa_fail(TDOA_ERR_INVALID, "tdoa_peaks: batch too large for one launch");
    if (prm->num_peaks < 1 || prm->num_peaks > TDOA_MAX_PEAKS)
        return tdoa_fail(TDOA_ERR_INVALID, "tdoa_peaks: num_peaks %d outside 1..%d", (int)prm->num_peaks,
                    TDOA_MAX_PEAKS);
    if (prm->radius < 0)
        return tdoa_fail(TDOA_ERR_INVALID, "tdoa_peaks: negative radius");
    if (!tdoa_peaks_fits(ctx->kp, is_float != 0))
        return tdoa_fail(TDOA_ERR_INVALID, "tdoa_peaks: the L map and one frame's scores (%zu bytes) exceed the LDS budget",
                    tdoa_peaks_lds(ctx->kp, is_float != 0));
    if (B == 0)
        return TDOA_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    const int Kp = prm->num_peaks;
    const bool ls = out->xy_ls || out->ls_rms;
    tdoa_peaks_kout k;
    k.count = out->count;
    k.cell = out->cell;
    k.xy = out->xy;
    k.L = out->L;
    k.Lf = out->Lf;
    k.lags = out->lags;
    if (ls && !k.lags) {  // the refinement reads each peak's lag tuple
        if (const int rc = ctx->pscratch.grow((size_t)B * Kp * ctx->t.P * sizeof(int32_t), stream,
                                                    "peak-lag"))
            return rc;
        k.lags = ctx->pscratch.get<int32_t>();
    }
    int rc = tdoa_launch_peaks(ctx->kp, k, scores, is_float != 0, B, Kp, prm->radius, prm->min_rel, stream);
    if (rc != 0 || !ls)
        return rc;
    // B * Kp virtual frames: row f refines peak f % Kp of frame f / Kp
    return tdoa_launch_ls(ctx->kp, scores, is_float != 0, nullptr, k.lags, k.cell, out->xy_ls, out->ls_rms,
                          B * Kp, stream, Kp);
}

// accessors for the streaming pipeline (tdoa_stream.cpp)
const tdoa_kparams *tdoa_ctx_kparams(const tdoa_ctx *c) { return &c->kp; }
int tdoa_ctx_device(const tdoa_ctx *c) { return c->device; }
int tdoa_ctx_engine(const tdoa_ctx *c) { return c->t.cfg.engine; }
int tdoa_ctx_rate(const tdoa_ctx *c) { return c->t.cfg.sample_rate_hz; }
float tdoa_ctx_phat_eps(const tdoa_ctx *c) { return c->t.cfg.phat_eps; }

int tdoa_ctx_beam(const tdoa_ctx *c, const char *fn, tdoa_beam_geometry *g, int *Dmax, const float **fir)
{
    if (c->beam_dmax <= 0) {
        int d = 0;
        const int rc = tdoa_beam_dmax(c->beam_g, &d);  // stores the cause
        return rc ? rc : tdoa_fail(TDOA_ERR_INVALID, "%s: the context has no beamformer geometry", fn);
    }
    *g = c->beam_g;
    *Dmax = c->beam_dmax;
    *fir = c->beam_fir.get<float>();
    return TDOA_OK;
}

extern "C" int tdoa_beam_latency(const tdoa_ctx *ctx, int32_t *A, int32_t *Dmax)
{
    if (!ctx)
        return tdoa_fail(TDOA_ERR_INVALID, "tdoa_beam_latency: NULL ctx");
    return tdoa_beam_latency_of(&ctx->beam_g, A, Dmax);
}

extern "C" int tdoa_get_beam_geometry(const tdoa_ctx *ctx, tdoa_beam_geometry *g)
{
    if (!ctx || !g)
        return tdoa_fail(TDOA_ERR_INVALID, "tdoa_get_beam_geometry: NULL argument");
    *g = ctx->beam_g;
    return TDOA_OK;
}

// What tdoa_beam_batch and tdoa_sep_batch share, before and after their own
// argument checks: the context's beamformer geometry ...
static int batch_beam_open(tdoa_ctx *ctx, const char *fn, const int16_t *frames, const float *xy,
                           const tdoa_beam_outputs *out, tdoa_beam_geometry *g, int *Dmax, const float **fir)
{
    if (!ctx || !frames || !xy || !out)
        return tdoa_fail(TDOA_ERR_INVALID, "%s: NULL argument", fn);
    return tdoa_ctx_beam(ctx, fn, g, Dmax, fir);
}

// ... and the batch of B frames as a launch's source, the caller's xy as its targets
static int batch_beam_io(const char *fn, const int16_t *frames, int64_t B, const int32_t *count, const float *xy,
                         int32_t Kt, tdoa_beam_source *source, tdoa_beam_targets *targets)
{
    if (B < 0 || B >= ((int64_t)1 << 31))
        return tdoa_fail(TDOA_ERR_INVALID, "%s: B %lld outside [0, 2^31)", fn, (long long)B);
    *source = tdoa_beam_source{frames, true, 0, nullptr, B};
    *targets = tdoa_beam_targets{count, xy, nullptr, 0, Kt};
    return TDOA_OK;
}

extern "C" int tdoa_beam_batch(tdoa_ctx *ctx, const int16_t *frames, int64_t B, const int32_t *count,
                               const float *xy, int32_t Kt, const tdoa_beam_outputs *out, void *stream)
{
    tdoa_beam_geometry g;
    int Dmax = 0;
    const float *fir = nullptr;
    tdoa_beam_source source;
    tdoa_beam_targets targets;
    if (const int rc = batch_beam_open(ctx, "tdoa_beam_batch", frames, xy, out, &g, &Dmax, &fir))
        return rc;
    if (const int rc = tdoa_beam_check("tdoa_beam_batch", g, Dmax, ctx->t.N, Kt, out, out->audio, true))
        return rc;
    if (const int rc = batch_beam_io("tdoa_beam_batch", frames, B, count, xy, Kt, &source, &targets))
        return rc;
    if (B == 0)
        return TDOA_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    return tdoa_launch_beam(g, Dmax, source, ctx->t.N, targets, fir, *out, stream);
}

extern "C" int tdoa_sep_set_block(tdoa_ctx *ctx, int32_t L)
{
    if (!ctx)
        return tdoa_fail(TDOA_ERR_INVALID, "tdoa_sep_set_block: NULL ctx");
    tdoa_beam_geometry g;
    int Dmax = 0;
    const float *fir = nullptr;
    if (const int rc = tdoa_ctx_beam(ctx, "tdoa_sep_set_block", &g, &Dmax, &fir))
        return rc;
    if (const int rc = tdoa_sep_check("tdoa_sep_set_block", Dmax, L, 1, TDOA_SEP_LOADING, ctx, ctx))
        return rc;
    if (L == ctx->sep_L)
        return TDOA_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipDeviceSynchronize());  // launches in flight read the table this replaces
    return upload_sep(ctx, L);
}

extern "C" int tdoa_sep_get_block(const tdoa_ctx *ctx, int32_t *L)
{
    if (!ctx || !L)
        return tdoa_fail(TDOA_ERR_INVALID, "tdoa_sep_get_block: NULL argument");
    *L = ctx->sep_L;
    return TDOA_OK;
}

extern "C" int tdoa_sep_batch(tdoa_ctx *ctx, const int16_t *frames, int64_t B, const int32_t *count, const float *xy,
                              int32_t Kt, float loading, const tdoa_beam_outputs *out, void *stream)
{
    tdoa_beam_geometry g;
    int Dmax = 0;
    const float *fir = nullptr;
    tdoa_beam_source source;
    tdoa_beam_targets targets;
    if (const int rc = batch_beam_open(ctx, "tdoa_sep_batch", frames, xy, out, &g, &Dmax, &fir))
        return rc;
    if (ctx->sep_L == 0)
        return tdoa_fail(TDOA_ERR_INVALID, "tdoa_sep_batch: the context has no block length: frame_len %d is no "
                                           "power of two in 128..2048 with L >= 8 Dmax = %d (tdoa_sep_set_block "
                                           "chooses one)", ctx->t.N, 8 * Dmax);
    if (const int rc = tdoa_sep_check("tdoa_sep_batch", Dmax, ctx->sep_L, Kt, loading, out, out->audio))
        return rc;
    if (const int rc = batch_beam_io("tdoa_sep_batch", frames, B, count, xy, Kt, &source, &targets))
        return rc;
    if (B == 0)
        return TDOA_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    return tdoa_launch_sep(g, Dmax, source, ctx->sep_L, targets, loading, ctx->sep_tab.get<float>(), nullptr, *out,
                           stream);
}

extern "C" int tdoa_localize_batch(tdoa_ctx *ctx, const int16_t *frames, int64_t B,
                                   const tdoa_outputs *out, void *stream)
{
    return run_batch(ctx, frames, B, out, stream, false);
}

extern "C" int tdoa_correlate_prepared(tdoa_ctx *ctx, const int16_t *prepared, int64_t B,
                                       const tdoa_outputs *out, void *stream)
{
    return run_batch(ctx, prepared, B, out, stream, true);
}

extern "C" int tdoa_average_batch(tdoa_ctx *ctx, int64_t S, int64_t *est, const int64_t *fresh,
                                  const float *decay, int32_t *best, const tdoa_outputs *solve,
                                  void *stream)
{
    if (!ctx || !est || !fresh || !decay || !best)
        return tdoa_fail(TDOA_ERR_INVALID, "tdoa_average_batch: NULL argument");
    if (S < 0)
        return tdoa_fail(TDOA_ERR_INVALID, "tdoa_average_batch: negative stream count");
    if (S == 0)
        return TDOA_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    tdoa_kout k;
    const tdoa_kout *kptr = nullptr;
    if (solve) {
        k = to_kout(solve);
        kptr = &k;
    }
    return tdoa_launch_average(ctx->kp, S, est, fresh, decay, best, kptr, stream);
}

// correlations.c:40-43
extern "C" float tdoa_decay_us(uint64_t now_us, uint64_t last_us)
{
    const float dt = (float)(now_us - last_us) / 1e6f;
    const float arg = -dt / 0.5f;
    return (float)(1.0 - std::exp((double)arg));
}

extern "C" int tdoa_get_window(const tdoa_ctx *c, int32_t *w)
{
    if (!c || !w)
        return tdoa_fail(TDOA_ERR_INVALID, "NULL");
    std::memcpy(w, c->t.win.data(), sizeof(int32_t) * c->t.N);
    return TDOA_OK;
}

extern "C" int tdoa_get_mics(const tdoa_ctx *c, float *xy)
{
    if (!c || !xy)
        return tdoa_fail(TDOA_ERR_INVALID, "NULL");
    std::memcpy(xy, c->t.mic.data(), sizeof(float) * 2 * c->t.M);
    return TDOA_OK;
}

extern "C" int tdoa_get_lut(const tdoa_ctx *c, uint8_t *lut)
{
    if (!c || !lut)
        return tdoa_fail(TDOA_ERR_INVALID, "NULL");
    std::memcpy(lut, c->t.lut.data(), c->t.lut.size());
    return TDOA_OK;
}

extern "C" int tdoa_get_prior(const tdoa_ctx *c, float *scale)
{
    if (!c || !scale)
        return tdoa_fail(TDOA_ERR_INVALID, "NULL");
    std::memcpy(scale, c->t.prior.data(), sizeof(float) * c->t.K);
    return TDOA_OK;
}

// ---------------------------------------------------- band-limited GCC_PHAT
extern "C" int tdoa_set_bin_weights(tdoa_ctx *ctx, const float *w)
{
    if (!ctx)
        return tdoa_fail(TDOA_ERR_INVALID, "tdoa_set_bin_weights: NULL ctx");
    if (ctx->t.cfg.engine != TDOA_ENGINE_GCC_PHAT)
        return tdoa_fail(TDOA_ERR_INVALID, "tdoa_set_bin_weights: the context's engine is not GCC_PHAT");
    if (!w) {  // back to the shape's own route; the scratch stays until tdoa_destroy
        ctx->bin_w.clear();
        ctx->kp.bin_w = nullptr;
        ctx->kp.bin_lo = ctx->kp.bin_hi = 0;
        return TDOA_OK;
    }
    const int n = ctx->t.N + 1;
    int lo = -1, hi = -1;
    for (int k = 0; k < n; k++) {
        if (!std::isfinite(w[k]) || w[k] < 0.0f)
            return tdoa_fail(TDOA_ERR_INVALID, "tdoa_set_bin_weights: w[%d] is negative or not finite", k);
        if (w[k] != 0.0f) {
            lo = lo < 0 ? k : lo;
            hi = k;
        }
    }
    if (lo < 0)
        return tdoa_fail(TDOA_ERR_INVALID, "tdoa_set_bin_weights: every weight is zero");
    HIP_TRY(hipSetDevice(ctx->device));
    // shapes whose own route needs no spectrum scratch get it here
    if (!ctx->spec && ctx->spec.alloc(TDOA_SPEC_BYTES) != hipSuccess)
        return tdoa_fail(TDOA_ERR_NOMEM, "GCC_PHAT spectrum scratch of %zu bytes", TDOA_SPEC_BYTES);
    if (!ctx->d_bin_w && ctx->d_bin_w.alloc(sizeof(float) * n) != hipSuccess)
        return tdoa_fail(TDOA_ERR_NOMEM, "tdoa_set_bin_weights: weight table of %d floats", n);
    // no call of the context is in flight (include/tdoa.h): nothing reads d_bin_w now
    HIP_TRY(ctx->d_bin_w.upload(w, sizeof(float) * n));
    ctx->bin_w.assign(w, w + n);
    ctx->kp.bin_w = ctx->d_bin_w.get<float>();
    ctx->kp.bin_lo = lo;
    ctx->kp.bin_hi = hi;
    return TDOA_OK;
}

extern "C" int tdoa_set_band_hz(tdoa_ctx *ctx, double lo_hz, double hi_hz, double taper_hz)
{
    if (!ctx)
        return tdoa_fail(TDOA_ERR_INVALID, "tdoa_set_band_hz: NULL ctx");
    std::vector<float> w((size_t)ctx->t.N + 1);
    const int rc = tdoa_band_weights(ctx->t.N, ctx->t.cfg.sample_rate_hz, lo_hz, hi_hz, taper_hz, w.data());
    return rc ? rc : tdoa_set_bin_weights(ctx, w.data());
}

extern "C" int tdoa_get_bin_weights(const tdoa_ctx *c, float *w)
{
    if (!c || !w)
        return tdoa_fail(TDOA_ERR_INVALID, "NULL");
    if (c->bin_w.empty())
        std::fill(w, w + c->t.N + 1, 1.0f);
    else
        std::memcpy(w, c->bin_w.data(), sizeof(float) * c->bin_w.size());
    return TDOA_OK;
}


// ------------------------------------------------------- 16-bit PCM input
extern "C" int tdoa_set_sample_format(tdoa_ctx *ctx, int format)
{
    if (!ctx)
        return tdoa_fail(TDOA_ERR_INVALID, "tdoa_set_sample_format: NULL ctx");
    if (format != TDOA_SAMPLES_ADC8 && format != TDOA_SAMPLES_PCM16)
        return tdoa_fail(TDOA_ERR_INVALID, "tdoa_set_sample_format: unknown format %d", format);
    if (format == TDOA_SAMPLES_PCM16) {
        if (ctx->t.cfg.engine != TDOA_ENGINE_GCC_PHAT)
            return tdoa_fail(TDOA_ERR_INVALID, "tdoa_set_sample_format: PCM16 needs a GCC_PHAT context");
        // a shape without a fused PCM16 kernel takes the two-pass route: a
        // context whose 8-bit kernel is fused gets the spectrum scratch here
        const bool fused = tdoa_phat1024_fits(ctx->kp) ||
                           (tdoa_phat_r16_fits(ctx->kp.M, ctx->kp.N, ctx->kp.S) && frame16_shape(ctx->kp));
        if (!fused && !ctx->spec) {
            HIP_TRY(hipSetDevice(ctx->device));
            if (ctx->spec.alloc(TDOA_SPEC_BYTES) != hipSuccess)
                return tdoa_fail(TDOA_ERR_NOMEM, "GCC_PHAT spectrum scratch of %zu bytes", TDOA_SPEC_BYTES);
        }
    }
    ctx->kp.pcm16 = format == TDOA_SAMPLES_PCM16 ? 1 : 0;
    return TDOA_OK;
}

extern "C" int tdoa_get_sample_format(const tdoa_ctx *ctx, int *format)
{
    if (!ctx || !format)
        return tdoa_fail(TDOA_ERR_INVALID, "tdoa_get_sample_format: NULL argument");
    *format = ctx->kp.pcm16 ? TDOA_SAMPLES_PCM16 : TDOA_SAMPLES_ADC8;
    return TDOA_OK;
}

extern "C" const char *tdoa_batch_kernel(const tdoa_ctx *ctx)
{
    if (!ctx)
        return "";
    if (ctx->t.cfg.engine == TDOA_ENGINE_GCC_PHAT)
        return tdoa_gcc_phat_kernel_name(ctx->kp);
    return tdoa_direct_fused_grid(ctx->kp) ? "k_direct_mfma" : "k_direct";
}

extern "C" int tdoa_batch_grid_fused(const tdoa_ctx *ctx)
{
    if (!ctx)
        return 0;
    return (ctx->t.cfg.engine == TDOA_ENGINE_GCC_PHAT ? tdoa_gcc_phat_grid_in_kernel(ctx->kp)
                                                    : tdoa_direct_fused_grid(ctx->kp))
               ? 1
               : 0;
}

extern "C" int tdoa_abi_version(void) { return TDOA_ABI_VERSION; }

