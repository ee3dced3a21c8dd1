/*
 * tdoa.h -- batched C ABI of the MI355X TDOA localizer (libtdoa.so).
 *
 * The reference (yuan-xy/Audio-Triangulation) processes one 3-mic frame at a
 * time inside protothread_sample_and_compute (src/sample_compute.h:105-139)
 * and solves the position on a 101x101 grid in vga_draw_heatmap
 * (src/components/vga/vga_heatmap.h:95-108).  This header is the batched,
 * error-returning form of that path: one call runs, for B frames at once,
 *
 *   rolling_buffer_write_out DC removal  rolling_buffer.c:64-66
 *   buffer_normalize_range (<<8 wrap)     buffer.c:13-18
 *   buffer_window (Q15 DPSS NW=2)         buffer.c:4-11, window.ipynb:43-60
 *   correlations_init (scores, argmax,    correlations.c:4-36
 *                      Gaussian lag prior)
 *   shift gate sum(best^2) > 4            sample_compute.h:124-134
 *   grid L = sum_p corr_p[LUT_p] max pass vga_heatmap.h:48-108
 *
 * as hand-written gfx950 kernels.  The per-frame reference symbols live in
 * tdoa_reference_abi.h and are implemented on top of this API.
 *
 * Conventions: all pointers in tdoa_outputs and the frames pointer of
 * tdoa_localize_batch are DEVICE pointers on the context's device; `stream`
 * is a hipStream_t (NULL = default stream).  Every function returns
 * TDOA_OK (0) or a negative tdoa_status; tdoa_last_error() describes the
 * last failure on the calling thread.  A context is bound to one device and
 * is not thread-safe: use one context per host thread / GPU.
 */
#ifndef TDOA_H
#define TDOA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TDOA_ABI_VERSION 1
#define TDOA_MAX_MICS 8

typedef enum tdoa_status {
    TDOA_OK = 0,
    TDOA_ERR_INVALID = -1,   /* bad argument / config */
    TDOA_ERR_HIP = -2,       /* HIP runtime error (message in tdoa_last_error) */
    TDOA_ERR_NO_DEVICE = -3, /* no gfx950 device visible */
    TDOA_ERR_NOMEM = -4
} tdoa_status;

typedef enum tdoa_engine {
    /* Exact integer time-domain cross-correlation: the reference's
     * correlations_init semantics bit-for-bit (int64 scores). */
    TDOA_ENGINE_DIRECT = 0,
    /* Generalised cross-correlation with PHAT weighting (fp32 radix-4 FFT,
     * |X| normalised cross-spectrum, inverse FFT), the north-star
     * formulation.  Float scores; lags equal DIRECT's on clean integer
     * delays, otherwise checked against a float64 GCC-PHAT oracle. */
    TDOA_ENGINE_GCC_PHAT = 1
} tdoa_engine;

typedef struct tdoa_config {
    int32_t num_mics;        /* M, 2..TDOA_MAX_MICS              (reference: 3) */
    int32_t frame_len;       /* N, power of two 256..4096        (buffer.h:5-6: 1024) */
    int32_t sample_rate_hz;  /* fs                               (constants.h:10: 50000) */
    int32_t max_shift;       /* <= 0 -> fs*32/34300              (constants.h:12: 46) */
    float speed_of_sound;    /* m/s                              (constants.h:14: 343) */
    int32_t engine;          /* tdoa_engine */
    /* mic positions [M][2] in metres; NULL -> microphones_init()'s triangle
     * (microphones.c:9-33) for M == 3, otherwise required. Copied. */
    const float *mic_xy;
    /* grid (vga.h:29-35, vga_heatmap.h:2-3): (2*half_w+1) x (2*half_h+1)
     * cells at grid_scale cells per metre, projected on a hemisphere of
     * radius height_offset. */
    int32_t grid_half_w;     /* 50 */
    int32_t grid_half_h;     /* 50 */
    float grid_scale;        /* 24.0f */
    float height_offset;     /* 1.2f */
    /* Q15 window [N]; NULL -> the reference's table: for N <= 1024 the
     * 1024-point DPSS(NW=2) table (window_function.h) subsampled as
     * buffer.c:8 indexes it, W[i << (10 - log2 N)]; for N > 1024 (where
     * buffer.c:8 is undefined) DPSS(N, NW=2) normalised to max 1, x32767,
     * rounded (window.ipynb procedure).  Copied. */
    const int32_t *window_q15;
    /* GCC_PHAT: per-mic soft floor, U_m = X_m / sqrt(|X_m|^2 + phat_eps),
     * R_ij = conj(U_i) U_j, with samples scaled by 2^-15 and X the 2N-point
     * spectrum; default 1e-12.  The scale is 2^-15 in both sample formats
     * (tdoa_set_sample_format) and TDOA_SAMPLES_PCM16 has no << 8: a frame of
     * 8-bit-sized samples is 256 times smaller there than in TDOA_SAMPLES_ADC8,
     * so the same phat_eps floors it 2^16 times harder in |X|^2. */
    float phat_eps;
} tdoa_config;

/* Per-frame results (device pointers; any may be NULL unless noted). */
typedef struct tdoa_outputs {
    int32_t *lags;           /* [B][P] best shift per pair (required)       */
    uint8_t *gate;           /* [B] sum_p lag^2 > 4 (sample_compute.h:134)   */
    int32_t *cell;           /* [B] first row-major argmax cell of L         */
    float *xy;               /* [B][2] ((x-hw)/scale, (hh-y)/scale) metres   */
    int64_t *max_L;          /* [B] DIRECT: max of L (vga_heatmap.h:99-108)  */
    float *max_Lf;           /* [B] GCC_PHAT: max of L                       */
    int64_t *scores;         /* [B][P][K] DIRECT raw int64 scores (debug)    */
    int64_t *weighted;       /* [B][P][K] DIRECT scores after the lag prior  */
    float *scores_f;         /* [B][P][K] GCC_PHAT raw correlation (debug)   */
    float *weighted_f;       /* [B][P][K] GCC_PHAT after the lag prior       */
    /* Least-squares refinement of the grid argmax (extension; absent in the
     * reference): sub-sample lags (parabolic vertex of the raw scores) fitted
     * by 10 Levenberg-Marquardt steps in double precision on the LUT's
     * hemisphere geometry, starting at the argmax cell, clamped to the grid. */
    float *xy_ls;            /* [B][2] refined (x, y) metres, grid frame     */
    float *ls_rms;           /* [B] rms lag residual (samples)               */
} tdoa_outputs;

typedef struct tdoa_ctx tdoa_ctx;

/* Fills the reference defaults (3 mics, 1024, 50 kHz, 46, DIRECT, ...). */
int tdoa_config_default(tdoa_config *cfg);

/* Validates cfg, builds the window, mic geometry, lag prior table and the
 * grid LUT on the host, uploads them to `device`. */
int tdoa_create(const tdoa_config *cfg, int device, tdoa_ctx **out);
int tdoa_destroy(tdoa_ctx *ctx);

/* Derived sizes of a context. */
int tdoa_get_dims(const tdoa_ctx *ctx, int32_t *M, int32_t *N, int32_t *P,
                  int32_t *K, int32_t *G);

/* Stateless batch: frames = device int16 [B][M][N] raw (pre-DC) samples, mic
 * rows contiguous.  Asynchronous on `stream`. */
int tdoa_localize_batch(tdoa_ctx *ctx, const int16_t *frames, int64_t B,
                        const tdoa_outputs *out, void *stream);

/* Same as tdoa_localize_batch for frames that already went through DC
 * removal, normalisation and the window (the inputs correlations_init sees).
 * Used by the per-frame reference symbols. */
int tdoa_correlate_prepared(tdoa_ctx *ctx, const int16_t *prepared, int64_t B,
                            const tdoa_outputs *out, void *stream);

/* Temporal averaging (correlations.c:38-63) for S independent streams:
 * est[S][P][K] (device, in/out) <- (int64)((float)est + (float)(fresh-est)*decay[s]),
 * best[S][P] re-argmaxed.  decay (device float[S]) comes from
 * tdoa_decay_us on the host.  If solve is non-NULL the grid solve runs on the
 * averaged scores (the reference solves on corr_*, vga_heatmap.h:102-104). */
int tdoa_average_batch(tdoa_ctx *ctx, int64_t S, int64_t *est,
                       const int64_t *fresh, const float *decay, int32_t *best,
                       const tdoa_outputs *solve, void *stream);

/* Heat-map classes of vga_draw_heatmap's colouring pass (vga_heatmap.h:
 * 110-130) for B frames: classes[B][G] = 4 (white, L >= (max*63)>>6),
 * 3 (green, (max*31)>>5), 2 (red, (max*15)>>4), 1 (blue, (max*7)>>3), else 0,
 * L = sum_p weighted_p[LUT_p].  weighted [B][P][K] and max_L [B] are device
 * int64 (is_float = 0; the reference's integer thresholds) or float
 * (is_float = 1; max * n / 2^b), e.g. a localize call's weighted / max_L
 * outputs or EMA scores with their grid max.  B <= 65535. */
int tdoa_heatmap(tdoa_ctx *ctx, const void *weighted, const void *max_L, int is_float,
                 int64_t B, uint8_t *classes, void *stream);

/* ---- Multiple sources: the top peaks of the likelihood map ----
 * tdoa_localize_batch reports one cell per frame, the first row-major argmax
 * of L(cell) = sum_p score_p[LUT_p(cell)].  tdoa_peaks reports up to
 * num_peaks maxima of the same map by greedy suppression, per frame:
 *   1. L[c] for every cell, in T = int64 or fp32, the pairs added in
 *      ascending p, one add per pair (as tdoa_heatmap evaluates it);
 *   2. up to num_peaks times: take the maximum L among the cells not yet
 *      suppressed, ties to the lowest cell index.  Peak 0 is always reported.
 *      Peak k >= 1 is reported only if a cell remains and, for min_rel > 0,
 *      (double)L_k >= (double)min_rel * (double)L_0; the first peak that is
 *      not reported ends the search.  Then every cell with |cx - px| <= radius
 *      and |cy - py| <= radius is suppressed.
 * With num_peaks = 1 on a localize call's weighted block the result is that
 * call's cell / xy / max_L (max_Lf).
 *
 * scores is a device [B][P][K] block, int64 (is_float = 0) or float
 * (is_float = 1).  Which block gives which meaning:
 *   scores / scores_f      the raw correlations: every source keeps its own
 *                          peak in every pair, so this is the block for
 *                          several simultaneous sources;
 *   weighted / weighted_f  after the Gaussian lag prior centred on each
 *                          pair's best lag: the map the reference displays
 *                          (vga_heatmap.h), with the strongest source
 *                          emphasised and the others damped by the prior;
 *   the EMA scores of tdoa_average_batch (int64): the time-averaged map.
 * A context whose batch route solves the grid inside its first kernel
 * (tdoa_batch_grid_fused) or keeps the scores on chip writes these blocks
 * only when the caller requests them in tdoa_outputs.
 * NaN float scores: which cells are reported is unspecified; every cell
 * written is in range or -1.
 *
 * xy_ls / ls_rms: the least-squares refinement of tdoa_outputs started at
 * each peak, with the peak's lag tuple LUT_p(cell) - S in place of the
 * pairs' argmax lags: tau_p = lag_p + the parabolic vertex of the given
 * score block at lag_p - 1 .. lag_p + 1 (none at the ends of the lag range
 * or where the three scores have no maximum).
 *
 * Asynchronous on `stream`; no host synchronisation and no allocation once
 * the context's scratch has grown (it is used when xy_ls / ls_rms are
 * requested without lags).  As for every call that may use the context's
 * scratch: one stream per context while a call is in flight. */
#define TDOA_MAX_PEAKS 8

typedef struct tdoa_peaks_params {
    int32_t num_peaks;   /* Kp, 1..TDOA_MAX_PEAKS */
    int32_t radius;      /* suppression half-width in cells, >= 0 (Chebyshev square) */
    float   min_rel;     /* > 0: peak k >= 1 is kept only if (double)L_k >= (double)min_rel * (double)L_0;
                            <= 0: no threshold */
} tdoa_peaks_params;

typedef struct tdoa_peaks_outputs {  /* device pointers; any may be NULL except cell */
    int32_t *count;   /* [B] peaks found, 1..Kp */
    int32_t *cell;    /* [B][Kp] row-major cell, -1 in slots >= count (required) */
    float   *xy;      /* [B][Kp][2] as tdoa_outputs.xy; NaN in empty slots */
    int64_t *L;       /* [B][Kp] is_float == 0: L at the peak; INT64_MIN in empty slots */
    float   *Lf;      /* [B][Kp] is_float == 1: L at the peak; -inf in empty slots */
    int32_t *lags;    /* [B][Kp][P] LUT_p(cell) - S: the peak's lag tuple; 0 in empty slots */
    float   *xy_ls;   /* [B][Kp][2] least-squares refinement started at the peak; NaN in empty slots */
    float   *ls_rms;  /* [B][Kp] NaN in empty slots */
} tdoa_peaks_outputs;

/* TDOA_ERR_INVALID: a NULL ctx / scores / prm / out / out->cell, B < 0,
 * num_peaks outside 1..TDOA_MAX_PEAKS, radius < 0, B >= 2^31, or a
 * grid whose L map plus one frame's scores exceed the kernel's 150 KiB of LDS
 * ((P*K + G) * sizeof(T)).  B = 0 returns TDOA_OK without a launch. */
int tdoa_peaks(tdoa_ctx *ctx, const void *scores, int is_float, int64_t B,
               const tdoa_peaks_params *prm, const tdoa_peaks_outputs *out, void *stream);

/* ---- Band-limited GCC_PHAT: per-bin weights on the cross spectrum ----
 * PHAT gives every bin of the 2N-point spectrum the same vote whatever its
 * energy, so a source that occupies part of the band loses to anything
 * broadband elsewhere in it.  A weight table w[0..N] (real, finite, >= 0; bin k
 * is f_k = k * fs / 2N) changes the definition to
 *     R_ij[k] = w[k] * conj(U_i[k]) U_j[k],   r_ij = irfft(R_ij, 2N)
 * and nothing else: lags, prior, gate, grid, least squares, heat map and
 * tdoa_peaks are defined on these scores as before.  There is no
 * renormalisation: a band that keeps a fraction q of the bins scales the peak
 * of a clean delay, and with it max_Lf and the peak values, to about q
 * (min_rel of tdoa_peaks is relative and unaffected).
 *
 * While a table is set, a tdoa_localize_batch of the context runs the two-pass
 * kernels (k_phat_spectra, then k_phat_pairs<true>) for every shape, through a
 * spectrum scratch of the context: tdoa_batch_kernel names the first of them
 * and tdoa_batch_grid_fused returns 0 -- one stream per context while a call
 * is in flight.  Without a table (never set, or cleared with NULL) the context
 * runs exactly the kernels, and computes exactly the bits, it does without
 * this section.  tdoa_correlate_prepared runs the integer path on any context
 * and the per-frame reference symbols (tdoa_reference_abi.h) have contexts of
 * their own: neither is affected by a table. */

/* Host only, no device: w[k] = 1 for lo <= f_k <= hi; with taper > 0 a raised
 * cosine outside, 0.5 (1 - cos(pi (f_k - (lo - taper)) / taper)) for
 * lo - taper < f_k < lo and 0.5 (1 + cos(pi (f_k - hi) / taper)) for
 * hi < f_k < hi + taper; 0 elsewhere.  Double arithmetic, rounded to float.
 * TDOA_ERR_INVALID unless 0 <= lo < hi <= fs/2, taper >= 0, N a power of two
 * in 256..4096 and at least one bin gets a non-zero weight. */
int tdoa_band_weights(int32_t N, int32_t fs, double lo_hz, double hi_hz, double taper_hz,
                      float *w /* [N+1] */);
/* Sets (w = host [N+1]) or clears (w = NULL) the context's table.
 * Synchronous: copies the table to the device, and on first use allocates the
 * spectrum scratch (128 MiB, as tdoa_create does for the two-pass shapes;
 * freed by tdoa_destroy) if the context has none.  Must not be called while a
 * call on the context is in flight.  TDOA_ERR_INVALID for a DIRECT context, a
 * non-finite or negative entry, or an all-zero table; the table in force
 * stays. */
int tdoa_set_bin_weights(tdoa_ctx *ctx, const float *w);
/* tdoa_band_weights with the context's N and fs, then tdoa_set_bin_weights. */
int tdoa_set_band_hz(tdoa_ctx *ctx, double lo_hz, double hi_hz, double taper_hz);
/* Host copy of the table in force; all 1.0f when none is set. */
int tdoa_get_bin_weights(const tdoa_ctx *ctx, float *w /* [N+1] */);

/* ---- 16-bit PCM input (GCC_PHAT) ----
 * The default front end is the firmware's 8-bit ADC path: (x - off) << 8 in
 * int16 keeps the low byte of every sample.  TDOA_SAMPLES_PCM16 takes
 * full-range int16 frames instead.  Per mic row x[0..N):
 *   off  = floor(sum(x) / N)             arithmetic shift; off in [-32768, 32767]
 *   y[n] = x[n] - off                    int32, no wrap; |y| <= 65535
 *   s[n] = (y[n] * W[n]) >> 15           int32 arithmetic shift (floor), W the Q15 window
 * and s enters the FFT where the 8-bit prepared sample does, in the same
 * units (x = s / 2^15): phat_eps, the lag rule, prior, gate, grid, least
 * squares, peaks and the heat map are defined on the scores and do not change.
 * Kernels: 3 x 1024 runs the fused k_p1k_pcm16 (it solves the grid: one HIP
 * stream per context is not required, two streams may overlap as with
 * k_p1k_lean); 4 x 2048, 8 x 2048, 3 x 4096 and 4 x 4096 run k_f16_pcm16;
 * every other shape, and every shape with a bin-weight table, runs the
 * two-pass route (k_phat_spectra_pcm16, k_phat_pairs).  A/B switches that pick
 * other kernels (TDOA_P1K, TDOA_F16, TDOA_F16_FG) are ignored in this format. */
typedef enum tdoa_sample_format {
    TDOA_SAMPLES_ADC8 = 0,  /* default: the reference's 8-bit path, every kernel and bit as without this section */
    TDOA_SAMPLES_PCM16 = 1  /* full-range int16, the definition above; GCC_PHAT only */
} tdoa_sample_format;
/* Synchronous; must not be called while a call on the context is in flight.
 * TDOA_ERR_INVALID for a NULL ctx, an unknown value, or PCM16 on a DIRECT
 * context: the format in force stays.  ADC8 is accepted on any context and
 * returns it to the kernels and bits it produced before.  A shape whose 8-bit
 * kernel is fused but whose PCM16 route has two passes gets the spectrum
 * scratch (128 MiB, freed by tdoa_destroy) on first need, as
 * tdoa_set_bin_weights does.  tdoa_correlate_prepared and the per-frame
 * reference symbols run the integer path whatever the format.  A streaming
 * pipeline takes its format at creation and keeps it whatever the context is
 * switched to afterwards: tdoa_stream_create takes 8-bit capture rings and is
 * TDOA_ERR_INVALID on a PCM16 context, tdoa_stream_create_pcm16 (below) takes
 * int16 rings and is TDOA_ERR_INVALID on an ADC8 one. */
int tdoa_set_sample_format(tdoa_ctx *ctx, int format);
int tdoa_get_sample_format(const tdoa_ctx *ctx, int *format);

/* Host helper: decay of correlations.c:42-43 from integer-us timestamps. */
float tdoa_decay_us(uint64_t now_us, uint64_t last_us);

/* Host copies of the context's tables (for tests / tooling). */
int tdoa_get_window(const tdoa_ctx *ctx, int32_t *window /* [N] */);
int tdoa_get_mics(const tdoa_ctx *ctx, float *mic_xy /* [M][2] */);
int tdoa_get_lut(const tdoa_ctx *ctx, uint8_t *lut /* [P][G] */);
int tdoa_get_prior(const tdoa_ctx *ctx, float *scale /* [K] by |d| */);

/* DPSS(N, NW) first Slepian taper, Q15 as in window.ipynb. */
int tdoa_dpss_q15(int32_t n, double nw, int32_t *out);

/* ---- Streaming pipeline (sample_compute.h:53-146; BASELINE config 5) ----
 * S independent mic-array streams whose 8-bit ADC bytes (dma_sampler.c:17-23:
 * one u8 per mic, round-robin; read as sample_t at sample_compute.h:67-73)
 * land in a device capture ring capture[S][capture_len][M].  Each
 * tdoa_stream_step consumes the next `hop` samples of every stream:
 *   trigger   after every sample, once N samples arrived since the stream's
 *             last trigger (the rings restart empty, sample_compute.h:55-57),
 *             fire when sum_m outgoing > 2 << 2(log2 N - 1) + sum_m incoming
 *             (rolling_buffer.c:16-41,73-85; sample_compute.h:75-91), first
 *             firing sample of the hop;
 *   frame     the N samples before it through the DIRECT path (write_out,
 *             normalize, window, xcorr, prior, gate);
 *   EMA       gated frames only: correlations.c:38-63 on the stream's scores
 *             with the clock now_us = end * 1e6 / fs (end = samples consumed
 *             at the trigger; the EMA clock starts at 0 like corr_*'s static
 *             zero init), then the grid solve on the EMA scores (the VGA
 *             thread solves on corr_*, vga_heatmap.h:99-108).
 * The step is a fixed kernel sequence reading its position from a device
 * clock, so with use_graph it is captured once into a hipGraph and replayed.
 * The producer keeps capture_len >= N + 2*hop samples of history per stream.
 * hop <= N.
 *
 * A GCC_PHAT context streams too: the same trigger, then per triggered frame
 * the GCC-PHAT scores as tdoa_localize_batch defines them (the integer front
 * end, U_m = X_m / sqrt(|X_m|^2 + phat_eps), r_ij = irfft(w conj(U_i) U_j),
 * first maximum, lag prior, gate), with the per-bin weight table in force on
 * the context at each step (tdoa_set_bin_weights / tdoa_set_band_hz: set it
 * only while no step is in flight).  The EMA state is float:
 *     est <- est + (fresh - est) * decay(now_us, last_us)     (fp32)
 * on gated frames, and the grid solve runs on it in float (max_Lf).  Such a
 * pipeline steps with tdoa_stream_step_f and is read with
 * tdoa_stream_state_f; tdoa_stream_step, and tdoa_stream_state with a non-NULL
 * est, return TDOA_ERR_INVALID on it, as the _f forms do on a DIRECT one.
 * Accepted GCC_PHAT shapes: M * N * 8 + N * 8 + 2 * P * K * 4 bytes of LDS
 * within 160 KiB (4 mics up to frame_len 2048, 8 mics up to 1024, 3 mics up to
 * 4096, ...: kernel k_stream_phat), and the two long-frame shapes beyond that
 * rule which the batch engine's per-frame kernel holds, 8 mics x 2048 and
 * 4 mics x 4096: there the hop is k_f16_ring (that kernel's body over the
 * step's listed frames, staged from the capture rings; its scores are the batch
 * call's for the same frame, and the weight table in force applies as above)
 * followed by k_stream_ema_grid (record, EMA, grid solve).  Records, state,
 * tdoa_stream_peaks and tdoa_stream_track are the same on either route; at the
 * two long-frame shapes a stream's ring (capture_len * M samples) must stay
 * under 2^31 bytes.  Other shapes (8 mics x 4096, ...) are TDOA_ERR_INVALID.
 * tdoa_stream_kernel names the route.  TDOA_STREAM_PHAT_GRID=n in the
 * environment at tdoa_stream_create caps the GCC_PHAT kernels' launch sizes
 * (A/B runs). */
typedef struct tdoa_stream tdoa_stream;

typedef struct tdoa_stream_outputs { /* device pointers; slot order is arbitrary */
    int32_t *count;     /* [1] frames triggered this step: slots 0..count-1 */
    int32_t *stream_id; /* [S] stream of each slot                           */
    int64_t *end;       /* [S] samples consumed at the trigger (frame = [end-N, end)) */
    int32_t *lags;      /* [S][P] best lags of the fresh frame               */
    uint8_t *gate;      /* [S] sum_p lag^2 > 4                               */
    int32_t *ema_best;  /* [S][P] EMA best lags (gated slots)                */
    int32_t *cell;      /* [S] grid argmax on the EMA scores; -1 if not gated */
    float *xy;          /* [S][2] (gated slots)                              */
    int64_t *max_L;     /* [S] (gated slots)                                 */
} tdoa_stream_outputs;

typedef struct tdoa_stream_outputs_f { /* the same for a GCC_PHAT pipeline */
    int32_t *count;
    int32_t *stream_id;
    int64_t *end;
    int32_t *lags;
    uint8_t *gate;
    int32_t *ema_best;
    int32_t *cell;
    float *xy;
    float *max_Lf;      /* [S] (gated slots)                                 */
} tdoa_stream_outputs_f;

int tdoa_stream_create(tdoa_ctx *ctx, int32_t num_streams, int32_t hop,
                       const uint8_t *capture, int64_t capture_len, int use_graph,
                       tdoa_stream **out);

/* ---- Streaming 16-bit PCM capture rings (GCC_PHAT in TDOA_SAMPLES_PCM16) ----
 * capture[S][capture_len][M] holds int16 samples (2-byte aligned; a stream's
 * ring starts at s * capture_len * M * 2 bytes).  The trigger is the one above
 * on int16 samples with a caller-supplied threshold.  For stream s, samples
 * x_m[t] (zero for t < 0), h = N/2, pos the samples consumed before the hop:
 *   a candidate end e lies in (pos, pos + hop] and is eligible iff
 *   e - ring_start[s] >= N;  older half O = [e-N, e-h), newer half I = [e-h, e);
 *   pw(m, R) = h * sum_R x_m^2 - (sum_R x_m)^2, exact in int64;
 *   the stream fires iff sum_m pw(m, O) > trigger_var * h^2 + sum_m pw(m, I);
 *   the first eligible firing e of the hop is taken, then ring_start[s] = e
 *   (ring_start starts at 0).
 * The 8-bit trigger is this rule with trigger_var = 2.  trigger_var is in
 * counts^2, in [0, 2^30]; with TDOA_STREAM_TRIGGER_VAR_PCM16 = 2 * 256^2 a ring
 * holding (u8 - 128) * 256 fires exactly where the 8-bit ring does (both sides
 * scale by 65536 and a DC shift cancels in pw).
 * Int64 bounds over every accepted shape (|x| <= 2^15, h <= 2048, M <= 8):
 * |sum_R x| <= h 2^15 = 2^26, so (sum_R x)^2 <= 2^52; sum_R x^2 <= h 2^30 and
 * h * sum_R x^2 <= 2^52; 0 <= pw <= 2^52 (Cauchy-Schwarz), over 8 mics each
 * side's sum <= 2^55; trigger_var * h^2 <= 2^30 * 2^22 = 2^52; the kernel's
 * prefix sums of x over the N + hop - 1 <= 8191 samples it reads stay below
 * 2^28 < 2^31 (int32) and those of x^2 below 2^43.
 * Each triggered frame x[e-N, e) goes through the PCM16 front end as defined
 * above (off = floor(mean), y = x - off, s = (y W) >> 15) and from there on
 * through what a GCC_PHAT pipeline does with an 8-bit frame: PHAT with
 * phat_eps, the context's bin-weight table read at every step, the inverses,
 * first maximum, prior, gate, the float EMA on gated frames with
 * now_us = e * 1e6 / fs, and the grid solve on the EMA scores.
 * The result is an ordinary tdoa_stream: it steps with tdoa_stream_step_f, is
 * read with tdoa_stream_state_f (and tdoa_stream_state with est = NULL), and
 * tdoa_stream_reset / tdoa_stream_destroy apply; graph mode and plain stream
 * launches both work.  Kernels: k_stream_trigger16, k_stream_phat_pcm16 (at
 * 8 mics x 2048 and 4 mics x 4096: k_f16_ring on the int16 ring, then
 * k_stream_ema_grid).
 * TDOA_ERR_INVALID, with tdoa_last_error naming the cause: a DIRECT context; a
 * GCC_PHAT context in ADC8 format; trigger_var outside [0, 2^30]; hop outside
 * [1, N]; capture_len < N + 2 hop; a shape outside the GCC_PHAT shapes above
 * (the LDS rule and the two long-frame shapes) or whose trigger needs more than
 * 150 KiB of LDS
 * (2 M (N + hop - 1) + 12 (N + hop) bytes). */
#define TDOA_STREAM_TRIGGER_VAR_PCM16 131072 /* 2 * 256^2: the 8-bit threshold for samples scaled by 256 */
int tdoa_stream_create_pcm16(tdoa_ctx *ctx, int32_t num_streams, int32_t hop,
                             const int16_t *capture /* device [S][capture_len][M] */,
                             int64_t capture_len, int64_t trigger_var, int use_graph,
                             tdoa_stream **out);

/* ---- Continuous streaming: a frame per hop behind an activity gate ----
 * A second way of choosing frames, for rings that carry continuous audio
 * (speech, a motor) where the click trigger above fires at chance positions or
 * not at all.  GCC_PHAT contexts only.  The ring's element type follows the
 * context's sample format at creation: capture[S][capture_len][M] holds uint8_t
 * for TDOA_SAMPLES_ADC8 and int16_t (2-byte aligned) for TDOA_SAMPLES_PCM16;
 * the pipeline keeps that format whatever the context is switched to afterwards.
 * For stream s with samples x_m[t], pos the samples consumed before the hop:
 *   one candidate per stream and hop, e = pos + hop, eligible iff e >= N (a
 *   frame never reaches before the stream's start);  the frame is F = [e-N, e);
 *   pw(m) = N * sum_F x_m^2 - (sum_F x_m)^2 on the ring's own sample values
 *   (u8 counts 0..255 or int16 counts), exact in int64;
 *   the stream is listed iff sum_m pw(m) >= activity_var * N^2.
 * The comparison is >=: activity_var = 0 lists every eligible stream (one frame
 * per stream and hop).  activity_var is in counts^2 of the ring's samples,
 * summed over mics, in [0, 2^30] -- trigger_var's convention: the frame's sample
 * variance summed over the mics.  ring_start is neither read nor written.
 * Int64 bounds over every accepted shape (|x| <= 2^15, N <= 4096, M <= 8):
 * sum_F x^2 <= N 2^30 = 2^42, so N * sum_F x^2 <= 2^54; |sum_F x| <= N 2^15 =
 * 2^27, so (sum_F x)^2 <= 2^54; 0 <= pw <= 2^54 (Cauchy-Schwarz), over 8 mics
 * the sum <= 2^57; activity_var * N^2 <= 2^30 * 2^24 = 2^54.  The kernel holds a
 * lane's partial sum of x^2 in 32 bits over at most two samples
 * ((-32768)^2 * 4 = 2^32 does not fit) and in 64 bits from there.
 * Each listed frame goes through exactly what a triggered frame does
 * (k_stream_phat staging it from the ring, or k_stream_phat_pcm16 with the
 * PCM16 front end; at 8 mics x 2048 and 4 mics x 4096 k_f16_ring and
 * k_stream_ema_grid, either ring type): PHAT with phat_eps, the context's bin-weight table read at
 * every step, the inverses, first maximum, prior, the gate sum_p lag^2 > 4
 * deciding whether the EMA updates, the float EMA with now_us = e * 1e6 / fs,
 * and the grid solve on the EMA scores.
 * The result is an ordinary tdoa_stream: it steps with tdoa_stream_step_f, is
 * read with tdoa_stream_state_f (and tdoa_stream_state with est = NULL;
 * stats[0] counts listed frames), and tdoa_stream_reset / tdoa_stream_destroy
 * apply; graph mode and plain stream launches both work.  Kernel:
 * k_stream_active, in place of a trigger.
 * TDOA_ERR_INVALID, with tdoa_last_error naming the cause: a NULL argument; a
 * DIRECT context (it reproduces the firmware, which has no such mode);
 * activity_var outside [0, 2^30]; hop outside [1, N]; capture_len < N + 2 hop;
 * an int16 ring that is not 2-byte aligned; a shape outside the GCC_PHAT
 * shapes above (the LDS rule and the two long-frame shapes).  The triggers' own
 * 150 KiB LDS limit does not apply. */
int tdoa_stream_create_continuous(tdoa_ctx *ctx, int32_t num_streams, int32_t hop,
                                  const void *capture /* device [S][capture_len][M] */,
                                  int64_t capture_len, int64_t activity_var, int use_graph,
                                  tdoa_stream **out);
/* One hop for every stream, asynchronous on `stream` (graph mode needs a
 * non-NULL stream; the captured graph is reused while `out` and `stream`
 * stay the same). */
int tdoa_stream_step(tdoa_stream *st, const tdoa_stream_outputs *out, void *stream);
int tdoa_stream_step_f(tdoa_stream *st, const tdoa_stream_outputs_f *out, void *stream);
/* Back to the start: position 0, rings empty, EMA scores 0, EMA clocks 0. */
int tdoa_stream_reset(tdoa_stream *st, void *stream);
/* Synchronous snapshot: samples consumed, EMA scores [S][P][K], EMA clocks
 * [S] and running totals {triggered, gated} frames [2] (host pointers; any
 * may be NULL). */
int tdoa_stream_state(tdoa_stream *st, int64_t *pos, int64_t *est, uint64_t *last,
                      int64_t *stats);
int tdoa_stream_state_f(tdoa_stream *st, int64_t *pos, float *est, uint64_t *last,
                        int64_t *stats);

/* ---- Streaming: peaks and least-squares refinement of the EMA map per hop ----
 * The EMA state est[S][P][K] of a pipeline is the time-averaged map tdoa_peaks
 * names among its inputs; several sources accumulate in it over hops.
 * tdoa_stream_peaks runs tdoa_peaks on it for the frames the pipeline's last
 * step listed, without a host synchronisation or a copy.
 *
 * Let h be the step enqueued last on st since its creation or last reset; if
 * there is none, nothing is launched and the call returns TDOA_OK.  Let cnt be
 * h's frame count as the hop kernels clamp it, to [0, S], and for slot i < cnt
 * let s be the stream the pipeline listed in slot i (its own list, the one the
 * step copies to stream_id, not a caller buffer).  Row i of every output is
 * the tdoa_peaks result for the single block est[s] as step h left it, in the
 * pipeline's type (L for DIRECT, Lf for GCC_PHAT; the other field is not
 * written), by tdoa_peaks' own definition: the L map in T with one add per pair
 * in ascending p, greedy suppression, ties to the lowest cell, min_rel, the
 * empty-slot fills.  Outputs are [S][Kp]..., indexed by slot; rows >= cnt are
 * not written, and a hop with cnt = 0 writes nothing.
 *
 * gate, if non-NULL, is the step's gate output (device [S]): a slot with
 * gate[i] == 0 gets the empty record -- count[i] = 0 and every peak slot filled
 * as empty (cell -1, xy NaN, L INT64_MIN / Lf -inf, lags 0, xy_ls / ls_rms
 * NaN) -- and its map is not evaluated.  With gate == NULL every listed slot is
 * evaluated, gated or not: the map of a stream whose frame was not gated is
 * the one its last gated frame left.  A stream never updated has an all-zero
 * map: peak 0 is cell 0 with L = 0 (and with radius < the grid further peaks
 * follow, all with L = 0).
 *
 * xy_ls / ls_rms: as in tdoa_peaks, the refinement started at each peak with
 * the peak's lag tuple and the parabolic vertex of est[s] at those lags (the
 * int64 values read exactly); NaN in empty slots.
 *
 * Asynchronous on `stream`; never synchronises the host; plain launches
 * (k_stream_peaks, k_ls_stream) whether or not the pipeline replays graphs.
 * The call must be stream-ordered after step h and before the pipeline's next
 * step: the next step's selector writes a new list and zeroes h's counter slot
 * (the two slots alternate by hop parity, so h's is reused two steps later).
 * The one allocation, made at the first call that asks for xy_ls / ls_rms
 * without out->lags and never again, is a lag-tuple scratch of
 * S * TDOA_MAX_PEAKS * P int32 owned by st.
 *
 * TDOA_ERR_INVALID, with tdoa_last_error naming the cause: a NULL st / prm /
 * out / out->cell (checked before any device call), num_peaks outside
 * 1..TDOA_MAX_PEAKS, radius < 0, or a grid whose L map plus one stream's scores
 * exceed k_peaks' 150 KiB of LDS for the pipeline's type.  Nothing is launched
 * and no output is touched. */
int tdoa_stream_peaks(tdoa_stream *st, const tdoa_peaks_params *prm,
                      const uint8_t *gate /* device [S] or NULL */,
                      const tdoa_peaks_outputs *out, void *stream);
/* The pipeline's EMA state as a device pointer: int64 [S][P][K] (DIRECT,
 * *is_float = 0) or float [S][P][K] (GCC_PHAT, 1).  Valid until
 * tdoa_stream_destroy.  It makes the whole state usable with what exists --
 * tdoa_peaks(ctx, est, is_float, S, ...) and tdoa_heatmap for every stream,
 * not only the listed ones; such calls follow the usual rule: stream-ordered
 * with the steps.  Host only; TDOA_ERR_INVALID for a NULL argument. */
int tdoa_stream_est_device(tdoa_stream *st, const void **est, int *is_float);
/* Name of the kernel that computes the hop's scores (diagnostics, like
 * tdoa_batch_kernel): "k_stream_phat" / "k_stream_phat_pcm16", "k_f16_ring" at
 * the long-frame shapes (either ring type), "k_direct_mfma" / "k_direct" for a
 * DIRECT pipeline.  A static string; NULL for a NULL st. */
const char *tdoa_stream_kernel(const tdoa_stream *st);

/* ---- Tracking: sources followed across hops from the per-hop peaks ----
 * The rows tdoa_stream_peaks (or tdoa_peaks) reports are unlabelled and
 * memoryless.  The tracker keeps, per stream, a table of TDOA_MAX_TRACKS
 * records -- each a stable id, a position, a velocity and a covariance (a
 * constant-velocity Kalman filter per axis, the two axes sharing one 2 x 2
 * covariance) -- and updates it once per evaluated row from that row's
 * measurements.  The reference has no such layer.
 *
 * State.  tracks[S][TDOA_MAX_TRACKS] tdoa_track records, all zero at start;
 * next_id[S] int32, 0 at start: the first id given to a stream is 1.
 *
 * Inputs of a row: its stream s, its time t (int64 us), n = its count clamped
 * to [0, Kp], and the measurements z_k = (zx, zy), k < n, of a float
 * [rows][Kp][2] block.  With T = max_tracks, r = meas_var, q = accel_psd:
 *
 * Per evaluated row.  All float arithmetic is fp32, every operation rounded on
 * its own (no fused multiply-add, no reassociation), division IEEE; the steps
 * run in exactly this order:
 *   0. A row with n <= 0 is not evaluated: the state is untouched (no miss is
 *      counted, no time advances), the row's outputs are the unchanged table
 *      and assigned is all 0.  A measurement with a non-finite coordinate is
 *      invalid: it is neither associated nor born.
 *   1. Coast-out.  Each live slot j < T, in slot order: if
 *      t - upd_us > max_coast_us the record is zeroed (freed).
 *   2. Predict every live track:
 *        dt  = (float)max(t - t_us, 0) / 1e6f
 *        x   = x + vx*dt;   y = y + vy*dt
 *        a   = dt*p11;      c = (p01 + p01) + a;   d = dt*c
 *        dt2 = dt*dt;       dt3 = dt2*dt
 *        p00 = (p00 + d) + (q*dt3)/3.0f
 *        p01 = (p01 + a) + (q*dt2)*0.5f
 *        p11 = p11 + q*dt
 *        t_us = t
 *   3. Cost, for live j and valid k:
 *        dx = zx - x;  dy = zy - y;  s = p00 + r;  c_jk = (dx*dx + dy*dy) / s
 *      the pair is eligible iff c_jk <= gate_d2 (a NaN compares false).
 *   4. Greedy association.  Repeatedly take the eligible pair of minimum c_jk
 *      among tracks and measurements both still unassigned, ties to the lowest
 *      j, then the lowest k; assign it; stop when no eligible pair remains.
 *   5. Assigned track, all from the old values:
 *        k0 = p00/s;  k1 = p01/s
 *        x = x + k0*dx;    y = y + k0*dy
 *        vx = vx + k1*dx;  vy = vy + k1*dy
 *        p11 = p11 - k1*p01;  p01 = p01 - k0*p01;  p00 = p00 - k0*p00
 *        hits += 1;  misses = 0;  upd_us = t;  peak = k
 *        if status == 1 && hits >= confirm_hits then status = 2
 *   6. Unassigned live track: misses += 1; peak = -1; if
 *      misses >= max_misses the record is zeroed (freed).
 *   7. Births.  Each unassigned valid measurement, in ascending k, takes the
 *      lowest free slot < T (slots freed in steps 1 and 6 count as free); with
 *      no free slot it is dropped.  The new track: id = ++next_id[s],
 *      status = confirm_hits <= 1 ? 2 : 1, hits = 1, misses = 0, (x, y) = z,
 *      vx = vy = 0, p00 = r, p01 = 0, p11 = init_vel_var, t_us = upd_us = t,
 *      peak = k.
 *
 * Outputs (tdoa_track_outputs; each optional, at least one set):
 *   tracks [rows][T]       a copy of the stream's slots 0..T-1 after the row;
 *   assigned [rows][Kp]    the id of the track measurement k was assigned to or
 *                          born as, 0 otherwise (dropped, invalid, k >= n);
 *   num_confirmed [rows]   the slots < T with status 2 after the row.
 * Slots >= T of the state are neither read nor written.  Two rows of one call
 * naming the same stream is undefined; the pipeline's lists never do. */
#define TDOA_MAX_TRACKS 8

typedef struct tdoa_track {          /* 64 bytes, 8-byte aligned */
    int32_t id;       /* >= 1; 0 = free slot (then every field is 0) */
    int32_t status;   /* 0 free, 1 tentative, 2 confirmed */
    int32_t hits;     /* measurements assigned since birth (birth counts 1) */
    int32_t misses;   /* consecutive evaluations without one */
    float   x, y, vx, vy;      /* metres, metres/s, grid frame (as xy / xy_ls) */
    float   p00, p01, p11;     /* per-axis covariance: pos, pos-vel, vel (shared by x and y) */
    int32_t peak;     /* peak index assigned at the last evaluation, -1 none */
    int64_t t_us;     /* time the state is predicted to */
    int64_t upd_us;   /* time of the last assigned measurement */
} tdoa_track;

typedef struct tdoa_track_params {
    int32_t max_tracks;    /* T, 1..TDOA_MAX_TRACKS: slots 0..T-1 are used */
    int32_t confirm_hits;  /* >= 1: tentative -> confirmed when hits >= this */
    int32_t max_misses;    /* >= 1: freed when misses reaches this */
    int64_t max_coast_us;  /* > 0: freed when t - upd_us exceeds this */
    float   gate_d2;       /* > 0: association gate on the normalised distance^2 */
    float   meas_var;      /* r  > 0, m^2 */
    float   accel_psd;     /* q >= 0, m^2/s^3 */
    float   init_vel_var;  /* > 0, m^2/s^2 */
} tdoa_track_params;

typedef struct tdoa_track_outputs {  /* any may be NULL, not all */
    tdoa_track *tracks;      /* [rows][T] */
    int32_t *assigned;       /* [rows][Kp] */
    int32_t *num_confirmed;  /* [rows] */
} tdoa_track_outputs;

/* The block form, as tdoa_peaks is to tdoa_stream_peaks: rows of caller-owned
 * device state (tracks [S][TDOA_MAX_TRACKS], next_id [S]) updated from device
 * blocks; row i is stream stream_of_row[i] (device [rows]; NULL: stream i).
 * Asynchronous on `stream`, no allocation, no synchronisation; kernel k_track,
 * one wave per row.  rows = 0 returns TDOA_OK without a launch.
 * TDOA_ERR_INVALID, with tdoa_last_error naming the cause, before any device
 * call (nothing is launched, no output is touched): a NULL prm, out, count,
 * xy, t_us or state pointer; all outputs NULL; Kp outside 1..TDOA_MAX_PEAKS;
 * a parameter outside its range above or non-finite; rows < 0 or
 * rows >= 2^31. */
int tdoa_track_batch(int device, tdoa_track *tracks, int32_t *next_id, int64_t rows,
                     const int32_t *stream_of_row /* NULL: row i is stream i */,
                     const int64_t *t_us /* [rows] */, const int32_t *count,
                     const float *xy /* [rows][Kp][2] */, int32_t Kp,
                     const tdoa_track_params *prm, const tdoa_track_outputs *out, void *stream);
/* The same rule on the host, from the same inline predict / cost / update
 * functions: every pointer is a host pointer, rows are evaluated in order. */
int tdoa_track_host(tdoa_track *tracks, int32_t *next_id, int64_t rows,
                    const int32_t *stream_of_row, const int64_t *t_us, const int32_t *count,
                    const float *xy, int32_t Kp, const tdoa_track_params *prm,
                    const tdoa_track_outputs *out);
/* The streaming form.  The rows are the slots of the step enqueued last on st
 * (tdoa_stream_peaks' contract: the pipeline's own list, its counter slot
 * clamped to [0, S] on the device; nothing is launched if there has been no
 * step since create / reset); count (device [S]) and xy (device [S][Kp][2]) are
 * a tdoa_stream_peaks call's count and xy or xy_ls, indexed by slot; a row's
 * time is the EMA's own clock t = (uint64)end[slot] * 1000000 / fs, read from
 * the pipeline's list on the device.  Outputs are indexed by slot; rows past
 * the step's count are not written.  Per call order: step, peaks, track.
 * The state, S * (8 * 64 + 4) bytes owned by st, is allocated and zeroed at
 * the first call and never again; tdoa_stream_reset zeroes it.  Asynchronous
 * on `stream`, never synchronises the host, a plain launch whether or not the
 * pipeline replays graphs; it must be stream-ordered after the peaks call and
 * before the pipeline's next step.  TDOA_ERR_INVALID as above (st in place of
 * the state pointers). */
int tdoa_stream_track(tdoa_stream *st, const tdoa_track_params *prm,
                      const int32_t *count /* device [S] */,
                      const float *xy /* device [S][Kp][2] */, int32_t Kp,
                      const tdoa_track_outputs *out, void *stream);
/* The pipeline's track state as device pointers (tracks [S][TDOA_MAX_TRACKS],
 * next_id [S]) for every stream, listed or not; both NULL before the first
 * tdoa_stream_track.  Valid until tdoa_stream_destroy.  Host only;
 * TDOA_ERR_INVALID for a NULL argument. */
int tdoa_stream_tracks_device(tdoa_stream *st, const tdoa_track **tracks, const int32_t **next_id);

/* ---- Listening: a steered delay-and-sum beamformer per peak / per track ----
 * Every layer above ends in coordinates.  This one returns the signal of a
 * source at plane coordinates (u, v) -- as xy / xy_ls / tdoa_track.x, y report
 * them -- by aligning the mics on that point with fractional delays and
 * averaging them: the source adds coherently, the other sources and the
 * uncorrelated noise do not (1/M in power for white noise).  The reference has
 * no such layer.
 *
 * FIR table h[TDOA_BEAM_PHASES][2 * TDOA_BEAM_HALF], built on the host in
 * double arithmetic (tdoa_beam_fir): tap k = -7..8 of phase q = 0..31 sits at
 * h[q][k + 7] and is a Kaiser-windowed sinc at the fractional delay q/32,
 *     x = k - q/32;  h[q][k] = sinc(x) * I0(8 sqrt(1 - (x/8)^2)) / I0(8)
 * for |x| <= 8, else 0 (sinc(x) = sin(pi x) / (pi x), sinc(0) = 1; I0 the
 * modified Bessel function of order 0); each phase is then divided by its sum
 * over k, so that it sums to 1, and rounded to float.  Phase 0 is exactly the
 * unit tap at k = 0.
 *
 * Latency and the largest delay, per geometry, on the host in double:
 *     Dmax = ceil(max_{i<j} |mic_i - mic_j| * fs / c) + 1   samples
 *     A    = Dmax + TDOA_BEAM_HALF
 * (by the triangle inequality no target's inter-mic delay exceeds the mic
 * separation; the + 1 covers the fp32 roundings below).  Output sample n needs
 * the input up to n + A: the streaming form runs A samples behind the clock.
 *
 * Steering of a target (u, v).  All arithmetic is fp32, every operation rounded
 * on its own (no fused multiply-add), division and square root IEEE -- the
 * tracker's convention -- in the expression order of the lag LUT
 * (vga_heatmap.h:48-93), with h = height_offset, hypot3(a, b, c) =
 * sqrtf((a*a + b*b) + c*c):
 *     k = h / hypot3(h, u, v)
 *     xs = u*k;  ys = v*k;  zs = h*k             the point on the hemisphere
 *     d_m = hypot3(zs, xs - mx_m, ys - my_m)      for every mic m
 *     dmin = min_m d_m
 *     t_m = ((d_m - dmin) / c) * (float)fs
 *     r_m = floorf(t_m * 32.0f + 0.5f)
 *     code_m = r_m >= 0 ? (r_m > 32 Dmax ? 32 Dmax : (int32)r_m) : 0   (a NaN r_m gives 0)
 *     D_m = code_m >> 5;  q_m = code_m & 31
 * The mic nearest to the point has code 0; a farther mic hears the source
 * code_m / 32 samples later and is read that much ahead.  A target whose u or
 * v is not finite is invalid, and so is target k >= count.
 *
 * Output of a valid target, with x_m[t] the samples' own values (u8 counts,
 * int16 counts) as float, 0 for t < 0 and outside a block-form frame:
 *     y[n] = (1/M) * sum_m sum_{k=-7..8} h[q_m][k] * x_m[n + D_m + k]
 * accumulated in fp32 from 0, m ascending, then k ascending, one fused
 * multiply-add per tap; the sum is multiplied by (1.0f / (float)M).  An invalid
 * target's block is all zeros, its codes are -1, its active byte 0.  No DC
 * removal, no gain control; u8 samples keep their offset (a constant 128 input
 * gives 128).  The delays are constant within a block: interpolating the
 * delays of a moving target inside a block is out of scope -- a block of a
 * moving track is steered at the position the track table holds when the call
 * runs, and the steering steps at block boundaries. */
#define TDOA_BEAM_HALF 8
#define TDOA_BEAM_PHASES 32
#define TDOA_BEAM_MAX_TARGETS 8

typedef struct tdoa_beam_geometry {  /* what steering reads of a context */
    int32_t num_mics;        /* M, 2..TDOA_MAX_MICS */
    int32_t sample_rate_hz;  /* fs > 0 */
    float speed_of_sound;    /* c > 0, m/s */
    float height_offset;     /* h > 0, m */
    float mic_xy[TDOA_MAX_MICS][2];  /* metres; rows >= M are not read */
} tdoa_beam_geometry;

typedef struct tdoa_beam_outputs {   /* audio is required, the others may be NULL */
    float *audio;            /* [rows][Kt][n]  n = frame_len (block form) or hop (streaming) */
    int32_t *delays;         /* [rows][Kt][M]  the codes, -1 for an invalid target */
    uint8_t *active;         /* [rows][Kt]     1 valid, 0 invalid */
    int64_t *block_start;    /* [1] streaming only: the absolute sample of audio[.][.][0] */
} tdoa_beam_outputs;

/* The FIR table above, float [32][16].  Host only. */
int tdoa_beam_fir(float *h);
/* The geometry of the context a config would make: validates num_mics,
 * sample_rate_hz, speed_of_sound, height_offset and mic_xy as tdoa_create does
 * (NULL mic_xy with 3 mics: the reference triangle).  Host only, no device. */
int tdoa_beam_geometry_of(const tdoa_config *cfg, tdoa_beam_geometry *g);
/* A and Dmax of a geometry / of a context (either pointer may be NULL).
 * TDOA_ERR_INVALID for a geometry outside the ranges above, a non-finite mic
 * coordinate, or Dmax > 65536. */
int tdoa_beam_latency_of(const tdoa_beam_geometry *g, int32_t *A, int32_t *Dmax);
int tdoa_beam_latency(const tdoa_ctx *ctx, int32_t *A, int32_t *Dmax);
int tdoa_get_beam_geometry(const tdoa_ctx *ctx, tdoa_beam_geometry *g);

/* The block form (kernel k_beam, one workgroup per frame): frames is device
 * int16 [B][M][N], the layout tdoa_localize_batch takes; count device [B] or
 * NULL for all Kt; xy device [B][Kt][2]; outputs audio [B][Kt][N] for
 * n in [0, N), delays [B][Kt][M], active [B][Kt] (block_start is not written).
 * Asynchronous on `stream`, no allocation, no synchronisation.  B = 0 returns
 * TDOA_OK without a launch.  TDOA_ERR_INVALID, with tdoa_last_error naming the
 * cause, before any device call: a NULL ctx, frames, xy, out or out->audio; Kt
 * outside 1..TDOA_BEAM_MAX_TARGETS; B < 0 or B >= 2^31; a workgroup's staging
 * (M (N + Dmax + 15) + 512) * 4 bytes beyond 150 KiB. */
int tdoa_beam_batch(tdoa_ctx *ctx, const int16_t *frames, int64_t B, const int32_t *count,
                    const float *xy, int32_t Kt, const tdoa_beam_outputs *out, void *stream);
/* The same on host pointers for frames of N samples, from the same inline
 * steering and tap-sum functions (csrc/tdoa_beam_rule.h): no device, no HIP. */
int tdoa_beam_host(const tdoa_beam_geometry *g, int32_t N, const int16_t *frames, int64_t B,
                   const int32_t *count, const float *xy, int32_t Kt, const tdoa_beam_outputs *out);
/* The streaming form (kernel k_beam_ring<uint8_t | int16_t>, one workgroup per
 * stream), for every pipeline kind: one more asynchronous call after
 * step -> peaks -> track, a plain launch stream-ordered after the step and
 * before the producer overwrites the ring rows it reads.  With e = the device
 * clock after the last step (read on the device), it reads samples
 * [e - hop - A - 7, e) of every stream's ring (sample t at row t mod
 * capture_len; t < 0 is zero) and writes, for ALL S streams indexed by stream
 * (not by slot, and whether or not the step listed the stream), the block
 * n in [e - hop - A, e - A): audio [S][Kt][hop], delays [S][Kt][M],
 * active [S][Kt], block_start [1] = e - hop - A.  Consecutive hops' blocks abut.
 * Targets: with xy != NULL, xy[s][k] (device [S][Kt][2]) for k < count[s]
 * (device [S]; NULL: all Kt) -- the caller scatters a step's peaks by
 * stream_id; with xy == NULL the pipeline's own track table, target k = slot k
 * of stream s at (x, y), valid iff its status >= min_status, so a channel is a
 * track slot and stays with its id (count is not read).
 * TDOA_ERR_INVALID before any device call: a NULL st, out or out->audio; Kt
 * outside 1..TDOA_BEAM_MAX_TARGETS; xy == NULL before the first
 * tdoa_stream_track; capture_len < 2 hop + A + Dmax + 16 (the reach of a block
 * plus one hop of margin for the producer); a workgroup's staging
 * (M (hop + Dmax + 15) + 512) * 4 bytes beyond 150 KiB.  With no step since
 * create / reset it returns TDOA_OK and launches nothing. */
int tdoa_stream_beam(tdoa_stream *st, const int32_t *count, const float *xy, int32_t Kt,
                     int32_t min_status, const tdoa_beam_outputs *out, void *stream);

/* ---- Separating: a null-steering beamformer, one channel per target ----
 * The delay-and-sum above averages uncorrelated noise out; a second SOURCE it
 * passes a few dB down at most, at low frequencies not down at all.  This
 * layer uses the other targets' positions: per frequency bin a linearly
 * constrained beamformer with unit gain on target j and nulls on the other
 * valid targets of the same row, diagonally loaded so that it degrades to the
 * delay-and-sum where the array cannot separate.  The reference has no such
 * layer.
 *
 * Per row (a block-form frame, a stream), block length L (a power of two in
 * 128..2048), M mics, Kt <= TDOA_SEP_MAX_TARGETS targets of which J are valid:
 *
 * 1. Steering.  code_{j,m} of target j and mic m is the delay-and-sum rule's
 *    (beam_code, "Listening"), unchanged, and so is validity: finite (u, v),
 *    k < count, or a track status >= min_status.  tau = code / 32 samples.
 * 2. Analysis.  x_m[t] is the samples' own values as float (u8 keeps its
 *    offset), 0 for t < 0.  Window: periodic sqrt-Hann,
 *        g[n] = sqrt(0.5 - 0.5 cos(2 pi n / L)),   n = 0..L-1,
 *    built on the host in double and rounded to float (tdoa_sep_window).
 *        X_m[k] = sum_n (g[n] * x_m[n]) e^{-2 pi i k n / L},   k = 0..L/2
 *    (the product in fp32; the transform an fp32 FFT).
 * 3. Steering vectors.
 *        p = (k * code_{j,m}) mod 32 L          in integers, before any float
 *        a_{j,m}[k] = exp(-2 pi i p / (32 L))
 * 4. Weights per bin.  A = [a_{j,m}] is M x J over the valid targets,
 *        G = A^H A + delta M I                  delta = `loading`
 *        W = (1 + delta) A G^-1
 *        Y_j[k] = sum_m conj(W[m][j]) X_m[k]  =  (1 + delta) [G^-1 (A^H X)]_j
 *    G is J x J Hermitian positive definite (its diagonal is M + delta M); it is
 *    solved by Cholesky factorisation and two triangular solves, one bin per
 *    thread, in registers.  The a_{j,m} and X_m are fp32 values; A^H A, A^H X
 *    and the solve are accumulated in double from them, because a pivot of G
 *    is delta M left of (1 + delta) M minus nearly as much -- in fp32 the bins
 *    the array cannot separate (the lowest ones, a u8 ring's offset among
 *    them) would lose 1 / delta of their precision.  Y_j is rounded to fp32.
 *    An invalid target takes part as a zero
 *    column: its row of G is delta M on the diagonal and 0 elsewhere, which
 *    leaves the valid targets' solution what the J x J system gives.
 *    With J = 1: G = M (1 + delta), Y = (1/M) sum_m conj(a_m) X_m, exactly the
 *    frequency-domain delay-and-sum.  With G0 = A^H A, the response of channel
 *    j to a source at target i's steering vector is
 *        [(1 + delta) (G0 + delta M I)^-1 G0]_ji :
 *    on the own target (i = j) it is 1 - O(delta) where G0 is well conditioned
 *    and exactly 1 for J = 1; on another target it is O(delta M / lambda_min(G0))
 *    -- a null as deep as the loading allows.  As delta -> infinity,
 *    (1 + delta) (G0 + delta M I)^-1 -> I / M: every channel tends to its
 *    delay-and-sum.  loading is a float in [1e-4, 1e4]; TDOA_SEP_LOADING is the
 *    default.
 * 5. Synthesis.  y_j[n] = g[n] * irfft(Y_j)[n], irfft the inverse real
 *    transform of length L including its 1/L (the imaginary parts of bins 0
 *    and L/2 are not read).  An invalid target's block is zeros, its codes are
 *    -1, its active byte 0.
 * 6. Circular-delay guard.  The delays act circularly within a block, so the
 *    block must be long against them: TDOA_ERR_INVALID unless L >= 8 Dmax
 *    (Dmax as tdoa_beam_latency reports it) and L is a power of two in
 *    128..2048.
 * g[n]^2 + g[n + L/2]^2 = 1: blocks at 50 % overlap add up to the full
 * reconstruction.  Steering is constant within a block, as above. */
#define TDOA_SEP_MAX_TARGETS 4
#define TDOA_SEP_LOADING 1e-2f
#define TDOA_SEP_LOADING_MIN 1e-4f
#define TDOA_SEP_LOADING_MAX 1e4f

/* g[0..L) above, float [L].  Host only.  TDOA_ERR_INVALID for a NULL g or an L
 * that is no power of two in 128..2048. */
int tdoa_sep_window(int32_t L, float *g);
/* The argument rules of both forms on the host, no device: TDOA_OK if a
 * geometry's Dmax, L, Kt and loading are a block the separator takes,
 * TDOA_ERR_INVALID with tdoa_last_error naming the cause otherwise. */
int tdoa_sep_check_of(const tdoa_beam_geometry *g, int32_t L, int32_t Kt, float loading);

/* The block form's block length L of a context: frame_len at creation where
 * that is a block the separator takes (a power of two in 128..2048 with
 * L >= 8 Dmax), else none (0).  tdoa_sep_set_block chooses another -- a context
 * whose frame_len is 1024 separates blocks of 128 -- and uploads its window and
 * twiddles: it allocates and synchronises the device, so it is a setup call,
 * not a per-block one.  TDOA_ERR_INVALID for a NULL ctx or an L step 6 refuses
 * (the block length in force stays). */
int tdoa_sep_set_block(tdoa_ctx *ctx, int32_t L);
int tdoa_sep_get_block(const tdoa_ctx *ctx, int32_t *L);
/* The block form (kernel k_sep, one workgroup per frame), the stateless core:
 * one STFT block per row of the context's block length L (tdoa_sep_get_block;
 * the kernel reads nothing else of frame_len).  frames is device int16 [B][M][L];
 * count device [B] or NULL for all Kt; xy device [B][Kt][2]; outputs
 * audio [B][Kt][L] -- the synthesis-windowed block y_j, which the caller
 * overlap-adds --, delays [B][Kt][M], active [B][Kt] (block_start is not
 * written).  Asynchronous on `stream`, no allocation, no synchronisation.
 * B = 0 returns TDOA_OK without a launch.  TDOA_ERR_INVALID, with
 * tdoa_last_error naming the cause, before any device call: a NULL ctx, frames,
 * xy, out or out->audio; Kt outside 1..TDOA_SEP_MAX_TARGETS; B < 0 or
 * B >= 2^31; loading outside [1e-4, 1e4] or not finite; a context without a
 * block length. */
int tdoa_sep_batch(tdoa_ctx *ctx, const int16_t *frames, int64_t B, const int32_t *count, const float *xy,
                   int32_t Kt, float loading, const tdoa_beam_outputs *out, void *stream);
/* The streaming form (kernel k_sep over the capture rings, uint8 or int16, one
 * workgroup per stream), for every pipeline kind: one more plain launch after
 * step -> peaks -> track.  L = 2 hop.  With e = the device clock after the last
 * step (read on the device), it reads samples [e - L, e) of every stream's
 * ring (t < 0 is zero), adds the first half of each target's block y_j to the
 * stream's saved tail and writes that as the block n in [e - L, e - hop):
 * audio [S][Kt][hop], delays [S][Kt][M], active [S][Kt], block_start [1] =
 * e - L; the second half is the new tail.  Consecutive hops' blocks abut and
 * add up to the full reconstruction, L samples behind the clock.  Targets as
 * tdoa_stream_beam takes them: xy [S][Kt][2] with count [S], or -- xy NULL --
 * the pipeline's own track table, channel k = slot k, valid iff its status >=
 * min_status.  The tail state, float [S][TDOA_SEP_MAX_TARGETS][hop], and the
 * window are allocated at the first call; the tails are zeroed then, by
 * tdoa_stream_reset, and by a call whose Kt differs from the call's before.
 * With no step since create / reset it returns TDOA_OK and launches nothing.
 * TDOA_ERR_INVALID before any device call: a NULL st, out or out->audio; Kt
 * outside 1..TDOA_SEP_MAX_TARGETS; xy == NULL before the first
 * tdoa_stream_track; loading outside its range; the L conditions of step 6 on
 * L = 2 hop; capture_len < 3 hop (the block plus one hop of margin for the
 * producer). */
int tdoa_stream_sep(tdoa_stream *st, const int32_t *count, const float *xy, int32_t Kt, int32_t min_status,
                    float loading, const tdoa_beam_outputs *out, void *stream);
int tdoa_stream_destroy(tdoa_stream *st);

const char *tdoa_last_error(void);
int tdoa_abi_version(void);
/* Name of the kernel a tdoa_localize_batch call of this context runs first
 * (diagnostics: profile and HBM-traffic attribution); "" if none applies. */
const char *tdoa_batch_kernel(const tdoa_ctx *ctx);
/* 1 if a grid-requesting tdoa_localize_batch of this context solves the grid
 * inside that first kernel (no weighted-score scratch, no separate grid
 * launch), 0 if a grid kernel follows it (diagnostics, like tdoa_batch_kernel). */
int tdoa_batch_grid_fused(const tdoa_ctx *ctx);
/* Measurement: the shader clock (MHz) `device` holds under VALU load -- every
 * CU's waves run FMA chains for about `ms` milliseconds (0 < ms <= 100) on
 * `stream` and compare s_memtime with the 100 MHz s_memrealtime; the median
 * over waves.  Synchronous.  bench.py records it after its timed region so a
 * slow box and a regression can be told apart. */
int tdoa_gpu_clock_mhz(int device, void *stream, double ms, double *mhz);

#ifdef __cplusplus
}
#endif
#endif /* TDOA_H */
