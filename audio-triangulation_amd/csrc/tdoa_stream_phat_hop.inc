// tdoa_stream_phat_hop.inc -- the body of k_stream_phat (8-bit capture rings) and
// k_stream_phat_pcm16 (int16 rings, tdoa_stream_create_pcm16), as text: it
// reads the kernel's parameters (sp, kp, out, est_all, max_Lf, nstreams, e2)
// and the constant PCM16 of the including scope.  Either stages the slot's
// frame from its stream's ring (every selector lists frames, none copies one).
// PCM16: sp.capture points at int16 samples and the front end is
// phat_front_end<true>; everything after it is the same text.  What follows a
// slot's scores (gate, record, EMA, grid scan) is tdoa_stream_ema_grid.inc.
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int N = kp.N, M = kp.M, P = kp.P, K = kp.K, S = kp.S, tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6, nwaves = TPB / 64;
    f2 *U = (f2 *)smem;                // [M][N] unit spectra (slot 0 = bins 0 and N); a mic's raw samples before
    f2 *buf = U + (size_t)M * N;       // [N] FFT work buffer
    float *Wf = (float *)(buf + N);    // [P][K] the frame's weighted scores
    float *E = Wf + P * K;             // [P][K] the stream's EMA scores
    __shared__ int red[TPB / 64];
    __shared__ float redv[TPB / 64];
    __shared__ int redi[TPB / 64];
    __shared__ float sc[128];
    __shared__ int lag_s[TDOA_MAX_PAIRS];

    // at most one slot per stream: a corrupted counter cannot index past [S]
    const int cnt_raw = *sp.count;
    const int cnt = cnt_raw < 0 ? 0 : (cnt_raw > nstreams ? nstreams : cnt_raw);
    if (blockIdx.x == 0 && tid == 0) {
        *sp.pos += sp.H;  // the trigger kernel has read it
        sp.stats[0] += cnt;
        if (out.count)
            *out.count = cnt;
    }
    const uint32_t *win = reinterpret_cast<const uint32_t *>(kp.window);
    const int64_t ring_bytes = sp.capture_len * M;
    int ngated = 0;  // this workgroup's gated frames
    SP_T0();
    // persistent over the compact batch (its size is only known on the device)
    for (int slot = blockIdx.x; slot < cnt; slot += gridDim.x) {
        __syncthreads();  // the previous slot's tables and reductions are consumed
        SP_MARK(3);
        const int s = sp.ids[slot];
        const int64_t end = sp.end[slot];

        // ---- the frame's samples as int16, mic m's row at the start of U[m]
        if constexpr (PCM16) {
            // ring samples [at, at + N) of the stream, [n][M] -> [m][n], wrapping
            // at the ring's end.  A thread takes samples 2q, 2q + 1 of one mic
            // (m fastest: a wave's 2-byte loads cover contiguous ring bytes; a
            // ring need not start 4-byte aligned) and writes them as one LDS word
            const int64_t cl = sp.capture_len;
            const int16_t *cap = reinterpret_cast<const int16_t *>(sp.capture) + (size_t)s * cl * M;
            const int64_t at = sp.ring_at[slot];
            for (int i = tid; i < (N >> 1) * M; i += TPB) {
                const int q = i / M, m = i - q * M;
                int64_t j0 = at + 2 * q;  // at < cl, 2q < N <= cl: one wrap at most
                if (j0 >= cl)
                    j0 -= cl;
                const int64_t j1 = j0 + 1 >= cl ? 0 : j0 + 1;
                const uint32_t lo = (uint16_t)cap[(size_t)j0 * M + m], hi = (uint16_t)cap[(size_t)j1 * M + m];
                reinterpret_cast<uint32_t *>(U + (size_t)m * N)[q] = lo | hi << 16;
            }
        } else {
            // ring bytes [at * M, at * M + N * M) of the stream, wrapping at the
            // ring's end; byte loads: a ring need not start 4-byte aligned.  No
            // zero fill before the stream's start: every selector lists end >= N
            const uint8_t *cap = sp.capture + (size_t)s * ring_bytes;
            const int64_t b0 = sp.ring_at[slot] * M;
            for (int i = tid; i < N * M; i += TPB) {
                const int l = i / M, m = i - l * M;
                int64_t b = b0 + i;
                if (b >= ring_bytes)
                    b -= ring_bytes;
                reinterpret_cast<int16_t *>(U + (size_t)m * N)[l] = (int16_t)cap[b];
            }
        }
        __syncthreads();
        SP_MARK(0);

        // ---- per mic: front end, FFT_N, split, unit spectrum
        for (int m = 0; m < M; m++) {
            f2 *row = U + (size_t)m * N;
            phat_front_end<PCM16>(reinterpret_cast<const uint32_t *>(row), win, N, kp.log2N, red, buf);
            fft_inplace<false>(buf, N, kp.tw);
            phat_split<true>(buf, row, N, kp.tw2, e2);  // U = X / sqrt(|X|^2 + e2)
            __syncthreads();  // buf and red are free for the next mic
        }

        SP_MARK(1);
        // ---- per pair: cross spectrum, inverse FFT_N, lags -S..S, first maximum, prior
        const float *bw = kp.bin_w;
        for (int p = 0; p < P; p++) {
            const f2 *Ui = U + (size_t)kp.pair_i[p] * N;
            const f2 *Uj = U + (size_t)kp.pair_j[p] * N;
            for (int k = tid; k <= N / 2; k += TPB) {  // R = conj(U_i) U_j
                const int kn = (N - k) & (N - 1);
                f2 ik = Ui[k], in = Ui[kn], jk = Uj[k], jn = Uj[kn];
                if (k == 0) {  // slot 0 = (U[0], U[N]), both real
                    ik = f2{ik.x, 0.0f};
                    jk = f2{jk.x, 0.0f};
                    in = f2{in.y, 0.0f};
                    jn = f2{jn.y, 0.0f};
                }
                f2 Rk = cmul(conj2(ik), jk), Rn = cmul(conj2(in), jn);
                if (bw) {  // band-limited: bin k by w[k], bin N - k by w[N - k]
                    Rk = bw[k] * Rk;
                    Rn = bw[N - k] * Rn;
                }
                phat_fold(buf, N, k, Rk, Rn, kp.tw2);
            }
            __syncthreads();
            fft_inplace<true>(buf, N, kp.tw);
            phat_lags(buf, sc, N, K, S);
            if (tid < 64) {
                const int k1 = lane, k2 = lane + 64;
                const float v1 = k1 < K ? sc[k1] : -INFINITY, v2 = k2 < K ? sc[k2] : -INFINITY;
                const int bk = wave_first_max(v1, v2, lane, K);
                prior_weighted(Wf + p * K, kp.prior, v1, v2, lane, K, bk);
                if (lane == 0)
                    lag_s[p] = bk - S;
            }
            __syncthreads();  // sc and buf are free for the next pair
        }

        SP_MARK(2);
#ifdef TDOA_DIAG
        sp_acc_[4] += 1;
#endif
        // ---- gate, record, float EMA, EMA rows' maxima, grid scan (shared with k_stream_ema_grid)
#include "tdoa_stream_ema_grid.inc"
    }
    SP_MARK(3);
    SP_FLUSH();
    // gated frames of this hop: one atomic per workgroup that had any
    if (tid == 0 && ngated)
        atomicAdd(reinterpret_cast<unsigned long long *>(sp.stats + 1), (unsigned long long)ngated);
