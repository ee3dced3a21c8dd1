// tdoa_frame16_frames.inc -- the body of the per-frame long-frame kernels of
// tdoa_phat_r16.hip, included once per kernel: k_frame16<C, M, DM, XS, FG>
// (8-bit ADC front end), k_f16_pcm16<C, M, DM> (TDOA_SAMPLES_PCM16) and
// k_f16_ring<C, M, PCM16, BW> (a streaming step's listed frames).  It
// reads the kernel's parameters (kp, out, frames, B, e2) and the constants C,
// M, DM, XS, FG, PCM16, RING and BW of the including scope; the two formats
// differ in frame16_forward's front-end block alone.  RING (k_f16_ring only):
// B is the step's clamped frame count, frame fr is the step's slot fr, staged
// by `fetch` from its stream's capture ring (rs: f16_ring_src) instead of
// `frames`, and every output is indexed by slot; BW (RING only): the pairs'
// cross spectra are multiplied by the weight table kp.bin_w, bin b by w[b] and
// bin C - b by w[C - b] (b = 0 pairs with bin C, the self-paired bin takes
// w[C / 2]: tdoa_stream_phat_hop.inc's mapping).  Text rather than a __device__
// function: inlined from one, every k_frame16 instantiation's code came out
// different (the callee is simplified on its own, without the kernel's
// work-group size, before it is inlined).
    constexpr int T = C / 16, R1 = C / 256, G = 16384 / C, NS = C / 2048, BUF = f16_buf<C, XS>();
    static_assert(M >= 2 && M <= G, "one forward round: every mic has its own group");
    constexpr int P = M * (M - 1) / 2, ROUNDS = (P + G - 1) / G;
    constexpr int WPG = T / 64;  // waves per group (4 or 2)
    static_assert(WPG == 2 || WPG == 4, "group of 2 or 4 waves");
    static_assert(DM == 0 || DM == 1, "deferred-output mode");
    static_assert(RING || !BW, "the batch kernels take no weight table (a weighted batch runs the two-pass route)");
    static_assert(!RING || !FG, "no fused grid over a ring");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    f2 *bufs = (f2 *)smem;                    // [G][BUF]
    f2 *xhalf = bufs + G * BUF;               // [G] U_m[C / 2]
    int *red = (int *)(xhalf + G);            // [16] per-wave DC partial sums
    int *lagl = red + 16;                     // [TDOA_MAX_PAIRS]
    f2 *ttl = (f2 *)(lagl + TDOA_MAX_PAIRS);  // [3][16][16] the r16 twiddle tables
    float *priorl = (float *)(ttl + 3 * 16 * 16);  // [128] the lag prior (K <= 127)
    f2 *tw3 = (f2 *)(priorl + 128);  // [R1][64] pass-3 twiddles per lane (row 0 unused)
    // BW: the weights take registers through the pair rounds, where a byte
    // ring's sixteen loads are in flight; the window words leave theirs for LDS
    // (free next to the deferred scores at both ring shapes)
    constexpr bool WINL = f16_win_lds<C>() || BW;
    constexpr int WMODE = BW ? 1 : f16_win_mode<C>();
    uint32_t *winl = (uint32_t *)(tw3 + R1 * 64);  // WINL: [C / 2] window words
    float *scl = (float *)(winl + (WINL ? C / 2 : 0));  // DM 1: [P][K] raw scores of the frame
    // FG: the fused grid's LDS (FgLds) after scl, 16-B aligned; its levels in
    // the last round's idle groups' buffers
    constexpr int GI0 = P - (ROUNDS - 1) * G;  // first idle group of the last round
    static_assert(!FG || (G - GI0) * (T / 64) >= FG_NGW, "the last round must leave FG_NGW idle waves");
    const int CKp = (kp.wc_CK + 3) & ~3;
    FgLds fgl{};
    if constexpr (FG) {
        const int fo = (int)(((char *)(scl + (DM == 1 ? P * kp.K : 0)) - smem + 15) & ~15);
        fgl.w = (float *)(smem + fo);
        fgl.bnd = fgl.w + (DM == 0 ? 2 : 1) * CKp;  // DM 1: one buffer (written after the last round)
        fgl.key = (uint64_t *)(fgl.bnd + 256);
        fgl.cand = (int *)(fgl.key + 2 * FG_NGW);
    }
    const FgGrid<P> fgg{fgl, (float *)(bufs + GI0 * BUF), kp.wc_CK, CKp};
    int64_t prev = -1;  // FG: the previous frame of this workgroup (its grid is still to solve)
    int fpar = 0;       // FG, DM 0: this iteration's half of the double-buffered scores (by iteration, not
                        // frame parity: a workgroup's frames are gridDim.x apart)
    const int g = (int)threadIdx.x / T;
    const int K = kp.K, S = kp.S;
    f2 *buf = bufs + g * BUF;
    const uint32_t *win = reinterpret_cast<const uint32_t *>(kp.window);
    const f2 *tw2 = reinterpret_cast<const f2 *>(kp.tw2);
    // the twiddle tables in LDS (6 KiB): every pass reads them right after a
    // barrier, where a global (L2) round trip would stall the whole workgroup
    if (threadIdx.x < 3 * 16 * 16)  // 8-B units: kp.r16_tw is 8-B aligned
        ttl[threadIdx.x] = reinterpret_cast<const f2 *>(kp.r16_tw)[threadIdx.x];
    // the prior too: a pass-3 global read waits (vmcnt) for the next frame's
    // words, requested just before the pair rounds
    if (threadIdx.x < (unsigned)kp.K)
        priorl[threadIdx.x] = kp.prior[threadIdx.x];
    // (pass 3 multiplied two table entries per term before: 4.51 vs 4.26 ms per config-3 step)
    if (threadIdx.x < R1 * 64) {  // lane l: conj(W_C^{r l}) (l < 32), W_C^{r (64 - l)}
        const int r = threadIdx.x >> 6, l = threadIdx.x & 63;
        const f2 t = twC(reinterpret_cast<const f2 *>(kp.r16_tw), r, l < 32 ? l : 64 - l);
        tw3[threadIdx.x] = f2{t.x, l < 32 ? -t.y : t.y};
    }
#if F16_TW_REG
    // W_2C^b of this thread's split bins and W_2C^{C/2}: loaded once for the
    // launch (read per frame from L2, their latency opened every split)
    f2 twb[NS];
#pragma unroll
    for (int s2 = 0; s2 < NS; s2++)
        twb[s2] = tw2[(int)threadIdx.x + 1024 * s2];
    f2 twh = tw2[C / 2];
#endif
    uint32_t wr[8] = {};  // f16_win_mode 2: this thread's window words
    if constexpr (WMODE == 2) {
        const int j0 = (int)threadIdx.x - g * T;
#pragma unroll
        for (int s2 = 0; s2 < 8; s2++)
            wr[s2] = win[j0 + T * s2];
    }
    if constexpr (WINL) {
        for (int i = threadIdx.x; i < C / 2; i += 1024)
            winl[i] = win[i];
        __syncthreads();  // the forward reads the window before its first barrier
    }
    const f2 *tt = ttl;  // visible after the first barrier (the DC sum's)
    const int mg = g < M ? g : 0;  // groups without a mic transform mic 0 (unused)
    const int P3W = (g / (4 / WPG)) % WPG;  // the group's pass-3 wave: SIMD (g WPG + P3W) mod 4
    // the compact-scratch ranges (kp.wc_lo / wc_w / wc_off) of every pair this
    // wave outputs, read once here: a kp byte indexed by a runtime pair is a
    // VMEM load whose vmcnt wait would also wait for the next frame's words.
    // rl_*[r]: round r's pair of the group (pass 3); ep_*: the epilogue's pairs
    int rl_lo[ROUNDS], rl_w[ROUNDS], rl_off[ROUNDS];
#pragma unroll
    for (int r = 0; r < ROUNDS; r++) {
        const int q = r * G + g < P ? r * G + g : 0;
        rl_lo[r] = __builtin_amdgcn_readfirstlane(kp.wc_lo[q]);
        rl_w[r] = __builtin_amdgcn_readfirstlane(kp.wc_w[q]);
        rl_off[r] = __builtin_amdgcn_readfirstlane(kp.wc_off[q]);
    }
    // DM 1 (frame16_out16): this lane's pair 4 w + (lane >> 4) and its compact range
    constexpr bool OUT16 = DM == 1 && !FG && F16_OUT16 != 0;
    // (one register: lo | w << 8 | off << 16; the lagged epilogue runs where the
    // forward's registers peak)
    uint32_t e16_rng = 0;
    if constexpr (OUT16) {
        const int e16_p = f16_epi_pair<P>((int)threadIdx.x);  // this lane's row's pair
        const int pq = e16_p < P ? e16_p : 0;
        // per-lane loads, waited for below.  Workaround for a codegen bug: picking
        // each row's range from the wave's four scalar loads (F16_RNG_SCALAR=1)
        // makes hipcc address wc_off[p] (u16, p = 4 w + 2) as SBASE = kernarg + p,
        // SOFFSET = p, and gfx950's scalar loads drop the base's low two address
        // bits: every wave's row 2 read the offset of its row 0 (round 5: cfg4
        // cells 72 % equal; root cause round 6, tools/probe/smem_sbase_align.hip,
        // tools/diag_rng.py; tests/test_code_objects.py flags the pattern)
#if F16_RNG_SCALAR
        // A/B for the ISA audit: the wave's four ranges as scalar loads, the
        // row's picked by a per-lane select
        (void)pq;
        const int w0 = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
        uint32_t rq[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int p = 4 * w0 + q < P ? 4 * w0 + q : 0;
            rq[q] = (uint32_t)kp.wc_lo[p] | (uint32_t)kp.wc_w[p] << 8 | (uint32_t)kp.wc_off[p] << 16;
        }
        const int row = ((int)threadIdx.x >> 4) & 3;
#if F16_RNG_SCALAR == 2
        // branch-free: the four ranges forced into SGPRs, a v_cndmask chain
#pragma unroll
        for (int q = 0; q < 4; q++)
            rq[q] = __builtin_amdgcn_readfirstlane(rq[q]);
        e16_rng = rq[0];
        e16_rng = row == 1 ? rq[1] : e16_rng;
        e16_rng = row == 2 ? rq[2] : e16_rng;
        e16_rng = row == 3 ? rq[3] : e16_rng;
#else
        e16_rng = row == 0 ? rq[0] : (row == 1 ? rq[1] : (row == 2 ? rq[2] : rq[3]));
#endif
#else
        const auto *kk = kernarg_kp();
        e16_rng = (uint32_t)kk->wc_lo[pq] | (uint32_t)kk->wc_w[pq] << 8 | (uint32_t)kk->wc_off[pq] << 16;
#endif
        asm volatile("" : "+v"(e16_rng));
    }
    // DM 1 (four-pairs epilogue), lagged (F16_EPI_LAG): frame f's outputs run in
    // frame f + 1's forward, after its pass-3 stores; its gate after that forward
    constexpr bool ELAG = OUT16 && F16_EPI_LAG != 0;
    // the waves (four pairs each) whose outputs run after the forward's pass-2
    // stores; the rest after its pass-3 stores (F16_EPI_SPLIT: -1 half, else count)
    constexpr int EPW = f16_epi_waves<P>(), EPS = F16_EPI_SPLIT < 0 ? EPW / 2 : (F16_EPI_SPLIT < EPW ? F16_EPI_SPLIT : EPW);
    auto epi16 = [&](int64_t f, int ps) F16_AI {
        const int t = opaque_idx((int)threadIdx.x);
        const int wv = __builtin_amdgcn_readfirstlane(t >> 6), pe = f16_epi_pair<P>(t);
        const bool mine = ps == 0 || (ps == 2 ? wv < EPS : wv >= EPS);
        if (!F16_NO_OUT && mine && wv < f16_epi_waves<P>() && pe < P) {
            const int r = t & 15, lo = (int)(e16_rng & 0xFFu), wd = (int)((e16_rng >> 8) & 0xFFu),
                      of = (int)(e16_rng >> 16);
            constexpr bool SPL = F16_OUT16_LOOPS != 0;
            if (kp.K <= 96)
                frame16_out16<6, SPL>(kp, out, scl, priorl, lagl, f, P, pe, r, lo, wd, of);
            else
                frame16_out16<8, SPL>(kp, out, scl, priorl, lagl, f, P, pe, r, lo, wd, of);
        }
    };
    auto gate_of = [&](int64_t f) F16_AI {
        // P > 16: wave 0's lanes one lag each, a DPP sum -- thread 0 alone read
        // and summed config 4's 28 lags one after another (83.2 vs 84.0 ms per
        // step, same box; at config 3's 6 lags the DPP sum cost more: 3.300 vs
        // 3.273 ms)
        if (F16_GATEW && P > 16 && threadIdx.x < 64 && out.gate) {
            const int ln = (int)threadIdx.x;
            int tot = 0;
            for (int q = ln; q < P; q += 64)
                tot += lagl[q] * lagl[q];
            tot = group_sum_dpp(tot, 64);
            if (ln == 63)
                out.gate[f] = tot > 4 ? 1 : 0;  // sample_compute.h:124-134
        } else if ((!F16_GATEW || P <= 16) && threadIdx.x == 0 && out.gate) {
            int tot = 0;
            for (int q = 0; q < P; q++)
                tot += lagl[q] * lagl[q];
            out.gate[f] = tot > 4 ? 1 : 0;
        }
    };
    // DM 1: the epilogue's pairs w, w + 16
    int ep_lo[2] = {0, 0}, ep_w[2] = {0, 0}, ep_off[2] = {0, 0};
    if constexpr (DM == 1 && !OUT16) {
        const int w0 = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int q = w0 + 16 * h < P ? w0 + 16 * h : 0;
            ep_lo[h] = __builtin_amdgcn_readfirstlane(kp.wc_lo[q]);
            ep_w[h] = __builtin_amdgcn_readfirstlane(kp.wc_w[q]);
            ep_off[h] = __builtin_amdgcn_readfirstlane(kp.wc_off[q]);
        }
    }
#ifdef TDOA_DIAG
    constexpr int NSTAMP = 48;  // k_frame16: up to 45 phase marks (config 4: 33)
    unsigned long long stamp[NSTAMP] = {};
    unsigned long long arrive[NSTAMP] = {};
    int nst = 0, nar = 0;
    const int64_t diag_fr = blockIdx.x + (B >= (int64_t)(F16_DIAG_FRAME + 1) * gridDim.x ? F16_DIAG_FRAME : 0) *
                                             (int64_t)gridDim.x;
#else
    constexpr int64_t diag_fr = -1;
#endif
    // persistent over frames (one workgroup per CU): the next frame's words are
    // requested when the pair rounds start, so their HBM latency hides behind
    // them instead of opening every frame
    uint32_t w[8];
    auto fetch = [&](int64_t f) {
        if constexpr (RING) {
            // slot f's frame from its stream's ring: word q = j + T s holds
            // samples 2q, 2q + 1 of mic mg, ring elements ((at + n) mod cl) M + mg
            // (bytes widened as the batch frames are, or the int16 samples);
            // element loads: a ring needs no alignment beyond its sample's,
            // and a frame (C <= cl samples from at < cl) wraps at most once
            // One stream's ring is under 2^31 bytes (tdoa_f16_ring_shape's
            // caller checks it): the stream's and the mic's base is scalar and
            // a sample's byte offset one 32-bit register, dead once its load is
            // issued (64-bit indices per sample spilled)
            using T_ = typename std::conditional<PCM16, uint16_t, uint8_t>::type;
            typedef unsigned short v2us_ __attribute__((ext_vector_type(2)));
            constexpr uint32_t ST = M * sizeof(T_);  // bytes from a sample to the mic's next
            const int64_t cl = rs.capture_len;
            int sid = __builtin_amdgcn_readfirstlane(rs.ids[f]);
            sid = sid < 0 ? 0 : (sid >= rs.nstreams ? rs.nstreams - 1 : sid);
            const int64_t at64 = rs.ring_at[f];
            const uint32_t cl32 = (uint32_t)cl;
            uint32_t at = (uint32_t)__builtin_amdgcn_readfirstlane((int)(at64 < 0 ? 0 : (at64 >= cl ? cl - 1 : at64)));
            const char *cap = reinterpret_cast<const char *>(rs.capture) +
                              ((size_t)sid * (size_t)cl * M + (size_t)__builtin_amdgcn_readfirstlane(mg)) * sizeof(T_);
            const uint32_t j0 = (uint32_t)((int)threadIdx.x - g * T);
#pragma unroll
            for (int s = 0; s < 8; s++) {
                uint32_t n0 = at + 2 * (j0 + T * s);
                n0 = n0 >= cl32 ? n0 - cl32 : n0;
                const uint32_t n1 = n0 + 1 >= cl32 ? 0 : n0 + 1;
                v2us_ x;
                x.x = *reinterpret_cast<const T_ *>(cap + n0 * ST);
                x.y = *reinterpret_cast<const T_ *>(cap + n1 * ST);
                w[s] = __builtin_bit_cast(uint32_t, x);
            }
        } else {
        const uint32_t *x = reinterpret_cast<const uint32_t *>(frames + (f * M + mg) * (int64_t)C) +
                            ((int)threadIdx.x - g * T);
#pragma unroll
        for (int s = 0; s < 8; s++)
            w[s] = __builtin_nontemporal_load(x + T * s);
        }
    };
    if constexpr (RING) {
        if ((int64_t)blockIdx.x >= B)
            return;  // no listed slot for this workgroup: no ring read
    }
    fetch(blockIdx.x);
    // the next frame's words are waited for here, before this wave's output
    // stores: gfx9's vmcnt counts stores and retires in order, and with stores
    // in branches the loop head's wait for the words was vmcnt(0) -- it also
    // waited for the frame's last stores to be acknowledged (F16_PIN=0: off)
    auto pin_words = [&] {
#if F16_PIN
#pragma unroll
        for (int s = 0; s < 8; s++)
            asm volatile("" : "+v"(w[s]));
#endif
    };
#if F16_PIN
    // and every value loaded before the loop is waited for before it: a load
    // still pending on the loop's entry edge put a vmcnt(0) at the loop head,
    // which on the back edge waited for the stores
    pin_words();
#pragma unroll
    for (int s = 0; s < 8; s++)
        asm volatile("" : "+v"(wr[s]));
#if F16_TW_REG
#pragma unroll
    for (int s = 0; s < NS; s++)
        asm volatile("" : "+v"(twb[s].x), "+v"(twb[s].y));
    asm volatile("" : "+v"(twh.x), "+v"(twh.y));
#endif
#endif
    for (int64_t fr = blockIdx.x; fr < B; fr += gridDim.x) {
    // thread indices the compiler cannot prove loop-invariant: the passes'
    // twiddle reads stay in the body instead of being hoisted (and spilled)
    const int tid = opaque_idx((int)threadIdx.x), j = tid - g * T, pj = pidx(j);
    // FG: this frame's compact scores go to fgw, the previous frame's are at pgw
    float *fgw = FG ? fgl.w + (DM == 0 ? fpar * CKp : 0) : nullptr;
    const float *pgw = FG ? fgl.w + (DM == 0 ? (fpar ^ 1) * CKp : 0) : nullptr;
    const bool fgr = FG && prev >= 0 && kp.fg_ok == 1;  // (fg_ok 2: TDOA_F16_FG=skip, A/B of the bare structure)
    if (fr == diag_fr) {
#ifdef TDOA_DIAG
        stamp[NSTAMP - 2] = __builtin_amdgcn_s_memrealtime();
#endif
        F16_MARK();
    }

    // ---- 1. forward transform of mic g (k_spec16's passes in slot g)
    auto fwd_mark = [&] {
        if (fr == diag_fr)
            F16_MARK();  // the forward's barriers (diagnostic build)
    };
    auto fwd_pre = [&] {
        if (fr == diag_fr)
            F16_PRE();  // ... and the waves' arrivals at them
    };
    if constexpr (ELAG) {
        auto lag_hook = [&](int ps) F16_AI {
            if (prev >= 0)
                epi16(prev, ps);  // the previous frame's outputs (scl holds its scores until round 0's pass 3)
        };
        frame16_forward<C, WMODE, decltype(fwd_mark), XS, decltype(lag_hook), decltype(fwd_pre), PCM16>(
            w, WINL ? winl : win, wr, buf, red, tt, tid, g, j, pj, kp.log2N, fwd_mark, lag_hook, fwd_pre);
        if (prev >= 0)
            gate_of(prev);  // its lags are in lagl since the forward's closing barrier
    } else {
        frame16_forward<C, WMODE, decltype(fwd_mark), XS, NoHook16, decltype(fwd_pre), PCM16>(
            w, WINL ? winl : win, wr, buf, red, tt, tid, g, j, pj, kp.log2N, fwd_mark, NoHook16(), fwd_pre);
    }
    if (fr == diag_fr)
        F16_MARK();  // forward transforms done
    // split + unit normalisation of every mic at this thread's bin pairs:
    // X[b] = (Z[b] + Z*[C-b]) - i W_2C^b (Z[b] - Z*[C-b]), X[C-b] = conj(e + i W od)
    // (b = 0: its partner output is X[C])
    // W_2C^b of this thread's bins (the split and every pair's pre-twiddle), W_2C^{C/2}
    // (requested before the forward's last pass instead, they measured slower:
    // 4.89 vs 4.71 ms per config-3 step)
#if !F16_TW_REG
    f2 twb[NS];
#pragma unroll
    for (int s = 0; s < NS; s++)
        twb[s] = tw2[tid + 1024 * s];
    const f2 twh = tw2[C / 2];
#endif
    f2 Ub[M][NS], Un[M][NS];
#pragma unroll
    for (int s = 0; s < NS; s++) {
        const int b = tid + 1024 * s;
        const int pb = lidx<XS>(b), pp = lidx<XS>((C - b) & (C - 1));
        const f2 wb = twb[s];
#pragma unroll
        for (int m = 0; m < M; m++) {
            const f2 *zb = bufs + m * BUF;
            const f2 z = F16_LD(zb + pb), zp = F16_LD(zb + pp);
            const f2 e = c_addconj(z, zp);
            const f2 od = c_mul(c_subconj(z, zp), wb);
            Ub[m][s] = c_unit(c_add_mi(e, od), e2);
            Un[m][s] = c_unit(c_conj_add_i(e, od), e2);
        }
    }
    if constexpr (F16_PRIO != 0)
        f16_prio<2>();  // split done (F16_PRIO checkpoint)
    if (tid < M) {  // X[C/2] = conj(Z[C/2]) (x2): self-paired bin
        const f2 zh = bufs[tid * BUF + lidx<XS>(C / 2)];
        xhalf[tid] = c_unit(f2{2.0f * zh.x, -2.0f * zh.y}, e2);
    }
    // No barrier before the first round's Y stores (F16_SPLIT_BAR=0): a thread
    // stores Y only at the positions it has just read (bins b and C - b of every
    // slot), and position C / 2 -- read for X[C/2] by threads 0 .. M - 1, stored
    // by thread 0 -- stays inside wave 0, whose LDS operations are in order
#if F16_SPLIT_BAR
    if (fr == diag_fr)
        F16_PRE();
    __syncthreads();  // slots consumed: they become the pairs' buffers
    f16_prio<3>();
#endif
    if (fr == diag_fr)
        F16_MARK();  // unit spectra in registers
    // BW: the weights of this thread's bins b = tid + 1024 s and C - b, and
    // w[C / 2], requested per frame ahead of the next frame's words (they
    // return first).  LDS is full at 8 x 2048, and registers held for the
    // launch spilled in the forward, where the lagged epilogue runs
    float bwk[NS] = {}, bwn[NS] = {}, bwh = 0.0f;
    if constexpr (BW) {
        // (the table's address through the opaque kernarg pointer: read here,
        // not held in scalar registers across the frame loop)
        const float *bwt = kernarg_kp()->bin_w;
#pragma unroll
        for (int s = 0; s < NS; s++) {
            bwk[s] = bwt[tid + 1024 * s];
            bwn[s] = bwt[C - (tid + 1024 * s)];
        }
        bwh = bwt[C / 2];
    }
    {
        const int64_t fn = fr + gridDim.x;
        fetch(fn < B ? fn : fr);  // the next frame's words (or a harmless re-read)
    }

    // ---- 2. pairs, G per round (rounds and pair slots unrolled: every
    // register index below is a compile-time constant)
    const float invL = 1.0f / (float)(2 * C);
    static_for<0, ROUNDS>([&](auto rc) {
        constexpr int p0 = decltype(rc)::value * G;
        const int tl = opaque_idx(tid), jl = tl - g * T, pjl = pidx(jl);
        const ColIdx<C, XS> cjl(jl);
        // this thread's Y slots b = tl + 1024 s and C - b (b = 0: C / 2, whose
        // value thread 0 writes after, in program order)
        int yb0[NS], yb1[NS];
#pragma unroll
        for (int s = 0; s < NS; s++) {
            const int b = tl + 1024 * s;
            yb0[s] = lidx<XS>(b);
            yb1[s] = b == 0 ? lidx<XS>(C / 2) : lidx<XS>(C - b);
        }
        // packed inverse input Y of pair p0 + gg into buffer gg (all threads)
        static_for<0, G>([&](auto gc) {
            constexpr int pc = p0 + decltype(gc)::value;
            if constexpr (F16_PRIO != 0 && decltype(gc)::value == G / 2)
                f16_prio<1>();
            if constexpr (pc < P) {
                constexpr int pi = pair_first<M>(pc), pj = pair_second<M>(pc);
                f2 *yb = bufs + decltype(gc)::value * BUF;
#pragma unroll
                for (int s = 0; s < NS; s++) {
                    f2 Rk = c_conjmul(Ub[pi][s], Ub[pj][s]);  // R[b]
                    f2 Rq = c_conjmul(Un[pi][s], Un[pj][s]);  // R[C-b]
                    if constexpr (BW) {
                        Rk = bwk[s] * Rk;
                        Rq = bwn[s] * Rq;
                    }
                    const f2 ss = c_addconj(Rk, Rq);
                    const f2 qq = c_mulconj(c_subconj(Rk, Rq), twb[s]);
                    yb[yb0[s]] = c_add_i(ss, qq);
                    yb[yb1[s]] = c_conj_add_mi(ss, qq);
                }
                if (!F16_YHALF && tl == 0) {  // Y[C/2] from R[C/2] alone
                    f2 Rh = c_conjmul(xhalf[pi], xhalf[pj]);
                    if constexpr (BW)
                        Rh = bwh * Rh;
                    yb[lidx<XS>(C / 2)] = c_add_i(c_addconj(Rh, Rh), c_mulconj(c_subconj(Rh, Rh), twh));
                }
            }
        });
#if F16_YHALF
        // Y[C/2] of the round's pairs, lane gg of wave 0 for pair p0 + gg: one
        // branch instead of one per pair on thread 0 (wave 0 ran ~1.1 k cycles
        // longer than its SIMD's other waves in every Y interval).  Wave 0 as
        // before: its LDS operations are in order -- X[C/2] (xhalf) was written by
        // its threads 0 .. M - 1 after they read Z[C/2] at the positions
        // written here, and thread 0's stores above put the partner value there first
        if (tl < G && p0 + tl < P) {
            const int pc = p0 + tl;
            int pi = 0, q = pc;
            while (q >= M - 1 - pi) {  // pair_first / pair_second at run time
                q -= M - 1 - pi;
                pi++;
            }
            f2 Rh = c_conjmul(xhalf[pi], xhalf[pi + 1 + q]);
            if constexpr (BW)
                Rh = bwh * Rh;
            bufs[tl * BUF + lidx<XS>(C / 2)] = c_add_i(c_addconj(Rh, Rh), c_mulconj(c_subconj(Rh, Rh), twh));
        }
#endif
        if (fr == diag_fr)
            F16_PRE();
        __syncthreads();
        f16_prio<3>();
        if (fr == diag_fr)
            F16_MARK();  // the round's Y buffers written
        const int p = p0 + g;
        const bool pair_on = p < P;
        // inverse pass 1 (radix 16, Ns = 1)
        // a partial last round (P mod G pairs): the idle groups skip the
        // transforms, leaving their SIMDs' issue slots to the busy groups
        const bool on = p0 + G <= P || pair_on;
        f2 v[16];
        if (on) {
#pragma unroll
            for (int r = 0; r < 16; r++)
                v[r] = F16_LD(buf + (XS ? cjl.at(r) : pjl + po(T * r)));
            dftp<16, true, false, F16_PRIO>(v);
        }
        // FG, last round: the idle groups' waves solve the previous frame's grid
        constexpr bool FGL = FG && decltype(rc)::value == ROUNDS - 1;
        const int gw = (tl - GI0 * T) >> 6, gln = tl & 63;
        uint4 fqr[4];
        if constexpr (FGL) {
            if (!on && fgr)
                fgg.levels(pgw, gw, gln, fqr);  // seg A
        }
        if (fr == diag_fr)
            F16_PRE();
        __syncthreads();
        f16_prio<3>();
        if (fr == diag_fr)
            F16_MARK();
        if (on) {
            const int b1 = 16 * jl | (jl & 15);  // xs(16 jl + r) = b1 ^ r
#pragma unroll
            for (int r = 0; r < 16; r++)
                buf[XS ? (b1 ^ r) : 17 * jl + r] = v[brev<16>(r)];
        }
        if constexpr (FGL) {
            if (!on && fgr)
                fgg.bounds(pgw, gw, gln, fqr);  // seg B
        }
        if (fr == diag_fr)
            F16_PRE();
        __syncthreads();
        f16_prio<3>();
        if (fr == diag_fr)
            F16_MARK();
        // pass 2: outputs r'' in {0, 1, 14, 15} only
        const int k = jl & 15;
        f2 x0 = f2{0, 0}, x1 = f2{0, 0}, x14 = f2{0, 0}, x15 = f2{0, 0};
#define F16_TW256(r) F16_LD(tt + 16 * (r) + k)
        if (on)
#pragma unroll
        for (int r = 0; r < 4; r++) {  // inputs r, r + 4, r + 8, r + 12 at a time
            if (r == 2)
                f16_prio<1>();
            f2 l0 = F16_LD(buf + (XS ? cjl.at(r) : pjl + po(T * r)));
            f2 l1 = F16_LD(buf + (XS ? cjl.at(r + 4) : pjl + po(T * (r + 4))));
            const f2 h0 = c_mulconj(F16_LD(buf + (XS ? cjl.at(r + 8) : pjl + po(T * (r + 8)))), F16_TW256(r + 8));
            const f2 h1 = c_mulconj(F16_LD(buf + (XS ? cjl.at(r + 12) : pjl + po(T * (r + 12)))), F16_TW256(r + 12));
            if (r)
                l0 = c_mulconj(l0, F16_TW256(r));  // tw256
            l1 = c_mulconj(l1, F16_TW256(r + 4));
            const f2 a0 = l0 + h0, a1 = l1 + h1;
            const f2 d0 = dif_tw<true>(l0, h0, 2 * r), d1 = dif_tw<true>(l1, h1, 2 * (r + 4));
            x0 = x0 + (a0 + a1);
            x1 = x1 + (d0 + d1);
            x14 = x14 + (r ? dif_tw<false>(a0, a1, 4 * r) : a0 - a1);
            x15 = x15 + (r ? dif_tw<false>(d0, d1, 4 * r) : d0 - d1);
        }
#undef F16_TW256
        uint64_t fgk = 0;
        int fgc = -1;
        if constexpr (FGL) {
            if (!on && fgr)
                fgk = fgg.candidate(pgw, gw, gln, fgc);  // seg C
        }
        // XS: the four outputs go to this thread's own column rows 0-3 (element
        // jl + T c for output c), positions no other thread reads in this pass:
        // no barrier between the pass's reads and its stores.  Padded layout:
        // element 64 a + 16 c + k (a = jl >> 4), after a barrier
        if constexpr (!XS) {
            if (fr == diag_fr)
                F16_PRE();
            __syncthreads();
            f16_prio<3>();
        }
        if (fr == diag_fr)
            F16_MARK();
        if (on) {
            if constexpr (XS) {
                buf[cjl.at(0)] = x0;
                buf[cjl.at(1)] = x1;
                buf[cjl.at(2)] = x14;
                buf[cjl.at(3)] = x15;
            } else {
                const int o = pidx((jl >> 4) * 64 + k);
                buf[o] = x0;
                buf[o + 17] = x1;
                buf[o + 34] = x14;
                buf[o + 51] = x15;
            }
        }
        if constexpr (FGL) {
            if (!on && fgr && gln == 0) {  // seg D
                fgl.key[gw] = fgk;
                fgl.cand[gw] = fgc;
            }
        }
        if (fr == diag_fr)
            F16_PRE();
        __syncthreads();
        f16_prio<3>();
        if (fr == diag_fr)
            F16_MARK();
        // pass 3 by one wave of the group, one output per column.  Waves of a
        // workgroup go to SIMD (wave index mod 4): the group's wave P3W lands
        // the G pass-3 waves evenly on the four SIMDs (the group's first wave
        // put them all on SIMD 0, or 0 and 2, one after another)
        if constexpr (DM == 0 && decltype(rc)::value == 0)
            pin_words();  // every wave, before the first round's output stores
        if ((jl >> 6) == P3W && pair_on) {
            const int l = jl & 63;
            const int mm = 64 - l;
            // column 192 + l (l >= 32): W_C^{-r (192 + l)} term == W_C^{r (64 - l)} after
            // the output index C - m; tw3 holds each lane's factors (conjugated for l < 32)
            // term r of lane l = 16 c + k: output c of pass-2 thread 16 r + k.  XS:
            // element 16 r + k + T c, xs = (T c + 16 r) | (k ^ ((r + (T / 16) c) & 15));
            // padded: element l + 64 r, pidx = pidx(l) + 68 r
            const int pl = lidx<XS>(l);
            const int c3 = l >> 4, k3 = l & 15;
            auto p3pos = [&](int r) {
                return XS ? ((T * c3 + 16 * r) | (k3 ^ ((r + (T / 16) * c3) & 15))) : pl + 68 * r;
            };
            // the R1 terms summed as a tree (a running sum was a dependent
            // chain of R1 - 1 complex products and adds on the round's critical path)
            f2 t[R1];
            t[0] = F16_LD(buf + p3pos(0));
#pragma unroll
            for (int r = 1; r < R1; r++)
                t[r] = c_mul(F16_LD(buf + p3pos(r)), F16_LD(tw3 + 64 * r + l));
#pragma unroll
            for (int h = R1 / 2; h >= 1; h >>= 1)
#pragma unroll
                for (int r = 0; r < h; r++)
                    t[r] = t[r] + t[r + h];
            const f2 y = t[0];
            const int n = l < 32 ? l : -mm;
            const int ka = 2 * n + S, kb = 2 * n + 1 + S;
            const bool oka = ka >= 0 && ka < K, okb = kb >= 0 && kb < K;
            const float sa = y.x * invL, sb = y.y * invL;
            constexpr int RI = decltype(rc)::value;
            if constexpr (DM == 1) {
                if (oka)
                    scl[p * K + ka] = sa;
                if (okb)
                    scl[p * K + kb] = sb;
            } else {
                const int pp[1] = {p}, lo[1] = {rl_lo[RI]}, wd[1] = {rl_w[RI]}, of[1] = {rl_off[RI]};
                const bool on1[1] = {true};
                const float a1[1] = {sa}, b1[1] = {sb};
                if (!F16_NO_OUT)
                frame16_pair_out<1>(kp, out, priorl, lagl, fr, P, pp, on1, ka, kb, oka, okb, a1, b1, l == 0, lo, wd,
                                    of, fgw);
            }
        }
        if constexpr (FGL) {
            if (!on && fgr) {  // seg E
                const uint64_t kk = fgg.rest(pgw, gw, gln);
                if (gln == 0)
                    fgl.key[FG_NGW + gw] = kk;
            }
        }
        if (fr == diag_fr)
            F16_PRE();
        __syncthreads();  // the buffers are rewritten by the next round
        f16_prio<3>();
        if (fr == diag_fr)
            F16_MARK();
    });
    if constexpr (FG) {
        if (fgr && tid == 0)
            fgg.finish(prev);  // the previous frame's cell, max L, (x, y)
    }
    if constexpr (DM == 1) {
        // every pair's argmax and outputs, wave w: pairs w, w + 16 (lane l:
        // lags l and l + 64, K <= 127)
        const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), ln = tid & 63;
        static_assert(P <= 32, "two epilogue pairs per wave at most");
        if constexpr (OUT16) {
            // waves 0 .. ceil(P / 4) - 1, four pairs each (rows past P idle);
            // ELAG: in the next frame's forward (or after the loop) instead
            if constexpr (!ELAG) {
                pin_words();
                epi16(fr, 0);
            }
        } else {
        const bool oka = ln < K, okb = ln + 64 < K;
        const int pp[2] = {wv, wv + 16 < P ? wv + 16 : wv};
        const bool on2[2] = {wv < P, wv + 16 < P};
        float sa[2], sb[2];
#pragma unroll
        for (int h = 0; h < 2; h++) {
            sa[h] = oka ? scl[pp[h] * K + ln] : 0.0f;
            sb[h] = okb ? scl[pp[h] * K + ln + 64] : 0.0f;
        }
        pin_words();
        if (on2[0])
            frame16_pair_out<2>(kp, out, priorl, lagl, fr, P, pp, on2, ln, ln + 64, oka, okb, sa, sb, ln == 0, ep_lo,
                                ep_w, ep_off, fgw);
        }
        if constexpr (!ELAG) {
            if (fr == diag_fr)
                F16_PRE();
            __syncthreads();  // lagl complete for the gate; scl free for the next frame
            f16_prio<3>();
            if (fr == diag_fr)
                F16_MARK();
        }
    }
    pin_words();
    if constexpr (!ELAG)
        gate_of(fr);
    prev = fr;
    fpar ^= 1;
#ifdef TDOA_DIAG
    if (fr == diag_fr) {
        stamp[NSTAMP - 1] = __builtin_amdgcn_s_memrealtime();
        stamp[NSTAMP - 3] = __builtin_amdgcn_s_memtime();
    }
#endif
    }  // frames
    if constexpr (ELAG) {
        // the last frame's outputs (its last round closed with a barrier: scl complete)
        if (prev >= 0) {
            epi16(prev, 0);
            __syncthreads();
            gate_of(prev);
        }
#ifdef F16_RNG_DUMP
        // diagnostic builds only: every thread's packed compact range over the
        // first 1024 lag slots (tools/diag_rng.py)
        __syncthreads();
        if (blockIdx.x == 0)
            out.lags[threadIdx.x] = (int32_t)e16_rng;
#endif
    }
    if constexpr (FG) {
        // the last frame's grid, by waves 0 .. FG_NGW - 1 (every buffer is free)
        if (prev >= 0 && kp.fg_ok == 1) {
            const int tid = (int)threadIdx.x, gw = tid >> 6, gln = tid & 63;
            const bool act = gw < FG_NGW;
            const float *pgw = fgl.w + (DM == 0 ? (fpar ^ 1) * CKp : 0);  // (fpar toggled after the last frame)
            uint4 fqr[4];
            __syncthreads();  // the last frame's scores are in LDS
            if (act)
                fgg.levels(pgw, gw, gln, fqr);
            __syncthreads();
            if (act)
                fgg.bounds(pgw, gw, gln, fqr);
            __syncthreads();
            int fgc = -1;
            uint64_t fgk = 0;
            if (act)
                fgk = fgg.candidate(pgw, gw, gln, fgc);
            if (act && gln == 0) {
                fgl.key[gw] = fgk;
                fgl.cand[gw] = fgc;
            }
            __syncthreads();
            if (act) {
                const uint64_t kk = fgg.rest(pgw, gw, gln);
                if (gln == 0)
                    fgl.key[FG_NGW + gw] = kk;
            }
            __syncthreads();
            if (tid == 0)
                fgg.finish(prev);
        }
    }
#ifdef TDOA_DIAG
    if ((threadIdx.x & 63) == 0 && blockIdx.x < 64)
        for (int i = 0; i < NSTAMP; i++) {
            g_diag_f16[(blockIdx.x * 16 + (threadIdx.x >> 6)) * NSTAMP + i] = stamp[i];
            g_diag_f16b[(blockIdx.x * 16 + (threadIdx.x >> 6)) * NSTAMP + i] = arrive[i];
        }
#endif
