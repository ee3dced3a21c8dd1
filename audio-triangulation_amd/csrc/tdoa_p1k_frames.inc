// tdoa_p1k_frames.inc -- the body of the config-2 GCC-PHAT kernels of
// tdoa_phat1024.hip, included once per kernel: k_p1k_lean<NW> (8-bit ADC front
// end) and k_p1k_pcm16 (TDOA_SAMPLES_PCM16).  It reads the kernel's parameters
// (kp, out, frames, B, e2) and the constants NW and PCM16 of the including
// scope; the two formats differ in lean_spectrum's front-end block alone.
// Text rather than a __device__ function: inlined from one, k_p1k_lean<4>'s
// hand-tuned schedule came out different (the callee is simplified on its own,
// without the kernel's work-group size, before it is inlined).
    static_assert(NW == 4 || NW == 8, "k_p1k_lean: 4 or 8 waves per workgroup");
    static_assert(!PCM16 || NW == 4, "the PCM16 form exists for the product's workgroup shape");
    constexpr int N = 1024, P = 3, NF = 2 * NW, NT = NW * 64;
    constexpr bool WG4 = NW == 4;
    constexpr bool PRUNE = WG4 && P1K_GRID_PRUNE;
    // the LDS read depths per call site (tdoa_phat1024.hip, P1K_TWM_* ...):
    // R in the four roomy transforms, T in the two at the register peak
    constexpr int TWM_R = PCM16 ? P1K_TWM_ROOMY_PCM16 : P1K_TWM_ROOMY, TWM_T = PCM16 ? P1K_TWM_TIGHT_PCM16 : P1K_TWM_TIGHT;
    constexpr int TW2_R = PCM16 ? P1K_TW2_ROOMY_PCM16 : P1K_TW2_ROOMY, TW2_T = PCM16 ? P1K_TW2_TIGHT_PCM16 : P1K_TW2_TIGHT;
    constexpr int ROW_R = PCM16 ? P1K_ROW_ROOMY_PCM16 : P1K_ROW_ROOMY;
    static_assert(TW2_T == 1 || TW2_T == 2, "the transforms at the register peak keep their twiddles one pair ahead");
    static_assert(!WG4 || NW * P1K_WAVE_LDS + P1K_IMG_LDS4 <= 80 * 1024, "two workgroups must fit a CU's 160 KiB of LDS");
    static_assert(!WG4 || !P1K_GROUPS, "the grouped scan reads its words from LDS");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char *tiles = smem;                               // [NW][2][TILE]
    char *twm = tiles + NW * 2 * P1K_TILE;            // [32][32] f2
    char *tw2 = twm + 32 * 32 * 8;                    // [16][32] f2
    const float *prior = (const float *)(tw2 + 16 * 32 * 8);  // [128]
    char *win = (char *)(prior + 128);                // [512] f2 (NW = 8 only)
    // the tuple words: after the window in LDS, or in the global image
    const uint32_t *tups = WG4 ? (const uint32_t *)((const char *)kp.p1k_img + P1K_IMG_FIXED)
                               : (const uint32_t *)(win + 512 * 8);

    const int tid = threadIdx.x, wave = tid >> 6, hw = (tid >> 5) & 1, lane64 = tid & 63;
#ifdef TDOA_DIAG
    // diagnostic build only: absolute s_memtime per phase of the first iteration
    unsigned long long stamp[16] = {};
    int nst = 0;
#define LEAN_MARK()                                               \
    do {                                                          \
        if (nst < 16)                                             \
            stamp[nst++] = __builtin_amdgcn_s_memtime();          \
    } while (0)
    stamp[nst++] = __builtin_amdgcn_s_memtime();
    stamp[14] = __builtin_amdgcn_s_memrealtime();  // 100 MHz constant clock
#else
#define LEAN_MARK() \
    do {            \
    } while (0)
#endif
    // issue balance between the two waves of a SIMD (waves w and w ^ 4: a
    // workgroup's waves are dealt to the CU's four SIMDs in turn).  The SIMD
    // issues oldest-first, so without this wave w runs ahead and wave w ^ 4
    // finishes its last ~9 us alone, with nothing to hide its latencies; here
    // a wave that has passed more phase boundaries than its partner drops to
    // the low priority until the partner catches up
    // (NW = 4 has none of this: a wave's SIMD partner belongs to another
    // workgroup, and the default priority leaves the issue oldest-first)
    __shared__ int prog[WG4 ? 1 : NW];
    if constexpr (!WG4) {
        if (lane64 == 0)
            prog[wave] = 0;
        __builtin_amdgcn_s_setprio(2);
    }
#if P1K_WG4_PRIO
    if constexpr (WG4)
        __builtin_amdgcn_s_setprio(3);
#endif
    int phase = 0;
    auto balance = [&]() {
        // through an LDS-address-space pointer: ds_write / ds_read.  A generic
        // volatile pointer made them flat accesses, and the flat load's wait
        // (vmcnt(0) lgkmcnt(0)) also waited for the next mic's words in flight
#if P1K_BALANCE
        if constexpr (!WG4) {
            volatile __attribute__((address_space(3))) int *pv = (volatile __attribute__((address_space(3))) int *)prog;
            ++phase;
            if (lane64 == 0)
                pv[wave] = phase;
            const int other = __builtin_amdgcn_readfirstlane(pv[wave ^ 4]);
            if (phase > other)
                __builtin_amdgcn_s_setprio(0);
            else
                __builtin_amdgcn_s_setprio(2);
        }
#endif
    };
    Lane L;
    L.hw = hw;
    L.lane = tid & 31;
    L.res = lane_res(L.lane);
    L.cs = slot(L.res);
    L.is0 = L.lane == 0;
    L.is1 = L.lane == 1;
    char *wtiles = tiles + wave * 2 * P1K_TILE;
    L.tileA = wtiles + hw * P1K_TILE;
    L.twm = twm;
    L.tw2 = tw2;
    L.win = win;

    const int K = kp.K, S = kp.S;
    const bool do_grid = out.cell || out.xy || out.max_Lf;
#if !P1K_GROUPS
    const int Upad = p1k_upad(kp.U);
#endif

    constexpr int NQ = WG4 ? 16 : 1;  // (NW = 8: one unused word)
    auto fetch_win = [&](uint32_t(&q)[NQ]) {
        if constexpr (WG4) {  // the window's taps of the same samples (L2 hits)
            const uint32_t *wq = reinterpret_cast<const uint32_t *>(kp.window) + L.res;
#pragma unroll
            for (int t = 0; t < 16; t++)
                q[t] = wq[32 * t];
        }
    };
    auto fetch = [&](uint32_t(&w)[16], uint32_t(&q)[NQ], int64_t fr, int m, bool win = true) {
        const uint32_t *row = reinterpret_cast<const uint32_t *>(
            frames + ((fr < B ? fr : B - 1) * 3 + m) * (int64_t)N) + L.res;
#pragma unroll
        for (int t = 0; t < 16; t++)
            w[t] = __builtin_nontemporal_load(row + 32 * t);
        if (win)
            fetch_win(q);
    };
    // table image: its loads first (L2 hits), then the first frames' words
    // (HBM), then the image's LDS writes -- the frames' latency overlaps the
    // staging instead of following it
    uint32_t w0[16], w1[16];
    [[maybe_unused]] uint32_t q0[NQ] = {}, q1[NQ] = {};
    {
        const uint4 *src = (const uint4 *)kp.p1k_img;
        uint4 *dst = (uint4 *)twm;
        const int n16 = WG4 ? P1K_IMG_LDS4 / 16 : (do_grid ? p1k_img_lds8(kp) / 16 : P1K_IMG_FIXED / 16);
        constexpr int SR = 4;  // image <= SR * NT * 16 B = 32 KiB (tdoa_phat1024_fits)
        uint4 img[SR];
#pragma unroll
        for (int r = 0; r < SR; r++)  // unconditional (clamped) loads: straight-line
            img[r] = src[tid + r * NT < n16 ? tid + r * NT : n16 - 1];  // code, counted waits
        const int64_t f = (int64_t)blockIdx.x * NF + 2 * wave + hw;
        fetch(w0, q0, f, 0);
#pragma unroll
        for (int r = 0; r < SR; r++)  // unconditional too (a clamped index rewrites
            dst[tid + r * NT < n16 ? tid + r * NT : n16 - 1] = img[r];  // the last unit)
    }
    __syncthreads();
    // keep the first row's use (and its wait) below the barrier: hoisted above
    // it, every wave of the workgroup would wait for the latest wave's row
#if P1K_WG4_PRIO
    if constexpr (WG4)
        __builtin_amdgcn_s_setprio(0);
#endif
#pragma unroll
    for (int t = 0; t < 16; t++)
        asm volatile("" : "+v"(w0[t]));
    if constexpr (WG4) {
#pragma unroll
        for (int t = 0; t < 16; t++)
            asm volatile("" : "+v"(q0[t]));
    }

    const float invL = 1.0f / 2048.0f;

    // one iteration per workgroup (grid = ceil(B / NF)): no value lives across
    // a loop back-edge, which the register allocator answered with spills
    {
        const int64_t base = (int64_t)blockIdx.x * NF;
        const int64_t f = base + 2 * wave + hw;
        const bool live = f < B;
        uint32_t w2[16];
        [[maybe_unused]] uint32_t q2[NQ] = {};
        LEAN_MARK();
        float wv[3][4];
        int best[3];
        // the pruned scan's per-pair term: an upper bound of the pair's weighted
        // scores, per frame of the wave (uniform values: scalar registers)
        [[maybe_unused]] float pm[3][2] = {};
        auto finish_pair = [&](int p, f2 y0, f2 y31) {
            // this lane's four candidate lags (recomputed here, see fresh_tid)
            const int ft = fresh_tid();
            const int fres = lane_res_sel(ft & 31), fhw = (ft >> 5) & 1;
            const int la = 2 * fres, lb = 2 * fres - 64;
            const int ck[4] = {lb + S, lb + 1 + S, la + S, la + 1 + S};
            const bool ok[4] = {lb >= -S, lb + 1 >= -S, la <= S, la + 1 <= S};
            const float cv[4] = {y31.x * invL, y31.y * invL, y0.x * invL, y0.y * invL};
            // the lane's first maximum of its candidates (ascending lags), then
            // the half-wave's (correlations.c:20-23 first max) by keys
            int bkey = INT_MIN, bk = INT_MAX;
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const int kc = fkey(cv[c]);
                if (ok[c] && kc > bkey) {
                    bkey = kc;
                    bk = ck[c];
                }
            }
            half_argmax_key(bkey, bk);  // every lane of the half-wave
            if constexpr (PRUNE) {
                // M = max(raw maximum, 0) >= every weighted score of the pair, in
                // float, without another reduction: a weighted score is
                // fl(c * s) with c the raw score and 0 <= s <= 1 a prior value
                // (exp of a non-positive float; s = 1 exactly at distance 0).
                // c >= 0: c * s <= c, and rounding is monotone with c itself
                // representable, so fl(c * s) <= c <= raw maximum.  c < 0:
                // c * s <= 0, so fl(c * s) <= 0.  Where the raw maximum is >= 0
                // it is its own weighted score (s = 1 at the best lag) and M is
                // the exact maximum; where every score is negative, weighting
                // moves scores toward zero and only 0 bounds them.
                const int mb = __builtin_bit_cast(int, fmaxf(fkey_value(bkey), 0.0f));
                pm[p][0] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(mb, 0));
                pm[p][1] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(mb, 32));
            }
            bk = bk < 0 ? 0 : (bk >= K ? K - 1 : bk);
            best[p] = bk - S;
            const int64_t ff = base + 2 * ((ft >> 6) & (NW - 1)) + fhw;
#if P1K_PRIOR_AHEAD
            // the four prior values in one LDS round trip: volatile reads at a
            // clamped index (d <= 127 for a candidate in range), so none sits
            // in an exec-masked branch with a wait of its own
            float pr[4];
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const int d = ck[c] > bk ? ck[c] - bk : bk - ck[c];
                pr[c] = __builtin_bit_cast(float, lds_rd_u32(reinterpret_cast<const uint32_t *>(prior) + (ok[c] ? d : 0)));
            }
#pragma unroll
            for (int c = 0; c < 4; c++)
                wv[p][c] = ok[c] ? cv[c] * pr[c] : 0.0f;
#else
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const int d = ck[c] > bk ? ck[c] - bk : bk - ck[c];
                wv[p][c] = ok[c] ? cv[c] * prior[ok[c] ? d : 0] : 0.0f;
            }
#endif
            if (out.scores_f || out.weighted_f) {  // debug / parity outputs (uniform branch)
                float *sr = out.scores_f ? out.scores_f + (size_t)(ff * P + p) * K : nullptr;
                float *wr = out.weighted_f ? out.weighted_f + (size_t)(ff * P + p) * K : nullptr;
#pragma unroll
                for (int c = 0; c < 4; c++)
                    if (ff < B && ok[c]) {
                        if (sr)
                            sr[ck[c]] = cv[c];
                        if (wr)
                            wr[ck[c]] = wv[p][c];
                    }
            }
#if !P1K_LATE_STORES
            if (ff < B && (ft & 31) == 0)
                out.lags[ff * P + p] = bk - S;
#endif
        };

        f2 U0[33], U1[33], y0, y31;
        // the mics' rows are requested one at a time, each after the previous
        // one's front end: at the kernel's start the memory system serves every
        // wave's first row (8 MB) instead of all rows at once
        lean_forward<PCM16, TWM_R, TW2_R>(L, w0, q0, U0, e2, [&] {
            fetch(w1, q1, f, 1);
            balance();
        });
        LEAN_MARK();
        balance();
#if P1K_W2_EARLY
        lean_forward<PCM16, TWM_R, TW2_R>(L, w1, q1, U1, e2, [&] {
            fetch(w2, q2, f, 2);
            balance();
        });
#else
        lean_forward<PCM16, TWM_R, TW2_R>(L, w1, q1, U1, e2, [&] { balance(); });
#endif
        LEAN_MARK();
        balance();
        {
            f2 v[32];
            lean_pretwiddle<true, TW2_T>(L, U0, U1, v);  // pair 0: (0, 1)
            fft_col_lds<true, false, TWM_T>(L, v, L.tileA);
#if !P1K_W2_EARLY
            // mic 2's words: fetched after the pair's column pass, the kernel's
            // register peak (two unit spectra + a working column)
            fetch(w2, q2, f, 2, !P1K_WG4_WQ_LATE);
#endif
            lean_row_inv<16>(L, L.tileA, y0, y31);
        }
        finish_pair(0, y0, y31);
#if P1K_WG4_WQ_LATE
        fetch_win(q2);
#endif
        LEAN_MARK();
        balance();
        lean_forward_cross<PCM16, TWM_T, TW2_T>(L, w2, q2, U0, U1, e2);  // pairs 1: (0, 2), 2: (1, 2)
        LEAN_MARK();
        balance();
        {
            f2 v[32];
            lean_pretwiddle<false, TW2_R>(L, U0, U0, v);
            fft_col_lds<true, false, TWM_R>(L, v, L.tileA);
            lean_row_inv<ROW_R>(L, L.tileA, y0, y31);
        }
        finish_pair(1, y0, y31);
        LEAN_MARK();
        balance();
        {
            f2 v[32];
            lean_pretwiddle<false, TW2_R>(L, U1, U1, v);
            fft_col_lds<true, false, TWM_R>(L, v, L.tileA);
            lean_row_inv<ROW_R>(L, L.tileA, y0, y31);
        }
        finish_pair(2, y0, y31);
        LEAN_MARK();
        balance();
        // the frame's lags and gate (sample_compute.h:124-134): stored last
        // unless P1K_LATE_STORES=0.  gfx9's vmcnt counts stores too, and the
        // grid's one global load (the winner's first cell) waits in issue
        // order: behind these stores it waited for their HBM write acks
        auto store_frame = [&]() {
            if constexpr (WG4) {
                // the frame index from the lane id again (fresh_tid): held from
                // the kernel's start it cost the register that spilled
                const int ft = fresh_tid();
                const int64_t fq = base + 2 * ((ft >> 6) & (NW - 1)) + ((ft >> 5) & 1);
                if (fq < B && (ft & 31) == 0) {
#pragma unroll
                    for (int p = 0; p < 3; p++)
                        out.lags[fq * P + p] = best[p];
                    if (out.gate)
                        out.gate[fq] = best[0] * best[0] + best[1] * best[1] + best[2] * best[2] > 4 ? 1 : 0;
                }
                return;
            }
            if (live && L.lane == 0) {
#pragma unroll
                for (int p = 0; p < 3; p++)
                    out.lags[f * P + p] = best[p];
                if (out.gate)
                    out.gate[f] = best[0] * best[0] + best[1] * best[1] + best[2] * best[2] > 4 ? 1 : 0;
            }
        };
#if !P1K_LATE_STORES
        store_frame();
#endif
        if (!do_grid) {
#if P1K_LATE_STORES
            store_frame();
#endif
            return;
        }
        // ---- grid solve (vga_heatmap.h:99-108) of the wave's two frames:
        // weighted scores [p][KPAD] f2 (frame hw in component hw) in the wave's
        // tile space, lanes split the distinct lag tuples (4 consecutive per
        // lane and step, ascending: a strict '>' keeps the first maximum)
#if P1K_WG4_PRIO
        if constexpr (WG4)
            __builtin_amdgcn_s_setprio(3);
#endif
        wave_lds_sync();  // after the last pair's row reads of these tiles
        // the pruned scan's row table (after the tuple words in the global
        // image): its header and this lane's row record, requested here so the
        // L2 round trip passes under the score writes below
#if P1K_GRID_PRUNE
        [[maybe_unused]] const uint32_t *ps = nullptr;
        [[maybe_unused]] uint32_t prows = 0, ppair = 0, pwid = 0, prec = 0;
        [[maybe_unused]] int pcell0 = 0;
        if constexpr (PRUNE) {
            ps = tups + Upad;
            prows = ps[0];
            ppair = ps[1];
            pwid = ps[2];
            pcell0 = (int)ps[3];
            prec = ps[TDOA_P1K_PRUNE_HDR + lane64];
        }
#endif
#if P1K_CELL_LDS && !P1K_GROUPS
        // [P][KPAD][2], 1 KiB-aligned in the wave's tiles: a gather address is
        // then one and-or of a tuple field with the table base
        float *wsc = (float *)(((uintptr_t)wtiles + 1023) & ~(uintptr_t)1023);
#else
        float *wsc = (float *)wtiles;  // [P][KPAD][2]
#endif
        const int gres = lane_res_sel(fresh_tid() & 31);
        const int gla = 2 * gres, glb = 2 * gres - 64;
        const int ck[4] = {glb + S, glb + 1 + S, gla + S, gla + 1 + S};
        const bool ok[4] = {glb >= -S, glb + 1 >= -S, gla <= S, gla + 1 <= S};
#pragma unroll
        for (int p = 0; p < P; p++)
#pragma unroll
            for (int c = 0; c < 4; c++)
                if (ok[c])
                    wsc[(p * P1K_KPAD + ck[c]) * 2 + hw] = wv[p][c];
        {
            const int ft = fresh_tid();  // (lane, half-wave) not held across the phases
            if ((ft & 31) < 3)  // lag slot 127 of every pair: the padding tuple
                wsc[((ft & 31) * P1K_KPAD + P1K_KPAD - 1) * 2 + ((ft >> 5) & 1)] = -INFINITY;
        }
        wave_lds_sync();  // the gathers read other lanes' score slots
        LEAN_MARK();
        float gv[2] = {-INFINITY, -INFINITY};
        int wcell[2];
        // the exhaustive scan runs: always without the pruned scan, and with it
        // where the row bounds prune too little to pay for themselves (below)
        bool full = !PRUNE;
#if P1K_GRID_PRUNE
        if constexpr (PRUNE) {
            // Pruned scan, exact.  The image holds the tuples sorted by the lag
            // of one pair p (ties in first-cell order) in rows of 64, one tuple
            // per lane, each with its first cell, and per row the range
            // [lo, hi] of pair p's lag slots.  For a frame, with w_q the
            // weighted scores of pair q and M_q >= max w_q (finish_pair),
            //   bound(row) = (t0 + t1) + t2,  t_p = max w_p[lo..hi],  t_q = M_q,
            // summed in L's own order and association.  Every tuple of the row
            // has w_q[l_q] <= t_q, and a rounded float sum never decreases when
            // a term grows, so bound >= the float L of each of its tuples: a row
            // with bound < (an L already found) holds neither the maximum nor a
            // tie with it.  Only a true '<' skips a row, so a NaN on either side
            // skips nothing (v_max drops a NaN score: its tuples' L is NaN and
            // never wins).  The lag prior makes w_p a narrow bump, so few rows
            // pass (~4 of 39 on ADC frames; all of them on uncorrelated noise).
            // Order: lane r bounds row r for both frames.  Pass 1 scans the rows
            // that have either frame's largest bound (the rows whose range holds
            // pair p's best lag: one to three a frame, and on ADC frames the
            // maximum is nearly always among them); pass 2 the rows whose bound
            // is not below either frame's best of pass 1 (usually none).  A pass
            // scans its rows four at a time, each batch's words and cells
            // requested (clamped, unguarded, no store before them) ahead of the
            // previous batch's gathers.  Sorted order is not first-cell order,
            // so every compare carries the cell: larger L, or equal L and a
            // smaller cell.
            // Flat scores (uncorrelated microphones) leave most rows to pass 2,
            // whose rows cost about twice the exhaustive scan's per tuple (the
            // cell words and compares): when pass 2 would scan more than half of
            // the rows, the exhaustive scan below runs instead and pass 1 is
            // dropped (4096 noise frames: 1.6 us per launch slower than the
            // exhaustive kernel without this, DESIGN.md has the figures with it).
            const char *ws = (const char *)wsc;
            const int lo = (int)(prec & 0xFFu), hi = (int)((prec >> 8) & 0xFFu);
            const char *wsp = ws + (int)ppair * (P1K_KPAD * 8);
            f2 wm = f2{-INFINITY, -INFINITY};
#pragma nounroll
            for (int j0 = 0; j0 < (int)pwid; j0 += 4) {  // (one trip: rows span <= 4 lags in config 2)
                f2 v[4];
#pragma unroll
                for (int j = 0; j < 4; j++)
                    v[j] = lds_f2_plain(wsp, 8 * imin(lo + j0 + j, hi));
#pragma unroll
                for (int j = 0; j < 4; j++)
                    wm = f2{fmaxf(wm.x, v[j].x), fmaxf(wm.y, v[j].y)};
            }
            const f2 t0 = ppair == 0 ? wm : f2{pm[0][0], pm[0][1]};
            const f2 t1 = ppair == 1 ? wm : f2{pm[1][0], pm[1][1]};
            const f2 t2 = ppair == 2 ? wm : f2{pm[2][0], pm[2][1]};
            const f2 bnd = (t0 + t1) + t2;
            const bool rowok = (uint32_t)lane64 < prows;
            const uint64_t allrows = __ballot(rowok);
            uint64_t mask = 0;
#pragma unroll
            for (int f = 0; f < 2; f++) {  // the rows that have the frame's largest bound
                const int k = rowok ? fkey(f ? bnd.y : bnd.x) : INT_MIN;
                mask |= __ballot(k == wave_reduce<true>(k));
            }
            mask &= allrows;
            // row R's words and cells: a uniform base plus the lane
            const uint32_t *ptw = ps + TDOA_P1K_PRUNE_HDR + 64;
            const int32_t *pcl = (const int32_t *)(ptw + 64 * prows);
            float bv[2] = {-INFINITY, -INFINITY};
            int bc[2] = {INT_MAX, INT_MAX}, vk[2] = {fkey(-INFINITY), fkey(-INFINITY)};
            constexpr int RB = 4;
            auto rowscan = [&](const uint32_t(&w)[RB], const int(&c)[RB]) {
                f2 g[RB][3];
#pragma unroll
                for (int i = 0; i < RB; i++) {
                    g[i][0] = lds_f2_plain(ws, (int)(w[i] & 0x3FFu));
                    g[i][1] = lds_f2_plain(ws, P1K_KPAD * 8 + (int)((w[i] >> 10) & 0x3FFu));
                    g[i][2] = lds_f2_plain(ws, 2 * P1K_KPAD * 8 + (int)(w[i] >> 20));
                }
#pragma unroll
                for (int i = 0; i < RB; i++) {
                    const f2 Lg = (g[i][0] + g[i][1]) + g[i][2];
#pragma unroll
                    for (int f = 0; f < 2; f++) {
                        const float l = f ? Lg.y : Lg.x;
                        const bool take = (l > bv[f]) | ((l == bv[f]) & (c[i] < bc[f]));  // (no branches)
                        bv[f] = take ? l : bv[f];
                        bc[f] = take ? c[i] : bc[f];
                    }
                }
            };
            int R = 0;
            // the next RB rows of the mask; once it is empty, the last row again
            // (scanning a row twice changes nothing: no larger L, no smaller cell)
            auto request = [&](uint32_t(&w)[RB], int(&c)[RB]) {
#pragma unroll
                for (int i = 0; i < RB; i++) {
                    if (mask) {
                        R = (int)__builtin_ctzll(mask);
                        mask &= mask - 1;
                    }
                    w[i] = (ptw + 64 * R)[lane64];
                    c[i] = (pcl + 64 * R)[lane64];
                }
                // the loads stay here: without this the compiler sinks a batch's
                // loads below the branch that ends the pass, behind the previous
                // batch's scan, and each batch is an L2 round trip of its own
                asm volatile("" ::: "memory");
            };
            uint64_t done = 0;
            for (int pass = 0; pass < 2 && mask && !full; pass++) {
                done |= mask;
                // two register sets, no copies (a copy would wait for its loads)
                uint32_t wa[RB], wb[RB];
                int ca[RB], cb[RB];
                request(wa, ca);
                for (;;) {
                    const bool more_b = mask != 0;
                    request(wb, cb);
                    rowscan(wa, ca);
                    if (!more_b)
                        break;
                    const bool more_a = mask != 0;
                    request(wa, ca);
                    rowscan(wb, cb);
                    if (!more_a)
                        break;
                }
                // the wave's best so far, and after pass 1 the rows that can
                // still hold a larger L or a tie of either frame
#pragma unroll
                for (int f = 0; f < 2; f++)
                    vk[f] = wave_reduce<true>(fkey(bv[f]));
                if (pass == 0) {
                    mask = __ballot(!(bnd.x < fkey_value(vk[0])) || !(bnd.y < fkey_value(vk[1]))) & allrows & ~done;
                    full = 2 * __builtin_popcountll(mask) > (int)prows;
                }
            }
            if (!full) {
                LEAN_MARK();
                // (max L, smallest first cell) over the wave; no L above -inf
                // (NaN scores): tuple 0, as the exhaustive scan answers
#pragma unroll
                for (int j = 0; j < 2; j++) {
                    const int ci = wave_reduce<false>(fkey(bv[j]) == vk[j] ? bc[j] : INT_MAX);
                    gv[j] = fkey_value(vk[j]);
                    wcell[j] = gv[j] > -INFINITY ? ci : pcell0;
                }
                LEAN_MARK();
            }
        }
#endif
        if (full) {
#if P1K_GROUPS
        // Tuples grouped by their first two lags (tdoa_phat1024_image): a
        // group word holds the LDS offsets of lags l0, l1 and the first of n
        // consecutive l2 (n = 3, 2, 1 by bucket), so a group costs 2 + n score
        // gathers for its n tuples instead of 3 n, and (w0 + w1) is formed once
        // -- the same association as ((w0 + w1) + w2), so the same floats.
        // A lane keeps per frame the largest group maximum and its slot (strict
        // '>', one compare per group instead of per tuple) and flags a tie with
        // its running maximum.  At the end each lane re-reads its best group
        // and takes the smallest first cell among the members equal to the
        // maximum; the wave reduces (L, cell) -- the smallest cell among maxima
        // is the first tuple (tuples are in first-cell order).  A lane whose
        // maximum tied another of its groups rescans everything (rare: flat or
        // equal scores).  Bucket sizes and tuple 0's cell: the image header,
        // read as scalars from the global image.
        const int *ghdr = reinterpret_cast<const int *>(static_cast<const char *>(kp.p1k_img) + P1K_IMG_FIXED);
        const int gn3 = ghdr[0], gn2 = ghdr[1], gn1 = ghdr[2], gcell0 = ghdr[3];
        const uint32_t *gw = tups + 4;
        const uint16_t *gcl = reinterpret_cast<const uint16_t *>(gw + gn3 + gn2 + gn1);
        const int gcb2 = 3 * gn3, gcb1 = gcb2 + 2 * gn2, gend = gn3 + gn2 + gn1;
        // per frame: the largest group maximum, the first slot that reached it
        // (strict '>') and the last slot that matched it ('>='); they differ
        // exactly when a later group tied the maximum
        int gs[2] = {0, 0}, gsl[2] = {0, 0};
        const char *ws = (const char *)wsc;
        constexpr int R1 = P1K_KPAD * 8, R2 = 2 * P1K_KPAD * 8;
        // volatile LDS reads: issued in program order, so the pipeline below is
        // the one the hardware sees (the scheduler otherwise sank each step's
        // word read to just before its gathers, and waited on it there)
        auto gat = [&](auto nm, uint32_t w, f2 &a, f2 &b, f2 (&c)[decltype(nm)::value]) {
            a = lds_rd(reinterpret_cast<const f2 *>(ws + (w & 0x3FFu)));
            b = lds_rd(reinterpret_cast<const f2 *>(ws + R1 + ((w >> 10) & 0x3FFu)));
#pragma unroll
            for (int j = 0; j < decltype(nm)::value; j++)
                c[j] = lds_rd(reinterpret_cast<const f2 *>(ws + R2 + (w >> 20) + 8 * j));
        };
        // one bucket of groups of NM tuples: slots [s0, s1), an even number of
        // 64-slot rows, taken two rows (a unit) at a time.  Software-pipelined
        // over two register sets (no copies, which would wait for the loads):
        // while unit u is compared, unit u+1's 2 (2 + NM) gathers are in flight,
        // and every word is read before the gathers issued ahead of its own, so
        // that waiting for it (LDS returns in order) never waits for those
        auto bucket = [&](auto nm, int s0, int s1) {
            constexpr int NM = decltype(nm)::value;
            if (s0 >= s1)
                return;
            const int last = s1 - 64;  // (clamped units past the end: harmless re-reads)
            const int nu = (s1 - s0) / 128;
            auto words = [&](uint32_t (&w)[2], int u) {
                w[0] = lds_rd_u32(gw + imin(s0 + 128 * u, last) + lane64);
                w[1] = lds_rd_u32(gw + imin(s0 + 128 * u + 64, last) + lane64);
            };
            auto gather = [&](const uint32_t (&w)[2], f2 (&a)[2], f2 (&b)[2], f2 (&c)[2][NM]) {
                gat(nm, w[0], a[0], b[0], c[0]);
                gat(nm, w[1], a[1], b[1], c[1]);
            };
            auto consume = [&](const f2 (&a)[2], const f2 (&b)[2], const f2 (&c)[2][NM], int u) {
#pragma unroll
                for (int r = 0; r < 2; r++) {
                    const f2 part = a[r] + b[r];
                    f2 L[NM];
#pragma unroll
                    for (int j = 0; j < NM; j++)
                        L[j] = part + c[r][j];
                    float m[2] = {L[0].x, L[0].y};
#pragma unroll
                    for (int j = 1; j < NM; j++) {
                        m[0] = fmaxf(m[0], L[j].x);
                        m[1] = fmaxf(m[1], L[j].y);
                    }
                    const int sl = s0 + 128 * u + 64 * r + lane64;
#pragma unroll
                    for (int f = 0; f < 2; f++) {
                        const bool gt = m[f] > gv[f];
                        gsl[f] = m[f] >= gv[f] ? sl : gsl[f];
                        gs[f] = gt ? sl : gs[f];
                        gv[f] = gt ? m[f] : gv[f];
                    }
                }
            };
            f2 a0[2], b0[2], c0[2][NM], a1[2], b1[2], c1[2][NM];
            uint32_t w2[2], w3[2];
            // (the prologue leaves the loads in the loop's own order -- unit 0,
            // then the words of unit 2, then unit 1 -- so the wait counts at the
            // loop head are the steady state's, not a full drain)
            words(w2, 0);
            gather(w2, a0, b0, c0);
            words(w3, 1);
            words(w2, 2);
            gather(w3, a1, b1, c1);
            // whole pairs of units whose loads stay inside the bucket, in a
            // branch-free body (a branch inside made the wait-count pass drain
            // every load at the loop head; scheduling barriers: the scheduler
            // hoisted unit u+1's sums above unit u+2's gathers, the same drain)
            int u = 0;
            for (; u + 3 < nu; u += 2) {
                consume(a0, b0, c0, u);
                words(w3, u + 3);
                gather(w2, a0, b0, c0);
                __builtin_amdgcn_sched_barrier(0);
                consume(a1, b1, c1, u + 1);
                words(w2, u + 4);
                gather(w3, a1, b1, c1);
                __builtin_amdgcn_sched_barrier(0);
            }
            // the last one to three units, none loaded past the end
            consume(a0, b0, c0, u);
            if (u + 2 < nu)
                gather(w2, a0, b0, c0);
            if (u + 1 < nu)
                consume(a1, b1, c1, u + 1);
            if (u + 2 < nu)
                consume(a0, b0, c0, u + 2);
        };
        bucket(std::integral_constant<int, 3>{}, 0, gn3);
        bucket(std::integral_constant<int, 2>{}, gn3, gn3 + gn2);
        bucket(std::integral_constant<int, 1>{}, gn3 + gn2, gend);
        LEAN_MARK();
        // smallest first cell among the members of group slot sl whose L (frame
        // f) equals v; INT_MAX if none (the rare full rescan)
        auto group_cell = [&](int sl, int f, float v) {
            const int nm = sl < gn3 ? 3 : (sl < gn3 + gn2 ? 2 : 1);
            const int cb = sl < gn3 ? 3 * sl : (sl < gn3 + gn2 ? gcb2 + 2 * (sl - gn3) : gcb1 + (sl - gn3 - gn2));
            const uint32_t w = gw[sl];
            const f2 part = lds_f2_plain(ws, (int)(w & 0x3FFu)) + lds_f2_plain(ws, R1 + (int)((w >> 10) & 0x3FFu));
            int mc = INT_MAX;
#pragma unroll
            for (int j = 0; j < 3; j++) {
                if (j < nm) {
                    const f2 Lg = part + lds_f2_plain(ws, R2 + (int)(w >> 20) + 8 * j);
                    if ((f ? Lg.y : Lg.x) == v)
                        mc = imin(mc, (int)gcl[cb + j]);
                }
            }
            return mc;
        };
        // each lane's candidate per frame: its best group's members equal to
        // the maximum, both frames' words and cells read together, then the
        // gathers (two LDS round trips)
        int cand[2];
        {
            uint32_t bw[2];
            int bnm[2], bc[2][3];
#pragma unroll
            for (int f = 0; f < 2; f++) {
                const int sl = gs[f];
                bnm[f] = sl < gn3 ? 3 : (sl < gn3 + gn2 ? 2 : 1);
                const int cb = sl < gn3 ? 3 * sl : (sl < gn3 + gn2 ? gcb2 + 2 * (sl - gn3) : gcb1 + (sl - gn3 - gn2));
                bw[f] = gw[sl];
#pragma unroll
                for (int j = 0; j < 3; j++)
                    bc[f][j] = gcl[cb + imin(j, bnm[f] - 1)];
            }
#pragma unroll
            for (int f = 0; f < 2; f++) {
                const uint32_t w = bw[f];
                const f2 part = lds_f2_plain(ws, (int)(w & 0x3FFu)) + lds_f2_plain(ws, R1 + (int)((w >> 10) & 0x3FFu));
                int mc = INT_MAX;
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    const f2 Lg = part + lds_f2_plain(ws, R2 + (int)(w >> 20) + 8 * j);
                    if (j < bnm[f] && (f ? Lg.y : Lg.x) == gv[f])
                        mc = imin(mc, bc[f][j]);
                }
                cand[f] = gv[f] > -INFINITY ? mc : INT_MAX;
            }
        }
#pragma unroll
        for (int j = 0; j < 2; j++) {
            int ci = cand[j];
            int gk = fkey(gv[j]);
            wave_argmax_key(gk, ci);
            const float V = fkey_value(gk);
            if (__ballot(gsl[j] != gs[j] && gv[j] == V && V > -INFINITY)) {
                // rare: some lane's maximum tied another of its groups -- the
                // smallest first cell of every member whose L equals it
                int mc = INT_MAX;
                for (int sl = lane64; sl < gend; sl += 64)
                    mc = imin(mc, group_cell(sl, j, V));
                ci = wave_reduce<false>(mc);
            }
            wcell[j] = ci == INT_MAX ? gcell0 : ci;  // no maximum (NaN scores): tuple 0
            gv[j] = V;
        }
        LEAN_MARK();
#else
        int gu[2] = {INT_MAX, INT_MAX};
        const char *ws = (const char *)wsc;
        // lane-strided: the 32 lanes of a gather read 32 consecutive tuples
        // (first-cell order: neighbouring cells, so equal or adjacent lag slots
        // -- broadcasts and distinct banks instead of 4-way conflicts).
        // Software-pipelined by one step: the next step's tuple words and 12
        // gathers are in flight while this step's sums and compares run (the
        // loop is bound by LDS latency, not by its few VALU operations).
#if P1K_CELL_LDS
        const uint32_t wsb = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) char *)ws;
#endif
        auto gather = [&](const uint32_t (&qq)[4], f2 (&g)[4][3]) {
#pragma unroll
            for (int i = 0; i < 4; i++) {
#if P1K_CELL_LDS
                // tuple fields: the lag slots' byte offsets (slot << 3) in bits
                // 3-9, 10-16 (>> 7), 17-23 (>> 14); the 1 KiB-aligned base
                // goes in by an or.  The first cell's offset from its row's
                // is in bits 24-31 and 0-2
                g[i][0] = lds_at((qq[i] & 0x3F8u) | wsb);
                g[i][1] = lds_at((((qq[i] >> 7) & 0x3F8u) | wsb) + P1K_KPAD * 8);
                g[i][2] = lds_at((((qq[i] >> 14) & 0x3F8u) | wsb) + 2 * P1K_KPAD * 8);
#else
                // tuple fields are byte offsets of f2 slots in [p][KPAD]
                g[i][0] = lds_f2_plain(ws, (int)(qq[i] & 0x3FFu));
                g[i][1] = lds_f2_plain(ws, P1K_KPAD * 8 + (int)((qq[i] >> 10) & 0x3FFu));
                g[i][2] = lds_f2_plain(ws, 2 * P1K_KPAD * 8 + (int)(qq[i] >> 20));
#endif
            }
        };
        uint32_t q[4];
        f2 g[4][3];
#pragma unroll
        for (int i = 0; i < 4; i++)
            q[i] = tups[64 * i + lane64];
        // NW = 4: the words come from L2, so each step's are requested two
        // steps ahead of its gathers, into the buffer the gathers of two steps
        // before have just read
        [[maybe_unused]] uint32_t qa[4], qb[4];
        [[maybe_unused]] auto words = [&](uint32_t (&qq)[4], int u) {
            const uint32_t *tl = tups + u + lane64;
#pragma unroll
            for (int i = 0; i < 4; i++)
                qq[i] = tl[64 * i];
        };
#if P1K_WG4_TUPS_ALL
        constexpr int TS = 14;  // steps of 256 tuples in the largest image that fits
        [[maybe_unused]] uint32_t qall[TS][4];
        if constexpr (WG4) {
#pragma unroll
            for (int s = 1; s < TS; s++)
                words(qall[s], imin(256 * s, Upad - 256));
        }
#else
        if constexpr (WG4) {
            words(qa, 256);
            words(qb, Upad > 512 ? 512 : 256);
        }
#endif
        gather(q, g);
        auto consume = [&](const f2 (&gg)[4][3], int ub) {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const f2 Lg = (gg[i][0] + gg[i][1]) + gg[i][2];
                const int u = ub + 64 * i + lane64;  // ascending per lane
                if (Lg.x > gv[0]) {
                    gv[0] = Lg.x;
                    gu[0] = u;
                }
                if (Lg.y > gv[1]) {
                    gv[1] = Lg.y;
                    gu[1] = u;
                }
            }
        };
        // two steps per trip (Upad is a multiple of 512): the step buffers
        // alternate instead of being copied back (24 moves a step)
#if P1K_WG4_TUPS_ALL
        if constexpr (WG4) {
#pragma unroll
            for (int s = 0; s < TS; s += 2) {
                if (256 * s >= Upad)
                    break;
                f2 gn[4][3];
                gather(qall[s + 1], gn);
                consume(g, 256 * s);
                gather(qall[s + 2 < TS ? s + 2 : TS - 1], g);
                consume(gn, 256 * (s + 1));
            }
        } else
#else
        if constexpr (WG4) {
            const int ulast = Upad - 256;  // (steps past the end re-read the last: never consumed)
            for (int u0 = 0; u0 < Upad; u0 += 512) {
                f2 gn[4][3];
                gather(qa, gn);  // step u0 + 256
                words(qa, imin(u0 + 768, ulast));
                consume(g, u0);
                gather(qb, g);  // step u0 + 512
                words(qb, imin(u0 + 1024, ulast));
                consume(gn, u0 + 256);
            }
        } else
#endif
        for (int u0 = 0; u0 < Upad; u0 += 512) {
            uint32_t qn[4];
#pragma unroll
            for (int i = 0; i < 4; i++)
                qn[i] = tups[u0 + 256 + 64 * i + lane64];
            f2 gn[4][3];
            gather(qn, gn);
            consume(g, u0);
            const int un = u0 + 512 < Upad ? u0 + 512 : u0 + 256;  // (a harmless re-read)
#pragma unroll
            for (int i = 0; i < 4; i++)
                q[i] = tups[un + 64 * i + lane64];
            gather(q, g);
            consume(gn, u0 + 256);
        }
        LEAN_MARK();
        // each lane looks up the first cell of its own candidate before the
        // wave reduction: the winner's comes back by a lane read, not by a
        // dependent load after it
        int mycell[2], myu[2];
#if P1K_CELL_LDS
        // from LDS: the tuple word's cell offset plus its 32-tuple row's first
        // cell (two LDS reads).  No global load may be pending here: gfx9's
        // vmcnt counts stores too, and every wait for such a load behind the
        // outputs below waited for their HBM write acks (~2.5 k cycles)
        const int *rowcell = reinterpret_cast<const int *>(tups + Upad);
#pragma unroll
        for (int j = 0; j < 2; j++) {
            myu[j] = gu[j];
            const int uc = (gu[j] < 0 || gu[j] >= kp.U) ? 0 : gu[j];
            const uint32_t tw = tups[uc];
            mycell[j] = rowcell[uc >> 5] + (int)((tw >> 24) | ((tw & 7u) << 8));
        }
#else
#pragma unroll
        for (int j = 0; j < 2; j++) {
            myu[j] = gu[j];
            mycell[j] = kp.tuple_cell[(gu[j] < 0 || gu[j] >= kp.U) ? 0 : gu[j]];
        }
#endif
        // (max L, first tuple) over the wave by keys (gv is -inf, never NaN,
        // where a lane had no L above it: those lanes keep gu = INT_MAX)
        int gk[2];
#pragma unroll
        for (int j = 0; j < 2; j++) {
            gk[j] = fkey(gv[j]);
            wave_argmax_key(gk[j], gu[j]);
            gv[j] = fkey_value(gk[j]);
        }
        LEAN_MARK();
#if P1K_CELL_LDS
        const int tuple_cell0 = rowcell[0];  // (offset 0)
#else
        const int tuple_cell0 = kp.tuple_cell[0];
#endif
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int fu = gu[j];
            const uint64_t wm = __ballot(myu[j] == fu && fu >= 0 && fu < kp.U);
            wcell[j] = wm ? __builtin_amdgcn_readlane(mycell[j], __builtin_ctzll(wm)) : tuple_cell0;
        }
#endif
        }
        if (lane64 == 63) {
            const int cells[2] = {wcell[0], wcell[1]};  // no winner (NaN scores): tuple 0
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const int64_t fs = base + 2 * (WG4 ? (fresh_tid() >> 6) & (NW - 1) : wave) + j;
                if (fs < B) {
                    if (out.cell)
                        out.cell[fs] = cells[j];
                    if (out.max_Lf)
                        out.max_Lf[fs] = gv[j];
                    if (out.xy) {
                        const int cx = cells[j] % kp.grid_W, cy = cells[j] / kp.grid_W;
                        out.xy[2 * fs] = (float)(cx - kp.half_w) / kp.grid_scale;
                        out.xy[2 * fs + 1] = (float)(kp.half_h - cy) / kp.grid_scale;
                    }
                }
            }
        }
#if P1K_LATE_STORES
        store_frame();
#endif
        LEAN_MARK();
    }
#ifdef TDOA_DIAG
    stamp[13] = __builtin_amdgcn_s_memtime();
    stamp[15] = __builtin_amdgcn_s_memrealtime();
    if (lane64 == 0 && (blockIdx.x * NW + wave) < 4096)
        for (int i = 0; i < 16; i++)
            g_diag_p1k[(blockIdx.x * NW + wave) * 16 + i] = stamp[i];
#endif
#undef LEAN_MARK
