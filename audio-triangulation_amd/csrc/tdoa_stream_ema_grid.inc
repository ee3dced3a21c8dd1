// tdoa_stream_ema_grid.inc -- what a GCC_PHAT hop does with one listed slot once
// its frame's scores exist, as text inside the including kernel's slot loop:
// k_stream_phat and k_stream_phat_pcm16 (through tdoa_stream_phat_hop.inc; the
// scores and lags are in LDS) and k_stream_ema_grid (SCRATCH: k_f16_ring left
// them in global memory).  The slot's record, the float EMA with ema_step,
// `last`, the EMA rows' first maxima, the grid scan over the distinct lag
// tuples (both TW forms), max_Lf, cell, xy and the workgroup's gated count.
// It reads slot, s, end, the kernel's parameters (sp, kp, out, est_all,
// max_Lf), tid / lane / wave / nwaves, P, K, S, the LDS arrays E [P][K], redv,
// redi, the counter ngated and the constant SCRATCH of the including scope, and
//   SCRATCH false: Wf (LDS [P][K], the frame's weighted scores), lag_s (LDS [P])
//   SCRATCH true:  Wf (global, the slot's [P][K] block), lags_in [S][P] and
//                  gate_in [S] (global, by slot)
        // ---- gate and the slot's record
        bool gated;
        if constexpr (SCRATCH) {
            gated = gate_in[slot] != 0;  // sample_compute.h:124-134, taken by k_f16_ring
            if (out.lags && out.lags != lags_in) {
                for (int p = tid; p < P; p += TPB)
                    out.lags[(size_t)slot * P + p] = lags_in[(size_t)slot * P + p];
            }
        } else {
            int g2 = 0;
            for (int p = 0; p < P; p++)
                g2 += lag_s[p] * lag_s[p];
            gated = g2 > 4;  // sample_compute.h:124-134
            if (out.lags) {
                for (int p = tid; p < P; p += TPB)
                    out.lags[(size_t)slot * P + p] = lag_s[p];
            }
        }
        if (tid == 0) {
            if (out.stream_id)
                out.stream_id[slot] = s;
            if (out.end)
                out.end[slot] = end;
            if (out.gate)
                out.gate[slot] = gated ? 1 : 0;
        }
        if (!gated) {  // sample_compute.h:134: only gated frames update
            if (tid == 0 && out.cell)
                out.cell[slot] = -1;
            continue;
        }
        ngated++;

        // ---- float EMA on the stream's scores, the rows' first maxima
        const uint64_t now = (uint64_t)end * 1000000u / (uint64_t)sp.fs;
        const float dec = tdoa_decay_dev(now, sp.last[s]);
        float *est = est_all + (size_t)s * P * K;
        for (int i = tid; i < P * K; i += TPB) {
            const float nv = ema_step(est[i], Wf[i], dec);
            est[i] = nv;
            E[i] = nv;
        }
        __syncthreads();
        if (tid == 0)
            sp.last[s] = now;
        if (out.ema_best) {
            for (int p = wave; p < P; p += nwaves) {
                const int k1 = lane, k2 = lane + 64;
                const float v1 = k1 < K ? E[p * K + k1] : -INFINITY, v2 = k2 < K ? E[p * K + k2] : -INFINITY;
                const int bk = wave_first_max(v1, v2, lane, K);
                if (lane == 0)
                    out.ema_best[(size_t)slot * P + p] = bk - S;
            }
        }

        // ---- grid solve on the EMA scores over the distinct lag tuples
        float bv = -INFINITY;
        int bu = INT_MAX;
        if (kp.TW == 1) {
            // 3-4 mic grids: a thread's tuple words are loaded 8 at a time ahead of
            // their gathers (one L2 round trip per 8 tuples, not per tuple)
            for (int u0 = tid; u0 < kp.U; u0 += 8 * TPB) {
                uint32_t wd[8];
#pragma unroll
                for (int t = 0; t < 8; t++) {
                    const int u = u0 + t * TPB;
                    wd[t] = u < kp.U ? kp.tuples[u] : 0u;
                }
#pragma unroll
                for (int t = 0; t < 8; t++) {
                    const int u = u0 + t * TPB;
                    if (u < kp.U) {
                        float Lv = 0.0f;
                        for (int p = 0; p < P; p++)
                            Lv += E[p * K + ((wd[t] >> (8 * p)) & 0xFFu)];
                        if (Lv > bv) {  // ascending u per thread: strict '>' keeps the first
                            bv = Lv;
                            bu = u;
                        }
                    }
                }
            }
        } else {
            for (int u = tid; u < kp.U; u += TPB) {
                float Lv = 0.0f;
                for (int tw = 0; tw < kp.TW; tw++) {
                    const uint32_t word = kp.tuples[u * kp.TW + tw];
                    for (int b = 0; b < 4; b++) {
                        const int p = 4 * tw + b;
                        if (p < P)
                            Lv += E[p * K + ((word >> (8 * b)) & 0xFFu)];
                    }
                }
                if (Lv > bv) {
                    bv = Lv;
                    bu = u;
                }
            }
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const float ov = __shfl_xor(bv, o, 64);
            const int ou = __shfl_xor(bu, o, 64);
            if (ov > bv || (ov == bv && ou < bu)) {
                bv = ov;
                bu = ou;
            }
        }
        if (lane == 0) {
            redv[wave] = bv;
            redi[wave] = bu;
        }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < nwaves; w++)
                if (redv[w] > bv || (redv[w] == bv && redi[w] < bu)) {
                    bv = redv[w];
                    bu = redi[w];
                }
            if (bu < 0 || bu >= kp.U)  // NaN scores: keep the index in range
                bu = 0;
            const int cell = kp.tuple_cell[bu];
            if (out.cell)
                out.cell[slot] = cell;
            if (max_Lf)
                max_Lf[slot] = bv;
            if (out.xy) {
                const int cx = cell % kp.grid_W, cy = cell / kp.grid_W;
                out.xy[2 * slot] = (float)(cx - kp.half_w) / kp.grid_scale;
                out.xy[2 * slot + 1] = (float)(kp.half_h - cy) / kp.grid_scale;
            }
        }
