// tdoa_peaks_frame.inc -- one frame's peaks, the body of k_peaks and of
// k_stream_peaks (tdoa_peaks.hip), as text: it reads kp, out, Kp, radius,
// min_rel, smem and the type T of the including kernel, and of the including
// scope
//   f                the frame's row in the outputs (int64_t),
//   PEAKS_FRAME_SRC  its [P][K] score block (an expression, may use PK),
//   lut              the u8 [P][G] LUT, in global memory or in LDS.
// Every thread of the workgroup runs it.  On entry no thread still reads W,
// Lmap or sup of an earlier frame: the last barrier of a frame's rounds
// follows its last scan.
    const int P = kp.P, K = kp.K, G = kp.G, GW = kp.grid_W, GH = G / GW, PK = P * K;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nth = blockDim.x;
    const int nwaves = nth >> 6, NS = (G + 31) >> 5;
    T *W = (T *)smem;
    T *Lmap = W + PK;
    T *redv = Lmap + G;
    int *redi = (int *)(redv + nwaves);
    uint32_t *sup = (uint32_t *)(redi + nwaves);

    const T *src = PEAKS_FRAME_SRC;
    for (int e = tid; e < PK; e += nth)
        W[e] = src[e];
    for (int e = tid; e < NS; e += nth)
        sup[e] = 0u;
    __syncthreads();
    // the L map: LUT bytes (from global memory: coalesced over c), scores gathered
    // from LDS; one add per pair in ascending p, no reassociation
    for (int c = tid; c < G; c += nth) {
        T L = 0;
        for (int p = 0; p < P; p++) {
            int k = lut[(size_t)p * G + c];
            k = k < K ? k : K - 1;  // the context's LUT never exceeds it
            L += W[p * K + k];
        }
        Lmap[c] = L;
    }
    __syncthreads();

    int count = 0;
    int my_cell = -1;         // thread k keeps peak k
    T my_val = lowest_t<T>();
    T v0 = lowest_t<T>();
    for (int k = 0; k < Kp; k++) {
        T bv = lowest_t<T>();
        int bu = INT_MAX;
        // increasing c per thread: strict '>' keeps the first; the first
        // unsuppressed cell is taken whatever its value.  PEAKS_SCAN cells'
        // reads (clamped, so unconditional) are issued before the first compare:
        // one cell at a time waited for the bit, then for the value.
        for (int c0 = tid; c0 < G; c0 += PEAKS_SCAN * nth) {
            T v[PEAKS_SCAN];
            uint32_t s[PEAKS_SCAN];
#pragma unroll
            for (int i = 0; i < PEAKS_SCAN; i++) {
                const int c = c0 + i * nth, cc = c < G ? c : G - 1;
                v[i] = Lmap[cc];
                s[i] = sup[cc >> 5];
            }
#pragma unroll
            for (int i = 0; i < PEAKS_SCAN; i++) {
                const int c = c0 + i * nth;
                const bool here = c < G && !((s[i] >> (c & 31)) & 1u);
                if (here && (v[i] > bv || bu == INT_MAX)) {
                    bv = v[i];
                    bu = c;
                }
            }
        }
        for (int m = 32; m >= 1; m >>= 1)
            better_t(bv, bu, __shfl_xor(bv, m, 64), __shfl_xor(bu, m, 64));
        if (lane == 0) {
            redv[wave] = bv;
            redi[wave] = bu;
        }
        __syncthreads();
        bv = redv[0];
        bu = redi[0];
        for (int w = 1; w < nwaves; w++)
            better_t(bv, bu, redv[w], redi[w]);
        // every thread holds the same (bv, bu): the decisions below are uniform
        if (bu < 0 || bu >= G)  // no cell remains
            break;
        if (k == 0)
            v0 = bv;
        else if (min_rel > 0.0f && !((double)bv >= (double)min_rel * (double)v0))
            break;
        if (tid == k) {
            my_cell = bu;
            my_val = bv;
        }
        count = k + 1;
        if (k + 1 == Kp)
            break;
        // suppress the peak's square, clipped to the grid
        const int px = bu % GW, py = bu / GW;
        const int x0 = px - radius > 0 ? px - radius : 0;
        const int x1 = px + radius < GW - 1 ? px + radius : GW - 1;
        const int y0 = py - radius > 0 ? py - radius : 0;
        const int y1 = py + radius < GH - 1 ? py + radius : GH - 1;
        const int sw = x1 - x0 + 1, n = sw * (y1 - y0 + 1);
        for (int e = tid; e < n; e += nth) {
            const int dy = e / sw, dx = e - dy * sw;
            const int c = (y0 + dy) * GW + x0 + dx;
            atomicOr(&sup[c >> 5], 1u << (c & 31));
        }
        __syncthreads();  // the bits are set, and redv / redi are free again
    }

    // one thread per slot writes the peak, or the empty slot's fills
    if (tid < Kp) {
        const int64_t i = f * Kp + tid;
        const bool have = tid < count;
        const int cell = have ? my_cell : -1;
        out.cell[i] = cell;
        store_L<T>(out, i, have ? my_val : lowest_t<T>());
        if (out.xy) {
            const int cx = have ? cell % GW : 0, cy = have ? cell / GW : 0;
            out.xy[2 * i] = have ? (float)(cx - kp.half_w) / kp.grid_scale : NAN;
            out.xy[2 * i + 1] = have ? (float)(kp.half_h - cy) / kp.grid_scale : NAN;
        }
        if (out.lags)
            for (int p = 0; p < P; p++)
                out.lags[i * P + p] = have ? (int)lut[(size_t)p * G + cell] - kp.S : 0;
    }
    if (tid == 0 && out.count)
        out.count[f] = count;
