// tdoa_tables.cpp -- the one-time tables of a context, built on the host
// before anything touches the GPU (tdoa_tables.h), and the library's other
// host-only entry points (tdoa_dpss_q15, tdoa_band_weights, the error store).
//
// The tables reproduce the reference's float arithmetic exactly; this file is
// compiled with -ffp-contract=off and no fast-math, and the order of the float
// expressions below is what makes the LUT bit-exact:
//   microphones_init      src/components/microphones.c:9-33
//   per-cell lag LUT      src/components/vga/vga_heatmap.h:48-93
//   Gaussian lag prior    src/components/correlations.c:26-33 (exp in libm)
//   DPSS(N, 2) Q15 window window.ipynb cells 2-4 (scipy dpss procedure)
// No HIP header is included: a plain host compiler builds this file too.

#include "tdoa_tables.h"

#include "tdoa_bb_layout.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

namespace {

thread_local std::string g_err;

}  // namespace

int tdoa_set_error(int code, const char *msg)
{
    g_err = msg;
    return code;
}

int tdoa_fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return tdoa_set_error(code, buf);
}

extern "C" const char *tdoa_last_error(void) { return g_err.c_str(); }

namespace {

int ilog2(int n)
{
    int b = 0;
    while ((1 << b) < n)
        b++;
    return b;
}

// ---------------------------------------------------------------- DPSS
// First Slepian taper of length n and time-bandwidth nw: the eigenvector of
// the largest eigenvalue of the symmetric tridiagonal matrix
//   diag_i = ((n-1-2i)/2)^2 cos(2 pi nw/n),  off_i = i(n-i)/2
// (Percival & Walden 1993, the system scipy.signal.windows.dpss solves).
// Largest eigenvalue by Sturm-count bisection, vector by inverse iteration
// with a partially pivoted tridiagonal LU.
int sturm_count_below(const std::vector<double> &d, const std::vector<double> &e2, double x)
{
    int cnt = 0;
    double q = d[0] - x;
    if (q < 0)
        cnt++;
    for (size_t i = 1; i < d.size(); i++) {
        if (q == 0.0)
            q = 1e-300;
        q = d[i] - x - e2[i] / q;
        if (q < 0)
            cnt++;
    }
    return cnt;
}

void tridiag_solve_pivoted(const std::vector<double> &d, const std::vector<double> &e,
                           double lam, std::vector<double> &b)
{
    // Solve (T - lam I) x = b in place; e[i] couples rows i-1 and i (e[0] unused).
    const int n = (int)d.size();
    std::vector<double> a(n), c(n), u2(n, 0.0), l(n, 0.0), dd(n);
    std::vector<int> piv(n, 0);
    // rows: sub a_i = e[i] (i>=1), diag dd_i = d_i - lam, super c_i = e[i+1]
    for (int i = 0; i < n; i++) {
        dd[i] = d[i] - lam;
        a[i] = i > 0 ? e[i] : 0.0;
        c[i] = i + 1 < n ? e[i + 1] : 0.0;
    }
    // Gaussian elimination with partial pivoting (LAPACK dgttrf style)
    for (int i = 0; i < n - 1; i++) {
        if (std::fabs(dd[i]) >= std::fabs(a[i + 1])) {
            double f = dd[i] != 0.0 ? a[i + 1] / dd[i] : 0.0;
            if (dd[i] == 0.0)
                dd[i] = 1e-300;
            l[i] = f;
            dd[i + 1] -= f * c[i];
            b[i + 1] -= f * b[i];
            u2[i] = 0.0;
            piv[i] = 0;
        } else {
            double f = dd[i] / a[i + 1];
            l[i] = f;
            // swap rows i and i+1
            double t_d = a[i + 1], t_c = dd[i + 1], t_u2 = i + 2 < n ? c[i + 1] : 0.0;
            double nd1 = c[i] - f * t_c;
            double nu2 = -f * t_u2;
            dd[i] = t_d;
            c[i] = t_c;
            u2[i] = t_u2;
            dd[i + 1] = nd1;
            if (i + 2 < n)
                c[i + 1] = nu2;
            double tb = b[i];
            b[i] = b[i + 1];
            b[i + 1] = tb - f * b[i];
            piv[i] = 1;
        }
    }
    if (dd[n - 1] == 0.0)
        dd[n - 1] = 1e-300;
    // back substitution
    b[n - 1] /= dd[n - 1];
    if (n > 1)
        b[n - 2] = (b[n - 2] - c[n - 2] * b[n - 1]) / dd[n - 2];
    for (int i = n - 3; i >= 0; i--)
        b[i] = (b[i] - c[i] * b[i + 1] - u2[i] * b[i + 2]) / dd[i];
}

}  // namespace

extern "C" int tdoa_dpss_q15(int32_t n, double nw, int32_t *out)
{
    if (n < 4 || !out || !(nw > 0))
        return tdoa_fail(TDOA_ERR_INVALID, "tdoa_dpss_q15: bad arguments");
    const double W = nw / n, cw = std::cos(2.0 * M_PI * W);
    std::vector<double> d(n), e(n, 0.0), e2(n, 0.0);
    for (int i = 0; i < n; i++) {
        const double t = (n - 1 - 2.0 * i) / 2.0;
        d[i] = t * t * cw;
    }
    for (int i = 1; i < n; i++) {
        e[i] = i * (double)(n - i) / 2.0;
        e2[i] = e[i] * e[i];
    }
    // Gershgorin bounds
    double lo = 1e300, hi = -1e300;
    for (int i = 0; i < n; i++) {
        double r = std::fabs(e[i]) + (i + 1 < n ? std::fabs(e[i + 1]) : 0.0);
        lo = std::min(lo, d[i] - r);
        hi = std::max(hi, d[i] + r);
    }
    // largest eigenvalue: smallest x with count_below(x) == n
    for (int it = 0; it < 200; it++) {
        double mid = 0.5 * (lo + hi);
        if (mid <= lo || mid >= hi)
            break;
        if (sturm_count_below(d, e2, mid) >= n)
            hi = mid;
        else
            lo = mid;
    }
    const double lam = 0.5 * (lo + hi);
    std::vector<double> v(n, 1.0);
    for (int it = 0; it < 4; it++) {
        tridiag_solve_pivoted(d, e, lam, v);
        double nrm = 0;
        for (double x : v)
            nrm += x * x;
        nrm = std::sqrt(nrm);
        for (double &x : v)
            x /= nrm;
    }
    double s = 0, mx = 0;
    for (double x : v)
        s += x;
    if (s < 0)
        for (double &x : v)
            x = -x;
    for (double x : v)
        mx = std::max(mx, std::fabs(x));
    for (int i = 0; i < n; i++)
        out[i] = (int32_t)std::nearbyint(v[i] / mx * 32767.0);
    return TDOA_OK;
}

// Band mask over the bins f_k = k fs / 2N, k = 0..N, of the 2N-point spectrum
// (include/tdoa.h): 1 inside [lo, hi], raised-cosine edges of width taper
// outside, 0 elsewhere; double arithmetic, rounded once to float.
extern "C" int tdoa_band_weights(int32_t N, int32_t fs, double lo_hz, double hi_hz, double taper_hz,
                                 float *w)
{
    if (!w)
        return tdoa_fail(TDOA_ERR_INVALID, "tdoa_band_weights: NULL table");
    if (N < 256 || N > 4096 || (N & (N - 1)))
        return tdoa_fail(TDOA_ERR_INVALID, "tdoa_band_weights: N %d must be a power of two in [256,4096]", (int)N);
    if (fs <= 0 || !(lo_hz >= 0.0) || !(lo_hz < hi_hz) || !(hi_hz <= 0.5 * fs) || !(taper_hz >= 0.0) ||
        !std::isfinite(taper_hz))
        return tdoa_fail(TDOA_ERR_INVALID, "tdoa_band_weights: need 0 <= lo < hi <= fs/2 and a finite taper >= 0");
    std::vector<float> t((size_t)N + 1);
    bool any = false;
    for (int k = 0; k <= N; k++) {
        const double f = (double)k * (double)fs / (2.0 * N);
        double v = 0.0;
        if (f >= lo_hz && f <= hi_hz)
            v = 1.0;
        else if (taper_hz > 0.0 && f > lo_hz - taper_hz && f < lo_hz)
            v = 0.5 * (1.0 - std::cos(M_PI * (f - (lo_hz - taper_hz)) / taper_hz));
        else if (taper_hz > 0.0 && f > hi_hz && f < hi_hz + taper_hz)
            v = 0.5 * (1.0 + std::cos(M_PI * (f - hi_hz) / taper_hz));
        t[k] = (float)v;
        any |= t[k] != 0.0f;
    }
    if (!any)
        return tdoa_fail(TDOA_ERR_INVALID, "tdoa_band_weights: no bin of the band has a non-zero weight");
    std::memcpy(w, t.data(), sizeof(float) * t.size());
    return TDOA_OK;
}

namespace {

// microphones.c:9-33 (constants.h:17-19: AB .132, BC .15, CA .20; MIRROR on)
void reference_triangle(float *xy)
{
    const float dAB = 0.132f, dBC = 0.15f, dCA = 0.20f;
    const float xC = (dAB * dAB + dCA * dCA - dBC * dBC) / (2.0f * dAB);
    const float yC = sqrtf(fmaxf(0.0f, dCA * dCA - xC * xC));
    const float pAx = 0.0f, pAy = 0.0f, pBx = dAB, pBy = 0.0f;
    const float pCx = xC, pCy = yC * -1.0f;
    const float cx = (pAx + pBx + pCx) / 3.0f;
    const float cy = (pAy + pBy + pCy) / 3.0f;
    xy[0] = pAx - cx;
    xy[1] = pAy - cy;
    xy[2] = pBx - cx;
    xy[3] = pBy - cy;
    xy[4] = pCx - cx;
    xy[5] = pCy - cy;
}

inline float hypot3(float x, float y, float z) { return sqrtf(x * x + y * y + z * z); }

// vga_heatmap.h:48-93, generalised to lexicographic pairs of M mics.
void build_lut(tdoa_tables *c)
{
    const int W = c->W, H = c->H, G = c->G;
    const float scale = c->cfg.grid_scale, hgt = c->cfg.height_offset;
    const float sos = c->cfg.speed_of_sound;
    const int fs = c->cfg.sample_rate_hz;
    c->lut.assign((size_t)c->P * G, 0);
    std::vector<float> d(c->M);
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            float xm = (float)(x - c->cfg.grid_half_w) / scale;
            float ym = (float)(c->cfg.grid_half_h - y) / scale;
            float zm = hgt;
            const float k = hgt / hypot3(zm, xm, ym);
            xm *= k;
            ym *= k;
            zm *= k;
            for (int m = 0; m < c->M; m++)
                d[m] = hypot3(zm, xm - c->mic[2 * m], ym - c->mic[2 * m + 1]);
            int p = 0;
            for (int i = 0; i < c->M; i++)
                for (int j = i + 1; j < c->M; j++, p++) {
                    const float dt = (d[j] - d[i]) / sos;
                    int s = (int)roundf(dt * (float)fs);
                    s = std::min(std::max(s, -c->S), c->S);
                    c->lut[(size_t)p * G + (size_t)y * W + x] = (uint8_t)(s + c->S);
                }
        }
    // Distinct lag tuples in order of their first (row-major) cell: the max
    // over cells equals the max over tuples, and the first argmax tuple
    // carries the first argmax cell (tuple first-cells are increasing).
    std::map<std::vector<uint8_t>, int> seen;
    c->tuples.clear();
    c->tuple_cell.clear();
    std::vector<uint8_t> key(c->P);
    for (int cell = 0; cell < G; cell++) {
        for (int p = 0; p < c->P; p++)
            key[p] = c->lut[(size_t)p * G + cell];
        if (seen.emplace(key, (int)c->tuple_cell.size()).second) {
            c->tuple_cell.push_back(cell);
            for (int w = 0; w < c->TW; w++) {
                uint32_t v = 0;
                for (int b = 0; b < 4; b++) {
                    int p = 4 * w + b;
                    if (p < c->P)
                        v |= (uint32_t)key[p] << (8 * b);
                }
                c->tuples.push_back(v);
            }
        }
    }
    c->U = (int)c->tuple_cell.size();
}

// An entry's range [lo, hi] of pair p as k_grid_bb's sparse-table query
// (tdoa_grid_bb.h): the LDS element offset o1 of the level-j window
// max w[lo .. lo + 2^j - 1] (2^j <= n = hi - lo + 1 < 2^(j+1)) from the wave's
// scores, and the distance d = n - 2^j of the second window, as o1 | d << 13;
// ranges wider than 15 are marked wide (o1 = 0x1FFF: the kernel loops)
uint16_t bb_query(int P, int K, int p, int lo, int hi)
{
    const int n = hi - lo + 1;
    if (n > 15)
        return 0x1FFF;  // wide: the table is not used (kp.bb_wide)
    // The query's two windows [lo, lo + 2^lv) and [hi + 1 - 2^lv, hi + 1) lie
    // inside [lo, hi] (2^lv <= n), and k_grid_bb's level build reads lags past
    // K - 1 (unclamped 16-B reads, tdoa_grid_bb.h): those level elements are
    // never queried only while every range stays inside the lag range.  A
    // range that does not is encoded wide (the exhaustive k_grid runs instead).
    if (lo < 0 || hi >= K || n < 1)
        return 0x1FFF;
    const int lv = n >= 8 ? 3 : (n >= 4 ? 2 : (n >= 2 ? 1 : 0));
    const int KS = tdoa_bb::bb_ks(P, K), PKp = tdoa_bb::bb_pk(P, K), RW = tdoa_bb::bb_row(K);
    int o1;
    if (lv == 0)
        o1 = p * KS + lo;  // the scores themselves
    else if (P <= 8)
        o1 = lv * PKp + p * K + lo;  // levels [3][P][K] after the scores
    else
        o1 = PKp + (lv - 1) * 4 * RW + (p & 3) * RW + lo;  // [3][4][RW]: four pairs a group
    if (o1 < 0 || o1 >= 0x1FFF)
        return 0x1FFF;  // the offset does not fit 13 bits: wide (exhaustive k_grid)
    return (uint16_t)(o1 | ((n - (1 << lv)) << 13));
}

// Tables of the exact branch-and-bound grid solve (k_grid_bb, tdoa_grid.hip):
// the distinct tuples regrouped by the TILE x TILE block of grid cells their
// first cell lies in (entries of at most 64 tuples, one per lane), and for
// every entry and pair the range of lag indices its tuples use.  The bound of
// an entry is the sum over pairs of the weighted-score maximum over that range.
// lo / hi: per pair the range over all tuples (the one scan of the tuples' lags).
void build_bb_tiles(tdoa_tables *c, std::vector<int> &all_lo, std::vector<int> &all_hi)
{
    constexpr int TILE = 8, CAP = 64;
    const int P = c->P, TW = c->TW, U = c->U;
    const int tx = (c->W + TILE - 1) / TILE, ty = (c->H + TILE - 1) / TILE;
    std::vector<std::vector<int>> members((size_t)tx * ty);
    for (int u = 0; u < U; u++) {
        const int cell = c->tuple_cell[u];
        const int x = cell % c->W, y = cell / c->W;
        members[(size_t)(y / TILE) * tx + x / TILE].push_back(u);
    }
    std::vector<int32_t> tile;
    std::vector<uint16_t> rng, qry;
    std::vector<uint32_t> tup;
    std::vector<int32_t> uidx;
    all_lo.assign(P, 255);
    all_hi.assign(P, -1);
    for (const auto &m : members)
        for (size_t c0 = 0; c0 < m.size(); c0 += CAP) {
            const size_t n = std::min(m.size() - c0, (size_t)CAP);
            tile.push_back((int32_t)uidx.size());
            tile.push_back((int32_t)n);
            std::vector<int> lo(P, 255), hi(P, 0);
            for (size_t i = 0; i < n; i++) {
                const int u = m[c0 + i];
                uidx.push_back(u);
                for (int w = 0; w < TW; w++)
                    tup.push_back(c->tuples[(size_t)u * TW + w]);
                for (int p = 0; p < P; p++) {
                    const int l = (c->tuples[(size_t)u * TW + p / 4] >> (8 * (p & 3))) & 0xFF;
                    lo[p] = std::min(lo[p], l);
                    hi[p] = std::max(hi[p], l);
                }
            }
            for (int p = 0; p < P; p++) {
                rng.push_back((uint16_t)(lo[p] | (hi[p] << 8)));
                qry.push_back(bb_query(P, c->K, p, lo[p], hi[p]));
                all_lo[p] = std::min(all_lo[p], lo[p]);
                all_hi[p] = std::max(all_hi[p], hi[p]);
            }
        }
    c->bb_NT = (int)tile.size() / 2;
    c->bb_wide = 0;
    for (const uint16_t q : qry)
        c->bb_wide |= (q & 0x1FFF) == 0x1FFF;
    auto put = [&](const void *src, size_t bytes) {
        const size_t at = c->bb_img.size();
        c->bb_img.resize(at + ((bytes + 15) & ~(size_t)15), 0);
        memcpy(c->bb_img.data() + at, src, bytes);
        return at;
    };
    c->bb_img.clear();
    c->bb_at[tdoa_tables::BB_TILE] = put(tile.data(), tile.size() * 4);
    c->bb_at[tdoa_tables::BB_RNG] = put(rng.data(), rng.size() * 2);
    c->bb_at[tdoa_tables::BB_TUPLES] = put(tup.data(), tup.size() * 4);
    c->bb_at[tdoa_tables::BB_UIDX] = put(uidx.data(), uidx.size() * 4);
    c->bb_at[tdoa_tables::BB_Q] = put(qry.data(), qry.size() * 2);
}

// Compact weighted-score layout: per pair the lag range the tuples use
// (vga_heatmap.h:68-93: the LUT clamps lags to it), padded to 4 floats.
void build_compact(tdoa_tables *c, std::vector<int> &lo, const std::vector<int> &hi)
{
    tdoa_kparams &kp = c->kp;
    int off = 0;
    bool ok = c->P <= TDOA_MAX_PAIRS;
    c->wc_chunks.clear();
    // many pairs (P > 8): k_grid_bb's score rows are bb_ks apart and a range
    // starts at a multiple of 4 lags, so every chunk lands 16-B aligned
    const int KS = tdoa_bb::bb_ks(c->P, c->K);
    for (int p = 0; ok && p < c->P; p++) {
        if (c->P > 8 && hi[p] >= lo[p])
            lo[p] &= ~3;
        const int w = hi[p] - lo[p] + 1;
        ok = w > 0 && off < 65536;
        if (!ok)
            break;
        kp.wc_lo[p] = (uint8_t)lo[p];
        kp.wc_w[p] = (uint8_t)w;
        kp.wc_off[p] = (uint16_t)off;
        for (int j = 0; j < w; j += 4)
            c->wc_chunks.push_back((uint32_t)(p * KS + lo[p] + j) | ((uint32_t)std::min(4, w - j) << 16));
        off += (w + 3) & ~3;
    }
    c->wc_ok = ok;
    if (ok) {
        kp.wc_CK = off;
        kp.wc_nch = (int32_t)c->wc_chunks.size();
    }
}

#if TDOA_AB
// The fused k_frame16 grid's queries (tdoa_shared.h, kp.fg_q): an A/B path,
// built only into tdoa/libtdoa_ab.so (every context would pay O(U P) host work
// and a device table for it), then the regrouped tuples (bb order) as compact
// element indices, so a tuple's gathers need no per-pair offsets: [U][32] u16
void build_fused_grid(tdoa_tables *c)
{
    const tdoa_kparams &kp = c->kp;
    const int P = c->P, NT = c->bb_NT;
    const uint16_t *rng = (const uint16_t *)(c->bb_img.data() + c->bb_at[tdoa_tables::BB_RNG]);
    const uint32_t *bt = (const uint32_t *)(c->bb_img.data() + c->bb_at[tdoa_tables::BB_TUPLES]);
    c->fg.assign((size_t)NT * 32, 0);
    c->fg_tup_at = c->fg.size() * 2;
    bool fok = c->wc_ok && kp.wc_CK <= 2048 && NT <= 256 && P <= 32;
    for (int t = 0; fok && t < NT; t++)
        for (int p = 0; p < P; p++) {
            const int lo = rng[(size_t)t * P + p] & 0xFF, hi = rng[(size_t)t * P + p] >> 8;
            const int n = hi - lo + 1;
            if (n < 1 || n > 15 || lo < kp.wc_lo[p] || hi >= kp.wc_lo[p] + kp.wc_w[p]) {
                fok = false;
                break;
            }
            const int lv = n >= 8 ? 3 : (n >= 4 ? 2 : (n >= 2 ? 1 : 0));
            const int e = kp.wc_off[p] + lo - kp.wc_lo[p];
            c->fg[(size_t)t * 32 + p] = (uint16_t)(e | (lv << 11) | ((n - (1 << lv)) << 13));
        }
    c->fg_ok = fok;
    if (!fok)
        return;
    c->fg.resize((size_t)NT * 32 + (size_t)c->U * 32, 0);
    uint16_t *tup = c->fg.data() + (size_t)NT * 32;
    for (int u = 0; u < c->U; u++)
        for (int p = 0; p < P; p++) {
            const int lag = (bt[(size_t)u * c->TW + p / 4] >> (8 * (p & 3))) & 0xFF;
            tup[(size_t)u * 32 + p] = (uint16_t)(kp.wc_off[p] + lag - kp.wc_lo[p]);
        }
}
#endif

// The Q15 window: the caller's, the 1024-point table subsampled, or DPSS(N, 2).
int build_window(const tdoa_config *cfg, tdoa_tables *c)
{
    const int N = c->N;
    c->win.resize(N);
    if (cfg->window_q15) {
        for (int i = 0; i < N; i++) {
            if (cfg->window_q15[i] < 0 || cfg->window_q15[i] > 32767)
                return tdoa_fail(TDOA_ERR_INVALID, "window_q15[%d] outside [0,32767]", i);
            c->win[i] = cfg->window_q15[i];
        }
        return TDOA_OK;
    }
    if (N < 1024 && 1024 % N == 0) {
        // buffer.c:8 indexes WINDOW_FUNCTION[i << (10 - BUFFER_SIZE_BITS)]: a
        // shorter frame subsamples the 1024-point Q15 table
        std::vector<int32_t> w1k(1024);
        const int rc = tdoa_dpss_q15(1024, 2.0, w1k.data());
        for (int i = 0; !rc && i < N; i++)
            c->win[i] = w1k[(size_t)i * (1024 / N)];
        return rc;
    }
    // N > 1024 (where buffer.c:8 is undefined): DPSS(N, NW=2) by the
    // window.ipynb procedure
    return tdoa_dpss_q15(N, 2.0, c->win.data());
}

// GCC_PHAT twiddles, in double then rounded once
void build_twiddles(tdoa_tables *c)
{
    const int N = c->N;
    std::vector<float> &tw = c->tw;
    c->tw2_at = 2 * (size_t)N;
    c->r16_at = 2 * (size_t)N + 2 * ((size_t)N + 1);
    tw.assign(c->r16_at + 2 * 3 * 256, 0.0f);
    for (int k = 0; k < N; k++) {
        const double a = -2.0 * M_PI * k / N;
        tw[2 * k] = (float)std::cos(a);
        tw[2 * k + 1] = (float)std::sin(a);
    }
    for (int k = 0; k <= N; k++) {
        const double a = -2.0 * M_PI * k / (2.0 * N);
        tw[2 * N + 2 * k] = (float)std::cos(a);
        tw[2 * N + 2 * k + 1] = (float)std::sin(a);
    }
    // coalesced twiddle tables of the long-frame kernels (tdoa_phat_r16.hip):
    // [r][k] W_N^{(N/256) r k}; [r][l] W_N^{r l}; [r][h] W_N^{16 r h}  (r, k, l, h < 16)
    float *t = tw.data() + c->r16_at;
    const int R1 = N >= 256 ? N / 256 : 1;
    const int mul[3] = {R1, 1, 16};
    for (int s = 0; s < 3; s++)
        for (int r = 0; r < 16; r++)
            for (int k = 0; k < 16; k++) {
                const long e = ((long)mul[s] * r * k) % N;
                const double a = -2.0 * M_PI * (double)e / N;
                t[2 * (256 * s + 16 * r + k)] = (float)std::cos(a);
                t[2 * (256 * s + 16 * r + k) + 1] = (float)std::sin(a);
            }
}

// every kernel parameter that is no device pointer and no table layout
void build_kparams(tdoa_tables *c)
{
    const int M = c->M, N = c->N, S = c->S;
    tdoa_kparams &kp = c->kp;
    std::memset(&kp, 0, sizeof kp);
    kp.M = M;
    kp.N = N;
    kp.log2N = ilog2(N);
    kp.P = c->P;
    kp.K = c->K;
    kp.S = S;
    kp.G = c->G;
    kp.U = c->U;
    kp.grid_W = c->W;
    kp.half_w = c->cfg.grid_half_w;
    kp.half_h = c->cfg.grid_half_h;
    kp.grid_scale = c->cfg.grid_scale;
    kp.sbase = (S % 2 == 0) ? -S : -S - 1;
    kp.T = (S - kp.sbase + 1 + TDOA_LT - 1) / TDOA_LT;
    kp.NSEG = (N / 2) / TDOA_SEGW;
    // rows are read at word offsets [h, h + SEGW*NSEG + LT2 + 1) with
    // h in [sbase/2, sbase/2 + LT2*(T-1)]
    const int need_left = -kp.sbase / 2;
    const int need_right = kp.sbase / 2 + TDOA_LT2 * (kp.T - 1) + TDOA_LT2 + 2;
    kp.PADW = ((std::max(need_left, need_right) + 3) / 4) * 4;
    kp.RS = N / 2 + 2 * kp.PADW;
    kp.TW = c->TW;
    int p = 0;
    for (int i = 0; i < M; i++)
        for (int j = i + 1; j < M; j++, p++) {
            kp.pair_i[p] = (uint8_t)i;
            kp.pair_j[p] = (uint8_t)j;
        }
    kp.fs = (float)c->cfg.sample_rate_hz;
    kp.c = c->cfg.speed_of_sound;
    kp.height = c->cfg.height_offset;
    kp.bb_NT = c->bb_NT;
    kp.bb_wide = c->bb_wide;
}

}  // namespace

// The pruned grid scan's row table (tdoa_tables.h has the layout): for each
// pair the tuples stably sorted by that pair's lag slot and cut into rows of
// 64; the sort pair is the one whose widest row spans the fewest lags (then
// the smallest sum of widths, then the lowest pair).
void tdoa_p1k_prune_section(int U, const uint32_t *tuples, const int32_t *tuple_cell, std::vector<uint32_t> &sec)
{
    sec.clear();
    const int rows = (U + 63) / 64;
    if (U <= 0 || rows > 64)
        return;
    std::vector<int> order[3];
    int wmax[3], wsum[3], best = 0;
    for (int p = 0; p < 3; p++) {
        order[p].resize(U);
        for (int u = 0; u < U; u++)
            order[p][u] = u;
        std::stable_sort(order[p].begin(), order[p].end(), [&](int a, int b) {
            return ((tuples[a] >> (8 * p)) & 0xFFu) < ((tuples[b] >> (8 * p)) & 0xFFu);
        });
        wmax[p] = wsum[p] = 0;
        for (int r = 0; r < rows; r++) {
            const int lo = (tuples[order[p][64 * r]] >> (8 * p)) & 0xFF;
            const int hi = (tuples[order[p][std::min(U, 64 * r + 64) - 1]] >> (8 * p)) & 0xFF;
            wmax[p] = std::max(wmax[p], hi - lo + 1);
            wsum[p] += hi - lo + 1;
        }
        if (wmax[p] < wmax[best] || (wmax[p] == wmax[best] && wsum[p] < wsum[best]))
            best = p;
    }
    const std::vector<int> &o = order[best];
    sec.resize(TDOA_P1K_PRUNE_HDR + 64 + 2 * (size_t)rows * 64);
    sec[0] = (uint32_t)rows;
    sec[1] = (uint32_t)best;
    sec[2] = (uint32_t)wmax[best];
    sec[3] = (uint32_t)tuple_cell[0];
    uint32_t *rec = sec.data() + TDOA_P1K_PRUNE_HDR, *wd = rec + 64, *cl = wd + (size_t)rows * 64;
    for (int r = 0; r < 64; r++) {
        // (records past the last row: the padding slot 127, whose score is -inf)
        const uint32_t lo = r < rows ? (tuples[o[64 * r]] >> (8 * best)) & 0xFFu : 127u;
        const uint32_t hi = r < rows ? (tuples[o[std::min(U, 64 * r + 64) - 1]] >> (8 * best)) & 0xFFu : 127u;
        rec[r] = lo | (hi << 8);
    }
    for (int e = 0; e < rows * 64; e++) {
        // the word as in the exhaustive scan's table: LDS byte offsets of the f2
        // slots, 10 bits a pair; the padding tuple (127, 127, 127) scores -inf
        const uint32_t t = e < U ? tuples[o[e]] : 0x007F7F7Fu;
        wd[e] = ((t & 0xFFu) << 3) | (((t >> 8) & 0xFFu) << 13) | (((t >> 16) & 0xFFu) << 23);
        cl[e] = e < U ? (uint32_t)tuple_cell[o[e]] : 0x7FFFFFFFu;
    }
}

int tdoa_build_tables(const tdoa_config *cfg, tdoa_tables *c)
{
    const int M = cfg->num_mics, N = cfg->frame_len;
    if (M < 2 || M > TDOA_MAX_MICS)
        return tdoa_fail(TDOA_ERR_INVALID, "num_mics %d outside [2,%d]", M, TDOA_MAX_MICS);
    if (N < 256 || N > 4096 || (N & (N - 1)))
        return tdoa_fail(TDOA_ERR_INVALID, "frame_len %d must be a power of two in [256,4096]", N);
    if (cfg->sample_rate_hz <= 0 || !(cfg->speed_of_sound > 0))
        return tdoa_fail(TDOA_ERR_INVALID, "sample_rate_hz / speed_of_sound must be positive");
    // constants.h:12 -- SAMPLE_RATE_HZ * 32 / 34300 (integer division)
    const int S = cfg->max_shift > 0 ? cfg->max_shift
                                     : (int)((int64_t)cfg->sample_rate_hz * 32 / 34300);
    if (S < 1 || S > 63)
        return tdoa_fail(TDOA_ERR_INVALID, "max_shift %d outside [1,63]", S);
    if (cfg->engine != TDOA_ENGINE_DIRECT && cfg->engine != TDOA_ENGINE_GCC_PHAT)
        return tdoa_fail(TDOA_ERR_INVALID, "unknown engine %d", cfg->engine);
    if (cfg->grid_half_w < 0 || cfg->grid_half_h < 0 || cfg->grid_half_w > 1000 ||
        cfg->grid_half_h > 1000 || !(cfg->grid_scale > 0) || !(cfg->height_offset > 0))
        return tdoa_fail(TDOA_ERR_INVALID, "bad grid geometry");
    if (M != 3 && !cfg->mic_xy)
        return tdoa_fail(TDOA_ERR_INVALID, "mic_xy is required unless num_mics == 3");

    c->cfg = *cfg;
    c->cfg.mic_xy = nullptr;
    c->cfg.window_q15 = nullptr;
    c->cfg.max_shift = S;
    c->M = M;
    c->N = N;
    c->P = M * (M - 1) / 2;
    c->S = S;
    c->K = 2 * S + 1;
    c->W = 2 * cfg->grid_half_w + 1;
    c->H = 2 * cfg->grid_half_h + 1;
    c->G = c->W * c->H;
    c->TW = (c->P + 3) / 4;

    c->mic.resize(2 * M);
    if (cfg->mic_xy)
        std::memcpy(c->mic.data(), cfg->mic_xy, sizeof(float) * 2 * M);
    else
        reference_triangle(c->mic.data());
    if (const int rc = build_window(cfg, c))
        return rc;
    // correlations.c:27-30: scale = (float)exp((double)((float)(-d^2) / 36.f))
    c->prior.resize(c->K);
    for (int d = 0; d < c->K; d++) {
        const float arg = (float)(-(d * d)) / 36.f;
        c->prior[d] = (float)std::exp((double)arg);
    }
    build_lut(c);
    std::vector<int> lo, hi;
    build_bb_tiles(c, lo, hi);
    build_kparams(c);
    build_compact(c, lo, hi);
    build_twiddles(c);
#if TDOA_AB
    build_fused_grid(c);
#endif
    return TDOA_OK;
}

// ---------------------------------------------------------------- beamformer
// The fractional-delay FIR table of include/tdoa.h ("Listening"): 32 phases of
// a 16-tap Kaiser-windowed sinc (beta 8), each normalised to sum 1, in double.
namespace {

// modified Bessel function I0 by its power series: terms ((x/2)^k / k!)^2
double bessel_i0(double x)
{
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 200; k++) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < 1e-18 * sum)
            break;
    }
    return sum;
}

}  // namespace

extern "C" int tdoa_beam_fir(float *h)
{
    if (!h)
        return tdoa_fail(TDOA_ERR_INVALID, "tdoa_beam_fir: NULL");
    const double pi = 3.14159265358979323846, beta = (double)TDOA_BEAM_HALF, i0b = bessel_i0(beta);
    for (int q = 0; q < TDOA_BEAM_PHASES; q++) {
        double w[2 * TDOA_BEAM_HALF], sum = 0.0;
        for (int i = 0; i < 2 * TDOA_BEAM_HALF; i++) {
            const int k = i - (TDOA_BEAM_HALF - 1);
            const double x = (double)k - (double)q / TDOA_BEAM_PHASES, r = x / TDOA_BEAM_HALF;
            // (at phase 0 x is an integer: the sinc is the unit tap itself, no sin(pi k) residue)
            const double sinc = q == 0 ? (k == 0 ? 1.0 : 0.0) : std::sin(pi * x) / (pi * x);
            w[i] = r * r <= 1.0 ? sinc * bessel_i0(beta * std::sqrt(1.0 - r * r)) / i0b : 0.0;
            sum += w[i];
        }
        for (int i = 0; i < 2 * TDOA_BEAM_HALF; i++)
            h[q * 2 * TDOA_BEAM_HALF + i] = (float)(w[i] / sum);
    }
    return TDOA_OK;
}

extern "C" int tdoa_beam_geometry_of(const tdoa_config *cfg, tdoa_beam_geometry *g)
{
    if (!cfg || !g)
        return tdoa_fail(TDOA_ERR_INVALID, "tdoa_beam_geometry_of: NULL argument");
    const int M = cfg->num_mics;
    if (M < 2 || M > TDOA_MAX_MICS)
        return tdoa_fail(TDOA_ERR_INVALID, "num_mics %d outside [2,%d]", M, TDOA_MAX_MICS);
    if (cfg->sample_rate_hz <= 0 || !(cfg->speed_of_sound > 0))
        return tdoa_fail(TDOA_ERR_INVALID, "sample_rate_hz / speed_of_sound must be positive");
    if (!(cfg->height_offset > 0))
        return tdoa_fail(TDOA_ERR_INVALID, "bad grid geometry");
    if (M != 3 && !cfg->mic_xy)
        return tdoa_fail(TDOA_ERR_INVALID, "mic_xy is required unless num_mics == 3");
    std::memset(g, 0, sizeof *g);
    g->num_mics = M;
    g->sample_rate_hz = cfg->sample_rate_hz;
    g->speed_of_sound = cfg->speed_of_sound;
    g->height_offset = cfg->height_offset;
    if (cfg->mic_xy)
        std::memcpy(&g->mic_xy[0][0], cfg->mic_xy, sizeof(float) * 2 * M);
    else
        reference_triangle(&g->mic_xy[0][0]);
    return TDOA_OK;
}
