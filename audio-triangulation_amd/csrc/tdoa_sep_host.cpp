// tdoa_sep_host.cpp -- the host side of the null-steering beamformer
// (include/tdoa.h, "Separating"): the sqrt-Hann window and the twiddle table in
// double arithmetic, and the argument checks its entry points share.  No HIP
// call: a plain host compiler builds this file (with tdoa_beam_host.cpp for the
// geometry's Dmax and tdoa_tables.cpp for the error store).
#include <cmath>

#include "../../include/tdoa.h"
#include "tdoa_sep_rule.h"
#include "tdoa_shared.h"

namespace {

bool block_length(int L) { return L >= 128 && L <= 2048 && (L & (L - 1)) == 0; }

constexpr double PI = 3.14159265358979323846;

}  // namespace

extern "C" int tdoa_sep_window(int32_t L, float *g)
{
    if (!g)
        return tdoa_fail(TDOA_ERR_INVALID, "tdoa_sep_window: NULL");
    if (!block_length(L))
        return tdoa_fail(TDOA_ERR_INVALID, "tdoa_sep_window: L %d is no power of two in 128..2048", (int)L);
    for (int n = 0; n < L; n++)
        g[n] = (float)std::sqrt(0.5 - 0.5 * std::cos(2.0 * PI * (double)n / (double)L));
    return TDOA_OK;
}

int tdoa_sep_table(int L, float *tab)
{
    if (const int rc = tdoa_sep_window(L, tab))
        return rc;
    float *tw = tab + L;
    for (int k = 0; k < L; k++) {
        const double a = 2.0 * PI * (double)k / (double)L;
        tw[2 * k] = (float)std::cos(a);
        tw[2 * k + 1] = (float)-std::sin(a);
    }
    return TDOA_OK;
}

int tdoa_sep_check(const char *fn, int Dmax, int L, int32_t Kt, float loading, const void *out, const void *audio)
{
    if (const int rc = tdoa_beam_check_outputs(fn, Kt, TDOA_SEP_MAX_TARGETS, out, audio))
        return rc;
    // (the negated comparison is also true for a NaN)
    if (!(loading >= TDOA_SEP_LOADING_MIN && loading <= TDOA_SEP_LOADING_MAX))
        return tdoa_fail(TDOA_ERR_INVALID, "%s: loading %g outside [%g, %g]", fn, (double)loading,
                         (double)TDOA_SEP_LOADING_MIN, (double)TDOA_SEP_LOADING_MAX);
    if (!block_length(L))
        return tdoa_fail(TDOA_ERR_INVALID, "%s: block length L %d is no power of two in 128..2048", fn, L);
    if ((int64_t)L < 8 * (int64_t)Dmax)
        return tdoa_fail(TDOA_ERR_INVALID, "%s: block length L %d < 8 Dmax = %lld: the delays act circularly within "
                                           "a block", fn, L, (long long)(8 * (int64_t)Dmax));
    return TDOA_OK;
}

extern "C" int tdoa_sep_check_of(const tdoa_beam_geometry *g, int32_t L, int32_t Kt, float loading)
{
    if (!g)
        return tdoa_fail(TDOA_ERR_INVALID, "tdoa_sep_check_of: NULL geometry");
    int Dmax = 0;
    if (const int rc = tdoa_beam_dmax(*g, &Dmax))
        return rc;
    return tdoa_sep_check("tdoa_sep_check_of", Dmax, L, Kt, loading, g, g);
}
