// sep_host_main.cpp -- the host side of the null-steering beamformer driven as
// a program of its own (no HIP, no Python): tests/test_sep_cpu.py builds it
// under ASan + UBSan (make -C audio-triangulation_amd sep_host_san).  It runs
// the table builders into heap blocks of exactly the size they state, so a
// write past a table is a report, and every argument check on a geometry read
// from a file.
//
//   sep_host_san <in> <out>
// in : tdoa_beam_geometry (80 bytes); int32 n; then n cases of int32 L, Kt and
//      float loading
// out: int32 rc [n] of tdoa_sep_check_of; then for every case with rc = 0 the
//      table of L: window float [L], twiddles float [2 L]
// stdout: sizeof(tdoa_beam_geometry).
#include <cstdio>
#include <vector>

#include "../include/tdoa.h"
#include "tdoa_sep_rule.h"

int main(int argc, char **argv)
{
    printf("sizeof %zu\n", sizeof(tdoa_beam_geometry));
    if (argc != 3)
        return 0;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) {
        fprintf(stderr, "cannot open %s / %s\n", argv[1], argv[2]);
        return 2;
    }
    tdoa_beam_geometry g;
    int32_t n = 0;
    if (fread(&g, sizeof g, 1, in) != 1 || fread(&n, sizeof n, 1, in) != 1 || n < 0 || n > 1024) {
        fprintf(stderr, "short header\n");
        return 2;
    }
    struct item {
        int32_t L, Kt;
        float loading;
    };
    std::vector<item> cases((size_t)n);
    if (n && fread(cases.data(), sizeof(item), cases.size(), in) != cases.size()) {
        fprintf(stderr, "short input\n");
        return 2;
    }
    std::vector<int32_t> rc((size_t)n);
    for (int i = 0; i < n; i++)
        rc[i] = tdoa_sep_check_of(&g, cases[i].L, cases[i].Kt, cases[i].loading);
    if (n && fwrite(rc.data(), sizeof(int32_t), rc.size(), out) != rc.size())
        return 2;
    for (int i = 0; i < n; i++) {
        if (rc[i] != TDOA_OK)
            continue;
        const int L = cases[i].L;
        std::vector<float> win((size_t)L), tab(tdoa_sep_table_floats(L));
        if (tdoa_sep_window(L, win.data()) != TDOA_OK || tdoa_sep_table(L, tab.data()) != TDOA_OK) {
            fprintf(stderr, "table of L = %d: %s\n", L, tdoa_last_error());
            return 3;
        }
        for (int k = 0; k < L; k++)
            if (win[k] != tab[k]) {
                fprintf(stderr, "the table's window differs from tdoa_sep_window at %d\n", k);
                return 3;
            }
        if (fwrite(tab.data(), sizeof(float), tab.size(), out) != tab.size())
            return 2;
    }
    // what the checks refuse must leave the tables alone
    float one = 7.0f;
    if (tdoa_sep_window(100, &one) == TDOA_OK || tdoa_sep_window(256, nullptr) == TDOA_OK ||
        tdoa_sep_table(4096, &one) == TDOA_OK || tdoa_sep_check_of(nullptr, 256, 1, 0.01f) == TDOA_OK || one != 7.0f) {
        fprintf(stderr, "a refused call wrote or returned TDOA_OK\n");
        return 3;
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 2;
}
