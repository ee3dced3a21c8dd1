// tables_dump -- build the host tables of one config (tdoa_build_tables,
// csrc/tdoa_tables.cpp) and write them out; links that one TU, no HIP runtime.
//
//   tables_dump CONFIG OUTDIR
//
// CONFIG: text, one "key value..." per line; floats as their IEEE-754 bit
// pattern in hex so a config is exact: num_mics, frame_len, sample_rate_hz,
// max_shift, engine, grid_half_w, grid_half_h (integers); speed_of_sound,
// grid_scale, height_offset, phat_eps (one float); mic_xy (2 M floats) and
// window_q15 (N integers) optional.
// OUTDIR gets one raw file per table (win, prior, mic, lut, tuples, tuple_cell,
// tw, bb_img, wc_lo, wc_w, wc_off, wc_chunks, fg, p1k_prune); stdout one JSON object of
// the scalars.  Exit 0, or 1 with {"error": code, "message": ...} on stdout
// when the config is rejected (2: the tool's own usage / IO errors).
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "tdoa_tables.h"

namespace {

float bits_float(uint32_t u)
{
    float f;
    memcpy(&f, &u, 4);
    return f;
}
uint32_t float_bits(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

bool read_config(const char *path, tdoa_config *cfg, std::vector<float> *mic, std::vector<int32_t> *win)
{
    std::ifstream in(path);
    if (!in)
        return false;
    memset(cfg, 0, sizeof *cfg);
    std::string line, key;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        if (!(ls >> key))
            continue;
        std::string v;
        std::vector<std::string> vals;
        while (ls >> v)
            vals.push_back(v);
        auto i32 = [&](size_t i) { return (int32_t)strtol(vals.at(i).c_str(), nullptr, 0); };
        auto f32 = [&](size_t i) { return bits_float((uint32_t)strtoul(vals.at(i).c_str(), nullptr, 16)); };
        if (vals.empty())
            return false;
        if (key == "num_mics")
            cfg->num_mics = i32(0);
        else if (key == "frame_len")
            cfg->frame_len = i32(0);
        else if (key == "sample_rate_hz")
            cfg->sample_rate_hz = i32(0);
        else if (key == "max_shift")
            cfg->max_shift = i32(0);
        else if (key == "engine")
            cfg->engine = i32(0);
        else if (key == "grid_half_w")
            cfg->grid_half_w = i32(0);
        else if (key == "grid_half_h")
            cfg->grid_half_h = i32(0);
        else if (key == "speed_of_sound")
            cfg->speed_of_sound = f32(0);
        else if (key == "grid_scale")
            cfg->grid_scale = f32(0);
        else if (key == "height_offset")
            cfg->height_offset = f32(0);
        else if (key == "phat_eps")
            cfg->phat_eps = f32(0);
        else if (key == "mic_xy")
            for (size_t i = 0; i < vals.size(); i++)
                mic->push_back(f32(i));
        else if (key == "window_q15")
            for (size_t i = 0; i < vals.size(); i++)
                win->push_back(i32(i));
        else
            return false;
    }
    // the library reads 2 M floats / N integers: hand it no shorter array
    if (!mic->empty()) {
        if (cfg->num_mics > 0 && mic->size() < 2 * (size_t)cfg->num_mics)
            return false;
        cfg->mic_xy = mic->data();
    }
    if (!win->empty()) {
        if (cfg->frame_len > 0 && win->size() < (size_t)cfg->frame_len)
            return false;
        cfg->window_q15 = win->data();
    }
    return true;
}

bool put_file(const std::string &dir, const char *name, const void *p, size_t bytes)
{
    FILE *f = fopen((dir + "/" + name + ".bin").c_str(), "wb");
    if (!f)
        return false;
    const bool ok = bytes == 0 || fwrite(p, 1, bytes, f) == bytes;
    return fclose(f) == 0 && ok;
}

template <typename T> bool put_vec(const std::string &dir, const char *name, const std::vector<T> &v)
{
    return put_file(dir, name, v.data(), v.size() * sizeof(T));
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 3) {
        fprintf(stderr, "usage: tables_dump CONFIG OUTDIR\n");
        return 2;
    }
    tdoa_config cfg;
    std::vector<float> mic;
    std::vector<int32_t> win;
    if (!read_config(argv[1], &cfg, &mic, &win)) {
        fprintf(stderr, "tables_dump: cannot read config %s\n", argv[1]);
        return 2;
    }
    tdoa_tables t;
    const int rc = tdoa_build_tables(&cfg, &t);
    if (rc) {
        printf("{\"error\": %d, \"message\": \"%s\"}\n", rc, tdoa_last_error());
        return 1;
    }
    const std::string dir = argv[2];
    const tdoa_kparams &kp = t.kp;
    const int P = t.P;
    bool ok = put_vec(dir, "win", t.win) && put_vec(dir, "prior", t.prior) && put_vec(dir, "mic", t.mic) &&
              put_vec(dir, "lut", t.lut) && put_vec(dir, "tuples", t.tuples) &&
              put_vec(dir, "tuple_cell", t.tuple_cell) && put_vec(dir, "tw", t.tw) &&
              put_vec(dir, "bb_img", t.bb_img) && put_vec(dir, "wc_chunks", t.wc_chunks) &&
              put_file(dir, "wc_lo", kp.wc_lo, P) && put_file(dir, "wc_w", kp.wc_w, P) &&
              put_file(dir, "wc_off", kp.wc_off, 2 * (size_t)P) && put_file(dir, "pair_i", kp.pair_i, P) &&
              put_file(dir, "pair_j", kp.pair_j, P);
#if TDOA_AB
    ok = ok && put_vec(dir, "fg", t.fg_ok ? t.fg : std::vector<uint16_t>());
    const int fg_ok = t.fg_ok;
    const size_t fg_tup_at = t.fg_ok ? t.fg_tup_at : 0;
#else
    const int fg_ok = 0;
    const size_t fg_tup_at = 0;
#endif
    // k_p1k_lean's pruned-scan row table (three pairs in one tuple word; else empty)
    std::vector<uint32_t> prune;
    if (t.P == 3 && t.TW == 1)
        tdoa_p1k_prune_section(t.U, t.tuples.data(), t.tuple_cell.data(), prune);
    ok = ok && put_vec(dir, "p1k_prune", prune);
    if (!ok) {
        fprintf(stderr, "tables_dump: cannot write under %s\n", argv[2]);
        return 2;
    }
    printf("{\"M\": %d, \"N\": %d, \"P\": %d, \"K\": %d, \"S\": %d, \"G\": %d, \"W\": %d, \"H\": %d, \"U\": %d, "
           "\"TW\": %d, \"NT\": %d, \"wide\": %d, \"bb_at\": [%zu, %zu, %zu, %zu, %zu], \"tw2_at\": %zu, "
           "\"r16_at\": %zu, \"wc_ok\": %d, \"wc_CK\": %d, \"wc_nch\": %d, \"fg_ok\": %d, \"fg_tup_at\": %zu, ",
           t.M, t.N, t.P, t.K, t.S, t.G, t.W, t.H, t.U, t.TW, t.bb_NT, t.bb_wide, t.bb_at[0], t.bb_at[1],
           t.bb_at[2], t.bb_at[3], t.bb_at[4], t.tw2_at, t.r16_at, (int)t.wc_ok, kp.wc_CK, kp.wc_nch, fg_ok,
           fg_tup_at);
    printf("\"kp\": {\"M\": %d, \"N\": %d, \"log2N\": %d, \"P\": %d, \"K\": %d, \"S\": %d, \"G\": %d, \"U\": %d, "
           "\"grid_W\": %d, \"half_w\": %d, \"half_h\": %d, \"grid_scale\": \"%08" PRIx32 "\", \"sbase\": %d, "
           "\"T\": %d, \"NSEG\": %d, \"PADW\": %d, \"RS\": %d, \"F\": %d, \"TW\": %d, \"xc3\": %d, \"bb_NT\": %d, "
           "\"bb_wide\": %d, \"fs\": \"%08" PRIx32 "\", \"c\": \"%08" PRIx32
           "\", \"height\": \"%08" PRIx32 "\", \"bin_lo\": %d, \"bin_hi\": %d}}\n",
           kp.M, kp.N, kp.log2N, kp.P, kp.K, kp.S, kp.G, kp.U, kp.grid_W, kp.half_w, kp.half_h,
           float_bits(kp.grid_scale), kp.sbase, kp.T, kp.NSEG, kp.PADW, kp.RS, kp.F, kp.TW, kp.xc3, kp.bb_NT,
           kp.bb_wide, float_bits(kp.fs), float_bits(kp.c), float_bits(kp.height), kp.bin_lo,
           kp.bin_hi);
    return 0;
}
