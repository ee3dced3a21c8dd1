// tdoa_sep_rule.h -- what the null-steering beamformer's entry points, its host
// side (tdoa_sep_host.cpp) and its kernel (tdoa_sep.hip, k_sep) share
// (include/tdoa.h, "Separating").  The steering is tdoa_beam_rule.h's.  No HIP
// header: a plain host compiler reads it.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "tdoa_beam_rule.h"

// floats of the device table of a block length L: the window g [L], then the
// FFT twiddles W_L^k = (cos, -sin)(2 pi k / L), k < L, interleaved [2 L]
inline size_t tdoa_sep_table_floats(int L) { return (size_t)3 * L; }
// ... built on the host in double (tdoa_sep_host.cpp); L as tdoa_sep_window takes it
int tdoa_sep_table(int L, float *tab);

// complex FFT buffers of L points a workgroup holds: the mic pairs, reused in
// place by the target pairs
inline int tdoa_sep_bufs(int M, int Kt) { return ((M > Kt ? M : Kt) + 1) / 2; }
inline size_t tdoa_sep_lds(int M, int L, int Kt) { return (size_t)tdoa_sep_bufs(M, Kt) * L * 2 * sizeof(float); }

// the argument checks of tdoa_sep_batch / tdoa_stream_sep (host only)
int tdoa_sep_check(const char *fn, int Dmax, int L, int32_t Kt, float loading, const void *out, const void *audio);

// the launcher of k_sep (tdoa_sep.hip): one workgroup per row, blocks of L
// samples.  A ring launch overlap-adds into tail [rows][4][L/2] and writes
// audio [rows][Kt][L/2]; a block launch reads int16 [rows][M][L] and writes
// audio [rows][Kt][L].  Source and targets as tdoa_launch_beam takes them
// (tdoa_beam_rule.h).  tab: the device copy of tdoa_sep_table(L).
int tdoa_launch_sep(const tdoa_beam_geometry &g, int Dmax, const tdoa_beam_source &source, int L,
                    const tdoa_beam_targets &targets, float loading, const float *tab, float *tail,
                    const tdoa_beam_outputs &out, void *stream);
