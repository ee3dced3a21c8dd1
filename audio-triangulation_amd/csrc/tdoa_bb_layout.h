// tdoa_bb_layout.h -- where k_grid_bb (tdoa_grid_bb.h) keeps one frame's
// weighted scores and their sparse-table levels in LDS.  One definition for
// the kernels and for the host tables that address that layout (bb_query and
// the compact chunks of tdoa_tables.cpp); a non-HIP compile sees plain constexpr.
#pragma once

#if defined(__HIP__) || defined(__HIPCC__)
#define TDOA_HD __host__ __device__
#else
#define TDOA_HD
#endif

namespace tdoa_bb {

// row stride of the grouped levels (P > 8): 8 lags per lane, 12 or 16 lanes
TDOA_HD constexpr int bb_row(int K) { return K <= 96 ? 96 : 128; }
// row stride of the frame's scores in LDS: K, or K rounded up to 16 B for many
// pairs (P > 8), whose level build then reads a lane's 16 scores as four
// aligned 16-B reads and whose compact chunks expand by one 16-B store each
TDOA_HD constexpr int bb_ks(int P, int K) { return P > 8 ? (K + 3) & ~3 : K; }
// the frame's scores per wave, padded to 16 B: the levels follow them
TDOA_HD constexpr int bb_pk(int P, int K) { return (P * bb_ks(P, K) + 3) & ~3; }

}  // namespace tdoa_bb
