// vsc_table.h - the table-driven off-target score (CFD form; DESIGN 4.20, include/varscot_hip.h "TABLE / SCORE / FIXED") as what
// the host code (vsc_table_score, the checks of vsc_score_table_build) shares with the kernels of vsc_table.hip.  A header of
// its own, as vsc_pattern.h and vsc_bulge.h are.
//
// table_score below IS the score of include/varscot_hip.h for one read and one site in read orientation: table_score_kernel
// calls it for every record (the weights in LDS), vsc_table_score calls it on the host - one function, one order of the
// multiplications, the same bits.  Plain inline functions that a stand-alone program can include without a device.
#pragma once

#include <stdint.h>

#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif

namespace vsc {

constexpr uint32_t kTablePairs = 20 * 4 * 4;            // pair[j][g][s] at (j * 4 + g) * 4 + s
constexpr uint32_t kTableWeights = kTablePairs + 16;    // ... then pam[4 * s21 + s22]: 336 doubles, 2 688 bytes
constexpr uint32_t kTableProto = 0xFFFFFu;              // read positions 0..19: the positions that take part
constexpr uint32_t kTableOne = 1u << 30;                // the fixed-point unit: f = rint(x * 2^30)

// The score of a read (planes gh, gl: bit j = the code's high / low bit at read position j, as guide_planes makes them)
// against a site in READ orientation (sh, sl; 23 bases): the product over the mismatched read positions 0..19 in ascending
// order, then the weight of the site's letters at read positions 21 and 22.  One rounding per multiplication (there is no
// addition to contract with).
__host__ __device__ inline double table_score(const double *w, uint32_t gh, uint32_t gl, uint32_t sh, uint32_t sl)
{
    double x = 1.0;
    for (uint32_t rest = ((gh ^ sh) | (gl ^ sl)) & kTableProto; rest; rest &= rest - 1u) {
        const uint32_t j = (uint32_t)__builtin_ctz(rest);
        const uint32_t g = ((gh >> j) & 1u) << 1 | ((gl >> j) & 1u), s = ((sh >> j) & 1u) << 1 | ((sl >> j) & 1u);
        x = x * w[(j * 4u + g) * 4u + s];
    }
    const uint32_t s21 = ((sh >> 21) & 1u) << 1 | ((sl >> 21) & 1u), s22 = ((sh >> 22) & 1u) << 1 | ((sl >> 22) & 1u);
    return x * w[kTablePairs + 4u * s21 + s22];
}

// x in [0, 1] -> the unit of every sum, floor and selection key: rint(x * 2^30), round half to even, <= 2^30
__host__ __device__ inline uint32_t table_fixed(double x) { return (uint32_t)__builtin_rint(x * (double)kTableOne); }

// Is w a table the definition allows: every weight finite and in [0, 1] (a NaN fails both compares), every pair[j][b][b] exactly 1?
inline bool table_valid(const double *w)
{
    for (uint32_t i = 0; i < kTableWeights; ++i)
        if (!(w[i] >= 0.0 && w[i] <= 1.0)) return false;
    for (uint32_t j = 0; j < 20; ++j)
        for (uint32_t b = 0; b < 4; ++b)
            if (w[(j * 4u + b) * 4u + b] != 1.0) return false;
    return true;
}

}  // namespace vsc
