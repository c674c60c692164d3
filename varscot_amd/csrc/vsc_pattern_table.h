// vsc_pattern_table.h - the table score of a pattern hit (CFD form for any nuclease; DESIGN 4.22, include/varscot_hip.h
// "TABLE / SCORE / FIXED" of vsc_search_pattern_table) as what the host code (vsc_pattern_table_build, vsc_pattern_table_score)
// shares with the kernels of vsc_pattern.hip.  A header of its own, modelled on vsc_table.h.
//
// pattern_table_score below IS the score of include/varscot_hip.h for one guide and one site in read orientation: the scored
// write pass calls it for every hit (the weights in LDS), vsc_pattern_table_score calls it on the host - one function, one
// order of the multiplications, the same bits.  Plain inline functions that a stand-alone program can include without a device.
#pragma once

#include <stdint.h>

#include "vsc_table.h"  // table_fixed, kTableOne: the fixed-point unit is the plain path's

namespace vsc {

constexpr uint32_t kPatTableMaxLen = 32, kPatTableMinLen = 16;
constexpr uint32_t kPatTableMaxPam = 4;
// the flat weights: pair[i][g][s] at (i * 4 + g) * 4 + s for i < ps_len, then pam[k] at ps_len * 16 + k for k < 4^n_pam -
// at the most 32 * 16 + 256 doubles, 6 KB
constexpr uint32_t kPatTableMaxWeights = kPatTableMaxLen * 16 + 256;

// vsc_pattern_table_shape, field for field
struct PatTableShape {
    uint32_t len, ps_start, ps_len, n_pam;
    uint32_t pam_pos[kPatTableMaxPam];
};

__host__ __device__ inline uint32_t pattern_table_pairs(const PatTableShape &sh) { return sh.ps_len * 16u; }
__host__ __device__ inline uint32_t pattern_table_weights(const PatTableShape &sh) { return sh.ps_len * 16u + (1u << (2u * sh.n_pam)); }
// bits ps_start .. ps_start + ps_len - 1
__host__ __device__ inline uint32_t pattern_table_proto(const PatTableShape &sh)
{
    return (sh.ps_len < 32u ? (1u << sh.ps_len) - 1u : ~0u) << sh.ps_start;
}

// Is the shape one the definition allows: L 16..32, a non-empty protospacer inside the L positions, at most four PAM
// positions, strictly ascending, below L and outside the protospacer?
inline bool pattern_table_shape_valid(const PatTableShape &sh)
{
    if (sh.len < kPatTableMinLen || sh.len > kPatTableMaxLen) return false;
    if (sh.ps_len < 1 || sh.ps_start > sh.len || sh.ps_len > sh.len - sh.ps_start) return false;
    if (sh.n_pam > kPatTableMaxPam) return false;
    for (uint32_t t = 0; t < sh.n_pam; ++t) {
        const uint32_t p = sh.pam_pos[t];
        if (p >= sh.len || (p >= sh.ps_start && p < sh.ps_start + sh.ps_len)) return false;
        if (t && p <= sh.pam_pos[t - 1]) return false;
    }
    return true;
}

// Is w (pattern_table_weights(sh) doubles) a table the definition allows: the shape valid, every weight finite and in [0, 1]
// (a NaN fails both compares), every pair[i][b][b] exactly 1?
inline bool pattern_table_valid(const PatTableShape &sh, const double *w)
{
    if (!pattern_table_shape_valid(sh)) return false;
    const uint32_t n = pattern_table_weights(sh);
    for (uint32_t i = 0; i < n; ++i)
        if (!(w[i] >= 0.0 && w[i] <= 1.0)) return false;
    for (uint32_t i = 0; i < sh.ps_len; ++i)
        for (uint32_t b = 0; b < 4; ++b)
            if (w[(i * 4u + b) * 4u + b] != 1.0) return false;
    return true;
}

// A guide as the score reads it: bit j of gh / gl = the high / low bit of the letter's code (A 00, C 01, G 10, T 11) at read
// position j, bit j of single = the letter is one of A, C, G, T.  sets[j]: the letter's set of bases (vsc_pattern.h: iupac_set).
__host__ __device__ inline void pattern_table_guide(const uint8_t *sets, uint32_t len, uint32_t *gh, uint32_t *gl, uint32_t *single)
{
    *gh = *gl = *single = 0;
    for (uint32_t j = 0; j < len; ++j) {
        const uint32_t s = sets[j];
        if (s == 1u || s == 2u || s == 4u || s == 8u) {
            const uint32_t code = s == 1u ? 0u : s == 2u ? 1u : s == 4u ? 2u : 3u;
            *gh |= (code >> 1) << j;
            *gl |= (code & 1u) << j;
            *single |= 1u << j;
        }
    }
}

// The score of a guide (gh, gl, single: pattern_table_guide) against a site in READ orientation (sh_, sl_: bit j = the code of
// s[j]; the bits from L on may hold anything): the product over the protospacer positions whose guide letter is a single
// base that the site does not hold, in ascending order, then the weight of the site's letters at the PAM positions.  One
// rounding per multiplication (there is no addition to contract with).
__host__ __device__ inline double pattern_table_score(const double *w, const PatTableShape &shape, uint32_t gh, uint32_t gl, uint32_t single,
                                                      uint32_t sh_, uint32_t sl_)
{
    double x = 1.0;
    for (uint32_t rest = ((gh ^ sh_) | (gl ^ sl_)) & single & pattern_table_proto(shape); rest; rest &= rest - 1u) {
        const uint32_t j = (uint32_t)__builtin_ctz(rest), i = j - shape.ps_start;
        const uint32_t g = ((gh >> j) & 1u) << 1 | ((gl >> j) & 1u), s = ((sh_ >> j) & 1u) << 1 | ((sl_ >> j) & 1u);
        x = x * w[(i * 4u + g) * 4u + s];
    }
    uint32_t k = 0;
    for (uint32_t t = 0; t < shape.n_pam; ++t) {
        const uint32_t p = shape.pam_pos[t];
        k = k << 2 | ((sh_ >> p) & 1u) << 1 | ((sl_ >> p) & 1u);
    }
    return x * w[pattern_table_pairs(shape) + k];
}

}  // namespace vsc
