// vsc_mh.h - the microhomology score and its out-of-frame share (include/varscot_hip.h "SHAPE / CONTEXT / CLASS /
// ROWS / SCORE / OUTPUT / FILTER") as what the host code (vsc_mh_score_text) shares with the kernels of vsc_mh.hip.  A header
// of its own, as vsc_efficiency.h is; the planes, the window and the reverse complement are that header's.
//
// mh_score below IS the score of one context in read orientation: mh_score_kernel and mh_filter_kernel call it for every
// candidate, vsc_mh_score_text calls it on the host - one function, integers only, the same bits.  mh_context is the other
// half: the class of a locus and the planes of its context out of a genome's plane words.  Plain inline functions that a
// stand-alone program can include without a device.
#pragma once

#include <stdint.h>

#include "vsc_efficiency.h"

namespace vsc {

constexpr uint32_t kMhMinFlank = 8, kMhMaxFlank = 32;  // W = 2 F <= 64
constexpr uint32_t kMhUndefined = 0xFFFFFFFFu;         // sum and oof of a candidate whose class is not defined

struct MhShape {
    uint32_t site_len, cut, flank;  // the break lies between read positions cut - 1 and cut of the site
};

// Is s a shape the definition allows?  site_len 16 .. 32, cut 0 .. site_len, flank 8 .. 32.
__host__ __device__ inline bool mh_shape_valid(const MhShape &s)
{
    return s.site_len >= kEffMinSite && s.site_len <= kEffMaxSite && s.cut <= s.site_len && s.flank >= kMhMinFlank && s.flank <= kMhMaxFlank;
}

// T[d] = round(exp(-d / 20), 3) * 1000: no d in 1 .. 63 lies within 0.0047 of a tie, so the table is the same under any rounding
__host__ __device__ inline uint32_t mh_weight(uint32_t d)
{
    constexpr uint32_t T[64] = {1000, 951, 905, 861, 819, 779, 741, 705, 670, 638, 607, 577, 549, 522, 497, 472,
                                449,  427, 407, 387, 368, 350, 333, 317, 301, 287, 273, 259, 247, 235, 223, 212,
                                202,  192, 183, 174, 165, 157, 150, 142, 135, 129, 122, 116, 111, 105, 100, 95,
                                91,   86,  82,  78,  74,  71,  67,  64,  61,  58,  55,  52,  50,  47,  45,  43};
    return T[d & 63u] & 0xFFFFu;  // (the mask tells the compiler that a 24-bit multiply holds the products)
}

// sum and oof (tenths of the published score) of a context of W = 2 F letters in READ orientation (planes ch, cl: bit j = the
// high / low bit of the letter at context position j, A 0, C 1, G 2, T 3; the bits from W on are 0).  Per deletion length d
// the kept rows are the maximal runs of length >= 2 of s[p] == s[p + d] over p in [max(0, F - d), min(F, W - d)): m2 holds
// their positions, and a run of length k with g G/C scores T[d] (k + g) - the sum over the runs is T[d] (popc(m2) + popc(m2 &
// gcm)).  The one run the published range(2, left) does not list is the run of length F at d = F: it counts as its two rows
// of length F - 1, and is put right behind the loop.  The loop has W - 1 steps whatever the letters are.
__host__ __device__ inline void mh_score(uint64_t ch, uint64_t cl, uint32_t F, uint32_t *sum, uint32_t *oof)
{
    const uint32_t W = 2u * F;
    const uint64_t gcm = ch ^ cl, left = eff_low_bits(F);  // G = 10, C = 01
    uint32_t all = 0, in_frame = 0;                        // over every d, over d % 3 == 0
    uint32_t phase = 1;                                    // d % 3
    for (uint32_t d = 1; d < W; ++d) {
        const uint64_t ne = (ch ^ (ch >> d)) | (cl ^ (cl >> d));
        // p < min(F, W - d) and p >= max(0, F - d)
        const uint64_t range = d <= F ? left & ~eff_low_bits(F - d) : eff_low_bits(W - d);
        const uint64_t m = ~ne & range;
        const uint64_t m2 = m & (m << 1 | m >> 1);
        const uint32_t rows = (uint32_t)(__builtin_popcountll(m2) + __builtin_popcountll(m2 & gcm));
        const uint32_t t = mh_weight(d);  // (d is the same on every lane: the weight and the choice below are scalar work)
        all += t * rows;
        in_frame += (phase == 0u ? t : 0u) * rows;
        phase = phase == 2u ? 0u : phase + 1u;
    }
    if ((((ch ^ (ch >> F)) | (cl ^ (cl >> F))) & left) == 0) {  // the left half repeated as the right half
        const uint32_t listed = F + (uint32_t)__builtin_popcountll(gcm & left);
        const uint32_t rows = 2u * (F - 1u) + (uint32_t)__builtin_popcountll(gcm & (left >> 1)) + (uint32_t)__builtin_popcountll(gcm & left & ~1ull);
        const uint32_t more = mh_weight(F) * (rows - listed);  // rows - listed = F - 2 + #G/C in [1, F - 1) > 0
        all += more;
        in_frame += F % 3u == 0u ? more : 0u;
    }
    *sum = all;
    *oof = all - in_frame;
}

// The FILTER rule: does a candidate of class cls with (sum, oof) pass the floors?
__host__ __device__ inline bool mh_keep(uint32_t cls, uint32_t sum, uint32_t oof, uint32_t min_sum, uint32_t min_oof_permille)
{
    if (cls != kEffDefined || sum < min_sum) return false;
    if (sum == 0u) return min_oof_permille == 0u;
    return 1000ull * oof >= (uint64_t)min_oof_permille * sum;
}

// The class of locus (contig, pos, strand) under shape s, tested in the order of EffClass, and - for kEffDefined - the planes
// of its context in read orientation: read positions [cut - F, cut + F) of the site, on '+' c[pos + cut - F, pos + cut + F),
// on '-' the reverse complement of c[pos + site_len - cut - F, pos + site_len - cut + F).  The context may start in front of
// the site (or of the contig: the start is a signed 64-bit number).
__host__ __device__ inline uint32_t mh_context(const EffPlanes &g, const MhShape &s, uint32_t contig, uint32_t pos, uint32_t strand,
                                               uint64_t *ch, uint64_t *cl)
{
    if (contig >= g.n_contigs || strand > 1u) return kEffInvalid;
    const uint32_t off = g.contig_off[contig], len = g.contig_end[contig] - off;
    if (pos > len || len - pos < s.site_len) return kEffInvalid;  // pos + site_len <= len, without the overflow
    const uint32_t W = 2u * s.flank;
    const int64_t start = (int64_t)pos + (int64_t)(strand ? s.site_len - s.cut : s.cut) - (int64_t)s.flank;  // in the contig
    if (start < 0 || start + (int64_t)W > (int64_t)len) return kEffOffContig;
    const uint64_t first = (uint64_t)off + (uint64_t)start;  // global position of the context's first base on the forward strand
    if (first < g.first_word * 32u || first + W > (g.first_word + g.held_words) * 32u) return kEffNotResident;
    const uint64_t at = first - g.first_word * 32u;
    // (the three planes' words are asked for together: one memory latency, not two, in front of the loop)
    const uint64_t n = eff_window(g.nm, g.n_words, at, W), h = eff_window(g.hi, g.n_words, at, W), l = eff_window(g.lo, g.n_words, at, W);
    if (n) return kEffHasN;
    *ch = strand ? eff_revcomp(h, W) : h;
    *cl = strand ? eff_revcomp(l, W) : l;
    return kEffDefined;
}

}  // namespace vsc
