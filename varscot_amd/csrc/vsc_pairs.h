// vsc_pairs.h - what the host code of the paired-nickase calls (vsc_loci_pairs, vsc_guides_pairs, vsc_hits_pairs in
// vsc_api.cpp) shares with their kernels (vsc_pairs.hip).  The geometry - which start positions a partner window
// may have, the bound inside a run of records sorted by (contig, pos), the signed delta - is written once, as host + device
// inline functions: vsc_loci_pairs on the host and the two kernels are one formulation, as regions_locate (vsc_enum.h) is
// for the labels.
#pragma once

#include "vsc_internal.h"

namespace vsc {

constexpr int32_t kPairDeltaLimit = 1 << 30;  // |delta_min|, |delta_max| <= this (include/varscot_hip.h)
constexpr uint32_t kPairNoContig = 0xFFFFFFFFu;  // vsc_locus: takes part in nothing
constexpr int kPairRowWords = 28;  // vsc_pair_summary in 8-byte words: sites, nm_sum[17], nm_max[9], on_target | reserved
constexpr int kPairRowNmSum = 1, kPairRowNmMax = 18, kPairRowOnTarget = 27;

__host__ __device__ inline bool pair_params_ok(int32_t delta_min, int32_t delta_max)
{
    return delta_min <= delta_max && delta_min >= -kPairDeltaLimit && delta_max <= kPairDeltaLimit;
}

// The start positions [*lo, *hi] a window must have to be PAIRED with the window at pos on `strand` (1 = '-'), on the other
// strand of the same contig:  delta = pos('+') - pos('-')  in [delta_min, delta_max], so the '+' partner of a '-' window lies
// at pos + delta and the '-' partner of a '+' window at pos - delta.  64-bit signed, clipped to [0, UINT32_MAX]; false: no
// position is left.
__host__ __device__ inline bool pair_range(uint32_t pos, uint32_t strand, int32_t delta_min, int32_t delta_max, uint32_t *lo, uint32_t *hi)
{
    const long long a = strand ? (long long)pos + delta_min : (long long)pos - delta_max;
    const long long b = strand ? (long long)pos + delta_max : (long long)pos - delta_min;
    if (b < 0 || a > 0xFFFFFFFFll) return false;
    *lo = a < 0 ? 0u : (uint32_t)a;
    *hi = b > 0xFFFFFFFFll ? 0xFFFFFFFFu : (uint32_t)b;
    return true;
}

// delta of a window at pos on `strand` and its partner at partner_pos on the other strand
__host__ __device__ inline int32_t pair_delta(uint32_t pos, uint32_t strand, uint32_t partner_pos)
{
    return strand ? (int32_t)((long long)partner_pos - (long long)pos) : (int32_t)((long long)pos - (long long)partner_pos);
}

// (contig, pos) of a 16-byte record: vsc_hit (words 1, 2) or vsc_locus (words 0, 1)
template <bool kHit> __host__ __device__ inline uint32_t pair_contig(const uint4 &r) { return kHit ? r.y : r.x; }
template <bool kHit> __host__ __device__ inline uint32_t pair_pos(const uint4 &r) { return kHit ? r.z : r.y; }

// The first of records[i0 .. i1) - ascending (contig, pos) - that is not before (contig, pos); i1: there is none.  From
// there the partners are the records up to the first that pair_after() names.
template <bool kHit>
__host__ __device__ inline uint32_t pair_lower_bound(const uint4 *records, uint32_t i0, uint32_t i1, uint32_t contig, uint32_t pos)
{
    uint32_t lo = i0, hi = i1;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        const uint4 r = records[mid];
        const uint32_t c = pair_contig<kHit>(r);
        if (c < contig || (c == contig && pair_pos<kHit>(r) < pos)) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// r lies behind the last partner (the upper bound of the walk): another contig, or a start above hi
template <bool kHit> __host__ __device__ inline bool pair_after(const uint4 &r, uint32_t contig, uint32_t hi)
{
    return pair_contig<kHit>(r) != contig || pair_pos<kHit>(r) > hi;
}

// ---- vsc_hits_pairs ---------------------------------------------------------------------------------------------------------
// seg[2 guide + strand] = the first record of the run, seg[2 n_guides] = n: key_of(record) >= k, 2 n_guides + 1 lower bounds
struct PairSegArgs {
    const uint4 *records;  // [n] vsc_hit in vsc_search order
    uint32_t n, n_guides;
    uint32_t *seg;         // [2 n_guides + 1] out
};

// Work item i = (pair j, record r of guide a_j): j = the last pair with pair_off[j] <= i, r = seg[2 a_j] + i - pair_off[j].
struct PairJoinArgs {
    const uint4 *records;
    const uint32_t *seg;
    const uint2 *pairs;                  // [n_pairs] (a, b)
    const unsigned long long *pair_off;  // [n_pairs + 1] records of a_0 .. a_(j-1)
    uint32_t n_pairs;
    unsigned long long n_items;
    int32_t delta_min, delta_max;
    const uint4 *exclude;                // [n_guides] vsc_locus, or null
    unsigned long long *rows;            // [n_pairs x kPairRowWords], zeroed; the count pass adds into them
    uint32_t *item_count;                // [n_items] count pass: the item's counted sites (null: rows only)
    const unsigned long long *item_off;  // [n_items + 1] write pass: sites of all earlier items
    uint4 *sites;                        // write pass: vsc_pair_site {pair, a_rec, b_rec, delta}
};

// ---- vsc_guides_pairs -------------------------------------------------------------------------------------------------------
// Work item i = candidate i of loci[] in ascending (contig, pos, '+' before '-'); '-' candidates look for '+' partners.
struct PairLociArgs {
    const uint4 *loci;  // [n] vsc_locus {contig, pos, strand, 0}
    uint32_t n;
    int32_t delta_min, delta_max;
    uint32_t *item_count;                // [n] count pass
    const unsigned long long *item_off;  // [n + 1] write pass
    uint2 *pairs;                        // write pass: vsc_guide_pair (a, b)
};

hipError_t launch_pair_segments(const PairSegArgs &args, hipStream_t stream);
hipError_t launch_pair_join(const PairJoinArgs &args, bool write, int n_cus, hipStream_t stream);
hipError_t launch_pair_loci(const PairLociArgs &args, bool write, int n_cus, hipStream_t stream);

}  // namespace vsc
