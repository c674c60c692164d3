// vsc_variation.h - known variation under candidate guides (include/varscot_hip.h "SHAPE / SITE / CLASS / VARIANTS /
// OVERLAP / SILENT / DISRUPTING / ROW / PAIR / COVERAGE / FILTER") as what the host code (vsc_variation_host) shares with the
// kernels of vsc_variation.hip.  A header of its own, as vsc_edit.h is; the planes and the class of a site are
// vsc_efficiency.h's.
//
// var_touch below IS the relation of one variant to one site, var_add IS the row's arithmetic, var_first IS the lookup and
// var_row IS the walk: var_rows_kernel, var_pairs_kernel and var_filter_kernel call them for every candidate,
// vsc_variation_host calls them on the host - one function each, integers only, the same bits.  var_site is the other half: the
// class of a locus out of a genome's plane words.  Plain inline functions that a stand-alone program can include without a device.
#pragma once

#include <stdint.h>

#include "vsc_efficiency.h"

namespace vsc {

constexpr uint32_t kVarUndefined = 0xFFFFFFFFu;  // the four words of the row of a candidate whose class is not defined
constexpr uint32_t kVarMaxCount = 0xFFFFFFFEu;   // candidates, variants and pairs of one call; the largest weight and cost
constexpr uint32_t kVarOther = 4u;               // alt of a variant that is no SNV
constexpr uint32_t kVarBlockBits = 8u;           // the lookup's default block: 256 global positions
constexpr uint32_t kVarMinBlockBits = 4u, kVarMaxBlockBits = 32u;

struct VarShape {
    uint32_t site_len;
    uint64_t zones;      // two bits per read position: the caller's label 0 .. 3
    uint64_t accept[2];  // four bits per read position: bit b = "read base b here leaves the site usable"
};

// Is s a shape the definition allows?  site_len 16 .. 32, no zone or accept bit at a position from site_len on.
__host__ __device__ inline bool var_shape_valid(const VarShape &s)
{
    if (s.site_len < kEffMinSite || s.site_len > kEffMaxSite) return false;
    if (s.site_len < 32u && (s.zones >> (2u * s.site_len)) != 0u) return false;
    const uint32_t behind = s.site_len - 16u;  // positions of accept[1] in use: 0 .. 16
    if (behind < 16u && (s.accept[1] >> (4u * behind)) != 0u) return false;
    return true;
}

// The class of locus (contig, pos, strand), tested in the order of EffClass: eff_context with no flank on either side, so that
// kEffOffContig cannot come out.  The letters of the site do not matter here, only whether it has them.
__host__ __device__ inline uint32_t var_site(const EffPlanes &g, const VarShape &s, uint32_t contig, uint32_t pos, uint32_t strand)
{
    const EffShape site{0u, s.site_len, 0u, 0u, 0u};
    uint64_t ch = 0, cl = 0;
    return eff_context(g, site, contig, pos, strand, &ch, &cl);
}

// A variant as the kernels hold it: its global position (contig offset + pos, 32-bit as contig_off is), span | alt << 16, its
// weight, and reach = the largest gpos + span over the variants up to and including this one - a prefix maximum, so that
// reach never decreases along the array.  16 bytes: one load per step of a walk.
struct alignas(16) VarRec {
    uint32_t gpos, span_alt, weight, reach;
};

// The variants of a call and the lookup's block table: first[b] = the first k with reach[k] > b << bits, for b = 0 .. n_blocks
// (n_blocks + 1 entries, n_blocks = the blocks the genome's global positions fill).
struct VarTable {
    const VarRec *rec;
    const uint32_t *first;
    uint32_t n, bits, n_blocks;
};

// the blocks that `total` global positions fill under blocks of 1 << bits
__host__ __device__ inline uint32_t var_block_count(uint64_t total, uint32_t bits)
{
    return (uint32_t)((total + ((1ull << bits) - 1ull)) >> bits);
}

// the first k in [lo, hi] with reach[k] > g (hi: none in [lo, hi)): a lower bound over the non-decreasing reach
__host__ __device__ inline uint32_t var_first_reach(const VarRec *rec, uint32_t lo, uint32_t hi, uint64_t g)
{
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if ((uint64_t)rec[mid].reach <= g) lo = mid + 1u;
        else hi = mid;
    }
    return lo;
}

// The first variant that can overlap a site whose first base is at global position g0: one table load (two adjacent entries)
// and a lower bound confined to them.  A g0 behind the table's blocks (no defined candidate has one) searches nothing.
__host__ __device__ inline uint32_t var_first(const VarTable &t, uint32_t g0)
{
    const uint64_t b = (uint64_t)g0 >> t.bits;
    if (b >= t.n_blocks) return t.n;
    uint32_t lo = t.first[b], hi = t.first[b + 1u];
    if (hi > t.n) hi = t.n;  // (a table entry never is: the bound keeps a walk inside rec whatever the table holds)
    if (lo > hi) lo = hi;
    return var_first_reach(t.rec, lo, hi, g0);
}

// OVERLAP / SILENT / DISRUPTING of variant r against the site [g0, g0 + site_len) read on `strand`: false when they do not
// overlap, else *info = smallest touched read position | touched positions << 8 | top << 16 | silent << 18.  top is the largest
// zone label among the touched positions (for a silent SNV: the label of its position).
__host__ __device__ inline bool var_touch(const VarRec &r, uint32_t g0, uint32_t strand, const VarShape &s, uint32_t *info)
{
    const uint32_t span = r.span_alt & 0xFFFFu, alt = r.span_alt >> 16;
    const uint32_t end = g0 + s.site_len, r_end = r.gpos + span;  // (both inside a contig: no overflow)
    if (!(r.gpos < end && r_end > g0)) return false;
    const uint32_t f_lo = (r.gpos > g0 ? r.gpos : g0) - g0, f_hi = (r_end < end ? r_end : end) - g0;  // touched forward [f_lo, f_hi)
    const uint32_t touched = f_hi - f_lo, j0 = strand ? s.site_len - f_hi : f_lo;                     // touched read [j0, j0 + touched)
    const uint64_t z = (s.zones >> (2u * j0)) & eff_low_bits(2u * touched);
    const uint64_t hb = z & 0xAAAAAAAAAAAAAAAAull, lb = z & 0x5555555555555555ull;
    const uint32_t top = hb ? 2u + (uint32_t)(((lb << 1) & hb) != 0ull) : (uint32_t)(lb != 0ull);
    uint32_t silent = 0;
    if (alt < kVarOther) {  // an SNV: span 1, one touched position
        const uint32_t b = strand ? 3u - alt : alt;
        silent = (uint32_t)(s.accept[j0 >> 4] >> (4u * (j0 & 15u)) >> b) & 1u;
    }
    *info = j0 | touched << 8 | top << 16 | silent << 18;
    return true;
}

// ROW as it is summed: by_zone with its bytes saturated at 255, the cost in 64 bits
struct VarRow {
    uint32_t by_zone, silent, max_weight;
    uint64_t cost;
};

__host__ __device__ inline void var_add(VarRow &row, uint32_t info, uint32_t weight)
{
    if (info >> 18 & 1u) {
        ++row.silent;
        return;
    }
    const uint32_t sh = 8u * (info >> 16 & 3u);
    row.by_zone += (uint32_t)((row.by_zone >> sh & 255u) != 255u) << sh;
    row.cost += weight;
    if (weight > row.max_weight) row.max_weight = weight;
}

// the clamped cost of a row
__host__ __device__ inline uint32_t var_cost(const VarRow &row) { return row.cost > kVarMaxCount ? kVarMaxCount : (uint32_t)row.cost; }

// The walk of a site at global g0: from var_first while gpos < g0 + site_len, OVERLAP tested per variant.  *pairs (optional) =
// the overlapping variants, silent ones included.
__host__ __device__ inline VarRow var_row(const VarTable &t, uint32_t g0, uint32_t strand, const VarShape &s, uint64_t *pairs)
{
    VarRow row{0u, 0u, 0u, 0ull};
    uint64_t n = 0;
    for (uint32_t k = var_first(t, g0); k < t.n; ++k) {
        const VarRec r = t.rec[k];
        if (r.gpos >= g0 + s.site_len) break;
        uint32_t info;
        if (!var_touch(r, g0, strand, s, &info)) continue;
        var_add(row, info, r.weight);
        ++n;
    }
    if (pairs) *pairs = n;
    return row;
}

// do the bytes of by_zone and `silent` give the pairs of a row?  Not when a byte stands at its bound.
__host__ __device__ inline bool var_row_counts(uint32_t by_zone)
{
    return (by_zone & 0xFFu) != 0xFFu && (by_zone >> 8 & 0xFFu) != 0xFFu && (by_zone >> 16 & 0xFFu) != 0xFFu && (by_zone >> 24) != 0xFFu;
}

struct VarFilter {
    uint32_t max_cost, max_by_zone, require_zones;
};

// The FILTER rule: does a candidate of class cls with (by_zone, cost) pass?
__host__ __device__ inline bool var_keep(uint32_t cls, uint32_t by_zone, uint32_t cost, const VarFilter &f)
{
    if (cls != kEffDefined || cost > f.max_cost) return false;
    bool required = f.require_zones == 0u;
    for (uint32_t z = 0; z < 4u; ++z) {
        const uint32_t have = by_zone >> (8u * z) & 255u;
        if (have > (f.max_by_zone >> (8u * z) & 255u)) return false;
        required = required || ((f.require_zones >> z & 1u) && have != 0u);
    }
    return required;
}

}  // namespace vsc
