// vsc_pattern_variants.h - pattern hits in an individual's genome (vsc_pattern_hits_variants, vsc_pattern_hits_shadowed,
// vsc_search_pattern_variants): what the host calls (vsc_varmap.cpp), the entry points (vsc_api.cpp), the kernels
// (vsc_pattern_variants.hip) and the stand-alone check program (tools/pattern_variants_check.cpp) share.  The walk over a
// window's variants is vsc_varmap.h's, with the site's length L in place of 23; what is added here is the length-aware interval
// search of the reference side and the L-base site compare of the window side, one __host__ __device__ definition each.
#pragma once

#include "vsc_varmap.h"

namespace vsc {

constexpr uint32_t kPatVarMinLen = 16, kPatVarMaxLen = 32;  // VSC_PATTERN_MIN_LEN .. VSC_PATTERN_MAX_LEN

// filterRefAlignment (variant_processing/filter_output_bam.h:70-124) for a site of `len` bases at global position pos, over the
// shadow intervals sorted by start: n = #{start <= pos}; inside iff n > 0 and end_max[n - 1] >= pos + len.  The interval that
// holds the running maximum starts at or before pos and ends at or behind the site, so the site lies inside ONE interval; no
// interval reaches across a contig boundary, so the maximum over earlier contigs stays below every later position.
__host__ __device__ inline bool shadow_search(const uint32_t *start, const uint32_t *end_max, uint32_t n, uint32_t pos, uint32_t len)
{
    uint32_t lo = 0, hi = n;  // -> #{start <= pos}
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (start[mid] <= pos) lo = mid + 1; else hi = mid;
    }
    return lo > 0 && (unsigned long long)end_max[lo - 1] >= (unsigned long long)pos + len;
}

// The low `len` bits, len in 1..32 (32: no shift by the word's width).
__host__ __device__ inline uint32_t site_mask(uint32_t len) { return len >= 32u ? ~0u : (1u << len) - 1u; }

// The `len` bits from bit sh (0..31) of the word pair {w1, w0} on: a funnel shift (one v_alignbit_b32 on the device) and a mask.
__host__ __device__ inline uint32_t site_bits(uint32_t w1, uint32_t w0, uint32_t sh, uint32_t len)
{
    return (uint32_t)((((unsigned long long)w1 << 32) | w0) >> (sh & 31u)) & site_mask(len);
}

// The site of `len` bases that starts at bit `rel` of a bit plane of n_words words (rel >> 5 < n_words: the caller has
// checked; the word behind the plane's last reads as 0).  Two words per plane and site.
__host__ __device__ inline uint32_t plane_site(const uint32_t *plane, unsigned long long n_words, unsigned long long rel, uint32_t len)
{
    const unsigned long long wi = rel >> 5;
    const uint32_t w0 = plane[wi], w1 = wi + 1 < n_words ? plane[wi + 1] : 0u;
    return site_bits(w1, w0, (uint32_t)(rel & 31u), len);
}

// A guide's row over the counted records of one side (vsc_pattern_variant_row of include/varscot_hip.h), as the kernels add to it.
struct PatVarRow {
    uint32_t count[VSC_MAX_MISMATCHES + 1];
    uint32_t on_target;
    unsigned long long dropped;
};
static_assert(sizeof(PatVarRow) == 48, "pattern variant row layout");
constexpr int kPatVarTableWords = 12;  // vsc_guide_table_row: score_sum, positive, positive_nm[9], reserved

// pattern_variant_merge_kernel / pattern_shadow_kernel: labels or flags and / or per-guide rows over vsc_pattern_hit records
// in the search's order.
struct PatVarArgs {
    VarMapView map;                 // window side: the context's device copy
    const uint32_t *records;        // [5 n] vsc_pattern_hit as words
    const uint32_t *fixed;          // [n] the records' score words (a scored search); only read by the scored kernels
    unsigned long long n;
    uint32_t len;                   // L, kPatVarMinLen..kPatVarMaxLen
    const uint32_t *hi, *lo;        // window side: the window genome's resident planes
    uint32_t first_pos;             // global position of bit 0 of word 0
    unsigned long long n_plane_words;
    const uint32_t *contig_off, *contig_end;  // the searched genome's table, global positions
    uint32_t n_contigs;             // ... and its entries (window side: == map.n_windows)
    const uint32_t *sh_start, *sh_end_max;    // reference side: the shadow intervals (shadow_search)
    uint32_t sh_n;
    const uint4 *exclude;           // [n_guides] vsc_locus in reference coordinates; null: none
    uint32_t n_guides;
    uint4 *labels;                  // window side: [n] vsc_variant_label out; null: not wanted
    uint8_t *flags;                 // reference side: [n] VSC_PATTERN_REF_* out; null: not wanted
    PatVarRow *rows_all, *rows_var; // [n_guides], zeroed by the caller; rows_all null: no rows (rows_var: window side only)
    unsigned long long *table_all, *table_var;  // [n_guides] x kPatVarTableWords, zeroed; the scored kernels only, with rows
    uint32_t *error;                // set to 1 when a record lies outside the map, its window or contig, or the guides
};

hipError_t launch_pattern_variant_merge(const PatVarArgs &args, hipStream_t stream);  // window side
hipError_t launch_pattern_shadow(const PatVarArgs &args, hipStream_t stream);         // reference side

}  // namespace vsc
