// vsc_varmap.h - the variant map (vsc_variant_map_*, vsc_hits_variants, vsc_search_summary_variants): what the
// host object (vsc_varmap.cpp), the entry points (vsc_api.cpp) and the merge kernel (vsc_variants.hip) share.  A header of its
// own, as vsc_enum.h is.  The walk over a window's variants (getSnpType, variant_processing/filter_output_bam.h:189-263) is one
// function for the host's vsc_variant_map_locate and for the kernel.
#pragma once

#include <string>
#include <vector>

#include "vsc_internal.h"

namespace vsc {

// One window (= contig of the window genome), 16 bytes: one load per record.  Entry n_windows closes the table (var_off = the
// number of variants).
struct VarWindow {
    uint32_t contig;   // reference contig of id[0]; UINT32_MAX: unknown
    uint32_t start;    // (uint32) atoi(id[1])
    uint32_t var_off;  // the window's variants are var[var_off .. next window's var_off)
    uint32_t chr_id;   // number of the string id[0]: equal ids <=> equal strings (unknown chromosomes differ among themselves)
};
// One variant of one window, 16 bytes, in id order.
struct VarEntry {
    int32_t p;                  // atoi(id[k])
    uint32_t len_ref, len_alt;  // lengths of id[k + 1], id[k + 2]
    uint32_t tag_id;            // number of the pair of strings (id[0], id[k])
};
static_assert(sizeof(VarWindow) == 16 && sizeof(VarEntry) == 16, "variant map layout");

struct VarMapView {
    const VarWindow *win;  // [n_windows + 1]
    const VarEntry *var;   // [n_variants]
    uint32_t n_windows, n_variants;
};

// Is the variant covered by the `len` bases from pos1 on (len = the site's length: VSC_READ_LEN for the plain search, the
// pattern's L for pattern hits)?  A substitution of equal lengths by its position, an indel by its two end points
// p + 1 and p + max(len) - 1 (:203-252; the reference computes in long).
__host__ __device__ inline bool var_covered(const VarEntry &e, uint32_t pos1, uint32_t len)
{
    const long long lo = (long long)pos1, hi = lo + (long long)len, p = e.p;
    if (e.len_ref == e.len_alt) return lo <= p && p < hi;
    const long long far = p + (long long)(e.len_ref > e.len_alt ? e.len_ref : e.len_alt) - 1;
    return (lo <= p + 1 && p + 1 < hi) || (lo <= far && far < hi);
}

// The variants [*b, *e) of window w, clamped to the table whatever it says.
__host__ __device__ inline void var_range(const VarMapView &m, uint32_t w, uint32_t *b, uint32_t *e)
{
    uint32_t first = m.win[w].var_off, last = m.win[w + 1].var_off;
    if (last > m.n_variants) last = m.n_variants;
    if (first > last) first = last;
    *b = first;
    *e = last;
}

// getSnpType for the site of `len` bases at the window position (w, pos), w < n_windows: pos1 = pos + start; the covered
// variants are counted, an uncovered indel before the first covered variant moves the position by len_ref - len_alt (int
// arithmetic in the reference: 32-bit wrap here); *pos2 = pos1 + that sum, *n_var = covered variants.
__host__ __device__ inline void varmap_walk(const VarMapView &m, uint32_t w, uint32_t pos, uint32_t len, uint32_t *pos2, uint32_t *n_var)
{
    const uint32_t pos1 = pos + m.win[w].start;
    uint32_t b, e, shift = 0, n = 0;
    var_range(m, w, &b, &e);
    for (uint32_t k = b; k < e; ++k) {
        const VarEntry v = m.var[k];
        if (var_covered(v, pos1, len)) ++n;
        else if (n == 0 && v.len_ref != v.len_alt) shift += v.len_ref - v.len_alt;
    }
    *pos2 = pos1 + shift;
    *n_var = n;
}

// Do the two sites of `len` bases at two window positions carry the same tag?  Both have n covered variants (n > 0: the caller has compared the counts and
// the chromosomes): the covered tag ids of the two windows, in lockstep.
__host__ __device__ inline bool var_tags_equal(const VarMapView &m, uint32_t wa, uint32_t posa, uint32_t wb, uint32_t posb, uint32_t n,
                                              uint32_t len)
{
    const uint32_t pa = posa + m.win[wa].start, pb = posb + m.win[wb].start;
    uint32_t ka, ea, kb, eb;
    var_range(m, wa, &ka, &ea);
    var_range(m, wb, &kb, &eb);
    for (uint32_t i = 0; i < n; ++i) {
        while (ka < ea && !var_covered(m.var[ka], pa, len)) ++ka;
        while (kb < eb && !var_covered(m.var[kb], pb, len)) ++kb;
        if (ka >= ea || kb >= eb) return false;  // (cannot happen with the counts equal)
        if (m.var[ka].tag_id != m.var[kb].tag_id) return false;
        ++ka;
        ++kb;
    }
    return true;
}

// variant_merge_kernel (vsc_variants.hip): labels and / or per-guide rows over sorted vsc_hit records of the window genome.
struct VariantArgs {
    VarMapView map;                       // the context's device copy
    const uint4 *records;                 // [n] vsc_hit, vsc_search order
    unsigned long long n;
    const uint32_t *hi, *lo;              // the window genome's resident planes
    uint32_t first_pos;                   // global position of bit 0 of word 0
    unsigned long long n_plane_words;
    const uint32_t *contig_off, *contig_end;  // [map.n_windows] the window genome's table, global positions
    const uint4 *exclude;                 // [n_guides] vsc_locus in reference coordinates; null: none
    uint32_t n_guides;
    uint4 *labels;                        // [n] vsc_variant_label out; null: not wanted
    unsigned long long *rows_all, *rows_var;  // [n_guides] rows of kSumWords words, zeroed by the caller; null: not wanted
    unsigned long long *dups;             // [n_guides]; null: not wanted
    uint32_t *error;                      // set to 1 when a record lies outside the map, its window or the guides
};

hipError_t launch_variant_merge(const VariantArgs &args, hipStream_t stream);

}  // namespace vsc

// The object behind vsc_variant_map (include/varscot_hip.h; built by vsc_varmap.cpp).  Immutable once built.
struct vsc_variant_map {
    std::vector<vsc::VarWindow> win;  // n_windows + 1
    std::vector<vsc::VarEntry> var;
    std::vector<uint32_t> win_len;    // the window genome's contig lengths (what a genome is checked against)
    std::vector<vsc_contig> ref_contigs;
    // the texts, for vsc_variant_map_tag: chr_names[chr_id], and per variant its id[k] as (offset, length) into text
    std::vector<std::string> chr_names;
    std::string text;
    std::vector<uint32_t> text_off;   // n_variants + 1
    // the shadow intervals of vsc_variant_map_shadow in the reference's global positions, sorted by start: start[] and the
    // running maximum of their ends (vsc::shadow_search, vsc_pattern_variants.h: the reference side for a site of any length)
    std::vector<uint32_t> shadow_start, shadow_end_max;
    uint64_t serial = 0;  // process-wide, as vsc_regions': what a context's device copy is keyed by
    vsc_variant_map_stats stats{};
    vsc::VarMapView view() const { return vsc::VarMapView{win.data(), var.data(), (uint32_t)(win.size() - 1), (uint32_t)var.size()}; }
};
