// vsc_edit.h - base-editor windows of candidate guides (include/varscot_hip.h "SHAPE / SITE / CLASS / MASK /
// FORWARD / TARGETS / HITS / ROW / PAIR / COVERAGE / FILTER") as what the host code (vsc_edit_site_text) shares with the
// kernels of vsc_edit.hip.  A header of its own, as vsc_mh.h is; the planes, the window and the reverse complement are
// vsc_efficiency.h's.
//
// edit_mask below IS the mask of one site in read orientation and edit_hits IS its join with the targets: edit_rows_kernel,
// edit_pairs_kernel and edit_filter_kernel call them for every candidate, vsc_edit_site_text calls edit_mask on the host - one
// function each, integers only, the same bits.  edit_site is the other half: the class of a locus and the planes of its site
// out of a genome's plane words.  Plain inline functions that a stand-alone program can include without a device.
#pragma once

#include <stdint.h>

#include "vsc_efficiency.h"

namespace vsc {

constexpr uint32_t kEditMaxWindow = 16;
constexpr uint32_t kEditUndefined = 0xFFFFFFFFu;  // mask and hits of a candidate whose class is not defined
constexpr uint32_t kEditMaxCount = 0xFFFFFFFEu;   // candidates, targets and pairs of one call

struct EditShape {
    uint32_t site_len, win_start, win_len;  // the window: read positions [win_start, win_start + win_len) of the site
    uint32_t from;                          // 0 .. 3 (A C G T): the base the editor converts on the read strand
};

// Is s a shape the definition allows?  site_len 16 .. 32, 1 <= win_len <= 16, the window inside the site, from 0 .. 3.
__host__ __device__ inline bool edit_shape_valid(const EditShape &s)
{
    return s.site_len >= kEffMinSite && s.site_len <= kEffMaxSite && s.win_len >= 1u && s.win_len <= kEditMaxWindow &&
           s.win_start <= s.site_len && s.win_len <= s.site_len - s.win_start && s.from <= 3u;
}

// The class of locus (contig, pos, strand), tested in the order of EffClass, and - for kEffDefined - the planes of its site in
// read orientation: eff_context with no flank on either side, so that kEffOffContig cannot come out.
__host__ __device__ inline uint32_t edit_site(const EffPlanes &g, const EditShape &s, uint32_t contig, uint32_t pos, uint32_t strand,
                                              uint64_t *ch, uint64_t *cl)
{
    const EffShape site{0u, s.site_len, 0u, 0u, 0u};
    return eff_context(g, site, contig, pos, strand, ch, cl);
}

// MASK: bit j is set iff the read base at win_start + j is `from` - two plane compares and a shift
__host__ __device__ inline uint32_t edit_mask(uint64_t ch, uint64_t cl, const EditShape &s)
{
    const uint64_t same = (s.from & 2u ? ch : ~ch) & (s.from & 1u ? cl : ~cl);
    return (uint32_t)(same >> s.win_start) & ((1u << s.win_len) - 1u);
}

// FORWARD: the position of window position j on the candidate's contig
__host__ __device__ inline uint32_t edit_forward(uint32_t pos, uint32_t strand, const EditShape &s, uint32_t j)
{
    return strand ? pos + s.site_len - 1u - (s.win_start + j) : pos + s.win_start + j;
}

// the smallest FORWARD over the window - j = 0 on '+', j = win_len - 1 on '-': the window is [that, that + win_len) forward
__host__ __device__ inline uint32_t edit_window_first(uint32_t pos, uint32_t strand, const EditShape &s)
{
    return edit_forward(pos, strand, s, strand ? s.win_len - 1u : 0u);
}

// The targets as the kernels hold them: their global positions (contig offset + pos, 32-bit as contig_off is), strictly
// ascending.  A site lies inside one contig, so a target's global position inside a window is a target on the window's contig.
struct EditTargets {
    const uint32_t *gpos;
    uint32_t n;
};

// the first target at or behind global position g (t.n: none): a lower bound, log2(n) dependent loads
__host__ __device__ inline uint32_t edit_first_target(const EditTargets &t, uint32_t g)
{
    uint32_t lo = 0, hi = t.n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (t.gpos[mid] < g) lo = mid + 1u;
        else hi = mid;
    }
    return lo;
}

// the window position of target k when it lies in the window that starts at global position g0, win_len otherwise (the walk ends)
__host__ __device__ inline uint32_t edit_target_at(const EditTargets &t, uint32_t k, uint32_t g0, uint32_t strand, const EditShape &s)
{
    if (k >= t.n) return s.win_len;
    const uint32_t f = t.gpos[k] - g0;  // (gpos[k] >= g0: k is at or behind the lower bound)
    if (f >= s.win_len) return s.win_len;
    return strand ? s.win_len - 1u - f : f;
}

// HITS of a candidate with MASK `mask` whose window starts at global position g0: `first` = edit_first_target(t, g0); the
// walk takes at most win_len targets, because their positions are strictly ascending.
__host__ __device__ inline uint32_t edit_hits(uint32_t mask, uint32_t first, const EditTargets &t, uint32_t g0, uint32_t strand,
                                              const EditShape &s)
{
    uint32_t hits = 0;
    for (uint32_t k = first; k - first < s.win_len; ++k) {
        const uint32_t j = edit_target_at(t, k, g0, strand, s);
        if (j >= s.win_len) break;
        hits |= mask & (1u << j);
    }
    return hits;
}

// info of a pair: at | bystanders << 8
__host__ __device__ inline uint32_t edit_pair_info(uint32_t mask, uint32_t j) { return j | ((uint32_t)__builtin_popcount(mask) - 1u) << 8; }

// The FILTER rule: does a candidate of class cls with (mask, hits) pass?
__host__ __device__ inline bool edit_keep(uint32_t cls, uint32_t mask, uint32_t hits, uint32_t min_editable, uint32_t max_editable,
                                          bool have_targets)
{
    if (cls != kEffDefined) return false;
    const uint32_t e = (uint32_t)__builtin_popcount(mask);
    return e >= min_editable && e <= max_editable && (!have_targets || hits != 0u);
}

}  // namespace vsc
