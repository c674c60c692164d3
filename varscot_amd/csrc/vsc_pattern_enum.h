// vsc_pattern_enum.h - what the host code of vsc_guides_enumerate_pattern / vsc_pattern_guide_text (vsc_api.cpp) shares with
// the kernels at the end of vsc_pattern.hip: pattern guide discovery, vsc_guides_enumerate for any pattern.
//
// The two host helpers are plain inline functions that a stand-alone program can include without a device
// (tools/pattern_enum_check.cpp runs them under the host sanitizers):
//   pattern_target_ranges  the target intervals as sorted, disjoint ranges of site STARTS in global coordinates - the region
//                          test for an L-base site.  vsc_regions' class table is built for 23-base windows; this needs none.
//   pattern_guide_text     the letters of one code.
#pragma once

#include <algorithm>
#include <vector>

#include "vsc_pattern.h"

namespace vsc {

// site starts [lo, hi) in global positions (contig offset + position in the contig)
struct PatStartRange {
    uint32_t lo, hi;
};

// Per interval the starts p of the L-base sites that qualify:
//   VSC_REGION_OVERLAP  p < end and p + L > start   <=>  p in [start - L + 1, end)
//   VSC_REGION_INSIDE   start <= p and p + L <= end  <=>  p in [start, end - L]
// with end clipped to the contig first and every range clipped to the contig's positions; then the union.  A site across the
// seam of two abutting intervals is inside neither: their INSIDE ranges do not touch.  contig_off / contig_end: the genome's
// table in global positions.  VSC_ERR_INVALID as vsc_regions_build refuses.
inline int pattern_target_ranges(const uint32_t *contig_off, const uint32_t *contig_end, uint32_t n_contigs, const vsc_interval *iv,
                                 uint64_t n, uint32_t rule, uint32_t len, std::vector<PatStartRange> *out)
{
    out->clear();
    if (rule != VSC_REGION_OVERLAP && rule != VSC_REGION_INSIDE) return VSC_ERR_INVALID;
    if (len == 0 || (n && !iv)) return VSC_ERR_INVALID;
    for (uint64_t i = 0; i < n; ++i)
        if (iv[i].contig >= n_contigs || iv[i].start > iv[i].end || iv[i].reserved) return VSC_ERR_INVALID;
    for (uint64_t i = 0; i < n; ++i) {
        const uint32_t off = contig_off[iv[i].contig], clen = contig_end[iv[i].contig] - off;
        const uint32_t start = iv[i].start, end = std::min(iv[i].end, clen);
        if (start >= end) continue;  // empty (after clipping)
        uint32_t lo, hi;
        if (rule == VSC_REGION_OVERLAP) {
            lo = start >= len - 1u ? start - (len - 1u) : 0u;
            hi = end;
        } else {
            if (end - start < len) continue;  // no site fits
            lo = start;
            hi = end - len + 1u;
        }
        out->push_back(PatStartRange{off + lo, off + hi});  // (hi <= clen: inside the contig)
    }
    std::sort(out->begin(), out->end(), [](const PatStartRange &a, const PatStartRange &b) { return a.lo < b.lo || (a.lo == b.lo && a.hi < b.hi); });
    size_t kept = 0;
    for (size_t i = 0; i < out->size(); ++i) {
        if (kept && (*out)[i].lo <= (*out)[kept - 1].hi)
            (*out)[kept - 1].hi = std::max((*out)[kept - 1].hi, (*out)[i].hi);
        else
            (*out)[kept++] = (*out)[i];
    }
    out->resize(kept);
    return VSC_OK;
}

// is global start position p in the ranges?  (the device's lookup for one start, on the host: what the stand-alone check
// compares with the rule applied position by position)
inline bool pattern_ranges_contain(const std::vector<PatStartRange> &r, uint32_t p)
{
    size_t lo = 0, hi = r.size();  // -> the first range with hi > p
    while (lo < hi) {
        const size_t mid = (lo + hi) / 2;
        if (r[mid].hi <= p) lo = mid + 1; else hi = mid;
    }
    return lo < r.size() && r[lo].lo <= p;
}

// The letters of one code (hi plane << 32 | lo plane, bit j = read position j, A 00 C 01 G 10 T 11): out[0 .. len), no
// terminator.  Inside the protospacer [ps_start, ps_start + ps_len) the site's letter; outside it N (spell == 0: the query
// form, those positions are not compared by vsc_search_pattern) or the site's letter (spell == 1).
inline int pattern_guide_text(uint64_t code, uint32_t len, uint32_t ps_start, uint32_t ps_len, uint32_t spell, char *out)
{
    if (!out || len < kPatMinLen || len > kPatMaxLen || spell > 1u) return VSC_ERR_INVALID;
    if (ps_len == 0 || ps_start > len || ps_len > len - ps_start) return VSC_ERR_INVALID;
    const uint32_t hi = (uint32_t)(code >> 32), lo = (uint32_t)code;
    if (len < 32u && ((hi | lo) >> len)) return VSC_ERR_INVALID;  // bits from len on must be 0
    for (uint32_t j = 0; j < len; ++j) {
        const bool inside = j >= ps_start && j - ps_start < ps_len;
        out[j] = inside || spell ? "ACGT"[((hi >> j) & 1u) << 1 | ((lo >> j) & 1u)] : 'N';
    }
    return VSC_OK;
}

struct PatEnumArgs {
    const uint32_t *hi, *lo, *nm;  // device planes, as ScanArgs
    uint32_t first_pos;            // global position of bit 0 of element 0
    const uint32_t *work;          // [n_work] ascending tiles of the shard to visit; null: tile i is work item i
    uint32_t n_work;
    uint32_t len;                  // L
    uint32_t len_mask;             // the low L bits
    PatFront front[2];             // '+': the pattern; '-': its reverse complement, as a second forward pattern
    uint32_t keep_fwd, keep_rev;   // all ones / zero: the strand is wanted
    uint32_t filter;               // non-zero: a GC bound or a T-run limit is set (else no site is looked at one by one)
    uint32_t ps_fwd, ps_rev;       // the protospacer's bits in the L forward bits of a site, per strand
    uint32_t gc_min, gc_max;       // G / C among the protospacer bases (gc_max = its length: no upper bound)
    uint32_t max_t_run;            // 0: no limit
    const uint2 *ranges;           // [n_ranges] kTargets kernels: sorted, disjoint start ranges [x, y), global positions
    uint32_t n_ranges;
    const uint32_t *contig_off, *contig_end;
    uint32_t n_contigs;
    uint32_t *tile_count;          // [n_work] count pass: candidates kept per work item
    const unsigned long long *tile_off;  // [n_work + 1] write pass: candidates of all earlier work items
    unsigned long long n_out;      // write pass: tile_off[n_work], the length of the two arrays
    unsigned long long *codes;     // out: hi plane << 32 | lo plane in read orientation
    uint4 *loci;                   // out: vsc_locus {contig, pos, strand, 0}
};

hipError_t launch_pattern_enum(const PatEnumArgs &args, bool write, hipStream_t stream);

}  // namespace vsc
