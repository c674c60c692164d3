// vsc_enum.h - what the host code of vsc_guides_enumerate (vsc_api.cpp) shares with its kernels (vsc_enum.hip).  A header of
// its own, so that the structs of vsc_internal.h - and with them the other kernels' translation units - stay what they were.
// Also the label lookup (regions_locate) that vsc_regions.cpp runs on the host and locate_kernel on the device.
#pragma once

#include "vsc_internal.h"

namespace vsc {

struct EnumArgs {
    const uint32_t *hi, *lo, *nm;  // device planes, as ScanArgs
    uint32_t first_pos;            // global position of bit 0 of element 0
    const uint32_t *work;          // [n_work] ascending tiles of the shard to visit; null: tile i is work item i
    uint32_t n_work;
    PamMasks pam;                  // the guide's PAM
    uint32_t keep_fwd, keep_rev;   // all ones / zero: the strand is wanted
    uint32_t filter;               // non-zero: a GC bound or a T-run limit is set (else no window is looked at one by one)
    uint32_t gc_min, gc_max;       // G / C among the 20 protospacer bases (gc_max = 20: no upper bound)
    uint32_t max_t_run;            // 0: no limit
    RegionsView reg;               // kRegions kernels only
    const uint32_t *contig_off, *contig_end;
    uint32_t n_contigs;
    uint32_t *tile_count;          // [n_work] count pass: candidates kept per work item
    const unsigned long long *tile_off;  // [n_work + 1] write pass: candidates of all earlier work items
    unsigned long long *codes;     // out: vsc_pack_guide codes
    uint4 *loci;                   // out: vsc_locus {contig, pos, strand, 0}
};

hipError_t launch_enum(const EnumArgs &args, bool write, bool regions, hipStream_t stream);
hipError_t launch_enum_scan(const uint32_t *tile_count, uint32_t n, unsigned long long *tile_off, hipStream_t stream);

// ---- labels (vsc_regions_locate, vsc_hits_locate, vsc_guides_locate) ------------------------------------------
// The kept intervals a second time, ordered by (start ascending, end descending, input index descending): the multiset of
// starts is RegionsView::start[], so entry k of these arrays goes with start[k].  Of the entries before a bound on the start,
// the LAST one whose end passes the rule's test is the label: largest start, then smallest end, then lowest input index.
// up[k] = the nearest j < k with end[j] > end[k] (kLocateNone: there is none): when end[k] is too small so is the end of every
// entry between up[k] and k, so the walk may skip them.
constexpr uint32_t kLocateNone = 0xFFFFFFFFu;  // == VSC_REGION_NONE

struct LocateView {
    const uint32_t *end;    // [RegionsView::n] global, clipped
    const uint32_t *index;  // [n] position in the caller's iv[]
    const uint32_t *up;     // [n]
};

// The label of the window of `len` bases that starts at global position pos (len < VSC_READ_LEN: cut off by its contig's
// end, the host's vsc_regions_locate only): regions_search's count, then the walk.  != kLocateNone iff regions_search is true.
// Every index is checked against v.n before it is used, and up[] must decrease, so no table can send the walk astray.
__host__ __device__ inline uint32_t regions_locate(const RegionsView &v, const LocateView &l, uint32_t pos, uint32_t len)
{
    const bool inside = v.rule == VSC_REGION_INSIDE;
    const uint32_t bound = inside ? pos + 1u : pos + len;
    uint32_t lo = 0, hi = v.n;  // -> #{start < bound}
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (v.start[mid] < bound) lo = mid + 1; else hi = mid;
    }
    const uint32_t need = inside ? pos + (uint32_t)VSC_READ_LEN : pos + 1u;  // the interval's end must reach this
    uint32_t k = lo - 1u;  // (lo == 0: all ones, not < v.n)
    while (k < v.n) {
        if (l.end[k] >= need) return l.index[k];
        const uint32_t j = l.up[k];
        if (j >= k) break;
        k = j;
    }
    return kLocateNone;
}

// One label per 16-byte record: vsc_hit (contig, pos at words 1, 2) or vsc_locus (words 0, 1).
struct LocateArgs {
    RegionsView reg;               // start[] and the class table (end_max is not read)
    LocateView loc;
    const uint32_t *contig_off, *contig_len;  // [n_contigs] the table the regions were built for
    uint32_t n_contigs;
    const uint4 *records;          // [n]
    unsigned long long n;
    uint32_t *labels;              // [n] out
};

hipError_t launch_locate(const LocateArgs &args, bool hit_records, int n_cus, hipStream_t stream);

}  // namespace vsc
