// vsc_sites.h - what the host code of vsc_hits_sites / vsc_sites_collapse (vsc_api.cpp) shares with the kernels of
// vsc_sites.hip: the readers of the three record kinds, the key order, the anchor, the better-than rank, the
// members word and the gather of one alignment's site.  One __host__ __device__ header, as vsc_bulge.h is: the host
// function and the kernels run the very same gather.
#pragma once

#include "vsc_internal.h"

namespace vsc {

constexpr uint32_t kSiteAbsent = 31;         // a members field without a member
constexpr uint32_t kSiteNoMembers = 0x1FFFFFFu;  // five absent fields
constexpr uint32_t kSiteRowWords = 3 + 3 * (VSC_MAX_MISMATCHES + 1);  // vsc_site_summary
constexpr uint32_t kSiteRowSites = 0, kSiteRowAlignments = 1, kSiteRowBulgeOnly = 2, kSiteRowCount = 3;
constexpr uint32_t kSiteTile = 64;           // records per tile: one per lane, one ballot word
// records a walk visits at most on either side: siblings lie within +-4 positions, at most four bulged records per position
constexpr uint32_t kSiteWalk = 20;

enum SiteList : int { kSiteHit = 0, kSitePattern = 1, kSiteBulge = 2 };  // vsc_hit, vsc_pattern_hit, vsc_bulge_hit

// An alignment, whatever record it came from.  pos is signed and wide: the key a lane looks for may lie in front of the contig
// (pos - 2 at pos = 1), and such a key compares as any other.
struct SiteAln {
    uint32_t guide, strand, contig;
    long long pos;
    int d;
    uint32_t nm, index;  // index: the split point of a bulged record, 0 for a plain one
};

template <int kList> __host__ __device__ inline SiteAln site_load(const void *records, uint32_t i)
{
    SiteAln x;
    if (kList == kSitePattern) {
        const uint32_t *r = (const uint32_t *)records + (size_t)i * 5u;
        const uint32_t info = r[3];
        x.guide = r[0];
        x.contig = r[1];
        x.pos = r[2];
        x.strand = info >> 31;
        x.d = 0;
        x.nm = info & 31u;
        x.index = 0;
    } else {
        const uint4 r = ((const uint4 *)records)[i];
        x.guide = r.x;
        x.contig = r.y;
        x.pos = r.z;
        x.strand = r.w >> 31;
        if (kList == kSiteBulge) {
            const int size = (int)((r.w >> 10) & 3u);
            x.d = ((r.w >> 12) & 1u) ? -size : size;
            x.nm = r.w & 31u;
            x.index = (r.w >> 5) & 31u;
        } else {
            x.d = 0;
            x.nm = (r.w >> 23) & 31u;
            x.index = 0;
        }
    }
    return x;
}

__host__ __device__ inline bool site_same_run(const SiteAln &x, const SiteAln &y)
{
    return x.guide == y.guide && x.strand == y.strand && x.contig == y.contig;
}

// ascending (guide, strand, contig, pos, d): the order of the inputs and of the output
__host__ __device__ inline bool site_key_less(const SiteAln &x, const SiteAln &y)
{
    if (x.guide != y.guide) return x.guide < y.guide;
    if (x.strand != y.strand) return x.strand < y.strand;
    if (x.contig != y.contig) return x.contig < y.contig;
    if (x.pos != y.pos) return x.pos < y.pos;
    return x.d < y.d;
}

// #{records with a key below `key`}
template <int kList> __host__ __device__ inline uint32_t site_lower_bound(const void *records, uint32_t n, const SiteAln &key)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (site_key_less(site_load<kList>(records, mid), key)) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the strands on which the anchor is the site's start: its members share pos there
__host__ __device__ inline bool site_anchor_at_start(uint32_t anchor, uint32_t strand) { return (anchor == 0u) == (strand == 1u); }

__host__ __device__ inline long long site_anchor(const SiteAln &x, uint32_t len, uint32_t anchor)
{
    return site_anchor_at_start(anchor, x.strand) ? x.pos : x.pos + (long long)len + x.d;
}

// The order inside a site as one number: (NM + |d|, |d|, DNA before RNA).  Distinct d give distinct ranks.
__host__ __device__ inline uint32_t site_rank(int d, uint32_t nm)
{
    const uint32_t size = (uint32_t)(d < 0 ? -d : d);
    return (nm + size) << 3 | size << 1 | (d < 0 ? 1u : 0u);
}

struct SiteView {
    uint32_t members;  // bits 5k .. 5k+4, k = d + 2: NM, kSiteAbsent = no member (the count is not in yet)
    uint32_t best;     // the smallest site_rank among the members
};

__host__ __device__ inline void site_add(SiteView &v, const SiteAln &y)
{
    if (y.d < -2 || y.d > 2) return;  // (a size of 3: no record of a search)
    const uint32_t at = 5u * (uint32_t)(y.d + 2);
    v.members = (v.members & ~(31u << at)) | (y.nm << at);
    const uint32_t r = site_rank(y.d, y.nm);
    v.best = r < v.best ? r : v.best;
}

// vsc_site.members: the fields and, in bits 25..27, how many of them hold a member
__host__ __device__ inline uint32_t site_members_word(uint32_t fields)
{
    uint32_t n = 0;
    for (uint32_t k = 0; k < 5u; ++k) n += ((fields >> (5u * k)) & 31u) != kSiteAbsent;
    return fields | n << 25;
}

// The site of alignment x = record i of the bulged list (in_bulged) or of the plain list: its own list by a bounded walk
// (the plain list holds one record per site: nothing to walk), the other list by one lower bound.  Every index is checked
// against its list's length; the first and the last record, a neighbour of another guide, strand or contig and a sibling
// that would start in front of the contig all fall out of the comparisons.
template <int kPlain>
__host__ __device__ inline SiteView site_gather(const void *plain, uint32_t n_plain, const void *bulged, uint32_t n_bulged, bool in_bulged,
                                                uint32_t i, const SiteAln &x, uint32_t len, uint32_t anchor)
{
    SiteView v{kSiteNoMembers, ~0u};
    site_add(v, x);
    const long long a = site_anchor(x, len, anchor);
    if (in_bulged) {
        for (uint32_t k = 1; k <= kSiteWalk && k <= i; ++k) {
            const SiteAln y = site_load<kSiteBulge>(bulged, i - k);
            if (!site_same_run(x, y) || y.pos + 4 < x.pos) break;
            if (y.d != x.d && site_anchor(y, len, anchor) == a) site_add(v, y);
        }
        for (uint32_t k = 1; k <= kSiteWalk && k < n_bulged - i; ++k) {
            const SiteAln y = site_load<kSiteBulge>(bulged, i + k);
            if (!site_same_run(x, y) || y.pos > x.pos + 4) break;
            if (y.d != x.d && site_anchor(y, len, anchor) == a) site_add(v, y);
        }
        SiteAln key = x;  // the plain member: d = 0 at the same anchor
        key.d = 0;
        key.pos = site_anchor_at_start(anchor, x.strand) ? x.pos : x.pos + x.d;
        const uint32_t j = site_lower_bound<kPlain>(plain, n_plain, key);
        if (j < n_plain) {
            const SiteAln y = site_load<kPlain>(plain, j);
            if (site_same_run(x, y) && y.pos == key.pos) site_add(v, y);
        }
    } else {
        SiteAln key = x;  // the first bulged record that can be a sibling
        key.pos = x.pos - 2;
        key.d = -2;
        uint32_t j = site_lower_bound<kSiteBulge>(bulged, n_bulged, key);
        for (uint32_t k = 0; k < kSiteWalk && j < n_bulged; ++k, ++j) {
            const SiteAln y = site_load<kSiteBulge>(bulged, j);
            if (!site_same_run(x, y) || y.pos > x.pos + 2) break;
            if (y.d != 0 && site_anchor(y, len, anchor) == a) site_add(v, y);
        }
    }
    return v;
}

// #{records of the OTHER list with a key below x's}: what a best alignment's rank adds to the survivors in front of it
template <int kPlain>
__host__ __device__ inline uint32_t site_other_below(const void *plain, uint32_t n_plain, const void *bulged, uint32_t n_bulged, bool in_bulged,
                                                     const SiteAln &x)
{
    return in_bulged ? site_lower_bound<kPlain>(plain, n_plain, x) : site_lower_bound<kSiteBulge>(bulged, n_bulged, x);
}

// the eight words of a vsc_site whose best alignment is x = record `index` of its list
__host__ __device__ inline void site_record(const SiteAln &x, uint32_t index, const SiteView &v, uint32_t len, uint32_t anchor, uint32_t *out)
{
    const uint32_t size = (uint32_t)(x.d < 0 ? -x.d : x.d);
    out[0] = x.guide;
    out[1] = x.contig;
    out[2] = (uint32_t)x.pos;
    out[3] = x.strand << 31 | (x.d < 0 ? 1u : 0u) << 12 | size << 10 | x.index << 5 | x.nm;
    out[4] = (uint32_t)site_anchor(x, len, anchor);
    out[5] = site_members_word(v.members);
    out[6] = index;
    out[7] = 0;
}

// the words of the guide's row that a site with best alignment x adds one to: sites, count[|d|][NM] and - flagged - bulge_only
__host__ __device__ inline uint32_t site_row_count_word(const SiteAln &x)
{
    const uint32_t size = (uint32_t)(x.d < 0 ? -x.d : x.d);
    const uint32_t nm = x.nm < (uint32_t)VSC_MAX_MISMATCHES ? x.nm : (uint32_t)VSC_MAX_MISMATCHES;
    return kSiteRowCount + size * (VSC_MAX_MISMATCHES + 1) + nm;
}
__host__ __device__ inline bool site_bulge_only(const SiteView &v) { return ((v.members >> 10) & 31u) == kSiteAbsent; }

struct SiteArgs {
    const void *plain;   // vsc_hit or vsc_pattern_hit records (the launch's kind)
    const void *bulged;  // vsc_bulge_hit records
    uint32_t n_plain, n_bulged;
    uint32_t tiles_plain, tiles_bulged;  // tiles of kSiteTile records: [plain tiles | bulged tiles]
    uint32_t n_guides, len, anchor;
    unsigned long long *ballot;          // [tiles] flag pass: the best alignments of the tile
    uint32_t *tile_count;                // [tiles] ... and how many they are
    const unsigned long long *tile_off;  // [tiles + 1] their exclusive scan
    uint32_t *invalid;                   // flag pass: set when a record's guide is not below n_guides
    uint32_t *rows;                      // vsc_site_summary rows, zeroed once per call (null: records only)
    uint4 *sites;                        // write pass: the vsc_site records, two uint4 each (null: rows only)
    unsigned long long n_sites;          // ... and how many there are (the scan's total)
};

hipError_t launch_site_flag(const SiteArgs &args, int plain_kind, int n_cus, hipStream_t stream);
hipError_t launch_site_write(const SiteArgs &args, int plain_kind, int n_cus, hipStream_t stream);

}  // namespace vsc
