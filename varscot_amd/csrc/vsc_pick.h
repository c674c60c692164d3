// vsc_pick.h - the per-target pick with spacing (include/varscot_hip.h "SHAPE / CANDIDATE / CUT COORDINATE /
// ELIGIBLE / BEFORE / CONFLICT / PICK / OUTPUT / TARGETS") as what the host code (vsc_pick_host) shares with the kernels of
// vsc_pick.hip.  A header of its own, as vsc_mh.h is: plain inline functions that a stand-alone program can include without a
// device.  The class of a candidate, its cut coordinate, the order of two candidates and the conflict of two candidates are
// each ONE function here; the kernels, the host call and tools/pick_check.cpp all call these.  pick_host at the end is the
// definition as straightforward host code: what vsc_pick_host runs.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <vector>

#if !defined(__HIPCC__) && !defined(__host__)  // (a plain C++ compiler)
#define __host__
#define __device__
#endif

namespace vsc {

constexpr uint32_t kPickNone = 0xFFFFFFFFu;  // == VSC_PICK_NONE == VSC_REGION_NONE
constexpr uint32_t kPickMinSite = 16, kPickMaxSite = 32, kPickMaxK = 32;
constexpr uint64_t kPickMaxCandidates = 0xFFFFFFFEull;

// the classes of a candidate, in the order in which they are tested
enum PickClass : uint32_t { kPickEligible = 0, kPickInvalid = 1, kPickNoTarget = 2, kPickBadTarget = 3, kPickBelowMinKey = 4, kPickClasses = 5 };

struct PickShape {
    uint32_t site_len, cut, k, spacing;
    uint64_t min_key;
};

// Is s a shape the definition allows?  site_len 16 .. 32, cut 0 .. site_len, k 1 .. 32; any spacing, any min_key.
__host__ __device__ inline bool pick_shape_valid(const PickShape &s)
{
    return s.site_len >= kPickMinSite && s.site_len <= kPickMaxSite && s.cut <= s.site_len && s.k >= 1u && s.k <= kPickMaxK;
}

// x = p + cut on '+', p + site_len - cut on '-' (the centre of vsc_mh's context).  64-bit: no sum can wrap.
__host__ __device__ inline uint64_t pick_cut_coordinate(const PickShape &s, uint32_t pos, uint32_t strand)
{
    return (uint64_t)pos + (uint64_t)(strand ? s.site_len - s.cut : s.cut);
}

// The class of candidate (contig, pos, strand) with its target and key; contig_len is the length of its contig, looked up by
// the caller only when contig < n_contigs (pass 0 otherwise).  The order of the tests is the order of the definition.
__host__ __device__ inline uint32_t pick_class(const PickShape &s, uint32_t n_contigs, uint32_t contig, uint32_t contig_len, uint32_t pos,
                                               uint32_t strand, uint32_t target, uint32_t n_targets, uint64_t key)
{
    if (contig >= n_contigs || strand > 1u) return kPickInvalid;
    if (pos > contig_len || contig_len - pos < s.site_len) return kPickInvalid;  // pos + site_len <= len, without the overflow
    if (target == kPickNone) return kPickNoTarget;
    if (target >= n_targets) return kPickBadTarget;
    if (key < s.min_key) return kPickBelowMinKey;
    return kPickEligible;
}

// a before b  <=>  key[a] > key[b], or key[a] == key[b] and a < b: a total order over candidates of distinct indices
__host__ __device__ inline bool pick_before(uint64_t key_a, uint32_t a, uint64_t key_b, uint32_t b)
{
    return key_a > key_b || (key_a == key_b && a < b);
}

// Do two candidates of one target conflict?  Same contig and |x_a - x_b| < spacing in 64-bit arithmetic; spacing 0: never.
__host__ __device__ inline bool pick_conflict(uint32_t spacing, uint32_t contig_a, uint64_t x_a, uint32_t contig_b, uint64_t x_b)
{
    if (contig_a != contig_b) return false;
    const uint64_t d = x_a > x_b ? x_a - x_b : x_b - x_a;
    return d < (uint64_t)spacing;
}

// stats[] of a call: the classes in the order of PickClass, then the targets with a pick, the targets that end short of k
// although eligible candidates were left, and the picks
enum { kPickStatTargets = kPickClasses, kPickStatShort, kPickStatPicks, kPickStats };

struct PickLocus {
    uint32_t contig, pos, strand, reserved;  // vsc_locus
};

inline void pick_outputs_empty(const PickShape &s, uint64_t n, uint32_t n_targets, uint32_t *picks, uint32_t *counts, uint32_t *rank)
{
    if (picks) std::fill(picks, picks + (size_t)n_targets * s.k, kPickNone);
    if (counts) std::fill(counts, counts + n_targets, 0u);
    if (rank) std::fill(rank, rank + n, kPickNone);
}

// The definition as host code (vsc_pick_host): the class of every candidate, the eligible ones bucketed by target (a counting
// sort: input order inside a bucket), every bucket ordered under BEFORE and walked - a candidate is taken iff it conflicts with
// no pick so far, which is the PICK loop's "first under BEFORE among those that conflict with no picked one", round by round.
// loci, target, key: n entries; picks: n_targets * k; counts: n_targets; rank: n or null; stats: kPickStats, added into.
inline void pick_host(const PickShape &s, const uint32_t *contig_len, uint32_t n_contigs, const PickLocus *loci, uint64_t n, const uint32_t *target,
                      const uint64_t *key, uint32_t n_targets, uint32_t *picks, uint32_t *counts, uint32_t *rank, uint64_t *stats)
{
    pick_outputs_empty(s, n, n_targets, picks, counts, rank);
    std::vector<uint32_t> tg((size_t)n, kPickNone);
    std::vector<uint64_t> off((size_t)n_targets + 1, 0);
    uint64_t eligible = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const PickLocus &l = loci[i];
        const uint32_t len = l.contig < n_contigs ? contig_len[l.contig] : 0u;
        const uint32_t cls = pick_class(s, n_contigs, l.contig, len, l.pos, l.strand, target[i], n_targets, key[i]);
        ++stats[cls];
        if (cls == kPickEligible) {
            tg[i] = target[i];
            ++off[(size_t)target[i] + 1];
            ++eligible;
        }
    }
    for (uint32_t t = 0; t < n_targets; ++t) off[(size_t)t + 1] += off[t];
    std::vector<uint32_t> seg((size_t)eligible);
    {
        std::vector<uint64_t> at(off.begin(), off.end() - 1);
        for (uint64_t i = 0; i < n; ++i)
            if (tg[i] != kPickNone) seg[at[tg[i]]++] = (uint32_t)i;
    }
    for (uint32_t t = 0; t < n_targets; ++t) {
        uint32_t *const first = seg.data() + off[t], *const last = seg.data() + off[(size_t)t + 1];
        std::sort(first, last, [&](uint32_t a, uint32_t b) { return pick_before(key[a], a, key[b], b); });
        uint32_t *const out = picks + (size_t)t * s.k;
        uint32_t got = 0;
        for (const uint32_t *p = first; p != last && got < s.k; ++p) {
            const uint64_t x = pick_cut_coordinate(s, loci[*p].pos, loci[*p].strand);
            bool open = true;
            for (uint32_t r = 0; r < got && open; ++r)
                open = !pick_conflict(s.spacing, loci[*p].contig, x, loci[out[r]].contig, pick_cut_coordinate(s, loci[out[r]].pos, loci[out[r]].strand));
            if (!open) continue;
            if (rank) rank[*p] = got;
            out[got++] = *p;
        }
        counts[t] = got;
        stats[kPickStatTargets] += got ? 1u : 0u;
        stats[kPickStatShort] += got < s.k && (uint64_t)(last - first) > got ? 1u : 0u;
        stats[kPickStatPicks] += got;
    }
}

}  // namespace vsc
