// vsc_bulge_table.h - the table score of a bulged alignment and of a cut site (include/varscot_hip.h "TABLE /
// SCORE" of vsc_bulge_hits_table / vsc_sites_table) as what the host code (vsc_bulge_table_build, vsc_bulge_table_score)
// shares with the kernels of vsc_bulge_table.hip.  A header of its own, modelled on vsc_pattern_table.h; it builds on
// vsc_pattern_table.h (the paired part of the score) and vsc_pattern_bulge.h (the split point of a member of a site).
//
// bulge_table_score below IS the score of include/varscot_hip.h for one guide, one site in read orientation, one d and one
// split point; site_table_scores IS the member loop of a cut site over one fetched span.  The kernels call them for every
// record (the weights in LDS), the host functions call them too - one function, one order of the multiplications, the same
// bits.  Plain inline code that a stand-alone program can include without a device.
//
// The score belongs to the alignment the search reports: the SMALLEST split point that reaches NM.  It is not a maximum over
// the split points.
#pragma once

#include "vsc_pattern_bulge.h"
#include "vsc_pattern_table.h"
#include "vsc_sites.h"

namespace vsc {

// the flat weights: the pattern table's (pair, then pam), then dna[i][s] at n + i * 4 + s, then rna[i][g] at n + (ps_len + i)
// * 4 + g, n = pattern_table_weights(shape) - at the most 768 + 128 + 128 doubles, 8 KB
constexpr uint32_t kBulgeTableMaxWeights = kPatTableMaxWeights + 2u * kPatTableMaxLen * 4u;
constexpr uint32_t kBulgeTableRowWords = kPatTableRowWords;  // vsc_guide_table_row as 64-bit words
constexpr uint32_t kSiteScoreWords = 4;                      // vsc_site_score
constexpr uint32_t kSiteWords = 8;                           // vsc_site

__host__ __device__ inline uint32_t bulge_table_dna_at(const PatTableShape &sh) { return pattern_table_weights(sh); }
__host__ __device__ inline uint32_t bulge_table_rna_at(const PatTableShape &sh) { return pattern_table_weights(sh) + sh.ps_len * 4u; }
__host__ __device__ inline uint32_t bulge_table_weights(const PatTableShape &sh) { return pattern_table_weights(sh) + sh.ps_len * 8u; }

// Is w (bulge_table_weights(sh) doubles) a table the definition allows: a valid pattern table whose protospacer has room for
// a bulge of two (ps_len >= kPatBulgeMinProto), every dna and rna weight finite and in [0, 1] - the rows that no score reads
// (dna row 0, rna rows 0 and ps_len - 1) included?
inline bool bulge_table_valid(const PatTableShape &sh, const double *w)
{
    if (!pattern_table_valid(sh, w) || sh.ps_len < kPatBulgeMinProto) return false;
    for (uint32_t i = bulge_table_dna_at(sh); i < bulge_table_weights(sh); ++i)
        if (!(w[i] >= 0.0 && w[i] <= 1.0)) return false;
    return true;
}

// Is (d, i) an alignment the definition knows under this shape: d in {-2, -1, +1, +2}, a site of 16 .. 32 letters, and
// a + 1 <= i, i + gap <= e - 1 (gap = the unpaired guide positions of an RNA bulge)?
__host__ __device__ inline bool bulge_table_defined(const PatTableShape &sh, int d, uint32_t i)
{
    if (d == 0 || d < -2 || d > 2 || sh.ps_len < kPatBulgeMinProto) return false;
    const int m = (int)sh.len + d;
    if (m < (int)kPatTableMinLen || m > (int)kPatTableMaxLen) return false;
    const uint32_t a = sh.ps_start, e = sh.ps_start + sh.ps_len, gap = d < 0 ? (uint32_t)-d : 0u;
    return i >= a + 1u && i + gap <= e - 1u;
}

// The score of a guide (gh, gl, single: pattern_table_guide) against a site of L + d letters in READ orientation (sh_, sl_:
// bit j = the code of s[j]; the bits from L + d on may hold anything) with the split point i: the paired site q through
// pattern_table_score - the unpaired guide positions of an RNA bulge taken out of `single` - then the weights of the unpaired
// letters in ascending order.  An alignment outside the definition (bulge_table_defined) scores 0.0 and reads no weight.
__host__ __device__ inline double bulge_table_score(const double *w, const PatTableShape &shape, uint32_t gh, uint32_t gl, uint32_t single,
                                                    uint32_t sh_, uint32_t sl_, int d, uint32_t i)
{
    if (!bulge_table_defined(shape, d, i)) return 0.0;
    const uint32_t a = shape.ps_start, front = low_bits(i);
    if (d > 0) {
        const uint32_t b = (uint32_t)d;
        const uint32_t qh = (sh_ & front) | ((sh_ >> b) & ~front), ql = (sl_ & front) | ((sl_ >> b) & ~front);
        double x = pattern_table_score(w, shape, gh, gl, single, qh, ql);
        const double *dna = w + bulge_table_dna_at(shape) + (i - a) * 4u;
        for (uint32_t t = 0; t < b; ++t) x = x * dna[((sh_ >> (i + t)) & 1u) << 1 | ((sl_ >> (i + t)) & 1u)];
        return x;
    }
    const uint32_t b = (uint32_t)-d, behind = ~low_bits(i + b);
    const uint32_t qh = (sh_ & front) | ((sh_ << b) & behind), ql = (sl_ & front) | ((sl_ << b) & behind);
    double x = pattern_table_score(w, shape, gh, gl, single & (front | behind), qh, ql);
    const double *rna = w + bulge_table_rna_at(shape);
    for (uint32_t t = 0; t < b; ++t) {
        const uint32_t j = i + t;
        if ((single >> j) & 1u) x = x * rna[(j - a) * 4u + (((gh >> j) & 1u) << 1 | ((gl >> j) & 1u))];
    }
    return x;
}

// A guide as the scores read it: the words of pattern_table_guide and the IUPAC planes of pattern_planes(sets, L).
struct BulgeGuide {
    uint32_t gh, gl, single;
    PatPlanes planes;
};

__host__ __device__ inline BulgeGuide bulge_table_guide(const uint8_t *sets, uint32_t len)
{
    BulgeGuide g;
    pattern_table_guide(sets, len, &g.gh, &g.gl, &g.single);
    g.planes = pattern_planes(sets, len);
    return g;
}

// f of one alignment whose (d, i) the caller brings (a vsc_bulge_hit); d = 0 is not one
__host__ __device__ inline uint32_t bulge_table_fixed(const double *w, const PatTableShape &shape, const BulgeGuide &g, uint32_t sh_, uint32_t sl_,
                                                      int d, uint32_t i)
{
    return table_fixed(bulge_table_score(w, shape, g.gh, g.gl, g.single, sh_, sl_, d, i));
}

// (NM, split point, f) of the member d of a site whose L + d letters are (sh_, sl_), bits from L + d on zero: the plain
// compare and pattern_table_score for d = 0, pattern_bulge_align and bulge_table_score otherwise.  A member whose length
// leaves 16 .. 32 or whose protospacer has no room: f = 0, NM = 0, index = 0.
__host__ __device__ inline uint32_t bulge_table_member(const double *w, const PatTableShape &shape, const BulgeGuide &g, uint32_t sh_, uint32_t sl_,
                                                       int d, uint32_t *nm, uint32_t *index)
{
    *nm = 0;
    *index = 0;
    if (d == 0) {
        const uint32_t x = pattern_mismatch(sh_, sl_, g.planes);
#if defined(__HIP_DEVICE_COMPILE__)
        *nm = (uint32_t)__popc(x);
#else
        *nm = (uint32_t)__builtin_popcount(x);
#endif
        return table_fixed(pattern_table_score(w, shape, g.gh, g.gl, g.single, sh_, sl_));
    }
    if (!bulge_table_defined(shape, d, shape.ps_start + 1u)) return 0u;
    *nm = pattern_bulge_align(sh_, sl_, g.planes, shape.ps_start, shape.ps_start + shape.ps_len, d, index);
    return bulge_table_fixed(w, shape, g, sh_, sl_, d, *index);
}

// the letters a site's span holds: L + the largest d among the members (members: vsc_site.members; 0 when there is none)
__host__ __device__ inline uint32_t site_span_letters(uint32_t len, uint32_t members)
{
    for (int k = 4; k >= 0; --k)
        if (((members >> (5 * k)) & 31u) != kSiteAbsent) return (uint32_t)((int)len + k - 2);
    return 0;
}

struct SiteScores {
    uint32_t best, top, top_d;
    uint32_t best_nm;  // NM of the best alignment, recomputed: the row's positive_nm index
};

// The member loop of a cut site over ONE span: span_h / span_l = the n = site_span_letters letters in READ orientation (bit j
// = letter j, the bits from n on zero) that end at the anchor (at_start false) or begin there (at_start true).  Every present
// member d is the last / first L + d letters of it.  best = f of the member best_d (the record's best alignment), top = the
// largest f, top_d = d + 2 of the member that attains it - on equal f the one with the smaller site_rank.  false (and zeros)
// when the record names no member or its best alignment is not among them.
__host__ __device__ inline bool site_table_scores(const double *w, const PatTableShape &shape, const BulgeGuide &g, unsigned long long span_h,
                                                  unsigned long long span_l, uint32_t n, bool at_start, uint32_t members, int best_d,
                                                  SiteScores *out)
{
    *out = SiteScores{0u, 0u, 0u, 0u};
    if (n == 0 || best_d < -2 || best_d > 2 || ((members >> (5 * (best_d + 2))) & 31u) == kSiteAbsent) return false;
    bool any = false;
    uint32_t top_rank = 0;
    for (int k = 0; k < 5; ++k) {
        if (((members >> (5 * k)) & 31u) == kSiteAbsent) continue;
        const int d = k - 2;
        const uint32_t m = (uint32_t)((int)shape.len + d);  // <= n
        uint32_t sh_ = 0, sl_ = 0, nm = 0, index = 0, f = 0;
        if (m <= kPatTableMaxLen && m <= n) {
            const uint32_t skip = at_start ? 0u : n - m;
            sh_ = (uint32_t)(span_h >> skip) & low_bits(m);
            sl_ = (uint32_t)(span_l >> skip) & low_bits(m);
            f = bulge_table_member(w, shape, g, sh_, sl_, d, &nm, &index);
        }
        const uint32_t rank = site_rank(d, nm);
        if (d == best_d) {
            out->best = f;
            out->best_nm = nm;
        }
        if (!any || f > out->top || (f == out->top && rank < top_rank)) {
            out->top = f;
            out->top_d = (uint32_t)k;
            top_rank = rank;
            any = true;
        }
    }
    return true;
}

// the reverse complement of an n-letter span, n in 1..64: reverse the order, complement both planes
__host__ __device__ inline unsigned long long span_revcomp(unsigned long long p, uint32_t n)
{
    unsigned long long r = 0;
#if defined(__HIP_DEVICE_COMPILE__)
    r = __brevll(p);
#else
    for (uint32_t j = 0; j < 64u; ++j) r |= ((p >> j) & 1ull) << (63u - j);
#endif
    return ~r >> (64u - n);
}

// ---- the kernels' arguments (vsc_bulge_table.hip) -----------------------------------------------------------------------
// The planes as the genome object holds them, and what bounds a fetch: n_words = the words the genome was LOADED with (own
// words + halo words, vsc_genome::held_words; the loader pads the device planes with kPadWords more, so every index below
// n_words is inside the allocation).  A span of 34 letters at bit offset 31 touches three words; every word a span touches
// is checked against n_words.  A shard is loaded with one halo word behind its last own word: a site that starts in the last
// own word's bit 31 and is 34 letters long touches a word behind the halo and scores 0 ON THAT SHARD.
struct BulgePlanes {
    const uint32_t *hi, *lo;
    uint32_t first_pos;  // global position of bit 0 of word 0
    uint32_t n_words;
    const uint32_t *contig_off, *contig_end;
    uint32_t n_contigs;
};

struct BulgeTableArgs {
    BulgePlanes planes;
    PatTableShape shape;
    const double *weights;  // device: bulge_table_weights(shape) doubles
    const uint4 *guides;    // device, two per guide: (gh, gl, single, 0), then the planes (A, C, G, T)
    uint32_t n_guides;
    uint32_t n;             // records
    unsigned long long *rows;  // vsc_guide_table_row rows of all guides, zeroed once per call (null: not asked for)
    // bulge_table_kernel
    const uint4 *hits;      // vsc_bulge_hit
    uint32_t *fixed;        // f per record (null: rows only)
    // site_table_kernel
    const uint4 *sites;     // vsc_site, two uint4 each
    uint32_t anchor;        // vsc_site_params.anchor
    uint4 *scores;          // vsc_site_score per site
};

// The selection over scored sites: per guide the sites with top >= min_score, of those the first top_k (0: all) by top
// descending, then record order - in record order.  bounds[g] = the first site of guide g, bounds[n_guides] = n.
struct SiteSelectArgs {
    const uint4 *sites, *scores;
    uint32_t n, n_guides;
    uint32_t *bounds;  // [n_guides + 1]
    uint32_t top_k, min_score;
    uint4 *sel;        // per guide: (T, take, kept low, kept high), as pattern_select_kernel leaves it
    uint4 *out_sites, *out_scores;
    unsigned long long n_out;
};

hipError_t launch_bulge_table(const BulgeTableArgs &args, int n_cus, hipStream_t stream);
hipError_t launch_site_table(const BulgeTableArgs &args, int n_cus, hipStream_t stream);
hipError_t launch_site_bounds(const SiteSelectArgs &args, hipStream_t stream);
hipError_t launch_site_select(const SiteSelectArgs &args, hipStream_t stream);
hipError_t launch_site_select_walk(const SiteSelectArgs &args, hipStream_t stream);

}  // namespace vsc
