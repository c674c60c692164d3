// vsc_pattern_bulge.h - what the host code of vsc_search_pattern_bulges / vsc_pattern_bulge_align (vsc_api.cpp) shares with
// the kernels of vsc_pattern_bulge.hip: bulges under a pattern.  vsc_bulge.h's three functions for a site of
// L + d bases, a protospacer [a, e) and IUPAC guide planes, over vsc_pattern.h's compare.
//
// pattern_bulge_align below IS the definition of include/varscot_hip.h for one guide and one site in read orientation: the
// kernels call its three parts (masks, bound, walk) for every (queued site, guide) pair, vsc_pattern_bulge_align calls it on
// the host, and so does the stand-alone check of tools/.  Everything but the two launches is plain inline code that needs no
// device.
#pragma once

#include "vsc_bulge.h"
#include "vsc_pattern.h"

namespace vsc {

constexpr uint32_t kPatBulgeMinProto = 4;  // a + 1 <= i, i + b <= e - 1 with b = 2 needs e - a >= 4
constexpr uint32_t kPatBulgeQueue = kTileBases;  // queue entries of a window: a tile's candidates go through in windows of this many

// bits [0, n), n in 0..32
__host__ __device__ inline uint32_t low_bits(uint32_t n) { return n < 32u ? (1u << n) - 1u : ~0u; }

// The two pairings of a guide (planes g of pattern_planes(.., L): the bits from L on set) against a site of L + d bases in read
// orientation (planes sh, sl, bit j = s[j], the bits from L + d on zero):
//   x0 bit j = s[j] is not in G[j]: the pairing in front of the bulge;
//   x1 bit j = s[j + d] is not in G[j]: the pairing behind it.
// Which bits each can see: the planes' bits from L on make x0 and x1 zero there, whatever the site holds (d > 0: s[L .. L + d)
// in x0, the zeros that the shift brings in x1).  For an RNA bulge x0's bits [L + d, L) compare the zeros behind the site,
// read as A: no nm(i) takes them (it takes j < i <= e - 1 + d from x0), and in the bound they can only clear a bit.  x1
// shifted up by -d leaves bits [0, -d) without a base: `live` clears them.
__host__ __device__ inline void pattern_bulge_masks(uint32_t sh, uint32_t sl, const PatPlanes &g, int d, uint32_t *x0, uint32_t *x1)
{
    const uint32_t th = d > 0 ? sh >> d : sh << -d, tl = d > 0 ? sl >> d : sl << -d;
    const uint32_t live = d > 0 ? ~0u : ~0u << -d;
    *x0 = pattern_mismatch(sh, sl, g);
    *x1 = pattern_mismatch(th, tl, g) & live;
}

// positions that pair from the 5' end for every split point (j <= a) ... and from the 3' end for every one (j >= e - 1)
__host__ __device__ inline uint32_t pattern_bulge_fixed5(uint32_t a) { return low_bits(a + 1u); }
__host__ __device__ inline uint32_t pattern_bulge_fixed3(uint32_t e, uint32_t len) { return low_bits(len) & ~low_bits(e - 1u); }

// A lower bound of nm(i) for every i, as bulge_bound_mask: a position <= a counts where x0 has it, one >= e - 1 where x1 has
// it, one between them unless it is unpaired (an RNA bulge: -d of them) or matches in the pairing its side of the split
// uses - so at least where it differs in both.  The caller compares popc(bound mask) with budget + gap.  A guide's N positions
// are 0 in x0 and in x1: they are in neither fixed set's way.
__host__ __device__ inline uint32_t pattern_bulge_bound_mask(uint32_t x0, uint32_t x1, uint32_t fixed5, uint32_t fixed3)
{
    return (x0 | fixed3) & (x1 | fixed5);
}

// NM = min over the split point i of nm(i), *index = the smallest i that reaches it.
//   DNA (d > 0): nm(i) = #x0[0, i) + #x1[i, L),      i = a + 1 .. e - 1
//   RNA (d < 0): nm(i) = #x0[0, i) + #x1[i - d, L),  i = a + 1 .. e - 1 + d
// as a running sum: nm(i + 1) = nm(i) + x0[i] - x1[i + gap], gap = 0 (DNA) / -d (RNA).  (x1 holds no bit from L on.)
__host__ __device__ inline uint32_t pattern_bulge_walk(uint32_t x0, uint32_t x1, uint32_t a, uint32_t e, int d, uint32_t *index)
{
    const uint32_t gap = d > 0 ? 0u : (uint32_t)-d;
    const uint32_t first = a + 1u, last = e - 1u - gap;  // (first + gap <= 31: e <= 32)
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t nm = (uint32_t)__popc(x0 & low_bits(first)) + (uint32_t)__popc(x1 >> (first + gap));
#else
    uint32_t nm = (uint32_t)__builtin_popcount(x0 & low_bits(first)) + (uint32_t)__builtin_popcount(x1 >> (first + gap));
#endif
    uint32_t best = nm, at = first;
    for (uint32_t i = first; i < last; ++i) {
        nm += ((x0 >> i) & 1u) - ((x1 >> (i + gap)) & 1u);
        if (nm < best) {
            best = nm;
            at = i + 1u;
        }
    }
    *index = at;
    return best;
}

__host__ __device__ inline uint32_t pattern_bulge_align(uint32_t sh, uint32_t sl, const PatPlanes &g, uint32_t a, uint32_t e, int d,
                                                        uint32_t *index)
{
    uint32_t x0, x1;
    pattern_bulge_masks(sh, sl, g, d, &x0, &x1);
    return pattern_bulge_walk(x0, x1, a, e, d, index);
}

// The bulged pattern of class d: P[0..a) + N x (n + d) + P[e..L), L + d sets (condition 3 of the definition).
__host__ __device__ inline void pattern_bulged(const uint8_t *sets, uint32_t len, uint32_t a, uint32_t e, int d, uint8_t *out)
{
    uint32_t k = 0;
    for (uint32_t j = 0; j < a; ++j) out[k++] = sets[j];
    for (uint32_t j = 0; j < (uint32_t)((int)(e - a) + d); ++j) out[k++] = (uint8_t)kPatAny;
    for (uint32_t j = e; j < len; ++j) out[k++] = sets[j];
}

// What the definition refuses of (L, protospacer, dna_max, rna_max, pattern): nullptr when all is well, else the reason.
inline const char *pattern_bulge_refusal(const uint8_t *sets, uint32_t len, uint32_t a, uint32_t n, uint32_t dna_max, uint32_t rna_max)
{
    if (dna_max > 2u || rna_max > 2u || (dna_max == 0u && rna_max == 0u)) return "dna_max and rna_max must be 0..2 and not both 0";
    if (n < kPatBulgeMinProto || a > len || n > len - a) return "the protospacer must have at least 4 positions and lie inside the pattern";
    for (uint32_t j = a; j < a + n; ++j)
        if (sets[j] != kPatAny) return "the pattern must be N at every protospacer position";
    if (len + dna_max > kPatMaxLen) return "pattern length + dna_max must not exceed 32";
    if (len < kPatMinLen + rna_max) return "pattern length - rna_max must be at least 16";
    return nullptr;
}

struct PatBulgeArgs {
    const uint32_t *hi, *lo, *nm;  // device planes, as ScanArgs
    uint32_t first_pos;            // global position of bit 0 of element 0
    uint32_t n_tiles;
    uint32_t len;                  // L
    uint32_t proto_a, proto_e;     // the protospacer [a, e)
    uint32_t classes;              // bit k: class k (d = bulge_d_of_class(k)) is enabled
    // per class and strand the front end's table over L + d positions: '+' the bulged pattern, '-' its reverse complement as a
    // second forward pattern (the tables of a class that is not enabled are empty and never read)
    PatFront front[kBulgeClasses][2];
    // the round's guides, a uint4 each - the planes (A, C, G, T) in READ orientation, one table for both strands: the kernels
    // turn a '-' site into read orientation, once per queued site; padded with all-zero guides to kPatUnroll, plus kPatUnroll spare
    const uint4 *guides;
    uint32_t n_guides;             // guides of the round, <= kPatMaxBatch
    uint32_t guide_base;           // index of the round's first guide in the caller's array
    uint32_t max_mm;
    const uint32_t *contig_off, *contig_end;
    uint32_t n_contigs;
    // cell (guide r of the round, strand s, tile t) = (2 r + s) * n_tiles + t: ascending cells = the record order
    uint32_t *count;               // [2 * n_guides * n_tiles] count pass: hits per cell
    const uint32_t *chunk_sum;     // write pass: hits of chunk c of kPatChunk cells ...
    const unsigned long long *group_off;  // ... and hits of all cells before group g of kPatChunk chunks
    unsigned long long *sites;     // count pass: += candidates of the enabled classes, both strands
    uint4 *records;                // write pass: the round's vsc_bulge_hit records (null: rows only)
    unsigned long long n_records;  // ... and how many there are (the scan's total)
    uint32_t *rows;                // write pass: vsc_bulge_summary rows of ALL guides, zeroed once per call (null: records only)
};

// waves of either pass: each takes a run of consecutive tiles
hipError_t launch_pattern_bulge_count(const PatBulgeArgs &args, int n_cus, hipStream_t stream);
hipError_t launch_pattern_bulge_write(const PatBulgeArgs &args, int n_cus, hipStream_t stream);

}  // namespace vsc
