// vsc_pattern.h - what the host code of vsc_search_pattern / vsc_pattern_match (vsc_api.cpp) shares with the kernels of
// vsc_pattern.hip.  A header of its own, as vsc_bulge.h is.
//
// pattern_mismatch below IS the compare of include/varscot_hip.h for one guide and one site: the kernels call it for every
// (candidate, guide) pair, vsc_pattern_match calls it on the host - for the guide and, with the pattern's planes, for the
// pattern.  The host packing (letters to sets, sets to planes, reverse complements, the front end's table) is here as well:
// plain inline functions that a stand-alone program can include without a device.
#pragma once

#include "vsc_internal.h"
#include "vsc_pattern_table.h"

namespace vsc {

constexpr uint32_t kPatMinLen = 16;         // the N fold of the front end covers 16 positions in its first four steps
constexpr uint32_t kPatMaxLen = 32;         // one word of each plane: a site that starts at bit 31 ends at bit 62 of the pair
constexpr uint32_t kPatRowWords = VSC_MAX_MISMATCHES + 1;  // vsc_pattern_summary
constexpr uint32_t kPatRecordWords = 5;     // vsc_pattern_hit
constexpr uint32_t kPatDefaultBatch = 16;   // guides per count / scan / write round (guide_batch = 0)
constexpr uint32_t kPatMaxBatch = 64;       // ... and the most a round takes: lane g of the count pass counts guide g
constexpr uint32_t kPatChunk = 64;          // cells (guide, strand, tile) per entry of the offset table (= kBulgeChunk)
constexpr uint32_t kPatUnroll = 4;          // guides per scalar load of the count pass (64 bytes)
constexpr uint32_t kPatSlots = 4;           // queued sites a lane compares per step of the guide loop
constexpr uint32_t kPatAny = 15;            // the set of N

// A letter as its set of bases: bit 0 A, bit 1 C, bit 2 G, bit 3 T; 0 = not an IUPAC letter (U included).
__host__ __device__ inline uint32_t iupac_set(char c)
{
    switch (c >= 'a' && c <= 'z' ? c - 'a' + 'A' : c) {
    case 'A': return 1;
    case 'C': return 2;
    case 'G': return 4;
    case 'T': return 8;
    case 'R': return 1 | 4;
    case 'Y': return 2 | 8;
    case 'S': return 2 | 4;
    case 'W': return 1 | 8;
    case 'K': return 4 | 8;
    case 'M': return 1 | 2;
    case 'B': return 2 | 4 | 8;
    case 'D': return 1 | 4 | 8;
    case 'H': return 1 | 2 | 8;
    case 'V': return 1 | 2 | 4;
    case 'N': return kPatAny;
    default: return 0;
    }
}

// the set of the complemented bases: A <-> T, C <-> G = the four bits in reverse order
__host__ __device__ inline uint32_t iupac_comp(uint32_t s) { return (s & 1u) << 3 | (s & 2u) << 1 | (s & 4u) >> 1 | (s & 8u) >> 3; }

// Four planes of a string of sets: bit j of .x / .y / .z / .w = A / C / G / T is allowed at position j.
struct PatPlanes {
    uint32_t a, c, g, t;
};

// The planes of sets[0..len); the bits from len on are set in all four, so that whatever the genome holds behind the site
// counts as a match and the mismatch mask needs no length mask.
__host__ __device__ inline PatPlanes pattern_planes(const uint8_t *sets, uint32_t len)
{
    const uint32_t high = len < 32u ? ~0u << len : 0u;
    PatPlanes p{high, high, high, high};
    for (uint32_t j = 0; j < len; ++j) {
        p.a |= (uint32_t)(sets[j] & 1u) << j;
        p.c |= (uint32_t)((sets[j] >> 1) & 1u) << j;
        p.g |= (uint32_t)((sets[j] >> 2) & 1u) << j;
        p.t |= (uint32_t)((sets[j] >> 3) & 1u) << j;
    }
    return p;
}

// out[j] = comp(in[len - 1 - j]): the string that the forward genome must satisfy where the input is meant for the '-' strand
__host__ __device__ inline void pattern_revcomp(const uint8_t *in, uint32_t len, uint8_t *out)
{
    for (uint32_t j = 0; j < len; ++j) out[j] = (uint8_t)iupac_comp(in[len - 1u - j]);
}

// letters to sets; false at the first letter that is no IUPAC letter
__host__ __device__ inline bool pattern_sets(const char *text, uint32_t len, uint8_t *sets)
{
    for (uint32_t j = 0; j < len; ++j) {
        sets[j] = (uint8_t)iupac_set(text[j]);
        if (!sets[j]) return false;
    }
    return true;
}

// The compare: bit j of the result is set when the base (h, l) bit j (A 00, C 01, G 10, T 11) is not in the planes' set at j.
//   match = (~h & ~l & gA) | (~h & l & gC) | (h & ~l & gG) | (h & l & gT)  =  l ? (h ? gT : gC) : (h ? gG : gA)
// three v_bitop3_b32 on the device (two selects by h, one inverted select by l).
__host__ __device__ inline uint32_t pattern_mismatch(uint32_t h, uint32_t l, const PatPlanes &g)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t hi = __builtin_amdgcn_bitop3_b32(h, g.t, g.c, 0xCA);  // h ? gT : gC
    const uint32_t lo = __builtin_amdgcn_bitop3_b32(h, g.g, g.a, 0xCA);  // h ? gG : gA
    return __builtin_amdgcn_bitop3_b32(l, hi, lo, 0x35);                 // ~(l ? hi : lo)
#else
    const uint32_t hi = (h & g.t) | (~h & g.c), lo = (h & g.g) | (~h & g.a);
    return ~((l & hi) | (~l & lo));
#endif
}

// The front end's table of one strand: an entry per pattern position that is not N, j | set << 8.
struct PatFront {
    uint32_t n;
    uint32_t ent[kPatMaxLen];
};

__host__ __device__ inline void pattern_front(const uint8_t *sets, uint32_t len, PatFront *f)
{
    f->n = 0;
    for (uint32_t j = 0; j < kPatMaxLen; ++j) f->ent[j] = 0;
    for (uint32_t j = 0; j < len; ++j)
        if (sets[j] != kPatAny) f->ent[f->n++] = j | (uint32_t)sets[j] << 8;
}

struct PatternArgs {
    const uint32_t *hi, *lo, *nm;  // device planes, as ScanArgs
    uint32_t first_pos;            // global position of bit 0 of element 0
    uint32_t n_tiles;
    uint32_t len;                  // L
    PatFront front[2];             // '+': the pattern; '-': its reverse complement, as a second forward pattern
    // the round's guides, a uint4 each - the planes (A, C, G, T) - in two tables guide_stride apart: the guides for '+', their
    // reverse complements for '-'; each padded with all-zero guides to kPatUnroll, plus kPatUnroll spare (the loop fetches ahead)
    const uint4 *guides;
    uint32_t guide_stride;
    uint32_t n_guides;             // guides of the round, <= kPatMaxBatch
    uint32_t guide_base;           // index of the round's first guide in the caller's array
    uint32_t max_mm;
    const uint32_t *contig_off, *contig_end;
    uint32_t n_contigs;
    // cell (guide r of the round, strand s, tile t) = (2 r + s) * n_tiles + t: ascending cells = the record order
    uint32_t *count;               // [2 * n_guides * n_tiles] count pass: hits per cell
    const uint32_t *chunk_sum;     // write pass: hits of chunk c of kPatChunk cells ...
    const unsigned long long *group_off;  // ... and hits of all cells before group g of kPatChunk chunks
    unsigned long long *sites;     // count pass: += candidates (sites that satisfy the pattern and hold no N, both strands)
    uint32_t *records;             // write pass: the round's vsc_pattern_hit records, five words each (null: rows only)
    unsigned long long n_records;  // ... and how many there are (the scan's total)
    uint32_t *rows;                // write pass: vsc_pattern_summary rows of ALL guides, zeroed once per call (null: records only)
};

// What the scored write pass (vsc_search_pattern_table) takes beside PatternArgs.  PatternArgs::guides then holds
// a third table, 2 * guide_stride in: per guide (gh, gl, single, 0), its read-orientation planes as pattern_table_guide makes them.
constexpr uint32_t kPatTableRowWords = 12;  // vsc_guide_table_row as 64-bit words: score_sum, positive, positive_nm[9], reserved
struct PatScoreArgs {
    PatTableShape shape;
    const double *weights;           // device: pattern_table_weights(shape) doubles
    uint32_t *fixed;                 // f per record, parallel to PatternArgs::records (null when those are)
    unsigned long long *table_rows;  // vsc_guide_table_row rows of ALL guides, zeroed once per call (null: not asked for)
};

// The selection stage behind the scored write pass: per guide of the round the hits with f >= min_score, of those the first
// top_k (0: all) by f descending, then record order - in record order.
struct PatSelectArgs {
    const uint32_t *count, *chunk_sum;     // the round's cells, as the write pass read them: guide r's records are those of
    const unsigned long long *group_off;   // cells [2 r * n_tiles, 2 (r + 1) * n_tiles) - one contiguous segment
    uint32_t n_tiles, n_guides;
    unsigned long long n_records;          // the round's records before the selection
    const uint32_t *records, *fixed;       // ... and where the write pass left them
    uint32_t top_k, min_score;
    uint4 *sel;                            // per guide of the round: (T, take, kept low, kept high)
    uint32_t *out_records, *out_fixed;     // walk: the round's survivors
    unsigned long long n_out;
};

// waves of either pass: each takes a run of consecutive tiles
hipError_t launch_pattern_count(const PatternArgs &args, int n_cus, hipStream_t stream);
hipError_t launch_pattern_write(const PatternArgs &args, int n_cus, hipStream_t stream);
hipError_t launch_pattern_write_scored(const PatternArgs &args, const PatScoreArgs &score, int n_cus, hipStream_t stream);
// one workgroup per guide of the round: the threshold (T, take, kept) of every guide, then the walk that keeps the survivors
hipError_t launch_pattern_select(const PatSelectArgs &args, hipStream_t stream);
hipError_t launch_pattern_select_walk(const PatSelectArgs &args, hipStream_t stream);

}  // namespace vsc
