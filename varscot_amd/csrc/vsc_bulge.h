// vsc_bulge.h - what the host code of vsc_search_bulges / vsc_bulge_align (vsc_api.cpp) shares with the kernels of
// vsc_bulge.hip.  A header of its own, as vsc_enum.h is: the structs of vsc_internal.h stay what they were.
//
// bulge_align below IS the definition of include/varscot_hip.h for one read and one site in read orientation: the kernels
// call it for every candidate that passes their popcount bound, vsc_bulge_align calls it on the host.
#pragma once

#include "vsc_internal.h"

namespace vsc {

constexpr uint32_t kBulgeClasses = 4;        // ascending d: RNA 2, RNA 1, DNA 1, DNA 2
constexpr uint32_t kBulgeRowWords = kBulgeClasses * (VSC_MAX_MISMATCHES + 1);  // vsc_bulge_summary
constexpr uint32_t kBulgeDefaultBatch = 16;  // reads per count / scan / write round (guide_batch = 0)
constexpr uint32_t kBulgeMaxBatch = 64;      // ... and the most a round takes: two LDS counters per read and wave
constexpr uint32_t kBulgeUnroll = 4;         // reads per step of the count pass: the table is padded to it, plus four spare reads
constexpr uint32_t kBulgeChunk = 64;         // cells (read, strand, tile) per entry of the offset table: one load per lane
constexpr int kBulgeMaxIndex = 19;           // the split point i runs over 1 .. 19 (DNA), 1 .. 19 - size (RNA)
constexpr uint32_t kBulgeFixed5 = 0x1u;      // read positions that pair from the 5' end for every i (j < 1) ...
constexpr uint32_t kBulgeFixed3 = 0x780000u; // ... and from the PAM end for every i (j >= 19)

// class k = 0..3 <-> d = -2, -1, +1, +2
__host__ __device__ inline int bulge_d_of_class(uint32_t k) { return k < 2 ? (int)k - 2 : (int)k - 1; }
__host__ __device__ inline uint32_t bulge_class_of_d(int d) { return d < 0 ? (uint32_t)(d + 2) : (uint32_t)(d + 1); }

// The mismatch masks of a read (planes rh, rl) against a site of 23 + d bases in read orientation (planes sh, sl, bit j =
// s[j]): x0 = read position j against s[j], the pairing in front of the bulge; x1 = against s[j + d], the pairing behind
// it (23 bits each; for an RNA bulge the positions j < -d of x1 pair with nothing and are 0).
__host__ __device__ inline void bulge_masks(uint32_t rh, uint32_t rl, uint32_t sh, uint32_t sl, int d, uint32_t *x0, uint32_t *x1)
{
    const uint32_t th = d > 0 ? sh >> d : sh << -d, tl = d > 0 ? sl >> d : sl << -d;
    const uint32_t live = d > 0 ? kMask23 : kMask23 & ~((1u << -d) - 1u);
    *x0 = ((rh ^ sh) | (rl ^ sl)) & kMask23;
    *x1 = ((rh ^ th) | (rl ^ tl)) & live;
}

// A lower bound of nm(i) for every i: position 0 always counts in x0, positions 19..22 in x1, a position between them
// counts unless it is unpaired (an RNA bulge: -d of them) or matches in the pairing its side of the split uses - so at least
// where it differs in both.  The caller compares popc(bound mask) with budget + gap.
__host__ __device__ inline uint32_t bulge_bound_mask(uint32_t x0, uint32_t x1) { return (x0 | kBulgeFixed3) & (x1 | kBulgeFixed5); }

// NM = min over the split point i of nm(i), *index = the smallest i that reaches it.
//   DNA (d > 0): nm(i) = #x0[0, i) + #x1[i, 23),      i = 1 .. 19
//   RNA (d < 0): nm(i) = #x0[0, i) + #x1[i - d, 23),  i = 1 .. 19 + d
// as a running sum: nm(i + 1) = nm(i) + x0[i] - x1[i + gap], gap = 0 (DNA) / -d (RNA).
__host__ __device__ inline uint32_t bulge_walk(uint32_t x0, uint32_t x1, int d, uint32_t *index)
{
    const int gap = d > 0 ? 0 : -d;
    const int last = kBulgeMaxIndex - gap;
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t nm = (x0 & 1u) + (uint32_t)__popc(x1 >> (1 + gap));
#else
    uint32_t nm = (x0 & 1u) + (uint32_t)__builtin_popcount(x1 >> (1 + gap));
#endif
    uint32_t best = nm, at = 1;
    for (int i = 1; i < last; ++i) {
        nm += ((x0 >> i) & 1u) - ((x1 >> (i + gap)) & 1u);
        if (nm < best) {
            best = nm;
            at = (uint32_t)(i + 1);
        }
    }
    *index = at;
    return best;
}

__host__ __device__ inline uint32_t bulge_align(uint32_t rh, uint32_t rl, uint32_t sh, uint32_t sl, int d, uint32_t *index)
{
    uint32_t x0, x1;
    bulge_masks(rh, rl, sh, sl, d, &x0, &x1);
    return bulge_walk(x0, x1, d, index);
}

__host__ __device__ inline uint32_t bulge_info(uint32_t strand, int d, uint32_t index, uint32_t nm)
{
    return strand << 31 | (d < 0 ? 1u : 0u) << 12 | (uint32_t)(d < 0 ? -d : d) << 10 | index << 5 | nm;
}

struct BulgeArgs {
    const uint32_t *hi, *lo, *nm;  // device planes, as ScanArgs
    uint32_t first_pos;            // global position of bit 0 of element 0
    uint32_t n_tiles;
    const uint4 *guides;           // the round's reads, two per uint4: (hi0, lo0, hi1, lo1); padded to kBulgeUnroll reads + four more
    uint32_t n_guides;             // reads of the round, <= kBulgeMaxBatch
    uint32_t guide_base;           // index of the round's first read in the caller's array
    uint32_t max_mm;
    uint32_t n_pam;
    PamMasks pam[3];               // GG, GA (+ -P)
    uint32_t dna_max, rna_max;
    const uint32_t *contig_off, *contig_end;
    uint32_t n_contigs;
    // cell (read r of the round, strand s, tile t) = (2 r + s) * n_tiles + t: ascending cells = the record order
    uint32_t *count;               // [2 * n_guides * n_tiles] count pass: hits per cell
    const unsigned long long *chunk_off;  // write pass: hits of all cells before chunk c of kBulgeChunk cells
    unsigned long long *sites;     // count pass: += candidates (PAM-valid, N-free sites of the enabled classes)
    uint4 *records;                // write pass: the round's vsc_bulge_hit records (null: rows only)
    unsigned long long n_records;  // ... and how many there are (the scan's total)
    uint32_t *rows;                // write pass: vsc_bulge_summary rows of ALL reads, zeroed once per call (null: records only)
};

// waves of either pass: each takes a run of consecutive tiles
hipError_t launch_bulge_count(const BulgeArgs &args, int n_cus, hipStream_t stream);
hipError_t launch_bulge_write(const BulgeArgs &args, int n_cus, hipStream_t stream);
// chunk_sum[c] = sum of count[64 c .. 64 c + 64) (n cells in all)
hipError_t launch_bulge_chunk_sums(const uint32_t *count, uint64_t n, uint32_t *chunk_sum, hipStream_t stream);

}  // namespace vsc
