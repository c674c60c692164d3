/*
 * varscot_hip_debug.h - test and experiment hooks of libvarscot_hip.so.
 *
 * NOT part of the drop-in boundary (include/varscot_hip.h): nothing here is needed to use the library, and a
 * caller that never includes this header gets the defaults every measurement in DESIGN.md was taken with.  The
 * hooks exist so that tests can drive the rare paths of the library on inputs of a few thousand records (many
 * sort levels, several scoring passes, a failing RCCL load) and so that experiments can vary launch constants
 * without rebuilding.  They are explicit calls on a context: the library reads NO environment variable.
 */
#ifndef VARSCOT_HIP_DEBUG_H
#define VARSCOT_HIP_DEBUG_H

#include "varscot_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 0 (or -1 where stated) = the library's default. */
typedef struct {
    uint32_t seed_groups_per_cu; /* seed_sliced_kernel: resident workgroups per CU */
    uint32_t seed_reserve;       /* record slots a wave reserves per atomic (rounded to a power of two in 64..1024) */
    uint32_t sort_cap;           /* LDS capacity of the finalize kernel in records (16 .. 8064): small values force levels */
    uint32_t sort_max_bits;      /* key bits per partition level (1 .. 11) */
    int32_t sort_xcd;            /* -1 default; 0: partition tiles in index order; 1: one contiguous eighth per XCD */
    uint32_t sort_debug;         /* 1: per-level statistics on stderr; 2: every bin recounted on the host */
    int32_t sort_optimistic;     /* -1 default; 0: always histogram first; 1: slot partition first whenever a level partitions */
    uint32_t sort_slot_cap;      /* record slots per bin of the slot partition (default: derived from sort_cap) */
    uint64_t score_chunk;        /* rows per scoring pass */
    int32_t score_slices;        /* -1 default; 0 / 1: slice-major scoring order off / forced */
    uint32_t score_slice_shift;  /* log2 positions per slice (8 .. 31) */
    int32_t seed_shared;         /* -1 default; 0 / 1: one chunk per wave / one chunk per workgroup in seed_sliced_kernel */
    int32_t seed_group_out;      /* -1 default (on with chunk sharing); 0 / 1: per-wave / workgroup-shared open output blocks */
    int32_t seed_tight;          /* -1 default: segment thresholds follow what the site's PAM leaves of the limit, the cut chosen by the
                                    cost model; 0: floor(m / 3) in all three; 1 + k0 + 3 k1: segments 0 / 1 within k0 / k1 substitutions (if that is a valid cut) */
    int32_t rf_form;             /* -1 default (the best node form the forest allows); 0: plain nodes; 1: at most the compact form; 2 = -1 */
    uint32_t seed_parts;         /* seed search whose records go straight to the sort: launches the chunk range is cut into, the level-1
                                    partition of each running beside the next; 0: the library's choice, 1: one launch, n: n parts */
} vsc_debug_params;

/* Replaces the context's hooks (NULL: back to the defaults). */
int vsc_ctx_set_debug_params(vsc_ctx *ctx, const vsc_debug_params *params);
int vsc_ctx_get_debug_params(const vsc_ctx *ctx, vsc_debug_params *out);

/* A context whose stream may only use the compute units of `cu_mask` (bit i of word i / 32 = CU i, n_words words:
 * hipExtStreamCreateWithCUMask) - experiments with kernels of two contexts on disjoint parts of the device (tools/cu_mask_probe.py). */
int vsc_ctx_create_masked(int device_id, const uint32_t *cu_mask, uint32_t n_words, vsc_ctx **out);

/* Host-side lap times of vsc_search and vsc_windows_build on stderr (process-wide; 0 = off). */
void vsc_debug_set_host_timing(int on);

/* The host half of vsc_guides_enumerate_pattern's target test on its own (no device needed): the intervals as the sorted,
 * disjoint ranges of site starts the kernels look up, in GLOBAL positions (contig offset + position), for sites of `len`
 * bases.  ranges: 2 * capacity words, [lo, hi) per range; *n_ranges = how many there are (nothing is written when there are
 * more than capacity: VSC_ERR_RANGE).  VSC_ERR_INVALID as the call refuses. */
int vsc_debug_pattern_target_ranges(const vsc_contig *contigs, uint32_t n_contigs, const vsc_interval *iv, uint64_t n, uint32_t rule,
                                    uint32_t len, uint32_t *ranges, uint64_t capacity, uint64_t *n_ranges);

/* A vsc_guides made of the caller's arrays (tests of the calls that take one: candidates no enumeration would return, more of
 * them than a small genome holds).  ctx != NULL: the arrays are copied to its device, as vsc_guides_enumerate leaves its
 * result; ctx == NULL: a host-only object, as vsc_multi_guides_enumerate returns.  Nothing is checked.  Freed with
 * vsc_guides_free. */
int vsc_debug_guides_from_host(vsc_ctx *ctx, const uint64_t *codes, const vsc_locus *loci, uint64_t n, vsc_guides **out);
/* The same for a vsc_pattern_guides (freed with vsc_pattern_guides_free). */
int vsc_debug_pattern_guides_from_host(vsc_ctx *ctx, const uint64_t *codes, const vsc_locus *loci, uint64_t n, vsc_pattern_guides **out);

/* The device milliseconds of the context's last vsc_hits_sites / vsc_pattern_hits_sites, between HIP events on its stream:
 * the flag pass with the scan, and the write pass (either may be NULL).  The call leaves vsc_ctx_timing alone; this is where
 * tools/sites_bench.py reads what its kernels took. */
int vsc_debug_sites_ms(const vsc_ctx *ctx, double *flag_scan_ms, double *write_ms);

/* The device milliseconds of the context's last vsc_sites_table / vsc_bulge_hits_table, between HIP events on its stream: the
 * score kernel, the selection's bounds and radix select, and its walk (any may be NULL; vsc_bulge_hits_table and a call
 * without a selection leave the last two 0).  The calls leave vsc_ctx_timing alone; tools/site_table_bench.py reads this. */
int vsc_debug_site_table_ms(const vsc_ctx *ctx, double *score_ms, double *select_ms, double *walk_ms);

/* A vsc_bulge_hits / vsc_sites object over n records copied from the host as they are - for the tests of vsc_bulge_hits_table
 * and vsc_sites_table: lists of chosen lengths, and records that no search returns (a guide index too large, a split point
 * outside the protospacer, a position behind its contig), which those calls must score 0 without reading outside an array.
 * Nothing is verified.  Freed with vsc_bulge_hits_free / vsc_sites_free. */
int vsc_debug_bulge_hits_from_host(vsc_ctx *ctx, const vsc_bulge_hit *records, uint64_t n, vsc_bulge_hits **out);
int vsc_debug_sites_from_host(vsc_ctx *ctx, const vsc_site *records, uint64_t n, vsc_sites **out);

/* The occupancy bitmap in front of the edit search of vsc_*_prime and vsc_*_filter_prime on this context: 1 (the
 * default) on, 0 off - every lane whose reach could hold an edit then searches.  No output bit depends on it; tools/prime_bench.py
 * and the tests compare the two. */
int vsc_debug_prime_bitmap(vsc_ctx *ctx, int on);
/* The workgroups (of 4 waves) per CU that prime_rows_kernel's grid is capped at on this context: 0 = the default, 1 .. 64.
 * The kernel is grid-stride: no output bit depends on it (tools/prime_bench.py times several against each other). */
int vsc_debug_prime_groups_per_cu(vsc_ctx *ctx, uint32_t groups);
/* The same two hooks for vsc_*_hdr and vsc_*_filter_hdr: the occupancy bitmap in front of the edit search (1, the
 * default: on), and the workgroups per CU that hdr_rows_kernel's grid is capped at (0 = the default, 1 .. 64).  No output bit
 * depends on either. */
int vsc_debug_hdr_bitmap(vsc_ctx *ctx, int on);
int vsc_debug_hdr_groups_per_cu(vsc_ctx *ctx, uint32_t groups);
/* The workgroups per CU that fold_rows_kernel's grid (vsc_*_fold) is capped at: 0 = the default (8), 1 .. 64.  The
 * kernel is grid-stride: no output bit depends on it. */
int vsc_debug_fold_groups_per_cu(vsc_ctx *ctx, uint32_t groups);
/* The workgroups per CU that motif_rows_kernel's grid (vsc_*_motifs) is capped at: 0 = the default (8), 1 .. 64.  The
 * kernel is grid-stride and its counts are sums of integers: no output bit depends on it. */
int vsc_debug_motif_groups_per_cu(vsc_ctx *ctx, uint32_t groups);
/* The workgroups per CU that knockout_rows_kernel's grid (vsc_*_knockout) is capped at: 0 = the default (8), 1 .. 64.
 * The kernel is grid-stride, its queue belongs to a workgroup and every row is a function of its candidate: no output bit depends
 * on it.  With few workgroups a workgroup takes many steps, which is how the tests meet the queue's edges. */
int vsc_debug_knockout_groups_per_cu(vsc_ctx *ctx, uint32_t groups);
/* on != 0: knockout_rows_kernel runs without its queue - every coding lane walks where it lies, two lanes in 64 busy on a genome.
 * The variant the queue is measured against (tools/knockout_bench.py); every row, the coverage and the counts but drains /
 * drained are the same, which then count the wave steps with a coding lane and their coding lanes. */
int vsc_debug_knockout_in_place(vsc_ctx *ctx, int on);
/* What vsc_cds_build derived for the knock-out walk (host only): table (optional) = four uint32 per transcript - shift, E_t, J_t,
 * segments (all 0 for a transcript without a segment); *n_blocks = the bits of the occupancy bitmap, one per 256 global positions;
 * bitmap (optional) = its (*n_blocks + 31) / 32 words. */
int vsc_debug_knockout_table(const vsc_cds *cds, uint32_t *table, uint32_t *bitmap, uint32_t *n_blocks);

/* The block of the variation lookup's table on this context: log2 of the global positions per entry, 4 .. 32, or 0 =
 * the default (8).  At 32 the table has one block and the lookup is the plain lower bound over all variants.  No output bit
 * depends on it; the tests compare the smallest and a large block, tools/variation_bench.py times them against each other. */
int vsc_debug_variation_block_bits(vsc_ctx *ctx, uint32_t bits);

/* ---- the bin sort on the caller's records ------------------------------------------------------------------
 * vsc_debug_sort_records runs the record sink of a search pass (level 0 of the streaming scan, the result's storage, the
 * "slots allowed" memory, the bin sort with its levels and the finalize kernel) on records the CALLER made, under the
 * context's current vsc_debug_params: the tests choose the distribution the sort sees - bins of exact sizes, tiles and
 * segments of chosen lengths, positions at the top of 32 bits, contig tables of any shape.  The product path is untouched. */

/* A genome object that carries a contig table and nothing else (no planes: a sort without rows never reads them; no call
 * but vsc_debug_sort_records and vsc_genome_free takes it).  contig_off: n_contigs (1 .. 2^24) ascending global start
 * positions; span: one past the last position of the last contig, at most 2^32.  It also carries the sort's "slots allowed"
 * memory, as every genome does. */
int vsc_debug_genome_from_contigs(vsc_ctx *ctx, const uint32_t *contig_off, uint32_t n_contigs, uint64_t span, vsc_genome **out);

typedef struct {
    uint64_t first_slot; /* first 8-byte slot of the segment */
    uint32_t n_slots;    /* slots of the segment: records, sentinels, holes */
    uint32_t guide_base; /* read index of the segment's read 0 */
} vsc_debug_sort_segment;

typedef struct {
    /* the position encoding: pos_bits 1 .. 32 meaningful bits of the records' 32-bit position field (they sit at its top:
     * field = (global position - pos_base) << (32 - pos_bits)); pos_bits 0: as a search derives them from a genome that
     * covers the table's span - ceil(log2(span)) bits, pos_base 0 */
    uint32_t pos_bits, pos_base;
    uint32_t read_bits;  /* SEED form: bits of the read index inside a segment, 0 .. 6 (the sort's key: pos_bits + 1 + read_bits) */
    /* SEED form - record slots as the seed search leaves them: packed records, sentinels (all ones), and anything at all
     * in the slots that the fill table leaves out */
    const uint64_t *slots;
    uint64_t n_slots;
    const vsc_debug_sort_segment *segments; /* each ordered on its own; the result is their concatenation */
    uint32_t n_segments;
    uint32_t fill_shift;  /* with fill: log2 slots per block, 6 .. 13; every segment starts on a block boundary */
    const uint32_t *fill; /* NULL, or per block of 1 << fill_shift slots (ceil(n_slots / block) entries) the slots it holds */
    /* SCAN form (pair_keys != NULL; no segments then) - (key, value) pairs as scan_kernel leaves them: key = (read index
     * in the pass) << 33 | strand << 32 | global position, value = NM << 23 | mask; they go through level 0 */
    const uint64_t *pair_keys;
    const uint32_t *pair_vals;
    uint64_t n_pairs;
    uint32_t n_regions;  /* regions of 64 reads the pass has, 1 .. 256: every key's read index is below 64 * n_regions */
    uint32_t guide_base; /* read index of the pass's read 0 (a multiple of 64) */
    /* the genome's "slots allowed" memory before the sort (SEED form; the scan form never asks): -1 as earlier calls left
     * it, 0 forget the permission, 1 give it back - so that a fallback in one call need not change the path of the next */
    int32_t slots_allowed;
    uint32_t reserved;
} vsc_debug_sort_input;

typedef struct {
    uint64_t n;              /* records of the result */
    uint64_t bytes;          /* what the sort's kernels moved (vsc_timing.sort_bytes) */
    uint32_t levels;         /* partition levels run, level 0 not counted (vsc_timing.sort_levels) */
    uint32_t bin_bits;       /* key bits of the first of them */
    uint32_t slot_fallbacks; /* slot partitions that overflowed and ran again with the histogram */
    uint32_t slots_allowed;  /* the genome's memory after the call */
} vsc_debug_sort_info;

/* Sorts `in`'s records into a result like any search's (freed with vsc_hits_free).  The records themselves are not verified
 * (a key may repeat, a position may lie behind its contig); what would make a kernel index outside its tables is refused
 * with VSC_ERR_INVALID before anything is uploaded: a NULL argument, both forms at once, pos_bits > 32, read_bits > 6, a
 * segment that ends behind n_slots, a fill_shift outside 6 .. 13 or a segment off the block boundaries with a fill table,
 * n_regions outside 1 .. 256, a guide_base that is no multiple of 64 or that leaves no room for the regions' reads, a key
 * whose read index is not below 64 * n_regions, 2^32 pairs or more.  Zero segments / zero pairs: an empty result.  `info`
 * may be NULL; vsc_ctx_timing reports the same figures. */
int vsc_debug_sort_records(vsc_ctx *ctx, vsc_genome *genome, const vsc_debug_sort_input *in, vsc_debug_sort_info *info, vsc_hits **out);

typedef struct {
    int32_t rccl;             /* -1: RCCL when n > 1 distinct devices; 0: device copies; 1: insist on RCCL (also n = 1);
                                  2: try RCCL also for n = 1, device copies when it cannot be set up */
    const char *rccl_library;  /* NULL: librccl.so.1 / librccl.so; else the one name to dlopen (tests: a name that fails) */
} vsc_multi_debug_params;
/* vsc_multi_create with hooks (NULL = vsc_multi_create). */
int vsc_multi_create_debug(const int *device_ids, int n, const vsc_multi_debug_params *params, vsc_multi **out);

#ifdef __cplusplus
}
#endif
#endif
