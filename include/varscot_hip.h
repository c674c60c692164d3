/*
 * varscot_hip.h - C ABI of libvarscot_hip.so, the MI355X (gfx950) implementation of VARSCOT's
 * genome-wide off-target search hot path.
 *
 * The reference (BauerLab/VARSCOT) has no plugin / FFI interface: its only seams are the argv +
 * file boundaries between stage binaries.  This ABI is therefore the boundary a maintainer would
 * bind *inside* those binaries; every entry point cites the reference code it replaces
 * (paths relative to VARSCOT_pipeline/).  INTEGRATION.md shows the binding.
 *
 * Conventions: every call returns an int status (0 = VSC_OK, negative errno-style otherwise); no
 * C++ exception crosses the boundary; no global state; a vsc_ctx is single-threaded (a process
 * may own several, one per device / stream); all sizes are explicit; all buffers little-endian;
 * pointers are HOST pointers unless the parameter name ends in _dev.
 *
 * Genome layout ("packed planes"): the genome is one global coordinate space.  Contig c occupies
 * global positions [offset_c, offset_c + length_c); consecutive contigs are separated by at least
 * one N position, and every position outside a contig is N.  Three bit planes describe it, one bit
 * per base, bit b of 32-bit word w <-> global position 32*w + b:
 *     hi, lo : the 2-bit base code (A = 00, C = 01, G = 10, T = 11 as hi:lo; complement = NOT both)
 *     nmask  : 1 where the position is N / a separator / padding (hi and lo are then ignored)
 * = 0.375 byte per base.  The total padded length must be < 2^32 - 4096 (the reference's own limit
 * is 4 Gbases: read_mapping/bidir_index.cpp:17, read_mapping/common.h:12-18).
 */
#ifndef VARSCOT_HIP_H
#define VARSCOT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VSC_ABI_VERSION 5

#define VSC_OK 0
#define VSC_ERR_INVALID (-22)  /* EINVAL: bad argument (e.g. mismatches outside 0..8)          */
#define VSC_ERR_NOMEM (-12)    /* ENOMEM: host or device allocation failed                      */
#define VSC_ERR_DEVICE (-5)    /* EIO:    a HIP call failed, see vsc_last_error()               */
#define VSC_ERR_RANGE (-34)    /* ERANGE: genome / result does not fit the 32-bit position space */
#define VSC_ERR_NODEVICE (-19) /* ENODEV: no usable gfx950 device                               */

#define VSC_READ_LEN 23 /* VARSCOT fixes SEQLENGTH=23 (VARSCOT:253; CIGAR "23M" bidir_mapping.cpp:102) */
#define VSC_MAX_MISMATCHES 8 /* read_mapping/bidir_mapping.cpp:234-238 */

typedef struct vsc_ctx vsc_ctx;
typedef struct vsc_genome vsc_genome;
typedef struct vsc_hits vsc_hits;

/* One contig of the global coordinate space. */
typedef struct {
    uint64_t offset; /* global position of the contig's first base */
    uint32_t length; /* number of bases */
    uint32_t reserved;
} vsc_contig;

/*
 * One candidate off-target site = one record the reference inserts into its `records` map
 * (read_mapping/bidir_mapping.cpp:88-125).
 *   info: bit 31       strand, 1 = '-' (BAM_FLAG_RC, :97-98)
 *         bits 23..27  NM = mismatches over all 23 positions (:79-86,121)
 *         bits 0..22   mismatch mask in forward-genome window coordinates, bit i = window position
 *                      i differs from fullRead[i] - the information the reference routes through
 *                      the MD tag (:114-122) and re-parses in
 *                      variant_processing/filter_output_bam.h:330-349.
 */
typedef struct {
    uint32_t guide;  /* index of the read in input order (:287) */
    uint32_t contig; /* record.r.rID (:99) */
    uint32_t pos;    /* record.r.beginPos, 0-based (:100) */
    uint32_t info;
} vsc_hit;

#define VSC_HIT_STRAND(info) (((info) >> 31) & 1u)
#define VSC_HIT_NM(info) (((info) >> 23) & 31u)
#define VSC_HIT_MASK(info) ((info)&0x7FFFFFu)

/* Search options = the -M and -P options of bidir_mapping (read_mapping/bidir_mapping.cpp:207-216). */
typedef struct {
    uint32_t max_mismatches; /* -M, 0..8 (:234-238) */
    uint8_t has_extra_pam;   /* -P given */
    char extra_pam[2];       /* -P: additional non-canonical PAM besides (N)GG and (N)GA (:240-247) */
    uint8_t algorithm;       /* VSC_ALGO_*: how the (identical) hit set is computed */
} vsc_search_params;

/* Both algorithms return the same records.  SCAN streams the packed planes and compares every
 * PAM-valid window with every read.  SEED keeps the PAM-valid windows filed by 7-base segments in HBM
 * (built once per genome and PAM set, vsc_genome_build_index) and compares a read only with the
 * windows that a pigeonhole argument cannot rule out - the role the FM-index halves play in
 * read_mapping/bidir_mapping.cpp:129-162.  AUTO picks SEED when the index exists or the search is
 * large enough to pay for building it. */
#define VSC_ALGO_AUTO 0
#define VSC_ALGO_SCAN 1
#define VSC_ALGO_SEED 2

/* Per-search device timings measured with HIP events on the context's stream (milliseconds). */
typedef struct {
    double scan_ms;          /* the dominant search kernel: scan_kernel or seed_sliced_kernel (last pass) */
    double prep_ms;          /* read upload (+ per-bucket read lists for VSC_ALGO_SEED) */
    double sort_ms;          /* bin sort of the hit records: histogram + partition level(s) */
    double finalize_ms;      /* ordering inside the bins + contig resolution + record assembly (+ deeper sort levels) */
    double score_ms;         /* last vsc_score_hits call */
    double total_ms;         /* first launch to last completion of the last vsc_search */
    double index_ms;         /* last seed-index build on this context */
    uint64_t sites;          /* PAM-valid, N-free windows of the shard (both strands) */
    uint64_t pairs;          /* (window, read) comparisons made */
    uint64_t hits;           /* hits reported */
    uint64_t genome_bytes;   /* genome bytes the search kernel streamed: planes (SCAN) or visited site records (SEED) */
    uint32_t passes;         /* search launches needed (1 per read pass unless a hit buffer overflowed) */
    uint32_t algorithm;      /* VSC_ALGO_SCAN or VSC_ALGO_SEED: what ran */
    uint64_t sort_bytes;     /* bytes the sort kernels moved (8 per packed record read or written, 16 per result record) */
    uint32_t sort_levels;    /* partition levels the bin sort ran (0: the regions fitted its last stage as they were) */
    uint32_t sort_bin_bits;  /* key bits of the first partition level */
    uint32_t read_passes;    /* passes over the read set (a pass takes at most 16 384 reads) */
    uint32_t sort_fallbacks; /* sort levels that started without a histogram pass (fixed bin slots) and had to run again with
                                one because a bin outgrew its slot (repeat-rich genomes; the genome remembers) */
    uint64_t list_entries;   /* VSC_ALGO_SEED: entries of the per-bucket read lists the last pass made (8 bytes each, padding included) */
    uint32_t seed_cut;       /* VSC_ALGO_SEED: k0 | k1 << 4 - substitutions within which read segments 0 and 1 were searched (the third:
                                what the site's PAM leaves of the limit - k0 - k1 - 2) */
    uint32_t seed_layout;    /* VSC_ALGO_SEED: how the last pass's search laid its records out (0 for VSC_ALGO_SCAN) - bit 0: one chunk per
                                workgroup (else per wave); bit 1: workgroup-shared open output blocks (else per wave); bit 2: unused block
                                tails named by the block fill table (else written as sentinels); bits 4..7: log2 of the slots per block
                                (6..10); bits 8..15: launches the search was cut into (1..64; 1 after a rerun for lost records) */
} vsc_timing;

/* ---- context ------------------------------------------------------------------------------- */
int vsc_abi_version(void);
/* Number of visible HIP devices (0 when there is none); never initialises a device. */
int vsc_device_count(void);
/* Binds device_id and creates the context's stream.  Replaces: process start-up of bidir_mapping
 * (read_mapping/bidir_mapping.cpp:190-258). */
int vsc_ctx_create(int device_id, vsc_ctx **out);
/* Genomes and results created on a context must be freed before it. */
int vsc_ctx_destroy(vsc_ctx *ctx);
/* Gives the context's pooled device memory back (search / sort / scoring scratch, record buffers of freed results -
 * tens of GB after a large search; they are kept because hipMalloc / hipFree of such sizes cost hundreds of
 * milliseconds).  Genomes and live results are untouched; the next call allocates what it needs again. */
int vsc_ctx_release_scratch(vsc_ctx *ctx);
/* Run on a caller-owned hipStream_t (e.g. the framework's current stream) instead of the context's own. */
int vsc_ctx_set_stream(vsc_ctx *ctx, void *hip_stream);
/* Text of the last error on this context ("" if none).  Valid until the next call on ctx. */
const char *vsc_last_error(const vsc_ctx *ctx);
int vsc_ctx_timing(const vsc_ctx *ctx, vsc_timing *out);

/* ---- host-side packing helpers (no device needed) -------------------------------------------- */
/* Lays out n contigs in the global coordinate space (one N separator between contigs) and returns
 * the number of 32-bit words each plane needs.  Replaces the StringSet<Dna5String> concatenation of
 * read_mapping/bidir_index.cpp:36-40. */
uint64_t vsc_layout_contigs(const uint32_t *contig_len, uint32_t n_contigs, vsc_contig *out_table);
/* Initialises planes of n_words words to "all N". */
void vsc_planes_init(uint32_t *hi, uint32_t *lo, uint32_t *nmask, uint64_t n_words);
/* Writes n characters (ACGT any case; everything else = N, SeqAn Dna5 conversion) at global
 * position dst_pos. */
void vsc_pack_bases(const char *seq, uint64_t n, uint64_t dst_pos, uint32_t *hi, uint32_t *lo, uint32_t *nmask);
/* Inverse of vsc_pack_bases: n characters from global position src_pos. */
void vsc_unpack_bases(const uint32_t *hi, const uint32_t *lo, const uint32_t *nmask, uint64_t src_pos, uint64_t n,
                      char *out);
/* Packs one 23-nt read: 2 bits per base, base i in bits 2i..2i+1, A=0 C=1 G=2 T=3; every other
 * character becomes A (SeqAn Dna conversion of the reads, read_mapping/bidir_mapping.cpp:194,256,264). */
uint64_t vsc_pack_guide(const char *seq23);

/* ---- genome ---------------------------------------------------------------------------------- */
/*
 * Uploads (a shard of) the packed genome.  The arrays hold words [first_word, first_word+n_words)
 * of the global planes; windows STARTING in the first own_words words are searched, the remaining
 * words are halo (a 22-base halo = 1 word is enough); positions past the arrays are N.
 * contigs / n_contigs always describe the WHOLE genome (positions are reported per contig).
 * The caller keeps ownership of the host arrays; the library owns the device copies.
 * Replaces: open(index, path) + contig-name pass of read_mapping/bidir_mapping.cpp:268-280 (the
 * FM index is replaced by the resident planes).
 */
int vsc_genome_load(vsc_ctx *ctx, const uint32_t *hi, const uint32_t *lo, const uint32_t *nmask, uint64_t first_word,
                    uint64_t n_words, uint64_t own_words, const vsc_contig *contigs, uint32_t n_contigs,
                    vsc_genome **out);
int vsc_genome_free(vsc_genome *genome);
/* Builds (or keeps, if it matches) the seed index of a resident genome for the PAM set of `params`
 * (NULL = GG, GA only): the PAM-valid, N-free windows of both strands, filed once per 7-base
 * segment in bucket order (an 8-byte record + 4 bytes of bit-sliced planes per window and segment:
 * 36 bytes per window).  Plays the part of `bidir_index`
 * (read_mapping/bidir_index.cpp:45-47); vsc_search builds it on demand. */
int vsc_genome_build_index(vsc_ctx *ctx, vsc_genome *genome, const vsc_search_params *params);
/* The seed index as a file, for callers that keep `bidir_index`'s contract of an index built once and loaded by
 * every later run (read_mapping/bidir_index.cpp:45-47 writes, bidir_mapping.cpp:96-99 opens): _save writes the
 * resident index of `genome` (VSC_ERR_INVALID if it has none), _load replaces the genome's index with the file's.
 * The file names the library version, the PAM set, a fingerprint of the genome and the sizes of its arrays; _load
 * refuses a file that does not match or whose length is not what its header announces (VSC_ERR_INVALID,
 * vsc_last_error says why; the genome's index stays as it was - only a read error half-way leaves it without one).  36 bytes per window:
 * at 3 Gbp the file is 27 GB and rebuilding on the device (0.19 s) is faster than reading it - the tools only use the
 * file when asked to (bidir_index -S). */
int vsc_genome_index_save(vsc_ctx *ctx, const vsc_genome *genome, const char *path);
int vsc_genome_index_load(vsc_ctx *ctx, vsc_genome *genome, const char *path);
/* Bytes of HBM the resident genome (planes + seed index) occupies. */
uint64_t vsc_genome_device_bytes(const vsc_genome *genome);

/* ---- search ---------------------------------------------------------------------------------- */
/*
 * Searches every guide on both strands and returns all candidate sites, i.e. for every read the
 * union of the two searchAndVerifyEntireRead calls of read_mapping/bidir_mapping.cpp:285-295
 * (pigeonhole halves :157-162, find<0,k> :129-146, verify delegate :39-126), as the predicate
 * DESIGN.md states.  guides = n_guides values of vsc_pack_guide.  The result is sorted ascending
 * by (guide, strand '+' before '-', contig, pos) - the order of the reference's std::map (:154)
 * per read and strand; primary/secondary selection (:167-187) is host-side formatting
 * (vsc_sam_order).  The result is library-owned; release it with vsc_hits_free.
 */
int vsc_search(vsc_ctx *ctx, const vsc_genome *genome, const uint64_t *guides, uint32_t n_guides,
               const vsc_search_params *params, vsc_hits **out);
/*
 * The same search for read sets whose result does not fit the device at once (100 000 reads at 8
 * mismatches on 3 Gbp are 1.6e10 records): the reads are searched in batches of batch_reads (0 or more
 * than 16 384: 16 384) and every batch's result - same record order, guide = index into `guides` - is
 * handed to on_batch and freed when it returns.  The callback may use the result with any vsc_hits_* /
 * vsc_score_hits* call on the same context; a non-zero return value stops the stream and is returned.
 * Replaces the OpenMP loop over reads of read_mapping/bidir_mapping.cpp:285-295 for workloads where the
 * reference appends every read's records to its output buffer and moves on.
 * vsc_ctx_timing afterwards reports sums over the batches (score_ms: the callbacks' scoring calls).
 */
typedef int (*vsc_batch_fn)(void *user, vsc_hits *batch, uint32_t first_guide, uint32_t n_guides);
int vsc_search_stream(vsc_ctx *ctx, const vsc_genome *genome, const uint64_t *guides, uint32_t n_guides,
                      const vsc_search_params *params, uint32_t batch_reads, vsc_batch_fn on_batch, void *user);
/*
 * vsc_search_stream with the per-hit feature rows made ON THE WAY (BASELINE configuration 5: "streamed ... + per-hit
 * classification feature scoring"): every batch arrives with its 64-byte packed rows - rows_dev: device memory,
 * vsc_hits_count(batch) * 64 bytes, row i belongs to record i, valid inside the callback; the same rows as
 * vsc_score_hits_packed writes.  The search keeps each site's bases beside its hit record (4 bytes per hit through the
 * sort) and the kernel that assembles the vsc_hit records writes the row in the same pass - instead of a second kernel
 * that re-reads the records and gathers 23 bases per hit from the planes (a 64-byte sector for 46 bits).
 * Replaces, per batch: read_mapping/bidir_mapping.cpp:285-295 + variant_processing/merge_output_bam.h:696-708
 * (featureMatrixRecord of every record, feature_matrix.h:25-126).
 */
typedef int (*vsc_rows_batch_fn)(void *user, vsc_hits *batch, uint32_t first_guide, uint32_t n_guides, const void *rows_dev);
int vsc_search_stream_rows(vsc_ctx *ctx, const vsc_genome *genome, const uint64_t *guides, uint32_t n_guides,
                           const vsc_search_params *params, uint32_t batch_reads, vsc_rows_batch_fn on_batch, void *user);
/*
 * Per-guide off-target summary: what a guide-library screen asks of the search (how specific is each guide?) without
 * the records.  The counted hits of guide i are exactly the hits vsc_search returns for the same genome, guides and
 * params, minus the one at exclude[i] if that locus is a hit.  Over them:
 *   nm[k]      hits with NM = k (popcount of the mismatch mask, as VSC_HIT_NM)
 *   mit_sum    sum of rint(MIT * 2^24) (MIT = vsc_score_hits' score of the hit, rint = round half to even): a fixed-point
 *              sum, independent of the order of the hits and exact when passes or shards are added
 *   mit_ub     counted hits whose MIT score raised the reference-UB flag (vsc_score_hits' mit_flags)
 *   on_target  1 if exclude[i] was a hit (and was left out), else 0
 * exclude: NULL (nothing excluded) or n_guides loci in vsc_hit coordinates - 0-based leftmost window position on the
 * forward genome, strand 1 = '-' (BED6: chr, start, strand); contig == UINT32_MAX: none.  A contig >= the genome's
 * contig count (and not UINT32_MAX) or a strand > 1 is VSC_ERR_INVALID.  A genome loaded as one shard counts its own
 * windows only.  The search kernel's records are summarised where they lie: no sort, no result buffer, no record
 * leaves the device.  vsc_ctx_timing afterwards fills the fields vsc_search fills, with sort_ms = 0 and finalize_ms =
 * the summary kernel.  out: host memory, n_guides entries.
 * Replaces, for a screen: bidir_mapping (read_mapping/bidir_mapping.cpp:285-295) + the per-hit MIT scores of the
 * mergers (variant_processing/mit_score.h:12-68) + the guide-level aggregation CRISPOR reports as mitSpecScore.
 */
typedef struct {
    uint32_t contig, pos, strand, reserved; /* contig == UINT32_MAX: none */
} vsc_locus;
typedef struct {
    uint64_t mit_sum; /* sum of rint(MIT * 2^24) */
    uint64_t nm[9];
    uint64_t mit_ub;
    uint32_t on_target;
    uint32_t reserved;
} vsc_guide_summary;
#ifdef __cplusplus
static_assert(sizeof(vsc_guide_summary) == 96, "vsc_guide_summary layout");
#else
_Static_assert(sizeof(vsc_guide_summary) == 96, "vsc_guide_summary layout");
#endif
int vsc_search_summary(vsc_ctx *ctx, const vsc_genome *genome, const uint64_t *guides, uint32_t n_guides,
                       const vsc_search_params *params, const vsc_locus *exclude, vsc_guide_summary *out);
/*
 * Per-guide selection: the specificity number AND the handful of off-targets that matter, from one search.  For every guide,
 * of the hits vsc_search would return for the same genome, guides and params - minus the one at exclude[i] if that locus is
 * a hit - with  score = rint(MIT * 2^24)  (MIT as vsc_score_hits computes it, round half to even: the summary's unit):
 *   min_score  keeps the hits with score >= min_score (0: no floor);
 *   top_k      keeps, of those, the first top_k in the total order (score descending, strand '+' before '-', global position
 *              ascending) - ties in the score are broken by the order of vsc_search's result (0: no limit).  Records are
 *              unique per guide, so the selected set is fully determined.
 * The result is an ordinary vsc_hits SORTED AS vsc_search SORTS IT (guide, strand, contig, pos) that holds the selected records
 * only: every vsc_hits_* / vsc_score_hits* / vsc_score_classify_hits / vsc_sam_order call works on it unchanged; the rank order
 * is the caller's to restore (<= top_k records per guide).  top_k = 0, min_score = 0, exclude = NULL returns vsc_search's bytes.
 * Selection composes over genome shards (the tie-break uses the global position): the selection of the union of the
 * shards' selections is the selection on the whole genome.  Any n_guides (passes of <= 16 384 reads as vsc_search, every
 * pass's survivors appended to the one result).
 * The decision is made on the device over the search kernel's records where they lie (an exact radix select per guide): the
 * sort, the result buffer and everything downstream see the survivors only - 100 000 guides at 8 mismatches on 3 Gbp with
 * top_k = 100 return 160 MB instead of 260 GB.
 * summary (optional, n_guides rows, host memory): the rows vsc_search_summary writes for the same arguments - over ALL hits -
 * from the same search.  exclude: as vsc_search_summary (same validation); the excluded locus is neither selected nor counted.
 * select == NULL or a non-zero reserved field: VSC_ERR_INVALID; the rest as vsc_search.
 * vsc_ctx_timing afterwards: hits = all hits found (before the selection), scan_ms / prep_ms as after vsc_search, sort_ms =
 * the selection kernels (+ the summary kernel if asked for) + the partition levels of the survivors' sort, finalize_ms as after
 * vsc_search; sort_bytes counts what the bin sort moved: survivors only.
 * Replaces, for a screen: bidir_mapping (read_mapping/bidir_mapping.cpp:285-295) + the per-hit MIT scores of the mergers
 * (variant_processing/mit_score.h:12-68) + the cut by score the evaluation applies to the output afterwards
 * (workflow/siteseqPipelineComparison.R:41-49, subset(..., Score > x)) or the top of CRISPOR's off-target list.
 */
typedef struct {
    uint32_t top_k;      /* hits kept per guide, best first by (score desc, strand, position); 0 = no limit */
    uint32_t min_score;  /* keep hits with rint(MIT * 2^24) >= min_score; 0 = no floor */
    uint32_t reserved[2];
} vsc_select;
int vsc_search_select(vsc_ctx *ctx, const vsc_genome *genome, const uint64_t *guides, uint32_t n_guides,
                      const vsc_search_params *params, const vsc_select *select, const vsc_locus *exclude,
                      vsc_guide_summary *summary, vsc_hits **out);
/*
 * Region-aware summary and selection: where do a guide's off-targets fall?  An annotation (exons, a gene of interest, regions
 * the experiment does not care about, variant windows) is a set of intervals on the forward genome; a hit is IN THE REGIONS
 * when its 23-base window [pos, pos + 23) meets the set under the set's rule:
 *   VSC_REGION_OVERLAP  the window shares at least one base with some interval
 *   VSC_REGION_INSIDE   the window lies fully inside ONE interval - the test filterRefAlignment applies to a reference hit
 *                       and a variant window (variant_processing/filter_output_bam.h:70-124); two abutting intervals do not
 *                       contain a window that spans their seam
 * vsc_regions_build (host only, no device needed): iv = n intervals, 0-based half-open per contig as in BED, in any order,
 * overlapping and nested as they come; `end` is clipped to the contig's length, empty intervals are dropped, n = 0 is valid
 * (nothing is in the regions).  contig >= n_contigs, start > end, a non-zero reserved field or an unknown rule:
 * VSC_ERR_INVALID.  contigs / n_contigs: the WHOLE genome's table, as for vsc_genome_load.  The object is immutable, owns no
 * device memory and may be used with any context and any shard of that genome, from several threads at once; a context keeps
 * the device copy of the regions it used last (uploaded on first use, given back by vsc_ctx_release_scratch).
 * Inside: the intervals in global coordinates sorted by start, the running maximum of their ends (one binary search answers
 * either rule), and two bits per block of block_bases window starts - no start of the block is in the regions / every start
 * is / look it up - so that most hits are decided by one read of a table that stays in the L2 cache.
 */
typedef struct {
    uint32_t contig, start, end, reserved; /* 0-based, half-open, forward genome (BED) */
} vsc_interval;
#define VSC_REGION_OVERLAP 0
#define VSC_REGION_INSIDE 1
typedef struct vsc_regions vsc_regions;
typedef struct {
    uint64_t intervals;    /* intervals kept (non-empty after clipping) */
    uint32_t rule;         /* VSC_REGION_* */
    uint32_t block_bases;  /* window starts per block of the class table: a power of two */
    uint64_t blocks_out;   /* blocks none of whose starts is in the regions */
    uint64_t blocks_in;    /* blocks all of whose starts are in the regions */
    uint64_t blocks_mixed; /* blocks that need the interval search */
} vsc_regions_stats;
int vsc_regions_build(const vsc_contig *contigs, uint32_t n_contigs, const vsc_interval *iv, uint64_t n, uint32_t rule,
                      vsc_regions **out);
void vsc_regions_free(vsc_regions *r);
/* 1 if the window that starts at (contig, pos) is in the regions, else 0 (also for a contig or position outside the genome). */
int vsc_regions_contains(const vsc_regions *r, uint32_t contig, uint32_t pos);
int vsc_regions_info(const vsc_regions *r, vsc_regions_stats *out);
/*
 * Labels: WHICH interval is a window in?  The LABEL of the window that starts at (contig, pos) under a vsc_regions is the
 * index, in the caller's iv[] array as it was passed to vsc_regions_build, of one interval the window is in under the set's
 * rule (it shares a base with it / lies fully inside it).  Dropped empty intervals still count in the numbering: the index
 * addresses the caller's own table of names.  If no interval qualifies the label is VSC_REGION_NONE.  When several qualify
 * the label is the most specific one:
 *   1. the one with the largest start;
 *   2. among those, the one with the smallest (clipped) end;
 *   3. among those, the one with the lowest input index.
 * With genes and their exons in one BED file a hit in an exon is labelled with the exon and a hit in an intron with the gene;
 * exact duplicates resolve to the first one given.  For every (contig, pos) of the genome
 *   vsc_regions_locate(r, contig, pos) != VSC_REGION_NONE  <=>  vsc_regions_contains(r, contig, pos) == 1,
 * the cut-off windows at a contig's end that the host call allows included.
 * vsc_regions_locate: host only, no device needed; VSC_REGION_NONE also for r == NULL, a contig or position outside the
 * genome, and a set of more than 0xFFFFFFFE input intervals (labels are 32-bit: such a set is built without the label
 * structure, and the two calls below return VSC_ERR_RANGE for it).
 * vsc_hits_locate / vsc_guides_locate: labels[i] = the label of record / candidate i, computed on the device over the
 * object's own arrays where they lie, by one gather kernel (class table, binary search over the sorted starts, a walk over
 * the enclosing intervals whose length is bounded by the nesting depth of the annotation, not by its size); labels: host
 * memory, vsc_hits_count / vsc_guides_count entries.  A record whose contig is outside the regions' contig table, or whose
 * window does not lie wholly inside its contig, gets VSC_REGION_NONE.  vsc_hits_locate runs on the hits' own context - for a
 * merged multi-device result that is the result context (vsc_multi_result_ctx).  vsc_guides_locate labels the host-only
 * object of vsc_multi_guides_enumerate on the host.  The context keeps the device copy of the label structure of the regions
 * it located against last, beside the copy the sinks use (uploaded on first use, given back by vsc_ctx_release_scratch); a
 * caller who never asks for labels uploads nothing.  Neither call changes the object it labels, the order of anything, or
 * what vsc_ctx_timing reports.  n == 0: VSC_OK, nothing is launched.  A NULL argument: VSC_ERR_INVALID.
 * Replaces: the per-off-target annotation lookup CRISPOR reports as locusDesc ("exon:FANCF", "intron:ELAVL2";
 * workflow/pipeline-comparison), and the host-side join of vsc_guides_enumerate's candidates back to the target intervals
 * they came from ("the four best guides per gene").
 */
#define VSC_REGION_NONE 0xFFFFFFFFu
uint32_t vsc_regions_locate(const vsc_regions *r, uint32_t contig, uint32_t pos);
/*
 * vsc_search_summary with a second set of rows: out_all = exactly what vsc_search_summary writes for the same arguments,
 * out_in = the same fields over the counted hits that are in the regions (on_target as in out_all: the excluded locus is
 * counted in neither).  One search, one pass of the summary kernel over the records where they lie; positions are global, so
 * the rows of genome shards add up as the plain ones do.  regions == NULL or built for another contig table: VSC_ERR_INVALID.
 */
int vsc_search_summary_regions(vsc_ctx *ctx, const vsc_genome *genome, const uint64_t *guides, uint32_t n_guides,
                               const vsc_search_params *params, const vsc_locus *exclude, const vsc_regions *regions,
                               vsc_guide_summary *out_all, vsc_guide_summary *out_in);
/*
 * vsc_search_select among the hits on one side of the regions: scope VSC_REGION_KEEP selects among the hits in the regions,
 * VSC_REGION_DROP among those that are not; the floor and top_k then apply to what is left.  With a filter the stage runs
 * also for top_k = 0, min_score = 0 and then returns exactly the filtered records in vsc_search's order: INSIDE + DROP is
 * the reference-side shadow filter of the mergers (variant_processing/filter_output_bam.h:70-124) on the device.
 * summary_all / summary_in (optional): the rows of vsc_search_summary_regions for the same arguments from the same search,
 * whatever the scope.  filter == NULL: vsc_search_select (summary_in must then be NULL).  A non-zero reserved field, a scope
 * > 1 or regions == NULL inside a filter: VSC_ERR_INVALID.
 */
#define VSC_REGION_KEEP 0
#define VSC_REGION_DROP 1
typedef struct {
    const vsc_regions *regions;
    uint32_t scope; /* VSC_REGION_KEEP / VSC_REGION_DROP */
    uint32_t reserved;
} vsc_region_filter;
int vsc_search_select_regions(vsc_ctx *ctx, const vsc_genome *genome, const uint64_t *guides, uint32_t n_guides,
                              const vsc_search_params *params, const vsc_select *select, const vsc_region_filter *filter,
                              const vsc_locus *exclude, vsc_guide_summary *summary_all, vsc_guide_summary *summary_in,
                              vsc_hits **out);
/*
 * Guide discovery: which guides does a target contain?  A CANDIDATE is a 23-base window w = c[p, p + 23) of the forward genome,
 * wholly inside contig c (p + 23 == length is allowed), without N, with
 *   strand '+'  w[21..23) == pam              the guide is g = w
 *   strand '-'  w[0..2)  == revcomp(pam)      the guide is g = revcomp(w)
 * and locus (c, p, strand) in vsc_hit / vsc_locus coordinates: vsc_search(g, 0 mismatches) reports that locus, and exclude =
 * locus gives on_target = 1 (with a PAM other than GG / GA the search needs the same extra_pam).  It is KEPT when, with
 * g[0..20) the protospacer in guide orientation,
 *   pam[2]      g[21], g[22] equal these two letters (ACGT, any case; anything else: VSC_ERR_INVALID) - the GUIDE's PAM, NGG
 *               by default, not the off-target PAM set of vsc_search_params
 *   strands     0 both, 1 '+' only, 2 '-' only (> 2: VSC_ERR_INVALID)
 *   gc_min/max  the number of G / C in g[0..20) lies in [gc_min, gc_max]; gc_max == 0: no upper bound (a zeroed struct filters
 *               nothing); either > 20, or gc_min > gc_max != 0: VSC_ERR_INVALID
 *   max_t_run   the longest run of T in g[0..20) is <= max_t_run; 0: no limit (3 is CRISPOR's TTTT rule)
 *   regions     NULL: every window of the genome or shard; else the window is in the regions under their own rule
 *               (vsc_regions_contains); regions built for another contig table: VSC_ERR_INVALID
 *   max_guides  0: no cap; when more candidates are kept the call returns VSC_ERR_RANGE, vsc_last_error names the count and
 *               nothing is returned
 * params == NULL or a non-zero reserved field: VSC_ERR_INVALID.  A zeroed struct with pam = "GG" is the default.
 * The result is ordered by ascending (contig, pos), '+' before '-' at one position - the ascending global position, so the
 * results of genome shards concatenate in shard order to the whole genome's (a shard enumerates the windows that START in its
 * own words, as the searches do).  The bytes depend on the genome and the parameters only: every candidate is written at a
 * rank computed from per-tile counts (count pass, scan, write pass), nothing is appended through an atomic.
 * codes = vsc_pack_guide codes (what every search takes), loci usable as `exclude` as they are: "every guide in these exons,
 * ranked by specificity" is this call followed by vsc_search_summary on the same resident genome.
 * vsc_ctx_timing afterwards: scan_ms = total_ms = the enumeration kernels, sites = candidates kept, genome_bytes = plane
 * bytes the kernels read (with regions only tiles that hold a block of the class table that is not OUT are visited), the
 * sort, score and hit fields 0.  Scratch comes from the context's pools (vsc_ctx_release_scratch gives it back); the result
 * owns its two arrays until vsc_guides_free.
 * Replaces, for a caller who has a target and not yet the loci: the extraction of on-targets from a BED
 * (variant_processing/extract_fasta_ontargets.h:92-139), which needs every 23-mer's coordinates up front.
 */
typedef struct {
    char pam[2];
    uint8_t strands, gc_min, gc_max, max_t_run;
    uint16_t reserved0;
    uint64_t max_guides;
    uint32_t reserved[2];
} vsc_enum_params;
#ifdef __cplusplus
static_assert(sizeof(vsc_enum_params) == 24, "vsc_enum_params layout");
#else
_Static_assert(sizeof(vsc_enum_params) == 24, "vsc_enum_params layout");
#endif
typedef struct vsc_guides vsc_guides;
int vsc_guides_enumerate(vsc_ctx *ctx, const vsc_genome *genome, const vsc_regions *regions /* may be NULL */,
                         const vsc_enum_params *params, vsc_guides **out);
uint64_t vsc_guides_count(const vsc_guides *guides);
/* Host copies of the two arrays (made on first use; valid until vsc_guides_free).  Either pointer may be NULL. */
int vsc_guides_data(vsc_guides *guides, const uint64_t **codes, const vsc_locus **loci);
/* Device pointers (valid until vsc_guides_free); NULL for a host-only object (vsc_multi_guides_enumerate's) and when the
 * result is empty. */
int vsc_guides_data_dev(const vsc_guides *guides, const void **codes_dev, const void **loci_dev);
int vsc_guides_free(vsc_guides *guides);
/* The labels of a result's records / of the candidates under `regions` (see vsc_regions_locate above). */
int vsc_hits_locate(vsc_hits *hits, const vsc_regions *regions, uint32_t *labels);
int vsc_guides_locate(vsc_guides *guides, const vsc_regions *regions, uint32_t *labels);
/*
 * Bulge-tolerant search: the sites at which Cas9 cuts although the target carries one or two extra bases (a DNA bulge) or
 * lacks one or two (an RNA bulge) - what Cas-OFFinder and CRISPRitz report beside the substitution-only sites of vsc_search.
 *
 * READ    r[0..23), as the searches take it (vsc_pack_guide: non-ACGT becomes A).  r[0..20) is the protospacer, r[20..23) the
 *         PAM letters; the PAM letters count towards the mismatches, exactly as in the plain search.
 * SITE    budget m = max_mismatches in 0..8.  Site length L = 23 + d, d in {-2, -1, +1, +2}, limited by rna_max / dna_max in
 *         0..2.  The site is c[p, p + L) of contig c; in read orientation s = c[p, p + L) on '+' and revcomp(c[p, p + L)) on '-'.
 * The site (g, strand, c, p, d) is a hit iff all four of these hold:
 *   1. p + L <= len(c).  The right-edge rule of the plain predicate is not applied.
 *   2. s[L-2..L) is in {GG, GA} + {-P}: the PAM set of vsc_search_params.
 *   3. No N (non-ACGT genome letter) appears anywhere in the L bases, the bulged bases included.
 *   4. min_i nm(i) <= m, with nm(i) = the number of unequal pairs when
 *        DNA bulge, b = d > 0, i in [1, 19]:        r[j] pairs s[j] for j < i and s[j + b] for i <= j < 23; s[i..i+b) is unpaired
 *        RNA bulge, b = -d > 0, 1 <= i, i + b <= 19: r[j] pairs s[j] for j < i and s[j - b] for i + b <= j < 23; r[i..i+b) is unpaired
 * RECORD  one per hit site: NM = min_i nm(i), index = the smallest i that reaches it.  d = 0 is vsc_search's business and is
 *         never reported here.  A plain hit with NM <= m - 1 has bulged neighbours at index 1 (the site one base longer or
 *         shorter at its 5' end pairs as the plain window does but for r[0]); they ARE reported, as Cas-OFFinder reports them.
 *         vsc_hits_sites (below) collapses them with the plain hits into one record per cut site.
 * ORDER   ascending (guide, strand, contig, pos, d).  The bytes depend on the planes and the parameters only: every record is
 *         written at a rank computed from counts (count pass, scan, write pass), nothing is appended through an atomic.
 *
 * params: max_mismatches and the PAM set as for vsc_search; algorithm must be VSC_ALGO_AUTO or VSC_ALGO_SCAN (the seed index is
 * neither needed nor used; anything else: VSC_ERR_INVALID).  bulge_params: dna_max and rna_max both 0, or either above 2, or a
 * non-zero reserved field: VSC_ERR_INVALID.  guide_batch = reads per round of the count / scan / write passes (0: 16; more
 * than 64: 64) - it bounds the counter scratch (8 bytes per read of a round and 2 048 bases) and never changes the result.
 * max_hits: 0 no cap; when there are more records the call returns VSC_ERR_RANGE, vsc_last_error names the count and nothing
 * is returned (as vsc_guides_enumerate).  out == NULL: no record is allocated or written (rows only); rows == NULL: records
 * only; both NULL: VSC_ERR_INVALID.  rows: host memory, n_guides entries - count[k][nm] = hits of the guide with class k
 * (ascending d: RNA 2, RNA 1, DNA 1, DNA 2) and NM = nm.  n_guides == 0: VSC_OK, nothing is launched (*out = an empty result).
 * A genome loaded as one shard reports the sites that START in its own words (one halo word covers the 25 bases); the records
 * of all shards, merged by the order above, are the whole genome's.
 * vsc_ctx_timing afterwards: scan_ms = total_ms = the kernels, hits, sites = PAM-valid N-free candidate sites examined (all
 * enabled classes, both strands), pairs = site x read comparisons, passes = rounds; the sort, finalize and score fields 0.
 */
typedef struct {
    uint32_t guide;  /* index of the read in input order */
    uint32_t contig;
    uint32_t pos;    /* 0-based start of the site's L bases on the forward genome */
    uint32_t info;   /* bit 31 strand (1 = '-') | bit 12 kind (0 DNA, 1 RNA) | bits 10..11 size | bits 5..9 index | bits 0..4 NM */
} vsc_bulge_hit;
#define VSC_BULGE_STRAND(info) (((info) >> 31) & 1u)
#define VSC_BULGE_KIND(info) (((info) >> 12) & 1u) /* VSC_BULGE_DNA / VSC_BULGE_RNA */
#define VSC_BULGE_SIZE(info) (((info) >> 10) & 3u)
#define VSC_BULGE_INDEX(info) (((info) >> 5) & 31u)
#define VSC_BULGE_NM(info) ((info)&31u)
#define VSC_BULGE_DNA 0u
#define VSC_BULGE_RNA 1u
/* d = site length - 23: +size for a DNA bulge, -size for an RNA bulge */
#define VSC_BULGE_D(info) (VSC_BULGE_KIND(info) ? -(int)VSC_BULGE_SIZE(info) : (int)VSC_BULGE_SIZE(info))
#define VSC_BULGE_INFO(strand, kind, size, index, nm) \
    ((uint32_t)(strand) << 31 | (uint32_t)(kind) << 12 | (uint32_t)(size) << 10 | (uint32_t)(index) << 5 | (uint32_t)(nm))
#define VSC_BULGE_CLASSES 4 /* rows of vsc_bulge_summary, ascending d: RNA 2, RNA 1, DNA 1, DNA 2 */
typedef struct {
    uint32_t dna_max, rna_max; /* 0..2 each, not both 0 */
    uint32_t guide_batch;      /* 0: default */
    uint32_t reserved;
    uint64_t max_hits;         /* 0: no cap */
} vsc_bulge_params;
typedef struct {
    uint32_t count[VSC_BULGE_CLASSES][VSC_MAX_MISMATCHES + 1];
} vsc_bulge_summary;
#ifdef __cplusplus
static_assert(sizeof(vsc_bulge_hit) == 16, "vsc_bulge_hit layout");
static_assert(sizeof(vsc_bulge_params) == 24, "vsc_bulge_params layout");
static_assert(sizeof(vsc_bulge_summary) == 144, "vsc_bulge_summary layout");
#else
_Static_assert(sizeof(vsc_bulge_hit) == 16, "vsc_bulge_hit layout");
_Static_assert(sizeof(vsc_bulge_params) == 24, "vsc_bulge_params layout");
_Static_assert(sizeof(vsc_bulge_summary) == 144, "vsc_bulge_summary layout");
#endif
typedef struct vsc_bulge_hits vsc_bulge_hits;
int vsc_search_bulges(vsc_ctx *ctx, const vsc_genome *genome, const uint64_t *guides, uint32_t n_guides,
                      const vsc_search_params *params, const vsc_bulge_params *bulge_params, vsc_bulge_hits **out /* may be NULL */,
                      vsc_bulge_summary *rows /* may be NULL */);
uint64_t vsc_bulge_hits_count(const vsc_bulge_hits *hits);
/* Host copy of the records (made on first use; valid until vsc_bulge_hits_free). */
int vsc_bulge_hits_data(vsc_bulge_hits *hits, const vsc_bulge_hit **out);
/* Device pointer (valid until vsc_bulge_hits_free); NULL when the result is empty. */
const void *vsc_bulge_hits_data_dev(const vsc_bulge_hits *hits);
int vsc_bulge_hits_free(vsc_bulge_hits *hits);
/* The definition above for ONE read and ONE site in read orientation, on the host (no device needed): guide_code = a
 * vsc_pack_guide code, site_text = the 23 + d letters of s (ACGT, any case), d in {-2, -1, +1, +2}.  *nm = min_i nm(i), *index
 * = the smallest i that reaches it (either may be NULL).  It runs the function the kernels run.  A wrong d, a text of
 * another length or a letter that is not ACGT (such a site is never a hit): VSC_ERR_INVALID. */
int vsc_bulge_align(uint64_t guide_code, const char *site_text, int d, uint32_t *nm, uint32_t *index);
/*
 * Pattern search: any PAM and any guide length of 16 .. 32 bases - SaCas9 (21-22 + NNGRRT), Cas12a (TTTV at the 5' end +
 * 23-25), SpCas9-NG / SpRY (NGN, NRN), truncated guides, NRG as one PAM, degenerate letters in a guide.  The pattern / query
 * model of Cas-OFFinder: an IUPAC pattern that the site must satisfy, IUPAC guides whose N positions are not compared, and a
 * mismatch budget.
 *
 * LETTERS  The 15 IUPAC letters ACGT RYSWKM BDHV N, in any case, each as its set of bases.  Anything else, U included, gives
 *          VSC_ERR_INVALID.  comp() of a letter is the letter of the complemented set.
 * PATTERN  P[0..L), 16 <= L <= 32.  Every guide G[0..L) has the same length L.  Both are IUPAC.  A guide's N positions are the
 *          ones that are not compared; for Cas-OFFinder-style queries these are the PAM positions.  A guide that spells its PAM
 *          letters has them counted, exactly as the plain search counts r[20..23).
 * SITE     (g, strand, c, p).  It is c[p, p + L) of contig c.  In read orientation, s = c[p, p + L) on '+' and
 *          revcomp(c[p, p + L)) on '-'.
 * HIT      The site is a hit iff all four hold:
 *            1. p + L <= len(c).
 *            2. There is no N in the L bases.  N here means a non-ACGT genome letter; the planes keep no ambiguity codes.
 *            3. s[j] is in P[j] for every j.
 *            4. NM = #{ j : s[j] is not in G[j] } <= m, with m in 0..VSC_MAX_MISMATCHES.
 *          There is no right-edge rule.  A site that satisfies the pattern on both strands is reported on both.  This happens
 *          with a palindromic pattern.
 * RECORD   Five uint32_t, vsc_pattern_hit { guide, contig, pos, info, mask }, 20 bytes.  pos is the 0-based start on the
 *          forward genome.  info = strand << 31 | NM (NM in the low 6 bits).  mask bit i is set when forward-genome window
 *          position i is a mismatch.  This is vsc_hit's convention.  On '-' it is the read-orientation mask with bit j moved to
 *          L-1-j.
 * ROWS     vsc_pattern_summary { uint32_t count[VSC_MAX_MISMATCHES + 1]; } per guide, 36 bytes.
 * ORDER    Ascending (guide, strand, contig, pos).  The bytes depend on the planes and the parameters only.  Every record is
 *          written at a rank computed from counts.  Nothing is appended through an atomic and nothing is sorted.
 *          vsc_guides_enumerate and vsc_search_bulges work the same way.
 *
 * vsc_search_pattern: pattern = L letters, guides = n_guides * L letters without terminators.  len outside 16..32, a letter
 * that is no IUPAC letter, max_mismatches above 8, a non-zero reserved field or both outputs NULL: VSC_ERR_INVALID.
 * guide_batch = guides per round of the count / scan / write passes (0: 16; more than 64: 64) - it bounds the counter scratch
 * (8 bytes per guide of a round and 2 048 bases) and never changes the result.  max_hits: 0 no cap; when there are more records
 * the call returns VSC_ERR_RANGE, vsc_last_error names the count and nothing is returned.  out == NULL: no record is allocated
 * or written (rows only); rows == NULL: records only.  rows: host memory, n_guides entries.  n_guides == 0: VSC_OK, nothing is
 * launched (*out = an empty result).  A genome loaded as one shard reports the sites that START in its own words (one halo word
 * covers the 32 bases); the records of all shards, merged by the order above, are the whole genome's.  No seed index is used
 * and none is needed; MIT scores and classifier rows are defined for 20 + NGG only and stay with their own calls (table scores: since
 * added, vsc_search_pattern_table further down; bulges under a pattern: since added, vsc_search_pattern_bulges below).
 * The guides of a pattern are found by vsc_guides_enumerate_pattern (below).
 * vsc_ctx_timing afterwards: scan_ms = total_ms = the kernels, hits, sites = candidates (sites that satisfy the pattern and hold
 * no N, both strands), pairs = candidate x guide comparisons, passes = rounds; the sort, finalize and score fields 0.
 */
typedef struct {
    uint32_t guide;  /* index of the guide in input order */
    uint32_t contig;
    uint32_t pos;    /* 0-based start of the site's L bases on the forward genome */
    uint32_t info;   /* bit 31 strand (1 = '-') | bits 0..5 NM */
    uint32_t mask;   /* bit i: forward-genome window position i is a mismatch */
} vsc_pattern_hit;
#define VSC_PATTERN_STRAND(info) (((info) >> 31) & 1u)
#define VSC_PATTERN_NM(info) ((info)&63u)
#define VSC_PATTERN_INFO(strand, nm) ((uint32_t)(strand) << 31 | (uint32_t)(nm))
#define VSC_PATTERN_MIN_LEN 16
#define VSC_PATTERN_MAX_LEN 32
typedef struct {
    uint32_t max_mismatches; /* 0..VSC_MAX_MISMATCHES */
    uint32_t guide_batch;    /* 0: default */
    uint64_t max_hits;       /* 0: no cap */
    uint32_t reserved[2];
} vsc_pattern_params;
typedef struct {
    uint32_t count[VSC_MAX_MISMATCHES + 1];
} vsc_pattern_summary;
#ifdef __cplusplus
static_assert(sizeof(vsc_pattern_hit) == 20, "vsc_pattern_hit layout");
static_assert(sizeof(vsc_pattern_params) == 24, "vsc_pattern_params layout");
static_assert(sizeof(vsc_pattern_summary) == 36, "vsc_pattern_summary layout");
#else
_Static_assert(sizeof(vsc_pattern_hit) == 20, "vsc_pattern_hit layout");
_Static_assert(sizeof(vsc_pattern_params) == 24, "vsc_pattern_params layout");
_Static_assert(sizeof(vsc_pattern_summary) == 36, "vsc_pattern_summary layout");
#endif
typedef struct vsc_pattern_hits vsc_pattern_hits;
int vsc_search_pattern(vsc_ctx *ctx, const vsc_genome *genome, const char *pattern, const char *guides /* n_guides * len letters */,
                       uint32_t n_guides, uint32_t len, const vsc_pattern_params *params, vsc_pattern_hits **out /* may be NULL */,
                       vsc_pattern_summary *rows /* may be NULL */);
uint64_t vsc_pattern_hits_count(const vsc_pattern_hits *hits);
/* Host copy of the records (made on first use; valid until vsc_pattern_hits_free). */
int vsc_pattern_hits_data(vsc_pattern_hits *hits, const vsc_pattern_hit **out);
/* Device pointer (valid until vsc_pattern_hits_free); NULL when the result is empty. */
const void *vsc_pattern_hits_data_dev(const vsc_pattern_hits *hits);
int vsc_pattern_hits_free(vsc_pattern_hits *hits);
/* Conditions 2 and 3 and the count of condition 4 for ONE guide and ONE site in read orientation, on the host (no device
 * needed): pattern, guide and site_text = len letters each.  *hit = 1 when the site holds ACGT only and satisfies the pattern
 * (the caller compares *nm with its budget), *nm = the mismatches against the guide, *mask = bit j set when s[j] is not in G[j]
 * (read orientation; any of the three may be NULL).  A site letter outside ACGT makes the site no hit: *hit = 0, *nm = 0,
 * *mask = 0.  It runs the function the kernels run.  len outside 16..32, a NULL text or a pattern / guide letter that is no
 * IUPAC letter: VSC_ERR_INVALID. */
int vsc_pattern_match(const char *pattern, const char *guide, const char *site_text, uint32_t len, uint32_t *hit, uint32_t *nm,
                      uint32_t *mask);
/*
 * Bulges under a pattern: vsc_search_bulges for any nuclease - the DNA / RNA bulge report of Cas-OFFinder and CRISPRitz for
 * SaCas9, Cas12a, SpCas9-NG, truncated guides.  The pattern / guide model of vsc_search_pattern with the pairing of
 * vsc_search_bulges, in the record and the rows of vsc_search_bulges.
 *
 * INPUT    Pattern P[0..L) and guides G[0..L), IUPAC, exactly as vsc_search_pattern takes them (same letters, same refusals),
 *          a budget m in 0..8, dna_max / rna_max in 0..2 (not both 0), and the PROTOSPACER (a, n): read positions [a, e),
 *          e = a + n, the part of the guide in which a bulge may lie (SaCas9 (0, 21), Cas12a (4, 23), SpCas9 (0, 20)).
 * REFUSED  (VSC_ERR_INVALID)  n < 4 or e > L;  P[j] != N for some a <= j < e (a pattern constrains the PAM, not the
 *          protospacer; this is what makes the pattern condition independent of the split point);  L + dna_max > 32 or
 *          L - rna_max < 16 (the front end's word pair and its N fold);  everything vsc_search_pattern refuses.
 * SITE     (g, strand, c, p, d), d in {-rna_max..-1} + {1..dna_max}: c[p, p + L + d) of contig c; in read orientation
 *          s = that text on '+', its reverse complement on '-'.
 * PAIRING  DNA bulge (b = d > 0), split point i in [a+1, e-1]:  position j pairs s[j] for j < i and s[j + b] for j >= i;
 *          s[i .. i+b) is unpaired.
 *          RNA bulge (b = -d > 0), a+1 <= i and i + b <= e-1:  position j pairs s[j] for j < i and s[j - b] for j >= i + b;
 *          guide positions [i, i+b) are unpaired and never counted.
 *          So positions j <= a always pair from the 5' end, positions j >= e-1 always from the 3' end, whatever i is.
 * HIT      iff  1. p + L + d <= len(c);  2. no N in the L + d bases, the unpaired ones included;
 *               3. s[j] in P[j] for j < a and s[j + d] in P[j] for j >= e  (= the site satisfies
 *                  P[0..a) + N x (n + d) + P[e..L), Cas-OFFinder's bulged pattern);
 *               4. NM = min_i nm(i) <= m, nm(i) = #{ paired j : the paired site base is not in G[j] }.  A guide's N positions
 *                  never count; spelled PAM letters count, through the pairing above.
 * RECORD   vsc_bulge_hit as it is (16 bytes, VSC_BULGE_* macros): d = site length - L, index = the smallest i that reaches NM
 *          (<= 31: fits the 5 bits), NM.  One record per hit site.  d = 0 is vsc_search_pattern's and is never reported here.
 *          The bulged neighbours of plain hits (index a+1) are reported, as by vsc_search_bulges.
 * ROWS     vsc_bulge_summary as it is: count[class][NM], classes ascending d.
 * ORDER    ascending (guide, strand, contig, pos, d); the bytes depend on the planes and the parameters only - ranks from counts,
 *          no atomic append, no sort, guide_batch never changes them.
 *
 * Under N x 21 + GR, the protospacer (0, 20) and spelled 23-letter ACGT guides this is vsc_search_bulges' definition word for
 * word, and the records are byte-equal to its (default PAM set).
 * vsc_search_pattern_bulges: the result object is vsc_search_bulges' (vsc_bulge_hits_count / _data / _data_dev / _free).
 * max_hits, guide_batch (0: 16; more than 64: 64), n_guides == 0, out == NULL (rows only), rows == NULL (records only), both
 * NULL (VSC_ERR_INVALID), shards and scratch (the context's pools; vsc_ctx_release_scratch gives it back) behave as
 * vsc_search_pattern's.  vsc_ctx_timing afterwards: scan_ms = total_ms = the kernels, hits, sites = candidates of the enabled
 * classes on both strands (sites that satisfy their class's bulged pattern and hold no N), pairs = sites x guides, passes =
 * rounds.
 * vsc_pattern_bulge_align: the definition for ONE guide and ONE site on the host (no device needed), by the functions the
 * kernels run.  site_text = len + d letters in read orientation, d in {-2, -1, +1, +2}.  *hit = 1 when the site holds ACGT only
 * and satisfies condition 3 (the caller compares *nm with its budget); then *nm = NM and *index = the smallest split point that
 * reaches it.  A non-ACGT site letter or a site that fails condition 3: *hit = 0, *nm = 0, *index = 0.  Any of the three may
 * be NULL.  Everything REFUSED above (with dna_max / rna_max = the size of d), a wrong d, a NULL text or a site text of another
 * length: VSC_ERR_INVALID.
 * Not provided: a vsc_multi_* entry point (shard results merge by ORDER), a seed index for patterns, MIT or classifier scores
 * for other nucleases.  Suppressing the bulged neighbours of plain hits: since added, vsc_hits_sites below.
 */
typedef struct {
    uint32_t max_mismatches; /* 0..VSC_MAX_MISMATCHES */
    uint32_t guide_batch;    /* 0: default */
    uint64_t max_hits;       /* 0: no cap */
    uint32_t proto_start, proto_len; /* the protospacer [proto_start, proto_start + proto_len) in read positions */
    uint32_t dna_max, rna_max;       /* 0..2 each, not both 0 */
} vsc_pattern_bulge_params;
#ifdef __cplusplus
static_assert(sizeof(vsc_pattern_bulge_params) == 32, "vsc_pattern_bulge_params layout");
#else
_Static_assert(sizeof(vsc_pattern_bulge_params) == 32, "vsc_pattern_bulge_params layout");
#endif
int vsc_search_pattern_bulges(vsc_ctx *ctx, const vsc_genome *genome, const char *pattern, const char *guides /* n_guides * len letters */,
                              uint32_t n_guides, uint32_t len, const vsc_pattern_bulge_params *params, vsc_bulge_hits **out /* may be NULL */,
                              vsc_bulge_summary *rows /* may be NULL */);
int vsc_pattern_bulge_align(const char *pattern, const char *guide, const char *site_text, uint32_t len, uint32_t proto_start,
                            uint32_t proto_len, int d, uint32_t *hit, uint32_t *nm, uint32_t *index);
/*
 * Cut sites: the plain and the bulged alignments of a search collapsed into one record per genomic cut site - the merge step
 * that CRISPRitz and CRISPRme run over a bulge report before anything is counted or ranked.  One cut site shows up as up to
 * five alignments: the plain window plus the sites one or two bases longer or shorter that share its PAM.
 *
 * An ALIGNMENT is a record of a plain search or of a bulge search over the same guides and genome.
 *   - Plain records are vsc_hit or vsc_pattern_hit.  Their d is 0.
 *   - Bulged records are vsc_bulge_hit.  Their d is in {-2, -1, +1, +2}.
 *   - The site length is len + d.
 * Parameters: len is 23 for SpCas9, or the pattern's length.  anchor is one of:
 *   - VSC_SITE_ANCHOR_END: the 3' end of the site in read orientation is the fixed, PAM-side end.  SpCas9 and SaCas9 use this.
 *   - VSC_SITE_ANCHOR_START: the 5' end is fixed.  Cas12a uses this.
 * The anchor coordinate a of an alignment at forward start pos:
 *     anchor  strand  a
 *     END     '+'     pos + len + d
 *     END     '-'     pos
 *     START   '+'     pos
 *     START   '-'     pos + len + d
 * A SITE is the set of all input alignments with equal (guide, strand, contig, a).
 *   - A site has at most five members, one per d.
 *   - On the strand where a = pos, a site's members share pos.
 *   - On the other strand, the member with d' starts at pos + d - d'.  len cancels out of membership.
 * Its BEST alignment is the minimum under (NM + |d|, |d|, DNA before RNA).  The order is total inside a site.  A plain hit
 * therefore beats its own index-1 bulged neighbours (equal cost, smaller |d|).
 * Output is one record per site, in ascending (guide, strand, contig, pos, d) order OF THE BEST ALIGNMENT.  This is the order
 * the inputs have.
 *
 * vsc_hits_sites / vsc_pattern_hits_sites: the collapse on the device, over the records of two results where they lie - a
 * flag pass (one alignment per lane: a bounded walk in its own list, one binary search in the other), a scan of the 64-record
 * tiles' counts, one read-back that sizes the result, a write pass.  No sort, no append atomic: the bytes depend on the inputs
 * only.  Rules for both:
 *   - Either input may be NULL or empty.  Both NULL is VSC_ERR_INVALID.  A result of another context: VSC_ERR_INVALID.
 *   - out or rows may be NULL.  Both NULL is VSC_ERR_INVALID.  rows: host memory, n_guides entries.
 *   - A record whose guide is >= n_guides, a non-zero reserved field, an unknown anchor, or len outside 16..32: VSC_ERR_INVALID.
 *   - More than 2^32 - 1 alignments in total: VSC_ERR_RANGE.
 *   - Inputs must be in the order their searches return.  The results of vsc_search_select* qualify.  The order is NOT
 *     verified: records in another order give sites that mean nothing (no access leaves the lists, every walk is bounded).
 *   - The inputs and vsc_ctx_timing stay as they are, as with vsc_hits_pairs.
 *   - Scratch comes from the context's pools and is returned by vsc_ctx_release_scratch.
 * Shards: the members of one site can start in different shards, so the call is defined on MERGED records - the plain result
 * of a multi-device search, bulged records merged by their order on the host through vsc_sites_collapse.  There is no
 * vsc_multi_* entry.
 * vsc_sites_collapse / vsc_sites_collapse_pattern: the same definition on host arrays, by the functions the kernels run; they
 * need no device.  sites: room for `capacity` records or NULL (count and rows only); *n_sites (optional) = the number of
 * sites.  More sites than capacity when sites != NULL: VSC_ERR_RANGE, nothing is written to sites (rows and *n_sites are
 * valid).  The refusals of the device calls apply.
 * Not provided: merging sites whose anchors merely lie close (CRISPRme's 3-bp window: it needs chaining over anchor order),
 * leaving out the on-target, a vsc_multi_* entry point.  Scores for bulged alignments and for sites: since added,
 * vsc_bulge_hits_table / vsc_sites_table below.
 */
#define VSC_SITE_ANCHOR_END 0u
#define VSC_SITE_ANCHOR_START 1u
#define VSC_SITE_ABSENT 31u /* a members field without a member */
#define VSC_SITE_MEMBER_NM(members, d) (((members) >> (5 * ((d) + 2))) & 31u)
#define VSC_SITE_MEMBERS(members) (((members) >> 25) & 7u)
typedef struct {
    uint32_t guide, contig, pos; /* of the best alignment */
    uint32_t info;     /* VSC_BULGE_* layout; a plain best has size 0, kind 0, index 0 */
    uint32_t anchor;   /* a, forward genome */
    uint32_t members;  /* bits 5k..5k+4, k = d + 2: NM of the member with that d, 31 = absent; bits 25..27 = number of members */
    uint32_t best;     /* index of the best alignment in ITS input list (plain if size 0, else bulged) */
    uint32_t reserved; /* 0 */
} vsc_site;
typedef struct {
    uint32_t sites, alignments;  /* sites of the guide; input records of the guide */
    uint32_t bulge_only;         /* sites without a plain member */
    uint32_t count[3][VSC_MAX_MISMATCHES + 1]; /* sites by |d| and NM of the best */
} vsc_site_summary;
typedef struct { uint32_t len, anchor, reserved[2]; } vsc_site_params;
#ifdef __cplusplus
static_assert(sizeof(vsc_site) == 32, "vsc_site layout");
static_assert(sizeof(vsc_site_summary) == 120, "vsc_site_summary layout");
static_assert(sizeof(vsc_site_params) == 16, "vsc_site_params layout");
#else
_Static_assert(sizeof(vsc_site) == 32, "vsc_site layout");
_Static_assert(sizeof(vsc_site_summary) == 120, "vsc_site_summary layout");
_Static_assert(sizeof(vsc_site_params) == 16, "vsc_site_params layout");
#endif
typedef struct vsc_sites vsc_sites;
int vsc_hits_sites(vsc_ctx *ctx, vsc_hits *plain /* may be NULL */, vsc_bulge_hits *bulged /* may be NULL */, uint32_t n_guides,
                   const vsc_site_params *params, vsc_sites **out /* may be NULL */, vsc_site_summary *rows /* may be NULL */);
int vsc_pattern_hits_sites(vsc_ctx *ctx, vsc_pattern_hits *plain /* may be NULL */, vsc_bulge_hits *bulged /* may be NULL */,
                           uint32_t n_guides, const vsc_site_params *params, vsc_sites **out /* may be NULL */,
                           vsc_site_summary *rows /* may be NULL */);
uint64_t vsc_sites_count(const vsc_sites *sites);
/* Host copy of the records (made on first use; valid until vsc_sites_free). */
int vsc_sites_data(vsc_sites *sites, const vsc_site **out);
/* Device pointer (valid until vsc_sites_free); NULL when the result is empty. */
const void *vsc_sites_data_dev(const vsc_sites *sites);
int vsc_sites_free(vsc_sites *sites);
int vsc_sites_collapse(const vsc_hit *plain, uint64_t n_plain, const vsc_bulge_hit *bulged, uint64_t n_bulged, uint32_t n_guides,
                       const vsc_site_params *params, vsc_site *sites /* may be NULL */, uint64_t capacity, uint64_t *n_sites,
                       vsc_site_summary *rows /* may be NULL */);
int vsc_sites_collapse_pattern(const vsc_pattern_hit *plain, uint64_t n_plain, const vsc_bulge_hit *bulged, uint64_t n_bulged,
                               uint32_t n_guides, const vsc_site_params *params, vsc_site *sites /* may be NULL */, uint64_t capacity,
                               uint64_t *n_sites, vsc_site_summary *rows /* may be NULL */);
/*
 * Pattern guide discovery: which guides of ANY nuclease does a target contain?  vsc_guides_enumerate for a pattern - the
 * beginning of the route that vsc_search_pattern continues: "every Cas12a guide in these exons with its off-target counts" is
 * this call, vsc_pattern_guide_text and vsc_search_pattern (rows only) on one resident genome.
 *
 * PATTERN    P[0..L), 16 <= L <= 32, IUPAC, exactly as vsc_search_pattern takes it (same letters, same refusals).
 * PROTOSP.   a range [a, a + k) of read positions, 1 <= k, a + k <= L: the part of the site that is the guide proper
 *            (SaCas9: a = 0, k = 21 of L = 27; Cas12a: a = 4, k = 23 of L = 27).  The filters look at it and nothing else.
 * CANDIDATE  (strand, c, p): the site c[p, p + L) of the forward genome with p + L <= len(c) (no right-edge rule), no non-ACGT
 *            genome letter in it, and s[j] in P[j] for every j, where s = c[p, p + L) on '+' and revcomp(c[p, p + L)) on '-'
 *            (conditions 1-3 of vsc_search_pattern's HIT).  A site that satisfies the pattern on both strands is two
 *            candidates.  On '-' the protospacer is forward window positions [L - a - k, L - a).
 * KEPT       strands  0 both, 1 '+' only, 2 '-' only.
 *            gc       #G/C in s[a, a + k) lies in [gc_min, gc_max]; gc_max == 0: no upper bound (a zeroed struct filters
 *                     nothing).  Either > k, or gc_min > gc_max != 0: VSC_ERR_INVALID.
 *            t run    the longest run of T inside s[a, a + k) is <= max_t_run (0: no limit).  Letters outside the protospacer
 *                     neither start nor extend a run: TTT at the protospacer's end followed by a T of the PAM is a run of 3.
 *            targets  NULL: every site of the genome or shard.  Else n vsc_interval (0-based half-open, any order, nested and
 *                     overlapping as they come, end clipped to the contig, empty ones dropped; n == 0: nothing is kept) and a
 *                     rule applied to the L-base site:
 *                       VSC_REGION_OVERLAP  p < end and p + L > start for some interval
 *                       VSC_REGION_INSIDE   start <= p and p + L <= end for ONE interval (a site across the seam of two
 *                                           abutting intervals is not inside)
 *                     contig >= n_contigs, start > end, a non-zero reserved field, an unknown rule: VSC_ERR_INVALID.
 *            max_guides  0: no cap; more kept: VSC_ERR_RANGE, the count in vsc_last_error, nothing returned.
 * ORDER      ascending (contig, pos), '+' before '-' at one position.  A shard enumerates the sites that START in its own
 *            words; shard results concatenate in shard order to the whole genome's.  The bytes depend on the planes and
 *            the parameters only: count pass, scan, write pass - no append atomic, no sort.
 * RECORD     code: uint64_t, hi plane << 32 | lo plane of s in READ orientation, bit j = s[j], A 00 C 01 G 10 T 11 as (hi, lo),
 *            bits from L on zero.  locus: vsc_locus { c, p, strand, 0 } - pos is the site's start on the forward genome, which
 *            is vsc_pattern_hit.pos of the hit that vsc_search_pattern reports for this guide at NM 0.
 *
 * For L = 23, P = N x 21 + GG and the protospacer (0, 20) this is vsc_guides_enumerate's definition with pam "GG", filter by
 * filter, and with targets vsc_regions_contains on the same intervals under the same rule.  The targets are a plain array, not
 * a vsc_regions: that object's class table is built for 23-base windows.  Here the intervals become sorted, disjoint ranges
 * of site starts ([start - L + 1, end) / [start, end - L] per interval, clipped to the contig, then the union), which holds
 * for any L; only the tiles that meet a range are visited.
 * vsc_guides_enumerate_pattern: pattern = len letters.  A NULL argument but `targets`, len outside 16..32, a letter that is no
 * IUPAC letter, a protospacer outside the pattern or empty, strands > 2, the gc refusals above, a non-zero reserved field or
 * n_targets != 0 with targets == NULL: VSC_ERR_INVALID.  The result owns its two arrays until vsc_pattern_guides_free;
 * scratch comes from the context's pools (vsc_ctx_release_scratch gives it back).
 * vsc_ctx_timing afterwards, as vsc_guides_enumerate: scan_ms = total_ms = the kernels, sites = candidates kept,
 * genome_bytes = plane bytes the kernels read, everything else 0.
 * vsc_pattern_guide_text (host only, no device needed): the letters of one code into out[0 .. len), no terminator - inside
 * the protospacer the site's letter; outside it N when spell == 0 (the Cas-OFFinder query form: those positions are not
 * compared by vsc_search_pattern) and the site's letter when spell == 1.  Upper-case ACGT.  The output is exactly one guide
 * of vsc_search_pattern's `guides` argument.  len outside 16..32, a protospacer outside the pattern or empty, spell > 1, a
 * code with a bit from len on set in either plane, out == NULL: VSC_ERR_INVALID.
 * Not provided: a vsc_multi_* entry point (the pattern search has none either; shard results concatenate, see ORDER),
 * labels (which target interval a candidate lies in), guide pairs, and MIT or classifier scores for patterns - those stay
 * defined for 20 + NGG with vsc_guides_enumerate's family.
 */
typedef struct {
    uint8_t ps_start, ps_len; /* the protospacer [ps_start, ps_start + ps_len) in read positions */
    uint8_t strands, gc_min, gc_max, max_t_run;
    uint16_t reserved0;
    uint32_t rule; /* VSC_REGION_OVERLAP / VSC_REGION_INSIDE: how `targets` are applied (ignored when targets == NULL) */
    uint32_t reserved1;
    uint64_t max_guides;
    uint32_t reserved[2];
} vsc_pattern_enum_params;
#ifdef __cplusplus
static_assert(sizeof(vsc_pattern_enum_params) == 32, "vsc_pattern_enum_params layout");
#else
_Static_assert(sizeof(vsc_pattern_enum_params) == 32, "vsc_pattern_enum_params layout");
#endif
typedef struct vsc_pattern_guides vsc_pattern_guides;
int vsc_guides_enumerate_pattern(vsc_ctx *ctx, const vsc_genome *genome, const char *pattern, uint32_t len,
                                 const vsc_pattern_enum_params *params, const vsc_interval *targets /* may be NULL */,
                                 uint64_t n_targets, vsc_pattern_guides **out);
uint64_t vsc_pattern_guides_count(const vsc_pattern_guides *guides);
/* Host copies of the two arrays (made on first use; valid until vsc_pattern_guides_free).  Either pointer may be NULL. */
int vsc_pattern_guides_data(vsc_pattern_guides *guides, const uint64_t **codes, const vsc_locus **loci);
/* Device pointers (valid until vsc_pattern_guides_free); NULL when the result is empty. */
int vsc_pattern_guides_data_dev(const vsc_pattern_guides *guides, const void **codes_dev, const void **loci_dev);
int vsc_pattern_guides_free(vsc_pattern_guides *guides);
int vsc_pattern_guide_text(uint64_t code, uint32_t len, uint32_t ps_start, uint32_t ps_len, uint32_t spell, char *out /* len letters */);
/*
 * Paired-nickase screen (Cas9 D10A double nickase, dimeric FokI-dCas9): a design of TWO guides cuts only where an off-target
 * of one guide and an off-target of the other lie close together on opposite strands.  Coordinates are vsc_hit's and
 * vsc_locus': pos = 0-based leftmost base of the 23-base window on the forward genome, strand 1 = '-'.  Two windows on the
 * same contig and on opposite strands have
 *     delta = pos(the '+' window) - pos(the '-' window)      (signed)
 * and are PAIRED under [delta_min, delta_max] iff delta_min <= delta <= delta_max.  delta does not depend on which guide sits
 * on which strand, and the reverse complement of a locus has the same delta, so one range meets both orientations of an
 * off-target locus.  The nickase literature's offset (gap between the protospacers' PAM-distal ends, negative = overlap) is
 * delta - 23; PAM-out (the '-' window to the left) is delta > 0, PAM-in a negative range.  Windows on different contigs or on
 * the same strand never pair.  pos +- delta is computed in 64-bit signed integers and clipped to [0, UINT32_MAX].
 * delta_min > delta_max, a bound outside +-2^30 or a non-zero reserved field: VSC_ERR_INVALID.
 *
 * vsc_loci_pairs: host only, no device needed.  Every (a, b) - indices into loci[], any order of loci[] - with loci[a] a '-'
 * window, loci[b] a '+' window and the two PAIRED, in ascending (a, b).  Entries with contig == UINT32_MAX (or a strand > 1)
 * take part in nothing; two equal loci are two entries.  *n_pairs = the full count, always; pairs == NULL only counts; a count
 * above capacity is VSC_ERR_RANGE and nothing is written.  Replaces a host loop over vsc_guides_enumerate's loci.
 * vsc_guides_pairs: the same contract and bytes over the object's own loci, computed on the device over the array where it
 * lies (ascending (contig, pos, '+' before '-'): per '-' candidate one bound and a walk that keeps '+'; count, scan, write as
 * vsc_guides_enumerate, no append atomic - the bytes depend on the input only).  A host-only object
 * (vsc_multi_guides_enumerate's) is answered by vsc_loci_pairs.  pairs: host memory.  More than 2^32 - 2048 candidates:
 * VSC_ERR_RANGE.  The object and what vsc_ctx_timing reports stay as they are.
 *
 * vsc_hits_pairs: the join.  hits: any result in vsc_search order (vsc_search, vsc_search_select*, a merged multi-device
 * result); the call runs on the hits' own context, as vsc_hits_locate.  For pair j = (a, b) a PAIRED SITE is a record of guide
 * a and a record of guide b whose windows are PAIRED - either strand assignment.  With exclude (n_guides loci, as
 * vsc_search_summary's; no genome is at hand, so of an entry only strand > 1 is refused) the pair's ON-TARGET - a-record at
 * exclude[a], b-record at exclude[b] in contig, position and strand - is not counted and sets on_target = 1.  Over the
 * counted sites of pair j, rows[j] holds
 *   sites      their number
 *   nm_sum[k]  sites with NM(a-record) + NM(b-record) = k
 *   nm_max[k]  sites with max(NM(a-record), NM(b-record)) = k
 * sites (optional, host memory, `capacity` entries): the counted sites in ascending (pair, a_rec, b_rec) - a_rec, b_rec:
 * record indices into hits, delta as above; the sites of one pair are contiguous, prefix sums of rows[].sites are their
 * offsets.  *n_sites (optional) = the full total.  A total above capacity when sites != NULL: VSC_ERR_RANGE, rows and *n_sites
 * are valid (size a second call from them).  a == b, an index >= n_guides, a record whose guide is >= n_guides, n_guides >=
 * 2^31, a NULL hits / p / rows (n_pairs > 0), a NULL pairs when n_pairs > 0: VSC_ERR_INVALID.  More than 2^32 - 1 records, or
 * - when sites are asked for - more than 2^32 - 2048 (pair, a-record) work items: VSC_ERR_RANGE.  n_pairs == 0 or an empty
 * result: VSC_OK, zeroed rows, nothing is launched.  A guide may be in any number of pairs; duplicate pairs get a row each.
 * The records and what vsc_ctx_timing reports stay as they are; scratch comes from the context's pools
 * (vsc_ctx_release_scratch gives it back).
 * Replaces: nothing in the reference (it has no pair notion; its mergers' rows are per guide); for a caller, the copy of all
 * records to the host and a join there.
 */
typedef struct {
    int32_t delta_min, delta_max;
    uint32_t reserved[2];
} vsc_pair_params;
typedef struct {
    uint32_t a, b; /* a: the '-' window / first guide, b: the '+' window / second guide */
} vsc_guide_pair;
typedef struct {
    uint64_t sites;
    uint64_t nm_sum[17];
    uint64_t nm_max[9];
    uint32_t on_target;
    uint32_t reserved;
} vsc_pair_summary;
typedef struct {
    uint32_t pair, a_rec, b_rec;
    int32_t delta;
} vsc_pair_site;
#ifdef __cplusplus
static_assert(sizeof(vsc_pair_params) == 16 && sizeof(vsc_guide_pair) == 8, "vsc_pair_params / vsc_guide_pair layout");
static_assert(sizeof(vsc_pair_summary) == 224 && sizeof(vsc_pair_site) == 16, "vsc_pair_summary / vsc_pair_site layout");
#else
_Static_assert(sizeof(vsc_pair_params) == 16 && sizeof(vsc_guide_pair) == 8, "vsc_pair_params / vsc_guide_pair layout");
_Static_assert(sizeof(vsc_pair_summary) == 224 && sizeof(vsc_pair_site) == 16, "vsc_pair_summary / vsc_pair_site layout");
#endif
int vsc_loci_pairs(const vsc_locus *loci, uint64_t n, const vsc_pair_params *p, vsc_guide_pair *pairs, uint64_t capacity,
                   uint64_t *n_pairs);
int vsc_guides_pairs(vsc_guides *guides, const vsc_pair_params *p, vsc_guide_pair *pairs, uint64_t capacity, uint64_t *n_pairs);
int vsc_hits_pairs(vsc_hits *hits, uint32_t n_guides, const vsc_guide_pair *pairs, uint32_t n_pairs, const vsc_pair_params *p,
                   const vsc_locus *exclude /* optional, n_guides */, vsc_pair_summary *rows /* n_pairs */,
                   vsc_pair_site *sites /* optional */, uint64_t capacity, uint64_t *n_sites /* optional */);
/* CRISPOR's guide specificity from a mit_sum: (100 / (100 + mit_sum * 2^-24)) * 100 in that order.  The tools round
 * it with floor(x + 0.5), the round() CRISPOR used.  Host only, no device needed. */
double vsc_mit_specificity(uint64_t mit_sum);
uint64_t vsc_hits_count(const vsc_hits *hits);
/* Device pointer to vsc_hits_count() records of type vsc_hit (valid until vsc_hits_free). */
const void *vsc_hits_data_dev(const vsc_hits *hits);
/* Host copy of the records (made on first use; valid until vsc_hits_free). */
int vsc_hits_data(vsc_hits *hits, const vsc_hit **out);
/* Copies the records into caller memory (host, or device when dst_is_device != 0 - e.g. a tensor the
 * caller hands to RCCL). */
int vsc_hits_copy(vsc_hits *hits, void *dst, int dst_is_device);
/*
 * Multi-GPU: merges the results of genome shards.  records = the vsc_hit records of shard 0,
 * shard 1, ... concatenated in shard order (shard_counts[s] records each, as vsc_search returned them;
 * contig and pos are already global, so nothing is rewritten), in device memory when
 * records_on_device != 0 (the buffer RCCL gathered into), else in host memory (uploaded first).
 * Shards partition the positions in ascending order, so the global result is, for every
 * (guide, strand), shard 0's segment followed by shard 1's, ...: segments are located and copied,
 * nothing is sorted.  Replaces the concatenation of per-thread output buffers,
 * read_mapping/bidir_mapping.cpp:307-308.
 */
int vsc_hits_merge(vsc_ctx *ctx, const void *records, int records_on_device, const uint64_t *shard_counts,
                   uint32_t n_shards, uint32_t n_guides, vsc_hits **out);
/*
 * The same merge over the 8-byte EXCHANGE RECORDS - what the multi-GPU drivers send over xGMI instead of the
 * 16-byte vsc_hit: bits 0..22 mismatch mask | bits 23..54 global position (contig offset + pos).  Guide and strand
 * are not sent: a shard's records are sorted by key = guide << 1 | strand, so 4 bytes per key (key_counts) say which
 * records belong to which key; NM is the popcount of the mask; the contig follows from the global position.
 *   vsc_hits_pack_exchange  writes vsc_hits_count(hits) records (device memory when records_on_device != 0, e.g. a
 *                           tensor handed to RCCL) and the 2 * n_guides per-key record counts (host memory).
 *   vsc_hits_merge_packed   records = the exchange records of shard 0, shard 1, ... concatenated, each shard's for the
 *                           keys [first_key, first_key + n_keys) only (a receiver may collect just its read range);
 *                           key_counts[s * n_keys + k] = records of shard s with key first_key + k.  The result holds
 *                           ordinary vsc_hit records (guide = key >> 1), sorted as vsc_search sorts them; `genome`
 *                           (any shard of the genome on this context) supplies the contig table.
 */
#define VSC_XREC_BYTES 8
int vsc_hits_pack_exchange(vsc_ctx *ctx, const vsc_genome *genome, const vsc_hits *hits, uint32_t n_guides, void *records,
                           int records_on_device, uint32_t *key_counts);
int vsc_hits_merge_packed(vsc_ctx *ctx, const vsc_genome *genome, const void *records, int records_on_device,
                          const uint32_t *key_counts, uint32_t n_shards, uint32_t first_key, uint32_t n_keys, vsc_hits **out);
/* vsc_hits_merge_packed for records that carry 2 bytes of per-hit results each (the votes of the shard's classifier,
 * vsc_score_classify_hits: computed where the hit was found, before the exchange): `votes` = one uint16 per exchange record, same
 * order and the same memory space as `records`; votes_out (count of the merged records x 2 bytes; device memory when
 * votes_out_on_device != 0) receives them in the order of the merged records. */
int vsc_hits_merge_packed_votes(vsc_ctx *ctx, const vsc_genome *genome, const void *records, const void *votes, int on_device,
                                const uint32_t *key_counts, uint32_t n_shards, uint32_t first_key, uint32_t n_keys, vsc_hits **out,
                                void *votes_out, int votes_out_on_device);
int vsc_hits_free(vsc_hits *hits);

/*
 * Per-hit scores for rows [first, first+count) of a result (rows R5/R6):
 *   mit       : count doubles  = calcMitScore (variant_processing/mit_score.h:12-68) on the hit's
 *               mismatch positions (forward-genome orientation, as merge_output_bam.h:549 passes them)
 *   mit_flags : count bytes, 1 where the reference would index its weight table out of bounds
 *   features  : count * 442 bytes = featureMatrixRecord (variant_processing/feature_matrix.h:25-126)
 *               of (guide, off-target in guide orientation), as merge_output_bam.h:696 calls it
 * Any of the three output pointers may be NULL.  guides must be the array passed to vsc_search.
 * A row range whose scores do not fit the free device memory at once is scored in several passes over
 * the same scratch buffers (VSC_ERR_NOMEM only if not even 65 536 rows fit).
 */
int vsc_score_hits(vsc_ctx *ctx, const vsc_genome *genome, const vsc_hits *hits, const uint64_t *guides,
                   uint32_t n_guides, uint64_t first, uint64_t count, double *mit, uint8_t *mit_flags,
                   uint8_t *features);
#define VSC_N_FEATURES 442
/*
 * Feature rows in packed form, 64 bytes (16 little-endian 32-bit words) per hit instead of 442:
 *   w0      bits 0..20 mismatchPos1..21 | 21..25 totalMismatches | 26..30 adjacentMismatches
 *   w1      bits 0..11 AtoC..TtoG | 12..16 transitionNumber | 17..21 transversionNumber | 22..25 seedMismatches
 *   w2..w4  A1..T20, PAMA..PAMT one-hots (bit 4 i + base)
 *   w5..w14 AA1..TT19 one-hots (bit 16 i + pair); the 16 dinucleotide counts are their column sums
 *   w15     0
 * The rows are written to packed_dev (device memory, count * 64 bytes) or, if that is NULL, to library
 * scratch - as many rows per pass as fit the free device memory (a 10 000-read result at 8 mismatches is
 * 1.6e9 rows = 104 GB) - and, if packed_host is not NULL, copied to the host pass by pass; with neither
 * destination the rows are computed and dropped (timing runs).  mit_host (optional) receives the MIT scores.
 * vsc_unpack_features expands rows to the dense 442-byte form of vsc_score_hits.
 */
int vsc_score_hits_packed(vsc_ctx *ctx, const vsc_genome *genome, const vsc_hits *hits, const uint64_t *guides,
                          uint32_t n_guides, uint64_t first, uint64_t count, void *packed_dev, uint32_t *packed_host,
                          double *mit_host);
#define VSC_PACKED_FEATURE_BYTES 64
void vsc_unpack_features(const uint32_t *packed, uint64_t n, uint8_t *features);
/*
 * The same scores for n explicit (on-target, off-target) pairs: both 23-mers as vsc_pack_guide codes
 * in read orientation, masks[i] = the mismatch positions calcMitScore is given for row i (bit p =
 * position p).  This is the form the mergers need: they score what they re-derived from the SAM
 * records (variant_processing/merge_output_bam.h:156,187,389,437,549,696), where the positions
 * come from the MD tag (filter_output_bam.h:330-349) and the sequences from the FASTA (:399,484).
 */
int vsc_score_pairs(vsc_ctx *ctx, const uint64_t *on_targets, const uint64_t *off_targets, const uint32_t *masks,
                    uint64_t n, double *mit, uint8_t *mit_flags, uint8_t *features);

/* ---- several devices of one node ----------------------------------------------------------------------- */
/*
 * The genome-sharded search of one host process over n devices (BASELINE north star: "partitioned across
 * the 8 GPUs of one node by genome shard with a single RCCL gather of candidate hits"): one vsc_ctx per
 * entry of device_ids, the planes cut into n tile-aligned position ranges (+ a one-word halo; a window
 * belongs to the shard that holds its first base), every device searching ALL reads on its shard from its own
 * host thread, then one exchange - the records (8-byte exchange records, vsc_hits_pack_exchange) by one grouped
 * ncclSend / ncclRecv per shard to the first device, over xGMI (the counts are known inside the process) - and
 * vsc_hits_merge_packed there.  The result is an
 * ordinary vsc_hits of a context on the first device (vsc_multi_result_ctx(m)): same records, same order as one device gives.
 * This replaces, inside the bidir_mapping process, the OpenMP loop over reads and the concatenation of the
 * per-thread output buffers (read_mapping/bidir_mapping.cpp:285-295,307-308): the parallel axis is the genome.
 * RCCL is bound at run time (dlopen) and used when n > 1 distinct devices are given; device ids may repeat
 * (several contexts on one GPU: tests and rehearsals on a one-GPU box) - the exchange then is device copies.
 * vsc_multi_last_error after vsc_multi_create says why copies are in use when RCCL could not be set up.
 */
typedef struct vsc_multi vsc_multi;
typedef struct vsc_multi_genome vsc_multi_genome;
typedef struct {
    double search_wall_ms;   /* host wall time until the slowest shard had searched (+ scored) and packed its last batch */
    double search_ms_max;    /* largest sum of vsc_timing.total_ms among the shards */
    double exchange_ms;      /* host wall time the exchange took beyond the searches: from the moment the last shard of a batch was
                                ready until that batch's records had arrived on the first device (summed over the batches) */
    double merge_ms;         /* vsc_hits_merge_packed on the first device (host wall, summed over the batches) */
    double total_ms;
    uint64_t hits;
    uint64_t exchanged_bytes; /* record (+ vote) bytes that crossed between devices */
    uint32_t n_devices;
    uint32_t used_rccl;      /* 1: RCCL carried the exchange, 0: device copies */
    double score_ms_max;     /* largest sum of the shards' scoring kernels (vsc_timing.score_ms) */
    double callback_ms;      /* host wall time inside on_batch (summed) */
    uint32_t batches;        /* batches the reads were searched in (vsc_multi_search: 1) */
    uint32_t reserved;
} vsc_multi_timing;
int vsc_multi_create(const int *device_ids, int n, vsc_multi **out);
int vsc_multi_destroy(vsc_multi *m);
/* vsc_ctx_release_scratch on every context of the set + the pooled exchange buffers (they stay allocated between searches). */
int vsc_multi_release_scratch(vsc_multi *m);
int vsc_multi_size(const vsc_multi *m);
vsc_ctx *vsc_multi_ctx(vsc_multi *m, int i);  /* the i-th shard's context */
/* The context on the first device that owns the merged results (its own stream: a batch is merged there while the shards -
 * the first device's among them - search the next one). */
vsc_ctx *vsc_multi_result_ctx(vsc_multi *m);
const char *vsc_multi_last_error(const vsc_multi *m);
int vsc_multi_uses_rccl(const vsc_multi *m);
int vsc_multi_get_timing(const vsc_multi *m, vsc_multi_timing *out);
/* hi / lo / nmask: the WHOLE genome's planes (n_words words each); every device receives its shard. */
int vsc_multi_genome_load(vsc_multi *m, const uint32_t *hi, const uint32_t *lo, const uint32_t *nmask, uint64_t n_words,
                          const vsc_contig *contigs, uint32_t n_contigs, vsc_multi_genome **out);
int vsc_multi_genome_free(vsc_multi_genome *g);
int vsc_multi_genome_build_index(vsc_multi *m, vsc_multi_genome *g, const vsc_search_params *params);
/* as vsc_search; *out belongs to vsc_multi_result_ctx(m) and is released with vsc_hits_free.  A shard's records leave for
 * the first device as soon as THAT shard is done (they do not wait for the slowest one). */
int vsc_multi_search(vsc_multi *m, const vsc_multi_genome *g, const uint64_t *guides, uint32_t n_guides,
                     const vsc_search_params *params, vsc_hits **out);
/* vsc_search_summary over the device set: every shard summarises its own windows on its own context (from its own host
 * thread, as vsc_multi_search), and the rows are added on the host (on_target: OR over the shards).  No record moves
 * between devices. */
int vsc_multi_search_summary(vsc_multi *m, const vsc_multi_genome *g, const uint64_t *guides, uint32_t n_guides,
                             const vsc_search_params *params, const vsc_locus *exclude, vsc_guide_summary *out);
/* vsc_search_select over the device set: every shard selects among its own windows on its own context (from its own host
 * thread); selection composes over shards, so with top_k > 0 the <= shards x top_k survivors per guide and their scores
 * (vsc_score_hits on the shard's result) go to the host, are cut per guide to top_k in the same order, and the surviving
 * records go in shard order through vsc_hits_merge on vsc_multi_result_ctx(m) - no RCCL leg; with top_k = 0 there is
 * nothing to cut and the survivors can be many: they take vsc_multi_search's packed exchange and merge.  summary rows are
 * added over the shards as vsc_multi_search_summary adds them. */
int vsc_multi_search_select(vsc_multi *m, const vsc_multi_genome *g, const uint64_t *guides, uint32_t n_guides,
                            const vsc_search_params *params, const vsc_select *select, const vsc_locus *exclude,
                            vsc_guide_summary *summary, vsc_hits **out);
/* vsc_search_summary_regions / vsc_search_select_regions over the device set: the two calls above with the extra arguments
 * handed to every shard (the regions are global, every context uploads its own copy on first use); out_in / summary_in are
 * added on the host as the other rows are. */
int vsc_multi_search_summary_regions(vsc_multi *m, const vsc_multi_genome *g, const uint64_t *guides, uint32_t n_guides,
                                     const vsc_search_params *params, const vsc_locus *exclude, const vsc_regions *regions,
                                     vsc_guide_summary *out_all, vsc_guide_summary *out_in);
int vsc_multi_search_select_regions(vsc_multi *m, const vsc_multi_genome *g, const uint64_t *guides, uint32_t n_guides,
                                    const vsc_search_params *params, const vsc_select *select, const vsc_region_filter *filter,
                                    const vsc_locus *exclude, vsc_guide_summary *summary_all, vsc_guide_summary *summary_in,
                                    vsc_hits **out);
/* vsc_guides_enumerate over the device set: every shard enumerates the windows that start in its own words on its own context
 * and host thread (as vsc_multi_search_summary does); shards partition the positions in ascending order, so the shards' arrays
 * concatenated in shard order on the host ARE the whole genome's result.  *out is a host-only object (vsc_guides_data_dev
 * gives NULL), released with vsc_guides_free.  max_guides holds for the total (a shard that exceeds it alone ends the call
 * early; vsc_multi_last_error then names that shard's count). */
int vsc_multi_guides_enumerate(vsc_multi *m, const vsc_multi_genome *g, const vsc_regions *regions,
                               const vsc_enum_params *params, vsc_guides **out);
/* (vsc_multi_search_stream, which scores on the owning shard, is declared behind the classifier below.) */

/* ---- variant windows (row R8) ------------------------------------------------------------------- */
/*
 * The alt-allele windows of one sample column of a VCF ("SNP genome"), built straight into packed planes:
 * what `vcf_loader FILE.vcf SNP.fa GENOME.fa SAMPLE SEQLENGTH THREADS` followed by `bidir_index -G SNP.fa`
 * produce (variant_processing/vcf_loader.cpp:40-68, process_vcf.h:54-269, overlap_sequences.h:35-240,
 * write_fasta.h:30-470; VARSCOT:296-307) - same windows, same order, same ids, planes byte-identical -
 * without the FASTA text in between.  Reference segments are copied bit-wise from the reference planes
 * hi / lo / nmask (whole genome, host memory; contigs / contig_names describe it, a chromosome is found by
 * the first word of its name as with an FAI index) instead of per-segment FAI reads (write_fasta.h:245-271);
 * parsing, sweep and window assembly run on `threads` host threads (0 = all).  Host-only, no device needed.
 * The result is a genome like any other: vsc_genome_load(planes, contigs) + vsc_search.  One call per sample
 * column replaces one run of the reference pipeline per sample (parallel.py:49-63); the reference genome and
 * its search are shared between the samples.
 * err (optional, err_len bytes) receives the text of a failure.
 */
typedef struct vsc_windows vsc_windows;
int vsc_windows_build(const char *vcf_path, uint32_t sample, uint32_t seq_len, uint32_t threads, const uint32_t *hi,
                      const uint32_t *lo, const uint32_t *nmask, const vsc_contig *contigs, const char *const *contig_names,
                      uint32_t n_contigs, vsc_windows **out, char *err, size_t err_len);
uint32_t vsc_windows_count(const vsc_windows *w);            /* windows = contigs of the SNP genome */
uint64_t vsc_windows_words(const vsc_windows *w);            /* 32-bit words per plane */
const uint32_t *vsc_windows_plane(const vsc_windows *w, int which); /* 0 hi, 1 lo, 2 nmask */
const vsc_contig *vsc_windows_contigs(const vsc_windows *w);
/* id of window i (chr_start_REF / chr_start_ALT_pos_ref_alt..., write_fasta.h:30-65); not NUL-terminated */
const char *vsc_windows_name(const vsc_windows *w, uint32_t i, uint32_t *len);
/* count + 1 offsets into the id pool that starts at vsc_windows_name(w, 0, NULL); every id is followed by '\n' */
const uint64_t *vsc_windows_name_offsets(const vsc_windows *w);
void vsc_windows_free(vsc_windows *w);

/* ---- variant-aware screen: the window side of the mergers on the device ------------------------------ */
/*
 * A hit of the window-genome search is a hit IN A WINDOW; the mergers turn it into a hit of the individual's genome
 * (variant_processing/filter_output_bam.h:279-317 filterSnpAlignment, :189-263 getSnpType): with id = the window's id split on
 * '_', chr = id[0] and pos1 = pos + (uint32) atoi(id[1]) (32-bit wrap; a negative start and a non-numeric field are legal; a
 * chromosome name that holds '_' is cut at it and its fields shift, as in the reference), the triples (id[k], id[k+1], id[k+2]),
 * k = 3, 6, ..., are the window's variants: position p = atoi(id[k]), lengths of the ref and the alt allele.  A variant is
 * COVERED by [pos1, pos1 + 23) if p lies in it (equal lengths) or p + 1 or p + max(len) - 1 does (an indel: only its two end
 * points are tested); an uncovered indel met before the first covered variant moves the position by len_ref - len_alt;
 * pos2 = pos1 + that sum.  The tag is REF if nothing is covered, else VAR_<chr>_<id[k] of the covered ones, comma separated>.
 * key = (guide, chr, pos2, strand, the window's 23 bases, mismatch mask, tag).  Record i of a result in vsc_search order is
 *   the ON-TARGET  iff exclude[guide] names a locus and chr is that contig, pos2 its position, the strands agree, NM = 0 and the
 *                  tag is REF (the caller's contract, as for vsc_search_summary: exclude[i] is the locus guide i was taken from);
 *   a DUPLICATE    iff i > 0 and key_i == key_(i-1) - the record before it, whatever that one's fate; duplicates that are not
 *                  neighbours are kept, as in the reference (:303-306);
 *   COUNTED        iff it is neither.
 * vsc_variant_map (host only, immutable, usable from several threads, like vsc_regions): every id parsed once into the reference
 * contig (found by the first word of the contig's name, as an FAI index does; UINT32_MAX if unknown - such hits are counted and
 * can never be the on-target), the start, and a flat table of (p, len_ref, len_alt, tag_id) per variant, tag_id numbering the
 * distinct (id[0], id[k]) strings so that tags compare as integers.
 * vsc_variant_map_build: ids / id_offsets = the id pool and the n_windows + 1 offsets exactly as vsc_windows_name(w, 0, NULL) and
 * vsc_windows_name_offsets return them (id i = bytes [off[i], off[i+1] - 1), a separator byte behind every id);
 * window_contigs = the window genome's table; ref_contigs / ref_names = the reference's.  n_windows == 0 is valid.  A null
 * argument that is needed or offsets that do not ascend: VSC_ERR_INVALID.
 */
typedef struct vsc_variant_map vsc_variant_map;
typedef struct {
    uint64_t windows;       /* windows of the map */
    uint64_t variants;      /* (window, variant) entries of the flat table */
    uint64_t unknown_chr;   /* windows whose chromosome is not a contig of the reference */
    uint32_t max_variants;  /* most variants in one window */
    uint32_t reserved;
} vsc_variant_map_stats;
typedef struct {
    uint32_t contig; /* reference contig of chr, UINT32_MAX: unknown */
    uint32_t pos;    /* pos2 */
    uint32_t n_var;  /* covered variants (0: the tag is REF) */
    uint32_t flags;  /* VSC_VARIANT_* */
} vsc_variant_label;
#ifdef __cplusplus
static_assert(sizeof(vsc_variant_label) == 16, "vsc_variant_label layout");
#else
_Static_assert(sizeof(vsc_variant_label) == 16, "vsc_variant_label layout");
#endif
#define VSC_VARIANT_VAR 1u       /* the tag is not REF */
#define VSC_VARIANT_DUP 2u       /* dropped: the same key as the record before it */
#define VSC_VARIANT_ON_TARGET 4u /* dropped: the guide's own locus */
int vsc_variant_map_build(const char *ids, const uint64_t *id_offsets, const vsc_contig *window_contigs, uint32_t n_windows,
                          const vsc_contig *ref_contigs, const char *const *ref_names, uint32_t n_ref_contigs,
                          vsc_variant_map **out);
void vsc_variant_map_free(vsc_variant_map *map);
int vsc_variant_map_info(const vsc_variant_map *map, vsc_variant_map_stats *out);
/* The INSIDE-rule regions of filterRefAlignment (variant_processing/filter_output_bam.h:70-124) over the reference's contig
 * table: one interval [start, start + window length) per window with a known chromosome and start >= 0 (`pos >= atoi(start)`
 * compares unsigned with int there: a negative start shadows nothing).  vsc_search_summary_regions' out_all - out_in and
 * vsc_search_select_regions with VSC_REGION_DROP under these regions are the reference side of the merge.  Released with
 * vsc_regions_free. */
int vsc_variant_map_shadow(const vsc_variant_map *map, vsc_regions **out);
/* The host's answer for the window position (window, pos): contig, pos2, n_var and VSC_VARIANT_VAR (never DUP / ON_TARGET: those
 * need the records).  window >= the map's windows or a null argument: VSC_ERR_INVALID. */
int vsc_variant_map_locate(const vsc_variant_map *map, uint32_t window, uint32_t pos, vsc_variant_label *label);
/* The tag text of (window, pos) - "REF" or "VAR_<chr>_<positions>" - into buf (NUL-terminated, cut at len - 1); returns the
 * text's full length, or a negative status. */
int64_t vsc_variant_map_tag(const vsc_variant_map *map, uint32_t window, uint32_t pos, char *buf, size_t len);
/*
 * labels[i] = the label of record i of `hits`, a result of a search of win_genome (any vsc_search* result in vsc_search order,
 * on the hits' own context, which must be win_genome's), flags included; exclude: NULL or n_guides loci IN REFERENCE
 * COORDINATES (contig >= the reference's contig count and not UINT32_MAX, or strand > 1: VSC_ERR_INVALID).  One kernel over the
 * records where they lie (variant_merge_kernel: the window's table entry, a walk over the window's variants, the key compared
 * with the neighbour's - cheap fields, covered tag ids in lockstep, the 23 bases of both windows from the resident planes);
 * the map's device copy is kept by the context (given back by vsc_ctx_release_scratch).  labels: host memory, vsc_hits_count
 * entries.  A map whose window count or lengths differ from win_genome's contig table, a record whose contig or position lies
 * outside the map, a record guide >= n_guides when exclude is given, or a null argument: VSC_ERR_INVALID.  n == 0: VSC_OK,
 * nothing is launched.  vsc_ctx_timing is left as it is.
 * Replaces: filterSnpAlignment + getSnpType per record on the host (variant_processing/filter_output_bam.h:189-317).
 */
int vsc_hits_variants(vsc_hits *hits, const vsc_genome *win_genome, const vsc_variant_map *map, const vsc_locus *exclude,
                      uint32_t n_guides, vsc_variant_label *labels);
/*
 * The screen: per guide the summary of the COUNTED window hits, without the records.  out_all = over all counted records,
 * out_var (optional) = over those whose tag is not REF, fields as vsc_search_summary computes them (nm by popcount of the
 * mask, mit_sum += rint(MIT * 2^24), mit_ub); on_target = 1 in both rows if the on-target was met in a window;
 * duplicates (optional) = dropped duplicates per guide (every record flagged VSC_VARIANT_DUP).  The guides are searched in batches of batch_reads (0 or more than
 * 16 384: 16 384) as vsc_search_stream searches them; every batch's sorted records are summarised where they lie and let go:
 * no record leaves the device.  Batches end on guide boundaries, so the neighbour rule needs nothing across them and the rows
 * do not depend on batch_reads.  The guide's rows in the individual's genome = (out_all - out_in of vsc_search_summary_regions
 * on the reference under vsc_variant_map_shadow's regions) + out_all of this call, field by field: the per-guide aggregation of
 * the rows mergeResults prints (variant_processing/merge_output_bam.h:46-215).
 * vsc_ctx_timing afterwards reports as after vsc_search (sums over the batches), the merge kernel in finalize_ms.
 * Replaces, for a screen: bidir_mapping on the SNP genome + filterSnpAlignment / getSnpType + the MIT scores of the merger.
 */
int vsc_search_summary_variants(vsc_ctx *ctx, const vsc_genome *win_genome, const vsc_variant_map *map, const uint64_t *guides,
                                uint32_t n_guides, const vsc_search_params *params, const vsc_locus *exclude, uint32_t batch_reads,
                                vsc_guide_summary *out_all, vsc_guide_summary *out_var /* optional */,
                                uint64_t *duplicates /* optional */);

/* ---- classifier ---------------------------------------------------------------------------------- */
/*
 * A trained random forest as randomForest stores it ($forest of the object in
 * classification/rfClassifier.RData), numeric splits only, two classes ("0", "1").  All arrays have
 * n_trees * n_nodes entries, tree-major.  feature[] = column of the dense feature row the node
 * tests (0..441, or 442 = the on-target activity).
 */
typedef struct {
    uint32_t n_trees, n_nodes;
    const int8_t *node_status;  /* 1 = split node, -1 = terminal */
    const uint16_t *feature;
    const uint16_t *left, *right; /* 1-based daughter nodes */
    const double *split;        /* x <= split goes left */
    const uint8_t *node_class;  /* terminal nodes: 1 = class "0", 2 = class "1" */
} vsc_rf_model;
/*
 * predict(rfClassifier, featureMatrix[, type = "prob"]) of classification/classificationPipeline.R:27-34
 * for n feature rows (dense 442-byte rows as vsc_score_hits / vsc_score_pairs produce them, plus the
 * on-target activity of each row): prob = share of trees voting class "1", cls = 1 if that share is
 * above one half, tie = 1 where the vote is exactly split (R breaks such ties at random).
 */
int vsc_rf_predict(vsc_ctx *ctx, const vsc_rf_model *model, const uint8_t *features, const double *activity, uint64_t n,
                   double *prob, uint8_t *cls, uint8_t *tie);
/* The same for rows in the packed 64-byte form of vsc_score_hits_packed (host memory, or device memory when
 * rows_on_device != 0 - e.g. the buffer vsc_score_hits_packed has just filled): the columns the forest tests
 * are decoded on the device, the 442-byte rows never exist. */
int vsc_rf_predict_packed(vsc_ctx *ctx, const vsc_rf_model *model, const void *packed_rows, int rows_on_device,
                          const double *activity, uint64_t n, double *prob, uint8_t *cls, uint8_t *tie);

/*
 * Score -> classify in one kernel, for results whose feature rows should never exist in memory (100 000 reads at 8
 * mismatches are 1.6e10 hits = 1 TB of packed rows): for rows [first, first + count) of a search result the kernel
 * computes the hit's feature row in registers (as vsc_score_hits_packed would write it), walks the forest and writes
 * the number of trees voting class "1" - 2 bytes per hit (prob = votes / n_trees, class = 2 * votes > n_trees,
 * tie = 2 * votes == n_trees), and optionally the MIT score.  guide_activity[g] = the on-target activity of read g
 * (the column classification/classificationPipeline.R:21-25 reads from the feature file, constant per target;
 * variant_processing/merge_output_bam.h:401,708 appends it to every row).  Identical, hit for hit, to
 * vsc_score_hits_packed followed by vsc_rf_predict_packed.  votes_dev (device, count * 2 bytes) and votes_host are
 * optional destinations; with neither the votes stay in library scratch (timing runs).
 * Replaces, for a streamed search: variant_processing/merge_output_bam.h:696-708 (feature rows as text) +
 * classification/classificationPipeline.R:21-49 (read them back, predict).
 */
int vsc_score_classify_hits(vsc_ctx *ctx, const vsc_genome *genome, const vsc_hits *hits, const uint64_t *guides, uint32_t n_guides,
                            const double *guide_activity, const vsc_rf_model *model, uint64_t first, uint64_t count, void *votes_dev,
                            uint16_t *votes_host, double *mit_host);

/*
 * Per-guide summary and selection BY THE CLASSIFIER: how many of a guide's off-targets does the forest call active, and which
 * are its most probably active sites - without the records.  votes(h) is the number vsc_score_classify_hits writes for hit h
 * for the same genome, guides, guide_activity and model (trees voting class "1"; the row from the guide and the site's 23 bases
 * in read orientation, the activity that of the hit's guide).  The counted hits of guide i are exactly those of
 * vsc_search_summary: the hits vsc_search returns, minus the one at exclude[i] if it is a hit.  Over them:
 *   votes_sum     sum of votes(h): the expected number of active off-targets * n_trees
 *   active        hits with 2 * votes >  n_trees (class "1")
 *   ties          hits with 2 * votes == n_trees
 *   active_nm[k]  the active ones with NM = k
 * Every field is a sum of integers: independent of the order of the records, exact when passes or genome shards are added.
 * The forest is walked over the search kernel's records where they lie (one word of votes beside every record slot); the
 * rows and the selection are taken from those words: no sort of all hits, no 16-byte records, no votes leave the device.
 * Selection (vsc_select_votes): of the counted hits with votes >= min_votes (0: no floor) the first top_k (0: no limit) in
 * the total order votes descending, strand '+' before '-', global position ascending - vsc_search_select's tie-break.  The
 * result is an ordinary vsc_hits sorted as vsc_search sorts it that holds the survivors only; their votes are what
 * vsc_score_classify_hits gives on that (small) result.  Selection composes over genome shards as vsc_search_select's does.
 * cls, cls->model, cls->guide_activity (n_guides > 0) or select NULL, a non-zero reserved field, a model of 0 trees or of
 * more than the 16-bit votes hold (65 535), an excluded locus vsc_search_summary refuses: VSC_ERR_INVALID.  n_guides == 0:
 * VSC_OK, nothing is launched.  out (optional) / summary (optional): the rows vsc_search_summary writes, from the same search.
 * vsc_ctx_timing afterwards: as after vsc_search_summary / vsc_search_select, with score_ms = the classify kernel (in neither
 * sort_ms nor finalize_ms); hits = all hits found.
 * Replaces, for a screen: variant_processing/merge_output_bam.h:696-708 (feature rows as text) +
 * classification/classificationPipeline.R:21-49 (read them back, predict) + a per-guide aggregate of the predictions.
 */
typedef struct {
    uint64_t votes_sum;     /* sum of votes(h) over the counted hits: expected active off-targets * n_trees */
    uint64_t active;        /* counted hits with 2 * votes >  n_trees  (class "1") */
    uint64_t ties;          /* counted hits with 2 * votes == n_trees */
    uint64_t active_nm[9];  /* the active ones by NM */
} vsc_guide_votes;
#ifdef __cplusplus
static_assert(sizeof(vsc_guide_votes) == 96, "vsc_guide_votes layout");
#else
_Static_assert(sizeof(vsc_guide_votes) == 96, "vsc_guide_votes layout");
#endif
typedef struct {
    uint32_t top_k;      /* hits kept per guide, best first by (votes desc, strand, position); 0 = no limit */
    uint32_t min_votes;  /* keep hits with votes >= min_votes; 0 = no floor */
    uint32_t reserved[2];
} vsc_select_votes;
typedef struct {
    const vsc_rf_model *model;     /* the forest */
    const double *guide_activity;  /* on-target activity per read (n_guides values) */
    uint32_t reserved[2];
} vsc_classify;
int vsc_search_summary_classified(vsc_ctx *ctx, const vsc_genome *genome, const uint64_t *guides, uint32_t n_guides,
                                  const vsc_search_params *params, const vsc_locus *exclude, const vsc_classify *cls,
                                  vsc_guide_summary *out /* optional */, vsc_guide_votes *out_votes);
int vsc_search_select_classified(vsc_ctx *ctx, const vsc_genome *genome, const uint64_t *guides, uint32_t n_guides,
                                 const vsc_search_params *params, const vsc_select_votes *select, const vsc_classify *cls,
                                 const vsc_locus *exclude, vsc_guide_summary *summary /* optional */,
                                 vsc_guide_votes *votes_rows /* optional */, vsc_hits **out);
/* vsc_search_summary_classified over the device set: every shard summarises its own windows on its own context, the rows are
 * added on the host (as vsc_multi_search_summary adds them).  (Selection by votes over several devices is not offered: the
 * re-selection on the result device would need the votes of merged records, which no shard holds there.) */
int vsc_multi_search_summary_classified(vsc_multi *m, const vsc_multi_genome *g, const uint64_t *guides, uint32_t n_guides,
                                        const vsc_search_params *params, const vsc_locus *exclude, const vsc_classify *cls,
                                        vsc_guide_summary *out /* optional */, vsc_guide_votes *out_votes);

/* ---- table-driven off-target scores (CFD form): per hit, per guide, top-K ------------------------------------ */
/*
 * A score that is a product of weights looked up by (read position, guide base, site base) times a weight for the site's PAM
 * dinucleotide - the form of the CFD score.  The library ships no table: the caller brings one (vsc_score_table_build).
 *
 * TABLE   pair[20][4][4] and pam[16], doubles.
 *         pair[j][g][s] is the weight of guide base g against site base s at read position j.
 *           j = 0 is the PAM-distal end.
 *           Bases are coded A 0, C 1, G 2, T 3, as vsc_pack_guide codes them.
 *           s is the letter of the site in READ orientation. This is the letter CRISPOR's offtargetSeq column shows.
 *         pam[4 * s21 + s22] is the weight of the site's letters at read positions 21 and 22.
 *         Every weight is finite and lies in [0, 1]. pair[j][b][b] is exactly 1.
 *         Anything else: VSC_ERR_INVALID.
 * SCORE   For a hit with read r and site s in read orientation:
 *           s = w on '+', revcomp(w) on '-', where w is the 23-base window.
 *           x = 1.0.
 *           For j = 0, 1, ..., 19 in this order: if r[j] != s[j] then x = x * pair[j][r[j]][s[j]].
 *           Then x = x * pam[s[21], s[22]].
 *         Arithmetic is fp64, one rounding per multiplication, no contraction.
 *         Positions 20..22 of the read and bits 20..22 of the mismatch mask take no part.
 *         On '-' the record's mask bit i is read position 22 - i.
 * FIXED   f = rint(x * 2^30), round half to even. f <= 2^30.
 *         This is the unit of every sum, floor and selection key. It is exact under any order, pass split or shard split.
 * HITS    Exactly the hits of vsc_search / vsc_search_summary for the same genome, guides and params, minus exclude[i].
 *         A site whose PAM is not in the search's PAM set is not a hit, whatever pam[] says.
 *         extra_pam is how NAG sites get in.
 * ROWS    vsc_guide_table_row { uint64_t score_sum, positive, positive_nm[9], reserved; }, 96 bytes.
 *         It is vsc_guide_votes' shape, so the sinks' LDS table and add_shard_rows serve it.
 *         positive counts the hits with f > 0.
 *         positive_nm[k] counts those with NM = k.
 * SPEC    vsc_table_specificity(sum) = 100.0 / (100.0 + sum * 2^-30) * 100.0, evaluated in that order.
 *         The tools round it with floor(x + 0.5), as they do for MIT.
 *
 * vsc_score_table is host-only and immutable; a context keeps the device copy of the table it used last (keyed by the table's
 * serial number) and vsc_ctx_release_scratch gives it back.  vsc_table_score scores one (guide, site) pair on the host - both
 * vsc_pack_guide codes in read orientation - with the very function the kernels call.  vsc_score_hits_table scores rows
 * [first, first + count) of a sorted result (either output may be NULL; the row range and the pass-wise scratch of
 * vsc_score_hits; a record that is no hit of this genome and these guides - its window outside the genome's planes, its guide
 * index >= n_guides - scores 0, as no result of the library's searches over them does).  vsc_search_summary_table writes one row per guide (plain: the rows of vsc_search_summary from the same
 * search, optional).  vsc_search_select_table is vsc_search_select with the key f: min_score is in f units, the order is f
 * descending, '+' before '-', global position ascending, the result is sorted as vsc_search sorts; with top_k = 0,
 * min_score = 0 and no exclude it returns vsc_search's bytes.  vsc_multi_search_summary_table adds the shards' rows on the
 * host.  Multi-device selection by table score is not offered (as for votes), nor a call with a table and the classifier at
 * once.  vsc_ctx_timing afterwards: score_ms = the table score kernel.
 */
typedef struct vsc_score_table vsc_score_table;
typedef struct {
    uint64_t score_sum;       /* sum of f over the counted hits */
    uint64_t positive;        /* counted hits with f > 0 */
    uint64_t positive_nm[9];  /* those by NM */
    uint64_t reserved;        /* 0 */
} vsc_guide_table_row;
#ifdef __cplusplus
static_assert(sizeof(vsc_guide_table_row) == 96, "vsc_guide_table_row layout");
#else
_Static_assert(sizeof(vsc_guide_table_row) == 96, "vsc_guide_table_row layout");
#endif
typedef struct {
    uint64_t serial;        /* process-wide number of the table */
    uint32_t zero_weights;  /* weights that are exactly 0 */
    uint32_t reserved;
} vsc_score_table_stats;
int vsc_score_table_build(const double *pair /* [20][4][4] */, const double *pam /* [16] */, vsc_score_table **out);
int vsc_score_table_free(vsc_score_table *table);
int vsc_score_table_info(const vsc_score_table *table, vsc_score_table_stats *out);
int vsc_table_score(const vsc_score_table *table, uint64_t guide_code, uint64_t site_code, double *score /* optional */,
                    uint32_t *fixed /* optional */);
double vsc_table_specificity(uint64_t score_sum);
int vsc_score_hits_table(vsc_ctx *ctx, const vsc_genome *genome, const vsc_hits *hits, const uint64_t *guides, uint32_t n_guides,
                         uint64_t first, uint64_t count, const vsc_score_table *table, double *scores /* optional */,
                         uint32_t *fixed /* optional */);
int vsc_search_summary_table(vsc_ctx *ctx, const vsc_genome *genome, const uint64_t *guides, uint32_t n_guides,
                             const vsc_search_params *params, const vsc_locus *exclude, const vsc_score_table *table,
                             vsc_guide_summary *plain /* optional */, vsc_guide_table_row *out);
int vsc_search_select_table(vsc_ctx *ctx, const vsc_genome *genome, const uint64_t *guides, uint32_t n_guides,
                            const vsc_search_params *params, const vsc_select *select, const vsc_locus *exclude,
                            const vsc_score_table *table, vsc_guide_table_row *rows /* optional */, vsc_hits **out);
int vsc_multi_search_summary_table(vsc_multi *m, const vsc_multi_genome *g, const uint64_t *guides, uint32_t n_guides,
                                   const vsc_search_params *params, const vsc_locus *exclude, const vsc_score_table *table,
                                   vsc_guide_summary *plain /* optional */, vsc_guide_table_row *out);

/* ---- table scores for pattern hits: per hit, per guide, floor and top-K --------------------------------------- */
/*
 * The score above for any nuclease: a product of weights by (protospacer position, guide base, site base) times a weight for
 * the site's letters at up to four PAM positions, over the hits of vsc_search_pattern.  The library ships no table.
 *
 * TABLE   vsc_pattern_table, host-only and immutable, with a process-wide serial number like vsc_score_table.
 *         Shape: { len L (16..32), ps_start, ps_len (ps_len >= 1, ps_start + ps_len <= L), n_pam (0..4), pam_pos[4] }.
 *         pam_pos[0..n_pam) are read positions, strictly ascending, all below L and outside [ps_start, ps_start + ps_len).
 *         Weights: pair[ps_len][4][4] and pam[4^n_pam], doubles.
 *         pair[i][g][s] is the weight of guide base g against site base s at read position ps_start + i.
 *           Bases are A 0, C 1, G 2, T 3.
 *           s is the site's letter in READ orientation, that is pattern orientation.
 *         pam[k] has k = sum over t of s[pam_pos[t]] * 4^(n_pam - 1 - t).  With n_pam = 0 there is one weight, pam[0].
 *         Every weight is finite and lies in [0, 1]. pair[i][b][b] is exactly 1.
 *         Anything else, or a bad shape: VSC_ERR_INVALID.
 * SCORE   For a hit of guide G at a site with s in read orientation (w on '+', revcomp(w) on '-'):
 *           x = 1.0.
 *           For i = 0 .. ps_len - 1 in this order, with j = ps_start + i:
 *             if G[j] is one of A, C, G, T and s[j] != G[j] then x = x * pair[i][G[j]][s[j]].
 *           Then x = x * pam[k].
 *         Arithmetic is fp64, one rounding per multiplication, no contraction.
 *         A protospacer position whose guide letter is degenerate (N or any other IUPAC set) takes no part, even where it
 *         counts as a mismatch in NM.  Guide letters outside the protospacer take no part.
 * FIXED   f = rint(x * 2^30), round half to even. f <= 2^30.  The unit of every sum, floor and selection key, as above.
 * HITS    Exactly the hits of vsc_search_pattern for the same planes, pattern, guides and params.
 *         A table whose len is not the call's len: VSC_ERR_INVALID.
 * ROWS    vsc_guide_table_row per guide: score_sum, positive (hits with f > 0) and positive_nm[NM] over ALL hits, before any
 *         selection.  vsc_table_specificity applies to score_sum as it does above.
 * SELECT  vsc_pattern_select { top_k, min_score, reserved[2] }.
 *         Per guide, the survivors are the hits with f >= min_score.
 *         Of those, the first top_k (0: all) are kept under the ranking f descending, then strand, contig, pos ascending.
 *         The result stays in record order (guide, strand, contig, pos). One uint32_t f per record runs parallel to the records.
 *         With select == NULL or { 0, 0 } the records are vsc_search_pattern's bytes.
 *         max_hits caps the RETURNED records: the survivors.  When there are more, the call returns VSC_ERR_RANGE,
 *         vsc_last_error names their count and nothing is returned.
 * SHARDS  Rows of shards add: they are integers.  Records and f words of shards merge by record order.  Top-K across shards
 *         is the caller's re-cut and is not offered here.
 * ANCHOR  With L = 23, protospacer (0, 20), pam_pos = {21, 22} and a vsc_score_table's weights, f equals vsc_table_score's f
 *         bit for bit for every (guide, site).
 *
 * vsc_pattern_table_score scores one guide (len IUPAC letters) against one site (len letters of ACGT in read orientation; any
 * other letter: VSC_ERR_INVALID) on the host, with the very function the kernels call.  vsc_search_pattern_table takes
 * vsc_search_pattern's arguments and refusals, a table and an optional selection; out, rows (the NM rows) and table_rows may
 * each be NULL, all three NULL: VSC_ERR_INVALID.  A non-zero reserved field of select: VSC_ERR_INVALID.  out == NULL: no
 * record is allocated or written and select is not applied (the rows are over all hits in any case).  The score is taken in
 * the write pass, where the hit is found; the selection, when one is asked for, runs per round behind it.
 * vsc_pattern_hits_scores / _dev return the f words of a scored result (NULL / VSC_ERR_INVALID on a result of
 * vsc_search_pattern).  The context keeps the device copy of the table it used last, keyed by the serial number;
 * vsc_ctx_release_scratch gives it back.  vsc_ctx_timing afterwards: score_ms = the selection stage, the rest as after
 * vsc_search_pattern (scan_ms includes the scored write pass).
 */
typedef struct vsc_pattern_table vsc_pattern_table;
typedef struct {
    uint32_t len;        /* L, 16..32 */
    uint32_t ps_start;   /* the protospacer: read positions [ps_start, ps_start + ps_len) */
    uint32_t ps_len;
    uint32_t n_pam;      /* 0..4 */
    uint32_t pam_pos[4]; /* read positions of the PAM letters that the score looks at; unused entries 0 */
} vsc_pattern_table_shape;
typedef struct {
    uint64_t serial;        /* process-wide number of the table */
    uint32_t zero_weights;  /* weights that are exactly 0 */
    uint32_t reserved;
    vsc_pattern_table_shape shape;
} vsc_pattern_table_stats;
typedef struct {
    uint32_t top_k;      /* 0: all */
    uint32_t min_score;  /* in f units */
    uint32_t reserved[2];
} vsc_pattern_select;
#ifdef __cplusplus
static_assert(sizeof(vsc_pattern_table_shape) == 32, "vsc_pattern_table_shape layout");
static_assert(sizeof(vsc_pattern_table_stats) == 48, "vsc_pattern_table_stats layout");
static_assert(sizeof(vsc_pattern_select) == 16, "vsc_pattern_select layout");
#else
_Static_assert(sizeof(vsc_pattern_table_shape) == 32, "vsc_pattern_table_shape layout");
_Static_assert(sizeof(vsc_pattern_table_stats) == 48, "vsc_pattern_table_stats layout");
_Static_assert(sizeof(vsc_pattern_select) == 16, "vsc_pattern_select layout");
#endif
int vsc_pattern_table_build(const vsc_pattern_table_shape *shape, const double *pair /* [ps_len][4][4] */,
                            const double *pam /* [4^n_pam] */, vsc_pattern_table **out);
int vsc_pattern_table_free(vsc_pattern_table *table);
int vsc_pattern_table_info(const vsc_pattern_table *table, vsc_pattern_table_stats *out);
int vsc_pattern_table_score(const vsc_pattern_table *table, const char *guide, const char *site_text /* read orientation, len letters */,
                            double *score /* optional */, uint32_t *fixed /* optional */);
int vsc_search_pattern_table(vsc_ctx *ctx, const vsc_genome *genome, const char *pattern, const char *guides, uint32_t n_guides,
                             uint32_t len, const vsc_pattern_params *params, const vsc_pattern_table *table,
                             const vsc_pattern_select *select /* may be NULL */, vsc_pattern_hits **out /* may be NULL */,
                             vsc_pattern_summary *rows /* may be NULL */, vsc_guide_table_row *table_rows /* may be NULL */);
/* Host copy of the f words (made on first use; valid until vsc_pattern_hits_free). */
int vsc_pattern_hits_scores(vsc_pattern_hits *hits, const uint32_t **fixed);
/* Device pointer (valid until vsc_pattern_hits_free); NULL when the result is empty or not a scored one. */
const void *vsc_pattern_hits_scores_dev(const vsc_pattern_hits *hits);

/* ---- variant-aware pattern screen: any nuclease in an individual's genome ----------------------------- */
/*
 * The two mergers above for the records of vsc_search_pattern / vsc_search_pattern_table: sites of L = 16..32 bases, 20-byte
 * vsc_pattern_hit records, the windows built with seq_len = L (vsc_windows_build).  Everything above holds with 23 replaced by L.
 * WINDOW SIDE     Per record i of a pattern search of the window genome, in that search's order (guide, strand, contig, pos):
 *                 pos1 = pos + (uint32) start(window); a variant is COVERED by [pos1, pos1 + L) under the rule above; an uncovered
 *                 indel met before the first covered variant moves the position; pos2, n_var and the tag follow (getSnpType
 *                 with seq_len = L).  key = (guide, chr number, pos2, strand, the site's L bases from the window planes, info
 *                 word, mask word, tag ids).  The record is the ON-TARGET iff exclude[guide] names a locus, the window's
 *                 reference contig, pos2 and the strand equal it, NM = 0 and n_var = 0; a DUPLICATE iff i > 0 and its key equals
 *                 the key of record i - 1, whatever that record's own fate (the neighbour rule of the reference, kept on purpose);
 *                 COUNTED otherwise.  The pattern search has no right-edge rule: a site that ends at a window's last base IS a
 *                 hit here, although the plain search drops it - so at L = 23 the pattern records hold every record of the plain
 *                 search and, besides, such sites.
 * REFERENCE SIDE  A record of the same search of the reference genome is SHADOWED iff [pos, pos + L) lies fully inside one
 *                 interval of vsc_variant_map_shadow's set (filterRefAlignment with seq_len = L): with the intervals sorted by
 *                 start and end_max their running maximum, n = #{start <= pos}, inside iff n > 0 and end_max[n - 1] >= pos + L
 *                 (vsc_regions_contains answers for 23-base windows only).  It is the ON-TARGET iff its (contig, pos, strand)
 *                 equal exclude[guide] and NM = 0; COUNTED iff it is neither shadowed nor the on-target.
 * THE INDIVIDUAL  A guide's rows in the individual's genome = the reference side's counted rows + the window side's counted
 *                 rows, field by field.  All fields are integers.
 * ROWS            vsc_pattern_variant_row { count[NM], on_target, dropped }, 48 bytes: count = counted records by NM;
 *                 on_target = 1 if the on-target was met on that side; dropped = shadowed records (reference side), duplicates
 *                 (window side), 0 in the rows over the VAR records.  With a table: vsc_guide_table_row over the same counted
 *                 records (score_sum = the integer sum of their f words, positive, positive_nm).
 */
typedef struct {
    uint32_t count[VSC_MAX_MISMATCHES + 1];
    uint32_t on_target;
    uint64_t dropped;
} vsc_pattern_variant_row;
#ifdef __cplusplus
static_assert(sizeof(vsc_pattern_variant_row) == 48, "vsc_pattern_variant_row layout");
#else
_Static_assert(sizeof(vsc_pattern_variant_row) == 48, "vsc_pattern_variant_row layout");
#endif
#define VSC_PATTERN_REF_SHADOWED 1u  /* dropped: the site lies inside a window */
#define VSC_PATTERN_REF_ON_TARGET 2u /* dropped: the guide's own locus */
/* vsc_variant_map_locate / vsc_variant_map_tag for a site of len bases (16..32; len = 23: the same answers).  len outside
 * 16..32, window >= the map's windows or a null argument: VSC_ERR_INVALID. */
int vsc_variant_map_locate_len(const vsc_variant_map *map, uint32_t window, uint32_t pos, uint32_t len, vsc_variant_label *label);
int64_t vsc_variant_map_tag_len(const vsc_variant_map *map, uint32_t window, uint32_t pos, uint32_t len, char *buf, size_t buflen);
/* 1 if the len bases from pos of reference contig ref_contig on lie inside one shadow interval (REFERENCE SIDE above), else 0 -
 * also where no site of len bases starts (pos + len beyond the contig).  len outside 16..32, ref_contig >= the reference's
 * contigs or a null map: VSC_ERR_INVALID.  Replaces: the loop of filterRefAlignment (filter_output_bam.h:95-118) per record. */
int vsc_variant_map_shadows(const vsc_variant_map *map, uint32_t ref_contig, uint32_t pos, uint32_t len);
/*
 * labels[i] = the label of record i of `hits`, a result of vsc_search_pattern / vsc_search_pattern_table on win_genome (on the
 * hits' own context), flags included (WINDOW SIDE above); L = the length the hits were searched with.  exclude: NULL or
 * n_guides loci in reference coordinates.  One kernel over the records where they lie (pattern_variant_merge_kernel: the
 * records staged through LDS as coalesced words, the walk, the key compared with the neighbour's - cheap fields, covered tag ids
 * in lockstep, the L bases of both sites from the resident planes).  Refusals (VSC_ERR_INVALID, vsc_last_error names them): a map
 * whose window count or lengths differ from win_genome's contig table, a record outside the map or its window, a record guide
 * >= n_guides when exclude is given, an exclude contig >= the reference's contigs (and not UINT32_MAX) or strand > 1, a null
 * argument.  An empty result: VSC_OK, nothing is launched.  vsc_ctx_timing is left as it is.
 * Replaces: filterSnpAlignment + getSnpType per record on the host (variant_processing/filter_output_bam.h:189-317).
 */
int vsc_pattern_hits_variants(vsc_pattern_hits *hits, const vsc_genome *win_genome, const vsc_variant_map *map,
                              const vsc_locus *exclude, uint32_t n_guides, vsc_variant_label *labels);
/*
 * flags[i] = VSC_PATTERN_REF_SHADOWED | VSC_PATTERN_REF_ON_TARGET of record i of `hits`, a result of a pattern search of
 * ref_genome, the genome the map's reference contigs describe (REFERENCE SIDE above; pattern_shadow_kernel).  Refusals as above,
 * with a ref_genome whose contig table is not the map's reference in place of the window genome's.
 * Replaces: filterRefAlignment per record on the host (variant_processing/filter_output_bam.h:70-124).
 */
int vsc_pattern_hits_shadowed(vsc_pattern_hits *hits, const vsc_genome *ref_genome, const vsc_variant_map *map,
                              const vsc_locus *exclude, uint32_t n_guides, uint8_t *flags);
/*
 * The screen: both sides per guide, without the records.  ref_rows / win_rows = the rows over the counted records of either side
 * (dropped: the shadowed records / the duplicates), var_rows (optional) = over the window side's counted VAR records; with a
 * table (vsc_search_pattern_table's scores) ref_table / win_table / var_table = the table rows over the same records - without
 * a table the three must be NULL.  All outputs: host memory, n_guides entries.  The guides are searched in chunks of chunk_guides
 * (0 or more than 64: 64); each chunk is a whole (scored) pattern search per side under `params`, whose records stay on the
 * device, are consumed where they lie and are freed; max_hits caps a chunk's records per side.  Chunks end on guide boundaries,
 * so the rows depend neither on chunk_guides nor on guide_batch.  The map's device copy and the shadow arrays are kept by the
 * context, keyed by the map's serial (vsc_ctx_release_scratch gives them back).  Refusals as for the two calls above, and: a
 * table whose len is not `len`, table rows wanted without a table.  n_guides == 0: VSC_OK, nothing is launched.  A map without
 * windows (a sample without alt alleles; no genome can be loaded from it) takes win_genome == NULL: the reference side alone.
 * vsc_ctx_timing afterwards: the sums over the chunks' searches, the merge kernels in finalize_ms.
 * Replaces, for a screen: the searches' records on the host + filterRefAlignment + filterSnpAlignment / getSnpType + the
 * per-guide aggregation of the rows mergeResults prints (variant_processing/merge_output_bam.h:46-215).
 * Not provided: bulged alignments and cut sites in windows, the merged records as one sorted result, top-K in the individual.
 */
int vsc_search_pattern_variants(vsc_ctx *ctx, const vsc_genome *ref_genome, const vsc_genome *win_genome,
                                const vsc_variant_map *map, const char *pattern, const char *guides, uint32_t n_guides,
                                uint32_t len, const vsc_pattern_params *params, const vsc_pattern_table *table /* may be NULL */,
                                const vsc_locus *exclude /* may be NULL, reference coordinates */, uint32_t chunk_guides,
                                vsc_pattern_variant_row *ref_rows, vsc_pattern_variant_row *win_rows,
                                vsc_pattern_variant_row *var_rows /* may be NULL */,
                                vsc_guide_table_row *ref_table, vsc_guide_table_row *win_table,
                                vsc_guide_table_row *var_table /* the three: NULL without a table */);

/* ---- table scores for bulged alignments and cut sites: per record, per guide, top-K sites --------------------- */
/*
 * The score above over everything the searches report: the bulged alignments of vsc_search_bulges /
 * vsc_search_pattern_bulges and the cut sites of vsc_hits_sites / vsc_pattern_hits_sites.  CRISPRitz and CRISPRme score every
 * bulged alignment, keep the best-scoring alignment of each cluster and rank the clusters; this is that listing's score,
 * rows and cut.  The library ships no weights.
 *
 * TABLE   vsc_bulge_table, host-only and immutable, with a process-wide serial number like the other tables.  Built from a
 *         vsc_pattern_table (its shape and weights are COPIED: the new table does not depend on the old one's lifetime) plus
 *         two arrays of doubles, dna[ps_len][4] and rna[ps_len][4].  Write a = ps_start, e = ps_start + ps_len.
 *         dna[i][s] is the weight of one unpaired site base s (read orientation, A 0 C 1 G 2 T 3) when the bulge lies in
 *           front of read position a + i.
 *         rna[i][g] is the weight of the unpaired guide base g at read position a + i.
 *         Every weight is finite and lies in [0, 1]; ps_len >= 4.  Anything else: VSC_ERR_INVALID.
 *         Row 0 of dna and rows 0 and ps_len - 1 of rna are never read; they are still validated.
 *         With L = 23, protospacer (0, 20), pam_pos {21, 22} and a vsc_score_table's weights this is the SpCas9 form.
 * SCORE   of a bulged alignment: guide G (L IUPAC letters), site s (L + d letters in read orientation), d in {-2, -1, +1, +2},
 *         split index i = the record's VSC_BULGE_INDEX as vsc_pattern_bulge_align defines it.  The paired site q:
 *           DNA bulge (b = d > 0):   q[j] = s[j] for j < i, q[j] = s[j + b] for j >= i.
 *           RNA bulge (b = -d > 0):  q[j] = s[j] for j < i, q[j] = s[j - b] for j >= i + b; positions [i, i + b) carry no letter.
 *         Then, in this order:
 *           1. x = the SCORE of vsc_search_pattern_table of G against q, the unpaired positions taking no part: the
 *              mismatch weights in ascending position, then the PAM weight of q at pam_pos.
 *           2. DNA bulge: for t = 0 .. b - 1 in this order, x = x * dna[i - a][s[i + t]].
 *           3. RNA bulge: for t = 0 .. b - 1 in this order, if G[i + t] is one of A, C, G, T then
 *              x = x * rna[i + t - a][G[i + t]].  A degenerate letter takes no part, as everywhere else.
 *         fp64, one rounding per multiplication, no contraction.  f = rint(x * 2^30) as above, f <= 2^30.
 *         The score belongs to the alignment the search REPORTS: the smallest i that reaches NM.  It is not a maximum over
 *         the split points.
 *         With every dna and rna weight equal to 1.0, f is vsc_pattern_table_score's f of (G, q), bit for bit.
 *         A record outside the definition scores f = 0 and nothing is read outside an array: a guide index >= n_guides, a
 *         size of 0 or 3, L + d outside 16..32, i outside a + 1 .. e - 1 (RNA: i + b <= e - 1), a contig index >= the
 *         genome's contig count, a site that leaves its contig, a site that touches a plane word outside the words the
 *         genome was loaded with.  A span of 34 letters at bit offset 31 touches three 32-base words; every one of them is
 *         checked.  A shard is loaded with one halo word behind its own words: a record that needs a second one scores 0 on
 *         that shard.
 * SITE    A vsc_site names guide, strand, contig, anchor and, in members, which d in -2 .. +2 are present.  In read
 *         orientation every member's letters are the L + d letters that end at the anchor (VSC_SITE_ANCHOR_END) or begin
 *         there (VSC_SITE_ANCHOR_START); all lie inside one span of L + (the largest d present) letters, fetched once.  For
 *         each present member (NM, i) is recomputed - vsc_pattern_bulge_align's walk, the plain compare for d = 0 - and the
 *         member scored as above (d = 0: the SCORE of vsc_search_pattern_table).  No record list is looked up: the site
 *         record, the planes and the guide are enough.
 *         vsc_site_score { best, top, top_d, reserved }, 16 bytes: best = f of the record's best alignment, top = the
 *         largest f among the members, top_d = d + 2 of the member that attains it - on equal f the member that is smaller
 *         under the site's order (NM + |d|, |d|, DNA before RNA).  A site outside the definition (as above, or whose best
 *         alignment is not among its members): all zero.
 * ROWS    vsc_guide_table_row per guide.  vsc_bulge_hits_table: score_sum = sum of f, positive = records with f > 0,
 *         positive_nm[k] = those by the record's NM (clamped to 8).  vsc_sites_table: score_sum = sum of top, positive = sites
 *         with top > 0, positive_nm[k] = those by the best alignment's NM (clamped to 8), over ALL sites, before any
 *         selection.  vsc_table_specificity(score_sum) applies as it does above: a bulge-aware specificity.
 * SELECT  vsc_pattern_select as it is, with the key top: per guide the survivors are the sites with top >= min_score, of
 *         those the first top_k (0: all) are kept under the ranking top descending, then record order; the result stays in
 *         record order.  NULL or { 0, 0 } returns every site.  A non-zero reserved field: VSC_ERR_INVALID.
 *
 * vsc_bulge_table_score: one guide (len IUPAC letters) against one site (len + d letters of ACGT in read orientation) on the
 * host, with the very functions the kernels call; d = 0 gives the plain score (*nm = the mismatches, *index = 0), otherwise
 * (*nm, *index) are vsc_pattern_bulge_align's walk over the table's protospacer.  A d outside -2 .. 2, len + d outside
 * 16..32 or a letter that is not ACGT: VSC_ERR_INVALID.  All four outputs are optional.
 * vsc_bulge_hits_table scores the records of a bulge result where they lie: fixed (host, one word per record) or rows may be
 * NULL, both NULL: VSC_ERR_INVALID.  vsc_sites_table scores the sites of a result of vsc_hits_sites /
 * vsc_pattern_hits_sites: *out is a NEW vsc_sites that holds the survivors and their score records (vsc_sites_scores / _dev;
 * VSC_ERR_INVALID / NULL on an unscored result); the input is not modified.  out or rows may be NULL, both NULL:
 * VSC_ERR_INVALID.  For both: guides are n_guides * len IUPAC letters (a caller with vsc_pack_guide codes spells them first);
 * a table whose len is not len, params->len other than len, a result or a genome of another context: VSC_ERR_INVALID; an
 * empty input returns VSC_OK and launches nothing; the inputs and vsc_ctx_timing stay as they are.  The context keeps the
 * device copy of the table it used last, keyed by the serial number; vsc_ctx_release_scratch gives it back.
 * Not provided: weights, a maximum over split points, scores of variant-window hits (since added for pattern hits: 4.25,
 * vsc_search_pattern_variants above), a vsc_multi_* entry (sites are defined on merged records).
 */
typedef struct vsc_bulge_table vsc_bulge_table;
typedef struct {
    uint64_t serial;        /* process-wide number of the table */
    uint32_t zero_weights;  /* weights that are exactly 0, dna and rna included */
    uint32_t reserved;
    vsc_pattern_table_shape shape;
} vsc_bulge_table_stats;
typedef struct {
    uint32_t best;     /* f of the record's best alignment */
    uint32_t top;      /* the largest f among the members */
    uint32_t top_d;    /* d + 2 of the member that attains top */
    uint32_t reserved; /* 0 */
} vsc_site_score;
#ifdef __cplusplus
static_assert(sizeof(vsc_bulge_table_stats) == 48, "vsc_bulge_table_stats layout");
static_assert(sizeof(vsc_site_score) == 16, "vsc_site_score layout");
#else
_Static_assert(sizeof(vsc_bulge_table_stats) == 48, "vsc_bulge_table_stats layout");
_Static_assert(sizeof(vsc_site_score) == 16, "vsc_site_score layout");
#endif
int vsc_bulge_table_build(const vsc_pattern_table *base, const double *dna /* [ps_len][4] */, const double *rna /* [ps_len][4] */,
                          vsc_bulge_table **out);
int vsc_bulge_table_free(vsc_bulge_table *table);
int vsc_bulge_table_info(const vsc_bulge_table *table, vsc_bulge_table_stats *out);
int vsc_bulge_table_score(const vsc_bulge_table *table, const char *guide, const char *site_text /* len + d letters, read orientation */,
                          int d, uint32_t *nm, uint32_t *index, double *score, uint32_t *fixed);
int vsc_bulge_hits_table(vsc_ctx *ctx, const vsc_genome *genome, vsc_bulge_hits *hits, const char *guides /* n_guides * len letters */,
                         uint32_t n_guides, uint32_t len, const vsc_bulge_table *table,
                         uint32_t *fixed /* host, one per record, may be NULL */, vsc_guide_table_row *rows /* may be NULL */);
int vsc_sites_table(vsc_ctx *ctx, const vsc_genome *genome, vsc_sites *sites, const vsc_site_params *params, const char *guides,
                    uint32_t n_guides, uint32_t len, const vsc_bulge_table *table, const vsc_pattern_select *select /* may be NULL */,
                    vsc_sites **out /* may be NULL */, vsc_guide_table_row *rows /* may be NULL */);
/* Host copy of the score records (made on first use; valid until vsc_sites_free). */
int vsc_sites_scores(vsc_sites *sites, const vsc_site_score **out);
/* Device pointer (valid until vsc_sites_free); NULL when the result is empty or not a scored one. */
const void *vsc_sites_scores_dev(const vsc_sites *sites);

/* ---- on-target efficiency of candidate guides (linear position-specific models) ------------------------------ */
/*
 * "Will this guide cut at its own site?" for the scores that are an intercept plus one weight per (position, base) and per
 * (position, dinucleotide) over a context window around the site, plus a term in the G/C count of a range - the form of
 * Doench 2014 "Rule Set 1" and of Moreno-Mateos 2015 "CRISPRscan" - optionally pushed through a logistic link.  The library
 * ships no model: the caller brings the weights (vsc_eff_model_build).
 *
 * SHAPE    vsc_eff_shape { up, site_len, down, gc_start, gc_len, link, reserved[2] }.
 *          C = up + site_len + down is the context length: the site and its flanks.
 *          up, down <= 16.  site_len 16 .. 32: 23 for vsc_guides' candidates, the pattern's length for vsc_pattern_guides'.
 *          C <= 64.
 *          The G/C range is [gc_start, gc_start + gc_len) in context coordinates and lies inside the context.
 *          gc_len == 0: no G/C term.
 *          link is VSC_EFF_IDENTITY or VSC_EFF_LOGISTIC.
 *          Anything else, or a non-zero reserved field: VSC_ERR_INVALID.
 * CONTEXT  of a locus (c, p, strand), in READ orientation:
 *            '+': c[p - up, p + site_len + down).
 *            '-': revcomp(c[p - down, p + site_len + up)).
 *          Context position up is the first base of the site as the guide reads it.
 *          It is defined only when it lies wholly inside contig c and holds no non-ACGT letter.
 * MODEL    intercept, mono[C][4], di[C - 1][16] indexed 4 * b_j + b_{j+1}, gc[gc_len + 1] (NULL iff gc_len == 0).
 *          Bases are coded A 0, C 1, G 2, T 3.
 *          Every value is a finite double.  Anything else: VSC_ERR_INVALID.
 *          -0.0 is stored as +0.0.
 * LINEAR   The linear predictor, fp64, in this order:
 *            x = intercept.
 *            For j = 0 .. C - 1 ascending: x = x + mono[j][b_j].
 *            For j = 0 .. C - 2 ascending: x = x + di[j][4 * b_j + b_{j+1}].
 *            If gc_len: x = x + gc[number of G and C in the range].
 *          Each addition rounds once.  There is no multiplication, so nothing contracts.
 *          Device, host (vsc_eff_score_text) and any restatement that adds in this order agree to the bit.
 * UNDEF    An undefined predictor is the quiet NaN with bits 0x7FF8000000000000.
 *          Each candidate falls in exactly one class, tested in this order (vsc_eff_stats counts them; they add up to n):
 *            invalid       contig >= n_contigs, strand > 1, or the site itself leaves its contig.
 *            off_contig    the flanks leave the contig.
 *            not_resident  the context is not wholly inside the plane words this genome object was loaded with.
 *                          (A shard: nothing in front of first_word, nothing behind its halo.)
 *            has_n         the context holds a non-ACGT letter.
 *            defined
 * LINK     identity: the score is x.  logistic: 1.0 / (1.0 + exp(-x)).
 *          vsc_eff_link evaluates it on the HOST, with the C library's exp.
 *          The device never calls exp: its exp is another function and the bits would differ.
 *          Floors (min_linear) are in the linear domain.  link(undefined) = undefined.
 *
 * vsc_eff_model is host-only and immutable.  vsc_eff_model_info returns its process-wide serial number, its shape and the
 * count of weights (mono, di, gc) that are not 0.  A context keeps the device copy of the model it used last, keyed by the
 * serial number; vsc_ctx_release_scratch gives it back, with the candidates and scores on their way.
 * vsc_eff_score_text scores one context of C letters (any case) in read orientation on the host, with the very function the
 * kernels call; a non-ACGT letter gives undefined (VSC_OK), a text of another length is VSC_ERR_INVALID.
 *
 * vsc_loci_efficiency: linear[i] = the predictor of loci[i] (host arrays, n entries; a locus names the site's first base on
 * the forward strand, as everywhere).  One upload, one kernel, one copy back.  stats is optional.  n == 0: VSC_OK, nothing is
 * launched.  vsc_guides_efficiency scores the candidates where they lie on the device - no locus travels - and requires
 * site_len == 23 (else VSC_ERR_INVALID); the host-only object of vsc_multi_guides_enumerate goes the vsc_loci_efficiency way.
 * vsc_pattern_guides_efficiency is the same for vsc_pattern_guides: site_len is the pattern's length, which the CALLER vouches
 * for, as with vsc_pattern_guide_text.  linear[i] belongs to candidate i.  A genome of another context, an object of another
 * context, a NULL model or a NULL linear with n > 0: VSC_ERR_INVALID.
 *
 * vsc_guides_filter_efficiency / vsc_pattern_guides_filter_efficiency: *out = the candidates of `in` whose predictor is
 * defined and >= min_linear - codes and loci copied unchanged, in the input's order; `in` stays as it is.  Count pass, scan,
 * write pass over tiles of 1 024 candidates: no append atomic, the bytes depend on the input and the model only.  min_linear
 * NaN: VSC_ERR_INVALID.  -inf keeps every defined candidate, +inf none (an empty result is a result).  The result is a normal
 * object of its kind on ctx's device: the searches, vsc_guides_locate, vsc_guides_pairs and these calls take it as any other.
 * A host-only input is uploaded first.
 *
 * vsc_ctx_timing afterwards: score_ms = total_ms = the kernel (the filter: both passes and the scan), sites = n, genome_bytes
 * = 16 bytes of locus read and 8 bytes of score written per candidate (the filter: the loci read twice, 24 bytes read and 24
 * written per survivor).  The other fields are 0.
 *
 * Not offered: a vsc_multi_* entry (the multi-device enumeration already joins its candidates on the host, and a shard cannot
 * see in front of its first word - load the genome on one device, or score by vsc_loci_efficiency there); ranking or top-K
 * per target interval; neural scores (Rule Set 3, DeepCpf1).  Rule Set 2 is a tree ensemble: the next section.
 */
#define VSC_EFF_IDENTITY 0
#define VSC_EFF_LOGISTIC 1
typedef struct vsc_eff_model vsc_eff_model;
typedef struct {
    uint32_t up, site_len, down; /* C = up + site_len + down */
    uint32_t gc_start, gc_len;   /* context coordinates; gc_len 0: no G/C term */
    uint32_t link;               /* VSC_EFF_* */
    uint32_t reserved[2];        /* 0 */
} vsc_eff_shape;
typedef struct {
    uint64_t serial;          /* process-wide number of the model */
    vsc_eff_shape shape;
    uint32_t nonzero_weights; /* entries of mono, di and gc that are not 0 */
    uint32_t reserved;
} vsc_eff_model_stats;
typedef struct {
    uint64_t defined, invalid, off_contig, not_resident, has_n;
    uint64_t reserved[3]; /* 0 */
} vsc_eff_stats;
#ifdef __cplusplus
static_assert(sizeof(vsc_eff_stats) == 64, "vsc_eff_stats layout");
#else
_Static_assert(sizeof(vsc_eff_stats) == 64, "vsc_eff_stats layout");
#endif
int vsc_eff_model_build(const vsc_eff_shape *shape, double intercept, const double *mono /* [C][4] */,
                        const double *di /* [C - 1][16] */, const double *gc /* [gc_len + 1]; NULL iff gc_len == 0 */,
                        vsc_eff_model **out);
int vsc_eff_model_free(vsc_eff_model *model);
int vsc_eff_model_info(const vsc_eff_model *model, vsc_eff_model_stats *out);
int vsc_eff_score_text(const vsc_eff_model *model, const char *context /* C letters, read orientation */, double *linear);
double vsc_eff_link(const vsc_eff_model *model, double linear);
int vsc_loci_efficiency(vsc_ctx *ctx, const vsc_genome *genome, const vsc_locus *loci /* host */, uint64_t n,
                        const vsc_eff_model *model, double *linear /* host, n */, vsc_eff_stats *stats /* optional */);
int vsc_guides_efficiency(vsc_ctx *ctx, const vsc_genome *genome, vsc_guides *guides, const vsc_eff_model *model,
                          double *linear /* host, one per candidate */, vsc_eff_stats *stats /* optional */);
int vsc_pattern_guides_efficiency(vsc_ctx *ctx, const vsc_genome *genome, vsc_pattern_guides *guides, const vsc_eff_model *model,
                                  double *linear /* host, one per candidate */, vsc_eff_stats *stats /* optional */);
int vsc_guides_filter_efficiency(vsc_ctx *ctx, const vsc_genome *genome, vsc_guides *in, const vsc_eff_model *model,
                                 double min_linear, vsc_guides **out);
int vsc_pattern_guides_filter_efficiency(vsc_ctx *ctx, const vsc_genome *genome, vsc_pattern_guides *in,
                                         const vsc_eff_model *model, double min_linear, vsc_pattern_guides **out);

/* ---- on-target efficiency from regression-tree ensembles -------------------------------------------------------- */
/*
 * The same question for the scores that are a gradient-boosted ensemble of small regression trees over sequence tests - the
 * form of Doench 2016 "Rule Set 2" / Azimuth, and of whatever a caller retrains on a screen of their own.  The library ships
 * no model: the caller brings the trees (vsc_eff_trees_build), with a learning rate folded into the leaves.
 *
 * SHAPE     up, site_len, down, link as vsc_eff_shape (C = up + site_len + down <= 64, flanks <= 16, site_len 16..32);
 *           CONTEXT, the five classes and their order, and UNDEF (the NaN 0x7FF8000000000000) are those of the linear
 *           model - eff_context of vsc_efficiency.h is used as it is, not copied.
 * SUMS      n_sums <= 16.  Sum i: a range [start, start + len) inside the context, int32 mono[4], int32 di[16], every |w| <= 2^20:
 *             S_i = sum over j in the range of mono[b_j]  +  sum over j with j and j+1 in the range of di[4 b_j + b_{j+1}]
 *           (int32, cannot overflow: 127 terms of at most 2^20).  len 0: S_i = 0.
 * TREES     1..1024 trees, at most 8 192 nodes in all, depth (edges from the root) at most 32.  A tree's nodes are numbered from 0
 *           (the root); an inner node's children have LARGER numbers than the node, and every node but the root is the child of
 *           exactly one node.  Node kinds:
 *             LEAF     value (finite double; -0.0 stored as +0.0)
 *             BASE     pos (0..C-1), mask (4 bits):            true iff bit b_pos of mask is set
 *             PAIR     pos_a != pos_b (0..C-1), mask (16 bits): true iff bit 4 b_{pos_a} + b_{pos_b} of mask is set
 *             SUM      i (< n_sums), t (int32):                 true iff S_i <= t
 *           true goes to `left`, false to `right`.  Masks 0 and all-ones are allowed (a constant test).
 * PREDICTOR x = base;  for t = 0 .. n_trees - 1 in this order:  x = x + value(the leaf the context reaches in tree t).
 *           fp64, one rounding per addition, no multiplication: a learning rate is folded into the leaves by the caller.
 * LINK      identity or logistic, on the HOST only, exactly as vsc_eff_link.
 *
 * A model that breaks any of these rules is refused with VSC_ERR_INVALID by vsc_eff_trees_build, never at a launch: a child
 * not larger than its parent, a child outside the tree, a node with two parents or with none, a depth of 33, 8 193 nodes, a
 * value (or a base) that is not finite, a weight of 2^20 + 1, a range that leaves the context, pos_a == pos_b, a position
 * outside the context, a mask wider than its kind's, a sum that does not exist, an unknown kind, a field that has no meaning
 * for the node's kind and is not 0, a shape with a G/C range (gc_start and gc_len are 0 here).
 *
 * vsc_eff_trees_build: sums[n_sums] (NULL iff n_sums == 0); nodes[tree_first[n_trees]], tree t's nodes being
 * nodes[tree_first[t] .. tree_first[t + 1]) with left / right numbered inside the tree; tree_first[0] == 0, ascending.
 * vsc_eff_trees is host-only and immutable.  vsc_eff_trees_info returns its process-wide serial number, its shape and the
 * counts of sums, trees and nodes by kind, and the depth of the deepest leaf.  A context keeps the device copy of the tree
 * model it used last, keyed by the serial number, beside the linear model's; vsc_ctx_release_scratch gives it back.
 * vsc_eff_trees_score_text and vsc_eff_trees_link are vsc_eff_score_text and vsc_eff_link for this model: the text is scored
 * with the very functions the kernels call.
 *
 * vsc_loci_efficiency_trees, vsc_guides_efficiency_trees (site_len == 23), vsc_pattern_guides_efficiency_trees,
 * vsc_guides_filter_efficiency_trees and vsc_pattern_guides_filter_efficiency_trees are the five calls above with this
 * predictor: the same arguments, classes, stats, refusals (a NaN min_linear among them), results and vsc_ctx_timing.  The
 * filter keeps defined && x >= min_linear; its bytes depend on the input and the model only.
 *
 * Not offered: shipped weights; features that are no function of the context (position in the peptide, a melting
 * temperature as a ratio); models above the caps; random-forest averages (a division follows the sum); a vsc_multi_* entry
 * (as above); neural scores (Rule Set 3, DeepCpf1).
 */
#define VSC_EFF_NODE_LEAF 0
#define VSC_EFF_NODE_BASE 1
#define VSC_EFF_NODE_PAIR 2
#define VSC_EFF_NODE_SUM 3
typedef struct vsc_eff_trees vsc_eff_trees;
typedef struct {
    uint32_t start, len; /* [start, start + len) in context coordinates */
    int32_t mono[4];     /* per letter */
    int32_t di[16];      /* 4 * b_j + b_{j+1} */
} vsc_eff_sum;
typedef struct {
    uint32_t kind;        /* VSC_EFF_NODE_* */
    uint32_t a;           /* BASE: pos; PAIR: pos_a; SUM: i; LEAF: 0 */
    uint32_t b;           /* PAIR: pos_b; else 0 */
    uint32_t mask;        /* BASE: 4 bits; PAIR: 16 bits; else 0 */
    int32_t t;            /* SUM: the threshold; else 0 */
    uint32_t left, right; /* inner nodes: the children's numbers inside the tree (true, false); LEAF: 0 */
    uint32_t reserved;    /* 0 */
    double value;         /* LEAF: its value; else 0 */
} vsc_eff_node;
typedef struct {
    uint64_t serial; /* process-wide number of the model */
    vsc_eff_shape shape;
    uint32_t n_sums, n_trees, n_nodes;
    uint32_t leaves, base_nodes, pair_nodes, sum_nodes;
    uint32_t max_depth; /* edges from a root to the deepest leaf */
    uint64_t reserved[2];
} vsc_eff_trees_stats;
#ifdef __cplusplus
static_assert(sizeof(vsc_eff_sum) == 88 && sizeof(vsc_eff_node) == 40 && sizeof(vsc_eff_trees_stats) == 88, "vsc_eff_trees layout");
#else
_Static_assert(sizeof(vsc_eff_sum) == 88 && sizeof(vsc_eff_node) == 40 && sizeof(vsc_eff_trees_stats) == 88, "vsc_eff_trees layout");
#endif
int vsc_eff_trees_build(const vsc_eff_shape *shape, double base, const vsc_eff_sum *sums, uint32_t n_sums, const vsc_eff_node *nodes,
                        const uint32_t *tree_first /* [n_trees + 1] */, uint32_t n_trees, vsc_eff_trees **out);
int vsc_eff_trees_free(vsc_eff_trees *model);
int vsc_eff_trees_info(const vsc_eff_trees *model, vsc_eff_trees_stats *out);
int vsc_eff_trees_score_text(const vsc_eff_trees *model, const char *context /* C letters, read orientation */, double *linear);
double vsc_eff_trees_link(const vsc_eff_trees *model, double linear);
int vsc_loci_efficiency_trees(vsc_ctx *ctx, const vsc_genome *genome, const vsc_locus *loci /* host */, uint64_t n,
                              const vsc_eff_trees *model, double *linear /* host, n */, vsc_eff_stats *stats /* optional */);
int vsc_guides_efficiency_trees(vsc_ctx *ctx, const vsc_genome *genome, vsc_guides *guides, const vsc_eff_trees *model,
                                double *linear /* host, one per candidate */, vsc_eff_stats *stats /* optional */);
int vsc_pattern_guides_efficiency_trees(vsc_ctx *ctx, const vsc_genome *genome, vsc_pattern_guides *guides, const vsc_eff_trees *model,
                                        double *linear /* host, one per candidate */, vsc_eff_stats *stats /* optional */);
int vsc_guides_filter_efficiency_trees(vsc_ctx *ctx, const vsc_genome *genome, vsc_guides *in, const vsc_eff_trees *model,
                                       double min_linear, vsc_guides **out);
int vsc_pattern_guides_filter_efficiency_trees(vsc_ctx *ctx, const vsc_genome *genome, vsc_pattern_guides *in,
                                               const vsc_eff_trees *model, double min_linear, vsc_pattern_guides **out);

/* ---- microhomology and out-of-frame scores of candidate guides ------------------------------------------------ */
/*
 * "When this guide cuts, will the repair knock the gene out?": the microhomology score of Bae, Kweon, Kim & Kim (Nat. Methods
 * 2014) over the bases around the cut site - every microhomology-mediated deletion, weighted by its length and G/C content -
 * and the share of it whose deletion length is no multiple of three (the "Out-of-Frame" column of guide-design tools).  A
 * formula: there is no model to bring.
 *
 * SHAPE    site_len 16 .. 32, cut 0 .. site_len, flank F 8 .. 32;  W = 2 F <= 64.
 *          cut: the break lies between read positions cut - 1 and cut of the site (SpCas9 23-mer: 17).
 * CONTEXT  of a locus (c, p, strand) - p the site's first base on the forward strand, as everywhere - in READ orientation:
 *          read positions [cut - F, cut + F) relative to the site's first read base; it may reach outside the site on either side.
 *            '+': c[p + cut - F, p + cut + F)
 *            '-': revcomp(c[p + site_len - cut - F, p + site_len - cut + F))
 * CLASS    one per candidate, tested in this order (as vsc_eff_stats):
 *            invalid      contig, strand, or the SITE leaves its contig
 *            off_contig   the context does
 *            not_resident the context is not wholly in the words this genome object was loaded with
 *            has_n
 *            defined
 * ROWS     over the context s[0, W), left = F:
 *            every (i, j, k) with 2 <= k <= F - 1, 0 <= i, i + k <= F, F <= j, j + k <= W, s[i, i + k) == s[j, j + k).
 *          A row is DROPPED when another row with the same j - i contains it (i' <= i, i + k <= i' + k').
 *          This is the published script, its range(2, left) included.
 * SCORE    of a kept row:
 *            d = j - i (the deletion length), g = number of G/C in s[i, i + k),
 *            v = T[d] * (k + g), in TENTHS of the published score.
 *            T[d] = round(exp(-d / 20), 3) * 1000 as an integer, d = 0 .. 63:
 *                   1000, 951, 905, 861, 819, 779, 741, 705, 670, 638, 607, ... 47, 45, 43
 * OUTPUT   two uint32 per candidate:
 *            sum = sum of v over kept rows
 *            oof = the same over rows with d % 3 != 0
 *          Both are 0xFFFFFFFF (VSC_MH_UNDEFINED) unless the class is defined.  sum <= 4.1e6.
 *          mhScore = sum / 10.
 *          oofScore = 100 * oof / sum (0 when sum == 0).
 *          Both are fp64 on the HOST only (vsc_mh_scores), one division each.
 * FILTER   keep a candidate iff all three hold, tested in uint64; with sum == 0 the last holds only for min_oof_permille == 0:
 *            its class is defined
 *            sum >= min_sum
 *            1000 * oof >= min_oof_permille * sum
 *
 * The integers are the exact value: every weight is a whole number of thousandths, so sum / 10 is the published sum without a
 * rounding.  The published script adds floats and truncates; where its float sum lands just under a whole number its int() is
 * one below sum / 10 rounded down.  No bit-parity with that int() is claimed.  Device, host (vsc_mh_score_text) and the row
 * list restated in integers agree to the bit.
 *
 * vsc_mh_score_text scores one context of W = 2 * flank letters (any case) in read orientation on the host, with the very
 * function the kernels call; a non-ACGT letter gives the undefined pair (VSC_OK), a text of another length or a flank outside
 * 8 .. 32 is VSC_ERR_INVALID.  vsc_mh_scores turns a pair into the two doubles; the undefined pair gives two NaNs (VSC_OK),
 * oof > sum is VSC_ERR_INVALID.
 *
 * vsc_loci_microhomology: pairs[2 i], pairs[2 i + 1] = sum, oof of loci[i] (host arrays, n entries).  One upload, one kernel,
 * one copy back.  stats is optional: the candidates by class (they add up to n), the kernel's time and the call's wall time
 * in milliseconds.  n == 0: VSC_OK, nothing is launched.  vsc_guides_microhomology scores the candidates where they lie on the
 * device - no locus travels - and requires site_len == 23 (else VSC_ERR_INVALID); the host-only object of
 * vsc_multi_guides_enumerate goes the vsc_loci_microhomology way.  vsc_pattern_guides_microhomology is the same for
 * vsc_pattern_guides: site_len is the pattern's length, which the CALLER vouches for.  A shape outside SHAPE or with a non-zero
 * reserved field, a genome of another context, an object of another context, a NULL shape or NULL pairs with n > 0:
 * VSC_ERR_INVALID.
 *
 * vsc_guides_filter_microhomology / vsc_pattern_guides_filter_microhomology: *out = the candidates of `in` that pass FILTER -
 * codes and loci copied unchanged, in the input's order; `in` stays as it is.  Count pass, scan, write pass over tiles of
 * 1 024 candidates: no append atomic, the bytes depend on the input, the shape and the floors only.  min_oof_permille > 1000:
 * VSC_ERR_INVALID.  The result is a normal object of its kind on ctx's device, as the efficiency filter's is.
 *
 * vsc_ctx_timing afterwards: as after the efficiency calls (8 bytes written per candidate).  The scratch is the efficiency
 * calls'; vsc_ctx_release_scratch gives it back.
 *
 * Not offered: a vsc_multi_* entry (for the reason given above for the efficiency calls); indel-outcome models that need
 * trained weights; windows with left != right.  (Ranking and top-K per target: vsc_*_pick below.)
 */
#define VSC_MH_UNDEFINED 0xFFFFFFFFu
typedef struct {
    uint32_t site_len, cut, flank;
    uint32_t reserved; /* 0 */
} vsc_mh_shape;
typedef struct {
    uint64_t defined, invalid, off_contig, not_resident, has_n;
    double kernel_ms, wall_ms;
    uint64_t reserved; /* 0 */
} vsc_mh_stats;
#ifdef __cplusplus
static_assert(sizeof(vsc_mh_stats) == 64 && sizeof(vsc_mh_shape) == 16, "vsc_mh_stats / vsc_mh_shape layout");
#else
_Static_assert(sizeof(vsc_mh_stats) == 64 && sizeof(vsc_mh_shape) == 16, "vsc_mh_stats / vsc_mh_shape layout");
#endif
int vsc_mh_score_text(const char *context /* 2 * flank letters, read orientation */, uint32_t flank, uint32_t *sum, uint32_t *oof);
int vsc_mh_scores(uint32_t sum, uint32_t oof, double *mh_score, double *oof_score);
int vsc_loci_microhomology(vsc_ctx *ctx, const vsc_genome *genome, const vsc_locus *loci /* host */, uint64_t n,
                           const vsc_mh_shape *shape, uint32_t *pairs /* host, 2 n */, vsc_mh_stats *stats /* optional */);
int vsc_guides_microhomology(vsc_ctx *ctx, const vsc_genome *genome, vsc_guides *guides, const vsc_mh_shape *shape,
                             uint32_t *pairs /* host, two per candidate */, vsc_mh_stats *stats /* optional */);
int vsc_pattern_guides_microhomology(vsc_ctx *ctx, const vsc_genome *genome, vsc_pattern_guides *guides, const vsc_mh_shape *shape,
                                     uint32_t *pairs /* host, two per candidate */, vsc_mh_stats *stats /* optional */);
int vsc_guides_filter_microhomology(vsc_ctx *ctx, const vsc_genome *genome, vsc_guides *in, const vsc_mh_shape *shape,
                                    uint32_t min_sum, uint32_t min_oof_permille, vsc_guides **out);
int vsc_pattern_guides_filter_microhomology(vsc_ctx *ctx, const vsc_genome *genome, vsc_pattern_guides *in,
                                            const vsc_mh_shape *shape, uint32_t min_sum, uint32_t min_oof_permille,
                                            vsc_pattern_guides **out);

/* ---- the best K guides per target, with spacing ------------------------------------------------- */
/*
 * The fifth step of a design: of the candidates of every target choose the K best under a caller-made key, no two of them
 * closer than `spacing` bases at their cut sites, so that one SNP or one small deletion does not disable all of them.  A
 * target is a number: an interval, or a group of intervals (the exons of a gene).  This text is normative:
 *
 * SHAPE      site_len 16 .. 32, cut 0 .. site_len (SpCas9 23-mer: 17), k 1 .. 32, spacing uint32 (0: none),
 *            min_key uint64 (0: none), reserved fields 0.
 * CANDIDATE  i = 0 .. n - 1 (n <= 0xFFFFFFFE): locus (c, p, strand) as everywhere (p = first base of the site on the forward
 *            strand), key[i] uint64 (LARGER IS BETTER), target[i] uint32 in [0, n_targets) or VSC_REGION_NONE.
 * CUT COORDINATE   x = p + cut on '+', p + site_len - cut on '-'  (the centre of vsc_mh's context).
 * ELIGIBLE   contig and strand valid, the site inside its contig, target[i] < n_targets, key[i] >= min_key.
 *            Every other candidate is never picked and is counted in its class in the stats (invalid, no_target,
 *            bad_target, below_min_key; tested in this order).
 * BEFORE     a before b  <=>  key[a] > key[b], or key[a] == key[b] and a < b.          (a total order)
 * CONFLICT   a, b of one target conflict <=> same contig and |x_a - x_b| < spacing, in 64-bit arithmetic.
 *            spacing 0: never.  spacing >= 1: a '+' and a '-' candidate with one cut coordinate conflict.
 * PICK of target t   picked = [];  repeat: among the eligible candidates of t that are not picked and conflict with no
 *            picked one, take the first under BEFORE and append it; stop at k picks or when none is left.
 * OUTPUT     picks[t * k + r] = index of the r-th pick of t, VSC_PICK_NONE (0xFFFFFFFF) beyond counts[t];  counts[t];
 *            optional rank[i] = r if i is the r-th pick of its target, else VSC_PICK_NONE;
 *            optional `picked`: a new candidate object holding the picked candidates in ascending index.
 * TARGETS    either target[] is given (host array), or regions (+ optional group[]): label = vsc_regions_locate of the
 *            site's first base under the regions' own rule, target = group ? group[label] : label; a group entry may be
 *            VSC_REGION_NONE ("this interval belongs to no target"); group has one entry per INPUT interval.
 *
 * The output is fully determined by the inputs.  It does not depend on launch shape, on the order in which waves finish, or
 * on any atomic.
 *
 * vsc_pick_host is the definition as straightforward host code and needs no device: contigs gives the contig lengths, loci,
 * target and key are host arrays of n entries, picks has n_targets * k entries, counts n_targets, rank (optional) n.  It is
 * also the route for the host-only object of vsc_multi_guides_enumerate.  vsc_loci_pick takes the same host arrays, in any
 * order, and picks on the device; vsc_loci_pick_regions is the same with regions (+ optional group) in place of target[]: the
 * loci are uploaded and labelled on the device as vsc_guides_pick labels its candidates.  vsc_guides_pick / vsc_pattern_guides_pick take the candidates where they lie on the
 * device; exactly one of `regions` (+ optional `group`) and `target` is given.  With regions the labels are made on the device
 * inside the first kernel and no label leaves it.  key: a host array of vsc_guides_count entries, uploaded through context
 * scratch that vsc_ctx_release_scratch gives back.  vsc_guides_pick requires site_len == 23; for vsc_pattern_guides the CALLER
 * vouches for site_len.  `picked` may be NULL; otherwise *picked is a normal object of its kind on ctx's device (for a
 * host-only input: a host-only object) that every later call takes, freed as every such object.  stats is optional.
 *
 * VSC_ERR_INVALID: a shape outside SHAPE or a non-zero reserved field; a NULL argument; an object or genome of another
 * context; site_len != 23 for vsc_guides; both or neither of regions and target; a group without regions; regions built for
 * another contig table; a group entry >= n_targets that is not VSC_REGION_NONE.  VSC_ERR_RANGE: regions without the label
 * structure (as vsc_guides_locate); n > 0xFFFFFFFE.  n == 0: VSC_OK, nothing is launched, counts zeroed, picks all
 * VSC_PICK_NONE.  Every refusal comes before anything is written.  vsc_last_error names the reason.
 *
 * Not offered: a vsc_multi_* entry (the host-only object goes through vsc_pick_host); keys composed on the device; weights or
 * trained models; an optimal instead of the greedy choice under spacing.
 */
#define VSC_PICK_NONE 0xFFFFFFFFu
typedef struct {
    uint32_t site_len, cut, k, spacing;
    uint64_t min_key;
    uint64_t reserved; /* 0 */
} vsc_pick_params;
typedef struct {
    uint64_t eligible, invalid, no_target, bad_target, below_min_key; /* the candidates by class: they add up to n */
    uint64_t targets_picked; /* targets with at least one pick */
    uint64_t targets_short;  /* targets that end short of k although eligible candidates were left (spacing exhausted) */
    uint64_t picks;
    double kernel_ms, wall_ms;
    double stage_ms[4];      /* mark + scan, scatter, select, rank + picked (device calls; 0 from vsc_pick_host) */
    uint64_t reserved[2];    /* 0 */
} vsc_pick_stats;
#ifdef __cplusplus
static_assert(sizeof(vsc_pick_params) == 32 && sizeof(vsc_pick_stats) == 128, "vsc_pick_params / vsc_pick_stats layout");
#else
_Static_assert(sizeof(vsc_pick_params) == 32 && sizeof(vsc_pick_stats) == 128, "vsc_pick_params / vsc_pick_stats layout");
#endif
int vsc_pick_host(const vsc_contig *contigs, uint32_t n_contigs, const vsc_locus *loci, uint64_t n, const uint32_t *target,
                  const uint64_t *key, uint32_t n_targets, const vsc_pick_params *params, uint32_t *picks /* n_targets * k */,
                  uint32_t *counts /* n_targets */, uint32_t *rank /* optional, n */, vsc_pick_stats *stats /* optional */);
int vsc_loci_pick(vsc_ctx *ctx, const vsc_genome *genome, const vsc_locus *loci /* host */, uint64_t n, const uint32_t *target /* host */,
                  const uint64_t *key /* host */, uint32_t n_targets, const vsc_pick_params *params, uint32_t *picks, uint32_t *counts,
                  uint32_t *rank /* optional */, vsc_pick_stats *stats /* optional */);
int vsc_loci_pick_regions(vsc_ctx *ctx, const vsc_genome *genome, const vsc_locus *loci /* host */, uint64_t n, const vsc_regions *regions,
                          const uint32_t *group /* optional, host */, const uint64_t *key /* host */, uint32_t n_targets,
                          const vsc_pick_params *params, uint32_t *picks, uint32_t *counts, uint32_t *rank /* optional */,
                          vsc_pick_stats *stats /* optional */);
int vsc_guides_pick(vsc_ctx *ctx, const vsc_genome *genome, vsc_guides *guides, const vsc_regions *regions, const uint32_t *group,
                    const uint32_t *target, uint32_t n_targets, const uint64_t *key, const vsc_pick_params *params, uint32_t *picks,
                    uint32_t *counts, uint32_t *rank /* optional */, vsc_guides **picked /* optional */, vsc_pick_stats *stats /* optional */);
int vsc_pattern_guides_pick(vsc_ctx *ctx, const vsc_genome *genome, vsc_pattern_guides *guides, const vsc_regions *regions,
                            const uint32_t *group, const uint32_t *target, uint32_t n_targets, const uint64_t *key,
                            const vsc_pick_params *params, uint32_t *picks, uint32_t *counts, uint32_t *rank /* optional */,
                            vsc_pattern_guides **picked /* optional */, vsc_pick_stats *stats /* optional */);

/* ---- base-editor guide design: editing windows and target join ----------------------------------- */
/*
 * Base editors (CBE: C->T, ABE: A->G) do not cut: they convert one kind of base inside a short window of the protospacer.
 * "Which candidates place my base inside the window, which other editable bases (bystanders) sit there, and which guides are
 * best for every target?" - answered on the resident genome, where the candidates lie.
 *
 * SHAPE    site_len 16 .. 32;  win_start, win_len with 1 <= win_len <= 16 and win_start + win_len <= site_len, in READ positions of
 *          the site (0 = its first read base; the window may reach into PAM letters - the shape is the caller's);
 *          from 0 .. 3 (A C G T): the base the editor converts ON THE READ STRAND (CBE: C, ABE: A);  reserved fields 0.
 * SITE     of a locus (c, p, strand), p = first base of the site on the forward strand as everywhere, in read orientation:
 *          '+': c[p, p + site_len);  '-': its reverse complement.  This is eff_context with up = down = 0.
 * CLASS    one per candidate, tested in EffClass order: invalid (contig, strand, or the site leaves its contig), not_resident,
 *          has_n (an N anywhere in the site), defined.  off_contig cannot occur; its count stays 0.
 * MASK     bit j (0 <= j < win_len) is set iff the read base at win_start + j equals `from`.  Bits from win_len on are 0.
 * FORWARD  position of window position j on the candidate's contig:  '+': p + win_start + j;  '-': p + site_len - 1 - (win_start + j).
 * TARGETS  n_t points (contig, pos), STRICTLY ascending by (contig, pos), pos < the contig's length, n_t <= 0xFFFFFFFE.
 *          A target's index is its place in the array.  NULL with n_t == 0: no targets.
 * HITS     bit j is set iff MASK bit j is set and (the candidate's contig, FORWARD(j)) is a target.  The strand needs no rule of
 *          its own: a '+' candidate reaches targets whose forward letter is `from`, a '-' candidate those whose forward letter
 *          is its complement, and no candidate reaches a target with another letter.
 * ROW      two uint32 per candidate: (mask, hits).  Both are 0xFFFFFFFF (VSC_EDIT_UNDEFINED) unless the class is defined.
 *          Without targets hits = 0.
 * PAIR     one per set bit of hits, 16 bytes: { candidate (index i), target (index), mask, info = at | bystanders << 8 },
 *          at = j, bystanders = popcount(mask) - 1.  Order: ascending (candidate, target).  For a '-' candidate that is
 *          DESCENDING j.  n <= 0xFFFFFFFE.
 * COVERAGE optional, two uint32 per target: the number of pairs of the target, and the smallest `bystanders` among them
 *          (0xFFFFFFFF when the target has no pair).
 * FILTER   keep a candidate iff its class is defined, min_editable <= popcount(mask) <= max_editable, and (no targets were
 *          given, or hits != 0).  Survivors keep their input order.
 *
 * The output is a function of the inputs alone: it does not depend on launch shape or wave order.  The coverage counters use
 * integer add / min atomics, which commute; nothing else depends on an atomic's order, and the pairs have no append cursor.
 *
 * vsc_edit_site_text: the MASK of one site of site_len letters (any case) in read orientation on the host, by the function the
 * kernels call.  A letter other than ACGT, a text of another length, a shape outside SHAPE: VSC_ERR_INVALID.
 *
 * vsc_loci_edit: loci are host entries in any order, duplicates allowed.  rows (optional): rows[2 i], rows[2 i + 1] = mask, hits of
 * loci[i].  The pairs follow vsc_loci_pairs' contract: *n_pairs (optional) is always the full count; pairs == NULL only counts;
 * a count above `capacity` is VSC_ERR_RANGE, and then nothing is written to `pairs`, while rows, coverage, stats and *n_pairs
 * are valid.  coverage (optional): 2 n_t entries.  stats (optional): the candidates by class (the five counts add up to n), the
 * candidates with a hit, the pairs, the targets with a pair, the rows kernel's time and the call's wall time in milliseconds.
 * n == 0: VSC_OK, nothing is launched, the coverage says "no pair".  vsc_guides_edit works over the candidates where they lie on
 * the device - no locus travels - and requires site_len == 23; the host-only object of vsc_multi_guides_enumerate goes the
 * vsc_loci_edit way.  vsc_pattern_guides_edit is the same for vsc_pattern_guides: site_len is the pattern's length, which the
 * CALLER vouches for, as in the pick calls.
 *
 * vsc_guides_filter_edit / vsc_pattern_guides_filter_edit: *out = the candidates of `in` that pass FILTER - codes and loci copied
 * unchanged, in the input's order; `in` stays as it is.  Count pass, scan, write pass over tiles of 1 024 candidates, as the
 * microhomology filter.  The result is a normal object of its kind on ctx's device.
 *
 * VSC_ERR_INVALID, checked on the host before anything is written (vsc_last_error names the reason): a shape outside SHAPE or
 * with a non-zero reserved field; NULL arguments; a genome or object of another context; site_len != 23 for vsc_guides; targets
 * not strictly ascending, on an unknown contig, or beyond their contig; min_editable > max_editable; n_t > 0 with NULL targets.
 * VSC_ERR_RANGE: n or n_t above 0xFFFFFFFE.  Uploads and results use context scratch; vsc_ctx_release_scratch gives it back.
 *
 * Not offered: a vsc_multi_* entry; editing-efficiency or outcome models that need trained weights;
 * sequence-context preferences of the deaminase beyond `from`; more than one window per call (call twice).
 * Codon and amino-acid consequences are the next section's.
 */
#define VSC_EDIT_UNDEFINED 0xFFFFFFFFu
typedef struct {
    uint32_t site_len, win_start, win_len;
    uint32_t from; /* 0 .. 3: A C G T */
    uint32_t reserved[4]; /* 0 */
} vsc_edit_shape;
typedef struct {
    uint32_t contig, pos;
} vsc_edit_target;
typedef struct {
    uint32_t candidate, target, mask;
    uint32_t info; /* at | bystanders << 8 */
} vsc_edit_pair;
typedef struct {
    uint64_t defined, invalid, off_contig, not_resident, has_n;
    uint64_t with_hit, pairs, targets_covered;
    double kernel_ms, wall_ms;
    uint64_t reserved[2]; /* 0 */
} vsc_edit_stats;
#ifdef __cplusplus
static_assert(sizeof(vsc_edit_shape) == 32 && sizeof(vsc_edit_target) == 8 && sizeof(vsc_edit_pair) == 16 && sizeof(vsc_edit_stats) == 96,
              "vsc_edit_* layout");
#else
_Static_assert(sizeof(vsc_edit_shape) == 32 && sizeof(vsc_edit_target) == 8 && sizeof(vsc_edit_pair) == 16 && sizeof(vsc_edit_stats) == 96,
               "vsc_edit_* layout");
#endif
int vsc_edit_site_text(const char *site /* site_len letters, read orientation, any case */, const vsc_edit_shape *shape, uint32_t *mask);
int vsc_loci_edit(vsc_ctx *ctx, const vsc_genome *genome, const vsc_locus *loci /* host, any order, duplicates allowed */, uint64_t n,
                  const vsc_edit_shape *shape, const vsc_edit_target *targets /* host */, uint64_t n_t, uint32_t *rows /* host, 2 n, optional */,
                  vsc_edit_pair *pairs /* host, optional */, uint64_t capacity, uint64_t *n_pairs /* optional */,
                  uint32_t *coverage /* host, 2 n_t, optional */, vsc_edit_stats *stats /* optional */);
int vsc_guides_edit(vsc_ctx *ctx, const vsc_genome *genome, vsc_guides *guides, const vsc_edit_shape *shape,
                    const vsc_edit_target *targets, uint64_t n_t, uint32_t *rows, vsc_edit_pair *pairs, uint64_t capacity,
                    uint64_t *n_pairs, uint32_t *coverage, vsc_edit_stats *stats);
int vsc_pattern_guides_edit(vsc_ctx *ctx, const vsc_genome *genome, vsc_pattern_guides *guides, const vsc_edit_shape *shape,
                            const vsc_edit_target *targets, uint64_t n_t, uint32_t *rows, vsc_edit_pair *pairs, uint64_t capacity,
                            uint64_t *n_pairs, uint32_t *coverage, vsc_edit_stats *stats);
int vsc_guides_filter_edit(vsc_ctx *ctx, const vsc_genome *genome, vsc_guides *in, const vsc_edit_shape *shape,
                           const vsc_edit_target *targets, uint64_t n_t, uint32_t min_editable, uint32_t max_editable, vsc_guides **out);
int vsc_pattern_guides_filter_edit(vsc_ctx *ctx, const vsc_genome *genome, vsc_pattern_guides *in, const vsc_edit_shape *shape,
                                   const vsc_edit_target *targets, uint64_t n_t, uint32_t min_editable, uint32_t max_editable,
                                   vsc_pattern_guides **out);

/* ---- coding consequences of base edits: codons, amino acids, stop gains -------------------------- */
/*
 * What a base editor does to the proteins: for every candidate, the codons its window converts and what becomes of them -
 * "which guides make a stop (CRISPR-STOP / iSTOP), in which transcript, how early", "which guides fix a base while every
 * bystander stays synonymous" - answered on the resident genome against a CDS annotation, where the candidates lie.
 *
 * CODE      64 amino-acid letters indexed 16 b0 + 4 b1 + b2 (A C G T = 0 .. 3), '*' = stop. NULL = the standard code:
 *           KNKNTTTTRSRSIIMIQHQHPPPPRRRRLLLLEDEDAAAAGGGGVVVV*Y*YSSSS*CWCLFLF
 * SEGMENT   { contig, start, end, transcript, strand (0 '+', 1 '-'), phase (0 .. 2, GFF column 8) }, forward genome, half-open,
 *           non-empty, inside its contig. Segments are STRICTLY ascending by (contig, start) and do not overlap
 *           (end_i <= start_i+1 on one contig) - one transcript set per call. A caller with overlapping isoforms calls once per set.
 *           transcript < n_tx (dense indices into the caller's own table). All segments of a transcript lie on one contig and one
 *           strand. Their order in the transcript is ascending start on '+' and descending start on '-'.
 *           n <= 0xFFFFFFFE, a transcript's coding length < 2^31.
 * CODING    the host derives, per segment: bases_before = the transcript's bases in earlier segments (transcript order).
 *           shift = (3 - phase of the transcript's FIRST segment) % 3.
 *           The coding index of forward position x:
 *             '+': ci = shift + bases_before + (x - start)      '-': ci = shift + bases_before + (end - 1 - x).
 *           codon = ci / 3, frame = ci % 3. The phase of every later segment must equal (3 - (shift + bases_before) % 3) % 3,
 *           otherwise VSC_ERR_INVALID naming the segment.
 *           The host also derives the previous / next segment in transcript order.
 * CODON     of a coding base: the three bases with coding indices 3 codon .. 3 codon + 2 of its transcript, in transcript
 *           orientation (complemented on '-'). They are found by walking to the previous / next segment (at most two hops a side:
 *           segments of one base exist).
 *           A codon is UNKNOWN when one of its indices lies in front of the transcript's first coding base or behind its last one,
 *           or when one of its bases is N or not resident.
 * PARAMS    the vsc_edit_shape of 4.28, and `to` 0 .. 3, to != from: the base the editor writes on the read strand
 *           (CBE: T, ABE: G). OUTCOME: every base of MASK is converted (full conversion, the iSTOP assumption).
 *           In transcript orientation a converted base goes from -> to when the candidate's strand equals the transcript's,
 *           comp(from) -> comp(to) otherwise.
 * EFFECT    one per (candidate, transcript, codon) with at least one MASK base in it:
 *           ref = the codon, alt = the codon with ALL MASK bases of the window that fall in it converted. Class, tested in this order:
 *             5 unknown       the codon is UNKNOWN (ref = alt = 0)
 *             4 start_lost    codon == 0 and the transcript's first phase is 0
 *                             (any change of the first codon. Alternative starts are not modelled.)
 *             2 stop_gained   CODE[ref] != '*' and CODE[alt] == '*'
 *             3 stop_lost     CODE[ref] == '*' and CODE[alt] != '*'
 *             0 synonymous    CODE[ref] == CODE[alt]
 *             1 missense      otherwise
 *           16 bytes: { candidate, transcript, codon, info }, info = ref | alt << 6 | class << 12 | (edited bases in the codon) << 16
 *           | at << 20, at = the smallest window position j among them.
 *           Order: ascending candidate. Inside a candidate, ascending forward position of the codon's lowest-forward edited base.
 *           That base emits the effect: it is an emitter iff no other base of its codon with a lower forward position is a MASK base
 *           of the window. n <= 0xFFFFFFFE.
 * ROW       two uint32 per candidate. word 0 = the candidate's effects by class, 5 bits each: class k in bits [5 k, 5 k + 5).
 *           word 1 = bit j set iff MASK bit j is set and that base lies in a segment.
 *           Both are 0xFFFFFFFF unless the candidate's CLASS (4.28) is defined.
 * COVERAGE  optional, two uint32 per transcript: its stop_gained effects, and the smallest codon index among them (0xFFFFFFFF: none).
 * FILTER    keep iff the class is defined, (require == 0 or some effect's class bit is in require), and no effect's class bit is in
 *           forbid. require / forbid are masks over bits 0 .. 5. Survivors keep their input order.
 *
 * The output is a function of the inputs alone: it does not depend on launch shape or wave order.  The coverage counters use
 * integer add / min atomics, which commute; nothing else depends on an atomic's order, and the records have no append cursor.
 * In an UNKNOWN codon the edited bases and `at` are counted over the bases the transcript has.
 *
 * vsc_cds_build (host only): `contigs` is the genome's table (vsc_layout_contigs makes it, as for vsc_regions_build); every rule of SEGMENT
 * and CODING is checked, a reserved field must be 0.  VSC_ERR_INVALID when a rule is broken - vsc_cds_build_error() then names
 * the rule and the segment's index (a text of the calling thread, valid until its next vsc_cds_build) - VSC_ERR_RANGE when n is
 * above 0xFFFFFFFE, a transcript's coding length reaches 2^31 or the contigs end beyond 2^32.  n == 0 is a valid, empty set.
 * vsc_cds_info: the segments, n_tx, the transcripts that have a segment and the coding bases.  The object is immutable and
 * belongs to no context; every context that uses it keeps a device copy while it is the last one it used.
 *
 * vsc_codon_effect (host only): the class of one effect by the function the kernels call - ref, alt 0 .. 63, first_phase
 * 0 .. 2, code as CODE (NULL: standard).  It applies the rules from start_lost on as they are written, also to ref == alt;
 * unknown cannot come out.  vsc_effects_site_text (host only): ROW and EFFECTS of the one site at (contig, pos, strand) from
 * letters: texts[c] holds the letters of contig c (any case, a letter other than ACGT is an N), as many as the contig table
 * the CDS was built with says.  row[0], row[1] = the ROW (0xFFFFFFFF twice where the site's class is not defined: the locus
 * is invalid or the site holds an N); effects (room for 16, candidate = 0) and *n_effects = the EFFECTS.  The same inline
 * functions, on planes packed from the letters on every call: a definition to test against, not a fast path.
 *
 * vsc_loci_effects: loci are host entries in any order, duplicates allowed.  rows (optional): rows[2 i], rows[2 i + 1] = the ROW
 * of loci[i].  The records follow vsc_loci_edit's pair contract: *n_effects (optional) is always the full count; effects == NULL
 * only counts; a count above `capacity` is VSC_ERR_RANGE, and then nothing is written to `effects`, while rows, coverage,
 * stats and *n_effects are valid.  coverage (optional): 2 n_tx entries.  stats (optional): the candidates by class (the five
 * counts add up to n), the candidates with an effect, the effects and the effects by class, the transcripts with a stop_gained
 * effect, the rows kernel's time and the call's wall time in milliseconds.  n == 0: VSC_OK, nothing is launched, the coverage
 * says "none".  vsc_guides_effects works over the candidates where they lie on the device and requires site_len == 23;
 * vsc_pattern_guides_effects is the same for vsc_pattern_guides: site_len is the pattern's length, which the CALLER vouches for.
 * vsc_guides_filter_effects / vsc_pattern_guides_filter_effects: *out = the candidates of `in` that pass FILTER, codes and loci
 * copied unchanged in the input's order, as vsc_guides_filter_edit.
 *
 * VSC_ERR_INVALID, checked on the host before anything is written (vsc_last_error names the reason): a shape outside SHAPE or
 * with a non-zero reserved field; to > 3 or to == from; NULL arguments; a genome or object of another context; a CDS built with
 * another contig table than the genome's; a code with fewer than 64 letters; site_len != 23 for vsc_guides; require or forbid
 * with a bit above 5.  VSC_ERR_RANGE: n above 0xFFFFFFFE.  Uploads and results use context scratch;
 * vsc_ctx_release_scratch gives it back, the device copy of the CDS included.
 *
 * Not offered: overlapping isoforms in one call (call once per transcript set); splice-site disruption (pass the GT / AG
 * positions as targets of vsc_*_edit); partial-conversion outcomes; non-standard start codons; a vsc_multi_* entry.
 */
#define VSC_EFFECTS_UNDEFINED 0xFFFFFFFFu
#define VSC_EFFECT_SYNONYMOUS 0u
#define VSC_EFFECT_MISSENSE 1u
#define VSC_EFFECT_STOP_GAINED 2u
#define VSC_EFFECT_STOP_LOST 3u
#define VSC_EFFECT_START_LOST 4u
#define VSC_EFFECT_UNKNOWN 5u
#define VSC_EFFECT_CLASSES 6u
typedef struct {
    uint32_t contig, start, end, transcript;
    uint32_t strand; /* 0 '+', 1 '-' */
    uint32_t phase;  /* 0 .. 2 */
    uint32_t reserved[2]; /* 0 */
} vsc_cds_segment;
typedef struct vsc_cds vsc_cds;
typedef struct {
    uint64_t segments, transcripts, transcripts_used, coding_bases;
    uint64_t reserved[4]; /* 0 */
} vsc_cds_stats;
typedef struct {
    uint32_t candidate, transcript, codon;
    uint32_t info; /* ref | alt << 6 | class << 12 | edited << 16 | at << 20 */
} vsc_effect;
typedef struct {
    uint64_t defined, invalid, off_contig, not_resident, has_n;
    uint64_t with_effect, effects, transcripts_stopped;
    uint64_t by_class[6]; /* VSC_EFFECT_* */
    double kernel_ms, wall_ms;
} vsc_effects_stats;
#ifdef __cplusplus
static_assert(sizeof(vsc_cds_segment) == 32 && sizeof(vsc_cds_stats) == 64 && sizeof(vsc_effect) == 16 && sizeof(vsc_effects_stats) == 128,
              "vsc_effects layout");
#else
_Static_assert(sizeof(vsc_cds_segment) == 32 && sizeof(vsc_cds_stats) == 64 && sizeof(vsc_effect) == 16 && sizeof(vsc_effects_stats) == 128,
               "vsc_effects layout");
#endif
int vsc_cds_build(const vsc_contig *contigs, uint32_t n_contigs, const vsc_cds_segment *segments, uint64_t n, uint32_t n_tx, vsc_cds **out);
const char *vsc_cds_build_error(void);
void vsc_cds_free(vsc_cds *cds);
int vsc_cds_info(const vsc_cds *cds, vsc_cds_stats *out);
int vsc_codon_effect(uint32_t ref, uint32_t alt, uint32_t codon, uint32_t first_phase, const char *code /* 64 letters, or NULL */,
                     uint32_t *effect_class);
int vsc_effects_site_text(const vsc_cds *cds, const char *const *texts /* one per contig */, uint32_t contig, uint32_t pos, uint32_t strand,
                          const vsc_edit_shape *shape, uint32_t to, const char *code, uint32_t *row /* 2 */, vsc_effect *effects /* 16 */,
                          uint32_t *n_effects);
int vsc_loci_effects(vsc_ctx *ctx, const vsc_genome *genome, const vsc_locus *loci /* host, any order, duplicates allowed */, uint64_t n,
                     const vsc_edit_shape *shape, uint32_t to, const vsc_cds *cds, const char *code, uint32_t *rows /* host, 2 n, optional */,
                     vsc_effect *effects /* host, optional */, uint64_t capacity, uint64_t *n_effects /* optional */,
                     uint32_t *coverage /* host, 2 n_tx, optional */, vsc_effects_stats *stats /* optional */);
int vsc_guides_effects(vsc_ctx *ctx, const vsc_genome *genome, vsc_guides *guides, const vsc_edit_shape *shape, uint32_t to,
                       const vsc_cds *cds, const char *code, uint32_t *rows, vsc_effect *effects, uint64_t capacity, uint64_t *n_effects,
                       uint32_t *coverage, vsc_effects_stats *stats);
int vsc_pattern_guides_effects(vsc_ctx *ctx, const vsc_genome *genome, vsc_pattern_guides *guides, const vsc_edit_shape *shape, uint32_t to,
                               const vsc_cds *cds, const char *code, uint32_t *rows, vsc_effect *effects, uint64_t capacity,
                               uint64_t *n_effects, uint32_t *coverage, vsc_effects_stats *stats);
int vsc_guides_filter_effects(vsc_ctx *ctx, const vsc_genome *genome, vsc_guides *in, const vsc_edit_shape *shape, uint32_t to,
                              const vsc_cds *cds, const char *code, uint32_t require, uint32_t forbid, vsc_guides **out);
int vsc_pattern_guides_filter_effects(vsc_ctx *ctx, const vsc_genome *genome, vsc_pattern_guides *in, const vsc_edit_shape *shape,
                                      uint32_t to, const vsc_cds *cds, const char *code, uint32_t require, uint32_t forbid,
                                      vsc_pattern_guides **out);

/* ---- knock-out design: cut position, frameshift stops, nonsense-mediated decay ------------------- */
/*
 * The oldest use of a nuclease: cut inside a gene and let the repair's indel destroy the protein.  For every candidate: is its
 * cut in coding sequence, in which transcript, codon and frame, how far along the protein, how close to the exon's edge; where is
 * the first premature stop codon (PTC) when the frame shifts by +1 or +2, and does that stop lie far enough upstream of the last
 * exon-exon junction for nonsense-mediated decay (NMD) - or does the cell make a truncated protein instead.  Answered on the
 * resident genome against a CDS annotation (4.29's object), where the candidates lie.
 *
 * CODE, SEGMENT, CODING   4.29's, unchanged (one transcript set per call).
 * SHAPE     { site_len 16 .. 32, cut 1 .. site_len - 1, nmd_window 0 .. 65535, start_window 0 .. 65535 (0: rule off),
 *             max_codons 1 .. 4096, reserved 0 }.  Presets in Python only (SpCas9 23 / 17, nmd_window 50).
 * CUT       x = p + cut on '+', p + site_len - cut on '-'  (4.27's CUT COORDINATE): the break lies between forward bases x - 1 and x.
 * DEFINED   the locus is valid and the site lies inside its contig. Otherwise the row is 0xFFFFFFFF four times.
 * CODING CUT  bases x - 1 and x lie in ONE segment S (start < x < end). Otherwise the row is NONCODING:
 *             word 0 = 0xFFFFFFFF, word 1 = 0, word 2 = JUNCTION << 31, word 3 = 0, JUNCTION iff x - 1 or x lies in some segment.
 * TRANSCRIPT  t = S.transcript; shift, ci as in CODING; B_t = the transcript's coding bases; E_t = shift + B_t;
 *             J_t = ci of the first base of t's LAST segment in transcript order (t has one segment: no junction).
 * K         the coding index of the first base 3' of the break in transcript orientation: ci(x) on a '+' transcript, ci(x - 1) on '-'.
 *             codon = K / 3, frame = K % 3; frac = ((K - shift) << 16) / B_t  (0 .. 65535, 64-bit arithmetic);
 *             edge = min(x - S.start, S.end - x, 255).
 * SHIFTED   for s = 1, 2: the transcript with s bases removed behind the break. Its index j is the transcript's j for j < K, j + s otherwise.
 * WALK(s)   c = codon, codon + 1, ... at most max_codons codons. The three bases of codon c of SHIFTED(s), in transcript orientation
 *             (complemented on '-'), read across segments:
 *               an index >= E_t        -> END      (no stop inside the coding sequence)       d_s = 0xFFFF
 *               an index <  shift      -> the codon is skipped
 *               a base N / not resident-> UNKNOWN                                              d_s = 0xFFFD
 *               CODE[codon] == '*'     -> PTC at c                                             d_s = c - codon
 *             max_codons codons without any of these -> CAP                                   d_s = 0xFFFE
 * NMD(s)    PTC found, t has a junction, J_t - e >= nmd_window with e = 1 + the transcript index of the stop codon's third base,
 *             and (start_window == 0 or the transcript index of its first base - shift >= start_window).
 * ROW       four uint32:  t;  codon | frame << 30;  frac | edge << 16 | flags << 24;  d_1 | d_2 << 16.
 *             flags: 0 FIRST (S has no previous segment), 1 LAST (no next), 2 PTC1, 3 PTC2, 4 NMD1, 5 NMD2, 6 UNKNOWN (either walk), 7 = 0.
 * COVERAGE  optional, two uint32 per transcript: the candidates that cut it with NMD1 and NMD2, and the smallest codon among them
 *             (0xFFFFFFFF: none) - 4.33's PairCoverage.
 * FILTER    { min_frac, max_frac 0 .. 65535, min_edge 0 .. 255, require, forbid: masks over flag bits 0 .. 6 }: keep iff DEFINED, CODING CUT,
 *             min_frac <= frac <= max_frac, edge >= min_edge, flags & require == require, flags & forbid == 0. Survivors keep their order.
 *
 * The tests of a codon are made in the order they are written; a skipped codon counts as one of the max_codons codons; the
 * comparison J_t - e >= nmd_window is signed (a stop in the last segment has e > J_t and is never NMD).
 * Integers only.  The output is a function of the inputs alone: it does not depend on launch shape or wave order.  Only the
 * coverage uses atomics: integer add and min, which commute.
 *
 * vsc_knockout_site_text (host only): the ROW of the one site at (contig, pos, strand) from letters, as vsc_effects_site_text
 * reads them: texts[c] holds the letters of contig c (any case, a letter other than ACGT is an N).  The same inline functions
 * as the kernels', on planes packed from the letters on every call: a definition to test against, not a fast path.
 *
 * vsc_loci_knockout: loci are host entries in any order, duplicates allowed.  rows (optional): rows[4 i .. 4 i + 3] = the ROW of
 * loci[i].  coverage (optional): 2 n_tx entries.  stats (optional): the defined and the undefined candidates (they add up to
 * n), the coding cuts, the non-coding cuts at a JUNCTION, the rows with PTC1 / PTC2, with NMD1 / NMD2 and with UNKNOWN, the
 * candidates the occupancy bitmap answered without a segment search, the drains of the kernel's queue and the entries they
 * held, the transcripts with a covered candidate, the kernel's time and the call's wall time in milliseconds.  n == 0:
 * VSC_OK, nothing is launched, the coverage says "none".  vsc_guides_knockout works over the candidates where they lie on the
 * device and requires site_len == 23; vsc_pattern_guides_knockout is the same for vsc_pattern_guides: site_len is the
 * pattern's length, which the CALLER vouches for.  vsc_guides_filter_knockout / vsc_pattern_guides_filter_knockout: *out = the
 * candidates of `in` that pass FILTER, codes and loci copied unchanged in the input's order, as vsc_guides_filter_effects.
 * vsc_ctx_timing reports the kernel as score_ms and genome_bytes = 32 n for the rows.
 *
 * VSC_ERR_INVALID, checked on the host before anything is written (vsc_last_error names the reason): a value outside SHAPE or
 * a non-zero reserved field; a mask with bit 7 or above; min_frac > max_frac, max_frac > 65535, min_edge > 255; NULL arguments;
 * a genome or object of another context; a CDS built with another contig table than the genome's; a code with fewer than 64
 * letters; site_len != 23 for vsc_guides.  VSC_ERR_RANGE: n above 0xFFFFFFFE.  Uploads and results use context scratch;
 * vsc_ctx_release_scratch gives it back, the device copies of the per-transcript table and the occupancy bitmap included.
 *
 * Not offered: introns in the 3' UTR (the last junction is the last CDS junction); overlapping isoforms in one call (call once
 * per transcript set); in-frame indels (that is vsc_*_microhomology's out-of-frame share); trained indel-outcome models; a
 * vsc_multi_* entry.
 */
#define VSC_KNOCKOUT_UNDEFINED 0xFFFFFFFFu
#define VSC_KNOCKOUT_END 0xFFFFu
#define VSC_KNOCKOUT_CAP 0xFFFEu
#define VSC_KNOCKOUT_UNKNOWN 0xFFFDu
#define VSC_KNOCKOUT_FIRST 1u
#define VSC_KNOCKOUT_LAST 2u
#define VSC_KNOCKOUT_PTC1 4u
#define VSC_KNOCKOUT_PTC2 8u
#define VSC_KNOCKOUT_NMD1 16u
#define VSC_KNOCKOUT_NMD2 32u
#define VSC_KNOCKOUT_UNKNOWN_WALK 64u
typedef struct {
    uint32_t site_len, cut, nmd_window, start_window, max_codons;
    uint32_t reserved[3]; /* 0 */
} vsc_knockout_shape;
typedef struct {
    uint32_t min_frac, max_frac, min_edge;
    uint32_t require, forbid; /* masks over VSC_KNOCKOUT_FIRST .. VSC_KNOCKOUT_UNKNOWN_WALK */
    uint32_t reserved[3];     /* 0 */
} vsc_knockout_limits;
typedef struct {
    uint64_t defined, undefined;
    uint64_t coding, junction;
    uint64_t ptc[2], nmd[2]; /* frames +1, +2 */
    uint64_t unknown;
    uint64_t past_find, drains, drained;
    uint64_t transcripts_covered;
    uint64_t reserved; /* 0 */
    double kernel_ms, wall_ms;
} vsc_knockout_stats;
#ifdef __cplusplus
static_assert(sizeof(vsc_knockout_shape) == 32 && sizeof(vsc_knockout_limits) == 32 && sizeof(vsc_knockout_stats) == 128, "vsc_knockout layout");
#else
_Static_assert(sizeof(vsc_knockout_shape) == 32 && sizeof(vsc_knockout_limits) == 32 && sizeof(vsc_knockout_stats) == 128, "vsc_knockout layout");
#endif
int vsc_knockout_site_text(const vsc_cds *cds, const char *const *texts /* one per contig */, uint32_t contig, uint32_t pos, uint32_t strand,
                           const vsc_knockout_shape *shape, const char *code /* 64 letters, or NULL */, uint32_t *row /* 4 */);
int vsc_loci_knockout(vsc_ctx *ctx, const vsc_genome *genome, const vsc_locus *loci /* host, any order, duplicates allowed */, uint64_t n,
                      const vsc_knockout_shape *shape, const vsc_cds *cds, const char *code, uint32_t *rows /* host, 4 n, optional */,
                      uint32_t *coverage /* host, 2 n_tx, optional */, vsc_knockout_stats *stats /* optional */);
int vsc_guides_knockout(vsc_ctx *ctx, const vsc_genome *genome, vsc_guides *guides, const vsc_knockout_shape *shape, const vsc_cds *cds,
                        const char *code, uint32_t *rows, uint32_t *coverage, vsc_knockout_stats *stats);
int vsc_pattern_guides_knockout(vsc_ctx *ctx, const vsc_genome *genome, vsc_pattern_guides *guides, const vsc_knockout_shape *shape,
                                const vsc_cds *cds, const char *code, uint32_t *rows, uint32_t *coverage, vsc_knockout_stats *stats);
int vsc_guides_filter_knockout(vsc_ctx *ctx, const vsc_genome *genome, vsc_guides *in, const vsc_knockout_shape *shape, const vsc_cds *cds,
                               const char *code, const vsc_knockout_limits *limits, vsc_guides **out);
int vsc_pattern_guides_filter_knockout(vsc_ctx *ctx, const vsc_genome *genome, vsc_pattern_guides *in, const vsc_knockout_shape *shape,
                                       const vsc_cds *cds, const char *code, const vsc_knockout_limits *limits, vsc_pattern_guides **out);

/* ---- known variation under candidate guides: population-robust and allele-specific design -------- */
/*
 * "Does this guide's own site carry known variation, where, and how common is it?" - the join of every candidate's site with a
 * sorted list of variant intervals, on the device where the candidates lie.  Two uses: drop or down-rank guides whose
 * protospacer or PAM overlaps common variants (population-robust design), and find the guides whose PAM or seed a heterozygous
 * variant falls in, so that only one allele is cut (allele-specific design).  Integers only.
 *
 * SHAPE    site_len 16 .. 32;  zones: two bits per READ position j at bits 2 j, 2 j + 1 - the caller's label 0 .. 3 of the position
 *          (the presets of the Python layer: 1 distal, 2 seed, 3 PAM, 0 a position of no interest such as the N of NGG); accept[2]:
 *          four bits per read position (position j: nibble j & 15 of accept[j >> 4]), bit b = "read base b (A C G T) at j leaves
 *          the site usable" (the R of NNGRRT accepts A and G; protospacer positions: 0).  No bit at a position from site_len on;
 *          reserved fields 0.
 * SITE     of a locus (c, p, strand) as in vsc_loci_edit: '+': c[p, p + site_len);  '-': its reverse complement.
 * CLASS    as in vsc_loci_edit, tested in that order: invalid, not_resident, has_n, defined.  off_contig cannot occur.
 * VARIANTS n_v records of 16 bytes { contig, pos, span_alt, weight }.  span = span_alt & 0xFFFF, 1 .. 65535: the variant touches
 *          the forward bases [pos, pos + span), which lie inside the contig.  alt = span_alt >> 16 & 7: 0 .. 3 the forward-strand
 *          alternative base of an SNV (span == 1), 4 any other change (indel, MNV); other bits 0.  weight <= 0xFFFFFFFE: the
 *          caller's integer cost.  Ascending (contig, pos); TIES ARE ALLOWED (multi-allelic sites) and keep their order.  A
 *          variant's index is its place in the array.  n_v <= 0xFFFFFFFE.
 * OVERLAP  variant k overlaps a site on its contig iff pos_k < p + site_len and pos_k + span_k > p.  The touched forward positions f
 *          are the intersection; the touched read position of f is j = f - p on '+', j = site_len - 1 - (f - p) on '-'.
 * SILENT   an overlapping SNV is silent iff nibble j of accept has bit b set, b = alt on '+', b = 3 - alt on '-'.
 * DISRUPTING every other overlapping variant.
 * TOP      of an overlapping variant: the largest zone label among its touched read positions.
 * ROW      four uint32 per candidate, all 0xFFFFFFFF (VSC_VARIATION_UNDEFINED) unless the class is defined:
 *          by_zone: byte z = min(255, disrupting variants with top z);  silent: the silent variants;
 *          cost = min(0xFFFFFFFE, sum of weight over the disrupting variants) - summed in 64 bits, then clamped: a clamped sum of
 *          non-negatives does not depend on the order;  max_weight: the largest weight among them, 0 when there is none.
 * PAIR     16 bytes { candidate, variant, info, weight } per overlapping variant, silent ones included;
 *          info = smallest touched read position | touched positions << 8 | top << 16 | silent << 18.
 *          Order: ascending (candidate, variant).
 * COVERAGE optional, two uint32 per variant: its disrupting pairs and its silent pairs.
 * FILTER   keep a candidate iff it is defined, cost <= max_cost, every byte z of by_zone <= byte z of max_by_zone (255: no bound),
 *          and (require_zones == 0, or a zone z with bit z of require_zones set has a non-zero byte).  The last condition is the
 *          allele-specific mode: "at least one disrupting variant in PAM or seed".  Survivors keep their input order.
 *
 * The output is a function of the inputs alone: it does not depend on launch shape or wave order, nor on the block of the lookup
 * below.  The coverage counters use integer add atomics, which commute; nothing else depends on an atomic's order, and the pairs
 * have no append cursor: count pass over the rows, scan, write pass over tiles of 1 024 candidates.
 *
 * The lookup.  A lower bound over positions finds points, not intervals: a long deletion that starts far to the left still
 * overlaps.  At upload the device builds gpos[k] = contig offset + pos (32-bit, as everywhere) and reach[k] = max over i <= k of
 * (gpos[i] + span[i]), which never decreases.  The first variant that can overlap a site at global g0 is the first k with
 * reach[k] > g0; the walk runs from there while gpos[k] < g0 + site_len and tests OVERLAP per variant.  Variants stay inside
 * contigs and contigs lie one base apart, so global overlap is overlap on the contig.  The first k is found through a block
 * table, first[b] = the first k with reach[k] > b * 256: one table load, then a search confined to [first[b], first[b + 1]].
 *
 * vsc_variation_host is the definition on the host and needs no device: contigs gives the contig lengths (they lie one base
 * apart, as vsc_pack_genome lays them), the other arrays are host arrays.  It has no planes, so its classes are invalid and
 * defined only.  rows: 4 n words.  It goes through the functions the kernels call, the lookup included.
 *
 * vsc_loci_variation: loci are host entries in any order, duplicates allowed.  rows (optional): 4 n words.  The pairs follow
 * vsc_loci_edit's contract: *n_pairs (optional) is always the full count; pairs == NULL only counts; a count above `capacity` is
 * VSC_ERR_RANGE, and then nothing is written to `pairs`, while rows, coverage, stats and *n_pairs are valid.  coverage (optional):
 * 2 n_v entries.  stats (optional): the candidates by class (the five counts add up to n), the candidates with a disrupting
 * variant, the pairs, the variants with a pair, the rows kernel's time and the call's wall time in milliseconds.  n == 0: VSC_OK,
 * nothing is launched, the coverage is 0.  vsc_guides_variation works over the candidates where they lie on the device and
 * requires site_len == 23; the host-only object of vsc_multi_guides_enumerate goes the vsc_loci_variation way.
 * vsc_pattern_guides_variation is the same for vsc_pattern_guides: the CALLER vouches for site_len, as in the edit calls.
 *
 * vsc_guides_filter_variation / vsc_pattern_guides_filter_variation: *out = the candidates of `in` that pass FILTER - codes and
 * loci copied unchanged, in the input's order; `in` stays as it is.  Count pass, scan, write pass, as vsc_guides_filter_edit.
 *
 * VSC_ERR_INVALID, checked on the host before anything is written (vsc_last_error names the reason): a shape outside SHAPE or
 * with a non-zero reserved field; a filter with require_zones > 15 or a non-zero reserved field; variants not ascending; on an
 * unknown contig; a span of 0 or beyond its contig; alt 0 .. 3 with span != 1; alt > 4 or other bits of span_alt; a weight of
 * 0xFFFFFFFF; NULL arguments; a genome or object of another context; site_len != 23 for vsc_guides.  VSC_ERR_RANGE: n or n_v above
 * 0xFFFFFFFE; more than 0xFFFFFFFE pairs.  Uploads and results use context scratch; vsc_ctx_release_scratch gives it back.
 *
 * Not offered: a vsc_multi_* entry; guides that exist only on the alternative allele (PAM-creating variants) - enumerate over
 * the alternative-allele windows genome (vsc_windows_build) for those; genotype or phase handling: every variant stands alone.
 */
#define VSC_VARIATION_UNDEFINED 0xFFFFFFFFu
#define VSC_VARIANT_OTHER 4u
typedef struct {
    uint32_t site_len;
    uint32_t reserved0; /* 0 */
    uint64_t zones;
    uint64_t accept[2];
    uint32_t reserved[4]; /* 0 */
} vsc_variation_shape;
typedef struct {
    uint32_t contig, pos;
    uint32_t span_alt; /* span | alt << 16 */
    uint32_t weight;
} vsc_variant;
typedef struct {
    uint32_t candidate, variant;
    uint32_t info; /* first | touched << 8 | top << 16 | silent << 18 */
    uint32_t weight;
} vsc_variation_pair;
typedef struct {
    uint32_t max_cost;
    uint32_t max_by_zone; /* byte z: the bound of zone z, 255 = none */
    uint32_t require_zones; /* bit z: zone z; 0: nothing is required */
    uint32_t reserved; /* 0 */
} vsc_variation_filter;
typedef struct {
    uint64_t defined, invalid, off_contig, not_resident, has_n;
    uint64_t with_disrupting, pairs, variants_covered;
    double kernel_ms, wall_ms;
    uint64_t reserved[2]; /* 0 */
} vsc_variation_stats;
#ifdef __cplusplus
static_assert(sizeof(vsc_variation_shape) == 48 && sizeof(vsc_variant) == 16 && sizeof(vsc_variation_pair) == 16 &&
              sizeof(vsc_variation_filter) == 16 && sizeof(vsc_variation_stats) == 96, "vsc_variation_* layout");
#else
_Static_assert(sizeof(vsc_variation_shape) == 48 && sizeof(vsc_variant) == 16 && sizeof(vsc_variation_pair) == 16 &&
               sizeof(vsc_variation_filter) == 16 && sizeof(vsc_variation_stats) == 96, "vsc_variation_* layout");
#endif
int vsc_variation_host(const vsc_contig *contigs, uint32_t n_contigs, const vsc_locus *loci, uint64_t n, const vsc_variation_shape *shape,
                       const vsc_variant *variants, uint64_t n_v, uint32_t *rows /* 4 n, optional */, vsc_variation_pair *pairs /* optional */,
                       uint64_t capacity, uint64_t *n_pairs /* optional */, uint32_t *coverage /* 2 n_v, optional */);
int vsc_loci_variation(vsc_ctx *ctx, const vsc_genome *genome, const vsc_locus *loci /* host, any order, duplicates allowed */, uint64_t n,
                       const vsc_variation_shape *shape, const vsc_variant *variants /* host */, uint64_t n_v,
                       uint32_t *rows /* host, 4 n, optional */, vsc_variation_pair *pairs /* host, optional */, uint64_t capacity,
                       uint64_t *n_pairs /* optional */, uint32_t *coverage /* host, 2 n_v, optional */, vsc_variation_stats *stats /* optional */);
int vsc_guides_variation(vsc_ctx *ctx, const vsc_genome *genome, vsc_guides *guides, const vsc_variation_shape *shape,
                         const vsc_variant *variants, uint64_t n_v, uint32_t *rows, vsc_variation_pair *pairs, uint64_t capacity,
                         uint64_t *n_pairs, uint32_t *coverage, vsc_variation_stats *stats);
int vsc_pattern_guides_variation(vsc_ctx *ctx, const vsc_genome *genome, vsc_pattern_guides *guides, const vsc_variation_shape *shape,
                                 const vsc_variant *variants, uint64_t n_v, uint32_t *rows, vsc_variation_pair *pairs, uint64_t capacity,
                                 uint64_t *n_pairs, uint32_t *coverage, vsc_variation_stats *stats);
int vsc_guides_filter_variation(vsc_ctx *ctx, const vsc_genome *genome, vsc_guides *in, const vsc_variation_shape *shape,
                                const vsc_variant *variants, uint64_t n_v, const vsc_variation_filter *filter, vsc_guides **out);
int vsc_pattern_guides_filter_variation(vsc_ctx *ctx, const vsc_genome *genome, vsc_pattern_guides *in, const vsc_variation_shape *shape,
                                        const vsc_variant *variants, uint64_t n_v, const vsc_variation_filter *filter,
                                        vsc_pattern_guides **out);

/* ---- prime-editing guide design: pegRNA extensions per edit --------------------------------------- */
/*
 * Prime editors write substitutions, insertions and deletions behind a nick.  "Which candidates nick close enough upstream of my
 * edit, what primer binding site (PBS) and reverse-transcriptase template (RTT) does the 3' extension need, does the edit
 * destroy the PAM or the seed, does the extension hold a poly-T terminator?" - answered on the resident genome, where the
 * candidates lie.  Everything is integer; device, host and a restatement on strings agree to the bit.
 *
 * SHAPE    site_len 16 .. 32;  down 0 .. 64 - site_len: bases of context behind the site in read orientation; C = site_len + down.
 *          nick 1 .. site_len: the nick lies between read positions nick - 1 and nick (SpCas9 23-mer: 17).
 *          1 <= pbs_min <= pbs_max <= nick;  1 <= rtt_min <= rtt_max <= C - nick;  pbs_max + rtt_max <= 64;
 *          min_homology 0 .. rtt_max;  pam_start, pam_len and seed_start, seed_len: two ranges of read positions inside the site,
 *          len 0 .. 8 (0: that flag is never set);  flags bit 0 AVOID_G_END;  reserved fields 0.
 *          STABILITY: int32 init, mono[4], di[16], target, every |weight| <= 2^20.
 * CONTEXT  of a locus (c, p, strand): eff_context with up = 0: '+': R = c[p, p + C);  '-': R = revcomp(c[p - down, p + site_len)).
 *          F0 = the context's first forward position (p, or p - down).  CLASS as EffClass, in its order; off_contig CAN occur.
 * PBS      S(L) = init + sum mono[R[j]], j in [nick - L, nick) + sum di[4 R[j] + R[j+1]], j in [nick - L, nick - 1).
 *          pbs_len = the smallest L in [pbs_min, pbs_max] with S(L) >= target; none: pbs_len = pbs_max and WEAK.
 *          pbs_gc = the G/C among R[nick - pbs_len, nick).
 * EDITS    n_e entries { contig, pos, del_len 0 .. 16, ins_len 0 .. 16, ins }: forward bases [pos, pos + del_len) are replaced by
 *          ins_len letters (2-bit code, letter k in bits 2k+1 .. 2k, the bits above them 0); del_len + ins_len >= 1;
 *          pos + del_len <= the contig's length;  STRICTLY ascending by (contig, pos);  n_e <= 0xFFFFFFFE.
 *          The replaced letters are not compared with ins (a substitution that writes the letter already there is the caller's business).
 *          Every pair treats its edit alone; edits do not combine.
 * READ     an edit is IN REACH of a defined candidate on its contig iff [pos, pos + del_len) lies inside [F0, F0 + C)
 *          (del_len 0: F0 <= pos <= F0 + C) and e0 >= nick, with
 *          '+': e0 = pos - F0, I = ins;   '-': e0 = C - (pos - F0) - del_len, I = revcomp(ins).
 *          E = R[0, e0) + I + R[e0 + del_len, C): the edited strand in read orientation;  d = e0 - nick.
 * RTT      t0 = max(rtt_min, d + ins_len + min_homology).  t = t0, or under AVOID_G_END the smallest t >= t0 with
 *          E[nick + t - 1] != G (a position beyond E counts as not G).  The pair EXISTS iff t <= rtt_max and nick + t <= |E|.
 *          h = t - d - ins_len.
 * FLAGS    bit 0 PAM: E[q] != R[q] for some q of the pam range (q >= |E| counts as different);  bit 1 SEED: the same over the
 *          seed range;  bit 2 POLY_T: E[nick - pbs_len, nick + t) holds four or more A in a row (the extension is its reverse
 *          complement);  bit 3 WEAK (the candidate's).
 * ROW      two uint32 per candidate: pbs = pbs_len | pbs_gc << 8 | WEAK << 16, and n_pairs.  Both 0xFFFFFFFF unless defined.
 *          Without edits n_pairs = 0.
 * PAIR     16 bytes { candidate, edit, info = t | d << 8 | h << 16 | flags << 24, ext = (pbs_len + t) | ext_gc << 8 | pbs_len << 16 },
 *          ext_gc = the G/C of E[nick - pbs_len, nick + t).  Order: ascending (candidate, edit).  n <= 0xFFFFFFFE.
 * COVERAGE optional, two uint32 per edit: its number of pairs and the smallest t among them (0xFFFFFFFF: none).
 * FILTER   keep iff defined, (no edits given or n_pairs >= 1), and (allow_weak or not WEAK).  Survivors keep their input order.
 * EXTENSION (host) revcomp(E[nick - pbs_len, nick + t)) as DNA letters: RTT then PBS, 5' to 3'.
 *
 * The output is a function of the inputs alone: it does not depend on launch shape or wave order.  The coverage and the pairs by
 * flag use integer add / min atomics, which commute; nothing else depends on an atomic's order, and the pairs have no append
 * cursor.  An occupancy bitmap over the edits' positions (one bit per 256 global positions) is asked before any search; it
 * changes no output bit.
 *
 * vsc_prime_site_text: one context of C letters (any case) in read orientation and one edit in READ coordinates (e0, del_len, the
 * inserted letters as the read strand has them, "" for none) on the host, by the functions the kernels call.  row[0] = the pbs
 * word, row[1] = 1 if the pair exists and 0 otherwise; then pair[0] = info, pair[1] = ext, and extension (optional, at least 65
 * bytes) holds the EXTENSION text.  The edit is optional (ins == NULL: the row's word alone, row[1] = 0).  A letter other than
 * ACGT, a text of another length, a shape outside SHAPE, an edit outside [0, C] or longer than 16: VSC_ERR_INVALID.  An edit with
 * e0 < nick is not in reach: row[1] = 0.
 *
 * vsc_loci_prime: loci are host entries in any order, duplicates allowed.  rows (optional): rows[2 i], rows[2 i + 1] = pbs, n_pairs
 * of loci[i].  The pairs follow vsc_loci_edit's contract: *n_pairs (optional) is always the full count; pairs == NULL only counts;
 * a count above `capacity` is VSC_ERR_RANGE, and then nothing is written to `pairs`, while rows, coverage, stats and *n_pairs
 * are valid.  coverage (optional): 2 n_e entries.  stats (optional): the candidates by class (the five counts add up to n), the
 * candidates with a pair, the weak candidates, the pairs, the pairs by flag (PAM, SEED, POLY_T, WEAK), the edits with a pair, the
 * rows kernel's time and the call's wall time in milliseconds.  n == 0: VSC_OK, nothing is launched, the coverage says "no pair".
 * vsc_guides_prime works over the candidates where they lie on the device - no locus travels - and requires site_len == 23; the
 * host-only object of vsc_multi_guides_enumerate goes the vsc_loci_prime way.  vsc_pattern_guides_prime is the same for
 * vsc_pattern_guides: site_len is the pattern's length, which the CALLER vouches for, as in the pick calls.
 *
 * vsc_guides_filter_prime / vsc_pattern_guides_filter_prime: *out = the candidates of `in` that pass FILTER - codes and loci
 * copied unchanged, in the input's order; `in` stays as it is.  Count pass, scan, write pass over tiles of 1 024 candidates.
 *
 * VSC_ERR_INVALID, checked on the host before anything is written (vsc_last_error names the reason): a shape outside SHAPE or
 * with a non-zero reserved field; NULL arguments; a genome or object of another context; site_len != 23 for vsc_guides; edits
 * not strictly ascending, on an unknown contig, or reaching beyond their contig; del_len or ins_len above 16, or both 0;
 * insertion bits above ins_len; n_e > 0 with NULL edits.  VSC_ERR_RANGE: n or n_e above 0xFFFFFFFE.  Uploads and results use
 * context scratch; vsc_ctx_release_scratch gives it back.
 *
 * Not offered: a vsc_multi_* entry; several alleles at one position in one call (call once per allele set); more than one RTT
 * length per pair (call again with another rtt_min); PE3 second-nick guides (vsc_loci_pairs with a delta range gives the
 * opposite-strand candidates); efficiency models with trained weights; a shipped thermodynamic table (the caller brings mono /
 * di); pegRNA scaffold or 3' motif text.
 */
#define VSC_PRIME_UNDEFINED 0xFFFFFFFFu
#define VSC_PRIME_AVOID_G_END 1u
#define VSC_PRIME_FLAG_PAM 1u
#define VSC_PRIME_FLAG_SEED 2u
#define VSC_PRIME_FLAG_POLY_T 4u
#define VSC_PRIME_FLAG_WEAK 8u
typedef struct {
    uint32_t site_len, down, nick;
    uint32_t pbs_min, pbs_max, rtt_min, rtt_max, min_homology;
    uint32_t pam_start, pam_len, seed_start, seed_len;
    uint32_t flags; /* VSC_PRIME_AVOID_G_END */
    int32_t init, mono[4], di[16], target; /* STABILITY */
    uint32_t reserved[5]; /* 0 */
} vsc_prime_shape;
typedef struct {
    uint32_t contig, pos;
    uint16_t del_len, ins_len;
    uint32_t ins; /* letter k in bits 2k+1 .. 2k */
} vsc_prime_edit;
typedef struct {
    uint32_t candidate, edit;
    uint32_t info; /* t | d << 8 | h << 16 | flags << 24 */
    uint32_t ext;  /* (pbs_len + t) | ext_gc << 8 | pbs_len << 16 */
} vsc_prime_pair;
typedef struct {
    uint64_t defined, invalid, off_contig, not_resident, has_n;
    uint64_t with_pair, weak, pairs;
    uint64_t pairs_by_flag[4]; /* PAM, SEED, POLY_T, WEAK */
    uint64_t edits_covered;
    double score_ms, wall_ms;
    uint64_t reserved; /* 0 */
} vsc_prime_stats;
#ifdef __cplusplus
static_assert(sizeof(vsc_prime_shape) == 160 && sizeof(vsc_prime_edit) == 16 && sizeof(vsc_prime_pair) == 16 && sizeof(vsc_prime_stats) == 128,
              "vsc_prime_* layout");
#else
_Static_assert(sizeof(vsc_prime_shape) == 160 && sizeof(vsc_prime_edit) == 16 && sizeof(vsc_prime_pair) == 16 && sizeof(vsc_prime_stats) == 128,
               "vsc_prime_* layout");
#endif
int vsc_prime_site_text(const char *context /* C letters, read orientation, any case */, const vsc_prime_shape *shape, uint32_t e0,
                        uint32_t del_len, const char *ins /* read orientation, "" for none; NULL: no edit */, uint32_t *row /* 2 */,
                        uint32_t *pair /* 2, optional */, char *extension /* >= 65 bytes, optional */);
int vsc_loci_prime(vsc_ctx *ctx, const vsc_genome *genome, const vsc_locus *loci /* host, any order, duplicates allowed */, uint64_t n,
                   const vsc_prime_shape *shape, const vsc_prime_edit *edits /* host */, uint64_t n_e, uint32_t *rows /* host, 2 n, optional */,
                   vsc_prime_pair *pairs /* host, optional */, uint64_t capacity, uint64_t *n_pairs /* optional */,
                   uint32_t *coverage /* host, 2 n_e, optional */, vsc_prime_stats *stats /* optional */);
int vsc_guides_prime(vsc_ctx *ctx, const vsc_genome *genome, vsc_guides *guides, const vsc_prime_shape *shape,
                     const vsc_prime_edit *edits, uint64_t n_e, uint32_t *rows, vsc_prime_pair *pairs, uint64_t capacity,
                     uint64_t *n_pairs, uint32_t *coverage, vsc_prime_stats *stats);
int vsc_pattern_guides_prime(vsc_ctx *ctx, const vsc_genome *genome, vsc_pattern_guides *guides, const vsc_prime_shape *shape,
                             const vsc_prime_edit *edits, uint64_t n_e, uint32_t *rows, vsc_prime_pair *pairs, uint64_t capacity,
                             uint64_t *n_pairs, uint32_t *coverage, vsc_prime_stats *stats);
int vsc_guides_filter_prime(vsc_ctx *ctx, const vsc_genome *genome, vsc_guides *in, const vsc_prime_shape *shape,
                            const vsc_prime_edit *edits, uint64_t n_e, uint32_t allow_weak, vsc_guides **out);
int vsc_pattern_guides_filter_prime(vsc_ctx *ctx, const vsc_genome *genome, vsc_pattern_guides *in, const vsc_prime_shape *shape,
                                    const vsc_prime_edit *edits, uint64_t n_e, uint32_t allow_weak, vsc_pattern_guides **out);

/* ---- HDR knock-in design: reach, re-cut block, silent changes ------------------------------------- */
/*
 * A nuclease cut repaired from a donor template (homology-directed repair, often with a single-stranded oligo donor): "which
 * candidates cut close enough to my edit, does the edit itself keep the nuclease from cutting the repaired allele again, and if
 * not, which single silent substitution in the donor would?" - answered on the resident genome, where the candidates lie.
 * Everything is integer.  Letters are A C G T = 0 .. 3.
 *
 * SHAPE    site_len 16 .. 32; up 0 .. 32, down 0 .. 32; C = up + site_len + down <= 64. The site is context positions
 *          [s0, s0 + site_len), s0 = up; "site position q" is context position s0 + q.
 *          cut 1 .. site_len - 1: the break lies between site positions cut - 1 and cut; K = s0 + cut (SpCas9 23-mer: cut 17).
 *          max_dist 0 .. 63.   anchor 0 | 1: the side of the site the PAM fixes (1: its last base, SpCas9; 0: its first, Cas12a).
 *          pam_start, pam_len 0 .. 8, inside the site; pam_accept[8]: for j < pam_len a non-empty set of letters, bit b = letter
 *          b (NGG: 15, 4, 4); 0 for j >= pam_len.
 *          seed_start, seed_len 0 .. 16 and proto_start, proto_len 0 .. 32: two ranges of site positions inside the site.
 *          min_seed_mm 0 .. seed_len, min_proto_mm 0 .. proto_len (0: that rule is off).
 *          flags bit 0 SUBSTITUTE, bit 1 SUB_SEED, bit 2 SUB_NONCODING; every other bit and every reserved field 0.
 * CONTEXT  eff_context with {up, site_len, down}: '+': R = c[p - up, p + site_len + down); '-': R = revcomp(c[p - down, p + site_len + up)).
 *          F0 = the context's first forward position. CLASS as EffClass, in its order.
 * EDITS    vsc_prime_edit entries under 4.30's rules (strictly ascending (contig, pos), del_len and ins_len 0 .. 16, not both 0,
 *          inside the contig, n_e <= 0xFFFFFFFE). Every pair treats its edit alone.
 * READ     e0 and I as in 4.30 ('+': e0 = pos - F0, I = ins; '-': e0 = C - (pos - F0) - del_len, I = revcomp(ins)); e1 = e0 + del_len.
 *          dist = 0 when e0 <= K <= e1, K - e1 when e1 < K, e0 - K when e0 > K. side = 0 | 1 | 2 in that order.
 *          The edit is IN REACH of a defined candidate on its contig iff [pos, pos + del_len) lies inside [F0, F0 + C)
 *          (del_len 0: F0 <= pos <= F0 + C) and dist <= max_dist.
 *          E = R[0, e0) + I + R[e1, C); delta = ins_len - del_len; |E| = C + delta.
 * SEEN     what the nuclease finds on the repaired allele, held at the PAM side:
 *          shift = delta when (anchor = 1 and e0 < s0 + site_len) or (anchor = 0 and e1 <= s0), otherwise 0.
 *          S[q] = E[s0 + q + shift] for q in [0, site_len). An index outside [0, |E|) gives NO LETTER, which differs from every
 *          letter and is in no pam_accept set.
 * BLOCKED  pam_broken = some j < pam_len with S[pam_start + j] not in pam_accept[j].
 *          seed_mm / proto_mm = the q of that range with S[q] != R[s0 + q].
 *          flag bit 0 B_PAM = pam_broken; bit 1 B_SEED = min_seed_mm != 0 and seed_mm >= min_seed_mm; bit 2 B_PROTO likewise.
 *          The pair is BLOCKED when one of them is set. (pam_broken speaks about S, not about a change: the caller vouches that the
 *          candidates' own PAM is in pam_accept.)
 * SUBSTITUTE  only under SUBSTITUTE and when the pair is not BLOCKED: ONE substitution of one base that the donor carries beside
 *          the edit. A site position q is a SLOT when x = s0 + q + shift lies in [0, |E|) and not in [e0, e0 + ins_len) (an
 *          inserted letter is not a slot); its reference context position is r = x (x < e0) or x - delta; its forward position
 *          f = F0 + r ('+') or F0 + C - 1 - r ('-'); the forward letter of a read letter b is b ('+') or 3 - b ('-').
 *          ALLOWED(r, b): without a CDS always. With one: f lies in no segment -> SUB_NONCODING. f lies in a segment -> all of:
 *            its codon is not UNKNOWN (4.29)
 *            none of the codon's three forward positions g has pos <= g + 1 and g <= pos + del_len
 *              (the codon does not touch the edit, one base of margin for an insertion point)
 *            CODE[ref] == CODE[alt], alt = the reference codon with that one base replaced
 *              (transcript orientation; complemented when the strands differ)
 *          Frameshifting edits do not move the frame the substitution is judged in (see "Not offered").
 *          ORDER of the tries, the first that holds is taken:
 *            1. j = 0 .. pam_len - 1 ascending, q = pam_start + j a slot, b = 0 .. 3 ascending with b not in pam_accept[j] and
 *               ALLOWED(r, b)                                                                       -> flag bit 3 SUB_PAM
 *            2. under SUB_SEED, when min_seed_mm != 0 and seed_mm + 1 >= min_seed_mm: the seed's q from the PAM side outward
 *               (anchor 1: descending, anchor 0: ascending), q a slot with S[q] == R[s0 + q], b ascending with b != R[s0 + q] and
 *               ALLOWED(r, b)                                                                       -> flag bit 4 SUB_SEED
 *          none: flag bit 5 OPEN (the repaired allele can be cut again). A pair is USABLE when it is not OPEN.
 *          Without SUBSTITUTE a pair that is not BLOCKED is OPEN.
 * PAIR     16 bytes { candidate, edit, info, block }; info = dist | side << 6 | seed_mm << 8 | proto_mm << 13 | flags << 24;
 *          block = 0xFFFFFFFF without a substitution, else q | b << 8 | coding << 10 | r << 16 (coding: f lies in a segment).
 *          Order: ascending (candidate, edit). n <= 0xFFFFFFFE.
 * ROW      two uint32 per candidate: n_pairs, n_usable. Both 0xFFFFFFFF unless defined. Without edits both 0.
 * COVERAGE optional, two uint32 per edit: its USABLE pairs and the smallest dist among them (0xFFFFFFFF: none).
 * FILTER   keep iff defined and (no edits given, or n_usable >= 1, or allow_open and n_pairs >= 1). Survivors keep their order.
 *
 * The output is a function of the inputs alone: it does not depend on launch shape or wave order.  The coverage and the pairs by
 * flag use integer add / min atomics, which commute; the pairs have no append cursor.  The occupancy bitmap over the edits'
 * positions (4.30) is asked before any search; it changes no output bit.  The CDS is read only for a pair that is in reach and
 * not BLOCKED.
 *
 * vsc_hdr_site_text: one context of C letters (any case) in read orientation and one edit in READ coordinates (e0, del_len, the
 * inserted letters as the read strand has them, "" for none) on the host, by the functions the kernels call.  allowed (optional):
 * C bytes, byte r = the set of read letters ALLOWED at reference context position r (bit b = letter b); NULL: every letter
 * everywhere.  pair[0] = info, pair[1] = block (coding is 0: there is no CDS); both 0xFFFFFFFF when the edit is not in reach.
 * edited (optional, at least 81 bytes): E with the substitution applied, as letters.  A letter other than ACGT, a text of another
 * length, a shape outside SHAPE, an edit outside [0, C] or longer than 16, a set above 15: VSC_ERR_INVALID.
 *
 * vsc_loci_hdr: vsc_loci_prime's arguments, with an optional CDS (NULL: ALLOWED always holds) and CODE (NULL: the standard code)
 * as vsc_loci_effects takes them.  rows (optional): rows[2 i], rows[2 i + 1] = n_pairs, n_usable of loci[i].  The pairs follow
 * vsc_loci_edit's contract: *n_pairs (optional) is always the full count; pairs == NULL only counts; a count above `capacity` is
 * VSC_ERR_RANGE, and then nothing is written to `pairs`, while rows, coverage, stats and *n_pairs are valid.  stats (optional):
 * the candidates by class, those with a pair and with a usable pair, the pairs, the pairs by flag (B_PAM, B_SEED, B_PROTO, SUB_PAM,
 * SUB_SEED, OPEN), the edits with a usable pair, the rows kernel's time and the call's wall time in milliseconds.  n == 0: VSC_OK,
 * nothing is launched.  vsc_guides_hdr works over the candidates where they lie on the device and requires site_len == 23; a
 * host-only object goes the vsc_loci_hdr way.  vsc_pattern_guides_hdr is the same for vsc_pattern_guides: site_len is the
 * pattern's length, which the CALLER vouches for.
 *
 * vsc_guides_filter_hdr / vsc_pattern_guides_filter_hdr: *out = the candidates of `in` that pass FILTER - codes and loci copied
 * unchanged, in the input's order; `in` stays as it is.  Count pass, scan, write pass over tiles of 1 024 candidates.
 *
 * VSC_ERR_INVALID, checked on the host before anything is written (vsc_last_error names the reason): a shape outside SHAPE or
 * with a non-zero reserved field; NULL arguments; a genome or object of another context; a CDS built for another contig table; a
 * code of fewer than 64 letters; site_len != 23 for vsc_guides; the refusals of EDITS as in 4.30.  VSC_ERR_RANGE: n or n_e above
 * 0xFFFFFFFE.  Uploads and results use context scratch; vsc_ctx_release_scratch gives it back.
 *
 * Not offered: several substitutions per pair; frame-aware judgement of a substitution behind a frameshifting edit; homology
 * arms or the donor's strand on the device (va.hdr_donor cuts the arms on the host); a vsc_multi_* entry; trained HDR-efficiency
 * models.
 */
#define VSC_HDR_UNDEFINED 0xFFFFFFFFu
#define VSC_HDR_NO_BLOCK 0xFFFFFFFFu
#define VSC_HDR_SUBSTITUTE 1u
#define VSC_HDR_SUB_SEED 2u
#define VSC_HDR_SUB_NONCODING 4u
#define VSC_HDR_FLAG_B_PAM 1u
#define VSC_HDR_FLAG_B_SEED 2u
#define VSC_HDR_FLAG_B_PROTO 4u
#define VSC_HDR_FLAG_SUB_PAM 8u
#define VSC_HDR_FLAG_SUB_SEED 16u
#define VSC_HDR_FLAG_OPEN 32u
typedef struct {
    uint32_t up, site_len, down, cut, max_dist, anchor;
    uint32_t pam_start, pam_len, pam_accept[8];
    uint32_t seed_start, seed_len, proto_start, proto_len, min_seed_mm, min_proto_mm;
    uint32_t flags; /* VSC_HDR_SUBSTITUTE | VSC_HDR_SUB_SEED | VSC_HDR_SUB_NONCODING */
    uint32_t reserved; /* 0 */
} vsc_hdr_shape;
typedef struct {
    uint32_t candidate, edit;
    uint32_t info;  /* dist | side << 6 | seed_mm << 8 | proto_mm << 13 | flags << 24 */
    uint32_t block; /* VSC_HDR_NO_BLOCK, or q | b << 8 | coding << 10 | r << 16 */
} vsc_hdr_pair;
typedef struct {
    uint64_t defined, invalid, off_contig, not_resident, has_n;
    uint64_t with_pair, with_usable, pairs;
    uint64_t pairs_by_flag[6]; /* B_PAM, B_SEED, B_PROTO, SUB_PAM, SUB_SEED, OPEN */
    uint64_t edits_covered;
    double score_ms, wall_ms;
    uint64_t reserved; /* 0 */
} vsc_hdr_stats;
#ifdef __cplusplus
static_assert(sizeof(vsc_hdr_shape) == 96 && sizeof(vsc_hdr_pair) == 16 && sizeof(vsc_hdr_stats) == 144, "vsc_hdr_* layout");
#else
_Static_assert(sizeof(vsc_hdr_shape) == 96 && sizeof(vsc_hdr_pair) == 16 && sizeof(vsc_hdr_stats) == 144, "vsc_hdr_* layout");
#endif
int vsc_hdr_site_text(const char *context /* C letters, read orientation, any case */, const vsc_hdr_shape *shape, uint32_t e0,
                      uint32_t del_len, const char *ins /* read orientation, "" for none */,
                      const uint8_t *allowed /* C bytes of letter sets, or NULL */, uint32_t *pair /* 2: info, block */,
                      char *edited /* >= 81 bytes, optional */);
int vsc_loci_hdr(vsc_ctx *ctx, const vsc_genome *genome, const vsc_locus *loci /* host, any order, duplicates allowed */, uint64_t n,
                 const vsc_hdr_shape *shape, const vsc_prime_edit *edits /* host */, uint64_t n_e, const vsc_cds *cds /* optional */,
                 const char *code /* 64 letters, or NULL */, uint32_t *rows /* host, 2 n, optional */,
                 vsc_hdr_pair *pairs /* host, optional */, uint64_t capacity, uint64_t *n_pairs /* optional */,
                 uint32_t *coverage /* host, 2 n_e, optional */, vsc_hdr_stats *stats /* optional */);
int vsc_guides_hdr(vsc_ctx *ctx, const vsc_genome *genome, vsc_guides *guides, const vsc_hdr_shape *shape, const vsc_prime_edit *edits,
                   uint64_t n_e, const vsc_cds *cds, const char *code, uint32_t *rows, vsc_hdr_pair *pairs, uint64_t capacity,
                   uint64_t *n_pairs, uint32_t *coverage, vsc_hdr_stats *stats);
int vsc_pattern_guides_hdr(vsc_ctx *ctx, const vsc_genome *genome, vsc_pattern_guides *guides, const vsc_hdr_shape *shape,
                           const vsc_prime_edit *edits, uint64_t n_e, const vsc_cds *cds, const char *code, uint32_t *rows,
                           vsc_hdr_pair *pairs, uint64_t capacity, uint64_t *n_pairs, uint32_t *coverage, vsc_hdr_stats *stats);
int vsc_guides_filter_hdr(vsc_ctx *ctx, const vsc_genome *genome, vsc_guides *in, const vsc_hdr_shape *shape, const vsc_prime_edit *edits,
                          uint64_t n_e, const vsc_cds *cds, const char *code, uint32_t allow_open, vsc_guides **out);
int vsc_pattern_guides_filter_hdr(vsc_ctx *ctx, const vsc_genome *genome, vsc_pattern_guides *in, const vsc_hdr_shape *shape,
                                  const vsc_prime_edit *edits, uint64_t n_e, const vsc_cds *cds, const char *code, uint32_t allow_open,
                                  vsc_pattern_guides **out);

/* ---- guide RNA self-complementarity: hairpin and scaffold stems --------------------------------- */
/*
 * "Will this guide RNA fold back on itself, or onto its own constant part?": the count of stems a spacer can form with
 * itself and with the scaffold text the caller brings (the sgRNA scaffold, the Cas12a direct repeat, a pegRNA's scaffold with
 * its extension) - the "self-complementarity" column of guide-design tools.  A relation between two positions of the same
 * guide, which no model of the other families can express.  This text is normative; everything is integer.  Letters are
 * A C G T = 0 .. 3, and U is read as T.
 *
 * SHAPE    site_len 16 .. 32.  proto_start, proto_len 12 .. 32 with proto_start + proto_len <= site_len: the site positions (read
 *          orientation) that become the guide RNA's spacer; n = proto_len.  (SpCas9 23-mer: 0, 20; Cas12a 27-mer: 4, 23.)
 *          stem k 3 .. 8;  gc_min 0 .. k;  min_loop 0 .. 16.
 *          seed_start, seed_len 0 .. 16 in SPACER positions, seed_start + seed_len <= n (seed_len 0: no seed).
 *          flags bit 0 WOBBLE; every other bit and every reserved field 0.
 * SCAFFOLD m letters s[0, m), 5' to 3', m 0 .. 128, A C G T U in any case; any other letter is refused.  It is the launch's, not
 *          the candidate's.  The library ships none.
 * SPACER   g[0, n) = the site of locus (c, p, strand) in read orientation ('+': c[p, p + site_len), '-': its reverse complement),
 *          positions [proto_start, proto_start + n).  CLASS as EffClass, in its order (off_contig cannot occur and stays 0).
 * PAIR(a, b)   a + b == 3; under WOBBLE also {a, b} == {G, T}.
 * SELF STEM (i, j, L)      0 <= i, i + L + min_loop <= j, j + L <= n, PAIR(g[i + t], g[j + L - 1 - t]) for t in [0, L).
 * SCAFFOLD STEM (i, j, L)  i + L <= n, j + L <= m,                  PAIR(g[i + t], s[j + L - 1 - t]) for t in [0, L).
 * QUAL(i)      the k-mer g[i, i + k), i in [0, n - k], holds at least gc_min letters G or C.
 * SELF5(i)     a self stem (i, j, k) exists.        SCAF(i)   a scaffold stem (i, j, k) exists.
 * self_starts  #{ i : QUAL(i) and SELF5(i) }
 * scaf_starts  #{ i : QUAL(i) and SCAF(i) }
 * starts       #{ i : QUAL(i) and (SELF5(i) or SCAF(i)) }   (the form of CHOPCHOP's count: k = 4, gc_min = 2)
 * COVERED      the union of [i, i + k) and [j, j + k) over self stems (i, j, k) with QUAL(i), and of [i, i + k) over scaffold stems
 *              (i, j, k) with QUAL(i).
 * seed_paired  # of COVERED positions inside [seed_start, seed_start + seed_len)
 * self_longest the largest L for which a self stem (i, j, L) exists (any G/C content), 0 when none
 * scaf_longest the largest L for which a scaffold stem (i, j, L) exists, 0 when none (m == 0: 0)
 * ROW      two uint32 per candidate: w0 = starts | self_starts << 8 | scaf_starts << 16 | seed_paired << 24,
 *          w1 = self_longest | scaf_longest << 8.  Both 0xFFFFFFFF (VSC_FOLD_UNDEFINED) unless the class is defined.
 * FILTER   limits max_starts, max_self_longest, max_scaf_longest, max_seed_paired, each 0 .. 32 or 0xFFFFFFFF (no limit):
 *          keep iff defined and every value <= its limit.  Survivors keep their order.
 *
 * No bit parity with CHOPCHOP's script is claimed: its loop bounds carry quirks of their own.  Device, host (vsc_fold_text) and
 * the definition restated on strings agree to the bit.
 *
 * vsc_fold_text gives the row of one spacer of n = shape->proto_len letters against a scaffold of m letters on the host, with
 * the very function the kernels call - for users who hold a guide list and no genome.  A spacer letter other than A C G T U
 * gives the undefined row (VSC_OK); a shape outside SHAPE, n != proto_len, a spacer shorter than n, m > 128 or a bad scaffold
 * letter is VSC_ERR_INVALID.
 *
 * vsc_loci_fold: rows[2 i], rows[2 i + 1] = w0, w1 of loci[i] (host arrays, n entries).  One upload, one kernel, one copy back.
 * stats is optional: the candidates by class (they add up to n), the kernel's time and the call's wall time in milliseconds.
 * n == 0: VSC_OK, nothing is launched.  vsc_guides_fold takes the candidates where they lie on the device and requires
 * site_len == 23 (else VSC_ERR_INVALID); the host-only object of vsc_multi_guides_enumerate goes the vsc_loci_fold way.
 * vsc_pattern_guides_fold is the same for vsc_pattern_guides: site_len is the pattern's length, which the CALLER vouches for.
 * VSC_ERR_INVALID, before anything is written: a shape outside SHAPE, a non-zero reserved field, m > 128, a bad scaffold letter,
 * a genome or an object of another context, a NULL shape, NULL rows with n > 0, a NULL scaffold with m > 0.
 *
 * vsc_guides_filter_fold / vsc_pattern_guides_filter_fold: *out = the candidates of `in` that pass FILTER - codes and loci copied
 * unchanged, in the input's order; `in` stays as it is.  Count pass, scan, write pass over tiles of 1 024 candidates: no append
 * atomic, the bytes depend on the input, the shape, the scaffold and the limits only.  A limit in 33 .. 0xFFFFFFFE:
 * VSC_ERR_INVALID.  The result is a normal object of its kind on ctx's device, as the efficiency filter's is.
 *
 * vsc_ctx_timing afterwards: as after the efficiency calls (8 bytes written per candidate).  The scratch is the efficiency
 * calls'; vsc_ctx_release_scratch gives it back.
 *
 * Not offered: minimum-free-energy folding (nearest-neighbour energies, bulges or internal loops inside a stem); a shipped
 * scaffold; the pegRNA extension of each (candidate, edit) pair folded against its spacer, which belongs to the prime-editing
 * pairs; a vsc_multi_* entry (for the reason given above for the efficiency calls).
 */
#define VSC_FOLD_UNDEFINED 0xFFFFFFFFu
#define VSC_FOLD_NO_LIMIT 0xFFFFFFFFu
#define VSC_FOLD_WOBBLE 1u
typedef struct {
    uint32_t site_len, proto_start, proto_len;
    uint32_t stem, gc_min, min_loop;
    uint32_t seed_start, seed_len;
    uint32_t flags;
    uint32_t reserved[3]; /* 0 */
} vsc_fold_shape;
typedef struct {
    uint32_t max_starts, max_self_longest, max_scaf_longest, max_seed_paired;
} vsc_fold_limits;
typedef struct {
    uint64_t defined, invalid, off_contig, not_resident, has_n;
    double kernel_ms, wall_ms;
    uint64_t reserved; /* 0 */
} vsc_fold_stats;
#ifdef __cplusplus
static_assert(sizeof(vsc_fold_stats) == 64 && sizeof(vsc_fold_shape) == 48 && sizeof(vsc_fold_limits) == 16, "vsc_fold_* layout");
#else
_Static_assert(sizeof(vsc_fold_stats) == 64 && sizeof(vsc_fold_shape) == 48 && sizeof(vsc_fold_limits) == 16, "vsc_fold_* layout");
#endif
int vsc_fold_text(const char *spacer /* n letters */, uint32_t n, const char *scaffold /* m letters */, uint32_t m,
                  const vsc_fold_shape *shape, uint32_t *row /* 2 */);
int vsc_loci_fold(vsc_ctx *ctx, const vsc_genome *genome, const vsc_locus *loci /* host */, uint64_t n, const vsc_fold_shape *shape,
                  const char *scaffold, uint32_t m, uint32_t *rows /* host, 2 n */, vsc_fold_stats *stats /* optional */);
int vsc_guides_fold(vsc_ctx *ctx, const vsc_genome *genome, vsc_guides *guides, const vsc_fold_shape *shape, const char *scaffold,
                    uint32_t m, uint32_t *rows /* host, two per candidate */, vsc_fold_stats *stats /* optional */);
int vsc_pattern_guides_fold(vsc_ctx *ctx, const vsc_genome *genome, vsc_pattern_guides *guides, const vsc_fold_shape *shape,
                            const char *scaffold, uint32_t m, uint32_t *rows /* host, two per candidate */,
                            vsc_fold_stats *stats /* optional */);
int vsc_guides_filter_fold(vsc_ctx *ctx, const vsc_genome *genome, vsc_guides *in, const vsc_fold_shape *shape, const char *scaffold,
                           uint32_t m, const vsc_fold_limits *limits, vsc_guides **out);
int vsc_pattern_guides_filter_fold(vsc_ctx *ctx, const vsc_genome *genome, vsc_pattern_guides *in, const vsc_fold_shape *shape,
                                   const char *scaffold, uint32_t m, const vsc_fold_limits *limits, vsc_pattern_guides **out);

/* ---- restriction sites and IUPAC motifs in candidate guides ------------------------------------- */
/*
 * "Can this guide be cloned with this enzyme, and can its edit be seen in a digest?": the recognition sites of restriction
 * enzymes - short IUPAC motifs in general - in the cloned construct of a candidate (the spacer between the vector's flanks)
 * and in its genomic context, at the cut and elsewhere.  A word anywhere in a text, which no model of the other families can
 * express.  This text is normative; everything is integer.  Letters are A C G T = 0 .. 3, and U is read as T.
 *
 * SHAPE     site_len 16 .. 32;  up, down 0 .. 16 with C = up + site_len + down <= 64 (the genomic context, as the efficiency
 *           shape's);  proto_start, proto_len 12 .. 32 with proto_start + proto_len <= site_len (the spacer, n = proto_len, as the
 *           fold shape's);  cut_start, cut_len 1 .. 16 in SITE positions with cut_start + cut_len <= site_len: the CUT ZONE, the
 *           site positions an indel at the cut is expected to change (SpCas9 23-mer: 16, 2 - the two bases beside the bond 3 bp
 *           from the PAM; Cas12a 27-mer TTTV + 23: 21, 6 - the staggered cuts);  every reserved field 0.
 * FLANKS    left a letters, right b letters, a, b 0 .. 16, A C G T U in any case, anything else refused: the vector's text on
 *           either side of the cloned spacer, 5' to 3' in the spacer's orientation.  The launch's, not the candidate's.  The
 *           library ships none.
 * MOTIFS    M 1 .. 63 motifs; motif m = IUPAC text of len 2 .. 16 (A C G T U R Y S W K M B D H V N, any case; not every letter
 *           N) and flags bit 0 BOTH_STRANDS; every other bit 0.  PATTERNS(m) = { text } and, under BOTH_STRANDS, its reverse
 *           complement (IUPAC complement letter by letter, reversed); a palindrome has one pattern.  The library ships none.
 * GENOMIC   x[0, C) = the context of locus (c, p, strand) in read orientation - the efficiency CONTEXT under (up, site_len,
 *           down); CLASS as EffClass, in its order (off_contig can occur when up or down > 0).
 * CONSTRUCT y[0, a + n + b) = left + x[up + proto_start, up + proto_start + n) + right.
 * OCC(t, P) the starts q with q + |P| <= |t| and t[q + k] in the letter set of P[k] for every k.  |P| > |t|: none.
 * Z         [z0, z1) = [up + cut_start, up + cut_start + cut_len) in context positions.
 * construct bit m  iff  OCC(y, P) is not empty for some P in PATTERNS(m)
 * cut       bit m  iff  some q in OCC(x, P), P in PATTERNS(m), has q < z1 and q + |P| > z0   (the occurrence overlaps Z)
 * elsewhere bit m  iff  some q in OCC(x, P), P in PATTERNS(m), has q >= z1 or q + |P| <= z0
 * ROW       three uint64 per candidate: construct, cut, elsewhere; bits M .. 63 are 0.  All three 0xFFFFFFFFFFFFFFFF
 *           (VSC_MOTIF_UNDEFINED) unless the class is defined - M <= 63 keeps that apart from every defined row.
 * TOTALS    optional, 3 M uint64: totals[3 m], [3 m + 1], [3 m + 2] = the number of defined candidates with motif m's construct,
 *           cut and cut-only (cut & ~elsewhere) bit.
 * FILTER    limits forbid_construct, forbid_context, require_cut (uint64 masks; a bit >= M set: refused), flags bit 0 CUT_ONLY:
 *           keep iff defined and construct & forbid_construct == 0 and (cut | elsewhere) & forbid_context == 0 and
 *           (require_cut == 0 or X & require_cut != 0), X = cut, under CUT_ONLY cut & ~elsewhere.  Survivors keep their order.
 *
 * Device, host (vsc_motif_text) and the definition restated on strings agree to the bit.
 *
 * vsc_motif_text gives the row of one context text of c_len = C letters on the host, with the very function the kernels call -
 * for users who hold a guide list and no genome (up = down = 0 and the site as the text).  A context letter other than
 * A C G T U gives the undefined row (VSC_OK); a shape outside SHAPE, c_len != C, a text shorter than c_len, bad flanks or
 * motifs are VSC_ERR_INVALID.
 *
 * vsc_loci_motifs: rows[3 i], [3 i + 1], [3 i + 2] = construct, cut, elsewhere of loci[i] (host arrays, n entries).  One upload,
 * one kernel, one copy back.  totals is optional (host, 3 M entries, written whole).  stats is optional: the candidates by
 * class (they add up to n), the candidates with any construct, any cut and any cut-only bit, the kernel's time and the call's
 * wall time in milliseconds.  n == 0: VSC_OK, nothing is launched (totals and stats are zeroed).  vsc_guides_motifs takes the
 * candidates where they lie on the device and requires site_len == 23 (else VSC_ERR_INVALID); the host-only object of
 * vsc_multi_guides_enumerate goes the vsc_loci_motifs way.  vsc_pattern_guides_motifs is the same for vsc_pattern_guides:
 * site_len is the pattern's length, which the CALLER vouches for.
 * VSC_ERR_INVALID, before anything is written: a shape outside SHAPE, a non-zero reserved field, a flank longer than 16 or with
 * a bad letter, M outside 1 .. 63, a motif's len outside 2 .. 16, a bad motif letter, an all-N motif, an unknown flag, a genome
 * or an object of another context, a NULL where a count says there is something (shape, motifs, rows with n > 0, a flank with
 * a letter count > 0).
 *
 * vsc_guides_filter_motifs / vsc_pattern_guides_filter_motifs: *out = the candidates of `in` that pass FILTER - codes and loci
 * copied unchanged, in the input's order; `in` stays as it is.  Count pass, scan, write pass over tiles of 1 024 candidates: no
 * append atomic, the bytes depend on the input, the shape, the flanks, the motifs and the limits only.  A limits bit at or
 * above M, an unknown limits flag or a non-zero reserved field: VSC_ERR_INVALID.
 *
 * vsc_ctx_timing afterwards: as after the efficiency calls (24 bytes written per candidate).  The scratch is the efficiency
 * calls'; vsc_ctx_release_scratch gives it back.
 *
 * Not offered: a shipped enzyme list or vector; motifs beyond 16 letters or more than 63 per call (call twice); uniqueness of a
 * site over an amplicon wider than the 64-base context; sites made or destroyed by an HDR or prime edit, which belong to those
 * pairs; a vsc_multi_* entry (for the reason given above for the efficiency calls).
 */
#define VSC_MOTIF_UNDEFINED 0xFFFFFFFFFFFFFFFFull
#define VSC_MOTIF_BOTH_STRANDS 1u
#define VSC_MOTIF_CUT_ONLY 1u
typedef struct {
    char text[16]; /* len letters; the rest is not read */
    uint32_t len;
    uint32_t flags;
} vsc_motif;
typedef struct {
    uint32_t up, site_len, down;
    uint32_t proto_start, proto_len;
    uint32_t cut_start, cut_len;
    uint32_t reserved[5]; /* 0 */
} vsc_motif_shape;
typedef struct {
    uint64_t forbid_construct, forbid_context, require_cut;
    uint32_t flags;
    uint32_t reserved; /* 0 */
} vsc_motif_limits;
typedef struct {
    uint64_t defined, invalid, off_contig, not_resident, has_n;
    uint64_t any_construct, any_cut, any_cut_only;
    double kernel_ms, wall_ms;
    uint64_t reserved[2]; /* 0 */
} vsc_motif_stats;
#ifdef __cplusplus
static_assert(sizeof(vsc_motif) == 24 && sizeof(vsc_motif_shape) == 48 && sizeof(vsc_motif_limits) == 32 && sizeof(vsc_motif_stats) == 96,
              "vsc_motif_* layout");
#else
_Static_assert(sizeof(vsc_motif) == 24 && sizeof(vsc_motif_shape) == 48 && sizeof(vsc_motif_limits) == 32 && sizeof(vsc_motif_stats) == 96,
               "vsc_motif_* layout");
#endif
int vsc_motif_text(const char *context /* c_len letters */, uint32_t c_len, const char *left /* a letters */, uint32_t a,
                   const char *right /* b letters */, uint32_t b, const vsc_motif *motifs, uint32_t n_motifs, const vsc_motif_shape *shape,
                   uint64_t *row /* 3 */);
int vsc_loci_motifs(vsc_ctx *ctx, const vsc_genome *genome, const vsc_locus *loci /* host */, uint64_t n, const vsc_motif_shape *shape,
                    const char *left, uint32_t a, const char *right, uint32_t b, const vsc_motif *motifs, uint32_t n_motifs,
                    uint64_t *rows /* host, 3 n */, uint64_t *totals /* optional: host, 3 n_motifs */, vsc_motif_stats *stats /* optional */);
int vsc_guides_motifs(vsc_ctx *ctx, const vsc_genome *genome, vsc_guides *guides, const vsc_motif_shape *shape, const char *left, uint32_t a,
                      const char *right, uint32_t b, const vsc_motif *motifs, uint32_t n_motifs, uint64_t *rows /* host, three per candidate */,
                      uint64_t *totals /* optional */, vsc_motif_stats *stats /* optional */);
int vsc_pattern_guides_motifs(vsc_ctx *ctx, const vsc_genome *genome, vsc_pattern_guides *guides, const vsc_motif_shape *shape, const char *left,
                              uint32_t a, const char *right, uint32_t b, const vsc_motif *motifs, uint32_t n_motifs,
                              uint64_t *rows /* host, three per candidate */, uint64_t *totals /* optional */,
                              vsc_motif_stats *stats /* optional */);
int vsc_guides_filter_motifs(vsc_ctx *ctx, const vsc_genome *genome, vsc_guides *in, const vsc_motif_shape *shape, const char *left, uint32_t a,
                             const char *right, uint32_t b, const vsc_motif *motifs, uint32_t n_motifs, const vsc_motif_limits *limits,
                             vsc_guides **out);
int vsc_pattern_guides_filter_motifs(vsc_ctx *ctx, const vsc_genome *genome, vsc_pattern_guides *in, const vsc_motif_shape *shape,
                                     const char *left, uint32_t a, const char *right, uint32_t b, const vsc_motif *motifs, uint32_t n_motifs,
                                     const vsc_motif_limits *limits, vsc_pattern_guides **out);

/* ---- several devices, streamed + scored on the owning shard ------------------------------------------------ */
/*
 * The streamed search of vsc_search_stream over the device set (BASELINE configuration 5: "100 000 guides streamed ... +
 * per-hit classification feature scoring, 8 x MI355X"): the reads go through all shards batch by batch; what `score` asks
 * for is computed per hit ON THE SHARD THAT FOUND IT, before the exchange; a batch's records (+ votes) travel to the first
 * device and are merged there WHILE the shards search the next batch (two exchange buffers per shard, a merge context of its
 * own on the first device); on_batch receives every merged batch - same records, same order, same read indices as one
 * device's vsc_search_stream gives - and the batch is freed when it returns.
 *   VSC_MULTI_SCORE_NONE   nothing
 *   VSC_MULTI_SCORE_ROWS   the 64-byte packed feature rows of vsc_score_hits_packed, computed and dropped on the shard (what
 *                          a consumer on the shard would read; a timing run like the one-device c5 bench)
 *   VSC_MULTI_SCORE_VOTES  vsc_score_classify_hits: the forest's votes, 2 bytes per hit, travel with the 8-byte record and
 *                          arrive merged: votes_dev[i] belongs to record i of the batch (device memory of the first device)
 * Replaces read_mapping/bidir_mapping.cpp:285-295,307-308 (the loop over reads and the concatenation of the per-thread
 * buffers) + variant_processing/merge_output_bam.h:696-708 + classification/classificationPipeline.R:21-49 for a read set
 * whose result fits no device.
 */
#define VSC_MULTI_SCORE_NONE 0
#define VSC_MULTI_SCORE_ROWS 1
#define VSC_MULTI_SCORE_VOTES 2
typedef struct {
    uint32_t mode;                 /* VSC_MULTI_SCORE_* */
    uint32_t reserved;
    const double *guide_activity;  /* VOTES: on-target activity per read (n_guides values) */
    const vsc_rf_model *model;     /* VOTES: the forest */
} vsc_multi_score;
typedef int (*vsc_multi_batch_fn)(void *user, vsc_hits *batch, uint32_t first_guide, uint32_t n_guides, const uint16_t *votes_dev);
int vsc_multi_search_stream(vsc_multi *m, const vsc_multi_genome *g, const uint64_t *guides, uint32_t n_guides,
                            const vsc_search_params *params, uint32_t batch_reads, const vsc_multi_score *score,
                            vsc_multi_batch_fn on_batch, void *user);

/* ---- host-side formatting helpers (no device needed) ------------------------------------------ */
/*
 * Order in which read_mapping/bidir_mapping.cpp:167-187 writes the records of one search result
 * and which of them it flags BAM_FLAG_SECONDARY.  hits must be sorted as vsc_search returns them.
 * order[i] = index into hits of the i-th record written; secondary[i] = 1 if that record carries
 * flag 256.
 */
void vsc_sam_order(const vsc_hit *hits, uint64_t n, uint64_t *order, uint8_t *secondary);
#ifdef __cplusplus
}
#endif
#endif
