// vsc_internal.h - types shared by the host code (vsc_api.cpp, vsc_multi.cpp) and the HIP kernels in vsc_seed.hip, vsc_sort.hip, vsc_enum.hip and the first kernel file
// (vsc_kernels.hip).  Not installed; the public contract is include/varscot_hip.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "varscot_hip.h"
#include "vsc_efficiency.h"
#include "vsc_eff_trees.h"
#include "vsc_mh.h"
#include "vsc_fold.h"
#include "vsc_motif.h"
#include "vsc_edit.h"
#include "vsc_variation.h"
#include "vsc_prime.h"
#include "vsc_hdr.h"
#include "vsc_effects.h"
#include "vsc_knockout.h"

namespace vsc {

// ---- scan geometry ---------------------------------------------------------------------------
constexpr int kWave = 64;                       // gfx950 wavefront
constexpr int kWavesPerGroup = 4;               // 256-thread workgroups; the 4 waves never synchronise
constexpr int kSitesPerLane = 8;                // candidate sites a lane keeps in VGPRs in the guide loop
constexpr int kBatch = kWave * kSitesPerLane;   // 512 sites per wave per guide-loop pass
constexpr int kQueueCap = kBatch + kWave;       // per-wave LDS site queue (a step adds at most 64)
constexpr int kHitCap = 128;                    // per-wave LDS hit staging buffer (flushed above 64)
constexpr int kTileWords = kWave;               // one 32-base word of each plane per lane = 2048 positions
constexpr int kTileBases = kTileWords * 32;
constexpr int kChunkTiles = 8;                  // tiles a wave takes per grab of the work counter
constexpr int kGuideUnroll = 4;                 // guides per inner iteration (guide table is padded to it)
constexpr uint32_t kMask23 = 0x7FFFFFu;
constexpr int kSiteStrandBit = 23;              // site word x: bit 23 = '-' strand
constexpr int kSiteEdgeBit = 24;                // site word x: bit 24 = the position after the window is N
constexpr uint32_t kPadWords = 4;               // words the device planes are padded with past the shard

// ---- seed-partitioned search (vsc_seed.hip) -------------------------------------------------------
constexpr int kSegments = 3;                    // read positions [0,7) [7,14) [14,21); the PAM is in no segment
constexpr int kSegBases = 7;
constexpr int kBucketsPerSeg = 1 << (2 * kSegBases);  // 16384 seven-mers
constexpr int kBuckets = kSegments * kBucketsPerSeg;
constexpr int kSeedHitCap = 256;                // smallest block of records a wave reserves per atomic
constexpr int kSlicedSites = 32;                // sites per lane of the bit-sliced comparison (one bit each)
constexpr int kSlicedChunk = kWave * kSlicedSites;  // 2048 sites per wave and chunk
constexpr int kRestBases = VSC_READ_LEN - kSegBases;  // 16 read positions outside the seed segment (what a site record keeps)
constexpr int kCmpBases = 2 * kSegBases;        // ... of which the comparison counts 14: the other two segments.  Read positions
                                                // 21 and 22 are the PAM, and a chunk holds sites of ONE PAM (its class)
constexpr int kVertWords = 2 * kCmpBases;       // words of a bit-sliced block of 32 sites: hi and lo plane bit of the 14 positions
constexpr int kSeedClasses = 3;                 // PAMs an index can hold: GG, GA (+ -P); class of a site = which one its window ends in
// read lists: one per bucket for segments 0 and 1 (shared by the classes - an entry holds a budget per class), one per
// (class, bucket) for segment 2, whose neighbourhood depends on what the class leaves of the mismatch limit (seed_enum_kernel)
constexpr int kLists = (kSegments - 1 + kSeedClasses) * kBucketsPerSeg;
constexpr int kListBudgetShift = 16;            // list entry y: read index | per class c: mismatches left for the 14 compared positions
constexpr uint32_t kListNoBudget = 15;          //   << (16 + 4 c), 15 = the read has no business with that class (list padding: all ones)
constexpr int kTokLaneShift = 26;               // sliced hit token, high word: read of the pass (14 bits) | chunk slot << 14 | lane << 26
constexpr int kTokSlotShift = 14;
constexpr uint32_t kTokReadMask = (1u << kTokSlotShift) - 1u;
constexpr int kSlicedResolve = 3;                // sliced kernel: resolve when this many passes of 64 tokens wait (the
                                                // gathers of the later passes overlap the earlier ones)
constexpr int kSlicedTokCap = 512;  // per-wave LDS ring of 8-byte hit tokens (a power of two: the slot is an AND): a group of four reads adds <= 256
// chunk table word z: bucket (16 bits) | rank in the chunk of its first '-' site (0 .. 2048) << 16 | "holds a window
// that is followed by N" << 28 | class of its sites << 29
constexpr uint32_t kChunkBucketMask = 0xFFFFu;
constexpr int kChunkMinusShift = 16;
constexpr int kChunkEdgeBit = 28;
constexpr int kChunkClassShift = 29;
constexpr uint32_t kIndexLayout = 2;            // seed index layout (index files of another layout are refused)
constexpr int kSlicedWavesPerSimd = 6;          // resident waves of the sliced kernel per SIMD (registers and LDS allow five)
constexpr int kSlicedGrab = 8;                  // chunks of 2048 sites per grab of the work counter (sliced kernel)

// counters[] slots of one scan launch
enum { kCntHits = 0, kCntChunk = 1, kCntSites = 2, kCntOverflow = 3, kCntVisited = 4, kCntPad = 5, kCntLost = 6, kCntGroups = 7, kCntSlots = 8 };
// The sliced kernel hands out chunks through kCursors work cursors, one per slice of the chunk range, 128
// bytes apart behind the counters: one device-wide cursor sustains only ~90 atomics/us
// (MI355X_MICROARCH.md), which for 270 000 grabs is 3 ms - as long as a whole 1 000-read search.
// The sliced kernel writes its hits into up to kParts regions by read range (region = read index >>
// kRegionBits, 64 reads): inside a region a hit is one packed 8-byte record (below), and the regions
// are ordered independently by the bin sort of vsc_sort.hip; their concatenation is the result.
// Per region: counters[kCntPart + 4 p + {0, 1, 2}] = records reserved, sentinels among them, records lost.
constexpr int kRegionBits = 6;
constexpr int kRegionReads = 1 << kRegionBits;
constexpr int kParts = 256;
constexpr int kMaxPassReads = kParts * kRegionReads;  // reads one search pass can take (vsc_search splits larger sets)
constexpr int kCntPart = 8;
constexpr int kCursors = 32;
constexpr int kCursorStride = 16;  // in 8-byte words
constexpr int kCursorBase = kCntPart + 4 * kParts + 8;  // first cursor, in 8-byte words from the start of the counter buffer
constexpr int kCounterWords = kCursorBase + kCursors * kCursorStride;

// ---- packed hit record (what the search kernels hand to the sort) --------------------------------------
//   bits  0..22  mismatch mask in forward-genome window coordinates (NM is its popcount)
//   bits 23..54  position of the window start RELATIVE TO THE SHARD's first position (a shard of the upper half of the
//                genome would otherwise leave the top key bits constant: bins by the top position bits fill unevenly, slots
//                overflow, levels are wasted), shifted left by pos_pad = 32 - (bits the shard's positions need): the zero
//                bits of a small genome sit at the bottom of the field, where the sort's last stage ignores them, instead
//                of in the middle of the key, where partition levels would be spent on them
//   bit  55      strand (1 = '-')
//   bits 56..61  read index inside its region (read & 63)
//   bits 62, 63  0; the all-ones word is the sentinel that pads reserved-but-unused record slots
// Ascending order of the records of one region = the result order (read, strand, position).
constexpr int kRecPosShift = 23;
constexpr int kRecStrandShift = 55;
constexpr int kRecReadShift = 56;
constexpr int kRecKeyBits = 33 + kRegionBits;  // sort key = rec >> kRecPosShift
constexpr uint64_t kRecSentinel = ~0ull;

// ---- bin sort (vsc_sort.hip) -------------------------------------------------------------------------
constexpr int kSortThreads = 512;                      // partition: 512 threads x 16 records = a tile of 8 192 in 64 KB of LDS, two workgroups per CU
                                                      // (one tile of 16 384 per CU: 6.3-6.5 ms per c3 partition against 5.9-6.0)
constexpr int kSortItems = 16;
constexpr int kSortTile = kSortThreads * kSortItems;  // records per partition tile
constexpr int kFinThreads = 512;                      // finalize kernel: 512 threads x 16 records, two workgroups per CU
constexpr int kFinItems = 16;
constexpr int kSortCap = kFinThreads * kFinItems - 128;  // the largest bin it orders in LDS (records + sub-bin table = half
                                                      // of the CU's 160 KiB, so that one workgroup computes while the other
                                                      // waits for memory)
constexpr int kSortMaxBinBits = 11;                   // <= 2048 bins per partition level
constexpr int kSortSubBits = 13;                      // <= 8 192 sub-bins inside the finalize kernel
constexpr int kSortSubBitsRows = 12;                  // ... 4 096 when it also writes the feature rows: the other half of the table's LDS
                                                      // stages the rows on their way out
constexpr int kHistTiles = 8;                         // tiles a block of the histogram kernel walks through

// Required plane bits of the two PAM letters, expanded to all-ones / all-zero words.
struct PamMasks {
    uint32_t ah, al;  // first letter  (window position 21 on '+')
    uint32_t bh, bl;  // second letter (window position 22 on '+')
};

struct ScanArgs {
    const uint32_t *hi, *lo, *nm;  // device planes; element 0 = the shard's first word; padded by kPadWords
    uint32_t first_pos;            // global position of bit 0 of element 0
    uint32_t n_tiles;              // tiles whose window starts are searched
    const uint4 *guides;           // two reads per uint4: (hi0, lo0, hi1, lo1); count padded to kGuideUnroll
    uint32_t n_guides_padded;
    uint32_t max_mm;               // -M
    uint32_t k_half;               // floor(max_mm / 2): the per-half budget of the reference's pigeonhole search
    uint32_t n_pam;
    PamMasks pam[3];               // GG, GA (+ -P)
    const uint32_t *contig_end;    // ascending global end positions (offset + length) of all contigs
    uint32_t n_contigs;
    uint64_t *hit_keys;            // out: guide << 33 | strand << 32 | global position
    uint32_t *hit_vals;            // out: NM << 23 | mismatch mask (window coordinates)
    unsigned long long hit_cap;
    unsigned long long *counters;  // kCntSlots values, zeroed before the launch
    // extract mode only: PAM-valid sites of both strands (x = hi plane | strand | edge, l = lo plane);
    // the append cursor is counters[kCntHits], the capacity hit_cap
    uint32_t *site_x, *site_l, *site_pos;
};

// One segment of the bin sort: a span of packed records that is ordered independently of all others (level 1:
// one output region of the search kernel; deeper levels: one bin that was too large for the finalize kernel).
struct SortSeg {
    uint64_t in_off;     // first record of the segment in the level's source buffer
    uint64_t out_off;    // first record of the segment's span in the level's destination buffer
    uint64_t final_off;  // index of the segment's first vsc_hit in the result
    uint32_t n_in;       // records in the source span (level 1: sentinels / unused block tails included)
    uint32_t guide_base; // read index of the region's first read
    // whose bin cursors and slots a partition appends to: (region << bin_bits) + bin.  The segment's own index, except
    // where a region's records arrive in several segments (a search in parts: one segment per part and region)
    uint32_t region = 0;
    uint32_t pad = 0;
};

struct SortArgs {
    const SortSeg *segs;
    const uint32_t *seg_tile0;     // [n_segs + 1] first tile of every segment (tile = kSortTile records)
    uint32_t n_segs, n_tiles;
    const uint64_t *in;            // packed records
    const uint64_t *pair_keys;     // level 0 only (streaming scan): guide << 33 | strand << 32 | position ...
    const uint32_t *pair_vals;     //                                ... and NM << 23 | mask; `in` is then unused
    uint64_t *out;
    const uint32_t *side_in;       // null, or one 32-bit side word per record of `in` (the site's lo plane) ...
    uint32_t *side_out;            // ... moved to the same places of this array as the records in `out`
    uint32_t *hist;                // [n_segs << bin_bits] records per bin
    uint32_t *cursor;              // [n_segs << bin_bits] next free record of every bin (relative to the segment)
    uint32_t *bin_start;           // [n_segs << bin_bits] first record of every bin (relative to the segment)
    uint32_t bin_bits, bin_shift;  // bin = (record >> bin_shift) & ((1 << bin_bits) - 1)
    uint32_t pos_pad;              // level 0: left shift of the position field
    uint32_t pos_base;             // level 0: first global position of the shard (records hold positions relative to it)
    uint32_t xcd_tiles;            // partition: tiles per XCD (0: workgroup b takes tile b)
    // a search in parts: XCD x takes tiles [xcd_first[x], xcd_first[x + 1]) - the segments of ITS regions, the same regions in
    // every part, so that the pieces of one bin still meet in one L2 (xcd_tiles = the longest of the eight ranges)
    uint32_t xcd_by_region;
    uint32_t xcd_first[9];
    // the block fill table of the search's records (SeedArgs::fill; null: unused slots hold sentinels): record i of `in` is
    // valid iff (i & ((1 << fill_shift) - 1)) < fill[i >> fill_shift]; the slots of a hole are not read
    const uint32_t *fill;
    uint32_t fill_shift;
    // slot mode (no histogram pass): bin i of the level owns records [i * slot_cap, (i + 1) * slot_cap) of `out`; the
    // partition reserves room with `cursor` (zeroed) alone and raises *overflow when a bin does not fit its slot -
    // the caller then repeats the level with the histogram.  0: exact mode (bin_start from the histogram)
    uint32_t slot_cap;
    uint32_t *overflow;
};

struct FinArgs {
    const SortSeg *segs;
    uint32_t n_segs;
    const uint64_t *src;           // the buffer the last partition level wrote (or the search kernel, if none ran)
    const uint32_t *hist;          // bins of the last partition level; null: every segment is one bin (its source span)
    const uint32_t *bin_start;
    uint32_t bin_bits;
    uint32_t sub_shift, sub_bits;  // LDS counting sort on (record >> sub_shift) & ((1 << sub_bits) - 1) ...
    uint32_t low_bits;             // ... then ranking on the key bits below (0: none left)
    uint32_t pos_pad;              // left shift of the records' position field
    uint32_t pos_base;             // first global position of the shard: the records' positions count from it
    SortSeg *over;                 // bins with more than `cap` records are listed here for another level
    uint32_t over_cap;
    uint32_t cap;                  // <= kSortCap (smaller in tests only)
    uint32_t *n_over;
    uint32_t *cursor;              // zeroed: the resident workgroups count the bins they take here
    const uint32_t *contig_off;    // ascending global start positions of all contigs
    uint32_t n_contigs;
    vsc_hit *out;
    uint32_t slot_cap;             // slot mode: bin i's records are src[i * slot_cap ...) (hist = the partition's cursors)
    const uint32_t *overflow;      // slot mode: non-zero = the partition gave up, nothing to do
    // a search that keeps the sites' bases (SeedArgs.hit_side): the side words beside `src`, the reads' planes, and where the
    // 64-byte packed feature row of result record i goes: rows + (i - rows_first) * 64 bytes
    const uint32_t *side_src;
    const uint2 *guides;           // (hi plane, lo plane) of read guide_first + j
    uint32_t guide_first;
    uint4 *rows;                   // null: plain records (low 23 bits = mismatch mask)
    uint64_t rows_first;
};

struct ScoreArgs {
    const vsc_hit *hits;  // device records, already offset to the first row to score
    uint64_t n;
    const uint2 *hl;          // interleaved (hi, lo) plane words of the shard that holds the hits
    uint32_t first_pos;
    uint64_t n_plane_words;
    const uint32_t *contig_off;
    const uint2 *guides;  // (hi plane, lo plane) per read
    double *mit;          // may be null
    uint8_t *mit_flags;   // may be null
    uint8_t *features;    // may be null; n * 442 bytes
    // optional processing order (score_packed_kernel): the rows are visited genome slice by genome slice so that
    // the window gathers of everything in flight fall into one slice of the planes (see launch_score_schedule);
    // virtual position v lies in segment j (seg_prefix[j] <= v < seg_prefix[j + 1]) and is row seg_start[j] + v - seg_prefix[j]
    const uint64_t *seg_prefix;  // [n_segs + 1]; null: rows in index order
    const uint64_t *seg_start;   // [n_segs]
    uint32_t n_segs;
};

// How one search cuts the pigeonhole (seed_enum_kernel).  A site of class c (its PAM) leaves a read left_c = max_mm -
// (mismatches of the read's last two letters with that PAM) for read positions 0..20.  Segment 0 is searched within k0
// substitutions, segment 1 within k1, segment 2 within left_c - k0 - k1 - 2 (not at all if negative): a window that fails all
// three has at least (k0 + 1) + (k1 + 1) + (left_c - k0 - k1 - 1) = left_c + 1 mismatches.  Every (k0, k1) in 0..2 that keeps
// the third threshold <= 2 is a valid cut; the host picks one by cost (vsc_api.cpp).  tight = 0: the round-3 cut -
// floor(max_mm / 3) in all three segments.
struct SeedPlan {
    uint32_t max_mm, k0, k1, tight;
    uint32_t n_nbr;      // neighbours enumerated per (read, segment): 1 / 22 / 211 = the largest threshold in use
    uint32_t n_pam;
    uint32_t pam_codes;  // class c: (first letter << 2 | second letter) << 4 c
};

struct SeedArgs {
    // (a search cut into several launches hands each launch its part of the table: chunk_tab + first chunk, n_chunks = the part's
    // chunks - an entry names its sites and blocks by absolute index.  The launches share the region cursors; every launch
    // opens fresh blocks and closes them)
    const uint4 *chunk_tab;        // [n_chunks] {first site, site count, bucket | first '-' rank << 16 | edge << 28 | class << 29, first vertical block}
    const uint32_t *vert;          // bit-sliced copies of the sites: kVertWords words per block of 32 sites (see seed_transpose_kernel)
    const uint2 *list_rest;        // per list entry {rest(hi) | rest(lo) << 16, read | budget per class << 16 ..}
    const uint2 *sites;            // {rest(hi) | rest(lo) << 16, position} per site
    const uint32_t *edge_bits;     // 1 bit per site: its window is followed by N
    const uint2 *guides;           // (hi plane, lo plane) per read
    uint32_t n_chunks;
    const uint32_t *poff;          // [kLists + 1] first entry of every read list (multiples of kGuideUnroll)
    uint32_t max_mm, k_half;
    uint32_t k_seg0, k_seg1;       // substitutions searched in segments 0 and 1 (SeedPlan.k0, .k1): what the duplicate rule tests
    const uint32_t *contig_end;
    uint32_t n_contigs;
    uint64_t *hit_recs;            // out: packed records (layout above), region p = [p * part_cap, (p + 1) * part_cap)
    uint32_t *hit_side;            // null, or (per-hit feature rows wanted): one word beside every record = the site's lo plane in read
                                   // orientation; its hi plane then sits in the record's low 23 bits in place of the mismatch mask
    uint32_t group_out;            // 1: the four waves of a workgroup share their open blocks (chunk-sharing kernel only)
    uint32_t reserve;              // records a wave reserves per atomic on its region's cursor: a power of two, 64 .. 1024
    uint32_t reserve_log2;
    uint32_t pos_pad;              // left shift of the position field of a record
    uint32_t pos_base;             // first global position of the shard: a record holds position - pos_base
    uint32_t n_parts;              // regions in use (region of a hit = read index >> kRegionBits)
    unsigned long long part_cap;   // records per region
    unsigned long long *counters;  // kCntPart + 4 p + {0,1,2}, kCntSites (= pairs compared), kCntVisited, kCntOverflow, cursors
    // Block fill table (null: the unused tail of every open block is written as sentinels and counted in kCntPart + 4 p + 1):
    // one word per block of `reserve` records of hit_recs - part_cap is a multiple of reserve, so block b of region p is word
    // (p * part_cap >> reserve_log2) + b -, set to all ones ("full") before the launch; a wave that leaves a block open at the
    // end of the kernel stores the records it holds.  Slots past that count are never written, and never read by the sort.
    uint32_t *fill;
};

// ---- the record sinks' input ---------------------------------------------------------------------------------------------
// Every consumer of a pass's records - summary_kernel, votes_summary_kernel, select_score_kernel / select_compact_kernel and
// rf_predict_kernel's classify in place - reads them where the search kernel left them: the packed records of every region
// that holds any (SEED; sentinels among them) or the one span of (key, value) pairs (SCAN).  The spans are cut into tiles of
// kSumTile record slots; slot k of tile i is word i * kSumTile + k of every array that lies beside the records (scores, votes).
// A workgroup walks a range of consecutive tiles; a SEED workgroup's tiles lie in one region at a time - 64 reads (helpers: vsc_sink.h).
constexpr int kSumThreads = 256;
constexpr int kSumItems = 8;      // consecutive records a lane takes (one running accumulator per lane)
constexpr int kSumTile = kSumThreads * kSumItems;
constexpr int kSumTilesPerBlock = 8;

struct SumSeg {
    uint64_t in_off;      // first record of the region (SEED) / of the pairs (SCAN)
    uint32_t n;           // records in the span (SEED: sentinels included)
    uint32_t first_read;  // pass-local index of the region's first read (SCAN: 0, the key holds the pass-local read)
};

struct SinkInput {
    const uint64_t *recs;       // SEED: packed records; SCAN: keys (read << 33 | strand << 32 | global position)
    const uint32_t *vals;       // SCAN: NM << 23 | mask; SEED: null
    const SumSeg *segs;
    const uint32_t *seg_tile0;  // [n_segs + 1]: first tile (kSumTile records) of every segment
    uint32_t n_segs, n_tiles;
    uint32_t pos_pad, pos_base; // SEED: the pass's position encoding (vsc_sort.hip pack_pair)
    const uint64_t *excl;       // per pass-local read: strand << 32 | global position of the excluded locus, ~0: none (null: none)
};

// ---- random-forest inference ---------------------------------------------------------------------------------
// Every split of the forest is a TEST `x <= thr` on a small non-negative integer: the predictors of the feature
// matrix are flags and counts (`x <= split` is `x <= floor(split)`), and the on-target activity (a double, constant
// per read) enters as its rank among the forest's distinct activity thresholds (rank = thresholds strictly below it),
// which turns `activity <= T_j` into `rank <= j` exactly.  The forest has few DISTINCT tests (rfClassifier: 217 for
// 105 235 split nodes), so a row is reduced to one bit per test first (7 words), and a node is 4 bytes:
//   bits 0..9 test | 10..19 left daughter | 20..29 right daughter (0-based; a terminal node points at itself) |
//   30 terminal | 31 votes class "1"
// A node visit is one 4-byte LDS read of the node + one of the row's test word.
// Trees of at most 512 nodes (rfClassifier: 275) use the COMPACT form, in which a node says of each daughter how many
// nodes further on the walk continues - at the daughter (which lies behind its parent), or, if the daughter is terminal,
// at the root of the NEXT tree (trees lie back to back) with the terminal node's vote in the field: terminal nodes are never
// visited, a lane moves on to its next tree the moment it reaches one, and a step is one add:
//   bits 0..9 test | 10..19 right: nodes to skip, 20 its vote | 21..30 left: nodes to skip, 31 vote
// (the all-zero word is the SINK behind the last tree of a chain: it skips nothing and votes nothing)
constexpr int kRfRows = 512;             // feature rows per workgroup (one thread each)
constexpr int kRfMaxTests = 1024;        // distinct (predictor, threshold) pairs a forest may use
constexpr int kRfMaxNodes = 1024;        // nodes of one tree (rfClassifier: 275)
constexpr int kRfTileBytes = 26624;      // whole trees staged in LDS per step (with 14 KB of test bits: 4 workgroups = 32 waves per CU)
constexpr int kRfPairFirstBit = 3;       // pair form: test bits lie at positions 3 .. 31 of their words (29 per word) ...
constexpr int kRfPairMaxTests = 8 * (32 - kRfPairFirstBit);  // ... of which a row has eight: 232 tests
constexpr int kRfPairBitsBytes = 16384;  // pair form: the test bits as two planes of 256 rows x 8 words
constexpr int kRfPairTileBytes = 24512;  // ... and its tree tile (16 + 24 KB: four workgroups per CU)
constexpr int kRfChains = 2;             // trees a thread walks at the same time (compact form)
constexpr int kRfRowWords = 20;          // a row as the test extraction sees it: 16 packed words, 3 words of dinucleotide
                                         // counts (5 bits each, 6 / 6 / 4), 1 word activity rank
// a test: field `width` bits at `shift` of row word `word` <= thr; dense rows read column `dense_col` instead
struct RfTest {
    uint8_t word, shift, width, thr;
    uint16_t dense_col;  // 0..441, or 442 = the activity rank
    uint16_t pad;
};

struct RfArgs {
    const uint32_t *nodes;      // [n_trees * n_nodes], tree-major
    const uint8_t *depth;       // [n_trees] steps from the root to the deepest terminal node
    uint32_t n_trees, n_nodes;
    uint32_t compact;           // 2: pair nodes (8 bytes, two levels each), 1: compact nodes (<= 512 per tree), both walked through
                                // per-lane tree queues; 0: the form above
    const RfTest *tests;        // [n_tests], sorted by the row word they read
    const uint32_t *test_begin; // [kRfRowWords + 1] first test of every row word
    uint32_t n_tests;
    // the rows: dense (n x 442 bytes), packed (n x 64 bytes), or - both null - computed in the kernel from `score`'s
    // hits (the fused score -> classify path: the feature rows never exist in memory)
    const uint8_t *dense;
    const uint4 *packed;
    const uint8_t *act_rank;    // activity rank per row (dense / packed) or per read (fused)
    uint64_t n;
    uint32_t *votes;            // [n] trees voting class "1" (zeroed before the launch when tree_splits > 1) ...
    uint16_t *votes16;          // ... or 16-bit (fused path; tree_splits == 1)
    uint32_t tree_splits;       // gridDim.y: every workgroup row walks n_trees / tree_splits trees
    ScoreArgs score;            // fused path: hits, planes, reads (+ optional MIT output)
    // classify in place (modes 3, 4): the rows are the search kernel's records where they lie (`in.recs` non-null: the sinks'
    // input, SinkInput above), 512 row slots per workgroup = a quarter of a tile of kSumTile; the votes go into one word per
    // record slot of every tile (SelectArgs::score's layout; kSelDropped: sentinel, read beyond the pass, excluded locus), added
    // with atomics into a zeroed array when tree_splits > 1.  score.hl / first_pos: the planes; score.guides and act_rank:
    // per pass-local read
    SinkInput in;
    uint32_t n_reads;
    uint32_t *slot_votes;
};

// ---- per-guide summary (vsc_search_summary; summary_kernel in vsc_kernels.hip) ----------------------------------------------
// The kernel adds the records of its SinkInput into one row of kSumWords 64-bit words per read of the pass, the layout of
// vsc_guide_summary: mit_sum, nm[0..8], mit_ub, on_target (low half of the last word).
constexpr int kSumWords = 12;
constexpr int kSumCounts = 11;    // LDS counters per read of the region: nm[0..8], mit_ub, on_target
constexpr int kSumCountBits = 7;  // nm counters of a lane packed into one 64-bit word (9 x 7 bits; a lane adds <= kSumItems)

struct SummaryArgs : SinkInput {
    unsigned long long *out;    // kSumWords per pass-local read, zeroed once per call
};

// Votes summary (vsc_search_summary_classified; votes_summary_kernel): the same input + the votes word of every record slot
// (RfArgs::slot_votes), added into rows of kSumWords words per pass-local read, the layout of vsc_guide_votes: votes_sum, active,
// ties, active_nm[0..8].
struct VotesSummaryArgs : SummaryArgs {
    const uint32_t *votes;
    uint32_t n_trees, n_reads;
};

// ---- table-driven score (vsc_score_hits_table, vsc_search_*_table; vsc_table.hip, vsc_table.h) ---------------------------------
// table_score_kernel scores sorted hits (`hits` non-null: one double and / or one fixed-point word per hit) or the search
// kernel's records where they lie (`in.recs` non-null: one fixed-point word per record slot of every tile - SelectArgs::score's
// layout; kSelDropped: sentinel, slot beyond its segment, read beyond the pass, excluded locus).
struct TableArgs {
    const double *weights;      // kTableWeights doubles: pair[20][4][4], pam[16]
    const uint2 *hl;            // interleaved (hi, lo) plane words of the shard
    uint32_t first_pos;
    uint64_t n_plane_words;
    const uint32_t *contig_off; // sorted hits only
    const uint2 *guides;        // (hi plane, lo plane) per read (records: per pass-local read)
    const vsc_hit *hits;
    uint64_t n;
    double *scores;             // may be null
    uint32_t *fixed;            // may be null
    SinkInput in;
    uint32_t n_reads;           // reads of the pass (sorted hits: of the call)
    uint32_t *slot_fixed;
};

// Table summary (vsc_search_summary_table; table_summary_kernel): the sinks' input + the fixed-point word of every record slot,
// added into rows of kSumWords words per pass-local read, the layout of vsc_guide_table_row: score_sum, positive,
// positive_nm[0..8], reserved.
struct TableSummaryArgs : SummaryArgs {
    const uint32_t *fixed;
    uint32_t n_reads;
};

// ---- per-guide selection (vsc_search_select; select_*_kernel in vsc_kernels.hip) -------------------------------------------
// An exact per-read radix select on the composite key  score (31 bits) << 33 | ~(strand << 32 | global position) (33 bits):
// the larger key is the better hit (score descending, '+' before '-', position ascending), and keys are unique per read.
// Round 1 runs over the records where the search kernel left them (SinkInput): every record's
// score goes into a word beside it and into its read's histogram over kSelBins monotone coarse bins of the score.  From the
// histogram every read gets its threshold bin (the bin the K-th best lies in); round 2 copies the records of the bins >=
// the threshold - the candidates - into per-read lists; the later rounds (select_resolve_kernel) run over a read's list only.
constexpr int kSelBins = 128;            // score bin: 0 for score 0, else 1 + 4 * (31 - clz) + the next 2 bits (<= 124)
constexpr int kSelThreads = 256;
constexpr int kSelMaxTilesPerBlock = 128;  // tiles of kSumTile records a workgroup of round 1 / 2 walks through: as many as leave
constexpr int kSelMinTilesPerBlock = 8;    // every CU a few workgroups (one LDS table flush of 8 192 cells per region a workgroup meets)
constexpr uint32_t kSelDropped = ~0u;    // score word of a record that is no candidate (sentinel, excluded locus, below the floor)
constexpr int kSelKeyPosBits = 33;

struct SelectArgs : SinkInput {
    uint32_t min_score;         // records below it are dropped
    uint32_t vote_trees;        // 0: the score is rint(MIT * 2^24), computed in round 1; else the forest's tree count: `score` holds
                                // the records' votes on entry (classify in place), min_score is a floor on them, linear bins
    uint32_t table_key;         // non-zero (vsc_search_select_table): `score` holds the records' fixed-point table scores on entry
                                // (table_score_kernel), min_score is a floor on them, the logarithmic bins
    uint32_t top_k;             // 0: no limit
    uint32_t n_reads;           // reads of the pass
    uint32_t tiles_per_block;   // kSelMinTilesPerBlock .. kSelMaxTilesPerBlock
    uint32_t *score;            // one word per record of every tile (record k of tile i: i * kSumTile + k): round 1 writes, round 2 reads
    uint32_t *hist;             // [n_reads * kSelBins], zeroed: records per (read, score bin)
    uint32_t *thr;              // [n_reads] threshold bin
    uint32_t *thr_region;       // [regions of kRegionReads reads], all ones before: the smallest threshold bin of the region's reads
    uint32_t *count;            // [n_reads] candidates = records in the bins >= thr
    uint32_t *cursor;           // [n_reads], zeroed: next free entry of the read's candidate list
    const uint64_t *cand_off;   // [n_reads] first entry of the read's list in cand_key / cand_mask
    const uint64_t *surv_off;   // [n_reads] first record of the read's survivors in `out`
    uint64_t *cand_key;         // composite keys
    uint32_t *cand_mask;        // mismatch masks beside them
    uint64_t *out;              // survivors as packed records (layout above), reads in order, unsorted inside a read
};

// ---- regions (vsc_regions; vsc_regions.cpp builds them, the two sinks above test their records against them) ---------------
// The intervals in global coordinates, sorted by start: start[] and end_max[] = the running maximum of their ends (no
// interval reaches across a contig boundary, so the maximum over earlier contigs stays below every later position), and
// two bits per block of 2^block_shift window starts: kRegOut - no start of the block is in the regions, kRegIn - every one
// is, kRegMixed - one binary search over start[] answers either rule (18 dependent loads for 250 000 intervals).
// The same arrays on the host (vsc_regions) and on the device (the context's copy).
constexpr uint32_t kRegOut = 0, kRegIn = 1, kRegMixed = 2;
constexpr uint32_t kRegMinBlockShift = 5;    // blocks of at least 32 starts ...
constexpr uint32_t kRegMaxBlocks = 1u << 23; // ... and as small as keeps the table within 2 MB (2 bits per block): 512 at 3 Gbp

struct RegionsView {
    const uint32_t *start;    // [n] ascending
    const uint32_t *end_max;  // [n]
    const uint32_t *cls;      // 16 blocks per word, block b in bits 2 (b & 15) .. of word b >> 4
    uint32_t n;
    uint32_t n_blocks;        // blocks the table covers (the genome's positions); a start beyond them is out
    uint32_t block_shift;
    uint32_t rule;            // VSC_REGION_OVERLAP / VSC_REGION_INSIDE
};

// The interval search, for the window of `len` bases that starts at global position pos (len < VSC_READ_LEN: a window cut off
// by its contig's end - the host's vsc_regions_contains only; it overlaps with what is left of it and lies inside nothing).
//   OVERLAP  n = #{start < pos + len}: in iff n > 0 and end_max[n - 1] > pos
//   INSIDE   n = #{start <= pos}:      in iff n > 0 and end_max[n - 1] >= pos + VSC_READ_LEN
__host__ __device__ inline bool regions_search(const RegionsView &v, uint32_t pos, uint32_t len)
{
    const bool inside = v.rule == VSC_REGION_INSIDE;
    const uint32_t bound = inside ? pos + 1u : pos + len;
    uint32_t lo = 0, hi = v.n;  // -> #{start < bound}
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (v.start[mid] < bound) lo = mid + 1; else hi = mid;
    }
    if (lo == 0) return false;
    const uint32_t e = v.end_max[lo - 1];
    return inside ? e >= pos + (uint32_t)VSC_READ_LEN : e > pos;
}

// Is the window that starts at global position pos in the regions?  One read of the class table, the search for mixed blocks.
__host__ __device__ inline bool regions_contains(const RegionsView &v, uint32_t pos, uint32_t len = VSC_READ_LEN)
{
    if (len != (uint32_t)VSC_READ_LEN) return len != 0 && regions_search(v, pos, len);  // (the table describes whole windows)
    const uint32_t b = pos >> v.block_shift;
    if (b >= v.n_blocks) return false;
    const uint32_t c = (v.cls[b >> 4] >> (2u * (b & 15u))) & 3u;
    return c == kRegMixed ? regions_search(v, pos, len) : c == kRegIn;
}

// the sinks' arguments with regions: the plain kernels keep the plain structs (and compile to what they were)
struct SummaryRegionArgs : SummaryArgs {
    RegionsView reg;
    unsigned long long *out_in;  // the rows over the hits in the regions, laid out and zeroed as `out`
};

struct SelectRegionArgs : SelectArgs {
    RegionsView reg;
    uint32_t drop;               // 0: records outside the regions are dropped (VSC_REGION_KEEP), 1: those inside
};

// Launch wrappers implemented in vsc_kernels.hip.  They only enqueue work on `stream`.
hipError_t launch_scan(const ScanArgs &args, int n_groups, bool extract, hipStream_t stream);
hipError_t launch_summary(const SummaryArgs &args, hipStream_t stream);
hipError_t launch_summary_regions(const SummaryRegionArgs &args, hipStream_t stream);
hipError_t launch_votes_summary(const VotesSummaryArgs &args, hipStream_t stream);
hipError_t launch_select_score(const SelectArgs &args, hipStream_t stream);      // round 1: scores + histograms
hipError_t launch_select_score_regions(const SelectRegionArgs &args, hipStream_t stream);  // ... on one side of the regions only
hipError_t launch_select_threshold(const SelectArgs &args, hipStream_t stream);  // histograms -> thr, count
hipError_t launch_select_compact(const SelectArgs &args, hipStream_t stream);    // round 2: candidates into their reads' lists
hipError_t launch_select_resolve(const SelectArgs &args, hipStream_t stream);    // later rounds + cut: survivors as packed records
// vsc_sort.hip
hipError_t launch_bin_hist(const SortArgs &args, hipStream_t stream);
hipError_t launch_bin_scan(const SortArgs &args, hipStream_t stream);
hipError_t launch_bin_partition(const SortArgs &args, hipStream_t stream);
hipError_t launch_bin_finalize(const FinArgs &args, int max_groups, hipStream_t stream);
// writes the sentinel into the unused slots of the segments' blocks (a level 1 that needs no partition: the finalize kernel reads
// the search's records as they lie)
hipError_t launch_fill_holes(const SortSeg *segs, uint32_t n_segs, uint64_t *recs, const uint32_t *fill, uint32_t fill_shift, hipStream_t stream);
hipError_t launch_rf_predict(const RfArgs &args, hipStream_t stream);
// vsc_table.hip
hipError_t launch_table_score(const TableArgs &args, hipStream_t stream);
hipError_t launch_table_summary(const TableSummaryArgs &args, hipStream_t stream);
// vsc_efficiency.hip (the definition: vsc_efficiency.h).  The model as the kernels read it: the weights in the
// order of vsc_efficiency.h (the context's device copy), at most kEffMaxWeights of them.
struct EffModelView {
    const double *w;
    double intercept;
    EffShape shape;
    uint32_t n_weights;
};
struct EffArgs {
    EffPlanes g;
    EffModelView m;
    const uint4 *loci;            // vsc_locus
    unsigned long long n;
    double *linear;               // [n] out: the predictor, kEffUndefinedBits where it is undefined
    unsigned long long *stats;    // [kEffClasses], zeroed before the launch: the kernel adds its candidates per class
};
// the filter's two passes, driven by run_enumeration (vsc_api.cpp): tile i of the work list = candidates [i * kEffTile, ..)
constexpr uint32_t kEffTile = 1024;
struct EffFilterArgs {
    EffPlanes g;
    EffModelView m;
    const unsigned long long *in_codes;  // [n] the input's codes and loci
    const uint4 *in_loci;
    unsigned long long n;
    double min_linear;
    const uint32_t *work;          // null: tiles 0 .. n_work - 1
    uint32_t n_work;
    uint32_t *tile_count;          // count pass out: survivors per tile
    const unsigned long long *tile_off;  // write pass in: their exclusive scan
    unsigned long long *codes;     // write pass out
    uint4 *loci;
};
hipError_t launch_eff_score(const EffArgs &args, int n_cus, hipStream_t stream);
hipError_t launch_eff_filter(const EffFilterArgs &args, bool write, hipStream_t stream);
// vsc_eff_trees.hip (the definition: vsc_eff_trees.h).  The model as the kernels read it: the packed words of
// vsc_eff_trees.h (the context's device copy), which every workgroup copies into its LDS.
struct EffTreesView {
    const uint32_t *words;
    uint32_t n_words, n_nodes, n_sums, n_trees;
    double base;
    EffShape shape;  // gc_len 0
};
struct EffTreesArgs {
    EffPlanes g;
    EffTreesView m;
    const uint4 *loci;            // vsc_locus
    unsigned long long n;
    double *linear;               // [n] out: the predictor, kEffUndefinedBits where it is undefined
    unsigned long long *stats;    // [kEffClasses], zeroed before the launch: the kernel adds its candidates per class
};
// the filter's two passes, driven by run_enumeration as EffFilterArgs is: tiles of kEffTile candidates
struct EffTreesFilterArgs {
    EffPlanes g;
    EffTreesView m;
    const unsigned long long *in_codes;  // [n] the input's codes and loci
    const uint4 *in_loci;
    unsigned long long n;
    double min_linear;
    const uint32_t *work;          // null: tiles 0 .. n_work - 1
    uint32_t n_work;
    uint32_t *tile_count;          // count pass out: survivors per tile
    const unsigned long long *tile_off;  // write pass in: their exclusive scan
    unsigned long long *codes;     // write pass out
    uint4 *loci;
};
hipError_t launch_eff_trees_score(const EffTreesArgs &args, int n_cus, hipStream_t stream);
hipError_t launch_eff_trees_filter(const EffTreesFilterArgs &args, bool write, hipStream_t stream);
// vsc_mh.hip (the definition: vsc_mh.h)
struct MhArgs {
    EffPlanes g;
    MhShape shape;
    const uint4 *loci;            // vsc_locus
    unsigned long long n;
    uint2 *out;                   // [n] out: (sum, oof), kMhUndefined twice where the class is not defined
    unsigned long long *stats;    // [kEffClasses], zeroed before the launch: the kernel adds its candidates per class
};
// the filter's two passes, driven by run_enumeration (vsc_api.cpp): tile i of the work list = candidates [i * kMhTile, ..)
constexpr uint32_t kMhTile = 1024;
struct MhFilterArgs {
    EffPlanes g;
    MhShape shape;
    const unsigned long long *in_codes;  // [n] the input's codes and loci
    const uint4 *in_loci;
    unsigned long long n;
    uint32_t min_sum, min_oof_permille;
    const uint32_t *work;          // null: tiles 0 .. n_work - 1
    uint32_t n_work;
    uint32_t *tile_count;          // count pass out: survivors per tile
    const unsigned long long *tile_off;  // write pass in: their exclusive scan
    unsigned long long *codes;     // write pass out
    uint4 *loci;
};
hipError_t launch_mh_score(const MhArgs &args, int n_cus, hipStream_t stream);
hipError_t launch_mh_filter(const MhFilterArgs &args, bool write, hipStream_t stream);
// vsc_fold.hip (the definition: vsc_fold.h)
struct FoldArgs {
    EffPlanes g;
    FoldShape shape;
    const FoldWindow *win;        // [n_diag] the scaffold's windows (fold_scaffold_windows), on the device
    uint32_t n_diag;              // 0: no scaffold
    const uint4 *loci;            // vsc_locus
    unsigned long long n;
    uint2 *out;                   // [n] out: the row, kFoldUndefined twice where the class is not defined
    unsigned long long *stats;    // [kEffClasses], zeroed before the launch: the kernel adds its candidates per class
};
// the filter's two passes, driven by run_enumeration (vsc_api.cpp): tile i of the work list = candidates [i * kFoldTile, ..)
constexpr uint32_t kFoldTile = 1024;
struct FoldFilterArgs {
    EffPlanes g;
    FoldShape shape;
    FoldLimits limits;
    const FoldWindow *win;
    uint32_t n_diag;
    const unsigned long long *in_codes;  // [n] the input's codes and loci
    const uint4 *in_loci;
    unsigned long long n;
    const uint32_t *work;          // null: tiles 0 .. n_work - 1
    uint32_t n_work;
    uint32_t *tile_count;          // count pass out: survivors per tile
    const unsigned long long *tile_off;  // write pass in: their exclusive scan
    unsigned long long *codes;     // write pass out
    uint4 *loci;
};
// groups_per_cu: workgroups per CU the rows kernel's grid is capped at (0: the default, kFoldGroupsPerCu)
hipError_t launch_fold_rows(const FoldArgs &args, int n_cus, uint32_t groups_per_cu, hipStream_t stream);
hipError_t launch_fold_filter(const FoldFilterArgs &args, bool write, hipStream_t stream);
constexpr uint32_t kFoldGroupsPerCu = 8, kFoldMaxGroupsPerCu = 64;
// vsc_motif.hip (the definition: vsc_motif.h)
struct MotifArgs {
    EffPlanes g;
    MotifShape shape;
    MotifTable tab;               // pat: [n_pat] the launch's patterns (motif_layout), on the device
    const uint4 *loci;            // vsc_locus
    unsigned long long n;
    MotifRow *out;                // [n] out: the row, kMotifUndefined three times where the class is not defined
    unsigned long long *stats;    // [kMotifStats], zeroed before the launch: the classes, then the candidates with any construct,
                                  // any cut, any cut-only bit
    unsigned long long *totals;   // null, or [3 n_motifs] zeroed before the launch: per motif the defined candidates with the
                                  // construct, the cut and the cut-only bit
};
// the filter's two passes, driven by run_enumeration (vsc_api.cpp): tile i of the work list = candidates [i * kMotifTile, ..)
constexpr uint32_t kMotifTile = 1024;
struct MotifFilterArgs {
    EffPlanes g;
    MotifShape shape;
    MotifLimits limits;
    MotifTable tab;
    const unsigned long long *in_codes;  // [n] the input's codes and loci
    const uint4 *in_loci;
    unsigned long long n;
    const uint32_t *work;          // null: tiles 0 .. n_work - 1
    uint32_t n_work;
    uint32_t *tile_count;          // count pass out: survivors per tile
    const unsigned long long *tile_off;  // write pass in: their exclusive scan
    unsigned long long *codes;     // write pass out
    uint4 *loci;
};
// groups_per_cu: workgroups per CU the rows kernel's grid is capped at (0: the default, kMotifGroupsPerCu)
hipError_t launch_motif_rows(const MotifArgs &args, int n_cus, uint32_t groups_per_cu, hipStream_t stream);
hipError_t launch_motif_filter(const MotifFilterArgs &args, bool write, hipStream_t stream);
constexpr uint32_t kMotifGroupsPerCu = 8, kMotifMaxGroupsPerCu = 64;
// vsc_edit.hip (the definition: vsc_edit.h)
constexpr uint32_t kEditCounts = kEffClasses + 1;  // the classes, then the candidates with a hit
struct EditArgs {
    EffPlanes g;
    EditShape shape;
    EditTargets targets;          // n == 0: no targets, hits = 0
    const uint4 *loci;            // vsc_locus
    unsigned long long n;
    uint2 *out;                   // [n] out: (mask, hits), kEditUndefined twice where the class is not defined
    unsigned long long *stats;    // [kEditCounts], zeroed before the launch: the kernel adds its candidates per class
};
// the pairs' and the filter's two passes: tile i = candidates [i * kEditTile, ..)
constexpr uint32_t kEditTile = 1024;
struct EditPairArgs {
    EditShape shape;
    EditTargets targets;
    const uint32_t *contig_off;
    const uint4 *loci;            // [n]
    const uint2 *rows;            // [n] what edit_rows_kernel left
    unsigned long long n;
    uint32_t n_work;              // tiles
    uint32_t *tile_count;         // count pass out: pairs per tile
    const unsigned long long *tile_off;  // write pass in: their exclusive scan
    uint4 *pairs;                 // write pass out (null: coverage only)
    uint32_t *cov_count, *cov_min;  // [targets.n] each, write pass: pairs and fewest bystanders per target, 0 / 0xFFFFFFFF before the launch; null: none
};
struct EditFilterArgs {
    EffPlanes g;
    EditShape shape;
    EditTargets targets;
    const unsigned long long *in_codes;  // [n] the input's codes and loci
    const uint4 *in_loci;
    unsigned long long n;
    uint32_t min_editable, max_editable;
    const uint32_t *work;          // null: tiles 0 .. n_work - 1
    uint32_t n_work;
    uint32_t *tile_count;          // count pass out: survivors per tile
    const unsigned long long *tile_off;  // write pass in: their exclusive scan
    unsigned long long *codes;     // write pass out
    uint4 *loci;
};
hipError_t launch_edit_rows(const EditArgs &args, int n_cus, hipStream_t stream);
hipError_t launch_edit_pairs(const EditPairArgs &args, bool write, hipStream_t stream);
hipError_t launch_edit_filter(const EditFilterArgs &args, bool write, hipStream_t stream);
// *out (zeroed) += the entries of cov_count that are not 0
hipError_t launch_edit_covered(const uint32_t *cov_count, uint32_t n_t, unsigned long long *out, int n_cus, hipStream_t stream);
// vsc_variation.hip (the definition: vsc_variation.h)
constexpr uint32_t kVarCounts = kEffClasses + 1;  // the classes, then the candidates with a disrupting variant
// The variants on the device.  They arrive as the caller's 16-byte records { contig, pos, span_alt, weight } in `rec` and are
// rewritten in place as VarRec by three launches: the largest end per tile of kEditTile variants, the prefix maximum over the
// tiles, the records; a fourth fills the block table.
struct VarBuildArgs {
    VarRec *rec;                  // [n] in: the caller's records; out: VarRec
    const uint32_t *contig_off;   // (every contig was checked on the host)
    uint32_t n, n_tiles;
    uint32_t *tile_max;           // [n_tiles] the largest gpos + span of a tile, then of the tiles in front of it
    uint32_t *first;              // [n_blocks + 1] out
    uint32_t bits, n_blocks;
};
struct VarArgs {
    EffPlanes g;
    VarShape shape;
    VarTable table;               // n == 0: no variants, every defined row is 0
    const uint4 *loci;            // vsc_locus
    unsigned long long n;
    uint4 *out;                   // [n] out: (by_zone, silent, cost, max_weight), kVarUndefined four times where the class is not defined
    unsigned long long *stats;    // [kVarCounts], zeroed before the launch: the kernel adds its candidates per class
};
// the pairs' and the filter's two passes: tile i = candidates [i * kEditTile, ..)
struct VarPairArgs {
    VarShape shape;
    VarTable table;
    const uint32_t *contig_off;
    const uint4 *loci;            // [n]
    const uint4 *rows;            // [n] what var_rows_kernel left
    unsigned long long n;
    uint32_t n_work;              // tiles
    uint32_t *tile_count;         // count pass out: pairs per tile, 0xFFFFFFFF: that many or more
    const unsigned long long *tile_off;  // write pass in: their exclusive scan
    uint4 *pairs;                 // write pass out (null: coverage only)
    uint32_t *coverage;           // [2 table.n] write pass: disrupting and silent pairs per variant, 0 before the launch; null: none
};
struct VarFilterArgs {
    EffPlanes g;
    VarShape shape;
    VarTable table;
    VarFilter filter;
    const unsigned long long *in_codes;  // [n] the input's codes and loci
    const uint4 *in_loci;
    unsigned long long n;
    const uint32_t *work;          // null: tiles 0 .. n_work - 1
    uint32_t n_work;
    uint32_t *tile_count;          // count pass out: survivors per tile
    const unsigned long long *tile_off;  // write pass in: their exclusive scan
    unsigned long long *codes;     // write pass out
    uint4 *loci;
};
hipError_t launch_var_build(const VarBuildArgs &args, int n_cus, hipStream_t stream);
hipError_t launch_var_rows(const VarArgs &args, int n_cus, hipStream_t stream);
hipError_t launch_var_pairs(const VarPairArgs &args, bool write, hipStream_t stream);
hipError_t launch_var_filter(const VarFilterArgs &args, bool write, hipStream_t stream);
// *out (zeroed) += the variants with a pair of either kind
hipError_t launch_var_covered(const uint32_t *coverage, uint32_t n_v, unsigned long long *out, int n_cus, hipStream_t stream);
// vsc_prime.hip (the definition: vsc_prime.h)
// the rows kernel's counters: the classes, the candidates with a pair, the weak candidates
constexpr uint32_t kPrimeCounts = kEffClasses + 2;
struct PrimeArgs {
    EffPlanes g;
    PrimeShape shape;
    PrimeEdits edits;             // n == 0: no edits, n_pairs = 0
    const uint4 *loci;            // vsc_locus
    unsigned long long n;
    uint2 *out;                   // [n] out: (pbs, n_pairs), kPrimeUndefined twice where the class is not defined
    unsigned long long *stats;    // [kPrimeCounts], zeroed before the launch: the kernel adds its candidates per counter
};
// the pairs' and the filter's two passes: tile i = candidates [i * kEditTile, ..)
struct PrimePairArgs {
    EffPlanes g;
    PrimeShape shape;
    PrimeEdits edits;
    const uint4 *loci;            // [n]
    const uint2 *rows;            // [n] what prime_rows_kernel left
    unsigned long long n;
    uint32_t n_work;              // tiles
    uint32_t *tile_count;         // count pass out: pairs per tile
    const unsigned long long *tile_off;  // write pass in: their exclusive scan
    uint4 *pairs;                 // write pass out (null: coverage and flag counts only)
    uint32_t *cov_count, *cov_min;  // [edits.n] each, write pass: pairs and smallest t per edit, 0 / 0xFFFFFFFF before the launch; null: none
    unsigned long long *flag_count;  // [kPrimeFlags], zeroed before the launch: the write pass adds its pairs per flag; null: none
};
struct PrimeFilterArgs {
    EffPlanes g;
    PrimeShape shape;
    PrimeEdits edits;
    const unsigned long long *in_codes;  // [n] the input's codes and loci
    const uint4 *in_loci;
    unsigned long long n;
    uint32_t allow_weak;
    const uint32_t *work;          // null: tiles 0 .. n_work - 1
    uint32_t n_work;
    uint32_t *tile_count;          // count pass out: survivors per tile
    const unsigned long long *tile_off;  // write pass in: their exclusive scan
    unsigned long long *codes;     // write pass out
    uint4 *loci;
};
// groups_per_cu: workgroups per CU the rows kernel's grid is capped at (0: the default, kPrimeGroupsPerCu)
hipError_t launch_prime_rows(const PrimeArgs &args, int n_cus, uint32_t groups_per_cu, hipStream_t stream);
hipError_t launch_prime_pairs(const PrimePairArgs &args, bool write, hipStream_t stream);
hipError_t launch_prime_filter(const PrimeFilterArgs &args, bool write, hipStream_t stream);
constexpr uint32_t kPrimeGroupsPerCu = 28, kPrimeMaxGroupsPerCu = 64;
// vsc_hdr.hip (the definition: vsc_hdr.h)
// the rows kernel's counters: the classes, the candidates with a pair, the candidates with a usable pair
constexpr uint32_t kHdrCounts = kEffClasses + 2;
// CODE and the PAM's letter sets, the tables a lane indexes: the kernels copy them to LDS once per workgroup
struct HdrTables {
    uint8_t aa[64];
    uint32_t accept[kHdrMaxPam];
};
struct HdrArgs {
    EffPlanes g;
    HdrShape shape;
    PrimeEdits edits;             // n == 0: no edits, both words of a defined row are 0
    CdsView cds;                  // have_cds == 0: none, ALLOWED always holds
    uint32_t have_cds;
    HdrTables tabs;
    const uint4 *loci;            // vsc_locus
    unsigned long long n;
    uint2 *out;                   // [n] out: (n_pairs, n_usable), kHdrUndefined twice where the class is not defined
    unsigned long long *stats;    // [kHdrCounts], zeroed before the launch: the kernel adds its candidates per counter
};
// the pairs' and the filter's two passes: tile i = candidates [i * kEditTile, ..)
struct HdrPairArgs {
    EffPlanes g;
    HdrShape shape;
    PrimeEdits edits;
    CdsView cds;
    uint32_t have_cds;
    HdrTables tabs;
    const uint4 *loci;            // [n]
    const uint2 *rows;            // [n] what hdr_rows_kernel left
    unsigned long long n;
    uint32_t n_work;              // tiles
    uint32_t *tile_count;         // count pass out: pairs per tile
    const unsigned long long *tile_off;  // write pass in: their exclusive scan
    uint4 *pairs;                 // write pass out (null: coverage and flag counts only)
    uint32_t *cov_count, *cov_min;  // [edits.n] each, write pass: usable pairs and their smallest dist per edit, 0 / 0xFFFFFFFF before the launch; null: none
    unsigned long long *flag_count;  // [kHdrFlags], zeroed before the launch: the write pass adds its pairs per flag; null: none
};
struct HdrFilterArgs {
    EffPlanes g;
    HdrShape shape;
    PrimeEdits edits;
    CdsView cds;
    uint32_t have_cds;
    HdrTables tabs;
    const unsigned long long *in_codes;  // [n] the input's codes and loci
    const uint4 *in_loci;
    unsigned long long n;
    uint32_t allow_open;
    const uint32_t *work;          // null: tiles 0 .. n_work - 1
    uint32_t n_work;
    uint32_t *tile_count;          // count pass out: survivors per tile
    const unsigned long long *tile_off;  // write pass in: their exclusive scan
    unsigned long long *codes;     // write pass out
    uint4 *loci;
};
// groups_per_cu: workgroups per CU the rows kernel's grid is capped at (0: the default, kHdrGroupsPerCu)
hipError_t launch_hdr_rows(const HdrArgs &args, int n_cus, uint32_t groups_per_cu, hipStream_t stream);
hipError_t launch_hdr_pairs(const HdrPairArgs &args, bool write, hipStream_t stream);
hipError_t launch_hdr_filter(const HdrFilterArgs &args, bool write, hipStream_t stream);
constexpr uint32_t kHdrGroupsPerCu = 28, kHdrMaxGroupsPerCu = 64;
// vsc_effects.hip (the definition: vsc_effects.h)
constexpr uint32_t kEffectsCounts = kEffClasses + 1 + kEffectClasses;  // the candidates' classes, the candidates with an effect, the effects by class
struct EffectsCode {
    uint8_t aa[64];               // CODE
};
struct EffectsArgs {
    EffPlanes g;
    EditShape shape;
    uint32_t to;
    CdsView cds;
    EffectsCode code;
    const uint4 *loci;            // vsc_locus
    unsigned long long n;
    uint2 *out;                   // [n] out: ROW, kEffectsUndefined twice where the class is not defined
    unsigned long long *stats;    // [kEffectsCounts], zeroed before the launch
};
// the records' two passes: tile i = candidates [i * kEditTile, ..)
struct EffectsRecordArgs {
    EffPlanes g;
    EditShape shape;
    uint32_t to;
    CdsView cds;
    EffectsCode code;
    const uint4 *loci;            // [n]
    const uint2 *rows;            // [n] what effects_rows_kernel left
    unsigned long long n;
    uint32_t n_work;              // tiles
    uint32_t *tile_count;         // count pass out: effects per tile
    const unsigned long long *tile_off;  // write pass in: their exclusive scan
    uint4 *effects;               // write pass out (null: coverage only)
    uint32_t *cov_count, *cov_min;  // [n_tx] each, write pass: stop_gained effects and their smallest codon per transcript, 0 / 0xFFFFFFFF before the launch; null: none
    uint32_t n_tx;
};
struct EffectsFilterArgs {
    EffPlanes g;
    EditShape shape;
    uint32_t to;
    CdsView cds;
    EffectsCode code;
    const unsigned long long *in_codes;  // [n] the input's codes and loci
    const uint4 *in_loci;
    unsigned long long n;
    uint32_t require, forbid;
    const uint32_t *work;          // null: tiles 0 .. n_work - 1
    uint32_t n_work;
    uint32_t *tile_count;          // count pass out: survivors per tile
    const unsigned long long *tile_off;  // write pass in: their exclusive scan
    unsigned long long *codes;     // write pass out
    uint4 *loci;
};
hipError_t launch_effects_rows(const EffectsArgs &args, int n_cus, hipStream_t stream);
hipError_t launch_effects_records(const EffectsRecordArgs &args, bool write, hipStream_t stream);
hipError_t launch_effects_filter(const EffectsFilterArgs &args, bool write, hipStream_t stream);
// vsc_knockout.hip (the definition: vsc_knockout.h)
// the rows kernel's counters: defined and undefined candidates, coding cuts, junction cuts, PTC and NMD in both frames, rows
// with an unknown walk, the candidates the bitmap sent past cds_find, the drains of the queue and the entries they held
constexpr uint32_t kKoCounts = 12;
struct KoArgs {
    EffPlanes g;
    KoShape shape;
    CdsView cds;
    const KoTx *tx;               // [n_tx]
    const uint32_t *bitmap;       // one bit per block of 2^kKoBlockBits global positions, n_blocks of them
    uint32_t n_blocks, n_tx;
    EffectsCode code;
    const uint4 *loci;            // vsc_locus
    unsigned long long n;
    uint4 *out;                   // [n] out: ROW
    unsigned long long *stats;    // [kKoCounts], zeroed before the launch
    uint32_t *cov_count, *cov_min;  // [n_tx] each: candidates with NMD1 and NMD2 and their smallest codon per transcript, 0 / 0xFFFFFFFF before the launch; null: none
};
struct KoFilterArgs {
    EffPlanes g;
    KoShape shape;
    KoFilter filter;
    CdsView cds;
    const KoTx *tx;
    const uint32_t *bitmap;
    uint32_t n_blocks, n_tx;
    EffectsCode code;
    const unsigned long long *in_codes;  // [n] the input's codes and loci
    const uint4 *in_loci;
    unsigned long long n;
    const uint32_t *work;          // null: tiles 0 .. n_work - 1
    uint32_t n_work;
    uint32_t *tile_count;          // count pass out: survivors per tile
    const unsigned long long *tile_off;  // write pass in: their exclusive scan
    unsigned long long *codes;     // write pass out
    uint4 *loci;
};
// groups_per_cu: workgroups per CU the rows kernel's grid is capped at (0: the default, kKoGroupsPerCu)
// in_place: the variant without the queue, every coding lane walking where it lies (vsc_debug_knockout_in_place)
hipError_t launch_knockout_rows(const KoArgs &args, int n_cus, uint32_t groups_per_cu, bool in_place, hipStream_t stream);
hipError_t launch_knockout_filter(const KoFilterArgs &args, bool write, hipStream_t stream);
constexpr uint32_t kKoGroupsPerCu = 8, kKoMaxGroupsPerCu = 64;
hipError_t launch_interleave(const uint32_t *hi, const uint32_t *lo, uint64_t n, uint2 *hl, hipStream_t stream);
hipError_t launch_score(const ScoreArgs &args, hipStream_t stream);
hipError_t launch_score_packed(const ScoreArgs &args, uint4 *packed, hipStream_t stream);
// Fills seg_start / seg_prefix for the hits of args (sorted by guide, strand, position; guides g_lo .. g_hi occur):
// segments = (slice of 2^slice_shift positions, guide, strand), slice-major.  bounds: scratch of
// (g_hi - g_lo + 1) * 2 * (n_slices + 1) 64-bit words.
hipError_t launch_score_schedule(const ScoreArgs &args, uint32_t g_lo, uint32_t g_hi, uint32_t slice_shift, uint32_t n_slices,
                                 uint64_t *bounds, uint64_t *seg_start, uint64_t *seg_prefix, hipStream_t stream);
hipError_t launch_score_pairs(const uint2 *on, const uint2 *off, const uint32_t *masks, uint64_t n, double *mit,
                              uint8_t *mit_flags, uint8_t *features, hipStream_t stream);
// 8-byte exchange records (vsc_hits_pack_exchange / vsc_hits_merge_packed)
hipError_t launch_xpack(const vsc_hit *in, uint64_t n, const uint32_t *contig_off, uint64_t *out, hipStream_t stream);
// bound[k] = first record of in[range_dev[0] .. range_dev[1]) whose key (guide << 1 | strand) is >= k, k = 0 .. K
hipError_t launch_key_bounds(const vsc_hit *in, const uint64_t *range_dev, uint32_t K, uint64_t *bound, hipStream_t stream);
// seg_src / seg_side: ADDRESSES of every (key, shard) segment's records / 16-bit side values (seg_side, side_out: null = none)
hipError_t launch_merge_packed(const uint64_t *seg_src, const uint64_t *seg_dst, const uint32_t *seg_n, uint32_t n_segs, uint32_t n_shards,
                               uint32_t first_key, const uint32_t *contig_off, const uint32_t *contig_end, uint32_t n_contigs, vsc_hit *out,
                               uint32_t *bad /* zeroed */, const uint64_t *seg_side, uint16_t *side_out, hipStream_t stream);
// *out += fingerprint of words [0, n_words) of the three planes (zero *out first)
hipError_t launch_plane_hash(const uint32_t *hi, const uint32_t *lo, const uint32_t *nm, uint64_t n_words, unsigned long long *out,
                             hipStream_t stream);
// vsc_seed.hip
hipError_t launch_seed_keys(const uint4 *rec, uint64_t n, int seg, uint32_t pam_codes, uint32_t n_pam, uint64_t *sort_records, hipStream_t stream);
hipError_t launch_seed_lists(const uint2 *guides, uint32_t n_guides, const SeedPlan &plan, uint32_t *count, uint32_t *poff, uint2 *list_rest,
                             hipStream_t stream);
hipError_t launch_seed_pack16(const uint32_t *x, const uint32_t *l, const uint32_t *pos, uint64_t n, uint4 *rec, hipStream_t stream);
hipError_t launch_seed_gather16(const uint4 *rec, const uint64_t *sorted, uint64_t n, uint4 *out, hipStream_t stream);
hipError_t launch_seed_compact(const uint4 *sites16, uint64_t n_per_table, uint64_t n, uint2 *sites8, uint32_t *edge_bits,
                               hipStream_t stream);
hipError_t launch_seed_chunk_flags(uint4 *chunk_tab, uint32_t n_chunks, const uint32_t *edge_bits, hipStream_t stream);
hipError_t launch_seed_transpose(const uint4 *sites, const uint4 *chunk_tab, uint32_t n_chunks, uint32_t *vert,
                                 hipStream_t stream);
hipError_t launch_seed_sliced(const SeedArgs &args, int n_groups, bool shared, hipStream_t stream);
hipError_t launch_merge(const vsc_hit *in, const uint64_t *shard_off_dev, uint32_t n_shards, uint32_t K, uint64_t *bound,
                        uint64_t *key_off, vsc_hit *out, hipStream_t stream);

}  // namespace vsc
