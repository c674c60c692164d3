// vsc_objects.h - the objects behind the opaque handles of include/varscot_hip.h, shared by the host-side
// translation units of the library (vsc_api.cpp, vsc_multi.cpp, vsc_regions.cpp) and by the device stand-in of the CPU
// tests (tools/multi_tsan/stub_device.cpp).  Not installed.
#pragma once

#include <string>
#include <vector>

#include "varscot_hip_debug.h"
#include "vsc_internal.h"
#include "vsc_pattern_table.h"

namespace vsc {

struct DeviceBuf {
    void *p = nullptr;
    size_t cap = 0;
    // hipMalloc / hipFree of multi-GB buffers cost hundreds of milliseconds: grow with 1/8 headroom so
    // that result sizes that wobble from search to search do not reallocate every time
    hipError_t ensure(size_t bytes)
    {
        if (bytes <= cap) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        size_t want = bytes + (bytes < ((size_t)32 << 30) ? bytes / 8 : bytes / 32);  // (3 % on buffers of tens of GB: batch sizes wobble by 1 %)
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess && want != bytes) {
            (void)hipGetLastError();
            want = bytes;
            e = hipMalloc(&p, want);
        }
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

inline vsc_debug_params default_debug_params()
{
    vsc_debug_params d{};
    d.sort_xcd = -1;
    d.sort_optimistic = -1;
    d.score_slices = -1;
    d.seed_shared = -1;
    d.seed_group_out = -1;
    d.seed_tight = -1;
    d.rf_form = -1;
    return d;
}

// process-wide: host-side lap times on stderr (vsc_debug_set_host_timing)
bool host_timing_on();

}  // namespace vsc

// The events of a context (vsc_ctx::ev), by what its stream has reached when they are recorded.  A search pass records
// kEvPassStart .. kEvSinkEnd and kEvPrepEnd: prep_ms = pass start -> prep end, scan_ms = search start -> end, sort_ms = search
// end -> sink start, finalize_ms = sink start -> end (the sink's last stage), total_ms = pass start -> sink end.  The index
// build has a pair of its own: it runs inside a search call, before the first pass.  The calls that are no search pass
// (scoring, forest, merge, enumeration) time their one or two stages with the first four events under the kEvStage names.
enum vsc_event {
    kEvPassStart = 0,
    kEvSearchStart,
    kEvSearchEnd,
    kEvSinkStart,
    kEvSinkEnd,
    kEvIndexStart,
    kEvIndexEnd,
    kEvPrepEnd,
    kEvClassStart,  // the classify kernel of a pass (vsc_search_*_classified): score_ms
    kEvClassEnd,
    kEvCount,
    kEvStageStart = kEvPassStart,
    kEvStageEnd = kEvSearchStart,
    kEvStage2Start = kEvSearchEnd,
    kEvStage2End = kEvSinkStart,
};

struct vsc_ctx {
    int device = 0;
    int n_cus = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    hipEvent_t ev[kEvCount] = {};  // by vsc_event
    std::string err;
    vsc_timing timing{};
    vsc_debug_params dbg = vsc::default_debug_params();  // test / experiment hooks (include/varscot_hip_debug.h)
    // keys_a / keys_b: the two record buffers the bin sort alternates between (keys_a + vals_a: the scan's (key, value) pairs)
    vsc::DeviceBuf counters, guides, keys_a, keys_b, vals_a, score_mit, score_flags, score_feat;
    vsc::DeviceBuf vals_b;  // side words beside keys_b (searches that keep the sites' bases; vals_a then holds those beside keys_a)
    // the read planes of the scoring calls (their own buffer: `guides` is the search passes'), kept while the read set stays the same
    vsc::DeviceBuf score_guides;
    uint64_t score_guides_hash = 0;
    uint32_t score_guides_n = ~0u;
    vsc::DeviceBuf sort_segs, sort_tabs, sort_over, score_sched;
    // host staging of the sort's segment tables: uploaded with hipMemcpyAsync, so they must outlive the call that enqueues them
    std::vector<vsc::SortSeg> host_segs;
    std::vector<uint32_t> host_tile0;  // bin sort: segment table + tile starts, per-bin tables, oversize list + counter
    vsc::DeviceBuf seed_off, seed_poff, seed_lrest;  // per-search read lists: bucket counts, padded list starts, entries
    vsc::DeviceBuf seed_fill;  // the block fill table of a seed search whose records go straight to the sort (SeedArgs.fill)
    // A seed search in parts (find_pass): the level-1 partition of every part runs on stream_b beside the next part of the
    // search on `stream`, ordered by the events of part_ev alone (per part: start, end, counters copied; then the join);
    // `pinned` stages what goes to and from the device while kernels run (per part: the counters, the segments, their tiles).
    // All made on first use.  cu_masked: the context's stream is bound to a set of CUs - such a context never searches in parts.
    hipStream_t stream_b = nullptr;
    std::vector<hipEvent_t> part_ev;
    void *pinned = nullptr;
    size_t pinned_cap = 0;
    bool cu_masked = false;
    vsc::DeviceBuf sum_rows, sum_excl;  // vsc_search_summary: the per-read rows it adds into, the excluded loci
    // vsc_search_select: per-read tables of a pass (score histograms, thresholds, counts, cursors, list starts), the candidates' keys and masks
    vsc::DeviceBuf sel_hist, sel_tabs, sel_keys, sel_masks;
    // vsc_search_*_regions: the rows over the hits in the regions (beside sum_rows), and the device copy of the regions this
    // context used last - start[], end_max[], class table in one buffer - keyed by the serial number of the vsc_regions
    vsc::DeviceBuf sum_rows_in, regions_buf;
    // vsc_search_*_classified: the per-read vsc_guide_votes rows (the votes words beside the records lie in vals_b)
    vsc::DeviceBuf votes_rows;
    uint64_t regions_serial = 0;  // 0: none resident
    // vsc_score_hits_table / vsc_search_*_table: the device copy of the score table this context used last (336 doubles, keyed
    // by the table's serial number) and the per-read vsc_guide_table_row rows (the fixed-point words beside the records lie
    // in vals_b; vsc_score_hits_table's outputs go through score_mit / score_flags)
    vsc::DeviceBuf table_buf, table_rows;
    uint64_t table_serial = 0;  // 0: none resident
    // vsc_*_efficiency: the device copy of the efficiency model this context used last (its weights in the order of
    // vsc_efficiency.h, keyed by the model's serial number), the candidates of a call that brings them from the host (loci;
    // the filter of a host-only object: codes, then loci) and the call's outputs (the class counts, then the scores).
    // vsc_*_microhomology (no model) bring their candidates in eff_in and leave their pairs in eff_out as well.
    vsc::DeviceBuf eff_buf, eff_in, eff_out;
    uint64_t eff_serial = 0;  // 0: none resident
    // vsc_*_efficiency_trees: the device copy of the tree model this context used last (its packed words,
    // vsc_eff_trees.h), keyed by the model's serial number, beside the linear model's
    vsc::DeviceBuf eff_trees_buf;
    uint64_t eff_trees_serial = 0;  // 0: none resident
    // vsc_*_pick: what a call uploads (keys, then the targets or the groups, then the loci of a call that brings
    // them from the host), the call's tables (targets per candidate, per-target counts, segment offsets, cursors, stats, picks,
    // counts, ranks) and the records of the eligible candidates in their targets' segments
    vsc::DeviceBuf pick_in, pick_tabs, pick_recs;
    // vsc_*_edit: the call's tables (the targets' global positions, the coverage counters, the pairs' per-tile
    // counts and offsets) and its pairs; the candidates a call brings from the host and the rows lie in eff_in / eff_out
    vsc::DeviceBuf edit_tabs, edit_pairs;
    // vsc_*_prime keep their tables (the edits' global positions, the edits, the occupancy bitmap, the coverage
    // counters, the per-tile counts and offsets) in edit_tabs and their pairs in edit_pairs as well
    bool prime_bitmap = true;  // vsc_debug_prime_bitmap: ask the occupancy bitmap before the edit search
    uint32_t prime_groups_per_cu = 0;  // vsc_debug_prime_groups_per_cu: the cap of prime_rows_kernel's grid (0: the default)
    bool hdr_bitmap = true;  // vsc_debug_hdr_bitmap: ask the occupancy bitmap before the edit search
    uint32_t hdr_groups_per_cu = 0;  // vsc_debug_hdr_groups_per_cu: the cap of hdr_rows_kernel's grid (0: the default)
    // vsc_*_fold upload their scaffold's windows into eff_buf (the efficiency model's copy is forgotten: eff_serial 0)
    uint32_t fold_groups_per_cu = 0;  // vsc_debug_fold_groups_per_cu: the cap of fold_rows_kernel's grid (0: the default)
    // vsc_*_motifs upload their patterns (and the zeroed totals behind them) into eff_buf, as the fold calls do
    uint32_t motif_groups_per_cu = 0;  // vsc_debug_motif_groups_per_cu: the cap of motif_rows_kernel's grid (0: the default)
    uint32_t variation_block_bits = 0;  // vsc_debug_variation_block_bits: the block of the variation lookup (0: kVarBlockBits)
    // vsc_*_effects: the device copy of the CDS this context walked last - the segments' global starts, then the
    // segments, keyed by the object's serial number as locate_buf is; the call's tables and records lie in edit_tabs / edit_pairs
    vsc::DeviceBuf cds_buf;
    uint64_t cds_serial = 0;  // 0: none resident
    // vsc_*_knockout: the per-transcript table and the occupancy bitmap of the CDS this context walked last,
    // beside cds_buf and keyed as it is
    vsc::DeviceBuf ko_buf;
    uint64_t ko_serial = 0;  // 0: none resident
    bool knockout_in_place = false;       // vsc_debug_knockout_in_place: knockout_rows_kernel without its queue
    uint32_t knockout_groups_per_cu = 0;  // vsc_debug_knockout_groups_per_cu: the cap of knockout_rows_kernel's grid (0: the default)
    // vsc_hits_locate / vsc_guides_locate: the device copy of the label structure of the regions this context located against
    // last - end[], index[], up[], contig offsets and lengths in one buffer, keyed as regions_buf is - and the labels on their
    // way to the host
    vsc::DeviceBuf locate_buf, locate_out;
    uint64_t locate_serial = 0;  // 0: none resident
    // vsc_hits_variants / vsc_search_summary_variants: the device copy of the variant map this context merged against last -
    // windows, then variants, keyed by the map's serial number - the call's state (error flag, then the zeroed rows and
    // duplicate counts), the excluded loci in reference coordinates, and the labels on their way to the host
    vsc::DeviceBuf varmap_buf, var_state, var_excl, var_labels;
    uint64_t varmap_serial = 0;  // 0: none resident
    // the pattern variant screen: the shadow intervals of the map last used (start[], then end_max[]), the call's
    // state (error flag and rows), and the flags of vsc_pattern_hits_shadowed
    vsc::DeviceBuf pv_shadow_buf, pv_state, pv_flags;
    uint64_t pv_shadow_serial = 0;
    // vsc_guides_enumerate: the work list (tiles to visit), the per-tile counts and their exclusive scan;
    // vsc_guides_enumerate_pattern: the same three parts, then the targets' start ranges
    vsc::DeviceBuf enum_tabs;
    // vsc_hits_pairs / vsc_guides_pairs: the call's tables (segment starts, pairs, their item offsets, excluded loci, rows),
    // the per-item counts with their exclusive scan, and the sites / pairs on their way to the host
    vsc::DeviceBuf pairs_tabs, pairs_items, pairs_out;
    // vsc_search_bulges: the call's rows and site counter, then per round the reads' planes, the counts per (read, strand,
    // tile) cell, their sums per 64 cells and the scan of those - guide_batch bounds it
    vsc::DeviceBuf bulge_tabs;
    // vsc_search_pattern: the same parts - rows and site counter, then per round the guides' planes, the counts per cell,
    // their sums per 64 cells and the scan of those
    vsc::DeviceBuf pattern_tabs;
    // vsc_search_pattern_table: the device copy of the pattern table this context used last (at most 768 doubles, keyed by
    // the table's serial number)
    vsc::DeviceBuf pattern_table_buf;
    uint64_t pattern_table_serial = 0;  // 0: none resident
    // vsc_hits_sites: the tiles' ballots, their offsets, the invalid flag, the rows and the tiles' counts; the milliseconds of
    // the call's two stages (flag pass + scan, write pass: vsc_debug_sites_ms - vsc_ctx_timing is not the call's to change)
    vsc::DeviceBuf sites_tabs;
    double sites_ms[2] = {0, 0};
    // vsc_bulge_hits_table / vsc_sites_table: the device copy of the bulge table this context used last (at most 1 024 doubles,
    // keyed by the table's serial number), the call's tables (the guides' words and planes, the rows, the selection's bounds
    // and thresholds), the score records of a call that selects, and the milliseconds of the call's stages (score kernel,
    // bounds + select, walk: vsc_debug_site_table_ms)
    vsc::DeviceBuf bulge_table_buf, site_table_tabs, site_table_scores;
    uint64_t bulge_table_serial = 0;  // 0: none resident
    double site_table_ms[3] = {0, 0, 0};
    // the forest of the last classification call, as the kernels read it (prepare_forest in vsc_api.cpp)
    struct Forest {
        vsc::DeviceBuf nodes, ranks;   // nodes + tree depths + test table; activity ranks of the reads of a fused call
        size_t depth_at = 0, tests_at = 0, begin_at = 0;
        uint32_t n_tests = 0, n_trees = 0, n_nodes = 0;
        uint32_t form = 0;              // node form (vsc_internal.h): 0 plain, 1 compact, 2 pairs
        uint32_t node_stride = 0;       // nodes from one tree's root to the next (n_nodes; pair form: the largest tree's pair nodes)
        std::vector<double> thresholds;  // distinct activity splits, ascending
        uint64_t fingerprint = 0;
        uint64_t ranks_key = 0;  // activities + forest the resident ranks were made from
        uint32_t ranks_n = ~0u;
    } forest;
    // record buffers of freed results, kept for the next search: hipMalloc / hipFree of tens of GB
    // cost hundreds of milliseconds each
    std::vector<vsc::DeviceBuf> spare_records;
};

struct vsc_genome {
    vsc_ctx *ctx = nullptr;
    uint32_t *d_hi = nullptr, *d_lo = nullptr, *d_nm = nullptr;
    uint32_t *d_contig_off = nullptr, *d_contig_end = nullptr;
    std::vector<uint32_t> h_contig_off, h_contig_end;  // the same table on the host (what regions are checked against)
    uint2 *d_hl = nullptr;  // interleaved planes, built on first scoring call
    uint64_t first_word = 0, own_words = 0, dev_words = 0;
    uint64_t held_words = 0;  // the words the genome was loaded with (own + halo): what dev_words pads with N is not the genome's
    uint32_t n_tiles = 0, n_contigs = 0;
    uint64_t device_bytes = 0;
    // sites, seen_rate, sort_slots_ok: sizing hints that searches learn (mutable: a search takes the genome as const)
    mutable uint64_t sites = 0;  // PAM-valid windows seen by the last scan (sizes the next hit buffer)
    mutable uint64_t checked_map_serial = 0;  // the vsc_variant_map whose windows were last found to be this genome's contigs (0: none)
    // hits per read the last search with mismatch budget m produced (scan: all reads; seed: the fullest output
    // region) - real genomes are not the uniform model the first buffer size comes from
    mutable double seen_rate[VSC_MAX_MISMATCHES + 1] = {};
    // the sort's first level may skip its histogram pass (slot partition) until a search with this budget has
    // produced a bin that outgrew its slot (repeats)
    mutable bool sort_slots_ok[VSC_MAX_MISMATCHES + 1] = {true, true, true, true, true, true, true, true, true};
    // seed index (vsc_seed.hip): the PAM-valid sites filed once per segment, sorted by bucket
    bool has_index = false;
    uint8_t index_has_extra_pam = 0;
    char index_extra_pam[2] = {0, 0};
    uint64_t index_sites = 0;  // S
    uint4 *d_ix_chunk_tab = nullptr;
    uint32_t *d_ix_vert = nullptr;  // bit-sliced blocks of 32 sites
    uint2 *d_ix_sites = nullptr;    // 8-byte site records {rest planes, position}
    uint32_t *d_ix_edge = nullptr;  // 1 bit per site: window followed by N
    uint32_t ix_chunks = 0;
    uint64_t ix_class_sites[4] = {};   // sites per PAM class in one table, chunks per class over all three (the search's cost model)
    uint64_t ix_class_chunks[4] = {};
    uint64_t ix_vert_bytes = 0, ix_edge_words = 0;  // sizes of d_ix_vert / d_ix_edge (the index file stores them)
    uint64_t index_bytes = 0;
    double index_ms = 0;
};

// An annotation as the sinks test hits against it (include/varscot_hip.h; built by vsc_regions.cpp).  Immutable once built.
struct vsc_regions {
    std::vector<uint32_t> start, end_max, cls;  // vsc::RegionsView's arrays
    std::vector<uint32_t> contig_off, contig_len;  // the genome's table the intervals were placed in
    // vsc::LocateView's arrays (vsc_enum.h): the kept intervals by (start ascending, end descending, input index descending).
    // has_locate == false: more input intervals than a 32-bit label can number, the three arrays are empty
    std::vector<uint32_t> loc_end, loc_index, loc_up;
    bool has_locate = false;
    uint64_t n_input = 0;  // intervals the caller gave (labels number them; vsc_*_pick's group[] has one entry per each)
    uint32_t rule = 0, block_shift = 0, n_blocks = 0;
    uint64_t serial = 0;  // process-wide, handed out by vsc_regions_build: what a context's device copy is keyed by
    vsc_regions_stats stats{};
    vsc::RegionsView view() const
    {
        return vsc::RegionsView{start.data(), end_max.data(), cls.data(), (uint32_t)start.size(), n_blocks, block_shift, rule};
    }
};

// A CDS annotation as the effects kernels walk it (include/varscot_hip.h "SEGMENT / CODING"; built and checked by
// vsc_cds_build).  Host-only, immutable once built.
struct vsc_cds {
    std::vector<uint32_t> contig_off, contig_len;  // the genome's table the segments were placed in
    std::vector<uint32_t> gstart;                  // vsc::CdsView's arrays
    std::vector<vsc::CdsSeg> seg;
    std::vector<vsc::KoTx> ko_tx;                  // per transcript, what the knock-out walk reads (vsc_knockout.h); n_tx entries
    std::vector<uint32_t> ko_bitmap;               // one bit per block of 2^kKoBlockBits global positions that overlaps a segment
    uint32_t ko_blocks = 0;                        // its bits
    uint32_t n_tx = 0;
    uint64_t serial = 0;  // process-wide, handed out by vsc_cds_build: what a context's device copy is keyed by
    vsc_cds_stats stats{};
    vsc::CdsView view() const { return vsc::CdsView{gstart.data(), seg.data(), (uint32_t)seg.size()}; }
};

// A score table (include/varscot_hip.h "TABLE"; built and checked by vsc_score_table_build).  Host-only, immutable once built.
struct vsc_score_table {
    double w[336];        // pair[20][4][4], then pam[16] (vsc_table.h: kTableWeights)
    uint64_t serial = 0;  // process-wide, handed out by vsc_score_table_build: what a context's device copy is keyed by
    uint32_t zeros = 0;   // weights that are exactly 0
};

// A pattern score table (include/varscot_hip.h "TABLE" of vsc_search_pattern_table; built and checked by
// vsc_pattern_table_build).  Host-only, immutable once built.
struct vsc_pattern_table {
    vsc::PatTableShape shape{};
    double w[vsc::kPatTableMaxWeights] = {};  // pair[ps_len][4][4], then pam[4^n_pam] (vsc_pattern_table.h)
    uint64_t serial = 0;  // process-wide, handed out by vsc_pattern_table_build: what a context's device copy is keyed by
    uint32_t zeros = 0;   // weights that are exactly 0
};

// A bulge score table (include/varscot_hip.h "TABLE" of vsc_bulge_hits_table; built and checked by vsc_bulge_table_build).
// Host-only, immutable once built.
struct vsc_bulge_table {
    vsc::PatTableShape shape{};
    double w[vsc::kPatTableMaxWeights + 2 * vsc::kPatTableMaxLen * 4] = {};  // the pattern table's, then dna, then rna (vsc_bulge_table.h)
    uint64_t serial = 0;  // process-wide, handed out by vsc_bulge_table_build: what a context's device copy is keyed by
    uint32_t zeros = 0;   // weights that are exactly 0
};

// An efficiency model (include/varscot_hip.h "MODEL"; built and checked by vsc_eff_model_build).  Host-only, immutable once built.
struct vsc_eff_model {
    vsc::EffShape shape{};
    uint32_t link = 0;
    double intercept = 0;
    std::vector<double> w;  // mono, the transposed di, gc (vsc_efficiency.h): what the device copy holds
    uint64_t serial = 0;    // process-wide, handed out by vsc_eff_model_build: what a context's device copy is keyed by
    uint32_t nonzero = 0;   // weights that are not 0
};

// A regression-tree efficiency model (include/varscot_hip.h "SUMS / TREES"; built and checked by vsc_eff_trees_build).
// Host-only, immutable once built.
struct vsc_eff_trees {
    vsc::EffShape shape{};  // gc_len 0
    uint32_t link = 0;
    double base = 0;
    std::vector<uint32_t> words;  // the packed model of vsc_eff_trees.h: what the device copy holds
    uint32_t n_sums = 0, n_trees = 0, n_nodes = 0;
    uint32_t by_kind[4] = {};     // nodes by VSC_EFF_NODE_*
    uint32_t max_depth = 0;
    uint64_t serial = 0;          // process-wide, handed out by vsc_eff_trees_build: what a context's device copy is keyed by
};

struct vsc_hits {
    vsc_ctx *ctx = nullptr;
    vsc_hit *d_records = nullptr;
    vsc::DeviceBuf storage;  // owns d_records
    uint64_t n = 0;
    std::vector<vsc_hit> host;
    bool host_valid = false;
};

namespace vsc {

// Candidate guides: two device arrays the object owns (ctx != null), or host arrays only (vsc_multi_guides_enumerate:
// ctx == null, host_valid from the start).
struct GuideList {
    vsc_ctx *ctx = nullptr;
    DeviceBuf storage;  // codes (n x 8 bytes), then the loci (n x 16 bytes) from loci_at on
    size_t loci_at = 0;
    uint64_t n = 0;
    std::vector<uint64_t> codes;
    std::vector<vsc_locus> loci;
    bool host_valid = false;
};

// The records of a count / scan / write search: one device array the object owns.
template <class Rec> struct RecordList {
    typedef Rec record;
    vsc_ctx *ctx = nullptr;
    DeviceBuf storage;
    uint64_t n = 0;
    std::vector<Rec> host;
    bool host_valid = false;
    // a scored search (vsc_search_pattern_table): one uint32_t per record behind the records, side_at bytes into storage
    bool has_side = false;
    size_t side_at = 0;
    std::vector<uint32_t> side_host;
    bool side_host_valid = false;
    uint32_t site_len = 0;  // a pattern search: the length L it was searched with (what vsc_pattern_hits_variants walks with)
};

}  // namespace vsc

// The five handles of include/varscot_hip.h behind which these stand: the candidates of vsc_guides_enumerate and of
// vsc_guides_enumerate_pattern, the records of vsc_search_bulges (and vsc_search_pattern_bulges), of vsc_search_pattern and of
// vsc_hits_sites.
struct vsc_guides : vsc::GuideList {};
struct vsc_pattern_guides : vsc::GuideList {};
struct vsc_bulge_hits : vsc::RecordList<vsc_bulge_hit> {};
struct vsc_pattern_hits : vsc::RecordList<vsc_pattern_hit> {};
struct vsc_sites : vsc::RecordList<vsc_site> {
    // a scored result (vsc_sites_table): one vsc_site_score per record behind the records, scores_at bytes into storage
    bool has_scores = false;
    size_t scores_at = 0;
    std::vector<vsc_site_score> scores_host;
    bool scores_host_valid = false;
};

namespace vsc {
// A genome object that only carries the contig table (no planes, nothing to search): what vsc_hits_merge_packed
// needs on a device whose shard of a tiny genome is empty (vsc_multi.cpp).  Freed with vsc_genome_free.
int genome_table_only(vsc_ctx *ctx, const vsc_contig *contigs, uint32_t n_contigs, vsc_genome **out);
// vsc_hits_merge_packed over per-shard record buffers on ctx's device, with optional 16-bit side values per record that
// arrive in side_out in merged order (vsc_api.cpp)
int merge_packed_shards(vsc_ctx *ctx, const vsc_genome *genome, const void *const *shard_records, const void *const *shard_side,
                        const uint32_t *key_counts, uint32_t n_shards, uint32_t first_key, uint32_t n_keys, vsc_hits **out,
                        DeviceBuf *side_out);
}  // namespace vsc
