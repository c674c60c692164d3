// vsc_table.hip - the table-driven off-target score on the device: table_score_kernel over sorted hits or over
// the search kernel's records where they lie, table_summary_kernel over the words it leaves beside them.  The score itself
// is table_score of vsc_table.h, the function vsc_table_score calls on the host.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "vsc_sink.h"
#include "vsc_table.h"

namespace vsc {

namespace {

constexpr int kTabThreads = 256;
constexpr int kTabTilesPerBlock = 4;  // record sources: tiles of kSumTile slots a workgroup walks with one load of the weights
enum { kTabHits = 0, kTabScan = 1, kTabSeed = 2 };

// the 23-base planes at shard-relative position rel, in read orientation for strand `rev`
__device__ __forceinline__ void table_site(const TableArgs &a, uint32_t rel, bool rev, uint32_t &sh, uint32_t &sl)
{
    const uint64_t wi = rel >> 5;
    const uint32_t shft = rel & 31u;
    const uint2 w0 = a.hl[wi], w1 = a.hl[wi + 1];
    sh = funnel(w1.x, w0.x, shft) & kMask23;
    sl = funnel(w1.y, w0.y, shft) & kMask23;
    if (rev) {
        sh = revcomp_plane(sh);
        sl = revcomp_plane(sl);
    }
}

// is every word the window at shard-relative position rel touches inside the shard's (padded) planes?
__device__ __forceinline__ bool table_in_planes(const TableArgs &a, uint32_t rel) { return (uint64_t)(rel >> 5) + 1u < a.n_plane_words; }

}  // namespace

// kSource kTabHits: one thread per sorted hit (a.hits, a.n), the score as a double and / or as its fixed-point word.
// kTabScan / kTabSeed: the records where the search kernel left them, addressed as select_score_kernel addresses them - slot
// k * 256 + t of tile i is word i * kSumTile + k * 256 + t - every slot of every tile gets its word.  The 336 weights are read
// once per workgroup into LDS: the index of a weight differs per lane (position, read base, site base), which a constant-memory
// load would serialise.
template <int kSource> __global__ __launch_bounds__(kTabThreads) void table_score_kernel(const TableArgs a)
{
    __shared__ double s_w[kTableWeights];
    const uint32_t t = threadIdx.x;
    for (uint32_t i = t; i < kTableWeights; i += kTabThreads) s_w[i] = a.weights[i];
    block_sync();
    if constexpr (kSource == kTabHits) {
        const uint64_t i = (uint64_t)blockIdx.x * kTabThreads + t;
        if (i >= a.n) return;
        const vsc_hit h = a.hits[i];
        const uint32_t rel = a.contig_off[h.contig] + h.pos - a.first_pos;
        double x = 0.0;
        if (table_in_planes(a, rel) && h.guide < a.n_reads) {  // (every hit of the shard and the read set; others are not followed out of the arrays)
            uint32_t sh, sl;
            table_site(a, rel, VSC_HIT_STRAND(h.info) != 0, sh, sl);
            const uint2 g = a.guides[h.guide];
            x = table_score(s_w, g.x, g.y, sh, sl);
        }
        if (a.scores) a.scores[i] = x;
        if (a.fixed) a.fixed[i] = table_fixed(x);
    } else {
        constexpr bool kSeed = kSource == kTabSeed;
        const uint32_t tile_begin = blockIdx.x * (uint32_t)kTabTilesPerBlock, tile_end = min(tile_begin + (uint32_t)kTabTilesPerBlock, a.in.n_tiles);
        if (tile_begin >= tile_end) return;
        uint32_t seg = segment_of_tile(a.in.seg_tile0, a.in.n_segs, tile_begin);
        for (uint32_t tile = tile_begin; tile < tile_end; ++tile) {
            while (tile >= a.in.seg_tile0[seg + 1]) ++seg;
            const SumSeg sg = a.in.segs[seg];
            const uint32_t first = (tile - a.in.seg_tile0[seg]) * (uint32_t)kSumTile;
#pragma unroll 2
            for (int k = 0; k < kSumItems; ++k) {
                const uint32_t slot = (uint32_t)k * kTabThreads + t, i = first + slot;
                uint32_t f = kSelDropped, read, mask;
                uint64_t locus;
                if (i < sg.n && sink_decode<kSeed>(a.in, sg, sg.in_off + i, read, locus, mask) && read < a.n_reads &&
                    !(a.in.excl && a.in.excl[read] == locus)) {
                    const uint32_t rel = (uint32_t)locus - a.first_pos;
                    if (table_in_planes(a, rel)) {
                        uint32_t sh, sl;
                        table_site(a, rel, (locus >> 32) != 0, sh, sl);
                        const uint2 g = a.guides[read];
                        f = table_fixed(table_score(s_w, g.x, g.y, sh, sl));
                    }
                }
                a.slot_fixed[(uint64_t)tile * kSumTile + slot] = f;
            }
        }
    }
}

hipError_t launch_table_score(const TableArgs &args, hipStream_t stream)
{
    if (args.hits) {
        if (args.n == 0) return hipSuccess;
        hipLaunchKernelGGL(table_score_kernel<kTabHits>, dim3((uint32_t)((args.n + kTabThreads - 1) / kTabThreads)), dim3(kTabThreads), 0, stream, args);
        return hipGetLastError();
    }
    if (args.in.n_tiles == 0) return hipSuccess;
    const dim3 grid((args.in.n_tiles + kTabTilesPerBlock - 1) / kTabTilesPerBlock);
    if (args.in.vals) hipLaunchKernelGGL(table_score_kernel<kTabScan>, grid, dim3(kTabThreads), 0, stream, args);
    else hipLaunchKernelGGL(table_score_kernel<kTabSeed>, grid, dim3(kTabThreads), 0, stream, args);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// per-guide table summary (vsc_search_summary_table): score_sum, positive, positive_nm[0..8]; TableSummaryArgs
// ------------------------------------------------------------------------------------------------
// votes_summary_kernel's scheme over the fixed-point words: every lane takes kSumItems CONSECUTIVE record slots - 32 bytes of
// words, and of the 64 bytes of records only those that are counted hits, for the read and the mismatch mask - and keeps one
// running accumulator for the read it is on, flushed when the read changes and at the end of the tile: into the region's LDS
// table (SEED), which goes out with one agent-scope atomic per nonzero cell, or straight into the result (SCAN: the reads
// arrive mixed).  A lane's sum of kSumItems words of at most 2^30 needs 33 bits: a 64-bit accumulator.
template <bool kSeed> __global__ __launch_bounds__(kSumThreads) void table_summary_kernel(const TableSummaryArgs a)
{
    static_assert(kSumCounts == 1 + VSC_MAX_MISMATCHES + 1 + 1 && kSumWords == kSumCounts + 1, "vsc_guide_table_row: score_sum + positive, positive_nm[9], reserved");
    __shared__ unsigned long long s_sum[kSeed ? kRegionReads : 1];
    __shared__ uint32_t s_cnt[(kSeed ? kRegionReads : 1) * kSumCounts];  // (SCAN: unused, one row - as in summary_kernel)
    const uint32_t t = threadIdx.x;
    if (kSeed) sink_table_zero<kSumThreads>(s_sum, s_cnt, t);
    const uint32_t tile_begin = blockIdx.x * kSumTilesPerBlock, tile_end = min(tile_begin + (uint32_t)kSumTilesPerBlock, a.n_tiles);
    if (tile_begin >= tile_end) return;
    uint32_t seg = segment_of_tile(a.seg_tile0, a.n_segs, tile_begin);
    for (uint32_t tile = tile_begin; tile < tile_end; ++tile) {
        if (tile >= a.seg_tile0[seg + 1]) {
            if (kSeed) sink_table_flush<kSumThreads>(s_sum, s_cnt, t, a.segs[seg], a.out);
            while (tile >= a.seg_tile0[seg + 1]) ++seg;
        }
        const SumSeg sg = a.segs[seg];
        const uint32_t slot0 = t * (uint32_t)kSumItems;  // this lane's slots of the tile
        const uint32_t first = (tile - a.seg_tile0[seg]) * (uint32_t)kSumTile + slot0;
        uint32_t cur = ~0u, pos = 0;
        unsigned long long fsum = 0;
        uint64_t nm = 0;
        // the accumulator into a row: its sum word and the counters behind it (an LDS row, SEED; a result row, SCAN)
        auto flush_row = [&](unsigned long long *sum, auto *counts) {
            using T = std::remove_pointer_t<decltype(counts)>;
            if (fsum) atomicAdd(sum, fsum);
            if (pos) atomicAdd(&counts[0], (T)pos);
            sink_add_counts(&counts[1], nm);
        };
        auto flush = [&]() {
            if (cur == ~0u) return;
            if constexpr (kSeed) flush_row(&s_sum[cur - sg.first_read], &s_cnt[(cur - sg.first_read) * kSumCounts]);
            else flush_row(&a.out[(size_t)cur * kSumWords], &a.out[(size_t)cur * kSumWords + 1]);
            fsum = 0;
            pos = 0;
            nm = 0;
        };
        for (int k = 0; k < kSumItems; ++k) {
            if (first + (uint32_t)k >= sg.n) break;
            const uint32_t f = a.fixed[(uint64_t)tile * kSumTile + slot0 + (uint32_t)k];
            if (f == kSelDropped || f == 0u) continue;  // no counted hit, or one that adds to no field: the record is not read
            uint32_t read, mask;
            uint64_t locus;
            if (!sink_decode<kSeed>(a, sg, sg.in_off + first + (uint32_t)k, read, locus, mask) || read >= a.n_reads) continue;
            if (read != cur) {
                flush();
                cur = read;
            }
            fsum += f;
            pos += 1u;
            nm += 1ull << (kSumCountBits * __popc(mask));
        }
        flush();
    }
    if (kSeed) sink_table_flush<kSumThreads>(s_sum, s_cnt, t, a.segs[seg], a.out);
}

hipError_t launch_table_summary(const TableSummaryArgs &args, hipStream_t stream)
{
    if (args.n_tiles == 0) return hipSuccess;
    void (*const kernel)(TableSummaryArgs) = args.vals ? table_summary_kernel<false> : table_summary_kernel<true>;
    hipLaunchKernelGGL(kernel, dim3((args.n_tiles + kSumTilesPerBlock - 1) / kSumTilesPerBlock), dim3(kSumThreads), 0, stream, args);
    return hipGetLastError();
}

}  // namespace vsc
