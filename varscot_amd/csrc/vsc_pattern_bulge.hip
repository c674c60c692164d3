// vsc_pattern_bulge.hip - bulges under a pattern (vsc_search_pattern_bulges): every site of L + d bases, d in
// -rna_max .. -1 and 1 .. dna_max, of the resident planes that satisfies the bulged pattern P[0..a) + N x (n + d) + P[e..L),
// holds no N and pairs with an IUPAC guide within the budget when d bases of the site (DNA bulge) or -d positions of the guide
// (RNA bulge) inside the protospacer [a, e) stay unpaired - as vsc_bulge_hit records in ascending (guide, strand, contig, pos,
// d) order and / or as per-guide rows of counts by (class, NM).
//
// The front end is the pattern search's (pattern_starts, vsc_pattern_device.h), run once per enabled class and strand with
// that class's table over L + d positions: up to 4 x 2 start masks per lane and tile.
//
// The candidate walk is the pattern search's LDS queue, not the lane walk of vsc_bulge.hip: per strand the (start, class)
// pairs of the tile get their rank in ascending (start, d) order - lanes in front + order in the lane - and go through the
// wave's queue in windows of 2 048 ranks (an all-N pattern with four classes has 8 192 per strand and tile; a PAM leaves one
// window).  Every step takes kPatSlots x 64 queued sites, all lanes busy, against the round's guides; a '-' site is turned into
// read orientation once, when it leaves the queue, so that one table of guides serves both strands and the split point is
// the definition's.  Per (site, guide): the two pairings and the popcount bound of vsc_pattern_bulge.h; only the pairs inside
// the bound take the walk over the split points.  The guides' planes come through the constant address space (scalar loads),
// four guides per load, the next four fetched while these are compared.
//
// The back end is count, scan, write, exactly as vsc_pattern.hip's, with one count per CELL (guide of the round, strand, tile);
// bulge_chunk_sum_kernel (twice) and enum_scan_kernel turn the counts into offsets.  The rows come from the write pass.
// No record is placed through an atomic and nothing is sorted: the bytes depend on the planes and the parameters only.
#include "vsc_internal.h"
#include "vsc_device.h"
#include "vsc_pattern_device.h"
#include "vsc_pattern_bulge.h"

namespace vsc {

static_assert(kPatChunk == kCellChunk, "cell_offset takes one load per lane");

namespace {

constexpr uint32_t kPbRowWords = kBulgeRowWords;  // 36 of the 64 words of PbLds::row

// The wave's LDS: the tile's words of both planes (65 each: the last lane's right neighbour), the queue of one window and the
// row of one cell.  4 880 bytes per wave, 19 520 per workgroup of four.
struct PbLds {
    uint32_t h[kTileWords + 2], l[kTileWords + 2];
    uint16_t q[kPatBulgeQueue];  // class << 11 | lane << 5 | bit, ascending (start, class)
    uint32_t row[kWave];         // write pass: the cell's hits by (class, NM)
};

// The tile's words into LDS and the start masks m[strand][class] of the lane's 32 starts (0 for a class that is not enabled).
__device__ __forceinline__ void pb_tile(const PatBulgeArgs &a, uint32_t tile, uint32_t lane, PbLds &s, uint32_t (&m)[2][kBulgeClasses])
{
    const size_t wi = (size_t)tile * kTileWords + lane;  // (< n_tiles * 64, and the planes are padded by kPadWords)
    const uint32_t H0 = a.hi[wi], H1 = a.hi[wi + 1];
    const uint32_t L0 = a.lo[wi], L1 = a.lo[wi + 1];
    const uint32_t N0 = a.nm[wi], N1 = a.nm[wi + 1];
    uint64_t nn = ((uint64_t)N1 << 32) | N0;
    nn |= nn >> 1;
    nn |= nn >> 2;
    nn |= nn >> 4;
    nn |= nn >> 8;  // bit i covers positions i .. i+15
#pragma unroll
    for (uint32_t k = 0; k < kBulgeClasses; ++k) {
        m[0][k] = m[1][k] = 0;
        if (((a.classes >> k) & 1u) == 0) continue;  // wave-uniform
        const uint32_t len = (uint32_t)((int)a.len + bulge_d_of_class(k));  // 16 .. 32
        const uint32_t clean = ~(uint32_t)(nn | nn >> (len - kPatMinLen));  // no N in positions i .. i+len-1
        m[0][k] = pattern_starts(a.front[k][0], H0, H1, L0, L1) & clean;
        m[1][k] = pattern_starts(a.front[k][1], H0, H1, L0, L1) & clean;
    }
    s.h[lane] = H0;
    s.l[lane] = L0;
    if (lane == kWave - 1) {
        s.h[kWave] = H1;
        s.l[kWave] = L1;
    }
}

__device__ __forceinline__ uint32_t pb_lane_count(const uint32_t (&m)[kBulgeClasses])
{
    return (uint32_t)__popc(m[0]) + (uint32_t)__popc(m[1]) + (uint32_t)__popc(m[2]) + (uint32_t)__popc(m[3]);
}

// The lane's (start, class) pairs whose rank lies in the window [win0, win0 + 2 048) into the queue; `before` = the rank of
// its first pair (start ascending, d ascending at one start).  The hand-offs before (the queue's last readers) and after are
// the caller's.
__device__ __forceinline__ void pb_enqueue(PbLds &s, const uint32_t (&m)[kBulgeClasses], uint32_t before, uint32_t win0, uint32_t lane)
{
    uint32_t at = before - win0;  // (wraps below the window: such a slot is >= 2 048 and is skipped)
    for (uint32_t r = m[0] | m[1] | m[2] | m[3]; r; r &= r - 1u) {
        const uint32_t b = (uint32_t)__builtin_ctz(r);
#pragma unroll
        for (uint32_t k = 0; k < kBulgeClasses; ++k) {
            if ((m[k] >> b) & 1u) {
                if (at < kPatBulgeQueue) s.q[at] = (uint16_t)(k << 11 | lane << 5 | b);
                ++at;
            }
        }
    }
}

// A queued site in read orientation: planes (sh, sl) of its L + d bases, bit j = s[j], the bits from L + d on zero.
struct PbSite {
    uint32_t sh, sl;
    int d;
};

__device__ __forceinline__ PbSite pb_site(const PbLds &s, uint32_t e, uint32_t strand, uint32_t L)
{
    const uint32_t src = (e >> 5) & 63u, b = e & 31u;  // (src + 1 <= 64 is the last lane's right neighbour)
    PbSite v;
    v.d = bulge_d_of_class((e >> 11) & 3u);
    const uint32_t len = (uint32_t)((int)L + v.d);  // 16 .. 32
    const uint32_t wh = funnel(s.h[src + 1], s.h[src], b), wl = funnel(s.l[src + 1], s.l[src], b);
    // '-': the reverse complement - bit j to len - 1 - j, both planes inverted
    v.sh = strand ? (~__brev(wh)) >> (32u - len) : wh & low_bits(len);
    v.sl = strand ? (~__brev(wl)) >> (32u - len) : wl & low_bits(len);
    return v;
}

// what of the arguments a pair needs, in scalar registers
struct PbConst {
    uint32_t L, a, e, m, fixed5, fixed3;
};

__device__ __forceinline__ PbConst pb_const(const PatBulgeArgs &a)
{
    return PbConst{a.len, a.proto_a, a.proto_e, a.max_mm, pattern_bulge_fixed5(a.proto_a), pattern_bulge_fixed3(a.proto_e, a.len)};
}

// One step of the count pass: kSlots x 64 queued sites from `base` on against every guide of the round; lane g adds the hits
// of guide g to cnt.  An instance per number of slots, as pattern_count_step.
template <uint32_t kSlots>
__device__ __forceinline__ void pb_count_step(const PbLds &s, const_v16u_ptr gq, uint32_t n_guides, const PbConst &c, uint32_t strand,
                                              uint32_t base, uint32_t total, uint32_t lane, uint32_t &cnt)
{
    PbSite site[kSlots];
    uint32_t limit[kSlots], dead[kSlots];
#pragma unroll
    for (uint32_t j = 0; j < kSlots; ++j) {
        const uint32_t idx = base + j * kWave + lane;
        const bool live = idx < total;
        site[j] = pb_site(s, live ? s.q[idx] : 0u, strand, c.L);
        limit[j] = c.m + (site[j].d < 0 ? (uint32_t)-site[j].d : 0u);
        dead[j] = live ? 0u : 64u;  // added to the popcount (v_bcnt's own addend): an empty slot is outside every bound
    }
    // four guides per scalar load (64 bytes), the next four fetched while these are compared; the table ends with four spare
    v16u next = gq[0];
    for (uint32_t g = 0; g < n_guides; g += kPatUnroll) {
        const v16u cur = next;
        next = gq[g / kPatUnroll + 1u];
#pragma unroll
        for (uint32_t u = 0; u < kPatUnroll; ++u) {
            const PatPlanes planes{cur[4 * u], cur[4 * u + 1], cur[4 * u + 2], cur[4 * u + 3]};
            uint32_t hits = 0;
#pragma unroll
            for (uint32_t j = 0; j < kSlots; ++j) {
                uint32_t x0, x1;
                pattern_bulge_masks(site[j].sh, site[j].sl, planes, site[j].d, &x0, &x1);
                const bool in = (uint32_t)__popc(pattern_bulge_bound_mask(x0, x1, c.fixed5, c.fixed3)) + dead[j] <= limit[j];
                if (__ballot(in) != 0) {  // the walk is the rare path
                    uint32_t index;
                    const bool hit = in && pattern_bulge_walk(x0, x1, c.a, c.e, site[j].d, &index) <= c.m;
                    hits += (uint32_t)__popcll(__ballot(hit));
                }
            }
            if (lane == g + u) cnt += hits;  // (a guide that pads the last four is all zero: it allows nothing and is outside the bound)
        }
    }
}

}  // namespace

// ---- count pass --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kWave *kWavesPerGroup) void pattern_bulge_count_kernel(const PatBulgeArgs a)
{
    __shared__ PbLds s_lds[kWavesPerGroup];
    const uint32_t lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    PbLds &s = s_lds[wave];
    uint32_t t0, t1;
    cell_tile_run(a.n_tiles, blockIdx.x * kWavesPerGroup + wave, gridDim.x * kWavesPerGroup, &t0, &t1);
    const PbConst c = pb_const(a);
    const const_v16u_ptr gq = (const_v16u_ptr)(uintptr_t)a.guides;
    unsigned long long sites = 0;
    for (uint32_t tile = t0; tile < t1; ++tile) {
        uint32_t mask[2][kBulgeClasses];
        wave_sync();  // (the last tile's readers of the planes and the queue are done)
        pb_tile(a, tile, lane, s, mask);
        uint32_t cnt[2] = {0, 0};  // lane g: the hits of guide g of the round, per strand
#pragma unroll
        for (uint32_t strand = 0; strand < 2; ++strand) {
            uint32_t all;
            const uint32_t before = wave_exclusive(pb_lane_count(mask[strand]), lane, &all);
            sites += all;
            for (uint32_t win0 = 0; win0 < all; win0 += kPatBulgeQueue) {
                wave_sync();  // (the steps of the window before have read the queue)
                pb_enqueue(s, mask[strand], before, win0, lane);
                wave_sync();
                const uint32_t total = all - win0 < kPatBulgeQueue ? all - win0 : kPatBulgeQueue;
                for (uint32_t base = 0; base < total; base += kPatSlots * kWave) {
                    const uint32_t left = (total - base + kWave - 1u) / kWave;  // wave-uniform: steps of 64 sites that are left
                    if (left >= 4u) pb_count_step<4>(s, gq, a.n_guides, c, strand, base, total, lane, cnt[strand]);
                    else if (left == 3u) pb_count_step<3>(s, gq, a.n_guides, c, strand, base, total, lane, cnt[strand]);
                    else if (left == 2u) pb_count_step<2>(s, gq, a.n_guides, c, strand, base, total, lane, cnt[strand]);
                    else pb_count_step<1>(s, gq, a.n_guides, c, strand, base, total, lane, cnt[strand]);
                }
            }
        }
        // the tile's cells: (guide, strand) of the round -> count[(2 g + strand) * n_tiles + tile]
        if (lane < a.n_guides) {
            a.count[(size_t)(2u * lane) * a.n_tiles + tile] = cnt[0];
            a.count[(size_t)(2u * lane + 1u) * a.n_tiles + tile] = cnt[1];
        }
    }
    if (lane == 0 && sites) atomicAdd(a.sites, sites);
}

// ---- write pass --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kWave *kWavesPerGroup) void pattern_bulge_write_kernel(const PatBulgeArgs a)
{
    __shared__ PbLds s_lds[kWavesPerGroup];
    const uint32_t lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    PbLds &s = s_lds[wave];
    s.row[lane] = 0;
    uint32_t t0, t1;
    cell_tile_run(a.n_tiles, blockIdx.x * kWavesPerGroup + wave, gridDim.x * kWavesPerGroup, &t0, &t1);
    const PbConst c = pb_const(a);
    const const_v4u_ptr gp = (const_v4u_ptr)(uintptr_t)a.guides;
    uint32_t c_id = 0, c_off = 1, c_end = 0;  // the contig of the lane's last hit: [c_off, c_end) in global positions (empty at first)
    for (uint32_t tile = t0; tile < t1; ++tile) {
        // which cells of the round have a hit in this tile: lane l looks at cell l (guide l / 2, strand l & 1), then at 64 + l
        const uint32_t n_cells = 2u * a.n_guides;
        const uint64_t live_lo = __ballot(lane < n_cells && a.count[(size_t)lane * a.n_tiles + tile] != 0);
        uint64_t live_hi = 0;
        if (n_cells > (uint32_t)kWave) live_hi = __ballot(kWave + lane < n_cells && a.count[(size_t)(kWave + lane) * a.n_tiles + tile] != 0);
        if ((live_lo | live_hi) == 0) continue;
        uint32_t mask[2][kBulgeClasses];
        wave_sync();  // (the last tile's readers of the planes and the queue are done)
        pb_tile(a, tile, lane, s, mask);
        const uint32_t tile_pos = a.first_pos + tile * (uint32_t)kTileBases;
#pragma unroll
        for (uint32_t strand = 0; strand < 2; ++strand) {
            const uint64_t odd = 0xAAAAAAAAAAAAAAAAull;
            const uint64_t sel = strand ? odd : odd >> 1;
            if (((live_lo | live_hi) & sel) == 0) continue;  // wave-uniform: no guide has a hit on this strand
            uint32_t all;
            const uint32_t before = wave_exclusive(pb_lane_count(mask[strand]), lane, &all);
            const bool windows = all > kPatBulgeQueue;  // more than one: every guide fills the queue again, window by window
            bool queued = false;
            for (uint32_t g = 0; g < a.n_guides; ++g) {
                const uint64_t word = g < 32u ? live_lo : live_hi;
                if (((word >> (2u * (g & 31u) + strand)) & 1u) == 0) continue;  // wave-uniform
                const v4u gg = gp[g];
                const PatPlanes planes{gg.x, gg.y, gg.z, gg.w};
                const unsigned long long cell = (unsigned long long)(2u * g + strand) * a.n_tiles + tile;
                unsigned long long at = a.records ? cell_offset(a.count, a.chunk_sum, a.group_off, cell, lane) : 0ull;
                for (uint32_t win0 = 0; win0 < all; win0 += kPatBulgeQueue) {
                    if (windows || !queued) {
                        wave_sync();  // (the queue's last readers are done)
                        pb_enqueue(s, mask[strand], before, win0, lane);
                        wave_sync();
                        queued = true;
                    }
                    const uint32_t total = all - win0 < kPatBulgeQueue ? all - win0 : kPatBulgeQueue;
                    for (uint32_t base = 0; base < total; base += kWave) {
                        const uint32_t idx = base + lane;
                        const bool live = idx < total;
                        const uint32_t e = live ? s.q[idx] : 0u;
                        const PbSite site = pb_site(s, e, strand, c.L);
                        uint32_t x0, x1, index = 0, nm = 0;
                        pattern_bulge_masks(site.sh, site.sl, planes, site.d, &x0, &x1);
                        const uint32_t gap = site.d < 0 ? (uint32_t)-site.d : 0u;
                        bool hit = live && (uint32_t)__popc(pattern_bulge_bound_mask(x0, x1, c.fixed5, c.fixed3)) <= c.m + gap;
                        if (hit) {
                            nm = pattern_bulge_walk(x0, x1, c.a, c.e, site.d, &index);
                            hit = nm <= c.m;
                        }
                        const uint64_t hits = __ballot(hit);
                        if (hits == 0) continue;
                        if (hit) {
                            if (a.rows) atomicAdd(&s.row[((e >> 11) & 3u) * (VSC_MAX_MISMATCHES + 1) + nm], 1u);  // (< 36: nm <= 8)
                            if (a.records) {
                                const uint32_t pos = tile_pos + (e & 2047u);  // (lane << 5 | bit = the start's offset in the tile)
                                if (pos >= c_end || pos < c_off) {  // the last contig that starts at or before pos (an N-free site lies inside one contig)
                                    uint32_t lo = 0, hi = a.n_contigs;
                                    while (lo < hi) {
                                        const uint32_t mid = (lo + hi) >> 1;
                                        if (a.contig_off[mid] <= pos) lo = mid + 1; else hi = mid;
                                    }
                                    c_id = lo ? lo - 1u : 0u;
                                    c_off = a.contig_off[c_id];
                                    c_end = a.contig_end[c_id];
                                }
                                const unsigned long long r = at + lanes_below(hits);
                                // (r < n_records whenever both passes see the same planes: the test keeps a write inside the result if not)
                                if (r < a.n_records)
                                    a.records[r] = make_uint4(a.guide_base + g, c_id, pos - c_off, bulge_info(strand, site.d, index, nm));
                            }
                        }
                        at += (uint32_t)__popcll(hits);
                    }
                }
                if (a.rows) {
                    wave_sync();
                    const uint32_t v = lane < kPbRowWords ? s.row[lane] : 0u;
                    if (v) {
                        atomicAdd(&a.rows[(size_t)(a.guide_base + g) * kPbRowWords + lane], v);
                        s.row[lane] = 0;
                    }
                    wave_sync();
                }
            }
        }
    }
}

// ---- launches ----------------------------------------------------------------------------------------------------------
hipError_t launch_pattern_bulge_count(const PatBulgeArgs &args, int n_cus, hipStream_t stream)
{
    if (args.n_tiles == 0 || args.n_guides == 0) return hipSuccess;
    hipLaunchKernelGGL(pattern_bulge_count_kernel, cell_grid(args.n_tiles, n_cus), dim3(kWave * kWavesPerGroup), 0, stream, args);
    return hipGetLastError();
}

hipError_t launch_pattern_bulge_write(const PatBulgeArgs &args, int n_cus, hipStream_t stream)
{
    if (args.n_tiles == 0 || args.n_guides == 0) return hipSuccess;
    hipLaunchKernelGGL(pattern_bulge_write_kernel, cell_grid(args.n_tiles, n_cus), dim3(kWave * kWavesPerGroup), 0, stream, args);
    return hipGetLastError();
}

}  // namespace vsc
