// vsc_bulge.hip - the bulge-tolerant search (vsc_search_bulges): every site of 21, 22, 24 or 25 bases of the
// resident planes that ends in a PAM of the set, holds no N and pairs with a read within the budget when one or two bases
// of the site (DNA bulge) or of the read (RNA bulge) stay unpaired, as vsc_bulge_hit records in ascending (read, strand,
// contig, pos, d) order and / or as per-read rows of counts by (class, NM).
//
// The front end is enum_kernel's (vsc_enum.hip): a tile of 2 048 site starts per wave step, one 32-start word of each plane
// per lane plus its right neighbour - a site of 25 bases that starts at bit 31 ends at bit 55 of the pair.  Per strand and
// class one start mask: the PAM at the site's 3' end AND no N in its 23 + d bases, 32 starts per instruction.
//
// The back end is count, scan, write, as vsc_enum.hip's, with one count per CELL (read of the round, strand, tile):
//   bulge_count_kernel  every candidate of a tile against every read of the round: two mismatch masks (paired from the 5'
//                       end, paired from the PAM end), a popcount bound that rejects nearly every pair, bulge_align
//                       (vsc_bulge.h) for the rest.  Hits are counted per cell in LDS; the wave stores the tile's cells.
//   bulge_chunk_sum_kernel + enum_scan_kernel (vsc_enum.hip)  the cells' counts to offsets, per 64 cells.
//   bulge_write_kernel  the same masks again; only the (tile, read) pairs whose cells are not empty are walked a second time,
//                       in the lane's start order, d ascending at one start, and every hit goes to  chunk offset + cells
//                       before it in the chunk + wave prefix over the lanes + rank in the lane.  The rows come from this
//                       pass: per (wave, tile, read) the hits are added in LDS and each nonzero (class, NM) word goes out
//                       with one atomic.
// No record is placed through an atomic and nothing is sorted: the bytes depend on the planes and the parameters only.
#include "vsc_internal.h"
#include "vsc_cells_device.h"
#include "vsc_device.h"
#include "vsc_enum.h"
#include "vsc_bulge.h"

namespace vsc {

static_assert(kBulgeChunk == kCellChunk, "cell_offset takes one load per lane");

namespace {

// The lane's share of a tile: its word and the right neighbour of both planes, and per class k (d ascending) the starts
// b = 0..31 at which the site c[p, p + 23 + d) is a candidate on '+' (mf) and on '-' (mr).
struct BulgeTile {
    uint32_t H0, H1, L0, L1;
    uint32_t mf[kBulgeClasses], mr[kBulgeClasses];
    uint32_t base_pos;
};

__device__ __forceinline__ void bulge_front(const BulgeArgs &a, uint32_t tile, uint32_t lane, BulgeTile &t)
{
    const size_t wi = (size_t)tile * kTileWords + lane;  // (< n_tiles * 64, and the planes are padded by kPadWords)
    t.H0 = a.hi[wi];
    t.H1 = a.hi[wi + 1];
    t.L0 = a.lo[wi];
    t.L1 = a.lo[wi + 1];
    const uint32_t N0 = a.nm[wi], N1 = a.nm[wi + 1];
    uint64_t nn = ((uint64_t)N1 << 32) | N0;
    nn |= nn >> 1;
    nn |= nn >> 2;
    nn |= nn >> 4;
    nn |= nn >> 8;  // bit i covers positions i .. i+15
    // '-': s[L-2..L) = comp(c[p+1]) comp(c[p]) whatever L is
    const uint32_t Hs1 = funnel(t.H1, t.H0, 1), Ls1 = funnel(t.L1, t.L0, 1);
    uint32_t vr = 0;
    for (uint32_t i = 0; i < a.n_pam; ++i) {
        const PamMasks p = a.pam[i];
        vr |= (t.H0 ^ p.bh) & (t.L0 ^ p.bl) & (Hs1 ^ p.ah) & (Ls1 ^ p.al);
    }
#pragma unroll
    for (uint32_t k = 0; k < kBulgeClasses; ++k) {
        const int d = bulge_d_of_class(k);
        const bool on = d < 0 ? (uint32_t)-d <= a.rna_max : (uint32_t)d <= a.dna_max;  // wave-uniform
        const uint32_t len = (uint32_t)(VSC_READ_LEN + d);
        const uint32_t clean = on ? ~(uint32_t)(nn | nn >> (len - 16u)) : 0u;  // no N in positions i .. i+len-1
        // '+': s[L-2] = c[p + 21 + d], s[L-1] = c[p + 22 + d]
        const uint32_t Ha = funnel(t.H1, t.H0, len - 2u), La = funnel(t.L1, t.L0, len - 2u);
        const uint32_t Hb = funnel(t.H1, t.H0, len - 1u), Lb = funnel(t.L1, t.L0, len - 1u);
        uint32_t vf = 0;
        for (uint32_t i = 0; i < a.n_pam; ++i) {
            const PamMasks p = a.pam[i];
            vf |= ~(Ha ^ p.ah) & ~(La ^ p.al) & ~(Hb ^ p.bh) & ~(Lb ^ p.bl);
        }
        t.mf[k] = vf & clean;
        t.mr[k] = vr & clean;
    }
    t.base_pos = a.first_pos + tile * (uint32_t)kTileBases + lane * 32u;
}

// bit k: start b is a '+' candidate of class k; bit 4 + k: a '-' candidate
__device__ __forceinline__ uint32_t bulge_classes_at(const BulgeTile &t, uint32_t b)
{
    uint32_t c = 0;
#pragma unroll
    for (uint32_t k = 0; k < kBulgeClasses; ++k) c |= ((t.mf[k] >> b) & 1u) << k | ((t.mr[k] >> b) & 1u) << (4u + k);
    return c;
}

__device__ __forceinline__ uint32_t bulge_any(const BulgeTile &t)
{
    uint32_t any = 0;
#pragma unroll
    for (uint32_t k = 0; k < kBulgeClasses; ++k) any |= t.mf[k] | t.mr[k];
    return any;
}

// The site of 23 + d bases that starts at bit b of the lane's word, in read orientation: bit j = s[j].  On '-' the bit
// order is reversed and both planes are complemented, which puts the PAM at the top of the 23 + d bits on either strand.
__device__ __forceinline__ void bulge_site(const BulgeTile &t, uint32_t b, uint32_t rev, int d, uint32_t *sh, uint32_t *sl)
{
    const uint32_t len = (uint32_t)(VSC_READ_LEN + d);
    const uint32_t keep = (1u << len) - 1u;
    const uint32_t wh = funnel(t.H1, t.H0, b) & keep, wl = funnel(t.L1, t.L0, b) & keep;
    *sh = rev ? (~__brev(wh)) >> (32u - len) : wh;
    *sl = rev ? (~__brev(wl)) >> (32u - len) : wl;
}

}  // namespace

// ---- count pass --------------------------------------------------------------------------------------------------------
// Each lane walks its candidates one per step - start ascending, the classes of both strands at one start - so that the
// lanes of a wave stay busy as long as the fullest lane has candidates; the reads are the inner loop, fetched through the
// constant address space (scalar loads, as scan_kernel's).
__global__ __launch_bounds__(kWave *kWavesPerGroup) void bulge_count_kernel(const BulgeArgs a)
{
    __shared__ uint32_t s_cnt[kWavesPerGroup][2 * kBulgeMaxBatch];
    const uint32_t lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    uint32_t *cnt = s_cnt[wave];
    for (uint32_t i = lane; i < 2 * kBulgeMaxBatch; i += kWave) cnt[i] = 0;
    wave_sync();
    uint32_t t0, t1;
    cell_tile_run(a.n_tiles, blockIdx.x * kWavesPerGroup + wave, gridDim.x * kWavesPerGroup, &t0, &t1);
    const const_v4u_ptr gp = (const_v4u_ptr)(uintptr_t)a.guides;
    const uint32_t m = a.max_mm;
    unsigned long long sites = 0;
    for (uint32_t tile = t0; tile < t1; ++tile) {
        BulgeTile t;
        bulge_front(a, tile, lane, t);
        uint32_t any = bulge_any(t);
        uint32_t cur = 0, b = 0;
        for (;;) {
            if (cur == 0 && any != 0) {
                b = (uint32_t)__builtin_ctz(any);
                any &= any - 1u;
                cur = bulge_classes_at(t, b);
            }
            const bool has = cur != 0;
            const uint64_t act = __ballot(has);
            if (act == 0) break;
            sites += (uint32_t)__popcll(act);
            const uint32_t c = has ? (uint32_t)__builtin_ctz(cur) : 0u;
            cur &= cur - 1u;
            const uint32_t rev = c >> 2;
            const int d = bulge_d_of_class(c & 3u);
            const uint32_t gap = d < 0 ? (uint32_t)-d : 0u;
            uint32_t sh, sl;
            bulge_site(t, b, rev, d, &sh, &sl);
            const uint32_t th = d > 0 ? sh >> d : sh << -d, tl = d > 0 ? sl >> d : sl << -d;
            const uint32_t live = d > 0 ? kMask23 : kMask23 & ~((1u << -d) - 1u);
            const uint32_t limit = m + gap;
            // four reads per step, the next four fetched while these are compared (the table ends with four spare reads); one
            // ballot over the four bounds: the walk is the rare path
            v4u na = gp[0], nb = gp[1];
            for (uint32_t g = 0; g < a.n_guides; g += kBulgeUnroll) {
                const v4u ga = na, gb = nb;
                na = gp[(g >> 1) + 2];
                nb = gp[(g >> 1) + 3];
                const uint32_t rh[kBulgeUnroll] = {ga.x, ga.z, gb.x, gb.z};
                const uint32_t rl[kBulgeUnroll] = {ga.y, ga.w, gb.y, gb.w};
                uint32_t x0[kBulgeUnroll], x1[kBulgeUnroll], low = 32;
#pragma unroll
                for (uint32_t u = 0; u < kBulgeUnroll; ++u) {
                    x0[u] = (rh[u] ^ sh) | (rl[u] ^ sl);
                    x1[u] = ((rh[u] ^ th) | (rl[u] ^ tl)) & live;
                    low = min(low, (uint32_t)__popc(bulge_bound_mask(x0[u], x1[u])));
                }
                if (__ballot(has && low <= limit) == 0) continue;
#pragma unroll
                for (uint32_t u = 0; u < kBulgeUnroll; ++u) {
                    // (g + u < n_guides: the reads that pad the last four are all A and count for nothing)
                    if (g + u < a.n_guides && has && (uint32_t)__popc(bulge_bound_mask(x0[u], x1[u])) <= limit) {
                        uint32_t index;
                        if (bulge_walk(x0[u] & kMask23, x1[u], d, &index) <= m) atomicAdd(&cnt[2u * (g + u) + rev], 1u);
                    }
                }
            }
        }
        // the tile's cells: (read, strand) l of the round -> count[l * n_tiles + tile]
        wave_sync();
        for (uint32_t l = lane; l < 2u * a.n_guides; l += kWave) {
            a.count[(size_t)l * a.n_tiles + tile] = cnt[l];
            cnt[l] = 0;
        }
        wave_sync();
    }
    if (lane == 0 && sites) atomicAdd(a.sites, sites);
}

// chunk_sum[c] = the hits of cells 64 c .. 64 c + 63: one wave per chunk, one cell per lane
__global__ __launch_bounds__(kWave *kWavesPerGroup) void bulge_chunk_sum_kernel(const uint32_t *count, unsigned long long n, uint32_t n_chunks,
                                                                               uint32_t *chunk_sum)
{
    const uint32_t lane = threadIdx.x % kWave;
    const uint32_t chunk = blockIdx.x * kWavesPerGroup + threadIdx.x / kWave;
    if (chunk >= n_chunks) return;
    const unsigned long long i = (unsigned long long)chunk * kBulgeChunk + lane;
    const uint32_t s = wave_sum(i < n ? count[i] : 0u);
    if (lane == 0) chunk_sum[chunk] = s;
}

// ---- write pass --------------------------------------------------------------------------------------------------------
namespace {

// The lane's hits of read (rh, rl) in the tile, in record order of each strand: start ascending, d ascending.
// kEmit = false: counts them per strand into nf / nr and, with rows, adds them into the wave's LDS row.
// kEmit = true: writes them from at_f / at_r on.
template <bool kEmit>
__device__ __forceinline__ void bulge_walk_lane(const BulgeArgs &a, const BulgeTile &t, uint32_t rh, uint32_t rl, uint32_t guide, uint32_t *row,
                                                uint32_t &nf, uint32_t &nr, unsigned long long at_f, unsigned long long at_r)
{
    uint32_t c_id = 0, c_end = 0;  // the contig of the lane's last hit: [.., c_end) in global positions
    for (uint32_t any = bulge_any(t); any; any &= any - 1u) {
        const uint32_t b = (uint32_t)__builtin_ctz(any);
        // bits 0..3 the '+' classes, 4..7 the '-' classes: ascending bits = d ascending inside either strand
        for (uint32_t here = bulge_classes_at(t, b); here; here &= here - 1u) {
            const uint32_t c = (uint32_t)__builtin_ctz(here), k = c & 3u, rev = c >> 2;
            const int d = bulge_d_of_class(k);
            const uint32_t gap = d < 0 ? (uint32_t)-d : 0u;
            uint32_t sh, sl, x0, x1, index;
            bulge_site(t, b, rev, d, &sh, &sl);
            bulge_masks(rh, rl, sh, sl, d, &x0, &x1);
            if ((uint32_t)__popc(bulge_bound_mask(x0, x1)) > a.max_mm + gap) continue;
            const uint32_t nm = bulge_walk(x0, x1, d, &index);
            if (nm > a.max_mm) continue;
            if (!kEmit) {
                if (rev) ++nr; else ++nf;
                if (row) atomicAdd(&row[k * (VSC_MAX_MISMATCHES + 1) + nm], 1u);
            } else {
                const uint32_t pos = t.base_pos + b;
                if (pos >= c_end) {  // the last contig that starts at or before pos (an N-free site lies inside one contig)
                    uint32_t lo = 0, hi = a.n_contigs;
                    while (lo < hi) {
                        const uint32_t mid = (lo + hi) >> 1;
                        if (a.contig_off[mid] <= pos) lo = mid + 1; else hi = mid;
                    }
                    c_id = lo ? lo - 1u : 0u;
                    c_end = a.contig_end[c_id];
                }
                const uint4 rec = make_uint4(guide, c_id, pos - a.contig_off[c_id], bulge_info(rev, d, index, nm));
                // (at < n_records whenever both passes see the same planes: the test keeps a write inside the result if not)
                unsigned long long &at = rev ? at_r : at_f;
                if (at < a.n_records) a.records[at] = rec;
                ++at;
            }
        }
    }
}

}  // namespace

__global__ __launch_bounds__(kWave *kWavesPerGroup) void bulge_write_kernel(const BulgeArgs a)
{
    __shared__ uint32_t s_row[kWavesPerGroup][kWave];  // kBulgeRowWords = 36 in use
    const uint32_t lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    uint32_t *row = a.rows ? s_row[wave] : nullptr;
    s_row[wave][lane] = 0;
    wave_sync();
    uint32_t t0, t1;
    cell_tile_run(a.n_tiles, blockIdx.x * kWavesPerGroup + wave, gridDim.x * kWavesPerGroup, &t0, &t1);
    const const_v4u_ptr gp = (const_v4u_ptr)(uintptr_t)a.guides;
    for (uint32_t tile = t0; tile < t1; ++tile) {
        // which reads of the round have a hit in this tile: lane l looks at cell l (read l / 2, strand l & 1)
        // (kBulgeMaxBatch = 64 reads: two words of 64 cells)
        const uint32_t n_cells = 2u * a.n_guides;
        const uint64_t live = __ballot(lane < n_cells && a.count[(size_t)lane * a.n_tiles + tile] != 0);
        uint64_t live_hi = 0;
        if (n_cells > (uint32_t)kWave) live_hi = __ballot(kWave + lane < n_cells && a.count[(size_t)(kWave + lane) * a.n_tiles + tile] != 0);
        if ((live | live_hi) == 0) continue;
        BulgeTile t;
        bulge_front(a, tile, lane, t);
        for (uint32_t g = 0; g < a.n_guides; ++g) {
            const uint64_t word = g < 32u ? live : live_hi;
            if (((word >> (2u * (g & 31u))) & 3u) == 0) continue;  // wave-uniform
            const v4u gg = gp[g >> 1];
            const uint32_t rh = (g & 1u) ? gg.z : gg.x, rl = (g & 1u) ? gg.w : gg.y;
            uint32_t nf = 0, nr = 0;
            bulge_walk_lane<false>(a, t, rh, rl, a.guide_base + g, row, nf, nr, 0, 0);
            if (row) {
                wave_sync();
                const uint32_t v = row[lane];
                if (lane < kBulgeRowWords && v) atomicAdd(&a.rows[(size_t)(a.guide_base + g) * kBulgeRowWords + lane], v);
                row[lane] = 0;
                wave_sync();
            }
            if (a.records) {
                const unsigned long long cell = (unsigned long long)(2u * g) * a.n_tiles + tile;
                const unsigned long long at_f = cell_offset(a.count, a.chunk_off, cell, lane) + wave_exclusive(nf, lane);
                const unsigned long long at_r = cell_offset(a.count, a.chunk_off, cell + a.n_tiles, lane) + wave_exclusive(nr, lane);
                bulge_walk_lane<true>(a, t, rh, rl, a.guide_base + g, nullptr, nf, nr, at_f, at_r);
            }
        }
    }
}

// ---- launches ----------------------------------------------------------------------------------------------------------
hipError_t launch_bulge_count(const BulgeArgs &args, int n_cus, hipStream_t stream)
{
    if (args.n_tiles == 0 || args.n_guides == 0) return hipSuccess;
    hipLaunchKernelGGL(bulge_count_kernel, cell_grid(args.n_tiles, n_cus), dim3(kWave * kWavesPerGroup), 0, stream, args);
    return hipGetLastError();
}

hipError_t launch_bulge_write(const BulgeArgs &args, int n_cus, hipStream_t stream)
{
    if (args.n_tiles == 0 || args.n_guides == 0) return hipSuccess;
    hipLaunchKernelGGL(bulge_write_kernel, cell_grid(args.n_tiles, n_cus), dim3(kWave * kWavesPerGroup), 0, stream, args);
    return hipGetLastError();
}

hipError_t launch_bulge_chunk_sums(const uint32_t *count, uint64_t n, uint32_t *chunk_sum, hipStream_t stream)
{
    const uint32_t n_chunks = (uint32_t)((n + kBulgeChunk - 1) / kBulgeChunk);
    if (n_chunks == 0) return hipSuccess;
    hipLaunchKernelGGL(bulge_chunk_sum_kernel, dim3((n_chunks + kWavesPerGroup - 1) / kWavesPerGroup), dim3(kWave * kWavesPerGroup), 0, stream,
                       count, (unsigned long long)n, n_chunks, chunk_sum);
    return hipGetLastError();
}

}  // namespace vsc
