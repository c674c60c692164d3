// vsc_sites.hip - plain and bulged alignments collapsed into cut sites (vsc_hits_sites, vsc_pattern_hits_sites):
// a count / scan / write pass over two record lists that are sorted and resident already.  No search kernel, no sort, no
// append atomic: the bytes depend on the inputs only.
//
// Two kernels around enum_scan_kernel (vsc_enum.hip).  site_flag_kernel takes one alignment per lane: waves take runs of
// 64-record tiles of the plain list, then of the bulged list; the lane gathers its site (vsc_sites.h: a bounded walk in its own
// list, one lower bound in the other) and is flagged iff it is the best of it; the wave stores the tile's ballot and its
// popcount.  site_write_kernel gives every flagged lane its rank - the survivors in front of it in its own list (tile offset
// + ballot bits below the lane) plus the survivors of the other list with a smaller key (one lower bound, then that tile's
// offset + the ballot bits below the bound) - gathers the site again for the members word and writes the 32-byte record as two
// 16-byte stores.  The rows: per-wave LDS counters and one integer atomic per non-zero word where the tile holds one guide
// (all but the tiles at a guide's end), one atomic per word and lane where it holds several.
//
// Gathers bound by the latency of their dependent loads, as pair_join_kernel: 8 workgroups of 4 waves per CU, the last tile of
// either list partly idle.  Every index is checked against its list's length before it is used, every store against the
// scan's total.
#include "vsc_internal.h"
#include "vsc_cells_device.h"
#include "vsc_sites.h"

namespace vsc {

namespace {

__device__ __forceinline__ unsigned long long bits_below(uint32_t b) { return b ? ~0ull >> (64u - b) : 0ull; }

// survivors among records [0, j) of the list whose tiles start at tile `base` (j <= n: n itself takes the next list's offset)
__device__ __forceinline__ unsigned long long site_survivors_below(const SiteArgs &a, uint32_t base, uint32_t tiles, uint32_t n, uint32_t j)
{
    const unsigned long long first = a.tile_off[base];
    if (j >= n) return a.tile_off[base + tiles] - first;
    const uint32_t t = base + j / kSiteTile;
    return a.tile_off[t] - first + (unsigned long long)__popcll(a.ballot[t] & bits_below(j % kSiteTile));
}

}  // namespace

template <int kPlain>
__global__ __launch_bounds__(kWave *kWavesPerGroup) void site_flag_kernel(const SiteArgs a)
{
    const uint32_t lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    const uint32_t n_tiles = a.tiles_plain + a.tiles_bulged;
    uint32_t t0, t1;
    cell_tile_run(n_tiles, blockIdx.x * kWavesPerGroup + wave, gridDim.x * kWavesPerGroup, &t0, &t1);
    for (uint32_t tile = t0; tile < t1; ++tile) {
        const bool in_bulged = tile >= a.tiles_plain;  // wave-uniform
        const uint32_t n = in_bulged ? a.n_bulged : a.n_plain;
        const unsigned long long at = (unsigned long long)(tile - (in_bulged ? a.tiles_plain : 0u)) * kSiteTile + lane;
        const bool has = at < n;
        const uint32_t i = has ? (uint32_t)at : 0u;  // (a tile exists only where its list has a record: record 0 is there)
        const SiteAln x = in_bulged ? site_load<kSiteBulge>(a.bulged, i) : site_load<kPlain>(a.plain, i);
        const bool known = x.guide < a.n_guides;
        SiteView v{kSiteNoMembers, ~0u};
        if (has) v = site_gather<kPlain>(a.plain, a.n_plain, a.bulged, a.n_bulged, in_bulged, i, x, a.len, a.anchor);
        const unsigned long long best = __ballot(has && v.best == site_rank(x.d, x.nm));
        if (has && !known) *a.invalid = 1u;
        if (a.rows) {  // alignments: the tile's records by guide - one add where the tile holds one guide
            const uint32_t g0 = uniform(x.guide);  // lane 0 holds a record
            const uint32_t n_here = (uint32_t)__popcll(__ballot(has));
            if (__ballot(has && x.guide != g0) == 0) {
                if (lane == 0 && known) atomicAdd(&a.rows[(size_t)g0 * kSiteRowWords + kSiteRowAlignments], n_here);
            } else if (has && known) {
                atomicAdd(&a.rows[(size_t)x.guide * kSiteRowWords + kSiteRowAlignments], 1u);
            }
        }
        if (lane == 0) {
            a.ballot[tile] = best;
            a.tile_count[tile] = (uint32_t)__popcll(best);
        }
    }
}

template <int kPlain>
__global__ __launch_bounds__(kWave *kWavesPerGroup) void site_write_kernel(const SiteArgs a)
{
    __shared__ uint32_t s_row[kWavesPerGroup][kWave];  // kSiteRowWords = 30 in use
    const uint32_t lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    uint32_t *row = s_row[wave];
    row[lane] = 0;
    wave_sync();
    const uint32_t n_tiles = a.tiles_plain + a.tiles_bulged;
    uint32_t t0, t1;
    cell_tile_run(n_tiles, blockIdx.x * kWavesPerGroup + wave, gridDim.x * kWavesPerGroup, &t0, &t1);
    for (uint32_t tile = t0; tile < t1; ++tile) {
        const unsigned long long best = a.ballot[tile];
        if (best == 0) continue;  // wave-uniform
        const bool mine = (best >> lane) & 1u;
        const bool in_bulged = tile >= a.tiles_plain;
        const uint32_t base = in_bulged ? a.tiles_plain : 0u;
        const uint32_t n = in_bulged ? a.n_bulged : a.n_plain;
        const unsigned long long at = (unsigned long long)(tile - base) * kSiteTile + lane;
        const uint32_t i = at < n ? (uint32_t)at : 0u;  // (a flagged lane has at < n)
        const SiteAln x = in_bulged ? site_load<kSiteBulge>(a.bulged, i) : site_load<kPlain>(a.plain, i);
        SiteView v{kSiteNoMembers, ~0u};
        if (mine) v = site_gather<kPlain>(a.plain, a.n_plain, a.bulged, a.n_bulged, in_bulged, i, x, a.len, a.anchor);
        if (a.sites && mine) {
            const uint32_t j = site_other_below<kPlain>(a.plain, a.n_plain, a.bulged, a.n_bulged, in_bulged, x);
            const unsigned long long other = in_bulged ? site_survivors_below(a, 0u, a.tiles_plain, a.n_plain, j)
                                                       : site_survivors_below(a, a.tiles_plain, a.tiles_bulged, a.n_bulged, j);
            const unsigned long long rank = a.tile_off[tile] - a.tile_off[base] + (unsigned long long)__popcll(best & bits_below(lane)) + other;
            uint32_t w[8];
            site_record(x, i, v, a.len, a.anchor, w);
            if (rank < a.n_sites) {  // (always, when both passes see the same records: the test keeps a store inside the result if not)
                a.sites[2u * rank] = make_uint4(w[0], w[1], w[2], w[3]);
                a.sites[2u * rank + 1u] = make_uint4(w[4], w[5], w[6], w[7]);
            }
        }
        if (a.rows) {
            const bool known = x.guide < a.n_guides;
            const uint32_t g0 = uniform(__shfl((int)x.guide, __ffsll((long long)best) - 1, kWave));  // the guide of the first flagged lane
            if (__ballot(mine && x.guide != g0) == 0) {
                if (mine) {
                    atomicAdd(&row[kSiteRowSites], 1u);
                    atomicAdd(&row[site_row_count_word(x)], 1u);
                    if (site_bulge_only(v)) atomicAdd(&row[kSiteRowBulgeOnly], 1u);
                }
                wave_sync();
                const uint32_t n_here = row[lane];
                if (lane < kSiteRowWords && n_here && g0 < a.n_guides) atomicAdd(&a.rows[(size_t)g0 * kSiteRowWords + lane], n_here);
                row[lane] = 0;
                wave_sync();
            } else if (mine && known) {
                uint32_t *out = a.rows + (size_t)x.guide * kSiteRowWords;
                atomicAdd(&out[kSiteRowSites], 1u);
                atomicAdd(&out[site_row_count_word(x)], 1u);
                if (site_bulge_only(v)) atomicAdd(&out[kSiteRowBulgeOnly], 1u);
            }
        }
    }
}

namespace {

template <int kPlain> hipError_t launch_site_pass(const SiteArgs &args, bool write, int n_cus, hipStream_t stream)
{
    const uint32_t n_tiles = args.tiles_plain + args.tiles_bulged;
    if (n_tiles == 0) return hipSuccess;
    const dim3 grid = cell_grid(n_tiles, n_cus), block(kWave * kWavesPerGroup);
    if (write) hipLaunchKernelGGL((site_write_kernel<kPlain>), grid, block, 0, stream, args);
    else hipLaunchKernelGGL((site_flag_kernel<kPlain>), grid, block, 0, stream, args);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_site_flag(const SiteArgs &args, int plain_kind, int n_cus, hipStream_t stream)
{
    return plain_kind == kSitePattern ? launch_site_pass<kSitePattern>(args, false, n_cus, stream) : launch_site_pass<kSiteHit>(args, false, n_cus, stream);
}

hipError_t launch_site_write(const SiteArgs &args, int plain_kind, int n_cus, hipStream_t stream)
{
    return plain_kind == kSitePattern ? launch_site_pass<kSitePattern>(args, true, n_cus, stream) : launch_site_pass<kSiteHit>(args, true, n_cus, stream);
}

}  // namespace vsc
