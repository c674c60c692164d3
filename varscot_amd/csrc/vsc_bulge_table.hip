// vsc_bulge_table.hip - table scores of bulged alignments and of cut sites (vsc_bulge_hits_table, vsc_sites_table; DESIGN
// 4.24): kernels over record lists that are sorted and resident already.  The scores themselves are bulge_table_score and
// site_table_scores of vsc_bulge_table.h, the functions vsc_bulge_table_score calls on the host.
//
// bulge_table_kernel and site_table_kernel take one record per lane: waves take runs of 64-record tiles, the lane fetches its
// site's letters from the two code planes (one span of at most 34 letters: three words at the most, every one checked against
// the loaded planes), turns a '-' site into read orientation, scores it and stores its word(s) with one vector store.  The
// weights (at most 8 KB) are copied to LDS once per workgroup: a weight's index differs per lane.  The rows: per-wave LDS
// accumulators and one 64-bit integer atomic per non-zero word where the tile holds one guide (all but the tiles at a guide's
// end), one atomic per word and lane where it holds several - site_write_kernel's scheme.  Integer sums: exact in any order.
//
// The selection is pattern_select_kernel's exact radix select and in-order walk (vsc_pattern.hip) over segments given as a
// bounds array - one lower bound per guide over the site records, site_bounds_kernel - for 8-word records with 4-word score
// records beside them; the key is the score record's `top`.  No append atomic anywhere: the bytes depend on the inputs only.
#include "vsc_internal.h"
#include "vsc_cells_device.h"
#include "vsc_bulge_table.h"

namespace vsc {

namespace {

constexpr uint32_t kBtThreads = kWave * kWavesPerGroup;
constexpr uint32_t kBtTile = kWave;  // records per tile: one per lane
constexpr uint32_t kBtRowSlots = 16;  // LDS words of a wave's row: kBulgeTableRowWords = 12 in use

// The n <= 34 letters from global position `start` on as 64-bit planes (bit j = letter j, the bits from n on zero); false
// when the span begins in front of the planes or touches a word that was not loaded.
__device__ __forceinline__ bool span_fetch(const BulgePlanes &p, unsigned long long start, uint32_t n, unsigned long long *h,
                                           unsigned long long *l)
{
    if (start < p.first_pos || n == 0 || n > 34u) return false;
    const unsigned long long rel = start - p.first_pos;
    const unsigned long long wi = rel >> 5;
    const uint32_t shift = (uint32_t)rel & 31u, last = (shift + n - 1u) >> 5;  // 0 .. 2: the words behind the first
    if (wi + last >= p.n_words) return false;
    const uint32_t h0 = p.hi[wi], l0 = p.lo[wi];
    const uint32_t h1 = last >= 1u ? p.hi[wi + 1] : 0u, l1 = last >= 1u ? p.lo[wi + 1] : 0u;
    const uint32_t h2 = last >= 2u ? p.hi[wi + 2] : 0u, l2 = last >= 2u ? p.lo[wi + 2] : 0u;
    unsigned long long vh = ((unsigned long long)h1 << 32 | h0) >> shift, vl = ((unsigned long long)l1 << 32 | l0) >> shift;
    if (shift) {  // (last == 2 needs shift >= 31)
        vh |= (unsigned long long)h2 << (64u - shift);
        vl |= (unsigned long long)l2 << (64u - shift);
    }
    const unsigned long long keep = ~0ull >> (64u - n);
    *h = vh & keep;
    *l = vl & keep;
    return true;
}

// the span [pos, pos + n) of contig c in read orientation for strand `rev`; false when the contig is unknown, the span leaves
// it or leaves the loaded planes
__device__ __forceinline__ bool site_span(const BulgePlanes &p, uint32_t contig, long long pos, uint32_t n, bool rev, unsigned long long *h,
                                          unsigned long long *l)
{
    if (contig >= p.n_contigs || pos < 0) return false;
    const unsigned long long start = (unsigned long long)p.contig_off[contig] + (unsigned long long)pos;
    if (start + n > p.contig_end[contig]) return false;
    if (!span_fetch(p, start, n, h, l)) return false;
    if (rev) {
        *h = span_revcomp(*h, n);
        *l = span_revcomp(*l, n);
    }
    return true;
}

__device__ __forceinline__ BulgeGuide load_guide(const uint4 *guides, uint32_t g)
{
    const uint4 w = guides[2u * g], q = guides[2u * g + 1u];
    return BulgeGuide{w.x, w.y, w.z, PatPlanes{q.x, q.y, q.z, q.w}};
}

// One scored record of the lane (f, NM; counted = it is one of a known guide) into the rows: through the wave's LDS row where
// all the tile's records are of one guide, straight into the result where they are not.
__device__ __forceinline__ void rows_add(unsigned long long *rows, unsigned long long *row, uint32_t lane, bool has, uint32_t guide, bool known,
                                         uint32_t f, uint32_t nm)
{
    const uint32_t at = 2u + (nm < (uint32_t)VSC_MAX_MISMATCHES ? nm : (uint32_t)VSC_MAX_MISMATCHES);
    const uint32_t g0 = uniform(guide);  // lane 0 holds a record
    const bool add = has && known && f > 0u;
    if (__ballot(has && guide != g0) == 0) {
        if (add) {
            atomicAdd(&row[0], (unsigned long long)f);
            atomicAdd(&row[1], 1ull);
            atomicAdd(&row[at], 1ull);
        }
        wave_sync();
        const unsigned long long here = lane < kBtRowSlots ? row[lane] : 0ull;
        if (lane < kBulgeTableRowWords && here) atomicAdd(&rows[(size_t)g0 * kBulgeTableRowWords + lane], here);
        if (lane < kBtRowSlots) row[lane] = 0;
        wave_sync();
    } else if (add) {
        unsigned long long *out = rows + (size_t)guide * kBulgeTableRowWords;
        atomicAdd(&out[0], (unsigned long long)f);
        atomicAdd(&out[1], 1ull);
        atomicAdd(&out[at], 1ull);
    }
}

__device__ __forceinline__ void load_weights(double *s_w, const BulgeTableArgs &a)
{
    const uint32_t n_w = bulge_table_weights(a.shape);  // (<= kBulgeTableMaxWeights: the host has checked the shape)
    for (uint32_t i = threadIdx.x; i < n_w && i < kBulgeTableMaxWeights; i += kBtThreads) s_w[i] = a.weights[i];
    block_sync();
}

}  // namespace

__global__ __launch_bounds__(kWave *kWavesPerGroup) void bulge_table_kernel(const BulgeTableArgs a)
{
    __shared__ double s_w[kBulgeTableMaxWeights];
    __shared__ unsigned long long s_row[kWavesPerGroup][kBtRowSlots];
    load_weights(s_w, a);
    const uint32_t lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    unsigned long long *row = s_row[wave];
    if (lane < kBtRowSlots) row[lane] = 0;
    wave_sync();
    const uint32_t n_tiles = (a.n + kBtTile - 1u) / kBtTile;
    uint32_t t0, t1;
    cell_tile_run(n_tiles, blockIdx.x * kWavesPerGroup + wave, gridDim.x * kWavesPerGroup, &t0, &t1);
    for (uint32_t tile = t0; tile < t1; ++tile) {
        const unsigned long long at = (unsigned long long)tile * kBtTile + lane;
        const bool has = at < a.n;
        const uint4 r = a.hits[has ? at : 0u];  // (a tile exists only where the list has a record: record 0 is there)
        const bool known = r.x < a.n_guides;
        const uint32_t size = (r.w >> 10) & 3u, index = (r.w >> 5) & 31u, nm = r.w & 31u;
        const int d = ((r.w >> 12) & 1u) ? -(int)size : (int)size;
        uint32_t f = 0;
        if (has && known && bulge_table_defined(a.shape, d, index)) {
            unsigned long long h, l;
            if (site_span(a.planes, r.y, (long long)r.z, (uint32_t)((int)a.shape.len + d), (r.w >> 31) != 0u, &h, &l))
                f = bulge_table_fixed(s_w, a.shape, load_guide(a.guides, r.x), (uint32_t)h, (uint32_t)l, d, index);
        }
        if (a.fixed && has) a.fixed[at] = f;
        if (a.rows) rows_add(a.rows, row, lane, has, r.x, known, f, nm);
    }
}

__global__ __launch_bounds__(kWave *kWavesPerGroup) void site_table_kernel(const BulgeTableArgs a)
{
    __shared__ double s_w[kBulgeTableMaxWeights];
    __shared__ unsigned long long s_row[kWavesPerGroup][kBtRowSlots];
    load_weights(s_w, a);
    const uint32_t lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    unsigned long long *row = s_row[wave];
    if (lane < kBtRowSlots) row[lane] = 0;
    wave_sync();
    const uint32_t n_tiles = (a.n + kBtTile - 1u) / kBtTile;
    uint32_t t0, t1;
    cell_tile_run(n_tiles, blockIdx.x * kWavesPerGroup + wave, gridDim.x * kWavesPerGroup, &t0, &t1);
    for (uint32_t tile = t0; tile < t1; ++tile) {
        const unsigned long long at = (unsigned long long)tile * kBtTile + lane;
        const bool has = at < a.n;
        const uint4 r = a.sites[2u * (has ? at : 0u)], q = a.sites[2u * (has ? at : 0u) + 1u];
        const bool known = r.x < a.n_guides;
        const uint32_t strand = r.w >> 31, size = (r.w >> 10) & 3u;
        const int best_d = ((r.w >> 12) & 1u) ? -(int)size : (int)size;
        const uint32_t n = site_span_letters(a.shape.len, q.y);
        const bool at_start = site_anchor_at_start(a.anchor, strand);  // ... of the forward span; in read orientation: anchor == START
        SiteScores s{0u, 0u, 0u, 0u};
        if (has && known && n) {
            unsigned long long h, l;
            const long long pos = at_start ? (long long)q.x : (long long)q.x - (long long)n;
            if (site_span(a.planes, r.y, pos, n, strand != 0u, &h, &l))
                site_table_scores(s_w, a.shape, load_guide(a.guides, r.x), h, l, n, a.anchor == VSC_SITE_ANCHOR_START, q.y, best_d, &s);
        }
        if (a.scores && has) a.scores[at] = make_uint4(s.best, s.top, s.top_d, 0u);
        if (a.rows) rows_add(a.rows, row, lane, has, r.x, known, s.top, s.best_nm);
    }
}

// ---- selection over scored sites ----------------------------------------------------------------------------------------
// bounds[g] = #{sites with guide < g}, g = 0 .. n_guides: one thread each.
__global__ __launch_bounds__(kWave *kWavesPerGroup) void site_bounds_kernel(const SiteSelectArgs a)
{
    const uint32_t g = blockIdx.x * kBtThreads + threadIdx.x;
    if (g > a.n_guides) return;
    uint32_t lo = 0, hi = a.n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (a.sites[2u * (size_t)mid].x < g) lo = mid + 1u; else hi = mid;
    }
    a.bounds[g] = lo;
}

namespace {

// [*begin, *end) of guide r's sites (ascending bounds when the sites are in their order; kept inside the list whatever they hold)
__device__ __forceinline__ void site_segment(const SiteSelectArgs &a, uint32_t r, uint32_t *begin, uint32_t *end)
{
    uint32_t b = a.bounds[r], e = a.bounds[r + 1u];
    if (e > a.n) e = a.n;
    if (b > e) b = e;
    *begin = b;
    *end = e;
}

__device__ __forceinline__ uint32_t site_key(const SiteSelectArgs &a, uint32_t i) { return ((const uint32_t *)a.scores)[(size_t)i * kSiteScoreWords + 1u]; }

}  // namespace

// pattern_select_kernel over a segment of score records: the value T of the top_k-th survivor by four 8-bit digits of `top`
// from the most significant on (top <= 2^30), and how many records with top = T are still to take.
__global__ __launch_bounds__(kWave *kWavesPerGroup) void site_select_kernel(const SiteSelectArgs a)
{
    __shared__ uint32_t s_hist[256];
    __shared__ uint32_t s_state[4];  // prefix, k, done
    const uint32_t r = blockIdx.x, tid = threadIdx.x;
    uint32_t begin, end;
    site_segment(a, r, &begin, &end);
    uint32_t prefix = 0, mask = 0, k = a.top_k;
    for (uint32_t pass = 0; pass < 4u; ++pass) {
        const uint32_t shift = 24u - 8u * pass;
        s_hist[tid] = 0;  // (kBtThreads == 256)
        block_sync();
        for (uint32_t i = begin + tid; i < end; i += kBtThreads) {
            const uint32_t v = site_key(a, i);
            if (v >= a.min_score && (v & mask) == prefix) atomicAdd(&s_hist[(v >> shift) & 255u], 1u);
        }
        block_sync();
        if (tid == 0) {
            uint32_t done = 0;
            if (pass == 0) {
                unsigned long long survivors = 0;
                for (uint32_t b = 0; b < 256u; ++b) survivors += s_hist[b];
                if (a.top_k == 0 || survivors <= a.top_k) {  // all of them: top > min_score, and every record with top = min_score
                    a.sel[r] = make_uint4(a.min_score, ~0u, (uint32_t)survivors, (uint32_t)(survivors >> 32));
                    done = 1;
                }
            }
            if (!done) {
                // the digit of the k-th largest: the first bin from the top at which the count reaches k
                uint32_t b = 255u, above = 0;
                while (b > 0u && above + s_hist[b] < k) above += s_hist[b--];
                s_state[0] = prefix | b << shift;
                s_state[1] = k - above;
            }
            s_state[2] = done;
        }
        block_sync();
        if (s_state[2]) return;  // (uniform over the workgroup)
        prefix = s_state[0];
        k = s_state[1];
        mask |= 255u << shift;
        block_sync();  // (s_state and s_hist are written again)
    }
    if (tid == 0) a.sel[r] = make_uint4(prefix, k, a.top_k, 0u);  // T = prefix; k of the records with top = T are taken
}

// pattern_select_walk_kernel over the segment: in record order, 256 records a step, keep top > T and the first `take` records
// with top = T - the ranking's tie-break IS the record order.
__global__ __launch_bounds__(kWave *kWavesPerGroup) void site_select_walk_kernel(const SiteSelectArgs a)
{
    __shared__ uint32_t s_ws[kWavesPerGroup], s_ws2[kWavesPerGroup];
    const uint32_t r = blockIdx.x, tid = threadIdx.x;
    uint32_t begin, end;
    site_segment(a, r, &begin, &end);
    unsigned long long out = 0;  // the survivors of the guides in front
    for (uint32_t q = 0; q < r; ++q) out += (unsigned long long)a.sel[q].w << 32 | a.sel[q].z;
    const uint4 mine = a.sel[r];
    const uint32_t T = mine.x;
    const unsigned long long take = mine.y == ~0u ? ~0ull : mine.y;
    unsigned long long ties = 0;  // records with top = T in front of this step
    for (uint32_t base = begin; base < end; base += kBtThreads) {
        const bool live = tid < end - base;
        const uint32_t i = live ? base + tid : begin;
        const uint32_t v = live ? site_key(a, i) : 0u;
        const bool tie = live && v == T;
        uint32_t step_ties, step_kept;
        const uint32_t tie_rank = block_exclusive(tie ? 1u : 0u, s_ws, &step_ties);
        const bool keep = live && (v > T || (tie && ties + tie_rank < take));  // (T >= min_score)
        const uint32_t rank = block_exclusive(keep ? 1u : 0u, s_ws2, &step_kept);
        const unsigned long long at = out + rank;
        if (keep && at < a.n_out) {
            a.out_sites[2u * at] = a.sites[2u * (size_t)i];
            a.out_sites[2u * at + 1u] = a.sites[2u * (size_t)i + 1u];
            a.out_scores[at] = a.scores[i];
        }
        ties += step_ties;
        out += step_kept;
    }
}

// ---- launches ----------------------------------------------------------------------------------------------------------
hipError_t launch_bulge_table(const BulgeTableArgs &args, int n_cus, hipStream_t stream)
{
    if (args.n == 0) return hipSuccess;
    hipLaunchKernelGGL(bulge_table_kernel, cell_grid((args.n + kBtTile - 1u) / kBtTile, n_cus), dim3(kBtThreads), 0, stream, args);
    return hipGetLastError();
}

hipError_t launch_site_table(const BulgeTableArgs &args, int n_cus, hipStream_t stream)
{
    if (args.n == 0) return hipSuccess;
    hipLaunchKernelGGL(site_table_kernel, cell_grid((args.n + kBtTile - 1u) / kBtTile, n_cus), dim3(kBtThreads), 0, stream, args);
    return hipGetLastError();
}

hipError_t launch_site_bounds(const SiteSelectArgs &args, hipStream_t stream)
{
    hipLaunchKernelGGL(site_bounds_kernel, dim3(args.n_guides / kBtThreads + 1u), dim3(kBtThreads), 0, stream, args);
    return hipGetLastError();
}

hipError_t launch_site_select(const SiteSelectArgs &args, hipStream_t stream)
{
    if (args.n_guides == 0) return hipSuccess;
    hipLaunchKernelGGL(site_select_kernel, dim3(args.n_guides), dim3(kBtThreads), 0, stream, args);
    return hipGetLastError();
}

hipError_t launch_site_select_walk(const SiteSelectArgs &args, hipStream_t stream)
{
    if (args.n_guides == 0) return hipSuccess;
    hipLaunchKernelGGL(site_select_walk_kernel, dim3(args.n_guides), dim3(kBtThreads), 0, stream, args);
    return hipGetLastError();
}

}  // namespace vsc
