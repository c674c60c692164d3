// vsc_pattern.hip - the pattern search (vsc_search_pattern): every site of L = 16 .. 32 bases of the resident
// planes that satisfies an IUPAC pattern, holds no N and lies within the budget of an IUPAC guide, as vsc_pattern_hit records in
// ascending (guide, strand, contig, pos) order and / or as per-guide rows of counts by NM.
//
// The front end is enum_kernel's and bulge_front's: a tile of 2 048 site starts per wave step, one 32-start word of each plane
// per lane plus its right neighbour - a site of 32 bases that starts at bit 31 ends at bit 62 of the pair.  Per strand one
// start mask, 32 starts per instruction: no N in the L bases, and for every pattern position that is not N one funnel shift
// of each plane and the position's truth table over (hi, lo).  The '-' strand is the reverse complement of the pattern as a
// second forward pattern: nothing is bit-reversed anywhere.
//
// The candidate walk is scan_kernel's queue, not the lane walk of the bulge kernels: per strand the starts of the tile are
// compacted into the wave's LDS queue (rank = lanes in front + order in the lane), and every step takes kPatSlots x 64 of them,
// all lanes busy, against the round's guides; the guides' planes come through the constant address space (scalar loads), four
// guides per load, the next four fetched while these are compared.  DESIGN 4.17 says why.
//
// The back end is count, scan, write, as vsc_bulge.hip's, with one count per CELL (guide of the round, strand, tile):
//   pattern_count_kernel    hits per cell: the ballots of a guide's compares are added in lane g of the wave.
//   bulge_chunk_sum_kernel twice + enum_scan_kernel (vsc_bulge.hip, vsc_enum.hip)  the cells' counts to sums per 64 cells, those
//                           to sums per 64 x 64 cells, and only these - a 64th of the chunks - through the one-workgroup scan.
//   pattern_write_kernel    only the tiles with a cell that is not empty are visited again, and of those only the live cells;
//                           every hit goes to  group offset + chunks before it in the group + cells before it in the chunk +
//                           hits of earlier steps + lanes in front.  The rows come from this pass.
// No record is placed through an atomic and nothing is sorted: the bytes depend on the planes and the parameters only.
//
// Beside the write pass: pattern_write_scored_kernel (vsc_search_pattern_table) - the same pass, every hit lane also
// taking the table score of its site, and pattern_select_kernel / pattern_select_walk_kernel, the floor and the top K per guide.
//
// Behind the search: pattern_enum_kernel (vsc_guides_enumerate_pattern) - the same front end without the queue,
// in front of enum_kernel's count / scan / write.
#include "vsc_internal.h"
#include "vsc_device.h"
#include "vsc_pattern.h"
#include "vsc_pattern_device.h"
#include "vsc_pattern_enum.h"

namespace vsc {

static_assert(kPatChunk == kCellChunk, "cell_offset takes one load per lane");

namespace {

constexpr uint32_t kPatQueue = kTileBases;  // every start of a tile can be a candidate (a pattern of N only)

// The wave's LDS: the tile's words of both planes (65 each: the last lane's right neighbour) and the queue of starts.
struct PatLds {
    uint32_t h[kTileWords + 2], l[kTileWords + 2];
    uint16_t q[kPatQueue];  // lane << 5 | bit, ascending
    uint32_t row[16];       // write pass: the cell's hits by NM
};

// A lane's word of each plane with its right neighbour, and the two start masks of its 32 starts (both searches' and the
// enumeration's front end).  kArgs: PatternArgs or PatEnumArgs.
template <typename kArgs>
__device__ __forceinline__ void pattern_words(const kArgs &a, uint32_t tile, uint32_t lane, uint32_t &H0, uint32_t &H1, uint32_t &L0,
                                              uint32_t &L1, uint32_t *mf, uint32_t *mr)
{
    const size_t wi = (size_t)tile * kTileWords + lane;  // (< n_tiles * 64, and the planes are padded by kPadWords)
    H0 = a.hi[wi], H1 = a.hi[wi + 1];
    L0 = a.lo[wi], L1 = a.lo[wi + 1];
    const uint32_t N0 = a.nm[wi], N1 = a.nm[wi + 1];
    uint64_t nn = ((uint64_t)N1 << 32) | N0;
    nn |= nn >> 1;
    nn |= nn >> 2;
    nn |= nn >> 4;
    nn |= nn >> 8;  // bit i covers positions i .. i+15
    const uint32_t clean = ~(uint32_t)(nn | nn >> (a.len - kPatMinLen));  // no N in positions i .. i+L-1
    *mf = pattern_starts(a.front[0], H0, H1, L0, L1) & clean;
    *mr = pattern_starts(a.front[1], H0, H1, L0, L1) & clean;
}

// The tile's words into LDS and the two start masks.
__device__ __forceinline__ void pattern_tile(const PatternArgs &a, uint32_t tile, uint32_t lane, PatLds &s, uint32_t *mf, uint32_t *mr)
{
    uint32_t H0, H1, L0, L1;
    pattern_words(a, tile, lane, H0, H1, L0, L1, mf, mr);
    s.h[lane] = H0;
    s.l[lane] = L0;
    if (lane == kWave - 1) {
        s.h[kWave] = H1;
        s.l[kWave] = L1;
    }
}

// The starts of mask m into the queue, in ascending order over the wave; returns how many there are.  The hand-offs before
// (the planes, the queue's last readers) and after are the caller's.
__device__ __forceinline__ uint32_t pattern_enqueue(PatLds &s, uint32_t m, uint32_t lane)
{
    uint32_t total;
    uint32_t at = wave_exclusive((uint32_t)__popc(m), lane, &total);
    for (; m; m &= m - 1u) s.q[at++] = (uint16_t)(lane << 5 | (uint32_t)__builtin_ctz(m));  // (at < 2 048: one entry per start)
    return total;
}

// the L (and more) bases from queue entry e on, on the forward genome
__device__ __forceinline__ void pattern_site(const PatLds &s, uint32_t e, uint32_t *wh, uint32_t *wl)
{
    const uint32_t src = e >> 5, b = e & 31u;  // (src <= 63: src + 1 <= 64 is the last lane's right neighbour)
    *wh = funnel(s.h[src + 1], s.h[src], b);
    *wl = funnel(s.l[src + 1], s.l[src], b);
}

__device__ __forceinline__ PatPlanes planes_of(v4u v) { return PatPlanes{v.x, v.y, v.z, v.w}; }

// the L-bit plane p of a forward site as the plane of its reverse complement: bit j to L - 1 - j, inverted; bits from L on 0
__device__ __forceinline__ uint32_t pattern_revcomp_plane(uint32_t p, uint32_t len) { return (~__brev(p)) >> (32u - len); }

// The scored write pass's LDS beside PatLds: the cell's table row (score_sum, positive_nm; positive is their sum).
struct PatScoreLds {
    unsigned long long sum;
    uint32_t pos[kPatRowWords];
};

// One step of the count pass: kSlots x 64 queued sites from `base` on against every guide of the round; lane g adds the hits
// of guide g to cnt.  An instance per number of slots (kPatSlots of them) instead of a test per slot and guide: the last step
// of a tile is as cheap per pair as a full one.
template <uint32_t kSlots>
__device__ __forceinline__ void pattern_count_step(const PatLds &s, const_v16u_ptr gq, uint32_t n_guides, uint32_t m,
                                                   uint32_t base, uint32_t total, uint32_t lane, uint32_t &cnt)
{
    uint32_t wh[kSlots], wl[kSlots], dead[kSlots];
#pragma unroll
    for (uint32_t j = 0; j < kSlots; ++j) {
        const uint32_t idx = base + j * kWave + lane;
        const bool live = idx < total;
        pattern_site(s, live ? s.q[idx] : 0u, &wh[j], &wl[j]);
        dead[j] = live ? 0u : 33u;  // added to the popcount (v_bcnt's own addend): an empty slot is over every budget
    }
    // four guides per scalar load (64 bytes), the next four fetched while these are compared: a wave waits for the scalar
    // cache once per four guides, and the table ends with four spare guides
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
                const uint32_t nm = (uint32_t)__popc(pattern_mismatch(wh[j], wl[j], planes)) + dead[j];
                hits += (uint32_t)__popcll(__ballot(nm <= m));
            }
            if (lane == g + u) cnt += hits;  // (a guide that pads the last four is all zero: it allows nothing and never hits)
        }
    }
}

}  // namespace

// ---- count pass --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kWave *kWavesPerGroup) void pattern_count_kernel(const PatternArgs a)
{
    __shared__ PatLds s_lds[kWavesPerGroup];
    const uint32_t lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    PatLds &s = s_lds[wave];
    uint32_t t0, t1;
    cell_tile_run(a.n_tiles, blockIdx.x * kWavesPerGroup + wave, gridDim.x * kWavesPerGroup, &t0, &t1);
    const uint32_t m = a.max_mm;
    unsigned long long sites = 0;
    for (uint32_t tile = t0; tile < t1; ++tile) {
        uint32_t mask[2];
        wave_sync();  // (the last tile's readers of the planes and the queue are done)
        pattern_tile(a, tile, lane, s, &mask[0], &mask[1]);
        uint32_t cnt[2] = {0, 0};  // lane g: the hits of guide g of the round, per strand
#pragma unroll
        for (uint32_t strand = 0; strand < 2; ++strand) {
            if (strand) wave_sync();  // (the '+' steps have read the queue)
            const uint32_t total = pattern_enqueue(s, mask[strand], lane);
            wave_sync();
            sites += total;
            const const_v16u_ptr gq = (const_v16u_ptr)(uintptr_t)(a.guides + strand * a.guide_stride);
            for (uint32_t base = 0; base < total; base += kPatSlots * kWave) {
                const uint32_t left = (total - base + kWave - 1u) / kWave;  // wave-uniform: steps of 64 sites that are left
                if (left >= 4u) pattern_count_step<4>(s, gq, a.n_guides, m, base, total, lane, cnt[strand]);
                else if (left == 3u) pattern_count_step<3>(s, gq, a.n_guides, m, base, total, lane, cnt[strand]);
                else if (left == 2u) pattern_count_step<2>(s, gq, a.n_guides, m, base, total, lane, cnt[strand]);
                else pattern_count_step<1>(s, gq, a.n_guides, m, base, total, lane, cnt[strand]);
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
namespace {

// kScore: the scored pass of vsc_search_pattern_table - every hit lane also takes the product of the table over
// its site, which it holds in registers, and the cell's table row is gathered beside the NM row.  w: the table's weights in
// LDS, rows_lds: the waves' table rows.  The unscored instance is the kernel of DESIGN 4.17: the same registers and LDS.
template <bool kScore>
__device__ __forceinline__ void pattern_write(const PatternArgs &a, const PatScoreArgs &sc, PatLds *lds, const double *w, PatScoreLds *rows_lds)
{
    const uint32_t lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    PatLds &s = lds[wave];
    PatScoreLds &ts = rows_lds[kScore ? wave : 0u];
    if (lane < 16u) s.row[lane] = 0;
    if (kScore) {
        if (lane < kPatRowWords) ts.pos[lane] = 0;
        if (lane == 0) ts.sum = 0;
    }
    uint32_t t0, t1;
    cell_tile_run(a.n_tiles, blockIdx.x * kWavesPerGroup + wave, gridDim.x * kWavesPerGroup, &t0, &t1);
    const const_v4u_ptr gp = (const_v4u_ptr)(uintptr_t)a.guides;
    const uint32_t m = a.max_mm;
    uint32_t c_id = 0, c_off = 1, c_end = 0;  // the contig of the lane's last hit: [c_off, c_end) in global positions (empty at first)
    for (uint32_t tile = t0; tile < t1; ++tile) {
        // which cells of the round have a hit in this tile: lane l looks at cell l (guide l / 2, strand l & 1), then at 64 + l
        const uint32_t n_cells = 2u * a.n_guides;
        const uint64_t live_lo = __ballot(lane < n_cells && a.count[(size_t)lane * a.n_tiles + tile] != 0);
        uint64_t live_hi = 0;
        if (n_cells > (uint32_t)kWave) live_hi = __ballot(kWave + lane < n_cells && a.count[(size_t)(kWave + lane) * a.n_tiles + tile] != 0);
        if ((live_lo | live_hi) == 0) continue;
        uint32_t mask[2];
        wave_sync();  // (the last tile's readers of the planes and the queue are done)
        pattern_tile(a, tile, lane, s, &mask[0], &mask[1]);
        const uint32_t tile_pos = a.first_pos + tile * (uint32_t)kTileBases;
        for (uint32_t strand = 0; strand < 2; ++strand) {
            const uint64_t odd = 0xAAAAAAAAAAAAAAAAull;
            const uint64_t sel = strand ? odd : odd >> 1;
            if (((live_lo | live_hi) & sel) == 0) continue;  // wave-uniform: no guide has a hit on this strand
            wave_sync();  // (the '+' steps have read the queue)
            const uint32_t total = pattern_enqueue(s, mask[strand], lane);
            wave_sync();
            for (uint32_t g = 0; g < a.n_guides; ++g) {
                const uint64_t word = g < 32u ? live_lo : live_hi;
                if (((word >> (2u * (g & 31u) + strand)) & 1u) == 0) continue;  // wave-uniform
                const PatPlanes planes = planes_of(gp[strand * a.guide_stride + g]);
                v4u read{};  // kScore: the guide in read orientation (gh, gl, single)
                if (kScore) read = gp[2u * a.guide_stride + g];
                const unsigned long long cell = (unsigned long long)(2u * g + strand) * a.n_tiles + tile;
                unsigned long long at = a.records ? cell_offset(a.count, a.chunk_sum, a.group_off, cell, lane) : 0ull;
                for (uint32_t base = 0; base < total; base += kWave) {
                    const uint32_t idx = base + lane;
                    const bool live = idx < total;
                    const uint32_t e = live ? s.q[idx] : 0u;
                    uint32_t wh, wl;
                    pattern_site(s, e, &wh, &wl);
                    const uint32_t x = pattern_mismatch(wh, wl, planes);  // the mismatches at forward-genome positions
                    const uint32_t nm = (uint32_t)__popc(x);
                    const bool hit = live && nm <= m;
                    const uint64_t hits = __ballot(hit);
                    if (hits == 0) continue;
                    if (hit) {
                        if (a.rows) atomicAdd(&s.row[nm], 1u);
                        uint32_t f = 0;
                        if (kScore) {
                            // the site in read orientation: as it lies on '+', reversed and complemented on '-'
                            const uint32_t rh = strand ? pattern_revcomp_plane(wh, a.len) : wh;
                            const uint32_t rl = strand ? pattern_revcomp_plane(wl, a.len) : wl;
                            f = table_fixed(pattern_table_score(w, sc.shape, read.x, read.y, read.z, rh, rl));
                            if (sc.table_rows) {
                                atomicAdd(&ts.sum, (unsigned long long)f);
                                if (f) atomicAdd(&ts.pos[nm], 1u);
                            }
                        }
                        if (a.records) {
                            const uint32_t pos = tile_pos + e;  // (e = lane << 5 | bit = the start's offset in the tile)
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
                            if (r < a.n_records) {
                                uint32_t *rec = a.records + r * kPatRecordWords;
                                rec[0] = a.guide_base + g;
                                rec[1] = c_id;
                                rec[2] = pos - c_off;
                                rec[3] = strand << 31 | nm;
                                rec[4] = x;
                                if (kScore) sc.fixed[r] = f;
                            }
                        }
                    }
                    at += (uint32_t)__popcll(hits);
                }
                if (a.rows) {
                    wave_sync();
                    const uint32_t v = lane < kPatRowWords ? s.row[lane] : 0u;
                    if (v) {
                        atomicAdd(&a.rows[(size_t)(a.guide_base + g) * kPatRowWords + lane], v);
                        s.row[lane] = 0;
                    }
                    wave_sync();
                }
                if (kScore && sc.table_rows) {
                    // the cell's table row: positive_nm from lanes 0..8, positive (their sum) from lane 9, score_sum from lane 10
                    wave_sync();
                    const uint32_t v = lane < kPatRowWords ? ts.pos[lane] : 0u;
                    const uint32_t positive = wave_sum(v);
                    const unsigned long long sum = ts.sum;
                    wave_sync();
                    unsigned long long *row = sc.table_rows + (size_t)(a.guide_base + g) * kPatTableRowWords;
                    if (lane < kPatRowWords && v) {
                        atomicAdd(&row[2u + lane], (unsigned long long)v);
                        ts.pos[lane] = 0;
                    }
                    if (lane == kPatRowWords && positive) atomicAdd(&row[1], (unsigned long long)positive);
                    if (lane == kPatRowWords + 1u && sum) {
                        atomicAdd(&row[0], sum);
                        ts.sum = 0;
                    }
                    wave_sync();
                }
            }
        }
    }
}

}  // namespace

__global__ __launch_bounds__(kWave *kWavesPerGroup) void pattern_write_kernel(const PatternArgs a)
{
    __shared__ PatLds s_lds[kWavesPerGroup];
    PatScoreLds none;
    pattern_write<false>(a, PatScoreArgs{}, s_lds, nullptr, &none);
}

// ---- scored write pass (vsc_search_pattern_table) ----------------------------------------------------------
__global__ __launch_bounds__(kWave *kWavesPerGroup) void pattern_write_scored_kernel(const PatternArgs a, const PatScoreArgs sc)
{
    __shared__ PatLds s_lds[kWavesPerGroup];
    __shared__ PatScoreLds s_rows[kWavesPerGroup];
    __shared__ double s_w[kPatTableMaxWeights];
    const uint32_t n_w = pattern_table_weights(sc.shape);  // (<= kPatTableMaxWeights: the host has checked the shape)
    for (uint32_t i = threadIdx.x; i < n_w && i < kPatTableMaxWeights; i += kWave * kWavesPerGroup) s_w[i] = sc.weights[i];
    block_sync();
    pattern_write<true>(a, sc, s_lds, s_w, s_rows);
}

// ---- selection stage --------------------------------------------------------------------------------------
// One workgroup per guide of the round.  The guide's records are one segment of the round's: from the offset of its first
// '+' cell to that of the next guide's.  pattern_select_kernel finds, by an exact radix select over the segment's f words
// (four 8-bit digits from the top: f <= 2^30), the value T of the top_k-th survivor and how many records with f = T are
// still to take; pattern_select_walk_kernel then walks the segment in record order, 256 records a step, and keeps f > T and
// the first `take` records with f = T - the ranking's tie-break IS the record order.  Nothing is appended through an atomic.
namespace {

constexpr uint32_t kPatSelThreads = kWave * kWavesPerGroup;

// [*begin, *end) of guide r's records among the round's (every wave computes both: cell_offset is a wave's)
__device__ __forceinline__ void select_segment(const PatSelectArgs &a, uint32_t r, uint32_t lane, unsigned long long *begin, unsigned long long *end)
{
    unsigned long long b = cell_offset(a.count, a.chunk_sum, a.group_off, (unsigned long long)(2u * r) * a.n_tiles, lane);
    unsigned long long e = r + 1u < a.n_guides ? cell_offset(a.count, a.chunk_sum, a.group_off, (unsigned long long)(2u * r + 2u) * a.n_tiles, lane)
                                               : a.n_records;
    if (e > a.n_records) e = a.n_records;  // (never, when the passes saw the same planes: keeps every read inside the arrays)
    if (b > e) b = e;
    *begin = b;
    *end = e;
}

}  // namespace

__global__ __launch_bounds__(kWave *kWavesPerGroup) void pattern_select_kernel(const PatSelectArgs a)
{
    __shared__ uint32_t s_hist[256];
    __shared__ uint32_t s_state[4];  // prefix, k, done
    const uint32_t r = blockIdx.x, tid = threadIdx.x, lane = tid % kWave;
    unsigned long long begin, end;
    select_segment(a, r, lane, &begin, &end);
    const unsigned long long n = end - begin;
    const uint32_t *f = a.fixed + begin;
    uint32_t prefix = 0, mask = 0, k = a.top_k;
    for (uint32_t pass = 0; pass < 4u; ++pass) {
        const uint32_t shift = 24u - 8u * pass;
        s_hist[tid] = 0;  // (kPatSelThreads == 256)
        block_sync();
        for (unsigned long long i = tid; i < n; i += kPatSelThreads) {
            const uint32_t v = f[i];
            if (v >= a.min_score && (v & mask) == prefix) atomicAdd(&s_hist[(v >> shift) & 255u], 1u);
        }
        block_sync();
        if (tid == 0) {
            uint32_t done = 0;
            if (pass == 0) {
                unsigned long long survivors = 0;
                for (uint32_t b = 0; b < 256u; ++b) survivors += s_hist[b];
                if (a.top_k == 0 || survivors <= a.top_k) {  // all of them: f > min_score, and every record with f = min_score
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
    if (tid == 0) a.sel[r] = make_uint4(prefix, k, a.top_k, 0u);  // T = prefix; k of the records with f = T are taken
}

__global__ __launch_bounds__(kWave *kWavesPerGroup) void pattern_select_walk_kernel(const PatSelectArgs a)
{
    __shared__ uint32_t s_ws[kWavesPerGroup], s_ws2[kWavesPerGroup];
    const uint32_t r = blockIdx.x, tid = threadIdx.x, lane = tid % kWave;
    unsigned long long begin, end;
    select_segment(a, r, lane, &begin, &end);
    const unsigned long long n = end - begin;
    unsigned long long out = 0;  // the survivors of the guides in front
    for (uint32_t q = 0; q < r; ++q) out += (unsigned long long)a.sel[q].w << 32 | a.sel[q].z;
    const uint4 mine = a.sel[r];
    const uint32_t T = mine.x;
    const unsigned long long take = mine.y == ~0u ? ~0ull : mine.y;
    unsigned long long ties = 0;  // records with f = T in front of this step
    for (unsigned long long base = 0; base < n; base += kPatSelThreads) {
        const unsigned long long i = base + tid;
        const bool live = i < n;
        const uint32_t v = live ? a.fixed[begin + i] : 0u;
        const bool tie = live && v == T;
        uint32_t step_ties, step_kept;
        const uint32_t tie_rank = block_exclusive(tie ? 1u : 0u, s_ws, &step_ties);
        const bool keep = live && (v > T || (tie && ties + tie_rank < take));
        const uint32_t rank = block_exclusive(keep ? 1u : 0u, s_ws2, &step_kept);
        const unsigned long long at = out + rank;
        if (keep && at < a.n_out) {
            const uint32_t *src = a.records + (begin + i) * kPatRecordWords;
            uint32_t *dst = a.out_records + at * kPatRecordWords;
#pragma unroll
            for (uint32_t k = 0; k < kPatRecordWords; ++k) dst[k] = src[k];
            a.out_fixed[at] = v;
        }
        ties += step_ties;
        out += step_kept;
    }
}

// ---- pattern guide discovery (vsc_guides_enumerate_pattern) ---------------------------------------------------
// The searches' front end in front of enum_kernel's back end (vsc_enum.hip): one wave per tile of the work list, the start
// masks of both strands from pattern_words, no LDS - there is no guide loop, so no queue.  Two passes over the same masks:
// pattern_enum_kernel<false> counts per tile, enum_scan_kernel turns the counts into offsets, pattern_enum_kernel<true>
// recomputes the masks and writes every candidate at  tile offset + wave prefix over the lanes + rank inside the lane.
namespace {

// The sequence filters on one site; wh / wl = its bases on the forward genome from the start on, ps = the protospacer's bits
// of this strand.  G/C stay G/C under the complement, a T of the guide is an A of the window on '-', and a run is as long
// read backwards - so neither plane is reversed.  The bits outside ps are 0 in y: they neither start nor extend a run.
__device__ __forceinline__ bool pattern_sequence_ok(const PatEnumArgs &a, uint32_t wh, uint32_t wl, uint32_t ps, bool rev)
{
    const uint32_t gc = (uint32_t)__popc((wh ^ wl) & ps);
    if (gc < a.gc_min || gc > a.gc_max) return false;
    if (a.max_t_run) {
        uint32_t y = (rev ? ~(wh | wl) : wh & wl) & ps;                // T of the guide
        for (uint32_t i = 0; i < a.max_t_run && y; ++i) y &= y >> 1;  // every step shortens every run by one
        if (y) return false;                                          // a run of more than max_t_run is left
    }
    return true;
}

// Which of the 32 starts from global position `base` on lie in the ranges: the first range that ends behind base by binary
// search, then the ranges that begin before base + 32 (disjoint and not abutting: 16 at the most).
__device__ __forceinline__ uint32_t pattern_range_mask(const PatEnumArgs &a, uint32_t base)
{
    uint32_t lo = 0, hi = a.n_ranges;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (a.ranges[mid].y <= base) lo = mid + 1; else hi = mid;
    }
    uint32_t m = 0;
    for (uint32_t k = lo; k < a.n_ranges; ++k) {
        const uint2 r = a.ranges[k];  // (r.y > base)
        if ((uint64_t)r.x >= (uint64_t)base + 32u) break;
        const uint32_t s = r.x > base ? r.x - base : 0u;          // 0 .. 31
        const uint32_t e = r.y - base < 32u ? r.y - base : 32u;   // s + 1 .. 32
        m |= (e < 32u ? (1u << e) - 1u : ~0u) & ~((1u << s) - 1u);
    }
    return m;
}

}  // namespace

template <bool kWrite, bool kTargets>
__global__ __launch_bounds__(kWave *kWavesPerGroup) void pattern_enum_kernel(const PatEnumArgs a)
{
    const uint32_t lane = threadIdx.x % kWave;
    const uint32_t item = blockIdx.x * kWavesPerGroup + threadIdx.x / kWave;  // wave-uniform
    if (item >= a.n_work) return;
    const uint32_t tile = a.work ? a.work[item] : item;
    uint32_t H0, H1, L0, L1, mf, mr;
    pattern_words(a, tile, lane, H0, H1, L0, L1, &mf, &mr);
    mf &= a.keep_fwd;
    mr &= a.keep_rev;
    const uint32_t base_pos = a.first_pos + tile * (uint32_t)kTileBases + lane * 32u;
    if (kTargets) {
        const uint32_t in = pattern_range_mask(a, base_pos);
        mf &= in;
        mr &= in;
    }
    // ---- per-site tests, only where one is asked for (a.filter is wave-uniform): set bit by set bit ----
    if (a.filter) {
        for (uint32_t m = mf | mr; m; m &= m - 1u) {
            const uint32_t b = (uint32_t)__builtin_ctz(m), bit = 1u << b;
            const uint32_t wh = funnel(H1, H0, b), wl = funnel(L1, L0, b);
            if ((mf & bit) && !pattern_sequence_ok(a, wh, wl, a.ps_fwd, false)) mf &= ~bit;
            if ((mr & bit) && !pattern_sequence_ok(a, wh, wl, a.ps_rev, true)) mr &= ~bit;
        }
    }
    // ---- rank: tile offset + wave prefix over the lanes + order inside the lane ----
    uint32_t total;
    const uint32_t before = wave_exclusive((uint32_t)__popc(mf) + (uint32_t)__popc(mr), lane, &total);
    if (!kWrite) {
        if (lane == 0) a.tile_count[item] = total;
        return;
    }
    if (total == 0) return;
    unsigned long long at = a.tile_off[item] + before;
    uint32_t c = 0, c_end = 0;  // the contig of the lane's last candidate: [.., c_end) in global positions
    for (uint32_t m = mf | mr; m; m &= m - 1u) {
        const uint32_t b = (uint32_t)__builtin_ctz(m), bit = 1u << b;
        const uint32_t pos = base_pos + b;
        if (pos >= c_end) {  // c = the last contig that starts at or before pos (an N-free site lies inside one contig)
            uint32_t lo = 0, hi = a.n_contigs;
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (a.contig_off[mid] <= pos) lo = mid + 1; else hi = mid;
            }
            c = lo ? lo - 1u : 0u;
            c_end = a.contig_end[c];
        }
        const uint32_t wh = funnel(H1, H0, b), wl = funnel(L1, L0, b);
        const uint32_t rel = pos - a.contig_off[c];
        // (at < n_out whenever both passes see the same planes: the test keeps a write inside the result if not)
        if ((mf & bit) && at < a.n_out) {
            a.codes[at] = (unsigned long long)(wh & a.len_mask) << 32 | (wl & a.len_mask);
            a.loci[at] = make_uint4(c, rel, 0u, 0u);
        }
        at += (mf & bit) ? 1u : 0u;
        if ((mr & bit) && at < a.n_out) {
            a.codes[at] = (unsigned long long)pattern_revcomp_plane(wh, a.len) << 32 | pattern_revcomp_plane(wl, a.len);
            a.loci[at] = make_uint4(c, rel, 1u, 0u);
        }
        at += (mr & bit) ? 1u : 0u;
    }
}

// ---- launches ----------------------------------------------------------------------------------------------------------
hipError_t launch_pattern_count(const PatternArgs &args, int n_cus, hipStream_t stream)
{
    if (args.n_tiles == 0 || args.n_guides == 0) return hipSuccess;
    hipLaunchKernelGGL(pattern_count_kernel, cell_grid(args.n_tiles, n_cus), dim3(kWave * kWavesPerGroup), 0, stream, args);
    return hipGetLastError();
}

hipError_t launch_pattern_write(const PatternArgs &args, int n_cus, hipStream_t stream)
{
    if (args.n_tiles == 0 || args.n_guides == 0) return hipSuccess;
    hipLaunchKernelGGL(pattern_write_kernel, cell_grid(args.n_tiles, n_cus), dim3(kWave * kWavesPerGroup), 0, stream, args);
    return hipGetLastError();
}

hipError_t launch_pattern_write_scored(const PatternArgs &args, const PatScoreArgs &score, int n_cus, hipStream_t stream)
{
    if (args.n_tiles == 0 || args.n_guides == 0) return hipSuccess;
    hipLaunchKernelGGL(pattern_write_scored_kernel, cell_grid(args.n_tiles, n_cus), dim3(kWave * kWavesPerGroup), 0, stream, args, score);
    return hipGetLastError();
}

hipError_t launch_pattern_select(const PatSelectArgs &args, hipStream_t stream)
{
    if (args.n_guides == 0) return hipSuccess;
    hipLaunchKernelGGL(pattern_select_kernel, dim3(args.n_guides), dim3(kWave * kWavesPerGroup), 0, stream, args);
    return hipGetLastError();
}

hipError_t launch_pattern_select_walk(const PatSelectArgs &args, hipStream_t stream)
{
    if (args.n_guides == 0) return hipSuccess;
    hipLaunchKernelGGL(pattern_select_walk_kernel, dim3(args.n_guides), dim3(kWave * kWavesPerGroup), 0, stream, args);
    return hipGetLastError();
}

// work item i is wave i, as launch_enum
hipError_t launch_pattern_enum(const PatEnumArgs &args, bool write, hipStream_t stream)
{
    if (args.n_work == 0) return hipSuccess;
    const dim3 grid((args.n_work + kWavesPerGroup - 1) / kWavesPerGroup), block(kWave * kWavesPerGroup);
    const bool targets = args.ranges != nullptr;
    if (write) {
        if (targets) hipLaunchKernelGGL((pattern_enum_kernel<true, true>), grid, block, 0, stream, args);
        else hipLaunchKernelGGL((pattern_enum_kernel<true, false>), grid, block, 0, stream, args);
    } else {
        if (targets) hipLaunchKernelGGL((pattern_enum_kernel<false, true>), grid, block, 0, stream, args);
        else hipLaunchKernelGGL((pattern_enum_kernel<false, false>), grid, block, 0, stream, args);
    }
    return hipGetLastError();
}

}  // namespace vsc
