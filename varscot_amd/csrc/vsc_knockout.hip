// vsc_knockout.hip - knock-out design on the device: knockout_rows_kernel over loci (vsc_loci_knockout,
// vsc_guides_knockout, vsc_pattern_guides_knockout) and knockout_filter_kernel<kWrite> over a candidate list (the two passes of
// vsc_guides_filter_knockout).  The cut, the coding-cut test, the cursor, both walks, the row and the filter's rule are the
// inline functions of vsc_knockout.h - the functions vsc_knockout_site_text and the stand-alone check call on the host.
//
// The rows kernel has two phases.  FIND, one candidate per lane and step: the cut out of the 16-byte locus, the occupancy bitmap
// (one bit per 256 positions; 95 % of a genome's candidates end here, with one 4-byte load that hits the L2), and only behind
// it the lower bound over the segments.  Undefined and non-coding lanes store their row at once.  WALK: a coding cut walks
// about 20 codons in each of two frames, and a wave's step holds anything from none to 64 of them (candidates are sorted by
// position, so the coding ones come in runs of an exon's length); so the coding lanes are compacted by ballot into a queue in
// LDS (candidate, segment, K: 12 bytes), and whenever the queue holds 64 entries they are drained with every lane busy; what
// is left when the grid-stride loop ends is drained once more.  The workgroup's queue is one slice per wave: a wave fills and
// drains its own, so no barrier stands in the loop (a queue shared by the four waves, with two barriers a step, was built first
// and measured slower than walking in place: DESIGN 4.37).
// Integers only: no MFMA, no floating point, no atomics but the counters and the coverage (integer add and min, which commute).
#include "vsc_internal.h"
#include "vsc_device.h"

namespace vsc {

namespace {

constexpr int kKoThreads = kWave * kWavesPerGroup;
// a wave's slice of the queue: a step adds at most kWave entries to fewer than kWave left over, and a whole 64 is read before
// the next step writes - a ring of 2 * kWave slots never overwrites an unread entry
constexpr uint32_t kKoQueue = 2u * kWave;
static_assert((kKoQueue & (kKoQueue - 1u)) == 0u, "the ring's index is a mask");
static_assert(kKoThreads >= 64, "the workgroup's first 64 lanes copy CODE, one letter each");
static_assert(kKoCounts <= kKoThreads, "one thread per counter");

// the wave-uniform counters of a drain
struct KoSeen {
    uint32_t ptc1 = 0, ptc2 = 0, nmd1 = 0, nmd2 = 0, unknown = 0, drains = 0, drained = 0;
};

// one queue entry per lane (live: this lane has one): both walks, the 16-byte row, the coverage, the counters by ballot
__device__ __forceinline__ void knockout_drain(const KoArgs &a, const uint8_t *code, bool live, uint32_t cand, uint32_t seg, uint32_t k, KoSeen &seen)
{
    uint32_t flags = 0;
    if (live) {
        const uint4 r = a.loci[cand];
        uint32_t gx = 0, row[4];
        (void)knockout_cut(a.g.contig_off, a.g.contig_end, a.g.n_contigs, a.shape, r.x, r.y, r.z, &gx);  // (queued: it is defined)
        knockout_finish(a.g, a.cds, a.tx, a.shape, code, gx, KoCut{seg, k}, row);
        a.out[cand] = make_uint4(row[0], row[1], row[2], row[3]);
        flags = row[2] >> 24;
        if (a.cov_count && (flags & (kKoNmd1 | kKoNmd2)) == (kKoNmd1 | kKoNmd2) && row[0] < a.n_tx) {
            atomicAdd(&a.cov_count[row[0]], 1u);
            atomicMin(&a.cov_min[row[0]], row[1] & 0x3FFFFFFFu);
        }
    }
    seen.ptc1 += (uint32_t)__popcll(__ballot(flags & kKoPtc1));
    seen.ptc2 += (uint32_t)__popcll(__ballot(flags & kKoPtc2));
    seen.nmd1 += (uint32_t)__popcll(__ballot(flags & kKoNmd1));
    seen.nmd2 += (uint32_t)__popcll(__ballot(flags & kKoNmd2));
    seen.unknown += (uint32_t)__popcll(__ballot(flags & kKoUnknownFlag));
    seen.drains += 1u;
    seen.drained += (uint32_t)__popcll(__ballot(live));
}

}  // namespace

// out[i] = ROW of loci[i]; step t of workgroup b covers candidates [(b + t gridDim.x) 256, + 256).  tail counts the entries a
// wave ever queued, head the entries it ever drained (registers, wave-uniform); entry e lies in slot e % kKoQueue of the wave's
// slice.  The lanes of a wave exchange the entries through LDS alone: DS operations of one wave execute in order (wave_sync).
// kQueue = false (vsc_debug_knockout_in_place, the measurement's other side): no queue, a coding lane walks where it lies; a
// "drain" is then a wave's step with a coding lane, and its fill the coding lanes of that step.
template <bool kQueue> __global__ __launch_bounds__(kKoThreads) void knockout_rows_kernel(const KoArgs a)
{
    __shared__ unsigned long long s_count[kKoCounts];
    __shared__ uint8_t s_code[64];
    __shared__ uint32_t s_cand[kWavesPerGroup][kKoQueue], s_seg[kWavesPerGroup][kKoQueue], s_k[kWavesPerGroup][kKoQueue];
    if (threadIdx.x < kKoCounts) s_count[threadIdx.x] = 0;
    if (threadIdx.x < 64) s_code[threadIdx.x] = a.code.aa[threadIdx.x];
    block_sync();
    const uint32_t lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    const unsigned long long stride = (unsigned long long)gridDim.x * kKoThreads;
    uint32_t n_defined = 0, n_undefined = 0, n_coding = 0, n_junction = 0, n_past = 0;  // wave-uniform
    KoSeen seen;
    uint32_t *const q_cand = s_cand[wave], *const q_seg = s_seg[wave], *const q_k = s_k[wave];
    uint32_t head = 0, tail = 0;
    for (unsigned long long base = (unsigned long long)blockIdx.x * kKoThreads; base < a.n; base += stride) {
        const unsigned long long i = base + threadIdx.x;
        const bool live = i < a.n;
        bool defined = false, coding = false, junction = false, past = false;
        KoCut cut{};
        if (live) {
            const uint4 r = a.loci[i];
            uint32_t gx = 0, row[4];
            defined = knockout_cut(a.g.contig_off, a.g.contig_end, a.g.n_contigs, a.shape, r.x, r.y, r.z, &gx);
            if (defined) {
                past = !knockout_occupied(a.bitmap, a.n_blocks, gx - 1u) && !knockout_occupied(a.bitmap, a.n_blocks, gx);
                if (!past) coding = knockout_find(a.cds, gx, &cut, &junction);
                if (!coding) knockout_noncoding(junction, row);
            } else {
                row[0] = row[1] = row[2] = row[3] = kKoUndefined;
            }
            if (!coding) a.out[i] = make_uint4(row[0], row[1], row[2], row[3]);
        }
        n_defined += (uint32_t)__popcll(__ballot(defined));
        n_undefined += (uint32_t)__popcll(__ballot(live && !defined));
        n_junction += (uint32_t)__popcll(__ballot(junction));
        n_past += (uint32_t)__popcll(__ballot(past));
        const uint64_t queued = __ballot(coding);
        const uint32_t n_queued = (uint32_t)__popcll(queued);
        n_coding += n_queued;
        if (!kQueue) {
            if (n_queued) knockout_drain(a, s_code, coding, (uint32_t)i, cut.seg, cut.k, seen);  // wave-uniform
            continue;
        }
        if (!n_queued) continue;  // wave-uniform
        if (coding) {
            const uint32_t slot = (tail + lanes_below(queued)) & (kKoQueue - 1u);
            q_cand[slot] = (uint32_t)i;  // (n <= 0xFFFFFFFE)
            q_seg[slot] = cut.seg;
            q_k[slot] = cut.k;
        }
        tail += n_queued;
        if (tail - head >= (uint32_t)kWave) {
            wave_sync();
            const uint32_t slot = (head + lane) & (kKoQueue - 1u);
            const uint32_t cand = q_cand[slot], seg = q_seg[slot], k = q_k[slot];
            wave_sync();
            head += kWave;
            knockout_drain(a, s_code, true, cand, seg, k, seen);
        }
    }
    // the rest of the wave's slice: fewer than 64 entries
    if (tail != head) {
        wave_sync();
        const bool live = lane < tail - head;
        const uint32_t slot = (head + lane) & (kKoQueue - 1u);
        knockout_drain(a, s_code, live, live ? q_cand[slot] : 0u, live ? q_seg[slot] : 0u, live ? q_k[slot] : 0u, seen);
    }
    if (lane == 0) {
        const uint32_t v[kKoCounts] = {n_defined, n_undefined, n_coding,  n_junction,   seen.ptc1,    seen.ptc2,
                                       seen.nmd1, seen.nmd2,   seen.unknown, n_past,    seen.drains,  seen.drained};
#pragma unroll
        for (uint32_t c = 0; c < kKoCounts; ++c)
            if (v[c]) atomicAdd(&s_count[c], (unsigned long long)v[c]);
    }
    block_sync();
    if (threadIdx.x < kKoCounts && s_count[threadIdx.x]) atomicAdd(&a.stats[threadIdx.x], s_count[threadIdx.x]);
}

// kWrite = false: tile_count[i] = the candidates of tile work[i] that pass FILTER (knockout_keep).  kWrite = true: the same
// test again, every survivor's code and locus to tile_off[i] + its rank in the tile - the input's order.  One wave per tile
// of kEditTile candidates; the rank inside a step is the survivors in the lanes below (a ballot), no atomic.  A candidate
// walks where it lies, and only when it is a coding cut that passes the tests on frac, edge, FIRST and LAST and the masks ask
// for a bit that a walk sets.
template <bool kWrite> __global__ __launch_bounds__(kKoThreads) void knockout_filter_kernel(const KoFilterArgs a)
{
    __shared__ uint8_t s_code[64];
    if (threadIdx.x < 64) s_code[threadIdx.x] = a.code.aa[threadIdx.x];
    block_sync();
    const uint32_t lane = threadIdx.x % kWave;
    const uint32_t item = blockIdx.x * kWavesPerGroup + threadIdx.x / kWave;  // wave-uniform
    if (item >= a.n_work) return;
    const uint32_t tile = a.work ? a.work[item] : item;
    const unsigned long long first = (unsigned long long)tile * kEditTile;
    unsigned long long at = kWrite ? a.tile_off[item] : 0;
    uint32_t count = 0;
    const bool walks = ((a.filter.require | a.filter.forbid) & kKoWalkFlags) != 0u;
    for (uint32_t step = 0; step < kEditTile / kWave; ++step) {
        const unsigned long long base = first + (unsigned long long)step * kWave;
        if (base >= a.n) break;
        const unsigned long long i = base + lane;
        bool keep = false;
        uint4 r = make_uint4(0u, 0u, 0u, 0u);
        if (i < a.n) {
            r = a.in_loci[i];
            uint32_t gx = 0, row[4];
            KoCut cut{};
            bool junction = false;
            if (knockout_cut(a.g.contig_off, a.g.contig_end, a.g.n_contigs, a.shape, r.x, r.y, r.z, &gx) &&
                (knockout_occupied(a.bitmap, a.n_blocks, gx - 1u) || knockout_occupied(a.bitmap, a.n_blocks, gx)) &&
                knockout_find(a.cds, gx, &cut, &junction)) {
                knockout_head(a.cds, a.tx, gx, cut, row);
                keep = knockout_keep_head(row, a.filter);
                if (keep && walks) {
                    knockout_finish(a.g, a.cds, a.tx, a.shape, s_code, gx, cut, row);
                    keep = knockout_keep(row, a.filter);
                }
            }
        }
        const uint64_t kept = __ballot(keep);
        if (kWrite) {
            if (keep) {
                const unsigned long long o = at + lanes_below(kept);
                a.codes[o] = a.in_codes[i];
                a.loci[o] = r;
            }
            at += (uint32_t)__popcll(kept);
        } else {
            count += (uint32_t)__popcll(kept);
        }
    }
    if (!kWrite && lane == 0) a.tile_count[item] = count;
}

hipError_t launch_knockout_rows(const KoArgs &args, int n_cus, uint32_t groups_per_cu, bool in_place, hipStream_t stream)
{
    if (args.n == 0) return hipSuccess;
    // 8 workgroups of 4 waves per CU fill every SIMD's 8 wave slots; fewer when the candidates do not need them (launch_effects_rows)
    const unsigned long long want = (args.n + kKoThreads - 1) / kKoThreads;
    const unsigned long long cap = (unsigned long long)(n_cus > 0 ? n_cus : 256) * (groups_per_cu ? groups_per_cu : kKoGroupsPerCu);
    const dim3 grid((uint32_t)(want < cap ? want : cap)), block(kKoThreads);
    if (in_place) hipLaunchKernelGGL((knockout_rows_kernel<false>), grid, block, 0, stream, args);
    else hipLaunchKernelGGL((knockout_rows_kernel<true>), grid, block, 0, stream, args);
    return hipGetLastError();
}

hipError_t launch_knockout_filter(const KoFilterArgs &args, bool write, hipStream_t stream)
{
    if (args.n_work == 0) return hipSuccess;
    const dim3 grid((args.n_work + kWavesPerGroup - 1) / kWavesPerGroup), block(kKoThreads);
    if (write) hipLaunchKernelGGL((knockout_filter_kernel<true>), grid, block, 0, stream, args);
    else hipLaunchKernelGGL((knockout_filter_kernel<false>), grid, block, 0, stream, args);
    return hipGetLastError();
}

}  // namespace vsc
