// vsc_hdr.hip - HDR knock-in design on the device: hdr_rows_kernel over loci (vsc_loci_hdr, vsc_guides_hdr,
// vsc_pattern_guides_hdr), hdr_pairs_kernel<kWrite> over the rows it left (the two passes behind the pairs, the coverage and the
// pairs by flag), hdr_filter_kernel<kWrite> over a candidate list (the two passes of vsc_guides_filter_hdr).  The class of a
// candidate, its context, the read of an edit, the site the nuclease sees, the block test, the substitution search, ALLOWED
// against the CDS, the join with the edits and the filter's rule are hdr_context, hdr_pair, hdr_allowed_cds, hdr_walk and
// hdr_keep of vsc_hdr.h - the functions vsc_hdr_site_text and the stand-alone check call on the host.
//
// The shapes are those of vsc_prime.hip.  The rows and the filter kernel take one candidate per lane and step: one 16-byte locus
// load, the bounds tests in the order of the classes, the context as a 64-bit window per plane, reversed and complemented on
// '-'.  A lane asks the occupancy bitmap for the (at most two) cells its reach touches before it searches the edits: a lower
// bound over their global positions and a walk over the reach.  The CDS is touched only by a lane that holds a pair which is in
// reach and not BLOCKED: a lower bound over the segments' starts, the segment as scalars, the codon's three positions.  CODE
// and the PAM's letter sets, which a lane indexes by its own letters, lie in LDS.  Integers only: no MFMA, no floating point, no
// LDS but the two tables and the counters, no atomics but the counters and the coverage (integer add and min, which commute).
#include "vsc_internal.h"
#include "vsc_device.h"

namespace vsc {

namespace {

constexpr int kHdrThreads = kWave * kWavesPerGroup;
static_assert(kEditTile % kWave == 0, "a tile is a whole number of steps of one wave");
static_assert(kHdrThreads >= 64 + (int)kHdrMaxPam, "the workgroup's first lanes copy CODE and the PAM's sets, one entry each");

// CODE and pam_accept from the kernel's arguments to LDS, one entry per lane; the caller synchronises
__device__ __forceinline__ void hdr_tables_to_lds(const HdrTables &t, uint8_t *s_code, uint32_t *s_accept)
{
    if (threadIdx.x < 64u) s_code[threadIdx.x] = t.aa[threadIdx.x];
    else if (threadIdx.x < 64u + kHdrMaxPam) s_accept[threadIdx.x - 64u] = t.accept[threadIdx.x - 64u];
}

// The join of the defined candidate r (planes ch, cl) with the edits: emit(k, info, block) per pair in reach.  ALLOWED asks the
// CDS when the call has one.
template <class Emit>
__device__ __forceinline__ uint32_t hdr_join(const EffPlanes &g, const HdrShape &s, const PrimeEdits &e, const CdsView &cds, uint32_t have_cds,
                                             const uint8_t *code, const uint32_t *accept, const uint4 r, uint64_t ch, uint64_t cl, Emit &&emit)
{
    const uint32_t g0 = g.contig_off[r.x] + hdr_first_forward(r.y, r.z, s);  // (defined: r.x is a contig)
    const bool noncoding = (s.flags & kHdrSubNoncoding) != 0u;
    uint32_t first = kCdsNone;  // the candidate's first segment: searched once, by the first pair that asks the CDS
    return hdr_walk(
        s, accept, e, ch, cl, r.x, g0, r.z,
        [&](uint32_t at, uint32_t ge, uint32_t del) -> uint32_t {
            if (!have_cds) return kHdrAnyLetter;
            return hdr_allowed_cds(g, cds, code, noncoding, hdr_forward(s, g0, r.z, at), r.z, ge, del, g0, &first);
        },
        emit);
}

// candidate r: its class; *v = (n_pairs, n_usable), the undefined pair unless the class is kEffDefined
__device__ __forceinline__ uint32_t hdr_candidate(const EffPlanes &g, const HdrShape &s, const PrimeEdits &e, const CdsView &cds, uint32_t have_cds,
                                                  const uint8_t *code, const uint32_t *accept, const uint4 r, uint2 *v)
{
    uint64_t ch = 0, cl = 0;
    const uint32_t cls = hdr_context(g, s, r.x, r.y, r.z, &ch, &cl);
    if (cls != kEffDefined) {
        *v = make_uint2(kHdrUndefined, kHdrUndefined);
        return cls;
    }
    uint32_t usable = 0;
    const uint32_t pairs =
        hdr_join(g, s, e, cds, have_cds, code, accept, r, ch, cl, [&](uint32_t, uint32_t info, uint32_t) { usable += ~info >> (24u + 5u) & 1u; });
    *v = make_uint2(pairs, usable);
    return cls;
}

// exclusive prefix of v over the lanes of the wave; *total = the wave's sum (cross-lane moves, no LDS memory)
__device__ __forceinline__ uint32_t hdr_wave_exclusive(uint32_t v, uint32_t lane, uint32_t *total)
{
    uint32_t s = v;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)s, d, kWave);
        if (lane >= (uint32_t)d) s += o;
    }
    *total = (uint32_t)__shfl((int)s, kWave - 1, kWave);
    return s - v;
}

}  // namespace

// out[i] = (n_pairs, n_usable) of loci[i], grid-stride over the 64-bit count in steps of whole waves; one coalesced 8-byte store
// per lane.  The classes, the candidates with a pair and those with a usable pair are counted per wave (a ballot per counter and
// step), added per workgroup in LDS and go out with one atomic add per counter and workgroup.
__global__ __launch_bounds__(kHdrThreads) void hdr_rows_kernel(const HdrArgs a)
{
    __shared__ unsigned long long s_count[kHdrCounts];
    __shared__ uint8_t s_code[64];
    __shared__ uint32_t s_accept[kHdrMaxPam];
    if (threadIdx.x < kHdrCounts) s_count[threadIdx.x] = 0;
    hdr_tables_to_lds(a.tabs, s_code, s_accept);
    block_sync();
    const uint32_t lane = threadIdx.x % kWave;
    const unsigned long long stride = (unsigned long long)gridDim.x * kHdrThreads;
    uint32_t seen[kHdrCounts] = {};  // wave-uniform
    const unsigned long long first = (unsigned long long)blockIdx.x * kHdrThreads + threadIdx.x;
    uint4 ahead = first < a.n ? a.loci[first] : make_uint4(0u, 0u, 0u, 0u);  // the next step's locus is on its way during a step
    for (unsigned long long base = first - lane; base < a.n; base += stride) {
        const unsigned long long i = base + lane;
        const bool live = i < a.n;
        const uint4 r = ahead;
        if (i + stride < a.n) ahead = a.loci[i + stride];
        uint32_t cls = kEffClasses;
        bool with_pair = false, with_usable = false;
        if (live) {
            uint2 v;
            cls = hdr_candidate(a.g, a.shape, a.edits, a.cds, a.have_cds, s_code, s_accept, r, &v);
            with_pair = cls == kEffDefined && v.x != 0u;
            with_usable = cls == kEffDefined && v.y != 0u;
            a.out[i] = v;
        }
#pragma unroll
        for (uint32_t k = 0; k < kEffClasses; ++k) seen[k] += (uint32_t)__popcll(__ballot(cls == k));
        seen[kEffClasses] += (uint32_t)__popcll(__ballot(with_pair));
        seen[kEffClasses + 1] += (uint32_t)__popcll(__ballot(with_usable));
    }
    if (lane == 0) {
#pragma unroll
        for (uint32_t k = 0; k < kHdrCounts; ++k)
            if (seen[k]) atomicAdd(&s_count[k], (unsigned long long)seen[k]);
    }
    block_sync();
    if (threadIdx.x < kHdrCounts && s_count[threadIdx.x]) atomicAdd(&a.stats[threadIdx.x], s_count[threadIdx.x]);
}

// kWrite = false: tile_count[i] = the pairs of tile i - n_pairs over its candidates, read from the rows.  kWrite = true: every
// pair to tile_off[i] + the pairs of the tile's earlier steps + the pairs of the lanes below (an exclusive scan over the wave) +
// its place among the candidate's own, which is the order of the walk over the edits: ascending (candidate, edit).  Only a lane
// with pairs reads its locus and its context again and judges its pairs again.  One wave per tile of kEditTile candidates; no
// append cursor: the bytes depend on the rows, the loci, the planes, the edits and the CDS only.  The coverage is taken here: one
// integer add and one integer min per usable pair; the pairs by flag are counted per lane, added over the wave and go out with
// one atomic add per flag and wave.
template <bool kWrite> __global__ __launch_bounds__(kHdrThreads) void hdr_pairs_kernel(const HdrPairArgs a)
{
    __shared__ uint8_t s_code[64];
    __shared__ uint32_t s_accept[kHdrMaxPam];
    if (kWrite) {
        hdr_tables_to_lds(a.tabs, s_code, s_accept);
        block_sync();
    }
    const uint32_t lane = threadIdx.x % kWave;
    const uint32_t item = blockIdx.x * kWavesPerGroup + threadIdx.x / kWave;  // wave-uniform
    if (item >= a.n_work) return;
    const unsigned long long first = (unsigned long long)item * kEditTile;
    unsigned long long at = kWrite ? a.tile_off[item] : 0;
    uint32_t count = 0;
    uint32_t by_flag[kHdrFlags] = {};
    for (uint32_t step = 0; step < kEditTile / kWave; ++step) {
        const unsigned long long base = first + (unsigned long long)step * kWave;
        if (base >= a.n) break;
        const unsigned long long i = base + lane;
        uint2 v = make_uint2(0u, 0u);
        if (i < a.n) v = a.rows[i];
        const uint32_t mine = v.x == kHdrUndefined ? 0u : v.x;
        uint32_t total;
        const uint32_t before = hdr_wave_exclusive(mine, lane, &total);
        if (kWrite) {
            if (mine) {
                const uint4 r = a.loci[i];
                uint64_t ch = 0, cl = 0;
                // (a row with pairs: the class is defined, r.x is a contig)
                if (hdr_context(a.g, a.shape, r.x, r.y, r.z, &ch, &cl) == kEffDefined) {
                    unsigned long long o = at + before;
                    const unsigned long long end = o + mine;  // (the rows' count bounds what this lane may write)
                    hdr_join(a.g, a.shape, a.edits, a.cds, a.have_cds, s_code, s_accept, r, ch, cl, [&](uint32_t k, uint32_t info, uint32_t block) {
                        if (o >= end) return;
                        if (a.pairs) a.pairs[o] = make_uint4((uint32_t)i, k, info, block);
                        ++o;
                        if (a.cov_count && !(info >> (24u + 5u) & 1u)) {
                            atomicAdd(&a.cov_count[k], 1u);
                            atomicMin(&a.cov_min[k], info & 0x3Fu);
                        }
#pragma unroll
                        for (uint32_t b = 0; b < kHdrFlags; ++b) by_flag[b] += info >> (24u + b) & 1u;
                    });
                }
            }
            at += total;
        } else {
            count += total;
        }
    }
    if (!kWrite) {
        if (lane == 0) a.tile_count[item] = count;
        return;
    }
    if (a.flag_count) {
#pragma unroll
        for (uint32_t b = 0; b < kHdrFlags; ++b) {
            uint32_t sum = by_flag[b];
#pragma unroll
            for (int d = kWave / 2; d >= 1; d >>= 1) sum += (uint32_t)__shfl_xor((int)sum, d, kWave);
            if (lane == 0 && sum) atomicAdd(&a.flag_count[b], (unsigned long long)sum);
        }
    }
}

// kWrite = false: tile_count[i] = the candidates of tile work[i] that pass FILTER (hdr_keep).  kWrite = true: the same test
// again, every survivor's code and locus to tile_off[i] + its rank in the tile - the input's order.  One wave per tile of
// kEditTile candidates; the rank inside a step is the survivors in the lanes below (a ballot), no atomic.
template <bool kWrite> __global__ __launch_bounds__(kHdrThreads) void hdr_filter_kernel(const HdrFilterArgs a)
{
    __shared__ uint8_t s_code[64];
    __shared__ uint32_t s_accept[kHdrMaxPam];
    hdr_tables_to_lds(a.tabs, s_code, s_accept);
    block_sync();
    const uint32_t lane = threadIdx.x % kWave;
    const uint32_t item = blockIdx.x * kWavesPerGroup + threadIdx.x / kWave;  // wave-uniform
    if (item >= a.n_work) return;
    const uint32_t tile = a.work ? a.work[item] : item;
    const unsigned long long first = (unsigned long long)tile * kEditTile;
    unsigned long long at = kWrite ? a.tile_off[item] : 0;
    uint32_t count = 0;
    for (uint32_t step = 0; step < kEditTile / kWave; ++step) {
        const unsigned long long base = first + (unsigned long long)step * kWave;
        if (base >= a.n) break;
        const unsigned long long i = base + lane;
        bool keep = false;
        uint4 r = make_uint4(0u, 0u, 0u, 0u);
        if (i < a.n) {
            r = a.in_loci[i];
            uint2 v;
            const uint32_t cls = hdr_candidate(a.g, a.shape, a.edits, a.cds, a.have_cds, s_code, s_accept, r, &v);
            keep = hdr_keep(cls, v.x, v.y, a.edits.n != 0u, a.allow_open != 0u);
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

hipError_t launch_hdr_rows(const HdrArgs &args, int n_cus, uint32_t groups_per_cu, hipStream_t stream)
{
    if (args.n == 0) return hipSuccess;
    // kHdrGroupsPerCu workgroups of 4 waves per CU, as launch_prime_rows starts them (the same context, join and launch shape);
    // fewer when the candidates do not need them.  The loop is grid-stride: the cap changes the schedule and no result.
    const unsigned long long want = (args.n + kHdrThreads - 1) / kHdrThreads;
    const unsigned long long cap = (unsigned long long)(n_cus > 0 ? n_cus : 256) * (groups_per_cu ? groups_per_cu : kHdrGroupsPerCu);
    const dim3 grid((uint32_t)(want < cap ? want : cap)), block(kHdrThreads);
    hipLaunchKernelGGL(hdr_rows_kernel, grid, block, 0, stream, args);
    return hipGetLastError();
}

hipError_t launch_hdr_pairs(const HdrPairArgs &args, bool write, hipStream_t stream)
{
    if (args.n_work == 0) return hipSuccess;
    const dim3 grid((args.n_work + kWavesPerGroup - 1) / kWavesPerGroup), block(kHdrThreads);
    if (write) hipLaunchKernelGGL((hdr_pairs_kernel<true>), grid, block, 0, stream, args);
    else hipLaunchKernelGGL((hdr_pairs_kernel<false>), grid, block, 0, stream, args);
    return hipGetLastError();
}

hipError_t launch_hdr_filter(const HdrFilterArgs &args, bool write, hipStream_t stream)
{
    if (args.n_work == 0) return hipSuccess;
    const dim3 grid((args.n_work + kWavesPerGroup - 1) / kWavesPerGroup), block(kHdrThreads);
    if (write) hipLaunchKernelGGL((hdr_filter_kernel<true>), grid, block, 0, stream, args);
    else hipLaunchKernelGGL((hdr_filter_kernel<false>), grid, block, 0, stream, args);
    return hipGetLastError();
}

}  // namespace vsc
