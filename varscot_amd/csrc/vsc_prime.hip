// vsc_prime.hip - prime-editing guide design on the device: prime_rows_kernel over loci (vsc_loci_prime,
// vsc_guides_prime, vsc_pattern_guides_prime), prime_pairs_kernel<kWrite> over the rows it left (the two passes behind the pairs,
// the coverage and the pairs by flag), prime_filter_kernel<kWrite> over a candidate list (the two passes of
// vsc_guides_filter_prime).  The class of a candidate, its context, its primer binding site, its join with the edits and the
// filter's rule are prime_context, prime_pbs, prime_walk and prime_keep of vsc_prime.h - the functions vsc_prime_site_text and
// the stand-alone check call on the host.
//
// The shapes are those of vsc_edit.hip.  The rows and the filter kernel take one candidate per lane and step: one 16-byte locus
// load, the bounds tests in the order of the classes (every index checked against its array's length before use), the context
// as a 64-bit window per plane out of up to three consecutive words of hi, lo and nm, reversed and complemented on '-'.  The
// 20 stability weights a lane indexes by its own letters lie in LDS; the loop over the primer binding site takes pbs_max steps
// in every lane.  A lane asks the occupancy bitmap for the (at most two) cells its reach touches before it searches the edits:
// a lower bound over their global positions (log2(n_e) dependent loads) and a walk over the reach.  Integers only: no MFMA, no
// floating point, no LDS but the weights and the counters, no atomics but the counters and the coverage (integer add and min,
// which commute).
#include "vsc_internal.h"
#include "vsc_device.h"

namespace vsc {

namespace {

constexpr int kPrimeThreads = kWave * kWavesPerGroup;
constexpr uint32_t kPrimeWeights = 20;  // mono[4], di[16]
static_assert(kEditTile % kWave == 0, "a tile is a whole number of steps of one wave");

// the weights a lane indexes, out of the kernel's arguments into LDS (wave-uniform reads, one store per weight)
__device__ __forceinline__ void prime_stage_weights(const PrimeShape &s, int32_t *w)
{
    if (threadIdx.x < 4u) w[threadIdx.x] = s.mono[threadIdx.x];
    else if (threadIdx.x < kPrimeWeights) w[threadIdx.x] = s.di[threadIdx.x - 4u];
}

// candidate r: its class; *v = (pbs, n_pairs), the undefined pair unless the class is kEffDefined
__device__ __forceinline__ uint32_t prime_candidate(const EffPlanes &g, const PrimeShape &s, const PrimeEdits &e, const int32_t *w, const uint4 r,
                                                    uint2 *v)
{
    uint64_t ch = 0, cl = 0;
    const uint32_t cls = prime_context(g, s, r.x, r.y, r.z, &ch, &cl);
    if (cls != kEffDefined) {
        *v = make_uint2(kPrimeUndefined, kPrimeUndefined);
        return cls;
    }
    const uint32_t pbs = prime_pbs(ch, cl, s, w, w + 4);
    const uint32_t g0 = g.contig_off[r.x] + prime_first_forward(r.y, r.z, s);  // (defined: r.x is a contig)
    const uint32_t pairs = prime_walk(s, e, ch, cl, r.x, g0, r.z, pbs, [](uint32_t, uint32_t, uint32_t, uint64_t, uint64_t) {});
    *v = make_uint2(pbs, pairs);
    return cls;
}

// exclusive prefix of v over the lanes of the wave; *total = the wave's sum (cross-lane moves, no LDS memory)
__device__ __forceinline__ uint32_t prime_wave_exclusive(uint32_t v, uint32_t lane, uint32_t *total)
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

// out[i] = (pbs, n_pairs) of loci[i], grid-stride over the 64-bit count in steps of whole waves; one coalesced 8-byte store per
// lane.  The classes, the candidates with a pair and the weak candidates are counted per wave (a ballot per counter and step),
// added per workgroup in LDS and go out with one atomic add per counter and workgroup.
__global__ __launch_bounds__(kPrimeThreads) void prime_rows_kernel(const PrimeArgs a)
{
    __shared__ unsigned long long s_count[kPrimeCounts];
    __shared__ int32_t s_w[kPrimeWeights];
    if (threadIdx.x < kPrimeCounts) s_count[threadIdx.x] = 0;
    prime_stage_weights(a.shape, s_w);
    block_sync();
    const uint32_t lane = threadIdx.x % kWave;
    const unsigned long long stride = (unsigned long long)gridDim.x * kPrimeThreads;
    uint32_t seen[kPrimeCounts] = {};  // wave-uniform
    const unsigned long long first = (unsigned long long)blockIdx.x * kPrimeThreads + threadIdx.x;
    uint4 ahead = first < a.n ? a.loci[first] : make_uint4(0u, 0u, 0u, 0u);  // the next step's locus is on its way during a step
    for (unsigned long long base = first - lane; base < a.n; base += stride) {
        const unsigned long long i = base + lane;
        const bool live = i < a.n;
        const uint4 r = ahead;
        if (i + stride < a.n) ahead = a.loci[i + stride];
        uint32_t cls = kEffClasses;
        bool with_pair = false, weak = false;
        if (live) {
            uint2 v;
            cls = prime_candidate(a.g, a.shape, a.edits, s_w, r, &v);
            with_pair = cls == kEffDefined && v.y != 0u;
            weak = cls == kEffDefined && (v.x >> 16 & 1u);
            a.out[i] = v;
        }
#pragma unroll
        for (uint32_t k = 0; k < kEffClasses; ++k) seen[k] += (uint32_t)__popcll(__ballot(cls == k));
        seen[kEffClasses] += (uint32_t)__popcll(__ballot(with_pair));
        seen[kEffClasses + 1] += (uint32_t)__popcll(__ballot(weak));
    }
    if (lane == 0) {
#pragma unroll
        for (uint32_t k = 0; k < kPrimeCounts; ++k)
            if (seen[k]) atomicAdd(&s_count[k], (unsigned long long)seen[k]);
    }
    block_sync();
    if (threadIdx.x < kPrimeCounts && s_count[threadIdx.x]) atomicAdd(&a.stats[threadIdx.x], s_count[threadIdx.x]);
}

// kWrite = false: tile_count[i] = the pairs of tile i - n_pairs over its candidates, read from the rows.  kWrite = true: every
// pair to tile_off[i] + the pairs of the tile's earlier steps + the pairs of the lanes below (an exclusive scan over the wave) +
// its place among the candidate's own, which is the order of the walk over the edits: ascending (candidate, edit).  Only a lane
// with pairs reads its locus and its context again and rebuilds E.  One wave per tile of kEditTile candidates; no append
// cursor: the bytes depend on the rows, the loci, the planes and the edits only.  The coverage is taken here: one integer add
// and one integer min per pair; the pairs by flag are counted per lane, added over the wave and go out with one atomic add per
// flag and wave.
template <bool kWrite> __global__ __launch_bounds__(kPrimeThreads) void prime_pairs_kernel(const PrimePairArgs a)
{
    const uint32_t lane = threadIdx.x % kWave;
    const uint32_t item = blockIdx.x * kWavesPerGroup + threadIdx.x / kWave;  // wave-uniform
    if (item >= a.n_work) return;
    const unsigned long long first = (unsigned long long)item * kEditTile;
    unsigned long long at = kWrite ? a.tile_off[item] : 0;
    uint32_t count = 0;
    uint32_t by_flag[kPrimeFlags] = {};
    for (uint32_t step = 0; step < kEditTile / kWave; ++step) {
        const unsigned long long base = first + (unsigned long long)step * kWave;
        if (base >= a.n) break;
        const unsigned long long i = base + lane;
        uint2 v = make_uint2(0u, 0u);
        if (i < a.n) v = a.rows[i];
        const uint32_t mine = v.y == kPrimeUndefined ? 0u : v.y;
        uint32_t total;
        const uint32_t before = prime_wave_exclusive(mine, lane, &total);
        if (kWrite) {
            if (mine) {
                const uint4 r = a.loci[i];
                uint64_t ch = 0, cl = 0;
                // (a row with pairs: the class is defined, r.x is a contig)
                if (prime_context(a.g, a.shape, r.x, r.y, r.z, &ch, &cl) == kEffDefined) {
                    const uint32_t g0 = a.g.contig_off[r.x] + prime_first_forward(r.y, r.z, a.shape);
                    unsigned long long o = at + before;
                    const unsigned long long end = o + mine;  // (the rows' count bounds what this lane may write)
                    prime_walk(a.shape, a.edits, ch, cl, r.x, g0, r.z, v.x, [&](uint32_t k, uint32_t info, uint32_t ext, uint64_t, uint64_t) {
                        if (o >= end) return;
                        if (a.pairs) a.pairs[o] = make_uint4((uint32_t)i, k, info, ext);
                        ++o;
                        if (a.cov_count) {
                            atomicAdd(&a.cov_count[k], 1u);
                            atomicMin(&a.cov_min[k], info & 0xFFu);
                        }
#pragma unroll
                        for (uint32_t b = 0; b < kPrimeFlags; ++b) by_flag[b] += info >> (24u + b) & 1u;
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
        for (uint32_t b = 0; b < kPrimeFlags; ++b) {
            uint32_t sum = by_flag[b];
#pragma unroll
            for (int d = kWave / 2; d >= 1; d >>= 1) sum += (uint32_t)__shfl_xor((int)sum, d, kWave);
            if (lane == 0 && sum) atomicAdd(&a.flag_count[b], (unsigned long long)sum);
        }
    }
}

// kWrite = false: tile_count[i] = the candidates of tile work[i] that pass FILTER (prime_keep).  kWrite = true: the same test
// again, every survivor's code and locus to tile_off[i] + its rank in the tile - the input's order.  One wave per tile of
// kEditTile candidates; the rank inside a step is the survivors in the lanes below (a ballot), no atomic.
template <bool kWrite> __global__ __launch_bounds__(kPrimeThreads) void prime_filter_kernel(const PrimeFilterArgs a)
{
    __shared__ int32_t s_w[kPrimeWeights];
    prime_stage_weights(a.shape, s_w);
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
            const uint32_t cls = prime_candidate(a.g, a.shape, a.edits, s_w, r, &v);
            keep = prime_keep(cls, v.x, v.y, a.edits.n != 0u, a.allow_weak != 0u);
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

hipError_t launch_prime_rows(const PrimeArgs &args, int n_cus, uint32_t groups_per_cu, hipStream_t stream)
{
    if (args.n == 0) return hipSuccess;
    // kPrimeGroupsPerCu = 28 workgroups of 4 waves per CU; fewer when the candidates do not need them.  The kernel's 106 SGPRs admit
    // 7 waves per SIMD, so 7 workgroups per CU are resident at once and the grid is four rounds of them: measured against 7, 8 (what
    // launch_edit_rows starts), 14, 16, 21, 42 and 56 per CU in one process (vsc_debug_prime_groups_per_cu), the
    // time falls with the number of workgroups - shorter lanes even out the searching waves - and by 2 to 3 % from 28 to 56.  The
    // loop is grid-stride: the cap changes the schedule and no result.
    const unsigned long long want = (args.n + kPrimeThreads - 1) / kPrimeThreads;
    const unsigned long long cap = (unsigned long long)(n_cus > 0 ? n_cus : 256) * (groups_per_cu ? groups_per_cu : kPrimeGroupsPerCu);
    const dim3 grid((uint32_t)(want < cap ? want : cap)), block(kPrimeThreads);
    hipLaunchKernelGGL(prime_rows_kernel, grid, block, 0, stream, args);
    return hipGetLastError();
}

hipError_t launch_prime_pairs(const PrimePairArgs &args, bool write, hipStream_t stream)
{
    if (args.n_work == 0) return hipSuccess;
    const dim3 grid((args.n_work + kWavesPerGroup - 1) / kWavesPerGroup), block(kPrimeThreads);
    if (write) hipLaunchKernelGGL((prime_pairs_kernel<true>), grid, block, 0, stream, args);
    else hipLaunchKernelGGL((prime_pairs_kernel<false>), grid, block, 0, stream, args);
    return hipGetLastError();
}

hipError_t launch_prime_filter(const PrimeFilterArgs &args, bool write, hipStream_t stream)
{
    if (args.n_work == 0) return hipSuccess;
    const dim3 grid((args.n_work + kWavesPerGroup - 1) / kWavesPerGroup), block(kPrimeThreads);
    if (write) hipLaunchKernelGGL((prime_filter_kernel<true>), grid, block, 0, stream, args);
    else hipLaunchKernelGGL((prime_filter_kernel<false>), grid, block, 0, stream, args);
    return hipGetLastError();
}

}  // namespace vsc
