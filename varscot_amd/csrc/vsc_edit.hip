// vsc_edit.hip - base-editor windows on the device: edit_rows_kernel over loci (vsc_loci_edit, vsc_guides_edit,
// vsc_pattern_guides_edit), edit_pairs_kernel<kWrite> over the rows it left (the two passes behind the pairs and the coverage),
// edit_filter_kernel<kWrite> over a candidate list (the two passes of vsc_guides_filter_edit).  The class of a candidate, its
// site, its mask, its hits and the filter's rule are edit_site, edit_mask, edit_hits and edit_keep of vsc_edit.h - the
// functions vsc_edit_site_text and the stand-alone check call on the host.
//
// The rows and the filter kernel take one candidate per lane and step, as the kernels of vsc_mh.hip do: one 16-byte locus
// load, the bounds tests in the order of the classes (every index checked against its array's length before use), the site as
// a 64-bit window per plane out of up to two consecutive words of hi, lo and nm, reversed and complemented on '-'.  A lane
// searches the targets only when its mask is not 0: a lower bound over their global positions (log2(n_t) dependent loads) and a
// walk over at most win_len entries.  Integers only: no MFMA, no floating point, no LDS but the class counts, no atomics but
// the class counts and the coverage (integer add and min, which commute).
#include "vsc_internal.h"
#include "vsc_device.h"

namespace vsc {

namespace {

constexpr int kEditThreads = kWave * kWavesPerGroup;
static_assert(kEditTile % kWave == 0, "a tile is a whole number of steps of one wave");

// candidate r: its class; *v = (mask, hits), the undefined pair unless the class is kEffDefined
__device__ __forceinline__ uint32_t edit_candidate(const EffPlanes &g, const EditShape &s, const EditTargets &t, const uint4 r, uint2 *v)
{
    uint64_t ch = 0, cl = 0;
    const uint32_t cls = edit_site(g, s, r.x, r.y, r.z, &ch, &cl);
    if (cls != kEffDefined) {
        *v = make_uint2(kEditUndefined, kEditUndefined);
        return cls;
    }
    const uint32_t mask = edit_mask(ch, cl, s);
    uint32_t hits = 0;
    if (mask && t.n) {
        const uint32_t g0 = g.contig_off[r.x] + edit_window_first(r.y, r.z, s);  // (defined: r.x is a contig)
        hits = edit_hits(mask, edit_first_target(t, g0), t, g0, r.z, s);
    }
    *v = make_uint2(mask, hits);
    return cls;
}

// exclusive prefix of v over the lanes of the wave; *total = the wave's sum (cross-lane moves, no LDS memory)
__device__ __forceinline__ uint32_t edit_wave_exclusive(uint32_t v, uint32_t lane, uint32_t *total)
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

// out[i] = (mask, hits) of loci[i], grid-stride over the 64-bit count in steps of whole waves; one coalesced 8-byte store per
// lane.  The classes and the candidates with a hit are counted per wave (a ballot per counter and step), added per workgroup
// in LDS and go out with one atomic add per counter and workgroup.
__global__ __launch_bounds__(kEditThreads) void edit_rows_kernel(const EditArgs a)
{
    __shared__ unsigned long long s_count[kEditCounts];
    if (threadIdx.x < kEditCounts) s_count[threadIdx.x] = 0;
    block_sync();
    const uint32_t lane = threadIdx.x % kWave;
    const unsigned long long stride = (unsigned long long)gridDim.x * kEditThreads;
    uint32_t seen[kEditCounts] = {};  // wave-uniform
    const unsigned long long first = (unsigned long long)blockIdx.x * kEditThreads + threadIdx.x;
    uint4 ahead = first < a.n ? a.loci[first] : make_uint4(0u, 0u, 0u, 0u);  // the next step's locus is on its way during a step
    for (unsigned long long base = first - lane; base < a.n; base += stride) {
        const unsigned long long i = base + lane;
        const bool live = i < a.n;
        const uint4 r = ahead;
        if (i + stride < a.n) ahead = a.loci[i + stride];
        uint32_t cls = kEffClasses;
        bool hit = false;
        if (live) {
            uint2 v;
            cls = edit_candidate(a.g, a.shape, a.targets, r, &v);
            hit = cls == kEffDefined && v.y != 0u;
            a.out[i] = v;
        }
#pragma unroll
        for (uint32_t k = 0; k < kEffClasses; ++k) seen[k] += (uint32_t)__popcll(__ballot(cls == k));
        seen[kEffClasses] += (uint32_t)__popcll(__ballot(hit));
    }
    if (lane == 0) {
#pragma unroll
        for (uint32_t k = 0; k < kEditCounts; ++k)
            if (seen[k]) atomicAdd(&s_count[k], (unsigned long long)seen[k]);
    }
    block_sync();
    if (threadIdx.x < kEditCounts && s_count[threadIdx.x]) atomicAdd(&a.stats[threadIdx.x], s_count[threadIdx.x]);
}

// kWrite = false: tile_count[i] = the pairs of tile i - popcount(hits) over its candidates, read from the rows.  kWrite = true:
// every pair to tile_off[i] + the pairs of the tile's earlier steps + the pairs of the lanes below (an exclusive scan over the
// wave) + its place among the candidate's own, which is the order of the walk over the targets: ascending (candidate, target).
// Only a lane with hits reads its locus and repeats the lower bound.  One wave per tile of kEditTile candidates; no append
// cursor: the bytes depend on the rows, the loci and the targets only.  The coverage is taken here: one integer add and one
// integer min per pair.
template <bool kWrite> __global__ __launch_bounds__(kEditThreads) void edit_pairs_kernel(const EditPairArgs a)
{
    const uint32_t lane = threadIdx.x % kWave;
    const uint32_t item = blockIdx.x * kWavesPerGroup + threadIdx.x / kWave;  // wave-uniform
    if (item >= a.n_work) return;
    const unsigned long long first = (unsigned long long)item * kEditTile;
    unsigned long long at = kWrite ? a.tile_off[item] : 0;
    uint32_t count = 0;
    for (uint32_t step = 0; step < kEditTile / kWave; ++step) {
        const unsigned long long base = first + (unsigned long long)step * kWave;
        if (base >= a.n) break;
        const unsigned long long i = base + lane;
        uint2 v = make_uint2(0u, 0u);
        if (i < a.n) v = a.rows[i];
        const uint32_t hits = v.y == kEditUndefined ? 0u : v.y & 0xFFFFu;
        const uint32_t mine = (uint32_t)__popc(hits);
        uint32_t total;
        const uint32_t before = edit_wave_exclusive(mine, lane, &total);
        if (kWrite) {
            if (hits) {
                const uint4 r = a.loci[i];
                const uint32_t g0 = a.contig_off[r.x] + edit_window_first(r.y, r.z, a.shape);  // (a row with hits: r.x is a contig)
                const uint32_t k0 = edit_first_target(a.targets, g0);
                unsigned long long o = at + before;
                for (uint32_t k = k0; k - k0 < a.shape.win_len; ++k) {
                    const uint32_t j = edit_target_at(a.targets, k, g0, r.z, a.shape);
                    if (j >= a.shape.win_len) break;
                    if (!(hits >> j & 1u)) continue;
                    const uint32_t info = edit_pair_info(v.x, j);
                    if (a.pairs) a.pairs[o] = make_uint4((uint32_t)i, k, v.x, info);
                    ++o;
                    if (a.cov_count) {
                        atomicAdd(&a.cov_count[k], 1u);
                        atomicMin(&a.cov_min[k], info >> 8);
                    }
                }
            }
            at += total;
        } else {
            count += total;
        }
    }
    if (!kWrite && lane == 0) a.tile_count[item] = count;
}

// kWrite = false: tile_count[i] = the candidates of tile work[i] that pass FILTER (edit_keep).  kWrite = true: the same test
// again, every survivor's code and locus to tile_off[i] + its rank in the tile - the input's order.  One wave per tile of
// kEditTile candidates; the rank inside a step is the survivors in the lanes below (a ballot), no atomic.
template <bool kWrite> __global__ __launch_bounds__(kEditThreads) void edit_filter_kernel(const EditFilterArgs a)
{
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
            const uint32_t cls = edit_candidate(a.g, a.shape, a.targets, r, &v);
            keep = edit_keep(cls, v.x, v.y, a.min_editable, a.max_editable, a.targets.n != 0u);
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

// *out += the targets with a pair (cov_count[k] != 0): a ballot per step, one atomic add per wave that saw any
__global__ __launch_bounds__(kEditThreads) void edit_covered_kernel(const uint32_t *cov_count, uint32_t n_t, unsigned long long *out)
{
    const uint32_t lane = threadIdx.x % kWave;
    const unsigned long long stride = (unsigned long long)gridDim.x * kEditThreads;
    uint32_t seen = 0;  // wave-uniform
    for (unsigned long long base = (unsigned long long)blockIdx.x * kEditThreads + threadIdx.x - lane; base < n_t; base += stride) {
        const unsigned long long i = base + lane;
        seen += (uint32_t)__popcll(__ballot(i < n_t && cov_count[i] != 0u));
    }
    if (lane == 0 && seen) atomicAdd(out, (unsigned long long)seen);
}

hipError_t launch_edit_rows(const EditArgs &args, int n_cus, hipStream_t stream)
{
    if (args.n == 0) return hipSuccess;
    // 8 workgroups of 4 waves per CU fill every SIMD's 8 wave slots; fewer when the candidates do not need them (launch_locate)
    const unsigned long long want = (args.n + kEditThreads - 1) / kEditThreads;
    const unsigned long long cap = (unsigned long long)(n_cus > 0 ? n_cus : 256) * 8u;
    const dim3 grid((uint32_t)(want < cap ? want : cap)), block(kEditThreads);
    hipLaunchKernelGGL(edit_rows_kernel, grid, block, 0, stream, args);
    return hipGetLastError();
}

hipError_t launch_edit_pairs(const EditPairArgs &args, bool write, hipStream_t stream)
{
    if (args.n_work == 0) return hipSuccess;
    const dim3 grid((args.n_work + kWavesPerGroup - 1) / kWavesPerGroup), block(kEditThreads);
    if (write) hipLaunchKernelGGL((edit_pairs_kernel<true>), grid, block, 0, stream, args);
    else hipLaunchKernelGGL((edit_pairs_kernel<false>), grid, block, 0, stream, args);
    return hipGetLastError();
}

hipError_t launch_edit_covered(const uint32_t *cov_count, uint32_t n_t, unsigned long long *out, int n_cus, hipStream_t stream)
{
    if (n_t == 0) return hipSuccess;
    const unsigned long long want = ((unsigned long long)n_t + kEditThreads - 1) / kEditThreads;
    const unsigned long long cap = (unsigned long long)(n_cus > 0 ? n_cus : 256) * 8u;
    hipLaunchKernelGGL(edit_covered_kernel, dim3((uint32_t)(want < cap ? want : cap)), dim3(kEditThreads), 0, stream, cov_count, n_t, out);
    return hipGetLastError();
}

hipError_t launch_edit_filter(const EditFilterArgs &args, bool write, hipStream_t stream)
{
    if (args.n_work == 0) return hipSuccess;
    const dim3 grid((args.n_work + kWavesPerGroup - 1) / kWavesPerGroup), block(kEditThreads);
    if (write) hipLaunchKernelGGL((edit_filter_kernel<true>), grid, block, 0, stream, args);
    else hipLaunchKernelGGL((edit_filter_kernel<false>), grid, block, 0, stream, args);
    return hipGetLastError();
}

}  // namespace vsc
