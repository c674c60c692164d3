// vsc_pairs.hip - the paired-nickase screen (vsc_hits_pairs, vsc_guides_pairs): range lookups in arrays that are
// sorted and resident already - the records of a result in (guide, strand, contig, pos) order, the candidates of
// vsc_guides_enumerate in (contig, pos, strand) order.  No search kernel, no sort, no scoring.
//
// Three kernels.  pair_segments_kernel writes the first record of every (guide, strand) run, so that every later search runs
// inside one run.  pair_join_kernel takes one (pair, record of the pair's first guide) per lane and step, finds the record's
// partners in the run (second guide, other strand) with one lower bound and walks them; its count pass adds into the pairs'
// rows and notes every item's count, its write pass - after an exclusive scan of the counts (enum_scan_kernel) - puts every
// item's sites behind the sites of all earlier items: ascending (pair, a_rec, b_rec), no sort, no append atomic.
// pair_loci_kernel is the same walk over 16-byte vsc_locus records.  The geometry is vsc_pairs.h's, shared with the host.
//
// Gathers bound by the latency of their dependent loads, as locate_kernel: one item per lane and step, grid-stride over a 64-bit
// count, 8 workgroups of 4 waves per CU, the last wave partly idle.  Every index is checked against its array's length (the
// segment table bounds every record index by n) before it is used.
#include "vsc_internal.h"
#include "vsc_device.h"
#include "vsc_pairs.h"

namespace vsc {

constexpr int kPairThreads = 256;

__global__ __launch_bounds__(kPairThreads) void pair_segments_kernel(const PairSegArgs a)
{
    const uint32_t k = blockIdx.x * kPairThreads + threadIdx.x;
    if (k > 2u * a.n_guides) return;
    uint32_t lo = 0, hi = a.n;  // -> #{records with 2 guide + strand < k}
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        const uint4 r = a.records[mid];
        if ((((unsigned long long)r.x << 1) | (r.w >> 31)) < k) lo = mid + 1; else hi = mid;
    }
    a.seg[k] = lo;
}

template <bool kWrite>
__global__ __launch_bounds__(kPairThreads) void pair_join_kernel(const PairJoinArgs a)
{
    const unsigned long long stride = (unsigned long long)gridDim.x * kPairThreads;
    for (unsigned long long item = (unsigned long long)blockIdx.x * kPairThreads + threadIdx.x; item < a.n_items; item += stride) {
        uint32_t lo = 0, hi = a.n_pairs;  // -> #{pairs with pair_off <= item}; >= 1 (pair_off[0] = 0)
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (a.pair_off[mid] <= item) lo = mid + 1; else hi = mid;
        }
        const uint32_t j = lo - 1u;
        const uint2 pr = a.pairs[j];
        const uint32_t r = a.seg[2u * pr.x] + (uint32_t)(item - a.pair_off[j]);  // < seg[2 a + 2] <= n
        const uint4 rec = a.records[r];
        const uint32_t strand = rec.w >> 31, nm_a = min((rec.w >> 23) & 31u, (uint32_t)VSC_MAX_MISMATCHES);
        uint32_t cnt = 0, p_lo, p_hi;
        if (pair_range(rec.z, strand, a.delta_min, a.delta_max, &p_lo, &p_hi)) {
            const uint32_t s = 2u * pr.y + (strand ^ 1u), i1 = a.seg[s + 1u];
            bool excl_a = false;
            uint4 eb = make_uint4(kPairNoContig, 0u, 0u, 0u);
            if (a.exclude) {
                const uint4 ea = a.exclude[pr.x];
                excl_a = ea.x == rec.y && ea.y == rec.z && ea.z == strand;
                eb = a.exclude[pr.y];
            }
            unsigned long long *row = a.rows + (size_t)j * kPairRowWords;
            const unsigned long long at = kWrite ? a.item_off[item] : 0ull;
            for (uint32_t k = pair_lower_bound<true>(a.records, a.seg[s], i1, rec.y, p_lo); k < i1; ++k) {
                const uint4 q = a.records[k];
                if (pair_after<true>(q, rec.y, p_hi)) break;
                if (excl_a && eb.x == q.y && eb.y == q.z && eb.z == (q.w >> 31)) {  // the pair's on-target: not counted
                    if (!kWrite) *(uint32_t *)(row + kPairRowOnTarget) = 1u;
                    continue;
                }
                if (kWrite) {
                    a.sites[at + cnt] = make_uint4(j, r, k, (uint32_t)pair_delta(rec.z, strand, q.z));
                } else {
                    const uint32_t nm_b = min((q.w >> 23) & 31u, (uint32_t)VSC_MAX_MISMATCHES);
                    atomicAdd(row + kPairRowNmSum + nm_a + nm_b, 1ull);
                    atomicAdd(row + kPairRowNmMax + max(nm_a, nm_b), 1ull);
                }
                ++cnt;
            }
            if (!kWrite && cnt) atomicAdd(row, (unsigned long long)cnt);
        }
        if (!kWrite && a.item_count) a.item_count[item] = cnt;
    }
}

template <bool kWrite>
__global__ __launch_bounds__(kPairThreads) void pair_loci_kernel(const PairLociArgs a)
{
    const unsigned long long stride = (unsigned long long)gridDim.x * kPairThreads;
    for (unsigned long long i = (unsigned long long)blockIdx.x * kPairThreads + threadIdx.x; i < a.n; i += stride) {
        const uint4 l = a.loci[i];
        uint32_t cnt = 0, p_lo, p_hi;
        if (l.z == 1u && l.x != kPairNoContig && pair_range(l.y, 1u, a.delta_min, a.delta_max, &p_lo, &p_hi)) {
            const unsigned long long at = kWrite ? a.item_off[i] : 0ull;
            for (uint32_t k = pair_lower_bound<false>(a.loci, 0u, a.n, l.x, p_lo); k < a.n; ++k) {
                const uint4 q = a.loci[k];
                if (pair_after<false>(q, l.x, p_hi)) break;
                if (q.z != 0u) continue;
                if (kWrite) a.pairs[at + cnt] = make_uint2((uint32_t)i, k);
                ++cnt;
            }
        }
        if (!kWrite) a.item_count[i] = cnt;
    }
}

namespace {

// 8 workgroups of 4 waves per CU fill every SIMD's 8 wave slots; fewer when the items do not need them
dim3 pair_grid(unsigned long long n, int n_cus)
{
    const unsigned long long want = (n + kPairThreads - 1) / kPairThreads;
    const unsigned long long cap = (unsigned long long)(n_cus > 0 ? n_cus : 256) * 8u;
    return dim3((uint32_t)(want < cap ? want : cap));
}

}  // namespace

hipError_t launch_pair_segments(const PairSegArgs &args, hipStream_t stream)
{
    const uint32_t n = 2u * args.n_guides + 1u;
    hipLaunchKernelGGL(pair_segments_kernel, dim3((n + kPairThreads - 1) / kPairThreads), dim3(kPairThreads), 0, stream, args);
    return hipGetLastError();
}

hipError_t launch_pair_join(const PairJoinArgs &args, bool write, int n_cus, hipStream_t stream)
{
    if (args.n_items == 0) return hipSuccess;
    const dim3 grid = pair_grid(args.n_items, n_cus), block(kPairThreads);
    if (write) hipLaunchKernelGGL((pair_join_kernel<true>), grid, block, 0, stream, args);
    else hipLaunchKernelGGL((pair_join_kernel<false>), grid, block, 0, stream, args);
    return hipGetLastError();
}

hipError_t launch_pair_loci(const PairLociArgs &args, bool write, int n_cus, hipStream_t stream)
{
    if (args.n == 0) return hipSuccess;
    const dim3 grid = pair_grid(args.n, n_cus), block(kPairThreads);
    if (write) hipLaunchKernelGGL((pair_loci_kernel<true>), grid, block, 0, stream, args);
    else hipLaunchKernelGGL((pair_loci_kernel<false>), grid, block, 0, stream, args);
    return hipGetLastError();
}

}  // namespace vsc
