// vsc_mh.hip - the microhomology score on the device: mh_score_kernel over loci (vsc_loci_microhomology,
// vsc_guides_microhomology, vsc_pattern_guides_microhomology), mh_filter_kernel<kWrite> over a candidate list (the two passes
// of vsc_guides_filter_microhomology).  The class of a candidate, its context and its score are mh_context and mh_score of
// vsc_mh.h - the functions vsc_mh_score_text and the stand-alone check call on the host.
//
// Both kernels take one candidate per lane and step, as the kernels of vsc_efficiency.hip do: one 16-byte locus load, the
// bounds tests in the order of the classes (every index checked against its array's length before use), the context as a
// 64-bit window per plane out of up to three consecutive words of hi, lo and nm, reversed and complemented on '-'.  The loop
// over the deletion length has W - 1 steps on every lane - the shape is the launch's, not the candidate's - and its table
// entry is one scalar load per step.  A lane whose candidate has no context runs the loop on zeros and drops the result.
// Integers only: no MFMA, no floating point, no atomics but the class counts.
#include "vsc_internal.h"
#include "vsc_device.h"

namespace vsc {

namespace {

constexpr int kMhThreads = kWave * kWavesPerGroup;
static_assert(kMhTile % kWave == 0, "a tile is a whole number of steps of one wave");

// candidate r: its class; *v = (sum, oof), the undefined pair unless the class is kEffDefined
__device__ __forceinline__ uint32_t mh_candidate(const EffPlanes &g, const MhShape &s, const uint4 r, uint2 *v)
{
    uint64_t ch = 0, cl = 0;
    const uint32_t cls = mh_context(g, s, r.x, r.y, r.z, &ch, &cl);
    uint32_t sum, oof;
    mh_score(ch, cl, s.flank, &sum, &oof);
    *v = cls == kEffDefined ? make_uint2(sum, oof) : make_uint2(kMhUndefined, kMhUndefined);
    return cls;
}

}  // namespace

// out[i] = (sum, oof) of loci[i], grid-stride over the 64-bit count in steps of whole waves; one coalesced 8-byte store per
// lane.  The classes are counted per wave (a ballot per class and step), added per workgroup in LDS and go out with one
// atomic add per class and workgroup.
__global__ __launch_bounds__(kMhThreads) void mh_score_kernel(const MhArgs a)
{
    __shared__ unsigned long long s_count[kEffClasses];
    if (threadIdx.x < kEffClasses) s_count[threadIdx.x] = 0;
    block_sync();
    const uint32_t lane = threadIdx.x % kWave;
    const unsigned long long stride = (unsigned long long)gridDim.x * kMhThreads;
    uint32_t seen[kEffClasses] = {};  // wave-uniform
    const unsigned long long first = (unsigned long long)blockIdx.x * kMhThreads + threadIdx.x;
    uint4 ahead = first < a.n ? a.loci[first] : make_uint4(0u, 0u, 0u, 0u);  // the next step's locus is on its way during a step
    for (unsigned long long base = first - lane; base < a.n; base += stride) {
        const unsigned long long i = base + lane;
        const bool live = i < a.n;
        const uint4 r = ahead;
        if (i + stride < a.n) ahead = a.loci[i + stride];
        uint32_t cls = kEffClasses;
        if (live) {
            uint2 v;
            cls = mh_candidate(a.g, a.shape, r, &v);
            a.out[i] = v;
        }
#pragma unroll
        for (uint32_t k = 0; k < kEffClasses; ++k) seen[k] += (uint32_t)__popcll(__ballot(cls == k));
    }
    if (lane == 0) {
#pragma unroll
        for (uint32_t k = 0; k < kEffClasses; ++k)
            if (seen[k]) atomicAdd(&s_count[k], (unsigned long long)seen[k]);
    }
    block_sync();
    if (threadIdx.x < kEffClasses && s_count[threadIdx.x]) atomicAdd(&a.stats[threadIdx.x], s_count[threadIdx.x]);
}

// kWrite = false: tile_count[i] = the candidates of tile work[i] that pass the floors (mh_keep).  kWrite = true: the same
// test again, every survivor's code and locus to tile_off[i] + its rank in the tile - the input's order.  One wave per tile
// of kMhTile candidates, kMhTile / 64 steps; the rank inside a step is the survivors in the lanes below (a ballot), no atomic:
// the bytes depend on the input, the shape and the floors only.
template <bool kWrite> __global__ __launch_bounds__(kMhThreads) void mh_filter_kernel(const MhFilterArgs a)
{
    const uint32_t lane = threadIdx.x % kWave;
    const uint32_t item = blockIdx.x * kWavesPerGroup + threadIdx.x / kWave;  // wave-uniform
    if (item >= a.n_work) return;
    const uint32_t tile = a.work ? a.work[item] : item;
    const unsigned long long first = (unsigned long long)tile * kMhTile;
    unsigned long long at = kWrite ? a.tile_off[item] : 0;
    uint32_t count = 0;
    for (uint32_t step = 0; step < kMhTile / kWave; ++step) {
        const unsigned long long base = first + (unsigned long long)step * kWave;
        if (base >= a.n) break;
        const unsigned long long i = base + lane;
        bool keep = false;
        uint4 r = make_uint4(0u, 0u, 0u, 0u);
        if (i < a.n) {
            r = a.in_loci[i];
            uint2 v;
            const uint32_t cls = mh_candidate(a.g, a.shape, r, &v);
            keep = mh_keep(cls, v.x, v.y, a.min_sum, a.min_oof_permille);
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

hipError_t launch_mh_score(const MhArgs &args, int n_cus, hipStream_t stream)
{
    if (args.n == 0) return hipSuccess;
    // 8 workgroups of 4 waves per CU fill every SIMD's 8 wave slots; fewer when the candidates do not need them (launch_locate)
    const unsigned long long want = (args.n + kMhThreads - 1) / kMhThreads;
    const unsigned long long cap = (unsigned long long)(n_cus > 0 ? n_cus : 256) * 8u;
    const dim3 grid((uint32_t)(want < cap ? want : cap)), block(kMhThreads);
    hipLaunchKernelGGL(mh_score_kernel, grid, block, 0, stream, args);
    return hipGetLastError();
}

hipError_t launch_mh_filter(const MhFilterArgs &args, bool write, hipStream_t stream)
{
    if (args.n_work == 0) return hipSuccess;
    const dim3 grid((args.n_work + kWavesPerGroup - 1) / kWavesPerGroup), block(kMhThreads);
    if (write) hipLaunchKernelGGL((mh_filter_kernel<true>), grid, block, 0, stream, args);
    else hipLaunchKernelGGL((mh_filter_kernel<false>), grid, block, 0, stream, args);
    return hipGetLastError();
}

}  // namespace vsc
