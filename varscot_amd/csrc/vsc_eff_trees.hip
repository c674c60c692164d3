// vsc_eff_trees.hip - the on-target efficiency score of a regression-tree ensemble on the device:
// eff_trees_score_kernel over loci (vsc_loci_efficiency_trees, vsc_guides_efficiency_trees, vsc_pattern_guides_efficiency_trees),
// eff_trees_filter_kernel<kWrite> over a candidate list (the two passes of vsc_guides_filter_efficiency_trees).  The class of a
// candidate and its context are eff_context of vsc_efficiency.h, its sums and its predictor eff_trees_sums and
// eff_trees_predict of vsc_eff_trees.h - the functions vsc_eff_trees_score_text and the stand-alone check call on the host.
//
// Both kernels are eff_score_kernel / eff_filter_kernel with another predictor: one candidate per lane and step, the locus of
// the next step on its way during a step, the three planes' words asked for together.  The packed model lies in the
// workgroup's LDS (dynamic: its words, then one row of kEffThreads int32 per sum), copied once per workgroup.  A candidate's
// sums are computed once, into its column of the rows - a lane reads its own S_i with one ds_read_b32, whatever i its node
// names, and no register is indexed by a lane's own number.  The walk keeps the tree index wave-uniform: a lane that reached
// its leaf waits for the deepest path of that tree, and every lane adds its leaves in tree order.  A lane whose candidate has
// no context walks an all-A context and drops the sum.  Additions only: no MFMA, nothing to contract, no exp.
#include "vsc_internal.h"
#include "vsc_device.h"

namespace vsc {

namespace {

constexpr int kEffTreesThreads = kWave * kWavesPerGroup;
constexpr size_t kEffTreesLdsPerCu = 160u * 1024u;  // gfx950

__host__ __device__ inline uint32_t eff_trees_lds_words(const EffTreesView &m) { return (m.n_words + 1u) & ~1u; }

size_t eff_trees_lds_bytes(const EffTreesView &m)
{
    return ((size_t)eff_trees_lds_words(m) + (size_t)m.n_sums * kEffTreesThreads) * sizeof(uint32_t);
}

// the packed model into the workgroup's LDS; every thread of the workgroup calls it.  Returns the model over LDS.
__device__ __forceinline__ EffTreesPacked eff_trees_load(uint32_t *s_words, const EffTreesView &m)
{
    for (uint32_t i = threadIdx.x; i < m.n_words; i += kEffTreesThreads) s_words[i] = m.words[i];
    block_sync();
    return EffTreesPacked{s_words, m.n_nodes, m.n_sums, m.n_trees, m.base};
}

// candidate r: its class; *x = its predictor (kEffUndefinedBits unless the class is kEffDefined).  s_sum: this lane's column
// of the sums' rows.
__device__ __forceinline__ uint32_t eff_trees_candidate(const EffPlanes &g, const EffShape &shape, const EffTreesPacked &m, int32_t *s_sum,
                                                        const uint4 r, double *x)
{
    uint64_t ch = 0, cl = 0;
    const uint32_t cls = eff_context(g, shape, r.x, r.y, r.z, &ch, &cl);
    eff_trees_sums(m, eff_context_len(shape), ch, cl, s_sum, kEffTreesThreads);
    const double v = eff_trees_predict(m, ch, cl, s_sum, kEffTreesThreads);
    *x = cls == kEffDefined ? v : eff_undefined();
    return cls;
}

}  // namespace

// linear[i] = the predictor of loci[i]; the loop, the store and the class counts are eff_score_kernel's.
__global__ __launch_bounds__(kEffTreesThreads) void eff_trees_score_kernel(const EffTreesArgs a)
{
    extern __shared__ __attribute__((aligned(8))) uint32_t s_trees[];
    __shared__ unsigned long long s_count[kEffClasses];
    if (threadIdx.x < kEffClasses) s_count[threadIdx.x] = 0;
    const EffTreesPacked m = eff_trees_load(s_trees, a.m);
    int32_t *s_sum = (int32_t *)(s_trees + eff_trees_lds_words(a.m)) + threadIdx.x;
    const uint32_t lane = threadIdx.x % kWave;
    const unsigned long long stride = (unsigned long long)gridDim.x * kEffTreesThreads;
    uint32_t seen[kEffClasses] = {};  // wave-uniform
    const unsigned long long first = (unsigned long long)blockIdx.x * kEffTreesThreads + threadIdx.x;
    uint4 ahead = first < a.n ? a.loci[first] : make_uint4(0u, 0u, 0u, 0u);  // the next step's locus is on its way during a step
    for (unsigned long long base = first - lane; base < a.n; base += stride) {
        const unsigned long long i = base + lane;
        const bool live = i < a.n;
        const uint4 r = ahead;
        if (i + stride < a.n) ahead = a.loci[i + stride];
        uint32_t cls = kEffClasses;
        if (live) {
            double x;
            cls = eff_trees_candidate(a.g, a.m.shape, m, s_sum, r, &x);
            a.linear[i] = x;
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

// eff_filter_kernel with the trees' predictor: one wave per tile of kEffTile candidates, the rank inside a step from a ballot,
// no atomic - the bytes depend on the input and the model only.
template <bool kWrite> __global__ __launch_bounds__(kEffTreesThreads) void eff_trees_filter_kernel(const EffTreesFilterArgs a)
{
    extern __shared__ __attribute__((aligned(8))) uint32_t s_trees[];
    const EffTreesPacked m = eff_trees_load(s_trees, a.m);
    int32_t *s_sum = (int32_t *)(s_trees + eff_trees_lds_words(a.m)) + threadIdx.x;
    const uint32_t lane = threadIdx.x % kWave;
    const uint32_t item = blockIdx.x * kWavesPerGroup + threadIdx.x / kWave;  // wave-uniform
    if (item >= a.n_work) return;
    const uint32_t tile = a.work ? a.work[item] : item;
    const unsigned long long first = (unsigned long long)tile * kEffTile;
    unsigned long long at = kWrite ? a.tile_off[item] : 0;
    uint32_t count = 0;
    for (uint32_t step = 0; step < kEffTile / kWave; ++step) {
        const unsigned long long base = first + (unsigned long long)step * kWave;
        if (base >= a.n) break;
        const unsigned long long i = base + lane;
        bool keep = false;
        uint4 r = make_uint4(0u, 0u, 0u, 0u);
        if (i < a.n) {
            r = a.in_loci[i];
            double x;
            keep = eff_trees_candidate(a.g, a.m.shape, m, s_sum, r, &x) == kEffDefined && x >= a.min_linear;
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

namespace {

// the model must be one the builder made: its words as vsc_eff_trees.h lays them out, inside the caps, inside a CU's LDS
bool eff_trees_view_valid(const EffTreesView &m)
{
    return m.words && m.n_nodes >= 1 && m.n_nodes <= kEffTreesMaxNodes && m.n_trees >= 1 && m.n_trees <= kEffTreesMaxTrees &&
           m.n_sums <= kEffTreesMaxSums && m.n_words == eff_trees_words(m.n_nodes, m.n_sums, m.n_trees) &&
           eff_trees_lds_bytes(m) + 256 <= kEffTreesLdsPerCu;
}

template <class Kernel, class Args> hipError_t eff_trees_launch(Kernel kernel, const Args &args, dim3 grid, size_t lds, hipStream_t stream)
{
    const hipError_t e = hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, grid, dim3(kEffTreesThreads), lds, stream, args);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_eff_trees_score(const EffTreesArgs &args, int n_cus, hipStream_t stream)
{
    if (args.n == 0) return hipSuccess;
    if (!eff_trees_view_valid(args.m)) return hipErrorInvalidValue;
    const size_t lds = eff_trees_lds_bytes(args.m);
    // as launch_eff_score: 8 workgroups of 4 waves per CU fill every SIMD's 8 wave slots - fewer where the model's LDS lets
    // fewer workgroups lie on a CU (every workgroup copies the model once), fewer when the candidates do not need them
    const unsigned long long fit = kEffTreesLdsPerCu / (lds + 256);
    const unsigned long long per_cu = fit < 1 ? 1 : fit > 8 ? 8 : fit;
    const unsigned long long want = (args.n + kEffTreesThreads - 1) / kEffTreesThreads;
    const unsigned long long cap = (unsigned long long)(n_cus > 0 ? n_cus : 256) * per_cu;
    return eff_trees_launch(eff_trees_score_kernel, args, dim3((uint32_t)(want < cap ? want : cap)), lds, stream);
}

hipError_t launch_eff_trees_filter(const EffTreesFilterArgs &args, bool write, hipStream_t stream)
{
    if (args.n_work == 0) return hipSuccess;
    if (!eff_trees_view_valid(args.m)) return hipErrorInvalidValue;
    const size_t lds = eff_trees_lds_bytes(args.m);
    const dim3 grid((args.n_work + kWavesPerGroup - 1) / kWavesPerGroup);
    if (write) return eff_trees_launch(eff_trees_filter_kernel<true>, args, grid, lds, stream);
    return eff_trees_launch(eff_trees_filter_kernel<false>, args, grid, lds, stream);
}

}  // namespace vsc
