// vsc_efficiency.hip - the on-target efficiency score on the device: eff_score_kernel over loci (vsc_loci_efficiency,
// vsc_guides_efficiency, vsc_pattern_guides_efficiency), eff_filter_kernel<kWrite> over a candidate list (the two passes of
// vsc_guides_filter_efficiency).  The class of a candidate, its context and its predictor are eff_context and eff_linear of
// vsc_efficiency.h - the functions vsc_eff_score_text and the stand-alone check call on the host.
//
// Both kernels take one candidate per lane and step: one 16-byte locus load, the bounds tests in the order of the classes
// (every index checked against its array's length before use, as locate_kernel does), the context as a 64-bit window per
// plane out of up to three consecutive words of hi, lo and nm, reversed and complemented on '-'.  The weights lie in LDS as
// [j][letter]: the loops over j have the model's C steps on every lane, so at step j the lanes of a wave read one of 4
// consecutive doubles (mono) or one of 16 (di) - distinct banks or the same address, a ds_read_b64 without a conflict.  A lane
// whose candidate has no context runs the same steps on an all-A context and drops the sum.  Additions only: no MFMA, nothing to
// contract, no exp (the logistic link is the host's, vsc_eff_link).
#include "vsc_internal.h"
#include "vsc_device.h"

namespace vsc {

namespace {

constexpr int kEffThreads = kWave * kWavesPerGroup;
static_assert(kEffTile % kWave == 0, "a tile is a whole number of steps of one wave");

// the model's weights into the workgroup's LDS; every thread of the workgroup calls it
__device__ __forceinline__ void eff_load_weights(double *s_w, const EffModelView &m)
{
    const uint32_t n = min(m.n_weights, kEffMaxWeights);
    for (uint32_t i = threadIdx.x; i < n; i += kEffThreads) s_w[i] = m.w[i];
    block_sync();
}

// candidate r: its class; *x = its predictor (kEffUndefinedBits unless the class is kEffDefined)
__device__ __forceinline__ uint32_t eff_candidate(const EffPlanes &g, const EffModelView &m, const double *s_w, const uint4 r, double *x)
{
    uint64_t ch = 0, cl = 0;
    const uint32_t cls = eff_context(g, m.shape, r.x, r.y, r.z, &ch, &cl);
    const double v = eff_linear(s_w, m.intercept, m.shape, ch, cl);
    *x = cls == kEffDefined ? v : eff_undefined();
    return cls;
}

}  // namespace

// linear[i] = the predictor of loci[i], grid-stride over the 64-bit count in steps of whole waves; one coalesced 8-byte store
// per lane.  The classes are counted per wave (a ballot per class and step), added per workgroup in LDS and go out with one
// atomic add per class and workgroup.
__global__ __launch_bounds__(kEffThreads) void eff_score_kernel(const EffArgs a)
{
    __shared__ double s_w[kEffMaxWeights];
    __shared__ unsigned long long s_count[kEffClasses];
    if (threadIdx.x < kEffClasses) s_count[threadIdx.x] = 0;
    eff_load_weights(s_w, a.m);
    const uint32_t lane = threadIdx.x % kWave;
    const unsigned long long stride = (unsigned long long)gridDim.x * kEffThreads;
    uint32_t seen[kEffClasses] = {};  // wave-uniform
    const unsigned long long first = (unsigned long long)blockIdx.x * kEffThreads + threadIdx.x;
    uint4 ahead = first < a.n ? a.loci[first] : make_uint4(0u, 0u, 0u, 0u);  // the next step's locus is on its way during a step
    for (unsigned long long base = first - lane; base < a.n; base += stride) {
        const unsigned long long i = base + lane;
        const bool live = i < a.n;
        const uint4 r = ahead;
        if (i + stride < a.n) ahead = a.loci[i + stride];
        uint32_t cls = kEffClasses;
        if (live) {
            double x;
            cls = eff_candidate(a.g, a.m, s_w, r, &x);
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

// kWrite = false: tile_count[i] = the candidates of tile work[i] whose predictor is defined and >= min_linear.  kWrite = true:
// the same test again, every survivor's code and locus to tile_off[i] + its rank in the tile - the input's order.  One wave per
// tile of kEffTile candidates, kEffTile / 64 steps; the rank inside a step is the survivors in the lanes below (a ballot), no
// atomic: the bytes depend on the input and the model only.
template <bool kWrite> __global__ __launch_bounds__(kEffThreads) void eff_filter_kernel(const EffFilterArgs a)
{
    __shared__ double s_w[kEffMaxWeights];
    eff_load_weights(s_w, a.m);
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
            keep = eff_candidate(a.g, a.m, s_w, r, &x) == kEffDefined && x >= a.min_linear;
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

hipError_t launch_eff_score(const EffArgs &args, int n_cus, hipStream_t stream)
{
    if (args.n == 0) return hipSuccess;
    // 8 workgroups of 4 waves per CU fill every SIMD's 8 wave slots; fewer when the candidates do not need them (launch_locate)
    const unsigned long long want = (args.n + kEffThreads - 1) / kEffThreads;
    const unsigned long long cap = (unsigned long long)(n_cus > 0 ? n_cus : 256) * 8u;
    const dim3 grid((uint32_t)(want < cap ? want : cap)), block(kEffThreads);
    hipLaunchKernelGGL(eff_score_kernel, grid, block, 0, stream, args);
    return hipGetLastError();
}

hipError_t launch_eff_filter(const EffFilterArgs &args, bool write, hipStream_t stream)
{
    if (args.n_work == 0) return hipSuccess;
    const dim3 grid((args.n_work + kWavesPerGroup - 1) / kWavesPerGroup), block(kEffThreads);
    if (write) hipLaunchKernelGGL((eff_filter_kernel<true>), grid, block, 0, stream, args);
    else hipLaunchKernelGGL((eff_filter_kernel<false>), grid, block, 0, stream, args);
    return hipGetLastError();
}

}  // namespace vsc
