// vsc_fold.hip - the self-complementarity of candidate guides on the device: fold_rows_kernel over loci
// (vsc_loci_fold, vsc_guides_fold, vsc_pattern_guides_fold), fold_filter_kernel<kWrite> over a candidate list (the two passes
// of vsc_guides_filter_fold).  The class of a candidate, its spacer and its row are fold_context and fold_row of vsc_fold.h -
// the functions vsc_fold_text and the stand-alone check call on the host.
//
// Both kernels take one candidate per lane and step, as the kernels of vsc_mh.hip do: one 16-byte locus load, the bounds
// tests in the order of the classes, the site as a window per plane, reversed and complemented on '-'.  The scaffold's
// windows - one per diagonal, the same for every lane - are copied into LDS once per workgroup (at most 159 * 16 bytes), so
// the arguments stay small and a diagonal reads its window with one uniform 16-byte LDS read.  The loops over the diagonals
// have the launch's trip count on every lane; a lane whose candidate has no context runs them on zeros and drops the result.
// Integers only: no MFMA, no floating point, no atomics but the class counts.
#include "vsc_internal.h"
#include "vsc_device.h"

namespace vsc {

namespace {

constexpr int kFoldThreads = kWave * kWavesPerGroup;
static_assert(kFoldTile % kWave == 0, "a tile is a whole number of steps of one wave");
static_assert(sizeof(FoldWindow) == sizeof(uint4), "a window is one 16-byte read");

// the launch's windows into LDS; every thread of the workgroup calls it, a barrier follows
__device__ __forceinline__ void fold_stage_windows(FoldWindow *s_win, const FoldWindow *win, uint32_t n_diag)
{
    for (uint32_t c = threadIdx.x; c < n_diag && c < kFoldMaxDiagonals; c += kFoldThreads) s_win[c] = win[c];
    block_sync();
}

// candidate r: its class; *v = its row, the undefined row unless the class is kEffDefined
__device__ __forceinline__ uint32_t fold_candidate(const EffPlanes &g, const FoldShape &s, const FoldScaffold &sc, const uint4 r, uint2 *v)
{
    uint32_t gh = 0, gl = 0;
    const uint32_t cls = fold_context(g, s, r.x, r.y, r.z, &gh, &gl);
    uint32_t w0, w1;
    fold_row(gh, gl, sc, s, &w0, &w1);
    *v = cls == kEffDefined ? make_uint2(w0, w1) : make_uint2(kFoldUndefined, kFoldUndefined);
    return cls;
}

}  // namespace

// out[i] = the row of loci[i], grid-stride over the 64-bit count in steps of whole waves; one coalesced 8-byte store per
// lane.  The classes are counted per wave (a ballot per class and step), added per workgroup in LDS and go out with one
// atomic add per class and workgroup.
__global__ __launch_bounds__(kFoldThreads) void fold_rows_kernel(const FoldArgs a)
{
    __shared__ unsigned long long s_count[kEffClasses];
    __shared__ FoldWindow s_win[kFoldMaxDiagonals];
    if (threadIdx.x < kEffClasses) s_count[threadIdx.x] = 0;
    fold_stage_windows(s_win, a.win, a.n_diag);
    const FoldScaffold sc{s_win, a.n_diag < kFoldMaxDiagonals ? a.n_diag : kFoldMaxDiagonals};
    const uint32_t lane = threadIdx.x % kWave;
    const unsigned long long stride = (unsigned long long)gridDim.x * kFoldThreads;
    uint32_t seen[kEffClasses] = {};  // wave-uniform
    const unsigned long long first = (unsigned long long)blockIdx.x * kFoldThreads + threadIdx.x;
    uint4 ahead = first < a.n ? a.loci[first] : make_uint4(0u, 0u, 0u, 0u);  // the next step's locus is on its way during a step
    for (unsigned long long base = first - lane; base < a.n; base += stride) {
        const unsigned long long i = base + lane;
        const bool live = i < a.n;
        const uint4 r = ahead;
        if (i + stride < a.n) ahead = a.loci[i + stride];
        uint32_t cls = kEffClasses;
        if (live) {
            uint2 v;
            cls = fold_candidate(a.g, a.shape, sc, r, &v);
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

// kWrite = false: tile_count[i] = the candidates of tile work[i] that pass the limits (fold_keep).  kWrite = true: the same
// test again, every survivor's code and locus to tile_off[i] + its rank in the tile - the input's order.  One wave per tile
// of kFoldTile candidates, kFoldTile / 64 steps; the rank inside a step is the survivors in the lanes below (a ballot), no
// atomic: the bytes depend on the input, the shape, the scaffold and the limits only.
template <bool kWrite> __global__ __launch_bounds__(kFoldThreads) void fold_filter_kernel(const FoldFilterArgs a)
{
    __shared__ FoldWindow s_win[kFoldMaxDiagonals];
    fold_stage_windows(s_win, a.win, a.n_diag);  // (in front of the wave's way out: every wave meets the barrier)
    const FoldScaffold sc{s_win, a.n_diag < kFoldMaxDiagonals ? a.n_diag : kFoldMaxDiagonals};
    const uint32_t lane = threadIdx.x % kWave;
    const uint32_t item = blockIdx.x * kWavesPerGroup + threadIdx.x / kWave;  // wave-uniform
    if (item >= a.n_work) return;
    const uint32_t tile = a.work ? a.work[item] : item;
    const unsigned long long first = (unsigned long long)tile * kFoldTile;
    unsigned long long at = kWrite ? a.tile_off[item] : 0;
    uint32_t count = 0;
    for (uint32_t step = 0; step < kFoldTile / kWave; ++step) {
        const unsigned long long base = first + (unsigned long long)step * kWave;
        if (base >= a.n) break;
        const unsigned long long i = base + lane;
        bool keep = false;
        uint4 r = make_uint4(0u, 0u, 0u, 0u);
        if (i < a.n) {
            r = a.in_loci[i];
            uint2 v;
            const uint32_t cls = fold_candidate(a.g, a.shape, sc, r, &v);
            keep = fold_keep(cls, v.x, v.y, a.limits);
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

hipError_t launch_fold_rows(const FoldArgs &args, int n_cus, uint32_t groups_per_cu, hipStream_t stream)
{
    if (args.n == 0) return hipSuccess;
    // 8 workgroups of 4 waves per CU fill every SIMD's 8 wave slots; fewer when the candidates do not need them
    const unsigned long long want = (args.n + kFoldThreads - 1) / kFoldThreads;
    const unsigned long long cap = (unsigned long long)(n_cus > 0 ? n_cus : 256) * (groups_per_cu ? groups_per_cu : kFoldGroupsPerCu);
    const dim3 grid((uint32_t)(want < cap ? want : cap)), block(kFoldThreads);
    hipLaunchKernelGGL(fold_rows_kernel, grid, block, 0, stream, args);
    return hipGetLastError();
}

hipError_t launch_fold_filter(const FoldFilterArgs &args, bool write, hipStream_t stream)
{
    if (args.n_work == 0) return hipSuccess;
    const dim3 grid((args.n_work + kWavesPerGroup - 1) / kWavesPerGroup), block(kFoldThreads);
    if (write) hipLaunchKernelGGL((fold_filter_kernel<true>), grid, block, 0, stream, args);
    else hipLaunchKernelGGL((fold_filter_kernel<false>), grid, block, 0, stream, args);
    return hipGetLastError();
}

}  // namespace vsc
