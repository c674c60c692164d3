// vsc_effects.hip - coding consequences of base edits on the device: effects_rows_kernel over loci
// (vsc_loci_effects, vsc_guides_effects, vsc_pattern_guides_effects), effects_records_kernel<kWrite> over the rows it left (the
// two passes behind the records and the coverage), effects_filter_kernel<kWrite> over a candidate list (the two passes of
// vsc_guides_filter_effects).  The class of a candidate, its site and its mask are edit_site and edit_mask of vsc_edit.h; the
// walk over the window, the codon, the class of an effect and the filter's rule are effects_row and effects_keep of
// vsc_effects.h - the functions vsc_effects_site_text and the stand-alone check call on the host.
//
// One candidate per lane and step, as the kernels of vsc_edit.hip: one 16-byte locus load, the site out of the planes, and -
// only for a lane whose mask is not 0 - a lower bound over the segments' global starts (log2(n) dependent loads) and a walk of
// at most win_len steps.  The 64 letters of CODE lie in LDS.  Integers only: no MFMA, no floating point, no atomics but the
// counters and the coverage (integer add and min, which commute).
#include "vsc_internal.h"
#include "vsc_device.h"

namespace vsc {

namespace {

constexpr int kEffectsThreads = kWave * kWavesPerGroup;
static_assert(kEditTile % kWave == 0, "a tile is a whole number of steps of one wave");
static_assert(kEffectsThreads >= 64, "the workgroup's first 64 lanes copy CODE, one letter each");

// CODE from the kernel's arguments to LDS, one letter per lane; the caller synchronises
__device__ __forceinline__ void effects_code_to_lds(const EffectsCode &code, uint8_t *s_code)
{
    if (threadIdx.x < 64) s_code[threadIdx.x] = code.aa[threadIdx.x];
}

// candidate r: its class; *v = its ROW, the undefined pair unless the class is kEffDefined; emit per effect
template <class Emit>
__device__ __forceinline__ uint32_t effects_candidate(const EffPlanes &g, const CdsView &cds, const EditShape &s, uint32_t to,
                                                      const uint8_t *code, const uint4 r, uint2 *v, Emit &&emit)
{
    uint64_t ch = 0, cl = 0;
    const uint32_t cls = edit_site(g, s, r.x, r.y, r.z, &ch, &cl);
    if (cls != kEffDefined) {
        *v = make_uint2(kEffectsUndefined, kEffectsUndefined);
        return cls;
    }
    const uint32_t mask = edit_mask(ch, cl, s);
    uint32_t w0 = 0, w1 = 0;
    if (mask && cds.n) {
        const uint32_t g0 = g.contig_off[r.x] + edit_window_first(r.y, r.z, s);  // (defined: r.x is a contig)
        effects_row(g, cds, s, to, code, g0, r.z, mask, &w0, &w1, emit);
    }
    *v = make_uint2(w0, w1);
    return cls;
}

// exclusive prefix of v over the lanes of the wave; *total = the wave's sum (cross-lane moves, no LDS memory)
__device__ __forceinline__ uint32_t effects_wave_exclusive(uint32_t v, uint32_t lane, uint32_t *total)
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

// the wave's sum of v in every lane
__device__ __forceinline__ uint32_t effects_wave_sum(uint32_t v)
{
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d, kWave);
    return v;
}

}  // namespace

// out[i] = ROW of loci[i], grid-stride over the 64-bit count in steps of whole waves; one coalesced 8-byte store per lane.
// The candidates' classes and the candidates with an effect are counted per wave (a ballot per counter and step); the
// effects by class are added up per lane and summed over the wave at the end.  All of them are added per workgroup in LDS
// and go out with one atomic add per counter and workgroup.
__global__ __launch_bounds__(kEffectsThreads) void effects_rows_kernel(const EffectsArgs a)
{
    __shared__ unsigned long long s_count[kEffectsCounts];
    __shared__ uint8_t s_code[64];
    if (threadIdx.x < kEffectsCounts) s_count[threadIdx.x] = 0;
    effects_code_to_lds(a.code, s_code);
    block_sync();
    const uint32_t lane = threadIdx.x % kWave;
    const unsigned long long stride = (unsigned long long)gridDim.x * kEffectsThreads;
    uint32_t seen[kEffClasses + 1] = {};  // wave-uniform
    uint32_t mine[kEffectClasses] = {};   // this lane's effects by class
    const unsigned long long first = (unsigned long long)blockIdx.x * kEffectsThreads + threadIdx.x;
    uint4 ahead = first < a.n ? a.loci[first] : make_uint4(0u, 0u, 0u, 0u);  // the next step's locus is on its way during a step
    for (unsigned long long base = first - lane; base < a.n; base += stride) {
        const unsigned long long i = base + lane;
        const bool live = i < a.n;
        const uint4 r = ahead;
        if (i + stride < a.n) ahead = a.loci[i + stride];
        uint32_t cls = kEffClasses;
        bool any = false;
        if (live) {
            uint2 v;
            cls = effects_candidate(a.g, a.cds, a.shape, a.to, s_code, r, &v, [](uint32_t, uint32_t, uint32_t) {});
            if (cls == kEffDefined) {
                any = (v.x & 0x3FFFFFFFu) != 0u;
#pragma unroll
                for (uint32_t k = 0; k < kEffectClasses; ++k) mine[k] += v.x >> (5u * k) & 31u;
            }
            a.out[i] = v;
        }
#pragma unroll
        for (uint32_t k = 0; k < kEffClasses; ++k) seen[k] += (uint32_t)__popcll(__ballot(cls == k));
        seen[kEffClasses] += (uint32_t)__popcll(__ballot(any));
    }
    // (a wave takes at most 2^32 / 64 steps of 64 candidates with at most 16 effects each, and the grid has at least 8
    // workgroups whenever a wave takes more than one step: a wave's sum stays below 2^32)
    uint32_t sums[kEffectClasses];
#pragma unroll
    for (uint32_t k = 0; k < kEffectClasses; ++k) sums[k] = effects_wave_sum(mine[k]);
    if (lane == 0) {
#pragma unroll
        for (uint32_t k = 0; k <= kEffClasses; ++k)
            if (seen[k]) atomicAdd(&s_count[k], (unsigned long long)seen[k]);
#pragma unroll
        for (uint32_t k = 0; k < kEffectClasses; ++k)
            if (sums[k]) atomicAdd(&s_count[kEffClasses + 1 + k], (unsigned long long)sums[k]);
    }
    block_sync();
    if (threadIdx.x < kEffectsCounts && s_count[threadIdx.x]) atomicAdd(&a.stats[threadIdx.x], s_count[threadIdx.x]);
}

// kWrite = false: tile_count[i] = the effects of tile i - the six fields of word 0 over its candidates, read from the rows.
// kWrite = true: every effect to tile_off[i] + the effects of the tile's earlier steps + the effects of the lanes below (an
// exclusive scan over the wave) + its place among the candidate's own, which is the order of the walk.  Only a lane with
// effects reads its locus and repeats the walk, over word 1 of its row - no site is read.  One wave per tile of kEditTile
// candidates; no append cursor: the bytes depend on the rows, the loci, the segments and the planes only.  The coverage is
// taken here: one integer add and one integer min per stop_gained effect.
template <bool kWrite> __global__ __launch_bounds__(kEffectsThreads) void effects_records_kernel(const EffectsRecordArgs a)
{
    __shared__ uint8_t s_code[64];
    if (kWrite) {
        effects_code_to_lds(a.code, s_code);
        block_sync();
    }
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
        const uint32_t mine = effects_count(v.x, v.y);
        uint32_t total;
        const uint32_t before = effects_wave_exclusive(mine, lane, &total);
        if (kWrite) {
            if (mine) {
                const uint4 r = a.loci[i];
                const uint32_t g0 = a.g.contig_off[r.x] + edit_window_first(r.y, r.z, a.shape);  // (a row with effects: r.x is a contig)
                unsigned long long o = at + before;
                const unsigned long long end = o + mine;
                uint32_t w0, w1;
                effects_row(a.g, a.cds, a.shape, a.to, s_code, g0, r.z, v.y, &w0, &w1, [&](uint32_t tx, uint32_t codon, uint32_t info) {
                    if (o >= end) return;  // (the walk gives what the row counted; never past this lane's share)
                    if (a.effects) a.effects[o] = make_uint4((uint32_t)i, tx, codon, info);
                    ++o;
                    if (a.cov_count && (info >> 12 & 7u) == kEffectStopGained && tx < a.n_tx) {
                        atomicAdd(&a.cov_count[tx], 1u);
                        atomicMin(&a.cov_min[tx], codon);
                    }
                });
            }
            at += total;
        } else {
            count += total;
        }
    }
    if (!kWrite && lane == 0) a.tile_count[item] = count;
}

// kWrite = false: tile_count[i] = the candidates of tile work[i] that pass FILTER (effects_keep).  kWrite = true: the same
// test again, every survivor's code and locus to tile_off[i] + its rank in the tile - the input's order.  One wave per tile
// of kEditTile candidates; the rank inside a step is the survivors in the lanes below (a ballot), no atomic.
template <bool kWrite> __global__ __launch_bounds__(kEffectsThreads) void effects_filter_kernel(const EffectsFilterArgs a)
{
    __shared__ uint8_t s_code[64];
    effects_code_to_lds(a.code, s_code);
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
            const uint32_t cls = effects_candidate(a.g, a.cds, a.shape, a.to, s_code, r, &v, [](uint32_t, uint32_t, uint32_t) {});
            keep = effects_keep(cls, v.x, a.require, a.forbid);
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

hipError_t launch_effects_rows(const EffectsArgs &args, int n_cus, hipStream_t stream)
{
    if (args.n == 0) return hipSuccess;
    // 8 workgroups of 4 waves per CU fill every SIMD's 8 wave slots; fewer when the candidates do not need them (launch_edit_rows)
    const unsigned long long want = (args.n + kEffectsThreads - 1) / kEffectsThreads;
    const unsigned long long cap = (unsigned long long)(n_cus > 0 ? n_cus : 256) * 8u;
    const dim3 grid((uint32_t)(want < cap ? want : cap)), block(kEffectsThreads);
    hipLaunchKernelGGL(effects_rows_kernel, grid, block, 0, stream, args);
    return hipGetLastError();
}

hipError_t launch_effects_records(const EffectsRecordArgs &args, bool write, hipStream_t stream)
{
    if (args.n_work == 0) return hipSuccess;
    const dim3 grid((args.n_work + kWavesPerGroup - 1) / kWavesPerGroup), block(kEffectsThreads);
    if (write) hipLaunchKernelGGL((effects_records_kernel<true>), grid, block, 0, stream, args);
    else hipLaunchKernelGGL((effects_records_kernel<false>), grid, block, 0, stream, args);
    return hipGetLastError();
}

hipError_t launch_effects_filter(const EffectsFilterArgs &args, bool write, hipStream_t stream)
{
    if (args.n_work == 0) return hipSuccess;
    const dim3 grid((args.n_work + kWavesPerGroup - 1) / kWavesPerGroup), block(kEffectsThreads);
    if (write) hipLaunchKernelGGL((effects_filter_kernel<true>), grid, block, 0, stream, args);
    else hipLaunchKernelGGL((effects_filter_kernel<false>), grid, block, 0, stream, args);
    return hipGetLastError();
}

}  // namespace vsc
