// vsc_motif.hip - restriction sites and IUPAC motifs in candidate guides on the device: motif_rows_kernel over
// loci (vsc_loci_motifs, vsc_guides_motifs, vsc_pattern_guides_motifs), motif_filter_kernel<kWrite> over a candidate list (the
// two passes of vsc_guides_filter_motifs).  The class of a candidate, its context and its row are motif_context and motif_row
// of vsc_motif.h - the functions vsc_motif_text and the stand-alone check call on the host.
//
// Both kernels take one candidate per lane and step, as the kernels of vsc_fold.hip do: one 16-byte locus load, the bounds
// tests in the order of the classes, the context as a window per plane, reversed and complemented on '-'.  The launch's
// patterns - at most 126 of 48 bytes, the same for every lane - are copied into LDS once per workgroup; a pattern's fields are
// read at a wave-wide address and made scalars, so its accept sets select among wave-wide masks and every shift count is the
// launch's.  The loops have the launch's trip count on every lane; a lane whose candidate has no context runs them on zeros
// and drops the result.  Integers only: no MFMA, no floating point, no atomics but the counts.
#include "vsc_internal.h"
#include "vsc_device.h"

namespace vsc {

namespace {

constexpr int kMotifThreads = kWave * kWavesPerGroup;
static_assert(kMotifTile % kWave == 0, "a tile is a whole number of steps of one wave");
static_assert(sizeof(MotifPattern) == 48 && sizeof(MotifPattern) % sizeof(uint4) == 0, "a pattern is three 16-byte reads");
static_assert(sizeof(MotifRow) == 24, "a row is three 64-bit words");

// the launch's patterns into LDS; every thread of the workgroup calls it, a barrier follows
__device__ __forceinline__ void motif_stage_patterns(MotifPattern *s_pat, const MotifPattern *pat, uint32_t n_pat)
{
    constexpr uint32_t kWords = sizeof(MotifPattern) / sizeof(uint4);
    const uint4 *src = (const uint4 *)pat;
    uint4 *dst = (uint4 *)s_pat;
    const uint32_t n = (n_pat < kMotifMaxPatterns ? n_pat : kMotifMaxPatterns) * kWords;
    for (uint32_t c = threadIdx.x; c < n; c += kMotifThreads) dst[c] = src[c];
    block_sync();
}

// candidate r: its class; *v = its row, the undefined row unless the class is kEffDefined
__device__ __forceinline__ uint32_t motif_candidate(const EffPlanes &g, const MotifShape &s, const MotifTable &t, const uint4 r, MotifRow *v)
{
    uint64_t ch = 0, cl = 0;
    const uint32_t cls = motif_context(g, s, r.x, r.y, r.z, &ch, &cl);
    const MotifRow row = motif_row(ch, cl, s, t);
    *v = cls == kEffDefined ? row : MotifRow{kMotifUndefined, kMotifUndefined, kMotifUndefined};
    return cls;
}

}  // namespace

// out[i] = the row of loci[i], grid-stride over the 64-bit count in steps of whole waves; one 24-byte store per lane.  The
// classes and the three "any bit" counts are counted per wave (a ballot each and step), added per workgroup in LDS and go out
// with one atomic add per count and workgroup.  The totals per motif, where asked for: a ballot per motif says whether any
// lane of the wave holds its bit at all - most steps of most motifs end there -, three more count its lanes; lane 0 adds them
// to the workgroup's counters in LDS, which go out with one atomic add per motif, column and workgroup.  Sums of integers: no
// output bit depends on the order.
__global__ __launch_bounds__(kMotifThreads) void motif_rows_kernel(const MotifArgs a)
{
    __shared__ unsigned long long s_count[kMotifStats];
    __shared__ unsigned long long s_total[3 * kMotifMaxMotifs];
    __shared__ MotifPattern s_pat[kMotifMaxPatterns];
    if (threadIdx.x < kMotifStats) s_count[threadIdx.x] = 0;
    if (threadIdx.x < 3 * kMotifMaxMotifs) s_total[threadIdx.x] = 0;
    motif_stage_patterns(s_pat, a.tab.pat, a.tab.n_pat);
    MotifTable tab = a.tab;
    tab.pat = s_pat;
    tab.n_pat = a.tab.n_pat < kMotifMaxPatterns ? a.tab.n_pat : kMotifMaxPatterns;
    const uint32_t n_motifs = a.tab.n_motifs < kMotifMaxMotifs ? a.tab.n_motifs : kMotifMaxMotifs;
    const uint32_t lane = threadIdx.x % kWave;
    const unsigned long long stride = (unsigned long long)gridDim.x * kMotifThreads;
    unsigned long long seen = 0;  // lane k < kMotifStats: the wave's count k (eight scalars less than an array of them)
    const unsigned long long first = (unsigned long long)blockIdx.x * kMotifThreads + threadIdx.x;
    uint4 ahead = first < a.n ? a.loci[first] : make_uint4(0u, 0u, 0u, 0u);  // the next step's locus is on its way during a step
    for (unsigned long long base = first - lane; base < a.n; base += stride) {
        const unsigned long long i = base + lane;
        const bool live = i < a.n;
        const uint4 r = ahead;
        if (i + stride < a.n) ahead = a.loci[i + stride];
        uint32_t cls = kEffClasses;
        MotifRow v{0ull, 0ull, 0ull};
        if (live) {
            cls = motif_candidate(a.g, a.shape, tab, r, &v);
            a.out[i] = v;
        }
        if (cls != kEffDefined) v = MotifRow{0ull, 0ull, 0ull};
        const uint64_t only = v.cut & ~v.elsewhere;
        // (every ballot is taken by the whole wave, in front of the lane's choice of its own count)
#pragma unroll
        for (uint32_t k = 0; k < kEffClasses; ++k) {
            const uint32_t in_class = (uint32_t)__popcll(__ballot(cls == k));
            seen += lane == k ? in_class : 0u;
        }
        const uint32_t with_construct = (uint32_t)__popcll(__ballot(v.construct != 0ull));
        const uint32_t with_cut = (uint32_t)__popcll(__ballot(v.cut != 0ull));
        const uint32_t with_only = (uint32_t)__popcll(__ballot(only != 0ull));
        seen += lane == kEffClasses ? with_construct : lane == kEffClasses + 1 ? with_cut : lane == kEffClasses + 2 ? with_only : 0u;
        if (a.totals) {
            const uint64_t any = v.construct | v.cut;
            for (uint32_t m = 0; m < n_motifs; ++m) {
                const uint64_t bit = 1ull << m;  // (wave-uniform)
                if (__ballot((any & bit) != 0ull) == 0ull) continue;
                const uint32_t c0 = (uint32_t)__popcll(__ballot((v.construct & bit) != 0ull));
                const uint32_t c1 = (uint32_t)__popcll(__ballot((v.cut & bit) != 0ull));
                const uint32_t c2 = (uint32_t)__popcll(__ballot((only & bit) != 0ull));
                if (lane == 0) {
                    if (c0) atomicAdd(&s_total[3 * m], (unsigned long long)c0);
                    if (c1) atomicAdd(&s_total[3 * m + 1], (unsigned long long)c1);
                    if (c2) atomicAdd(&s_total[3 * m + 2], (unsigned long long)c2);
                }
            }
        }
    }
    if (lane < kMotifStats && seen) atomicAdd(&s_count[lane], seen);
    block_sync();
    if (threadIdx.x < kMotifStats && s_count[threadIdx.x]) atomicAdd(&a.stats[threadIdx.x], s_count[threadIdx.x]);
    if (a.totals && threadIdx.x < 3 * n_motifs && s_total[threadIdx.x]) atomicAdd(&a.totals[threadIdx.x], s_total[threadIdx.x]);
}

// kWrite = false: tile_count[i] = the candidates of tile work[i] that pass the limits (motif_keep).  kWrite = true: the same
// test again, every survivor's code and locus to tile_off[i] + its rank in the tile - the input's order.  One wave per tile
// of kMotifTile candidates, kMotifTile / 64 steps; the rank inside a step is the survivors in the lanes below (a ballot), no
// atomic: the bytes depend on the input, the shape, the flanks, the motifs and the limits only.
template <bool kWrite> __global__ __launch_bounds__(kMotifThreads) void motif_filter_kernel(const MotifFilterArgs a)
{
    __shared__ MotifPattern s_pat[kMotifMaxPatterns];
    motif_stage_patterns(s_pat, a.tab.pat, a.tab.n_pat);  // (in front of the wave's way out: every wave meets the barrier)
    MotifTable tab = a.tab;
    tab.pat = s_pat;
    tab.n_pat = a.tab.n_pat < kMotifMaxPatterns ? a.tab.n_pat : kMotifMaxPatterns;
    const uint32_t lane = threadIdx.x % kWave;
    const uint32_t item = blockIdx.x * kWavesPerGroup + threadIdx.x / kWave;  // wave-uniform
    if (item >= a.n_work) return;
    const uint32_t tile = a.work ? a.work[item] : item;
    const unsigned long long first = (unsigned long long)tile * kMotifTile;
    unsigned long long at = kWrite ? a.tile_off[item] : 0;
    uint32_t count = 0;
    for (uint32_t step = 0; step < kMotifTile / kWave; ++step) {
        const unsigned long long base = first + (unsigned long long)step * kWave;
        if (base >= a.n) break;
        const unsigned long long i = base + lane;
        bool keep = false;
        uint4 r = make_uint4(0u, 0u, 0u, 0u);
        if (i < a.n) {
            r = a.in_loci[i];
            MotifRow v;
            const uint32_t cls = motif_candidate(a.g, a.shape, tab, r, &v);
            keep = motif_keep(cls, v, a.limits);
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

hipError_t launch_motif_rows(const MotifArgs &args, int n_cus, uint32_t groups_per_cu, hipStream_t stream)
{
    if (args.n == 0) return hipSuccess;
    // 8 workgroups of 4 waves per CU fill every SIMD's 8 wave slots; fewer when the candidates do not need them
    const unsigned long long want = (args.n + kMotifThreads - 1) / kMotifThreads;
    const unsigned long long cap = (unsigned long long)(n_cus > 0 ? n_cus : 256) * (groups_per_cu ? groups_per_cu : kMotifGroupsPerCu);
    const dim3 grid((uint32_t)(want < cap ? want : cap)), block(kMotifThreads);
    hipLaunchKernelGGL(motif_rows_kernel, grid, block, 0, stream, args);
    return hipGetLastError();
}

hipError_t launch_motif_filter(const MotifFilterArgs &args, bool write, hipStream_t stream)
{
    if (args.n_work == 0) return hipSuccess;
    const dim3 grid((args.n_work + kWavesPerGroup - 1) / kWavesPerGroup), block(kMotifThreads);
    if (write) hipLaunchKernelGGL((motif_filter_kernel<true>), grid, block, 0, stream, args);
    else hipLaunchKernelGGL((motif_filter_kernel<false>), grid, block, 0, stream, args);
    return hipGetLastError();
}

}  // namespace vsc
