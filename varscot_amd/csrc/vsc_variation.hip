// vsc_variation.hip - known variation under candidate guides on the device: the four launches that turn the
// caller's variants into the walk's records and the lookup's block table, var_rows_kernel over loci (vsc_loci_variation,
// vsc_guides_variation, vsc_pattern_guides_variation), var_pairs_kernel<kWrite> over the rows it left (the two passes behind the
// pairs and the coverage), var_filter_kernel<kWrite> over a candidate list (the two passes of vsc_guides_filter_variation).  The
// class of a candidate, the lookup, the relation of a variant to a site, the row's arithmetic and the filter's rule are
// var_site, var_first, var_touch, var_add and var_keep of vsc_variation.h - the functions vsc_variation_host and the stand-alone
// check call on the host.
//
// The rows and the filter kernel take one candidate per lane and step, as the kernels of vsc_edit.hip do: one 16-byte locus load
// (the next step's is on its way during a step), the bounds tests in the order of the classes, then the lookup: ONE load of two
// adjacent block-table entries and a lower bound over `reach` confined to them - at the default block of 256 positions and 10^8
// variants about three dependent loads where the full lower bound takes 27 - and a walk of one 16-byte record per step.
// Integers only: no MFMA, no floating point, no LDS but the class counts, no atomics but the class counts and the coverage
// (integer adds, which commute).
#include "vsc_internal.h"
#include "vsc_device.h"

namespace vsc {

namespace {

constexpr int kVarThreads = kWave * kWavesPerGroup;
static_assert(kEditTile % kWave == 0, "a tile is a whole number of steps of one wave");
static_assert(sizeof(VarRec) == sizeof(uint4), "a record is one 16-byte load");

// inclusive prefix maximum of v over the lanes of the wave (cross-lane moves, no LDS memory)
__device__ __forceinline__ uint32_t var_wave_max_inclusive(uint32_t v, uint32_t lane)
{
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)v, d, kWave);
        if (lane >= (uint32_t)d && o > v) v = o;
    }
    return v;
}

// exclusive prefix of v over the lanes of the wave; *total = the wave's sum
__device__ __forceinline__ uint32_t var_wave_exclusive(uint32_t v, uint32_t lane, uint32_t *total)
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

// the wave's sum of v in 64 bits (every lane gets it)
__device__ __forceinline__ unsigned long long var_wave_sum64(unsigned long long v)
{
#pragma unroll
    for (int d = kWave / 2; d >= 1; d >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d, kWave), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d, kWave);
        v += (unsigned long long)hi << 32 | lo;
    }
    return v;
}

// the end (global, exclusive) of the caller's record in[k], 0 behind the array
__device__ __forceinline__ uint32_t var_end_of(const VarBuildArgs &a, unsigned long long k, uint4 *in)
{
    if (k >= a.n) return 0u;
    *in = *(const uint4 *)&a.rec[k];  // { contig, pos, span_alt, weight }
    return a.contig_off[in->x] + in->y + (in->z & 0xFFFFu);
}

// candidate r: its class; *row = the four words, kVarUndefined each unless the class is kEffDefined
__device__ __forceinline__ uint32_t var_candidate(const EffPlanes &g, const VarShape &s, const VarTable &t, const uint4 r, uint4 *row)
{
    const uint32_t cls = var_site(g, s, r.x, r.y, r.z);
    if (cls != kEffDefined) {
        *row = make_uint4(kVarUndefined, kVarUndefined, kVarUndefined, kVarUndefined);
        return cls;
    }
    VarRow v{0u, 0u, 0u, 0ull};
    if (t.n) v = var_row(t, g.contig_off[r.x] + r.y, r.z, s, nullptr);  // (defined: r.x is a contig)
    *row = make_uint4(v.by_zone, v.silent, var_cost(v), v.max_weight);
    return cls;
}

}  // namespace

// tile_max[t] = the largest end of the variants of tile t; one wave per tile of kEditTile variants
__global__ __launch_bounds__(kVarThreads) void var_ends_kernel(const VarBuildArgs a)
{
    const uint32_t lane = threadIdx.x % kWave;
    const uint32_t tile = blockIdx.x * kWavesPerGroup + threadIdx.x / kWave;  // wave-uniform
    if (tile >= a.n_tiles) return;
    uint32_t best = 0;
    for (uint32_t step = 0; step < kEditTile / kWave; ++step) {
        uint4 in;
        const uint32_t end = var_end_of(a, (unsigned long long)tile * kEditTile + step * kWave + lane, &in);
        if (end > best) best = end;
    }
    best = var_wave_max_inclusive(best, lane);
    if (lane == kWave - 1) a.tile_max[tile] = best;
}

// tile_max[t] = the largest end of the tiles in front of t (0 for the first): ONE wave, 64 tiles per step and a carry
__global__ __launch_bounds__(kWave) void var_scan_kernel(const VarBuildArgs a)
{
    const uint32_t lane = threadIdx.x;
    uint32_t carry = 0;  // wave-uniform
    for (uint32_t base = 0; base < a.n_tiles; base += kWave) {
        const uint32_t t = base + lane;
        const uint32_t own = t < a.n_tiles ? a.tile_max[t] : 0u;
        const uint32_t incl = var_wave_max_inclusive(own, lane);
        uint32_t before = (uint32_t)__shfl_up((int)incl, 1, kWave);
        if (lane == 0 || before < carry) before = carry;
        if (t < a.n_tiles) a.tile_max[t] = before;
        const uint32_t last = (uint32_t)__shfl((int)incl, kWave - 1, kWave);
        if (last > carry) carry = last;
    }
}

// rec[k] = { gpos, span_alt, weight, reach } in place of the caller's record - every lane reads its own 16 bytes before it
// writes them; reach = max(what the tiles in front reach, the ends up to and including k).  One wave per tile.
__global__ __launch_bounds__(kVarThreads) void var_records_kernel(const VarBuildArgs a)
{
    const uint32_t lane = threadIdx.x % kWave;
    const uint32_t tile = blockIdx.x * kWavesPerGroup + threadIdx.x / kWave;  // wave-uniform
    if (tile >= a.n_tiles) return;
    uint32_t carry = a.tile_max[tile];
    for (uint32_t step = 0; step < kEditTile / kWave; ++step) {
        const unsigned long long k = (unsigned long long)tile * kEditTile + step * kWave + lane;
        uint4 in = make_uint4(0u, 0u, 0u, 0u);
        const uint32_t end = var_end_of(a, k, &in);
        uint32_t reach = var_wave_max_inclusive(end, lane);
        if (reach < carry) reach = carry;
        if (k < a.n) {
            const uint32_t span = in.z & 0xFFFFu;
            a.rec[k] = VarRec{end - span, in.z, in.w, reach};
        }
        carry = (uint32_t)__shfl((int)reach, kWave - 1, kWave);
    }
}

// first[b] = the first k with reach[k] > b << bits, b = 0 .. n_blocks: one lower bound per entry
__global__ __launch_bounds__(kVarThreads) void var_first_kernel(const VarBuildArgs a)
{
    const unsigned long long stride = (unsigned long long)gridDim.x * kVarThreads;
    for (unsigned long long b = (unsigned long long)blockIdx.x * kVarThreads + threadIdx.x; b <= a.n_blocks; b += stride)
        a.first[b] = var_first_reach(a.rec, 0u, a.n, b << a.bits);
}

// out[i] = the row of loci[i], grid-stride over the 64-bit count in steps of whole waves; one coalesced 16-byte store per lane.
// The classes and the candidates with a disrupting variant are counted per wave (a ballot per counter and step), added per
// workgroup in LDS and go out with one atomic add per counter and workgroup.
__global__ __launch_bounds__(kVarThreads) void var_rows_kernel(const VarArgs a)
{
    __shared__ unsigned long long s_count[kVarCounts];
    if (threadIdx.x < kVarCounts) s_count[threadIdx.x] = 0;
    block_sync();
    const uint32_t lane = threadIdx.x % kWave;
    const unsigned long long stride = (unsigned long long)gridDim.x * kVarThreads;
    uint32_t seen[kVarCounts] = {};  // wave-uniform
    const unsigned long long first = (unsigned long long)blockIdx.x * kVarThreads + threadIdx.x;
    uint4 ahead = first < a.n ? a.loci[first] : make_uint4(0u, 0u, 0u, 0u);  // the next step's locus is on its way during a step
    for (unsigned long long base = first - lane; base < a.n; base += stride) {
        const unsigned long long i = base + lane;
        const bool live = i < a.n;
        const uint4 r = ahead;
        if (i + stride < a.n) ahead = a.loci[i + stride];
        uint32_t cls = kEffClasses;
        bool hit = false;
        if (live) {
            uint4 v;
            cls = var_candidate(a.g, a.shape, a.table, r, &v);
            hit = cls == kEffDefined && v.x != 0u;
            a.out[i] = v;
        }
#pragma unroll
        for (uint32_t k = 0; k < kEffClasses; ++k) seen[k] += (uint32_t)__popcll(__ballot(cls == k));
        seen[kEffClasses] += (uint32_t)__popcll(__ballot(hit));
    }
    if (lane == 0) {
#pragma unroll
        for (uint32_t k = 0; k < kVarCounts; ++k)
            if (seen[k]) atomicAdd(&s_count[k], (unsigned long long)seen[k]);
    }
    block_sync();
    if (threadIdx.x < kVarCounts && s_count[threadIdx.x]) atomicAdd(&a.stats[threadIdx.x], s_count[threadIdx.x]);
}

// kWrite = false: tile_count[i] = the pairs of tile i, read from the rows: the bytes of by_zone plus `silent` - a row with a
// byte at its bound repeats its walk to count.  kWrite = true: every pair to tile_off[i] + the pairs of the tile's earlier steps
// + the pairs of the lanes below (an exclusive scan over the wave) + its place among the candidate's own, which is the order of
// the walk over the variants: ascending (candidate, variant).  Only a lane with pairs reads its locus and repeats the lookup.
// One wave per tile of kEditTile candidates; no append cursor: the bytes depend on the rows, the loci and the variants only.
// The coverage is taken here: one integer add per pair.
template <bool kWrite> __global__ __launch_bounds__(kVarThreads) void var_pairs_kernel(const VarPairArgs a)
{
    const uint32_t lane = threadIdx.x % kWave;
    const uint32_t item = blockIdx.x * kWavesPerGroup + threadIdx.x / kWave;  // wave-uniform
    if (item >= a.n_work) return;
    const unsigned long long first = (unsigned long long)item * kEditTile;
    unsigned long long at = kWrite ? a.tile_off[item] : 0;
    unsigned long long count = 0;
    for (uint32_t step = 0; step < kEditTile / kWave; ++step) {
        const unsigned long long base = first + (unsigned long long)step * kWave;
        if (base >= a.n) break;
        const unsigned long long i = base + lane;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (i < a.n) v = a.rows[i];
        const bool defined = !(v.x == kVarUndefined && v.y == kVarUndefined && v.z == kVarUndefined && v.w == kVarUndefined);
        unsigned long long mine = 0;
        uint4 r = make_uint4(0u, 0u, 0u, 0u);
        uint32_t g0 = 0;
        if (defined && (v.x | v.y)) {
            const bool counts = var_row_counts(v.x);
            if (kWrite || !counts) {
                r = a.loci[i];
                g0 = a.contig_off[r.x] + r.y;  // (a defined row: r.x is a contig)
            }
            if (counts) mine = (unsigned long long)(v.x & 0xFFu) + (v.x >> 8 & 0xFFu) + (v.x >> 16 & 0xFFu) + (v.x >> 24) + v.y;
            else {
                uint64_t walked = 0;
                (void)var_row(a.table, g0, r.z, a.shape, &walked);
                mine = walked;
            }
        }
        if (kWrite) {
            uint32_t total;  // (the write pass runs only when all pairs of the call fit 32 bits)
            const uint32_t before = var_wave_exclusive((uint32_t)mine, lane, &total);
            if (mine) {
                unsigned long long o = at + before;
                for (uint32_t k = var_first(a.table, g0); k < a.table.n; ++k) {
                    const VarRec rec = a.table.rec[k];
                    if (rec.gpos >= g0 + a.shape.site_len) break;
                    uint32_t info;
                    if (!var_touch(rec, g0, r.z, a.shape, &info)) continue;
                    if (a.pairs) a.pairs[o] = make_uint4((uint32_t)i, k, info, rec.weight);
                    ++o;
                    if (a.coverage) atomicAdd(&a.coverage[2ull * k + (info >> 18 & 1u)], 1u);
                }
            }
            at += total;
        } else {
            count += var_wave_sum64(mine);
        }
    }
    if (!kWrite && lane == 0) a.tile_count[item] = count > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)count;
}

// kWrite = false: tile_count[i] = the candidates of tile work[i] that pass FILTER (var_keep).  kWrite = true: the same test
// again, every survivor's code and locus to tile_off[i] + its rank in the tile - the input's order.  One wave per tile of
// kEditTile candidates; the rank inside a step is the survivors in the lanes below (a ballot), no atomic.
template <bool kWrite> __global__ __launch_bounds__(kVarThreads) void var_filter_kernel(const VarFilterArgs a)
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
            uint4 v;
            const uint32_t cls = var_candidate(a.g, a.shape, a.table, r, &v);
            keep = var_keep(cls, v.x, v.z, a.filter);
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

// *out += the variants with a pair of either kind: a ballot per step, one atomic add per wave that saw any
__global__ __launch_bounds__(kVarThreads) void var_covered_kernel(const uint32_t *coverage, uint32_t n_v, unsigned long long *out)
{
    const uint32_t lane = threadIdx.x % kWave;
    const unsigned long long stride = (unsigned long long)gridDim.x * kVarThreads;
    uint32_t seen = 0;  // wave-uniform
    for (unsigned long long base = (unsigned long long)blockIdx.x * kVarThreads + threadIdx.x - lane; base < n_v; base += stride) {
        const unsigned long long i = base + lane;
        seen += (uint32_t)__popcll(__ballot(i < n_v && (coverage[2 * i] | coverage[2 * i + 1]) != 0u));
    }
    if (lane == 0 && seen) atomicAdd(out, (unsigned long long)seen);
}

namespace {

// 8 workgroups of 4 waves per CU fill every SIMD's 8 wave slots; fewer when the items do not need them (launch_edit_rows)
uint32_t var_grid(unsigned long long items, int n_cus)
{
    const unsigned long long want = (items + kVarThreads - 1) / kVarThreads;
    const unsigned long long cap = (unsigned long long)(n_cus > 0 ? n_cus : 256) * 8u;
    return (uint32_t)(want < cap ? want : cap);
}

}  // namespace

hipError_t launch_var_build(const VarBuildArgs &args, int n_cus, hipStream_t stream)
{
    if (args.n_tiles) {
        const dim3 grid((args.n_tiles + kWavesPerGroup - 1) / kWavesPerGroup), block(kVarThreads);
        hipLaunchKernelGGL(var_ends_kernel, grid, block, 0, stream, args);
        hipLaunchKernelGGL(var_scan_kernel, dim3(1), dim3(kWave), 0, stream, args);
        hipLaunchKernelGGL(var_records_kernel, grid, block, 0, stream, args);
    }
    hipLaunchKernelGGL(var_first_kernel, dim3(var_grid((unsigned long long)args.n_blocks + 1u, n_cus)), dim3(kVarThreads), 0, stream, args);
    return hipGetLastError();
}

hipError_t launch_var_rows(const VarArgs &args, int n_cus, hipStream_t stream)
{
    if (args.n == 0) return hipSuccess;
    hipLaunchKernelGGL(var_rows_kernel, dim3(var_grid(args.n, n_cus)), dim3(kVarThreads), 0, stream, args);
    return hipGetLastError();
}

hipError_t launch_var_pairs(const VarPairArgs &args, bool write, hipStream_t stream)
{
    if (args.n_work == 0) return hipSuccess;
    const dim3 grid((args.n_work + kWavesPerGroup - 1) / kWavesPerGroup), block(kVarThreads);
    if (write) hipLaunchKernelGGL((var_pairs_kernel<true>), grid, block, 0, stream, args);
    else hipLaunchKernelGGL((var_pairs_kernel<false>), grid, block, 0, stream, args);
    return hipGetLastError();
}

hipError_t launch_var_covered(const uint32_t *coverage, uint32_t n_v, unsigned long long *out, int n_cus, hipStream_t stream)
{
    if (n_v == 0) return hipSuccess;
    hipLaunchKernelGGL(var_covered_kernel, dim3(var_grid(n_v, n_cus)), dim3(kVarThreads), 0, stream, coverage, n_v, out);
    return hipGetLastError();
}

hipError_t launch_var_filter(const VarFilterArgs &args, bool write, hipStream_t stream)
{
    if (args.n_work == 0) return hipSuccess;
    const dim3 grid((args.n_work + kWavesPerGroup - 1) / kWavesPerGroup), block(kVarThreads);
    if (write) hipLaunchKernelGGL((var_filter_kernel<true>), grid, block, 0, stream, args);
    else hipLaunchKernelGGL((var_filter_kernel<false>), grid, block, 0, stream, args);
    return hipGetLastError();
}

}  // namespace vsc
