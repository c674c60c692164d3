// vsc_pick.hip - the per-target pick with spacing on the device (the definition: vsc_pick.h).  Five kernels:
//   pick_mark_kernel     one candidate per lane and step: its class, its target (the given array, or regions_locate + group),
//                        the class counts (ballots) and the per-target counts (one atomic add per run of equal targets in a wave)
//   (enum_scan_kernel)   the per-target counts to segment offsets
//   pick_scatter_kernel  one 20-byte record per eligible candidate into its target's segment, through an append cursor per
//                        target; the order inside a segment is the order in which waves arrive and DOES NOT MATTER: the
//                        select takes the first unblocked record under BEFORE, a total order on (key, index), in every round
//   pick_select_kernel   one wave per target: segments of <= 256 records from registers, larger ones in a loop over memory
//   pick_rank_kernel     rank[] from the picks;  pick_gather_kernel<kWrite>: the `picked` object, in input order
// Plain HIP C++: no MFMA, no inline assembly, integers only.  Every index is checked against its array's length before use.
#include "vsc_pick_device.h"
#include "vsc_device.h"

namespace vsc {

namespace {

constexpr int kPickThreads = kWave * kWavesPerGroup;
static_assert(kPickTile % kWave == 0, "a tile is a whole number of steps of one wave");
static_assert(kPickPerLane <= 32, "a lane's open records are one 32-bit mask");

// The run of equal t around this lane (all 64 lanes call it): *head = the run's first lane, *len = lanes from this one to the
// run's end (the run length on the head lane).
__device__ __forceinline__ void wave_run(uint32_t t, uint32_t lane, uint32_t *head, uint32_t *len)
{
    const uint32_t prev = __shfl_up(t, 1);
    const uint64_t heads = __ballot(lane == 0u || prev != t);  // bit 0 is always set
    *head = 63u - (uint32_t)__clzll((long long)(heads & (~0ull >> (63u - lane))));
    const uint64_t above = lane == 63u ? 0ull : heads & (~0ull << (lane + 1u));
    *len = (above ? (uint32_t)__ffsll((unsigned long long)above) - 1u : 64u) - lane;
}

// candidate i = locus r: its class, and its target when the class is kPickEligible
__device__ __forceinline__ uint32_t pick_candidate(const PickArgs &a, unsigned long long i, const uint4 r, uint32_t *target)
{
    const uint32_t contig = r.x, pos = r.y, strand = r.z;
    uint32_t len = 0, t = kPickNone;
    if (contig < a.n_contigs) {
        const uint32_t off = a.contig_off[contig];
        len = a.contig_end[contig] - off;
        if (a.target) {
            t = a.target[i];
        } else if (pos < len) {  // vsc_regions_locate of (contig, pos): a window at the contig's end is cut off there
            const uint32_t left = len - pos, wl = left < (uint32_t)VSC_READ_LEN ? left : (uint32_t)VSC_READ_LEN, g = off + pos;
            bool out = false;
            if (wl == (uint32_t)VSC_READ_LEN) {  // (the table describes whole windows)
                const uint32_t b = g >> a.reg.block_shift;
                out = b >= a.reg.n_blocks || ((a.reg.cls[b >> 4] >> (2u * (b & 15u))) & 3u) == kRegOut;
            }
            if (!out) {
                const uint32_t label = regions_locate(a.reg, a.loc, g, wl);
                if (label != kLocateNone) t = a.group ? (label < a.n_group ? a.group[label] : kPickNone) : label;
            }
        }
    }
    *target = t;
    return pick_class(a.shape, a.n_contigs, contig, len, pos, strand, t, a.n_targets, a.key[i]);
}

}  // namespace

// tgt[i] = the target of candidate i if it is eligible, else kPickNone; count[t] += eligible candidates of t; stats[class] +=.
// Grid-stride over the 64-bit count in steps of whole waves, as mh_score_kernel.  The candidates mostly come in position
// order, so neighbouring lanes mostly share a target: the first lane of every run of equal targets adds the run's length.
__global__ __launch_bounds__(kPickThreads) void pick_mark_kernel(const PickArgs a)
{
    __shared__ unsigned long long s_count[kPickClasses];
    if (threadIdx.x < kPickClasses) s_count[threadIdx.x] = 0;
    block_sync();
    const uint32_t lane = threadIdx.x % kWave;
    const unsigned long long stride = (unsigned long long)gridDim.x * kPickThreads;
    uint32_t seen[kPickClasses] = {};  // wave-uniform
    const unsigned long long first = (unsigned long long)blockIdx.x * kPickThreads + threadIdx.x;
    for (unsigned long long base = first - lane; base < a.n; base += stride) {
        const unsigned long long i = base + lane;
        uint32_t cls = kPickClasses, t = kPickNone;
        if (i < a.n) {
            cls = pick_candidate(a, i, a.loci[i], &t);
            if (cls != kPickEligible) t = kPickNone;
            a.tgt[i] = t;
        }
#pragma unroll
        for (uint32_t k = 0; k < kPickClasses; ++k) seen[k] += (uint32_t)__popcll(__ballot(cls == k));
        uint32_t head, len;
        wave_run(t, lane, &head, &len);
        if (head == lane && t < a.n_targets) atomicAdd(&a.count[t], len);
    }
    if (lane == 0) {
#pragma unroll
        for (uint32_t k = 0; k < kPickClasses; ++k)
            if (seen[k]) atomicAdd(&s_count[k], (unsigned long long)seen[k]);
    }
    block_sync();
    if (threadIdx.x < kPickClasses && s_count[threadIdx.x]) atomicAdd(&a.stats[threadIdx.x], s_count[threadIdx.x]);
}

// One record per eligible candidate into its target's segment: the run's first lane reserves the run's slots on the target's
// cursor, the lanes of the run fill them.  Which slots a run gets depends on the order in which waves arrive; the select's
// result does not (see the head of the file).
__global__ __launch_bounds__(kPickThreads) void pick_scatter_kernel(const PickArgs a)
{
    const uint32_t lane = threadIdx.x % kWave;
    const unsigned long long stride = (unsigned long long)gridDim.x * kPickThreads;
    const unsigned long long first = (unsigned long long)blockIdx.x * kPickThreads + threadIdx.x;
    for (unsigned long long base = first - lane; base < a.n; base += stride) {
        const unsigned long long i = base + lane;
        const uint32_t t = i < a.n ? a.tgt[i] : kPickNone;
        uint32_t head, len;
        wave_run(t, lane, &head, &len);
        const bool in = t < a.n_targets;
        uint32_t at = 0;
        if (head == lane && in) at = atomicAdd(&a.cursor[t], len);
        at = __shfl(at, (int)head);
        if (in) {
            const unsigned long long slot = a.seg_off[t] + at + (lane - head);
            if (slot < a.seg_off[t + 1] && slot < a.n_rec) {  // (always, when count[] is what pick_mark_kernel left)
                const uint4 r = a.loci[i];
                const unsigned long long key = a.key[i];
                a.rec[slot] = make_uint4((uint32_t)key, (uint32_t)(key >> 32), (uint32_t)pick_cut_coordinate(a.shape, r.y, r.z), r.x);
                a.rec_index[slot] = (uint32_t)i;
            }
        }
    }
}

namespace {

// wave-wide first of (key, index) under BEFORE; index kPickNone = the lane has none.  The same pair on every lane afterwards.
__device__ __forceinline__ void wave_first(uint64_t *key, uint32_t *index)
{
#pragma unroll
    for (int d = kWave / 2; d; d >>= 1) {
        const uint32_t olo = __shfl_xor((uint32_t)*key, d), ohi = __shfl_xor((uint32_t)(*key >> 32), d), oi = __shfl_xor(*index, d);
        const uint64_t ok = (uint64_t)ohi << 32 | olo;
        if (oi != kPickNone && (*index == kPickNone || pick_before(ok, oi, *key, *index))) {
            *key = ok;
            *index = oi;
        }
    }
}

}  // namespace

// The PICK loop, one wave per target (a wave walks targets wave, wave + waves of the launch, ...).  Per round: every lane's
// first open record under BEFORE, the wave's first of those by a butterfly over (key, index), the winner's (contig, x) from
// the lane that owns it, then every lane closes its records that conflict with it (and the winner itself).  A segment of at
// most kPickWaveCap records lives in registers with one open bit per record; a larger one is read from memory in every round,
// each record tested against the picks so far, which lie in the wave's slice of LDS.  The loop ends at k picks or when no
// lane has an open record.
__global__ __launch_bounds__(kPickThreads) void pick_select_kernel(const PickArgs a)
{
    __shared__ uint4 s_pick[kWavesPerGroup][kPickMaxK];  // large segments: (index, contig, x, 0) of the picks so far
    const uint32_t lane = threadIdx.x % kWave, w = threadIdx.x / kWave;
    const unsigned long long n_waves = (unsigned long long)gridDim.x * kWavesPerGroup;
    const uint32_t k = a.shape.k, spacing = a.shape.spacing;
    uint32_t with = 0, ended_short = 0, n_picks = 0;  // wave-uniform
    for (unsigned long long tt = (unsigned long long)blockIdx.x * kWavesPerGroup + w; tt < a.n_targets; tt += n_waves) {
        const uint32_t t = (uint32_t)tt;
        const unsigned long long s0 = a.seg_off[t], s1 = a.seg_off[t + 1];
        const unsigned long long m = s1 >= s0 && s1 <= a.n_rec ? s1 - s0 : 0;
        uint32_t *const out = a.picks + (size_t)t * k;
        uint32_t got = 0;
        if (m <= kPickWaveCap) {
            uint64_t key[kPickPerLane];
            uint32_t x[kPickPerLane], c[kPickPerLane], idx[kPickPerLane];
            uint32_t open = 0;
#pragma unroll
            for (int j = 0; j < kPickPerLane; ++j) {
                const uint32_t e = (uint32_t)j * kWave + lane;
                key[j] = 0;
                x[j] = c[j] = 0;
                idx[j] = kPickNone;
                if (e < m) {
                    const uint4 v = a.rec[s0 + e];
                    key[j] = (uint64_t)v.y << 32 | v.x;
                    x[j] = v.z;
                    c[j] = v.w;
                    idx[j] = a.rec_index[s0 + e];
                    open |= 1u << j;
                }
            }
            while (got < k) {
                uint64_t bk = 0;
                uint32_t bi = kPickNone, bx = 0, bc = 0;
#pragma unroll
                for (int j = 0; j < kPickPerLane; ++j)
                    if (((open >> j) & 1u) && (bi == kPickNone || pick_before(key[j], idx[j], bk, bi))) {
                        bk = key[j];
                        bi = idx[j];
                        bx = x[j];
                        bc = c[j];
                    }
                uint64_t wk = bk;
                uint32_t wi = bi;
                wave_first(&wk, &wi);
                if (wi == kPickNone) break;  // (the same on every lane)
                const uint64_t owners = __ballot(bi == wi);
                const int owner = owners ? __ffsll((unsigned long long)owners) - 1 : 0;
                const uint32_t wx = __shfl(bx, owner), wc = __shfl(bc, owner);
                if (lane == 0) out[got] = wi;
                ++got;
#pragma unroll
                for (int j = 0; j < kPickPerLane; ++j)
                    if (idx[j] == wi || pick_conflict(spacing, c[j], x[j], wc, wx)) open &= ~(1u << j);
            }
        } else {
            while (got < k) {
                uint64_t bk = 0;
                uint32_t bi = kPickNone, bx = 0, bc = 0;
                for (unsigned long long e = lane; e < m; e += kWave) {
                    const uint4 v = a.rec[s0 + e];
                    const uint64_t ke = (uint64_t)v.y << 32 | v.x;
                    const uint32_t ie = a.rec_index[s0 + e];
                    if (bi != kPickNone && !pick_before(ke, ie, bk, bi)) continue;  // not in front of the lane's first so far
                    bool is_open = true;
                    for (uint32_t r = 0; r < got && is_open; ++r) {
                        const uint4 p = s_pick[w][r];
                        is_open = p.x != ie && !pick_conflict(spacing, v.w, v.z, p.y, p.z);
                    }
                    if (is_open) {
                        bk = ke;
                        bi = ie;
                        bx = v.z;
                        bc = v.w;
                    }
                }
                uint64_t wk = bk;
                uint32_t wi = bi;
                wave_first(&wk, &wi);
                if (wi == kPickNone) break;
                const uint64_t owners = __ballot(bi == wi);
                const int owner = owners ? __ffsll((unsigned long long)owners) - 1 : 0;
                const uint32_t wx = __shfl(bx, owner), wc = __shfl(bc, owner);
                if (lane == 0) {
                    out[got] = wi;
                    s_pick[w][got] = make_uint4(wi, wc, wx, 0u);
                }
                wave_sync();  // (the next round's reads of s_pick come after this store)
                ++got;
            }
        }
        if (lane >= got && lane < k) out[lane] = kPickNone;  // k <= 32 < 64 lanes
        if (lane == 0) a.counts[t] = got;
        with += got ? 1u : 0u;
        ended_short += got < k && m > got ? 1u : 0u;
        n_picks += got;
    }
    if (lane == 0) {
        if (with) atomicAdd(&a.stats[kPickStatTargets], (unsigned long long)with);
        if (ended_short) atomicAdd(&a.stats[kPickStatShort], (unsigned long long)ended_short);
        if (n_picks) atomicAdd(&a.stats[kPickStatPicks], (unsigned long long)n_picks);
    }
}

// rank[picks[t * k + r]] = r (rank[] is all ones before): every candidate is picked at most once, so no two lanes store to
// one word
__global__ __launch_bounds__(kPickThreads) void pick_rank_kernel(const PickArgs a)
{
    const unsigned long long total = (unsigned long long)a.n_targets * a.shape.k;
    const unsigned long long stride = (unsigned long long)gridDim.x * kPickThreads;
    for (unsigned long long j = (unsigned long long)blockIdx.x * kPickThreads + threadIdx.x; j < total; j += stride) {
        const uint32_t p = a.picks[j];
        if (p != kPickNone && p < a.n) a.rank[p] = (uint32_t)(j % a.shape.k);
    }
}

// kWrite = false: tile_count[i] = the picked candidates of tile work[i].  kWrite = true: their codes and loci to tile_off[i] +
// the rank in the tile - the input's order, no atomic (mh_filter_kernel's passes over a keep flag).
template <bool kWrite> __global__ __launch_bounds__(kPickThreads) void pick_gather_kernel(const PickGatherArgs a)
{
    const uint32_t lane = threadIdx.x % kWave;
    const uint32_t item = blockIdx.x * kWavesPerGroup + threadIdx.x / kWave;  // wave-uniform
    if (item >= a.n_work) return;
    const uint32_t tile = a.work ? a.work[item] : item;
    const unsigned long long first = (unsigned long long)tile * kPickTile;
    unsigned long long at = kWrite ? a.tile_off[item] : 0;
    uint32_t count = 0;
    for (uint32_t step = 0; step < kPickTile / kWave; ++step) {
        const unsigned long long base = first + (unsigned long long)step * kWave;
        if (base >= a.n) break;
        const unsigned long long i = base + lane;
        const bool keep = i < a.n && a.rank[i] != kPickNone;
        const uint64_t kept = __ballot(keep);
        if (kWrite) {
            if (keep) {
                const unsigned long long o = at + lanes_below(kept);
                a.codes[o] = a.in_codes[i];
                a.loci[o] = a.in_loci[i];
            }
            at += (uint32_t)__popcll(kept);
        } else {
            count += (uint32_t)__popcll(kept);
        }
    }
    if (!kWrite && lane == 0) a.tile_count[item] = count;
}

namespace {

// 8 workgroups of 4 waves per CU fill every SIMD's 8 wave slots; fewer when the items do not need them (launch_locate)
dim3 pick_grid(unsigned long long items, int n_cus)
{
    const unsigned long long want = (items + kPickThreads - 1) / kPickThreads;
    const unsigned long long cap = (unsigned long long)(n_cus > 0 ? n_cus : 256) * 8u;
    return dim3((uint32_t)(want < cap ? want : cap));
}

}  // namespace

hipError_t launch_pick_mark(const PickArgs &args, int n_cus, hipStream_t stream)
{
    if (args.n == 0) return hipSuccess;
    hipLaunchKernelGGL(pick_mark_kernel, pick_grid(args.n, n_cus), dim3(kPickThreads), 0, stream, args);
    return hipGetLastError();
}

hipError_t launch_pick_scatter(const PickArgs &args, int n_cus, hipStream_t stream)
{
    if (args.n == 0 || args.n_rec == 0) return hipSuccess;
    hipLaunchKernelGGL(pick_scatter_kernel, pick_grid(args.n, n_cus), dim3(kPickThreads), 0, stream, args);
    return hipGetLastError();
}

hipError_t launch_pick_select(const PickArgs &args, int n_cus, hipStream_t stream)
{
    if (args.n_targets == 0) return hipSuccess;
    // one wave per target, at most the waves the device holds: more targets than that and each wave walks several
    hipLaunchKernelGGL(pick_select_kernel, pick_grid((unsigned long long)args.n_targets * kWave, n_cus), dim3(kPickThreads), 0, stream, args);
    return hipGetLastError();
}

hipError_t launch_pick_rank(const PickArgs &args, int n_cus, hipStream_t stream)
{
    const unsigned long long total = (unsigned long long)args.n_targets * args.shape.k;
    if (total == 0 || args.n == 0) return hipSuccess;
    hipLaunchKernelGGL(pick_rank_kernel, pick_grid(total, n_cus), dim3(kPickThreads), 0, stream, args);
    return hipGetLastError();
}

hipError_t launch_pick_gather(const PickGatherArgs &args, bool write, hipStream_t stream)
{
    if (args.n_work == 0) return hipSuccess;
    const dim3 grid((args.n_work + kWavesPerGroup - 1) / kWavesPerGroup), block(kPickThreads);
    if (write) hipLaunchKernelGGL((pick_gather_kernel<true>), grid, block, 0, stream, args);
    else hipLaunchKernelGGL((pick_gather_kernel<false>), grid, block, 0, stream, args);
    return hipGetLastError();
}

}  // namespace vsc
