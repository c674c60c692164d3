// vsc_enum.hip - guide discovery (vsc_guides_enumerate): every 23-base window of the resident planes that ends in
// the GUIDE's PAM (one PAM, NGG by default - not the off-target PAM set), holds no N, passes the GC / T-run filters and lies in
// the regions, as (vsc_pack_guide code, vsc_locus) in ascending (position, '+' before '-') order.
//
// The front end is scan_kernel's (vsc_kernels.hip): one wave per tile of 2 048 window starts, one 32-start word of each plane
// per lane plus its right neighbour, the same N mask and funnel shifts, one PamMasks entry.  What differs is the back end: the
// result is a RESULT, not an index that is sorted afterwards, so nothing is appended through an atomic cursor.  Two passes over
// the same masks - enum_kernel<false> counts per tile, enum_scan_kernel turns the counts into offsets, enum_kernel<true>
// recomputes the masks and writes every candidate at  tile offset + wave prefix over the lanes + rank inside the lane.  The
// bytes depend on the planes and the parameters only: no atomic, no work cursor, tile i of the work list is wave i.
//
// At the end of the file: locate_kernel (vsc_hits_locate / vsc_guides_locate), the other reader of the regions'
// class table outside the sinks - per record the interval of the regions its window lies in.
#include "vsc_internal.h"
#include "vsc_device.h"
#include "vsc_enum.h"

namespace vsc {

namespace {

constexpr uint32_t kMask20 = 0xFFFFFu;  // the protospacer: guide positions 0..19

// bit i of p -> bit 2 i (23 bits in, 45 out)
__device__ __forceinline__ uint64_t spread23(uint32_t p)
{
    uint64_t x = p;
    x = (x | (x << 16)) & 0x0000FFFF0000FFFFull;
    x = (x | (x << 8)) & 0x00FF00FF00FF00FFull;
    x = (x | (x << 4)) & 0x0F0F0F0F0F0F0F0Full;
    x = (x | (x << 2)) & 0x3333333333333333ull;
    x = (x | (x << 1)) & 0x5555555555555555ull;
    return x;
}

// The sequence filters on one window; wh / wl = its 23 bases on the forward genome.  The protospacer g[0..20) is w[0..20) on
// '+' and the reverse complement of w[3..23) on '-': G/C stay G/C under the complement, a T of the guide is an A of the
// window, and a run is as long read backwards - so neither plane has to be reversed.
__device__ __forceinline__ bool sequence_ok(const EnumArgs &a, uint32_t wh, uint32_t wl, bool rev)
{
    const uint32_t sh = rev ? 3u : 0u;
    const uint32_t h = (wh >> sh) & kMask20, l = (wl >> sh) & kMask20;
    const uint32_t gc = (uint32_t)__popc(h ^ l);
    if (gc < a.gc_min || gc > a.gc_max) return false;
    if (a.max_t_run) {
        uint32_t y = rev ? ~(h | l) & kMask20 : h & l;  // T of the guide
        for (uint32_t i = 0; i < a.max_t_run && y; ++i) y &= y >> 1;  // every step shortens every run by one
        if (y) return false;                            // a run of more than max_t_run is left
    }
    return true;
}

// exclusive prefix of v over the lanes of the wave; *total = the wave's sum
__device__ __forceinline__ uint32_t wave_exclusive(uint32_t v, uint32_t lane, uint32_t *total)
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

// kWrite = false: tile_count[i] = candidates kept in tile work[i].  kWrite = true: the same masks again, every candidate to
// its rank behind tile_off[i].  kRegions: the window must be in a.reg.
template <bool kWrite, bool kRegions>
__global__ __launch_bounds__(kWave *kWavesPerGroup) void enum_kernel(const EnumArgs a)
{
    const uint32_t lane = threadIdx.x % kWave;
    const uint32_t item = blockIdx.x * kWavesPerGroup + threadIdx.x / kWave;  // wave-uniform
    if (item >= a.n_work) return;
    const uint32_t tile = a.work ? a.work[item] : item;

    // ---- scan_kernel's front end: 32 window starts per lane ----
    const size_t wi = (size_t)tile * kTileWords + lane;
    const uint32_t H0 = a.hi[wi], H1 = a.hi[wi + 1];
    const uint32_t L0 = a.lo[wi], L1 = a.lo[wi + 1];
    const uint32_t N0 = a.nm[wi], N1 = a.nm[wi + 1];
    uint64_t nn = ((uint64_t)N1 << 32) | N0;
    nn |= nn >> 1;
    nn |= nn >> 2;
    nn |= nn >> 4;
    nn |= nn >> 8;   // bit i covers positions i .. i+15
    nn |= nn >> 7;   // bit i covers positions i .. i+22
    const uint32_t clean = ~(uint32_t)nn;
    const uint32_t H21 = funnel(H1, H0, 21), L21 = funnel(L1, L0, 21);
    const uint32_t H22 = funnel(H1, H0, 22), L22 = funnel(L1, L0, 22);
    const uint32_t Hs1 = funnel(H1, H0, 1), Ls1 = funnel(L1, L0, 1);
    const PamMasks p = a.pam;
    // '+': window[21] == a and window[22] == b;  '-': window[0] == comp(b) and window[1] == comp(a)
    uint32_t mf = ~(H21 ^ p.ah) & ~(L21 ^ p.al) & ~(H22 ^ p.bh) & ~(L22 ^ p.bl) & clean & a.keep_fwd;
    uint32_t mr = (H0 ^ p.bh) & (L0 ^ p.bl) & (Hs1 ^ p.ah) & (Ls1 ^ p.al) & clean & a.keep_rev;
    const uint32_t base_pos = a.first_pos + tile * (uint32_t)kTileBases + lane * 32u;

    // ---- region class of the lane's 32 starts: one block of the table (block_shift >= 5, base_pos is a multiple of 32) ----
    bool search = false;
    if (kRegions) {
        const uint32_t b = base_pos >> a.reg.block_shift;
        const uint32_t c = b < a.reg.n_blocks ? (a.reg.cls[b >> 4] >> (2u * (b & 15u))) & 3u : kRegOut;
        if (c == kRegOut) mf = mr = 0;
        search = c == kRegMixed;
    }
    // ---- per-window tests, only where one is asked for: set bit by set bit ----
    if (a.filter || search) {
        for (uint32_t m = mf | mr; m; m &= m - 1u) {
            const uint32_t b = (uint32_t)__builtin_ctz(m), bit = 1u << b;
            if (search && !regions_search(a.reg, base_pos + b, VSC_READ_LEN)) {
                mf &= ~bit;
                mr &= ~bit;
                continue;
            }
            if (a.filter) {
                const uint32_t wh = funnel(H1, H0, b), wl = funnel(L1, L0, b);
                if ((mf & bit) && !sequence_ok(a, wh, wl, false)) mf &= ~bit;
                if ((mr & bit) && !sequence_ok(a, wh, wl, true)) mr &= ~bit;
            }
        }
    }

    // ---- rank: tile offset + wave prefix over the lanes + order inside the lane ----
    uint32_t total;
    const uint32_t before = wave_exclusive((uint32_t)__popc(mf) + (uint32_t)__popc(mr), lane, &total);
    if (!kWrite) {
        if (lane == 0) a.tile_count[item] = total;
        return;
    }
    if (total == 0) return;
    unsigned long long at = a.tile_off[item] + before;
    uint32_t c = 0, c_end = 0;  // the contig of the lane's last candidate: [.., c_end) in global positions
    for (uint32_t m = mf | mr; m; m &= m - 1u) {
        const uint32_t b = (uint32_t)__builtin_ctz(m), bit = 1u << b;
        const uint32_t pos = base_pos + b;
        if (pos >= c_end) {  // c = the last contig that starts at or before pos (an N-free window lies inside one contig)
            uint32_t lo = 0, hi = a.n_contigs;
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (a.contig_off[mid] <= pos) lo = mid + 1; else hi = mid;
            }
            c = lo ? lo - 1u : 0u;
            c_end = a.contig_end[c];
        }
        const uint32_t wh = funnel(H1, H0, b) & kMask23, wl = funnel(L1, L0, b) & kMask23;
        const uint32_t rel = pos - a.contig_off[c];
        if (mf & bit) {
            a.codes[at] = spread23(wh) << 1 | spread23(wl);
            a.loci[at] = make_uint4(c, rel, 0u, 0u);
            ++at;
        }
        if (mr & bit) {
            a.codes[at] = spread23(revcomp_plane(wh)) << 1 | spread23(revcomp_plane(wl));
            a.loci[at] = make_uint4(c, rel, 1u, 0u);
            ++at;
        }
    }
}

// tile_off[i] = sum of tile_count[0 .. i), i = 0 .. n (tile_off[n] = all candidates); one workgroup, as merge_scan_kernel
__global__ __launch_bounds__(1024) void enum_scan_kernel(const uint32_t *tile_count, uint32_t n, unsigned long long *tile_off)
{
    __shared__ unsigned long long partial[1024];
    const uint32_t t = threadIdx.x;
    const uint32_t per = (n + 1023) / 1024;
    const uint32_t i0 = min(t * per, n), i1 = min(i0 + per, n);
    unsigned long long sum = 0;
    for (uint32_t i = i0; i < i1; ++i) sum += tile_count[i];
    partial[t] = sum;
    block_sync();
    for (uint32_t d = 1; d < 1024; d <<= 1) {
        const unsigned long long v = t >= d ? partial[t - d] : 0;
        block_sync();
        partial[t] += v;
        block_sync();
    }
    unsigned long long run = partial[t] - sum;
    for (uint32_t i = i0; i < i1; ++i) {
        tile_off[i] = run;
        run += tile_count[i];
    }
    if (t == 1023) tile_off[n] = partial[1023];
}

hipError_t launch_enum(const EnumArgs &args, bool write, bool regions, hipStream_t stream)
{
    if (args.n_work == 0) return hipSuccess;
    const dim3 grid((args.n_work + kWavesPerGroup - 1) / kWavesPerGroup), block(kWave * kWavesPerGroup);
    if (write) {
        if (regions) hipLaunchKernelGGL((enum_kernel<true, true>), grid, block, 0, stream, args);
        else hipLaunchKernelGGL((enum_kernel<true, false>), grid, block, 0, stream, args);
    } else {
        if (regions) hipLaunchKernelGGL((enum_kernel<false, true>), grid, block, 0, stream, args);
        else hipLaunchKernelGGL((enum_kernel<false, false>), grid, block, 0, stream, args);
    }
    return hipGetLastError();
}

hipError_t launch_enum_scan(const uint32_t *tile_count, uint32_t n, unsigned long long *tile_off, hipStream_t stream)
{
    hipLaunchKernelGGL(enum_scan_kernel, dim3(1), dim3(1024), 0, stream, tile_count, n, tile_off);
    return hipGetLastError();
}

// ---- labels --------------------------------------------------------------------------------------------------
// labels[i] = the label of record i under the regions: one record per lane and step (one 16-byte load), grid-stride over the
// 64-bit count.  A record outside the contig table, a window that leaves its contig and a start in an OUT block are
// kLocateNone without a further read; IN and MIXED blocks take the binary search over start[] and the walk over up[]
// (regions_locate, vsc_enum.h).  A gather bound by the latency of its dependent loads: no LDS, no atomics, one coalesced
// 4-byte store per lane.  Every index is checked against its array's length before it is used.
constexpr int kLocateThreads = 256;

template <bool kHit>
__global__ __launch_bounds__(kLocateThreads) void locate_kernel(const LocateArgs a)
{
    const unsigned long long stride = (unsigned long long)gridDim.x * kLocateThreads;
    for (unsigned long long i = (unsigned long long)blockIdx.x * kLocateThreads + threadIdx.x; i < a.n; i += stride) {
        const uint4 r = a.records[i];
        const uint32_t contig = kHit ? r.y : r.x, pos = kHit ? r.z : r.y;
        uint32_t label = kLocateNone;
        if (contig < a.n_contigs) {
            const uint32_t len = a.contig_len[contig];
            if (pos <= len && len - pos >= (uint32_t)VSC_READ_LEN) {  // pos + 23 <= len, without the overflow
                const uint32_t g = a.contig_off[contig] + pos;
                const uint32_t b = g >> a.reg.block_shift;
                const uint32_t c = b < a.reg.n_blocks ? (a.reg.cls[b >> 4] >> (2u * (b & 15u))) & 3u : kRegOut;
                if (c != kRegOut) label = regions_locate(a.reg, a.loc, g, VSC_READ_LEN);
            }
        }
        a.labels[i] = label;
    }
}

hipError_t launch_locate(const LocateArgs &args, bool hit_records, int n_cus, hipStream_t stream)
{
    if (args.n == 0) return hipSuccess;
    // 8 workgroups of 4 waves per CU fill every SIMD's 8 wave slots; fewer when the records do not need them
    const unsigned long long want = (args.n + kLocateThreads - 1) / kLocateThreads;
    const unsigned long long cap = (unsigned long long)(n_cus > 0 ? n_cus : 256) * 8u;
    const dim3 grid((uint32_t)(want < cap ? want : cap)), block(kLocateThreads);
    if (hit_records) hipLaunchKernelGGL((locate_kernel<true>), grid, block, 0, stream, args);
    else hipLaunchKernelGGL((locate_kernel<false>), grid, block, 0, stream, args);
    return hipGetLastError();
}

}  // namespace vsc
