// vsc_variants.hip - the window side of the mergers on the device (vsc_hits_variants, vsc_search_summary_variants):
//   variant_merge_kernel  per sorted vsc_hit record of the window genome: chromosome coordinates and REF / VAR tag
//                         (filterSnpAlignment + getSnpType, variant_processing/filter_output_bam.h:189-317), the duplicate and
//                         on-target rules (:297-306), and the per-guide rows over what is left
#include "vsc_varmap.h"
#include "vsc_device.h"
#include "vsc_mit.h"

namespace vsc {

// One record per thread.  A record's fate depends on the record before it, so every thread leaves its record and its label in
// LDS and reads its left neighbour's from there; only the first thread of a workgroup loads the record before the workgroup's
// first one again and walks that window's variants itself.  Per record: the window's table entry (16 bytes), the walk over the
// window's variants (varmap_walk: bounded by the variants of that window), then the key comparison - guide and info word,
// pos2, chromosome and the count of covered variants first; only if all of them agree the covered tag ids in lockstep and the
// 23 bases of the two windows from the resident planes.
// Rows: the records are sorted by guide, so a wave holds runs of guides.  Every lane's contribution - 0 or 1 record - is added
// up per run with a segmented reduction over lane shuffles (six steps; the nine NM counters share one 64-bit word, 7 bits
// each: a run in a wave has at most 64 records), and the first lane of every run issues one device atomic per nonzero field of
// the run - never one per record.
// Every index is checked before it is used: a record whose window, position or guide lies outside the tables raises a.error
// and is not looked at further.
constexpr int kVarThreads = 256;
constexpr int kVarCountBits = 7;

// record r lies in the map and in its window (and, where guides index anything, among the guides)
__device__ __forceinline__ bool var_record_ok(const VariantArgs &a, const uint4 &r)
{
    if (r.y >= a.map.n_windows) return false;
    if ((a.exclude || a.rows_all) && r.x >= a.n_guides) return false;
    const uint32_t off = a.contig_off[r.y], len = a.contig_end[r.y] - off;
    if (len < (uint32_t)VSC_READ_LEN || r.z > len - (uint32_t)VSC_READ_LEN) return false;
    const uint32_t g = off + r.z;
    return g >= a.first_pos && (unsigned long long)((g - a.first_pos) >> 5) < a.n_plane_words;
}

// the 23 bases of record r's window position (var_record_ok holds): forward genome, one bit plane pair
__device__ __forceinline__ void var_site_planes(const VariantArgs &a, const uint4 &r, uint32_t &h, uint32_t &l)
{
    const uint32_t rel = a.contig_off[r.y] + r.z - a.first_pos;
    const unsigned long long wi = rel >> 5;
    const uint32_t sh = rel & 31u;
    const bool next = wi + 1 < a.n_plane_words;  // (past the planes: N, and no hit reaches there)
    const uint32_t h0 = a.hi[wi], l0 = a.lo[wi], h1 = next ? a.hi[wi + 1] : 0u, l1 = next ? a.lo[wi + 1] : 0u;
    h = funnel(h1, h0, sh) & kMask23;
    l = funnel(l1, l0, sh) & kMask23;
}

__global__ __launch_bounds__(kVarThreads) void variant_merge_kernel(const VariantArgs a)
{
    __shared__ uint4 s_rec[kVarThreads];
    __shared__ uint2 s_lab[kVarThreads];  // pos2, covered variants (all ones: the record is outside the tables)
    const uint32_t t = threadIdx.x, lane = t % kWave;
    const unsigned long long i = (unsigned long long)blockIdx.x * kVarThreads + t;
    const bool have = i < a.n;
    uint4 r = make_uint4(~0u, 0u, 0u, 0u);
    uint32_t pos2 = 0, n_var = ~0u;
    if (have) {
        r = a.records[i];
        if (var_record_ok(a, r)) varmap_walk(a.map, r.y, r.z, VSC_READ_LEN, &pos2, &n_var);
        else *a.error = 1u;
    }
    const bool ok = n_var != ~0u;
    s_rec[t] = r;
    s_lab[t] = make_uint2(pos2, n_var);
    block_sync();

    bool dup = false, on = false;
    VarWindow win{};
    if (ok) {
        win = a.map.win[r.y];
        if (i > 0) {
            uint4 q;
            uint2 ql;
            if (t > 0) {
                q = s_rec[t - 1];
                ql = s_lab[t - 1];
            } else {  // the record before this workgroup's first
                q = a.records[i - 1];
                ql = make_uint2(0u, ~0u);
                if (var_record_ok(a, q)) varmap_walk(a.map, q.y, q.z, VSC_READ_LEN, &ql.x, &ql.y);
            }
            // key = (guide, chr, pos2, strand, bases, mask, tag): the info word holds strand and mask
            if (ql.y != ~0u && q.x == r.x && q.w == r.w && ql.x == pos2 && ql.y == n_var && a.map.win[q.y].chr_id == win.chr_id) {
                bool same = n_var == 0 || var_tags_equal(a.map, r.y, r.z, q.y, q.z, n_var, VSC_READ_LEN);
                if (same) {
                    uint32_t rh, rl, qh, ql2;
                    var_site_planes(a, r, rh, rl);
                    var_site_planes(a, q, qh, ql2);
                    same = rh == qh && rl == ql2;
                }
                dup = same;
            }
        }
        if (a.exclude) {  // the guide's own locus: that chromosome position and strand, no mismatch, no variant
            const uint4 ex = a.exclude[r.x];
            on = ex.x != UINT32_MAX && win.contig == ex.x && pos2 == ex.y && VSC_HIT_STRAND(r.w) == ex.z && VSC_HIT_MASK(r.w) == 0u &&
                 n_var == 0;
        }
    }
    if (a.labels && have) {
        uint4 lab = make_uint4(0u, 0u, 0u, 0u);
        if (ok) lab = make_uint4(win.contig, pos2, n_var, (n_var ? VSC_VARIANT_VAR : 0u) | (dup ? VSC_VARIANT_DUP : 0u) | (on ? VSC_VARIANT_ON_TARGET : 0u));
        a.labels[i] = lab;
    }
    if (!a.rows_all) return;  // (uniform: a kernel argument)

    // this lane's contribution to its guide's rows
    uint32_t g = ok ? r.x : ~0u;
    unsigned long long mit_all = 0, cnt_all = 0, mit_var = 0, cnt_var = 0;
    uint32_t small = 0;  // reference-UB flags of the counted records (all, var), on-targets met, duplicates: 8 bits each
    if (ok) {
        small = (on ? 1u << 16 : 0u) | (dup ? 1u << 24 : 0u);
        if (!dup && !on) {
            const uint32_t mask = VSC_HIT_MASK(r.w);
            int f;
            const double s = mit_score(mask, &f);
            mit_all = (uint32_t)__builtin_rint(s * 0x1p24);  // as summary_kernel: <= 100 * 2^24 < 2^32, exact power-of-two scale
            cnt_all = 1ull << (kVarCountBits * __popc(mask));
            small |= (uint32_t)f;
            if (n_var) {
                mit_var = mit_all;
                cnt_var = cnt_all;
                small |= (uint32_t)f << 8;
            }
        }
    }
    // segmented reduction towards the first lane of every run of one guide: after the step with distance d a lane holds the
    // sum over the lanes [lane, lane + 2 d) of its run (the run is contiguous: the guide d lanes on is mine iff all between are)
    for (int d = 1; d < kWave; d <<= 1) {
        const uint32_t og = __shfl_down(g, d, kWave);
        const unsigned long long oma = __shfl_down(mit_all, d, kWave), oca = __shfl_down(cnt_all, d, kWave);
        const unsigned long long omv = __shfl_down(mit_var, d, kWave), ocv = __shfl_down(cnt_var, d, kWave);
        const uint32_t os = __shfl_down(small, d, kWave);
        if (lane + (uint32_t)d < (uint32_t)kWave && og == g) {
            mit_all += oma;
            cnt_all += oca;
            mit_var += omv;
            cnt_var += ocv;
            small += os;
        }
    }
    const uint32_t left = __shfl_up(g, 1, kWave);
    if (g == ~0u || (lane > 0 && left == g)) return;
    auto flush = [&](unsigned long long *row, unsigned long long m, unsigned long long c9, uint32_t ub) {
        if (m) atomicAdd(&row[0], m);
#pragma unroll
        for (int k = 0; k <= VSC_MAX_MISMATCHES; ++k) {
            const uint32_t c = (uint32_t)(c9 >> (kVarCountBits * k)) & ((1u << kVarCountBits) - 1u);
            if (c) atomicAdd(&row[1 + k], (unsigned long long)c);
        }
        if (ub) atomicAdd(&row[10], (unsigned long long)ub);
        if ((small >> 16) & 0xFFu) atomicOr(&row[11], 1ull);  // on_target (the low word of the row's last 8 bytes)
    };
    flush(a.rows_all + (size_t)g * kSumWords, mit_all, cnt_all, small & 0xFFu);
    if (a.rows_var) flush(a.rows_var + (size_t)g * kSumWords, mit_var, cnt_var, (small >> 8) & 0xFFu);
    if (a.dups && (small >> 24)) atomicAdd(&a.dups[g], (unsigned long long)(small >> 24));
}

hipError_t launch_variant_merge(const VariantArgs &args, hipStream_t stream)
{
    if (args.n == 0) return hipSuccess;
    const unsigned long long blocks = (args.n + kVarThreads - 1) / kVarThreads;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(variant_merge_kernel, dim3((uint32_t)blocks), dim3(kVarThreads), 0, stream, args);
    return hipGetLastError();
}

}  // namespace vsc
