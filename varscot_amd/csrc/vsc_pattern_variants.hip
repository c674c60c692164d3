// vsc_pattern_variants.hip - both sides of the mergers for pattern hits on the device (vsc_pattern_hits_variants,
// vsc_pattern_hits_shadowed, vsc_search_pattern_variants):
//   pattern_variant_merge_kernel  per vsc_pattern_hit record of the window genome: chromosome coordinates and REF / VAR tag
//                                 (filterSnpAlignment + getSnpType with seq_len = L, variant_processing/filter_output_bam.h:
//                                 189-317), the duplicate and on-target rules (:297-306), the per-guide rows over what is left
//   pattern_shadow_kernel         per record of the reference genome: shadowed by a window (filterRefAlignment with seq_len =
//                                 L, :70-124) or the on-target, and the per-guide rows over what is left
// One body, two template modes (and each with and without the records' score words).
#include "vsc_pattern_variants.h"
#include "vsc_device.h"

namespace vsc {

// One record per thread, 256 threads.  A workgroup's 256 records of five words are 1 280 consecutive words: thread t loads
// words t, t + 256, ... into LDS (coalesced dwords) and takes its record from words 5 t .. 5 t + 4 (a stride of five words:
// no bank conflict).  Window side: a record's fate depends on the record before it, so every thread leaves its label in LDS
// and reads its left neighbour's record and label from there; only the first thread of a workgroup loads the record before the
// workgroup's first one again and walks that window's variants itself.  The key is compared cheapest first - guide, info word,
// mask, pos2, covered variants, chromosome - then the covered tag ids in lockstep, last the L bases of both sites from the
// resident planes (plane_site: two words per plane and site, a mask of L bits).
// Rows: the records are sorted by guide, so a wave holds runs of guides.  Every lane's contribution - 0 or 1 record - is added
// up per run with a segmented reduction over lane shuffles (six steps; the nine NM counters share one 64-bit word, 7 bits
// each: a run in a wave has at most 64 records; the positive-by-NM counters likewise; the f sums in a 64-bit word: 64 x 2^30
// fits), and the first lane of every run issues one device atomic per nonzero field of the run - never one per record.
// Every index is checked before it is used: a record whose contig, position, NM or guide lies outside the tables raises
// a.error and is not looked at further.
constexpr int kPvThreads = 256;
constexpr int kPvRecWords = 5;
constexpr int kPvCountBits = 7;

struct PvRec {
    uint32_t guide, contig, pos, info, mask;
};

// record r lies in the searched genome's table with its L bases (and, where guides index anything, among the guides)
__device__ __forceinline__ bool pv_record_ok(const PatVarArgs &a, const PvRec &r, uint32_t *global)
{
    if (r.contig >= a.n_contigs) return false;
    if ((r.info & 63u) > (uint32_t)VSC_MAX_MISMATCHES) return false;  // (NM indexes the counters)
    if ((a.exclude || a.rows_all) && r.guide >= a.n_guides) return false;
    const uint32_t off = a.contig_off[r.contig], len = a.contig_end[r.contig] - off;
    if (len < a.len || r.pos > len - a.len) return false;
    *global = off + r.pos;
    return true;
}

// ... and, window side, in the map and in the resident planes
__device__ __forceinline__ bool pv_window_ok(const PatVarArgs &a, const PvRec &r)
{
    uint32_t g;
    if (r.contig >= a.map.n_windows || !pv_record_ok(a, r, &g)) return false;
    return g >= a.first_pos && (unsigned long long)((g - a.first_pos) >> 5) < a.n_plane_words;
}

__device__ __forceinline__ bool pv_same_bases(const PatVarArgs &a, const PvRec &r, const PvRec &q)
{
    const unsigned long long rr = a.contig_off[r.contig] + r.pos - a.first_pos, rq = a.contig_off[q.contig] + q.pos - a.first_pos;
    return plane_site(a.hi, a.n_plane_words, rr, a.len) == plane_site(a.hi, a.n_plane_words, rq, a.len) &&
           plane_site(a.lo, a.n_plane_words, rr, a.len) == plane_site(a.lo, a.n_plane_words, rq, a.len);
}

template <bool kRef, bool kScored> __global__ __launch_bounds__(kPvThreads) void pattern_variant_kernel(const PatVarArgs a)
{
    __shared__ uint32_t s_w[kPvThreads * kPvRecWords];
    __shared__ uint2 s_lab[kRef ? 1 : kPvThreads];  // pos2, covered variants (all ones: the record is outside the tables)
    const uint32_t t = threadIdx.x, lane = t % kWave;
    const unsigned long long i = (unsigned long long)blockIdx.x * kPvThreads + t;
    const unsigned long long w_first = (unsigned long long)blockIdx.x * (kPvThreads * kPvRecWords), w_total = a.n * kPvRecWords;
#pragma unroll
    for (int k = 0; k < kPvRecWords; ++k) {
        const unsigned long long w = w_first + t + (uint32_t)(k * kPvThreads);
        s_w[t + k * kPvThreads] = w < w_total ? a.records[w] : ~0u;
    }
    block_sync();
    const bool have = i < a.n;
    const uint32_t *m = s_w + t * kPvRecWords;
    const PvRec r{m[0], m[1], m[2], m[3], m[4]};
    const uint32_t nm = r.info & 63u, strand = r.info >> 31;

    bool ok = false, dropped = false, on = false;  // dropped: a duplicate (window side), shadowed (reference side)
    uint32_t n_var = 0;
    if (kRef) {
        uint32_t g = 0;
        if (have) {
            ok = pv_record_ok(a, r, &g);
            if (!ok) *a.error = 1u;
        }
        if (ok) {
            dropped = shadow_search(a.sh_start, a.sh_end_max, a.sh_n, g, a.len);
            if (a.exclude) {  // the guide's own locus: that contig, position and strand, no mismatch
                const uint4 ex = a.exclude[r.guide];
                on = ex.x != UINT32_MAX && r.contig == ex.x && r.pos == ex.y && strand == ex.z && nm == 0u;
            }
        }
        if (a.flags && have) a.flags[i] = (uint8_t)(ok ? (dropped ? VSC_PATTERN_REF_SHADOWED : 0u) | (on ? VSC_PATTERN_REF_ON_TARGET : 0u) : 0u);
    } else {
        uint32_t pos2 = 0;
        n_var = ~0u;
        if (have) {
            if (pv_window_ok(a, r)) varmap_walk(a.map, r.contig, r.pos, a.len, &pos2, &n_var);
            else *a.error = 1u;
        }
        ok = n_var != ~0u;
        s_lab[t] = make_uint2(pos2, n_var);
        block_sync();
        VarWindow win{};
        if (ok) {
            win = a.map.win[r.contig];
            if (i > 0) {
                PvRec q;
                uint2 ql;
                if (t > 0) {
                    const uint32_t *qm = m - kPvRecWords;
                    q = PvRec{qm[0], qm[1], qm[2], qm[3], qm[4]};
                    ql = s_lab[t - 1];
                } else {  // the record before this workgroup's first
                    const uint32_t *qm = a.records + (i - 1) * kPvRecWords;
                    q = PvRec{qm[0], qm[1], qm[2], qm[3], qm[4]};
                    ql = make_uint2(0u, ~0u);
                    if (pv_window_ok(a, q)) varmap_walk(a.map, q.contig, q.pos, a.len, &ql.x, &ql.y);
                }
                // key = (guide, chr, pos2, strand, bases, mask, tag): the info word holds the strand
                if (ql.y != ~0u && q.guide == r.guide && q.info == r.info && q.mask == r.mask && ql.x == pos2 && ql.y == n_var &&
                    a.map.win[q.contig].chr_id == win.chr_id) {
                    const bool same = n_var == 0 || var_tags_equal(a.map, r.contig, r.pos, q.contig, q.pos, n_var, a.len);
                    dropped = same && pv_same_bases(a, r, q);
                }
            }
            if (a.exclude) {  // the guide's own locus: that chromosome position and strand, no mismatch, no variant
                const uint4 ex = a.exclude[r.guide];
                on = ex.x != UINT32_MAX && win.contig == ex.x && pos2 == ex.y && strand == ex.z && nm == 0u && n_var == 0;
            }
        }
        if (a.labels && have) {
            uint4 lab = make_uint4(0u, 0u, 0u, 0u);
            if (ok) lab = make_uint4(win.contig, pos2, n_var, (n_var ? VSC_VARIANT_VAR : 0u) | (dropped ? VSC_VARIANT_DUP : 0u) | (on ? VSC_VARIANT_ON_TARGET : 0u));
            a.labels[i] = lab;
        }
    }
    if (!a.rows_all) return;  // (uniform: a kernel argument)

    // this lane's contribution to its guide's rows
    const uint32_t g = ok ? r.guide : ~0u;
    unsigned long long cnt_all = 0, cnt_var = 0, pos_all = 0, pos_var = 0, f_all = 0, f_var = 0;
    uint32_t small = 0;  // on-targets met, dropped records: 8 bits each
    if (ok) {
        small = (on ? 1u : 0u) | (dropped ? 1u << 8 : 0u);
        if (!dropped && !on) {
            cnt_all = 1ull << (kPvCountBits * nm);
            if (kScored) {
                f_all = a.fixed[i];
                pos_all = f_all ? cnt_all : 0ull;
            }
            if (!kRef && n_var) {
                cnt_var = cnt_all;
                pos_var = pos_all;
                f_var = f_all;
            }
        }
    }
    // segmented reduction towards the first lane of every run of one guide: after the step with distance d a lane holds the
    // sum over the lanes [lane, lane + 2 d) of its run (the run is contiguous: the guide d lanes on is mine iff all between are)
    for (int d = 1; d < kWave; d <<= 1) {
        const uint32_t og = __shfl_down(g, d, kWave);  // (every lane takes part in every shuffle: no short-circuit in front of it)
        const bool mine = lane + (uint32_t)d < (uint32_t)kWave && og == g;
        const unsigned long long oca = __shfl_down(cnt_all, d, kWave);
        const uint32_t os = __shfl_down(small, d, kWave);
        cnt_all += mine ? oca : 0ull;
        small += mine ? os : 0u;
        if (!kRef) {
            const unsigned long long ocv = __shfl_down(cnt_var, d, kWave);
            cnt_var += mine ? ocv : 0ull;
        }
        if (kScored) {
            const unsigned long long opa = __shfl_down(pos_all, d, kWave), ofa = __shfl_down(f_all, d, kWave);
            pos_all += mine ? opa : 0ull;
            f_all += mine ? ofa : 0ull;
            if (!kRef) {
                const unsigned long long opv = __shfl_down(pos_var, d, kWave), ofv = __shfl_down(f_var, d, kWave);
                pos_var += mine ? opv : 0ull;
                f_var += mine ? ofv : 0ull;
            }
        }
    }
    const uint32_t left = __shfl_up(g, 1, kWave);
    if (g == ~0u || (lane > 0 && left == g)) return;
    const uint32_t field = (1u << kPvCountBits) - 1u;
    auto flush = [&](PatVarRow *row, unsigned long long c9, uint32_t n_dropped) {
#pragma unroll
        for (int k = 0; k <= VSC_MAX_MISMATCHES; ++k) {
            const uint32_t c = (uint32_t)(c9 >> (kPvCountBits * k)) & field;
            if (c) atomicAdd(&row->count[k], c);
        }
        if (small & 0xFFu) atomicOr(&row->on_target, 1u);
        if (n_dropped) atomicAdd(&row->dropped, (unsigned long long)n_dropped);
    };
    auto flush_table = [&](unsigned long long *row, unsigned long long f, unsigned long long p9) {
        if (f) atomicAdd(&row[0], f);
        uint32_t positive = 0;
#pragma unroll
        for (int k = 0; k <= VSC_MAX_MISMATCHES; ++k) {
            const uint32_t c = (uint32_t)(p9 >> (kPvCountBits * k)) & field;
            positive += c;
            if (c) atomicAdd(&row[2 + k], (unsigned long long)c);
        }
        if (positive) atomicAdd(&row[1], (unsigned long long)positive);
    };
    flush(a.rows_all + g, cnt_all, (small >> 8) & 0xFFu);
    if (kScored && a.table_all) flush_table(a.table_all + (size_t)g * kPatVarTableWords, f_all, pos_all);
    if (!kRef) {
        if (a.rows_var) flush(a.rows_var + g, cnt_var, 0u);
        if (kScored && a.table_var) flush_table(a.table_var + (size_t)g * kPatVarTableWords, f_var, pos_var);
    }
}

template <bool kRef> static hipError_t launch_pv(const PatVarArgs &args, hipStream_t stream)
{
    if (args.n == 0) return hipSuccess;
    if (args.len < kPatVarMinLen || args.len > kPatVarMaxLen) return hipErrorInvalidValue;
    const unsigned long long blocks = (args.n + kPvThreads - 1) / kPvThreads;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    if (args.fixed) hipLaunchKernelGGL((pattern_variant_kernel<kRef, true>), dim3((uint32_t)blocks), dim3(kPvThreads), 0, stream, args);
    else hipLaunchKernelGGL((pattern_variant_kernel<kRef, false>), dim3((uint32_t)blocks), dim3(kPvThreads), 0, stream, args);
    return hipGetLastError();
}

hipError_t launch_pattern_variant_merge(const PatVarArgs &args, hipStream_t stream) { return launch_pv<false>(args, stream); }
hipError_t launch_pattern_shadow(const PatVarArgs &args, hipStream_t stream) { return launch_pv<true>(args, stream); }

}  // namespace vsc
