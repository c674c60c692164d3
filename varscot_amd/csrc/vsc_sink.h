// vsc_sink.h - device helpers of the kernels that read a pass's records where the search kernel left them (SinkInput,
// vsc_internal.h): the record decode, the region's LDS row table and the unpack of a lane's packed counters.  Used by the sink
// kernels of vsc_kernels.hip.
#pragma once

#include "vsc_device.h"

namespace vsc {

// The record decode, in two steps for a caller that has the record's words already (summary_kernel stages them through LDS).
// Is record word r a sentinel - a reserved slot nobody wrote?  (SEED only: the pairs of the SCAN form are all hits)
template <bool kSeed> __device__ __forceinline__ bool sink_sentinel(uint64_t r) { return kSeed && (r >> 63); }

// Record word r that is no sentinel (and, SCAN, the value word beside it; SEED: unused) of segment sg: pass-local read,
// strand, global position, mismatch mask.
template <bool kSeed>
__device__ __forceinline__ void sink_decode_word(const SinkInput &a, const SumSeg &sg, uint64_t r, uint32_t val, uint32_t &read, uint32_t &strand,
                                                 uint32_t &pos, uint32_t &mask)
{
    if (kSeed) {
        read = sg.first_read + (uint32_t)((r >> kRecReadShift) & (kRegionReads - 1));
        strand = (uint32_t)(r >> kRecStrandShift) & 1u;
        pos = ((uint32_t)(r >> kRecPosShift) >> a.pos_pad) + a.pos_base;
        mask = (uint32_t)r & kMask23;
    } else {
        read = (uint32_t)(r >> 33);
        strand = (uint32_t)(r >> 32) & 1u;
        pos = (uint32_t)r;
        mask = val & kMask23;
    }
}

// Record `at` of segment sg, loaded here (the value word in the SCAN form only): pass-local read, strand << 32 | global
// position, mismatch mask; false: a sentinel.
template <bool kSeed>
__device__ __forceinline__ bool sink_decode(const SinkInput &a, const SumSeg &sg, uint64_t at, uint32_t &read, uint64_t &locus, uint32_t &mask)
{
    const uint64_t r = a.recs[at];
    if (sink_sentinel<kSeed>(r)) return false;
    uint32_t strand, pos;
    sink_decode_word<kSeed>(a, sg, r, kSeed ? 0u : a.vals[at], read, strand, pos, mask);
    locus = (uint64_t)strand << 32 | pos;
    return true;
}

// The counters a lane packed into one word (counter k in bits kSumCountBits * k .., k = NM = 0 .. VSC_MAX_MISMATCHES) added
// to row[k]: an LDS row of 32-bit counters or a result row of 64-bit words.
template <class T> __device__ __forceinline__ void sink_add_counts(T *row, uint64_t packed)
{
#pragma unroll
    for (int k = 0; k <= VSC_MAX_MISMATCHES; ++k) {
        const uint32_t c = (uint32_t)(packed >> (kSumCountBits * k)) & ((1u << kSumCountBits) - 1u);
        if (c) atomicAdd(&row[k], (T)c);
    }
}

// The LDS table of a region's result rows (kSumWords words per read: one 64-bit sum in sum[], kSumCounts counters in cnt[]),
// gathered while a SEED workgroup's tiles lie in the region.  kRows = kRegionReads, or twice that: the rows from kRegionReads
// on are a second set over the same reads for a second result array.  Both calls are made by all kThreads threads of the
// workgroup and synchronise it.
template <uint32_t kThreads, uint32_t kRows>
__device__ __forceinline__ void sink_table_zero(unsigned long long (&sum)[kRows], uint32_t (&cnt)[kRows * kSumCounts], uint32_t t)
{
    for (uint32_t i = t; i < kRows * kSumCounts; i += kThreads) cnt[i] = 0;
    for (uint32_t i = t; i < kRows; i += kThreads) sum[i] = 0;
    block_sync();
}

// the table -> the rows of segment sg's reads in `out` (second set: out_in), one agent-scope atomic per nonzero
// (read, field); leaves the table zeroed
template <uint32_t kThreads, uint32_t kRows>
__device__ __forceinline__ void sink_table_flush(unsigned long long (&sum)[kRows], uint32_t (&cnt)[kRows * kSumCounts], uint32_t t, const SumSeg &sg,
                                                 unsigned long long *out, unsigned long long *out_in = nullptr)
{
    block_sync();
    for (uint32_t i = t; i < kRows * kSumWords; i += kThreads) {
        const uint32_t r = i / kSumWords, f = i % kSumWords;
        unsigned long long v;
        if (f == 0) {
            v = sum[r];
            sum[r] = 0;
        } else {
            v = cnt[r * kSumCounts + f - 1];
            cnt[r * kSumCounts + f - 1] = 0;
        }
        if constexpr (kRows > (uint32_t)kRegionReads) {
            if (v) atomicAdd(&(r < (uint32_t)kRegionReads ? out : out_in)[(size_t)(sg.first_read + (r & (kRegionReads - 1))) * kSumWords + f], v);
        } else {
            if (v) atomicAdd(&out[(size_t)(sg.first_read + r) * kSumWords + f], v);
        }
    }
    block_sync();
}

}  // namespace vsc
