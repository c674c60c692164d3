// vsc_effects.h - coding consequences of base edits (include/varscot_hip.h "CODE / SEGMENT / CODING / CODON /
// PARAMS / EFFECT / ROW / COVERAGE / FILTER") as what the host code (vsc_cds_build, vsc_codon_effect, vsc_effects_site_text)
// shares with the kernels of vsc_effects.hip.  A header of its own, as vsc_edit.h is; the shape, the site, the mask and the
// forward positions of the window are vsc_edit.h's, the planes vsc_efficiency.h's.
//
// effects_row below IS the walk over one candidate's window: effects_rows_kernel calls it with the candidate's MASK and keeps
// the row, effects_records_kernel calls it with word 1 of that row (the MASK bases inside segments - every base of a codon
// lies in a segment, so the effects are the same) and keeps the records, effects_filter_kernel keeps the verdict of
// effects_keep, vsc_effects_site_text calls it on planes packed from letters - one function, integers only, the same bits.
// Plain inline functions that a stand-alone program can include without a device.
#pragma once

#include <stdint.h>

#include "vsc_edit.h"

// (the walk keeps a codon's three positions and a segment in registers: every function below is inlined into it)
#define VSC_FX_INLINE __attribute__((always_inline)) inline

namespace vsc {

constexpr uint32_t kEffectsUndefined = 0xFFFFFFFFu;  // both words of the row of a candidate whose class is not defined
constexpr uint32_t kEffectsMaxCount = 0xFFFFFFFEu;   // candidates, segments and effects of one call
constexpr uint32_t kCdsNone = 0xFFFFFFFFu;           // no segment; no position
constexpr uint32_t kEffectBaseUnknown = 4u;          // effects_base: N, or not resident

// the classes of an effect; the index into ROW's 5-bit fields and into the require / forbid masks
enum EffectClass : uint32_t {
    kEffectSynonymous = 0,
    kEffectMissense,
    kEffectStopGained,
    kEffectStopLost,
    kEffectStartLost,
    kEffectUnknown,
    kEffectClasses
};

// the standard genetic code, indexed 16 b0 + 4 b1 + b2 (A C G T = 0 .. 3)
constexpr char kStandardCode[65] = "KNKNTTTTRSRSIIMIQHQHPPPPRRRRLLLLEDEDAAAAGGGGVVVV*Y*YSSSS*CWCLFLF";

// One segment as the functions below read it, two 16-byte loads: its global range (contig offset + position, 32-bit as
// contig_off is), its transcript, ci0 = shift + bases_before (the coding index of its first base in transcript order), the
// previous / next segment of its transcript in transcript order (kCdsNone: none), its strand and its transcript's shift.
struct alignas(16) CdsSeg {
    uint32_t gstart, gend, transcript, ci0;
    uint32_t prev, next, strand, shift;
};

// The segments as the kernels hold them: strictly ascending global starts (a second array of their own, which the search
// reads), no two overlapping.
struct CdsView {
    const uint32_t *gstart;
    const CdsSeg *seg;
    uint32_t n;
};

// the first segment that ends behind global position g (v.n: none) - the segment g lies in, or the next one: a lower bound
// over the starts, log2(n) dependent loads, and one look at the segment in front
__host__ __device__ VSC_FX_INLINE uint32_t cds_find(const CdsView &v, uint32_t g)
{
    uint32_t lo = 0, hi = v.n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (v.gstart[mid] <= g) lo = mid + 1u;
        else hi = mid;
    }
    if (lo > 0u && v.seg[lo - 1u].gend > g) return lo - 1u;
    return lo;
}

// the forward letter (0 .. 3) at global position x, kEffectBaseUnknown for an N or a base this object does not hold: the
// bounds first, then the class plane, then the 2-bit letter
__host__ __device__ VSC_FX_INLINE uint32_t effects_base(const EffPlanes &g, uint32_t x)
{
    const uint64_t first = g.first_word * 32u, end = (g.first_word + g.held_words) * 32u;
    if ((uint64_t)x < first || (uint64_t)x >= end) return kEffectBaseUnknown;
    const uint64_t at = (uint64_t)x - first, w = at >> 5;
    if (w >= g.n_words) return kEffectBaseUnknown;
    const uint32_t b = (uint32_t)at & 31u;
    if ((g.nm[w] >> b) & 1u) return kEffectBaseUnknown;
    return ((g.hi[w] >> b) & 1u) << 1 | ((g.lo[w] >> b) & 1u);
}

// the global position of coding index c of the transcript of a segment (kCdsNone: the transcript has no such base): at most
// two hops to either side, because a codon has three bases and no segment is empty.  (The segment travels as scalars, so
// that the walk's copy of it stays in registers.)
__host__ __device__ VSC_FX_INLINE uint32_t cds_position(const CdsView &v, uint32_t gstart, uint32_t gend, uint32_t ci0, uint32_t prev,
                                                        uint32_t next, uint32_t strand, uint32_t c)
{
    for (uint32_t h = 0; h < 2u && c < ci0; ++h) {
        if (prev >= v.n) return kCdsNone;
        const CdsSeg *q = v.seg + prev;
        gstart = q->gstart, gend = q->gend, ci0 = q->ci0, prev = q->prev, next = q->next;
    }
    if (c < ci0) return kCdsNone;
    for (uint32_t h = 0; h < 2u && c - ci0 >= gend - gstart; ++h) {
        if (next >= v.n) return kCdsNone;
        const CdsSeg *q = v.seg + next;
        gstart = q->gstart, gend = q->gend, ci0 = q->ci0, next = q->next;
    }
    if (c < ci0 || c - ci0 >= gend - gstart) return kCdsNone;
    return strand ? gend - 1u - (c - ci0) : gstart + (c - ci0);
}

// CODON: p[i] = the global position of the base with coding index 3 codon + i of the transcript of segment s, or kCdsNone
// (gstart .. strand: the fields of s)
__host__ __device__ VSC_FX_INLINE void codon_of(const CdsView &v, uint32_t gstart, uint32_t gend, uint32_t ci0, uint32_t prev, uint32_t next,
                                                uint32_t strand, uint32_t codon, uint32_t *p0, uint32_t *p1, uint32_t *p2)
{
    *p0 = cds_position(v, gstart, gend, ci0, prev, next, strand, 3u * codon);
    *p1 = cds_position(v, gstart, gend, ci0, prev, next, strand, 3u * codon + 1u);
    *p2 = cds_position(v, gstart, gend, ci0, prev, next, strand, 3u * codon + 2u);
}

// alt: the codon ref (16 b0 + 4 b1 + b2) with the bases of `edited` (bit i: base i) replaced by `letter`
__host__ __device__ VSC_FX_INLINE uint32_t effect_alt(uint32_t ref, uint32_t edited, uint32_t letter)
{
    uint32_t alt = ref;
    VSC_EFF_UNROLL
    for (uint32_t i = 0; i < 3u; ++i)
        if (edited >> i & 1u) alt = (alt & ~(3u << (4u - 2u * i))) | letter << (4u - 2u * i);
    return alt;
}

// the class of an effect, tested in the order of the definition; starts_whole: the transcript's first phase is 0 (its shift
// is 0 then and only then), so that codon 0 is its start codon; code: 64 amino-acid letters
__host__ __device__ VSC_FX_INLINE uint32_t effect_class(uint32_t ref, uint32_t alt, uint32_t codon, bool starts_whole, const uint8_t *code,
                                                        bool unknown)
{
    if (unknown) return kEffectUnknown;
    if (codon == 0u && starts_whole) return kEffectStartLost;
    const bool ref_stop = code[ref] == (uint8_t)'*', alt_stop = code[alt] == (uint8_t)'*';
    if (!ref_stop && alt_stop) return kEffectStopGained;
    if (ref_stop && !alt_stop) return kEffectStopLost;
    return code[ref] == code[alt] ? kEffectSynonymous : kEffectMissense;
}

// info of an effect: ref | alt << 6 | class << 12 | edited bases in the codon << 16 | at << 20
__host__ __device__ VSC_FX_INLINE uint32_t effect_info(uint32_t ref, uint32_t alt, uint32_t cls, uint32_t n_edited, uint32_t at)
{
    return ref | alt << 6 | cls << 12 | n_edited << 16 | at << 20;
}

// the window position of global position p in the window that starts at global position g0, win_len when it lies outside
__host__ __device__ VSC_FX_INLINE uint32_t effects_window_at(uint32_t p, uint32_t g0, uint32_t strand, const EditShape &s)
{
    const uint32_t f = p - g0;
    if (p < g0 || f >= s.win_len) return s.win_len;
    return strand ? s.win_len - 1u - f : f;
}

// ROW and EFFECTS of a candidate of a defined class on `strand` whose window starts at global position g0: the walk over the
// window in ascending forward order, at most win_len steps, the segment advancing with it.  mask: the candidate's MASK, or
// word 1 of its row.  *w0, *w1 = the row; emit(transcript, codon, info) is called once per effect, in the order of the
// definition.  `to` is the base the editor writes on the read strand; code: 64 amino-acid letters.
template <class Emit>
__host__ __device__ VSC_FX_INLINE void effects_row(const EffPlanes &g, const CdsView &v, const EditShape &s, uint32_t to, const uint8_t *code,
                                            uint32_t g0, uint32_t strand, uint32_t mask, uint32_t *w0, uint32_t *w1, Emit &&emit)
{
    uint32_t row0 = 0, row1 = 0;
    if (mask && v.n) {
        uint32_t k = cds_find(v, g0);
        // segment k as scalars (two 16-byte loads; no copy of the struct, which would live in scratch memory)
        uint32_t sg_start = 0, sg_end = 0, sg_tx = 0, sg_ci0 = 0, sg_prev = kCdsNone, sg_next = kCdsNone, sg_strand = 0, sg_shift = 0;
#define VSC_FX_LOAD_SEGMENT(k_)                                                                                    \
    do {                                                                                                           \
        const CdsSeg *q_ = v.seg + (k_);                                                                           \
        sg_start = q_->gstart, sg_end = q_->gend, sg_tx = q_->transcript, sg_ci0 = q_->ci0, sg_prev = q_->prev;    \
        sg_next = q_->next, sg_strand = q_->strand, sg_shift = q_->shift;                                          \
    } while (0)
        if (k < v.n) VSC_FX_LOAD_SEGMENT(k);
        for (uint32_t f = 0; f < s.win_len && k < v.n; ++f) {
            const uint32_t x = g0 + f;
            while (sg_end <= x) {  // (the segments do not overlap: their ends ascend as their starts do)
                if (++k >= v.n) break;
                VSC_FX_LOAD_SEGMENT(k);
            }
            if (k >= v.n) break;
            if (sg_start > x) continue;
            const uint32_t j = strand ? s.win_len - 1u - f : f;
            if (!(mask >> j & 1u)) continue;
            row1 |= 1u << j;
            const uint32_t ci = sg_ci0 + (sg_strand ? sg_end - 1u - x : x - sg_start), codon = ci / 3u;
            uint32_t p[3];
            codon_of(v, sg_start, sg_end, sg_ci0, sg_prev, sg_next, sg_strand, codon, &p[0], &p[1], &p[2]);
            uint32_t edited = 0, n_edited = 0, at = s.win_len;
            bool emitter = true;
            VSC_EFF_UNROLL
            for (uint32_t i = 0; i < 3u; ++i) {
                if (p[i] == kCdsNone) continue;
                const uint32_t ji = effects_window_at(p[i], g0, strand, s);
                if (ji >= s.win_len || !(mask >> ji & 1u)) continue;
                edited |= 1u << i;
                ++n_edited;
                if (ji < at) at = ji;
                if (p[i] < x) emitter = false;
            }
            if (!emitter) continue;
            bool unknown = false;
            uint32_t ref = 0;
            VSC_EFF_UNROLL
            for (uint32_t i = 0; i < 3u; ++i) {
                const uint32_t b = p[i] == kCdsNone ? kEffectBaseUnknown : effects_base(g, p[i]);
                if (b > 3u) unknown = true;
                ref = ref << 2 | ((sg_strand ? 3u - b : b) & 3u);
            }
            uint32_t alt = effect_alt(ref, edited, strand == sg_strand ? to : 3u - to);
            const uint32_t cls = effect_class(ref, alt, codon, sg_shift == 0u, code, unknown);
            if (unknown) ref = alt = 0;
            row0 += 1u << (5u * cls);
            emit(sg_tx, codon, effect_info(ref, alt, cls, n_edited, at));
        }
#undef VSC_FX_LOAD_SEGMENT
    }
    *w0 = row0;
    *w1 = row1;
}

// the effects of a row: the sum of the six 5-bit fields of word 0; 0 for the row of an undefined candidate
__host__ __device__ VSC_FX_INLINE uint32_t effects_count(uint32_t w0, uint32_t w1)
{
    if (w0 == kEffectsUndefined && w1 == kEffectsUndefined) return 0u;
    uint32_t n = 0;
    VSC_EFF_UNROLL
    for (uint32_t k = 0; k < kEffectClasses; ++k) n += w0 >> (5u * k) & 31u;
    return n;
}

// The FILTER rule: does a candidate of class cls with word 0 of its row pass?
__host__ __device__ VSC_FX_INLINE bool effects_keep(uint32_t cls, uint32_t w0, uint32_t require, uint32_t forbid)
{
    if (cls != kEffDefined) return false;
    uint32_t have = 0;
    VSC_EFF_UNROLL
    for (uint32_t k = 0; k < kEffectClasses; ++k)
        if (w0 >> (5u * k) & 31u) have |= 1u << k;
    return (require == 0u || (have & require) != 0u) && (have & forbid) == 0u;
}

}  // namespace vsc
