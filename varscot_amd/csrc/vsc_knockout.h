// vsc_knockout.h - knock-out design (include/varscot_hip.h "SHAPE / CUT / DEFINED / CODING CUT / TRANSCRIPT / K /
// SHIFTED / WALK / NMD / ROW / COVERAGE / FILTER") as what the host code (vsc_knockout_site_text, the per-transcript table and
// the occupancy bitmap of vsc_cds_build), the kernels of vsc_knockout.hip and the stand-alone check share.  A header of its
// own, as vsc_effects.h is, whose segments (CdsSeg, CdsView), lower bound (cds_find) and letters (effects_base) it reuses.
//
// What is new here is the walk ALONG a transcript: a cursor that stands on one coding base, advances one transcript base at a
// time and hops to the next segment when its segment ends.  There is no lower bound and no cds_position inside the walk.
// knockout_row IS the definition: the rows kernel calls its two halves (knockout_find where the candidate lies,
// knockout_finish in the drained queue), the filter kernel, vsc_knockout_site_text and the stand-alone check call it whole.
// Integers only; plain inline functions that a stand-alone program can include without a device.
#pragma once

#include <stdint.h>

#include "vsc_effects.h"

namespace vsc {

constexpr uint32_t kKoUndefined = 0xFFFFFFFFu;  // the four words of the row of a candidate that is not DEFINED
constexpr uint32_t kKoMaxCount = 0xFFFFFFFEu;   // candidates of one call
constexpr uint32_t kKoMaxCodons = 4096u;
constexpr uint32_t kKoEnd = 0xFFFFu, kKoCap = 0xFFFEu, kKoUnknown = 0xFFFDu;  // d_s where the walk finds no stop
// the occupancy bitmap: one bit per block of 2^kKoBlockBits global positions that overlaps a segment
constexpr uint32_t kKoBlockBits = 8u;

// the flag bits of ROW's word 2, from bit 24 on; the bits of the filter's require / forbid masks
enum KoFlag : uint32_t { kKoFirst = 1u, kKoLast = 2u, kKoPtc1 = 4u, kKoPtc2 = 8u, kKoNmd1 = 16u, kKoNmd2 = 32u, kKoUnknownFlag = 64u };
constexpr uint32_t kKoFlagBits = 7u;
constexpr uint32_t kKoWalkFlags = kKoPtc1 | kKoPtc2 | kKoNmd1 | kKoNmd2 | kKoUnknownFlag;  // what only a walk can tell

struct KoShape {
    uint32_t site_len, cut, nmd_window, start_window, max_codons;
};

struct KoFilter {
    uint32_t min_frac, max_frac, min_edge, require, forbid;
};

// TRANSCRIPT: what the walk needs of a transcript beside its segments, 16 bytes, derived on the host with the CDS:
// shift, E_t = shift + B_t, J_t = ci of the first base of its last segment in transcript order, its segments (0: unused)
struct alignas(16) KoTx {
    uint32_t shift, end, junction, n_seg;
};

// what knockout_find hands to the walk: the segment of the cut and K
struct KoCut {
    uint32_t seg, k;
};

__host__ __device__ VSC_FX_INLINE bool knockout_shape_valid(const KoShape &s)
{
    return s.site_len >= 16u && s.site_len <= 32u && s.cut >= 1u && s.cut < s.site_len && s.nmd_window <= 65535u && s.start_window <= 65535u &&
           s.max_codons >= 1u && s.max_codons <= kKoMaxCodons;
}

__host__ __device__ VSC_FX_INLINE bool knockout_filter_valid(const KoFilter &f)
{
    return f.min_frac <= f.max_frac && f.max_frac <= 65535u && f.min_edge <= 255u && !(f.require >> kKoFlagBits) && !(f.forbid >> kKoFlagBits);
}

// DEFINED and CUT: is (contig, pos, strand) a valid locus whose site lies inside its contig?  *gx = the global cut coordinate:
// the break lies between global forward bases gx - 1 and gx, both of which lie in the site.
__host__ __device__ VSC_FX_INLINE bool knockout_cut(const uint32_t *contig_off, const uint32_t *contig_end, uint32_t n_contigs, const KoShape &s,
                                                    uint32_t contig, uint32_t pos, uint32_t strand, uint32_t *gx)
{
    if (contig >= n_contigs || strand > 1u) return false;
    const uint32_t off = contig_off[contig], len = contig_end[contig] - off;
    if (pos > len || len - pos < s.site_len) return false;  // pos + site_len <= len, without the overflow
    *gx = off + pos + (strand ? s.site_len - s.cut : s.cut);
    return true;
}

// may global position g lie in a segment?  (bits: one per block; beyond the bitmap: no)
__host__ __device__ VSC_FX_INLINE bool knockout_occupied(const uint32_t *bitmap, uint32_t n_blocks, uint32_t g)
{
    const uint32_t b = g >> kKoBlockBits;
    return b < n_blocks && (bitmap[b >> 5] >> (b & 31u) & 1u);
}

// the NONCODING row
__host__ __device__ VSC_FX_INLINE void knockout_noncoding(bool junction, uint32_t *row)
{
    row[0] = 0xFFFFFFFFu, row[1] = 0u, row[2] = junction ? 0x80000000u : 0u, row[3] = 0u;
}

// CODING CUT of the defined cut gx: true with the segment and K, or false with *junction.  One lower bound.
__host__ __device__ VSC_FX_INLINE bool knockout_find(const CdsView &v, uint32_t gx, KoCut *cut, bool *junction)
{
    *junction = false;
    if (!v.n) return false;
    const uint32_t k = cds_find(v, gx - 1u);  // the segment of base gx - 1, or the next one
    if (k >= v.n) return false;
    const CdsSeg *q = v.seg + k;
    const uint32_t gstart = q->gstart, gend = q->gend;
    const bool left = gstart <= gx - 1u;  // (cds_find: gend > gx - 1)
    if (left && gend > gx) {
        cut->seg = k;
        cut->k = q->ci0 + (q->strand ? gend - gx : gx - gstart);  // ci(gx) on '+', ci(gx - 1) on '-'
        return true;
    }
    // gx - 1 lies in segment k, which ends at gx; or gx is the first base of segment k, or of the one behind it
    *junction = left || gstart == gx || (k + 1u < v.n && v.seg[k + 1u].gstart == gx);
    return false;
}

// The cursor: one coding base of a transcript - its global position, the bases its segment still has from it on (itself
// included) in the direction it moves, and the segment that follows in that direction.  dead: it moved off the transcript.
struct KoCursor {
    uint32_t g, left, link;
    bool dead;
};

// the letter under the cursor in transcript orientation, kEffectBaseUnknown for an N, a base not resident, a dead cursor
__host__ __device__ VSC_FX_INLINE uint32_t knockout_letter(const EffPlanes &g, const KoCursor &c, uint32_t strand)
{
    if (c.dead) return kEffectBaseUnknown;
    const uint32_t b = effects_base(g, c.g);
    return b > 3u ? kEffectBaseUnknown : (strand ? 3u - b : b);
}

// one transcript base on (kBack: one base back), into the next (previous) segment where this one ends
template <bool kBack> __host__ __device__ VSC_FX_INLINE void knockout_step(const CdsView &v, uint32_t strand, KoCursor *c)
{
    if (c->dead) return;
    const bool down = (strand != 0u) != kBack;  // towards lower forward positions
    if (--c->left) {
        c->g = down ? c->g - 1u : c->g + 1u;
        return;
    }
    if (c->link >= v.n) {
        c->dead = true;
        return;
    }
    const CdsSeg *q = v.seg + c->link;
    const uint32_t gstart = q->gstart, gend = q->gend;
    c->left = gend - gstart;
    c->g = down ? gend - 1u : gstart;
    c->link = kBack ? q->prev : q->next;
}

// WALK(s) from a coding cut: d_s; for a PTC *first = the transcript index of the stop codon's first base, *e = 1 + that of its
// third.  gstart .. next: the fields of the cut's segment; gk: the global position of transcript base K; pre[r] = the letter
// of transcript index 3 codon + r for r < frame (kEffectBaseUnknown: unknown; the indices below shift are not read).
__host__ __device__ VSC_FX_INLINE uint32_t knockout_walk(const EffPlanes &g, const CdsView &v, const KoShape &sh, const KoTx &tx, const uint8_t *code,
                                                         uint32_t s, uint32_t gstart, uint32_t gend, uint32_t next, uint32_t strand, uint32_t gk,
                                                         uint32_t k, uint32_t pre0, uint32_t pre1, uint32_t *first, uint32_t *e)
{
    const uint32_t codon = k / 3u, frame = k % 3u;
    KoCursor c{gk, strand ? gk - gstart + 1u : gend - gk, next, false};
    for (uint32_t i = 0; i < s; ++i) knockout_step<false>(v, strand, &c);
    uint32_t j = k + s;  // the transcript index under the cursor
    for (uint32_t n = 0; n < sh.max_codons; ++n) {
        const uint32_t have = n ? 0u : frame;             // the codon's bases in front of the break
        const uint32_t last = j + 2u - have;              // the transcript index of its third base
        if (last >= tx.end) return kKoEnd;
        const uint32_t head = have ? 3u * codon : j;      // ... and of its first
        uint32_t idx = 0;
        bool unknown = false;
        VSC_EFF_UNROLL
        for (uint32_t r = 0; r < 3u; ++r) {
            uint32_t b;
            if (r < have) {
                b = r ? pre1 : pre0;
            } else {
                b = knockout_letter(g, c, strand);
                knockout_step<false>(v, strand, &c);
                ++j;
            }
            if (b > 3u) unknown = true;
            idx = idx << 2 | (b & 3u);
        }
        if (head < tx.shift) continue;  // the codon is skipped
        if (unknown) return kKoUnknown;
        if (code[idx] == (uint8_t)'*') {
            *first = head;
            *e = last + 1u;
            return n;
        }
    }
    return kKoCap;
}

// NMD(s) of a PTC
__host__ __device__ VSC_FX_INLINE bool knockout_nmd(const KoShape &sh, const KoTx &tx, uint32_t first, uint32_t e)
{
    if (tx.n_seg < 2u) return false;
    if ((int64_t)tx.junction - (int64_t)e < (int64_t)sh.nmd_window) return false;
    return sh.start_window == 0u || first - tx.shift >= sh.start_window;
}

// ROW of a coding cut without its walks: words 0 .. 2 with the flags FIRST and LAST alone, word 3 = 0.  What the filter's
// tests on frac and edge need.
__host__ __device__ VSC_FX_INLINE void knockout_head(const CdsView &v, const KoTx *txs, uint32_t gx, const KoCut &cut, uint32_t *row)
{
    const CdsSeg *q = v.seg + cut.seg;
    const uint32_t gstart = q->gstart, gend = q->gend, t = q->transcript;
    const KoTx tx = txs[t];
    const uint32_t codon = cut.k / 3u, frame = cut.k % 3u;
    const uint32_t frac = (uint32_t)(((uint64_t)(cut.k - tx.shift) << 16) / (uint64_t)(tx.end - tx.shift));
    uint32_t edge = gx - gstart < gend - gx ? gx - gstart : gend - gx;
    if (edge > 255u) edge = 255u;
    const uint32_t flags = (q->prev >= v.n ? (uint32_t)kKoFirst : 0u) | (q->next >= v.n ? (uint32_t)kKoLast : 0u);
    row[0] = t, row[1] = codon | frame << 30, row[2] = frac | edge << 16 | flags << 24, row[3] = 0u;
}

// ROW of a coding cut: the head, the letters in front of the break, both walks
__host__ __device__ VSC_FX_INLINE void knockout_finish(const EffPlanes &g, const CdsView &v, const KoTx *txs, const KoShape &sh, const uint8_t *code,
                                                       uint32_t gx, const KoCut &cut, uint32_t *row)
{
    knockout_head(v, txs, gx, cut, row);
    const CdsSeg *q = v.seg + cut.seg;
    const uint32_t gstart = q->gstart, gend = q->gend, strand = q->strand, prev = q->prev, next = q->next;
    const KoTx tx = txs[q->transcript];
    const uint32_t codon = cut.k / 3u, frame = cut.k % 3u;
    const uint32_t gk = strand ? gx - 1u : gx;  // transcript base K
    // the bases K - 1, K - 2 of the codon the break lies in: one cursor, backwards, not below shift
    uint32_t pre[2] = {kEffectBaseUnknown, kEffectBaseUnknown};
    KoCursor b{gk, strand ? gend - gk : gk - gstart + 1u, prev, false};
    VSC_EFF_UNROLL
    for (uint32_t i = 0; i < 2u; ++i) {
        const uint32_t r = 1u - i;
        if (r >= frame || 3u * codon + r < tx.shift) continue;
        knockout_step<true>(v, strand, &b);
        pre[r] = knockout_letter(g, b, strand);
    }
    uint32_t flags = 0, d[2];
    VSC_EFF_UNROLL
    for (uint32_t s = 1u; s <= 2u; ++s) {
        uint32_t first = 0, e = 0;
        const uint32_t ds = knockout_walk(g, v, sh, tx, code, s, gstart, gend, next, strand, gk, cut.k, pre[0], pre[1], &first, &e);
        d[s - 1u] = ds;
        if (ds == kKoUnknown) flags |= kKoUnknownFlag;
        if (ds < kKoUnknown) {
            flags |= kKoPtc1 << (s - 1u);
            if (knockout_nmd(sh, tx, first, e)) flags |= kKoNmd1 << (s - 1u);
        }
    }
    row[2] |= flags << 24;
    row[3] = d[0] | d[1] << 16;
}

// ROW of locus (contig, pos, strand): the definition, whole
__host__ __device__ VSC_FX_INLINE void knockout_row(const EffPlanes &g, const CdsView &v, const KoTx *txs, const KoShape &sh, const uint8_t *code,
                                                    uint32_t contig, uint32_t pos, uint32_t strand, uint32_t *row)
{
    uint32_t gx = 0;
    if (!knockout_cut(g.contig_off, g.contig_end, g.n_contigs, sh, contig, pos, strand, &gx)) {
        row[0] = row[1] = row[2] = row[3] = kKoUndefined;
        return;
    }
    KoCut cut{};
    bool junction = false;
    if (!knockout_find(v, gx, &cut, &junction)) {
        knockout_noncoding(junction, row);
        return;
    }
    knockout_finish(g, v, txs, sh, code, gx, cut, row);
}

__host__ __device__ VSC_FX_INLINE bool knockout_row_defined(const uint32_t *row)
{
    return !(row[0] == kKoUndefined && row[1] == kKoUndefined && row[2] == kKoUndefined && row[3] == kKoUndefined);
}

// is the row that of a coding cut?  (a transcript index is at most 0xFFFFFFFD)
__host__ __device__ VSC_FX_INLINE bool knockout_row_coding(const uint32_t *row) { return row[0] != 0xFFFFFFFFu; }

// FILTER's tests that need no walk: frac and edge, and the flags FIRST and LAST
__host__ __device__ VSC_FX_INLINE bool knockout_keep_head(const uint32_t *row, const KoFilter &f)
{
    const uint32_t frac = row[2] & 0xFFFFu, edge = row[2] >> 16 & 0xFFu, flags = row[2] >> 24 & (kKoFirst | kKoLast);
    return frac >= f.min_frac && frac <= f.max_frac && edge >= f.min_edge && (flags & f.require & ~kKoWalkFlags) == (f.require & ~kKoWalkFlags) &&
           !(flags & f.forbid);
}

// FILTER
__host__ __device__ VSC_FX_INLINE bool knockout_keep(const uint32_t *row, const KoFilter &f)
{
    if (!knockout_row_defined(row) || !knockout_row_coding(row)) return false;
    const uint32_t flags = row[2] >> 24 & 0x7Fu;
    return knockout_keep_head(row, f) && (flags & f.require) == f.require && !(flags & f.forbid);
}

}  // namespace vsc
