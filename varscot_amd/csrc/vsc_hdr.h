// vsc_hdr.h - HDR knock-in design: reach, re-cut block and silent blocking substitution of every (candidate, edit) pair (DESIGN
// 4.34, include/varscot_hip.h "SHAPE / CONTEXT / EDITS / READ / SEEN / BLOCKED / SUBSTITUTE / PAIR / ROW / COVERAGE / FILTER") as
// what the host code (vsc_hdr_site_text) shares with the kernels of vsc_hdr.hip.  A header of its own, as vsc_prime.h is: the
// edit entry, its occupancy bitmap and its lower bound are vsc_prime.h's, the segment search and the codon vsc_effects.h's, the
// planes, the window and the reverse complement vsc_efficiency.h's - called, not copied.
//
// hdr_read / hdr_seen / hdr_blocked / hdr_substitute / hdr_pair ARE the pair of one context with one edit, hdr_allowed_cds IS
// ALLOWED against a CDS, hdr_walk IS the join with the edits: hdr_rows_kernel, hdr_pairs_kernel and hdr_filter_kernel call them
// for every candidate, vsc_hdr_site_text and the stand-alone check call them on the host - one function each, integers only, the
// same bits.  E and S are shifts and masks over the two 64-bit planes of the context.  Plain inline functions that a stand-alone
// program can include without a device.
#pragma once

#include <stdint.h>

#include "vsc_effects.h"
#include "vsc_prime.h"

namespace vsc {

constexpr uint32_t kHdrUndefined = 0xFFFFFFFFu;  // both words of the row of a candidate whose class is not defined
constexpr uint32_t kHdrMaxCount = 0xFFFFFFFEu;   // candidates, edits and pairs of one call
constexpr uint32_t kHdrNoBlock = 0xFFFFFFFFu;    // the block word of a pair without a substitution
constexpr uint32_t kHdrMaxFlank = 32;            // up and down
constexpr uint32_t kHdrMaxPam = 8, kHdrMaxSeed = 16, kHdrMaxProto = 32, kHdrMaxDist = 63;
enum HdrShapeFlag : uint32_t { kHdrSubstitute = 1u, kHdrSubSeed = 2u, kHdrSubNoncoding = 4u };
enum HdrFlag : uint32_t { kHdrBPam = 1u, kHdrBSeed = 2u, kHdrBProto = 4u, kHdrSubbedPam = 8u, kHdrSubbedSeed = 16u, kHdrOpen = 32u };
constexpr uint32_t kHdrFlags = 6;
constexpr uint32_t kHdrBlocked = kHdrBPam | kHdrBSeed | kHdrBProto;
// what ALLOWED(r) gives: bits 0 .. 3 the read letters that may be written at reference context position r, bit 4: r lies in a segment
constexpr uint32_t kHdrAnyLetter = 15u, kHdrCoding = 16u;

struct HdrShape {
    uint32_t up, site_len, down, cut, max_dist, anchor;
    uint32_t pam_start, pam_len, pam_accept[kHdrMaxPam];
    uint32_t seed_start, seed_len, proto_start, proto_len, min_seed_mm, min_proto_mm;
    uint32_t flags;
};

__host__ __device__ inline uint32_t hdr_context_len(const HdrShape &s) { return s.up + s.site_len + s.down; }

// Is s a shape the definition allows?
__host__ __device__ inline bool hdr_shape_valid(const HdrShape &s)
{
    if (s.site_len < kEffMinSite || s.site_len > kEffMaxSite || s.up > kHdrMaxFlank || s.down > kHdrMaxFlank) return false;
    if (hdr_context_len(s) > kEffMaxContext) return false;
    if (s.cut < 1u || s.cut > s.site_len - 1u || s.max_dist > kHdrMaxDist || s.anchor > 1u) return false;
    if (s.pam_len > kHdrMaxPam || s.pam_start > s.site_len || s.pam_len > s.site_len - s.pam_start) return false;
    for (uint32_t j = 0; j < kHdrMaxPam; ++j)
        if (j < s.pam_len ? (s.pam_accept[j] < 1u || s.pam_accept[j] > kHdrAnyLetter) : s.pam_accept[j] != 0u) return false;
    if (s.seed_len > kHdrMaxSeed || s.seed_start > s.site_len || s.seed_len > s.site_len - s.seed_start) return false;
    if (s.proto_len > kHdrMaxProto || s.proto_start > s.site_len || s.proto_len > s.site_len - s.proto_start) return false;
    if (s.min_seed_mm > s.seed_len || s.min_proto_mm > s.proto_len) return false;
    return (s.flags & ~(kHdrSubstitute | kHdrSubSeed | kHdrSubNoncoding)) == 0u;
}

// CONTEXT: the class of locus (contig, pos, strand), tested in the order of EffClass, and - for kEffDefined - the planes of its
// C bases in read orientation.  (The shape does not go through eff_shape_valid: its 16-base flank limit is the efficiency
// models', eff_window serves any C up to 64.)
__host__ __device__ inline uint32_t hdr_context(const EffPlanes &g, const HdrShape &s, uint32_t contig, uint32_t pos, uint32_t strand, uint64_t *ch,
                                                uint64_t *cl)
{
    const EffShape c{s.up, s.site_len, s.down, 0u, 0u};
    return eff_context(g, c, contig, pos, strand, ch, cl);
}

// F0 of a defined candidate: the context's first forward position on its contig
__host__ __device__ inline uint32_t hdr_first_forward(uint32_t pos, uint32_t strand, const HdrShape &s) { return pos - (strand ? s.down : s.up); }

// bit q of the result = bit q + n of x, for any signed n (0 where there is no such bit)
__host__ __device__ inline uint64_t hdr_from(uint64_t x, int32_t n) { return n >= 0 ? prime_shr(x, (uint32_t)n) : prime_shl(x, (uint32_t)-n); }
// the bits below n / the bits [lo, hi) of a plane, for any signed bounds
__host__ __device__ inline uint64_t hdr_below(int32_t n) { return n <= 0 ? 0ull : eff_low_bits((uint32_t)n); }
__host__ __device__ inline uint64_t hdr_span(int32_t lo, int32_t hi) { return hdr_below(hi) & ~hdr_below(lo); }

// the forward global positions an edit IN REACH of a candidate can start at: [*lo, *hi], g0 = the context's first global
// position.  With Kf = the break in forward context positions (K on '+', C - K on '-'), dist <= max_dist is pos - F0 <= Kf +
// max_dist and pos - F0 + del_len >= Kf - max_dist; del_len is at most 16.  hi - lo <= 64.
__host__ __device__ inline void hdr_reach(const HdrShape &s, uint32_t g0, uint32_t strand, uint32_t *lo, uint32_t *hi)
{
    const uint32_t C = hdr_context_len(s), K = s.up + s.cut, kf = strand ? C - K : K, back = s.max_dist + kPrimeMaxIndel;
    *lo = g0 + (kf > back ? kf - back : 0u);
    *hi = g0 + (kf + s.max_dist < C ? kf + s.max_dist : C);
}

// READ: is the edit (f = its global position - g0, f >= 0, on the candidate's contig) in reach of the candidate?  Then *e0 is
// where it starts in read orientation, (*ih, *il) are the planes of I and *reach = dist | side << 6.
__host__ __device__ inline bool hdr_read(const HdrShape &s, uint32_t strand, uint32_t f, const PrimeEdit &e, uint32_t *e0, uint64_t *ih,
                                         uint64_t *il, uint32_t *reach)
{
    const uint32_t C = hdr_context_len(s), del = prime_del_len(e), ins = prime_ins_len(e);
    if (f > C || del > C - f) return false;  // [pos, pos + del_len) inside [F0, F0 + C); del_len 0: F0 <= pos <= F0 + C
    const uint32_t at = strand ? C - f - del : f, e1 = at + del, K = s.up + s.cut;
    const uint32_t side = e1 < K ? 1u : at > K ? 2u : 0u;
    const uint32_t dist = side == 1u ? K - e1 : side == 2u ? at - K : 0u;
    if (dist > s.max_dist) return false;
    *e0 = at;
    *reach = dist | side << 6;
    uint64_t h = prime_gather16(e.ins >> 1), l = prime_gather16(e.ins);
    if (strand && ins) {
        h = eff_revcomp(h, ins);
        l = eff_revcomp(l, ins);
    }
    *ih = h;
    *il = l;
    return true;
}

// SEEN: the planes of S, the site the nuclease finds on the repaired allele held at the PAM side, and *have = the site
// positions that hold a letter.  The result is a = s0 + shift: site position q is position x = a + q of E = R[0, e0) + I +
// R[e0 + del, C).  E is never built whole (it may be 80 letters long): its three parts are shifted into the site's window and
// joined under their masks, as prime_edited joins them.
__host__ __device__ inline int32_t hdr_seen(const HdrShape &s, uint64_t ch, uint64_t cl, uint32_t e0, uint32_t del, uint32_t ins, uint64_t ih,
                                            uint64_t il, uint64_t *sh, uint64_t *sl, uint64_t *have)
{
    const int32_t delta = (int32_t)ins - (int32_t)del, C = (int32_t)hdr_context_len(s);
    const bool moved = s.anchor ? e0 < s.up + s.site_len : e0 + del <= s.up;
    const int32_t a = (int32_t)s.up + (moved ? delta : 0);
    const int32_t i0 = (int32_t)e0 - a, i1 = i0 + (int32_t)ins;  // the site positions of the inserted letters: [i0, i1)
    const uint64_t head = hdr_below(i0), mid = hdr_span(i0, i1), tail = ~hdr_below(i1);
    const uint64_t in = hdr_span(-a, C + delta - a) & eff_low_bits(s.site_len);
    *sh = ((hdr_from(ch, a) & head) | (hdr_from(ih, -i0) & mid) | (hdr_from(ch, a - delta) & tail)) & in;
    *sl = ((hdr_from(cl, a) & head) | (hdr_from(il, -i0) & mid) | (hdr_from(cl, a - delta) & tail)) & in;
    *have = in;
    return a;
}

// the site positions where S differs from the reference site (a position without a letter differs)
__host__ __device__ inline uint64_t hdr_differs(const HdrShape &s, uint64_t ch, uint64_t cl, uint64_t sh, uint64_t sl, uint64_t have)
{
    return (sh ^ (ch >> s.up)) | (sl ^ (cl >> s.up)) | ~have;
}

// BLOCKED: flag bits 0 .. 2 of a pair and its seed_mm / proto_mm.  accept: s.pam_accept, or a copy of it where a lane may index
// it (the kernels keep one in LDS).  The letters the PAM accepts become four masks over the site, one per letter.
__host__ __device__ inline uint32_t hdr_blocked(const HdrShape &s, const uint32_t *accept, uint64_t differs, uint64_t sh, uint64_t sl, uint64_t have,
                                                uint32_t *seed_mm, uint32_t *proto_mm)
{
    uint64_t ok0 = 0, ok1 = 0, ok2 = 0, ok3 = 0;  // (four scalars: an array would live in scratch memory)
    VSC_EFF_UNROLL
    for (uint32_t j = 0; j < kHdrMaxPam; ++j) {
        const uint32_t set = j < s.pam_len ? accept[j] : 0u;
        ok0 |= (uint64_t)(set & 1u) << (s.pam_start + j);
        ok1 |= (uint64_t)(set >> 1 & 1u) << (s.pam_start + j);
        ok2 |= (uint64_t)(set >> 2 & 1u) << (s.pam_start + j);
        ok3 |= (uint64_t)(set >> 3 & 1u) << (s.pam_start + j);
    }
    const uint64_t accepted = ((~sh & ~sl & ok0) | (~sh & sl & ok1) | (sh & ~sl & ok2) | (sh & sl & ok3)) & have;
    *seed_mm = (uint32_t)__builtin_popcountll(differs & prime_range(s.seed_start, s.seed_start + s.seed_len));
    *proto_mm = (uint32_t)__builtin_popcountll(differs & prime_range(s.proto_start, s.proto_start + s.proto_len));
    uint32_t f = 0;
    if (prime_range(s.pam_start, s.pam_start + s.pam_len) & ~accepted) f |= kHdrBPam;
    if (s.min_seed_mm && *seed_mm >= s.min_seed_mm) f |= kHdrBSeed;
    if (s.min_proto_mm && *proto_mm >= s.min_proto_mm) f |= kHdrBProto;
    return f;
}

// the reference context position of site position q of S (a slot), a = what hdr_seen returned
__host__ __device__ inline uint32_t hdr_slot_reference(int32_t a, uint32_t q, uint32_t e0, uint32_t del, uint32_t ins)
{
    const int32_t x = a + (int32_t)q;
    return (uint32_t)(x < (int32_t)e0 ? x : x - ((int32_t)ins - (int32_t)del));
}

// SUBSTITUTE of a pair that is not BLOCKED: the block word of the first try that holds and *flag = its flag, or kHdrNoBlock and
// kHdrOpen.  allowed(r): ALLOWED of reference context position r as a letter set | kHdrCoding.
template <class Allowed>
__host__ __device__ VSC_FX_INLINE uint32_t hdr_substitute(const HdrShape &s, const uint32_t *accept, uint64_t differs, uint64_t sh, uint64_t sl, uint64_t have,
                                                   int32_t a, uint32_t e0, uint32_t del, uint32_t ins, uint32_t seed_mm, Allowed &&allowed,
                                                   uint32_t *flag)
{
    *flag = kHdrOpen;
    if (!(s.flags & kHdrSubstitute)) return kHdrNoBlock;
    const int32_t i0 = (int32_t)e0 - a;
    const uint64_t slots = have & ~hdr_span(i0, i0 + (int32_t)ins);  // an inserted letter is not a slot
    for (uint32_t j = 0; j < kHdrMaxPam; ++j) {
        if (j >= s.pam_len) break;
        const uint32_t q = s.pam_start + j, want = ~accept[j] & kHdrAnyLetter;
        if (!(slots >> q & 1u) || !want) continue;
        const uint32_t r = hdr_slot_reference(a, q, e0, del, ins), set = allowed(r);
        if (!(set & want)) continue;
        *flag = kHdrSubbedPam;
        return q | (uint32_t)__builtin_ctz(set & want) << 8 | (set >> 4 & 1u) << 10 | r << 16;
    }
    if (!(s.flags & kHdrSubSeed) || !s.min_seed_mm || seed_mm + 1u < s.min_seed_mm) return kHdrNoBlock;
    for (uint32_t k = 0; k < kHdrMaxSeed; ++k) {
        if (k >= s.seed_len) break;
        const uint32_t q = s.anchor ? s.seed_start + s.seed_len - 1u - k : s.seed_start + k;  // from the PAM side outward
        if (!(slots >> q & 1u) || (differs >> q & 1u)) continue;
        const uint32_t now = (uint32_t)(sh >> q & 1u) << 1 | (uint32_t)(sl >> q & 1u), want = kHdrAnyLetter & ~(1u << now);
        const uint32_t r = hdr_slot_reference(a, q, e0, del, ins), set = allowed(r);
        if (!(set & want)) continue;
        *flag = kHdrSubbedSeed;
        return q | (uint32_t)__builtin_ctz(set & want) << 8 | (set >> 4 & 1u) << 10 | r << 16;
    }
    return kHdrNoBlock;
}

// PAIR of a defined candidate (planes ch, cl, strand) with an edit at f = its global position - g0 on the candidate's contig: is
// the edit in reach?  Then *info = dist | side << 6 | seed_mm << 8 | proto_mm << 13 | flags << 24 and *block = the substitution.
// allowed(r) is asked only for a pair that is in reach and not BLOCKED.
template <class Allowed>
__host__ __device__ VSC_FX_INLINE bool hdr_pair(const HdrShape &s, const uint32_t *accept, uint64_t ch, uint64_t cl, uint32_t strand, uint32_t f,
                                         const PrimeEdit &e, Allowed &&allowed, uint32_t *info, uint32_t *block)
{
    uint32_t e0, reach;
    uint64_t ih, il;
    if (!hdr_read(s, strand, f, e, &e0, &ih, &il, &reach)) return false;
    const uint32_t del = prime_del_len(e), ins = prime_ins_len(e);
    uint64_t sh, sl, have;
    const int32_t a = hdr_seen(s, ch, cl, e0, del, ins, ih, il, &sh, &sl, &have);
    const uint64_t differs = hdr_differs(s, ch, cl, sh, sl, have);
    uint32_t seed_mm, proto_mm;
    uint32_t flags = hdr_blocked(s, accept, differs, sh, sl, have, &seed_mm, &proto_mm);
    *block = kHdrNoBlock;
    if (!flags) {
        uint32_t sub;
        *block = hdr_substitute(s, accept, differs, sh, sl, have, a, e0, del, ins, seed_mm, allowed, &sub);
        flags = sub;
    }
    *info = reach | seed_mm << 8 | proto_mm << 13 | flags << 24;
    return true;
}

// ALLOWED against a CDS, for the base at global position x (the forward position f of a slot on the candidate's contig) of a
// candidate on `strand`, beside an edit at global position ge that deletes `del` bases: the read letters whose codon stays
// synonymous | kHdrCoding, or - x in no segment - every letter under SUB_NONCODING and none without it.  code: 64 amino-acid
// letters.  The segments are searched ONCE per candidate: *first (kCdsNone before the first call) is the first segment that ends
// behind g0, the context's first global position; every slot lies in [g0, g0 + C), so its segment is found from there by a walk
// over the few segments a context can hold.  (The segment travels as scalars, as in effects_row: a copy of the struct would live
// in scratch memory.)
__host__ __device__ VSC_FX_INLINE uint32_t hdr_allowed_cds(const EffPlanes &g, const CdsView &v, const uint8_t *code, bool noncoding, uint32_t x,
                                                           uint32_t strand, uint32_t ge, uint32_t del, uint32_t g0, uint32_t *first)
{
    const uint32_t outside = noncoding ? kHdrAnyLetter : 0u;
    if (!v.n) return outside;
    if (*first == kCdsNone) *first = cds_find(v, g0);
    uint32_t k = *first;
    while (k < v.n && v.seg[k].gend <= x) ++k;  // (x - g0 < 64 and no segment is empty: at most 64 steps)
    if (k >= v.n) return outside;
    const CdsSeg *q = v.seg + k;
    const uint32_t sg_start = q->gstart, sg_end = q->gend, sg_ci0 = q->ci0, sg_prev = q->prev, sg_next = q->next, sg_strand = q->strand;
    if (sg_start > x) return outside;
    const uint32_t ci = sg_ci0 + (sg_strand ? sg_end - 1u - x : x - sg_start), codon = ci / 3u, at = ci - 3u * codon;
    uint32_t p0, p1, p2;
    codon_of(v, sg_start, sg_end, sg_ci0, sg_prev, sg_next, sg_strand, codon, &p0, &p1, &p2);
    uint32_t ref = 0;
    bool ok = true;
    VSC_EFF_UNROLL
    for (uint32_t i = 0; i < 3u; ++i) {
        const uint32_t p = i == 0u ? p0 : i == 1u ? p1 : p2;
        if (p == kCdsNone || (ge <= p + 1u && p <= ge + del)) {  // UNKNOWN, or the codon touches the edit
            ok = false;
            continue;
        }
        const uint32_t b = effects_base(g, p);
        if (b > 3u) ok = false;
        ref = ref << 2 | ((sg_strand ? 3u - b : b) & 3u);
    }
    if (!ok) return kHdrCoding;
    uint32_t set = kHdrCoding;
    VSC_EFF_UNROLL
    for (uint32_t b = 0; b < 4u; ++b) {
        const uint32_t letter = strand == sg_strand ? b : 3u - b;  // the read letter in transcript orientation
        if (code[ref] == code[effect_alt(ref, 1u << at, letter)]) set |= 1u << b;
    }
    return set;
}

// The join of a defined candidate on `contig` whose context starts at global position g0 with the edits: emit(k, info, block)
// for every edit in reach, in ascending k; the result is their number.  allowed(r, ge, del): ALLOWED of reference context
// position r beside the edit at global position ge.  The bitmap (when there is one) is asked before any search; the lower bound
// is over the reach's first position, the walk ends behind its last.
template <class Allowed, class Emit>
__host__ __device__ VSC_FX_INLINE uint32_t hdr_walk(const HdrShape &s, const uint32_t *accept, const PrimeEdits &e, uint64_t ch, uint64_t cl,
                                             uint32_t contig, uint32_t g0, uint32_t strand, Allowed &&allowed, Emit &&emit)
{
    if (!e.n) return 0u;
    uint32_t lo, hi;
    hdr_reach(s, g0, strand, &lo, &hi);
    if (e.bitmap && !prime_cells_occupied(e.bitmap, lo, hi)) return 0u;
    uint32_t count = 0;
    for (uint32_t k = prime_first_edit(e, lo); k < e.n; ++k) {
        const uint32_t gp = e.gpos[k];
        if (gp > hi) break;
        const PrimeEdit rec = e.rec[k];
        if (rec.contig != contig) continue;
        uint32_t info, block;
        const uint32_t del = prime_del_len(rec);
        if (!hdr_pair(s, accept, ch, cl, strand, gp - g0, rec, [&](uint32_t r) { return allowed(r, gp, del); }, &info, &block)) continue;
        emit(k, info, block);
        ++count;
    }
    return count;
}

// the global position of reference context position r of a candidate on `strand` whose context starts at global position g0
__host__ __device__ inline uint32_t hdr_forward(const HdrShape &s, uint32_t g0, uint32_t strand, uint32_t r)
{
    return g0 + (strand ? hdr_context_len(s) - 1u - r : r);
}

// The FILTER rule: does a candidate of class cls with row (n_pairs, n_usable) pass?
__host__ __device__ inline bool hdr_keep(uint32_t cls, uint32_t n_pairs, uint32_t n_usable, bool have_edits, bool allow_open)
{
    if (cls != kEffDefined) return false;
    return !have_edits || n_usable >= 1u || (allow_open && n_pairs >= 1u);
}

}  // namespace vsc
