// vsc_prime.h - prime-editing guide design: the pegRNA extension of every (candidate, edit) pair (DESIGN 4.30,
// include/varscot_hip.h "SHAPE / CONTEXT / PBS / EDITS / READ / RTT / FLAGS / ROW / PAIR / COVERAGE / FILTER / EXTENSION") as
// what the host code (vsc_prime_site_text) shares with the kernels of vsc_prime.hip.  A header of its own, as vsc_edit.h is;
// the planes, the window and the reverse complement are vsc_efficiency.h's.
//
// prime_pbs IS the primer binding site of one context, prime_read / prime_edited / prime_rtt / prime_flags / prime_pair ARE
// the pair of one context with one edit, prime_walk IS the join with the edits: prime_rows_kernel, prime_pairs_kernel and
// prime_filter_kernel call them for every candidate, vsc_prime_site_text and the stand-alone check call them on the host - one
// function each, integers only, the same bits.  Plain inline functions that a stand-alone program can include without a device.
#pragma once

#include <stdint.h>

#include "vsc_efficiency.h"

namespace vsc {

constexpr uint32_t kPrimeUndefined = 0xFFFFFFFFu;  // both words of the row of a candidate whose class is not defined
constexpr uint32_t kPrimeMaxCount = 0xFFFFFFFEu;   // candidates, edits and pairs of one call
constexpr uint32_t kPrimeMaxIndel = 16;            // del_len and ins_len
constexpr uint32_t kPrimeMaxRange = 8;             // pam_len and seed_len
constexpr int32_t kPrimeMaxWeight = 1 << 20;       // |every stability weight|
constexpr uint32_t kPrimeAvoidGEnd = 1u;           // shape flag bit 0
enum PrimeFlag : uint32_t { kPrimePam = 1u, kPrimeSeed = 2u, kPrimePolyT = 4u, kPrimeWeak = 8u };
constexpr uint32_t kPrimeFlags = 4;
// the occupancy bitmap in front of the lower bound: one bit per cell of 2^kPrimeCellShift global positions that hold an edit's
// position.  8: 2^32 positions are 2 MiB, a 3.1 Gbp genome 1.5 MiB - it stays in an XCD's 4 MiB L2 beside the streams, and a
// reach of at most 65 positions touches at most two cells.
constexpr uint32_t kPrimeCellShift = 8;

struct PrimeShape {
    uint32_t site_len, down, nick;
    uint32_t pbs_min, pbs_max, rtt_min, rtt_max, min_homology;
    uint32_t pam_start, pam_len, seed_start, seed_len;
    uint32_t flags;
    int32_t init, mono[4], di[16], target;  // STABILITY
};

__host__ __device__ inline uint32_t prime_context_len(const PrimeShape &s) { return s.site_len + s.down; }

// Is s a shape the definition allows?
__host__ __device__ inline bool prime_shape_valid(const PrimeShape &s)
{
    if (s.site_len < kEffMinSite || s.site_len > kEffMaxSite || s.down > kEffMaxContext - s.site_len) return false;
    const uint32_t C = prime_context_len(s);
    if (s.nick < 1u || s.nick > s.site_len) return false;
    if (s.pbs_min < 1u || s.pbs_min > s.pbs_max || s.pbs_max > s.nick) return false;
    if (s.rtt_min < 1u || s.rtt_min > s.rtt_max || s.rtt_max > C - s.nick) return false;
    if (s.pbs_max + s.rtt_max > kEffMaxContext || s.min_homology > s.rtt_max) return false;
    if (s.pam_len > kPrimeMaxRange || s.pam_start > s.site_len || s.pam_len > s.site_len - s.pam_start) return false;
    if (s.seed_len > kPrimeMaxRange || s.seed_start > s.site_len || s.seed_len > s.site_len - s.seed_start) return false;
    if (s.flags & ~kPrimeAvoidGEnd) return false;
    bool ok = s.init >= -kPrimeMaxWeight && s.init <= kPrimeMaxWeight && s.target >= -kPrimeMaxWeight && s.target <= kPrimeMaxWeight;
    for (uint32_t k = 0; k < 4u; ++k) ok = ok && s.mono[k] >= -kPrimeMaxWeight && s.mono[k] <= kPrimeMaxWeight;
    for (uint32_t k = 0; k < 16u; ++k) ok = ok && s.di[k] >= -kPrimeMaxWeight && s.di[k] <= kPrimeMaxWeight;
    return ok;
}

// CONTEXT: the class of locus (contig, pos, strand), tested in the order of EffClass, and - for kEffDefined - the planes of
// its C bases in read orientation: eff_context with no flank in front of the site and `down` bases behind it.  (The shape does
// not go through eff_shape_valid: its 16-base flank limit is the efficiency models', eff_window serves any C up to 64.)
__host__ __device__ inline uint32_t prime_context(const EffPlanes &g, const PrimeShape &s, uint32_t contig, uint32_t pos, uint32_t strand,
                                                  uint64_t *ch, uint64_t *cl)
{
    const EffShape c{0u, s.site_len, s.down, 0u, 0u};
    return eff_context(g, c, contig, pos, strand, ch, cl);
}

// F0 of a defined candidate: the context's first forward position on its contig
__host__ __device__ inline uint32_t prime_first_forward(uint32_t pos, uint32_t strand, const PrimeShape &s) { return strand ? pos - s.down : pos; }

__host__ __device__ inline uint64_t prime_shl(uint64_t x, uint32_t n) { return n >= 64u ? 0ull : x << n; }
__host__ __device__ inline uint64_t prime_shr(uint64_t x, uint32_t n) { return n >= 64u ? 0ull : x >> n; }
// the bits [lo, hi) of a plane, hi <= 64
__host__ __device__ inline uint64_t prime_range(uint32_t lo, uint32_t hi) { return eff_low_bits(hi) & ~eff_low_bits(lo); }

// PBS: the row word pbs_len | pbs_gc << 8 | WEAK << 16 of a context.  S(L) grows by one mononucleotide and (from L = 2 on) one
// dinucleotide term per step towards the context's start; every candidate takes pbs_max steps.  mono / di: s.mono / s.di, or a
// copy of them where a lane may index it (the kernels keep one in LDS).
__host__ __device__ inline uint32_t prime_pbs(uint64_t ch, uint64_t cl, const PrimeShape &s, const int32_t *mono, const int32_t *di)
{
    int32_t sum = s.init;
    uint32_t len = 0, next = 0;  // next: the letter at nick - L + 1
    for (uint32_t L = 1; L <= s.pbs_max; ++L) {
        const uint32_t j = s.nick - L, b = (uint32_t)(ch >> j & 1u) << 1 | (uint32_t)(cl >> j & 1u);
        sum += mono[b];
        if (L >= 2u) sum += di[4u * b + next];
        next = b;
        if (!len && L >= s.pbs_min && sum >= s.target) len = L;
    }
    const uint32_t weak = len ? 0u : 1u;
    if (!len) len = s.pbs_max;
    const uint32_t gc = (uint32_t)__builtin_popcountll((ch ^ cl) & prime_range(s.nick - len, s.nick));
    return len | gc << 8 | weak << 16;
}

// EDITS as the kernels hold them: the global positions (contig offset + pos, 32-bit as contig_off is; ascending, two edits of
// neighbouring contigs may share one when the first is an insertion at its contig's end), the entries themselves
// { contig, pos, del_len | ins_len << 16, ins }, and the occupancy bitmap over the positions (null: none is asked).
struct PrimeEdit {
    uint32_t contig, pos, lens, ins;
};
struct PrimeEdits {
    const uint32_t *gpos;
    const PrimeEdit *rec;
    const uint32_t *bitmap;
    uint32_t n;
};
__host__ __device__ inline uint32_t prime_del_len(const PrimeEdit &e) { return e.lens & 0xFFFFu; }
__host__ __device__ inline uint32_t prime_ins_len(const PrimeEdit &e) { return e.lens >> 16; }

// Is e an entry EDITS allows on a contig of `len` bases?
__host__ __device__ inline bool prime_edit_valid(const PrimeEdit &e, uint32_t len)
{
    const uint32_t del = prime_del_len(e), ins = prime_ins_len(e);
    if (del > kPrimeMaxIndel || ins > kPrimeMaxIndel || del + ins < 1u) return false;
    if (ins < 16u && (e.ins >> (2u * ins)) != 0u) return false;
    return e.pos <= len && del <= len - e.pos;
}

// the forward global positions an edit IN REACH of a candidate can start at: [*lo, *hi], g0 = the context's first global position.
// e0 >= nick is pos - F0 >= nick on '+' and pos - F0 + del_len <= C - nick on '-'.
__host__ __device__ inline void prime_reach(const PrimeShape &s, uint32_t g0, uint32_t strand, uint32_t *lo, uint32_t *hi)
{
    const uint32_t C = prime_context_len(s);
    *lo = strand ? g0 : g0 + s.nick;
    *hi = strand ? g0 + C - s.nick : g0 + C;
}

// does any cell that [lo, hi] touches hold an edit?  (hi - lo <= 64: at most two cells)
__host__ __device__ inline bool prime_cells_occupied(const uint32_t *bitmap, uint32_t lo, uint32_t hi)
{
    const uint32_t c0 = lo >> kPrimeCellShift, c1 = hi >> kPrimeCellShift;
    const uint32_t b0 = bitmap[c0 >> 5] >> (c0 & 31u) & 1u;
    if (c1 == c0) return b0 != 0u;
    return (b0 | (bitmap[c1 >> 5] >> (c1 & 31u) & 1u)) != 0u;
}

// the first edit at or behind global position g (e.n: none): a lower bound, log2(n) dependent loads
__host__ __device__ inline uint32_t prime_first_edit(const PrimeEdits &e, uint32_t g)
{
    uint32_t lo = 0, hi = e.n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (e.gpos[mid] < g) lo = mid + 1u;
        else hi = mid;
    }
    return lo;
}

// bit k of the result = bit 2 k of x (the inverse of eff_spread32 over 16 letters)
__host__ __device__ inline uint32_t prime_gather16(uint32_t x)
{
    x &= 0x55555555u;
    x = (x | x >> 1) & 0x33333333u;
    x = (x | x >> 2) & 0x0F0F0F0Fu;
    x = (x | x >> 4) & 0x00FF00FFu;
    x = (x | x >> 8) & 0x0000FFFFu;
    return x;
}

// READ: is the edit (f = its global position - g0, f >= 0, on the candidate's contig) in reach of the candidate?  Then *e0 is
// where it starts in read orientation and (*ih, *il) are the planes of I, the inserted letters as the read strand has them.
__host__ __device__ inline bool prime_read(const PrimeShape &s, uint32_t strand, uint32_t f, const PrimeEdit &e, uint32_t *e0, uint64_t *ih,
                                           uint64_t *il)
{
    const uint32_t C = prime_context_len(s), del = prime_del_len(e), ins = prime_ins_len(e);
    if (f > C || del > C - f) return false;  // [pos, pos + del_len) inside [F0, F0 + C); del_len 0: F0 <= pos <= F0 + C
    const uint32_t at = strand ? C - f - del : f;
    if (at < s.nick) return false;
    *e0 = at;
    uint64_t h = prime_gather16(e.ins >> 1), l = prime_gather16(e.ins);
    if (strand && ins) {
        h = eff_revcomp(h, ins);
        l = eff_revcomp(l, ins);
    }
    *ih = h;
    *il = l;
    return true;
}

// E = R[0, e0) + I + R[e0 + del_len, C): its first 64 letters as planes (nothing behind position 63 is ever asked: nick +
// rtt_max <= C <= 64) and its length, by mask, shift and or.  The bits from |E| on are 0.
__host__ __device__ inline uint32_t prime_edited(const PrimeShape &s, uint64_t ch, uint64_t cl, uint32_t e0, uint32_t del, uint32_t ins,
                                                 uint64_t ih, uint64_t il, uint64_t *eh, uint64_t *el)
{
    const uint64_t head = eff_low_bits(e0);
    *eh = (ch & head) | prime_shl(ih, e0) | prime_shl(prime_shr(ch, e0 + del), e0 + ins);
    *el = (cl & head) | prime_shl(il, e0) | prime_shl(prime_shr(cl, e0 + del), e0 + ins);
    return prime_context_len(s) - del + ins;
}

// RTT: the template's length t of a pair with d = e0 - nick, 0 when the pair does not exist
__host__ __device__ inline uint32_t prime_rtt(const PrimeShape &s, uint64_t eh, uint64_t el, uint32_t e_len, uint32_t d, uint32_t ins)
{
    const uint32_t need = d + ins + s.min_homology;
    uint32_t t = s.rtt_min > need ? s.rtt_min : need;
    if (t > s.rtt_max) return 0u;
    if (s.flags & kPrimeAvoidGEnd) {
        // the first letter at or behind nick + t - 1 (<= 63) that is not G (10); the bits behind |E| are 0: not G
        const uint64_t not_g = ~(eh & ~el) >> (s.nick + t - 1u);
        if (!not_g) return 0u;
        t += (uint32_t)__builtin_ctzll(not_g);
        if (t > s.rtt_max) return 0u;
    }
    return s.nick + t <= e_len ? t : 0u;
}

// does E differ from R anywhere in read positions [start, start + len)?  A position behind E counts as different.
__host__ __device__ inline bool prime_changed(uint64_t ch, uint64_t cl, uint64_t eh, uint64_t el, uint32_t e_len, uint32_t start, uint32_t len)
{
    if (!len) return false;
    if (start + len > e_len) return true;
    return (((ch ^ eh) | (cl ^ el)) & prime_range(start, start + len)) != 0ull;
}

// FLAGS of a pair that exists (pbs = the candidate's row word)
__host__ __device__ inline uint32_t prime_flags(const PrimeShape &s, uint64_t ch, uint64_t cl, uint64_t eh, uint64_t el, uint32_t e_len,
                                                uint32_t pbs, uint32_t t)
{
    uint32_t f = 0;
    if (prime_changed(ch, cl, eh, el, e_len, s.pam_start, s.pam_len)) f |= kPrimePam;
    if (prime_changed(ch, cl, eh, el, e_len, s.seed_start, s.seed_len)) f |= kPrimeSeed;
    const uint64_t a = ~eh & ~el & prime_range(s.nick - (pbs & 0xFFu), s.nick + t);  // A (00) inside the extension's range
    if (a & a >> 1 & a >> 2 & a >> 3) f |= kPrimePolyT;
    if (pbs >> 16 & 1u) f |= kPrimeWeak;
    return f;
}

// PAIR of a defined candidate (planes ch, cl, strand, row word pbs) with an edit at f = its global position - g0 on the
// candidate's contig: does it exist?  Then *info = t | d << 8 | h << 16 | flags << 24 and *ext = (pbs_len + t) | ext_gc << 8 |
// pbs_len << 16; (*eh, *el) = the planes of E.
__host__ __device__ inline bool prime_pair(const PrimeShape &s, uint64_t ch, uint64_t cl, uint32_t strand, uint32_t pbs, uint32_t f,
                                           const PrimeEdit &e, uint32_t *info, uint32_t *ext, uint64_t *eh, uint64_t *el)
{
    uint32_t e0;
    uint64_t ih, il;
    if (!prime_read(s, strand, f, e, &e0, &ih, &il)) return false;
    const uint32_t del = prime_del_len(e), ins = prime_ins_len(e), d = e0 - s.nick;
    const uint32_t e_len = prime_edited(s, ch, cl, e0, del, ins, ih, il, eh, el);
    const uint32_t t = prime_rtt(s, *eh, *el, e_len, d, ins);
    if (!t) return false;
    const uint32_t pbs_len = pbs & 0xFFu;
    const uint32_t gc = (uint32_t)__builtin_popcountll((*eh ^ *el) & prime_range(s.nick - pbs_len, s.nick + t));
    *info = t | d << 8 | (t - d - ins) << 16 | prime_flags(s, ch, cl, *eh, *el, e_len, pbs, t) << 24;
    *ext = (pbs_len + t) | gc << 8 | pbs_len << 16;
    return true;
}

// The join of a defined candidate on `contig` whose context starts at global position g0 with the edits: emit(k, info, ext, eh,
// el) for every pair that exists, in ascending k; the result is their number.  The bitmap (when there is one) is asked before
// any search; the lower bound is over the reach's first position, the walk ends behind its last: at most C - nick + 1 entries
// are in reach (and at most that many plus the ties of neighbouring contigs are visited).
template <class Emit>
__host__ __device__ inline uint32_t prime_walk(const PrimeShape &s, const PrimeEdits &e, uint64_t ch, uint64_t cl, uint32_t contig, uint32_t g0,
                                               uint32_t strand, uint32_t pbs, Emit &&emit)
{
    if (!e.n) return 0u;
    uint32_t lo, hi;
    prime_reach(s, g0, strand, &lo, &hi);
    if (e.bitmap && !prime_cells_occupied(e.bitmap, lo, hi)) return 0u;
    uint32_t count = 0;
    for (uint32_t k = prime_first_edit(e, lo); k < e.n; ++k) {
        const uint32_t gp = e.gpos[k];
        if (gp > hi) break;
        const PrimeEdit rec = e.rec[k];
        if (rec.contig != contig) continue;
        uint32_t info, ext;
        uint64_t eh, el;
        if (!prime_pair(s, ch, cl, strand, pbs, gp - g0, rec, &info, &ext, &eh, &el)) continue;
        emit(k, info, ext, eh, el);
        ++count;
    }
    return count;
}

// The FILTER rule: does a candidate of class cls with row (pbs, n_pairs) pass?
__host__ __device__ inline bool prime_keep(uint32_t cls, uint32_t pbs, uint32_t n_pairs, bool have_edits, bool allow_weak)
{
    if (cls != kEffDefined) return false;
    return (!have_edits || n_pairs >= 1u) && (allow_weak || !(pbs >> 16 & 1u));
}

}  // namespace vsc
