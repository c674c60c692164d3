// vsc_motif.h - restriction sites and IUPAC motifs in candidate guides (include/varscot_hip.h "SHAPE / FLANKS /
// MOTIFS / GENOMIC / CONSTRUCT / OCC / Z / ROW / TOTALS / FILTER") as what the host code (vsc_motif_text, the check of a call)
// shares with the kernels of vsc_motif.hip.  A header of its own, as vsc_fold.h is; the planes, the context and the reverse
// complement are vsc_efficiency.h's, called and not copied.
//
// motif_row below IS the row of one context: motif_rows_kernel and motif_filter_kernel call it for every candidate,
// vsc_motif_text calls it on the host, tools/motif_check.cpp against a walk on letters - one function, integers only, the same
// bits.  motif_context is the other half: the class of a locus and the planes of its context.  Plain inline functions that a
// stand-alone program can include without a device.
//
// The formulation.  A text of at most 64 letters is two planes (bit j = the high / low bit of letter j).  A pattern of L letters
// is L accept sets of 4 bits, one nibble each in one 64-bit word.  E_k = the positions whose letter lies in set k is the OR
// of the text's four letter masks that the set selects, by launch-wide masks; the starts of the pattern's occurrences are
// valid & E_0 & (E_1 >> 1) & ... & (E_(L-1) >> (L-1)) - shift-and, with the launch's trip count and the launch's shift counts
// whatever the letters are.  What depends on the launch alone is made on the host once per call (motif_layout): every pattern
// of every motif (the reverse complement as a pattern of its own, a palindrome's dropped), its valid starts in the genomic
// text and in the construct, the starts whose occurrence overlaps the cut zone, and the planes of the flanks.
#pragma once

#include <stdint.h>

#include "vsc_efficiency.h"

namespace vsc {

constexpr uint32_t kMotifMinProto = 12, kMotifMaxProto = 32;
constexpr uint32_t kMotifMaxCut = 16, kMotifMaxFlank = 16;
constexpr uint32_t kMotifMinLen = 2, kMotifMaxLen = 16;
constexpr uint32_t kMotifMaxMotifs = 63, kMotifMaxPatterns = 2 * kMotifMaxMotifs;
constexpr uint32_t kMotifBothStrands = 1u;  // a motif's flags bit 0
constexpr uint32_t kMotifCutOnly = 1u;      // the limits' flags bit 0
constexpr uint64_t kMotifUndefined = ~0ull;  // all three words of a candidate whose class is not defined
constexpr uint32_t kMotifStats = kEffClasses + 3;  // the classes, then the candidates with a construct, a cut, a cut-only bit

struct MotifShape {
    uint32_t up, site_len, down;      // the genomic context, as EffShape's: C = up + site_len + down
    uint32_t proto_start, proto_len;  // the spacer in site positions, read orientation
    uint32_t cut_start, cut_len;      // the cut zone in site positions
};

struct MotifLimits {
    uint64_t forbid_construct, forbid_context, require_cut;
    uint32_t flags;  // bit 0: CUT_ONLY
};

// One pattern as motif_row reads it.  48 bytes: three 16-byte reads.
struct MotifPattern {
    uint64_t accept;    // nibble k = the accept set of letter k: bit 0 A, 1 C, 2 G, 3 T
    uint64_t valid_x;   // the starts q with q + len <= C
    uint64_t valid_y;   // the starts q with q + len <= a + n + b
    uint64_t zone;      // the starts of valid_x whose occurrence overlaps Z
    uint32_t len, bit;  // its motif's bit m
    uint32_t zero[2];
};

// What a launch reads beside the genome and the loci: the patterns, then the flanks' planes in construct positions (left at
// [0, a), right at [a + n, a + n + b)) and the left flank's length.
struct MotifTable {
    const MotifPattern *pat;
    uint32_t n_pat, n_motifs;
    uint64_t flank_h, flank_l;
    uint32_t a, b;
};

struct MotifRow {
    uint64_t construct, cut, elsewhere;
};

__host__ __device__ inline uint32_t motif_context_len(const MotifShape &s) { return s.up + s.site_len + s.down; }

// Is s a shape the definition allows?
__host__ __device__ inline bool motif_shape_valid(const MotifShape &s)
{
    if (s.up > kEffMaxFlank || s.down > kEffMaxFlank || s.site_len < kEffMinSite || s.site_len > kEffMaxSite) return false;
    if (motif_context_len(s) > kEffMaxContext) return false;
    if (s.proto_len < kMotifMinProto || s.proto_len > kMotifMaxProto || s.proto_start > s.site_len || s.proto_len > s.site_len - s.proto_start)
        return false;
    return s.cut_len >= 1u && s.cut_len <= kMotifMaxCut && s.cut_start <= s.site_len && s.cut_len <= s.site_len - s.cut_start;
}

__host__ __device__ inline bool motif_limits_valid(const MotifLimits &l, uint32_t n_motifs)
{
    const uint64_t known = eff_low_bits(n_motifs);
    return !((l.forbid_construct | l.forbid_context | l.require_cut) & ~known) && !(l.flags & ~kMotifCutOnly);
}

// the letter of a flank or context text: A C G T = 0 .. 3, U as T, any case; 4: another letter
__host__ __device__ inline uint32_t motif_letter(char c)
{
    switch (c) {
    case 'A': case 'a': return 0u;
    case 'C': case 'c': return 1u;
    case 'G': case 'g': return 2u;
    case 'T': case 't': case 'U': case 'u': return 3u;
    default: return 4u;
    }
}

// the accept set of an IUPAC letter (bit 0 A, 1 C, 2 G, 3 T), any case, U as T; 0: no IUPAC letter
inline uint32_t motif_iupac(char c)
{
    switch (c >= 'a' && c <= 'z' ? c - 'a' + 'A' : c) {
    case 'A': return 1u;
    case 'C': return 2u;
    case 'G': return 4u;
    case 'T': case 'U': return 8u;
    case 'R': return 5u;    // A G
    case 'Y': return 10u;   // C T
    case 'S': return 6u;    // C G
    case 'W': return 9u;    // A T
    case 'K': return 12u;   // G T
    case 'M': return 3u;    // A C
    case 'B': return 14u;   // not A
    case 'D': return 13u;   // not C
    case 'H': return 11u;   // not G
    case 'V': return 7u;    // not T
    case 'N': return 15u;
    default: return 0u;
    }
}

// the complement of an accept set: A <-> T, C <-> G, which is the nibble's bit order reversed
inline uint32_t motif_complement(uint32_t set) { return (set & 1u) << 3 | (set & 2u) << 1 | (set & 4u) >> 1 | (set & 8u) >> 3; }

// A motif's accept sets out of its text: false for len outside 2 .. 16, a letter that is no IUPAC letter, or every letter N.
inline bool motif_accepts(const char *text, uint32_t len, uint64_t *accept)
{
    if (len < kMotifMinLen || len > kMotifMaxLen) return false;
    uint64_t acc = 0;
    bool all_n = true;
    for (uint32_t k = 0; k < len; ++k) {
        const uint32_t set = motif_iupac(text[k]);
        if (!set) return false;
        all_n = all_n && set == 15u;
        acc |= (uint64_t)set << (4u * k);
    }
    *accept = acc;
    return !all_n;
}

inline uint64_t motif_revcomp(uint64_t accept, uint32_t len)
{
    uint64_t rc = 0;
    for (uint32_t k = 0; k < len; ++k) rc |= (uint64_t)motif_complement((uint32_t)(accept >> (4u * (len - 1u - k))) & 15u) << (4u * k);
    return rc;
}

// the starts q in [0, text_len - len], none when the pattern is longer than the text
inline uint64_t motif_valid_starts(uint32_t text_len, uint32_t len) { return len > text_len ? 0ull : eff_low_bits(text_len - len + 1u); }

// One pattern of motif `bit` under shape s and flanks of a and b letters.
inline MotifPattern motif_pattern(uint64_t accept, uint32_t len, uint32_t bit, const MotifShape &s, uint32_t a, uint32_t b)
{
    MotifPattern p{};
    p.accept = accept;
    p.len = len;
    p.bit = bit;
    p.valid_x = motif_valid_starts(motif_context_len(s), len);
    p.valid_y = motif_valid_starts(a + s.proto_len + b, len);
    // q < z1 and q + len > z0
    const uint32_t z0 = s.up + s.cut_start, z1 = z0 + s.cut_len;
    const uint32_t from = z0 + 1u > len ? z0 + 1u - len : 0u;
    p.zone = p.valid_x & eff_low_bits(z1) & ~eff_low_bits(from);
    return p;
}

// The patterns of motifs whose accept sets, lengths and flags are given, into pat[kMotifMaxPatterns]; returns their number.
inline uint32_t motif_layout(const uint64_t *accept, const uint32_t *len, const uint32_t *flags, uint32_t n_motifs, const MotifShape &s, uint32_t a,
                             uint32_t b, MotifPattern *pat)
{
    uint32_t n = 0;
    for (uint32_t m = 0; m < n_motifs; ++m) {
        pat[n++] = motif_pattern(accept[m], len[m], m, s, a, b);
        const uint64_t rc = motif_revcomp(accept[m], len[m]);
        if ((flags[m] & kMotifBothStrands) && rc != accept[m]) pat[n++] = motif_pattern(rc, len[m], m, s, a, b);
    }
    return n;
}

// The flanks' planes in construct positions out of their letters (0 .. 3): left at [0, a), right at [a + n, a + n + b).
inline void motif_flank_planes(const uint8_t *left, uint32_t a, const uint8_t *right, uint32_t b, uint32_t n, uint64_t *fh, uint64_t *fl)
{
    uint64_t h = 0, l = 0;
    for (uint32_t j = 0; j < a; ++j) {
        h |= (uint64_t)(left[j] >> 1) << j;
        l |= (uint64_t)(left[j] & 1u) << j;
    }
    for (uint32_t j = 0; j < b; ++j) {
        h |= (uint64_t)(right[j] >> 1) << (a + n + j);
        l |= (uint64_t)(right[j] & 1u) << (a + n + j);
    }
    *fh = h;
    *fl = l;
}

// The four letter masks of a text of `len` letters (planes h, l): bit j of is[b] = letter j is b.
struct MotifLetters {
    uint64_t is[4];
};
__host__ __device__ inline MotifLetters motif_letters(uint64_t h, uint64_t l, uint32_t len)
{
    const uint64_t all = eff_low_bits(len);
    return MotifLetters{{~h & ~l & all, ~h & l, h & ~l, h & l}};
}

// bit j = the letter at j lies in the accept set `set`: the OR of the letter masks the set selects.  The four selecting masks
// are the launch's (all ones or zero): an AND and three AND-ORs per word.
__host__ __device__ inline uint64_t motif_accepted(const MotifLetters &t, uint32_t set)
{
    const uint64_t a = 0ull - (uint64_t)(set & 1u), c = 0ull - (uint64_t)((set >> 1) & 1u);
    const uint64_t g = 0ull - (uint64_t)((set >> 2) & 1u), u = 0ull - (uint64_t)((set >> 3) & 1u);
    return (t.is[3] & u) | ((t.is[2] & g) | ((t.is[1] & c) | (t.is[0] & a)));
}

// A value that is the same on every lane of a wave - a pattern's field, read from LDS at a wave-wide address - as a scalar:
// the accept sets, their masks and the loop's count then cost no vector instruction.  The host has nothing to do.
__host__ __device__ inline uint32_t motif_uniform(uint32_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
#else
    return v;
#endif
}
__host__ __device__ inline uint64_t motif_uniform(uint64_t v)
{
    return (uint64_t)motif_uniform((uint32_t)(v >> 32)) << 32 | motif_uniform((uint32_t)v);
}

// The row of a context in read orientation (planes ch, cl: the bits from C on are 0) under a valid shape s and the table t.
__host__ __device__ inline MotifRow motif_row(uint64_t ch, uint64_t cl, const MotifShape &s, const MotifTable &t)
{
    // CONSTRUCT: the spacer's letters between the flanks
    const uint32_t at = s.up + s.proto_start;
    const uint64_t sp = eff_low_bits(s.proto_len);
    const uint64_t yh = (((ch >> at) & sp) << t.a) | t.flank_h, yl = (((cl >> at) & sp) << t.a) | t.flank_l;
    const MotifLetters x = motif_letters(ch, cl, motif_context_len(s)), y = motif_letters(yh, yl, t.a + s.proto_len + t.b);
    MotifRow r{0ull, 0ull, 0ull};
    for (uint32_t i = 0; i < t.n_pat; ++i) {
        const MotifPattern &p = t.pat[i];
        const uint64_t accept = motif_uniform(p.accept), zone = motif_uniform(p.zone);
        const uint32_t len = motif_uniform(p.len);
        // both texts in one walk over the pattern's letters
        uint64_t mx = motif_uniform(p.valid_x), my = motif_uniform(p.valid_y);
        for (uint32_t k = 0; k < len; ++k) {
            const uint32_t set = (uint32_t)(accept >> (4u * k)) & 15u;
            mx &= motif_accepted(x, set) >> k;
            my &= motif_accepted(y, set) >> k;
        }
        const uint64_t bit = 1ull << motif_uniform(p.bit);
        r.construct |= my ? bit : 0ull;
        r.cut |= (mx & zone) ? bit : 0ull;
        r.elsewhere |= (mx & ~zone) ? bit : 0ull;
    }
    return r;
}

// The FILTER rule: does a candidate of class cls with row r pass the limits?
__host__ __device__ inline bool motif_keep(uint32_t cls, const MotifRow &r, const MotifLimits &l)
{
    if (cls != kEffDefined) return false;
    const uint64_t x = (l.flags & kMotifCutOnly) ? r.cut & ~r.elsewhere : r.cut;
    return !(r.construct & l.forbid_construct) && !((r.cut | r.elsewhere) & l.forbid_context) && (l.require_cut == 0ull || (x & l.require_cut));
}

// The class of locus (contig, pos, strand) under shape s - eff_context's, with the shape's flanks - and, for kEffDefined, the
// planes of its context.
__host__ __device__ inline uint32_t motif_context(const EffPlanes &g, const MotifShape &s, uint32_t contig, uint32_t pos, uint32_t strand, uint64_t *ch,
                                                  uint64_t *cl)
{
    const EffShape ctx{s.up, s.site_len, s.down, 0u, 0u};
    return eff_context(g, ctx, contig, pos, strand, ch, cl);
}

}  // namespace vsc
