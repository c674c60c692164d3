// vsc_fold.h - the self-complementarity of a guide RNA (include/varscot_hip.h "SHAPE / SCAFFOLD / SPACER / PAIR /
// SELF STEM / SCAFFOLD STEM / QUAL / COVERED / ROW / FILTER") as what the host code (vsc_fold_text, the check of a call)
// shares with the kernels of vsc_fold.hip.  A header of its own, as vsc_mh.h is; the planes, the window and the reverse
// complement are vsc_efficiency.h's, called and not copied.
//
// fold_row below IS the row of one spacer: fold_rows_kernel and fold_filter_kernel call it for every candidate, vsc_fold_text
// calls it on the host, tools/fold_check.cpp against a brute-force walk on letters - one function, integers only, the same
// bits.  fold_context is the other half: the class of a locus and the planes of its spacer.  Plain inline functions that a
// stand-alone program can include without a device.
//
// The formulation.  A stem is a run on an anti-diagonal a + b = c of the pairing matrix.  For the spacer against itself
// M_c[a] = PAIR(g[a], g[c - a]) is the spacer compared with its own reversal shifted by n - 1 - c; PAIR is symmetric, so the
// bits a < floor((c + 1 - min_loop) / 2) are exactly the 5' arms whose loop is long enough.  For the spacer against the
// scaffold the reversed scaffold shifted by m - 1 - c takes the reversal's place, with no loop limit; that window is the same
// for every candidate of a launch, so the host lays the windows of all n + m - 1 diagonals out once (fold_scaffold_windows)
// and a diagonal costs one 16-byte read, no shift and no bounds test.  The spacer has at most 32 letters: every mask is one
// 32-bit word.  Both loops have the launch's trip count whatever the letters are.
#pragma once

#include <stdint.h>

#include "vsc_efficiency.h"

namespace vsc {

constexpr uint32_t kFoldMinProto = 12, kFoldMaxProto = 32;
constexpr uint32_t kFoldMinStem = 3, kFoldMaxStem = 8;
constexpr uint32_t kFoldMaxLoop = 16, kFoldMaxSeed = 16;
constexpr uint32_t kFoldMaxScaffold = 128;
constexpr uint32_t kFoldMaxDiagonals = kFoldMaxProto + kFoldMaxScaffold - 1;  // of spacer against scaffold
constexpr uint32_t kFoldWobble = 1u;                                          // flags bit 0
constexpr uint32_t kFoldUndefined = 0xFFFFFFFFu;  // both words of a candidate whose class is not defined
constexpr uint32_t kFoldNoLimit = 0xFFFFFFFFu, kFoldMaxLimit = 32;

struct FoldShape {
    uint32_t site_len, proto_start, proto_len;  // the spacer: site positions [proto_start, proto_start + proto_len), read orientation
    uint32_t stem, gc_min, min_loop;            // k; QUAL: at least gc_min G/C in the k-mer; unpaired letters between a self stem's arms
    uint32_t seed_start, seed_len;              // in spacer positions; seed_len 0: no seed
    uint32_t flags;                             // bit 0: G-U wobble pairs count
};

struct FoldLimits {
    uint32_t max_starts, max_self_longest, max_scaf_longest, max_seed_paired;  // each 0 .. 32, or kFoldNoLimit
};

// One diagonal c of spacer against scaffold, as fold_row reads it: bit a of h / l = the high / low bit of s[c - a], bit a of
// has = 0 <= c - a < m and a < n.
struct FoldWindow {
    uint32_t h, l, has, zero;
};

// The scaffold of a launch: win[c], c in [0, n_diag); n_diag = n + m - 1, or 0 for m == 0.
struct FoldScaffold {
    const FoldWindow *win;
    uint32_t n_diag;
};

// Is s a shape the definition allows?
__host__ __device__ inline bool fold_shape_valid(const FoldShape &s)
{
    if (s.site_len < kEffMinSite || s.site_len > kEffMaxSite) return false;
    if (s.proto_len < kFoldMinProto || s.proto_len > kFoldMaxProto || s.proto_start > s.site_len || s.proto_len > s.site_len - s.proto_start) return false;
    if (s.stem < kFoldMinStem || s.stem > kFoldMaxStem || s.gc_min > s.stem || s.min_loop > kFoldMaxLoop) return false;
    if (s.seed_start > kFoldMaxSeed || s.seed_len > kFoldMaxSeed || s.seed_start + s.seed_len > s.proto_len) return false;
    return (s.flags & ~kFoldWobble) == 0u;
}

__host__ __device__ inline bool fold_limit_valid(uint32_t v) { return v <= kFoldMaxLimit || v == kFoldNoLimit; }
__host__ __device__ inline bool fold_limits_valid(const FoldLimits &l)
{
    return fold_limit_valid(l.max_starts) && fold_limit_valid(l.max_self_longest) && fold_limit_valid(l.max_scaf_longest) &&
           fold_limit_valid(l.max_seed_paired);
}

__host__ __device__ inline uint32_t fold_low_bits(uint32_t n) { return n >= 32u ? ~0u : (1u << n) - 1u; }

// the letter of a scaffold or spacer text: A C G T = 0 .. 3, U as T, any case; 4: another letter
__host__ __device__ inline uint32_t fold_letter(char c)
{
    switch (c) {
    case 'A': case 'a': return 0u;
    case 'C': case 'c': return 1u;
    case 'G': case 'g': return 2u;
    case 'T': case 't': case 'U': case 'u': return 3u;
    default: return 4u;
    }
}

__host__ __device__ inline uint32_t fold_diagonals(uint32_t n, uint32_t m) { return m ? n + m - 1u : 0u; }

// The windows of scaffold letters s[0, m) (codes 0 .. 3) for a spacer of n letters into win[fold_diagonals(n, m)].  Host work,
// once per call.
inline void fold_scaffold_windows(const uint8_t *s, uint32_t m, uint32_t n, FoldWindow *win)
{
    const uint32_t n_diag = fold_diagonals(n, m);
    for (uint32_t c = 0; c < n_diag; ++c) {
        FoldWindow w{0u, 0u, 0u, 0u};
        for (uint32_t a = 0; a < n && a <= c; ++a) {
            const uint32_t j = c - a;
            if (j >= m) continue;
            w.h |= (uint32_t)(s[j] >> 1) << a;
            w.l |= (uint32_t)(s[j] & 1u) << a;
            w.has |= 1u << a;
        }
        win[c] = w;
    }
}

// bit a = PAIR(x[a], y[a]) of two letter planes: complementary letters differ in both bits; G (10) and T (11) share the high
// bit and differ in the low one.  wob is all ones under WOBBLE, else 0.
__host__ __device__ inline uint32_t fold_pairs(uint32_t xh, uint32_t xl, uint32_t yh, uint32_t yl, uint32_t wob)
{
    return (xl ^ yl) & ((xh ^ yh) | (xh & yh & wob));
}

// bit i = bits [i, i + k) of m are all set, k 3 .. 8: runs of 2, then of 3 or 4, then of k - three steps whatever k is, their
// shift counts the launch's (a shift by 0 changes nothing)
__host__ __device__ inline uint32_t fold_run_starts(uint32_t m, uint32_t k)
{
    m &= m >> 1;
    m &= m >> (k == 3u ? 1u : 2u);
    m &= m >> (k <= 4u ? 0u : k - 4u);
    return m;
}

// the union of [i, i + k) over the set bits i of m, k 3 .. 8; no set bit lies above 32 - k
__host__ __device__ inline uint32_t fold_spread(uint32_t m, uint32_t k)
{
    m |= m << 1;
    m |= m << (k == 3u ? 1u : 2u);
    m |= m << (k <= 4u ? 0u : k - 4u);
    return m;
}

// the longest run of set bits of m
__host__ __device__ inline uint32_t fold_longest_run(uint32_t m)
{
    uint32_t len = 0;
    for (; m; m &= m >> 1) ++len;
    return len;
}

__host__ __device__ inline uint32_t fold_reverse32(uint32_t x)
{
#if defined(__clang__)
    return __builtin_bitreverse32(x);
#else
    return (uint32_t)(eff_reverse64(x) >> 32);
#endif
}

struct FoldAcc {
    uint32_t starts, cover5, longest;
};

// one diagonal's mask m of paired positions (5' arms): its qualified k-run starts, their cover and its longest run into acc;
// returns the cover of this diagonal's qualified 5' arms
__host__ __device__ inline uint32_t fold_diagonal(uint32_t m, uint32_t qual, uint32_t k, FoldAcc &acc)
{
    const uint32_t q = fold_run_starts(m, k) & qual;
    const uint32_t cover = fold_spread(q, k);
    const uint32_t run = fold_longest_run(m);
    acc.starts |= q;
    acc.cover5 |= cover;
    acc.longest = run > acc.longest ? run : acc.longest;
    return cover;
}

// The row (w0, w1) of a spacer g[0, n), n = s.proto_len (planes gh, gl: bit a = the high / low bit of g[a]; the bits from n on
// are 0), against itself and the scaffold sc, under a valid shape s.
__host__ __device__ inline void fold_row(uint32_t gh, uint32_t gl, const FoldScaffold &sc, const FoldShape &s, uint32_t *w0, uint32_t *w1)
{
    const uint32_t n = s.proto_len, k = s.stem;
    const uint32_t wob = (s.flags & kFoldWobble) ? ~0u : 0u;
    const uint32_t all = fold_low_bits(n);
    // QUAL: bit i = the k-mer at i holds at least gc_min G/C (G = 10, C = 01), i in [0, n - k]
    const uint32_t gc = gh ^ gl, lowk = fold_low_bits(k);
    uint32_t qual = 0;
    for (uint32_t i = 0; i + k <= n; ++i) qual |= (uint32_t)((uint32_t)__builtin_popcount((gc >> i) & lowk) >= s.gc_min) << i;
    // the reversal: bit x = letter n - 1 - x
    const uint32_t rh = fold_reverse32(gh) >> (32u - n), rl = fold_reverse32(gl) >> (32u - n);
    FoldAcc self{0u, 0u, 0u};
    uint32_t cover_r = 0;  // the 3' arms' cover in the reversal's coordinates: bit x = position n - 1 - x
    // diagonal c: a pairs with c - a, which is bit a + (n - 1 - c) of the reversal; a in [max(0, c - n + 1), lim), where
    // lim = floor((c + 1 - min_loop) / 2) <= (c + 1) / 2 keeps a below its partner and the loop long enough
    for (uint32_t c = s.min_loop + 1u; c + 1u < 2u * n; ++c) {
        const uint32_t lim = (c + 1u - s.min_loop) >> 1;
        uint32_t m;
        if (c < n) {
            const uint32_t d = n - 1u - c;
            m = fold_pairs(gh, gl, rh >> d, rl >> d, wob) & fold_low_bits(lim);
            cover_r |= fold_diagonal(m, qual, k, self) << d;
        } else {
            const uint32_t e = c - (n - 1u);
            m = fold_pairs(gh, gl, rh << e, rl << e, wob) & fold_low_bits(lim) & ~fold_low_bits(e);
            cover_r |= fold_diagonal(m, qual, k, self) >> e;
        }
    }
    FoldAcc scaf{0u, 0u, 0u};
    for (uint32_t c = 0; c < sc.n_diag; ++c) {
        const FoldWindow w = sc.win[c];
        fold_diagonal(fold_pairs(gh, gl, w.h, w.l, wob) & w.has & all, qual, k, scaf);
    }
    const uint32_t cover3 = fold_reverse32(cover_r) >> (32u - n);
    const uint32_t covered = self.cover5 | cover3 | scaf.cover5;
    const uint32_t seed = fold_low_bits(s.seed_len) << s.seed_start;
    *w0 = (uint32_t)__builtin_popcount(self.starts | scaf.starts) | (uint32_t)__builtin_popcount(self.starts) << 8 |
          (uint32_t)__builtin_popcount(scaf.starts) << 16 | (uint32_t)__builtin_popcount(covered & seed) << 24;
    *w1 = self.longest | scaf.longest << 8;
}

// The FILTER rule: does a candidate of class cls with row (w0, w1) pass the limits?
__host__ __device__ inline bool fold_keep(uint32_t cls, uint32_t w0, uint32_t w1, const FoldLimits &l)
{
    if (cls != kEffDefined) return false;
    return (w0 & 0xFFu) <= l.max_starts && (w1 & 0xFFu) <= l.max_self_longest && ((w1 >> 8) & 0xFFu) <= l.max_scaf_longest &&
           (w0 >> 24) <= l.max_seed_paired;
}

// The class of locus (contig, pos, strand) under shape s - eff_context's, on the site with no flanks - and, for kEffDefined,
// the planes of its spacer.
__host__ __device__ inline uint32_t fold_context(const EffPlanes &g, const FoldShape &s, uint32_t contig, uint32_t pos, uint32_t strand, uint32_t *gh,
                                                 uint32_t *gl)
{
    const EffShape site{0u, s.site_len, 0u, 0u, 0u};
    uint64_t ch = 0, cl = 0;
    const uint32_t cls = eff_context(g, site, contig, pos, strand, &ch, &cl);
    const uint32_t all = fold_low_bits(s.proto_len);
    *gh = (uint32_t)(ch >> s.proto_start) & all;
    *gl = (uint32_t)(cl >> s.proto_start) & all;
    return cls;
}

}  // namespace vsc
