// vsc_efficiency.h - the on-target efficiency score (include/varscot_hip.h "SHAPE / CONTEXT / MODEL / LINEAR
// PREDICTOR / UNDEFINED") as what the host code (vsc_eff_model_build, vsc_eff_score_text) shares with the kernels of
// vsc_efficiency.hip.  A header of its own, as vsc_table.h is.
//
// eff_linear below IS the linear predictor of include/varscot_hip.h for one context in read orientation: eff_score_kernel and
// eff_filter_kernel call it for every candidate (the weights in LDS), vsc_eff_score_text calls it on the host - one function,
// one order of the additions, the same bits.  eff_context is the other half: the class of a locus and the planes of its
// context out of a genome's plane words - the kernels call it on the resident planes, a stand-alone program on host arrays.
// Plain inline functions that a stand-alone program can include without a device.
#pragma once

#include <stdint.h>

#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif
#if defined(__clang__)
#define VSC_EFF_UNROLL _Pragma("unroll")
#else
#define VSC_EFF_UNROLL
#endif

namespace vsc {

constexpr uint32_t kEffMaxContext = 64;  // C = up + site_len + down
constexpr uint32_t kEffMaxFlank = 16;
constexpr uint32_t kEffMinSite = 16, kEffMaxSite = 32;
// the weights as the functions below read them, one array: mono[C][4], then the dinucleotide weights TRANSPOSED -
// dit[j][b_j + 4 b_{j+1}] = di[j][4 b_j + b_{j+1}], the four bits as they lie in the 2-bit code of the context - then
// gc[gc_len + 1]: at most 256 + 1 008 + 65 doubles, 10 632 bytes
constexpr uint32_t kEffMaxWeights = 4 * kEffMaxContext + 16 * (kEffMaxContext - 1) + kEffMaxContext + 1;
constexpr uint64_t kEffUndefinedBits = 0x7FF8000000000000ull;  // the one NaN an undefined predictor is

// the classes of a candidate, in the order they are tested; the index into vsc_eff_stats' counts
enum EffClass : uint32_t { kEffDefined = 0, kEffInvalid, kEffOffContig, kEffNotResident, kEffHasN, kEffClasses };

struct EffShape {
    uint32_t up, site_len, down;  // C = up + site_len + down
    uint32_t gc_start, gc_len;    // [gc_start, gc_start + gc_len) in context coordinates; gc_len 0: no G/C term
};

__host__ __device__ inline uint32_t eff_context_len(const EffShape &s) { return s.up + s.site_len + s.down; }
__host__ __device__ inline uint32_t eff_di_at(uint32_t C) { return 4u * C; }
__host__ __device__ inline uint32_t eff_gc_at(uint32_t C) { return 4u * C + 16u * (C - 1u); }
__host__ __device__ inline uint32_t eff_n_weights(const EffShape &s)
{
    return eff_gc_at(eff_context_len(s)) + (s.gc_len ? s.gc_len + 1u : 0u);
}

// Is s a shape the definition allows?  site_len 16 .. 32 (23: the candidates of vsc_guides_enumerate), flanks <= 16, C <= 64,
// the G/C range inside the context.
inline bool eff_shape_valid(const EffShape &s)
{
    if (s.up > kEffMaxFlank || s.down > kEffMaxFlank || s.site_len < kEffMinSite || s.site_len > kEffMaxSite) return false;
    const uint32_t C = eff_context_len(s);
    if (C > kEffMaxContext) return false;
    return s.gc_start <= C && s.gc_len <= C - s.gc_start;
}

__host__ __device__ inline double eff_undefined()
{
    union {
        uint64_t u;
        double d;
    } v;
    v.u = kEffUndefinedBits;
    return v.d;
}

// bit i of p -> bit 2 i
__host__ __device__ inline uint64_t eff_spread32(uint32_t p)
{
    uint64_t x = p;
    x = (x | (x << 16)) & 0x0000FFFF0000FFFFull;
    x = (x | (x << 8)) & 0x00FF00FF00FF00FFull;
    x = (x | (x << 4)) & 0x0F0F0F0F0F0F0F0Full;
    x = (x | (x << 2)) & 0x3333333333333333ull;
    x = (x | (x << 1)) & 0x5555555555555555ull;
    return x;
}

__host__ __device__ inline uint64_t eff_low_bits(uint32_t n) { return n >= 64u ? ~0ull : (1ull << n) - 1ull; }

// The linear predictor of a context in READ orientation (planes ch, cl: bit j = the high / low bit of the letter at context
// position j, A 0, C 1, G 2, T 3; the bits from C on are 0):  x = intercept;  x = x + mono[j][b_j], j ascending;
// x = x + di[j][4 b_j + b_{j+1}], j ascending;  x = x + gc[#G/C of the range].  Additions only, each rounded once, nothing to
// contract.  Every lane of a wave runs the same C and so the same number of steps; no term is skipped.
__host__ __device__ inline double eff_linear(const double *w, double intercept, const EffShape &s, uint64_t ch, uint64_t cl)
{
    const uint32_t C = eff_context_len(s);
    // the context as a 2-bit code, letter j in bits 2 j + 1, 2 j of word j / 16 (a fifth word of zeros behind them).  Both
    // loops go in blocks of four terms and are unrolled over the 16 blocks, so that the word, every shift count and every
    // row's offset is a constant: a term is one bit-field extract, one address add, one LDS read and the fp64 add, the four
    // reads of a block are in flight together, and leaving at C is a scalar compare per block.  The additions keep their order.
    const uint64_t c0 = eff_spread32((uint32_t)ch) << 1 | eff_spread32((uint32_t)cl);
    const uint64_t c1 = eff_spread32((uint32_t)(ch >> 32)) << 1 | eff_spread32((uint32_t)(cl >> 32));
    const uint32_t code[5] = {(uint32_t)c0, (uint32_t)(c0 >> 32), (uint32_t)c1, (uint32_t)(c1 >> 32), 0u};
    double x = intercept;
    const double *mono = w;
    VSC_EFF_UNROLL
    for (uint32_t q = 0; q < 16u; ++q) {
        const uint32_t j0 = 4u * q, sh = 8u * (q & 3u);
        if (j0 >= C) break;
        const uint32_t word = code[q >> 2];
        if (j0 + 4u <= C) {
            const double t0 = mono[4u * j0 + ((word >> sh) & 3u)], t1 = mono[4u * j0 + 4u + ((word >> (sh + 2u)) & 3u)];
            const double t2 = mono[4u * j0 + 8u + ((word >> (sh + 4u)) & 3u)], t3 = mono[4u * j0 + 12u + ((word >> (sh + 6u)) & 3u)];
            x = x + t0;
            x = x + t1;
            x = x + t2;
            x = x + t3;
        } else {
            for (uint32_t i = 0; i < 3u && j0 + i < C; ++i) x = x + mono[4u * (j0 + i) + ((word >> (sh + 2u * i)) & 3u)];
        }
    }
    const double *dit = w + eff_di_at(C);
    const uint32_t n_di = C - 1u;
    VSC_EFF_UNROLL
    for (uint32_t q = 0; q < 16u; ++q) {
        const uint32_t j0 = 4u * q, sh = 8u * (q & 3u);
        if (j0 >= n_di) break;
        const uint64_t pair = (uint64_t)code[(q >> 2) + 1u] << 32 | code[q >> 2];  // (a word's last letter has its partner in the next)
        if (j0 + 4u <= n_di) {
            const double t0 = dit[16u * j0 + ((uint32_t)(pair >> sh) & 15u)], t1 = dit[16u * j0 + 16u + ((uint32_t)(pair >> (sh + 2u)) & 15u)];
            const double t2 = dit[16u * j0 + 32u + ((uint32_t)(pair >> (sh + 4u)) & 15u)], t3 = dit[16u * j0 + 48u + ((uint32_t)(pair >> (sh + 6u)) & 15u)];
            x = x + t0;
            x = x + t1;
            x = x + t2;
            x = x + t3;
        } else {
            for (uint32_t i = 0; i < 3u && j0 + i < n_di; ++i) x = x + dit[16u * (j0 + i) + ((uint32_t)(pair >> (sh + 2u * i)) & 15u)];
        }
    }
    if (s.gc_len) {
        const uint64_t gc = ((ch ^ cl) >> s.gc_start) & eff_low_bits(s.gc_len);  // G = 10, C = 01
        x = x + w[eff_gc_at(C) + (uint32_t)__builtin_popcountll(gc)];
    }
    return x;
}

// ---- the context of a locus out of the planes -------------------------------------------------------------------------------
// The plane words a genome object holds: word i of hi / lo / nm is word first_word + i of the genome, words [0, held_words)
// are the genome's (what was loaded), the arrays have n_words >= held_words elements.
struct EffPlanes {
    const uint32_t *hi, *lo, *nm;
    uint64_t first_word, held_words, n_words;
    const uint32_t *contig_off, *contig_end;  // global start and end (offset + length) of every contig
    uint32_t n_contigs;
};

// bits [at, at + 64) of a plane; at + C <= 32 held_words.  The words a C-bit window does not reach are not read, and every
// word that is read is checked against the array's length first.
__host__ __device__ inline uint64_t eff_window(const uint32_t *plane, uint64_t n_words, uint64_t at, uint32_t C)
{
    const uint64_t w = at >> 5;
    const uint32_t sh = (uint32_t)at & 31u, need = (sh + C + 31u) >> 5;  // 1 .. 3 words
    const uint32_t w0 = w < n_words ? plane[w] : 0u;
    const uint32_t w1 = need > 1u && w + 1u < n_words ? plane[w + 1u] : 0u;
    const uint32_t w2 = need > 2u && w + 2u < n_words ? plane[w + 2u] : 0u;
    // two funnel shifts: ({w1, w0} >> sh)[31:0] and ({w2, w1} >> sh)[31:0]
    const uint32_t lo = (uint32_t)((((uint64_t)w1 << 32) | w0) >> sh), hi = (uint32_t)((((uint64_t)w2 << 32) | w1) >> sh);
    return (((uint64_t)hi << 32) | lo) & eff_low_bits(C);
}

__host__ __device__ inline uint64_t eff_reverse64(uint64_t x)
{
#if defined(__clang__)
    return __builtin_bitreverse64(x);  // v_bfrev_b32 twice on the device
#else
    x = (x >> 32) | (x << 32);
    x = (x & 0xFFFF0000FFFF0000ull) >> 16 | (x & 0x0000FFFF0000FFFFull) << 16;
    x = (x & 0xFF00FF00FF00FF00ull) >> 8 | (x & 0x00FF00FF00FF00FFull) << 8;
    x = (x & 0xF0F0F0F0F0F0F0F0ull) >> 4 | (x & 0x0F0F0F0F0F0F0F0Full) << 4;
    x = (x & 0xCCCCCCCCCCCCCCCCull) >> 2 | (x & 0x3333333333333333ull) << 2;
    x = (x & 0xAAAAAAAAAAAAAAAAull) >> 1 | (x & 0x5555555555555555ull) << 1;
    return x;
#endif
}

// reverse complement of a C-base plane (revcomp_plane of vsc_device.h at any length): reverse the bit order, complement
__host__ __device__ inline uint64_t eff_revcomp(uint64_t p, uint32_t C) { return (~eff_reverse64(p)) >> (64u - C); }

// The class of locus (contig, pos, strand) under shape s, tested in the order of EffClass, and - for kEffDefined - the planes
// of its context in read orientation: on '+' c[pos - up, pos + site_len + down), on '-' the reverse complement of
// c[pos - down, pos + site_len + up).
__host__ __device__ inline uint32_t eff_context(const EffPlanes &g, const EffShape &s, uint32_t contig, uint32_t pos, uint32_t strand,
                                                uint64_t *ch, uint64_t *cl)
{
    if (contig >= g.n_contigs || strand > 1u) return kEffInvalid;
    const uint32_t off = g.contig_off[contig], len = g.contig_end[contig] - off;
    if (pos > len || len - pos < s.site_len) return kEffInvalid;  // pos + site_len <= len, without the overflow
    const uint32_t left = strand ? s.down : s.up, right = strand ? s.up : s.down;
    if (pos < left || len - pos - s.site_len < right) return kEffOffContig;
    const uint32_t C = eff_context_len(s);
    const uint64_t first = (uint64_t)off + pos - left;  // global position of the context's first base on the forward strand
    if (first < g.first_word * 32u || first + C > (g.first_word + g.held_words) * 32u) return kEffNotResident;
    const uint64_t at = first - g.first_word * 32u;
    // (the three planes' words are asked for together: one memory latency, not two, in front of the sum)
    const uint64_t n = eff_window(g.nm, g.n_words, at, C), h = eff_window(g.hi, g.n_words, at, C), l = eff_window(g.lo, g.n_words, at, C);
    if (n) return kEffHasN;
    *ch = strand ? eff_revcomp(h, C) : h;
    *cl = strand ? eff_revcomp(l, C) : l;
    return kEffDefined;
}

}  // namespace vsc
