// vsc_eff_trees.h - the on-target efficiency score of a regression-tree ensemble (include/varscot_hip.h "SUMS /
// TREES / PREDICTOR") as what the host code (vsc_eff_trees_build, vsc_eff_trees_score_text) shares with the kernels of
// vsc_eff_trees.hip.  The context, its classes and the undefined NaN are eff_context's of vsc_efficiency.h, used as they are.
//
// eff_trees_sums and eff_trees_predict below ARE the definition for one context in read orientation: the kernels call them
// for every candidate (the packed model in LDS), vsc_eff_trees_score_text and the stand-alone check call them on the host -
// one function, one order of the additions, the same bits.  Plain inline functions that a program can include without a device.
//
// The packed model is one array of 32-bit words:
//   [nodes: 2 words each, n_nodes][sums: kEffTreesSumWords each, n_sums][roots: 16 bits each, two per word, n_trees]
// A reference to a node is 14 bits: its number among all nodes of the model (trees one behind the other) and
// kEffTreesLeafBit when that node is a leaf.  A leaf's two words are its double.  An inner node's words:
//   y = left reference | right reference << 14 | (SUM ? 1 << 28 : 0)
//   x = PAIR: pos_a | pos_b << 6 | mask << 12    (a BASE test is the PAIR test with pos_b = pos_a and every letter's nibble
//                                                 of the mask full or empty: index 4 b + b picks the bit of letter b)
//       SUM:  i | t << 4                         (t clamped to 28 signed bits: |S_i| <= 127 * 2^20 < 2^27)
#pragma once

#include <cmath>
#include <cstring>
#include <vector>

#include "varscot_hip.h"
#include "vsc_efficiency.h"

namespace vsc {

constexpr uint32_t kEffTreesMaxSums = 16, kEffTreesMaxTrees = 1024, kEffTreesMaxNodes = 8192, kEffTreesMaxDepth = 32;
constexpr int32_t kEffTreesMaxWeight = 1 << 20;
constexpr uint32_t kEffTreesSumWords = 22;  // start, len, mono[4], di[16]
constexpr uint32_t kEffTreesLeafBit = 1u << 13, kEffTreesRefMask = (1u << 14) - 1u, kEffTreesSumBit = 1u << 28;
constexpr int32_t kEffTreesMaxT = (1 << 27) - 1, kEffTreesMinT = -(1 << 27);

__host__ __device__ inline uint32_t eff_trees_sums_at(uint32_t n_nodes) { return 2u * n_nodes; }
__host__ __device__ inline uint32_t eff_trees_roots_at(uint32_t n_nodes, uint32_t n_sums)
{
    return 2u * n_nodes + kEffTreesSumWords * n_sums;
}
__host__ __device__ inline uint32_t eff_trees_words(uint32_t n_nodes, uint32_t n_sums, uint32_t n_trees)
{
    return eff_trees_roots_at(n_nodes, n_sums) + (n_trees + 1u) / 2u;
}

// The packed model as the two functions read it: `words` in LDS on the device, the model's vector on the host.
struct EffTreesPacked {
    const uint32_t *words;
    uint32_t n_nodes, n_sums, n_trees;
    double base;
};

// S[i * stride] = S_i of the context (planes ch, cl as eff_linear takes them; C its length).  The four letter masks once; a
// letter's count in a range is one popcount, a dinucleotide's popcount(mX & (mY >> 1) & pairs of the range).  The weights
// are the same for every lane of a wave: a term whose weight is 0 is skipped on a scalar condition.
__host__ __device__ inline void eff_trees_sums(const EffTreesPacked &m, uint32_t C, uint64_t ch, uint64_t cl, int32_t *S, uint32_t stride)
{
    const uint64_t all = eff_low_bits(C);
    const uint64_t letter[4] = {~ch & ~cl & all, ~ch & cl, ch & ~cl, ch & cl};
    const uint32_t *w = m.words + eff_trees_sums_at(m.n_nodes);
    for (uint32_t i = 0; i < m.n_sums; ++i, w += kEffTreesSumWords) {
        const uint32_t start = w[0], len = w[1];
        const uint64_t range = eff_low_bits(len) << (start & 63u);  // (len 0: no bit; start = C = 64 comes with len 0 only)
        const uint64_t pairs = range & (range >> 1);                // bit j: j and j + 1 lie in the range
        int32_t s = 0;
        VSC_EFF_UNROLL
        for (uint32_t b = 0; b < 4u; ++b) {
            const int32_t wb = (int32_t)w[2u + b];
            if (wb != 0) s += wb * (int32_t)__builtin_popcountll(letter[b] & range);
        }
        VSC_EFF_UNROLL
        for (uint32_t d = 0; d < 16u; ++d) {
            const int32_t wd = (int32_t)w[6u + d];
            if (wd != 0) s += wd * (int32_t)__builtin_popcountll(letter[d >> 2] & (letter[d & 3u] >> 1) & pairs);
        }
        S[i * stride] = s;
    }
}

// PREDICTOR: x = base; x = x + the leaf the context reaches in tree t, t ascending - every lane of a wave is at the same tree
// and waits for the deepest path of that tree, so that its additions come in tree order.  One 8-byte read per node visited.
__host__ __device__ inline double eff_trees_predict(const EffTreesPacked &m, uint64_t ch, uint64_t cl, const int32_t *S, uint32_t stride)
{
    const uint32_t *nodes = (const uint32_t *)__builtin_assume_aligned(m.words, 8);
    const uint32_t *roots = m.words + eff_trees_roots_at(m.n_nodes, m.n_sums);
    double x = m.base;
    for (uint32_t t = 0; t < m.n_trees; ++t) {
        uint32_t at = (roots[t >> 1] >> (16u * (t & 1u))) & 0xFFFFu;
        while (!(at & kEffTreesLeafBit)) {
            uint32_t n[2];
            __builtin_memcpy(n, nodes + 2u * at, 8);
            bool yes;
            if (n[1] & kEffTreesSumBit) {
                yes = S[(n[0] & 15u) * stride] <= ((int32_t)n[0] >> 4);
            } else {
                const uint32_t pa = n[0] & 63u, pb = (n[0] >> 6) & 63u;
                const uint32_t ba = ((uint32_t)(ch >> pa) & 1u) << 1 | ((uint32_t)(cl >> pa) & 1u);
                const uint32_t bb = ((uint32_t)(ch >> pb) & 1u) << 1 | ((uint32_t)(cl >> pb) & 1u);
                yes = (n[0] >> (12u + 4u * ba + bb)) & 1u;
            }
            at = (yes ? n[1] : n[1] >> 14) & kEffTreesRefMask;
        }
        double v;
        __builtin_memcpy(&v, nodes + 2u * (at & (kEffTreesLeafBit - 1u)), 8);
        x = x + v;
    }
    return x;
}

// ---- the builder (host) -------------------------------------------------------------------------------------------------------
// What a checked model is, beside its packed words.
struct EffTreesBuilt {
    std::vector<uint32_t> words;
    uint32_t by_kind[4] = {};  // nodes by VSC_EFF_NODE_*
    uint32_t n_nodes = 0, max_depth = 0;
    double base = 0;
};

// Checks a model against every rule of the definition and packs it; false: the model breaks a rule (VSC_ERR_INVALID), `out`
// is then not to be used.  shape: gc_len 0.  The kernels and eff_trees_predict rely on what is checked here - every
// reference inside the model, every sum index below n_sums, every walk finite - and check nothing again.
inline bool eff_trees_pack(const EffShape &shape, double base, const vsc_eff_sum *sums, uint32_t n_sums, const vsc_eff_node *nodes,
                           const uint32_t *tree_first, uint32_t n_trees, EffTreesBuilt &out)
{
    if (!eff_shape_valid(shape) || shape.gc_start || shape.gc_len || !std::isfinite(base)) return false;
    if (n_sums > kEffTreesMaxSums || (n_sums != 0) != (sums != nullptr)) return false;
    if (n_trees < 1 || n_trees > kEffTreesMaxTrees || !tree_first || !nodes || tree_first[0] != 0) return false;
    for (uint32_t t = 0; t < n_trees; ++t)
        if (tree_first[t + 1] <= tree_first[t] || tree_first[t + 1] > kEffTreesMaxNodes) return false;
    const uint32_t C = eff_context_len(shape), n_nodes = tree_first[n_trees];
    out = EffTreesBuilt{};
    out.n_nodes = n_nodes;
    out.base = base == 0.0 ? 0.0 : base;
    out.words.assign(eff_trees_words(n_nodes, n_sums, n_trees), 0u);
    uint32_t *w = out.words.data() + eff_trees_sums_at(n_nodes);
    for (uint32_t i = 0; i < n_sums; ++i, w += kEffTreesSumWords) {
        const vsc_eff_sum &s = sums[i];
        if (s.start > C || s.len > C - s.start) return false;
        w[0] = s.start;
        w[1] = s.len;
        for (uint32_t k = 0; k < 20; ++k) {
            const int32_t v = k < 4 ? s.mono[k] : s.di[k - 4];
            if (v > kEffTreesMaxWeight || v < -kEffTreesMaxWeight) return false;
            w[2 + k] = (uint32_t)v;
        }
    }
    uint32_t *roots = out.words.data() + eff_trees_roots_at(n_nodes, n_sums);
    std::vector<uint32_t> depth, parents;
    for (uint32_t t = 0; t < n_trees; ++t) {
        const uint32_t first = tree_first[t], m = tree_first[t + 1] - first;
        const vsc_eff_node *tree = nodes + first;
        depth.assign(m, 0u);
        parents.assign(m, 0u);
        auto ref = [&](uint32_t k) { return (first + k) | (tree[k].kind == VSC_EFF_NODE_LEAF ? kEffTreesLeafBit : 0u); };
        for (uint32_t k = 0; k < m; ++k) {  // parents come before their children: a node's depth is known when it is reached
            const vsc_eff_node &n = tree[k];
            if (n.kind > VSC_EFF_NODE_SUM || n.reserved) return false;
            if (parents[k] != (k ? 1u : 0u)) return false;  // a node with no parent (or the root with one), or with two
            if (depth[k] > out.max_depth) out.max_depth = depth[k];
            ++out.by_kind[n.kind];
            uint32_t *p = out.words.data() + 2u * (first + k);
            if (n.kind == VSC_EFF_NODE_LEAF) {
                if (!std::isfinite(n.value) || n.a || n.b || n.mask || n.t || n.left || n.right) return false;
                const double v = n.value == 0.0 ? 0.0 : n.value;
                memcpy(p, &v, 8);
                continue;
            }
            if (n.value != 0.0 || n.left <= k || n.right <= k || n.left >= m || n.right >= m || n.left == n.right) return false;
            if (depth[k] + 1u > kEffTreesMaxDepth) return false;
            for (uint32_t c : {n.left, n.right}) {
                if (++parents[c] > 1u) return false;
                depth[c] = depth[k] + 1u;
            }
            p[1] = ref(n.left) | ref(n.right) << 14;
            if (n.kind == VSC_EFF_NODE_SUM) {
                if (n.a >= n_sums || n.b || n.mask) return false;
                const int32_t tt = n.t > kEffTreesMaxT ? kEffTreesMaxT : n.t < kEffTreesMinT ? kEffTreesMinT : n.t;
                p[0] = n.a | (uint32_t)tt << 4;
                p[1] |= kEffTreesSumBit;
            } else if (n.kind == VSC_EFF_NODE_PAIR) {
                if (n.a >= C || n.b >= C || n.a == n.b || n.mask > 0xFFFFu || n.t) return false;
                p[0] = n.a | n.b << 6 | n.mask << 12;
            } else {
                if (n.a >= C || n.b || n.mask > 0xFu || n.t) return false;
                uint32_t wide = 0;  // letter b's bit at 4 b + b
                for (uint32_t b = 0; b < 4; ++b) wide |= ((n.mask >> b) & 1u) << (5u * b);
                p[0] = n.a | n.a << 6 | wide << 12;
            }
        }
        roots[t >> 1] |= ref(0) << (16u * (t & 1u));
    }
    return true;
}

}  // namespace vsc
