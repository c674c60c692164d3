// efficiency_trees_check.cpp - the tree-ensemble efficiency score of varscot_amd/csrc/vsc_eff_trees.h (eff_trees_pack,
// eff_trees_sums, eff_trees_predict) on top of eff_context of vsc_efficiency.h, in a stand-alone program with its own main, for
// the host sanitizers.  No device is opened and no kernel is launched.  Build and run on the CPU:
//   hipcc --offload-arch=gfx950 -x hip -O1 -g -std=c++17 -ffp-contract=off -Iinclude -Ivarscot_amd/csrc -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tools/efficiency_trees_check.cpp -o build/efficiency_trees_check && build/efficiency_trees_check
// Three shapes (4+23+3; C = 64; no flanks), seven families of models (100 trees of depth 3; stumps; a chain of depth 32 beside
// single leaves; 1 024 single leaves; leaves of 1e16 / 1 / 1e-16; the largest model of 8 192 nodes and 16 sums; the edges:
// thresholds on attainable sums, constant masks, ranges of length 0, 1 and C):
//   - every (contig, position, strand) of a small genome packed into plane arrays of exactly the held words - the whole genome
//     and a view that starts at word 1 and ends one word early - through eff_context, eff_trees_sums and eff_trees_predict,
//     against the sums and the walk taken letter by letter from the text over the caller's nodes, bit for bit.  The packed model
//     holds exactly eff_trees_words words and the sums exactly n_sums ints: a read past either end is the sanitizer's to find;
//   - the builder over every model the definition refuses, and over its nearest neighbour that it accepts.
// Exit code 0 and "ok" when all agree.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "vsc_eff_trees.h"

using namespace vsc;

static int code(char c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 4; }

static std::string revcomp(const std::string &s)
{
    std::string r(s.rbegin(), s.rend());
    for (char &c : r) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : 'N';
    return r;
}

static void planes_of(const std::string &t, uint64_t *h, uint64_t *l)
{
    *h = *l = 0;
    for (size_t j = 0; j < t.size(); ++j) {
        *h |= (uint64_t)(code(t[j]) >> 1) << j;
        *l |= (uint64_t)(code(t[j]) & 1) << j;
    }
}

struct Model {
    EffShape s;
    double base;
    std::vector<vsc_eff_sum> sums;
    std::vector<vsc_eff_node> nodes;
    std::vector<uint32_t> first;  // n_trees + 1
};

static bool pack(const Model &m, EffTreesBuilt &out)
{
    return eff_trees_pack(m.s, m.base, m.sums.empty() ? nullptr : m.sums.data(), (uint32_t)m.sums.size(), m.nodes.data(), m.first.data(),
                          (uint32_t)m.first.size() - 1, out);
}

// the definition, letter by letter
static int32_t sum_by_letters(const vsc_eff_sum &s, const std::string &t)
{
    int32_t v = 0;
    for (uint32_t j = s.start; j < s.start + s.len; ++j) {
        v += s.mono[code(t[j])];
        if (j + 1 < s.start + s.len) v += s.di[4 * code(t[j]) + code(t[j + 1])];
    }
    return v;
}

static double by_letters(const Model &m, const std::string &t)
{
    std::vector<int32_t> S;
    for (const vsc_eff_sum &s : m.sums) S.push_back(sum_by_letters(s, t));
    double x = m.base;
    for (size_t tr = 0; tr + 1 < m.first.size(); ++tr) {
        const vsc_eff_node *tree = m.nodes.data() + m.first[tr];
        uint32_t k = 0;
        while (tree[k].kind != VSC_EFF_NODE_LEAF) {
            const vsc_eff_node &n = tree[k];
            bool yes;
            if (n.kind == VSC_EFF_NODE_BASE) yes = (n.mask >> code(t[n.a])) & 1u;
            else if (n.kind == VSC_EFF_NODE_PAIR) yes = (n.mask >> (4 * code(t[n.a]) + code(t[n.b]))) & 1u;
            else yes = S[n.a] <= n.t;
            k = yes ? n.left : n.right;
        }
        x = x + tree[k].value;
    }
    return x;
}

static double rnd_leaf(int family)
{
    const double u = (double)(std::rand() % 200001 - 100000) / 50000.0;
    const double scale[3] = {1e16, 1.0, 1e-16};
    return family == 4 ? u * scale[std::rand() % 3] : u;
}

static vsc_eff_node leaf(double v)
{
    vsc_eff_node n{};
    n.kind = VSC_EFF_NODE_LEAF;
    n.value = v;
    return n;
}

static vsc_eff_node rnd_test(const Model &m, uint32_t C)
{
    vsc_eff_node n{};
    n.kind = 1 + (uint32_t)std::rand() % (m.sums.empty() ? 2 : 3);
    if (n.kind == VSC_EFF_NODE_BASE) {
        n.a = (uint32_t)std::rand() % C;
        n.mask = (uint32_t)std::rand() % 16;
    } else if (n.kind == VSC_EFF_NODE_PAIR) {
        n.a = (uint32_t)std::rand() % C;
        n.b = (n.a + 1 + (uint32_t)std::rand() % (C - 1)) % C;
        n.mask = (uint32_t)std::rand() & 0xFFFFu;
    } else {
        n.a = (uint32_t)std::rand() % m.sums.size();
        std::string t(C, 'A');
        for (char &c : t) c = "ACGT"[std::rand() % 4];
        n.t = sum_by_letters(m.sums[n.a], t) + std::rand() % 3 - 1;  // on, or next to, a sum some context has
    }
    return n;
}

// a complete tree of `depth`, numbered level by level: node k's children are 2 k + 1 and 2 k + 2
static void add_complete(Model &m, uint32_t C, uint32_t depth, int family)
{
    const uint32_t inner = (1u << depth) - 1, all = (2u << depth) - 1;
    for (uint32_t k = 0; k < all; ++k) {
        if (k >= inner) {
            m.nodes.push_back(leaf(rnd_leaf(family)));
            continue;
        }
        vsc_eff_node n = rnd_test(m, C);
        n.left = 2 * k + 1, n.right = 2 * k + 2;
        if (std::rand() % 2) std::swap(n.left, n.right);
        m.nodes.push_back(n);
    }
    m.first.push_back((uint32_t)m.nodes.size());
}

// a chain of `depth` edges in preorder: node 2 k is inner, 2 k + 1 its leaf, 2 k + 2 the next inner node
static void add_chain(Model &m, uint32_t C, uint32_t depth, int family)
{
    for (uint32_t k = 0; k < depth; ++k) {
        vsc_eff_node n = rnd_test(m, C);
        if (k % 4) n.kind = VSC_EFF_NODE_BASE, n.a = k % C, n.b = 0, n.t = 0, n.mask = 0;  // (constant: most walks go deep)
        n.left = 2 * k + 1, n.right = 2 * k + 2;
        m.nodes.push_back(n);
        m.nodes.push_back(leaf(rnd_leaf(family)));
    }
    m.nodes.push_back(leaf(rnd_leaf(family)));
    m.first.push_back((uint32_t)m.nodes.size());
}

static vsc_eff_sum rnd_sum(uint32_t start, uint32_t len, int32_t scale)
{
    vsc_eff_sum s{};
    s.start = start, s.len = len;
    for (int32_t &w : s.mono) w = std::rand() % 3 ? std::rand() % (2 * scale + 1) - scale : 0;
    for (int32_t &w : s.di) w = std::rand() % 3 ? 0 : std::rand() % (2 * scale + 1) - scale;
    return s;
}

static Model make_model(const EffShape &s, int family)
{
    Model m{s, family == 2 ? -1.0 : 0.4921, {}, {}, {0}};
    const uint32_t C = eff_context_len(s);
    if (family != 3) {
        vsc_eff_sum gc{};
        gc.start = s.up, gc.len = s.site_len < 20 ? s.site_len : 20;
        gc.mono[1] = gc.mono[2] = 1;
        m.sums = {gc, rnd_sum(0, C, 1), rnd_sum(s.up, s.site_len, 300)};
    }
    if (family == 0) for (int t = 0; t < 100; ++t) add_complete(m, C, 3, family);
    if (family == 1) for (int t = 0; t < 64; ++t) add_complete(m, C, 1, family);
    if (family == 2) for (int t = 0; t < 64; ++t) t == 31 ? add_chain(m, C, 32, family) : add_complete(m, C, 0, family);
    if (family == 3) for (int t = 0; t < 1024; ++t) add_complete(m, C, 0, family);
    if (family == 4) for (int t = 0; t < 60; ++t) add_complete(m, C, 2, family);
    if (family == 5) {
        while (m.sums.size() < 16) {
            const uint32_t start = (uint32_t)std::rand() % (C + 1);
            m.sums.push_back(rnd_sum(start, (uint32_t)std::rand() % (C - start + 1), 1 << 20));
        }
        for (int k = 0; k < 4; ++k) m.sums[3].mono[k] = 1 << 20, m.sums[4].mono[k] = -(1 << 20);  // the largest sums there are
        for (int k = 0; k < 16; ++k) m.sums[3].di[k] = 1 << 20, m.sums[4].di[k] = -(1 << 20);
        m.sums[3].start = m.sums[4].start = 0, m.sums[3].len = m.sums[4].len = C;
        for (int t = 0; t < 544; ++t) add_complete(m, C, 3, family);
        add_complete(m, C, 4, family);
        add_complete(m, C, 0, family);
    }
    if (family == 6) {
        m.sums[1] = rnd_sum(C, 0, 5);      // ranges of length 0 (at the context's end), 1 and C
        m.sums[2] = rnd_sum(C - 1, 1, 5);
        m.sums.push_back(rnd_sum(0, C, 1 << 20));
        auto stump = [&](vsc_eff_node n) {
            n.left = 1, n.right = 2;
            m.nodes.push_back(n);
            m.nodes.push_back(leaf(rnd_leaf(family)));
            m.nodes.push_back(leaf(rnd_leaf(family)));
            m.first.push_back((uint32_t)m.nodes.size());
        };
        vsc_eff_node n{};
        n.kind = VSC_EFF_NODE_SUM;
        for (int32_t t = -1; t <= 21; ++t) n.a = 0, n.t = t, stump(n);
        for (int32_t t = -1; t <= 1; ++t) n.a = 1, n.t = t, stump(n);
        for (int32_t t = -6; t <= 6; ++t) n.a = 2, n.t = t, stump(n);
        for (int32_t t : {INT32_MIN, -(1 << 27), -(1 << 27) + 1, -1, 0, (1 << 27) - 1, 1 << 27, INT32_MAX}) n.a = 3, n.t = t, stump(n);
        n = vsc_eff_node{};
        n.kind = VSC_EFF_NODE_BASE;
        for (uint32_t pos : {0u, C - 1}) for (uint32_t mask : {0u, 15u, 1u, 14u}) n.a = pos, n.mask = mask, stump(n);
        n = vsc_eff_node{};
        n.kind = VSC_EFF_NODE_PAIR;
        for (uint32_t mask : {0u, 0xFFFFu, 1u << 1, 1u << 4, 0x8421u}) {
            n.a = C - 1, n.b = 0, n.mask = mask, stump(n);
            n.a = 0, n.b = C - 1, stump(n);
        }
    }
    return m;
}

// every model the definition refuses, made from one that it accepts
static int refusals()
{
    const EffShape s{4, 23, 3, 0, 0};
    Model good{s, 0.0, {}, {}, {0}};
    vsc_eff_sum sum{};
    sum.len = 30;
    good.sums.push_back(sum);
    vsc_eff_node root{};
    root.kind = VSC_EFF_NODE_BASE, root.a = 3, root.mask = 5, root.left = 1, root.right = 2;
    vsc_eff_node second = root;
    second.kind = VSC_EFF_NODE_SUM, second.a = 0, second.mask = 0, second.t = 7, second.left = 3, second.right = 4;
    good.nodes = {root, second, leaf(1.0), leaf(2.0), leaf(3.0)};
    good.first = {0, 5};
    EffTreesBuilt built;
    if (!pack(good, built)) return 20;
    int at = 21;
    auto refused = [&](Model m) { ++at; return !pack(m, built); };
    Model m = good;
    m.nodes[1].left = 1;  // a child not larger than its parent
    if (!refused(m)) return at;
    m = good, m.nodes[1].right = 5;  // a child outside the tree
    if (!refused(m)) return at;
    m = good, m.nodes[1].left = 2;  // a node with two parents (and one with none)
    if (!refused(m)) return at;
    m = good, m.nodes.push_back(leaf(4.0)), m.first[1] = 6;  // a node with no parent
    if (!refused(m)) return at;
    m = good, m.nodes[1].left = m.nodes[1].right = 3;
    if (!refused(m)) return at;
    for (uint32_t depth : {32u, 33u}) {  // a depth of 33, next to a depth of 32
        Model c{s, 0.0, {}, {}, {0}};
        add_chain(c, 30, depth, 0);
        if (pack(c, built) != (depth == 32)) return 30;
    }
    for (uint32_t extra : {2u, 3u}) {  // 8 193 nodes, next to 8 192
        Model c{s, 0.0, {}, {}, {0}};
        for (int t = 0; t < 126; ++t) add_chain(c, 30, 32, 0);
        for (uint32_t t = 0; t < extra; ++t) add_complete(c, 30, 0, 0);
        if (pack(c, built) != (extra == 2)) return 31;
    }
    for (uint32_t trees : {1024u, 1025u}) {
        Model c{s, 0.0, {}, {}, {0}};
        for (uint32_t t = 0; t < trees; ++t) add_complete(c, 30, 0, 0);
        if (pack(c, built) != (trees == 1024)) return 32;
    }
    m = good, m.nodes[2].value = INFINITY;  // a value that is not finite
    if (!refused(m)) return at;
    m = good, m.nodes[3].value = NAN;
    if (!refused(m)) return at;
    m = good, m.base = -INFINITY;
    if (!refused(m)) return at;
    m = good, m.sums[0].mono[2] = (1 << 20) + 1;  // a weight of 2^20 + 1
    if (!refused(m)) return at;
    m = good, m.sums[0].di[15] = -(1 << 20) - 1;
    if (!refused(m)) return at;
    m = good, m.sums[0].mono[2] = 1 << 20, m.sums[0].di[15] = -(1 << 20);
    if (refused(m)) return at;
    m = good, m.sums[0].start = 1;  // a range that leaves the context
    if (!refused(m)) return at;
    m = good, m.sums[0].start = 0xFFFFFFF0u, m.sums[0].len = 0x20u;
    if (!refused(m)) return at;
    m = good, m.nodes[0].kind = VSC_EFF_NODE_PAIR, m.nodes[0].b = 3;  // pos_a == pos_b
    if (!refused(m)) return at;
    m = good, m.nodes[0].a = 30;  // a position outside the context
    if (!refused(m)) return at;
    m = good, m.nodes[0].mask = 16;
    if (!refused(m)) return at;
    m = good, m.nodes[1].a = 1;  // a sum that does not exist
    if (!refused(m)) return at;
    m = good, m.nodes[1].kind = 4;
    if (!refused(m)) return at;
    m = good, m.sums.resize(17);
    if (!refused(m)) return at;
    m = good, m.s.up = 17;
    if (!refused(m)) return at;
    m = good, m.first = {0, 3, 3, 5};  // a tree without a node
    if (!refused(m)) return at;
    return 0;
}

int main()
{
    std::srand(37);
    const uint32_t shapes[3][3] = {{4, 23, 3}, {16, 32, 16}, {0, 16, 0}};
    unsigned long long loci = 0, defined = 0, models = 0;
    for (const auto &sh : shapes) {
        const uint32_t C = sh[0] + sh[1] + sh[2];
        const EffShape s{sh[0], sh[1], sh[2], 0, 0};
        // contigs of C - 1, C, C + 1, 5, 200 (an N at 100) and 131 bases, one N apart
        const uint32_t lens[6] = {C - 1, C, C + 1, 5, 200, 131};
        std::vector<std::string> contig;
        std::vector<uint32_t> off, end;
        std::string genome;
        for (uint32_t len : lens) {
            std::string t(len, 'A');
            for (char &c : t) c = "ACGT"[std::rand() % 4];
            if (len == 200) t[100] = 'N';
            off.push_back((uint32_t)genome.size());
            genome += t;
            end.push_back((uint32_t)genome.size());
            genome += 'N';
            contig.push_back(t);
        }
        const uint64_t words = (genome.size() + 31) / 32;
        std::vector<uint32_t> hi(words, 0), lo(words, 0), nm(words, 0);
        for (uint64_t g = 0; g < words * 32; ++g) {
            const int b = g < genome.size() ? code(genome[g]) : 4;
            if (b > 3) nm[g >> 5] |= 1u << (g & 31);
            else {
                hi[g >> 5] |= (uint32_t)(b >> 1) << (g & 31);
                lo[g >> 5] |= (uint32_t)(b & 1) << (g & 31);
            }
        }
        for (int family = 0; family < 7; ++family) {
            const Model m = make_model(s, family);
            EffTreesBuilt built;
            if (!pack(m, built)) return 1;
            const uint32_t n_sums = (uint32_t)m.sums.size(), n_trees = (uint32_t)m.first.size() - 1;
            if (built.words.size() != eff_trees_words(built.n_nodes, n_sums, n_trees)) return 2;
            if (family == 5 && (built.n_nodes != 8192 || n_sums != 16)) return 2;
            const std::vector<uint32_t> words_exact(built.words.begin(), built.words.end());  // capacity == size: a read past the end is seen
            const EffTreesPacked packed{words_exact.data(), built.n_nodes, n_sums, n_trees, built.base};
            ++models;
            for (int view = 0; view < 2; ++view) {  // the whole genome; words [1, words - 1) in arrays of exactly that length
                const uint64_t first = view ? 1 : 0, held = words - 2 * first;
                const std::vector<uint32_t> vh(hi.begin() + first, hi.begin() + first + held), vl(lo.begin() + first, lo.begin() + first + held),
                    vn(nm.begin() + first, nm.begin() + first + held);
                const EffPlanes g{vh.data(), vl.data(), vn.data(), first, held, held, off.data(), end.data(), (uint32_t)contig.size()};
                for (uint32_t c = 0; c < contig.size(); ++c)
                    for (uint32_t p = 0; p + s.site_len <= contig[c].size(); p += family == 5 ? 3 : 1)
                        for (uint32_t strand = 0; strand < 2; ++strand) {
                            uint64_t h = 0, l = 0;
                            const uint32_t cls = eff_context(g, s, c, p, strand, &h, &l);
                            ++loci;
                            // what the kernels do: a candidate without a context walks an all-A context
                            std::vector<int32_t> S(n_sums);
                            eff_trees_sums(packed, C, h, l, S.data(), 1);
                            const double x = eff_trees_predict(packed, h, l, S.data(), 1);
                            std::string text(C, 'A');
                            if (cls == kEffDefined) {
                                const uint32_t left = strand ? s.down : s.up;
                                text = contig[c].substr(p - left, C);
                                if (strand) text = revcomp(text);
                                uint64_t wh, wl;
                                planes_of(text, &wh, &wl);
                                if (h != wh || l != wl) return 3;
                                ++defined;
                            }
                            for (uint32_t i = 0; i < n_sums; ++i)
                                if (S[i] != sum_by_letters(m.sums[i], text)) return 4;
                            const double y = by_letters(m, text);
                            if (std::memcmp(&x, &y, sizeof x) != 0) return 5;
                        }
            }
        }
    }
    if (const int rc = refusals()) return rc;
    if (defined == 0 || defined == loci) return 10;
    std::printf("ok: %llu models, %llu loci (%llu defined), every refusal\n", models, loci, defined);
    return 0;
}
