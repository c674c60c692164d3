// eff_trees_host.hpp - the -Y option of guide_summary and pattern_search with a TREE model: an on-target efficiency model that
// is a sum of regression trees (include/varscot_hip.h "regression-tree ensembles") read from the text file that
// varscot_amd.TreeEfficiencyModel.to_tsv writes (tools/README.md):
//   shape up site_len down | link identity|logistic | intercept x (the base) | sum I START LENGTH | sumw I X|XY W | tree T |
//   leaf K V | base_in K POS LETTERS L R | pair_in K POSA POSB XY[,XY...] L R | sum_le K I T L R
// one entry per line, tab- or blank-separated, '#' starts a comment, '-' is the empty set of letters.  I, T and K ascend from
// 0; a node belongs to the last `tree` line.  A file is a tree model when it holds a `tree` line: the lines of a linear model
// (mono, di, gc, gc_range) are then refused.  Every refusal - of a line, or of the tree it completes - carries FILE:LINE.
// EffAnyModel is what the tools hold: the one or the other model, and the calls that go to the one or the other entry.
#pragma once

#include <cerrno>
#include <cstdint>

#include "eff_model_host.hpp"

namespace vsc_host {

// does `path` hold a `tree` line?
inline bool is_eff_trees_file(const std::string &path)
{
    std::ifstream in(path);
    if (!in) throw std::runtime_error("Could not open the -Y file.");
    for (std::string line; std::getline(in, line);) {
        std::istringstream is(line.substr(0, line.find('#')));
        std::string key;
        if (is >> key && key == "tree") return true;
    }
    return false;
}

// the model of `path` (freed with vsc_eff_trees_free); *shape = its shape
inline vsc_eff_trees *load_eff_trees(const std::string &path, vsc_eff_shape *shape)
{
    std::ifstream in(path);
    if (!in) throw std::runtime_error("Could not open the -Y file.");
    vsc_eff_shape s{};
    bool have_shape = false;
    double intercept = 0.0;
    std::vector<vsc_eff_sum> sums;
    std::vector<vsc_eff_node> nodes;
    std::vector<uint32_t> first;       // first node of every tree
    std::set<std::string> once;
    std::string line;
    size_t n = 0;
    auto base = [](char c) { return c == 'A' || c == 'a' ? 0 : c == 'C' || c == 'c' ? 1 : c == 'G' || c == 'g' ? 2 : c == 'T' || c == 't' || c == 'U' || c == 'u' ? 3 : -1; };
    const auto where = [&](size_t at) { return "-Y: " + path + ":" + std::to_string(at) + ": "; };
    // the tree that ends in front of line `at` (or the file's end): the rules of a tree are checked where the tree is complete
    const auto close_tree = [&](size_t at) {
        if (first.empty()) return;
        const uint32_t from = first.back(), m = (uint32_t)nodes.size() - from;
        const std::string tree = "tree " + std::to_string(first.size() - 1) + " ";
        if (m == 0) throw std::runtime_error(where(at) + tree + "has no node");
        std::vector<uint32_t> parents(m, 0), depth(m, 0);
        for (uint32_t k = 0; k < m; ++k) {
            const vsc_eff_node &nd = nodes[from + k];
            if (parents[k] != (k ? 1u : 0u)) throw std::runtime_error(where(at) + tree + "node " + std::to_string(k) + " is the child of no node, or of two");
            if (nd.kind == VSC_EFF_NODE_LEAF) continue;
            if (nd.left <= k || nd.right <= k || nd.left >= m || nd.right >= m || nd.left == nd.right)
                throw std::runtime_error(where(at) + tree + "node " + std::to_string(k) + ": its children are two nodes of the tree with larger numbers");
            if (depth[k] + 1 > 32) throw std::runtime_error(where(at) + tree + "is deeper than 32");
            for (uint32_t c : {nd.left, nd.right}) {
                if (++parents[c] > 1) throw std::runtime_error(where(at) + tree + "node " + std::to_string(c) + " is the child of two nodes");
                depth[c] = depth[k] + 1;
            }
        }
    };
    while (std::getline(in, line)) {
        ++n;
        const auto bad = [&](const std::string &what) { return std::runtime_error(where(n) + what); };
        std::istringstream is(line.substr(0, line.find('#')));
        std::vector<std::string> f;
        for (std::string w; is >> w;) f.push_back(w);
        if (f.empty()) continue;
        const std::string &key = f[0];
        const auto integer = [&](const std::string &v, long lo, long hi) {
            char *e = nullptr;
            errno = 0;
            const long x = std::strtol(v.c_str(), &e, 10);
            if (e == v.c_str() || *e || errno) throw bad("'" + v + "' is no integer");
            if (x < lo || x > hi) throw bad("'" + v + "' lies outside " + std::to_string(lo) + " .. " + std::to_string(hi));
            return x;
        };
        const auto number = [&](const std::string &v) {
            char *e = nullptr;
            const double x = std::strtod(v.c_str(), &e);
            if (e == v.c_str() || *e || !std::isfinite(x)) throw bad("'" + v + "' is no finite number");
            return x;
        };
        // LETTERS of a BASE test (width 1) or XY[,XY...] of a PAIR test (width 2) as a mask; '-': no bit
        const auto mask_of = [&](const std::string &v, size_t width) {
            uint32_t mask = 0;
            if (v == "-") return mask;
            for (size_t at = 0; at < v.size();) {
                uint32_t code = 0;
                for (size_t i = 0; i < width; ++i, ++at) {
                    if (at >= v.size() || base(v[at]) < 0) throw bad("'" + v + "' holds a letter that is no base");
                    code = 4 * code + (uint32_t)base(v[at]);
                }
                if (mask >> code & 1u) throw bad("'" + v + "' names a letter twice");
                mask |= 1u << code;
                if (width == 2 && at < v.size()) {
                    if (v[at] != ',' || at + 1 == v.size()) throw bad("'" + v + "' is no list of dinucleotides");
                    ++at;
                }
            }
            return mask;
        };
        if (key == "mono" || key == "di" || key == "gc" || key == "gc_range")
            throw bad("'" + key + "' belongs to a linear model; this file holds a tree model");
        if (key == "shape" || key == "link" || key == "intercept") {
            if (!once.insert(key).second) throw bad("'" + key + "' is given twice");
        } else if (!have_shape) {
            throw bad("'" + key + "' before the 'shape' line");
        }
        const long C = (long)(s.up + s.site_len + s.down);
        const bool node = key == "leaf" || key == "base_in" || key == "pair_in" || key == "sum_le";
        if (node) {
            if (first.empty()) throw bad("'" + key + "' before the first 'tree' line");
            if (f.size() < 2 || integer(f[1], 0, 8192) != (long)(nodes.size() - first.back()))
                throw bad("node out of turn: node " + std::to_string(nodes.size() - first.back()) + " of tree " + std::to_string(first.size() - 1) + " comes next");
            if (nodes.size() >= 8192) throw bad("more than 8192 nodes");
        }
        vsc_eff_node nd{};
        if (key == "shape" && f.size() == 4) {
            const long a = integer(f[1], 0, 16), b = integer(f[2], 16, 32), c = integer(f[3], 0, 16);
            if (a + b + c > 64) throw bad("a shape has flanks of 0 .. 16, a site of 16 .. 32 and a context of at most 64 bases");
            s.up = (uint32_t)a, s.site_len = (uint32_t)b, s.down = (uint32_t)c;
            have_shape = true;
        } else if (key == "link" && f.size() == 2) {
            if (f[1] != "identity" && f[1] != "logistic") throw bad("link must be 'identity' or 'logistic'");
            s.link = f[1] == "logistic" ? VSC_EFF_LOGISTIC : VSC_EFF_IDENTITY;
        } else if (key == "intercept" && f.size() == 2) {
            intercept = number(f[1]);
        } else if (key == "sum" && f.size() == 4) {
            if (sums.size() >= 16) throw bad("more than 16 sums");
            if (integer(f[1], 0, 16) != (long)sums.size()) throw bad("sum out of turn: sum " + std::to_string(sums.size()) + " comes next");
            vsc_eff_sum sum{};
            sum.start = (uint32_t)integer(f[2], 0, C);
            sum.len = (uint32_t)integer(f[3], 0, C - (long)sum.start);
            sums.push_back(sum);
        } else if (key == "sumw" && f.size() == 4) {
            const long i = integer(f[1], 0, 15);
            if (i >= (long)sums.size()) throw bad("'sumw' before its 'sum " + f[1] + "' line");
            if (f[2].size() != 1 && f[2].size() != 2) throw bad("'sumw' takes one letter or two");
            int code = 0;
            std::string canon = "sumw " + std::to_string(i) + ' ';
            for (char ch : f[2]) {
                if (base(ch) < 0) throw bad("'" + f[2] + "' holds a letter that is no base");
                code = 4 * code + base(ch);
                canon += "ACGT"[base(ch)];
            }
            if (!once.insert(canon).second) throw bad("weight " + f[2] + " of sum " + f[1] + " is given twice");
            (f[2].size() == 1 ? sums[(size_t)i].mono[code] : sums[(size_t)i].di[code]) = (int32_t)integer(f[3], -(1l << 20), 1l << 20);
        } else if (key == "tree" && f.size() == 2) {
            if (first.size() >= 1024) throw bad("more than 1024 trees");
            if (integer(f[1], 0, 1024) != (long)first.size()) throw bad("tree out of turn: tree " + std::to_string(first.size()) + " comes next");
            close_tree(n);
            first.push_back((uint32_t)nodes.size());
        } else if (key == "leaf" && f.size() == 3) {
            nd.kind = VSC_EFF_NODE_LEAF;
            nd.value = number(f[2]);
            nodes.push_back(nd);
        } else if (key == "base_in" && f.size() == 6) {
            nd.kind = VSC_EFF_NODE_BASE;
            nd.a = (uint32_t)integer(f[2], 0, C - 1);
            nd.mask = mask_of(f[3], 1);
            nd.left = (uint32_t)integer(f[4], 0, 8191), nd.right = (uint32_t)integer(f[5], 0, 8191);
            nodes.push_back(nd);
        } else if (key == "pair_in" && f.size() == 7) {
            nd.kind = VSC_EFF_NODE_PAIR;
            nd.a = (uint32_t)integer(f[2], 0, C - 1), nd.b = (uint32_t)integer(f[3], 0, C - 1);
            if (nd.a == nd.b) throw bad("a pair names two positions");
            nd.mask = mask_of(f[4], 2);
            nd.left = (uint32_t)integer(f[5], 0, 8191), nd.right = (uint32_t)integer(f[6], 0, 8191);
            nodes.push_back(nd);
        } else if (key == "sum_le" && f.size() == 6) {
            nd.kind = VSC_EFF_NODE_SUM;
            nd.a = (uint32_t)integer(f[2], 0, 15);
            if (nd.a >= sums.size()) throw bad("sum " + f[2] + " is not defined");
            nd.t = (int32_t)integer(f[3], INT32_MIN, INT32_MAX);
            nd.left = (uint32_t)integer(f[4], 0, 8191), nd.right = (uint32_t)integer(f[5], 0, 8191);
            nodes.push_back(nd);
        } else {
            throw bad("unknown key or wrong number of fields: '" + line + "'");
        }
    }
    if (!have_shape) throw std::runtime_error("-Y: " + path + ": no 'shape' line");
    if (first.empty()) throw std::runtime_error("-Y: " + path + ": no 'tree' line");
    close_tree(n + 1);
    first.push_back((uint32_t)nodes.size());
    vsc_eff_trees *model = nullptr;
    if (vsc_eff_trees_build(&s, intercept, sums.empty() ? nullptr : sums.data(), (uint32_t)sums.size(), nodes.data(), first.data(),
                            (uint32_t)first.size() - 1, &model) != VSC_OK)
        throw std::runtime_error("-Y: " + path + ":" + std::to_string(n) + ": the library refuses this model");
    *shape = s;
    return model;
}

// The model of a -Y file, of the one kind or the other.
struct EffAnyModel {
    vsc_eff_model *linear = nullptr;
    vsc_eff_trees *trees = nullptr;
};

inline EffAnyModel load_eff_any(const std::string &path, vsc_eff_shape *shape)
{
    EffAnyModel m;
    if (is_eff_trees_file(path)) m.trees = load_eff_trees(path, shape);
    else m.linear = load_eff_model(path, shape);
    return m;
}

inline void eff_any_free(EffAnyModel &m)
{
    vsc_eff_model_free(m.linear);
    vsc_eff_trees_free(m.trees);
    m = EffAnyModel{};
}

inline double eff_any_link(const EffAnyModel &m, double x) { return m.trees ? vsc_eff_trees_link(m.trees, x) : vsc_eff_link(m.linear, x); }

inline int eff_any_score(vsc_ctx *ctx, const vsc_genome *genome, vsc_guides *g, const EffAnyModel &m, double *linear)
{
    return m.trees ? vsc_guides_efficiency_trees(ctx, genome, g, m.trees, linear, nullptr) : vsc_guides_efficiency(ctx, genome, g, m.linear, linear, nullptr);
}
inline int eff_any_score(vsc_ctx *ctx, const vsc_genome *genome, vsc_pattern_guides *g, const EffAnyModel &m, double *linear)
{
    return m.trees ? vsc_pattern_guides_efficiency_trees(ctx, genome, g, m.trees, linear, nullptr)
                   : vsc_pattern_guides_efficiency(ctx, genome, g, m.linear, linear, nullptr);
}
inline int eff_any_filter(vsc_ctx *ctx, const vsc_genome *genome, vsc_guides *in, const EffAnyModel &m, double floor, vsc_guides **out)
{
    return m.trees ? vsc_guides_filter_efficiency_trees(ctx, genome, in, m.trees, floor, out) : vsc_guides_filter_efficiency(ctx, genome, in, m.linear, floor, out);
}
inline int eff_any_filter(vsc_ctx *ctx, const vsc_genome *genome, vsc_pattern_guides *in, const EffAnyModel &m, double floor, vsc_pattern_guides **out)
{
    return m.trees ? vsc_pattern_guides_filter_efficiency_trees(ctx, genome, in, m.trees, floor, out)
                   : vsc_pattern_guides_filter_efficiency(ctx, genome, in, m.linear, floor, out);
}

}  // namespace vsc_host
