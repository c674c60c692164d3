// variation_check.cpp - the variation functions of varscot_amd/csrc/vsc_variation.h (var_shape_valid, var_site, var_first_reach,
// var_first, var_touch, var_add, var_row, var_row_counts, var_keep and what they call) in a stand-alone program with its own main,
// for the host sanitizers.  No device is opened and no kernel is launched.  Build and run on the CPU:
//   hipcc --offload-arch=gfx950 -x hip -O1 -g -std=c++17 -Iinclude -Ivarscot_amd/csrc -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tools/variation_check.cpp -o build/variation_check && build/variation_check
//   - a small genome (contigs of site_len - 1, site_len, site_len + 1, 900 with an N run, and 300 bases, one N apart) packed into
//     plane arrays of exactly the held words: every (contig, position, strand) and the loci the definition calls invalid,
//     site_len 16, 23 and 32, the whole genome and a view that starts at word 1 and ends one word early;
//   - variant sets in heap arrays of exactly n_v records: none, one, every position with three alts (ties), every third
//     position, deletions of span 1 .. 40 that end at, start at and cover one base of a site's edges, a span of 700 bases with
//     short variants under it, 300 records at one position, two weights of 0xFFFFFFFE; the block table in an array of exactly
//     n_blocks + 1 entries at blocks of 16, 256 and 2^32 positions;
//   - against a naive loop: per site every variant of the array, the touched read positions one base at a time, the top zone
//     and the accepted letters read from per-position arrays.
// Exit code 0 and "ok" when all agree.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "vsc_variation.h"

using namespace vsc;

static int code(char c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 4; }

static std::string random_text(size_t n)
{
    std::string t(n, 'A');
    for (char &c : t) c = "ACGT"[std::rand() % 4];
    return t;
}

struct Variant {
    uint32_t contig, pos, span, alt, weight;
};

int main()
{
    std::srand(32);
    unsigned long long loci = 0, defined = 0, disrupted = 0, pairs = 0, silent_pairs = 0, saturated = 0, clamped = 0, classes[kEffClasses] = {};
    for (uint32_t site_len : {16u, 23u, 32u}) {
        const uint32_t lens[5] = {site_len - 1, site_len, site_len + 1, 900, 300};
        std::vector<std::string> contig;
        std::vector<uint32_t> off, end;
        std::string genome;
        for (uint32_t len : lens) {
            std::string t = random_text(len);
            if (len == 900) t.replace(100, 3, "NNN");
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
        // the shape: labels and accepted letters per read position, random, and their packed form
        std::vector<uint32_t> zone(site_len), accept(site_len);
        VarShape s{site_len, 0, {0, 0}};
        for (uint32_t j = 0; j < site_len; ++j) {
            zone[j] = (uint32_t)std::rand() % 4;
            accept[j] = std::rand() % 3 ? 0u : (uint32_t)std::rand() % 16;
            s.zones |= (uint64_t)zone[j] << (2 * j);
            s.accept[j >> 4] |= (uint64_t)accept[j] << (4 * (j & 15));
        }
        if (!var_shape_valid(s)) return 3;
        // the variant sets, ascending (contig, pos) with ties
        std::vector<std::vector<Variant>> sets(8);
        sets[1].push_back({3, 154, 1, 2, 7});
        for (uint32_t c = 0; c < contig.size(); ++c)
            for (uint32_t p = 0; p < contig[c].size(); ++p) {
                for (uint32_t a = 0; a < 3; ++a) sets[2].push_back({c, p, 1, (p + a) % 4, 2 + a});
                if (p % 3 == 0 || p + 1 == contig[c].size()) sets[3].push_back({c, p, 1, p % 5 == 4 ? 4u : p % 4, 1 + p % 5});
            }
        for (uint32_t p = 160; p <= 200 + site_len + 1; ++p)  // (by position, so that the set is ascending)
            for (uint32_t span = 1; span <= 40; ++span)
                if (p + span == 200 || p == 200 + site_len || p + span == 201 || p == 200 + site_len - 1) sets[4].push_back({3, p, span, 4, span});
        sets[5].push_back({3, 50, 700, 4, 5});
        for (uint32_t p = 60; p < 880; p += 37) sets[5].push_back({3, p, p % 2 ? 1u : 9u, p % 2 ? p % 4 : 4u, 8});
        for (uint32_t k = 0; k < 300; ++k) sets[6].push_back({3, 420, 1, 4, 1});
        sets[7] = {{3, 500, 2, 4, kVarMaxCount}, {3, 501, 1, 4, kVarMaxCount}, {3, 502, 1, 0, 5}};
        for (const auto &set : sets) {
            const uint32_t n_v = (uint32_t)set.size();
            std::unique_ptr<VarRec[]> rec(new VarRec[n_v]);  // exactly the held size: the sanitizer sees one element too far
            uint32_t reach = 0;
            for (uint32_t k = 0; k < n_v; ++k) {
                const uint32_t gpos = off[set[k].contig] + set[k].pos;
                if (k && (set[k - 1].contig > set[k].contig || (set[k - 1].contig == set[k].contig && set[k - 1].pos > set[k].pos))) return 4;
                if (set[k].pos + set[k].span > contig[set[k].contig].size()) return 5;
                if (gpos + set[k].span > reach) reach = gpos + set[k].span;
                rec[k] = VarRec{gpos, set[k].span | set[k].alt << 16, set[k].weight, reach};
            }
            for (uint32_t bits : {4u, 8u, 32u}) {
                const uint32_t n_blocks = n_v ? var_block_count(genome.size(), bits) : 0u;
                std::unique_ptr<uint32_t[]> first(new uint32_t[n_blocks + 1]);
                for (uint64_t b = 0; b <= n_blocks; ++b) first[b] = var_first_reach(rec.get(), 0u, n_v, b << bits);
                const VarTable t{rec.get(), first.get(), n_v, bits, n_blocks};
                for (int view = 0; view < (bits == 8u ? 2 : 1); ++view) {  // the whole genome; words [1, words - 1) in arrays of exactly that length
                    const uint64_t first_word = view ? 1 : 0, held = words - 2 * first_word;
                    const std::vector<uint32_t> vh(hi.begin() + first_word, hi.begin() + first_word + held),
                        vl(lo.begin() + first_word, lo.begin() + first_word + held), vn(nm.begin() + first_word, nm.begin() + first_word + held);
                    const EffPlanes g{vh.data(), vl.data(), vn.data(), first_word, held, held, off.data(), end.data(), (uint32_t)contig.size()};
                    auto check = [&](uint32_t c, uint32_t p, uint32_t strand) -> int {
                        uint32_t want = kEffDefined;
                        if (c >= contig.size() || strand > 1 || (uint64_t)p + site_len > contig[c].size()) want = kEffInvalid;
                        else {
                            const uint64_t g0 = (uint64_t)off[c] + p;
                            if (g0 < first_word * 32 || g0 + site_len > (first_word + held) * 32) want = kEffNotResident;
                            else if (contig[c].substr(p, site_len).find('N') != std::string::npos) want = kEffHasN;
                        }
                        const uint32_t got = var_site(g, s, c, p, strand);
                        if (got != want) return 6;
                        ++loci;
                        ++classes[got];
                        if (got != kEffDefined) return var_keep(got, 0, 0, VarFilter{0xFFFFFFFFu, 0xFFFFFFFFu, 0}) ? 7 : 0;
                        ++defined;
                        // the naive loop
                        unsigned long long by[4] = {}, n_silent = 0, cost = 0, n_pairs = 0;
                        uint32_t largest = 0;
                        std::vector<uint32_t> want_k, want_info;
                        for (uint32_t k = 0; k < n_v; ++k) {
                            if (set[k].contig != c) continue;
                            uint32_t touched = 0, j_min = site_len, top = 0;
                            for (uint32_t f = set[k].pos; f < set[k].pos + set[k].span; ++f) {
                                if (f < p || f >= p + site_len) continue;
                                const uint32_t j = strand ? site_len - 1 - (f - p) : f - p;
                                ++touched;
                                if (j < j_min) j_min = j;
                                if (zone[j] > top) top = zone[j];
                            }
                            if (!touched) continue;
                            const bool silent = set[k].alt < 4 && (accept[j_min] >> (strand ? 3 - set[k].alt : set[k].alt) & 1u);
                            want_k.push_back(k);
                            want_info.push_back(j_min | touched << 8 | top << 16 | (uint32_t)silent << 18);
                            ++n_pairs;
                            if (silent) {
                                ++n_silent;
                                continue;
                            }
                            ++by[top];
                            cost += set[k].weight;
                            if (set[k].weight > largest) largest = set[k].weight;
                        }
                        const uint32_t g0 = off[c] + p;
                        const uint32_t k0 = var_first(t, g0);
                        if (k0 > n_v || (k0 < n_v && rec[k0].reach <= g0) || (k0 > 0 && rec[k0 - 1].reach > g0)) return 8;
                        uint64_t walked = 0;
                        const VarRow row = var_row(t, g0, strand, s, &walked);
                        uint32_t want_by = 0;
                        for (uint32_t z = 0; z < 4; ++z) want_by |= (uint32_t)(by[z] > 255 ? 255 : by[z]) << (8 * z);
                        if (row.by_zone != want_by || row.silent != n_silent || row.cost != cost || row.max_weight != largest || walked != n_pairs) return 9;
                        if (var_cost(row) != (cost > kVarMaxCount ? kVarMaxCount : (uint32_t)cost)) return 10;
                        const bool counts = var_row_counts(row.by_zone);
                        if (counts != (by[0] < 255 && by[1] < 255 && by[2] < 255 && by[3] < 255)) return 11;
                        if (counts && (row.by_zone & 255u) + (row.by_zone >> 8 & 255u) + (row.by_zone >> 16 & 255u) + (row.by_zone >> 24) + row.silent != n_pairs)
                            return 12;
                        // the pairs' walk: ascending variant, every overlapping one once
                        size_t at = 0;
                        for (uint32_t k = k0; k < n_v; ++k) {
                            if (rec[k].gpos >= g0 + site_len) break;
                            uint32_t info;
                            if (!var_touch(rec[k], g0, strand, s, &info)) continue;
                            if (at >= want_k.size() || want_k[at] != k || want_info[at] != info) return 13;
                            ++at;
                        }
                        if (at != want_k.size()) return 14;
                        pairs += n_pairs;
                        silent_pairs += n_silent;
                        disrupted += want_by != 0;
                        saturated += !counts;
                        clamped += cost > kVarMaxCount;
                        // FILTER
                        for (uint32_t max_cost : {0u, 5u, 0xFFFFFFFFu})
                            for (uint32_t bounds : {0xFFFFFFFFu, 0xFF00FFFFu, 0x0000FF01u})
                                for (uint32_t require : {0u, 8u, 12u, 1u}) {
                                    bool keep = (cost > kVarMaxCount ? kVarMaxCount : cost) <= max_cost, any = require == 0;
                                    for (uint32_t z = 0; z < 4; ++z) {
                                        if ((by[z] > 255 ? 255 : by[z]) > (bounds >> (8 * z) & 255u)) keep = false;
                                        if ((require >> z & 1u) && by[z]) any = true;
                                    }
                                    if (var_keep(got, row.by_zone, var_cost(row), VarFilter{max_cost, bounds, require}) != (keep && any)) return 15;
                                }
                        return 0;
                    };
                    for (uint32_t c = 0; c < contig.size(); ++c)
                        for (uint32_t p = 0; p <= contig[c].size() + 2; ++p)  // (the last starts leave the contig: invalid)
                            for (uint32_t strand = 0; strand < 2; ++strand)
                                if (const int rc = check(c, p, strand)) return rc;
                    const uint32_t bad[][3] = {{5, 0, 0}, {0xFFFFFFFFu, 0, 0}, {3, 10, 2}, {3, 900 - site_len + 1, 0}, {3, 0xFFFFFFFFu, 1},
                                               {4, 0xFFFFFFF0u, 0}, {3, 10, 0xFFFFFFFFu}};
                    for (const auto &b : bad)
                        if (var_site(g, s, b[0], b[1], b[2]) != kEffInvalid) return 16;
                }
            }
        }
    }
    // the shapes the definition refuses, and the largest it takes
    const VarShape refused[] = {{15, 0, {0, 0}}, {33, 0, {0, 0}}, {0xFFFFFFFFu, 0, {0, 0}}, {23, 1ull << 46, {0, 0}}, {16, 1ull << 32, {0, 0}},
                                {23, 0, {0, 1ull << 28}}, {16, 0, {0, 1}}, {31, 1ull << 62, {0, 0}}, {31, 0, {0, 1ull << 60}}};
    for (const VarShape &r : refused)
        if (var_shape_valid(r)) return 17;
    if (!var_shape_valid(VarShape{32, ~0ull, {~0ull, ~0ull}}) || !var_shape_valid(VarShape{16, 0xFFFFFFFFull, {~0ull, 0}}) ||
        !var_shape_valid(VarShape{23, (1ull << 46) - 1, {~0ull, (1ull << 28) - 1}}))
        return 18;
    if (classes[kEffOffContig] != 0) return 19;  // cannot occur
    for (uint32_t k : {(uint32_t)kEffDefined, (uint32_t)kEffInvalid, (uint32_t)kEffNotResident, (uint32_t)kEffHasN})
        if (classes[k] == 0) return 20;
    if (!disrupted || !pairs || !silent_pairs || !saturated || !clamped) return 21;
    std::printf("ok: %llu loci (%llu defined, %llu with a disrupting variant), %llu pairs (%llu silent), %llu saturated rows, %llu clamped costs\n", loci,
                defined, disrupted, pairs, silent_pairs, saturated, clamped);
    return 0;
}
