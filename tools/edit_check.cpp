// edit_check.cpp - the base-editor window functions of varscot_amd/csrc/vsc_edit.h (edit_shape_valid, edit_site, edit_mask,
// edit_forward, edit_first_target, edit_hits, edit_pair_info, edit_keep and what they call) in a stand-alone program with its
// own main, for the host sanitizers.  No device is opened and no kernel is launched.  Build and run on the CPU:
//   hipcc --offload-arch=gfx950 -x hip -O1 -g -std=c++17 -Iinclude -Ivarscot_amd/csrc -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tools/edit_check.cpp -o build/edit_check && build/edit_check
//   - a small genome (contigs of site_len - 1, site_len, site_len + 1, 300 with an N run, a run of 16 C and a run of 16 A, and
//     150 bases, one N apart) packed into plane arrays of exactly the held words: every (contig, position, strand) and the loci
//     the definition calls invalid, site_len 16, 23 and 32, windows at both ends of the site, win_len 1 and 16, all four bases,
//     the whole genome and a view that starts at word 1 and ends one word early;
//   - target sets in heap arrays of exactly n_t entries: none, every position, every third, one, the first and last base of
//     every contig;
//   - against a restatement on strings: the site by slicing and reverse complement, the mask letter by letter, the hits by
//     looking (contig, forward position) up in a std::set.
// Exit code 0 and "ok" when all agree.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "vsc_edit.h"

using namespace vsc;

static int code(char c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 4; }

static std::string revcomp(const std::string &s)
{
    std::string r(s.rbegin(), s.rend());
    for (char &c : r) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : 'N';
    return r;
}

static std::string random_text(size_t n)
{
    std::string t(n, 'A');
    for (char &c : t) c = "ACGT"[std::rand() % 4];
    return t;
}

int main()
{
    std::srand(28);
    unsigned long long loci = 0, defined = 0, with_hit = 0, pairs = 0, full = 0, empty = 0, classes[kEffClasses] = {};
    for (uint32_t site_len : {16u, 23u, 32u}) {
        const uint32_t lens[5] = {site_len - 1, site_len, site_len + 1, 300, 150};
        std::vector<std::string> contig;
        std::vector<uint32_t> off, end;
        std::string genome;
        for (uint32_t len : lens) {
            std::string t = random_text(len);
            if (len == 300) {
                t.replace(100, 3, "NNN");
                t.replace(140, 16, std::string(16, 'C'));
                t.replace(200, 16, std::string(16, 'A'));
            }
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
        // the target sets, as (contig, pos) and as global positions in an array of exactly n_t entries
        std::vector<std::set<std::pair<uint32_t, uint32_t>>> sets(5);
        for (uint32_t c = 0; c < contig.size(); ++c)
            for (uint32_t p = 0; p < contig[c].size(); ++p) {
                sets[1].insert({c, p});
                if (p % 3 == 0) sets[2].insert({c, p});
                if (p == 0 || p + 1 == contig[c].size()) sets[4].insert({c, p});
            }
        sets[3].insert({3, 147});
        const uint32_t windows[][2] = {{0, 1}, {0, 16}, {site_len - 1, 1}, {site_len - 16, 16}, {3, 5}, {3, 4}};
        for (const auto &w : windows)
            for (uint32_t from = 0; from < 4; ++from) {
                const EditShape s{site_len, w[0], w[1], from};
                if (!edit_shape_valid(s)) return 3;
                for (const auto &set : sets) {
                    const uint32_t n_t = (uint32_t)set.size();
                    std::unique_ptr<uint32_t[]> gpos(new uint32_t[n_t]);  // exactly the held size: the sanitizer sees one element too far
                    uint32_t k = 0;
                    for (const auto &t : set) gpos[k++] = off[t.first] + t.second;
                    const EditTargets tg{gpos.get(), n_t};
                    for (int view = 0; view < 2; ++view) {  // the whole genome; words [1, words - 1) in arrays of exactly that length
                        const uint64_t first = view ? 1 : 0, held = words - 2 * first;
                        const std::vector<uint32_t> vh(hi.begin() + first, hi.begin() + first + held), vl(lo.begin() + first, lo.begin() + first + held),
                            vn(nm.begin() + first, nm.begin() + first + held);
                        const EffPlanes g{vh.data(), vl.data(), vn.data(), first, held, held, off.data(), end.data(), (uint32_t)contig.size()};
                        auto check = [&](uint32_t c, uint32_t p, uint32_t strand) -> int {
                            uint32_t want = kEffDefined;
                            std::string text;
                            if (c >= contig.size() || strand > 1 || (uint64_t)p + site_len > contig[c].size()) want = kEffInvalid;
                            else {
                                const uint64_t g0 = (uint64_t)off[c] + p;
                                if (g0 < first * 32 || g0 + site_len > (first + held) * 32) want = kEffNotResident;
                                else {
                                    text = contig[c].substr(p, site_len);
                                    if (text.find('N') != std::string::npos) want = kEffHasN;
                                    else if (strand) text = revcomp(text);
                                }
                            }
                            uint64_t h = 0, l = 0;
                            const uint32_t got = edit_site(g, s, c, p, strand, &h, &l);
                            if (got != want) return 4;
                            ++loci;
                            ++classes[got];
                            if (got != kEffDefined) return edit_keep(got, 0, 0, 0, 16, false) ? 5 : 0;
                            ++defined;
                            uint32_t want_mask = 0, want_hits = 0;
                            for (uint32_t j = 0; j < s.win_len; ++j) {
                                if (text[s.win_start + j] != "ACGT"[from]) continue;
                                want_mask |= 1u << j;
                                const uint32_t fwd = strand ? p + site_len - 1 - (s.win_start + j) : p + s.win_start + j;
                                if (edit_forward(p, strand, s, j) != fwd) return 6;
                                // a hit's forward letter is `from` on '+' and its complement on '-'
                                if (set.count({c, fwd})) {
                                    want_hits |= 1u << j;
                                    if (contig[c][fwd] != (strand ? "TGCA"[from] : "ACGT"[from])) return 7;
                                }
                            }
                            const uint32_t mask = edit_mask(h, l, s);
                            if (mask != want_mask) return 8;
                            const uint32_t g0 = off[c] + edit_window_first(p, strand, s);
                            const uint32_t k0 = edit_first_target(tg, g0);
                            if (k0 > n_t || (k0 < n_t && gpos[k0] < g0) || (k0 > 0 && gpos[k0 - 1] >= g0)) return 9;
                            const uint32_t hits = edit_hits(mask, k0, tg, g0, strand, s);
                            if (hits != want_hits) return 10;
                            // the pairs' walk: ascending target, every set bit of hits once, info = at | bystanders << 8
                            uint32_t seen = 0, last = 0;
                            for (uint32_t t = k0; t - k0 < s.win_len; ++t) {
                                const uint32_t j = edit_target_at(tg, t, g0, strand, s);
                                if (j >= s.win_len) break;
                                if (!(hits >> j & 1u)) continue;
                                if (seen && t <= last) return 11;
                                if (seen >> j & 1u) return 12;
                                seen |= 1u << j;
                                last = t;
                                const uint32_t info = edit_pair_info(mask, j);
                                if ((info & 0xFFu) != j || (info >> 8) + 1u != (uint32_t)__builtin_popcount(want_mask)) return 13;
                                if (gpos[t] != off[c] + edit_forward(p, strand, s, j)) return 14;
                                ++pairs;
                            }
                            if (seen != hits) return 15;
                            with_hit += hits != 0;
                            full += mask == 0xFFFFu;
                            empty += mask == 0;
                            const uint32_t e = (uint32_t)__builtin_popcount(want_mask);
                            for (uint32_t lo_e : {0u, 1u, 2u})
                                for (uint32_t hi_e : {0u, 1u, 16u}) {
                                    const bool want_keep = e >= lo_e && e <= hi_e && (n_t == 0 || want_hits != 0);
                                    if (edit_keep(got, mask, hits, lo_e, hi_e, n_t != 0) != want_keep) return 16;
                                }
                            return 0;
                        };
                        for (uint32_t c = 0; c < contig.size(); ++c)
                            for (uint32_t p = 0; p <= contig[c].size() + 2; ++p)  // (the last starts leave the contig: invalid)
                                for (uint32_t strand = 0; strand < 2; ++strand)
                                    if (const int rc = check(c, p, strand)) return rc;
                        const uint32_t bad[][3] = {{5, 0, 0}, {0xFFFFFFFFu, 0, 0}, {3, 10, 2}, {3, 300 - site_len + 1, 0}, {3, 0xFFFFFFFFu, 1},
                                                   {4, 0xFFFFFFF0u, 0}, {3, 10, 0xFFFFFFFFu}};
                        for (const auto &b : bad) {
                            uint64_t h, l;
                            if (edit_site(g, s, b[0], b[1], b[2], &h, &l) != kEffInvalid) return 17;
                        }
                    }
                }
            }
    }
    // the shapes the definition refuses
    const EditShape refused[] = {{15, 3, 5, 1}, {33, 3, 5, 1}, {23, 3, 0, 1}, {23, 3, 17, 1}, {23, 19, 5, 1}, {23, 24, 1, 1}, {23, 3, 5, 4},
                                 {23, 0xFFFFFFFFu, 2, 1}, {23, 3, 0xFFFFFFFFu, 1}, {23, 3, 5, 0xFFFFFFFFu}, {0xFFFFFFFFu, 3, 5, 1}};
    for (const EditShape &s : refused)
        if (edit_shape_valid(s)) return 18;
    if (!edit_shape_valid(EditShape{23, 22, 1, 2}) || !edit_shape_valid(EditShape{16, 0, 16, 0}) || !edit_shape_valid(EditShape{32, 16, 16, 3})) return 19;
    if (classes[kEffOffContig] != 0) return 20;  // cannot occur
    for (uint32_t k : {(uint32_t)kEffDefined, (uint32_t)kEffInvalid, (uint32_t)kEffNotResident, (uint32_t)kEffHasN})
        if (classes[k] == 0) return 21;
    if (!with_hit || !pairs || !full || !empty) return 22;
    std::printf("ok: %llu loci (%llu defined, %llu with a hit), %llu pairs, %llu full masks, %llu empty masks\n", loci, defined, with_hit, pairs,
                full, empty);
    return 0;
}
