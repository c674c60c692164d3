// prime_check.cpp - the prime-editing functions of varscot_amd/csrc/vsc_prime.h (prime_shape_valid, prime_context, prime_pbs,
// prime_reach, prime_cells_occupied, prime_first_edit, prime_read, prime_edited, prime_rtt, prime_flags, prime_pair, prime_walk,
// prime_keep and what they call) in a stand-alone program with its own main, for the host sanitizers.  No device is opened and
// no kernel is launched.  Build and run on the CPU:
//   hipcc --offload-arch=gfx950 -x hip -O1 -g -std=c++17 -Iinclude -Ivarscot_amd/csrc -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tools/prime_check.cpp -o build/prime_check && build/prime_check
//   - a small genome (contigs of site_len - 1, C - 1, C, C + 1, 400 with an N run and runs of A, T, G and C, and 200 bases, one N
//     apart) packed into plane arrays of exactly the held words: every (contig, position, strand) and the loci the definition
//     calls invalid, several shapes (site_len 16, 23, 32; down 0 and the largest; nick at 1 and at site_len; a stability model;
//     AVOID_G_END on and off), the whole genome and a view that starts at word 1 and ends one word early;
//   - edit sets in heap arrays of exactly n_e entries, with a bitmap of exactly its words and without one: none, an SNV at every
//     position, and insertions, deletions and replacements of 1 to 16 letters in turn with edits at the first base, at the end
//     (an insertion at pos = length) and ending at the end of every contig;
//   - against a brute-force walk on letters: the context by slicing and reverse complement, the edit applied to the forward
//     text, the primer binding site, the template, the flags and the extension's G/C read off the strings, every edit of the
//     candidate's contig tried.
// Exit code 0 and "ok" when all agree.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "vsc_prime.h"

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

struct TextEdit {
    uint32_t contig, pos, del;
    std::string ins;
};

struct Pair {
    uint32_t edit, info, ext;
};

static PrimeShape make_shape(uint32_t site_len, uint32_t down, uint32_t nick, uint32_t pbs_min, uint32_t pbs_max, uint32_t rtt_min,
                             uint32_t rtt_max, uint32_t hom, uint32_t pam_start, uint32_t pam_len, uint32_t seed_start, uint32_t seed_len,
                             uint32_t flags, bool model)
{
    PrimeShape s{};
    s.site_len = site_len, s.down = down, s.nick = nick, s.pbs_min = pbs_min, s.pbs_max = pbs_max, s.rtt_min = rtt_min, s.rtt_max = rtt_max;
    s.min_homology = hom, s.pam_start = pam_start, s.pam_len = pam_len, s.seed_start = seed_start, s.seed_len = seed_len, s.flags = flags;
    if (model) {
        const int32_t mono[4] = {2, 3, 3, 2};
        for (int k = 0; k < 4; ++k) s.mono[k] = mono[k];
        for (int a = 0; a < 4; ++a)
            for (int b = 0; b < 4; ++b) s.di[4 * a + b] = (a == 1 || a == 2) && (b == 1 || b == 2) ? 1 : (a + b == 3 && (a == 0 || a == 3)) ? -1 : 0;
        s.init = -1;
        s.target = 2 * (int32_t)pbs_max + 4;
    }
    return s;
}

int main()
{
    std::srand(30);
    unsigned long long loci = 0, defined = 0, with_pair = 0, pairs = 0, weak = 0, lengthened = 0, by_flag[kPrimeFlags] = {}, classes[kEffClasses] = {};
    unsigned long long no_g_end = 0, past_end = 0, over_max = 0;
    const PrimeShape shapes[] = {
        make_shape(23, 41, 17, 13, 13, 10, 34, 5, 21, 2, 17, 3, kPrimeAvoidGEnd, false),
        make_shape(23, 20, 17, 8, 15, 5, 20, 3, 21, 2, 17, 3, 0, true),
        make_shape(16, 0, 8, 4, 8, 2, 8, 1, 13, 3, 8, 4, kPrimeAvoidGEnd, false),
        make_shape(32, 32, 32, 10, 17, 8, 32, 0, 0, 0, 24, 8, kPrimeAvoidGEnd, true),
        make_shape(23, 0, 1, 1, 1, 1, 22, 2, 21, 2, 0, 8, 0, false),
        make_shape(20, 44, 10, 5, 10, 20, 54, 5, 17, 3, 10, 0, kPrimeAvoidGEnd, true),
    };
    for (const PrimeShape &s : shapes) {
        if (!prime_shape_valid(s)) return 3;
        const uint32_t C = prime_context_len(s), site_len = s.site_len, nick = s.nick;
        const uint32_t lens[6] = {site_len - 1, C - 1, C, C + 1, 400, 200};
        std::vector<std::string> contig;
        std::vector<uint32_t> off, end;
        std::string genome;
        for (uint32_t len : lens) {
            std::string t = random_text(len);
            if (len == 400) {
                t.replace(60, 3, "NNN");
                t.replace(100, 9, std::string(9, 'A'));
                t.replace(140, 9, std::string(9, 'T'));
                t.replace(180, 30, std::string(30, 'G'));
                t.replace(240, 30, std::string(30, 'C'));
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
        // the edit sets as text, ascending (contig, pos), one edit per position
        std::vector<std::vector<TextEdit>> sets(3);
        const uint32_t kinds[7][2] = {{0, 1}, {0, 3}, {0, 16}, {1, 0}, {3, 0}, {16, 0}, {3, 2}};
        uint32_t turn = 0;
        for (uint32_t c = 0; c < contig.size(); ++c) {
            const uint32_t len = (uint32_t)contig[c].size();
            for (uint32_t p = 0; p <= len; ++p) {
                if (p < len) sets[1].push_back({c, p, 1, std::string(1, "ACGT"[(code(contig[c][p]) + 1 + p % 3) % 4])});
                if (p == 0) sets[2].push_back({c, p, 1, "G"});
                else if (p == len) sets[2].push_back({c, p, 0, "TAC"});
                else if (p == len - 3) sets[2].push_back({c, p, 3, ""});
                else if (p == len - 1) sets[2].push_back({c, p, 1, "C"});
                else if (p % 5 == 2 && p + 20 < len) {
                    const uint32_t *k = kinds[turn++ % 7];
                    sets[2].push_back({c, p, k[0], random_text(k[1])});
                }
            }
        }
        for (const auto &set : sets) {
            const uint32_t n_e = (uint32_t)set.size();
            // exactly the held sizes: the sanitizer sees one element too far
            std::unique_ptr<uint32_t[]> gpos(new uint32_t[n_e]);
            std::unique_ptr<PrimeEdit[]> rec(new PrimeEdit[n_e]);
            const uint32_t map_words = ((end.back() >> kPrimeCellShift) + 32) / 32;
            std::unique_ptr<uint32_t[]> bitmap(new uint32_t[map_words]());
            for (uint32_t k = 0; k < n_e; ++k) {
                uint32_t ins = 0;
                for (size_t j = 0; j < set[k].ins.size(); ++j) ins |= (uint32_t)code(set[k].ins[j]) << (2 * j);
                rec[k] = PrimeEdit{set[k].contig, set[k].pos, set[k].del | (uint32_t)set[k].ins.size() << 16, ins};
                if (!prime_edit_valid(rec[k], (uint32_t)contig[set[k].contig].size())) return 4;
                gpos[k] = off[set[k].contig] + set[k].pos;
                bitmap[(gpos[k] >> kPrimeCellShift) >> 5] |= 1u << ((gpos[k] >> kPrimeCellShift) & 31u);
            }
            for (int view = 0; view < 2; ++view) {  // the whole genome; words [1, words - 1) in arrays of exactly that length
                const uint64_t first = view ? 1 : 0, held = words - 2 * first;
                const std::vector<uint32_t> vh(hi.begin() + first, hi.begin() + first + held), vl(lo.begin() + first, lo.begin() + first + held),
                    vn(nm.begin() + first, nm.begin() + first + held);
                const EffPlanes g{vh.data(), vl.data(), vn.data(), first, held, held, off.data(), end.data(), (uint32_t)contig.size()};
                auto check = [&](uint32_t c, uint32_t p, uint32_t strand) -> int {
                    uint32_t want = kEffDefined;
                    std::string R;
                    uint32_t F0 = 0;
                    if (c >= contig.size() || strand > 1 || (uint64_t)p + site_len > contig[c].size()) want = kEffInvalid;
                    else if (strand ? p < s.down : (uint64_t)p + C > contig[c].size()) want = kEffOffContig;
                    else {
                        F0 = strand ? p - s.down : p;
                        const uint64_t g0 = (uint64_t)off[c] + F0;
                        if (g0 < first * 32 || g0 + C > (first + held) * 32) want = kEffNotResident;
                        else {
                            R = contig[c].substr(F0, C);
                            if (R.find('N') != std::string::npos) want = kEffHasN;
                            else if (strand) R = revcomp(R);
                        }
                    }
                    uint64_t h = 0, l = 0;
                    const uint32_t got = prime_context(g, s, c, p, strand, &h, &l);
                    if (got != want) return 5;
                    ++loci;
                    ++classes[got];
                    if (got != kEffDefined) return prime_keep(got, 0, 1, false, true) ? 6 : 0;
                    ++defined;
                    if (prime_first_forward(p, strand, s) != F0) return 7;
                    // PBS on letters
                    uint32_t pbs_len = 0;
                    for (uint32_t L = s.pbs_min; L <= s.pbs_max && !pbs_len; ++L) {
                        int32_t sum = s.init;
                        for (uint32_t j = nick - L; j < nick; ++j) sum += s.mono[code(R[j])];
                        for (uint32_t j = nick - L; j + 1 < nick; ++j) sum += s.di[4 * code(R[j]) + code(R[j + 1])];
                        if (sum >= s.target) pbs_len = L;
                    }
                    const uint32_t is_weak = pbs_len ? 0u : 1u;
                    if (!pbs_len) pbs_len = s.pbs_max;
                    uint32_t pbs_gc = 0;
                    for (uint32_t j = nick - pbs_len; j < nick; ++j) pbs_gc += R[j] == 'G' || R[j] == 'C';
                    const uint32_t pbs = prime_pbs(h, l, s, s.mono, s.di);
                    if (pbs != (pbs_len | pbs_gc << 8 | is_weak << 16)) return 8;
                    weak += is_weak;
                    // every edit of the set, by brute force
                    std::vector<Pair> want_pairs;
                    const std::string forward = strand ? revcomp(R) : R;
                    for (uint32_t k = 0; k < n_e; ++k) {
                        const TextEdit &e = set[k];
                        if (e.contig != c || e.pos < F0 || e.pos - F0 + e.del > C) continue;
                        const uint32_t f = e.pos - F0;
                        const uint32_t e0 = strand ? C - f - e.del : f;
                        if (e0 < nick) continue;
                        const std::string fe = forward.substr(0, f) + e.ins + forward.substr(f + e.del);
                        const std::string E = strand ? revcomp(fe) : fe;
                        const uint32_t d = e0 - nick, ins_len = (uint32_t)e.ins.size();
                        const uint32_t t0 = std::max(s.rtt_min, d + ins_len + s.min_homology);
                        uint32_t t = t0;
                        if (s.flags & kPrimeAvoidGEnd)
                            while (nick + t - 1 < E.size() && E[nick + t - 1] == 'G') ++t;
                        if (t0 > s.rtt_max) {
                            ++over_max;
                            continue;
                        }
                        if (t > s.rtt_max) {
                            ++no_g_end;
                            continue;
                        }
                        if (nick + t > E.size()) {
                            ++past_end;
                            continue;
                        }
                        lengthened += t > t0;
                        uint32_t flags = is_weak ? (uint32_t)kPrimeWeak : 0u;
                        for (uint32_t q = s.pam_start; q < s.pam_start + s.pam_len; ++q)
                            if (q >= E.size() || E[q] != R[q]) flags |= kPrimePam;
                        for (uint32_t q = s.seed_start; q < s.seed_start + s.seed_len; ++q)
                            if (q >= E.size() || E[q] != R[q]) flags |= kPrimeSeed;
                        const std::string body = E.substr(nick - pbs_len, pbs_len + t);
                        if (body.find("AAAA") != std::string::npos) flags |= kPrimePolyT;
                        uint32_t gc = 0;
                        for (char ch : body) gc += ch == 'G' || ch == 'C';
                        want_pairs.push_back({k, t | d << 8 | (t - d - ins_len) << 16 | flags << 24, (pbs_len + t) | gc << 8 | pbs_len << 16});
                        // E as planes, letter by letter
                        uint32_t r0;
                        uint64_t ih, il, eh, el;
                        if (!prime_read(s, strand, f, rec[k], &r0, &ih, &il) || r0 != e0) return 9;
                        if (prime_edited(s, h, l, e0, e.del, ins_len, ih, il, &eh, &el) != E.size()) return 10;
                        for (uint32_t q = 0; q < 64; ++q) {
                            const uint32_t b = (uint32_t)(eh >> q & 1u) << 1 | (uint32_t)(el >> q & 1u);
                            if (b != (q < E.size() ? (uint32_t)code(E[q]) : 0u)) return 11;
                        }
                    }
                    const uint32_t g0 = off[c] + F0;
                    for (int with_map = 0; with_map < 2; ++with_map) {
                        const PrimeEdits pe{gpos.get(), rec.get(), with_map ? bitmap.get() : nullptr, n_e};
                        std::vector<Pair> got_pairs;
                        const uint32_t n = prime_walk(s, pe, h, l, c, g0, strand, pbs, [&](uint32_t k, uint32_t info, uint32_t ext, uint64_t, uint64_t) {
                            got_pairs.push_back({k, info, ext});
                        });
                        if (n != got_pairs.size() || n != want_pairs.size()) return 12;
                        for (uint32_t k = 0; k < n; ++k)
                            if (got_pairs[k].edit != want_pairs[k].edit || got_pairs[k].info != want_pairs[k].info || got_pairs[k].ext != want_pairs[k].ext)
                                return 13;
                    }
                    if (want_pairs.size() > C - nick + 1) return 14;
                    pairs += want_pairs.size();
                    with_pair += !want_pairs.empty();
                    for (const Pair &q : want_pairs)
                        for (uint32_t b = 0; b < kPrimeFlags; ++b) by_flag[b] += q.info >> (24 + b) & 1u;
                    const uint32_t np = (uint32_t)want_pairs.size();
                    for (int have = 0; have < 2; ++have)
                        for (int allow = 0; allow < 2; ++allow)
                            if (prime_keep(got, pbs, np, have != 0, allow != 0) != ((!have || np >= 1) && (allow || !is_weak))) return 15;
                    return 0;
                };
                for (uint32_t c = 0; c < contig.size(); ++c)
                    for (uint32_t p = 0; p <= contig[c].size() + 2; ++p)  // (the last starts leave the contig: invalid)
                        for (uint32_t strand = 0; strand < 2; ++strand)
                            if (const int rc = check(c, p, strand)) {
                                std::fprintf(stderr, "shape %u/%u/%u set %u view %d locus %u %u %u\n", site_len, s.down, nick, n_e, view, c, p, strand);
                                return rc;
                            }
                const uint32_t bad[][3] = {{6, 0, 0}, {0xFFFFFFFFu, 0, 0}, {4, 10, 2}, {4, 400 - site_len + 1, 0}, {4, 0xFFFFFFFFu, 1},
                                           {5, 0xFFFFFFF0u, 0}, {4, 10, 0xFFFFFFFFu}};
                for (const auto &b : bad) {
                    uint64_t h, l;
                    if (prime_context(g, s, b[0], b[1], b[2], &h, &l) != kEffInvalid) return 16;
                }
            }
        }
    }
    // the shapes and the edits the definition refuses
    const PrimeShape good = make_shape(23, 41, 17, 13, 13, 10, 34, 5, 21, 2, 17, 3, 1, false);
    PrimeShape bad[14];
    for (PrimeShape &b : bad) b = good;
    bad[0].site_len = 15, bad[1].site_len = 33, bad[2].down = 42, bad[3].nick = 0, bad[4].nick = 24, bad[5].pbs_min = 0, bad[6].pbs_max = 18;
    bad[7].rtt_min = 0, bad[8].rtt_max = 48, bad[9].min_homology = 35, bad[10].pam_len = 3, bad[11].seed_len = 9, bad[12].flags = 2;
    bad[13].di[7] = kPrimeMaxWeight + 1;
    for (const PrimeShape &b : bad)
        if (prime_shape_valid(b)) return 17;
    const PrimeEdit refused[] = {{0, 0, 0, 0}, {0, 0, 17, 0}, {0, 0, 17u << 16, 0}, {0, 5, 1u << 16, 4}, {0, 98, 3, 0}, {0, 101, 1u << 16, 0}};
    for (const PrimeEdit &e : refused)
        if (prime_edit_valid(e, 100)) return 18;
    if (!prime_edit_valid(PrimeEdit{0, 100, 1u << 16, 3}, 100) || !prime_edit_valid(PrimeEdit{0, 84, 16 | 16u << 16, 0xFFFFFFFFu}, 100)) return 19;
    for (uint32_t k = 0; k < kEffClasses; ++k)
        if (classes[k] == 0) return 20;
    if (!with_pair || !pairs || !weak || !lengthened || !no_g_end || !past_end || !over_max) return 21;
    for (uint32_t b = 0; b < kPrimeFlags; ++b)
        if (!by_flag[b] || by_flag[b] == pairs) return 22;
    std::printf("ok: %llu loci (%llu defined, %llu weak, %llu with a pair), %llu pairs (PAM %llu, SEED %llu, POLY_T %llu, WEAK %llu), "
                "%llu lengthened, refused: %llu rtt_max, %llu no non-G end, %llu end of E\n",
                loci, defined, weak, with_pair, pairs, by_flag[0], by_flag[1], by_flag[2], by_flag[3], lengthened, over_max, no_g_end, past_end);
    return 0;
}
