// hdr_check.cpp - the HDR knock-in functions of varscot_amd/csrc/vsc_hdr.h (hdr_shape_valid, hdr_context, hdr_reach, hdr_read,
// hdr_seen, hdr_blocked, hdr_substitute, hdr_pair, hdr_allowed_cds, hdr_walk, hdr_keep and what they call of vsc_prime.h and
// vsc_effects.h) in a stand-alone program with its own main, for the host sanitizers.  No device is opened and no kernel is
// launched.  Build and run on the CPU:
//   hipcc --offload-arch=gfx950 -x hip -O1 -g -std=c++17 -Iinclude -Ivarscot_amd/csrc -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tools/hdr_check.cpp -o build/hdr_check && build/hdr_check
//   - a small genome (contigs of site_len - 1, C - 1, C, C + 1, 400 with an N run, and 200 bases twice, one N apart) packed into
//     plane arrays of exactly the held words: every (contig, position, strand) and the loci the definition calls invalid, several
//     shapes (site_len 16, 23, 27, 32; no context and the largest; cut at 1 and at site_len - 1; both anchors; max_dist 0 and 63;
//     SUBSTITUTE, SUB_SEED and SUB_NONCODING on and off), the whole genome and a view that starts at word 1 and ends one word early;
//   - edit sets in heap arrays of exactly n_e entries, with a bitmap of exactly its words and without one: none, an SNV at every
//     position, and insertions, deletions and replacements of 1 to 16 letters in turn with edits at the first base and at the end
//     (an insertion at pos = length) of every contig;
//   - a CDS in heap arrays of exactly its segments: transcripts on both strands, segments of one and two bases, a first phase
//     other than 0, a transcript that runs into the N run - and no CDS;
//   - against a brute-force walk on letters: the context by slicing and reverse complement, E and S as strings, the rules letter
//     by letter, ALLOWED by translating codons of the contig text, every edit of the candidate's contig tried.
// Exit code 0 and "ok" when all agree.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "vsc_hdr.h"

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
    uint32_t edit, info, block;
};

struct TextSeg {
    uint32_t contig, start, end, tx, strand, phase;
};

// the codon of a forward base, on letters: the transcript's strand, the base's place in the codon and the three (contig-local)
// forward positions, -1 where the transcript has no such base
struct Codon {
    uint32_t strand, at;
    long p[3];
};

static HdrShape make_shape(uint32_t site_len, uint32_t up, uint32_t down, uint32_t cut, uint32_t max_dist, uint32_t anchor, uint32_t pam_start,
                           const char *pam, uint32_t seed_start, uint32_t seed_len, uint32_t proto_start, uint32_t proto_len, uint32_t min_seed,
                           uint32_t min_proto, uint32_t flags)
{
    HdrShape s{};
    s.site_len = site_len, s.up = up, s.down = down, s.cut = cut, s.max_dist = max_dist, s.anchor = anchor, s.pam_start = pam_start;
    for (s.pam_len = 0; pam[s.pam_len]; ++s.pam_len) {
        const char c = pam[s.pam_len];
        s.pam_accept[s.pam_len] = c == 'N' ? 15u : c == 'V' ? 7u : 1u << code(c);
    }
    s.seed_start = seed_start, s.seed_len = seed_len, s.proto_start = proto_start, s.proto_len = proto_len;
    s.min_seed_mm = min_seed, s.min_proto_mm = min_proto, s.flags = flags;
    return s;
}

int main()
{
    std::srand(34);
    unsigned long long loci = 0, defined = 0, with_pair = 0, with_usable = 0, pairs = 0, coding_subs = 0, by_flag[kHdrFlags] = {};
    unsigned long long classes[kEffClasses] = {}, no_letter_front = 0, no_letter_back = 0, far = 0, forbidden = 0;
    const uint32_t all = kHdrSubstitute | kHdrSubSeed | kHdrSubNoncoding;
    const HdrShape shapes[] = {
        make_shape(23, 20, 21, 17, 30, 1, 20, "NGG", 10, 10, 0, 20, 2, 4, all),
        make_shape(27, 18, 19, 22, 30, 0, 0, "TTTV", 4, 6, 4, 23, 2, 4, all),
        make_shape(16, 0, 0, 1, 63, 1, 13, "NGG", 5, 8, 0, 13, 1, 2, all),
        make_shape(32, 32, 0, 31, 63, 0, 0, "TTTV", 4, 16, 4, 28, 2, 4, kHdrSubstitute | kHdrSubSeed),
        make_shape(23, 20, 21, 17, 0, 1, 20, "NGG", 10, 10, 0, 20, 1, 4, kHdrSubstitute),
        make_shape(20, 10, 12, 3, 25, 1, 0, "CCN", 3, 8, 3, 17, 1, 3, all),
        make_shape(24, 8, 8, 20, 25, 0, 21, "NGG", 11, 10, 0, 21, 2, 0, 0u),
    };
    const char *codes[2] = {kStandardCode, "KNKNTTTT*S*SMIMIQHQHPPPPRRRRLLLLEDEDAAAAGGGGVVVV*Y*YSSSSWCWCLFLF"};
    for (const HdrShape &s : shapes) {
        if (!hdr_shape_valid(s)) return 3;
        const uint32_t C = hdr_context_len(s), site_len = s.site_len, s0 = s.up, K = s.up + s.cut;
        const uint32_t lens[7] = {site_len - 1, C - 1, C, C + 1, 400, 200, 200};
        std::vector<std::string> contig;
        std::vector<uint32_t> off, end;
        std::string genome;
        for (uint32_t len : lens) {
            std::string t = random_text(len);
            if (len == 400) t.replace(150, 7, "NNNNNNN");
            // the shape's PAM at every 29th site start, so that not every pair is BLOCKED by the PAM
            for (uint32_t p = 3; p + site_len <= len && len >= 200; p += 29)
                for (uint32_t j = 0; j < s.pam_len; ++j) {
                    const uint32_t acc = s.pam_accept[j], b = acc & 4u ? 2u : acc & 8u ? 3u : acc & 2u ? 1u : 0u;
                    const uint32_t at = p % 2 ? p + site_len - 1 - (s.pam_start + j) : p + s.pam_start + j;  // odd: a '-' site
                    if (t[at] != 'N') t[at] = "ACGT"[p % 2 ? 3u - b : b];
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
        // the CDS as text, ascending (contig, start), and as the kernels hold it, in arrays of exactly its segments
        const std::vector<TextSeg> segs = {{4, 20, 30, 0, 0, 0},  {4, 33, 34, 0, 0, 2},  {4, 40, 42, 0, 0, 1},   {4, 50, 70, 0, 0, 2},
                                           {4, 140, 153, 1, 1, 0}, {4, 160, 171, 1, 1, 2}, {4, 180, 200, 1, 1, 1}, {4, 230, 330, 2, 0, 2},
                                           {5, 10, 61, 3, 1, 2},  {5, 70, 72, 3, 1, 1},  {5, 80, 130, 3, 1, 0},  {6, 0, 200, 4, 0, 0}};
        const uint32_t n_seg = (uint32_t)segs.size();
        std::unique_ptr<uint32_t[]> seg_start(new uint32_t[n_seg]);
        std::unique_ptr<CdsSeg[]> seg(new CdsSeg[n_seg]);
        std::map<std::pair<uint32_t, uint32_t>, Codon> codon_at;
        for (uint32_t tx = 0; tx < 5; ++tx) {
            std::vector<uint32_t> mine;
            for (uint32_t i = 0; i < n_seg; ++i)
                if (segs[i].tx == tx) mine.push_back(i);
            const uint32_t strand = segs[mine[0]].strand;
            if (strand) std::reverse(mine.begin(), mine.end());  // transcript order
            const uint32_t shift = (3u - segs[mine[0]].phase) % 3u;
            uint32_t ci = shift;
            std::vector<long> where(shift, -1);  // coding index -> contig-local forward position
            for (size_t k = 0; k < mine.size(); ++k) {
                const TextSeg &t = segs[mine[k]];
                seg_start[mine[k]] = off[t.contig] + t.start;
                seg[mine[k]] = CdsSeg{off[t.contig] + t.start, off[t.contig] + t.end,           tx,     ci,
                                      k ? mine[k - 1] : kCdsNone,   k + 1 < mine.size() ? mine[k + 1] : kCdsNone, strand, shift};
                for (uint32_t j = 0; j < t.end - t.start; ++j) where.push_back(strand ? (long)t.end - 1 - j : (long)t.start + j);
                ci += t.end - t.start;
            }
            for (uint32_t c = shift; c < where.size(); ++c) {
                Codon cd{strand, c % 3u, {-1, -1, -1}};
                for (uint32_t i = 0; i < 3u; ++i)
                    if (3u * (c / 3u) + i < where.size()) cd.p[i] = where[3u * (c / 3u) + i];
                codon_at[{segs[mine[0]].contig, (uint32_t)where[c]}] = cd;
            }
        }
        // the edit sets as text, ascending (contig, pos), one edit per position
        std::vector<std::vector<TextEdit>> sets(3);
        uint32_t turn = 0;
        for (uint32_t c = 0; c < contig.size(); ++c) {
            const uint32_t len = (uint32_t)contig[c].size();
            for (uint32_t p = 0; p <= len; ++p) {
                if (p < len) sets[1].push_back({c, p, 1, std::string(1, "ACGT"[(code(contig[c][p]) + 1 + p % 3) % 4])});
                if (p == 0) sets[2].push_back({c, p, 1, "G"});
                else if (p == len) sets[2].push_back({c, p, 0, "TAC"});
                else if (p % 4 == 2 && p + 17 < len) {
                    const uint32_t n = 1 + turn % 16, kind = turn % 3;
                    ++turn;
                    sets[2].push_back({c, p, kind == 0 ? 0u : n, kind == 1 ? std::string() : random_text(1 + (n * 5) % 16)});
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
              for (int with_cds = 0; with_cds < 3; ++with_cds) {  // none; the standard code; another code
                if (n_e == 0 && with_cds) continue;
                const uint64_t first = view ? 1 : 0, held = words - 2 * first;
                const std::vector<uint32_t> vh(hi.begin() + first, hi.begin() + first + held), vl(lo.begin() + first, lo.begin() + first + held),
                    vn(nm.begin() + first, nm.begin() + first + held);
                const EffPlanes g{vh.data(), vl.data(), vn.data(), first, held, held, off.data(), end.data(), (uint32_t)contig.size()};
                const CdsView cds{seg_start.get(), seg.get(), n_seg};
                const uint8_t *aa = (const uint8_t *)codes[with_cds == 2];
                const bool noncoding = (s.flags & kHdrSubNoncoding) != 0u;
                auto check = [&](uint32_t c, uint32_t p, uint32_t strand) -> int {
                    uint32_t want = kEffDefined;
                    std::string R;
                    uint32_t F0 = 0;
                    const uint32_t left = strand ? s.down : s.up, right = strand ? s.up : s.down;
                    if (c >= contig.size() || strand > 1 || (uint64_t)p + site_len > contig[c].size()) want = kEffInvalid;
                    else if (p < left || (uint64_t)p + site_len + right > contig[c].size()) want = kEffOffContig;
                    else {
                        F0 = p - left;
                        const uint64_t g0 = (uint64_t)off[c] + F0;
                        if (g0 < first * 32 || g0 + C > (first + held) * 32) want = kEffNotResident;
                        else {
                            R = contig[c].substr(F0, C);
                            if (R.find('N') != std::string::npos) want = kEffHasN;
                            else if (strand) R = revcomp(R);
                        }
                    }
                    uint64_t h = 0, l = 0;
                    const uint32_t got = hdr_context(g, s, c, p, strand, &h, &l);
                    if (got != want) return 5;
                    ++loci;
                    ++classes[got];
                    if (got != kEffDefined) return hdr_keep(got, 1, 1, false, true) ? 6 : 0;
                    ++defined;
                    if (hdr_first_forward(p, strand, s) != F0) return 7;
                    // ALLOWED on letters: (ok, coding) of writing read letter b at reference context position r beside edit e
                    auto allowed = [&](uint32_t r, uint32_t b, const TextEdit &e, bool *coding) -> bool {
                        *coding = false;
                        if (!with_cds) return true;
                        const uint32_t f = F0 + (strand ? C - 1 - r : r);
                        const auto it = codon_at.find({c, f});
                        if (it == codon_at.end()) return noncoding;
                        *coding = true;
                        const Codon &cd = it->second;
                        std::string ref;
                        for (long q : cd.p) {
                            if (q < 0) return false;
                            if ((long)e.pos <= q + 1 && q <= (long)e.pos + (long)e.del) return false;
                            const char ch = contig[c][(size_t)q];
                            if (code(ch) > 3) return false;
                            ref += cd.strand ? revcomp(std::string(1, ch))[0] : ch;
                        }
                        std::string alt = ref;
                        const char fwd = "ACGT"[strand ? 3u - b : b];
                        alt[cd.at] = cd.strand ? revcomp(std::string(1, fwd))[0] : fwd;
                        auto amino = [&](const std::string &x) { return aa[16 * code(x[0]) + 4 * code(x[1]) + code(x[2])]; };
                        const bool same = amino(ref) == amino(alt);
                        forbidden += !same;
                        return same;
                    };
                    // every edit of the set, by brute force
                    std::vector<Pair> want_pairs;
                    for (uint32_t k = 0; k < n_e; ++k) {
                        const TextEdit &e = set[k];
                        if (e.contig != c || e.pos < F0 || e.pos - F0 + e.del > C) continue;
                        const uint32_t f = e.pos - F0, e0 = strand ? C - f - e.del : f, e1 = e0 + e.del;
                        const uint32_t side = e1 < K ? 1u : e0 > K ? 2u : 0u, dist = side == 1u ? K - e1 : side == 2u ? e0 - K : 0u;
                        if (dist > s.max_dist) {
                            ++far;
                            continue;
                        }
                        const std::string I = strand ? revcomp(e.ins) : e.ins, E = R.substr(0, e0) + I + R.substr(e1);
                        const long delta = (long)I.size() - (long)e.del;
                        const bool moved = s.anchor ? e0 < s0 + site_len : e1 <= s0;
                        const long shift = moved ? delta : 0;
                        std::string S(site_len, '-');  // '-': NO LETTER
                        for (uint32_t q = 0; q < site_len; ++q) {
                            const long x = (long)s0 + q + shift;
                            if (x >= 0 && x < (long)E.size()) S[q] = E[(size_t)x];
                            no_letter_front += x < 0;
                            no_letter_back += x >= (long)E.size();
                        }
                        bool pam_broken = false;
                        for (uint32_t j = 0; j < s.pam_len; ++j) {
                            const char ch = S[s.pam_start + j];
                            if (ch == '-' || !(s.pam_accept[j] >> code(ch) & 1u)) pam_broken = true;
                        }
                        uint32_t seed_mm = 0, proto_mm = 0;
                        for (uint32_t q = s.seed_start; q < s.seed_start + s.seed_len; ++q) seed_mm += S[q] != R[s0 + q];
                        for (uint32_t q = s.proto_start; q < s.proto_start + s.proto_len; ++q) proto_mm += S[q] != R[s0 + q];
                        uint32_t flags = (pam_broken ? (uint32_t)kHdrBPam : 0u) | (s.min_seed_mm && seed_mm >= s.min_seed_mm ? (uint32_t)kHdrBSeed : 0u) |
                                         (s.min_proto_mm && proto_mm >= s.min_proto_mm ? (uint32_t)kHdrBProto : 0u);
                        uint32_t block = kHdrNoBlock;
                        if (!flags) {
                            flags = kHdrOpen;
                            auto slot = [&](uint32_t q, uint32_t *r) {
                                const long x = (long)s0 + q + shift;
                                if (x < 0 || x >= (long)E.size() || (x >= (long)e0 && x < (long)(e0 + I.size()))) return false;
                                *r = (uint32_t)(x < (long)e0 ? x : x - delta);
                                return true;
                            };
                            if (s.flags & kHdrSubstitute) {
                                for (uint32_t j = 0; j < s.pam_len && flags == kHdrOpen; ++j) {
                                    uint32_t r;
                                    if (!slot(s.pam_start + j, &r)) continue;
                                    for (uint32_t b = 0; b < 4u && flags == kHdrOpen; ++b) {
                                        bool coding;
                                        if ((s.pam_accept[j] >> b & 1u) || !allowed(r, b, e, &coding)) continue;
                                        flags = kHdrSubbedPam;
                                        block = (s.pam_start + j) | b << 8 | (coding ? 1u : 0u) << 10 | r << 16;
                                    }
                                }
                                if (flags == kHdrOpen && (s.flags & kHdrSubSeed) && s.min_seed_mm && seed_mm + 1u >= s.min_seed_mm)
                                    for (uint32_t k2 = 0; k2 < s.seed_len && flags == kHdrOpen; ++k2) {
                                        const uint32_t q = s.anchor ? s.seed_start + s.seed_len - 1u - k2 : s.seed_start + k2;
                                        uint32_t r;
                                        if (!slot(q, &r) || S[q] != R[s0 + q]) continue;
                                        for (uint32_t b = 0; b < 4u && flags == kHdrOpen; ++b) {
                                            bool coding;
                                            if ("ACGT"[b] == R[s0 + q] || !allowed(r, b, e, &coding)) continue;
                                            flags = kHdrSubbedSeed;
                                            block = q | b << 8 | (coding ? 1u : 0u) << 10 | r << 16;
                                        }
                                    }
                            }
                        }
                        want_pairs.push_back({k, dist | side << 6 | seed_mm << 8 | proto_mm << 13 | flags << 24, block});
                        // S as planes, letter by letter
                        uint32_t r0, reach;
                        uint64_t ih, il, sh, sl, have;
                        if (!hdr_read(s, strand, f, rec[k], &r0, &ih, &il, &reach) || r0 != e0 || reach != (dist | side << 6)) return 9;
                        if (hdr_seen(s, h, l, e0, e.del, (uint32_t)I.size(), ih, il, &sh, &sl, &have) != (long)s0 + shift) return 10;
                        for (uint32_t q = 0; q < 64; ++q) {
                            const uint32_t b = (uint32_t)(sh >> q & 1u) << 1 | (uint32_t)(sl >> q & 1u);
                            const bool letter = q < site_len && S[q] != '-';
                            if ((have >> q & 1u) != (letter ? 1u : 0u) || b != (letter ? (uint32_t)code(S[q]) : 0u)) return 11;
                        }
                    }
                    const uint32_t g0 = off[c] + F0;
                    uint32_t usable = 0;
                    for (int with_map = 0; with_map < 2; ++with_map) {
                        uint32_t first_seg = kCdsNone;
                        const PrimeEdits pe{gpos.get(), rec.get(), with_map ? bitmap.get() : nullptr, n_e};
                        std::vector<Pair> got_pairs;
                        const uint32_t n = hdr_walk(
                            s, s.pam_accept, pe, h, l, c, g0, strand,
                            [&](uint32_t r, uint32_t ge, uint32_t del) -> uint32_t {
                                if (!with_cds) return kHdrAnyLetter;
                                return hdr_allowed_cds(g, cds, aa, noncoding, hdr_forward(s, g0, strand, r), strand, ge, del, g0, &first_seg);
                            },
                            [&](uint32_t k, uint32_t info, uint32_t block) { got_pairs.push_back({k, info, block}); });
                        if (n != got_pairs.size() || n != want_pairs.size()) return 12;
                        for (uint32_t k = 0; k < n; ++k)
                            if (got_pairs[k].edit != want_pairs[k].edit || got_pairs[k].info != want_pairs[k].info ||
                                got_pairs[k].block != want_pairs[k].block)
                                return 13;
                    }
                    pairs += want_pairs.size();
                    with_pair += !want_pairs.empty();
                    for (const Pair &q : want_pairs) {
                        for (uint32_t b = 0; b < kHdrFlags; ++b) by_flag[b] += q.info >> (24 + b) & 1u;
                        usable += !(q.info >> 24 & kHdrOpen);
                        coding_subs += q.block != kHdrNoBlock && (q.block >> 10 & 1u);
                    }
                    with_usable += usable != 0;
                    const uint32_t np = (uint32_t)want_pairs.size();
                    for (int have = 0; have < 2; ++have)
                        for (int allow = 0; allow < 2; ++allow)
                            if (hdr_keep(got, np, usable, have != 0, allow != 0) != (!have || usable >= 1 || (allow && np >= 1))) return 15;
                    return 0;
                };
                for (uint32_t c = 0; c < contig.size(); ++c)
                    for (uint32_t p = 0; p <= contig[c].size() + 2; ++p)  // (the last starts leave the contig: invalid)
                        for (uint32_t strand = 0; strand < 2; ++strand)
                            if (const int rc = check(c, p, strand)) {
                                std::fprintf(stderr, "shape %u/%u/%u set %u view %d cds %d locus %u %u %u\n", site_len, s.up, s.down, n_e, view, with_cds, c, p,
                                             strand);
                                return rc;
                            }
                const uint32_t bad[][3] = {{7, 0, 0}, {0xFFFFFFFFu, 0, 0}, {4, 10, 2}, {4, 400 - site_len + 1, 0}, {4, 0xFFFFFFFFu, 1},
                                           {5, 0xFFFFFFF0u, 0}, {4, 10, 0xFFFFFFFFu}};
                for (const auto &b : bad) {
                    uint64_t h, l;
                    if (hdr_context(g, s, b[0], b[1], b[2], &h, &l) != kEffInvalid) return 16;
                }
              }
            }
        }
    }
    // the shapes the definition refuses, one per rule
    const HdrShape good = make_shape(23, 20, 21, 17, 30, 1, 20, "NGG", 10, 10, 0, 20, 2, 4, all);
    HdrShape bad[20];
    for (HdrShape &b : bad) b = good;
    bad[0].site_len = 15, bad[1].site_len = 33, bad[2].up = 33, bad[2].down = 0, bad[3].down = 33, bad[3].up = 0, bad[4].up = 21, bad[5].cut = 0;
    bad[6].cut = 23, bad[7].max_dist = 64, bad[8].anchor = 2, bad[9].pam_len = 9, bad[10].pam_start = 21, bad[11].pam_accept[1] = 0;
    bad[12].pam_accept[1] = 16, bad[13].pam_accept[3] = 1, bad[14].seed_len = 17, bad[15].seed_start = 14, bad[16].proto_len = 33;
    bad[17].min_seed_mm = 11, bad[18].min_proto_mm = 21, bad[19].flags = 8;
    if (!hdr_shape_valid(good)) return 17;
    for (const HdrShape &b : bad)
        if (hdr_shape_valid(b)) return 18;
    for (uint32_t k = 0; k < kEffClasses; ++k)
        if (classes[k] == 0) return 20;
    if (!with_pair || !with_usable || !pairs || !coding_subs || !no_letter_front || !no_letter_back || !far || !forbidden) return 21;
    for (uint32_t b = 0; b < kHdrFlags; ++b)
        if (!by_flag[b] || by_flag[b] == pairs) return 22;
    std::printf("ok: %llu loci (%llu defined, %llu with a pair, %llu with a usable pair), %llu pairs (B_PAM %llu, B_SEED %llu, B_PROTO %llu, "
                "SUB_PAM %llu, SUB_SEED %llu, OPEN %llu), %llu substitutions in coding bases, %llu codons kept from changing, %llu edits too far\n",
                loci, defined, with_pair, with_usable, pairs, by_flag[0], by_flag[1], by_flag[2], by_flag[3], by_flag[4], by_flag[5], coding_subs,
                forbidden, far);
    return 0;
}
