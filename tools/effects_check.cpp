// effects_check.cpp - the coding-consequence functions of varscot_amd/csrc/vsc_effects.h (cds_find, effects_base, codon_of,
// effect_alt, effect_class, effect_info, effects_row, effects_count, effects_keep and what they call) in a stand-alone program
// with its own main, for the host sanitizers.  No device is opened and no kernel is launched.  Build and run on the CPU:
//   hipcc --offload-arch=gfx950 -x hip -O1 -g -std=c++17 -Iinclude -Ivarscot_amd/csrc -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tools/effects_check.cpp -o build/effects_check && build/effects_check
//   - a generated genome (contigs of 400, 250 and 120 bases with a few N, one N apart) packed into plane arrays of exactly the
//     held words, and generated transcripts: segments of 1 .. 12 bases, gaps of 0 .. 30, three interleaved transcripts per
//     contig on either strand with first phases 0, 1 and 2, a segment at base 0 and one at the contig's end, in heap arrays of
//     exactly n entries;
//   - every (contig, position, strand), site_len 16, 23 and 32, windows at both ends of the site, win_len 1, 5 and 16, every
//     from -> to, the standard code and one with other stops, the whole genome and a view that starts at word 1 and ends one
//     word early;
//   - against a second walk by brute force: a letter array and a position array per transcript, every codon of every transcript
//     of the contig looked at for every site.
// Exit code 0 and "effects_check: ok" when all agree.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <tuple>
#include <vector>

#include "vsc_effects.h"

using namespace vsc;

static int code_of(char c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 4; }

static std::string random_text(size_t n)
{
    std::string t(n, 'A');
    for (char &c : t) c = "ACGT"[std::rand() % 4];
    return t;
}

struct Segment {
    uint32_t contig, start, end, tx;
};
struct Transcript {
    uint32_t contig = 0, strand = 0, phase = 0;
    std::vector<uint32_t> segs;      // indices in genome order
    std::vector<uint32_t> where;     // global position of every coding base, transcript order
};

int main()
{
    std::srand(429);
    const uint32_t lens[3] = {400, 250, 120};
    std::vector<std::string> contig;
    std::vector<uint32_t> off, end;
    std::string genome;
    for (uint32_t len : lens) {
        std::string t = random_text(len);
        for (int k = 0; k < 3; ++k) t[40 + std::rand() % (len - 80)] = 'N';
        off.push_back((uint32_t)genome.size());
        genome += t;
        end.push_back((uint32_t)genome.size());
        genome += 'N';
        contig.push_back(t);
    }
    const uint64_t words = (genome.size() + 31) / 32;
    std::vector<uint32_t> hi(words, 0), lo(words, 0), nm(words, 0);
    for (uint64_t g = 0; g < words * 32; ++g) {
        const int b = g < genome.size() ? code_of(genome[g]) : 4;
        if (b > 3) nm[g >> 5] |= 1u << (g & 31);
        else {
            hi[g >> 5] |= (uint32_t)(b >> 1) << (g & 31);
            lo[g >> 5] |= (uint32_t)(b & 1) << (g & 31);
        }
    }
    // the segments in genome order, three interleaved transcripts per contig
    std::vector<Segment> segments;
    std::vector<Transcript> txs(3 * contig.size());
    for (uint32_t c = 0; c < contig.size(); ++c) {
        uint32_t at = 0;
        while (at < lens[c]) {
            uint32_t len = 1 + std::rand() % 12;
            if (at + len + 14 > lens[c]) len = lens[c] - at;  // the last one ends at the contig's end
            const uint32_t tx = 3 * c + std::rand() % 3;
            txs[tx].segs.push_back((uint32_t)segments.size());
            segments.push_back(Segment{c, at, at + len, tx});
            at += len + std::rand() % 31;  // (a gap of 0: two segments that touch)
        }
    }
    const uint32_t n = (uint32_t)segments.size();
    std::unique_ptr<uint32_t[]> gstart(new uint32_t[n]);  // exactly the held size: the sanitizer sees one element too far
    std::unique_ptr<CdsSeg[]> seg(new CdsSeg[n]);
    for (uint32_t t = 0; t < txs.size(); ++t) {
        Transcript &x = txs[t];
        x.contig = t / 3;
        x.strand = std::rand() % 2;
        x.phase = t % 3;
        if (x.segs.empty()) return 2;
        std::vector<uint32_t> order = x.segs;
        if (x.strand) std::reverse(order.begin(), order.end());
        const uint32_t shift = (3u - x.phase) % 3u;
        uint32_t ci = shift;
        for (size_t k = 0; k < order.size(); ++k) {
            const Segment &s = segments[order[k]];
            const uint32_t g0 = off[s.contig] + s.start, g1 = off[s.contig] + s.end;
            gstart[order[k]] = g0;
            seg[order[k]] = CdsSeg{g0, g1, t, ci, k ? order[k - 1] : kCdsNone, k + 1 < order.size() ? order[k + 1] : kCdsNone, x.strand, shift};
            for (uint32_t i = 0; i < g1 - g0; ++i) x.where.push_back(x.strand ? g1 - 1 - i : g0 + i);
            ci += g1 - g0;
        }
    }
    const CdsView cds{gstart.get(), seg.get(), n};
    // cds_find against a linear scan, at every global position
    for (uint32_t g = 0; g <= genome.size() + 2; ++g) {
        uint32_t want = n;
        for (uint32_t k = 0; k < n; ++k)
            if (seg[k].gend > g) {
                want = k;
                break;
            }
        if (cds_find(cds, g) != want) return 3;
    }
    if (cds_find(CdsView{nullptr, nullptr, 0}, 5) != 0) return 4;

    // the standard code, and one where AGA and AGG are stops and TGA is W
    std::unique_ptr<uint8_t[]> codes[2] = {std::unique_ptr<uint8_t[]>(new uint8_t[64]), std::unique_ptr<uint8_t[]>(new uint8_t[64])};
    std::memcpy(codes[0].get(), kStandardCode, 64);
    std::memcpy(codes[1].get(), kStandardCode, 64);
    codes[1][8] = codes[1][10] = '*';  // AGA, AGG
    codes[1][56] = 'W';                // TGA

    unsigned long long loci = 0, defined = 0, effects = 0, by_class[kEffectClasses] = {}, split = 0, kept = 0;
    struct Effect {
        uint32_t low, tx, codon, info;
    };
    const uint32_t shapes[][3] = {{16, 0, 16}, {16, 15, 1}, {23, 3, 5}, {23, 0, 1}, {23, 7, 16}, {32, 16, 16}, {32, 0, 5}};
    for (const auto &sp : shapes)
        for (uint32_t from = 0; from < 4; ++from)
            for (uint32_t to = 0; to < 4; ++to) {
                if (to == from) continue;
                const EditShape s{sp[0], sp[1], sp[2], from};
                if (!edit_shape_valid(s)) return 5;
                const uint32_t which = (from + to) & 1u;
                const uint8_t *code = codes[which].get();
                for (int view = 0; view < 2; ++view) {  // the whole genome; words [1, words - 1) in arrays of exactly that length
                    const uint64_t first = view ? 1 : 0, held = words - 2 * first;
                    const std::vector<uint32_t> vh(hi.begin() + first, hi.begin() + first + held), vl(lo.begin() + first, lo.begin() + first + held),
                        vn(nm.begin() + first, nm.begin() + first + held);
                    const EffPlanes g{vh.data(), vl.data(), vn.data(), first, held, held, off.data(), end.data(), (uint32_t)contig.size()};
                    auto letter_at = [&](uint32_t x) -> int {  // 0 .. 3, 4: N or not held
                        if ((uint64_t)x < first * 32 || (uint64_t)x >= (first + held) * 32) return 4;
                        return code_of(genome[x]);
                    };
                    for (uint32_t c = 0; c < contig.size(); ++c)
                        for (uint32_t p = 0; p + s.site_len <= contig[c].size(); ++p)
                            for (uint32_t strand = 0; strand < 2; ++strand) {
                                ++loci;
                                uint64_t h = 0, l = 0;
                                if (edit_site(g, s, c, p, strand, &h, &l) != kEffDefined) continue;
                                ++defined;
                                const uint32_t mask = edit_mask(h, l, s);
                                const uint32_t g0 = off[c] + edit_window_first(p, strand, s);
                                // the brute-force walk: every codon of every transcript of the contig
                                std::vector<Effect> want;
                                uint32_t want0 = 0, want1 = 0;
                                auto window_at = [&](uint32_t x) -> uint32_t {  // the window position of global position x when MASK has it
                                    for (uint32_t j = 0; j < s.win_len; ++j)
                                        if ((mask >> j & 1u) && off[c] + edit_forward(p, strand, s, j) == x) return j;
                                    return s.win_len;
                                };
                                for (uint32_t t = 3 * c; t < 3 * c + 3; ++t) {
                                    const Transcript &x = txs[t];
                                    const uint32_t shift = (3u - x.phase) % 3u, total = shift + (uint32_t)x.where.size();
                                    for (uint32_t k = 0; 3 * k < total; ++k) {
                                        uint32_t n_edited = 0, at = s.win_len, low = 0xFFFFFFFFu, ref = 0, alt = 0, lo_pos = 0xFFFFFFFFu, hi_pos = 0;
                                        bool unknown = false;
                                        for (uint32_t i = 0; i < 3; ++i) {
                                            const uint32_t idx = 3 * k + i;
                                            if (idx < shift || idx >= total) {
                                                unknown = true;
                                                ref <<= 2, alt <<= 2;
                                                continue;
                                            }
                                            const uint32_t pos = x.where[idx - shift];
                                            lo_pos = std::min(lo_pos, pos), hi_pos = std::max(hi_pos, pos);
                                            const int b = letter_at(pos);
                                            if (b > 3) unknown = true;
                                            const uint32_t letter = (uint32_t)(x.strand ? 3 - b : b) & 3u;
                                            const uint32_t j = window_at(pos);
                                            ref = ref << 2 | letter;
                                            if (j < s.win_len) {
                                                ++n_edited;
                                                at = std::min(at, j);
                                                low = std::min(low, pos);
                                                alt = alt << 2 | (strand == x.strand ? to : 3u - to);
                                            } else {
                                                alt = alt << 2 | letter;
                                            }
                                        }
                                        if (!n_edited) continue;
                                        uint32_t cls;
                                        if (unknown) cls = kEffectUnknown, ref = alt = 0;
                                        else if (k == 0 && x.phase == 0) cls = kEffectStartLost;
                                        else if (code[ref] != '*' && code[alt] == '*') cls = kEffectStopGained;
                                        else if (code[ref] == '*' && code[alt] != '*') cls = kEffectStopLost;
                                        else cls = code[ref] == code[alt] ? kEffectSynonymous : kEffectMissense;
                                        want.push_back(Effect{low, t, k, ref | alt << 6 | cls << 12 | n_edited << 16 | at << 20});
                                        want0 += 1u << (5 * cls);
                                        ++by_class[cls];
                                        split += hi_pos - lo_pos > 2 && lo_pos != 0xFFFFFFFFu;
                                    }
                                    for (uint32_t pos : x.where) {
                                        const uint32_t j = window_at(pos);
                                        if (j < s.win_len) want1 |= 1u << j;
                                    }
                                }
                                std::sort(want.begin(), want.end(), [](const Effect &a, const Effect &b) { return a.low < b.low; });
                                std::vector<Effect> got;
                                uint32_t w0 = 7, w1 = 7;
                                effects_row(g, cds, s, to, code, g0, strand, mask, &w0, &w1,
                                            [&](uint32_t tx, uint32_t codon, uint32_t info) { got.push_back(Effect{0, tx, codon, info}); });
                                if (w0 != want0 || w1 != want1 || got.size() != want.size()) return 6;
                                for (size_t k = 0; k < got.size(); ++k)
                                    if (got[k].tx != want[k].tx || got[k].codon != want[k].codon || got[k].info != want[k].info) return 7;
                                if (effects_count(w0, w1) != got.size() || got.size() > kEditMaxWindow) return 8;
                                // the records' pass walks word 1 of the row: the same effects, the same row
                                std::vector<Effect> again;
                                uint32_t r0 = 7, r1 = 7;
                                effects_row(g, cds, s, to, code, g0, strand, w1, &r0, &r1,
                                            [&](uint32_t tx, uint32_t codon, uint32_t info) { again.push_back(Effect{0, tx, codon, info}); });
                                if (r0 != w0 || r1 != w1 || again.size() != got.size()) return 9;
                                for (size_t k = 0; k < got.size(); ++k)
                                    if (again[k].tx != got[k].tx || again[k].codon != got[k].codon || again[k].info != got[k].info) return 10;
                                effects += got.size();
                                // FILTER
                                uint32_t have = 0;
                                for (const Effect &e : want) have |= 1u << (e.info >> 12 & 7u);
                                for (uint32_t require : {0u, 4u, 6u, 63u})
                                    for (uint32_t forbid : {0u, 2u, 32u, 48u}) {
                                        const bool keep = (require == 0 || (have & require)) && !(have & forbid);
                                        if (effects_keep(kEffDefined, w0, require, forbid) != keep) return 11;
                                        kept += keep;
                                    }
                            }
                }
            }
    if (effects_keep(kEffHasN, 0, 0, 0) || effects_keep(kEffInvalid, 0, 0, 0) || effects_count(kEffectsUndefined, kEffectsUndefined) != 0) return 12;
    // effect_alt and effect_class, case by case
    if (effect_alt(16, 1, 3) != 48 || effect_alt(16, 4, 2) != 18 || effect_alt(0, 7, 3) != 63 || effect_alt(27, 0, 2) != 27) return 13;
    const uint8_t *std_code = codes[0].get();
    if (effect_class(16, 48, 3, true, std_code, false) != kEffectStopGained || effect_class(48, 16, 3, true, std_code, false) != kEffectStopLost ||
        effect_class(14, 12, 0, true, std_code, false) != kEffectStartLost || effect_class(14, 12, 0, false, std_code, false) != kEffectMissense ||
        effect_class(28, 30, 2, true, std_code, false) != kEffectSynonymous || effect_class(28, 30, 2, true, std_code, true) != kEffectUnknown)
        return 14;
    for (uint32_t k = 0; k < kEffectClasses; ++k)
        if (!by_class[k]) return 15;
    if (!split || !kept || !effects) return 16;
    std::printf("effects_check: ok: %llu loci (%llu defined), %llu effects (synonymous %llu, missense %llu, stop_gained %llu, stop_lost %llu, "
                "start_lost %llu, unknown %llu), %llu in split codons\n",
                loci, defined, effects, by_class[0], by_class[1], by_class[2], by_class[3], by_class[4], by_class[5], split);
    return 0;
}
