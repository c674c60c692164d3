// knockout_check.cpp - the knock-out functions of varscot_amd/csrc/vsc_knockout.h (knockout_shape_valid, knockout_cut,
// knockout_occupied, knockout_find, the cursor, knockout_walk, knockout_row, knockout_keep and what they call of vsc_effects.h)
// in a stand-alone program with its own main, for the host sanitizers.  No device is opened and no kernel is launched.  Build
// and run on the CPU:
//   g++ -O1 -g -std=c++17 -Iinclude -Ivarscot_amd/csrc -fsanitize=address,undefined -fno-sanitize-recover=undefined
//       tools/knockout_check.cpp -o build/knockout_check && build/knockout_check
//   - a generated genome (contigs of 15, 33, 700, 900 and 400 bases one N apart, N runs and single N inside) packed into plane
//     arrays of exactly the held words, the whole genome and a view that starts at word 2 and ends one word early;
//   - a CDS in heap arrays of exactly its segments, per-transcript table and bitmap words: exon-like segments of 1 to 90 bases
//     with introns of 0 (abutting) to 60, grouped 1 to 5 per transcript, both strands, every first phase, transcripts that end
//     in the middle of a codon; and no CDS at all;
//   - every (contig, position, strand), the loci the definition calls invalid, several shapes (site_len 16, 23, 32; cut 1 and
//     site_len - 1; windows 0, 50, 65535; max_codons 1, 7, 4096), two codes;
//   - against a brute-force second route: every transcript's coding string is materialised, s letters are deleted at K, the
//     rest is translated codon by codon and searched for '*'; and knockout_keep against the rule applied to the fields.
// Exit code 0 and "ok" when all agree.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "vsc_knockout.h"

using namespace vsc;

static int code_of(char c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 4; }

struct TextSeg {
    uint32_t contig, start, end, tx, strand, phase;
};

// a transcript on letters: T = '?' x shift + its coding letters in transcript orientation, where[j] = the global position of T[j]
struct TextTx {
    uint32_t shift = 0, n_seg = 0, junction = 0;
    std::string T;
    std::vector<long> where;
    std::vector<uint32_t> first_of_seg;  // per segment in transcript order: the index of its first base
};

static char comp(char c) { return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : 'N'; }

int main()
{
    std::srand(437);
    // ---- the genome: letters, and planes of exactly the held words
    const size_t lens[] = {15, 33, 700, 900, 400};
    std::vector<std::string> contigs;
    std::vector<uint32_t> off, end;
    std::string genome;
    for (size_t n : lens) {
        std::string t(n, 'A');
        for (char &c : t) c = "ACGT"[std::rand() % 4];
        if (n >= 400) {
            for (size_t i = 100; i < 106; ++i) t[i] = 'N';
            t[300] = 'N';
        }
        off.push_back((uint32_t)genome.size());
        genome += t;
        end.push_back((uint32_t)genome.size());
        genome += 'N';
        contigs.push_back(t);
    }
    const uint64_t words = (genome.size() + 31) / 32;
    // ---- the CDS: segments in (contig, start) order, grouped into transcripts
    std::vector<TextSeg> segs;
    uint32_t n_tx = 0;
    for (uint32_t c = 2; c < contigs.size(); ++c) {
        std::vector<std::pair<uint32_t, uint32_t>> mine;
        uint32_t at = 5 + std::rand() % 30;
        while (at + 100 < contigs[c].size()) {
            const uint32_t n = std::rand() % 6 == 0 ? 1 + std::rand() % 2 : 1 + std::rand() % 90;
            mine.push_back({at, at + n});
            at += n + (std::rand() % 5 == 0 ? 0 : 1 + std::rand() % 60);
        }
        for (size_t k = 0; k < mine.size();) {
            const size_t group = std::min(mine.size() - k, (size_t)(1 + std::rand() % 5));
            const uint32_t strand = std::rand() % 2, phase = std::rand() % 3;
            uint32_t ci = (3 - phase) % 3;
            for (size_t j = 0; j < group; ++j) {
                const auto &m = mine[strand ? k + group - 1 - j : k + j];
                segs.push_back(TextSeg{c, m.first, m.second, n_tx, strand, j == 0 ? phase : (3 - ci % 3) % 3});
                ci += m.second - m.first;
            }
            ++n_tx;
            k += group;
        }
    }
    std::sort(segs.begin(), segs.end(), [](const TextSeg &a, const TextSeg &b) { return a.contig != b.contig ? a.contig < b.contig : a.start < b.start; });
    const uint32_t codes_n = 2;
    // the standard code and one with AGA / AGG as stops and TGA as W
    std::string code_text[codes_n] = {kStandardCode, kStandardCode};
    code_text[1][8] = '*', code_text[1][10] = '*', code_text[1][56] = 'W';
    const KoShape shapes[] = {{23, 17, 50, 0, 4096}, {23, 17, 0, 0, 4096}, {23, 17, 65535, 65535, 4096}, {16, 1, 50, 10, 1},
                              {16, 15, 0, 50, 7},    {32, 31, 50, 0, 4096}, {32, 1, 20, 0, 4096},         {23, 22, 50, 0, 2}};
    unsigned long long rows = 0, coding = 0, junctions = 0, undefined = 0, by_d[4] = {}, flags_seen = 0, kept = 0, past = 0;
    for (int with_cds = 1; with_cds >= 0; --with_cds) {
        const size_t n = with_cds ? segs.size() : 0;
        // the library's arrays, exactly as long as they are used: global starts, segments, per-transcript table, bitmap
        std::unique_ptr<uint32_t[]> gstart(new uint32_t[n]);
        std::unique_ptr<CdsSeg[]> seg(new CdsSeg[n]);
        std::unique_ptr<KoTx[]> txs(new KoTx[n_tx]);
        std::vector<TextTx> text_tx(n_tx);
        for (uint32_t t = 0; t < n_tx; ++t) txs[t] = KoTx{0, 0, 0, 0};
        const uint32_t n_blocks = (uint32_t)((genome.size() + (1u << kKoBlockBits) - 1) >> kKoBlockBits);
        const size_t map_words = (n_blocks + 31) / 32;
        std::unique_ptr<uint32_t[]> bitmap(new uint32_t[map_words]());
        for (size_t i = 0; i < n; ++i) {
            const TextSeg &s = segs[i];
            gstart[i] = off[s.contig] + s.start;
            seg[i] = CdsSeg{off[s.contig] + s.start, off[s.contig] + s.end, s.tx, 0, kCdsNone, kCdsNone, s.strand, 0};
            for (uint32_t b = seg[i].gstart >> kKoBlockBits; b <= (seg[i].gend - 1) >> kKoBlockBits; ++b) bitmap[b >> 5] |= 1u << (b & 31);
        }
        for (uint32_t t = 0; t < n_tx && n; ++t) {
            std::vector<uint32_t> order;
            for (size_t i = 0; i < n; ++i)
                if (segs[i].tx == t) order.push_back((uint32_t)i);
            if (segs[order[0]].strand) std::reverse(order.begin(), order.end());
            TextTx &tt = text_tx[t];
            tt.shift = (3 - segs[order[0]].phase) % 3;
            tt.T.assign(tt.shift, '?');
            tt.where.assign(tt.shift, -1);
            for (size_t j = 0; j < order.size(); ++j) {
                const TextSeg &s = segs[order[j]];
                CdsSeg &q = seg[order[j]];
                q.ci0 = (uint32_t)tt.T.size();
                q.shift = tt.shift;
                q.prev = j ? order[j - 1] : kCdsNone;
                q.next = j + 1 < order.size() ? order[j + 1] : kCdsNone;
                tt.first_of_seg.push_back((uint32_t)tt.T.size());
                for (uint32_t i = 0; i < s.end - s.start; ++i) {
                    const uint32_t p = s.strand ? s.end - 1 - i : s.start + i;
                    tt.T += s.strand ? comp(contigs[s.contig][p]) : contigs[s.contig][p];
                    tt.where.push_back((long)off[s.contig] + p);
                }
            }
            tt.n_seg = (uint32_t)order.size();
            tt.junction = tt.first_of_seg.back();
            txs[t] = KoTx{tt.shift, (uint32_t)tt.T.size(), tt.junction, tt.n_seg};
        }
        const CdsView view{gstart.get(), seg.get(), (uint32_t)n};
        for (int partial = 0; partial < 2; ++partial) {
            const uint64_t first_word = partial ? 2 : 0, held = partial ? words - 3 : words;
            std::unique_ptr<uint32_t[]> hi(new uint32_t[held]()), lo(new uint32_t[held]()), nm(new uint32_t[held]());
            for (uint64_t w = 0; w < held; ++w)
                for (uint32_t b = 0; b < 32; ++b) {
                    const uint64_t x = (first_word + w) * 32 + b;
                    const int v = x < genome.size() ? code_of(genome[x]) : 4;
                    if (v > 3) nm[w] |= 1u << b;
                    else hi[w] |= (uint32_t)(v >> 1) << b, lo[w] |= (uint32_t)(v & 1) << b;
                }
            const EffPlanes g{hi.get(), lo.get(), nm.get(), first_word, held, held, off.data(), end.data(), (uint32_t)contigs.size()};
            auto letter = [&](long x) -> char {  // the letter the object holds at global position x
                if (x < (long)(first_word * 32) || x >= (long)((first_word + held) * 32) || x >= (long)genome.size()) return 'N';
                return genome[(size_t)x];
            };
            for (const KoShape &sh : shapes) {
                if (!knockout_shape_valid(sh)) return std::printf("a shape of the check is not valid\n"), 1;
                for (uint32_t cd = 0; cd < codes_n; ++cd) {
                    const uint8_t *code = (const uint8_t *)code_text[cd].data();
                    const KoFilter filter{3277, 42598, 3, kKoNmd1 | kKoPtc2, kKoUnknownFlag | kKoLast};
                    for (uint32_t c = 0; c <= contigs.size(); ++c) {
                        const size_t len = c < contigs.size() ? contigs[c].size() : 40;
                        for (uint32_t p = 0; p <= len + 1; ++p) {
                            for (uint32_t strand = 0; strand <= 2; ++strand) {
                                uint32_t got[4];
                                knockout_row(g, view, txs.get(), sh, code, c, p, strand, got);
                                ++rows;
                                // ---- the second route
                                uint32_t want[4] = {kKoUndefined, kKoUndefined, kKoUndefined, kKoUndefined};
                                bool is_coding = false;
                                if (c < contigs.size() && strand <= 1 && (size_t)p + sh.site_len <= len) {
                                    const long x = (long)off[c] + p + (strand ? sh.site_len - sh.cut : sh.cut);
                                    long s_at = -1;
                                    bool junction = false;
                                    for (size_t i = 0; i < n; ++i) {
                                        if ((long)seg[i].gstart < x && x < (long)seg[i].gend) s_at = (long)i;
                                        for (long y = x - 1; y <= x; ++y) junction |= (long)seg[i].gstart <= y && y < (long)seg[i].gend;
                                    }
                                    if (s_at < 0) {
                                        want[0] = 0xFFFFFFFFu, want[1] = 0, want[2] = junction ? 0x80000000u : 0u, want[3] = 0;
                                        junctions += junction;
                                        if (!knockout_occupied(bitmap.get(), n_blocks, (uint32_t)x - 1) && !knockout_occupied(bitmap.get(), n_blocks, (uint32_t)x)) {
                                            ++past;
                                            if (junction) return std::printf("the bitmap hides a junction at %ld\n", x), 1;
                                        }
                                    } else {
                                        is_coding = true;
                                        const CdsSeg &q = seg[(size_t)s_at];
                                        const TextTx &tt = text_tx[q.transcript];
                                        const long at = q.strand ? x - 1 : x;
                                        const uint32_t K = (uint32_t)(std::find(tt.where.begin(), tt.where.end(), at) - tt.where.begin());
                                        std::string T = tt.T;  // as the object holds it
                                        for (size_t j = tt.shift; j < T.size(); ++j)
                                            if (letter(tt.where[j]) == 'N') T[j] = 'N';
                                        const uint32_t codon = K / 3, frame = K % 3, bases = (uint32_t)T.size() - tt.shift;
                                        const uint32_t frac = (uint32_t)(((uint64_t)(K - tt.shift) << 16) / bases);
                                        const uint32_t edge = (uint32_t)std::min<long>({x - (long)q.gstart, (long)q.gend - x, 255});
                                        uint32_t flags = (q.prev == kCdsNone ? 1u : 0u) | (q.next == kCdsNone ? 2u : 0u), d[2];
                                        for (uint32_t s = 1; s <= 2; ++s) {
                                            std::string shifted = T;
                                            shifted.erase(K, s);
                                            uint32_t ds = kKoCap;
                                            for (uint32_t k = 0; k < sh.max_codons; ++k) {
                                                const size_t j = 3 * (size_t)(codon + k);
                                                if (j + 3 > shifted.size()) {
                                                    ds = kKoEnd;
                                                    break;
                                                }
                                                if (j < tt.shift) continue;  // (j < K here, so it is the transcript's own index)
                                                const int b0 = code_of(shifted[j]), b1 = code_of(shifted[j + 1]), b2 = code_of(shifted[j + 2]);
                                                if (b0 > 3 || b1 > 3 || b2 > 3) {
                                                    ds = kKoUnknown;
                                                    break;
                                                }
                                                if (code_text[cd][16 * b0 + 4 * b1 + b2] == '*') {
                                                    ds = k;
                                                    const long first = (long)(j < K ? j : j + s), e = (long)(j + 2 < K ? j + 2 : j + 2 + s) + 1;
                                                    flags |= 4u << (s - 1);
                                                    if (tt.n_seg > 1 && (long)tt.junction - e >= (long)sh.nmd_window &&
                                                        (sh.start_window == 0 || first - (long)tt.shift >= (long)sh.start_window))
                                                        flags |= 16u << (s - 1);
                                                    break;
                                                }
                                            }
                                            if (ds == kKoUnknown) flags |= 64u;
                                            d[s - 1] = ds;
                                            ++by_d[ds == kKoEnd ? 0 : ds == kKoCap ? 1 : ds == kKoUnknown ? 2 : 3];
                                        }
                                        flags_seen |= flags;
                                        want[0] = q.transcript, want[1] = codon | frame << 30, want[2] = frac | edge << 16 | flags << 24;
                                        want[3] = d[0] | d[1] << 16;
                                        ++coding;
                                    }
                                } else {
                                    ++undefined;
                                }
                                for (int w = 0; w < 4; ++w)
                                    if (got[w] != want[w])
                                        return std::printf("locus (%u, %u, %u) shape (%u, %u, %u, %u, %u) code %u partial %d: word %d is %08x, not %08x\n", c,
                                                           p, strand, sh.site_len, sh.cut, sh.nmd_window, sh.start_window, sh.max_codons, cd, partial, w,
                                                           got[w], want[w]),
                                               1;
                                bool keep = false;
                                if (is_coding) {
                                    const uint32_t frac = want[2] & 0xFFFF, edge = want[2] >> 16 & 0xFF, flags = want[2] >> 24;
                                    keep = frac >= filter.min_frac && frac <= filter.max_frac && edge >= filter.min_edge &&
                                           (flags & filter.require) == filter.require && !(flags & filter.forbid);
                                }
                                if (knockout_keep(got, filter) != keep) return std::printf("locus (%u, %u, %u): the filter's verdict differs\n", c, p, strand), 1;
                                kept += keep;
                            }
                        }
                    }
                }
            }
        }
    }
    if (!coding || !junctions || !undefined || !past || !kept || flags_seen != 0x7F || !by_d[0] || !by_d[1] || !by_d[2] || !by_d[3])
        return std::printf("the check does not reach every case: flags %llx, d %llu %llu %llu %llu, kept %llu\n", flags_seen, by_d[0], by_d[1],
                           by_d[2], by_d[3], kept),
               1;
    std::printf("ok: %llu rows against the deleted and translated coding strings (%llu coding cuts, %llu at a junction, %llu undefined, "
                "%llu past the bitmap, %llu kept by the filter; walks: %llu end, %llu cap, %llu unknown, %llu stop)\n",
                rows, coding, junctions, undefined, past, kept, by_d[0], by_d[1], by_d[2], by_d[3]);
    return 0;
}
