// motif_check.cpp - the motif rows of varscot_amd/csrc/vsc_motif.h (motif_shape_valid, motif_accepts, motif_layout,
// motif_flank_planes, motif_row, motif_keep, motif_context and what they call, vsc_efficiency.h's eff_context among them) in a
// stand-alone program with its own main, for the host sanitizers.  No device is opened and no kernel is launched.  Build and run
// on the CPU:
//   hipcc --offload-arch=gfx950 -x hip -O1 -g -std=c++17 -Iinclude -Ivarscot_amd/csrc -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tools/motif_check.cpp -o build/motif_check && build/motif_check
//   - motif_row over the planes of random and planted contexts for random shapes - every site length, flanks of 0 .. 16 letters,
//     C up to 64, n 12 .. 32, the zone anywhere in the site - random flanks of 0 .. 16 letters and motif sets of 1 .. 63 motifs of
//     2 .. 16 IUPAC letters on one or both strands, the pattern array of exactly the laid-out patterns, against a walk on LETTERS:
//     every start of every pattern tested letter by letter;
//   - motif_context over a small genome packed into plane arrays of exactly the held words - every (contig, position, strand),
//     the loci the definition calls invalid, the whole genome and a view that starts at word 1 and ends one word early - against
//     the class and the context taken from the text by slicing and reverse complement;
//   - motif_shape_valid, motif_accepts, motif_limits_valid and motif_keep at their bounds.
// Exit code 0 and "ok" when all agree.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "vsc_efficiency.h"
#include "vsc_motif.h"

using namespace vsc;

static int failures = 0;

static void fail(const char *what, const std::string &a, const std::string &b)
{
    if (++failures <= 20) std::fprintf(stderr, "MISMATCH %s: %s %s\n", what, a.c_str(), b.c_str());
}

static int code(char c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 4; }

static std::string revcomp(const std::string &s)
{
    std::string r(s.rbegin(), s.rend());
    for (char &c : r) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : 'N';
    return r;
}

static std::string random_text(size_t n, const char *alphabet = "ACGT", int letters = 4)
{
    std::string t(n, 'A');
    for (char &c : t) c = alphabet[std::rand() % letters];
    return t;
}

// the letters an IUPAC letter stands for, and its complement
static const char *letters_of(char c)
{
    switch (c) {
    case 'A': return "A";
    case 'C': return "C";
    case 'G': return "G";
    case 'T': return "T";
    case 'R': return "AG";
    case 'Y': return "CT";
    case 'S': return "CG";
    case 'W': return "AT";
    case 'K': return "GT";
    case 'M': return "AC";
    case 'B': return "CGT";
    case 'D': return "AGT";
    case 'H': return "ACT";
    case 'V': return "ACG";
    default: return "ACGT";
    }
}

static char iupac_complement(char c)
{
    const char from[] = "ACGTRYSWKMBDHVN", to[] = "TGCAYRSWMKVHDBN";
    for (int i = 0; from[i]; ++i)
        if (from[i] == c) return to[i];
    return 'N';
}

static std::string iupac_revcomp(const std::string &s)
{
    std::string r(s.rbegin(), s.rend());
    for (char &c : r) c = iupac_complement(c);
    return r;
}

static bool occurs_at(const std::string &t, size_t q, const std::string &p)
{
    if (q + p.size() > t.size()) return false;
    for (size_t k = 0; k < p.size(); ++k) {
        bool in = false;
        for (const char *l = letters_of(p[k]); *l; ++l) in = in || *l == t[q + k];
        if (!in) return false;
    }
    return true;
}

struct Motif {
    std::string text;
    bool both;
};

// the definition on letters
static MotifRow by_letters(const std::string &x, const std::string &left, const std::string &right, const std::vector<Motif> &motifs, const MotifShape &s)
{
    const std::string y = left + x.substr(s.up + s.proto_start, s.proto_len) + right;
    const size_t z0 = s.up + s.cut_start, z1 = z0 + s.cut_len;
    MotifRow r{0, 0, 0};
    for (size_t m = 0; m < motifs.size(); ++m) {
        std::vector<std::string> pats = {motifs[m].text};
        if (motifs[m].both) pats.push_back(iupac_revcomp(motifs[m].text));
        for (const std::string &p : pats) {
            for (size_t q = 0; q < y.size(); ++q)
                if (occurs_at(y, q, p)) r.construct |= 1ull << m;
            for (size_t q = 0; q < x.size(); ++q)
                if (occurs_at(x, q, p)) (q < z1 && q + p.size() > z0 ? r.cut : r.elsewhere) |= 1ull << m;
        }
    }
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

static std::string shape_text(const MotifShape &s)
{
    return std::to_string(s.up) + "+" + std::to_string(s.site_len) + "+" + std::to_string(s.down) + " spacer " + std::to_string(s.proto_start) + "," +
           std::to_string(s.proto_len) + " cut " + std::to_string(s.cut_start) + "," + std::to_string(s.cut_len);
}

// one context under one launch: motif_row on planes and a pattern array of exactly its size against the letters
static int check_row(const std::string &x, const std::string &left, const std::string &right, const std::vector<Motif> &motifs, const MotifShape &s)
{
    std::vector<uint64_t> accept(motifs.size());
    std::vector<uint32_t> len(motifs.size()), flags(motifs.size());
    for (size_t m = 0; m < motifs.size(); ++m) {
        if (!motif_accepts(motifs[m].text.data(), (uint32_t)motifs[m].text.size(), &accept[m])) fail("motif_accepts", motifs[m].text, "refused");
        len[m] = (uint32_t)motifs[m].text.size();
        flags[m] = motifs[m].both ? kMotifBothStrands : 0u;
    }
    std::vector<MotifPattern> all(kMotifMaxPatterns);
    const uint32_t n_pat =
        motif_layout(accept.data(), len.data(), flags.data(), (uint32_t)motifs.size(), s, (uint32_t)left.size(), (uint32_t)right.size(), all.data());
    const std::vector<MotifPattern> pat(all.begin(), all.begin() + n_pat);  // exactly n_pat elements
    std::vector<uint8_t> lf(left.size()), rf(right.size());
    for (size_t j = 0; j < left.size(); ++j) lf[j] = (uint8_t)code(left[j]);
    for (size_t j = 0; j < right.size(); ++j) rf[j] = (uint8_t)code(right[j]);
    MotifTable t{pat.data(), n_pat, (uint32_t)motifs.size(), 0, 0, (uint32_t)left.size(), (uint32_t)right.size()};
    motif_flank_planes(lf.data(), t.a, rf.data(), t.b, s.proto_len, &t.flank_h, &t.flank_l);
    uint64_t ch, cl;
    planes_of(x, &ch, &cl);
    const MotifRow got = motif_row(ch, cl, s, t), want = by_letters(x, left, right, motifs, s);
    if (got.construct != want.construct || got.cut != want.cut || got.elsewhere != want.elsewhere)
        fail("motif_row", x + " " + left + "|" + right + " " + shape_text(s),
             std::to_string(got.construct) + "," + std::to_string(got.cut) + "," + std::to_string(got.elsewhere) + " want " + std::to_string(want.construct) +
                 "," + std::to_string(want.cut) + "," + std::to_string(want.elsewhere));
    return 1;
}

static std::string put(std::string t, size_t q, const std::string &w)
{
    if (q + w.size() <= t.size()) t.replace(q, w.size(), w);
    return t;
}

int main()
{
    std::srand(36);
    unsigned long long rows = 0, contexts = 0;
    const char iupac[] = "ACGTRYSWKMBDHVN";
    for (int round = 0; round < 400; ++round) {
        MotifShape s{};
        s.site_len = 16 + std::rand() % 17;
        s.up = std::rand() % 17, s.down = std::rand() % 17;
        if (round % 7 == 0) s.site_len = 32, s.up = s.down = 16;
        if (round % 7 == 1) s.up = s.down = 0;
        s.proto_len = 12 + std::rand() % (s.site_len - 11);
        s.proto_start = std::rand() % (s.site_len - s.proto_len + 1);
        s.cut_len = 1 + std::rand() % 16;
        s.cut_start = std::rand() % (s.site_len - s.cut_len + 1);
        if (!motif_shape_valid(s)) fail("motif_shape_valid", shape_text(s), "refused");
        const uint32_t C = motif_context_len(s);
        const std::string left = random_text(round % 5 == 0 ? 16 : std::rand() % 17), right = random_text(round % 5 == 1 ? 16 : std::rand() % 17);
        const uint32_t M = round % 9 == 0 ? 63 : round % 9 == 1 ? 1 : 1 + std::rand() % 12;
        std::vector<Motif> motifs;
        for (uint32_t m = 0; m < M; ++m) {
            const uint32_t L = m == 0 ? 16 : m == 1 ? 2 : 2 + std::rand() % 7;
            std::string text(L, 'A');
            bool all_n = true;
            for (char &c : text) c = std::rand() % 4 ? "ACGT"[std::rand() % 4] : iupac[std::rand() % 15], all_n = all_n && c == 'N';
            if (all_n) text[0] = 'G';
            motifs.push_back(Motif{text, (bool)(std::rand() % 2)});
        }
        motifs.push_back(Motif{"GAATTC", true});  // a palindrome: one pattern
        if (motifs.size() > 63) motifs.resize(63);
        std::vector<std::string> xs;
        for (int i = 0; i < 6; ++i) xs.push_back(random_text(C));
        xs.push_back(random_text(C, "AC", 2));
        // planted: every motif's first pattern (its IUPAC letters spelled by their first letter) at both ends, at the zone's
        // edges and in the spacer; its reverse complement too
        const uint32_t z0 = s.up + s.cut_start, z1 = z0 + s.cut_len;
        for (size_t m = 0; m < motifs.size() && m < 4; ++m) {
            std::string w = motifs[m].text;
            for (char &c : w) c = letters_of(c)[0];
            const size_t L = w.size();
            const std::string blank(C, w[0] == 'A' ? 'C' : 'A');
            xs.push_back(put(blank, 0, w));
            xs.push_back(put(blank, C - L, w));
            if (z0 >= L) xs.push_back(put(blank, z0 - L, w));
            if (z0 + 1 >= L) xs.push_back(put(blank, z0 + 1 - L, w));
            xs.push_back(put(blank, z1, w));
            xs.push_back(put(blank, z1 - 1, w));
            xs.push_back(put(blank, s.up + s.proto_start, w));
            xs.push_back(put(blank, s.up + s.proto_start + s.proto_len - (L < s.proto_len ? L : s.proto_len), w));
            xs.push_back(put(blank, s.up + s.proto_start + 1, revcomp(w)));
            xs.push_back(put(put(blank, z0, w), 0, w));
        }
        for (const std::string &x : xs) rows += check_row(x, left, right, motifs, s);
    }

    // the bounds of the shape, the motifs, the limits and the filter rule
    {
        const MotifShape ok{16, 23, 16, 0, 20, 16, 2};
        MotifShape bad[] = {ok, ok, ok, ok, ok, ok, ok, ok, ok, ok};
        bad[0].site_len = 15, bad[1].site_len = 33, bad[2].up = 17, bad[3].down = 17, bad[4].proto_len = 11, bad[5].proto_start = 4;
        bad[6].cut_len = 0, bad[7].cut_len = 17, bad[8].cut_start = 22, bad[9].site_len = 32, bad[9].proto_len = 33;
        const MotifShape wide{16, 32, 16, 0, 32, 8, 16};  // C = 64
        if (!motif_shape_valid(ok) || !motif_shape_valid(wide)) fail("motif_shape_valid", shape_text(ok), "refused");
        for (const MotifShape &b : bad)
            if (motif_shape_valid(b)) fail("motif_shape_valid", shape_text(b), "accepted");
        uint64_t acc = 0;
        if (motif_accepts("A", 1, &acc) || motif_accepts("ACGTACGTACGTACGTA", 17, &acc) || motif_accepts("NN", 2, &acc) || motif_accepts("AX", 2, &acc) ||
            !motif_accepts("an", 2, &acc) || !motif_accepts("ACGTURYSWKMBDHVN", 16, &acc))
            fail("motif_accepts", "bounds", "");
        if (!motif_limits_valid(MotifLimits{1, 2, 4, 1}, 3) || motif_limits_valid(MotifLimits{8, 0, 0, 0}, 3) || motif_limits_valid(MotifLimits{0, 0, 0, 2}, 3) ||
            !motif_limits_valid(MotifLimits{1ull << 62, 0, 0, 0}, 63) || motif_limits_valid(MotifLimits{0, 1ull << 63, 0, 0}, 63))
            fail("motif_limits_valid", "bounds", "");
        for (uint32_t bits = 0; bits < 8; ++bits) {
            const MotifRow r{bits & 1u, (bits >> 1) & 1u, (bits >> 2) & 1u};
            const bool c = r.construct, cut = r.cut, el = r.elsewhere;
            if (motif_keep(kEffDefined, r, MotifLimits{1, 0, 0, 0}) != !c || motif_keep(kEffDefined, r, MotifLimits{0, 1, 0, 0}) != !(cut || el) ||
                motif_keep(kEffDefined, r, MotifLimits{0, 0, 1, 0}) != cut || motif_keep(kEffDefined, r, MotifLimits{0, 0, 1, 1}) != (cut && !el) ||
                !motif_keep(kEffDefined, r, MotifLimits{0, 0, 0, 0}) || motif_keep(kEffHasN, r, MotifLimits{0, 0, 0, 0}))
                fail("motif_keep", std::to_string(bits), "");
        }
    }

    // motif_context over a small genome: plane arrays of exactly the held words
    {
        std::vector<std::string> contigs = {random_text(22), random_text(23), random_text(27), random_text(180), random_text(61)};
        contigs[3].replace(70, 3, "NNN");
        std::vector<uint32_t> off, end;
        std::string text;
        for (const std::string &c : contigs) {
            off.push_back((uint32_t)text.size());
            text += c;
            end.push_back((uint32_t)text.size());
            text += 'N';
        }
        const uint64_t words = (text.size() + 31) / 32;
        std::vector<uint32_t> hi(words, 0), lo(words, 0), nm(words, 0);
        for (size_t p = 0; p < words * 32; ++p) {
            const int b = p < text.size() ? code(text[p]) : 4;
            if (b > 3) nm[p / 32] |= 1u << (p % 32);
            else hi[p / 32] |= (uint32_t)(b >> 1) << (p % 32), lo[p / 32] |= (uint32_t)(b & 1) << (p % 32);
        }
        const MotifShape shapes[] = {{16, 23, 16, 0, 20, 16, 2}, {16, 27, 16, 4, 23, 21, 6}, {0, 16, 0, 2, 12, 0, 1}, {16, 32, 16, 0, 32, 8, 16}, {3, 20, 11, 0, 20, 19, 1}};
        for (int view = 0; view < 2; ++view) {
            const uint64_t first = view ? 1 : 0, held = view ? words - 2 : words;
            const std::vector<uint32_t> vh(hi.begin() + first, hi.begin() + first + held), vl(lo.begin() + first, lo.begin() + first + held),
                vn(nm.begin() + first, nm.begin() + first + held);
            const EffPlanes g{vh.data(), vl.data(), vn.data(), first, held, held, off.data(), end.data(), (uint32_t)contigs.size()};
            for (const MotifShape &sh : shapes) {
                const uint32_t C = motif_context_len(sh);
                std::vector<uint32_t> loci;
                for (uint32_t c = 0; c <= contigs.size(); ++c)
                    for (uint32_t p = 0; p <= 181; ++p)
                        for (uint32_t strand = 0; strand < 3; ++strand) loci.insert(loci.end(), {c, p, strand});
                loci.insert(loci.end(), {0xFFFFFFFFu, 0u, 0u, 3u, 0xFFFFFFFFu, 1u, 3u, 0xFFFFFFFFu - 22u, 0u});
                for (size_t q = 0; q < loci.size(); q += 3) {
                    const uint32_t c = loci[q], p = loci[q + 1], strand = loci[q + 2];
                    uint32_t want = kEffDefined;
                    std::string x;
                    if (c >= contigs.size() || strand > 1 || (uint64_t)p + sh.site_len > contigs[c].size()) {
                        want = kEffInvalid;
                    } else {
                        const uint32_t before = strand ? sh.down : sh.up, behind = strand ? sh.up : sh.down;
                        if (p < before || (uint64_t)p + sh.site_len + behind > contigs[c].size()) {
                            want = kEffOffContig;
                        } else if ((uint64_t)off[c] + p - before < first * 32 || (uint64_t)off[c] + p - before + C > (first + held) * 32) {
                            want = kEffNotResident;
                        } else {
                            x = contigs[c].substr(p - before, C);
                            if (x.find('N') != std::string::npos) want = kEffHasN;
                            if (strand) x = revcomp(x);
                        }
                    }
                    uint64_t ch = 0, cl = 0;
                    const uint32_t got = motif_context(g, sh, c, p, strand, &ch, &cl);
                    ++contexts;
                    if (got != want) {
                        fail("motif_context class", std::to_string(c) + ":" + std::to_string(p) + ":" + std::to_string(strand),
                             std::to_string(got) + " want " + std::to_string(want));
                        continue;
                    }
                    if (want != kEffDefined) continue;
                    uint64_t wh, wl;
                    planes_of(x, &wh, &wl);
                    if (ch != wh || cl != wl) fail("motif_context planes", x, shape_text(sh));
                }
            }
        }
    }
    if (failures) {
        std::fprintf(stderr, "%d mismatches\n", failures);
        return 1;
    }
    std::printf("ok: %llu rows against the walk on letters, %llu loci against the text\n", rows, contexts);
    return 0;
}
