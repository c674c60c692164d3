// efficiency_check.cpp - the on-target efficiency score of varscot_amd/csrc/vsc_efficiency.h (eff_shape_valid, eff_linear,
// eff_context and what they call) in a stand-alone program with its own main, for the host sanitizers.  No device is opened and
// no kernel is launched.  Build and run on the CPU:
//   hipcc --offload-arch=gfx950 -x hip -O1 -g -std=c++17 -ffp-contract=off -Iinclude -Ivarscot_amd/csrc -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tools/efficiency_check.cpp -o build/efficiency_check && build/efficiency_check
// The six shapes of the tests, four families of weights (dense, sparse, zero, magnitudes of 1e16 / 1 / 1e-16 mixed):
//   - eff_linear over the planes of random contexts against a letter-by-letter sum in the definition's order, bit for bit - the
//     weight arrays hold exactly eff_n_weights doubles, so a read past their end is the sanitizer's to find;
//   - eff_context over a small genome packed into plane arrays of exactly the held words - every (contig, position, strand),
//     the loci the definition calls invalid, the whole genome and a view that starts at word 1 and ends one word early -
//     against the class and the context taken from the text by slicing and reverse complement.
// Exit code 0 and "ok" when all agree.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "vsc_efficiency.h"

using namespace vsc;

static double rnd_weight(int family)
{
    const double u = (double)(std::rand() % 200001 - 100000) / 50000.0;
    if (family == 0) return u;
    if (family == 1) return std::rand() % 12 ? 0.0 : u;
    if (family == 2) return 0.0;
    const double scale[3] = {1e16, 1.0, 1e-16};
    return u * scale[std::rand() % 3];
}

static int code(char c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 4; }

static std::string revcomp(const std::string &s)
{
    std::string r(s.rbegin(), s.rend());
    for (char &c : r) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : 'N';
    return r;
}

struct Model {
    EffShape s;
    double intercept;
    std::vector<double> mono, di, gc;  // the caller's layout: mono[j][b], di[j][4 b_j + b_{j+1}], gc[k]
    std::vector<double> w;             // the layout of vsc_efficiency.h
};

static Model make_model(const EffShape &s, int family)
{
    Model m{s, rnd_weight(family), {}, {}, {}, {}};
    const uint32_t C = eff_context_len(s);
    m.mono.resize(4 * C);
    m.di.resize(16 * (C - 1));
    m.gc.resize(s.gc_len ? s.gc_len + 1 : 0);
    for (double &v : m.mono) v = rnd_weight(family);
    for (double &v : m.di) v = rnd_weight(family);
    for (double &v : m.gc) v = rnd_weight(family);
    m.w.assign(eff_n_weights(s), 0.0);
    for (uint32_t i = 0; i < 4 * C; ++i) m.w[i] = m.mono[i];
    for (uint32_t j = 0; j + 1 < C; ++j)
        for (uint32_t a = 0; a < 4; ++a)
            for (uint32_t b = 0; b < 4; ++b) m.w[eff_di_at(C) + 16 * j + a + 4 * b] = m.di[16 * j + 4 * a + b];
    for (uint32_t k = 0; k < m.gc.size(); ++k) m.w[eff_gc_at(C) + k] = m.gc[k];
    return m;
}

// the definition, letter by letter
static double by_letters(const Model &m, const std::string &t)
{
    double x = m.intercept;
    for (size_t j = 0; j < t.size(); ++j) x = x + m.mono[4 * j + code(t[j])];
    for (size_t j = 0; j + 1 < t.size(); ++j) x = x + m.di[16 * j + 4 * code(t[j]) + code(t[j + 1])];
    if (m.s.gc_len) {
        uint32_t n = 0;
        for (uint32_t j = m.s.gc_start; j < m.s.gc_start + m.s.gc_len; ++j) n += t[j] == 'G' || t[j] == 'C';
        x = x + m.gc[n];
    }
    return x;
}

static void planes_of(const std::string &t, uint64_t *h, uint64_t *l)
{
    *h = *l = 0;
    for (size_t j = 0; j < t.size(); ++j) {
        *h |= (uint64_t)(code(t[j]) >> 1) << j;
        *l |= (uint64_t)(code(t[j]) & 1) << j;
    }
}

int main()
{
    std::srand(31);
    const uint32_t shapes[6][3] = {{4, 23, 3}, {6, 23, 6}, {0, 16, 0}, {16, 32, 16}, {0, 23, 16}, {16, 23, 0}};
    unsigned long long sums = 0, loci = 0, defined = 0;
    for (const auto &sh : shapes) {
        const uint32_t C = sh[0] + sh[1] + sh[2];
        for (int family = 0; family < 4; ++family) {
            const EffShape s{sh[0], sh[1], sh[2], family == 2 ? 0u : sh[0], family == 2 ? 0u : (sh[1] < 20 ? sh[1] : 20u)};
            if (!eff_shape_valid(s)) return 1;
            const Model m = make_model(s, family);

            // ---- eff_linear ----
            for (int trial = 0; trial < 300; ++trial) {
                std::string t(C, 'A');
                for (char &c : t) c = "ACGT"[std::rand() % 4];
                uint64_t h, l;
                planes_of(t, &h, &l);
                const double x = eff_linear(m.w.data(), m.intercept, s, h, l), want = by_letters(m, t);
                if (std::memcmp(&x, &want, sizeof x) != 0) return 2;
                ++sums;
            }

            // ---- eff_context: contigs of C - 1, C, C + 1, 5, 200 (an N at 100) and 131 bases, one N apart ----
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
            for (int view = 0; view < 2; ++view) {  // the whole genome; words [1, words - 1) in arrays of exactly that length
                const uint64_t first = view ? 1 : 0, held = words - 2 * first;
                const std::vector<uint32_t> vh(hi.begin() + first, hi.begin() + first + held), vl(lo.begin() + first, lo.begin() + first + held),
                    vn(nm.begin() + first, nm.begin() + first + held);
                const EffPlanes g{vh.data(), vl.data(), vn.data(), first, held, held, off.data(), end.data(), (uint32_t)contig.size()};
                auto check = [&](uint32_t c, uint32_t p, uint32_t strand) -> int {
                    uint32_t want = kEffDefined;
                    std::string text;
                    if (c >= contig.size() || strand > 1 || (uint64_t)p + s.site_len > contig[c].size()) want = kEffInvalid;
                    else {
                        const uint32_t left = strand ? s.down : s.up, right = strand ? s.up : s.down;
                        if (p < left || p + s.site_len + right > contig[c].size()) want = kEffOffContig;
                        else {
                            const uint64_t g0 = (uint64_t)off[c] + p - left;
                            if (g0 < first * 32 || g0 + C > (first + held) * 32) want = kEffNotResident;
                            else {
                                text = contig[c].substr(p - left, C);
                                if (text.find('N') != std::string::npos) want = kEffHasN;
                                else if (strand) text = revcomp(text);
                            }
                        }
                    }
                    uint64_t h = 0, l = 0;
                    const uint32_t got = eff_context(g, s, c, p, strand, &h, &l);
                    if (got != want) return 3;
                    ++loci;
                    if (got != kEffDefined) return 0;
                    uint64_t wh, wl;
                    planes_of(text, &wh, &wl);
                    if (h != wh || l != wl) return 4;
                    const double x = eff_linear(m.w.data(), m.intercept, s, h, l), y = by_letters(m, text);
                    if (std::memcmp(&x, &y, sizeof x) != 0) return 5;
                    ++defined;
                    return 0;
                };
                for (uint32_t c = 0; c < contig.size(); ++c)
                    for (uint32_t p = 0; p <= contig[c].size() + 2; ++p)  // (the last starts leave the contig: invalid)
                        for (uint32_t strand = 0; strand < 2; ++strand)
                            if (const int rc = check(c, p, strand)) return rc;
                const uint32_t bad[][3] = {{6, 0, 0}, {0xFFFFFFFFu, 0, 0}, {4, 10, 2}, {4, 200 - sh[1] + 1, 0}, {4, 0xFFFFFFFFu, 1},
                                           {5, 0xFFFFFFF0u, 0}, {4, 10, 0xFFFFFFFFu}};
                for (const auto &b : bad) {
                    uint64_t h, l;
                    if (eff_context(g, s, b[0], b[1], b[2], &h, &l) != kEffInvalid) return 6;
                }
            }
        }
    }
    // the shapes the definition refuses
    const EffShape refused[] = {{17, 23, 0, 0, 0}, {0, 23, 17, 0, 0}, {16, 33, 15, 0, 0}, {4, 15, 3, 0, 0}, {4, 23, 3, 11, 20},
                                {4, 23, 3, 31, 0}, {4, 23, 3, 0xFFFFFFF0u, 0x20u}};
    for (const EffShape &s : refused)
        if (eff_shape_valid(s)) return 7;
    if (eff_revcomp(0x1ull, 64) != 0x7FFFFFFFFFFFFFFFull || eff_revcomp(0x1ull, 16) != 0x7FFFull) return 8;
    double u = eff_undefined();
    uint64_t ub;
    std::memcpy(&ub, &u, sizeof ub);
    if (ub != kEffUndefinedBits) return 9;
    if (defined == 0 || defined == loci) return 10;
    std::printf("ok: %llu sums, %llu loci (%llu defined)\n", sums, loci, defined);
    return 0;
}
