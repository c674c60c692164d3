// microhomology_check.cpp - the microhomology score of varscot_amd/csrc/vsc_mh.h (mh_shape_valid, mh_score, mh_keep, mh_context
// and what they call) in a stand-alone program with its own main, for the host sanitizers.  No device is opened and no kernel
// is launched.  Build and run on the CPU:
//   hipcc --offload-arch=gfx950 -x hip -O1 -g -std=c++17 -Iinclude -Ivarscot_amd/csrc -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tools/microhomology_check.cpp -o build/microhomology_check && build/microhomology_check
//   - mh_score over the planes of the tests' context families (random, the left half repeated, repeated but for one base,
//     period 1 to 4, two-letter alphabets, no row at all, one row) at F = 8, 9, 16, 30, 32 against the ROW LIST of the
//     definition: the triple loop, the drop of contained rows, the weights from exp;
//   - mh_context over a small genome packed into plane arrays of exactly the held words - every (contig, position, strand),
//     the loci the definition calls invalid, cut 0, 17 and 23, F = 8 and 32, the whole genome and a view that starts at word 1
//     and ends one word early - against the class and the context taken from the text by slicing and reverse complement.
// Exit code 0 and "ok" when all agree.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "vsc_mh.h"

using namespace vsc;

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

static void planes_of(const std::string &t, uint64_t *h, uint64_t *l)
{
    *h = *l = 0;
    for (size_t j = 0; j < t.size(); ++j) {
        *h |= (uint64_t)(code(t[j]) >> 1) << j;
        *l |= (uint64_t)(code(t[j]) & 1) << j;
    }
}

// the definition as the row list
struct Row {
    uint32_t i, j, k;
};
static void by_rows(const std::string &s, uint32_t F, uint32_t *sum, uint32_t *oof)
{
    const uint32_t W = 2 * F;
    std::vector<Row> rows;
    for (uint32_t k = F - 1; k >= 2; --k)
        for (uint32_t j = F; j + k <= W; ++j)
            for (uint32_t i = 0; i + k <= F; ++i)
                if (s.compare(i, k, s, j, k) == 0) rows.push_back(Row{i, j, k});
    *sum = *oof = 0;
    for (size_t a = 0; a < rows.size(); ++a) {
        const Row &r = rows[a];
        bool dropped = false;
        for (size_t b = 0; b < rows.size() && !dropped; ++b) {
            const Row &o = rows[b];
            dropped = a != b && o.j - o.i == r.j - r.i && o.i <= r.i && r.i + r.k <= o.i + o.k;
        }
        if (dropped) continue;
        const uint32_t d = r.j - r.i;
        uint32_t g = 0;
        for (uint32_t p = r.i; p < r.i + r.k; ++p) g += s[p] == 'G' || s[p] == 'C';
        const uint32_t t = (uint32_t)std::lround(std::round(std::exp(-(double)d / 20.0) * 1000.0));
        *sum += t * (r.k + g);
        if (d % 3) *oof += t * (r.k + g);
    }
}

static int check_text(const std::string &t, uint32_t F, unsigned long long *n)
{
    uint64_t h, l;
    planes_of(t, &h, &l);
    uint32_t sum, oof, want_sum, want_oof;
    mh_score(h, l, F, &sum, &oof);
    by_rows(t, F, &want_sum, &want_oof);
    ++*n;
    return sum == want_sum && oof == want_oof && oof <= sum ? 0 : 2;
}

int main()
{
    std::srand(26);
    unsigned long long texts = 0, loci = 0, defined = 0, classes[kEffClasses] = {};
    for (uint32_t d = 0; d < 64; ++d)
        if (mh_weight(d) != (uint32_t)std::lround(std::round(std::exp(-(double)d / 20.0) * 1000.0))) return 1;

    // ---- mh_score over the families ----
    const uint32_t flanks[5] = {8, 9, 16, 30, 32};
    for (uint32_t F : flanks) {
        const uint32_t W = 2 * F;
        std::vector<std::string> family;
        for (int i = 0; i < 40; ++i) family.push_back(random_text(W));
        for (int i = 0; i < 10; ++i) {
            const std::string half = random_text(F);
            family.push_back(half + half);
            for (uint32_t at : {0u, F - 1, (uint32_t)std::rand() % F}) {
                std::string other = half;
                other[at] = "ACGT"[(code(half[at]) + 1 + std::rand() % 3) % 4];
                family.push_back(half + other);
                family.push_back(other + half);
            }
        }
        for (uint32_t period = 1; period <= 4; ++period)
            for (int i = 0; i < 4; ++i) {
                const std::string unit = period == 1 ? std::string(1, "ACGT"[i]) : random_text(period);
                std::string t;
                while (t.size() < W) t += unit;
                family.push_back(t.substr(0, W));
            }
        for (const char *pair : {"AT", "GC", "AG", "CT"})
            for (int i = 0; i < 4; ++i) family.push_back(random_text(W, pair, 2));
        family.push_back(std::string(F, 'A') + std::string(F, 'C'));
        for (uint32_t d : {F - 1, F, F + 1}) {
            std::string t = std::string(F, 'A') + std::string(F, 'C');
            t.replace(2, 2, "GT");
            t.replace(2 + d, 2, "GT");
            family.push_back(t);
        }
        for (const std::string &t : family)
            if (const int rc = check_text(t, F, &texts)) return rc;
    }

    // ---- mh_context: contigs of F - 1, F, 2 F - 1, 2 F, 2 F + 1, 260 (three N at 100, a tandem duplication of F bases at 130)
    // and 90 bases, one N apart ----
    for (uint32_t F : {8u, 32u}) {
        const uint32_t W = 2 * F, site_len = 23;
        const uint32_t lens[7] = {F - 1, F, 2 * F - 1, 2 * F, 2 * F + 1, 260, 90};
        std::vector<std::string> contig;
        std::vector<uint32_t> off, end;
        std::string genome;
        for (uint32_t len : lens) {
            std::string t = random_text(len);
            if (len == 260) {
                t.replace(100, 3, "NNN");
                t.replace(130 + F, F, t, 130, F);
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
        for (uint32_t cut : {0u, 17u, 23u}) {
            const MhShape s{site_len, cut, F};
            if (!mh_shape_valid(s)) return 3;
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
                        const long long start = (long long)p + (strand ? (long long)site_len - cut : (long long)cut) - F;
                        if (start < 0 || start + W > (long long)contig[c].size()) want = kEffOffContig;
                        else {
                            const uint64_t g0 = (uint64_t)off[c] + (uint64_t)start;
                            if (g0 < first * 32 || g0 + W > (first + held) * 32) want = kEffNotResident;
                            else {
                                text = contig[c].substr((size_t)start, W);
                                if (text.find('N') != std::string::npos) want = kEffHasN;
                                else if (strand) text = revcomp(text);
                            }
                        }
                    }
                    uint64_t h = 0, l = 0;
                    const uint32_t got = mh_context(g, s, c, p, strand, &h, &l);
                    if (got != want) return 4;
                    ++loci;
                    ++classes[got];
                    if (got != kEffDefined) return 0;
                    uint64_t wh, wl;
                    planes_of(text, &wh, &wl);
                    if (h != wh || l != wl) return 5;
                    ++defined;
                    return check_text(text, F, &texts);
                };
                for (uint32_t c = 0; c < contig.size(); ++c)
                    for (uint32_t p = 0; p <= contig[c].size() + 2; ++p)  // (the last starts leave the contig: invalid)
                        for (uint32_t strand = 0; strand < 2; ++strand)
                            if (const int rc = check(c, p, strand)) return rc;
                const uint32_t bad[][3] = {{7, 0, 0}, {0xFFFFFFFFu, 0, 0}, {5, 10, 2}, {5, 260 - site_len + 1, 0}, {5, 0xFFFFFFFFu, 1},
                                           {6, 0xFFFFFFF0u, 0}, {5, 10, 0xFFFFFFFFu}};
                for (const auto &b : bad) {
                    uint64_t h, l;
                    if (mh_context(g, s, b[0], b[1], b[2], &h, &l) != kEffInvalid) return 6;
                }
            }
        }
    }
    // the shapes the definition refuses, and the filter rule at its edges
    const MhShape refused[] = {{23, 17, 7}, {23, 17, 33}, {23, 24, 30}, {15, 10, 30}, {33, 17, 30}, {23, 0xFFFFFFFFu, 30}, {23, 17, 0xFFFFFFF8u}};
    for (const MhShape &s : refused)
        if (mh_shape_valid(s)) return 7;
    if (!mh_keep(kEffDefined, 1098, 732, 1098, 666) || mh_keep(kEffDefined, 1098, 732, 1099, 0) || mh_keep(kEffDefined, 1098, 732, 0, 667)) return 8;
    if (!mh_keep(kEffDefined, 3, 2, 0, 666) || !mh_keep(kEffDefined, 3000, 2001, 0, 667) || !mh_keep(kEffDefined, 0, 0, 0, 0) ||
        mh_keep(kEffDefined, 0, 0, 0, 1) || mh_keep(kEffHasN, kMhUndefined, kMhUndefined, 0, 0) || !mh_keep(kEffDefined, 4100000, 4100000, 0, 1000))
        return 9;
    for (uint32_t k = 0; k < kEffClasses; ++k)
        if (classes[k] == 0) return 10;
    std::printf("ok: %llu contexts, %llu loci (%llu defined)\n", texts, loci, defined);
    return 0;
}
