// fold_check.cpp - the self-complementarity of varscot_amd/csrc/vsc_fold.h (fold_shape_valid, fold_scaffold_windows, fold_row,
// fold_keep, fold_context and what they call) in a stand-alone program with its own main, for the host sanitizers.  No device is
// opened and no kernel is launched.  Build and run on the CPU:
//   hipcc --offload-arch=gfx950 -x hip -O1 -g -std=c++17 -Iinclude -Ivarscot_amd/csrc -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tools/fold_check.cpp -o build/fold_check && build/fold_check
//   - fold_row over the planes of random and planted spacers (hairpins at the shortest loop and one shorter, arms at both ends,
//     palindromes, two-letter alphabets, the reverse complement of scaffold words at both scaffold ends and across the 32-letter
//     boundaries) for random shapes - n 12 .. 32, k 3 .. 8, every gc_min, min_loop 0 .. 16, a random seed, WOBBLE on and off - and
//     scaffolds of 0 .. 128 letters, the window array of exactly n + m - 1 elements, against a brute-force walk on LETTERS: every
//     (i, j, L) tested pair by pair;
//   - fold_context over a small genome packed into plane arrays of exactly the held words - every (contig, position, strand),
//     the loci the definition calls invalid, the whole genome and a view that starts at word 1 and ends one word early - against
//     the class and the spacer taken from the text by slicing and reverse complement;
//   - fold_shape_valid and fold_keep at their bounds.
// Exit code 0 and "ok" when all agree.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "vsc_fold.h"

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

static bool pair(char a, char b, bool wobble)
{
    if (code(a) + code(b) == 3) return true;
    return wobble && ((a == 'G' && b == 'T') || (a == 'T' && b == 'G'));
}

// the definition on letters
static void by_letters(const std::string &g, const std::string &s, const FoldShape &sh, uint32_t *w0, uint32_t *w1)
{
    const int n = (int)g.size(), m = (int)s.size(), k = (int)sh.stem, loop = (int)sh.min_loop;
    const bool wob = sh.flags & kFoldWobble;
    auto qual = [&](int i) {
        int gc = 0;
        for (int t = 0; t < k; ++t) gc += g[i + t] == 'G' || g[i + t] == 'C';
        return gc >= (int)sh.gc_min;
    };
    auto self_stem = [&](int i, int j, int L) {
        if (i + L + loop > j || j + L > n) return false;
        for (int t = 0; t < L; ++t)
            if (!pair(g[i + t], g[j + L - 1 - t], wob)) return false;
        return true;
    };
    auto scaf_stem = [&](int i, int j, int L) {
        if (i + L > n || j + L > m) return false;
        for (int t = 0; t < L; ++t)
            if (!pair(g[i + t], s[j + L - 1 - t], wob)) return false;
        return true;
    };
    std::vector<char> self5(n, 0), scaf5(n, 0), covered(n, 0);
    for (int i = 0; i + k <= n; ++i) {
        if (!qual(i)) continue;
        for (int j = 0; j + k <= n; ++j)
            if (self_stem(i, j, k)) {
                self5[i] = 1;
                for (int t = 0; t < k; ++t) covered[i + t] = covered[j + t] = 1;
            }
        for (int j = 0; j + k <= m; ++j)
            if (scaf_stem(i, j, k)) {
                scaf5[i] = 1;
                for (int t = 0; t < k; ++t) covered[i + t] = 1;
            }
    }
    uint32_t starts = 0, n_self = 0, n_scaf = 0, seed = 0, self_longest = 0, scaf_longest = 0;
    for (int i = 0; i < n; ++i) {
        starts += self5[i] || scaf5[i];
        n_self += self5[i];
        n_scaf += scaf5[i];
        seed += covered[i] && i >= (int)sh.seed_start && i < (int)(sh.seed_start + sh.seed_len);
    }
    for (int L = 1; L <= n; ++L)
        for (int i = 0; i < n; ++i) {
            for (int j = 0; j < n; ++j)
                if (self_stem(i, j, L)) self_longest = (uint32_t)L;
            for (int j = 0; j < m; ++j)
                if (scaf_stem(i, j, L)) scaf_longest = (uint32_t)L;
        }
    *w0 = starts | n_self << 8 | n_scaf << 16 | seed << 24;
    *w1 = self_longest | scaf_longest << 8;
}

static int failures = 0;
static void fail(const char *what, const std::string &a, const std::string &b)
{
    if (++failures <= 10) std::fprintf(stderr, "MISMATCH %s: %s %s\n", what, a.c_str(), b.c_str());
}

static std::string shape_text(const FoldShape &s)
{
    char buf[160];
    std::snprintf(buf, sizeof buf, "(%u %u %u k=%u gc=%u loop=%u seed=%u,%u flags=%u)", s.site_len, s.proto_start, s.proto_len, s.stem, s.gc_min,
                  s.min_loop, s.seed_start, s.seed_len, s.flags);
    return buf;
}

static uint64_t check_rows(const std::string &g, const std::string &s, const FoldShape &sh)
{
    const uint32_t n = (uint32_t)g.size(), m = (uint32_t)s.size();
    uint32_t gh = 0, gl = 0;
    for (uint32_t a = 0; a < n; ++a) {
        gh |= (uint32_t)(code(g[a]) >> 1) << a;
        gl |= (uint32_t)(code(g[a]) & 1) << a;
    }
    std::vector<uint8_t> letters(m);  // exactly m letters, exactly n + m - 1 windows: a read past either is the sanitizer's
    for (uint32_t j = 0; j < m; ++j) letters[j] = (uint8_t)code(s[j]);
    std::vector<FoldWindow> win(fold_diagonals(n, m));
    fold_scaffold_windows(letters.data(), m, n, win.data());
    uint32_t w0, w1, b0, b1;
    fold_row(gh, gl, FoldScaffold{win.data(), (uint32_t)win.size()}, sh, &w0, &w1);
    by_letters(g, s, sh, &b0, &b1);
    if (w0 != b0 || w1 != b1) {
        char buf[96];
        std::snprintf(buf, sizeof buf, " got %08x %08x want %08x %08x", w0, w1, b0, b1);
        fail("fold_row", g + " / " + s + " " + shape_text(sh), buf);
    }
    return 1;
}

static std::string plant(uint32_t n, char background, std::initializer_list<std::pair<uint32_t, std::string>> pieces)
{
    std::string t(n, background);
    for (const auto &p : pieces)
        if (p.first + p.second.size() <= n) t.replace(p.first, p.second.size(), p.second);
    return t;
}

int main()
{
    std::srand(35);
    uint64_t rows = 0, contexts = 0;
    const uint32_t scaffold_lengths[] = {0, 2, 3, 7, 8, 20, 31, 32, 33, 64, 65, 76, 96, 97, 128};
    for (int round = 0; round < 400; ++round) {
        FoldShape sh{};
        sh.proto_len = 12 + std::rand() % 21;
        if (round % 7 == 0) sh.proto_len = 32;
        sh.proto_start = 0;
        sh.site_len = sh.proto_len < 16 ? 16 : sh.proto_len;
        sh.stem = 3 + std::rand() % 6;
        sh.gc_min = std::rand() % (sh.stem + 1);
        sh.min_loop = std::rand() % 17;
        if (round % 3 == 0) sh.min_loop = std::rand() % 4;
        sh.seed_start = std::rand() % 17;
        if (sh.seed_start > sh.proto_len) sh.seed_start = sh.proto_len;
        const uint32_t room = sh.proto_len - sh.seed_start;
        sh.seed_len = std::rand() % ((room < 16 ? room : 16) + 1);
        sh.flags = round & 1;
        if (!fold_shape_valid(sh)) fail("fold_shape_valid", shape_text(sh), "refused");
        const uint32_t n = sh.proto_len, k = sh.stem, loop = sh.min_loop;
        const uint32_t m = scaffold_lengths[round % 15];
        const std::string s = random_text(m);
        std::vector<std::string> spacers;
        spacers.push_back(random_text(n));
        spacers.push_back(random_text(n, "GC", 2));
        spacers.push_back(random_text(n, "GT", 2));
        spacers.push_back(random_text(n, "AC", 2));
        spacers.push_back(std::string(n, 'A'));
        const std::string arm = random_text(k, "GC", 2), arm2 = random_text(k + 2);
        if (2 * k + loop <= n) {
            spacers.push_back(plant(n, 'A', {{0, arm}, {k + loop, revcomp(arm)}}));
            spacers.push_back(plant(n, 'A', {{0, arm}, {n - k, revcomp(arm)}}));
            spacers.push_back(plant(n, 'C', {{0, std::string(k, 'G')}, {n - k, std::string(k, 'T')}}));
        }
        if (loop && 2 * k + loop - 1 <= n) spacers.push_back(plant(n, 'A', {{1, arm}, {k + loop, revcomp(arm)}}));
        if (2 * (k + 2) + loop <= n) spacers.push_back(plant(n, 'C', {{0, arm2}, {n - k - 2, revcomp(arm2)}}));
        const std::string half = random_text(n / 2);
        spacers.push_back((half + revcomp(half) + "A").substr(0, n));
        if (m >= k) {
            const uint32_t at[] = {0, m - k, 32 - k / 2, 64 - k / 2, 96 - k / 2};
            for (uint32_t j : at)
                if (j + k <= m) {
                    spacers.push_back(plant(n, 'A', {{0, revcomp(s.substr(j, k))}}));
                    spacers.push_back(plant(n, 'C', {{n - k, revcomp(s.substr(j, k))}}));
                }
            const uint32_t width = m < n ? m : n;
            spacers.push_back(plant(n, 'A', {{n - width, revcomp(s.substr(m - width, width))}}));
        }
        for (const std::string &g : spacers) rows += check_rows(g, s, sh);
    }
    // the full spacer against its own reverse complement as the scaffold: a stem of 32
    {
        FoldShape sh{32, 0, 32, 8, 0, 0, 16, 16, 0};
        const std::string g = random_text(32);
        rows += check_rows(g, revcomp(g), sh);
        rows += check_rows(g, random_text(48) + revcomp(g) + random_text(48), sh);
    }

    // fold_shape_valid and fold_keep at their bounds
    {
        const FoldShape ok{23, 0, 20, 4, 2, 3, 8, 12, 0};
        FoldShape bad[] = {ok, ok, ok, ok, ok, ok, ok, ok, ok, ok, ok, ok};
        bad[0].site_len = 15, bad[1].site_len = 33, bad[2].proto_len = 11, bad[3].proto_start = 4, bad[4].stem = 2, bad[5].stem = 9;
        bad[6].gc_min = 5, bad[7].min_loop = 17, bad[8].seed_start = 17, bad[9].seed_len = 13, bad[10].flags = 2, bad[11].proto_len = 33;
        if (!fold_shape_valid(ok)) fail("fold_shape_valid", shape_text(ok), "refused");
        for (const FoldShape &b : bad)
            if (fold_shape_valid(b)) fail("fold_shape_valid", shape_text(b), "accepted");
        const FoldLimits none{kFoldNoLimit, kFoldNoLimit, kFoldNoLimit, kFoldNoLimit};
        const uint32_t w0 = 3u | 2u << 8 | 1u << 16 | 5u << 24, w1 = 6u | 7u << 8;
        if (!fold_keep(kEffDefined, w0, w1, none) || fold_keep(kEffHasN, w0, w1, none) || fold_keep(kEffInvalid, kFoldUndefined, kFoldUndefined, none))
            fail("fold_keep", "no limit", "");
        const FoldLimits at{3, 6, 7, 5};
        const FoldLimits below[] = {{2, 6, 7, 5}, {3, 5, 7, 5}, {3, 6, 6, 5}, {3, 6, 7, 4}};
        if (!fold_keep(kEffDefined, w0, w1, at)) fail("fold_keep", "at the limits", "");
        for (const FoldLimits &l : below)
            if (fold_keep(kEffDefined, w0, w1, l)) fail("fold_keep", "one below", "");
        if (!fold_limits_valid(at) || !fold_limits_valid(none) || fold_limits_valid(FoldLimits{33, 0, 0, 0}) ||
            fold_limits_valid(FoldLimits{0, 0, 0, 0xFFFFFFFEu}))
            fail("fold_limits_valid", "", "");
    }

    // fold_context over a small genome: plane arrays of exactly the held words
    {
        std::vector<std::string> contigs = {random_text(22), random_text(23), random_text(27), random_text(140), random_text(61)};
        contigs[3].replace(50, 3, "NNN");
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
        const FoldShape shapes[] = {{23, 0, 20, 4, 2, 3, 8, 12, 0}, {27, 4, 23, 4, 2, 3, 0, 6, 0}, {16, 4, 12, 3, 0, 0, 0, 0, 0}, {32, 0, 32, 8, 4, 16, 16, 16, 1}};
        for (int view = 0; view < 2; ++view) {
            const uint64_t first = view ? 1 : 0, held = view ? words - 2 : words;
            const std::vector<uint32_t> vh(hi.begin() + first, hi.begin() + first + held), vl(lo.begin() + first, lo.begin() + first + held),
                vn(nm.begin() + first, nm.begin() + first + held);
            const EffPlanes g{vh.data(), vl.data(), vn.data(), first, held, held, off.data(), end.data(), (uint32_t)contigs.size()};
            for (const FoldShape &sh : shapes) {
                std::vector<uint32_t> loci;
                for (uint32_t c = 0; c <= contigs.size(); ++c)
                    for (uint32_t p = 0; p <= 141; ++p)
                        for (uint32_t strand = 0; strand < 3; ++strand) loci.insert(loci.end(), {c, p, strand});
                loci.insert(loci.end(), {0xFFFFFFFFu, 0u, 0u, 3u, 0xFFFFFFFFu, 1u, 3u, 0xFFFFFFFFu - 22u, 0u});
                for (size_t q = 0; q < loci.size(); q += 3) {
                    const uint32_t c = loci[q], p = loci[q + 1], strand = loci[q + 2];
                    uint32_t want = kEffDefined;
                    std::string spacer;
                    if (c >= contigs.size() || strand > 1 || (uint64_t)p + sh.site_len > contigs[c].size()) {
                        want = kEffInvalid;
                    } else if ((uint64_t)off[c] + p < first * 32 || (uint64_t)off[c] + p + sh.site_len > (first + held) * 32) {
                        want = kEffNotResident;
                    } else {
                        std::string site = contigs[c].substr(p, sh.site_len);
                        if (site.find('N') != std::string::npos) want = kEffHasN;
                        if (strand) site = revcomp(site);
                        spacer = site.substr(sh.proto_start, sh.proto_len);
                    }
                    uint32_t gh = 0, gl = 0;
                    const uint32_t got = fold_context(g, sh, c, p, strand, &gh, &gl);
                    ++contexts;
                    if (got != want) {
                        fail("fold_context class", std::to_string(c) + ":" + std::to_string(p) + ":" + std::to_string(strand),
                             std::to_string(got) + " want " + std::to_string(want));
                        continue;
                    }
                    if (want != kEffDefined) continue;
                    uint32_t wh = 0, wl = 0;
                    for (uint32_t a = 0; a < sh.proto_len; ++a) {
                        wh |= (uint32_t)(code(spacer[a]) >> 1) << a;
                        wl |= (uint32_t)(code(spacer[a]) & 1) << a;
                    }
                    if (gh != wh || gl != wl) fail("fold_context planes", spacer, shape_text(sh));
                }
            }
        }
    }
    if (failures) {
        std::fprintf(stderr, "%d mismatches\n", failures);
        return 1;
    }
    std::printf("ok: %llu rows against the walk on letters, %llu loci against the text\n", (unsigned long long)rows, (unsigned long long)contexts);
    return 0;
}
