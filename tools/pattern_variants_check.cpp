// pattern_variants_check.cpp - the __host__ __device__ functions of varscot_amd/csrc/vsc_varmap.h and vsc_pattern_variants.h
// that the pattern variant screen shares between the host calls and the kernels - var_covered / varmap_walk /
// var_tags_equal with a site length, site_mask / site_bits / plane_site, shadow_search - in a stand-alone program with its own
// main, for the host sanitizers.  No device is opened and no kernel is launched.  Build and run on the CPU:
//   hipcc --offload-arch=gfx950 -x hip -O1 -g -std=c++17 -Iinclude -Ivarscot_amd/csrc -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tools/pattern_variants_check.cpp -o build/pattern_variants_check && build/pattern_variants_check
// Random maps (windows with 0..6 variants: substitutions, insertions, deletions; starts that wrapped), every L in 16..32 and
// every window position: the walk against a naive restatement of getSnpType in 64-bit arithmetic, the tag comparison against
// the lists of covered tag ids; synthetic planes whose arrays end exactly at the last word: the L bases of a site at every bit
// offset (0, word-straddling, the plane's last word) against a bit-by-bit loop; random interval sets (nested, overlapping,
// touching, up to the top of the 32-bit range): the interval search against a loop over the intervals.  Exit code 0 and "ok"
// when all agree.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "vsc_pattern_variants.h"

using namespace vsc;

static unsigned long long g_checks = 0;
#define CHECK(cond, ...)                          \
    do {                                          \
        ++g_checks;                               \
        if (!(cond)) {                            \
            std::fprintf(stderr, "FAILED %s:%d: %s\n  ", __FILE__, __LINE__, #cond); \
            std::fprintf(stderr, __VA_ARGS__);    \
            std::fprintf(stderr, "\n");           \
            std::exit(1);                         \
        }                                         \
    } while (0)

// getSnpType (variant_processing/filter_output_bam.h:189-263) for the len bases from pos1 on, naively: the covered tag ids in
// order, and the shift of the uncovered indels met before the first covered variant
static void naive_walk(const std::vector<VarEntry> &vars, uint32_t pos1, uint32_t len, uint32_t *pos2, std::vector<uint32_t> *tags)
{
    tags->clear();
    long long count = 0;
    bool found = false;
    const long long lo = pos1, hi = (long long)pos1 + len;
    auto inside = [&](long long q) { return lo <= q && q < hi; };
    for (const VarEntry &v : vars) {
        const long long p = v.p, lr = v.len_ref, la = v.len_alt;
        bool cov;
        if (lr == la) cov = inside(p);
        else if (lr < la) cov = inside(p + 1) || inside(p + la - 1);
        else cov = inside(p + 1) || inside(p + lr - 1);
        if (cov) {
            tags->push_back(v.tag_id);
            found = true;
        } else if (!found && lr != la) count += lr - la;
    }
    *pos2 = (uint32_t)((long long)pos1 + count);
}

static void check_walk(std::mt19937_64 &rng)
{
    auto rnd = [&](uint32_t n) { return (uint32_t)(rng() % n); };
    for (int round = 0; round < 60; ++round) {
        const uint32_t n_win = 1 + rnd(12);
        std::vector<VarWindow> win;
        std::vector<VarEntry> var;
        std::vector<uint32_t> win_len;
        uint32_t next_tag = 0;
        for (uint32_t w = 0; w < n_win; ++w) {
            const uint32_t start = rnd(8) == 0 ? (uint32_t)-(int)(1 + rnd(30)) : rnd(5000);  // (a start that wrapped)
            win.push_back(VarWindow{rnd(3), start, (uint32_t)var.size(), rnd(3)});
            const uint32_t k = rnd(7);
            int p = (int)start + (int)rnd(20);
            for (uint32_t i = 0; i < k; ++i) {
                const uint32_t kind = rnd(3), a = 1 + rnd(6), b = 1 + rnd(6);
                const uint32_t lr = kind == 0 ? a : kind == 1 ? 1u : a + 1, la = kind == 0 ? a : kind == 1 ? b + 1 : 1u;
                // the tag id of (chromosome, position): the same pair in two windows of one chromosome gets the same id sometimes
                var.push_back(VarEntry{p, lr, la, rnd(4) == 0 && next_tag ? rnd(next_tag) : next_tag++});
                p += 1 + (int)rnd(25);
            }
            win_len.push_back(40 + rnd(90));
        }
        win.push_back(VarWindow{UINT32_MAX, 0u, (uint32_t)var.size(), UINT32_MAX});
        // the arrays end exactly where the tables end: a read behind them is the sanitizer's to find
        const VarMapView m{win.data(), var.data(), n_win, (uint32_t)var.size()};
        std::vector<std::vector<uint32_t>> tags_at;
        for (uint32_t len = kPatVarMinLen; len <= kPatVarMaxLen; ++len) {
            for (uint32_t w = 0; w < n_win; ++w) {
                const std::vector<VarEntry> mine(var.begin() + win[w].var_off, var.begin() + win[w + 1].var_off);
                tags_at.assign(win_len[w], {});
                for (uint32_t pos = 0; pos < win_len[w]; ++pos) {
                    uint32_t pos2, n_var, want2;
                    varmap_walk(m, w, pos, len, &pos2, &n_var);
                    naive_walk(mine, pos + win[w].start, len, &want2, &tags_at[pos]);
                    CHECK(pos2 == want2 && n_var == tags_at[pos].size(), "walk: window %u pos %u len %u: %u %u, want %u %zu", w, pos, len, pos2,
                          n_var, want2, tags_at[pos].size());
                }
                // the tag comparison: this window's positions among themselves and against another window's first positions
                const uint32_t w2 = rnd(n_win);
                const std::vector<VarEntry> other(var.begin() + win[w2].var_off, var.begin() + win[w2 + 1].var_off);
                for (uint32_t pos = 0; pos < win_len[w]; pos += 1 + rnd(3)) {
                    const uint32_t n = (uint32_t)tags_at[pos].size();
                    if (n == 0) continue;
                    for (uint32_t q = 0; q < win_len[w]; q += 1 + rnd(5))
                        if (tags_at[q].size() == n)
                            CHECK(var_tags_equal(m, w, pos, w, q, n, len) == (tags_at[pos] == tags_at[q]), "tags: window %u pos %u %u len %u", w, pos, q, len);
                    for (uint32_t q = 0; q < win_len[w2]; q += 1 + rnd(5)) {
                        uint32_t p2;
                        std::vector<uint32_t> t2;
                        naive_walk(other, q + win[w2].start, len, &p2, &t2);
                        if (t2.size() == n)
                            CHECK(var_tags_equal(m, w, pos, w2, q, n, len) == (tags_at[pos] == t2), "tags: windows %u %u pos %u %u len %u", w, w2, pos, q, len);
                    }
                }
            }
        }
    }
}

static void check_sites(std::mt19937_64 &rng)
{
    for (uint32_t len = 1; len <= 32; ++len) {
        const uint32_t want = len == 32 ? 0xFFFFFFFFu : (1u << len) - 1u;
        CHECK(site_mask(len) == want, "mask %u", len);
    }
    for (int round = 0; round < 200; ++round) {
        const unsigned long long n_words = 1 + rng() % 6;
        std::vector<uint32_t> plane(n_words);  // (exactly n_words: the word behind the last must not be read)
        for (auto &w : plane) w = (uint32_t)rng();
        auto bit = [&](unsigned long long k) { return k < 32 * n_words ? (plane[k >> 5] >> (k & 31)) & 1u : 0u; };
        for (uint32_t len = kPatVarMinLen; len <= kPatVarMaxLen; ++len)
            for (unsigned long long rel = 0; rel < 32 * n_words; ++rel) {
                uint32_t want = 0;
                for (uint32_t j = 0; j < len; ++j) want |= bit(rel + j) << j;
                const uint32_t got = plane_site(plane.data(), n_words, rel, len);
                CHECK(got == want, "site: %llu words, bit %llu, len %u: %08x, want %08x", n_words, rel, len, got, want);
            }
    }
    // the word pair itself: every shift, the lengths at both ends
    for (int round = 0; round < 2000; ++round) {
        const uint32_t w0 = (uint32_t)rng(), w1 = (uint32_t)rng();
        for (uint32_t sh = 0; sh < 32; ++sh)
            for (uint32_t len : {16u, 17u, 31u, 32u}) {
                uint32_t want = 0;
                for (uint32_t j = 0; j < len; ++j) {
                    const uint32_t k = sh + j;
                    want |= ((k < 32 ? w0 >> k : w1 >> (k - 32)) & 1u) << j;
                }
                CHECK(site_bits(w1, w0, sh, len) == want, "bits: shift %u len %u", sh, len);
            }
    }
}

static void check_intervals(std::mt19937_64 &rng)
{
    for (int round = 0; round < 400; ++round) {
        const uint32_t n = (uint32_t)(rng() % 40);
        const bool top = round % 5 == 0;  // intervals and sites at the top of the 32-bit range: pos + len does not wrap
        const uint32_t base = top ? 0xFFFFFFFFu - 600u : 20u + (uint32_t)(rng() % 1000);
        std::vector<std::pair<uint32_t, uint32_t>> iv;
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t s = base + (uint32_t)(rng() % 500);
            const unsigned long long e = (unsigned long long)s + 1 + rng() % 90;
            iv.emplace_back(s, (uint32_t)std::min<unsigned long long>(e, 0xFFFFFFFFull));
        }
        std::sort(iv.begin(), iv.end());
        std::vector<uint32_t> start, end_max;
        uint32_t run = 0;
        for (const auto &i : iv) {
            run = std::max(run, i.second);
            start.push_back(i.first);
            end_max.push_back(run);
        }
        for (uint32_t len = kPatVarMinLen; len <= kPatVarMaxLen; ++len)
            for (uint32_t k = 0; k < 640; ++k) {
                const unsigned long long p64 = (unsigned long long)base - 20 + k;
                if (p64 > 0xFFFFFFFFull) break;
                const uint32_t pos = (uint32_t)p64;
                bool want = false;
                for (const auto &i : iv) want = want || (i.first <= pos && (unsigned long long)pos + len <= i.second);
                CHECK(shadow_search(start.data(), end_max.data(), n, pos, len) == want, "intervals: round %d pos %u len %u", round, pos, len);
            }
        CHECK(!shadow_search(nullptr, nullptr, 0, 5, 23), "no interval");
    }
}

int main()
{
    std::mt19937_64 rng(20251020);
    check_walk(rng);
    check_sites(rng);
    check_intervals(rng);
    std::printf("pattern_variants_check: ok (%llu comparisons)\n", g_checks);
    return 0;
}
