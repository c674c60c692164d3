// bulge_table_check.cpp - the table score of bulged alignments and cut sites of varscot_amd/csrc/vsc_bulge_table.h
// (bulge_table_score, bulge_table_member, site_table_scores, span_revcomp, bulge_table_valid) in a stand-alone program with its
// own main, for the host sanitizers.  No device is opened and no kernel is launched.  Build and run on the CPU:
//   hipcc --offload-arch=gfx950 -x hip -O1 -g -std=c++17 -ffp-contract=off -Iinclude -Ivarscot_amd/csrc -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tools/bulge_table_check.cpp -o build/bulge_table_check && build/bulge_table_check
// Random shapes (L 16..32, a protospacer of at least four positions anywhere, 0..4 PAM positions), random tables (weights of
// exactly 0 and 1 among them, in dna and rna too), random IUPAC guides and random sites: for every d and EVERY split point the
// planes' score against a naive letter loop in the definition's order, bit for bit; the all-ones anchor against
// pattern_table_score of the paired site; alignments outside the definition (score 0.0, no weight read: the weight array is
// exactly as long as the shape needs); the member loop of a site over one span, both anchors, against the same loop over
// separately cut letters; the tables the definition refuses.  Exit code 0 and "ok" when all agree.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "vsc_bulge_table.h"

using namespace vsc;

static bool same(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }
static bool is_single(uint8_t set) { return set && (set & (set - 1)) == 0; }

static void site_planes(const uint8_t *c, uint32_t len, uint32_t *h, uint32_t *l)
{
    *h = *l = 0;
    for (uint32_t j = 0; j < len; ++j) {
        *h |= (uint32_t)(c[j] >> 1) << j;
        *l |= (uint32_t)(c[j] & 1u) << j;
    }
}

// the definition, letter by letter: sets = the guide's L sets, s = the site's L + d codes, split point i
static double naive(const double *w, const PatTableShape &sh, const uint8_t *sets, const uint8_t *s, int d, uint32_t i)
{
    const uint32_t a = sh.ps_start, L = sh.len, b = (uint32_t)(d < 0 ? -d : d);
    double x = 1.0;
    for (uint32_t k = 0; k < sh.ps_len; ++k) {
        const uint32_t j = a + k;
        int q;  // the paired site letter, -1: none
        if (d > 0) q = j < i ? s[j] : s[j + b];
        else q = j < i ? s[j] : j >= i + b ? s[j - b] : -1;
        if (q < 0 || !is_single(sets[j])) continue;
        const uint32_t g = (uint32_t)__builtin_ctz(sets[j]);
        if (g != (uint32_t)q) x = x * w[(k * 4 + g) * 4 + (uint32_t)q];
    }
    uint32_t key = 0;
    for (uint32_t t = 0; t < sh.n_pam; ++t) {
        const uint32_t j = sh.pam_pos[t];
        key = 4 * key + (d > 0 ? (j < i ? s[j] : s[j + b]) : (j < i ? s[j] : s[j - b]));
    }
    x = x * w[pattern_table_pairs(sh) + key];
    (void)L;
    if (d > 0)
        for (uint32_t t = 0; t < b; ++t) x = x * w[bulge_table_dna_at(sh) + (i - a) * 4 + s[i + t]];
    else
        for (uint32_t t = 0; t < b; ++t)
            if (is_single(sets[i + t])) x = x * w[bulge_table_rna_at(sh) + (i + t - a) * 4 + (uint32_t)__builtin_ctz(sets[i + t])];
    return x;
}

// NM and the smallest split point that reaches it, letter by letter
static uint32_t naive_align(const PatTableShape &sh, const uint8_t *sets, const uint8_t *s, int d, uint32_t *index)
{
    const uint32_t a = sh.ps_start, e = a + sh.ps_len, b = (uint32_t)(d < 0 ? -d : d);
    uint32_t best = ~0u;
    for (uint32_t i = a + 1; i + (d < 0 ? b : 0u) <= e - 1; ++i) {
        uint32_t nm = 0;
        for (uint32_t j = 0; j < sh.len; ++j) {
            int q;
            if (d > 0) q = j < i ? s[j] : s[j + b];
            else q = j < i ? s[j] : j >= i + b ? s[j - b] : -1;
            if (q >= 0 && !((sets[j] >> q) & 1u)) ++nm;
        }
        if (nm < best) best = nm, *index = i;
    }
    return best;
}

int main()
{
    std::srand(41);
    unsigned long long checked = 0;
    for (int t = 0; t < 200; ++t) {
        PatTableShape sh{};
        // L + d must stay inside 16..32 for every d that is tried: 18..30
        sh.len = 18 + (uint32_t)(std::rand() % 13);
        sh.ps_len = 4 + (uint32_t)std::rand() % (sh.len - 3);
        sh.ps_start = (uint32_t)std::rand() % (sh.len - sh.ps_len + 1);
        std::vector<uint32_t> outside;
        for (uint32_t j = 0; j < sh.len; ++j)
            if (j < sh.ps_start || j >= sh.ps_start + sh.ps_len) outside.push_back(j);
        const uint32_t room = outside.size() < 4 ? (uint32_t)outside.size() : 4u;
        sh.n_pam = (uint32_t)std::rand() % (room + 1);
        for (uint32_t k = 0, from = 0; k < sh.n_pam; ++k) {
            const uint32_t left = sh.n_pam - k, span = (uint32_t)outside.size() - from - (left - 1);
            const uint32_t pick = from + (uint32_t)std::rand() % span;
            sh.pam_pos[k] = outside[pick];
            from = pick + 1;
        }
        const uint32_t n_w = bulge_table_weights(sh), a = sh.ps_start, e = a + sh.ps_len;
        if (n_w > kBulgeTableMaxWeights) return 1;
        std::vector<double> w(n_w);  // exactly as many doubles as the shape needs: a read past the end is the sanitizer's to find
        for (uint32_t i = 0; i < n_w; ++i) {
            const int r = std::rand() % 16;
            w[i] = r == 0 ? 0.0 : r == 1 ? 1.0 : (double)(std::rand() % 100000 + 1) / 100001.0;
        }
        for (uint32_t i = 0; i < sh.ps_len; ++i)
            for (uint32_t b = 0; b < 4; ++b) w[(i * 4 + b) * 4 + b] = 1.0;
        if (!bulge_table_valid(sh, w.data())) return 2;
        std::vector<double> ones = w;
        for (uint32_t i = bulge_table_dna_at(sh); i < n_w; ++i) ones[i] = 1.0;
        for (int trial = 0; trial < 60; ++trial) {
            uint8_t sets[32], span[34];
            for (uint32_t j = 0; j < sh.len; ++j)
                sets[j] = std::rand() % 4 ? (uint8_t)(1u << (std::rand() % 4)) : (uint8_t)(1 + std::rand() % 15);  // any IUPAC set
            for (uint32_t j = 0; j < sh.len + 2; ++j) {
                span[j] = (uint8_t)(std::rand() % 4);
                if (j < sh.len && std::rand() % 3 && is_single(sets[j])) span[j] = (uint8_t)__builtin_ctz(sets[j]);  // mostly the guide's base
            }
            const BulgeGuide g = bulge_table_guide(sets, sh.len);
            for (int d = -2; d <= 2; ++d) {
                if (d == 0) continue;
                const uint32_t m = (uint32_t)((int)sh.len + d), b = (uint32_t)(d < 0 ? -d : d);
                uint32_t ph, pl;
                site_planes(span, m, &ph, &pl);
                // garbage behind the site must change nothing
                const uint32_t high = m < 32 ? ~0u << m : 0u, jh = ph | ((uint32_t)std::rand() * 2654435761u & high), jl = pl | ((uint32_t)std::rand() * 40503u & high);
                for (uint32_t i = a + 1; i + (d < 0 ? b : 0u) <= e - 1; ++i) {  // every split point
                    const double want = naive(w.data(), sh, sets, span, d, i);
                    const double x = bulge_table_score(w.data(), sh, g.gh, g.gl, g.single, ph, pl, d, i);
                    if (!same(x, want)) return 3;
                    if (!same(bulge_table_score(w.data(), sh, g.gh, g.gl, g.single, jh, jl, d, i), x)) return 4;
                    if (!(x >= 0.0 && x <= 1.0) || table_fixed(x) > kTableOne) return 5;
                    // the all-ones anchor: the pattern score of the paired site, the unpaired guide positions taken out
                    uint8_t q[32], qs[32];
                    std::memcpy(qs, sets, sizeof qs);
                    for (uint32_t j = 0; j < sh.len; ++j) {
                        if (d > 0) q[j] = j < i ? span[j] : span[j + b];
                        else if (j >= i && j < i + b) q[j] = 0, qs[j] = (uint8_t)kPatAny;
                        else q[j] = j < i ? span[j] : span[j - b];
                    }
                    uint32_t qh, ql, gh, gl, single;
                    site_planes(q, sh.len, &qh, &ql);
                    pattern_table_guide(qs, sh.len, &gh, &gl, &single);
                    if (!same(bulge_table_score(ones.data(), sh, g.gh, g.gl, g.single, ph, pl, d, i), pattern_table_score(w.data(), sh, gh, gl, single, qh, ql)))
                        return 6;
                    ++checked;
                }
                // outside the definition: 0.0
                const uint32_t outside_i[] = {0u, a, e - (d < 0 ? b : 0u), e, 31u, ~0u};
                for (uint32_t i : outside_i)
                    if (!(i >= a + 1 && i + (d < 0 ? b : 0u) <= e - 1) && bulge_table_score(w.data(), sh, g.gh, g.gl, g.single, ph, pl, d, i) != 0.0) return 7;
                // the member: the walk's (NM, i) and its score
                uint32_t nm, index, want_i = 0;
                const uint32_t f = bulge_table_member(w.data(), sh, g, ph, pl, d, &nm, &index);
                const uint32_t want_nm = naive_align(sh, sets, span, d, &want_i);
                if (nm != want_nm || index != want_i || f != table_fixed(naive(w.data(), sh, sets, span, d, want_i))) return 8;
            }
            for (int bad : {0, 3, -3, 100})
                if (bulge_table_score(w.data(), sh, g.gh, g.gl, g.single, 0, 0, bad, a + 1) != 0.0) return 9;
            // ---- the member loop of a site over one span, both anchors, against separately cut letters ----
            for (int at_start = 0; at_start < 2; ++at_start) {
                uint32_t members = kSiteNoMembers;
                int present[5], n_present = 0;
                for (int k = 0; k < 5; ++k)
                    if (std::rand() % 2) {
                        members = (members & ~(31u << (5 * k))) | 3u << (5 * k);  // (the field's NM is not read: it is recomputed)
                        present[n_present++] = k - 2;
                    }
                if (!n_present) continue;
                const int best_d = present[std::rand() % n_present];
                const uint32_t n = site_span_letters(sh.len, members);
                if (n != (uint32_t)((int)sh.len + present[n_present - 1])) return 10;
                unsigned long long hh = 0, ll = 0;
                for (uint32_t j = 0; j < n; ++j) {
                    hh |= (unsigned long long)(span[j] >> 1) << j;
                    ll |= (unsigned long long)(span[j] & 1u) << j;
                }
                SiteScores got;
                if (!site_table_scores(w.data(), sh, g, hh, ll, n, at_start != 0, members, best_d, &got)) return 11;
                uint32_t top = 0, top_d = 0, top_rank = 0, best = 0, best_nm = 0;
                for (int k = 0; k < n_present; ++k) {
                    const int d = present[k];
                    const uint32_t m = (uint32_t)((int)sh.len + d);
                    const uint8_t *s = at_start ? span : span + (n - m);
                    uint32_t ph, pl, nm, index;
                    site_planes(s, m, &ph, &pl);
                    const uint32_t f = bulge_table_member(w.data(), sh, g, ph, pl, d, &nm, &index);
                    if (d == 0) {
                        uint32_t want_nm = 0;
                        for (uint32_t j = 0; j < sh.len; ++j) want_nm += !((sets[j] >> s[j]) & 1u);
                        if (nm != want_nm || index != 0) return 12;
                    }
                    const uint32_t rank = site_rank(d, nm);
                    if (d == best_d) best = f, best_nm = nm;
                    if (k == 0 || f > top || (f == top && rank < top_rank)) top = f, top_d = (uint32_t)(d + 2), top_rank = rank;
                }
                if (got.best != best || got.top != top || got.top_d != top_d || got.best_nm != best_nm) return 13;
                // a best alignment that is not among the members, and no member at all
                for (int k = 0; k < 5; ++k)
                    if (((members >> (5 * k)) & 31u) == kSiteAbsent && site_table_scores(w.data(), sh, g, hh, ll, n, at_start != 0, members, k - 2, &got)) return 14;
                if (site_table_scores(w.data(), sh, g, 0, 0, 0, false, kSiteNoMembers, 0, &got) || got.top || got.best) return 15;
                ++checked;
            }
            // the reverse complement of a span
            const uint32_t n = sh.len + 2;
            unsigned long long hh = 0, ll = 0, rh = 0, rl = 0;
            for (uint32_t j = 0; j < n; ++j) {
                hh |= (unsigned long long)(span[j] >> 1) << j;
                ll |= (unsigned long long)(span[j] & 1u) << j;
                const uint8_t c = (uint8_t)(3 - span[n - 1 - j]);
                rh |= (unsigned long long)(c >> 1) << j;
                rl |= (unsigned long long)(c & 1u) << j;
            }
            if (span_revcomp(hh, n) != rh || span_revcomp(ll, n) != rl) return 16;
        }
        // what the definition refuses
        const double bad[] = {-0.5, 1.5, std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity()};
        for (double b : bad) {
            std::vector<double> v = w;
            v[bulge_table_dna_at(sh) + (size_t)std::rand() % (sh.ps_len * 8)] = b;
            if (bulge_table_valid(sh, v.data())) return 17;
        }
        std::vector<double> v = w;
        v[bulge_table_dna_at(sh)] = 2.0;  // row 0 of dna is never read and still validated
        if (bulge_table_valid(sh, v.data())) return 18;
        PatTableShape b2 = sh;
        b2.ps_len = 3;
        if (bulge_table_valid(b2, w.data())) return 19;
    }
    std::printf("ok: %llu cases\n", checked);
    return 0;
}
