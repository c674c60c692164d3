// pattern_table_check.cpp - the table score of pattern hits of varscot_amd/csrc/vsc_pattern_table.h (pattern_table_score,
// pattern_table_guide, pattern_table_valid) in a stand-alone program with its own main, for the host sanitizers.  No device is
// opened and no kernel is launched.  Build and run on the CPU:
//   hipcc --offload-arch=gfx950 -x hip -O1 -g -std=c++17 -ffp-contract=off -Iinclude -Ivarscot_amd/csrc -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tools/pattern_table_check.cpp -o build/pattern_table_check && build/pattern_table_check
// Random shapes (L 16..32, the protospacer anywhere, 0..4 PAM positions), random tables (weights of exactly 0 and 1 among
// them), random IUPAC guides and random sites: the planes' walk against a letter-by-letter product in the definition's order,
// bit for bit; the fixed-point word; garbage in the site's bits from L on and letters outside the protospacer, which must
// change nothing; the SpCas9 shape against table_score of vsc_table.h; the shapes and tables the definition refuses.  Exit
// code 0 and "ok" when all agree.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "vsc_pattern_table.h"

using namespace vsc;

static void site_planes(const uint8_t *c, uint32_t len, uint32_t *h, uint32_t *l)
{
    *h = *l = 0;
    for (uint32_t j = 0; j < len; ++j) {
        *h |= (uint32_t)(c[j] >> 1) << j;
        *l |= (uint32_t)(c[j] & 1u) << j;
    }
}

static bool same(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

int main()
{
    std::srand(31);
    unsigned long long checked = 0;
    for (int t = 0; t < 300; ++t) {
        PatTableShape sh{};
        sh.len = 16 + (uint32_t)(std::rand() % 17);
        sh.ps_len = 1 + (uint32_t)std::rand() % sh.len;
        sh.ps_start = (uint32_t)std::rand() % (sh.len - sh.ps_len + 1);
        if (t % 7 == 0) sh.ps_start = 0, sh.ps_len = sh.len;  // the whole site: no room for a PAM position
        std::vector<uint32_t> outside;
        for (uint32_t j = 0; j < sh.len; ++j)
            if (j < sh.ps_start || j >= sh.ps_start + sh.ps_len) outside.push_back(j);
        const uint32_t room = outside.size() < 4 ? (uint32_t)outside.size() : 4u;
        sh.n_pam = (uint32_t)std::rand() % (room + 1);
        // n_pam ascending positions out of `outside`
        for (uint32_t k = 0, from = 0; k < sh.n_pam; ++k) {
            const uint32_t left = sh.n_pam - k, span = (uint32_t)outside.size() - from - (left - 1);
            const uint32_t pick = from + (uint32_t)std::rand() % span;
            sh.pam_pos[k] = outside[pick];
            from = pick + 1;
        }
        if (!pattern_table_shape_valid(sh)) return 1;
        const uint32_t n_w = pattern_table_weights(sh), pairs = pattern_table_pairs(sh);
        std::vector<double> w(n_w);  // exactly as many doubles as the shape needs: a read past the end is the sanitizer's to find
        for (uint32_t i = 0; i < n_w; ++i) {
            const int r = std::rand() % 16;
            w[i] = r == 0 ? 0.0 : r == 1 ? 1.0 : (double)(std::rand() % 100000 + 1) / 100001.0;
        }
        for (uint32_t i = 0; i < sh.ps_len; ++i)
            for (uint32_t b = 0; b < 4; ++b) w[(i * 4 + b) * 4 + b] = 1.0;
        if (!pattern_table_valid(sh, w.data())) return 2;
        for (int trial = 0; trial < 400; ++trial) {
            uint8_t sets[32], s[32];
            for (uint32_t j = 0; j < sh.len; ++j) {
                sets[j] = std::rand() % 4 ? (uint8_t)(1u << (std::rand() % 4)) : (uint8_t)(1 + std::rand() % 15);  // any IUPAC set
                s[j] = (uint8_t)(std::rand() % 4);
                if (std::rand() % 3 && (sets[j] & (sets[j] - 1)) == 0) s[j] = (uint8_t)__builtin_ctz(sets[j]);  // mostly the guide's base
            }
            double want = 1.0;
            for (uint32_t i = 0; i < sh.ps_len; ++i) {
                const uint32_t j = sh.ps_start + i, set = sets[j];
                if ((set & (set - 1)) != 0) continue;  // a degenerate letter takes no part
                const uint32_t g = (uint32_t)__builtin_ctz(set);
                if (g != s[j]) want = want * w[(i * 4 + g) * 4 + s[j]];
            }
            uint32_t k = 0;
            for (uint32_t q = 0; q < sh.n_pam; ++q) k = 4 * k + s[sh.pam_pos[q]];
            want = want * w[pairs + k];
            uint32_t gh, gl, single, ph, pl;
            pattern_table_guide(sets, sh.len, &gh, &gl, &single);
            site_planes(s, sh.len, &ph, &pl);
            const double x = pattern_table_score(w.data(), sh, gh, gl, single, ph, pl);
            if (!same(x, want)) return 3;
            if (!(x >= 0.0 && x <= 1.0) || table_fixed(x) > kTableOne || table_fixed(x) != (uint32_t)std::nearbyint(x * 1073741824.0)) return 4;
            // the kernels' site words hold the genome's next bases from bit L on: they must not count
            const uint32_t high = sh.len < 32 ? ~0u << sh.len : 0u;
            const double y = pattern_table_score(w.data(), sh, gh, gl, single, ph | ((uint32_t)std::rand() * 2654435761u & high),
                                                 pl | ((uint32_t)std::rand() * 40503u & high));
            if (!same(y, x)) return 5;
            // a guide letter outside the protospacer takes no part
            if (!outside.empty()) {
                uint8_t other[32];
                std::memcpy(other, sets, sizeof other);
                other[outside[(size_t)std::rand() % outside.size()]] = (uint8_t)(1u << (std::rand() % 4));
                uint32_t oh, ol, os;
                pattern_table_guide(other, sh.len, &oh, &ol, &os);
                if (!same(pattern_table_score(w.data(), sh, oh, ol, os, ph, pl), x)) return 6;
            }
            ++checked;
        }
        // what the definition refuses
        const double bad[] = {-0.5, 1.5, std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity()};
        for (double b : bad) {
            std::vector<double> v = w;
            v[(size_t)std::rand() % n_w] = b;
            if (pattern_table_valid(sh, v.data())) return 7;
        }
        std::vector<double> v = w;
        v[(((uint32_t)std::rand() % sh.ps_len) * 4 + 2) * 4 + 2] = 0.5;  // a diagonal entry other than 1
        if (pattern_table_valid(sh, v.data())) return 8;
        PatTableShape b2 = sh;
        b2.len = 15;
        if (pattern_table_shape_valid(b2)) return 9;
        b2 = sh;
        b2.ps_len = 0;
        if (pattern_table_shape_valid(b2)) return 10;
        b2 = sh;
        b2.ps_start = sh.len - sh.ps_len + 1;
        if (pattern_table_shape_valid(b2)) return 11;
        if (sh.n_pam) {
            b2 = sh;
            b2.pam_pos[sh.n_pam - 1] = sh.ps_start;  // inside the protospacer
            if (pattern_table_shape_valid(b2)) return 12;
            b2 = sh;
            b2.pam_pos[0] = sh.len;  // outside the site
            if (pattern_table_shape_valid(b2)) return 13;
        }
        if (sh.n_pam >= 2) {
            b2 = sh;
            b2.pam_pos[1] = b2.pam_pos[0];  // not strictly ascending
            if (pattern_table_shape_valid(b2)) return 14;
        }
        b2 = sh;
        b2.n_pam = 5;
        if (pattern_table_shape_valid(b2)) return 15;
    }
    // the anchor: the SpCas9 shape over a vsc_score_table's weights is table_score, bit for bit
    PatTableShape sp{23, 0, 20, 2, {21, 22, 0, 0}};
    if (pattern_table_weights(sp) != kTableWeights || pattern_table_pairs(sp) != kTablePairs) return 16;
    for (int t = 0; t < 50; ++t) {
        std::vector<double> w(kTableWeights);
        for (uint32_t i = 0; i < kTableWeights; ++i) w[i] = std::rand() % 9 ? (double)(std::rand() % 100000 + 1) / 100001.0 : 0.0;
        for (uint32_t j = 0; j < 20; ++j)
            for (uint32_t b = 0; b < 4; ++b) w[(j * 4 + b) * 4 + b] = 1.0;
        if (!table_valid(w.data()) || !pattern_table_valid(sp, w.data())) return 17;
        for (int trial = 0; trial < 400; ++trial) {
            uint8_t sets[23], g[23], s[23];
            for (int j = 0; j < 23; ++j) {
                g[j] = (uint8_t)(std::rand() % 4);
                sets[j] = (uint8_t)(1u << g[j]);
                s[j] = std::rand() % 3 ? g[j] : (uint8_t)(std::rand() % 4);
            }
            uint32_t gh, gl, single, rh, rl, ph, pl;
            pattern_table_guide(sets, 23, &gh, &gl, &single);
            site_planes(g, 23, &rh, &rl);
            site_planes(s, 23, &ph, &pl);
            if (gh != rh || gl != rl || single != 0x7FFFFFu) return 18;
            if (!same(pattern_table_score(w.data(), sp, gh, gl, single, ph, pl), table_score(w.data(), rh, rl, ph, pl))) return 19;
            ++checked;
        }
    }
    std::printf("ok: %llu cases\n", checked);
    return 0;
}
