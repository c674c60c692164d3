// table_score_check.cpp - the table-driven score of varscot_amd/csrc/vsc_table.h (table_score, table_fixed, table_valid) in a
// stand-alone program with its own main, for the host sanitizers.  No device is opened and no kernel is launched.  Build and
// run on the CPU:
//   hipcc --offload-arch=gfx950 -x hip -O1 -g -std=c++17 -ffp-contract=off -Iinclude -Ivarscot_amd/csrc -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tools/table_score_check.cpp -o build/table_score_check && build/table_score_check
// Random tables (weights of exactly 0 and 1 among them) and random (read, site) pairs: the planes' walk against a letter-by-
// letter product in the definition's order, bit for bit; the fixed-point word; mismatches at read positions 20..22, which must
// change nothing; the tables the definition refuses.  Exit code 0 and "ok" when all agree.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "vsc_table.h"

using namespace vsc;

static void planes(const uint8_t *c, uint32_t *h, uint32_t *l)
{
    *h = *l = 0;
    for (int j = 0; j < 23; ++j) {
        *h |= (uint32_t)(c[j] >> 1) << j;
        *l |= (uint32_t)(c[j] & 1u) << j;
    }
}

int main()
{
    std::srand(29);
    unsigned long long checked = 0;
    for (int t = 0; t < 200; ++t) {
        std::vector<double> w(kTableWeights);  // exactly 336 doubles: a read past the end is the sanitizer's to find
        for (uint32_t i = 0; i < kTableWeights; ++i) {
            const int r = std::rand() % 16;
            w[i] = r == 0 ? 0.0 : r == 1 ? 1.0 : (double)(std::rand() % 100000 + 1) / 100001.0;
        }
        for (uint32_t j = 0; j < 20; ++j)
            for (uint32_t b = 0; b < 4; ++b) w[(j * 4 + b) * 4 + b] = 1.0;
        if (!table_valid(w.data())) return 1;
        for (int trial = 0; trial < 500; ++trial) {
            uint8_t g[23], s[23];
            for (int j = 0; j < 23; ++j) {
                g[j] = (uint8_t)(std::rand() % 4);
                s[j] = std::rand() % 3 ? g[j] : (uint8_t)(std::rand() % 4);
            }
            double want = 1.0;
            for (int j = 0; j < 20; ++j)
                if (g[j] != s[j]) want = want * w[(j * 4 + g[j]) * 4 + s[j]];
            want = want * w[kTablePairs + 4 * s[21] + s[22]];
            uint32_t gh, gl, sh, sl;
            planes(g, &gh, &gl);
            planes(s, &sh, &sl);
            const double x = table_score(w.data(), gh, gl, sh, sl);
            if (std::memcmp(&x, &want, sizeof x) != 0) return 2;
            if (!(x >= 0.0 && x <= 1.0) || table_fixed(x) > kTableOne || table_fixed(x) != (uint32_t)std::nearbyint(x * 1073741824.0)) return 3;
            for (int j = 20; j < 23; ++j) {  // the read's letters 20..22 take no part
                uint8_t g2[23];
                std::memcpy(g2, g, sizeof g2);
                g2[j] = (uint8_t)((g[j] + 1 + std::rand() % 3) % 4);
                planes(g2, &gh, &gl);
                const double y = table_score(w.data(), gh, gl, sh, sl);
                if (std::memcmp(&y, &x, sizeof y) != 0) return 4;
            }
            ++checked;
        }
        // what the definition refuses
        const double bad[] = {-0.5, 1.5, std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity()};
        for (double b : bad) {
            std::vector<double> v = w;
            v[std::rand() % kTableWeights] = b;
            if (table_valid(v.data())) return 5;
        }
        std::vector<double> v = w;
        v[((std::rand() % 20) * 4 + 2) * 4 + 2] = 0.5;  // a diagonal entry other than 1
        if (table_valid(v.data())) return 6;
    }
    if (table_fixed(1.0) != kTableOne || table_fixed(0.0) != 0 || table_fixed(0.5 / 1073741824.0) != 0 || table_fixed(1.5 / 1073741824.0) != 2)
        return 7;  // round half to even
    std::printf("ok: %llu cases\n", checked);
    return 0;
}
