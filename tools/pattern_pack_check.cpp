// pattern_pack_check.cpp - the host packing of the pattern search (varscot_amd/csrc/vsc_pattern.h: letters to sets, sets to
// planes, reverse complements, the front end's table, the compare) in a stand-alone program with its own main, for the host
// sanitizers.  No device is opened and no kernel is launched.  Build and run on the CPU:
//   hipcc --offload-arch=gfx950 -x hip -O1 -g -std=c++17 -Iinclude -Ivarscot_amd/csrc -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tools/pattern_pack_check.cpp -o build/pattern_pack_check && build/pattern_pack_check
// Every length 16..32, random IUPAC patterns and guides, random sites: the planes' compare against a letter-by-letter one,
// the reverse complement twice, and the table against the sets.  Exit code 0 and "ok" when all agree.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "vsc_pattern.h"

using namespace vsc;

int main()
{
    const char letters[] = "ACGTRYSWKMBDHVNacgtryswkmbdhvn";
    unsigned long long checked = 0;
    std::srand(17);
    for (uint32_t len = kPatMinLen; len <= kPatMaxLen; ++len) {
        for (int trial = 0; trial < 2000; ++trial) {
            std::vector<char> text(len), site(len);  // exactly len bytes: a read past the end is the sanitizer's to find
            for (uint32_t j = 0; j < len; ++j) {
                text[j] = letters[std::rand() % 30];
                site[j] = "ACGT"[std::rand() % 4];
            }
            std::vector<uint8_t> sets(len), back(len), twice(len);
            if (!pattern_sets(text.data(), len, sets.data())) return 1;
            pattern_revcomp(sets.data(), len, back.data());
            pattern_revcomp(back.data(), len, twice.data());
            if (twice != sets) return 2;
            const PatPlanes fwd = pattern_planes(sets.data(), len), rev = pattern_planes(back.data(), len);
            uint32_t h = 0, l = 0, rh = 0, rl = 0, want = 0;
            for (uint32_t j = 0; j < len; ++j) {
                const uint32_t c = (uint32_t)(site[j] == 'C') | (uint32_t)(site[j] == 'G') << 1 | (site[j] == 'T' ? 3u : 0u);
                h |= (c >> 1) << j;
                l |= (c & 1u) << j;
                rh |= ((3u - c) >> 1) << (len - 1u - j);
                rl |= ((3u - c) & 1u) << (len - 1u - j);
                if (!((sets[j] >> c) & 1u)) want |= 1u << j;
            }
            const uint32_t x = pattern_mismatch(h, l, fwd), y = pattern_mismatch(rh, rl, rev);
            if (x != want) return 3;
            uint32_t mirrored = 0;
            for (uint32_t j = 0; j < len; ++j) mirrored |= ((x >> j) & 1u) << (len - 1u - j);
            if (y != mirrored) return 4;
            PatFront f;
            pattern_front(sets.data(), len, &f);
            uint32_t constrained = 0;
            for (uint32_t j = 0; j < len; ++j) constrained += sets[j] != kPatAny;
            if (f.n != constrained) return 5;
            for (uint32_t i = 0; i < f.n; ++i)
                if ((f.ent[i] >> 8) != sets[f.ent[i] & 31u]) return 6;
            ++checked;
        }
    }
    uint8_t one[1];
    if (pattern_sets("U", 1, one) || pattern_sets("x", 1, one) || iupac_comp(iupac_set('R')) != iupac_set('Y')) return 7;
    std::printf("ok: %llu cases\n", checked);
    return 0;
}
