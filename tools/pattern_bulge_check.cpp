// pattern_bulge_check.cpp - the header-only functions of bulges under a pattern (varscot_amd/csrc/vsc_pattern_bulge.h: the two
// pairings, the bound, the walk over the split points, the bulged pattern, the refusals) in a stand-alone program with its own
// main, for the host sanitizers.  No device is opened and no kernel is launched.  Build and run on the CPU:
//   g++ -O1 -g -std=c++17 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude -Ivarscot_amd/csrc -fsanitize=address,undefined \
//       -fno-sanitize-recover=undefined tools/pattern_bulge_check.cpp -o build/pattern_bulge_check && build/pattern_bulge_check
// (or hipcc --offload-arch=gfx950 -x hip with -Xarch_host in front of the two sanitizer options, as pattern_pack_check.cpp).
// Every length 16..32, every protospacer (a, n) of a set that holds a = 0, e = L and a PAM at both ends, every d the length
// takes, random IUPAC guides, random sites and sites planted at every split point: NM and the index against a naive loop over
// the letters, the bound against every nm(i), the bulged pattern letter by letter.  Exit code 0 and "ok" when all agree.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "vsc_pattern_bulge.h"

using namespace vsc;

namespace {

bool in_set(uint8_t set, char base) { return (set >> (base == 'A' ? 0 : base == 'C' ? 1 : base == 'G' ? 2 : 3)) & 1u; }

// nm(i) of the definition, letter by letter
uint32_t naive_nm(const std::vector<uint8_t> &g, const std::vector<char> &s, uint32_t len, int d, uint32_t i)
{
    uint32_t nm = 0;
    for (uint32_t j = 0; j < i; ++j) nm += !in_set(g[j], s[j]);
    if (d > 0) {
        for (uint32_t j = i; j < len; ++j) nm += !in_set(g[j], s[j + (uint32_t)d]);
    } else {
        const uint32_t b = (uint32_t)-d;
        for (uint32_t j = i + b; j < len; ++j) nm += !in_set(g[j], s[j - b]);
    }
    return nm;
}

}  // namespace

int main()
{
    const char letters[] = "ACGTRYSWKMBDHVNacgtryswkmbdhvn";
    unsigned long long checked = 0;
    std::srand(19);
    for (uint32_t len = kPatMinLen; len <= kPatMaxLen; ++len) {
        const uint32_t protos[][2] = {{0, len}, {0, len - 3}, {4, len - 4}, {3, len - 6}, {2, 4}, {len - 4, 4}, {5, 9}};
        for (const auto &pr : protos) {
            const uint32_t a = pr[0], n = pr[1], e = a + n;
            for (int d = -2; d <= 2; ++d) {
                if (d == 0) continue;
                std::vector<uint8_t> p_sets(len), bulged(len + 2);
                for (uint32_t j = 0; j < len; ++j) p_sets[j] = (uint8_t)(a <= j && j < e ? kPatAny : iupac_set(letters[std::rand() % 30]));
                const uint32_t dna = d > 0 ? (uint32_t)d : 0u, rna = d < 0 ? (uint32_t)-d : 0u;
                const bool fits = len + dna <= kPatMaxLen && len >= kPatMinLen + rna;
                if ((pattern_bulge_refusal(p_sets.data(), len, a, n, dna, rna) == nullptr) != fits) return 1;
                if (!fits) continue;
                const uint32_t site_len = (uint32_t)((int)len + d), gap = rna;
                pattern_bulged(p_sets.data(), len, a, e, d, bulged.data());
                for (uint32_t j = 0; j < site_len; ++j) {
                    const uint8_t want = j < a ? p_sets[j] : (j < (uint32_t)((int)e + d) ? (uint8_t)kPatAny : p_sets[(uint32_t)((int)j - d)]);
                    if (bulged[j] != want) return 2;
                }
                const uint32_t first = a + 1u, last = e - 1u - gap;
                for (int trial = 0; trial < 40; ++trial) {
                    std::vector<char> text(len);
                    std::vector<uint8_t> g(len);
                    for (uint32_t j = 0; j < len; ++j) text[j] = trial % 4 == 0 ? "ACGT"[std::rand() % 4] : letters[std::rand() % 30];
                    if (!pattern_sets(text.data(), len, g.data())) return 3;
                    const PatPlanes planes = pattern_planes(g.data(), len);
                    for (uint32_t at = first - 1u; at <= last; ++at) {  // at = first - 1: a random site; else planted at split point `at`
                        std::vector<char> s(site_len);  // exactly L + d bytes: a read past the end is the sanitizer's to find
                        for (uint32_t j = 0; j < site_len; ++j) s[j] = "ACGT"[std::rand() % 4];
                        if (at >= first) {
                            // every paired position takes a base of the guide's set (its lowest), then up to three are changed
                            for (uint32_t j = 0; j < len; ++j) {
                                const char base = "ACGT"[__builtin_ctz(g[j])];
                                if (j < at) s[j] = base;
                                else if (d > 0) s[j + (uint32_t)d] = base;
                                else if (j >= at + gap) s[j - gap] = base;
                            }
                            for (int k = std::rand() % 4; k > 0; --k) s[(uint32_t)std::rand() % site_len] = "ACGT"[std::rand() % 4];
                        }
                        uint32_t sh = 0, sl = 0;
                        for (uint32_t j = 0; j < site_len; ++j) {
                            const uint32_t c = (uint32_t)(s[j] == 'C') | (uint32_t)(s[j] == 'G') << 1 | (s[j] == 'T' ? 3u : 0u);
                            sh |= (c >> 1) << j;
                            sl |= (c & 1u) << j;
                        }
                        uint32_t best = ~0u, where = 0, low = ~0u;
                        for (uint32_t i = first; i <= last; ++i) {
                            const uint32_t nm = naive_nm(g, s, len, d, i);
                            if (nm < best) best = nm, where = i;
                            if (nm < low) low = nm;
                        }
                        uint32_t index = 0, x0, x1;
                        if (pattern_bulge_align(sh, sl, planes, a, e, d, &index) != best || index != where) return 4;
                        pattern_bulge_masks(sh, sl, planes, d, &x0, &x1);
                        const uint32_t bound = (uint32_t)__builtin_popcount(
                            pattern_bulge_bound_mask(x0, x1, pattern_bulge_fixed5(a), pattern_bulge_fixed3(e, len)));
                        if (bound > low + gap) return 5;  // the bound never rejects a pair that the walk would accept
                        if ((x0 | x1) & ~low_bits(len)) return 6;
                        ++checked;
                    }
                }
            }
        }
    }
    std::printf("ok: %llu cases\n", checked);
    return 0;
}
