// pattern_enum_check.cpp - the header-only host helpers of pattern guide discovery (varscot_amd/csrc/vsc_pattern_enum.h: the
// target intervals as ranges of site starts, the letters of a code) in a stand-alone program with its own main, for the host
// sanitizers.  No device is opened and no kernel is launched.  Build and run on the CPU:
//   hipcc --offload-arch=gfx950 -x hip -O1 -g -std=c++17 -Iinclude -Ivarscot_amd/csrc -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tools/pattern_enum_check.cpp -o build/pattern_enum_check && build/pattern_enum_check
// Random contig tables and interval sets (nested, abutting, overlapping, shorter than the site, cut by either end of the
// contig, empty), both rules, every site length 16..32: the ranges against the rule applied to every position one by one, and
// that they are sorted, disjoint and not abutting.  Every length, random codes and protospacers: the text against a
// letter-by-letter expansion.  What the call refuses.  Exit code 0 and "ok" when all agree.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "vsc_pattern_enum.h"

using namespace vsc;

namespace {

bool site_in(const std::vector<vsc_interval> &iv, const std::vector<uint32_t> &lens, uint32_t c, uint32_t p, uint32_t L, uint32_t rule)
{
    for (const vsc_interval &v : iv) {
        const uint32_t end = v.end < lens[v.contig] ? v.end : lens[v.contig];
        if (v.contig != c || v.start >= end) continue;
        if (rule == VSC_REGION_OVERLAP ? (p < end && (uint64_t)p + L > v.start) : (v.start <= p && (uint64_t)p + L <= end)) return true;
    }
    return false;
}

}  // namespace

int main()
{
    std::srand(29);
    unsigned long long checked = 0;
    for (uint32_t L = kPatMinLen; L <= kPatMaxLen; ++L) {
        for (int trial = 0; trial < 60; ++trial) {
            const uint32_t n_contigs = 1 + (uint32_t)(std::rand() % 3);
            std::vector<uint32_t> lens(n_contigs), off(n_contigs), end(n_contigs);  // exactly n_contigs entries each
            uint32_t at = 0;
            for (uint32_t c = 0; c < n_contigs; ++c) {
                lens[c] = (uint32_t)(std::rand() % 3 ? 40 + std::rand() % 400 : std::rand() % 40);
                off[c] = at;
                end[c] = at + lens[c];
                at += lens[c] + 1;  // the separator
            }
            const uint32_t n = (uint32_t)(std::rand() % 12);
            std::vector<vsc_interval> iv(n);
            for (uint32_t i = 0; i < n; ++i) {
                const uint32_t c = (uint32_t)std::rand() % n_contigs;
                const uint32_t a = (uint32_t)std::rand() % (lens[c] + 20), span = (uint32_t)(std::rand() % 4 ? std::rand() % 90 : 0);
                iv[i] = vsc_interval{c, a, a + span, 0u};
                if (i && std::rand() % 4 == 0) iv[i] = vsc_interval{iv[i - 1].contig, iv[i - 1].end, iv[i - 1].end + span, 0u};  // abutting
            }
            for (uint32_t rule : {(uint32_t)VSC_REGION_OVERLAP, (uint32_t)VSC_REGION_INSIDE}) {
                std::vector<PatStartRange> r;
                if (pattern_target_ranges(off.data(), end.data(), n_contigs, iv.data(), n, rule, L, &r) != VSC_OK) return 1;
                for (size_t k = 0; k < r.size(); ++k) {
                    if (r[k].lo >= r[k].hi) return 2;
                    if (k && r[k].lo <= r[k - 1].hi) return 3;  // sorted, disjoint, not abutting
                }
                for (uint32_t c = 0; c < n_contigs; ++c)
                    for (uint32_t p = 0; p <= lens[c]; ++p) {  // (p == lens[c]: the separator, in no range)
                        const bool want = p < lens[c] && site_in(iv, lens, c, p, L, rule);
                        if (pattern_ranges_contain(r, off[c] + p) != want) return 4;
                        ++checked;
                    }
            }
        }
        for (int trial = 0; trial < 400; ++trial) {
            const uint32_t mask = L < 32 ? (1u << L) - 1u : ~0u;
            const uint32_t hi = ((uint32_t)std::rand() << 16 ^ (uint32_t)std::rand()) & mask, lo = ((uint32_t)std::rand() << 16 ^ (uint32_t)std::rand()) & mask;
            const uint32_t k = 1 + (uint32_t)std::rand() % L, a = (uint32_t)std::rand() % (L - k + 1);
            for (uint32_t spell = 0; spell < 2; ++spell) {
                std::vector<char> out(L);  // exactly L bytes: a write past the end is the sanitizer's to find
                if (pattern_guide_text((uint64_t)hi << 32 | lo, L, a, k, spell, out.data()) != VSC_OK) return 5;
                for (uint32_t j = 0; j < L; ++j) {
                    const char letter = "ACGT"[((hi >> j) & 1u) * 2 + ((lo >> j) & 1u)];
                    if (out[j] != ((j >= a && j < a + k) || spell ? letter : 'N')) return 6;
                }
                ++checked;
            }
        }
    }
    // refusals
    char buf[32];
    std::vector<PatStartRange> r;
    const uint32_t off1[1] = {0}, end1[1] = {100};
    const vsc_interval bad_contig{1, 0, 10, 0}, bad_order{0, 11, 10, 0}, bad_reserved{0, 0, 10, 1}, fine{0, 0, 10, 0};
    if (pattern_target_ranges(off1, end1, 1, &bad_contig, 1, VSC_REGION_OVERLAP, 20, &r) != VSC_ERR_INVALID) return 7;
    if (pattern_target_ranges(off1, end1, 1, &bad_order, 1, VSC_REGION_OVERLAP, 20, &r) != VSC_ERR_INVALID) return 8;
    if (pattern_target_ranges(off1, end1, 1, &bad_reserved, 1, VSC_REGION_INSIDE, 20, &r) != VSC_ERR_INVALID) return 9;
    if (pattern_target_ranges(off1, end1, 1, &fine, 1, 2, 20, &r) != VSC_ERR_INVALID) return 10;
    if (pattern_target_ranges(off1, end1, 1, nullptr, 0, VSC_REGION_INSIDE, 20, &r) != VSC_OK || !r.empty()) return 11;
    if (pattern_guide_text(0, 15, 0, 15, 0, buf) != VSC_ERR_INVALID || pattern_guide_text(0, 33, 0, 20, 0, buf) != VSC_ERR_INVALID) return 12;
    if (pattern_guide_text(0, 20, 0, 0, 0, buf) != VSC_ERR_INVALID || pattern_guide_text(0, 20, 1, 20, 0, buf) != VSC_ERR_INVALID) return 13;
    if (pattern_guide_text(0, 20, 0, 20, 2, buf) != VSC_ERR_INVALID || pattern_guide_text(0, 20, 0, 20, 0, nullptr) != VSC_ERR_INVALID) return 14;
    if (pattern_guide_text(1ull << 20, 20, 0, 20, 0, buf) != VSC_ERR_INVALID || pattern_guide_text(1ull << 52, 20, 0, 20, 0, buf) != VSC_ERR_INVALID) return 15;
    if (pattern_guide_text(~0ull, 32, 0, 32, 1, buf) != VSC_OK || std::string(buf, 32) != std::string(32, 'T')) return 16;
    std::printf("ok: %llu cases\n", checked);
    return 0;
}
