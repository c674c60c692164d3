// pick_check.cpp - the per-target pick of varscot_amd/csrc/vsc_pick.h (pick_shape_valid, pick_cut_coordinate, pick_class,
// pick_before, pick_conflict and pick_host, the body of vsc_pick_host) in a stand-alone program with its own main, for the host
// sanitizers.  No device is opened and no kernel is launched.  Build and run on the CPU:
//   hipcc --offload-arch=gfx950 -x hip -O1 -g -std=c++17 -Iinclude -Ivarscot_amd/csrc -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tools/pick_check.cpp -o build/pick_check && build/pick_check
//   - pick_host on heap arrays of exactly the held sizes (n loci, n targets, n keys, n_targets * k picks, n_targets counts, n
//     ranks) over the shapes of the tests' fixtures - K 1, 4, 32, spacing 0, 1, 20, 1000, 3-bit keys, keys that differ at the
//     top and bottom bits only, crowded and sparse positions, loci that are invalid, without a target or with a bad one - and
//     over random shapes (site_len 16 .. 32, every cut), against the PICK loop of the definition run round by round: in every
//     round a scan of all candidates of the target for the first under BEFORE that is not picked and conflicts with no pick;
//   - the small functions at their edges: coordinates next to 2^32, spacing 0 and 0xFFFFFFFF, the order's ties.
// Exit code 0 and "ok" when all agree.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "vsc_pick.h"

using namespace vsc;

static uint64_t rnd64() { return (uint64_t)std::rand() << 42 ^ (uint64_t)std::rand() << 21 ^ (uint64_t)std::rand(); }

static long g_cases = 0, g_picks = 0;

// the PICK loop as the definition words it; returns false on the first difference from pick_host
static bool check(const PickShape &s, const std::vector<uint32_t> &lens, uint64_t n, uint32_t n_targets, int key_kind, int crowd)
{
    // exactly the held sizes: the sanitizer sees one element too far
    std::unique_ptr<PickLocus[]> loci(new PickLocus[n]);
    std::unique_ptr<uint32_t[]> target(new uint32_t[n]), picks(new uint32_t[(size_t)n_targets * s.k]), counts(new uint32_t[n_targets]), rank(new uint32_t[n]);
    std::unique_ptr<uint64_t[]> key(new uint64_t[n]);
    for (uint64_t i = 0; i < n; ++i) {
        const uint32_t c = (uint32_t)(std::rand() % lens.size());
        const uint32_t room = lens[c] >= s.site_len ? lens[c] - s.site_len + 1 : 1;
        loci[i] = PickLocus{c, (uint32_t)(std::rand() % (crowd ? (room < 60 ? room : 60) : room)), (uint32_t)(std::rand() & 1), 0};
        target[i] = (uint32_t)(std::rand() % n_targets);
        switch (std::rand() % 16) {  // the loci and targets the definition sets aside
        case 0: loci[i].contig = (uint32_t)lens.size() + (uint32_t)(std::rand() % 3) * 0x7FFFFFFFu; break;
        case 1: loci[i].strand = 2u + (uint32_t)(std::rand() % 3); break;
        case 2: loci[i].pos = lens[c] - (uint32_t)(std::rand() % s.site_len); break;
        case 3: loci[i].pos = 0xFFFFFFFFu - (uint32_t)(std::rand() % 40); break;
        case 4: target[i] = kPickNone; break;
        case 5: target[i] = n_targets + (uint32_t)(std::rand() % 2) * 0x7FFFFFF0u; break;
        default: break;
        }
        key[i] = key_kind == 0 ? (uint64_t)(std::rand() & 7) : key_kind == 1 ? 1ull << 63 | (rnd64() & 0xFFFFF) : key_kind == 2 ? (rnd64() & 3) << 62 | (rnd64() & 3) : rnd64();
    }
    uint64_t stats[kPickStats] = {};
    pick_host(s, lens.data(), (uint32_t)lens.size(), loci.get(), n, target.get(), key.get(), n_targets, picks.get(), counts.get(), rank.get(), stats);
    uint64_t want_stats[kPickStats] = {};
    std::vector<uint32_t> cls(n);
    for (uint64_t i = 0; i < n; ++i) {
        const uint32_t c = loci[i].contig;
        cls[i] = pick_class(s, (uint32_t)lens.size(), c, c < lens.size() ? lens[c] : 0u, loci[i].pos, loci[i].strand, target[i], n_targets, key[i]);
        ++want_stats[cls[i]];
    }
    std::vector<uint32_t> want_rank(n, kPickNone);
    for (uint32_t t = 0; t < n_targets; ++t) {
        std::vector<uint32_t> picked;
        uint64_t members = 0;
        for (uint64_t i = 0; i < n; ++i) members += cls[i] == kPickEligible && target[i] == t;
        while (picked.size() < s.k) {
            uint32_t best = kPickNone;
            for (uint64_t i = 0; i < n; ++i) {
                if (cls[i] != kPickEligible || target[i] != t || want_rank[i] != kPickNone) continue;
                bool open = true;
                for (uint32_t j : picked)
                    open = open && !pick_conflict(s.spacing, loci[i].contig, pick_cut_coordinate(s, loci[i].pos, loci[i].strand), loci[j].contig,
                                                  pick_cut_coordinate(s, loci[j].pos, loci[j].strand));
                if (open && (best == kPickNone || pick_before(key[i], (uint32_t)i, key[best], best))) best = (uint32_t)i;
            }
            if (best == kPickNone) break;
            want_rank[best] = (uint32_t)picked.size();
            picked.push_back(best);
        }
        for (uint32_t r = 0; r < s.k; ++r)
            if (picks[(size_t)t * s.k + r] != (r < picked.size() ? picked[r] : kPickNone)) return false;
        if (counts[t] != picked.size()) return false;
        want_stats[kPickStatTargets] += !picked.empty();
        want_stats[kPickStatShort] += picked.size() < s.k && members > picked.size();
        want_stats[kPickStatPicks] += picked.size();
        g_picks += (long)picked.size();
    }
    for (uint64_t i = 0; i < n; ++i)
        if (rank[i] != want_rank[i]) return false;
    for (int j = 0; j < kPickStats; ++j)
        if (stats[j] != want_stats[j]) return false;
    ++g_cases;
    return true;
}

#define REQUIRE(x)                                                     \
    do {                                                               \
        if (!(x)) {                                                    \
            std::printf("FAILED at line %d: %s\n", __LINE__, #x);      \
            return 1;                                                  \
        }                                                              \
    } while (0)

int main()
{
    std::srand(12345);
    // the small functions at their edges
    REQUIRE(pick_shape_valid(PickShape{23, 17, 4, 20, 0}) && pick_shape_valid(PickShape{16, 0, 1, 0, ~0ull}) && pick_shape_valid(PickShape{32, 32, 32, ~0u, 0}));
    REQUIRE(!pick_shape_valid(PickShape{15, 0, 1, 0, 0}) && !pick_shape_valid(PickShape{33, 0, 1, 0, 0}) && !pick_shape_valid(PickShape{23, 24, 1, 0, 0}));
    REQUIRE(!pick_shape_valid(PickShape{23, 17, 0, 0, 0}) && !pick_shape_valid(PickShape{23, 17, 33, 0, 0}));
    const PickShape sp{23, 17, 4, 20, 0};
    REQUIRE(pick_cut_coordinate(sp, 40, 0) == 57 && pick_cut_coordinate(sp, 51, 1) == 57);
    REQUIRE(pick_cut_coordinate(PickShape{32, 32, 1, 0, 0}, 0xFFFFFFFFu, 0) == 0x100000000ull + 31);  // 64-bit: no wrap
    REQUIRE(!pick_conflict(0, 0, 5, 0, 5) && pick_conflict(1, 0, 5, 0, 5) && !pick_conflict(1, 0, 5, 0, 6) && !pick_conflict(1000, 0, 5, 1, 5));
    REQUIRE(pick_conflict(0xFFFFFFFFu, 0, 0, 0, 0xFFFFFFFEull) && !pick_conflict(0xFFFFFFFFu, 0, 0, 0, 0xFFFFFFFFull));
    REQUIRE(pick_conflict(20, 3, 100, 3, 81) && pick_conflict(20, 3, 81, 3, 100) && !pick_conflict(20, 3, 100, 3, 80));
    REQUIRE(pick_before(2, 9, 1, 0) && !pick_before(1, 0, 2, 9) && pick_before(5, 3, 5, 4) && !pick_before(5, 4, 5, 3) && !pick_before(5, 3, 5, 3));
    REQUIRE(pick_before(~0ull, 7, 1ull << 63, 0));
    REQUIRE(pick_class(sp, 2, 2, 0, 0, 0, 0, 1, 0) == kPickInvalid && pick_class(sp, 2, 0, 100, 0, 2, 0, 1, 0) == kPickInvalid);
    REQUIRE(pick_class(sp, 2, 0, 100, 77, 0, 0, 1, 0) == kPickEligible && pick_class(sp, 2, 0, 100, 78, 0, 0, 1, 0) == kPickInvalid);
    REQUIRE(pick_class(sp, 2, 0, 100, 0xFFFFFFF0u, 0, 0, 1, 0) == kPickInvalid && pick_class(sp, 2, 0, 10, 0, 0, 0, 1, 0) == kPickInvalid);
    REQUIRE(pick_class(sp, 2, 0, 100, 0, 0, kPickNone, 1, 0) == kPickNoTarget && pick_class(sp, 2, 0, 100, 0, 0, 1, 1, 0) == kPickBadTarget);
    REQUIRE(pick_class(PickShape{23, 17, 4, 20, 9}, 2, 0, 100, 0, 0, 0, 1, 8) == kPickBelowMinKey);
    REQUIRE(pick_class(PickShape{23, 17, 4, 20, 9}, 2, 0, 100, 0, 0, 0, 1, 9) == kPickEligible);
    REQUIRE(pick_class(PickShape{23, 17, 4, 20, 9}, 2, 0, 100, 0, 0, kPickNone, 1, 8) == kPickNoTarget);  // the order of the classes

    // the fixtures' shapes
    const std::vector<uint32_t> lens = {6000, 900, 60, 23};
    const uint32_t ks[] = {1, 4, 32}, spacings[] = {0, 1, 20, 1000};
    for (uint32_t k : ks)
        for (uint32_t spacing : spacings)
            for (int key_kind = 0; key_kind < 3; ++key_kind)
                for (int crowd = 0; crowd < 2; ++crowd)
                    REQUIRE(check(PickShape{23, 17, k, spacing, (uint64_t)(key_kind == 0 ? crowd * 3 : 0)}, lens, 700, 14, key_kind, crowd));
    // no candidate, one candidate, one target, more targets than candidates
    REQUIRE(check(PickShape{23, 17, 4, 20, 0}, lens, 0, 3, 0, 0));
    REQUIRE(check(PickShape{23, 17, 4, 20, 0}, lens, 1, 1, 0, 0));
    REQUIRE(check(PickShape{23, 17, 32, 5, 0}, lens, 900, 1, 3, 0));
    REQUIRE(check(PickShape{23, 17, 2, 5, 0}, lens, 50, 400, 3, 0));
    // random shapes
    for (int it = 0; it < 300; ++it) {
        const uint32_t L = 16 + (uint32_t)(std::rand() % 17);
        const PickShape s{L, (uint32_t)(std::rand() % (L + 1)), 1 + (uint32_t)(std::rand() % 32), (uint32_t)(std::rand() % 4 == 0 ? 0 : std::rand() % 200),
                          std::rand() % 3 == 0 ? (uint64_t)(std::rand() & 7) : 0};
        std::vector<uint32_t> cl(1 + std::rand() % 4);
        for (uint32_t &x : cl) x = 10 + (uint32_t)(std::rand() % 3000);
        REQUIRE(check(s, cl, (uint64_t)(std::rand() % 400), 1 + (uint32_t)(std::rand() % 20), std::rand() % 4, std::rand() % 2));
    }
    std::printf("ok: %ld cases, %ld picks\n", g_cases, g_picks);
    return 0;
}
