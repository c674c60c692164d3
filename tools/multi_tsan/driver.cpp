// driver.cpp - runs csrc/vsc_multi.cpp (the real engine) over the host stand-in of the device layer (stub_device.cpp) under
// ThreadSanitizer: plain and streamed searches over 1..7 shards (repeated device ids = device copies, distinct ids with the
// rccl hook off = peer copies), batches of several sizes incl. a ragged last one and more batches than exchange slots, votes
// travelling with the records, a callback that stops the stream, a shard whose search fails in the middle, an empty read set.
// The calls that fan out over the shards and join on the host: the summary rows (plain, region-aware, classified with and
// without the plain rows) against the per-read counts, the timing every join publishes, a shard that fails inside each of
// them (status, no result, the error text, and the same call working afterwards), and a genome of fewer tiles than shards
// (shards without words, the merge context's device among them) through every one of them.
// Every merged batch is compared with the result computed here without threads.  TEST INFRASTRUCTURE ONLY (see run.sh).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "stub_device.h"
#include "varscot_hip_debug.h"
#include "vsc_objects.h"

namespace {
int failures = 0;
#define CHECK(cond, ...)                          \
    do {                                          \
        if (!(cond)) {                            \
            ++failures;                           \
            std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
            std::fprintf(stderr, __VA_ARGS__);    \
            std::fprintf(stderr, "\n");           \
        }                                         \
    } while (0)

struct Expect {
    std::vector<vsc_hit> hits;
    std::vector<uint16_t> votes;
};

// what one batch must look like after the merge: keys ascending, inside a key the shards in order
Expect expected(const std::vector<uint64_t> &codes, uint32_t first, uint32_t cnt, const std::vector<uint64_t> &shard_first_word)
{
    Expect e;
    for (uint32_t i = 0; i < cnt; ++i)
        for (uint32_t s = 0; s < 2; ++s)
            for (uint64_t fw : shard_first_word) {
                const uint64_t code = codes[first + i];
                const uint32_t c = stub::fake_count(code, s, fw);
                for (uint32_t j = 0; j < c; ++j) {
                    vsc_hit r{};
                    r.guide = first + i;
                    r.pos = (uint32_t)(fw * 32 + 7 * j + (uint32_t)(stub::mix(code + s) % 5));
                    r.info = s << 31;
                    e.hits.push_back(r);
                    e.votes.push_back(stub::fake_vote(code, s, r.pos));
                }
            }
    return e;
}

bool same(const vsc_hits *h, const Expect &e)
{
    if (h->n != e.hits.size()) return false;
    for (size_t i = 0; i < e.hits.size(); ++i)
        if (h->host[i].guide != e.hits[i].guide || h->host[i].pos != e.hits[i].pos || h->host[i].info != e.hits[i].info) return false;
    return true;
}

// the first word of every shard that owns words of an n_words genome cut over n shards (vsc_multi.cpp's shard_range)
std::vector<uint64_t> first_words(uint64_t n_words, int n)
{
    std::vector<uint64_t> fw;
    const uint64_t tiles = (n_words + 63) / 64;
    for (int r = 0; r < n; ++r) {
        const uint64_t b = std::min<uint64_t>(tiles * r / n * 64, n_words), e = std::min<uint64_t>(tiles * (r + 1) / n * 64, n_words);
        if (e > b) fw.push_back(b);
    }
    return fw;
}

// the first top_k records of every read (0: all of them), and the reads' record counts before the cut
Expect cut(const Expect &all_of, uint32_t top_k, std::vector<uint64_t> &per_read)
{
    Expect want;
    for (const vsc_hit &r : all_of.hits)
        if (per_read[r.guide]++ < top_k || !top_k) want.hits.push_back(r);
    return want;
}

// the stand-in's rows: every hit counts as an NM 0 hit, and as one vote
bool rows_are(const std::vector<vsc_guide_summary> &rows, const std::vector<uint64_t> &per_read)
{
    for (size_t i = 0; i < per_read.size(); ++i)
        if (rows[i].nm[0] != per_read[i]) return false;
    return true;
}
bool votes_are(const std::vector<vsc_guide_votes> &rows, const std::vector<uint64_t> &per_read)
{
    for (size_t i = 0; i < per_read.size(); ++i)
        if (rows[i].votes_sum != per_read[i] || rows[i].active || rows[i].ties) return false;
    return true;
}

// what a call that joins the shards' results publishes: all contexts of the set, one batch
void check_join_timing(const vsc_multi *m, int n, const char *what)
{
    vsc_multi_timing t{};
    CHECK(vsc_multi_get_timing(m, &t) == VSC_OK && t.n_devices == (uint32_t)n && t.batches == 1u, "timing after %s over %d shards: %u devices, %u batches",
          what, n, t.n_devices, t.batches);
}

struct StreamState {
    const std::vector<uint64_t> *codes;
    const std::vector<uint64_t> *fw;
    bool votes;
    int stop_at;  // batch index at which the callback returns an error (-1: never)
    int seen = 0;
    uint32_t next_first = 0;
};

int on_batch(void *user, vsc_hits *batch, uint32_t first, uint32_t cnt, const uint16_t *votes_dev)
{
    StreamState &st = *(StreamState *)user;
    CHECK(first == st.next_first, "batch starts at read %u, expected %u", first, st.next_first);
    st.next_first = first + cnt;
    const Expect e = expected(*st.codes, first, cnt, *st.fw);
    CHECK(same(batch, e), "batch %d (reads %u..%u): %llu records, expected %zu (or different ones)", st.seen, first, first + cnt,
          (unsigned long long)batch->n, e.hits.size());
    if (st.votes && !e.hits.empty()) {
        CHECK(votes_dev != nullptr, "no votes with batch %d", st.seen);
        if (votes_dev)
            for (size_t i = 0; i < e.votes.size(); ++i)
                if (votes_dev[i] != e.votes[i]) {
                    CHECK(false, "vote %zu of batch %d", i, st.seen);
                    break;
                }
    }
    return st.seen++ == st.stop_at ? VSC_ERR_INVALID : VSC_OK;
}
}  // namespace

int main()
{
    const uint64_t n_words = 64 * 23 + 17;  // 24 tiles, the last one ragged
    std::vector<uint32_t> plane(n_words, 0);
    vsc_contig contig{0, (uint32_t)(n_words * 32), 0};
    vsc_search_params params{};
    params.max_mismatches = 4;
    std::vector<uint64_t> codes(173);
    for (size_t i = 0; i < codes.size(); ++i) codes[i] = stub::mix(i + 1) >> 18;
    vsc_rf_model model{};
    vsc_rf_model one_tree{};  // (the classified summary refuses a forest of 0 trees)
    one_tree.n_trees = 1;
    std::vector<double> activity(codes.size(), 0.5);
    const uint32_t n_codes = (uint32_t)codes.size();
    const vsc_regions regions{};  // (a real object, empty; the stand-in does not consult it and counts every hit as inside)
    const vsc_classify cls{&one_tree, activity.data(), {0, 0}};
    int runs = 0;
    for (int n = 1; n <= 7; ++n)
        for (int distinct = 0; distinct < 2; ++distinct) {
            std::vector<int> ids(n, 0);
            if (distinct)
                for (int i = 0; i < n; ++i) ids[i] = i;
            vsc_multi_debug_params dbg{};
            dbg.rccl = 0;  // device copies / peer copies: RCCL itself is not what this run is about
            vsc_multi *m = nullptr;
            stub::ctx_serial = 0;
            CHECK(vsc_multi_create_debug(ids.data(), n, &dbg, &m) == VSC_OK && m, "create");
            if (!m) continue;
            vsc_multi_genome *g = nullptr;
            CHECK(vsc_multi_genome_load(m, plane.data(), plane.data(), plane.data(), n_words, &contig, 1, &g) == VSC_OK && g, "genome load");
            CHECK(vsc_multi_genome_build_index(m, g, &params) == VSC_OK, "index");
            const std::vector<uint64_t> fw = first_words(n_words, n);
            const uint64_t tiles = (n_words + 63) / 64;
            // one batch
            vsc_hits *all = nullptr;
            CHECK(vsc_multi_search(m, g, codes.data(), (uint32_t)codes.size(), &params, &all) == VSC_OK && all, "search: %s", vsc_multi_last_error(m));
            if (all) {
                CHECK(same(all, expected(codes, 0, (uint32_t)codes.size(), fw)), "vsc_multi_search over %d shards", n);
                vsc_hits_free(all);
            }
            // selection: no cut = the search's records through the exchange; a cut = the first top_k of every read, cut on the host
            for (uint32_t top_k : {0u, 3u}) {
                vsc_select sel{};
                sel.top_k = top_k;
                std::vector<vsc_guide_summary> rows(codes.size());
                vsc_hits *some = nullptr;
                CHECK(vsc_multi_search_select(m, g, codes.data(), (uint32_t)codes.size(), &params, &sel, nullptr, rows.data(), &some) == VSC_OK && some,
                      "select: %s", vsc_multi_last_error(m));
                check_join_timing(m, n, "select");
                std::vector<uint64_t> per_read(codes.size(), 0);
                const Expect want = cut(expected(codes, 0, (uint32_t)codes.size(), fw), top_k, per_read);
                if (some) {
                    CHECK(same(some, want), "vsc_multi_search_select (top_k %u) over %d shards", top_k, n);
                    vsc_hits_free(some);
                }
                for (size_t i = 0; i < codes.size(); ++i)
                    if (rows[i].nm[0] != per_read[i]) {
                        CHECK(false, "summary row %zu of the selection (top_k %u)", i, top_k);
                        break;
                    }
            }
            // the summary rows: the shards' rows added on the host - plain, and the classifier's votes rows with and without the
            // plain ones beside them
            {
                std::vector<uint64_t> per_read(codes.size(), 0);
                (void)cut(expected(codes, 0, n_codes, fw), 0, per_read);
                std::vector<vsc_guide_summary> rows(codes.size());
                CHECK(vsc_multi_search_summary(m, g, codes.data(), n_codes, &params, nullptr, rows.data()) == VSC_OK, "summary: %s", vsc_multi_last_error(m));
                check_join_timing(m, n, "summary");
                CHECK(rows_are(rows, per_read), "vsc_multi_search_summary over %d shards", n);
                for (int with_rows = 1; with_rows >= 0; --with_rows) {
                    std::vector<vsc_guide_summary> plain(codes.size());
                    std::vector<vsc_guide_votes> votes(codes.size());
                    std::memset(votes.data(), 0xEE, votes.size() * sizeof(vsc_guide_votes));  // (the call writes every row)
                    CHECK(vsc_multi_search_summary_classified(m, g, codes.data(), n_codes, &params, nullptr, &cls, with_rows ? plain.data() : nullptr,
                                                              votes.data()) == VSC_OK, "summary_classified: %s", vsc_multi_last_error(m));
                    check_join_timing(m, n, "summary_classified");
                    CHECK(votes_are(votes, per_read), "votes rows of vsc_multi_search_summary_classified over %d shards (out %d)", n, with_rows);
                    CHECK(!with_rows || rows_are(plain, per_read), "plain rows of vsc_multi_search_summary_classified over %d shards", n);
                }
            }
            // the region-aware forms: the same two paths with the extra arguments and the second set of rows
            for (uint32_t top_k : {0u, 3u}) {
                vsc_select sel{};
                sel.top_k = top_k;
                vsc_region_filter flt{&regions, VSC_REGION_KEEP, 0};
                std::vector<vsc_guide_summary> rows(codes.size()), rows_in(codes.size()), sum(codes.size()), sum_in(codes.size());
                vsc_hits *some = nullptr;
                CHECK(vsc_multi_search_select_regions(m, g, codes.data(), (uint32_t)codes.size(), &params, &sel, &flt, nullptr, rows.data(),
                                                      rows_in.data(), &some) == VSC_OK && some, "select_regions: %s", vsc_multi_last_error(m));
                check_join_timing(m, n, "select_regions");
                CHECK(vsc_multi_search_summary_regions(m, g, codes.data(), (uint32_t)codes.size(), &params, nullptr, flt.regions, sum.data(),
                                                       sum_in.data()) == VSC_OK, "summary_regions: %s", vsc_multi_last_error(m));
                check_join_timing(m, n, "summary_regions");
                std::vector<uint64_t> per_read(codes.size(), 0);
                const Expect want = cut(expected(codes, 0, (uint32_t)codes.size(), fw), top_k, per_read);
                if (some) {
                    CHECK(same(some, want), "vsc_multi_search_select_regions (top_k %u) over %d shards", top_k, n);
                    vsc_hits_free(some);
                }
                for (size_t i = 0; i < codes.size(); ++i)
                    if (rows[i].nm[0] != per_read[i] || rows_in[i].nm[0] != per_read[i] || sum[i].nm[0] != per_read[i] || sum_in[i].nm[0] != per_read[i]) {
                        CHECK(false, "rows %zu of the region-aware calls (top_k %u)", i, top_k);
                        break;
                    }
                flt.scope = 2;
                CHECK(vsc_multi_search_select_regions(m, g, codes.data(), (uint32_t)codes.size(), &params, &sel, &flt, nullptr, nullptr, nullptr,
                                                      &some) == VSC_ERR_INVALID && !some, "a bad filter is refused");
            }
            // guide discovery: every shard's arrays, joined in shard order = one entry per tile, ascending; the cap holds for the total
            {
                vsc_enum_params ep{};
                ep.pam[0] = ep.pam[1] = 'G';
                vsc_guides *found = nullptr;
                CHECK(vsc_multi_guides_enumerate(m, g, nullptr, &ep, &found) == VSC_OK && found, "enumerate: %s", vsc_multi_last_error(m));
                check_join_timing(m, n, "enumerate");
                if (found) {
                    const uint64_t *fc = nullptr;
                    const vsc_locus *fl = nullptr;
                    CHECK(vsc_guides_data(found, &fc, &fl) == VSC_OK && vsc_guides_count(found) == tiles, "enumerate: %llu guides",
                          (unsigned long long)vsc_guides_count(found));
                    for (uint64_t t = 0; t < tiles && t < vsc_guides_count(found); ++t)
                        if (fc[t] != t || fl[t].pos != t * 2048) {
                            CHECK(false, "guide %llu of the enumeration over %d shards", (unsigned long long)t, n);
                            break;
                        }
                    vsc_guides_free(found);
                }
                ep.max_guides = tiles - 1;
                CHECK(vsc_multi_guides_enumerate(m, g, nullptr, &ep, &found) == VSC_ERR_RANGE && !found, "the cap holds for the total");
                ep.max_guides = tiles;
                CHECK(vsc_multi_guides_enumerate(m, g, nullptr, &ep, &found) == VSC_OK && found, "a cap at the count");
                vsc_guides_free(found);
            }
            // streams: batch sizes that give 1, 2, 3, many batches (a ragged last one), every scoring mode
            for (uint32_t batch : {173u, 100u, 64u, 7u, 1u})
                for (uint32_t mode : {(uint32_t)VSC_MULTI_SCORE_NONE, (uint32_t)VSC_MULTI_SCORE_ROWS, (uint32_t)VSC_MULTI_SCORE_VOTES}) {
                    if (batch == 1u && (n > 3 || mode == VSC_MULTI_SCORE_ROWS)) continue;  // (173 batches: kept to a few combinations)
                    vsc_multi_score sc{};
                    sc.mode = mode;
                    sc.guide_activity = activity.data();
                    sc.model = &model;
                    StreamState st{&codes, &fw, mode == VSC_MULTI_SCORE_VOTES, -1};
                    const int rc = vsc_multi_search_stream(m, g, codes.data(), (uint32_t)codes.size(), &params, batch, &sc, on_batch, &st);
                    CHECK(rc == VSC_OK, "stream (n %d, batch %u, mode %u): %s", n, batch, mode, vsc_multi_last_error(m));
                    CHECK(st.seen == (int)((codes.size() + batch - 1) / batch) && st.next_first == codes.size(), "stream saw %d batches", st.seen);
                    vsc_multi_timing t{};
                    CHECK(vsc_multi_get_timing(m, &t) == VSC_OK && t.batches == (uint32_t)st.seen && t.n_devices == (uint32_t)n, "timing");
                    ++runs;
                }
            // the callback stops the stream at its third batch: an error, nobody left waiting, the next call works
            {
                StreamState st{&codes, &fw, false, 2};
                const int rc = vsc_multi_search_stream(m, g, codes.data(), (uint32_t)codes.size(), &params, 16, nullptr, on_batch, &st);
                CHECK(rc == VSC_ERR_INVALID && st.seen == 3, "stopped stream: rc %d after %d batches", rc, st.seen);
            }
            // a shard fails in the middle (its fourth batch)
            {
                stub::fail_shard = n - 1;
                stub::fail_code = codes[3 * 16];
                StreamState st{&codes, &fw, false, -1};
                const int rc = vsc_multi_search_stream(m, g, codes.data(), (uint32_t)codes.size(), &params, 16, nullptr, on_batch, &st);
                CHECK(rc == VSC_ERR_DEVICE && st.seen <= 3, "failing shard: rc %d after %d batches (%s)", rc, st.seen, vsc_multi_last_error(m));
                stub::fail_shard = -1;
                stub::fail_code = ~0ull;
            }
            // the last shard fails inside every call that fans out over the shards: the shard's status, its text behind the shard's
            // number, no result - and with the fault cleared the same call works on the same object
            {
                std::vector<vsc_guide_summary> rows(codes.size()), rows_in(codes.size());
                std::vector<vsc_guide_votes> votes(codes.size());
                vsc_select cut3{}, cut0{};
                cut3.top_k = 3;
                const vsc_region_filter flt{&regions, VSC_REGION_KEEP, 0};
                struct Call {
                    const char *name;
                    bool exact;  // the whole text is pinned (the batch engine's: only that it names a shard)
                    std::function<int(vsc_hits **)> run;
                };
                const Call calls[] = {
                    {"summary", true, [&](vsc_hits **) { return vsc_multi_search_summary(m, g, codes.data(), n_codes, &params, nullptr, rows.data()); }},
                    {"summary_regions", true,
                     [&](vsc_hits **) { return vsc_multi_search_summary_regions(m, g, codes.data(), n_codes, &params, nullptr, &regions, rows.data(), rows_in.data()); }},
                    {"summary_classified", true,
                     [&](vsc_hits **) { return vsc_multi_search_summary_classified(m, g, codes.data(), n_codes, &params, nullptr, &cls, rows.data(), votes.data()); }},
                    {"select, top_k 3", true, [&](vsc_hits **h) { return vsc_multi_search_select(m, g, codes.data(), n_codes, &params, &cut3, nullptr, rows.data(), h); }},
                    {"select, top_k 0", false, [&](vsc_hits **h) { return vsc_multi_search_select(m, g, codes.data(), n_codes, &params, &cut0, nullptr, rows.data(), h); }},
                    {"select_regions, top_k 3", true,
                     [&](vsc_hits **h) { return vsc_multi_search_select_regions(m, g, codes.data(), n_codes, &params, &cut3, &flt, nullptr, rows.data(), rows_in.data(), h); }},
                };
                const std::string text = "shard " + std::to_string(n - 1) + ": stub: this shard was told to fail";
                for (const Call &c : calls) {
                    stub::fail_shard = n - 1;
                    stub::fail_code = codes[0];
                    vsc_hits *h = nullptr;
                    const int rc = c.run(&h);
                    const std::string err = vsc_multi_last_error(m);
                    CHECK(rc == VSC_ERR_DEVICE && !h, "%s with a failing shard (n %d): rc %d", c.name, n, rc);
                    CHECK(c.exact ? err == text : err.rfind("shard ", 0) == 0, "%s with a failing shard (n %d) says \"%s\"", c.name, n, err.c_str());
                    stub::fail_shard = -1;
                    stub::fail_code = ~0ull;
                    h = nullptr;
                    CHECK(c.run(&h) == VSC_OK, "%s after the failure (n %d): %s", c.name, n, vsc_multi_last_error(m));
                    check_join_timing(m, n, c.name);
                    if (h) vsc_hits_free(h);
                }
            }
            // no reads; then an ordinary search again on the same object
            {
                vsc_hits *none = nullptr;
                CHECK(vsc_multi_search(m, g, codes.data(), 0, &params, &none) == VSC_OK && none && none->n == 0, "empty read set");
                if (none) vsc_hits_free(none);
                vsc_hits *again = nullptr;
                CHECK(vsc_multi_search(m, g, codes.data(), 50, &params, &again) == VSC_OK && again && same(again, expected(codes, 0, 50, fw)), "search after the failures");
                if (again) vsc_hits_free(again);
            }
            CHECK(vsc_multi_release_scratch(m) == VSC_OK, "release scratch");
            vsc_multi_genome_free(g);
            vsc_multi_destroy(m);
        }
    // fewer tiles than shards: 3 tiles on 5 contexts leave shards 0 and 2 without words - shard 0 is the merge context's device
    for (int distinct = 0; distinct < 2; ++distinct) {
        const int n = 5;
        const uint64_t small_words = 64 * 2 + 5, tiles = 3;
        std::vector<int> ids(n, 0);
        if (distinct)
            for (int i = 0; i < n; ++i) ids[i] = i;
        vsc_multi_debug_params dbg{};
        dbg.rccl = 0;
        vsc_multi *m = nullptr;
        stub::ctx_serial = 0;
        CHECK(vsc_multi_create_debug(ids.data(), n, &dbg, &m) == VSC_OK && m, "create (small genome)");
        if (!m) continue;
        vsc_contig small_contig{0, (uint32_t)(small_words * 32), 0};
        vsc_multi_genome *g = nullptr;
        CHECK(vsc_multi_genome_load(m, plane.data(), plane.data(), plane.data(), small_words, &small_contig, 1, &g) == VSC_OK && g, "small genome load");
        CHECK(vsc_multi_genome_build_index(m, g, &params) == VSC_OK, "small genome index");
        const std::vector<uint64_t> fw = first_words(small_words, n);
        CHECK(fw.size() == 3 && fw[0] == 0 && fw[1] == 64 && fw[2] == 128, "the small genome's owning shards");
        std::vector<uint64_t> per_read(codes.size(), 0);
        const Expect all_of = expected(codes, 0, n_codes, fw);
        (void)cut(all_of, 0, per_read);
        vsc_hits *all = nullptr;
        CHECK(vsc_multi_search(m, g, codes.data(), n_codes, &params, &all) == VSC_OK && all, "small genome search: %s", vsc_multi_last_error(m));
        check_join_timing(m, n, "search (small genome)");
        if (all) {
            CHECK(same(all, all_of), "vsc_multi_search of the small genome");
            vsc_hits_free(all);
        }
        std::vector<vsc_guide_summary> rows(codes.size()), plain(codes.size());
        std::vector<vsc_guide_votes> votes(codes.size());
        CHECK(vsc_multi_search_summary(m, g, codes.data(), n_codes, &params, nullptr, rows.data()) == VSC_OK, "small genome summary: %s", vsc_multi_last_error(m));
        check_join_timing(m, n, "summary (small genome)");
        CHECK(rows_are(rows, per_read), "vsc_multi_search_summary of the small genome");
        CHECK(vsc_multi_search_summary_classified(m, g, codes.data(), n_codes, &params, nullptr, &cls, plain.data(), votes.data()) == VSC_OK,
              "small genome summary_classified: %s", vsc_multi_last_error(m));
        check_join_timing(m, n, "summary_classified (small genome)");
        CHECK(rows_are(plain, per_read) && votes_are(votes, per_read), "vsc_multi_search_summary_classified of the small genome");
        for (uint32_t top_k : {0u, 3u}) {
            vsc_select sel{};
            sel.top_k = top_k;
            std::vector<vsc_guide_summary> srows(codes.size());
            vsc_hits *some = nullptr;
            CHECK(vsc_multi_search_select(m, g, codes.data(), n_codes, &params, &sel, nullptr, srows.data(), &some) == VSC_OK && some,
                  "small genome select: %s", vsc_multi_last_error(m));
            check_join_timing(m, n, "select (small genome)");
            std::vector<uint64_t> counted(codes.size(), 0);
            const Expect want = cut(all_of, top_k, counted);
            if (some) {
                CHECK(same(some, want), "vsc_multi_search_select (top_k %u) of the small genome", top_k);
                vsc_hits_free(some);
            }
            CHECK(rows_are(srows, per_read), "rows of the selection (top_k %u) of the small genome", top_k);
        }
        vsc_enum_params ep{};
        ep.pam[0] = ep.pam[1] = 'G';
        vsc_guides *found = nullptr;
        CHECK(vsc_multi_guides_enumerate(m, g, nullptr, &ep, &found) == VSC_OK && found, "small genome enumerate: %s", vsc_multi_last_error(m));
        check_join_timing(m, n, "enumerate (small genome)");
        if (found) {
            const uint64_t *fc = nullptr;
            const vsc_locus *fl = nullptr;
            CHECK(vsc_guides_data(found, &fc, &fl) == VSC_OK && vsc_guides_count(found) == tiles, "small genome enumerate: %llu guides",
                  (unsigned long long)vsc_guides_count(found));
            for (uint64_t t = 0; t < tiles && t < vsc_guides_count(found); ++t)
                CHECK(fc[t] == t && fl[t].pos == t * 2048, "guide %llu of the small genome's enumeration", (unsigned long long)t);
            vsc_guides_free(found);
        }
        CHECK(vsc_multi_release_scratch(m) == VSC_OK, "release scratch (small genome)");
        vsc_multi_genome_free(g);
        vsc_multi_destroy(m);
    }
    std::printf("multi_tsan: %d streamed runs over 1..7 shards, %llu merges, %llu queued copies performed, %d failures\n", runs,
                (unsigned long long)stub::merges.load(), (unsigned long long)stub::copies.load(), failures);
    return failures ? 1 : 0;
}
