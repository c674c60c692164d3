// vsc_multi.cpp - the genome-sharded multi-GPU search behind the C ABI: one host process, one vsc_ctx per
// device, the packed planes cut into tile-aligned position ranges (+ one halo word), every device searching ALL
// reads on its shard from its own host thread, then exactly one exchange of hit records to the first device
// over RCCL (xGMI) and the segment merge there.  This is where VARSCOT_pipeline/read_mapping/bidir_mapping.cpp
// has its OpenMP loop over reads (:285-295) and the concatenation of the per-thread buffers (:307-308): the
// parallel axis is the genome instead of the reads, the concatenation becomes gather + merge.
//
// RCCL is bound at run time (dlopen): the library loads and works on one device without it, and in a Python
// process it shares the copy PyTorch has already loaded.  Devices may repeat in the list (several contexts on
// one GPU - how the tests run N shards on a one-GPU box); the exchange then is plain device copies.
//
// One engine (BatchRun) serves vsc_multi_search (one batch), vsc_multi_search_stream and the selection without a cut: a host
// thread per shard searches (and scores) batch after batch into one of two exchange slots; the calling thread sends every
// shard's records to the first device the moment THAT shard is ready, merges the batch on a context of its own there and hands
// it to the caller - while the shards are already searching the next batch.
//
// Every other call runs one single-device call per shard and joins the results on the host: fan_out() is that one step (a thread
// per shard, shards without words skipped, the shards' timings and the wall time recorded, the first failing shard reported),
// join_rows() adds the per-guide rows of the summaries (plain, region-aware, classified), multi_select() cuts the shards'
// survivors on the host, vsc_multi_guides_enumerate concatenates the shards' arrays.
#include <dlfcn.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include <rccl/rccl.h>

#include "vsc_objects.h"

using namespace vsc;

namespace {

struct Rccl {
    void *lib = nullptr;
    decltype(&ncclCommInitAll) CommInitAll = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclCommAbort) CommAbort = nullptr;  // optional
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclSend) Send = nullptr;
    decltype(&ncclRecv) Recv = nullptr;
    decltype(&ncclAllGather) AllGather = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;

    // `only` (tests): the one library name to try instead of the usual two
    bool load(std::string *why, const char *only = nullptr)
    {
        if (lib) return true;
        std::string last;
        std::vector<const char *> names;
        if (only) names = {only};
        else names = {"librccl.so.1", "librccl.so"};
        for (const char *name : names) {
            lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
            if (lib) break;
            const char *e = dlerror();  // (one call: dlerror() clears the state it reports)
            last = e ? e : "dlopen failed";
        }
        if (!lib) {
            *why = "RCCL not found: " + last;
            return false;
        }
        auto sym = [&](const char *n) { return dlsym(lib, n); };
        CommInitAll = (decltype(CommInitAll))sym("ncclCommInitAll");
        CommDestroy = (decltype(CommDestroy))sym("ncclCommDestroy");
        CommAbort = (decltype(CommAbort))sym("ncclCommAbort");
        GroupStart = (decltype(GroupStart))sym("ncclGroupStart");
        GroupEnd = (decltype(GroupEnd))sym("ncclGroupEnd");
        Send = (decltype(Send))sym("ncclSend");
        Recv = (decltype(Recv))sym("ncclRecv");
        AllGather = (decltype(AllGather))sym("ncclAllGather");
        GetErrorString = (decltype(GetErrorString))sym("ncclGetErrorString");
        if (!CommInitAll || !CommDestroy || !GroupStart || !GroupEnd || !Send || !Recv || !AllGather || !GetErrorString) {
            *why = "RCCL library lacks a required entry point";
            return false;
        }
        return true;
    }
};

}  // namespace

struct vsc_multi {
    std::vector<int> device;
    std::vector<vsc_ctx *> ctx;
    vsc_ctx *merge_ctx = nullptr;       // on device[0]: owns the merged results; its stream is not a shard's
    std::vector<hipStream_t> xstream;   // exchange streams, one per context (RCCL's streams)
    bool use_rccl = false;
    Rccl rccl;
    std::vector<ncclComm_t> comm;
    // exchange buffers: two slots per shard on the shard's device (records, votes) - a shard fills one while the other is
    // being sent - and one landing buffer per shard on device[0]
    std::vector<DeviceBuf> xbuf[2], vbuf[2];
    std::vector<DeviceBuf> gbuf, gvotes;
    DeviceBuf votes_out;                // on device[0]: the merged batch's votes
    std::string err;
    vsc_multi_timing timing{};
};

struct vsc_multi_genome {
    vsc_multi *multi = nullptr;
    std::vector<vsc_genome *> shard;    // null: the shard owns no words of this (small) genome
    vsc_genome *table = nullptr;        // the contig table on the first device, for the merge context
};

namespace {

int mfail(vsc_multi *m, int code, const std::string &what)
{
    if (m) m->err = what;
    return code;
}

// inside BatchRun's exchange steps (-> bool): a HIP call that fails stops the run, with the call as the error's text
#define VSC_X(call)                                                                                                                   \
    do {                                                                                                                              \
        const hipError_t e_ = (call);                                                                                                 \
        if (e_ != hipSuccess)                                                                                                         \
            return stop(e_ == hipErrorOutOfMemory ? VSC_ERR_NOMEM : VSC_ERR_DEVICE, std::string(#call ": ") + hipGetErrorString(e_)); \
    } while (0)

using clk = std::chrono::steady_clock;
double ms_between(clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); }

// tile-aligned word range of shard r of n (the same cut as varscot_amd.api.PackedGenome.shard_words)
void shard_range(uint64_t n_words, unsigned r, unsigned n, uint64_t *b, uint64_t *e)
{
    const uint64_t tiles = (n_words + kTileWords - 1) / kTileWords;
    *b = std::min<uint64_t>(tiles * r / n * kTileWords, n_words);
    *e = std::min<uint64_t>(tiles * (r + 1) / n * kTileWords, n_words);
}

// joins what was started, whatever ends the scope (a thread that cannot be started, an exception in body(0))
struct JoinAll {
    std::vector<std::thread> &pool;
    ~JoinAll()
    {
        for (auto &t : pool)
            if (t.joinable()) t.join();
    }
};

// body(i) for every i on a thread of its own (i = 0 on this one).  The bodies call the C ABI, which throws nothing.
template <class F> void on_all(size_t n, F &&body)
{
    std::vector<std::thread> pool;
    pool.reserve(n);
    JoinAll join{pool};
    for (size_t i = 1; i < n; ++i) pool.emplace_back([&, i] { body(i); });
    if (n) body(0);
}

// what fan_out recorded for the timing of the call (store_join_timing): begun at t0, tm[r] = shard r's own timing (zero: it owns
// no words), wall = the fan-out up to the last shard
struct FanOut {
    clk::time_point t0;
    std::vector<vsc_timing> tm;
    double wall = 0;
};

// The step every call but the batch engine is made of: body(r) -> status for every shard on a thread of its own (on_all), the
// first failing shard in shard order as the call's error.  g: the shards that own no words of this genome are skipped (null:
// the body decides).  `rec` (optional) records the timing.  A shard's timing is taken after its body whatever the status: a
// failed call publishes no timing, and what the bodies do after their search (vsc_hits_copy, vsc_score_hits, vsc_guides_data)
// changes neither total_ms nor hits of the context's timing - all that store_join_timing reads.
template <class F> int fan_out(vsc_multi *m, const vsc_multi_genome *g, FanOut *rec, F &&body)
{
    const size_t n = m->ctx.size();
    const auto t0 = clk::now();
    std::vector<int> rc(n, VSC_OK);
    std::vector<vsc_timing> tm(n);
    on_all(n, [&](size_t r) {
        if (g && !g->shard[r]) return;
        rc[r] = body(r);
        (void)vsc_ctx_timing(m->ctx[r], &tm[r]);
    });
    for (size_t r = 0; r < n; ++r)
        if (rc[r] != VSC_OK) return mfail(m, rc[r], "shard " + std::to_string(r) + ": " + vsc_last_error(m->ctx[r]));
    if (rec) *rec = FanOut{t0, std::move(tm), ms_between(t0, clk::now())};
    return VSC_OK;
}

// the exchange, landing and votes buffers go back to their devices
void release_buffers(vsc_multi *m)
{
    if (!m->device.empty()) {
        (void)hipSetDevice(m->device[0]);
        for (auto &b : m->gbuf) b.release();
        for (auto &b : m->gvotes) b.release();
        m->votes_out.release();
    }
    for (size_t i = 0; i < m->ctx.size(); ++i) {
        (void)hipSetDevice(m->device[i]);
        for (int k = 0; k < 2; ++k) {
            if (i < m->xbuf[k].size()) m->xbuf[k][i].release();
            if (i < m->vbuf[k].size()) m->vbuf[k][i].release();
        }
    }
}

// no C++ exception crosses the C boundary
template <class F> int mguarded(vsc_multi *m, F &&body) noexcept
{
    try {
        return body();
    } catch (const std::bad_alloc &) {
        try {
            if (m) m->err = "out of host memory";
        } catch (...) {
        }
        return VSC_ERR_NOMEM;
    } catch (...) {
        try {
            if (m) m->err = "unexpected C++ exception";
        } catch (...) {
        }
        return VSC_ERR_DEVICE;
    }
}

// on_batch(hits, first read, reads, votes on the first device or null) -> status; *keep = true: the callback took the hits over
typedef std::function<int(vsc_hits *, uint32_t, uint32_t, const uint16_t *, bool *)> BatchSink;
// what shard r runs in place of vsc_search on its context (vsc_multi_search_select without a cut: one batch, all reads)
typedef std::function<int(size_t, vsc_hits **)> ShardSearch;

// what the shard threads hand to the exchange thread, per slot
struct Slot {
    std::vector<uint64_t> count;       // records of shard r
    std::vector<uint32_t> key_counts;  // [r * K + k], K = 2 x the batch's reads (keys of a batch: read << 1 | strand)
    Slot(size_t n, uint32_t max_reads) : count(n, 0), key_counts(n * (size_t)(2 * max_reads), 0) {}
};

// Whatever ends the scope it lives in - also an exception on the exchange thread, or a shard thread that cannot be started -:
// the shard threads are told to stop (they wait on `failed`) before they are joined.
struct StopAndJoin {
    JoinAll join;  // (a member's destructor runs after the body of this one's: told to stop first, then joined)
    std::mutex &mu;
    std::condition_variable &cv;
    std::atomic<int> &failed;
    bool done = false;  // the loop over the batches finished (a stream that broke off has set `failed` itself)
    ~StopAndJoin()
    {
        if (!done) {
            std::lock_guard<std::mutex> lk(mu);
            if (failed == VSC_OK) failed = VSC_ERR_NOMEM;
        }
        cv.notify_all();
    }
};

// An exchange buffer of a shard, for `bytes` -> status (`what` as the context's error).  One that does not fit beside the context's
// pooled scratch: the scratch goes back first.
int ensure_beside_scratch(vsc_ctx *ctx, DeviceBuf &buf, size_t bytes, const char *what)
{
    if (buf.ensure(bytes) == hipSuccess) return VSC_OK;
    (void)hipGetLastError();
    (void)vsc_ctx_release_scratch(ctx);
    if (buf.ensure(bytes) == hipSuccess) return VSC_OK;
    ctx->err = what;
    return VSC_ERR_NOMEM;
}

// The engine behind vsc_multi_search, vsc_multi_search_stream and the selection without a cut (see the head of this file): one
// run over the batches of a read set.  shard_thread (one per shard) -> pack; the calling thread is the exchange thread: run ->
// transfer, finish_transfers, merge_and_deliver.
struct BatchRun {
    // ---- the call: run_batches' arguments (batch: 1..n_guides reads, or 1 for no reads) ----
    vsc_multi *const m;
    const vsc_multi_genome *const g;
    const uint64_t *const guides;
    const uint32_t n_guides;
    const vsc_search_params *const params;
    const uint32_t batch;
    const vsc_multi_score *const score;
    const BatchSink &sink;
    const ShardSearch &shard_search;
    const size_t n = m->ctx.size();
    const uint32_t mode = score ? score->mode : VSC_MULTI_SCORE_NONE;
    const bool votes = mode == VSC_MULTI_SCORE_VOTES;
    const uint32_t n_batches = std::max<uint32_t>(1, (n_guides + batch - 1) / batch);
    const clk::time_point t0 = clk::now();

    // ---- what the shard threads and the exchange thread share ----
    // `mu` guards produced, transferred, finished, why and every write to `failed`; `cv` is notified after each change of them.
    std::mutex mu{};  // (the {}: the struct is filled by aggregate initialisation, which wants every member named or initialised)
    std::condition_variable cv{};
    std::vector<uint32_t> produced = std::vector<uint32_t>(n, 0);  // batches shard r has searched, scored and packed
    uint32_t transferred = 0;                                      // batches whose exchange slots have been read out
    // (written under `mu`, which is what the waits re-check it under; atomic because the exchange thread's loops also look at it
    // between two waits, without the lock)
    std::atomic<int> failed{VSC_OK};
    std::string why{};
    std::vector<clk::time_point> finished = std::vector<clk::time_point>(n, t0);
    // Per shard, written by the shard's own thread only, without the lock: row r of slot[b & 1] between the wait for
    // `transferred + 2 > b` and the publication of produced[r] = b + 1 (the exchange thread reads it between seeing that and
    // publishing transferred = b + 1); search_ms, score_ms and shard_hits until the thread ends (read after the join).
    Slot slot[2] = {Slot(n, batch), Slot(n, batch)};
    std::vector<double> search_ms = std::vector<double>(n, 0), score_ms = search_ms;
    std::vector<uint64_t> shard_hits = std::vector<uint64_t>(n, 0);
    // ---- the exchange thread's own ----
    vsc_multi_timing mt{};

    uint32_t first_of(uint32_t b) const { return b * batch; }
    uint32_t reads_of(uint32_t b) const { return std::min<uint32_t>(batch, n_guides - std::min(n_guides, first_of(b))); }

    void fail_all(int code, const std::string &text)
    {
        std::lock_guard<std::mutex> lk(mu);
        if (failed == VSC_OK) {
            failed = code;
            why = text;
        }
        cv.notify_all();
    }
    bool stop(int code, const std::string &text)  // (as the exchange thread's steps fail)
    {
        fail_all(code, text);
        return false;
    }

    // What happens to the result of batch b on shard r: the caller's per-hit scores where the hits were found (rows_done: the
    // search has written them on its way), then the records (+ votes) packed for the exchange.
    int pack(size_t r, uint32_t b, vsc_hits *part, bool rows_done)
    {
        vsc_ctx *ctx = m->ctx[r];
        const uint32_t first = first_of(b), cnt = reads_of(b);
        Slot &s = slot[b & 1];
        int rc = VSC_OK;
        vsc_timing t{};
        (void)vsc_ctx_timing(ctx, &t);
        search_ms[r] += t.total_ms;
        shard_hits[r] += t.hits;
        const uint64_t c = vsc_hits_count(part);
        s.count[r] = c;
        if (c && mode == VSC_MULTI_SCORE_ROWS && !rows_done)
            rc = vsc_score_hits_packed(ctx, g->shard[r], part, guides + first, cnt, 0, c, nullptr, nullptr, nullptr);
        if (rc == VSC_OK && c && votes) rc = ensure_beside_scratch(ctx, m->vbuf[b & 1][r], c * sizeof(uint16_t), "vote buffer allocation failed");
        if (rc == VSC_OK && c && votes)
            rc = vsc_score_classify_hits(ctx, g->shard[r], part, guides + first, cnt, score->guide_activity + first, score->model, 0, c,
                                         m->vbuf[b & 1][r].p, nullptr, nullptr);
        if (rc == VSC_OK && mode != VSC_MULTI_SCORE_NONE && c && !rows_done) {
            (void)vsc_ctx_timing(ctx, &t);
            score_ms[r] += t.score_ms;
        }
        if (rc == VSC_OK) rc = ensure_beside_scratch(ctx, m->xbuf[b & 1][r], std::max<uint64_t>(c, 1) * VSC_XREC_BYTES, "exchange buffer allocation failed");
        if (rc == VSC_OK) rc = vsc_hits_pack_exchange(ctx, g->shard[r], part, cnt, m->xbuf[b & 1][r].p, 1, s.key_counts.data() + r * (size_t)(2 * cnt));
        return rc;
    }

    // shard r's thread: batch after batch searched and packed into its row of the batch's slot
    void shard_thread(size_t r)
    {
        try {  // (no exception leaves a thread: the host allocations in there are strings and small vectors)
            if (hipSetDevice(m->device[r]) != hipSuccess) return fail_all(VSC_ERR_DEVICE, "shard " + std::to_string(r) + ": hipSetDevice failed");
            for (uint32_t b = 0; b < n_batches; ++b) {
                {
                    std::unique_lock<std::mutex> lk(mu);  // this batch's slot was batch b - 2's: wait until that one has been sent
                    cv.wait(lk, [&] { return failed != VSC_OK || transferred + 2 > b; });
                    if (failed != VSC_OK) return;
                }
                const uint32_t first = first_of(b), cnt = reads_of(b), K = 2 * cnt;
                Slot &s = slot[b & 1];
                s.count[r] = 0;
                std::fill(s.key_counts.begin() + r * (size_t)K, s.key_counts.begin() + (r + 1) * (size_t)K, 0u);
                if (g->shard[r]) {
                    vsc_ctx *ctx = m->ctx[r];
                    int rc;
                    if (mode == VSC_MULTI_SCORE_ROWS) {
                        // the feature rows are written on the way (vsc_search_stream_rows: one batch = the whole read range of this
                        // step), a consumer on the shard would read them inside the callback.  (No reads: no batch, no callback.)
                        auto packed = [&](vsc_hits *part) { return pack(r, b, part, true); };
                        rc = vsc_search_stream_rows(ctx, g->shard[r], guides + first, cnt, params, cnt,
                                                    [](void *u, vsc_hits *part, uint32_t, uint32_t, const void *) { return (*(decltype(packed) *)u)(part); }, &packed);
                    } else {
                        vsc_hits *part = nullptr;
                        rc = shard_search ? shard_search(r, &part) : vsc_search(ctx, g->shard[r], guides + first, cnt, params, &part);
                        if (rc == VSC_OK) {
                            rc = pack(r, b, part, false);
                            vsc_hits_free(part);  // the 8-byte records carry everything the merge needs
                        }
                    }
                    if (rc != VSC_OK) return fail_all(rc, "shard " + std::to_string(r) + ": " + vsc_last_error(ctx));
                }
                {
                    std::lock_guard<std::mutex> lk(mu);
                    produced[r] = b + 1;
                    finished[r] = clk::now();
                }
                cv.notify_all();
            }
        } catch (...) {
            std::lock_guard<std::mutex> lk(mu);
            if (failed == VSC_OK) failed = VSC_ERR_NOMEM;
            cv.notify_all();
        }
    }

    // Inside an RCCL group nothing may return early: an open group makes every later call on these communicators queue
    // forever.  The first failure is kept, the group is closed, and the communicators are given up (a half-issued
    // send / receive pairing cannot be repaired): later searches use device copies.
    bool give_up_rccl(const char *where, ncclResult_t bad)
    {
        for (ncclComm_t &c : m->comm) {
            if (c && m->rccl.CommAbort) (void)m->rccl.CommAbort(c);
            c = nullptr;
        }
        m->comm.clear();
        m->use_rccl = false;
        return stop(VSC_ERR_DEVICE, std::string(where) + ": " + m->rccl.GetErrorString(bad) + " (RCCL given up, later searches copy)");
    }

    // shard r's records (+ votes) of batch b to the first device
    bool transfer(size_t r, uint32_t b)
    {
        const uint64_t c = slot[b & 1].count[r];
        if (!c) return true;
        struct Leg {
            DeviceBuf &land;  // on the first device
            const void *src;  // on the shard's
            size_t bytes;
        };
        std::vector<Leg> legs{{m->gbuf[r], m->xbuf[b & 1][r].p, c * VSC_XREC_BYTES}};
        if (votes) legs.push_back({m->gvotes[r], m->vbuf[b & 1][r].p, c * sizeof(uint16_t)});
        VSC_X(hipSetDevice(m->device[0]));
        for (const Leg &l : legs) VSC_X(l.land.ensure(l.bytes));
        // (RCCL with ONE device - the hook rccl = 1 / 2 on a one-GPU box - sends to itself, so that the calls are exercised there)
        if (m->device[r] == m->device[0] && !(m->use_rccl && n == 1)) {
            // (r != 0: another context on the same device, a rehearsal)
            for (const Leg &l : legs) VSC_X(hipMemcpyAsync(l.land.p, l.src, l.bytes, hipMemcpyDeviceToDevice, m->xstream[0]));
        } else if (m->use_rccl) {
            ncclResult_t bad = ncclSuccess;
            auto in_group = [&](ncclResult_t x) {
                if (bad == ncclSuccess && x != ncclSuccess) bad = x;
            };
            in_group(m->rccl.GroupStart());
            if (bad == ncclSuccess) {
                // (one thread drives both ends: the current device is set to the communicator's before each call, as
                // RCCL's single-process examples do)
                (void)hipSetDevice(m->device[0]);
                for (const Leg &l : legs) in_group(m->rccl.Recv(l.land.p, l.bytes, ncclUint8, (int)r, m->comm[0], m->xstream[0]));
                (void)hipSetDevice(m->device[r]);
                for (const Leg &l : legs) in_group(m->rccl.Send(l.src, l.bytes, ncclUint8, 0, m->comm[r], m->xstream[r]));
                in_group(m->rccl.GroupEnd());
                (void)hipSetDevice(m->device[0]);
            }
            if (bad != ncclSuccess) return give_up_rccl("send / receive of the hit records", bad);
        } else {
            for (const Leg &l : legs) VSC_X(hipMemcpyPeerAsync(l.land.p, m->device[0], l.src, m->device[r], l.bytes, m->xstream[0]));
        }
        // (shard 0's records never leave the first device; a peer copy's shard is never shard 0)
        if (r != 0)
            for (const Leg &l : legs) mt.exchanged_bytes += l.bytes;
        return true;
    }

    // everything issued for this batch has arrived / left
    bool finish_transfers()
    {
        VSC_X(hipSetDevice(m->device[0]));
        VSC_X(hipStreamSynchronize(m->xstream[0]));
        if (m->use_rccl)
            for (size_t r = 1; r < n; ++r) {
                VSC_X(hipSetDevice(m->device[r]));
                VSC_X(hipStreamSynchronize(m->xstream[r]));
            }
        return true;
    }

    // Batch b has arrived (at t_arrived): its slot goes back to the shards, the merge on the first device - shards partition the
    // positions in ascending order -, and the batch to the caller.
    bool merge_and_deliver(uint32_t b, clk::time_point t_arrived)
    {
        const uint32_t first = first_of(b), cnt = reads_of(b), K = 2 * cnt;
        const Slot &s = slot[b & 1];
        std::vector<uint32_t> kc(s.key_counts.begin(), s.key_counts.begin() + n * (size_t)K);  // (the slot is reused two batches on)
        {
            std::lock_guard<std::mutex> lk(mu);
            transferred = b + 1;
        }
        cv.notify_all();
        std::vector<const void *> rec_ptr(n), vote_ptr(n);
        for (size_t r = 0; r < n; ++r) {
            rec_ptr[r] = m->gbuf[r].p;
            vote_ptr[r] = m->gvotes[r].p;
        }
        vsc_hits *merged = nullptr;
        const int mrc = merge_packed_shards(m->merge_ctx, g->table, rec_ptr.data(), votes ? vote_ptr.data() : nullptr, kc.data(), (uint32_t)n,
                                            2 * first, K, &merged, votes ? &m->votes_out : nullptr);
        if (mrc != VSC_OK) return stop(mrc, std::string("merge: ") + vsc_last_error(m->merge_ctx));
        const auto t_merged = clk::now();
        mt.merge_ms += ms_between(t_arrived, t_merged);
        bool keep = false;
        const int crc = sink(merged, first, cnt, votes && vsc_hits_count(merged) ? (const uint16_t *)m->votes_out.p : nullptr, &keep);
        if (!keep) vsc_hits_free(merged);
        mt.callback_ms += ms_between(t_merged, clk::now());
        return crc == VSC_OK || stop(crc, "the batch callback stopped the stream");
    }

    // the exchange thread: starts the shards' threads, then per batch sends what is ready, waits for it, merges and delivers
    int run()
    {
        std::vector<std::thread> pool;
        pool.reserve(n);
        StopAndJoin joiner{{pool}, mu, cv, failed};
        for (size_t r = 0; r < n; ++r) pool.emplace_back(&BatchRun::shard_thread, this, r);
        for (uint32_t b = 0; b < n_batches && failed == VSC_OK; ++b) {
            std::vector<char> sent(n, 0);
            size_t n_sent = 0;
            bool ok = true;
            clk::time_point all_ready = clk::now();
            while (n_sent < n && ok) {
                std::vector<size_t> ready;
                {
                    std::unique_lock<std::mutex> lk(mu);
                    cv.wait(lk, [&] {
                        if (failed != VSC_OK) return true;
                        for (size_t r = 0; r < n; ++r)
                            if (!sent[r] && produced[r] > b) return true;
                        return false;
                    });
                    if (failed != VSC_OK) break;
                    for (size_t r = 0; r < n; ++r)
                        if (!sent[r] && produced[r] > b) ready.push_back(r);
                }
                all_ready = clk::now();
                for (size_t r : ready) {  // a shard's records leave the moment it is done - the others are still sorting
                    ok = ok && transfer(r, b);
                    sent[r] = 1;
                    ++n_sent;
                }
            }
            if (failed != VSC_OK || !ok) break;
            if (!finish_transfers()) break;
            const auto t_arrived = clk::now();
            mt.exchange_ms += ms_between(all_ready, t_arrived);
            if (!merge_and_deliver(b, t_arrived)) break;
            mt.batches++;
        }
        joiner.done = true;
        for (auto &t : pool) t.join();
        // (the exchange and landing buffers stay pooled, like every context's scratch: hipMalloc / hipFree of 13 GB cost hundreds
        // of milliseconds per search - vsc_multi_release_scratch gives them back)
        if (failed != VSC_OK) return mfail(m, failed, why);
        clk::time_point last = t0;
        for (size_t r = 0; r < n; ++r) {
            last = std::max(last, finished[r]);
            mt.search_ms_max = std::max(mt.search_ms_max, search_ms[r]);
            mt.score_ms_max = std::max(mt.score_ms_max, score_ms[r]);
            mt.hits += shard_hits[r];
        }
        mt.search_wall_ms = ms_between(t0, last);
        mt.total_ms = ms_between(t0, clk::now());
        mt.n_devices = (uint32_t)n;
        mt.used_rccl = m->use_rccl;
        m->timing = mt;
        return VSC_OK;
    }
};
#undef VSC_X

int run_batches(vsc_multi *m, const vsc_multi_genome *g, const uint64_t *guides, uint32_t n_guides, const vsc_search_params *params,
                uint32_t batch, const vsc_multi_score *score, const BatchSink &sink, const ShardSearch &shard_search = nullptr)
{
    if (batch == 0 || batch > n_guides) batch = std::max<uint32_t>(n_guides, 1);
    return BatchRun{m, g, guides, n_guides, params, batch, score, sink, shard_search}.run();
}

// the sink of a run of one batch whose merged hits are the call's result
BatchSink hand_over(vsc_hits **out)
{
    return [out](vsc_hits *h, uint32_t, uint32_t, const uint16_t *, bool *keep) {
        *out = h;
        *keep = true;
        return VSC_OK;
    };
}

// o += p, as the rows of genome shards add: fixed-point MIT sums and counts exactly; a locus lies in one shard only
void add_row(vsc_guide_summary &o, const vsc_guide_summary &p)
{
    o.mit_sum += p.mit_sum;
    for (int k = 0; k <= VSC_MAX_MISMATCHES; ++k) o.nm[k] += p.nm[k];
    o.mit_ub += p.mit_ub;
    o.on_target |= p.on_target;
}
// ... and the votes rows: every field is a sum of integers
void add_row(vsc_guide_votes &o, const vsc_guide_votes &p)
{
    o.votes_sum += p.votes_sum;
    o.active += p.active;
    o.ties += p.ties;
    for (int k = 0; k <= VSC_MAX_MISMATCHES; ++k) o.active_nm[k] += p.active_nm[k];
}

// ... and the table rows: sums of fixed-point scores and counts
void add_row(vsc_guide_table_row &o, const vsc_guide_table_row &p)
{
    o.score_sum += p.score_sum;
    o.positive += p.positive;
    for (int k = 0; k <= VSC_MAX_MISMATCHES; ++k) o.positive_nm[k] += p.positive_nm[k];
}

// Where a shard's call writes its rows: one vector per shard, n_guides rows where the shard owns words of the genome and the
// rows are wanted.  (Made before the fan-out, on the calling thread: no allocation can fail on a shard's thread.)
template <class Row> std::vector<std::vector<Row>> shard_rows(const vsc_multi_genome *g, uint32_t n_guides, bool wanted)
{
    std::vector<std::vector<Row>> part(g->shard.size());
    for (size_t r = 0; wanted && r < part.size(); ++r)
        if (g->shard[r]) part[r].resize(n_guides);
    return part;
}

// out[i] = the sum of the shards' rows part[r][i] (a shard that owns no words of the genome has none); out == null: not wanted
template <class Row> void add_shard_rows(const vsc_multi_genome *g, const std::vector<std::vector<Row>> &part, uint32_t n_guides, Row *out)
{
    if (!out) return;
    std::fill(out, out + n_guides, Row{});
    for (size_t r = 0; r < part.size(); ++r)
        for (uint32_t i = 0; g->shard[r] && i < n_guides; ++i) add_row(out[i], part[r][i]);
}

// The excluded loci of `who` against the genome's contig table.  (The shards check them too, but a shard that owns no words
// of the genome does not search.)
int check_excluded(vsc_multi *m, const vsc_multi_genome *g, const vsc_locus *exclude, uint32_t n_guides, const std::string &who)
{
    for (uint32_t i = 0; exclude && i < n_guides; ++i)
        if ((exclude[i].contig != UINT32_MAX && exclude[i].contig >= g->table->n_contigs) || exclude[i].strand > 1)
            return mfail(m, VSC_ERR_INVALID, who + ": excluded locus outside the genome's contigs or strands");
    return VSC_OK;
}

// The timing of a call that fans out over the shards and joins their results on the host: what fan_out recorded, merge_ms = what
// followed on the first device.
void store_join_timing(vsc_multi *m, const FanOut &fo, bool used_rccl, double merge_ms = 0)
{
    vsc_multi_timing mt{};
    for (const vsc_timing &t : fo.tm) {
        mt.search_ms_max = std::max(mt.search_ms_max, t.total_ms);
        mt.hits += t.hits;
    }
    mt.search_wall_ms = fo.wall;
    mt.merge_ms = merge_ms;
    mt.total_ms = ms_between(fo.t0, clk::now());
    mt.n_devices = (uint32_t)fo.tm.size();
    mt.used_rccl = used_rccl ? 1u : 0u;
    mt.batches = 1;
    m->timing = mt;
}

// what a summary call wants from join_rows
struct RowsWanted {
    const vsc_regions *regions;  // the region-aware form: out_in beside out (null: not that form)
    const vsc_classify *cls;     // the classified form: out_votes, `out` optional, reserved fields and tree count checked (null: not that form)
    vsc_guide_summary *out, *out_in;
    vsc_guide_votes *out_votes;
    const char *who;             // the entry point, for the error texts
    const vsc_score_table *table = nullptr;    // the table form: out_table, `out` optional (null: not that form)
    vsc_guide_table_row *out_table = nullptr;
};

// vsc_multi_search_summary, _regions and _classified: every shard summarises its own windows with the single-device call of the
// form, the rows are added on the host.  null_arg: the entry point's own test of its pointers.
int join_rows(vsc_multi *m, const vsc_multi_genome *g, const uint64_t *guides, uint32_t n_guides, const vsc_search_params *params,
              const vsc_locus *exclude, bool null_arg, const RowsWanted &w)
{
    return mguarded(m, [&]() -> int {
    if (!m) return VSC_ERR_INVALID;
    m->err.clear();
    const std::string who = w.who;
    if (null_arg) return mfail(m, VSC_ERR_INVALID, who + ": null argument");
    if (w.cls && (w.cls->reserved[0] || w.cls->reserved[1])) return mfail(m, VSC_ERR_INVALID, who + ": reserved fields must be 0");
    if (w.cls && (w.cls->model->n_trees == 0 || w.cls->model->n_trees > 65535u))
        return mfail(m, VSC_ERR_INVALID, who + ": a forest of 0 trees, or of more than the 16-bit votes hold");
    const int erc = check_excluded(m, g, exclude, n_guides, who);
    if (erc != VSC_OK) return erc;
    auto part = shard_rows<vsc_guide_summary>(g, n_guides, w.out), part_in = shard_rows<vsc_guide_summary>(g, n_guides, w.regions);
    auto part_votes = shard_rows<vsc_guide_votes>(g, n_guides, w.cls);
    auto part_table = shard_rows<vsc_guide_table_row>(g, n_guides, w.table);
    FanOut fo;
    const int rc = fan_out(m, g, &fo, [&](size_t r) {
        vsc_guide_summary *rows = w.out ? part[r].data() : nullptr;
        if (w.table) return vsc_search_summary_table(m->ctx[r], g->shard[r], guides, n_guides, params, exclude, w.table, rows, part_table[r].data());
        if (w.cls) return vsc_search_summary_classified(m->ctx[r], g->shard[r], guides, n_guides, params, exclude, w.cls, rows, part_votes[r].data());
        if (w.regions) return vsc_search_summary_regions(m->ctx[r], g->shard[r], guides, n_guides, params, exclude, w.regions, rows, part_in[r].data());
        return vsc_search_summary(m->ctx[r], g->shard[r], guides, n_guides, params, exclude, rows);
    });
    if (rc != VSC_OK) return rc;
    add_shard_rows(g, part, n_guides, w.out);
    add_shard_rows(g, part_in, n_guides, w.out_in);
    add_shard_rows(g, part_votes, n_guides, w.out_votes);
    add_shard_rows(g, part_table, n_guides, w.out_table);
    store_join_timing(m, fo, m->use_rccl);
    return VSC_OK;
    });
}

// vsc_multi_search_select (filter == null) and vsc_multi_search_select_regions (`who`)
int multi_select(vsc_multi *m, const vsc_multi_genome *g, const uint64_t *guides, uint32_t n_guides, const vsc_search_params *params,
                 const vsc_select *select, const vsc_region_filter *filter, const vsc_locus *exclude, vsc_guide_summary *summary,
                 vsc_guide_summary *summary_in, vsc_hits **out, const std::string &who)
{
    return mguarded(m, [&]() -> int {
    if (!m || !out) return VSC_ERR_INVALID;
    *out = nullptr;
    m->err.clear();
    if (!g || g->multi != m || !params || !select || (n_guides && !guides))
        return mfail(m, VSC_ERR_INVALID, who + ": null argument");
    if (select->reserved[0] || select->reserved[1]) return mfail(m, VSC_ERR_INVALID, who + ": reserved fields must be 0");
    if (filter && (!filter->regions || filter->scope > VSC_REGION_DROP || filter->reserved))  // (checked here too, as the loci below)
        return mfail(m, VSC_ERR_INVALID, who + ": a filter needs regions, a scope of 0 or 1 and a reserved field of 0");
    if (!filter && summary_in) return mfail(m, VSC_ERR_INVALID, who + ": summary_in without a filter");
    const int erc = check_excluded(m, g, exclude, n_guides, who);
    if (erc != VSC_OK) return erc;
    const size_t n = m->ctx.size();
    auto part = shard_rows<vsc_guide_summary>(g, n_guides, summary), part_in = shard_rows<vsc_guide_summary>(g, n_guides, summary_in);
    auto select_on = [&](size_t r, vsc_hits **h) {
        vsc_guide_summary *rows = summary ? part[r].data() : nullptr;
        if (!filter) return vsc_search_select(m->ctx[r], g->shard[r], guides, n_guides, params, select, exclude, rows, h);
        return vsc_search_select_regions(m->ctx[r], g->shard[r], guides, n_guides, params, select, filter, exclude, rows,
                                         summary_in ? part_in[r].data() : nullptr, h);
    };
    // the rows add exactly, as in vsc_multi_search_summary
    auto add_rows = [&]() {
        add_shard_rows(g, part, n_guides, summary);
        add_shard_rows(g, part_in, n_guides, summary_in);
    };
    if (select->top_k == 0) {
        // nothing to cut: the shards' survivors are the result - through the packed exchange, they can be many
        const int rc = run_batches(m, g, guides, n_guides, params, 0, nullptr, hand_over(out), select_on);
        if (rc == VSC_OK) add_rows();
        return rc;
    }
    // every shard: select, score the survivors, records and scores to the host
    struct Cand {
        uint32_t score, strand, contig, pos, shard;
        uint64_t index;  // in the shard's records
    };
    std::vector<std::vector<vsc_hit>> rec(n);
    std::vector<std::vector<double>> mit(n);
    FanOut fo;
    const int frc = fan_out(m, g, &fo, [&](size_t r) {
        vsc_hits *h = nullptr;
        int rc = select_on(r, &h);
        if (rc != VSC_OK) return rc;
        const uint64_t c = vsc_hits_count(h);
        try {
            rec[r].resize(c);
            mit[r].resize(c);
        } catch (...) {
            m->ctx[r]->err = "out of host memory";
            rc = VSC_ERR_NOMEM;
        }
        if (rc == VSC_OK && c) rc = vsc_hits_copy(h, rec[r].data(), 0);
        if (rc == VSC_OK && c) rc = vsc_score_hits(m->ctx[r], g->shard[r], h, guides, n_guides, 0, c, mit[r].data(), nullptr, nullptr);
        vsc_hits_free(h);
        return rc;
    });
    if (frc != VSC_OK) return frc;
    // the cut: per guide the top_k of the shards' survivors by (score desc, strand, contig, pos) - (contig, pos) orders as the
    // global position does.  A shard's records are sorted by guide: one cursor per shard walks them guide by guide.
    std::vector<std::vector<char>> keep(n);
    for (size_t r = 0; r < n; ++r) keep[r].assign(rec[r].size(), 0);
    std::vector<uint64_t> at(n, 0);
    std::vector<Cand> cand;
    for (uint32_t gi = 0; gi < n_guides; ++gi) {
        cand.clear();
        for (size_t r = 0; r < n; ++r)
            for (; at[r] < rec[r].size() && rec[r][at[r]].guide == gi; ++at[r]) {
                const vsc_hit &h = rec[r][at[r]];
                cand.push_back(Cand{(uint32_t)std::nearbyint(mit[r][at[r]] * 0x1p24), VSC_HIT_STRAND(h.info), h.contig, h.pos, (uint32_t)r, at[r]});
            }
        if (cand.size() > select->top_k) {
            std::nth_element(cand.begin(), cand.begin() + select->top_k, cand.end(), [](const Cand &a, const Cand &b) {
                if (a.score != b.score) return a.score > b.score;
                if (a.strand != b.strand) return a.strand < b.strand;
                if (a.contig != b.contig) return a.contig < b.contig;
                return a.pos < b.pos;
            });
            cand.resize(select->top_k);
        }
        for (const Cand &c : cand) keep[c.shard][c.index] = 1;
    }
    std::vector<vsc_hit> all;
    std::vector<uint64_t> counts(n, 0);
    for (size_t r = 0; r < n; ++r)
        for (size_t i = 0; i < rec[r].size(); ++i)
            if (keep[r][i]) {
                all.push_back(rec[r][i]);
                counts[r]++;
            }
    const auto t_cut = clk::now();
    const int mrc = vsc_hits_merge(m->merge_ctx, all.data(), 0, counts.data(), (uint32_t)n, n_guides, out);
    if (mrc != VSC_OK) return mfail(m, mrc, std::string("merge: ") + vsc_last_error(m->merge_ctx));
    add_rows();
    store_join_timing(m, fo, m->use_rccl, ms_between(t_cut, clk::now()));
    return VSC_OK;
    });
}

}  // namespace

extern "C" {

int vsc_multi_create(const int *device_ids, int n, vsc_multi **out) { return vsc_multi_create_debug(device_ids, n, nullptr, out); }

int vsc_multi_create_debug(const int *device_ids, int n, const vsc_multi_debug_params *params, vsc_multi **out)
{
    return mguarded(nullptr, [&]() -> int {
    if (!out) return VSC_ERR_INVALID;
    *out = nullptr;
    if (!device_ids || n <= 0 || n > 64) return VSC_ERR_INVALID;
    // (held by a smart pointer until it is handed over: an exception half-way releases the contexts and streams made so far)
    std::unique_ptr<vsc_multi, int (*)(vsc_multi *)> holder(new (std::nothrow) vsc_multi(), vsc_multi_destroy);
    vsc_multi *m = holder.get();
    if (!m) return VSC_ERR_NOMEM;
    m->device.assign(device_ids, device_ids + n);
    m->ctx.assign(n, nullptr);
    m->xstream.assign(n, nullptr);
    for (auto *v : {&m->xbuf[0], &m->xbuf[1], &m->vbuf[0], &m->vbuf[1], &m->gbuf, &m->gvotes}) v->assign(n, DeviceBuf{});
    for (int i = 0; i < n; ++i) {
        const int rc = vsc_ctx_create(device_ids[i], &m->ctx[i]);
        if (rc != VSC_OK) return rc;
        if (hipSetDevice(device_ids[i]) != hipSuccess || hipStreamCreate(&m->xstream[i]) != hipSuccess) return VSC_ERR_DEVICE;
    }
    const int mrc = vsc_ctx_create(device_ids[0], &m->merge_ctx);
    if (mrc != VSC_OK) return mrc;
    // RCCL needs one communicator rank per DISTINCT device; a list with repeats (tests, rehearsals) exchanges by
    // device copies.  Hooks (varscot_hip_debug.h): rccl = 0 forces copies, 1 insists on RCCL (an error if it
    // cannot be set up).
    std::vector<int> sorted(m->device);
    std::sort(sorted.begin(), sorted.end());
    const bool distinct = std::adjacent_find(sorted.begin(), sorted.end()) == sorted.end();
    const bool forced = params && params->rccl == 1, off = params && params->rccl == 0, attempt = params && params->rccl == 2;
    if (distinct && !off && (n > 1 || forced || attempt)) {
        std::string why;
        bool ok = m->rccl.load(&why, params ? params->rccl_library : nullptr);
        if (ok) {
            m->comm.assign(n, nullptr);
            const ncclResult_t r = m->rccl.CommInitAll(m->comm.data(), n, m->device.data());
            if (r != ncclSuccess) {
                ok = false;
                why = std::string("ncclCommInitAll: ") + m->rccl.GetErrorString(r);
                m->comm.clear();
            }
        }
        if (!ok && forced) {
            std::fprintf(stderr, "vsc_multi_create: %s\n", why.c_str());
            return VSC_ERR_DEVICE;
        }
        m->use_rccl = ok;  // not forced and unavailable: peer copies carry the records instead
        if (!ok) m->err = why;  // (vsc_multi_last_error says why the copies are in use)
    } else if (forced) {
        std::fprintf(stderr, "vsc_multi_create: RCCL was asked for but needs distinct devices\n");
        return VSC_ERR_INVALID;
    }
    *out = holder.release();
    return VSC_OK;
    });
}

int vsc_multi_destroy(vsc_multi *m)
{
    if (!m) return VSC_OK;
    if (!m->comm.empty())
        for (ncclComm_t c : m->comm)
            if (c) (void)m->rccl.CommDestroy(c);
    release_buffers(m);
    if (m->merge_ctx) vsc_ctx_destroy(m->merge_ctx);
    for (size_t i = 0; i < m->ctx.size(); ++i) {
        (void)hipSetDevice(m->device[i]);
        if (i < m->xstream.size() && m->xstream[i]) (void)hipStreamDestroy(m->xstream[i]);
        if (m->ctx[i]) vsc_ctx_destroy(m->ctx[i]);
    }
    delete m;
    return VSC_OK;
}

int vsc_multi_release_scratch(vsc_multi *m)
{
    if (!m) return VSC_ERR_INVALID;
    release_buffers(m);
    if (m->merge_ctx) (void)vsc_ctx_release_scratch(m->merge_ctx);
    for (vsc_ctx *c : m->ctx)
        if (c) (void)vsc_ctx_release_scratch(c);
    return VSC_OK;
}

int vsc_multi_size(const vsc_multi *m) { return m ? (int)m->ctx.size() : 0; }
vsc_ctx *vsc_multi_ctx(vsc_multi *m, int i) { return (m && i >= 0 && i < (int)m->ctx.size()) ? m->ctx[i] : nullptr; }
vsc_ctx *vsc_multi_result_ctx(vsc_multi *m) { return m ? m->merge_ctx : nullptr; }
const char *vsc_multi_last_error(const vsc_multi *m) { return m ? m->err.c_str() : "null multi-device context"; }
int vsc_multi_uses_rccl(const vsc_multi *m) { return m && m->use_rccl; }

int vsc_multi_get_timing(const vsc_multi *m, vsc_multi_timing *out)
{
    if (!m || !out) return VSC_ERR_INVALID;
    *out = m->timing;
    return VSC_OK;
}

int vsc_multi_genome_load(vsc_multi *m, const uint32_t *hi, const uint32_t *lo, const uint32_t *nmask, uint64_t n_words,
                          const vsc_contig *contigs, uint32_t n_contigs, vsc_multi_genome **out)
{
    return mguarded(m, [&]() -> int {
    if (!m || !out) return VSC_ERR_INVALID;
    *out = nullptr;
    m->err.clear();
    if (!hi || !lo || !nmask || !contigs || n_words == 0 || n_contigs == 0)
        return mfail(m, VSC_ERR_INVALID, "vsc_multi_genome_load: null or empty argument");
    std::unique_ptr<vsc_multi_genome, int (*)(vsc_multi_genome *)> holder(new (std::nothrow) vsc_multi_genome(), vsc_multi_genome_free);
    vsc_multi_genome *g = holder.get();
    if (!g) return mfail(m, VSC_ERR_NOMEM, "vsc_multi_genome_load: out of host memory");
    g->multi = m;
    const unsigned n = (unsigned)m->ctx.size();
    g->shard.assign(n, nullptr);
    // (the genome's shards do not exist yet: which shard owns words is decided here)
    const int rc = fan_out(m, nullptr, nullptr, [&](size_t r) -> int {
        uint64_t b, e;
        shard_range(n_words, (unsigned)r, n, &b, &e);
        if (e <= b) return VSC_OK;
        const uint64_t halo_end = std::min(e + 1, n_words);  // a 22-base halo = one word
        return vsc_genome_load(m->ctx[r], hi + b, lo + b, nmask + b, b, halo_end - b, e - b, contigs, n_contigs, &g->shard[r]);
    });
    if (rc != VSC_OK) return rc;
    const int trc = genome_table_only(m->merge_ctx, contigs, n_contigs, &g->table);
    if (trc != VSC_OK) return mfail(m, trc, std::string("contig table on the first device: ") + vsc_last_error(m->merge_ctx));
    *out = holder.release();
    return VSC_OK;
    });
}

int vsc_multi_genome_free(vsc_multi_genome *g)
{
    if (!g) return VSC_OK;
    for (vsc_genome *s : g->shard)
        if (s) vsc_genome_free(s);
    if (g->table) vsc_genome_free(g->table);
    delete g;
    return VSC_OK;
}

int vsc_multi_genome_build_index(vsc_multi *m, vsc_multi_genome *g, const vsc_search_params *params)
{
    return mguarded(m, [&]() -> int {
    if (!m || !g || g->multi != m) return VSC_ERR_INVALID;
    m->err.clear();
    return fan_out(m, g, nullptr, [&](size_t r) { return vsc_genome_build_index(m->ctx[r], g->shard[r], params); });
    });
}

int vsc_multi_search(vsc_multi *m, const vsc_multi_genome *g, const uint64_t *guides, uint32_t n_guides,
                     const vsc_search_params *params, vsc_hits **out)
{
    return mguarded(m, [&]() -> int {
    if (!m || !out) return VSC_ERR_INVALID;
    *out = nullptr;
    m->err.clear();
    if (!g || g->multi != m || !params || (n_guides && !guides)) return mfail(m, VSC_ERR_INVALID, "vsc_multi_search: null argument");
    // one batch = one exchange; a read set beyond one search pass is handled inside every shard's vsc_search
    return run_batches(m, g, guides, n_guides, params, 0, nullptr, hand_over(out));
    });
}

int vsc_multi_search_summary(vsc_multi *m, const vsc_multi_genome *g, const uint64_t *guides, uint32_t n_guides,
                             const vsc_search_params *params, const vsc_locus *exclude, vsc_guide_summary *out)
{
    const bool null_arg = !g || g->multi != m || !params || (n_guides && (!guides || !out));
    return join_rows(m, g, guides, n_guides, params, exclude, null_arg, RowsWanted{nullptr, nullptr, out, nullptr, nullptr, "vsc_multi_search_summary"});
}

int vsc_multi_search_summary_classified(vsc_multi *m, const vsc_multi_genome *g, const uint64_t *guides, uint32_t n_guides,
                                        const vsc_search_params *params, const vsc_locus *exclude, const vsc_classify *cls,
                                        vsc_guide_summary *out, vsc_guide_votes *out_votes)
{
    const bool null_arg = !g || g->multi != m || !params || !cls || !cls->model || (n_guides && (!guides || !out_votes || !cls->guide_activity));
    return join_rows(m, g, guides, n_guides, params, exclude, null_arg,
                     RowsWanted{nullptr, cls, out, nullptr, out_votes, "vsc_multi_search_summary_classified"});
}

int vsc_multi_search_summary_table(vsc_multi *m, const vsc_multi_genome *g, const uint64_t *guides, uint32_t n_guides,
                                   const vsc_search_params *params, const vsc_locus *exclude, const vsc_score_table *table,
                                   vsc_guide_summary *plain, vsc_guide_table_row *out)
{
    const bool null_arg = !g || g->multi != m || !params || !table || (n_guides && (!guides || !out));
    RowsWanted w{nullptr, nullptr, plain, nullptr, nullptr, "vsc_multi_search_summary_table"};
    w.table = table;
    w.out_table = out;
    return join_rows(m, g, guides, n_guides, params, exclude, null_arg, w);
}

int vsc_multi_search_summary_regions(vsc_multi *m, const vsc_multi_genome *g, const uint64_t *guides, uint32_t n_guides,
                                     const vsc_search_params *params, const vsc_locus *exclude, const vsc_regions *regions,
                                     vsc_guide_summary *out_all, vsc_guide_summary *out_in)
{
    const bool null_arg = !regions || !g || g->multi != m || !params || (n_guides && (!guides || !out_all || !out_in));
    return join_rows(m, g, guides, n_guides, params, exclude, null_arg,
                     RowsWanted{regions, nullptr, out_all, out_in, nullptr, "vsc_multi_search_summary_regions"});
}

// Every shard enumerates the windows that start in its own words; shards ascend in position, so their arrays in shard order
// are the whole genome's result.  No record moves between devices: the arrays go to the host and are joined there.
int vsc_multi_guides_enumerate(vsc_multi *m, const vsc_multi_genome *g, const vsc_regions *regions, const vsc_enum_params *params,
                               vsc_guides **out)
{
    return mguarded(m, [&]() -> int {
    if (!m || !out) return VSC_ERR_INVALID;
    *out = nullptr;
    m->err.clear();
    if (!g || g->multi != m || !params) return mfail(m, VSC_ERR_INVALID, "vsc_multi_guides_enumerate: null argument");
    const size_t n = m->ctx.size();
    std::vector<vsc_guides *> part(n, nullptr);
    struct FreeParts {
        std::vector<vsc_guides *> &p;
        ~FreeParts()
        {
            for (vsc_guides *x : p) vsc_guides_free(x);
        }
    } free_parts{part};
    std::vector<const uint64_t *> codes(n, nullptr);
    std::vector<const vsc_locus *> loci(n, nullptr);
    FanOut fo;
    const int rc = fan_out(m, g, &fo, [&](size_t r) {  // (a small genome: not every shard owns words of it; some shard always does)
        const int erc = vsc_guides_enumerate(m->ctx[r], g->shard[r], regions, params, &part[r]);
        return erc != VSC_OK ? erc : vsc_guides_data(part[r], &codes[r], &loci[r]);
    });
    if (rc != VSC_OK) return rc;
    uint64_t total = 0;
    for (size_t r = 0; r < n; ++r) total += vsc_guides_count(part[r]);
    if (params->max_guides && total > params->max_guides)
        return mfail(m, VSC_ERR_RANGE, "vsc_multi_guides_enumerate: " + std::to_string(total) + " candidates exceed max_guides = " +
                                           std::to_string(params->max_guides));
    std::unique_ptr<vsc_guides, int (*)(vsc_guides *)> res(new vsc_guides(), vsc_guides_free);
    res->codes.reserve(total);
    res->loci.reserve(total);
    for (size_t r = 0; r < n; ++r) {
        if (!part[r]) continue;
        const uint64_t k = vsc_guides_count(part[r]);
        res->codes.insert(res->codes.end(), codes[r], codes[r] + k);
        res->loci.insert(res->loci.end(), loci[r], loci[r] + k);
    }
    res->n = total;
    res->host_valid = true;
    store_join_timing(m, fo, false);  // (an enumeration finds no hits: the shards' timings count none)
    *out = res.release();
    return VSC_OK;
    });
}

int vsc_multi_search_select(vsc_multi *m, const vsc_multi_genome *g, const uint64_t *guides, uint32_t n_guides,
                            const vsc_search_params *params, const vsc_select *select, const vsc_locus *exclude,
                            vsc_guide_summary *summary, vsc_hits **out)
{
    return multi_select(m, g, guides, n_guides, params, select, nullptr, exclude, summary, nullptr, out, "vsc_multi_search_select");
}

int vsc_multi_search_select_regions(vsc_multi *m, const vsc_multi_genome *g, const uint64_t *guides, uint32_t n_guides,
                                    const vsc_search_params *params, const vsc_select *select, const vsc_region_filter *filter,
                                    const vsc_locus *exclude, vsc_guide_summary *summary_all, vsc_guide_summary *summary_in,
                                    vsc_hits **out)
{
    return multi_select(m, g, guides, n_guides, params, select, filter, exclude, summary_all, summary_in, out,
                        "vsc_multi_search_select_regions");
}

int vsc_multi_search_stream(vsc_multi *m, const vsc_multi_genome *g, const uint64_t *guides, uint32_t n_guides,
                            const vsc_search_params *params, uint32_t batch_reads, const vsc_multi_score *score,
                            vsc_multi_batch_fn on_batch, void *user)
{
    return mguarded(m, [&]() -> int {
    if (!m) return VSC_ERR_INVALID;
    m->err.clear();
    if (!g || g->multi != m || !params || (n_guides && !guides) || !on_batch)
        return mfail(m, VSC_ERR_INVALID, "vsc_multi_search_stream: null argument");
    if (score && score->mode > VSC_MULTI_SCORE_VOTES) return mfail(m, VSC_ERR_INVALID, "vsc_multi_search_stream: unknown scoring mode");
    if (score && score->mode == VSC_MULTI_SCORE_VOTES && (!score->model || (n_guides && !score->guide_activity)))
        return mfail(m, VSC_ERR_INVALID, "vsc_multi_search_stream: the votes need a forest and the reads' activities");
    if (batch_reads == 0 || batch_reads > (uint32_t)kMaxPassReads) batch_reads = kMaxPassReads;
    return run_batches(m, g, guides, n_guides, params, batch_reads, score,
                       [&](vsc_hits *h, uint32_t first, uint32_t cnt, const uint16_t *votes_dev, bool *) { return on_batch(user, h, first, cnt, votes_dev); });
    });
}

}  // extern "C"
