// vsc_api.cpp - the C ABI of include/varscot_hip.h: context, resident genome, search orchestration
// (find -> summary / selection -> bin sort, one pass loop: run_search), the count / scan / write searches and
// enumerations (one rounds driver: run_rounds; one two-pass body: run_enumeration) and per-hit scoring.  Host C++ only; all
// device work is in the kernel files:
//   vsc_kernels.hip        scan, summary, selection, scoring, forest, merge
//   vsc_seed.hip           seed index and search
//   vsc_sort.hip           bin sort
//   vsc_enum.hip           guide discovery, labels
//   vsc_pairs.hip          guide pairs and their paired sites
//   vsc_variants.hip       the window side of the variant mergers
//   vsc_bulge.hip          bulge-tolerant search
//   vsc_pattern.hip        pattern search, pattern guide discovery
//   vsc_pattern_bulge.hip  bulges under a pattern
//   vsc_efficiency.hip     on-target efficiency of candidates
//   vsc_eff_trees.hip      ... from regression-tree ensembles
//   vsc_mh.hip             microhomology and out-of-frame scores of candidates
//   vsc_fold.hip           self-complementarity of the candidates' guide RNA: hairpin and scaffold stems
//   vsc_motif.hip          restriction sites and IUPAC motifs in the candidates' construct and genomic context
//   vsc_edit.hip           base-editor windows of candidates and their join with targets
//   vsc_prime.hip          prime-editing extensions of candidates and their join with edits
//   vsc_variation.hip      known variation under candidates: the join of their sites with variant intervals
//   vsc_pick.hip           the best K candidates per target, with spacing
// No CPU implementation of the search exists in this library: without a HIP device every compute entry point fails with
// VSC_ERR_NODEVICE / VSC_ERR_DEVICE.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "vsc_bulge.h"
#include "vsc_efficiency.h"
#include "vsc_pattern.h"
#include "vsc_pattern_enum.h"
#include "vsc_pattern_bulge.h"
#include "vsc_enum.h"
#include "vsc_internal.h"
#include "vsc_objects.h"
#include "vsc_pairs.h"
#include "vsc_pick_device.h"
#include "vsc_sites.h"
#include "vsc_bulge_table.h"
#include "vsc_table.h"
#include "vsc_varmap.h"
#include "vsc_pattern_variants.h"

using namespace vsc;

namespace {

// vsc_debug_set_host_timing(1): host-side wall times of the phases of vsc_search on stderr
struct HostTimer {
    bool on = vsc::host_timing_on();
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    void lap(const char *what)
    {
        if (!on) return;
        auto t1 = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[vsc timing] %-28s %9.3f ms\n", what, std::chrono::duration<double, std::milli>(t1 - t0).count());
        t0 = t1;
    }
};

}  // namespace

namespace vsc {
static std::atomic<int> g_host_timing{0};
bool host_timing_on() { return g_host_timing.load(std::memory_order_relaxed) != 0; }
}  // namespace vsc

namespace {

int fail(vsc_ctx *ctx, int code, const char *what, hipError_t e = hipSuccess)
{
    if (ctx) {
        char buf[512];
        if (e != hipSuccess)
            std::snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
        else
            std::snprintf(buf, sizeof buf, "%s", what);
        ctx->err = buf;
    }
    return code;
}

// fail with the caller's name in front of the text: "<who>: <what>"
int fail_in(vsc_ctx *ctx, int code, const char *who, const char *what) { return fail(ctx, code, (std::string(who) + ": " + what).c_str()); }

#define VSC_HIP(ctx, call)                                                 \
    do {                                                                   \
        hipError_t e_ = (call);                                            \
        if (e_ != hipSuccess) return fail((ctx), e_ == hipErrorOutOfMemory ? VSC_ERR_NOMEM : VSC_ERR_DEVICE, #call, e_); \
    } while (0)

// Scoring reads the genome at random hit positions: give it the interleaved copy of the planes.
hipError_t ensure_hl(vsc_ctx *ctx, const vsc_genome *genome)
{
    vsc_genome *g = const_cast<vsc_genome *>(genome);
    if (g->d_hl) return hipSuccess;
    hipError_t e = hipMalloc((void **)&g->d_hl, g->dev_words * sizeof(uint2));
    if (e != hipSuccess) return e;
    g->device_bytes += g->dev_words * sizeof(uint2);
    return launch_interleave(g->d_hi, g->d_lo, g->dev_words, g->d_hl, ctx->stream);
}

// Record storage for a result: the smallest spare buffer that fits, else a new allocation.
hipError_t take_records(vsc_ctx *ctx, vsc_hits *hits, uint64_t n)
{
    const size_t bytes = n * sizeof(vsc_hit);
    int best = -1;
    for (size_t i = 0; i < ctx->spare_records.size(); ++i)
        if (ctx->spare_records[i].cap >= bytes && (best < 0 || ctx->spare_records[i].cap < ctx->spare_records[best].cap))
            best = (int)i;
    if (best >= 0) {
        hits->storage = ctx->spare_records[best];
        ctx->spare_records.erase(ctx->spare_records.begin() + best);
    } else {
        // nothing fits: drop the spares first so that their memory can be reused
        for (auto &b : ctx->spare_records) b.release();
        ctx->spare_records.clear();
        hipError_t e = hits->storage.ensure(bytes);
        if (e != hipSuccess) return e;
    }
    hits->d_records = (vsc_hit *)hits->storage.p;
    return hipSuccess;
}

// P[Binomial(21, 3/4) <= m]: chance that a PAM-valid random window is within m mismatches of a read
double hit_probability(unsigned m)
{
    double p = 0, c = 1;
    for (unsigned j = 0; j <= m && j <= 21; ++j) {
        if (j > 0) c = c * (21 - (j - 1)) / j;
        p += c * std::pow(0.75, (double)j) * std::pow(0.25, (double)(21 - j));
    }
    return p;
}

PamMasks pam_masks(int a, int b)
{
    PamMasks m;
    m.ah = (a & 2) ? 0xFFFFFFFFu : 0u;
    m.al = (a & 1) ? 0xFFFFFFFFu : 0u;
    m.bh = (b & 2) ? 0xFFFFFFFFu : 0u;
    m.bl = (b & 1) ? 0xFFFFFFFFu : 0u;
    return m;
}

int base_code(char c)
{
    switch (c) {
    case 'A': case 'a': return 0;
    case 'C': case 'c': return 1;
    case 'G': case 'g': return 2;
    case 'T': case 't': return 3;
    default: return 4;
    }
}

void guide_planes(uint64_t g, uint32_t *h, uint32_t *l)
{
    uint32_t hh = 0, ll = 0;
    for (int i = 0; i < VSC_READ_LEN; ++i) {
        const unsigned c = (unsigned)(g >> (2 * i)) & 3u;
        hh |= (c >> 1) << i;
        ll |= (c & 1u) << i;
    }
    *h = hh;
    *l = ll;
}

}  // namespace

// No C++ exception crosses the C boundary (include/varscot_hip.h): every entry point that allocates on the host runs
// inside this guard.
template <class F> int guarded(vsc_ctx *ctx, F &&body) noexcept
{
    try {
        return body();
    } catch (const std::bad_alloc &) {
        try {
            if (ctx) ctx->err = "out of host memory";
        } catch (...) {
        }
        return VSC_ERR_NOMEM;
    } catch (...) {
        try {
            if (ctx) ctx->err = "unexpected C++ exception";
        } catch (...) {
        }
        return VSC_ERR_DEVICE;
    }
}


extern "C" {

int vsc_abi_version(void) { return VSC_ABI_VERSION; }

int vsc_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int vsc_ctx_create(int device_id, vsc_ctx **out) { return vsc_ctx_create_masked(device_id, nullptr, 0, out); }

int vsc_ctx_create_masked(int device_id, const uint32_t *cu_mask, uint32_t n_mask_words, vsc_ctx **out)
{
    if (!out) return VSC_ERR_INVALID;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return VSC_ERR_NODEVICE;
    if (device_id < 0 || device_id >= n) return VSC_ERR_INVALID;
    vsc_ctx *ctx = new (std::nothrow) vsc_ctx();
    if (!ctx) return VSC_ERR_NOMEM;
    ctx->device = device_id;
    hipDeviceProp_t prop;
    if (hipSetDevice(device_id) != hipSuccess || hipGetDeviceProperties(&prop, device_id) != hipSuccess ||
        (cu_mask && n_mask_words ? hipExtStreamCreateWithCUMask(&ctx->stream, n_mask_words, cu_mask) : hipStreamCreate(&ctx->stream)) != hipSuccess) {
        delete ctx;
        return VSC_ERR_DEVICE;
    }
    ctx->own_stream = true;
    ctx->cu_masked = cu_mask && n_mask_words;
    ctx->n_cus = prop.multiProcessorCount;
    for (auto &e : ctx->ev)
        if (hipEventCreate(&e) != hipSuccess) {
            vsc_ctx_destroy(ctx);
            return VSC_ERR_DEVICE;
        }
    *out = ctx;
    return VSC_OK;
}

int vsc_ctx_release_scratch(vsc_ctx *ctx)
{
    if (!ctx) return VSC_ERR_INVALID;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    for (DeviceBuf *b : {&ctx->counters, &ctx->guides, &ctx->score_guides, &ctx->keys_a, &ctx->keys_b, &ctx->vals_a, &ctx->vals_b, &ctx->votes_rows,
                         &ctx->score_mit, &ctx->score_flags, &ctx->score_feat, &ctx->score_sched, &ctx->sort_segs, &ctx->sort_tabs,
                         &ctx->sort_over, &ctx->seed_off, &ctx->seed_fill,
                         &ctx->seed_poff, &ctx->seed_lrest, &ctx->sum_rows, &ctx->sum_excl, &ctx->sel_hist, &ctx->sel_tabs, &ctx->sel_keys,
                         &ctx->sel_masks, &ctx->sum_rows_in, &ctx->regions_buf, &ctx->enum_tabs, &ctx->locate_buf, &ctx->locate_out,
                         &ctx->varmap_buf, &ctx->var_state, &ctx->var_excl, &ctx->var_labels, &ctx->pairs_tabs, &ctx->pairs_items,
                         &ctx->pairs_out, &ctx->bulge_tabs, &ctx->sites_tabs, &ctx->bulge_table_buf, &ctx->site_table_tabs, &ctx->site_table_scores,
                         &ctx->pattern_tabs, &ctx->pattern_table_buf, &ctx->table_buf, &ctx->table_rows, &ctx->eff_buf, &ctx->eff_trees_buf, &ctx->eff_in,
                         &ctx->eff_out, &ctx->pick_in, &ctx->pick_tabs, &ctx->pick_recs, &ctx->edit_tabs, &ctx->edit_pairs, &ctx->cds_buf, &ctx->ko_buf, &ctx->pv_shadow_buf, &ctx->pv_state, &ctx->pv_flags})
        b->release();
    ctx->table_serial = 0;
    ctx->pattern_table_serial = 0;
    ctx->bulge_table_serial = 0;
    ctx->eff_serial = 0;
    ctx->eff_trees_serial = 0;
    ctx->regions_serial = 0;
    ctx->locate_serial = 0;
    ctx->cds_serial = 0;
    ctx->ko_serial = 0;
    ctx->varmap_serial = 0;
    ctx->pv_shadow_serial = 0;
    for (auto &b : ctx->spare_records) b.release();
    ctx->spare_records.clear();
    ctx->forest.nodes.release();
    ctx->forest.ranks.release();
    ctx->forest.fingerprint = 0;
    return VSC_OK;
}

int vsc_ctx_destroy(vsc_ctx *ctx)
{
    if (!ctx) return VSC_OK;
    (void)vsc_ctx_release_scratch(ctx);
    for (auto &e : ctx->ev)
        if (e) (void)hipEventDestroy(e);
    for (auto &e : ctx->part_ev)
        if (e) (void)hipEventDestroy(e);
    if (ctx->stream_b) (void)hipStreamDestroy(ctx->stream_b);
    if (ctx->pinned) (void)hipHostFree(ctx->pinned);
    if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
    return VSC_OK;
}

int vsc_ctx_set_stream(vsc_ctx *ctx, void *hip_stream)
{
    if (!ctx) return VSC_ERR_INVALID;
    if (ctx->own_stream && ctx->stream) {
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipStreamDestroy(ctx->stream);
    }
    ctx->stream = (hipStream_t)hip_stream;
    ctx->own_stream = false;
    return VSC_OK;
}

const char *vsc_last_error(const vsc_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int vsc_ctx_set_debug_params(vsc_ctx *ctx, const vsc_debug_params *params)
{
    if (!ctx) return VSC_ERR_INVALID;
    ctx->dbg = params ? *params : default_debug_params();
    return VSC_OK;
}

int vsc_ctx_get_debug_params(const vsc_ctx *ctx, vsc_debug_params *out)
{
    if (!ctx || !out) return VSC_ERR_INVALID;
    *out = ctx->dbg;
    return VSC_OK;
}

void vsc_debug_set_host_timing(int on) { vsc::g_host_timing.store(on ? 1 : 0, std::memory_order_relaxed); }

int vsc_ctx_timing(const vsc_ctx *ctx, vsc_timing *out)
{
    if (!ctx || !out) return VSC_ERR_INVALID;
    *out = ctx->timing;
    return VSC_OK;
}

// ------------------------------------------------------------------------------------------------
int vsc_genome_load(vsc_ctx *ctx, const uint32_t *hi, const uint32_t *lo, const uint32_t *nmask, uint64_t first_word,
                    uint64_t n_words, uint64_t own_words, const vsc_contig *contigs, uint32_t n_contigs,
                    vsc_genome **out)
{
    return guarded(ctx, [&]() -> int {
    if (!ctx || !out) return VSC_ERR_INVALID;
    *out = nullptr;
    ctx->err.clear();
    if (!hi || !lo || !nmask || !contigs || n_contigs == 0 || n_words == 0 || own_words == 0 || own_words > n_words)
        return fail(ctx, VSC_ERR_INVALID, "vsc_genome_load: null or empty argument");
    if (own_words < n_words && own_words % kTileWords != 0)
        return fail(ctx, VSC_ERR_INVALID, "vsc_genome_load: a shard followed by halo words must own a multiple of 64 words");
    const uint64_t n_tiles = (own_words + kTileWords - 1) / kTileWords;
    const uint64_t dev_words = std::max<uint64_t>(n_tiles * kTileWords, n_words) + kPadWords;
    if ((first_word + dev_words) * 32 >= (1ull << 32) - 4096)
        return fail(ctx, VSC_ERR_RANGE, "vsc_genome_load: genome exceeds the 32-bit position space (4 Gbases)");
    std::vector<uint32_t> off(n_contigs), end(n_contigs);
    for (uint32_t c = 0; c < n_contigs; ++c) {
        const uint64_t e = contigs[c].offset + contigs[c].length;
        if (e >= (1ull << 32) - 4096) return fail(ctx, VSC_ERR_RANGE, "vsc_genome_load: contig table exceeds 4 Gbases");
        if (c > 0 && contigs[c].offset < contigs[c - 1].offset + contigs[c - 1].length + 1)
            return fail(ctx, VSC_ERR_INVALID, "vsc_genome_load: contigs must be ascending and separated by >= 1 N position");
        off[c] = (uint32_t)contigs[c].offset;
        end[c] = (uint32_t)e;
    }
    VSC_HIP(ctx, hipSetDevice(ctx->device));
    vsc_genome *g = new (std::nothrow) vsc_genome();
    if (!g) return fail(ctx, VSC_ERR_NOMEM, "vsc_genome_load: out of host memory");
    g->ctx = ctx;
    g->first_word = first_word;
    g->own_words = own_words;
    g->dev_words = dev_words;
    g->held_words = n_words;
    g->n_tiles = (uint32_t)n_tiles;
    g->n_contigs = n_contigs;
    g->h_contig_off = off;
    g->h_contig_end = end;
    const size_t pb = dev_words * sizeof(uint32_t), cb = (size_t)n_contigs * sizeof(uint32_t);
    hipError_t e = hipSuccess;
    auto step = [&](hipError_t r) {
        if (e == hipSuccess) e = r;
    };
    step(hipMalloc((void **)&g->d_hi, pb));
    step(hipMalloc((void **)&g->d_lo, pb));
    step(hipMalloc((void **)&g->d_nm, pb));
    step(hipMalloc((void **)&g->d_contig_off, cb));
    step(hipMalloc((void **)&g->d_contig_end, cb));
    if (e == hipSuccess) {
        step(hipMemsetAsync(g->d_hi, 0, pb, ctx->stream));
        step(hipMemsetAsync(g->d_lo, 0, pb, ctx->stream));
        step(hipMemsetAsync(g->d_nm, 0xFF, pb, ctx->stream));  // everything past the shard is N
        step(hipMemcpyAsync(g->d_hi, hi, n_words * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        step(hipMemcpyAsync(g->d_lo, lo, n_words * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        step(hipMemcpyAsync(g->d_nm, nmask, n_words * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        step(hipMemcpyAsync(g->d_contig_off, off.data(), cb, hipMemcpyHostToDevice, ctx->stream));
        step(hipMemcpyAsync(g->d_contig_end, end.data(), cb, hipMemcpyHostToDevice, ctx->stream));
        step(hipStreamSynchronize(ctx->stream));
    }
    if (e != hipSuccess) {
        vsc_genome_free(g);
        return fail(ctx, e == hipErrorOutOfMemory ? VSC_ERR_NOMEM : VSC_ERR_DEVICE, "vsc_genome_load", e);
    }
    g->device_bytes = 3 * pb + 2 * cb;
    *out = g;
    return VSC_OK;
    });
}

}  // extern "C"

int vsc::genome_table_only(vsc_ctx *ctx, const vsc_contig *contigs, uint32_t n_contigs, vsc_genome **out)
{
    if (!ctx || !out || !contigs || n_contigs == 0) return VSC_ERR_INVALID;
    *out = nullptr;
    std::vector<uint32_t> off(n_contigs), end(n_contigs);
    for (uint32_t c = 0; c < n_contigs; ++c) {
        off[c] = (uint32_t)contigs[c].offset;
        end[c] = (uint32_t)(contigs[c].offset + contigs[c].length);
    }
    VSC_HIP(ctx, hipSetDevice(ctx->device));
    vsc_genome *g = new (std::nothrow) vsc_genome();
    if (!g) return fail(ctx, VSC_ERR_NOMEM, "out of host memory");
    g->ctx = ctx;
    g->n_contigs = n_contigs;
    g->h_contig_off = off;
    g->h_contig_end = end;
    const size_t cb = (size_t)n_contigs * sizeof(uint32_t);
    hipError_t e = hipMalloc((void **)&g->d_contig_off, cb);
    if (e == hipSuccess) e = hipMalloc((void **)&g->d_contig_end, cb);
    if (e == hipSuccess) e = hipMemcpy(g->d_contig_off, off.data(), cb, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(g->d_contig_end, end.data(), cb, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        vsc_genome_free(g);
        return fail(ctx, e == hipErrorOutOfMemory ? VSC_ERR_NOMEM : VSC_ERR_DEVICE, "contig table upload", e);
    }
    g->device_bytes = 2 * cb;
    *out = g;
    return VSC_OK;
}

extern "C" {

int vsc_genome_free(vsc_genome *g)
{
    if (!g) return VSC_OK;
    if (g->ctx) (void)hipSetDevice(g->ctx->device);
    for (void *p : {(void *)g->d_hi, (void *)g->d_lo, (void *)g->d_nm, (void *)g->d_contig_off, (void *)g->d_contig_end, (void *)g->d_hl,
                    (void *)g->d_ix_chunk_tab, (void *)g->d_ix_vert, (void *)g->d_ix_sites, (void *)g->d_ix_edge})
        if (p) (void)hipFree(p);
    delete g;
    return VSC_OK;
}

uint64_t vsc_genome_device_bytes(const vsc_genome *g) { return g ? g->device_bytes + g->index_bytes : 0; }

// ------------------------------------------------------------------------------------------------
namespace {

#define VSC_TRY(call)                        \
    do {                                     \
        hipError_t e_ = (call);              \
        if (e_ != hipSuccess) return e_;     \
    } while (0)

void fill_pam(ScanArgs &a, const vsc_search_params *params)
{
    a.n_pam = 2;
    a.pam[0] = pam_masks(2, 2);  // GG  (bidir_mapping.cpp:240)
    a.pam[1] = pam_masks(2, 0);  // GA
    if (params && params->has_extra_pam) {  // :242-247
        const int p0 = base_code(params->extra_pam[0]), p1 = base_code(params->extra_pam[1]);
        // a PAM containing a non-ACGT letter can only match windows that contain N, which never
        // pass the verification (:81-82) - it adds nothing
        if (p0 < 4 && p1 < 4) a.pam[a.n_pam++] = pam_masks(p0, p1);
    }
}

// the PAM set as the seed index numbers it: class c = PAM c, (first letter << 2 | second letter) << 4 c
uint32_t pam_code_set(const ScanArgs &a)
{
    uint32_t codes = 0;
    for (uint32_t c = 0; c < a.n_pam; ++c)
        codes |= ((((a.pam[c].ah & 2u) | (a.pam[c].al & 1u)) << 2) | (a.pam[c].bh & 2u) | (a.pam[c].bl & 1u)) << (4 * c);
    return codes;
}

void fill_genome(ScanArgs &a, const vsc_ctx *ctx, const vsc_genome *genome)
{
    a.hi = genome->d_hi;
    a.lo = genome->d_lo;
    a.nm = genome->d_nm;
    a.first_pos = (uint32_t)(genome->first_word * 32);
    a.n_tiles = genome->n_tiles;
    a.contig_end = genome->d_contig_end;
    a.n_contigs = genome->n_contigs;
    a.counters = (unsigned long long *)ctx->counters.p;
}

int scan_groups(const vsc_ctx *ctx, uint32_t n_tiles)
{
    const uint32_t n_waves_max = (uint32_t)ctx->n_cus * 4 * kWavesPerGroup;
    const uint32_t n_chunks = (n_tiles + kChunkTiles - 1) / kChunkTiles;
    const uint32_t n_waves = std::max<uint32_t>(1, std::min<uint32_t>(n_waves_max, n_chunks));
    return (int)((n_waves + kWavesPerGroup - 1) / kWavesPerGroup);
}

bool index_matches(const vsc_genome *g, const vsc_search_params *p)
{
    if (!g->has_index) return false;
    const bool want = p && p->has_extra_pam && base_code(p->extra_pam[0]) < 4 && base_code(p->extra_pam[1]) < 4;
    if (want != (g->index_has_extra_pam != 0)) return false;
    return !want || (base_code(p->extra_pam[0]) == base_code(g->index_extra_pam[0]) &&
                     base_code(p->extra_pam[1]) == base_code(g->index_extra_pam[1]));
}

void free_index(vsc_genome *g)
{
    for (void **p : {(void **)&g->d_ix_chunk_tab, (void **)&g->d_ix_vert, (void **)&g->d_ix_sites, (void **)&g->d_ix_edge}) {
        if (*p) (void)hipFree(*p);
        *p = nullptr;
    }
    g->has_index = false;
    g->index_bytes = 0;
    g->ix_chunks = 0;
}

void class_counts(vsc_genome *g, const std::vector<uint32_t> &ctab);

// Builds the seed index of a resident genome: extract the PAM-valid sites of both strands, then file
// them once per segment in bucket order.  All temporaries are released before returning.
hipError_t build_index(vsc_ctx *ctx, vsc_genome *g, const vsc_search_params *params, std::string *why)
{
    free_index(g);
    hipStream_t st = ctx->stream;
    ScanArgs a{};
    fill_pam(a, params);
    fill_genome(a, ctx, g);
    const int n_groups = scan_groups(ctx, a.n_tiles);
    VSC_TRY(ctx->counters.ensure(kCounterWords * sizeof(unsigned long long)));
    a.counters = (unsigned long long *)ctx->counters.p;
    unsigned long long cnt[kCntSlots];
    VSC_TRY(hipEventRecord(ctx->ev[kEvIndexStart], st));
    // pass 1: count (capacity 0: nothing is written, the cursor still counts)
    VSC_TRY(hipMemsetAsync(ctx->counters.p, 0, sizeof cnt, st));
    VSC_TRY(launch_scan(a, n_groups, true, st));
    VSC_TRY(hipMemcpyAsync(cnt, ctx->counters.p, sizeof cnt, hipMemcpyDeviceToHost, st));
    VSC_TRY(hipStreamSynchronize(st));
    const uint64_t S = cnt[kCntHits];
    if (3 * S >= (1ull << 32) - (1u << 20)) {
        *why = "too many PAM-valid sites for 32-bit table indices";
        return hipErrorInvalidValue;
    }
    // Temporaries: the extracted sites (sx, sl, sp), sort scratch, the bucket-ordered sites as 16-byte records
    // (full planes: what the bit-slicing pass reads) and the (bucket, strand) starts; all released before returning.
    DeviceBuf sx, sl, sp, full, rec16;
    auto release = [&]() {
        for (DeviceBuf *b : {&sx, &sl, &sp, &full, &rec16}) b->release();
    };
    hipError_t e = hipSuccess;
    auto step = [&](hipError_t r) {
        if (e == hipSuccess) e = r;
    };
    HostTimer ht;
    constexpr uint32_t kKeys = 8 * kBuckets;  // (bucket, class, strand) triples: inside a bucket the sites lie class by class (four
                                              // slots, kSeedClasses in use), inside a class '+' sites precede '-' sites
    const uint32_t pam_codes = pam_code_set(a);
    // Allocations follow the phases, so that the peak stays at 84 bytes per site:
    //   extract   sx, sl, sp (12 B/site) -> rec16 (16)                          then sx, sl, sp go
    //   order     rec16 (16) + two buffers of sort records (16: the context's pooled keys_a / keys_b, which the searches use
    //             afterwards anyway) -> full (48)                               then rec16 goes
    //   compact   full (48) -> the resident 8-byte records (24) + edge bits
    //   slice     full (48) + records (24) -> bit-sliced blocks (12)            then full goes
    const size_t n4 = std::max<uint64_t>(S, 1) * sizeof(uint32_t);
    for (DeviceBuf *b : {&sx, &sl, &sp}) step(b->ensure(n4));
    step(rec16.ensure(std::max<uint64_t>(S, 1) * sizeof(uint4)));
    const size_t edge_words = (size_t)((3 * S + 31) / 32 + 1);
    ht.lap("index: count pass + buffers");
    if (e == hipSuccess && S > 0) {
        // pass 2: emit
        a.site_x = (uint32_t *)sx.p;
        a.site_l = (uint32_t *)sl.p;
        a.site_pos = (uint32_t *)sp.p;
        a.hit_cap = S;
        step(hipMemsetAsync(ctx->counters.p, 0, sizeof cnt, st));
        step(launch_scan(a, n_groups, true, st));
        step(launch_seed_pack16((const uint32_t *)sx.p, (const uint32_t *)sl.p, (const uint32_t *)sp.p, S, (uint4 *)rec16.p, st));
        step(hipStreamSynchronize(st));
    }
    for (DeviceBuf *b : {&sx, &sl, &sp}) b->release();
    ht.lap("index: emit pass");
    // ---- the three tables: the sites ordered by (bucket of the table's segment, strand) -----------------------------------
    // A counting sort in the shape of the memory system, by the bin sort's own partition kernels (vsc_sort.hip; rounds 1-3
    // used rocPRIM's radix sort here): one 8-byte record (key << 32 | site index) per site, level 1 on the top 8 of the 17
    // key bits, level 2 on the other 9 inside every level-1 bin (256 segments) - each level one read and one write of the
    // records, a tile's records of a bin leaving as one contiguous piece.  The order inside a (bucket, class, strand) group is
    // whatever the tiles' reservations give: nothing depends on it.  The level-2 histogram IS the table of group starts.
    constexpr unsigned kKeyBits = 2 * kSegBases + 3, kBits1 = 8, kBits2 = kKeyBits - kBits1;
    constexpr uint32_t kBins1 = 1u << kBits1, kBins2 = 1u << kBits2;
    step(ctx->keys_a.ensure(std::max<uint64_t>(S, 1) * sizeof(uint64_t)));
    step(ctx->keys_b.ensure(std::max<uint64_t>(S, 1) * sizeof(uint64_t)));
    step(full.ensure(std::max<uint64_t>(3 * S, 1) * sizeof(uint4)));
    step(ctx->sort_tabs.ensure(3 * (size_t)(kBins1 * kBins2) * sizeof(uint32_t)));
    const size_t seg_bytes = (kBins1 * sizeof(SortSeg) + 255) / 256 * 256;
    step(ctx->sort_segs.ensure(seg_bytes + (kBins1 + 1) * sizeof(uint32_t)));
    uint4 *const sites16 = (uint4 *)full.p;
    std::vector<uint32_t> bs(kKeys + 1, 0);  // bs[8 b + 2 class + strand] = first site of that group (over all three tables)
    ht.lap("index: order buffers");
    for (int s = 0; s < kSegments && e == hipSuccess && S > 0; ++s) {
        uint64_t *ra = (uint64_t *)ctx->keys_a.p, *rb = (uint64_t *)ctx->keys_b.p;
        SortSeg *d_segs = (SortSeg *)ctx->sort_segs.p;
        uint32_t *d_tile0 = (uint32_t *)((char *)ctx->sort_segs.p + seg_bytes);
        uint32_t *tabs = (uint32_t *)ctx->sort_tabs.p;
        step(launch_seed_keys((const uint4 *)rec16.p, S, s, pam_codes, a.n_pam, ra, st));
        // level 1: one segment, 256 bins
        std::vector<SortSeg> &segs = ctx->host_segs;
        std::vector<uint32_t> &tile0 = ctx->host_tile0;
        const uint32_t tiles = (uint32_t)((S + kSortTile - 1) / kSortTile);
        segs.assign(1, SortSeg{0, 0, 0, (uint32_t)S, 0});
        tile0.assign({0u, tiles});
        SortArgs l1{};
        l1.segs = d_segs;
        l1.seg_tile0 = d_tile0;
        l1.n_segs = 1;
        l1.n_tiles = tiles;
        l1.in = ra;
        l1.out = rb;
        l1.hist = tabs;
        l1.cursor = tabs + kBins1;
        l1.bin_start = tabs + 2 * kBins1;
        l1.bin_bits = kBits1;
        l1.bin_shift = 32 + kBits2;
        if (tiles >= 64) l1.xcd_tiles = (tiles + 7) / 8;
        step(hipMemcpyAsync(d_segs, segs.data(), sizeof(SortSeg), hipMemcpyHostToDevice, st));
        step(hipMemcpyAsync(d_tile0, tile0.data(), 2 * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        step(hipMemsetAsync(l1.hist, 0, kBins1 * sizeof(uint32_t), st));
        if (e == hipSuccess) step(launch_bin_hist(l1, st));
        if (e == hipSuccess) step(launch_bin_scan(l1, st));
        if (e == hipSuccess) step(launch_bin_partition(l1, st));
        std::vector<uint32_t> h1(kBins1);
        step(hipMemcpyAsync(h1.data(), l1.hist, kBins1 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        step(hipStreamSynchronize(st));
        if (e != hipSuccess) break;
        // level 2: every level-1 bin is a segment of its own, 512 bins each
        segs.assign(kBins1, SortSeg{});
        tile0.assign(kBins1 + 1, 0);
        uint64_t at = 0, t2 = 0;
        for (uint32_t i = 0; i < kBins1; ++i) {
            segs[i] = SortSeg{at, at, 0, h1[i], 0, i, 0};
            tile0[i] = (uint32_t)t2;
            t2 += (h1[i] + kSortTile - 1) / kSortTile;
            at += h1[i];
        }
        tile0[kBins1] = (uint32_t)t2;
        SortArgs l2{};
        l2.segs = d_segs;
        l2.seg_tile0 = d_tile0;
        l2.n_segs = kBins1;
        l2.n_tiles = (uint32_t)t2;
        l2.in = rb;
        l2.out = ra;
        l2.hist = tabs;
        l2.cursor = tabs + kBins1 * kBins2;
        l2.bin_start = tabs + 2 * kBins1 * kBins2;
        l2.bin_bits = kBits2;
        l2.bin_shift = 32;
        if (t2 >= 64) l2.xcd_tiles = (uint32_t)((t2 + 7) / 8);
        step(hipMemcpyAsync(d_segs, segs.data(), kBins1 * sizeof(SortSeg), hipMemcpyHostToDevice, st));
        step(hipMemcpyAsync(d_tile0, tile0.data(), (kBins1 + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        step(hipMemsetAsync(l2.hist, 0, (size_t)kBins1 * kBins2 * sizeof(uint32_t), st));
        if (e == hipSuccess) step(launch_bin_hist(l2, st));
        if (e == hipSuccess) step(launch_bin_scan(l2, st));
        if (e == hipSuccess) step(launch_bin_partition(l2, st));
        if (e == hipSuccess) step(launch_seed_gather16((const uint4 *)rec16.p, ra, S, sites16 + (size_t)s * S, st));
        std::vector<uint32_t> h2((size_t)kBins1 * kBins2);
        step(hipMemcpyAsync(h2.data(), l2.hist, h2.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        step(hipStreamSynchronize(st));  // (the host tables of this table's levels go out of use here)
        if (e != hipSuccess) break;
        uint64_t run = (uint64_t)s * S;  // key = level-1 bin << 9 | level-2 bin: the groups lie in key order
        for (size_t k = 0; k < h2.size(); ++k) {
            bs[(size_t)s * 8 * kBucketsPerSeg + k] = (uint32_t)run;
            run += h2[k];
        }
        if (run != (uint64_t)(s + 1) * S) {
            *why = "index build: the ordered table lost or gained sites";
            e = hipErrorUnknown;
        }
    }
    bs[kKeys] = (uint32_t)(3 * S);
    rec16.release();
    ht.lap("index: three tables ordered");
    step(hipMalloc((void **)&g->d_ix_sites, std::max<uint64_t>(3 * S, 1) * sizeof(uint2)));
    step(hipMalloc((void **)&g->d_ix_edge, edge_words * sizeof(uint32_t)));
    if (e == hipSuccess) step(hipMemsetAsync(g->d_ix_edge, 0, edge_words * sizeof(uint32_t), st));
    if (e == hipSuccess) {
        step(launch_seed_compact(sites16, std::max<uint64_t>(S, 1), 3 * S, g->d_ix_sites, g->d_ix_edge, st));
        step(hipStreamSynchronize(st));
    }
    if (e != hipSuccess) {
        release();
        free_index(g);
        return e;
    }
    ht.lap("index: site records");
    // chunks: at most kSlicedChunk sites of one bucket and class each; the sites of a chunk also exist bit-sliced, in
    // blocks of 32, from block `vfirst` on.  Word z: bucket | rank in the chunk of its first '-' site << 16 | class << 29
    // (| edge flag << 28, set on the device below)
    const uint64_t chunk_sites = kSlicedChunk;
    std::vector<uint32_t> ctab;  // {first site, site count, z, first vertical block} per chunk
    ctab.reserve(4 * (3 * S / chunk_sites + (size_t)kSeedClasses * kBuckets));
    uint64_t n_blocks = 0;
    for (uint32_t b = 0; b < (uint32_t)kBuckets; ++b) {
        for (uint32_t c = 0; c < 4; ++c) {
            const size_t k = 8 * (size_t)b + 2 * c;
            const uint64_t minus = bs[k + 1];
            for (uint64_t p = bs[k]; p < bs[k + 2]; p += chunk_sites) {
                const uint64_t count = std::min<uint64_t>(chunk_sites, bs[k + 2] - p);
                const uint64_t minus_from = minus <= p ? 0 : std::min<uint64_t>(minus - p, count);
                ctab.push_back((uint32_t)p);
                ctab.push_back((uint32_t)count);
                ctab.push_back(b | (uint32_t)(minus_from << kChunkMinusShift) | (c << kChunkClassShift));
                ctab.push_back((uint32_t)n_blocks);
                n_blocks += (count + kSlicedSites - 1) / kSlicedSites;
            }
        }
    }
    g->ix_chunks = (uint32_t)(ctab.size() / 4);
    class_counts(g, ctab);
    const size_t cb = std::max<size_t>(ctab.size(), 4) * sizeof(uint32_t);
    const size_t vb = std::max<uint64_t>(n_blocks, 1) * kVertWords * sizeof(uint32_t);
    step(hipMalloc((void **)&g->d_ix_chunk_tab, cb));
    if (e == hipSuccess && !ctab.empty())
        step(hipMemcpyAsync(g->d_ix_chunk_tab, ctab.data(), ctab.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    step(hipMalloc((void **)&g->d_ix_vert, vb));
    if (e == hipSuccess) step(launch_seed_transpose(sites16, g->d_ix_chunk_tab, g->ix_chunks, g->d_ix_vert, st));
    if (e == hipSuccess) step(launch_seed_chunk_flags(g->d_ix_chunk_tab, g->ix_chunks, g->d_ix_edge, st));
    step(hipEventRecord(ctx->ev[kEvIndexEnd], st));
    step(hipStreamSynchronize(st));
    ht.lap("index: chunk table, bit-sliced blocks");
    release();
    if (e != hipSuccess) {
        free_index(g);
        return e;
    }
    float ms = 0;
    (void)hipEventElapsedTime(&ms, ctx->ev[kEvIndexStart], ctx->ev[kEvIndexEnd]);
    g->index_ms = ms;
    g->index_sites = S;
    g->sites = S;
    g->has_index = true;
    g->index_has_extra_pam = a.n_pam > 2;
    if (a.n_pam > 2) {
        g->index_extra_pam[0] = params->extra_pam[0];
        g->index_extra_pam[1] = params->extra_pam[1];
    }
    g->ix_vert_bytes = vb;
    g->ix_edge_words = edge_words;
    g->index_bytes = 3 * S * sizeof(uint2) + edge_words * sizeof(uint32_t) + cb + vb;
    return hipSuccess;
}

// ---- seed index on disk (vsc_genome_index_save / _load) ---------------------------------------------
// One header, then the four device arrays as they lie in HBM.  The header pins what the arrays depend on: the
// library's layout constants, the PAM set and a fingerprint of the genome (size, contig table, the first plane words).
struct IndexFileHeader {
    char magic[8];  // "VSCSEED\0"
    uint32_t abi, seg_bases, sliced_chunk, sliced_sites;
    uint64_t sites;  // S
    uint64_t own_words, vert_bytes, edge_words, fingerprint;
    uint32_t chunks, n_contigs;
    uint8_t has_extra_pam;
    char extra_pam[2];
    uint8_t layout;  // kIndexLayout
    uint8_t pad[4];
};
static_assert(sizeof(IndexFileHeader) == 80, "index file header layout");
constexpr char kIndexMagic[8] = {'V', 'S', 'C', 'S', 'E', 'E', 'D', 0};
constexpr size_t kIndexIoChunk = 64u << 20;

// Every word of all three planes of the shard (a device-side reduction: under 1 ms at 3 Gbp) + the contig table
// (offsets and ends) + the shard's place in the genome.  A genome of the same size and layout that differs in one
// base, or only in what is masked as N, gets another fingerprint.
hipError_t genome_fingerprint(vsc_ctx *ctx, const vsc_genome *g, uint64_t *out)
{
    VSC_TRY(ctx->counters.ensure(kCounterWords * sizeof(unsigned long long)));
    unsigned long long *d_sum = (unsigned long long *)ctx->counters.p;
    VSC_TRY(hipMemsetAsync(d_sum, 0, sizeof *d_sum, ctx->stream));
    const uint64_t words = std::min<uint64_t>(g->own_words + 1, g->dev_words);  // own words + the halo word
    VSC_TRY(launch_plane_hash(g->d_hi, g->d_lo, g->d_nm, words, d_sum, ctx->stream));
    unsigned long long sum = 0;
    VSC_TRY(hipMemcpyAsync(&sum, d_sum, sizeof sum, hipMemcpyDeviceToHost, ctx->stream));
    std::vector<uint32_t> tab(2 * (size_t)g->n_contigs);
    if (g->n_contigs) {
        VSC_TRY(hipMemcpyAsync(tab.data(), g->d_contig_off, (size_t)g->n_contigs * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        VSC_TRY(hipMemcpyAsync(tab.data() + g->n_contigs, g->d_contig_end, (size_t)g->n_contigs * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    }
    VSC_TRY(hipStreamSynchronize(ctx->stream));
    uint64_t h = 0xcbf29ce484222325ull;  // FNV-1a over the rest
    auto eat = [&](uint64_t v) {
        for (int i = 0; i < 8; ++i) h = (h ^ ((v >> (8 * i)) & 0xFF)) * 0x100000001b3ull;
    };
    eat(sum);
    eat(g->own_words);
    eat(g->first_word);
    for (uint32_t w : tab) eat(w);
    *out = h;
    return hipSuccess;
}

// What seed_sliced_kernel reads through the chunk table must lie inside the arrays: a damaged file whose length
// happens to match its header must not become out-of-bounds device reads.
bool chunk_table_ok(const std::vector<uint32_t> &ctab, uint64_t S, uint64_t vert_bytes, std::string *why)
{
    const uint64_t n_blocks = vert_bytes / (kVertWords * sizeof(uint32_t));
    uint64_t expect_site = 0, expect_block = 0;
    uint32_t last_group = 0;  // bucket << 2 | class: the chunks lie in this order
    for (size_t c = 0; c * 4 < ctab.size(); ++c) {
        const uint64_t first = ctab[4 * c], count = ctab[4 * c + 1], vfirst = ctab[4 * c + 3];
        const uint32_t z = ctab[4 * c + 2], bucket = z & kChunkBucketMask, minus_from = (z >> kChunkMinusShift) & 0xFFFu;
        const uint32_t cls = z >> kChunkClassShift;
        const uint64_t blocks = (count + kSlicedSites - 1) / kSlicedSites;
        const char *bad = nullptr;
        if (count == 0 || count > (uint64_t)kSlicedChunk) bad = "site count";
        else if (first != expect_site || first + count > 3 * S) bad = "first site";
        else if (vfirst != expect_block || vfirst + blocks > n_blocks) bad = "first block";
        else if (bucket >= (uint32_t)kBuckets || cls >= (uint32_t)kSeedClasses || (bucket << 2 | cls) < last_group) bad = "bucket";
        else if (minus_from > count) bad = "strand boundary";
        if (bad) {
            *why = "chunk " + std::to_string(c) + ": bad " + bad;
            return false;
        }
        expect_site = first + count;
        expect_block = vfirst + blocks;
        last_group = bucket << 2 | cls;
    }
    if (expect_site != 3 * S) {
        *why = "the chunks do not cover the site table";
        return false;
    }
    return true;
}

// sites and chunks per PAM class (what the search's cost model wants to know about the index)
void class_counts(vsc_genome *g, const std::vector<uint32_t> &ctab)
{
    for (int c = 0; c < 4; ++c) g->ix_class_sites[c] = g->ix_class_chunks[c] = 0;
    for (size_t c = 0; c * 4 < ctab.size(); ++c) {
        const uint32_t cls = ctab[4 * c + 2] >> kChunkClassShift;
        g->ix_class_sites[cls] += ctab[4 * c + 1];
        g->ix_class_chunks[cls] += 1;
    }
    for (int c = 0; c < 4; ++c) g->ix_class_sites[c] /= kSegments;  // every site is filed once per table
}

struct FileCloser {
    std::FILE *f;
    ~FileCloser() { if (f) std::fclose(f); }
};

// device array <-> file, through one host buffer
hipError_t index_io(std::FILE *f, void *dev, uint64_t bytes, bool to_file, std::vector<char> &host, bool *io_ok)
{
    for (uint64_t off = 0; off < bytes; off += kIndexIoChunk) {
        const size_t n = (size_t)std::min<uint64_t>(kIndexIoChunk, bytes - off);
        if (to_file) {
            VSC_TRY(hipMemcpy(host.data(), (const char *)dev + off, n, hipMemcpyDeviceToHost));
            if (std::fwrite(host.data(), 1, n, f) != n) { *io_ok = false; return hipSuccess; }
        } else {
            if (std::fread(host.data(), 1, n, f) != n) { *io_ok = false; return hipSuccess; }
            VSC_TRY(hipMemcpy((char *)dev + off, host.data(), n, hipMemcpyHostToDevice));
        }
    }
    return hipSuccess;
}

}  // namespace

int vsc_genome_build_index(vsc_ctx *ctx, vsc_genome *genome, const vsc_search_params *params)
{
    return guarded(ctx, [&]() -> int {
    if (!ctx || !genome || genome->ctx != ctx) return VSC_ERR_INVALID;
    ctx->err.clear();
    if (index_matches(genome, params)) return VSC_OK;
    VSC_HIP(ctx, hipSetDevice(ctx->device));
    std::string why;
    hipError_t e = build_index(ctx, genome, params, &why);
    if (e != hipSuccess) {
        if (!why.empty()) return fail(ctx, VSC_ERR_RANGE, ("vsc_genome_build_index: " + why).c_str());
        return fail(ctx, e == hipErrorOutOfMemory ? VSC_ERR_NOMEM : VSC_ERR_DEVICE, "vsc_genome_build_index", e);
    }
    ctx->timing.index_ms = genome->index_ms;
    return VSC_OK;
    });
}

int vsc_genome_index_save(vsc_ctx *ctx, const vsc_genome *genome, const char *path)
{
    return guarded(ctx, [&]() -> int {
    if (!ctx || !genome || genome->ctx != ctx || !path) return VSC_ERR_INVALID;
    ctx->err.clear();
    if (!genome->has_index) return fail(ctx, VSC_ERR_INVALID, "vsc_genome_index_save: the genome has no seed index (vsc_genome_build_index)");
    VSC_HIP(ctx, hipSetDevice(ctx->device));
    IndexFileHeader h{};
    std::memcpy(h.magic, kIndexMagic, sizeof h.magic);
    h.abi = VSC_ABI_VERSION;
    h.seg_bases = kSegBases;
    h.sliced_chunk = kSlicedChunk;
    h.sliced_sites = kSlicedSites;
    h.layout = (uint8_t)kIndexLayout;
    h.sites = genome->index_sites;
    h.own_words = genome->own_words;
    h.vert_bytes = genome->ix_vert_bytes;
    h.edge_words = genome->ix_edge_words;
    h.chunks = genome->ix_chunks;
    h.n_contigs = genome->n_contigs;
    h.has_extra_pam = genome->index_has_extra_pam;
    h.extra_pam[0] = genome->index_extra_pam[0];
    h.extra_pam[1] = genome->index_extra_pam[1];
    VSC_HIP(ctx, genome_fingerprint(ctx, genome, &h.fingerprint));
    FileCloser fc{std::fopen(path, "wb")};
    if (!fc.f) return fail(ctx, VSC_ERR_INVALID, (std::string("vsc_genome_index_save: cannot write ") + path).c_str());
    bool ok = std::fwrite(&h, sizeof h, 1, fc.f) == 1;
    std::vector<char> host(kIndexIoChunk);
    const uint64_t S = genome->index_sites;
    if (ok) VSC_HIP(ctx, index_io(fc.f, genome->d_ix_sites, 3 * S * sizeof(uint2), true, host, &ok));
    if (ok) VSC_HIP(ctx, index_io(fc.f, genome->d_ix_edge, h.edge_words * sizeof(uint32_t), true, host, &ok));
    if (ok) VSC_HIP(ctx, index_io(fc.f, genome->d_ix_chunk_tab, (uint64_t)h.chunks * sizeof(uint4), true, host, &ok));
    if (ok) VSC_HIP(ctx, index_io(fc.f, genome->d_ix_vert, h.vert_bytes, true, host, &ok));
    if (ok) ok = std::fflush(fc.f) == 0;
    if (!ok) return fail(ctx, VSC_ERR_DEVICE, (std::string("vsc_genome_index_save: write to ") + path + " failed").c_str());
    return VSC_OK;
    });
}

int vsc_genome_index_load(vsc_ctx *ctx, vsc_genome *genome, const char *path)
{
    return guarded(ctx, [&]() -> int {
    if (!ctx || !genome || genome->ctx != ctx || !path) return VSC_ERR_INVALID;
    ctx->err.clear();
    VSC_HIP(ctx, hipSetDevice(ctx->device));
    const auto t0 = std::chrono::steady_clock::now();
    FileCloser fc{std::fopen(path, "rb")};
    if (!fc.f) return fail(ctx, VSC_ERR_INVALID, (std::string("vsc_genome_index_load: cannot read ") + path).c_str());
    IndexFileHeader h{};
    if (std::fread(&h, sizeof h, 1, fc.f) != 1 || std::memcmp(h.magic, kIndexMagic, sizeof h.magic) != 0)
        return fail(ctx, VSC_ERR_INVALID, (std::string("vsc_genome_index_load: ") + path + " is not a seed index file").c_str());
    if (h.abi != VSC_ABI_VERSION || h.seg_bases != (uint32_t)kSegBases || h.sliced_chunk != (uint32_t)kSlicedChunk ||
        h.sliced_sites != (uint32_t)kSlicedSites || h.layout != (uint8_t)kIndexLayout)
        return fail(ctx, VSC_ERR_INVALID, "vsc_genome_index_load: the file was written by another version of the library");
    uint64_t fp = 0;
    VSC_HIP(ctx, genome_fingerprint(ctx, genome, &fp));
    if (h.own_words != genome->own_words || h.n_contigs != genome->n_contigs || h.fingerprint != fp)
        return fail(ctx, VSC_ERR_INVALID, "vsc_genome_index_load: the file belongs to another genome");
    const uint64_t S = h.sites;
    if (3 * S >= (1ull << 32) || h.edge_words != (3 * S + 31) / 32 + 1 || h.vert_bytes % (kVertWords * sizeof(uint32_t)) != 0)
        return fail(ctx, VSC_ERR_INVALID, "vsc_genome_index_load: inconsistent header");
    {
        // the arrays the header announces must be what the file holds (a cut or padded file is refused before
        // anything is allocated)
        const long at = std::ftell(fc.f);
        const uint64_t want = (uint64_t)sizeof h + 3 * S * sizeof(uint2) + h.edge_words * sizeof(uint32_t) +
                              (uint64_t)h.chunks * sizeof(uint4) + h.vert_bytes;
        if (at < 0 || std::fseek(fc.f, 0, SEEK_END) != 0) return fail(ctx, VSC_ERR_INVALID, "vsc_genome_index_load: cannot seek in the file");
        const long size = std::ftell(fc.f);
        if (size < 0 || (uint64_t)size != want || std::fseek(fc.f, at, SEEK_SET) != 0)
            return fail(ctx, VSC_ERR_INVALID, (std::string("vsc_genome_index_load: ") + path + " is truncated or does not match its header").c_str());
    }
    free_index(genome);
    hipError_t e = hipSuccess;
    auto step = [&](hipError_t r) {
        if (e == hipSuccess) e = r;
    };
    const uint64_t sb = std::max<uint64_t>(3 * S, 1) * sizeof(uint2), eb = h.edge_words * sizeof(uint32_t);
    const uint64_t cb = std::max<uint64_t>(h.chunks, 1) * sizeof(uint4), vb = std::max<uint64_t>(h.vert_bytes, kVertWords * sizeof(uint32_t));
    step(hipMalloc((void **)&genome->d_ix_sites, sb));
    step(hipMalloc((void **)&genome->d_ix_edge, eb));
    step(hipMalloc((void **)&genome->d_ix_chunk_tab, cb));
    step(hipMalloc((void **)&genome->d_ix_vert, vb));
    bool ok = true;
    std::vector<char> host(kIndexIoChunk);
    if (e == hipSuccess) step(index_io(fc.f, genome->d_ix_sites, 3 * S * sizeof(uint2), false, host, &ok));
    if (e == hipSuccess && ok) step(index_io(fc.f, genome->d_ix_edge, eb, false, host, &ok));
    if (e == hipSuccess && ok) step(index_io(fc.f, genome->d_ix_chunk_tab, (uint64_t)h.chunks * sizeof(uint4), false, host, &ok));
    if (e == hipSuccess && ok) step(index_io(fc.f, genome->d_ix_vert, h.vert_bytes, false, host, &ok));
    if (e != hipSuccess || !ok) {
        free_index(genome);
        if (e != hipSuccess) return fail(ctx, e == hipErrorOutOfMemory ? VSC_ERR_NOMEM : VSC_ERR_DEVICE, "vsc_genome_index_load", e);
        return fail(ctx, VSC_ERR_INVALID, (std::string("vsc_genome_index_load: ") + path + " is truncated").c_str());
    }
    {
        std::vector<uint32_t> ctab((size_t)h.chunks * 4);
        if (h.chunks) VSC_HIP(ctx, hipMemcpy(ctab.data(), genome->d_ix_chunk_tab, ctab.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        std::string why;
        if (!chunk_table_ok(ctab, S, h.vert_bytes, &why)) {
            free_index(genome);
            return fail(ctx, VSC_ERR_INVALID, (std::string("vsc_genome_index_load: ") + path + " is damaged (" + why + ")").c_str());
        }
        class_counts(genome, ctab);
    }
    genome->ix_chunks = h.chunks;
    genome->ix_vert_bytes = vb;
    genome->ix_edge_words = h.edge_words;
    genome->index_sites = S;
    genome->sites = S;
    genome->has_index = true;
    genome->index_has_extra_pam = h.has_extra_pam;
    genome->index_extra_pam[0] = h.extra_pam[0];
    genome->index_extra_pam[1] = h.extra_pam[1];
    genome->index_bytes = sb + eb + cb + vb;
    genome->index_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    ctx->timing.index_ms = genome->index_ms;
    return VSC_OK;
    });
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------
// search
// ------------------------------------------------------------------------------------------------
namespace {

unsigned ceil_log2(uint64_t x)
{
    unsigned b = 0;
    while (b < 63 && (1ull << b) < x) ++b;
    return b;
}

// what one bin sort did (goes into vsc_timing)
// A search that keeps the sites' bases (vsc_search_stream_rows): every record travels with a 32-bit side word (the site's lo
// plane; parallel arrays beside the two record buffers) and the finalize kernel writes the hits' packed feature rows.
struct SortRows {
    uint32_t *side_src = nullptr;     // side words beside `src`
    DeviceBuf *side_other = nullptr;  // grows to the size of `other` (in records) x 4 bytes
    const uint2 *guides = nullptr;    // planes of the pass's reads
    uint32_t guide_first = 0;         // read index of guides[0]
    uint4 *rows = nullptr;            // row of result record i at rows + (i - rows_first)
    uint64_t rows_first = 0;
};

// Level 1 of a seed search whose records go straight to the sort (find_pass): the block fill table that says which slots
// of the search's buffer hold records, how many they are, and - a search in parts - the slot partition that has already run,
// part by part, beside the search: bin_sort then starts at the bin starts.
struct SortLevel1 {
    const uint32_t *fill = nullptr;  // SeedArgs.fill (null: unused slots hold sentinels)
    unsigned fill_shift = 0;
    uint64_t n_real = 0;             // records among the segments' slots
    bool done = false;               // the partition has run (slot mode, over one segment per part and region)
    unsigned bits = 0;               // ... on this many key bits, into slots of slot_cap records; segment i is region i
    uint64_t slot_cap = 0;
};

// The first partition level's key bits for segments of at most n_max records (0: the finalize kernel takes them as they are)
unsigned level_bits(uint64_t n_max, uint64_t sort_cap, unsigned max_bits, unsigned rem, size_t n_segs)
{
    if (n_max <= sort_cap || rem == 0) return 0;
    const uint64_t want = std::max<uint64_t>(1, sort_cap * 7 / 10);  // average bin: 70 % of what the finalize kernel holds
    unsigned bits = std::min<unsigned>({std::max(1u, ceil_log2((n_max + want - 1) / want)), max_bits, rem});
    while (bits > 1 && ((uint64_t)n_segs << bits) > (1ull << 22)) --bits;  // bounded bin tables
    return bits;
}

// the hooks' say on the sort's constants (varscot_hip_debug.h)
void sort_limits(const vsc_debug_params &dbg, uint64_t *sort_cap, unsigned *max_bits, uint64_t *slot_cap)
{
    *sort_cap = kSortCap;
    *max_bits = kSortMaxBinBits;
    if (dbg.sort_cap) *sort_cap = std::min<uint64_t>(kSortCap, std::max<uint32_t>(16, dbg.sort_cap));
    if (dbg.sort_max_bits) *max_bits = std::min<unsigned>(kSortMaxBinBits, std::max<uint32_t>(1, dbg.sort_max_bits));
    // a slot holds a quarter more than the finalize kernel orders in LDS: bins between the two go to another level
    // from their slot, bins beyond make the level fall back
    *slot_cap = dbg.sort_slot_cap ? dbg.sort_slot_cap : (*sort_cap + *sort_cap / 4 + 15) / 16 * 16;
    *slot_cap = std::max<uint64_t>(*slot_cap, 16);
}

// does the slot layout of a level (n_bins slots of slot_cap records for n_all records) fit the device beside everything else?
bool slots_fit(uint64_t n_bins, uint64_t slot_cap, uint64_t n_all, size_t other_cap, size_t side_cap, bool side)
{
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = 0;
    const uint64_t room = (uint64_t)free_b + other_cap;  // (the buffer's present allocation is given back first)
    const uint64_t slot_records = n_bins * slot_cap;
    // (a search that keeps the sites' bases has a side word beside every slot)
    const uint64_t slot_bytes = slot_records * (sizeof(uint64_t) + (side ? sizeof(uint32_t) : 0));
    return !(slot_records > 4 * n_all + (1ull << 20) || slot_bytes + (1ull << 30) > room + side_cap);
}

struct SortInfo {
    unsigned levels = 0;     // partition levels run (0: every region fitted the finalize kernel as it was)
    unsigned bin_bits = 0;   // key bits of the first partition level
    uint64_t bytes = 0;      // bytes the sort kernels moved: 8 per record read or written, 16 per result record
    unsigned slot_fallbacks = 0;  // slot-mode levels that overflowed and ran again with the histogram
};

// Orders the packed records of `segs` (each segment independently, ascending) and writes the vsc_hit
// records: hist -> scan -> partition per level, then finalize; bins too large for the finalize kernel come
// back as the segments of the next level (vsc_sort.hip).  `src` holds the segments' records, `other` is a
// buffer of the same size; `key_bits` = significant bits of record >> kRecPosShift inside a segment.
// pair_keys != null: level 0 of the streaming scan - one segment of (key, value) pairs, partitioned by region
// into `other` and packed on the way; the regions then are the segments.
// slots != null (the seed search's level 1): the first partition level runs in SLOT MODE when *slots allows it -
// no histogram pass: every bin owns a fixed slot of `other` (grown to n_bins x slot capacity through `other_buf`), the
// partition reserves room with the bin cursors alone; a bin that outgrows its slot (repeats) makes the level run again
// with the histogram and clears *slots, so that later searches of this genome and budget go the exact way at once.
hipError_t bin_sort(vsc_ctx *ctx, const vsc_genome *genome, std::vector<SortSeg> segs, uint64_t *src, uint64_t *other,
                    unsigned key_bits, unsigned pos_pad, uint32_t pos_base, vsc_hit *out, hipEvent_t ev_sorted, SortInfo *info,
                    DeviceBuf *other_buf = nullptr, bool *slots = nullptr, const SortRows *rows = nullptr, const SortLevel1 *l1 = nullptr)
{
    uint32_t *side_src = rows ? rows->side_src : nullptr, *side_other = nullptr;
    // (key_bits counts the meaningful bits: the pos_pad zero bits at the bottom of every position field are not among them)
    hipStream_t st = ctx->stream;
    unsigned rem = key_bits;  // key bits no partition level has used yet
    bool sorted_marked = false;
    // test hooks (varscot_hip_debug.h): a smaller bin capacity / fewer bits per level make the partition levels
    // and the oversize path run on inputs of a few thousand records
    const vsc_debug_params &dbg = ctx->dbg;
    uint64_t sort_cap, slot_cap;
    unsigned max_bits;
    sort_limits(dbg, &sort_cap, &max_bits, &slot_cap);
    for (unsigned level = 1; !segs.empty(); ++level) {
        if (level > 48) return hipErrorUnknown;  // cannot happen: every level consumes key bits, keys are unique
        uint64_t n_max = 0, n_all = 0;
        for (const SortSeg &s : segs) {
            n_max = std::max<uint64_t>(n_max, s.n_in);
            n_all += s.n_in;
        }
        if (n_max > sort_cap && rem == 0) return hipErrorUnknown;
        // (level 1 of a search in parts: the partition has run - on the bits chosen before the search, into the slots made then)
        bool parted = level == 1 && l1 && l1->done;
        const uint32_t *const fill = level == 1 && l1 ? l1->fill : nullptr;
        const uint64_t n_moved = fill ? l1->n_real : n_all;  // records the level's kernels move (the fill table leaves the rest out)
        const unsigned bits = parted ? l1->bits : level_bits(n_max, sort_cap, max_bits, rem, segs.size());
        if (parted) slot_cap = l1->slot_cap;
        const size_t n_segs = segs.size();
        const size_t n_bins = n_segs << bits;
        for (size_t i = 0; i < n_segs; ++i) segs[i].region = (uint32_t)i;
        bool use_slots = parted || (level == 1 && bits && slots && other_buf && (dbg.sort_optimistic == 1 || (dbg.sort_optimistic != 0 && *slots)));
        if (parted) {
            other = (uint64_t *)other_buf->p;
        } else if (level == 1 && bits && other_buf) {
            // the level's destination is sized here, once, for the layout that will be used: fixed slots (n_bins x slot
            // capacity: 1.8 - 3.6 x the records with average bins at 70 % of the finalize kernel's capacity) when they are
            // allowed and fit the device beside everything else, the compact layout otherwise
            uint64_t span = 1;
            for (const SortSeg &sg : segs) span = std::max<uint64_t>(span, sg.out_off + sg.n_in);
            const uint64_t slot_records = (uint64_t)n_bins * slot_cap;
            if (use_slots && dbg.sort_optimistic != 1 && !slots_fit(n_bins, slot_cap, n_all, other_buf->cap, rows ? rows->side_other->cap : 0, rows != nullptr)) {
                use_slots = false;
                *slots = false;  // remembered per genome and budget: later searches do not ask again
            }
            // (never less than the compact layout: a slot partition that overflows runs again the exact way, into the same buffer)
            hipError_t ge = other_buf->ensure((size_t)(use_slots ? std::max(slot_records, span) : span) * sizeof(uint64_t));
            if (ge == hipErrorOutOfMemory && use_slots) {
                (void)hipGetLastError();
                use_slots = false;
                *slots = false;
                ge = other_buf->ensure((size_t)span * sizeof(uint64_t));
            }
            if (ge != hipSuccess) return ge;
            other = (uint64_t *)other_buf->p;
            if (rows) {  // the side words' second buffer: as many words as `other` has records
                VSC_TRY(rows->side_other->ensure(other_buf->cap / sizeof(uint64_t) * sizeof(uint32_t)));
                side_other = (uint32_t *)rows->side_other->p;
            }
        }
        std::vector<uint32_t> &tile0 = ctx->host_tile0;
        tile0.assign(n_segs + 1, 0);
        uint64_t tiles = 0;
        for (size_t i = 0; i < n_segs; ++i) {
            tile0[i] = (uint32_t)tiles;
            tiles += (segs[i].n_in + kSortTile - 1) / kSortTile;
        }
        if (tiles >= (1ull << 31)) return hipErrorInvalidValue;
        tile0[n_segs] = (uint32_t)tiles;
        const size_t seg_bytes = (n_segs * sizeof(SortSeg) + 255) / 256 * 256;
        VSC_TRY(ctx->sort_segs.ensure(seg_bytes + tile0.size() * sizeof(uint32_t)));
        SortSeg *d_segs = (SortSeg *)ctx->sort_segs.p;
        uint32_t *d_tile0 = (uint32_t *)((char *)ctx->sort_segs.p + seg_bytes);
        ctx->host_segs = segs;  // (the copy the asynchronous upload reads from)
        VSC_TRY(hipMemcpyAsync(d_segs, ctx->host_segs.data(), n_segs * sizeof(SortSeg), hipMemcpyHostToDevice, st));
        VSC_TRY(hipMemcpyAsync(d_tile0, tile0.data(), tile0.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        VSC_TRY(ctx->sort_over.ensure(256 + n_bins * sizeof(SortSeg)));
        uint32_t *d_n_over = (uint32_t *)ctx->sort_over.p;  // [0] listed bins, [1] the finalize kernel's bin cursor, [2] slot overflow
        if (bits) VSC_TRY(ctx->sort_tabs.ensure(3 * n_bins * sizeof(uint32_t)));
        uint32_t flags[3] = {0, 0, 0};
        for (;;) {  // once; twice when the slot partition overflowed
            if (dbg.sort_debug)
                std::fprintf(stderr, "[vsc sort] level %u: %zu segments, %llu records, largest %llu, %u bits (of %u left), cap %llu%s\n", level,
                             n_segs, (unsigned long long)n_all, (unsigned long long)n_max, bits, rem, (unsigned long long)sort_cap,
                             use_slots ? ", slot mode" : "");
            // (parted: word 2, the partition's overflow flag, was cleared before the first part and may be raised by now)
            VSC_TRY(hipMemsetAsync(d_n_over, 0, (parted ? 2 : 3) * sizeof(uint32_t), st));
            FinArgs f{};
            f.segs = d_segs;
            f.n_segs = (uint32_t)n_segs;
            f.src = src;
            f.side_src = side_src;
            if (rows) {
                f.guides = rows->guides;
                f.guide_first = rows->guide_first;
                f.rows = rows->rows;
                f.rows_first = rows->rows_first;
            }
            if (bits) {
                SortArgs a{};
                a.segs = d_segs;
                a.seg_tile0 = d_tile0;
                a.n_segs = (uint32_t)n_segs;
                a.n_tiles = (uint32_t)tiles;
                a.in = src;
                a.out = other;
                a.side_in = rows ? side_src : nullptr;
                a.side_out = rows ? side_other : nullptr;
                a.hist = (uint32_t *)ctx->sort_tabs.p;
                a.cursor = a.hist + n_bins;
                a.bin_start = a.cursor + n_bins;
                a.bin_bits = bits;
                a.bin_shift = kRecPosShift + pos_pad + rem - bits;
                a.fill = fill;
                a.fill_shift = fill ? l1->fill_shift : 0;
                if (dbg.sort_xcd != 0 && tiles >= 64) a.xcd_tiles = (uint32_t)((tiles + 7) / 8);
                if (use_slots) {
                    // partition first (cursors from zero), then the bin starts of the RESULT from the cursors
                    a.hist = a.cursor;
                    a.slot_cap = (uint32_t)slot_cap;
                    a.overflow = d_n_over + 2;
                    if (!parted) {
                        VSC_TRY(hipMemsetAsync(a.cursor, 0, n_bins * sizeof(uint32_t), st));
                        VSC_TRY(launch_bin_partition(a, st));
                    }
                    VSC_TRY(launch_bin_scan(a, st));
                } else {
                    VSC_TRY(hipMemsetAsync(a.hist, 0, n_bins * sizeof(uint32_t), st));
                    VSC_TRY(launch_bin_hist(a, st));
                    VSC_TRY(launch_bin_scan(a, st));
                    if (dbg.sort_debug >= 2 && !fill) {
                        // recount every bin on the host and compare with the device histogram
                        std::vector<uint32_t> h(n_bins);
                        VSC_TRY(hipMemcpyAsync(h.data(), a.hist, n_bins * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
                        VSC_TRY(hipStreamSynchronize(st));
                        for (size_t i = 0; i < n_segs; ++i) {
                            std::vector<uint64_t> recs(segs[i].n_in);
                            VSC_TRY(hipMemcpy(recs.data(), src + segs[i].in_off, recs.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
                            std::vector<uint32_t> want((size_t)1 << bits, 0);
                            for (uint64_t r : recs) {
                                if (r >> 63) continue;
                                want[(r >> a.bin_shift) & (((uint64_t)1 << bits) - 1)]++;
                            }
                            for (size_t b = 0; b < want.size(); ++b)
                                if (want[b] != h[(i << bits) + b])
                                    std::fprintf(stderr, "[vsc sort]   seg %zu (in_off %llu n %u) bin %zu: device %u host %u\n", i,
                                                 (unsigned long long)segs[i].in_off, segs[i].n_in, b, h[(i << bits) + b], want[b]);
                        }
                    }
                    VSC_TRY(launch_bin_partition(a, st));
                }
                f.src = other;
                f.side_src = side_other;
                f.hist = a.hist;
                f.bin_start = a.bin_start;
                f.bin_bits = bits;
                f.slot_cap = a.slot_cap;
                f.overflow = a.overflow;
            } else if (fill) {
                // no partition: the finalize kernel reads the search's buffer, whose unused slots get their sentinels now
                VSC_TRY(launch_fill_holes(d_segs, (uint32_t)n_segs, src, fill, l1->fill_shift, st));
            }
            if (!sorted_marked && ev_sorted) {
                VSC_TRY(hipEventRecord(ev_sorted, st));
                sorted_marked = true;
            }
            const unsigned rem_after = rem - bits;
            f.sub_bits = std::min<unsigned>(rows ? kSortSubBitsRows : kSortSubBits, rem_after);
            f.sub_shift = kRecPosShift + pos_pad + rem_after - f.sub_bits;
            f.pos_pad = pos_pad;
            f.pos_base = pos_base;
            f.low_bits = rem_after - f.sub_bits;
            f.over = (SortSeg *)((char *)ctx->sort_over.p + 256);
            f.over_cap = (uint32_t)std::min<size_t>(n_bins, 0xFFFFFFFFu);
            f.n_over = d_n_over;
            f.cursor = d_n_over + 1;
            f.cap = (uint32_t)sort_cap;
            f.contig_off = genome->d_contig_off;
            f.n_contigs = genome->n_contigs;
            f.out = out;
            VSC_TRY(launch_bin_finalize(f, 2 * ctx->n_cus, st));  // two workgroups fit a CU (LDS)
            if (bits) {
                VSC_TRY(hipMemcpyAsync(flags, d_n_over, sizeof flags, hipMemcpyDeviceToHost, st));
                VSC_TRY(hipStreamSynchronize(st));
                if (use_slots && flags[2]) {
                    // a bin outgrew its slot: the source is untouched, nothing was finalized (the finalize kernel left at
                    // once) - the same level again, exactly.  What the failed attempt moved: the partition's read + write
                    use_slots = false;
                    parted = false;
                    *slots = false;
                    if (info) {
                        info->slot_fallbacks++;
                        info->bytes += 16 * n_moved;
                    }
                    continue;
                }
            }
            if (info && bits) {
                if (info->levels == 0) info->bin_bits = bits;
                info->levels++;
                info->bytes += (use_slots ? 16 : 24) * n_moved;  // (histogram read,) partition read + write
            }
            if (info) info->bytes += 24 * n_moved;  // finalize: 8-byte read, 16-byte write
            if (info && rows) info->bytes += (bits ? 8 : 0) * n_all + (4 + 12 + 64) * n_all;  // side words moved, read (twice: + the records again), rows written
            break;
        }
        if (!bits) break;
        rem -= bits;
        const uint32_t n_over = flags[0];
        if (n_over == 0) break;
        segs.resize(n_over);
        VSC_TRY(hipMemcpyAsync(segs.data(), (char *)ctx->sort_over.p + 256, (size_t)n_over * sizeof(SortSeg), hipMemcpyDeviceToHost, st));
        VSC_TRY(hipStreamSynchronize(st));
        std::swap(src, other);  // the listed bins are spans of the buffer this level wrote
        std::swap(side_src, side_other);
        if (rows && !side_other) {  // (level 1 did not partition: the first buffer's sibling has no twin yet)
            uint64_t span = 1;
            for (const SortSeg &sg : segs) span = std::max<uint64_t>(span, sg.out_off + sg.n_in);
            VSC_TRY(rows->side_other->ensure(span * sizeof(uint32_t)));
            side_other = (uint32_t *)rows->side_other->p;
        }
    }
    return hipSuccess;
}

// Room for `n` more records behind the `used` records a result already holds (multi-pass searches grow
// their result; `projected` = expected final size, allocated at once when the buffer has to grow).
hipError_t result_room(vsc_ctx *ctx, vsc_hits *hits, uint64_t used, uint64_t n, uint64_t projected)
{
    const uint64_t need = used + n;
    if (hits->storage.p && hits->storage.cap >= need * sizeof(vsc_hit)) return hipSuccess;
    if (used == 0) {
        if (hits->storage.p) {
            ctx->spare_records.push_back(hits->storage);
            hits->storage = DeviceBuf{};
        }
        VSC_TRY(take_records(ctx, hits, std::max(need, projected)));
        return hipSuccess;
    }
    DeviceBuf bigger;
    VSC_TRY(bigger.ensure(std::max(need, projected) * sizeof(vsc_hit)));
    hipError_t e = hipMemcpyAsync(bigger.p, hits->storage.p, used * sizeof(vsc_hit), hipMemcpyDeviceToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        bigger.release();
        return e;
    }
    hits->storage.release();
    hits->storage = bigger;
    hits->d_records = (vsc_hit *)bigger.p;
    return hipSuccess;
}

// What a pass's search found, its records final: a sink's input.  The records lie in ctx->keys_a (SCAN: values in ctx->vals_a).
struct PassFound {
    HostTimer ht;  // laps from the start of the pass; the sink goes on with them
    int algo = 0, n_parts = 0;             // n_parts: output regions of kRegionReads reads
    uint32_t max_mm = 0, guide_base = 0;  // guide_base: read index of the pass's first read
    uint64_t cap = 0, n = 0;               // records the search's buffers hold; hits
    // SEED: one segment per region that holds records (sentinels included); SCAN: the one segment of (key, value) pairs,
    // before the level-0 partition by region.  final_off counts from the pass's first hit.
    std::vector<SortSeg> segs;
    unsigned key_bits = 0, pos_pad = 0;  // bin_sort's key bits; the records' position encoding (with pos_base)
    uint32_t pos_base = 0;
    bool bases = false;  // SEED: every record's site lo plane lies beside it in ctx->vals_a (feature rows wanted)
    bool selected = false;  // select_pass has run: n, segs, cap describe the survivors, packed records at the start of ctx->keys_a
    // host staging of the sinks, uploaded with hipMemcpyAsync: it lives here because the pass outlives every such copy (the
    // pass ends with a synchronise) - select_pass's offsets, written once behind a synchronise of its own, and sink_input's
    // tables, written once per pass
    std::vector<uint64_t> sel_off;
    std::vector<SumSeg> sink_segs;
    std::vector<uint32_t> sink_tile0;
    SinkInput sink{};         // what sink_input staged (recs null: nothing yet)
    bool classified = false;  // classify_pass's kernel has run between kEvClassStart and kEvClassEnd
    SortLevel1 l1;            // SEED, records for the sort alone: the block fill table; a search in parts: its level-1 partition
};

// words within k substitutions of a 7-base segment (k < 0: none)
uint32_t neighbours(int k) { return k < 0 ? 0u : (k == 0 ? 1u : (k == 1 ? 22u : 211u)); }

// The cut of the pigeonhole (SeedPlan, vsc_internal.h): segment 0 within k0 substitutions, segment 1 within k1, segment 2
// within what the site's PAM class leaves of the limit - k0 - k1 - 2.  Hook seed_tight = 0: floor(m / 3) everywhere (the
// round-3 cut); 1 + k0 + 3 k1: that cut, if it is a valid one.  Host arithmetic only.  *k2_max: segment 2's largest threshold.
SeedPlan seed_cut(const vsc_genome *genome, const uint32_t *gp, uint32_t n_guides, uint32_t m, int n_cus, const vsc_debug_params &dbg,
                  int *k2_max)
{
    SeedPlan plan{};
    plan.max_mm = m;
    ScanArgs pa{};
    vsc_search_params ip{};
    ip.has_extra_pam = genome->index_has_extra_pam;
    ip.extra_pam[0] = genome->index_extra_pam[0];
    ip.extra_pam[1] = genome->index_extra_pam[1];
    fill_pam(pa, &ip);  // the classes of the index, in the order build_index gave them
    plan.n_pam = pa.n_pam;
    plan.pam_codes = pam_code_set(pa);
    plan.tight = dbg.seed_tight != 0;
    if (!plan.tight) {
        plan.k0 = plan.k1 = m / kSegments;
        *k2_max = (int)plan.k0;
    } else {
        // reads per (class, what the class leaves them for positions 0..20)
        uint32_t left_reads[kSeedClasses][VSC_MAX_MISMATCHES + 1] = {};
        int left_max = -1;
        for (uint32_t i = 0; i < n_guides; ++i) {
            const uint32_t x = gp[2 * (size_t)i], l = gp[2 * (size_t)i + 1];
            const uint32_t mine = (((x >> 21) & 1u) << 3) | (((l >> 21) & 1u) << 2) | (((x >> 22) & 1u) << 1) | ((l >> 22) & 1u);
            for (uint32_t c = 0; c < plan.n_pam; ++c) {
                const uint32_t diff = mine ^ ((plan.pam_codes >> (4 * c)) & 15u);
                const uint32_t spent = ((diff & 12u) ? 1u : 0u) + ((diff & 3u) ? 1u : 0u);
                if (spent > m) continue;
                left_reads[c][m - spent]++;
                left_max = std::max(left_max, (int)(m - spent));
            }
        }
        // Every (k0, k1) in 0..2 that keeps the third threshold within two substitutions is a valid cut; they differ in what
        // they cost.  Fewer buckets per read = fewer comparisons (what a dense search is bound by: c3), but a table whose
        // lists are short still has nearly all of its chunks loaded for a read or two each (what a sparse search is bound by:
        // at 1 000 reads and m = 6 the cut (2, 2, 0) compares 2.6 x the pairs of (1, 1, 2) and loads 14 % fewer blocks).
        // cost = max(block bytes at 4.2 TB/s, chunk visits x 215 SIMD-cycles over all SIMDs at 2 GHz)
        double cost[9];  // [k0 + 3 k1]; < 0: not a valid cut
        double chunks_all = 0, sites_all = 0;
        uint64_t reads_any = 0;
        for (uint32_t c = 0; c < plan.n_pam; ++c) {
            chunks_all += (double)genome->ix_class_chunks[c] / kSegments;
            sites_all += (double)genome->ix_class_sites[c];
            uint64_t reads_c = 0;
            for (int left = 0; left <= (int)m; ++left) reads_c += left_reads[c][left];
            reads_any = std::max(reads_any, reads_c);
        }
        const double block_bytes = (double)kVertWords * 4 / kSlicedSites;  // per site
        for (int cut = 0; cut < 9; ++cut) {
            const int k0 = cut % 3, k1 = cut / 3;
            cost[cut] = -1;
            if (left_max - k0 - k1 - 2 > 2) continue;
            double bytes = 0, visits = 0;
            for (uint32_t c = 0; c < plan.n_pam; ++c) {
                double e2 = 0;  // entries of class c's lists of segment 2
                for (int left = 0; left <= (int)m; ++left) e2 += (double)left_reads[c][left] * neighbours(left - k0 - k1 - 2);
                const double per_list = e2 / kBucketsPerSeg;
                bytes += (1.0 - std::exp(-per_list)) * (double)genome->ix_class_sites[c] * block_bytes;
                visits += per_list * (double)genome->ix_class_chunks[c] / kSegments;
            }
            for (int k : {k0, k1}) {  // segments 0 and 1: one list per bucket for all classes
                const double per_list = (double)reads_any * neighbours(k) / kBucketsPerSeg;
                bytes += (1.0 - std::exp(-per_list)) * sites_all * block_bytes;
                visits += per_list * chunks_all;
            }
            cost[cut] = std::max(bytes / 4.2e12, visits * 215.0 / ((double)n_cus * 4 * 2.0e9));
        }
        int best = -1;
        for (int cut = 0; cut < 9; ++cut)
            if (cost[cut] >= 0 && (best < 0 || cost[cut] < cost[best])) best = cut;
        const int forced = dbg.seed_tight >= 1 ? dbg.seed_tight - 1 : -1;  // hook: 1 + k0 + 3 k1
        if (forced >= 0 && forced < 9 && cost[forced] >= 0) best = forced;
        if (best < 0) best = 4 * (int)(m ? (m - 1) / kSegments : 0u);  // (no read can reach any class: nothing to search)
        plan.k0 = (uint32_t)(best % 3);
        plan.k1 = (uint32_t)(best / 3);
        *k2_max = std::min<int>(2, (int)m - (int)plan.k0 - (int)plan.k1 - 2);
    }
    plan.n_nbr = neighbours(std::max<int>(std::max<int>((int)plan.k0, (int)plan.k1), *k2_max));
    return plan;
}

// The seed search's plan of a pass: the cut, the per-bucket read lists (a counting sort of the reads' segment neighbourhoods
// over the buckets, enqueued here) and the sliced kernel's launch, which fills sa but for its record buffers.
hipError_t seed_plan(vsc_ctx *ctx, const vsc_genome *genome, const uint32_t *gp, uint32_t n_guides, const PassFound &f, SeedArgs &sa,
                     int *n_groups, bool *shared)
{
    int k2_max = 0;
    const SeedPlan plan = seed_cut(genome, gp, n_guides, f.max_mm, ctx->n_cus, ctx->dbg, &k2_max);
    // entries: one per (read, neighbour within the threshold) of segments 0 and 1, one per class and neighbour of segment 2
    const uint64_t n_pairs = (uint64_t)n_guides * (neighbours((int)plan.k0) + neighbours((int)plan.k1) + plan.n_pam * neighbours(k2_max));
    const uint64_t list_cap = n_pairs + (uint64_t)kLists * (kGuideUnroll - 1) + 2 * kGuideUnroll;
    VSC_TRY(ctx->seed_off.ensure((kLists + 1) * sizeof(uint32_t)));
    VSC_TRY(ctx->seed_poff.ensure((kLists + 1) * sizeof(uint32_t)));
    VSC_TRY(ctx->seed_lrest.ensure(list_cap * sizeof(uint2)));
    VSC_TRY(hipMemsetAsync(ctx->seed_lrest.p, 0xFF, list_cap * sizeof(uint2), ctx->stream));  // padding: y = ~0, skipped
    VSC_TRY(launch_seed_lists((const uint2 *)ctx->guides.p, n_guides, plan, (uint32_t *)ctx->seed_off.p, (uint32_t *)ctx->seed_poff.p,
                              (uint2 *)ctx->seed_lrest.p, ctx->stream));
    VSC_TRY(hipEventRecord(ctx->ev[kEvPrepEnd], ctx->stream));
    sa.chunk_tab = genome->d_ix_chunk_tab;
    sa.n_chunks = genome->ix_chunks;
    sa.vert = genome->d_ix_vert;
    sa.list_rest = (const uint2 *)ctx->seed_lrest.p;
    sa.sites = genome->d_ix_sites;
    sa.edge_bits = genome->d_ix_edge;
    sa.guides = (const uint2 *)ctx->guides.p;
    sa.poff = (const uint32_t *)ctx->seed_poff.p;
    sa.max_mm = f.max_mm;
    sa.k_half = f.max_mm / 2;
    sa.k_seg0 = plan.k0;
    sa.k_seg1 = plan.k1;
    sa.contig_end = genome->d_contig_end;
    sa.n_contigs = genome->n_contigs;
    sa.counters = (unsigned long long *)ctx->counters.p;
    sa.n_parts = (uint32_t)f.n_parts;
    uint32_t groups_per_cu = kSlicedWavesPerSimd;  // resident groups (of four waves) per CU: registers / LDS of the kernel
    if (ctx->dbg.seed_groups_per_cu) groups_per_cu = ctx->dbg.seed_groups_per_cu;
    // dense searches (c3: 129 reads per bucket) share a chunk between the four waves of a workgroup, sparse ones
    // (c2: 13) keep a chunk per wave - see seed_sliced_kernel.  Measured at <= 8 mismatches (tools/
    // experiments.sh shared-threshold): 51 reads per bucket 12.1 vs 11.4 ms, 77: 15.9 vs 16.0, 103: 19.9 vs 20.7
    // (reads per list of segments 0 and 1 - and of segment 2 wherever it is searched as widely)
    *shared = (uint64_t)n_guides * neighbours((int)std::max(plan.k0, plan.k1)) / kBucketsPerSeg >= 72;
    if (ctx->dbg.seed_shared >= 0) *shared = ctx->dbg.seed_shared == 1;
    const uint32_t n_grabs = (sa.n_chunks + kSlicedGrab - 1) / kSlicedGrab;
    const uint32_t n_waves_max = (uint32_t)ctx->n_cus * groups_per_cu * kWavesPerGroup;
    const uint32_t n_waves = std::max<uint32_t>(1, std::min<uint32_t>(n_waves_max, *shared ? n_grabs * kWavesPerGroup : n_grabs));
    *n_groups = (int)((n_waves + kWavesPerGroup - 1) / kWavesPerGroup);
    // block of records a wave reserves per atomic and region (a power of two, 64 .. 1024): large when many hits
    // are expected, small otherwise (the unused tail of every wave's last block is written as sentinels
    // and read by the sort)
    // with chunk sharing the four waves of a workgroup also share their open output blocks: a quarter of the open
    // lines and of the padding, so the blocks can be eight times as large (c3: per-wave blocks of 128 records 40.6 ms
    // per step, group blocks of 512 39.3, of 1 024 39.0 - tools/experiments.sh group-out; hook seed_group_out = 0 switches it off)
    sa.group_out = *shared && ctx->dbg.seed_group_out != 0 ? 1u : 0u;
    const uint32_t owners = sa.group_out ? (uint32_t)*n_groups : (uint32_t)*n_groups * kWavesPerGroup;  // open blocks per region
    const uint64_t per_wave = f.cap / ((uint64_t)owners * 8 * f.n_parts);
    uint32_t want_reserve = (uint32_t)std::min<uint64_t>(f.n_parts > 8 ? (sa.group_out ? 1024 : 128) : 1024, std::max<uint64_t>(kWave, per_wave));
    if (ctx->dbg.seed_reserve) want_reserve = std::min<uint32_t>(1024, std::max<uint32_t>(kWave, ctx->dbg.seed_reserve));
    sa.reserve_log2 = 6;
    while ((2u << sa.reserve_log2) <= want_reserve) ++sa.reserve_log2;
    sa.reserve = 1u << sa.reserve_log2;
    sa.pos_pad = f.pos_pad;
    sa.pos_base = f.pos_base;
    // a region gets its share of the expected hits + 15 % (read ranges differ) + the open blocks
    uint64_t part_cap = f.cap / f.n_parts + f.cap / f.n_parts / 7 + 4096;
    part_cap = std::max<uint64_t>(part_cap, (uint64_t)(1.2 * genome->seen_rate[f.max_mm] * std::min<uint32_t>(n_guides, kRegionReads)) + 4096);
    sa.part_cap = part_cap + (uint64_t)owners * sa.reserve;
    return hipSuccess;
}

// ---- a seed search in parts -------------------------------------------------------------------------------------------------
// In slot mode the level-1 partition appends a tile's records to their bins through the bin cursors: it needs no histogram and
// no total, so it can start on the records of the chunks searched so far.  The chunk range is cut into K launches; the
// partition of part i runs on the context's second stream beside part i + 1, which leaves it room on every CU (three search
// workgroups instead of six: registers and LDS then hold one partition workgroup as well).  Only the bin starts and the last
// stage wait for all records (bin_sort, SortLevel1.done).
constexpr uint32_t kSeedPartsDefault = 1;       // launches of a search that qualifies (hook seed_parts = 0)
constexpr uint32_t kSeedPartsMax = 64;
// search workgroups per CU beside a partition.  Per SIMD the search's waves take 80 registers each, a partition workgroup's
// two waves 104 each (92 + 5 accumulation registers, allocated in eights): 4 x 80 + 208 = 528 of 512 - with four search
// workgroups no partition workgroup ever became resident (kernel trace: the first part's partition ended after the search) -,
// 3 x 80 + 208 = 448; LDS 3 x 20 992 + 74 752 of 163 840 bytes.
constexpr uint32_t kSeedPartGroupsPerCu = 3;
// A part pays a launch tail of the search, a partition launch and an event round trip through the host - some tens of
// microseconds - to hide its partition: 2^27 records are 0.4 ms of partition at 4.85 TB/s, ten times that.
constexpr uint64_t kSeedPartMinRecords = 1ull << 27;

// How many launches the pass's search is cut into, with the level-1 layout (l1.bits, l1.slot_cap) its partitions will use:
// chosen before the search, from what the last search of this genome and budget produced.  1: one launch, the sort as ever.
// Always 1: per-wave chunks (sparse searches), a context bound to a set of CUs, a genome whose bins have outgrown their slots
// at this budget (or the hook that forbids slots), slots that do not fit the device, and - unless the hook forces parts - a
// pass that needs no partition level or expects fewer than kSeedPartMinRecords records per part.
uint32_t plan_parts(vsc_ctx *ctx, const vsc_genome *genome, const PassFound &f, const SeedArgs &sa, uint32_t n_guides, bool shared, SortLevel1 &l1)
{
    const vsc_debug_params &dbg = ctx->dbg;
    uint32_t want = dbg.seed_parts ? dbg.seed_parts : kSeedPartsDefault;
    if (want <= 1 || !shared || ctx->cu_masked || dbg.sort_optimistic == 0 || !genome->sort_slots_ok[f.max_mm]) return 1;
    const double rate = genome->seen_rate[f.max_mm];  // records per read of the fullest region
    const uint64_t n_max = (uint64_t)(rate * std::min<uint32_t>(n_guides, kRegionReads)), n_all = (uint64_t)(rate * n_guides);
    want = std::min<uint32_t>({want, std::max<uint32_t>(1, sa.n_chunks), kSeedPartsMax});
    if (!dbg.seed_parts && n_all < (uint64_t)want * kSeedPartMinRecords) return 1;
    uint64_t sort_cap, slot_cap;
    unsigned max_bits;
    sort_limits(dbg, &sort_cap, &max_bits, &slot_cap);
    unsigned bits = level_bits(n_max, sort_cap, max_bits, f.key_bits, (size_t)f.n_parts);
    if (bits == 0) {
        if (!dbg.seed_parts) return 1;
        bits = 1;  // (forced: a partition level the records would not need)
    }
    if (dbg.sort_optimistic != 1 && !slots_fit((uint64_t)f.n_parts << bits, slot_cap, std::max<uint64_t>(n_all, 1), ctx->keys_b.cap, 0, false)) return 1;
    l1.bits = bits;
    l1.slot_cap = slot_cap;
    return want;
}

size_t round256(size_t n) { return (n + 255) / 256 * 256; }

// The search of a pass in K parts with their level-1 partitions (above).  Stream A = ctx->stream: the parts back to back, after
// each a copy of the counters to pinned memory and an event.  The host waits for event i while part i + 1 is queued, cuts the
// records of part i - per region [cursor after part i - 1, cursor after part i) - into segments and launches their partition
// on stream B; A waits for B at the end.  Ordering is by events alone.  cnt: the counters after the last part; l1.done unless
// records were lost (the caller runs the pass again, in one launch).
hipError_t search_in_parts(vsc_ctx *ctx, PassFound &f, const SeedArgs &all, uint32_t K, bool shared, unsigned long long *cnt, size_t cnt_bytes,
                           uint32_t *list_total, float *scan_ms)
{
    const hipStream_t A = ctx->stream;
    SeedArgs sa = all;
    const uint32_t R = (uint32_t)f.n_parts;
    const size_t cnt_at = 0, segs_at = round256(cnt_bytes), tile_at = segs_at + round256(R * sizeof(SortSeg));
    const size_t stride = tile_at + round256((R + 1) * sizeof(uint32_t)), dev_stride = stride - segs_at;
    if (!ctx->stream_b) VSC_TRY(hipStreamCreateWithFlags(&ctx->stream_b, hipStreamNonBlocking));
    const hipStream_t B = ctx->stream_b;
    while (ctx->part_ev.size() < 3 * (size_t)K + 1) {
        hipEvent_t e = nullptr;
        VSC_TRY(hipEventCreate(&e));
        ctx->part_ev.push_back(e);
    }
    if (ctx->pinned_cap < K * stride + 256) {
        if (ctx->pinned) (void)hipHostFree(ctx->pinned);
        ctx->pinned = nullptr;
        ctx->pinned_cap = 0;
        VSC_TRY(hipHostMalloc(&ctx->pinned, K * stride + 256, hipHostMallocDefault));
        ctx->pinned_cap = K * stride + 256;
    }
    char *const pin = (char *)ctx->pinned;
    uint32_t *const pin_total = (uint32_t *)(pin + K * stride);
    SortLevel1 &l1 = f.l1;
    const size_t n_bins = (size_t)R << l1.bits;
    // the level's tables and its destination, as bin_sort would make them (it finds them made)
    VSC_TRY(ctx->keys_b.ensure(std::max<uint64_t>((uint64_t)n_bins * l1.slot_cap, f.cap) * sizeof(uint64_t)));
    VSC_TRY(ctx->sort_tabs.ensure(3 * n_bins * sizeof(uint32_t)));
    VSC_TRY(ctx->sort_over.ensure(256 + n_bins * sizeof(SortSeg)));
    VSC_TRY(ctx->sort_segs.ensure(std::max<size_t>(K * dev_stride, round256(R * sizeof(SortSeg)) + (R + 1) * sizeof(uint32_t))));
    SortArgs pa{};
    pa.n_segs = R;
    pa.in = (const uint64_t *)ctx->keys_a.p;
    pa.out = (uint64_t *)ctx->keys_b.p;
    pa.cursor = (uint32_t *)ctx->sort_tabs.p + n_bins;
    pa.hist = pa.cursor;
    pa.bin_start = pa.cursor + n_bins;
    pa.bin_bits = l1.bits;
    pa.bin_shift = kRecPosShift + f.pos_pad + f.key_bits - l1.bits;
    pa.fill = l1.fill;
    pa.fill_shift = l1.fill_shift;
    pa.slot_cap = (uint32_t)l1.slot_cap;
    pa.overflow = (uint32_t *)ctx->sort_over.p + 2;
    VSC_TRY(hipMemsetAsync(pa.cursor, 0, n_bins * sizeof(uint32_t), A));
    VSC_TRY(hipMemsetAsync(ctx->sort_over.p, 0, 3 * sizeof(uint32_t), A));
    VSC_TRY(hipMemcpyAsync(pin_total, (const uint32_t *)ctx->seed_poff.p + kLists, sizeof(uint32_t), hipMemcpyDeviceToHost, A));
    VSC_TRY(hipEventRecord(ctx->ev[kEvSearchStart], A));
    for (uint32_t i = 0; i < K; ++i) {
        // part i: chunks [n i / K, n (i + 1) / K) - its own piece of the chunk table, sliced by the 32 work cursors as a whole table is
        const uint32_t chunk_first = (uint32_t)((uint64_t)all.n_chunks * i / K);
        sa.chunk_tab = all.chunk_tab + chunk_first;
        sa.n_chunks = (uint32_t)((uint64_t)all.n_chunks * (i + 1) / K) - chunk_first;
        // part 1 has the CUs to itself, the others share them with a partition (the hook overrides both)
        const uint32_t per_cu = ctx->dbg.seed_groups_per_cu ? ctx->dbg.seed_groups_per_cu : (i ? kSeedPartGroupsPerCu : (uint32_t)kSlicedWavesPerSimd);
        const uint32_t n_grabs = (sa.n_chunks + kSlicedGrab - 1) / kSlicedGrab;
        const uint32_t n_waves = std::max<uint32_t>(1, std::min<uint32_t>((uint32_t)ctx->n_cus * per_cu * kWavesPerGroup, shared ? n_grabs * kWavesPerGroup : n_grabs));
        if (i) VSC_TRY(hipMemsetAsync(sa.counters + kCursorBase, 0, (size_t)kCursors * kCursorStride * sizeof(unsigned long long), A));
        VSC_TRY(hipEventRecord(ctx->part_ev[3 * i], A));
        VSC_TRY(launch_seed_sliced(sa, (int)((n_waves + kWavesPerGroup - 1) / kWavesPerGroup), shared, A));
        VSC_TRY(hipEventRecord(ctx->part_ev[3 * i + 1], A));
        VSC_TRY(hipMemcpyAsync(pin + i * stride + cnt_at, sa.counters, cnt_bytes, hipMemcpyDeviceToHost, A));
        VSC_TRY(hipEventRecord(ctx->part_ev[3 * i + 2], A));
    }
    VSC_TRY(hipEventRecord(ctx->ev[kEvSearchEnd], A));
    bool lost = false;
    for (uint32_t i = 0; i < K; ++i) {
        VSC_TRY(hipEventSynchronize(ctx->part_ev[3 * i + 2]));
        const unsigned long long *const now = (const unsigned long long *)(pin + i * stride + cnt_at);
        const unsigned long long *const before = i ? (const unsigned long long *)(pin + (i - 1) * stride + cnt_at) : nullptr;
        if (now[kCntOverflow]) lost = true;
        if (lost) continue;  // (the parts still queued run out; nothing more is partitioned)
        SortSeg *const segs = (SortSeg *)(pin + i * stride + segs_at);
        uint32_t *const tile0 = (uint32_t *)(pin + i * stride + tile_at);
        uint64_t tiles = 0;
        for (uint32_t q = 0; q < R; ++q) {
            const uint64_t b = before ? before[kCntPart + 4 * q] : 0, e = now[kCntPart + 4 * q];
            const uint64_t at = (uint64_t)q * sa.part_cap + b;
            segs[q] = SortSeg{at, at, 0, (uint32_t)(e - b), 0, q, 0};
            tile0[q] = (uint32_t)tiles;
            tiles += (e - b + kSortTile - 1) / kSortTile;
        }
        tile0[R] = (uint32_t)tiles;
        if (tiles == 0) continue;
        if (tiles >= (1ull << 31)) return hipErrorInvalidValue;
        char *const dev = (char *)ctx->sort_segs.p + i * dev_stride;
        VSC_TRY(hipStreamWaitEvent(B, ctx->part_ev[3 * i + 2], 0));
        VSC_TRY(hipMemcpyAsync(dev, segs, dev_stride, hipMemcpyHostToDevice, B));
        pa.segs = (const SortSeg *)dev;
        pa.seg_tile0 = (const uint32_t *)(dev + (tile_at - segs_at));
        pa.n_tiles = (uint32_t)tiles;
        pa.xcd_tiles = 0;
        pa.xcd_by_region = 0;
        if (ctx->dbg.sort_xcd != 0 && tiles >= 64) {
            // XCD x takes the segments of regions [R x / 8, R (x + 1) / 8): the same regions in every part
            pa.xcd_by_region = 1;
            for (uint32_t x = 0; x <= 8; ++x) pa.xcd_first[x] = tile0[(uint64_t)R * x / 8];
            for (uint32_t x = 0; x < 8; ++x) pa.xcd_tiles = std::max(pa.xcd_tiles, pa.xcd_first[x + 1] - pa.xcd_first[x]);
        }
        VSC_TRY(launch_bin_partition(pa, B));
    }
    VSC_TRY(hipEventRecord(ctx->part_ev[3 * K], B));
    VSC_TRY(hipStreamWaitEvent(A, ctx->part_ev[3 * K], 0));
    std::memcpy(cnt, pin + (K - 1) * stride + cnt_at, cnt_bytes);
    *list_total = *pin_total;
    *scan_ms = 0;
    for (uint32_t i = 0; i < K; ++i) {
        float ms = 0;
        VSC_TRY(hipEventElapsedTime(&ms, ctx->part_ev[3 * i], ctx->part_ev[3 * i + 1]));
        *scan_ms += ms;
    }
    l1.done = !lost;
    if (lost) VSC_TRY(hipStreamSynchronize(A));  // (B's partitions included: the pass starts over)
    return hipSuccess;
}

// The search of a pass over guides[0 .. n_guides) (<= kMaxPassReads; read indices guide_base + i) up to final records, with
// the genome's sizing hints it learns.  keep_bases (SEED): every hit's site lo plane beside its record.  Timings ADD to t.
// sort_only: the sort is the only reader of the records (SEED: block fill table instead of sentinels, perhaps a search in parts).
int find_pass(vsc_ctx *ctx, const vsc_genome *genome, const uint64_t *guides, uint32_t n_guides, uint32_t guide_base,
              const vsc_search_params *params, bool keep_bases, bool sort_only, vsc_timing &t, PassFound &f)
{
    const int algo = (int)t.algorithm;  // search_setup's choice
    const uint32_t m = params->max_mismatches;
    f.algo = algo;
    f.max_mm = m;
    f.guide_base = guide_base;
    f.bases = keep_bases;
    // reads as (hi, lo) plane pairs, padded to the unroll factor with reads that can never match
    const uint32_t n_pad = (n_guides + kGuideUnroll - 1) / kGuideUnroll * kGuideUnroll;
    std::vector<uint32_t> gp((size_t)(n_pad + kGuideUnroll) * 2, 0xFFFFFFFFu);  // + one prefetch group
    for (uint32_t i = 0; i < n_guides; ++i) guide_planes(guides[i], &gp[2 * (size_t)i], &gp[2 * (size_t)i + 1]);
    VSC_HIP(ctx, ctx->guides.ensure(gp.size() * sizeof(uint32_t)));
    VSC_HIP(ctx, ctx->counters.ensure(kCounterWords * sizeof(unsigned long long)));
    VSC_HIP(ctx, hipEventRecord(ctx->ev[kEvPassStart], ctx->stream));
    VSC_HIP(ctx, hipMemcpyAsync(ctx->guides.p, gp.data(), gp.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));

    const double own_bases = (double)genome->n_tiles * kTileBases;
    const double sites_est = genome->sites ? (double)genome->sites : own_bases / 4;
    f.cap = (uint64_t)(1.5 * sites_est * n_guides * hit_probability(m)) + (1u << 20);
    const double seen_rate = genome->seen_rate[m];  // 0: no search with this budget yet
    if (algo == VSC_ALGO_SCAN) f.cap = std::max<uint64_t>(f.cap, (uint64_t)(1.2 * seen_rate * n_guides) + 4096);
    unsigned long long cnt[kCntPart + 4 * kParts] = {};
    f.n_parts = (int)((n_guides + kRegionReads - 1) / kRegionReads);  // output regions of 64 reads
    // bits the positions of this shard need, counted from the shard's first position (a shard of the upper part of a
    // genome must not leave the top key bits constant); the records keep them at the top of their 32-bit position field
    f.pos_base = (uint32_t)(genome->first_word * 32);
    const unsigned pos_bits = std::max(1u, ceil_log2((uint64_t)genome->dev_words * 32));
    f.pos_pad = pos_bits < 32 ? 32 - pos_bits : 0;
    f.key_bits = pos_bits + 1 + ceil_log2(std::min<uint32_t>(n_guides, kRegionReads));

    ScanArgs a{};
    SeedArgs sa{};
    int n_groups = 1;
    bool seed_shared = false;
    // records that go to the sort and nowhere else (no other sink walks them, no side words): the unused tails of the
    // search's blocks are named by the block fill table instead of being written as sentinels and read back
    const bool use_fill = algo == VSC_ALGO_SEED && sort_only && !keep_bases;
    uint32_t n_parts_k = 1;  // launches of the search (plan_parts)
    auto owners_of = [](const SeedArgs &s, int groups) { return (uint64_t)(s.group_out ? groups : groups * kWavesPerGroup); };
    if (algo == VSC_ALGO_SCAN) {
        fill_pam(a, params);
        fill_genome(a, ctx, genome);
        a.guides = (const uint4 *)ctx->guides.p;
        a.n_guides_padded = n_pad;
        a.max_mm = m;
        a.k_half = m / 2;  // bidir_mapping.cpp:129-146
        n_groups = scan_groups(ctx, a.n_tiles);
        t.genome_bytes += (uint64_t)genome->n_tiles * kTileWords * 3 * sizeof(uint32_t);
        VSC_HIP(ctx, hipEventRecord(ctx->ev[kEvPrepEnd], ctx->stream));
    } else {
        VSC_HIP(ctx, seed_plan(ctx, genome, gp.data(), n_guides, f, sa, &n_groups, &seed_shared));
        if (use_fill) {
            // a tile of the sort never straddles regions, and a block of the fill table never does (reserve divides kSortTile);
            // every launch of a search in parts leaves a block open per owner and region
            n_parts_k = plan_parts(ctx, genome, f, sa, n_guides, seed_shared, f.l1);
            sa.part_cap += (uint64_t)(n_parts_k - 1) * owners_of(sa, n_groups) * sa.reserve;
            sa.part_cap = (sa.part_cap + kSortTile - 1) / kSortTile * kSortTile;
        }
        f.cap = sa.part_cap * f.n_parts;
    }

    f.ht.lap("prep enqueue");
    uint32_t list_total = 0;
    float parts_ms = -1;  // a search in parts: the sum of its launches
    for (unsigned tries = 0;; ++tries) {
        // (the kernel keeps a block number in 20 bits, all ones meaning "full": part_cap / reserve < 2^20 - 1)
        if (algo == VSC_ALGO_SEED && (sa.part_cap >= (1ull << 32) - (1u << 20) || sa.part_cap >= ((uint64_t)sa.reserve << 20) - sa.reserve))
            return fail(ctx, VSC_ERR_RANGE, "vsc_search: more than 2^32 hits in a block of 64 reads");
        VSC_HIP(ctx, ctx->keys_a.ensure(f.cap * sizeof(uint64_t)));
        VSC_HIP(ctx, hipMemsetAsync(ctx->counters.p, 0, kCounterWords * sizeof(unsigned long long), ctx->stream));
        if (use_fill) {
            const size_t fill_bytes = (size_t)(f.cap >> sa.reserve_log2) * sizeof(uint32_t);
            VSC_HIP(ctx, ctx->seed_fill.ensure(fill_bytes));
            VSC_HIP(ctx, hipMemsetAsync(ctx->seed_fill.p, 0xFF, fill_bytes, ctx->stream));  // every block "full" until a wave leaves it open
            sa.fill = (uint32_t *)ctx->seed_fill.p;
            f.l1.fill = sa.fill;
            f.l1.fill_shift = sa.reserve_log2;
        }
        if (n_parts_k > 1) {
            sa.hit_recs = (uint64_t *)ctx->keys_a.p;
            VSC_HIP(ctx, search_in_parts(ctx, f, sa, n_parts_k, seed_shared, cnt, sizeof cnt, &list_total, &parts_ms));
            f.ht.lap("search in parts");
            t.passes++;
            if (!cnt[kCntOverflow]) break;
            if (tries >= 2) return fail(ctx, VSC_ERR_DEVICE, "vsc_search: hit buffer overflowed repeatedly");
            // records were lost: the whole pass again in one launch, with room for what the counters say
            uint64_t need = 0;
            for (int q = 0; q < f.n_parts; ++q) need = std::max<uint64_t>(need, cnt[kCntPart + 4 * q] + cnt[kCntPart + 4 * q + 2]);
            n_parts_k = 1;
            f.l1.done = false;
            sa.part_cap = need + (need >> 6) + 4096 + owners_of(sa, n_groups) * sa.reserve;
            sa.part_cap = (sa.part_cap + kSortTile - 1) / kSortTile * kSortTile;
            f.cap = sa.part_cap * f.n_parts;
            continue;
        }
        VSC_HIP(ctx, hipEventRecord(ctx->ev[kEvSearchStart], ctx->stream));
        if (algo == VSC_ALGO_SCAN) {
            VSC_HIP(ctx, ctx->vals_a.ensure(f.cap * sizeof(uint32_t)));
            a.hit_keys = (uint64_t *)ctx->keys_a.p;
            a.hit_vals = (uint32_t *)ctx->vals_a.p;
            a.hit_cap = f.cap;
            VSC_HIP(ctx, launch_scan(a, n_groups, false, ctx->stream));
        } else {
            sa.hit_recs = (uint64_t *)ctx->keys_a.p;
            if (keep_bases) {
                VSC_HIP(ctx, ctx->vals_a.ensure(f.cap * sizeof(uint32_t)));
                sa.hit_side = (uint32_t *)ctx->vals_a.p;
            }
            VSC_HIP(ctx, launch_seed_sliced(sa, n_groups, seed_shared, ctx->stream));
        }
        VSC_HIP(ctx, hipEventRecord(ctx->ev[kEvSearchEnd], ctx->stream));
        VSC_HIP(ctx, hipMemcpyAsync(cnt, ctx->counters.p, sizeof cnt, hipMemcpyDeviceToHost, ctx->stream));
        if (algo == VSC_ALGO_SEED)
            VSC_HIP(ctx, hipMemcpyAsync(&list_total, (const uint32_t *)ctx->seed_poff.p + kLists, sizeof list_total, hipMemcpyDeviceToHost, ctx->stream));
        VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        f.ht.lap("search kernel + sync");
        t.passes++;
        if (!cnt[kCntOverflow]) break;
        if (tries >= 2) return fail(ctx, VSC_ERR_DEVICE, "vsc_search: hit buffer overflowed repeatedly");
        // the counters hold the true totals (SEED: records placed + records lost per region, + one block per wave)
        if (algo == VSC_ALGO_SEED) {
            uint64_t need = 0;
            for (int q = 0; q < f.n_parts; ++q) need = std::max<uint64_t>(need, cnt[kCntPart + 4 * q] + cnt[kCntPart + 4 * q + 2]);
            sa.part_cap = need + (need >> 6) + 4096 + owners_of(sa, n_groups) * sa.reserve;
            if (use_fill) sa.part_cap = (sa.part_cap + kSortTile - 1) / kSortTile * kSortTile;
            f.cap = sa.part_cap * f.n_parts;
        } else {
            f.cap = cnt[kCntHits] + (cnt[kCntHits] >> 6) + 4096;
        }
    }
    float ms = 0;
    VSC_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev[kEvPassStart], ctx->ev[kEvPrepEnd]));
    t.prep_ms += ms;
    if (f.l1.done) {
        ms = parts_ms;
    } else {
        VSC_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev[kEvSearchStart], ctx->ev[kEvSearchEnd]));
    }
    t.scan_ms += ms;

    // ---- the records: one segment of pairs (SCAN) or one per region (SEED) ----------------------------------------
    if (algo == VSC_ALGO_SCAN) {
        genome->sites = cnt[kCntSites];
        t.sites = cnt[kCntSites];
        t.pairs += cnt[kCntSites] * n_guides;
        t.seed_layout = 0;
        f.n = cnt[kCntHits];
        genome->seen_rate[m] = (double)f.n / n_guides;
        if (f.n >= (1ull << 32)) return fail(ctx, VSC_ERR_RANGE, "vsc_search: more than 2^32 hits in one scan pass (split the read set)");
        if (f.n > 0) f.segs.push_back(SortSeg{0, 0, 0, (uint32_t)f.n, guide_base});
    } else {
        t.list_entries = list_total;
        t.seed_cut = sa.k_seg0 | (sa.k_seg1 << 4);
        // the layout of the attempt that produced the records (after a lost-records rerun: one launch)
        t.seed_layout = (seed_shared ? 1u : 0u) | (sa.group_out ? 2u : 0u) | (use_fill ? 4u : 0u) | (sa.reserve_log2 << 4) | (n_parts_k << 8);
        t.sites = genome->index_sites;
        t.pairs += cnt[kCntSites];
        t.genome_bytes += cnt[kCntVisited] * kVertWords * sizeof(uint32_t) / kSlicedSites;  // sites visited, 3.5 bytes each bit-sliced
        double fullest = 0;
        for (int q = 0; q < f.n_parts; ++q) {
            const uint64_t placed = cnt[kCntPart + 4 * q], real = placed - cnt[kCntPart + 4 * q + 1];
            fullest = std::max(fullest, (double)placed / std::min<uint32_t>(kRegionReads, n_guides - (uint32_t)q * kRegionReads));
            // (a search in parts: every region, so that segment i is region i, as its partitions had it)
            if (placed || f.l1.done) f.segs.push_back(SortSeg{(uint64_t)q * sa.part_cap, (uint64_t)q * sa.part_cap, f.n, (uint32_t)placed,
                                                              guide_base + (uint32_t)q * kRegionReads, (uint32_t)q, 0});
            f.n += real;
        }
        f.l1.n_real = f.n;
        genome->seen_rate[m] = fullest;
        // (the sort's second buffer, ctx->keys_b, is sized by bin_sort for the layout its first level uses)
    }
    t.hits += f.n;
    return VSC_OK;
}

// The sinks' input of the pass (SinkInput, vsc_internal.h) in f.sink: the pass's records where the search left them, and f.segs
// on the device (in ctx->sort_segs) as segments relative to the pass's first read with the prefix of their tile counts.  The
// first sink of the pass that asks builds and uploads the tables (staged in f, see PassFound); the others take them as they
// are - every sink of a pass runs before select_pass and sort_pass put ctx->sort_segs and f.segs to their own use.
// What the callers keep to: every sink of a pass passes the same `excluded` (only the first call reads it; run_search hands
// all of them !excl.empty()), and f.sink holds device addresses of ctx->keys_a, vals_a, sort_segs and sum_excl, so none of
// these buffers goes through ensure() between the first sink_input of a pass and the last sink's launch.
hipError_t sink_input(vsc_ctx *ctx, PassFound &f, bool excluded)
{
    if (f.sink.recs) return hipSuccess;
    f.sink_tile0.assign(1, 0);
    for (const SortSeg &sg : f.segs) {
        f.sink_segs.push_back(SumSeg{sg.in_off, sg.n_in, sg.guide_base - f.guide_base});
        f.sink_tile0.push_back(f.sink_tile0.back() + (sg.n_in + kSumTile - 1) / kSumTile);
    }
    const size_t seg_bytes = f.sink_segs.size() * sizeof(SumSeg), tile0_bytes = f.sink_tile0.size() * sizeof(uint32_t);
    const size_t tile0_at = (seg_bytes + 255) / 256 * 256;
    VSC_TRY(ctx->sort_segs.ensure(tile0_at + tile0_bytes));
    VSC_TRY(hipMemcpyAsync(ctx->sort_segs.p, f.sink_segs.data(), seg_bytes, hipMemcpyHostToDevice, ctx->stream));
    VSC_TRY(hipMemcpyAsync((char *)ctx->sort_segs.p + tile0_at, f.sink_tile0.data(), tile0_bytes, hipMemcpyHostToDevice, ctx->stream));
    SinkInput &a = f.sink;
    a.vals = f.algo == VSC_ALGO_SCAN ? (const uint32_t *)ctx->vals_a.p : nullptr;
    a.segs = (const SumSeg *)ctx->sort_segs.p;
    a.seg_tile0 = (const uint32_t *)((char *)ctx->sort_segs.p + tile0_at);
    a.n_segs = (uint32_t)f.sink_segs.size();
    a.n_tiles = f.sink_tile0.back();
    a.pos_pad = f.pos_pad;
    a.pos_base = f.pos_base;
    a.excl = excluded ? (const uint64_t *)ctx->sum_excl.p + f.guide_base : nullptr;
    a.recs = (const uint64_t *)ctx->keys_a.p;
    return hipSuccess;
}

// The end of a sink: waits for the pass; the sink's own stage (kEvSinkStart -> kEvSinkEnd) is finalize_ms, the whole pass total_ms.
hipError_t end_pass(vsc_ctx *ctx, PassFound &f, const char *lap, vsc_timing &t)
{
    VSC_TRY(hipEventRecord(ctx->ev[kEvSinkEnd], ctx->stream));
    VSC_TRY(hipStreamSynchronize(ctx->stream));
    f.ht.lap(lap);
    float ms = 0;
    VSC_TRY(hipEventElapsedTime(&ms, ctx->ev[kEvSinkStart], ctx->ev[kEvSinkEnd]));
    t.finalize_ms += ms;
    VSC_TRY(hipEventElapsedTime(&ms, ctx->ev[kEvPassStart], ctx->ev[kEvSinkEnd]));
    t.total_ms += ms;
    t.read_passes++;
    return hipSuccess;
}

// Record sink (vsc_search, the stream calls): sorts the records into `hits` behind its `used` ones (`projected`: its expected
// final size).  With f.bases the last stage also writes every hit's feature row into ctx->score_feat (pass row i at 64 i).
int sort_pass(vsc_ctx *ctx, const vsc_genome *genome, PassFound &f, vsc_hits *hits, uint64_t used, uint64_t projected, vsc_timing &t)
{
    SortInfo info;
    if (f.n > 0) {
        uint64_t *src = (uint64_t *)ctx->keys_a.p, *other = nullptr;
        if (f.algo == VSC_ALGO_SCAN && !f.selected) {
            // level 0: (key, value) pairs -> packed records, partitioned by region
            VSC_HIP(ctx, ctx->keys_b.ensure(f.cap * sizeof(uint64_t)));
            const unsigned bits0 = ceil_log2((uint64_t)f.n_parts);
            const size_t n_bins = (size_t)1 << bits0;
            VSC_HIP(ctx, ctx->sort_segs.ensure(512));
            VSC_HIP(ctx, ctx->sort_tabs.ensure(3 * n_bins * sizeof(uint32_t)));
            const uint32_t tile0[2] = {0u, (uint32_t)((f.n + kSortTile - 1) / kSortTile)};
            VSC_HIP(ctx, hipMemcpyAsync(ctx->sort_segs.p, f.segs.data(), sizeof(SortSeg), hipMemcpyHostToDevice, ctx->stream));
            VSC_HIP(ctx, hipMemcpyAsync((char *)ctx->sort_segs.p + 256, tile0, sizeof tile0, hipMemcpyHostToDevice, ctx->stream));
            SortArgs l0{};
            l0.segs = (const SortSeg *)ctx->sort_segs.p;
            l0.seg_tile0 = (const uint32_t *)((char *)ctx->sort_segs.p + 256);
            l0.n_segs = 1;
            l0.n_tiles = tile0[1];
            l0.pair_keys = (const uint64_t *)ctx->keys_a.p;
            l0.pair_vals = (const uint32_t *)ctx->vals_a.p;
            l0.out = (uint64_t *)ctx->keys_b.p;
            l0.hist = (uint32_t *)ctx->sort_tabs.p;
            l0.cursor = l0.hist + n_bins;
            l0.bin_start = l0.cursor + n_bins;
            l0.bin_bits = bits0;
            l0.bin_shift = kRecKeyBits;  // key >> 39 = read index >> 6 = region
            l0.pos_pad = f.pos_pad;
            l0.pos_base = f.pos_base;
            VSC_HIP(ctx, hipMemsetAsync(l0.hist, 0, n_bins * sizeof(uint32_t), ctx->stream));
            VSC_HIP(ctx, launch_bin_hist(l0, ctx->stream));
            VSC_HIP(ctx, launch_bin_scan(l0, ctx->stream));
            VSC_HIP(ctx, launch_bin_partition(l0, ctx->stream));
            std::vector<uint32_t> tabs(3 * n_bins);
            VSC_HIP(ctx, hipMemcpyAsync(tabs.data(), l0.hist, tabs.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
            VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));
            f.segs.clear();
            for (int q = 0; q < f.n_parts; ++q) {
                const uint32_t count = tabs[q], start = tabs[2 * n_bins + q];
                if (count) f.segs.push_back(SortSeg{start, start, start, count, f.guide_base + (uint32_t)q * kRegionReads});
            }
            src = (uint64_t *)ctx->keys_b.p;
            other = (uint64_t *)ctx->keys_a.p;
            info.bytes += 12 * f.n + 20 * f.n;  // histogram read; partition read 12, write 8
        }
        for (SortSeg &s : f.segs) s.final_off += used;
        f.ht.lap("sort buffers");
        VSC_HIP(ctx, result_room(ctx, hits, used, f.n, projected));
        f.ht.lap("record storage");
        // the seed search's regions go through the slot partition (no histogram pass) unless this genome has shown
        // bins that outgrow their slots at this budget
        // (survivors of a selection say nothing about the genome's bins: they neither use nor change what it remembers)
        bool *slots = f.algo == VSC_ALGO_SEED && !f.selected ? &genome->sort_slots_ok[f.max_mm] : nullptr;
        SortRows rows;
        if (f.bases) {
            // the batch's rows, all at once (the caller reads them in its callback): 64 bytes per hit - 104 GB for 10 000 reads at
            // 8 mismatches on 3 Gbp.  If that does not fit beside the pooled buffers, those go back first.
            if (ctx->score_feat.ensure(f.n * VSC_PACKED_FEATURE_BYTES) != hipSuccess) {
                (void)hipGetLastError();
                for (auto &b : ctx->spare_records) b.release();
                ctx->spare_records.clear();
                for (DeviceBuf *b : {&ctx->score_mit, &ctx->score_flags, &ctx->score_sched, &ctx->keys_b, &ctx->vals_b}) b->release();
                VSC_HIP(ctx, ctx->score_feat.ensure(f.n * VSC_PACKED_FEATURE_BYTES));
            }
            rows.side_src = (uint32_t *)ctx->vals_a.p;
            rows.side_other = &ctx->vals_b;
            rows.guides = (const uint2 *)ctx->guides.p;
            rows.guide_first = f.guide_base;
            rows.rows = (uint4 *)ctx->score_feat.p;
            rows.rows_first = used;
        }
        VSC_HIP(ctx, bin_sort(ctx, genome, std::move(f.segs), src, other, f.key_bits, f.pos_pad, f.pos_base, hits->d_records, ctx->ev[kEvSinkStart],
                              &info, f.algo == VSC_ALGO_SEED || f.selected ? &ctx->keys_b : nullptr, slots, f.bases ? &rows : nullptr,
                              f.algo == VSC_ALGO_SEED && !f.selected && (f.l1.fill || f.l1.done) ? &f.l1 : nullptr));
    } else {
        VSC_HIP(ctx, hipEventRecord(ctx->ev[kEvSinkStart], ctx->stream));
    }
    VSC_HIP(ctx, end_pass(ctx, f, "sort + finalize + sync", t));
    float ms = 0;
    VSC_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev[kEvSearchEnd], ctx->ev[kEvSinkStart]));
    t.sort_ms += ms;
    t.sort_levels = std::max(t.sort_levels, info.levels);
    t.sort_bin_bits = std::max(t.sort_bin_bits, info.bin_bits);
    t.sort_bytes += info.bytes;
    t.sort_fallbacks += info.slot_fallbacks;
    return VSC_OK;
}

// the forest calls further down, which classify_pass shares with vsc_score_classify_hits
int prepare_forest(vsc_ctx *ctx, const vsc_rf_model *model, const char *who);
void fill_forest(RfArgs &a, const vsc_ctx *ctx);
int resident_ranks(vsc_ctx *ctx, const double *guide_activity, uint32_t n_guides);

// Classify stage (vsc_search_*_classified), between find_pass and the sinks: rf_predict_kernel walks the forest (made resident
// by prepare_forest, the reads' activity ranks by resident_ranks, the interleaved planes by ensure_hl - all before the first
// pass) over the records where the search kernel left them and leaves every record slot's votes in ctx->vals_b, one word per
// slot of every tile of kSumTile - the layout of SelectArgs::score, which select_pass then takes as its keys.  Few rows: the
// trees are split over several workgroups per row tile, the votes meet in atomics.  Nothing is read back: the kernel's time
// (kEvClassStart -> kEvClassEnd) is taken at the end of the pass.
int classify_pass(vsc_ctx *ctx, const vsc_genome *genome, PassFound &f, uint32_t n_reads, bool excluded)
{
    if (f.segs.empty()) return VSC_OK;
    RfArgs a{};
    VSC_HIP(ctx, sink_input(ctx, f, excluded));
    fill_forest(a, ctx);
    a.in = f.sink;
    a.score.hl = genome->d_hl;
    a.score.first_pos = (uint32_t)(genome->first_word * 32);
    a.score.n_plane_words = genome->dev_words;
    a.score.guides = (const uint2 *)ctx->guides.p;  // the pass's reads
    a.act_rank = (const uint8_t *)ctx->forest.ranks.p + f.guide_base;
    a.n_reads = n_reads;
    a.n = (uint64_t)a.in.n_tiles * kSumTile;
    VSC_HIP(ctx, ctx->vals_b.ensure((size_t)a.n * sizeof(uint32_t)));
    a.slot_votes = (uint32_t *)ctx->vals_b.p;
    const uint64_t groups = a.n / kRfRows;
    a.tree_splits = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>({(uint64_t)2 * ctx->n_cus / groups, 32, ctx->forest.n_trees}));
    if (a.tree_splits > 1) VSC_HIP(ctx, hipMemsetAsync(a.slot_votes, 0, (size_t)a.n * sizeof(uint32_t), ctx->stream));
    VSC_HIP(ctx, hipEventRecord(ctx->ev[kEvClassStart], ctx->stream));
    VSC_HIP(ctx, launch_rf_predict(a, ctx->stream));
    VSC_HIP(ctx, hipEventRecord(ctx->ev[kEvClassEnd], ctx->stream));
    f.classified = true;
    return VSC_OK;
}

hipError_t end_pass(vsc_ctx *ctx, PassFound &f, const char *lap, vsc_timing &t);

// The device copy of `table` on this context: the context keeps the copy of the table it used last, keyed by its serial
// number; another table is uploaded over it on the context's stream.
int resident_table(vsc_ctx *ctx, const vsc_score_table *table)
{
    if (ctx->table_serial == table->serial && ctx->table_buf.p) return VSC_OK;
    ctx->table_serial = 0;
    VSC_HIP(ctx, ctx->table_buf.ensure(sizeof table->w));
    VSC_HIP(ctx, hipMemcpyAsync(ctx->table_buf.p, table->w, sizeof table->w, hipMemcpyHostToDevice, ctx->stream));
    VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (the caller may free the table as soon as its call returns)
    ctx->table_serial = table->serial;
    return VSC_OK;
}

// ... and of a pattern table (vsc_search_pattern_table), the same way
int resident_pattern_table(vsc_ctx *ctx, const vsc_pattern_table *table)
{
    if (ctx->pattern_table_serial == table->serial && ctx->pattern_table_buf.p) return VSC_OK;
    ctx->pattern_table_serial = 0;
    const size_t bytes = pattern_table_weights(table->shape) * sizeof(double);
    VSC_HIP(ctx, ctx->pattern_table_buf.ensure(bytes));
    VSC_HIP(ctx, hipMemcpyAsync(ctx->pattern_table_buf.p, table->w, bytes, hipMemcpyHostToDevice, ctx->stream));
    VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (the caller may free the table as soon as its call returns)
    ctx->pattern_table_serial = table->serial;
    return VSC_OK;
}

// Table score stage (vsc_search_*_table), between find_pass and the sinks, where classify_pass sits for the classifier:
// table_score_kernel scores the records where the search kernel left them (the table made resident by resident_table, the
// interleaved planes by ensure_hl - both before the first pass) and leaves every record slot's fixed-point score in
// ctx->vals_b, one word per slot of every tile of kSumTile - the layout of SelectArgs::score, which select_pass then takes as
// its keys.  Nothing is read back: the kernel's time (kEvClassStart -> kEvClassEnd) is taken at the end of the pass.
int table_score_pass(vsc_ctx *ctx, const vsc_genome *genome, PassFound &f, uint32_t n_reads, bool excluded)
{
    if (f.segs.empty()) return VSC_OK;
    TableArgs a{};
    VSC_HIP(ctx, sink_input(ctx, f, excluded));
    a.in = f.sink;
    a.weights = (const double *)ctx->table_buf.p;
    a.hl = genome->d_hl;
    a.first_pos = (uint32_t)(genome->first_word * 32);
    a.n_plane_words = genome->dev_words;
    a.guides = (const uint2 *)ctx->guides.p;  // the pass's reads
    a.n_reads = n_reads;
    VSC_HIP(ctx, ctx->vals_b.ensure((size_t)a.in.n_tiles * kSumTile * sizeof(uint32_t)));
    a.slot_fixed = (uint32_t *)ctx->vals_b.p;
    VSC_HIP(ctx, hipEventRecord(ctx->ev[kEvClassStart], ctx->stream));
    VSC_HIP(ctx, launch_table_score(a, ctx->stream));
    VSC_HIP(ctx, hipEventRecord(ctx->ev[kEvClassEnd], ctx->stream));
    f.classified = true;
    return VSC_OK;
}

// Table summary sink (vsc_search_*_table), behind table_score_pass: table_summary_kernel adds the fixed-point words into the
// pass's rows of ctx->table_rows.  first / last: as votes_summary_pass takes them.
int table_summary_pass(vsc_ctx *ctx, PassFound &f, uint32_t n_reads, bool excluded, vsc_timing &t, bool first, bool last)
{
    TableSummaryArgs a{};
    if (!f.segs.empty()) {
        VSC_HIP(ctx, sink_input(ctx, f, excluded));
        static_cast<SinkInput &>(a) = f.sink;
        a.out = (unsigned long long *)ctx->table_rows.p + (size_t)f.guide_base * kSumWords;
        a.fixed = (const uint32_t *)ctx->vals_b.p;
        a.n_reads = n_reads;
    }
    if (first && last) VSC_HIP(ctx, hipEventRecord(ctx->ev[kEvSinkStart], ctx->stream));
    VSC_HIP(ctx, launch_table_summary(a, ctx->stream));
    if (last) VSC_HIP(ctx, end_pass(ctx, f, "table summary + sync", t));
    return VSC_OK;
}

// Votes summary sink (vsc_search_*_classified), behind classify_pass: votes_summary_kernel adds the votes words into the pass's
// rows of ctx->votes_rows.  first: no sink ran before it in this pass (it opens finalize_ms); last: none follows (it ends the pass).
int votes_summary_pass(vsc_ctx *ctx, PassFound &f, uint32_t n_reads, bool excluded, vsc_timing &t, bool first, bool last)
{
    VotesSummaryArgs a{};
    if (!f.segs.empty()) {
        VSC_HIP(ctx, sink_input(ctx, f, excluded));
        static_cast<SinkInput &>(a) = f.sink;
        a.out = (unsigned long long *)ctx->votes_rows.p + (size_t)f.guide_base * kSumWords;
        a.votes = (const uint32_t *)ctx->vals_b.p;
        a.n_trees = ctx->forest.n_trees;
        a.n_reads = n_reads;
    }
    if (first && last) VSC_HIP(ctx, hipEventRecord(ctx->ev[kEvSinkStart], ctx->stream));
    VSC_HIP(ctx, launch_votes_summary(a, ctx->stream));
    if (last) VSC_HIP(ctx, end_pass(ctx, f, "votes summary + sync", t));
    return VSC_OK;
}

// Summary sink (vsc_search_summary): summary_kernel adds the records where they lie into the pass's rows of ctx->sum_rows,
// minus its loci in ctx->sum_excl if `excluded`.  No sort, no result buffer: finalize_ms times that kernel, sort_ms stays 0.
// last = false (vsc_search_select with a summary): another sink follows and ends the pass; the kernel is then only enqueued.
// Nothing waits for it here: the copies sink_input enqueued read f.sink_segs and f.sink_tile0, which are written once per
// pass and live until the pass has ended; what the later stages rewrite (f.segs, f.n, f.cap, f.sel_off, ctx->sort_segs) is
// read by no host-to-device copy of the sinks, and the stream orders their device work behind this kernel.  The host-timer
// lap of the stage that synchronises next ("select: scores + thresholds + sync", or the sort's) therefore takes in this
// kernel's time; vsc_timing, which is taken from events, is as it was.
// reg: the device copy of the regions (resident_regions) - the rows over the hits inside go to ctx->sum_rows_in as well.
int summarize_pass(vsc_ctx *ctx, PassFound &f, bool excluded, vsc_timing &t, bool last = true, const RegionsView *reg = nullptr)
{
    SummaryRegionArgs a{};
    if (!f.segs.empty()) {
        VSC_HIP(ctx, sink_input(ctx, f, excluded));
        static_cast<SinkInput &>(a) = f.sink;
        a.out = (unsigned long long *)ctx->sum_rows.p + (size_t)f.guide_base * kSumWords;
        if (reg) {
            a.reg = *reg;
            a.out_in = (unsigned long long *)ctx->sum_rows_in.p + (size_t)f.guide_base * kSumWords;
        }
    }
    VSC_HIP(ctx, hipEventRecord(ctx->ev[kEvSinkStart], ctx->stream));
    VSC_HIP(ctx, reg ? launch_summary_regions(a, ctx->stream) : launch_summary(a, ctx->stream));
    if (last) VSC_HIP(ctx, end_pass(ctx, f, "summary + sync", t));
    return VSC_OK;
}

// Selection stage (vsc_search_select), between find_pass and sort_pass: decides on the device, over the records where the
// search kernel left them, which survive - per read the sel.top_k best by rint(MIT * 2^24) among those >= sel.min_score that
// are not the read's excluded locus (SelectArgs, vsc_internal.h) - and leaves the survivors as packed records, region after
// region, at the start of ctx->keys_a: f.n, f.segs, f.cap describe them from here on, whichever algorithm found them, so the
// bin sort, the result buffer and everything downstream see survivors only.  Beyond the search's own buffers: 4 bytes per
// placed record (ctx->vals_b: the scores), 512 bytes per read of the pass (histograms) and 12 bytes per candidate.  One read-back
// (the reads' candidate counts), as find_pass has one for its counters.
// reg / drop: the selection is made among the records on one side of the regions (SelectRegionArgs).
// vote_trees (vsc_search_select_classified): the keys are the votes classify_pass left in ctx->vals_b, of a forest of that many trees.
// table_key (vsc_search_select_table): the keys are the fixed-point scores table_score_pass left there.
int select_pass(vsc_ctx *ctx, PassFound &f, uint32_t n_reads, const vsc_select &sel, bool excluded, const RegionsView *reg = nullptr,
                uint32_t drop = 0, uint32_t vote_trees = 0, uint32_t table_key = 0)
{
    f.selected = true;
    if (f.n == 0) return VSC_OK;
    hipStream_t st = ctx->stream;
    SelectRegionArgs a{};
    VSC_HIP(ctx, sink_input(ctx, f, excluded));
    static_cast<SinkInput &>(a) = f.sink;
    if (reg) {
        a.reg = *reg;
        a.drop = drop;
    }
    // per-read tables: thr, count, cursor, the regions' smallest thresholds (32-bit), then the lists' and the survivors' starts (64-bit)
    const size_t words = ((size_t)n_reads + 63) / 64 * 64;
    VSC_HIP(ctx, ctx->sel_tabs.ensure(4 * words * sizeof(uint32_t) + 2 * words * sizeof(uint64_t)));
    VSC_HIP(ctx, ctx->sel_hist.ensure((size_t)n_reads * kSelBins * sizeof(uint32_t)));
    VSC_HIP(ctx, ctx->vals_b.ensure((size_t)a.n_tiles * kSumTile * sizeof(uint32_t)));  // (the records the search placed, tiles rounded up)
    a.min_score = sel.min_score;
    a.vote_trees = vote_trees;
    a.table_key = table_key;
    a.top_k = sel.top_k;
    a.n_reads = n_reads;
    // enough workgroups for every CU, few table flushes per region
    a.tiles_per_block = std::min<uint32_t>(kSelMaxTilesPerBlock, std::max<uint32_t>(kSelMinTilesPerBlock, a.n_tiles / (16u * (uint32_t)ctx->n_cus)));
    a.score = (uint32_t *)ctx->vals_b.p;
    a.hist = (uint32_t *)ctx->sel_hist.p;
    a.thr = (uint32_t *)ctx->sel_tabs.p;
    a.count = a.thr + words;
    a.cursor = a.count + words;
    a.thr_region = a.cursor + words;
    uint64_t *d_off = (uint64_t *)(a.thr_region + words);
    a.cand_off = d_off;
    a.surv_off = d_off + words;
    VSC_HIP(ctx, hipMemsetAsync(a.hist, 0, (size_t)n_reads * kSelBins * sizeof(uint32_t), st));
    VSC_HIP(ctx, hipMemsetAsync(a.cursor, 0, words * sizeof(uint32_t), st));
    VSC_HIP(ctx, hipMemsetAsync(a.thr_region, 0xFF, words * sizeof(uint32_t), st));
    VSC_HIP(ctx, reg ? launch_select_score_regions(a, st) : launch_select_score(a, st));
    VSC_HIP(ctx, launch_select_threshold(a, st));
    std::vector<uint32_t> count(n_reads);
    VSC_HIP(ctx, hipMemcpyAsync(count.data(), a.count, (size_t)n_reads * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    VSC_HIP(ctx, hipStreamSynchronize(st));
    f.ht.lap("select: scores + thresholds + sync");
    // the lists' and the survivors' starts; the survivors' regions are the segments of the sort
    f.sel_off.assign(2 * words, 0);
    uint64_t n_cand = 0, n_surv = 0;
    for (uint32_t i = 0; i < n_reads; ++i) {
        f.sel_off[i] = n_cand;
        f.sel_off[words + i] = n_surv;
        n_cand += count[i];
        n_surv += sel.top_k ? std::min<uint32_t>(count[i], sel.top_k) : count[i];
    }
    f.segs.clear();
    for (uint32_t q = 0; q * (uint32_t)kRegionReads < n_reads; ++q) {
        const uint64_t begin = f.sel_off[words + (size_t)q * kRegionReads];
        const uint32_t next = (q + 1) * (uint32_t)kRegionReads;
        const uint64_t end = next < n_reads ? f.sel_off[words + next] : n_surv;
        if (end - begin >= (1ull << 32)) return fail(ctx, VSC_ERR_RANGE, "vsc_search_select: more than 2^32 selected hits in a block of 64 reads");
        if (end > begin) f.segs.push_back(SortSeg{begin, begin, begin, (uint32_t)(end - begin), f.guide_base + q * (uint32_t)kRegionReads});
    }
    f.n = n_surv;
    f.cap = n_surv;
    if (n_surv == 0) return VSC_OK;
    VSC_HIP(ctx, ctx->sel_keys.ensure(n_cand * sizeof(uint64_t)));
    VSC_HIP(ctx, ctx->sel_masks.ensure(n_cand * sizeof(uint32_t)));
    a.cand_key = (uint64_t *)ctx->sel_keys.p;
    a.cand_mask = (uint32_t *)ctx->sel_masks.p;
    a.out = (uint64_t *)ctx->keys_a.p;  // (read for the last time by the compaction, which the stream runs first)
    VSC_HIP(ctx, hipMemcpyAsync(d_off, f.sel_off.data(), f.sel_off.size() * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    VSC_HIP(ctx, launch_select_compact(a, st));
    VSC_HIP(ctx, launch_select_resolve(a, st));
    return VSC_OK;
}

// The excluded loci of vsc_search_summary / vsc_search_select (`who`) as the records carry them - strand << 32 | global
// position, ~0: none - in excl (left empty without loci or reads).
int excluded_loci(vsc_ctx *ctx, const vsc_genome *genome, const vsc_locus *exclude, uint32_t n_guides, const char *who, std::vector<uint64_t> &excl)
{
    if (!exclude || !n_guides) return VSC_OK;
    std::vector<uint32_t> off(genome->n_contigs), end(genome->n_contigs);
    if (genome->n_contigs) {
        VSC_HIP(ctx, hipMemcpy(off.data(), genome->d_contig_off, off.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        VSC_HIP(ctx, hipMemcpy(end.data(), genome->d_contig_end, end.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    excl.assign(n_guides, ~0ull);
    for (uint32_t i = 0; i < n_guides; ++i) {
        const vsc_locus &l = exclude[i];
        if (l.contig == UINT32_MAX) continue;
        if (l.contig >= genome->n_contigs || l.strand > 1)
            return fail_in(ctx, VSC_ERR_INVALID, who, "excluded locus outside the genome's contigs or strands");
        if (l.pos >= end[l.contig] - off[l.contig]) continue;  // no window starts there: nothing to exclude
        excl[i] = (uint64_t)l.strand << 32 | (off[l.contig] + l.pos);
    }
    return VSC_OK;
}

// the zeroed rows (if wanted) and the excluded loci of a call on the device
int upload_summary_state(vsc_ctx *ctx, uint32_t n_guides, bool rows, const std::vector<uint64_t> &excl, bool rows_in = false)
{
    if (!n_guides) return VSC_OK;
    if (rows) {
        const size_t row_bytes = (size_t)n_guides * sizeof(vsc_guide_summary);
        VSC_HIP(ctx, ctx->sum_rows.ensure(row_bytes));
        VSC_HIP(ctx, hipMemsetAsync(ctx->sum_rows.p, 0, row_bytes, ctx->stream));
        if (rows_in) {
            VSC_HIP(ctx, ctx->sum_rows_in.ensure(row_bytes));
            VSC_HIP(ctx, hipMemsetAsync(ctx->sum_rows_in.p, 0, row_bytes, ctx->stream));
        }
    }
    if (!excl.empty()) {
        VSC_HIP(ctx, ctx->sum_excl.ensure(excl.size() * sizeof(uint64_t)));
        VSC_HIP(ctx, hipMemcpyAsync(ctx->sum_excl.p, excl.data(), excl.size() * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
    }
    return VSC_OK;
}

// The device copy of `regions` on this context: the context keeps the copy of the regions it used last, keyed by their serial
// number; another set is uploaded over it on the context's stream.
int upload_regions(vsc_ctx *ctx, const vsc_regions *regions, RegionsView &dev)
{
    const size_t n = regions->start.size(), cls_at = (2 * n * sizeof(uint32_t) + 255) / 256 * 256;
    if (ctx->regions_serial != regions->serial) {
        ctx->regions_serial = 0;
        VSC_HIP(ctx, ctx->regions_buf.ensure(cls_at + regions->cls.size() * sizeof(uint32_t)));
        char *p = (char *)ctx->regions_buf.p;
        if (n) {
            VSC_HIP(ctx, hipMemcpyAsync(p, regions->start.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
            VSC_HIP(ctx, hipMemcpyAsync(p + n * sizeof(uint32_t), regions->end_max.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        }
        VSC_HIP(ctx, hipMemcpyAsync(p + cls_at, regions->cls.data(), regions->cls.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (the caller may free the regions as soon as its call returns)
        ctx->regions_serial = regions->serial;
    }
    const char *p = (const char *)ctx->regions_buf.p;
    dev = regions->view();
    dev.start = (const uint32_t *)p;
    dev.end_max = (const uint32_t *)p + n;
    dev.cls = (const uint32_t *)(p + cls_at);
    return VSC_OK;
}

// upload_regions for a call that takes a genome (`who`: the caller, for error texts): the regions must have been built for
// the genome's contig table.
int resident_regions(vsc_ctx *ctx, const vsc_genome *genome, const vsc_regions *regions, const char *who, RegionsView &dev)
{
    bool same = regions->contig_off.size() == genome->n_contigs;
    for (uint32_t c = 0; same && c < genome->n_contigs; ++c)  // (the genome's host copy of its table: no device read per call)
        same = genome->h_contig_off[c] == regions->contig_off[c] && genome->h_contig_end[c] - genome->h_contig_off[c] == regions->contig_len[c];
    if (!same) return fail_in(ctx, VSC_ERR_INVALID, who, "the regions were built for another contig table");
    return upload_regions(ctx, regions, dev);
}

// What a kernel locates with, resident on ctx's device: the regions' copy the sinks use (start[], class table), beside it the
// label structure - end[], index[], up[], the contig offsets and lengths the regions were built for, in one buffer keyed by
// the regions' serial number as regions_buf is.  Fills a.reg, a.loc and the contig table of `a` (locate_records below, and
// the first kernel of vsc_*_pick).
int resident_locate(vsc_ctx *ctx, const vsc_regions *regions, LocateArgs &a, const char *who)
{
    if (!regions->has_locate) return fail_in(ctx, VSC_ERR_RANGE, who, "the regions hold more intervals than a 32-bit label can number");
    VSC_HIP(ctx, hipSetDevice(ctx->device));
    const int urc = upload_regions(ctx, regions, a.reg);
    if (urc != VSC_OK) return urc;
    const size_t m = regions->loc_end.size(), nc = regions->contig_off.size();
    if (ctx->locate_serial != regions->serial) {
        ctx->locate_serial = 0;
        VSC_HIP(ctx, ctx->locate_buf.ensure((3 * m + 2 * nc + 1) * sizeof(uint32_t)));  // (+ 1: never empty)
        uint32_t *p = (uint32_t *)ctx->locate_buf.p;
        if (m) {
            VSC_HIP(ctx, hipMemcpyAsync(p, regions->loc_end.data(), m * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
            VSC_HIP(ctx, hipMemcpyAsync(p + m, regions->loc_index.data(), m * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
            VSC_HIP(ctx, hipMemcpyAsync(p + 2 * m, regions->loc_up.data(), m * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        }
        if (nc) {
            VSC_HIP(ctx, hipMemcpyAsync(p + 3 * m, regions->contig_off.data(), nc * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
            VSC_HIP(ctx, hipMemcpyAsync(p + 3 * m + nc, regions->contig_len.data(), nc * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        }
        VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (the caller may free the regions as soon as its call returns)
        ctx->locate_serial = regions->serial;
    }
    const uint32_t *p = (const uint32_t *)ctx->locate_buf.p;
    a.loc = LocateView{p, p + m, p + 2 * m};
    a.contig_off = p + 3 * m;
    a.contig_len = p + 3 * m + nc;
    a.n_contigs = (uint32_t)nc;
    return VSC_OK;
}

// The labels of n 16-byte records on ctx's device (vsc_hit or vsc_locus) into host memory: the tables resident, then
// locate_kernel and one copy back.  The context's timing is left as it is.
int locate_records(vsc_ctx *ctx, const vsc_regions *regions, const void *records, uint64_t n, bool hit_records, uint32_t *labels,
                   const char *who)
{
    ctx->err.clear();
    HostTimer lap;
    LocateArgs a{};
    const int rrc = resident_locate(ctx, regions, a, who);
    if (rrc != VSC_OK) return rrc;
    lap.lap("locate: tables resident");
    a.records = (const uint4 *)records;
    a.n = n;
    VSC_HIP(ctx, ctx->locate_out.ensure(n * sizeof(uint32_t)));
    a.labels = (uint32_t *)ctx->locate_out.p;
    VSC_HIP(ctx, launch_locate(a, hit_records, ctx->n_cus, ctx->stream));
    if (lap.on) {
        VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        lap.lap("locate: kernel");
    }
    VSC_HIP(ctx, hipMemcpyAsync(labels, a.labels, n * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    lap.lap("locate: labels to the host");
    return VSC_OK;
}

// common front end of vsc_search / vsc_search_stream: argument checks, choice of the algorithm (t->algorithm), index
int search_setup(vsc_ctx *ctx, const vsc_genome *genome, const uint64_t *guides, uint32_t n_guides,
                 const vsc_search_params *params, const char *who, vsc_timing *t)
{
    ctx->err.clear();
    if (!genome || !params || (n_guides && !guides)) return fail_in(ctx, VSC_ERR_INVALID, who, "null argument");
    if (genome->ctx != ctx) return fail_in(ctx, VSC_ERR_INVALID, who, "genome belongs to another context");
    if (params->max_mismatches > VSC_MAX_MISMATCHES)  // read_mapping/bidir_mapping.cpp:234-238
        return fail(ctx, VSC_ERR_INVALID, "Maximum number of mismatches must lie between 0 and 8.");
    if (params->algorithm > VSC_ALGO_SEED) return fail_in(ctx, VSC_ERR_INVALID, who, "unknown algorithm");
    if (n_guides >= (1u << 31)) return fail_in(ctx, VSC_ERR_RANGE, who, "too many reads");
    VSC_HIP(ctx, hipSetDevice(ctx->device));
    *t = vsc_timing{};
    t->index_ms = ctx->timing.index_ms;
    const double own_bases = (double)genome->n_tiles * kTileBases;
    int algo = params->algorithm;
    if (algo == VSC_ALGO_AUTO) {
        // the index costs about as much as scanning a few hundred reads; it pays for itself when it is
        // already there or when the search is big enough
        const bool worth_building = (double)n_guides * own_bases >= 2.0e10;
        algo = (index_matches(genome, params) || worth_building) ? VSC_ALGO_SEED : VSC_ALGO_SCAN;
    }
    if (n_guides && algo == VSC_ALGO_SEED && !index_matches(genome, params)) {
        std::string why;
        hipError_t e = build_index(ctx, const_cast<vsc_genome *>(genome), params, &why);
        if (e != hipSuccess) {
            if (params->algorithm == VSC_ALGO_SEED || why.empty())
                return fail(ctx, e == hipErrorOutOfMemory ? VSC_ERR_NOMEM : VSC_ERR_DEVICE,
                            why.empty() ? "vsc_search: building the seed index" : why.c_str(), why.empty() ? e : hipSuccess);
            algo = VSC_ALGO_SCAN;  // auto mode: a genome too large for the index is still searchable
        } else {
            t->index_ms = genome->index_ms;
        }
    }
    t->algorithm = (uint32_t)algo;
    return VSC_OK;
}

// What a search call wants from every pass (run_search).
enum class Records { kNone, kAccumulate, kPerBatch };  // no result; one result over all passes; one per batch, handed to `deliver`
struct SearchPlan {
    SearchPlan(const char *who_, Records records_, vsc_hits **out_ = nullptr) : who(who_), records(records_), out(out_) {}
    const char *who;                       // the entry point, for error texts
    Records records;
    vsc_hits **out;                        // kAccumulate: where the result goes
    const vsc_locus *exclude = nullptr;    // per read (null: none)
    const vsc_regions *regions = nullptr;  // what rows_in counts in and the filter selects by
    vsc_guide_summary *rows = nullptr, *rows_in = nullptr;  // the row sets to write, in host memory (null: not wanted)
    bool selects = false;                  // the call takes a vsc_select: checked after search_setup, as the call always did
    const vsc_select *select = nullptr;
    const vsc_region_filter *filter = nullptr;  // (its fields have been checked)
    uint32_t batch_reads = 0;              // kPerBatch: reads per batch (0 or too many: kMaxPassReads)
    // kPerBatch: deliver(deliver_self, hits, first read, reads, t) hands a batch on; what it adds to t.score_ms stays in the call's timing
    int (*deliver)(void *, vsc_hits *, uint32_t, uint32_t, vsc_timing &) = nullptr;
    void *deliver_self = nullptr;
    bool keep_bases = false;  // the seed search keeps the sites' bases: the hits' feature rows are written with the records
    // vsc_search_*_classified: the forest and the activities (checked after search_setup), the votes rows to write (null: not
    // wanted), the selection by votes (select_votes != null: the call takes one)
    bool classifies = false;
    const vsc_classify *classify = nullptr;
    vsc_guide_votes *votes_rows = nullptr;
    bool selects_votes = false;
    const vsc_select_votes *select_votes = nullptr;
    // vsc_search_*_table: the score table (checked after search_setup), the table rows to write (null: not wanted); a call
    // that selects (`selects`) then selects by the table score
    bool tables = false;
    const vsc_score_table *table = nullptr;
    vsc_guide_table_row *table_rows = nullptr;
};

// The one pass loop behind every search entry point: search_setup; the call's state on the device (excluded loci, regions,
// zeroed rows); per pass of at most kMaxPassReads reads find_pass, then what the plan asks for - summarize_pass, select_pass,
// sort_pass - the read index being the major sort key, so that the passes' records simply follow each other; the rows and the
// timing at the end.
int run_search(vsc_ctx *ctx, const vsc_genome *genome, const uint64_t *guides, uint32_t n_guides, const vsc_search_params *params,
               const SearchPlan &p)
{
    vsc_timing t{};
    int rc = search_setup(ctx, genome, guides, n_guides, params, p.who, &t);
    if (rc != VSC_OK) return rc;
    const bool per_batch = p.records == Records::kPerBatch;
    if (per_batch && !p.deliver) return fail_in(ctx, VSC_ERR_INVALID, p.who, "null callback");
    if (p.selects && !p.select) return fail_in(ctx, VSC_ERR_INVALID, p.who, "null argument");
    if (p.selects && (p.select->reserved[0] || p.select->reserved[1])) return fail_in(ctx, VSC_ERR_INVALID, p.who, "reserved fields must be 0");
    if (p.tables && !p.table) return fail_in(ctx, VSC_ERR_INVALID, p.who, "null argument");
    if (p.classifies) {
        if (!p.classify || !p.classify->model || (n_guides && !p.classify->guide_activity) || (p.selects_votes && !p.select_votes))
            return fail_in(ctx, VSC_ERR_INVALID, p.who, "null argument");
        if (p.classify->reserved[0] || p.classify->reserved[1] || (p.select_votes && (p.select_votes->reserved[0] || p.select_votes->reserved[1])))
            return fail_in(ctx, VSC_ERR_INVALID, p.who, "reserved fields must be 0");
        if (p.classify->model->n_trees == 0 || p.classify->model->n_trees > 65535u)
            return fail_in(ctx, VSC_ERR_INVALID, p.who, "a forest of 0 trees, or of more than the 16-bit votes hold");
    }
    std::vector<uint64_t> excl;
    if ((rc = excluded_loci(ctx, genome, p.exclude, n_guides, p.who, excl)) != VSC_OK) return rc;
    RegionsView reg{};
    if (p.regions && (rc = resident_regions(ctx, genome, p.regions, p.who, reg)) != VSC_OK) return rc;
    // the summary kernel writes both sets of rows or the plain one: rows_in alone takes the plain rows along
    const bool rows = p.rows || p.rows_in;
    if ((rc = upload_summary_state(ctx, n_guides, rows, excl, p.rows_in != nullptr)) != VSC_OK) return rc;
    // nothing to decide: the records go to the sort as the search hands them over
    vsc_select by_votes{};  // the selection by votes in select_pass's terms
    if (p.select_votes) {
        by_votes.top_k = p.select_votes->top_k;
        by_votes.min_score = p.select_votes->min_votes;
    }
    const vsc_select *const select = p.select_votes ? &by_votes : p.select;
    const bool selecting = select && (select->top_k || select->min_score || !excl.empty() || p.filter);
    // the classifier runs when something reads its votes: the rows, or a selection that decides anything
    const bool classifying = p.classifies && n_guides && (p.votes_rows || selecting);
    if (classifying) {
        if ((rc = prepare_forest(ctx, p.classify->model, p.who)) != VSC_OK) return rc;
        if ((rc = resident_ranks(ctx, p.classify->guide_activity, n_guides)) != VSC_OK) return rc;
        VSC_HIP(ctx, ensure_hl(ctx, genome));
        if (p.votes_rows) {
            VSC_HIP(ctx, ctx->votes_rows.ensure((size_t)n_guides * sizeof(vsc_guide_votes)));
            VSC_HIP(ctx, hipMemsetAsync(ctx->votes_rows.p, 0, (size_t)n_guides * sizeof(vsc_guide_votes), ctx->stream));
        }
    }
    const uint32_t vote_trees = classifying && p.select_votes ? p.classify->model->n_trees : 0u;
    // the table scores are computed when something reads them: the rows, or a selection that decides anything
    const bool tabling = p.tables && n_guides && (p.table_rows || selecting);
    if (tabling) {
        if ((rc = resident_table(ctx, p.table)) != VSC_OK) return rc;
        VSC_HIP(ctx, ensure_hl(ctx, genome));
        if (p.table_rows) {
            VSC_HIP(ctx, ctx->table_rows.ensure((size_t)n_guides * sizeof(vsc_guide_table_row)));
            VSC_HIP(ctx, hipMemsetAsync(ctx->table_rows.p, 0, (size_t)n_guides * sizeof(vsc_guide_table_row), ctx->stream));
        }
    }
    const uint32_t step = per_batch && p.batch_reads && p.batch_reads <= (uint32_t)kMaxPassReads ? p.batch_reads : (uint32_t)kMaxPassReads;

    std::unique_ptr<vsc_hits, int (*)(vsc_hits *)> hits(nullptr, vsc_hits_free);
    uint64_t used = 0;  // records in `hits`
    auto fresh_result = [&]() {
        hits.reset(new (std::nothrow) vsc_hits());
        if (!hits) return fail_in(ctx, VSC_ERR_NOMEM, p.who, "out of host memory");
        hits->ctx = ctx;
        used = 0;
        return VSC_OK;
    };
    auto seal_result = [&]() {
        hits->n = used;
        if (used == 0) hits->host_valid = true;
    };
    if (p.records == Records::kAccumulate && (rc = fresh_result()) != VSC_OK) return rc;
    for (uint32_t first = 0; first < n_guides; first += step) {
        const uint32_t count = std::min<uint32_t>(step, n_guides - first);
        if (per_batch && (rc = fresh_result()) != VSC_OK) return rc;
        // (an accumulated result grows to its expected final size at once)
        const uint64_t projected = !per_batch && first ? (uint64_t)((double)used / first * n_guides * 1.02) + 4096 : 0;
        PassFound f;
        const bool votes_rows = classifying && p.votes_rows;
        const bool table_rows = tabling && p.table_rows;
        // (the sort is the records' only reader: no classifier, no table, no rows, no selection walks them where the search left them)
        const bool sort_only = p.records != Records::kNone && !classifying && !tabling && !rows && !selecting;
        rc = find_pass(ctx, genome, guides + first, count, first, params, p.keep_bases && t.algorithm == VSC_ALGO_SEED, sort_only, t, f);
        if (rc == VSC_OK && classifying) rc = classify_pass(ctx, genome, f, count, !excl.empty());
        if (rc == VSC_OK && tabling) rc = table_score_pass(ctx, genome, f, count, !excl.empty());
        // (with another sink to follow, the summary leaves the end of the pass - and finalize_ms - to the sort)
        if (rc == VSC_OK && rows)
            rc = summarize_pass(ctx, f, !excl.empty(), t, p.records == Records::kNone && !votes_rows && !table_rows, p.rows_in ? &reg : nullptr);
        if (rc == VSC_OK && votes_rows) rc = votes_summary_pass(ctx, f, count, !excl.empty(), t, !rows, p.records == Records::kNone);
        if (rc == VSC_OK && table_rows) rc = table_summary_pass(ctx, f, count, !excl.empty(), t, !rows, p.records == Records::kNone);
        if (rc == VSC_OK && selecting)
            rc = select_pass(ctx, f, count, *select, !excl.empty(), p.filter ? &reg : nullptr, p.filter ? p.filter->scope : 0u, vote_trees,
                             tabling ? 1u : 0u);
        if (rc == VSC_OK && p.records != Records::kNone) rc = sort_pass(ctx, genome, f, hits.get(), used, projected, t);
        if (rc != VSC_OK) return rc;
        if (f.classified) {  // (the pass has ended: its stream is idle)
            float ms = 0;
            VSC_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev[kEvClassStart], ctx->ev[kEvClassEnd]));
            t.score_ms += ms;
            if (p.records != Records::kNone) t.sort_ms -= ms;  // (sort_ms spans search end -> sink start: the classifier ran in between)
        }
        used += f.n;
        if (per_batch) {
            seal_result();
            ctx->timing = t;
            ctx->timing.score_ms = 0;
            rc = p.deliver(p.deliver_self, hits.get(), first, count, t);
            if (rc != VSC_OK && ctx->err.empty()) (void)fail_in(ctx, rc, p.who, "the batch callback failed");
            hits.reset();  // (before the next batch: its records go into this one's storage)
            if (rc != VSC_OK) return rc;
        }
    }
    if (rows && n_guides) {
        const size_t row_bytes = (size_t)n_guides * sizeof(vsc_guide_summary);
        if (p.rows) VSC_HIP(ctx, hipMemcpyAsync(p.rows, ctx->sum_rows.p, row_bytes, hipMemcpyDeviceToHost, ctx->stream));
        if (p.rows_in) VSC_HIP(ctx, hipMemcpyAsync(p.rows_in, ctx->sum_rows_in.p, row_bytes, hipMemcpyDeviceToHost, ctx->stream));
        VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    if (classifying && p.votes_rows) {
        VSC_HIP(ctx, hipMemcpyAsync(p.votes_rows, ctx->votes_rows.p, (size_t)n_guides * sizeof(vsc_guide_votes), hipMemcpyDeviceToHost, ctx->stream));
        VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    if (tabling && p.table_rows) {
        VSC_HIP(ctx, hipMemcpyAsync(p.table_rows, ctx->table_rows.p, (size_t)n_guides * sizeof(vsc_guide_table_row), hipMemcpyDeviceToHost, ctx->stream));
        VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    ctx->timing = t;
    if (p.records == Records::kAccumulate) {
        seal_result();
        *p.out = hits.release();
    }
    return VSC_OK;
}

// vsc_search_summary (regions == null) and vsc_search_summary_regions (`who`)
int search_summary(vsc_ctx *ctx, const vsc_genome *genome, const uint64_t *guides, uint32_t n_guides, const vsc_search_params *params,
                   const vsc_locus *exclude, const vsc_regions *regions, vsc_guide_summary *out, vsc_guide_summary *out_in, const char *who)
{
    return guarded(ctx, [&]() -> int {
    if (!ctx) return VSC_ERR_INVALID;
    if (n_guides && !out) return fail_in(ctx, VSC_ERR_INVALID, who, "null argument");
    SearchPlan p(who, Records::kNone);
    p.exclude = exclude;
    p.regions = regions;
    p.rows = out;
    p.rows_in = out_in;
    return run_search(ctx, genome, guides, n_guides, params, p);
    });
}

// vsc_search_select (filter == null) and vsc_search_select_regions (`who`; the filter's fields have been checked)
int search_select(vsc_ctx *ctx, const vsc_genome *genome, const uint64_t *guides, uint32_t n_guides, const vsc_search_params *params,
                  const vsc_select *select, const vsc_region_filter *filter, const vsc_locus *exclude, vsc_guide_summary *summary,
                  vsc_guide_summary *summary_in, vsc_hits **out, const char *who)
{
    return guarded(ctx, [&]() -> int {
    if (!ctx || !out) return VSC_ERR_INVALID;
    *out = nullptr;
    SearchPlan p(who, Records::kAccumulate, out);
    p.exclude = exclude;
    p.regions = filter ? filter->regions : nullptr;
    p.rows = summary;
    p.rows_in = summary_in;
    p.selects = true;
    p.select = select;
    p.filter = filter;
    return run_search(ctx, genome, guides, n_guides, params, p);
    });
}

// vsc_search_stream / vsc_search_stream_rows (`who`): one pass per batch into a result of its own, which deliver hands on.
// rows: the seed search writes the hits' feature rows with the records.
template <class Deliver>
int search_stream(vsc_ctx *ctx, const vsc_genome *genome, const uint64_t *guides, uint32_t n_guides, const vsc_search_params *params,
                  uint32_t batch_reads, bool rows, const char *who, bool have_callback, Deliver deliver)
{
    return guarded(ctx, [&]() -> int {
    if (!ctx) return VSC_ERR_INVALID;
    SearchPlan p(who, Records::kPerBatch);
    p.batch_reads = batch_reads;
    p.keep_bases = rows;
    if (have_callback) {
        p.deliver = [](void *self, vsc_hits *hits, uint32_t first, uint32_t count, vsc_timing &t) { return (*(Deliver *)self)(hits, first, count, t); };
        p.deliver_self = &deliver;
    }
    return run_search(ctx, genome, guides, n_guides, params, p);
    });
}


// ---- variant-aware screen (vsc_hits_variants, vsc_search_summary_variants) -------------------------------------
// The device copy of `map` on this context - windows (n + 1 entries), then variants, in one buffer keyed by the map's serial
// number as regions_buf is - and the checks every call makes: the map was built for win_genome's contig table, the excluded
// loci lie in the reference's.  Fills a.map, the planes, the contig table and a.exclude / a.n_guides.
int resident_variant_map(vsc_ctx *ctx, const vsc_genome *win_genome, const vsc_variant_map *map, const vsc_locus *exclude, uint32_t n_guides,
                         const char *who, VariantArgs &a)
{
    if (win_genome->ctx != ctx) return fail_in(ctx, VSC_ERR_INVALID, who, "genome belongs to another context");
    const uint32_t n_win = (uint32_t)(map->win.size() - 1);
    // (both objects are immutable and the serial is process-wide: a pair that has passed need not be walked again - millions of
    // windows per call otherwise)
    bool same = win_genome->checked_map_serial == map->serial || n_win == win_genome->n_contigs;
    for (uint32_t c = 0; same && win_genome->checked_map_serial != map->serial && c < n_win; ++c)
        same = win_genome->h_contig_end[c] - win_genome->h_contig_off[c] == map->win_len[c];
    if (!same) return fail_in(ctx, VSC_ERR_INVALID, who, "the variant map was built for another window genome");
    win_genome->checked_map_serial = map->serial;
    for (uint32_t i = 0; exclude && i < n_guides; ++i)
        if ((exclude[i].contig != UINT32_MAX && exclude[i].contig >= map->ref_contigs.size()) || exclude[i].strand > 1)
            return fail_in(ctx, VSC_ERR_INVALID, who, "excluded locus outside the reference's contigs or strands");
    VSC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t win_bytes = map->win.size() * sizeof(VarWindow), var_bytes = map->var.size() * sizeof(VarEntry);
    if (ctx->varmap_serial != map->serial) {
        ctx->varmap_serial = 0;
        VSC_HIP(ctx, ctx->varmap_buf.ensure(win_bytes + var_bytes));
        VSC_HIP(ctx, hipMemcpyAsync(ctx->varmap_buf.p, map->win.data(), win_bytes, hipMemcpyHostToDevice, ctx->stream));
        if (var_bytes)
            VSC_HIP(ctx, hipMemcpyAsync((char *)ctx->varmap_buf.p + win_bytes, map->var.data(), var_bytes, hipMemcpyHostToDevice, ctx->stream));
        VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (the caller may free the map as soon as its call returns)
        ctx->varmap_serial = map->serial;
    }
    a.map = VarMapView{(const VarWindow *)ctx->varmap_buf.p, (const VarEntry *)((const char *)ctx->varmap_buf.p + win_bytes), n_win,
                       (uint32_t)map->var.size()};
    a.hi = win_genome->d_hi;
    a.lo = win_genome->d_lo;
    a.first_pos = (uint32_t)(win_genome->first_word * 32);
    a.n_plane_words = win_genome->dev_words;
    a.contig_off = win_genome->d_contig_off;
    a.contig_end = win_genome->d_contig_end;
    a.n_guides = n_guides;
    a.exclude = nullptr;
    if (exclude && n_guides) {
        VSC_HIP(ctx, ctx->var_excl.ensure((size_t)n_guides * sizeof(vsc_locus)));
        VSC_HIP(ctx, hipMemcpyAsync(ctx->var_excl.p, exclude, (size_t)n_guides * sizeof(vsc_locus), hipMemcpyHostToDevice, ctx->stream));
        a.exclude = (const uint4 *)ctx->var_excl.p;
    }
    return VSC_OK;
}

// The call's state on the device: the error flag (its own 256 bytes), then - rows wanted - the zeroed rows over all counted
// records, those over the VAR ones and the duplicate counts.
constexpr size_t kVarStateHead = 256;
int variant_state(vsc_ctx *ctx, uint32_t n_guides, bool rows, VariantArgs &a)
{
    const size_t row_bytes = (size_t)n_guides * sizeof(vsc_guide_summary);
    const size_t bytes = kVarStateHead + (rows ? 2 * row_bytes + (size_t)n_guides * sizeof(uint64_t) : 0);
    VSC_HIP(ctx, ctx->var_state.ensure(bytes));
    VSC_HIP(ctx, hipMemsetAsync(ctx->var_state.p, 0, bytes, ctx->stream));
    char *p = (char *)ctx->var_state.p;
    a.error = (uint32_t *)p;
    if (rows) {
        a.rows_all = (unsigned long long *)(p + kVarStateHead);
        a.rows_var = (unsigned long long *)(p + kVarStateHead + row_bytes);
        a.dups = (unsigned long long *)(p + kVarStateHead + 2 * row_bytes);
    }
    return VSC_OK;
}

// has the kernel met a record outside the map? (after the stream has been waited for)
int variant_error(vsc_ctx *ctx, const VariantArgs &a, const char *who)
{
    uint32_t bad = 0;
    VSC_HIP(ctx, hipMemcpy(&bad, a.error, sizeof bad, hipMemcpyDeviceToHost));
    if (bad) return fail_in(ctx, VSC_ERR_INVALID, who, "a record lies outside the variant map, its window or the guides");
    return VSC_OK;
}

// the planes and the contig table of a resident genome, as the kernels of the enumerations and of the rounds read them
template <class Args> void bind_genome(Args &a, const vsc_genome *genome)
{
    a.hi = genome->d_hi;
    a.lo = genome->d_lo;
    a.nm = genome->d_nm;
    a.first_pos = (uint32_t)(genome->first_word * 32);
    a.contig_off = genome->d_contig_off;
    a.contig_end = genome->d_contig_end;
    a.n_contigs = genome->n_contigs;
}

// ---- the result objects of the enumerations and of the rounds (vsc::GuideList, vsc::RecordList) ---------------------------
template <class Guides> int guide_list_data(Guides *guides, const uint64_t **codes, const vsc_locus **loci)
{
    if (!guides) return VSC_ERR_INVALID;
    return guarded(guides->ctx, [&]() -> int {
    if (!guides->host_valid) {
        vsc_ctx *ctx = guides->ctx;
        guides->codes.resize(guides->n);
        guides->loci.resize(guides->n);
        VSC_HIP(ctx, hipSetDevice(ctx->device));
        VSC_HIP(ctx, hipMemcpyAsync(guides->codes.data(), guides->storage.p, guides->n * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
        VSC_HIP(ctx, hipMemcpyAsync(guides->loci.data(), (const char *)guides->storage.p + guides->loci_at, guides->n * sizeof(vsc_locus),
                                    hipMemcpyDeviceToHost, ctx->stream));
        VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        guides->host_valid = true;
    }
    if (codes) *codes = guides->codes.data();
    if (loci) *loci = guides->loci.data();
    return VSC_OK;
    });
}

int guide_list_data_dev(const GuideList *guides, const void **codes_dev, const void **loci_dev)
{
    if (!guides) return VSC_ERR_INVALID;
    const bool dev = guides->ctx && guides->n && guides->storage.p;  // (storage is a context's: no ctx, no storage)
    if (codes_dev) *codes_dev = dev ? guides->storage.p : nullptr;
    if (loci_dev) *loci_dev = dev ? (const char *)guides->storage.p + guides->loci_at : nullptr;
    return VSC_OK;
}

template <class Hits> int record_list_data(Hits *hits, const typename Hits::record **out)
{
    if (!hits || !out) return VSC_ERR_INVALID;
    return guarded(hits->ctx, [&]() -> int {
    if (!hits->host_valid) {
        vsc_ctx *ctx = hits->ctx;
        hits->host.resize(hits->n);
        VSC_HIP(ctx, hipSetDevice(ctx->device));
        VSC_HIP(ctx, hipMemcpyAsync(hits->host.data(), hits->storage.p, hits->n * sizeof(typename Hits::record), hipMemcpyDeviceToHost, ctx->stream));
        VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        hits->host_valid = true;
    }
    *out = hits->host.data();
    return VSC_OK;
    });
}

template <class Rec> const void *record_list_data_dev(const RecordList<Rec> *hits) { return hits && hits->n ? hits->storage.p : nullptr; }

// frees a GuideList or a RecordList by its handle type (the objects have no virtual destructor)
template <class Object> int object_free(Object *o)
{
    if (!o) return VSC_OK;
    if (o->ctx && o->storage.p) {
        (void)hipSetDevice(o->ctx->device);
        o->storage.release();
    }
    delete o;
    return VSC_OK;
}

// ---- the two passes of the enumerations ----------------------------------------------------------------
// Count pass over the work list, exclusive scan of the per-tile counts, one 8-byte read-back (the total: it sizes the result
// and is what max_guides is checked against), write pass into the result's own arrays.  The caller has filled `a` but for
// the work list, the counts, the offsets and the result; work == null: tiles 0 .. n_work - 1.  `tail` is a table of the
// caller's that goes to the device behind the scratch of the passes.  launch(d_tail, total, write) starts a pass.
template <class Guides, class Args, class Launch>
int run_enumeration(vsc_ctx *ctx, const char *fn, Args &a, const std::vector<uint32_t> *work, uint32_t n_work, const void *tail,
                    size_t tail_bytes, uint64_t max_guides, Guides **out, Launch launch)
{
    vsc_timing t{};
    t.index_ms = ctx->timing.index_ms;
    std::unique_ptr<Guides, int (*)(Guides *)> g(new (std::nothrow) Guides(), object_free<Guides>);
    if (!g) return fail_in(ctx, VSC_ERR_NOMEM, fn, "out of host memory");
    g->ctx = ctx;
    unsigned long long total = 0;
    if (n_work) {
        // scratch: [work list][counts][offsets][tail], 256-byte aligned parts
        const size_t list_bytes = round256((size_t)n_work * sizeof(uint32_t));
        const size_t off_bytes = round256(((size_t)n_work + 1) * sizeof(unsigned long long));
        VSC_HIP(ctx, ctx->enum_tabs.ensure(2 * list_bytes + off_bytes + tail_bytes));
        char *base = (char *)ctx->enum_tabs.p;
        unsigned long long *d_off = (unsigned long long *)(base + 2 * list_bytes);
        char *d_tail = tail_bytes ? base + 2 * list_bytes + off_bytes : nullptr;
        if (work) {
            VSC_HIP(ctx, hipMemcpyAsync(base, work->data(), (size_t)n_work * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
            a.work = (const uint32_t *)base;
        }
        if (tail_bytes) VSC_HIP(ctx, hipMemcpyAsync(d_tail, tail, tail_bytes, hipMemcpyHostToDevice, ctx->stream));
        a.n_work = n_work;
        a.tile_count = (uint32_t *)(base + list_bytes);
        a.tile_off = d_off;
        VSC_HIP(ctx, hipEventRecord(ctx->ev[kEvStageStart], ctx->stream));
        VSC_HIP(ctx, launch(d_tail, total, false));
        VSC_HIP(ctx, launch_enum_scan(a.tile_count, n_work, d_off, ctx->stream));
        VSC_HIP(ctx, hipEventRecord(ctx->ev[kEvStageEnd], ctx->stream));
        VSC_HIP(ctx, hipMemcpyAsync(&total, d_off + n_work, sizeof total, hipMemcpyDeviceToHost, ctx->stream));
        VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (also: the work list and the tail are the caller's vectors)
        float ms = 0;
        VSC_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev[kEvStageStart], ctx->ev[kEvStageEnd]));
        t.scan_ms += ms;
        t.genome_bytes += (uint64_t)n_work * kTileWords * 3 * sizeof(uint32_t);
        t.passes = 1;
        if (max_guides && total > max_guides) {
            char msg[160];
            std::snprintf(msg, sizeof msg, "%s: %llu candidates exceed max_guides = %llu", fn, total, (unsigned long long)max_guides);
            return fail(ctx, VSC_ERR_RANGE, msg);
        }
        if (total) {
            g->loci_at = round256((size_t)total * sizeof(uint64_t));
            VSC_HIP(ctx, g->storage.ensure(g->loci_at + (size_t)total * sizeof(vsc_locus)));
            a.codes = (unsigned long long *)g->storage.p;
            a.loci = (uint4 *)((char *)g->storage.p + g->loci_at);
            VSC_HIP(ctx, hipEventRecord(ctx->ev[kEvStage2Start], ctx->stream));
            VSC_HIP(ctx, launch(d_tail, total, true));
            VSC_HIP(ctx, hipEventRecord(ctx->ev[kEvStage2End], ctx->stream));
            VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));
            VSC_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev[kEvStage2Start], ctx->ev[kEvStage2End]));
            t.scan_ms += ms;
            t.genome_bytes += (uint64_t)n_work * kTileWords * 3 * sizeof(uint32_t);
            t.passes = 2;
        }
    }
    g->n = total;
    if (total == 0) g->host_valid = true;
    t.total_ms = t.scan_ms;
    t.sites = total;
    ctx->timing = t;
    *out = g.release();
    return VSC_OK;
}

// ---- the rounds of the count / scan / write searches ---------------------------------------------------------
// Per round of `batch` guides: count pass (hits per (guide, strand, tile) cell), sums per 64 cells - and, with two levels,
// per 64 of those, so that the one-workgroup scan sees a 64th of the chunks (at 3 Gbp and 16 guides: 11 000 entries, not
// 730 000) - exclusive scan of the sums, one 8-byte read-back (the round's records), write pass into the round's own buffer.
// The rounds' buffers are consecutive pieces of the result (the order starts with the guide); with more than one round they
// are copied into one array.
static_assert(kPatChunk == kBulgeChunk, "the sums of every round are taken per kBulgeChunk cells");

// What vsc_search_pattern_table adds to the rounds: per record one 32-bit side word behind the records, a second
// set of rows (64-bit words), and - with a selection - a stage behind every round's write pass, which then writes to scratch.
struct RoundsScore {
    unsigned long long *rows;   // host: kPatTableRowWords words per guide (null: not asked for)
    uint32_t top_k, min_score;  // both 0: no selection stage
};

// What a search tells run_rounds about itself.
struct RoundsPlan {
    const char *fn;  // for messages
    uint32_t n_guides, n_tiles;
    uint32_t batch;       // guides per round
    DeviceBuf *pool;      // the context's scratch of the search's family
    uint32_t levels;      // 1: offsets per chunk of 64 cells; 2: per group of 64 chunks
    uint32_t row_words;   // 32-bit words of a guide's row
    uint64_t max_hits;    // 0: no cap
    const RoundsScore *score = nullptr;  // the scored pattern search alone
};

// What the launches of a round are bound to.
struct Round {
    uint32_t g0, n;                 // guides [g0, g0 + n) of the call
    const uint4 *guides;            // the round's table, as the search staged it
    uint32_t *count;                // hits per cell
    const uint32_t *chunk_sum;      // two levels: hits per chunk
    const unsigned long long *off;  // hits of all cells before a chunk (one level) or a group (two)
    unsigned long long *sites;
    uint32_t *rows;                 // null: no rows are asked for
    void *records;                  // write pass: the round's piece (null: it has no records)
    unsigned long long n_records;
    uint32_t *side;                 // a scored search: the side words of the round's records (null as `records` is)
    unsigned long long *rows64;     // ... and its second rows (null: not asked for)
};

// table_uint4s(n): the uint4s of the table of a round of n guides; stage(g0, n, table): fills that table, zeroed, for guides
// [g0, g0 + n); launch(round, write): the count or the write kernel on the round.
template <class Hits, class Slots, class Stage, class Launch>
int run_rounds(vsc_ctx *ctx, const RoundsPlan &p, Hits **out, uint32_t *rows, Slots table_uint4s, Stage stage, Launch launch)
{
    const size_t rec_bytes = sizeof(typename Hits::record);
    std::unique_ptr<Hits, int (*)(Hits *)> holder(nullptr, object_free<Hits>);
    if (out) {
        holder.reset(new (std::nothrow) Hits());
        if (!holder) return fail_in(ctx, VSC_ERR_NOMEM, p.fn, "out of host memory");
        holder->ctx = ctx;
        holder->host_valid = true;  // (empty until records are written)
        holder->has_side = holder->side_host_valid = p.score != nullptr;
    }
    vsc_timing t{};
    t.index_ms = ctx->timing.index_ms;
    t.algorithm = VSC_ALGO_SCAN;
    const size_t rows_words = (size_t)p.n_guides * p.row_words;
    if (rows) std::memset(rows, 0, rows_words * sizeof(uint32_t));
    unsigned long long *const rows64 = p.score ? p.score->rows : nullptr;
    const size_t rows64_words = rows64 ? (size_t)p.n_guides * kPatTableRowWords : 0;
    if (rows64) std::memset(rows64, 0, rows64_words * sizeof(unsigned long long));
    const bool selecting = p.score && out && (p.score->top_k || p.score->min_score);
    const uint32_t n_guides = p.n_guides, n_tiles = p.n_tiles, batch = p.batch;
    if (n_guides == 0 || n_tiles == 0) {
        t.pairs = 0;
        ctx->timing = t;
        if (out) *out = holder.release();
        return VSC_OK;
    }
    VSC_HIP(ctx, hipSetDevice(ctx->device));
    // scratch, 256-byte aligned parts: [rows of all guides][site counter] | per round: [guides][counts][chunk sums][group sums
    // (two levels)][offsets of the chunks or groups]
    const uint64_t max_cells = (uint64_t)2 * batch * n_tiles;
    const uint64_t max_chunks = (max_cells + kBulgeChunk - 1) / kBulgeChunk;
    if (max_chunks >= (1ull << 32)) return fail_in(ctx, VSC_ERR_RANGE, p.fn, "counter table too large");
    const bool grouped = p.levels == 2;
    const uint64_t max_groups = (max_chunks + kBulgeChunk - 1) / kBulgeChunk;  // the one-workgroup scan takes these, not the chunks
    const size_t rows_bytes = round256(rows_words * sizeof(uint32_t));
    const size_t rows64_bytes = round256(rows64_words * sizeof(unsigned long long)), sel_bytes = selecting ? round256(batch * sizeof(uint4)) : 0;
    const size_t table_bytes = round256((size_t)table_uint4s(batch) * sizeof(uint4));
    const size_t count_bytes = round256((size_t)max_cells * sizeof(uint32_t)), sums_bytes = round256((size_t)max_chunks * sizeof(uint32_t));
    const size_t groups_bytes = grouped ? round256((size_t)max_groups * sizeof(uint32_t)) : 0;
    VSC_HIP(ctx, p.pool->ensure(rows_bytes + 256 + rows64_bytes + sel_bytes + table_bytes + count_bytes + sums_bytes + groups_bytes +
                                (size_t)((grouped ? max_groups : max_chunks) + 1) * sizeof(unsigned long long)));
    char *base = (char *)p.pool->p;
    uint32_t *d_rows = (uint32_t *)base;
    unsigned long long *d_sites = (unsigned long long *)(base + rows_bytes);
    unsigned long long *d_rows64 = (unsigned long long *)(base + rows_bytes + 256);  // (a scored search: zeroed with the rows)
    uint4 *d_sel = (uint4 *)((char *)d_rows64 + rows64_bytes);
    uint4 *d_table = (uint4 *)((char *)d_sel + sel_bytes);
    uint32_t *d_count = (uint32_t *)((char *)d_table + table_bytes);
    uint32_t *d_sums = (uint32_t *)((char *)d_count + count_bytes);
    uint32_t *d_groups = (uint32_t *)((char *)d_sums + sums_bytes);
    unsigned long long *d_off = (unsigned long long *)((char *)d_groups + groups_bytes);
    VSC_HIP(ctx, hipMemsetAsync(base, 0, rows_bytes + 256 + rows64_bytes, ctx->stream));
    Round r{};
    r.rows64 = rows64 ? d_rows64 : nullptr;
    r.guides = d_table;
    r.count = d_count;
    r.chunk_sum = d_sums;
    r.off = d_off;
    r.rows = rows ? d_rows : nullptr;

    std::vector<DeviceBuf> pieces;  // the rounds' records (released on every way out)
    DeviceBuf raw;                  // with a selection: a round's records and side words before it
    struct Release {
        std::vector<DeviceBuf> &v;
        DeviceBuf &raw;
        ~Release()
        {
            for (auto &b : v) b.release();
            raw.release();
        }
    } release{pieces, raw};
    // a piece of n records: the records, then - a scored search - their side words from side_at(n) on
    const size_t side_bytes = p.score ? sizeof(uint32_t) : 0;
    auto side_at = [&](uint64_t n) { return round256((size_t)n * rec_bytes); };
    auto piece_bytes = [&](uint64_t n) { return side_bytes ? side_at(n) + (size_t)n * side_bytes : (size_t)n * rec_bytes; };
    std::vector<uint4> sel_host;
    std::vector<uint64_t> piece_n;
    std::vector<uint4> staged;
    unsigned long long total = 0, found = 0;
    // the count pass of the round that starts at guide g0 (and, for records, the offsets of its cells): found = its records
    auto count_round = [&](uint32_t g0) -> int {
        r.g0 = g0;
        r.n = std::min(batch, n_guides - g0);
        staged.assign(table_uint4s(r.n), make_uint4(0, 0, 0, 0));
        stage(g0, r.n, staged.data());
        VSC_HIP(ctx, hipMemcpyAsync(d_table, staged.data(), staged.size() * sizeof(uint4), hipMemcpyHostToDevice, ctx->stream));
        r.sites = g0 ? d_sites + 1 : d_sites;  // (every round sees the same sites: the first counts them, the others add into a spare word)
        const uint64_t cells = (uint64_t)2 * r.n * n_tiles;
        const uint32_t chunks = (uint32_t)((cells + kBulgeChunk - 1) / kBulgeChunk), groups = (chunks + kBulgeChunk - 1) / kBulgeChunk;
        const uint32_t scanned = grouped ? groups : chunks;
        found = 0;
        VSC_HIP(ctx, hipEventRecord(ctx->ev[kEvStageStart], ctx->stream));
        VSC_HIP(ctx, launch(r, false));
        if (out) {
            VSC_HIP(ctx, launch_bulge_chunk_sums(d_count, cells, d_sums, ctx->stream));
            if (grouped) VSC_HIP(ctx, launch_bulge_chunk_sums(d_sums, chunks, d_groups, ctx->stream));
            VSC_HIP(ctx, launch_enum_scan(grouped ? d_groups : d_sums, scanned, d_off, ctx->stream));
        }
        VSC_HIP(ctx, hipEventRecord(ctx->ev[kEvStageEnd], ctx->stream));
        if (out) VSC_HIP(ctx, hipMemcpyAsync(&found, d_off + scanned, sizeof found, hipMemcpyDeviceToHost, ctx->stream));
        VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (also: `staged` is reused by the next round)
        float ms = 0;
        VSC_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev[kEvStageStart], ctx->ev[kEvStageEnd]));
        t.scan_ms += ms;
        t.genome_bytes += (uint64_t)n_tiles * kTileWords * 3 * sizeof(uint32_t);
        t.passes += 1;
        total += found;
        return VSC_OK;
    };
    for (uint32_t g0 = 0; g0 < n_guides; g0 += batch) {
        int rc = count_round(g0);
        if (rc != VSC_OK) return rc;
        if (!selecting && p.max_hits && total > p.max_hits) {
            // the count the message names is the whole call's: the remaining rounds are counted, nothing more is written
            for (uint32_t h0 = g0 + batch; h0 < n_guides; h0 += batch)
                if ((rc = count_round(h0)) != VSC_OK) return rc;
            char msg[160];
            std::snprintf(msg, sizeof msg, "%s: %llu records exceed max_hits = %llu", p.fn, total, (unsigned long long)p.max_hits);
            return fail(ctx, VSC_ERR_RANGE, msg);
        }
        float ms = 0;
        pieces.emplace_back();
        piece_n.push_back(found);
        r.records = nullptr;
        r.side = nullptr;
        r.n_records = found;
        if (found) {
            DeviceBuf &into = selecting ? raw : pieces.back();
            VSC_HIP(ctx, into.ensure(piece_bytes(found)));
            r.records = into.p;
            if (side_bytes) r.side = (uint32_t *)((char *)into.p + side_at(found));
        }
        if (found || rows || rows64) {  // (rows without records: the write pass adds the rows of the cells that are not empty and writes nothing)
            VSC_HIP(ctx, hipEventRecord(ctx->ev[kEvStage2Start], ctx->stream));
            VSC_HIP(ctx, launch(r, true));
            VSC_HIP(ctx, hipEventRecord(ctx->ev[kEvStage2End], ctx->stream));
            VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));
            VSC_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev[kEvStage2Start], ctx->ev[kEvStage2End]));
            t.scan_ms += ms;
            t.genome_bytes += (uint64_t)n_tiles * kTileWords * 3 * sizeof(uint32_t);
        }
        if (selecting && found) {
            // the selection stage: every guide's threshold, one read-back of the survivors per guide (they size the round's
            // piece), then the walk that keeps them in record order
            PatSelectArgs sa{};
            sa.count = r.count;
            sa.chunk_sum = r.chunk_sum;
            sa.group_off = r.off;
            sa.n_tiles = n_tiles;
            sa.n_guides = r.n;
            sa.n_records = found;
            sa.records = (const uint32_t *)r.records;
            sa.fixed = r.side;
            sa.top_k = p.score->top_k;
            sa.min_score = p.score->min_score;
            sa.sel = d_sel;
            sel_host.resize(r.n);
            VSC_HIP(ctx, hipEventRecord(ctx->ev[kEvStage2Start], ctx->stream));
            VSC_HIP(ctx, launch_pattern_select(sa, ctx->stream));
            VSC_HIP(ctx, hipMemcpyAsync(sel_host.data(), d_sel, r.n * sizeof(uint4), hipMemcpyDeviceToHost, ctx->stream));
            VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));
            unsigned long long kept = 0;
            for (const uint4 &q : sel_host) kept += (unsigned long long)q.w << 32 | q.z;
            if (kept) {
                VSC_HIP(ctx, pieces.back().ensure(piece_bytes(kept)));
                sa.out_records = (uint32_t *)pieces.back().p;
                sa.out_fixed = (uint32_t *)((char *)pieces.back().p + side_at(kept));
                sa.n_out = kept;
                VSC_HIP(ctx, launch_pattern_select_walk(sa, ctx->stream));
            }
            VSC_HIP(ctx, hipEventRecord(ctx->ev[kEvStage2End], ctx->stream));
            VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));
            VSC_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev[kEvStage2Start], ctx->ev[kEvStage2End]));
            t.score_ms += ms;
            piece_n.back() = kept;
            total = total - found + kept;
        }
    }
    if (selecting && p.max_hits && total > p.max_hits) {
        char msg[160];
        std::snprintf(msg, sizeof msg, "%s: %llu records exceed max_hits = %llu", p.fn, total, (unsigned long long)p.max_hits);
        return fail(ctx, VSC_ERR_RANGE, msg);
    }
    unsigned long long sites = 0;
    VSC_HIP(ctx, hipMemcpyAsync(&sites, d_sites, sizeof sites, hipMemcpyDeviceToHost, ctx->stream));
    if (rows) VSC_HIP(ctx, hipMemcpyAsync(rows, d_rows, rows_words * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (rows64) VSC_HIP(ctx, hipMemcpyAsync(rows64, d_rows64, rows64_words * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    if (out && total) {
        if (pieces.size() == 1) {
            holder->storage = pieces[0];
            pieces[0] = DeviceBuf();
        } else {
            VSC_HIP(ctx, holder->storage.ensure(piece_bytes(total)));
            size_t at = 0, at_side = side_at(total);
            for (size_t i = 0; i < pieces.size(); ++i) {
                if (piece_n[i]) {
                    VSC_HIP(ctx, hipMemcpyAsync((char *)holder->storage.p + at, pieces[i].p, (size_t)piece_n[i] * rec_bytes, hipMemcpyDeviceToDevice,
                                                ctx->stream));
                    if (side_bytes)
                        VSC_HIP(ctx, hipMemcpyAsync((char *)holder->storage.p + at_side, (char *)pieces[i].p + side_at(piece_n[i]),
                                                    (size_t)piece_n[i] * side_bytes, hipMemcpyDeviceToDevice, ctx->stream));
                }
                at += (size_t)piece_n[i] * rec_bytes;
                at_side += (size_t)piece_n[i] * side_bytes;
            }
        }
        holder->n = total;
        holder->host_valid = false;
        holder->side_at = side_at(total);
        holder->side_host_valid = false;
    }
    VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (rows && !out)
        for (size_t k = 0; k < rows_words; ++k) total += rows[k];
    t.total_ms = t.scan_ms;
    t.hits = total;
    t.sites = sites;
    t.pairs = sites * n_guides;
    ctx->timing = t;
    if (out) *out = holder.release();
    return VSC_OK;
}

// uint4s of one table of n pattern guides: padded to kPatUnroll, plus kPatUnroll spare (the count pass fetches ahead)
uint32_t pattern_table_slots(uint32_t n) { return (n + kPatUnroll - 1) / kPatUnroll * kPatUnroll + kPatUnroll; }


}  // namespace

extern "C" {

int vsc_search(vsc_ctx *ctx, const vsc_genome *genome, const uint64_t *guides, uint32_t n_guides,
               const vsc_search_params *params, vsc_hits **out)
{
    return guarded(ctx, [&]() -> int {
    if (!ctx || !out) return VSC_ERR_INVALID;
    *out = nullptr;
    SearchPlan p("vsc_search", Records::kAccumulate, out);
    return run_search(ctx, genome, guides, n_guides, params, p);
    });
}

int vsc_search_summary(vsc_ctx *ctx, const vsc_genome *genome, const uint64_t *guides, uint32_t n_guides,
                       const vsc_search_params *params, const vsc_locus *exclude, vsc_guide_summary *out)
{
    return search_summary(ctx, genome, guides, n_guides, params, exclude, nullptr, out, nullptr, "vsc_search_summary");
}

int vsc_search_summary_regions(vsc_ctx *ctx, const vsc_genome *genome, const uint64_t *guides, uint32_t n_guides,
                               const vsc_search_params *params, const vsc_locus *exclude, const vsc_regions *regions,
                               vsc_guide_summary *out_all, vsc_guide_summary *out_in)
{
    if (!ctx) return VSC_ERR_INVALID;
    if (!regions || (n_guides && !out_in)) return fail(ctx, VSC_ERR_INVALID, "vsc_search_summary_regions: null argument");
    return search_summary(ctx, genome, guides, n_guides, params, exclude, regions, out_all, out_in, "vsc_search_summary_regions");
}

int vsc_search_select(vsc_ctx *ctx, const vsc_genome *genome, const uint64_t *guides, uint32_t n_guides,
                      const vsc_search_params *params, const vsc_select *select, const vsc_locus *exclude,
                      vsc_guide_summary *summary, vsc_hits **out)
{
    return search_select(ctx, genome, guides, n_guides, params, select, nullptr, exclude, summary, nullptr, out, "vsc_search_select");
}

int vsc_search_select_regions(vsc_ctx *ctx, const vsc_genome *genome, const uint64_t *guides, uint32_t n_guides,
                              const vsc_search_params *params, const vsc_select *select, const vsc_region_filter *filter,
                              const vsc_locus *exclude, vsc_guide_summary *summary_all, vsc_guide_summary *summary_in,
                              vsc_hits **out)
{
    if (!ctx || !out) return VSC_ERR_INVALID;
    *out = nullptr;
    if (filter && (!filter->regions || filter->scope > VSC_REGION_DROP || filter->reserved))
        return fail(ctx, VSC_ERR_INVALID, "vsc_search_select_regions: a filter needs regions, a scope of 0 or 1 and a reserved field of 0");
    if (!filter && summary_in) return fail(ctx, VSC_ERR_INVALID, "vsc_search_select_regions: summary_in without a filter");
    return search_select(ctx, genome, guides, n_guides, params, select, filter, exclude, summary_all, summary_in, out,
                         "vsc_search_select_regions");
}

int vsc_search_summary_classified(vsc_ctx *ctx, const vsc_genome *genome, const uint64_t *guides, uint32_t n_guides,
                                  const vsc_search_params *params, const vsc_locus *exclude, const vsc_classify *cls,
                                  vsc_guide_summary *out, vsc_guide_votes *out_votes)
{
    return guarded(ctx, [&]() -> int {
    if (!ctx) return VSC_ERR_INVALID;
    if (n_guides && !out_votes) return fail(ctx, VSC_ERR_INVALID, "vsc_search_summary_classified: null argument");
    SearchPlan p("vsc_search_summary_classified", Records::kNone);
    p.exclude = exclude;
    p.rows = out;
    p.classifies = true;
    p.classify = cls;
    p.votes_rows = out_votes;
    return run_search(ctx, genome, guides, n_guides, params, p);
    });
}

int vsc_search_select_classified(vsc_ctx *ctx, const vsc_genome *genome, const uint64_t *guides, uint32_t n_guides,
                                 const vsc_search_params *params, const vsc_select_votes *select, const vsc_classify *cls,
                                 const vsc_locus *exclude, vsc_guide_summary *summary, vsc_guide_votes *votes_rows, vsc_hits **out)
{
    return guarded(ctx, [&]() -> int {
    if (!ctx || !out) return VSC_ERR_INVALID;
    *out = nullptr;
    SearchPlan p("vsc_search_select_classified", Records::kAccumulate, out);
    p.exclude = exclude;
    p.rows = summary;
    p.classifies = true;
    p.classify = cls;
    p.votes_rows = votes_rows;
    p.selects_votes = true;
    p.select_votes = select;
    return run_search(ctx, genome, guides, n_guides, params, p);
    });
}

int vsc_search_summary_table(vsc_ctx *ctx, const vsc_genome *genome, const uint64_t *guides, uint32_t n_guides,
                             const vsc_search_params *params, const vsc_locus *exclude, const vsc_score_table *table,
                             vsc_guide_summary *plain, vsc_guide_table_row *out)
{
    return guarded(ctx, [&]() -> int {
    if (!ctx) return VSC_ERR_INVALID;
    if (n_guides && !out) return fail(ctx, VSC_ERR_INVALID, "vsc_search_summary_table: null argument");
    SearchPlan p("vsc_search_summary_table", Records::kNone);
    p.exclude = exclude;
    p.rows = plain;
    p.tables = true;
    p.table = table;
    p.table_rows = out;
    return run_search(ctx, genome, guides, n_guides, params, p);
    });
}

int vsc_search_select_table(vsc_ctx *ctx, const vsc_genome *genome, const uint64_t *guides, uint32_t n_guides,
                            const vsc_search_params *params, const vsc_select *select, const vsc_locus *exclude,
                            const vsc_score_table *table, vsc_guide_table_row *rows, vsc_hits **out)
{
    return guarded(ctx, [&]() -> int {
    if (!ctx || !out) return VSC_ERR_INVALID;
    *out = nullptr;
    SearchPlan p("vsc_search_select_table", Records::kAccumulate, out);
    p.exclude = exclude;
    p.selects = true;
    p.select = select;
    p.tables = true;
    p.table = table;
    p.table_rows = rows;
    return run_search(ctx, genome, guides, n_guides, params, p);
    });
}

// ---- guide discovery (kernels: vsc_enum.hip; the passes: run_enumeration) --------------------------------------------------
int vsc_guides_enumerate(vsc_ctx *ctx, const vsc_genome *genome, const vsc_regions *regions, const vsc_enum_params *params,
                         vsc_guides **out)
{
    return guarded(ctx, [&]() -> int {
    if (!ctx || !out) return VSC_ERR_INVALID;
    *out = nullptr;
    ctx->err.clear();
    const char *const fn = "vsc_guides_enumerate";
    if (!genome || !params) return fail_in(ctx, VSC_ERR_INVALID, fn, "null argument");
    if (genome->ctx != ctx) return fail_in(ctx, VSC_ERR_INVALID, fn, "genome belongs to another context");
    const int p0 = base_code(params->pam[0]), p1 = base_code(params->pam[1]);
    if (p0 > 3 || p1 > 3) return fail_in(ctx, VSC_ERR_INVALID, fn, "the PAM must be two letters of ACGT");
    if (params->strands > 2) return fail_in(ctx, VSC_ERR_INVALID, fn, "strands must be 0 (both), 1 ('+') or 2 ('-')");
    if (params->gc_min > 20 || params->gc_max > 20 || (params->gc_max && params->gc_min > params->gc_max))
        return fail_in(ctx, VSC_ERR_INVALID, fn, "GC bounds must satisfy gc_min <= gc_max <= 20 (gc_max 0: no upper bound)");
    if (params->reserved0 || params->reserved[0] || params->reserved[1]) return fail_in(ctx, VSC_ERR_INVALID, fn, "reserved fields must be 0");
    VSC_HIP(ctx, hipSetDevice(ctx->device));
    EnumArgs a{};
    if (regions) {
        const int rrc = resident_regions(ctx, genome, regions, fn, a.reg);
        if (rrc != VSC_OK) return rrc;
    }
    bind_genome(a, genome);
    a.pam = pam_masks(p0, p1);
    a.keep_fwd = params->strands != 2 ? 0xFFFFFFFFu : 0u;
    a.keep_rev = params->strands != 1 ? 0xFFFFFFFFu : 0u;
    a.gc_min = params->gc_min;
    a.gc_max = params->gc_max ? params->gc_max : 20u;
    a.max_t_run = params->max_t_run;
    a.filter = (a.gc_min > 0 || a.gc_max < 20 || a.max_t_run) ? 1u : 0u;

    // the work list: with regions, the tiles that hold a block of the class table that is not OUT (a block is >= 32 starts,
    // a tile 2 048: 64 blocks or fewer); without, every tile of the shard
    std::vector<uint32_t> work;
    uint32_t n_work = genome->d_hi ? genome->n_tiles : 0;
    if (regions && n_work) {
        const uint32_t shift = regions->block_shift;
        for (uint32_t t = 0; t < genome->n_tiles; ++t) {
            const uint64_t p = (uint64_t)a.first_pos + (uint64_t)t * kTileBases;
            const uint64_t b0 = p >> shift, b1 = std::min<uint64_t>((p + kTileBases - 1) >> shift, (uint64_t)regions->n_blocks - 1);
            bool any = false;
            for (uint64_t b = b0; !any && regions->n_blocks && b <= b1; ++b) any = ((regions->cls[b >> 4] >> (2 * (b & 15))) & 3u) != kRegOut;
            if (any) work.push_back(t);
        }
        n_work = (uint32_t)work.size();
    }
    return run_enumeration(ctx, fn, a, regions ? &work : nullptr, n_work, nullptr, 0, params->max_guides, out,
                           [&](const void *, unsigned long long, bool write) { return launch_enum(a, write, regions != nullptr, ctx->stream); });
    });
}

uint64_t vsc_guides_count(const vsc_guides *guides) { return guides ? guides->n : 0; }
int vsc_guides_data(vsc_guides *guides, const uint64_t **codes, const vsc_locus **loci) { return guide_list_data(guides, codes, loci); }
int vsc_guides_data_dev(const vsc_guides *guides, const void **codes_dev, const void **loci_dev)
{
    return guide_list_data_dev(guides, codes_dev, loci_dev);
}
int vsc_guides_free(vsc_guides *guides) { return object_free(guides); }

// ---- bulge-tolerant search (kernels: vsc_bulge.hip; the rounds: run_rounds, one level of sums) ----------------
int vsc_search_bulges(vsc_ctx *ctx, const vsc_genome *genome, const uint64_t *guides, uint32_t n_guides, const vsc_search_params *params,
                      const vsc_bulge_params *bulge_params, vsc_bulge_hits **out, vsc_bulge_summary *rows)
{
    return guarded(ctx, [&]() -> int {
    if (!ctx) return VSC_ERR_INVALID;
    if (out) *out = nullptr;
    ctx->err.clear();
    const char *const fn = "vsc_search_bulges";
    if (!out && !rows) return fail_in(ctx, VSC_ERR_INVALID, fn, "neither records nor rows are asked for");
    if (!genome || !params || !bulge_params || (n_guides && !guides)) return fail_in(ctx, VSC_ERR_INVALID, fn, "null argument");
    if (genome->ctx != ctx) return fail_in(ctx, VSC_ERR_INVALID, fn, "genome belongs to another context");
    if (params->max_mismatches > VSC_MAX_MISMATCHES) return fail_in(ctx, VSC_ERR_INVALID, fn, "max_mismatches must be 0..8");
    if (params->algorithm != VSC_ALGO_AUTO && params->algorithm != VSC_ALGO_SCAN)
        return fail_in(ctx, VSC_ERR_INVALID, fn, "algorithm must be VSC_ALGO_AUTO or VSC_ALGO_SCAN (no seed index is used)");
    if (bulge_params->dna_max > 2 || bulge_params->rna_max > 2 || (bulge_params->dna_max == 0 && bulge_params->rna_max == 0))
        return fail_in(ctx, VSC_ERR_INVALID, fn, "dna_max and rna_max must be 0..2 and not both 0");
    if (bulge_params->reserved) return fail_in(ctx, VSC_ERR_INVALID, fn, "reserved fields must be 0");
    ScanArgs pams{};
    fill_pam(pams, params);
    BulgeArgs a{};
    bind_genome(a, genome);
    a.n_tiles = genome->d_hi ? genome->n_tiles : 0;
    a.max_mm = params->max_mismatches;
    a.n_pam = pams.n_pam;
    for (uint32_t i = 0; i < pams.n_pam; ++i) a.pam[i] = pams.pam[i];
    a.dna_max = bulge_params->dna_max;
    a.rna_max = bulge_params->rna_max;

    static_assert(sizeof(vsc_bulge_summary) == kBulgeRowWords * sizeof(uint32_t), "a row is its counts");
    const uint32_t batch = std::min(bulge_params->guide_batch ? std::min(bulge_params->guide_batch, kBulgeMaxBatch) : kBulgeDefaultBatch, n_guides);
    const RoundsPlan plan{fn, n_guides, a.n_tiles, batch, &ctx->bulge_tabs, 1, kBulgeRowWords, bulge_params->max_hits};
    return run_rounds(
        ctx, plan, out, (uint32_t *)rows,
        // two reads per uint4: padded to kBulgeUnroll reads, plus four spare
        [](uint32_t n) { return (n + kBulgeUnroll - 1) / kBulgeUnroll * (kBulgeUnroll / 2) + kBulgeUnroll / 2; },
        [&](uint32_t g0, uint32_t n, uint4 *table) {
            for (uint32_t i = 0; i < n; ++i) {
                uint32_t h, l;
                guide_planes(guides[g0 + i], &h, &l);
                uint4 &r = table[i / 2];
                if (i & 1) r.z = h, r.w = l; else r.x = h, r.y = l;
            }
        },
        [&](const Round &r, bool write) {
            a.guides = r.guides;
            a.n_guides = r.n;
            a.guide_base = r.g0;
            a.count = r.count;
            a.chunk_off = r.off;
            a.sites = r.sites;
            a.rows = r.rows;
            a.records = (uint4 *)r.records;
            a.n_records = r.n_records;
            return write ? launch_bulge_write(a, ctx->n_cus, ctx->stream) : launch_bulge_count(a, ctx->n_cus, ctx->stream);
        });
    });
}

uint64_t vsc_bulge_hits_count(const vsc_bulge_hits *hits) { return hits ? hits->n : 0; }
int vsc_bulge_hits_data(vsc_bulge_hits *hits, const vsc_bulge_hit **out) { return record_list_data(hits, out); }
const void *vsc_bulge_hits_data_dev(const vsc_bulge_hits *hits) { return record_list_data_dev(hits); }
int vsc_bulge_hits_free(vsc_bulge_hits *hits) { return object_free(hits); }

int vsc_bulge_align(uint64_t guide_code, const char *site_text, int d, uint32_t *nm, uint32_t *index)
{
    if (!site_text || d < -2 || d > 2 || d == 0) return VSC_ERR_INVALID;
    const size_t len = (size_t)(VSC_READ_LEN + d);
    if (std::strlen(site_text) != len) return VSC_ERR_INVALID;
    uint32_t sh = 0, sl = 0, rh, rl;
    for (size_t j = 0; j < len; ++j) {
        const int c = base_code(site_text[j]);
        if (c > 3) return VSC_ERR_INVALID;
        sh |= (uint32_t)(c >> 1) << j;
        sl |= (uint32_t)(c & 1) << j;
    }
    guide_planes(guide_code, &rh, &rl);
    uint32_t at = 0;
    const uint32_t best = bulge_align(rh, rl, sh, sl, d, &at);
    if (nm) *nm = best;
    if (index) *index = at;
    return VSC_OK;
}

// ---- pattern search (kernels: vsc_pattern.hip; the rounds: run_rounds, two levels of sums) -------------------
// table != null: vsc_search_pattern_table - the scored write pass, the table rows and the selection stage
static int search_pattern_call(vsc_ctx *ctx, const char *fn, const vsc_genome *genome, const char *pattern, const char *guides, uint32_t n_guides,
                               uint32_t len, const vsc_pattern_params *params, const vsc_pattern_table *table, const vsc_pattern_select *select,
                               vsc_pattern_hits **out, vsc_pattern_summary *rows, vsc_guide_table_row *table_rows)
{
    return guarded(ctx, [&]() -> int {
    if (!ctx) return VSC_ERR_INVALID;
    if (out) *out = nullptr;
    ctx->err.clear();
    if (!out && !rows && !table_rows) return fail_in(ctx, VSC_ERR_INVALID, fn, table ? "neither records nor rows of either kind are asked for" : "neither records nor rows are asked for");
    if (!genome || !params || !pattern || (n_guides && !guides)) return fail_in(ctx, VSC_ERR_INVALID, fn, "null argument");
    if (genome->ctx != ctx) return fail_in(ctx, VSC_ERR_INVALID, fn, "genome belongs to another context");
    if (len < kPatMinLen || len > kPatMaxLen) return fail_in(ctx, VSC_ERR_INVALID, fn, "the pattern must have 16..32 letters");
    if (params->max_mismatches > VSC_MAX_MISMATCHES) return fail_in(ctx, VSC_ERR_INVALID, fn, "max_mismatches must be 0..8");
    if (params->reserved[0] || params->reserved[1]) return fail_in(ctx, VSC_ERR_INVALID, fn, "reserved fields must be 0");
    if (table && table->shape.len != len) return fail_in(ctx, VSC_ERR_INVALID, fn, "the table is built for another length");
    if (select && (select->reserved[0] || select->reserved[1])) return fail_in(ctx, VSC_ERR_INVALID, fn, "reserved fields of the selection must be 0");
    uint8_t sets[kPatMaxLen], rc_sets[kPatMaxLen];
    if (!pattern_sets(pattern, len, sets)) return fail_in(ctx, VSC_ERR_INVALID, fn, "the pattern holds a letter that is no IUPAC letter");
    PatternArgs a{};
    pattern_front(sets, len, &a.front[0]);
    pattern_revcomp(sets, len, rc_sets);
    pattern_front(rc_sets, len, &a.front[1]);
    // every guide as two uint4: its planes for '+', those of its reverse complement for '-' (scored: a third, its
    // read-orientation planes as the score reads them)
    std::vector<uint4> planes((size_t)2 * n_guides), reads(table ? n_guides : 0);
    for (uint32_t g = 0; g < n_guides; ++g) {
        if (!pattern_sets(guides + (size_t)g * len, len, sets)) {
            char msg[120];
            std::snprintf(msg, sizeof msg, "%s: guide %u holds a letter that is no IUPAC letter", fn, g);
            return fail(ctx, VSC_ERR_INVALID, msg);
        }
        pattern_revcomp(sets, len, rc_sets);
        const PatPlanes f = pattern_planes(sets, len), r = pattern_planes(rc_sets, len);
        planes[2 * (size_t)g] = make_uint4(f.a, f.c, f.g, f.t);
        planes[2 * (size_t)g + 1] = make_uint4(r.a, r.c, r.g, r.t);
        if (table) {
            uint32_t gh, gl, single;
            pattern_table_guide(sets, len, &gh, &gl, &single);
            reads[g] = make_uint4(gh, gl, single, 0);
        }
    }
    bind_genome(a, genome);
    a.n_tiles = genome->d_hi ? genome->n_tiles : 0;
    a.len = len;
    a.max_mm = params->max_mismatches;

    static_assert(sizeof(vsc_pattern_summary) == kPatRowWords * sizeof(uint32_t), "a row is its counts");
    static_assert(sizeof(vsc_guide_table_row) == kPatTableRowWords * sizeof(unsigned long long), "a table row is its twelve words");
    static_assert(sizeof(vsc_pattern_table_shape) == sizeof(PatTableShape), "the shape is the kernels'");
    const uint32_t batch = std::min(params->guide_batch ? std::min(params->guide_batch, kPatMaxBatch) : kPatDefaultBatch, n_guides);
    RoundsPlan plan{fn, n_guides, a.n_tiles, batch, &ctx->pattern_tabs, 2, kPatRowWords, params->max_hits};
    RoundsScore scored{(unsigned long long *)table_rows, select ? select->top_k : 0u, select ? select->min_score : 0u};
    PatScoreArgs sc{};
    std::vector<vsc_pattern_summary> own_rows;  // table rows alone: the NM rows are what the call's hit count comes from
    if (table) {
        plan.score = &scored;
        sc.shape = table->shape;
        if (n_guides && a.n_tiles) {
            VSC_HIP(ctx, hipSetDevice(ctx->device));
            const int trc = resident_pattern_table(ctx, table);
            if (trc != VSC_OK) return trc;
        }
        sc.weights = (const double *)ctx->pattern_table_buf.p;
        if (!out && !rows) {
            own_rows.resize(n_guides);
            rows = own_rows.data();
        }
    }
    const uint32_t tables = table ? 3 : 2;
    const int rounds_rc = run_rounds(
        ctx, plan, out, (uint32_t *)rows,
        // two tables, '+' and '-', one stride apart (scored: a third, the guides in read orientation)
        [tables](uint32_t n) { return tables * pattern_table_slots(n); },
        [&](uint32_t g0, uint32_t n, uint4 *tab) {
            const uint32_t stride = pattern_table_slots(n);
            for (uint32_t i = 0; i < n; ++i) {
                tab[i] = planes[2 * (size_t)(g0 + i)];
                tab[stride + i] = planes[2 * (size_t)(g0 + i) + 1];
                if (table) tab[2 * stride + i] = reads[g0 + i];
            }
        },
        [&](const Round &r, bool write) {
            a.guides = r.guides;
            a.guide_stride = pattern_table_slots(r.n);
            a.n_guides = r.n;
            a.guide_base = r.g0;
            a.count = r.count;
            a.chunk_sum = r.chunk_sum;
            a.group_off = r.off;
            a.sites = r.sites;
            a.rows = r.rows;
            a.records = (uint32_t *)r.records;
            a.n_records = r.n_records;
            if (write && table) {
                sc.fixed = r.side;
                sc.table_rows = r.rows64;
                return launch_pattern_write_scored(a, sc, ctx->n_cus, ctx->stream);
            }
            return write ? launch_pattern_write(a, ctx->n_cus, ctx->stream) : launch_pattern_count(a, ctx->n_cus, ctx->stream);
        });
    if (rounds_rc == VSC_OK && out && *out) (*out)->site_len = len;  // (what vsc_pattern_hits_variants walks with)
    return rounds_rc;
    });
}

int vsc_search_pattern(vsc_ctx *ctx, const vsc_genome *genome, const char *pattern, const char *guides, uint32_t n_guides, uint32_t len,
                       const vsc_pattern_params *params, vsc_pattern_hits **out, vsc_pattern_summary *rows)
{
    return search_pattern_call(ctx, "vsc_search_pattern", genome, pattern, guides, n_guides, len, params, nullptr, nullptr, out, rows, nullptr);
}

// ---- table scores for pattern hits (the score: vsc_pattern_table.h; the kernels: vsc_pattern.hip) -------------
int vsc_search_pattern_table(vsc_ctx *ctx, const vsc_genome *genome, const char *pattern, const char *guides, uint32_t n_guides, uint32_t len,
                             const vsc_pattern_params *params, const vsc_pattern_table *table, const vsc_pattern_select *select,
                             vsc_pattern_hits **out, vsc_pattern_summary *rows, vsc_guide_table_row *table_rows)
{
    if (!table) {
        if (out) *out = nullptr;
        return ctx ? fail_in(ctx, VSC_ERR_INVALID, "vsc_search_pattern_table", "null argument") : VSC_ERR_INVALID;
    }
    return search_pattern_call(ctx, "vsc_search_pattern_table", genome, pattern, guides, n_guides, len, params, table, select, out, rows,
                               table_rows);
}

int vsc_pattern_hits_scores(vsc_pattern_hits *hits, const uint32_t **fixed)
{
    if (!hits || !fixed || !hits->has_side) return VSC_ERR_INVALID;
    return guarded(hits->ctx, [&]() -> int {
    if (!hits->side_host_valid) {
        vsc_ctx *ctx = hits->ctx;
        hits->side_host.resize(hits->n);
        VSC_HIP(ctx, hipSetDevice(ctx->device));
        VSC_HIP(ctx, hipMemcpyAsync(hits->side_host.data(), (const char *)hits->storage.p + hits->side_at, hits->n * sizeof(uint32_t),
                                    hipMemcpyDeviceToHost, ctx->stream));
        VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        hits->side_host_valid = true;
    }
    *fixed = hits->side_host.data();
    return VSC_OK;
    });
}

const void *vsc_pattern_hits_scores_dev(const vsc_pattern_hits *hits)
{
    return hits && hits->has_side && hits->n ? (const char *)hits->storage.p + hits->side_at : nullptr;
}

int vsc_pattern_table_build(const vsc_pattern_table_shape *shape, const double *pair, const double *pam, vsc_pattern_table **out)
{
    if (!out) return VSC_ERR_INVALID;
    *out = nullptr;
    if (!shape || !pair || !pam) return VSC_ERR_INVALID;
    static std::atomic<uint64_t> serial{0};
    PatTableShape sh{};
    std::memcpy(&sh, shape, sizeof sh);
    if (!pattern_table_shape_valid(sh)) return VSC_ERR_INVALID;  // (before the weights are read: the shape sizes them)
    for (uint32_t t = sh.n_pam; t < kPatTableMaxPam; ++t) sh.pam_pos[t] = 0;
    vsc_pattern_table *t = new (std::nothrow) vsc_pattern_table();
    if (!t) return VSC_ERR_NOMEM;
    t->shape = sh;
    const uint32_t pairs = pattern_table_pairs(sh), n = pattern_table_weights(sh);
    std::memcpy(t->w, pair, pairs * sizeof(double));
    std::memcpy(t->w + pairs, pam, (n - pairs) * sizeof(double));
    if (!pattern_table_valid(sh, t->w)) {  // a weight outside [0, 1] (NaN included) or a diagonal entry other than 1
        delete t;
        return VSC_ERR_INVALID;
    }
    for (uint32_t i = 0; i < n; ++i) t->zeros += t->w[i] == 0.0;
    t->serial = serial.fetch_add(1, std::memory_order_relaxed) + 1;
    *out = t;
    return VSC_OK;
}

int vsc_pattern_table_free(vsc_pattern_table *table)
{
    delete table;
    return VSC_OK;
}

int vsc_pattern_table_info(const vsc_pattern_table *table, vsc_pattern_table_stats *out)
{
    if (!table || !out) return VSC_ERR_INVALID;
    *out = vsc_pattern_table_stats{};
    out->serial = table->serial;
    out->zero_weights = table->zeros;
    std::memcpy(&out->shape, &table->shape, sizeof out->shape);
    return VSC_OK;
}

int vsc_pattern_table_score(const vsc_pattern_table *table, const char *guide, const char *site_text, double *score, uint32_t *fixed)
{
    if (!table || !guide || !site_text) return VSC_ERR_INVALID;
    const uint32_t len = table->shape.len;
    uint8_t sets[kPatMaxLen];
    if (!pattern_sets(guide, len, sets)) return VSC_ERR_INVALID;
    uint32_t gh, gl, single, sh = 0, sl = 0;
    pattern_table_guide(sets, len, &gh, &gl, &single);
    for (uint32_t j = 0; j < len; ++j) {
        const int c = base_code(site_text[j]);
        if (c > 3) return VSC_ERR_INVALID;
        sh |= (uint32_t)(c >> 1) << j;
        sl |= (uint32_t)(c & 1) << j;
    }
    const double x = pattern_table_score(table->w, table->shape, gh, gl, single, sh, sl);
    if (score) *score = x;
    if (fixed) *fixed = table_fixed(x);
    return VSC_OK;
}

uint64_t vsc_pattern_hits_count(const vsc_pattern_hits *hits) { return hits ? hits->n : 0; }
int vsc_pattern_hits_data(vsc_pattern_hits *hits, const vsc_pattern_hit **out) { return record_list_data(hits, out); }
const void *vsc_pattern_hits_data_dev(const vsc_pattern_hits *hits) { return record_list_data_dev(hits); }
int vsc_pattern_hits_free(vsc_pattern_hits *hits) { return object_free(hits); }

// ---- variant-aware pattern screen (kernels: vsc_pattern_variants.hip) ------------------------------------------
// The window side's tables: resident_variant_map's checks and device copies, as the pattern kernels read them.
static int pv_bind_window(vsc_ctx *ctx, const vsc_genome *win_genome, const vsc_variant_map *map, const vsc_locus *exclude, uint32_t n_guides,
                          const char *who, PatVarArgs &a)
{
    VariantArgs v{};
    const int rc = resident_variant_map(ctx, win_genome, map, exclude, n_guides, who, v);
    if (rc != VSC_OK) return rc;
    a.map = v.map;
    a.hi = v.hi;
    a.lo = v.lo;
    a.first_pos = v.first_pos;
    a.n_plane_words = v.n_plane_words;
    a.contig_off = v.contig_off;
    a.contig_end = v.contig_end;
    a.n_contigs = v.map.n_windows;
    a.exclude = v.exclude;
    a.n_guides = n_guides;
    return VSC_OK;
}

// The reference side's: ref_genome carries the contig table the map was built over; the shadow intervals - start[], then
// end_max[] - in one buffer keyed by the map's serial; the excluded loci in `excl` (the window side's copy, or this call's).
static int pv_bind_reference(vsc_ctx *ctx, const vsc_genome *ref_genome, const vsc_variant_map *map, const vsc_locus *exclude,
                             uint32_t n_guides, const uint4 *resident_exclude, const char *who, PatVarArgs &a)
{
    if (ref_genome->ctx != ctx) return fail_in(ctx, VSC_ERR_INVALID, who, "genome belongs to another context");
    bool same = ref_genome->n_contigs == map->ref_contigs.size();
    for (uint32_t c = 0; same && c < ref_genome->n_contigs; ++c)
        same = ref_genome->h_contig_off[c] == map->ref_contigs[c].offset &&
               ref_genome->h_contig_end[c] - ref_genome->h_contig_off[c] == map->ref_contigs[c].length;
    if (!same) return fail_in(ctx, VSC_ERR_INVALID, who, "the variant map was built over another reference genome");
    for (uint32_t i = 0; exclude && i < n_guides; ++i)
        if ((exclude[i].contig != UINT32_MAX && exclude[i].contig >= map->ref_contigs.size()) || exclude[i].strand > 1)
            return fail_in(ctx, VSC_ERR_INVALID, who, "excluded locus outside the reference's contigs or strands");
    VSC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = map->shadow_start.size(), bytes = n * sizeof(uint32_t);
    if (ctx->pv_shadow_serial != map->serial) {
        ctx->pv_shadow_serial = 0;
        VSC_HIP(ctx, ctx->pv_shadow_buf.ensure(2 * bytes + 256));  // (never empty: a device copy has an address)
        if (n) {
            VSC_HIP(ctx, hipMemcpyAsync(ctx->pv_shadow_buf.p, map->shadow_start.data(), bytes, hipMemcpyHostToDevice, ctx->stream));
            VSC_HIP(ctx, hipMemcpyAsync((char *)ctx->pv_shadow_buf.p + bytes, map->shadow_end_max.data(), bytes, hipMemcpyHostToDevice, ctx->stream));
        }
        VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (the caller may free the map as soon as its call returns)
        ctx->pv_shadow_serial = map->serial;
    }
    a.sh_start = (const uint32_t *)ctx->pv_shadow_buf.p;
    a.sh_end_max = (const uint32_t *)((const char *)ctx->pv_shadow_buf.p + bytes);
    a.sh_n = (uint32_t)n;
    a.contig_off = ref_genome->d_contig_off;
    a.contig_end = ref_genome->d_contig_end;
    a.n_contigs = ref_genome->n_contigs;
    a.n_guides = n_guides;
    a.exclude = nullptr;
    if (exclude && n_guides) {
        if (resident_exclude) a.exclude = resident_exclude;
        else {
            VSC_HIP(ctx, ctx->var_excl.ensure((size_t)n_guides * sizeof(vsc_locus)));
            VSC_HIP(ctx, hipMemcpyAsync(ctx->var_excl.p, exclude, (size_t)n_guides * sizeof(vsc_locus), hipMemcpyHostToDevice, ctx->stream));
            a.exclude = (const uint4 *)ctx->var_excl.p;
        }
    }
    return VSC_OK;
}

// A call's state on the device: the error flag (its own 256 bytes), then `extra` zeroed bytes (the screen's rows).
constexpr size_t kPvStateHead = 256;
static int pv_state(vsc_ctx *ctx, size_t extra)
{
    VSC_HIP(ctx, ctx->pv_state.ensure(kPvStateHead + extra));
    VSC_HIP(ctx, hipMemsetAsync(ctx->pv_state.p, 0, kPvStateHead + extra, ctx->stream));
    return VSC_OK;
}

// has a kernel met a record outside the tables? (after the stream has been waited for)
static int pv_error(vsc_ctx *ctx, const char *who)
{
    uint32_t bad = 0;
    VSC_HIP(ctx, hipMemcpy(&bad, ctx->pv_state.p, sizeof bad, hipMemcpyDeviceToHost));
    if (bad) return fail_in(ctx, VSC_ERR_INVALID, who, "a record lies outside the variant map, its window or contig, or the guides");
    return VSC_OK;
}

// the records of a pattern result (and, scored, their f words) where they lie
static void pv_bind_records(const vsc_pattern_hits *hits, PatVarArgs &a)
{
    a.records = (const uint32_t *)hits->storage.p;
    a.fixed = hits->has_side ? (const uint32_t *)((const char *)hits->storage.p + hits->side_at) : nullptr;
    a.n = hits->n;
    a.len = hits->site_len;
}

int vsc_pattern_hits_variants(vsc_pattern_hits *hits, const vsc_genome *win_genome, const vsc_variant_map *map, const vsc_locus *exclude,
                              uint32_t n_guides, vsc_variant_label *labels)
{
    if (!hits || !hits->ctx) return VSC_ERR_INVALID;
    vsc_ctx *ctx = hits->ctx;
    const char *const who = "vsc_pattern_hits_variants";
    return guarded(ctx, [&]() -> int {
    ctx->err.clear();
    if (!win_genome || !map || (hits->n && !labels)) return fail_in(ctx, VSC_ERR_INVALID, who, "null argument");
    PatVarArgs a{};
    int rc = pv_bind_window(ctx, win_genome, map, exclude, n_guides, who, a);
    if (rc != VSC_OK || hits->n == 0) return rc;
    if (hits->site_len < kPatVarMinLen || hits->site_len > kPatVarMaxLen) return fail_in(ctx, VSC_ERR_INVALID, who, "the records are no pattern search's");
    if ((rc = pv_state(ctx, 0)) != VSC_OK) return rc;
    a.error = (uint32_t *)ctx->pv_state.p;
    pv_bind_records(hits, a);
    a.fixed = nullptr;  // (labels only: the scores are not read)
    VSC_HIP(ctx, ctx->var_labels.ensure(hits->n * sizeof(vsc_variant_label)));
    a.labels = (uint4 *)ctx->var_labels.p;
    VSC_HIP(ctx, launch_pattern_variant_merge(a, ctx->stream));
    VSC_HIP(ctx, hipMemcpyAsync(labels, a.labels, hits->n * sizeof(vsc_variant_label), hipMemcpyDeviceToHost, ctx->stream));
    VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return pv_error(ctx, who);
    });
}

int vsc_pattern_hits_shadowed(vsc_pattern_hits *hits, const vsc_genome *ref_genome, const vsc_variant_map *map, const vsc_locus *exclude,
                              uint32_t n_guides, uint8_t *flags)
{
    if (!hits || !hits->ctx) return VSC_ERR_INVALID;
    vsc_ctx *ctx = hits->ctx;
    const char *const who = "vsc_pattern_hits_shadowed";
    return guarded(ctx, [&]() -> int {
    ctx->err.clear();
    if (!ref_genome || !map || (hits->n && !flags)) return fail_in(ctx, VSC_ERR_INVALID, who, "null argument");
    PatVarArgs a{};
    int rc = pv_bind_reference(ctx, ref_genome, map, exclude, n_guides, nullptr, who, a);
    if (rc != VSC_OK || hits->n == 0) return rc;
    if (hits->site_len < kPatVarMinLen || hits->site_len > kPatVarMaxLen) return fail_in(ctx, VSC_ERR_INVALID, who, "the records are no pattern search's");
    if ((rc = pv_state(ctx, 0)) != VSC_OK) return rc;
    a.error = (uint32_t *)ctx->pv_state.p;
    pv_bind_records(hits, a);
    a.fixed = nullptr;
    VSC_HIP(ctx, ctx->pv_flags.ensure(hits->n));
    a.flags = (uint8_t *)ctx->pv_flags.p;
    VSC_HIP(ctx, launch_pattern_shadow(a, ctx->stream));
    VSC_HIP(ctx, hipMemcpyAsync(flags, a.flags, hits->n, hipMemcpyDeviceToHost, ctx->stream));
    VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return pv_error(ctx, who);
    });
}

int vsc_search_pattern_variants(vsc_ctx *ctx, const vsc_genome *ref_genome, const vsc_genome *win_genome, const vsc_variant_map *map,
                                const char *pattern, const char *guides, uint32_t n_guides, uint32_t len, const vsc_pattern_params *params,
                                const vsc_pattern_table *table, const vsc_locus *exclude, uint32_t chunk_guides,
                                vsc_pattern_variant_row *ref_rows, vsc_pattern_variant_row *win_rows, vsc_pattern_variant_row *var_rows,
                                vsc_guide_table_row *ref_table, vsc_guide_table_row *win_table, vsc_guide_table_row *var_table)
{
    if (!ctx) return VSC_ERR_INVALID;
    const char *const who = "vsc_search_pattern_variants";
    static_assert(sizeof(vsc_pattern_variant_row) == sizeof(PatVarRow), "the rows are the kernels'");
    static_assert(sizeof(vsc_guide_table_row) == kPatVarTableWords * sizeof(unsigned long long), "a table row is its twelve words");
    PatVarArgs aw{}, ar{};
    const size_t row_bytes = (size_t)n_guides * sizeof(PatVarRow), table_bytes = (size_t)n_guides * sizeof(vsc_guide_table_row);
    const int rc = guarded(ctx, [&]() -> int {
        ctx->err.clear();
        // (a sample without alt alleles has no windows and no window genome: win_genome may be null with such a map)
        if (!ref_genome || !map || (!win_genome && map->win.size() > 1) || !pattern || !params || (n_guides && (!guides || !ref_rows || !win_rows)))
            return fail_in(ctx, VSC_ERR_INVALID, who, "null argument");
        if (!table && (ref_table || win_table || var_table)) return fail_in(ctx, VSC_ERR_INVALID, who, "table rows are asked for without a table");
        if (table && n_guides && (!ref_table || !win_table)) return fail_in(ctx, VSC_ERR_INVALID, who, "null argument");
        if (len < kPatVarMinLen || len > kPatVarMaxLen) return fail_in(ctx, VSC_ERR_INVALID, who, "the pattern must have 16..32 letters");
        if (table && table->shape.len != len) return fail_in(ctx, VSC_ERR_INVALID, who, "the table is built for another length");
        int brc = win_genome ? pv_bind_window(ctx, win_genome, map, exclude, n_guides, who, aw) : VSC_OK;
        if (brc != VSC_OK) return brc;
        if ((brc = pv_bind_reference(ctx, ref_genome, map, exclude, n_guides, aw.exclude, who, ar)) != VSC_OK) return brc;
        return pv_state(ctx, 3 * row_bytes + 3 * table_bytes);
    });
    if (rc != VSC_OK) return rc;
    char *const state = (char *)ctx->pv_state.p;
    PatVarRow *const d_rows = (PatVarRow *)(state + kPvStateHead);  // ref, win, var
    unsigned long long *const d_table = (unsigned long long *)(state + kPvStateHead + 3 * row_bytes);
    const size_t table_words = (size_t)n_guides * kPatVarTableWords;
    aw.error = ar.error = (uint32_t *)state;
    const uint32_t chunk = chunk_guides == 0 || chunk_guides > 64 ? 64 : chunk_guides;
    vsc_timing sum{};
    sum.index_ms = ctx->timing.index_ms;
    sum.algorithm = VSC_ALGO_SCAN;
    for (uint32_t g0 = 0; g0 < n_guides; g0 += chunk) {
        const uint32_t cn = std::min(chunk, n_guides - g0);
        for (int side = 0; side < (win_genome ? 2 : 1); ++side) {  // the reference, then the windows
            vsc_pattern_hits *hits = nullptr;
            const int src = search_pattern_call(ctx, who, side ? win_genome : ref_genome, pattern, guides + (size_t)g0 * len, cn, len, params, table,
                                                nullptr, &hits, nullptr, nullptr);
            if (src != VSC_OK) return src;
            std::unique_ptr<vsc_pattern_hits, int (*)(vsc_pattern_hits *)> holder(hits, object_free<vsc_pattern_hits>);
            const vsc_timing &t = ctx->timing;
            sum.scan_ms += t.scan_ms;
            sum.score_ms += t.score_ms;
            sum.total_ms += t.total_ms;
            sum.hits += t.hits;
            sum.sites += t.sites;
            sum.pairs += t.pairs;
            sum.passes += t.passes;
            sum.genome_bytes += t.genome_bytes;
            if (hits->n == 0) continue;
            const int mrc = guarded(ctx, [&]() -> int {
                PatVarArgs &a = side ? aw : ar;
                pv_bind_records(hits, a);
                const uint4 *const all_exclude = a.exclude;
                if (all_exclude) a.exclude = all_exclude + g0;  // the chunk's guides are numbered from 0
                a.n_guides = cn;
                a.rows_all = d_rows + (side ? n_guides : 0) + g0;
                a.rows_var = side && var_rows ? d_rows + 2 * (size_t)n_guides + g0 : nullptr;
                a.table_all = table ? d_table + (side ? table_words : 0) + (size_t)g0 * kPatVarTableWords : nullptr;
                a.table_var = side && table && var_table ? d_table + 2 * table_words + (size_t)g0 * kPatVarTableWords : nullptr;
                VSC_HIP(ctx, hipEventRecord(ctx->ev[kEvStageStart], ctx->stream));
                const hipError_t le = side ? launch_pattern_variant_merge(a, ctx->stream) : launch_pattern_shadow(a, ctx->stream);
                a.exclude = all_exclude;
                VSC_HIP(ctx, le);
                VSC_HIP(ctx, hipEventRecord(ctx->ev[kEvStageEnd], ctx->stream));
                VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (the records are freed when this round ends)
                float ms = 0;
                VSC_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev[kEvStageStart], ctx->ev[kEvStageEnd]));
                sum.finalize_ms += ms;
                sum.total_ms += ms;
                return VSC_OK;
            });
            if (mrc != VSC_OK) return mrc;
        }
    }
    return guarded(ctx, [&]() -> int {
        ctx->timing = sum;
        if (n_guides == 0) return VSC_OK;
        VSC_HIP(ctx, hipMemcpyAsync(ref_rows, d_rows, row_bytes, hipMemcpyDeviceToHost, ctx->stream));
        VSC_HIP(ctx, hipMemcpyAsync(win_rows, d_rows + n_guides, row_bytes, hipMemcpyDeviceToHost, ctx->stream));
        if (var_rows) VSC_HIP(ctx, hipMemcpyAsync(var_rows, d_rows + 2 * (size_t)n_guides, row_bytes, hipMemcpyDeviceToHost, ctx->stream));
        if (table) {
            VSC_HIP(ctx, hipMemcpyAsync(ref_table, d_table, table_bytes, hipMemcpyDeviceToHost, ctx->stream));
            VSC_HIP(ctx, hipMemcpyAsync(win_table, d_table + table_words, table_bytes, hipMemcpyDeviceToHost, ctx->stream));
            if (var_table) VSC_HIP(ctx, hipMemcpyAsync(var_table, d_table + 2 * table_words, table_bytes, hipMemcpyDeviceToHost, ctx->stream));
        }
        VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return pv_error(ctx, who);
    });
}

int vsc_pattern_match(const char *pattern, const char *guide, const char *site_text, uint32_t len, uint32_t *hit, uint32_t *nm, uint32_t *mask)
{
    if (!pattern || !guide || !site_text || len < kPatMinLen || len > kPatMaxLen) return VSC_ERR_INVALID;
    uint8_t p_sets[kPatMaxLen], g_sets[kPatMaxLen];
    if (!pattern_sets(pattern, len, p_sets) || !pattern_sets(guide, len, g_sets)) return VSC_ERR_INVALID;
    uint32_t sh = 0, sl = 0;
    bool acgt = true;
    for (uint32_t j = 0; j < len; ++j) {
        const int c = base_code(site_text[j]);
        if (c > 3) {
            acgt = false;
            break;
        }
        sh |= (uint32_t)(c >> 1) << j;
        sl |= (uint32_t)(c & 1) << j;
    }
    const uint32_t x = acgt ? pattern_mismatch(sh, sl, pattern_planes(g_sets, len)) : 0u;
    if (hit) *hit = acgt && pattern_mismatch(sh, sl, pattern_planes(p_sets, len)) == 0u;
    if (nm) *nm = (uint32_t)__builtin_popcount(x);
    if (mask) *mask = x;
    return VSC_OK;
}

// ---- bulges under a pattern (kernels: vsc_pattern_bulge.hip) ---------------------------------------------------
// vsc_search_pattern's rounds and scratch (the context's pattern pool) with vsc_search_bulges' result object and rows.  Per
// enabled class the front end gets two tables: the bulged pattern over L + d positions and its reverse complement.
int vsc_search_pattern_bulges(vsc_ctx *ctx, const vsc_genome *genome, const char *pattern, const char *guides, uint32_t n_guides, uint32_t len,
                              const vsc_pattern_bulge_params *params, vsc_bulge_hits **out, vsc_bulge_summary *rows)
{
    return guarded(ctx, [&]() -> int {
    if (!ctx) return VSC_ERR_INVALID;
    if (out) *out = nullptr;
    ctx->err.clear();
    const char *const fn = "vsc_search_pattern_bulges";
    if (!out && !rows) return fail_in(ctx, VSC_ERR_INVALID, fn, "neither records nor rows are asked for");
    if (!genome || !params || !pattern || (n_guides && !guides)) return fail_in(ctx, VSC_ERR_INVALID, fn, "null argument");
    if (genome->ctx != ctx) return fail_in(ctx, VSC_ERR_INVALID, fn, "genome belongs to another context");
    if (len < kPatMinLen || len > kPatMaxLen) return fail_in(ctx, VSC_ERR_INVALID, fn, "the pattern must have 16..32 letters");
    if (params->max_mismatches > VSC_MAX_MISMATCHES) return fail_in(ctx, VSC_ERR_INVALID, fn, "max_mismatches must be 0..8");
    uint8_t sets[kPatMaxLen], bulged[kPatMaxLen], rc_sets[kPatMaxLen];
    if (!pattern_sets(pattern, len, sets)) return fail_in(ctx, VSC_ERR_INVALID, fn, "the pattern holds a letter that is no IUPAC letter");
    if (const char *why = pattern_bulge_refusal(sets, len, params->proto_start, params->proto_len, params->dna_max, params->rna_max))
        return fail_in(ctx, VSC_ERR_INVALID, fn, why);
    PatBulgeArgs a{};
    a.len = len;
    a.proto_a = params->proto_start;
    a.proto_e = params->proto_start + params->proto_len;
    for (uint32_t k = 0; k < kBulgeClasses; ++k) {
        const int d = bulge_d_of_class(k);
        if (d < 0 ? (uint32_t)-d > params->rna_max : (uint32_t)d > params->dna_max) continue;
        a.classes |= 1u << k;
        const uint32_t site_len = (uint32_t)((int)len + d);
        pattern_bulged(sets, len, a.proto_a, a.proto_e, d, bulged);
        pattern_front(bulged, site_len, &a.front[k][0]);
        pattern_revcomp(bulged, site_len, rc_sets);
        pattern_front(rc_sets, site_len, &a.front[k][1]);
    }
    // every guide as one uint4: its planes in read orientation (the kernels turn the '-' sites)
    std::vector<uint4> planes(n_guides);
    for (uint32_t g = 0; g < n_guides; ++g) {
        if (!pattern_sets(guides + (size_t)g * len, len, sets)) {
            char msg[120];
            std::snprintf(msg, sizeof msg, "%s: guide %u holds a letter that is no IUPAC letter", fn, g);
            return fail(ctx, VSC_ERR_INVALID, msg);
        }
        const PatPlanes f = pattern_planes(sets, len);
        planes[g] = make_uint4(f.a, f.c, f.g, f.t);
    }
    bind_genome(a, genome);
    a.n_tiles = genome->d_hi ? genome->n_tiles : 0;
    a.max_mm = params->max_mismatches;

    const uint32_t batch = std::min(params->guide_batch ? std::min(params->guide_batch, kPatMaxBatch) : kPatDefaultBatch, n_guides);
    const RoundsPlan plan{fn, n_guides, a.n_tiles, batch, &ctx->pattern_tabs, 2, kBulgeRowWords, params->max_hits};
    return run_rounds(
        ctx, plan, out, (uint32_t *)rows, pattern_table_slots,
        [&](uint32_t g0, uint32_t n, uint4 *table) { std::copy_n(planes.begin() + g0, n, table); },
        [&](const Round &r, bool write) {
            a.guides = r.guides;
            a.n_guides = r.n;
            a.guide_base = r.g0;
            a.count = r.count;
            a.chunk_sum = r.chunk_sum;
            a.group_off = r.off;
            a.sites = r.sites;
            a.rows = r.rows;
            a.records = (uint4 *)r.records;
            a.n_records = r.n_records;
            return write ? launch_pattern_bulge_write(a, ctx->n_cus, ctx->stream) : launch_pattern_bulge_count(a, ctx->n_cus, ctx->stream);
        });
    });
}

int vsc_pattern_bulge_align(const char *pattern, const char *guide, const char *site_text, uint32_t len, uint32_t proto_start, uint32_t proto_len,
                            int d, uint32_t *hit, uint32_t *nm, uint32_t *index)
{
    if (!pattern || !guide || !site_text || len < kPatMinLen || len > kPatMaxLen || d < -2 || d > 2 || d == 0) return VSC_ERR_INVALID;
    uint8_t p_sets[kPatMaxLen], g_sets[kPatMaxLen], bulged[kPatMaxLen];
    if (!pattern_sets(pattern, len, p_sets) || !pattern_sets(guide, len, g_sets)) return VSC_ERR_INVALID;
    if (pattern_bulge_refusal(p_sets, len, proto_start, proto_len, d > 0 ? (uint32_t)d : 0u, d < 0 ? (uint32_t)-d : 0u)) return VSC_ERR_INVALID;
    const uint32_t site_len = (uint32_t)((int)len + d), a = proto_start, e = proto_start + proto_len;
    if (strnlen(site_text, site_len + 1u) != site_len) return VSC_ERR_INVALID;
    uint32_t sh = 0, sl = 0;
    bool acgt = true;
    for (uint32_t j = 0; j < site_len; ++j) {
        const int c = base_code(site_text[j]);
        if (c > 3) {
            acgt = false;
            break;
        }
        sh |= (uint32_t)(c >> 1) << j;
        sl |= (uint32_t)(c & 1) << j;
    }
    pattern_bulged(p_sets, len, a, e, d, bulged);
    const bool ok = acgt && pattern_mismatch(sh, sl, pattern_planes(bulged, site_len)) == 0u;
    uint32_t at = 0;
    const uint32_t best = ok ? pattern_bulge_align(sh, sl, pattern_planes(g_sets, len), a, e, d, &at) : 0u;
    if (hit) *hit = ok;
    if (nm) *nm = best;
    if (index) *index = ok ? at : 0u;
    return VSC_OK;
}

// ---- pattern guide discovery (kernels: the end of vsc_pattern.hip) --------------------------------------------
// vsc_guides_enumerate's passes (run_enumeration) behind the pattern search's front end.  The targets are no vsc_regions: their
// intervals become ranges of site starts on the host (pattern_target_ranges), the work list holds the tiles that meet one.
int vsc_guides_enumerate_pattern(vsc_ctx *ctx, const vsc_genome *genome, const char *pattern, uint32_t len, const vsc_pattern_enum_params *params,
                                 const vsc_interval *targets, uint64_t n_targets, vsc_pattern_guides **out)
{
    return guarded(ctx, [&]() -> int {
    if (!ctx || !out) return VSC_ERR_INVALID;
    *out = nullptr;
    ctx->err.clear();
    const char *const fn = "vsc_guides_enumerate_pattern";
    if (!genome || !params || !pattern || (n_targets && !targets)) return fail_in(ctx, VSC_ERR_INVALID, fn, "null argument");
    if (genome->ctx != ctx) return fail_in(ctx, VSC_ERR_INVALID, fn, "genome belongs to another context");
    if (len < kPatMinLen || len > kPatMaxLen) return fail_in(ctx, VSC_ERR_INVALID, fn, "the pattern must have 16..32 letters");
    uint8_t sets[kPatMaxLen], rc_sets[kPatMaxLen];
    if (!pattern_sets(pattern, len, sets)) return fail_in(ctx, VSC_ERR_INVALID, fn, "the pattern holds a letter that is no IUPAC letter");
    const uint32_t ps_a = params->ps_start, ps_k = params->ps_len;
    if (ps_k == 0 || ps_a + ps_k > len)
        return fail_in(ctx, VSC_ERR_INVALID, fn, "the protospacer must be a non-empty range of the pattern's positions");
    if (params->strands > 2) return fail_in(ctx, VSC_ERR_INVALID, fn, "strands must be 0 (both), 1 ('+') or 2 ('-')");
    if (params->gc_min > ps_k || params->gc_max > ps_k || (params->gc_max && params->gc_min > params->gc_max))
        return fail_in(ctx, VSC_ERR_INVALID, fn, "GC bounds must satisfy gc_min <= gc_max <= the protospacer's length (gc_max 0: no upper bound)");
    if (params->reserved0 || params->reserved1 || params->reserved[0] || params->reserved[1])
        return fail_in(ctx, VSC_ERR_INVALID, fn, "reserved fields must be 0");
    std::vector<PatStartRange> ranges;
    if (targets) {
        if (params->rule != VSC_REGION_OVERLAP && params->rule != VSC_REGION_INSIDE) return fail_in(ctx, VSC_ERR_INVALID, fn, "unknown target rule");
        if (pattern_target_ranges(genome->h_contig_off.data(), genome->h_contig_end.data(), genome->n_contigs, targets, n_targets, params->rule,
                                  len, &ranges) != VSC_OK)
            return fail_in(ctx, VSC_ERR_INVALID, fn, "a target interval is outside the contig table, has start > end or a non-zero reserved field");
    }
    VSC_HIP(ctx, hipSetDevice(ctx->device));
    PatEnumArgs a{};
    pattern_front(sets, len, &a.front[0]);
    pattern_revcomp(sets, len, rc_sets);
    pattern_front(rc_sets, len, &a.front[1]);
    bind_genome(a, genome);
    a.len = len;
    a.len_mask = len < 32u ? (1u << len) - 1u : ~0u;
    a.keep_fwd = params->strands != 2 ? 0xFFFFFFFFu : 0u;
    a.keep_rev = params->strands != 1 ? 0xFFFFFFFFu : 0u;
    const uint32_t ps_bits = ps_k < 32u ? (1u << ps_k) - 1u : ~0u;
    a.ps_fwd = ps_bits << ps_a;
    a.ps_rev = ps_bits << (len - ps_a - ps_k);
    a.gc_min = params->gc_min;
    a.gc_max = params->gc_max ? params->gc_max : ps_k;
    a.max_t_run = params->max_t_run;
    a.filter = (a.gc_min > 0 || a.gc_max < ps_k || a.max_t_run) ? 1u : 0u;

    // the work list: with targets, the tiles of the shard that hold a start of a range; without, every tile of the shard
    std::vector<uint32_t> work;
    uint32_t n_work = genome->d_hi ? genome->n_tiles : 0;
    if (targets) {
        const uint64_t first = a.first_pos, last = first + (uint64_t)n_work * kTileBases;  // the shard's starts: [first, last)
        for (const PatStartRange &r : ranges) {
            const uint64_t lo = std::max<uint64_t>(r.lo, first), hi = std::min<uint64_t>(r.hi, last);
            if (lo >= hi) continue;
            const uint32_t t0 = (uint32_t)((lo - first) / kTileBases), t1 = (uint32_t)((hi - 1 - first) / kTileBases);
            for (uint32_t t = t0; t <= t1; ++t)
                if (work.empty() || work.back() < t) work.push_back(t);  // (the ranges ascend)
        }
        n_work = (uint32_t)work.size();
    }
    // the ranges go to the device with the work list (with targets and a tile to visit there is a range)
    return run_enumeration(ctx, fn, a, targets ? &work : nullptr, n_work, ranges.data(), ranges.size() * sizeof(PatStartRange), params->max_guides, out,
                           [&](const void *d_ranges, unsigned long long total, bool write) {
                               a.ranges = (const uint2 *)d_ranges;
                               a.n_ranges = (uint32_t)ranges.size();
                               a.n_out = total;
                               return launch_pattern_enum(a, write, ctx->stream);
                           });
    });
}

uint64_t vsc_pattern_guides_count(const vsc_pattern_guides *guides) { return guides ? guides->n : 0; }
int vsc_pattern_guides_data(vsc_pattern_guides *guides, const uint64_t **codes, const vsc_locus **loci) { return guide_list_data(guides, codes, loci); }
int vsc_pattern_guides_data_dev(const vsc_pattern_guides *guides, const void **codes_dev, const void **loci_dev)
{
    return guide_list_data_dev(guides, codes_dev, loci_dev);
}
int vsc_pattern_guides_free(vsc_pattern_guides *guides) { return object_free(guides); }

int vsc_pattern_guide_text(uint64_t code, uint32_t len, uint32_t ps_start, uint32_t ps_len, uint32_t spell, char *out)
{
    return pattern_guide_text(code, len, ps_start, ps_len, spell, out);
}

int vsc_debug_pattern_target_ranges(const vsc_contig *contigs, uint32_t n_contigs, const vsc_interval *iv, uint64_t n, uint32_t rule,
                                    uint32_t len, uint32_t *ranges, uint64_t capacity, uint64_t *n_ranges)
{
    if ((n_contigs && !contigs) || !n_ranges || (capacity && !ranges) || len < kPatMinLen || len > kPatMaxLen) return VSC_ERR_INVALID;
    std::vector<uint32_t> off(n_contigs), end(n_contigs);
    for (uint32_t c = 0; c < n_contigs; ++c) {
        off[c] = (uint32_t)contigs[c].offset;
        end[c] = off[c] + contigs[c].length;
    }
    std::vector<PatStartRange> r;
    const int rc = pattern_target_ranges(off.data(), end.data(), n_contigs, iv, n, rule, len, &r);
    if (rc != VSC_OK) return rc;
    *n_ranges = r.size();
    if (r.size() > capacity) return VSC_ERR_RANGE;
    for (size_t i = 0; i < r.size(); ++i) {
        ranges[2 * i] = r[i].lo;
        ranges[2 * i + 1] = r[i].hi;
    }
    return VSC_OK;
}

int vsc_hits_locate(vsc_hits *hits, const vsc_regions *regions, uint32_t *labels)
{
    if (!hits || !regions || (hits->n && !labels)) return VSC_ERR_INVALID;
    if (hits->n == 0) return VSC_OK;
    return guarded(hits->ctx, [&]() -> int {
    return locate_records(hits->ctx, regions, hits->d_records, hits->n, true, labels, "vsc_hits_locate");
    });
}

int vsc_guides_locate(vsc_guides *guides, const vsc_regions *regions, uint32_t *labels)
{
    if (!guides || !regions || (guides->n && !labels)) return VSC_ERR_INVALID;
    if (guides->n == 0) return VSC_OK;
    if (!guides->ctx) {  // vsc_multi_guides_enumerate's host-only object: the same labels by the host's lookup
        if (!regions->has_locate) return VSC_ERR_RANGE;
        for (uint64_t i = 0; i < guides->n; ++i) {
            const vsc_locus &l = guides->loci[i];
            const bool whole = l.contig < regions->contig_len.size() && l.pos <= regions->contig_len[l.contig] &&
                               regions->contig_len[l.contig] - l.pos >= (uint32_t)VSC_READ_LEN;
            labels[i] = whole ? vsc_regions_locate(regions, l.contig, l.pos) : VSC_REGION_NONE;
        }
        return VSC_OK;
    }
    return guarded(guides->ctx, [&]() -> int {
    return locate_records(guides->ctx, regions, (const char *)guides->storage.p + guides->loci_at, guides->n, false, labels,
                          "vsc_guides_locate");
    });
}

}  // extern "C"

// ---- the host path of the candidate annotations ----------------------------------------------------------------
// What the families that annotate candidate guides - linear and tree efficiency, microhomology, edit windows, coding effects,
// prime editing, variation, HDR, the guide RNA's fold, motifs - do alike on the host: the checks in front of a call over candidates,
// the filter (staging, run_enumeration, the timing restated), the rows pass, and the join of the rows with a family's table (count pass, scan,
// write pass, coverage).  A family keeps its check, its table upload, the fields of its Args, its launchers and its stats;
// what differs between families enters here as a value or a callable of the family's.
namespace {

double wall_ms_since(std::chrono::steady_clock::time_point t0)
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// What a family tells candidate_front about itself.
struct CandidateRule {
    const char *need_23;   // the refusal of another site_len than 23 by a call over vsc_guides, with the family's noun
    uint64_t max_n;        // more candidates than this are refused ...
    const char *too_many;  // ... in these words
};

// Where the loci of a call's candidates lie: on the context's device already (dev), or on the host (host: uploaded first).
struct CandidateLoci {
    const void *dev;
    const vsc_locus *host;
    uint64_t n;
};

int no_refusal() { return VSC_OK; }

// The checks in front of every call over a candidate list, in their order: check() is the family's own check of its other
// arguments - the first, because it clears ctx->err -, after which *site_len is the site length the family works with;
// refuse() holds the refusals of the call's own parameters (no_refusal: it has none).  at = where the loci lie.
template <class Guides, class Check, class Refuse>
int candidate_front(vsc_ctx *ctx, Guides *guides, bool need_23, const CandidateRule &rule, const char *who, CandidateLoci &at,
                    const uint32_t *site_len, Check check, Refuse refuse)
{
    if (!ctx) return VSC_ERR_INVALID;
    const int rc = check();
    if (rc != VSC_OK) return rc;
    if (!guides) return fail_in(ctx, VSC_ERR_INVALID, who, "null argument");
    if (guides->ctx && guides->ctx != ctx) return fail_in(ctx, VSC_ERR_INVALID, who, "the candidates belong to another context");
    if (need_23 && *site_len != (uint32_t)VSC_READ_LEN) return fail_in(ctx, VSC_ERR_INVALID, who, rule.need_23);
    const int frc = refuse();
    if (frc != VSC_OK) return frc;
    if (guides->n > rule.max_n) return fail_in(ctx, VSC_ERR_RANGE, who, rule.too_many);
    const bool dev = guides->ctx != nullptr;  // (a host-only object: from the host)
    at = CandidateLoci{dev ? (const char *)guides->storage.p + guides->loci_at : nullptr, dev ? nullptr : guides->loci.data(), guides->n};
    return VSC_OK;
}

// candidate_front for a filter, whose result is null until there is one; on VSC_OK the context's device is the current one
template <class Guides, class Check, class Refuse>
int filter_front(vsc_ctx *ctx, Guides *in, Guides **out, bool need_23, const CandidateRule &rule, const char *who, const uint32_t *site_len,
                 Check check, Refuse refuse)
{
    if (!ctx || !out) return VSC_ERR_INVALID;
    *out = nullptr;
    CandidateLoci at{};
    const int rc = candidate_front(ctx, in, need_23, rule, who, at, site_len, check, refuse);
    if (rc != VSC_OK) return rc;
    VSC_HIP(ctx, hipSetDevice(ctx->device));
    return VSC_OK;
}

// The candidates of `in` that a family keeps, as a new object: run_enumeration's two passes over tiles of `tile` candidates
// (a host-only object: uploaded first, into eff_in); its timing is then restated as the scoring calls report theirs.  The
// family has filled the fields of `a` that are its own; launch(write) starts a pass.
template <class Guides, class Args, class Launch>
int filter_candidates(vsc_ctx *ctx, Guides *in, Args &a, uint32_t tile, Guides **out, const char *who, Launch launch)
{
    const uint64_t n = in->n;
    a.n = n;
    if (n && in->ctx) {
        a.in_codes = (const unsigned long long *)in->storage.p;
        a.in_loci = (const uint4 *)((const char *)in->storage.p + in->loci_at);
    } else if (n) {
        const size_t loci_at = round256((size_t)n * sizeof(uint64_t));
        VSC_HIP(ctx, ctx->eff_in.ensure(loci_at + (size_t)n * sizeof(vsc_locus)));
        char *base = (char *)ctx->eff_in.p;
        VSC_HIP(ctx, hipMemcpyAsync(base, in->codes.data(), (size_t)n * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
        VSC_HIP(ctx, hipMemcpyAsync(base + loci_at, in->loci.data(), (size_t)n * sizeof(vsc_locus), hipMemcpyHostToDevice, ctx->stream));
        a.in_codes = (const unsigned long long *)base;
        a.in_loci = (const uint4 *)(base + loci_at);
    }
    const int erc = run_enumeration(ctx, who, a, nullptr, (uint32_t)((n + tile - 1) / tile), nullptr, 0, 0, out,
                                    [&](const void *, unsigned long long, bool write) { return launch(write); });
    if (erc != VSC_OK) return erc;
    vsc_timing t{};
    t.score_ms = t.total_ms = ctx->timing.scan_ms;
    t.sites = n;
    t.genome_bytes = n * 2 * sizeof(vsc_locus) + (*out)->n * 2 * (sizeof(uint64_t) + sizeof(vsc_locus));
    ctx->timing = t;
    return VSC_OK;
}

// The rows pass of at.n > 0 candidates, enqueued on the context's stream: eff_out is laid out as a zeroed head of 256 bytes
// (the family's counters; what lies behind them in the head is scratch of the call) and the rows of row_bytes each, the loci
// are uploaded into eff_in where they lie on the host, launch(stats, rows, loci) starts the family's kernel between the stage
// events, and the rows (rows == null: not asked for) and the first n_seen counters are copied back.  Nothing is synchronised.
template <class Launch>
int rows_pass(vsc_ctx *ctx, const CandidateLoci &at, size_t row_bytes, void *rows, unsigned long long *seen, uint32_t n_seen, Launch launch)
{
    const size_t head = 256;
    VSC_HIP(ctx, ctx->eff_out.ensure(head + (size_t)at.n * row_bytes));
    unsigned long long *d_stats = (unsigned long long *)ctx->eff_out.p;
    void *d_rows = (char *)ctx->eff_out.p + head;
    const void *d_loci = at.dev;
    if (at.host) {
        VSC_HIP(ctx, ctx->eff_in.ensure((size_t)at.n * sizeof(vsc_locus)));
        VSC_HIP(ctx, hipMemcpyAsync(ctx->eff_in.p, at.host, (size_t)at.n * sizeof(vsc_locus), hipMemcpyHostToDevice, ctx->stream));
        d_loci = ctx->eff_in.p;
    }
    VSC_HIP(ctx, hipMemsetAsync(d_stats, 0, head, ctx->stream));
    VSC_HIP(ctx, hipEventRecord(ctx->ev[kEvStageStart], ctx->stream));
    VSC_HIP(ctx, launch(d_stats, d_rows, (const uint4 *)d_loci));
    VSC_HIP(ctx, hipEventRecord(ctx->ev[kEvStageEnd], ctx->stream));
    if (rows) VSC_HIP(ctx, hipMemcpyAsync(rows, d_rows, (size_t)at.n * row_bytes, hipMemcpyDeviceToHost, ctx->stream));
    VSC_HIP(ctx, hipMemcpyAsync(seen, d_stats, n_seen * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    return VSC_OK;
}

// What a rows pass reports as the call's timing; the pass has ended.  A join adds its passes as scan_ms.
int rows_timing(vsc_ctx *ctx, uint64_t n, size_t row_bytes, float pass_ms, float *rows_ms)
{
    VSC_HIP(ctx, hipEventElapsedTime(rows_ms, ctx->ev[kEvStageStart], ctx->ev[kEvStageEnd]));
    vsc_timing t{};
    t.score_ms = *rows_ms;
    t.scan_ms = pass_ms;
    t.total_ms = t.score_ms + t.scan_ms;
    t.sites = n;
    t.genome_bytes = n * (sizeof(vsc_locus) + row_bytes);
    ctx->timing = t;
    return VSC_OK;
}

// A scoring call's whole device work: the rows pass alone, waited for.  at.n > 0; rows is the caller's array; prepare() makes
// resident what the family's kernel reads beside the genome.
template <class Prepare, class Launch>
int score_rows(vsc_ctx *ctx, const CandidateLoci &at, size_t row_bytes, void *rows, unsigned long long *seen, uint32_t n_seen, float *rows_ms,
               const char *who, Prepare prepare, Launch launch)
{
    if (!rows) return fail_in(ctx, VSC_ERR_INVALID, who, "null argument");
    if (at.n > (1ull << 40)) return fail_in(ctx, VSC_ERR_RANGE, who, "more than 2^40 candidates");
    VSC_HIP(ctx, hipSetDevice(ctx->device));
    const int prc = prepare();
    if (prc != VSC_OK) return prc;
    const int rc = rows_pass(ctx, at, row_bytes, rows, seen, n_seen, launch);
    if (rc != VSC_OK) return rc;
    VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return rows_timing(ctx, at.n, row_bytes, 0.0f, rows_ms);
}

// the classes of the candidates, which every family's rows kernel counts first, into the family's stats
template <class Stats> void class_counts(Stats *stats, const unsigned long long *seen)
{
    stats->defined = seen[kEffDefined];
    stats->invalid = seen[kEffInvalid];
    stats->off_contig = seen[kEffOffContig];
    stats->not_resident = seen[kEffNotResident];
    stats->has_n = seen[kEffHasN];
}

// The part of edit_tabs that a join uses behind the family's own table: [coverage][pairs per tile][offsets per tile][extra],
// 256-byte aligned parts.  The family needs its size before the table is uploaded, and its place from the upload.
struct JoinTabs {
    uint32_t tiles;
    size_t cov_bytes, count_bytes, off_bytes, extra_bytes;
    char *base = nullptr;
    JoinTabs(uint64_t n, size_t cov, size_t extra)
        : tiles((uint32_t)((n + kEditTile - 1) / kEditTile)), cov_bytes(cov), count_bytes(round256((size_t)tiles * sizeof(uint32_t))),
          off_bytes(round256(((size_t)tiles + 1) * sizeof(unsigned long long))), extra_bytes(extra)
    {
    }
    size_t bytes() const { return cov_bytes + count_bytes + off_bytes + extra_bytes; }
    uint32_t *tile_count() const { return (uint32_t *)(base + cov_bytes); }
    unsigned long long *tile_off() const { return (unsigned long long *)(base + cov_bytes + count_bytes); }
    char *extra() const { return base + cov_bytes + count_bytes + off_bytes; }
};

// What a join is asked for, and what it found.
struct Join {
    uint64_t n;             // candidates (> 0)
    size_t row_bytes;       // of the rows pass in front of it, for the timing
    bool counted;           // false: the family's table is empty - no pass runs, there is no pair
    void *pairs;            // the caller's array (null: not asked for) of `capacity` pairs of pair_bytes each
    size_t pair_bytes;
    uint64_t capacity;
    uint64_t *n_pairs;      // the caller's (null: not asked for)
    uint64_t max_pairs;     // more are refused
    const char *too_many, *beyond_capacity;  // the two refusals, in the family's words
    unsigned long long total = 0;  // out: the pairs
    float rows_ms = 0;             // out: the rows pass
};

// The join of the rows with a family's table, behind a rows_pass that is still in flight: the count pass and the scan between
// the second pair of stage events, one 8-byte read-back (the pairs) and the first synchronise; then - where pairs are written
// or the coverage is counted - the write pass into edit_pairs, the pairs and the coverage copied back, the second synchronise;
// last the call's timing.  The family has bound its pair args to tabs.tile_count() and tabs.tile_off(); its callables:
// launch(pairs, write) starts a pass (pairs == null: the count pass, or a write pass for the coverage alone);
// wants_cover(too_many) says after the first synchronise whether the coverage is to be counted; clear_cover() binds and
// clears the family's coverage arrays; read_cover() enqueues what of them goes back.
// VSC_OK also where the pairs are refused: the family fills its stats, then returns join_refusal().
template <class Launch, class WantsCover, class ClearCover, class ReadCover>
int join_passes(vsc_ctx *ctx, const JoinTabs &tabs, Join &j, Launch launch, WantsCover wants_cover, ClearCover clear_cover, ReadCover read_cover)
{
    float pass_ms = 0;
    if (j.counted) {
        VSC_HIP(ctx, hipEventRecord(ctx->ev[kEvStage2Start], ctx->stream));
        VSC_HIP(ctx, launch((uint4 *)nullptr, false));
        VSC_HIP(ctx, launch_enum_scan(tabs.tile_count(), tabs.tiles, tabs.tile_off(), ctx->stream));
        VSC_HIP(ctx, hipEventRecord(ctx->ev[kEvStage2End], ctx->stream));
        VSC_HIP(ctx, hipMemcpyAsync(&j.total, tabs.tile_off() + tabs.tiles, sizeof j.total, hipMemcpyDeviceToHost, ctx->stream));
    }
    VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (j.counted) VSC_HIP(ctx, hipEventElapsedTime(&pass_ms, ctx->ev[kEvStage2Start], ctx->ev[kEvStage2End]));
    if (j.n_pairs) *j.n_pairs = j.total;
    const bool too_many = j.total > j.max_pairs, write = j.pairs && j.total && j.total <= j.capacity && !too_many;
    const bool cover = j.total && wants_cover(too_many);
    if (write || cover) {
        uint4 *d_pairs = nullptr;
        if (write) {
            VSC_HIP(ctx, ctx->edit_pairs.ensure((size_t)j.total * j.pair_bytes));
            d_pairs = (uint4 *)ctx->edit_pairs.p;
        }
        if (cover) {
            const int crc = clear_cover();
            if (crc != VSC_OK) return crc;
        }
        VSC_HIP(ctx, hipEventRecord(ctx->ev[kEvStage2Start], ctx->stream));
        VSC_HIP(ctx, launch(d_pairs, true));
        VSC_HIP(ctx, hipEventRecord(ctx->ev[kEvStage2End], ctx->stream));
        if (write) VSC_HIP(ctx, hipMemcpyAsync(j.pairs, d_pairs, (size_t)j.total * j.pair_bytes, hipMemcpyDeviceToHost, ctx->stream));
        if (cover) {
            const int rrc = read_cover();
            if (rrc != VSC_OK) return rrc;
        }
        VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        float wms = 0;
        VSC_HIP(ctx, hipEventElapsedTime(&wms, ctx->ev[kEvStage2Start], ctx->ev[kEvStage2End]));
        pass_ms += wms;
    }
    return rows_timing(ctx, j.n, j.row_bytes, pass_ms, &j.rows_ms);
}

// how a call with a join returns, its stats filled: the pairs it could not give are a refusal
int join_refusal(vsc_ctx *ctx, const Join &j, const char *who)
{
    if (j.total > j.max_pairs) return fail_in(ctx, VSC_ERR_RANGE, who, j.too_many);
    if (j.pairs && j.total > j.capacity) return fail_in(ctx, VSC_ERR_RANGE, who, j.beyond_capacity);
    return VSC_OK;
}

// The coverage of the edit, prime and effects joins: per entry of the family's table (a target, an edit, a transcript) its
// pairs and the smallest of a value over them, (0, undefined) without a pair; on the device two arrays at the front of the
// join's part of edit_tabs, for the caller interleaved.
struct PairCoverage {
    size_t n;                          // entries
    uint32_t *coverage;                // the caller's 2 n words (null: not asked for; the stats then want the covered entries alone)
    uint32_t *count = nullptr, *min = nullptr;  // device
    std::vector<uint32_t> host;        // both arrays as they come back
    unsigned long long d_covered = 0;  // the covered entries as the device counted them
    static size_t bytes(size_t entries) { return round256(entries * sizeof(uint32_t) + 4); }  // of one array

    PairCoverage(size_t n_entries, uint32_t *out, uint32_t undefined) : n(n_entries), coverage(out)
    {
        for (size_t k = 0; coverage && k < n; ++k) {
            coverage[2 * k] = 0;
            coverage[2 * k + 1] = undefined;
        }
    }
    int clear(vsc_ctx *ctx, const JoinTabs &tabs)
    {
        count = (uint32_t *)tabs.base;
        min = (uint32_t *)(tabs.base + bytes(n));
        VSC_HIP(ctx, hipMemsetAsync(count, 0, n * sizeof(uint32_t), ctx->stream));
        VSC_HIP(ctx, hipMemsetAsync(min, 0xFF, n * sizeof(uint32_t), ctx->stream));
        return VSC_OK;
    }
    // slot: 8 bytes inside the zeroed head of eff_out, behind the rows kernel's counters
    int read(vsc_ctx *ctx, unsigned long long *slot)
    {
        if (!coverage) {  // the stats alone: the covered entries are counted where they lie, 8 bytes come back
            VSC_HIP(ctx, launch_edit_covered(count, (uint32_t)n, slot, ctx->n_cus, ctx->stream));
            VSC_HIP(ctx, hipMemcpyAsync(&d_covered, slot, sizeof d_covered, hipMemcpyDeviceToHost, ctx->stream));
        } else {
            host.resize(2 * n);
            VSC_HIP(ctx, hipMemcpyAsync(host.data(), count, n * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
            VSC_HIP(ctx, hipMemcpyAsync(host.data() + n, min, n * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        }
        return VSC_OK;
    }
    // after the join: the caller's coverage filled, the covered entries
    uint64_t take()
    {
        uint64_t covered = d_covered;
        for (size_t k = 0; !host.empty() && k < n; ++k) {
            covered += host[k] != 0;
            coverage[2 * k] = host[k];
            coverage[2 * k + 1] = host[n + k];
        }
        return covered;
    }
};

}  // namespace

// ---- on-target efficiency (the definition: vsc_efficiency.h, the kernels: vsc_efficiency.hip) -------------------
namespace {

// The device copy of `model` on this context, as resident_table keeps the score table's: the copy of the model the context
// used last, keyed by its serial number; another model is uploaded over it on the context's stream.
int resident_eff_model(vsc_ctx *ctx, const vsc_eff_model *model, EffModelView &view)
{
    if (!(ctx->eff_serial == model->serial && ctx->eff_buf.p)) {
        ctx->eff_serial = 0;
        const size_t bytes = model->w.size() * sizeof(double);
        VSC_HIP(ctx, ctx->eff_buf.ensure(bytes));
        VSC_HIP(ctx, hipMemcpyAsync(ctx->eff_buf.p, model->w.data(), bytes, hipMemcpyHostToDevice, ctx->stream));
        VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (the caller may free the model as soon as its call returns)
        ctx->eff_serial = model->serial;
    }
    view = EffModelView{(const double *)ctx->eff_buf.p, model->intercept, model->shape, (uint32_t)model->w.size()};
    return VSC_OK;
}

// the planes of a resident genome as eff_context reads them (an object that carries the contig table only holds no word)
EffPlanes eff_planes(const vsc_genome *g)
{
    const bool planes = g->d_hi && g->d_lo && g->d_nm;
    return EffPlanes{g->d_hi, g->d_lo, g->d_nm, g->first_word, planes ? g->held_words : 0, planes ? g->dev_words : 0,
                     g->d_contig_off, g->d_contig_end, g->n_contigs};
}

int eff_check(vsc_ctx *ctx, const vsc_genome *genome, const vsc_eff_model *model, const char *who)
{
    ctx->err.clear();
    if (!genome || !model) return fail_in(ctx, VSC_ERR_INVALID, who, "null argument");
    if (genome->ctx != ctx) return fail_in(ctx, VSC_ERR_INVALID, who, "genome belongs to another context");
    return VSC_OK;
}

const CandidateRule kEffScoreRule{"the model's site_len must be 23", ~0ull, ""};  // (the scoring itself refuses above 2^40)
const CandidateRule kEffFilterRule{"the model's site_len must be 23", 0xFFFFFFFFull * kEffTile, "more candidates than 2^32 tiles hold"};
static_assert(kEffClasses * sizeof(unsigned long long) <= 256, "the class counts fit their part of eff_out");

// The predictors of the loci `at` into host memory: the model resident, eff_score_kernel, one copy back of the scores and one
// of the class counts.
int eff_score(vsc_ctx *ctx, const vsc_genome *genome, const vsc_eff_model *model, const CandidateLoci &at, double *linear, vsc_eff_stats *stats,
              const char *who)
{
    if (stats) *stats = vsc_eff_stats{};
    if (at.n == 0) {
        ctx->timing = vsc_timing{};
        return VSC_OK;
    }
    EffArgs a{};
    a.g = eff_planes(genome);
    a.n = at.n;
    unsigned long long seen[kEffClasses] = {};
    float ms = 0;
    const int rc = score_rows(
        ctx, at, sizeof(double), linear, seen, kEffClasses, &ms, who, [&] { return resident_eff_model(ctx, model, a.m); },
        [&](unsigned long long *d_stats, void *d_rows, const uint4 *d_loci) {
            a.stats = d_stats;
            a.linear = (double *)d_rows;
            a.loci = d_loci;
            return launch_eff_score(a, ctx->n_cus, ctx->stream);
        });
    if (rc != VSC_OK) return rc;
    if (stats) class_counts(stats, seen);
    return VSC_OK;
}

// vsc_guides_efficiency / vsc_pattern_guides_efficiency: over the candidates where they lie, a host-only object from the host
template <class Guides>
int eff_score_guides(vsc_ctx *ctx, const vsc_genome *genome, Guides *guides, const vsc_eff_model *model, bool need_23, double *linear,
                     vsc_eff_stats *stats, const char *who)
{
    return guarded(ctx, [&]() -> int {
    CandidateLoci at{};
    const int rc = candidate_front(ctx, guides, need_23, kEffScoreRule, who, at, model ? &model->shape.site_len : nullptr,
                                   [&] { return eff_check(ctx, genome, model, who); }, no_refusal);
    if (rc != VSC_OK) return rc;
    return eff_score(ctx, genome, model, at, linear, stats, who);
    });
}

// vsc_guides_filter_efficiency / vsc_pattern_guides_filter_efficiency: the candidates whose predictor is at least min_linear
template <class Guides>
int eff_filter(vsc_ctx *ctx, const vsc_genome *genome, Guides *in, const vsc_eff_model *model, bool need_23, double min_linear, Guides **out,
               const char *who)
{
    return guarded(ctx, [&]() -> int {
    const int rc = filter_front(
        ctx, in, out, need_23, kEffFilterRule, who, model ? &model->shape.site_len : nullptr,
        [&] { return eff_check(ctx, genome, model, who); },
        [&] { return std::isnan(min_linear) ? fail_in(ctx, VSC_ERR_INVALID, who, "min_linear is NaN") : VSC_OK; });
    if (rc != VSC_OK) return rc;
    EffFilterArgs a{};
    const int mrc = resident_eff_model(ctx, model, a.m);
    if (mrc != VSC_OK) return mrc;
    a.g = eff_planes(genome);
    a.min_linear = min_linear;
    return filter_candidates(ctx, in, a, kEffTile, out, who, [&](bool write) { return launch_eff_filter(a, write, ctx->stream); });
    });
}

}  // namespace

extern "C" {

int vsc_eff_model_build(const vsc_eff_shape *shape, double intercept, const double *mono, const double *di, const double *gc,
                        vsc_eff_model **out)
{
    if (!out) return VSC_ERR_INVALID;
    *out = nullptr;
    if (!shape || !mono || !di) return VSC_ERR_INVALID;
    if (shape->reserved[0] || shape->reserved[1] || shape->link > VSC_EFF_LOGISTIC) return VSC_ERR_INVALID;
    const EffShape s{shape->up, shape->site_len, shape->down, shape->gc_start, shape->gc_len};
    if (!eff_shape_valid(s) || (s.gc_len != 0) != (gc != nullptr)) return VSC_ERR_INVALID;
    return guarded(nullptr, [&]() -> int {
    static std::atomic<uint64_t> serial{0};
    std::unique_ptr<vsc_eff_model> m(new vsc_eff_model());
    const uint32_t C = eff_context_len(s);
    m->shape = s;
    m->link = shape->link;
    m->w.assign(eff_n_weights(s), 0.0);
    bool finite = std::isfinite(intercept);
    auto put = [&](uint32_t at, double v) {  // -0.0 is stored as +0.0: x is then never -0.0, and x + 0.0 keeps its bits
        finite = finite && std::isfinite(v);
        m->w[at] = v == 0.0 ? 0.0 : v;
        m->nonzero += v != 0.0;
    };
    for (uint32_t i = 0; i < 4 * C; ++i) put(i, mono[i]);
    for (uint32_t j = 0; j + 1 < C; ++j)
        for (uint32_t b0 = 0; b0 < 4; ++b0)
            for (uint32_t b1 = 0; b1 < 4; ++b1) put(eff_di_at(C) + 16 * j + b0 + 4 * b1, di[16 * j + 4 * b0 + b1]);
    for (uint32_t k = 0; s.gc_len && k <= s.gc_len; ++k) put(eff_gc_at(C) + k, gc[k]);
    if (!finite) return VSC_ERR_INVALID;
    m->intercept = intercept == 0.0 ? 0.0 : intercept;
    m->serial = serial.fetch_add(1, std::memory_order_relaxed) + 1;
    *out = m.release();
    return VSC_OK;
    });
}

int vsc_eff_model_free(vsc_eff_model *model)
{
    delete model;
    return VSC_OK;
}

int vsc_eff_model_info(const vsc_eff_model *model, vsc_eff_model_stats *out)
{
    if (!model || !out) return VSC_ERR_INVALID;
    const EffShape &s = model->shape;
    *out = vsc_eff_model_stats{model->serial, vsc_eff_shape{s.up, s.site_len, s.down, s.gc_start, s.gc_len, model->link, {0, 0}}, model->nonzero, 0};
    return VSC_OK;
}

int vsc_eff_score_text(const vsc_eff_model *model, const char *context, double *linear)
{
    if (!model || !context || !linear) return VSC_ERR_INVALID;
    const uint32_t C = eff_context_len(model->shape);
    if (strnlen(context, C + 1) != C) return VSC_ERR_INVALID;
    uint64_t ch = 0, cl = 0;
    *linear = eff_undefined();
    for (uint32_t j = 0; j < C; ++j) {
        const int b = base_code(context[j]);
        if (b > 3) return VSC_OK;
        ch |= (uint64_t)(b >> 1) << j;
        cl |= (uint64_t)(b & 1) << j;
    }
    *linear = eff_linear(model->w.data(), model->intercept, model->shape, ch, cl);
    return VSC_OK;
}

double vsc_eff_link(const vsc_eff_model *model, double linear)
{
    if (!model || std::isnan(linear)) return eff_undefined();
    return model->link == VSC_EFF_LOGISTIC ? 1.0 / (1.0 + std::exp(-linear)) : linear;
}

int vsc_loci_efficiency(vsc_ctx *ctx, const vsc_genome *genome, const vsc_locus *loci, uint64_t n, const vsc_eff_model *model,
                        double *linear, vsc_eff_stats *stats)
{
    return guarded(ctx, [&]() -> int {
    if (!ctx) return VSC_ERR_INVALID;
    const char *const fn = "vsc_loci_efficiency";
    const int rc = eff_check(ctx, genome, model, fn);
    if (rc != VSC_OK) return rc;
    if (n && !loci) return fail_in(ctx, VSC_ERR_INVALID, fn, "null argument");
    return eff_score(ctx, genome, model, CandidateLoci{nullptr, loci, n}, linear, stats, fn);
    });
}

int vsc_guides_efficiency(vsc_ctx *ctx, const vsc_genome *genome, vsc_guides *guides, const vsc_eff_model *model, double *linear,
                          vsc_eff_stats *stats)
{
    return eff_score_guides(ctx, genome, guides, model, true, linear, stats, "vsc_guides_efficiency");
}

int vsc_pattern_guides_efficiency(vsc_ctx *ctx, const vsc_genome *genome, vsc_pattern_guides *guides, const vsc_eff_model *model,
                                  double *linear, vsc_eff_stats *stats)
{
    return eff_score_guides(ctx, genome, guides, model, false, linear, stats, "vsc_pattern_guides_efficiency");
}

int vsc_guides_filter_efficiency(vsc_ctx *ctx, const vsc_genome *genome, vsc_guides *in, const vsc_eff_model *model, double min_linear,
                                 vsc_guides **out)
{
    return eff_filter(ctx, genome, in, model, true, min_linear, out, "vsc_guides_filter_efficiency");
}

int vsc_pattern_guides_filter_efficiency(vsc_ctx *ctx, const vsc_genome *genome, vsc_pattern_guides *in, const vsc_eff_model *model,
                                         double min_linear, vsc_pattern_guides **out)
{
    return eff_filter(ctx, genome, in, model, false, min_linear, out, "vsc_pattern_guides_filter_efficiency");
}

}  // extern "C"

// ---- on-target efficiency from regression-tree ensembles (the definition: vsc_eff_trees.h, the kernels:
// vsc_eff_trees.hip).  The calls are the linear model's, one for one, with another model and another kernel.
namespace {

// The device copy of `model` on this context, kept beside the linear model's and keyed by its own serial number.
int resident_eff_trees(vsc_ctx *ctx, const vsc_eff_trees *model, EffTreesView &view)
{
    if (!(ctx->eff_trees_serial == model->serial && ctx->eff_trees_buf.p)) {
        ctx->eff_trees_serial = 0;
        const size_t bytes = model->words.size() * sizeof(uint32_t);
        VSC_HIP(ctx, ctx->eff_trees_buf.ensure(bytes));
        VSC_HIP(ctx, hipMemcpyAsync(ctx->eff_trees_buf.p, model->words.data(), bytes, hipMemcpyHostToDevice, ctx->stream));
        VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (the caller may free the model as soon as its call returns)
        ctx->eff_trees_serial = model->serial;
    }
    view = EffTreesView{(const uint32_t *)ctx->eff_trees_buf.p, (uint32_t)model->words.size(), model->n_nodes, model->n_sums, model->n_trees,
                        model->base, model->shape};
    return VSC_OK;
}

int eff_trees_check(vsc_ctx *ctx, const vsc_genome *genome, const vsc_eff_trees *model, const char *who)
{
    ctx->err.clear();
    if (!genome || !model) return fail_in(ctx, VSC_ERR_INVALID, who, "null argument");
    if (genome->ctx != ctx) return fail_in(ctx, VSC_ERR_INVALID, who, "genome belongs to another context");
    return VSC_OK;
}

// eff_score with the tree model: the model resident, eff_trees_score_kernel, one copy back of the scores and one of the counts
int eff_trees_score(vsc_ctx *ctx, const vsc_genome *genome, const vsc_eff_trees *model, const CandidateLoci &at, double *linear,
                    vsc_eff_stats *stats, const char *who)
{
    if (stats) *stats = vsc_eff_stats{};
    if (at.n == 0) {
        ctx->timing = vsc_timing{};
        return VSC_OK;
    }
    EffTreesArgs a{};
    a.g = eff_planes(genome);
    a.n = at.n;
    unsigned long long seen[kEffClasses] = {};
    float ms = 0;
    const int rc = score_rows(
        ctx, at, sizeof(double), linear, seen, kEffClasses, &ms, who, [&] { return resident_eff_trees(ctx, model, a.m); },
        [&](unsigned long long *d_stats, void *d_rows, const uint4 *d_loci) {
            a.stats = d_stats;
            a.linear = (double *)d_rows;
            a.loci = d_loci;
            return launch_eff_trees_score(a, ctx->n_cus, ctx->stream);
        });
    if (rc != VSC_OK) return rc;
    if (stats) class_counts(stats, seen);
    return VSC_OK;
}

template <class Guides>
int eff_trees_score_guides(vsc_ctx *ctx, const vsc_genome *genome, Guides *guides, const vsc_eff_trees *model, bool need_23, double *linear,
                           vsc_eff_stats *stats, const char *who)
{
    return guarded(ctx, [&]() -> int {
    CandidateLoci at{};
    const int rc = candidate_front(ctx, guides, need_23, kEffScoreRule, who, at, model ? &model->shape.site_len : nullptr,
                                   [&] { return eff_trees_check(ctx, genome, model, who); }, no_refusal);
    if (rc != VSC_OK) return rc;
    return eff_trees_score(ctx, genome, model, at, linear, stats, who);
    });
}

template <class Guides>
int eff_trees_filter(vsc_ctx *ctx, const vsc_genome *genome, Guides *in, const vsc_eff_trees *model, bool need_23, double min_linear,
                     Guides **out, const char *who)
{
    return guarded(ctx, [&]() -> int {
    const int rc = filter_front(
        ctx, in, out, need_23, kEffFilterRule, who, model ? &model->shape.site_len : nullptr,
        [&] { return eff_trees_check(ctx, genome, model, who); },
        [&] { return std::isnan(min_linear) ? fail_in(ctx, VSC_ERR_INVALID, who, "min_linear is NaN") : VSC_OK; });
    if (rc != VSC_OK) return rc;
    EffTreesFilterArgs a{};
    const int mrc = resident_eff_trees(ctx, model, a.m);
    if (mrc != VSC_OK) return mrc;
    a.g = eff_planes(genome);
    a.min_linear = min_linear;
    return filter_candidates(ctx, in, a, kEffTile, out, who, [&](bool write) { return launch_eff_trees_filter(a, write, ctx->stream); });
    });
}

}  // namespace

extern "C" {

int vsc_eff_trees_build(const vsc_eff_shape *shape, double base, const vsc_eff_sum *sums, uint32_t n_sums, const vsc_eff_node *nodes,
                        const uint32_t *tree_first, uint32_t n_trees, vsc_eff_trees **out)
{
    if (!out) return VSC_ERR_INVALID;
    *out = nullptr;
    if (!shape || !nodes || !tree_first) return VSC_ERR_INVALID;
    if (shape->reserved[0] || shape->reserved[1] || shape->link > VSC_EFF_LOGISTIC) return VSC_ERR_INVALID;
    const EffShape s{shape->up, shape->site_len, shape->down, shape->gc_start, shape->gc_len};
    return guarded(nullptr, [&]() -> int {
    static std::atomic<uint64_t> serial{0};
    EffTreesBuilt built;
    if (!eff_trees_pack(s, base, sums, n_sums, nodes, tree_first, n_trees, built)) return VSC_ERR_INVALID;
    std::unique_ptr<vsc_eff_trees> m(new vsc_eff_trees());
    m->shape = s;
    m->link = shape->link;
    m->base = built.base;
    m->words = std::move(built.words);
    m->n_sums = n_sums;
    m->n_trees = n_trees;
    m->n_nodes = built.n_nodes;
    for (int k = 0; k < 4; ++k) m->by_kind[k] = built.by_kind[k];
    m->max_depth = built.max_depth;
    m->serial = serial.fetch_add(1, std::memory_order_relaxed) + 1;
    *out = m.release();
    return VSC_OK;
    });
}

int vsc_eff_trees_free(vsc_eff_trees *model)
{
    delete model;
    return VSC_OK;
}

int vsc_eff_trees_info(const vsc_eff_trees *model, vsc_eff_trees_stats *out)
{
    if (!model || !out) return VSC_ERR_INVALID;
    const EffShape &s = model->shape;
    *out = vsc_eff_trees_stats{model->serial, vsc_eff_shape{s.up, s.site_len, s.down, 0, 0, model->link, {0, 0}}, model->n_sums, model->n_trees,
                               model->n_nodes, model->by_kind[VSC_EFF_NODE_LEAF], model->by_kind[VSC_EFF_NODE_BASE],
                               model->by_kind[VSC_EFF_NODE_PAIR], model->by_kind[VSC_EFF_NODE_SUM], model->max_depth, {0, 0}};
    return VSC_OK;
}

int vsc_eff_trees_score_text(const vsc_eff_trees *model, const char *context, double *linear)
{
    if (!model || !context || !linear) return VSC_ERR_INVALID;
    const uint32_t C = eff_context_len(model->shape);
    if (strnlen(context, C + 1) != C) return VSC_ERR_INVALID;
    uint64_t ch = 0, cl = 0;
    *linear = eff_undefined();
    for (uint32_t j = 0; j < C; ++j) {
        const int b = base_code(context[j]);
        if (b > 3) return VSC_OK;
        ch |= (uint64_t)(b >> 1) << j;
        cl |= (uint64_t)(b & 1) << j;
    }
    const EffTreesPacked m{model->words.data(), model->n_nodes, model->n_sums, model->n_trees, model->base};
    int32_t S[kEffTreesMaxSums] = {};
    eff_trees_sums(m, C, ch, cl, S, 1);
    *linear = eff_trees_predict(m, ch, cl, S, 1);
    return VSC_OK;
}

double vsc_eff_trees_link(const vsc_eff_trees *model, double linear)
{
    if (!model || std::isnan(linear)) return eff_undefined();
    return model->link == VSC_EFF_LOGISTIC ? 1.0 / (1.0 + std::exp(-linear)) : linear;
}

int vsc_loci_efficiency_trees(vsc_ctx *ctx, const vsc_genome *genome, const vsc_locus *loci, uint64_t n, const vsc_eff_trees *model,
                              double *linear, vsc_eff_stats *stats)
{
    return guarded(ctx, [&]() -> int {
    if (!ctx) return VSC_ERR_INVALID;
    const char *const fn = "vsc_loci_efficiency_trees";
    const int rc = eff_trees_check(ctx, genome, model, fn);
    if (rc != VSC_OK) return rc;
    if (n && !loci) return fail_in(ctx, VSC_ERR_INVALID, fn, "null argument");
    return eff_trees_score(ctx, genome, model, CandidateLoci{nullptr, loci, n}, linear, stats, fn);
    });
}

int vsc_guides_efficiency_trees(vsc_ctx *ctx, const vsc_genome *genome, vsc_guides *guides, const vsc_eff_trees *model, double *linear,
                                vsc_eff_stats *stats)
{
    return eff_trees_score_guides(ctx, genome, guides, model, true, linear, stats, "vsc_guides_efficiency_trees");
}

int vsc_pattern_guides_efficiency_trees(vsc_ctx *ctx, const vsc_genome *genome, vsc_pattern_guides *guides, const vsc_eff_trees *model,
                                        double *linear, vsc_eff_stats *stats)
{
    return eff_trees_score_guides(ctx, genome, guides, model, false, linear, stats, "vsc_pattern_guides_efficiency_trees");
}

int vsc_guides_filter_efficiency_trees(vsc_ctx *ctx, const vsc_genome *genome, vsc_guides *in, const vsc_eff_trees *model, double min_linear,
                                       vsc_guides **out)
{
    return eff_trees_filter(ctx, genome, in, model, true, min_linear, out, "vsc_guides_filter_efficiency_trees");
}

int vsc_pattern_guides_filter_efficiency_trees(vsc_ctx *ctx, const vsc_genome *genome, vsc_pattern_guides *in, const vsc_eff_trees *model,
                                               double min_linear, vsc_pattern_guides **out)
{
    return eff_trees_filter(ctx, genome, in, model, false, min_linear, out, "vsc_pattern_guides_filter_efficiency_trees");
}

}  // extern "C"

// ---- microhomology and out-of-frame scores (the definition: vsc_mh.h, the kernels: vsc_mh.hip) ------------------
namespace {

int mh_check(vsc_ctx *ctx, const vsc_genome *genome, const vsc_mh_shape *shape, MhShape &s, const char *who)
{
    ctx->err.clear();
    if (!genome || !shape) return fail_in(ctx, VSC_ERR_INVALID, who, "null argument");
    if (genome->ctx != ctx) return fail_in(ctx, VSC_ERR_INVALID, who, "genome belongs to another context");
    s = MhShape{shape->site_len, shape->cut, shape->flank};
    if (shape->reserved || !mh_shape_valid(s)) return fail_in(ctx, VSC_ERR_INVALID, who, "site_len 16 .. 32, cut 0 .. site_len, flank 8 .. 32");
    return VSC_OK;
}

const CandidateRule kMhScoreRule{"the shape's site_len must be 23", ~0ull, ""};  // (the scoring itself refuses above 2^40)
const CandidateRule kMhFilterRule{"the shape's site_len must be 23", 0xFFFFFFFFull * kMhTile, "more candidates than 2^32 tiles hold"};

// The pairs of the loci `at` into host memory: mh_score_kernel, one copy back of the pairs and one of the class counts.
int mh_score_loci(vsc_ctx *ctx, const vsc_genome *genome, const MhShape &shape, const CandidateLoci &at, uint32_t *pairs, vsc_mh_stats *stats,
                  const char *who)
{
    const auto t0 = std::chrono::steady_clock::now();
    if (stats) *stats = vsc_mh_stats{};
    if (at.n == 0) {
        ctx->timing = vsc_timing{};
        return VSC_OK;
    }
    MhArgs a{};
    a.g = eff_planes(genome);
    a.shape = shape;
    a.n = at.n;
    unsigned long long seen[kEffClasses] = {};
    float ms = 0;
    const int rc = score_rows(
        ctx, at, sizeof(uint2), pairs, seen, kEffClasses, &ms, who, [] { return VSC_OK; },
        [&](unsigned long long *d_stats, void *d_rows, const uint4 *d_loci) {
            a.stats = d_stats;
            a.out = (uint2 *)d_rows;
            a.loci = d_loci;
            return launch_mh_score(a, ctx->n_cus, ctx->stream);
        });
    if (rc != VSC_OK) return rc;
    if (stats) {
        class_counts(stats, seen);
        stats->kernel_ms = ms;
        stats->wall_ms = wall_ms_since(t0);
    }
    return VSC_OK;
}

// vsc_guides_microhomology / vsc_pattern_guides_microhomology: over the candidates where they lie, a host-only object from the host
template <class Guides>
int mh_score_guides(vsc_ctx *ctx, const vsc_genome *genome, Guides *guides, const vsc_mh_shape *shape, bool need_23, uint32_t *pairs,
                    vsc_mh_stats *stats, const char *who)
{
    return guarded(ctx, [&]() -> int {
    MhShape s{};
    CandidateLoci at{};
    const int rc = candidate_front(ctx, guides, need_23, kMhScoreRule, who, at, &s.site_len,
                                   [&] { return mh_check(ctx, genome, shape, s, who); }, no_refusal);
    if (rc != VSC_OK) return rc;
    return mh_score_loci(ctx, genome, s, at, pairs, stats, who);
    });
}

// vsc_guides_filter_microhomology / vsc_pattern_guides_filter_microhomology: the candidates within the two bounds
template <class Guides>
int mh_filter(vsc_ctx *ctx, const vsc_genome *genome, Guides *in, const vsc_mh_shape *shape, bool need_23, uint32_t min_sum,
              uint32_t min_oof_permille, Guides **out, const char *who)
{
    return guarded(ctx, [&]() -> int {
    MhShape s{};
    const int rc = filter_front(
        ctx, in, out, need_23, kMhFilterRule, who, &s.site_len,
        [&] { return mh_check(ctx, genome, shape, s, who); },
        [&] { return min_oof_permille > 1000u ? fail_in(ctx, VSC_ERR_INVALID, who, "min_oof_permille is more than 1000") : VSC_OK; });
    if (rc != VSC_OK) return rc;
    MhFilterArgs a{};
    a.g = eff_planes(genome);
    a.shape = s;
    a.min_sum = min_sum;
    a.min_oof_permille = min_oof_permille;
    return filter_candidates(ctx, in, a, kMhTile, out, who, [&](bool write) { return launch_mh_filter(a, write, ctx->stream); });
    });
}

}  // namespace

extern "C" {

int vsc_mh_score_text(const char *context, uint32_t flank, uint32_t *sum, uint32_t *oof)
{
    if (!context || !sum || !oof) return VSC_ERR_INVALID;
    if (flank < kMhMinFlank || flank > kMhMaxFlank) return VSC_ERR_INVALID;
    const uint32_t W = 2u * flank;
    if (strnlen(context, W + 1) != W) return VSC_ERR_INVALID;
    uint64_t ch = 0, cl = 0;
    *sum = *oof = kMhUndefined;
    for (uint32_t j = 0; j < W; ++j) {
        const int b = base_code(context[j]);
        if (b > 3) return VSC_OK;
        ch |= (uint64_t)(b >> 1) << j;
        cl |= (uint64_t)(b & 1) << j;
    }
    mh_score(ch, cl, flank, sum, oof);
    return VSC_OK;
}

int vsc_mh_scores(uint32_t sum, uint32_t oof, double *mh_score_out, double *oof_score_out)
{
    if (!mh_score_out || !oof_score_out) return VSC_ERR_INVALID;
    if (sum == kMhUndefined || oof > sum) {
        *mh_score_out = *oof_score_out = eff_undefined();
        return sum == kMhUndefined && oof == kMhUndefined ? VSC_OK : VSC_ERR_INVALID;
    }
    *mh_score_out = (double)sum / 10.0;
    *oof_score_out = sum ? 100.0 * (double)oof / (double)sum : 0.0;
    return VSC_OK;
}

int vsc_loci_microhomology(vsc_ctx *ctx, const vsc_genome *genome, const vsc_locus *loci, uint64_t n, const vsc_mh_shape *shape,
                           uint32_t *pairs, vsc_mh_stats *stats)
{
    return guarded(ctx, [&]() -> int {
    if (!ctx) return VSC_ERR_INVALID;
    const char *const fn = "vsc_loci_microhomology";
    MhShape s{};
    const int rc = mh_check(ctx, genome, shape, s, fn);
    if (rc != VSC_OK) return rc;
    if (n && !loci) return fail_in(ctx, VSC_ERR_INVALID, fn, "null argument");
    return mh_score_loci(ctx, genome, s, CandidateLoci{nullptr, loci, n}, pairs, stats, fn);
    });
}

int vsc_guides_microhomology(vsc_ctx *ctx, const vsc_genome *genome, vsc_guides *guides, const vsc_mh_shape *shape, uint32_t *pairs,
                             vsc_mh_stats *stats)
{
    return mh_score_guides(ctx, genome, guides, shape, true, pairs, stats, "vsc_guides_microhomology");
}

int vsc_pattern_guides_microhomology(vsc_ctx *ctx, const vsc_genome *genome, vsc_pattern_guides *guides, const vsc_mh_shape *shape,
                                     uint32_t *pairs, vsc_mh_stats *stats)
{
    return mh_score_guides(ctx, genome, guides, shape, false, pairs, stats, "vsc_pattern_guides_microhomology");
}

int vsc_guides_filter_microhomology(vsc_ctx *ctx, const vsc_genome *genome, vsc_guides *in, const vsc_mh_shape *shape, uint32_t min_sum,
                                    uint32_t min_oof_permille, vsc_guides **out)
{
    return mh_filter(ctx, genome, in, shape, true, min_sum, min_oof_permille, out, "vsc_guides_filter_microhomology");
}

int vsc_pattern_guides_filter_microhomology(vsc_ctx *ctx, const vsc_genome *genome, vsc_pattern_guides *in, const vsc_mh_shape *shape,
                                            uint32_t min_sum, uint32_t min_oof_permille, vsc_pattern_guides **out)
{
    return mh_filter(ctx, genome, in, shape, false, min_sum, min_oof_permille, out, "vsc_pattern_guides_filter_microhomology");
}

}  // extern "C"

namespace {

template <class Guides> int guides_from_host(vsc_ctx *ctx, const uint64_t *codes, const vsc_locus *loci, uint64_t n, Guides **out)
{
    if (!out) return VSC_ERR_INVALID;
    *out = nullptr;
    if (n && (!codes || !loci)) return VSC_ERR_INVALID;
    return guarded(ctx, [&]() -> int {
    std::unique_ptr<Guides, int (*)(Guides *)> g(new Guides(), object_free<Guides>);
    g->n = n;
    g->codes.assign(codes, codes + n);
    g->loci.assign(loci, loci + n);
    g->host_valid = true;
    if (ctx && n) {
        VSC_HIP(ctx, hipSetDevice(ctx->device));
        g->ctx = ctx;
        g->loci_at = round256((size_t)n * sizeof(uint64_t));
        VSC_HIP(ctx, g->storage.ensure(g->loci_at + (size_t)n * sizeof(vsc_locus)));
        VSC_HIP(ctx, hipMemcpyAsync(g->storage.p, codes, (size_t)n * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
        VSC_HIP(ctx, hipMemcpyAsync((char *)g->storage.p + g->loci_at, loci, (size_t)n * sizeof(vsc_locus), hipMemcpyHostToDevice, ctx->stream));
        VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    g->ctx = ctx;
    *out = g.release();
    return VSC_OK;
    });
}

}  // namespace

extern "C" {

int vsc_debug_guides_from_host(vsc_ctx *ctx, const uint64_t *codes, const vsc_locus *loci, uint64_t n, vsc_guides **out)
{
    return guides_from_host(ctx, codes, loci, n, out);
}

int vsc_debug_pattern_guides_from_host(vsc_ctx *ctx, const uint64_t *codes, const vsc_locus *loci, uint64_t n, vsc_pattern_guides **out)
{
    return guides_from_host(ctx, codes, loci, n, out);
}

}  // extern "C"

// ---- the best K guides per target, with spacing (the definition: vsc_pick.h, the kernels: vsc_pick.hip) ----------
namespace {

int pick_check(vsc_ctx *ctx, const vsc_pick_params *params, PickShape &s, const char *who)
{
    if (!params) return fail_in(ctx, VSC_ERR_INVALID, who, "null argument");
    s = PickShape{params->site_len, params->cut, params->k, params->spacing, params->min_key};
    if (params->reserved || !pick_shape_valid(s))
        return fail_in(ctx, VSC_ERR_INVALID, who, "site_len 16 .. 32, cut 0 .. site_len, k 1 .. 32, reserved 0");
    return VSC_OK;
}

// vsc::pick_host (vsc_pick.h: the definition as host code) with its counts as a vsc_pick_stats
void pick_host_stats(const PickShape &s, const uint32_t *contig_len, uint32_t n_contigs, const vsc_locus *loci, uint64_t n, const uint32_t *target,
                     const uint64_t *key, uint32_t n_targets, uint32_t *picks, uint32_t *counts, uint32_t *rank, vsc_pick_stats *stats)
{
    static_assert(sizeof(vsc_locus) == sizeof(PickLocus), "vsc_locus is four 32-bit words");
    uint64_t seen[kPickStats] = {};
    pick_host(s, contig_len, n_contigs, (const PickLocus *)loci, n, target, key, n_targets, picks, counts, rank, seen);
    if (stats) {
        stats->eligible = seen[kPickEligible];
        stats->invalid = seen[kPickInvalid];
        stats->no_target = seen[kPickNoTarget];
        stats->bad_target = seen[kPickBadTarget];
        stats->below_min_key = seen[kPickBelowMinKey];
        stats->targets_picked = seen[kPickStatTargets];
        stats->targets_short = seen[kPickStatShort];
        stats->picks = seen[kPickStatPicks];
    }
}

// The gather of the picked candidates of a host-only object, in ascending index
template <class Guides> int pick_gather_host(const Guides *in, const uint32_t *rank, Guides **picked)
{
    std::unique_ptr<Guides, int (*)(Guides *)> g(new Guides(), object_free<Guides>);
    for (uint64_t i = 0; i < in->n; ++i)
        if (rank[i] != kPickNone) {
            g->codes.push_back(in->codes[i]);
            g->loci.push_back(in->loci[i]);
        }
    g->n = g->codes.size();
    g->host_valid = true;
    *picked = g.release();
    return VSC_OK;
}

// What a device call picks from: the loci on ctx's device already (d_loci) or the host's (h_loci: uploaded first), the keys
// (host), and either the targets (host) or the regions (+ group, host).
struct PickInput {
    const void *d_loci = nullptr;
    const vsc_locus *h_loci = nullptr;
    uint64_t n = 0;
    const uint64_t *key = nullptr;
    const uint32_t *target = nullptr;
    const vsc_regions *regions = nullptr;
    const uint32_t *group = nullptr;
    uint32_t n_targets = 0;
};

// Mark + scan, one 8-byte read-back (the eligible candidates: it sizes the records), scatter, select, rank; picks, counts, rank
// and the stats to the host.  *d_rank (optional) = the ranks on the device afterwards, for the `picked` passes.
int pick_device(vsc_ctx *ctx, const vsc_genome *genome, const PickShape &s, const PickInput &in, uint32_t *picks, uint32_t *counts, uint32_t *rank,
                bool want_rank, const uint32_t **d_rank, vsc_pick_stats *stats, const char *who)
{
    const uint64_t n = in.n;
    const uint32_t nt = in.n_targets;
    VSC_HIP(ctx, hipSetDevice(ctx->device));
    PickArgs a{};
    a.shape = s;
    a.n = n;
    a.n_targets = nt;
    a.contig_off = genome->d_contig_off;
    a.contig_end = genome->d_contig_end;
    a.n_contigs = genome->n_contigs;
    size_t n_group = 0;
    if (in.regions) {
        LocateArgs la{};
        const int lrc = resident_locate(ctx, in.regions, la, who);
        if (lrc != VSC_OK) return lrc;
        a.reg = la.reg;
        a.loc = la.loc;
        if (in.group) n_group = (size_t)in.regions->n_input;
    }
    // uploads: [keys][targets or groups][loci], 256-byte aligned parts
    const size_t key_bytes = round256((size_t)n * sizeof(uint64_t));
    const size_t tg_bytes = round256((in.target ? (size_t)n : n_group) * sizeof(uint32_t));
    VSC_HIP(ctx, ctx->pick_in.ensure(key_bytes + tg_bytes + (in.h_loci ? (size_t)n * sizeof(vsc_locus) : 0) + 256));
    char *ib = (char *)ctx->pick_in.p;
    VSC_HIP(ctx, hipMemcpyAsync(ib, in.key, (size_t)n * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
    a.key = (const unsigned long long *)ib;
    if (in.target) {
        VSC_HIP(ctx, hipMemcpyAsync(ib + key_bytes, in.target, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        a.target = (const uint32_t *)(ib + key_bytes);
    } else if (n_group) {
        VSC_HIP(ctx, hipMemcpyAsync(ib + key_bytes, in.group, n_group * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        a.group = (const uint32_t *)(ib + key_bytes);
        a.n_group = (uint32_t)n_group;
    }
    if (in.h_loci) {
        VSC_HIP(ctx, hipMemcpyAsync(ib + key_bytes + tg_bytes, in.h_loci, (size_t)n * sizeof(vsc_locus), hipMemcpyHostToDevice, ctx->stream));
        a.loci = (const uint4 *)(ib + key_bytes + tg_bytes);
    } else {
        a.loci = (const uint4 *)in.d_loci;
    }
    // tables: [stats][count][cursor] (zeroed together) [segment offsets][tgt][picks][counts][rank]
    const size_t stats_bytes = 256, cnt_bytes = round256(((size_t)nt + 1) * sizeof(uint32_t));
    const size_t off_bytes = round256(((size_t)nt + 1) * sizeof(unsigned long long)), tgt_bytes = round256((size_t)n * sizeof(uint32_t));
    const size_t picks_bytes = round256((size_t)nt * s.k * sizeof(uint32_t) + 4);
    VSC_HIP(ctx, ctx->pick_tabs.ensure(stats_bytes + 3 * cnt_bytes + off_bytes + 2 * tgt_bytes + picks_bytes));
    char *tb = (char *)ctx->pick_tabs.p;
    a.stats = (unsigned long long *)tb;
    a.count = (uint32_t *)(tb + stats_bytes);
    a.cursor = (uint32_t *)(tb + stats_bytes + cnt_bytes);
    unsigned long long *const d_off = (unsigned long long *)(tb + stats_bytes + 2 * cnt_bytes);
    a.seg_off = d_off;
    a.tgt = (uint32_t *)(tb + stats_bytes + 2 * cnt_bytes + off_bytes);
    a.picks = (uint32_t *)(tb + stats_bytes + 2 * cnt_bytes + off_bytes + tgt_bytes);
    a.counts = (uint32_t *)(tb + stats_bytes + 2 * cnt_bytes + off_bytes + tgt_bytes + picks_bytes);
    a.rank = (uint32_t *)(tb + stats_bytes + 3 * cnt_bytes + off_bytes + tgt_bytes + picks_bytes);
    VSC_HIP(ctx, hipMemsetAsync(tb, 0, stats_bytes + 2 * cnt_bytes, ctx->stream));
    hipEvent_t *const ev = ctx->ev;  // five marks: the first five events of the context
    VSC_HIP(ctx, hipEventRecord(ev[0], ctx->stream));
    VSC_HIP(ctx, launch_pick_mark(a, ctx->n_cus, ctx->stream));
    VSC_HIP(ctx, launch_enum_scan(a.count, nt, d_off, ctx->stream));
    VSC_HIP(ctx, hipEventRecord(ev[1], ctx->stream));
    unsigned long long n_rec = 0;
    VSC_HIP(ctx, hipMemcpyAsync(&n_rec, d_off + nt, sizeof n_rec, hipMemcpyDeviceToHost, ctx->stream));
    VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (n_rec > n) return fail_in(ctx, VSC_ERR_DEVICE, who, "more eligible candidates than candidates");
    const size_t rec_bytes = round256((size_t)n_rec * sizeof(uint4));
    VSC_HIP(ctx, ctx->pick_recs.ensure(rec_bytes + (size_t)n_rec * sizeof(uint32_t) + 256));
    a.rec = (uint4 *)ctx->pick_recs.p;
    a.rec_index = (uint32_t *)((char *)ctx->pick_recs.p + rec_bytes);
    a.n_rec = n_rec;
    VSC_HIP(ctx, launch_pick_scatter(a, ctx->n_cus, ctx->stream));
    VSC_HIP(ctx, hipEventRecord(ev[2], ctx->stream));
    VSC_HIP(ctx, launch_pick_select(a, ctx->n_cus, ctx->stream));
    VSC_HIP(ctx, hipEventRecord(ev[3], ctx->stream));
    if (want_rank) {
        VSC_HIP(ctx, hipMemsetAsync(a.rank, 0xFF, (size_t)n * sizeof(uint32_t), ctx->stream));
        VSC_HIP(ctx, launch_pick_rank(a, ctx->n_cus, ctx->stream));
    }
    VSC_HIP(ctx, hipEventRecord(ev[4], ctx->stream));
    unsigned long long seen[kPickStats] = {};
    if (nt) {
        VSC_HIP(ctx, hipMemcpyAsync(picks, a.picks, (size_t)nt * s.k * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        VSC_HIP(ctx, hipMemcpyAsync(counts, a.counts, (size_t)nt * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    }
    if (rank) VSC_HIP(ctx, hipMemcpyAsync(rank, a.rank, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    VSC_HIP(ctx, hipMemcpyAsync(seen, a.stats, sizeof seen, hipMemcpyDeviceToHost, ctx->stream));
    VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (d_rank) *d_rank = a.rank;
    float ms[4] = {};
    for (int i = 0; i < 4; ++i) VSC_HIP(ctx, hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]));
    if (stats) {
        stats->eligible = seen[kPickEligible];
        stats->invalid = seen[kPickInvalid];
        stats->no_target = seen[kPickNoTarget];
        stats->bad_target = seen[kPickBadTarget];
        stats->below_min_key = seen[kPickBelowMinKey];
        stats->targets_picked = seen[kPickStatTargets];
        stats->targets_short = seen[kPickStatShort];
        stats->picks = seen[kPickStatPicks];
        for (int i = 0; i < 4; ++i) stats->stage_ms[i] = ms[i];
        stats->kernel_ms = (double)ms[0] + ms[1] + ms[2] + ms[3];
    }
    vsc_timing t{};
    t.score_ms = t.total_ms = ms[0] + ms[1] + ms[2] + ms[3];
    t.sites = n;
    // DESIGN 4.27's floors: mark reads 16 + 8 and writes 4 per candidate; scatter reads 16 + 8 + 4 per candidate and writes 20 per
    // record; select reads 20 per record and writes 4 k + 4 per target
    t.genome_bytes = n * 28 + (n * 28 + n_rec * 20) + (n_rec * 20 + (uint64_t)nt * (4 * s.k + 4));
    ctx->timing = t;
    return VSC_OK;
}

// the checks every call shares; nothing is written
int pick_front(vsc_ctx *ctx, const vsc_pick_params *params, PickShape &s, uint64_t n, uint32_t n_targets, const uint64_t *key, uint32_t *picks,
               uint32_t *counts, const char *who)
{
    const int rc = pick_check(ctx, params, s, who);
    if (rc != VSC_OK) return rc;
    if ((n_targets && (!picks || !counts)) || (n && !key)) return fail_in(ctx, VSC_ERR_INVALID, who, "null argument");
    if (n > kPickMaxCandidates) return fail_in(ctx, VSC_ERR_RANGE, who, "more than 0xFFFFFFFE candidates");
    return VSC_OK;
}

// behind every refusal: the stats zeroed; true: n == 0, the outputs are written and the call is done
bool pick_begin(const PickShape &s, uint64_t n, uint32_t n_targets, uint32_t *picks, uint32_t *counts, uint32_t *rank, vsc_pick_stats *stats)
{
    if (stats) *stats = vsc_pick_stats{};
    if (n == 0) pick_outputs_empty(s, 0, n_targets, picks, counts, rank);
    return n == 0;
}

// regions (+ group) as a call's targets: built for the genome's contig table, with the label structure, every group entry a
// target or VSC_REGION_NONE
int pick_regions_check(vsc_ctx *ctx, const vsc_genome *genome, const vsc_regions *regions, const uint32_t *group, uint32_t n_targets, const char *who)
{
    bool same = regions->contig_off.size() == genome->n_contigs;
    for (uint32_t c = 0; same && c < genome->n_contigs; ++c)
        same = genome->h_contig_off[c] == regions->contig_off[c] && genome->h_contig_end[c] - genome->h_contig_off[c] == regions->contig_len[c];
    if (!same) return fail_in(ctx, VSC_ERR_INVALID, who, "the regions were built for another contig table");
    if (!regions->has_locate) return fail_in(ctx, VSC_ERR_RANGE, who, "the regions hold more intervals than a 32-bit label can number");
    if (group)
        for (uint64_t j = 0; j < regions->n_input; ++j)
            if (group[j] != kPickNone && group[j] >= n_targets)
                return fail_in(ctx, VSC_ERR_INVALID, who, "a group entry is neither a target nor VSC_REGION_NONE");
    return VSC_OK;
}

// vsc_guides_pick / vsc_pattern_guides_pick
template <class Guides>
int pick_guides(vsc_ctx *ctx, const vsc_genome *genome, Guides *guides, const vsc_regions *regions, const uint32_t *group, const uint32_t *target,
                uint32_t n_targets, const uint64_t *key, const vsc_pick_params *params, bool need_23, uint32_t *picks, uint32_t *counts,
                uint32_t *rank, Guides **picked, vsc_pick_stats *stats, const char *who)
{
    return guarded(ctx, [&]() -> int {
    if (!ctx) return VSC_ERR_INVALID;
    const auto t0 = std::chrono::steady_clock::now();
    ctx->err.clear();
    if (picked) *picked = nullptr;
    if (!genome || !guides) return fail_in(ctx, VSC_ERR_INVALID, who, "null argument");
    if (genome->ctx != ctx) return fail_in(ctx, VSC_ERR_INVALID, who, "genome belongs to another context");
    if (guides->ctx && guides->ctx != ctx) return fail_in(ctx, VSC_ERR_INVALID, who, "the candidates belong to another context");
    PickShape s{};
    const uint64_t n = guides->n;
    const int rc = pick_front(ctx, params, s, n, n_targets, key, picks, counts, who);
    if (rc != VSC_OK) return rc;
    if (need_23 && s.site_len != (uint32_t)VSC_READ_LEN) return fail_in(ctx, VSC_ERR_INVALID, who, "the shape's site_len must be 23");
    if ((regions != nullptr) == (target != nullptr)) return fail_in(ctx, VSC_ERR_INVALID, who, "exactly one of regions and target must be given");
    if (group && !regions) return fail_in(ctx, VSC_ERR_INVALID, who, "a group needs regions");
    if (regions) {
        const int grc = pick_regions_check(ctx, genome, regions, group, n_targets, who);
        if (grc != VSC_OK) return grc;
    }
    if (pick_begin(s, n, n_targets, picks, counts, rank, stats)) {
        if (picked) {
            std::unique_ptr<Guides, int (*)(Guides *)> g(new Guides(), object_free<Guides>);
            g->ctx = guides->ctx;
            g->host_valid = true;
            *picked = g.release();
        }
        return VSC_OK;
    }
    if (!guides->ctx) {  // vsc_multi_guides_enumerate's host-only object: the same picks by the host's definition
        std::vector<uint32_t> tg, lens(genome->n_contigs), rk;
        for (uint32_t c = 0; c < genome->n_contigs; ++c) lens[c] = genome->h_contig_end[c] - genome->h_contig_off[c];
        if (regions) {
            tg.resize((size_t)n);
            for (uint64_t i = 0; i < n; ++i) {
                const uint32_t label = vsc_regions_locate(regions, guides->loci[i].contig, guides->loci[i].pos);
                tg[i] = label == VSC_REGION_NONE || !group ? label : group[label];
            }
            target = tg.data();
        }
        if (picked && !rank) {
            rk.resize((size_t)n);
            rank = rk.data();
        }
        pick_host_stats(s, lens.data(), genome->n_contigs, guides->loci.data(), n, target, key, n_targets, picks, counts, rank, stats);
        if (stats) stats->wall_ms = wall_ms_since(t0);
        return picked ? pick_gather_host(guides, rank, picked) : VSC_OK;
    }
    PickInput in;
    in.d_loci = (const char *)guides->storage.p + guides->loci_at;
    in.n = n;
    in.key = key;
    in.target = target;
    in.regions = regions;
    in.group = group;
    in.n_targets = n_targets;
    const uint32_t *d_rank = nullptr;
    const int prc = pick_device(ctx, genome, s, in, picks, counts, rank, rank || picked, &d_rank, stats, who);
    if (prc != VSC_OK) return prc;
    if (picked) {
        const vsc_timing kept = ctx->timing;
        PickGatherArgs ga{};
        ga.in_codes = (const unsigned long long *)guides->storage.p;
        ga.in_loci = (const uint4 *)in.d_loci;
        ga.rank = d_rank;
        ga.n = n;
        const uint64_t tiles = (n + kPickTile - 1) / kPickTile;
        const int erc = run_enumeration(ctx, who, ga, nullptr, (uint32_t)tiles, nullptr, 0, 0, picked,
                                        [&](const void *, unsigned long long, bool write) { return launch_pick_gather(ga, write, ctx->stream); });
        if (erc != VSC_OK) return erc;
        if (stats) {
            stats->stage_ms[3] += ctx->timing.scan_ms;
            stats->kernel_ms += ctx->timing.scan_ms;
        }
        ctx->timing = kept;
    }
    if (stats) stats->wall_ms = wall_ms_since(t0);
    return VSC_OK;
    });
}

// vsc_loci_pick / vsc_loci_pick_regions behind their own checks: host loci, the targets as an array or as regions (+ group)
int pick_loci(vsc_ctx *ctx, const vsc_genome *genome, const vsc_locus *loci, uint64_t n, const uint32_t *target, const vsc_regions *regions,
              const uint32_t *group, const uint64_t *key, uint32_t n_targets, const vsc_pick_params *params, uint32_t *picks, uint32_t *counts,
              uint32_t *rank, vsc_pick_stats *stats, const char *fn, std::chrono::steady_clock::time_point t0)
{
    PickShape s{};
    const int rc = pick_front(ctx, params, s, n, n_targets, key, picks, counts, fn);
    if (rc != VSC_OK) return rc;
    if (n && (!loci || (!regions && !target))) return fail_in(ctx, VSC_ERR_INVALID, fn, "null argument");
    if (regions) {
        const int grc = pick_regions_check(ctx, genome, regions, group, n_targets, fn);
        if (grc != VSC_OK) return grc;
    }
    if (pick_begin(s, n, n_targets, picks, counts, rank, stats)) return VSC_OK;
    PickInput in;
    in.h_loci = loci;
    in.n = n;
    in.key = key;
    in.target = target;
    in.regions = regions;
    in.group = group;
    in.n_targets = n_targets;
    const int prc = pick_device(ctx, genome, s, in, picks, counts, rank, rank != nullptr, nullptr, stats, fn);
    if (prc == VSC_OK && stats) stats->wall_ms = wall_ms_since(t0);
    return prc;
}

}  // namespace

extern "C" {

int vsc_pick_host(const vsc_contig *contigs, uint32_t n_contigs, const vsc_locus *loci, uint64_t n, const uint32_t *target, const uint64_t *key,
                  uint32_t n_targets, const vsc_pick_params *params, uint32_t *picks, uint32_t *counts, uint32_t *rank, vsc_pick_stats *stats)
{
    return guarded(nullptr, [&]() -> int {
    const auto t0 = std::chrono::steady_clock::now();
    PickShape s{};
    if (n_contigs && !contigs) return VSC_ERR_INVALID;
    const int rc = pick_front(nullptr, params, s, n, n_targets, key, picks, counts, "vsc_pick_host");
    if (rc != VSC_OK) return rc;
    if (n && (!loci || !target)) return VSC_ERR_INVALID;
    if (pick_begin(s, n, n_targets, picks, counts, rank, stats)) return VSC_OK;
    std::vector<uint32_t> lens(n_contigs);
    for (uint32_t c = 0; c < n_contigs; ++c) lens[c] = contigs[c].length;
    pick_host_stats(s, lens.data(), n_contigs, loci, n, target, key, n_targets, picks, counts, rank, stats);
    if (stats) stats->wall_ms = wall_ms_since(t0);
    return VSC_OK;
    });
}

int vsc_loci_pick(vsc_ctx *ctx, const vsc_genome *genome, const vsc_locus *loci, uint64_t n, const uint32_t *target, const uint64_t *key,
                  uint32_t n_targets, const vsc_pick_params *params, uint32_t *picks, uint32_t *counts, uint32_t *rank, vsc_pick_stats *stats)
{
    return guarded(ctx, [&]() -> int {
    if (!ctx) return VSC_ERR_INVALID;
    const char *const fn = "vsc_loci_pick";
    const auto t0 = std::chrono::steady_clock::now();
    ctx->err.clear();
    if (!genome) return fail_in(ctx, VSC_ERR_INVALID, fn, "null argument");
    if (genome->ctx != ctx) return fail_in(ctx, VSC_ERR_INVALID, fn, "genome belongs to another context");
    return pick_loci(ctx, genome, loci, n, target, nullptr, nullptr, key, n_targets, params, picks, counts, rank, stats, fn, t0);
    });
}

int vsc_loci_pick_regions(vsc_ctx *ctx, const vsc_genome *genome, const vsc_locus *loci, uint64_t n, const vsc_regions *regions, const uint32_t *group,
                          const uint64_t *key, uint32_t n_targets, const vsc_pick_params *params, uint32_t *picks, uint32_t *counts, uint32_t *rank,
                          vsc_pick_stats *stats)
{
    return guarded(ctx, [&]() -> int {
    if (!ctx) return VSC_ERR_INVALID;
    const char *const fn = "vsc_loci_pick_regions";
    const auto t0 = std::chrono::steady_clock::now();
    ctx->err.clear();
    if (!genome || !regions) return fail_in(ctx, VSC_ERR_INVALID, fn, "null argument");
    if (genome->ctx != ctx) return fail_in(ctx, VSC_ERR_INVALID, fn, "genome belongs to another context");
    return pick_loci(ctx, genome, loci, n, nullptr, regions, group, key, n_targets, params, picks, counts, rank, stats, fn, t0);
    });
}

int vsc_guides_pick(vsc_ctx *ctx, const vsc_genome *genome, vsc_guides *guides, const vsc_regions *regions, const uint32_t *group,
                    const uint32_t *target, uint32_t n_targets, const uint64_t *key, const vsc_pick_params *params, uint32_t *picks,
                    uint32_t *counts, uint32_t *rank, vsc_guides **picked, vsc_pick_stats *stats)
{
    return pick_guides(ctx, genome, guides, regions, group, target, n_targets, key, params, true, picks, counts, rank, picked, stats, "vsc_guides_pick");
}

int vsc_pattern_guides_pick(vsc_ctx *ctx, const vsc_genome *genome, vsc_pattern_guides *guides, const vsc_regions *regions, const uint32_t *group,
                            const uint32_t *target, uint32_t n_targets, const uint64_t *key, const vsc_pick_params *params, uint32_t *picks,
                            uint32_t *counts, uint32_t *rank, vsc_pattern_guides **picked, vsc_pick_stats *stats)
{
    return pick_guides(ctx, genome, guides, regions, group, target, n_targets, key, params, false, picks, counts, rank, picked, stats,
                       "vsc_pattern_guides_pick");
}

}  // extern "C"

// ---- base-editor windows and their join with targets (the definition: vsc_edit.h, the kernels: vsc_edit.hip) ----
namespace {

// The shape, the genome and the targets of an edit call, checked on the host; gpos = the targets' global positions.
int edit_check(vsc_ctx *ctx, const vsc_genome *genome, const vsc_edit_shape *shape, const vsc_edit_target *targets, uint64_t n_t,
               EditShape &s, std::vector<uint32_t> &gpos, const char *who)
{
    ctx->err.clear();
    if (!genome || !shape) return fail_in(ctx, VSC_ERR_INVALID, who, "null argument");
    if (genome->ctx != ctx) return fail_in(ctx, VSC_ERR_INVALID, who, "genome belongs to another context");
    s = EditShape{shape->site_len, shape->win_start, shape->win_len, shape->from};
    if (shape->reserved[0] || shape->reserved[1] || shape->reserved[2] || shape->reserved[3] || !edit_shape_valid(s))
        return fail_in(ctx, VSC_ERR_INVALID, who, "site_len 16 .. 32, 1 <= win_len <= 16, win_start + win_len <= site_len, from 0 .. 3, reserved fields 0");
    if (n_t && !targets) return fail_in(ctx, VSC_ERR_INVALID, who, "targets are null with n_t > 0");
    if (n_t > kEditMaxCount) return fail_in(ctx, VSC_ERR_RANGE, who, "more than 0xFFFFFFFE targets");
    gpos.resize((size_t)n_t);
    for (uint64_t k = 0; k < n_t; ++k) {
        const vsc_edit_target &t = targets[k];
        if (t.contig >= genome->n_contigs || t.contig >= genome->h_contig_off.size())
            return fail_in(ctx, VSC_ERR_INVALID, who, "a target lies on an unknown contig");
        const uint32_t off = genome->h_contig_off[t.contig], len = genome->h_contig_end[t.contig] - off;
        if (t.pos >= len) return fail_in(ctx, VSC_ERR_INVALID, who, "a target lies beyond its contig");
        if (k && !(targets[k - 1].contig < t.contig || (targets[k - 1].contig == t.contig && targets[k - 1].pos < t.pos)))
            return fail_in(ctx, VSC_ERR_INVALID, who, "the targets are not strictly ascending by (contig, pos)");
        gpos[k] = off + t.pos;
    }
    return VSC_OK;
}

// the targets' global positions at the front of edit_tabs; `more` bytes behind them (256-byte aligned) for the caller
int edit_upload_targets(vsc_ctx *ctx, const std::vector<uint32_t> &gpos, size_t more, EditTargets &t, char **behind)
{
    const size_t t_bytes = round256(gpos.size() * sizeof(uint32_t) + 4);
    VSC_HIP(ctx, ctx->edit_tabs.ensure(t_bytes + more));
    if (!gpos.empty())
        VSC_HIP(ctx, hipMemcpyAsync(ctx->edit_tabs.p, gpos.data(), gpos.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    t = EditTargets{(const uint32_t *)ctx->edit_tabs.p, (uint32_t)gpos.size()};
    if (behind) *behind = (char *)ctx->edit_tabs.p + t_bytes;
    return VSC_OK;
}

const CandidateRule kEditRule{"the shape's site_len must be 23", kEditMaxCount, "more than 0xFFFFFFFE candidates"};

// Rows, pairs and coverage of the loci `at`: edit_rows_kernel, then - with targets - the join of the rows with them.
int edit_run(vsc_ctx *ctx, const vsc_genome *genome, const EditShape &shape, const std::vector<uint32_t> &gpos, const CandidateLoci &at,
             uint32_t *rows, vsc_edit_pair *pairs, uint64_t capacity, uint64_t *n_pairs, uint32_t *coverage, vsc_edit_stats *stats, const char *who)
{
    const auto t0 = std::chrono::steady_clock::now();
    const size_t n_t = gpos.size();
    const uint64_t n = at.n;
    if (stats) *stats = vsc_edit_stats{};
    if (n_pairs) *n_pairs = 0;
    PairCoverage cov(n_t, coverage, kEditUndefined);
    if (n == 0) {
        ctx->timing = vsc_timing{};
        if (stats) stats->wall_ms = wall_ms_since(t0);
        return VSC_OK;
    }
    VSC_HIP(ctx, hipSetDevice(ctx->device));
    // edit_tabs: [targets][pairs per target][fewest bystanders per target][pairs per tile][offsets per tile]
    JoinTabs tabs(n, 2 * PairCoverage::bytes(n_t), 0);
    EditArgs a{};
    const int urc = edit_upload_targets(ctx, gpos, tabs.bytes(), a.targets, &tabs.base);
    if (urc != VSC_OK) return urc;
    a.g = eff_planes(genome);
    a.shape = shape;
    a.n = n;
    unsigned long long seen[kEditCounts] = {};
    const int rrc = rows_pass(ctx, at, sizeof(uint2), rows, seen, kEditCounts, [&](unsigned long long *d_stats, void *d_rows, const uint4 *d_loci) {
        a.stats = d_stats;
        a.out = (uint2 *)d_rows;
        a.loci = d_loci;
        return launch_edit_rows(a, ctx->n_cus, ctx->stream);
    });
    if (rrc != VSC_OK) return rrc;
    EditPairArgs p{};
    p.shape = shape;
    p.targets = a.targets;
    p.contig_off = genome->d_contig_off;
    p.loci = a.loci;
    p.rows = a.out;
    p.n = n;
    p.n_work = tabs.tiles;
    p.tile_count = tabs.tile_count();
    p.tile_off = tabs.tile_off();
    Join j{n, sizeof(uint2), n_t != 0, pairs, sizeof(vsc_edit_pair), capacity, n_pairs, kEditMaxCount, "more than 0xFFFFFFFE pairs",
           "more pairs than `capacity` holds; *n_pairs is their number"};
    const int jrc = join_passes(
        ctx, tabs, j,
        [&](uint4 *d_pairs, bool write) {
            p.pairs = d_pairs;
            return launch_edit_pairs(p, write, ctx->stream);
        },
        [&](bool) { return coverage || stats; },
        [&] {
            const int crc = cov.clear(ctx, tabs);
            p.cov_count = cov.count;
            p.cov_min = cov.min;
            return crc;
        },
        [&] { return cov.read(ctx, a.stats + kEditCounts + 1); });
    if (jrc != VSC_OK) return jrc;
    const uint64_t covered = cov.take();
    if (stats) {
        class_counts(stats, seen);
        stats->with_hit = seen[kEffClasses];
        stats->pairs = j.total;
        stats->targets_covered = covered;
        stats->kernel_ms = j.rows_ms;
        stats->wall_ms = wall_ms_since(t0);
    }
    return join_refusal(ctx, j, who);
}

// vsc_guides_edit / vsc_pattern_guides_edit: over the candidates where they lie, a host-only object from the host
template <class Guides>
int edit_guides(vsc_ctx *ctx, const vsc_genome *genome, Guides *guides, const vsc_edit_shape *shape, const vsc_edit_target *targets, uint64_t n_t,
                bool need_23, uint32_t *rows, vsc_edit_pair *pairs, uint64_t capacity, uint64_t *n_pairs, uint32_t *coverage,
                vsc_edit_stats *stats, const char *who)
{
    return guarded(ctx, [&]() -> int {
    EditShape s{};
    std::vector<uint32_t> gpos;
    CandidateLoci at{};
    const int rc = candidate_front(ctx, guides, need_23, kEditRule, who, at, &s.site_len,
                                   [&] { return edit_check(ctx, genome, shape, targets, n_t, s, gpos, who); }, no_refusal);
    if (rc != VSC_OK) return rc;
    return edit_run(ctx, genome, s, gpos, at, rows, pairs, capacity, n_pairs, coverage, stats, who);
    });
}

// vsc_guides_filter_edit / vsc_pattern_guides_filter_edit: the candidates with a hit and an editable count within the bounds
template <class Guides>
int edit_filter(vsc_ctx *ctx, const vsc_genome *genome, Guides *in, const vsc_edit_shape *shape, const vsc_edit_target *targets, uint64_t n_t,
                bool need_23, uint32_t min_editable, uint32_t max_editable, Guides **out, const char *who)
{
    return guarded(ctx, [&]() -> int {
    EditShape s{};
    std::vector<uint32_t> gpos;
    const int rc = filter_front(
        ctx, in, out, need_23, kEditRule, who, &s.site_len,
        [&] { return edit_check(ctx, genome, shape, targets, n_t, s, gpos, who); },
        [&] { return min_editable > max_editable ? fail_in(ctx, VSC_ERR_INVALID, who, "min_editable is more than max_editable") : VSC_OK; });
    if (rc != VSC_OK) return rc;
    EditFilterArgs a{};
    const int urc = edit_upload_targets(ctx, gpos, 0, a.targets, nullptr);
    if (urc != VSC_OK) return urc;
    if (in->n == 0) VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (gpos is this call's vector, and no pass will wait)
    a.g = eff_planes(genome);
    a.shape = s;
    a.min_editable = min_editable;
    a.max_editable = max_editable;
    return filter_candidates(ctx, in, a, kEditTile, out, who, [&](bool write) { return launch_edit_filter(a, write, ctx->stream); });
    });
}

}  // namespace

extern "C" {

int vsc_edit_site_text(const char *site, const vsc_edit_shape *shape, uint32_t *mask)
{
    if (!site || !shape || !mask) return VSC_ERR_INVALID;
    const EditShape s{shape->site_len, shape->win_start, shape->win_len, shape->from};
    if (shape->reserved[0] || shape->reserved[1] || shape->reserved[2] || shape->reserved[3] || !edit_shape_valid(s)) return VSC_ERR_INVALID;
    if (strnlen(site, s.site_len + 1) != s.site_len) return VSC_ERR_INVALID;
    uint64_t ch = 0, cl = 0;
    for (uint32_t j = 0; j < s.site_len; ++j) {
        const int b = base_code(site[j]);
        if (b > 3) return VSC_ERR_INVALID;
        ch |= (uint64_t)(b >> 1) << j;
        cl |= (uint64_t)(b & 1) << j;
    }
    *mask = edit_mask(ch, cl, s);
    return VSC_OK;
}

int vsc_loci_edit(vsc_ctx *ctx, const vsc_genome *genome, const vsc_locus *loci, uint64_t n, const vsc_edit_shape *shape,
                  const vsc_edit_target *targets, uint64_t n_t, uint32_t *rows, vsc_edit_pair *pairs, uint64_t capacity, uint64_t *n_pairs,
                  uint32_t *coverage, vsc_edit_stats *stats)
{
    return guarded(ctx, [&]() -> int {
    if (!ctx) return VSC_ERR_INVALID;
    const char *const fn = "vsc_loci_edit";
    EditShape s{};
    std::vector<uint32_t> gpos;
    const int rc = edit_check(ctx, genome, shape, targets, n_t, s, gpos, fn);
    if (rc != VSC_OK) return rc;
    if (n && !loci) return fail_in(ctx, VSC_ERR_INVALID, fn, "null argument");
    if (n > kEditMaxCount) return fail_in(ctx, VSC_ERR_RANGE, fn, "more than 0xFFFFFFFE candidates");
    return edit_run(ctx, genome, s, gpos, CandidateLoci{nullptr, loci, n}, rows, pairs, capacity, n_pairs, coverage, stats, fn);
    });
}

int vsc_guides_edit(vsc_ctx *ctx, const vsc_genome *genome, vsc_guides *guides, const vsc_edit_shape *shape, const vsc_edit_target *targets,
                    uint64_t n_t, uint32_t *rows, vsc_edit_pair *pairs, uint64_t capacity, uint64_t *n_pairs, uint32_t *coverage,
                    vsc_edit_stats *stats)
{
    return edit_guides(ctx, genome, guides, shape, targets, n_t, true, rows, pairs, capacity, n_pairs, coverage, stats, "vsc_guides_edit");
}

int vsc_pattern_guides_edit(vsc_ctx *ctx, const vsc_genome *genome, vsc_pattern_guides *guides, const vsc_edit_shape *shape,
                            const vsc_edit_target *targets, uint64_t n_t, uint32_t *rows, vsc_edit_pair *pairs, uint64_t capacity,
                            uint64_t *n_pairs, uint32_t *coverage, vsc_edit_stats *stats)
{
    return edit_guides(ctx, genome, guides, shape, targets, n_t, false, rows, pairs, capacity, n_pairs, coverage, stats, "vsc_pattern_guides_edit");
}

int vsc_guides_filter_edit(vsc_ctx *ctx, const vsc_genome *genome, vsc_guides *in, const vsc_edit_shape *shape, const vsc_edit_target *targets,
                           uint64_t n_t, uint32_t min_editable, uint32_t max_editable, vsc_guides **out)
{
    return edit_filter(ctx, genome, in, shape, targets, n_t, true, min_editable, max_editable, out, "vsc_guides_filter_edit");
}

int vsc_pattern_guides_filter_edit(vsc_ctx *ctx, const vsc_genome *genome, vsc_pattern_guides *in, const vsc_edit_shape *shape,
                                   const vsc_edit_target *targets, uint64_t n_t, uint32_t min_editable, uint32_t max_editable,
                                   vsc_pattern_guides **out)
{
    return edit_filter(ctx, genome, in, shape, targets, n_t, false, min_editable, max_editable, out, "vsc_pattern_guides_filter_edit");
}

}  // extern "C"

// ---- known variation under candidate guides (the definition: vsc_variation.h, the kernels: vsc_variation.hip) ----
namespace {

// The shape and the variants of a variation call against contigs [off[c], end[c]) in global positions; null: fine, else the reason.
const char *var_check(const vsc_variation_shape *shape, const vsc_variant *variants, uint64_t n_v, const uint32_t *off, const uint32_t *end,
                      size_t n_contigs, VarShape &s, int *code)
{
    *code = VSC_ERR_INVALID;
    if (!shape) return "null argument";
    s = VarShape{shape->site_len, shape->zones, {shape->accept[0], shape->accept[1]}};
    if (shape->reserved0 || shape->reserved[0] || shape->reserved[1] || shape->reserved[2] || shape->reserved[3] || !var_shape_valid(s))
        return "site_len 16 .. 32, no zone or accept bit at a position from site_len on, reserved fields 0";
    if (n_v && !variants) return "variants are null with n_v > 0";
    if (n_v > kVarMaxCount) {
        *code = VSC_ERR_RANGE;
        return "more than 0xFFFFFFFE variants";
    }
    for (uint64_t k = 0; k < n_v; ++k) {
        const vsc_variant &v = variants[k];
        if (v.contig >= n_contigs) return "a variant lies on an unknown contig";
        const uint32_t len = end[v.contig] - off[v.contig], span = v.span_alt & 0xFFFFu, alt = v.span_alt >> 16;
        if (span == 0) return "a variant's span is 0";
        if (v.pos >= len || span > len - v.pos) return "a variant reaches beyond its contig";
        if (alt > kVarOther) return "a variant's alt is above 4, or span_alt has other bits";
        if (alt < kVarOther && span != 1) return "an SNV (alt 0 .. 3) has a span other than 1";
        if (v.weight > kVarMaxCount) return "a variant's weight is 0xFFFFFFFF";
        if (k && (variants[k - 1].contig > v.contig || (variants[k - 1].contig == v.contig && variants[k - 1].pos > v.pos)))
            return "the variants are not ascending by (contig, pos)";
    }
    *code = VSC_OK;
    return nullptr;
}

// var_check for a device call: the context and the genome first
int var_check_ctx(vsc_ctx *ctx, const vsc_genome *genome, const vsc_variation_shape *shape, const vsc_variant *variants, uint64_t n_v, VarShape &s,
                  const char *who)
{
    ctx->err.clear();
    if (!genome || !shape) return fail_in(ctx, VSC_ERR_INVALID, who, "null argument");
    if (genome->ctx != ctx) return fail_in(ctx, VSC_ERR_INVALID, who, "genome belongs to another context");
    int code = VSC_OK;
    const size_t n_contigs = std::min<size_t>(genome->n_contigs, genome->h_contig_off.size());
    const char *why = var_check(shape, variants, n_v, genome->h_contig_off.data(), genome->h_contig_end.data(), n_contigs, s, &code);
    return why ? fail_in(ctx, code, who, why) : VSC_OK;
}

// The variants at the front of edit_tabs, rewritten there as the walk's records, and the block table behind them; `more` bytes
// behind those (256-byte aligned) for the caller.  The caller's array is read until the stream is synchronised.
int var_upload(vsc_ctx *ctx, const vsc_genome *genome, const vsc_variant *variants, uint64_t n_v, size_t more, VarTable &t, char **behind)
{
    const uint32_t bits = ctx->variation_block_bits ? ctx->variation_block_bits : kVarBlockBits;
    const uint64_t total = genome->h_contig_end.empty() ? 0 : genome->h_contig_end.back();
    VarBuildArgs b{};
    b.n = (uint32_t)n_v;
    b.n_tiles = (uint32_t)((n_v + kEditTile - 1) / kEditTile);
    b.bits = bits;
    b.n_blocks = n_v ? var_block_count(total, bits) : 0u;
    const size_t rec_bytes = round256((size_t)n_v * sizeof(VarRec) + 16), first_bytes = round256(((size_t)b.n_blocks + 1) * sizeof(uint32_t));
    const size_t max_bytes = round256((size_t)b.n_tiles * sizeof(uint32_t) + 4);
    VSC_HIP(ctx, ctx->edit_tabs.ensure(rec_bytes + first_bytes + max_bytes + more));
    char *base = (char *)ctx->edit_tabs.p;
    b.rec = (VarRec *)base;
    b.first = (uint32_t *)(base + rec_bytes);
    b.tile_max = (uint32_t *)(base + rec_bytes + first_bytes);
    b.contig_off = genome->d_contig_off;
    if (n_v) {
        VSC_HIP(ctx, hipMemcpyAsync(b.rec, variants, (size_t)n_v * sizeof(vsc_variant), hipMemcpyHostToDevice, ctx->stream));
        VSC_HIP(ctx, launch_var_build(b, ctx->n_cus, ctx->stream));
    }
    t = VarTable{b.rec, b.first, b.n, bits, b.n_blocks};
    if (behind) *behind = base + rec_bytes + first_bytes + max_bytes;
    return VSC_OK;
}

const CandidateRule kVarRule{"the shape's site_len must be 23", kVarMaxCount, "more than 0xFFFFFFFE candidates"};

// Rows, pairs and coverage of the loci `at`: the variants' build, var_rows_kernel, then - with variants - the join of the rows
// with them.  The coverage is one array of two words per variant, zeros without a pair, and comes back as it lies.
int var_run(vsc_ctx *ctx, const vsc_genome *genome, const VarShape &shape, const vsc_variant *variants, uint64_t n_v, const CandidateLoci &at,
            uint32_t *rows, vsc_variation_pair *pairs, uint64_t capacity, uint64_t *n_pairs, uint32_t *coverage, vsc_variation_stats *stats,
            const char *who)
{
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t n = at.n;
    if (stats) *stats = vsc_variation_stats{};
    if (n_pairs) *n_pairs = 0;
    if (coverage) std::fill(coverage, coverage + 2 * n_v, 0u);
    if (n == 0) {
        ctx->timing = vsc_timing{};
        if (stats) stats->wall_ms = wall_ms_since(t0);
        return VSC_OK;
    }
    VSC_HIP(ctx, hipSetDevice(ctx->device));
    // edit_tabs behind the variants and their table: [pairs per variant, two kinds][pairs per tile][offsets per tile]
    JoinTabs tabs(n, round256(2 * (size_t)n_v * sizeof(uint32_t) + 4), 0);
    VarArgs a{};
    const int urc = var_upload(ctx, genome, variants, n_v, tabs.bytes(), a.table, &tabs.base);
    if (urc != VSC_OK) return urc;
    a.g = eff_planes(genome);
    a.shape = shape;
    a.n = n;
    unsigned long long seen[kVarCounts] = {};
    const int rrc = rows_pass(ctx, at, sizeof(uint4), rows, seen, kVarCounts, [&](unsigned long long *d_stats, void *d_rows, const uint4 *d_loci) {
        a.stats = d_stats;
        a.out = (uint4 *)d_rows;
        a.loci = d_loci;
        return launch_var_rows(a, ctx->n_cus, ctx->stream);
    });
    if (rrc != VSC_OK) return rrc;
    VarPairArgs p{};
    p.shape = shape;
    p.table = a.table;
    p.contig_off = genome->d_contig_off;
    p.loci = a.loci;
    p.rows = a.out;
    p.n = n;
    p.n_work = tabs.tiles;
    p.tile_count = tabs.tile_count();
    p.tile_off = tabs.tile_off();
    Join j{n, sizeof(uint4), n_v != 0, pairs, sizeof(vsc_variation_pair), capacity, n_pairs, kVarMaxCount, "more than 0xFFFFFFFE pairs",
           "more pairs than `capacity` holds; *n_pairs is their number"};
    unsigned long long d_covered = 0;
    const int jrc = join_passes(
        ctx, tabs, j,
        [&](uint4 *d_pairs, bool write) {
            p.pairs = d_pairs;
            return launch_var_pairs(p, write, ctx->stream);
        },
        // (a tile's count saturates at 0xFFFFFFFF, so a total within the bound is the exact one - and only such a one is covered)
        [&](bool too_many) { return !too_many && (coverage || stats); },
        [&] {
            p.coverage = (uint32_t *)tabs.base;
            VSC_HIP(ctx, hipMemsetAsync(p.coverage, 0, 2 * (size_t)n_v * sizeof(uint32_t), ctx->stream));
            return VSC_OK;
        },
        [&] {
            if (!coverage) {  // the stats alone: the covered variants are counted where they lie, 8 bytes come back
                unsigned long long *slot = a.stats + kVarCounts + 1;  // (inside the zeroed head, behind the rows kernel's counters)
                VSC_HIP(ctx, launch_var_covered(p.coverage, (uint32_t)n_v, slot, ctx->n_cus, ctx->stream));
                VSC_HIP(ctx, hipMemcpyAsync(&d_covered, slot, sizeof d_covered, hipMemcpyDeviceToHost, ctx->stream));
            } else {
                VSC_HIP(ctx, hipMemcpyAsync(coverage, p.coverage, 2 * (size_t)n_v * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
            }
            return VSC_OK;
        });
    if (jrc != VSC_OK) return jrc;
    uint64_t covered = d_covered;
    for (uint64_t k = 0; coverage && p.coverage && k < n_v; ++k) covered += (coverage[2 * k] | coverage[2 * k + 1]) != 0;
    if (stats) {
        class_counts(stats, seen);
        stats->with_disrupting = seen[kEffClasses];
        stats->pairs = j.total;
        stats->variants_covered = covered;
        stats->kernel_ms = j.rows_ms;
        stats->wall_ms = wall_ms_since(t0);
    }
    return join_refusal(ctx, j, who);
}

// vsc_guides_variation / vsc_pattern_guides_variation: over the candidates where they lie, a host-only object from the host
template <class Guides>
int var_guides(vsc_ctx *ctx, const vsc_genome *genome, Guides *guides, const vsc_variation_shape *shape, const vsc_variant *variants, uint64_t n_v,
               bool need_23, uint32_t *rows, vsc_variation_pair *pairs, uint64_t capacity, uint64_t *n_pairs, uint32_t *coverage,
               vsc_variation_stats *stats, const char *who)
{
    return guarded(ctx, [&]() -> int {
    VarShape s{};
    CandidateLoci at{};
    const int rc = candidate_front(ctx, guides, need_23, kVarRule, who, at, &s.site_len,
                                   [&] { return var_check_ctx(ctx, genome, shape, variants, n_v, s, who); }, no_refusal);
    if (rc != VSC_OK) return rc;
    return var_run(ctx, genome, s, variants, n_v, at, rows, pairs, capacity, n_pairs, coverage, stats, who);
    });
}

// vsc_guides_filter_variation / vsc_pattern_guides_filter_variation: the candidates within the bounds of `filter`
template <class Guides>
int var_filter(vsc_ctx *ctx, const vsc_genome *genome, Guides *in, const vsc_variation_shape *shape, const vsc_variant *variants, uint64_t n_v,
               bool need_23, const vsc_variation_filter *filter, Guides **out, const char *who)
{
    return guarded(ctx, [&]() -> int {
    VarShape s{};
    const int rc = filter_front(
        ctx, in, out, need_23, kVarRule, who, &s.site_len,
        [&] {
            const int crc = var_check_ctx(ctx, genome, shape, variants, n_v, s, who);
            return crc == VSC_OK && !filter ? fail_in(ctx, VSC_ERR_INVALID, who, "null argument") : crc;
        },
        [&] {
            if (filter->require_zones > 15u || filter->reserved)
                return fail_in(ctx, VSC_ERR_INVALID, who, "require_zones is a mask of four bits, the reserved field 0");
            return VSC_OK;
        });
    if (rc != VSC_OK) return rc;
    VarFilterArgs a{};
    if (in->n) {  // (no candidate: no pass reads the variants)
        const int urc = var_upload(ctx, genome, variants, n_v, 0, a.table, nullptr);
        if (urc != VSC_OK) return urc;
    }
    a.g = eff_planes(genome);
    a.shape = s;
    a.filter = VarFilter{filter->max_cost, filter->max_by_zone, filter->require_zones};
    return filter_candidates(ctx, in, a, kEditTile, out, who, [&](bool write) { return launch_var_filter(a, write, ctx->stream); });
    });
}

}  // namespace

extern "C" {

int vsc_debug_variation_block_bits(vsc_ctx *ctx, uint32_t bits)
{
    if (!ctx || (bits && (bits < kVarMinBlockBits || bits > kVarMaxBlockBits))) return VSC_ERR_INVALID;
    ctx->variation_block_bits = bits;
    return VSC_OK;
}

int vsc_variation_host(const vsc_contig *contigs, uint32_t n_contigs, const vsc_locus *loci, uint64_t n, const vsc_variation_shape *shape,
                       const vsc_variant *variants, uint64_t n_v, uint32_t *rows, vsc_variation_pair *pairs, uint64_t capacity, uint64_t *n_pairs,
                       uint32_t *coverage)
{
    return guarded(nullptr, [&]() -> int {
    if ((n_contigs && !contigs) || (n && !loci)) return VSC_ERR_INVALID;
    if (n > kVarMaxCount) return VSC_ERR_RANGE;
    // the contigs one base apart, as the packed genome lays them
    std::vector<uint32_t> off(n_contigs), end(n_contigs);
    uint64_t at = 0;
    for (uint32_t c = 0; c < n_contigs; ++c) {
        if (at + contigs[c].length > 0xFFFFFFFFull) return VSC_ERR_RANGE;
        off[c] = (uint32_t)at;
        end[c] = (uint32_t)(at + contigs[c].length);
        at += (uint64_t)contigs[c].length + 1;
    }
    VarShape s{};
    int code = VSC_OK;
    if (var_check(shape, variants, n_v, off.data(), end.data(), n_contigs, s, &code)) return code;
    if (n_pairs) *n_pairs = 0;
    if (coverage) std::fill(coverage, coverage + 2 * n_v, 0u);
    // the records and the block table, as the device builds them
    std::vector<VarRec> rec((size_t)n_v);
    uint32_t reach = 0;
    for (uint64_t k = 0; k < n_v; ++k) {
        const uint32_t gpos = off[variants[k].contig] + variants[k].pos;
        reach = std::max(reach, gpos + (variants[k].span_alt & 0xFFFFu));
        rec[k] = VarRec{gpos, variants[k].span_alt, variants[k].weight, reach};
    }
    const uint64_t total = n_contigs ? end[n_contigs - 1] : 0;
    const uint32_t n_blocks = n_v ? var_block_count(total, kVarBlockBits) : 0u;
    std::vector<uint32_t> first((size_t)n_blocks + 1);
    for (uint64_t b = 0; b <= n_blocks; ++b) first[b] = var_first_reach(rec.data(), 0u, (uint32_t)n_v, b << kVarBlockBits);
    const VarTable t{rec.data(), first.data(), (uint32_t)n_v, kVarBlockBits, n_blocks};
    // no planes: every word of a site is "held" and none is read, so that the classes are invalid and defined only
    const EffPlanes g{nullptr, nullptr, nullptr, 0, (total + 31) / 32 + 1, 0, off.data(), end.data(), n_contigs};
    // the count first: a refusal for capacity writes no pair
    uint64_t count = 0;
    bool refused = false;
    for (int pass = 0; pass < 2; ++pass) {
        uint64_t o = 0;
        for (uint64_t i = 0; i < n; ++i) {
            const vsc_locus &l = loci[i];
            const uint32_t cls = var_site(g, s, l.contig, l.pos, l.strand);
            if (cls != kEffDefined) {
                if (pass == 0 && rows) std::fill(rows + 4 * i, rows + 4 * i + 4, kVarUndefined);
                continue;
            }
            const uint32_t g0 = off[l.contig] + l.pos;
            if (pass == 0) {
                uint64_t mine = 0;
                const VarRow row = var_row(t, g0, l.strand, s, &mine);
                count += mine;
                if (rows) {
                    rows[4 * i] = row.by_zone;
                    rows[4 * i + 1] = row.silent;
                    rows[4 * i + 2] = var_cost(row);
                    rows[4 * i + 3] = row.max_weight;
                }
                continue;
            }
            for (uint32_t k = var_first(t, g0); k < t.n; ++k) {
                if (rec[k].gpos >= g0 + s.site_len) break;
                uint32_t info;
                if (!var_touch(rec[k], g0, l.strand, s, &info)) continue;
                if (pairs) pairs[o] = vsc_variation_pair{(uint32_t)i, k, info, rec[k].weight};
                ++o;
                if (coverage) ++coverage[2 * (uint64_t)k + (info >> 18 & 1u)];
            }
        }
        if (pass == 0) {
            if (n_pairs) *n_pairs = count;
            if (count > kVarMaxCount) return VSC_ERR_RANGE;
            refused = pairs && count > capacity;
            if (refused) pairs = nullptr;  // (the coverage stays valid: counted without the pairs)
            if (!pairs && !coverage) break;
        }
    }
    return refused ? VSC_ERR_RANGE : VSC_OK;
    });
}

int vsc_loci_variation(vsc_ctx *ctx, const vsc_genome *genome, const vsc_locus *loci, uint64_t n, const vsc_variation_shape *shape,
                       const vsc_variant *variants, uint64_t n_v, uint32_t *rows, vsc_variation_pair *pairs, uint64_t capacity, uint64_t *n_pairs,
                       uint32_t *coverage, vsc_variation_stats *stats)
{
    return guarded(ctx, [&]() -> int {
    if (!ctx) return VSC_ERR_INVALID;
    const char *const fn = "vsc_loci_variation";
    VarShape s{};
    const int rc = var_check_ctx(ctx, genome, shape, variants, n_v, s, fn);
    if (rc != VSC_OK) return rc;
    if (n && !loci) return fail_in(ctx, VSC_ERR_INVALID, fn, "null argument");
    if (n > kVarMaxCount) return fail_in(ctx, VSC_ERR_RANGE, fn, "more than 0xFFFFFFFE candidates");
    return var_run(ctx, genome, s, variants, n_v, CandidateLoci{nullptr, loci, n}, rows, pairs, capacity, n_pairs, coverage, stats, fn);
    });
}

int vsc_guides_variation(vsc_ctx *ctx, const vsc_genome *genome, vsc_guides *guides, const vsc_variation_shape *shape, const vsc_variant *variants,
                         uint64_t n_v, uint32_t *rows, vsc_variation_pair *pairs, uint64_t capacity, uint64_t *n_pairs, uint32_t *coverage,
                         vsc_variation_stats *stats)
{
    return var_guides(ctx, genome, guides, shape, variants, n_v, true, rows, pairs, capacity, n_pairs, coverage, stats, "vsc_guides_variation");
}

int vsc_pattern_guides_variation(vsc_ctx *ctx, const vsc_genome *genome, vsc_pattern_guides *guides, const vsc_variation_shape *shape,
                                 const vsc_variant *variants, uint64_t n_v, uint32_t *rows, vsc_variation_pair *pairs, uint64_t capacity,
                                 uint64_t *n_pairs, uint32_t *coverage, vsc_variation_stats *stats)
{
    return var_guides(ctx, genome, guides, shape, variants, n_v, false, rows, pairs, capacity, n_pairs, coverage, stats,
                      "vsc_pattern_guides_variation");
}

int vsc_guides_filter_variation(vsc_ctx *ctx, const vsc_genome *genome, vsc_guides *in, const vsc_variation_shape *shape, const vsc_variant *variants,
                                uint64_t n_v, const vsc_variation_filter *filter, vsc_guides **out)
{
    return var_filter(ctx, genome, in, shape, variants, n_v, true, filter, out, "vsc_guides_filter_variation");
}

int vsc_pattern_guides_filter_variation(vsc_ctx *ctx, const vsc_genome *genome, vsc_pattern_guides *in, const vsc_variation_shape *shape,
                                        const vsc_variant *variants, uint64_t n_v, const vsc_variation_filter *filter, vsc_pattern_guides **out)
{
    return var_filter(ctx, genome, in, shape, variants, n_v, false, filter, out, "vsc_pattern_guides_filter_variation");
}

}  // extern "C"

// ---- prime-editing guide design (the definition: vsc_prime.h, the kernels: vsc_prime.hip) ---------------------
namespace {

const char *const kPrimeShapeRule =
    "site_len 16 .. 32, down <= 64 - site_len, 1 <= nick <= site_len, 1 <= pbs_min <= pbs_max <= nick, 1 <= rtt_min <= rtt_max <= C - nick, "
    "pbs_max + rtt_max <= 64, min_homology <= rtt_max, pam and seed ranges inside the site with len <= 8, flags <= 1, |weights| <= 2^20, reserved fields 0";

bool prime_shape_in(const vsc_prime_shape *shape, PrimeShape &s)
{
    s = PrimeShape{};
    s.site_len = shape->site_len;
    s.down = shape->down;
    s.nick = shape->nick;
    s.pbs_min = shape->pbs_min;
    s.pbs_max = shape->pbs_max;
    s.rtt_min = shape->rtt_min;
    s.rtt_max = shape->rtt_max;
    s.min_homology = shape->min_homology;
    s.pam_start = shape->pam_start;
    s.pam_len = shape->pam_len;
    s.seed_start = shape->seed_start;
    s.seed_len = shape->seed_len;
    s.flags = shape->flags;
    s.init = shape->init;
    for (int k = 0; k < 4; ++k) s.mono[k] = shape->mono[k];
    for (int k = 0; k < 16; ++k) s.di[k] = shape->di[k];
    s.target = shape->target;
    for (uint32_t r : shape->reserved)
        if (r) return false;
    return prime_shape_valid(s);
}

// the edits of a call as the kernels hold them, on the host
struct PrimeHostEdits {
    std::vector<uint32_t> gpos;
    std::vector<PrimeEdit> rec;
    std::vector<uint32_t> bitmap;  // one bit per cell of 2^kPrimeCellShift global positions, over the whole genome
};

// EDITS of a call (the prime and the HDR family share the entry and its rules), checked on the host and laid out as the kernels
// hold them
int prime_edits_check(vsc_ctx *ctx, const vsc_genome *genome, const vsc_prime_edit *edits, uint64_t n_e, PrimeHostEdits &h, const char *who)
{
    if (n_e && !edits) return fail_in(ctx, VSC_ERR_INVALID, who, "edits are null with n_e > 0");
    if (n_e > kPrimeMaxCount) return fail_in(ctx, VSC_ERR_RANGE, who, "more than 0xFFFFFFFE edits");
    h.gpos.resize((size_t)n_e);
    h.rec.resize((size_t)n_e);
    uint32_t genome_end = 0;
    for (uint32_t end : genome->h_contig_end) genome_end = end > genome_end ? end : genome_end;
    if (n_e) h.bitmap.assign(((size_t)(genome_end >> kPrimeCellShift) + 32) / 32, 0u);
    for (uint64_t k = 0; k < n_e; ++k) {
        const vsc_prime_edit &e = edits[k];
        if (e.contig >= genome->n_contigs || e.contig >= genome->h_contig_off.size())
            return fail_in(ctx, VSC_ERR_INVALID, who, "an edit lies on an unknown contig");
        const uint32_t off = genome->h_contig_off[e.contig], len = genome->h_contig_end[e.contig] - off;
        if (e.del_len > kPrimeMaxIndel || e.ins_len > kPrimeMaxIndel) return fail_in(ctx, VSC_ERR_INVALID, who, "an edit's del_len or ins_len is above 16");
        if (e.del_len + e.ins_len < 1) return fail_in(ctx, VSC_ERR_INVALID, who, "an edit's del_len and ins_len are both 0");
        const PrimeEdit rec{e.contig, e.pos, (uint32_t)e.del_len | (uint32_t)e.ins_len << 16, e.ins};
        if (e.pos > len || e.del_len > len - e.pos) return fail_in(ctx, VSC_ERR_INVALID, who, "an edit reaches beyond its contig");
        if (!prime_edit_valid(rec, len)) return fail_in(ctx, VSC_ERR_INVALID, who, "an edit's ins has bits above its ins_len letters");
        if (k && !(edits[k - 1].contig < e.contig || (edits[k - 1].contig == e.contig && edits[k - 1].pos < e.pos)))
            return fail_in(ctx, VSC_ERR_INVALID, who, "the edits are not strictly ascending by (contig, pos)");
        const uint32_t gp = off + e.pos, cell = gp >> kPrimeCellShift;
        h.gpos[k] = gp;
        h.rec[k] = rec;
        h.bitmap[cell >> 5] |= 1u << (cell & 31u);
    }
    return VSC_OK;
}

// The shape, the genome and the edits of a prime call, checked on the host.
int prime_check(vsc_ctx *ctx, const vsc_genome *genome, const vsc_prime_shape *shape, const vsc_prime_edit *edits, uint64_t n_e, PrimeShape &s,
                PrimeHostEdits &h, const char *who)
{
    ctx->err.clear();
    if (!genome || !shape) return fail_in(ctx, VSC_ERR_INVALID, who, "null argument");
    if (genome->ctx != ctx) return fail_in(ctx, VSC_ERR_INVALID, who, "genome belongs to another context");
    if (!prime_shape_in(shape, s)) return fail_in(ctx, VSC_ERR_INVALID, who, kPrimeShapeRule);
    return prime_edits_check(ctx, genome, edits, n_e, h, who);
}

// the edits at the front of edit_tabs: [global positions][entries][bitmap]; `more` bytes behind them (256-byte aligned) for the
// caller; bitmap: the kernels ask it (the family's debug switch)
int prime_upload_edits(vsc_ctx *ctx, const PrimeHostEdits &h, size_t more, PrimeEdits &e, char **behind, bool bitmap)
{
    const size_t n = h.gpos.size();
    const size_t g_bytes = round256(n * sizeof(uint32_t) + 4), r_bytes = round256(n * sizeof(PrimeEdit) + 4);
    const size_t b_bytes = round256(h.bitmap.size() * sizeof(uint32_t) + 4);
    VSC_HIP(ctx, ctx->edit_tabs.ensure(g_bytes + r_bytes + b_bytes + more));
    char *base = (char *)ctx->edit_tabs.p;
    if (n) {
        VSC_HIP(ctx, hipMemcpyAsync(base, h.gpos.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        VSC_HIP(ctx, hipMemcpyAsync(base + g_bytes, h.rec.data(), n * sizeof(PrimeEdit), hipMemcpyHostToDevice, ctx->stream));
        VSC_HIP(ctx, hipMemcpyAsync(base + g_bytes + r_bytes, h.bitmap.data(), h.bitmap.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    }
    e = PrimeEdits{(const uint32_t *)base, (const PrimeEdit *)(base + g_bytes),
                   n && bitmap ? (const uint32_t *)(base + g_bytes + r_bytes) : nullptr, (uint32_t)n};
    if (behind) *behind = base + g_bytes + r_bytes + b_bytes;
    return VSC_OK;
}

const CandidateRule kPrimeRule{"the shape's site_len must be 23", kPrimeMaxCount, "more than 0xFFFFFFFE candidates"};

// Rows, pairs and coverage of the loci `at`: prime_rows_kernel, then - with edits - the join of the rows with them, whose write
// pass also counts the pairs by flag.
int prime_run(vsc_ctx *ctx, const vsc_genome *genome, const PrimeShape &shape, const PrimeHostEdits &h, const CandidateLoci &at, uint32_t *rows,
              vsc_prime_pair *pairs, uint64_t capacity, uint64_t *n_pairs, uint32_t *coverage, vsc_prime_stats *stats, const char *who)
{
    const auto t0 = std::chrono::steady_clock::now();
    const size_t n_e = h.gpos.size();
    const uint64_t n = at.n;
    if (stats) *stats = vsc_prime_stats{};
    if (n_pairs) *n_pairs = 0;
    PairCoverage cov(n_e, coverage, kPrimeUndefined);
    if (n == 0) {
        ctx->timing = vsc_timing{};
        if (stats) stats->wall_ms = wall_ms_since(t0);
        return VSC_OK;
    }
    VSC_HIP(ctx, hipSetDevice(ctx->device));
    // edit_tabs behind the edits: [pairs per edit][smallest t per edit][pairs per tile][offsets per tile][pairs by flag]
    const size_t flag_bytes = 256;
    JoinTabs tabs(n, 2 * PairCoverage::bytes(n_e), flag_bytes);
    PrimeArgs a{};
    const int urc = prime_upload_edits(ctx, h, tabs.bytes(), a.edits, &tabs.base, ctx->prime_bitmap);
    if (urc != VSC_OK) return urc;
    a.g = eff_planes(genome);
    a.shape = shape;
    a.n = n;
    unsigned long long seen[kPrimeCounts] = {};
    const int rrc = rows_pass(ctx, at, sizeof(uint2), rows, seen, kPrimeCounts, [&](unsigned long long *d_stats, void *d_rows, const uint4 *d_loci) {
        a.stats = d_stats;
        a.out = (uint2 *)d_rows;
        a.loci = d_loci;
        return launch_prime_rows(a, ctx->n_cus, ctx->prime_groups_per_cu, ctx->stream);
    });
    if (rrc != VSC_OK) return rrc;
    PrimePairArgs p{};
    p.g = a.g;
    p.shape = shape;
    p.edits = a.edits;
    p.loci = a.loci;
    p.rows = a.out;
    p.n = n;
    p.n_work = tabs.tiles;
    p.tile_count = tabs.tile_count();
    p.tile_off = tabs.tile_off();
    Join j{n, sizeof(uint2), n_e != 0, pairs, sizeof(vsc_prime_pair), capacity, n_pairs, kPrimeMaxCount, "more than 0xFFFFFFFE pairs",
           "more pairs than `capacity` holds; *n_pairs is their number"};
    unsigned long long by_flag[kPrimeFlags] = {};
    const int jrc = join_passes(
        ctx, tabs, j,
        [&](uint4 *d_pairs, bool write) {
            p.pairs = d_pairs;
            return launch_prime_pairs(p, write, ctx->stream);
        },
        [&](bool) { return coverage || stats; },
        [&] {
            const int crc = cov.clear(ctx, tabs);
            if (crc != VSC_OK) return crc;
            p.cov_count = cov.count;
            p.cov_min = cov.min;
            p.flag_count = (unsigned long long *)tabs.extra();
            VSC_HIP(ctx, hipMemsetAsync(p.flag_count, 0, flag_bytes, ctx->stream));
            return VSC_OK;
        },
        [&] {
            VSC_HIP(ctx, hipMemcpyAsync(by_flag, p.flag_count, sizeof by_flag, hipMemcpyDeviceToHost, ctx->stream));
            return cov.read(ctx, a.stats + kPrimeCounts + 1);
        });
    if (jrc != VSC_OK) return jrc;
    const uint64_t covered = cov.take();
    if (stats) {
        class_counts(stats, seen);
        stats->with_pair = seen[kEffClasses];
        stats->weak = seen[kEffClasses + 1];
        stats->pairs = j.total;
        for (uint32_t b = 0; b < kPrimeFlags; ++b) stats->pairs_by_flag[b] = by_flag[b];
        stats->edits_covered = covered;
        stats->score_ms = j.rows_ms;
        stats->wall_ms = wall_ms_since(t0);
    }
    return join_refusal(ctx, j, who);
}

// vsc_guides_prime / vsc_pattern_guides_prime: over the candidates where they lie, a host-only object from the host
template <class Guides>
int prime_guides(vsc_ctx *ctx, const vsc_genome *genome, Guides *guides, const vsc_prime_shape *shape, const vsc_prime_edit *edits, uint64_t n_e,
                 bool need_23, uint32_t *rows, vsc_prime_pair *pairs, uint64_t capacity, uint64_t *n_pairs, uint32_t *coverage,
                 vsc_prime_stats *stats, const char *who)
{
    return guarded(ctx, [&]() -> int {
    PrimeShape s{};
    PrimeHostEdits h;
    CandidateLoci at{};
    const int rc = candidate_front(ctx, guides, need_23, kPrimeRule, who, at, &s.site_len,
                                   [&] { return prime_check(ctx, genome, shape, edits, n_e, s, h, who); }, no_refusal);
    if (rc != VSC_OK) return rc;
    return prime_run(ctx, genome, s, h, at, rows, pairs, capacity, n_pairs, coverage, stats, who);
    });
}

// vsc_guides_filter_prime / vsc_pattern_guides_filter_prime: the candidates with a pair, weak ones only where allowed
template <class Guides>
int prime_filter(vsc_ctx *ctx, const vsc_genome *genome, Guides *in, const vsc_prime_shape *shape, const vsc_prime_edit *edits, uint64_t n_e,
                 bool need_23, uint32_t allow_weak, Guides **out, const char *who)
{
    return guarded(ctx, [&]() -> int {
    PrimeShape s{};
    PrimeHostEdits h;
    const int rc = filter_front(ctx, in, out, need_23, kPrimeRule, who, &s.site_len,
                                [&] { return prime_check(ctx, genome, shape, edits, n_e, s, h, who); }, no_refusal);
    if (rc != VSC_OK) return rc;
    PrimeFilterArgs a{};
    const int urc = prime_upload_edits(ctx, h, 0, a.edits, nullptr, ctx->prime_bitmap);
    if (urc != VSC_OK) return urc;
    if (in->n == 0) VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (the edits are this call's vectors, and no pass will wait)
    a.g = eff_planes(genome);
    a.shape = s;
    a.allow_weak = allow_weak ? 1u : 0u;
    return filter_candidates(ctx, in, a, kEditTile, out, who, [&](bool write) { return launch_prime_filter(a, write, ctx->stream); });
    });
}

}  // namespace

extern "C" {

int vsc_debug_prime_bitmap(vsc_ctx *ctx, int on)
{
    if (!ctx) return VSC_ERR_INVALID;
    ctx->prime_bitmap = on != 0;
    return VSC_OK;
}

int vsc_debug_prime_groups_per_cu(vsc_ctx *ctx, uint32_t groups)
{
    if (!ctx || groups > kPrimeMaxGroupsPerCu) return VSC_ERR_INVALID;
    ctx->prime_groups_per_cu = groups;
    return VSC_OK;
}

int vsc_prime_site_text(const char *context, const vsc_prime_shape *shape, uint32_t e0, uint32_t del_len, const char *ins, uint32_t *row,
                        uint32_t *pair, char *extension)
{
    if (!context || !shape || !row) return VSC_ERR_INVALID;
    PrimeShape s{};
    if (!prime_shape_in(shape, s)) return VSC_ERR_INVALID;
    const uint32_t C = prime_context_len(s);
    if (strnlen(context, C + 1) != C) return VSC_ERR_INVALID;
    uint64_t ch = 0, cl = 0;
    for (uint32_t j = 0; j < C; ++j) {
        const int b = base_code(context[j]);
        if (b > 3) return VSC_ERR_INVALID;
        ch |= (uint64_t)(b >> 1) << j;
        cl |= (uint64_t)(b & 1) << j;
    }
    PrimeEdit e{0u, 0u, 0u, 0u};
    if (ins) {
        const size_t ins_len = strnlen(ins, kPrimeMaxIndel + 1);
        if (ins_len > kPrimeMaxIndel || del_len > kPrimeMaxIndel || del_len + ins_len < 1 || e0 > C || del_len > C - e0) return VSC_ERR_INVALID;
        for (size_t k = 0; k < ins_len; ++k) {
            const int b = base_code(ins[k]);
            if (b > 3) return VSC_ERR_INVALID;
            e.ins |= (uint32_t)b << (2 * k);
        }
        e.lens = del_len | (uint32_t)ins_len << 16;
    }
    row[0] = prime_pbs(ch, cl, s, s.mono, s.di);
    row[1] = 0;
    if (pair) pair[0] = pair[1] = 0;
    if (extension) extension[0] = 0;
    uint32_t info = 0, ext = 0;
    uint64_t eh = 0, el = 0;
    if (!ins || !prime_pair(s, ch, cl, 0u, row[0], e0, e, &info, &ext, &eh, &el)) return VSC_OK;
    row[1] = 1;
    if (pair) {
        pair[0] = info;
        pair[1] = ext;
    }
    if (extension) {
        const uint32_t lo = s.nick - (ext >> 16 & 0xFFu), hi = s.nick + (info & 0xFFu);
        uint32_t o = 0;
        for (uint32_t q = hi; q-- > lo;) extension[o++] = "TGCA"[(eh >> q & 1u) << 1 | (el >> q & 1u)];
        extension[o] = 0;
    }
    return VSC_OK;
}

int vsc_loci_prime(vsc_ctx *ctx, const vsc_genome *genome, const vsc_locus *loci, uint64_t n, const vsc_prime_shape *shape,
                   const vsc_prime_edit *edits, uint64_t n_e, uint32_t *rows, vsc_prime_pair *pairs, uint64_t capacity, uint64_t *n_pairs,
                   uint32_t *coverage, vsc_prime_stats *stats)
{
    return guarded(ctx, [&]() -> int {
    if (!ctx) return VSC_ERR_INVALID;
    const char *const fn = "vsc_loci_prime";
    PrimeShape s{};
    PrimeHostEdits h;
    const int rc = prime_check(ctx, genome, shape, edits, n_e, s, h, fn);
    if (rc != VSC_OK) return rc;
    if (n && !loci) return fail_in(ctx, VSC_ERR_INVALID, fn, "null argument");
    if (n > kPrimeMaxCount) return fail_in(ctx, VSC_ERR_RANGE, fn, "more than 0xFFFFFFFE candidates");
    return prime_run(ctx, genome, s, h, CandidateLoci{nullptr, loci, n}, rows, pairs, capacity, n_pairs, coverage, stats, fn);
    });
}

int vsc_guides_prime(vsc_ctx *ctx, const vsc_genome *genome, vsc_guides *guides, const vsc_prime_shape *shape, const vsc_prime_edit *edits,
                     uint64_t n_e, uint32_t *rows, vsc_prime_pair *pairs, uint64_t capacity, uint64_t *n_pairs, uint32_t *coverage,
                     vsc_prime_stats *stats)
{
    return prime_guides(ctx, genome, guides, shape, edits, n_e, true, rows, pairs, capacity, n_pairs, coverage, stats, "vsc_guides_prime");
}

int vsc_pattern_guides_prime(vsc_ctx *ctx, const vsc_genome *genome, vsc_pattern_guides *guides, const vsc_prime_shape *shape,
                             const vsc_prime_edit *edits, uint64_t n_e, uint32_t *rows, vsc_prime_pair *pairs, uint64_t capacity,
                             uint64_t *n_pairs, uint32_t *coverage, vsc_prime_stats *stats)
{
    return prime_guides(ctx, genome, guides, shape, edits, n_e, false, rows, pairs, capacity, n_pairs, coverage, stats, "vsc_pattern_guides_prime");
}

int vsc_guides_filter_prime(vsc_ctx *ctx, const vsc_genome *genome, vsc_guides *in, const vsc_prime_shape *shape, const vsc_prime_edit *edits,
                            uint64_t n_e, uint32_t allow_weak, vsc_guides **out)
{
    return prime_filter(ctx, genome, in, shape, edits, n_e, true, allow_weak, out, "vsc_guides_filter_prime");
}

int vsc_pattern_guides_filter_prime(vsc_ctx *ctx, const vsc_genome *genome, vsc_pattern_guides *in, const vsc_prime_shape *shape,
                                    const vsc_prime_edit *edits, uint64_t n_e, uint32_t allow_weak, vsc_pattern_guides **out)
{
    return prime_filter(ctx, genome, in, shape, edits, n_e, false, allow_weak, out, "vsc_pattern_guides_filter_prime");
}

}  // extern "C"

// ---- coding consequences of base edits (the definition: vsc_effects.h, the kernels: vsc_effects.hip) ----------
namespace {

std::atomic<uint64_t> g_cds_serial{0};
thread_local std::string t_cds_error;

int cds_refuse(int code, const char *what, uint64_t segment)
{
    char msg[200];
    std::snprintf(msg, sizeof msg, "vsc_cds_build: segment %llu: %s", (unsigned long long)segment, what);
    t_cds_error = msg;
    return code;
}

// CODE of a call: the caller's 64 letters, or the standard code
bool effects_code(const char *code, EffectsCode &out)
{
    if (code && strnlen(code, 64) != 64) return false;
    std::memcpy(out.aa, code ? code : kStandardCode, 64);
    return true;
}

// shape and `to` of an effects call
bool effects_params(const vsc_edit_shape *shape, uint32_t to, EditShape &s)
{
    s = EditShape{shape->site_len, shape->win_start, shape->win_len, shape->from};
    return !(shape->reserved[0] || shape->reserved[1] || shape->reserved[2] || shape->reserved[3]) && edit_shape_valid(s) && to <= 3u &&
           to != s.from;
}

// The arguments every device entry shares, checked on the host.
int effects_check(vsc_ctx *ctx, const vsc_genome *genome, const vsc_edit_shape *shape, uint32_t to, const vsc_cds *cds, const char *code,
                  EditShape &s, EffectsCode &ec, const char *who)
{
    ctx->err.clear();
    if (!genome || !shape || !cds) return fail_in(ctx, VSC_ERR_INVALID, who, "null argument");
    if (genome->ctx != ctx) return fail_in(ctx, VSC_ERR_INVALID, who, "genome belongs to another context");
    if (!effects_params(shape, to, s))
        return fail_in(ctx, VSC_ERR_INVALID, who,
                       "site_len 16 .. 32, 1 <= win_len <= 16, win_start + win_len <= site_len, from 0 .. 3, to 0 .. 3 and not from, reserved fields 0");
    if (!effects_code(code, ec)) return fail_in(ctx, VSC_ERR_INVALID, who, "the code has fewer than 64 letters");
    bool same = cds->contig_off.size() == genome->h_contig_off.size() && genome->h_contig_off.size() == genome->h_contig_end.size();
    for (size_t c = 0; same && c < cds->contig_off.size(); ++c)
        same = cds->contig_off[c] == genome->h_contig_off[c] && cds->contig_off[c] + cds->contig_len[c] == genome->h_contig_end[c];
    if (!same) return fail_in(ctx, VSC_ERR_INVALID, who, "the CDS was built with another contig table than the genome's");
    return VSC_OK;
}

// the device copy of the segments: [global starts][segments], keyed by the object's serial number
int effects_upload_cds(vsc_ctx *ctx, const vsc_cds *cds, CdsView &v)
{
    const size_t n = cds->seg.size(), start_bytes = round256(n * sizeof(uint32_t) + 4);
    if (ctx->cds_serial != cds->serial) {
        ctx->cds_serial = 0;
        VSC_HIP(ctx, ctx->cds_buf.ensure(start_bytes + n * sizeof(CdsSeg) + sizeof(CdsSeg)));  // (never empty)
        if (n) {
            VSC_HIP(ctx, hipMemcpyAsync(ctx->cds_buf.p, cds->gstart.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
            VSC_HIP(ctx, hipMemcpyAsync((char *)ctx->cds_buf.p + start_bytes, cds->seg.data(), n * sizeof(CdsSeg), hipMemcpyHostToDevice,
                                        ctx->stream));
        }
        VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (the caller may free the object as soon as its call returns)
        ctx->cds_serial = cds->serial;
    }
    v = CdsView{(const uint32_t *)ctx->cds_buf.p, (const CdsSeg *)((const char *)ctx->cds_buf.p + start_bytes), (uint32_t)n};
    return VSC_OK;
}

// the planes of the letters of a CDS object's contigs, as the genome's are packed: what lies between the contigs is N
// (vsc_effects_site_text, vsc_knockout_site_text); total = the end of the last contig
struct TextPlanes {
    std::vector<uint32_t> hi, lo, nm, ends;
    uint64_t words;
    TextPlanes(const vsc_cds *cds, const char *const *texts, uint64_t total)
        : hi((size_t)((total + 31) / 32 + 1), 0u), lo(hi.size(), 0u), nm(hi.size(), 0xFFFFFFFFu), ends(cds->contig_off.size()), words(hi.size())
    {
        for (uint32_t c = 0; c < (uint32_t)ends.size(); ++c) {
            ends[c] = cds->contig_off[c] + cds->contig_len[c];
            for (uint32_t i = 0; i < cds->contig_len[c]; ++i) {
                const int b = base_code(texts[c][i]);
                if (b > 3) continue;
                const uint64_t x = (uint64_t)cds->contig_off[c] + i;
                nm[x >> 5] &= ~(1u << (x & 31));
                hi[x >> 5] |= (uint32_t)(b >> 1) << (x & 31);
                lo[x >> 5] |= (uint32_t)(b & 1) << (x & 31);
            }
        }
    }
    EffPlanes view(const vsc_cds *cds) const
    {
        return EffPlanes{hi.data(), lo.data(), nm.data(), 0, words, words, cds->contig_off.data(), ends.data(), (uint32_t)ends.size()};
    }
};

const CandidateRule kEffectsRule{"the shape's site_len must be 23", kEffectsMaxCount, "more than 0xFFFFFFFE candidates"};
static_assert((kEffectsCounts + 2) * sizeof(unsigned long long) <= 256, "the counters and the covered transcripts lie in the head");

// Rows, records and coverage of the loci `at`: effects_rows_kernel, then the join of the rows with the transcripts - always,
// the records do not depend on a table of the call's - whose coverage is the stop_gained effects per transcript.
int effects_run(vsc_ctx *ctx, const vsc_genome *genome, const EditShape &shape, uint32_t to, const vsc_cds *cds, const EffectsCode &code,
                const CandidateLoci &at, uint32_t *rows, vsc_effect *effects, uint64_t capacity, uint64_t *n_effects, uint32_t *coverage,
                vsc_effects_stats *stats, const char *who)
{
    const auto t0 = std::chrono::steady_clock::now();
    const size_t n_tx = cds->n_tx;
    const uint64_t n = at.n;
    if (stats) *stats = vsc_effects_stats{};
    if (n_effects) *n_effects = 0;
    PairCoverage cov(n_tx, coverage, kEffectsUndefined);
    if (n == 0) {
        ctx->timing = vsc_timing{};
        if (stats) stats->wall_ms = wall_ms_since(t0);
        return VSC_OK;
    }
    VSC_HIP(ctx, hipSetDevice(ctx->device));
    // edit_tabs: [stop_gained effects per transcript][their smallest codon][effects per tile][offsets per tile]
    JoinTabs tabs(n, 2 * PairCoverage::bytes(n_tx), 0);
    VSC_HIP(ctx, ctx->edit_tabs.ensure(tabs.bytes()));
    tabs.base = (char *)ctx->edit_tabs.p;
    EffectsArgs a{};
    const int urc = effects_upload_cds(ctx, cds, a.cds);
    if (urc != VSC_OK) return urc;
    a.g = eff_planes(genome);
    a.shape = shape;
    a.to = to;
    a.code = code;
    a.n = n;
    unsigned long long seen[kEffectsCounts] = {};
    const int rrc = rows_pass(ctx, at, sizeof(uint2), rows, seen, kEffectsCounts, [&](unsigned long long *d_stats, void *d_rows, const uint4 *d_loci) {
        a.stats = d_stats;
        a.out = (uint2 *)d_rows;
        a.loci = d_loci;
        return launch_effects_rows(a, ctx->n_cus, ctx->stream);
    });
    if (rrc != VSC_OK) return rrc;
    EffectsRecordArgs p{};
    p.g = a.g;
    p.shape = shape;
    p.to = to;
    p.cds = a.cds;
    p.code = code;
    p.loci = a.loci;
    p.rows = a.out;
    p.n = n;
    p.n_work = tabs.tiles;
    p.n_tx = (uint32_t)n_tx;
    p.tile_count = tabs.tile_count();
    p.tile_off = tabs.tile_off();
    Join j{n, sizeof(uint2), true, effects, sizeof(vsc_effect), capacity, n_effects, kEffectsMaxCount, "more than 0xFFFFFFFE effects",
           "more effects than `capacity` holds; *n_effects is their number"};
    const int jrc = join_passes(
        ctx, tabs, j,
        [&](uint4 *d_effects, bool write) {
            p.effects = d_effects;
            return launch_effects_records(p, write, ctx->stream);
        },
        [&](bool) { return n_tx && seen[kEffClasses + 1 + kEffectStopGained] && (coverage || stats); },
        [&] {
            const int crc = cov.clear(ctx, tabs);
            p.cov_count = cov.count;
            p.cov_min = cov.min;
            return crc;
        },
        [&] { return cov.read(ctx, a.stats + kEffectsCounts + 1); });
    if (jrc != VSC_OK) return jrc;
    const uint64_t covered = cov.take();
    if (stats) {
        class_counts(stats, seen);
        stats->with_effect = seen[kEffClasses];
        stats->effects = j.total;
        for (uint32_t k = 0; k < kEffectClasses; ++k) stats->by_class[k] = seen[kEffClasses + 1 + k];
        stats->transcripts_stopped = covered;
        stats->kernel_ms = j.rows_ms;
        stats->wall_ms = wall_ms_since(t0);
    }
    return join_refusal(ctx, j, who);
}

// vsc_guides_effects / vsc_pattern_guides_effects: over the candidates where they lie, a host-only object from the host
template <class Guides>
int effects_guides(vsc_ctx *ctx, const vsc_genome *genome, Guides *guides, const vsc_edit_shape *shape, uint32_t to, const vsc_cds *cds,
                   const char *code, bool need_23, uint32_t *rows, vsc_effect *effects, uint64_t capacity, uint64_t *n_effects,
                   uint32_t *coverage, vsc_effects_stats *stats, const char *who)
{
    return guarded(ctx, [&]() -> int {
    EditShape s{};
    EffectsCode ec{};
    CandidateLoci at{};
    const int rc = candidate_front(ctx, guides, need_23, kEffectsRule, who, at, &s.site_len,
                                   [&] { return effects_check(ctx, genome, shape, to, cds, code, s, ec, who); }, no_refusal);
    if (rc != VSC_OK) return rc;
    return effects_run(ctx, genome, s, to, cds, ec, at, rows, effects, capacity, n_effects, coverage, stats, who);
    });
}

// vsc_guides_filter_effects / vsc_pattern_guides_filter_effects: the candidates with every required class and no forbidden one
template <class Guides>
int effects_filter(vsc_ctx *ctx, const vsc_genome *genome, Guides *in, const vsc_edit_shape *shape, uint32_t to, const vsc_cds *cds,
                   const char *code, bool need_23, uint32_t require, uint32_t forbid, Guides **out, const char *who)
{
    return guarded(ctx, [&]() -> int {
    EditShape s{};
    EffectsFilterArgs a{};
    const int rc = filter_front(
        ctx, in, out, need_23, kEffectsRule, who, &s.site_len,
        [&] { return effects_check(ctx, genome, shape, to, cds, code, s, a.code, who); },
        [&] { return (require | forbid) >> kEffectClasses ? fail_in(ctx, VSC_ERR_INVALID, who, "require / forbid are masks over bits 0 .. 5") : VSC_OK; });
    if (rc != VSC_OK) return rc;
    const int urc = effects_upload_cds(ctx, cds, a.cds);
    if (urc != VSC_OK) return urc;
    a.g = eff_planes(genome);
    a.shape = s;
    a.to = to;
    a.require = require;
    a.forbid = forbid;
    return filter_candidates(ctx, in, a, kEditTile, out, who, [&](bool write) { return launch_effects_filter(a, write, ctx->stream); });
    });
}

}  // namespace

extern "C" {

int vsc_cds_build(const vsc_contig *contigs, uint32_t n_contigs, const vsc_cds_segment *segments, uint64_t n, uint32_t n_tx, vsc_cds **out)
{
    if (!out) return VSC_ERR_INVALID;
    *out = nullptr;
    try {
        t_cds_error.clear();
        if ((n_contigs && !contigs) || (n && !segments)) {
            t_cds_error = "vsc_cds_build: null argument";
            return VSC_ERR_INVALID;
        }
        if (n > kEffectsMaxCount) {
            t_cds_error = "vsc_cds_build: more than 0xFFFFFFFE segments";
            return VSC_ERR_RANGE;
        }
        std::unique_ptr<vsc_cds> c(new vsc_cds());
        for (uint32_t k = 0; k < n_contigs; ++k) {
            if (contigs[k].offset + contigs[k].length >= (1ull << 32)) {
                t_cds_error = "vsc_cds_build: the contigs end beyond 2^32";
                return VSC_ERR_RANGE;
            }
            c->contig_off.push_back((uint32_t)contigs[k].offset);
            c->contig_len.push_back(contigs[k].length);
        }
        c->n_tx = n_tx;
        c->ko_tx.assign(n_tx, KoTx{0u, 0u, 0u, 0u});
        uint64_t genome_end = 0;
        for (uint32_t k = 0; k < n_contigs; ++k) genome_end = std::max<uint64_t>(genome_end, (uint64_t)c->contig_off[k] + c->contig_len[k]);
        c->ko_blocks = (uint32_t)((genome_end + (1u << kKoBlockBits) - 1u) >> kKoBlockBits);
        c->ko_bitmap.assign((size_t)c->ko_blocks / 32u + 1u, 0u);
        c->gstart.resize((size_t)n);
        c->seg.resize((size_t)n);
        // per transcript: its first segment in genome order, its last one, contig and strand, its bases
        struct Tx {
            uint32_t first = kCdsNone, last = kCdsNone, contig = 0, strand = 0;
            uint64_t bases = 0;
        };
        std::vector<Tx> tx(n_tx);
        std::vector<uint32_t> after((size_t)n, kCdsNone), before((size_t)n, kCdsNone);  // the transcript's next / previous segment in GENOME order
        for (uint64_t i = 0; i < n; ++i) {
            const vsc_cds_segment &s = segments[i];
            if (s.reserved[0] || s.reserved[1]) return cds_refuse(VSC_ERR_INVALID, "a reserved field is not 0", i);
            if (s.contig >= n_contigs) return cds_refuse(VSC_ERR_INVALID, "it lies on an unknown contig", i);
            if (s.strand > 1u || s.phase > 2u) return cds_refuse(VSC_ERR_INVALID, "strand is 0 or 1, phase 0 .. 2", i);
            if (s.start >= s.end) return cds_refuse(VSC_ERR_INVALID, "it is empty", i);
            if (s.end > contigs[s.contig].length) return cds_refuse(VSC_ERR_INVALID, "it reaches beyond its contig", i);
            if (s.transcript >= n_tx) return cds_refuse(VSC_ERR_INVALID, "its transcript is not below n_tx", i);
            if (i) {
                const vsc_cds_segment &q = segments[i - 1];
                if (q.contig > s.contig || (q.contig == s.contig && q.start >= s.start))
                    return cds_refuse(VSC_ERR_INVALID, "the segments are not strictly ascending by (contig, start)", i);
                if (q.contig == s.contig && q.end > s.start) return cds_refuse(VSC_ERR_INVALID, "it overlaps the segment in front of it", i);
            }
            Tx &t = tx[s.transcript];
            if (t.first == kCdsNone) {
                t.first = (uint32_t)i;
                t.contig = s.contig;
                t.strand = s.strand;
            } else {
                if (t.contig != s.contig) return cds_refuse(VSC_ERR_INVALID, "its transcript lies on two contigs", i);
                if (t.strand != s.strand) return cds_refuse(VSC_ERR_INVALID, "its transcript lies on two strands", i);
                after[t.last] = (uint32_t)i;
                before[i] = t.last;
            }
            t.last = (uint32_t)i;
            t.bases += s.end - s.start;
            if (t.bases + 2u >= (1ull << 31)) return cds_refuse(VSC_ERR_RANGE, "its transcript's coding length reaches 2^31", i);
            const uint32_t off = c->contig_off[s.contig];
            c->gstart[i] = off + s.start;
            c->seg[i] = CdsSeg{off + s.start, off + s.end, s.transcript, 0u, kCdsNone, kCdsNone, s.strand, 0u};
        }
        uint64_t used = 0, bases = 0;
        for (uint32_t k = 0; k < n_tx; ++k) {
            const Tx &t = tx[k];
            if (t.first == kCdsNone) continue;
            ++used;
            bases += t.bases;
            // transcript order: ascending start on '+', descending on '-'
            const std::vector<uint32_t> &fwd = t.strand ? before : after, &bwd = t.strand ? after : before;
            const uint32_t head = t.strand ? t.last : t.first;
            const uint32_t shift = (3u - segments[head].phase) % 3u;
            uint32_t ci = shift;
            KoTx &ko = c->ko_tx[k];
            for (uint32_t i = head; i != kCdsNone; i = fwd[i]) {
                ko.junction = ci;  // (the last one stays: the first base of the last segment in transcript order)
                ++ko.n_seg;
                if (i != head && segments[i].phase != (3u - ci % 3u) % 3u)
                    return cds_refuse(VSC_ERR_INVALID, "its phase does not continue its transcript's reading frame", i);
                CdsSeg &sg = c->seg[i];
                sg.ci0 = ci;
                sg.prev = bwd[i];
                sg.next = fwd[i];
                sg.shift = shift;
                ci += sg.gend - sg.gstart;
            }
            ko.shift = shift;
            ko.end = ci;
        }
        for (const CdsSeg &sg : c->seg)
            for (uint32_t b = sg.gstart >> kKoBlockBits; b <= (sg.gend - 1u) >> kKoBlockBits; ++b) c->ko_bitmap[b >> 5] |= 1u << (b & 31u);
        c->stats.segments = n;
        c->stats.transcripts = n_tx;
        c->stats.transcripts_used = used;
        c->stats.coding_bases = bases;
        c->serial = g_cds_serial.fetch_add(1, std::memory_order_relaxed) + 1;
        *out = c.release();
        return VSC_OK;
    } catch (const std::bad_alloc &) {
        return VSC_ERR_NOMEM;
    } catch (...) {
        return VSC_ERR_INVALID;
    }
}

const char *vsc_cds_build_error(void) { return t_cds_error.c_str(); }

void vsc_cds_free(vsc_cds *cds) { delete cds; }

int vsc_cds_info(const vsc_cds *cds, vsc_cds_stats *out)
{
    if (!cds || !out) return VSC_ERR_INVALID;
    *out = cds->stats;
    return VSC_OK;
}

int vsc_codon_effect(uint32_t ref, uint32_t alt, uint32_t codon, uint32_t first_phase, const char *code, uint32_t *effect_class_out)
{
    EffectsCode ec{};
    if (!effect_class_out || ref > 63u || alt > 63u || first_phase > 2u || !effects_code(code, ec)) return VSC_ERR_INVALID;
    *effect_class_out = effect_class(ref, alt, codon, first_phase == 0u, ec.aa, false);
    return VSC_OK;
}

int vsc_effects_site_text(const vsc_cds *cds, const char *const *texts, uint32_t contig, uint32_t pos, uint32_t strand,
                          const vsc_edit_shape *shape, uint32_t to, const char *code, uint32_t *row, vsc_effect *effects, uint32_t *n_effects)
{
    if (!cds || !shape || !row || !effects || !n_effects) return VSC_ERR_INVALID;
    try {
        EditShape s{};
        EffectsCode ec{};
        if (!effects_params(shape, to, s) || !effects_code(code, ec)) return VSC_ERR_INVALID;
        const uint32_t nc = (uint32_t)cds->contig_off.size();
        if (nc && !texts) return VSC_ERR_INVALID;
        uint64_t total = 0;
        for (uint32_t c = 0; c < nc; ++c) {
            if (cds->contig_len[c] && !texts[c]) return VSC_ERR_INVALID;
            total = std::max<uint64_t>(total, (uint64_t)cds->contig_off[c] + cds->contig_len[c]);
        }
        const TextPlanes planes(cds, texts, total);
        const EffPlanes g = planes.view(cds);
        *n_effects = 0;
        row[0] = row[1] = kEffectsUndefined;
        uint64_t ch = 0, cl = 0;
        if (edit_site(g, s, contig, pos, strand, &ch, &cl) != kEffDefined) return VSC_OK;
        const uint32_t mask = edit_mask(ch, cl, s);
        uint32_t count = 0;
        effects_row(g, cds->view(), s, to, ec.aa, cds->contig_off[contig] + edit_window_first(pos, strand, s), strand, mask, &row[0], &row[1],
                    [&](uint32_t tx, uint32_t codon, uint32_t info) {
                        if (count < kEditMaxWindow) effects[count++] = vsc_effect{0u, tx, codon, info};
                    });
        *n_effects = count;
        return VSC_OK;
    } catch (const std::bad_alloc &) {
        return VSC_ERR_NOMEM;
    } catch (...) {
        return VSC_ERR_INVALID;
    }
}

int vsc_loci_effects(vsc_ctx *ctx, const vsc_genome *genome, const vsc_locus *loci, uint64_t n, const vsc_edit_shape *shape, uint32_t to,
                     const vsc_cds *cds, const char *code, uint32_t *rows, vsc_effect *effects, uint64_t capacity, uint64_t *n_effects,
                     uint32_t *coverage, vsc_effects_stats *stats)
{
    return guarded(ctx, [&]() -> int {
    if (!ctx) return VSC_ERR_INVALID;
    const char *const fn = "vsc_loci_effects";
    EditShape s{};
    EffectsCode ec{};
    const int rc = effects_check(ctx, genome, shape, to, cds, code, s, ec, fn);
    if (rc != VSC_OK) return rc;
    if (n && !loci) return fail_in(ctx, VSC_ERR_INVALID, fn, "null argument");
    if (n > kEffectsMaxCount) return fail_in(ctx, VSC_ERR_RANGE, fn, "more than 0xFFFFFFFE candidates");
    return effects_run(ctx, genome, s, to, cds, ec, CandidateLoci{nullptr, loci, n}, rows, effects, capacity, n_effects, coverage, stats, fn);
    });
}

int vsc_guides_effects(vsc_ctx *ctx, const vsc_genome *genome, vsc_guides *guides, const vsc_edit_shape *shape, uint32_t to,
                       const vsc_cds *cds, const char *code, uint32_t *rows, vsc_effect *effects, uint64_t capacity, uint64_t *n_effects,
                       uint32_t *coverage, vsc_effects_stats *stats)
{
    return effects_guides(ctx, genome, guides, shape, to, cds, code, true, rows, effects, capacity, n_effects, coverage, stats,
                          "vsc_guides_effects");
}

int vsc_pattern_guides_effects(vsc_ctx *ctx, const vsc_genome *genome, vsc_pattern_guides *guides, const vsc_edit_shape *shape, uint32_t to,
                               const vsc_cds *cds, const char *code, uint32_t *rows, vsc_effect *effects, uint64_t capacity,
                               uint64_t *n_effects, uint32_t *coverage, vsc_effects_stats *stats)
{
    return effects_guides(ctx, genome, guides, shape, to, cds, code, false, rows, effects, capacity, n_effects, coverage, stats,
                          "vsc_pattern_guides_effects");
}

int vsc_guides_filter_effects(vsc_ctx *ctx, const vsc_genome *genome, vsc_guides *in, const vsc_edit_shape *shape, uint32_t to,
                              const vsc_cds *cds, const char *code, uint32_t require, uint32_t forbid, vsc_guides **out)
{
    return effects_filter(ctx, genome, in, shape, to, cds, code, true, require, forbid, out, "vsc_guides_filter_effects");
}

int vsc_pattern_guides_filter_effects(vsc_ctx *ctx, const vsc_genome *genome, vsc_pattern_guides *in, const vsc_edit_shape *shape,
                                      uint32_t to, const vsc_cds *cds, const char *code, uint32_t require, uint32_t forbid,
                                      vsc_pattern_guides **out)
{
    return effects_filter(ctx, genome, in, shape, to, cds, code, false, require, forbid, out, "vsc_pattern_guides_filter_effects");
}

}  // extern "C"

// ---- knock-out design (the definition: vsc_knockout.h, the kernels: vsc_knockout.hip) ----------------------------
namespace {

const char *const kKoShapeRule =
    "site_len 16 .. 32, 1 <= cut <= site_len - 1, nmd_window and start_window <= 65535, 1 <= max_codons <= 4096, reserved fields 0";

bool knockout_params(const vsc_knockout_shape *shape, KoShape &s)
{
    s = KoShape{shape->site_len, shape->cut, shape->nmd_window, shape->start_window, shape->max_codons};
    return !(shape->reserved[0] || shape->reserved[1] || shape->reserved[2]) && knockout_shape_valid(s);
}

bool knockout_limits(const vsc_knockout_limits *limits, KoFilter &f)
{
    f = KoFilter{limits->min_frac, limits->max_frac, limits->min_edge, limits->require, limits->forbid};
    return !(limits->reserved[0] || limits->reserved[1] || limits->reserved[2]) && knockout_filter_valid(f);
}

// The arguments every device entry shares, checked on the host.
int knockout_check(vsc_ctx *ctx, const vsc_genome *genome, const vsc_knockout_shape *shape, const vsc_cds *cds, const char *code, KoShape &s,
                   EffectsCode &ec, const char *who)
{
    ctx->err.clear();
    if (!genome || !shape || !cds) return fail_in(ctx, VSC_ERR_INVALID, who, "null argument");
    if (genome->ctx != ctx) return fail_in(ctx, VSC_ERR_INVALID, who, "genome belongs to another context");
    if (!knockout_params(shape, s)) return fail_in(ctx, VSC_ERR_INVALID, who, kKoShapeRule);
    if (!effects_code(code, ec)) return fail_in(ctx, VSC_ERR_INVALID, who, "the code has fewer than 64 letters");
    bool same = cds->contig_off.size() == genome->h_contig_off.size() && genome->h_contig_off.size() == genome->h_contig_end.size();
    for (size_t c = 0; same && c < cds->contig_off.size(); ++c)
        same = cds->contig_off[c] == genome->h_contig_off[c] && cds->contig_off[c] + cds->contig_len[c] == genome->h_contig_end[c];
    if (!same) return fail_in(ctx, VSC_ERR_INVALID, who, "the CDS was built with another contig table than the genome's");
    return VSC_OK;
}

// the device copy of what the walk reads beside the segments: [per-transcript table][occupancy bitmap], keyed as cds_buf is
int knockout_upload(vsc_ctx *ctx, const vsc_cds *cds, const KoTx **tx, const uint32_t **bitmap)
{
    const size_t tx_bytes = round256(cds->ko_tx.size() * sizeof(KoTx) + sizeof(KoTx)), map_bytes = cds->ko_bitmap.size() * sizeof(uint32_t);
    if (ctx->ko_serial != cds->serial) {
        ctx->ko_serial = 0;
        VSC_HIP(ctx, ctx->ko_buf.ensure(tx_bytes + map_bytes));
        if (!cds->ko_tx.empty())
            VSC_HIP(ctx, hipMemcpyAsync(ctx->ko_buf.p, cds->ko_tx.data(), cds->ko_tx.size() * sizeof(KoTx), hipMemcpyHostToDevice, ctx->stream));
        VSC_HIP(ctx, hipMemcpyAsync((char *)ctx->ko_buf.p + tx_bytes, cds->ko_bitmap.data(), map_bytes, hipMemcpyHostToDevice, ctx->stream));
        VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (the caller may free the object as soon as its call returns)
        ctx->ko_serial = cds->serial;
    }
    *tx = (const KoTx *)ctx->ko_buf.p;
    *bitmap = (const uint32_t *)((const char *)ctx->ko_buf.p + tx_bytes);
    return VSC_OK;
}

const CandidateRule kKoRule{"the shape's site_len must be 23", kKoMaxCount, "more than 0xFFFFFFFE candidates"};
static_assert((kKoCounts + 1) * sizeof(unsigned long long) <= 256, "the counters and the covered transcripts lie in the head");

// Rows, coverage and stats of the loci `at`: knockout_rows_kernel alone - the coverage is taken where a row is made.
int knockout_run(vsc_ctx *ctx, const vsc_genome *genome, const KoShape &shape, const vsc_cds *cds, const EffectsCode &code, const CandidateLoci &at,
                 uint32_t *rows, uint32_t *coverage, vsc_knockout_stats *stats, const char *who)
{
    const auto t0 = std::chrono::steady_clock::now();
    const size_t n_tx = cds->n_tx;
    const uint64_t n = at.n;
    if (stats) *stats = vsc_knockout_stats{};
    PairCoverage cov(n_tx, coverage, kKoUndefined);
    if (n == 0) {
        ctx->timing = vsc_timing{};
        if (stats) stats->wall_ms = wall_ms_since(t0);
        return VSC_OK;
    }
    VSC_HIP(ctx, hipSetDevice(ctx->device));
    KoArgs a{};
    const int urc = effects_upload_cds(ctx, cds, a.cds);
    if (urc != VSC_OK) return urc;
    const int krc = knockout_upload(ctx, cds, &a.tx, &a.bitmap);
    if (krc != VSC_OK) return krc;
    a.g = eff_planes(genome);
    a.shape = shape;
    a.n_blocks = cds->ko_blocks;
    a.n_tx = (uint32_t)n_tx;
    a.code = code;
    a.n = n;
    const bool cover = n_tx && (coverage || stats);
    if (cover) {  // edit_tabs: [candidates with NMD in both frames per transcript][their smallest codon]
        JoinTabs tabs(0, 2 * PairCoverage::bytes(n_tx), 0);
        VSC_HIP(ctx, ctx->edit_tabs.ensure(tabs.bytes()));
        tabs.base = (char *)ctx->edit_tabs.p;
        const int crc = cov.clear(ctx, tabs);
        if (crc != VSC_OK) return crc;
        a.cov_count = cov.count;
        a.cov_min = cov.min;
    }
    unsigned long long seen[kKoCounts] = {};
    const int rrc = rows_pass(ctx, at, sizeof(uint4), rows, seen, kKoCounts, [&](unsigned long long *d_stats, void *d_rows, const uint4 *d_loci) {
        a.stats = d_stats;
        a.out = (uint4 *)d_rows;
        a.loci = d_loci;
        return launch_knockout_rows(a, ctx->n_cus, ctx->knockout_groups_per_cu, ctx->knockout_in_place, ctx->stream);
    });
    if (rrc != VSC_OK) return rrc;
    if (cover) {
        const int crc = cov.read(ctx, a.stats + kKoCounts);
        if (crc != VSC_OK) return crc;
    }
    VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    float ms = 0;
    const int trc = rows_timing(ctx, n, sizeof(uint4), 0.0f, &ms);
    if (trc != VSC_OK) return trc;
    const uint64_t covered = cov.take();
    if (stats) {
        stats->defined = seen[0];
        stats->undefined = seen[1];
        stats->coding = seen[2];
        stats->junction = seen[3];
        stats->ptc[0] = seen[4];
        stats->ptc[1] = seen[5];
        stats->nmd[0] = seen[6];
        stats->nmd[1] = seen[7];
        stats->unknown = seen[8];
        stats->past_find = seen[9];
        stats->drains = seen[10];
        stats->drained = seen[11];
        stats->transcripts_covered = covered;
        stats->kernel_ms = ms;
        stats->wall_ms = wall_ms_since(t0);
    }
    return VSC_OK;
}

// vsc_guides_knockout / vsc_pattern_guides_knockout: over the candidates where they lie, a host-only object from the host
template <class Guides>
int knockout_guides(vsc_ctx *ctx, const vsc_genome *genome, Guides *guides, const vsc_knockout_shape *shape, const vsc_cds *cds, const char *code,
                    bool need_23, uint32_t *rows, uint32_t *coverage, vsc_knockout_stats *stats, const char *who)
{
    return guarded(ctx, [&]() -> int {
    KoShape s{};
    EffectsCode ec{};
    CandidateLoci at{};
    const int rc = candidate_front(ctx, guides, need_23, kKoRule, who, at, &s.site_len,
                                   [&] { return knockout_check(ctx, genome, shape, cds, code, s, ec, who); }, no_refusal);
    if (rc != VSC_OK) return rc;
    return knockout_run(ctx, genome, s, cds, ec, at, rows, coverage, stats, who);
    });
}

// vsc_guides_filter_knockout / vsc_pattern_guides_filter_knockout: the candidates that pass FILTER, in the input's order
template <class Guides>
int knockout_filter(vsc_ctx *ctx, const vsc_genome *genome, Guides *in, const vsc_knockout_shape *shape, const vsc_cds *cds, const char *code,
                    bool need_23, const vsc_knockout_limits *limits, Guides **out, const char *who)
{
    return guarded(ctx, [&]() -> int {
    KoShape s{};
    KoFilterArgs a{};
    const int rc = filter_front(
        ctx, in, out, need_23, kKoRule, who, &s.site_len, [&] { return knockout_check(ctx, genome, shape, cds, code, s, a.code, who); },
        [&] {
            if (!limits) return fail_in(ctx, VSC_ERR_INVALID, who, "null argument");
            return knockout_limits(limits, a.filter)
                       ? VSC_OK
                       : fail_in(ctx, VSC_ERR_INVALID, who,
                                 "min_frac <= max_frac <= 65535, min_edge <= 255, require / forbid are masks over bits 0 .. 6, reserved fields 0");
        });
    if (rc != VSC_OK) return rc;
    const int urc = effects_upload_cds(ctx, cds, a.cds);
    if (urc != VSC_OK) return urc;
    const int krc = knockout_upload(ctx, cds, &a.tx, &a.bitmap);
    if (krc != VSC_OK) return krc;
    a.g = eff_planes(genome);
    a.shape = s;
    a.n_blocks = cds->ko_blocks;
    a.n_tx = cds->n_tx;
    return filter_candidates(ctx, in, a, kEditTile, out, who, [&](bool write) { return launch_knockout_filter(a, write, ctx->stream); });
    });
}

}  // namespace

extern "C" {

int vsc_debug_knockout_groups_per_cu(vsc_ctx *ctx, uint32_t groups)
{
    if (!ctx || groups > kKoMaxGroupsPerCu) return VSC_ERR_INVALID;
    ctx->knockout_groups_per_cu = groups;
    return VSC_OK;
}

int vsc_debug_knockout_in_place(vsc_ctx *ctx, int on)
{
    if (!ctx) return VSC_ERR_INVALID;
    ctx->knockout_in_place = on != 0;
    return VSC_OK;
}

int vsc_debug_knockout_table(const vsc_cds *cds, uint32_t *table, uint32_t *bitmap, uint32_t *n_blocks)
{
    if (!cds || !n_blocks) return VSC_ERR_INVALID;
    *n_blocks = cds->ko_blocks;
    if (table && !cds->ko_tx.empty()) std::memcpy(table, cds->ko_tx.data(), cds->ko_tx.size() * sizeof(KoTx));
    if (bitmap) std::memcpy(bitmap, cds->ko_bitmap.data(), ((size_t)cds->ko_blocks + 31) / 32 * sizeof(uint32_t));
    return VSC_OK;
}

int vsc_knockout_site_text(const vsc_cds *cds, const char *const *texts, uint32_t contig, uint32_t pos, uint32_t strand,
                           const vsc_knockout_shape *shape, const char *code, uint32_t *row)
{
    if (!cds || !shape || !row) return VSC_ERR_INVALID;
    try {
        KoShape s{};
        EffectsCode ec{};
        if (!knockout_params(shape, s) || !effects_code(code, ec)) return VSC_ERR_INVALID;
        const uint32_t nc = (uint32_t)cds->contig_off.size();
        if (nc && !texts) return VSC_ERR_INVALID;
        uint64_t total = 0;
        for (uint32_t c = 0; c < nc; ++c) {
            if (cds->contig_len[c] && !texts[c]) return VSC_ERR_INVALID;
            total = std::max<uint64_t>(total, (uint64_t)cds->contig_off[c] + cds->contig_len[c]);
        }
        const TextPlanes planes(cds, texts, total);
        knockout_row(planes.view(cds), cds->view(), cds->ko_tx.data(), s, ec.aa, contig, pos, strand, row);
        return VSC_OK;
    } catch (const std::bad_alloc &) {
        return VSC_ERR_NOMEM;
    } catch (...) {
        return VSC_ERR_INVALID;
    }
}

int vsc_loci_knockout(vsc_ctx *ctx, const vsc_genome *genome, const vsc_locus *loci, uint64_t n, const vsc_knockout_shape *shape,
                      const vsc_cds *cds, const char *code, uint32_t *rows, uint32_t *coverage, vsc_knockout_stats *stats)
{
    return guarded(ctx, [&]() -> int {
    if (!ctx) return VSC_ERR_INVALID;
    const char *const fn = "vsc_loci_knockout";
    KoShape s{};
    EffectsCode ec{};
    const int rc = knockout_check(ctx, genome, shape, cds, code, s, ec, fn);
    if (rc != VSC_OK) return rc;
    if (n && !loci) return fail_in(ctx, VSC_ERR_INVALID, fn, "null argument");
    if (n > kKoMaxCount) return fail_in(ctx, VSC_ERR_RANGE, fn, "more than 0xFFFFFFFE candidates");
    return knockout_run(ctx, genome, s, cds, ec, CandidateLoci{nullptr, loci, n}, rows, coverage, stats, fn);
    });
}

int vsc_guides_knockout(vsc_ctx *ctx, const vsc_genome *genome, vsc_guides *guides, const vsc_knockout_shape *shape, const vsc_cds *cds,
                        const char *code, uint32_t *rows, uint32_t *coverage, vsc_knockout_stats *stats)
{
    return knockout_guides(ctx, genome, guides, shape, cds, code, true, rows, coverage, stats, "vsc_guides_knockout");
}

int vsc_pattern_guides_knockout(vsc_ctx *ctx, const vsc_genome *genome, vsc_pattern_guides *guides, const vsc_knockout_shape *shape,
                                const vsc_cds *cds, const char *code, uint32_t *rows, uint32_t *coverage, vsc_knockout_stats *stats)
{
    return knockout_guides(ctx, genome, guides, shape, cds, code, false, rows, coverage, stats, "vsc_pattern_guides_knockout");
}

int vsc_guides_filter_knockout(vsc_ctx *ctx, const vsc_genome *genome, vsc_guides *in, const vsc_knockout_shape *shape, const vsc_cds *cds,
                               const char *code, const vsc_knockout_limits *limits, vsc_guides **out)
{
    return knockout_filter(ctx, genome, in, shape, cds, code, true, limits, out, "vsc_guides_filter_knockout");
}

int vsc_pattern_guides_filter_knockout(vsc_ctx *ctx, const vsc_genome *genome, vsc_pattern_guides *in, const vsc_knockout_shape *shape,
                                       const vsc_cds *cds, const char *code, const vsc_knockout_limits *limits, vsc_pattern_guides **out)
{
    return knockout_filter(ctx, genome, in, shape, cds, code, false, limits, out, "vsc_pattern_guides_filter_knockout");
}

}  // extern "C"

// ---- HDR knock-in design (the definition: vsc_hdr.h, the kernels: vsc_hdr.hip) -----------------------------------
namespace {

const char *const kHdrShapeRule =
    "site_len 16 .. 32, up and down <= 32, up + site_len + down <= 64, 1 <= cut <= site_len - 1, max_dist <= 63, anchor 0 or 1, the pam "
    "(len <= 8), seed (len <= 16) and protospacer (len <= 32) ranges inside the site, pam_accept 1 .. 15 below pam_len and 0 from it on, "
    "min_seed_mm <= seed_len, min_proto_mm <= proto_len, flags <= 7, reserved fields 0";

bool hdr_shape_in(const vsc_hdr_shape *shape, HdrShape &s)
{
    s = HdrShape{};
    s.up = shape->up;
    s.site_len = shape->site_len;
    s.down = shape->down;
    s.cut = shape->cut;
    s.max_dist = shape->max_dist;
    s.anchor = shape->anchor;
    s.pam_start = shape->pam_start;
    s.pam_len = shape->pam_len;
    for (uint32_t j = 0; j < kHdrMaxPam; ++j) s.pam_accept[j] = shape->pam_accept[j];
    s.seed_start = shape->seed_start;
    s.seed_len = shape->seed_len;
    s.proto_start = shape->proto_start;
    s.proto_len = shape->proto_len;
    s.min_seed_mm = shape->min_seed_mm;
    s.min_proto_mm = shape->min_proto_mm;
    s.flags = shape->flags;
    return shape->reserved == 0u && hdr_shape_valid(s);
}

// The shape, the genome, the edits, the CDS and CODE of an HDR call, checked on the host.
int hdr_check(vsc_ctx *ctx, const vsc_genome *genome, const vsc_hdr_shape *shape, const vsc_prime_edit *edits, uint64_t n_e, const vsc_cds *cds,
              const char *code, HdrShape &s, PrimeHostEdits &h, HdrTables &tabs, const char *who)
{
    ctx->err.clear();
    if (!genome || !shape) return fail_in(ctx, VSC_ERR_INVALID, who, "null argument");
    if (genome->ctx != ctx) return fail_in(ctx, VSC_ERR_INVALID, who, "genome belongs to another context");
    if (!hdr_shape_in(shape, s)) return fail_in(ctx, VSC_ERR_INVALID, who, kHdrShapeRule);
    EffectsCode ec{};
    if (!effects_code(code, ec)) return fail_in(ctx, VSC_ERR_INVALID, who, "the code has fewer than 64 letters");
    std::memcpy(tabs.aa, ec.aa, 64);
    for (uint32_t j = 0; j < kHdrMaxPam; ++j) tabs.accept[j] = s.pam_accept[j];
    if (cds) {
        bool same = cds->contig_off.size() == genome->h_contig_off.size() && genome->h_contig_off.size() == genome->h_contig_end.size();
        for (size_t c = 0; same && c < cds->contig_off.size(); ++c)
            same = cds->contig_off[c] == genome->h_contig_off[c] && cds->contig_off[c] + cds->contig_len[c] == genome->h_contig_end[c];
        if (!same) return fail_in(ctx, VSC_ERR_INVALID, who, "the CDS was built with another contig table than the genome's");
    }
    return prime_edits_check(ctx, genome, edits, n_e, h, who);
}

const CandidateRule kHdrRule{"the shape's site_len must be 23", kHdrMaxCount, "more than 0xFFFFFFFE candidates"};

// Rows, pairs and coverage of the loci `at`: hdr_rows_kernel, then - with edits - the join of the rows with them, whose write
// pass also counts the pairs by flag.
int hdr_run(vsc_ctx *ctx, const vsc_genome *genome, const HdrShape &shape, const PrimeHostEdits &h, const vsc_cds *cds, const HdrTables &tables,
            const CandidateLoci &at, uint32_t *rows, vsc_hdr_pair *pairs, uint64_t capacity, uint64_t *n_pairs, uint32_t *coverage,
            vsc_hdr_stats *stats, const char *who)
{
    const auto t0 = std::chrono::steady_clock::now();
    const size_t n_e = h.gpos.size();
    const uint64_t n = at.n;
    if (stats) *stats = vsc_hdr_stats{};
    if (n_pairs) *n_pairs = 0;
    PairCoverage cov(n_e, coverage, kHdrUndefined);
    if (n == 0) {
        ctx->timing = vsc_timing{};
        if (stats) stats->wall_ms = wall_ms_since(t0);
        return VSC_OK;
    }
    VSC_HIP(ctx, hipSetDevice(ctx->device));
    // edit_tabs behind the edits: [usable pairs per edit][their smallest dist][pairs per tile][offsets per tile][pairs by flag]
    const size_t flag_bytes = 256;
    JoinTabs tabs(n, 2 * PairCoverage::bytes(n_e), flag_bytes);
    HdrArgs a{};
    const int urc = prime_upload_edits(ctx, h, tabs.bytes(), a.edits, &tabs.base, ctx->hdr_bitmap);
    if (urc != VSC_OK) return urc;
    if (cds) {
        const int crc = effects_upload_cds(ctx, cds, a.cds);
        if (crc != VSC_OK) return crc;
        a.have_cds = 1u;
    }
    a.g = eff_planes(genome);
    a.shape = shape;
    a.tabs = tables;
    a.n = n;
    unsigned long long seen[kHdrCounts] = {};
    const int rrc = rows_pass(ctx, at, sizeof(uint2), rows, seen, kHdrCounts, [&](unsigned long long *d_stats, void *d_rows, const uint4 *d_loci) {
        a.stats = d_stats;
        a.out = (uint2 *)d_rows;
        a.loci = d_loci;
        return launch_hdr_rows(a, ctx->n_cus, ctx->hdr_groups_per_cu, ctx->stream);
    });
    if (rrc != VSC_OK) return rrc;
    HdrPairArgs p{};
    p.g = a.g;
    p.shape = shape;
    p.edits = a.edits;
    p.cds = a.cds;
    p.have_cds = a.have_cds;
    p.tabs = tables;
    p.loci = a.loci;
    p.rows = a.out;
    p.n = n;
    p.n_work = tabs.tiles;
    p.tile_count = tabs.tile_count();
    p.tile_off = tabs.tile_off();
    Join j{n, sizeof(uint2), n_e != 0, pairs, sizeof(vsc_hdr_pair), capacity, n_pairs, kHdrMaxCount, "more than 0xFFFFFFFE pairs",
           "more pairs than `capacity` holds; *n_pairs is their number"};
    unsigned long long by_flag[kHdrFlags] = {};
    const int jrc = join_passes(
        ctx, tabs, j,
        [&](uint4 *d_pairs, bool write) {
            p.pairs = d_pairs;
            return launch_hdr_pairs(p, write, ctx->stream);
        },
        [&](bool) { return coverage || stats; },
        [&] {
            const int crc = cov.clear(ctx, tabs);
            if (crc != VSC_OK) return crc;
            p.cov_count = cov.count;
            p.cov_min = cov.min;
            p.flag_count = (unsigned long long *)tabs.extra();
            VSC_HIP(ctx, hipMemsetAsync(p.flag_count, 0, flag_bytes, ctx->stream));
            return VSC_OK;
        },
        [&] {
            VSC_HIP(ctx, hipMemcpyAsync(by_flag, p.flag_count, sizeof by_flag, hipMemcpyDeviceToHost, ctx->stream));
            return cov.read(ctx, a.stats + kHdrCounts + 1);
        });
    if (jrc != VSC_OK) return jrc;
    const uint64_t covered = cov.take();
    if (stats) {
        class_counts(stats, seen);
        stats->with_pair = seen[kEffClasses];
        stats->with_usable = seen[kEffClasses + 1];
        stats->pairs = j.total;
        for (uint32_t b = 0; b < kHdrFlags; ++b) stats->pairs_by_flag[b] = by_flag[b];
        stats->edits_covered = covered;
        stats->score_ms = j.rows_ms;
        stats->wall_ms = wall_ms_since(t0);
    }
    return join_refusal(ctx, j, who);
}

// vsc_guides_hdr / vsc_pattern_guides_hdr: over the candidates where they lie, a host-only object from the host
template <class Guides>
int hdr_guides(vsc_ctx *ctx, const vsc_genome *genome, Guides *guides, const vsc_hdr_shape *shape, const vsc_prime_edit *edits, uint64_t n_e,
               const vsc_cds *cds, const char *code, bool need_23, uint32_t *rows, vsc_hdr_pair *pairs, uint64_t capacity, uint64_t *n_pairs,
               uint32_t *coverage, vsc_hdr_stats *stats, const char *who)
{
    return guarded(ctx, [&]() -> int {
    HdrShape s{};
    PrimeHostEdits h;
    HdrTables tables{};
    CandidateLoci at{};
    const int rc = candidate_front(ctx, guides, need_23, kHdrRule, who, at, &s.site_len,
                                   [&] { return hdr_check(ctx, genome, shape, edits, n_e, cds, code, s, h, tables, who); }, no_refusal);
    if (rc != VSC_OK) return rc;
    return hdr_run(ctx, genome, s, h, cds, tables, at, rows, pairs, capacity, n_pairs, coverage, stats, who);
    });
}

// vsc_guides_filter_hdr / vsc_pattern_guides_filter_hdr: the candidates with a usable pair, or - allow_open - with any pair
template <class Guides>
int hdr_filter(vsc_ctx *ctx, const vsc_genome *genome, Guides *in, const vsc_hdr_shape *shape, const vsc_prime_edit *edits, uint64_t n_e,
               const vsc_cds *cds, const char *code, bool need_23, uint32_t allow_open, Guides **out, const char *who)
{
    return guarded(ctx, [&]() -> int {
    HdrShape s{};
    PrimeHostEdits h;
    HdrFilterArgs a{};
    const int rc = filter_front(ctx, in, out, need_23, kHdrRule, who, &s.site_len,
                                [&] { return hdr_check(ctx, genome, shape, edits, n_e, cds, code, s, h, a.tabs, who); }, no_refusal);
    if (rc != VSC_OK) return rc;
    const int urc = prime_upload_edits(ctx, h, 0, a.edits, nullptr, ctx->hdr_bitmap);
    if (urc != VSC_OK) return urc;
    if (cds) {
        const int crc = effects_upload_cds(ctx, cds, a.cds);
        if (crc != VSC_OK) return crc;
        a.have_cds = 1u;
    }
    if (in->n == 0) VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (the edits are this call's vectors, and no pass will wait)
    a.g = eff_planes(genome);
    a.shape = s;
    a.allow_open = allow_open ? 1u : 0u;
    return filter_candidates(ctx, in, a, kEditTile, out, who, [&](bool write) { return launch_hdr_filter(a, write, ctx->stream); });
    });
}

}  // namespace

extern "C" {

int vsc_debug_hdr_bitmap(vsc_ctx *ctx, int on)
{
    if (!ctx) return VSC_ERR_INVALID;
    ctx->hdr_bitmap = on != 0;
    return VSC_OK;
}

int vsc_debug_hdr_groups_per_cu(vsc_ctx *ctx, uint32_t groups)
{
    if (!ctx || groups > kHdrMaxGroupsPerCu) return VSC_ERR_INVALID;
    ctx->hdr_groups_per_cu = groups;
    return VSC_OK;
}

int vsc_hdr_site_text(const char *context, const vsc_hdr_shape *shape, uint32_t e0, uint32_t del_len, const char *ins, const uint8_t *allowed,
                      uint32_t *pair, char *edited)
{
    if (!context || !shape || !ins || !pair) return VSC_ERR_INVALID;
    HdrShape s{};
    if (!hdr_shape_in(shape, s)) return VSC_ERR_INVALID;
    const uint32_t C = hdr_context_len(s);
    if (strnlen(context, C + 1) != C) return VSC_ERR_INVALID;
    uint64_t ch = 0, cl = 0;
    for (uint32_t j = 0; j < C; ++j) {
        const int b = base_code(context[j]);
        if (b > 3) return VSC_ERR_INVALID;
        ch |= (uint64_t)(b >> 1) << j;
        cl |= (uint64_t)(b & 1) << j;
        if (allowed && allowed[j] > kHdrAnyLetter) return VSC_ERR_INVALID;
    }
    PrimeEdit e{0u, 0u, 0u, 0u};
    const size_t ins_len = strnlen(ins, kPrimeMaxIndel + 1);
    if (ins_len > kPrimeMaxIndel || del_len > kPrimeMaxIndel || del_len + ins_len < 1 || e0 > C || del_len > C - e0) return VSC_ERR_INVALID;
    for (size_t k = 0; k < ins_len; ++k) {
        const int b = base_code(ins[k]);
        if (b > 3) return VSC_ERR_INVALID;
        e.ins |= (uint32_t)b << (2 * k);
    }
    e.lens = del_len | (uint32_t)ins_len << 16;
    pair[0] = pair[1] = kHdrUndefined;
    if (edited) edited[0] = 0;
    uint32_t info = 0, block = 0;
    if (!hdr_pair(s, s.pam_accept, ch, cl, 0u, e0, e, [&](uint32_t r) -> uint32_t { return allowed ? allowed[r] : kHdrAnyLetter; }, &info, &block))
        return VSC_OK;
    pair[0] = info;
    pair[1] = block;
    if (edited) {
        uint32_t o = 0;
        for (uint32_t j = 0; j < e0; ++j) edited[o++] = (char)std::toupper((unsigned char)context[j]);
        for (size_t k = 0; k < ins_len; ++k) edited[o++] = (char)std::toupper((unsigned char)ins[k]);
        for (uint32_t j = e0 + del_len; j < C; ++j) edited[o++] = (char)std::toupper((unsigned char)context[j]);
        edited[o] = 0;
        if (block != kHdrNoBlock) {
            const uint32_t r = block >> 16 & 0xFFu;
            edited[r < e0 ? r : r + (uint32_t)ins_len - del_len] = "ACGT"[block >> 8 & 3u];
        }
    }
    return VSC_OK;
}

int vsc_loci_hdr(vsc_ctx *ctx, const vsc_genome *genome, const vsc_locus *loci, uint64_t n, const vsc_hdr_shape *shape, const vsc_prime_edit *edits,
                 uint64_t n_e, const vsc_cds *cds, const char *code, uint32_t *rows, vsc_hdr_pair *pairs, uint64_t capacity, uint64_t *n_pairs,
                 uint32_t *coverage, vsc_hdr_stats *stats)
{
    return guarded(ctx, [&]() -> int {
    if (!ctx) return VSC_ERR_INVALID;
    const char *const fn = "vsc_loci_hdr";
    HdrShape s{};
    PrimeHostEdits h;
    HdrTables tables{};
    const int rc = hdr_check(ctx, genome, shape, edits, n_e, cds, code, s, h, tables, fn);
    if (rc != VSC_OK) return rc;
    if (n && !loci) return fail_in(ctx, VSC_ERR_INVALID, fn, "null argument");
    if (n > kHdrMaxCount) return fail_in(ctx, VSC_ERR_RANGE, fn, "more than 0xFFFFFFFE candidates");
    return hdr_run(ctx, genome, s, h, cds, tables, CandidateLoci{nullptr, loci, n}, rows, pairs, capacity, n_pairs, coverage, stats, fn);
    });
}

int vsc_guides_hdr(vsc_ctx *ctx, const vsc_genome *genome, vsc_guides *guides, const vsc_hdr_shape *shape, const vsc_prime_edit *edits, uint64_t n_e,
                   const vsc_cds *cds, const char *code, uint32_t *rows, vsc_hdr_pair *pairs, uint64_t capacity, uint64_t *n_pairs,
                   uint32_t *coverage, vsc_hdr_stats *stats)
{
    return hdr_guides(ctx, genome, guides, shape, edits, n_e, cds, code, true, rows, pairs, capacity, n_pairs, coverage, stats, "vsc_guides_hdr");
}

int vsc_pattern_guides_hdr(vsc_ctx *ctx, const vsc_genome *genome, vsc_pattern_guides *guides, const vsc_hdr_shape *shape,
                           const vsc_prime_edit *edits, uint64_t n_e, const vsc_cds *cds, const char *code, uint32_t *rows, vsc_hdr_pair *pairs,
                           uint64_t capacity, uint64_t *n_pairs, uint32_t *coverage, vsc_hdr_stats *stats)
{
    return hdr_guides(ctx, genome, guides, shape, edits, n_e, cds, code, false, rows, pairs, capacity, n_pairs, coverage, stats,
                      "vsc_pattern_guides_hdr");
}

int vsc_guides_filter_hdr(vsc_ctx *ctx, const vsc_genome *genome, vsc_guides *in, const vsc_hdr_shape *shape, const vsc_prime_edit *edits,
                          uint64_t n_e, const vsc_cds *cds, const char *code, uint32_t allow_open, vsc_guides **out)
{
    return hdr_filter(ctx, genome, in, shape, edits, n_e, cds, code, true, allow_open, out, "vsc_guides_filter_hdr");
}

int vsc_pattern_guides_filter_hdr(vsc_ctx *ctx, const vsc_genome *genome, vsc_pattern_guides *in, const vsc_hdr_shape *shape,
                                  const vsc_prime_edit *edits, uint64_t n_e, const vsc_cds *cds, const char *code, uint32_t allow_open,
                                  vsc_pattern_guides **out)
{
    return hdr_filter(ctx, genome, in, shape, edits, n_e, cds, code, false, allow_open, out, "vsc_pattern_guides_filter_hdr");
}

}  // extern "C"

// ---- guide RNA self-complementarity (the definition: vsc_fold.h, the kernels: vsc_fold.hip) -----------------------
namespace {

const char *const kFoldShapeRule =
    "site_len 16 .. 32, proto_len 12 .. 32 inside the site, stem 3 .. 8, gc_min 0 .. stem, min_loop 0 .. 16, the seed (each 0 .. 16) inside "
    "the spacer, flags bit 0 only, reserved fields 0";

bool fold_shape_in(const vsc_fold_shape *shape, FoldShape &s)
{
    s = FoldShape{shape->site_len, shape->proto_start, shape->proto_len, shape->stem,  shape->gc_min,
                  shape->min_loop, shape->seed_start,  shape->seed_len,  shape->flags};
    return !shape->reserved[0] && !shape->reserved[1] && !shape->reserved[2] && fold_shape_valid(s);
}

// the scaffold text of a call as letters 0 .. 3; false: longer than 128 or another letter
bool fold_scaffold_in(const char *scaffold, uint32_t m, std::vector<uint8_t> &letters)
{
    if (m > kFoldMaxScaffold || (m && !scaffold)) return false;
    letters.resize(m);
    for (uint32_t j = 0; j < m; ++j) {
        const uint32_t b = fold_letter(scaffold[j]);
        if (b > 3u) return false;
        letters[j] = (uint8_t)b;
    }
    return true;
}

// The shape, the genome and the scaffold of a fold call, checked on the host; win = the scaffold's windows for the shape's spacer.
int fold_check(vsc_ctx *ctx, const vsc_genome *genome, const vsc_fold_shape *shape, const char *scaffold, uint32_t m, FoldShape &s,
               std::vector<FoldWindow> &win, const char *who)
{
    ctx->err.clear();
    if (!genome || !shape) return fail_in(ctx, VSC_ERR_INVALID, who, "null argument");
    if (genome->ctx != ctx) return fail_in(ctx, VSC_ERR_INVALID, who, "genome belongs to another context");
    if (!fold_shape_in(shape, s)) return fail_in(ctx, VSC_ERR_INVALID, who, kFoldShapeRule);
    std::vector<uint8_t> letters;
    if (!fold_scaffold_in(scaffold, m, letters)) return fail_in(ctx, VSC_ERR_INVALID, who, "the scaffold: at most 128 letters of A C G T U");
    win.resize(fold_diagonals(s.proto_len, m));
    fold_scaffold_windows(letters.data(), m, s.proto_len, win.data());
    return VSC_OK;
}

// The windows of a call onto the device, enqueued on the context's stream: into eff_buf, whose efficiency model is forgotten.
// Every call uploads its own, so no call reads another's scaffold; `win` outlives the call's last synchronise.
int fold_upload(vsc_ctx *ctx, const std::vector<FoldWindow> &win, const FoldWindow **d_win, uint32_t *n_diag)
{
    *d_win = nullptr;
    *n_diag = (uint32_t)win.size();
    if (win.empty()) return VSC_OK;
    ctx->eff_serial = 0;
    VSC_HIP(ctx, ctx->eff_buf.ensure(win.size() * sizeof(FoldWindow)));
    VSC_HIP(ctx, hipMemcpyAsync(ctx->eff_buf.p, win.data(), win.size() * sizeof(FoldWindow), hipMemcpyHostToDevice, ctx->stream));
    *d_win = (const FoldWindow *)ctx->eff_buf.p;
    return VSC_OK;
}

const CandidateRule kFoldRowsRule{"the shape's site_len must be 23", ~0ull, ""};  // (the scoring itself refuses above 2^40)
const CandidateRule kFoldFilterRule{"the shape's site_len must be 23", 0xFFFFFFFFull * kFoldTile, "more candidates than 2^32 tiles hold"};

// The rows of the loci `at` into host memory: fold_rows_kernel, one copy back of the rows and one of the class counts.
int fold_rows_loci(vsc_ctx *ctx, const vsc_genome *genome, const FoldShape &shape, const std::vector<FoldWindow> &win, const CandidateLoci &at,
                   uint32_t *rows, vsc_fold_stats *stats, const char *who)
{
    const auto t0 = std::chrono::steady_clock::now();
    if (stats) *stats = vsc_fold_stats{};
    if (at.n == 0) {
        ctx->timing = vsc_timing{};
        return VSC_OK;
    }
    FoldArgs a{};
    a.g = eff_planes(genome);
    a.shape = shape;
    a.n = at.n;
    unsigned long long seen[kEffClasses] = {};
    float ms = 0;
    const int rc = score_rows(
        ctx, at, sizeof(uint2), rows, seen, kEffClasses, &ms, who, [&] { return fold_upload(ctx, win, &a.win, &a.n_diag); },
        [&](unsigned long long *d_stats, void *d_rows, const uint4 *d_loci) {
            a.stats = d_stats;
            a.out = (uint2 *)d_rows;
            a.loci = d_loci;
            return launch_fold_rows(a, ctx->n_cus, ctx->fold_groups_per_cu, ctx->stream);
        });
    if (rc != VSC_OK) return rc;
    if (stats) {
        class_counts(stats, seen);
        stats->kernel_ms = ms;
        stats->wall_ms = wall_ms_since(t0);
    }
    return VSC_OK;
}

// vsc_guides_fold / vsc_pattern_guides_fold: over the candidates where they lie, a host-only object from the host
template <class Guides>
int fold_rows_guides(vsc_ctx *ctx, const vsc_genome *genome, Guides *guides, const vsc_fold_shape *shape, const char *scaffold, uint32_t m,
                     bool need_23, uint32_t *rows, vsc_fold_stats *stats, const char *who)
{
    return guarded(ctx, [&]() -> int {
    FoldShape s{};
    std::vector<FoldWindow> win;
    CandidateLoci at{};
    const int rc = candidate_front(ctx, guides, need_23, kFoldRowsRule, who, at, &s.site_len,
                                   [&] { return fold_check(ctx, genome, shape, scaffold, m, s, win, who); }, no_refusal);
    if (rc != VSC_OK) return rc;
    return fold_rows_loci(ctx, genome, s, win, at, rows, stats, who);
    });
}

// vsc_guides_filter_fold / vsc_pattern_guides_filter_fold: the candidates within the limits
template <class Guides>
int fold_filter(vsc_ctx *ctx, const vsc_genome *genome, Guides *in, const vsc_fold_shape *shape, const char *scaffold, uint32_t m, bool need_23,
                const vsc_fold_limits *limits, Guides **out, const char *who)
{
    return guarded(ctx, [&]() -> int {
    FoldShape s{};
    std::vector<FoldWindow> win;
    FoldFilterArgs a{};
    const int rc = filter_front(
        ctx, in, out, need_23, kFoldFilterRule, who, &s.site_len, [&] { return fold_check(ctx, genome, shape, scaffold, m, s, win, who); },
        [&]() -> int {
            if (!limits) return fail_in(ctx, VSC_ERR_INVALID, who, "null argument");
            a.limits = FoldLimits{limits->max_starts, limits->max_self_longest, limits->max_scaf_longest, limits->max_seed_paired};
            return fold_limits_valid(a.limits) ? VSC_OK : fail_in(ctx, VSC_ERR_INVALID, who, "a limit is 0 .. 32 or VSC_FOLD_NO_LIMIT");
        });
    if (rc != VSC_OK) return rc;
    const int urc = fold_upload(ctx, win, &a.win, &a.n_diag);
    if (urc != VSC_OK) return urc;
    a.g = eff_planes(genome);
    a.shape = s;
    return filter_candidates(ctx, in, a, kFoldTile, out, who, [&](bool write) { return launch_fold_filter(a, write, ctx->stream); });
    });
}

}  // namespace

extern "C" {

int vsc_debug_fold_groups_per_cu(vsc_ctx *ctx, uint32_t groups)
{
    if (!ctx || groups > kFoldMaxGroupsPerCu) return VSC_ERR_INVALID;
    ctx->fold_groups_per_cu = groups;
    return VSC_OK;
}

int vsc_fold_text(const char *spacer, uint32_t n, const char *scaffold, uint32_t m, const vsc_fold_shape *shape, uint32_t *row)
{
    if (!spacer || !shape || !row) return VSC_ERR_INVALID;
    FoldShape s{};
    if (!fold_shape_in(shape, s) || n != s.proto_len) return VSC_ERR_INVALID;
    std::vector<uint8_t> letters;
    if (!fold_scaffold_in(scaffold, m, letters)) return VSC_ERR_INVALID;
    if (strnlen(spacer, n) != n) return VSC_ERR_INVALID;
    row[0] = row[1] = kFoldUndefined;
    uint32_t gh = 0, gl = 0;
    for (uint32_t j = 0; j < n; ++j) {
        const uint32_t b = fold_letter(spacer[j]);
        if (b > 3u) return VSC_OK;
        gh |= (b >> 1) << j;
        gl |= (b & 1u) << j;
    }
    std::vector<FoldWindow> win(fold_diagonals(n, m));
    fold_scaffold_windows(letters.data(), m, n, win.data());
    fold_row(gh, gl, FoldScaffold{win.data(), (uint32_t)win.size()}, s, &row[0], &row[1]);
    return VSC_OK;
}

int vsc_loci_fold(vsc_ctx *ctx, const vsc_genome *genome, const vsc_locus *loci, uint64_t n, const vsc_fold_shape *shape, const char *scaffold,
                  uint32_t m, uint32_t *rows, vsc_fold_stats *stats)
{
    return guarded(ctx, [&]() -> int {
    if (!ctx) return VSC_ERR_INVALID;
    const char *const fn = "vsc_loci_fold";
    FoldShape s{};
    std::vector<FoldWindow> win;
    const int rc = fold_check(ctx, genome, shape, scaffold, m, s, win, fn);
    if (rc != VSC_OK) return rc;
    if (n && !loci) return fail_in(ctx, VSC_ERR_INVALID, fn, "null argument");
    return fold_rows_loci(ctx, genome, s, win, CandidateLoci{nullptr, loci, n}, rows, stats, fn);
    });
}

int vsc_guides_fold(vsc_ctx *ctx, const vsc_genome *genome, vsc_guides *guides, const vsc_fold_shape *shape, const char *scaffold, uint32_t m,
                    uint32_t *rows, vsc_fold_stats *stats)
{
    return fold_rows_guides(ctx, genome, guides, shape, scaffold, m, true, rows, stats, "vsc_guides_fold");
}

int vsc_pattern_guides_fold(vsc_ctx *ctx, const vsc_genome *genome, vsc_pattern_guides *guides, const vsc_fold_shape *shape, const char *scaffold,
                            uint32_t m, uint32_t *rows, vsc_fold_stats *stats)
{
    return fold_rows_guides(ctx, genome, guides, shape, scaffold, m, false, rows, stats, "vsc_pattern_guides_fold");
}

int vsc_guides_filter_fold(vsc_ctx *ctx, const vsc_genome *genome, vsc_guides *in, const vsc_fold_shape *shape, const char *scaffold, uint32_t m,
                           const vsc_fold_limits *limits, vsc_guides **out)
{
    return fold_filter(ctx, genome, in, shape, scaffold, m, true, limits, out, "vsc_guides_filter_fold");
}

int vsc_pattern_guides_filter_fold(vsc_ctx *ctx, const vsc_genome *genome, vsc_pattern_guides *in, const vsc_fold_shape *shape,
                                   const char *scaffold, uint32_t m, const vsc_fold_limits *limits, vsc_pattern_guides **out)
{
    return fold_filter(ctx, genome, in, shape, scaffold, m, false, limits, out, "vsc_pattern_guides_filter_fold");
}

}  // extern "C"

// ---- restriction sites and IUPAC motifs (the definition: vsc_motif.h, the kernels: vsc_motif.hip) -----------------
namespace {

const char *const kMotifShapeRule =
    "site_len 16 .. 32, up and down 0 .. 16 with a context of at most 64, proto_len 12 .. 32 inside the site, cut_len 1 .. 16 inside the "
    "site, reserved fields 0";

bool motif_shape_in(const vsc_motif_shape *shape, MotifShape &s)
{
    s = MotifShape{shape->up, shape->site_len, shape->down, shape->proto_start, shape->proto_len, shape->cut_start, shape->cut_len};
    for (uint32_t r : shape->reserved)
        if (r) return false;
    return motif_shape_valid(s);
}

// a flank's text as letters 0 .. 3; false: longer than 16 or another letter
bool motif_flank_in(const char *text, uint32_t n, uint8_t *letters)
{
    if (n > kMotifMaxFlank || (n && !text)) return false;
    for (uint32_t j = 0; j < n; ++j) {
        const uint32_t b = motif_letter(text[j]);
        if (b > 3u) return false;
        letters[j] = (uint8_t)b;
    }
    return true;
}

// What a call makes of its shape, flanks and motifs on the host: the table as the kernels read it (pat: host), and its image
// for the device - the patterns, then 3 * 63 zeroed totals.
struct MotifCall {
    MotifShape s{};
    MotifTable tab{};
    std::vector<MotifPattern> pat;
};
constexpr size_t kMotifTotalsAt = (kMotifMaxPatterns * sizeof(MotifPattern) + 255) / 256 * 256;
constexpr size_t kMotifImage = kMotifTotalsAt + 3 * kMotifMaxMotifs * sizeof(uint64_t);

// nullptr: fine; else the words of the refusal
const char *motif_call_in(const vsc_motif_shape *shape, const char *left, uint32_t a, const char *right, uint32_t b, const vsc_motif *motifs,
                          uint32_t n_motifs, MotifCall &c)
{
    if (!shape) return "null argument";
    if (!motif_shape_in(shape, c.s)) return kMotifShapeRule;
    uint8_t lf[kMotifMaxFlank], rf[kMotifMaxFlank];
    if (!motif_flank_in(left, a, lf) || !motif_flank_in(right, b, rf)) return "a flank: at most 16 letters of A C G T U";
    if (n_motifs < 1u || n_motifs > kMotifMaxMotifs) return "1 .. 63 motifs";
    if (!motifs) return "null argument";
    uint64_t accept[kMotifMaxMotifs];
    uint32_t len[kMotifMaxMotifs], flags[kMotifMaxMotifs];
    for (uint32_t m = 0; m < n_motifs; ++m) {
        if (motifs[m].flags & ~kMotifBothStrands) return "a motif's flags: bit 0 only";
        if (motifs[m].len < kMotifMinLen || motifs[m].len > kMotifMaxLen) return "a motif has 2 .. 16 letters";
        if (!motif_accepts(motifs[m].text, motifs[m].len, &accept[m])) return "a motif: IUPAC letters, not every one N";
        len[m] = motifs[m].len;
        flags[m] = motifs[m].flags;
    }
    c.pat.resize(kMotifMaxPatterns);
    c.pat.resize(motif_layout(accept, len, flags, n_motifs, c.s, a, b, c.pat.data()));
    c.tab = MotifTable{c.pat.data(), (uint32_t)c.pat.size(), n_motifs, 0ull, 0ull, a, b};
    motif_flank_planes(lf, a, rf, b, c.s.proto_len, &c.tab.flank_h, &c.tab.flank_l);
    return nullptr;
}

// The shape, the genome, the flanks and the motifs of a call, checked on the host.
int motif_check(vsc_ctx *ctx, const vsc_genome *genome, const vsc_motif_shape *shape, const char *left, uint32_t a, const char *right, uint32_t b,
                const vsc_motif *motifs, uint32_t n_motifs, MotifCall &c, const char *who)
{
    ctx->err.clear();
    if (!genome || !shape) return fail_in(ctx, VSC_ERR_INVALID, who, "null argument");
    if (genome->ctx != ctx) return fail_in(ctx, VSC_ERR_INVALID, who, "genome belongs to another context");
    const char *why = motif_call_in(shape, left, a, right, b, motifs, n_motifs, c);
    return why ? fail_in(ctx, VSC_ERR_INVALID, who, why) : VSC_OK;
}

// The patterns of a call onto the device, enqueued on the context's stream: into eff_buf, whose efficiency model is forgotten,
// with the zeroed totals behind them.  Every call uploads its own, so no call reads another's motifs.  *d_tab = the table
// with the device's patterns.
int motif_upload(vsc_ctx *ctx, const MotifCall &c, MotifTable *d_tab, unsigned long long **d_totals)
{
    ctx->eff_serial = 0;
    VSC_HIP(ctx, ctx->eff_buf.ensure(kMotifImage));
    VSC_HIP(ctx, hipMemcpyAsync(ctx->eff_buf.p, c.pat.data(), c.pat.size() * sizeof(MotifPattern), hipMemcpyHostToDevice, ctx->stream));
    VSC_HIP(ctx, hipMemsetAsync((char *)ctx->eff_buf.p + kMotifTotalsAt, 0, kMotifImage - kMotifTotalsAt, ctx->stream));
    *d_tab = c.tab;
    d_tab->pat = (const MotifPattern *)ctx->eff_buf.p;
    if (d_totals) *d_totals = (unsigned long long *)((char *)ctx->eff_buf.p + kMotifTotalsAt);
    return VSC_OK;
}

const CandidateRule kMotifRowsRule{"the shape's site_len must be 23", ~0ull, ""};  // (the scoring itself refuses above 2^40)
const CandidateRule kMotifFilterRule{"the shape's site_len must be 23", 0xFFFFFFFFull * kMotifTile, "more candidates than 2^32 tiles hold"};

// The rows of the loci `at` into host memory: motif_rows_kernel, one copy back of the rows, one of the counts and - where asked
// for - one of the totals.
int motif_rows_loci(vsc_ctx *ctx, const vsc_genome *genome, const MotifCall &c, const CandidateLoci &at, uint64_t *rows, uint64_t *totals,
                    vsc_motif_stats *stats, const char *who)
{
    const auto t0 = std::chrono::steady_clock::now();
    if (at.n && !rows) return fail_in(ctx, VSC_ERR_INVALID, who, "null argument");
    if (stats) *stats = vsc_motif_stats{};
    if (totals) std::fill(totals, totals + 3 * (size_t)c.tab.n_motifs, (uint64_t)0);
    if (at.n == 0) {
        ctx->timing = vsc_timing{};
        return VSC_OK;
    }
    MotifArgs a{};
    a.g = eff_planes(genome);
    a.shape = c.s;
    a.n = at.n;
    unsigned long long seen[kMotifStats] = {};
    float ms = 0;
    const int rc = score_rows(
        ctx, at, sizeof(MotifRow), rows, seen, kMotifStats, &ms, who,
        [&] {
            unsigned long long *d_totals = nullptr;
            const int urc = motif_upload(ctx, c, &a.tab, &d_totals);
            a.totals = totals ? d_totals : nullptr;
            return urc;
        },
        [&](unsigned long long *d_stats, void *d_rows, const uint4 *d_loci) {
            a.stats = d_stats;
            a.out = (MotifRow *)d_rows;
            a.loci = d_loci;
            return launch_motif_rows(a, ctx->n_cus, ctx->motif_groups_per_cu, ctx->stream);
        });
    if (rc != VSC_OK) return rc;
    if (totals) {
        VSC_HIP(ctx, hipMemcpyAsync(totals, a.totals, 3 * (size_t)c.tab.n_motifs * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
        VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    if (stats) {
        class_counts(stats, seen);
        stats->any_construct = seen[kEffClasses];
        stats->any_cut = seen[kEffClasses + 1];
        stats->any_cut_only = seen[kEffClasses + 2];
        stats->kernel_ms = ms;
        stats->wall_ms = wall_ms_since(t0);
    }
    return VSC_OK;
}

// vsc_guides_motifs / vsc_pattern_guides_motifs: over the candidates where they lie, a host-only object from the host
template <class Guides>
int motif_rows_guides(vsc_ctx *ctx, const vsc_genome *genome, Guides *guides, const vsc_motif_shape *shape, const char *left, uint32_t fa,
                      const char *right, uint32_t fb, const vsc_motif *motifs, uint32_t n_motifs, bool need_23, uint64_t *rows, uint64_t *totals,
                      vsc_motif_stats *stats, const char *who)
{
    return guarded(ctx, [&]() -> int {
    MotifCall c;
    CandidateLoci at{};
    const int rc = candidate_front(ctx, guides, need_23, kMotifRowsRule, who, at, &c.s.site_len,
                                   [&] { return motif_check(ctx, genome, shape, left, fa, right, fb, motifs, n_motifs, c, who); }, no_refusal);
    if (rc != VSC_OK) return rc;
    return motif_rows_loci(ctx, genome, c, at, rows, totals, stats, who);
    });
}

// vsc_guides_filter_motifs / vsc_pattern_guides_filter_motifs: the candidates the limits keep
template <class Guides>
int motif_filter(vsc_ctx *ctx, const vsc_genome *genome, Guides *in, const vsc_motif_shape *shape, const char *left, uint32_t fa, const char *right,
                 uint32_t fb, const vsc_motif *motifs, uint32_t n_motifs, bool need_23, const vsc_motif_limits *limits, Guides **out,
                 const char *who)
{
    return guarded(ctx, [&]() -> int {
    MotifCall c;
    MotifFilterArgs a{};
    const int rc = filter_front(
        ctx, in, out, need_23, kMotifFilterRule, who, &c.s.site_len,
        [&] { return motif_check(ctx, genome, shape, left, fa, right, fb, motifs, n_motifs, c, who); },
        [&]() -> int {
            if (!limits) return fail_in(ctx, VSC_ERR_INVALID, who, "null argument");
            a.limits = MotifLimits{limits->forbid_construct, limits->forbid_context, limits->require_cut, limits->flags};
            return !limits->reserved && motif_limits_valid(a.limits, n_motifs)
                       ? VSC_OK
                       : fail_in(ctx, VSC_ERR_INVALID, who, "the limits: bits below the number of motifs, flags bit 0 only, reserved 0");
        });
    if (rc != VSC_OK) return rc;
    const int urc = motif_upload(ctx, c, &a.tab, nullptr);
    if (urc != VSC_OK) return urc;
    a.g = eff_planes(genome);
    a.shape = c.s;
    return filter_candidates(ctx, in, a, kMotifTile, out, who, [&](bool write) { return launch_motif_filter(a, write, ctx->stream); });
    });
}

}  // namespace

extern "C" {

int vsc_debug_motif_groups_per_cu(vsc_ctx *ctx, uint32_t groups)
{
    if (!ctx || groups > kMotifMaxGroupsPerCu) return VSC_ERR_INVALID;
    ctx->motif_groups_per_cu = groups;
    return VSC_OK;
}

int vsc_motif_text(const char *context, uint32_t c_len, const char *left, uint32_t a, const char *right, uint32_t b, const vsc_motif *motifs,
                   uint32_t n_motifs, const vsc_motif_shape *shape, uint64_t *row)
{
    if (!context || !row) return VSC_ERR_INVALID;
    MotifCall c;
    if (motif_call_in(shape, left, a, right, b, motifs, n_motifs, c)) return VSC_ERR_INVALID;
    if (c_len != motif_context_len(c.s) || strnlen(context, c_len) != c_len) return VSC_ERR_INVALID;
    row[0] = row[1] = row[2] = kMotifUndefined;
    uint64_t ch = 0, cl = 0;
    for (uint32_t j = 0; j < c_len; ++j) {
        const uint32_t l = motif_letter(context[j]);
        if (l > 3u) return VSC_OK;
        ch |= (uint64_t)(l >> 1) << j;
        cl |= (uint64_t)(l & 1u) << j;
    }
    const MotifRow r = motif_row(ch, cl, c.s, c.tab);
    row[0] = r.construct;
    row[1] = r.cut;
    row[2] = r.elsewhere;
    return VSC_OK;
}

int vsc_loci_motifs(vsc_ctx *ctx, const vsc_genome *genome, const vsc_locus *loci, uint64_t n, const vsc_motif_shape *shape, const char *left,
                    uint32_t a, const char *right, uint32_t b, const vsc_motif *motifs, uint32_t n_motifs, uint64_t *rows, uint64_t *totals,
                    vsc_motif_stats *stats)
{
    return guarded(ctx, [&]() -> int {
    if (!ctx) return VSC_ERR_INVALID;
    const char *const fn = "vsc_loci_motifs";
    MotifCall c;
    const int rc = motif_check(ctx, genome, shape, left, a, right, b, motifs, n_motifs, c, fn);
    if (rc != VSC_OK) return rc;
    if (n && !loci) return fail_in(ctx, VSC_ERR_INVALID, fn, "null argument");
    return motif_rows_loci(ctx, genome, c, CandidateLoci{nullptr, loci, n}, rows, totals, stats, fn);
    });
}

int vsc_guides_motifs(vsc_ctx *ctx, const vsc_genome *genome, vsc_guides *guides, const vsc_motif_shape *shape, const char *left, uint32_t a,
                      const char *right, uint32_t b, const vsc_motif *motifs, uint32_t n_motifs, uint64_t *rows, uint64_t *totals,
                      vsc_motif_stats *stats)
{
    return motif_rows_guides(ctx, genome, guides, shape, left, a, right, b, motifs, n_motifs, true, rows, totals, stats, "vsc_guides_motifs");
}

int vsc_pattern_guides_motifs(vsc_ctx *ctx, const vsc_genome *genome, vsc_pattern_guides *guides, const vsc_motif_shape *shape, const char *left,
                              uint32_t a, const char *right, uint32_t b, const vsc_motif *motifs, uint32_t n_motifs, uint64_t *rows,
                              uint64_t *totals, vsc_motif_stats *stats)
{
    return motif_rows_guides(ctx, genome, guides, shape, left, a, right, b, motifs, n_motifs, false, rows, totals, stats,
                             "vsc_pattern_guides_motifs");
}

int vsc_guides_filter_motifs(vsc_ctx *ctx, const vsc_genome *genome, vsc_guides *in, const vsc_motif_shape *shape, const char *left, uint32_t a,
                             const char *right, uint32_t b, const vsc_motif *motifs, uint32_t n_motifs, const vsc_motif_limits *limits,
                             vsc_guides **out)
{
    return motif_filter(ctx, genome, in, shape, left, a, right, b, motifs, n_motifs, true, limits, out, "vsc_guides_filter_motifs");
}

int vsc_pattern_guides_filter_motifs(vsc_ctx *ctx, const vsc_genome *genome, vsc_pattern_guides *in, const vsc_motif_shape *shape,
                                     const char *left, uint32_t a, const char *right, uint32_t b, const vsc_motif *motifs, uint32_t n_motifs,
                                     const vsc_motif_limits *limits, vsc_pattern_guides **out)
{
    return motif_filter(ctx, genome, in, shape, left, a, right, b, motifs, n_motifs, false, limits, out, "vsc_pattern_guides_filter_motifs");
}

}  // extern "C"

// ---- paired-nickase screen -------------------------------------------------------------------------------------
namespace {

int pair_params_check(const vsc_pair_params *p)
{
    if (!p || p->reserved[0] || p->reserved[1] || !pair_params_ok(p->delta_min, p->delta_max)) return VSC_ERR_INVALID;
    return VSC_OK;
}

// The pairs of a candidate array on ctx's device (vsc_guides_pairs): count per '-' candidate, exclusive scan, one 8-byte
// read-back (the total, checked against the capacity), write pass, one copy to the host.
int guides_pairs_device(vsc_guides *g, const vsc_pair_params *p, vsc_guide_pair *pairs, uint64_t capacity, uint64_t *n_pairs)
{
    vsc_ctx *ctx = g->ctx;
    ctx->err.clear();
    if (g->n > 0xFFFFFFFFull - 2048) return fail(ctx, VSC_ERR_RANGE, "vsc_guides_pairs: more candidates than the 32-bit item space holds");
    VSC_HIP(ctx, hipSetDevice(ctx->device));
    const uint32_t n = (uint32_t)g->n;
    const size_t count_bytes = ((size_t)n * sizeof(uint32_t) + 255) / 256 * 256;
    VSC_HIP(ctx, ctx->pairs_items.ensure(count_bytes + ((size_t)n + 1) * sizeof(unsigned long long)));
    PairLociArgs a{};
    a.loci = (const uint4 *)((const char *)g->storage.p + g->loci_at);
    a.n = n;
    a.delta_min = p->delta_min;
    a.delta_max = p->delta_max;
    a.item_count = (uint32_t *)ctx->pairs_items.p;
    unsigned long long *d_off = (unsigned long long *)((char *)ctx->pairs_items.p + count_bytes);
    a.item_off = d_off;
    VSC_HIP(ctx, launch_pair_loci(a, false, ctx->n_cus, ctx->stream));
    VSC_HIP(ctx, launch_enum_scan(a.item_count, n, d_off, ctx->stream));
    unsigned long long total = 0;
    VSC_HIP(ctx, hipMemcpyAsync(&total, d_off + n, sizeof total, hipMemcpyDeviceToHost, ctx->stream));
    VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *n_pairs = total;
    if (!pairs || total == 0) return VSC_OK;
    if (total > capacity) return fail(ctx, VSC_ERR_RANGE, "vsc_guides_pairs: more pairs than the capacity");
    VSC_HIP(ctx, ctx->pairs_out.ensure((size_t)total * sizeof(vsc_guide_pair)));
    a.pairs = (uint2 *)ctx->pairs_out.p;
    VSC_HIP(ctx, launch_pair_loci(a, true, ctx->n_cus, ctx->stream));
    VSC_HIP(ctx, hipMemcpyAsync(pairs, a.pairs, (size_t)total * sizeof(vsc_guide_pair), hipMemcpyDeviceToHost, ctx->stream));
    VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return VSC_OK;
}

// The join of vsc_hits_pairs; the arguments are checked, rows[] zeroed and *total = 0 already.
int hits_pairs_device(vsc_hits *hits, uint32_t n_guides, const vsc_guide_pair *pairs, uint32_t n_pairs, const vsc_pair_params *p,
                      const vsc_locus *exclude, vsc_pair_summary *rows, vsc_pair_site *sites, uint64_t capacity, uint64_t *total)
{
    vsc_ctx *ctx = hits->ctx;
    const char *const who = "vsc_hits_pairs";
    HostTimer lap;
    VSC_HIP(ctx, hipSetDevice(ctx->device));
    const uint32_t n = (uint32_t)hits->n;
    vsc_hit last{};  // the records ascend by guide: the last one holds the largest
    VSC_HIP(ctx, hipMemcpyAsync(&last, hits->d_records + (n - 1), sizeof last, hipMemcpyDeviceToHost, ctx->stream));
    VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (last.guide >= n_guides) return fail_in(ctx, VSC_ERR_INVALID, who, "a record's guide is not below n_guides");

    // tables, 256-byte aligned parts: [segment starts][pairs][item offsets of the pairs][excluded loci][rows]
    auto round = [](size_t b) { return (b + 255) / 256 * 256; };
    const size_t n_seg = 2 * (size_t)n_guides + 1;
    const size_t pairs_at = round(n_seg * sizeof(uint32_t));
    const size_t off_at = pairs_at + round((size_t)n_pairs * sizeof(vsc_guide_pair));
    const size_t excl_at = off_at + round(((size_t)n_pairs + 1) * sizeof(unsigned long long));
    const size_t rows_at = excl_at + round(exclude ? (size_t)n_guides * sizeof(vsc_locus) : 0);
    const size_t row_bytes = (size_t)n_pairs * sizeof(vsc_pair_summary);
    VSC_HIP(ctx, ctx->pairs_tabs.ensure(rows_at + row_bytes));
    char *base = (char *)ctx->pairs_tabs.p;

    PairSegArgs sa{};
    sa.records = (const uint4 *)hits->d_records;
    sa.n = n;
    sa.n_guides = n_guides;
    sa.seg = (uint32_t *)base;
    VSC_HIP(ctx, launch_pair_segments(sa, ctx->stream));
    std::vector<uint32_t> seg(n_seg);
    VSC_HIP(ctx, hipMemcpyAsync(seg.data(), sa.seg, n_seg * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    lap.lap("pairs: segment table");
    // the work items: (pair j, record of guide a_j), flattened by the prefix sum of the record counts
    std::vector<unsigned long long> pair_off((size_t)n_pairs + 1);
    unsigned long long n_items = 0;
    for (uint32_t j = 0; j < n_pairs; ++j) {
        pair_off[j] = n_items;
        n_items += seg[2 * (size_t)pairs[j].a + 2] - seg[2 * (size_t)pairs[j].a];
    }
    pair_off[n_pairs] = n_items;
    if (n_items == 0) return VSC_OK;
    if (sites && n_items > 0xFFFFFFFFull - 2048)
        return fail_in(ctx, VSC_ERR_RANGE, who, "more (pair, record) work items than the site pass can number (fewer pairs per call)");

    PairJoinArgs a{};
    a.records = sa.records;
    a.seg = sa.seg;
    a.pairs = (const uint2 *)(base + pairs_at);
    a.pair_off = (const unsigned long long *)(base + off_at);
    a.n_pairs = n_pairs;
    a.n_items = n_items;
    a.delta_min = p->delta_min;
    a.delta_max = p->delta_max;
    a.rows = (unsigned long long *)(base + rows_at);
    VSC_HIP(ctx, hipMemcpyAsync(base + pairs_at, pairs, (size_t)n_pairs * sizeof(vsc_guide_pair), hipMemcpyHostToDevice, ctx->stream));
    VSC_HIP(ctx, hipMemcpyAsync(base + off_at, pair_off.data(), pair_off.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, ctx->stream));
    if (exclude) {
        VSC_HIP(ctx, hipMemcpyAsync(base + excl_at, exclude, (size_t)n_guides * sizeof(vsc_locus), hipMemcpyHostToDevice, ctx->stream));
        a.exclude = (const uint4 *)(base + excl_at);
    }
    VSC_HIP(ctx, hipMemsetAsync(a.rows, 0, row_bytes, ctx->stream));
    unsigned long long *d_off = nullptr;
    if (sites) {
        const size_t count_bytes = round((size_t)n_items * sizeof(uint32_t));
        VSC_HIP(ctx, ctx->pairs_items.ensure(count_bytes + ((size_t)n_items + 1) * sizeof(unsigned long long)));
        a.item_count = (uint32_t *)ctx->pairs_items.p;
        d_off = (unsigned long long *)((char *)ctx->pairs_items.p + count_bytes);
        a.item_off = d_off;
    }
    VSC_HIP(ctx, launch_pair_join(a, false, ctx->n_cus, ctx->stream));
    if (sites) VSC_HIP(ctx, launch_enum_scan(a.item_count, (uint32_t)n_items, d_off, ctx->stream));
    VSC_HIP(ctx, hipMemcpyAsync(rows, a.rows, row_bytes, hipMemcpyDeviceToHost, ctx->stream));
    VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (also: pair_off above is this call's vector)
    lap.lap("pairs: count pass, rows");
    for (uint32_t j = 0; j < n_pairs; ++j) *total += rows[j].sites;
    if (!sites || *total == 0) return VSC_OK;
    if (*total > capacity) return fail_in(ctx, VSC_ERR_RANGE, who, "more paired sites than the capacity (the rows are valid)");
    VSC_HIP(ctx, ctx->pairs_out.ensure((size_t)*total * sizeof(vsc_pair_site)));
    a.sites = (uint4 *)ctx->pairs_out.p;
    VSC_HIP(ctx, launch_pair_join(a, true, ctx->n_cus, ctx->stream));
    VSC_HIP(ctx, hipMemcpyAsync(sites, a.sites, (size_t)*total * sizeof(vsc_pair_site), hipMemcpyDeviceToHost, ctx->stream));
    VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    lap.lap("pairs: write pass, sites");
    return VSC_OK;
}

}  // namespace

extern "C" {

int vsc_loci_pairs(const vsc_locus *loci, uint64_t n, const vsc_pair_params *p, vsc_guide_pair *pairs, uint64_t capacity,
                   uint64_t *n_pairs)
{
    if (!n_pairs) return VSC_ERR_INVALID;
    *n_pairs = 0;
    if (pair_params_check(p) != VSC_OK || (n && !loci)) return VSC_ERR_INVALID;
    if (n > 0xFFFFFFFFull) return VSC_ERR_RANGE;  // (a and b are 32-bit indices)
    return guarded(nullptr, [&]() -> int {
    // the entries that take part, by (contig, pos, strand, index): the order vsc_guides_enumerate gives, the index in word 3
    std::vector<uint4> s;
    s.reserve(n);
    for (uint64_t i = 0; i < n; ++i)
        if (loci[i].contig != kPairNoContig && loci[i].strand <= 1) s.push_back(make_uint4(loci[i].contig, loci[i].pos, loci[i].strand, (uint32_t)i));
    std::sort(s.begin(), s.end(), [](const uint4 &x, const uint4 &y) {
        return x.x != y.x ? x.x < y.x : x.y != y.y ? x.y < y.y : x.z != y.z ? x.z < y.z : x.w < y.w;
    });
    const uint32_t m = (uint32_t)s.size();
    // pair_loci_kernel's walk per '-' entry: first to count, then - when the pairs fit - to write
    for (int pass = 0; pass < 2; ++pass) {
        uint64_t at = 0;
        for (uint32_t i = 0; i < m; ++i) {
            uint32_t lo, hi;
            if (s[i].z != 1u || !pair_range(s[i].y, 1u, p->delta_min, p->delta_max, &lo, &hi)) continue;
            for (uint32_t k = pair_lower_bound<false>(s.data(), 0u, m, s[i].x, lo); k < m && !pair_after<false>(s[k], s[i].x, hi); ++k) {
                if (s[k].z != 0u) continue;
                if (pass) pairs[at] = vsc_guide_pair{s[i].w, s[k].w};
                ++at;
            }
        }
        if (pass == 0) {
            *n_pairs = at;
            if (!pairs || at == 0) return VSC_OK;
            if (at > capacity) return VSC_ERR_RANGE;
        }
    }
    std::sort(pairs, pairs + *n_pairs, [](const vsc_guide_pair &x, const vsc_guide_pair &y) { return x.a != y.a ? x.a < y.a : x.b < y.b; });
    return VSC_OK;
    });
}

int vsc_guides_pairs(vsc_guides *guides, const vsc_pair_params *p, vsc_guide_pair *pairs, uint64_t capacity, uint64_t *n_pairs)
{
    if (!guides || !n_pairs) return VSC_ERR_INVALID;
    *n_pairs = 0;
    if (pair_params_check(p) != VSC_OK) {
        if (guides->ctx) (void)fail(guides->ctx, VSC_ERR_INVALID, "vsc_guides_pairs: delta_min <= delta_max within +-2^30 and zeroed reserved fields are needed");
        return VSC_ERR_INVALID;
    }
    if (guides->n == 0) return VSC_OK;
    if (!guides->ctx)  // vsc_multi_guides_enumerate's host-only object: the same pairs by the host's walk
        return vsc_loci_pairs(guides->loci.data(), guides->n, p, pairs, capacity, n_pairs);
    return guarded(guides->ctx, [&]() -> int { return guides_pairs_device(guides, p, pairs, capacity, n_pairs); });
}

int vsc_hits_pairs(vsc_hits *hits, uint32_t n_guides, const vsc_guide_pair *pairs, uint32_t n_pairs, const vsc_pair_params *p,
                   const vsc_locus *exclude, vsc_pair_summary *rows, vsc_pair_site *sites, uint64_t capacity, uint64_t *n_sites)
{
    if (n_sites) *n_sites = 0;
    if (!hits) return VSC_ERR_INVALID;
    vsc_ctx *ctx = hits->ctx;
    const char *const who = "vsc_hits_pairs";
    return guarded(ctx, [&]() -> int {
    ctx->err.clear();
    if (!p || (n_pairs && (!pairs || !rows))) return fail_in(ctx, VSC_ERR_INVALID, who, "null argument");
    if (pair_params_check(p) != VSC_OK)
        return fail_in(ctx, VSC_ERR_INVALID, who, "delta_min <= delta_max within +-2^30 and zeroed reserved fields are needed");
    if (n_guides > 0x7FFFFFFFu) return fail_in(ctx, VSC_ERR_INVALID, who, "n_guides must be below 2^31");
    for (uint32_t j = 0; j < n_pairs; ++j)
        if (pairs[j].a == pairs[j].b || pairs[j].a >= n_guides || pairs[j].b >= n_guides)
            return fail_in(ctx, VSC_ERR_INVALID, who, "a pair needs two different guides below n_guides");
    for (uint32_t i = 0; exclude && i < n_guides; ++i)
        if (exclude[i].contig != UINT32_MAX && exclude[i].strand > 1) return fail_in(ctx, VSC_ERR_INVALID, who, "excluded locus with a strand above 1");
    if (hits->n > 0xFFFFFFFFull) return fail_in(ctx, VSC_ERR_RANGE, who, "more than 2^32 - 1 records");
    if (n_pairs) std::memset(rows, 0, (size_t)n_pairs * sizeof(vsc_pair_summary));
    if (n_pairs == 0 || hits->n == 0) return VSC_OK;
    uint64_t total = 0;
    const int rc = hits_pairs_device(hits, n_guides, pairs, n_pairs, p, exclude, rows, sites, capacity, &total);
    if (n_sites) *n_sites = total;
    return rc;
    });
}

double vsc_mit_specificity(uint64_t mit_sum)
{
    // CRISPOR's mitSpecScore before its round(): 100 / (100 + Σ mitOfftargetScore) * 100, the sum in units of 2^-24
    return (100.0 / (100.0 + (double)mit_sum * 0x1p-24)) * 100.0;
}

int vsc_search_stream(vsc_ctx *ctx, const vsc_genome *genome, const uint64_t *guides, uint32_t n_guides,
                      const vsc_search_params *params, uint32_t batch_reads, vsc_batch_fn on_batch, void *user)
{
    return search_stream(ctx, genome, guides, n_guides, params, batch_reads, false, "vsc_search_stream", on_batch != nullptr,
                          [&](vsc_hits *hits, uint32_t first, uint32_t count, vsc_timing &t) {
                              const int prc = on_batch(user, hits, first, count);
                              t.score_ms += ctx->timing.score_ms;  // what the callback's scoring calls measured
                              return prc;
                          });
}

int vsc_search_stream_rows(vsc_ctx *ctx, const vsc_genome *genome, const uint64_t *guides, uint32_t n_guides,
                           const vsc_search_params *params, uint32_t batch_reads, vsc_rows_batch_fn on_batch, void *user)
{
    return search_stream(ctx, genome, guides, n_guides, params, batch_reads, true, "vsc_search_stream_rows", on_batch != nullptr,
                          [&](vsc_hits *hits, uint32_t first, uint32_t count, vsc_timing &t) {
                              // the seed search wrote the rows with the records; the streaming scan's hits (small searches on a
                              // genome without an index) are scored the usual way
                              if (hits->n && t.algorithm != VSC_ALGO_SEED) {
                                  int prc = vsc_score_hits_packed(ctx, genome, hits, guides, n_guides, 0, hits->n, nullptr, nullptr, nullptr);
                                  if (prc == VSC_OK && ctx->score_feat.cap < hits->n * VSC_PACKED_FEATURE_BYTES)
                                      prc = fail(ctx, VSC_ERR_NOMEM, "vsc_search_stream_rows: the batch's rows do not fit the device at once (smaller batches)");
                                  t.score_ms += ctx->timing.score_ms;
                                  if (prc != VSC_OK) return prc;
                              }
                              return on_batch(user, hits, first, count, hits->n ? ctx->score_feat.p : nullptr);
                          });
}

int vsc_hits_variants(vsc_hits *hits, const vsc_genome *win_genome, const vsc_variant_map *map, const vsc_locus *exclude,
                      uint32_t n_guides, vsc_variant_label *labels)
{
    if (!hits || !win_genome || !map || (hits->n && !labels)) return VSC_ERR_INVALID;
    vsc_ctx *ctx = hits->ctx;
    return guarded(ctx, [&]() -> int {
    ctx->err.clear();
    VariantArgs a{};
    int rc = resident_variant_map(ctx, win_genome, map, exclude, n_guides, "vsc_hits_variants", a);
    if (rc != VSC_OK || hits->n == 0) return rc;
    if ((rc = variant_state(ctx, 0, false, a)) != VSC_OK) return rc;
    a.records = (const uint4 *)hits->d_records;
    a.n = hits->n;
    VSC_HIP(ctx, ctx->var_labels.ensure(hits->n * sizeof(vsc_variant_label)));
    a.labels = (uint4 *)ctx->var_labels.p;
    VSC_HIP(ctx, launch_variant_merge(a, ctx->stream));
    VSC_HIP(ctx, hipMemcpyAsync(labels, a.labels, hits->n * sizeof(vsc_variant_label), hipMemcpyDeviceToHost, ctx->stream));
    VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return variant_error(ctx, a, "vsc_hits_variants");
    });
}

int vsc_search_summary_variants(vsc_ctx *ctx, const vsc_genome *win_genome, const vsc_variant_map *map, const uint64_t *guides,
                                uint32_t n_guides, const vsc_search_params *params, const vsc_locus *exclude, uint32_t batch_reads,
                                vsc_guide_summary *out_all, vsc_guide_summary *out_var, uint64_t *duplicates)
{
    if (!ctx) return VSC_ERR_INVALID;
    const char *const who = "vsc_search_summary_variants";
    if (!win_genome || !map || !params || (n_guides && (!guides || !out_all))) return fail_in(ctx, VSC_ERR_INVALID, who, "null argument");
    VariantArgs a{};
    const int rc = guarded(ctx, [&]() -> int {
        ctx->err.clear();
        const int mrc = resident_variant_map(ctx, win_genome, map, exclude, n_guides, who, a);
        return mrc != VSC_OK ? mrc : variant_state(ctx, n_guides, true, a);
    });
    if (rc != VSC_OK) return rc;
    // every batch's sorted records are summarised where they lie; the batch is freed when this returns
    const int src = search_stream(ctx, win_genome, guides, n_guides, params, batch_reads, false, who, true,
                                  [&](vsc_hits *hits, uint32_t, uint32_t, vsc_timing &t) -> int {
                                      if (hits->n == 0) return VSC_OK;
                                      a.records = (const uint4 *)hits->d_records;
                                      a.n = hits->n;
                                      VSC_HIP(ctx, hipEventRecord(ctx->ev[kEvStageStart], ctx->stream));
                                      VSC_HIP(ctx, launch_variant_merge(a, ctx->stream));
                                      VSC_HIP(ctx, hipEventRecord(ctx->ev[kEvStageEnd], ctx->stream));
                                      VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));
                                      float ms = 0;
                                      VSC_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev[kEvStageStart], ctx->ev[kEvStageEnd]));
                                      t.finalize_ms += ms;
                                      t.total_ms += ms;
                                      return VSC_OK;
                                  });
    if (src != VSC_OK || n_guides == 0) return src;
    return guarded(ctx, [&]() -> int {
        const size_t row_bytes = (size_t)n_guides * sizeof(vsc_guide_summary);
        VSC_HIP(ctx, hipMemcpyAsync(out_all, a.rows_all, row_bytes, hipMemcpyDeviceToHost, ctx->stream));
        if (out_var) VSC_HIP(ctx, hipMemcpyAsync(out_var, a.rows_var, row_bytes, hipMemcpyDeviceToHost, ctx->stream));
        if (duplicates) VSC_HIP(ctx, hipMemcpyAsync(duplicates, a.dups, (size_t)n_guides * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
        VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return variant_error(ctx, a, who);
    });
}

uint64_t vsc_hits_count(const vsc_hits *hits) { return hits ? hits->n : 0; }

const void *vsc_hits_data_dev(const vsc_hits *hits) { return hits ? hits->d_records : nullptr; }

int vsc_hits_data(vsc_hits *hits, const vsc_hit **out)
{
    return guarded(nullptr, [&]() -> int {
    if (!hits || !out) return VSC_ERR_INVALID;
    *out = nullptr;
    if (!hits->host_valid) {
        vsc_ctx *ctx = hits->ctx;
        try {
            hits->host.resize(hits->n);
        } catch (...) {
            return fail(ctx, VSC_ERR_NOMEM, "vsc_hits_data: out of host memory");
        }
        if (hits->n) {
            VSC_HIP(ctx, hipSetDevice(ctx->device));
            VSC_HIP(ctx, hipMemcpyAsync(hits->host.data(), hits->d_records, hits->n * sizeof(vsc_hit),
                                        hipMemcpyDeviceToHost, ctx->stream));
            VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        }
        hits->host_valid = true;
    }
    *out = hits->host.data();
    return VSC_OK;
    });
}

int vsc_hits_copy(vsc_hits *hits, void *dst, int dst_is_device)
{
    return guarded(nullptr, [&]() -> int {
    if (!hits || (!dst && hits->n)) return VSC_ERR_INVALID;
    if (hits->n == 0) return VSC_OK;
    vsc_ctx *ctx = hits->ctx;
    VSC_HIP(ctx, hipSetDevice(ctx->device));
    VSC_HIP(ctx, hipMemcpyAsync(dst, hits->d_records, hits->n * sizeof(vsc_hit),
                                dst_is_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
    VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return VSC_OK;
    });
}

int vsc_hits_merge(vsc_ctx *ctx, const void *records, int records_on_device, const uint64_t *shard_counts,
                   uint32_t n_shards, uint32_t n_guides, vsc_hits **out)
{
    return guarded(ctx, [&]() -> int {
    if (!ctx || !out) return VSC_ERR_INVALID;
    *out = nullptr;
    ctx->err.clear();
    if (!shard_counts || n_shards == 0) return fail(ctx, VSC_ERR_INVALID, "vsc_hits_merge: null argument");
    std::vector<uint64_t> off(n_shards + 1, 0);
    for (uint32_t s = 0; s < n_shards; ++s) off[s + 1] = off[s] + shard_counts[s];
    const uint64_t n = off[n_shards];
    if (n && !records) return fail(ctx, VSC_ERR_INVALID, "vsc_hits_merge: null argument");
    if (n_guides >= (1u << 30)) return fail(ctx, VSC_ERR_RANGE, "vsc_hits_merge: too many reads");
    VSC_HIP(ctx, hipSetDevice(ctx->device));
    vsc_hits *hits = new (std::nothrow) vsc_hits();
    if (!hits) return fail(ctx, VSC_ERR_NOMEM, "vsc_hits_merge: out of host memory");
    hits->ctx = ctx;
    hits->n = n;
    if (n == 0) {
        hits->host_valid = true;
        *out = hits;
        return VSC_OK;
    }
    const uint32_t K = 2 * std::max<uint32_t>(n_guides, 1);  // keys guide << 1 | strand
    const uint64_t nb = (uint64_t)n_shards * (K + 1);
    hipError_t e = hipSuccess;
    auto step = [&](hipError_t r) {
        if (e == hipSuccess) e = r;
    };
    // small work arrays reuse the search scratch buffers
    step(ctx->keys_b.ensure((nb + n_shards + 1) * sizeof(uint64_t)));
    step(ctx->vals_a.ensure(((uint64_t)K + 1) * sizeof(uint64_t)));
    step(take_records(ctx, hits, n));
    const vsc_hit *records_dev = (const vsc_hit *)records;
    if (!records_on_device) {
        step(ctx->score_feat.ensure(n * sizeof(vsc_hit)));  // staging buffer for host input
        if (e == hipSuccess)
            step(hipMemcpyAsync(ctx->score_feat.p, records, n * sizeof(vsc_hit), hipMemcpyHostToDevice, ctx->stream));
        records_dev = (const vsc_hit *)ctx->score_feat.p;
    }
    uint64_t *bound = (uint64_t *)ctx->keys_b.p;
    uint64_t *shard_off_dev = bound + nb;
    if (e == hipSuccess)
        step(hipMemcpyAsync(shard_off_dev, off.data(), off.size() * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
    step(hipEventRecord(ctx->ev[kEvStageStart], ctx->stream));
    if (e == hipSuccess)
        step(launch_merge(records_dev, shard_off_dev, n_shards, K, bound, (uint64_t *)ctx->vals_a.p, hits->d_records, ctx->stream));
    step(hipEventRecord(ctx->ev[kEvStageEnd], ctx->stream));
    step(hipStreamSynchronize(ctx->stream));
    if (e != hipSuccess) {
        vsc_hits_free(hits);
        return fail(ctx, e == hipErrorOutOfMemory ? VSC_ERR_NOMEM : VSC_ERR_DEVICE, "vsc_hits_merge", e);
    }
    *out = hits;
    return VSC_OK;
    });
}

int vsc_hits_pack_exchange(vsc_ctx *ctx, const vsc_genome *genome, const vsc_hits *hits, uint32_t n_guides, void *records,
                           int records_on_device, uint32_t *key_counts)
{
    return guarded(ctx, [&]() -> int {
    if (!ctx) return VSC_ERR_INVALID;
    ctx->err.clear();
    if (!genome || !hits || genome->ctx != ctx || hits->ctx != ctx || (n_guides && !key_counts) || (hits->n && !records))
        return fail(ctx, VSC_ERR_INVALID, "vsc_hits_pack_exchange: null argument or object of another context");
    if (n_guides >= (1u << 30)) return fail(ctx, VSC_ERR_RANGE, "vsc_hits_pack_exchange: too many reads");
    const uint32_t K = 2 * n_guides;
    const uint64_t n = hits->n;
    if (n == 0) {
        std::fill(key_counts, key_counts + K, 0u);
        return VSC_OK;
    }
    VSC_HIP(ctx, hipSetDevice(ctx->device));
    VSC_HIP(ctx, ctx->sort_tabs.ensure(((size_t)K + 1 + 2) * sizeof(uint64_t)));
    uint64_t *d_bound = (uint64_t *)ctx->sort_tabs.p, *d_range = d_bound + K + 1;
    const uint64_t range[2] = {0, n};
    VSC_HIP(ctx, hipMemcpyAsync(d_range, range, sizeof range, hipMemcpyHostToDevice, ctx->stream));
    VSC_HIP(ctx, launch_key_bounds(hits->d_records, d_range, K, d_bound, ctx->stream));
    uint64_t *dst = (uint64_t *)records;
    if (!records_on_device) {
        VSC_HIP(ctx, ctx->score_feat.ensure(n * sizeof(uint64_t)));
        dst = (uint64_t *)ctx->score_feat.p;
    }
    VSC_HIP(ctx, launch_xpack(hits->d_records, n, genome->d_contig_off, dst, ctx->stream));
    std::vector<uint64_t> bound((size_t)K + 1);
    VSC_HIP(ctx, hipMemcpyAsync(bound.data(), d_bound, bound.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    if (!records_on_device) VSC_HIP(ctx, hipMemcpyAsync(records, dst, n * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (bound[0] != 0 || bound[K] != n) return fail(ctx, VSC_ERR_INVALID, "vsc_hits_pack_exchange: the result holds reads beyond n_guides");
    for (uint32_t k = 0; k < K; ++k) {
        const uint64_t c = bound[k + 1] - bound[k];
        if (c >= (1ull << 32)) return fail(ctx, VSC_ERR_RANGE, "vsc_hits_pack_exchange: more than 2^32 hits of one read and strand");
        key_counts[k] = (uint32_t)c;
    }
    return VSC_OK;
    });
}

}  // extern "C"

namespace {
// the common body of vsc_hits_merge_packed / _votes: records (and votes) of all shards concatenated, host or device
int merge_packed_concat(vsc_ctx *ctx, const vsc_genome *genome, const void *records, const void *votes, int on_device, const uint32_t *key_counts,
                        uint32_t n_shards, uint32_t first_key, uint32_t n_keys, vsc_hits **out, void *votes_out, int votes_out_on_device,
                        const char *who)
{
    if (!ctx || !out) return VSC_ERR_INVALID;
    *out = nullptr;
    ctx->err.clear();
    const std::string w(who);
    if (!genome || genome->ctx != ctx || n_shards == 0 || (n_keys && !key_counts))
        return fail(ctx, VSC_ERR_INVALID, (w + ": null argument or genome of another context").c_str());
    if ((uint64_t)first_key + n_keys > (1ull << 31) || (uint64_t)n_keys * n_shards >= (1ull << 31))
        return fail(ctx, VSC_ERR_RANGE, (w + ": too many keys").c_str());
    uint64_t n = 0;
    std::vector<uint64_t> shard_n(n_shards, 0);
    for (uint32_t s = 0; s < n_shards; ++s) {
        for (uint32_t k = 0; k < n_keys; ++k) shard_n[s] += key_counts[(size_t)s * n_keys + k];
        n += shard_n[s];
    }
    if (n && (!records || (votes_out && !votes))) return fail(ctx, VSC_ERR_INVALID, (w + ": null records").c_str());
    VSC_HIP(ctx, hipSetDevice(ctx->device));
    const uint64_t *records_dev = (const uint64_t *)records;
    const uint16_t *votes_dev = (const uint16_t *)votes;
    if (n && !on_device) {  // staging buffers for host input
        VSC_HIP(ctx, ctx->score_feat.ensure(n * sizeof(uint64_t)));
        VSC_HIP(ctx, hipMemcpyAsync(ctx->score_feat.p, records, n * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
        records_dev = (const uint64_t *)ctx->score_feat.p;
        if (votes) {
            VSC_HIP(ctx, ctx->score_flags.ensure(n * sizeof(uint16_t)));
            VSC_HIP(ctx, hipMemcpyAsync(ctx->score_flags.p, votes, n * sizeof(uint16_t), hipMemcpyHostToDevice, ctx->stream));
            votes_dev = (const uint16_t *)ctx->score_flags.p;
        }
    }
    std::vector<const void *> shard_ptr(n_shards), side_ptr(n_shards);
    uint64_t at = 0;
    for (uint32_t s = 0; s < n_shards; ++s) {
        shard_ptr[s] = records_dev + at;
        side_ptr[s] = votes_dev ? votes_dev + at : nullptr;
        at += shard_n[s];
    }
    DeviceBuf side;  // the merged votes, before they go where the caller wants them
    const int rc = vsc::merge_packed_shards(ctx, genome, shard_ptr.data(), votes ? side_ptr.data() : nullptr, key_counts, n_shards, first_key,
                                            n_keys, out, votes && votes_out ? &side : nullptr);
    if (rc == VSC_OK && n && votes && votes_out) {
        hipError_t e = hipMemcpyAsync(votes_out, side.p, n * sizeof(uint16_t), votes_out_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                                      ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) {
            side.release();
            vsc_hits_free(*out);
            *out = nullptr;
            return fail(ctx, VSC_ERR_DEVICE, who, e);
        }
    }
    side.release();
    return rc;
}
}  // namespace

extern "C" {

int vsc_hits_merge_packed(vsc_ctx *ctx, const vsc_genome *genome, const void *records, int records_on_device, const uint32_t *key_counts,
                          uint32_t n_shards, uint32_t first_key, uint32_t n_keys, vsc_hits **out)
{
    return guarded(ctx, [&]() -> int {
        return merge_packed_concat(ctx, genome, records, nullptr, records_on_device, key_counts, n_shards, first_key, n_keys, out, nullptr, 0,
                                   "vsc_hits_merge_packed");
    });
}

int vsc_hits_merge_packed_votes(vsc_ctx *ctx, const vsc_genome *genome, const void *records, const void *votes, int on_device,
                                const uint32_t *key_counts, uint32_t n_shards, uint32_t first_key, uint32_t n_keys, vsc_hits **out,
                                void *votes_out, int votes_out_on_device)
{
    return guarded(ctx, [&]() -> int {
        return merge_packed_concat(ctx, genome, records, votes, on_device, key_counts, n_shards, first_key, n_keys, out, votes_out,
                                   votes_out_on_device, "vsc_hits_merge_packed_votes");
    });
}

}  // extern "C"

// The merge of vsc_hits_merge_packed over per-shard record buffers (device memory of ctx's device, shard s's records for the
// keys [first_key, first_key + n_keys) at shard_records[s]) - what the multi-device search hands over: every shard's records
// arrive in a buffer of their own, whenever that shard is done.  shard_side (optional): 2 bytes per record that travel with
// it (the shard's classifier votes); they arrive in side_out, in the order of the merged records.
int vsc::merge_packed_shards(vsc_ctx *ctx, const vsc_genome *genome, const void *const *shard_records, const void *const *shard_side,
                             const uint32_t *key_counts, uint32_t n_shards, uint32_t first_key, uint32_t n_keys, vsc_hits **out,
                             DeviceBuf *side_out)
{
    // where every (key, shard) segment lies, and where it goes
    const size_t n_segs = (size_t)n_keys * n_shards;
    std::vector<uint64_t> seg_src(n_segs), seg_dst(n_segs), seg_side(shard_side ? n_segs : 0);
    std::vector<uint32_t> seg_n(n_segs);
    for (uint32_t s = 0; s < n_shards; ++s) {
        uint64_t at = 0;
        for (uint32_t k = 0; k < n_keys; ++k) {
            const size_t seg = (size_t)k * n_shards + s;
            seg_src[seg] = (uint64_t)(uintptr_t)shard_records[s] + at * sizeof(uint64_t);
            if (shard_side) seg_side[seg] = (uint64_t)(uintptr_t)shard_side[s] + at * sizeof(uint16_t);
            at += key_counts[(size_t)s * n_keys + k];
        }
    }
    uint64_t n = 0;
    for (uint32_t k = 0; k < n_keys; ++k)
        for (uint32_t s = 0; s < n_shards; ++s) {
            const size_t seg = (size_t)k * n_shards + s;
            seg_n[seg] = key_counts[(size_t)s * n_keys + k];
            seg_dst[seg] = n;
            n += seg_n[seg];
        }
    VSC_HIP(ctx, hipSetDevice(ctx->device));
    vsc_hits *hits = new (std::nothrow) vsc_hits();
    if (!hits) return fail(ctx, VSC_ERR_NOMEM, "vsc_hits_merge_packed: out of host memory");
    hits->ctx = ctx;
    hits->n = n;
    if (n == 0) {
        hits->host_valid = true;
        *out = hits;
        return VSC_OK;
    }
    hipError_t e = hipSuccess;
    auto step = [&](hipError_t r) {
        if (e == hipSuccess) e = r;
    };
    const size_t tab_bytes = n_segs * (3 * sizeof(uint64_t) + sizeof(uint32_t)) + 2 * sizeof(uint32_t);
    step(ctx->keys_b.ensure(tab_bytes));
    step(take_records(ctx, hits, n));
    if (side_out) step(side_out->ensure(n * sizeof(uint16_t)));
    uint64_t *d_src = (uint64_t *)ctx->keys_b.p, *d_dst = d_src + n_segs, *d_side = d_dst + n_segs;
    uint32_t *d_n = (uint32_t *)(d_side + n_segs);
    uint32_t *d_bad = d_n + n_segs;  // records whose position lies in no contig or that do not ascend inside a segment
    uint32_t n_bad = 0;
    if (e == hipSuccess) {
        step(hipMemcpyAsync(d_src, seg_src.data(), n_segs * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
        step(hipMemcpyAsync(d_dst, seg_dst.data(), n_segs * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
        if (shard_side) step(hipMemcpyAsync(d_side, seg_side.data(), n_segs * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
        step(hipMemcpyAsync(d_n, seg_n.data(), n_segs * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        step(hipMemsetAsync(d_bad, 0, sizeof(uint32_t), ctx->stream));
        step(launch_merge_packed(d_src, d_dst, d_n, (uint32_t)n_segs, n_shards, first_key, genome->d_contig_off, genome->d_contig_end,
                                 genome->n_contigs, hits->d_records, d_bad, shard_side ? d_side : nullptr,
                                 shard_side && side_out ? (uint16_t *)side_out->p : nullptr, ctx->stream));
        step(hipMemcpyAsync(&n_bad, d_bad, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        step(hipStreamSynchronize(ctx->stream));  // (the host tables go out of scope)
    }
    if (e != hipSuccess) {
        vsc_hits_free(hits);
        return fail(ctx, e == hipErrorOutOfMemory ? VSC_ERR_NOMEM : VSC_ERR_DEVICE, "vsc_hits_merge_packed", e);
    }
    if (n_bad) {  // what a peer or the caller sent is not a sorted shard result of this genome
        vsc_hits_free(hits);
        return fail(ctx, VSC_ERR_INVALID, ("vsc_hits_merge_packed: " + std::to_string(n_bad) +
                    " exchange records lie in no contig of the genome or do not ascend inside their (key, shard) segment").c_str());
    }
    *out = hits;
    return VSC_OK;
}

extern "C" {

int vsc_hits_free(vsc_hits *hits)
{
    if (!hits) return VSC_OK;
    if (hits->storage.p) {
        vsc_ctx *ctx = hits->ctx;
        if (ctx->spare_records.size() < 2) {
            ctx->spare_records.push_back(hits->storage);  // reused by the next search
        } else {
            (void)hipSetDevice(ctx->device);
            hits->storage.release();
        }
    }
    delete hits;
    return VSC_OK;
}

// ------------------------------------------------------------------------------------------------
}  // extern "C"

namespace {

// Rows of scratch a scoring call gets: as many as fit.  Halves the request until the device has room (down
// to 64 Ki rows), so that a result larger than the free memory is scored in several passes over the same
// scratch buffers.  vsc_debug_params.score_chunk (tests) forces passes of at most that many rows.
hipError_t score_scratch(vsc_ctx *ctx, uint64_t count, size_t mit_bytes, size_t flag_bytes, size_t feat_bytes, uint64_t *rows_out)
{
    uint64_t rows = count;
    if (ctx->dbg.score_chunk) rows = std::min<uint64_t>(rows, ctx->dbg.score_chunk);
    for (;;) {
        hipError_t e = hipSuccess;
        if (mit_bytes) e = ctx->score_mit.ensure(rows * mit_bytes);
        if (e == hipSuccess && flag_bytes) e = ctx->score_flags.ensure(rows * flag_bytes);
        if (e == hipSuccess && feat_bytes) e = ctx->score_feat.ensure(rows * feat_bytes);
        if (e == hipSuccess) break;
        (void)hipGetLastError();
        if (e != hipErrorOutOfMemory || rows <= (1u << 16)) return e;
        // give back what this attempt got before asking for less
        ctx->score_mit.release();
        ctx->score_flags.release();
        ctx->score_feat.release();
        rows = (rows + 1) / 2;
    }
    *rows_out = rows;
    return hipSuccess;
}

// Word-wise hash of a host array (four independent multiply-xorshift lanes over its 8-byte words + the tail bytes): what the
// caches below key on - an order of magnitude cheaper than walking the bytes, and called once per scoring call.
uint64_t hash_words(const void *p, size_t bytes, uint64_t seed)
{
    const unsigned char *b = (const unsigned char *)p;
    uint64_t h[4] = {seed, seed ^ 0x9E3779B97F4A7C15ull, seed + 0xBF58476D1CE4E5B9ull, ~seed};
    const size_t nw = bytes / 8;
    size_t i = 0;
    for (; i + 4 <= nw; i += 4)
        for (int k = 0; k < 4; ++k) {
            uint64_t w;
            std::memcpy(&w, b + 8 * (i + k), 8);
            h[k] = (h[k] ^ w) * 0x100000001b3ull;
            h[k] ^= h[k] >> 29;
        }
    uint64_t tail = 0xcbf29ce484222325ull;
    for (size_t q = 8 * i; q < bytes; ++q) tail = (tail ^ b[q]) * 0x100000001b3ull;
    uint64_t r = tail ^ (uint64_t)bytes;
    for (int k = 0; k < 4; ++k) r = (r ^ h[k]) * 0xff51afd7ed558ccdull, r ^= r >> 33;
    return r;
}

// The reads as (hi, lo) plane pairs for the scoring kernels, in a buffer of their own (ctx->guides is the search passes'
// and changes with every batch of a streamed search): uploaded when the read set differs from the last call's.
hipError_t upload_read_planes(vsc_ctx *ctx, const uint64_t *guides, uint32_t n_guides)
{
    const uint64_t h = hash_words(guides, (size_t)n_guides * sizeof(uint64_t), 0x5c0 + n_guides);
    if (ctx->score_guides.p && ctx->score_guides_n == n_guides && ctx->score_guides_hash == h) return hipSuccess;
    ctx->score_guides_n = ~0u;
    std::vector<uint32_t> gp((size_t)std::max<uint32_t>(n_guides, 1) * 2, 0);
    for (uint32_t i = 0; i < n_guides; ++i) guide_planes(guides[i], &gp[2 * (size_t)i], &gp[2 * (size_t)i + 1]);
    VSC_TRY(ctx->score_guides.ensure(gp.size() * sizeof(uint32_t)));
    VSC_TRY(hipMemcpyAsync(ctx->score_guides.p, gp.data(), gp.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    VSC_TRY(hipStreamSynchronize(ctx->stream));  // gp goes out of scope
    ctx->score_guides_n = n_guides;
    ctx->score_guides_hash = h;
    return hipSuccess;
}

void fill_score_args(ScoreArgs &s, vsc_ctx *ctx, const vsc_genome *genome)
{
    s.hl = genome->d_hl;
    s.first_pos = (uint32_t)(genome->first_word * 32);
    s.n_plane_words = genome->dev_words;
    s.contig_off = genome->d_contig_off;
    s.guides = (const uint2 *)ctx->score_guides.p;
}

}  // namespace

extern "C" {

int vsc_score_hits(vsc_ctx *ctx, const vsc_genome *genome, const vsc_hits *hits, const uint64_t *guides,
                   uint32_t n_guides, uint64_t first, uint64_t count, double *mit, uint8_t *mit_flags,
                   uint8_t *features)
{
    return guarded(ctx, [&]() -> int {
    if (!ctx) return VSC_ERR_INVALID;
    ctx->err.clear();
    if (!genome || !hits || (n_guides && !guides)) return fail(ctx, VSC_ERR_INVALID, "vsc_score_hits: null argument");
    if (first > hits->n || count > hits->n - first) return fail(ctx, VSC_ERR_INVALID, "vsc_score_hits: row range outside the result");
    ctx->timing.score_ms = 0;
    if (count == 0 || (!mit && !mit_flags && !features)) return VSC_OK;
    VSC_HIP(ctx, hipSetDevice(ctx->device));
    VSC_HIP(ctx, upload_read_planes(ctx, guides, n_guides));
    VSC_HIP(ctx, ensure_hl(ctx, genome));
    uint64_t rows = 0;
    VSC_HIP(ctx, score_scratch(ctx, count, mit ? sizeof(double) : 0, mit_flags ? 1 : 0, features ? VSC_N_FEATURES : 0, &rows));
    double total_ms = 0;
    for (uint64_t done = 0; done < count; done += rows) {  // one pass unless the scratch buffers had to be smaller than the result
        const uint64_t m = std::min(rows, count - done);
        ScoreArgs s{};
        fill_score_args(s, ctx, genome);
        s.hits = hits->d_records + first + done;
        s.n = m;
        if (mit) s.mit = (double *)ctx->score_mit.p;
        if (mit_flags) s.mit_flags = (uint8_t *)ctx->score_flags.p;
        if (features) s.features = (uint8_t *)ctx->score_feat.p;
        VSC_HIP(ctx, hipEventRecord(ctx->ev[kEvStageStart], ctx->stream));
        VSC_HIP(ctx, launch_score(s, ctx->stream));
        VSC_HIP(ctx, hipEventRecord(ctx->ev[kEvStageEnd], ctx->stream));
        if (mit) VSC_HIP(ctx, hipMemcpyAsync(mit + done, s.mit, m * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        if (mit_flags) VSC_HIP(ctx, hipMemcpyAsync(mit_flags + done, s.mit_flags, m, hipMemcpyDeviceToHost, ctx->stream));
        if (features)
            VSC_HIP(ctx, hipMemcpyAsync(features + done * VSC_N_FEATURES, s.features, m * VSC_N_FEATURES, hipMemcpyDeviceToHost, ctx->stream));
        VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        float ms = 0;
        VSC_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev[kEvStageStart], ctx->ev[kEvStageEnd]));
        total_ms += ms;
    }
    ctx->timing.score_ms = total_ms;
    return VSC_OK;
    });
}

// ---- table-driven scores (the score: vsc_table.h, the kernels: vsc_table.hip) ---------------------------------
int vsc_score_table_build(const double *pair, const double *pam, vsc_score_table **out)
{
    if (!out) return VSC_ERR_INVALID;
    *out = nullptr;
    if (!pair || !pam) return VSC_ERR_INVALID;
    static std::atomic<uint64_t> serial{0};
    vsc_score_table *t = new (std::nothrow) vsc_score_table();
    if (!t) return VSC_ERR_NOMEM;
    static_assert(sizeof t->w == kTableWeights * sizeof(double), "vsc_score_table holds pair[20][4][4] and pam[16]");
    std::memcpy(t->w, pair, kTablePairs * sizeof(double));
    std::memcpy(t->w + kTablePairs, pam, 16 * sizeof(double));
    if (!table_valid(t->w)) {  // a weight outside [0, 1] (NaN included) or a diagonal entry other than 1
        delete t;
        return VSC_ERR_INVALID;
    }
    for (double w : t->w) t->zeros += w == 0.0;
    t->serial = serial.fetch_add(1, std::memory_order_relaxed) + 1;
    *out = t;
    return VSC_OK;
}

int vsc_score_table_free(vsc_score_table *table)
{
    delete table;
    return VSC_OK;
}

int vsc_score_table_info(const vsc_score_table *table, vsc_score_table_stats *out)
{
    if (!table || !out) return VSC_ERR_INVALID;
    *out = vsc_score_table_stats{table->serial, table->zeros, 0};
    return VSC_OK;
}

int vsc_table_score(const vsc_score_table *table, uint64_t guide_code, uint64_t site_code, double *score, uint32_t *fixed)
{
    if (!table) return VSC_ERR_INVALID;
    uint32_t gh, gl, sh, sl;
    guide_planes(guide_code, &gh, &gl);
    guide_planes(site_code, &sh, &sl);
    const double x = table_score(table->w, gh, gl, sh, sl);
    if (score) *score = x;
    if (fixed) *fixed = table_fixed(x);
    return VSC_OK;
}

double vsc_table_specificity(uint64_t score_sum)
{
    return 100.0 / (100.0 + (double)score_sum * 0x1p-30) * 100.0;
}

int vsc_score_hits_table(vsc_ctx *ctx, const vsc_genome *genome, const vsc_hits *hits, const uint64_t *guides, uint32_t n_guides,
                         uint64_t first, uint64_t count, const vsc_score_table *table, double *scores, uint32_t *fixed)
{
    return guarded(ctx, [&]() -> int {
    if (!ctx) return VSC_ERR_INVALID;
    ctx->err.clear();
    if (!genome || !hits || !table || (n_guides && !guides)) return fail(ctx, VSC_ERR_INVALID, "vsc_score_hits_table: null argument");
    if (genome->ctx != ctx || hits->ctx != ctx) return fail(ctx, VSC_ERR_INVALID, "vsc_score_hits_table: genome or hits belong to another context");
    if (first > hits->n || count > hits->n - first) return fail(ctx, VSC_ERR_INVALID, "vsc_score_hits_table: row range outside the result");
    ctx->timing.score_ms = 0;
    if (count == 0 || (!scores && !fixed)) return VSC_OK;
    VSC_HIP(ctx, hipSetDevice(ctx->device));
    VSC_HIP(ctx, upload_read_planes(ctx, guides, n_guides));
    VSC_HIP(ctx, ensure_hl(ctx, genome));
    const int trc = resident_table(ctx, table);
    if (trc != VSC_OK) return trc;
    uint64_t rows = 0;
    VSC_HIP(ctx, score_scratch(ctx, count, scores ? sizeof(double) : 0, fixed ? sizeof(uint32_t) : 0, 0, &rows));
    double total_ms = 0;
    for (uint64_t done = 0; done < count; done += rows) {  // one pass unless the scratch buffers had to be smaller than the result
        const uint64_t m = std::min(rows, count - done);
        TableArgs a{};
        a.weights = (const double *)ctx->table_buf.p;
        a.hl = genome->d_hl;
        a.first_pos = (uint32_t)(genome->first_word * 32);
        a.n_plane_words = genome->dev_words;
        a.contig_off = genome->d_contig_off;
        a.guides = (const uint2 *)ctx->score_guides.p;
        a.n_reads = n_guides;
        a.hits = hits->d_records + first + done;
        a.n = m;
        if (scores) a.scores = (double *)ctx->score_mit.p;
        if (fixed) a.fixed = (uint32_t *)ctx->score_flags.p;
        VSC_HIP(ctx, hipEventRecord(ctx->ev[kEvStageStart], ctx->stream));
        VSC_HIP(ctx, launch_table_score(a, ctx->stream));
        VSC_HIP(ctx, hipEventRecord(ctx->ev[kEvStageEnd], ctx->stream));
        if (scores) VSC_HIP(ctx, hipMemcpyAsync(scores + done, a.scores, m * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        if (fixed) VSC_HIP(ctx, hipMemcpyAsync(fixed + done, a.fixed, m * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        float ms = 0;
        VSC_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev[kEvStageStart], ctx->ev[kEvStageEnd]));
        total_ms += ms;
    }
    ctx->timing.score_ms = total_ms;
    return VSC_OK;
    });
}

int vsc_score_pairs(vsc_ctx *ctx, const uint64_t *on_targets, const uint64_t *off_targets, const uint32_t *masks,
                    uint64_t n, double *mit, uint8_t *mit_flags, uint8_t *features)
{
    return guarded(ctx, [&]() -> int {
    if (!ctx) return VSC_ERR_INVALID;
    ctx->err.clear();
    if (n && (!on_targets || !off_targets || !masks)) return fail(ctx, VSC_ERR_INVALID, "vsc_score_pairs: null argument");
    ctx->timing.score_ms = 0;
    if (n == 0 || (!mit && !mit_flags && !features)) return VSC_OK;
    VSC_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<uint32_t> planes((size_t)n * 4);
    for (uint64_t i = 0; i < n; ++i) {
        guide_planes(on_targets[i], &planes[2 * i], &planes[2 * i + 1]);
        guide_planes(off_targets[i], &planes[2 * (n + i)], &planes[2 * (n + i) + 1]);
    }
    VSC_HIP(ctx, ctx->guides.ensure(planes.size() * sizeof(uint32_t) + n * sizeof(uint32_t)));
    uint32_t *d_planes = (uint32_t *)ctx->guides.p;
    uint32_t *d_masks = d_planes + planes.size();
    VSC_HIP(ctx, hipMemcpyAsync(d_planes, planes.data(), planes.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    VSC_HIP(ctx, hipMemcpyAsync(d_masks, masks, n * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    double *d_mit = nullptr;
    uint8_t *d_flags = nullptr, *d_feat = nullptr;
    if (mit) {
        VSC_HIP(ctx, ctx->score_mit.ensure(n * sizeof(double)));
        d_mit = (double *)ctx->score_mit.p;
    }
    if (mit_flags) {
        VSC_HIP(ctx, ctx->score_flags.ensure(n));
        d_flags = (uint8_t *)ctx->score_flags.p;
    }
    if (features) {
        VSC_HIP(ctx, ctx->score_feat.ensure(n * VSC_N_FEATURES));
        d_feat = (uint8_t *)ctx->score_feat.p;
    }
    VSC_HIP(ctx, hipEventRecord(ctx->ev[kEvStageStart], ctx->stream));
    VSC_HIP(ctx, launch_score_pairs((const uint2 *)d_planes, (const uint2 *)(d_planes + 2 * n), d_masks, n, d_mit, d_flags,
                                    d_feat, ctx->stream));
    VSC_HIP(ctx, hipEventRecord(ctx->ev[kEvStageEnd], ctx->stream));
    if (mit) VSC_HIP(ctx, hipMemcpyAsync(mit, d_mit, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (mit_flags) VSC_HIP(ctx, hipMemcpyAsync(mit_flags, d_flags, n, hipMemcpyDeviceToHost, ctx->stream));
    if (features) VSC_HIP(ctx, hipMemcpyAsync(features, d_feat, n * VSC_N_FEATURES, hipMemcpyDeviceToHost, ctx->stream));
    VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    float ms = 0;
    VSC_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev[kEvStageStart], ctx->ev[kEvStageEnd]));
    ctx->timing.score_ms = ms;
    return VSC_OK;
    });
}

int vsc_score_hits_packed(vsc_ctx *ctx, const vsc_genome *genome, const vsc_hits *hits, const uint64_t *guides,
                          uint32_t n_guides, uint64_t first, uint64_t count, void *packed_dev, uint32_t *packed_host,
                          double *mit_host)
{
    return guarded(ctx, [&]() -> int {
    if (!ctx) return VSC_ERR_INVALID;
    ctx->err.clear();
    if (!genome || !hits || (n_guides && !guides)) return fail(ctx, VSC_ERR_INVALID, "vsc_score_hits_packed: null argument");
    if (first > hits->n || count > hits->n - first) return fail(ctx, VSC_ERR_INVALID, "vsc_score_hits_packed: row range outside the result");
    ctx->timing.score_ms = 0;
    if (count == 0) return VSC_OK;
    VSC_HIP(ctx, hipSetDevice(ctx->device));
    VSC_HIP(ctx, upload_read_planes(ctx, guides, n_guides));
    VSC_HIP(ctx, ensure_hl(ctx, genome));
    // rows go to the caller's device buffer (whole result, one pass unless the MIT scratch is short) or through
    // library scratch, as many rows per pass as fit (c3's 1.6e9 rows are 104 GB: several passes)
    uint64_t rows = 0;
    VSC_HIP(ctx, score_scratch(ctx, count, mit_host ? sizeof(double) : 0, 0, packed_dev ? 0 : VSC_PACKED_FEATURE_BYTES, &rows));
    double total_ms = 0;
    for (uint64_t done = 0; done < count; done += rows) {
        const uint64_t m = std::min(rows, count - done);
        ScoreArgs s{};
        fill_score_args(s, ctx, genome);
        s.hits = hits->d_records + first + done;
        s.n = m;
        if (mit_host) s.mit = (double *)ctx->score_mit.p;
        uint4 *dst = packed_dev ? (uint4 *)packed_dev + done * 4 : (uint4 *)ctx->score_feat.p;
        VSC_HIP(ctx, hipEventRecord(ctx->ev[kEvStageStart], ctx->stream));
        // large results on a large genome: visit the rows genome slice by genome slice (launch_score_schedule)
        uint32_t kSliceShift = 28;  // 2^28 positions = 64 MB of interleaved planes
        const uint64_t positions = genome->dev_words * 32;
        bool scheduled = m >= (1u << 22) && positions > (3ull << kSliceShift);
        if (ctx->dbg.score_slices >= 0) scheduled = ctx->dbg.score_slices == 1;  // tests / experiments
        if (ctx->dbg.score_slice_shift) kSliceShift = std::min<uint32_t>(31, std::max<uint32_t>(8, ctx->dbg.score_slice_shift));
        if (scheduled) {
            uint32_t g_edge[2] = {0, 0};
            VSC_HIP(ctx, hipMemcpyAsync(&g_edge[0], &s.hits[0].guide, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
            VSC_HIP(ctx, hipMemcpyAsync(&g_edge[1], &s.hits[m - 1].guide, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
            VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));
            const uint32_t n_slices = (uint32_t)((positions + (1ull << kSliceShift) - 1) >> kSliceShift);
            const uint64_t n_pairs = 2ull * (g_edge[1] - g_edge[0] + 1), n_segs = n_pairs * n_slices;
            if (g_edge[1] >= g_edge[0] && n_segs < (1u << 24)) {
                const size_t words = (size_t)(n_pairs * (n_slices + 1) + n_segs + n_segs + 1);
                VSC_HIP(ctx, ctx->score_sched.ensure(words * sizeof(uint64_t)));
                uint64_t *bounds = (uint64_t *)ctx->score_sched.p;
                uint64_t *seg_start = bounds + n_pairs * (n_slices + 1), *seg_prefix = seg_start + n_segs;
                VSC_HIP(ctx, launch_score_schedule(s, g_edge[0], g_edge[1], kSliceShift, n_slices, bounds, seg_start, seg_prefix, ctx->stream));
                s.seg_start = seg_start;
                s.seg_prefix = seg_prefix;
                s.n_segs = (uint32_t)n_segs;
            }
        }
        VSC_HIP(ctx, launch_score_packed(s, dst, ctx->stream));
        VSC_HIP(ctx, hipEventRecord(ctx->ev[kEvStageEnd], ctx->stream));
        if (packed_host)
            VSC_HIP(ctx, hipMemcpyAsync(packed_host + done * 16, dst, m * VSC_PACKED_FEATURE_BYTES, hipMemcpyDeviceToHost, ctx->stream));
        if (mit_host) VSC_HIP(ctx, hipMemcpyAsync(mit_host + done, s.mit, m * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        float ms = 0;
        VSC_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev[kEvStageStart], ctx->ev[kEvStageEnd]));
        total_ms += ms;
    }
    ctx->timing.score_ms = total_ms;
    return VSC_OK;
    });
}

}  // extern "C"

namespace {

// The forest on the device (vsc_rf_predict*, vsc_score_classify_hits): 8-byte integer nodes over the forest's own
// compact column numbering + the sorted distinct activity thresholds.  Kept on the context until a call brings
// another forest (fingerprint of the model's arrays): a streamed search classifies batch after batch.
// Where column `col` (0..441; 442 = the activity rank) sits in the row the kernel extracts tests from
// (rf_row_words in vsc_kernels.hip; the packed layout is feature_row_packed's)
void row_field(uint32_t col, uint8_t *word, uint8_t *shift, uint8_t *width)
{
    auto set = [&](uint32_t w, uint32_t s, uint32_t n) {
        *word = (uint8_t)w;
        *shift = (uint8_t)s;
        *width = (uint8_t)n;
    };
    if (col == VSC_N_FEATURES) return set(19, 0, 8);          // activity rank
    if (col == 0) return set(0, 21, 5);                        // totalMismatches
    if (col <= 21) return set(0, col - 1, 1);                  // mismatchPos1..21
    if (col <= 33) return set(1, col - 22, 1);                 // AtoC..TtoG
    if (col == 34) return set(1, 12, 5);                       // transitions
    if (col == 35) return set(1, 17, 5);                       // transversions
    if (col < 120) return set(2 + ((col - 36) >> 5), (col - 36) & 31u, 1);    // A1..T20, PAMA..PAMT
    if (col < 424) return set(5 + ((col - 120) >> 5), (col - 120) & 31u, 1);  // AA1..TT19
    if (col < 440) return set(16 + (col - 424) / 6, 5 * ((col - 424) % 6), 5);  // AA..TT (dinucleotide counts)
    if (col == 440) return set(0, 26, 5);                      // adjacentMismatches
    return set(1, 22, 4);                                      // seedMismatches
}

int prepare_forest(vsc_ctx *ctx, const vsc_rf_model *model, const char *who)
{
    if (!model || !model->node_status || !model->feature || !model->left || !model->right || !model->split ||
        !model->node_class || model->n_trees == 0 || model->n_nodes == 0)
        return fail_in(ctx, VSC_ERR_INVALID, who, "null or empty forest");
    const size_t nn = (size_t)model->n_trees * model->n_nodes;
    if (model->n_nodes > (uint32_t)kRfMaxNodes || (size_t)model->n_nodes * sizeof(uint32_t) > (size_t)kRfTileBytes)
        return fail_in(ctx, VSC_ERR_RANGE, who, "a tree has more nodes than the kernel stages at once");
    if (model->n_trees > 65535u) return fail_in(ctx, VSC_ERR_RANGE, who, "more than 65 535 trees");
    uint64_t h = 0xcbf29ce484222325ull ^ ((uint64_t)model->n_trees << 32 | model->n_nodes);
    h = hash_words(model->node_status, nn, h);
    h = hash_words(model->feature, nn * 2, h);
    h = hash_words(model->left, nn * 2, h);
    h = hash_words(model->right, nn * 2, h);
    h = hash_words(model->split, nn * 8, h);
    h = hash_words(model->node_class, nn, h);
    vsc_ctx::Forest &f = ctx->forest;
    const int want_form = ctx->dbg.rf_form;  // (test hook: -1 = the best form the forest allows)
    h ^= (uint64_t)(uint32_t)(want_form + 2) * 0x9E3779B97F4A7C15ull;
    if (f.nodes.p && f.fingerprint == h && f.n_trees == model->n_trees && f.n_nodes == model->n_nodes) return VSC_OK;
    f.fingerprint = 0;
    // distinct activity thresholds, ascending: `activity <= T_j` <=> `rank(activity) <= j`
    std::vector<double> thr;
    for (size_t i = 0; i < nn; ++i)
        if (model->node_status[i] == 1 && model->feature[i] == VSC_N_FEATURES) thr.push_back(model->split[i]);
    std::sort(thr.begin(), thr.end());
    thr.erase(std::unique(thr.begin(), thr.end()), thr.end());
    if (thr.size() > 255) return fail_in(ctx, VSC_ERR_RANGE, who, "the forest splits the on-target activity at more than 255 values");
    // the distinct tests (column, integer threshold); a split below zero is never met, one at or above 255 always
    struct Split { uint16_t col; uint8_t thr; bool never; };
    auto split_of = [&](size_t i) {
        Split sp{model->feature[i], 0, false};
        const double v = model->split[i];
        if (sp.col == VSC_N_FEATURES) sp.thr = (uint8_t)(std::lower_bound(thr.begin(), thr.end(), v) - thr.begin());
        else if (v < 0) sp.never = true;
        else sp.thr = (uint8_t)std::min(255.0, std::floor(v));
        return sp;
    };
    std::vector<uint32_t> keys;  // col << 8 | thr of every split node that can go either way
    for (size_t i = 0; i < nn; ++i) {
        if (model->node_status[i] != 1) continue;
        const uint16_t ft = model->feature[i];
        // randomForest numbers the daughters of a node behind it: a daughter at or before its parent is a cycle
        const uint32_t own = (uint32_t)(i % model->n_nodes) + 1;  // 1-based index of this node in its tree
        if (ft > VSC_N_FEATURES || model->left[i] <= own || model->right[i] <= own || model->left[i] > model->n_nodes ||
            model->right[i] > model->n_nodes)
            return fail_in(ctx, VSC_ERR_INVALID, who, "malformed forest (feature or daughter index out of range, or a daughter that does not lie behind its parent)");
        if (!(model->split[i] == model->split[i])) return fail_in(ctx, VSC_ERR_INVALID, who, "malformed forest (NaN split)");
        const Split sp = split_of(i);
        if (!sp.never) keys.push_back((uint32_t)sp.col << 8 | sp.thr);
    }
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    if (keys.empty()) keys.push_back(0);  // (a forest of stumps without a usable split still needs a test table)
    if (keys.size() > (size_t)kRfMaxTests)
        return fail_in(ctx, VSC_ERR_RANGE, who, "the forest uses more than 1 024 distinct (predictor, threshold) tests");
    // tests sorted by the row word they read (the kernel walks the words in a compile-time loop)
    std::vector<RfTest> tests(keys.size());
    for (size_t i = 0; i < keys.size(); ++i) {
        RfTest &ts = tests[i];
        ts.dense_col = (uint16_t)(keys[i] >> 8);
        ts.thr = (uint8_t)keys[i];
        ts.pad = 0;
        row_field(ts.dense_col, &ts.word, &ts.shift, &ts.width);
    }
    std::stable_sort(tests.begin(), tests.end(), [](const RfTest &x, const RfTest &y) { return x.word < y.word; });
    std::vector<uint32_t> test_begin(kRfRowWords + 1, 0);
    for (const RfTest &ts : tests) test_begin[ts.word + 1]++;
    for (int k = 0; k < kRfRowWords; ++k) test_begin[k + 1] += test_begin[k];
    auto test_index = [&](uint16_t col, uint8_t t) {
        for (size_t i = 0; i < tests.size(); ++i)
            if (tests[i].dense_col == col && tests[i].thr == t) return (uint32_t)i;
        return 0u;
    };
    std::vector<uint32_t> index_of(keys.size());  // by position in `keys`
    for (size_t i = 0; i < keys.size(); ++i) index_of[i] = test_index((uint16_t)(keys[i] >> 8), (uint8_t)keys[i]);
    // nodes: test | left << 10 | right << 20 (0-based) | terminal << 30 | votes class "1" << 31; or the compact form
    // (trees of <= 512 nodes): test | (nodes to skip | vote << 10) << 10 (right) / << 21 (left)
    const bool compact = model->n_nodes <= 512 && want_form != 0;
    std::vector<uint32_t> nodes(nn);
    std::vector<uint8_t> depth(model->n_trees, 0);
    std::vector<uint16_t> level(model->n_nodes);
    for (uint32_t tr = 0; tr < model->n_trees; ++tr) {
        std::fill(level.begin(), level.end(), 0);
        for (uint32_t k = 0; k < model->n_nodes; ++k) {
            const size_t i = (size_t)tr * model->n_nodes + k;
            if (model->node_status[i] != 1) {  // terminal (or an unused slot behind the tree's last node: never reached)
                nodes[i] = k << 10 | k << 20 | 1u << 30 | (model->node_class[i] == 2 ? 1u << 31 : 0u);
                continue;
            }
            const Split sp = split_of(i);
            uint32_t l = model->left[i] - 1u, r = model->right[i] - 1u, test = 0;
            if (sp.never) l = r;  // x <= (negative) never holds: both ways lead right
            else test = index_of[std::lower_bound(keys.begin(), keys.end(), (uint32_t)sp.col << 8 | sp.thr) - keys.begin()];
            nodes[i] = test | l << 10 | r << 20;
            if (compact) {
                // (x <= thr takes the LEFT daughter: filed in the upper field, which the kernel selects with 10 + 11 * bit)
                // a daughter field = how many nodes further on the walk continues (10 bits) | vote (bit 10): a split
                // daughter lies d - k nodes behind its parent; a terminal one sends the walk to the NEXT tree's root,
                // n_nodes - k nodes on (trees lie back to back at a stride of n_nodes), and brings its vote along
                auto daughter = [&](uint32_t d) {
                    const size_t j = (size_t)tr * model->n_nodes + d;
                    return model->node_status[j] == 1 ? d - k : ((model->n_nodes - k) | (model->node_class[j] == 2 ? 1u << 10 : 0u));
                };
                nodes[i] = test | daughter(r) << 10 | daughter(l) << 21;
            }
            level[l] = level[r] = (uint16_t)(level[k] + 1);  // (daughters lie behind their parent: level[k] is final here)
            depth[tr] = (uint8_t)std::min<uint32_t>(255, std::max<uint32_t>(depth[tr], level[k] + 1u));
        }
        if (compact && model->node_status[(size_t)tr * model->n_nodes] != 1) {
            // a tree that is one terminal node: a root whose daughters both are "terminal, the root's vote"
            const uint32_t leaf = model->n_nodes | (model->node_class[(size_t)tr * model->n_nodes] == 2 ? 1u << 10 : 0u);
            nodes[(size_t)tr * model->n_nodes] = leaf << 10 | leaf << 21;
        }
    }
    // PAIR form (vsc_internal.h): a node of 8 bytes holds a split node AND its two daughters - two levels per LDS read.
    // Pair nodes are rooted at the split nodes on even levels; a tree's pair nodes lie in breadth-first order (every exit
    // leads forward), the trees back to back at a stride of `pair_stride` nodes.  For forests of at most 232 tests and 127
    // pair nodes per tree (rfClassifier: 217 and 70).
    std::vector<uint64_t> pairs;
    uint32_t pair_stride = 0;
    if (compact && want_form != 1 && tests.size() <= (size_t)kRfPairMaxTests) {
        auto split = [&](uint32_t tr, uint32_t k) { return model->node_status[(size_t)tr * model->n_nodes + k] == 1; };
        std::vector<std::vector<uint32_t>> roots(model->n_trees);  // per tree: the split nodes that root a pair node, in order
        std::vector<uint32_t> index_in(model->n_nodes);
        // (first pass: the roots of every tree; second pass below fills the words once the stride is known)
        auto daughters = [&](uint32_t tr, uint32_t k, uint32_t &l, uint32_t &r, uint32_t &test) {
            const size_t i = (size_t)tr * model->n_nodes + k;
            const Split sp = split_of(i);
            l = model->left[i] - 1u, r = model->right[i] - 1u, test = 0;
            if (sp.never) l = r;
            else test = index_of[std::lower_bound(keys.begin(), keys.end(), (uint32_t)sp.col << 8 | sp.thr) - keys.begin()];
        };
        for (uint32_t tr = 0; tr < model->n_trees; ++tr) {
            auto &q = roots[tr];
            q.push_back(0);  // (a tree that is one terminal node: a pair node whose four exits carry the root's vote)
            for (size_t at = 0; at < q.size() && split(tr, q[at]); ++at) {
                uint32_t l, r, test;
                daughters(tr, q[at], l, r, test);
                for (uint32_t c : {l, r}) {
                    if (!split(tr, c)) continue;
                    uint32_t cl, cr, ct;
                    daughters(tr, c, cl, cr, ct);
                    for (uint32_t g : {cl, cr})
                        if (split(tr, g) && std::find(q.begin(), q.end(), g) == q.end()) q.push_back(g);
                }
            }
            pair_stride = std::max<uint32_t>(pair_stride, (uint32_t)q.size());
        }
        if (pair_stride <= 127) {
            pairs.assign((size_t)model->n_trees * pair_stride, 0);
            for (uint32_t tr = 0; tr < model->n_trees; ++tr) {
                const auto &q = roots[tr];
                for (uint32_t j = 0; j < q.size(); ++j) index_in[q[j]] = j;
                auto vote_of = [&](uint32_t k) { return model->node_class[(size_t)tr * model->n_nodes + k] == 2 ? 1u : 0u; };
                for (uint32_t j = 0; j < q.size(); ++j) {
                    // an exit (one byte): vote | pair nodes to skip << 1 - to the pair node rooted at a split granddaughter, or -
                    // terminal - to the next tree's root with the vote
                    auto exit_to = [&](uint32_t g) { return split(tr, g) ? (index_in[g] - j) << 1 : ((pair_stride - j) << 1 | vote_of(g)); };
                    uint32_t ex[4], t_root = 0, t_left = 0, t_right = 0;  // ex[2 * (root bit) + (daughter bit)]; bit set = x <= thr = LEFT
                    if (!split(tr, q[j])) {
                        ex[0] = ex[1] = ex[2] = ex[3] = exit_to(q[j]);
                    } else {
                        uint32_t l, r;
                        daughters(tr, q[j], l, r, t_root);
                        auto half = [&](uint32_t c, uint32_t &t, uint32_t &on_left, uint32_t &on_right) {
                            if (!split(tr, c)) { t = 0; on_left = on_right = exit_to(c); return; }
                            uint32_t cl, cr;
                            daughters(tr, c, cl, cr, t);
                            on_left = exit_to(cl), on_right = exit_to(cr);
                        };
                        half(l, t_left, ex[3], ex[2]);
                        half(r, t_right, ex[1], ex[0]);
                    }
                    // a test in the upper word: its bit in the row's test word at bits s .. s + 4, the word's number at s + 10 ..
                    // s + 12 (s = 0 root, 5 right daughter, 18 left daughter: rf_predict_kernel masks the word number in place)
                    // (test i: word i / 29, bit 3 + i % 29; the root's field holds the bit's position, a daughter's the position - 3)
                    const uint32_t per = 32u - (uint32_t)kRfPairFirstBit;
                    auto field = [&](uint32_t test, uint32_t s, bool root) {
                        return (uint64_t)((test % per + (root ? (uint32_t)kRfPairFirstBit : 0u)) | (test / per) << 10) << s;
                    };
                    uint64_t w = 0;
                    for (int e = 0; e < 4; ++e) w |= (uint64_t)ex[e] << (8 * e);
                    w |= (field(t_root, 0, true) | field(t_right, 5, false) | field(t_left, 18, false)) << 32;
                    pairs[(size_t)tr * pair_stride + j] = w;
                }
            }
        }
    }
    VSC_HIP(ctx, hipSetDevice(ctx->device));
    auto pad = [](size_t n) { return (n + 255) / 256 * 256; };
    const size_t node_bytes = pairs.empty() ? nn * sizeof(uint32_t) : pairs.size() * sizeof(uint64_t);
    const size_t nodes_b = pad(node_bytes), depth_b = pad(depth.size()), tests_b = pad(tests.size() * sizeof(RfTest));
    VSC_HIP(ctx, f.nodes.ensure(nodes_b + depth_b + tests_b + pad(test_begin.size() * sizeof(uint32_t))));
    char *base = (char *)f.nodes.p;
    VSC_HIP(ctx, hipMemcpyAsync(base, pairs.empty() ? (const void *)nodes.data() : (const void *)pairs.data(), node_bytes, hipMemcpyHostToDevice, ctx->stream));
    VSC_HIP(ctx, hipMemcpyAsync(base + nodes_b, depth.data(), depth.size(), hipMemcpyHostToDevice, ctx->stream));
    VSC_HIP(ctx, hipMemcpyAsync(base + nodes_b + depth_b, tests.data(), tests.size() * sizeof(RfTest), hipMemcpyHostToDevice, ctx->stream));
    VSC_HIP(ctx, hipMemcpyAsync(base + nodes_b + depth_b + tests_b, test_begin.data(), test_begin.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (the host vectors go out of scope)
    f.depth_at = nodes_b;
    f.tests_at = nodes_b + depth_b;
    f.begin_at = nodes_b + depth_b + tests_b;
    f.n_tests = (uint32_t)tests.size();
    f.form = !pairs.empty() ? 2u : compact ? 1u : 0u;
    f.node_stride = !pairs.empty() ? pair_stride : model->n_nodes;
    f.n_trees = model->n_trees;
    f.n_nodes = model->n_nodes;
    f.thresholds = thr;
    f.fingerprint = h;
    return VSC_OK;
}

void fill_forest(RfArgs &a, const vsc_ctx *ctx)
{
    const vsc_ctx::Forest &f = ctx->forest;
    const char *base = (const char *)f.nodes.p;
    a.nodes = (const uint32_t *)base;
    a.depth = (const uint8_t *)(base + f.depth_at);
    a.tests = (const RfTest *)(base + f.tests_at);
    a.test_begin = (const uint32_t *)(base + f.begin_at);
    a.n_tests = f.n_tests;
    a.compact = f.form;
    a.n_trees = f.n_trees;
    a.n_nodes = f.node_stride;
}

uint8_t activity_rank(const std::vector<double> &thr, double activity)
{
    return (uint8_t)(std::lower_bound(thr.begin(), thr.end(), activity) - thr.begin());  // thresholds strictly below
}

// The reads' activity ranks for the resident forest in ctx->forest.ranks: uploaded when the activities or the forest differ from
// the last call's (vsc_score_classify_hits batch after batch, the passes of vsc_search_*_classified).
int resident_ranks(vsc_ctx *ctx, const double *guide_activity, uint32_t n_guides)
{
    const uint64_t rank_key = hash_words(guide_activity, (size_t)n_guides * sizeof(double), ctx->forest.fingerprint ^ n_guides);
    if (!ctx->forest.ranks.p || ctx->forest.ranks_key != rank_key || ctx->forest.ranks_n != n_guides) {
        std::vector<uint8_t> ranks(std::max<uint32_t>(n_guides, 1));
        for (uint32_t g = 0; g < n_guides; ++g) ranks[g] = activity_rank(ctx->forest.thresholds, guide_activity[g]);
        ctx->forest.ranks_n = ~0u;
        VSC_HIP(ctx, ctx->forest.ranks.ensure(ranks.size()));
        VSC_HIP(ctx, hipMemcpyAsync(ctx->forest.ranks.p, ranks.data(), ranks.size(), hipMemcpyHostToDevice, ctx->stream));
        VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));  // `ranks` goes out of scope
        ctx->forest.ranks_key = rank_key;
        ctx->forest.ranks_n = n_guides;
    }
    return VSC_OK;
}

// vsc_rf_predict / vsc_rf_predict_packed: the rows from the host (dense) or from host / device memory (packed)
int rf_predict(vsc_ctx *ctx, const vsc_rf_model *model, const uint8_t *dense, const void *packed, int packed_on_device,
               const double *activity, uint64_t n, double *prob, uint8_t *cls, uint8_t *tie, const char *who)
{
    ctx->err.clear();
    if (n && ((!dense && !packed) || !activity)) return fail_in(ctx, VSC_ERR_INVALID, who, "null or empty argument");
    const int frc = prepare_forest(ctx, model, who);
    if (frc != VSC_OK) return frc;
    if (n == 0) return VSC_OK;
    VSC_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<uint8_t> ranks(n);
    for (uint64_t i = 0; i < n; ++i) ranks[i] = activity_rank(ctx->forest.thresholds, activity[i]);
    VSC_HIP(ctx, ctx->score_mit.ensure(n));
    VSC_HIP(ctx, ctx->score_flags.ensure(n * sizeof(uint32_t)));
    VSC_HIP(ctx, hipMemcpyAsync(ctx->score_mit.p, ranks.data(), n, hipMemcpyHostToDevice, ctx->stream));
    RfArgs a{};
    fill_forest(a, ctx);
    a.act_rank = (const uint8_t *)ctx->score_mit.p;
    a.n = n;
    a.votes = (uint32_t *)ctx->score_flags.p;
    if (dense) {
        VSC_HIP(ctx, ctx->score_feat.ensure(n * VSC_N_FEATURES));
        VSC_HIP(ctx, hipMemcpyAsync(ctx->score_feat.p, dense, n * VSC_N_FEATURES, hipMemcpyHostToDevice, ctx->stream));
        a.dense = (const uint8_t *)ctx->score_feat.p;
    } else if (packed_on_device) {
        a.packed = (const uint4 *)packed;
    } else {
        VSC_HIP(ctx, ctx->score_feat.ensure(n * VSC_PACKED_FEATURE_BYTES));
        VSC_HIP(ctx, hipMemcpyAsync(ctx->score_feat.p, packed, n * VSC_PACKED_FEATURE_BYTES, hipMemcpyHostToDevice, ctx->stream));
        a.packed = (const uint4 *)ctx->score_feat.p;
    }
    // few rows: split the trees over several workgroups per row tile so that the device is filled
    const uint64_t tiles = (n + kRfRows - 1) / kRfRows;
    a.tree_splits = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>({(uint64_t)2 * ctx->n_cus / tiles, 32, model->n_trees}));
    if (a.tree_splits > 1) VSC_HIP(ctx, hipMemsetAsync(a.votes, 0, n * sizeof(uint32_t), ctx->stream));
    VSC_HIP(ctx, hipEventRecord(ctx->ev[kEvStageStart], ctx->stream));
    VSC_HIP(ctx, launch_rf_predict(a, ctx->stream));
    VSC_HIP(ctx, hipEventRecord(ctx->ev[kEvStageEnd], ctx->stream));
    std::vector<uint32_t> votes(n);
    VSC_HIP(ctx, hipMemcpyAsync(votes.data(), a.votes, n * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (uint64_t i = 0; i < n; ++i) {
        if (prob) prob[i] = (double)votes[i] / (double)model->n_trees;  // type = "prob": votes / ntree
        if (cls) cls[i] = 2 * votes[i] > model->n_trees;
        if (tie) tie[i] = 2 * votes[i] == model->n_trees;
    }
    float ms = 0;
    VSC_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev[kEvStageStart], ctx->ev[kEvStageEnd]));
    ctx->timing.score_ms = ms;
    return VSC_OK;
}

}  // namespace

extern "C" {

int vsc_rf_predict(vsc_ctx *ctx, const vsc_rf_model *model, const uint8_t *features, const double *activity, uint64_t n,
                   double *prob, uint8_t *cls, uint8_t *tie)
{
    return guarded(ctx, [&]() -> int {
    if (!ctx) return VSC_ERR_INVALID;
    return rf_predict(ctx, model, features, nullptr, 0, activity, n, prob, cls, tie, "vsc_rf_predict");
    });
}

int vsc_rf_predict_packed(vsc_ctx *ctx, const vsc_rf_model *model, const void *packed_rows, int rows_on_device,
                          const double *activity, uint64_t n, double *prob, uint8_t *cls, uint8_t *tie)
{
    return guarded(ctx, [&]() -> int {
    if (!ctx) return VSC_ERR_INVALID;
    return rf_predict(ctx, model, nullptr, packed_rows, rows_on_device, activity, n, prob, cls, tie, "vsc_rf_predict_packed");
    });
}

int vsc_score_classify_hits(vsc_ctx *ctx, const vsc_genome *genome, const vsc_hits *hits, const uint64_t *guides, uint32_t n_guides,
                            const double *guide_activity, const vsc_rf_model *model, uint64_t first, uint64_t count, void *votes_dev,
                            uint16_t *votes_host, double *mit_host)
{
    return guarded(ctx, [&]() -> int {
    if (!ctx) return VSC_ERR_INVALID;
    ctx->err.clear();
    if (!genome || !hits || (n_guides && (!guides || !guide_activity)))
        return fail(ctx, VSC_ERR_INVALID, "vsc_score_classify_hits: null argument");
    if (first > hits->n || count > hits->n - first) return fail(ctx, VSC_ERR_INVALID, "vsc_score_classify_hits: row range outside the result");
    const int frc = prepare_forest(ctx, model, "vsc_score_classify_hits");
    if (frc != VSC_OK) return frc;
    ctx->timing.score_ms = 0;
    if (count == 0) return VSC_OK;
    VSC_HIP(ctx, hipSetDevice(ctx->device));
    VSC_HIP(ctx, upload_read_planes(ctx, guides, n_guides));
    VSC_HIP(ctx, ensure_hl(ctx, genome));
    // the reads' activity ranks: uploaded when the activities or the forest differ from the last call's (a streamed search
    // classifies batch after batch with the same ones)
    const int rrc = resident_ranks(ctx, guide_activity, n_guides);
    if (rrc != VSC_OK) return rrc;
    // 2 bytes (+ 8 with the MIT score) per hit of scratch: one pass for any result that fits the device at all
    uint64_t rows = 0;
    VSC_HIP(ctx, score_scratch(ctx, count, mit_host ? sizeof(double) : 0, votes_dev ? 0 : sizeof(uint16_t), 0, &rows));
    double total_ms = 0;
    for (uint64_t done = 0; done < count; done += rows) {
        const uint64_t m = std::min(rows, count - done);
        RfArgs a{};
        fill_forest(a, ctx);
        fill_score_args(a.score, ctx, genome);
        a.score.hits = hits->d_records + first + done;
        a.score.n = m;
        if (mit_host) a.score.mit = (double *)ctx->score_mit.p;
        a.act_rank = (const uint8_t *)ctx->forest.ranks.p;
        a.n = m;
        a.votes16 = votes_dev ? (uint16_t *)votes_dev + done : (uint16_t *)ctx->score_flags.p;
        a.tree_splits = 1;
        VSC_HIP(ctx, hipEventRecord(ctx->ev[kEvStageStart], ctx->stream));
        VSC_HIP(ctx, launch_rf_predict(a, ctx->stream));
        VSC_HIP(ctx, hipEventRecord(ctx->ev[kEvStageEnd], ctx->stream));
        if (votes_host) VSC_HIP(ctx, hipMemcpyAsync(votes_host + done, a.votes16, m * sizeof(uint16_t), hipMemcpyDeviceToHost, ctx->stream));
        if (mit_host) VSC_HIP(ctx, hipMemcpyAsync(mit_host + done, a.score.mit, m * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        float ms = 0;
        VSC_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev[kEvStageStart], ctx->ev[kEvStageEnd]));
        total_ms += ms;
    }
    ctx->timing.score_ms = total_ms;
    return VSC_OK;
    });
}

}  // extern "C"

// ---- cut sites: vsc_hits_sites / vsc_pattern_hits_sites on the device, vsc_sites_collapse* on the host ---------
namespace {

int site_params_check(const vsc_site_params *p)
{
    if (!p || p->reserved[0] || p->reserved[1] || p->anchor > VSC_SITE_ANCHOR_START) return VSC_ERR_INVALID;
    return p->len >= VSC_PATTERN_MIN_LEN && p->len <= VSC_PATTERN_MAX_LEN ? VSC_OK : VSC_ERR_INVALID;
}

// The definition on host arrays, by vsc_sites.h's gather: the flags of both lists, the survivors in front of every record, and
// for every best alignment the rank the write pass of vsc_sites.hip gives it.
template <int kPlain>
int sites_collapse_host(const void *plain, uint64_t n_plain, const vsc_bulge_hit *bulged, uint64_t n_bulged, uint32_t n_guides,
                        const vsc_site_params *p, vsc_site *sites, uint64_t capacity, uint64_t *n_sites, vsc_site_summary *rows)
{
    if (n_sites) *n_sites = 0;
    if (site_params_check(p) != VSC_OK || (n_plain && !plain) || (n_bulged && !bulged) || (!plain && !bulged) || (!rows && !sites && !n_sites))
        return VSC_ERR_INVALID;
    if (n_plain + n_bulged > 0xFFFFFFFFull || n_plain > 0xFFFFFFFFull || n_bulged > 0xFFFFFFFFull) return VSC_ERR_RANGE;
    return guarded(nullptr, [&]() -> int {
    const uint32_t np = (uint32_t)n_plain, nb = (uint32_t)n_bulged;
    auto load = [&](bool in_bulged, uint32_t i) { return in_bulged ? site_load<kSiteBulge>(bulged, i) : site_load<kPlain>(plain, i); };
    for (int l = 0; l < 2; ++l)
        for (uint32_t i = 0; i < (l ? nb : np); ++i)
            if (load(l, i).guide >= n_guides) return VSC_ERR_INVALID;
    std::vector<uint32_t> row_words;
    if (rows) row_words.assign((size_t)n_guides * kSiteRowWords, 0u);
    // before[l][i] = best alignments among records [0, i) of list l
    std::vector<uint32_t> before[2];
    before[0].assign((size_t)np + 1, 0u);
    before[1].assign((size_t)nb + 1, 0u);
    for (int l = 0; l < 2; ++l)
        for (uint32_t i = 0; i < (l ? nb : np); ++i) {
            const SiteAln x = load(l, i);
            const SiteView v = site_gather<kPlain>(plain, np, bulged, nb, l, i, x, p->len, p->anchor);
            before[l][i + 1] = before[l][i] + (v.best == site_rank(x.d, x.nm) ? 1u : 0u);
            if (rows) ++row_words[(size_t)x.guide * kSiteRowWords + kSiteRowAlignments];
        }
    const uint64_t total = (uint64_t)before[0][np] + before[1][nb];
    if (n_sites) *n_sites = total;
    const bool write = sites && total <= capacity;
    for (int l = 0; l < 2; ++l)
        for (uint32_t i = 0; i < (l ? nb : np); ++i) {
            if (before[l][i + 1] == before[l][i]) continue;
            const SiteAln x = load(l, i);
            const SiteView v = site_gather<kPlain>(plain, np, bulged, nb, l, i, x, p->len, p->anchor);
            if (write) {
                const uint32_t j = site_other_below<kPlain>(plain, np, bulged, nb, l, x);
                site_record(x, i, v, p->len, p->anchor, (uint32_t *)&sites[(size_t)before[l][i] + before[l ^ 1][j]]);
            }
            if (rows) {
                uint32_t *row = &row_words[(size_t)x.guide * kSiteRowWords];
                ++row[kSiteRowSites];
                ++row[site_row_count_word(x)];
                if (site_bulge_only(v)) ++row[kSiteRowBulgeOnly];
            }
        }
    if (rows && n_guides) std::memcpy(rows, row_words.data(), row_words.size() * sizeof(uint32_t));
    return sites && !write ? VSC_ERR_RANGE : VSC_OK;
    });
}

// The device call behind both entry points: d_plain / n_plain = the plain result's records (kind = kSiteHit / kSitePattern).
int hits_sites_device(vsc_ctx *ctx, const char *who, int kind, const void *d_plain, uint64_t n_plain, vsc_bulge_hits *bulged,
                      uint32_t n_guides, const vsc_site_params *p, vsc_sites **out, vsc_site_summary *rows)
{
    ctx->err.clear();
    if (site_params_check(p) != VSC_OK)
        return fail_in(ctx, VSC_ERR_INVALID, who, "len in 16..32, a known anchor and zeroed reserved fields are needed");
    if (!out && !rows) return fail_in(ctx, VSC_ERR_INVALID, who, "neither records nor rows are asked for");
    const uint64_t n_bulged = bulged ? bulged->n : 0;
    if (n_plain + n_bulged > 0xFFFFFFFFull) return fail_in(ctx, VSC_ERR_RANGE, who, "more than 2^32 - 1 alignments");
    if (rows && n_guides) std::memset(rows, 0, (size_t)n_guides * sizeof(vsc_site_summary));
    std::unique_ptr<vsc_sites, int (*)(vsc_sites *)> res(nullptr, object_free<vsc_sites>);
    if (out) {
        res.reset(new (std::nothrow) vsc_sites());
        if (!res) return fail_in(ctx, VSC_ERR_NOMEM, who, "out of host memory");
        res->ctx = ctx;
    }
    SiteArgs a{};
    a.plain = d_plain;
    a.bulged = n_bulged ? bulged->storage.p : nullptr;
    a.n_plain = (uint32_t)n_plain;
    a.n_bulged = (uint32_t)n_bulged;
    a.tiles_plain = (uint32_t)((n_plain + kSiteTile - 1) / kSiteTile);
    a.tiles_bulged = (uint32_t)((n_bulged + kSiteTile - 1) / kSiteTile);
    a.n_guides = n_guides;
    a.len = p->len;
    a.anchor = p->anchor;
    const uint32_t n_tiles = a.tiles_plain + a.tiles_bulged;
    if (n_tiles) {
        VSC_HIP(ctx, hipSetDevice(ctx->device));
        // scratch, 256-byte aligned parts: [ballots][offsets + total, then the invalid flag][rows][counts]
        const size_t off_at = round256((size_t)n_tiles * sizeof(unsigned long long));
        const size_t flag_at = off_at + ((size_t)n_tiles + 1) * sizeof(unsigned long long);
        const size_t rows_at = round256(flag_at + 8);
        const size_t row_bytes = rows ? (size_t)n_guides * sizeof(vsc_site_summary) : 0;
        const size_t count_at = rows_at + round256(row_bytes);
        VSC_HIP(ctx, ctx->sites_tabs.ensure(count_at + (size_t)n_tiles * sizeof(uint32_t)));
        char *base = (char *)ctx->sites_tabs.p;
        a.ballot = (unsigned long long *)base;
        a.tile_off = (const unsigned long long *)(base + off_at);
        a.invalid = (uint32_t *)(base + flag_at);
        a.rows = row_bytes ? (uint32_t *)(base + rows_at) : nullptr;
        a.tile_count = (uint32_t *)(base + count_at);
        VSC_HIP(ctx, hipMemsetAsync(base + flag_at, 0, rows_at + row_bytes - flag_at, ctx->stream));
        VSC_HIP(ctx, hipEventRecord(ctx->ev[kEvStageStart], ctx->stream));
        VSC_HIP(ctx, launch_site_flag(a, kind, ctx->n_cus, ctx->stream));
        VSC_HIP(ctx, launch_enum_scan(a.tile_count, n_tiles, (unsigned long long *)(base + off_at), ctx->stream));
        VSC_HIP(ctx, hipEventRecord(ctx->ev[kEvStageEnd], ctx->stream));
        // one read-back: the total (it sizes the result) with the invalid flag behind it
        unsigned long long back[2] = {0, 0};
        VSC_HIP(ctx, hipMemcpyAsync(back, a.tile_off + n_tiles, sizeof back, hipMemcpyDeviceToHost, ctx->stream));
        VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if ((uint32_t)back[1]) return fail_in(ctx, VSC_ERR_INVALID, who, "a record's guide is not below n_guides");
        a.n_sites = back[0];
        if (out && a.n_sites) {
            VSC_HIP(ctx, res->storage.ensure((size_t)a.n_sites * sizeof(vsc_site)));
            a.sites = (uint4 *)res->storage.p;
            res->n = a.n_sites;
        }
        VSC_HIP(ctx, hipEventRecord(ctx->ev[kEvStage2Start], ctx->stream));
        if (a.sites || a.rows) VSC_HIP(ctx, launch_site_write(a, kind, ctx->n_cus, ctx->stream));
        VSC_HIP(ctx, hipEventRecord(ctx->ev[kEvStage2End], ctx->stream));
        if (a.rows) VSC_HIP(ctx, hipMemcpyAsync(rows, a.rows, row_bytes, hipMemcpyDeviceToHost, ctx->stream));
        VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        float ms = 0;
        VSC_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev[kEvStageStart], ctx->ev[kEvStageEnd]));
        ctx->sites_ms[0] = ms;
        VSC_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev[kEvStage2Start], ctx->ev[kEvStage2End]));
        ctx->sites_ms[1] = ms;
    }
    if (out) *out = res.release();
    return VSC_OK;
}

template <class Plain>
int hits_sites_entry(vsc_ctx *ctx, const char *who, int kind, Plain *plain, const void *d_plain, vsc_bulge_hits *bulged, uint32_t n_guides,
                     const vsc_site_params *p, vsc_sites **out, vsc_site_summary *rows)
{
    if (out) *out = nullptr;
    if (!ctx) return VSC_ERR_INVALID;
    return guarded(ctx, [&]() -> int {
    if (!plain && !bulged) return fail_in(ctx, VSC_ERR_INVALID, who, "neither plain nor bulged records");
    if ((plain && plain->ctx != ctx) || (bulged && bulged->ctx != ctx)) return fail_in(ctx, VSC_ERR_INVALID, who, "a result of another context");
    return hits_sites_device(ctx, who, kind, plain && plain->n ? d_plain : nullptr, plain ? plain->n : 0, bulged, n_guides, p, out, rows);
    });
}

}  // namespace

extern "C" {

int vsc_hits_sites(vsc_ctx *ctx, vsc_hits *plain, vsc_bulge_hits *bulged, uint32_t n_guides, const vsc_site_params *params, vsc_sites **out,
                   vsc_site_summary *rows)
{
    return hits_sites_entry(ctx, "vsc_hits_sites", kSiteHit, plain, plain ? (const void *)plain->d_records : nullptr, bulged, n_guides, params, out,
                            rows);
}

int vsc_pattern_hits_sites(vsc_ctx *ctx, vsc_pattern_hits *plain, vsc_bulge_hits *bulged, uint32_t n_guides, const vsc_site_params *params,
                           vsc_sites **out, vsc_site_summary *rows)
{
    return hits_sites_entry(ctx, "vsc_pattern_hits_sites", kSitePattern, plain, plain ? (const void *)plain->storage.p : nullptr, bulged, n_guides,
                            params, out, rows);
}

uint64_t vsc_sites_count(const vsc_sites *sites) { return sites ? sites->n : 0; }
int vsc_sites_data(vsc_sites *sites, const vsc_site **out) { return record_list_data(sites, out); }
const void *vsc_sites_data_dev(const vsc_sites *sites) { return record_list_data_dev(sites); }
int vsc_sites_free(vsc_sites *sites) { return object_free(sites); }

int vsc_sites_collapse(const vsc_hit *plain, uint64_t n_plain, const vsc_bulge_hit *bulged, uint64_t n_bulged, uint32_t n_guides,
                       const vsc_site_params *params, vsc_site *sites, uint64_t capacity, uint64_t *n_sites, vsc_site_summary *rows)
{
    return sites_collapse_host<kSiteHit>(plain, n_plain, bulged, n_bulged, n_guides, params, sites, capacity, n_sites, rows);
}

int vsc_sites_collapse_pattern(const vsc_pattern_hit *plain, uint64_t n_plain, const vsc_bulge_hit *bulged, uint64_t n_bulged, uint32_t n_guides,
                               const vsc_site_params *params, vsc_site *sites, uint64_t capacity, uint64_t *n_sites, vsc_site_summary *rows)
{
    return sites_collapse_host<kSitePattern>(plain, n_plain, bulged, n_bulged, n_guides, params, sites, capacity, n_sites, rows);
}

int vsc_debug_sites_ms(const vsc_ctx *ctx, double *flag_scan_ms, double *write_ms)
{
    if (!ctx) return VSC_ERR_INVALID;
    if (flag_scan_ms) *flag_scan_ms = ctx->sites_ms[0];
    if (write_ms) *write_ms = ctx->sites_ms[1];
    return VSC_OK;
}

}  // extern "C"

// ---- table scores for bulged alignments and cut sites (the score: vsc_bulge_table.h; the kernels: vsc_bulge_table.hip) ----
namespace {

// the device copy of a bulge table: uploaded unless this context used this very table last
int resident_bulge_table(vsc_ctx *ctx, const vsc_bulge_table *table)
{
    if (ctx->bulge_table_serial == table->serial && ctx->bulge_table_buf.p) return VSC_OK;
    ctx->bulge_table_serial = 0;
    const size_t bytes = bulge_table_weights(table->shape) * sizeof(double);
    VSC_HIP(ctx, ctx->bulge_table_buf.ensure(bytes));
    VSC_HIP(ctx, hipMemcpyAsync(ctx->bulge_table_buf.p, table->w, bytes, hipMemcpyHostToDevice, ctx->stream));
    VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (the table may be freed when the call returns)
    ctx->bulge_table_serial = table->serial;
    return VSC_OK;
}

// What both device calls share: the checks of (genome, guides, len, table), the guides' words and planes, the table and the
// zeroed rows on the device.  The call's tables in ctx->site_table_tabs, 256-byte aligned parts:
// [guides: two uint4 each][rows][bounds: n_guides + 1 words][sel: a uint4 per guide]
struct BulgeTableCall {
    BulgeTableArgs a{};
    std::vector<uint4> host_guides;  // (outlives the asynchronous upload)
    size_t rows_at = 0, row_bytes = 0, bounds_at = 0, sel_at = 0;
};

int bulge_table_prepare(vsc_ctx *ctx, const char *who, const vsc_genome *genome, const char *guides, uint32_t n_guides, uint32_t len,
                        const vsc_bulge_table *table, bool want_rows, BulgeTableCall *call)
{
    if (genome->ctx != ctx) return fail_in(ctx, VSC_ERR_INVALID, who, "a genome of another context");
    if (table->shape.len != len) return fail_in(ctx, VSC_ERR_INVALID, who, "the table's len is not the call's");
    if (n_guides && !guides) return fail_in(ctx, VSC_ERR_INVALID, who, "null argument");
    call->host_guides.resize(2 * (size_t)n_guides);
    for (uint32_t g = 0; g < n_guides; ++g) {
        uint8_t sets[kPatMaxLen];
        if (!pattern_sets(guides + (size_t)g * len, len, sets)) return fail_in(ctx, VSC_ERR_INVALID, who, "a guide letter that is no IUPAC letter");
        const BulgeGuide b = bulge_table_guide(sets, len);
        call->host_guides[2 * (size_t)g] = make_uint4(b.gh, b.gl, b.single, 0u);
        call->host_guides[2 * (size_t)g + 1] = make_uint4(b.planes.a, b.planes.c, b.planes.g, b.planes.t);
    }
    VSC_HIP(ctx, hipSetDevice(ctx->device));
    const int trc = resident_bulge_table(ctx, table);
    if (trc != VSC_OK) return trc;
    const size_t guide_bytes = call->host_guides.size() * sizeof(uint4);
    call->rows_at = round256(guide_bytes);
    call->row_bytes = want_rows ? (size_t)n_guides * sizeof(vsc_guide_table_row) : 0;
    call->bounds_at = call->rows_at + round256(call->row_bytes);
    call->sel_at = call->bounds_at + round256(((size_t)n_guides + 1) * sizeof(uint32_t));
    VSC_HIP(ctx, ctx->site_table_tabs.ensure(call->sel_at + round256((size_t)n_guides * sizeof(uint4)) + 256));
    char *base = (char *)ctx->site_table_tabs.p;
    if (guide_bytes) VSC_HIP(ctx, hipMemcpyAsync(base, call->host_guides.data(), guide_bytes, hipMemcpyHostToDevice, ctx->stream));
    if (call->row_bytes) VSC_HIP(ctx, hipMemsetAsync(base + call->rows_at, 0, call->row_bytes, ctx->stream));
    BulgeTableArgs &a = call->a;
    // held_words: what the genome was loaded with (vsc_genome_load pads the device planes with kPadWords behind them); a
    // genome object without planes (genome_table_only) holds none, and every record scores 0 over it
    a.planes = BulgePlanes{genome->d_hi, genome->d_lo, (uint32_t)(genome->first_word * 32), genome->d_hi ? (uint32_t)genome->held_words : 0u,
                           genome->d_contig_off, genome->d_contig_end, genome->n_contigs};
    std::memcpy(&a.shape, &table->shape, sizeof a.shape);
    a.weights = (const double *)ctx->bulge_table_buf.p;
    a.guides = (const uint4 *)base;
    a.n_guides = n_guides;
    a.rows = call->row_bytes ? (unsigned long long *)(base + call->rows_at) : nullptr;
    return VSC_OK;
}

// Results from host arrays (tests: records of chosen lengths and records that no search returns)
template <class List, class Rec> int record_list_from_host(vsc_ctx *ctx, const Rec *records, uint64_t n, List **out)
{
    if (!out) return VSC_ERR_INVALID;
    *out = nullptr;
    if (!ctx || (n && !records)) return VSC_ERR_INVALID;
    return guarded(ctx, [&]() -> int {
    std::unique_ptr<List, int (*)(List *)> r(new List(), object_free<List>);
    r->ctx = ctx;
    r->n = n;
    if (n) {
        VSC_HIP(ctx, hipSetDevice(ctx->device));
        VSC_HIP(ctx, r->storage.ensure((size_t)n * sizeof(Rec)));
        VSC_HIP(ctx, hipMemcpyAsync(r->storage.p, records, (size_t)n * sizeof(Rec), hipMemcpyHostToDevice, ctx->stream));
        VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    *out = r.release();
    return VSC_OK;
    });
}

int stage_ms(vsc_ctx *ctx, int from, int to, double *out)
{
    float ms = 0;
    VSC_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev[from], ctx->ev[to]));
    *out = ms;
    return VSC_OK;
}

}  // namespace

extern "C" {

int vsc_bulge_table_build(const vsc_pattern_table *base, const double *dna, const double *rna, vsc_bulge_table **out)
{
    if (!out) return VSC_ERR_INVALID;
    *out = nullptr;
    if (!base || !dna || !rna) return VSC_ERR_INVALID;
    static std::atomic<uint64_t> serial{0};
    if (base->shape.ps_len < kPatBulgeMinProto) return VSC_ERR_INVALID;  // (before the weights are read: the shape sizes them)
    vsc_bulge_table *t = new (std::nothrow) vsc_bulge_table();
    if (!t) return VSC_ERR_NOMEM;
    t->shape = base->shape;
    const uint32_t n_base = pattern_table_weights(t->shape), rows = t->shape.ps_len * 4u;
    std::memcpy(t->w, base->w, n_base * sizeof(double));
    std::memcpy(t->w + bulge_table_dna_at(t->shape), dna, rows * sizeof(double));
    std::memcpy(t->w + bulge_table_rna_at(t->shape), rna, rows * sizeof(double));
    if (!bulge_table_valid(t->shape, t->w)) {  // a weight outside [0, 1], NaN included
        delete t;
        return VSC_ERR_INVALID;
    }
    for (uint32_t i = 0; i < bulge_table_weights(t->shape); ++i) t->zeros += t->w[i] == 0.0;
    t->serial = serial.fetch_add(1, std::memory_order_relaxed) + 1;
    *out = t;
    return VSC_OK;
}

int vsc_bulge_table_free(vsc_bulge_table *table)
{
    delete table;
    return VSC_OK;
}

int vsc_bulge_table_info(const vsc_bulge_table *table, vsc_bulge_table_stats *out)
{
    if (!table || !out) return VSC_ERR_INVALID;
    *out = vsc_bulge_table_stats{};
    out->serial = table->serial;
    out->zero_weights = table->zeros;
    std::memcpy(&out->shape, &table->shape, sizeof out->shape);
    return VSC_OK;
}

int vsc_bulge_table_score(const vsc_bulge_table *table, const char *guide, const char *site_text, int d, uint32_t *nm, uint32_t *index,
                          double *score, uint32_t *fixed)
{
    if (!table || !guide || !site_text || d < -2 || d > 2) return VSC_ERR_INVALID;
    const uint32_t len = table->shape.len;
    const int m = (int)len + d;
    if (m < (int)kPatMinLen || m > (int)kPatMaxLen) return VSC_ERR_INVALID;
    uint8_t sets[kPatMaxLen];
    if (!pattern_sets(guide, len, sets)) return VSC_ERR_INVALID;
    uint32_t sh = 0, sl = 0;
    for (int j = 0; j < m; ++j) {
        const int c = base_code(site_text[j]);
        if (c > 3) return VSC_ERR_INVALID;
        sh |= (uint32_t)(c >> 1) << j;
        sl |= (uint32_t)(c & 1) << j;
    }
    const BulgeGuide g = bulge_table_guide(sets, len);
    uint32_t n = 0, i = 0;
    double x;
    if (d == 0) {
        n = (uint32_t)__builtin_popcount(pattern_mismatch(sh, sl, g.planes));
        x = pattern_table_score(table->w, table->shape, g.gh, g.gl, g.single, sh, sl);
    } else {
        n = pattern_bulge_align(sh, sl, g.planes, table->shape.ps_start, table->shape.ps_start + table->shape.ps_len, d, &i);
        x = bulge_table_score(table->w, table->shape, g.gh, g.gl, g.single, sh, sl, d, i);
    }
    if (nm) *nm = n;
    if (index) *index = i;
    if (score) *score = x;
    if (fixed) *fixed = table_fixed(x);
    return VSC_OK;
}

int vsc_bulge_hits_table(vsc_ctx *ctx, const vsc_genome *genome, vsc_bulge_hits *hits, const char *guides, uint32_t n_guides, uint32_t len,
                         const vsc_bulge_table *table, uint32_t *fixed, vsc_guide_table_row *rows)
{
    const char *who = "vsc_bulge_hits_table";
    if (!ctx) return VSC_ERR_INVALID;
    return guarded(ctx, [&]() -> int {
    ctx->err.clear();
    if (!genome || !hits || !table) return fail_in(ctx, VSC_ERR_INVALID, who, "null argument");
    if (!fixed && !rows) return fail_in(ctx, VSC_ERR_INVALID, who, "neither scores nor rows are asked for");
    if (hits->ctx != ctx) return fail_in(ctx, VSC_ERR_INVALID, who, "a result of another context");
    if (hits->n > 0xFFFFFFFFull) return fail_in(ctx, VSC_ERR_RANGE, who, "more than 2^32 - 1 records");
    BulgeTableCall call;
    if (rows && n_guides) std::memset(rows, 0, (size_t)n_guides * sizeof(vsc_guide_table_row));
    if (table->shape.len != len) return fail_in(ctx, VSC_ERR_INVALID, who, "the table's len is not the call's");
    if (genome->ctx != ctx) return fail_in(ctx, VSC_ERR_INVALID, who, "a genome of another context");
    if (hits->n == 0) return VSC_OK;
    const int rc = bulge_table_prepare(ctx, who, genome, guides, n_guides, len, table, rows != nullptr, &call);
    if (rc != VSC_OK) return rc;
    BulgeTableArgs &a = call.a;
    a.n = (uint32_t)hits->n;
    a.hits = (const uint4 *)hits->storage.p;
    if (fixed) {
        VSC_HIP(ctx, ctx->site_table_scores.ensure((size_t)a.n * sizeof(uint32_t)));
        a.fixed = (uint32_t *)ctx->site_table_scores.p;
    }
    VSC_HIP(ctx, hipEventRecord(ctx->ev[kEvStageStart], ctx->stream));
    VSC_HIP(ctx, launch_bulge_table(a, ctx->n_cus, ctx->stream));
    VSC_HIP(ctx, hipEventRecord(ctx->ev[kEvStageEnd], ctx->stream));
    if (fixed) VSC_HIP(ctx, hipMemcpyAsync(fixed, a.fixed, (size_t)a.n * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (a.rows) VSC_HIP(ctx, hipMemcpyAsync(rows, a.rows, call.row_bytes, hipMemcpyDeviceToHost, ctx->stream));
    VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->site_table_ms[1] = ctx->site_table_ms[2] = 0;
    return stage_ms(ctx, kEvStageStart, kEvStageEnd, &ctx->site_table_ms[0]);
    });
}

int vsc_sites_table(vsc_ctx *ctx, const vsc_genome *genome, vsc_sites *sites, const vsc_site_params *params, const char *guides,
                    uint32_t n_guides, uint32_t len, const vsc_bulge_table *table, const vsc_pattern_select *select, vsc_sites **out,
                    vsc_guide_table_row *rows)
{
    const char *who = "vsc_sites_table";
    if (out) *out = nullptr;
    if (!ctx) return VSC_ERR_INVALID;
    return guarded(ctx, [&]() -> int {
    ctx->err.clear();
    if (!genome || !sites || !table) return fail_in(ctx, VSC_ERR_INVALID, who, "null argument");
    if (!out && !rows) return fail_in(ctx, VSC_ERR_INVALID, who, "neither records nor rows are asked for");
    if (site_params_check(params) != VSC_OK || params->len != len)
        return fail_in(ctx, VSC_ERR_INVALID, who, "params: len = the call's len, a known anchor and zeroed reserved fields are needed");
    if (select && (select->reserved[0] || select->reserved[1])) return fail_in(ctx, VSC_ERR_INVALID, who, "a non-zero reserved field of select");
    if (sites->ctx != ctx) return fail_in(ctx, VSC_ERR_INVALID, who, "a result of another context");
    if (table->shape.len != len) return fail_in(ctx, VSC_ERR_INVALID, who, "the table's len is not the call's");
    if (genome->ctx != ctx) return fail_in(ctx, VSC_ERR_INVALID, who, "a genome of another context");
    if (sites->n > 0xFFFFFFFFull) return fail_in(ctx, VSC_ERR_RANGE, who, "more than 2^32 - 1 sites");
    if (rows && n_guides) std::memset(rows, 0, (size_t)n_guides * sizeof(vsc_guide_table_row));
    std::unique_ptr<vsc_sites, int (*)(vsc_sites *)> res(nullptr, object_free<vsc_sites>);
    if (out) {
        res.reset(new (std::nothrow) vsc_sites());
        if (!res) return fail_in(ctx, VSC_ERR_NOMEM, who, "out of host memory");
        res->ctx = ctx;
        res->has_scores = true;
    }
    if (sites->n == 0) {
        if (out) *out = res.release();
        return VSC_OK;
    }
    BulgeTableCall call;
    const int rc = bulge_table_prepare(ctx, who, genome, guides, n_guides, len, table, rows != nullptr, &call);
    if (rc != VSC_OK) return rc;
    BulgeTableArgs &a = call.a;
    const uint32_t n = (uint32_t)sites->n;
    a.n = n;
    a.sites = (const uint4 *)sites->storage.p;
    a.anchor = params->anchor;
    const bool selects = out && select && (select->top_k || select->min_score);
    const size_t site_bytes = round256((size_t)n * sizeof(vsc_site));
    if (selects) {  // all the sites' scores go to scratch: the result is sized by the selection
        VSC_HIP(ctx, ctx->site_table_scores.ensure((size_t)n * sizeof(vsc_site_score)));
        a.scores = (uint4 *)ctx->site_table_scores.p;
    } else if (out) {  // every site stays: its record is copied, its scores are written where they stay
        VSC_HIP(ctx, res->storage.ensure(site_bytes + (size_t)n * sizeof(vsc_site_score)));
        res->n = n;
        res->scores_at = site_bytes;
        VSC_HIP(ctx, hipMemcpyAsync(res->storage.p, sites->storage.p, (size_t)n * sizeof(vsc_site), hipMemcpyDeviceToDevice, ctx->stream));
        a.scores = (uint4 *)((char *)res->storage.p + site_bytes);
    }
    ctx->site_table_ms[1] = ctx->site_table_ms[2] = 0;
    VSC_HIP(ctx, hipEventRecord(ctx->ev[kEvStageStart], ctx->stream));
    VSC_HIP(ctx, launch_site_table(a, ctx->n_cus, ctx->stream));
    VSC_HIP(ctx, hipEventRecord(ctx->ev[kEvStageEnd], ctx->stream));
    if (a.rows) VSC_HIP(ctx, hipMemcpyAsync(rows, a.rows, call.row_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (selects && n_guides) {
        char *base = (char *)ctx->site_table_tabs.p;
        SiteSelectArgs s{};
        s.sites = a.sites;
        s.scores = a.scores;
        s.n = n;
        s.n_guides = n_guides;
        s.bounds = (uint32_t *)(base + call.bounds_at);
        s.top_k = select->top_k;
        s.min_score = select->min_score;
        s.sel = (uint4 *)(base + call.sel_at);
        VSC_HIP(ctx, hipEventRecord(ctx->ev[kEvStage2Start], ctx->stream));
        VSC_HIP(ctx, launch_site_bounds(s, ctx->stream));
        VSC_HIP(ctx, launch_site_select(s, ctx->stream));
        VSC_HIP(ctx, hipEventRecord(ctx->ev[kEvStage2End], ctx->stream));
        // one read-back: every guide's survivors (they size the result)
        std::vector<uint4> sel(n_guides);
        VSC_HIP(ctx, hipMemcpyAsync(sel.data(), s.sel, (size_t)n_guides * sizeof(uint4), hipMemcpyDeviceToHost, ctx->stream));
        VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        unsigned long long kept = 0;
        for (const uint4 &q : sel) kept += (unsigned long long)q.w << 32 | q.z;
        if (kept > n) kept = n;  // (never, when the sites are in their order: segments of a list in another order may overlap)
        s.n_out = kept;
        if (kept) {
            const size_t kept_bytes = round256((size_t)kept * sizeof(vsc_site));
            VSC_HIP(ctx, res->storage.ensure(kept_bytes + (size_t)kept * sizeof(vsc_site_score)));
            res->n = kept;
            res->scores_at = kept_bytes;
            s.out_sites = (uint4 *)res->storage.p;
            s.out_scores = (uint4 *)((char *)res->storage.p + kept_bytes);
            VSC_HIP(ctx, hipEventRecord(ctx->ev[kEvSinkEnd], ctx->stream));
            VSC_HIP(ctx, launch_site_select_walk(s, ctx->stream));
            VSC_HIP(ctx, hipEventRecord(ctx->ev[kEvPrepEnd], ctx->stream));
        }
        VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        int trc = stage_ms(ctx, kEvStage2Start, kEvStage2End, &ctx->site_table_ms[1]);
        if (trc == VSC_OK && kept) trc = stage_ms(ctx, kEvSinkEnd, kEvPrepEnd, &ctx->site_table_ms[2]);
        if (trc != VSC_OK) return trc;
    } else {
        VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    const int trc = stage_ms(ctx, kEvStageStart, kEvStageEnd, &ctx->site_table_ms[0]);
    if (trc != VSC_OK) return trc;
    if (out) *out = res.release();
    return VSC_OK;
    });
}

int vsc_sites_scores(vsc_sites *sites, const vsc_site_score **out)
{
    if (!sites || !out || !sites->has_scores) return VSC_ERR_INVALID;
    return guarded(sites->ctx, [&]() -> int {
    if (!sites->scores_host_valid) {
        vsc_ctx *ctx = sites->ctx;
        sites->scores_host.resize(sites->n);
        if (sites->n) {
            VSC_HIP(ctx, hipSetDevice(ctx->device));
            VSC_HIP(ctx, hipMemcpyAsync(sites->scores_host.data(), (const char *)sites->storage.p + sites->scores_at,
                                        sites->n * sizeof(vsc_site_score), hipMemcpyDeviceToHost, ctx->stream));
            VSC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        }
        sites->scores_host_valid = true;
    }
    *out = sites->scores_host.data();
    return VSC_OK;
    });
}

const void *vsc_sites_scores_dev(const vsc_sites *sites)
{
    return sites && sites->has_scores && sites->n ? (const char *)sites->storage.p + sites->scores_at : nullptr;
}

int vsc_debug_bulge_hits_from_host(vsc_ctx *ctx, const vsc_bulge_hit *records, uint64_t n, vsc_bulge_hits **out)
{
    return record_list_from_host(ctx, records, n, out);
}

int vsc_debug_sites_from_host(vsc_ctx *ctx, const vsc_site *records, uint64_t n, vsc_sites **out)
{
    return record_list_from_host(ctx, records, n, out);
}

int vsc_debug_site_table_ms(const vsc_ctx *ctx, double *score_ms, double *select_ms, double *walk_ms)
{
    if (!ctx) return VSC_ERR_INVALID;
    if (score_ms) *score_ms = ctx->site_table_ms[0];
    if (select_ms) *select_ms = ctx->site_table_ms[1];
    if (walk_ms) *walk_ms = ctx->site_table_ms[2];
    return VSC_OK;
}

int vsc_debug_genome_from_contigs(vsc_ctx *ctx, const uint32_t *contig_off, uint32_t n_contigs, uint64_t span, vsc_genome **out)
{
    if (!ctx || !out) return VSC_ERR_INVALID;
    return guarded(ctx, [&]() -> int {
    *out = nullptr;
    if (!contig_off || n_contigs == 0 || n_contigs > (1u << 24) || span > (1ull << 32) || contig_off[n_contigs - 1] > span)
        return fail(ctx, VSC_ERR_INVALID, "vsc_debug_genome_from_contigs: bad contig table");
    std::vector<vsc_contig> table(n_contigs);
    for (uint32_t c = 0; c < n_contigs; ++c) {
        const uint64_t end = c + 1 < n_contigs ? contig_off[c + 1] : span;
        if (end < contig_off[c]) return fail(ctx, VSC_ERR_INVALID, "vsc_debug_genome_from_contigs: contig starts must ascend");
        table[c] = vsc_contig{contig_off[c], (uint32_t)std::min<uint64_t>(end - contig_off[c], 0xFFFFFFFFu), 0};
    }
    return genome_table_only(ctx, table.data(), n_contigs, out);
    });
}

// The record sink of a pass (sort_pass) over a hand-made PassFound: the caller's slots or pairs uploaded into the buffers
// the search would have left them in.
int vsc_debug_sort_records(vsc_ctx *ctx, vsc_genome *genome, const vsc_debug_sort_input *in, vsc_debug_sort_info *info, vsc_hits **out)
{
    if (!ctx || !out) return VSC_ERR_INVALID;
    return guarded(ctx, [&]() -> int {
    const char *const who = "vsc_debug_sort_records";
    *out = nullptr;
    if (!genome || !in || genome->ctx != ctx || !genome->d_contig_off || genome->n_contigs == 0) return fail_in(ctx, VSC_ERR_INVALID, who, "null argument");
    const bool scan = in->pair_keys != nullptr || in->pair_vals != nullptr || in->n_pairs != 0;
    if (scan && (in->slots || in->segments || in->n_slots || in->n_segments || in->fill)) return fail_in(ctx, VSC_ERR_INVALID, who, "both forms at once");
    if (in->pos_bits > 32 || in->read_bits > (uint32_t)kRegionBits || in->reserved || in->slots_allowed < -1 || in->slots_allowed > 1)
        return fail_in(ctx, VSC_ERR_INVALID, who, "bad position or read bits");
    PassFound f;
    f.max_mm = 0;  // (whose entry of the genome's "slots allowed" memory the call uses)
    uint64_t span = genome->h_contig_end.back() ? genome->h_contig_end.back() : (1ull << 32);  // (an end of 2^32 wrapped)
    span = std::max<uint64_t>(span, (uint64_t)genome->h_contig_off.back() + 1);
    const unsigned pos_bits = in->pos_bits ? in->pos_bits : std::max(1u, ceil_log2(span));
    f.pos_base = in->pos_bits ? in->pos_base : 0u;
    f.pos_pad = 32 - pos_bits;
    size_t fill_words = 0;
    if (scan) {
        if (!in->pair_keys || !in->pair_vals) return fail_in(ctx, VSC_ERR_INVALID, who, "null argument");
        if (in->n_regions < 1 || in->n_regions > (uint32_t)kParts || in->n_pairs >= (1ull << 32) || in->guide_base % kRegionReads ||
            (uint64_t)in->guide_base + (uint64_t)in->n_regions * kRegionReads > (1ull << 32))
            return fail_in(ctx, VSC_ERR_INVALID, who, "bad regions");
        for (uint64_t i = 0; i < in->n_pairs; ++i)
            if ((in->pair_keys[i] >> kRecKeyBits) >= in->n_regions) return fail_in(ctx, VSC_ERR_INVALID, who, "a key's read lies outside the regions");
        f.algo = VSC_ALGO_SCAN;
        f.n_parts = (int)in->n_regions;
        f.guide_base = in->guide_base;
        f.cap = std::max<uint64_t>(in->n_pairs, 1);
        f.n = in->n_pairs;
        f.key_bits = pos_bits + 1 + kRegionBits;
        if (f.n > 0) f.segs.push_back(SortSeg{0, 0, 0, (uint32_t)f.n, in->guide_base});
    } else {
        if ((in->n_slots && !in->slots) || (in->n_segments && !in->segments)) return fail_in(ctx, VSC_ERR_INVALID, who, "null argument");
        if (in->fill && (in->fill_shift < 6 || in->fill_shift > 13)) return fail_in(ctx, VSC_ERR_INVALID, who, "bad block size");
        const uint64_t block_mask = in->fill ? (1ull << in->fill_shift) - 1 : 0;
        for (uint32_t s = 0; s < in->n_segments; ++s) {
            const vsc_debug_sort_segment &g = in->segments[s];
            if (g.first_slot > in->n_slots || g.n_slots > in->n_slots - g.first_slot) return fail_in(ctx, VSC_ERR_INVALID, who, "a segment ends behind the slots");
            if (g.first_slot & block_mask) return fail_in(ctx, VSC_ERR_INVALID, who, "a segment off the block boundaries");
        }
        f.algo = VSC_ALGO_SEED;
        f.n_parts = (int)in->n_segments;
        f.cap = in->n_slots + kSortTile;
        f.key_bits = pos_bits + 1 + in->read_bits;
        for (uint32_t s = 0; s < in->n_segments; ++s) {
            const vsc_debug_sort_segment &g = in->segments[s];
            if (g.n_slots == 0) continue;
            // the records the sort will find: slots the fill table does not leave out and that hold no sentinel
            uint64_t real = 0;
            for (uint64_t i = g.first_slot; i < g.first_slot + g.n_slots; ++i)
                real += (!in->fill || (i & block_mask) < in->fill[i >> in->fill_shift]) && !(in->slots[i] >> 63);
            f.segs.push_back(SortSeg{g.first_slot, g.first_slot, f.n, g.n_slots, g.guide_base, s, 0});
            f.n += real;
        }
        if (in->fill) {
            fill_words = (size_t)((in->n_slots + block_mask) >> in->fill_shift);
            f.l1.fill_shift = in->fill_shift;
            f.l1.n_real = f.n;
        }
        if (in->slots_allowed >= 0) genome->sort_slots_ok[f.max_mm] = in->slots_allowed != 0;
    }
    VSC_HIP(ctx, hipSetDevice(ctx->device));
    VSC_HIP(ctx, hipEventRecord(ctx->ev[kEvPassStart], ctx->stream));
    VSC_HIP(ctx, ctx->keys_a.ensure(f.cap * sizeof(uint64_t)));
    if (scan) {
        VSC_HIP(ctx, ctx->vals_a.ensure(f.cap * sizeof(uint32_t)));
        if (f.n) {
            VSC_HIP(ctx, hipMemcpyAsync(ctx->keys_a.p, in->pair_keys, f.n * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
            VSC_HIP(ctx, hipMemcpyAsync(ctx->vals_a.p, in->pair_vals, f.n * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        }
    } else {
        if (in->n_slots) VSC_HIP(ctx, hipMemcpyAsync(ctx->keys_a.p, in->slots, in->n_slots * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
        if (fill_words) {
            VSC_HIP(ctx, ctx->seed_fill.ensure(fill_words * sizeof(uint32_t)));
            VSC_HIP(ctx, hipMemcpyAsync(ctx->seed_fill.p, in->fill, fill_words * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
            f.l1.fill = (const uint32_t *)ctx->seed_fill.p;
        }
    }
    VSC_HIP(ctx, hipEventRecord(ctx->ev[kEvSearchStart], ctx->stream));
    VSC_HIP(ctx, hipEventRecord(ctx->ev[kEvSearchEnd], ctx->stream));
    std::unique_ptr<vsc_hits, int (*)(vsc_hits *)> hits(new (std::nothrow) vsc_hits(), vsc_hits_free);
    if (!hits) return fail_in(ctx, VSC_ERR_NOMEM, who, "out of host memory");
    hits->ctx = ctx;
    vsc_timing t{};
    t.algorithm = (uint32_t)f.algo;
    t.hits = f.n;
    const int rc = sort_pass(ctx, genome, f, hits.get(), 0, 0, t);
    if (rc != VSC_OK) return rc;
    hits->n = f.n;
    if (f.n == 0) hits->host_valid = true;
    ctx->timing = t;
    if (info) {
        info->n = f.n;
        info->bytes = t.sort_bytes;
        info->levels = t.sort_levels;
        info->bin_bits = t.sort_bin_bits;
        info->slot_fallbacks = t.sort_fallbacks;
        info->slots_allowed = genome->sort_slots_ok[f.max_mm] ? 1u : 0u;
    }
    *out = hits.release();
    return VSC_OK;
    });
}

}  // extern "C"
