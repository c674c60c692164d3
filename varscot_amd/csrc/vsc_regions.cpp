// vsc_regions.cpp - the interval sets of include/varscot_hip.h (vsc_regions_*): validation, global coordinates, the sorted
// starts with the running maximum of the ends, and the coarse class table.  Host C++ only, no device call: the membership
// test itself is vsc::regions_contains (vsc_internal.h), which the summary and selection kernels share.  The label structure
// (which interval: vsc_regions_locate) is built here as well; its lookup is vsc::regions_locate (vsc_enum.h).
#include <algorithm>
#include <atomic>
#include <new>
#include <utility>
#include <vector>

#include "vsc_enum.h"
#include "vsc_internal.h"
#include "vsc_objects.h"

using namespace vsc;

namespace {

std::atomic<uint64_t> g_serial{0};

// The window starts that are in the regions, as ascending disjoint ranges [first, second): interval [s, e) takes in the starts
// [s - 22, e) under OVERLAP and [s, e - 22) under INSIDE (none if it is shorter than a window).  Starts of the first kind that
// fall before the interval's contig belong to windows no contig holds; vsc::regions_contains never asks the table about them.
std::vector<std::pair<uint64_t, uint64_t>> member_ranges(const std::vector<std::pair<uint32_t, uint32_t>> &iv, uint32_t rule)
{
    std::vector<std::pair<uint64_t, uint64_t>> out;
    for (const auto &i : iv) {  // ascending starts, so the ranges' starts ascend as well
        uint64_t a, b;
        if (rule == VSC_REGION_INSIDE) {
            if (i.second - i.first < (uint32_t)VSC_READ_LEN) continue;
            a = i.first;
            b = (uint64_t)i.second - (VSC_READ_LEN - 1);
        } else {
            a = i.first >= (uint32_t)(VSC_READ_LEN - 1) ? i.first - (uint32_t)(VSC_READ_LEN - 1) : 0u;
            b = i.second;
        }
        if (!out.empty() && a <= out.back().second) out.back().second = std::max(out.back().second, b);
        else out.emplace_back(a, b);
    }
    return out;
}

}  // namespace

extern "C" {

int vsc_regions_build(const vsc_contig *contigs, uint32_t n_contigs, const vsc_interval *iv, uint64_t n, uint32_t rule, vsc_regions **out)
{
    if (!out) return VSC_ERR_INVALID;
    *out = nullptr;
    if ((n_contigs && !contigs) || (n && !iv) || rule > VSC_REGION_INSIDE) return VSC_ERR_INVALID;
    try {
        vsc_regions *r = new vsc_regions();
        struct Guard {
            vsc_regions *p;
            ~Guard() { delete p; }
        } guard{r};
        uint64_t total = 0;  // positions of the genome: the end of its last contig
        for (uint32_t c = 0; c < n_contigs; ++c) {
            const uint64_t end = contigs[c].offset + contigs[c].length;
            if (end >= (1ull << 32)) return VSC_ERR_RANGE;
            r->contig_off.push_back((uint32_t)contigs[c].offset);
            r->contig_len.push_back(contigs[c].length);
            total = std::max(total, end);
        }
        std::vector<std::pair<uint32_t, uint32_t>> g;  // global [start, end)
        g.reserve(n);
        struct Numbered {
            uint32_t start, end, index;
        };
        std::vector<Numbered> byspec;  // the same intervals with their place in iv[] (labels are 32-bit: not beyond 0xFFFFFFFE)
        const bool numbered = n <= 0xFFFFFFFEull;
        if (numbered) byspec.reserve(n);
        for (uint64_t i = 0; i < n; ++i) {
            const vsc_interval &v = iv[i];
            if (v.contig >= n_contigs || v.start > v.end || v.reserved) return VSC_ERR_INVALID;
            const uint32_t end = std::min(v.end, r->contig_len[v.contig]);
            if (v.start >= end) continue;  // empty, or beyond the contig
            g.emplace_back(r->contig_off[v.contig] + v.start, r->contig_off[v.contig] + end);
            if (numbered) byspec.push_back(Numbered{g.back().first, g.back().second, (uint32_t)i});
        }
        std::sort(g.begin(), g.end());
        r->start.resize(g.size());
        r->end_max.resize(g.size());
        uint32_t run = 0;
        for (size_t i = 0; i < g.size(); ++i) {
            run = std::max(run, g[i].second);
            r->start[i] = g[i].first;
            r->end_max[i] = run;
        }
        r->rule = rule;
        r->n_input = n;
        // the label structure, eagerly (the object is immutable and shared between threads): of the intervals before a bound on
        // the start, the last one in this order whose end is large enough is the most specific one - largest start, smallest end,
        // lowest input index.  up[k] = the previous entry with a greater end, by a monotonic stack: the entries between it and k
        // end no later than k does, so a walk that finds end[k] too small skips them
        if (numbered) {
            std::sort(byspec.begin(), byspec.end(), [](const Numbered &a, const Numbered &b) {
                if (a.start != b.start) return a.start < b.start;
                if (a.end != b.end) return a.end > b.end;
                return a.index > b.index;
            });
            const size_t m = byspec.size();
            r->loc_end.resize(m);
            r->loc_index.resize(m);
            r->loc_up.resize(m);
            std::vector<uint32_t> stack;  // entries whose ends strictly decrease
            for (size_t k = 0; k < m; ++k) {
                r->loc_end[k] = byspec[k].end;
                r->loc_index[k] = byspec[k].index;
                while (!stack.empty() && r->loc_end[stack.back()] <= byspec[k].end) stack.pop_back();
                r->loc_up[k] = stack.empty() ? kLocateNone : stack.back();
                stack.push_back((uint32_t)k);
            }
            r->has_locate = true;
        }
        // the class table: the smallest blocks that keep it within kRegMaxBlocks
        uint32_t shift = kRegMinBlockShift;
        while (((total + (1ull << shift) - 1) >> shift) > kRegMaxBlocks) ++shift;
        r->block_shift = shift;
        r->n_blocks = (uint32_t)((total + (1ull << shift) - 1) >> shift);
        r->cls.assign(((size_t)r->n_blocks + 15) / 16 + 1, 0);  // (kRegOut = 0; never empty: a device copy has an address)
        auto set_cls = [&](uint64_t b, uint32_t c) {
            uint32_t &w = r->cls[b >> 4];
            w = (w & ~(3u << (2 * (b & 15)))) | (c << (2 * (b & 15)));
        };
        const uint64_t bsize = 1ull << shift;
        for (const auto &m : member_ranges(g, rule)) {
            const uint64_t a = m.first, b = std::min<uint64_t>(m.second, total);
            if (a >= b) continue;
            const uint64_t first = a >> shift, last = (b - 1) >> shift;
            for (uint64_t k = first; k <= last; ++k) {
                const bool whole = a <= k * bsize && (k + 1) * bsize <= b;
                set_cls(k, whole ? kRegIn : kRegMixed);  // (ranges are disjoint: a block one of them fills meets no other)
            }
        }
        vsc_regions_stats &st = r->stats;
        st.intervals = g.size();
        st.rule = rule;
        st.block_bases = (uint32_t)bsize;
        for (uint32_t b = 0; b < r->n_blocks; ++b) {
            const uint32_t c = (r->cls[b >> 4] >> (2 * (b & 15))) & 3u;
            (c == kRegOut ? st.blocks_out : c == kRegIn ? st.blocks_in : st.blocks_mixed)++;
        }
        r->serial = g_serial.fetch_add(1, std::memory_order_relaxed) + 1;
        guard.p = nullptr;
        *out = r;
        return VSC_OK;
    } catch (const std::bad_alloc &) {
        return VSC_ERR_NOMEM;
    } catch (...) {
        return VSC_ERR_INVALID;
    }
}

void vsc_regions_free(vsc_regions *r) { delete r; }

int vsc_regions_contains(const vsc_regions *r, uint32_t contig, uint32_t pos)
{
    if (!r || contig >= r->contig_len.size() || pos >= r->contig_len[contig]) return 0;
    const uint32_t left = r->contig_len[contig] - pos;  // a window at the contig's end is cut off there
    return regions_contains(r->view(), r->contig_off[contig] + pos, std::min<uint32_t>(left, VSC_READ_LEN)) ? 1 : 0;
}

uint32_t vsc_regions_locate(const vsc_regions *r, uint32_t contig, uint32_t pos)
{
    if (!r || !r->has_locate || contig >= r->contig_len.size() || pos >= r->contig_len[contig]) return VSC_REGION_NONE;
    const uint32_t left = r->contig_len[contig] - pos;  // a window at the contig's end is cut off there, as in vsc_regions_contains
    const uint32_t len = std::min<uint32_t>(left, VSC_READ_LEN), g = r->contig_off[contig] + pos;
    const RegionsView v = r->view();
    if (len == (uint32_t)VSC_READ_LEN) {  // (the table describes whole windows)
        const uint32_t b = g >> v.block_shift;
        if (b >= v.n_blocks || ((v.cls[b >> 4] >> (2u * (b & 15u))) & 3u) == kRegOut) return VSC_REGION_NONE;
    }
    return regions_locate(v, LocateView{r->loc_end.data(), r->loc_index.data(), r->loc_up.data()}, g, len);
}

int vsc_regions_info(const vsc_regions *r, vsc_regions_stats *out)
{
    if (!r || !out) return VSC_ERR_INVALID;
    *out = r->stats;
    return VSC_OK;
}

}  // extern "C"
