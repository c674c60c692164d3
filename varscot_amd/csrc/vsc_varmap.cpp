// vsc_varmap.cpp - the variant map of include/varscot_hip.h (vsc_variant_map_*): every window id of a window genome parsed once
// into the tables the merge kernel reads (vsc_varmap.h), the shadow regions of the reference side, and the host's answer for
// one window position.  Host C++ only, no device call.  The parsing follows split_id / snp_type of tools/merge_host.hpp, i.e.
// filterSnpAlignment and getSnpType (variant_processing/filter_output_bam.h:189-317).
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <unordered_map>
#include <vector>

#include <algorithm>

#include "vsc_pattern_variants.h"

using namespace vsc;

namespace {

std::atomic<uint64_t> g_serial{0};

// atoi = (int) strtol (tools/merge_host.hpp c_atoi)
int c_atoi(const std::string &s) { return (int)std::strtol(s.c_str(), nullptr, 10); }

uint32_t intern(std::unordered_map<std::string, uint32_t> &table, const std::string &s)
{
    return table.emplace(s, (uint32_t)table.size()).first->second;
}

}  // namespace

extern "C" {

int vsc_variant_map_build(const char *ids, const uint64_t *id_offsets, const vsc_contig *window_contigs, uint32_t n_windows,
                          const vsc_contig *ref_contigs, const char *const *ref_names, uint32_t n_ref_contigs, vsc_variant_map **out)
{
    if (!out) return VSC_ERR_INVALID;
    *out = nullptr;
    if ((n_windows && (!ids || !id_offsets || !window_contigs)) || (n_ref_contigs && (!ref_contigs || !ref_names))) return VSC_ERR_INVALID;
    try {
        vsc_variant_map *m = new vsc_variant_map();
        struct Guard {
            vsc_variant_map *p;
            ~Guard() { delete p; }
        } guard{m};
        std::unordered_map<std::string, uint32_t> by_chrom, chr_ids, tag_ids;
        for (uint32_t c = 0; c < n_ref_contigs; ++c) {  // the first word of the name, the first contig of that name (an FAI index)
            if (!ref_names[c]) return VSC_ERR_INVALID;
            if (ref_contigs[c].offset + ref_contigs[c].length >= (1ull << 32)) return VSC_ERR_RANGE;
            const std::string name(ref_names[c]);
            by_chrom.emplace(name.substr(0, name.find_first_of(" \t")), c);
            m->ref_contigs.push_back(ref_contigs[c]);
        }
        m->win.reserve((size_t)n_windows + 1);
        m->win_len.reserve(n_windows);
        m->text_off.push_back(0);
        std::vector<std::string> f;
        for (uint32_t w = 0; w < n_windows; ++w) {
            if (id_offsets[w + 1] <= id_offsets[w]) return VSC_ERR_INVALID;  // (an id and the byte behind it)
            const std::string id(ids + id_offsets[w], (size_t)(id_offsets[w + 1] - id_offsets[w] - 1));
            f.clear();
            for (size_t b = 0;;) {  // split_id
                const size_t e = id.find('_', b);
                f.push_back(id.substr(b, e == std::string::npos ? std::string::npos : e - b));
                if (e == std::string::npos) break;
                b = e + 1;
            }
            VarWindow vw{};
            const auto it = by_chrom.find(f[0]);
            vw.contig = it == by_chrom.end() ? UINT32_MAX : it->second;
            vw.start = (uint32_t)(f.size() > 1 ? c_atoi(f[1]) : 0);
            vw.var_off = (uint32_t)m->var.size();
            vw.chr_id = intern(chr_ids, f[0]);
            if (vw.chr_id == m->chr_names.size()) m->chr_names.push_back(f[0]);
            if (vw.contig == UINT32_MAX) ++m->stats.unknown_chr;
            uint32_t count = 0;
            for (size_t k = 3; k + 2 < f.size(); k += 3, ++count) {
                if (m->var.size() >= 0xFFFFFFFEull || m->text.size() + f[k].size() >= 0xFFFFFFFEull) return VSC_ERR_RANGE;
                m->var.push_back(VarEntry{c_atoi(f[k]), (uint32_t)f[k + 1].size(), (uint32_t)f[k + 2].size(), intern(tag_ids, f[0] + '_' + f[k])});
                m->text += f[k];
                m->text_off.push_back((uint32_t)m->text.size());
            }
            if (count > m->stats.max_variants) m->stats.max_variants = count;
            m->win.push_back(vw);
            m->win_len.push_back(window_contigs[w].length);
        }
        m->win.push_back(VarWindow{UINT32_MAX, 0u, (uint32_t)m->var.size(), UINT32_MAX});
        // the shadow intervals as vsc_variant_map_shadow hands them to vsc_regions_build: cut at the contig's end, sorted
        std::vector<std::pair<uint32_t, uint32_t>> iv;
        for (uint32_t w = 0; w < n_windows; ++w) {
            const VarWindow &vw = m->win[w];
            if (vw.contig == UINT32_MAX || (int32_t)vw.start < 0) continue;
            const vsc_contig &rc = m->ref_contigs[vw.contig];
            const uint64_t end = std::min<uint64_t>((uint64_t)vw.start + m->win_len[w], rc.length);
            if (vw.start >= end) continue;
            iv.emplace_back((uint32_t)(rc.offset + vw.start), (uint32_t)(rc.offset + end));
        }
        std::sort(iv.begin(), iv.end());
        uint32_t run = 0;
        for (const auto &i : iv) {
            run = std::max(run, i.second);
            m->shadow_start.push_back(i.first);
            m->shadow_end_max.push_back(run);
        }
        m->stats.windows = n_windows;
        m->stats.variants = m->var.size();
        m->serial = g_serial.fetch_add(1, std::memory_order_relaxed) + 1;
        guard.p = nullptr;
        *out = m;
        return VSC_OK;
    } catch (const std::bad_alloc &) {
        return VSC_ERR_NOMEM;
    } catch (...) {
        return VSC_ERR_INVALID;
    }
}

void vsc_variant_map_free(vsc_variant_map *map) { delete map; }

int vsc_variant_map_info(const vsc_variant_map *map, vsc_variant_map_stats *out)
{
    if (!map || !out) return VSC_ERR_INVALID;
    *out = map->stats;
    return VSC_OK;
}

int vsc_variant_map_shadow(const vsc_variant_map *map, vsc_regions **out)
{
    if (!out) return VSC_ERR_INVALID;
    *out = nullptr;
    if (!map) return VSC_ERR_INVALID;
    try {
        std::vector<vsc_interval> iv;
        for (size_t w = 0; w + 1 < map->win.size(); ++w) {
            const VarWindow &vw = map->win[w];
            if (vw.contig == UINT32_MAX || (int32_t)vw.start < 0) continue;  // (WindowIndex: a negative start shadows nothing)
            const uint64_t end = (uint64_t)vw.start + map->win_len[w];
            iv.push_back(vsc_interval{vw.contig, vw.start, (uint32_t)(end < 0xFFFFFFFFull ? end : 0xFFFFFFFFull), 0u});
        }
        return vsc_regions_build(map->ref_contigs.data(), (uint32_t)map->ref_contigs.size(), iv.data(), iv.size(), VSC_REGION_INSIDE, out);
    } catch (const std::bad_alloc &) {
        return VSC_ERR_NOMEM;
    }
}

int vsc_variant_map_locate(const vsc_variant_map *map, uint32_t window, uint32_t pos, vsc_variant_label *label)
{
    return vsc_variant_map_locate_len(map, window, pos, VSC_READ_LEN, label);
}

int vsc_variant_map_locate_len(const vsc_variant_map *map, uint32_t window, uint32_t pos, uint32_t len, vsc_variant_label *label)
{
    if (!map || !label || (size_t)window + 1 >= map->win.size() || len < kPatVarMinLen || len > kPatVarMaxLen) return VSC_ERR_INVALID;
    uint32_t pos2, n_var;
    varmap_walk(map->view(), window, pos, len, &pos2, &n_var);
    *label = vsc_variant_label{map->win[window].contig, pos2, n_var, n_var ? VSC_VARIANT_VAR : 0u};
    return VSC_OK;
}

int vsc_variant_map_shadows(const vsc_variant_map *map, uint32_t ref_contig, uint32_t pos, uint32_t len)
{
    if (!map || ref_contig >= map->ref_contigs.size() || len < kPatVarMinLen || len > kPatVarMaxLen) return VSC_ERR_INVALID;
    const vsc_contig &rc = map->ref_contigs[ref_contig];
    if (rc.length < len || pos > rc.length - len) return 0;  // (no site of len bases starts there)
    return shadow_search(map->shadow_start.data(), map->shadow_end_max.data(), (uint32_t)map->shadow_start.size(),
                         (uint32_t)(rc.offset + pos), len) ? 1 : 0;
}

int64_t vsc_variant_map_tag(const vsc_variant_map *map, uint32_t window, uint32_t pos, char *buf, size_t len)
{
    return vsc_variant_map_tag_len(map, window, pos, VSC_READ_LEN, buf, len);
}

int64_t vsc_variant_map_tag_len(const vsc_variant_map *map, uint32_t window, uint32_t pos, uint32_t site_len, char *buf, size_t len)
{
    if (!map || (len && !buf) || (size_t)window + 1 >= map->win.size() || site_len < kPatVarMinLen || site_len > kPatVarMaxLen)
        return VSC_ERR_INVALID;
    try {
        const VarMapView v = map->view();
        const uint32_t pos1 = pos + v.win[window].start;
        std::string tag;
        uint32_t b, e;
        var_range(v, window, &b, &e);
        for (uint32_t k = b; k < e; ++k)
            if (var_covered(v.var[k], pos1, site_len)) {
                tag += tag.empty() ? "VAR_" + map->chr_names[v.win[window].chr_id] + "_" : std::string(",");
                tag.append(map->text, map->text_off[k], map->text_off[k + 1] - map->text_off[k]);
            }
        if (tag.empty()) tag = "REF";
        if (len) {
            const size_t n = tag.size() < len - 1 ? tag.size() : len - 1;
            std::memcpy(buf, tag.data(), n);
            buf[n] = 0;
        }
        return (int64_t)tag.size();
    } catch (const std::bad_alloc &) {
        return VSC_ERR_NOMEM;
    }
}

}  // extern "C"
