// pick_host.hpp - the -k, -b and -c options of guide_summary and pattern_search: the best K guides of every target, with
// spacing (include/varscot_hip.h "the best K guides per target"; tools/README.md).
//   -k K[,SPACING]     pick K guides (1 .. 32) per target, their cut sites at least SPACING bases apart (default 0: no spacing)
//   -b COLS            what to rank by, comma-separated, in priority order: mit, table, eff, oof, mh (default mit); needs -k
//   -c interval|name   the target is the interval (default), or all intervals with one BED name (4th column); needs -k
// The key of a candidate is made HERE, in one fixed quantisation, the columns packed most significant first:
//   mit / table  rint(100 x specificity), 14 bits        eff  the top 20 bits of the order-preserving bits of the predictor
//   oof          floor(1000 oof / sum), 10 bits, undefined -> 0        mh   min(sum, 2^20 - 1), 20 bits, undefined -> 0
// The guide listing gains the last columns pickTarget pickRank (NA NA for a guide that is not picked).  Host C++ only.
#pragma once

#include <cstring>
#include <fstream>
#include <map>
#include <sstream>
#include <vector>

#include "mh_host.hpp"

namespace vsc_host {

struct PickOptions {
    bool on = false, by_name = false;
    uint32_t k = 0, spacing = 0;
    std::vector<std::string> cols;
};

inline uint32_t pick_bits(const std::string &col) { return col == "mit" || col == "table" ? 14u : col == "oof" ? 10u : 20u; }

// "" and *o filled, or the message of a refusal.  needs: for every column the call cannot rank by, the option that would
// compute it (a column that is not in the map is available).
inline std::string parse_pick_options(bool k_set, const std::string &k, bool b_set, const std::string &b, bool c_set, const std::string &c,
                                      bool has_targets, const std::string &targets_flag, bool device_list,
                                      const std::map<std::string, std::string> &needs, PickOptions *o)
{
    if ((b_set || c_set) && !k_set) return std::string(b_set ? "-b" : "-c") + " belongs to the pick of -k: give -k";
    if (!k_set) return "";
    if (!has_targets) return "-k picks the best guides of every " + targets_flag + " target: give " + targets_flag;
    if (device_list) return "-k picks on one device: it does not combine with a device list";
    char *e = nullptr;
    const long kk = std::strtol(k.c_str(), &e, 10);
    long sp = 0;
    bool ok = e != k.c_str() && kk >= 1 && kk <= 32;
    if (ok && *e == ',') {
        const char *second = e + 1;
        sp = std::strtol(second, &e, 10);
        ok = e != second && sp >= 0 && sp <= 0xFFFFFFFFl;
    }
    if (!ok || *e) return "-k takes K[,SPACING]: 1 .. 32 guides per target, at least SPACING bases apart, not '" + k + "'";
    o->k = (uint32_t)kk;
    o->spacing = (uint32_t)sp;
    if (c_set && c != "interval" && c != "name") return "-c takes interval or name, not '" + c + "'";
    o->by_name = c_set && c == "name";
    std::istringstream is(b_set ? b : "mit");
    std::string col;
    uint32_t bits = 0;
    while (std::getline(is, col, ',')) {
        if (col != "mit" && col != "table" && col != "eff" && col != "oof" && col != "mh")
            return "-b takes columns out of mit, table, eff, oof, mh, not '" + col + "'";
        const auto it = needs.find(col);
        if (it != needs.end()) return "-b " + col + " ranks by a column this call does not compute: " + it->second;
        o->cols.push_back(col);
        bits += pick_bits(col);
    }
    if (o->cols.empty() || bits > 64) return "-b takes one to four columns that fit 64 bits, not '" + b + "'";
    o->on = true;
    return "";
}

// the order-preserving bits of an fp64: all bits of a negative flipped, the sign bit of the others; NaN -> 0
inline uint64_t order_bits(double v)
{
    if (std::isnan(v)) return 0;
    uint64_t b;
    std::memcpy(&b, &v, sizeof b);
    return b >> 63 ? ~b : b ^ (1ull << 63);
}

inline uint64_t pick_specificity(double spec) { return std::isnan(spec) || spec <= 0 ? 0 : (uint64_t)std::llrint(100.0 * spec); }

// what a call computed, per candidate; a pointer the chosen columns do not read may be null
struct PickColumns {
    const vsc_guide_summary *mit_rows = nullptr;
    const vsc_guide_table_row *table_rows = nullptr;
    const double *eff = nullptr;
    const uint32_t *pairs = nullptr;  // (sum, oof) per candidate
};

inline std::vector<uint64_t> pick_keys(const PickOptions &o, uint64_t n, const PickColumns &c)
{
    std::vector<uint64_t> key(n, 0);
    for (uint64_t i = 0; i < n; ++i)
        for (const std::string &col : o.cols) {
            uint64_t v = 0;
            if (col == "mit") v = pick_specificity(vsc_mit_specificity(c.mit_rows[i].mit_sum));
            else if (col == "table") v = pick_specificity(vsc_table_specificity(c.table_rows[i].score_sum));
            else if (col == "eff") v = order_bits(c.eff[i]) >> 44;
            else {
                const uint64_t sum = c.pairs[2 * i], oof = c.pairs[2 * i + 1];
                const bool undefined = sum == VSC_MH_UNDEFINED;
                if (col == "oof") v = undefined || sum == 0 ? 0 : 1000 * oof / sum;
                else v = undefined ? 0 : sum;
            }
            const uint32_t bits = pick_bits(col);
            const uint64_t top = (1ull << bits) - 1;
            key[i] = key[i] << bits | (v < top ? v : top);
        }
    return key;
}

// The targets of the intervals of a BED file, line by line as the tools read it.  -c interval: every interval is its own target,
// named by its 0-based line among the intervals (group stays empty).  -c name: the intervals with one 4th column are one target,
// numbered by first appearance; a line without a 4th column is refused.
inline void pick_targets(const PickOptions &o, const std::string &path, const std::string &flag, std::vector<uint32_t> *group,
                         std::vector<std::string> *names)
{
    std::ifstream bed(path);
    if (!bed) throw std::runtime_error("Could not open the " + flag + " file.");
    std::map<std::string, uint32_t> seen;
    std::string line;
    size_t n = 0;
    while (std::getline(bed, line)) {
        if (line.empty() || line[0] == '#' || line.compare(0, 5, "track") == 0 || line.compare(0, 7, "browser") == 0) continue;
        if (!o.by_name) {
            names->push_back(std::to_string(n++));
            continue;
        }
        std::istringstream is(line);
        std::string chr, start, stop, name;
        if (!(is >> chr >> start >> stop >> name)) throw std::runtime_error("-c name: the " + flag + " line '" + line + "' has no name column");
        const auto it = seen.emplace(name, (uint32_t)names->size());
        if (it.second) names->push_back(name);
        group->push_back(it.first->second);
    }
}

// "\tpickTarget\tpickRank" per candidate from the picks: the target's name and the 0-based rank, NA NA where it is not picked
inline std::vector<std::string> pick_text(const PickOptions &o, uint64_t n, const std::vector<std::string> &names, const std::vector<uint32_t> &picks,
                                          const std::vector<uint32_t> &counts)
{
    std::vector<std::string> out(n, "\tNA\tNA");
    for (size_t t = 0; t < counts.size(); ++t)
        for (uint32_t r = 0; r < counts[t]; ++r) {
            const uint32_t i = picks[t * o.k + r];
            if (i < n) out[i] = '\t' + names[t] + '\t' + std::to_string(r);
        }
    return out;
}

}  // namespace vsc_host
