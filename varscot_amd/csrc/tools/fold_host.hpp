// fold_host.hpp - the --fold, --fold-scaffold and --max-fold options of guide_summary and pattern_search: the self-complementarity
// of the guides that -E finds (include/varscot_hip.h "guide RNA self-complementarity"; tools/README.md).
//   --fold SpCas9 | Cas12a | SPEC   SpCas9: the preset for the 23-mer (spacer 0,20, stem 4, gc_min 2, min_loop 3, seed 8,12); Cas12a:
//                          the preset for a 27-mer (spacer 4,23, stem 4, gc_min 2, min_loop 3, seed 0,6) - or SPEC = SITELEN,PROTOSTART,
//                          PROTOLEN,STEM,GCMIN,MINLOOP,SEEDSTART,SEEDLEN,FLAGS: the shape's eight fields in that order and the flags
//   --fold-scaffold TEXT | @FILE   the constant part of the guide RNA, 5' to 3', at most 128 letters of A C G T U (a file: its
//                          letters, white space skipped); without it the scaffold is empty
//   --max-fold STARTS[,SELF[,SCAF[,SEED]]]   limits on starts, self_longest, scaf_longest and seed_paired, each 0 .. 32 or - for none
// With --max-fold the candidates are FILTERED before the off-target search.  Host C++ only.
#pragma once

#include <fstream>
#include <sstream>

#include "hdr_host.hpp"

namespace vsc_host {

struct FoldOptions {
    bool on = false, limited = false;
    vsc_fold_shape shape{};
    vsc_fold_limits limits{VSC_FOLD_NO_LIMIT, VSC_FOLD_NO_LIMIT, VSC_FOLD_NO_LIMIT, VSC_FOLD_NO_LIMIT};
    std::string scaffold;
};

// is s a shape SHAPE of the definition allows?  (the library's rule, so that the refusal comes before a device is opened)
inline bool fold_shape_ok(const vsc_fold_shape &s)
{
    if (s.site_len < 16 || s.site_len > 32 || s.proto_len < 12 || s.proto_len > 32 || s.proto_start > s.site_len || s.proto_len > s.site_len - s.proto_start)
        return false;
    if (s.stem < 3 || s.stem > 8 || s.gc_min > s.stem || s.min_loop > 16) return false;
    if (s.seed_start > 16 || s.seed_len > 16 || s.seed_start + s.seed_len > s.proto_len) return false;
    return s.flags <= 1 && !s.reserved[0] && !s.reserved[1] && !s.reserved[2];
}

// "" and *o filled, or the message of a refusal
inline std::string parse_fold_options(const Option &f, const Option &sc, const Option &mx, bool enumerating, bool several_devices, uint32_t site_len,
                                      FoldOptions *o)
{
    if ((sc.set || mx.set) && !f.set) return "--fold-scaffold and --max-fold belong to the shape of --fold: give --fold";
    if (!f.set) return "";
    if (!enumerating) return "--fold looks at the guides that -E finds: give -E";
    if (several_devices) return "--fold works on the candidates of one device: it does not combine with a device list";
    vsc_fold_shape s{};
    const std::string &p = f.value;
    if (p == "SpCas9" || p == "Cas12a") {
        const bool cas9 = p == "SpCas9";
        if (site_len != (cas9 ? 23u : 27u))
            return "--fold " + p + " is a preset for sites of " + (cas9 ? "23" : "27") + " bases: give the nine fields of a SPEC";
        s.site_len = site_len, s.stem = 4, s.gc_min = 2, s.min_loop = 3;
        if (cas9) s.proto_start = 0, s.proto_len = 20, s.seed_start = 8, s.seed_len = 12;
        else s.proto_start = 4, s.proto_len = 23, s.seed_start = 0, s.seed_len = 6;
    } else {
        std::vector<std::string> part;
        std::istringstream is(p);
        for (std::string t; std::getline(is, t, ',');) part.push_back(t);
        bool ok = part.size() == 9 && p.back() != ',';
        unsigned long v[9] = {};
        for (size_t k = 0; k < 9 && ok; ++k) {
            char *end = nullptr;
            ok = !part[k].empty() && part[k][0] >= '0' && part[k][0] <= '9';
            v[k] = ok ? std::strtoul(part[k].c_str(), &end, 10) : 0;
            ok = ok && *end == '\0' && v[k] <= 64;
        }
        if (ok) {
            s.site_len = (uint32_t)v[0], s.proto_start = (uint32_t)v[1], s.proto_len = (uint32_t)v[2], s.stem = (uint32_t)v[3], s.gc_min = (uint32_t)v[4];
            s.min_loop = (uint32_t)v[5], s.seed_start = (uint32_t)v[6], s.seed_len = (uint32_t)v[7], s.flags = (uint32_t)v[8];
            ok = s.site_len == site_len && fold_shape_ok(s);
        }
        if (!ok)
            return "--fold takes SpCas9, Cas12a or SITELEN,PROTOSTART,PROTOLEN,STEM,GCMIN,MINLOOP,SEEDSTART,SEEDLEN,FLAGS - a shape the definition "
                   "allows for sites of " + std::to_string(site_len) + " bases - not '" + p + "'";
    }
    std::string text;
    if (sc.set && !sc.value.empty() && sc.value[0] == '@') {
        std::ifstream in(sc.value.substr(1));
        if (!in) return "--fold-scaffold: cannot read '" + sc.value.substr(1) + "'";
        for (char c; in.get(c);)
            if (!std::isspace((unsigned char)c)) text.push_back(c);
    } else if (sc.set) {
        text = sc.value;
    }
    if (text.size() > 128) return "--fold-scaffold: a scaffold has at most 128 letters, not " + std::to_string(text.size());
    for (char c : text)
        if (!std::strchr("ACGTUacgtu", c) || !c) return std::string("--fold-scaffold: the letters are A C G T U, not '") + c + "'";
    if (mx.set) {
        std::vector<std::string> part;
        std::istringstream is(mx.value);
        for (std::string t; std::getline(is, t, ',');) part.push_back(t);
        bool ok = !part.empty() && part.size() <= 4 && mx.value.back() != ',';
        uint32_t *const to[4] = {&o->limits.max_starts, &o->limits.max_self_longest, &o->limits.max_scaf_longest, &o->limits.max_seed_paired};
        for (size_t k = 0; k < part.size() && ok; ++k) {
            if (part[k] == "-") continue;
            char *end = nullptr;
            ok = !part[k].empty() && part[k][0] >= '0' && part[k][0] <= '9';
            const unsigned long v = ok ? std::strtoul(part[k].c_str(), &end, 10) : 0;
            ok = ok && *end == '\0' && v <= 32;
            if (ok) *to[k] = (uint32_t)v;
        }
        if (!ok) return "--max-fold takes STARTS[,SELF[,SCAF[,SEED]]]: each 0 .. 32 or - for no limit, not '" + mx.value + "'";
        o->limited = true;
    }
    o->on = true;
    o->shape = s;
    o->scaffold = text;
    return "";
}

// "\tfoldStarts\tfoldSelf\tfoldScaffold\tfoldSeed" of a row, NA where it is undefined
inline std::string fold_columns(const uint32_t *row)
{
    if (row[0] == VSC_FOLD_UNDEFINED && row[1] == VSC_FOLD_UNDEFINED) return "\tNA\tNA\tNA\tNA";
    return '\t' + std::to_string(row[0] & 0xFFu) + '\t' + std::to_string(row[1] & 0xFFu) + '\t' + std::to_string((row[1] >> 8) & 0xFFu) + '\t' +
           std::to_string(row[0] >> 24);
}

}  // namespace vsc_host
