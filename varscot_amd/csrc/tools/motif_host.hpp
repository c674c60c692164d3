// motif_host.hpp - the --motifs options of guide_summary and pattern_search: restriction sites and IUPAC motifs in the guides that
// -E finds (include/varscot_hip.h "restriction sites and IUPAC motifs"; tools/README.md).
//   --motifs FILE              a TSV, one motif per line: name, IUPAC text of 2 .. 16 letters, 1 or 2 (strands); 1 .. 63 lines; '#'
//                              starts a comment line
//   --motif-left TEXT / --motif-right TEXT   the vector's text on either side of the cloned spacer, at most 16 letters of A C G T U
//   --motif-forbid NAMES       drop the candidates whose construct holds one of these motifs (names of the file, comma separated)
//   --motif-forbid-context NAMES   ... whose genomic context holds one
//   --motif-require-cut NAMES  keep the candidates with one of these motifs over the cut zone; --motif-cut-only: and nowhere else
//   --motifs-out FILE          one line per candidate: guide id, then the names per mask (construct, cut, elsewhere, cut-only)
// The site is the candidates' (23 bases: the SpCas9 shape 0,20 / 16,2; 27 bases: the Cas12a shape 4,23 / 21,6; another length is
// refused) with 16 bases of context a side; a candidate closer than that to its contig's end has no context: NA, and a limit
// drops it.  With a limit the candidates are FILTERED before the off-target search.  Host C++ only.
#pragma once

#include <fstream>
#include <sstream>

#include "fold_host.hpp"

namespace vsc_host {

struct MotifOptions {
    bool on = false, limited = false;
    vsc_motif_shape shape{};
    vsc_motif_limits limits{};
    std::vector<vsc_motif> motifs;
    std::vector<std::string> names;
    std::string left, right, out_path;
};

// the accept set of an IUPAC letter is not empty (the library's rule, so that the refusal comes before a device is opened)
inline bool motif_iupac_ok(char c) { return c && std::strchr("ACGTURYSWKMBDHVNacgturyswkmbdhvn", c); }

// names -> a mask over o.names; "" or the message of a refusal
inline std::string motif_mask_of(const std::string &opt, const std::string &list, const MotifOptions &o, uint64_t *mask)
{
    *mask = 0;
    std::istringstream is(list);
    for (std::string t; std::getline(is, t, ',');) {
        size_t m = 0;
        while (m < o.names.size() && o.names[m] != t) ++m;
        if (m == o.names.size()) return opt + ": '" + t + "' is no motif of --motifs";
        *mask |= 1ull << m;
    }
    if (!*mask) return opt + " takes the names of motifs, comma separated";
    return "";
}

// "" and *o filled, or the message of a refusal
inline std::string parse_motif_options(const Option &file, const Option &left, const Option &right, const Option &forbid, const Option &forbid_ctx,
                                       const Option &require, const Option &cut_only, const Option &out, bool enumerating, bool several_devices,
                                       uint32_t site_len, MotifOptions *o)
{
    if ((left.set || right.set || forbid.set || forbid_ctx.set || require.set || cut_only.set || out.set) && !file.set)
        return "--motif-left, --motif-right, --motif-forbid, --motif-forbid-context, --motif-require-cut, --motif-cut-only and --motifs-out belong to "
               "the motifs of --motifs: give --motifs";
    if (!file.set) return "";
    if (!enumerating) return "--motifs looks at the guides that -E finds: give -E";
    if (several_devices) return "--motifs works on the candidates of one device: it does not combine with a device list";
    if (site_len != 23u && site_len != 27u) return "--motifs knows the shapes of sites of 23 (SpCas9) and 27 (Cas12a) bases, not of " + std::to_string(site_len);
    if (cut_only.set && !require.set) return "--motif-cut-only belongs to --motif-require-cut";
    vsc_motif_shape s{};
    s.site_len = site_len, s.up = 16, s.down = 16;
    if (site_len == 23u) s.proto_start = 0, s.proto_len = 20, s.cut_start = 16, s.cut_len = 2;
    else s.proto_start = 4, s.proto_len = 23, s.cut_start = 21, s.cut_len = 6;
    std::ifstream in(file.value);
    if (!in) return "--motifs: cannot read '" + file.value + "'";
    for (std::string line; std::getline(in, line);) {
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.empty() || line[0] == '#') continue;
        std::vector<std::string> part;
        std::istringstream is(line);
        for (std::string t; std::getline(is, t, '\t');) part.push_back(t);
        if (part.size() != 3 || part[0].empty() || (part[2] != "1" && part[2] != "2"))
            return "--motifs: a line is name, IUPAC text, 1 or 2 (tab separated), not '" + line + "'";
        if (part[0].find(',') != std::string::npos) return "--motifs: a name holds no comma: '" + part[0] + "'";
        for (const std::string &n : o->names)
            if (n == part[0]) return "--motifs: the name '" + part[0] + "' occurs twice";
        const std::string &text = part[1];
        if (text.size() < 2 || text.size() > 16) return "--motifs: a motif has 2 .. 16 letters, not '" + text + "'";
        bool all_n = true;
        for (char c : text) {
            if (!motif_iupac_ok(c)) return "--motifs: the letters are IUPAC letters, not '" + text + "'";
            all_n = all_n && (c == 'N' || c == 'n');
        }
        if (all_n) return "--motifs: a motif of N alone matches everywhere: '" + text + "'";
        vsc_motif m{};
        std::memcpy(m.text, text.data(), text.size());
        m.len = (uint32_t)text.size();
        m.flags = part[2] == "2" ? VSC_MOTIF_BOTH_STRANDS : 0u;
        o->motifs.push_back(m);
        o->names.push_back(part[0]);
        if (o->motifs.size() > 63) return "--motifs: at most 63 motifs a call";
    }
    if (o->motifs.empty()) return "--motifs: '" + file.value + "' holds no motif";
    for (const Option *f : {&left, &right}) {
        if (!f->set) continue;
        if (f->value.size() > 16) return std::string("--") + f->long_name + ": a flank has at most 16 letters, not " + std::to_string(f->value.size());
        for (char c : f->value)
            if (!c || !std::strchr("ACGTUacgtu", c)) return std::string("--") + f->long_name + ": the letters are A C G T U, not '" + c + "'";
    }
    o->left = left.set ? left.value : "";
    o->right = right.set ? right.value : "";
    const struct {
        const Option *opt;
        const char *name;
        uint64_t *mask;
    } masks[3] = {{&forbid, "--motif-forbid", &o->limits.forbid_construct},
                  {&forbid_ctx, "--motif-forbid-context", &o->limits.forbid_context},
                  {&require, "--motif-require-cut", &o->limits.require_cut}};
    for (const auto &m : masks) {
        if (!m.opt->set) continue;
        const std::string why = motif_mask_of(m.name, m.opt->value, *o, m.mask);
        if (!why.empty()) return why;
        o->limited = true;
    }
    o->limits.flags = cut_only.set ? VSC_MOTIF_CUT_ONLY : 0u;
    o->out_path = out.set ? out.value : "";
    o->shape = s;
    o->on = true;
    return "";
}

// the names of the set bits of a mask, comma separated; "-" for none
inline std::string motif_names(const MotifOptions &o, uint64_t mask)
{
    std::string s;
    for (size_t m = 0; m < o.names.size(); ++m)
        if ((mask >> m) & 1u) s += (s.empty() ? "" : ",") + o.names[m];
    return s.empty() ? "-" : s;
}

// "\tmotifsConstruct\tmotifsCut\tmotifsElsewhere\tmotifsCutOnly" of a row, NA where it is undefined
inline std::string motif_columns(const MotifOptions &o, const uint64_t *row)
{
    if (row[0] == VSC_MOTIF_UNDEFINED && row[1] == VSC_MOTIF_UNDEFINED && row[2] == VSC_MOTIF_UNDEFINED) return "\tNA\tNA\tNA\tNA";
    return '\t' + motif_names(o, row[0]) + '\t' + motif_names(o, row[1]) + '\t' + motif_names(o, row[2]) + '\t' + motif_names(o, row[1] & ~row[2]);
}

// --motifs-out: "#guideId construct cut elsewhere cutOnly", the names per mask, one line per candidate
inline void write_motifs(const MotifOptions &o, const std::vector<uint64_t> &rows, const std::vector<std::string> &ids)
{
    std::ofstream out(o.out_path);
    if (!out.is_open()) throw std::runtime_error("Could not open the --motifs-out path.");
    out << "#guideId\tconstruct\tcut\telsewhere\tcutOnly\n";
    for (size_t i = 0; i < ids.size(); ++i) out << ids[i] << motif_columns(o, &rows[3 * i]) << '\n';
    out.close();
    if (!out) throw std::runtime_error("Could not write the --motifs-out file.");
}

}  // namespace vsc_host
