// edit_host.hpp - the -x, -z, -l and -o options of guide_summary and pattern_search: the base-editor windows of the guides that
// -E finds and their join with target bases (include/varscot_hip.h "base-editor guide design"; tools/README.md).
//   -x EDITOR    CBE (window 3,5 base C) | ABE (window 3,4 base A) - two common published windows of the SpCas9 23-mer and
//                nothing more - or START,LEN,BASE: the window in read positions of the site and the base the editor converts
//   -z FILE      the target bases (.bed, one base per line: chrom start start+1); needs -x
//   -l MIN,MAX   keep only the candidates with MIN .. MAX editable bases in the window; needs -x
//   -o FILE      the listing of the (target, guide) pairs; needs -z
// With -z or -l the candidates are FILTERED before the off-target search (FILTER of the definition: a defined site, the bounds
// - 0,16 when -l is not given - and, with -z, a hit).  Host C++ only.
#pragma once

#include <algorithm>
#include <cctype>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>

#include "eff_model_host.hpp"

namespace vsc_host {

struct EditOptions {
    bool on = false, filtered = false, with_targets = false, with_pairs = false;
    vsc_edit_shape shape{};
    uint32_t min_editable = 0, max_editable = 16;
    std::string targets_path, pairs_path;
};

// "" and *o filled, or the message of a refusal
inline std::string parse_edit_options(bool x_set, const std::string &x, bool z_set, const std::string &z, bool l_set, const std::string &l,
                                      bool o_set, const std::string &out, bool enumerating, bool several_devices, uint32_t site_len,
                                      EditOptions *o)
{
    if ((z_set || l_set || o_set) && !x_set) return "-z, -l and -o belong to the editor of -x: give -x";
    if (!x_set) return "";
    if (!enumerating) return "-x looks at the guides that -E finds: give -E";
    if (several_devices) return "-x works on the candidates of one device: it does not combine with a device list";
    if (o_set && !z_set) return "-o lists the pairs of guides and target bases: give -z";
    uint32_t start = 0, len = 0, base = 4;
    if (x == "CBE" || x == "ABE") {
        if (site_len != (uint32_t)VSC_READ_LEN) return "-x " + x + " is a preset for sites of 23 bases: give START,LEN,BASE";
        start = 3;
        len = x == "CBE" ? 5 : 4;
        base = x == "CBE" ? 1 : 0;
    } else {
        char *e = nullptr;
        const long a = std::strtol(x.c_str(), &e, 10);
        bool ok = e != x.c_str() && *e == ',';
        long b = 0;
        if (ok) {
            const char *second = e + 1;
            b = std::strtol(second, &e, 10);
            ok = e != second && *e == ',' && e[1] && !e[2];
        }
        if (ok) {
            const char *p = std::strchr("ACGT", std::toupper((unsigned char)e[1]));
            ok = p && a >= 0 && b >= 1 && b <= 16 && a + b <= (long)site_len;
            if (ok) start = (uint32_t)a, len = (uint32_t)b, base = (uint32_t)(p - "ACGT");
        }
        if (!ok)
            return "-x takes CBE, ABE or START,LEN,BASE: a window of 1 .. 16 read positions inside the " + std::to_string(site_len) +
                   " bases of the site and one of A C G T, not '" + x + "'";
    }
    o->on = true;
    o->shape = vsc_edit_shape{site_len, start, len, base, {0, 0, 0, 0}};
    if (l_set) {
        char *e = nullptr;
        const long a = std::strtol(l.c_str(), &e, 10);
        bool ok = e != l.c_str() && *e == ',';
        long b = 0;
        if (ok) {
            const char *second = e + 1;
            b = std::strtol(second, &e, 10);
            ok = e != second && !*e && a >= 0 && a <= b && b <= 16;
        }
        if (!ok) return "-l takes MIN,MAX: the editable bases of the window, 0 <= MIN <= MAX <= 16, not '" + l + "'";
        o->min_editable = (uint32_t)a;
        o->max_editable = (uint32_t)b;
    }
    o->with_targets = z_set;
    o->with_pairs = o_set;
    o->filtered = z_set || l_set;
    o->targets_path = z;
    o->pairs_path = out;
    return "";
}

// The -z file: BED, one base per line; chrom = first word of a contig name.  Sorted by (contig, pos), duplicates dropped: what
// the library takes, and a target's index is its place here.
inline std::vector<vsc_edit_target> read_edit_targets(const std::string &path, const std::vector<std::string> &names)
{
    std::map<std::string, uint32_t> by_chrom;
    for (size_t c = names.size(); c-- > 0;) by_chrom[names[c].substr(0, names[c].find_first_of(" \t"))] = (uint32_t)c;
    std::ifstream bed(path);
    if (!bed) throw std::runtime_error("Could not open the -z file.");
    std::vector<vsc_edit_target> t;
    std::string line;
    while (std::getline(bed, line)) {
        if (line.empty() || line[0] == '#' || line.compare(0, 5, "track") == 0 || line.compare(0, 7, "browser") == 0) continue;
        std::istringstream is(line);
        std::string chr;
        unsigned long long start = 0, stop = 0;
        if (!(is >> chr >> start >> stop)) throw std::runtime_error("-z: not a BED line: '" + line + "'");
        auto it = by_chrom.find(chr);
        if (it == by_chrom.end()) throw std::runtime_error("-z: no sequence '" + chr + "' in the genome");
        if (stop != start + 1 || stop > 0xFFFFFFFFull) throw std::runtime_error("-z: a target is one base per line, not '" + line + "'");
        t.push_back(vsc_edit_target{it->second, (uint32_t)start});
    }
    std::sort(t.begin(), t.end(), [](const vsc_edit_target &a, const vsc_edit_target &b) { return a.contig != b.contig ? a.contig < b.contig : a.pos < b.pos; });
    t.erase(std::unique(t.begin(), t.end(), [](const vsc_edit_target &a, const vsc_edit_target &b) { return a.contig == b.contig && a.pos == b.pos; }),
            t.end());
    return t;
}

// "\teditWindow\teditable\ttargetsHit" of a candidate: the window's read letters out of the site's (read orientation), the number
// of editable bases and of target bases among them; NA three times where the row is undefined
inline std::string edit_columns(const vsc_edit_shape &s, const std::string &site, const uint32_t *row)
{
    if (row[0] == VSC_EDIT_UNDEFINED) return "\tNA\tNA\tNA";
    return '\t' + site.substr(s.win_start, s.win_len) + '\t' + std::to_string(__builtin_popcount(row[0])) + '\t' +
           std::to_string(__builtin_popcount(row[1]));
}

// the -o file: one line per pair in the library's order - ascending (guide, target)
inline void write_edit_pairs(const std::string &path, const std::vector<vsc_edit_pair> &pairs, const std::vector<vsc_edit_target> &targets,
                             const std::vector<std::string> &names, const std::vector<std::string> &ids)
{
    std::ofstream out(path);
    if (!out.is_open()) throw std::runtime_error("Could not open the -o path.");
    out << "#chrom\tpos\tguideId\tat\tbystanders\n";
    for (const vsc_edit_pair &p : pairs) {
        const vsc_edit_target &t = targets.at(p.target);
        const std::string &name = names.at(t.contig);
        out << name.substr(0, name.find_first_of(" \t")) << '\t' << t.pos << '\t' << ids.at(p.candidate) << '\t' << (p.info & 0xFFu) << '\t'
            << (p.info >> 8) << '\n';
    }
    out.close();
    if (!out) throw std::runtime_error("Could not write the -o file.");
}

// Rows and - with targets - pairs of the candidates where they lie: edit(rows, pairs, capacity, &n_pairs) is the library call
template <class Call>
inline void edit_rows_and_pairs(const EditOptions &o, uint64_t n, Call edit, std::vector<uint32_t> *rows, std::vector<vsc_edit_pair> *pairs)
{
    rows->assign(2 * n, 0u);
    pairs->clear();
    uint64_t n_pairs = 0;
    edit(rows->data(), (vsc_edit_pair *)nullptr, (uint64_t)0, &n_pairs);  // the rows; the pairs are counted
    if (o.with_pairs && n_pairs) {
        pairs->resize(n_pairs);
        edit((uint32_t *)nullptr, pairs->data(), n_pairs, &n_pairs);
    }
}

}  // namespace vsc_host
