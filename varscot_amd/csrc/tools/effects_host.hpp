// effects_host.hpp - the --cds, --edit-to, --effect-filter and --effects options of guide_summary and pattern_search: the coding
// consequences of the base editor of -x in the guides that -E finds (include/varscot_hip.h "coding consequences of base edits";
// tools/README.md).
//   -d, --cds FILE                     the coding segments (.bed, BED6: chrom start end name score strand; name = the transcript,
//                                      score = the segment's phase 0 .. 2, strand + or -); sorted here; needs -x
//   -2, --edit-to BASE                 the base the editor writes on the read strand (default: the transition partner of the
//                                      base of -x: C -> T, A -> G, G -> A, T -> C); needs --cds
//   -f, --effect-filter REQUIRE[/FORBID]  class names joined by +: keep only the candidates with an effect of a REQUIRE class
//                                      (empty: no requirement) and none of a FORBID class; needs --cds
//   -Q, --effects FILE                 the listing of the effects; needs --cds
// d, f and Q were the letters still free in both tools; no fourth one is, so --edit-to has a digit.  With --effect-filter the
// candidates are FILTERED before the off-target search, after the editor's own filter.  Host C++ only.
#pragma once

#include <algorithm>
#include <cctype>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>

#include "edit_host.hpp"

namespace vsc_host {

inline const char *const *effect_class_names()
{
    static const char *const names[VSC_EFFECT_CLASSES] = {"synonymous", "missense", "stop_gained", "stop_lost", "start_lost", "unknown"};
    return names;
}

struct EffectsOptions {
    bool on = false, filtered = false, with_listing = false;
    uint32_t to = 0, require = 0, forbid = 0;
    std::string cds_path, effects_path;
};

// the mask of class names joined by +; false: a word that is no class
inline bool parse_effect_classes(const std::string &text, uint32_t *mask)
{
    *mask = 0;
    size_t at = 0;
    while (at <= text.size() && !text.empty()) {
        const size_t end = std::min(text.find('+', at), text.size());
        const std::string word = text.substr(at, end - at);
        uint32_t k = 0;
        while (k < VSC_EFFECT_CLASSES && word != effect_class_names()[k]) ++k;
        if (k == VSC_EFFECT_CLASSES) return false;
        *mask |= 1u << k;
        at = end + 1;
    }
    return true;
}

// "" and *o filled, or the message of a refusal; edit: what parse_edit_options left
inline std::string parse_effects_options(bool d_set, const std::string &d, bool t_set, const std::string &t, bool f_set, const std::string &f,
                                         bool q_set, const std::string &q, const EditOptions &edit, EffectsOptions *o)
{
    if (!(d_set || t_set || f_set || q_set)) return "";
    if (!edit.on) return "--cds, --edit-to, --effect-filter and --effects belong to the editor of -x: give -x";
    if (!d_set) return "--edit-to, --effect-filter and --effects look at the coding segments: give --cds";
    o->to = (edit.shape.from + 2u) % 4u;
    if (t_set) {
        const char *p = t.size() == 1 ? std::strchr("ACGT", std::toupper((unsigned char)t[0])) : nullptr;
        if (!p || !*p || (uint32_t)(p - "ACGT") == edit.shape.from)
            return "--edit-to takes one of A C G T other than the base of -x, not '" + t + "'";
        o->to = (uint32_t)(p - "ACGT");
    }
    if (f_set) {
        const size_t slash = f.find('/');
        const std::string require = f.substr(0, slash), forbid = slash == std::string::npos ? "" : f.substr(slash + 1);
        if (!parse_effect_classes(require, &o->require) || !parse_effect_classes(forbid, &o->forbid) || (o->require | o->forbid) == 0)
            return "--effect-filter takes REQUIRE[/FORBID], class names joined by + out of synonymous missense stop_gained stop_lost "
                   "start_lost unknown, not '" + f + "'";
        o->filtered = true;
    }
    o->on = true;
    o->with_listing = q_set;
    o->cds_path = d;
    o->effects_path = q;
    return "";
}

// A vsc_cds and the names of its transcripts; freed with the object.
struct CdsOfFile {
    vsc_cds *cds = nullptr;
    std::vector<std::string> transcripts;
    CdsOfFile() = default;
    CdsOfFile(const CdsOfFile &) = delete;
    CdsOfFile &operator=(const CdsOfFile &) = delete;
    ~CdsOfFile() { vsc_cds_free(cds); }
};

// The --cds file: BED6; chrom = first word of a contig name, name = the transcript, score = the phase.  Sorted by (contig,
// start) here; a transcript's index is its place among the names in the order the sorted segments meet them.  Everything else
// - overlaps, two strands in a transcript, phases that do not continue the frame - is vsc_cds_build's to refuse.
inline void read_cds(const std::string &path, const std::vector<std::string> &names, const std::vector<vsc_contig> &contigs, CdsOfFile *out)
{
    std::map<std::string, uint32_t> by_chrom;
    for (size_t c = names.size(); c-- > 0;) by_chrom[names[c].substr(0, names[c].find_first_of(" \t"))] = (uint32_t)c;
    std::ifstream bed(path);
    if (!bed) throw std::runtime_error("Could not open the --cds file.");
    struct Line {
        vsc_cds_segment s;
        std::string transcript;
    };
    std::vector<Line> lines;
    std::string line;
    while (std::getline(bed, line)) {
        if (line.empty() || line[0] == '#' || line.compare(0, 5, "track") == 0 || line.compare(0, 7, "browser") == 0) continue;
        std::istringstream is(line);
        std::string chr, name, strand;
        unsigned long long start = 0, stop = 0;
        long long phase = 0;
        if (!(is >> chr >> start >> stop >> name >> phase >> strand)) throw std::runtime_error("--cds: not a BED6 line: '" + line + "'");
        auto it = by_chrom.find(chr);
        if (it == by_chrom.end()) throw std::runtime_error("--cds: no sequence '" + chr + "' in the genome");
        if (stop > 0xFFFFFFFFull || start > stop || phase < 0 || phase > 2 || (strand != "+" && strand != "-"))
            throw std::runtime_error("--cds: a segment is chrom start end transcript phase (0 .. 2) strand (+ or -), not '" + line + "'");
        lines.push_back(Line{vsc_cds_segment{it->second, (uint32_t)start, (uint32_t)stop, 0u, strand == "-" ? 1u : 0u, (uint32_t)phase, {0, 0}}, name});
    }
    std::stable_sort(lines.begin(), lines.end(),
                     [](const Line &a, const Line &b) { return a.s.contig != b.s.contig ? a.s.contig < b.s.contig : a.s.start < b.s.start; });
    std::map<std::string, uint32_t> index;
    std::vector<vsc_cds_segment> segments;
    for (Line &l : lines) {
        auto it = index.find(l.transcript);
        if (it == index.end()) {
            it = index.emplace(l.transcript, (uint32_t)out->transcripts.size()).first;
            out->transcripts.push_back(l.transcript);
        }
        l.s.transcript = it->second;
        segments.push_back(l.s);
    }
    if (vsc_cds_build(contigs.data(), (uint32_t)contigs.size(), segments.data(), segments.size(), (uint32_t)out->transcripts.size(), &out->cds) != VSC_OK)
        throw std::runtime_error(std::string("--cds: ") + vsc_cds_build_error() + " (segments in (chrom, start) order)");
}

// "\tcodingEdits\tstopGained\tmissense\tsynonymous" of a candidate: the editable bases that lie in a segment and its effects
// of three classes; NA four times where the row is undefined
inline std::string effects_columns(const uint32_t *row)
{
    if (row[0] == VSC_EFFECTS_UNDEFINED && row[1] == VSC_EFFECTS_UNDEFINED) return "\tNA\tNA\tNA\tNA";
    auto field = [&](uint32_t k) { return std::to_string(row[0] >> (5u * k) & 31u); };
    return '\t' + std::to_string(__builtin_popcount(row[1])) + '\t' + field(VSC_EFFECT_STOP_GAINED) + '\t' + field(VSC_EFFECT_MISSENSE) + '\t' +
           field(VSC_EFFECT_SYNONYMOUS);
}

inline std::string codon_letters(uint32_t c) { return std::string{"ACGT"[c >> 4 & 3u], "ACGT"[c >> 2 & 3u], "ACGT"[c & 3u]}; }

// the --effects file: one line per effect in the library's order; the codon is its 0-based index in the transcript, ref and alt
// are letters in transcript orientation (NA for an unknown codon), at the window position of the first edited base
inline void write_effects(const std::string &path, const std::vector<vsc_effect> &effects, const std::vector<std::string> &transcripts,
                          const std::vector<std::string> &ids)
{
    static const char code[] = "KNKNTTTTRSRSIIMIQHQHPPPPRRRRLLLLEDEDAAAAGGGGVVVV*Y*YSSSS*CWCLFLF";
    std::ofstream out(path);
    if (!out.is_open()) throw std::runtime_error("Could not open the --effects path.");
    out << "#guideId\ttranscript\tcodon\tref\talt\trefAA\taltAA\tclass\tat\n";
    for (const vsc_effect &e : effects) {
        const uint32_t ref = e.info & 63u, alt = e.info >> 6 & 63u, cls = e.info >> 12 & 7u;
        out << ids.at(e.candidate) << '\t' << transcripts.at(e.transcript) << '\t' << e.codon << '\t';
        if (cls == VSC_EFFECT_UNKNOWN) out << "NA\tNA\tNA\tNA";
        else out << codon_letters(ref) << '\t' << codon_letters(alt) << '\t' << code[ref] << '\t' << code[alt];
        out << '\t' << (cls < VSC_EFFECT_CLASSES ? effect_class_names()[cls] : "NA") << '\t' << (e.info >> 20 & 15u) << '\n';
    }
    out.close();
    if (!out) throw std::runtime_error("Could not write the --effects file.");
}

// Rows and - with --effects - records of the candidates where they lie: call(rows, effects, capacity, &n_effects) is the library call
template <class Call>
inline void effects_rows_and_records(const EffectsOptions &o, uint64_t n, Call call, std::vector<uint32_t> *rows, std::vector<vsc_effect> *effects)
{
    rows->assign(2 * n, 0u);
    effects->clear();
    uint64_t count = 0;
    call(rows->data(), (vsc_effect *)nullptr, (uint64_t)0, &count);  // the rows; the effects are counted
    if (o.with_listing && count) {
        effects->resize(count);
        call((uint32_t *)nullptr, effects->data(), count, &count);
    }
}

}  // namespace vsc_host
