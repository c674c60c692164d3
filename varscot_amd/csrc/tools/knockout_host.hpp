// knockout_host.hpp - the --knockout options of guide_summary and pattern_search: where the cut of every guide that -E finds falls
// in the coding sequence, and what a frameshift there does (include/varscot_hip.h "knock-out design"; tools/README.md).
//   --knockout [CUT]           the break lies between read positions CUT - 1 and CUT of the site, 1 .. site_len - 1 (default: 17 for
//                              sites of 23 bases, the SpCas9 cut; 22 for sites of 27, the Cas12a TTTV cut; another length needs CUT)
//   --knockout-cds FILE        the coding segments, as --cds reads them (BED6: chrom start end transcript phase strand)
//   --knockout-nmd WINDOW[,START]   a premature stop triggers nonsense-mediated decay when it ends at least WINDOW coding bases in front
//                              of the last exon-exon junction (default 50) and begins at least START coding bases behind the first
//                              one (default 0: the rule is off); each 0 .. 65535
//   --knockout-filter MINPCT,MAXPCT[,EDGE[,REQUIRE[/FORBID]]]   keep the coding cuts between MINPCT and MAXPCT per cent of the protein
//                              (decimals allowed; a lower bound is rounded up and an upper one down to the row's 1/65536), at least
//                              EDGE (0 .. 255) bases from either end of the exon, with every REQUIRE flag and no FORBID flag: names
//                              joined by + out of first last ptc1 ptc2 nmd1 nmd2 unknown
//   --knockout-out FILE        one line per candidate: guide id, the eight columns of the listing, the flags by name
// Long options only: no short letter is free in both tools.  With --knockout-filter the candidates are FILTERED before the
// off-target search, after every other filter.  Host C++ only.
#pragma once

#include <cmath>
#include <cstdlib>
#include <fstream>
#include <sstream>

#include "effects_host.hpp"

namespace vsc_host {

inline const char *const *knockout_flag_names()
{
    static const char *const names[7] = {"first", "last", "ptc1", "ptc2", "nmd1", "nmd2", "unknown"};
    return names;
}

struct KnockoutOptions {
    bool on = false, filtered = false;
    vsc_knockout_shape shape{};
    vsc_knockout_limits limits{};
    std::string cds_path, out_path;
};

// the mask of flag names joined by +; false: a word that is no flag
inline bool parse_knockout_flags(const std::string &text, uint32_t *mask)
{
    *mask = 0;
    size_t at = 0;
    while (at <= text.size() && !text.empty()) {
        const size_t end = std::min(text.find('+', at), text.size());
        const std::string word = text.substr(at, end - at);
        uint32_t k = 0;
        while (k < 7u && word != knockout_flag_names()[k]) ++k;
        if (k == 7u) return false;
        *mask |= 1u << k;
        at = end + 1;
    }
    return true;
}

// a whole number 0 .. max, all of the text
inline bool knockout_number(const std::string &text, unsigned long max, uint32_t *out)
{
    if (text.empty() || text.find_first_not_of("0123456789") != std::string::npos || text.size() > 9) return false;
    const unsigned long v = std::strtoul(text.c_str(), nullptr, 10);
    if (v > max) return false;
    *out = (uint32_t)v;
    return true;
}

// a share in per cent, 0 .. 100, as the row's frac: a lower bound rounded up, an upper one down, capped at 65535
inline bool knockout_percent(const std::string &text, bool upper, uint32_t *out)
{
    if (text.empty() || text.find_first_not_of("0123456789.") != std::string::npos) return false;
    char *end = nullptr;
    const double pct = std::strtod(text.c_str(), &end);
    if (!end || *end || !(pct >= 0.0 && pct <= 100.0)) return false;
    const double units = 65536.0 * pct / 100.0;
    const double v = upper ? std::floor(units) : std::ceil(units);
    *out = v > 65535.0 ? 65535u : (uint32_t)v;
    return true;
}

// "" and *o filled, or the message of a refusal
inline std::string parse_knockout_options(const Option &ko, const Option &cds, const Option &nmd, const Option &filter, const Option &out,
                                          bool enumerating, bool several_devices, uint32_t site_len, KnockoutOptions *o)
{
    if ((cds.set || nmd.set || filter.set || out.set) && !ko.set)
        return "--knockout-cds, --knockout-nmd, --knockout-filter and --knockout-out belong to the cut of --knockout: give --knockout";
    if (!ko.set) return "";
    if (!enumerating) return "--knockout looks at the guides that -E finds: give -E";
    if (several_devices) return "--knockout works on the candidates of one device: it does not combine with a device list";
    if (!cds.set) return "--knockout looks at the coding segments: give --knockout-cds";
    if (site_len < 16u || site_len > 32u) return "--knockout takes sites of 16 .. 32 bases, not of " + std::to_string(site_len);
    vsc_knockout_shape s{};
    s.site_len = site_len, s.nmd_window = 50, s.start_window = 0, s.max_codons = 4096;
    if (ko.value.empty()) {
        if (site_len != 23u && site_len != 27u)
            return "--knockout knows the cut of sites of 23 (SpCas9: 17) and 27 (Cas12a: 22) bases; give --knockout CUT for " + std::to_string(site_len);
        s.cut = site_len == 23u ? 17u : 22u;
    } else if (!knockout_number(ko.value, site_len - 1u, &s.cut) || s.cut < 1u) {
        return "--knockout takes a cut of 1 .. " + std::to_string(site_len - 1u) + ", not '" + ko.value + "'";
    }
    if (nmd.set) {
        const size_t comma = nmd.value.find(',');
        if (!knockout_number(nmd.value.substr(0, comma), 65535ul, &s.nmd_window) ||
            (comma != std::string::npos && !knockout_number(nmd.value.substr(comma + 1), 65535ul, &s.start_window)))
            return "--knockout-nmd takes WINDOW[,START], each 0 .. 65535, not '" + nmd.value + "'";
    }
    vsc_knockout_limits lim{};
    lim.max_frac = 65535;
    if (filter.set) {
        std::vector<std::string> part;
        std::istringstream is(filter.value);
        for (std::string t; std::getline(is, t, ',');) part.push_back(t);
        const char *const rule = "--knockout-filter takes MINPCT,MAXPCT[,EDGE[,REQUIRE[/FORBID]]]: per cent 0 .. 100 with MINPCT <= MAXPCT, EDGE 0 .. 255, "
                                 "flag names joined by + out of first last ptc1 ptc2 nmd1 nmd2 unknown, not '";
        if (part.size() < 2 || part.size() > 4 || !knockout_percent(part[0], false, &lim.min_frac) || !knockout_percent(part[1], true, &lim.max_frac) ||
            lim.min_frac > lim.max_frac || (part.size() > 2 && !knockout_number(part[2], 255ul, &lim.min_edge)))
            return rule + filter.value + "'";
        if (part.size() > 3) {
            const size_t slash = part[3].find('/');
            if (!parse_knockout_flags(part[3].substr(0, slash), &lim.require) ||
                !parse_knockout_flags(slash == std::string::npos ? "" : part[3].substr(slash + 1), &lim.forbid) || (lim.require | lim.forbid) == 0)
                return rule + filter.value + "'";
        }
        o->filtered = true;
    }
    o->shape = s;
    o->limits = lim;
    o->cds_path = cds.value;
    o->out_path = out.set ? out.value : "";
    o->on = true;
    return "";
}

inline const char *knockout_header() { return "\tkoTranscript\tkoCodon\tkoFrame\tkoCutPct\tkoEdge\tkoPtc1\tkoPtc2\tkoNmd"; }

// d_s as text: the codons to the first stop, or END / CAP / NA (unknown)
inline std::string knockout_distance(uint32_t d)
{
    return d == VSC_KNOCKOUT_END ? "END" : d == VSC_KNOCKOUT_CAP ? "CAP" : d == VSC_KNOCKOUT_UNKNOWN ? "NA" : std::to_string(d);
}

// the eight columns of a row: NA where it is undefined; "-" (or "junction") and "-" seven times where the cut is no coding cut;
// koCutPct = 100 frac / 65536 with one decimal, koNmd = the frames with NMD: - 1 2 1+2
inline std::string knockout_columns(const uint32_t *row, const std::vector<std::string> &transcripts)
{
    if (row[0] == VSC_KNOCKOUT_UNDEFINED && row[1] == VSC_KNOCKOUT_UNDEFINED && row[2] == VSC_KNOCKOUT_UNDEFINED && row[3] == VSC_KNOCKOUT_UNDEFINED)
        return "\tNA\tNA\tNA\tNA\tNA\tNA\tNA\tNA";
    if (row[0] == 0xFFFFFFFFu) return std::string(row[2] >> 31 ? "\tjunction" : "\t-") + "\t-\t-\t-\t-\t-\t-\t-";
    const uint32_t flags = row[2] >> 24, tenths = (uint32_t)(((uint64_t)(row[2] & 0xFFFFu) * 1000u) >> 16);
    const bool n1 = flags & VSC_KNOCKOUT_NMD1, n2 = flags & VSC_KNOCKOUT_NMD2;
    return '\t' + (row[0] < transcripts.size() ? transcripts[row[0]] : std::to_string(row[0])) + '\t' + std::to_string(row[1] & 0x3FFFFFFFu) + '\t' +
           std::to_string(row[1] >> 30) + '\t' + std::to_string(tenths / 10u) + '.' + std::to_string(tenths % 10u) + '\t' +
           std::to_string(row[2] >> 16 & 0xFFu) + '\t' + knockout_distance(row[3] & 0xFFFFu) + '\t' + knockout_distance(row[3] >> 16) + '\t' +
           (n1 && n2 ? "1+2" : n1 ? "1" : n2 ? "2" : "-");
}

// --knockout-out: "#guideId", the eight columns, and the flags of a coding cut by name ("-": none)
inline void write_knockout(const std::string &path, const std::vector<uint32_t> &rows, const std::vector<std::string> &transcripts,
                           const std::vector<std::string> &ids)
{
    std::ofstream out(path);
    if (!out.is_open()) throw std::runtime_error("Could not open the --knockout-out path.");
    out << "#guideId" << knockout_header() << "\tkoFlags\n";
    for (size_t i = 0; i < ids.size(); ++i) {
        const uint32_t *row = &rows[4 * i];
        std::string flags;
        if (row[0] != 0xFFFFFFFFu)
            for (uint32_t k = 0; k < 7u; ++k)
                if (row[2] >> (24u + k) & 1u) flags += (flags.empty() ? "" : "+") + std::string(knockout_flag_names()[k]);
        out << ids[i] << knockout_columns(row, transcripts) << '\t' << (flags.empty() ? "-" : flags) << '\n';
    }
    out.close();
    if (!out) throw std::runtime_error("Could not write the --knockout-out file.");
}

}  // namespace vsc_host
