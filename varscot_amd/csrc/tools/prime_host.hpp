// prime_host.hpp - the --prime, --prime-edits, --prime-allow-weak and --prime-out options of guide_summary and pattern_search: the
// pegRNA extensions of the guides that -E finds for a list of wanted edits (include/varscot_hip.h "prime-editing guide design";
// tools/README.md).
//   --prime PE2 | SPEC     PE2: the preset for the SpCas9 23-mer (nick 17, 41 bases behind the site, PBS 13, RTT 10 .. 34, 5 bases
//                          of homology, PAM 21,2, seed 17,3, no template that ends on G) - commonly published settings and nothing
//                          more - or SPEC = NICK,DOWN,PBSMIN,PBSMAX,RTTMIN,RTTMAX,HOMOLOGY,PAMSTART,PAMLEN,SEEDSTART,SEEDLEN,AVOIDG:
//                          twelve numbers, the shape's fields in that order (all stability weights 0: the PBS is PBSMIN long)
//   --prime-edits FILE     the wanted edits (TSV: chrom, 0-based pos, ref length, alt letters or -); needs --prime
//   --prime-allow-weak     keep the candidates whose primer binding site is WEAK; needs --prime
//   --prime-out FILE       the listing of the (edit, guide) pairs; needs --prime-edits
// With --prime the candidates are FILTERED before the off-target search (FILTER of the definition: a defined context, with edits
// a pair, and - without --prime-allow-weak - a PBS that is not WEAK).  Host C++ only.
#pragma once

#include <algorithm>
#include <cctype>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>

#include "eff_model_host.hpp"

namespace vsc_host {

struct PrimeOptions {
    bool on = false, with_edits = false, with_pairs = false;
    uint32_t allow_weak = 0;
    vsc_prime_shape shape{};
    std::string edits_path, pairs_path;
};

// "" and *o filled, or the message of a refusal
inline std::string parse_prime_options(bool p_set, const std::string &p, bool e_set, const std::string &e, bool w_set, bool o_set,
                                       const std::string &out, bool enumerating, bool several_devices, uint32_t site_len, PrimeOptions *o)
{
    if ((e_set || w_set || o_set) && !p_set) return "--prime-edits, --prime-allow-weak and --prime-out belong to the editor of --prime: give --prime";
    if (!p_set) return "";
    if (!enumerating) return "--prime looks at the guides that -E finds: give -E";
    if (several_devices) return "--prime works on the candidates of one device: it does not combine with a device list";
    if (o_set && !e_set) return "--prime-out lists the pairs of guides and edits: give --prime-edits";
    vsc_prime_shape s{};
    s.site_len = site_len;
    if (p == "PE2") {
        if (site_len != (uint32_t)VSC_READ_LEN) return "--prime PE2 is a preset for sites of 23 bases: give the twelve numbers of a SPEC";
        s.down = 41, s.nick = 17, s.pbs_min = s.pbs_max = 13, s.rtt_min = 10, s.rtt_max = 34, s.min_homology = 5;
        s.pam_start = 21, s.pam_len = 2, s.seed_start = 17, s.seed_len = 3, s.flags = VSC_PRIME_AVOID_G_END;
    } else {
        unsigned long v[12];
        const char *at = p.c_str();
        bool ok = true;
        for (int k = 0; k < 12 && ok; ++k) {
            char *end = nullptr;
            ok = *at >= '0' && *at <= '9';
            v[k] = std::strtoul(at, &end, 10);
            ok = ok && end != at && v[k] <= 64 && *end == (k < 11 ? ',' : '\0');
            at = end + 1;
        }
        if (ok) {
            s.nick = (uint32_t)v[0], s.down = (uint32_t)v[1], s.pbs_min = (uint32_t)v[2], s.pbs_max = (uint32_t)v[3], s.rtt_min = (uint32_t)v[4];
            s.rtt_max = (uint32_t)v[5], s.min_homology = (uint32_t)v[6], s.pam_start = (uint32_t)v[7], s.pam_len = (uint32_t)v[8];
            s.seed_start = (uint32_t)v[9], s.seed_len = (uint32_t)v[10], s.flags = (uint32_t)v[11];
            const uint32_t C = site_len + s.down;
            ok = s.down <= 64 - site_len && s.nick >= 1 && s.nick <= site_len && s.pbs_min >= 1 && s.pbs_min <= s.pbs_max && s.pbs_max <= s.nick &&
                 s.rtt_min >= 1 && s.rtt_min <= s.rtt_max && s.rtt_max <= C - s.nick && s.min_homology <= s.rtt_max && s.pam_len <= 8 &&
                 s.pam_start + s.pam_len <= site_len && s.seed_len <= 8 && s.seed_start + s.seed_len <= site_len && s.flags <= 1;
        }
        if (!ok)
            return "--prime takes PE2 or NICK,DOWN,PBSMIN,PBSMAX,RTTMIN,RTTMAX,HOMOLOGY,PAMSTART,PAMLEN,SEEDSTART,SEEDLEN,AVOIDG - a shape the "
                   "definition allows for sites of " + std::to_string(site_len) + " bases - not '" + p + "'";
    }
    o->on = true;
    o->shape = s;
    o->with_edits = e_set;
    o->with_pairs = o_set;
    o->allow_weak = w_set ? 1u : 0u;
    o->edits_path = e;
    o->pairs_path = out;
    return "";
}

// The --prime-edits file: TSV, chrom pos ref-length alt; chrom = first word of a contig name, alt = letters of ACGT or - for
// none.  Sorted by (contig, pos): what the library takes, and an edit's index is its place here.  Two edits at one position are
// refused: several alleles of one position go into several runs.
inline std::vector<vsc_prime_edit> read_prime_edits(const std::string &path, const std::vector<std::string> &names)
{
    std::map<std::string, uint32_t> by_chrom;
    for (size_t c = names.size(); c-- > 0;) by_chrom[names[c].substr(0, names[c].find_first_of(" \t"))] = (uint32_t)c;
    std::ifstream in(path);
    if (!in) throw std::runtime_error("Could not open the --prime-edits file.");
    std::vector<vsc_prime_edit> edits;
    std::string line;
    while (std::getline(in, line)) {
        if (line.empty() || line[0] == '#') continue;
        std::istringstream is(line);
        std::string chr, alt;
        unsigned long long pos = 0, ref = 0;
        if (!(is >> chr >> pos >> ref >> alt)) throw std::runtime_error("--prime-edits: not 'chrom pos ref-length alt': '" + line + "'");
        auto it = by_chrom.find(chr);
        if (it == by_chrom.end()) throw std::runtime_error("--prime-edits: no sequence '" + chr + "' in the genome");
        if (alt == "-") alt.clear();
        if (pos > 0xFFFFFFFFull || ref > 16 || alt.size() > 16 || ref + alt.size() < 1)
            throw std::runtime_error("--prime-edits: an edit replaces 0 .. 16 bases by 0 .. 16 letters, not both 0: '" + line + "'");
        vsc_prime_edit e{it->second, (uint32_t)pos, (uint16_t)ref, (uint16_t)alt.size(), 0u};
        for (size_t k = 0; k < alt.size(); ++k) {
            const char *q = std::strchr("ACGT", std::toupper((unsigned char)alt[k]));
            if (!q || !alt[k]) throw std::runtime_error("--prime-edits: the alt letters are A C G T or -: '" + line + "'");
            e.ins |= (uint32_t)(q - "ACGT") << (2 * k);
        }
        edits.push_back(e);
    }
    std::sort(edits.begin(), edits.end(), [](const vsc_prime_edit &a, const vsc_prime_edit &b) { return a.contig != b.contig ? a.contig < b.contig : a.pos < b.pos; });
    for (size_t k = 1; k < edits.size(); ++k)
        if (edits[k].contig == edits[k - 1].contig && edits[k].pos == edits[k - 1].pos)
            throw std::runtime_error("--prime-edits: two edits at one position; several alleles of one position go into several runs");
    return edits;
}

// "\tpbsLen\tpbsGC\tprimePairs" of a candidate; NA three times where the row is undefined
inline std::string prime_columns(const uint32_t *row)
{
    if (row[0] == VSC_PRIME_UNDEFINED) return "\tNA\tNA\tNA";
    return '\t' + std::to_string(row[0] & 0xFFu) + '\t' + std::to_string(row[0] >> 8 & 0xFFu) + '\t' + std::to_string(row[1]);
}

inline std::string prime_revcomp(const std::string &s)
{
    std::string r(s.rbegin(), s.rend());
    for (char &c : r) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : 'N';
    return r;
}

// the --prime-out file: one line per pair in the library's order - ascending (guide, edit); the extension (RTT then PBS, 5' to 3')
// by vsc_prime_site_text over the candidate's context out of the packed genome
template <class Index>
inline void write_prime_pairs(const std::string &path, const vsc_prime_shape &s, const std::vector<vsc_prime_pair> &pairs,
                              const std::vector<vsc_prime_edit> &edits, const std::vector<vsc_locus> &loci, const Index &ix,
                              const std::vector<std::string> &ids)
{
    std::ofstream out(path);
    if (!out.is_open()) throw std::runtime_error("Could not open the --prime-out path.");
    out << "#chrom\tpos\tguideId\tpbsLen\trttLen\tnickToEdit\thomology\tflags\textension\n";
    const uint32_t C = s.site_len + s.down;
    for (const vsc_prime_pair &p : pairs) {
        const vsc_prime_edit &e = edits.at(p.edit);
        const vsc_locus &l = loci.at(p.candidate);
        const uint32_t f0 = l.strand ? l.pos - s.down : l.pos, f = e.pos - f0;
        std::string context(C, 'N'), ins;
        vsc_unpack_bases(ix.hi.data(), ix.lo.data(), ix.nm.data(), ix.contigs[l.contig].offset + f0, C, &context[0]);
        for (uint32_t k = 0; k < e.ins_len; ++k) ins += "ACGT"[e.ins >> (2 * k) & 3u];
        if (l.strand) context = prime_revcomp(context), ins = prime_revcomp(ins);
        uint32_t row[2], pair[2];
        char ext[80];
        if (vsc_prime_site_text(context.c_str(), &s, l.strand ? C - f - e.del_len : f, e.del_len, ins.c_str(), row, pair, ext) != VSC_OK || !row[1] ||
            pair[0] != p.info || pair[1] != p.ext)
            throw std::runtime_error("--prime-out: the host's pair differs from the device's");
        const uint32_t flags = p.info >> 24;
        std::string names;
        const char *const flag_names[4] = {"PAM", "SEED", "POLY_T", "WEAK"};
        for (int b = 0; b < 4; ++b)
            if (flags >> b & 1u) names += (names.empty() ? "" : "+") + std::string(flag_names[b]);
        const std::string &name = ix.names.at(e.contig);
        out << name.substr(0, name.find_first_of(" \t")) << '\t' << e.pos << '\t' << ids.at(p.candidate) << '\t' << (p.ext >> 16 & 0xFFu) << '\t'
            << (p.info & 0xFFu) << '\t' << (p.info >> 8 & 0xFFu) << '\t' << (p.info >> 16 & 0xFFu) << '\t' << (names.empty() ? "-" : names) << '\t' << ext
            << '\n';
    }
    out.close();
    if (!out) throw std::runtime_error("Could not write the --prime-out file.");
}

// Rows and - with --prime-out - pairs of the candidates where they lie: prime(rows, pairs, capacity, &n_pairs) is the library call
template <class Call>
inline void prime_rows_and_pairs(const PrimeOptions &o, uint64_t n, Call prime, std::vector<uint32_t> *rows, std::vector<vsc_prime_pair> *pairs)
{
    rows->assign(2 * n, 0u);
    pairs->clear();
    uint64_t n_pairs = 0;
    prime(rows->data(), (vsc_prime_pair *)nullptr, (uint64_t)0, &n_pairs);  // the rows; the pairs are counted
    if (o.with_pairs && n_pairs) {
        pairs->resize(n_pairs);
        prime((uint32_t *)nullptr, pairs->data(), n_pairs, &n_pairs);
    }
}

}  // namespace vsc_host
