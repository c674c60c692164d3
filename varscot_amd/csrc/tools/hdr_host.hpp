// hdr_host.hpp - the --hdr, --hdr-edits, --hdr-out, --hdr-cds and --hdr-allow-open options of guide_summary and pattern_search:
// knock-in design by homology-directed repair for the guides that -E finds and a list of wanted edits (include/varscot_hip.h "HDR
// knock-in design"; tools/README.md).
//   --hdr SpCas9 | Cas12a | SPEC   SpCas9: the preset for the 23-mer (20 bases in front, 21 behind, cut 17, anchor 1, PAM NGG at 20,
//                          seed 10,10, protospacer 0,20); Cas12a: the preset for a 27-mer (18 in front, 19 behind, cut 22, anchor 0,
//                          PAM TTTV at 0, seed 4,6, protospacer 4,23); both with max_dist 30, min_seed_mm 2, min_proto_mm 4 and every
//                          flag - or SPEC = UP,DOWN,CUT,MAXDIST,ANCHOR,PAMSTART,PAM,SEEDSTART,SEEDLEN,PROTOSTART,PROTOLEN,MINSEED,
//                          MINPROTO,FLAGS: fourteen fields, the shape's in that order, PAM in IUPAC letters (- for none)
//   --hdr-edits FILE       the wanted edits (TSV: chrom, 0-based pos, ref length, alt letters or -, as --prime-edits); needs --hdr
//   --hdr-cds FILE         coding segments (BED6 as --cds): a blocking substitution inside them is synonymous; needs --hdr
//   --hdr-allow-open       keep the candidates with a pair, usable or not; needs --hdr
//   --hdr-out FILE         the listing of the (edit, guide) pairs; needs --hdr-edits
// With --hdr the candidates are FILTERED before the off-target search (FILTER of the definition: a defined context, and with edits
// a usable pair - with --hdr-allow-open any pair).  Host C++ only.
#pragma once

#include "effects_host.hpp"
#include "prime_host.hpp"

namespace vsc_host {

struct HdrOptions {
    bool on = false, with_edits = false, with_pairs = false, with_cds = false;
    uint32_t allow_open = 0;
    vsc_hdr_shape shape{};
    std::string edits_path, pairs_path, cds_path;
};

// the letters an IUPAC letter accepts (bit b = letter b of ACGT), 0 for another character
inline uint32_t hdr_iupac_set(char c)
{
    static const char *const letters = "ACGTRYSWKMBDHVN";
    static const uint32_t sets[15] = {1, 2, 4, 8, 5, 10, 6, 9, 12, 3, 14, 13, 11, 7, 15};
    const char *q = std::strchr(letters, std::toupper((unsigned char)c));
    return q && c ? sets[q - letters] : 0u;
}

// is s a shape SHAPE of the definition allows?  (the library's rule, so that the refusal comes before a device is opened)
inline bool hdr_shape_ok(const vsc_hdr_shape &s)
{
    if (s.site_len < 16 || s.site_len > 32 || s.up > 32 || s.down > 32 || s.up + s.site_len + s.down > 64) return false;
    if (s.cut < 1 || s.cut > s.site_len - 1 || s.max_dist > 63 || s.anchor > 1) return false;
    if (s.pam_len > 8 || s.pam_start > s.site_len || s.pam_len > s.site_len - s.pam_start) return false;
    for (uint32_t j = 0; j < 8; ++j)
        if (j < s.pam_len ? (s.pam_accept[j] < 1 || s.pam_accept[j] > 15) : s.pam_accept[j] != 0) return false;
    if (s.seed_len > 16 || s.seed_start > s.site_len || s.seed_len > s.site_len - s.seed_start) return false;
    if (s.proto_len > 32 || s.proto_start > s.site_len || s.proto_len > s.site_len - s.proto_start) return false;
    return s.min_seed_mm <= s.seed_len && s.min_proto_mm <= s.proto_len && s.flags <= 7 && s.reserved == 0;
}

// "" and *o filled, or the message of a refusal
inline std::string parse_hdr_options(const Option &h, const Option &e, const Option &out, const Option &cds, const Option &open, bool enumerating,
                                     bool several_devices, uint32_t site_len, HdrOptions *o)
{
    if ((e.set || out.set || cds.set || open.set) && !h.set)
        return "--hdr-edits, --hdr-out, --hdr-cds and --hdr-allow-open belong to the nuclease of --hdr: give --hdr";
    if (!h.set) return "";
    if (!enumerating) return "--hdr looks at the guides that -E finds: give -E";
    if (several_devices) return "--hdr works on the candidates of one device: it does not combine with a device list";
    if (out.set && !e.set) return "--hdr-out lists the pairs of guides and edits: give --hdr-edits";
    vsc_hdr_shape s{};
    s.site_len = site_len;
    const std::string &p = h.value;
    auto pam = [&](const std::string &text) {
        if (text.size() > 8) return false;
        for (size_t j = 0; j < text.size(); ++j)
            if (!(s.pam_accept[j] = hdr_iupac_set(text[j]))) return false;
        s.pam_len = (uint32_t)text.size();
        return true;
    };
    if (p == "SpCas9" || p == "Cas12a") {
        const bool cas9 = p == "SpCas9";
        if (site_len != (cas9 ? 23u : 27u))
            return "--hdr " + p + " is a preset for sites of " + (cas9 ? "23" : "27") + " bases: give the fourteen fields of a SPEC";
        s.max_dist = 30, s.min_seed_mm = 2, s.min_proto_mm = 4, s.flags = 7;
        if (cas9) s.up = 20, s.down = 21, s.cut = 17, s.anchor = 1, s.pam_start = 20, s.seed_start = 10, s.seed_len = 10, s.proto_start = 0, s.proto_len = 20;
        else s.up = 18, s.down = 19, s.cut = 22, s.anchor = 0, s.pam_start = 0, s.seed_start = 4, s.seed_len = 6, s.proto_start = 4, s.proto_len = 23;
        pam(cas9 ? "NGG" : "TTTV");
    } else {
        std::vector<std::string> f;
        std::istringstream is(p);
        for (std::string part; std::getline(is, part, ',');) f.push_back(part);
        bool ok = f.size() == 14 && p.back() != ',';
        unsigned long v[14] = {};
        for (size_t k = 0; k < 14 && ok; ++k) {
            if (k == 6) continue;
            char *end = nullptr;
            ok = !f[k].empty() && f[k][0] >= '0' && f[k][0] <= '9';
            v[k] = ok ? std::strtoul(f[k].c_str(), &end, 10) : 0;
            ok = ok && *end == '\0' && v[k] <= 64;
        }
        if (ok) {
            s.up = (uint32_t)v[0], s.down = (uint32_t)v[1], s.cut = (uint32_t)v[2], s.max_dist = (uint32_t)v[3], s.anchor = (uint32_t)v[4];
            s.pam_start = (uint32_t)v[5], s.seed_start = (uint32_t)v[7], s.seed_len = (uint32_t)v[8], s.proto_start = (uint32_t)v[9];
            s.proto_len = (uint32_t)v[10], s.min_seed_mm = (uint32_t)v[11], s.min_proto_mm = (uint32_t)v[12], s.flags = (uint32_t)v[13];
            ok = pam(f[6] == "-" ? std::string() : f[6]) && hdr_shape_ok(s);
        }
        if (!ok)
            return "--hdr takes SpCas9, Cas12a or UP,DOWN,CUT,MAXDIST,ANCHOR,PAMSTART,PAM,SEEDSTART,SEEDLEN,PROTOSTART,PROTOLEN,MINSEED,MINPROTO,FLAGS - "
                   "a shape the definition allows for sites of " + std::to_string(site_len) + " bases - not '" + p + "'";
    }
    o->on = true;
    o->shape = s;
    o->with_edits = e.set;
    o->with_pairs = out.set;
    o->with_cds = cds.set;
    o->allow_open = open.set ? 1u : 0u;
    o->edits_path = e.value;
    o->pairs_path = out.value;
    o->cds_path = cds.value;
    return "";
}

// "\thdrPairs\thdrUsable" of a candidate; NA twice where the row is undefined
inline std::string hdr_columns(const uint32_t *row)
{
    if (row[0] == VSC_HDR_UNDEFINED) return "\tNA\tNA";
    return '\t' + std::to_string(row[0]) + '\t' + std::to_string(row[1]);
}

// the --hdr-out file: one line per pair in the library's order - ascending (guide, edit): the edit's chrom and pos, the guide, the
// bases between the break and the edit, the changed letters the nuclease finds in the seed and the protospacer, the flags, and the
// blocking substitution as chrom, forward pos and forward letter (- three times: none)
inline void write_hdr_pairs(const std::string &path, const vsc_hdr_shape &s, const std::vector<vsc_hdr_pair> &pairs,
                            const std::vector<vsc_prime_edit> &edits, const std::vector<vsc_locus> &loci, const std::vector<std::string> &names,
                            const std::vector<std::string> &ids)
{
    std::ofstream out(path);
    if (!out.is_open()) throw std::runtime_error("Could not open the --hdr-out path.");
    out << "#chrom\tpos\tguideId\tdist\tseedMm\tprotoMm\tflags\tsubChrom\tsubPos\tsubBase\n";
    const uint32_t C = s.up + s.site_len + s.down;
    const char *const flag_names[6] = {"B_PAM", "B_SEED", "B_PROTO", "SUB_PAM", "SUB_SEED", "OPEN"};
    for (const vsc_hdr_pair &p : pairs) {
        const vsc_prime_edit &e = edits.at(p.edit);
        const vsc_locus &l = loci.at(p.candidate);
        const std::string &name = names.at(e.contig);
        const std::string chrom = name.substr(0, name.find_first_of(" \t"));
        std::string flags;
        for (int b = 0; b < 6; ++b)
            if (p.info >> (24 + b) & 1u) flags += (flags.empty() ? "" : "+") + std::string(flag_names[b]);
        out << chrom << '\t' << e.pos << '\t' << ids.at(p.candidate) << '\t' << (p.info & 0x3Fu) << '\t' << (p.info >> 8 & 0x1Fu) << '\t'
            << (p.info >> 13 & 0x3Fu) << '\t' << (flags.empty() ? "-" : flags);
        if (p.block == VSC_HDR_NO_BLOCK) out << "\t-\t-\t-\n";
        else {
            const uint32_t r = p.block >> 16 & 0xFFu, b = p.block >> 8 & 3u, f0 = l.pos - (l.strand ? s.down : s.up);
            out << '\t' << chrom << '\t' << (f0 + (l.strand ? C - 1 - r : r)) << '\t' << "ACGT"[l.strand ? 3u - b : b] << '\n';
        }
    }
    out.close();
    if (!out) throw std::runtime_error("Could not write the --hdr-out file.");
}

// Rows and - with --hdr-out - pairs of the candidates where they lie: hdr(rows, pairs, capacity, &n_pairs) is the library call
template <class Call>
inline void hdr_rows_and_pairs(const HdrOptions &o, uint64_t n, Call hdr, std::vector<uint32_t> *rows, std::vector<vsc_hdr_pair> *pairs)
{
    rows->assign(2 * n, 0u);
    pairs->clear();
    uint64_t n_pairs = 0;
    hdr(rows->data(), (vsc_hdr_pair *)nullptr, (uint64_t)0, &n_pairs);  // the rows; the pairs are counted
    if (o.with_pairs && n_pairs) {
        pairs->resize(n_pairs);
        hdr((uint32_t *)nullptr, pairs->data(), n_pairs, &n_pairs);
    }
}

}  // namespace vsc_host
