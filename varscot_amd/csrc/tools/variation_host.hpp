// variation_host.hpp - the --variants options of guide_summary and pattern_search: the known variants under the sites of the guides
// that -E finds (include/varscot_hip.h "known variation under candidate guides"; tools/README.md).
//   --variants FILE              a VCF (.vcf: CHROM POS ID REF ALT QUAL FILTER INFO, POS 1-based, one variant per ALT allele) or a TSV
//                                (chrom pos ref alt [weight], pos 0-based)
//   --variant-af KEY             VCF: the weight of a variant is round(-log1p(-AF) * 2^20) of the INFO key's value (one per ALT)
//   --variant-seed N             the seed: the N protospacer bases next to the PAM (default 10)
//   --max-variant-cost N         keep only the candidates whose cost - the sum of their disrupting variants' weights - is at most N
//   --max-variants-by-zone a,b,c,d   ... with at most a, b, c, d disrupting variants of top zone none, distal, seed, PAM (255: no bound)
//   --require-variant-zones LIST ... with a disrupting variant in one of the zones (numbers or none, distal, seed, pam)
//   --variation-out FILE         the rows of the guides and the (guide, variant) pairs as TSV
// The alleles are normalised as varscot_amd.site_variants normalises them: the common prefix, then the common suffix is trimmed;
// an SNV has span 1 and its alt, a deletion spans its deleted bases, an insertion the two bases that flank it, anything else the
// bases of its ref.  With a bound or a requirement the candidates are FILTERED before the off-target search.  Host C++ only.
#pragma once

#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>

#include "eff_model_host.hpp"
#include "vcf_expand.hpp"

namespace vsc_host {

struct VariationOptions {
    bool on = false, filtered = false, with_out = false;
    vsc_variation_shape shape{};
    vsc_variation_filter filter{0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u};
    std::string variants_path, af_key, out_path;
};

inline bool variation_number(const std::string &text, unsigned long long max, unsigned long long *out)
{
    char *e = nullptr;
    if (text.empty() || !std::isdigit((unsigned char)text[0])) return false;
    const unsigned long long v = std::strtoull(text.c_str(), &e, 10);
    if (*e || v > max) return false;
    *out = v;
    return true;
}

// the IUPAC set of a pattern letter as bits A C G T, 0: no such letter
inline uint32_t variation_iupac(char c)
{
    static const char *const letters = "ACGTRYSWKMBDHVN";
    static const uint32_t bits[] = {1, 2, 4, 8, 5, 10, 6, 9, 12, 3, 14, 13, 11, 7, 15};
    const char *p = std::strchr(letters, std::toupper((unsigned char)c));
    return p && c ? bits[p - letters] : 0u;
}

// The shape of a pattern with its protospacer [start, start + length): inside it the `seed` bases next to the PAM are zone 2, the
// others zone 1, and nothing is accepted; outside it a letter is zone 3 and accepts its IUPAC set, an N zone 0 and everything.
inline bool variation_shape_of(const std::string &pattern, uint32_t start, uint32_t length, uint32_t seed, vsc_variation_shape *s)
{
    const uint32_t n = (uint32_t)pattern.size();
    if (n < 16 || n > 32 || length < 1 || start + length > n || seed > length || (start > 0 && start + length < n)) return false;
    *s = vsc_variation_shape{};
    s->site_len = n;
    const uint32_t seed_first = start > 0 ? start : start + length - seed;
    for (uint32_t j = 0; j < n; ++j) {
        uint64_t zone, accept = 0;
        if (j >= start && j < start + length) zone = j >= seed_first && j < seed_first + seed ? 2 : 1;
        else {
            accept = variation_iupac(pattern[j]);
            if (!accept) return false;
            zone = accept == 15 ? 0 : 3;
        }
        s->zones |= zone << (2 * j);
        s->accept[j >> 4] |= accept << (4 * (j & 15));
    }
    return true;
}

// "" and *o filled, or the message of a refusal
inline std::string parse_variation_options(const Option &variants, const Option &af, const Option &seed, const Option &cost, const Option &by_zone,
                                           const Option &require, const Option &out, bool enumerating, bool several_devices,
                                           const std::string &pattern, uint32_t proto_start, uint32_t proto_len, VariationOptions *o)
{
    if ((af.set || seed.set || cost.set || by_zone.set || require.set || out.set) && !variants.set)
        return "--variant-af, --variant-seed, --max-variant-cost, --max-variants-by-zone, --require-variant-zones and --variation-out belong to "
               "the variants of --variants: give --variants";
    if (!variants.set) return "";
    if (!enumerating) return "--variants looks at the guides that -E finds: give -E";
    if (several_devices) return "--variants works on the candidates of one device: it does not combine with a device list";
    unsigned long long v = 10;
    if (seed.set && !variation_number(seed.value, proto_len, &v))
        return "--variant-seed takes the seed's length, 0 .. " + std::to_string(proto_len) + ", not '" + seed.value + "'";
    if (!variation_shape_of(pattern, proto_start, proto_len, (uint32_t)std::min<unsigned long long>(v, proto_len), &o->shape))
        return "--variants needs a pattern of 16 .. 32 IUPAC letters with the PAM on one side of the protospacer";
    if (cost.set) {
        if (!variation_number(cost.value, 0xFFFFFFFFull, &v)) return "--max-variant-cost takes a number 0 .. 4294967295, not '" + cost.value + "'";
        o->filter.max_cost = (uint32_t)v;
    }
    if (by_zone.set) {
        const auto parts = vsc_vcf::split(by_zone.value, ',');
        uint32_t packed = 0;
        bool ok = parts.size() == 4;
        for (size_t z = 0; ok && z < 4; ++z) {
            ok = variation_number(parts[z], 255, &v);
            packed |= (uint32_t)v << (8 * z);
        }
        if (!ok) return "--max-variants-by-zone takes a,b,c,d: the bounds of the zones none, distal, seed and pam, 0 .. 255 (255: no bound), not '" +
                        by_zone.value + "'";
        o->filter.max_by_zone = packed;
    }
    if (require.set) {
        static const char *const names[] = {"none", "distal", "seed", "pam"};
        for (const std::string &part : vsc_vcf::split(require.value, ',')) {
            int z = -1;
            for (int k = 0; k < 4; ++k)
                if (part == names[k] || part == std::to_string(k)) z = k;
            if (z < 0) return "--require-variant-zones takes zones out of none, distal, seed, pam (or 0 .. 3), comma-separated, not '" + require.value + "'";
            o->filter.require_zones |= 1u << z;
        }
    }
    if (af.set && af.value.empty()) return "--variant-af takes the INFO key of the allele frequency";
    o->on = true;
    o->filtered = cost.set || by_zone.set || require.set;
    o->with_out = out.set;
    o->variants_path = variants.value;
    o->af_key = af.set ? af.value : "";
    o->out_path = out.value;
    return "";
}

// round(-log1p(-af) * 2^20), at most 0xFFFFFFFE: varscot_amd.variant_weight
inline uint32_t variation_weight(double af)
{
    if (!(af >= 0)) throw std::runtime_error("--variant-af: an allele frequency is a number in 0 .. 1");
    if (af >= 1.0) return 0xFFFFFFFEu;
    const double x = std::floor(-std::log1p(-af) * 1048576.0 + 0.5);
    return x >= 4294967294.0 ? 0xFFFFFFFEu : (uint32_t)x;
}

// One variant out of (contig, 0-based pos of ref's first base, ref, alt, weight), normalised; false: the alleles are equal
inline bool variation_normalise(uint32_t contig, uint64_t pos, std::string ref, std::string alt, uint32_t weight, uint64_t contig_len, vsc_variant *out)
{
    ref = vsc_vcf::dna5(ref);
    alt = vsc_vcf::dna5(alt);
    size_t k = 0;
    while (k < ref.size() && k < alt.size() && ref[k] == alt[k]) ++k;
    ref.erase(0, k);
    alt.erase(0, k);
    pos += k;
    k = 0;
    while (k < ref.size() && k < alt.size() && ref[ref.size() - 1 - k] == alt[alt.size() - 1 - k]) ++k;
    ref.erase(ref.size() - k);
    alt.erase(alt.size() - k);
    if (ref.empty() && alt.empty()) return false;
    uint64_t span = ref.size();
    uint32_t code = VSC_VARIANT_OTHER;
    if (ref.size() == 1 && alt.size() == 1) {
        const char *p = std::strchr("ACGT", alt[0]);
        if (p && alt[0]) code = (uint32_t)(p - "ACGT");
    } else if (ref.empty()) {  // an insertion in front of pos: the bases on either side of it
        const uint64_t first = pos ? pos - 1 : 0, last = std::min<uint64_t>(pos + 1, contig_len);
        pos = first;
        span = last > first ? last - first : 0;
    }
    if (span < 1 || span > 65535 || pos + span > contig_len) throw std::runtime_error("--variants: a variant spans 1 .. 65535 bases inside its sequence");
    *out = vsc_variant{contig, (uint32_t)pos, (uint32_t)span | code << 16, weight};
    return true;
}

// The --variants file, ascending (contig, pos), lines of one position in the file's order: what the library takes.
inline std::vector<vsc_variant> read_variants(const VariationOptions &o, const std::vector<std::string> &names, const std::vector<vsc_contig> &contigs)
{
    std::map<std::string, uint32_t> by_chrom;
    for (size_t c = names.size(); c-- > 0;) by_chrom[names[c].substr(0, names[c].find_first_of(" \t"))] = (uint32_t)c;
    std::ifstream in(o.variants_path);
    if (!in) throw std::runtime_error("Could not open the --variants file.");
    const bool vcf = has_extension(o.variants_path, {"vcf"});
    if (!vcf && !o.af_key.empty()) throw std::runtime_error("--variant-af reads the INFO column of a VCF; a TSV has its weight in the fifth column");
    std::vector<vsc_variant> out;
    std::string line;
    while (std::getline(in, line)) {
        while (!line.empty() && (line.back() == '\r' || line.back() == '\n')) line.pop_back();
        if (line.empty() || line[0] == '#') continue;
        auto f = vsc_vcf::split(line, '\t');
        if (!vcf && f.size() < 4) {  // (a TSV may be separated by blanks)
            std::istringstream is(line);
            f.clear();
            for (std::string w; is >> w;) f.push_back(w);
        }
        if (f.size() < (vcf ? 5u : 4u)) throw std::runtime_error("--variants: not a variant line: '" + line + "'");
        auto it = by_chrom.find(f[0]);
        if (it == by_chrom.end()) throw std::runtime_error("--variants: no sequence '" + f[0] + "' in the genome");
        unsigned long long pos = 0, w = 0;
        if (!variation_number(f[1], 0xFFFFFFFFull, &pos) || (vcf && pos == 0)) throw std::runtime_error("--variants: not a position: '" + line + "'");
        if (vcf) --pos;
        const std::string &ref = f[vcf ? 3 : 2];
        const auto alts = vcf ? vsc_vcf::split(f[4], ',') : std::vector<std::string>{f[3]};
        std::vector<std::string> afs;
        if (vcf && !o.af_key.empty() && f.size() > 7)
            for (const std::string &entry : vsc_vcf::split(f[7], ';'))
                if (entry.compare(0, o.af_key.size() + 1, o.af_key + "=") == 0) afs = vsc_vcf::split(entry.substr(o.af_key.size() + 1), ',');
        if (!vcf && f.size() > 4 && !variation_number(f[4], 0xFFFFFFFEull, &w)) throw std::runtime_error("--variants: not a weight: '" + line + "'");
        for (size_t a = 0; a < alts.size(); ++a) {
            if (alts[a].empty() || alts[a] == "." || alts[a] == "*" || alts[a][0] == '<') continue;  // no allele, a spanning deletion, a symbolic allele
            uint32_t weight = (uint32_t)w;
            if (!o.af_key.empty()) {
                if (a >= afs.size()) throw std::runtime_error("--variant-af: no " + o.af_key + " for an allele of '" + line + "'");
                weight = variation_weight(std::strtod(afs[a].c_str(), nullptr));
            }
            vsc_variant v{};
            if (variation_normalise(it->second, pos, ref, alts[a], weight, contigs.at(it->second).length, &v)) out.push_back(v);
        }
    }
    std::stable_sort(out.begin(), out.end(), [](const vsc_variant &a, const vsc_variant &b) { return a.contig != b.contig ? a.contig < b.contig : a.pos < b.pos; });
    return out;
}

// the --variation-out file: the rows of the guides, a blank line, the pairs in the library's order - ascending (guide, variant)
inline void write_variation(const std::string &path, const std::vector<uint32_t> &rows, const std::vector<vsc_variation_pair> &pairs,
                            const std::vector<vsc_variant> &variants, const std::vector<std::string> &names, const std::vector<std::string> &ids)
{
    std::ofstream out(path);
    if (!out.is_open()) throw std::runtime_error("Could not open the --variation-out path.");
    out << "#guideId\tnone\tdistal\tseed\tpam\tsilent\tcost\tmaxWeight\n";
    for (size_t i = 0; i < ids.size(); ++i) {
        const uint32_t *r = &rows.at(4 * i);
        out << ids[i];
        if (r[2] == VSC_VARIATION_UNDEFINED) out << "\tNA\tNA\tNA\tNA\tNA\tNA\tNA\n";
        else out << '\t' << (r[0] & 255u) << '\t' << (r[0] >> 8 & 255u) << '\t' << (r[0] >> 16 & 255u) << '\t' << (r[0] >> 24) << '\t' << r[1] << '\t' << r[2]
                 << '\t' << r[3] << '\n';
    }
    out << "\n#chrom\tpos\tspan\talt\tguideId\tfirst\ttouched\ttop\tsilent\tweight\n";
    for (const vsc_variation_pair &p : pairs) {
        const vsc_variant &v = variants.at(p.variant);
        const std::string &name = names.at(v.contig);
        const uint32_t alt = v.span_alt >> 16;
        out << name.substr(0, name.find_first_of(" \t")) << '\t' << v.pos << '\t' << (v.span_alt & 0xFFFFu) << '\t' << (alt < 4 ? std::string(1, "ACGT"[alt]) : ".")
            << '\t' << ids.at(p.candidate) << '\t' << (p.info & 0xFFu) << '\t' << (p.info >> 8 & 0xFFu) << '\t' << (p.info >> 16 & 3u) << '\t'
            << (p.info >> 18 & 1u) << '\t' << p.weight << '\n';
    }
    out.close();
    if (!out) throw std::runtime_error("Could not write the --variation-out file.");
}

// Rows and pairs of the candidates where they lie: call(rows, pairs, capacity, &n_pairs) is the library call
template <class Call>
inline void variation_rows_and_pairs(uint64_t n, Call call, std::vector<uint32_t> *rows, std::vector<vsc_variation_pair> *pairs)
{
    rows->assign(4 * n, 0u);
    pairs->clear();
    uint64_t n_pairs = 0;
    call(rows->data(), (vsc_variation_pair *)nullptr, (uint64_t)0, &n_pairs);  // the rows; the pairs are counted
    if (n_pairs) {
        pairs->resize(n_pairs);
        call((uint32_t *)nullptr, pairs->data(), n_pairs, &n_pairs);
    }
}

}  // namespace vsc_host
