// pattern_search - off-targets of any nuclease and guide shape over a packed genome: an IUPAC pattern the site must satisfy
// (the PAM, at either end or both), IUPAC guides of the pattern's length (N = not compared) and a mismatch budget - the
// pattern / query model of Cas-OFFinder.  Per-guide counts by mismatches (-O) and / or the hits themselves (-T).
// Host C++ only: the search runs in libvarscot_hip.so (vsc_search_pattern); there is no CPU search here.  Every argument is
// checked before a device is opened.
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <fstream>

#include "vsc_host.hpp"

using namespace vsc_host;

namespace {

bool iupac(char c)
{
    for (const char *p = "ACGTRYSWKMBDHVNacgtryswkmbdhvn"; *p; ++p)
        if (*p == c) return true;
    return false;
}

// chrom and guideId are the first word of the FASTA header, as guide_summary prints them
std::string first_word(const std::string &s) { return s.substr(0, s.find_first_of(" \t")); }

}  // namespace

int main(int argc, char **argv)
{
    std::vector<Option> opts = {
        {'i', "index", "Prefix of the packed genome (bidir_index -I)", true},
        {'q', "pattern", "IUPAC pattern of 16..32 letters that a site must satisfy, e.g. NNNNNNNNNNNNNNNNNNNNNGRRT", true},
        {'R', "guides", "FASTA of the guides: IUPAC records of the pattern's length, N = position not compared", true},
        {'M', "mismatches", "Number of allowed mismatches (0..8)", true},
        {'D', "device", "HIP device index (default 0)", false},
        {'O', "output", "Summary TSV: #guideId guideSeq offtargetCount mm0 .. mm<M>", false},
        {'T', "hits", "Hits TSV: #guideId chrom start end strand mismatches mismatchPositions sequence", false},
    };
    const int pr = parse_args(argc, argv, opts, "Pattern search",
                              "Off-target search for any PAM and any guide of 16..32 bases: the sites of the genome that satisfy "
                              "the pattern and differ from a guide in at most -M compared positions. Give -O, -T or both.");
    if (pr) return pr == 1;
    const std::string prefix = opts[0].value, pattern = opts[1].value, guides_path = opts[2].value;
    if (pattern.size() < VSC_PATTERN_MIN_LEN || pattern.size() > VSC_PATTERN_MAX_LEN) {
        std::fprintf(stderr, "%s: the pattern must have 16..32 letters, '%s' has %zu\n", argv[0], pattern.c_str(), pattern.size());
        return 1;
    }
    for (char c : pattern)
        if (!iupac(c)) {
            std::fprintf(stderr, "%s: '%c' in the pattern '%s' is no IUPAC letter\n", argv[0], c, pattern.c_str());
            return 1;
        }
    if (!has_extension(guides_path, {"fa", "fasta"}) || (opts[5].set && !has_extension(opts[5].value, {"tsv", "txt"})) ||
        (opts[6].set && !has_extension(opts[6].value, {"tsv", "txt"}))) {
        std::fprintf(stderr, "%s: the guides must be a .fa/.fasta file, the outputs .tsv/.txt files\n", argv[0]);
        return 1;
    }
    if (!opts[5].set && !opts[6].set) {
        std::fprintf(stderr, "%s: give -O, -T or both\n", argv[0]);
        return 1;
    }
    char *end = nullptr;
    const long mm = std::strtol(opts[3].value.c_str(), &end, 10);
    if (end == opts[3].value.c_str() || *end) {
        std::fprintf(stderr, "%s: the given value '%s' cannot be casted to integer\n", argv[0], opts[3].value.c_str());
        return 1;
    }
    if (mm < 0 || mm > VSC_MAX_MISMATCHES) {
        std::fprintf(stderr, "Error: Maximum number of mismatches must lie between 0 and 8.\n");
        return 1;
    }
    long device = 0;
    if (opts[4].set) {
        device = std::strtol(opts[4].value.c_str(), &end, 10);
        if (end == opts[4].value.c_str() || *end || device < 0) {
            std::fprintf(stderr, "%s: -D takes one device index, not '%s'\n", argv[0], opts[4].value.c_str());
            return 1;
        }
    }

    vsc_ctx *ctx = nullptr;
    vsc_genome *genome = nullptr;
    vsc_pattern_hits *hits = nullptr;
    int rc = 1;
    try {
        const auto guides = read_fasta(guides_path);
        const uint32_t len = (uint32_t)pattern.size();
        std::string letters;
        for (const auto &g : guides) {
            if (g.seq.size() != len)
                throw std::runtime_error("guide '" + g.id + "' has " + std::to_string(g.seq.size()) + " letters, the pattern has " + std::to_string(len));
            for (char c : g.seq)
                if (!iupac(c)) throw std::runtime_error("guide '" + g.id + "' holds '" + std::string(1, c) + "', which is no IUPAC letter");
            letters += g.seq;
        }
        std::printf("Guides loaded (total: %zu).\n", guides.size());
        const PackedIndex ix = read_index(prefix);
        int st = vsc_ctx_create((int)device, &ctx);
        if (st != VSC_OK) throw std::runtime_error(st == VSC_ERR_NODEVICE ? "no HIP device available (there is no CPU fallback)" : "could not create the device context");
        st = vsc_genome_load(ctx, ix.hi.data(), ix.lo.data(), ix.nm.data(), 0, ix.hi.size(), ix.hi.size(), ix.contigs.data(),
                             (uint32_t)ix.contigs.size(), &genome);
        if (st != VSC_OK) throw std::runtime_error(vsc_last_error(ctx));
        std::printf("Index loaded.\n");

        vsc_pattern_params p{};
        p.max_mismatches = (uint32_t)mm;
        std::vector<vsc_pattern_summary> rows(guides.size());
        st = vsc_search_pattern(ctx, genome, pattern.c_str(), letters.c_str(), (uint32_t)guides.size(), len, &p, opts[6].set ? &hits : nullptr,
                                rows.data());
        if (st != VSC_OK) throw std::runtime_error(vsc_last_error(ctx));

        if (opts[5].set) {
            std::ofstream out(opts[5].value);
            if (!out.is_open()) throw std::runtime_error("Could not open output path.");
            out << "#guideId\tguideSeq\tofftargetCount";
            for (long k = 0; k <= mm; ++k) out << "\tmm" << k;
            out << '\n';
            for (size_t g = 0; g < guides.size(); ++g) {
                uint64_t total = 0;
                for (long k = 0; k <= mm; ++k) total += rows[g].count[k];
                out << first_word(guides[g].id) << '\t' << guides[g].seq << '\t' << total;
                for (long k = 0; k <= mm; ++k) out << '\t' << rows[g].count[k];
                out << '\n';
            }
            if (!out) throw std::runtime_error("Write error on " + opts[5].value);
        }
        if (opts[6].set) {
            const uint64_t n = vsc_pattern_hits_count(hits);
            const vsc_pattern_hit *h = nullptr;
            st = vsc_pattern_hits_data(hits, &h);
            if (st != VSC_OK) throw std::runtime_error(vsc_last_error(ctx));
            std::ofstream out(opts[6].value);
            if (!out.is_open()) throw std::runtime_error("Could not open output path.");
            out << "#guideId\tchrom\tstart\tend\tstrand\tmismatches\tmismatchPositions\tsequence\n";
            std::string window(len, 'N'), text;
            for (uint64_t i = 0; i < n; ++i) {
                const vsc_pattern_hit &r = h[i];
                vsc_unpack_bases(ix.hi.data(), ix.lo.data(), ix.nm.data(), ix.contigs[r.contig].offset + r.pos, len, &window[0]);
                std::string where;  // 0-based window positions on the forward genome, ascending; - if none
                for (uint32_t b = 0; b < len; ++b)
                    if ((r.mask >> b) & 1u) where += (where.empty() ? "" : ",") + std::to_string(b);
                text += first_word(guides[r.guide].id) + '\t' + first_word(ix.names[r.contig]) + '\t' + std::to_string(r.pos) + '\t' + std::to_string(r.pos + len) + '\t' +
                        (VSC_PATTERN_STRAND(r.info) ? '-' : '+') + '\t' + std::to_string(VSC_PATTERN_NM(r.info)) + '\t' + (where.empty() ? "-" : where) +
                        '\t' + window + '\n';
                if (text.size() > (1u << 22)) {
                    out << text;
                    text.clear();
                }
            }
            out << text;
            if (!out) throw std::runtime_error("Write error on " + opts[6].value);
        }
        rc = 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "ERROR: %s\n", e.what());
        rc = 1;
    }
    vsc_pattern_hits_free(hits);
    vsc_genome_free(genome);
    vsc_ctx_destroy(ctx);
    return rc;
}
