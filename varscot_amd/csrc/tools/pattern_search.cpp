// pattern_search - off-targets of any nuclease and guide shape over a packed genome: an IUPAC pattern the site must satisfy
// (the PAM, at either end or both), IUPAC guides of the pattern's length (N = not compared) and a mismatch budget - the
// pattern / query model of Cas-OFFinder.  Per-guide counts by mismatches (-O) and / or the hits themselves (-T).
// With -E the guides are not given but found: every site of the genome, or of the -B targets, that satisfies the pattern
// (vsc_guides_enumerate_pattern), filtered over the -p protospacer, written as a TSV of guide, contig, pos and strand - and,
// with -M and -O, screened in the same run (the design: every guide of the targets with its off-target counts).
// -u DNA,RNA (e.g. -u 1,1; each 0 .. 2, not both 0; needs -p) adds the BULGED sites (vsc_search_pattern_bulges): the sites one or
// two bases longer (DNA bulge) or shorter (RNA bulge) than the pattern that pair with the guide within -M when the extra bases
// of the site or of the guide, inside the -p protospacer, stay unpaired.  The -O summary gains, behind its columns, bulgeCount
// and per enabled class in ascending site length - br2 br1 bd1 bd2 - the columns <class>mm0 .. <class>mm<M>; -U bulges.tsv
// lists the sites in ascending (guide, strand, chrom, start, site length) order under guide_summary -U's columns
//   #guideId chrom start end strand kind size index mismatches sequence
// Without -u every output is what it was.
// -Z sites.tsv (needs -u, as -U) collapses the plain and the bulged alignments into CUT SITES on the device
// (vsc_pattern_hits_sites): one record per (guide, strand, chrom, PAM-side end) - the site's 3' end in read orientation when the
// -p protospacer starts the pattern, its 5' end when it ends the pattern (Cas12a) - with its best alignment.  The -O summary
// gains, behind all other columns, siteCount siteBulgeOnly; the listing goes under guide_summary -Z's columns
//   #guideId chrom start end strand kind size index mismatches members sequence
// Without -Z every output is what it was.
// -v in.vcf [-n SAMPLE] (needs -O and -M) screens the guides in an individual's genome as well (vsc_search_pattern_variants):
// variant windows of the pattern's length are built from the packed planes, searched on the same context and merged with the
// reference hits per guide on the device.  -O gains indCount imm0 .. imm<M> (the reference hits no window shadows plus the
// counted window hits) varCount vmm0 .. vmm<M> (the window hits that carry a variant) varDuplicates refShadowed, with -W also
// indScoreSum indSpec varScoreSum.  With -E the enumerated loci are the excluded on-targets, with -R nothing is excluded.
// Without -v every output is what it was.
// -w bulge.tsv (needs -W, -u, -p and -Z) scores the cut sites on the device (vsc_sites_table): -W stays the base table, whose
// protospacer must be -p's; the -w file holds `dna j s w` and `rna j g w` for every protospacer position j and base
// (tools/README.md).  The -O summary gains siteScoreSum siteSpecScore sitePositive behind all other columns, the -Z listing
// tableScore (%.9f) and scoredAs, and -K / -S cut the -Z listing per guide by that score.  Without -w every output is what it was.
// -Y model.tsv (needs -E) scores every found guide's ON-TARGET EFFICIENCY with a linear position-specific model
// (vsc_pattern_guides_efficiency; the file is what varscot_amd.EfficiencyModel.to_tsv writes, tools/README.md; its site_len
// must be the pattern's length): the -E listing gains two last columns, efficiencyLinear (%.17g; NA when the context leaves
// its sequence or holds an N) and efficiency (the predictor through the model's link).  -y MIN (needs -Y) keeps only the
// candidates whose predictor is defined and >= MIN, linear domain, BEFORE the search.  Without -Y every output is what it was.
// A -Y file that holds a `tree` line is an ensemble of regression trees instead (varscot_amd.TreeEfficiencyModel.to_tsv,
// tools/eff_trees_host.hpp; vsc_pattern_guides_efficiency_trees): the same columns, the same -y.
// -H FLANK[,CUT] (needs -E) scores every found guide's MICROHOMOLOGY around its cut site (vsc_pattern_guides_microhomology: the
// score of Bae et al. 2014 over FLANK bases on either side of the break in front of read position CUT; default CUT: 3 bases
// before the end of a protospacer that starts the pattern - SpCas9, SaCas9 - else 18 bases behind its start - Cas12a): the -E
// listing gains the last columns mhScore oofScore (%.17g; NA when the window leaves its sequence or holds an N).  -m
// MIN_OOF[,MIN_MH] (needs -H) keeps only the candidates whose out-of-frame share is at least MIN_OOF per cent and whose score
// is at least MIN_MH, BEFORE the search.
// -x START,LEN,BASE (needs -E; CBE | ABE for a pattern of 23 letters) looks at every found guide's BASE-EDITOR window
// (vsc_pattern_guides_edit): the -E listing gains the last columns editWindow editable targetsHit.  -z targets.bed (one base per
// line) and -l MIN,MAX (both need -x) keep only the candidates that reach a target base / hold MIN .. MAX editable bases, BEFORE
// the search; -o pairs.tsv (needs -z) lists the pairs.
// --prime SPEC (needs -E; PE2 for a pattern of 23 letters; SPEC = twelve numbers, tools/prime_host.hpp) looks at the pegRNA a PRIME
// EDITOR needs on every found guide (vsc_pattern_guides_prime): the candidates without a context (or, without
// --prime-allow-weak, with a WEAK primer binding site) are dropped BEFORE the search, with --prime-edits edits.tsv those that can
// write none of the edits as well; the -E listing gains the last columns pbsLen pbsGC primePairs; --prime-out pairs.tsv (needs
// --prime-edits) lists the pairs with their extensions.
// -W table.tsv scores every hit with a pattern TABLE (vsc_search_pattern_table; the CFD form for any nuclease: a product of
// weights by protospacer position, guide base and site base times a weight for the site's letters at up to four PAM positions;
// the file is what varscot_amd.PatternTable.to_tsv writes, tools/README.md: `shape L ps_start ps_len`, `pam_pos p...`,
// `pair j g s w`, `pam LETTERS w`; its L must be the pattern's length).  The -O summary gains, behind all other columns,
//   tableScoreSum tableSpecScore tablePositive
// = the sum of the hits' scores (fixed point, 2^-30 units, %.6f), floor(100 / (100 + sum) * 100 + 0.5) and the hits that score
// above 0; with -E a found guide's own locus is taken out of them as it is out of mm0.  With -T the listing is selected by the
// table score: -K the best K of every guide, -S a floor on the score, 0 .. 1, and a last column tableScore (%.9f); the summary
// stays over all hits.  -K and -S need -W and -T.  Without -W every output is what it was.
// Host C++ only: the search runs in libvarscot_hip.so (vsc_search_pattern); there is no CPU search here.  Every argument is
// checked before a device is opened.
// -k K[,SPACING] -b COLS [-c interval|name] (needs -E and -B) picks the K best guides of every -B target, their cut sites at
// least SPACING bases apart (vsc_pattern_guides_pick; tools/pick_host.hpp): ranked by table, eff, oof, mh in the order
// of -b - pattern hits have no MIT score, so -b is required -; the -E listing gains the last columns pickTarget pickRank.
// --hdr SpCas9 | Cas12a | SPEC (needs -E, one device; tools/hdr_host.hpp) asks whether a cut at every found guide can be repaired
// from a donor that carries a wanted edit: the candidates without a context are dropped BEFORE the off-target search,
// with --hdr-edits edits.tsv those without a usable pair as well (--hdr-allow-open: without any pair); --hdr-cds cds.bed keeps the
// blocking substitution synonymous; the -E listing gains the last columns hdrPairs hdrUsable; --hdr-out pairs.tsv (needs
// --hdr-edits) lists the pairs with their substitutions.
// --motifs motifs.tsv (needs -E, one device; tools/motif_host.hpp) looks for restriction sites and IUPAC motifs in the cloned construct
// (the spacer between --motif-left and --motif-right) and in the genomic context of every found guide: the listing gains the last
// columns motifsConstruct motifsCut motifsElsewhere motifsCutOnly; --motif-forbid / --motif-forbid-context / --motif-require-cut NAMES
// (--motif-cut-only) keep the candidates that pass; --motifs-out sites.tsv lists the names per candidate.
// --knockout [CUT] --knockout-cds cds.bed (needs -E, one device; tools/knockout_host.hpp) says where the cut of every found guide falls in
// the coding sequence and what a frameshift there does: the listing gains the last columns koTranscript koCodon koFrame koCutPct
// koEdge koPtc1 koPtc2 koNmd; --knockout-nmd WINDOW[,START] sets the decay rule, --knockout-filter MINPCT,MAXPCT[,EDGE[,REQUIRE[/FORBID]]]
// keeps the candidates that pass, --knockout-out rows.tsv lists the rows with their flags.
// --fold SpCas9 | Cas12a | SPEC (needs -E, one device; tools/fold_host.hpp) counts the stems the guide RNA of every found guide can
// form with itself and with the --fold-scaffold text (at most 128 letters, or @FILE; default: none): the -E listing gains the last
// columns foldStarts foldSelf foldScaffold foldSeed; --max-fold STARTS[,SELF[,SCAF[,SEED]]] keeps the candidates within the limits.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <fstream>
#include <map>
#include <sstream>

#include "eff_model_host.hpp"
#include "eff_trees_host.hpp"
#include "mh_host.hpp"
#include "edit_host.hpp"
#include "effects_host.hpp"
#include "prime_host.hpp"
#include "hdr_host.hpp"
#include "fold_host.hpp"
#include "motif_host.hpp"
#include "knockout_host.hpp"
#include "variation_host.hpp"
#include "pick_host.hpp"
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

// "a,b" as two integers in 0..255
bool two_numbers(const std::string &s, long *a, long *b)
{
    char *end = nullptr;
    *a = std::strtol(s.c_str(), &end, 10);
    if (end == s.c_str() || *end != ',') return false;
    const char *second = end + 1;
    *b = std::strtol(second, &end, 10);
    return end != second && !*end && *a >= 0 && *a <= 255 && *b >= 0 && *b <= 255;
}

// the -B intervals: BED3+, chrom = first word of a contig name
std::vector<vsc_interval> read_targets(const std::string &path, const PackedIndex &ix)
{
    std::map<std::string, uint32_t> by_chrom;
    for (size_t c = ix.names.size(); c-- > 0;) by_chrom[first_word(ix.names[c])] = (uint32_t)c;
    std::ifstream bed(path);
    if (!bed) throw std::runtime_error("Could not open the -B file.");
    std::vector<vsc_interval> iv;
    std::string line;
    while (std::getline(bed, line)) {
        if (line.empty() || line[0] == '#' || line.compare(0, 5, "track") == 0 || line.compare(0, 7, "browser") == 0) continue;
        std::istringstream is(line);
        std::string chr;
        unsigned long long start = 0, stop = 0;
        if (!(is >> chr >> start >> stop)) throw std::runtime_error("-B: not a BED line: '" + line + "'");
        auto it = by_chrom.find(chr);
        if (it == by_chrom.end()) throw std::runtime_error("-B: no sequence '" + chr + "' in the genome");
        if (start > stop || stop > 0xFFFFFFFFull) throw std::runtime_error("-B: bad interval in '" + line + "'");
        iv.push_back(vsc_interval{it->second, (uint32_t)start, (uint32_t)stop, 0u});
    }
    return iv;
}

// the -W file: what varscot_amd.PatternTable.to_tsv writes
vsc_pattern_table *load_pattern_table(const std::string &path, vsc_pattern_table_shape *shape)
{
    std::ifstream in(path);
    if (!in) throw std::runtime_error("Could not open the -W file.");
    vsc_pattern_table_shape s{};
    bool have_shape = false, have_pam_pos = false;
    std::vector<double> pair, pam(1, NAN);
    std::string line;
    size_t n = 0;
    auto base = [](char c) { return c == 'A' || c == 'a' ? 0 : c == 'C' || c == 'c' ? 1 : c == 'G' || c == 'g' ? 2 : c == 'T' || c == 't' || c == 'U' || c == 'u' ? 3 : -1; };
    while (std::getline(in, line)) {
        ++n;
        const auto bad = [&](const std::string &what) { return std::runtime_error("-W: " + path + ":" + std::to_string(n) + ": " + what); };
        std::istringstream is(line.substr(0, line.find('#')));
        std::vector<std::string> f;
        for (std::string w; is >> w;) f.push_back(w);
        if (f.empty()) continue;
        const auto integer = [&](const std::string &v) {
            char *e = nullptr;
            const long x = std::strtol(v.c_str(), &e, 10);
            if (e == v.c_str() || *e || x < 0 || x > 64) throw bad("'" + v + "' is no position");
            return (uint32_t)x;
        };
        const auto number = [&](const std::string &v) {
            char *e = nullptr;
            const double x = std::strtod(v.c_str(), &e);
            if (e == v.c_str() || *e || !std::isfinite(x)) throw bad("'" + v + "' is no finite number");
            return x;
        };
        if (f[0] != "shape" && !have_shape) throw bad("'" + f[0] + "' before the 'shape' line");
        if (f[0] == "shape" && f.size() == 4 && !have_shape) {
            s.len = integer(f[1]), s.ps_start = integer(f[2]), s.ps_len = integer(f[3]);
            if (s.ps_len < 1 || s.ps_len > 32) throw bad("the protospacer has 1..32 positions");
            pair.assign((size_t)s.ps_len * 16, NAN);
            for (uint32_t i = 0; i < s.ps_len; ++i)
                for (uint32_t b = 0; b < 4; ++b) pair[(i * 4 + b) * 4 + b] = 1.0;
            have_shape = true;
        } else if (f[0] == "pam_pos" && f.size() <= 5 && !have_pam_pos) {
            s.n_pam = (uint32_t)f.size() - 1;
            for (uint32_t t = 0; t < s.n_pam; ++t) s.pam_pos[t] = integer(f[1 + t]);
            pam.assign((size_t)1 << (2 * s.n_pam), NAN);
            have_pam_pos = true;
        } else if (f[0] == "pair" && f.size() == 5 && f[2].size() == 1 && f[3].size() == 1) {
            const uint32_t j = integer(f[1]);
            const int g = base(f[2][0]), b = base(f[3][0]);
            if (j < s.ps_start || j >= s.ps_start + s.ps_len) throw bad("position " + f[1] + " lies outside the protospacer");
            if (g < 0 || b < 0) throw bad("'" + f[2] + "' or '" + f[3] + "' is no base");
            pair[((size_t)(j - s.ps_start) * 4 + (size_t)g) * 4 + (size_t)b] = number(f[4]);
        } else if (f[0] == "pam" && f.size() == 3) {
            const std::string letters = f[1] == "-" ? "" : f[1];
            if (letters.size() != s.n_pam) throw bad("'pam' takes one letter per PAM position");
            size_t k = 0;
            for (char c : letters) {
                if (base(c) < 0) throw bad("'" + f[1] + "' holds a letter that is no base");
                k = 4 * k + (size_t)base(c);
            }
            have_pam_pos = true;  // (a 'pam_pos' line behind a weight would resize the weights)
            pam[k] = number(f[2]);
        } else {
            throw bad("unknown key, a line given twice or wrong number of fields");
        }
    }
    if (!have_shape) throw std::runtime_error("-W: " + path + ": no 'shape' line");
    size_t missing = 0;
    for (double w : pair) missing += std::isnan(w);
    for (double w : pam) missing += std::isnan(w);
    if (missing) throw std::runtime_error("-W: " + path + ": " + std::to_string(missing) + " entries are missing");
    vsc_pattern_table *t = nullptr;
    if (vsc_pattern_table_build(&s, pair.data(), pam.data(), &t) != VSC_OK)
        throw std::runtime_error("-W: " + path + ": not a table (a bad shape, a weight outside 0 .. 1 or a diagonal entry that is not 1)");
    *shape = s;
    return t;
}

}  // namespace

int main(int argc, char **argv)
{
    std::vector<Option> opts = {
        {'i', "index", "Prefix of the packed genome (bidir_index -I)", true},
        {'q', "pattern", "IUPAC pattern of 16..32 letters that a site must satisfy, e.g. NNNNNNNNNNNNNNNNNNNNNGRRT", true},
        {'R', "guides", "FASTA of the guides: IUPAC records of the pattern's length, N = position not compared", false},
        {'M', "mismatches", "Number of allowed mismatches (0..8)", false},
        {'D', "device", "HIP device index (default 0)", false},
        {'O', "output", "Summary TSV: #guideId guideSeq offtargetCount mm0 .. mm<M>", false},
        {'T', "hits", "Hits TSV: #guideId chrom start end strand mismatches mismatchPositions sequence", false},
        {'E', "enumerate", "Guides TSV: #guide chrom pos strand - the guides are FOUND in the genome instead of read from -R "
                           "(needs -p; with -M and -O they are screened in the same run, their own locus not counted)", false},
        {'B', "targets", "With -E: target intervals (.bed, BED3+); without, the whole genome is enumerated", false},
        {'p', "protospacer", "With -E or -u: START,LENGTH of the protospacer in the pattern (SaCas9 0,21; Cas12a 4,23); the -E filters look "
                             "at it, the bulges of -u lie in it", false},
        {'r', "rule", "With -B: overlap (default; the site shares a base with a target) or inside (it lies in one target)", false},
        {'s', "strands", "With -E: both (default), + or -", false},
        {'g', "gc", "With -E: MIN,MAX number of G/C in the protospacer (MAX 0: no upper bound)", false},
        {'t', "t-run", "With -E: longest run of T allowed in the protospacer (0: no limit)", false},
        {'u', "bulges", "DNA,RNA: largest DNA and RNA bulge, 0 .. 2 each (e.g. 1,1; needs -p): adds the bulged sites - -O gains bulgeCount "
                        "and <class>mm0 .. <class>mm<M> (br2 br1 bd1 bd2)", false},
        {'U', "bulge-hits", "Path to the TSV file of the bulged sites (.tsv/.txt); needs -u", false},
        {'Y', "efficiency-model", "With -E: path to an on-target efficiency model (.tsv/.txt) whose site_len is the pattern's length: "
                                  "the -E listing gains the columns efficiencyLinear efficiency", false},
        {'y', "min-efficiency", "With -Y: keep only the candidates whose efficiency predictor is defined and >= this value, linear domain", false},
        {'W', "score-table", "Path to a pattern score table (.tsv/.txt; what PatternTable.to_tsv writes) of the pattern's length: -O gains the "
                             "columns tableScoreSum tableSpecScore tablePositive, -T the column tableScore", false},
        {'K', "top", "With -W: list the K best hits of every guide by table score in the -T file (default: no limit)", false},
        {'S', "min-score", "With -W: list only hits with a table score >= this value, 0 .. 1, in the -T file (default: no floor)", false},
        {'Z', "sites", "Path to the TSV file of the cut sites (.tsv/.txt): the plain and the bulged alignments collapsed per PAM-side end; "
                       "-O gains siteCount siteBulgeOnly; needs -u and a -p protospacer at one end of the pattern", false},
        {'w', "bulge-table", "Path to the bulge weights (.tsv/.txt; lines 'dna j s w' and 'rna j g w', j = read position in the protospacer) beside "
                             "the -W table: the cut sites are scored; -O gains siteScoreSum siteSpecScore sitePositive, the -Z file tableScore "
                             "scoredAs, and -K / -S cut the -Z listing by the site's score; needs -W, -u, -p and -Z", false},
        {'v', "vcf", "Path to a .vcf file: the guides are screened in that individual's genome as well (variant windows of the pattern's "
                     "length; the reference hits no window shadows plus the window hits) - -O gains indCount imm0 .. imm<M> varCount "
                     "vmm0 .. vmm<M> varDuplicates refShadowed, with -W also indScoreSum indSpec varScoreSum; needs -O and -M, not with "
                     "-u -U -Z -w -T -K -S", false},
        {'n', "sample", "With -v: 0-based sample column of the .vcf file (default 0)", false},
        {'H', "microhomology", "With -E: FLANK[,CUT]: the -E listing gains the columns mhScore oofScore (the microhomology score of Bae et al. "
                               "2014 and its out-of-frame share in per cent) over FLANK bases (8 .. 32) on either side of the break in front "
                               "of read position CUT (default: 3 bases before the end of a -p protospacer that starts the pattern, else 18 "
                               "bases behind its start)", false},
        {'m', "min-out-of-frame", "With -H: MIN_OOF[,MIN_MH]: keep only the candidates whose out-of-frame share is at least MIN_OOF per cent "
                                  "and whose microhomology score is at least MIN_MH", false},
        {'k', "pick", "With -E and -B: K[,SPACING]: pick the K best guides (1 .. 32) of every -B target, their cut sites at least SPACING bases "
                      "apart; the -E listing gains the columns pickTarget pickRank", false},
        {'b', "pick-by", "With -k: what to rank by, comma-separated in priority order, out of table (needs -W, -M and -O), eff (needs -Y), oof, mh "
                         "(need -H); the default, mit, is guide_summary's: give -b", false},
        {'c', "pick-target", "With -k: interval (default; every -B interval is a target) or name (the -B intervals with one BED name are one target)", false},
        {'x', "editor", "With -E: CBE | ABE | START,LEN,BASE: the base editor's window in read positions of the site and the base it converts; "
                        "the -E listing gains the last columns editWindow editable targetsHit", false},
        {'z', "edit-targets", "With -x: path to the target bases (.bed, one base per line): only the candidates whose window holds a target base "
                              "that the editor converts are kept", false},
        {'l', "editable", "With -x: MIN,MAX: keep only the candidates with MIN .. MAX editable bases in the window (0 .. 16)", false},
        {'o', "edit-pairs", "With -z: path to the listing of the pairs: #chrom pos guideId at bystanders", false},
        {'d', "cds", "With -x: path to the coding segments (.bed, BED6: chrom start end transcript phase strand): the -E listing gains the "
                     "last columns codingEdits stopGained missense synonymous - what the editor's full conversion does to the codons", false},
        {'2', "edit-to", "With --cds: the base the editor writes on the read strand (default: the transition partner of the base of -x)", false},
        {'f', "effect-filter", "With --cds: REQUIRE[/FORBID], class names joined by + (synonymous missense stop_gained stop_lost start_lost "
                               "unknown): keep only the candidates with an effect of a REQUIRE class and none of a FORBID class", false},
        {'Q', "effects", "With --cds: path to the listing of the effects: #guideId transcript codon ref alt refAA altAA class at", false},
        {'3', "prime", "With -E: NICK,DOWN,PBSMIN,PBSMAX,RTTMIN,RTTMAX,HOMOLOGY,PAMSTART,PAMLEN,SEEDSTART,SEEDLEN,AVOIDG (or PE2 for sites of 23 "
                       "bases): the prime editor's shape; only the candidates with a defined context are kept, and the -E listing gains the last "
                       "columns pbsLen pbsGC primePairs", false},
        {'4', "prime-edits", "With --prime: path to the wanted edits (.tsv/.txt: chrom pos ref-length alt-letters-or--): only the candidates that "
                             "can write one of them are kept", false},
        {'5', "prime-allow-weak", "With --prime: keep the candidates whose primer binding site is WEAK", false, false},
        {'6', "prime-out", "With --prime-edits: path to the listing of the pairs: #chrom pos guideId pbsLen rttLen nickToEdit homology flags "
                           "extension", false},
        {'7', "variants", "With -E: path to known variants (.vcf: POS 1-based, one variant per ALT allele; or a TSV: chrom pos ref alt [weight], pos "
                          "0-based): the variants under every found guide's own site are joined with it on the device (one device)", false},
        {'8', "variant-af", "With --variants (a VCF): the INFO key of the allele frequency; a variant's weight is round(-log1p(-AF) * 2^20)", false},
        {'9', "variant-seed", "With --variants: the seed, the N protospacer bases next to the PAM (default 10)", false},
        {'0', "max-variant-cost", "With --variants: keep only the candidates whose cost (the sum of their disrupting variants' weights) is at most this", false},
        {'1', "max-variants-by-zone", "With --variants: a,b,c,d: keep only the candidates with at most a, b, c, d disrupting variants whose top zone is "
                                      "none, distal, seed, pam (255: no bound)", false},
        {'@', "require-variant-zones", "With --variants: zones out of none, distal, seed, pam: keep only the candidates with a disrupting variant "
                                       "in one of them (allele-specific design)", false},
        {'%', "variation-out", "With --variants: path to the TSV of the guides' rows (#guideId none distal seed pam silent cost maxWeight) and, "
                               "behind a blank line, of the pairs (#chrom pos span alt guideId first touched top silent weight)", false},
        {'^', "hdr", "With -E: SpCas9 | Cas12a | UP,DOWN,CUT,MAXDIST,ANCHOR,PAMSTART,PAM,SEEDSTART,SEEDLEN,PROTOSTART,PROTOLEN,MINSEED,MINPROTO,FLAGS: "
                     "the cutting nuclease's shape for knock-ins by homology-directed repair; only the candidates with a defined context are "
                     "kept, and the guide listing gains the last columns hdrPairs hdrUsable (one device)", false},
        {'&', "hdr-edits", "With --hdr: path to the wanted edits (.tsv/.txt: chrom pos ref-length alt-letters-or--): only the candidates with a "
                           "usable pair are kept", false},
        {'=', "hdr-out", "With --hdr-edits: path to the listing of the pairs: #chrom pos guideId dist seedMm protoMm flags subChrom subPos subBase", false},
        {'+', "hdr-cds", "With --hdr: path to the coding segments (.bed, BED6 as --cds): a blocking substitution inside them is synonymous", false},
        {'~', "hdr-allow-open", "With --hdr: keep the candidates with a pair whose repaired allele can be cut again", false, false},
        {'!', "fold", "With -E: SpCas9 | Cas12a | SITELEN,PROTOSTART,PROTOLEN,STEM,GCMIN,MINLOOP,SEEDSTART,SEEDLEN,FLAGS: how the guide RNA's "
                      "self-complementarity is counted; the guide listing gains the last columns foldStarts foldSelf foldScaffold foldSeed "
                      "(one device)", false},
        {':', "fold-scaffold", "With --fold: the constant part of the guide RNA, 5' to 3', at most 128 letters of A C G T U, or @FILE", false},
        {';', "max-fold", "With --fold: STARTS[,SELF[,SCAF[,SEED]]] - only the candidates with at most so many stem starts, so long a "
                          "hairpin stem, so long a scaffold stem and so many paired seed bases (each 0 .. 32, - for no limit)", false},
        {'[', "motifs", "With -E: path to the motifs (.tsv: name, IUPAC text of 2 .. 16 letters, 1 or 2 strands; at most 63): restriction sites "
                        "in the cloned construct and the genomic context; the guide listing gains the last columns motifsConstruct motifsCut "
                        "motifsElsewhere motifsCutOnly (one device)", false},
        {']', "motif-left", "With --motifs: the vector's text in front of the cloned spacer, at most 16 letters of A C G T U", false},
        {'{', "motif-right", "With --motifs: the vector's text behind the cloned spacer, at most 16 letters of A C G T U", false},
        {'}', "motif-forbid", "With --motifs: NAMES - drop the candidates whose construct holds one of these motifs", false},
        {'<', "motif-forbid-context", "With --motifs: NAMES - drop the candidates whose genomic context holds one of these motifs", false},
        {'>', "motif-require-cut", "With --motifs: NAMES - keep the candidates with one of these motifs over the cut zone", false},
        {'/', "motif-cut-only", "With --motif-require-cut: ... and nowhere else in the context", false, false},
        {'?', "motifs-out", "With --motifs: path to the listing, one line per candidate: #guideId construct cut elsewhere cutOnly (names)", false},
        {0, "knockout", "With -E: knock-out design - where the cut of every found guide falls in the coding sequence of --knockout-cds and what "
                        "a frameshift there does; CUT = the break lies between read positions CUT - 1 and CUT (default: 17 for sites of 23 "
                        "bases, 22 for sites of 27); the guide listing gains the last columns koTranscript koCodon koFrame koCutPct koEdge "
                        "koPtc1 koPtc2 koNmd (one device)", false},
        {0, "knockout-cds", "With --knockout: path to the coding segments (.bed, BED6: chrom start end transcript phase strand)", false},
        {0, "knockout-nmd", "With --knockout: WINDOW[,START] - a premature stop triggers nonsense-mediated decay when it ends at least WINDOW "
                            "coding bases in front of the last exon-exon junction (default 50) and begins at least START behind the first "
                            "coding base (default 0: off)", false},
        {0, "knockout-filter", "With --knockout: MINPCT,MAXPCT[,EDGE[,REQUIRE[/FORBID]]] - only the coding cuts between MINPCT and MAXPCT per cent "
                               "of the protein, at least EDGE bases from the exon's ends, with every REQUIRE and no FORBID flag (names joined "
                               "by + out of first last ptc1 ptc2 nmd1 nmd2 unknown)", false},
        {0, "knockout-out", "With --knockout: path to the listing, one line per candidate: #guideId, the eight columns, koFlags", false},
    };
    opts[65].optional_value = true;  // --knockout [CUT]
    const int pr = parse_args(argc, argv, opts, "Pattern search",
                              "Off-target search for any PAM and any guide of 16..32 bases: the sites of the genome that satisfy "
                              "the pattern and differ from a guide in at most -M compared positions. Give -O, -T or both. "
                              "With -E the guides are enumerated from the genome or the -B targets.");
    if (pr) return pr == 1;
    const std::string prefix = opts[0].value, pattern = opts[1].value, guides_path = opts[2].value;
    const bool enumerate = opts[7].set;
    if (!enumerate)
        for (int k : {2, 3})
            if (!opts[k].set) {
                std::fprintf(stderr, "%s: Missing value for option: -%c\n", argv[0], opts[k].short_name);
                return 1;
            }
    if (pattern.size() < VSC_PATTERN_MIN_LEN || pattern.size() > VSC_PATTERN_MAX_LEN) {
        std::fprintf(stderr, "%s: the pattern must have 16..32 letters, '%s' has %zu\n", argv[0], pattern.c_str(), pattern.size());
        return 1;
    }
    for (char c : pattern)
        if (!iupac(c)) {
            std::fprintf(stderr, "%s: '%c' in the pattern '%s' is no IUPAC letter\n", argv[0], c, pattern.c_str());
            return 1;
        }
    if ((opts[2].set && !has_extension(guides_path, {"fa", "fasta"})) || (opts[5].set && !has_extension(opts[5].value, {"tsv", "txt"})) ||
        (opts[6].set && !has_extension(opts[6].value, {"tsv", "txt"}))) {
        std::fprintf(stderr, "%s: the guides must be a .fa/.fasta file, the outputs .tsv/.txt files\n", argv[0]);
        return 1;
    }
    const bool bulged = opts[14].set;
    const bool sited = opts[21].set;
    // -v / -n: the individual
    const bool individual = opts[23].set;
    uint32_t vcf_sample = 0;
    if (individual && !has_extension(opts[23].value, {"vcf"})) {
        std::fprintf(stderr, "%s: the -v file must be a .vcf file\n", argv[0]);
        return 1;
    }
    if (individual && (opts[14].set || opts[15].set || opts[21].set || opts[22].set || opts[6].set || opts[19].set || opts[20].set)) {
        std::fprintf(stderr, "%s: -v screens plain pattern hits per guide: it does not combine with -u, -U, -Z, -w, -T, -K or -S\n", argv[0]);
        return 1;
    }
    if (individual && (!opts[5].set || !opts[3].set)) {
        std::fprintf(stderr, "%s: -v adds columns to the -O summary of a search: give -O and -M\n", argv[0]);
        return 1;
    }
    if (opts[24].set) {
        const std::string &v = opts[24].value;
        char *nend = nullptr;
        const long long k = std::strtoll(v.c_str(), &nend, 10);
        if (!individual || v.empty() || *nend || k < 0 || k > 0xFFFFFFFFll) {
            std::fprintf(stderr, "%s: -n takes the 0-based sample column of the -v file, not '%s'\n", argv[0], v.c_str());
            return 1;
        }
        vcf_sample = (uint32_t)k;
    }
    if (!enumerate && !opts[5].set && !opts[6].set && !(bulged && (opts[15].set || sited))) {
        std::fprintf(stderr, "%s: give -O, -T or both\n", argv[0]);
        return 1;
    }
    vsc_pattern_enum_params ep{};
    if (!enumerate) {
        for (int k = 8; k <= 13; ++k)
            if (opts[k].set && !(k == 9 && bulged)) {
                std::fprintf(stderr, "%s: -%c belongs to the enumeration: give -E\n", argv[0], opts[k].short_name);
                return 1;
            }
    } else {
        if (opts[2].set || opts[6].set) {
            std::fprintf(stderr, "%s: -E finds the guides in the genome: -R and -T cannot be given with it\n", argv[0]);
            return 1;
        }
        if (opts[3].set != opts[5].set) {
            std::fprintf(stderr, "%s: with -E, -M and -O go together (the screened rows) or are both left out\n", argv[0]);
            return 1;
        }
        if (!has_extension(opts[7].value, {"tsv", "txt"}) || (opts[8].set && !has_extension(opts[8].value, {"bed"}))) {
            std::fprintf(stderr, "%s: the -E output must be a .tsv/.txt file, the -B targets a .bed file\n", argv[0]);
            return 1;
        }
        long a = 0, k = 0;
        if (!opts[9].set || !two_numbers(opts[9].value, &a, &k) || k < 1 || a + k > (long)pattern.size()) {
            std::fprintf(stderr, "%s: -E needs -p START,LENGTH with 1 <= LENGTH and START + LENGTH <= %zu, the pattern's length\n", argv[0], pattern.size());
            return 1;
        }
        ep.ps_start = (uint8_t)a;
        ep.ps_len = (uint8_t)k;
        if (opts[10].set) {
            if (!opts[8].set || (opts[10].value != "overlap" && opts[10].value != "inside")) {
                std::fprintf(stderr, "%s: -r takes overlap or inside and needs -B\n", argv[0]);
                return 1;
            }
            ep.rule = opts[10].value == "inside" ? VSC_REGION_INSIDE : VSC_REGION_OVERLAP;
        }
        if (opts[11].set) {
            const std::string &s = opts[11].value;
            if (s != "both" && s != "+" && s != "-") {
                std::fprintf(stderr, "%s: -s takes both, + or -\n", argv[0]);
                return 1;
            }
            ep.strands = s == "both" ? 0 : (s == "+" ? 1 : 2);
        }
        if (opts[12].set) {
            long lo = 0, hi = 0;
            if (!two_numbers(opts[12].value, &lo, &hi) || lo > k || hi > k || (hi && lo > hi)) {
                std::fprintf(stderr, "%s: -g takes MIN,MAX with MIN <= MAX <= %ld, the protospacer's length (MAX 0: no upper bound)\n", argv[0], k);
                return 1;
            }
            ep.gc_min = (uint8_t)lo;
            ep.gc_max = (uint8_t)hi;
        }
        if (opts[13].set) {
            char *e = nullptr;
            const long run = std::strtol(opts[13].value.c_str(), &e, 10);
            if (e == opts[13].value.c_str() || *e || run < 0 || run > 255) {
                std::fprintf(stderr, "%s: -t takes a run length of 0..255\n", argv[0]);
                return 1;
            }
            ep.max_t_run = (uint8_t)run;
        }
    }
    // -u / -U: the bulged sites
    vsc_pattern_bulge_params bp{};
    if (bulged) {
        long dna = 0, rna = 0, a = 0, k = 0;
        if (!two_numbers(opts[14].value, &dna, &rna) || dna > 2 || rna > 2 || (dna == 0 && rna == 0)) {
            std::fprintf(stderr, "%s: -u takes DNA,RNA, the largest bulges, 0 .. 2 each and not both 0 (e.g. 1,1), not '%s'\n", argv[0], opts[14].value.c_str());
            return 1;
        }
        if (!opts[9].set || !two_numbers(opts[9].value, &a, &k) || k < 4 || a + k > (long)pattern.size()) {
            std::fprintf(stderr, "%s: -u needs -p START,LENGTH with 4 <= LENGTH and START + LENGTH <= %zu, the pattern's length\n", argv[0], pattern.size());
            return 1;
        }
        for (long j = a; j < a + k; ++j)
            if (pattern[(size_t)j] != 'N' && pattern[(size_t)j] != 'n') {
                std::fprintf(stderr, "%s: -u: the pattern must be N at every position of the -p protospacer\n", argv[0]);
                return 1;
            }
        if ((long)pattern.size() + dna > VSC_PATTERN_MAX_LEN || (long)pattern.size() - rna < VSC_PATTERN_MIN_LEN) {
            std::fprintf(stderr, "%s: -u: the pattern's length + DNA must not exceed 32 and its length - RNA must be at least 16\n", argv[0]);
            return 1;
        }
        if (enumerate && !opts[3].set) {
            std::fprintf(stderr, "%s: with -E, -u screens the found guides: give -M and -O\n", argv[0]);
            return 1;
        }
        bp.proto_start = (uint32_t)a;
        bp.proto_len = (uint32_t)k;
        bp.dna_max = (uint32_t)dna;
        bp.rna_max = (uint32_t)rna;
    }
    if (opts[15].set && (!bulged || !has_extension(opts[15].value, {"tsv", "txt"}))) {
        std::fprintf(stderr, "%s: -U lists the bulged sites of -u in a .tsv/.txt file: give -u\n", argv[0]);
        return 1;
    }
    vsc_site_params sp{};
    if (sited) {
        if (!bulged || !has_extension(opts[21].value, {"tsv", "txt"})) {
            std::fprintf(stderr, "%s: -Z lists the cut sites of -u in a .tsv/.txt file: give -u\n", argv[0]);
            return 1;
        }
        if (bp.proto_start != 0 && bp.proto_start + bp.proto_len != pattern.size()) {
            std::fprintf(stderr, "%s: -Z: the -p protospacer must start or end the pattern (the other end is the sites' fixed end)\n", argv[0]);
            return 1;
        }
        sp.len = (uint32_t)pattern.size();
        sp.anchor = bp.proto_start == 0 ? VSC_SITE_ANCHOR_END : VSC_SITE_ANCHOR_START;
    }
    // -Y / -y: the efficiency model of the found guides
    const bool efficient = opts[16].set;
    double min_eff = 0.0;
    if (opts[17].set && !efficient) {
        std::fprintf(stderr, "%s: -y is a floor on the efficiency predictor of the -Y model: give -Y\n", argv[0]);
        return 1;
    }
    if (efficient && !enumerate) {
        std::fprintf(stderr, "%s: -Y scores the guides that -E finds: give -E\n", argv[0]);
        return 1;
    }
    if (efficient && !has_extension(opts[16].value, {"tsv", "txt"})) {
        std::fprintf(stderr, "%s: the -Y model must be a .tsv/.txt file\n", argv[0]);
        return 1;
    }
    if (opts[17].set) {
        const std::string &v = opts[17].value;
        char *yend = nullptr;
        min_eff = std::strtod(v.c_str(), &yend);
        if (v.empty() || *yend || min_eff != min_eff) {
            std::fprintf(stderr, "%s: -y takes a floor on the linear predictor, a number, not '%s'\n", argv[0], v.c_str());
            return 1;
        }
    }
    // -H / -m: the microhomology scores of the found guides
    MhOptions mh;
    {
        const uint32_t plen = (uint32_t)pattern.size();
        uint32_t cut = ep.ps_start == 0 ? (ep.ps_len >= 3 ? ep.ps_len - 3 : 0) : ep.ps_start + 18;
        if (cut > plen) cut = plen;
        const std::string why = parse_mh_options(opts[25].set, opts[25].value, opts[26].set, opts[26].value, enumerate, plen, cut, &mh);
        if (!why.empty()) {
            std::fprintf(stderr, "%s: %s\n", argv[0], why.c_str());
            return 1;
        }
    }
    // -x / -z / -l / -o: the base-editor windows of the found guides
    EditOptions edit;
    {
        const std::string why = parse_edit_options(opts[30].set, opts[30].value, opts[31].set, opts[31].value, opts[32].set, opts[32].value,
                                                   opts[33].set, opts[33].value, enumerate, opts[4].value.find(',') != std::string::npos,
                                                   (uint32_t)pattern.size(), &edit);
        if (!why.empty()) {
            std::fprintf(stderr, "%s: %s\n", argv[0], why.c_str());
            return 1;
        }
    }
    // --cds / --edit-to / --effect-filter / --effects: what the editor does to the codons
    EffectsOptions fx;
    {
        const std::string why = parse_effects_options(opts[34].set, opts[34].value, opts[35].set, opts[35].value, opts[36].set, opts[36].value,
                                                      opts[37].set, opts[37].value, edit, &fx);
        if (!why.empty()) {
            std::fprintf(stderr, "%s: %s\n", argv[0], why.c_str());
            return 1;
        }
    }
    CdsOfFile coding;
    // --prime / --prime-edits / --prime-allow-weak / --prime-out: the pegRNA extensions of the found guides
    PrimeOptions prime;
    {
        const std::string why = parse_prime_options(opts[38].set, opts[38].value, opts[39].set, opts[39].value, opts[40].set, opts[41].set,
                                                    opts[41].value, enumerate, opts[4].value.find(',') != std::string::npos,
                                                    (uint32_t)pattern.size(), &prime);
        if (!why.empty()) {
            std::fprintf(stderr, "%s: %s\n", argv[0], why.c_str());
            return 1;
        }
    }
    // --hdr / --hdr-edits / --hdr-out / --hdr-cds / --hdr-allow-open: knock-in design for the found guides
    HdrOptions hdr;
    {
        const std::string why = parse_hdr_options(opts[49], opts[50], opts[51], opts[52], opts[53], enumerate, opts[4].value.find(',') != std::string::npos, (uint32_t)pattern.size(), &hdr);
        if (!why.empty()) {
            std::fprintf(stderr, "%s: %s\n", argv[0], why.c_str());
            return 1;
        }
    }
    CdsOfFile hdr_coding;
    // --fold / --fold-scaffold / --max-fold: the self-complementarity of the found guides
    FoldOptions fold;
    {
        const std::string why = parse_fold_options(opts[54], opts[55], opts[56], enumerate, opts[4].value.find(',') != std::string::npos, (uint32_t)pattern.size(), &fold);
        if (!why.empty()) {
            std::fprintf(stderr, "%s: %s\n", argv[0], why.c_str());
            return 1;
        }
    }

    // --motifs and its options: restriction sites and motifs in the found guides' construct and context
    MotifOptions motif;
    {
        const std::string why = parse_motif_options(opts[57], opts[58], opts[59], opts[60], opts[61], opts[62], opts[63], opts[64], enumerate,
                                                    opts[4].value.find(',') != std::string::npos, (uint32_t)pattern.size(), &motif);
        if (!why.empty()) {
            std::fprintf(stderr, "%s: %s\n", argv[0], why.c_str());
            return 1;
        }
    }

    // --knockout and its options: where the found guides cut the coding sequence, and what a frameshift there does
    KnockoutOptions knockout;
    {
        const std::string why = parse_knockout_options(opts[65], opts[66], opts[67], opts[68], opts[69], enumerate, opts[4].value.find(',') != std::string::npos, (uint32_t)pattern.size(), &knockout);
        if (!why.empty()) {
            std::fprintf(stderr, "%s: %s\n", argv[0], why.c_str());
            return 1;
        }
    }
    CdsOfFile knockout_coding;

    // --variants and its options: the known variants under the found guides' own sites
    VariationOptions variation;
    {
        const std::string why = parse_variation_options(opts[42], opts[43], opts[44], opts[45], opts[46], opts[47], opts[48], enumerate,
                                                        opts[4].value.find(',') != std::string::npos, pattern, ep.ps_start, ep.ps_len, &variation);
        if (!why.empty()) {
            std::fprintf(stderr, "%s: %s\n", argv[0], why.c_str());
            return 1;
        }
    }
    // -W / -K / -S: the table score of the hits
    const bool tabled = opts[18].set;
    // -k / -b / -c: the best guides of every -B target
    PickOptions pick;
    // the cut that -H defaults to: three bases in front of a 3' PAM, 18 behind the start of a protospacer that follows a 5' PAM
    const uint32_t pick_cut = std::min<uint32_t>((uint32_t)pattern.size(), ep.ps_start == 0 ? (ep.ps_len >= 3 ? ep.ps_len - 3 : 0) : ep.ps_start + 18);
    {
        std::map<std::string, std::string> needs;
        needs["mit"] = "pattern hits have no MIT score; give -b";
        if (!tabled || !opts[3].set) needs["table"] = "give -W with -M and -O";
        if (!efficient) needs["eff"] = "give -Y";
        if (!mh.on) needs["oof"] = needs["mh"] = "give -H";
        const std::string why = parse_pick_options(opts[27].set, opts[27].value, opts[28].set, opts[28].value, opts[29].set, opts[29].value,
                                                   enumerate && opts[8].set, "-E -B", opts[4].value.find(',') != std::string::npos, needs, &pick);
        if (!why.empty()) {
            std::fprintf(stderr, "%s: %s\n", argv[0], why.c_str());
            return 1;
        }
    }
    vsc_pattern_select sel{};
    const bool site_scored = opts[22].set;
    if (site_scored && (!tabled || !bulged || !sited || !has_extension(opts[22].value, {"tsv", "txt"}))) {
        std::fprintf(stderr, "%s: -w scores the cut sites of -Z with the bulge weights of a .tsv/.txt file beside the -W table: give -W, -u, -p and -Z\n", argv[0]);
        return 1;
    }
    if ((opts[19].set || opts[20].set) && (!tabled || (!opts[6].set && !site_scored))) {
        std::fprintf(stderr, "%s: -K and -S select the -T listing by the score of the -W table: give -W and -T\n", argv[0]);
        return 1;
    }
    if (tabled && !has_extension(opts[18].value, {"tsv", "txt"})) {
        std::fprintf(stderr, "%s: the -W table must be a .tsv/.txt file\n", argv[0]);
        return 1;
    }
    if (tabled && !opts[3].set) {
        std::fprintf(stderr, "%s: -W scores the hits of a search: give -M (with -E: -M and -O)\n", argv[0]);
        return 1;
    }
    if (opts[19].set) {
        char *kend = nullptr;
        const std::string &v = opts[19].value;
        const long long k = std::strtoll(v.c_str(), &kend, 10);
        if (v.empty() || *kend || k < 1 || k > 0xFFFFFFFFll) {
            std::fprintf(stderr, "%s: -K takes a count of 1 or more, not '%s'\n", argv[0], v.c_str());
            return 1;
        }
        sel.top_k = (uint32_t)k;
    }
    if (opts[20].set) {
        char *send = nullptr;
        const std::string &v = opts[20].value;
        const double x = std::strtod(v.c_str(), &send);
        if (v.empty() || *send || !(x >= 0.0 && x <= 1.0)) {
            std::fprintf(stderr, "%s: -S takes a table score of 0 .. 1, not '%s'\n", argv[0], v.c_str());
            return 1;
        }
        sel.min_score = (uint32_t)std::ceil(x * 0x1p30);  // the smallest fixed-point score that is >= x
    }
    char *end = nullptr;
    long mm = 0;
    if (opts[3].set) {
        mm = std::strtol(opts[3].value.c_str(), &end, 10);
        if (end == opts[3].value.c_str() || *end) {
            std::fprintf(stderr, "%s: the given value '%s' cannot be casted to integer\n", argv[0], opts[3].value.c_str());
            return 1;
        }
        if (mm < 0 || mm > VSC_MAX_MISMATCHES) {
            std::fprintf(stderr, "Error: Maximum number of mismatches must lie between 0 and 8.\n");
            return 1;
        }
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
    vsc_pattern_guides *found = nullptr;
    vsc_bulge_hits *bulge_hits = nullptr;
    vsc_pattern_hits *site_plain = nullptr;
    vsc_sites *sites = nullptr;
    EffAnyModel eff_model;  // -Y: a linear model, or - a file with a `tree` line - a tree model
    vsc_pattern_table *table = nullptr;
    vsc_bulge_table *bulge_table = nullptr;
    vsc_sites *scored_sites = nullptr;
    vsc_windows *windows = nullptr;
    vsc_variant_map *vmap = nullptr;
    vsc_genome *win_genome = nullptr;
    int rc = 1;
    try {
        std::vector<FastaRecord> guides;
        const uint32_t len = (uint32_t)pattern.size();
        if (efficient) {  // (read before the index and the device: a model that does not fit costs nothing)
            vsc_eff_shape eff_shape{};
            eff_model = load_eff_any(opts[16].value, &eff_shape);
            if (eff_shape.site_len != len)
                throw std::runtime_error("-Y: the model's site_len is " + std::to_string(eff_shape.site_len) + "; the pattern has " + std::to_string(len) + " letters");
        }
        if (tabled) {  // (read before the index and the device, as the model is)
            vsc_pattern_table_shape table_shape{};
            table = load_pattern_table(opts[18].value, &table_shape);
            if (table_shape.len != len)
                throw std::runtime_error("-W: the table is built for " + std::to_string(table_shape.len) + " letters; the pattern has " + std::to_string(len));
            if (site_scored) {
                if (table_shape.ps_start != bp.proto_start || table_shape.ps_len != bp.proto_len)
                    throw std::runtime_error("-w: the -W table's protospacer is not the -p protospacer");
                bulge_table = read_bulge_table(opts[22].value, "-w", table);
            }
        }
        std::string letters;
        if (!enumerate) {
            guides = read_fasta(guides_path);
            for (const auto &g : guides) {
                if (g.seq.size() != len)
                    throw std::runtime_error("guide '" + g.id + "' has " + std::to_string(g.seq.size()) + " letters, the pattern has " + std::to_string(len));
                for (char c : g.seq)
                    if (!iupac(c)) throw std::runtime_error("guide '" + g.id + "' holds '" + std::string(1, c) + "', which is no IUPAC letter");
                letters += g.seq;
            }
            std::printf("Guides loaded (total: %zu).\n", guides.size());
        }
        const PackedIndex ix = read_index(prefix);
        std::vector<vsc_interval> targets;
        if (opts[8].set) targets = read_targets(opts[8].value, ix);
        std::vector<uint32_t> pick_group;       // -k -c name: the target of every -B interval
        std::vector<std::string> target_names;  // -k: what pickTarget prints per target
        if (pick.on) pick_targets(pick, opts[8].value, "-B", &pick_group, &target_names);  // (before a device is opened: -c name may refuse the file)
        int st = vsc_ctx_create((int)device, &ctx);
        if (st != VSC_OK) throw std::runtime_error(st == VSC_ERR_NODEVICE ? "no HIP device available (there is no CPU fallback)" : "could not create the device context");
        st = vsc_genome_load(ctx, ix.hi.data(), ix.lo.data(), ix.nm.data(), 0, ix.hi.size(), ix.hi.size(), ix.contigs.data(),
                             (uint32_t)ix.contigs.size(), &genome);
        if (st != VSC_OK) throw std::runtime_error(vsc_last_error(ctx));
        std::printf("Index loaded.\n");

        const vsc_locus *loci = nullptr;
        std::vector<double> eff_linear;       // -Y: the found guides' predictors
        std::vector<uint32_t> mh_pairs;       // -H: their (sum, oof) pairs
        std::vector<std::string> pick_lines;  // -k: the -E lines wait for the search, whose rows the picks may rank by
        std::vector<std::string> edit_cols;   // -k with -x: the edit columns stay the last ones, behind the picks'
        std::vector<uint32_t> own_fixed;  // -E with -W: the table score of every found guide against its own site
        if (enumerate) {
            // an empty -B file is a target set that holds nothing: a pointer that is not NULL with n = 0
            const vsc_interval none{};
            st = vsc_guides_enumerate_pattern(ctx, genome, pattern.c_str(), len, &ep, opts[8].set ? (targets.empty() ? &none : targets.data()) : nullptr,
                                              targets.size(), &found);
            if (st != VSC_OK) throw std::runtime_error(vsc_last_error(ctx));
            if (efficient) {  // -y: the survivors replace the candidates; -Y: their predictors, where they lie
                if (opts[17].set) {
                    vsc_pattern_guides *kept = nullptr;
                    if (eff_any_filter(ctx, genome, found, eff_model, min_eff, &kept) != VSC_OK) throw std::runtime_error(vsc_last_error(ctx));
                    vsc_pattern_guides_free(found);
                    found = kept;
                }
            }
            if (mh.floored) {  // -m: the same for the microhomology floors
                vsc_pattern_guides *kept = nullptr;
                if (vsc_pattern_guides_filter_microhomology(ctx, genome, found, &mh.shape, mh.min_sum, mh.min_oof_permille, &kept) != VSC_OK)
                    throw std::runtime_error(vsc_last_error(ctx));
                vsc_pattern_guides_free(found);
                found = kept;
            }
            std::vector<vsc_edit_target> edit_targets;
            if (edit.with_targets) edit_targets = read_edit_targets(edit.targets_path, ix.names);
            if (edit.filtered) {  // -z / -l: the same for the editor's FILTER
                vsc_pattern_guides *kept = nullptr;
                if (vsc_pattern_guides_filter_edit(ctx, genome, found, &edit.shape, edit_targets.empty() ? nullptr : edit_targets.data(),
                                                   edit_targets.size(), edit.min_editable, edit.max_editable, &kept) != VSC_OK)
                    throw std::runtime_error(vsc_last_error(ctx));
                vsc_pattern_guides_free(found);
                found = kept;
            }
            if (fx.on) read_cds(fx.cds_path, ix.names, ix.contigs, &coding);
            if (fx.filtered) {  // --effect-filter: the same for the effects' FILTER, after the editor's
                vsc_pattern_guides *kept = nullptr;
                if (vsc_pattern_guides_filter_effects(ctx, genome, found, &edit.shape, fx.to, coding.cds, nullptr, fx.require, fx.forbid, &kept) != VSC_OK)
                    throw std::runtime_error(vsc_last_error(ctx));
                vsc_pattern_guides_free(found);
                found = kept;
            }
            std::vector<vsc_prime_edit> prime_edits;
            if (prime.with_edits) prime_edits = read_prime_edits(prime.edits_path, ix.names);
            if (prime.on) {  // --prime: the same for the prime editor's FILTER, after the editor's and the effects'
                vsc_pattern_guides *kept = nullptr;
                if (vsc_pattern_guides_filter_prime(ctx, genome, found, &prime.shape, prime_edits.empty() ? nullptr : prime_edits.data(),
                                                    prime_edits.size(), prime.allow_weak, &kept) != VSC_OK)
                    throw std::runtime_error(vsc_last_error(ctx));
                vsc_pattern_guides_free(found);
                found = kept;
            }
            std::vector<vsc_variant> variants;
            if (variation.on) variants = read_variants(variation, ix.names, ix.contigs);
            if (variation.filtered) {  // the bounds and the required zones: the same for the variation FILTER, after all others
                vsc_pattern_guides *kept = nullptr;
                if (vsc_pattern_guides_filter_variation(ctx, genome, found, &variation.shape, variants.empty() ? nullptr : variants.data(),
                                                        variants.size(), &variation.filter, &kept) != VSC_OK)
                    throw std::runtime_error(vsc_last_error(ctx));
                vsc_pattern_guides_free(found);
                found = kept;
            }
            std::vector<vsc_prime_edit> hdr_edits;
            if (hdr.with_edits) hdr_edits = read_prime_edits(hdr.edits_path, ix.names);
            if (hdr.with_cds) read_cds(hdr.cds_path, ix.names, ix.contigs, &hdr_coding);
            if (hdr.on) {  // --hdr: the same for the knock-in FILTER, after all others
                vsc_pattern_guides *kept = nullptr;
                if (vsc_pattern_guides_filter_hdr(ctx, genome, found, &hdr.shape, hdr_edits.empty() ? nullptr : hdr_edits.data(), hdr_edits.size(), hdr_coding.cds,
                        nullptr, hdr.allow_open, &kept) != VSC_OK)
                    throw std::runtime_error(vsc_last_error(ctx));
                vsc_pattern_guides_free(found);
                found = kept;
            }
            if (fold.limited) {  // --max-fold: the same for the fold limits, after the knock-in FILTER
                vsc_pattern_guides *kept = nullptr;
                if (vsc_pattern_guides_filter_fold(ctx, genome, found, &fold.shape, fold.scaffold.c_str(), (uint32_t)fold.scaffold.size(), &fold.limits, &kept) != VSC_OK)
                    throw std::runtime_error(vsc_last_error(ctx));
                vsc_pattern_guides_free(found);
                found = kept;
            }
            if (motif.limited) {  // --motif-forbid / --motif-forbid-context / --motif-require-cut: the same, after the fold FILTER
                vsc_pattern_guides *kept = nullptr;
                if (vsc_pattern_guides_filter_motifs(ctx, genome, found, &motif.shape, motif.left.c_str(), (uint32_t)motif.left.size(), motif.right.c_str(),
                                     (uint32_t)motif.right.size(), motif.motifs.data(), (uint32_t)motif.motifs.size(), &motif.limits, &kept) != VSC_OK)
                    throw std::runtime_error(vsc_last_error(ctx));
                vsc_pattern_guides_free(found);
                found = kept;
            }
            if (knockout.on) read_cds(knockout.cds_path, ix.names, ix.contigs, &knockout_coding);
            if (knockout.filtered) {  // --knockout-filter: the same, after the motif FILTER
                vsc_pattern_guides *kept = nullptr;
                if (vsc_pattern_guides_filter_knockout(ctx, genome, found, &knockout.shape, knockout_coding.cds, nullptr, &knockout.limits, &kept) != VSC_OK)
                    throw std::runtime_error(vsc_last_error(ctx));
                vsc_pattern_guides_free(found);
                found = kept;
            }
            if (efficient) {
                eff_linear.resize(vsc_pattern_guides_count(found));
                if (eff_any_score(ctx, genome, found, eff_model, eff_linear.data()) != VSC_OK) throw std::runtime_error(vsc_last_error(ctx));
            }
            mh_pairs.resize(mh.on ? 2 * vsc_pattern_guides_count(found) : 0);
            if (mh.on && vsc_pattern_guides_microhomology(ctx, genome, found, &mh.shape, mh_pairs.data(), nullptr) != VSC_OK)
                throw std::runtime_error(vsc_last_error(ctx));
            std::vector<uint32_t> edit_rows;  // -x: the (mask, hits) rows, and with -o the pairs
            std::vector<vsc_edit_pair> edit_pairs;
            if (edit.on)
                edit_rows_and_pairs(edit, vsc_pattern_guides_count(found), [&](uint32_t *r, vsc_edit_pair *pp, uint64_t cap, uint64_t *np) {
                    if (vsc_pattern_guides_edit(ctx, genome, found, &edit.shape, edit_targets.empty() ? nullptr : edit_targets.data(),
                                                edit_targets.size(), r, pp, cap, np, nullptr, nullptr) != VSC_OK)
                        throw std::runtime_error(vsc_last_error(ctx));
                }, &edit_rows, &edit_pairs);
            std::vector<uint32_t> fx_rows;  // --cds: the effect rows, and with --effects the records
            std::vector<vsc_effect> fx_records;
            if (fx.on)
                effects_rows_and_records(fx, vsc_pattern_guides_count(found), [&](uint32_t *r, vsc_effect *e, uint64_t cap, uint64_t *ne) {
                    if (vsc_pattern_guides_effects(ctx, genome, found, &edit.shape, fx.to, coding.cds, nullptr, r, e, cap, ne, nullptr, nullptr) != VSC_OK)
                        throw std::runtime_error(vsc_last_error(ctx));
                }, &fx_rows, &fx_records);
            std::vector<uint32_t> prime_rows;  // --prime: the (pbs, n_pairs) rows, and with --prime-out the pairs
            std::vector<vsc_prime_pair> prime_pairs;
            if (prime.on)
                prime_rows_and_pairs(prime, vsc_pattern_guides_count(found), [&](uint32_t *r, vsc_prime_pair *pp, uint64_t cap, uint64_t *np) {
                    if (vsc_pattern_guides_prime(ctx, genome, found, &prime.shape, prime_edits.empty() ? nullptr : prime_edits.data(),
                                                 prime_edits.size(), r, pp, cap, np, nullptr, nullptr) != VSC_OK)
                        throw std::runtime_error(vsc_last_error(ctx));
                }, &prime_rows, &prime_pairs);
            std::vector<uint32_t> variation_rows;  // --variation-out: the rows and the pairs
            std::vector<vsc_variation_pair> variation_pairs;
            if (variation.with_out)
                variation_rows_and_pairs(vsc_pattern_guides_count(found), [&](uint32_t *r, vsc_variation_pair *pp, uint64_t cap, uint64_t *np) {
                    if (vsc_pattern_guides_variation(ctx, genome, found, &variation.shape, variants.empty() ? nullptr : variants.data(),
                                                     variants.size(), r, pp, cap, np, nullptr, nullptr) != VSC_OK)
                        throw std::runtime_error(vsc_last_error(ctx));
                }, &variation_rows, &variation_pairs);
            std::vector<uint32_t> hdr_rows;  // --hdr: the (n_pairs, n_usable) rows, and with --hdr-out the pairs
            std::vector<vsc_hdr_pair> hdr_pairs;
            if (hdr.on)
                hdr_rows_and_pairs(hdr, vsc_pattern_guides_count(found), [&](uint32_t *r, vsc_hdr_pair *pp, uint64_t cap, uint64_t *np) {
                    if (vsc_pattern_guides_hdr(ctx, genome, found, &hdr.shape, hdr_edits.empty() ? nullptr : hdr_edits.data(), hdr_edits.size(), hdr_coding.cds, nullptr,
                            r, pp, cap, np, nullptr, nullptr) != VSC_OK)
                        throw std::runtime_error(vsc_last_error(ctx));
                }, &hdr_rows, &hdr_pairs);
            std::vector<uint32_t> fold_rows(fold.on ? 2 * vsc_pattern_guides_count(found) : 0);  // --fold: the rows
            if (fold.on && vsc_pattern_guides_fold(ctx, genome, found, &fold.shape, fold.scaffold.c_str(), (uint32_t)fold.scaffold.size(), fold_rows.data(), nullptr) != VSC_OK)
                throw std::runtime_error(vsc_last_error(ctx));
            std::vector<uint64_t> motif_rows(motif.on ? 3 * vsc_pattern_guides_count(found) : 0);  // --motifs: the rows
            if (motif.on && vsc_pattern_guides_motifs(ctx, genome, found, &motif.shape, motif.left.c_str(), (uint32_t)motif.left.size(),
                                                      motif.right.c_str(), (uint32_t)motif.right.size(), motif.motifs.data(),
                                                      (uint32_t)motif.motifs.size(), motif_rows.data(), nullptr, nullptr) != VSC_OK)
                throw std::runtime_error(vsc_last_error(ctx));
            std::vector<uint32_t> knockout_rows(knockout.on ? 4 * vsc_pattern_guides_count(found) : 0);  // --knockout: the rows
            if (knockout.on && vsc_pattern_guides_knockout(ctx, genome, found, &knockout.shape, knockout_coding.cds, nullptr, knockout_rows.data(),
                                                           nullptr, nullptr) != VSC_OK)
                throw std::runtime_error(vsc_last_error(ctx));
            const uint64_t n = vsc_pattern_guides_count(found);
            const uint64_t *codes = nullptr;
            st = vsc_pattern_guides_data(found, &codes, &loci);
            if (st != VSC_OK) throw std::runtime_error(vsc_last_error(ctx));
            std::printf("Guides found (total: %llu).\n", (unsigned long long)n);
            std::ofstream out(opts[7].value);
            if (!out.is_open()) throw std::runtime_error("Could not open output path.");
            out << "#guide\tchrom\tpos\tstrand" << (efficient ? "\tefficiencyLinear\tefficiency" : "") << (mh.on ? "\tmhScore\toofScore" : "")
                << (pick.on ? "\tpickTarget\tpickRank" : "") << (edit.on ? "\teditWindow\teditable\ttargetsHit" : "")
                << (fx.on ? "\tcodingEdits\tstopGained\tmissense\tsynonymous" : "") << (prime.on ? "\tpbsLen\tpbsGC\tprimePairs" : "")
                << (hdr.on ? "\thdrPairs\thdrUsable" : "") << (fold.on ? "\tfoldStarts\tfoldSelf\tfoldScaffold\tfoldSeed" : "")
                << (motif.on ? "\tmotifsConstruct\tmotifsCut\tmotifsElsewhere\tmotifsCutOnly" : "") << (knockout.on ? knockout_header() : "") << '\n';
            guides.resize(n);
            letters.resize(n * len);
            for (uint64_t i = 0; i < n; ++i) {
                if (vsc_pattern_guide_text(codes[i], len, ep.ps_start, ep.ps_len, 0, &letters[i * len]) != VSC_OK)
                    throw std::runtime_error("a code of the enumeration is no guide");
                guides[i].seq = letters.substr(i * len, len);
                if (tabled) {
                    char own[VSC_PATTERN_MAX_LEN];
                    uint32_t f = 0;
                    if (vsc_pattern_guide_text(codes[i], len, ep.ps_start, ep.ps_len, 1, own) != VSC_OK ||
                        vsc_pattern_table_score(table, guides[i].seq.c_str(), own, nullptr, &f) != VSC_OK)
                        throw std::runtime_error("a code of the enumeration is no site");
                    own_fixed.push_back(f);
                }
                guides[i].id = first_word(ix.names[loci[i].contig]) + ':' + std::to_string(loci[i].pos) + ':' + (loci[i].strand ? '-' : '+');
                std::string line = guides[i].seq + '\t' + first_word(ix.names[loci[i].contig]) + '\t' + std::to_string(loci[i].pos) + '\t' + (loci[i].strand ? '-' : '+');
                if (efficient) line += '\t' + eff_text(eff_linear[i]) + '\t' + eff_text(eff_any_link(eff_model, eff_linear[i]));
                if (mh.on) line += mh_columns(&mh_pairs[2 * i]);
                std::string ecol;
                if (edit.on) {
                    char own[VSC_PATTERN_MAX_LEN];
                    if (vsc_pattern_guide_text(codes[i], len, ep.ps_start, ep.ps_len, 1, own) != VSC_OK) throw std::runtime_error("a code of the enumeration is no site");
                    ecol = edit_columns(edit.shape, std::string(own, len), &edit_rows[2 * i]);
                }
                if (fx.on) ecol += effects_columns(&fx_rows[2 * i]);
                if (prime.on) ecol += prime_columns(&prime_rows[2 * i]);
                if (hdr.on) ecol += hdr_columns(&hdr_rows[2 * i]);
                if (fold.on) ecol += fold_columns(&fold_rows[2 * i]);
                if (motif.on) ecol += motif_columns(motif, &motif_rows[3 * i]);
                if (knockout.on) ecol += knockout_columns(&knockout_rows[4 * i], knockout_coding.transcripts);
                if (pick.on) pick_lines.push_back(line), edit_cols.push_back(ecol);
                else out << line << ecol << '\n';
            }
            if (edit.with_pairs) {
                std::vector<std::string> ids;
                for (const auto &g : guides) ids.push_back(g.id);
                write_edit_pairs(edit.pairs_path, edit_pairs, edit_targets, ix.names, ids);
            }
            if (fx.with_listing) {
                std::vector<std::string> ids;
                for (const auto &g : guides) ids.push_back(g.id);
                write_effects(fx.effects_path, fx_records, coding.transcripts, ids);
            }
            if (prime.with_pairs) {
                std::vector<std::string> ids;
                for (const auto &g : guides) ids.push_back(g.id);
                write_prime_pairs(prime.pairs_path, prime.shape, prime_pairs, prime_edits, std::vector<vsc_locus>(loci, loci + n), ix, ids);
            }
            if (variation.with_out) {
                std::vector<std::string> ids;
                for (const auto &g : guides) ids.push_back(g.id);
                write_variation(variation.out_path, variation_rows, variation_pairs, variants, ix.names, ids);
            }
            if (hdr.with_pairs) {
                std::vector<std::string> ids;
                for (const auto &g : guides) ids.push_back(g.id);
                write_hdr_pairs(hdr.pairs_path, hdr.shape, hdr_pairs, hdr_edits, std::vector<vsc_locus>(loci, loci + n), ix.names, ids);
            }
            if (motif.on && !motif.out_path.empty()) {
                std::vector<std::string> ids;
                for (const auto &g : guides) ids.push_back(g.id);
                write_motifs(motif, motif_rows, ids);
            }
            if (knockout.on && !knockout.out_path.empty()) {
                std::vector<std::string> ids;
                for (const auto &g : guides) ids.push_back(g.id);
                write_knockout(knockout.out_path, knockout_rows, knockout_coding.transcripts, ids);
            }
            if (!out) throw std::runtime_error("Write error on " + opts[7].value);
        }

        std::vector<vsc_pattern_summary> rows(guides.size());
        std::vector<vsc_guide_table_row> table_rows(tabled ? guides.size() : 0);
        if (!enumerate || opts[3].set) {
            if (guides.size() > 0xFFFFFFFFull) throw std::runtime_error("more guides than one search takes");
            vsc_pattern_params p{};
            p.max_mismatches = (uint32_t)mm;
            if (tabled)
                st = vsc_search_pattern_table(ctx, genome, pattern.c_str(), letters.c_str(), (uint32_t)guides.size(), len, &p, table, &sel,
                                              opts[6].set ? &hits : nullptr, rows.data(), table_rows.data());
            else
                st = vsc_search_pattern(ctx, genome, pattern.c_str(), letters.c_str(), (uint32_t)guides.size(), len, &p, opts[6].set ? &hits : nullptr,
                                        rows.data());
            if (st != VSC_OK) throw std::runtime_error(vsc_last_error(ctx));
            // a found guide's own locus is a hit at 0 mismatches (N at the positions outside the protospacer): not an off-target
            if (enumerate)
                for (auto &r : rows) r.count[0] -= r.count[0] ? 1u : 0u;
            if (enumerate && tabled)
                for (size_t g = 0; g < table_rows.size(); ++g) {
                    table_rows[g].score_sum -= own_fixed[g];
                    if (own_fixed[g]) table_rows[g].positive -= 1, table_rows[g].positive_nm[0] -= 1;
                }
        }
        if (pick.on) {  // -k: the picks of every -B target where the candidates lie; the -E listing's lines follow its header
            vsc_regions *pick_regions = nullptr;
            if (vsc_regions_build(ix.contigs.data(), (uint32_t)ix.contigs.size(), targets.data(), targets.size(), ep.rule, &pick_regions) != VSC_OK)
                throw std::runtime_error("could not build the regions of the -B file");
            int prc = VSC_OK;
            std::vector<uint32_t> picks, counts;
            try {
                PickColumns cols;
                cols.table_rows = table_rows.data();
                cols.eff = eff_linear.data();
                cols.pairs = mh_pairs.data();
                const std::vector<uint64_t> keys = pick_keys(pick, guides.size(), cols);
                const uint32_t n_targets = (uint32_t)target_names.size();
                const vsc_pick_params pp{len, mh.on ? mh.shape.cut : pick_cut, pick.k, pick.spacing, 0, 0};
                picks.resize((size_t)n_targets * pick.k);
                counts.resize(n_targets);
                prc = vsc_pattern_guides_pick(ctx, genome, found, pick_regions, pick.by_name ? pick_group.data() : nullptr, nullptr, n_targets, keys.data(), &pp,
                                              picks.data(), counts.data(), nullptr, nullptr, nullptr);
            } catch (...) {
                vsc_regions_free(pick_regions);
                throw;
            }
            vsc_regions_free(pick_regions);
            if (prc != VSC_OK) throw std::runtime_error(vsc_last_error(ctx));
            const std::vector<std::string> marks = pick_text(pick, guides.size(), target_names, picks, counts);
            std::ofstream out(opts[7].value, std::ios::app);
            if (!out.is_open()) throw std::runtime_error("Could not open output path.");
            for (size_t i = 0; i < pick_lines.size(); ++i) out << pick_lines[i] << marks[i] << edit_cols[i] << '\n';
            out.close();
            if (!out) throw std::runtime_error("Write error on " + opts[7].value);
        }
        // -v: the same search in the individual's genome - windows of the pattern's length from the packed planes, on the same
        // context; with -E the enumerated loci are the excluded on-targets, with -R nothing is excluded
        std::vector<vsc_pattern_variant_row> ind_ref(individual ? guides.size() : 0), ind_win(ind_ref.size()), ind_var(ind_ref.size());
        std::vector<vsc_guide_table_row> ind_ref_table(individual && tabled ? guides.size() : 0), ind_win_table(ind_ref_table.size()),
            ind_var_table(ind_ref_table.size());
        if (individual) {
            std::vector<const char *> names;
            for (const std::string &n : ix.names) names.push_back(n.c_str());
            char why[512] = "";
            if (vsc_windows_build(opts[23].value.c_str(), vcf_sample, len, 0, ix.hi.data(), ix.lo.data(), ix.nm.data(), ix.contigs.data(), names.data(),
                                  (uint32_t)ix.contigs.size(), &windows, why, sizeof why) != VSC_OK)
                throw std::runtime_error(std::string("-v: ") + (why[0] ? why : "could not build the variant windows"));
            const uint32_t n_win = vsc_windows_count(windows);
            std::fprintf(stderr, "Variant windows built (total: %u).\n", n_win);
            if (vsc_variant_map_build(n_win ? vsc_windows_name(windows, 0, nullptr) : nullptr, n_win ? vsc_windows_name_offsets(windows) : nullptr,
                                      n_win ? vsc_windows_contigs(windows) : nullptr, n_win, ix.contigs.data(), names.data(),
                                      (uint32_t)ix.contigs.size(), &vmap) != VSC_OK)
                throw std::runtime_error("-v: could not parse the ids of the variant windows");
            if (n_win) {
                st = vsc_genome_load(ctx, vsc_windows_plane(windows, 0), vsc_windows_plane(windows, 1), vsc_windows_plane(windows, 2), 0,
                                     vsc_windows_words(windows), vsc_windows_words(windows), vsc_windows_contigs(windows), n_win, &win_genome);
                if (st != VSC_OK) throw std::runtime_error(vsc_last_error(ctx));
            }
            vsc_pattern_params p{};
            p.max_mismatches = (uint32_t)mm;
            st = vsc_search_pattern_variants(ctx, genome, win_genome, vmap, pattern.c_str(), letters.c_str(), (uint32_t)guides.size(), len, &p, table,
                                             enumerate ? loci : nullptr, 0, ind_ref.data(), ind_win.data(), ind_var.data(),
                                             tabled ? ind_ref_table.data() : nullptr, tabled ? ind_win_table.data() : nullptr,
                                             tabled ? ind_var_table.data() : nullptr);
            if (st != VSC_OK) throw std::runtime_error(vsc_last_error(ctx));
        }
        // the bulged sites of the same guides (the bulged neighbours of a found guide's own locus are among them)
        std::vector<vsc_bulge_summary> bulge_rows(bulged ? guides.size() : 0);
        const bool bulge_on[VSC_BULGE_CLASSES] = {bp.rna_max >= 2, bp.rna_max >= 1, bp.dna_max >= 1, bp.dna_max >= 2};
        static const char *const kBulgeClass[VSC_BULGE_CLASSES] = {"br2", "br1", "bd1", "bd2"};
        if (bulged) {
            bp.max_mismatches = (uint32_t)mm;
            st = vsc_search_pattern_bulges(ctx, genome, pattern.c_str(), letters.c_str(), (uint32_t)guides.size(), len, &bp,
                                           opts[15].set || sited ? &bulge_hits : nullptr, bulge_rows.data());
            if (st != VSC_OK) throw std::runtime_error(vsc_last_error(ctx));
        }
        std::vector<vsc_site_summary> site_rows(sited ? guides.size() : 0);
        if (sited) {  // all plain records kept on the device beside the bulged ones, collapsed where they lie
            vsc_pattern_params p{};
            p.max_mismatches = (uint32_t)mm;
            st = vsc_search_pattern(ctx, genome, pattern.c_str(), letters.c_str(), (uint32_t)guides.size(), len, &p, &site_plain, nullptr);
            if (st == VSC_OK) st = vsc_pattern_hits_sites(ctx, site_plain, bulge_hits, (uint32_t)guides.size(), &sp, &sites, site_rows.data());
            if (st != VSC_OK) throw std::runtime_error(vsc_last_error(ctx));
        }
        std::vector<vsc_guide_table_row> site_table_rows(site_scored ? guides.size() : 0);
        if (site_scored) {  // the sites scored where the collapse left them; -K / -S cut the listing, the rows are over all sites
            st = vsc_sites_table(ctx, genome, sites, &sp, letters.c_str(), (uint32_t)guides.size(), len, bulge_table, &sel, &scored_sites,
                                 site_table_rows.data());
            if (st != VSC_OK) throw std::runtime_error(vsc_last_error(ctx));
        }

        if (opts[5].set) {
            std::ofstream out(opts[5].value);
            if (!out.is_open()) throw std::runtime_error("Could not open output path.");
            out << "#guideId\tguideSeq\tofftargetCount";
            for (long k = 0; k <= mm; ++k) out << "\tmm" << k;
            if (bulged) {
                out << "\tbulgeCount";
                for (int c = 0; c < VSC_BULGE_CLASSES; ++c)
                    for (long k = 0; bulge_on[c] && k <= mm; ++k) out << '\t' << kBulgeClass[c] << "mm" << k;
            }
            if (tabled) out << "\ttableScoreSum\ttableSpecScore\ttablePositive";
            if (sited) out << "\tsiteCount\tsiteBulgeOnly";
            if (site_scored) out << "\tsiteScoreSum\tsiteSpecScore\tsitePositive";
            if (individual) {
                out << "\tindCount";
                for (long k = 0; k <= mm; ++k) out << "\timm" << k;
                out << "\tvarCount";
                for (long k = 0; k <= mm; ++k) out << "\tvmm" << k;
                out << "\tvarDuplicates\trefShadowed";
                if (tabled) out << "\tindScoreSum\tindSpec\tvarScoreSum";
            }
            out << '\n';
            for (size_t g = 0; g < guides.size(); ++g) {
                uint64_t total = 0;
                for (long k = 0; k <= mm; ++k) total += rows[g].count[k];
                out << first_word(guides[g].id) << '\t' << guides[g].seq << '\t' << total;
                for (long k = 0; k <= mm; ++k) out << '\t' << rows[g].count[k];
                if (bulged) {
                    uint64_t bulge_total = 0;
                    for (int c = 0; c < VSC_BULGE_CLASSES; ++c)
                        for (long k = 0; bulge_on[c] && k <= mm; ++k) bulge_total += bulge_rows[g].count[c][k];
                    out << '\t' << bulge_total;
                    for (int c = 0; c < VSC_BULGE_CLASSES; ++c)
                        for (long k = 0; bulge_on[c] && k <= mm; ++k) out << '\t' << bulge_rows[g].count[c][k];
                }
                if (tabled) {
                    char buf[64];
                    std::snprintf(buf, sizeof buf, "\t%.6f", (double)table_rows[g].score_sum * 0x1p-30);
                    out << buf;
                    std::snprintf(buf, sizeof buf, "\t%.0f", std::floor(vsc_table_specificity(table_rows[g].score_sum) + 0.5));
                    out << buf << '\t' << table_rows[g].positive;
                }
                if (sited) out << '\t' << site_rows[g].sites << '\t' << site_rows[g].bulge_only;
                if (site_scored) {
                    char buf[64];
                    std::snprintf(buf, sizeof buf, "\t%.6f", (double)site_table_rows[g].score_sum * 0x1p-30);
                    out << buf;
                    std::snprintf(buf, sizeof buf, "\t%.0f", std::floor(vsc_table_specificity(site_table_rows[g].score_sum) + 0.5));
                    out << buf << '\t' << site_table_rows[g].positive;
                }
                if (individual) {
                    uint64_t ind_total = 0, var_total = 0;
                    for (long k = 0; k <= mm; ++k) ind_total += (uint64_t)ind_ref[g].count[k] + ind_win[g].count[k], var_total += ind_var[g].count[k];
                    out << '\t' << ind_total;
                    for (long k = 0; k <= mm; ++k) out << '\t' << (uint64_t)ind_ref[g].count[k] + ind_win[g].count[k];
                    out << '\t' << var_total;
                    for (long k = 0; k <= mm; ++k) out << '\t' << ind_var[g].count[k];
                    out << '\t' << ind_win[g].dropped << '\t' << ind_ref[g].dropped;
                    if (tabled) {
                        const uint64_t ind_sum = ind_ref_table[g].score_sum + ind_win_table[g].score_sum;
                        char buf[64];
                        std::snprintf(buf, sizeof buf, "\t%.6f", (double)ind_sum * 0x1p-30);
                        out << buf;
                        std::snprintf(buf, sizeof buf, "\t%.0f", std::floor(vsc_table_specificity(ind_sum) + 0.5));
                        out << buf;
                        std::snprintf(buf, sizeof buf, "\t%.6f", (double)ind_var_table[g].score_sum * 0x1p-30);
                        out << buf;
                    }
                }
                out << '\n';
            }
            if (!out) throw std::runtime_error("Write error on " + opts[5].value);
        }
        if (opts[6].set) {
            const uint64_t n = vsc_pattern_hits_count(hits);
            const vsc_pattern_hit *h = nullptr;
            st = vsc_pattern_hits_data(hits, &h);
            if (st != VSC_OK) throw std::runtime_error(vsc_last_error(ctx));
            const uint32_t *fixed = nullptr;
            if (tabled && vsc_pattern_hits_scores(hits, &fixed) != VSC_OK) throw std::runtime_error(vsc_last_error(ctx));
            std::ofstream out(opts[6].value);
            if (!out.is_open()) throw std::runtime_error("Could not open output path.");
            out << "#guideId\tchrom\tstart\tend\tstrand\tmismatches\tmismatchPositions\tsequence" << (tabled ? "\ttableScore\n" : "\n");
            std::string window(len, 'N'), text;
            for (uint64_t i = 0; i < n; ++i) {
                const vsc_pattern_hit &r = h[i];
                vsc_unpack_bases(ix.hi.data(), ix.lo.data(), ix.nm.data(), ix.contigs[r.contig].offset + r.pos, len, &window[0]);
                std::string where;  // 0-based window positions on the forward genome, ascending; - if none
                for (uint32_t b = 0; b < len; ++b)
                    if ((r.mask >> b) & 1u) where += (where.empty() ? "" : ",") + std::to_string(b);
                text += first_word(guides[r.guide].id) + '\t' + first_word(ix.names[r.contig]) + '\t' + std::to_string(r.pos) + '\t' + std::to_string(r.pos + len) + '\t' +
                        (VSC_PATTERN_STRAND(r.info) ? '-' : '+') + '\t' + std::to_string(VSC_PATTERN_NM(r.info)) + '\t' + (where.empty() ? "-" : where) +
                        '\t' + window;
                if (tabled) {
                    char buf[32];
                    std::snprintf(buf, sizeof buf, "\t%.9f", (double)fixed[i] * 0x1p-30);
                    text += buf;
                }
                text += '\n';
                if (text.size() > (1u << 22)) {
                    out << text;
                    text.clear();
                }
            }
            out << text;
            if (!out) throw std::runtime_error("Write error on " + opts[6].value);
        }
        if (sited) {
            const vsc_site *rec = nullptr;
            const vsc_site_score *scores = nullptr;
            vsc_sites *listed = site_scored ? scored_sites : sites;
            if (vsc_sites_data(listed, &rec) != VSC_OK || (site_scored && vsc_sites_scores(listed, &scores) != VSC_OK))
                throw std::runtime_error(vsc_last_error(ctx));
            std::vector<std::string> ids;
            for (const auto &g : guides) ids.push_back(first_word(g.id));
            write_sites(opts[21].value, "-Z", rec, vsc_sites_count(listed), len, ids, ix, scores);
        }
        if (bulge_hits && opts[15].set) {
            const vsc_bulge_hit *rec = nullptr;
            if (vsc_bulge_hits_data(bulge_hits, &rec) != VSC_OK) throw std::runtime_error(vsc_last_error(ctx));
            const uint64_t n = vsc_bulge_hits_count(bulge_hits);
            std::ofstream out(opts[15].value);
            if (!out.is_open()) throw std::runtime_error("Could not open the -U path.");
            out << "#guideId\tchrom\tstart\tend\tstrand\tkind\tsize\tindex\tmismatches\tsequence\n";
            std::string site, text;
            for (uint64_t j = 0; j < n; ++j) {
                const vsc_bulge_hit &h = rec[j];
                const uint32_t site_len = (uint32_t)((int)len + VSC_BULGE_D(h.info));
                site.assign(site_len, 'N');
                vsc_unpack_bases(ix.hi.data(), ix.lo.data(), ix.nm.data(), ix.contigs[h.contig].offset + h.pos, site_len, &site[0]);
                text += first_word(guides[h.guide].id) + '\t' + first_word(ix.names[h.contig]) + '\t' + std::to_string(h.pos) + '\t' +
                        std::to_string(h.pos + site_len) + '\t' + (VSC_BULGE_STRAND(h.info) ? '-' : '+') + '\t' +
                        (VSC_BULGE_KIND(h.info) == VSC_BULGE_RNA ? "RNA" : "DNA") + '\t' + std::to_string(VSC_BULGE_SIZE(h.info)) + '\t' +
                        std::to_string(VSC_BULGE_INDEX(h.info)) + '\t' + std::to_string(VSC_BULGE_NM(h.info)) + '\t' + site + '\n';
                if (text.size() > (1u << 22)) {
                    out << text;
                    text.clear();
                }
            }
            out << text;
            out.close();
            if (!out) throw std::runtime_error("Could not write the -U file.");
        }
        rc = 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "ERROR: %s\n", e.what());
        rc = 1;
    }
    vsc_pattern_hits_free(hits);
    vsc_pattern_guides_free(found);
    eff_any_free(eff_model);
    vsc_pattern_table_free(table);
    vsc_bulge_table_free(bulge_table);
    vsc_sites_free(scored_sites);
    vsc_bulge_hits_free(bulge_hits);
    vsc_sites_free(sites);
    vsc_pattern_hits_free(site_plain);
    vsc_genome_free(win_genome);
    vsc_variant_map_free(vmap);
    vsc_windows_free(windows);
    vsc_genome_free(genome);
    vsc_ctx_destroy(ctx);
    return rc;
}
