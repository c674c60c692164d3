// guide_summary - per-guide off-target summary of a guide library (vsc_search_summary): for every guide the number of
// off-targets at each mismatch count and CRISPOR's MIT specificity score, without writing a single hit record.
// Flags, validation, exit codes and genome loading follow bidir_mapping (read_mapping/bidir_mapping.cpp:190-280).
// Guides come from exactly one of
//   -R reads.fa       23-mers (non-ACGT letters become A); nothing is excluded
//   -B ontargets.bed  BED6 on-targets, the 23-mer extracted as fasta_writer does (extract_fasta_ontargets.h:92-139); the
//                     on-target locus itself (chr, start, strand) is left out of the counts and reported as onTargetFound
//   -E targets.bed    BED3+ intervals of a target: the guides are the candidates the device finds in them (vsc_guides_enumerate:
//                     N-free 23-mers with the guide PAM -p, default GG, on the strands -s; inside the intervals by the rule -e,
//                     default inside; GC bounds -g MIN,MAX and largest T run -t over the 20 protospacer bases), in enumeration
//                     order (chrom, start, '+' before '-'), guideId = chrom:start:strand; the candidate's own locus is left out
//                     as -B's is.  -L guides.bed writes them as BED6 (chrom start start+23 guideId 0 strand), the on-target
//                     format the VARSCOT driver and -B read.  A guide PAM other than GG / GA is searched as -P unless -P is given.
// Output (-O, default stdout): one line per guide in input order under the header
//   #guideId guideSeq mitSpecScore offtargetCount onTargetFound mm0 .. mm<M> mitHitSum
// mitSpecScore = floor(100 / (100 + mitHitSum) * 100 + 0.5) (CRISPOR's guide score and Python 2 round()),
// mitHitSum = the sum of the counted hits' MIT scores (fixed point, 2^-24 units, printed with %.6f).
// With -T hits.tsv the same search also lists every guide's off-targets that matter (vsc_search_select): the -K best by MIT
// score and / or those with an MIT score >= -S, per guide in rank order (score descending, '+' before '-', position) under
//   #guideId rank chrom start end strand mismatches mismatchPositions mitScore sequence
// chrom = first word of the contig name, start / end 0-based half-open on the forward genome, mismatchPositions = 0-based
// window positions on the forward genome (ascending, comma-separated, - if none), sequence = the window's forward-genome
// bases.  The summary TSV is the same with and without these options.
// With -A regions.bed (BED3+: chrom start end ..., chrom = first word of a contig name; an unknown chrom is an error) every
// guide's hits are also summarised over those IN THE REGIONS (vsc_search_summary_regions) - a hit is in when its window shares a
// base with an interval (-a overlap, the default) or lies fully inside one (-a inside) - and every line gains the columns
//   regionMitSpecScore regionCount rmm0 .. rmm<M> regionMitHitSum
// -X keep|drop (needs -A and -T) lists in the -T file only hits in the regions / only hits outside them: -K and -S then apply
// to that side.  With -A and -T but no -X the genome is searched twice: the unfiltered listing (vsc_search_select_regions
// takes region rows only beside a filter) and then the region rows (vsc_search_summary_regions); with -X one search gives
// both.  Without -A the output is what it was.
// -N name|coords names the interval a listed hit or a found guide lies in (vsc_hits_locate / vsc_guides_locate: of the intervals
// it is in, the one with the largest start, then the smallest end, then the first in the file - the exon before its gene):
// with -A and -T the -T file gains a last column `region`, with -E and -L every -L line a 7th column.  name prints the 4th
// column of that BED line, or chrom:start-end as the line has them if it has only three; coords always the latter; - if the
// hit is in no interval.  Without -N every output is what it was.
// -F model.vscrf with -C activity.txt (the on-target activity table the mergers read: guideId, sequence, activity per line; every
// guide needs a line) adds what the CLASSIFIER says of every guide's off-targets (vsc_search_summary_classified) - the columns
//   rfExpectedActive rfActive rfTies ra0 .. ra<M>
// = the sum of the forest's probabilities (votes / trees) over the counted hits, the hits it calls active (more than half of the
// trees), those with exactly half, and the active ones by mismatch count - behind all other columns, from the same search unless
// -A or a listing by MIT score need one of their own.  With -T, -r votes ranks the listing by the forest's votes instead of the
// MIT score (vsc_search_select_classified; -r mit is the default): -K still applies, -V MIN lists only off-targets with at least
// MIN votes (-S belongs to -r mit), the ranks follow (votes descending, '+' before '-', position) and the listing gains a last
// column rfVotes.  -r votes runs on one device and without -A.  Without -F every output is what it was.
// -v sample.vcf [-n SAMPLE] screens the guides in ONE INDIVIDUAL'S genome: SAMPLE is the 0-based sample column of the VCF
// (default 0, as vcf_loader counts them).  The alt-allele windows are built from the packed planes (vsc_windows_build), the
// reference is searched with the windows' shadow as regions (vsc_search_summary_regions under vsc_variant_map_shadow: a
// reference hit that lies inside a window is the window search's to report), the window genome is loaded on the same device and
// screened (vsc_search_summary_variants: hits in chromosome coordinates, the mergers' duplicates and the on-target dropped), and
// every line gains, behind all other columns,
//   indMitSpecScore indCount imm0 .. imm<M> indMitHitSum varCount vmm0 .. vmm<M> varMitHitSum varDuplicates
// ind* = the guide in the individual's genome (unshadowed reference hits + counted window hits: the rows bam_merger prints, per
// guide), var* = the counted window hits that cover a variant, varDuplicates = window hits dropped as duplicates.  A sample
// without variants gives the reference's numbers and zeros.  -v runs on one device and not with -A, -X, -T or -F.  Without -v
// every output is what it was.
// -J pairs.tsv with -j MIN,MAX screens GUIDE PAIRS for a paired-nickase design (Cas9 D10A, FokI-dCas9): the pairs are every
// guide on '-' with every guide on '+' of the same sequence whose offset - the gap between the two protospacers' PAM-distal
// ends, negative when they overlap; PAM-out pairs only need MIN > -23 - lies in MIN .. MAX (with -E found on the device among
// the candidates, vsc_guides_pairs; with -B among the on-targets, vsc_loci_pairs; -R has no loci: a usage error).  One more
// search keeps the guides' records on the device and joins them there (vsc_hits_pairs): a pair's off-target is a locus where a
// hit of one guide and a hit of the other lie on opposite strands within the same offset range - the pair's own locus left out
// and reported as onTarget.  One line per pair, in ascending (guideA, guideB) input order, under
//   #pairId guideA guideB offset sites onTarget minNmSum ps0 .. ps<2M>
// pairId = guideA|guideB, guideA the '-' guide, sites = the paired off-target sites, minNmSum = the smallest sum of the two
// hits' mismatches among them (- if none), ps<k> = sites with that sum.  -J does not combine with -v.  Without -J every other
// output is what it was; the -T listing gains nothing.
// -u DNA,RNA (e.g. -u 1,1; each 0 .. 2, not both 0) adds the BULGED sites (vsc_search_bulges): the sites one or two bases longer
// (DNA bulge) or shorter (RNA bulge) than 23 that pair with the guide within -M when the extra bases of the site or of the guide
// stay unpaired.  Every line gains, behind all other columns, bulgeCount and per enabled class in ascending site length -
// br2 br1 bd1 bd2 = RNA bulge of 2, of 1, DNA bulge of 1, of 2 - the columns <class>mm0 .. <class>mm<M>.  The bulged neighbours of
// a plain off-target (the same locus one base longer or shorter at its 5' end) are among them, as in Cas-OFFinder's output.
// -U bulges.tsv (needs -u) lists the sites, in ascending (guide, strand, chrom, start, site length) order, under
//   #guideId chrom start end strand kind size index mismatches sequence
// kind = DNA | RNA, index = the read position in front of which the bulge lies (the smallest that gives the fewest mismatches),
// sequence = the site's forward-genome bases.  -u runs on one device and does not combine with -v or -J.  Without -u every
// output is what it was.
// -Z sites.tsv (needs -u, as -U) collapses the plain and the bulged alignments into CUT SITES on the device (vsc_hits_sites): one
// record per (guide, strand, chrom, PAM-side end) with its best alignment - fewest mismatches + bulge bases, then the smaller
// bulge, then DNA before RNA.  Every line gains, behind all other columns, siteCount siteBulgeOnly (the sites; those without a
// plain member).  The listing, in ascending (guide, strand, chrom, start, site length) order of the best alignments, goes under
//   #guideId chrom start end strand kind size index mismatches members sequence
// kind = plain | DNA | RNA, members = the site's alignments as d:mismatches (e.g. -1:3,0:2,+1:3), sequence = the best
// alignment's forward-genome bases.  Without -Z every output is what it was.
// -w bulge.tsv (needs -W, -u and -Z) scores the cut sites on the device (vsc_sites_table): -W stays the base table, the -w file
// holds the bulge weights, `dna j s w` (one unpaired site base s when the bulge lies in front of read position j) and
// `rna j g w` (the unpaired guide base g at read position j), every j in 0 .. 19 and every base once.  Every line gains, behind
// all other columns, siteScoreSum siteSpecScore sitePositive (over the sites' largest member scores); the -Z listing gains
// tableScore (that score, %.9f) and scoredAs (the d of the member that attains it) and is cut per guide by -K / -S on that
// score.  Without -w every output is what it was.
// -W table.tsv scores every off-target with a TABLE (vsc_search_summary_table; the CFD form: a product of weights by position,
// guide base and site base times a weight for the site's PAM letters).  The file holds one entry per line, `j g s w` (0-based
// read position, guide letter, site letter in read orientation, weight) or `PAM XY w`; '#' starts a comment; the diagonal is 1;
// every other entry must be there.  Every line gains, behind all other columns,
//   tableScoreSum tableSpecScore tablePositive
// = the sum of the counted hits' scores (fixed point, 2^-30 units, %.6f), floor(100 / (100 + sum) * 100 + 0.5) - for a CFD table
// CRISPOR's cfdSpecScore - and the hits that score above 0.  With -T the listing is selected and ranked by the table score
// (vsc_search_select_table): -K the best K, -S a floor on the table score, 0 .. 1, and a last column tableScore (%.9f); that
// runs on one device, without -A and -r votes.  -W does not combine with -v.  Without -W every output is what it was.
// -Y model.tsv (needs -E, one device) scores every found guide's ON-TARGET EFFICIENCY with a linear position-specific model
// (vsc_guides_efficiency; the form of Rule Set 1 and CRISPRscan: an intercept plus a weight per (position, base) and per
// (position, dinucleotide) over a context window around the site plus a G/C term; the file is what
// varscot_amd.EfficiencyModel.to_tsv writes, tools/README.md; its site_len must be 23).  The -L listing gains two last columns,
//   efficiencyLinear efficiency
// = the linear predictor (%.17g; NA when the context leaves its sequence or holds an N) and the predictor through the model's
// link.  -y MIN (needs -Y) keeps only the candidates whose predictor is defined and >= MIN, linear domain
// (vsc_guides_filter_efficiency), BEFORE the off-target search: every output holds the survivors only.  A -Y file that holds
// a `tree` line is an ensemble of regression trees instead (the form of Rule Set 2; varscot_amd.TreeEfficiencyModel.to_tsv,
// tools/eff_trees_host.hpp; vsc_guides_efficiency_trees, vsc_guides_filter_efficiency_trees): the same columns, the same -y.
// -H FLANK[,CUT] (needs -E, one device) scores every found guide's MICROHOMOLOGY around its cut site (vsc_guides_microhomology: the
// score of Bae et al. 2014 over FLANK bases on either side of the break in front of read position CUT, default 17): the -L
// listing gains the last columns mhScore oofScore (%.17g; NA when the window leaves its sequence or holds an N).  -m
// MIN_OOF[,MIN_MH] (needs -H) keeps only the candidates whose out-of-frame share is at least MIN_OOF per cent and whose score is
// at least MIN_MH (vsc_guides_filter_microhomology), BEFORE the off-target search, as -y does.
// -x CBE | ABE | START,LEN,BASE (needs -E, one device) looks at every found guide's BASE-EDITOR window (vsc_guides_edit): the -L
// listing gains the last columns editWindow (the window's read letters) editable targetsHit.  -z targets.bed (one base per line)
// and -l MIN,MAX (both need -x) keep only the candidates that reach a target base / hold MIN .. MAX editable bases
// (vsc_guides_filter_edit), BEFORE the off-target search; -o pairs.tsv (needs -z) lists the pairs.  Without -Y every
// output is what it was.
// --prime PE2 | SPEC (needs -E, one device) looks at the pegRNA a PRIME EDITOR needs on every found guide (vsc_guides_prime,
// DESIGN 4.30; tools/prime_host.hpp): the candidates without a context (or, without --prime-allow-weak, with a WEAK primer binding
// site) are dropped BEFORE the off-target search (vsc_guides_filter_prime), with --prime-edits edits.tsv those that can write none
// of the edits as well; the -L listing gains the last columns pbsLen pbsGC primePairs; --prime-out pairs.tsv (needs --prime-edits)
// lists the pairs with their extensions.  Without --prime every output is what it was.
// -k K[,SPACING] [-b COLS] [-c interval|name] (needs -E and -L, one device) picks the K best guides of every -E target, their cut
// sites at least SPACING bases apart (vsc_guides_pick; tools/pick_host.hpp makes the key from mit, table, eff, oof, mh
// in the order of -b): the -L listing, written after the search whose rows rank the guides, gains the last columns pickTarget
// pickRank (NA NA where a guide is not picked).  Without -k every output is byte for byte what it was.
// --hdr SpCas9 | Cas12a | SPEC (needs -E, one device; tools/hdr_host.hpp) asks whether a cut at every found guide can be repaired
// from a donor that carries a wanted edit: the candidates without a context are dropped BEFORE the off-target search,
// with --hdr-edits edits.tsv those without a usable pair as well (--hdr-allow-open: without any pair); --hdr-cds cds.bed keeps the
// blocking substitution synonymous; the -L listing gains the last columns hdrPairs hdrUsable; --hdr-out pairs.tsv (needs
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
// form with itself and with the --fold-scaffold text (at most 128 letters, or @FILE; default: none): the -L listing gains the last
// columns foldStarts foldSelf foldScaffold foldSeed; --max-fold STARTS[,SELF[,SCAF[,SEED]]] keeps the candidates within the limits.
#include <algorithm>
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
#include "forest_host.hpp"
#include "merge_host.hpp"

using namespace vsc_host;

int main(int argc, char **argv)
{
    std::vector<Option> opts = {
        {'G', "genome", "Path to genome fasta file", true},
        {'I', "index", "Path to the indexed genome", true},
        {'R', "reads", "Path to the guides as 23-mers (.fa/.fasta; everything else than ACGT is converted to A)", false},
        {'B', "bed", "Path to BED6 on-targets (.bed): the 23-mer is extracted from the genome, the locus is excluded", false},
        {'M', "mismatches", "Number of allowed mismatches", true},
        {'O', "output", "Path to output TSV file (default: standard output)", false},
        {'P', "pam", "Additional non-canonical PAM that should be allowed for off-target search besides (N)GG and (N)GA (default).", false},
        {'D', "device", "HIP device index (default 0), or a comma-separated list (0,1,2,...): the genome is sharded over these "
                        "devices, each summarises its own windows, the counts are added on the host", false},
        {'K', "top", "List the K best off-targets of every guide by MIT score in the -T file (default: no limit)", false},
        {'S', "min-score", "List only off-targets with an MIT score >= this value, 0 .. 100, in the -T file (default: no floor)", false},
        {'T', "hits", "Path to the TSV file of the listed off-targets (.tsv/.txt); required with -K / -S", false},
        {'A', "regions", "Path to an annotation (.bed, BED3+): adds the summary columns over the hits in these regions", false},
        {'a', "region-rule", "overlap (default): a hit is in the regions when its window shares a base with an interval; "
                             "inside: when it lies fully inside one interval", false},
        {'X', "region-scope", "keep | drop: list in the -T file only hits in the regions / outside them (needs -A and -T)", false},
        {'E', "targets", "Path to target intervals (.bed, BED3+): the guides are the candidate guides found in them, each with its own locus excluded", false},
        {'e', "target-rule", "inside (default): a candidate's 23-base window lies fully inside one -E interval; overlap: it shares a base with one", false},
        {'p', "guide-pam", "PAM of the guides to find with -E, two letters of ACGT (default GG)", false},
        {'g', "gc", "MIN,MAX: keep -E candidates with MIN <= G/C among the 20 protospacer bases <= MAX, 0 .. 20 (MAX 0: no upper bound)", false},
        {'t', "t-run", "Keep -E candidates whose longest run of T in the protospacer is at most this, 0 .. 20 (0, the default: no limit; 3 drops TTTT)", false},
        {'s', "strands", "+ | - | both (default): strands on which -E looks for guides", false},
        {'L', "list-guides", "Path to a BED6 file (.bed) that receives the -E candidates: chrom start end guideId 0 strand", false},
        {'N', "region-names", "name | coords: add the interval a hit lies in to the -T file (of the -A regions) and the interval a guide "
                              "was found in to the -L file (of the -E targets), as the BED line's 4th column or as chrom:start-end", false},
        {'F', "forest", "Path to a classifier (.vscrf): adds the columns rfExpectedActive rfActive rfTies ra0 .. ra<M> (needs -C)", false},
        {'C', "activity", "Path to the on-target activities (guideId, sequence, activity per line) of the guides, for -F", false},
        {'r', "rank-by", "mit (default) | votes: rank the -T listing by MIT score or by the classifier's votes (votes needs -F; adds the column rfVotes)", false},
        {'V', "min-votes", "With -r votes: list only off-targets with at least this many of the forest's votes (default: no floor)", false},
        {'v', "vcf", "Path to a VCF (.vcf): adds the columns of the guides in that individual's genome, ind* and var* "
                     "(one device; not with -A, -X, -T, -F)", false},
        {'n', "sample", "With -v: 0-based sample column of the VCF (default 0)", false},
        {'j', "pair-offset", "MIN,MAX: the nickase offset range of the guide pairs of -J (gap between the protospacers' PAM-distal ends, "
                             "negative: overlap; e.g. -4,20); required with -J", false},
        {'J', "pairs", "Path to the TSV file of the guide pairs and their paired off-target sites (.tsv/.txt); needs -j and -E or -B", false},
        {'u', "bulges", "DNA,RNA: largest DNA and RNA bulge, 0 .. 2 each (e.g. 1,1): adds the columns bulgeCount and <class>mm0 .. <class>mm<M> "
                        "of the bulged sites (one device; not with -v, -J)", false},
        {'U', "bulge-hits", "Path to the TSV file of the bulged sites (.tsv/.txt); needs -u", false},
        {'W', "score-table", "Path to a score table (.tsv/.txt; lines 'j g s w' and 'PAM XY w'): adds the columns tableScoreSum tableSpecScore "
                             "tablePositive; with -T, -K / -S (then a table score, 0 .. 1) select by the table score", false},
        {'Y', "efficiency-model", "Path to an on-target efficiency model (.tsv/.txt; lines shape, link, intercept, gc_range, mono, di, gc): "
                                  "adds the columns efficiencyLinear efficiency to the -L file (needs -E, one device)", false},
        {'y', "min-efficiency", "Keep only the -E candidates whose efficiency predictor is defined and >= this value, linear domain (needs -Y)", false},
        {'Z', "sites", "Path to the TSV file of the cut sites (.tsv/.txt): the plain and the bulged alignments collapsed per PAM-side end; "
                       "adds the columns siteCount siteBulgeOnly; needs -u", false},
        {'w', "bulge-table", "Path to the bulge weights (.tsv/.txt; lines 'dna j s w' and 'rna j g w', j = read position 0 .. 19) beside the -W table: "
                             "the cut sites are scored; adds the columns siteScoreSum siteSpecScore sitePositive, and tableScore scoredAs to the -Z "
                             "file, which -K / -S then cut by the site's score; needs -W, -u and -Z", false},
        {'H', "microhomology", "FLANK[,CUT]: adds the columns mhScore oofScore (the microhomology score of Bae et al. 2014 and its out-of-frame "
                               "share in per cent) to the -L file, over FLANK bases (8 .. 32) on either side of the break in front of read "
                               "position CUT (default 17) (needs -E, one device)", false},
        {'m', "min-out-of-frame", "MIN_OOF[,MIN_MH]: keep only the -E candidates whose out-of-frame share is at least MIN_OOF per cent and whose "
                                  "microhomology score is at least MIN_MH (needs -H)", false},
        {'k', "pick", "K[,SPACING]: pick the K best guides (1 .. 32) of every -E target, their cut sites at least SPACING bases apart; adds the "
                      "columns pickTarget pickRank to the -L file (needs -E and -L, one device)", false},
        {'b', "pick-by", "With -k: what to rank by, comma-separated in priority order, out of mit (default), table (needs -W), eff (needs -Y), "
                         "oof, mh (need -H)", false},
        {'c', "pick-target", "With -k: interval (default; every -E interval is a target) or name (the -E intervals with one BED name are one target)", false},
        {'x', "editor", "With -E: CBE | ABE | START,LEN,BASE: the base editor's window in read positions of the site and the base it converts; "
                        "the guide listing gains the last columns editWindow editable targetsHit (one device)", false},
        {'z', "edit-targets", "With -x: path to the target bases (.bed, one base per line): only the candidates whose window holds a target base "
                              "that the editor converts are kept", false},
        {'l', "editable", "With -x: MIN,MAX: keep only the candidates with MIN .. MAX editable bases in the window (0 .. 16)", false},
        {'o', "edit-pairs", "With -z: path to the listing of the pairs: #chrom pos guideId at bystanders", false},
        {'d', "cds", "With -x: path to the coding segments (.bed, BED6: chrom start end transcript phase strand): the guide listing gains the "
                     "last columns codingEdits stopGained missense synonymous - what the editor's full conversion does to the codons", false},
        {'2', "edit-to", "With --cds: the base the editor writes on the read strand (default: the transition partner of the base of -x)", false},
        {'f', "effect-filter", "With --cds: REQUIRE[/FORBID], class names joined by + (synonymous missense stop_gained stop_lost start_lost "
                               "unknown): keep only the candidates with an effect of a REQUIRE class and none of a FORBID class", false},
        {'Q', "effects", "With --cds: path to the listing of the effects: #guideId transcript codon ref alt refAA altAA class at", false},
        {'3', "prime", "With -E: PE2 | NICK,DOWN,PBSMIN,PBSMAX,RTTMIN,RTTMAX,HOMOLOGY,PAMSTART,PAMLEN,SEEDSTART,SEEDLEN,AVOIDG: the prime editor's "
                       "shape; only the candidates with a defined context are kept, and the guide listing gains the last columns pbsLen pbsGC "
                       "primePairs (one device)", false},
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
    opts[77].optional_value = true;  // --knockout [CUT]
    const int pr = parse_args(argc, argv, opts, "Guide summary",
                              "Per-guide off-target counts by mismatch number and MIT specificity score (CRISPOR's "
                              "mitSpecScore) over the same hits as the read mapper, without writing them.");
    if (pr) return pr == 1;
    const std::string genome_path = opts[0].value, index_prefix = opts[1].value, reads_path = opts[2].value, bed_path = opts[3].value;
    const std::string out_path = opts[5].value, pam = opts[6].value;
    const bool discover = opts[14].set;
    const std::string targets_path = opts[14].value, guides_bed_path = opts[20].value;
    if ((int)opts[2].set + (int)opts[3].set + (int)discover != 1) {
        std::fprintf(stderr, "%s: give the guides with exactly one of -R (reads), -B (on-targets) and -E (targets to find guides in)\n", argv[0]);
        return 1;
    }
    if (!has_extension(genome_path, {"fa", "fasta"}) || (opts[2].set && !has_extension(reads_path, {"fa", "fasta"})) ||
        (opts[3].set && !has_extension(bed_path, {"bed"})) || (opts[5].set && !has_extension(out_path, {"tsv", "txt"})) ||
        (discover && !has_extension(targets_path, {"bed"})) || (opts[20].set && !has_extension(guides_bed_path, {"bed"}))) {
        std::fprintf(stderr, "%s: genome and reads must be .fa/.fasta files, on-targets, targets and the guide list .bed files, the output a .tsv/.txt file\n", argv[0]);
        return 1;
    }
    char *end = nullptr;
    const long mm = std::strtol(opts[4].value.c_str(), &end, 10);
    if (end == opts[4].value.c_str() || *end) {
        std::fprintf(stderr, "%s: the given value '%s' cannot be casted to integer\n", argv[0], opts[4].value.c_str());
        return 1;
    }
    if (mm < 0 || mm > 8) {  // bidir_mapping.cpp:234-238
        std::fprintf(stderr, "Error: Maximum number of mismatches must lie between 0 and 8.\n");
        return 1;
    }
    vsc_select sel{};
    const bool listing = opts[10].set;
    const std::string hits_path = opts[10].value;
    if (opts[8].set) {
        const std::string &v = opts[8].value;
        char *kend = nullptr;
        const long long k = std::strtoll(v.c_str(), &kend, 10);
        if (v.empty() || *kend || k < 0 || k > 0xFFFFFFFFll) {
            std::fprintf(stderr, "%s: -K takes a number of hits, 0 (no limit) .. 4294967295, not '%s'\n", argv[0], v.c_str());
            return 1;
        }
        sel.top_k = (uint32_t)k;
    }
    if (opts[9].set) {
        const std::string &v = opts[9].value;
        char *send = nullptr;
        const double x = std::strtod(v.c_str(), &send);
        if (opts[32].set && (v.empty() || *send || !(x >= 0.0 && x <= 1.0))) {
            std::fprintf(stderr, "%s: with -W, -S takes a table score, 0 .. 1, not '%s'\n", argv[0], v.c_str());
            return 1;
        }
        if (v.empty() || *send || !(x >= 0.0 && x <= 100.0)) {
            std::fprintf(stderr, "%s: -S takes an MIT score, 0 .. 100, not '%s'\n", argv[0], v.c_str());
            return 1;
        }
        sel.min_score = (uint32_t)std::ceil(x * (opts[32].set ? 0x1p30 : 0x1p24));  // the smallest fixed-point score that is >= x
    }
    if ((opts[8].set || opts[9].set) && !listing && !opts[36].set) {
        std::fprintf(stderr, "%s: -K / -S select the off-targets listed in the -T file: give -T\n", argv[0]);
        return 1;
    }
    if (listing && !has_extension(hits_path, {"tsv", "txt"})) {
        std::fprintf(stderr, "%s: the -T file must be a .tsv/.txt file\n", argv[0]);
        return 1;
    }
    const bool annotated = opts[11].set;
    const std::string regions_path = opts[11].value;
    uint32_t region_rule = VSC_REGION_OVERLAP;
    vsc_region_filter filter{};
    if (annotated && !has_extension(regions_path, {"bed"})) {
        std::fprintf(stderr, "%s: the -A annotation must be a .bed file\n", argv[0]);
        return 1;
    }
    if (opts[12].set) {
        if (opts[12].value != "overlap" && opts[12].value != "inside") {
            std::fprintf(stderr, "%s: -a takes overlap or inside, not '%s'\n", argv[0], opts[12].value.c_str());
            return 1;
        }
        region_rule = opts[12].value == "inside" ? VSC_REGION_INSIDE : VSC_REGION_OVERLAP;
    }
    if (opts[13].set) {
        if (opts[13].value != "keep" && opts[13].value != "drop") {
            std::fprintf(stderr, "%s: -X takes keep or drop, not '%s'\n", argv[0], opts[13].value.c_str());
            return 1;
        }
        if (!annotated || !listing) {
            std::fprintf(stderr, "%s: -X restricts the -T listing to one side of the -A regions: give both\n", argv[0]);
            return 1;
        }
        filter.scope = opts[13].value == "drop" ? VSC_REGION_DROP : VSC_REGION_KEEP;
    }
    if (opts[12].set && !annotated) {
        std::fprintf(stderr, "%s: -a chooses the rule of the -A regions: give -A\n", argv[0]);
        return 1;
    }
    // -E and its filters (vsc_enum_params)
    vsc_enum_params ep{};
    ep.pam[0] = ep.pam[1] = 'G';
    uint32_t target_rule = VSC_REGION_INSIDE;
    for (int k : {15, 16, 17, 18, 19, 20})
        if (opts[k].set && !discover) {
            std::fprintf(stderr, "%s: -%c belongs to the guide discovery of -E: give -E\n", argv[0], opts[k].short_name);
            return 1;
        }
    if (opts[15].set) {
        if (opts[15].value != "overlap" && opts[15].value != "inside") {
            std::fprintf(stderr, "%s: -e takes inside or overlap, not '%s'\n", argv[0], opts[15].value.c_str());
            return 1;
        }
        target_rule = opts[15].value == "inside" ? VSC_REGION_INSIDE : VSC_REGION_OVERLAP;
    }
    if (opts[16].set) {
        const std::string &v = opts[16].value;
        const std::string acgt = "ACGTacgt";
        if (v.size() != 2 || acgt.find(v[0]) == std::string::npos || acgt.find(v[1]) == std::string::npos) {
            std::fprintf(stderr, "%s: -p takes the two PAM letters of the guides (ACGT), e.g. GG, not '%s'\n", argv[0], v.c_str());
            return 1;
        }
        ep.pam[0] = v[0];
        ep.pam[1] = v[1];
    }
    if (opts[17].set) {
        const std::string &v = opts[17].value;
        char *e1 = nullptr, *e2 = nullptr;
        const long lo = std::strtol(v.c_str(), &e1, 10);
        const long hi = (e1 != v.c_str() && *e1 == ',') ? std::strtol(e1 + 1, &e2, 10) : -1;
        if (e1 == v.c_str() || *e1 != ',' || e2 == e1 + 1 || *e2 || lo < 0 || lo > 20 || hi < 0 || hi > 20 || (hi && lo > hi)) {
            std::fprintf(stderr, "%s: -g takes MIN,MAX with 0 <= MIN <= MAX <= 20 (MAX 0: no upper bound), not '%s'\n", argv[0], v.c_str());
            return 1;
        }
        ep.gc_min = (uint8_t)lo;
        ep.gc_max = (uint8_t)hi;
    }
    if (opts[18].set) {
        const std::string &v = opts[18].value;
        char *tend = nullptr;
        const long k = std::strtol(v.c_str(), &tend, 10);
        if (v.empty() || *tend || k < 0 || k > 20) {
            std::fprintf(stderr, "%s: -t takes the largest run of T, 0 (no limit) .. 20, not '%s'\n", argv[0], v.c_str());
            return 1;
        }
        ep.max_t_run = (uint8_t)k;
    }
    if (opts[19].set) {
        const std::string &v = opts[19].value;
        if (v != "+" && v != "-" && v != "both") {
            std::fprintf(stderr, "%s: -s takes +, - or both, not '%s'\n", argv[0], v.c_str());
            return 1;
        }
        ep.strands = v == "+" ? 1 : v == "-" ? 2 : 0;
    }
    // -Y / -y: the efficiency model of the found guides
    const bool efficient = opts[33].set;
    double min_eff = 0.0;
    if (opts[34].set && !efficient) {
        std::fprintf(stderr, "%s: -y is a floor on the efficiency predictor of the -Y model: give -Y\n", argv[0]);
        return 1;
    }
    if (efficient && !discover) {
        std::fprintf(stderr, "%s: -Y scores the guides that -E finds: give -E\n", argv[0]);
        return 1;
    }
    if (efficient && !has_extension(opts[33].value, {"tsv", "txt"})) {
        std::fprintf(stderr, "%s: the -Y model must be a .tsv/.txt file\n", argv[0]);
        return 1;
    }
    if (opts[34].set) {
        const std::string &v = opts[34].value;
        char *yend = nullptr;
        min_eff = std::strtod(v.c_str(), &yend);
        if (v.empty() || *yend || std::isnan(min_eff)) {
            std::fprintf(stderr, "%s: -y takes a floor on the linear predictor, a number, not '%s'\n", argv[0], v.c_str());
            return 1;
        }
    }
    // -H / -m: the microhomology scores of the found guides
    MhOptions mh;
    {
        const std::string why = parse_mh_options(opts[37].set, opts[37].value, opts[38].set, opts[38].value, discover, (uint32_t)VSC_READ_LEN, 17, &mh);
        if (!why.empty()) {
            std::fprintf(stderr, "%s: %s\n", argv[0], why.c_str());
            return 1;
        }
    }
    const bool naming = opts[21].set;
    if (naming) {
        if (opts[21].value != "name" && opts[21].value != "coords") {
            std::fprintf(stderr, "%s: -N takes name or coords, not '%s'\n", argv[0], opts[21].value.c_str());
            return 1;
        }
        if (!(annotated && listing) && !(discover && opts[20].set)) {
            std::fprintf(stderr, "%s: -N names the -A interval of a hit in the -T file or the -E interval of a guide in the -L file: give -A and -T, or -E and -L\n", argv[0]);
            return 1;
        }
    }
    const bool by_name = naming && opts[21].value == "name";
    std::vector<int> devices;  // -D 0 | -D 0,1,2,3 (an id may repeat: several shards on one device)
    {
        const std::string d = opts[7].set ? opts[7].value : "0";
        size_t b = 0;
        for (;;) {
            const size_t e = d.find(',', b);
            const std::string item = d.substr(b, e == std::string::npos ? std::string::npos : e - b);
            char *iend = nullptr;
            const long v = std::strtol(item.c_str(), &iend, 10);
            if (item.empty() || *iend || v < 0) {
                std::fprintf(stderr, "%s: bad device list '%s'\n", argv[0], d.c_str());
                return 1;
            }
            devices.push_back((int)v);
            if (e == std::string::npos) break;
            b = e + 1;
        }
    }

    // -F / -C / -r / -V: the classifier
    const bool classified = opts[22].set;
    if (opts[22].set != opts[23].set || (classified && !has_extension(opts[22].value, {"vscrf"}))) {
        std::fprintf(stderr, "%s: the classifier needs both -F (a .vscrf forest) and -C (the guides' on-target activities)\n", argv[0]);
        return 1;
    }
    if (opts[24].set && opts[24].value != "mit" && opts[24].value != "votes") {
        std::fprintf(stderr, "%s: -r takes mit or votes, not '%s'\n", argv[0], opts[24].value.c_str());
        return 1;
    }
    const bool by_votes = opts[24].set && opts[24].value == "votes";
    vsc_select_votes vsel{};
    vsel.top_k = sel.top_k;
    if (by_votes && (!classified || !listing || annotated || opts[9].set || devices.size() != 1)) {
        std::fprintf(stderr, "%s: -r votes ranks the -T listing by the classifier: give -T, -F and -C, on one device, without -A and -S\n", argv[0]);
        return 1;
    }
    if (opts[25].set) {
        const std::string &v = opts[25].value;
        char *vend = nullptr;
        const long long k = std::strtoll(v.c_str(), &vend, 10);
        if (!by_votes || v.empty() || *vend || k < 0 || k > 65535) {
            std::fprintf(stderr, "%s: -V takes a number of votes, 0 .. 65535, with -r votes, not '%s'\n", argv[0], v.c_str());
            return 1;
        }
        vsel.min_votes = (uint32_t)k;
    }

    // -v / -n: the individual
    const bool individual = opts[26].set;
    uint32_t vcf_sample = 0;
    if (individual && !has_extension(opts[26].value, {"vcf"})) {
        std::fprintf(stderr, "%s: the -v file must be a .vcf file\n", argv[0]);
        return 1;
    }
    if (individual && (annotated || opts[13].set || listing || classified || devices.size() != 1)) {
        std::fprintf(stderr, "%s: -v screens one individual on one device: it does not combine with -A, -X, -T, -F or a device list\n", argv[0]);
        return 1;
    }
    if (opts[27].set) {
        const std::string &v = opts[27].value;
        char *nend = nullptr;
        const long long k = std::strtoll(v.c_str(), &nend, 10);
        if (!individual || v.empty() || *nend || k < 0 || k > 0xFFFFFFFFll) {
            std::fprintf(stderr, "%s: -n takes the 0-based sample column of the -v file, not '%s'\n", argv[0], v.c_str());
            return 1;
        }
        vcf_sample = (uint32_t)k;
    }

    // -j / -J: the guide pairs
    const bool pairing = opts[29].set;
    const std::string pairs_path = opts[29].value;
    vsc_pair_params pp{};
    if (pairing != opts[28].set) {
        std::fprintf(stderr, "%s: the pair screen needs both -J (the pairs' file) and -j MIN,MAX (the offset range)\n", argv[0]);
        return 1;
    }
    if (pairing) {
        const std::string &v = opts[28].value;
        char *e1 = nullptr, *e2 = nullptr;
        const long lo = std::strtol(v.c_str(), &e1, 10);
        const long hi = (e1 != v.c_str() && *e1 == ',') ? std::strtol(e1 + 1, &e2, 10) : 0;
        const long lim = (1l << 30) - VSC_READ_LEN;
        if (e1 == v.c_str() || *e1 != ',' || e2 == e1 + 1 || *e2 || lo > hi || lo < -lim || hi > lim) {
            std::fprintf(stderr, "%s: -j takes MIN,MAX with MIN <= MAX, e.g. -4,20, not '%s'\n", argv[0], v.c_str());
            return 1;
        }
        pp.delta_min = (int32_t)lo + VSC_READ_LEN;  // delta = pos('+') - pos('-') = offset + 23
        pp.delta_max = (int32_t)hi + VSC_READ_LEN;
        if (!has_extension(pairs_path, {"tsv", "txt"})) {
            std::fprintf(stderr, "%s: the -J file must be a .tsv/.txt file\n", argv[0]);
            return 1;
        }
        if (opts[2].set) {
            std::fprintf(stderr, "%s: -J pairs guides by their loci, which -R reads do not have: give the guides with -E or -B\n", argv[0]);
            return 1;
        }
        if (individual) {
            std::fprintf(stderr, "%s: -J does not combine with -v\n", argv[0]);
            return 1;
        }
    }

    // -u / -U: the bulged sites
    const bool bulged = opts[30].set;
    const std::string bulges_path = opts[31].value;
    vsc_bulge_params bp{};
    if (bulged) {
        const std::string &v = opts[30].value;
        char *e1 = nullptr, *e2 = nullptr;
        const long dna = std::strtol(v.c_str(), &e1, 10);
        const long rna = (e1 != v.c_str() && *e1 == ',') ? std::strtol(e1 + 1, &e2, 10) : -1;
        if (e1 == v.c_str() || *e1 != ',' || e2 == e1 + 1 || *e2 || dna < 0 || dna > 2 || rna < 0 || rna > 2 || (dna == 0 && rna == 0)) {
            std::fprintf(stderr, "%s: -u takes DNA,RNA, the largest bulges, 0 .. 2 each and not both 0 (e.g. 1,1), not '%s'\n", argv[0], v.c_str());
            return 1;
        }
        bp.dna_max = (uint32_t)dna;
        bp.rna_max = (uint32_t)rna;
        if (individual || pairing || devices.size() != 1) {
            std::fprintf(stderr, "%s: -u searches the bulged sites on one device: it does not combine with -v, -J or a device list\n", argv[0]);
            return 1;
        }
    }
    if (opts[31].set && (!bulged || !has_extension(bulges_path, {"tsv", "txt"}))) {
        std::fprintf(stderr, "%s: -U lists the bulged sites of -u in a .tsv/.txt file: give -u\n", argv[0]);
        return 1;
    }

    const bool sited = opts[35].set;
    const std::string sites_path = opts[35].value;
    if (sited && (!bulged || !has_extension(sites_path, {"tsv", "txt"}))) {
        std::fprintf(stderr, "%s: -Z lists the cut sites of -u in a .tsv/.txt file: give -u\n", argv[0]);
        return 1;
    }

    // -W: the score table
    const bool tabled = opts[32].set;
    if (tabled && !has_extension(opts[32].value, {"tsv", "txt"})) {
        std::fprintf(stderr, "%s: the -W table must be a .tsv/.txt file\n", argv[0]);
        return 1;
    }
    if (tabled && (individual || (listing && (annotated || by_votes || devices.size() != 1)))) {
        std::fprintf(stderr, "%s: -W does not combine with -v; with -T it selects by the table score on one device, without -A and -r votes\n", argv[0]);
        return 1;
    }

    // -w: the bulge weights beside -W
    const bool site_scored = opts[36].set;
    if (site_scored && (!tabled || !bulged || !sited || !has_extension(opts[36].value, {"tsv", "txt"}))) {
        std::fprintf(stderr, "%s: -w scores the cut sites of -Z with the bulge weights of a .tsv/.txt file beside the -W table: give -W, -u and -Z\n", argv[0]);
        return 1;
    }

    if (efficient && devices.size() != 1) {
        std::fprintf(stderr, "%s: -Y scores the candidates on one device: it does not combine with a device list\n", argv[0]);
        return 1;
    }

    if (mh.on && devices.size() != 1) {
        std::fprintf(stderr, "%s: -H scores the candidates on one device: it does not combine with a device list\n", argv[0]);
        return 1;
    }

    // -k / -b / -c: the best guides of every -E target
    PickOptions pick;
    {
        std::map<std::string, std::string> needs;
        if (!tabled) needs["table"] = "give -W";
        if (!efficient) needs["eff"] = "give -Y";
        if (!mh.on) needs["oof"] = needs["mh"] = "give -H";
        std::string why = parse_pick_options(opts[39].set, opts[39].value, opts[40].set, opts[40].value, opts[41].set, opts[41].value, discover, "-E",
                                             devices.size() != 1, needs, &pick);
        if (why.empty() && pick.on && !opts[20].set) why = "-k marks its picks in the -L file: give -L";
        if (!why.empty()) {
            std::fprintf(stderr, "%s: %s\n", argv[0], why.c_str());
            return 1;
        }
    }

    // -x / -z / -l / -o: the base-editor windows of the found guides
    EditOptions edit;
    {
        const std::string why = parse_edit_options(opts[42].set, opts[42].value, opts[43].set, opts[43].value, opts[44].set, opts[44].value,
                                                   opts[45].set, opts[45].value, discover, devices.size() != 1, (uint32_t)VSC_READ_LEN, &edit);
        if (!why.empty()) {
            std::fprintf(stderr, "%s: %s\n", argv[0], why.c_str());
            return 1;
        }
    }

    // --cds / --edit-to / --effect-filter / --effects: what the editor does to the codons
    EffectsOptions fx;
    {
        const std::string why = parse_effects_options(opts[46].set, opts[46].value, opts[47].set, opts[47].value, opts[48].set, opts[48].value,
                                                      opts[49].set, opts[49].value, edit, &fx);
        if (!why.empty()) {
            std::fprintf(stderr, "%s: %s\n", argv[0], why.c_str());
            return 1;
        }
    }
    CdsOfFile coding;

    // --prime / --prime-edits / --prime-allow-weak / --prime-out: the pegRNA extensions of the found guides
    PrimeOptions prime;
    {
        const std::string why = parse_prime_options(opts[50].set, opts[50].value, opts[51].set, opts[51].value, opts[52].set, opts[53].set,
                                                    opts[53].value, discover, devices.size() != 1, (uint32_t)VSC_READ_LEN, &prime);
        if (!why.empty()) {
            std::fprintf(stderr, "%s: %s\n", argv[0], why.c_str());
            return 1;
        }
    }

    // --hdr / --hdr-edits / --hdr-out / --hdr-cds / --hdr-allow-open: knock-in design for the found guides
    HdrOptions hdr;
    {
        const std::string why = parse_hdr_options(opts[61], opts[62], opts[63], opts[64], opts[65], discover, devices.size() != 1, (uint32_t)VSC_READ_LEN, &hdr);
        if (!why.empty()) {
            std::fprintf(stderr, "%s: %s\n", argv[0], why.c_str());
            return 1;
        }
    }
    CdsOfFile hdr_coding;
    // --fold / --fold-scaffold / --max-fold: the self-complementarity of the found guides
    FoldOptions fold;
    {
        const std::string why = parse_fold_options(opts[66], opts[67], opts[68], discover, devices.size() != 1, (uint32_t)VSC_READ_LEN, &fold);
        if (!why.empty()) {
            std::fprintf(stderr, "%s: %s\n", argv[0], why.c_str());
            return 1;
        }
    }

    // --motifs and its options: restriction sites and motifs in the found guides' construct and context
    MotifOptions motif;
    {
        const std::string why = parse_motif_options(opts[69], opts[70], opts[71], opts[72], opts[73], opts[74], opts[75], opts[76], discover, devices.size() != 1, (uint32_t)VSC_READ_LEN, &motif);
        if (!why.empty()) {
            std::fprintf(stderr, "%s: %s\n", argv[0], why.c_str());
            return 1;
        }
    }

    // --knockout and its options: where the found guides cut the coding sequence, and what a frameshift there does
    KnockoutOptions knockout;
    {
        const std::string why = parse_knockout_options(opts[77], opts[78], opts[79], opts[80], opts[81], discover, devices.size() != 1, (uint32_t)VSC_READ_LEN, &knockout);
        if (!why.empty()) {
            std::fprintf(stderr, "%s: %s\n", argv[0], why.c_str());
            return 1;
        }
    }
    CdsOfFile knockout_coding;

    // --variants and its options: the known variants under the found guides' own sites
    VariationOptions variation;
    {
        const std::string guide_pam = opts[16].set ? opts[16].value : "GG";
        const std::string why = parse_variation_options(opts[54], opts[55], opts[56], opts[57], opts[58], opts[59], opts[60], discover, devices.size() != 1,
                                                        std::string(21, 'N') + guide_pam, 0, 20, &variation);
        if (!why.empty()) {
            std::fprintf(stderr, "%s: %s\n", argv[0], why.c_str());
            return 1;
        }
    }

    vsc_ctx *ctx = nullptr;
    vsc_score_table *table = nullptr;
    vsc_bulge_table *bulge_table = nullptr;
    vsc_sites *scored_sites = nullptr;
    EffAnyModel eff_model;  // -Y: a linear model, or - a file with a `tree` line - a tree model
    vsc_genome *genome = nullptr;
    vsc_bulge_hits *bulge_hits = nullptr;
    vsc_hits *site_plain = nullptr;
    vsc_sites *sites = nullptr;
    vsc_genome *win_genome = nullptr;
    vsc_windows *windows = nullptr;
    vsc_variant_map *vmap = nullptr;
    vsc_multi *multi = nullptr;
    vsc_multi_genome *mgenome = nullptr;
    vsc_hits *hits = nullptr, *pair_hits = nullptr;
    vsc_regions *regions = nullptr, *targets = nullptr;
    vsc_guides *found = nullptr;
    int rc = 1;
    try {
        if (efficient) {  // (read before the index and the device: a model that does not fit costs nothing)
            vsc_eff_shape eff_shape{};
            eff_model = load_eff_any(opts[33].value, &eff_shape);
            if (eff_shape.site_len != (uint32_t)VSC_READ_LEN)
                throw std::runtime_error("-Y: the model's site_len is " + std::to_string(eff_shape.site_len) + "; the guides are 23 bases long");
        }
        const PackedIndex ix = read_index(index_prefix);
        uint64_t size = 0;
        int64_t mtime = 0;
        if (ix.src_size && (!file_stamp(genome_path, &size, &mtime) || size != ix.src_size || mtime != ix.src_mtime))
            throw std::runtime_error("index " + index_path(index_prefix) + " was not packed from " + genome_path);
        std::map<std::string, uint32_t> by_chrom;  // first word of the contig name, as the -T file prints it
        for (size_t c = ix.names.size(); c-- > 0;) by_chrom[ix.names[c].substr(0, ix.names[c].find_first_of(" \t"))] = (uint32_t)c;
        // the intervals of a BED3+ file (-A, -E); desc (-N): what names each of them - its 4th column or chrom:start-end as given
        auto read_bed3 = [&](const std::string &path, const std::string &flag, std::vector<std::string> *desc) {
            std::ifstream bed(path);
            if (!bed) throw std::runtime_error("Could not open the " + flag + " file.");
            std::vector<vsc_interval> iv;
            std::string line;
            while (std::getline(bed, line)) {
                if (line.empty() || line[0] == '#' || line.compare(0, 5, "track") == 0 || line.compare(0, 7, "browser") == 0) continue;
                std::istringstream is(line);
                std::string chr;
                unsigned long long start = 0, stop = 0;
                if (!(is >> chr >> start >> stop)) throw std::runtime_error(flag + ": not a BED line: '" + line + "'");
                auto it = by_chrom.find(chr);
                if (it == by_chrom.end()) throw std::runtime_error(flag + ": no sequence '" + chr + "' in the genome");
                if (start > stop || stop > 0xFFFFFFFFull) throw std::runtime_error(flag + ": bad interval in '" + line + "'");
                iv.push_back(vsc_interval{it->second, (uint32_t)start, (uint32_t)stop, 0u});
                if (desc) {
                    std::string name;
                    if (!by_name || !(is >> name)) name = chr + ':' + std::to_string(start) + '-' + std::to_string(stop);
                    desc->push_back(name);
                }
            }
            return iv;
        };
        // the guides (+ their excluded loci)
        std::vector<std::string> ids, seqs;
        std::vector<vsc_locus> loci;
        std::vector<std::string> region_desc, target_desc;  // -N: per line of the -A / -E file
        std::vector<uint32_t> pick_group;       // -k -c name: the target of every -E interval
        std::vector<std::string> target_names;  // -k: what pickTarget prints per target
        if (pick.on) pick_targets(pick, targets_path, "-E", &pick_group, &target_names);  // (before a device is opened: -c name may refuse the file)
        if (discover) {  // the guides themselves come from the device, below
            const std::vector<vsc_interval> iv = read_bed3(targets_path, "-E", naming && opts[20].set ? &target_desc : nullptr);
            if (vsc_regions_build(ix.contigs.data(), (uint32_t)ix.contigs.size(), iv.data(), iv.size(), target_rule, &targets) != VSC_OK)
                throw std::runtime_error("could not build the regions of the -E file");
            std::fprintf(stderr, "Targets loaded (total: %zu).\n", iv.size());
        } else if (opts[2].set) {
            for (auto &r : read_fasta(reads_path)) {
                ids.push_back(r.id);
                seqs.push_back(r.seq);
            }
        } else {
            const vsc_merge::Genome text(genome_path);
            std::ifstream bed(bed_path);
            if (!bed) throw std::runtime_error("Could not open BED file.");
            std::string line;
            while (std::getline(bed, line)) {  // as fasta_writer reads it
                if (line.empty() || line[0] == '#') continue;
                std::istringstream is(line);
                std::string chr, name, score, strand;
                unsigned long start = 0, stop = 0;
                if (!(is >> chr >> start >> stop >> name >> score >> strand)) continue;
                const char s = strand.empty() ? '+' : strand[0];
                auto it = text.by_name.find(chr);
                if (it == text.by_name.end()) throw std::runtime_error("on-target '" + name + "': no sequence '" + chr + "' in the genome");
                ids.push_back(name);
                seqs.push_back(text.region_at(it->second, (uint32_t)start, (uint32_t)stop, s));
                loci.push_back(vsc_locus{(uint32_t)it->second, (uint32_t)start, s == '-' ? 1u : 0u, 0u});
            }
        }
        std::vector<uint64_t> codes(seqs.size());
        for (size_t i = 0; i < seqs.size(); ++i) {
            if (seqs[i].size() != VSC_READ_LEN)
                throw std::runtime_error("guide '" + ids[i] + "' is not 23 nt long (VARSCOT searches 20 nt + PAM)");
            codes[i] = vsc_pack_guide(seqs[i].c_str());
        }
        if (!discover) std::fprintf(stderr, "Guides loaded (total: %zu).\n", seqs.size());
        if (annotated) {
            const std::vector<vsc_interval> iv = read_bed3(regions_path, "-A", naming && listing ? &region_desc : nullptr);
            if (vsc_regions_build(ix.contigs.data(), (uint32_t)ix.contigs.size(), iv.data(), iv.size(), region_rule, &regions) != VSC_OK)
                throw std::runtime_error("could not build the regions of the -A file");
            filter.regions = regions;
            std::fprintf(stderr, "Regions loaded (total: %zu).\n", iv.size());
        }
        int st;
        if (devices.size() == 1) {
            st = vsc_ctx_create(devices[0], &ctx);
            if (st != VSC_OK) throw std::runtime_error(st == VSC_ERR_NODEVICE ? "no HIP device available (there is no CPU fallback)" : "could not create the device context");
            st = vsc_genome_load(ctx, ix.hi.data(), ix.lo.data(), ix.nm.data(), 0, ix.hi.size(), ix.hi.size(), ix.contigs.data(),
                                 (uint32_t)ix.contigs.size(), &genome);
            if (st != VSC_OK) throw std::runtime_error(vsc_last_error(ctx));
            if (pam.size() != 2 && std::ifstream(seed_index_path(index_prefix)).good() &&
                vsc_genome_index_load(ctx, genome, seed_index_path(index_prefix).c_str()) != VSC_OK)
                std::fprintf(stderr, "%s: %s - building the seed index instead\n", argv[0], vsc_last_error(ctx));
        } else {
            st = vsc_multi_create(devices.data(), (int)devices.size(), &multi);
            if (st != VSC_OK) throw std::runtime_error(st == VSC_ERR_NODEVICE ? "no HIP device available (there is no CPU fallback)" : "could not create the device contexts");
            st = vsc_multi_genome_load(multi, ix.hi.data(), ix.lo.data(), ix.nm.data(), ix.hi.size(), ix.contigs.data(),
                                       (uint32_t)ix.contigs.size(), &mgenome);
            if (st != VSC_OK) throw std::runtime_error(vsc_multi_last_error(multi));
        }
        std::fprintf(stderr, "Index loaded.\n");

        vsc_search_params p{};
        p.max_mismatches = (uint32_t)mm;
        if (pam.size() == 2) {  // a PAM of any other length can never equal a 2-base window slice (:71-76)
            p.has_extra_pam = 1;
            p.extra_pam[0] = pam[0];
            p.extra_pam[1] = pam[1];
        }
        std::vector<double> eff_linear;    // -Y: the found guides' predictors
        std::vector<uint32_t> mh_pairs;    // -H: their (sum, oof) pairs
        std::vector<std::string> bed_lines;  // -k: the -L lines wait for the search, whose rows the picks rank by
        std::vector<std::string> edit_cols;  // -k with -x: the edit columns stay the last ones, behind the picks'
        if (discover) {
            st = multi ? vsc_multi_guides_enumerate(multi, mgenome, targets, &ep, &found) : vsc_guides_enumerate(ctx, genome, targets, &ep, &found);
            if (st != VSC_OK) throw std::runtime_error(multi ? vsc_multi_last_error(multi) : vsc_last_error(ctx));
            if (efficient) {  // -y: the survivors replace the candidates; -Y: their predictors, where they lie
                if (opts[34].set) {
                    vsc_guides *kept = nullptr;
                    if (eff_any_filter(ctx, genome, found, eff_model, min_eff, &kept) != VSC_OK) throw std::runtime_error(vsc_last_error(ctx));
                    vsc_guides_free(found);
                    found = kept;
                }
            }
            if (mh.floored) {  // -m: the same for the microhomology floors
                vsc_guides *kept = nullptr;
                if (vsc_guides_filter_microhomology(ctx, genome, found, &mh.shape, mh.min_sum, mh.min_oof_permille, &kept) != VSC_OK)
                    throw std::runtime_error(vsc_last_error(ctx));
                vsc_guides_free(found);
                found = kept;
            }
            std::vector<vsc_edit_target> edit_targets;
            if (edit.with_targets) edit_targets = read_edit_targets(edit.targets_path, ix.names);
            if (edit.filtered) {  // -z / -l: the same for the editor's FILTER
                vsc_guides *kept = nullptr;
                if (vsc_guides_filter_edit(ctx, genome, found, &edit.shape, edit_targets.empty() ? nullptr : edit_targets.data(), edit_targets.size(),
                                           edit.min_editable, edit.max_editable, &kept) != VSC_OK)
                    throw std::runtime_error(vsc_last_error(ctx));
                vsc_guides_free(found);
                found = kept;
            }
            if (fx.on) read_cds(fx.cds_path, ix.names, ix.contigs, &coding);
            if (fx.filtered) {  // --effect-filter: the same for the effects' FILTER, after the editor's
                vsc_guides *kept = nullptr;
                if (vsc_guides_filter_effects(ctx, genome, found, &edit.shape, fx.to, coding.cds, nullptr, fx.require, fx.forbid, &kept) != VSC_OK)
                    throw std::runtime_error(vsc_last_error(ctx));
                vsc_guides_free(found);
                found = kept;
            }
            std::vector<vsc_prime_edit> prime_edits;
            if (prime.with_edits) prime_edits = read_prime_edits(prime.edits_path, ix.names);
            if (prime.on) {  // --prime: the same for the prime editor's FILTER, after the editor's and the effects'
                vsc_guides *kept = nullptr;
                if (vsc_guides_filter_prime(ctx, genome, found, &prime.shape, prime_edits.empty() ? nullptr : prime_edits.data(), prime_edits.size(),
                                            prime.allow_weak, &kept) != VSC_OK)
                    throw std::runtime_error(vsc_last_error(ctx));
                vsc_guides_free(found);
                found = kept;
            }
            std::vector<vsc_variant> variants;
            if (variation.on) variants = read_variants(variation, ix.names, ix.contigs);
            if (variation.filtered) {  // the bounds and the required zones: the same for the variation FILTER, after all others
                vsc_guides *kept = nullptr;
                if (vsc_guides_filter_variation(ctx, genome, found, &variation.shape, variants.empty() ? nullptr : variants.data(), variants.size(),
                                                &variation.filter, &kept) != VSC_OK)
                    throw std::runtime_error(vsc_last_error(ctx));
                vsc_guides_free(found);
                found = kept;
            }
            std::vector<vsc_prime_edit> hdr_edits;
            if (hdr.with_edits) hdr_edits = read_prime_edits(hdr.edits_path, ix.names);
            if (hdr.with_cds) read_cds(hdr.cds_path, ix.names, ix.contigs, &hdr_coding);
            if (hdr.on) {  // --hdr: the same for the knock-in FILTER, after all others
                vsc_guides *kept = nullptr;
                if (vsc_guides_filter_hdr(ctx, genome, found, &hdr.shape, hdr_edits.empty() ? nullptr : hdr_edits.data(), hdr_edits.size(), hdr_coding.cds,
                        nullptr, hdr.allow_open, &kept) != VSC_OK)
                    throw std::runtime_error(vsc_last_error(ctx));
                vsc_guides_free(found);
                found = kept;
            }
            if (fold.limited) {  // --max-fold: the same for the fold limits, after the knock-in FILTER
                vsc_guides *kept = nullptr;
                if (vsc_guides_filter_fold(ctx, genome, found, &fold.shape, fold.scaffold.c_str(), (uint32_t)fold.scaffold.size(), &fold.limits, &kept) != VSC_OK)
                    throw std::runtime_error(vsc_last_error(ctx));
                vsc_guides_free(found);
                found = kept;
            }
            if (motif.limited) {  // --motif-forbid / --motif-forbid-context / --motif-require-cut: the same, after the fold FILTER
                vsc_guides *kept = nullptr;
                if (vsc_guides_filter_motifs(ctx, genome, found, &motif.shape, motif.left.c_str(), (uint32_t)motif.left.size(), motif.right.c_str(),
                                     (uint32_t)motif.right.size(), motif.motifs.data(), (uint32_t)motif.motifs.size(), &motif.limits, &kept) != VSC_OK)
                    throw std::runtime_error(vsc_last_error(ctx));
                vsc_guides_free(found);
                found = kept;
            }
            if (knockout.on) read_cds(knockout.cds_path, ix.names, ix.contigs, &knockout_coding);
            if (knockout.filtered) {  // --knockout-filter: the same, after the motif FILTER
                vsc_guides *kept = nullptr;
                if (vsc_guides_filter_knockout(ctx, genome, found, &knockout.shape, knockout_coding.cds, nullptr, &knockout.limits, &kept) != VSC_OK)
                    throw std::runtime_error(vsc_last_error(ctx));
                vsc_guides_free(found);
                found = kept;
            }
            if (efficient) {
                eff_linear.resize(vsc_guides_count(found));
                if (eff_any_score(ctx, genome, found, eff_model, eff_linear.data()) != VSC_OK) throw std::runtime_error(vsc_last_error(ctx));
            }
            mh_pairs.resize(mh.on ? 2 * vsc_guides_count(found) : 0);
            if (mh.on && vsc_guides_microhomology(ctx, genome, found, &mh.shape, mh_pairs.data(), nullptr) != VSC_OK)
                throw std::runtime_error(vsc_last_error(ctx));
            std::vector<uint32_t> edit_rows;  // -x: the (mask, hits) rows, and with -o the pairs
            std::vector<vsc_edit_pair> edit_pairs;
            if (edit.on)
                edit_rows_and_pairs(edit, vsc_guides_count(found), [&](uint32_t *r, vsc_edit_pair *pp, uint64_t cap, uint64_t *np) {
                    if (vsc_guides_edit(ctx, genome, found, &edit.shape, edit_targets.empty() ? nullptr : edit_targets.data(), edit_targets.size(), r, pp,
                                        cap, np, nullptr, nullptr) != VSC_OK)
                        throw std::runtime_error(vsc_last_error(ctx));
                }, &edit_rows, &edit_pairs);
            std::vector<uint32_t> fx_rows;  // --cds: the effect rows, and with --effects the records
            std::vector<vsc_effect> fx_records;
            if (fx.on)
                effects_rows_and_records(fx, vsc_guides_count(found), [&](uint32_t *r, vsc_effect *e, uint64_t cap, uint64_t *ne) {
                    if (vsc_guides_effects(ctx, genome, found, &edit.shape, fx.to, coding.cds, nullptr, r, e, cap, ne, nullptr, nullptr) != VSC_OK)
                        throw std::runtime_error(vsc_last_error(ctx));
                }, &fx_rows, &fx_records);
            std::vector<uint32_t> prime_rows;  // --prime: the (pbs, n_pairs) rows, and with --prime-out the pairs
            std::vector<vsc_prime_pair> prime_pairs;
            if (prime.on)
                prime_rows_and_pairs(prime, vsc_guides_count(found), [&](uint32_t *r, vsc_prime_pair *pp, uint64_t cap, uint64_t *np) {
                    if (vsc_guides_prime(ctx, genome, found, &prime.shape, prime_edits.empty() ? nullptr : prime_edits.data(), prime_edits.size(), r, pp,
                                         cap, np, nullptr, nullptr) != VSC_OK)
                        throw std::runtime_error(vsc_last_error(ctx));
                }, &prime_rows, &prime_pairs);
            std::vector<uint32_t> variation_rows;  // --variation-out: the rows and the pairs
            std::vector<vsc_variation_pair> variation_pairs;
            if (variation.with_out)
                variation_rows_and_pairs(vsc_guides_count(found), [&](uint32_t *r, vsc_variation_pair *pp, uint64_t cap, uint64_t *np) {
                    if (vsc_guides_variation(ctx, genome, found, &variation.shape, variants.empty() ? nullptr : variants.data(), variants.size(), r, pp,
                                             cap, np, nullptr, nullptr) != VSC_OK)
                        throw std::runtime_error(vsc_last_error(ctx));
                }, &variation_rows, &variation_pairs);
            std::vector<uint32_t> hdr_rows;  // --hdr: the (n_pairs, n_usable) rows, and with --hdr-out the pairs
            std::vector<vsc_hdr_pair> hdr_pairs;
            if (hdr.on)
                hdr_rows_and_pairs(hdr, vsc_guides_count(found), [&](uint32_t *r, vsc_hdr_pair *pp, uint64_t cap, uint64_t *np) {
                    if (vsc_guides_hdr(ctx, genome, found, &hdr.shape, hdr_edits.empty() ? nullptr : hdr_edits.data(), hdr_edits.size(), hdr_coding.cds, nullptr,
                            r, pp, cap, np, nullptr, nullptr) != VSC_OK)
                        throw std::runtime_error(vsc_last_error(ctx));
                }, &hdr_rows, &hdr_pairs);
            std::vector<uint32_t> fold_rows(fold.on ? 2 * vsc_guides_count(found) : 0);  // --fold: the rows
            if (fold.on && vsc_guides_fold(ctx, genome, found, &fold.shape, fold.scaffold.c_str(), (uint32_t)fold.scaffold.size(), fold_rows.data(), nullptr) != VSC_OK)
                throw std::runtime_error(vsc_last_error(ctx));
            std::vector<uint64_t> motif_rows(motif.on ? 3 * vsc_guides_count(found) : 0);  // --motifs: the rows
            if (motif.on && vsc_guides_motifs(ctx, genome, found, &motif.shape, motif.left.c_str(), (uint32_t)motif.left.size(), motif.right.c_str(),
                                              (uint32_t)motif.right.size(), motif.motifs.data(), (uint32_t)motif.motifs.size(), motif_rows.data(),
                                              nullptr, nullptr) != VSC_OK)
                throw std::runtime_error(vsc_last_error(ctx));
            std::vector<uint32_t> knockout_rows(knockout.on ? 4 * vsc_guides_count(found) : 0);  // --knockout: the rows
            if (knockout.on && vsc_guides_knockout(ctx, genome, found, &knockout.shape, knockout_coding.cds, nullptr, knockout_rows.data(), nullptr,
                                                   nullptr) != VSC_OK)
                throw std::runtime_error(vsc_last_error(ctx));
            const uint64_t *fc = nullptr;
            const vsc_locus *fl = nullptr;
            if (vsc_guides_data(found, &fc, &fl) != VSC_OK) throw std::runtime_error(multi ? "could not read the candidates" : vsc_last_error(ctx));
            const uint64_t n = vsc_guides_count(found);
            if (n >= (1ull << 31)) throw std::runtime_error("-E: too many candidates for one search; narrow the targets or the filters");
            codes.assign(fc, fc + n);
            loci.assign(fl, fl + n);
            std::vector<uint32_t> from(target_desc.empty() ? 0 : n);  // -N: the -E interval each candidate lies in
            if (!from.empty() && (st = vsc_guides_locate(found, targets, from.data())) != VSC_OK)
                throw std::runtime_error(multi || st == VSC_ERR_RANGE ? "could not name the targets of the candidates" : vsc_last_error(ctx));
            std::string bed6;
            for (uint64_t i = 0; i < n; ++i) {
                const std::string &name = ix.names[fl[i].contig];
                const std::string chrom = name.substr(0, name.find_first_of(" \t"));
                const char strand = fl[i].strand ? '-' : '+';
                std::string seq(VSC_READ_LEN, 'A');
                for (int j = 0; j < VSC_READ_LEN; ++j) seq[j] = "ACGT"[(fc[i] >> (2 * j)) & 3u];
                ids.push_back(chrom + ':' + std::to_string(fl[i].pos) + ':' + strand);
                seqs.push_back(seq);
                if (opts[20].set) {
                    const std::string line = chrom + '\t' + std::to_string(fl[i].pos) + '\t' + std::to_string(fl[i].pos + VSC_READ_LEN) + '\t' + ids.back() +
                            "\t0\t" + strand + (from.empty() ? "" : '\t' + (from[i] < target_desc.size() ? target_desc[from[i]] : "-")) +
                            (efficient ? '\t' + eff_text(eff_linear[i]) + '\t' + eff_text(eff_any_link(eff_model, eff_linear[i])) : "") +
                            (mh.on ? mh_columns(&mh_pairs[2 * i]) : "");
                    const std::string ecol = (edit.on ? edit_columns(edit.shape, seq, &edit_rows[2 * i]) : "") +
                                             (fx.on ? effects_columns(&fx_rows[2 * i]) : "") + (prime.on ? prime_columns(&prime_rows[2 * i]) : "") +
                                             (hdr.on ? hdr_columns(&hdr_rows[2 * i]) : "") + (fold.on ? fold_columns(&fold_rows[2 * i]) : "") +
                                             (motif.on ? motif_columns(motif, &motif_rows[3 * i]) : "") +
                                             (knockout.on ? knockout_columns(&knockout_rows[4 * i], knockout_coding.transcripts) : "");
                    if (pick.on) bed_lines.push_back(line), edit_cols.push_back(ecol);
                    else bed6 += line + ecol + '\n';
                }
            }
            if (opts[20].set && !pick.on) {
                std::ofstream out(guides_bed_path);
                if (!out.is_open()) throw std::runtime_error("Could not open the -L path.");
                out << bed6;
                out.close();
                if (!out) throw std::runtime_error("Could not write the -L file.");
            }
            if (edit.with_pairs) write_edit_pairs(edit.pairs_path, edit_pairs, edit_targets, ix.names, ids);
            if (fx.with_listing) write_effects(fx.effects_path, fx_records, coding.transcripts, ids);
            if (prime.with_pairs) write_prime_pairs(prime.pairs_path, prime.shape, prime_pairs, prime_edits, loci, ix, ids);
            if (variation.with_out) write_variation(variation.out_path, variation_rows, variation_pairs, variants, ix.names, ids);
            if (hdr.with_pairs) write_hdr_pairs(hdr.pairs_path, hdr.shape, hdr_pairs, hdr_edits, loci, ix.names, ids);
            if (motif.on && !motif.out_path.empty()) write_motifs(motif, motif_rows, ids);
            if (knockout.on && !knockout.out_path.empty()) write_knockout(knockout.out_path, knockout_rows, knockout_coding.transcripts, ids);
            std::fprintf(stderr, "Guides found (total: %zu).\n", seqs.size());
            // the guide's own locus is a hit only if the search allows its PAM
            const bool canonical = (ep.pam[0] == 'G' || ep.pam[0] == 'g') && (ep.pam[1] == 'G' || ep.pam[1] == 'g' || ep.pam[1] == 'A' || ep.pam[1] == 'a');
            if (!canonical && !p.has_extra_pam) {
                p.has_extra_pam = 1;
                p.extra_pam[0] = ep.pam[0];
                p.extra_pam[1] = ep.pam[1];
                std::fprintf(stderr, "%s: searching with -P %c%c, the guide PAM of -p\n", argv[0], ep.pam[0], ep.pam[1]);
            }
        }
        std::vector<vsc_guide_summary> sum(codes.size()), sum_in(annotated || individual ? codes.size() : 0);
        std::vector<vsc_guide_summary> win_all(individual ? codes.size() : 0), win_var(win_all.size());
        std::vector<uint64_t> win_dups(win_all.size());
        const vsc_locus *ex = loci.empty() ? nullptr : loci.data();
        const uint32_t n_codes = (uint32_t)codes.size();
        // -F / -C: the forest over the feature matrix's columns, one activity per guide
        vsc_forest::Forest forest;
        vsc_rf_model model{};
        std::vector<double> activity(classified ? codes.size() : 0);
        std::vector<vsc_guide_votes> votes_rows(classified ? codes.size() : 0);
        vsc_classify cls{};
        if (classified) {
            forest = vsc_forest::load_forest(opts[22].value);
            vsc_forest::bind_features(forest, [](const std::string &) { return true; });
            model = vsc_forest::model_of(forest);
            const auto table = vsc_merge::read_tuscan(opts[23].value);
            for (size_t i = 0; i < ids.size(); ++i) {
                auto it = table.find(ids[i]);
                if (it == table.end()) throw std::runtime_error("-C: no on-target activity for guide '" + ids[i] + "'");
                activity[i] = it->second;
            }
            cls.model = &model;
            cls.guide_activity = activity.data();
        }
        // -W: the table's entries; the diagonal is 1, every other entry has to be in the file
        std::vector<vsc_guide_table_row> table_rows(tabled ? codes.size() : 0);
        bool table_done = false;
        if (tabled) {
            std::ifstream in(opts[32].value);
            if (!in) throw std::runtime_error("Could not open the -W file.");
            std::vector<double> pair(20 * 4 * 4, std::nan("")), pamw(16, std::nan(""));  // (NaN: not given yet)
            for (int j = 0; j < 20; ++j)
                for (int b = 0; b < 4; ++b) pair[(j * 4 + b) * 4 + b] = 1.0;
            auto base = [](const std::string &t, size_t at) {
                static const std::string letters = "ACGT";
                const char c = at < t.size() ? (char)std::toupper((unsigned char)t[at]) : '?';
                return (int)letters.find(c == 'U' ? 'T' : c);  // (-1: no base)
            };
            std::string line;
            while (std::getline(in, line)) {
                line = line.substr(0, line.find('#'));
                std::istringstream is(line);
                std::string a, b, c, rest;
                double w = 0;
                if (!(is >> a)) continue;
                const std::string bad = "-W: neither 'j g s w' nor 'PAM XY w': '" + line + "'";
                if (a == "PAM") {
                    if (!(is >> b >> w) || (is >> rest) || std::isnan(w) || b.size() != 2 || base(b, 0) < 0 || base(b, 1) < 0)
                        throw std::runtime_error(bad);
                    pamw[4 * base(b, 0) + base(b, 1)] = w;
                } else {
                    char *jend = nullptr;
                    const long j = std::strtol(a.c_str(), &jend, 10);
                    if (*jend || j < 0 || j > 19 || !(is >> b >> c >> w) || (is >> rest) || std::isnan(w) || b.size() != 1 || c.size() != 1 ||
                        base(b, 0) < 0 || base(c, 0) < 0)
                        throw std::runtime_error(bad);
                    pair[(j * 4 + base(b, 0)) * 4 + base(c, 0)] = w;
                }
            }
            for (double w : pair)
                if (std::isnan(w)) throw std::runtime_error("-W: the table lacks an entry (240 'j g s w' lines and 16 'PAM XY w' lines make a table)");
            for (double w : pamw)
                if (std::isnan(w)) throw std::runtime_error("-W: the table lacks a PAM entry (16 'PAM XY w' lines)");
            if (vsc_score_table_build(pair.data(), pamw.data(), &table) != VSC_OK)
                throw std::runtime_error("-W: every weight lies in 0 .. 1 and the weight of a base against itself is 1");
            if (site_scored) {  // the same weights as a pattern table of the SpCas9 shape, plus the -w lines
                const vsc_pattern_table_shape spcas9{VSC_READ_LEN, 0, 20, 2, {21, 22, 0, 0}};
                vsc_pattern_table *base = nullptr;
                if (vsc_pattern_table_build(&spcas9, pair.data(), pamw.data(), &base) != VSC_OK) throw std::runtime_error("-W: no pattern table");
                try {
                    bulge_table = read_bulge_table(opts[36].value, "-w", base);
                } catch (...) {
                    vsc_pattern_table_free(base);
                    throw;
                }
                vsc_pattern_table_free(base);
            }
        }
        if (individual) {
            std::vector<const char *> names;
            for (const std::string &n : ix.names) names.push_back(n.c_str());
            char why[512] = "";
            if (vsc_windows_build(opts[26].value.c_str(), vcf_sample, VSC_READ_LEN, 0, ix.hi.data(), ix.lo.data(), ix.nm.data(), ix.contigs.data(),
                                  names.data(), (uint32_t)ix.contigs.size(), &windows, why, sizeof why) != VSC_OK)
                throw std::runtime_error(std::string("-v: ") + (why[0] ? why : "could not build the variant windows"));
            const uint32_t n_win = vsc_windows_count(windows);
            std::fprintf(stderr, "Variant windows built (total: %u).\n", n_win);
            if (vsc_variant_map_build(n_win ? vsc_windows_name(windows, 0, nullptr) : nullptr, n_win ? vsc_windows_name_offsets(windows) : nullptr,
                                      n_win ? vsc_windows_contigs(windows) : nullptr, n_win, ix.contigs.data(), names.data(),
                                      (uint32_t)ix.contigs.size(), &vmap) != VSC_OK ||
                vsc_variant_map_shadow(vmap, &regions) != VSC_OK)
                throw std::runtime_error("-v: could not parse the ids of the variant windows");
            // the reference side: all hits (the columns every run prints) and those a window shadows
            st = vsc_search_summary_regions(ctx, genome, codes.data(), n_codes, &p, ex, regions, sum.data(), sum_in.data());
            if (st != VSC_OK) throw std::runtime_error(vsc_last_error(ctx));
            if (n_win) {  // the window side, on the same device
                st = vsc_genome_load(ctx, vsc_windows_plane(windows, 0), vsc_windows_plane(windows, 1), vsc_windows_plane(windows, 2), 0,
                                     vsc_windows_words(windows), vsc_windows_words(windows), vsc_windows_contigs(windows), n_win, &win_genome);
                if (st == VSC_OK)
                    st = vsc_search_summary_variants(ctx, win_genome, vmap, codes.data(), n_codes, &p, ex, 0, win_all.data(), win_var.data(),
                                                     win_dups.data());
                if (st != VSC_OK) throw std::runtime_error(vsc_last_error(ctx));
            }
        } else if (by_votes) {
            st = vsc_search_select_classified(ctx, genome, codes.data(), n_codes, &p, &vsel, &cls, ex, sum.data(), votes_rows.data(), &hits);
            if (st != VSC_OK) throw std::runtime_error(vsc_last_error(ctx));
        } else if (tabled && listing) {  // the listing by the table score and its rows from one search, the plain rows from a second
            st = vsc_search_select_table(ctx, genome, codes.data(), n_codes, &p, &sel, ex, table, table_rows.data(), &hits);
            if (st == VSC_OK) st = vsc_search_summary(ctx, genome, codes.data(), n_codes, &p, ex, sum.data());
            if (st != VSC_OK) throw std::runtime_error(vsc_last_error(ctx));
            table_done = true;
        } else if (annotated && listing) {  // without -X the listing is not filtered: the rows then come from a second search, a summary call
            const vsc_region_filter *flt = opts[13].set ? &filter : nullptr;
            vsc_guide_summary *rows_in = flt ? sum_in.data() : nullptr;
            st = multi ? vsc_multi_search_select_regions(multi, mgenome, codes.data(), n_codes, &p, &sel, flt, ex, sum.data(), rows_in, &hits)
                       : vsc_search_select_regions(ctx, genome, codes.data(), n_codes, &p, &sel, flt, ex, sum.data(), rows_in, &hits);
            if (st == VSC_OK && !flt)
                st = multi ? vsc_multi_search_summary_regions(multi, mgenome, codes.data(), n_codes, &p, ex, regions, sum.data(), sum_in.data())
                           : vsc_search_summary_regions(ctx, genome, codes.data(), n_codes, &p, ex, regions, sum.data(), sum_in.data());
            if (st != VSC_OK) throw std::runtime_error(multi ? vsc_multi_last_error(multi) : vsc_last_error(ctx));
        } else if (annotated) {
            st = multi ? vsc_multi_search_summary_regions(multi, mgenome, codes.data(), n_codes, &p, ex, regions, sum.data(), sum_in.data())
                       : vsc_search_summary_regions(ctx, genome, codes.data(), n_codes, &p, ex, regions, sum.data(), sum_in.data());
            if (st != VSC_OK) throw std::runtime_error(multi ? vsc_multi_last_error(multi) : vsc_last_error(ctx));
        } else if (listing && multi) {
            st = vsc_multi_search_select(multi, mgenome, codes.data(), (uint32_t)codes.size(), &p, &sel, ex, sum.data(), &hits);
            if (st != VSC_OK) throw std::runtime_error(vsc_multi_last_error(multi));
        } else if (listing) {
            st = vsc_search_select(ctx, genome, codes.data(), (uint32_t)codes.size(), &p, &sel, ex, sum.data(), &hits);
            if (st != VSC_OK) throw std::runtime_error(vsc_last_error(ctx));
        } else if (multi) {
            table_done = tabled && !classified;  // (the plain rows and the table's from one search)
            st = classified ? vsc_multi_search_summary_classified(multi, mgenome, codes.data(), n_codes, &p, ex, &cls, sum.data(), votes_rows.data())
                 : tabled   ? vsc_multi_search_summary_table(multi, mgenome, codes.data(), n_codes, &p, ex, table, sum.data(), table_rows.data())
                            : vsc_multi_search_summary(multi, mgenome, codes.data(), (uint32_t)codes.size(), &p, ex, sum.data());
            if (st != VSC_OK) throw std::runtime_error(vsc_multi_last_error(multi));
        } else {
            table_done = tabled && !classified;
            st = classified ? vsc_search_summary_classified(ctx, genome, codes.data(), n_codes, &p, ex, &cls, sum.data(), votes_rows.data())
                 : tabled   ? vsc_search_summary_table(ctx, genome, codes.data(), n_codes, &p, ex, table, sum.data(), table_rows.data())
                            : vsc_search_summary(ctx, genome, codes.data(), (uint32_t)codes.size(), &p, ex, sum.data());
            if (st != VSC_OK) throw std::runtime_error(vsc_last_error(ctx));
        }
        if (tabled && !table_done) {  // (the calls above take no table: its rows from a search of their own)
            st = multi ? vsc_multi_search_summary_table(multi, mgenome, codes.data(), n_codes, &p, ex, table, nullptr, table_rows.data())
                       : vsc_search_summary_table(ctx, genome, codes.data(), n_codes, &p, ex, table, nullptr, table_rows.data());
            if (st != VSC_OK) throw std::runtime_error(multi ? vsc_multi_last_error(multi) : vsc_last_error(ctx));
        }
        if (classified && !by_votes && (annotated || listing)) {  // (those calls take no forest: the classifier's rows from a search of their own)
            st = multi ? vsc_multi_search_summary_classified(multi, mgenome, codes.data(), n_codes, &p, ex, &cls, nullptr, votes_rows.data())
                       : vsc_search_summary_classified(ctx, genome, codes.data(), n_codes, &p, ex, &cls, nullptr, votes_rows.data());
            if (st != VSC_OK) throw std::runtime_error(multi ? vsc_multi_last_error(multi) : vsc_last_error(ctx));
        }
        if (pick.on) {  // -k: the picks of every target where the candidates lie, then the -L file with pickTarget pickRank
            PickColumns cols;
            cols.mit_rows = sum.data();
            cols.table_rows = table_rows.data();
            cols.eff = eff_linear.data();
            cols.pairs = mh_pairs.data();
            const std::vector<uint64_t> keys = pick_keys(pick, codes.size(), cols);
            const uint32_t n_targets = (uint32_t)target_names.size();
            const vsc_pick_params pp{(uint32_t)VSC_READ_LEN, 17, pick.k, pick.spacing, 0, 0};
            std::vector<uint32_t> picks((size_t)n_targets * pick.k), counts(n_targets);
            if (vsc_guides_pick(ctx, genome, found, targets, pick.by_name ? pick_group.data() : nullptr, nullptr, n_targets, keys.data(), &pp, picks.data(),
                                counts.data(), nullptr, nullptr, nullptr) != VSC_OK)
                throw std::runtime_error(vsc_last_error(ctx));
            const std::vector<std::string> marks = pick_text(pick, codes.size(), target_names, picks, counts);
            std::ofstream out(guides_bed_path);
            if (!out.is_open()) throw std::runtime_error("Could not open the -L path.");
            for (size_t i = 0; i < bed_lines.size(); ++i) out << bed_lines[i] << marks[i] << edit_cols[i] << '\n';
            out.close();
            if (!out) throw std::runtime_error("Could not write the -L file.");
        }
        std::vector<vsc_bulge_summary> bulge_rows(bulged ? codes.size() : 0);
        if (bulged) {
            st = vsc_search_bulges(ctx, genome, codes.data(), n_codes, &p, &bp, opts[31].set || sited ? &bulge_hits : nullptr, bulge_rows.data());
            if (st != VSC_OK) throw std::runtime_error(vsc_last_error(ctx));
        }
        std::vector<vsc_site_summary> site_rows(sited ? codes.size() : 0);
        if (sited) {  // the plain records kept on the device beside the bulged ones, collapsed where they lie
            const vsc_site_params sp{VSC_READ_LEN, VSC_SITE_ANCHOR_END, {0, 0}};
            st = vsc_search(ctx, genome, codes.data(), n_codes, &p, &site_plain);
            if (st == VSC_OK) st = vsc_hits_sites(ctx, site_plain, bulge_hits, n_codes, &sp, &sites, site_rows.data());
            if (st != VSC_OK) throw std::runtime_error(vsc_last_error(ctx));
        }
        std::vector<vsc_guide_table_row> site_table_rows(site_scored ? codes.size() : 0);
        if (site_scored) {  // the sites scored where the collapse left them; -K / -S cut the listing, the rows are over all sites
            const vsc_site_params sp{VSC_READ_LEN, VSC_SITE_ANCHOR_END, {0, 0}};
            const vsc_pattern_select ssel{sel.top_k, sel.min_score, {0, 0}};
            std::string spelled;
            for (uint64_t code : codes)
                for (int j = 0; j < VSC_READ_LEN; ++j) spelled += "ACGT"[(code >> (2 * j)) & 3u];
            st = vsc_sites_table(ctx, genome, sites, &sp, spelled.data(), n_codes, VSC_READ_LEN, bulge_table, &ssel, &scored_sites,
                                 site_table_rows.data());
            if (st != VSC_OK) throw std::runtime_error(vsc_last_error(ctx));
        }
        // the enabled bulge classes in the rows' order (ascending site length) and their column prefixes
        static const char *const kBulgeClass[VSC_BULGE_CLASSES] = {"br2", "br1", "bd1", "bd2"};
        const bool bulge_on[VSC_BULGE_CLASSES] = {bp.rna_max >= 2, bp.rna_max >= 1, bp.dna_max >= 1, bp.dna_max >= 2};

        std::string text = "#guideId\tguideSeq\tmitSpecScore\tofftargetCount\tonTargetFound";
        for (long k = 0; k <= mm; ++k) text += "\tmm" + std::to_string(k);
        text += "\tmitHitSum";
        if (annotated) {
            text += "\tregionMitSpecScore\tregionCount";
            for (long k = 0; k <= mm; ++k) text += "\trmm" + std::to_string(k);
            text += "\tregionMitHitSum";
        }
        if (classified) {
            text += "\trfExpectedActive\trfActive\trfTies";
            for (long k = 0; k <= mm; ++k) text += "\tra" + std::to_string(k);
        }
        if (tabled) text += "\ttableScoreSum\ttableSpecScore\ttablePositive";
        if (individual) {
            text += "\tindMitSpecScore\tindCount";
            for (long k = 0; k <= mm; ++k) text += "\timm" + std::to_string(k);
            text += "\tindMitHitSum\tvarCount";
            for (long k = 0; k <= mm; ++k) text += "\tvmm" + std::to_string(k);
            text += "\tvarMitHitSum\tvarDuplicates";
        }
        if (bulged) {
            text += "\tbulgeCount";
            for (int c = 0; c < VSC_BULGE_CLASSES; ++c)
                for (long k = 0; bulge_on[c] && k <= mm; ++k) text += std::string("\t") + kBulgeClass[c] + "mm" + std::to_string(k);
        }
        if (sited) text += "\tsiteCount\tsiteBulgeOnly";
        if (site_scored) text += "\tsiteScoreSum\tsiteSpecScore\tsitePositive";
        text += '\n';
        char buf[64];
        for (size_t i = 0; i < sum.size(); ++i) {
            const vsc_guide_summary &s = sum[i];
            uint64_t total = 0;
            for (int k = 0; k <= VSC_MAX_MISMATCHES; ++k) total += s.nm[k];
            text += ids[i] + '\t' + dna4(seqs[i]) + '\t';
            std::snprintf(buf, sizeof buf, "%.0f", std::floor(vsc_mit_specificity(s.mit_sum) + 0.5));
            text += std::string(buf) + '\t' + std::to_string(total) + '\t' + std::to_string(s.on_target);
            for (long k = 0; k <= mm; ++k) text += '\t' + std::to_string(s.nm[k]);
            std::snprintf(buf, sizeof buf, "%.6f", (double)s.mit_sum * 0x1p-24);
            text += '\t' + std::string(buf);
            if (annotated) {
                const vsc_guide_summary &r = sum_in[i];
                uint64_t inside = 0;
                for (int k = 0; k <= VSC_MAX_MISMATCHES; ++k) inside += r.nm[k];
                std::snprintf(buf, sizeof buf, "%.0f", std::floor(vsc_mit_specificity(r.mit_sum) + 0.5));
                text += '\t' + std::string(buf) + '\t' + std::to_string(inside);
                for (long k = 0; k <= mm; ++k) text += '\t' + std::to_string(r.nm[k]);
                std::snprintf(buf, sizeof buf, "%.6f", (double)r.mit_sum * 0x1p-24);
                text += '\t' + std::string(buf);
            }
            if (classified) {
                const vsc_guide_votes &v = votes_rows[i];
                std::snprintf(buf, sizeof buf, "%.6f", (double)v.votes_sum / (double)model.n_trees);
                text += '\t' + std::string(buf) + '\t' + std::to_string(v.active) + '\t' + std::to_string(v.ties);
                for (long k = 0; k <= mm; ++k) text += '\t' + std::to_string(v.active_nm[k]);
            }
            if (tabled) {
                const vsc_guide_table_row &r = table_rows[i];
                std::snprintf(buf, sizeof buf, "%.6f", (double)r.score_sum * 0x1p-30);
                text += '\t' + std::string(buf);
                std::snprintf(buf, sizeof buf, "%.0f", std::floor(vsc_table_specificity(r.score_sum) + 0.5));
                text += '\t' + std::string(buf) + '\t' + std::to_string(r.positive);
            }
            if (individual) {  // unshadowed reference hits + counted window hits; then the window hits that cover a variant
                const vsc_guide_summary &in = sum_in[i], &w = win_all[i], &v = win_var[i];
                const uint64_t ind_mit = s.mit_sum - in.mit_sum + w.mit_sum;
                uint64_t ind = 0, var = 0;
                for (int k = 0; k <= VSC_MAX_MISMATCHES; ++k) {
                    ind += s.nm[k] - in.nm[k] + w.nm[k];
                    var += v.nm[k];
                }
                std::snprintf(buf, sizeof buf, "%.0f", std::floor(vsc_mit_specificity(ind_mit) + 0.5));
                text += '\t' + std::string(buf) + '\t' + std::to_string(ind);
                for (long k = 0; k <= mm; ++k) text += '\t' + std::to_string(s.nm[k] - in.nm[k] + w.nm[k]);
                std::snprintf(buf, sizeof buf, "%.6f", (double)ind_mit * 0x1p-24);
                text += '\t' + std::string(buf) + '\t' + std::to_string(var);
                for (long k = 0; k <= mm; ++k) text += '\t' + std::to_string(v.nm[k]);
                std::snprintf(buf, sizeof buf, "%.6f", (double)v.mit_sum * 0x1p-24);
                text += '\t' + std::string(buf) + '\t' + std::to_string(win_dups[i]);
            }
            if (bulged) {
                const vsc_bulge_summary &b = bulge_rows[i];
                uint64_t all = 0;
                for (int c = 0; c < VSC_BULGE_CLASSES; ++c)
                    for (int k = 0; k <= VSC_MAX_MISMATCHES; ++k) all += b.count[c][k];
                text += '\t' + std::to_string(all);
                for (int c = 0; c < VSC_BULGE_CLASSES; ++c)
                    for (long k = 0; bulge_on[c] && k <= mm; ++k) text += '\t' + std::to_string(b.count[c][k]);
            }
            if (sited) text += '\t' + std::to_string(site_rows[i].sites) + '\t' + std::to_string(site_rows[i].bulge_only);
            if (site_scored) {
                const vsc_guide_table_row &r = site_table_rows[i];
                std::snprintf(buf, sizeof buf, "%.6f", (double)r.score_sum * 0x1p-30);
                text += '\t' + std::string(buf);
                std::snprintf(buf, sizeof buf, "%.0f", std::floor(vsc_table_specificity(r.score_sum) + 0.5));
                text += '\t' + std::string(buf) + '\t' + std::to_string(r.positive);
            }
            text += '\n';
        }
        if (opts[5].set) {
            std::ofstream out(out_path);
            if (!out.is_open()) throw std::runtime_error("Could not open output path.");
            out << text;
            out.close();
            if (!out) throw std::runtime_error("Could not write the output.");
        } else {
            std::fwrite(text.data(), 1, text.size(), stdout);
        }
        if (listing) {
            // the selected records (sorted by guide, strand, contig, pos) and their scores, per guide into rank order
            vsc_ctx *hctx = multi ? vsc_multi_result_ctx(multi) : ctx;
            const uint64_t n = vsc_hits_count(hits);
            std::vector<vsc_hit> rec(n);
            std::vector<uint64_t> on(n);
            std::vector<uint32_t> masks(n), score(n);
            std::vector<double> mit(n);
            if (n && vsc_hits_copy(hits, rec.data(), 0) != VSC_OK) throw std::runtime_error(vsc_last_error(hctx));
            for (uint64_t i = 0; i < n; ++i) {
                on[i] = codes[rec[i].guide];
                masks[i] = VSC_HIT_MASK(rec[i].info);
            }
            if (vsc_score_pairs(hctx, on.data(), on.data(), masks.data(), n, mit.data(), nullptr, nullptr) != VSC_OK)
                throw std::runtime_error(vsc_last_error(hctx));
            std::vector<uint64_t> order(n);
            for (uint64_t i = 0; i < n; ++i) {
                score[i] = (uint32_t)std::nearbyint(mit[i] * 0x1p24);
                order[i] = i;
            }
            std::vector<uint16_t> votes(by_votes ? n : 0);  // -r votes: the survivors' votes, from the classifier over the small result
            if (by_votes && n && vsc_score_classify_hits(ctx, genome, hits, codes.data(), n_codes, activity.data(), &model, 0, n, nullptr,
                                                         votes.data(), nullptr) != VSC_OK)
                throw std::runtime_error(vsc_last_error(ctx));
            const bool by_table = tabled;  // (a listing beside -W is one by the table score)
            std::vector<uint32_t> fixed(by_table ? n : 0);  // the survivors' table scores, over the small result
            if (by_table && n && vsc_score_hits_table(ctx, genome, hits, codes.data(), n_codes, 0, n, table, nullptr, fixed.data()) != VSC_OK)
                throw std::runtime_error(vsc_last_error(ctx));
            std::stable_sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) {  // (stable: ties keep the result order)
                if (rec[a].guide != rec[b].guide) return rec[a].guide < rec[b].guide;
                return by_table ? fixed[a] > fixed[b] : by_votes ? votes[a] > votes[b] : score[a] > score[b];
            });
            const bool named = naming && annotated;  // -N: the -A interval each record lies in
            std::vector<uint32_t> in(named ? n : 0);
            if (named && n && (st = vsc_hits_locate(hits, regions, in.data())) != VSC_OK)
                throw std::runtime_error(st == VSC_ERR_RANGE ? "could not name the regions of the hits" : vsc_last_error(hctx));
            std::string list = std::string("#guideId\trank\tchrom\tstart\tend\tstrand\tmismatches\tmismatchPositions\tmitScore\tsequence") +
                               (named ? "\tregion" : "") + (by_table ? "\ttableScore\n" : by_votes ? "\trfVotes\n" : "\n");
            std::string window(VSC_READ_LEN, 'N');
            uint32_t rank = 0;
            for (uint64_t j = 0; j < n; ++j) {
                const vsc_hit &h = rec[order[j]];
                rank = j && rec[order[j - 1]].guide == h.guide ? rank + 1 : 1;
                const std::string &name = ix.names[h.contig];
                std::string positions;
                for (int b = 0; b < VSC_READ_LEN; ++b)
                    if ((VSC_HIT_MASK(h.info) >> b) & 1u) positions += (positions.empty() ? "" : ",") + std::to_string(b);
                vsc_unpack_bases(ix.hi.data(), ix.lo.data(), ix.nm.data(), ix.contigs[h.contig].offset + h.pos, VSC_READ_LEN, &window[0]);
                char tbuf[32] = "";
                if (by_table) std::snprintf(tbuf, sizeof tbuf, "\t%.9f", (double)fixed[order[j]] * 0x1p-30);
                std::snprintf(buf, sizeof buf, "%.6f", (double)score[order[j]] * 0x1p-24);
                list += ids[h.guide] + '\t' + std::to_string(rank) + '\t' + name.substr(0, name.find_first_of(" \t")) + '\t' +
                        std::to_string(h.pos) + '\t' + std::to_string(h.pos + VSC_READ_LEN) + '\t' + (VSC_HIT_STRAND(h.info) ? '-' : '+') + '\t' +
                        std::to_string(VSC_HIT_NM(h.info)) + '\t' + (positions.empty() ? "-" : positions) + '\t' + buf + '\t' + window +
                        (named ? '\t' + (in[order[j]] < region_desc.size() ? region_desc[in[order[j]]] : "-") : "") +
                        (by_table ? std::string(tbuf) : by_votes ? '\t' + std::to_string(votes[order[j]]) : "") + '\n';
            }
            std::ofstream out(hits_path);
            if (!out.is_open()) throw std::runtime_error("Could not open the -T path.");
            out << list;
            out.close();
            if (!out) throw std::runtime_error("Could not write the -T file.");
        }
        if (bulge_hits && opts[31].set) {
            const vsc_bulge_hit *rec = nullptr;
            if (vsc_bulge_hits_data(bulge_hits, &rec) != VSC_OK) throw std::runtime_error(vsc_last_error(ctx));
            const uint64_t n = vsc_bulge_hits_count(bulge_hits);
            std::string list = "#guideId\tchrom\tstart\tend\tstrand\tkind\tsize\tindex\tmismatches\tsequence\n";
            std::string site;
            for (uint64_t j = 0; j < n; ++j) {
                const vsc_bulge_hit &h = rec[j];
                const uint32_t len = (uint32_t)(VSC_READ_LEN + VSC_BULGE_D(h.info));
                const std::string &name = ix.names[h.contig];
                site.assign(len, 'N');
                vsc_unpack_bases(ix.hi.data(), ix.lo.data(), ix.nm.data(), ix.contigs[h.contig].offset + h.pos, len, &site[0]);
                list += ids[h.guide] + '\t' + name.substr(0, name.find_first_of(" \t")) + '\t' + std::to_string(h.pos) + '\t' +
                        std::to_string(h.pos + len) + '\t' + (VSC_BULGE_STRAND(h.info) ? '-' : '+') + '\t' +
                        (VSC_BULGE_KIND(h.info) == VSC_BULGE_RNA ? "RNA" : "DNA") + '\t' + std::to_string(VSC_BULGE_SIZE(h.info)) + '\t' +
                        std::to_string(VSC_BULGE_INDEX(h.info)) + '\t' + std::to_string(VSC_BULGE_NM(h.info)) + '\t' + site + '\n';
            }
            std::ofstream out(bulges_path);
            if (!out.is_open()) throw std::runtime_error("Could not open the -U path.");
            out << list;
            out.close();
            if (!out) throw std::runtime_error("Could not write the -U file.");
        }
        if (sited) {
            const vsc_site *rec = nullptr;
            const vsc_site_score *scores = nullptr;
            vsc_sites *listed = site_scored ? scored_sites : sites;
            if (vsc_sites_data(listed, &rec) != VSC_OK || (site_scored && vsc_sites_scores(listed, &scores) != VSC_OK))
                throw std::runtime_error(vsc_last_error(ctx));
            write_sites(sites_path, "-Z", rec, vsc_sites_count(listed), VSC_READ_LEN, ids, ix, scores);
        }
        if (pairing) {
            // the pairs among the guides' loci, then one search that keeps the records and the join over them on the device
            uint64_t n_found = 0;
            std::vector<vsc_guide_pair> pairs;
            for (int pass = 0; pass < 2; ++pass) {  // count, then fill
                st = discover ? vsc_guides_pairs(found, &pp, pass ? pairs.data() : nullptr, pairs.size(), &n_found)
                              : vsc_loci_pairs(loci.data(), loci.size(), &pp, pass ? pairs.data() : nullptr, pairs.size(), &n_found);
                if (st != VSC_OK) throw std::runtime_error(discover && !multi ? vsc_last_error(ctx) : "could not pair the guides");
                if (n_found > 0xFFFFFFFFull) throw std::runtime_error("-J: too many guide pairs for one join; narrow -j or the targets");
                pairs.resize(n_found);
            }
            std::fprintf(stderr, "Guide pairs found (total: %zu).\n", pairs.size());
            std::vector<vsc_pair_summary> prow(pairs.size());
            if (!pairs.empty()) {
                st = multi ? vsc_multi_search(multi, mgenome, codes.data(), n_codes, &p, &pair_hits) : vsc_search(ctx, genome, codes.data(), n_codes, &p, &pair_hits);
                if (st != VSC_OK) throw std::runtime_error(multi ? vsc_multi_last_error(multi) : vsc_last_error(ctx));
                st = vsc_hits_pairs(pair_hits, n_codes, pairs.data(), (uint32_t)pairs.size(), &pp, ex, prow.data(), nullptr, 0, nullptr);
                if (st != VSC_OK) throw std::runtime_error(vsc_last_error(multi ? vsc_multi_result_ctx(multi) : ctx));
            }
            std::string list = "#pairId\tguideA\tguideB\toffset\tsites\tonTarget\tminNmSum";
            for (long k = 0; k <= 2 * mm; ++k) list += "\tps" + std::to_string(k);
            list += '\n';
            for (size_t j = 0; j < pairs.size(); ++j) {
                const vsc_guide_pair &q = pairs[j];
                const vsc_pair_summary &r = prow[j];
                int min_sum = -1;
                for (int k = 16; k >= 0; --k)
                    if (r.nm_sum[k]) min_sum = k;
                const long long offset = (long long)loci[q.b].pos - (long long)loci[q.a].pos - VSC_READ_LEN;
                list += ids[q.a] + '|' + ids[q.b] + '\t' + ids[q.a] + '\t' + ids[q.b] + '\t' + std::to_string(offset) + '\t' +
                        std::to_string(r.sites) + '\t' + std::to_string(r.on_target) + '\t' + (min_sum < 0 ? "-" : std::to_string(min_sum));
                for (long k = 0; k <= 2 * mm; ++k) list += '\t' + std::to_string(r.nm_sum[k]);
                list += '\n';
            }
            std::ofstream out(pairs_path);
            if (!out.is_open()) throw std::runtime_error("Could not open the -J path.");
            out << list;
            out.close();
            if (!out) throw std::runtime_error("Could not write the -J file.");
        }
        rc = 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "ERROR: %s\n", e.what());
        rc = 1;
    }
    if (hits) vsc_hits_free(hits);
    vsc_score_table_free(table);
    vsc_bulge_table_free(bulge_table);
    vsc_sites_free(scored_sites);
    eff_any_free(eff_model);
    if (pair_hits) vsc_hits_free(pair_hits);
    vsc_bulge_hits_free(bulge_hits);
    vsc_sites_free(sites);
    if (site_plain) vsc_hits_free(site_plain);
    vsc_guides_free(found);
    vsc_regions_free(regions);
    vsc_regions_free(targets);
    if (multi) {
        vsc_multi_genome_free(mgenome);
        vsc_multi_destroy(multi);
    } else {
        if (win_genome) vsc_genome_free(win_genome);
        vsc_genome_free(genome);
        vsc_ctx_destroy(ctx);
    }
    vsc_variant_map_free(vmap);
    if (windows) vsc_windows_free(windows);
    return rc;
}
