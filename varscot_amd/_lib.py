"""ctypes binding of libvarscot_hip.so (include/varscot_hip.h).

The library is the product: there is no Python or CPU implementation of the search behind this
module.  Importing it fails loudly when the shared library has not been built
(`python -c "import __graft_entry__ as g; g.build()"` or `make -C varscot_amd/csrc`).
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VSC_LIB_PATH") or os.path.join(_HERE, "libvarscot_hip.so")  # override for A/B experiments

VSC_OK = 0
VSC_ERR_RANGE = -34
ERRORS = {-22: "VSC_ERR_INVALID", -12: "VSC_ERR_NOMEM", -5: "VSC_ERR_DEVICE", -34: "VSC_ERR_RANGE",
          -19: "VSC_ERR_NODEVICE"}

HIT_DTYPE = np.dtype([("guide", "<u4"), ("contig", "<u4"), ("pos", "<u4"), ("info", "<u4")])
CONTIG_DTYPE = np.dtype([("offset", "<u8"), ("length", "<u4"), ("reserved", "<u4")])
N_FEATURES = 442
# vsc_guide_summary (vsc_search_summary): 96 bytes per guide
SUMMARY_DTYPE = np.dtype([("mit_sum", "<u8"), ("nm", "<u8", (9,)), ("mit_ub", "<u8"), ("on_target", "<u4"),
                          ("reserved", "<u4")])
assert SUMMARY_DTYPE.itemsize == 96
# vsc_guide_votes (vsc_search_summary_classified): 96 bytes per guide
VOTES_DTYPE = np.dtype([("votes_sum", "<u8"), ("active", "<u8"), ("ties", "<u8"), ("active_nm", "<u8", (9,))])
assert VOTES_DTYPE.itemsize == 96
# vsc_guide_table_row (vsc_search_summary_table): 96 bytes per guide
TABLE_ROW_DTYPE = np.dtype([("score_sum", "<u8"), ("positive", "<u8"), ("positive_nm", "<u8", (9,)), ("reserved", "<u8")])
assert TABLE_ROW_DTYPE.itemsize == 96
# vsc_locus: an excluded locus (contig == 0xFFFFFFFF: none)
LOCUS_DTYPE = np.dtype([("contig", "<u4"), ("pos", "<u4"), ("strand", "<u4"), ("reserved", "<u4")])


class SearchParams(C.Structure):
    _fields_ = [("max_mismatches", C.c_uint32), ("has_extra_pam", C.c_uint8), ("extra_pam", C.c_char * 2),
                ("algorithm", C.c_uint8)]


ALGO_AUTO, ALGO_SCAN, ALGO_SEED = 0, 1, 2


class Select(C.Structure):
    """vsc_select: per guide, the top_k hits by rint(MIT * 2^24) among those >= min_score (0 = no limit / no floor)."""
    _fields_ = [("top_k", C.c_uint32), ("min_score", C.c_uint32), ("reserved", C.c_uint32 * 2)]


SELECT = Select
assert C.sizeof(Select) == 16


# vsc_interval: one interval of an annotation (vsc_regions_build), 0-based half-open on the forward genome
INTERVAL_DTYPE = np.dtype([("contig", "<u4"), ("start", "<u4"), ("end", "<u4"), ("reserved", "<u4")])
REGION_OVERLAP, REGION_INSIDE = 0, 1
REGION_KEEP, REGION_DROP = 0, 1
# vsc_variant_label: a window hit in chromosome coordinates (vsc_hits_variants, vsc_variant_map_locate)
VARIANT_LABEL_DTYPE = np.dtype([("contig", "<u4"), ("pos", "<u4"), ("n_var", "<u4"), ("flags", "<u4")])
VARIANT_VAR, VARIANT_DUP, VARIANT_ON_TARGET = 1, 2, 4  # VSC_VARIANT_*
# vsc_pattern_variant_row: a guide's counted pattern hits of one side of the individual's genome (vsc_search_pattern_variants)
PATTERN_VARIANT_ROW_DTYPE = np.dtype([("count", "<u4", (9,)), ("on_target", "<u4"), ("dropped", "<u8")])
assert PATTERN_VARIANT_ROW_DTYPE.itemsize == 48
PATTERN_REF_SHADOWED, PATTERN_REF_ON_TARGET = 1, 2  # VSC_PATTERN_REF_*
REGION_NONE = 0xFFFFFFFF  # VSC_REGION_NONE: the label of a window that is in no interval


class RegionFilter(C.Structure):
    """vsc_region_filter: select among the hits in the regions (scope REGION_KEEP) or among those outside (REGION_DROP)."""
    _fields_ = [("regions", C.c_void_p), ("scope", C.c_uint32), ("reserved", C.c_uint32)]


class EnumParams(C.Structure):
    """vsc_enum_params (vsc_guides_enumerate): the guide's PAM, strands (0 both, 1 '+', 2 '-'), GC bounds and largest T run over
    the 20 protospacer bases (0 = no upper bound / no limit), max_guides (0 = no cap)."""
    _fields_ = [("pam", C.c_char * 2), ("strands", C.c_uint8), ("gc_min", C.c_uint8), ("gc_max", C.c_uint8),
                ("max_t_run", C.c_uint8), ("reserved0", C.c_uint16), ("max_guides", C.c_uint64), ("reserved", C.c_uint32 * 2)]


assert C.sizeof(EnumParams) == 24


class BulgeParams(C.Structure):
    """vsc_bulge_params (vsc_search_bulges): largest DNA / RNA bulge (0..2, not both 0), reads per round (0 = default), max_hits
    (0 = no cap)."""
    _fields_ = [("dna_max", C.c_uint32), ("rna_max", C.c_uint32), ("guide_batch", C.c_uint32), ("reserved", C.c_uint32),
                ("max_hits", C.c_uint64)]


assert C.sizeof(BulgeParams) == 24
# vsc_bulge_hit: pos = start of the site's 23 + d bases; info = strand << 31 | kind << 12 | size << 10 | index << 5 | NM
BULGE_HIT_DTYPE = np.dtype([("guide", "<u4"), ("contig", "<u4"), ("pos", "<u4"), ("info", "<u4")])
BULGE_DNA, BULGE_RNA = 0, 1
BULGE_CLASSES = 4  # rows of vsc_bulge_summary, ascending d: RNA 2, RNA 1, DNA 1, DNA 2


class PatternParams(C.Structure):
    """vsc_pattern_params (vsc_search_pattern): mismatch budget (0..8), guides per round (0 = default), max_hits (0 = no cap)."""
    _fields_ = [("max_mismatches", C.c_uint32), ("guide_batch", C.c_uint32), ("max_hits", C.c_uint64), ("reserved", C.c_uint32 * 2)]


assert C.sizeof(PatternParams) == 24
# vsc_pattern_hit: pos = start of the site's L bases; info = strand << 31 | NM; mask bit i = forward-genome position i mismatches
PATTERN_HIT_DTYPE = np.dtype([("guide", "<u4"), ("contig", "<u4"), ("pos", "<u4"), ("info", "<u4"), ("mask", "<u4")])
assert PATTERN_HIT_DTYPE.itemsize == 20
PATTERN_MIN_LEN, PATTERN_MAX_LEN = 16, 32


class PatternEnumParams(C.Structure):
    """vsc_pattern_enum_params (vsc_guides_enumerate_pattern): the protospacer [ps_start, ps_start + ps_len) in read positions,
    strands (0 both, 1 '+', 2 '-'), GC bounds and largest T run over the protospacer (0 = no upper bound / no limit), the rule
    the targets are applied with (REGION_OVERLAP / REGION_INSIDE), max_guides (0 = no cap)."""
    _fields_ = [("ps_start", C.c_uint8), ("ps_len", C.c_uint8), ("strands", C.c_uint8), ("gc_min", C.c_uint8), ("gc_max", C.c_uint8),
                ("max_t_run", C.c_uint8), ("reserved0", C.c_uint16), ("rule", C.c_uint32), ("reserved1", C.c_uint32),
                ("max_guides", C.c_uint64), ("reserved", C.c_uint32 * 2)]


assert C.sizeof(PatternEnumParams) == 32


class PatternBulgeParams(C.Structure):
    """vsc_pattern_bulge_params (vsc_search_pattern_bulges): mismatch budget (0..8), guides per round (0 = default), max_hits
    (0 = no cap), the protospacer [proto_start, proto_start + proto_len) in read positions, largest DNA / RNA bulge (0..2, not
    both 0)."""
    _fields_ = [("max_mismatches", C.c_uint32), ("guide_batch", C.c_uint32), ("max_hits", C.c_uint64), ("proto_start", C.c_uint32),
                ("proto_len", C.c_uint32), ("dna_max", C.c_uint32), ("rna_max", C.c_uint32)]


assert C.sizeof(PatternBulgeParams) == 32


class SiteParams(C.Structure):
    """vsc_site_params (vsc_hits_sites, vsc_sites_collapse): the plain site length (23, or the pattern's) and the anchor."""
    _fields_ = [("len", C.c_uint32), ("anchor", C.c_uint32), ("reserved", C.c_uint32 * 2)]


assert C.sizeof(SiteParams) == 16
SITE_ANCHOR_END, SITE_ANCHOR_START = 0, 1
SITE_ABSENT = 31  # a members field without a member
# vsc_site: guide, contig, pos, info of the best alignment (info in the vsc_bulge_hit layout; a plain best has size 0); anchor = a;
# members = NM per d in 5-bit fields (d = -2 lowest), the number of members in bits 25..27; best = its index in its input list
SITE_DTYPE = np.dtype([("guide", "<u4"), ("contig", "<u4"), ("pos", "<u4"), ("info", "<u4"), ("anchor", "<u4"), ("members", "<u4"),
                       ("best", "<u4"), ("reserved", "<u4")])
# vsc_site_summary: count[|d|][NM of the best]
SITE_ROW_DTYPE = np.dtype([("sites", "<u4"), ("alignments", "<u4"), ("bulge_only", "<u4"), ("count", "<u4", (3, 9))])
assert SITE_DTYPE.itemsize == 32 and SITE_ROW_DTYPE.itemsize == 120


class PairParams(C.Structure):
    """vsc_pair_params: two windows on opposite strands of one contig are PAIRED iff delta_min <= pos('+') - pos('-') <= delta_max."""
    _fields_ = [("delta_min", C.c_int32), ("delta_max", C.c_int32), ("reserved", C.c_uint32 * 2)]


class GuidePair(C.Structure):
    """vsc_guide_pair: a = the '-' window (vsc_loci_pairs) / first guide, b = the '+' window / second guide."""
    _fields_ = [("a", C.c_uint32), ("b", C.c_uint32)]


class PairSummary(C.Structure):
    """vsc_pair_summary (vsc_hits_pairs): the counted paired sites of one pair, by NM sum and by larger NM."""
    _fields_ = [("sites", C.c_uint64), ("nm_sum", C.c_uint64 * 17), ("nm_max", C.c_uint64 * 9), ("on_target", C.c_uint32),
                ("reserved", C.c_uint32)]


class PairSite(C.Structure):
    """vsc_pair_site: one paired site - the pair, its two records in the result, delta = pos('+') - pos('-')."""
    _fields_ = [("pair", C.c_uint32), ("a_rec", C.c_uint32), ("b_rec", C.c_uint32), ("delta", C.c_int32)]


assert C.sizeof(PairParams) == 16 and C.sizeof(GuidePair) == 8 and C.sizeof(PairSummary) == 224 and C.sizeof(PairSite) == 16
PAIR_SUMMARY_DTYPE = np.dtype([("sites", "<u8"), ("nm_sum", "<u8", (17,)), ("nm_max", "<u8", (9,)), ("on_target", "<u4"),
                               ("reserved", "<u4")])
PAIR_SITE_DTYPE = np.dtype([("pair", "<u4"), ("a_rec", "<u4"), ("b_rec", "<u4"), ("delta", "<i4")])
assert PAIR_SUMMARY_DTYPE.itemsize == 224 and PAIR_SITE_DTYPE.itemsize == 16


class RegionsStats(C.Structure):
    """vsc_regions_stats (vsc_regions_info)."""
    _fields_ = [("intervals", C.c_uint64), ("rule", C.c_uint32), ("block_bases", C.c_uint32), ("blocks_out", C.c_uint64),
                ("blocks_in", C.c_uint64), ("blocks_mixed", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class VariantMapStats(C.Structure):
    """vsc_variant_map_stats (vsc_variant_map_info)."""
    _fields_ = [("windows", C.c_uint64), ("variants", C.c_uint64), ("unknown_chr", C.c_uint64), ("max_variants", C.c_uint32),
                ("reserved", C.c_uint32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "reserved"}


class RfModel(C.Structure):
    _fields_ = [("n_trees", C.c_uint32), ("n_nodes", C.c_uint32), ("node_status", C.c_void_p), ("feature", C.c_void_p),
                ("left", C.c_void_p), ("right", C.c_void_p), ("split", C.c_void_p), ("node_class", C.c_void_p)]


class Timing(C.Structure):
    _fields_ = [("scan_ms", C.c_double), ("prep_ms", C.c_double), ("sort_ms", C.c_double),
                ("finalize_ms", C.c_double), ("score_ms", C.c_double), ("total_ms", C.c_double),
                ("index_ms", C.c_double), ("sites", C.c_uint64), ("pairs", C.c_uint64), ("hits", C.c_uint64),
                ("genome_bytes", C.c_uint64), ("passes", C.c_uint32), ("algorithm", C.c_uint32),
                ("sort_bytes", C.c_uint64), ("sort_levels", C.c_uint32), ("sort_bin_bits", C.c_uint32),
                ("read_passes", C.c_uint32), ("sort_fallbacks", C.c_uint32), ("list_entries", C.c_uint64), ("seed_cut", C.c_uint32),
                ("seed_layout", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class MultiTiming(C.Structure):
    _fields_ = [("search_wall_ms", C.c_double), ("search_ms_max", C.c_double), ("exchange_ms", C.c_double),
                ("merge_ms", C.c_double), ("total_ms", C.c_double), ("hits", C.c_uint64), ("exchanged_bytes", C.c_uint64),
                ("n_devices", C.c_uint32), ("used_rccl", C.c_uint32), ("score_ms_max", C.c_double), ("callback_ms", C.c_double),
                ("batches", C.c_uint32), ("reserved", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class SelectVotes(C.Structure):
    """vsc_select_votes: per guide, the top_k hits by the forest's votes among those >= min_votes (0 = no limit / no floor)."""
    _fields_ = [("top_k", C.c_uint32), ("min_votes", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class Classify(C.Structure):
    """vsc_classify: the forest and the reads' on-target activities of the classified sinks."""
    _fields_ = [("model", C.POINTER(RfModel)), ("guide_activity", C.c_void_p), ("reserved", C.c_uint32 * 2)]


assert C.sizeof(SelectVotes) == 16 and C.sizeof(Classify) == 24


class MultiScore(C.Structure):
    """vsc_multi_score: what every shard computes per hit before the exchange (vsc_multi_search_stream)."""
    _fields_ = [("mode", C.c_uint32), ("reserved", C.c_uint32), ("guide_activity", C.c_void_p), ("model", C.POINTER(RfModel))]


MULTI_SCORE_NONE, MULTI_SCORE_ROWS, MULTI_SCORE_VOTES = 0, 1, 2


class ScoreTableStats(C.Structure):
    """vsc_score_table_stats"""
    _fields_ = [("serial", C.c_uint64), ("zero_weights", C.c_uint32), ("reserved", C.c_uint32)]


class PatternTableShape(C.Structure):
    """vsc_pattern_table_shape: the length, the protospacer [ps_start, ps_start + ps_len) and the read positions of the PAM
    letters that a pattern table looks at."""
    _fields_ = [("len", C.c_uint32), ("ps_start", C.c_uint32), ("ps_len", C.c_uint32), ("n_pam", C.c_uint32), ("pam_pos", C.c_uint32 * 4)]


class PatternTableStats(C.Structure):
    """vsc_pattern_table_stats"""
    _fields_ = [("serial", C.c_uint64), ("zero_weights", C.c_uint32), ("reserved", C.c_uint32), ("shape", PatternTableShape)]


class PatternSelect(C.Structure):
    """vsc_pattern_select (vsc_search_pattern_table): per guide the hits with f >= min_score, of those the top_k (0: all) best"""
    _fields_ = [("top_k", C.c_uint32), ("min_score", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class BulgeTableStats(C.Structure):
    """vsc_bulge_table_stats"""
    _fields_ = [("serial", C.c_uint64), ("zero_weights", C.c_uint32), ("reserved", C.c_uint32), ("shape", PatternTableShape)]


# vsc_site_score (vsc_sites_table): f of the record's best alignment, the largest f among the members, d + 2 of that member
SITE_SCORE_DTYPE = np.dtype([("best", "<u4"), ("top", "<u4"), ("top_d", "<u4"), ("reserved", "<u4")])

assert C.sizeof(PatternTableShape) == 32 and C.sizeof(PatternTableStats) == 48 and C.sizeof(PatternSelect) == 16
assert C.sizeof(BulgeTableStats) == 48 and SITE_SCORE_DTYPE.itemsize == 16

EFF_IDENTITY, EFF_LOGISTIC = 0, 1  # VSC_EFF_*


class EffShape(C.Structure):
    """vsc_eff_shape: the context window of an efficiency model (C = up + site_len + down), its G/C range in context
    coordinates (gc_len 0: no G/C term) and its link."""
    _fields_ = [("up", C.c_uint32), ("site_len", C.c_uint32), ("down", C.c_uint32), ("gc_start", C.c_uint32), ("gc_len", C.c_uint32),
                ("link", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class EffModelStats(C.Structure):
    """vsc_eff_model_stats"""
    _fields_ = [("serial", C.c_uint64), ("shape", EffShape), ("nonzero_weights", C.c_uint32), ("reserved", C.c_uint32)]


class EffStats(C.Structure):
    """vsc_eff_stats: the candidates of a call by class; the five counts add up to n."""
    _fields_ = [("defined", C.c_uint64), ("invalid", C.c_uint64), ("off_contig", C.c_uint64), ("not_resident", C.c_uint64),
                ("has_n", C.c_uint64), ("reserved", C.c_uint64 * 3)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k in ("defined", "invalid", "off_contig", "not_resident", "has_n")}


EFF_NODE_LEAF, EFF_NODE_BASE, EFF_NODE_PAIR, EFF_NODE_SUM = 0, 1, 2, 3  # VSC_EFF_NODE_*
# vsc_eff_sum: a range of the context and the integer weights of its letters and dinucleotides
EFF_SUM_DTYPE = np.dtype([("start", "<u4"), ("len", "<u4"), ("mono", "<i4", (4,)), ("di", "<i4", (16,))])
# vsc_eff_node: one node of a regression tree, its children numbered inside the tree
EFF_NODE_DTYPE = np.dtype([("kind", "<u4"), ("a", "<u4"), ("b", "<u4"), ("mask", "<u4"), ("t", "<i4"), ("left", "<u4"), ("right", "<u4"),
                           ("reserved", "<u4"), ("value", "<f8")])


class EffTreesStats(C.Structure):
    """vsc_eff_trees_stats"""
    _fields_ = [("serial", C.c_uint64), ("shape", EffShape), ("n_sums", C.c_uint32), ("n_trees", C.c_uint32), ("n_nodes", C.c_uint32),
                ("leaves", C.c_uint32), ("base_nodes", C.c_uint32), ("pair_nodes", C.c_uint32), ("sum_nodes", C.c_uint32),
                ("max_depth", C.c_uint32), ("reserved", C.c_uint64 * 2)]


assert EFF_SUM_DTYPE.itemsize == 88 and EFF_NODE_DTYPE.itemsize == 40 and C.sizeof(EffTreesStats) == 88

MH_UNDEFINED = 0xFFFFFFFF  # VSC_MH_UNDEFINED


class MhShape(C.Structure):
    """vsc_mh_shape: the site's length, the cut (the break lies between read positions cut - 1 and cut) and the flank F; the
    context is read positions [cut - F, cut + F)."""
    _fields_ = [("site_len", C.c_uint32), ("cut", C.c_uint32), ("flank", C.c_uint32), ("reserved", C.c_uint32)]


class MhStats(C.Structure):
    """vsc_mh_stats: the candidates of a call by class (the five counts add up to n), the kernel's and the call's time."""
    _fields_ = [("defined", C.c_uint64), ("invalid", C.c_uint64), ("off_contig", C.c_uint64), ("not_resident", C.c_uint64),
                ("has_n", C.c_uint64), ("kernel_ms", C.c_double), ("wall_ms", C.c_double), ("reserved", C.c_uint64)]

    def as_dict(self):
        d = {k: int(getattr(self, k)) for k in ("defined", "invalid", "off_contig", "not_resident", "has_n")}
        d.update(kernel_ms=float(self.kernel_ms), wall_ms=float(self.wall_ms))
        return d


assert C.sizeof(MhShape) == 16 and C.sizeof(MhStats) == 64

FOLD_UNDEFINED = 0xFFFFFFFF  # VSC_FOLD_UNDEFINED: both words of a candidate whose class is not defined
FOLD_NO_LIMIT = 0xFFFFFFFF  # VSC_FOLD_NO_LIMIT
FOLD_WOBBLE = 1  # VSC_FOLD_WOBBLE


class FoldShapeStruct(C.Structure):
    """vsc_fold_shape: the site's length, the spacer inside it, the stem length k, the G/C floor of a k-mer, the shortest loop,
    the seed in spacer positions and the flags (bit 0: G-U wobble pairs count)."""
    _fields_ = [("site_len", C.c_uint32), ("proto_start", C.c_uint32), ("proto_len", C.c_uint32), ("stem", C.c_uint32),
                ("gc_min", C.c_uint32), ("min_loop", C.c_uint32), ("seed_start", C.c_uint32), ("seed_len", C.c_uint32),
                ("flags", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class FoldLimits(C.Structure):
    """vsc_fold_limits: the largest starts, self_longest, scaf_longest and seed_paired a kept candidate may have (0 .. 32, or
    FOLD_NO_LIMIT)."""
    _fields_ = [("max_starts", C.c_uint32), ("max_self_longest", C.c_uint32), ("max_scaf_longest", C.c_uint32),
                ("max_seed_paired", C.c_uint32)]


class FoldStats(MhStats):
    """vsc_fold_stats: the candidates of a call by class (the five counts add up to n), the kernel's and the call's time."""


assert C.sizeof(FoldShapeStruct) == 48 and C.sizeof(FoldLimits) == 16 and C.sizeof(FoldStats) == 64

MOTIF_UNDEFINED = 0xFFFFFFFFFFFFFFFF  # VSC_MOTIF_UNDEFINED: all three words of a candidate whose class is not defined
MOTIF_BOTH_STRANDS = 1  # VSC_MOTIF_BOTH_STRANDS
MOTIF_CUT_ONLY = 1  # VSC_MOTIF_CUT_ONLY


class MotifStruct(C.Structure):
    """vsc_motif: an IUPAC text of len 2 .. 16 letters and the flags (bit 0: its reverse complement counts too)."""
    _fields_ = [("text", C.c_char * 16), ("len", C.c_uint32), ("flags", C.c_uint32)]


class MotifShapeStruct(C.Structure):
    """vsc_motif_shape: the genomic context (up, site_len, down), the spacer and the cut zone in site positions."""
    _fields_ = [("up", C.c_uint32), ("site_len", C.c_uint32), ("down", C.c_uint32), ("proto_start", C.c_uint32),
                ("proto_len", C.c_uint32), ("cut_start", C.c_uint32), ("cut_len", C.c_uint32), ("reserved", C.c_uint32 * 5)]


class MotifLimits(C.Structure):
    """vsc_motif_limits: the motifs (bit masks) a kept candidate may not hold in its construct / in its genomic context, those of
    which it must hold one at the cut, and the flags (bit 0: at the cut and nowhere else in the context)."""
    _fields_ = [("forbid_construct", C.c_uint64), ("forbid_context", C.c_uint64), ("require_cut", C.c_uint64), ("flags", C.c_uint32),
                ("reserved", C.c_uint32)]


class MotifStats(C.Structure):
    """vsc_motif_stats: the candidates of a call by class (the five counts add up to n), those with any construct, any cut and
    any cut-only bit, the kernel's and the call's time."""
    _fields_ = [("defined", C.c_uint64), ("invalid", C.c_uint64), ("off_contig", C.c_uint64), ("not_resident", C.c_uint64),
                ("has_n", C.c_uint64), ("any_construct", C.c_uint64), ("any_cut", C.c_uint64), ("any_cut_only", C.c_uint64),
                ("kernel_ms", C.c_double), ("wall_ms", C.c_double), ("reserved", C.c_uint64 * 2)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


assert C.sizeof(MotifStruct) == 24 and C.sizeof(MotifShapeStruct) == 48 and C.sizeof(MotifLimits) == 32 and C.sizeof(MotifStats) == 96

PICK_NONE = 0xFFFFFFFF  # VSC_PICK_NONE: a picks entry beyond counts[t], the rank of a candidate that is not picked


class PickParams(C.Structure):
    """vsc_pick_params: the sites' length and cut, k picks per target at least `spacing` bases apart, the floor on the key."""
    _fields_ = [("site_len", C.c_uint32), ("cut", C.c_uint32), ("k", C.c_uint32), ("spacing", C.c_uint32), ("min_key", C.c_uint64),
                ("reserved", C.c_uint64)]


class PickStats(C.Structure):
    """vsc_pick_stats: the candidates of a call by class (the five counts add up to n), the targets with a pick, the targets
    that end short of k with eligible candidates left, the picks, and the times."""
    _fields_ = [("eligible", C.c_uint64), ("invalid", C.c_uint64), ("no_target", C.c_uint64), ("bad_target", C.c_uint64),
                ("below_min_key", C.c_uint64), ("targets_picked", C.c_uint64), ("targets_short", C.c_uint64), ("picks", C.c_uint64),
                ("kernel_ms", C.c_double), ("wall_ms", C.c_double), ("stage_ms", C.c_double * 4), ("reserved", C.c_uint64 * 2)]

    def as_dict(self):
        d = {k: int(getattr(self, k)) for k in ("eligible", "invalid", "no_target", "bad_target", "below_min_key", "targets_picked",
                                                "targets_short", "picks")}
        d.update(kernel_ms=float(self.kernel_ms), wall_ms=float(self.wall_ms), stage_ms=[float(x) for x in self.stage_ms])
        return d


assert C.sizeof(PickParams) == 32 and C.sizeof(PickStats) == 128


EDIT_UNDEFINED = 0xFFFFFFFF  # VSC_EDIT_UNDEFINED
EDIT_TARGET_DTYPE = np.dtype([("contig", "<u4"), ("pos", "<u4")])
EDIT_PAIR_DTYPE = np.dtype([("candidate", "<u4"), ("target", "<u4"), ("mask", "<u4"), ("info", "<u4")])


class EditShapeStruct(C.Structure):
    """vsc_edit_shape: the site's length, the window [win_start, win_start + win_len) in read positions and the base (0..3: A C G
    T) the editor converts on the read strand."""
    _fields_ = [("site_len", C.c_uint32), ("win_start", C.c_uint32), ("win_len", C.c_uint32), ("base", C.c_uint32),
                ("reserved", C.c_uint32 * 4)]


class EditStats(C.Structure):
    """vsc_edit_stats: the candidates of a call by class (the five counts add up to n), the candidates with a hit, the pairs,
    the targets with a pair, the rows kernel's and the call's time."""
    _fields_ = [("defined", C.c_uint64), ("invalid", C.c_uint64), ("off_contig", C.c_uint64), ("not_resident", C.c_uint64),
                ("has_n", C.c_uint64), ("with_hit", C.c_uint64), ("pairs", C.c_uint64), ("targets_covered", C.c_uint64),
                ("kernel_ms", C.c_double), ("wall_ms", C.c_double), ("reserved", C.c_uint64 * 2)]

    def as_dict(self):
        d = {k: int(getattr(self, k)) for k in ("defined", "invalid", "off_contig", "not_resident", "has_n", "with_hit", "pairs",
                                                "targets_covered")}
        d.update(kernel_ms=float(self.kernel_ms), wall_ms=float(self.wall_ms))
        return d


assert C.sizeof(EditShapeStruct) == 32 and C.sizeof(EditStats) == 96 and EDIT_PAIR_DTYPE.itemsize == 16 and EDIT_TARGET_DTYPE.itemsize == 8


VARIATION_UNDEFINED = 0xFFFFFFFF  # VSC_VARIATION_UNDEFINED
VARIANT_OTHER = 4  # VSC_VARIANT_OTHER: the alt of a variant that is no SNV
VARIANT_DTYPE = np.dtype([("contig", "<u4"), ("pos", "<u4"), ("span_alt", "<u4"), ("weight", "<u4")])
VARIATION_PAIR_DTYPE = np.dtype([("candidate", "<u4"), ("variant", "<u4"), ("info", "<u4"), ("weight", "<u4")])


class VariationShapeStruct(C.Structure):
    """vsc_variation_shape: the site's length, two bits of zone label and four bits of accepted read bases per read position."""
    _fields_ = [("site_len", C.c_uint32), ("reserved0", C.c_uint32), ("zones", C.c_uint64), ("accept", C.c_uint64 * 2),
                ("reserved", C.c_uint32 * 4)]


class VariationFilterStruct(C.Structure):
    """vsc_variation_filter: the largest cost, the largest count per zone (a byte each, 255: none) and the mask of zones of which
    one must hold a disrupting variant (0: nothing is required)."""
    _fields_ = [("max_cost", C.c_uint32), ("max_by_zone", C.c_uint32), ("require_zones", C.c_uint32), ("reserved", C.c_uint32)]


class VariationStats(C.Structure):
    """vsc_variation_stats: the candidates of a call by class (the five counts add up to n), the candidates with a disrupting
    variant, the pairs, the variants with a pair, the rows kernel's and the call's time."""
    _fields_ = [("defined", C.c_uint64), ("invalid", C.c_uint64), ("off_contig", C.c_uint64), ("not_resident", C.c_uint64),
                ("has_n", C.c_uint64), ("with_disrupting", C.c_uint64), ("pairs", C.c_uint64), ("variants_covered", C.c_uint64),
                ("kernel_ms", C.c_double), ("wall_ms", C.c_double), ("reserved", C.c_uint64 * 2)]

    def as_dict(self):
        d = {k: int(getattr(self, k)) for k in ("defined", "invalid", "off_contig", "not_resident", "has_n", "with_disrupting", "pairs",
                                                "variants_covered")}
        d.update(kernel_ms=float(self.kernel_ms), wall_ms=float(self.wall_ms))
        return d


assert C.sizeof(VariationShapeStruct) == 48 and C.sizeof(VariationFilterStruct) == 16 and C.sizeof(VariationStats) == 96
assert VARIANT_DTYPE.itemsize == 16 and VARIATION_PAIR_DTYPE.itemsize == 16


PRIME_UNDEFINED = 0xFFFFFFFF  # VSC_PRIME_UNDEFINED
PRIME_EDIT_DTYPE = np.dtype([("contig", "<u4"), ("pos", "<u4"), ("del_len", "<u2"), ("ins_len", "<u2"), ("ins", "<u4")])
PRIME_PAIR_DTYPE = np.dtype([("candidate", "<u4"), ("edit", "<u4"), ("info", "<u4"), ("ext", "<u4")])


class PrimeShapeStruct(C.Structure):
    """vsc_prime_shape: the site and its context behind it, the nick, the ranges of the PBS and RTT lengths, the homology behind
    the edit, the PAM and seed ranges in read positions, the flags and the integer stability model of the PBS."""
    _fields_ = [("site_len", C.c_uint32), ("down", C.c_uint32), ("nick", C.c_uint32), ("pbs_min", C.c_uint32), ("pbs_max", C.c_uint32),
                ("rtt_min", C.c_uint32), ("rtt_max", C.c_uint32), ("min_homology", C.c_uint32), ("pam_start", C.c_uint32),
                ("pam_len", C.c_uint32), ("seed_start", C.c_uint32), ("seed_len", C.c_uint32), ("flags", C.c_uint32),
                ("init", C.c_int32), ("mono", C.c_int32 * 4), ("di", C.c_int32 * 16), ("target", C.c_int32),
                ("reserved", C.c_uint32 * 5)]


class PrimeStats(C.Structure):
    """vsc_prime_stats: the candidates of a call by class (the five counts add up to n), the candidates with a pair, the weak
    candidates, the pairs, the pairs by flag (PAM, SEED, POLY_T, WEAK), the edits with a pair, the rows kernel's and the call's time."""
    _fields_ = [("defined", C.c_uint64), ("invalid", C.c_uint64), ("off_contig", C.c_uint64), ("not_resident", C.c_uint64),
                ("has_n", C.c_uint64), ("with_pair", C.c_uint64), ("weak", C.c_uint64), ("pairs", C.c_uint64),
                ("pairs_by_flag", C.c_uint64 * 4), ("edits_covered", C.c_uint64), ("score_ms", C.c_double), ("wall_ms", C.c_double),
                ("reserved", C.c_uint64)]

    def as_dict(self):
        d = {k: int(getattr(self, k)) for k in ("defined", "invalid", "off_contig", "not_resident", "has_n", "with_pair", "weak", "pairs",
                                                "edits_covered")}
        d.update(pairs_by_flag=[int(v) for v in self.pairs_by_flag], score_ms=float(self.score_ms), wall_ms=float(self.wall_ms))
        return d


assert C.sizeof(PrimeShapeStruct) == 160 and C.sizeof(PrimeStats) == 128 and PRIME_PAIR_DTYPE.itemsize == 16 and PRIME_EDIT_DTYPE.itemsize == 16


HDR_UNDEFINED = 0xFFFFFFFF  # VSC_HDR_UNDEFINED
HDR_NO_BLOCK = 0xFFFFFFFF  # VSC_HDR_NO_BLOCK
HDR_PAIR_DTYPE = np.dtype([("candidate", "<u4"), ("edit", "<u4"), ("info", "<u4"), ("block", "<u4")])


class HdrShapeStruct(C.Structure):
    """vsc_hdr_shape: the site with its context on both sides, the break, the reach, the side the PAM fixes, the PAM with the
    letters it accepts, the seed and protospacer ranges with their mismatch thresholds, and the flags."""
    _fields_ = [("up", C.c_uint32), ("site_len", C.c_uint32), ("down", C.c_uint32), ("cut", C.c_uint32), ("max_dist", C.c_uint32),
                ("anchor", C.c_uint32), ("pam_start", C.c_uint32), ("pam_len", C.c_uint32), ("pam_accept", C.c_uint32 * 8),
                ("seed_start", C.c_uint32), ("seed_len", C.c_uint32), ("proto_start", C.c_uint32), ("proto_len", C.c_uint32),
                ("min_seed_mm", C.c_uint32), ("min_proto_mm", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class HdrStats(C.Structure):
    """vsc_hdr_stats: the candidates of a call by class (the five counts add up to n), the candidates with a pair and with a
    usable pair, the pairs, the pairs by flag (B_PAM, B_SEED, B_PROTO, SUB_PAM, SUB_SEED, OPEN), the edits with a usable pair, the
    rows kernel's and the call's time."""
    _fields_ = [("defined", C.c_uint64), ("invalid", C.c_uint64), ("off_contig", C.c_uint64), ("not_resident", C.c_uint64),
                ("has_n", C.c_uint64), ("with_pair", C.c_uint64), ("with_usable", C.c_uint64), ("pairs", C.c_uint64),
                ("pairs_by_flag", C.c_uint64 * 6), ("edits_covered", C.c_uint64), ("score_ms", C.c_double), ("wall_ms", C.c_double),
                ("reserved", C.c_uint64)]

    def as_dict(self):
        d = {k: int(getattr(self, k)) for k in ("defined", "invalid", "off_contig", "not_resident", "has_n", "with_pair", "with_usable",
                                                "pairs", "edits_covered")}
        d.update(pairs_by_flag=[int(v) for v in self.pairs_by_flag], score_ms=float(self.score_ms), wall_ms=float(self.wall_ms))
        return d


assert C.sizeof(HdrShapeStruct) == 96 and C.sizeof(HdrStats) == 144 and HDR_PAIR_DTYPE.itemsize == 16


EFFECTS_UNDEFINED = 0xFFFFFFFF  # VSC_EFFECTS_UNDEFINED
EFFECT_CLASS_NAMES = ("synonymous", "missense", "stop_gained", "stop_lost", "start_lost", "unknown")  # VSC_EFFECT_*
CDS_SEGMENT_DTYPE = np.dtype([("contig", "<u4"), ("start", "<u4"), ("end", "<u4"), ("transcript", "<u4"), ("strand", "<u4"),
                              ("phase", "<u4"), ("reserved", "<u4", (2,))])
EFFECT_DTYPE = np.dtype([("candidate", "<u4"), ("transcript", "<u4"), ("codon", "<u4"), ("info", "<u4")])


class CdsStats(C.Structure):
    """vsc_cds_stats: the segments, n_tx, the transcripts that have a segment and the coding bases of a CDS object."""
    _fields_ = [("segments", C.c_uint64), ("transcripts", C.c_uint64), ("transcripts_used", C.c_uint64), ("coding_bases", C.c_uint64),
                ("reserved", C.c_uint64 * 4)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k in ("segments", "transcripts", "transcripts_used", "coding_bases")}


class EffectsStats(C.Structure):
    """vsc_effects_stats: the candidates of a call by class (the five counts add up to n), the candidates with an effect, the
    effects, the transcripts with a stop_gained effect, the effects by class, the rows kernel's and the call's time."""
    _fields_ = [("defined", C.c_uint64), ("invalid", C.c_uint64), ("off_contig", C.c_uint64), ("not_resident", C.c_uint64),
                ("has_n", C.c_uint64), ("with_effect", C.c_uint64), ("effects", C.c_uint64), ("transcripts_stopped", C.c_uint64),
                ("by_class", C.c_uint64 * 6), ("kernel_ms", C.c_double), ("wall_ms", C.c_double)]

    def as_dict(self):
        d = {k: int(getattr(self, k)) for k in ("defined", "invalid", "off_contig", "not_resident", "has_n", "with_effect", "effects",
                                                "transcripts_stopped")}
        d["by_class"] = {name: int(self.by_class[k]) for k, name in enumerate(EFFECT_CLASS_NAMES)}
        d.update(kernel_ms=float(self.kernel_ms), wall_ms=float(self.wall_ms))
        return d


assert C.sizeof(CdsStats) == 64 and C.sizeof(EffectsStats) == 128 and CDS_SEGMENT_DTYPE.itemsize == 32 and EFFECT_DTYPE.itemsize == 16


KNOCKOUT_UNDEFINED = 0xFFFFFFFF  # VSC_KNOCKOUT_UNDEFINED
KNOCKOUT_END, KNOCKOUT_CAP, KNOCKOUT_UNKNOWN = 0xFFFF, 0xFFFE, 0xFFFD  # d_s of a walk that finds no stop
KNOCKOUT_FLAG_NAMES = ("first", "last", "ptc1", "ptc2", "nmd1", "nmd2", "unknown")  # flag bit k of a row; VSC_KNOCKOUT_FIRST ..


class KnockoutShapeStruct(C.Structure):
    """vsc_knockout_shape"""
    _fields_ = [("site_len", C.c_uint32), ("cut", C.c_uint32), ("nmd_window", C.c_uint32), ("start_window", C.c_uint32),
                ("max_codons", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class KnockoutLimits(C.Structure):
    """vsc_knockout_limits"""
    _fields_ = [("min_frac", C.c_uint32), ("max_frac", C.c_uint32), ("min_edge", C.c_uint32), ("require", C.c_uint32),
                ("forbid", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class KnockoutStats(C.Structure):
    """vsc_knockout_stats: the defined and undefined candidates of a call (they add up to n), the coding cuts, the non-coding
    cuts at a junction, the rows with a PTC and with NMD in frames +1 / +2, the rows with an unknown walk, the candidates the
    occupancy bitmap answered, the drains of the kernel's queue and the entries they held, the transcripts with a candidate
    that has NMD in both frames, the kernel's and the call's time."""
    _fields_ = [("defined", C.c_uint64), ("undefined", C.c_uint64), ("coding", C.c_uint64), ("junction", C.c_uint64),
                ("ptc", C.c_uint64 * 2), ("nmd", C.c_uint64 * 2), ("unknown", C.c_uint64), ("past_find", C.c_uint64),
                ("drains", C.c_uint64), ("drained", C.c_uint64), ("transcripts_covered", C.c_uint64), ("reserved", C.c_uint64),
                ("kernel_ms", C.c_double), ("wall_ms", C.c_double)]

    def as_dict(self):
        d = {k: int(getattr(self, k)) for k in ("defined", "undefined", "coding", "junction", "unknown", "past_find", "drains", "drained",
                                                "transcripts_covered")}
        d.update(ptc=[int(v) for v in self.ptc], nmd=[int(v) for v in self.nmd], kernel_ms=float(self.kernel_ms),
                 wall_ms=float(self.wall_ms))
        return d


assert C.sizeof(KnockoutShapeStruct) == 32 and C.sizeof(KnockoutLimits) == 32 and C.sizeof(KnockoutStats) == 128


class DebugParams(C.Structure):
    """vsc_debug_params (include/varscot_hip_debug.h): test / experiment hooks; 0 or -1 = the library's default."""
    _fields_ = [("seed_groups_per_cu", C.c_uint32), ("seed_reserve", C.c_uint32), ("sort_cap", C.c_uint32),
                ("sort_max_bits", C.c_uint32), ("sort_xcd", C.c_int32), ("sort_debug", C.c_uint32),
                ("sort_optimistic", C.c_int32), ("sort_slot_cap", C.c_uint32), ("score_chunk", C.c_uint64),
                ("score_slices", C.c_int32), ("score_slice_shift", C.c_uint32), ("seed_shared", C.c_int32),
                ("seed_group_out", C.c_int32), ("seed_tight", C.c_int32), ("rf_form", C.c_int32),
                ("seed_parts", C.c_uint32)]
    SIGNED_DEFAULT = ("sort_xcd", "sort_optimistic", "score_slices", "seed_shared", "seed_group_out", "seed_tight", "rf_form")

    @classmethod
    def defaults(cls):
        d = cls()
        for k in cls.SIGNED_DEFAULT:
            setattr(d, k, -1)
        return d


class MultiDebugParams(C.Structure):
    _fields_ = [("rccl", C.c_int32), ("rccl_library", C.c_char_p)]


# vsc_debug_sort_segment / _input / _info (include/varscot_hip_debug.h): the bin sort on the caller's records
SORT_SEGMENT_DTYPE = np.dtype([("first_slot", "<u8"), ("n_slots", "<u4"), ("guide_base", "<u4")])


class DebugSortInput(C.Structure):
    _fields_ = [("pos_bits", C.c_uint32), ("pos_base", C.c_uint32), ("read_bits", C.c_uint32), ("slots", C.c_void_p),
                ("n_slots", C.c_uint64), ("segments", C.c_void_p), ("n_segments", C.c_uint32), ("fill_shift", C.c_uint32),
                ("fill", C.c_void_p), ("pair_keys", C.c_void_p), ("pair_vals", C.c_void_p), ("n_pairs", C.c_uint64),
                ("n_regions", C.c_uint32), ("guide_base", C.c_uint32), ("slots_allowed", C.c_int32), ("reserved", C.c_uint32)]


class DebugSortInfo(C.Structure):
    _fields_ = [("n", C.c_uint64), ("bytes", C.c_uint64), ("levels", C.c_uint32), ("bin_bits", C.c_uint32),
                ("slot_fallbacks", C.c_uint32), ("slots_allowed", C.c_uint32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


assert SORT_SEGMENT_DTYPE.itemsize == 16 and C.sizeof(DebugSortInput) == 96 and C.sizeof(DebugSortInfo) == 32


BATCH_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32)  # vsc_batch_fn
ROWS_BATCH_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p)  # vsc_rows_batch_fn
MULTI_BATCH_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p)  # vsc_multi_batch_fn

# every symbol include/varscot_hip.h declares: (name, restype, argtypes)
_u32p = C.POINTER(C.c_uint32)
_vp = C.c_void_p
SYMBOLS = [
    ("vsc_abi_version", C.c_int, []),
    ("vsc_device_count", C.c_int, []),
    ("vsc_ctx_create", C.c_int, [C.c_int, C.POINTER(_vp)]),
    ("vsc_ctx_destroy", C.c_int, [_vp]),
    ("vsc_ctx_release_scratch", C.c_int, [_vp]),
    ("vsc_ctx_set_stream", C.c_int, [_vp, _vp]),
    ("vsc_last_error", C.c_char_p, [_vp]),
    ("vsc_ctx_timing", C.c_int, [_vp, C.POINTER(Timing)]),
    ("vsc_layout_contigs", C.c_uint64, [_vp, C.c_uint32, _vp]),
    ("vsc_planes_init", None, [_vp, _vp, _vp, C.c_uint64]),
    ("vsc_pack_bases", None, [C.c_char_p, C.c_uint64, C.c_uint64, _vp, _vp, _vp]),
    ("vsc_unpack_bases", None, [_vp, _vp, _vp, C.c_uint64, C.c_uint64, _vp]),
    ("vsc_pack_guide", C.c_uint64, [C.c_char_p]),
    ("vsc_genome_load", C.c_int, [_vp, _vp, _vp, _vp, C.c_uint64, C.c_uint64, C.c_uint64, _vp, C.c_uint32,
                                  C.POINTER(_vp)]),
    ("vsc_genome_free", C.c_int, [_vp]),
    ("vsc_genome_build_index", C.c_int, [_vp, _vp, C.POINTER(SearchParams)]),
    ("vsc_genome_index_save", C.c_int, [_vp, _vp, C.c_char_p]),
    ("vsc_genome_index_load", C.c_int, [_vp, _vp, C.c_char_p]),
    ("vsc_genome_device_bytes", C.c_uint64, [_vp]),
    ("vsc_search", C.c_int, [_vp, _vp, _vp, C.c_uint32, C.POINTER(SearchParams), C.POINTER(_vp)]),
    ("vsc_search_stream", C.c_int, [_vp, _vp, _vp, C.c_uint32, C.POINTER(SearchParams), C.c_uint32, BATCH_FN, _vp]),
    ("vsc_search_stream_rows", C.c_int, [_vp, _vp, _vp, C.c_uint32, C.POINTER(SearchParams), C.c_uint32, ROWS_BATCH_FN, _vp]),
    ("vsc_search_summary", C.c_int, [_vp, _vp, _vp, C.c_uint32, C.POINTER(SearchParams), _vp, _vp]),
    ("vsc_search_select", C.c_int, [_vp, _vp, _vp, C.c_uint32, C.POINTER(SearchParams), C.POINTER(Select), _vp, _vp, C.POINTER(_vp)]),
    ("vsc_regions_build", C.c_int, [_vp, C.c_uint32, _vp, C.c_uint64, C.c_uint32, C.POINTER(_vp)]),
    ("vsc_regions_free", None, [_vp]),
    ("vsc_regions_contains", C.c_int, [_vp, C.c_uint32, C.c_uint32]),
    ("vsc_regions_info", C.c_int, [_vp, C.POINTER(RegionsStats)]),
    ("vsc_search_summary_regions", C.c_int, [_vp, _vp, _vp, C.c_uint32, C.POINTER(SearchParams), _vp, _vp, _vp, _vp]),
    ("vsc_search_select_regions", C.c_int, [_vp, _vp, _vp, C.c_uint32, C.POINTER(SearchParams), C.POINTER(Select), C.POINTER(RegionFilter),
                                            _vp, _vp, _vp, C.POINTER(_vp)]),
    ("vsc_guides_enumerate", C.c_int, [_vp, _vp, _vp, C.POINTER(EnumParams), C.POINTER(_vp)]),
    ("vsc_guides_count", C.c_uint64, [_vp]),
    ("vsc_guides_data", C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_vp)]),
    ("vsc_guides_data_dev", C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_vp)]),
    ("vsc_guides_free", C.c_int, [_vp]),
    ("vsc_regions_locate", C.c_uint32, [_vp, C.c_uint32, C.c_uint32]),
    ("vsc_hits_locate", C.c_int, [_vp, _vp, _vp]),
    ("vsc_guides_locate", C.c_int, [_vp, _vp, _vp]),
    ("vsc_search_bulges", C.c_int, [_vp, _vp, _vp, C.c_uint32, C.POINTER(SearchParams), C.POINTER(BulgeParams), C.POINTER(_vp), _vp]),
    ("vsc_bulge_hits_count", C.c_uint64, [_vp]),
    ("vsc_bulge_hits_data", C.c_int, [_vp, C.POINTER(_vp)]),
    ("vsc_bulge_hits_data_dev", _vp, [_vp]),
    ("vsc_bulge_hits_free", C.c_int, [_vp]),
    ("vsc_bulge_align", C.c_int, [C.c_uint64, C.c_char_p, C.c_int, _u32p, _u32p]),
    ("vsc_search_pattern", C.c_int, [_vp, _vp, C.c_char_p, C.c_char_p, C.c_uint32, C.c_uint32, C.POINTER(PatternParams), C.POINTER(_vp), _vp]),
    ("vsc_pattern_hits_count", C.c_uint64, [_vp]),
    ("vsc_pattern_hits_data", C.c_int, [_vp, C.POINTER(_vp)]),
    ("vsc_pattern_hits_data_dev", _vp, [_vp]),
    ("vsc_pattern_hits_free", C.c_int, [_vp]),
    ("vsc_pattern_match", C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint32, _u32p, _u32p, _u32p]),
    ("vsc_search_pattern_bulges", C.c_int, [_vp, _vp, C.c_char_p, C.c_char_p, C.c_uint32, C.c_uint32, C.POINTER(PatternBulgeParams), C.POINTER(_vp), _vp]),
    ("vsc_pattern_bulge_align", C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, _u32p, _u32p, _u32p]),
    ("vsc_hits_sites", C.c_int, [_vp, _vp, _vp, C.c_uint32, C.POINTER(SiteParams), C.POINTER(_vp), _vp]),
    ("vsc_pattern_hits_sites", C.c_int, [_vp, _vp, _vp, C.c_uint32, C.POINTER(SiteParams), C.POINTER(_vp), _vp]),
    ("vsc_sites_count", C.c_uint64, [_vp]),
    ("vsc_sites_data", C.c_int, [_vp, C.POINTER(_vp)]),
    ("vsc_sites_data_dev", _vp, [_vp]),
    ("vsc_sites_free", C.c_int, [_vp]),
    ("vsc_sites_collapse", C.c_int, [_vp, C.c_uint64, _vp, C.c_uint64, C.c_uint32, C.POINTER(SiteParams), _vp, C.c_uint64,
                                     C.POINTER(C.c_uint64), _vp]),
    ("vsc_sites_collapse_pattern", C.c_int, [_vp, C.c_uint64, _vp, C.c_uint64, C.c_uint32, C.POINTER(SiteParams), _vp, C.c_uint64,
                                             C.POINTER(C.c_uint64), _vp]),
    ("vsc_guides_enumerate_pattern", C.c_int, [_vp, _vp, C.c_char_p, C.c_uint32, C.POINTER(PatternEnumParams), _vp, C.c_uint64, C.POINTER(_vp)]),
    ("vsc_pattern_guides_count", C.c_uint64, [_vp]),
    ("vsc_pattern_guides_data", C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_vp)]),
    ("vsc_pattern_guides_data_dev", C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_vp)]),
    ("vsc_pattern_guides_free", C.c_int, [_vp]),
    ("vsc_pattern_guide_text", C.c_int, [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_char_p]),
    ("vsc_loci_pairs", C.c_int, [_vp, C.c_uint64, C.POINTER(PairParams), _vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    ("vsc_guides_pairs", C.c_int, [_vp, C.POINTER(PairParams), _vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    ("vsc_hits_pairs", C.c_int, [_vp, C.c_uint32, _vp, C.c_uint32, C.POINTER(PairParams), _vp, _vp, _vp, C.c_uint64,
                                 C.POINTER(C.c_uint64)]),
    ("vsc_mit_specificity", C.c_double, [C.c_uint64]),
    ("vsc_hits_count", C.c_uint64, [_vp]),
    ("vsc_hits_data_dev", _vp, [_vp]),
    ("vsc_hits_data", C.c_int, [_vp, C.POINTER(_vp)]),
    ("vsc_hits_copy", C.c_int, [_vp, _vp, C.c_int]),
    ("vsc_hits_merge", C.c_int, [_vp, _vp, C.c_int, _vp, C.c_uint32, C.c_uint32, C.POINTER(_vp)]),
    ("vsc_hits_pack_exchange", C.c_int, [_vp, _vp, _vp, C.c_uint32, _vp, C.c_int, _vp]),
    ("vsc_hits_merge_packed", C.c_int, [_vp, _vp, _vp, C.c_int, _vp, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(_vp)]),
    ("vsc_hits_merge_packed_votes", C.c_int, [_vp, _vp, _vp, _vp, C.c_int, _vp, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(_vp), _vp, C.c_int]),
    ("vsc_hits_free", C.c_int, [_vp]),
    ("vsc_score_hits", C.c_int, [_vp, _vp, _vp, _vp, C.c_uint32, C.c_uint64, C.c_uint64, _vp, _vp, _vp]),
    ("vsc_score_hits_packed", C.c_int, [_vp, _vp, _vp, _vp, C.c_uint32, C.c_uint64, C.c_uint64, _vp, _vp, _vp]),
    ("vsc_unpack_features", None, [_vp, C.c_uint64, _vp]),
    ("vsc_score_pairs", C.c_int, [_vp, _vp, _vp, _vp, C.c_uint64, _vp, _vp, _vp]),
    ("vsc_multi_create", C.c_int, [C.POINTER(C.c_int), C.c_int, C.POINTER(_vp)]),
    ("vsc_multi_destroy", C.c_int, [_vp]),
    ("vsc_multi_release_scratch", C.c_int, [_vp]),
    ("vsc_multi_size", C.c_int, [_vp]),
    ("vsc_multi_ctx", _vp, [_vp, C.c_int]),
    ("vsc_multi_result_ctx", _vp, [_vp]),
    ("vsc_multi_last_error", C.c_char_p, [_vp]),
    ("vsc_multi_uses_rccl", C.c_int, [_vp]),
    ("vsc_multi_get_timing", C.c_int, [_vp, C.POINTER(MultiTiming)]),
    ("vsc_multi_genome_load", C.c_int, [_vp, _vp, _vp, _vp, C.c_uint64, _vp, C.c_uint32, C.POINTER(_vp)]),
    ("vsc_multi_genome_free", C.c_int, [_vp]),
    ("vsc_multi_genome_build_index", C.c_int, [_vp, _vp, C.POINTER(SearchParams)]),
    ("vsc_multi_search", C.c_int, [_vp, _vp, _vp, C.c_uint32, C.POINTER(SearchParams), C.POINTER(_vp)]),
    ("vsc_multi_search_summary", C.c_int, [_vp, _vp, _vp, C.c_uint32, C.POINTER(SearchParams), _vp, _vp]),
    ("vsc_multi_search_select", C.c_int, [_vp, _vp, _vp, C.c_uint32, C.POINTER(SearchParams), C.POINTER(Select), _vp, _vp, C.POINTER(_vp)]),
    ("vsc_multi_search_summary_regions", C.c_int, [_vp, _vp, _vp, C.c_uint32, C.POINTER(SearchParams), _vp, _vp, _vp, _vp]),
    ("vsc_multi_search_select_regions", C.c_int, [_vp, _vp, _vp, C.c_uint32, C.POINTER(SearchParams), C.POINTER(Select),
                                                  C.POINTER(RegionFilter), _vp, _vp, _vp, C.POINTER(_vp)]),
    ("vsc_multi_guides_enumerate", C.c_int, [_vp, _vp, _vp, C.POINTER(EnumParams), C.POINTER(_vp)]),
    ("vsc_multi_search_stream", C.c_int, [_vp, _vp, _vp, C.c_uint32, C.POINTER(SearchParams), C.c_uint32, C.POINTER(MultiScore), MULTI_BATCH_FN, _vp]),
    ("vsc_windows_build", C.c_int, [C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, _vp, _vp, _vp, _vp, _vp, C.c_uint32,
                                    C.POINTER(_vp), C.c_char_p, C.c_size_t]),
    ("vsc_windows_count", C.c_uint32, [_vp]),
    ("vsc_windows_words", C.c_uint64, [_vp]),
    ("vsc_windows_plane", _vp, [_vp, C.c_int]),
    ("vsc_windows_contigs", _vp, [_vp]),
    ("vsc_windows_name", _vp, [_vp, C.c_uint32, C.POINTER(C.c_uint32)]),
    ("vsc_windows_name_offsets", _vp, [_vp]),
    ("vsc_windows_free", None, [_vp]),
    ("vsc_variant_map_build", C.c_int, [_vp, _vp, _vp, C.c_uint32, _vp, _vp, C.c_uint32, C.POINTER(_vp)]),
    ("vsc_variant_map_free", None, [_vp]),
    ("vsc_variant_map_info", C.c_int, [_vp, C.POINTER(VariantMapStats)]),
    ("vsc_variant_map_shadow", C.c_int, [_vp, C.POINTER(_vp)]),
    ("vsc_variant_map_locate", C.c_int, [_vp, C.c_uint32, C.c_uint32, _vp]),
    ("vsc_variant_map_tag", C.c_int64, [_vp, C.c_uint32, C.c_uint32, _vp, C.c_size_t]),
    ("vsc_hits_variants", C.c_int, [_vp, _vp, _vp, _vp, C.c_uint32, _vp]),
    ("vsc_search_summary_variants", C.c_int, [_vp, _vp, _vp, _vp, C.c_uint32, C.POINTER(SearchParams), _vp, C.c_uint32, _vp, _vp, _vp]),
    ("vsc_variant_map_locate_len", C.c_int, [_vp, C.c_uint32, C.c_uint32, C.c_uint32, _vp]),
    ("vsc_variant_map_tag_len", C.c_int64, [_vp, C.c_uint32, C.c_uint32, C.c_uint32, _vp, C.c_size_t]),
    ("vsc_variant_map_shadows", C.c_int, [_vp, C.c_uint32, C.c_uint32, C.c_uint32]),
    ("vsc_pattern_hits_variants", C.c_int, [_vp, _vp, _vp, _vp, C.c_uint32, _vp]),
    ("vsc_pattern_hits_shadowed", C.c_int, [_vp, _vp, _vp, _vp, C.c_uint32, _vp]),
    ("vsc_search_pattern_variants", C.c_int, [_vp, _vp, _vp, _vp, C.c_char_p, C.c_char_p, C.c_uint32, C.c_uint32, C.POINTER(PatternParams), _vp,
                                              _vp, C.c_uint32, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("vsc_rf_predict", C.c_int, [_vp, C.POINTER(RfModel), _vp, _vp, C.c_uint64, _vp, _vp, _vp]),
    ("vsc_rf_predict_packed", C.c_int, [_vp, C.POINTER(RfModel), _vp, C.c_int, _vp, C.c_uint64, _vp, _vp, _vp]),
    ("vsc_score_classify_hits", C.c_int, [_vp, _vp, _vp, _vp, C.c_uint32, _vp, C.POINTER(RfModel), C.c_uint64, C.c_uint64, _vp, _vp, _vp]),
    ("vsc_search_summary_classified", C.c_int, [_vp, _vp, _vp, C.c_uint32, C.POINTER(SearchParams), _vp, C.POINTER(Classify), _vp, _vp]),
    ("vsc_search_select_classified", C.c_int, [_vp, _vp, _vp, C.c_uint32, C.POINTER(SearchParams), C.POINTER(SelectVotes),
                                               C.POINTER(Classify), _vp, _vp, _vp, C.POINTER(_vp)]),
    ("vsc_multi_search_summary_classified", C.c_int, [_vp, _vp, _vp, C.c_uint32, C.POINTER(SearchParams), _vp, C.POINTER(Classify), _vp, _vp]),
    ("vsc_score_table_build", C.c_int, [_vp, _vp, C.POINTER(_vp)]),
    ("vsc_score_table_free", C.c_int, [_vp]),
    ("vsc_score_table_info", C.c_int, [_vp, C.POINTER(ScoreTableStats)]),
    ("vsc_table_score", C.c_int, [_vp, C.c_uint64, C.c_uint64, C.POINTER(C.c_double), C.POINTER(C.c_uint32)]),
    ("vsc_table_specificity", C.c_double, [C.c_uint64]),
    ("vsc_score_hits_table", C.c_int, [_vp, _vp, _vp, _vp, C.c_uint32, C.c_uint64, C.c_uint64, _vp, _vp, _vp]),
    ("vsc_search_summary_table", C.c_int, [_vp, _vp, _vp, C.c_uint32, C.POINTER(SearchParams), _vp, _vp, _vp, _vp]),
    ("vsc_search_select_table", C.c_int, [_vp, _vp, _vp, C.c_uint32, C.POINTER(SearchParams), C.POINTER(Select), _vp, _vp, _vp,
                                          C.POINTER(_vp)]),
    ("vsc_pattern_table_build", C.c_int, [C.POINTER(PatternTableShape), _vp, _vp, C.POINTER(_vp)]),
    ("vsc_pattern_table_free", C.c_int, [_vp]),
    ("vsc_pattern_table_info", C.c_int, [_vp, C.POINTER(PatternTableStats)]),
    ("vsc_pattern_table_score", C.c_int, [_vp, C.c_char_p, C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_uint32)]),
    ("vsc_search_pattern_table", C.c_int, [_vp, _vp, C.c_char_p, C.c_char_p, C.c_uint32, C.c_uint32, C.POINTER(PatternParams), _vp,
                                           C.POINTER(PatternSelect), C.POINTER(_vp), _vp, _vp]),
    ("vsc_pattern_hits_scores", C.c_int, [_vp, C.POINTER(_vp)]),
    ("vsc_pattern_hits_scores_dev", _vp, [_vp]),
    ("vsc_multi_search_summary_table", C.c_int, [_vp, _vp, _vp, C.c_uint32, C.POINTER(SearchParams), _vp, _vp, _vp, _vp]),
    ("vsc_bulge_table_build", C.c_int, [_vp, _vp, _vp, C.POINTER(_vp)]),
    ("vsc_bulge_table_free", C.c_int, [_vp]),
    ("vsc_bulge_table_info", C.c_int, [_vp, C.POINTER(BulgeTableStats)]),
    ("vsc_bulge_table_score", C.c_int, [_vp, C.c_char_p, C.c_char_p, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                        C.POINTER(C.c_double), C.POINTER(C.c_uint32)]),
    ("vsc_bulge_hits_table", C.c_int, [_vp, _vp, _vp, C.c_char_p, C.c_uint32, C.c_uint32, _vp, _vp, _vp]),
    ("vsc_sites_table", C.c_int, [_vp, _vp, _vp, C.POINTER(SiteParams), C.c_char_p, C.c_uint32, C.c_uint32, _vp, C.POINTER(PatternSelect),
                                  C.POINTER(_vp), _vp]),
    ("vsc_sites_scores", C.c_int, [_vp, C.POINTER(_vp)]),
    ("vsc_sites_scores_dev", _vp, [_vp]),
    ("vsc_eff_model_build", C.c_int, [C.POINTER(EffShape), C.c_double, _vp, _vp, _vp, C.POINTER(_vp)]),
    ("vsc_eff_model_free", C.c_int, [_vp]),
    ("vsc_eff_model_info", C.c_int, [_vp, C.POINTER(EffModelStats)]),
    ("vsc_eff_score_text", C.c_int, [_vp, C.c_char_p, C.POINTER(C.c_double)]),
    ("vsc_eff_link", C.c_double, [_vp, C.c_double]),
    ("vsc_loci_efficiency", C.c_int, [_vp, _vp, _vp, C.c_uint64, _vp, _vp, C.POINTER(EffStats)]),
    ("vsc_guides_efficiency", C.c_int, [_vp, _vp, _vp, _vp, _vp, C.POINTER(EffStats)]),
    ("vsc_pattern_guides_efficiency", C.c_int, [_vp, _vp, _vp, _vp, _vp, C.POINTER(EffStats)]),
    ("vsc_guides_filter_efficiency", C.c_int, [_vp, _vp, _vp, _vp, C.c_double, C.POINTER(_vp)]),
    ("vsc_pattern_guides_filter_efficiency", C.c_int, [_vp, _vp, _vp, _vp, C.c_double, C.POINTER(_vp)]),
    ("vsc_eff_trees_build", C.c_int, [C.POINTER(EffShape), C.c_double, _vp, C.c_uint32, _vp, _vp, C.c_uint32, C.POINTER(_vp)]),
    ("vsc_eff_trees_free", C.c_int, [_vp]),
    ("vsc_eff_trees_info", C.c_int, [_vp, C.POINTER(EffTreesStats)]),
    ("vsc_eff_trees_score_text", C.c_int, [_vp, C.c_char_p, C.POINTER(C.c_double)]),
    ("vsc_eff_trees_link", C.c_double, [_vp, C.c_double]),
    ("vsc_loci_efficiency_trees", C.c_int, [_vp, _vp, _vp, C.c_uint64, _vp, _vp, C.POINTER(EffStats)]),
    ("vsc_guides_efficiency_trees", C.c_int, [_vp, _vp, _vp, _vp, _vp, C.POINTER(EffStats)]),
    ("vsc_pattern_guides_efficiency_trees", C.c_int, [_vp, _vp, _vp, _vp, _vp, C.POINTER(EffStats)]),
    ("vsc_guides_filter_efficiency_trees", C.c_int, [_vp, _vp, _vp, _vp, C.c_double, C.POINTER(_vp)]),
    ("vsc_pattern_guides_filter_efficiency_trees", C.c_int, [_vp, _vp, _vp, _vp, C.c_double, C.POINTER(_vp)]),
    ("vsc_mh_score_text", C.c_int, [C.c_char_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    ("vsc_mh_scores", C.c_int, [C.c_uint32, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    ("vsc_loci_microhomology", C.c_int, [_vp, _vp, _vp, C.c_uint64, C.POINTER(MhShape), _vp, C.POINTER(MhStats)]),
    ("vsc_guides_microhomology", C.c_int, [_vp, _vp, _vp, C.POINTER(MhShape), _vp, C.POINTER(MhStats)]),
    ("vsc_pattern_guides_microhomology", C.c_int, [_vp, _vp, _vp, C.POINTER(MhShape), _vp, C.POINTER(MhStats)]),
    ("vsc_guides_filter_microhomology", C.c_int, [_vp, _vp, _vp, C.POINTER(MhShape), C.c_uint32, C.c_uint32, C.POINTER(_vp)]),
    ("vsc_pattern_guides_filter_microhomology", C.c_int, [_vp, _vp, _vp, C.POINTER(MhShape), C.c_uint32, C.c_uint32, C.POINTER(_vp)]),
    ("vsc_pick_host", C.c_int, [_vp, C.c_uint32, _vp, C.c_uint64, _vp, _vp, C.c_uint32, C.POINTER(PickParams), _vp, _vp, _vp,
                                C.POINTER(PickStats)]),
    ("vsc_loci_pick", C.c_int, [_vp, _vp, _vp, C.c_uint64, _vp, _vp, C.c_uint32, C.POINTER(PickParams), _vp, _vp, _vp,
                                C.POINTER(PickStats)]),
    ("vsc_loci_pick_regions", C.c_int, [_vp, _vp, _vp, C.c_uint64, _vp, _vp, _vp, C.c_uint32, C.POINTER(PickParams), _vp, _vp, _vp,
                                        C.POINTER(PickStats)]),
    ("vsc_guides_pick", C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, C.c_uint32, _vp, C.POINTER(PickParams), _vp, _vp, _vp, C.POINTER(_vp),
                                  C.POINTER(PickStats)]),
    ("vsc_pattern_guides_pick", C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, C.c_uint32, _vp, C.POINTER(PickParams), _vp, _vp, _vp,
                                          C.POINTER(_vp), C.POINTER(PickStats)]),
    ("vsc_edit_site_text", C.c_int, [C.c_char_p, C.POINTER(EditShapeStruct), C.POINTER(C.c_uint32)]),
    ("vsc_loci_edit", C.c_int, [_vp, _vp, _vp, C.c_uint64, C.POINTER(EditShapeStruct), _vp, C.c_uint64, _vp, _vp, C.c_uint64,
                                C.POINTER(C.c_uint64), _vp, C.POINTER(EditStats)]),
    ("vsc_guides_edit", C.c_int, [_vp, _vp, _vp, C.POINTER(EditShapeStruct), _vp, C.c_uint64, _vp, _vp, C.c_uint64,
                                  C.POINTER(C.c_uint64), _vp, C.POINTER(EditStats)]),
    ("vsc_pattern_guides_edit", C.c_int, [_vp, _vp, _vp, C.POINTER(EditShapeStruct), _vp, C.c_uint64, _vp, _vp, C.c_uint64,
                                          C.POINTER(C.c_uint64), _vp, C.POINTER(EditStats)]),
    ("vsc_guides_filter_edit", C.c_int, [_vp, _vp, _vp, C.POINTER(EditShapeStruct), _vp, C.c_uint64, C.c_uint32, C.c_uint32,
                                         C.POINTER(_vp)]),
    ("vsc_pattern_guides_filter_edit", C.c_int, [_vp, _vp, _vp, C.POINTER(EditShapeStruct), _vp, C.c_uint64, C.c_uint32, C.c_uint32,
                                                 C.POINTER(_vp)]),
    ("vsc_cds_build", C.c_int, [_vp, C.c_uint32, _vp, C.c_uint64, C.c_uint32, C.POINTER(_vp)]),
    ("vsc_cds_build_error", C.c_char_p, []),
    ("vsc_cds_free", None, [_vp]),
    ("vsc_cds_info", C.c_int, [_vp, C.POINTER(CdsStats)]),
    ("vsc_codon_effect", C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_char_p, C.POINTER(C.c_uint32)]),
    ("vsc_effects_site_text", C.c_int, [_vp, C.POINTER(C.c_char_p), C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(EditShapeStruct),
                                        C.c_uint32, C.c_char_p, _vp, _vp, C.POINTER(C.c_uint32)]),
    ("vsc_loci_effects", C.c_int, [_vp, _vp, _vp, C.c_uint64, C.POINTER(EditShapeStruct), C.c_uint32, _vp, C.c_char_p, _vp, _vp,
                                   C.c_uint64, C.POINTER(C.c_uint64), _vp, C.POINTER(EffectsStats)]),
    ("vsc_guides_effects", C.c_int, [_vp, _vp, _vp, C.POINTER(EditShapeStruct), C.c_uint32, _vp, C.c_char_p, _vp, _vp, C.c_uint64,
                                     C.POINTER(C.c_uint64), _vp, C.POINTER(EffectsStats)]),
    ("vsc_pattern_guides_effects", C.c_int, [_vp, _vp, _vp, C.POINTER(EditShapeStruct), C.c_uint32, _vp, C.c_char_p, _vp, _vp,
                                             C.c_uint64, C.POINTER(C.c_uint64), _vp, C.POINTER(EffectsStats)]),
    ("vsc_guides_filter_effects", C.c_int, [_vp, _vp, _vp, C.POINTER(EditShapeStruct), C.c_uint32, _vp, C.c_char_p, C.c_uint32,
                                            C.c_uint32, C.POINTER(_vp)]),
    ("vsc_pattern_guides_filter_effects", C.c_int, [_vp, _vp, _vp, C.POINTER(EditShapeStruct), C.c_uint32, _vp, C.c_char_p, C.c_uint32,
                                                    C.c_uint32, C.POINTER(_vp)]),
    ("vsc_knockout_site_text", C.c_int, [_vp, C.POINTER(C.c_char_p), C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(KnockoutShapeStruct),
                                         C.c_char_p, _vp]),
    ("vsc_loci_knockout", C.c_int, [_vp, _vp, _vp, C.c_uint64, C.POINTER(KnockoutShapeStruct), _vp, C.c_char_p, _vp, _vp,
                                    C.POINTER(KnockoutStats)]),
    ("vsc_guides_knockout", C.c_int, [_vp, _vp, _vp, C.POINTER(KnockoutShapeStruct), _vp, C.c_char_p, _vp, _vp, C.POINTER(KnockoutStats)]),
    ("vsc_pattern_guides_knockout", C.c_int, [_vp, _vp, _vp, C.POINTER(KnockoutShapeStruct), _vp, C.c_char_p, _vp, _vp,
                                              C.POINTER(KnockoutStats)]),
    ("vsc_guides_filter_knockout", C.c_int, [_vp, _vp, _vp, C.POINTER(KnockoutShapeStruct), _vp, C.c_char_p, C.POINTER(KnockoutLimits),
                                             C.POINTER(_vp)]),
    ("vsc_pattern_guides_filter_knockout", C.c_int, [_vp, _vp, _vp, C.POINTER(KnockoutShapeStruct), _vp, C.c_char_p,
                                                     C.POINTER(KnockoutLimits), C.POINTER(_vp)]),
    ("vsc_prime_site_text", C.c_int, [C.c_char_p, C.POINTER(PrimeShapeStruct), C.c_uint32, C.c_uint32, C.c_char_p, _vp, _vp, _vp]),
    ("vsc_loci_prime", C.c_int, [_vp, _vp, _vp, C.c_uint64, C.POINTER(PrimeShapeStruct), _vp, C.c_uint64, _vp, _vp, C.c_uint64,
                                 C.POINTER(C.c_uint64), _vp, C.POINTER(PrimeStats)]),
    ("vsc_guides_prime", C.c_int, [_vp, _vp, _vp, C.POINTER(PrimeShapeStruct), _vp, C.c_uint64, _vp, _vp, C.c_uint64,
                                   C.POINTER(C.c_uint64), _vp, C.POINTER(PrimeStats)]),
    ("vsc_pattern_guides_prime", C.c_int, [_vp, _vp, _vp, C.POINTER(PrimeShapeStruct), _vp, C.c_uint64, _vp, _vp, C.c_uint64,
                                           C.POINTER(C.c_uint64), _vp, C.POINTER(PrimeStats)]),
    ("vsc_guides_filter_prime", C.c_int, [_vp, _vp, _vp, C.POINTER(PrimeShapeStruct), _vp, C.c_uint64, C.c_uint32, C.POINTER(_vp)]),
    ("vsc_pattern_guides_filter_prime", C.c_int, [_vp, _vp, _vp, C.POINTER(PrimeShapeStruct), _vp, C.c_uint64, C.c_uint32, C.POINTER(_vp)]),
    ("vsc_hdr_site_text", C.c_int, [C.c_char_p, C.POINTER(HdrShapeStruct), C.c_uint32, C.c_uint32, C.c_char_p, _vp, _vp, _vp]),
    ("vsc_loci_hdr", C.c_int, [_vp, _vp, _vp, C.c_uint64, C.POINTER(HdrShapeStruct), _vp, C.c_uint64, _vp, C.c_char_p, _vp, _vp, C.c_uint64,
                               C.POINTER(C.c_uint64), _vp, C.POINTER(HdrStats)]),
    ("vsc_guides_hdr", C.c_int, [_vp, _vp, _vp, C.POINTER(HdrShapeStruct), _vp, C.c_uint64, _vp, C.c_char_p, _vp, _vp, C.c_uint64,
                                 C.POINTER(C.c_uint64), _vp, C.POINTER(HdrStats)]),
    ("vsc_pattern_guides_hdr", C.c_int, [_vp, _vp, _vp, C.POINTER(HdrShapeStruct), _vp, C.c_uint64, _vp, C.c_char_p, _vp, _vp, C.c_uint64,
                                         C.POINTER(C.c_uint64), _vp, C.POINTER(HdrStats)]),
    ("vsc_guides_filter_hdr", C.c_int, [_vp, _vp, _vp, C.POINTER(HdrShapeStruct), _vp, C.c_uint64, _vp, C.c_char_p, C.c_uint32,
                                        C.POINTER(_vp)]),
    ("vsc_pattern_guides_filter_hdr", C.c_int, [_vp, _vp, _vp, C.POINTER(HdrShapeStruct), _vp, C.c_uint64, _vp, C.c_char_p, C.c_uint32,
                                                C.POINTER(_vp)]),
    ("vsc_fold_text", C.c_int, [C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32, C.POINTER(FoldShapeStruct), _vp]),
    ("vsc_loci_fold", C.c_int, [_vp, _vp, _vp, C.c_uint64, C.POINTER(FoldShapeStruct), C.c_char_p, C.c_uint32, _vp, C.POINTER(FoldStats)]),
    ("vsc_guides_fold", C.c_int, [_vp, _vp, _vp, C.POINTER(FoldShapeStruct), C.c_char_p, C.c_uint32, _vp, C.POINTER(FoldStats)]),
    ("vsc_pattern_guides_fold", C.c_int, [_vp, _vp, _vp, C.POINTER(FoldShapeStruct), C.c_char_p, C.c_uint32, _vp, C.POINTER(FoldStats)]),
    ("vsc_guides_filter_fold", C.c_int, [_vp, _vp, _vp, C.POINTER(FoldShapeStruct), C.c_char_p, C.c_uint32, C.POINTER(FoldLimits),
                                         C.POINTER(_vp)]),
    ("vsc_pattern_guides_filter_fold", C.c_int, [_vp, _vp, _vp, C.POINTER(FoldShapeStruct), C.c_char_p, C.c_uint32, C.POINTER(FoldLimits),
                                                 C.POINTER(_vp)]),
    ("vsc_motif_text", C.c_int, [C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32, C.POINTER(MotifStruct), C.c_uint32,
                                 C.POINTER(MotifShapeStruct), _vp]),
    ("vsc_loci_motifs", C.c_int, [_vp, _vp, _vp, C.c_uint64, C.POINTER(MotifShapeStruct), C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32, C.POINTER(MotifStruct), C.c_uint32, _vp, _vp,
                                  C.POINTER(MotifStats)]),
    ("vsc_guides_motifs", C.c_int, [_vp, _vp, _vp, C.POINTER(MotifShapeStruct), C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32, C.POINTER(MotifStruct), C.c_uint32, _vp, _vp,
                                    C.POINTER(MotifStats)]),
    ("vsc_pattern_guides_motifs", C.c_int, [_vp, _vp, _vp, C.POINTER(MotifShapeStruct), C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32, C.POINTER(MotifStruct), C.c_uint32, _vp, _vp,
                                            C.POINTER(MotifStats)]),
    ("vsc_guides_filter_motifs", C.c_int, [_vp, _vp, _vp, C.POINTER(MotifShapeStruct), C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32, C.POINTER(MotifStruct), C.c_uint32,
                                           C.POINTER(MotifLimits), C.POINTER(_vp)]),
    ("vsc_pattern_guides_filter_motifs", C.c_int, [_vp, _vp, _vp, C.POINTER(MotifShapeStruct), C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32, C.POINTER(MotifStruct), C.c_uint32,
                                                   C.POINTER(MotifLimits), C.POINTER(_vp)]),
    ("vsc_variation_host", C.c_int, [_vp, C.c_uint32, _vp, C.c_uint64, C.POINTER(VariationShapeStruct), _vp, C.c_uint64, _vp, _vp,
                                     C.c_uint64, C.POINTER(C.c_uint64), _vp]),
    ("vsc_loci_variation", C.c_int, [_vp, _vp, _vp, C.c_uint64, C.POINTER(VariationShapeStruct), _vp, C.c_uint64, _vp, _vp, C.c_uint64,
                                     C.POINTER(C.c_uint64), _vp, C.POINTER(VariationStats)]),
    ("vsc_guides_variation", C.c_int, [_vp, _vp, _vp, C.POINTER(VariationShapeStruct), _vp, C.c_uint64, _vp, _vp, C.c_uint64,
                                       C.POINTER(C.c_uint64), _vp, C.POINTER(VariationStats)]),
    ("vsc_pattern_guides_variation", C.c_int, [_vp, _vp, _vp, C.POINTER(VariationShapeStruct), _vp, C.c_uint64, _vp, _vp, C.c_uint64,
                                               C.POINTER(C.c_uint64), _vp, C.POINTER(VariationStats)]),
    ("vsc_guides_filter_variation", C.c_int, [_vp, _vp, _vp, C.POINTER(VariationShapeStruct), _vp, C.c_uint64,
                                              C.POINTER(VariationFilterStruct), C.POINTER(_vp)]),
    ("vsc_pattern_guides_filter_variation", C.c_int, [_vp, _vp, _vp, C.POINTER(VariationShapeStruct), _vp, C.c_uint64,
                                                      C.POINTER(VariationFilterStruct), C.POINTER(_vp)]),
    ("vsc_sam_order", None, [_vp, C.c_uint64, _vp, _vp]),
]
# include/varscot_hip_debug.h (test / experiment hooks, not part of the drop-in boundary)
DEBUG_SYMBOLS = [
    ("vsc_ctx_set_debug_params", C.c_int, [_vp, C.POINTER(DebugParams)]),
    ("vsc_ctx_get_debug_params", C.c_int, [_vp, C.POINTER(DebugParams)]),
    ("vsc_debug_set_host_timing", None, [C.c_int]),
    ("vsc_ctx_create_masked", C.c_int, [C.c_int, _vp, C.c_uint32, C.POINTER(_vp)]),
    ("vsc_debug_pattern_target_ranges", C.c_int, [_vp, C.c_uint32, _vp, C.c_uint64, C.c_uint32, C.c_uint32, _vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    ("vsc_multi_create_debug", C.c_int, [C.POINTER(C.c_int), C.c_int, C.POINTER(MultiDebugParams), C.POINTER(_vp)]),
    ("vsc_debug_guides_from_host", C.c_int, [_vp, _vp, _vp, C.c_uint64, C.POINTER(_vp)]),
    ("vsc_debug_pattern_guides_from_host", C.c_int, [_vp, _vp, _vp, C.c_uint64, C.POINTER(_vp)]),
    ("vsc_debug_sites_ms", C.c_int, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    ("vsc_debug_site_table_ms", C.c_int, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    ("vsc_debug_bulge_hits_from_host", C.c_int, [_vp, _vp, C.c_uint64, C.POINTER(_vp)]),
    ("vsc_debug_sites_from_host", C.c_int, [_vp, _vp, C.c_uint64, C.POINTER(_vp)]),
    ("vsc_debug_prime_bitmap", C.c_int, [_vp, C.c_int]),
    ("vsc_debug_prime_groups_per_cu", C.c_int, [_vp, C.c_uint32]),
    ("vsc_debug_hdr_bitmap", C.c_int, [_vp, C.c_int]),
    ("vsc_debug_hdr_groups_per_cu", C.c_int, [_vp, C.c_uint32]),
    ("vsc_debug_fold_groups_per_cu", C.c_int, [_vp, C.c_uint32]),
    ("vsc_debug_motif_groups_per_cu", C.c_int, [_vp, C.c_uint32]),
    ("vsc_debug_knockout_groups_per_cu", C.c_int, [_vp, C.c_uint32]),
    ("vsc_debug_knockout_in_place", C.c_int, [_vp, C.c_int]),
    ("vsc_debug_knockout_table", C.c_int, [_vp, _vp, _vp, C.POINTER(C.c_uint32)]),
    ("vsc_debug_variation_block_bits", C.c_int, [_vp, C.c_uint32]),
    ("vsc_debug_genome_from_contigs", C.c_int, [_vp, _vp, C.c_uint32, C.c_uint64, C.POINTER(_vp)]),
    ("vsc_debug_sort_records", C.c_int, [_vp, _vp, C.POINTER(DebugSortInput), C.POINTER(DebugSortInfo), C.POINTER(_vp)]),
]

_lib = None


class VarscotError(RuntimeError):
    def __init__(self, code, message=""):
        self.code = code
        super().__init__("%s (%d)%s" % (ERRORS.get(code, "VSC_ERR"), code, ": " + message if message else ""))


def lib():
    """The loaded shared library.  Raises ImportError (never falls back) when it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "libvarscot_hip.so is not built (%s). Build it with `make -C varscot_amd/csrc` or "
                "`python -c 'import __graft_entry__ as g; g.build()'`; there is no CPU fallback." % LIB_PATH)
        # PyTorch-ROCm bundles its own copy of the HIP runtime.  Two runtimes in one process do not share
        # the device: whichever initialises it second reports "no GPU".  With torch imported first the
        # dynamic loader resolves this library's libamdhip64 dependency to the copy torch already
        # loaded, so there is ONE runtime whatever the later order of initialisation.  (varscot_amd.dist
        # and bench.py need torch anyway; the C++ tools never load it.)
        if os.environ.get("VSC_NO_TORCH_PRELOAD") != "1":
            try:
                import torch  # noqa: F401
            except ImportError:
                pass
        L = C.CDLL(LIB_PATH)
        for name, restype, argtypes in SYMBOLS + DEBUG_SYMBOLS:
            fn = getattr(L, name)  # AttributeError = header and library out of sync
            fn.restype = restype
            fn.argtypes = argtypes
        _lib = L
    return _lib


def check(code, ctx=None):
    if code != VSC_OK:
        msg = ""
        if ctx:
            msg = lib().vsc_last_error(ctx).decode(errors="replace")
        raise VarscotError(code, msg)


def ptr(a):
    """void* of a C-contiguous numpy array (or None)."""
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.c_void_p)
