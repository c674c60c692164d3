"""varscot_amd - MI355X-native implementation of VARSCOT's genome-wide off-target search hot path.

The compute lives in libvarscot_hip.so (hand-written HIP for gfx950 behind the C ABI of
include/varscot_hip.h); this package is the thin host-side mirror used by tests, bench.py and the
Python entry points.  There is no CPU fallback: without the built library importing fails.
"""
from ._lib import HIT_DTYPE, CONTIG_DTYPE, N_FEATURES, SUMMARY_DTYPE, VOTES_DTYPE, TABLE_ROW_DTYPE, LOCUS_DTYPE, INTERVAL_DTYPE, LIB_PATH, REGION_NONE, VARIANT_LABEL_DTYPE, VARIANT_VAR, VARIANT_DUP, VARIANT_ON_TARGET, PATTERN_VARIANT_ROW_DTYPE, PATTERN_REF_SHADOWED, PATTERN_REF_ON_TARGET, SELECT, EnumParams, PairParams, GuidePair, PairSummary, PairSite, PAIR_SUMMARY_DTYPE, PAIR_SITE_DTYPE, BULGE_HIT_DTYPE, BULGE_DNA, BULGE_RNA, BulgeParams, PATTERN_HIT_DTYPE, PatternParams, PatternEnumParams, PatternBulgeParams, PatternTableShape, PatternSelect, SiteParams, EffShape, EffStats, MhShape, MhStats, EditStats, EDIT_TARGET_DTYPE, VarscotError, lib  # noqa: F401
from .api import (Context, Genome, Hits, MultiContext, PackedGenome, Regions, VariantMap, device_count, expected_active, individual_rows, mit_fixed, mit_specificity, ScoreTable, PatternTable, BulgeTable, SITE_SCORE_DTYPE, table_specificity, TABLE_ONE, EfficiencyModel, EFF_UNDEFINED_BITS, MicrohomologyShape, MH_UNDEFINED, microhomology_text, microhomology_scores, EditShape, EDITORS, EDIT_PAIR_DTYPE, EDIT_UNDEFINED, edit_site_text, unpack_edit_info, edit_targets, edit_pick_inputs, PickShape, PICK_NONE, pick_host, order_bits, pick_key, pick_column, PICK_COLUMNS, nickase_delta, pair_loci,  # noqa: F401
                  bulge_align, pack_guides, PATTERNS, pattern_match, pattern_bulge_align, pattern_strings, pattern_protospacer, pattern_guide_text, PatternGuides, unpack_pattern_info, sam_order, unpack_bulge_info, collapse_sites, unpack_site_members, SITE_DTYPE, SITE_ROW_DTYPE, unpack_features, unpack_guides, variant_windows, PatternHits, pattern_variants_screen, individual_pattern_rows)

lib()  # fail loudly at import time if the HIP extension is missing
