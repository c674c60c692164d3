"""Host-side Python mirror of the C ABI (include/varscot_hip.h): packed genome, device context,
search and per-hit scoring.  Thin plumbing only - every computation happens in libvarscot_hip.so.
"""
import ctypes as C
import math
import os
import weakref

import numpy as np

from . import _lib
from ._lib import (ALGO_AUTO, ALGO_SCAN, ALGO_SEED, HIT_DTYPE, CONTIG_DTYPE, N_FEATURES, SearchParams, Timing, check,
                   lib, ptr)

READ_LEN = 23
TILE_WORDS = 64  # shard boundaries are multiples of this many 32-base words (one scan tile)


def pack_guides(guides):
    """23-nt reads -> uint64 codes (vsc_pack_guide; non-ACGT letters become A like SeqAn's Dna)."""
    L = lib()
    out = np.empty(len(guides), dtype=np.uint64)
    for i, g in enumerate(guides):
        b = g if isinstance(g, bytes) else g.encode()
        if len(b) != READ_LEN:
            raise ValueError("read %d has length %d; VARSCOT searches 23-nt reads (20 nt + PAM)" % (i, len(b)))
        out[i] = L.vsc_pack_guide(b)
    return out


def unpack_guides(codes):
    """uint64 codes (pack_guides, enumerate_guides) -> 23-nt strings: base i = "ACGT"[code >> 2 i & 3]."""
    c = np.ascontiguousarray(codes, dtype=np.uint64).reshape(-1, 1)
    idx = ((c >> (2 * np.arange(READ_LEN, dtype=np.uint64))) & np.uint64(3)).astype(np.intp)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)[idx]
    return [row.tobytes().decode() for row in letters]


BULGE_HIT_DTYPE = _lib.BULGE_HIT_DTYPE


def unpack_bulge_info(info):
    """The fields of vsc_bulge_hit.info (VSC_BULGE_* of the header), of one word or an array of them: a dict of strand (1 =
    '-'), kind (0 DNA, 1 RNA), size, d (site length - 23: +size DNA, -size RNA), index and nm."""
    w = np.asarray(info, dtype=np.uint32)
    kind, size = (w >> np.uint32(12)) & np.uint32(1), (w >> np.uint32(10)) & np.uint32(3)
    return {"strand": w >> np.uint32(31), "kind": kind, "size": size,
            "d": np.where(kind == 1, -size.astype(np.int32), size.astype(np.int32)),
            "index": (w >> np.uint32(5)) & np.uint32(31), "nm": w & np.uint32(31)}


SITE_DTYPE = _lib.SITE_DTYPE
SITE_ROW_DTYPE = _lib.SITE_ROW_DTYPE
_SITE_ANCHORS = {"end": _lib.SITE_ANCHOR_END, "start": _lib.SITE_ANCHOR_START}


def unpack_site_members(members):
    """The fields of vsc_site.members, of one word or an array of them: a dict of nm (int64, a last axis of five entries for
    d = -2, -1, 0, 1, 2; -1 where the site has no member with that d) and count (the number of members)."""
    m = np.asarray(members, dtype=np.uint32)
    nm = ((m[..., None] >> (5 * np.arange(5, dtype=np.uint32))) & 31).astype(np.int64)
    nm[nm == _lib.SITE_ABSENT] = -1
    return {"nm": nm, "count": ((m >> 25) & 7).astype(np.int64)}


def _site_params(length, anchor):
    if anchor not in _SITE_ANCHORS:
        raise ValueError("anchor must be 'end' or 'start', not %r" % (anchor,))
    return _lib.SiteParams(int(length), _SITE_ANCHORS[anchor])


def collapse_sites(plain, bulged, n_guides, length=23, anchor="end"):
    """vsc_sites_collapse / vsc_sites_collapse_pattern: plain records (HIT_DTYPE or PATTERN_HIT_DTYPE; the dtype picks the
    function) and bulged records (BULGE_HIT_DTYPE) of the same guides and genome, each in the order its search returns,
    collapsed into one SITE_DTYPE record per cut site - the definition of Genome.search_sites on the host, by the functions the
    kernels run.  Either may be None (not both).  Returns (sites in the order of their best alignments, SITE_ROW_DTYPE rows
    per guide).  No device is needed."""
    p = _site_params(length, anchor)
    pattern = plain is not None and np.asarray(plain).dtype == PATTERN_HIT_DTYPE
    if plain is not None:
        plain = np.ascontiguousarray(plain, dtype=PATTERN_HIT_DTYPE if pattern else HIT_DTYPE)
    if bulged is not None:
        bulged = np.ascontiguousarray(bulged, dtype=BULGE_HIT_DTYPE)
    n_plain, n_bulged = (0 if plain is None else len(plain)), (0 if bulged is None else len(bulged))
    fn = lib().vsc_sites_collapse_pattern if pattern else lib().vsc_sites_collapse
    rows = np.zeros(int(n_guides), dtype=SITE_ROW_DTYPE)
    sites = np.zeros(n_plain + n_bulged, dtype=SITE_DTYPE)
    n = C.c_uint64(0)
    # (an empty array has a data pointer of its own: None is what says "no such list")
    check(fn(None if plain is None else plain.ctypes.data_as(C.c_void_p), n_plain, None if bulged is None else bulged.ctypes.data_as(C.c_void_p),
             n_bulged, int(n_guides), C.byref(p), sites.ctypes.data_as(C.c_void_p), len(sites), C.byref(n), rows.ctypes.data_as(C.c_void_p)))
    return sites[:n.value].copy(), rows


def bulge_align(read, site, d):
    """vsc_bulge_align: (NM, index) of one 23-nt read against one site of 23 + d letters in read orientation, d in -2, -1, 1, 2 -
    the definition of the bulge search on the host, by the function the kernels run.  No device is needed."""
    r = read if isinstance(read, bytes) else read.encode()
    s = site if isinstance(site, bytes) else site.encode()
    if len(r) != READ_LEN:
        raise ValueError("the read has length %d; a read is 23 nt (20 nt + PAM)" % len(r))
    nm, index = C.c_uint32(), C.c_uint32()
    check(lib().vsc_bulge_align(lib().vsc_pack_guide(r), s, int(d), C.byref(nm), C.byref(index)))
    return int(nm.value), int(index.value)


PATTERN_HIT_DTYPE = _lib.PATTERN_HIT_DTYPE

# Presets of search_pattern: name -> (PAM at the 5' end, protospacer length, PAM at the 3' end).  pattern_strings() makes the
# pattern and the guide of a protospacer from a row; any other shape is two strings written by hand.
PATTERNS = {
    "SpCas9": ("", 20, "NGG"),
    "SpCas9-NRG": ("", 20, "NRG"),
    "SpCas9-NG": ("", 20, "NGN"),
    "SaCas9": ("", 21, "NNGRRT"),
    "Cas12a": ("TTTV", 23, ""),
}


def pattern_strings(preset, protospacer=None):
    """(pattern, guide) of a row of PATTERNS (its name, or a (5' PAM, length, 3' PAM) tuple): the pattern is the PAM letters
    around N x length, the guide the protospacer with N at the PAM positions - they are not compared, as in Cas-OFFinder.
    Without a protospacer the guide is None."""
    five, n, three = PATTERNS[preset] if isinstance(preset, str) else preset
    pattern = five + "N" * n + three
    if protospacer is None:
        return pattern, None
    if len(protospacer) != n:
        raise ValueError("the protospacer has %d letters; this preset takes %d" % (len(protospacer), n))
    return pattern, "N" * len(five) + protospacer + "N" * len(three)


def pattern_protospacer(preset):
    """(start, length) of the protospacer in the pattern of a row of PATTERNS (its name, or a (5' PAM, length, 3' PAM) tuple):
    what enumerate_pattern takes as `protospacer`."""
    five, n, _ = PATTERNS[preset] if isinstance(preset, str) else preset
    return len(five), n


def pattern_guide_text(code, length, protospacer, spell_pam=False):
    """vsc_pattern_guide_text: the `length` letters of one code of enumerate_pattern - the site's letters inside the
    protospacer (start, length), outside it N (the query form: not compared by search_pattern) or, with spell_pam, the site's
    letters.  No device is needed."""
    out = C.create_string_buffer(int(length))
    check(lib().vsc_pattern_guide_text(int(code), int(length), int(protospacer[0]), int(protospacer[1]), 1 if spell_pam else 0, out))
    return out.raw.decode()


class PatternGuides:
    """The candidates of Genome.enumerate_pattern: codes (uint64: hi plane << 32 | lo plane of the site in read orientation),
    loci (LOCUS_DTYPE, pos = the site's start on the forward genome) in ascending (contig, pos), '+' before '-'."""

    def __init__(self, pattern, protospacer, codes, loci):
        self.pattern, self.protospacer, self.codes, self.loci = pattern, (int(protospacer[0]), int(protospacer[1])), codes, loci

    def __len__(self):
        return len(self.codes)

    def text(self, spell_pam=False):
        """The guides as strings that search_pattern takes: N outside the protospacer, or the site's letters there too."""
        return [pattern_guide_text(c, len(self.pattern), self.protospacer, spell_pam) for c in self.codes]


def _pattern_enum_params(protospacer, rule, strands, gc, max_t_run, max_guides):
    """vsc_pattern_enum_params of enumerate_pattern's arguments.  Only what cannot be put into the struct is refused here: the
    library checks the values."""
    if rule not in ("overlap", "inside", 0, 1):
        raise ValueError("rule must be 'overlap' or 'inside'")
    if strands not in ("both", "+", "-", 0, 1, 2, 3):
        raise ValueError("strands must be 'both', '+' or '-'")
    fields = [int(protospacer[0]), int(protospacer[1]), {"both": 0, "+": 1, "-": 2}.get(strands, strands), int(gc[0]), int(gc[1]), int(max_t_run)]
    if any(not 0 <= v <= 255 for v in fields):
        raise ValueError("protospacer, gc and max_t_run must lie in 0..255")
    p = _lib.PatternEnumParams()
    p.ps_start, p.ps_len, p.strands, p.gc_min, p.gc_max, p.max_t_run = fields
    p.rule = {"overlap": _lib.REGION_OVERLAP, "inside": _lib.REGION_INSIDE}.get(rule, rule)
    p.max_guides = int(max_guides)
    return p


def _intervals(targets):
    """INTERVAL_DTYPE array of (contig, start, end) triples (or of such an array), as Regions takes them."""
    if isinstance(targets, np.ndarray) and targets.dtype == _lib.INTERVAL_DTYPE:
        return np.ascontiguousarray(targets)
    a = np.asarray(targets, dtype=np.int64).reshape(-1, 3)
    if len(a) and (a.min() < 0 or a.max() >= 2 ** 32):
        raise ValueError("interval fields must fit 32 unsigned bits")
    iv = np.zeros(len(a), dtype=_lib.INTERVAL_DTYPE)
    iv["contig"], iv["start"], iv["end"] = a[:, 0], a[:, 1], a[:, 2]
    return iv


def unpack_pattern_info(info):
    """The fields of vsc_pattern_hit.info (VSC_PATTERN_* of the header), of one word or an array of them: a dict of strand
    (1 = '-') and nm."""
    w = np.asarray(info, dtype=np.uint32)
    return {"strand": w >> np.uint32(31), "nm": w & np.uint32(63)}


def pattern_match(pattern, guide, site):
    """vsc_pattern_match: (hit, nm, mask) of one site in read orientation under one pattern and one guide, all of one length
    in 16..32 - hit = the site holds ACGT only and satisfies the pattern, nm and mask (bit j: site letter j is not in guide
    letter j) = the compare the kernels run.  No device is needed."""
    p, g, s = (x if isinstance(x, bytes) else x.encode() for x in (pattern, guide, site))
    if not len(p) == len(g) == len(s):
        raise ValueError("pattern, guide and site must have the same length (%d, %d, %d)" % (len(p), len(g), len(s)))
    hit, nm, mask = C.c_uint32(), C.c_uint32(), C.c_uint32()
    check(lib().vsc_pattern_match(p, g, s, len(p), C.byref(hit), C.byref(nm), C.byref(mask)))
    return bool(hit.value), int(nm.value), int(mask.value)


def pattern_bulge_align(pattern, guide, site, protospacer, d):
    """vsc_pattern_bulge_align: (hit, nm, index) of one site of len(pattern) + d letters in read orientation under one pattern
    and one guide, d in -2, -1, 1, 2, with a bulge inside protospacer = (start, length) - hit = the site holds ACGT only and
    satisfies the bulged pattern, nm = the fewest mismatches over the split points, index = the smallest split point that
    reaches it: the definition of search_pattern_bulges on the host, by the functions the kernels run.  No device is needed."""
    p, g, s = (x if isinstance(x, bytes) else x.encode() for x in (pattern, guide, site))
    if len(p) != len(g):
        raise ValueError("pattern and guide must have the same length (%d, %d)" % (len(p), len(g)))
    hit, nm, index = C.c_uint32(), C.c_uint32(), C.c_uint32()
    check(lib().vsc_pattern_bulge_align(p, g, s, len(p), int(protospacer[0]), int(protospacer[1]), int(d), C.byref(hit), C.byref(nm),
                                        C.byref(index)))
    return bool(hit.value), int(nm.value), int(index.value)


def _enum_params(pam, strands, gc, max_t_run, max_guides):
    """vsc_enum_params of enumerate_guides' arguments.  Only what cannot be put into the struct is refused here: the library
    checks the values (a PAM letter outside ACGT, gc bounds above 20, ... are VSC_ERR_INVALID there)."""
    b = pam if isinstance(pam, bytes) else pam.encode()
    if len(b) != 2:
        raise ValueError("the guide PAM must be 2 letters (NGG: 'GG')")
    if strands not in ("both", "+", "-", 0, 1, 2, 3):
        raise ValueError("strands must be 'both', '+' or '-'")
    gc_min, gc_max = gc
    p = _lib.EnumParams()
    p.pam = b
    p.strands = {"both": 0, "+": 1, "-": 2}.get(strands, strands)
    p.gc_min, p.gc_max, p.max_t_run, p.max_guides = int(gc_min), int(gc_max), int(max_t_run), int(max_guides)
    return p


def _label_regions(labels, regions):
    """The Regions that enumerate_guides' labels= option asks to label against: None (labels=False), `regions` (labels=True)
    or the Regions given as labels= itself."""
    if labels is None or labels is False:
        return None
    if labels is True:
        if regions is None:
            raise ValueError("labels=True labels the candidates with the interval of `regions` they lie in: give regions")
        return regions
    if not isinstance(labels, Regions):
        raise ValueError("labels must be False, True or a Regions")
    return labels


def _guides_arrays(handle, check_fn, label_regions=None):
    """(codes uint64[n], loci LOCUS_DTYPE[n]) copied out of a vsc_guides, which is freed - with label_regions also the
    candidates' labels under those regions (uint32[n], vsc_guides_locate), taken before the handle goes."""
    L = lib()
    try:
        n = int(L.vsc_guides_count(handle))
        pc, pl = C.c_void_p(), C.c_void_p()
        check_fn(L.vsc_guides_data(handle, C.byref(pc), C.byref(pl)))
        if n == 0:
            codes, loci = np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=_lib.LOCUS_DTYPE)
        else:
            codes = np.frombuffer((C.c_char * (n * 8)).from_address(pc.value), dtype=np.uint64).copy()
            loci = np.frombuffer((C.c_char * (n * 16)).from_address(pl.value), dtype=_lib.LOCUS_DTYPE).copy()
        if label_regions is None:
            return codes, loci
        labels = np.full(n, _lib.REGION_NONE, dtype=np.uint32)
        check_fn(L.vsc_guides_locate(handle, label_regions._h, ptr(labels)))
        return codes, loci, labels
    finally:
        L.vsc_guides_free(handle)


def nickase_delta(offset_min, offset_max):
    """The delta range of a nickase offset range: offset = the gap between the two protospacers' PAM-distal ends (negative:
    they overlap), delta = pos('+' window) - pos('-' window) = offset + 23."""
    return int(offset_min) + READ_LEN, int(offset_max) + READ_LEN


def _pair_params(delta):
    """vsc_pair_params of a (delta_min, delta_max) pair; the library checks the values."""
    lo, hi = delta
    if not (-2 ** 31 <= int(lo) < 2 ** 31 and -2 ** 31 <= int(hi) < 2 ** 31):
        raise ValueError("delta bounds must fit 32 signed bits")
    p = _lib.PairParams()
    p.delta_min, p.delta_max = int(lo), int(hi)
    return p


def _collect_pairs(call):
    """call(pairs_ptr, capacity, byref(count)) -> status, run twice: count, then fill.  Returns uint32[n, 2]."""
    n = C.c_uint64()
    call(None, 0, C.byref(n))
    out = np.zeros((int(n.value), 2), dtype=np.uint32)
    if n.value:
        call(ptr(out), int(n.value), C.byref(n))
    return out


def pair_loci(loci, delta):
    """vsc_loci_pairs, on the host: every (a, b) with loci[a] a '-' window, loci[b] a '+' window on the same contig and
    delta[0] <= pos(b) - pos(a) <= delta[1], as uint32[n, 2] in ascending (a, b).  loci: LOCUS_DTYPE or (contig, pos, strand)
    rows, in any order; contig 0xFFFFFFFF takes part in nothing."""
    lo = _loci(loci, len(loci))
    p = _pair_params(delta)
    return _collect_pairs(lambda out, cap, n: check(lib().vsc_loci_pairs(ptr(lo), len(lo), C.byref(p), out, cap, n)))


def _guides_pairs(handle, check_fn, delta):
    """vsc_guides_pairs of a vsc_guides (on its device; a host-only object: on the host) as uint32[n, 2]."""
    p = _pair_params(delta)
    return _collect_pairs(lambda out, cap, n: check_fn(lib().vsc_guides_pairs(handle, C.byref(p), out, cap, n)))


def _loci(exclude, n):
    """(contig, pos, strand) per guide -> vsc_locus array (None stays None)."""
    if exclude is None:
        return None
    if isinstance(exclude, np.ndarray) and exclude.dtype == _lib.LOCUS_DTYPE:
        ex = np.ascontiguousarray(exclude)
    else:
        a = np.asarray(exclude, dtype=np.int64).reshape(-1, 3)
        ex = np.zeros(len(a), dtype=_lib.LOCUS_DTYPE)
        ex["contig"], ex["pos"], ex["strand"] = (a[:, 0] & 0xFFFFFFFF), a[:, 1], a[:, 2]
    if len(ex) != n:
        raise ValueError("exclude holds %d loci for %d guides" % (len(ex), n))
    return ex


def mit_specificity(mit_sum):
    """CRISPOR's guide specificity (mitSpecScore before rounding) from a summary's mit_sum (vsc_mit_specificity)."""
    return lib().vsc_mit_specificity(int(mit_sum))


def mit_fixed(mit):
    """An MIT score as a floor for search_select: the smallest fixed-point score (units of 2^-24) that is >= mit."""
    return int(np.ceil(float(mit) * 2.0 ** 24))


def _select(top_k, min_score):
    if not (0 <= int(top_k) < 2 ** 32 and 0 <= int(min_score) < 2 ** 32):
        raise ValueError("top_k and min_score must fit 32 unsigned bits")
    s = _lib.Select()
    s.top_k, s.min_score = int(top_k), int(min_score)
    return s


def _classify(forest, activity, n):
    """vsc_classify for a classifier.Forest and one on-target activity per guide; returns (struct, what it points at)."""
    act = np.ascontiguousarray(activity, dtype=np.float64)
    if len(act) != n:
        raise ValueError("one on-target activity per guide")
    model = _lib.RfModel(forest.n_trees, forest.n_nodes, ptr(forest.status), ptr(forest.feature), ptr(forest.left), ptr(forest.right),
                         ptr(forest.split), ptr(forest.node_class))
    return _lib.Classify(C.pointer(model), ptr(act), (C.c_uint32 * 2)(0, 0)), (model, act)


def expected_active(votes_rows, n_trees):
    """The expected number of active off-targets per guide - the sum of the forest's probabilities votes / n_trees over the
    guide's counted hits - from the VOTES_DTYPE rows of summarize_classified."""
    return votes_rows["votes_sum"].astype(np.float64) / float(n_trees)


TABLE_ROW_DTYPE = _lib.TABLE_ROW_DTYPE
TABLE_ONE = 1 << 30  # the fixed-point unit of the table scores: f = rint(score * 2^30)


def table_specificity(score_sum):
    """A guide's specificity from a table row's score_sum (vsc_table_specificity): 100 / (100 + sum * 2^-30) * 100 - for a CFD
    table CRISPOR's cfdSpecScore before rounding (the tools round with floor(x + 0.5))."""
    return lib().vsc_table_specificity(int(score_sum))


def _base(letter, what):
    i = "ACGT".find(letter.upper().replace("U", "T")) if len(letter) == 1 else -1
    if i < 0:
        raise ValueError("%s: %r is no base" % (what, letter))
    return i


class ScoreTable:
    """A table-driven off-target score (vsc_score_table; the CFD form): pair[20][4][4] - the weight of guide base g against
    site base s (the site's letter in READ orientation) at read position j, j = 0 the PAM-distal end, bases A 0, C 1, G 2,
    T 3 - and pam[16], the weight of the site's letters at read positions 21 and 22 (4 * first + second).  Every weight in
    [0, 1], pair[j][b][b] == 1.  The package ships no table."""

    def __init__(self, pair, pam):
        self.pair = np.ascontiguousarray(pair, dtype=np.float64)
        self.pam = np.ascontiguousarray(pam, dtype=np.float64).reshape(-1)
        if self.pair.shape != (20, 4, 4) or self.pam.shape != (16,):
            raise ValueError("a score table is pair[20][4][4] and pam[16]")
        h = C.c_void_p()
        self._h = None
        check(lib().vsc_score_table_build(ptr(self.pair), ptr(self.pam), C.byref(h)))
        self._h = h

    @classmethod
    def from_tsv(cls, path, default=None):
        """A table from a text file: a line is `j<TAB>g<TAB>s<TAB>w` (j 0-based read position, g the guide's letter, s the
        site's letter in read orientation) or `PAM<TAB>XY<TAB>w`; '#' starts a comment, a weight of '?' stands for an
        entry that is not known.  Entries that are missing or unknown are an error unless default= gives their weight."""
        pair = np.full((20, 4, 4), np.nan)
        pam = np.full(16, np.nan)
        for b in range(4):
            pair[:, b, b] = 1.0
        with open(path) as fh:
            for n, line in enumerate(fh, 1):
                f = line.split("#", 1)[0].split()
                if not f:
                    continue
                where = "%s:%d" % (path, n)
                try:
                    w = np.nan if f[-1] == "?" else float(f[-1])
                    if f[0] == "PAM" and len(f) == 3 and len(f[1]) == 2:
                        pam[4 * _base(f[1][0], where) + _base(f[1][1], where)] = w
                    elif len(f) == 4 and 0 <= int(f[0]) < 20:
                        pair[int(f[0]), _base(f[1], where), _base(f[2], where)] = w
                    else:
                        raise ValueError("neither 'j g s w' nor 'PAM XY w'")
                except ValueError as e:
                    raise ValueError(str(e) if str(e).startswith(where) else "%s: %s" % (where, e)) from None
        missing = int(np.isnan(pair).sum() + np.isnan(pam).sum())
        if missing:
            if default is None:
                raise ValueError("%s: %d entries are missing or unknown and no default= is given" % (path, missing))
            pair[np.isnan(pair)] = float(default)
            pam[np.isnan(pam)] = float(default)
        return cls(pair, pam)

    @classmethod
    def from_doench(cls, mm_scores, pam_scores, default=None):
        """A table from dictionaries keyed the way Doench et al.'s published CFD calculator is remembered to key its pickles:
        mm_scores["rX:dY,pos"] with X the guide's letter (T written U), Y the COMPLEMENT of the site's letter and pos
        1-based; pam_scores["XY"] for the site's last two letters.  NOTHING PINS THIS MAPPING: the reference this project is
        tested against holds no copy of those files - check a few scores against a calculator you trust before relying on
        it.  Entries the dictionaries lack are an error unless default= gives their weight."""
        comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
        pair = np.ones((20, 4, 4))
        pam = np.empty(16)
        missing = 0
        for j in range(20):
            for g, gl in enumerate("ACGT"):
                for s, sl in enumerate("ACGT"):
                    if g != s:
                        w = mm_scores.get("r%s:d%s,%d" % (gl.replace("T", "U"), comp[sl], j + 1), default)
                        missing += w is None
                        pair[j, g, s] = np.nan if w is None else float(w)
        for a, al in enumerate("ACGT"):
            for b, bl in enumerate("ACGT"):
                w = pam_scores.get(al + bl, default)
                missing += w is None
                pam[4 * a + b] = np.nan if w is None else float(w)
        if missing:
            raise ValueError("%d entries are missing and no default= is given" % missing)
        return cls(pair, pam)

    def info(self):
        st = _lib.ScoreTableStats()
        check(lib().vsc_score_table_info(self._h, C.byref(st)))
        return {"serial": int(st.serial), "zero_weights": int(st.zero_weights)}

    def score(self, guide, site, fixed=False):
        """vsc_table_score: the score of one guide against one site, both 23-nt strings (or pack_guides codes) in read
        orientation; fixed=True: (score, rint(score * 2^30))."""
        g = int(guide) if isinstance(guide, (int, np.integer)) else int(pack_guides([guide])[0])
        s = int(site) if isinstance(site, (int, np.integer)) else int(pack_guides([site])[0])
        x, f = C.c_double(), C.c_uint32()
        check(lib().vsc_table_score(self._h, g, s, C.byref(x), C.byref(f)))
        return (x.value, f.value) if fixed else x.value

    def close(self):
        if getattr(self, "_h", None):
            lib().vsc_score_table_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PatternTable:
    """A table score for the hits of a pattern search (vsc_pattern_table; the CFD form for any nuclease): length = the pattern's
    L, protospacer = (start, length) in read positions, pair[ps_len][4][4] - the weight of guide base g against site base s
    (the site's letter in READ orientation) at read position start + i, bases A 0, C 1, G 2, T 3 - pam_positions = up to four
    read positions outside the protospacer, ascending, and pam[4 ** len(pam_positions)], the weight of the site's letters
    there (first position most significant).  Every weight in [0, 1], pair[i][b][b] == 1.  The package ships no table."""

    def __init__(self, length, protospacer, pair, pam_positions=(), pam=(1.0,)):
        self.length = int(length)
        self.protospacer = (int(protospacer[0]), int(protospacer[1]))
        self.pam_positions = tuple(int(q) for q in pam_positions)
        self.pair = np.ascontiguousarray(pair, dtype=np.float64)
        self.pam = np.ascontiguousarray(pam, dtype=np.float64).reshape(-1)
        if len(self.pam_positions) > 4:
            raise ValueError("a pattern table looks at four PAM positions at the most")
        if self.pair.shape != (self.protospacer[1], 4, 4) or self.pam.shape != (4 ** len(self.pam_positions),):
            raise ValueError("a pattern table is pair[ps_len][4][4] and pam[4 ** n_pam]")
        shape = _lib.PatternTableShape(self.length, self.protospacer[0], self.protospacer[1], len(self.pam_positions))
        for t, q in enumerate(self.pam_positions):
            shape.pam_pos[t] = q
        h = C.c_void_p()
        self._h = None
        check(lib().vsc_pattern_table_build(C.byref(shape), ptr(self.pair), ptr(self.pam), C.byref(h)))
        self._h = h

    @classmethod
    def from_score_table(cls, table):
        """The SpCas9 shape with a ScoreTable's weights: 23 letters, protospacer (0, 20), PAM positions (21, 22) - every score
        is that table's, bit for bit."""
        return cls(23, (0, 20), table.pair, (21, 22), table.pam)

    @classmethod
    def from_tsv(cls, path):
        """A table from the text file to_tsv writes (tools/README.md): tab- or blank-separated lines `shape L ps_start ps_len`,
        `pam_pos p...` (none: no PAM letter is looked at), `pair j g s w` (j the 0-based READ position, g the guide's letter, s
        the site's letter in read orientation), `pam LETTERS w` (one letter per PAM position, '-' when there is none); '#'
        starts a comment.  `shape` comes first.  pair[j][b][b] is 1 and is not written; every other entry must be there."""
        with open(path) as fh:
            return cls._from_lines(path, enumerate(fh, 1))

    @classmethod
    def _from_lines(cls, path, numbered):
        """from_tsv over (line number, line) pairs of the file `path` (BulgeTable.from_tsv hands over the lines that are not its own)."""
        shape, pam_pos, pair, pam = None, (), None, None
        for n, line in numbered:
            f = line.split("#", 1)[0].split()
            if not f:
                continue
            where = "%s:%d" % (path, n)
            try:
                key, a = f[0], f[1:]
                if key != "shape" and shape is None:
                    raise ValueError("'%s' before the 'shape' line" % key)
                if key == "shape" and len(a) == 3 and shape is None:
                    shape = tuple(int(v) for v in a)
                    if not 0 < shape[2] <= 32:
                        raise ValueError("the protospacer has 1..32 positions")
                    pair = np.full((shape[2], 4, 4), np.nan)
                    for b in range(4):
                        pair[:, b, b] = 1.0
                    pam = np.full(1, np.nan)
                elif key == "pam_pos" and len(a) <= 4 and not pam_pos and np.isnan(pam).all():
                    pam_pos = tuple(int(v) for v in a)
                    pam = np.full(4 ** len(pam_pos), np.nan)
                elif key == "pair" and len(a) == 4:
                    i = int(a[0]) - shape[1]
                    if not 0 <= i < shape[2]:
                        raise ValueError("position %s lies outside the protospacer" % a[0])
                    pair[i, _base(a[1], where), _base(a[2], where)] = float(a[3])
                elif key == "pam" and len(a) == 2:
                    letters = "" if a[0] == "-" else a[0]
                    if len(letters) != len(pam_pos):
                        raise ValueError("'pam' takes one letter per PAM position")
                    k = 0
                    for ch in letters:
                        k = 4 * k + _base(ch, where)
                    pam[k] = float(a[1])
                else:
                    raise ValueError("unknown key, a line given twice or wrong number of fields: %r" % " ".join(f))
            except ValueError as e:
                raise ValueError(str(e) if str(e).startswith(where) else "%s: %s" % (where, e)) from None
        if shape is None:
            raise ValueError("%s: no 'shape' line" % path)
        missing = int(np.isnan(pair).sum() + np.isnan(pam).sum())
        if missing:
            raise ValueError("%s: %d entries are missing" % (path, missing))
        return cls(shape[0], (shape[1], shape[2]), pair, pam_pos, pam)

    def to_tsv(self, path):
        """The table as a text file from_tsv reads back to the bit: the weights as repr() prints them."""
        with open(path, "w") as fh:
            fh.write("# pattern score table: %d letters, protospacer at %d + %d, read orientation\n"
                     % (self.length, self.protospacer[0], self.protospacer[1]))
            fh.write("shape\t%d\t%d\t%d\n" % (self.length, self.protospacer[0], self.protospacer[1]))
            fh.write("pam_pos%s\n" % "".join("\t%d" % q for q in self.pam_positions))
            for i in range(self.protospacer[1]):
                for g in range(4):
                    for b in range(4):
                        if g != b:
                            fh.write("pair\t%d\t%s\t%s\t%r\n" % (self.protospacer[0] + i, "ACGT"[g], "ACGT"[b], float(self.pair[i, g, b])))
            n = len(self.pam_positions)
            for k in range(4 ** n):
                letters = "".join("ACGT"[(k >> (2 * (n - 1 - t))) & 3] for t in range(n)) or "-"
                fh.write("pam\t%s\t%r\n" % (letters, float(self.pam[k])))

    def info(self):
        st = _lib.PatternTableStats()
        check(lib().vsc_pattern_table_info(self._h, C.byref(st)))
        return {"serial": int(st.serial), "zero_weights": int(st.zero_weights), "length": int(st.shape.len),
                "protospacer": (int(st.shape.ps_start), int(st.shape.ps_len)),
                "pam_positions": tuple(int(st.shape.pam_pos[t]) for t in range(st.shape.n_pam))}

    def score(self, guide, site, fixed=False):
        """vsc_pattern_table_score: the score of one guide (IUPAC letters) against one site (ACGT, read orientation), both of
        the table's length; fixed=True: (score, rint(score * 2^30))."""
        g = guide if isinstance(guide, bytes) else guide.encode()
        t = site if isinstance(site, bytes) else site.encode()
        if len(g) != self.length or len(t) != self.length:
            raise ValueError("guide and site have the table's %d letters" % self.length)
        x, f = C.c_double(), C.c_uint32()
        check(lib().vsc_pattern_table_score(self._h, g, t, C.byref(x), C.byref(f)))
        return (x.value, f.value) if fixed else x.value

    def close(self):
        if getattr(self, "_h", None):
            lib().vsc_pattern_table_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


SITE_SCORE_DTYPE = _lib.SITE_SCORE_DTYPE


class BulgeTable:
    """A table score for bulged alignments and cut sites (vsc_bulge_table): a PatternTable (or a ScoreTable, taken as
    PatternTable.from_score_table takes it) for the paired positions plus dna[ps_len][4] - the weight of one unpaired SITE base
    s (read orientation, A 0 C 1 G 2 T 3) when the bulge lies in front of read position ps_start + i - and rna[ps_len][4] - the
    weight of the unpaired GUIDE base g at read position ps_start + i.  Every weight in [0, 1]; the protospacer has at least
    four positions.  The base's weights are copied: the BulgeTable does not need it afterwards.  The package ships no table."""

    def __init__(self, base, dna, rna):
        own = isinstance(base, ScoreTable)
        pt = PatternTable.from_score_table(base) if own else base
        try:
            self.length, self.protospacer, self.pam_positions = pt.length, pt.protospacer, pt.pam_positions
            self.pair, self.pam = pt.pair.copy(), pt.pam.copy()
            self.dna = np.ascontiguousarray(dna, dtype=np.float64)
            self.rna = np.ascontiguousarray(rna, dtype=np.float64)
            if self.dna.shape != (self.protospacer[1], 4) or self.rna.shape != (self.protospacer[1], 4):
                raise ValueError("a bulge table is dna[ps_len][4] and rna[ps_len][4]")
            h = C.c_void_p()
            self._h = None
            check(lib().vsc_bulge_table_build(pt._h, ptr(self.dna), ptr(self.rna), C.byref(h)))
            self._h = h
        finally:
            if own:
                pt.close()

    @classmethod
    def from_tsv(cls, path, base_path=None):
        """A table from the text file to_tsv writes: the pattern table's file format (PatternTable.from_tsv) plus lines
        `dna j s w` and `rna j g w`, j the 0-based READ position, s / g a letter of ACGT; '#' starts a comment.  Every entry
        of both arrays must be there.  base_path: the pattern table's lines are in that file and `path` holds the dna and rna
        lines alone (what the tools take as -W and -w)."""
        lines, extra = [], []
        with open(path) as fh:
            for n, line in enumerate(fh, 1):
                f = line.split("#", 1)[0].split()
                (extra if f and f[0] in ("dna", "rna") else lines).append((n, line, f))
        if base_path is None:
            base = PatternTable._from_lines(path, ((n, line) for n, line, _ in lines))
        else:
            for n, _, f in lines:
                if f:
                    raise ValueError("%s:%d: unknown key %r (only 'dna' and 'rna' lines)" % (path, n, f[0]))
            base = PatternTable.from_tsv(base_path)
        try:
            a, k = base.protospacer
            arr = {"dna": np.full((k, 4), np.nan), "rna": np.full((k, 4), np.nan)}
            for n, _, f in extra:
                where = "%s:%d" % (path, n)
                try:
                    if len(f) != 4:
                        raise ValueError("'%s' takes a position, a letter and a weight" % f[0])
                    i = int(f[1]) - a
                    if not 0 <= i < k:
                        raise ValueError("position %s lies outside the protospacer" % f[1])
                    b = _base(f[2], where)
                    if not np.isnan(arr[f[0]][i, b]):
                        raise ValueError("a line given twice: %r" % " ".join(f))
                    arr[f[0]][i, b] = float(f[3])
                except ValueError as e:
                    raise ValueError(str(e) if str(e).startswith(where) else "%s: %s" % (where, e)) from None
            missing = int(np.isnan(arr["dna"]).sum() + np.isnan(arr["rna"]).sum())
            if missing:
                raise ValueError("%s: %d entries are missing" % (path, missing))
            return cls(base, arr["dna"], arr["rna"])
        finally:
            base.close()

    def to_tsv(self, path, base_path=None):
        """The dna and rna lines as from_tsv reads them back to the bit.  base_path: where the pattern table's lines go (None:
        into the same file, in front)."""
        base = PatternTable(self.length, self.protospacer, self.pair, self.pam_positions, self.pam)
        try:
            base.to_tsv(path if base_path is None else base_path)
        finally:
            base.close()
        with open(path, "a" if base_path is None else "w") as fh:
            fh.write("# bulge weights: dna = an unpaired site base in front of the position, rna = the unpaired guide base at it\n")
            for key, arr in (("dna", self.dna), ("rna", self.rna)):
                for i in range(self.protospacer[1]):
                    for b in range(4):
                        fh.write("%s\t%d\t%s\t%r\n" % (key, self.protospacer[0] + i, "ACGT"[b], float(arr[i, b])))

    def info(self):
        st = _lib.BulgeTableStats()
        check(lib().vsc_bulge_table_info(self._h, C.byref(st)))
        return {"serial": int(st.serial), "zero_weights": int(st.zero_weights), "length": int(st.shape.len),
                "protospacer": (int(st.shape.ps_start), int(st.shape.ps_len)),
                "pam_positions": tuple(int(st.shape.pam_pos[t]) for t in range(st.shape.n_pam))}

    def score(self, guide, site, d, fixed=False):
        """vsc_bulge_table_score: one guide (IUPAC letters, the table's length) against one site of length + d letters (ACGT,
        read orientation), d in -2 .. 2; the split point is the smallest that reaches NM.  Returns (nm, index, score), with
        fixed=True (nm, index, score, rint(score * 2^30)); d = 0: the plain score, index 0."""
        g = guide if isinstance(guide, bytes) else guide.encode()
        t = site if isinstance(site, bytes) else site.encode()
        if len(g) != self.length or len(t) != self.length + int(d):
            raise ValueError("the guide has the table's %d letters, the site d more" % self.length)
        nm, index, x, f = C.c_uint32(), C.c_uint32(), C.c_double(), C.c_uint32()
        check(lib().vsc_bulge_table_score(self._h, g, t, int(d), C.byref(nm), C.byref(index), C.byref(x), C.byref(f)))
        return (nm.value, index.value, x.value, f.value) if fixed else (nm.value, index.value, x.value)

    def close(self):
        if getattr(self, "_h", None):
            lib().vsc_bulge_table_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


EFF_UNDEFINED_BITS = 0x7FF8000000000000  # the one NaN an undefined efficiency predictor is


class EfficiencyModel:
    """An on-target efficiency model (vsc_eff_model): a linear predictor over the context of a site - `up` bases in front of
    it, its site_len bases, `down` bases behind it, C = up + site_len + down, in READ orientation - that is
    intercept + sum_j mono[j][b_j] + sum_j di[j][4 b_j + b_{j+1}] + gc[G/C count of gc_range], bases A 0, C 1, G 2, T 3, added
    in exactly that order (include/varscot_hip.h "LINEAR").  mono is [C][4], di [C - 1][16], gc [gc_range[1] + 1] with
    gc_range = (start, length) in context coordinates (both None: no G/C term).  link: "identity" or "logistic" - the link is
    applied on the host by link(); every device call works in the linear domain.  The package ships no model."""

    LINKS = {"identity": _lib.EFF_IDENTITY, "logistic": _lib.EFF_LOGISTIC}

    def __init__(self, up, site_len, down, intercept, mono, di, gc=None, gc_range=None, link="identity", shape=None):
        """shape: an EffShape to pass as it is (tests)."""
        if link not in self.LINKS:
            raise ValueError("link must be 'identity' or 'logistic'")
        if (gc is None) != (gc_range is None) and shape is None:
            raise ValueError("gc and gc_range come together")
        self.up, self.site_len, self.down, self.link_name = int(up), int(site_len), int(down), link
        self.intercept = float(intercept)
        self.mono = np.ascontiguousarray(mono, dtype=np.float64)
        self.di = np.ascontiguousarray(di, dtype=np.float64)
        self.gc = None if gc is None else np.ascontiguousarray(gc, dtype=np.float64).reshape(-1)
        self.gc_range = None if gc_range is None else (int(gc_range[0]), int(gc_range[1]))
        self._h = None
        if shape is None:
            fields = (self.up, self.site_len, self.down) + (self.gc_range or (0, 0))
            if any(not 0 <= v < 2 ** 32 for v in fields):
                raise ValueError("the shape's fields must fit 32 unsigned bits")
            C_ = self.context_len
            if self.mono.shape != (C_, 4) or self.di.shape != (max(C_ - 1, 0), 16) or \
                    (self.gc is not None and len(self.gc) != self.gc_range[1] + 1):
                raise ValueError("an efficiency model of context length %d is mono[%d][4], di[%d][16] and gc[gc_len + 1]" % (C_, C_, C_ - 1))
            shape = _lib.EffShape(self.up, self.site_len, self.down, fields[3], fields[4], self.LINKS[link])
        h = C.c_void_p()
        check(lib().vsc_eff_model_build(C.byref(shape), self.intercept, ptr(self.mono), ptr(self.di), ptr(self.gc), C.byref(h)))
        self._h = h

    @property
    def context_len(self):
        return self.up + self.site_len + self.down

    @classmethod
    def from_features(cls, up, site_len, down, intercept, features, gc=None, gc_range=None, link="identity"):
        """A model from a parameter list as the papers print it: (pos, letters, weight) triples - pos 0-based in context
        coordinates, letters one base (mono) or two (the dinucleotide that starts at pos).  What the list does not name
        weighs 0; a feature named twice is an error."""
        C_ = int(up) + int(site_len) + int(down)
        mono, di = np.zeros((C_, 4)), np.zeros((max(C_ - 1, 0), 16))
        seen = set()
        for pos, letters, weight in features:
            pos, key = int(pos), (int(pos), letters.upper().replace("U", "T"))
            if key in seen:
                raise ValueError("feature (%d, %r) is given twice" % (pos, letters))
            seen.add(key)
            if len(letters) not in (1, 2) or not 0 <= pos <= C_ - len(letters):
                raise ValueError("feature (%d, %r): one or two letters that lie inside the context of %d" % (pos, letters, C_))
            b = [_base(ch, "feature (%d, %r)" % (pos, letters)) for ch in letters]
            if len(b) == 1:
                mono[pos, b[0]] = float(weight)
            else:
                di[pos, 4 * b[0] + b[1]] = float(weight)
        return cls(up, site_len, down, intercept, mono, di, gc=gc, gc_range=gc_range, link=link)

    @classmethod
    def from_tsv(cls, path):
        """A model from the text file to_tsv writes (tools/README.md): tab- or blank-separated lines `shape up site_len down`,
        `link identity|logistic`, `intercept x`, `gc_range start length`, `mono pos X w`, `di pos XY w`, `gc count w`; '#'
        starts a comment.  `shape` comes before every weight, `gc_range` before every `gc`.  What the file does not name
        weighs 0.  An unknown key, a weight before its shape, a line given twice and anything that does not parse are
        refused with the line number."""
        shape = gc_range = None
        intercept, link, feats, gc_w = 0.0, "identity", [], {}
        once = set()
        with open(path) as fh:
            for n, line in enumerate(fh, 1):
                f = line.split("#", 1)[0].split()
                if not f:
                    continue
                where = "%s:%d" % (path, n)
                try:
                    key, a = f[0], f[1:]
                    if key in ("shape", "link", "intercept", "gc_range"):
                        if key in once:
                            raise ValueError("'%s' is given twice" % key)
                        once.add(key)
                    if key in ("mono", "di", "gc") and shape is None:
                        raise ValueError("'%s' before the 'shape' line" % key)
                    if key == "shape" and len(a) == 3:
                        shape = tuple(int(v) for v in a)
                    elif key == "link" and len(a) == 1:
                        if a[0] not in cls.LINKS:
                            raise ValueError("link must be 'identity' or 'logistic'")
                        link = a[0]
                    elif key == "intercept" and len(a) == 1:
                        intercept = float(a[0])
                    elif key == "gc_range" and len(a) == 2:
                        gc_range = (int(a[0]), int(a[1]))
                    elif key in ("mono", "di") and len(a) == 3:
                        if len(a[1]) != (1 if key == "mono" else 2):
                            raise ValueError("'%s' takes %s" % (key, "one letter" if key == "mono" else "two letters"))
                        if (int(a[0]), a[1].upper()) in once:
                            raise ValueError("feature (%s, %s) is given twice" % (a[0], a[1]))
                        once.add((int(a[0]), a[1].upper()))
                        if not 0 <= int(a[0]) <= sum(shape) - len(a[1]):
                            raise ValueError("position %s lies outside the context of %d" % (a[0], sum(shape)))
                        for ch in a[1]:
                            _base(ch, where)
                        feats.append((int(a[0]), a[1], float(a[2])))
                    elif key == "gc" and len(a) == 2:
                        if gc_range is None:
                            raise ValueError("'gc' before the 'gc_range' line")
                        if int(a[0]) in gc_w or not 0 <= int(a[0]) <= gc_range[1]:
                            raise ValueError("G/C count %s is given twice or lies outside 0..%d" % (a[0], gc_range[1]))
                        gc_w[int(a[0])] = float(a[1])
                    else:
                        raise ValueError("unknown key or wrong number of fields: %r" % " ".join(f))
                except ValueError as e:
                    raise ValueError(str(e) if str(e).startswith(where) else "%s: %s" % (where, e)) from None
        if shape is None:
            raise ValueError("%s: no 'shape' line" % path)
        gc = None if gc_range is None else [gc_w.get(k, 0.0) for k in range(gc_range[1] + 1)]
        return cls.from_features(shape[0], shape[1], shape[2], intercept, feats, gc=gc, gc_range=gc_range, link=link)

    def to_tsv(self, path):
        """The model as a text file from_tsv reads back to the bit: the weights that are not 0, as repr() prints them."""
        with open(path, "w") as fh:
            fh.write("# on-target efficiency model: context = %d upstream + %d site + %d downstream bases, read orientation\n"
                     % (self.up, self.site_len, self.down))
            fh.write("shape\t%d\t%d\t%d\nlink\t%s\nintercept\t%r\n" % (self.up, self.site_len, self.down, self.link_name, self.intercept))
            if self.gc_range is not None:
                fh.write("gc_range\t%d\t%d\n" % self.gc_range)
            for j, b in zip(*np.nonzero(self.mono)):
                fh.write("mono\t%d\t%s\t%r\n" % (j, "ACGT"[b], float(self.mono[j, b])))
            for j, d in zip(*np.nonzero(self.di)):
                fh.write("di\t%d\t%s%s\t%r\n" % (j, "ACGT"[d // 4], "ACGT"[d % 4], float(self.di[j, d])))
            if self.gc is not None:
                for k in np.nonzero(self.gc)[0]:
                    fh.write("gc\t%d\t%r\n" % (k, float(self.gc[k])))

    def info(self):
        st = _lib.EffModelStats()
        check(lib().vsc_eff_model_info(self._h, C.byref(st)))
        s = st.shape
        return {"serial": int(st.serial), "up": int(s.up), "site_len": int(s.site_len), "down": int(s.down), "gc_start": int(s.gc_start),
                "gc_len": int(s.gc_len), "link": {v: k for k, v in self.LINKS.items()}[int(s.link)],
                "nonzero_weights": int(st.nonzero_weights)}

    def score_text(self, context):
        """vsc_eff_score_text: the linear predictor of one context of C letters in read orientation, on the host by the
        function the kernels run; a letter outside ACGT gives the undefined NaN.  No device is needed."""
        b = context if isinstance(context, bytes) else context.encode()
        x = C.c_double()
        check(lib().vsc_eff_score_text(self._h, b, C.byref(x)))
        return x.value

    def link(self, x):
        """vsc_eff_link: a linear predictor (or an array of them) through the model's link, on the host."""
        L = lib()
        if np.ndim(x) == 0:
            return L.vsc_eff_link(self._h, float(x))
        a = np.asarray(x, dtype=np.float64)
        return np.array([L.vsc_eff_link(self._h, float(v)) for v in a.reshape(-1)], dtype=np.float64).reshape(a.shape)

    def close(self):
        if getattr(self, "_h", None):
            lib().vsc_eff_model_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _letter_mask(letters, width, what):
    """The mask of a BASE test (width 1: a string of letters, bit b per letter) or of a PAIR test (width 2: a list of
    two-letter strings, or one string of them separated by commas; bit 4 b_a + b_b per dinucleotide).  "" / "-" / []: no bit."""
    if isinstance(letters, str):
        items = [] if letters in ("", "-") else (list(letters) if width == 1 else letters.split(","))
    else:
        items = list(letters)
    mask = 0
    for it in items:
        if not isinstance(it, str) or len(it) != width:
            raise ValueError("%s: %r is no %s" % (what, it, "base" if width == 1 else "dinucleotide"))
        code = 0
        for ch in it:
            code = 4 * code + _base(ch, what)
        if mask >> code & 1:
            raise ValueError("%s: %r is given twice" % (what, it))
        mask |= 1 << code
    return mask


def _mask_letters(mask, width):
    """The inverse of _letter_mask, as to_tsv writes it."""
    if width == 1:
        return "".join("ACGT"[b] for b in range(4) if mask >> b & 1) or "-"
    return ",".join("ACGT"[d // 4] + "ACGT"[d % 4] for d in range(16) if mask >> d & 1) or "-"


class TreeEfficiencyModel:
    """An on-target efficiency model that is a sum of regression trees (vsc_eff_trees; include/varscot_hip.h "SUMS / TREES /
    PREDICTOR"): x = base + the value of the leaf the context reaches in tree 0, + ... in tree 1, and so on, in this order -
    the form of Doench 2016 "Rule Set 2" and of a scikit-learn GradientBoostingRegressor (from_sklearn).  The context is the
    linear model's: `up` bases in front of the site, its site_len bases, `down` behind, read orientation.
      sums   [(start, length, {letters: int weight})]: S_i = the weights of the letters ("G") and dinucleotides ("GC") inside
             context range [start, start + length), added up - a G/C count is {"G": 1, "C": 1}.
      trees  a list of node lists; a tree's nodes are numbered from 0 (the root) and a node's children have larger numbers:
             ("leaf", v), ("base", pos, "AG", left, right) - true iff the letter at pos is one of these -,
             ("pair", a, b, ["AG", "CC"], left, right) - true iff the letters at a and b are one of these pairs -,
             ("sum", i, t, left, right) - true iff S_i <= t.  True goes left.
    link: "identity" or "logistic", applied on the host by link().  The package ships no model."""

    LINKS = EfficiencyModel.LINKS
    KINDS = {"leaf": _lib.EFF_NODE_LEAF, "base": _lib.EFF_NODE_BASE, "pair": _lib.EFF_NODE_PAIR, "sum": _lib.EFF_NODE_SUM}

    def __init__(self, up, site_len, down, base, sums, trees, link="identity"):
        if link not in self.LINKS:
            raise ValueError("link must be 'identity' or 'logistic'")
        self.up, self.site_len, self.down, self.link_name = int(up), int(site_len), int(down), link
        if any(not 0 <= v < 2 ** 32 for v in (self.up, self.site_len, self.down)):
            raise ValueError("the shape's fields must fit 32 unsigned bits")
        self.base = float(base)
        self.sums = [(int(s), int(n), {str(k).upper().replace("U", "T"): int(w) for k, w in dict(wts).items()}) for s, n, wts in sums]
        self.trees = [[tuple(node) for node in tree] for tree in trees]
        self._h = None
        i32 = lambda v, what: self._int(v, -2 ** 31, 2 ** 31 - 1, what)  # noqa: E731
        u32 = lambda v, what: self._int(v, 0, 2 ** 32 - 1, what)        # noqa: E731
        sum_arr = np.zeros(len(self.sums), dtype=_lib.EFF_SUM_DTYPE)
        for i, (start, length, wts) in enumerate(self.sums):
            sum_arr[i]["start"], sum_arr[i]["len"] = u32(start, "sum %d" % i), u32(length, "sum %d" % i)
            for letters, w in wts.items():
                what = "sum %d, weight %r" % (i, letters)
                if len(letters) not in (1, 2):
                    raise ValueError("%s: one letter or two" % what)
                code = 0
                for ch in letters:
                    code = 4 * code + _base(ch, what)
                sum_arr[i]["mono" if len(letters) == 1 else "di"][code] = i32(w, what)
        first = np.zeros(len(self.trees) + 1, dtype=np.uint32)
        first[1:] = np.cumsum([len(t) for t in self.trees])
        nodes = np.zeros(int(first[-1]), dtype=_lib.EFF_NODE_DTYPE)
        at = 0
        for t, tree in enumerate(self.trees):
            for k, node in enumerate(tree):
                what = "tree %d, node %d" % (t, k)
                n = nodes[at]
                at += 1
                kind = node[0] if len(node) else None
                if kind not in self.KINDS or len(node) != {"leaf": 2, "base": 5, "pair": 6, "sum": 5}[kind]:
                    raise ValueError("%s: %r is no node" % (what, node))
                n["kind"] = self.KINDS[kind]
                if kind == "leaf":
                    n["value"] = float(node[1])
                    continue
                n["left"], n["right"] = u32(node[-2], what), u32(node[-1], what)
                if kind == "base":
                    n["a"], n["mask"] = u32(node[1], what), _letter_mask(node[2], 1, what)
                elif kind == "pair":
                    n["a"], n["b"], n["mask"] = u32(node[1], what), u32(node[2], what), _letter_mask(node[3], 2, what)
                else:
                    n["a"], n["t"] = u32(node[1], what), i32(node[2], what)
        shape = _lib.EffShape(self.up, self.site_len, self.down, 0, 0, self.LINKS[link])
        h = C.c_void_p()
        check(lib().vsc_eff_trees_build(C.byref(shape), self.base, ptr(sum_arr) if len(sum_arr) else None, len(sum_arr),
                                        ptr(nodes) if len(nodes) else None, ptr(first), len(self.trees), C.byref(h)))
        self._h = h

    @staticmethod
    def _int(v, lo, hi, what):
        if int(v) != v or not lo <= int(v) <= hi:
            raise ValueError("%s: %r is no integer in %d .. %d" % (what, v, lo, hi))
        return int(v)

    @property
    def context_len(self):
        return self.up + self.site_len + self.down

    @classmethod
    def from_sklearn(cls, estimator, features, up, site_len, down, sums=(), link="identity"):
        """The model of a fitted scikit-learn GradientBoostingRegressor (squared error; its constant init or init="zero").
        features[k] says what column k of the training matrix was: ("base", pos, "A") - 1 where the letter at pos is A, else 0 -,
        ("pair", a, b, "AG") - 1 where the letters at a and b are A and G -, or ("sum", i) - S_i of `sums`.  A split x <= thr on
        an indicator becomes the complement mask (a constant mask when thr lies outside [0, 1)), a split on a sum
        S_i <= floor(thr); the leaves are learning_rate * value, the base is the init's constant: score_text then equals
        estimator.predict to the bit.  Every other estimator is refused."""
        name = type(estimator).__name__
        if name != "GradientBoostingRegressor" or not type(estimator).__module__.startswith("sklearn."):
            raise ValueError("from_sklearn takes a fitted sklearn GradientBoostingRegressor, not a %s" % name)
        if not hasattr(estimator, "estimators_"):
            raise ValueError("the estimator is not fitted")
        if getattr(estimator, "loss", None) != "squared_error":
            raise ValueError("from_sklearn takes the squared_error loss only, not %r" % (getattr(estimator, "loss", None),))
        if isinstance(estimator.init, str) and estimator.init == "zero":
            base = 0.0
        elif estimator.init is None and type(estimator.init_).__name__ == "DummyRegressor":
            base = float(np.asarray(estimator.init_.constant_, dtype=np.float64).reshape(-1)[0])
        else:
            raise ValueError("from_sklearn takes the estimator's constant init or init='zero'")
        if len(features) != estimator.n_features_in_:
            raise ValueError("the estimator has %d columns, features names %d" % (estimator.n_features_in_, len(features)))
        rate = float(estimator.learning_rate)
        trees = []
        for stage in estimator.estimators_[:, 0]:
            tr = stage.tree_
            left, right, feat, thr, value = tr.children_left, tr.children_right, tr.feature, tr.threshold, tr.value
            order, stack = [], [0]  # preorder: a child's new number is larger than its parent's
            while stack:
                k = stack.pop()
                order.append(k)
                if left[k] >= 0:
                    stack += [int(right[k]), int(left[k])]
            new = {k: i for i, k in enumerate(order)}
            nodes = []
            for k in order:
                if left[k] < 0:
                    nodes.append(("leaf", rate * float(value[k, 0, 0])))
                    continue
                f, x, lr = features[int(feat[k])], float(thr[k]), (new[int(left[k])], new[int(right[k])])
                if f[0] == "sum" and len(f) == 2:
                    nodes.append(("sum", int(f[1]), int(min(max(math.floor(x), -2 ** 31), 2 ** 31 - 1))) + lr)
                elif f[0] in ("base", "pair") and len(f) == (3 if f[0] == "base" else 4):
                    width = 1 if f[0] == "base" else 2
                    full = 0xF if width == 1 else 0xFFFF
                    one = _letter_mask([f[-1]], width, "feature %r" % (f,))
                    mask = full if x >= 1.0 else 0 if x < 0.0 else full & ~one  # x_k <= thr, x_k 0 or 1
                    text = _mask_letters(mask, width)
                    nodes.append((f[0],) + tuple(int(p) for p in f[1:-1]) + (text if width == 1 else [] if text == "-" else text.split(","),) + lr)
                else:
                    raise ValueError("feature %r is none of ('base', pos, X), ('pair', a, b, XY), ('sum', i)" % (f,))
            trees.append(nodes)
        return cls(up, site_len, down, base, sums, trees, link=link)

    @classmethod
    def from_tsv(cls, path):
        """A model from the text file to_tsv writes (tools/README.md): `shape up site_len down`, `link identity|logistic`,
        `intercept x` (the base), `sum I START LENGTH`, `sumw I X|XY W`, `tree T`, `leaf K V`, `base_in K POS LETTERS L R`,
        `pair_in K POSA POSB XY[,XY...] L R`, `sum_le K I T L R`; '-' is the empty set of letters, '#' starts a comment.  I, T
        and K ascend from 0; a node belongs to the last `tree` line.  Anything that does not parse, a key given twice, an
        index out of turn and a `mono` / `di` / `gc` line are refused with the line number."""
        shape = None
        base, link, sums, trees = 0.0, "identity", [], []
        once = set()
        with open(path) as fh:
            for n, line in enumerate(fh, 1):
                f = line.split("#", 1)[0].split()
                if not f:
                    continue
                where = "%s:%d" % (path, n)
                try:
                    key, a = f[0], f[1:]
                    if key in ("shape", "link", "intercept"):
                        if key in once:
                            raise ValueError("'%s' is given twice" % key)
                        once.add(key)
                    if key in ("mono", "di", "gc", "gc_range"):
                        raise ValueError("'%s' belongs to a linear model; this file holds a tree model" % key)
                    if key in ("leaf", "base_in", "pair_in", "sum_le"):
                        if not trees:
                            raise ValueError("'%s' before the first 'tree' line" % key)
                        if len(a) < 1 or int(a[0]) != len(trees[-1]):
                            raise ValueError("node %s out of turn: node %d of tree %d comes next" % (a[0] if a else "?", len(trees[-1]), len(trees) - 1))
                    if key == "shape" and len(a) == 3:
                        shape = tuple(int(v) for v in a)
                    elif key == "link" and len(a) == 1:
                        if a[0] not in cls.LINKS:
                            raise ValueError("link must be 'identity' or 'logistic'")
                        link = a[0]
                    elif key == "intercept" and len(a) == 1:
                        base = float(a[0])
                    elif key == "sum" and len(a) == 3:
                        if int(a[0]) != len(sums):
                            raise ValueError("sum %s out of turn: sum %d comes next" % (a[0], len(sums)))
                        sums.append((int(a[1]), int(a[2]), {}))
                    elif key == "sumw" and len(a) == 3:
                        if not 0 <= int(a[0]) < len(sums):
                            raise ValueError("'sumw' before its 'sum %s' line" % a[0])
                        letters = a[1].upper().replace("U", "T")
                        if len(letters) not in (1, 2):
                            raise ValueError("'sumw' takes one letter or two")
                        for ch in letters:
                            _base(ch, where)
                        if letters in sums[int(a[0])][2]:
                            raise ValueError("weight %s of sum %s is given twice" % (a[1], a[0]))
                        sums[int(a[0])][2][letters] = int(a[2])
                    elif key == "tree" and len(a) == 1:
                        if int(a[0]) != len(trees):
                            raise ValueError("tree %s out of turn: tree %d comes next" % (a[0], len(trees)))
                        if trees and not trees[-1]:
                            raise ValueError("tree %d has no node" % (len(trees) - 1))
                        trees.append([])
                    elif key == "leaf" and len(a) == 2:
                        trees[-1].append(("leaf", float(a[1])))
                    elif key == "base_in" and len(a) == 5:
                        _letter_mask(a[2], 1, where)
                        trees[-1].append(("base", int(a[1]), a[2], int(a[3]), int(a[4])))
                    elif key == "pair_in" and len(a) == 6:
                        _letter_mask(a[3], 2, where)
                        trees[-1].append(("pair", int(a[1]), int(a[2]), a[3], int(a[4]), int(a[5])))
                    elif key == "sum_le" and len(a) == 5:
                        trees[-1].append(("sum", int(a[1]), int(a[2]), int(a[3]), int(a[4])))
                    else:
                        raise ValueError("unknown key or wrong number of fields: %r" % " ".join(f))
                except ValueError as e:
                    raise ValueError(str(e) if str(e).startswith(where) else "%s: %s" % (where, e)) from None
        if shape is None:
            raise ValueError("%s: no 'shape' line" % path)
        if not trees:
            raise ValueError("%s: no 'tree' line" % path)
        return cls(shape[0], shape[1], shape[2], base, sums, trees, link=link)

    def to_tsv(self, path):
        """The model as a text file from_tsv reads back to the bit: doubles as repr() prints them."""
        with open(path, "w") as fh:
            fh.write("# on-target efficiency model (regression trees): context = %d upstream + %d site + %d downstream bases, read orientation\n"
                     % (self.up, self.site_len, self.down))
            fh.write("shape\t%d\t%d\t%d\nlink\t%s\nintercept\t%r\n" % (self.up, self.site_len, self.down, self.link_name, self.base))
            for i, (start, length, wts) in enumerate(self.sums):
                fh.write("sum\t%d\t%d\t%d\n" % (i, start, length))
                for letters, w in wts.items():
                    fh.write("sumw\t%d\t%s\t%d\n" % (i, letters, w))
            for t, tree in enumerate(self.trees):
                fh.write("tree\t%d\n" % t)
                for k, node in enumerate(tree):
                    if node[0] == "leaf":
                        fh.write("leaf\t%d\t%r\n" % (k, float(node[1])))
                    elif node[0] == "base":
                        fh.write("base_in\t%d\t%d\t%s\t%d\t%d\n" % (k, node[1], _mask_letters(_letter_mask(node[2], 1, "node"), 1), node[3], node[4]))
                    elif node[0] == "pair":
                        fh.write("pair_in\t%d\t%d\t%d\t%s\t%d\t%d\n"
                                 % (k, node[1], node[2], _mask_letters(_letter_mask(node[3], 2, "node"), 2), node[4], node[5]))
                    else:
                        fh.write("sum_le\t%d\t%d\t%d\t%d\t%d\n" % (k, node[1], node[2], node[3], node[4]))

    def info(self):
        st = _lib.EffTreesStats()
        check(lib().vsc_eff_trees_info(self._h, C.byref(st)))
        s = st.shape
        return {"serial": int(st.serial), "up": int(s.up), "site_len": int(s.site_len), "down": int(s.down),
                "link": {v: k for k, v in self.LINKS.items()}[int(s.link)], "n_sums": int(st.n_sums), "n_trees": int(st.n_trees),
                "n_nodes": int(st.n_nodes), "leaves": int(st.leaves), "base_nodes": int(st.base_nodes), "pair_nodes": int(st.pair_nodes),
                "sum_nodes": int(st.sum_nodes), "max_depth": int(st.max_depth)}

    def score_text(self, context):
        """vsc_eff_trees_score_text: the predictor of one context of C letters in read orientation, on the host by the
        functions the kernels run; a letter outside ACGT gives the undefined NaN.  No device is needed."""
        b = context if isinstance(context, bytes) else context.encode()
        x = C.c_double()
        check(lib().vsc_eff_trees_score_text(self._h, b, C.byref(x)))
        return x.value

    def link(self, x):
        """vsc_eff_trees_link: a predictor (or an array of them) through the model's link, on the host."""
        L = lib()
        if np.ndim(x) == 0:
            return L.vsc_eff_trees_link(self._h, float(x))
        a = np.asarray(x, dtype=np.float64)
        return np.array([L.vsc_eff_trees_link(self._h, float(v)) for v in a.reshape(-1)], dtype=np.float64).reshape(a.shape)

    def close(self):
        if getattr(self, "_h", None):
            lib().vsc_eff_trees_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _eff_partial(stats, allow_partial):
    if stats["not_resident"] and not allow_partial:
        raise ValueError("%d candidates have a context that is not resident on this genome object (a shard holds nothing in "
                         "front of its first word); allow_partial=True returns them as undefined" % stats["not_resident"])


MH_UNDEFINED = _lib.MH_UNDEFINED  # sum and oof of a candidate whose microhomology score is undefined


class MicrohomologyShape:
    """vsc_mh_shape: where the microhomology score looks.  site_len 16..32 is the candidates' length (23 for
    enumerate_guides', the pattern's for enumerate_pattern's), cut 0..site_len says that the break lies between read positions
    cut - 1 and cut of the site (SpCas9: 17; Cas12a TTTV + 23: 22), flank 8..32 is the number of bases taken on either side
    of the break.  validate=False passes the numbers to the library as they are (tests)."""

    def __init__(self, site_len=READ_LEN, cut=17, flank=30, validate=True):
        self.site_len, self.cut, self.flank = int(site_len), int(cut), int(flank)
        if validate and not (16 <= self.site_len <= 32 and 0 <= self.cut <= self.site_len and 8 <= self.flank <= 32):
            raise ValueError("a microhomology shape has site_len 16..32, cut 0..site_len and flank 8..32")

    def _struct(self):
        return _lib.MhShape(self.site_len, self.cut, self.flank, 0)

    def __repr__(self):
        return "MicrohomologyShape(site_len=%d, cut=%d, flank=%d)" % (self.site_len, self.cut, self.flank)


def microhomology_text(context, flank=None):
    """vsc_mh_score_text: (sum, oof) of one context of 2 * flank letters (any case) in read orientation - the break in its
    middle - on the host, by the function the kernels call.  sum is the microhomology score in tenths, oof the part of it whose
    deletion length is no multiple of three; a non-ACGT letter gives (MH_UNDEFINED, MH_UNDEFINED).  flank=None: half the
    text's length."""
    b = context if isinstance(context, bytes) else context.encode()
    if flank is None:
        if len(b) % 2:
            raise ValueError("a microhomology context has an even number of letters")
        flank = len(b) // 2
    s, o = C.c_uint32(), C.c_uint32()
    check(lib().vsc_mh_score_text(b, int(flank), C.byref(s), C.byref(o)))
    return int(s.value), int(o.value)


def microhomology_scores(pairs):
    """vsc_mh_scores: (mhScore, oofScore) float64 arrays for (sum, oof) pairs - sum / 10 and 100 * oof / sum (0 where sum is 0),
    NaN where the pair is undefined.  pairs: one pair or an array of shape (n, 2)."""
    a = np.asarray(pairs, dtype=np.uint32)
    flat = a.reshape(-1, 2)
    mh, oof = np.empty(len(flat), dtype=np.float64), np.empty(len(flat), dtype=np.float64)
    L = lib()
    x, y = C.c_double(), C.c_double()
    for i, (s, o) in enumerate(flat):
        check(L.vsc_mh_scores(int(s), int(o), C.byref(x), C.byref(y)))
        mh[i], oof[i] = x.value, y.value
    if a.ndim == 1:
        return float(mh[0]), float(oof[0])
    return mh, oof


FOLD_UNDEFINED = _lib.FOLD_UNDEFINED  # both words of a candidate whose fold row is undefined
FOLD_NO_LIMIT = _lib.FOLD_NO_LIMIT
FOLD_WOBBLE = _lib.FOLD_WOBBLE
_FOLD_RULE = ("a fold shape has site_len 16..32, a spacer of 12..32 bases inside the site, stem 3..8, gc_min 0..stem, min_loop 0..16, a seed "
              "(start and length 0..16) inside the spacer and no flag but FOLD_WOBBLE")


class FoldShape:
    """vsc_fold_shape: how the self-complementarity of a guide RNA is counted.  site_len 16..32 is the candidates' length (23 for
    enumerate_guides', the pattern's for enumerate_pattern's); spacer = (start, length) in read positions of the site, length
    12..32: the bases that become the guide RNA's spacer; stem 3..8 is the length k of a counted stem, gc_min 0..k the G/C a
    k-mer needs to count, min_loop 0..16 the unpaired bases between the arms of a hairpin; seed = (start, length), each 0..16, in
    SPACER positions (length 0: none); wobble=True counts G-U pairs.  FOLD_SHAPES holds "SpCas9" and "Cas12a": shapes only, the
    scaffold is the caller's.  validate=False passes the numbers to the library as they are (tests)."""

    def __init__(self, site_len=READ_LEN, spacer=(0, 20), stem=4, gc_min=2, min_loop=3, seed=(8, 12), wobble=False, flags=None,
                 validate=True):
        self.site_len, self.proto_start, self.proto_len = int(site_len), int(spacer[0]), int(spacer[1])
        self.stem, self.gc_min, self.min_loop = int(stem), int(gc_min), int(min_loop)
        self.seed_start, self.seed_len = int(seed[0]), int(seed[1])
        self.flags = int(flags) if flags is not None else (FOLD_WOBBLE if wobble else 0)
        self.reserved = (0, 0, 0)
        if validate and not self.valid():
            raise ValueError(_FOLD_RULE)

    def valid(self):
        return (16 <= self.site_len <= 32 and 12 <= self.proto_len <= 32 and 0 <= self.proto_start
                and self.proto_start + self.proto_len <= self.site_len and 3 <= self.stem <= 8 and 0 <= self.gc_min <= self.stem
                and 0 <= self.min_loop <= 16 and 0 <= self.seed_start <= 16 and 0 <= self.seed_len <= 16
                and self.seed_start + self.seed_len <= self.proto_len and self.flags in (0, FOLD_WOBBLE)
                and tuple(self.reserved) == (0, 0, 0))

    def _struct(self):
        s = _lib.FoldShapeStruct(self.site_len, self.proto_start, self.proto_len, self.stem, self.gc_min, self.min_loop,
                                 self.seed_start, self.seed_len, self.flags)
        for i, v in enumerate(self.reserved):
            s.reserved[i] = int(v)
        return s

    def __repr__(self):
        return "FoldShape(site_len=%d, spacer=(%d, %d), stem=%d, gc_min=%d, min_loop=%d, seed=(%d, %d), flags=%d)" % (
            self.site_len, self.proto_start, self.proto_len, self.stem, self.gc_min, self.min_loop, self.seed_start, self.seed_len,
            self.flags)


FOLD_SHAPES = {"SpCas9": FoldShape(23, (0, 20), 4, 2, 3, (8, 12)), "Cas12a": FoldShape(27, (4, 23), 4, 2, 3, (0, 6))}


def _fold_shape(shape, what="shape"):
    if isinstance(shape, str):
        if shape not in FOLD_SHAPES:
            raise ValueError("%s names one of %s, or is a FoldShape" % (what, ", ".join(sorted(FOLD_SHAPES))))
        shape = FOLD_SHAPES[shape]
    if not isinstance(shape, FoldShape):
        raise ValueError("%s must be a FoldShape or the name of a preset" % what)
    return shape


def _fold_scaffold(scaffold, validate=True):
    """The scaffold text of a call as bytes (None: empty).  At most 128 letters of A C G T U, in any case."""
    if scaffold is None:
        return b""
    b = scaffold if isinstance(scaffold, bytes) else str(scaffold).encode()
    if validate and (len(b) > 128 or any(c not in b"ACGTUacgtu" for c in b)):
        raise ValueError("a scaffold has at most 128 letters of A C G T U")
    return b


def _fold_limits(max_starts, max_self, max_scaffold, max_seed):
    """The four limits as integers, once: None is FOLD_NO_LIMIT; a limit is a whole number 0..32."""
    out = []
    for name, v in (("max_fold_starts", max_starts), ("max_fold_self", max_self), ("max_fold_scaffold", max_scaffold),
                    ("max_fold_seed", max_seed)):
        if v is None:
            out.append(FOLD_NO_LIMIT)
            continue
        i = int(v)
        if i != v or not (0 <= i <= 32 or i == FOLD_NO_LIMIT):
            raise ValueError("%s is a whole number 0 .. 32, or None for no limit" % name)
        out.append(i)
    return tuple(out)


def fold_text(spacer, shape, scaffold=None):
    """vsc_fold_text: the row (w0, w1) of one spacer of shape.proto_len letters (A C G T U, any case) against itself and a
    scaffold text, on the host, by the function the kernels call - for a guide list without a genome.  A spacer letter other
    than A C G T U gives (FOLD_UNDEFINED, FOLD_UNDEFINED); unpack_fold_row names the fields."""
    shape = _fold_shape(shape)
    b = spacer if isinstance(spacer, bytes) else spacer.encode()
    sc = _fold_scaffold(scaffold)
    if len(b) != shape.proto_len:
        raise ValueError("the spacer has %d letters, the shape's spacer %d" % (len(b), shape.proto_len))
    sh = shape._struct()
    row = (C.c_uint32 * 2)()
    check(lib().vsc_fold_text(b, len(b), sc, len(sc), C.byref(sh), row))
    return int(row[0]), int(row[1])


def unpack_fold_row(rows):
    """The fields of fold rows (one (w0, w1) pair or an array of shape (n, 2)) as a dict of integer arrays: starts,
    self_starts, scaf_starts, seed_paired, self_longest, scaf_longest, and defined (bool; the other fields of an undefined row
    are 0)."""
    a = np.asarray(rows, dtype=np.uint32)
    flat = a.reshape(-1, 2)
    w0, w1 = flat[:, 0], flat[:, 1]
    defined = ~((w0 == FOLD_UNDEFINED) & (w1 == FOLD_UNDEFINED))
    z = np.uint32(0)
    out = {"starts": np.where(defined, w0 & 0xFF, z), "self_starts": np.where(defined, (w0 >> 8) & 0xFF, z),
           "scaf_starts": np.where(defined, (w0 >> 16) & 0xFF, z), "seed_paired": np.where(defined, w0 >> 24, z),
           "self_longest": np.where(defined, w1 & 0xFF, z), "scaf_longest": np.where(defined, (w1 >> 8) & 0xFF, z),
           "defined": defined}
    if a.ndim == 1:
        return {k: (bool(v[0]) if k == "defined" else int(v[0])) for k, v in out.items()}
    return out


def pack_fold_row(starts, self_starts, scaf_starts, seed_paired, self_longest, scaf_longest):
    """(w0, w1) of the six fields: the inverse of unpack_fold_row on a defined row."""
    return (int(starts) | int(self_starts) << 8 | int(scaf_starts) << 16 | int(seed_paired) << 24,
            int(self_longest) | int(scaf_longest) << 8)


MOTIF_UNDEFINED = _lib.MOTIF_UNDEFINED  # all three words of a candidate whose motif row is undefined
MOTIF_BOTH_STRANDS = _lib.MOTIF_BOTH_STRANDS
MOTIF_CUT_ONLY = _lib.MOTIF_CUT_ONLY
_MOTIF_RULE = ("a motif shape has site_len 16..32, up and down 0..16 with a context of at most 64 bases, a spacer of 12..32 bases inside the "
               "site and a cut zone of 1..16 bases inside the site")
_MOTIF_LETTERS = b"ACGTURYSWKMBDHVNacgturyswkmbdhvn"


class MotifShape:
    """vsc_motif_shape: where motifs are looked for.  site_len 16..32 is the candidates' length (23 for enumerate_guides', the
    pattern's for enumerate_pattern's); up / down 0..16 are the bases of genomic context in front of and behind the site (read
    orientation; the context has at most 64 bases); spacer = (start, length) in read positions of the site, length 12..32: the
    bases that are cloned between the flanks; cut = (start, length) in SITE positions, length 1..16: the cut zone, the positions
    an indel at the cut is expected to change.  MOTIF_SHAPES holds "SpCas9" and "Cas12a" with 16 bases of context a side: shapes
    only, the motifs and the flanks are the caller's.  validate=False passes the numbers to the library as they are (tests)."""

    def __init__(self, site_len=READ_LEN, spacer=(0, 20), cut=(16, 2), up=0, down=0, validate=True):
        self.site_len, self.up, self.down = int(site_len), int(up), int(down)
        self.proto_start, self.proto_len = int(spacer[0]), int(spacer[1])
        self.cut_start, self.cut_len = int(cut[0]), int(cut[1])
        self.reserved = (0, 0, 0, 0, 0)
        if validate and not self.valid():
            raise ValueError(_MOTIF_RULE)

    @property
    def context_len(self):
        return self.up + self.site_len + self.down

    def valid(self):
        return (16 <= self.site_len <= 32 and 0 <= self.up <= 16 and 0 <= self.down <= 16 and self.context_len <= 64
                and 12 <= self.proto_len <= 32 and 0 <= self.proto_start and self.proto_start + self.proto_len <= self.site_len
                and 1 <= self.cut_len <= 16 and 0 <= self.cut_start and self.cut_start + self.cut_len <= self.site_len
                and tuple(self.reserved) == (0, 0, 0, 0, 0))

    def _struct(self):
        s = _lib.MotifShapeStruct(self.up, self.site_len, self.down, self.proto_start, self.proto_len, self.cut_start, self.cut_len)
        for i, v in enumerate(self.reserved):
            s.reserved[i] = int(v)
        return s

    def __repr__(self):
        return "MotifShape(site_len=%d, spacer=(%d, %d), cut=(%d, %d), up=%d, down=%d)" % (
            self.site_len, self.proto_start, self.proto_len, self.cut_start, self.cut_len, self.up, self.down)


MOTIF_SHAPES = {"SpCas9": MotifShape(23, (0, 20), (16, 2), 16, 16), "Cas12a": MotifShape(27, (4, 23), (21, 6), 16, 16)}


def _motif_shape(shape, what="shape"):
    if isinstance(shape, str):
        if shape not in MOTIF_SHAPES:
            raise ValueError("%s names one of %s, or is a MotifShape" % (what, ", ".join(sorted(MOTIF_SHAPES))))
        shape = MOTIF_SHAPES[shape]
    if not isinstance(shape, MotifShape):
        raise ValueError("%s must be a MotifShape or the name of a preset" % what)
    return shape


class MotifSet:
    """A checked list of motifs that keeps their names: motif m is bit m of every mask.  names, texts (bytes) and both (bool)
    are parallel lists; mask() turns names into a bit mask; made by motifs()."""

    def __init__(self, names, texts, both, flags=None):
        self.names, self.texts, self.both = list(names), list(texts), list(both)
        self.flags = list(flags) if flags is not None else [MOTIF_BOTH_STRANDS if b else 0 for b in self.both]

    def __len__(self):
        return len(self.names)

    def mask(self, which, what="a motif mask"):
        """The bit mask of `which`: None -> 0, an integer below 2^len as it is, a name or a list of names."""
        if which is None:
            return 0
        if isinstance(which, (int, np.integer)) and not isinstance(which, bool):
            m = int(which)
            if m < 0 or m >> len(self):
                raise ValueError("%s has a bit at or above the number of motifs (%d)" % (what, len(self)))
            return m
        m = 0
        for name in ([which] if isinstance(which, str) else list(which)):
            if name not in self.names:
                raise ValueError("%s names %r, which is no motif of the set" % (what, name))
            m |= 1 << self.names.index(name)
        return m

    def names_of(self, mask):
        return [n for i, n in enumerate(self.names) if (int(mask) >> i) & 1]

    def _array(self):
        arr = (_lib.MotifStruct * max(len(self), 1))()
        for i, (t, f) in enumerate(zip(self.texts, self.flags)):
            arr[i].text = t[:16]
            arr[i].len = len(t)
            arr[i].flags = int(f)
        return arr


def motifs(entries, validate=True):
    """A MotifSet out of (name, text[, both_strands]) entries: 1..63 motifs, a text of 2..16 IUPAC letters (A C G T U R Y S W
    K M B D H V N, any case), not every letter N, names that differ; both_strands (default True) counts the reverse complement
    too.  validate=False passes the entries to the library as they are (tests)."""
    names, texts, both = [], [], []
    for e in entries:
        e = tuple(e)
        if validate and len(e) not in (2, 3):
            raise ValueError("a motif is (name, text) or (name, text, both_strands)")
        t = e[1] if isinstance(e[1], bytes) else str(e[1]).encode()
        if validate:
            if not 2 <= len(t) <= 16:
                raise ValueError("the motif %r has %d letters; a motif has 2..16" % (e[0], len(t)))
            if any(c not in _MOTIF_LETTERS for c in t):
                raise ValueError("the motif %r holds a letter that is no IUPAC letter" % (e[0],))
            if all(c in b"Nn" for c in t):
                raise ValueError("the motif %r is N alone" % (e[0],))
            if str(e[0]) in names:
                raise ValueError("the motif name %r occurs twice" % (e[0],))
        names.append(str(e[0]))
        texts.append(t)
        both.append(bool(e[2]) if len(e) > 2 else True)
    if validate and not 1 <= len(names) <= 63:
        raise ValueError("a motif set has 1..63 motifs, not %d" % len(names))
    return MotifSet(names, texts, both)


def _motif_set(m, what="motif_set"):
    if isinstance(m, MotifSet):
        return m
    if m is None:
        raise ValueError("%s is a MotifSet (motifs(...)) or a list of (name, text[, both_strands])" % what)
    return motifs(m)


def _motif_flank(text, what, validate=True):
    """A flank of a call as bytes (None: empty).  At most 16 letters of A C G T U, in any case."""
    if text is None:
        return b""
    b = text if isinstance(text, bytes) else str(text).encode()
    if validate and (len(b) > 16 or any(c not in b"ACGTUacgtu" for c in b)):
        raise ValueError("%s has at most 16 letters of A C G T U" % what)
    return b


def motif_text(context, shape, motif_set, left=None, right=None):
    """vsc_motif_text: the row (construct, cut, elsewhere) of one context of shape.context_len letters (A C G T U, any case; read
    orientation) under a MotifSet and the flanks, on the host, by the function the kernels call - for a guide list without a
    genome.  A context letter other than A C G T U gives (MOTIF_UNDEFINED,) * 3; unpack_motif_row names the bits."""
    shape = _motif_shape(shape)
    ms = _motif_set(motif_set)
    b = context if isinstance(context, bytes) else context.encode()
    if len(b) != shape.context_len:
        raise ValueError("the context has %d letters, the shape's context %d" % (len(b), shape.context_len))
    lf, rf = _motif_flank(left, "left"), _motif_flank(right, "right")
    sh = shape._struct()
    row = (C.c_uint64 * 3)()
    check(lib().vsc_motif_text(b, len(b), lf, len(lf), rf, len(rf), ms._array(), len(ms), C.byref(sh), row))
    return int(row[0]), int(row[1]), int(row[2])


def unpack_motif_row(rows, motif_set=None):
    """The masks of motif rows (one (construct, cut, elsewhere) triple or an array of shape (n, 3)) as a dict: construct, cut,
    elsewhere, cut_only (cut & ~elsewhere) and defined (bool; the masks of an undefined row are 0).  With a MotifSet also
    construct_names, cut_names, elsewhere_names and cut_only_names: the motifs' names per set bit (a list for one row, a list
    of lists for an array)."""
    a = np.asarray(rows, dtype=np.uint64)
    flat = a.reshape(-1, 3)
    und = np.uint64(MOTIF_UNDEFINED)
    defined = ~((flat[:, 0] == und) & (flat[:, 1] == und) & (flat[:, 2] == und))
    z = np.uint64(0)
    out = {"construct": np.where(defined, flat[:, 0], z), "cut": np.where(defined, flat[:, 1], z),
           "elsewhere": np.where(defined, flat[:, 2], z)}
    out["cut_only"] = out["cut"] & ~out["elsewhere"]
    keys = list(out)
    out["defined"] = defined
    if motif_set is not None:
        for k in keys:
            out[k + "_names"] = [motif_set.names_of(v) for v in out[k]]
    if a.ndim == 1:
        return {k: (bool(v[0]) if k == "defined" else v[0] if k.endswith("_names") else int(v[0])) for k, v in out.items()}
    return out


PICK_NONE = _lib.PICK_NONE  # a picks entry beyond counts[t]; the rank of a candidate that is not picked


class PickShape:
    """vsc_pick_params: k picks per target (1..32) whose cut sites lie at least `spacing` bases apart (0: no spacing), for
    sites of site_len bases (16..32) cut between read positions cut - 1 and cut (SpCas9: 17); candidates whose key is below
    min_key are never picked.  validate=False passes the numbers to the library as they are (tests)."""

    def __init__(self, k, spacing=0, site_len=READ_LEN, cut=17, min_key=0, validate=True):
        self.k, self.spacing, self.site_len, self.cut, self.min_key = int(k), int(spacing), int(site_len), int(cut), int(min_key)
        if validate and not (1 <= self.k <= 32 and 0 <= self.spacing < 2 ** 32 and 16 <= self.site_len <= 32
                             and 0 <= self.cut <= self.site_len and 0 <= self.min_key < 2 ** 64):
            raise ValueError("a pick shape has k 1..32, spacing and min_key unsigned, site_len 16..32 and cut 0..site_len")

    def _struct(self):
        return _lib.PickParams(self.site_len, self.cut, self.k, self.spacing, self.min_key, 0)

    def __repr__(self):
        return "PickShape(k=%d, spacing=%d, site_len=%d, cut=%d, min_key=%d)" % (self.k, self.spacing, self.site_len, self.cut,
                                                                                 self.min_key)


def order_bits(values):
    """The monotone map of float64 to uint64: all bits of a negative number flipped, the sign bit of every other - so that
    a < b as numbers implies order_bits(a) < order_bits(b) (-0.0 lies just below +0.0).  NaN maps to 0, below everything."""
    v = np.ascontiguousarray(values, dtype=np.float64)
    b = v.view(np.uint64)
    out = np.where((b >> np.uint64(63)).astype(bool), ~b, b ^ np.uint64(1 << 63)).astype(np.uint64)
    out[np.isnan(v)] = 0
    return out


def pick_key(columns, bits):
    """One uint64 key per candidate out of unsigned integer columns in priority order: column i is clipped to its bits[i] bits
    and the columns are packed most significant first, so that the larger key is the better candidate when larger is better
    in every column.  More than 64 bits in all, a bit count outside 1..64, a signed or float column or columns of different
    lengths are refused."""
    if len(columns) != len(bits) or not columns:
        raise ValueError("one bit count per column")
    if any(not (1 <= int(b) <= 64) for b in bits) or sum(int(b) for b in bits) > 64:
        raise ValueError("every column takes 1..64 bits and all of them at most 64")
    n = len(columns[0])
    key = np.zeros(n, dtype=np.uint64)
    for col, b in zip(columns, bits):
        c = np.asarray(col)
        if c.dtype.kind != "u" or c.ndim != 1 or len(c) != n:
            raise ValueError("a key column is a one-dimensional unsigned integer array, all of one length")
        top = np.uint64(2 ** int(b) - 1)
        key = (key << np.uint64(int(b) % 64)) | np.minimum(c.astype(np.uint64), top)
    return key


def _pick_arrays(n, n_targets, k, rank):
    return (np.full((n_targets, k), PICK_NONE, dtype=np.uint32), np.zeros(n_targets, dtype=np.uint32),
            np.full(n, PICK_NONE, dtype=np.uint32) if rank else None)


def _pick_loci(loci_or_found):
    """(codes or None, loci) of what a pick call is given: a PatternGuides, enumerate_guides' tuple, or loci."""
    if isinstance(loci_or_found, PatternGuides):
        return loci_or_found.codes, loci_or_found.loci
    if isinstance(loci_or_found, tuple) and len(loci_or_found) >= 2 and isinstance(loci_or_found[1], np.ndarray) \
            and loci_or_found[1].dtype == _lib.LOCUS_DTYPE:
        return loci_or_found[0], loci_or_found[1]
    return None, loci_or_found


def pick_host(contigs, loci, target, key, n_targets, shape, rank=False):
    """vsc_pick_host: the definition of the per-target pick as host code - no device.  contigs: a CONTIG_DTYPE array (a
    PackedGenome's .contigs); loci, target (uint32, REGION_NONE: no target) and key (uint64, larger is better): one entry per
    candidate.  Returns (picks uint32[n_targets, k], counts uint32[n_targets][, rank uint32[n]], stats)."""
    ct = np.ascontiguousarray(contigs, dtype=CONTIG_DTYPE)
    lo = _loci(loci, len(loci))
    tg = np.ascontiguousarray(target, dtype=np.uint32)
    ky = np.ascontiguousarray(key, dtype=np.uint64)
    if len(tg) != len(lo) or len(ky) != len(lo):
        raise ValueError("one target and one key per candidate")
    picks, counts, rk = _pick_arrays(len(lo), int(n_targets), shape.k, rank)
    st = _lib.PickStats()
    sh = shape._struct()
    check(lib().vsc_pick_host(ptr(ct), len(ct), ptr(lo), len(lo), ptr(tg), ptr(ky), int(n_targets), C.byref(sh), ptr(picks), ptr(counts),
                              ptr(rk) if rk is not None else None, C.byref(st)))
    return (picks, counts) + ((rk,) if rank else ()) + (st.as_dict(),)


# The fixed quantisation of the columns a design call (and the tools' -b) can rank by: (bits, what the column is made from)
PICK_COLUMNS = {"mit": 14, "table": 14, "eff": 20, "oof": 10, "mh": 20, "fold": 6, "rflp": 6, "knockout": 17}


def pick_column(name, values):
    """One key column in the tools' fixed quantisation (PICK_COLUMNS bits): mit / table: rint(100 x specificity) of float64
    specificities; eff: the top 20 bits of order_bits of the linear predictors; oof: floor(1000 oof / sum) of (sum, oof)
    pairs, undefined -> 0; mh: min(sum, 2^20 - 1) of the pairs, undefined -> 0; fold: 32 - starts of the fold rows (fewer stems
    are better), undefined -> 0; rflp: min(popcount(cut & ~elsewhere), 63) of the motif rows (more motifs that lie over the
    cut and nowhere else in the context are better), undefined -> 0; knockout: of the knock-out rows, bit 16 = NMD in both
    frames, bits 0 .. 15 = 65535 - frac (an earlier cut is better); a row that is undefined or no coding cut -> 0."""
    if name == "knockout":
        r = unpack_knockout_row(values)
        both = (r["flags"] & 0x30) == 0x30
        key = (both.astype(np.uint64) << np.uint64(16)) | (np.uint64(65535) - r["frac"].astype(np.uint64))
        return np.where(r["coding"], key, np.uint64(0)).astype(np.uint64)
    if name in ("mit", "table"):  # (NaN and negative values: 0, as the undefined values of the other columns)
        v = np.asarray(values, dtype=np.float64)
        return np.rint(100.0 * np.where(np.isnan(v) | (v <= 0), 0.0, np.minimum(v, 1e6))).astype(np.uint64)
    if name == "eff":
        return order_bits(values) >> np.uint64(44)
    if name == "rflp":
        only = unpack_motif_row(np.asarray(values, dtype=np.uint64).reshape(-1, 3))["cut_only"]
        count = np.zeros(len(only), dtype=np.uint64)
        for m in range(63):
            count += (only >> np.uint64(m)) & np.uint64(1)
        return np.minimum(count, np.uint64(63))
    pairs = np.asarray(values, dtype=np.uint32).reshape(-1, 2).astype(np.uint64)
    undefined = pairs[:, 0] == MH_UNDEFINED
    if name == "fold":
        return np.where(undefined, np.uint64(0), np.uint64(32) - np.minimum(pairs[:, 0] & np.uint64(0xFF), np.uint64(32))).astype(np.uint64)
    if name == "oof":
        q = np.uint64(1000) * pairs[:, 1] // np.maximum(pairs[:, 0], np.uint64(1))
        return np.where(undefined | (pairs[:, 0] == 0), np.uint64(0), q).astype(np.uint64)
    if name == "mh":
        return np.where(undefined, np.uint64(0), np.minimum(pairs[:, 0], np.uint64(2 ** 20 - 1))).astype(np.uint64)
    raise ValueError("a pick column is one of mit, table, eff, oof, mh, fold, rflp, knockout")


EDIT_UNDEFINED = _lib.EDIT_UNDEFINED  # mask and hits of a candidate whose site is undefined
EDIT_PAIR_DTYPE = _lib.EDIT_PAIR_DTYPE


class EditShape:
    """vsc_edit_shape: where a base editor edits.  site_len 16..32 is the candidates' length (23 for enumerate_guides', the
    pattern's for enumerate_pattern's); window = (start, length) in read positions of the site, 0 = its first read base,
    length 1..16; base is the letter the editor converts on the read strand ("C" for a CBE, "A" for an ABE; or 0..3).
    EDITORS holds two presets for the SpCas9 23-mer, "CBE" (window (3, 5), C) and "ABE" (window (3, 4), A): common published
    windows and nothing more - an editor's real window depends on the deaminase, the linker and the target.
    validate=False passes the numbers to the library as they are (tests)."""

    def __init__(self, site_len=READ_LEN, window=(3, 5), base="C", validate=True):
        self.site_len, self.win_start, self.win_len = int(site_len), int(window[0]), int(window[1])
        if isinstance(base, (str, bytes)):
            b = base.decode() if isinstance(base, bytes) else base
            if len(b) != 1 or b.upper() not in "ACGT":
                raise ValueError("an editor converts one of A, C, G, T")
            self.base = "ACGT".index(b.upper())
        else:
            self.base = int(base)
        if validate and not (16 <= self.site_len <= 32 and 1 <= self.win_len <= 16 and 0 <= self.win_start
                             and self.win_start + self.win_len <= self.site_len and 0 <= self.base <= 3):
            raise ValueError("an edit shape has site_len 16..32, a window of 1..16 bases inside the site and a base A, C, G or T")

    @property
    def window(self):
        return self.win_start, self.win_len

    def _struct(self):
        return _lib.EditShapeStruct(self.site_len, self.win_start, self.win_len, self.base, (C.c_uint32 * 4)(0, 0, 0, 0))

    def __repr__(self):
        return "EditShape(site_len=%d, window=(%d, %d), base=%r)" % (self.site_len, self.win_start, self.win_len,
                                                                     "ACGT"[self.base] if 0 <= self.base <= 3 else self.base)


# Two presets for the SpCas9 23-mer (20 protospacer bases, then NGG; read position 0 is the PAM-distal end): the windows
# commonly published for BE3 / BE4-type cytosine editors (protospacer positions 4-8) and ABE7.10-type adenine editors
# (positions 4-7).  They are common published windows and nothing more: an editor's real window depends on the deaminase,
# the linker and the target, and a caller who knows better passes an EditShape.
EDITORS = {"CBE": EditShape(READ_LEN, (3, 5), "C"), "ABE": EditShape(READ_LEN, (3, 4), "A")}


def edit_site_text(site, shape):
    """vsc_edit_site_text: the MASK of one site of shape.site_len letters (any case) in read orientation on the host, by the
    function the kernels call: bit j is set iff the letter at window position j is the editor's base.  A letter other than
    ACGT or a text of another length raises VarscotError."""
    b = site if isinstance(site, bytes) else site.encode()
    m = C.c_uint32()
    sh = shape._struct()
    check(lib().vsc_edit_site_text(b, C.byref(sh), C.byref(m)))
    return int(m.value)


def unpack_edit_info(info):
    """(at, bystanders) of an edit pair's info word (or an array of them): the window position of the target's base and the
    number of other editable bases in the window."""
    i = np.asarray(info, dtype=np.uint32)
    return i & np.uint32(0xFF), i >> np.uint32(8)


def edit_targets(targets):
    """The targets of an edit call as the library takes them: (sorted EDIT_TARGET_DTYPE array without duplicates - strictly
    ascending (contig, pos) -, order, inverse).  order[k] is the caller's index of sorted target k (the first of its
    duplicates), inverse[i] the sorted index of the caller's target i.  targets: (contig, pos) rows or an array with
    "contig" and "pos" fields, in any order."""
    if isinstance(targets, np.ndarray) and targets.dtype.names and {"contig", "pos"} <= set(targets.dtype.names):
        c, p = targets["contig"].astype(np.int64), targets["pos"].astype(np.int64)
    else:
        a = np.asarray(targets, dtype=np.int64).reshape(-1, 2)
        c, p = a[:, 0], a[:, 1]
    if len(c) and (c.min() < 0 or c.max() > 0xFFFFFFFF or p.min() < 0 or p.max() > 0xFFFFFFFF):
        raise ValueError("a target is a (contig, pos) of unsigned 32-bit numbers")
    key = (c.astype(np.uint64) << np.uint64(32)) | p.astype(np.uint64)
    uniq, order, inverse = np.unique(key, return_index=True, return_inverse=True)
    out = np.zeros(len(uniq), dtype=_lib.EDIT_TARGET_DTYPE)
    out["contig"], out["pos"] = (uniq >> np.uint64(32)).astype(np.uint32), (uniq & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    return out, order.astype(np.int64), np.asarray(inverse, dtype=np.int64).reshape(-1)


def edit_pick_inputs(pairs, loci, extra_columns=()):
    """What Genome.pick takes for "of every target the K guides with the fewest bystanders": (loci[pairs.candidate],
    pairs.target, key) - one pick candidate per edit pair, its target the pair's, its key made with pick_key so that fewer
    bystanders is better: the first column is 15 - bystanders (4 bits).  extra_columns: (values per CANDIDATE of the edit
    call, bits) in priority order behind it - unsigned integer arrays, larger is better (pick_column makes them)."""
    pr = np.asarray(pairs, dtype=_lib.EDIT_PAIR_DTYPE)
    lo = _loci(loci, len(loci))
    cand = pr["candidate"].astype(np.int64)
    cols = [(np.uint64(15) - (pr["info"] >> np.uint32(8)).astype(np.uint64))]
    bits = [4]
    for values, b in extra_columns:
        v = np.asarray(values)
        if v.dtype.kind != "u" or v.ndim != 1 or len(v) != len(lo):
            raise ValueError("an extra column is a one-dimensional unsigned integer array with one value per candidate")
        cols.append(v[cand])
        bits.append(int(b))
    return lo[cand], pr["target"].astype(np.uint32), pick_key(cols, bits)


# ---- known variation under candidate guides -----------------------------------------------------------------
VARIATION_UNDEFINED = _lib.VARIATION_UNDEFINED  # the four words of the row of a candidate whose site is undefined
VARIANT_OTHER = _lib.VARIANT_OTHER              # the alt of a variant that is no SNV
VARIANT_DTYPE = _lib.VARIANT_DTYPE
VARIATION_PAIR_DTYPE = _lib.VARIATION_PAIR_DTYPE
VARIATION_ZONES = ("none", "distal", "seed", "pam")  # the labels the presets use
VARIANT_WEIGHT_ONE = 1 << 20                    # variant_weight's scale: cost / 2^20 = -ln P(no disrupting variant)
_IUPAC_BITS = {"A": 1, "C": 2, "G": 4, "T": 8, "R": 5, "Y": 10, "S": 6, "W": 9, "K": 12, "M": 3, "B": 14, "D": 13, "H": 11, "V": 7,
               "N": 15}


class VariationShape:
    """vsc_variation_shape: how known variants count against a site.  site_len 16..32 is the candidates' length; zones: one
    label 0..3 per read position (a sequence of site_len numbers, or the packed integer: two bits per position) - the presets
    use 1 distal, 2 seed, 3 PAM, 0 a position of no interest such as the N of NGG; accept: per read position the read bases
    that leave the site usable, as a sequence of site_len IUPAC letters ("-" or "": none) or numbers 0..15 (bit b: base b of A
    C G T), or the packed (low, high) pair of integers: four bits per position.  validate=False passes the numbers to the
    library as they are (tests)."""

    def __init__(self, site_len=READ_LEN, zones=0, accept=(0, 0), validate=True):
        self.site_len = int(site_len)
        if isinstance(zones, (int, np.integer)):
            self.zones = int(zones)
        else:
            z = [int(v) for v in zones]
            if len(z) != self.site_len or any(not 0 <= v <= 3 for v in z):
                raise ValueError("zones holds one label 0..3 per read position")
            self.zones = sum(v << (2 * j) for j, v in enumerate(z))
        if isinstance(accept, tuple) and len(accept) == 2 and all(isinstance(v, (int, np.integer)) for v in accept):
            self.accept = (int(accept[0]), int(accept[1]))
        else:
            a = [(_IUPAC_BITS[v.upper()] if v not in ("", "-") else 0) if isinstance(v, str) else int(v) for v in accept]
            if len(a) != self.site_len or any(not 0 <= v <= 15 for v in a):
                raise ValueError("accept holds one IUPAC letter or number 0..15 per read position")
            self.accept = (sum(v << (4 * j) for j, v in enumerate(a[:16])), sum(v << (4 * j) for j, v in enumerate(a[16:])))
        if validate and not (16 <= self.site_len <= 32 and 0 <= self.zones < 1 << (2 * self.site_len) and 0 <= self.accept[0] < 1 << 64
                             and 0 <= self.accept[1] < 1 << (4 * (self.site_len - 16))):
            raise ValueError("a variation shape has site_len 16..32 and no zone or accept bit at a position from site_len on")

    def zone(self, j):
        return self.zones >> (2 * j) & 3

    def accepts(self, j):
        return self.accept[j >> 4] >> (4 * (j & 15)) & 15

    def _struct(self):
        m = (1 << 64) - 1
        return _lib.VariationShapeStruct(self.site_len & 0xFFFFFFFF, 0, self.zones & m, (C.c_uint64 * 2)(self.accept[0] & m, self.accept[1] & m),
                                         (C.c_uint32 * 4)(0, 0, 0, 0))

    def __repr__(self):
        return "VariationShape(site_len=%d, zones=%r, accept=%r)" % (self.site_len, "".join(str(self.zone(j)) for j in range(self.site_len)),
                                                                      [self.accepts(j) for j in range(self.site_len)])


def variation_shape_from_pattern(pattern, protospacer, seed_len):
    """The VariationShape of an IUPAC pattern of 16..32 letters with the protospacer (start, length) in read positions
    (pattern_protospacer gives it for a preset): inside the protospacer the seed_len bases next to the PAM are seed (2), the
    others distal (1), and no base is accepted there; outside it a position is PAM (3) and accepts the pattern's IUPAC set -
    an N is of no interest (0) and accepts every base.  The PAM lies on one side of the protospacer: behind it (SpCas9: the
    seed is the protospacer's end) or in front of it (Cas12a: its start)."""
    p = pattern.decode() if isinstance(pattern, bytes) else pattern
    start, length = int(protospacer[0]), int(protospacer[1])
    n = len(p)
    if not (0 <= start and 1 <= length and start + length <= n) or not 0 <= int(seed_len) <= length:
        raise ValueError("the protospacer lies inside the pattern, and the seed inside the protospacer")
    if start > 0 and start + length < n:
        raise ValueError("the PAM lies on one side of the protospacer")
    seed_first = start if start > 0 else start + length - int(seed_len)  # PAM in front: the first bases; behind: the last
    zones, accept = [], []
    for j, ch in enumerate(p.upper()):
        if start <= j < start + length:
            zones.append(2 if seed_first <= j < seed_first + int(seed_len) else 1)
            accept.append(0)
        else:
            if ch not in _IUPAC_BITS:
                raise ValueError("%r is no IUPAC letter" % ch)
            zones.append(0 if ch == "N" else 3)
            accept.append(_IUPAC_BITS[ch])
    return VariationShape(n, zones, accept)


# SpCas9 NGG with a 10-base seed (read positions 10..19; the N at 20 is of no interest, the GG accept G only), and the other
# rows of PATTERNS by the same rule.  The seed's length is a convention (8 to 12 bases are in use); a caller who knows better
# makes a shape.
VARIATION_SHAPES = {"SpCas9": variation_shape_from_pattern("N" * 20 + "NGG", (0, 20), 10),
                    "SaCas9": variation_shape_from_pattern("N" * 21 + "NNGRRT", (0, 21), 10),
                    "Cas12a": variation_shape_from_pattern("TTTV" + "N" * 23, (4, 23), 8)}


def _variation_shape(shape, what="shape"):
    if isinstance(shape, str):
        if shape not in VARIATION_SHAPES:
            raise ValueError("%s names one of %s, or is a VariationShape" % (what, ", ".join(sorted(VARIATION_SHAPES))))
        return VARIATION_SHAPES[shape]
    if not isinstance(shape, VariationShape):
        raise ValueError("%s must be a VariationShape or the name of a preset" % what)
    return shape


def variant_weight(af):
    """The integer weight of a variant of allele frequency af (a number or an array): round(-log1p(-af) * 2^20), at most
    0xFFFFFFFE (af >= 1 included).  Under independence the cost of a candidate - the sum over its disrupting variants - is then
    -ln P(a haplotype carries none of them) in units of 2^-20; carrier_free turns it back."""
    a = np.asarray(af, dtype=np.float64)
    if (a < 0).any() or np.isnan(a).any():
        raise ValueError("an allele frequency is a number in 0 .. 1")
    with np.errstate(divide="ignore"):
        x = np.where(a >= 1.0, np.inf, -np.log1p(-np.minimum(a, 1.0)) * float(VARIANT_WEIGHT_ONE))
    w = np.minimum(np.floor(x + 0.5), float(0xFFFFFFFE)).astype(np.uint32)
    return int(w) if w.ndim == 0 else w


def carrier_free(cost):
    """exp(-cost / 2^20): the probability that a haplotype carries no disrupting variant, from a row's cost made of
    variant_weight weights (a clamped cost, 0xFFFFFFFE, gives practically 0)."""
    c = np.asarray(cost, dtype=np.float64)
    out = np.exp(-c / float(VARIANT_WEIGHT_ONE))
    return float(out) if out.ndim == 0 else out


def site_variants(rows, lengths=None):
    """The variants of a variation call as the library takes them: (VARIANT_DTYPE array in ascending (contig, pos) - rows of
    one position keep the caller's order -, order, inverse).  order[k] is the caller's index of sorted variant k, inverse[i]
    the sorted index of the caller's row i.  rows: (contig, pos, ref, alt[, weight]) in any order - pos the 0-based position of
    ref's first base on the contig, ref and alt VCF-style allele texts, weight an integer 0..0xFFFFFFFE (0 without one).
    The alleles are normalised: the common prefix, then the common suffix is trimmed; what is left is an SNV (span 1 with its
    alt), a deletion (its deleted bases), an insertion (the two bases that flank the insertion point; one at a contig's
    first base - and at its end, for which lengths= gives the contig lengths), or anything else (alt 4 over the bases of ref:
    an MNV its length).  Equal alleles, symbolic alleles and spans above 65535 are refused."""
    rec, keys = [], []
    for row in rows:
        if len(row) not in (4, 5):
            raise ValueError("a variant is (contig, pos, ref, alt[, weight])")
        contig, pos = int(row[0]), int(row[1])
        ref, alt = (x.decode() if isinstance(x, bytes) else str(x) for x in (row[2], row[3]))
        ref, alt = ref.upper(), alt.upper()
        weight = int(row[4]) if len(row) == 5 else 0
        if not (0 <= contig <= 0xFFFFFFFF and 0 <= pos <= 0xFFFFFFFF and 0 <= weight <= 0xFFFFFFFE):
            raise ValueError("contig and pos are unsigned 32-bit numbers, a weight is at most 0xFFFFFFFE")
        if not ref or not alt or any(ch not in "ACGTN" for ch in ref + alt):
            raise ValueError("alleles are texts over ACGTN (symbolic alleles are not taken): %r -> %r" % (ref, alt))
        k = 0
        while k < len(ref) and k < len(alt) and ref[k] == alt[k]:
            k += 1
        ref, alt, pos = ref[k:], alt[k:], pos + k
        k = 0
        while k < len(ref) and k < len(alt) and ref[-1 - k] == alt[-1 - k]:
            k += 1
        if k:
            ref, alt = ref[:-k], alt[:-k]
        if not ref and not alt:
            raise ValueError("a variant's alleles are equal")
        if len(ref) == 1 and len(alt) == 1:
            span, code = 1, "ACGT".index(alt) if alt in "ACGT" else VARIANT_OTHER
        elif not ref:  # an insertion in front of pos: the bases on either side of it
            first = max(pos - 1, 0)
            last = pos + 1
            if lengths is not None and contig < len(lengths):
                last = min(last, int(lengths[contig]))
            pos, span, code = first, last - first, VARIANT_OTHER
        else:
            span, code = len(ref), VARIANT_OTHER
        if not 1 <= span <= 65535 or pos > 0xFFFFFFFF:
            raise ValueError("a variant spans 1 .. 65535 bases")
        rec.append((contig, pos, span | code << 16, weight))
        keys.append(contig << 32 | pos)
    out = np.zeros(len(rec), dtype=_lib.VARIANT_DTYPE)
    order = np.argsort(np.asarray(keys, dtype=np.uint64), kind="stable").astype(np.int64) if rec else np.zeros(0, dtype=np.int64)
    for k, i in enumerate(order):
        out[k] = rec[int(i)]
    inverse = np.empty(len(rec), dtype=np.int64)
    inverse[order] = np.arange(len(rec), dtype=np.int64)
    return out, order, inverse


def unpack_variation_row(rows):
    """(by_zone uint8[n, 4], silent, cost, max_weight) of variation rows uint32[n, 4]: the disrupting variants by their top zone
    (255: that many or more), the silent variants, the clamped sum and the largest of the disrupting variants' weights.  A row
    of an undefined site is VARIATION_UNDEFINED four times: 255 in every zone."""
    r = np.asarray(rows, dtype=np.uint32).reshape(-1, 4)
    by_zone = np.stack([(r[:, 0] >> np.uint32(8 * z)) & np.uint32(0xFF) for z in range(4)], axis=1).astype(np.uint8)
    return by_zone, r[:, 1].copy(), r[:, 2].copy(), r[:, 3].copy()


def unpack_variation_info(info):
    """(first, touched, top, silent) of a variation pair's info word (or an array of them): the smallest touched read position,
    the number of touched read positions, the largest zone label among them, and 1 for a silent SNV."""
    i = np.asarray(info, dtype=np.uint32)
    return i & np.uint32(0xFF), (i >> np.uint32(8)) & np.uint32(0xFF), (i >> np.uint32(16)) & np.uint32(3), (i >> np.uint32(18)) & np.uint32(1)


def variation_pick_inputs(pairs, loci, zones=(2, 3), extra_columns=()):
    """What Genome.pick takes for "of every variant the K guides that tell its alleles apart best": (loci[pairs.candidate],
    pairs.variant, key, index) over the DISRUPTING pairs whose top zone is in `zones` (default: seed and PAM) - one pick
    candidate per such pair, its target the pair's variant, its key made with pick_key: the first column is the top zone (2
    bits: PAM before seed).  index holds the kept pairs' places in `pairs`.  extra_columns: (values per CANDIDATE of the
    variation call, bits) in priority order behind it - unsigned integer arrays, larger is better (pick_column makes them)."""
    pr = np.asarray(pairs, dtype=_lib.VARIATION_PAIR_DTYPE)
    lo = _loci(loci, len(loci))
    _, _, top, silent = unpack_variation_info(pr["info"])
    index = np.flatnonzero((silent == 0) & np.isin(top, np.asarray(sorted({int(z) for z in zones}), dtype=np.uint32)))
    cand = pr["candidate"][index].astype(np.int64)
    cols, bits = [top[index].astype(np.uint64)], [2]
    for values, b in extra_columns:
        v = np.asarray(values)
        if v.dtype.kind != "u" or v.ndim != 1 or len(v) != len(lo):
            raise ValueError("an extra column is a one-dimensional unsigned integer array with one value per candidate")
        cols.append(v[cand])
        bits.append(int(b))
    return lo[cand], pr["variant"][index].astype(np.uint32), pick_key(cols, bits), index


def _variants_in(variants):
    """(sorted VARIANT_DTYPE array, order, inverse) of what a variation call is given: a VARIANT_DTYPE array as the library takes
    it (passed as it is: order and inverse None), or rows for site_variants."""
    if isinstance(variants, np.ndarray) and variants.dtype == _lib.VARIANT_DTYPE:
        return np.ascontiguousarray(variants), None, None
    return site_variants(variants)


def variation_host(contigs, loci, shape, variants, pairs=True, coverage=False):
    """vsc_variation_host: the definition of the variation join as host code - no device.  contigs: a CONTIG_DTYPE array (a
    PackedGenome's .contigs); loci, shape, variants: as Genome.variation takes them.  Without planes a site's class is invalid
    or defined only.  Returns (rows uint32[n, 4], pairs or None, coverage uint32[n_v, 2] or None), as Genome.variation."""
    shape = _variation_shape(shape)
    ct = np.ascontiguousarray(contigs, dtype=CONTIG_DTYPE)
    _, loci = _pick_loci(loci)
    lo = _loci(loci, len(loci))
    vr, order, inverse = _variants_in(variants)
    n, n_v = len(lo), len(vr)
    rows = np.empty((n, 4), dtype=np.uint32)
    cov = np.empty((n_v, 2), dtype=np.uint32) if coverage else None
    sh = shape._struct()
    count = C.c_uint64()
    L = lib()
    check(L.vsc_variation_host(ptr(ct), len(ct), ptr(lo), n, C.byref(sh), ptr(vr) if n_v else None, n_v, ptr(rows), None, 0, C.byref(count),
                               ptr(cov)))
    pr = None
    if pairs:
        pr = np.empty(int(count.value), dtype=_lib.VARIATION_PAIR_DTYPE)
        check(L.vsc_variation_host(ptr(ct), len(ct), ptr(lo), n, C.byref(sh), ptr(vr) if n_v else None, n_v, None, ptr(pr), len(pr),
                                   C.byref(count), None))
    return rows, _variation_pairs_out(pr, order), (cov[inverse] if cov is not None and inverse is not None else cov)


def _variation_pairs_out(pr, order):
    """The pairs with the variant's index in the caller's order, ascending (candidate, variant)."""
    if pr is None or order is None:
        return pr
    pr["variant"] = order[pr["variant"].astype(np.int64)].astype(np.uint32)
    return pr[np.lexsort((pr["variant"], pr["candidate"]))]


# ---- prime-editing guide design -----------------------------------------------------------------------------
PRIME_UNDEFINED = _lib.PRIME_UNDEFINED  # both words of the row of a candidate whose context is undefined
PRIME_EDIT_DTYPE = _lib.PRIME_EDIT_DTYPE
PRIME_PAIR_DTYPE = _lib.PRIME_PAIR_DTYPE
PRIME_FLAGS = ("PAM", "SEED", "POLY_T", "WEAK")  # bit k of a pair's flags


class PrimeShape:
    """vsc_prime_shape: how a prime editor's pegRNA is laid out on a candidate.  site_len 16..32 is the candidates' length, down
    the bases of context behind the site in read orientation (C = site_len + down <= 64), nick the read position the nick lies
    in front of (17 for the SpCas9 23-mer).  pbs = (min, max) lengths of the primer binding site, 1 <= min <= max <= nick; rtt =
    (min, max) lengths of the template, 1 <= min <= max <= C - nick; pbs max + rtt max <= 64.  min_homology: template bases
    behind the edit.  pam / seed = (start, length 0..8) in read positions inside the site: a pair whose edit changes a letter
    there carries the PAM / SEED flag.  avoid_g_end: lengthen the template until it does not end on G.  stability = (init,
    mono[4], di[16], target): the integer model of the PBS, every |weight| <= 2^20 - the PBS is the shortest of pbs whose sum
    reaches target, else pbs max and WEAK; None: all 0 (the PBS is pbs min).  validate=False passes the numbers to the library as
    they are (tests)."""

    def __init__(self, site_len=READ_LEN, down=41, nick=17, pbs=(13, 13), rtt=(10, 34), min_homology=5, pam=(21, 2), seed=(17, 3),
                 avoid_g_end=True, stability=None, validate=True):
        self.site_len, self.down, self.nick = int(site_len), int(down), int(nick)
        self.pbs_min, self.pbs_max = int(pbs[0]), int(pbs[1])
        self.rtt_min, self.rtt_max = int(rtt[0]), int(rtt[1])
        self.min_homology = int(min_homology)
        self.pam_start, self.pam_len = int(pam[0]), int(pam[1])
        self.seed_start, self.seed_len = int(seed[0]), int(seed[1])
        self.flags = int(avoid_g_end)
        if stability is None:
            stability = (0, (0,) * 4, (0,) * 16, 0)
        self.init, self.target = int(stability[0]), int(stability[3])
        self.mono, self.di = tuple(int(v) for v in stability[1]), tuple(int(v) for v in stability[2])
        if len(self.mono) != 4 or len(self.di) != 16:
            raise ValueError("a stability model has 4 mononucleotide and 16 dinucleotide weights")
        if validate and not self.valid():
            raise ValueError("a prime shape has site_len 16..32, down <= 64 - site_len, 1 <= nick <= site_len, 1 <= pbs min <= max "
                             "<= nick, 1 <= rtt min <= max <= C - nick, pbs max + rtt max <= 64, min_homology <= rtt max, pam and "
                             "seed ranges of at most 8 positions inside the site and weights of at most 2^20")

    def valid(self):
        C_ = self.site_len + self.down
        w = (self.init, self.target) + self.mono + self.di

        def inside(start, length):
            return 0 <= length <= 8 and 0 <= start and start + length <= self.site_len
        return (16 <= self.site_len <= 32 and 0 <= self.down <= 64 - self.site_len and 1 <= self.nick <= self.site_len
                and 1 <= self.pbs_min <= self.pbs_max <= self.nick and 1 <= self.rtt_min <= self.rtt_max <= C_ - self.nick
                and self.pbs_max + self.rtt_max <= 64 and 0 <= self.min_homology <= self.rtt_max
                and inside(self.pam_start, self.pam_len) and inside(self.seed_start, self.seed_len) and self.flags in (0, 1)
                and all(abs(v) <= 1 << 20 for v in w))

    @property
    def context_len(self):
        return self.site_len + self.down

    def _struct(self):
        return _lib.PrimeShapeStruct(self.site_len, self.down, self.nick, self.pbs_min, self.pbs_max, self.rtt_min, self.rtt_max,
                                     self.min_homology, self.pam_start, self.pam_len, self.seed_start, self.seed_len, self.flags,
                                     self.init, (C.c_int32 * 4)(*self.mono), (C.c_int32 * 16)(*self.di), self.target,
                                     (C.c_uint32 * 5)(0, 0, 0, 0, 0))

    def __repr__(self):
        return "PrimeShape(site_len=%d, down=%d, nick=%d, pbs=(%d, %d), rtt=(%d, %d), min_homology=%d, pam=(%d, %d), seed=(%d, %d), " \
               "avoid_g_end=%r)" % (self.site_len, self.down, self.nick, self.pbs_min, self.pbs_max, self.rtt_min, self.rtt_max,
                                    self.min_homology, self.pam_start, self.pam_len, self.seed_start, self.seed_len, bool(self.flags))


# One preset for the SpCas9 23-mer (20 protospacer bases, then NGG; the nick lies three bases in front of the PAM): a 13-base
# primer binding site, templates of 10 to 34 bases with at least 5 bases of homology behind the edit that do not end on G, the GG
# of the PAM and the three protospacer bases next to the nick as the ranges whose change keeps the edited strand from being
# nicked again.  These are commonly published settings for PE2 and nothing more: the best lengths depend on the target, and a
# caller who knows better passes a PrimeShape (with a stability model, if the PBS is to be chosen by one).
PRIME_EDITORS = {"PE2": PrimeShape(READ_LEN, 41, 17, (13, 13), (10, 34), 5, (21, 2), (17, 3), True)}


def _prime_shape(shape, what="shape"):
    if isinstance(shape, str):
        if shape not in PRIME_EDITORS:
            raise ValueError("%s names one of %s, or is a PrimeShape" % (what, ", ".join(sorted(PRIME_EDITORS))))
        shape = PRIME_EDITORS[shape]
    if not isinstance(shape, PrimeShape):
        raise ValueError("%s must be a PrimeShape or the name of a preset" % what)
    return shape


def _prime_ins(ins):
    """(ins_len, 2-bit code) of an insertion given as letters (or as (ins_len, code))."""
    if isinstance(ins, (str, bytes)):
        t = (ins.decode() if isinstance(ins, bytes) else ins).upper()
        if t in ("", "-"):
            return 0, 0
        if len(t) > 16 or any(c not in "ACGT" for c in t):
            raise ValueError("an insertion is at most 16 letters of ACGT")
        return len(t), sum("ACGT".index(c) << (2 * k) for k, c in enumerate(t))
    n, code = ins
    return int(n), int(code)


def prime_edits(rows):
    """The edits of a prime call as the library takes them: (sorted PRIME_EDIT_DTYPE array - strictly ascending (contig, pos) -,
    order, inverse).  order[k] is the caller's index of sorted edit k, inverse[i] the sorted index of the caller's edit i.  rows:
    (contig, pos, del_len, ins) tuples with ins the inserted letters ("" or "-": none), or a PRIME_EDIT_DTYPE array, in any
    order.  Two edits at one (contig, pos) are refused: several alleles of one position go into several calls."""
    if isinstance(rows, np.ndarray) and rows.dtype == _lib.PRIME_EDIT_DTYPE:
        e = rows.copy().reshape(-1)
    else:
        rows = list(rows)
        e = np.zeros(len(rows), dtype=_lib.PRIME_EDIT_DTYPE)
        for k, (contig, pos, del_len, ins) in enumerate(rows):
            if not (0 <= int(contig) <= 0xFFFFFFFF and 0 <= int(pos) <= 0xFFFFFFFF and 0 <= int(del_len) <= 0xFFFF):
                raise ValueError("an edit is (contig, pos, del_len, ins) of unsigned numbers")
            n, code = _prime_ins(ins)
            e[k] = (int(contig), int(pos), int(del_len), n, code)
    key = (e["contig"].astype(np.uint64) << np.uint64(32)) | e["pos"].astype(np.uint64)
    order = np.argsort(key, kind="stable").astype(np.int64)
    if len(key) > 1 and (np.diff(key[order].astype(np.int64).view(np.uint64)) == 0).any():
        raise ValueError("two edits at one (contig, pos): several alleles of one position go into several calls")
    inverse = np.empty(len(order), dtype=np.int64)
    inverse[order] = np.arange(len(order), dtype=np.int64)
    return np.ascontiguousarray(e[order]), order, inverse


def unpack_prime_info(info):
    """(t, d, h, flags) of a prime pair's info word (or an array of them): the template's length, the bases between the nick and
    the edit, the homology behind the edit, and the flags (bit k: PRIME_FLAGS[k])."""
    i = np.asarray(info, dtype=np.uint32)
    return i & np.uint32(0xFF), (i >> np.uint32(8)) & np.uint32(0xFF), (i >> np.uint32(16)) & np.uint32(0xFF), i >> np.uint32(24)


def unpack_prime_ext(ext):
    """(length, gc, pbs_len) of a prime pair's ext word (or an array of them): the extension's length (PBS + RTT), its G/C and
    the length of its primer binding site."""
    x = np.asarray(ext, dtype=np.uint32)
    return x & np.uint32(0xFF), (x >> np.uint32(8)) & np.uint32(0xFF), x >> np.uint32(16)


def unpack_prime_row(pbs):
    """(pbs_len, pbs_gc, weak) of a prime row's first word (or an array of them)."""
    x = np.asarray(pbs, dtype=np.uint32)
    return x & np.uint32(0xFF), (x >> np.uint32(8)) & np.uint32(0xFF), (x >> np.uint32(16)) & np.uint32(1)


def prime_site_text(context, shape, e0=None, del_len=0, ins=""):
    """vsc_prime_site_text: one context of shape.context_len letters (any case) in read orientation on the host, by the
    functions the kernels call - and, with e0, its pair with one edit in READ coordinates: read bases [e0, e0 + del_len) are
    replaced by the letters `ins` (as the read strand has them).  Returns (pbs word, exists, info, ext, extension): exists is
    False (and info = ext = 0, extension = "") without an edit, for an edit in front of the nick and for a pair the shape
    refuses.  A letter other than ACGT or a text of another length raises VarscotError."""
    b = context if isinstance(context, bytes) else context.encode()
    sh = _prime_shape(shape)._struct()
    row = (C.c_uint32 * 2)()
    pair = (C.c_uint32 * 2)()
    text = C.create_string_buffer(80)
    it = None
    if e0 is not None:
        it = ins if isinstance(ins, bytes) else ins.encode()
    check(lib().vsc_prime_site_text(b, C.byref(sh), 0 if e0 is None else int(e0), int(del_len), it, row, pair, text))
    return int(row[0]), bool(row[1]), int(pair[0]), int(pair[1]), text.value.decode()


def _revcomp_text(s):
    return s.translate(str.maketrans("ACGTacgt", "TGCAtgca"))[::-1]


def prime_extension(packed, shape, locus, edit, strict=True):
    """The 3' extension of the pegRNA of one pair as DNA letters, RTT then PBS, 5' to 3' (EXTENSION): the context of `locus` =
    (contig, pos, strand) out of a PackedGenome, the edit = (contig, pos, del_len, ins) in forward coordinates as prime_edits
    takes it, turned into read coordinates and given to prime_site_text.  "" when the pair does not exist; strict=True raises
    ValueError then."""
    shape = _prime_shape(shape)
    contig, pos, strand = int(locus[0]), int(locus[1]), int(locus[2])
    C_ = shape.context_len
    f0 = pos - shape.down if strand else pos
    row = packed.contigs[contig]
    seq = packed.decode(int(row["offset"]) + f0, C_) if 0 <= f0 and f0 + C_ <= int(row["length"]) else ""
    n, code = _prime_ins(edit[3])
    letters = "".join("ACGT"[(code >> (2 * k)) & 3] for k in range(n))
    del_len = int(edit[2])
    f = int(edit[1]) - f0
    ok = int(edit[0]) == contig and 0 <= f and f + del_len <= C_ and len(seq) == C_ and "N" not in seq
    text = ""
    if ok:
        e0 = C_ - f - del_len if strand else f
        ctx_text = _revcomp_text(seq) if strand else seq
        _, exists, _, _, text = prime_site_text(ctx_text, shape, e0, del_len, _revcomp_text(letters) if strand else letters)
        ok = exists
    if not ok and strict:
        raise ValueError("the edit is not in reach of the candidate, or the shape refuses the pair")
    return text if ok else ""


def prime_pick_inputs(pairs, loci, extra_columns=()):
    """What Genome.pick takes for "of every edit the K best pegRNAs": (loci[pairs.candidate], pairs.edit, key) - one pick
    candidate per prime pair, its target the pair's edit, its key made with pick_key.  The first columns are: the edit changes
    the PAM or the seed (1 bit, set is better: the edited strand is not nicked again); no poly-T terminator in the extension (1
    bit); 255 - t (8 bits: the shorter template).  extra_columns: (values per CANDIDATE of the prime call, bits) in priority
    order behind them - unsigned integer arrays, larger is better (pick_column makes them)."""
    pr = np.asarray(pairs, dtype=_lib.PRIME_PAIR_DTYPE)
    lo = _loci(loci, len(loci))
    cand = pr["candidate"].astype(np.int64)
    t, _, _, flags = unpack_prime_info(pr["info"])
    cols = [((flags & np.uint32(3)) != 0).astype(np.uint64), ((flags & np.uint32(4)) == 0).astype(np.uint64),
            np.uint64(255) - t.astype(np.uint64)]
    bits = [1, 1, 8]
    for values, b in extra_columns:
        v = np.asarray(values)
        if v.dtype.kind != "u" or v.ndim != 1 or len(v) != len(lo):
            raise ValueError("an extra column is a one-dimensional unsigned integer array with one value per candidate")
        cols.append(v[cand])
        bits.append(int(b))
    return lo[cand], pr["edit"].astype(np.uint32), pick_key(cols, bits)


# ---- HDR knock-in design ----------------------------------------------------------------------------------------
HDR_UNDEFINED = _lib.HDR_UNDEFINED  # both words of the row of a candidate whose context is undefined; "not in reach" of hdr_site_text
HDR_NO_BLOCK = _lib.HDR_NO_BLOCK    # the block word of a pair without a substitution
HDR_PAIR_DTYPE = _lib.HDR_PAIR_DTYPE
HDR_FLAGS = ("B_PAM", "B_SEED", "B_PROTO", "SUB_PAM", "SUB_SEED", "OPEN")  # bit k of a pair's flags
_IUPAC_SETS = {"A": 1, "C": 2, "G": 4, "T": 8, "R": 5, "Y": 10, "S": 6, "W": 9, "K": 12, "M": 3, "B": 14, "D": 13, "H": 11, "V": 7, "N": 15}


class HdrShape:
    """vsc_hdr_shape: how a cutting nuclease sits on a candidate, for knock-ins by homology-directed repair.  site_len 16..32 is
    the candidates' length, up / down (0..32 each) the bases of context in front of and behind the site in read orientation (C =
    up + site_len + down <= 64).  cut: the break lies in front of site position cut (17 for the SpCas9 23-mer); max_dist
    0..63: an edit further from the break is not in reach.  anchor: the side of the site the PAM fixes (1: its last base, 0: its
    first).  pam = (start, accept): accept one letter set per PAM position - an IUPAC string ("NGG") or numbers 1..15 (bit b =
    letter b of ACGT), at most 8.  seed / proto = (start, length) in site positions (at most 16 / 32 long); min_seed_mm /
    min_proto_mm: that many changed letters there keep the nuclease from cutting the repaired allele again (0: the rule is
    off).  substitute: look for one blocking substitution where the edit does not block; sub_seed: also in the seed;
    sub_noncoding: with a CDS, also outside its segments.  validate=False passes the numbers to the library as they are (tests)."""

    def __init__(self, site_len=READ_LEN, up=20, down=21, cut=17, max_dist=30, anchor=1, pam=(20, "NGG"), seed=(10, 10), proto=(0, 20),
                 min_seed_mm=2, min_proto_mm=4, substitute=True, sub_seed=True, sub_noncoding=True, flags=None, validate=True):
        self.site_len, self.up, self.down, self.cut = int(site_len), int(up), int(down), int(cut)
        self.max_dist, self.anchor = int(max_dist), int(anchor)
        self.pam_start = int(pam[0])
        acc = pam[1]
        if isinstance(acc, (str, bytes)):
            t = (acc.decode() if isinstance(acc, bytes) else acc).upper()
            if any(c not in _IUPAC_SETS for c in t):
                raise ValueError("a PAM is spelled in IUPAC letters")
            acc = [_IUPAC_SETS[c] for c in t]
        self.pam_accept = tuple(int(v) for v in acc)
        self.pam_len = len(self.pam_accept)
        self.seed_start, self.seed_len = int(seed[0]), int(seed[1])
        self.proto_start, self.proto_len = int(proto[0]), int(proto[1])
        self.min_seed_mm, self.min_proto_mm = int(min_seed_mm), int(min_proto_mm)
        self.flags = (int(bool(substitute)) | int(bool(sub_seed)) << 1 | int(bool(sub_noncoding)) << 2) if flags is None else int(flags)
        if validate and not self.valid():
            raise ValueError("an HDR shape has site_len 16..32, up and down 0..32, up + site_len + down <= 64, 1 <= cut <= site_len - 1, "
                             "max_dist 0..63, anchor 0 or 1, a PAM of at most 8 non-empty letter sets, a seed of at most 16 and a "
                             "protospacer of at most 32 positions, all inside the site, and thresholds of at most the ranges' lengths")

    def valid(self):
        def inside(start, length, most):
            return 0 <= length <= most and 0 <= start and start + length <= self.site_len
        return (16 <= self.site_len <= 32 and 0 <= self.up <= 32 and 0 <= self.down <= 32 and self.context_len <= 64
                and 1 <= self.cut <= self.site_len - 1 and 0 <= self.max_dist <= 63 and self.anchor in (0, 1)
                and inside(self.pam_start, self.pam_len, 8) and all(1 <= v <= 15 for v in self.pam_accept)
                and inside(self.seed_start, self.seed_len, 16) and inside(self.proto_start, self.proto_len, 32)
                and 0 <= self.min_seed_mm <= self.seed_len and 0 <= self.min_proto_mm <= self.proto_len and 0 <= self.flags <= 7)

    @property
    def context_len(self):
        return self.up + self.site_len + self.down

    def _struct(self, reserved=0):
        acc = (list(self.pam_accept) + [0] * 8)[:8]
        return _lib.HdrShapeStruct(self.up & 0xFFFFFFFF, self.site_len & 0xFFFFFFFF, self.down & 0xFFFFFFFF, self.cut & 0xFFFFFFFF,
                                   self.max_dist & 0xFFFFFFFF, self.anchor & 0xFFFFFFFF, self.pam_start & 0xFFFFFFFF,
                                   self.pam_len & 0xFFFFFFFF, (C.c_uint32 * 8)(*[v & 0xFFFFFFFF for v in acc]),
                                   self.seed_start & 0xFFFFFFFF, self.seed_len & 0xFFFFFFFF, self.proto_start & 0xFFFFFFFF,
                                   self.proto_len & 0xFFFFFFFF, self.min_seed_mm & 0xFFFFFFFF, self.min_proto_mm & 0xFFFFFFFF,
                                   self.flags & 0xFFFFFFFF, int(reserved))

    def __repr__(self):
        return "HdrShape(site_len=%d, up=%d, down=%d, cut=%d, max_dist=%d, anchor=%d, pam=(%d, %r), seed=(%d, %d), proto=(%d, %d), " \
               "min_seed_mm=%d, min_proto_mm=%d, flags=%d)" % (self.site_len, self.up, self.down, self.cut, self.max_dist, self.anchor,
                                                               self.pam_start, self.pam_accept, self.seed_start, self.seed_len,
                                                               self.proto_start, self.proto_len, self.min_seed_mm, self.min_proto_mm,
                                                               self.flags)


# Two presets.  SpCas9 on its 23-mer (20 protospacer bases, then NGG; the blunt break lies three bases in front of the PAM): the
# PAM-proximal 10 bases as the seed.  Cas12a on a 27-mer (TTTV, then 23 protospacer bases; the break is taken at the cut of the
# non-target strand, 18 bases behind the PAM): the 6 PAM-proximal bases as the seed.  Two seed or four protospacer mismatches
# count as a block, an edit up to 30 bases from the break as in reach.  Commonly used settings and nothing more.
HDR_NUCLEASES = {
    "SpCas9": HdrShape(READ_LEN, 20, 21, 17, 30, 1, (20, "NGG"), (10, 10), (0, 20), 2, 4),
    "Cas12a": HdrShape(27, 18, 19, 22, 30, 0, (0, "TTTV"), (4, 6), (4, 23), 2, 4),
}


def _hdr_shape(shape, what="shape"):
    if isinstance(shape, str):
        if shape not in HDR_NUCLEASES:
            raise ValueError("%s names one of %s, or is an HdrShape" % (what, ", ".join(sorted(HDR_NUCLEASES))))
        shape = HDR_NUCLEASES[shape]
    if not isinstance(shape, HdrShape):
        raise ValueError("%s must be an HdrShape or the name of a preset" % what)
    return shape


def unpack_hdr_info(info):
    """(dist, side, seed_mm, proto_mm, flags) of an HDR pair's info word (or an array of them): the bases between the break and
    the edit, the side the edit lies on (0: it spans the break, 1: in front of it, 2: behind it, in read orientation), the changed
    letters the nuclease finds in the seed and in the protospacer, and the flags (bit k: HDR_FLAGS[k])."""
    i = np.asarray(info, dtype=np.uint32)
    return (i & np.uint32(0x3F), (i >> np.uint32(6)) & np.uint32(3), (i >> np.uint32(8)) & np.uint32(0x1F),
            (i >> np.uint32(13)) & np.uint32(0x3F), i >> np.uint32(24))


def unpack_hdr_block(block):
    """(q, letter, coding, r, has) of an HDR pair's block word (or an array of them): the site position of the blocking
    substitution, the read letter 0..3 it writes, whether the base lies in a CDS segment, its reference context position - and
    has = False (the other four 0) where the pair carries no substitution."""
    b = np.asarray(block, dtype=np.uint32)
    has = b != np.uint32(HDR_NO_BLOCK)
    z = np.where(has, b, np.uint32(0))
    return z & np.uint32(0xFF), (z >> np.uint32(8)) & np.uint32(3), (z >> np.uint32(10)) & np.uint32(1), (z >> np.uint32(16)) & np.uint32(0xFF), has


def hdr_site_text(context, shape, e0, del_len=0, ins="", allowed=None):
    """vsc_hdr_site_text: one context of shape.context_len letters (any case) in read orientation and one edit in READ
    coordinates - read bases [e0, e0 + del_len) are replaced by the letters `ins` (as the read strand has them) - on the host, by
    the functions the kernels call.  allowed: None, or one letter set 0..15 per context position (ALLOWED of a substitution
    there).  Returns (in_reach, info, block, edited): in_reach False (info = block = HDR_UNDEFINED, edited = "") for an edit too
    far from the break; edited is E with the substitution applied.  A letter other than ACGT or a text of another length
    raises VarscotError."""
    b = context if isinstance(context, bytes) else context.encode()
    sh = _hdr_shape(shape)._struct()
    it = ins if isinstance(ins, bytes) else ins.encode()
    al = None
    if allowed is not None:
        al = np.ascontiguousarray(allowed, dtype=np.uint8)
        if len(al) != len(b):
            raise ValueError("one letter set per context position")
    pair = (C.c_uint32 * 2)()
    text = C.create_string_buffer(96)
    check(lib().vsc_hdr_site_text(b, C.byref(sh), int(e0), int(del_len), it, ptr(al), pair, text))
    reach = not (int(pair[0]) == HDR_UNDEFINED and int(pair[1]) == HDR_UNDEFINED)
    return reach, int(pair[0]), int(pair[1]), text.value.decode()


def hdr_pick_inputs(pairs, loci, extra_columns=()):
    """What Genome.pick takes for "of every edit the K best cutting guides": (loci[pairs.candidate], pairs.edit, key) - one pick
    candidate per HDR pair, its target the pair's edit, its key made with pick_key.  The first columns are: not OPEN (1 bit);
    BLOCKED by the edit itself (1 bit: the donor needs no further change); the substitution breaks the PAM (1 bit, before one in
    the seed); 63 - dist (6 bits: the nearer break).  extra_columns: (values per CANDIDATE of the HDR call, bits) in priority
    order behind them - unsigned integer arrays, larger is better (pick_column makes them)."""
    pr = np.asarray(pairs, dtype=_lib.HDR_PAIR_DTYPE)
    lo = _loci(loci, len(loci))
    cand = pr["candidate"].astype(np.int64)
    dist, _, _, _, flags = unpack_hdr_info(pr["info"])
    cols = [((flags & np.uint32(32)) == 0).astype(np.uint64), ((flags & np.uint32(7)) != 0).astype(np.uint64),
            ((flags & np.uint32(8)) != 0).astype(np.uint64), np.uint64(63) - dist.astype(np.uint64)]
    bits = [1, 1, 1, 6]
    for values, b in extra_columns:
        v = np.asarray(values)
        if v.dtype.kind != "u" or v.ndim != 1 or len(v) != len(lo):
            raise ValueError("an extra column is a one-dimensional unsigned integer array with one value per candidate")
        cols.append(v[cand])
        bits.append(int(b))
    return lo[cand], pr["edit"].astype(np.uint32), pick_key(cols, bits)


def hdr_donor(contig_text, locus, shape, edit, pair, arms=(40, 40)):
    """The donor of one HDR pair as forward DNA letters, on the host: the contig's text with the edit = (contig, pos, del_len,
    ins) and the pair's blocking substitution (if it has one) applied, cut to the span of the break, the edit and the
    substitution plus arms = (left, right) reference bases on either side - clipped at the contig's ends, and as long as the
    caller likes (they are not bound to the 64-base context).  locus = (contig, pos, strand) of the candidate; pair: an
    HDR_PAIR_DTYPE record or (info, block).  A pair whose substitution does not fit the locus and the edit raises ValueError."""
    shape = _hdr_shape(shape)
    pos, strand = int(locus[1]), int(locus[2])
    C_ = shape.context_len
    f0 = pos - (shape.down if strand else shape.up)
    K = shape.up + shape.cut
    brk = f0 + (C_ - K if strand else K)  # the break lies in front of this forward position
    e_pos, del_len = int(edit[1]), int(edit[2])
    n, code = _prime_ins(edit[3])
    letters = "".join("ACGT"[(code >> (2 * k)) & 3] for k in range(n))
    block = int(pair["block"]) if isinstance(pair, (np.void, np.ndarray)) else int(pair[1])
    text = contig_text.upper()
    if int(edit[0]) != int(locus[0]) or f0 < 0 or f0 + C_ > len(text) or e_pos + del_len > len(text):
        raise ValueError("the locus and the edit do not lie together on this contig")
    lo, hi = min(brk, e_pos), max(brk, e_pos + del_len)
    sub = None
    if block != HDR_NO_BLOCK:
        _, b, _, r, _ = (int(v) for v in unpack_hdr_block(block))
        f = f0 + (C_ - 1 - r if strand else r)
        if r >= C_ or e_pos <= f < e_pos + del_len:
            raise ValueError("the pair's substitution does not fit the locus and the edit")
        sub = (f, "ACGT"[3 - b if strand else b])
        lo, hi = min(lo, f), max(hi, f + 1)
    left, right = max(0, lo - int(arms[0])), min(len(text), hi + int(arms[1]))
    ref = list(text[left:right])
    if sub is not None:
        ref[sub[0] - left] = sub[1]
    return "".join(ref[:e_pos - left]) + letters + "".join(ref[e_pos + del_len - left:])


# ---- coding consequences of base edits --------------------------------------------------------------------
# CODE: 64 amino-acid letters indexed 16 b0 + 4 b1 + b2 (A C G T = 0 .. 3), '*' = stop - the standard genetic code
GENETIC_CODE = "KNKNTTTTRSRSIIMIQHQHPPPPRRRRLLLLEDEDAAAAGGGGVVVV*Y*YSSSS*CWCLFLF"
EFFECT_DTYPE = _lib.EFFECT_DTYPE
EFFECT_CLASSES = _lib.EFFECT_CLASS_NAMES  # the name of class k; the bit of a require / forbid mask
EFFECTS_UNDEFINED = _lib.EFFECTS_UNDEFINED  # both words of the row of a candidate whose site is undefined
# the base the presets of EDITORS write on the read strand
EDITOR_TO = {"CBE": "T", "ABE": "G"}


def _effect_to(shape, to):
    """`to` as 0..3: a letter, a number, or None - the transition partner of the shape's base (C <-> T, A <-> G)."""
    if to is None:
        return (shape.base + 2) % 4
    if isinstance(to, (str, bytes)):
        t = to.decode() if isinstance(to, bytes) else to
        if len(t) != 1 or t.upper() not in "ACGT":
            raise ValueError("an editor writes one of A, C, G, T")
        return "ACGT".index(t.upper())
    return int(to)


def _effect_code(code):
    """CODE as the library takes it: None (the standard code) or 64 letters."""
    if code is None:
        return None
    b = code if isinstance(code, bytes) else code.encode()
    if len(b) != 64:
        raise ValueError("a genetic code has 64 letters")
    return b


def effect_class_mask(classes):
    """The require / forbid mask of class names (EFFECT_CLASSES), one name or several; None: 0; a number passes as it is."""
    if classes is None:
        return 0
    if isinstance(classes, (int, np.integer)):
        return int(classes)
    if isinstance(classes, str):
        classes = [c for c in classes.split("+") if c]
    m = 0
    for c in classes:
        if c not in EFFECT_CLASSES:
            raise ValueError("an effect class is one of %s" % ", ".join(EFFECT_CLASSES))
        m |= 1 << EFFECT_CLASSES.index(c)
    return m


class Cds:
    """A CDS annotation to walk base edits against (vsc_cds): `segments` = (contig, start, end, transcript, strand, phase)
    rows - 0-based, half-open, on the forward genome; strand 0 / "+" or 1 / "-"; phase 0..2 as in GFF column 8 - or a
    CDS_SEGMENT_DTYPE array.  One transcript set: no two segments overlap.  sort=True (the default) orders the rows by
    (contig, start) first; the library refuses anything else that breaks SEGMENT / CODING of include/varscot_hip.h, and
    VarscotError then names the rule and the segment (its index after sorting).  n_tx defaults to the largest transcript +
    1.  Host-side and immutable, as Regions; every context that uses it keeps a device copy while it is the last one it used."""

    def __init__(self, packed_genome, segments, n_tx=None, sort=True):
        if isinstance(segments, np.ndarray) and segments.dtype == _lib.CDS_SEGMENT_DTYPE:
            sg = np.ascontiguousarray(segments).copy()
        else:
            rows = [tuple(r) for r in segments]
            sg = np.zeros(len(rows), dtype=_lib.CDS_SEGMENT_DTYPE)
            for i, r in enumerate(rows):
                if len(r) != 6:
                    raise ValueError("a segment is (contig, start, end, transcript, strand, phase)")
                strand = {"+": 0, "-": 1}.get(r[4], r[4])
                vals = [int(r[0]), int(r[1]), int(r[2]), int(r[3]), int(strand), int(r[5])]
                if min(vals) < 0 or max(vals) >= 2 ** 32:
                    raise ValueError("segment fields must fit 32 unsigned bits")
                sg[i] = (vals[0], vals[1], vals[2], vals[3], vals[4], vals[5], (0, 0))
        if sort and len(sg):
            sg = sg[np.lexsort((sg["start"], sg["contig"]))]
        self.segments = sg
        self.n_tx = int(n_tx) if n_tx is not None else (int(sg["transcript"].max()) + 1 if len(sg) else 0)
        contigs = np.ascontiguousarray(packed_genome.contigs, dtype=CONTIG_DTYPE)
        self._h = C.c_void_p()
        L = lib()
        rc = L.vsc_cds_build(ptr(contigs), len(contigs), ptr(sg) if len(sg) else None, len(sg), self.n_tx, C.byref(self._h))
        if rc != 0:
            raise _lib.VarscotError(rc, (L.vsc_cds_build_error() or b"").decode())

    def info(self):
        """vsc_cds_info: segments, transcripts (n_tx), transcripts_used and coding_bases."""
        st = _lib.CdsStats()
        check(lib().vsc_cds_info(self._h, C.byref(st)))
        return st.as_dict()

    def close(self):
        if self._h:
            lib().vsc_cds_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def codon_effect(ref, alt, codon, first_phase, code=None):
    """vsc_codon_effect: the class (0..5, EFFECT_CLASSES) of one effect by the function the kernels call.  ref, alt: codons as
    16 b0 + 4 b1 + b2 or three letters; codon: its index in the transcript; first_phase: the phase of the transcript's first
    segment."""
    def num(c):
        if isinstance(c, str):
            return 16 * "ACGT".index(c[0]) + 4 * "ACGT".index(c[1]) + "ACGT".index(c[2])
        return int(c)
    out = C.c_uint32()
    check(lib().vsc_codon_effect(num(ref), num(alt), int(codon), int(first_phase), _effect_code(code), C.byref(out)))
    return int(out.value)


def effects_site_text(cds, texts, contig, pos, strand, shape, to=None, code=None):
    """vsc_effects_site_text: (row uint32[2], effects EFFECT_DTYPE[..]) of the one site at (contig, pos, strand) from letters,
    on the host, by the functions the kernels call.  texts: the letters of every contig of the genome the Cds was built for."""
    if isinstance(shape, str):
        to = EDITOR_TO[shape] if to is None else to
        shape = EDITORS[shape]
    raw = [t if isinstance(t, bytes) else t.encode() for t in texts]
    arr = (C.c_char_p * max(len(raw), 1))(*raw)
    row = np.zeros(2, dtype=np.uint32)
    eff = np.zeros(16, dtype=_lib.EFFECT_DTYPE)
    n = C.c_uint32()
    sh = shape._struct()
    check(lib().vsc_effects_site_text(cds._h, arr, int(contig), int(pos), int(strand), C.byref(sh), _effect_to(shape, to), _effect_code(code),
                                      ptr(row), ptr(eff), C.byref(n)))
    return row, eff[:int(n.value)].copy()


def unpack_effect_info(info):
    """(ref, alt, class, edited, at) of an effect's info word (or an array of them): the codon before and after as
    16 b0 + 4 b1 + b2, the class (EFFECT_CLASSES), the edited bases in the codon and the smallest window position among them."""
    i = np.asarray(info, dtype=np.uint32)
    return (i & np.uint32(63), (i >> np.uint32(6)) & np.uint32(63), (i >> np.uint32(12)) & np.uint32(7),
            (i >> np.uint32(16)) & np.uint32(15), (i >> np.uint32(20)) & np.uint32(15))


def unpack_effect_row(rows):
    """(counts uint32[n, 6], coding uint32[n]) of effect rows uint32[n, 2]: the candidate's effects by class, and the bits
    of its MASK that lie in a segment.  An undefined row gives zeros."""
    r = np.asarray(rows, dtype=np.uint32).reshape(-1, 2)
    undefined = (r[:, 0] == EFFECTS_UNDEFINED) & (r[:, 1] == EFFECTS_UNDEFINED)
    counts = np.stack([(r[:, 0] >> np.uint32(5 * k)) & np.uint32(31) for k in range(6)], axis=1).astype(np.uint32)
    counts[undefined] = 0
    return counts, np.where(undefined, np.uint32(0), r[:, 1]).astype(np.uint32)


def codon_text(codon):
    """The three letters of a codon number 16 b0 + 4 b1 + b2."""
    c = int(codon)
    return "ACGT"[c >> 4 & 3] + "ACGT"[c >> 2 & 3] + "ACGT"[c & 3]


def effects_pick_inputs(effects, loci, classes=("stop_gained",), extra_columns=()):
    """What Genome.pick takes for "of every transcript the K guides whose effect of `classes` comes earliest in the protein":
    (loci[effects.candidate], effects.transcript, key) over the effects of those classes - one pick candidate per effect, its
    target the effect's transcript, its key made with pick_key so that an earlier codon is better: the first column is
    2^31 - 1 - codon (31 bits).  extra_columns: (values per CANDIDATE of the effects call, bits) in priority order behind it
    - unsigned integer arrays, larger is better (pick_column makes them)."""
    ef = np.asarray(effects, dtype=_lib.EFFECT_DTYPE)
    want = effect_class_mask(classes)
    cls = (ef["info"] >> np.uint32(12)) & np.uint32(7)
    ef = ef[((np.uint32(1) << cls) & np.uint32(want)) != 0]
    lo = _loci(loci, len(loci))
    cand = ef["candidate"].astype(np.int64)
    cols = [np.uint64(2 ** 31 - 1) - ef["codon"].astype(np.uint64)]
    bits = [31]
    for values, b in extra_columns:
        v = np.asarray(values)
        if v.dtype.kind != "u" or v.ndim != 1 or len(v) != len(lo):
            raise ValueError("an extra column is a one-dimensional unsigned integer array with one value per candidate")
        cols.append(v[cand])
        bits.append(int(b))
    return lo[cand], ef["transcript"].astype(np.uint32), pick_key(cols, bits)


# ---- knock-out design: cut position, frameshift stops, NMD ----------------------------------------------------
KNOCKOUT_UNDEFINED = _lib.KNOCKOUT_UNDEFINED  # all four words of the row of a candidate that is not defined
KNOCKOUT_END, KNOCKOUT_CAP, KNOCKOUT_UNKNOWN = _lib.KNOCKOUT_END, _lib.KNOCKOUT_CAP, _lib.KNOCKOUT_UNKNOWN  # d1 / d2 without a stop
KNOCKOUT_FLAGS = _lib.KNOCKOUT_FLAG_NAMES  # the name of flag bit k of a row; the bit of a require / forbid mask
KNOCKOUT_ROW_DTYPE = np.dtype([("transcript", "<u4"), ("codon", "<u4"), ("frame", "u1"), ("frac", "<u2"), ("edge", "u1"), ("flags", "u1"),
                               ("d1", "<u2"), ("d2", "<u2"), ("coding", "?"), ("defined", "?")])


class KnockoutShape:
    """vsc_knockout_shape: where a nuclease cuts and what counts as a knock-out.  site_len 16..32 is the candidates' length (23
    for enumerate_guides', the pattern's for enumerate_pattern's); cut 1..site_len - 1: the break lies between read positions
    cut - 1 and cut of the site (SpCas9: 17; Cas12a TTTV + 23: 22); nmd_window 0..65535: a premature stop triggers
    nonsense-mediated decay when it ends at least that many coding bases in front of the last exon-exon junction (the 50-55 nt
    rule); start_window 0..65535: and begins at least that many coding bases behind the transcript's first one (0: the rule is
    off); max_codons 1..4096: how far a walk looks for a stop.  KNOCKOUT_SHAPES holds the preset "SpCas9" (23, 17, 50, 0,
    4096).  validate=False passes the numbers to the library as they are (tests)."""

    def __init__(self, site_len=READ_LEN, cut=17, nmd_window=50, start_window=0, max_codons=4096, validate=True):
        self.site_len, self.cut, self.nmd_window = int(site_len), int(cut), int(nmd_window)
        self.start_window, self.max_codons = int(start_window), int(max_codons)
        if validate and not (16 <= self.site_len <= 32 and 1 <= self.cut < self.site_len and 0 <= self.nmd_window <= 65535
                             and 0 <= self.start_window <= 65535 and 1 <= self.max_codons <= 4096):
            raise ValueError("a knock-out shape has site_len 16..32, cut 1..site_len - 1, windows 0..65535 and max_codons 1..4096")

    def _struct(self):
        return _lib.KnockoutShapeStruct(self.site_len, self.cut, self.nmd_window, self.start_window, self.max_codons,
                                        (C.c_uint32 * 3)(0, 0, 0))

    def __repr__(self):
        return "KnockoutShape(site_len=%d, cut=%d, nmd_window=%d, start_window=%d, max_codons=%d)" % (
            self.site_len, self.cut, self.nmd_window, self.start_window, self.max_codons)


KNOCKOUT_SHAPES = {"SpCas9": KnockoutShape(READ_LEN, 17, 50, 0, 4096)}


def _knockout_shape(shape, what="shape"):
    if isinstance(shape, str):
        if shape not in KNOCKOUT_SHAPES:
            raise ValueError("%s names one of %s, or is a KnockoutShape" % (what, ", ".join(sorted(KNOCKOUT_SHAPES))))
        shape = KNOCKOUT_SHAPES[shape]
    if not isinstance(shape, KnockoutShape):
        raise ValueError("%s must be a KnockoutShape or the name of a preset" % what)
    return shape


def knockout_flag_mask(flags):
    """The require / forbid mask of flag names (KNOCKOUT_FLAGS), one name, several joined by "+", or a list; None: 0; a number
    passes as it is."""
    if flags is None:
        return 0
    if isinstance(flags, (int, np.integer)):
        return int(flags)
    if isinstance(flags, str):
        flags = [f for f in flags.split("+") if f]
    m = 0
    for f in flags:
        if f not in KNOCKOUT_FLAGS:
            raise ValueError("a knock-out flag is one of %s" % ", ".join(KNOCKOUT_FLAGS))
        m |= 1 << KNOCKOUT_FLAGS.index(f)
    return m


def knockout_cut_frac(share, upper=False):
    """A share of the protein (0 .. 1) in the units of a row's frac (0 .. 65535), the rule of min_cut_frac= / max_cut_frac=:
    a lower bound becomes ceil(65536 x share), an upper bound floor(65536 x share), both capped at 65535 - so that the bounds
    keep exactly the cuts K with share_min <= (K - shift) / B_t <= share_max up to frac's own rounding down."""
    x = float(share)
    if not 0.0 <= x <= 1.0:
        raise ValueError("a share of the protein lies in 0 .. 1")
    v = int(np.floor(65536.0 * x)) if upper else int(np.ceil(65536.0 * x))
    return min(v, 65535)


def knockout_site_text(cds, texts, contig, pos, strand, shape, code=None):
    """vsc_knockout_site_text: the row (uint32[4]) of the one site at (contig, pos, strand) from letters, on the host, by the
    functions the kernels call.  texts: the letters of every contig of the genome the Cds was built for."""
    shape = _knockout_shape(shape)
    raw = [t if isinstance(t, bytes) else t.encode() for t in texts]
    arr = (C.c_char_p * max(len(raw), 1))(*raw)
    row = np.zeros(4, dtype=np.uint32)
    sh = shape._struct()
    check(lib().vsc_knockout_site_text(cds._h, arr, int(contig), int(pos), int(strand), C.byref(sh), _effect_code(code), ptr(row)))
    return row


def unpack_knockout_row(rows):
    """Knock-out rows uint32[n, 4] (or one row) as a KNOCKOUT_ROW_DTYPE array: transcript, codon, frame, frac (0..65535 along
    the protein), edge (bases to the nearer end of the segment, capped at 255), flags (bit k: KNOCKOUT_FLAGS[k]), d1, d2 (codons
    from the cut's codon to the first stop in frame +1 / +2; KNOCKOUT_END / KNOCKOUT_CAP / KNOCKOUT_UNKNOWN), coding, defined.
    A row that is not defined, or not a coding cut, has zeros but for flags bit 7 = JUNCTION of a non-coding cut."""
    r = np.asarray(rows, dtype=np.uint32).reshape(-1, 4)
    out = np.zeros(len(r), dtype=KNOCKOUT_ROW_DTYPE)
    defined = ~np.all(r == np.uint32(KNOCKOUT_UNDEFINED), axis=1)
    coding = defined & (r[:, 0] != np.uint32(0xFFFFFFFF))
    out["defined"], out["coding"] = defined, coding
    out["transcript"] = np.where(coding, r[:, 0], 0)
    out["codon"] = np.where(coding, r[:, 1] & np.uint32(0x3FFFFFFF), 0)
    out["frame"] = np.where(coding, r[:, 1] >> np.uint32(30), 0)
    out["frac"] = np.where(coding, r[:, 2] & np.uint32(0xFFFF), 0)
    out["edge"] = np.where(coding, (r[:, 2] >> np.uint32(16)) & np.uint32(0xFF), 0)
    out["flags"] = np.where(defined, r[:, 2] >> np.uint32(24), 0)
    out["d1"] = np.where(coding, r[:, 3] & np.uint32(0xFFFF), 0)
    out["d2"] = np.where(coding, r[:, 3] >> np.uint32(16), 0)
    return out


def _region_filter(regions, scope):
    """(vsc_region_filter or None) for search_select's regions / region_scope arguments."""
    if regions is None:
        return None
    if scope not in ("keep", "drop"):
        raise ValueError("region_scope must be 'keep' or 'drop'")
    return _lib.RegionFilter(regions._h, _lib.REGION_DROP if scope == "drop" else _lib.REGION_KEEP, 0)


class Regions:
    """An annotation to test hits against (vsc_regions): `intervals` = (contig, start, end) triples - 0-based, half-open, on
    the forward genome as in BED; unsorted, overlapping, nested as they come - or an INTERVAL_DTYPE array.  A hit is in the
    regions when its 23-base window shares a base with some interval (rule="overlap") or lies fully inside one interval
    (rule="inside", the reference's filterRefAlignment test).  Host-side and immutable; every context that uses it keeps a
    device copy while it is the last one it used."""

    def __init__(self, packed_genome, intervals, rule="overlap"):
        if rule not in ("overlap", "inside"):
            raise ValueError("rule must be 'overlap' or 'inside'")
        if isinstance(intervals, np.ndarray) and intervals.dtype == _lib.INTERVAL_DTYPE:
            iv = np.ascontiguousarray(intervals)
        else:
            a = np.asarray(intervals, dtype=np.int64).reshape(-1, 3)
            if len(a) and (a.min() < 0 or a.max() >= 2 ** 32):
                raise ValueError("interval fields must fit 32 unsigned bits")
            iv = np.zeros(len(a), dtype=_lib.INTERVAL_DTYPE)
            iv["contig"], iv["start"], iv["end"] = a[:, 0], a[:, 1], a[:, 2]
        contigs = np.ascontiguousarray(packed_genome.contigs, dtype=CONTIG_DTYPE)
        self.rule = rule
        self.n_intervals = len(iv)
        self._h = C.c_void_p()
        check(lib().vsc_regions_build(ptr(contigs), len(contigs), ptr(iv), len(iv),
                                      _lib.REGION_INSIDE if rule == "inside" else _lib.REGION_OVERLAP, C.byref(self._h)))

    def contains(self, contig, pos):
        """Is the window that starts at (contig, pos) in the regions?  (vsc_regions_contains, on the host)"""
        return bool(lib().vsc_regions_contains(self._h, int(contig), int(pos)))

    def locate(self, contig, pos):
        """The label of the window that starts at (contig, pos): the index in `intervals` of the most specific interval it is
        in - largest start, then smallest end, then first given - or REGION_NONE.  (vsc_regions_locate, on the host)"""
        return int(lib().vsc_regions_locate(self._h, int(contig), int(pos)))

    def info(self):
        """vsc_regions_info: intervals kept, rule, block_bases and the class table's blocks_out / blocks_in / blocks_mixed."""
        st = _lib.RegionsStats()
        check(lib().vsc_regions_info(self._h, C.byref(st)))
        return st.as_dict()

    def close(self):
        if self._h:
            lib().vsc_regions_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class VariantMap:
    """The ids of a variant-window genome parsed for the merge (vsc_variant_map): per window the reference contig of its
    chromosome, its start and its variants.  windows_genome: the PackedGenome variant_windows returned (its `names` are the ids),
    reference: the PackedGenome the windows were built from.  Host-side and immutable, as Regions; a context keeps a device copy
    while it is the last map it merged against."""

    def __init__(self, windows_genome, reference):
        names = windows_genome.names
        n = len(names)
        if isinstance(names, LazyNames):  # the library's own pool, as it is
            pool, offsets = np.ascontiguousarray(names._pool), np.ascontiguousarray(names._off, dtype=np.uint64)
        else:
            raw = [x.encode() + b"\n" for x in names]
            pool = np.frombuffer(b"".join(raw) or b"\n", dtype=np.uint8).copy()
            offsets = np.concatenate([[0], np.cumsum([len(x) for x in raw])]).astype(np.uint64)
        contigs = np.ascontiguousarray(windows_genome.contigs, dtype=CONTIG_DTYPE)
        if len(contigs) != n:
            raise ValueError("the window genome has %d contigs and %d names" % (len(contigs), n))
        ref_contigs = np.ascontiguousarray(reference.contigs, dtype=CONTIG_DTYPE)
        ref_names = (C.c_char_p * len(reference.names))(*[x.encode() for x in reference.names])
        self.n_windows = n
        self._h = C.c_void_p()
        check(lib().vsc_variant_map_build(ptr(pool), ptr(offsets), ptr(contigs), n, ptr(ref_contigs), ref_names, len(ref_contigs),
                                          C.byref(self._h)))

    def shadow(self):
        """vsc_variant_map_shadow: the INSIDE-rule Regions over the reference that filterRefAlignment tests reference hits
        against - a reference hit in them is shadowed by a window."""
        r = Regions.__new__(Regions)
        r.rule = "inside"
        r._h = C.c_void_p()
        check(lib().vsc_variant_map_shadow(self._h, C.byref(r._h)))
        return r

    def locate(self, window, pos, length=23):
        """vsc_variant_map_locate (length = 23) / vsc_variant_map_locate_len (a site of `length` = 16..32 bases): the
        VARIANT_LABEL_DTYPE record of the window position - reference contig (0xFFFFFFFF: unknown), position on the chromosome,
        covered variants, VARIANT_VAR."""
        out = np.zeros(1, dtype=_lib.VARIANT_LABEL_DTYPE)
        if int(length) == READ_LEN:
            check(lib().vsc_variant_map_locate(self._h, int(window), int(pos), ptr(out)))
        else:
            check(lib().vsc_variant_map_locate_len(self._h, int(window), int(pos), int(length), ptr(out)))
        return out[0]

    def tag(self, window, pos, length=23):
        """vsc_variant_map_tag / vsc_variant_map_tag_len: "REF" or "VAR_<chr>_<positions of the covered variants>" of the site of
        `length` bases at the window position."""
        if int(length) == READ_LEN:
            call = lambda buf, n: lib().vsc_variant_map_tag(self._h, int(window), int(pos), buf, n)
        else:
            call = lambda buf, n: lib().vsc_variant_map_tag_len(self._h, int(window), int(pos), int(length), buf, n)
        n = int(call(None, 0))
        if n < 0:
            check(n)
        buf = C.create_string_buffer(n + 1)
        call(buf, n + 1)
        return buf.value.decode()

    def shadows(self, contig, pos, length):
        """vsc_variant_map_shadows: do the `length` bases from `pos` of reference contig `contig` on lie inside one window's
        interval - is a reference hit there shadowed by a window?"""
        r = int(lib().vsc_variant_map_shadows(self._h, int(contig), int(pos), int(length)))
        if r < 0:
            check(r)
        return bool(r)

    def info(self):
        """vsc_variant_map_info: windows, variants, unknown_chr (windows of a chromosome the reference does not have),
        max_variants (most variants in one window)."""
        st = _lib.VariantMapStats()
        check(lib().vsc_variant_map_info(self._h, C.byref(st)))
        return st.as_dict()

    def close(self):
        if self._h:
            lib().vsc_variant_map_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def individual_pattern_rows(ref, win):
    """A guide's rows in the individual's genome: the reference side's counted rows plus the window side's (the `ref` and `win`
    arrays of pattern_variants_screen, or its `ref_table` and `win_table`), field by field; on_target: met on either side;
    `dropped` / `reserved` stay 0.  Rows of either dtype in, the same dtype out."""
    out = np.zeros(len(ref), dtype=ref.dtype)
    for f in ref.dtype.names:
        if f == "on_target":
            out[f] = (ref[f] != 0) | (win[f] != 0)
        elif f not in ("dropped", "reserved"):
            out[f] = ref[f] + win[f]
    return out


def pattern_variants_screen(ref_genome, win_genome, vmap, pattern, guides, max_mismatches, table=None, exclude=None, chunk=0, guide_batch=0,
                            max_hits=0):
    """vsc_search_pattern_variants: the pattern search of both genomes of an individual - ref_genome, the resident reference, and
    win_genome, the resident variant windows built with seq_len = len(pattern) - merged per guide on the device.  Returns a dict
    of PATTERN_VARIANT_ROW_DTYPE arrays "ref" (counted reference hits; dropped = shadowed by a window), "win" (counted window
    hits; dropped = duplicates), "var" (the window hits that carry a variant) and, with a PatternTable, TABLE_ROW_DTYPE arrays
    "ref_table", "win_table", "var_table" over the same records (None without a table).  exclude: None or one (contig, pos,
    strand) per guide in reference coordinates; chunk: guides per search (0: 64) - the rows depend neither on it nor on
    guide_batch; max_hits caps a chunk's records per side.  win_genome = None with a map without windows (a sample without alt
    alleles): the reference side alone."""
    p = pattern if isinstance(pattern, bytes) else pattern.encode()
    gs = [g if isinstance(g, bytes) else g.encode() for g in guides]
    for i, g in enumerate(gs):
        if len(g) != len(p):
            raise ValueError("guide %d has %d letters; the pattern has %d" % (i, len(g), len(p)))
    n = len(gs)
    pp = _lib.PatternParams(int(max_mismatches), int(guide_batch), int(max_hits))
    ex = _loci(exclude, n)
    out = {k: np.zeros(n, dtype=_lib.PATTERN_VARIANT_ROW_DTYPE) for k in ("ref", "win", "var")}
    for k in ("ref_table", "win_table", "var_table"):
        out[k] = np.zeros(n, dtype=_lib.TABLE_ROW_DTYPE) if table is not None else None
    ctx = ref_genome.ctx
    check(lib().vsc_search_pattern_variants(ctx._h, ref_genome._h, win_genome._h if win_genome is not None else None, vmap._h, p, b"".join(gs), n, len(p), C.byref(pp),
                                            table._h if table is not None else None, ptr(ex), int(chunk), ptr(out["ref"]), ptr(out["win"]),
                                            ptr(out["var"]), ptr(out["ref_table"]), ptr(out["win_table"]), ptr(out["var_table"])), ctx._h)
    return out


def individual_rows(ref_all, ref_in, win_all):
    """A guide's rows in the individual's genome: the reference hits no window shadows (ref_all - ref_in of
    Genome.summarize(..., regions=vmap.shadow())) plus the counted window hits (Genome.summarize_variants' `all` rows), field
    by field; on_target: met on either side.  SUMMARY_DTYPE rows in, SUMMARY_DTYPE rows out."""
    out = np.zeros(len(ref_all), dtype=_lib.SUMMARY_DTYPE)
    for f in ("mit_sum", "nm", "mit_ub"):
        out[f] = ref_all[f] - ref_in[f] + win_all[f]
    out["on_target"] = (ref_all["on_target"] != 0) | (win_all["on_target"] != 0)
    return out


class PackedGenome:
    """The host-side packed planes of a genome (0.375 byte per base) plus its contig table.

    Counterpart of the reference's on-disk index (read_mapping/bidir_index.cpp) - here three bit
    planes (hi, lo, nmask) over one global coordinate space, see include/varscot_hip.h.
    """

    def __init__(self, hi, lo, nmask, contigs, names=None):
        self.hi, self.lo, self.nmask = hi, lo, nmask
        self.contigs = np.ascontiguousarray(contigs, dtype=CONTIG_DTYPE)
        self.names = list(names) if names is not None else ["contig%d" % i for i in range(len(self.contigs))]

    @property
    def n_words(self):
        return len(self.hi)

    @property
    def n_bases(self):
        return int(self.contigs["length"].sum())

    @classmethod
    def from_sequences(cls, seqs, names=None):
        L = lib()
        bufs = [s if isinstance(s, bytes) else s.encode() for s in seqs]
        lens = np.array([len(b) for b in bufs], dtype=np.uint32)
        table = np.zeros(len(bufs), dtype=CONTIG_DTYPE)
        n_words = int(L.vsc_layout_contigs(ptr(lens), len(bufs), ptr(table)))
        n_words = max(n_words, 1)
        hi = np.empty(n_words, dtype=np.uint32)
        lo = np.empty(n_words, dtype=np.uint32)
        nm = np.empty(n_words, dtype=np.uint32)
        L.vsc_planes_init(ptr(hi), ptr(lo), ptr(nm), n_words)
        for b, row in zip(bufs, table):
            L.vsc_pack_bases(b, len(b), int(row["offset"]), ptr(hi), ptr(lo), ptr(nm))
        return cls(hi, lo, nm, table, names)

    @classmethod
    def from_index_file(cls, prefix):
        """Reads <prefix>.vsc as written by the bidir_index tool (tools/vsc_host.hpp)."""
        with open(prefix + ".vsc", "rb") as f:
            magic = f.read(8)
            assert magic in (b"VSCIDX01", b"VSCIDX02"), "not a packed genome"
            nc, nw = (int(x) for x in np.frombuffer(f.read(16), dtype="<u8"))
            if magic == b"VSCIDX02":
                f.read(16)  # size and modification time of the FASTA it was packed from
            table = np.frombuffer(f.read(nc * CONTIG_DTYPE.itemsize), dtype=CONTIG_DTYPE).copy()
            names, name_bytes = [], 0
            for _ in range(nc):
                ln = int(np.frombuffer(f.read(4), dtype="<u4")[0])
                names.append(f.read(ln).decode())
                name_bytes += 4 + ln
            if magic == b"VSCIDX02":
                f.read((8 - name_bytes % 8) % 8)  # the planes start 8-byte aligned
            hi = np.frombuffer(f.read(nw * 4), dtype="<u4").copy()
            lo = np.frombuffer(f.read(nw * 4), dtype="<u4").copy()
            nm = np.frombuffer(f.read(nw * 4), dtype="<u4").copy()
        return cls(hi, lo, nm, table, names)

    def decode(self, pos, n):
        """n characters starting at global position pos (N outside contigs)."""
        out = C.create_string_buffer(n)
        lib().vsc_unpack_bases(ptr(self.hi), ptr(self.lo), ptr(self.nmask), pos, n, out)
        return out.raw.decode()

    def contig_sequence(self, c):
        row = self.contigs[c]
        return self.decode(int(row["offset"]), int(row["length"]))

    def shard_words(self, rank, world):
        """Tile-aligned word range [begin, end) of the planes that rank `rank` of `world` owns."""
        tiles = (self.n_words + TILE_WORDS - 1) // TILE_WORDS
        b = (tiles * rank // world) * TILE_WORDS
        e = (tiles * (rank + 1) // world) * TILE_WORDS
        return min(b, self.n_words), min(e, self.n_words)


class Context:
    """One device + one stream (vsc_ctx).  Single-threaded."""

    def __init__(self, device=0, cu_mask=None):
        """cu_mask (experiments, include/varscot_hip_debug.h): uint32 words, bit i of word i // 32 = compute unit i may be used."""
        self._h = C.c_void_p()
        if cu_mask is None:
            check(lib().vsc_ctx_create(device, C.byref(self._h)))
        else:
            mask = np.ascontiguousarray(cu_mask, dtype=np.uint32)
            check(lib().vsc_ctx_create_masked(device, mask.ctypes.data, len(mask), C.byref(self._h)))
        self.device = device
        self._children = weakref.WeakSet()  # genomes and results must go before their context

    def close(self):
        if self._h:
            for child in sorted(self._children, key=lambda c: isinstance(c, Genome)):
                child.close()  # results first, then genomes
            lib().vsc_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, hip_stream_handle):
        check(lib().vsc_ctx_set_stream(self._h, C.c_void_p(hip_stream_handle)), self._h)

    def timing(self):
        t = Timing()
        check(lib().vsc_ctx_timing(self._h, C.byref(t)), self._h)
        return t.as_dict()

    def release_scratch(self):
        """vsc_ctx_release_scratch: give the pooled scratch and record buffers back to the device."""
        check(lib().vsc_ctx_release_scratch(self._h), self._h)

    def set_debug(self, **hooks):
        """Test / experiment hooks of include/varscot_hip_debug.h (vsc_ctx_set_debug_params): e.g.
        set_debug(sort_cap=16) forces many sort levels on a few thousand records.  No arguments: back to the
        defaults.  The library reads no environment variable."""
        d = _lib.DebugParams.defaults()
        for k, v in hooks.items():
            if k not in dict(_lib.DebugParams._fields_) or k == "reserved":
                raise TypeError("unknown debug hook %r" % k)
            setattr(d, k, int(v))
        check(lib().vsc_ctx_set_debug_params(self._h, C.byref(d) if hooks else None), self._h)

    def load_genome(self, packed, rank=0, world=1):
        return Genome(self, packed, rank, world)

    def score_pairs(self, on_targets, off_targets, masks, mit=True, features=False):
        """vsc_score_pairs: MIT score / feature rows of explicit (on-target, off-target) 23-mer pairs."""
        on = np.ascontiguousarray(on_targets if isinstance(on_targets, np.ndarray) else pack_guides(on_targets), dtype=np.uint64)
        off = np.ascontiguousarray(off_targets if isinstance(off_targets, np.ndarray) else pack_guides(off_targets), dtype=np.uint64)
        mk = np.ascontiguousarray(masks, dtype=np.uint32)
        n = len(on)
        assert len(off) == n and len(mk) == n
        m = np.empty(n, dtype=np.float64) if mit else None
        fl = np.empty(n, dtype=np.uint8) if mit else None
        ft = np.empty((n, N_FEATURES), dtype=np.uint8) if features else None
        check(lib().vsc_score_pairs(self._h, ptr(on), ptr(off), ptr(mk), n, ptr(m), ptr(fl), ptr(ft)), self._h)
        return m, fl, ft


class Genome:
    """(A shard of) a packed genome resident in HBM (vsc_genome)."""

    def __init__(self, ctx, packed, rank=0, world=1):
        b, e = packed.shard_words(rank, world)
        if e <= b:
            raise ValueError("rank %d of %d owns no words of this genome" % (rank, world))
        halo_end = min(e + 1, packed.n_words)  # 22-base halo = 1 word
        self._load(ctx, packed.hi[b:halo_end], packed.lo[b:halo_end], packed.nmask[b:halo_end], b, e - b,
                   packed.contigs)
        self.packed = packed

    @classmethod
    def from_shard(cls, ctx, hi, lo, nmask, first_word, own_words, contigs):
        """Planes of words [first_word, first_word + len(hi)) of which the first own_words are owned."""
        self = cls.__new__(cls)
        self.packed = None
        self._load(ctx, hi, lo, nmask, first_word, own_words, contigs)
        return self

    def _load(self, ctx, hi, lo, nm, first_word, own_words, contigs):
        self.ctx = ctx
        self.first_word, self.own_words = first_word, own_words
        hi = np.ascontiguousarray(hi, dtype=np.uint32)
        lo = np.ascontiguousarray(lo, dtype=np.uint32)
        nm = np.ascontiguousarray(nm, dtype=np.uint32)
        contigs = np.ascontiguousarray(contigs, dtype=CONTIG_DTYPE)
        self._h = C.c_void_p()
        check(lib().vsc_genome_load(ctx._h, ptr(hi), ptr(lo), ptr(nm), first_word, len(hi), own_words, ptr(contigs),
                                    len(contigs), C.byref(self._h)), ctx._h)
        ctx._children.add(self)

    @property
    def device_bytes(self):
        return int(lib().vsc_genome_device_bytes(self._h))

    def close(self):
        if self._h:
            lib().vsc_genome_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _params(max_mismatches, extra_pam, algorithm):
        p = SearchParams()
        p.max_mismatches = max_mismatches
        p.algorithm = {"auto": ALGO_AUTO, "scan": ALGO_SCAN, "seed": ALGO_SEED}.get(algorithm, algorithm)
        if extra_pam:
            e = extra_pam if isinstance(extra_pam, bytes) else extra_pam.encode()
            if len(e) != 2:
                raise ValueError("the additional PAM (-P) must be 2 letters")
            p.has_extra_pam = 1
            p.extra_pam = e
        return p

    def build_index(self, extra_pam=None):
        """Build the seed index now (vsc_genome_build_index); searches build it on demand otherwise."""
        p = self._params(0, extra_pam, ALGO_SEED)
        check(lib().vsc_genome_build_index(self.ctx._h, self._h, C.byref(p)), self.ctx._h)

    def save_index(self, path):
        """Write the resident seed index to a file (vsc_genome_index_save)."""
        check(lib().vsc_genome_index_save(self.ctx._h, self._h, os.fsencode(path)), self.ctx._h)

    def load_index(self, path):
        """Replace the seed index by a file's (vsc_genome_index_load); refused if it belongs to another genome."""
        check(lib().vsc_genome_index_load(self.ctx._h, self._h, os.fsencode(path)), self.ctx._h)

    def search(self, guides, max_mismatches, extra_pam=None, algorithm="auto"):
        """guides: list of 23-nt strings or a uint64 array from pack_guides().
        algorithm: "auto" | "scan" | "seed" - same records either way (see include/varscot_hip.h)."""
        codes = guides if isinstance(guides, np.ndarray) else pack_guides(guides)
        codes = np.ascontiguousarray(codes, dtype=np.uint64)
        p = self._params(max_mismatches, extra_pam, algorithm)
        h = C.c_void_p()
        check(lib().vsc_search(self.ctx._h, self._h, ptr(codes), len(codes), C.byref(p), C.byref(h)), self.ctx._h)
        return Hits(self, h, codes)

    def search_bulges(self, guides, max_mismatches, dna=1, rna=1, extra_pam=None, max_hits=0, guide_batch=0, records=True,
                      rows=True, table=None):
        """vsc_search_bulges: the sites of 23 + d bases, d in -rna .. -1 and 1 .. dna, that pair with a guide within
        max_mismatches when one or two bases of the site (DNA bulge) or of the guide (RNA bulge) stay unpaired.  The bulged
        neighbours of plain hits are among them; d = 0 is search()'s.  Returns (BULGE_HIT_DTYPE records in ascending (guide,
        strand, contig, pos, d) order | None, uint32 rows of shape (n, 4, 9) - hits by class (RNA 2, RNA 1, DNA 1, DNA 2) and
        NM | None).  max_hits: 0 = no cap, else VSC_ERR_RANGE when there are more records; guide_batch never changes the result.
        table: a BulgeTable of 23 letters - the return gains (uint32 f per record | None, TABLE_ROW_DTYPE rows | None), scored by
        vsc_bulge_hits_table over the records where they lie."""
        codes = guides if isinstance(guides, np.ndarray) else pack_guides(guides)
        codes = np.ascontiguousarray(codes, dtype=np.uint64)
        p = self._params(max_mismatches, extra_pam, ALGO_SCAN)
        bp = _lib.BulgeParams(int(dna), int(rna), int(guide_batch), 0, int(max_hits))
        L = lib()
        h = C.c_void_p()
        out_rows = np.zeros((len(codes), _lib.BULGE_CLASSES, 9), dtype=np.uint32) if rows else None
        check(L.vsc_search_bulges(self.ctx._h, self._h, ptr(codes), len(codes), C.byref(p), C.byref(bp),
                                  C.byref(h) if records or table is not None else None, ptr(out_rows)), self.ctx._h)
        if table is not None:
            try:
                fixed, table_rows = self._bulge_scores(h, [t.encode() for t in unpack_guides(codes)], table, records, rows)
            except Exception:
                L.vsc_bulge_hits_free(h)
                raise
            if not records:
                L.vsc_bulge_hits_free(h)
                return None, out_rows, None, table_rows
            return self._bulge_records(h) + (out_rows, fixed, table_rows)
        if not records:
            return None, out_rows
        return self._bulge_records(h) + (out_rows,)

    def search_pattern(self, pattern, guides, max_mismatches, max_hits=0, guide_batch=0, records=True, rows=True):
        """vsc_search_pattern: the sites of len(pattern) = 16..32 bases that satisfy the IUPAC pattern, hold no N and differ
        from a guide in at most max_mismatches positions; a guide's N positions are not compared.  guides: strings of the
        pattern's length (PATTERNS / pattern_strings make both from a protospacer).  Returns (PATTERN_HIT_DTYPE records in
        ascending (guide, strand, contig, pos) order | None, uint32 rows of shape (n, 9) - hits by NM | None).  max_hits: 0 = no
        cap, else VSC_ERR_RANGE when there are more records; guide_batch never changes the result."""
        p = pattern if isinstance(pattern, bytes) else pattern.encode()
        gs = [g if isinstance(g, bytes) else g.encode() for g in guides]
        for i, g in enumerate(gs):
            if len(g) != len(p):
                raise ValueError("guide %d has %d letters; the pattern has %d" % (i, len(g), len(p)))
        pp = _lib.PatternParams(int(max_mismatches), int(guide_batch), int(max_hits))
        L = lib()
        h = C.c_void_p()
        out_rows = np.zeros((len(gs), 9), dtype=np.uint32) if rows else None
        check(L.vsc_search_pattern(self.ctx._h, self._h, p, b"".join(gs), len(gs), len(p), C.byref(pp),
                                   C.byref(h) if records else None, ptr(out_rows)), self.ctx._h)
        if not records:
            return None, out_rows
        try:
            n = int(L.vsc_pattern_hits_count(h))
            data = C.c_void_p()
            check(L.vsc_pattern_hits_data(h, C.byref(data)), self.ctx._h)
            if n == 0:
                recs = np.zeros(0, dtype=PATTERN_HIT_DTYPE)
            else:
                recs = np.frombuffer((C.c_char * (n * 20)).from_address(data.value), dtype=PATTERN_HIT_DTYPE).copy()
        finally:
            L.vsc_pattern_hits_free(h)
        return recs, out_rows

    def search_pattern_table(self, pattern, guides, max_mismatches, table, top_k=0, min_score=0, max_hits=0, guide_batch=0,
                             records=True, rows=True):
        """vsc_search_pattern_table: search_pattern with every hit scored by a PatternTable of the pattern's length.  Per guide
        the hits with f >= min_score (f = rint(score * 2^30), TABLE_ONE = 1.0) survive, and of those the top_k (0: all) under f
        descending, then record order; the result stays in record order.  Returns (PATTERN_HIT_DTYPE records | None, uint32 f
        per record | None, uint32 rows of shape (n, 9) - hits by NM | None, TABLE_ROW_DTYPE rows | None); both kinds of rows are
        over ALL hits, before the selection.  max_hits caps the returned records; guide_batch never changes the result."""
        p = pattern if isinstance(pattern, bytes) else pattern.encode()
        gs = [g if isinstance(g, bytes) else g.encode() for g in guides]
        for i, g in enumerate(gs):
            if len(g) != len(p):
                raise ValueError("guide %d has %d letters; the pattern has %d" % (i, len(g), len(p)))
        pp = _lib.PatternParams(int(max_mismatches), int(guide_batch), int(max_hits))
        sel = _lib.PatternSelect(int(top_k), int(min_score))
        L = lib()
        h = C.c_void_p()
        out_rows = np.zeros((len(gs), 9), dtype=np.uint32) if rows else None
        out_table = np.zeros(len(gs), dtype=TABLE_ROW_DTYPE) if rows else None
        check(L.vsc_search_pattern_table(self.ctx._h, self._h, p, b"".join(gs), len(gs), len(p), C.byref(pp), table._h, C.byref(sel),
                                         C.byref(h) if records else None, ptr(out_rows), ptr(out_table)), self.ctx._h)
        if not records:
            return None, None, out_rows, out_table
        try:
            n = int(L.vsc_pattern_hits_count(h))
            data, side = C.c_void_p(), C.c_void_p()
            check(L.vsc_pattern_hits_data(h, C.byref(data)), self.ctx._h)
            check(L.vsc_pattern_hits_scores(h, C.byref(side)), self.ctx._h)
            if n == 0:
                recs, fixed = np.zeros(0, dtype=PATTERN_HIT_DTYPE), np.zeros(0, dtype=np.uint32)
            else:
                recs = np.frombuffer((C.c_char * (n * 20)).from_address(data.value), dtype=PATTERN_HIT_DTYPE).copy()
                fixed = np.frombuffer((C.c_char * (n * 4)).from_address(side.value), dtype=np.uint32).copy()
        finally:
            L.vsc_pattern_hits_free(h)
        return recs, fixed, out_rows, out_table

    def search_pattern_hits(self, pattern, guides, max_mismatches, table=None, max_hits=0, guide_batch=0):
        """vsc_search_pattern (table=None) or vsc_search_pattern_table without a selection, the records kept on the device:
        a PatternHits object (to_numpy, scores, variants, shadowed; close it when done)."""
        p = pattern if isinstance(pattern, bytes) else pattern.encode()
        gs = [g if isinstance(g, bytes) else g.encode() for g in guides]
        for i, g in enumerate(gs):
            if len(g) != len(p):
                raise ValueError("guide %d has %d letters; the pattern has %d" % (i, len(g), len(p)))
        pp = _lib.PatternParams(int(max_mismatches), int(guide_batch), int(max_hits))
        h = C.c_void_p()
        if table is None:
            check(lib().vsc_search_pattern(self.ctx._h, self._h, p, b"".join(gs), len(gs), len(p), C.byref(pp), C.byref(h), None), self.ctx._h)
        else:
            sel = _lib.PatternSelect(0, 0)
            check(lib().vsc_search_pattern_table(self.ctx._h, self._h, p, b"".join(gs), len(gs), len(p), C.byref(pp), table._h, C.byref(sel),
                                                 C.byref(h), None, None), self.ctx._h)
        return PatternHits(self, h, len(gs), len(p), table is not None)

    def _bulge_records(self, h):
        """(records,) of a bulge result, which is freed."""
        L = lib()
        try:
            n = int(L.vsc_bulge_hits_count(h))
            data = C.c_void_p()
            check(L.vsc_bulge_hits_data(h, C.byref(data)), self.ctx._h)
            if n == 0:
                return (np.zeros(0, dtype=BULGE_HIT_DTYPE),)
            return (np.frombuffer((C.c_char * (n * 16)).from_address(data.value), dtype=BULGE_HIT_DTYPE).copy(),)
        finally:
            L.vsc_bulge_hits_free(h)

    def search_pattern_bulges(self, pattern, guides, max_mismatches, protospacer, dna=1, rna=1, max_hits=0, guide_batch=0,
                              records=True, rows=True, table=None):
        """vsc_search_pattern_bulges: search_bulges for any nuclease - the sites of len(pattern) + d bases, d in -rna .. -1 and
        1 .. dna, that satisfy the pattern with its protospacer = (start, length) stretched or shortened by d, hold no N and pair
        with a guide within max_mismatches when d bases of the site (DNA bulge) or -d positions of the guide (RNA bulge) inside
        the protospacer stay unpaired.  pattern and guides as search_pattern takes them; the pattern must be N over the
        protospacer (pattern_protospacer gives it for a preset).  Returns (BULGE_HIT_DTYPE records in ascending (guide, strand,
        contig, pos, d) order | None, uint32 rows of shape (n, 4, 9) - hits by class (RNA 2, RNA 1, DNA 1, DNA 2) and NM | None);
        unpack_bulge_info reads the info word, d = site length - len(pattern).  max_hits: 0 = no cap, else VSC_ERR_RANGE when
        there are more records; guide_batch never changes the result.  table: a BulgeTable of the pattern's length - the return
        gains (uint32 f per record | None, TABLE_ROW_DTYPE rows | None), as search_bulges'."""
        p = pattern if isinstance(pattern, bytes) else pattern.encode()
        gs = [g if isinstance(g, bytes) else g.encode() for g in guides]
        for i, g in enumerate(gs):
            if len(g) != len(p):
                raise ValueError("guide %d has %d letters; the pattern has %d" % (i, len(g), len(p)))
        pp = _lib.PatternBulgeParams(int(max_mismatches), int(guide_batch), int(max_hits), int(protospacer[0]), int(protospacer[1]),
                                     int(dna), int(rna))
        L = lib()
        h = C.c_void_p()
        out_rows = np.zeros((len(gs), _lib.BULGE_CLASSES, 9), dtype=np.uint32) if rows else None
        check(L.vsc_search_pattern_bulges(self.ctx._h, self._h, p, b"".join(gs), len(gs), len(p), C.byref(pp),
                                          C.byref(h) if records or table is not None else None, ptr(out_rows)), self.ctx._h)
        if table is not None:
            try:
                fixed, table_rows = self._bulge_scores(h, gs, table, records, rows)
            except Exception:
                L.vsc_bulge_hits_free(h)
                raise
            if not records:
                L.vsc_bulge_hits_free(h)
                return None, out_rows, None, table_rows
            return self._bulge_records(h) + (out_rows, fixed, table_rows)
        if not records:
            return None, out_rows
        return self._bulge_records(h) + (out_rows,)

    def _bulge_scores(self, bulged_h, texts, table, records, rows):
        """vsc_bulge_hits_table over a device result: (uint32 f per record | None, TABLE_ROW_DTYPE rows | None)."""
        L = lib()
        n = int(L.vsc_bulge_hits_count(bulged_h))
        fixed = np.zeros(n, dtype=np.uint32) if records else None
        out_rows = np.zeros(len(texts), dtype=TABLE_ROW_DTYPE) if rows else None
        check(L.vsc_bulge_hits_table(self.ctx._h, self._h, bulged_h, b"".join(texts), len(texts), table.length, table._h, ptr(fixed),
                                     ptr(out_rows)), self.ctx._h)
        return fixed, out_rows

    def _site_scores(self, sites_h, params, texts, table, top_k, min_score, records, rows):
        """vsc_sites_table over a device result: (SITE_DTYPE records | None, SITE_SCORE_DTYPE records | None, TABLE_ROW_DTYPE
        rows | None) - the records are the survivors of the selection, the rows are over all sites."""
        L = lib()
        h = C.c_void_p()
        sel = _lib.PatternSelect(int(top_k), int(min_score))
        out_rows = np.zeros(len(texts), dtype=TABLE_ROW_DTYPE) if rows else None
        check(L.vsc_sites_table(self.ctx._h, self._h, sites_h, C.byref(params), b"".join(texts), len(texts), table.length, table._h,
                                C.byref(sel), C.byref(h) if records else None, ptr(out_rows)), self.ctx._h)
        if not records:
            return None, None, out_rows
        try:
            n = int(L.vsc_sites_count(h))
            data, side = C.c_void_p(), C.c_void_p()
            check(L.vsc_sites_data(h, C.byref(data)), self.ctx._h)
            check(L.vsc_sites_scores(h, C.byref(side)), self.ctx._h)
            if n == 0:
                recs, scores = np.zeros(0, dtype=SITE_DTYPE), np.zeros(0, dtype=SITE_SCORE_DTYPE)
            else:
                recs = np.frombuffer((C.c_char * (n * 32)).from_address(data.value), dtype=SITE_DTYPE).copy()
                scores = np.frombuffer((C.c_char * (n * 16)).from_address(side.value), dtype=SITE_SCORE_DTYPE).copy()
        finally:
            L.vsc_sites_free(h)
        return recs, scores, out_rows

    def _collapse_scored(self, fn, plain_h, bulged_h, texts, params, table, top_k, min_score, records, rows):
        """The collapse with its records kept on the device, then _site_scores: (records | None, SITE_ROW_DTYPE rows | None,
        score records | None, TABLE_ROW_DTYPE rows | None)."""
        L = lib()
        h = C.c_void_p()
        site_rows = np.zeros(len(texts), dtype=SITE_ROW_DTYPE) if rows else None
        check(fn(self.ctx._h, plain_h, bulged_h, len(texts), C.byref(params), C.byref(h), ptr(site_rows)), self.ctx._h)
        try:
            recs, scores, table_rows = self._site_scores(h, params, texts, table, top_k, min_score, records, rows)
        finally:
            L.vsc_sites_free(h)
        return recs, site_rows, scores, table_rows

    def _collapse(self, fn, plain_h, bulged_h, n_guides, params, records, rows):
        """vsc_hits_sites / vsc_pattern_hits_sites over two device results: (SITE_DTYPE records | None, SITE_ROW_DTYPE rows | None)."""
        L = lib()
        h = C.c_void_p()
        out_rows = np.zeros(n_guides, dtype=SITE_ROW_DTYPE) if rows else None
        check(fn(self.ctx._h, plain_h, bulged_h, n_guides, C.byref(params), C.byref(h) if records else None, ptr(out_rows)), self.ctx._h)
        if not records:
            return None, out_rows
        try:
            n = int(L.vsc_sites_count(h))
            data = C.c_void_p()
            check(L.vsc_sites_data(h, C.byref(data)), self.ctx._h)
            if n == 0:
                recs = np.zeros(0, dtype=SITE_DTYPE)
            else:
                recs = np.frombuffer((C.c_char * (n * 32)).from_address(data.value), dtype=SITE_DTYPE).copy()
        finally:
            L.vsc_sites_free(h)
        return recs, out_rows

    def search_sites(self, guides, max_mismatches, dna=1, rna=1, extra_pam=None, algorithm="auto", guide_batch=0, records=True,
                     rows=True, table=None, top_k=0, min_score=0):
        """The cut sites of a search: vsc_search, vsc_search_bulges and vsc_hits_sites with the two intermediate results kept on
        the device (and freed) - the plain hits and the bulged alignments of 23 + d bases collapsed into one SITE_DTYPE record
        per (guide, strand, contig, PAM-side end), with the best alignment's fields (fewest mismatches + bulge bases, then the
        smaller bulge, then DNA before RNA) and the NM of every member (unpack_site_members).  Returns (records in the order of
        their best alignments | None, SITE_ROW_DTYPE rows per guide | None).  collapse_sites is the same on host arrays.
        table: a BulgeTable of 23 letters - every site is scored by vsc_sites_table where the collapse left it; per guide the
        sites with top >= min_score survive, of those the top_k (0: all) under top descending, then record order.  The return
        gains (SITE_SCORE_DTYPE records of the surviving sites | None, TABLE_ROW_DTYPE rows | None); both kinds of rows are over
        ALL sites."""
        codes = guides if isinstance(guides, np.ndarray) else pack_guides(guides)
        codes = np.ascontiguousarray(codes, dtype=np.uint64)
        p = self._params(max_mismatches, extra_pam, algorithm)
        bp = _lib.BulgeParams(int(dna), int(rna), int(guide_batch), 0, 0)
        pb = self._params(max_mismatches, extra_pam, ALGO_SCAN)
        L = lib()
        plain, bulged = C.c_void_p(), C.c_void_p()
        try:
            check(L.vsc_search(self.ctx._h, self._h, ptr(codes), len(codes), C.byref(p), C.byref(plain)), self.ctx._h)
            check(L.vsc_search_bulges(self.ctx._h, self._h, ptr(codes), len(codes), C.byref(pb), C.byref(bp), C.byref(bulged), None), self.ctx._h)
            if table is not None:
                return self._collapse_scored(L.vsc_hits_sites, plain, bulged, [t.encode() for t in unpack_guides(codes)],
                                             _site_params(23, "end"), table, top_k, min_score, records, rows)
            return self._collapse(L.vsc_hits_sites, plain, bulged, len(codes), _site_params(23, "end"), records, rows)
        finally:
            L.vsc_bulge_hits_free(bulged)
            L.vsc_hits_free(plain)

    def search_pattern_sites(self, pattern, guides, max_mismatches, protospacer, dna=1, rna=1, anchor=None, guide_batch=0, records=True,
                             rows=True, table=None, top_k=0, min_score=0):
        """search_sites for any nuclease: vsc_search_pattern, vsc_search_pattern_bulges and vsc_pattern_hits_sites on the device.
        anchor: "end" (the site's 3' end in read orientation is the fixed, PAM-side end: SpCas9, SaCas9), "start" (the 5' end:
        Cas12a) or None - "end" when the protospacer starts at 0, "start" when it ends at the pattern's end, else ValueError.
        table, top_k, min_score: as search_sites takes them, a BulgeTable of the pattern's length."""
        p = pattern if isinstance(pattern, bytes) else pattern.encode()
        gs = [g if isinstance(g, bytes) else g.encode() for g in guides]
        for i, g in enumerate(gs):
            if len(g) != len(p):
                raise ValueError("guide %d has %d letters; the pattern has %d" % (i, len(g), len(p)))
        if anchor is None:
            if int(protospacer[0]) == 0:
                anchor = "end"
            elif int(protospacer[0]) + int(protospacer[1]) == len(p):
                anchor = "start"
            else:
                raise ValueError("the protospacer touches neither end of the pattern: say anchor='end' or 'start'")
        sp = _site_params(len(p), anchor)
        pp = _lib.PatternParams(int(max_mismatches), int(guide_batch), 0)
        pbp = _lib.PatternBulgeParams(int(max_mismatches), int(guide_batch), 0, int(protospacer[0]), int(protospacer[1]), int(dna), int(rna))
        L = lib()
        plain, bulged = C.c_void_p(), C.c_void_p()
        try:
            check(L.vsc_search_pattern(self.ctx._h, self._h, p, b"".join(gs), len(gs), len(p), C.byref(pp), C.byref(plain), None), self.ctx._h)
            check(L.vsc_search_pattern_bulges(self.ctx._h, self._h, p, b"".join(gs), len(gs), len(p), C.byref(pbp), C.byref(bulged), None),
                  self.ctx._h)
            if table is not None:
                return self._collapse_scored(L.vsc_pattern_hits_sites, plain, bulged, gs, sp, table, top_k, min_score, records, rows)
            return self._collapse(L.vsc_pattern_hits_sites, plain, bulged, len(gs), sp, records, rows)
        finally:
            L.vsc_bulge_hits_free(bulged)
            L.vsc_pattern_hits_free(plain)

    def enumerate_pattern(self, pattern, protospacer, targets=None, rule="overlap", strands="both", gc=(0, 0), max_t_run=0,
                          max_guides=0, params=None, efficiency=None, min_efficiency=None, microhomology=None,
                          min_out_of_frame=None, min_microhomology=None, edit=None, edit_targets=None, min_editable=None,
                          max_editable=None, cds=None, edit_to=None, require_effect=None, forbid_effect=None, prime=None,
                          prime_edits=None, prime_allow_weak=None, variation=None, variants=None, max_variant_cost=None,
                          max_variants_by_zone=None, require_variant_zones=None, hdr=None, hdr_edits=None, hdr_cds=None,
                          hdr_allow_open=None, fold=None, fold_scaffold=None, max_fold_starts=None, max_fold_self=None,
                          max_fold_scaffold=None, max_fold_seed=None, motifs=None, motif_set=None, motif_left=None, motif_right=None,
                          forbid_motifs=None, forbid_context_motifs=None, require_cut_motifs=None, cut_only=None, knockout=None, knockout_cds=None,
                          min_cut_frac=None, max_cut_frac=None, min_cut_edge=None, require_knockout=None, forbid_knockout=None):
        """vsc_guides_enumerate_pattern: the candidate guides of this genome (or shard) under an IUPAC pattern of 16..32
        letters - every N-free site that satisfies it, on either strand.  protospacer = (start, length) in read positions
        (pattern_protospacer gives it for a preset): gc[0] <= its G/C <= gc[1] (gc[1] = 0: no upper bound) and no run of more
        than max_t_run T in it (0: no limit).  targets: None (everywhere) or (contig, start, end) triples / an INTERVAL_DTYPE
        array, applied to the whole site under `rule` ("overlap" / "inside"); an empty list keeps nothing.  Returns a
        PatternGuides (.codes, .loci, .text()) in ascending (contig, pos), '+' before '-'.  More than max_guides (0: no cap)
        candidates raise VarscotError -34.  params: a PatternEnumParams to pass as it is (tests).
        efficiency= an EfficiencyModel or a TreeEfficiencyModel whose site_len is the pattern's length: returns (PatternGuides, linear float64[n]) - the
        candidates' predictors, computed where the candidates lie on the device (vsc_pattern_guides_efficiency).
        min_efficiency=x (needs efficiency=): only the candidates whose predictor is defined and >= x, linear domain
        (vsc_pattern_guides_filter_efficiency).
        microhomology= a MicrohomologyShape whose site_len is the pattern's length: the candidates' (sum, oof) pairs
        (uint32[n, 2], vsc_pattern_guides_microhomology) come last, after the predictors when both are asked for.
        min_out_of_frame=x (per cent) / min_microhomology=y (score units; both need microhomology=): only the candidates
        whose score is defined, at least y, and out of frame for at least x per cent of it
        (vsc_pattern_guides_filter_microhomology).  Both floors are applied on the device, in either order the same bytes.
        edit= an EditShape whose site_len is the pattern's length: the candidates' (mask, hits) rows (uint32[n, 2],
        vsc_pattern_guides_edit) come last of all.  edit_targets= (contig, pos) rows / min_editable= / max_editable= (all need
        edit=): only the candidates whose site is defined, whose window holds min_editable .. max_editable editable bases and
        - with targets - reaches a target (vsc_pattern_guides_filter_edit), on the device after the other floors.
        cds= a Cds (needs edit=): the candidates' effect rows (uint32[n, 2], vsc_pattern_guides_effects) come last of all, after
        the edit rows.  edit_to= the base the editor writes (default: the transition partner of the shape's base) /
        require_effect= / forbid_effect= class names of EFFECT_CLASSES (all need cds=): only the candidates with an effect of
        a required class and none of a forbidden one (vsc_pattern_guides_filter_effects), after the edit filter.
        prime= a PrimeShape whose site_len is the pattern's length: the candidates' (pbs, n_pairs) rows (uint32[n, 2],
        vsc_pattern_guides_prime) come last of all.  prime_edits= (contig, pos, del_len, ins) rows / prime_allow_weak= (both need
        prime=): only the candidates whose context is defined, that - with edits - can write one of them, and - with
        prime_allow_weak=False - whose PBS is not WEAK (vsc_pattern_guides_filter_prime), after the edit and effects filters.
        variation= a VariationShape whose site_len is the pattern's length (or the name of a preset of VARIATION_SHAPES) with
        variants= (as Genome.variation takes them): the candidates' variation rows (uint32[n, 4], vsc_pattern_guides_variation)
        come last of all.  max_variant_cost= / max_variants_by_zone= four bounds (255: none) / require_variant_zones= zone
        numbers or names of VARIATION_ZONES (all need variation=): only the candidates that pass the variation filter
        (vsc_pattern_guides_filter_variation), after the other filters.
        hdr= an HdrShape whose site_len is the pattern's length (or the name of a preset of HDR_NUCLEASES): the candidates'
        (n_pairs, n_usable) rows (uint32[n, 2], vsc_pattern_guides_hdr) come last of all.  hdr_edits= (contig, pos, del_len, ins)
        rows / hdr_cds= a Cds / hdr_allow_open= (all need hdr=): with edits or hdr_allow_open only the candidates whose context
        is defined and that - with edits - have a usable pair, or with hdr_allow_open=True any pair
        (vsc_pattern_guides_filter_hdr), after the other families' filters.
        fold= a FoldShape whose site_len is the pattern's length (or the name of a preset of FOLD_SHAPES): the candidates' fold
        rows (uint32[n, 2], vsc_pattern_guides_fold; unpack_fold_row names the fields) come last of all, after the HDR rows.
        fold_scaffold= the constant part of the guide RNA (at most 128 letters of A C G T U; default: none) / max_fold_starts= /
        max_fold_self= / max_fold_scaffold= / max_fold_seed= whole numbers 0 .. 32 (all need fold=): with a limit only the
        candidates whose row is defined and within every limit (vsc_pattern_guides_filter_fold), after the HDR filter.
        motifs= a MotifShape whose site_len is the pattern's length (or the name of a preset of MOTIF_SHAPES) with motif_set= a
        MotifSet (motifs(...)) or its entries: the candidates' motif rows (uint64[n, 3]: construct, cut, elsewhere;
        vsc_pattern_guides_motifs; unpack_motif_row names the bits) come last of all, after the fold rows.  motif_left= /
        motif_right= the vector's text on either side of the cloned spacer (at most 16 letters of A C G T U; default: none) /
        forbid_motifs= / forbid_context_motifs= / require_cut_motifs= names or bit masks / cut_only= (all need motifs=): with one of
        them only the candidates whose row is defined and passes FILTER (vsc_pattern_guides_filter_motifs), after the fold
        filter.
        knockout= a KnockoutShape whose site_len is the pattern's length (or the name of a preset of KNOCKOUT_SHAPES) with
        knockout_cds= a Cds: the candidates' knock-out rows (uint32[n, 4], vsc_pattern_guides_knockout; unpack_knockout_row names
        the fields) come last of all, after the motif rows.  min_cut_frac= / max_cut_frac= shares of the protein, floats in 0 .. 1
        (knockout_cut_frac states how they become 0 .. 65535) / min_cut_edge= 0 .. 255 bases to the nearer end of the exon /
        require_knockout= / forbid_knockout= flag names of KNOCKOUT_FLAGS or masks (all need knockout=): with one of them only
        the candidates whose cut is a coding cut and passes FILTER (vsc_pattern_guides_filter_knockout), after the motif
        filter."""
        p = pattern if isinstance(pattern, bytes) else pattern.encode()
        ep = params if params is not None else _pattern_enum_params(protospacer, rule, strands, gc, max_t_run, max_guides)
        iv = None if targets is None else _intervals(targets)
        # (an empty target set is a pointer that is not NULL with n = 0)
        iv_ptr = None if iv is None else ptr(iv if len(iv) else np.zeros(1, dtype=_lib.INTERVAL_DTYPE))
        L = lib()
        self._eff_args(efficiency, min_efficiency, len(p))
        mh = self._mh_args(microhomology, min_out_of_frame, min_microhomology, len(p))
        ed = self._edit_args(edit, edit_targets, min_editable, max_editable, len(p))
        fx = self._effects_args(ed, edit, cds, edit_to, require_effect, forbid_effect)
        pe = self._prime_args(prime, prime_edits, prime_allow_weak, len(p))
        vr = self._variation_args(variation, variants, max_variant_cost, max_variants_by_zone, require_variant_zones, len(p))
        hd = self._hdr_args(hdr, hdr_edits, hdr_cds, hdr_allow_open, len(p))
        fo = self._fold_args(fold, fold_scaffold, max_fold_starts, max_fold_self, max_fold_scaffold, max_fold_seed, len(p))
        mo = self._motif_args(motifs, motif_set, motif_left, motif_right, forbid_motifs, forbid_context_motifs, require_cut_motifs, cut_only, len(p))
        ko = self._knockout_args(knockout, knockout_cds, min_cut_frac, max_cut_frac, min_cut_edge, require_knockout, forbid_knockout, len(p))
        h = C.c_void_p()
        check(L.vsc_guides_enumerate_pattern(self.ctx._h, self._h, p, len(p), C.byref(ep), iv_ptr, 0 if iv is None else len(iv),
                                             C.byref(h)), self.ctx._h)
        held = [h]
        try:
            extra = self._scores_on_handle(held, efficiency, min_efficiency, mh, L.vsc_pattern_guides_count,
                                           (L.vsc_pattern_guides_efficiency, L.vsc_pattern_guides_filter_efficiency),
                                           (L.vsc_pattern_guides_microhomology, L.vsc_pattern_guides_filter_microhomology),
                                           L.vsc_pattern_guides_free, ed,
                                           (L.vsc_pattern_guides_edit, L.vsc_pattern_guides_filter_edit), fx,
                                           (L.vsc_pattern_guides_effects, L.vsc_pattern_guides_filter_effects), pe,
                                           (L.vsc_pattern_guides_prime, L.vsc_pattern_guides_filter_prime), vr,
                                           (L.vsc_pattern_guides_variation, L.vsc_pattern_guides_filter_variation), hd,
                                           (L.vsc_pattern_guides_hdr, L.vsc_pattern_guides_filter_hdr), fo,
                                           (L.vsc_pattern_guides_fold, L.vsc_pattern_guides_filter_fold), mo,
                                           (L.vsc_pattern_guides_motifs, L.vsc_pattern_guides_filter_motifs), ko,
                                           (L.vsc_pattern_guides_knockout, L.vsc_pattern_guides_filter_knockout))
            h = held[0]
            n = int(L.vsc_pattern_guides_count(h))
            pc, pl = C.c_void_p(), C.c_void_p()
            check(L.vsc_pattern_guides_data(h, C.byref(pc), C.byref(pl)), self.ctx._h)
            if n == 0:
                codes, loci = np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=_lib.LOCUS_DTYPE)
            else:
                codes = np.frombuffer((C.c_char * (n * 8)).from_address(pc.value), dtype=np.uint64).copy()
                loci = np.frombuffer((C.c_char * (n * 16)).from_address(pl.value), dtype=_lib.LOCUS_DTYPE).copy()
        finally:
            L.vsc_pattern_guides_free(held[0])
        found = PatternGuides(p.decode(), protospacer, codes, loci)
        return (found,) + extra if extra else found

    def design_pattern(self, pattern, protospacer, max_mismatches, targets=None, guide_batch=0, table=None, pick=None, pick_by=None,
                       pick_groups=None, **filters):
        """Every guide of `targets` under a pattern, with its off-target counts: enumerate_pattern(pattern, protospacer,
        targets, **filters) followed by search_pattern (rows only) of the guides in query form on the same resident genome.
        Returns (PatternGuides, uint32 rows of shape (n, 9)); count[0] is reduced by one for the guide's own locus, which is
        always a hit at NM 0 (the query form has N outside the protospacer).  With efficiency= (and min_efficiency=) among
        the filters, as enumerate_pattern takes them: only the survivors are searched, and their predictors come last; the
        same holds for microhomology= (and its floors), whose pairs come after the predictors.
        table= a PatternTable: search_pattern_table instead, and the TABLE_ROW_DTYPE rows follow the NM rows - each with the
        guide's own locus taken out as well, by the host's score of the guide (query form) against its own site (the
        candidate's letters, PAM included), as count[0] is reduced.
        pick= a PickShape whose site_len is the pattern's length (with pick_by= / pick_groups=): as Genome.design takes them,
        over `targets` as a Regions under the enumeration's rule; the columns are "table" (the default; needs table=), "eff",
        "oof" and "mh".  (picks, counts) come last of all.  edit= (and its options), as enumerate_pattern takes them: only the
        survivors are searched; the edit rows come after the microhomology pairs, before (picks, counts).  cds= / edit_to= /
        require_effect= / forbid_effect=: as enumerate_pattern; the effect rows come after the edit rows.  prime= /
        prime_edits= / prime_allow_weak=: as enumerate_pattern; the prime rows come after the effect rows.  variation= /
        variants= / max_variant_cost= / max_variants_by_zone= / require_variant_zones=: as enumerate_pattern; only the survivors
        are searched, and the variation rows come after the prime rows.  fold= (and its options): as enumerate_pattern; only the
        survivors are searched, the fold rows come last of the rows but the motif rows, and pick_by= knows the column "fold".
        motifs= (and its options): as enumerate_pattern; only the survivors are searched, the motif rows come last of the rows but
        the knock-out rows, and pick_by= knows the column "rflp".  knockout= (and its options): as enumerate_pattern; only the
        survivors are searched, the knock-out rows come last of the rows, and pick_by= knows the column "knockout"."""
        if pick is None and (pick_by is not None or pick_groups is not None):
            raise ValueError("pick_by= / pick_groups= need pick=")
        found = self.enumerate_pattern(pattern, protospacer, targets, **filters)
        extra = ()
        if isinstance(found, tuple):
            found, extra = found[0], tuple(found[1:])
        if table is not None:
            queries = found.text()
            _, _, rows, trows = self.search_pattern_table(pattern, queries, max_mismatches, table, guide_batch=guide_batch, records=False)
            rows[:, 0] -= np.minimum(rows[:, 0], 1).astype(np.uint32)
            for i, (q, own) in enumerate(zip(queries, found.text(spell_pam=True))):
                f = table.score(q, own, fixed=True)[1]
                trows["score_sum"][i] -= f
                if f:
                    trows["positive"][i] -= 1
                    trows["positive_nm"][i, 0] -= 1
            out = (found, rows, trows) + extra
        else:
            _, rows = self.search_pattern(pattern, found.text(), max_mismatches, guide_batch=guide_batch, records=False)
            rows[:, 0] -= np.minimum(rows[:, 0], 1).astype(np.uint32)
            out = (found, rows) + extra
        if pick is None:
            return out
        return self._design_pattern_pick(out, found, extra, targets, table, pick, pick_by, pick_groups, filters)

    def _design_pattern_pick(self, out, found, extra, targets, table, pick, pick_by, pick_groups, filters):
        if targets is None or self.packed is None:
            raise ValueError("pick= needs targets and a genome made from a PackedGenome")
        if isinstance(pick, PickShape) and pick.site_len != len(found.pattern):
            raise ValueError("pick.site_len is %d, the pattern has %d letters" % (pick.site_len, len(found.pattern)))
        rest = list(extra)
        linear = rest.pop(0) if filters.get("efficiency") is not None else None
        pairs = rest.pop(0) if filters.get("microhomology") is not None else None
        kos = rest.pop() if filters.get("knockout") is not None else None
        sites = rest.pop() if filters.get("motifs") is not None else None
        folds = rest[-1] if filters.get("fold") is not None else None
        spec = None
        if table is not None:
            spec = np.array([table_specificity(x) for x in out[2]["score_sum"]], dtype=np.float64)
        regions = Regions(self.packed, targets, rule=filters.get("rule", "overlap"))
        try:
            return tuple(out) + self._pick_found(pick, pick_by, pick_groups, regions, found,
                                                 {"table": spec, "eff": linear, "oof": pairs, "mh": pairs, "fold": folds, "rflp": sites,
                                                  "knockout": kos})
        finally:
            regions.close()

    # ---- on-target efficiency (vsc_*_efficiency) ------------------------------------------------------------------------
    @staticmethod
    def _eff_args(model, floor, site_len):
        if model is None:
            if floor is not None:
                raise ValueError("min_efficiency needs efficiency=model")
            return
        if not isinstance(model, (EfficiencyModel, TreeEfficiencyModel)):
            raise ValueError("efficiency must be an EfficiencyModel or a TreeEfficiencyModel")
        if model.site_len != site_len:
            raise ValueError("the model's site_len is %d; these candidates are %d bases long" % (model.site_len, site_len))

    def _eff_on_handle(self, held, model, floor, count_fn, score_fn, filter_fn, free_fn, score=True):
        """The predictors of the candidate handle held[0] under a model, computed where the candidates lie.  With a floor the
        handle is first replaced by the filter's result: the input is freed and held[0] is the result - the caller frees
        held[0], whatever happens here.  score=False: the filter only.  A TreeEfficiencyModel goes through the calls of the
        same names that end in _trees."""
        if isinstance(model, TreeEfficiencyModel):
            score_fn, filter_fn = (getattr(lib(), fn.__name__ + "_trees") for fn in (score_fn, filter_fn))
        if floor is not None:
            out = C.c_void_p()
            check(filter_fn(self.ctx._h, self._h, held[0], model._h, float(floor), C.byref(out)), self.ctx._h)
            free_fn(held[0])
            held[0] = out
        if not score:
            return None
        linear = np.empty(int(count_fn(held[0])), dtype=np.float64)
        st = _lib.EffStats()
        check(score_fn(self.ctx._h, self._h, held[0], model._h, ptr(linear), C.byref(st)), self.ctx._h)
        _eff_partial(st.as_dict(), False)
        return linear

    # ---- microhomology and out-of-frame scores (vsc_*_microhomology) ----------------------------------------------------
    @staticmethod
    def _mh_args(shape, min_oof, min_sum, site_len):
        """(shape, min_sum in tenths, min_oof in per mille) - the floors None when neither is given - or None without a
        shape.  min_out_of_frame is in per cent and becomes per mille here, once: round(10 * x); min_microhomology is in the
        published score's units and becomes tenths: ceil(10 * x)."""
        if shape is None:
            if min_oof is not None or min_sum is not None:
                raise ValueError("min_out_of_frame / min_microhomology need microhomology=shape")
            return None
        if not isinstance(shape, MicrohomologyShape):
            raise ValueError("microhomology must be a MicrohomologyShape")
        if shape.site_len != site_len:
            raise ValueError("the shape's site_len is %d; these candidates are %d bases long" % (shape.site_len, site_len))
        if min_oof is None and min_sum is None:
            return shape, None, None
        permille = 0 if min_oof is None else int(round(10.0 * float(min_oof)))
        tenths = 0 if min_sum is None else int(np.ceil(10.0 * float(min_sum) - 1e-9))
        if not 0 <= permille <= 1000:
            raise ValueError("min_out_of_frame is a share in per cent, 0 .. 100")
        if not 0 <= tenths <= 0xFFFFFFFF:
            raise ValueError("min_microhomology is out of range")
        return shape, tenths, permille

    def _mh_on_handle(self, held, mh, count_fn, score_fn, filter_fn, free_fn, score=True):
        """As _eff_on_handle, for the microhomology pairs: mh = what _mh_args returned."""
        shape, tenths, permille = mh
        sh = shape._struct()
        if tenths is not None:
            out = C.c_void_p()
            check(filter_fn(self.ctx._h, self._h, held[0], C.byref(sh), tenths, permille, C.byref(out)), self.ctx._h)
            free_fn(held[0])
            held[0] = out
        if not score:
            return None
        pairs = np.empty((int(count_fn(held[0])), 2), dtype=np.uint32)
        st = _lib.MhStats()
        check(score_fn(self.ctx._h, self._h, held[0], C.byref(sh), ptr(pairs), C.byref(st)), self.ctx._h)
        _eff_partial(st.as_dict(), False)
        return pairs

    def _scores_on_handle(self, held, efficiency, min_efficiency, mh, count_fn, eff_fns, mh_fns, free_fn, ed=None, ed_fns=None,
                          fx=None, fx_fns=None, pe=None, pe_fns=None, va=None, va_fns=None, hd=None, hd_fns=None, fo=None,
                          fo_fns=None, mo=None, mo_fns=None, ko=None, ko_fns=None):
        """The floors, then the scores over the survivors: the extras of an enumeration, the efficiency predictors before
        the microhomology pairs before the edit rows before the effect rows before the prime rows before the variation rows before the HDR rows
        before the fold rows before the motif rows before the knock-out rows.
        held[0] is replaced as _eff_on_handle replaces it."""
        if efficiency is not None:
            self._eff_on_handle(held, efficiency, min_efficiency, count_fn, eff_fns[0], eff_fns[1], free_fn, score=False)
        if mh is not None:
            self._mh_on_handle(held, mh, count_fn, mh_fns[0], mh_fns[1], free_fn, score=False)
        if ed is not None:
            self._edit_on_handle(held, ed, count_fn, ed_fns[0], ed_fns[1], free_fn, rows=False)
        if fx is not None:
            self._effects_on_handle(held, ed[0], fx, count_fn, fx_fns[0], fx_fns[1], free_fn, rows=False)
        if pe is not None:
            self._prime_on_handle(held, pe, count_fn, pe_fns[0], pe_fns[1], free_fn, rows=False)
        if va is not None:
            self._variation_on_handle(held, va, count_fn, va_fns[0], va_fns[1], free_fn, rows=False)
        if hd is not None:
            self._hdr_on_handle(held, hd, count_fn, hd_fns[0], hd_fns[1], free_fn, rows=False)
        if fo is not None:
            self._fold_on_handle(held, fo, count_fn, fo_fns[0], fo_fns[1], free_fn, rows=False)
        if mo is not None:
            self._motif_on_handle(held, mo, count_fn, mo_fns[0], mo_fns[1], free_fn, rows=False)
        if ko is not None:
            self._knockout_on_handle(held, ko, count_fn, ko_fns[0], ko_fns[1], free_fn, rows=False)
        extra = ()
        if efficiency is not None:
            extra += (self._eff_on_handle(held, efficiency, None, count_fn, eff_fns[0], eff_fns[1], free_fn),)
        if mh is not None:
            extra += (self._mh_on_handle(held, (mh[0], None, None), count_fn, mh_fns[0], mh_fns[1], free_fn),)
        if ed is not None:
            extra += (self._edit_on_handle(held, ed[:4] + (None,), count_fn, ed_fns[0], ed_fns[1], free_fn),)
        if fx is not None:
            extra += (self._effects_on_handle(held, ed[0], fx[:2] + (0, 0) + fx[4:], count_fn, fx_fns[0], fx_fns[1], free_fn),)
        if pe is not None:
            extra += (self._prime_on_handle(held, pe, count_fn, pe_fns[0], pe_fns[1], free_fn, filt=False),)
        if va is not None:
            extra += (self._variation_on_handle(held, va, count_fn, va_fns[0], va_fns[1], free_fn, filt=False),)
        if hd is not None:
            extra += (self._hdr_on_handle(held, hd, count_fn, hd_fns[0], hd_fns[1], free_fn, filt=False),)
        if fo is not None:
            extra += (self._fold_on_handle(held, fo, count_fn, fo_fns[0], fo_fns[1], free_fn, filt=False),)
        if mo is not None:
            extra += (self._motif_on_handle(held, mo, count_fn, mo_fns[0], mo_fns[1], free_fn, filt=False),)
        if ko is not None:
            extra += (self._knockout_on_handle(held, ko, count_fn, ko_fns[0], ko_fns[1], free_fn, filt=False),)
        return extra

    # ---- guide RNA self-complementarity (vsc_*_fold) -------------------------------------------------------------------
    @staticmethod
    def _fold_args(shape, scaffold, max_starts, max_self, max_scaffold, max_seed, site_len):
        """(shape, scaffold bytes, the four limits as integers or None when none is given) - or None without a shape.  The
        limits become integers here, once."""
        given = [v is not None for v in (max_starts, max_self, max_scaffold, max_seed)]
        if shape is None:
            if scaffold is not None or any(given):
                raise ValueError("fold_scaffold / max_fold_starts / max_fold_self / max_fold_scaffold / max_fold_seed need fold=shape")
            return None
        shape = _fold_shape(shape, "fold")
        if shape.site_len != site_len:
            raise ValueError("the shape's site_len is %d; these candidates are %d bases long" % (shape.site_len, site_len))
        limits = _fold_limits(max_starts, max_self, max_scaffold, max_seed) if any(given) else None
        return shape, _fold_scaffold(scaffold), limits

    def _fold_on_handle(self, held, fo, count_fn, rows_fn, filter_fn, free_fn, rows=True, filt=True):
        """As _mh_on_handle, for the fold rows: fo = what _fold_args returned.  With limits the handle is first replaced by
        the filter's result."""
        shape, scaffold, limits = fo
        sh = shape._struct()
        if filt and limits is not None:
            lim = _lib.FoldLimits(*limits)
            out = C.c_void_p()
            check(filter_fn(self.ctx._h, self._h, held[0], C.byref(sh), scaffold, len(scaffold), C.byref(lim), C.byref(out)), self.ctx._h)
            free_fn(held[0])
            held[0] = out
        if not rows:
            return None
        out_rows = np.empty((int(count_fn(held[0])), 2), dtype=np.uint32)
        st = _lib.FoldStats()
        check(rows_fn(self.ctx._h, self._h, held[0], C.byref(sh), scaffold, len(scaffold), ptr(out_rows), C.byref(st)), self.ctx._h)
        _eff_partial(st.as_dict(), False)
        return out_rows

    def fold(self, loci_or_found, shape, scaffold=None, allow_partial=False):
        """vsc_loci_fold: the fold rows of candidates under a FoldShape (or the name of a preset of FOLD_SHAPES) and a scaffold
        text (None: empty), computed on the device from the resident planes: (uint32[n, 2], stats) - unpack_fold_row names the
        fields of a row.  loci_or_found: as Genome.efficiency takes it.  An undefined row is (FOLD_UNDEFINED, FOLD_UNDEFINED);
        stats counts the candidates by class - defined, invalid, off_contig, not_resident, has_n - and holds kernel_ms and
        wall_ms.  Raises when a site is not resident on this object (a shard) unless allow_partial=True."""
        shape = _fold_shape(shape)
        sc = _fold_scaffold(scaffold)
        if isinstance(loci_or_found, PatternGuides):
            loci = loci_or_found.loci
        elif isinstance(loci_or_found, tuple) and len(loci_or_found) >= 2 and isinstance(loci_or_found[1], np.ndarray) \
                and loci_or_found[1].dtype == _lib.LOCUS_DTYPE:
            loci = loci_or_found[1]
        else:
            loci = loci_or_found
        lo = _loci(loci, len(loci))
        rows = np.empty((len(lo), 2), dtype=np.uint32)
        st = _lib.FoldStats()
        sh = shape._struct()
        check(lib().vsc_loci_fold(self.ctx._h, self._h, ptr(lo), len(lo), C.byref(sh), sc, len(sc), ptr(rows), C.byref(st)), self.ctx._h)
        stats = st.as_dict()
        _eff_partial(stats, allow_partial)
        return rows, stats

    # ---- restriction sites and IUPAC motifs (vsc_*_motifs) -------------------------------------------------------------
    @staticmethod
    def _motif_args(shape, motif_set, left, right, forbid, forbid_context, require_cut, cut_only, site_len):
        """(shape, MotifSet, left bytes, right bytes, the limits as (forbid_construct, forbid_context, require_cut, flags) or None
        when none is given) - or None without a shape.  The names become masks here, once."""
        given = [v is not None for v in (forbid, forbid_context, require_cut)]
        if shape is None:
            if motif_set is not None or left is not None or right is not None or any(given) or cut_only is not None:
                raise ValueError("motif_set / motif_left / motif_right / forbid_motifs / forbid_context_motifs / require_cut_motifs / "
                                 "cut_only need motifs=shape")
            return None
        shape = _motif_shape(shape, "motifs")
        if shape.site_len != site_len:
            raise ValueError("the shape's site_len is %d; these candidates are %d bases long" % (shape.site_len, site_len))
        ms = _motif_set(motif_set)
        if cut_only and require_cut is None:
            raise ValueError("cut_only= belongs to require_cut_motifs=")
        limits = None
        if any(given):
            limits = (ms.mask(forbid, "forbid_motifs"), ms.mask(forbid_context, "forbid_context_motifs"),
                      ms.mask(require_cut, "require_cut_motifs"), MOTIF_CUT_ONLY if cut_only else 0)
        return shape, ms, _motif_flank(left, "motif_left"), _motif_flank(right, "motif_right"), limits

    def _motif_on_handle(self, held, mo, count_fn, rows_fn, filter_fn, free_fn, rows=True, filt=True):
        """As _fold_on_handle, for the motif rows: mo = what _motif_args returned.  With limits the handle is first replaced by
        the filter's result."""
        shape, ms, lf, rf, limits = mo
        sh = shape._struct()
        arr = ms._array()
        if filt and limits is not None:
            lim = _lib.MotifLimits(*limits)
            out = C.c_void_p()
            check(filter_fn(self.ctx._h, self._h, held[0], C.byref(sh), lf, len(lf), rf, len(rf), arr, len(ms), C.byref(lim), C.byref(out)),
                  self.ctx._h)
            free_fn(held[0])
            held[0] = out
        if not rows:
            return None
        out_rows = np.empty((int(count_fn(held[0])), 3), dtype=np.uint64)
        st = _lib.MotifStats()
        check(rows_fn(self.ctx._h, self._h, held[0], C.byref(sh), lf, len(lf), rf, len(rf), arr, len(ms), ptr(out_rows), None, C.byref(st)),
              self.ctx._h)
        _eff_partial(st.as_dict(), False)
        return out_rows

    def motifs(self, loci_or_found, shape, motif_set, left=None, right=None, totals=False, allow_partial=False):
        """vsc_loci_motifs: the motif rows of candidates under a MotifShape (or the name of a preset of MOTIF_SHAPES), a MotifSet
        (or its entries) and the flanks (None: empty), computed on the device from the resident planes: (uint64[n, 3], stats) -
        columns construct, cut, elsewhere; unpack_motif_row names the bits.  totals=True: (rows, totals uint64[M, 3], stats) with
        per motif the defined candidates that hold its construct, cut and cut-only bit.  loci_or_found: as Genome.efficiency
        takes it.  An undefined row is (MOTIF_UNDEFINED,) * 3; stats counts the candidates by class - defined, invalid,
        off_contig, not_resident, has_n -, those with any construct, any cut and any cut-only bit, and holds kernel_ms and
        wall_ms.  Raises when a context is not resident on this object (a shard) unless allow_partial=True."""
        shape = _motif_shape(shape)
        ms = _motif_set(motif_set)
        lf, rf = _motif_flank(left, "left"), _motif_flank(right, "right")
        if isinstance(loci_or_found, PatternGuides):
            loci = loci_or_found.loci
        elif isinstance(loci_or_found, tuple) and len(loci_or_found) >= 2 and isinstance(loci_or_found[1], np.ndarray) \
                and loci_or_found[1].dtype == _lib.LOCUS_DTYPE:
            loci = loci_or_found[1]
        else:
            loci = loci_or_found
        lo = _loci(loci, len(loci))
        rows = np.empty((len(lo), 3), dtype=np.uint64)
        tot = np.zeros((len(ms), 3), dtype=np.uint64) if totals else None
        st = _lib.MotifStats()
        sh = shape._struct()
        check(lib().vsc_loci_motifs(self.ctx._h, self._h, ptr(lo), len(lo), C.byref(sh), lf, len(lf), rf, len(rf), ms._array(), len(ms),
                                    ptr(rows), ptr(tot) if totals else None, C.byref(st)), self.ctx._h)
        stats = st.as_dict()
        _eff_partial(stats, allow_partial)
        return (rows, tot, stats) if totals else (rows, stats)

    def microhomology(self, loci_or_found, shape, allow_partial=False):
        """vsc_loci_microhomology: the microhomology pairs of candidates under a MicrohomologyShape, computed on the device from
        the resident planes: (uint32[n, 2], stats) - column 0 is sum (the score of Bae et al. 2014 in tenths), column 1 oof
        (the part of it whose deletion length is no multiple of three); microhomology_scores turns them into mhScore and
        oofScore.  loci_or_found: as Genome.efficiency takes it.  An undefined pair is (MH_UNDEFINED, MH_UNDEFINED); stats
        counts the candidates by class - defined, invalid, off_contig, not_resident, has_n - and holds kernel_ms and wall_ms.
        Raises when a context is not resident on this object (a shard) unless allow_partial=True."""
        if isinstance(loci_or_found, PatternGuides):
            loci = loci_or_found.loci
        elif isinstance(loci_or_found, tuple) and len(loci_or_found) >= 2 and isinstance(loci_or_found[1], np.ndarray) \
                and loci_or_found[1].dtype == _lib.LOCUS_DTYPE:
            loci = loci_or_found[1]
        else:
            loci = loci_or_found
        lo = _loci(loci, len(loci))
        pairs = np.empty((len(lo), 2), dtype=np.uint32)
        st = _lib.MhStats()
        sh = shape._struct()
        check(lib().vsc_loci_microhomology(self.ctx._h, self._h, ptr(lo), len(lo), C.byref(sh), ptr(pairs), C.byref(st)), self.ctx._h)
        stats = st.as_dict()
        _eff_partial(stats, allow_partial)
        return pairs, stats

    # ---- base-editor windows (vsc_*_edit) --------------------------------------------------------------------------------
    @staticmethod
    def _edit_args(shape, targets, min_editable, max_editable, site_len):
        """(shape, sorted targets or None, order, inverse, (min, max) or None) - or None without a shape."""
        if shape is None:
            if targets is not None or min_editable is not None or max_editable is not None:
                raise ValueError("edit_targets / min_editable / max_editable need edit=shape")
            return None
        if isinstance(shape, str):
            if shape not in EDITORS:
                raise ValueError("edit names one of %s, or is an EditShape" % ", ".join(sorted(EDITORS)))
            shape = EDITORS[shape]
        if not isinstance(shape, EditShape):
            raise ValueError("edit must be an EditShape or the name of a preset")
        if shape.site_len != site_len:
            raise ValueError("the shape's site_len is %d; these candidates are %d bases long" % (shape.site_len, site_len))
        tg = order = inverse = None
        if targets is not None:
            tg, order, inverse = edit_targets(targets)
        bounds = None
        if min_editable is not None or max_editable is not None or tg is not None:
            bounds = (0 if min_editable is None else int(min_editable), 16 if max_editable is None else int(max_editable))
            if not 0 <= bounds[0] <= bounds[1] <= 0xFFFFFFFF:
                raise ValueError("0 <= min_editable <= max_editable is needed")
        return shape, tg, order, inverse, bounds

    def _edit_on_handle(self, held, ed, count_fn, rows_fn, filter_fn, free_fn, rows=True):
        """As _mh_on_handle, for the edit rows: ed = what _edit_args returned.  With bounds (or targets) the handle is first
        replaced by the filter's result; the rows of the survivors come back as uint32[n, 2]."""
        shape, tg, _, _, bounds = ed
        sh = shape._struct()
        n_t = 0 if tg is None else len(tg)
        tp = ptr(tg) if n_t else None
        if bounds is not None:
            out = C.c_void_p()
            check(filter_fn(self.ctx._h, self._h, held[0], C.byref(sh), tp, n_t, bounds[0], bounds[1], C.byref(out)), self.ctx._h)
            free_fn(held[0])
            held[0] = out
        if not rows:
            return None
        r = np.empty((int(count_fn(held[0])), 2), dtype=np.uint32)
        st = _lib.EditStats()
        check(rows_fn(self.ctx._h, self._h, held[0], C.byref(sh), tp, n_t, ptr(r), None, 0, None, None, C.byref(st)), self.ctx._h)
        _eff_partial(st.as_dict(), False)
        return r

    # ---- coding consequences of base edits (vsc_*_effects) -----------------------------------------------------------------
    @staticmethod
    def _effects_args(ed, edit, cds, edit_to, require_effect, forbid_effect):
        """(cds, to, require mask, forbid mask, code) - or None without a Cds.  ed: what _edit_args returned."""
        if cds is None:
            if edit_to is not None or require_effect is not None or forbid_effect is not None:
                raise ValueError("edit_to / require_effect / forbid_effect need cds=")
            return None
        if ed is None:
            raise ValueError("cds= needs edit=shape")
        if not isinstance(cds, Cds):
            raise ValueError("cds must be a Cds")
        if edit_to is None and isinstance(edit, str):
            edit_to = EDITOR_TO[edit]
        return cds, _effect_to(ed[0], edit_to), effect_class_mask(require_effect), effect_class_mask(forbid_effect), None

    def _effects_on_handle(self, held, shape, fx, count_fn, rows_fn, filter_fn, free_fn, rows=True):
        """As _edit_on_handle, for the effect rows: fx = what _effects_args returned.  With a require or forbid mask the handle
        is first replaced by the filter's result; the rows of the survivors come back as uint32[n, 2]."""
        cds, to, require, forbid, code = fx
        sh = shape._struct()
        if require or forbid:
            out = C.c_void_p()
            check(filter_fn(self.ctx._h, self._h, held[0], C.byref(sh), to, cds._h, code, require, forbid, C.byref(out)), self.ctx._h)
            free_fn(held[0])
            held[0] = out
        if not rows:
            return None
        r = np.empty((int(count_fn(held[0])), 2), dtype=np.uint32)
        st = _lib.EffectsStats()
        check(rows_fn(self.ctx._h, self._h, held[0], C.byref(sh), to, cds._h, code, ptr(r), None, 0, None, None, C.byref(st)), self.ctx._h)
        _eff_partial(st.as_dict(), False)
        return r

    def effects(self, loci_or_found, shape, to, cds, effects=True, coverage=False, code=None, allow_partial=False):
        """vsc_loci_effects: what a base editor's full conversion of every candidate's window does to the codons of a Cds, on
        the device from the resident planes.  shape: an EditShape or the name of a preset of EDITORS; to: the base
        the editor writes on the read strand (a letter or 0..3; None: EDITOR_TO of the preset, else the transition partner of
        the shape's base).  Returns (rows, effects, coverage, stats).  rows uint32[n, 2] (unpack_effect_row): the candidate's
        effects by class, 5 bits each, and the bits of its mask that lie in a segment; (EFFECTS_UNDEFINED, EFFECTS_UNDEFINED)
        where the site is undefined.  effects (EFFECT_DTYPE; None with effects=False): candidate, transcript, codon, info
        (unpack_effect_info: ref, alt, class, edited, at), ascending candidate and inside it ascending forward position.
        coverage (uint32[cds.n_tx, 2] with coverage=True, else None): the stop_gained effects of every transcript and the
        smallest codon among them (EFFECTS_UNDEFINED: none).  code: 64 letters instead of GENETIC_CODE.  stats: the candidates
        by class, with_effect, effects, by_class, transcripts_stopped, kernel_ms, wall_ms.  loci_or_found: as Genome.efficiency
        takes it.  Raises when a site is not resident on this object (a shard) unless allow_partial=True."""
        if isinstance(shape, str):
            if shape not in EDITORS:
                raise ValueError("shape names one of %s, or is an EditShape" % ", ".join(sorted(EDITORS)))
            to = EDITOR_TO[shape] if to is None else to
            shape = EDITORS[shape]
        if not isinstance(cds, Cds):
            raise ValueError("cds must be a Cds")
        t = _effect_to(shape, to)
        cd = _effect_code(code)
        _, loci = _pick_loci(loci_or_found)
        lo = _loci(loci, len(loci))
        n = len(lo)
        rows = np.empty((n, 2), dtype=np.uint32)
        cov = np.empty((cds.n_tx, 2), dtype=np.uint32) if coverage else None
        want = bool(effects)
        cap = min(max(n, 1024), 1 << 22) if want else 0
        ef = np.empty(cap, dtype=_lib.EFFECT_DTYPE) if want else None
        st = _lib.EffectsStats()
        sh = shape._struct()
        count = C.c_uint64()
        L = lib()
        rc = L.vsc_loci_effects(self.ctx._h, self._h, ptr(lo), n, C.byref(sh), t, cds._h, cd, ptr(rows), ptr(ef), cap, C.byref(count),
                                ptr(cov), C.byref(st))
        if rc == _lib.VSC_ERR_RANGE and want and cap < int(count.value) <= 0xFFFFFFFE:
            # (the rows, the coverage and the stats of the first call stand; the second brings the effects alone)
            cap = int(count.value)
            ef = np.empty(cap, dtype=_lib.EFFECT_DTYPE)
            check(L.vsc_loci_effects(self.ctx._h, self._h, ptr(lo), n, C.byref(sh), t, cds._h, cd, None, ptr(ef), cap, C.byref(count), None,
                                     None), self.ctx._h)
        else:
            check(rc, self.ctx._h)
        stats = st.as_dict()
        _eff_partial(stats, allow_partial)
        if want:
            ef = ef[:int(count.value)].copy()
        return rows, ef, cov, stats

    # ---- knock-out design (vsc_*_knockout) ---------------------------------------------------------------------------------
    @staticmethod
    def _knockout_args(shape, cds, min_frac, max_frac, min_edge, require, forbid, site_len):
        """(shape, cds, code, the limits as (min_frac, max_frac, min_edge, require, forbid) or None when none is given) - or None
        without a shape.  The shares and the names become integers here, once (knockout_cut_frac, knockout_flag_mask)."""
        given = [v is not None for v in (min_frac, max_frac, min_edge, require, forbid)]
        if shape is None:
            if cds is not None or any(given):
                raise ValueError("knockout_cds / min_cut_frac / max_cut_frac / min_cut_edge / require_knockout / forbid_knockout need "
                                 "knockout=shape")
            return None
        shape = _knockout_shape(shape, "knockout")
        if shape.site_len != site_len:
            raise ValueError("the shape's site_len is %d; these candidates are %d bases long" % (shape.site_len, site_len))
        if not isinstance(cds, Cds):
            raise ValueError("knockout= needs knockout_cds=, a Cds")
        limits = None
        if any(given):
            limits = (0 if min_frac is None else knockout_cut_frac(min_frac), 65535 if max_frac is None else knockout_cut_frac(max_frac, True),
                      0 if min_edge is None else int(min_edge), knockout_flag_mask(require), knockout_flag_mask(forbid))
            if limits[0] > limits[1]:
                raise ValueError("min_cut_frac is above max_cut_frac")
            if not 0 <= limits[2] <= 255:
                raise ValueError("min_cut_edge is 0 .. 255")
            if (limits[3] | limits[4]) >> 7:
                raise ValueError("require_knockout / forbid_knockout are masks over the 7 flags")
        return shape, cds, None, limits

    def _knockout_on_handle(self, held, ko, count_fn, rows_fn, filter_fn, free_fn, rows=True, filt=True):
        """As _fold_on_handle, for the knock-out rows: ko = what _knockout_args returned.  With limits the handle is first
        replaced by the filter's result."""
        shape, cds, code, limits = ko
        sh = shape._struct()
        if filt and limits is not None:
            lim = _lib.KnockoutLimits(*limits, (C.c_uint32 * 3)(0, 0, 0))
            out = C.c_void_p()
            check(filter_fn(self.ctx._h, self._h, held[0], C.byref(sh), cds._h, code, C.byref(lim), C.byref(out)), self.ctx._h)
            free_fn(held[0])
            held[0] = out
        if not rows:
            return None
        out_rows = np.empty((int(count_fn(held[0])), 4), dtype=np.uint32)
        st = _lib.KnockoutStats()
        check(rows_fn(self.ctx._h, self._h, held[0], C.byref(sh), cds._h, code, ptr(out_rows), None, C.byref(st)), self.ctx._h)
        return out_rows

    def knockout(self, loci_or_found, shape, cds, coverage=False, code=None):
        """vsc_loci_knockout: where the cut of every candidate falls in the coding sequence of a Cds and what a frameshift
        there does, on the device from the resident planes.  shape: a KnockoutShape or the name of a preset of
        KNOCKOUT_SHAPES.  Returns (rows, coverage, stats).  rows uint32[n, 4] (unpack_knockout_row names the fields):
        transcript; codon | frame << 30; frac | edge << 16 | flags << 24; d1 | d2 << 16 - KNOCKOUT_UNDEFINED four times where
        the locus is invalid or the site leaves its contig, (0xFFFFFFFF, 0, JUNCTION << 31, 0) where the cut is not inside one
        segment.  coverage (uint32[cds.n_tx, 2] with coverage=True, else None): the candidates that cut the transcript with
        NMD in both frames and the smallest codon among them (KNOCKOUT_UNDEFINED: none).  code: 64 letters instead of
        GENETIC_CODE.  stats: defined, undefined, coding, junction, ptc, nmd (a pair each: frames +1, +2), unknown, past_find,
        drains, drained, transcripts_covered, kernel_ms, wall_ms.  loci_or_found: as Genome.efficiency takes it.  A base
        that is not resident on this object (a shard) makes the walk that reads it UNKNOWN."""
        shape = _knockout_shape(shape)
        if not isinstance(cds, Cds):
            raise ValueError("cds must be a Cds")
        cd = _effect_code(code)
        _, loci = _pick_loci(loci_or_found)
        lo = _loci(loci, len(loci))
        n = len(lo)
        rows = np.empty((n, 4), dtype=np.uint32)
        cov = np.empty((cds.n_tx, 2), dtype=np.uint32) if coverage else None
        st = _lib.KnockoutStats()
        sh = shape._struct()
        check(lib().vsc_loci_knockout(self.ctx._h, self._h, ptr(lo), n, C.byref(sh), cds._h, cd, ptr(rows), ptr(cov), C.byref(st)),
              self.ctx._h)
        return rows, cov, st.as_dict()

    def edit(self, loci_or_found, shape, targets=None, pairs=True, coverage=False, allow_partial=False):
        """vsc_loci_edit: the editing windows of candidates under an EditShape (or the name of a preset of EDITORS), and their
        join with targets, on the device from the resident planes.  Returns (rows, pairs, coverage, stats).
        rows uint32[n, 2]: (mask, hits) per candidate - bit j of mask is set iff the read base at window position j is the
        editor's base, bit j of hits iff that base is a target as well; (EDIT_UNDEFINED, EDIT_UNDEFINED) where the site is
        undefined.  targets: (contig, pos) rows or an array with those fields in any order, duplicates allowed (edit_targets
        sorts them); None: no targets, hits = 0.  pairs (EDIT_PAIR_DTYPE; None with pairs=False or without targets): one per
        set bit of hits - candidate, target (the index in the CALLER's array; of duplicates the first), mask, info
        (unpack_edit_info: at, bystanders) - in ascending (candidate, target).  coverage (uint32[len(targets), 2] in the
        caller's order with coverage=True, else None): pairs of the target, fewest bystanders among them (EDIT_UNDEFINED: no
        pair).  stats: the candidates by class, with_hit, pairs, targets_covered (over distinct targets), kernel_ms, wall_ms
        and target_order (the caller's index of every sorted target).  loci_or_found: as Genome.efficiency takes it.  Raises
        when a site is not resident on this object (a shard) unless allow_partial=True."""
        if isinstance(shape, str):
            if shape not in EDITORS:
                raise ValueError("shape names one of %s, or is an EditShape" % ", ".join(sorted(EDITORS)))
            shape = EDITORS[shape]
        _, loci = _pick_loci(loci_or_found)
        lo = _loci(loci, len(loci))
        n = len(lo)
        tg = order = inverse = None
        if targets is not None:
            tg, order, inverse = edit_targets(targets)
        n_t = 0 if tg is None else len(tg)
        tp = ptr(tg) if n_t else None
        rows = np.empty((n, 2), dtype=np.uint32)
        cov = np.empty((n_t, 2), dtype=np.uint32) if coverage and tg is not None else None
        want_pairs = bool(pairs) and tg is not None
        cap = min(max(n, 1024), 1 << 22) if want_pairs else 0
        pr = np.empty(cap, dtype=_lib.EDIT_PAIR_DTYPE) if want_pairs else None
        st = _lib.EditStats()
        sh = shape._struct()
        count = C.c_uint64()
        L = lib()
        rc = L.vsc_loci_edit(self.ctx._h, self._h, ptr(lo), n, C.byref(sh), tp, n_t, ptr(rows), ptr(pr), cap, C.byref(count), ptr(cov),
                             C.byref(st))
        if rc == _lib.VSC_ERR_RANGE and want_pairs and cap < int(count.value) <= 0xFFFFFFFE:
            # (the rows, the coverage and the stats of the first call stand; the second brings the pairs alone)
            cap = int(count.value)
            pr = np.empty(cap, dtype=_lib.EDIT_PAIR_DTYPE)
            check(L.vsc_loci_edit(self.ctx._h, self._h, ptr(lo), n, C.byref(sh), tp, n_t, None, ptr(pr), cap, C.byref(count), None, None),
                  self.ctx._h)
        else:
            check(rc, self.ctx._h)
        stats = st.as_dict()
        _eff_partial(stats, allow_partial)
        if want_pairs:
            pr = pr[:int(count.value)].copy()
            pr["target"] = order[pr["target"].astype(np.int64)].astype(np.uint32)
            pr = pr[np.lexsort((pr["target"], pr["candidate"]))]
        if cov is not None:
            cov = cov[inverse]
        if order is not None:
            stats["target_order"] = order
        return rows, pr, cov, stats

    # ---- known variation under candidates (vsc_*_variation) --------------------------------------------------------------------
    @staticmethod
    def _variation_args(shape, variants, max_cost, max_by_zone, require_zones, site_len):
        """(shape, sorted variants, order, inverse, VariationFilterStruct or None) - or None without a shape."""
        if shape is None:
            if variants is not None or max_cost is not None or max_by_zone is not None or require_zones is not None:
                raise ValueError("variants / max_variant_cost / max_variants_by_zone / require_variant_zones need variation=shape")
            return None
        shape = _variation_shape(shape, "variation")
        if shape.site_len != site_len:
            raise ValueError("the shape's site_len is %d; these candidates are %d bases long" % (shape.site_len, site_len))
        if variants is None:
            raise ValueError("variation= needs variants=")
        vr, order, inverse = _variants_in(variants)
        filt = None
        if max_cost is not None or max_by_zone is not None or require_zones is not None:
            cost = 0xFFFFFFFF if max_cost is None else int(max_cost)
            by = [255, 255, 255, 255] if max_by_zone is None else [int(v) for v in max_by_zone]
            req = 0
            for z in (() if require_zones is None else require_zones):
                z = VARIATION_ZONES.index(z) if isinstance(z, str) and z in VARIATION_ZONES else z
                if isinstance(z, str) or not 0 <= int(z) <= 3:
                    raise ValueError("a required zone is 0..3 or one of %s" % ", ".join(VARIATION_ZONES))
                req |= 1 << int(z)
            if not 0 <= cost <= 0xFFFFFFFF or len(by) != 4 or any(not 0 <= v <= 255 for v in by):
                raise ValueError("max_variant_cost is an unsigned 32-bit number, max_variants_by_zone four numbers 0..255 (255: no bound)")
            filt = _lib.VariationFilterStruct(cost, by[0] | by[1] << 8 | by[2] << 16 | by[3] << 24, req, 0)
        return shape, vr, order, inverse, filt

    def _variation_on_handle(self, held, va, count_fn, rows_fn, filter_fn, free_fn, rows=True, filt=True):
        """As _edit_on_handle, for the variation rows: va = what _variation_args returned.  With a filter the handle is first
        replaced by the filter's result (filt); the rows of the survivors come back as uint32[n, 4]."""
        shape, vr, _, _, f = va
        sh = shape._struct()
        vp = ptr(vr) if len(vr) else None
        if filt and f is not None:
            out = C.c_void_p()
            check(filter_fn(self.ctx._h, self._h, held[0], C.byref(sh), vp, len(vr), C.byref(f), C.byref(out)), self.ctx._h)
            free_fn(held[0])
            held[0] = out
        if not rows:
            return None
        r = np.empty((int(count_fn(held[0])), 4), dtype=np.uint32)
        st = _lib.VariationStats()
        check(rows_fn(self.ctx._h, self._h, held[0], C.byref(sh), vp, len(vr), ptr(r), None, 0, None, None, C.byref(st)), self.ctx._h)
        _eff_partial(st.as_dict(), False)
        return r

    def variation(self, loci_or_found, shape, variants, pairs=True, coverage=False, allow_partial=False):
        """vsc_loci_variation: the known variants under candidates' own sites, on the device.  shape: a
        VariationShape or the name of a preset of VARIATION_SHAPES.  variants: (contig, pos, ref, alt[, weight]) rows in any
        order (site_variants sorts and normalises them), or a VARIANT_DTYPE array as the library takes it.  Returns (rows,
        pairs, coverage, stats).  rows uint32[n, 4] (unpack_variation_row): by_zone, silent, cost, max_weight per candidate;
        VARIATION_UNDEFINED four times where the site is undefined.  pairs (VARIATION_PAIR_DTYPE; None with pairs=False): one
        per overlapping variant, silent ones included - candidate, variant (the index in the CALLER's rows), info
        (unpack_variation_info: first, touched, top, silent), weight - in ascending (candidate, variant).  coverage
        (uint32[len(variants), 2] in the caller's order with coverage=True, else None): the disrupting and the silent pairs of
        every variant.  stats: the candidates by class, with_disrupting, pairs, variants_covered, kernel_ms, wall_ms and - for
        rows - variant_order (the caller's index of every sorted variant).  loci_or_found: as Genome.efficiency takes it.
        Raises when a site is not resident on this object (a shard) unless allow_partial=True."""
        shape = _variation_shape(shape)
        _, loci = _pick_loci(loci_or_found)
        lo = _loci(loci, len(loci))
        n = len(lo)
        vr, order, inverse = _variants_in(variants)
        n_v = len(vr)
        vp = ptr(vr) if n_v else None
        rows = np.empty((n, 4), dtype=np.uint32)
        cov = np.empty((n_v, 2), dtype=np.uint32) if coverage else None
        want_pairs = bool(pairs)
        cap = min(max(n, 1024), 1 << 22) if want_pairs else 0
        pr = np.empty(cap, dtype=_lib.VARIATION_PAIR_DTYPE) if want_pairs else None
        st = _lib.VariationStats()
        sh = shape._struct()
        count = C.c_uint64()
        L = lib()
        rc = L.vsc_loci_variation(self.ctx._h, self._h, ptr(lo), n, C.byref(sh), vp, n_v, ptr(rows), ptr(pr), cap, C.byref(count), ptr(cov),
                                  C.byref(st))
        if rc == _lib.VSC_ERR_RANGE and want_pairs and cap < int(count.value) <= 0xFFFFFFFE:
            # (the rows, the coverage and the stats of the first call stand; the second brings the pairs alone)
            cap = int(count.value)
            pr = np.empty(cap, dtype=_lib.VARIATION_PAIR_DTYPE)
            check(L.vsc_loci_variation(self.ctx._h, self._h, ptr(lo), n, C.byref(sh), vp, n_v, None, ptr(pr), cap, C.byref(count), None, None),
                  self.ctx._h)
        else:
            check(rc, self.ctx._h)
        stats = st.as_dict()
        _eff_partial(stats, allow_partial)
        if want_pairs:
            pr = _variation_pairs_out(pr[:int(count.value)].copy(), order)
        if cov is not None and inverse is not None:
            cov = cov[inverse]
        if order is not None:
            stats["variant_order"] = order
        return rows, pr, cov, stats

    # ---- prime-editing extensions (vsc_*_prime) ---------------------------------------------------------------------------
    @staticmethod
    def _prime_args(shape, edits, allow_weak, site_len):
        """(shape, sorted edits or None, order, inverse, allow_weak or None) - or None without a shape."""
        if shape is None:
            if edits is not None or allow_weak is not None:
                raise ValueError("prime_edits / prime_allow_weak need prime=shape")
            return None
        shape = _prime_shape(shape, "prime")
        if shape.site_len != site_len:
            raise ValueError("the shape's site_len is %d; these candidates are %d bases long" % (shape.site_len, site_len))
        ed = order = inverse = None
        if edits is not None:
            ed, order, inverse = prime_edits(edits)
        return shape, ed, order, inverse, None if allow_weak is None else bool(allow_weak)

    def _prime_on_handle(self, held, pe, count_fn, rows_fn, filter_fn, free_fn, rows=True, filt=True):
        """As _edit_on_handle, for the prime rows: pe = what _prime_args returned.  With edits or prime_allow_weak the handle
        is first replaced by the filter's result (filt); the rows of the survivors come back as uint32[n, 2]."""
        shape, ed, _, _, allow_weak = pe
        sh = shape._struct()
        n_e = 0 if ed is None else len(ed)
        ep = ptr(ed) if n_e else None
        if filt and (ed is not None or allow_weak is not None):
            out = C.c_void_p()
            check(filter_fn(self.ctx._h, self._h, held[0], C.byref(sh), ep, n_e, 1 if allow_weak in (None, True) else 0, C.byref(out)),
                  self.ctx._h)
            free_fn(held[0])
            held[0] = out
        if not rows:
            return None
        r = np.empty((int(count_fn(held[0])), 2), dtype=np.uint32)
        st = _lib.PrimeStats()
        check(rows_fn(self.ctx._h, self._h, held[0], C.byref(sh), ep, n_e, ptr(r), None, 0, None, None, C.byref(st)), self.ctx._h)
        _eff_partial(st.as_dict(), False)
        return r

    def prime(self, loci_or_found, shape, edits=None, pairs=True, coverage=False, allow_partial=False):
        """vsc_loci_prime: the pegRNA extensions of candidates under a PrimeShape (or the name of a preset of PRIME_EDITORS) for
        a list of wanted edits, on the device from the resident planes.  Returns (rows, pairs, coverage, stats).
        rows uint32[n, 2]: (pbs, n_pairs) per candidate - unpack_prime_row gives pbs_len, pbs_gc and WEAK, n_pairs is the number
        of edits the candidate can write; (PRIME_UNDEFINED, PRIME_UNDEFINED) where the context is undefined.  edits: (contig,
        pos, del_len, ins) rows or a PRIME_EDIT_DTYPE array in any order (prime_edits sorts them and refuses two at one
        position); None: no edits, n_pairs = 0.  pairs (PRIME_PAIR_DTYPE; None with pairs=False or without edits): candidate,
        edit (the index in the CALLER's array), info (unpack_prime_info: t, d, h, flags), ext (unpack_prime_ext: length, gc,
        pbs_len) - in ascending (candidate, edit).  coverage (uint32[len(edits), 2] in the caller's order with coverage=True,
        else None): pairs of the edit, smallest t among them (PRIME_UNDEFINED: no pair).  stats: the candidates by class,
        with_pair, weak, pairs, pairs_by_flag, edits_covered, score_ms, wall_ms and edit_order (the caller's index of every
        sorted edit).  loci_or_found: as Genome.efficiency takes it.  Raises when a context is not resident on this object (a
        shard) unless allow_partial=True."""
        shape = _prime_shape(shape)
        _, loci = _pick_loci(loci_or_found)
        lo = _loci(loci, len(loci))
        n = len(lo)
        ed = order = inverse = None
        if edits is not None:
            ed, order, inverse = prime_edits(edits)
        n_e = 0 if ed is None else len(ed)
        ep = ptr(ed) if n_e else None
        rows = np.empty((n, 2), dtype=np.uint32)
        cov = np.empty((n_e, 2), dtype=np.uint32) if coverage and ed is not None else None
        want_pairs = bool(pairs) and ed is not None
        cap = min(max(n, 1024), 1 << 22) if want_pairs else 0
        pr = np.empty(cap, dtype=_lib.PRIME_PAIR_DTYPE) if want_pairs else None
        st = _lib.PrimeStats()
        sh = shape._struct()
        count = C.c_uint64()
        L = lib()
        rc = L.vsc_loci_prime(self.ctx._h, self._h, ptr(lo), n, C.byref(sh), ep, n_e, ptr(rows), ptr(pr), cap, C.byref(count), ptr(cov),
                              C.byref(st))
        if rc == _lib.VSC_ERR_RANGE and want_pairs and cap < int(count.value) <= 0xFFFFFFFE:
            # (the rows, the coverage and the stats of the first call stand; the second brings the pairs alone)
            cap = int(count.value)
            pr = np.empty(cap, dtype=_lib.PRIME_PAIR_DTYPE)
            check(L.vsc_loci_prime(self.ctx._h, self._h, ptr(lo), n, C.byref(sh), ep, n_e, None, ptr(pr), cap, C.byref(count), None, None),
                  self.ctx._h)
        else:
            check(rc, self.ctx._h)
        stats = st.as_dict()
        _eff_partial(stats, allow_partial)
        if want_pairs:
            pr = pr[:int(count.value)].copy()
            pr["edit"] = order[pr["edit"].astype(np.int64)].astype(np.uint32)
            pr = pr[np.lexsort((pr["edit"], pr["candidate"]))]
        if cov is not None:
            cov = cov[inverse]
        if order is not None:
            stats["edit_order"] = order
        return rows, pr, cov, stats

    # ---- HDR knock-in design (vsc_*_hdr) ----------------------------------------------------------------------------------
    @staticmethod
    def _hdr_args(shape, edits, cds, allow_open, site_len, code=None):
        """(shape, sorted edits or None, order, inverse, cds or None, code, allow_open or None) - or None without a shape."""
        if shape is None:
            if edits is not None or cds is not None or allow_open is not None:
                raise ValueError("hdr_edits / hdr_cds / hdr_allow_open need hdr=shape")
            return None
        shape = _hdr_shape(shape, "hdr")
        if shape.site_len != site_len:
            raise ValueError("the shape's site_len is %d; these candidates are %d bases long" % (shape.site_len, site_len))
        if cds is not None and not isinstance(cds, Cds):
            raise ValueError("hdr_cds must be a Cds")
        ed = order = inverse = None
        if edits is not None:
            ed, order, inverse = prime_edits(edits)
        return shape, ed, order, inverse, cds, _effect_code(code), None if allow_open is None else bool(allow_open)

    def _hdr_on_handle(self, held, hd, count_fn, rows_fn, filter_fn, free_fn, rows=True, filt=True):
        """As _prime_on_handle, for the HDR rows: hd = what _hdr_args returned.  With edits or hdr_allow_open the handle is
        first replaced by the filter's result (filt); the rows of the survivors come back as uint32[n, 2]."""
        shape, ed, _, _, cds, code, allow_open = hd
        sh = shape._struct()
        n_e = 0 if ed is None else len(ed)
        ep = ptr(ed) if n_e else None
        ch = cds._h if cds is not None else None
        if filt and (ed is not None or allow_open is not None):
            out = C.c_void_p()
            check(filter_fn(self.ctx._h, self._h, held[0], C.byref(sh), ep, n_e, ch, code, 1 if allow_open else 0, C.byref(out)), self.ctx._h)
            free_fn(held[0])
            held[0] = out
        if not rows:
            return None
        r = np.empty((int(count_fn(held[0])), 2), dtype=np.uint32)
        st = _lib.HdrStats()
        check(rows_fn(self.ctx._h, self._h, held[0], C.byref(sh), ep, n_e, ch, code, ptr(r), None, 0, None, None, C.byref(st)), self.ctx._h)
        _eff_partial(st.as_dict(), False)
        return r

    def hdr(self, loci_or_found, shape, edits=None, cds=None, code=None, pairs=True, coverage=False, allow_partial=False):
        """vsc_loci_hdr: knock-in design by homology-directed repair for candidates under an HdrShape (or the name of a preset of
        HDR_NUCLEASES) and a list of wanted edits, on the device from the resident planes.  Returns (rows, pairs,
        coverage, stats).  rows uint32[n, 2]: (n_pairs, n_usable) per candidate - the edits in reach of its break, and those
        among them whose repaired allele the nuclease does not cut again; (HDR_UNDEFINED, HDR_UNDEFINED) where the context is
        undefined.  edits: as Genome.prime takes them; None: no edits, both 0.  cds: a Cds - a blocking substitution inside
        its segments is synonymous (under `code`, 64 letters, or GENETIC_CODE); None: any substitution is allowed.  pairs
        (HDR_PAIR_DTYPE; None with pairs=False or without edits): candidate, edit (the index in the CALLER's array), info
        (unpack_hdr_info: dist, side, seed_mm, proto_mm, flags), block (unpack_hdr_block: q, letter, coding, r) - in ascending
        (candidate, edit).  coverage (uint32[len(edits), 2] in the caller's order with coverage=True, else None): usable pairs
        of the edit, smallest dist among them (HDR_UNDEFINED: none).  stats: the candidates by class, with_pair, with_usable,
        pairs, pairs_by_flag, edits_covered, score_ms, wall_ms and edit_order.  loci_or_found: as Genome.efficiency takes it.
        Raises when a context is not resident on this object (a shard) unless allow_partial=True."""
        shape = _hdr_shape(shape)
        if cds is not None and not isinstance(cds, Cds):
            raise ValueError("cds must be a Cds")
        cd = _effect_code(code)
        ch = cds._h if cds is not None else None
        _, loci = _pick_loci(loci_or_found)
        lo = _loci(loci, len(loci))
        n = len(lo)
        ed = order = inverse = None
        if edits is not None:
            ed, order, inverse = prime_edits(edits)
        n_e = 0 if ed is None else len(ed)
        ep = ptr(ed) if n_e else None
        rows = np.empty((n, 2), dtype=np.uint32)
        cov = np.empty((n_e, 2), dtype=np.uint32) if coverage and ed is not None else None
        want_pairs = bool(pairs) and ed is not None
        cap = min(max(n, 1024), 1 << 22) if want_pairs else 0
        pr = np.empty(cap, dtype=_lib.HDR_PAIR_DTYPE) if want_pairs else None
        st = _lib.HdrStats()
        sh = shape._struct()
        count = C.c_uint64()
        L = lib()
        rc = L.vsc_loci_hdr(self.ctx._h, self._h, ptr(lo), n, C.byref(sh), ep, n_e, ch, cd, ptr(rows), ptr(pr), cap, C.byref(count), ptr(cov),
                            C.byref(st))
        if rc == _lib.VSC_ERR_RANGE and want_pairs and cap < int(count.value) <= 0xFFFFFFFE:
            # (the rows, the coverage and the stats of the first call stand; the second brings the pairs alone)
            cap = int(count.value)
            pr = np.empty(cap, dtype=_lib.HDR_PAIR_DTYPE)
            check(L.vsc_loci_hdr(self.ctx._h, self._h, ptr(lo), n, C.byref(sh), ep, n_e, ch, cd, None, ptr(pr), cap, C.byref(count), None, None),
                  self.ctx._h)
        else:
            check(rc, self.ctx._h)
        stats = st.as_dict()
        _eff_partial(stats, allow_partial)
        if want_pairs:
            pr = pr[:int(count.value)].copy()
            pr["edit"] = order[pr["edit"].astype(np.int64)].astype(np.uint32)
            pr = pr[np.lexsort((pr["edit"], pr["candidate"]))]
        if cov is not None:
            cov = cov[inverse]
        if order is not None:
            stats["edit_order"] = order
        return rows, pr, cov, stats

    def pick(self, loci_or_found, key, shape, regions=None, groups=None, target=None, n_targets=None, rank=False):
        """The best shape.k candidates of every target under `key` (uint64 per candidate, larger is better), no two of one
        target closer than shape.spacing bases at their cut sites - picked on the device.  loci_or_found: as
        Genome.efficiency takes it.  The targets: either target= (uint32 per candidate, REGION_NONE: none; vsc_loci_pick) with
        n_targets=, or regions= a Regions - the target of a candidate is the label of its first base, or groups[label] with
        groups= (uint32 per interval as given to the Regions, REGION_NONE: the interval belongs to no target); the labels are
        made on the device inside the first kernel (vsc_loci_pick_regions).
        n_targets defaults to the largest target + 1 / the number of groups' targets / the number of intervals.  Returns
        (picks uint32[n_targets, k], counts uint32[n_targets][, rank uint32[n]], stats): picks[t, r] is the index of the r-th
        pick of target t, PICK_NONE beyond counts[t]; rank[i] = r where candidate i is the r-th pick of its target."""
        codes, loci = _pick_loci(loci_or_found)
        lo = _loci(loci, len(loci))
        n = len(lo)
        ky = np.ascontiguousarray(key, dtype=np.uint64)
        if len(ky) != n:
            raise ValueError("one key per candidate")
        if (regions is None) == (target is None):
            raise ValueError("exactly one of regions= and target= must be given")
        if groups is not None and regions is None:
            raise ValueError("groups= needs regions=")
        L = lib()
        st = _lib.PickStats()
        sh = shape._struct()
        if target is not None:
            tg = np.ascontiguousarray(target, dtype=np.uint32)
            if len(tg) != n:
                raise ValueError("one target per candidate")
            if n_targets is None:
                named = tg[tg != _lib.REGION_NONE]
                n_targets = int(named.max()) + 1 if len(named) else 0
            picks, counts, rk = _pick_arrays(n, int(n_targets), shape.k, rank)
            check(L.vsc_loci_pick(self.ctx._h, self._h, ptr(lo), n, ptr(tg), ptr(ky), int(n_targets), C.byref(sh), ptr(picks), ptr(counts),
                                  ptr(rk) if rk is not None else None, C.byref(st)), self.ctx._h)
            return (picks, counts) + ((rk,) if rank else ()) + (st.as_dict(),)
        gr = None
        if groups is not None:
            gr = np.ascontiguousarray(groups, dtype=np.uint32)
            if len(gr) != regions.n_intervals:
                raise ValueError("groups holds %d entries for %d intervals" % (len(gr), regions.n_intervals))
            if n_targets is None:
                named = gr[gr != _lib.REGION_NONE]
                n_targets = int(named.max()) + 1 if len(named) else 0
        elif n_targets is None:
            n_targets = regions.n_intervals
        picks, counts, rk = _pick_arrays(n, int(n_targets), shape.k, rank)
        check(L.vsc_loci_pick_regions(self.ctx._h, self._h, ptr(lo), n, regions._h, ptr(gr) if gr is not None else None, ptr(ky), int(n_targets),
                                      C.byref(sh), ptr(picks), ptr(counts), ptr(rk) if rk is not None else None, C.byref(st)), self.ctx._h)
        return (picks, counts) + ((rk,) if rank else ()) + (st.as_dict(),)

    def _pick_found(self, pick, pick_by, pick_groups, regions, loci_or_found, columns):
        """design's / design_pattern's pick= : the key out of the columns the call computed (columns: name -> values, None
        where the call did not compute it) in the fixed quantisation of pick_column, then Genome.pick."""
        if not isinstance(pick, PickShape):
            raise ValueError("pick must be a PickShape")
        if regions is None:
            raise ValueError("pick= needs targets")
        names = list(pick_by) if pick_by is not None else [next(iter(columns))]
        cols = []
        for name in names:
            if name not in columns:
                raise ValueError("this call cannot rank by %r" % (name,))
            if columns[name] is None:
                raise ValueError("pick_by=%r needs the option that computes it" % (name,))
            cols.append(pick_column(name, columns[name]))
        key = pick_key(cols, [PICK_COLUMNS[name] for name in names])
        picks, counts, _ = self.pick(loci_or_found, key, pick, regions=regions, groups=pick_groups)
        return picks, counts

    def efficiency(self, loci_or_found, model, allow_partial=False):
        """vsc_loci_efficiency (vsc_loci_efficiency_trees for a TreeEfficiencyModel): the linear predictors of candidates under an
        EfficiencyModel or a TreeEfficiencyModel, computed on the device from the
        resident planes: (linear float64[n], stats).  loci_or_found: what enumerate_guides returns (its loci are taken), a
        PatternGuides, or a LOCUS_DTYPE array / (contig, pos, strand) rows - a locus names the site's first base on the
        forward strand.  An undefined predictor is the NaN with bits EFF_UNDEFINED_BITS; stats counts the candidates by
        class: defined, invalid, off_contig, not_resident, has_n.  Raises when a context is not resident on this object (a
        shard) unless allow_partial=True."""
        if isinstance(loci_or_found, PatternGuides):
            loci = loci_or_found.loci
        elif isinstance(loci_or_found, tuple) and len(loci_or_found) >= 2 and isinstance(loci_or_found[1], np.ndarray) \
                and loci_or_found[1].dtype == _lib.LOCUS_DTYPE:
            loci = loci_or_found[1]
        else:
            loci = loci_or_found
        lo = _loci(loci, len(loci))
        linear = np.empty(len(lo), dtype=np.float64)
        st = _lib.EffStats()
        fn = lib().vsc_loci_efficiency_trees if isinstance(model, TreeEfficiencyModel) else lib().vsc_loci_efficiency
        check(fn(self.ctx._h, self._h, ptr(lo), len(lo), model._h, ptr(linear), C.byref(st)), self.ctx._h)
        stats = st.as_dict()
        _eff_partial(stats, allow_partial)
        return linear, stats

    def summarize(self, guides, max_mismatches, extra_pam=None, algorithm="auto", exclude=None, regions=None):
        """vsc_search_summary: per guide, the NM counts, the fixed-point MIT sum (units of 2^-24), the reference-UB count
        and whether the excluded locus was a hit - over the hits search() would return, without the records.
        exclude: None or one (contig, pos, strand) per guide (contig 0xFFFFFFFF: none).  Returns SUMMARY_DTYPE rows - or,
        with regions (a Regions; vsc_search_summary_regions), the pair (those rows, the same over the hits in the regions)."""
        codes = guides if isinstance(guides, np.ndarray) else pack_guides(guides)
        codes = np.ascontiguousarray(codes, dtype=np.uint64)
        p = self._params(max_mismatches, extra_pam, algorithm)
        ex = _loci(exclude, len(codes))
        out = np.zeros(len(codes), dtype=_lib.SUMMARY_DTYPE)
        if regions is None:
            check(lib().vsc_search_summary(self.ctx._h, self._h, ptr(codes), len(codes), C.byref(p), ptr(ex), ptr(out)), self.ctx._h)
            return out
        inside = np.zeros(len(codes), dtype=_lib.SUMMARY_DTYPE)
        check(lib().vsc_search_summary_regions(self.ctx._h, self._h, ptr(codes), len(codes), C.byref(p), ptr(ex), regions._h, ptr(out),
                                               ptr(inside)), self.ctx._h)
        return out, inside

    def summarize_variants(self, guides, max_mismatches, vmap, exclude=None, batch=0, extra_pam=None, algorithm="auto"):
        """vsc_search_summary_variants on a window genome: per guide the SUMMARY_DTYPE rows over the counted window hits
        (`all`), over those that carry a variant (`var`), and the dropped duplicates - (all, var, duplicates).  vmap: the
        VariantMap of this genome; exclude: None or one (contig, pos, strand) per guide IN REFERENCE COORDINATES, the locus the
        guide was taken from; batch: guides per pass (0: the default), the rows do not depend on it."""
        codes = guides if isinstance(guides, np.ndarray) else pack_guides(guides)
        codes = np.ascontiguousarray(codes, dtype=np.uint64)
        p = self._params(max_mismatches, extra_pam, algorithm)
        ex = _loci(exclude, len(codes))
        rows, var = np.zeros(len(codes), dtype=_lib.SUMMARY_DTYPE), np.zeros(len(codes), dtype=_lib.SUMMARY_DTYPE)
        dups = np.zeros(len(codes), dtype=np.uint64)
        check(lib().vsc_search_summary_variants(self.ctx._h, self._h, vmap._h, ptr(codes), len(codes), C.byref(p), ptr(ex), int(batch),
                                                ptr(rows), ptr(var), ptr(dups)), self.ctx._h)
        return rows, var, dups

    def search_select(self, guides, max_mismatches, top_k=0, min_score=0, extra_pam=None, algorithm="auto", exclude=None,
                      summary=False, regions=None, region_scope="keep"):
        """vsc_search_select: per guide, of the hits search() would return (minus the excluded locus), those with
        rint(MIT * 2^24) >= min_score (mit_fixed() turns an MIT value into one) and of them the top_k best by (score
        descending, strand, position); 0 = no floor / no limit.  Returns Hits sorted as search() sorts them - or, with
        summary=True, (Hits, the SUMMARY_DTYPE rows of summarize() for the same arguments) from the one search.
        regions (a Regions; vsc_search_select_regions): the selection is made among the hits in the regions
        (region_scope="keep") or among those outside (region_scope="drop"); with summary=True the result is then (Hits, rows,
        rows over the hits in the regions), the two row sets of summarize(..., regions=regions) whatever the scope."""
        codes = guides if isinstance(guides, np.ndarray) else pack_guides(guides)
        codes = np.ascontiguousarray(codes, dtype=np.uint64)
        p = self._params(max_mismatches, extra_pam, algorithm)
        sel = _select(top_k, min_score)
        ex = _loci(exclude, len(codes))
        flt = _region_filter(regions, region_scope)
        rows = np.zeros(len(codes), dtype=_lib.SUMMARY_DTYPE) if summary else None
        h = C.c_void_p()
        if flt is None:
            check(lib().vsc_search_select(self.ctx._h, self._h, ptr(codes), len(codes), C.byref(p), C.byref(sel), ptr(ex), ptr(rows),
                                          C.byref(h)), self.ctx._h)
            hits = Hits(self, h, codes)
            return (hits, rows) if summary else hits
        inside = np.zeros(len(codes), dtype=_lib.SUMMARY_DTYPE) if summary else None
        check(lib().vsc_search_select_regions(self.ctx._h, self._h, ptr(codes), len(codes), C.byref(p), C.byref(sel), C.byref(flt),
                                              ptr(ex), ptr(rows), ptr(inside), C.byref(h)), self.ctx._h)
        hits = Hits(self, h, codes)
        return (hits, rows, inside) if summary else hits

    def summarize_classified(self, guides, max_mismatches, forest, activity, extra_pam=None, algorithm="auto", exclude=None):
        """vsc_search_summary_classified: summarize() and, from the same search, the classifier's rows - per guide the sum of
        the forest's votes over the counted hits, the hits it calls active (2 * votes > n_trees), the ties and the active
        ones by NM - without the records.  forest: a classifier.Forest; activity: the on-target activity per guide.
        Returns (SUMMARY_DTYPE rows, VOTES_DTYPE rows)."""
        codes = guides if isinstance(guides, np.ndarray) else pack_guides(guides)
        codes = np.ascontiguousarray(codes, dtype=np.uint64)
        p = self._params(max_mismatches, extra_pam, algorithm)
        ex = _loci(exclude, len(codes))
        cls, keep = _classify(forest, activity, len(codes))
        out = np.zeros(len(codes), dtype=_lib.SUMMARY_DTYPE)
        votes = np.zeros(len(codes), dtype=_lib.VOTES_DTYPE)
        check(lib().vsc_search_summary_classified(self.ctx._h, self._h, ptr(codes), len(codes), C.byref(p), ptr(ex), C.byref(cls),
                                                  ptr(out), ptr(votes)), self.ctx._h)
        del keep
        return out, votes

    def search_select_classified(self, guides, max_mismatches, forest, activity, top_k=0, min_votes=0, extra_pam=None,
                                 algorithm="auto", exclude=None, summary=False):
        """vsc_search_select_classified: per guide, of the hits search() would return (minus the excluded locus), those with at
        least min_votes of the forest's votes and of them the top_k best by (votes descending, strand, position); 0 = no floor
        / no limit.  Returns Hits sorted as search() sorts them (forest.classify_hits gives the survivors' votes) - or, with
        summary=True, (Hits, SUMMARY_DTYPE rows, VOTES_DTYPE rows) over all counted hits from the one search."""
        codes = guides if isinstance(guides, np.ndarray) else pack_guides(guides)
        codes = np.ascontiguousarray(codes, dtype=np.uint64)
        p = self._params(max_mismatches, extra_pam, algorithm)
        ex = _loci(exclude, len(codes))
        cls, keep = _classify(forest, activity, len(codes))
        sel = _lib.SelectVotes(int(top_k), int(min_votes), (C.c_uint32 * 2)(0, 0))
        rows = np.zeros(len(codes), dtype=_lib.SUMMARY_DTYPE) if summary else None
        votes = np.zeros(len(codes), dtype=_lib.VOTES_DTYPE) if summary else None
        h = C.c_void_p()
        check(lib().vsc_search_select_classified(self.ctx._h, self._h, ptr(codes), len(codes), C.byref(p), C.byref(sel), C.byref(cls),
                                                 ptr(ex), ptr(rows), ptr(votes), C.byref(h)), self.ctx._h)
        del keep
        hits = Hits(self, h, codes)
        return (hits, rows, votes) if summary else hits

    def summarize_table(self, guides, max_mismatches, table, extra_pam=None, algorithm="auto", exclude=None, plain=False):
        """vsc_search_summary_table: per guide, over the hits search() would return (minus the excluded locus), the sum of the
        table's fixed-point scores (units of 2^-30; table_specificity() turns it into a specificity), the hits that score
        above 0 and those by NM - without the records.  table: a ScoreTable.  Returns TABLE_ROW_DTYPE rows - or, with
        plain=True, (SUMMARY_DTYPE rows of summarize(), those rows) from the one search."""
        codes = guides if isinstance(guides, np.ndarray) else pack_guides(guides)
        codes = np.ascontiguousarray(codes, dtype=np.uint64)
        p = self._params(max_mismatches, extra_pam, algorithm)
        ex = _loci(exclude, len(codes))
        out = np.zeros(len(codes), dtype=_lib.SUMMARY_DTYPE) if plain else None
        rows = np.zeros(len(codes), dtype=_lib.TABLE_ROW_DTYPE)
        check(lib().vsc_search_summary_table(self.ctx._h, self._h, ptr(codes), len(codes), C.byref(p), ptr(ex), table._h, ptr(out),
                                             ptr(rows)), self.ctx._h)
        return (out, rows) if plain else rows

    def search_select_table(self, guides, max_mismatches, table, top_k=0, min_score=0, extra_pam=None, algorithm="auto",
                            exclude=None, summary=False):
        """vsc_search_select_table: search_select() with the table's fixed-point score as the key - min_score in units of
        2^-30, order (score descending, strand, position).  Returns Hits sorted as search() sorts them (Hits.table_scores
        gives the survivors' scores) - or, with summary=True, (Hits, TABLE_ROW_DTYPE rows over all counted hits)."""
        codes = guides if isinstance(guides, np.ndarray) else pack_guides(guides)
        codes = np.ascontiguousarray(codes, dtype=np.uint64)
        p = self._params(max_mismatches, extra_pam, algorithm)
        sel = _select(top_k, min_score)
        ex = _loci(exclude, len(codes))
        rows = np.zeros(len(codes), dtype=_lib.TABLE_ROW_DTYPE) if summary else None
        h = C.c_void_p()
        check(lib().vsc_search_select_table(self.ctx._h, self._h, ptr(codes), len(codes), C.byref(p), C.byref(sel), ptr(ex), table._h,
                                            ptr(rows), C.byref(h)), self.ctx._h)
        hits = Hits(self, h, codes)
        return (hits, rows) if summary else hits

    def enumerate_guides(self, regions=None, pam="GG", strands="both", gc=(0, 0), max_t_run=0, max_guides=0, params=None,
                         labels=False, efficiency=None, min_efficiency=None, microhomology=None, min_out_of_frame=None,
                         min_microhomology=None, edit=None, edit_targets=None, min_editable=None, max_editable=None, cds=None,
                         edit_to=None, require_effect=None, forbid_effect=None, prime=None, prime_edits=None, prime_allow_weak=None,
                         variation=None, variants=None, max_variant_cost=None, max_variants_by_zone=None, require_variant_zones=None,
                         hdr=None, hdr_edits=None, hdr_cds=None, hdr_allow_open=None, fold=None, fold_scaffold=None,
                         max_fold_starts=None, max_fold_self=None, max_fold_scaffold=None, max_fold_seed=None, motifs=None, motif_set=None, motif_left=None, motif_right=None,
                         forbid_motifs=None, forbid_context_motifs=None, require_cut_motifs=None, cut_only=None, knockout=None, knockout_cds=None,
                          min_cut_frac=None, max_cut_frac=None, min_cut_edge=None, require_knockout=None, forbid_knockout=None):
        """vsc_guides_enumerate: the candidate guides of this genome (or shard) - every N-free 23-base window that ends in
        `pam` on '+' or starts with its reverse complement on '-' - that lie in `regions` (a Regions, under its own rule; None:
        everywhere), with gc[0] <= G/C of the 20 protospacer bases <= gc[1] (gc[1] = 0: no upper bound) and no run of more
        than max_t_run T in them (0: no limit).  Returns (codes uint64[n], loci LOCUS_DTYPE[n]) in ascending (contig, pos),
        '+' before '-': codes are what every search takes, loci what `exclude` takes.  More than max_guides (0: no cap)
        candidates raise VarscotError -34.  params: an EnumParams to pass as it is (tests).
        labels=True (needs regions; or labels=another Regions): returns (codes, loci, labels uint32[n]) - per candidate the
        index of the interval it lies in, REGION_NONE if none, as Regions.locate gives it (vsc_guides_locate, on the device).
        efficiency= an EfficiencyModel or a TreeEfficiencyModel with site_len 23: the candidates' linear predictors (float64[n], computed where the
        candidates lie on the device: vsc_guides_efficiency) come last in the returned tuple.  min_efficiency=x (needs
        efficiency=): only the candidates whose predictor is defined and >= x, linear domain (vsc_guides_filter_efficiency).
        microhomology= a MicrohomologyShape with site_len 23: the candidates' (sum, oof) pairs (uint32[n, 2],
        vsc_guides_microhomology) come last of all, after the predictors.  min_out_of_frame=x (per cent) /
        min_microhomology=y (score units; both need microhomology=): only the candidates whose score is defined, at least y,
        and out of frame for at least x per cent of it (vsc_guides_filter_microhomology).
        edit= an EditShape with site_len 23 or the name of a preset of EDITORS: the candidates' (mask, hits) rows (uint32[n, 2],
        vsc_guides_edit) come last of all.  edit_targets= (contig, pos) rows in any order / min_editable= / max_editable= (all
        need edit=): only the candidates whose site is defined, whose window holds min_editable .. max_editable editable
        bases and - with targets - reaches a target (vsc_guides_filter_edit), on the device after the other floors.
        cds= a Cds (needs edit=): the candidates' effect rows (uint32[n, 2], vsc_guides_effects) come last of all, after the
        edit rows.  edit_to= the base the editor writes (default: EDITOR_TO of a preset, else the transition partner of the
        shape's base) / require_effect= / forbid_effect= class names of EFFECT_CLASSES (all need cds=): only the candidates
        with an effect of a required class and none of a forbidden one (vsc_guides_filter_effects), after the edit filter.
        prime= a PrimeShape with site_len 23 or the name of a preset of PRIME_EDITORS: the candidates' (pbs, n_pairs) rows
        (uint32[n, 2], vsc_guides_prime) come last of all.  prime_edits= (contig, pos, del_len, ins) rows in any order /
        prime_allow_weak= (both need prime=): only the candidates whose context is defined, that - with edits - can write one of
        them, and - with prime_allow_weak=False - whose PBS is not WEAK (vsc_guides_filter_prime), after the edit and effects
        filters.
        variation= a VariationShape with site_len 23 or the name of a preset of VARIATION_SHAPES, with variants= (as
        Genome.variation takes them): the candidates' variation rows (uint32[n, 4], vsc_guides_variation) come last of all.
        max_variant_cost= / max_variants_by_zone= four bounds (255: none) / require_variant_zones= zone numbers or names of
        VARIATION_ZONES (all need variation=): only the candidates that pass the variation filter
        (vsc_guides_filter_variation), after the other filters.
        hdr= an HdrShape with site_len 23 or the name of a preset of HDR_NUCLEASES: the candidates' (n_pairs, n_usable) rows
        (uint32[n, 2], vsc_guides_hdr) come last of all.  hdr_edits= (contig, pos, del_len, ins) rows in any order / hdr_cds= a
        Cds / hdr_allow_open= (all need hdr=): with edits or hdr_allow_open only the candidates whose context is defined and
        that - with edits - have a usable pair, or with hdr_allow_open=True any pair (vsc_guides_filter_hdr), after the other
        families' filters.
        fold= a FoldShape with site_len 23 or the name of a preset of FOLD_SHAPES: the candidates' fold rows (uint32[n, 2],
        vsc_guides_fold; unpack_fold_row names the fields) come last of all, after the HDR rows.  fold_scaffold= the constant part
        of the guide RNA (at most 128 letters of A C G T U; default: none) / max_fold_starts= / max_fold_self= /
        max_fold_scaffold= / max_fold_seed= whole numbers 0 .. 32 (all need fold=): with a limit only the candidates whose row is
        defined and within every limit (vsc_guides_filter_fold), after the HDR filter.
        motifs= a MotifShape with site_len 23 (or the name of a preset of MOTIF_SHAPES) with motif_set= a
        MotifSet (motifs(...)) or its entries: the candidates' motif rows (uint64[n, 3]: construct, cut, elsewhere;
        vsc_guides_motifs; unpack_motif_row names the bits) come last of all, after the fold rows.  motif_left= /
        motif_right= the vector's text on either side of the cloned spacer (at most 16 letters of A C G T U; default: none) /
        forbid_motifs= / forbid_context_motifs= / require_cut_motifs= names or bit masks / cut_only= (all need motifs=): with one of
        them only the candidates whose row is defined and passes FILTER (vsc_guides_filter_motifs), after the fold
        filter.
        knockout= a KnockoutShape with site_len 23 (or the name of a preset of KNOCKOUT_SHAPES) with
        knockout_cds= a Cds: the candidates' knock-out rows (uint32[n, 4], vsc_guides_knockout; unpack_knockout_row names
        the fields) come last of all, after the motif rows.  min_cut_frac= / max_cut_frac= shares of the protein, floats in 0 .. 1
        (knockout_cut_frac states how they become 0 .. 65535) / min_cut_edge= 0 .. 255 bases to the nearer end of the exon /
        require_knockout= / forbid_knockout= flag names of KNOCKOUT_FLAGS or masks (all need knockout=): with one of them only
        the candidates whose cut is a coding cut and passes FILTER (vsc_guides_filter_knockout), after the motif
        filter."""
        lab = _label_regions(labels, regions)
        p = params if params is not None else _enum_params(pam, strands, gc, max_t_run, max_guides)
        self._eff_args(efficiency, min_efficiency, READ_LEN)
        mh = self._mh_args(microhomology, min_out_of_frame, min_microhomology, READ_LEN)
        ed = self._edit_args(edit, edit_targets, min_editable, max_editable, READ_LEN)
        fx = self._effects_args(ed, edit, cds, edit_to, require_effect, forbid_effect)
        pe = self._prime_args(prime, prime_edits, prime_allow_weak, READ_LEN)
        vr = self._variation_args(variation, variants, max_variant_cost, max_variants_by_zone, require_variant_zones, READ_LEN)
        hd = self._hdr_args(hdr, hdr_edits, hdr_cds, hdr_allow_open, READ_LEN)
        fo = self._fold_args(fold, fold_scaffold, max_fold_starts, max_fold_self, max_fold_scaffold, max_fold_seed, READ_LEN)
        mo = self._motif_args(motifs, motif_set, motif_left, motif_right, forbid_motifs, forbid_context_motifs, require_cut_motifs, cut_only, READ_LEN)
        ko = self._knockout_args(knockout, knockout_cds, min_cut_frac, max_cut_frac, min_cut_edge, require_knockout, forbid_knockout, READ_LEN)
        L = lib()
        h = C.c_void_p()
        check(L.vsc_guides_enumerate(self.ctx._h, self._h, regions._h if regions is not None else None, C.byref(p), C.byref(h)),
              self.ctx._h)
        if efficiency is None and mh is None and ed is None and pe is None and vr is None and hd is None and fo is None and mo is None and ko is None:
            return _guides_arrays(h, lambda code: check(code, self.ctx._h), lab)
        held = [h]
        try:
            extra = self._scores_on_handle(held, efficiency, min_efficiency, mh, L.vsc_guides_count,
                                           (L.vsc_guides_efficiency, L.vsc_guides_filter_efficiency),
                                           (L.vsc_guides_microhomology, L.vsc_guides_filter_microhomology), L.vsc_guides_free,
                                           ed, (L.vsc_guides_edit, L.vsc_guides_filter_edit), fx,
                                           (L.vsc_guides_effects, L.vsc_guides_filter_effects), pe,
                                           (L.vsc_guides_prime, L.vsc_guides_filter_prime), vr,
                                           (L.vsc_guides_variation, L.vsc_guides_filter_variation), hd,
                                           (L.vsc_guides_hdr, L.vsc_guides_filter_hdr), fo,
                                           (L.vsc_guides_fold, L.vsc_guides_filter_fold), mo,
                                           (L.vsc_guides_motifs, L.vsc_guides_filter_motifs), ko,
                                           (L.vsc_guides_knockout, L.vsc_guides_filter_knockout))
        except BaseException:
            L.vsc_guides_free(held[0])
            raise
        return _guides_arrays(held[0], lambda code: check(code, self.ctx._h), lab) + extra

    def enumerate_pairs(self, delta, regions=None, **filters):
        """enumerate_guides(regions, **filters) and the guide pairs among its candidates (vsc_guides_pairs, on the device
        over the candidates where they lie): returns (codes, loci, pairs) - pairs uint32[n, 2], every (a, b) with candidate
        a on '-', candidate b on '+' of the same contig and delta[0] <= pos(b) - pos(a) <= delta[1] (nickase_delta turns an
        offset range into one), in ascending (a, b).  With labels= the labels come last."""
        lab = _label_regions(filters.pop("labels", False), regions)
        params = filters.pop("params", None)
        p = params if params is not None else _enum_params(filters.pop("pam", "GG"), filters.pop("strands", "both"),
                                                           filters.pop("gc", (0, 0)), filters.pop("max_t_run", 0),
                                                           filters.pop("max_guides", 0))
        if filters:
            raise TypeError("unknown filter: %s" % ", ".join(sorted(filters)))
        h = C.c_void_p()
        check(lib().vsc_guides_enumerate(self.ctx._h, self._h, regions._h if regions is not None else None, C.byref(p), C.byref(h)),
              self.ctx._h)
        chk = lambda code: check(code, self.ctx._h)  # noqa: E731
        try:
            pairs = _guides_pairs(h, chk, delta)
        except BaseException:
            lib().vsc_guides_free(h)
            raise
        found = _guides_arrays(h, chk, lab)
        return (found[0], found[1], pairs) + tuple(found[2:])

    def design(self, regions, max_mismatches, pam="GG", strands="both", gc=(0, 0), max_t_run=0, max_guides=0, labels=False,
               efficiency=None, min_efficiency=None, microhomology=None, min_out_of_frame=None, min_microhomology=None,
               pick=None, pick_by=None, pick_groups=None, edit=None, edit_targets=None, min_editable=None, max_editable=None,
               cds=None, edit_to=None, require_effect=None, forbid_effect=None, prime=None, prime_edits=None, prime_allow_weak=None,
               variation=None, variants=None, max_variant_cost=None, max_variants_by_zone=None, require_variant_zones=None,
               hdr=None, hdr_edits=None, hdr_cds=None, hdr_allow_open=None, fold=None, fold_scaffold=None, max_fold_starts=None,
               max_fold_self=None, max_fold_scaffold=None, max_fold_seed=None, motifs=None, motif_set=None, motif_left=None, motif_right=None,
               forbid_motifs=None, forbid_context_motifs=None, require_cut_motifs=None, cut_only=None, knockout=None, knockout_cds=None,
                          min_cut_frac=None, max_cut_frac=None, min_cut_edge=None, require_knockout=None, forbid_knockout=None, **search_options):
        """Every guide of `regions`, with its specificity: enumerate_guides(regions, ...) followed by summarize(codes,
        max_mismatches, exclude=loci, **search_options) on the same resident genome.  Returns (codes, loci, rows) - or, with
        summarize's own regions= option among the search options, (codes, loci, (rows, rows over the hits in those regions)).
        A PAM other than GG / GA needs extra_pam=pam among the search options for the guide's own locus to be a hit.
        labels: as enumerate_guides; the labels then come last: (codes, loci, rows, labels).
        efficiency= / min_efficiency=: as enumerate_guides; only the survivors are searched, and the linear predictors come
        last of all: (codes, loci, rows[, labels], linear).  microhomology= / min_out_of_frame= / min_microhomology=: as
        enumerate_guides; the pairs come after the predictors.
        pick= a PickShape: the best pick.k guides of every interval of `regions` (pick_groups= uint32 per interval: of every
        group of intervals), Genome.pick under a key made of what this call computed - pick_by= column names in priority
        order out of "mit" (the default; rint(100 x specificity), 14 bits), "eff" (the top 20 bits of order_bits of the
        predictor), "oof" (floor(1000 oof / sum), 10 bits) and "mh" (min(sum, 2^20 - 1), 20 bits); a column whose option was
        not given is refused.  (picks, counts) come last of all.  Without pick= nothing changes.
        edit= / edit_targets= / min_editable= / max_editable=: as enumerate_guides; only the survivors are searched, and the
        edit rows come after the microhomology pairs, before (picks, counts).  cds= / edit_to= / require_effect= /
        forbid_effect=: as enumerate_guides; the effect rows come after the edit rows.  prime= / prime_edits= /
        prime_allow_weak=: as enumerate_guides; the prime rows come after the effect rows, before (picks, counts).
        variation= / variants= / max_variant_cost= / max_variants_by_zone= / require_variant_zones=: as enumerate_guides; only
        the survivors are searched, and the variation rows come after the prime rows, before (picks, counts).
        hdr= / hdr_edits= / hdr_cds= / hdr_allow_open=: as enumerate_guides; only the survivors are searched, and the HDR rows
        come after the variation rows, before (picks, counts).
        fold= / fold_scaffold= / max_fold_starts= / max_fold_self= / max_fold_scaffold= / max_fold_seed=: as enumerate_guides; only
        the survivors are searched, and the fold rows come after the HDR rows, before (picks, counts); pick_by= then knows the
        column "fold" (32 - starts, 6 bits: fewer stems are better).
        motifs= / motif_set= / motif_left= / motif_right= / forbid_motifs= / forbid_context_motifs= / require_cut_motifs= / cut_only=:
        as enumerate_guides; only the survivors are searched, and the motif rows come after the fold rows, before (picks, counts);
        pick_by= then knows the column "rflp" (the motifs over the cut and nowhere else in the context, 6 bits: more are better).
        knockout= / knockout_cds= / min_cut_frac= / max_cut_frac= / min_cut_edge= / require_knockout= / forbid_knockout=: as
        enumerate_guides; only the survivors are searched, and the knock-out rows come after the motif rows, before (picks,
        counts); pick_by= then knows the column "knockout" (17 bits: bit 16 = NMD in both frames, bits 0 .. 15 = 65535 - frac, so
        that among equals the earlier cut wins; no coding cut: 0)."""
        if pick is None and (pick_by is not None or pick_groups is not None):
            raise ValueError("pick_by= / pick_groups= need pick=")
        found = self.enumerate_guides(regions, pam=pam, strands=strands, gc=gc, max_t_run=max_t_run, max_guides=max_guides,
                                      labels=labels, efficiency=efficiency, min_efficiency=min_efficiency,
                                      microhomology=microhomology, min_out_of_frame=min_out_of_frame,
                                      min_microhomology=min_microhomology, edit=edit, edit_targets=edit_targets,
                                      min_editable=min_editable, max_editable=max_editable, cds=cds, edit_to=edit_to,
                                      require_effect=require_effect, forbid_effect=forbid_effect, prime=prime,
                                      prime_edits=prime_edits, prime_allow_weak=prime_allow_weak, variation=variation,
                                      variants=variants, max_variant_cost=max_variant_cost,
                                      max_variants_by_zone=max_variants_by_zone, require_variant_zones=require_variant_zones,
                                      hdr=hdr, hdr_edits=hdr_edits, hdr_cds=hdr_cds, hdr_allow_open=hdr_allow_open, fold=fold,
                                      fold_scaffold=fold_scaffold, max_fold_starts=max_fold_starts, max_fold_self=max_fold_self,
                                      max_fold_scaffold=max_fold_scaffold, max_fold_seed=max_fold_seed, motifs=motifs,
                                      motif_set=motif_set, motif_left=motif_left, motif_right=motif_right, forbid_motifs=forbid_motifs,
                                      forbid_context_motifs=forbid_context_motifs, require_cut_motifs=require_cut_motifs,
                                      cut_only=cut_only, knockout=knockout, knockout_cds=knockout_cds, min_cut_frac=min_cut_frac,
                                      max_cut_frac=max_cut_frac, min_cut_edge=min_cut_edge, require_knockout=require_knockout,
                                      forbid_knockout=forbid_knockout)
        codes, loci = found[0], found[1]
        rows = self.summarize(codes, max_mismatches, exclude=loci, **search_options)
        out = (codes, loci, rows) + tuple(found[2:])
        if pick is None:
            return out
        extra = list(found[3:] if len(found) > 2 and _label_regions(labels, regions) is not None else found[2:])
        linear = extra.pop(0) if efficiency is not None else None
        pairs = extra.pop(0) if microhomology is not None else None
        kos = extra.pop() if knockout is not None else None
        sites = extra.pop() if motifs is not None else None
        folds = extra[-1] if fold is not None else None
        all_rows = rows[0] if isinstance(rows, tuple) else rows
        spec = np.array([mit_specificity(x) for x in all_rows["mit_sum"]], dtype=np.float64)
        return out + self._pick_found(pick, pick_by, pick_groups, regions, (codes, loci),
                                      {"mit": spec, "eff": linear, "oof": pairs, "mh": pairs, "fold": folds, "rflp": sites,
                                       "knockout": kos})

    def search_streamed(self, guides, max_mismatches, on_batch, batch=0, extra_pam=None, algorithm="auto"):
        """vsc_search_stream: the reads are searched in batches of `batch` (0 = the library's maximum, 16 384)
        and on_batch(hits, first_guide, n_guides) is called with every batch's result - a Hits object that is
        only valid inside the call (score it, copy it out, gather it; the library frees it afterwards).
        Record order and read indices are those of one big search.  ctx.timing() afterwards holds sums."""
        codes = guides if isinstance(guides, np.ndarray) else pack_guides(guides)
        codes = np.ascontiguousarray(codes, dtype=np.uint64)
        p = self._params(max_mismatches, extra_pam, algorithm)
        failure = []

        def trampoline(_user, handle, first, count):
            try:
                h = Hits(self, C.c_void_p(handle), codes, owned=False)
                try:
                    on_batch(h, int(first), int(count))
                finally:
                    h.close()
                return 0
            except BaseException as e:  # no exception may cross the C boundary
                failure.append(e)
                return -5

        cb = _lib.BATCH_FN(trampoline)
        rc = lib().vsc_search_stream(self.ctx._h, self._h, ptr(codes), len(codes), C.byref(p), int(batch), cb, None)
        if failure:
            raise failure[0]
        check(rc, self.ctx._h)


    def search_streamed_rows(self, guides, max_mismatches, on_batch, batch=0, extra_pam=None, algorithm="auto"):
        """vsc_search_stream_rows: as search_streamed, and every batch arrives with its 64-byte packed feature rows -
        on_batch(hits, first_guide, n_guides, rows_dev) with rows_dev = device address of len(hits) * 64 bytes (row i belongs
        to record i; valid inside the call; None for an empty batch).  The rows are written by the kernel that assembles the
        records - no second pass over the hits, no gather from the planes."""
        codes = guides if isinstance(guides, np.ndarray) else pack_guides(guides)
        codes = np.ascontiguousarray(codes, dtype=np.uint64)
        p = self._params(max_mismatches, extra_pam, algorithm)
        failure = []

        def trampoline(_user, handle, first, count, rows_dev):
            try:
                h = Hits(self, C.c_void_p(handle), codes, owned=False)
                try:
                    on_batch(h, int(first), int(count), rows_dev)
                finally:
                    h.close()
                return 0
            except BaseException as e:  # no exception may cross the C boundary
                failure.append(e)
                return -5

        cb = _lib.ROWS_BATCH_FN(trampoline)
        rc = lib().vsc_search_stream_rows(self.ctx._h, self._h, ptr(codes), len(codes), C.byref(p), int(batch), cb, None)
        if failure:
            raise failure[0]
        check(rc, self.ctx._h)


class ContigTable:
    """A genome object that carries a contig table alone (vsc_debug_genome_from_contigs, include/varscot_hip_debug.h) and
    sorts the caller's records over it (vsc_debug_sort_records): the tests' way to the bin sort.  contig_off: ascending
    global start positions; span: one past the last position, at most 2^32."""

    def __init__(self, ctx, contig_off, span):
        self.ctx = ctx
        self.contig_off = np.ascontiguousarray(contig_off, dtype=np.uint32)
        self.span = int(span)
        self._h = C.c_void_p()
        check(lib().vsc_debug_genome_from_contigs(ctx._h, ptr(self.contig_off), len(self.contig_off), self.span, C.byref(self._h)), ctx._h)
        ctx._children.add(self)

    def close(self):
        if self._h:
            lib().vsc_genome_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _sort(self, inp, keep):
        info, h = _lib.DebugSortInfo(), C.c_void_p()
        check(lib().vsc_debug_sort_records(self.ctx._h, self._h, C.byref(inp), C.byref(info), C.byref(h)), self.ctx._h)
        del keep  # (the arrays `inp` points into lived until here)
        return Hits(self, h, None), info.as_dict()

    def sort_slots(self, slots, segments, read_bits, pos_bits=0, pos_base=0, fill=None, fill_shift=0, slots_allowed=-1):
        """Seed form: `slots` (uint64: packed records, sentinels, anything in the holes of `fill`), `segments`
        (_lib.SORT_SEGMENT_DTYPE).  Returns (Hits, info dict: n, bytes, levels, bin_bits, slot_fallbacks, slots_allowed)."""
        slots = np.ascontiguousarray(slots, dtype=np.uint64)
        segments = np.ascontiguousarray(segments, dtype=_lib.SORT_SEGMENT_DTYPE)
        fill = None if fill is None else np.ascontiguousarray(fill, dtype=np.uint32)
        inp = _lib.DebugSortInput(pos_bits=pos_bits, pos_base=pos_base, read_bits=read_bits, slots=ptr(slots), n_slots=len(slots),
                                  segments=ptr(segments), n_segments=len(segments), fill=ptr(fill), fill_shift=fill_shift,
                                  slots_allowed=slots_allowed)
        return self._sort(inp, (slots, segments, fill))

    def sort_pairs(self, keys, vals, n_regions, guide_base=0, pos_bits=0, pos_base=0):
        """Scan form: (key, value) pairs as the streaming scan leaves them, through level 0.  Returns as sort_slots."""
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        vals = np.ascontiguousarray(vals, dtype=np.uint32)
        assert len(keys) == len(vals)
        inp = _lib.DebugSortInput(pos_bits=pos_bits, pos_base=pos_base, pair_keys=ptr(keys), pair_vals=ptr(vals), n_pairs=len(keys),
                                  n_regions=n_regions, guide_base=guide_base, slots_allowed=-1)
        return self._sort(inp, (keys, vals))


class Hits:
    """Result of one search (vsc_hits): records sorted by (guide, strand, contig, pos)."""

    def __init__(self, genome, handle, codes, owned=True):
        self.genome, self._h, self.codes = genome, handle, codes
        self.ctx = genome.ctx
        self._owned = owned  # a batch of search_streamed belongs to the library: never freed from here
        if owned:
            self.ctx._children.add(self)

    def __len__(self):
        return int(lib().vsc_hits_count(self._h))

    @property
    def device_ptr(self):
        return lib().vsc_hits_data_dev(self._h)

    def to_numpy(self):
        n = len(self)
        p = C.c_void_p()
        check(lib().vsc_hits_data(self._h, C.byref(p)), self.ctx._h)
        if n == 0:
            return np.zeros(0, dtype=HIT_DTYPE)
        buf = (C.c_char * (n * HIT_DTYPE.itemsize)).from_address(p.value)
        return np.frombuffer(buf, dtype=HIT_DTYPE).copy()

    def locate(self, regions):
        """vsc_hits_locate: per record the index of the interval of `regions` its window is in (uint32[len(self)], REGION_NONE:
        in none), as Regions.locate gives it - computed on the device over the records where they lie."""
        labels = np.full(len(self), _lib.REGION_NONE, dtype=np.uint32)
        check(lib().vsc_hits_locate(self._h, regions._h, ptr(labels)), self.ctx._h)
        return labels

    def variants(self, vmap, exclude=None):
        """vsc_hits_variants on a result of a window genome's search: per record a VARIANT_LABEL_DTYPE row - reference contig,
        position on the chromosome, covered variants, flags VARIANT_VAR / VARIANT_DUP / VARIANT_ON_TARGET - computed on the
        device over the records where they lie.  exclude: None or one (contig, pos, strand) per guide in reference coordinates."""
        labels = np.zeros(len(self), dtype=_lib.VARIANT_LABEL_DTYPE)
        ex = _loci(exclude, len(self.codes))
        check(lib().vsc_hits_variants(self._h, self.genome._h, vmap._h, ptr(ex), len(self.codes), ptr(labels)), self.ctx._h)
        return labels

    def pairs(self, pairs, delta, n_guides=None, exclude=None, sites=False, max_sites=0):
        """vsc_hits_pairs: for every guide pair (a, b) of `pairs` (uint32[n, 2]) the paired sites - a record of guide a and a
        record of guide b on opposite strands of one contig with delta[0] <= pos('+') - pos('-') <= delta[1] - joined on the
        device over the records where they lie.  Returns the rows (PAIR_SUMMARY_DTYPE[n]: sites, nm_sum, nm_max, on_target);
        with sites=True (rows, site records PAIR_SITE_DTYPE in ascending (pair, a_rec, b_rec)).  exclude: None or one
        (contig, pos, strand) per guide - the paired site at exclude[a], exclude[b] is the pair's on-target and is not
        counted.  n_guides: the guides the records were searched with (default: this result's).  max_sites: 0 sizes the site
        array from the rows (a second call); a max_sites below the total raises VarscotError -34."""
        pr = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 2)
        if n_guides is None:
            if self.codes is None:
                raise ValueError("a merged result does not know its guides: give n_guides")
            n_guides = len(self.codes)
        p = _pair_params(delta)
        ex = _loci(exclude, int(n_guides))
        rows = np.zeros(len(pr), dtype=_lib.PAIR_SUMMARY_DTYPE)
        total = C.c_uint64()
        L = lib()
        if not sites:
            check(L.vsc_hits_pairs(self._h, int(n_guides), ptr(pr), len(pr), C.byref(p), ptr(ex), ptr(rows), None, 0,
                                   C.byref(total)), self.ctx._h)
            return rows
        cap = int(max_sites)
        if cap == 0:  # size the sites from the rows
            check(L.vsc_hits_pairs(self._h, int(n_guides), ptr(pr), len(pr), C.byref(p), ptr(ex), ptr(rows), None, 0,
                                   C.byref(total)), self.ctx._h)
            cap = int(total.value)
        out = np.zeros(max(cap, 1), dtype=_lib.PAIR_SITE_DTYPE)
        check(L.vsc_hits_pairs(self._h, int(n_guides), ptr(pr), len(pr), C.byref(p), ptr(ex), ptr(rows), ptr(out), cap,
                               C.byref(total)), self.ctx._h)
        return rows, out[:int(total.value)].copy()

    def copy_to(self, dst_ptr, dst_is_device):
        """Copy the records to caller memory (e.g. the data_ptr() of a uint8 tensor handed to RCCL)."""
        check(lib().vsc_hits_copy(self._h, C.c_void_p(dst_ptr), int(bool(dst_is_device))), self.ctx._h)

    def pack_exchange(self, dst_ptr, dst_is_device):
        """vsc_hits_pack_exchange: the records as 8-byte exchange records into caller memory (len(self) * 8 bytes,
        e.g. the data_ptr() of a uint8 tensor handed to RCCL); returns the per-key record counts
        (uint32[2 * reads], key = read << 1 | strand)."""
        counts = np.zeros(2 * len(self.codes), dtype=np.uint32)
        check(lib().vsc_hits_pack_exchange(self.ctx._h, self.genome._h, self._h, len(self.codes), C.c_void_p(dst_ptr),
                                           int(bool(dst_is_device)), ptr(counts)), self.ctx._h)
        return counts

    def scores(self, first=0, count=None, mit=True, features=False):
        """(mit float64[count] | None, mit_flags uint8[count] | None, features uint8[count,442] | None)."""
        count = len(self) - first if count is None else count
        m = np.empty(count, dtype=np.float64) if mit else None
        fl = np.empty(count, dtype=np.uint8) if mit else None
        ft = np.empty((count, N_FEATURES), dtype=np.uint8) if features else None
        check(lib().vsc_score_hits(self.genome.ctx._h, self.genome._h, self._h, ptr(self.codes), len(self.codes),
                                   first, count, ptr(m), ptr(fl), ptr(ft)), self.genome.ctx._h)
        return m, fl, ft

    def table_scores(self, table, first=0, count=None, scores=True, fixed=True):
        """vsc_score_hits_table: (score float64[count] | None, fixed uint32[count] | None) of rows first .. first + count under
        a ScoreTable - per hit what ScoreTable.score gives for the hit's guide and its site in read orientation."""
        count = len(self) - first if count is None else count
        x = np.empty(count, dtype=np.float64) if scores else None
        f = np.empty(count, dtype=np.uint32) if fixed else None
        check(lib().vsc_score_hits_table(self.genome.ctx._h, self.genome._h, self._h, ptr(self.codes), len(self.codes), first, count,
                                         table._h, ptr(x), ptr(f)), self.genome.ctx._h)
        return x, f

    def packed_features(self, first=0, count=None, to_host=True, mit=False, dev_ptr=None):
        """vsc_score_hits_packed: 64-byte feature rows (uint32[count, 16]) and optionally MIT scores.
        dev_ptr: device memory for count * 64 bytes (e.g. a torch tensor's data_ptr()) that receives the rows;
        without it they pass through library scratch (to_host=False: computed and dropped - timing runs)."""
        count = len(self) - first if count is None else count
        rows = np.empty((count, 16), dtype=np.uint32) if to_host else None
        m = np.empty(count, dtype=np.float64) if mit else None
        check(lib().vsc_score_hits_packed(self.genome.ctx._h, self.genome._h, self._h, ptr(self.codes), len(self.codes),
                                          first, count, C.c_void_p(dev_ptr) if dev_ptr else None, ptr(rows), ptr(m)),
              self.genome.ctx._h)
        return rows, m

    def close(self):
        if self._h:
            if self._owned:
                lib().vsc_hits_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PatternHits:
    """Result of one pattern search kept on the device (vsc_pattern_hits; Genome.search_pattern_hits): PATTERN_HIT_DTYPE
    records in ascending (guide, strand, contig, pos) order, with one f word per record when the search was scored."""

    def __init__(self, genome, handle, n_guides, length, scored):
        self.genome, self._h, self.n_guides, self.length, self.scored = genome, handle, n_guides, length, scored
        self.ctx = genome.ctx
        self.ctx._children.add(self)

    def __len__(self):
        return int(lib().vsc_pattern_hits_count(self._h))

    def _copy(self, fn, itemsize, dtype):
        n = len(self)
        data = C.c_void_p()
        check(fn(self._h, C.byref(data)), self.ctx._h)
        if n == 0:
            return np.zeros(0, dtype=dtype)
        return np.frombuffer((C.c_char * (n * itemsize)).from_address(data.value), dtype=dtype).copy()

    def to_numpy(self):
        return self._copy(lib().vsc_pattern_hits_data, 20, PATTERN_HIT_DTYPE)

    def scores(self):
        """vsc_pattern_hits_scores: f = rint(score * 2^30) per record of a scored search."""
        if not self.scored:
            raise ValueError("the search was not scored")
        return self._copy(lib().vsc_pattern_hits_scores, 4, np.uint32)

    def variants(self, vmap, exclude=None):
        """vsc_pattern_hits_variants on a result of a window genome's pattern search: per record a VARIANT_LABEL_DTYPE row -
        reference contig, position on the chromosome, covered variants, flags VARIANT_VAR / VARIANT_DUP / VARIANT_ON_TARGET.
        exclude: None or one (contig, pos, strand) per guide in reference coordinates."""
        labels = np.zeros(len(self), dtype=_lib.VARIANT_LABEL_DTYPE)
        ex = _loci(exclude, self.n_guides)
        check(lib().vsc_pattern_hits_variants(self._h, self.genome._h, vmap._h, ptr(ex), self.n_guides, ptr(labels)), self.ctx._h)
        return labels

    def shadowed(self, vmap, exclude=None):
        """vsc_pattern_hits_shadowed on a result of the reference genome's pattern search: per record a uint8 of
        PATTERN_REF_SHADOWED (the site lies inside a window of vmap) | PATTERN_REF_ON_TARGET (the guide's own locus)."""
        flags = np.zeros(len(self), dtype=np.uint8)
        ex = _loci(exclude, self.n_guides)
        check(lib().vsc_pattern_hits_shadowed(self._h, self.genome._h, vmap._h, ptr(ex), self.n_guides, ptr(flags)), self.ctx._h)
        return flags

    def close(self):
        if self._h:
            lib().vsc_pattern_hits_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MergedHits(Hits):
    """Result of vsc_hits_merge: the records of all genome shards in global order (rank 0 only)."""

    def __init__(self, ctx, handle):
        self.ctx, self._h, self.codes, self.genome = ctx, handle, None, None
        self._owned = True
        ctx._children.add(self)

    def to_numpy(self):
        n = len(self)
        out = np.zeros(n, dtype=HIT_DTYPE)
        if n:
            check(lib().vsc_hits_copy(self._h, ptr(out), 0), self.ctx._h)
        return out

    def scores(self, *a, **k):
        raise NotImplementedError("score hits on the rank that owns the shard, before the gather")


def merge_shard_records(ctx, records_ptr, on_device, shard_counts, n_guides):
    """records_ptr: pointer to the vsc_hit records of all shards concatenated in shard order
    (shard_counts[s] each; device memory if on_device, e.g. the buffer RCCL gathered into)."""
    counts = np.ascontiguousarray(shard_counts, dtype=np.uint64)
    h = C.c_void_p()
    check(lib().vsc_hits_merge(ctx._h, C.c_void_p(records_ptr), int(bool(on_device)), ptr(counts), len(counts), n_guides,
                               C.byref(h)), ctx._h)
    return MergedHits(ctx, h)


def merge_packed_records(ctx, genome, records_ptr, on_device, key_counts, first_key=0, votes_ptr=None, votes_out_ptr=None,
                         votes_out_on_device=False):
    """vsc_hits_merge_packed: records_ptr = the 8-byte exchange records of all shards concatenated in shard order,
    key_counts = uint32[n_shards, n_keys] (records of shard s with key first_key + k); `genome` = any shard of the
    genome on `ctx` (contig table).  Returns the merged vsc_hit records (guide = key >> 1).
    votes_ptr / votes_out_ptr (vsc_hits_merge_packed_votes): one uint16 per exchange record, in the memory space of the
    records, that travelled with them (the votes of the shard's classifier) -> the same values in merged order."""
    kc = np.ascontiguousarray(key_counts, dtype=np.uint32)
    assert kc.ndim == 2
    h = C.c_void_p()
    if votes_ptr is None:
        check(lib().vsc_hits_merge_packed(ctx._h, genome._h, C.c_void_p(records_ptr), int(bool(on_device)), ptr(kc), kc.shape[0],
                                          int(first_key), kc.shape[1], C.byref(h)), ctx._h)
    else:
        check(lib().vsc_hits_merge_packed_votes(ctx._h, genome._h, C.c_void_p(records_ptr), C.c_void_p(votes_ptr), int(bool(on_device)),
                                                ptr(kc), kc.shape[0], int(first_key), kc.shape[1], C.byref(h), C.c_void_p(votes_out_ptr),
                                                int(bool(votes_out_on_device))), ctx._h)
    return MergedHits(ctx, h)


class MultiContext:
    """vsc_multi: the genome-sharded search of ONE process over several devices behind the C ABI (one context per
    entry of `devices`; ids may repeat - several contexts on one GPU).  search() returns the merged records on
    the first context."""

    def __init__(self, devices, rccl=None, rccl_library=None):
        """rccl / rccl_library: the hooks of vsc_multi_create_debug (None: vsc_multi_create) - rccl=False forces
        device copies, rccl=True insists on RCCL (also with one device), rccl="try" attempts it and falls back, rccl_library names the one library to load."""
        ids = (C.c_int * len(devices))(*devices)
        self._h = C.c_void_p()
        if rccl is None and rccl_library is None:
            check(lib().vsc_multi_create(ids, len(devices), C.byref(self._h)))
        else:
            p = _lib.MultiDebugParams(-1 if rccl is None else (2 if rccl == "try" else int(bool(rccl))),
                                      rccl_library.encode() if rccl_library else None)
            check(lib().vsc_multi_create_debug(ids, len(devices), C.byref(p), C.byref(self._h)))
        self.devices = list(devices)
        self._genomes = weakref.WeakSet()
        self._results = weakref.WeakSet()

    def _check(self, code):
        if code != 0:
            raise _lib.VarscotError(code, lib().vsc_multi_last_error(self._h).decode(errors="replace"))

    @property
    def uses_rccl(self):
        return bool(lib().vsc_multi_uses_rccl(self._h))

    def last_error(self):
        return lib().vsc_multi_last_error(self._h).decode(errors="replace")

    def set_debug(self, **hooks):
        """Context.set_debug on every context of the set."""
        d = _lib.DebugParams.defaults()
        for k, v in hooks.items():
            setattr(d, k, int(v))
        for i in range(len(self.devices)):
            check(lib().vsc_ctx_set_debug_params(lib().vsc_multi_ctx(self._h, i), C.byref(d) if hooks else None))

    def release_scratch(self):
        """vsc_multi_release_scratch: the pooled scratch of every context and the exchange buffers back to the devices."""
        self._check(lib().vsc_multi_release_scratch(self._h))

    def timing(self):
        t = _lib.MultiTiming()
        self._check(lib().vsc_multi_get_timing(self._h, C.byref(t)))
        return t.as_dict()

    def load_genome(self, packed):
        g = MultiGenome(self, packed)
        self._genomes.add(g)
        return g

    def close(self):
        if self._h:
            for r in list(self._results):
                r.close()
            for g in list(self._genomes):
                g.close()
            lib().vsc_multi_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _BorrowedContext:
    """The first context of a MultiContext as far as a result object needs it (owned by the vsc_multi)."""

    def __init__(self, handle):
        self._h = handle
        self._children = weakref.WeakSet()


class MultiGenome:
    def __init__(self, multi, packed):
        self.multi, self.packed = multi, packed
        self._h = C.c_void_p()
        hi, lo, nm = (np.ascontiguousarray(a, dtype=np.uint32) for a in (packed.hi, packed.lo, packed.nmask))
        contigs = np.ascontiguousarray(packed.contigs, dtype=CONTIG_DTYPE)
        multi._check(lib().vsc_multi_genome_load(multi._h, ptr(hi), ptr(lo), ptr(nm), len(hi), ptr(contigs), len(contigs),
                                                 C.byref(self._h)))

    def build_index(self, extra_pam=None):
        p = Genome._params(0, extra_pam, ALGO_SEED)
        self.multi._check(lib().vsc_multi_genome_build_index(self.multi._h, self._h, C.byref(p)))

    def search(self, guides, max_mismatches, extra_pam=None, algorithm="auto"):
        codes = guides if isinstance(guides, np.ndarray) else pack_guides(guides)
        codes = np.ascontiguousarray(codes, dtype=np.uint64)
        p = Genome._params(max_mismatches, extra_pam, algorithm)
        h = C.c_void_p()
        self.multi._check(lib().vsc_multi_search(self.multi._h, self._h, ptr(codes), len(codes), C.byref(p), C.byref(h)))
        res = MergedHits(_BorrowedContext(C.c_void_p(lib().vsc_multi_result_ctx(self.multi._h))), h)
        self.multi._results.add(res)
        return res

    def summarize(self, guides, max_mismatches, extra_pam=None, algorithm="auto", exclude=None, regions=None):
        """vsc_multi_search_summary: Genome.summarize over the shards, rows added on the host (with regions: both row sets,
        vsc_multi_search_summary_regions)."""
        codes = guides if isinstance(guides, np.ndarray) else pack_guides(guides)
        codes = np.ascontiguousarray(codes, dtype=np.uint64)
        p = Genome._params(max_mismatches, extra_pam, algorithm)
        ex = _loci(exclude, len(codes))
        out = np.zeros(len(codes), dtype=_lib.SUMMARY_DTYPE)
        if regions is None:
            self.multi._check(lib().vsc_multi_search_summary(self.multi._h, self._h, ptr(codes), len(codes), C.byref(p), ptr(ex),
                                                             ptr(out)))
            return out
        inside = np.zeros(len(codes), dtype=_lib.SUMMARY_DTYPE)
        self.multi._check(lib().vsc_multi_search_summary_regions(self.multi._h, self._h, ptr(codes), len(codes), C.byref(p), ptr(ex),
                                                                 regions._h, ptr(out), ptr(inside)))
        return out, inside

    def summarize_classified(self, guides, max_mismatches, forest, activity, extra_pam=None, algorithm="auto", exclude=None):
        """vsc_multi_search_summary_classified: Genome.summarize_classified over the shards, both row sets added on the host."""
        codes = guides if isinstance(guides, np.ndarray) else pack_guides(guides)
        codes = np.ascontiguousarray(codes, dtype=np.uint64)
        p = Genome._params(max_mismatches, extra_pam, algorithm)
        ex = _loci(exclude, len(codes))
        cls, keep = _classify(forest, activity, len(codes))
        out = np.zeros(len(codes), dtype=_lib.SUMMARY_DTYPE)
        votes = np.zeros(len(codes), dtype=_lib.VOTES_DTYPE)
        self.multi._check(lib().vsc_multi_search_summary_classified(self.multi._h, self._h, ptr(codes), len(codes), C.byref(p), ptr(ex),
                                                                    C.byref(cls), ptr(out), ptr(votes)))
        del keep
        return out, votes

    def summarize_table(self, guides, max_mismatches, table, extra_pam=None, algorithm="auto", exclude=None, plain=False):
        """vsc_multi_search_summary_table: Genome.summarize_table over the shards, the rows added on the host."""
        codes = guides if isinstance(guides, np.ndarray) else pack_guides(guides)
        codes = np.ascontiguousarray(codes, dtype=np.uint64)
        p = Genome._params(max_mismatches, extra_pam, algorithm)
        ex = _loci(exclude, len(codes))
        out = np.zeros(len(codes), dtype=_lib.SUMMARY_DTYPE) if plain else None
        rows = np.zeros(len(codes), dtype=_lib.TABLE_ROW_DTYPE)
        self.multi._check(lib().vsc_multi_search_summary_table(self.multi._h, self._h, ptr(codes), len(codes), C.byref(p), ptr(ex),
                                                               table._h, ptr(out), ptr(rows)))
        return (out, rows) if plain else rows

    def search_select(self, guides, max_mismatches, top_k=0, min_score=0, extra_pam=None, algorithm="auto", exclude=None,
                      summary=False, regions=None, region_scope="keep"):
        """vsc_multi_search_select: Genome.search_select over the shards; the merged records on the first context (with
        regions: vsc_multi_search_select_regions, results as Genome.search_select returns them)."""
        codes = guides if isinstance(guides, np.ndarray) else pack_guides(guides)
        codes = np.ascontiguousarray(codes, dtype=np.uint64)
        p = Genome._params(max_mismatches, extra_pam, algorithm)
        sel = _select(top_k, min_score)
        ex = _loci(exclude, len(codes))
        flt = _region_filter(regions, region_scope)
        rows = np.zeros(len(codes), dtype=_lib.SUMMARY_DTYPE) if summary else None
        inside = np.zeros(len(codes), dtype=_lib.SUMMARY_DTYPE) if summary and flt is not None else None
        h = C.c_void_p()
        if flt is None:
            self.multi._check(lib().vsc_multi_search_select(self.multi._h, self._h, ptr(codes), len(codes), C.byref(p), C.byref(sel),
                                                            ptr(ex), ptr(rows), C.byref(h)))
        else:
            self.multi._check(lib().vsc_multi_search_select_regions(self.multi._h, self._h, ptr(codes), len(codes), C.byref(p),
                                                                    C.byref(sel), C.byref(flt), ptr(ex), ptr(rows), ptr(inside), C.byref(h)))
        res = MergedHits(_BorrowedContext(C.c_void_p(lib().vsc_multi_result_ctx(self.multi._h))), h)
        self.multi._results.add(res)
        if not summary:
            return res
        return (res, rows) if flt is None else (res, rows, inside)

    def enumerate_guides(self, regions=None, pam="GG", strands="both", gc=(0, 0), max_t_run=0, max_guides=0, params=None,
                         labels=False):
        """vsc_multi_guides_enumerate: Genome.enumerate_guides over the shards, their arrays joined in shard order on the
        host - the same bytes as one device gives (the labels of labels= too: looked up on the host)."""
        lab = _label_regions(labels, regions)
        p = params if params is not None else _enum_params(pam, strands, gc, max_t_run, max_guides)
        h = C.c_void_p()
        self.multi._check(lib().vsc_multi_guides_enumerate(self.multi._h, self._h, regions._h if regions is not None else None,
                                                           C.byref(p), C.byref(h)))
        return _guides_arrays(h, self.multi._check, lab)

    def enumerate_pairs(self, delta, regions=None, **filters):
        """Genome.enumerate_pairs over the shards: the joined host-only candidates are paired on the host (vsc_guides_pairs
        hands them to vsc_loci_pairs) - the same bytes as one device gives."""
        lab = _label_regions(filters.pop("labels", False), regions)
        params = filters.pop("params", None)
        p = params if params is not None else _enum_params(filters.pop("pam", "GG"), filters.pop("strands", "both"),
                                                           filters.pop("gc", (0, 0)), filters.pop("max_t_run", 0),
                                                           filters.pop("max_guides", 0))
        if filters:
            raise TypeError("unknown filter: %s" % ", ".join(sorted(filters)))
        h = C.c_void_p()
        self.multi._check(lib().vsc_multi_guides_enumerate(self.multi._h, self._h, regions._h if regions is not None else None,
                                                           C.byref(p), C.byref(h)))
        try:
            pairs = _guides_pairs(h, self.multi._check, delta)
        except BaseException:
            lib().vsc_guides_free(h)
            raise
        found = _guides_arrays(h, self.multi._check, lab)
        return (found[0], found[1], pairs) + tuple(found[2:])

    def search_streamed(self, guides, max_mismatches, on_batch, batch=0, extra_pam=None, algorithm="auto", score=None,
                        forest=None, guide_activity=None):
        """vsc_multi_search_stream: the reads go through all shards in batches of `batch`; what `score` names is computed
        per hit on the shard that found it, before the exchange ("rows": the packed feature rows, computed and dropped;
        "votes": `forest` walked per hit with the reads' `guide_activity`, 2 bytes per hit travel with the record); every
        merged batch is handed to on_batch(hits, first_guide, n_guides, votes_dev) - votes_dev: device address (first
        device) of one uint16 per record, or None - and freed afterwards.  The exchange and merge of a batch run while the
        shards search the next one."""
        codes = guides if isinstance(guides, np.ndarray) else pack_guides(guides)
        codes = np.ascontiguousarray(codes, dtype=np.uint64)
        p = Genome._params(max_mismatches, extra_pam, algorithm)
        sc, keep = None, []
        if score:
            sc = _lib.MultiScore()
            sc.mode = {"rows": _lib.MULTI_SCORE_ROWS, "votes": _lib.MULTI_SCORE_VOTES}[score]
            if score == "votes":
                act = np.ascontiguousarray(guide_activity, dtype=np.float64)
                assert len(act) == len(codes)
                model = _lib.RfModel(forest.n_trees, forest.n_nodes, ptr(forest.status), ptr(forest.feature), ptr(forest.left),
                                     ptr(forest.right), ptr(forest.split), ptr(forest.node_class))
                keep += [act, model]
                sc.guide_activity = act.ctypes.data
                sc.model = C.pointer(model)
        failure = []
        rctx = _BorrowedContext(C.c_void_p(lib().vsc_multi_result_ctx(self.multi._h)))

        def trampoline(_user, handle, first, count, votes_dev):
            try:
                h = MergedHits(rctx, C.c_void_p(handle))
                h._owned = False  # the batch belongs to the library
                try:
                    on_batch(h, int(first), int(count), votes_dev)
                finally:
                    h.close()
                return 0
            except BaseException as e:  # no exception may cross the C boundary
                failure.append(e)
                return -5

        cb = _lib.MULTI_BATCH_FN(trampoline)
        rc = lib().vsc_multi_search_stream(self.multi._h, self._h, ptr(codes), len(codes), C.byref(p), int(batch),
                                           C.byref(sc) if sc is not None else None, cb, None)
        if failure:
            raise failure[0]
        self.multi._check(rc)

    def close(self):
        if self._h:
            lib().vsc_multi_genome_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class LazyNames:
    """The ids of a variant-window genome (millions of them), decoded from the library's name pool on demand."""

    def __init__(self, pool, offsets):
        self._pool, self._off = pool, offsets

    def __len__(self):
        return len(self._off) - 1

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[k] for k in range(*i.indices(len(self)))]
        if i < 0:
            i += len(self)
        return self._pool[int(self._off[i]):int(self._off[i + 1]) - 1].tobytes().decode()

    def __iter__(self):
        return (self[i] for i in range(len(self)))


def variant_windows(reference, vcf_path, sample=0, seq_len=23, threads=0):
    """vsc_windows_build: the alt-allele windows of one VCF sample column as a PackedGenome (the "SNP genome"
    of VARSCOT:296-307), built straight from the reference's packed planes - no FASTA in between."""
    L = lib()
    names = (C.c_char_p * len(reference.names))(*[n.encode() for n in reference.names])
    h = C.c_void_p()
    err = C.create_string_buffer(512)
    code = L.vsc_windows_build(str(vcf_path).encode(), sample, seq_len, threads, ptr(reference.hi), ptr(reference.lo),
                               ptr(reference.nmask), ptr(reference.contigs), names, len(reference.contigs), C.byref(h), err, 512)
    if code != 0:
        raise _lib.VarscotError(code, err.value.decode(errors="replace"))
    owner = _WindowsOwner(h)  # the arrays below are views of the library's memory: it lives as long as they do
    n, nw = int(L.vsc_windows_count(h)), int(L.vsc_windows_words(h))

    def view(address, ctype, count, dtype):
        a = np.ctypeslib.as_array(C.cast(address, C.POINTER(ctype)), shape=(count,)).view(dtype)
        return _OwnedArray.wrap(a, owner)

    out = PackedGenome.__new__(PackedGenome)
    out.hi, out.lo, out.nmask = (view(L.vsc_windows_plane(h, k), C.c_uint32, nw, np.uint32) for k in range(3))
    if n:
        out.contigs = view(L.vsc_windows_contigs(h), C.c_uint8, n * CONTIG_DTYPE.itemsize, CONTIG_DTYPE)
        offsets = view(L.vsc_windows_name_offsets(h), C.c_uint64, n + 1, np.uint64)
        pool = view(L.vsc_windows_name(h, 0, None), C.c_uint8, int(offsets[n]), np.uint8)
        out.names = LazyNames(pool, offsets)
    else:
        out.contigs, out.names = np.zeros(0, dtype=CONTIG_DTYPE), []
    return out


class _WindowsOwner:
    def __init__(self, handle):
        self._h = handle

    def __del__(self):
        try:
            if self._h:
                lib().vsc_windows_free(self._h)
                self._h = None
        except Exception:
            pass


class _OwnedArray(np.ndarray):
    """ndarray view that keeps the owner of its memory alive."""

    @classmethod
    def wrap(cls, a, owner):
        v = a.view(cls)
        v._owner = owner
        return v

    def __array_finalize__(self, obj):
        self._owner = getattr(obj, "_owner", None)


def unpack_features(rows):
    """Packed 64-byte feature rows -> dense uint8[n, 442] (vsc_unpack_features)."""
    rows = np.ascontiguousarray(rows, dtype=np.uint32).reshape(-1, 16)
    out = np.empty((len(rows), N_FEATURES), dtype=np.uint8)
    lib().vsc_unpack_features(ptr(rows), len(rows), ptr(out))
    return out


def sam_order(hits):
    """(order, secondary) in which read_mapping/bidir_mapping.cpp:167-187 writes a sorted result."""
    hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
    order = np.empty(len(hits), dtype=np.uint64)
    sec = np.empty(len(hits), dtype=np.uint8)
    lib().vsc_sam_order(ptr(hits), len(hits), ptr(order), ptr(sec))
    return order, sec


def device_count():
    return int(lib().vsc_device_count())
