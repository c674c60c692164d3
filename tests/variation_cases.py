"""Shared helpers of test_variation.py (GPU) and test_variation_cpu.py: the definition of the variation join
(include/varscot_hip.h: SHAPE, SITE, CLASS, VARIANTS, OVERLAP, SILENT, DISRUPTING, TOP, ROW, PAIR, COVERAGE, FILTER) in plain
Python on strings and lists, and the case builders.  A shape is (site_len, zone labels as a list, accepted letters per read
position as a list of strings); a variant is (contig, pos, span, alt letter or None, weight).  Per site there is one loop over
all variants of its contig: no search, no prefix maximum, no block table, and no bit of the library's packing - the touched
read positions are a list, the top zone its maximum, silence a letter looked up in a string."""
import functools

import numpy as np

import edit_cases as ed
import varscot_amd as va
from helpers import random_seq

CLASSES = ed.CLASSES
UNDEF = 0xFFFFFFFF
MAX_U32 = 0xFFFFFFFE
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
BIG = 5  # the long contig of the wide genome


# ---- shapes ---------------------------------------------------------------------------------------------------------------------
def spcas9():
    """23: ten distal, ten seed, N, GG - the PAM behind the protospacer."""
    return (23, [1] * 10 + [2] * 10 + [0, 3, 3], [""] * 20 + ["ACGT", "G", "G"])


def front16():
    """16: TTN in front of 13 protospacer bases - the PAM in front, the seed next to it."""
    return (16, [3, 3, 0] + [2] * 6 + [1] * 7, ["T", "T", "ACGT"] + [""] * 13)


def sacas32():
    """32: 26 protospacer bases, then NNGRRT - an `accept` with more than one letter, and letters in both of its words."""
    return (32, [1] * 16 + [2] * 10 + [0, 0, 3, 3, 3, 3], [""] * 26 + ["ACGT", "ACGT", "G", "AG", "AG", "T"])


def odd23():
    """23: a protospacer position that accepts a base, a PAM position that accepts none, labels in no order."""
    return (23, [3, 0, 2, 1] * 5 + [2, 3, 1], ["C", "", "AT", ""] * 5 + ["", "", "CGT"])


def cas12a27():
    """27: TTTV in front of 23 protospacer bases with an 8-base seed (va.VARIATION_SHAPES["Cas12a"])."""
    return (27, [3, 3, 3, 3] + [2] * 8 + [1] * 15, ["T", "T", "T", "ACG"] + [""] * 23)


SHAPES = {"spcas9": spcas9, "front16": front16, "sacas32": sacas32, "odd23": odd23, "cas12a27": cas12a27}


def shape_of(shape):
    site_len, zones, accept = shape
    return va.VariationShape(site_len, zones, [sum(1 << "ACGT".index(ch) for ch in a) for a in accept])


# ---- genomes --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def wide_genome(site_len=ed.SITE_LEN):
    """edit_cases.small_genome and one contig of 4 000 bases behind it: about 5 300 global positions, 21 lookup blocks of 256."""
    rng = np.random.default_rng([32, site_len])
    return ed.small_genome(site_len) + (random_seq(rng, 4000),)


def contig_array(contigs):
    return va.PackedGenome.from_sequences(list(contigs)).contigs


def loci_of(contigs, which):
    """Every (contig, p, strand) of the contigs in `which`: (contig, first, last) ranges of starts or contig numbers."""
    out = []
    for w in which:
        c, a, b = (w, 0, len(contigs[w]) + 1) if isinstance(w, int) else w
        out += [(c, p, s) for p in range(a, b) for s in (0, 1)]
    return out


# ---- variants -------------------------------------------------------------------------------------------------------------------
def snv(contigs, c, p, k=1, weight=1):
    """An SNV at (c, p) whose alt is the k-th letter after the reference's."""
    ref = contigs[c][p]
    return (c, p, 1, "ACGT"[("ACGT".index(ref) + k) % 4] if ref in "ACGT" else "A", weight)


def ordered(variants):
    """Ascending (contig, pos), ties in the given order: the order the library takes."""
    return sorted(variants, key=lambda v: (v[0], v[1]))


def variant_array(variants):
    out = np.zeros(len(variants), dtype=va.VARIANT_DTYPE)
    for k, (c, p, span, alt, w) in enumerate(variants):
        out[k] = (c, p, span | (4 if alt is None else "ACGT".index(alt)) << 16, w)
    return out


def variant_sets(contigs, site_len):
    """name -> (variants in library order, the contigs or ranges whose every locus the case looks at)."""
    main, second = ed.MAIN, ed.SECOND
    small = [0, 1, 2, main, second]
    sets = {"none": ([], small), "one": ([snv(contigs, main, 154, weight=7)], small)}
    third = [snv(contigs, c, p, 1 + p % 3, 1 + p % 5) for c in small for p in range(len(contigs[c]))
             if p % 3 == 0 or p == len(contigs[c]) - 1]
    sets["third"] = (third, small)
    sets["one_contig"] = ([v for v in third if v[0] == second], small)
    # every position with all three alts: ties, 3 x site_len SNVs under a site
    every = [snv(contigs, c, p, k, 2 + k) for c in (0, 1, 2) for p in range(len(contigs[c])) for k in (1, 2, 3)]
    every += [snv(contigs, main, p, k, 2 + k) for p in range(120, 330) for k in (1, 2, 3)]
    sets["every3"] = (every, [0, 1, 2, (main, 90, 340)])
    # deletions around the site at p0: ending at its first base and starting at its end (no overlap), one base at either edge,
    # and the whole site and more
    p0 = 200
    edges = []
    for span in range(1, 41):
        edges += [(main, p0 - span, span, None, span), (main, p0 + site_len, span, None, 100 + span),
                  (main, p0 - span + 1, span, None, 200 + span), (main, p0 + site_len - 1, span, None, 300 + span)]
    edges += [(main, p0 - 5, site_len + 10, None, 999), (main, p0, site_len, None, 998), (main, p0 - 40, site_len + 80, None, 997)]
    sets["edges"] = (ordered(edges), [(main, 130, 300)])
    # the first and last base of every contig, either side of every separator, deletions that end at a contig's last base
    ends = []
    for c in small:
        n = len(contigs[c])
        ends += [snv(contigs, c, 0, 1, 11), (c, 0, 2, None, 12), snv(contigs, c, n - 1, 2, 13), (c, n - 3, 3, None, 14), (c, 0, n, None, 15)]
    sets["ends"] = (ordered(ends), small)
    if len(contigs) > BIG:
        # a span of 3 000 bases over a dozen lookup blocks with short variants under it, a second long one that ends behind it,
        # variants behind both, and 600 positions without any: the prefix maximum, and blocks with no variant of their own
        long_ = [(BIG, 300, 3000, None, 5), (BIG, 1000, 2500, None, 6)]
        long_ += [snv(contigs, BIG, p, 1, 7) for p in range(310, 3290, 97)] + [(BIG, p, 9, None, 8) for p in range(350, 3200, 211)]
        long_ += [snv(contigs, BIG, p, 2, 9) for p in (3499, 3500, 3501, 3999)] + [snv(contigs, BIG, 3, 1, 10)]
        sets["long"] = (ordered(long_), [BIG])
        sets["third_wide"] = (third + [snv(contigs, BIG, p, 1, 3) for p in range(0, 600, 3)], small + [(BIG, 0, 700), (BIG, 2000, 2512)])
    # more than 255 disrupting records in one zone, and two weights of 0xFFFFFFFE
    sat = [(main, 420, 1, None, 1)] * 300 + [(main, 500, 2, None, MAX_U32), (main, 501, 1, None, MAX_U32), (main, 502, 1, None, 5)]
    sets["saturated"] = (sat, [(main, 380, 530)])
    return sets


# ---- the definition --------------------------------------------------------------------------------------------------------------
def touch(shape, locus, variant):
    """None when the variant does not overlap the site of locus, else (touched read positions, top, silent)."""
    site_len, zones, accept = shape
    c, p, strand = locus
    vc, pos, span, alt, _ = variant
    if vc != c:
        return None
    forward = list(range(max(pos, p), min(pos + span, p + site_len)))  # the bases of [pos, pos + span) inside [p, p + site_len)
    if not forward:
        return None
    read = sorted((site_len - 1 - (f - p)) if strand else (f - p) for f in forward)
    silent = False
    if alt is not None:
        letter = COMP[alt] if strand else alt
        silent = letter in accept[read[0]]
    return read, max(zones[j] for j in read), silent


def expected(contigs, loci, shape, variants, resident=None, planes=True):
    """What a variation call gives (planes=False: what vsc_variation_host gives, which has no letters and so calls a site with
    an N defined): {"rows": uint32[n, 4], "pairs": VARIATION_PAIR_DTYPE in ascending (candidate, variant),
    "coverage": uint32[n_v, 2], "stats", "by_zone": [[4 counts, unclamped] or None], "cost": [unclamped sum or None]}."""
    by_contig = {}
    for k, v in enumerate(variants):
        by_contig.setdefault(v[0], []).append((k, v))
    rows = np.empty((len(loci), 4), dtype=np.uint32)
    stats = dict.fromkeys(CLASSES, 0)
    stats.update(with_disrupting=0, pairs=0, variants_covered=0)
    pairs, by_zone, cost = [], [], []
    coverage = np.zeros((len(variants), 2), dtype=np.uint32)
    for i, locus in enumerate(loci):
        cls, _ = ed.site_of(contigs, locus, shape[0], resident)
        if cls == "has_n" and not planes:
            cls = "defined"
        stats[cls] += 1
        if cls != "defined":
            rows[i] = (UNDEF, UNDEF, UNDEF, UNDEF)
            by_zone.append(None)
            cost.append(None)
            continue
        zone, silent, total, largest = [0, 0, 0, 0], 0, 0, 0
        for k, v in by_contig.get(locus[0], ()):
            t = touch(shape, locus, v)
            if t is None:
                continue
            read, top, is_silent = t
            pairs.append((i, k, read[0] + 256 * len(read) + 65536 * top + 262144 * int(is_silent), v[4]))
            coverage[k, int(is_silent)] += 1
            if is_silent:
                silent += 1
            else:
                zone[top] += 1
                total += v[4]
                largest = max(largest, v[4])
        rows[i] = (sum(min(255, zone[z]) * 256 ** z for z in range(4)), silent, min(MAX_U32, total), largest)
        by_zone.append(zone)
        cost.append(total)
        stats["with_disrupting"] += any(zone)
    out = np.zeros(len(pairs), dtype=va.VARIATION_PAIR_DTYPE)
    for k, row in enumerate(pairs):
        out[k] = row
    stats["pairs"] = len(pairs)
    stats["variants_covered"] = int((coverage.sum(axis=1) > 0).sum())
    return {"rows": rows, "pairs": out, "coverage": coverage, "stats": stats, "by_zone": by_zone, "cost": cost}


def keep(zone, cost, max_cost=0xFFFFFFFF, max_by_zone=(255, 255, 255, 255), require=()):
    """FILTER for one expected candidate given as (unclamped counts per zone or None, unclamped cost)."""
    if zone is None:
        return False
    if min(MAX_U32, cost) > max_cost or any(min(255, zone[z]) > max_by_zone[z] for z in range(4)):
        return False
    return not require or any(zone[z] for z in require)


# ---- the weight helper's cases ---------------------------------------------------------------------------------------------------
def weight_cases():
    """(af, the weight) for allele frequencies whose scaled value -log1p(-af) 2^20 lies at least 1e-3 from a rounding boundary
    (x.5), so that the last bits of a libm's log1p cannot move the integer; checked here, where the data is made."""
    import math
    out = []
    for af in (0.0, 1e-9, 1e-6, 2.5e-5, 1e-4, 0.001, 0.01, 0.05, 0.1, 0.25, 0.5, 0.75, 0.9, 0.99, 0.999999):
        x = -math.log1p(-af) * 2.0 ** 20
        frac = x - math.floor(x)
        assert abs(frac - 0.5) >= 1e-3, (af, x)
        out.append((af, int(math.floor(x + 0.5))))
    return out
