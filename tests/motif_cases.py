"""Restriction sites and IUPAC motifs (include/varscot_hip.h "restriction sites and IUPAC motifs") restated on STRINGS, with
the cases the tests walk.  The letter sets are a dictionary, OCC is slicing and all(), the reverse complement is a dictionary
and [::-1].  Nothing here looks at a bit plane.

A motif has at most 16 letters and a genomic context at least 16, so "a motif longer than C" cannot be built; the motif of 16
letters on the context of 16 (one start) and on constructs of 12 .. 15 letters (no start, not refused) stand in for it."""
import collections
import functools

import numpy as np

import varscot_amd as va
from helpers import random_seq, revcomp

UNDEF = 0xFFFFFFFFFFFFFFFF
CLASSES = ("defined", "invalid", "off_contig", "not_resident", "has_n")
SETS = {"A": "A", "C": "C", "G": "G", "T": "T", "U": "T", "R": "AG", "Y": "CT", "S": "CG", "W": "AT", "K": "GT", "M": "AC", "B": "CGT",
        "D": "AGT", "H": "ACT", "V": "ACG", "N": "ACGT"}
IUPAC_COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "U": "A", "R": "Y", "Y": "R", "S": "S", "W": "W", "K": "M", "M": "K", "B": "V", "D": "H",
              "H": "D", "V": "B", "N": "N"}

Shape = collections.namedtuple("Shape", "up site_len down proto_start proto_len cut_start cut_len")
Limits = collections.namedtuple("Limits", "forbid_construct forbid_context require_cut cut_only")

SHAPE_OF = {
    "SpCas9": Shape(16, 23, 16, 0, 20, 16, 2),
    "Cas12a": Shape(16, 27, 16, 4, 23, 21, 6),
    "c64": Shape(16, 32, 16, 0, 32, 8, 16),       # C = 64, n = 32, cut_len 16
    "bare": Shape(0, 23, 0, 0, 20, 16, 2),        # up = down = 0
    "n12_site16": Shape(3, 16, 5, 2, 12, 0, 1),   # n = 12 on a 16-site, the zone at the site's first position, cut_len 1
    "zone_last": Shape(0, 16, 0, 0, 16, 15, 1),   # C = 16, the zone at the site's last position
}
# (left, right) letters per flank case: none, 16 on either side, the usual few
FLANKS = {"none": ("", ""), "left16": ("TTGTGGAAAGGACGAA", ""), "right16": ("", "GTTTTAGAGCTAGAAA"), "both16": ("TTGTGGAAAGGACGAA", "GTTTTAGAGCTAGAAA"),
          "short": ("cacCG", "GUUu")}

P = "CGTCTC"  # BsmBI: no palindrome, none of its letters pairs up in an all-A background


def va_shape(s):
    return va.MotifShape(s.site_len, (s.proto_start, s.proto_len), (s.cut_start, s.cut_len), s.up, s.down)


def context_len(s):
    return s.up + s.site_len + s.down


def iupac_revcomp(text):
    return "".join(IUPAC_COMP[c] for c in text.upper())[::-1]


def patterns(text, both):
    """PATTERNS(m)"""
    text = text.upper()
    return {text, iupac_revcomp(text)} if both else {text}


def occ(t, pat):
    """OCC(t, P)"""
    return [q for q in range(len(t) - len(pat) + 1) if all(t[q + k] in SETS[pat[k]] for k in range(len(pat)))]


def entry(e):
    return e[0], e[1], (bool(e[2]) if len(e) > 2 else True)


def row(x, left, right, entries, shape):
    """ROW of the context text x (read orientation, A C G T U in any case) under the motif entries."""
    x = x.upper().replace("U", "T")
    left, right = left.upper().replace("U", "T"), right.upper().replace("U", "T")
    at = shape.up + shape.proto_start
    y = left + x[at:at + shape.proto_len] + right
    z0 = shape.up + shape.cut_start
    z1 = z0 + shape.cut_len
    construct = cut = elsewhere = 0
    for m, e in enumerate(entries):
        _, text, both = entry(e)
        for pat in patterns(text, both):
            if occ(y, pat):
                construct |= 1 << m
            for q in occ(x, pat):
                if q < z1 and q + len(pat) > z0:
                    cut |= 1 << m
                else:
                    elsewhere |= 1 << m
    return construct, cut, elsewhere


def keep(r, lim):
    """FILTER on a row (None: undefined)"""
    if r is None or tuple(r) == (UNDEF,) * 3:
        return False
    construct, cut, elsewhere = (int(v) for v in r)
    x = cut & ~elsewhere if lim.cut_only else cut
    return (construct & lim.forbid_construct == 0 and (cut | elsewhere) & lim.forbid_context == 0
            and (lim.require_cut == 0 or x & lim.require_cut != 0))


# the filter's truth table: every combination of the three bits of one motif against each limit alone and together
def truth_table():
    out = []
    for bits in range(8):
        r = (bits & 1, (bits >> 1) & 1, (bits >> 2) & 1)
        for lim in (Limits(1, 0, 0, False), Limits(0, 1, 0, False), Limits(0, 0, 1, False), Limits(0, 0, 1, True), Limits(1, 1, 1, True),
                    Limits(0, 0, 0, False)):
            construct, cut, elsewhere = r
            want = not (lim.forbid_construct and construct) and not (lim.forbid_context and (cut or elsewhere))
            if lim.require_cut:
                want = want and bool(cut and not (lim.cut_only and elsewhere))
            out.append((r, lim, want))
    return out


# ---- motif sets -----------------------------------------------------------------------------------------------------------------
CLONING = [("BsmBI", "CGTCTC"), ("BbsI", "GAAGAC"), ("BsaI", "GGTCTC")]
IUPAC = [("acgu", "acgu", False), ("RY", "RYRY"), ("SW", "SWS", False), ("KM", "KMK"), ("BD", "BDB", False), ("HV", "HVH"), ("N", "GNNNC"),
         ("EcoRI", "GAATTC"), ("EcoRI1", "GAATTC", False), ("two", "CG"), ("fwd", P, False), ("rc", iupac_revcomp(P), False), ("sixteen", "ACGTNNRYACGTACGT")]


@functools.lru_cache(maxsize=None)
def full_set():
    """63 motifs: lengths 2 and 16, every IUPAC letter, and words of 4 .. 8 letters."""
    rng = np.random.default_rng(63)
    out = list(IUPAC)
    while len(out) < 62:
        out.append(("w%d" % len(out), random_seq(rng, int(rng.integers(4, 9))), bool(len(out) % 2)))
    out.append(("last", P, False))  # bit 62
    return tuple(out)


def never_set():
    """63 motifs of which only the last can occur in a background of A with P planted: the others hold GG."""
    out = [("n%d" % m, "GG" + "".join("GT"[(m >> b) & 1] for b in range(6)), False) for m in range(62)]
    return tuple(out) + (("last", P, False),)


MOTIF_SETS = {"one": (("BsmBI", P),), "cloning": tuple(CLONING), "iupac": tuple(IUPAC)}


# ---- planted families -------------------------------------------------------------------------------------------------------------
def put(text, q, word):
    assert 0 <= q and q + len(word) <= len(text), (q, word, len(text))
    return text[:q] + word + text[q + len(word):]


def planted(name, flanks):
    """[(family, x, left, right, entries, holds)]: contexts of shape `name` in a background of A under the flank case; holds(row)
    says what the family is there to show and is asserted on the string row too."""
    s = SHAPE_OF[name]
    C, n = context_len(s), s.proto_len
    left, right = (t.upper().replace("U", "T") for t in FLANKS[flanks])
    a, b = len(left), len(right)
    at = s.up + s.proto_start
    z0 = s.up + s.cut_start
    z1 = z0 + s.cut_len
    L = len(P)
    one = (("P", P, False),)
    blank = "A" * C
    out = []

    def add(family, x, holds, entries=one, lf=left, rf=right):
        out.append((family, x, lf, rf, entries, holds))

    add("x_q0", put(blank, 0, P), lambda r: (r[1] | r[2]) & 1)
    add("x_qlast", put(blank, C - L, P), lambda r: (r[1] | r[2]) & 1)
    # the construct's first and last start: in the flank where there is one, else in the spacer
    if a >= L:
        add("y_q0", blank, lambda r: r[0] & 1 and not (r[1] | r[2]), lf=P + "A" * (a - L))
    elif a == 0:
        add("y_q0", put(blank, at, P), lambda r: r[0] & 1)
    if b >= L:
        add("y_qlast", blank, lambda r: r[0] & 1 and not (r[1] | r[2]), rf="A" * (b - L) + P)
    elif b == 0:
        add("y_qlast", put(blank, at + n - L, P), lambda r: r[0] & 1)
    if a >= 3:
        add("left_junction", put(blank, at, P[3:]), lambda r: r[0] & 1 and not (r[1] | r[2]), lf="A" * (a - 3) + P[:3])
    if b >= 3:
        add("right_junction", put(blank, at + n - 3, P[:3]), lambda r: r[0] & 1 and not (r[1] | r[2]), rf=P[3:] + "A" * (b - 3))
    add("spacer_alone", put(blank, at + 3, P), lambda r: r[0] & 1 and (r[1] | r[2]) & 1)
    if z0 >= L:
        add("ends_at_z0", put(blank, z0 - L, P), lambda r: r[2] & 1 and not r[1] & 1)
    if z0 >= L - 1:
        add("reaches_z0", put(blank, z0 - L + 1, P), lambda r: r[1] & 1 and not r[2] & 1)
    if z1 + L <= C:
        add("starts_at_z1", put(blank, z1, P), lambda r: r[2] & 1 and not r[1] & 1)
    if z1 - 1 + L <= C:
        add("starts_in_z1", put(blank, z1 - 1, P), lambda r: r[1] & 1 and not r[2] & 1)
    if z0 >= L - 1 and z1 + 1 + L <= C:
        add("cut_and_elsewhere", put(put(blank, z0 - L + 1, P), C - L, P), lambda r: r[1] & 1 and r[2] & 1)  # cut-only clear
    add("bit62", put(blank, at + 2, P), lambda r: r[0] == 1 << 62 and (r[1] | r[2]) == 1 << 62, entries=never_set())
    # the reverse complement alone: seen with the flag, not without it
    rc = iupac_revcomp(P)
    add("rc_with_flag", put(blank, at + 1, rc), lambda r: r[0] & 1 and (r[1] | r[2]) & 1, entries=(("P", P, True),))
    add("rc_without_flag", put(blank, at + 1, rc), lambda r: r == (0, 0, 0))
    # a palindrome has one pattern: the flag changes nothing
    eco = put(blank, at + 4, "GAATTC")
    add("palindrome", eco, lambda r: r[0] == 3 and (r[1] | r[2]) == 3, entries=(("E2", "GAATTC", True), ("E1", "GAATTC", False)))
    # the motif of 16 letters: no start in a construct of fewer letters (not refused), one start in a context of 16
    long16 = "ACGTCCGGACGTACGT"
    if C >= 16:
        add("sixteen", put(blank, C - 16, long16), lambda r: (r[1] | r[2]) & 1 and bool(r[0] & 1) == (at <= C - 16 and C <= at + n),
            entries=(("long", long16, False),), lf="", rf="")
    return out


# ---- the small genome ------------------------------------------------------------------------------------------------------------
def offsets(contigs):
    """Global position of every contig's first base: the contigs lie one N apart (PackedGenome.from_sequences)."""
    off, at = [], 0
    for s in contigs:
        off.append(at)
        at += len(s) + 1
    return off


@functools.lru_cache(maxsize=None)
def small_genome(name):
    """A few hundred bases: contigs of site_len - 1, site_len and site_len + 1 bases, then a long one that carries the planted
    contexts of shape `name` (flank case both16) alternately on '+' and '-', with an N run between two of them, then one of 70
    random bases.  The one-N separators and the word boundaries at 32, 64, ... fall inside contexts."""
    s = SHAPE_OF[name]
    rng = np.random.default_rng([36, 1, len(name)])
    L = s.site_len
    seqs = [random_seq(rng, n) for n in (L - 1, L, L + 1)]
    main = random_seq(rng, 5)
    for i, (_, x, _, _, _, _) in enumerate(planted(name, "both16")[:14]):
        main += (revcomp(x) if i % 2 else x) + random_seq(rng, int(rng.integers(0, 3)))
        if i == 4:
            main += "NN"
    seqs.append(main + random_seq(rng, 40))
    seqs.append(random_seq(rng, 70))
    return tuple(seqs)


def every_locus(contigs):
    """Every (contig, p, strand) with p in [0, len]: the last site_len starts of a contig name a site that leaves it."""
    return [(c, p, s) for c, text in enumerate(contigs) for p in range(len(text) + 1) for s in (0, 1)]


def locus_array(loci):
    out = np.zeros(len(loci), dtype=va.LOCUS_DTYPE)
    if len(loci):
        a = np.asarray(loci, dtype=np.int64).reshape(-1, 3)
        out["contig"], out["pos"], out["strand"] = a[:, 0] & 0xFFFFFFFF, a[:, 1] & 0xFFFFFFFF, a[:, 2] & 0xFFFFFFFF
    return out


def classify(contigs, locus, shape, resident=None):
    """(class, context text or None) of locus (contig, pos, strand): GENOMIC and CLASS in their order.  resident: None (the whole
    genome is) or the half-open range of global positions the genome object holds."""
    c, p, strand = locus
    if c >= len(contigs) or strand > 1 or p + shape.site_len > len(contigs[c]):
        return "invalid", None
    before, behind = (shape.down, shape.up) if strand else (shape.up, shape.down)
    if p < before or p + shape.site_len + behind > len(contigs[c]):
        return "off_contig", None
    first = p - before
    if resident is not None:
        g = offsets(contigs)[c] + first
        if g < resident[0] or g + context_len(shape) > resident[1]:
            return "not_resident", None
    text = contigs[c][first:first + context_len(shape)].upper()
    if any(ch not in "ACGT" for ch in text):
        return "has_n", None
    return "defined", revcomp(text) if strand else text


def expected(contigs, loci, shape, left, right, entries, resident=None):
    """(uint64[n, 3] rows, stats dict, [context or None]) of loci under shape, flanks and motifs."""
    out = np.empty((len(loci), 3), dtype=np.uint64)
    stats = dict.fromkeys(CLASSES, 0)
    texts = []
    memo = {}
    for i, locus in enumerate(loci):
        cls, text = classify(contigs, locus, shape, resident)
        stats[cls] += 1
        texts.append(text)
        if cls == "defined" and text not in memo:
            memo[text] = row(text, left, right, entries, shape)
        out[i] = memo[text] if cls == "defined" else (UNDEF,) * 3
    return out, stats, texts


def totals_of(rows, n_motifs):
    """TOTALS out of rows: uint64[M, 3]"""
    out = np.zeros((n_motifs, 3), dtype=np.uint64)
    for construct, cut, elsewhere in rows:
        if (int(construct), int(cut), int(elsewhere)) == (UNDEF,) * 3:
            continue
        for m in range(n_motifs):
            out[m, 0] += (int(construct) >> m) & 1
            out[m, 1] += (int(cut) >> m) & 1
            out[m, 2] += (int(cut) & ~int(elsewhere)) >> m & 1
    return out
