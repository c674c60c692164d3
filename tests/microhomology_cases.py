"""Shared helpers of test_microhomology.py (GPU) and test_microhomology_cpu.py: the definition of the microhomology score
(include/varscot_hip.h: SHAPE, CONTEXT, CLASS, ROWS, SCORE, OUTPUT, FILTER) in plain Python as the ROW LIST - the triple loop of
the published script, the drop of contained rows, the weights from math.exp - the seeded context families and the small genome
of the tests.  Nothing here forms a mask and nothing here calls the library: that the library's mask form gives what the row
list gives is what the tests test."""
import functools
import math

import numpy as np

import varscot_amd as va
from helpers import random_seq, revcomp

FLANKS = (8, 9, 16, 30, 32)
CLASSES = ("defined", "invalid", "off_contig", "not_resident", "has_n")
UNDEF = 0xFFFFFFFF
SITE_LEN = 23


def weight(d):
    """T[d]: the published length factor round(1 / e^(d / 20), 3) as a whole number of thousandths."""
    return int(round(round(math.exp(-d / 20.0), 3) * 1000.0))


def rows(s, F):
    """The kept rows (i, j, k) of context s (2 F letters, ACGT): ROWS, literally."""
    W, left = 2 * F, F
    assert len(s) == W
    by_d = {}
    for k in reversed(range(2, left)):
        for j in range(left, W - k + 1):
            for i in range(0, left - k + 1):
                if s[i:i + k] == s[j:j + k]:
                    by_d.setdefault(j - i, []).append((i, j, k))
    kept = []
    for d in sorted(by_d):
        group = by_d[d]  # longest first: a container is met early
        for r in group:
            if not any(o is not r and o[0] <= r[0] and r[0] + r[2] <= o[0] + o[2] for o in group):
                kept.append(r)
    return kept


def score(s, F):
    """(sum, oof) of context s: SCORE and OUTPUT over the kept rows, in integers."""
    total = oof = 0
    for i, j, k in rows(s.upper(), F):
        d = j - i
        v = weight(d) * (k + sum(ch in "GC" for ch in s[i:i + k].upper()))
        total += v
        if d % 3:
            oof += v
    return total, oof


def published_float(s, F):
    """The published script's sum: 100 * length_factor * (AT + 2 GC) per kept row, added as floats."""
    x = 0.0
    for i, j, k in rows(s.upper(), F):
        gc = sum(ch in "GC" for ch in s[i:i + k].upper())
        x += 100.0 * round(1.0 / math.exp((j - i) / 20.0), 3) * ((k - gc) + 2 * gc)
    return x


def keep(pair, min_sum, permille):
    """FILTER for a (sum, oof) pair; Python integers do not overflow."""
    total, oof = int(pair[0]), int(pair[1])
    if total == UNDEF or total < min_sum:
        return False
    if total == 0:
        return permille == 0
    return 1000 * oof >= permille * total


def two_thirds(F=30):
    """A context whose out-of-frame share is exactly 2 : 3 (F = 30): the left half is A and the right half C but for two planted
    words over {T, G}: GT at deletion length 42 (in frame, 122 * 3) and GG at 34 (out of frame, 183 * 4 = 2 * 366)."""
    assert F == 30
    left, right = ["A"] * F, ["C"] * F
    left[4:6] = "GT"
    right[46 - F:48 - F] = "GT"
    left[20:22] = "GG"
    right[54 - F:56 - F] = "GG"
    return "".join(left + right)


def one_row(F, d):
    """A context with exactly one row: the left half is A and the right half C but for GT at deletion length d."""
    left, right = ["A"] * F, ["C"] * F
    left[2:4] = "GT"
    right[2 + d - F:4 + d - F] = "GT"
    return "".join(left + right)


# ---- context families ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def contexts(F):
    """[(family, text)] for flank F, seeded."""
    rng = np.random.default_rng([26, F])
    W = 2 * F
    out = []
    for _ in range(24):
        out.append(("random", random_seq(rng, W)))
    for _ in range(6):
        half = random_seq(rng, F)
        out.append(("halves", half + half))  # the d = F quirk
    for at in [0, F - 1] + [int(v) for v in rng.integers(0, F, size=8)]:  # (a run of F - 1 needs the odd base at an end)
        half = random_seq(rng, F)
        other = "ACGT"[("ACGT".index(half[at]) + 1 + int(rng.integers(0, 3))) % 4]
        out.append(("halves_but_one", half + half[:at] + other + half[at + 1:]))  # runs of F - 1 and shorter at d = F
    out.append(("period", "A" * W))
    out.append(("period", "G" * W))  # the largest sum there is
    for period in (2, 3, 4):
        for _ in range(2):
            unit = random_seq(rng, period)
            out.append(("period", (unit * W)[:W]))
    for pair in ("AT", "GC", "AG", "CT"):
        for _ in range(3):
            out.append(("two_letters", "".join(pair[int(b)] for b in rng.integers(0, 2, size=W))))
    out.append(("none", "A" * F + "C" * F))
    out.append(("none", "AC" * (F // 2) + "A" * (F % 2) + "GT" * (F // 2) + "G" * (F % 2)))
    out.append(("none", ("ACAAC" * F)[:F] + ("GTTGG" * F)[:F]))
    for d in (F - 1, F, F + 1):
        out.append(("one_row", one_row(F, d)))
    if F == 30:
        out.append(("two_thirds", two_thirds()))
    return tuple(out)


# ---- the small genome ------------------------------------------------------------------------------------------------------------
def offsets(contigs):
    """Global position of every contig's first base: the contigs lie one N apart (PackedGenome.from_sequences)."""
    off, at = [], 0
    for s in contigs:
        off.append(at)
        at += len(s) + 1
    return off


@functools.lru_cache(maxsize=None)
def small_genome(F):
    """600 to 900 bases: contigs of F - 1, F, 2 F - 1, 2 F and 2 F + 1 bases, then a long one with an N run, a tandem
    duplication of exactly F bases, one of F + 3 bases, a poly-A / poly-C junction (no row at all), three contexts with one row
    each (of which one is in frame) and the 2 : 3 context (F = 30), then one of 90.  The one-N separators and the word
    boundaries at 32, 64, ... fall inside contexts."""
    rng = np.random.default_rng([26, 1, F])
    seqs = [random_seq(rng, n) for n in (F - 1, F, 2 * F - 1, 2 * F, 2 * F + 1)]
    x, y = random_seq(rng, F), random_seq(rng, F + 3)
    main = random_seq(rng, 20) + x + x + random_seq(rng, 15) + "NNN" + random_seq(rng, 25) + y + y + random_seq(rng, 9)
    main += "A" * 32 + "C" * 32 + random_seq(rng, 7)
    for d in (F - 1, F, F + 1):
        main += one_row(F, d) + random_seq(rng, 3)
    if F == 30:
        main += two_thirds() + random_seq(rng, 5)
    seqs.append(main)
    seqs.append(random_seq(rng, 90))
    return tuple(seqs)


def every_locus(contigs, site_len=SITE_LEN):
    """Every (contig, p, strand) with p in [0, len]: the last site_len starts of a contig name a site that leaves it."""
    return [(c, p, s) for c, text in enumerate(contigs) for p in range(len(text) + 1) for s in (0, 1)]


def locus_array(loci):
    out = np.zeros(len(loci), dtype=va.LOCUS_DTYPE)
    if len(loci):
        a = np.asarray(loci, dtype=np.int64).reshape(-1, 3)
        out["contig"], out["pos"], out["strand"] = a[:, 0] & 0xFFFFFFFF, a[:, 1] & 0xFFFFFFFF, a[:, 2] & 0xFFFFFFFF
    return out


def classify(contigs, locus, shape, resident=None):
    """(class, context text or None) of locus (contig, pos, strand) under shape (site_len, cut, F): CONTEXT and CLASS in their
    order.  resident: None (the whole genome is) or the half-open range of global positions the genome object holds."""
    site_len, cut, F = shape
    c, p, strand = locus
    if c >= len(contigs) or strand > 1 or p + site_len > len(contigs[c]):
        return "invalid", None
    start = p + site_len - cut - F if strand else p + cut - F
    if start < 0 or start + 2 * F > len(contigs[c]):
        return "off_contig", None
    if resident is not None:
        g = offsets(contigs)[c] + start
        if g < resident[0] or g + 2 * F > resident[1]:
            return "not_resident", None
    text = contigs[c][start:start + 2 * F].upper()
    if any(ch not in "ACGT" for ch in text):
        return "has_n", None
    return "defined", revcomp(text) if strand else text


_memo = {}


def expected(contigs, loci, shape, resident=None):
    """(uint32[n, 2] pairs, stats dict, [context or None]) of loci under shape."""
    out = np.empty((len(loci), 2), dtype=np.uint32)
    stats = dict.fromkeys(CLASSES, 0)
    texts = []
    for i, locus in enumerate(loci):
        cls, text = classify(contigs, locus, shape, resident)
        stats[cls] += 1
        texts.append(text)
        if cls == "defined":
            key = (text, shape[2])
            if key not in _memo:
                _memo[key] = score(text, shape[2])
            out[i] = _memo[key]
        else:
            out[i] = (UNDEF, UNDEF)
    return out, stats, texts
