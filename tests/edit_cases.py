"""Shared helpers of test_edit.py (GPU) and test_edit_cpu.py: the definition of the base-editor windows (include/varscot_hip.h:
SHAPE, SITE, CLASS, MASK, FORWARD, TARGETS, HITS, ROW, PAIR, COVERAGE, FILTER) in plain Python on strings, and the small genome
of the tests.  The site is sliced out of the contig's text and reverse-complemented as text, letters are compared as letters, a
hit is `(contig, forward position) in set(targets)`, the pairs come out of a nested loop and are sorted.  Nothing here calls the
library and nothing here shares a mask or a bit trick with it: a row's two numbers are written from lists of window positions."""
import functools

import numpy as np

import varscot_amd as va
from helpers import random_seq, revcomp

CLASSES = ("defined", "invalid", "off_contig", "not_resident", "has_n")
UNDEF = 0xFFFFFFFF
SITE_LEN = 23
MAIN, SECOND = 3, 4  # the long contigs of the small genome


def offsets(contigs):
    """Global position of every contig's first base: the contigs lie one N apart (PackedGenome.from_sequences)."""
    off, at = [], 0
    for s in contigs:
        off.append(at)
        at += len(s) + 1
    return off


@functools.lru_cache(maxsize=None)
def small_genome(site_len=SITE_LEN):
    """About 1.3 kb: contigs of site_len - 1 (no site), site_len (one site per strand) and site_len + 1 bases, then one of 700
    with an N run, a run of 16 C (mask all ones under a 16-base window for C), a run of 16 A (the same for A, and a window
    without any C), a run of 16 G and one of 16 T (the same on '-'), and one of 500.  The one-N separators and the word
    boundaries at 32, 64, ... fall inside sites."""
    rng = np.random.default_rng([28, site_len])
    seqs = [random_seq(rng, n) for n in (site_len - 1, site_len, site_len + 1)]
    main = list(random_seq(rng, 700))
    main[90:97] = "NNNNNNN"
    for at, ch in ((150, "C"), (230, "A"), (310, "G"), (390, "T")):
        main[at:at + 16] = ch * 16
    seqs.append("".join(main))
    seqs.append(random_seq(rng, 500))
    return tuple(seqs)


def every_locus(contigs):
    """Every (contig, p, strand) with p in [0, len]: the last starts of a contig name a site that leaves it."""
    return [(c, p, s) for c, text in enumerate(contigs) for p in range(len(text) + 1) for s in (0, 1)]


def invalid_loci(contigs):
    n, main = len(contigs), MAIN
    length = len(contigs[main])
    return [(n, 0, 0), (0xFFFFFFFF, 0, 0), (0xFFFFFFFF, 0xFFFFFFFF, 1), (main, 10, 2), (main, 10, 0xFFFFFFFF), (main, length - 15, 0),
            (main, length - 15, 1), (main, 0xFFFFFFFF, 0), (main + 1, 0xFFFFFFFF, 1), (0, 7, 0), (main, 0xFFFFFFFF - 22, 0)]


def locus_array(loci):
    out = np.zeros(len(loci), dtype=va.LOCUS_DTYPE)
    if len(loci):
        a = np.asarray(loci, dtype=np.int64).reshape(-1, 3)
        out["contig"], out["pos"], out["strand"] = a[:, 0] & 0xFFFFFFFF, a[:, 1] & 0xFFFFFFFF, a[:, 2] & 0xFFFFFFFF
    return out


def loci_tuples(loci):
    return [(int(c), int(p), int(s)) for c, p, s in zip(loci["contig"], loci["pos"], loci["strand"])]


def target_sets(contigs):
    """The target sets of the tests, each a list of (contig, pos) in the caller's order (not sorted): none, every third position
    with the first and last base of every contig and one planted neighbour (150 and 151 of the long contig lie in its run of C:
    two adjacent targets in one window), every position, one target, the targets of one contig only."""
    every = [(c, p) for c, text in enumerate(contigs) for p in range(len(text))]
    third = [(c, p) for c, p in every if p % 3 == 0 or p == len(contigs[c]) - 1 or (c, p) == (MAIN, 151)]
    return {"none": None, "third": third[::-1], "every": every, "one": [(MAIN, 154)], "one_contig": [(c, p) for c, p in third if c == SECOND]}


def site_of(contigs, locus, site_len, resident=None):
    """(class, site text in read orientation or None) of locus (contig, pos, strand): SITE and CLASS in their order.  resident:
    None (the whole genome is) or the half-open range of global positions the genome object holds."""
    c, p, strand = locus
    if c >= len(contigs) or strand > 1 or p + site_len > len(contigs[c]):
        return "invalid", None
    if resident is not None:
        g = offsets(contigs)[c] + p
        if g < resident[0] or g + site_len > resident[1]:
            return "not_resident", None
    text = contigs[c][p:p + site_len].upper()
    if any(ch not in "ACGT" for ch in text):
        return "has_n", None
    return "defined", revcomp(text) if strand else text


def number(positions):
    """The number whose binary digits are 1 at `positions`."""
    return sum(2 ** j for j in set(positions))


def expected(contigs, loci, shape, targets=None, resident=None):
    """What an edit call gives for loci under shape = (site_len, win_start, win_len, base letter) and targets (a list of
    (contig, pos) in the caller's order, duplicates allowed; None: no targets): {"rows": uint32[n, 2], "pairs":
    EDIT_PAIR_DTYPE in ascending (candidate, target) with the target's index in the CALLER's list (the first of duplicates),
    "coverage": uint32[len(targets), 2], "stats", "editable": [window positions or None], "hit": [window positions or None]}."""
    site_len, start, length, base = shape
    index = {}
    for k, t in enumerate(targets or []):
        index.setdefault(tuple(t), k)
    members = set(index)
    rows = np.empty((len(loci), 2), dtype=np.uint32)
    stats = dict.fromkeys(CLASSES, 0)
    stats.update(with_hit=0, pairs=0, targets_covered=0)
    pairs, editable, hit = [], [], []
    for i, locus in enumerate(loci):
        cls, text = site_of(contigs, locus, site_len, resident)
        stats[cls] += 1
        if cls != "defined":
            rows[i] = (UNDEF, UNDEF)
            editable.append(None)
            hit.append(None)
            continue
        c, p, strand = locus
        window = text[start:start + length]
        at = [j for j in range(length) if window[j] == base]
        forward = {j: (p + site_len - 1 - (start + j) if strand else p + start + j) for j in at}
        hits = [j for j in at if (c, forward[j]) in members]
        rows[i] = (number(at), number(hits))
        editable.append(at)
        hit.append(hits)
        stats["with_hit"] += bool(hits)
        for j in hits:
            pairs.append((i, index[(c, forward[j])], number(at), j, len(at) - 1))
    pairs.sort()
    out = np.zeros(len(pairs), dtype=va.EDIT_PAIR_DTYPE)
    for k, (i, t, m, j, by) in enumerate(pairs):
        out[k] = (i, t, m, j + 256 * by)
    stats["pairs"] = len(pairs)
    coverage = None
    if targets is not None:
        coverage = np.zeros((len(targets), 2), dtype=np.uint32)
        coverage[:, 1] = UNDEF
        by_target = {}
        for _, t, _, _, by in pairs:
            by_target.setdefault(t, []).append(by)
        for k, t in enumerate(targets):
            mine = by_target.get(index[tuple(t)])
            if mine:
                coverage[k] = (len(mine), min(mine))
        stats["targets_covered"] = len({t for _, t, _, _, _ in pairs})
    return {"rows": rows, "pairs": out, "coverage": coverage, "stats": stats, "editable": editable, "hit": hit}


def keep(row, hits_needed, min_editable, max_editable):
    """FILTER for one expected row given as (editable positions or None, hit positions or None)."""
    at, hits = row
    if at is None:
        return False
    return min_editable <= len(at) <= max_editable and (not hits_needed or bool(hits))
