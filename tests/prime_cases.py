"""Shared helpers of test_prime.py (GPU) and test_prime_cpu.py: the definition of the prime-editing extensions
(include/varscot_hip.h: SHAPE, CONTEXT, PBS, EDITS, READ, RTT, FLAGS, ROW, PAIR, COVERAGE, FILTER, EXTENSION) in plain Python on
strings, and the small genome and edit sets of the tests.  The context is sliced out of the contig's text and
reverse-complemented as text, the edit is applied to the FORWARD text and the result reverse-complemented, the primer binding
site, the template's length, the flags and the extension are read off the letters, the pairs come out of a nested loop and are
sorted.  Nothing here calls the library and nothing here shares a mask or a bit trick with it."""
import functools

import numpy as np

import varscot_amd as va
from helpers import random_seq, revcomp

CLASSES = ("defined", "invalid", "off_contig", "not_resident", "has_n")
UNDEF = 0xFFFFFFFF
PAM, SEED, POLY_T, WEAK = 1, 2, 4, 8
CELL = 256  # global positions per cell of the library's occupancy bitmap

# a stability model in which G/C-rich primer binding sites reach the target early and A/T-rich ones never do
GC_MODEL = (0, (2, 3, 3, 2), tuple(1 if a + b in ("GC", "CG", "GG", "CC") else (-1 if a + b in ("TA", "AT") else 0) for a in "ACGT" for b in "ACGT"), 36)

# name -> PrimeShape arguments.  Between them: site_len 16, 20, 23 and 32; down 0 and the largest (C = 64); nick at 1 and at
# site_len; pbs_min == pbs_max and a range; a model that yields WEAK and not WEAK; AVOID_G_END on and off; a range of length 0.
SHAPES = {
    "pe2": dict(site_len=23, down=41, nick=17, pbs=(13, 13), rtt=(10, 34), min_homology=5, pam=(21, 2), seed=(17, 3), avoid_g_end=True),
    "model": dict(site_len=23, down=20, nick=17, pbs=(8, 15), rtt=(5, 20), min_homology=3, pam=(21, 2), seed=(17, 3), avoid_g_end=False,
                  stability=GC_MODEL),
    "short": dict(site_len=16, down=0, nick=8, pbs=(4, 8), rtt=(2, 8), min_homology=1, pam=(13, 3), seed=(8, 4), avoid_g_end=True),
    "long": dict(site_len=32, down=32, nick=32, pbs=(10, 17), rtt=(8, 32), min_homology=0, pam=(0, 0), seed=(24, 8), avoid_g_end=True,
                 stability=GC_MODEL),
    "first": dict(site_len=23, down=0, nick=1, pbs=(1, 1), rtt=(1, 22), min_homology=2, pam=(21, 2), seed=(0, 8), avoid_g_end=False),
    "deep": dict(site_len=20, down=44, nick=10, pbs=(5, 10), rtt=(20, 54), min_homology=5, pam=(17, 3), seed=(10, 0), avoid_g_end=True,
                 stability=(-5, (1, 2, 2, 1), (0,) * 16, 7)),
}


def shape_of(name):
    return va.PrimeShape(**SHAPES[name])


def context_len(name):
    return SHAPES[name]["site_len"] + SHAPES[name]["down"]


def offsets(contigs):
    """Global position of every contig's first base: the contigs lie one N apart (PackedGenome.from_sequences)."""
    off, at = [], 0
    for s in contigs:
        off.append(at)
        at += len(s) + 1
    return off


@functools.lru_cache(maxsize=None)
def small_genome(site_len, C):
    """Contigs of site_len - 1 (no site), C - 1, C and C + 1 bases (no context, one per strand, two), one of about 700 with an N
    run, runs of A (poly-T on either strand: runs of T as well), of G (AVOID_G_END; runs of C for '-') and one of about 500."""
    rng = np.random.default_rng([30, site_len, C])
    seqs = [random_seq(rng, n) for n in (site_len - 1, C - 1, C, C + 1)]
    main = list(random_seq(rng, 700))
    main[90:97] = "NNNNNNN"
    for at, ch, n in ((150, "A", 9), (200, "T", 9), (250, "G", 12), (300, "C", 12), (350, "A", 4), (380, "T", 4), (420, "G", 40), (480, "C", 40)):
        main[at:at + n] = ch * n
    seqs.append("".join(main))
    seqs.append(random_seq(rng, 500))
    return tuple(seqs)


MAIN, SECOND = 4, 5  # the long contigs of the small genome


def every_locus(contigs):
    """Every (contig, p, strand) with p in [0, len]: the last starts of a contig name a site that leaves it."""
    return [(c, p, s) for c, text in enumerate(contigs) for p in range(len(text) + 1) for s in (0, 1)]


def invalid_loci(contigs):
    n = len(contigs)
    length = len(contigs[MAIN])
    return [(n, 0, 0), (0xFFFFFFFF, 0, 0), (0xFFFFFFFF, 0xFFFFFFFF, 1), (MAIN, 10, 2), (MAIN, 10, 0xFFFFFFFF), (MAIN, length - 15, 0),
            (MAIN, length - 15, 1), (MAIN, 0xFFFFFFFF, 0), (SECOND, 0xFFFFFFFF, 1), (0, 7, 0), (MAIN, 0xFFFFFFFF - 22, 0)]


def locus_array(loci):
    out = np.zeros(len(loci), dtype=va.LOCUS_DTYPE)
    if len(loci):
        a = np.asarray(loci, dtype=np.int64).reshape(-1, 3)
        out["contig"], out["pos"], out["strand"] = a[:, 0] & 0xFFFFFFFF, a[:, 1] & 0xFFFFFFFF, a[:, 2] & 0xFFFFFFFF
    return out


def other_letter(ch, step=1):
    return "ACGT"[("ACGT".index(ch) + step) % 4] if ch in "ACGT" else "A"


def edit_sets(contigs):
    """The edit sets of the tests, each a list of (contig, pos, del_len, inserted letters) in the caller's order (not sorted), one
    edit per position: none (no list), empty (a list of none), an SNV at every position of the long contig; insertions of 1, 3
    and 16 letters, deletions of 1, 3 and 16 bases and a 2-for-3 replacement in turn over both long contigs, with an edit at
    pos 0, an insertion at pos = length and a deletion that ends at the end of every contig; and edits at the global positions
    around the edges of the bitmap's cells."""
    rng = np.random.default_rng(31)
    snv = [(MAIN, p, 1, other_letter(ch, 1 + p % 3)) for p, ch in enumerate(contigs[MAIN])]
    kinds = [(0, 1), (0, 3), (0, 16), (1, 0), (3, 0), (16, 0), (3, 2)]
    indel, taken = [], set()
    for c, text in enumerate(contigs):
        n = len(text)
        for e in ((c, 0, 1, "G"), (c, n, 0, "TAC"), (c, n - 3, 3, ""), (c, n - 1, 1, "C")):
            indel.append(e)
            taken.add((c, e[1]))
    k = 0
    for c in (MAIN, SECOND):
        for p in range(2, len(contigs[c]) - 20, 5):
            if (c, p) in taken:
                continue
            del_len, ins_len = kinds[k % len(kinds)]
            k += 1
            indel.append((c, p, del_len, random_seq(rng, ins_len) if ins_len else ""))
    off = offsets(contigs)
    cells = []
    for g in (CELL - 1, CELL, 2 * CELL - 1, 2 * CELL, 3 * CELL - 1, 3 * CELL, 4 * CELL):
        for c, text in enumerate(contigs):
            if off[c] <= g < off[c] + len(text):
                p = g - off[c]
                cells.append((c, p, 1, other_letter(text[p])) if g % 2 else (c, p, 0, "GA"))
    order = rng.permutation(len(indel))
    return {"none": None, "empty": [], "snv": snv[::-1], "indel": [indel[i] for i in order], "cells": cells}


def context_of(contigs, locus, shape, resident=None):
    """(class, context in read orientation or None, F0) of locus (contig, pos, strand): CONTEXT and CLASS in their order.
    resident: None (the whole genome is) or the half-open range of global positions the genome object holds."""
    c, p, strand = locus
    site_len, down = shape.site_len, shape.down
    if c >= len(contigs) or strand > 1 or p + site_len > len(contigs[c]):
        return "invalid", None, None
    lo, hi = (p - down, p + site_len) if strand else (p, p + site_len + down)
    if lo < 0 or hi > len(contigs[c]):
        return "off_contig", None, None
    if resident is not None:
        g = offsets(contigs)[c] + lo
        if g < resident[0] or g + (hi - lo) > resident[1]:
            return "not_resident", None, None
    text = contigs[c][lo:hi].upper()
    if any(ch not in "ACGT" for ch in text):
        return "has_n", None, None
    return "defined", revcomp(text) if strand else text, lo


def pbs_of(R, shape):
    """(pbs_len, pbs_gc, weak) of a context: PBS."""
    nick = shape.nick
    chosen = None
    for L in range(shape.pbs_min, shape.pbs_max + 1):
        s = shape.init + sum(shape.mono["ACGT".index(R[j])] for j in range(nick - L, nick))
        s += sum(shape.di[4 * "ACGT".index(R[j]) + "ACGT".index(R[j + 1])] for j in range(nick - L, nick - 1))
        if s >= shape.target:
            chosen = L
            break
    weak = chosen is None
    L = shape.pbs_max if weak else chosen
    return L, sum(ch in "GC" for ch in R[nick - L:nick]), weak


def pair_of(R, F0, strand, shape, edit, pbs_len, weak):
    """READ, RTT, FLAGS and EXTENSION of a context with one edit (contig, pos, del_len, ins) on its contig: a dict (t, d, h, flags,
    ext_gc, extension, lengthened), or the reason there is no pair: "reach", "rtt_max", "g_end" or "end"."""
    C, nick = len(R), shape.nick
    _, pos, del_len, ins = edit
    f = pos - F0
    if f < 0 or f + del_len > C:
        return "reach"
    forward = revcomp(R) if strand else R
    edited_forward = forward[:f] + ins + forward[f + del_len:]
    E = revcomp(edited_forward) if strand else edited_forward
    e0 = C - f - del_len if strand else f
    if e0 < nick:
        return "reach"
    assert E == R[:e0] + (revcomp(ins) if strand else ins) + R[e0 + del_len:]
    d = e0 - nick
    t0 = max(shape.rtt_min, d + len(ins) + shape.min_homology)
    t = t0
    if shape.flags & 1:
        while nick + t - 1 < len(E) and E[nick + t - 1] == "G":
            t += 1
    if t0 > shape.rtt_max:
        return "rtt_max"
    if t > shape.rtt_max:
        return "g_end"
    if nick + t > len(E):
        return "end"
    flags = 0
    if any(q >= len(E) or E[q] != R[q] for q in range(shape.pam_start, shape.pam_start + shape.pam_len)):
        flags |= PAM
    if any(q >= len(E) or E[q] != R[q] for q in range(shape.seed_start, shape.seed_start + shape.seed_len)):
        flags |= SEED
    body = E[nick - pbs_len:nick + t]
    if "AAAA" in body:
        flags |= POLY_T
    if weak:
        flags |= WEAK
    return {"t": t, "d": d, "h": t - d - len(ins), "flags": flags, "ext_gc": sum(ch in "GC" for ch in body), "extension": revcomp(body),
            "lengthened": t > t0}


def expected(contigs, loci, shape, edits=None, resident=None):
    """What a prime call gives for loci under a PrimeShape and edits (a list in the caller's order; None: no edits): {"rows":
    uint32[n, 2], "pairs": PRIME_PAIR_DTYPE in ascending (candidate, edit) with the edit's index in the CALLER's list,
    "coverage": uint32[len(edits), 2], "stats", "extension": the texts in the pairs' order, "detail": the pairs' dicts with
    the candidate's strand, "refused": {strand: {reason: count}}, "weak": [bool or None per candidate]}."""
    C = shape.site_len + shape.down
    at = {}
    for k, e in enumerate(edits or []):
        assert (e[0], e[1]) not in at
        at[(e[0], e[1])] = k
    rows = np.empty((len(loci), 2), dtype=np.uint32)
    stats = dict.fromkeys(CLASSES, 0)
    stats.update(with_pair=0, weak=0, pairs=0, edits_covered=0, pairs_by_flag=[0, 0, 0, 0])
    found, weak_of = [], []
    refused = {0: {}, 1: {}}
    for i, locus in enumerate(loci):
        cls, R, F0 = context_of(contigs, locus, shape, resident)
        stats[cls] += 1
        if cls != "defined":
            rows[i] = (UNDEF, UNDEF)
            weak_of.append(None)
            continue
        c, _, strand = locus
        pbs_len, pbs_gc, weak = pbs_of(R, shape)
        weak_of.append(weak)
        stats["weak"] += weak
        mine = 0
        for pos in range(F0, F0 + C + 1):
            k = at.get((c, pos))
            if k is None:
                continue
            got = pair_of(R, F0, strand, shape, edits[k], pbs_len, weak)
            if isinstance(got, str):
                refused[strand][got] = refused[strand].get(got, 0) + 1
                continue
            got.update(strand=strand, pbs_len=pbs_len)
            found.append((i, k, got))
            mine += 1
        rows[i] = (pbs_len + 256 * pbs_gc + 65536 * weak, mine)
        stats["with_pair"] += bool(mine)
    found.sort(key=lambda x: (x[0], x[1]))
    out = np.zeros(len(found), dtype=va.PRIME_PAIR_DTYPE)
    for n, (i, k, g) in enumerate(found):
        out[n] = (i, k, g["t"] + 256 * g["d"] + 65536 * g["h"] + 2 ** 24 * g["flags"], g["pbs_len"] + g["t"] + 256 * g["ext_gc"] + 65536 * g["pbs_len"])
        for b in range(4):
            stats["pairs_by_flag"][b] += g["flags"] >> b & 1
    stats["pairs"] = len(found)
    coverage = None
    if edits is not None:
        coverage = np.zeros((len(edits), 2), dtype=np.uint32)
        coverage[:, 1] = UNDEF
        for _, k, g in found:
            coverage[k, 0] += 1
            coverage[k, 1] = min(int(coverage[k, 1]), g["t"])
        stats["edits_covered"] = int((coverage[:, 0] > 0).sum())
    return {"rows": rows, "pairs": out, "coverage": coverage, "stats": stats, "extension": [g["extension"] for _, _, g in found],
            "detail": [g for _, _, g in found], "refused": refused, "weak": weak_of}


def keep(row, have_edits, allow_weak):
    """FILTER for one expected row (pbs, n_pairs)."""
    if int(row[0]) == UNDEF:
        return False
    return (not have_edits or int(row[1]) >= 1) and (allow_weak or not (int(row[0]) >> 16 & 1))
