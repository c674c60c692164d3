"""The per-target pick with spacing (include/varscot_hip.h "SHAPE / CANDIDATE / CUT COORDINATE / ELIGIBLE / BEFORE / CONFLICT /
PICK / OUTPUT / TARGETS") restated in plain Python, with an NGG enumerator and a labeller of its own, and the fixtures of
tests/test_pick_cpu.py and tests/test_pick.py.  Nothing here calls the library.

The restatement is the PICK loop over Python lists: the eligible candidates of a target sorted by (-key, index), walked once,
each tested against the picks so far."""
import functools

import numpy as np

NONE = 0xFFFFFFFF
WINDOW = 23
CLASSES = ("eligible", "invalid", "no_target", "bad_target", "below_min_key")
KS = (1, 4, 32)
SPACINGS = (0, 1, 20, 1000)
COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}


# ---- the definition -------------------------------------------------------------------------------------------------------
def cut_coordinate(pos, strand, site_len, cut):
    return pos + cut if strand == 0 else pos + site_len - cut


def classify(lens, locus, target, key, n_targets, site_len, min_key):
    c, p, s = locus
    if not (0 <= c < len(lens)) or s not in (0, 1) or p < 0 or p + site_len > lens[c]:
        return "invalid"
    if target == NONE:
        return "no_target"
    if target >= n_targets:
        return "bad_target"
    if key < min_key:
        return "below_min_key"
    return "eligible"


def pick(lens, loci, target, key, n_targets, k, spacing, site_len=WINDOW, cut=17, min_key=0):
    """loci: (contig, pos, strand) tuples; target, key: one int each.  Returns (picks [n_targets][k], counts [n_targets],
    rank [n], stats)."""
    stats = dict.fromkeys(CLASSES, 0)
    per = [[] for _ in range(n_targets)]
    for i, (l, t, q) in enumerate(zip(loci, target, key)):
        cls = classify(lens, l, t, q, n_targets, site_len, min_key)
        stats[cls] += 1
        if cls == "eligible":
            per[t].append(i)
    picks = [[NONE] * k for _ in range(n_targets)]
    counts = [0] * n_targets
    rank = [NONE] * len(loci)
    short = 0
    for t, members in enumerate(per):
        picked = []
        for i in sorted(members, key=lambda i: (-key[i], i)):
            if len(picked) == k:
                break
            x = cut_coordinate(loci[i][1], loci[i][2], site_len, cut)
            if any(loci[j][0] == loci[i][0] and abs(cut_coordinate(loci[j][1], loci[j][2], site_len, cut) - x) < spacing for j in picked):
                continue
            rank[i] = len(picked)
            picked.append(i)
        picks[t][:len(picked)] = picked
        counts[t] = len(picked)
        short += len(picked) < k and len(members) > len(picked)
    stats.update(targets_picked=sum(1 for c in counts if c), targets_short=short, picks=sum(counts))
    return picks, counts, rank, stats


def as_arrays(result):
    picks, counts, rank, stats = result
    return (np.array(picks, dtype=np.uint32).reshape(len(counts), -1), np.array(counts, dtype=np.uint32), np.array(rank, dtype=np.uint32),
            stats)


# ---- candidates and labels ------------------------------------------------------------------------------------------------
def revcomp(s):
    return "".join(COMP[c] for c in reversed(s))


def enumerate_ngg(contigs):
    """(contig, pos, strand) of every N-free 23-base window that ends in GG ('+') or starts with CC ('-'), in ascending
    (contig, pos), '+' before '-'."""
    out = []
    for c, text in enumerate(contigs):
        for p in range(len(text) - WINDOW + 1):
            w = text[p:p + WINDOW]
            if "N" in w:
                continue
            if w.endswith("GG"):
                out.append((c, p, 0))
            if w.startswith("CC"):
                out.append((c, p, 1))
    return out


def enumerate_pattern(contigs, pattern):
    """The same for an IUPAC pattern of any length: '+' where the window matches it, '-' where its reverse complement does."""
    iupac = {"A": "A", "C": "C", "G": "G", "T": "T", "R": "AG", "Y": "CT", "V": "ACG", "N": "ACGT", "W": "AT", "S": "CG", "M": "AC",
             "K": "GT", "B": "CGT", "D": "AGT", "H": "ACT"}
    L = len(pattern)
    fits = lambda w: all(b in iupac[q] for b, q in zip(w, pattern))
    out = []
    for c, text in enumerate(contigs):
        for p in range(len(text) - L + 1):
            w = text[p:p + L]
            if "N" in w:
                continue
            if fits(w):
                out.append((c, p, 0))
            if fits(revcomp(w)):
                out.append((c, p, 1))
    return out


def label(lens, intervals, rule, contig, pos):
    """vsc_regions_locate restated: the index of the most specific interval the 23-base window at (contig, pos) is in - cut
    off at the contig's end, where it overlaps with what is left and lies inside nothing - or NONE.  Most specific: the
    largest start, then the smallest clipped end, then the lowest index."""
    if not (0 <= contig < len(lens)) or not (0 <= pos < lens[contig]):
        return NONE
    end = min(pos + WINDOW, lens[contig])
    best = None
    for i, (c, a, b) in enumerate(intervals):
        b = min(b, lens[c])
        if c != contig or a >= b:
            continue
        inside = a <= pos and pos + WINDOW <= b
        overlap = a < end and b > pos
        if inside if rule == "inside" else overlap:
            cand = (-a, b, i)
            if best is None or cand < best:
                best = cand
    return NONE if best is None else best[2]


def targets_of(lens, intervals, rule, groups, loci):
    out = []
    for c, p, _ in loci:
        lab = label(lens, intervals, rule, c, p) if 0 <= c < len(lens) else NONE
        out.append(lab if lab == NONE or groups is None else groups[lab])
    return out


# ---- the small fixture ----------------------------------------------------------------------------------------------------
SEED = 7


def _rnd(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].tobytes().decode()


@functools.lru_cache(maxsize=None)
def small():
    """Contigs of 6000, 900, 60 and 23 random bases, an N run in the second, 200 bases of CCAGG repeats in the first (crowded
    candidates); 40 exons of 100 bases tiling the start of contig 0, contig 1 whole, a gene [0, 3000) given after its exons,
    contig 2 whole, an interval of 10 bases; rule inside; four exons per target, 14 targets in all."""
    rng = np.random.default_rng(SEED)
    contigs = [_rnd(rng, n) for n in (6000, 900, 60, 23)]
    contigs[0] = contigs[0][:1010] + "CCAGG" * 40 + contigs[0][1210:]
    contigs[1] = contigs[1][:400] + "N" * 30 + contigs[1][430:]
    lens = [len(c) for c in contigs]
    intervals = [(0, 100 * i, 100 * i + 100) for i in range(40)] + [(1, 0, 900), (0, 0, 3000), (2, 0, 60), (0, 5000, 5010)]
    groups = [i // 4 for i in range(40)] + [10, 11, 12, 13]
    loci = enumerate_ngg(contigs)
    target = targets_of(lens, intervals, "inside", groups, loci)
    n = len(loci)
    keys = {
        "ties": [int(x) for x in rng.integers(0, 8, n)],
        "high": [(1 << 63) | int(x) for x in rng.integers(0, 1 << 20, n)],
        "ends": [(int(x) << 62) | int(y) for x, y in zip(rng.integers(0, 4, n), rng.integers(0, 4, n))],
    }
    return {"contigs": contigs, "lens": lens, "intervals": intervals, "groups": groups, "rule": "inside", "n_targets": 14, "loci": loci,
            "target": target, "keys": keys}


@functools.lru_cache(maxsize=None)
def small_expected(key_set, k, spacing, min_key=0):
    f = small()
    return pick(f["lens"], f["loci"], f["target"], f["keys"][key_set], f["n_targets"], k, spacing, min_key=min_key)


def small_floors():
    """What the small fixture is built for, asserted on the restatement's own output."""
    f = small()
    sizes = [sum(1 for t in f["target"] if t == g) for g in range(f["n_targets"])]
    assert sum(1 for s in sizes if s > 64) >= 1, sizes
    assert min(sizes) == 0, sizes
    for key_set in f["keys"]:
        differ = lambda k, s: sum(1 for a, b in zip(small_expected(key_set, k, s)[0], small_expected(key_set, k, 0)[0]) if a != b)
        assert differ(4, 20) >= 5, (key_set, differ(4, 20))
        assert differ(32, 1) >= 3, (key_set, differ(32, 1))
        assert small_expected(key_set, 4, 1000)[3]["targets_short"] >= 1
        counts = small_expected(key_set, 4, 20)[1]
        assert any(c == 4 for c in counts) and any(c == 0 for c in counts)
    return sizes


def loci_array(loci, dtype):
    a = np.zeros(len(loci), dtype=dtype)
    if len(loci):
        m = np.array(loci, dtype=np.int64).reshape(-1, 3)
        a["contig"], a["pos"], a["strand"] = m[:, 0] & 0xFFFFFFFF, m[:, 1] & 0xFFFFFFFF, m[:, 2] & 0xFFFFFFFF
    return a


# ---- synthetic loci: more targets than a launch has waves ------------------------------------------------------------------
def many_targets(n_targets, contig_len, seed=11):
    """1 to 3 synthetic '+' / '-' loci per target on one contig, in target order, with 3-bit keys."""
    rng = np.random.default_rng(seed)
    per = rng.integers(1, 4, n_targets)
    target = np.repeat(np.arange(n_targets), per)
    n = len(target)
    loci = [(0, int(p), int(s)) for p, s in zip(rng.integers(0, contig_len - WINDOW + 1, n), rng.integers(0, 2, n))]
    return loci, [int(t) for t in target], [int(x) for x in rng.integers(0, 8, n)]
