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


# ---- segment sizes around every boundary of the select ----------------------------------------------------------------------
# 64 / 128 / 192: a lane's second, third and fourth register slot; 256: the last segment the select takes from registers
SIZES = (0, 1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 258, 319, 320, 321, 511, 512, 513, 1025)
WAVE_CAP = 256
BOUNDARY_SPACING = 20   # the spacing the planted candidates are placed for
BOUNDARY_KEYS = ("equal", "ties", "wide", "top")
ORDERS = ("blocks", "interleaved")


def _apart(target):
    """An order of the candidates in which no two neighbours share a target and every target's candidates keep their order:
    always the target with the most candidates left that is not the one just taken."""
    left = {}
    for i, t in enumerate(target):
        left.setdefault(t, []).append(i)
    for members in left.values():
        members.reverse()
    order, last = [], None
    while left:
        t = max((t for t in left if t != last), key=lambda t: (len(left[t]), -t))
        order.append(left[t].pop())
        if not left[t]:
            del left[t]
        last = t
    return order


@functools.lru_cache(maxsize=None)
def boundary(n_contigs):
    """One target per size in SIZES, the target numbers scrambled against the sizes; synthetic '+' / '-' loci on n_contigs
    contigs of ACGT repeats, the positions of a target of s candidates from a span of max(4 s, 64) bases (the same span on
    every contig).  The first candidates of every target of three or more are planted for spacing 20: '+' with cut
    coordinate x, one with its cut at x + 19, '-' with its cut at x + 20, '-' with its cut at x, all on one contig and first
    under BEFORE in every key set.  Two input orders: "blocks" (a target's candidates are contiguous) and "interleaved" (no
    two neighbours share a target; the order inside a target is the same, so the planted ones stay its first)."""
    rng = np.random.default_rng(29 + n_contigs)
    S = BOUNDARY_SPACING
    number = [int(t) for t in rng.permutation(len(SIZES))]
    contig_len = 4 * (sum(max(4 * s, 64) for s in SIZES) // 4 + 32)
    loci, target, planted = [], [], {}
    keys = {name: [] for name in BOUNDARY_KEYS}
    off = 32
    for size, t in zip(SIZES, number):
        span = max(4 * size, 64)
        block = [(int(c), off + int(p), int(s)) for c, p, s in zip(rng.integers(0, n_contigs, size), rng.integers(0, span - WINDOW, size),
                                                                    rng.integers(0, 2, size))]
        ks = {"equal": [5] * size, "ties": [int(x) for x in rng.integers(0, 8, size)], "wide": [int(x) for x in rng.integers(0, 1 << 62, size)],
              "top": [(1 << 63) | (int(x) << 32) for x in rng.integers(0, (1 << 31) - 8, size)]}
        if size >= 3:
            c, p = int(rng.integers(0, n_contigs)), off + int(rng.integers(0, span - 32 - WINDOW))
            block[:4] = [(c, p, 0), (c, p + S - 1, 0), (c, p + S + 11, 1), (c, p + 11, 1)][:size]
            x = [cut_coordinate(q, s, WINDOW, 17) for _, q, s in block[:4]]
            assert x[1] == x[0] + S - 1 and x[2] == x[0] + S and x[3:] == [x[0]][:size - 3] and block[2][1] + 6 == x[0] + S
            for j in range(min(size, 4)):
                ks["ties"][j] = 7
                ks["wide"][j] = (1 << 62) - 1 - j
                ks["top"][j] = (1 << 63) | (((1 << 31) - 1 - j) << 32)
            planted[t] = len(loci)   # the index of the first of them under "blocks"
        loci += block
        target += [t] * size
        for name in BOUNDARY_KEYS:
            keys[name] += ks[name]
        off += span
    assert all(0 <= p and p + WINDOW <= contig_len for _, p, _ in loci)
    orders = {"blocks": list(range(len(loci))), "interleaved": _apart(target)}
    return {"contigs": ["ACGT" * (contig_len // 4)] * n_contigs, "lens": [contig_len] * n_contigs, "n_targets": len(SIZES), "loci": loci,
            "target": target, "keys": keys, "orders": orders, "size_of": {t: s for s, t in zip(SIZES, number)}, "planted": planted}


def boundary_inputs(n_contigs, key_set, order):
    """(loci, target, key) of the fixture in one of its two orders."""
    f = boundary(n_contigs)
    o = f["orders"][order]
    return [f["loci"][i] for i in o], [f["target"][i] for i in o], [f["keys"][key_set][i] for i in o]


def boundary_planted(n_contigs, order):
    """target -> the indices, in this order, of its planted candidates: cut x, x + 19, x + 20 and (from four on) x again."""
    f = boundary(n_contigs)
    at = {j: i for i, j in enumerate(f["orders"][order])}
    return {t: [at[first + j] for j in range(min(f["size_of"][t], 4))] for t, first in f["planted"].items()}


@functools.lru_cache(maxsize=None)
def boundary_expected(n_contigs, key_set, order, k, spacing, one_contig=False):
    """The restatement on the fixture; one_contig: with every contig number set to 0 (what a select that ignores it sees)."""
    f = boundary(n_contigs)
    loci, target, key = boundary_inputs(n_contigs, key_set, order)
    if one_contig:
        loci = [(0, p, s) for _, p, s in loci]
    return pick(f["lens"], loci, target, key, f["n_targets"], k, spacing)


def boundary_floors():
    """What the boundary fixtures are built for, asserted on the restatement's own output."""
    S = BOUNDARY_SPACING
    assert SIZES[0] == 0 and all(b in SIZES for s in (64, 128, 192, 256) for b in (s - 1, s, s + 1)) and max(SIZES) > 4 * WAVE_CAP
    for n_contigs in (1, 3):
        f = boundary(n_contigs)
        size_of = f["size_of"]
        assert sorted(size_of.values()) == list(SIZES) and [size_of[t] for t in range(len(SIZES))] != list(SIZES)
        assert len(f["loci"]) == sum(SIZES) > 5000 and len({c for c, _, _ in f["loci"]}) == n_contigs
        assert {s for _, _, s in f["loci"]} == {0, 1}
        on = {}   # (target, cut coordinate) -> the contigs it occurs on
        for (c, p, s), t in zip(f["loci"], f["target"]):
            on.setdefault((t, cut_coordinate(p, s, WINDOW, 17)), set()).add(c)
        assert n_contigs == 1 or sum(1 for contigs in on.values() if len(contigs) > 1) > 200   # one coordinate on two contigs is frequent
        for order in ORDERS:
            _, target, _ = boundary_inputs(n_contigs, "equal", order)
            sizes = [sum(1 for t in target if t == g) for g in range(len(SIZES))]
            assert sizes == [size_of[g] for g in range(len(SIZES))]
            runs = sum(1 for a, b in zip(target, target[1:]) if a != b) + 1
            assert runs == (len(target) if order == "interleaved" else len(SIZES) - 1), (order, runs)
            planted = boundary_planted(n_contigs, order)
            assert sorted(planted) == sorted(t for t, size in size_of.items() if size >= 3)
            for key_set in BOUNDARY_KEYS:
                exp = lambda k, s, **kw: boundary_expected(n_contigs, key_set, order, k, s, **kw)  # noqa: E731
                spaced, free = exp(4, S), exp(4, 0)
                for t, size in size_of.items():
                    if size >= 63:
                        assert spaced[0][t] != free[0][t], (key_set, size)
                    if size >= 3:
                        p = planted[t]
                        assert spaced[0][t][:2] == [p[0], p[2]] and free[0][t][:len(p)] == p, (key_set, size)
                        assert spaced[2][p[1]] == NONE and (size < 4 or spaced[2][p[3]] == NONE)
                full, far = exp(32, 0), exp(32, 1000)
                assert all(full[1][t] == min(size, 32) for t, size in size_of.items())
                short = [size_of[t] for t in range(len(SIZES)) if far[1][t] < 32 and size_of[t] > far[1][t]]
                assert sum(1 for s in short if s > WAVE_CAP) >= 3 and sum(1 for s in short if s <= WAVE_CAP) >= 3
                assert far[3]["targets_short"] == len(short)
                if n_contigs > 1:
                    flat = exp(32, S, one_contig=True)   # (at k = 4 two of the picks are the planted ones, on one contig)
                    differ = [size_of[t] for t in range(len(SIZES)) if flat[0][t] != exp(32, S)[0][t]]
                    assert sum(1 for s in differ if s > WAVE_CAP) >= 3 and sum(1 for s in differ if s <= WAVE_CAP) >= 3, (key_set, differ)
                if key_set == "equal":
                    for k in KS:
                        lowest = [[i for i, t in enumerate(target) if t == g][:k] for g in range(len(SIZES))]
                        assert [row[:c] for row, c in zip(exp(k, 0)[0], exp(k, 0)[1])] == lowest
    return list(SIZES)


# ---- a wave that takes a large, a small and a large target in turn ----------------------------------------------------------
SAME_WAVE_K, SAME_WAVE_SPACING = 32, 50
SAME_WAVE_TRIPLES = ((1, (700, 5, 300)), (2, (200, 400, 3)))   # the first target of a triple and the three sizes
SAME_WAVE_SPAN = 2000


@functools.lru_cache(maxsize=None)
def same_wave(n_waves, contig_len=100000, seed=13):
    """2 n_waves + 3 targets in target order, so that a launch of n_waves waves gives wave w the targets w, w + n_waves and
    w + 2 n_waves: 1 to 3 loci each as many_targets, but for the two triples of SAME_WAVE_TRIPLES, whose three targets draw
    their sizes' worth of loci from one range of SAME_WAVE_SPAN bases each."""
    n_targets = 2 * n_waves + 3
    rng = np.random.default_rng(seed)
    per = rng.integers(1, 4, n_targets)
    spans = {}
    for j, (first, sizes) in enumerate(SAME_WAVE_TRIPLES):
        for r, size in enumerate(sizes):
            per[first + r * n_waves] = size
            spans[first + r * n_waves] = 1000 + 2 * j * SAME_WAVE_SPAN
    target = np.repeat(np.arange(n_targets), per)
    n = len(target)
    pos = rng.integers(0, contig_len - WINDOW + 1, n)
    for t, lo in spans.items():
        mine = np.flatnonzero(target == t)
        pos[mine] = lo + rng.integers(0, SAME_WAVE_SPAN, len(mine))
    loci = [(0, int(p), int(s)) for p, s in zip(pos, rng.integers(0, 2, n))]
    return {"lens": [contig_len], "n_targets": n_targets, "loci": loci, "target": [int(t) for t in target],
            "key": [int(x) for x in rng.integers(0, 8, n)]}


@functools.lru_cache(maxsize=None)
def same_wave_expected(n_waves):
    f = same_wave(n_waves)
    return pick(f["lens"], f["loci"], f["target"], f["key"], f["n_targets"], SAME_WAVE_K, SAME_WAVE_SPACING)


def _pick_behind(loci, members, key, k, spacing, taken):
    """The PICK loop over one target's members with the candidates `taken` treated as picks that are already there (they
    block, they do not count): what a select sees that keeps the picks of the targets it took before."""
    picked = []
    x = lambda i: cut_coordinate(loci[i][1], loci[i][2], WINDOW, 17)  # noqa: E731
    for i in sorted(members, key=lambda i: (-key[i], i)):
        if len(picked) == k:
            break
        if any(loci[j][0] == loci[i][0] and abs(x(j) - x(i)) < spacing for j in list(taken) + picked):
            continue
        picked.append(i)
    return picked


def same_wave_floors(n_waves):
    """The path of every target of the two triples, and: with the picks of a triple's earlier targets left standing, its
    second and its third target get other picks."""
    f = same_wave(n_waves)
    picks, counts, _, stats = same_wave_expected(n_waves)
    assert f["n_targets"] == 2 * n_waves + 3 and stats["targets_picked"] == f["n_targets"]
    members = lambda t: [i for i, g in enumerate(f["target"]) if g == t]  # noqa: E731
    paths = []
    for first, sizes in SAME_WAVE_TRIPLES:
        taken = []
        for r, size in enumerate(sizes):
            t = first + r * n_waves
            mine = members(t)
            assert len(mine) == size and mine == list(range(mine[0], mine[0] + size))
            paths.append(size > WAVE_CAP)
            clean = picks[t][:counts[t]]
            assert clean == _pick_behind(f["loci"], mine, f["key"], SAME_WAVE_K, SAME_WAVE_SPACING, [])
            if r:
                assert clean != _pick_behind(f["loci"], mine, f["key"], SAME_WAVE_K, SAME_WAVE_SPACING, taken), (t, size)
            taken += clean
    assert paths == [True, False, True, False, True, False]
    sizes = np.bincount(f["target"], minlength=f["n_targets"])
    assert sizes.min() >= 1 and (sizes > 3).sum() == 5   # (1 to 3 each but for the triples' five larger ones)
    return paths


# ---- beyond one launch: the small fixture over and over -------------------------------------------------------------------
def replicas(n, distinct=False):
    """n candidates as numpy arrays: the small fixture (key set "high") again and again, the targets of replica r shifted by
    14 r; distinct: key = (key << 20 | index in the block), bit 63 kept, so that no target has two equal keys.  Returns
    (index in the block [n], target [n], key [n], n_targets, the block's target and key lists)."""
    f = small()
    m = len(f["loci"])
    base_key = [(((q << 20) | i) & ((1 << 64) - 1)) | (1 << 63) for i, q in enumerate(f["keys"]["high"])] if distinct else f["keys"]["high"]
    if distinct:
        for g in range(f["n_targets"]):
            mine = [q for q, t in zip(base_key, f["target"]) if t == g]
            assert len(set(mine)) == len(mine)
    i = np.arange(n, dtype=np.int64)
    idx, rep = i % m, i // m
    tg = np.array(f["target"], dtype=np.uint32)[idx]
    target = np.where(tg == NONE, tg, tg + (f["n_targets"] * rep).astype(np.uint32)).astype(np.uint32)
    key = np.array(base_key, dtype=np.uint64)[idx]
    return idx, target, key, f["n_targets"] * int(-(-n // m)), (f["target"], base_key)


def replicas_expected(n, k, spacing, block):
    """(picks, counts, rank, stats) of replicas(n) as arrays, composed from two restatement calls: the whole block and the
    last, partial one."""
    f = small()
    m = len(f["loci"])
    target, key = block
    reps, rem = divmod(n, m)
    whole = as_arrays(pick(f["lens"], f["loci"], target, key, f["n_targets"], k, spacing))
    last = as_arrays(pick(f["lens"], f["loci"][:rem], target[:rem], key[:rem], f["n_targets"], k, spacing))
    first = np.arange(reps + 1, dtype=np.int64)[:, None, None] * m   # the index of every replica's first candidate
    blocks = np.concatenate([np.broadcast_to(whole[0], (reps,) + whole[0].shape), last[0][None]]).astype(np.int64)
    picks = np.where(blocks == NONE, blocks, blocks + first).astype(np.uint32)
    counts = np.concatenate([np.tile(whole[1], reps), last[1]])
    rank = np.concatenate([np.tile(whole[2], reps), last[2]])
    if not rem:
        picks, counts = picks[:reps], counts[:reps * f["n_targets"]]
    stats = {name: reps * whole[3][name] + last[3][name] for name in whole[3]}
    return picks.reshape(-1, k), counts, rank, stats


def permuted(expected, order):
    """The result for the candidates taken in `order` (new[j] = old[order[j]]), given the one for the old order - where no
    target has two equal keys, so that no index decides."""
    picks, counts, rank, stats = expected
    where = np.empty(len(order) + 1, dtype=np.uint32)
    where[order] = np.arange(len(order), dtype=np.uint32)
    where[-1] = NONE
    return where[np.where(picks == NONE, len(order), picks)], counts, rank[order], stats
