"""Shared by tests/test_pairs_cpu.py and tests/test_pairs.py: the definitions of the paired-nickase screen by brute force in
plain numpy - every (a-record, b-record) combination of a pair, every (a, b) combination of a loci array; no bisect, nothing
shared with the library - and the planter: the three-contig layout of regions_cases.LENS with guide pairs planted at, inside
and just outside the bounds of a delta range."""
import numpy as np

from helpers import plant, random_guides, random_seq
from regions_cases import LENS

PAIR_SUMMARY = np.dtype([("sites", "<u8"), ("nm_sum", "<u8", (17,)), ("nm_max", "<u8", (9,)), ("on_target", "<u4"),
                         ("reserved", "<u4")])
PAIR_SITE = np.dtype([("pair", "<u4"), ("a_rec", "<u4"), ("b_rec", "<u4"), ("delta", "<i4")])
NONE = 0xFFFFFFFF
M = 4
N_GUIDES = 16
DELTA = (23, 43)        # nickase offsets 0 .. 20: PAM-out, the protospacers do not overlap
WIDE = (-2000, 2000)    # every record has many partners
A, B, C3, D, E, NOHIT, ONCE, NEVER = 0, 1, 2, 3, 4, 5, 6, 7  # guides with a role; 8 .. 15 are only planted at random
# (0, 1) twice: duplicate pairs get a row each; guide 0 is in three different pairs; guide 5 has no hit at all
PAIRS = [(A, B), (A, C3), (D, A), (E, NOHIT), (A, B), (B, A)]


def brute_loci_pairs(loci, delta):
    """Every (a, b) with loci[a] on '-', loci[b] on '+', the same contig (not NONE) and delta[0] <= pos[b] - pos[a] <=
    delta[1], in ascending (a, b): all n x n combinations against the definition."""
    c = loci["contig"].astype(np.int64)
    p = loci["pos"].astype(np.int64)
    s = loci["strand"].astype(np.int64)
    d = p[None, :] - p[:, None]  # [a, b]
    ok = (s[:, None] == 1) & (s[None, :] == 0) & (c[:, None] == c[None, :]) & (c[:, None] != NONE)
    ok &= (d >= delta[0]) & (d <= delta[1])
    return np.argwhere(ok).astype(np.uint32).reshape(-1, 2)


def brute_hits_pairs(hits, pairs, delta, exclude=None):
    """(rows, sites) of vsc_hits_pairs from the records (HIT_DTYPE, result order): per pair every record of guide a against
    every record of guide b.  exclude: None or (contig, pos, strand) per guide."""
    g = hits["guide"].astype(np.int64)
    c = hits["contig"].astype(np.int64)
    p = hits["pos"].astype(np.int64)
    s = (hits["info"] >> 31).astype(np.int64)
    nm = ((hits["info"] >> 23) & 31).astype(np.int64)
    ex = None if exclude is None else np.asarray(exclude, dtype=np.int64).reshape(-1, 3)
    rows = np.zeros(len(pairs), dtype=PAIR_SUMMARY)
    sites = []
    for j, (a, b) in enumerate(pairs):
        ia, ib = np.nonzero(g == a)[0], np.nonzero(g == b)[0]
        plus_minus = np.where(s[ia][:, None] == 0, p[ia][:, None] - p[ib][None, :], p[ib][None, :] - p[ia][:, None])
        ok = (c[ia][:, None] == c[ib][None, :]) & (s[ia][:, None] != s[ib][None, :])
        ok &= (plus_minus >= delta[0]) & (plus_minus <= delta[1])
        if ex is not None:
            at_a = (c[ia] == ex[a, 0]) & (p[ia] == ex[a, 1]) & (s[ia] == ex[a, 2])
            at_b = (c[ib] == ex[b, 0]) & (p[ib] == ex[b, 1]) & (s[ib] == ex[b, 2])
            on = ok & at_a[:, None] & at_b[None, :]
            rows["on_target"][j] = int(on.any())
            ok &= ~on
        for x, y in np.argwhere(ok):  # row-major: ascending (a_rec, b_rec)
            ra, rb = ia[x], ib[y]
            sites.append((j, ra, rb, plus_minus[x, y]))
            rows["nm_sum"][j, nm[ra] + nm[rb]] += 1
            rows["nm_max"][j, max(nm[ra], nm[rb])] += 1
        rows["sites"][j] = int(ok.sum())
    return rows, np.array(sites, dtype=np.int64).reshape(-1, 4).astype(np.int64)


def sites_array(sites):
    """brute_hits_pairs' site tuples as PAIR_SITE records (the library's bytes)."""
    out = np.zeros(len(sites), dtype=PAIR_SITE)
    if len(sites):
        out["pair"], out["a_rec"], out["b_rec"], out["delta"] = sites[:, 0], sites[:, 1], sites[:, 2], sites[:, 3]
    return out


def shard_boundary():
    """Global base position where the second of two shards of the LENS layout begins (contig 0 starts at 0 and spans it)."""
    import varscot_amd as va
    packed = va.PackedGenome.from_sequences(["A" * n for n in LENS])
    assert int(packed.contigs["offset"][0]) == 0
    b = packed.shard_words(0, 2)[1] * 32
    assert 7000 < b < LENS[0] - 200, b
    return b


def planted(seed=7, n_random=110):
    """dict: contigs, guides, planted = {name: ...} positions the tests assert on, exclude (one locus per guide).
    Contig 0 [300, 6300): the structured cases, 250 bases apart; the rest of contig 0 and contig 1: random sites of all
    guides but NOHIT, ONCE and NEVER, 0 .. M substitutions, both strands; around the shard boundary one paired site whose two
    windows lie on different sides of it."""
    rng = np.random.default_rng(seed)
    guides = random_guides(rng, N_GUIDES)
    contigs = [random_seq(rng, n) for n in LENS]
    boundary = shard_boundary()
    c0 = contigs[0]
    # random sites first, so that the structured ones are never overwritten
    for _ in range(n_random):
        g = int(rng.choice([x for x in range(N_GUIDES) if x not in (NOHIT, ONCE, NEVER)]))
        strand = "+-"[int(rng.integers(0, 2))]
        nsub = int(rng.integers(0, M + 1))
        if rng.random() < 0.7:
            pos = int(rng.integers(6400, LENS[0] - 200))
            if abs(pos - boundary) < 200:
                continue
            c0 = plant(rng, c0, guides[g], pos, strand, nsub)
        else:
            contigs[1] = plant(rng, contigs[1], guides[g], int(rng.integers(100, LENS[1] - 100)), strand, nsub)
    out = {"minus_plus": {}, "plus_minus": {}}
    p = 300
    lo, hi = DELTA
    for d in (lo - 1, lo, hi, hi + 1):  # A on '-' at p, B on '+' at p + d: delta = d (B second: at d = 22 it owns the shared base)
        c0 = plant(rng, c0, guides[A], p, "-", 0)
        c0 = plant(rng, c0, guides[B], p + d, "+", 0)
        out["minus_plus"][d] = (p, p + d)
        p += 250
    for d in (lo - 1, lo, hi, hi + 1):  # mirrored: B on '-' at p, A on '+' at p + d
        c0 = plant(rng, c0, guides[B], p, "-", 0)
        c0 = plant(rng, c0, guides[A], p + d, "+", 0)
        out["plus_minus"][d] = (p + d, p)
        p += 250
    out["graded"] = []
    for k in range(M + 1):  # 0 .. M substitutions on both sides, then k against M - k
        for sub_b in (k, M - k):
            c0 = plant(rng, c0, guides[A], p, "-", k)
            c0 = plant(rng, c0, guides[B], p + 30, "+", sub_b)
            out["graded"].append((p, p + 30, k, sub_b))
            p += 250
    out["perfect"] = out["graded"][0][:2]  # k = 0 on both sides: the excluded on-target of pair (A, B)
    c0 = plant(rng, c0, guides[A], p, "+", 0)  # the same strand, close: never a pair
    c0 = plant(rng, c0, guides[B], p + 30, "+", 0)
    out["same_strand"] = (p, p + 30)
    p += 250
    c0 = plant(rng, c0, guides[A], p, "-", 1)  # guide A in two more pairs: (A, C3) and (D, A)
    c0 = plant(rng, c0, guides[C3], p + 35, "+", 2)
    p += 250
    c0 = plant(rng, c0, guides[D], p, "-", 0)
    c0 = plant(rng, c0, guides[A], p + 25, "+", 3)
    p += 250
    c0 = plant(rng, c0, guides[E], p, "-", 0)  # (E, NOHIT): guide NOHIT is planted nowhere
    c0 = plant(rng, c0, guides[ONCE], p + 100, "+", 0)  # ONCE: exactly one perfect site
    out["once"] = p + 100
    p += 250
    assert p < 6400
    # close in global position, on different contigs: the last 60 bases of contig 0 and the first 60 of contig 1
    c0 = plant(rng, c0, guides[A], LENS[0] - 23 - 7, "-", 0)
    contigs[1] = plant(rng, contigs[1], guides[B], 3, "+", 0)
    out["cross_contig"] = (LENS[0] - 30, 3)
    # one paired site across the shard boundary: the '-' window ends before it, the '+' window starts after it
    c0 = plant(rng, c0, guides[A], boundary - 28, "-", 0)
    c0 = plant(rng, c0, guides[B], boundary + 2, "+", 0)
    out["across"] = (boundary - 28, boundary + 2, boundary)
    contigs[0] = c0
    exclude = np.full((N_GUIDES, 3), 0, dtype=np.int64)
    exclude[:, 0] = NONE
    exclude[A] = (0, out["perfect"][0], 1)
    exclude[B] = (0, out["perfect"][1], 0)
    out.update(contigs=contigs, guides=guides, exclude=exclude)
    return out


def all_ordered_pairs(n=N_GUIDES):
    return [(a, b) for a in range(n) for b in range(n) if a != b]
