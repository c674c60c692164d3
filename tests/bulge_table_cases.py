"""The table score of bulged alignments and cut sites (include/varscot_hip.h, vsc_bulge_hits_table / vsc_sites_table) restated
in plain Python, letter by letter.  Nothing here calls the library: py_bulge_score() is the definition for one table, one guide,
one site, one d and one split point in IEEE doubles and the fixed order; member() recomputes (NM, i) with
pattern_bulge_cases.best; site_scores() is the member loop of a cut site; bulged_scored() / site_records() / rows / cut() apply
them to the alignments and sites of the other *_cases restatements."""
import functools

import numpy as np

import pattern_bulge_cases as pbc
import pattern_cases as pc
import pattern_table_cases as ptc
import sites_cases as sc

ONE = ptc.ONE
TABLE_ROW_DTYPE = ptc.TABLE_ROW_DTYPE
SITE_SCORE_DTYPE = np.dtype([("best", "<u4"), ("top", "<u4"), ("top_d", "<u4"), ("reserved", "<u4")])
SHAPES = {"SpCas9": (23, (0, 20), (21, 22)), "SaCas9": (27, (0, 21), (23, 24, 25, 26)), "Cas12a": (27, (4, 23), (0, 1, 2, 3))}


def random_bulge_table(rng, shape, zeros=0, ones=0):
    """ptc.random_pattern_table plus "dna" and "rna" [ps_len][4]: full mantissas in (0, 1) with `zeros` // 4 + 1 entries of
    each array exactly 0 and `ones` // 4 + 1 exactly 1 when any are asked for."""
    t = ptc.random_pattern_table(rng, shape, zeros, ones)
    n = t["ps"][1]
    for key in ("dna", "rna"):
        w = rng.random((n, 4))
        if zeros or ones:
            cells = rng.permutation(n * 4)
            nz, no = (zeros // 4 + 1 if zeros else 0), (ones // 4 + 1 if ones else 0)
            for k, cell in enumerate(cells[:nz + no]):
                w[int(cell) // 4, int(cell) % 4] = 0.0 if k < nz else 1.0
        t[key] = w
    return t


def all_ones(table):
    """The same base with every dna and rna weight 1.0."""
    t = dict(table)
    t["dna"], t["rna"] = np.ones_like(table["dna"]), np.ones_like(table["rna"])
    return t


def defined(table, d, i):
    """Is (d, i) an alignment of the definition: a + 1 <= i <= e - 1 (RNA: i + b <= e - 1), 16 <= L + d <= 32?"""
    a, n = table["ps"]
    if d not in (-2, -1, 1, 2) or not 16 <= table["L"] + d <= 32 or n < 4:
        return False
    return a + 1 <= i and i + max(-d, 0) <= a + n - 1


def py_bulge_score(table, guide, s, d, i):
    """The definition: the paired site q, the pattern score of (G, q) without the unpaired positions, then the weights of
    the unpaired letters in ascending order.  Python floats are IEEE doubles: one rounding per product."""
    guide, s = guide.upper(), s.upper()
    L, (a, n) = table["L"], table["ps"]
    assert len(guide) == L and len(s) == L + d and all(ch in "ACGT" for ch in s) and defined(table, d, i)
    if d > 0:
        q = s[:i] + s[i + d:]
        x = ptc.py_score(table, guide, q)
        for t in range(d):
            x = x * float(table["dna"][i - a, "ACGT".index(s[i + t])])
        return x
    b = -d
    # positions [i, i + b) carry no letter: an N of the guide takes no part in the pattern score, whatever stands in q there
    q = s[:i] + "A" * b + s[i:]
    x = ptc.py_score(table, guide[:i] + "N" * b + guide[i + b:], q)
    for t in range(b):
        g = guide[i + t]
        if g in "ACGT":
            x = x * float(table["rna"][i + t - a, "ACGT".index(g)])
    return x


def member(table, guide, s, d):
    """(NM, i, f) of the member d of a site, recomputed from its letters s (read orientation)."""
    guide, s = guide.upper(), s.upper()
    if d == 0:
        nm = sum(s[j] not in pc.IUPAC[guide[j]] for j in range(len(guide)))
        return nm, 0, ptc.py_fixed(ptc.py_score(table, guide, s))
    nm, i, _ = pbc.best(guide, s, table["ps"], d)
    return nm, i, ptc.py_fixed(py_bulge_score(table, guide, s, d, i))


_clean = functools.lru_cache(maxsize=16)(pc.genome_of)  # (a contig's letters once, not once per site)


def text_of(contigs, strand, c, pos, n):
    """The n letters at forward position pos of contig c in read orientation."""
    w = _clean(contigs[c])[pos:pos + n]
    assert len(w) == n and pos >= 0
    return w if strand == 0 else pc.rc(w)


def bulged_scored(contigs, guides, alignments, table):
    """f per bulged alignment (guide, strand, contig, pos, d, nm, index), by the RECORD's index."""
    L = table["L"]
    return np.array([ptc.py_fixed(py_bulge_score(table, guides[g], text_of(contigs, strand, c, p, L + d), d, index))
                     for g, strand, c, p, d, _, index in alignments], dtype=np.uint32)


def bulged_rows(alignments, f, n_guides):
    rows = np.zeros(n_guides, dtype=TABLE_ROW_DTYPE)
    for x, v in zip(alignments, f):
        rows["score_sum"][x[0]] += int(v)
        if v:
            rows["positive"][x[0]] += 1
            rows["positive_nm"][x[0], min(x[5], 8)] += 1
    return rows


def site_scores(table, contigs, guides, site, anchor="end"):
    """(best, top, top_d, NM of the best alignment) of one entry of sites_cases.collapse()."""
    x, _, _, a, nm_by_d = site
    g, strand, c, _, best_d, _, _ = x
    L = table["L"]
    at_start = (anchor == "end") == (strand == 1)
    best = top = top_d = best_nm = top_rank = None
    for d in sorted(nm_by_d):
        pos = a if at_start else a - (L + d)
        nm, _, f = member(table, guides[g], text_of(contigs, strand, c, pos, L + d), d)
        rank = (nm + abs(d), abs(d), 0 if d >= 0 else 1)
        if d == best_d:
            best, best_nm = f, nm
        if top is None or f > top or (f == top and rank < top_rank):
            top, top_d, top_rank = f, d + 2, rank
    return best, top, top_d, best_nm


def site_records(table, contigs, guides, sites, n_guides, anchor="end"):
    """(SITE_SCORE_DTYPE records, TABLE_ROW_DTYPE rows) over the entries of collapse()."""
    rec = np.zeros(len(sites), dtype=SITE_SCORE_DTYPE)
    rows = np.zeros(n_guides, dtype=TABLE_ROW_DTYPE)
    for k, s in enumerate(sites):
        best, top, top_d, best_nm = site_scores(table, contigs, guides, s, anchor)
        rec[k] = (best, top, top_d, 0)
        g = s[0][0]
        rows["score_sum"][g] += top
        if top:
            rows["positive"][g] += 1
            rows["positive_nm"][g, min(best_nm, 8)] += 1
    return rec, rows


def cut(site_guides, top, top_k=0, min_score=0):
    """The indices of the sites the selection keeps, ascending: per guide those with top >= min_score, of them the first top_k
    (0: all) under top descending, then record order."""
    by_guide = {}
    for k, g in enumerate(site_guides):
        if top[k] >= min_score:
            by_guide.setdefault(int(g), []).append(k)
    keep = []
    for idx in by_guide.values():
        if top_k and len(idx) > top_k:
            idx = sorted(idx, key=lambda k: (-int(top[k]), k))[:top_k]
        keep.extend(idx)
    return np.array(sorted(keep), dtype=np.int64)


# ---- the site selection digit by digit ------------------------------------------------------------------------------------
def digits_bulge_table():
    """pattern_table_cases.digits_table() with dyadic bulge weights: dna 1 - 2^-min(3 + i + 7 b, 29), rna 1 - 2^-min(2 + i + 5 b,
    29) for protospacer position i and base b - a site's top then agrees with its neighbours' in its upper bytes as the pattern
    hits' f does."""
    t = ptc.digits_table()
    i, b = np.arange(20)[:, None], np.arange(4)[None, :]
    t["dna"] = 1.0 - 2.0 ** -np.minimum(3 + i + 7 * b, 29)
    t["rna"] = 1.0 - 2.0 ** -np.minimum(2 + i + 5 * b, 29)
    return t


@functools.lru_cache(maxsize=None)
def digits_sites():
    """pattern_table_cases.digits_scenario()'s genome and guides as cut sites at dna = rna = 1: the plain hits and the bulged
    alignments of the pattern restatements, collapsed and scored, and the cuts that ptc.digit_cases finds on `top`.  The floors
    are ptc.digit_floors', on top."""
    d = ptc.digits_scenario()
    pattern, contigs, guides, m, proto = d["pattern"], d["contigs"], d["guides"], d["m"], (0, 20)
    n = len(guides)
    table = digits_bulge_table()
    plain_rec = pc.arrays(d["hits"], n)[0]
    plain = sc.plain_of_pattern(plain_rec)
    hits, _ = pbc.brute_force(contigs, pattern, guides, proto, m, 1, 1)
    bulged = sc.bulged_of_hits(hits)
    sites = sc.collapse(plain, bulged, len(pattern), "end")
    site_rec, site_rows = sc.arrays(sites, plain, bulged, n)
    scores, rows = site_records(table, contigs, guides, sites, n, "end")
    guide_of, top = site_rec["guide"], scores["top"]
    found = ptc.digit_cases(guide_of, top, n)
    s = {"pattern": pattern, "proto": proto, "contigs": contigs, "guides": guides, "m": m, "table": table, "sites": sites, "site_rec": site_rec,
         "site_rows": site_rows, "scores": scores, "rows": rows, "cases": [c[:2] for c in found], "serves": [c[2] for c in found]}
    unmet = ptc.digit_floors(guide_of, top, n, s["cases"], lambda k, ms: cut(guide_of, top, k, ms))
    assert not unmet, unmet
    assert any(len(x[4]) > 1 for x in sites) and (scores["top"] != scores["best"]).any()  # sites of several members, scored as another
    return s


def make_table(va, table):
    """The library's object of a restated table."""
    base = ptc.make_table(va, table)
    try:
        return va.BulgeTable(base, table["dna"], table["rna"])
    finally:
        base.close()
