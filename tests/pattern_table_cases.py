"""The table score of pattern hits (include/varscot_hip.h, vsc_search_pattern_table) restated in plain Python, and the scenarios
the tests run it on.  Nothing here calls the library: py_score() is the definition for one table, one guide and one site in
IEEE doubles and the fixed order, scored() / table_rows() / cut() apply it, the rows and the selection to the hits of
pattern_cases.brute_force, and every scenario asserts floors on the restatement's OWN output."""
import functools

import numpy as np

import pattern_cases as pc

ONE = 1 << 30
TABLE_ROW_DTYPE = np.dtype([("score_sum", "<u8"), ("positive", "<u8"), ("positive_nm", "<u8", (9,)), ("reserved", "<u8")])


def shape_of(pattern, protospacer=None):
    """(L, (ps_start, ps_len), pam positions): the PAM positions are the pattern's letters that are not N, the protospacer -
    unless given - is the longest run of N."""
    L = len(pattern)
    pam_pos = tuple(j for j, ch in enumerate(pattern.upper()) if ch != "N")
    if protospacer is None:
        runs, j = [], 0
        while j < L:
            if pattern[j].upper() == "N":
                k = j
                while k < L and pattern[k].upper() == "N":
                    k += 1
                runs.append((k - j, j))
                j = k
            else:
                j += 1
        n, start = max(runs)
        protospacer = (start, n)
    return L, (int(protospacer[0]), int(protospacer[1])), pam_pos


def random_pattern_table(rng, shape, zeros=0, ones=0):
    """{"L", "ps", "pam_pos", "pair", "pam"}: weights with full mantissas in (0, 1), the diagonal 1, `zeros` entries off the
    diagonal exactly 0 and `ones` exactly 1; with PAM positions, also one PAM weight of each."""
    L, ps, pam_pos = shape
    pair = rng.random((ps[1], 4, 4))
    off = [(i, g, s) for i in range(ps[1]) for g in range(4) for s in range(4) if g != s]
    picks = rng.permutation(len(off))
    for n, k in enumerate(picks[:zeros + ones]):
        pair[off[int(k)]] = 0.0 if n < zeros else 1.0
    for b in range(4):
        pair[:, b, b] = 1.0
    pam = rng.random(4 ** len(pam_pos))
    if len(pam) > 1 and (zeros or ones):
        a, b = (int(x) for x in rng.choice(len(pam), size=2, replace=False))
        pam[a], pam[b] = (0.0 if zeros else pam[a]), (1.0 if ones else pam[b])
    return {"L": L, "ps": ps, "pam_pos": tuple(pam_pos), "pair": pair, "pam": pam}


def py_score(table, guide, site):
    """The definition: x = 1; for the protospacer positions in ascending order, where the guide's letter is one of ACGT and
    the site's differs, x = x * pair; then x = x * pam[k].  Python floats are IEEE doubles: one rounding per product."""
    guide, site = guide.upper(), site.upper()
    assert len(guide) == len(site) == table["L"] and all(ch in "ACGT" for ch in site)
    x = 1.0
    start, n = table["ps"]
    for i in range(n):
        g, s = guide[start + i], site[start + i]
        if g in "ACGT" and g != s:
            x = x * float(table["pair"][i, "ACGT".index(g), "ACGT".index(s)])
    k = 0
    for q in table["pam_pos"]:
        k = 4 * k + "ACGT".index(site[q])
    return x * float(table["pam"][k])


def py_fixed(x):
    return int(np.rint(np.float64(x) * np.float64(ONE)))  # round half to even


def site_text(contigs, L, strand, c, p):
    """The site in read orientation."""
    w = pc.genome_of(contigs[c])[p:p + L]
    return w if strand == 0 else pc.rc(w)


def scored(contigs, guides, hits, table):
    """f per hit of brute_force / definition."""
    L = table["L"]
    return np.array([py_fixed(py_score(table, guides[g], site_text(contigs, L, strand, c, p))) for g, strand, c, p, _, _ in hits],
                    dtype=np.uint32)


def table_rows(hits, f, n_guides):
    rows = np.zeros(n_guides, dtype=TABLE_ROW_DTYPE)
    for (g, _, _, _, nm, _), v in zip(hits, f):
        rows["score_sum"][g] += int(v)
        if v:
            rows["positive"][g] += 1
            rows["positive_nm"][g, nm] += 1
    return rows


def cut(hits, f, top_k=0, min_score=0):
    """The indices of the hits that the selection keeps, ascending: per guide those with f >= min_score, of them the first
    top_k (0: all) under f descending, then record order (the hits ARE in (guide, strand, contig, pos) order)."""
    keep = []
    by_guide = {}
    for k, h in enumerate(hits):
        if f[k] >= min_score:
            by_guide.setdefault(h[0], []).append(k)
    for g, idx in by_guide.items():
        if top_k and len(idx) > top_k:
            idx = sorted(idx, key=lambda k: (-int(f[k]), k))[:top_k]
        keep.extend(idx)
    return np.array(sorted(keep), dtype=np.int64)


# ---- scenarios ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def edge_table(L=23, place="3"):
    """pattern_cases.edge_scenario(L, place) with a table over its protospacer and its PAM letters, the hits at m = 8 scored."""
    e = pc.edge_scenario(L, place)
    rng = np.random.default_rng(5000 + 10 * L + pc.PLACES.index(place))
    table = random_pattern_table(rng, shape_of(e["pattern"]), zeros=L, ones=8)
    assert len(table["pam_pos"]) == (4 if place == "both" else 3)
    f = scored(e["contigs"], e["guides"], e["hits"], table)
    for strand in (0, 1):
        mine = [v for h, v in zip(e["hits"], f) if h[1] == strand]
        assert any(v == 0 for v in mine) and any(v > 0 for v in mine), strand  # a zero weight met, and not met, on both strands
    assert any(0 < v < ONE for v in f)
    return {"e": e, "table": table, "f": f}


def at(t, m):
    """(hits, f) of an edge_table at budget m."""
    keep = [k for k, h in enumerate(t["e"]["hits"]) if h[4] <= m]
    return [t["e"]["hits"][k] for k in keep], t["f"][keep]


@functools.lru_cache(maxsize=None)
def select_scenario():
    """What the selection can get wrong, on 20 + NGG over three tiles: guide 0 with 150 identical sites in a row across a tile
    end (ties in f, more than 64 in a cell), better and worse sites around them on both strands and sites that meet a zero
    weight; guide 1 with three hits; guide 2 whose hits all stay under the floor; guide 3 with a hit whose only mismatch is at a
    degenerate letter.  K = 5 and FLOOR are the scenario's cut."""
    rng = np.random.default_rng(4242)
    pattern = "N" * 20 + "NGG"
    shape = (23, (0, 20), (21, 22))
    table = random_pattern_table(rng, shape, zeros=0, ones=0)
    table["pair"][:] = 0.25 + 0.5 * table["pair"]  # every weight off the diagonal in (0.25, 0.75)
    for b in range(4):
        table["pair"][:, b, b] = 1.0
    table["pam"][:] = 0.5 + 0.25 * table["pam"]
    table["pam"][4 * 2 + 2] = 1.0                   # GG
    protos = [pc.rnd(rng, 20) for _ in range(4)]
    protos[3] = protos[3][:5] + "R" + protos[3][6:]
    guides = [p + "NNN" for p in protos]
    other = lambda ch: next(b for b in "ACGT" if b != ch)
    table["pair"][7, "ACGT".index(protos[0][7]), "ACGT".index(other(protos[0][7]))] = 0.0  # guide 0's zero weight
    sub = lambda proto, j: proto[:j] + other(proto[j]) + proto[j + 1:]
    site = lambda proto, pam="TGG": proto + pam
    body = list(pc.rnd(rng, 3 * pc.TILE).replace("GG", "GA").replace("CC", "CA"))  # no PAM but the planted ones

    def plant(pos, text, strand=0):
        text = text if strand == 0 else pc.rc(text)
        body[pos:pos + len(text)] = text

    exact = site(protos[0])
    for n in range(150):
        plant(pc.TILE - 70 * 23 + 23 * n, exact)               # the ties, 70 of them in front of the tile end
    plant(100, site(protos[0], "AGG"))                          # another letter at the PAM's N: the same f, one more tie
    plant(200, site(sub(protos[0], 3)))                         # one mismatch: below the ties
    plant(300, site(sub(protos[0], 7)))                         # the zero weight: f = 0
    plant(5000, exact, 1)                                       # '-': ties behind the run in record order
    plant(5100, site(sub(protos[0], 12)), 1)
    plant(5200, site(sub(protos[0], 7)), 1)                     # f = 0 on '-'
    for n, pos in enumerate((400, 5300, 5400)):
        plant(pos, site(sub(protos[1], 2 + n)) if n else site(protos[1]), n % 2)
    for n, pos in enumerate((4200, 4300, 5500)):
        plant(pos, site(sub(sub(sub(protos[2], 1), 9), 15 + n)), n % 2)   # three mismatches each: < 0.75^3
    plant(4400, site(protos[3][:5] + "C" + protos[3][6:]))       # C at the guide's R: NM 1, no pair factor
    contigs = ["".join(body)]
    m = 3
    hits, n_cands = pc.brute_force(contigs, pattern, guides, m)
    f = scored(contigs, guides, hits, table)
    K, FLOOR = 5, int(0.75 ** 3 * ONE) + 1
    s = {"pattern": pattern, "contigs": contigs, "guides": guides, "m": m, "table": table, "hits": hits, "f": f, "K": K, "floor": FLOOR}
    # ---- floors ----
    per = lambda g: [(h, int(v)) for h, v in zip(hits, f) if h[0] == g]
    g0 = per(0)
    ties = [h for h, v in g0 if v == ONE]
    assert len(ties) >= 152 and {h[1] for h in ties} == {0, 1}
    assert max(np.bincount([h[3] // pc.TILE for h in ties if h[1] == 0])) > 64   # more ties in a cell than a wave has lanes
    assert min(h[3] for h in ties) < pc.TILE < max(h[3] for h in ties if h[1] == 0)
    for strand in (0, 1):
        assert any(h[1] == strand and v == 0 for h, v in g0) and any(h[1] == strand and 0 < v < ONE for h, v in g0), strand
    assert len(ties) > K and 0 < len(per(1)) < K                                 # more, and fewer, survivors than K
    assert sum(v >= FLOOR for _, v in per(1)) >= 1
    assert per(2) and all(0 < v < FLOOR for _, v in per(2))                       # hits, none above the floor
    lone = [(h, v) for h, v in per(3) if h[3] == 4400 and h[1] == 0]
    assert lone and lone[0][0][4] == 1 and lone[0][1] == ONE                      # NM 1 at a degenerate letter: no pair factor
    kept = cut(hits, f, top_k=K)
    assert [hits[k] for k in kept if hits[k][0] == 0] == ties[:K]                 # across the K-th place: the FIRST ties
    assert not any(hits[k][0] == 2 for k in cut(hits, f, min_score=FLOOR))
    return s


def make_table(va, table):
    """The library's object of a restated table."""
    return va.PatternTable(table["L"], table["ps"], table["pair"], table["pam_pos"], table["pam"])
