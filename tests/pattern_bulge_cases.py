"""Bulges under a pattern: the definition (include/varscot_hip.h, vsc_search_pattern_bulges) restated in plain Python, and the
scenarios the tests run it on.  Nothing here calls the library: nm_at() / best() are the definition for one guide and one site,
candidates() is conditions 1 to 3 site by site, brute_force() applies condition 4 to the sites of one class at a time with
numpy, and every scenario asserts floors on the restatement's OWN output, so that no edge it is built for is missing from it."""
import functools

import numpy as np

from pattern_cases import IUPAC, TILE, _codes, _set_bits, genome_of, make_site, put, rc, rnd

CLASSES = (-2, -1, 1, 2)  # ascending d: the row order of vsc_bulge_summary
HIT_DTYPE = np.dtype([("guide", "<u4"), ("contig", "<u4"), ("pos", "<u4"), ("info", "<u4")])
PRESETS = {"SaCas9": ("N" * 21 + "NNGRRT", (0, 21)), "Cas12a": ("TTTV" + "N" * 23, (4, 23))}


def enabled(dna, rna):
    return [d for d in CLASSES if (d > 0 and d <= dna) or (d < 0 and -d <= rna)]


def indices(proto, d):
    """The split points of class d: a+1 .. e-1 (DNA), a+1 .. e-1-b (RNA)."""
    a, e = proto[0], proto[0] + proto[1]
    return range(a + 1, (e - 1 if d > 0 else e - 1 + d) + 1)


def refused(pattern, proto, dna, rna):
    """REFUSED of the definition (beyond what the pattern search refuses)."""
    L, (a, n) = len(pattern), proto
    return (not (0 <= dna <= 2 and 0 <= rna <= 2 and dna + rna > 0) or n < 4 or a + n > L or any(ch not in "Nn" for ch in pattern[a:a + n])
            or L + dna > 32 or L - rna < 16)


def bulged_pattern(pattern, proto, d):
    a, e = proto[0], proto[0] + proto[1]
    return pattern[:a] + "N" * (proto[1] + d) + pattern[e:]


def nm_at(guide, s, proto, d, i):
    """nm(i) of the definition: guide of L IUPAC letters, s a site of L + d letters in read orientation."""
    L, G = len(guide), [IUPAC[ch] for ch in guide.upper()]
    if d > 0:
        return sum(s[j] not in G[j] for j in range(i)) + sum(s[j + d] not in G[j] for j in range(i, L))
    b = -d
    return sum(s[j] not in G[j] for j in range(i)) + sum(s[j - b] not in G[j] for j in range(i + b, L))


def best(guide, s, proto, d):
    """(NM, index, tie): the minimum of nm(i), the smallest i that reaches it, and whether a larger i reaches it too."""
    assert len(s) == len(guide) + d and d in CLASSES
    idx = list(indices(proto, d))
    all_nm = [nm_at(guide, s.upper(), proto, d, i) for i in idx]
    nm = min(all_nm)
    return nm, idx[all_nm.index(nm)], all_nm.count(nm) > 1


def fits(pattern, proto, s, d):
    """Conditions 2 and 3 for a site in read orientation (d = 0: the plain pattern)."""
    bp = bulged_pattern(pattern, proto, d).upper()
    return len(s) == len(bp) and all(ch in "ACGT" for ch in s) and all(s[j] in IUPAC[bp[j]] for j in range(len(s)))


def candidates(contigs, pattern, proto, dna, rna, classes=None):
    """Every (strand, contig, pos, d, s): conditions 1 to 3 of the definition, s in read orientation.  numpy finds the windows
    of a class that hold no N and satisfy the bulged pattern; fits() is asserted on each."""
    out = []
    for d in (enabled(dna, rna) if classes is None else classes):
        n = len(pattern) + d
        P = _set_bits(bulged_pattern(pattern, proto, d))
        for c, raw in enumerate(contigs):
            seq, text = _codes(raw), genome_of(raw)
            if len(seq) < n:
                continue
            W = np.lib.stride_tricks.sliding_window_view(seq, n)
            clean = np.nonzero((W < 4).all(1))[0]
            for strand in (0, 1):
                S = W[clean] if strand == 0 else 3 - W[clean][:, ::-1]
                for p in clean[((P[None, :] >> S) & 1).all(1)]:
                    w = text[p:p + n]
                    s = w if strand == 0 else rc(w)
                    assert fits(pattern, proto, s, d)
                    out.append((strand, c, int(p), d, s))
    return out


def brute_force(contigs, pattern, guides, proto, m, dna, rna, cands=None):
    """The hits as (guide, strand, contig, pos, d, nm, index, tie) in ascending (guide, strand, contig, pos, d) order, and the
    number of candidates.  Condition 4 for all sites of one class at a time: nm(i) exactly as nm_at writes it, with numpy sums."""
    cands = candidates(contigs, pattern, proto, dna, rna) if cands is None else cands
    L = len(pattern)
    hits = []
    for d in enabled(dna, rna):
        sub = [x for x in cands if x[3] == d]
        if not sub:
            continue
        S = np.stack([_codes(x[4]) for x in sub])  # [n, L + d]
        idx = list(indices(proto, d))
        for g, text in enumerate(guides):
            G = _set_bits(text)
            wrong = lambda cols, js: (((G[js][None, :] >> S[:, cols]) & 1) == 0).sum(1)  # site columns against guide positions
            rows = []
            for i in idx:
                front = wrong(np.arange(0, i), np.arange(0, i))
                js = np.arange(i, L) if d > 0 else np.arange(i - d, L)
                rows.append(front + wrong(js + d, js))
            A = np.stack(rows)  # [split point, site]
            nm_min, first, ties = A.min(0), A.argmin(0), (A == A.min(0)).sum(0) > 1
            for k in np.nonzero(nm_min <= m)[0]:
                strand, c, p, _, _ = sub[k]
                hits.append((g, strand, c, p, d, int(nm_min[k]), idx[int(first[k])], bool(ties[k])))
    hits.sort(key=lambda h: h[:5])
    return hits, len(cands)


def info_word(strand, d, index, nm):
    return strand << 31 | (1 if d < 0 else 0) << 12 | abs(d) << 10 | index << 5 | nm


def arrays(hits, n_guides):
    """(records, rows) as vsc_search_pattern_bulges returns them."""
    rec = np.zeros(len(hits), dtype=HIT_DTYPE)
    rows = np.zeros((n_guides, 4, 9), dtype=np.uint32)
    for k, (g, strand, c, p, d, nm, index, _) in enumerate(hits):
        rec[k] = (g, c, p, info_word(strand, d, index, nm))
        rows[g, CLASSES.index(d), nm] += 1
    return rec, rows


def d_of_info(info):
    info = np.asarray(info, dtype=np.uint32)
    size = ((info >> 10) & 3).astype(np.int64)
    return np.where((info >> 12) & 1 == 1, -size, size)


def merge_order(rec):
    """The indices that put records into ascending (guide, strand, contig, pos, d) order."""
    return np.lexsort((d_of_info(rec["info"]), rec["pos"], rec["contig"], rec["info"] >> 31, rec["guide"]))


# ---- scenarios ------------------------------------------------------------------------------------------------------------
def distinct_guide(rng, pattern, proto, pam=""):
    """A guide whose protospacer has no equal letters at distance 1 or 2 (a planted bulge then has one best split point) and
    whose other positions are N, or the letters of `pam` in turn."""
    a, n = proto
    p, pam, out = [], list(pam), []
    for _ in range(n):
        p.append(next(str(x) for x in rng.permutation(list("ACGT")) if x not in p[-2:]))
    for j in range(len(pattern)):
        out.append(p[j - a] if a <= j < a + n else (pam.pop(0) if pam else "N"))
    return "".join(out)


def plant(rng, pattern, guide, proto, d, i, subs=(), bulge=None):
    """A site of L + d letters in read orientation that satisfies the bulged pattern and pairs with `guide` at split point i
    with the substitutions `subs`: a DNA bulge inserts `bulge` (default: letters that differ from both neighbours, so that no
    other i pairs as well), an RNA bulge drops site positions [i, i - d)."""
    r = make_site(rng, pattern, guide, set(int(j) for j in subs))
    if d > 0:
        if bulge is None:
            bulge = ""
            for _ in range(d):
                bulge += next(x for x in "ACGT" if x not in (r[i - 1], r[i], bulge[-1:] or "-"))
        assert len(bulge) == d
        return r[:i] + bulge + r[i:]
    return r[:i] + r[i - d:]


def _build(seed, pattern, proto, dna, rna, m):
    rng = np.random.default_rng(seed)
    L, (a, n) = len(pattern), proto
    e = a + n
    assert not refused(pattern, proto, dna, rna)
    classes = enabled(dna, rna)
    g0 = distinct_guide(rng, pattern, proto)                                                    # N at the PAM positions
    sample = make_site(rng, pattern, g0)
    g1 = distinct_guide(rng, pattern, proto, [sample[j] for j in range(L) if not a <= j < e])  # a spelled PAM: its letters count
    g2 = list(distinct_guide(rng, pattern, proto))
    for k, letter in ((a + 1, "R"), (a + 3, "Y"), (e - 2, "B")):
        g2[k] = next(x for x in (letter, "N") if g2[k] in IUPAC[x])                             # degenerate protospacer letters
    g2 = "".join(g2)
    g3 = list(distinct_guide(rng, pattern, proto))
    g3[a + n // 2] = "N"                                                                        # N inside the protospacer
    g3 = "".join(g3)
    # both strands at one start: w pairs with g4 on '+' (DNA 1 / RNA 1 at a + 3) and its reverse complement with g5 on '-' (at a + 5)
    d_both = 1 if 1 in classes else -1
    bp = bulged_pattern(pattern, proto, d_both)
    w = "".join(next(x for x in rng.permutation(list("ACGT")) if x in IUPAC[p] and rc(x) in IUPAC[q]) for p, q in zip(bp, reversed(bp)))
    assert fits(pattern, proto, w, d_both) and fits(pattern, proto, rc(w), d_both)
    unbulge = lambda s, i: s[:i] + s[i + 1:] if d_both > 0 else s[:i] + ("C" if s[i] != "C" else "G") + s[i:]
    as_guide = lambda s: "".join(ch if a <= j < e else "N" for j, ch in enumerate(s))
    g4, g5 = as_guide(unbulge(w, a + 3)), as_guide(unbulge(rc(w), a + 5))
    guides = [g0, g1, g2, g3, g4, g5, g0.lower()[:L - 1] + g0[L - 1]]

    planted = []  # (strand, site on the forward genome): every class and strand with 0 .. m substitutions, the split point in turn
    for d in classes:
        idx = list(indices(proto, d))
        for strand in (0, 1):
            for k in range(m + 1):
                i = (idx[0], idx[-1], idx[len(idx) // 2])[(k + strand) % 3]
                free = [j for j in range(a, e) if j < i - 2 or j > i + 3]  # (not beside or in the bulge)
                site = plant(rng, pattern, g0, proto, d, i, rng.choice(free, size=k, replace=False))
                planted.append((strand, site if strand == 0 else rc(site)))
        for i in (idx[0], idx[-1]):  # the smallest and the largest split point without substitutions, once more
            planted.append((0, plant(rng, pattern, g0, proto, d, i)))
    for g in (g1, g2, g3):  # the other kinds of guide: the largest class on '+', the smallest on '-'
        planted.append((0, plant(rng, pattern, g, proto, classes[-1], a + 6)))
        planted.append((1, rc(plant(rng, pattern, g, proto, classes[0], a + 2))))
    order = [int(x) for x in rng.permutation(len(planted))]
    take = lambda strand: planted[order.pop(next(k for k, x in enumerate(order) if planted[x][0] == strand))][1]
    body = rnd(rng, 3 * TILE)
    # p = 0; across the first tile end on '+' and the second on '-'; then one site every 67 bases (many cross a 32-base word)
    body = put(body, 0, take(0))
    body = put(body, TILE - 10, take(0))
    body = put(body, 2 * TILE - 13, take(1))
    slots = [100 + 67 * k for k in range(75) if not any(abs(100 + 67 * k - q) < 80 for q in (TILE, 2 * TILE))]
    assert len(slots) >= len(order) and slots[len(order) - 1] < 5000
    for pos in slots[:len(order)]:
        body = put(body, pos, planted[order.pop()][1])
    d1, i1 = classes[-1], a + 5  # the largest DNA bulge, for the single cases below
    assert d1 > 0
    exact = plant(rng, pattern, g0, proto, d1, i1)
    body = put(body, 5100, w)
    # a tie: the inserted bases repeat their left neighbour, so split points i1 - 1 and i1 pair alike and the smaller is
    # reported - on either strand
    r = make_site(rng, pattern, g0)
    tie_site = r[:i1] + r[i1 - 1] * d1 + r[i1:]
    body = put(body, 5200, tie_site)
    body = put(body, 5270, rc(tie_site))
    # an N at an unpaired base and an IUPAC letter inside a site: absent; lower-case sites: present
    body = put(body, 5340, exact[:i1] + "N" + exact[i1 + 1:])
    body = put(body, 5410, exact[:a + 2] + "R" + exact[a + 3:])
    body = put(body, 5480, exact.lower())
    body = put(body, 5550, rc(exact).lower())
    body = put(body, 5727, exact)                # starts at bit 31 of a word
    body = body[:len(body) - len(exact)] + exact  # p + L + d == len(c)
    left, right = rnd(rng, 150) + exact[:L // 2], exact[L // 2:] + rnd(rng, 150)  # a would-be site across two contigs
    small = []  # contigs of L - 3 .. L + 2 bases: each a site of its own length where a class has that length
    for k in range(-3, 3):
        small.append(plant(rng, pattern, g0, proto, k, list(indices(proto, k))[1]) if k in classes else rnd(rng, L + k))
    assert [len(s) for s in small] == list(range(L - 3, L + 3))
    contigs = [body, left, right] + small + [rnd(rng, 300)]
    assert sum(len(c) for c in contigs) < 8000

    cands = candidates(contigs, pattern, proto, dna, rna)
    hits, n_cands = brute_force(contigs, pattern, guides, proto, m, dna, rna, cands=cands)
    # ---- floors ----
    size = lambda h: L + h[4]
    for d in classes:
        idx = list(indices(proto, d))
        for strand in (0, 1):
            mine = [h for h in hits if h[4] == d and h[1] == strand]
            assert {h[5] for h in mine} == set(range(m + 1)), (d, strand)                 # every class, strand and NM
        assert {idx[0], idx[-1]} <= {h[6] for h in hits if h[4] == d}, d                  # the smallest and the largest split point
    for strand, pos in ((0, 5200), (1, 5270)):                                            # the tie, resolved downwards
        t = [h for h in hits if h[0] == 0 and h[1:5] == (strand, 0, pos, d1)]
        assert t and t[0][7] and t[0][6] == i1 - 1 and t[0][5] == 0, (strand, t)
    assert any(h[2] == 0 and h[3] == 0 for h in hits)                                     # p = 0
    assert any(h[2] == 0 and h[3] + size(h) == len(body) and h[5] == 0 for h in hits)     # p + L + d == len(c)
    for s in (0, 1):
        assert any(h[1] == s and h[2] == 0 and h[3] < (1 + s) * TILE < h[3] + size(h) for h in hits), s  # across a tile end
        assert any(h[1] == s and h[2] == 0 and h[3] // 32 != (h[3] + size(h) - 1) // 32 for h in hits), s  # across a word end
    assert 5727 % 32 == 31 and any(h[:5] == (0, 0, 0, 5727, d1) and h[5] == 0 for h in hits)  # a start at bit 31
    assert any(h[:5] == (4, 0, 0, 5100, d_both) and h[5] == 0 for h in hits)              # both strands at one start
    assert any(h[:5] == (5, 1, 0, 5100, d_both) and h[5] == 0 for h in hits)
    assert not any(h[2] == 0 and h[3] in (5340, 5410) and h[0] == 0 and h[5] <= 1 for h in hits)  # N / IUPAC in the site
    assert not any(x[1] == 0 and x[2] == 5340 and x[3] == d1 for x in cands)
    assert any(h[:5] == (0, 0, 0, 5480, d1) and h[5] == 0 for h in hits)                  # lower case in the genome
    assert any(h[:5] == (0, 1, 0, 5550, d1) and h[5] == 0 for h in hits)
    assert not any(h[0] == 0 and h[2] in (1, 2) and h[5] == 0 for h in hits)              # the site across two contigs
    for k in range(-3, 3):                                                                # contigs that are one site
        here = [h for h in hits if h[2] == 3 + (k + 3)]
        assert all(h[4] <= k for h in here)
        assert (k in classes) == any(h[3] == 0 and h[4] == k and h[5] == 0 and h[0] == 0 for h in here), k
    assert not any(h[2] == 3 for h in hits)                                               # a contig too short for any site
    by_guide = lambda g: [h for h in hits if h[0] == g]
    assert any(h[5] == 0 for h in by_guide(2)) and any(h[5] == 0 for h in by_guide(3))    # degenerate letters, N in the protospacer
    both = {h[1:5]: h[5] for h in by_guide(0)}                                            # the spelled PAM counts
    assert by_guide(1) and {h[1] for h in by_guide(1)} == {0, 1}
    assert [h[1:] for h in by_guide(6)] == [h[1:] for h in by_guide(0)]                   # a lower-case guide
    # a site that fits the pattern at d = 0 but not at d = +1 (or, without DNA bulges, -1), and the converse - both N-free
    dd = 1 if 1 in classes else -1
    plain = {x[:3] for x in candidates(contigs, pattern, proto, 0, 0, classes=[0])}
    bulged = {x[:3] for x in cands if x[3] == dd}
    whole = lambda strand, c, p: p + L + max(dd, 0) <= len(contigs[c]) and "N" not in genome_of(contigs[c][p:p + L + max(dd, 0)])
    assert any(whole(*x) for x in plain - bulged) and any(whole(*x) for x in bulged - plain)
    return {"pattern": pattern, "proto": proto, "dna": dna, "rna": rna, "m": m, "contigs": contigs, "guides": guides, "cands": cands,
            "hits": hits, "n_cands": n_cands}


EDGE_M = 4


@functools.lru_cache(maxsize=None)
def edge_scenario(preset):
    """Contigs, guides and the restatement's hits at m = 4, dna = rna = 2 for SaCas9 / Cas12a - with the edge cases of the
    search's front end and floors on the hits (asserted in _build)."""
    pattern, proto = PRESETS[preset]
    return _build(3000 + sorted(PRESETS).index(preset), pattern, proto, 2, 2, EDGE_M)


LIMITS = {16: ("N" * 13 + "RRT", (0, 13), 2, 0), 18: ("TTV" + "N" * 15, (3, 15), 2, 2), 30: ("N" * 24 + "NNGRRT", (0, 24), 2, 2)}


@functools.lru_cache(maxsize=None)
def limit_scenario(L):
    """The edge layout at the refusal limits: L = 16 with DNA bulges only and L = 18 with RNA 2 (L - rna_max = 16), L = 30 with
    DNA 2 (L + dna_max = 32)."""
    pattern, proto, dna, rna = LIMITS[L]
    assert len(pattern) == L and (L - rna == 16 or L + dna == 32)
    return _build(4000 + L, pattern, proto, dna, rna, 3)


def hits_at(e, m, dna=2, rna=2, guides=None):
    """The scenario's hits under a smaller budget, fewer classes or the first `guides` guides."""
    return [h for h in e["hits"] if h[5] <= m and h[4] in enabled(dna, rna) and (guides is None or h[0] < guides)]


def cands_at(e, dna, rna):
    return sum(1 for x in e["cands"] if x[3] in enabled(dna, rna))


@functools.lru_cache(maxsize=None)
def many_guides_scenario():
    """70 guides - two rounds at guide_batch = 64 - on the SaCas9 edge genome, m = 3, dna = rna = 1."""
    e = edge_scenario("SaCas9")
    rng = np.random.default_rng(78)
    guides = list(e["guides"]) + [distinct_guide(rng, e["pattern"], e["proto"]) for _ in range(70 - len(e["guides"]))]
    guides[66], guides[69] = e["guides"][0], e["guides"][2]  # the second round has records of its own
    hits, n_cands = brute_force(e["contigs"], e["pattern"], guides, e["proto"], 3, 1, 1)
    assert len(guides) == 70 and {66, 69} <= {h[0] for h in hits}
    return {"pattern": e["pattern"], "proto": e["proto"], "contigs": e["contigs"], "guides": guides, "hits": hits, "n_cands": n_cands,
            "m": 3, "dna": 1, "rna": 1}


@functools.lru_cache(maxsize=None)
def tandem_scenario():
    """One 28-base SaCas9 site (a DNA bulge of 1 for the guide), 210 copies back to back across two tile ends."""
    rng = np.random.default_rng(20263)
    pattern, proto = PRESETS["SaCas9"]
    guide = distinct_guide(rng, pattern, proto)
    site = plant(rng, pattern, guide, proto, 1, 11)
    contigs = [rnd(rng, 1000) + site * 210 + rnd(rng, 400)]
    guides = [guide, distinct_guide(rng, pattern, proto)]
    hits, n_cands = brute_force(contigs, pattern, guides, proto, 3, 1, 1)
    copies = [h for h in hits if h[0] == 0 and h[1] == 0 and h[4] == 1 and h[5] == 0]
    assert len(copies) >= 200
    assert min(h[3] for h in copies) < TILE < 2 * TILE < max(h[3] for h in copies)
    assert max(np.bincount([h[3] // 32 for h in hits if h[0] == 0])) >= 2  # more than one hit in a lane's 32 starts
    assert max(np.bincount([h[3] // TILE for h in copies])) > 64            # more hits in a cell than a wave has lanes
    return {"pattern": pattern, "proto": proto, "contigs": contigs, "guides": guides, "hits": hits, "n_cands": n_cands, "m": 3,
            "dna": 1, "rna": 1}


@functools.lru_cache(maxsize=None)
def all_n_scenario():
    """A pattern of N only with four classes: every start of a tile is a candidate of every class on both strands - 4 x 2 048
    queue entries per strand and tile, four windows of the queue."""
    rng = np.random.default_rng(20264)
    pattern, proto = "N" * 23, (0, 23)
    g = [distinct_guide(rng, pattern, proto) for _ in range(3)]
    contigs = [rnd(rng, 2600), rnd(rng, 700)]
    for k, (d, strand, pos) in enumerate(((1, 0, 300), (-2, 1, 900), (2, 0, 2040), (-1, 1, 2300), (2, 1, 1500))):
        site = plant(rng, pattern, g[k % 3], proto, d, 5 + 3 * k, (1, 20)[:k % 3])
        contigs[0] = put(contigs[0], pos, site if strand == 0 else rc(site))
    hits, n_cands = brute_force(contigs, pattern, g, proto, 3, 2, 2)
    assert n_cands > 4 * 2 * 3000 and {h[4] for h in hits} == set(CLASSES) and {h[1] for h in hits} == {0, 1}
    assert any(h[3] < TILE < h[3] + 23 + h[4] for h in hits)
    return {"pattern": pattern, "proto": proto, "contigs": contigs, "guides": g, "hits": hits, "n_cands": n_cands, "m": 3, "dna": 2, "rna": 2}
