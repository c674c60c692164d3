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
    clean = [pc.genome_of(c) for c in contigs]  # site_text's letters, once per contig
    text = lambda strand, c, p: clean[c][p:p + L] if strand == 0 else pc.rc(clean[c][p:p + L])
    return np.array([py_fixed(py_score(table, guides[g], text(strand, c, p))) for g, strand, c, p, _, _ in hits], dtype=np.uint32)


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


# ---- the radix select digit by digit --------------------------------------------------------------------------------------
# The selection reads a guide's f words as four 8-bit digits from the top and walks the guide's segment 256 records a step.  The
# cases below are searched for on the restatement: shared_digits / segments / threshold_facts describe what a cut (top_k,
# min_score) does to one guide's words, digit_cases picks cuts that reach every digit pass and every step of the walk, and
# digit_floors says which of the conditions a case list does NOT meet - on cut() and the f words alone.
STEP = 256          # records a step of the walk, and the stride of the select's loops
DIGITS_SEED = 7
DIGITS_ZERO_AT = 19  # the protospacer position at which every mismatch weighs 0
MAX_CASES = 48


def shared_digits(a, b):
    """How many of the four bytes, from the top, two different 32-bit values have in common."""
    assert a != b
    return 4 - (((int(a) ^ int(b)).bit_length() + 7) // 8)


def segments(guide_of, n_guides):
    """[begin, end) of every guide's records in a list that is in guide order."""
    guide_of = np.asarray(guide_of, dtype=np.int64)
    assert (np.diff(guide_of) >= 0).all()
    bounds = np.searchsorted(guide_of, np.arange(n_guides + 1))
    return [(int(bounds[g]), int(bounds[g + 1])) for g in range(n_guides)]


def threshold_facts(fg, kept, min_score):
    """One guide's words fg in record order and the mask of those a TRUNCATING cut keeps -> T (the smallest kept value), the
    digits that larger and smaller survivor values (f >= min_score) share with T, and the ties (f = T) kept and dropped, as
    indices into the segment."""
    fg = np.asarray(fg, dtype=np.int64)
    T = int(fg[kept].min())
    values = set(fg[fg >= min_score].tolist())
    ties = np.nonzero(fg == T)[0]
    return {"T": T, "larger": {shared_digits(T, v) for v in values if v > T}, "smaller": {shared_digits(T, v) for v in values if v < T},
            "kept_ties": [int(i) for i in ties if kept[i]], "dropped_ties": [int(i) for i in ties if not kept[i]]}


def case_facts(guide_of, f, n_guides, keep, top_k, min_score):
    """{guide: threshold_facts} of the guides that the cut (top_k, min_score) truncates - more survivors than top_k.  keep: the
    indices cut() returns."""
    f = np.asarray(f, dtype=np.int64)
    kept = np.zeros(len(f), dtype=bool)
    kept[keep] = True
    out = {}
    for g, (b, e) in enumerate(segments(guide_of, n_guides)):
        if top_k and int((f[b:e] >= min_score).sum()) > top_k:
            assert int(kept[b:e].sum()) == top_k
            out[g] = threshold_facts(f[b:e], kept[b:e], min_score)
    return out


def spread_ties(t):
    """A truncated guide's ties are kept and dropped, lie in two steps of the walk or more, a kept one behind the first step that
    holds ties (the running count of ties decides it), and a dropped one in a later step than the last kept one."""
    if not t["kept_ties"] or not t["dropped_ties"]:
        return False
    steps = {i // STEP for i in t["kept_ties"] + t["dropped_ties"]}
    last_kept = t["kept_ties"][-1] // STEP
    return len(steps) >= 2 and last_kept > min(steps) and t["dropped_ties"][-1] // STEP > last_kept


def digit_cases(guide_of, f, n_guides):
    """[(top_k, min_score, what the case is there for)]: a search over the restatement, in a fixed order - per guide with more
    than one step of records, the smallest top_k (at min_score = 0) that reaches a condition."""
    f = np.asarray(f, dtype=np.int64)
    segs = segments(guide_of, n_guides)
    cases = []

    def add(top_k, min_score, why):
        at = [n for n, c in enumerate(cases) if c[:2] == (top_k, min_score)]
        if at:
            cases[at[0]] = cases[at[0]][:2] + (cases[at[0]][2] + "; " + why,)
        elif len(cases) < MAX_CASES:
            cases.append((int(top_k), int(min_score), why))

    long_ones = [g for g, (b, e) in enumerate(segs) if e - b > STEP]
    for g in long_ones:
        n = segs[g][1] - segs[g][0]
        for k in (1, STEP - 1, STEP, STEP + 1, n, n + 1):
            add(k, 0, "top_k = %d (guide %d has %d records)" % (k, g, n))
    for g in long_ones:
        b, e = segs[g]
        fg, n = f[b:e], e - b
        order = np.lexsort((np.arange(n), -fg))  # f descending, then record order: the ranking
        found = {}
        for k in range(1, n):
            kept = np.zeros(n, dtype=bool)
            kept[order[:k]] = True
            t = threshold_facts(fg, kept, 0)
            for d in t["larger"]:
                found.setdefault(("larger", d), k)
            for d in t["smaller"]:
                found.setdefault(("smaller", d), k)
            if 3 in t["larger"] and 3 in t["smaller"]:
                found.setdefault(("both", 3), k)
            if spread_ties(t):
                found.setdefault(("ties", t["T"]), k)  # (one case per tied value)
        tied = sorted((key[1] for key in found if key[0] == "ties"), key=lambda T: (-int((fg == T).sum()), T))[:3]  # the longest tie runs
        for (kind, d), k in sorted(found.items()):
            if kind == "ties" and d not in tied:
                continue
            why = {"larger": "a larger value shares %d digits with T" % d, "smaller": "a smaller value shares %d digits with T" % d,
                   "both": "larger and smaller values share 3 digits with T", "ties": "ties at %#x kept and dropped over several steps" % d}[kind]
            add(k, 0, "%s (guide %d)" % (why, g))
            if kind == "ties" and d == tied[0]:
                add(k, d, "min_score = T of (%d, 0) on guide %d" % (k, g))
                add(k, d + 1, "min_score = T + 1 of (%d, 0) on guide %d" % (k, g))
                add(int((fg >= d).sum()) - 1, 0, "every tie at %#x but the last one kept (guide %d)" % (d, g))
        positive = int((fg > 0).sum())
        if 0 < positive < n - 1:
            add(positive + (n - positive + 1) // 2, 0, "T = 0: some of guide %d's f = 0 records are taken" % g)
        values = np.unique(fg)
        pairs = [(int(lo), int(hi)) for lo, hi in zip(values[:-1], values[1:]) if hi - lo >= 2 and shared_digits(lo, hi) == 3]
        if pairs:
            lo, hi = pairs[len(pairs) // 2]
            add(0, lo + 1, "the floor between %#x and %#x of guide %d: three digits shared" % (lo, hi, g))
            add(max(int((fg > lo).sum()) // 2, 1), lo + 1, "the same floor with a top_k that truncates guide %d" % g)
    return cases


def digit_floors(hits_guides, f, n_guides, cases, cut_of):
    """The names of the conditions that the case list does NOT meet (empty: all met).  cut_of(top_k, min_score) -> kept indices:
    the restatement's cut(); everything else is read off the f words."""
    f = np.asarray(f, dtype=np.int64)
    segs = segments(hits_guides, n_guides)
    lens = [e - b for b, e in segs]
    met, ks = set(), set()
    plain_T = {}
    pairs = [(int(c[0]), int(c[1])) for c in cases]
    for top_k, min_score in pairs:
        ks.add(top_k)
        for g, t in case_facts(hits_guides, f, n_guides, cut_of(top_k, min_score), top_k, min_score).items():
            for d in t["larger"]:
                met.add("larger %d" % d)
            for d in t["smaller"]:
                met.add("smaller %d" % d)
            if 3 in t["larger"] and 3 in t["smaller"]:
                met.add("both 3")
            if spread_ties(t):
                met.add("ties over steps")
            if t["T"] == 0 and min_score == 0 and t["kept_ties"] and t["dropped_ties"]:
                met.add("T = 0")
            if min_score == 0:
                plain_T.setdefault(top_k, set()).add(t["T"])
    for top_k, min_score in pairs:
        if min_score and min_score in plain_T.get(top_k, ()):
            met.add("min_score = T")
        if min_score and min_score - 1 in plain_T.get(top_k, ()):
            met.add("min_score = T + 1")
        for b, e in segs:
            values = np.unique(f[b:e])
            at = int(np.searchsorted(values, min_score))
            if 0 < at < len(values) and values[at] > min_score and shared_digits(values[at - 1], values[at]) == 3:
                met.add("floor between")  # values[at - 1] < min_score < values[at]
    if any(n > 2 * STEP for n in lens) and any(STEP < n < 2 * STEP for n in lens):
        met.add("two and three steps")
    if any(lens[g] == 0 and any(lens[:g]) and any(lens[g + 1:]) for g in range(n_guides)):
        met.add("empty segment")
    if {1, STEP - 1, STEP, STEP + 1} <= ks and any(n > STEP and {n, n + 1} <= ks for n in lens):
        met.add("top_k values")
    want = ["larger %d" % d for d in range(4)] + ["smaller %d" % d for d in range(4)] + \
           ["both 3", "ties over steps", "T = 0", "floor between", "min_score = T", "min_score = T + 1", "two and three steps",
            "empty segment", "top_k values"]
    return [name for name in want if name not in met] + (["at most %d cases" % MAX_CASES] if len(cases) > MAX_CASES else [])


def digits_table():
    """20 N + NGG with dyadic weights: 1 - 2^-e, e = min(1 + i + 10 k, 29) for position i and the k-th of the three bases that
    are not the guide's - each exact in a double, so a product of up to three lands on f words that agree with their neighbours'
    in the top one, two or three bytes and differ below.  Every mismatch at DIGITS_ZERO_AT weighs 0; every PAM weight is 1."""
    pair = np.ones((20, 4, 4))
    for i in range(20):
        for g in range(4):
            for k, s in enumerate(b for b in range(4) if b != g):
                pair[i, g, s] = 0.0 if i == DIGITS_ZERO_AT else 1.0 - 2.0 ** -min(1 + i + 10 * k, 29)
    return {"L": 23, "ps": (0, 20), "pam_pos": (21, 22), "pair": pair, "pam": np.ones(16)}


def _no_candidates(text):
    """No GG and no CC: no NGG site on either strand."""
    return text.replace("GG", "GA").replace("CC", "CA")


def _digits_genome(rng, protos, counts):
    """One planted site every 26 bases (23 + ATA) in shuffled order and on alternating strands: counts[g] sites of guide g with
    0 to 3 substitutions each, every second one of guide 0 one and the same one-mismatch site."""
    def mutated(proto, n):
        s = list(proto)
        for j in rng.choice(20, size=n, replace=False):
            s[int(j)] = [b for b in "ACGT" if b != proto[int(j)]][int(rng.integers(3))]
        return "".join(s)

    j, base = 5, [b for b in "ACGT" if b != protos[0][5]][2]  # e = 26: f = 2^30 - 16, no digit of it decides alone
    common = protos[0][:j] + base + protos[0][j + 1:] + "TGG"
    planted = []
    for g, n in enumerate(counts):
        for k in range(n):
            planted.append(common if g == 0 and k % 2 == 0 else mutated(protos[g], int(rng.integers(0, 4))) + "ACGT"[int(rng.integers(4))] + "GG")
    order = rng.permutation(len(planted))
    slots = [(planted[int(k)] if n % 2 == 0 else pc.rc(planted[int(k)])) + "ATA" for n, k in enumerate(order)]
    return _no_candidates(pc.rnd(rng, 50)) + "".join(slots) + _no_candidates(pc.rnd(rng, 50))


@functools.lru_cache(maxsize=None)
def digits_scenario():
    """What the four digit passes and the walk's running counts can get wrong, on 20 + NGG, m = 3: four guides with about 700,
    300, 0 and 40 records whose f values agree in their top one, two or three bytes and differ below, ties spread over three
    steps, f = 0 records - and the cuts ("cases") that digit_cases finds on them.  The floors are digit_floors'."""
    rng = np.random.default_rng(DIGITS_SEED)
    pattern, m = "N" * 20 + "NGG", 3
    table = digits_table()
    protos = [pc.rnd(rng, 20) for _ in range(4)]
    guides = [p + "NNN" for p in protos]
    contigs = [_digits_genome(rng, protos, (700, 300, 0, 40))]
    hits, n_cands = pc.brute_force(contigs, pattern, guides, m)
    f = scored(contigs, guides, hits, table)
    guide_of = [h[0] for h in hits]
    found = digit_cases(guide_of, f, 4)
    s = {"pattern": pattern, "contigs": contigs, "guides": guides, "m": m, "table": table, "hits": hits, "f": f,
         "cases": [c[:2] for c in found], "serves": [c[2] for c in found]}
    unmet = digit_floors(guide_of, f, 4, s["cases"], lambda k, ms: cut(hits, f, k, ms))
    assert not unmet, unmet
    return s


WIDE_TILES = 36
WIDE_AT = {59: 1, 60: 0, 61: 2, 62: 3, 64: 0, 65: 3, 3: 3}  # index among the 66 guides -> guide of digits_scenario


@functools.lru_cache(maxsize=None)
def digits_wide():
    """digits_scenario's table and planted sites on a contig of more than WIDE_TILES tiles and among 66 guides: at guide_batch =
    64 a round has 2 x 64 x n_tiles > 4096 cells, that is two groups of 64 x 64, and the segments of guides 59 to 62 begin in
    the second one; guides 64 and 65 are the second round."""
    d = digits_scenario()
    rng = np.random.default_rng(DIGITS_SEED + 1)
    body = d["contigs"][0]
    contigs = [body + _no_candidates(pc.rnd(rng, WIDE_TILES * pc.TILE + 100 - len(body)))]
    guides = [pc.rnd(rng, 20) + "NNN" for _ in range(66)]
    for at, g in WIDE_AT.items():
        guides[at] = d["guides"][g]
    hits, n_cands = pc.brute_force(contigs, d["pattern"], guides, d["m"])
    f = scored(contigs, guides, hits, d["table"])
    guide_of = [h[0] for h in hits]
    segs = segments(guide_of, 66)
    n = segs[60][1] - segs[60][0]
    small_of = [h[0] for h in d["hits"]]
    inside_ties = lambda c: any(spread_ties(t) and t["T"] & 0xFFFFFF for t in case_facts(small_of, d["f"], 4, cut(d["hits"], d["f"], *c), *c).values())
    tie_case = next(c for c in d["cases"] if c[1] == 0 and inside_ties(c))       # the cut falls inside ties whose low digits are not 0
    between = next(c for c in d["cases"] if c[0] and c[1] and (0, c[1]) in d["cases"])  # a floor between two near values, and a top_k
    cases = [tie_case, (1, 0), (STEP + 1, 0), (n, 0), (0, between[1]), between]
    s = {"pattern": d["pattern"], "contigs": contigs, "guides": guides, "m": d["m"], "table": d["table"], "hits": hits, "f": f, "cases": cases}
    # ---- floors ----
    n_tiles = len(contigs[0]) // pc.TILE  # (whole tiles: the device counts no fewer)
    assert 2 * 64 * n_tiles > 4096
    beyond = [g for g in range(64) if 2 * g * n_tiles >= 4096 and segs[g][1] > segs[g][0]]
    assert len(beyond) >= 2 and min(beyond) >= 32, beyond
    for at, g in WIDE_AT.items():  # the same records as in the small scenario, guide by guide
        b, e = segs[at]
        mine = [h[1:] for h in d["hits"] if h[0] == g]
        assert [h[1:] for h in hits[b:e]] == mine and (f[b:e] == d["f"][[k for k, h in enumerate(d["hits"]) if h[0] == g]]).all(), at
    t = case_facts(guide_of, f, 66, cut(hits, f, *tie_case), *tie_case)
    assert any(g in t and spread_ties(t[g]) for g in beyond)               # a guide of the second group truncates inside its ties
    for k, ms in cases:
        assert {64, 65} <= {hits[i][0] for i in cut(hits, f, k, ms)}, (k, ms)  # the second round keeps records of its own
    return s


def make_table(va, table):
    """The library's object of a restated table."""
    return va.PatternTable(table["L"], table["ps"], table["pair"], table["pam_pos"], table["pam"])
