"""The pattern search's definition (include/varscot_hip.h, vsc_search_pattern) restated in plain Python, and the scenarios
the tests run it on.  Nothing here calls the library: site_match() is the definition for one pattern, one guide and one site,
definition() applies it site by site, brute_force() is the same over all starts with numpy, and every scenario asserts floors
on the restatement's OWN output, so that no edge it is built for is missing from it."""
import functools

import numpy as np

TILE = 2048
MAX_M = 8
IUPAC = {"A": "A", "C": "C", "G": "G", "T": "T", "R": "AG", "Y": "CT", "S": "CG", "W": "AT", "K": "GT", "M": "AC",
         "B": "CGT", "D": "AGT", "H": "ACT", "V": "ACG", "N": "ACGT"}
COMP = str.maketrans("ACGTN", "TGCAN")
HIT_DTYPE = np.dtype([("guide", "<u4"), ("contig", "<u4"), ("pos", "<u4"), ("info", "<u4"), ("mask", "<u4")])


def rc(s):
    return s.translate(COMP)[::-1]


def comp_letter(ch):
    """The letter of the complemented set."""
    want = "".join(sorted(b.translate(COMP) for b in IUPAC[ch.upper()]))
    return next(k for k, v in IUPAC.items() if v == want)


def rc_iupac(s):
    return "".join(comp_letter(ch) for ch in reversed(s))


def genome_of(text):
    """Genome letters: ACGT in any case are bases, everything else is N."""
    return "".join(ch if ch in "ACGT" else "N" for ch in text.upper())


def site_match(pattern, guide, s):
    """(conditions 2 and 3, NM, mask in read orientation) of site s in read orientation; letters outside IUPAC raise KeyError."""
    pattern, guide, s = pattern.upper(), guide.upper(), s.upper()
    assert len(pattern) == len(guide) == len(s)
    sets_p, sets_g = [IUPAC[ch] for ch in pattern], [IUPAC[ch] for ch in guide]
    if any(ch not in "ACGT" for ch in s):
        return False, 0, 0
    ok = all(s[j] in sets_p[j] for j in range(len(s)))
    wrong = [j for j in range(len(s)) if s[j] not in sets_g[j]]
    return ok, len(wrong), sum(1 << j for j in wrong)


def forward_mask(mask, strand, L):
    """The record's mask: on '-' bit j of the read-orientation mask moves to L - 1 - j."""
    return mask if strand == 0 else sum(1 << (L - 1 - j) for j in range(L) if (mask >> j) & 1)


def definition(contigs, pattern, guides, m, starts=None):
    """The hits, site by site: (guide, strand, contig, pos, NM, forward mask) in ascending (guide, strand, contig, pos)
    order.  starts: only these (contig, pos)."""
    L = len(pattern)
    hits = []
    for c, raw in enumerate(contigs):
        seq = genome_of(raw)
        for p in range(len(seq)):
            if starts is not None and (c, p) not in starts:
                continue
            if p + L > len(seq):
                continue
            w = seq[p:p + L]
            for strand in (0, 1):
                s = w if strand == 0 else rc(w)
                for g, guide in enumerate(guides):
                    ok, nm, mask = site_match(pattern, guide, s)
                    if ok and nm <= m:
                        hits.append((g, strand, c, p, nm, forward_mask(mask, strand, L)))
    hits.sort(key=lambda h: h[:4])
    return hits


def _set_bits(text):
    return np.array([sum(1 << "ACGT".index(b) for b in IUPAC[ch]) for ch in text.upper()], dtype=np.int64)


def _codes(text):
    table = np.full(256, 4, dtype=np.int64)
    for k, ch in enumerate("ACGT"):
        table[ord(ch)] = table[ord(ch.lower())] = k
    return table[np.frombuffer(text.encode(), dtype=np.uint8)]


def brute_force(contigs, pattern, guides, m):
    """(hits as definition() gives them, number of candidates = sites that satisfy conditions 1 to 3, both strands)."""
    L = len(pattern)
    P = _set_bits(pattern)
    G = [_set_bits(g) for g in guides]
    weights = 1 << np.arange(L, dtype=np.int64)
    hits, n_cands = [], 0
    for c, raw in enumerate(contigs):
        seq = _codes(raw)
        if len(seq) < L:
            continue
        W = np.lib.stride_tricks.sliding_window_view(seq, L)
        clean = np.nonzero((W < 4).all(1))[0]
        for strand in (0, 1):
            S = W[clean] if strand == 0 else 3 - W[clean][:, ::-1]  # the complement of code k is 3 - k
            ok = ((P[None, :] >> S) & 1).all(1)
            idx, S = clean[ok], S[ok]
            n_cands += len(idx)
            for g in range(len(guides)):
                wrong = ((G[g][None, :] >> S) & 1) == 0  # read orientation
                nm = wrong.sum(1)
                fwd = wrong if strand == 0 else wrong[:, ::-1]
                masks = (fwd * weights[None, :]).sum(1)
                for k in np.nonzero(nm <= m)[0]:
                    hits.append((g, strand, c, int(idx[k]), int(nm[k]), int(masks[k])))
    hits.sort(key=lambda h: h[:4])
    return hits, n_cands


def arrays(hits, n_guides):
    """(records, rows) as vsc_search_pattern returns them."""
    rec = np.zeros(len(hits), dtype=HIT_DTYPE)
    rows = np.zeros((n_guides, 9), dtype=np.uint32)
    for k, (g, strand, c, p, nm, mask) in enumerate(hits):
        rec[k] = (g, c, p, strand << 31 | nm, mask)
        rows[g, nm] += 1
    return rec, rows


def merge_order(rec):
    """The indices that put records into ascending (guide, strand, contig, pos) order."""
    return np.lexsort((rec["pos"], rec["contig"], rec["info"] >> 31, rec["guide"]))


# ---- scenarios ------------------------------------------------------------------------------------------------------------
def rnd(rng, n):
    return "".join("ACGT"[k] for k in rng.integers(0, 4, n))


def put(seq, pos, site):
    return seq[:pos] + site + seq[pos + len(site):]


def make_site(rng, pattern, guide, subs=()):
    """A site in read orientation that satisfies the pattern and agrees with the guide wherever it can, but at `subs`."""
    s = []
    for j, (p, g) in enumerate(zip(pattern.upper(), guide.upper())):
        inside = [b for b in IUPAC[p] if b in IUPAC[g]]
        outside = [b for b in IUPAC[p] if b not in IUPAC[g]]
        pool = outside if (j in subs or not inside) else inside
        assert pool, (pattern, guide, j)
        s.append(pool[int(rng.integers(len(pool)))])
    return "".join(s)


PLACES = ("3", "5", "both")


def pattern_of(L, place):
    """The PAM at the 3' end, at the 5' end, or letters at both ends - that one is its own reverse complement."""
    return {"3": "N" * (L - 3) + "RRT", "5": "TTV" + "N" * (L - 3), "both": "SW" + "N" * (L - 4) + "WS"}[place]


def _with_pam(pattern, proto, pam):
    """proto at the pattern's N positions, the letters of pam (or N) at the others."""
    proto, pam, out = list(proto), list(pam), []
    for ch in pattern:
        out.append(proto.pop(0) if ch == "N" else (pam.pop(0) if pam else "N"))
    return "".join(out)


@functools.lru_cache(maxsize=None)
def edge_scenario(L=23, place="3"):
    """Contigs, pattern, guides and the restatement's hits at m = 8 (hits_at() cuts them down) - with the edge cases of the
    search's front end and floors on the hits (asserted here)."""
    rng = np.random.default_rng(1000 * L + PLACES.index(place))
    pattern = pattern_of(L, place)
    free = [j for j, ch in enumerate(pattern) if ch == "N"]  # the protospacer: where substitutions are planted
    spelled = {"3": "AGT", "5": "TTA", "both": "CATG"}[place]
    against = {"3": "CGT", "5": "TTT", "both": "AATG"}[place]  # one of its letters is outside the pattern's set
    proto = rnd(rng, len(free))
    g0 = _with_pam(pattern, proto, spelled)                    # the PAM letters spelled out: they count
    g1 = _with_pam(pattern, proto, "")                         # the same protospacer with N at the PAM positions
    p2 = list(rnd(rng, len(free)))
    for k, letter in ((1, "R"), (4, "Y"), (6, "N"), (9, "B"), (11, "W")):
        p2[k] = next(x for x in (letter, "N") if p2[k] in IUPAC[x])  # a degenerate letter that holds the base
    g2 = _with_pam(pattern, "".join(p2), "")
    g3 = _with_pam(pattern, rnd(rng, len(free)), against)      # contradicts the pattern: every hit pays one mismatch there
    g4 = _with_pam(pattern, rnd(rng, len(free)), "").lower()
    twin = make_site(rng, pattern, _with_pam(pattern, rnd(rng, len(free)), ""))  # g1-like site whose reverse complement is g5's
    g5 = "".join("N" if pattern[j] != "N" else ch for j, ch in enumerate(rc(twin)))
    g6 = "".join("N" if pattern[j] != "N" else ch for j, ch in enumerate(twin))
    guides = [g0, g1, g2, g3, g4, g5, g6]

    planted = []  # (strand, site on the forward genome)
    for g in (g0, g1):
        for strand in (0, 1):
            for n in range(MAX_M + 1):
                site = make_site(rng, pattern, g, set(int(x) for x in rng.choice(free, size=n, replace=False)))
                planted.append((strand, site if strand == 0 else rc(site)))
    for g in (g2, g3, g4):
        for strand in (0, 1):
            for n in (0, 2):
                single = [j for j in free if g.upper()[j] in "ACGT"]
                site = make_site(rng, pattern, g, set(int(x) for x in rng.choice(single, size=n, replace=False)))
                planted.append((strand, site if strand == 0 else rc(site)))
    order = [int(x) for x in rng.permutation(len(planted))]
    take = lambda strand: planted[order.pop(next(n for n, x in enumerate(order) if planted[x][0] == strand))][1]
    body = rnd(rng, 3 * TILE)
    # p = 0; across the first tile end on '+' and the second on '-'; then one site every 67 bases (many cross a 32-base word)
    body = put(body, 0, take(0))
    body = put(body, TILE - 10, make_site(rng, pattern, g1))
    body = put(body, 2 * TILE - 13, rc(make_site(rng, pattern, g1)))
    slots = [100 + 67 * n for n in range(70) if not any(abs(100 + 67 * n - q) < 80 for q in (TILE, 2 * TILE))]
    assert len(slots) >= len(order) and slots[len(order) - 1] < 5100
    for pos in slots[:len(order)]:
        body = put(body, pos, planted[order.pop()][1])
    exact = make_site(rng, pattern, g1)
    damaged = lambda ch: exact[:L // 2] + ch + exact[L // 2 + 1:]
    body = put(body, 5200, damaged("N"))        # an N and an IUPAC letter of the genome inside a site: absent
    body = put(body, 5300, damaged("R"))
    body = put(body, 5400, exact.lower())       # lower case: present
    body = put(body, 5500, rc(exact).lower())
    body = put(body, 5600, twin)                # g6 on '+' and g5 on '-' at one start where the pattern is its own reverse complement
    body = put(body, 5727, exact)               # starts at bit 31 of a word: for L = 32 it ends at bit 62 of the pair
    body = body[:len(body) - L] + exact         # p + L == len(c)
    left, right = rnd(rng, 150) + exact[:L // 2], exact[L // 2:] + rnd(rng, 150)  # a would-be site across two contigs
    small = [rnd(rng, L - 1), exact, rnd(rng, 1) + rc(exact)]
    contigs = [body, left, right] + small + [rnd(rng, 300)]
    hits, n_cands = brute_force(contigs, pattern, guides, MAX_M)
    e = {"L": L, "place": place, "pattern": pattern, "contigs": contigs, "guides": guides, "hits": hits, "n_cands": n_cands}
    # ---- floors ----
    on = lambda g, strand, c, p: [h for h in hits if h[:4] == (g, strand, c, p)]
    for strand in (0, 1):
        assert {h[4] for h in hits if h[1] == strand and h[0] in (0, 1)} == set(range(MAX_M + 1)), strand  # every NM, both strands
        assert any(h[1] == strand and h[2] == 0 and h[3] // 32 != (h[3] + L - 1) // 32 for h in hits), strand  # across a word end
        assert any(h[1] == strand and h[2] == 0 and h[3] < (1 + strand) * TILE < h[3] + L and h[4] == 0 for h in hits), strand  # across a tile end
    assert any(h[2] == 0 and h[3] == 0 for h in hits)                                    # p = 0
    assert on(1, 0, 0, len(body) - L) and on(1, 0, 0, len(body) - L)[0][4] == 0          # p + L == len(c)
    assert 5727 % 32 == 31 and on(1, 0, 0, 5727)[0][4] == 0                              # bit 31 of a word
    assert not any(h[2] == 3 for h in hits)                                              # a contig of L - 1 bases
    assert on(1, 0, 4, 0)[0][4] == 0 and on(1, 1, 5, 1)[0][4] == 0                       # contigs of L and L + 1 bases
    assert not any(h[0] == 1 and h[2] in (1, 2) and h[4] == 0 for h in hits)             # the site across two contigs
    assert not any(h[0] == 1 and h[2] == 0 and h[3] in (5200, 5300) for h in hits if h[4] <= 1)  # N / IUPAC inside a site
    assert on(1, 0, 0, 5400)[0][4] == 0 and on(1, 1, 0, 5500)[0][4] == 0                 # lower case in the genome
    assert any(h[0] == 2 and h[4] == 0 for h in hits)                                    # a guide with degenerate letters
    mine = [h for h in hits if h[0] == 3]
    assert mine and min(h[4] for h in mine) == 1 and {h[1] for h in mine} == {0, 1}      # a guide letter against the pattern
    assert any(h[0] == 4 and h[4] == 0 for h in hits)                                    # a lower-case guide
    # the spelled PAM counts: where g1 (N at the PAM) has NM n, g0 has n + the PAM letters that differ - somewhere more
    both = {h[1:4]: h[4] for h in hits if h[0] == 1}
    assert any(h[0] == 0 and h[1:4] in both and h[4] > both[h[1:4]] for h in hits)
    assert all(both[h[1:4]] <= h[4] for h in hits if h[0] == 0 and h[1:4] in both)
    assert on(6, 0, 0, 5600)[0][4] == 0
    if place == "both":
        assert pattern == rc_iupac(pattern) and on(5, 1, 0, 5600)[0][4] == 0             # both strands at one start
    else:
        assert pattern != rc_iupac(pattern)
    return e


def hits_at(e, m):
    return [h for h in e["hits"] if h[4] <= m]


@functools.lru_cache(maxsize=None)
def many_guides_scenario():
    """70 guides - two rounds at guide_batch = 64 - on the edge genome of L = 23, PAM at the 3' end, m = 3."""
    e = edge_scenario(23, "3")
    rng = np.random.default_rng(77)
    free = [j for j, ch in enumerate(e["pattern"]) if ch == "N"]
    guides = list(e["guides"]) + [_with_pam(e["pattern"], rnd(rng, len(free)), "") for _ in range(70 - len(e["guides"]))]
    guides[66], guides[69] = e["guides"][1], e["guides"][2]  # the second round has records of its own
    hits, n_cands = brute_force(e["contigs"], e["pattern"], guides, 3)
    assert len(guides) == 70 and {66, 69} <= {h[0] for h in hits}
    return {"pattern": e["pattern"], "contigs": e["contigs"], "guides": guides, "hits": hits, "n_cands": n_cands, "m": 3}


@functools.lru_cache(maxsize=None)
def tandem_scenario():
    """One 23-base SpCas9 site, 210 copies back to back across two tile ends: many hits per cell, several in a lane's 32 starts."""
    rng = np.random.default_rng(20262)
    pattern = "N" * 20 + "NGG"
    guide = rnd(rng, 20) + "NNN"
    site = make_site(rng, pattern, guide)
    contigs = [rnd(rng, 1000) + site * 210 + rnd(rng, 400)]
    guides = [guide, rnd(rng, 20) + "NNN"]
    hits, n_cands = brute_force(contigs, pattern, guides, 3)
    copies = [h for h in hits if h[0] == 0 and h[1] == 0 and h[4] == 0]
    assert len(copies) >= 200
    assert min(h[3] for h in copies) < TILE < 2 * TILE < max(h[3] for h in copies)
    assert max(np.bincount([h[3] // 32 for h in hits if h[0] == 0])) >= 2
    assert max(np.bincount([h[3] // TILE for h in copies])) > 64  # more hits in a cell than a wave has lanes
    return {"pattern": pattern, "contigs": contigs, "guides": guides, "hits": hits, "n_cands": n_cands, "m": 3}
