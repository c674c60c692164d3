"""Cut sites (include/varscot_hip.h, vsc_hits_sites) restated in plain Python, and the scenarios the tests run it on.  The
restatement calls nothing of the library: collapse() is the definition - a dict by (guide, strand, contig, a), then min by
(NM + |d|, |d|, DNA before RNA) - over alignment tuples, and every scenario asserts floors on the restatement's OWN output, so
that no branch of the definition is empty in it.  The plain hits of the SpCas9 scenarios come from the oracle's search, the
bulged ones from bulges_cases; the Cas12a scenario takes both from the pattern restatements."""
import functools

import numpy as np

import bulges_cases as bc
import pattern_bulge_cases as pbc
import pattern_cases as pc

HIT_DTYPE = np.dtype([("guide", "<u4"), ("contig", "<u4"), ("pos", "<u4"), ("info", "<u4")])
SITE_DTYPE = np.dtype([("guide", "<u4"), ("contig", "<u4"), ("pos", "<u4"), ("info", "<u4"), ("anchor", "<u4"), ("members", "<u4"),
                       ("best", "<u4"), ("reserved", "<u4")])
SITE_ROW_DTYPE = np.dtype([("sites", "<u4"), ("alignments", "<u4"), ("bulge_only", "<u4"), ("count", "<u4", (3, 9))])
TILE = 64  # records per tile of the device's passes


# ---- alignments: (guide, strand, contig, pos, d, nm, index) -------------------------------------------------------------
def plain_of_hits(rec):
    """vsc_hit records -> alignments (d = 0, index = 0)."""
    return [(int(g), int(i) >> 31, int(c), int(p), 0, (int(i) >> 23) & 31, 0) for g, c, p, i in zip(rec["guide"], rec["contig"], rec["pos"], rec["info"])]


def plain_of_pattern(rec):
    """vsc_pattern_hit records -> alignments."""
    return [(int(g), int(i) >> 31, int(c), int(p), 0, int(i) & 63, 0) for g, c, p, i in zip(rec["guide"], rec["contig"], rec["pos"], rec["info"])]


def bulged_of_records(rec):
    """vsc_bulge_hit records -> alignments."""
    out = []
    for g, c, p, i in zip(rec["guide"], rec["contig"], rec["pos"], rec["info"]):
        i = int(i)
        size = (i >> 10) & 3
        out.append((int(g), i >> 31, int(c), int(p), -size if (i >> 12) & 1 else size, i & 31, (i >> 5) & 31))
    return out


def bulged_of_hits(hits):
    """The hit tuples of bulges_cases / pattern_bulge_cases -> alignments."""
    return [(g, strand, c, p, d, nm, index) for g, strand, c, p, d, nm, index, _ in hits]


def anchor_of(x, length, anchor):
    """a of the definition's table."""
    _, strand, _, pos, d, _, _ = x
    at_start = (anchor == "end") == (strand == 1)
    return pos if at_start else pos + length + d


def better(x):
    """The order inside a site: (NM + |d|, |d|, DNA before RNA)."""
    return (x[5] + abs(x[4]), abs(x[4]), 0 if x[4] >= 0 else 1)


def collapse(plain, bulged, length=23, anchor="end"):
    """The definition: [(best alignment, its list (0 plain / 1 bulged), its index there, a, {d: nm} of the members)] in ascending
    (guide, strand, contig, pos, d) order of the best alignments."""
    sites = {}
    for which, lst in ((0, plain), (1, bulged)):
        for k, x in enumerate(lst):
            a = anchor_of(x, length, anchor)
            sites.setdefault((x[0], x[1], x[2], a), []).append((x, which, k))
    out = []
    for (_, _, _, a), members in sites.items():
        assert len({m[0][4] for m in members}) == len(members) <= 5  # one member per d
        x, which, k = min(members, key=lambda m: better(m[0]))
        out.append((x, which, k, a, {m[0][4]: m[0][5] for m in members}))
    out.sort(key=lambda s: s[0][:5])
    return out


def members_word(nm_by_d):
    w = 0
    for k, d in enumerate((-2, -1, 0, 1, 2)):
        w |= nm_by_d.get(d, 31) << (5 * k)
    return w | len(nm_by_d) << 25


def arrays(sites, plain, bulged, n_guides):
    """(records, rows) as vsc_hits_sites returns them."""
    rec = np.zeros(len(sites), dtype=SITE_DTYPE)
    rows = np.zeros(n_guides, dtype=SITE_ROW_DTYPE)
    for k, (x, which, at, a, nm_by_d) in enumerate(sites):
        g, strand, c, p, d, nm, index = x
        rec[k] = (g, c, p, bc.info_word(strand, d, index, nm), a, members_word(nm_by_d), at, 0)
        rows["sites"][g] += 1
        rows["bulge_only"][g] += 0 not in nm_by_d
        rows["count"][g, abs(d), nm] += 1
    for x in list(plain) + list(bulged):
        rows["alignments"][x[0]] += 1
    return rec, rows


def expected(plain, bulged, n_guides, length=23, anchor="end"):
    return arrays(collapse(plain, bulged, length, anchor), plain, bulged, n_guides)


def site_key(x, length=23, anchor="end"):
    return (x[0], x[1], x[2], anchor_of(x, length, anchor))


def unstraddled(bulged, length=23, anchor="end"):
    """The tile ends of the bulged list (multiples of 64 below its length) that no site has bulged members on both sides of."""
    first, last = {}, {}
    for k, x in enumerate(bulged):
        first.setdefault(site_key(x, length, anchor), k)
        last[site_key(x, length, anchor)] = k
    return [end for end in range(TILE, len(bulged), TILE) if not any(first[s] < end <= last[s] for s in first)]


def cost_tie(nm_by_d):
    costs = sorted(nm + abs(d) for d, nm in nm_by_d.items())
    return len(costs) > 1 and costs[0] == costs[1]


# ---- scenarios ------------------------------------------------------------------------------------------------------------
def edge_scenario(oracle):
    """bulges_cases.edge_scenario() plus the plain hits of the same guides at m = 4 (the oracle's search), collapsed."""
    e = dict(bc.edge_scenario())
    reads = [bc.read_of(g) for g in e["guides"]]
    e["plain_rec"] = oracle.search(e["contigs"], reads, bc.EDGE_M, mode=oracle.MODE_PREDICATE)
    e["plain"] = plain_of_hits(e["plain_rec"])
    e["bulged"] = bulged_of_hits(e["hits"])
    e["bulged_rec"] = bc.arrays(e["hits"], len(e["guides"]))[0]
    sites = e["sites"] = collapse(e["plain"], e["bulged"])
    # ---- floors ----
    assert (len(e["plain"]), len(e["bulged"]), len(sites)) == (33, 272, 140), (len(e["plain"]), len(e["bulged"]), len(sites))
    assert {len(s[4]) for s in sites} == {1, 2, 3, 4, 5}                                      # site sizes 1 .. 5
    assert {s[0][4] for s in sites} == {-2, -1, 0, 1, 2}                                      # a best of every d
    assert any(s[1] == 1 and 0 in s[4] for s in sites)                                        # a bulged alignment beats the plain one
    assert any(cost_tie(s[4]) for s in sites)                                                 # a cost tie
    assert {s[0][1] for s in sites if len(s[4]) > 1} == {0, 1}                                # both strands among the multi-member sites
    return e


def at_budget(e, m, dna=2, rna=2, guides=None):
    """(plain, bulged) alignments of a scenario under a smaller budget, fewer classes or the first `guides` guides."""
    keep = lambda x: x[5] <= m and (guides is None or x[0] < guides)
    classes = bc.enabled(dna, rna)
    return [x for x in e["plain"] if keep(x)], [x for x in e["bulged"] if keep(x) and x[4] in classes]


HOMO_N = 400


def homopolymer_scenario(oracle):
    """A contig of 400 G, one of 400 C, one of 23 G and the guide G x 23 at dna = rna = 2: every position is a hit of every
    class.  (The short contig's five '+' records shift the '-' run of the bulged list by one: its sites of four adjacent records
    then lie across the tile ends, not between them.)"""
    contigs, guides = ["G" * HOMO_N, "C" * HOMO_N, "G" * 23], ["G" * 23]
    hits = bc.brute_force(contigs, guides, 4, 2, 2)
    e = {"contigs": contigs, "guides": guides, "hits": hits}
    e["plain_rec"] = oracle.search(contigs, guides, 4, mode=oracle.MODE_PREDICATE)
    e["plain"] = plain_of_hits(e["plain_rec"])
    e["bulged"] = bulged_of_hits(hits)
    e["bulged_rec"] = bc.arrays(hits, 1)[0]
    sites = e["sites"] = collapse(e["plain"], e["bulged"])
    plain, bulged = e["plain"], e["bulged"]
    # ---- floors ----
    for strand, c in ((0, 0), (1, 1)):  # every interior PAM is a five-member site on one strand
        mine = {s[3]: s for s in sites if s[0][1] == strand and s[0][2] == c}
        interior = range(30, HOMO_N - 5) if strand == 0 else range(5, HOMO_N - 30)
        assert all(len(mine[a][4]) == 5 and mine[a][0][4] == 0 for a in interior), strand
        assert not any(s[0][1] != strand for s in sites if s[0][2] == c)
    assert {len(s[4]) for s in sites if s[0][2] == 0 and s[3] <= 25} >= {2, 3, 4}             # fewer members at the contig start
    # a sibling would lie at a negative position: a '+' site so close to the contig start that its d = +2 member would start in front of it
    assert any(s[0][1] == 0 and s[0][3] + s[0][4] - 2 < 0 for s in sites)
    assert len(plain) > 2 * TILE and len(bulged) > 8 * TILE
    # a site's members straddle every tile end of the bulged list; the plain list holds one member per site, so there the
    # records on either side of every tile end belong to sites with bulged members (their lookups cross into the other list)
    assert unstraddled(bulged) == []
    with_bulged = {site_key(x) for x in bulged}
    assert all(site_key(plain[k]) in with_bulged for end in range(TILE, len(plain), TILE) for k in (end - 1, end))
    # sites have members on both sides of the seam between the lists: the last plain record's site holds bulged members, and a
    # record of the first bulged tile lies in a site with a plain member
    plain_keys = {site_key(x) for x in plain}
    assert site_key(plain[-1]) in with_bulged and any(site_key(x) in plain_keys for x in bulged[:TILE])
    return e


@functools.lru_cache(maxsize=None)
def cas12a_scenario():
    """pattern_bulge_cases' Cas12a edge scenario (TTTV + 23, the protospacer at the pattern's end: anchor "start") with the plain
    hits of the pattern restatement."""
    b = pbc.edge_scenario("Cas12a")
    plain_hits, _ = pc.brute_force(b["contigs"], b["pattern"], b["guides"], b["m"])
    e = {"pattern": b["pattern"], "proto": b["proto"], "contigs": b["contigs"], "guides": b["guides"], "m": b["m"], "length": len(b["pattern"])}
    e["plain_rec"] = pc.arrays(plain_hits, len(b["guides"]))[0]
    e["plain"] = plain_of_pattern(e["plain_rec"])
    e["bulged"] = bulged_of_hits(b["hits"])
    e["bulged_rec"] = pbc.arrays(b["hits"], len(b["guides"]))[0]
    sites = e["sites"] = collapse(e["plain"], e["bulged"], e["length"], "start")
    assert e["plain"] and len(sites) < len(e["plain"]) + len(e["bulged"])
    assert {s[0][1] for s in sites if len(s[4]) > 1} == {0, 1} and max(len(s[4]) for s in sites) >= 3
    assert any(s[1] == 0 for s in sites) and any(s[1] == 1 for s in sites)
    assert collapse(e["plain"], e["bulged"], e["length"], "end") != sites  # the anchor matters
    return e
