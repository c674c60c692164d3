"""A sparse, wide genome for the count / scan / write searches (vsc_guides_enumerate, vsc_search_bulges, vsc_search_pattern,
vsc_guides_enumerate_pattern, vsc_search_pattern_bulges): tens of thousands of tiles, so that a wave of the launch takes a run
of several tiles and a round has more than one group of cells - and an expected output that stays cheap.  Nothing here calls
the library.

The genome is N but for ACGT islands at chosen tiles.  A window that holds an N is no candidate under any of the five
definitions, and islands of one contig lie at least GAP = 64 N apart, so no site spans two islands: the genome's output is
every island's restatement output (enumerate_cases, bulges_cases, pattern_cases, pattern_enum_cases, pattern_bulge_cases - as
they are, once per distinct island text) with contig and position mapped, merged in record order.  tests/test_wide_cpu.py
checks that composition against the restatements run on the whole text of a miniature; placement_floors() asserts on the
expected hits themselves that every place the layout is built for is hit."""
import functools

import numpy as np

import bulges_cases as bc
import enumerate_cases as ec
import pattern_bulge_cases as pb
import pattern_cases as pc
import pattern_enum_cases as pe

TILE = 2048
GAP = 64
WAVES_PER_GROUP, GROUPS_PER_CU = 4, 8   # cell_grid (vsc_cells_device.h): at most CUs x 8 workgroups of 4 waves
CHUNK = 64                              # cells per chunk, chunks per group
SCAN_THREADS = 1024                     # enum_scan_kernel: one workgroup; beyond 1 024 entries a thread walks several
SHORT_MAX, BODY_TILES = 900, 3
APART = (70, 150, 700)                  # tiles between further short islands: other chunks of cells, the same group


# ---- size -----------------------------------------------------------------------------------------------------------------
def shape(n_tiles, W):
    """How a launch capped at W waves cuts n_tiles into runs: wave w takes tiles [w * per, (w + 1) * per)."""
    waves = min(-(-n_tiles // WAVES_PER_GROUP) * WAVES_PER_GROUP, W)
    per = -(-n_tiles // waves)
    working = -(-n_tiles // per)
    return {"W": W, "n_tiles": n_tiles, "waves": waves, "per": per, "working": working, "last_run": n_tiles - (working - 1) * per,
            "idle": waves - working}


def sizing_holds(s, guides=64):
    """What the wide genome's size is chosen for (and the tests assert for the device they run on)."""
    n = s["n_tiles"]
    return (n > s["W"] and s["per"] >= 3 and n % CHUNK != 0 and 0 < s["last_run"] < s["per"] and s["idle"] >= 1
            and groups_of(guides, n) > SCAN_THREADS)


def groups_of(guides, n_tiles):
    """Groups of 64 x 64 cells of a round of `guides` guides: what the two-level offset tables hand to the scan."""
    cells = 2 * guides * n_tiles
    chunks = -(-cells // CHUNK)
    return -(-chunks // CHUNK)


def size_for(cus):
    """The smallest n_tiles = max(32 768, 2 W) + k, W = CUs x 8 x 4, at which sizing_holds."""
    W = cus * GROUPS_PER_CU * WAVES_PER_GROUP
    base = max(32768, 2 * W)
    for k in range(1, 4 * CHUNK):
        s = shape(base + k, W)
        if sizing_holds(s):
            return s
    raise AssertionError("no size for %d CUs" % cus)


# ---- layout ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def layout(n_tiles, per):
    """Three contigs over n_tiles tiles and the islands' places, by kind of text ("short": at most SHORT_MAX bases, "body":
    more than two tiles and at most BODY_TILES, "roster_a" / "roster_b": at most BODY_TILES tiles less GAP), relative to the runs of `per` tiles:
      run 0: a short island at tile 0 (contig 0, position 0) and one in the run's last tile, empty tiles between them
      run 1: nothing
      run 2: a body over the run's first three tiles; then, as the runs have room, the end of contig 0 inside a tile with a
             short island that ends at the contig's end and one that starts contig 1; roster_a inside one run; a body that
             starts 100 bases into the last tile of a run and ends in the next run; roster_b inside one run; three short
             islands 70, 150 and 700 tiles further on: a guide's hits in several chunks of one group of cells
      half way: a short island in contig 1; at 5/8 the end of contig 1 in N; at 3/4 a short island in contig 2
      the last tile: a short island that ends at the end of contig 2, which is the end of the genome.
    Returns {"n_tiles", "per", "lens", "off", "islands": [(kind, contig, position in the contig, "start" | "end")]}."""
    assert per >= BODY_TILES
    t = 0

    def fit(k):  # the next k tiles that lie in one run
        nonlocal t
        if t % per + k > per:
            t = (t // per + 1) * per
        t += k
        return t - k

    spots = [("short", 0, "start"), ("short", (per - 1) * TILE + 300, "start")]  # (kind, global position, anchor)
    t = 2 * per
    spots.append(("body", fit(BODY_TILES) * TILE, "start"))
    t += 1  # (the body fills its last tile: one empty tile behind it)
    end0 = fit(1) * TILE + 1000
    spots += [("short", end0, "end"), ("short", end0 + 1, "start")]
    spots.append(("roster_a", fit(BODY_TILES) * TILE, "start"))
    seam = (t // per) * per + per - 1
    spots.append(("body", seam * TILE + 100, "start"))
    t = seam + BODY_TILES + 1
    spots.append(("roster_b", fit(BODY_TILES) * TILE, "start"))
    if t + len(APART) * max(APART) < n_tiles // 2:  # (not in the miniature: it has one chunk of cells per row)
        for step in APART:
            t += step
            spots.append(("short", fit(1) * TILE + 400, "start"))
    t = max(t, n_tiles // 2)
    spots.append(("short", fit(1) * TILE + 1234, "start"))
    t = max(t, 5 * n_tiles // 8)
    end1 = fit(1) * TILE + 500
    t = max(t, 3 * n_tiles // 4)
    spots.append(("short", fit(1) * TILE + 777, "start"))
    assert t <= n_tiles - 1, "the layout needs more tiles"
    end2 = (n_tiles - 1) * TILE + 1000
    spots.append(("short", end2, "end"))
    off = [0, end0 + 1, end1 + 1]
    lens = [end0, end1 - off[1], end2 - off[2]]
    islands = []
    for kind, g, anchor in spots:
        c = max(k for k in range(3) if off[k] <= g)
        islands.append((kind, c, g - off[c], anchor))
    return {"n_tiles": n_tiles, "per": per, "lens": lens, "off": off, "islands": islands}


def placed(lay, texts):
    """[(contig, start in the contig, text)] of the layout's islands for one family's texts - in ascending order, inside
    their contigs, GAP apart."""
    cap = {"short": SHORT_MAX, "body": BODY_TILES * TILE, "roster_a": BODY_TILES * TILE - GAP, "roster_b": BODY_TILES * TILE - GAP}
    assert len(texts["body"]) > (BODY_TILES - 1) * TILE  # from a tile's start on it reaches into the third tile
    out = []
    for kind, c, pos, anchor in lay["islands"]:
        text = texts[kind]
        assert 0 < len(text) <= cap[kind], (kind, len(text))
        out.append((c, pos if anchor == "start" else pos - len(text), text))
    assert out == sorted(out, key=lambda x: x[:2])
    for (c0, p0, t0), (c1, p1, _) in zip(out, out[1:]):
        assert c1 > c0 or p1 >= p0 + len(t0) + GAP, (c0, p0, c1, p1)
    assert all(0 <= p and p + len(text) <= lay["lens"][c] for c, p, text in out)
    return out


def contigs_of(lay, texts):
    """The contigs as bytes: N with the islands spliced in."""
    seqs = [bytearray(b"N") * n for n in lay["lens"]]
    for c, p, text in placed(lay, texts):
        seqs[c][p:p + len(text)] = text.encode()
    return [bytes(s) for s in seqs]


def compose(lay, texts, per_text, c_at, p_at, key):
    """per_text: {text: the restatement's tuples for the contig list [text]}.  Every island's tuples with the contig (field
    c_at) and the position (field p_at) mapped to the island's place, sorted by `key`."""
    out = []
    for c, p, text in placed(lay, texts):
        for h in per_text[text]:
            assert h[c_at] == 0
            out.append(h[:c_at] + (c,) + h[c_at + 1:p_at] + (h[p_at] + p,) + h[p_at + 1:])
    out.sort(key=key)
    return out


def times_placed(lay, texts, per_text):
    """The sum over the islands of a per-text number (the candidates)."""
    return sum(per_text[text] for _, _, text in placed(lay, texts))


def once_per_text(texts, fn):
    return {text: fn(text) for text in set(texts.values())}


# ---- floors on the expected output ----------------------------------------------------------------------------------------
def placement_floors(lay, W, sites, rows=None):
    """sites: (contig, position, length) of every expected hit or candidate; rows: its (guide, strand), where the call has
    guides.  Asserts that the expected output itself has something at every place the layout is built for, relative to the
    runs of shape(n_tiles, W)."""
    s = shape(lay["n_tiles"], W)
    per, n_tiles = s["per"], lay["n_tiles"]
    assert per == lay["per"]
    g = np.array([lay["off"][c] + p for c, p, _ in sites], dtype=np.int64)
    contig = np.array([c for c, _, _ in sites])
    ends_contig = np.array([p + n == lay["lens"][c] for c, p, n in sites])
    tile = g // TILE
    run = tile // per
    assert tile.max() == n_tiles - 1 and run.max() == s["working"] - 1           # the last tile, in the last working wave's run
    assert (tile == 0).any()                                                      # tile 0
    assert (ends_contig & (tile == n_tiles - 1)).any()                            # a site that ends with the genome
    hit_tiles = set(tile.tolist())
    in_run = lambda r: sorted(t for t in hit_tiles if t // per == r)
    runs = sorted(set(run.tolist()))
    assert any(all(t + k in hit_tiles and (t + k) // per == t // per for k in range(BODY_TILES)) for t in hit_tiles)  # three tiles of one run
    assert any(t + 1 in hit_tiles and (t + 1) // per != t // per for t in hit_tiles)                                  # across a seam of two runs
    assert any(in_run(r) == [r * per, r * per + per - 1] for r in runs)           # first and last tile of a run, nothing between
    assert any(len(set(contig[run == r].tolist())) > 1 for r in runs)             # both sides of a contig boundary in one run
    assert any(r > 0 and r - 1 not in runs for r in runs)                         # a run behind a run without any island
    assert len(set(contig.tolist())) == 3
    if rows is not None:
        have = set(rows)
        n_guides = 1 + max(gd for gd, _ in have)
        assert have == {(gd, st) for gd in range(n_guides) for st in (0, 1)}      # every guide on both strands: every row is live
        # a (guide, strand) row is n_tiles cells: the last tile's cell and tile 0's of the next row are neighbours, in one
        # chunk wherever the seam is no multiple of 64 - and both are live somewhere
        at = lambda gd, st, t: any(r == (gd, st) and tl == t for r, tl in zip(rows, tile.tolist()))
        seams = [(2 * gd + st) for gd in range(n_guides) for st in (0, 1)][:-1]
        assert any(((k + 1) * n_tiles) % CHUNK and at(k // 2, k % 2, n_tiles - 1) and at((k + 1) // 2, (k + 1) % 2, 0) for k in seams)
        # a cell's offset = its group's + the chunks of the group in front of its chunk + the cells of the chunk in front of
        # it: somewhere behind group 0 a group has hits in three chunks or more, and a chunk has hits in two cells or more
        cell = np.array([(2 * gd + st) * n_tiles for gd, st in rows], dtype=np.int64) + tile
        chunks = np.unique(cell // CHUNK)
        assert np.bincount(chunks[chunks >= CHUNK] // CHUNK).max() >= 3
        cells = np.unique(cell)
        assert np.bincount(cells[cells >= CHUNK * CHUNK] // CHUNK).max() >= 2


# ---- families: the texts, the guides and the expected output of each call --------------------------------------------------
def _spaced(rng, sites, first_at_0=True):
    out = ""
    for k, s in enumerate(sites):
        out += ("" if k == 0 and first_at_0 else pc.rnd(rng, int(rng.integers(3, 9)))) + s
    return out


@functools.lru_cache(maxsize=None)
def pattern_family(preset):
    """SaCas9 / Cas12a: pattern_bulge_cases' edge body and its 7 guides, 63 guides more, and the texts
      roster_a: every guide's plain site on both strands, 0 .. 3 substitutions
      roster_b: every guide's bulged site on both strands - one DNA and one RNA bulge of 1 - with 0 .. 2 substitutions
      short:    a plain and a bulged site of each of the 7 guides; it starts with a plain site and ends with bases that are a
                plain site and, with one base more, a DNA bulge of 1."""
    e = pb.edge_scenario(preset)
    pattern, proto = e["pattern"], e["proto"]
    L, (a, n) = len(pattern), proto
    rng = np.random.default_rng(5100 + sorted(pb.PRESETS).index(preset))
    guides = list(e["guides"]) + [pb.distinct_guide(rng, pattern, proto) for _ in range(63)]
    plain, bulged = [], []
    spread = {0: 0, 11: 1, 22: 2, 33: 3, 44: 4, 55: 5, 69: 6}  # the 7 guides' places among the 70: in every tile of a roster
    rest = iter(range(7, 70))
    for k in (spread[slot] if slot in spread else next(rest) for slot in range(70)):
        g = guides[k]
        letters = [j for j in range(a, a + n) if g.upper()[j] in "ACGT"]
        for strand in (0, 1):
            site = pc.make_site(rng, pattern, g, set(int(x) for x in rng.choice(letters, size=(k + 2 * strand) % 4, replace=False)))
            plain.append(site if strand == 0 else pc.rc(site))
            d = 1 if (k + strand) % 2 == 0 else -1
            i = a + 2 + k % 15
            free = [j for j in letters if j < i - 2 or j > i + 3]
            site = pb.plant(rng, pattern, g, proto, d, i, rng.choice(free, size=(k + strand) % 3, replace=False))
            bulged.append(site if strand == 0 else pc.rc(site))
    g0 = guides[0]
    exact = pc.make_site(rng, pattern, g0)
    if a == 0:
        tail = g0[0] + exact                 # '+': the last L bases a plain site, the last L + 1 a DNA bulge of 1 at split point 1
    else:
        assert a + n == L
        tail = pc.rc(exact + g0[L - 1])      # '-': the same with the unpaired base at the protospacer's other end
    few = []
    for k, g in enumerate(guides[:7]):
        site = pc.make_site(rng, pattern, g)
        few.append(site if k % 2 == 0 else pc.rc(site))
        site = pb.plant(rng, pattern, g, proto, 1, a + 4 + k)
        few.append(site if k % 2 == 1 else pc.rc(site))
    texts = {"body": e["contigs"][0], "roster_a": _spaced(rng, plain), "roster_b": _spaced(rng, bulged),
             "short": _spaced(rng, few + [tail])}
    return {"preset": preset, "pattern": pattern, "proto": proto, "guides": guides, "texts": texts}


@functools.lru_cache(maxsize=None)
def reads_family():
    """The 23-base searches (vsc_search_bulges, vsc_guides_enumerate): bulges_cases' edge body and its 7 guides, 13 reads more;
    roster_a is random text (candidate guides on both strands, bulge candidates), roster_b every read's bulged site on both
    strands, short a bulged site of each of the 7 reads, ending with a read behind its own first base: a window that ends in
    GG and a DNA bulge of 1."""
    e = bc.edge_scenario()
    rng = np.random.default_rng(5200)
    guides = list(e["guides"]) + [bc.distinct_read(rng, ("TGG", "AGG", "CGA")[k % 3]) for k in range(13)]
    reads = [bc.read_of(g) for g in guides]
    bulged = []
    for k, r in enumerate(reads):
        for strand in (0, 1):
            d = 1 if (k + strand) % 2 == 0 else -1
            i = 2 + k % 15
            free = [j for j in range(21) if j < i - 1 or j > i + 2]
            site = bc.plant(rng, r, d, i, rng.choice(free, size=(k + strand) % 3, replace=False))
            bulged.append(site if strand == 0 else bc.rc(site))
    few = []
    for k, r in enumerate(reads[:7]):
        site = bc.plant(rng, r, 1 if k % 2 else -1, 4 + k)
        few.append(site if k % 2 == 0 else bc.rc(site))
    tail = reads[0][0] + reads[0]
    texts = {"body": e["contigs"][0], "roster_a": pc.rnd(rng, BODY_TILES * TILE - GAP), "roster_b": _spaced(rng, bulged),
             "short": _spaced(rng, few + [tail])}
    return {"guides": guides, "texts": texts}


def expect_pattern(lay, texts, pattern, guides, m):
    """vsc_search_pattern: (hits in record order, candidates)."""
    per = once_per_text(texts, lambda text: pc.brute_force([text], pattern, guides, m))
    hits = compose(lay, texts, {t: v[0] for t, v in per.items()}, 2, 3, lambda h: h[:4])
    return hits, times_placed(lay, texts, {t: v[1] for t, v in per.items()})


def expect_pattern_bulges(lay, texts, pattern, guides, proto, m, dna, rna):
    """vsc_search_pattern_bulges: (hits in record order, candidates)."""
    per = once_per_text(texts, lambda text: pb.brute_force([text], pattern, guides, proto, m, dna, rna))
    hits = compose(lay, texts, {t: v[0] for t, v in per.items()}, 2, 3, lambda h: h[:5])
    return hits, times_placed(lay, texts, {t: v[1] for t, v in per.items()})


def expect_bulges(lay, texts, guides, m, dna, rna):
    """vsc_search_bulges: (hits in record order, candidates)."""
    cands = once_per_text(texts, lambda text: bc.candidates([text], dna, rna))
    per = {text: bc.brute_force([text], guides, m, dna, rna, cands=cands[text]) for text in cands}
    hits = compose(lay, texts, per, 2, 3, lambda h: h[:5])
    return hits, times_placed(lay, texts, {t: len(v) for t, v in cands.items()})


def in_targets(found, L, targets, rule, lens):
    """The candidates (contig, pos, strand, ..) whose L-base site lies in the targets: pattern_enum_cases.in_targets, which is
    the regions' rule too (a candidate's window never leaves its contig)."""
    return [x for x in found if pe.in_targets(x[0], x[1], L, targets, rule, lens)]


def expect_enumerate(lay, texts, targets=None, rule="overlap", **filters):
    """vsc_guides_enumerate: the candidates in result order."""
    per = once_per_text(texts, lambda text: ec.brute_force([text], **filters))
    found = compose(lay, texts, per, 0, 1, lambda x: x[:3])
    return found if targets is None else in_targets(found, ec.WINDOW, targets, rule, lay["lens"])


def expect_enumerate_pattern(lay, texts, pattern, proto, targets=None, rule="overlap", **filters):
    """vsc_guides_enumerate_pattern: the candidates in result order."""
    L = len(pattern)
    per = once_per_text(texts, lambda text: pe.kept(pe.candidates([text], pattern), [text], L, proto, **filters))
    found = compose(lay, texts, per, 0, 1, lambda x: x[:3])
    return found if targets is None else in_targets(found, L, targets, rule, lay["lens"])


def targets_of(lay, texts, n_only_tiles):
    """(contig, start, end) targets: the first body wholly, the body across the seam cut from its middle on, roster_a cut
    before its end, the island at the end of contig 0 with the boundary (clipped to the contig), one island of contig 2 by a
    handful of bases - and intervals in N only: two small ones and, where n_only_tiles is not 0, one of that many tiles in
    contig 2 (it is what makes the work list long)."""
    spots = placed(lay, texts)
    bodies = [(c, p) for c, p, text in spots if text == texts["body"]]
    roster = next((c, p) for c, p, text in spots if text == texts["roster_a"])
    at_end0 = next((c, p) for c, p, text in spots if c == 0 and p + len(text) == lay["lens"][0])
    c1 = [(c, p) for c, p, text in spots if c == 1]
    c2 = [(c, p) for c, p, text in spots if c == 2]
    out = [(bodies[0][0], bodies[0][1] - 100, bodies[0][1] + len(texts["body"]) + 77),
           (bodies[1][0], bodies[1][1] + 3000, bodies[1][1] + len(texts["body"]) + 50),
           (roster[0], roster[1] - 40, roster[1] + 2500),
           (0, at_end0[1] + 40, lay["lens"][0] + 999),
           (2, c2[0][1] + 100, c2[0][1] + 130),
           (0, bodies[0][1] - 3 * TILE, bodies[0][1] - 3 * TILE + 50),       # in the run without an island
           (1, c1[-1][1] + SHORT_MAX + 100, c1[-1][1] + SHORT_MAX + 800)]    # behind the last island of contig 1
    if n_only_tiles:
        wide_from = c2[0][1] + SHORT_MAX + 5 * TILE
        assert wide_from + n_only_tiles * TILE + 300 < c2[1][1] - GAP
        out.append((2, wide_from, wide_from + n_only_tiles * TILE + 300))
    return out
