"""Table scores of bulged alignments and cut sites on the device: the f words, the score records, the rows and the selected
records of vsc_bulge_hits_table / vsc_sites_table byte for byte what the definition gives when it is restated in plain Python
(tests/bulge_table_cases.py) - over the edge and homopolymer scenarios, budgets and classes, Cas12a and SaCas9 through the
pattern calls, SpCas9 as a pattern, list lengths around one workgroup, records that no search returns (each scores 0), sites
at the ends of contigs and of the planes, the two outputs, the selection's ties and its digit passes, repetition, the table
cache and the timing fields."""
import ctypes as C

import numpy as np
import pytest

import varscot_amd as va
from varscot_amd import _lib
import bulge_table_cases as btc
import bulges_cases as bc
import pattern_bulge_cases as pbc
import pattern_cases as pc
import sites_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = va.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def sp():
    """An SpCas9 table with planted zeros and ones, and one without zeros."""
    rng = np.random.default_rng(811)
    zeroed, plain = btc.random_bulge_table(rng, btc.SHAPES["SpCas9"], zeros=20, ones=12), btc.random_bulge_table(rng, btc.SHAPES["SpCas9"])
    t = {"zeroed": zeroed, "plain": plain, "h_zeroed": btc.make_table(va, zeroed), "h_plain": btc.make_table(va, plain)}
    yield t
    t["h_zeroed"].close()
    t["h_plain"].close()


@pytest.fixture(scope="module")
def edge(oracle, ctx, sp):
    e = sc.edge_scenario(oracle)
    e["texts"] = [bc.read_of(g) for g in e["guides"]]
    e["gen"] = ctx.load_genome(va.PackedGenome.from_sequences(e["contigs"]))
    n = len(e["guides"])
    e["site_rec"] = sc.arrays(e["sites"], e["plain"], e["bulged"], n)[0]
    e["f"] = btc.bulged_scored(e["contigs"], e["texts"], e["bulged"], sp["zeroed"])
    e["scores"], e["rows"] = btc.site_records(sp["zeroed"], e["contigs"], e["texts"], e["sites"], n)
    assert (e["f"] == 0).any() and (e["f"] > 0).any() and (e["scores"]["top"] != e["scores"]["best"]).any()
    assert len({int(s["top_d"]) for s in e["scores"]}) >= 4
    yield e
    e["gen"].close()


@pytest.fixture(scope="module")
def homo(oracle, ctx, sp):
    e = sc.homopolymer_scenario(oracle)
    e["texts"] = list(e["guides"])
    e["gen"] = ctx.load_genome(va.PackedGenome.from_sequences(e["contigs"]))
    e["site_rec"] = sc.arrays(e["sites"], e["plain"], e["bulged"], 1)[0]
    e["f"] = btc.bulged_scored(e["contigs"], e["texts"], e["bulged"], sp["plain"])
    e["scores"], e["rows"] = btc.site_records(sp["plain"], e["contigs"], e["texts"], e["sites"], 1)
    yield e
    e["gen"].close()


class Handle:
    """A vsc_bulge_hits / vsc_sites object over host records (vsc_debug_*_from_host)."""

    def __init__(self, ctx, rec, kind):
        self.kind, self._h = kind, C.c_void_p()
        rec = np.ascontiguousarray(rec)
        fn = va.lib().vsc_debug_bulge_hits_from_host if kind == "bulged" else va.lib().vsc_debug_sites_from_host
        va.api.check(fn(ctx._h, rec.ctypes.data, len(rec), C.byref(self._h)), ctx._h)

    def close(self):
        (va.lib().vsc_bulge_hits_free if self.kind == "bulged" else va.lib().vsc_sites_free)(self._h)
        self._h = None


def bulged_table(gen, rec, texts, table, records=True, rows=True):
    h = Handle(gen.ctx, rec, "bulged")
    try:
        return gen._bulge_scores(h._h, [t.encode() for t in texts], table, records, rows)
    finally:
        h.close()


def sites_table(gen, rec, texts, table, length=23, anchor="end", top_k=0, min_score=0, records=True, rows=True):
    h = Handle(gen.ctx, rec, "sites")
    try:
        return gen._site_scores(h._h, _lib.SiteParams(length, {"end": 0, "start": 1}[anchor]), [t.encode() for t in texts], table, top_k,
                                min_score, records, rows)
    finally:
        h.close()


def same_bytes(got, want):
    assert got.dtype == want.dtype and len(got) == len(want) and got.tobytes() == want.tobytes()


# ---- 1. the scenarios -----------------------------------------------------------------------------------------------------
def test_edge_scenario_equals_the_restatement(edge, sp):
    n = len(edge["guides"])
    rec, _, fixed, rows = edge["gen"].search_bulges(edge["guides"], bc.EDGE_M, dna=2, rna=2, table=sp["h_zeroed"])
    same_bytes(rec, edge["bulged_rec"])
    same_bytes(fixed, edge["f"])
    same_bytes(rows, btc.bulged_rows(edge["bulged"], edge["f"], n))
    sites, site_rows, scores, table_rows = edge["gen"].search_sites(edge["guides"], bc.EDGE_M, dna=2, rna=2, table=sp["h_zeroed"])
    assert len(sites) == 140 and int(site_rows["alignments"].sum()) == 305
    same_bytes(sites, edge["site_rec"])
    same_bytes(scores, edge["scores"])
    same_bytes(table_rows, edge["rows"])
    assert scores.dtype == va.SITE_SCORE_DTYPE and table_rows.dtype == va.TABLE_ROW_DTYPE


@pytest.mark.parametrize("m", [0, 4])
@pytest.mark.parametrize("dna,rna", [(1, 0), (0, 2), (2, 2)])
def test_budgets_and_classes(oracle, edge, sp, m, dna, rna):
    n = len(edge["guides"])
    plain = sc.plain_of_hits(oracle.search(edge["contigs"], edge["texts"], m, mode=oracle.MODE_PREDICATE))
    bulged = [x for x in edge["bulged"] if x[5] <= m and x[4] in bc.enabled(dna, rna)]
    assert bulged
    f = btc.bulged_scored(edge["contigs"], edge["texts"], bulged, sp["zeroed"])
    _, _, fixed, rows = edge["gen"].search_bulges(edge["guides"], m, dna=dna, rna=rna, table=sp["h_zeroed"])
    same_bytes(fixed, f)
    same_bytes(rows, btc.bulged_rows(bulged, f, n))
    sites = sc.collapse(plain, bulged)
    want = btc.site_records(sp["zeroed"], edge["contigs"], edge["texts"], sites, n)
    got = edge["gen"].search_sites(edge["guides"], m, dna=dna, rna=rna, table=sp["h_zeroed"])
    same_bytes(got[0], sc.arrays(sites, plain, bulged, n)[0])
    same_bytes(got[2], want[0])
    same_bytes(got[3], want[1])


def test_homopolymer_ties_and_the_selection(homo, sp):
    """Every interior site has the same top: the cut falls inside a tie run that crosses a 256-record step of the walk; at 1, at
    the segment's length and above it; the floor just at, just above and just below the common value."""
    gen, table = homo["gen"], sp["h_plain"]
    top = homo["scores"]["top"]
    values, counts = np.unique(top, return_counts=True)
    common = int(values[counts.argmax()])
    interior = [k for k, s in enumerate(homo["sites"]) if len(s[4]) == 5]
    assert len(interior) > 600 and all(int(top[k]) == common for k in interior) and common > 0
    n = len(top)
    full = gen.search_sites(homo["guides"], 4, dna=2, rna=2, table=table)
    same_bytes(full[0], homo["site_rec"])
    same_bytes(full[2], homo["scores"])
    same_bytes(full[3], homo["rows"])
    above = int((top > common).sum())
    ties = np.nonzero(top == common)[0]
    k_inside = above + int((ties < 256).sum()) + 40  # the last survivor is a tie behind the first step of the walk
    assert ties[0] < 256 < ties[k_inside - above - 1] and k_inside - above < len(ties)
    for top_k, floor in ((k_inside, 0), (1, 0), (n, 0), (n + 7, 0), (0, common), (0, common + 1), (0, common - 1), (300, common), (5, common + 1)):
        keep = btc.cut(homo["site_rec"]["guide"], top, top_k, floor)
        got = gen.search_sites(homo["guides"], 4, dna=2, rna=2, table=table, top_k=top_k, min_score=floor)
        assert len(got[0]) == len(keep), (top_k, floor)
        same_bytes(got[0], homo["site_rec"][keep])
        same_bytes(got[2], homo["scores"][keep])
        same_bytes(got[1], full[1])  # the rows are over all sites, whatever is kept
        same_bytes(got[3], homo["rows"])
    assert len(btc.cut(homo["site_rec"]["guide"], top, 0, common + 1)) < len(btc.cut(homo["site_rec"]["guide"], top, 0, common)) < n + 1


def test_selection_over_several_guides_in_one_workgroup(edge, sp):
    """140 sites of several guides: every segment ends inside the first workgroup's 256 records."""
    top = edge["scores"]["top"]
    assert len(set(edge["site_rec"]["guide"].tolist())) >= 3
    floor = int(np.median(top[top > 0]))
    for top_k, min_score in ((1, 0), (3, 0), (3, floor), (0, floor), (1000, 1)):
        keep = btc.cut(edge["site_rec"]["guide"], top, top_k, min_score)
        got = sites_table(edge["gen"], edge["site_rec"], edge["texts"], sp["h_zeroed"], top_k=top_k, min_score=min_score)
        same_bytes(got[0], edge["site_rec"][keep])
        same_bytes(got[1], edge["scores"][keep])
        same_bytes(got[2], edge["rows"])


@pytest.fixture(scope="module")
def digits(ctx):
    s = dict(btc.digits_sites())
    s["keep"] = {case: btc.cut(s["site_rec"]["guide"], s["scores"]["top"], *case) for case in s["cases"]}
    s["obj"] = btc.make_table(va, s["table"])
    s["gen"] = ctx.load_genome(va.PackedGenome.from_sequences(s["contigs"]))
    yield s
    s["gen"].close()
    s["obj"].close()


def test_site_selection_digit_by_digit(digits):
    """digits_sites(): the pattern hits' digit cases on the site copy of the select - thresholds that share one, two and three
    digits of `top` with their neighbours, ties over the steps of the walk, T = 0, floors at and beside T."""
    s = digits
    search = lambda **kw: s["gen"].search_pattern_sites(s["pattern"], s["guides"], s["m"], s["proto"], dna=1, rna=1, table=s["obj"], **kw)
    full = search()
    same_bytes(full[0], s["site_rec"])  # the collapse and the scores first: a failure below is the selection's
    same_bytes(full[1], s["site_rows"])
    same_bytes(full[2], s["scores"])
    same_bytes(full[3], s["rows"])
    for (top_k, min_score), keep in s["keep"].items():
        got = search(top_k=top_k, min_score=min_score)
        assert len(got[0]) == len(keep), (top_k, min_score)
        same_bytes(got[0], s["site_rec"][keep])
        same_bytes(got[2], s["scores"][keep])
        same_bytes(got[1], s["site_rows"])  # the rows are over all sites, whatever is kept
        same_bytes(got[3], s["rows"])


# ---- 2. the pattern form --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["Cas12a", "SaCas9"])
def test_other_nucleases_through_the_pattern_calls(ctx, name):
    if name == "Cas12a":
        e = sc.cas12a_scenario()
        pattern, proto, contigs, guides, m, anchor = e["pattern"], e["proto"], e["contigs"], e["guides"], e["m"], "start"
        plain, bulged = e["plain"], e["bulged"]
    else:
        b = pbc.edge_scenario("SaCas9")
        pattern, proto, contigs, guides, m, anchor = b["pattern"], b["proto"], b["contigs"], b["guides"], b["m"], "end"
        plain = sc.plain_of_pattern(pc.arrays(pc.brute_force(contigs, pattern, guides, m)[0], len(guides))[0])
        bulged = sc.bulged_of_hits(b["hits"])
    n, L = len(guides), len(pattern)
    table = btc.random_bulge_table(np.random.default_rng(900 + L + proto[0]), btc.SHAPES[name], zeros=16, ones=8)
    sites = sc.collapse(plain, bulged, L, anchor)
    f = btc.bulged_scored(contigs, guides, bulged, table)
    want = btc.site_records(table, contigs, guides, sites, n, anchor)
    assert (f > 0).any() and (want[0]["top"] > 0).any()
    t = btc.make_table(va, table)
    gen = ctx.load_genome(va.PackedGenome.from_sequences(contigs))
    try:
        _, _, fixed, rows = gen.search_pattern_bulges(pattern, guides, m, proto, dna=2, rna=2, table=t)
        same_bytes(fixed, f)
        same_bytes(rows, btc.bulged_rows(bulged, f, n))
        got = gen.search_pattern_sites(pattern, guides, m, proto, dna=2, rna=2, table=t)
        same_bytes(got[0], sc.arrays(sites, plain, bulged, n)[0])
        same_bytes(got[2], want[0])
        same_bytes(got[3], want[1])
        keep = btc.cut(got[0]["guide"], want[0]["top"], 2, 1)
        cut = gen.search_pattern_sites(pattern, guides, m, proto, dna=2, rna=2, table=t, top_k=2, min_score=1)
        same_bytes(cut[0], got[0][keep])
        same_bytes(cut[2], want[0][keep])
    finally:
        gen.close()
        t.close()


def test_spcas9_as_a_pattern_gives_the_plain_route_bytes(edge, sp):
    pattern = "N" * 21 + "GR"
    a = edge["gen"].search_pattern_sites(pattern, edge["texts"], bc.EDGE_M, (0, 20), dna=2, rna=2, table=sp["h_zeroed"])
    b = edge["gen"].search_sites(edge["guides"], bc.EDGE_M, dna=2, rna=2, table=sp["h_zeroed"])
    same_bytes(a[2], b[2])
    same_bytes(a[3], b[3])
    same_bytes(a[2], edge["scores"])
    pa = edge["gen"].search_pattern_bulges(pattern, edge["texts"], bc.EDGE_M, (0, 20), dna=2, rna=2, table=sp["h_zeroed"])
    same_bytes(pa[2], edge["f"])
    same_bytes(pa[0], edge["bulged_rec"])


# ---- 3. list lengths ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_list_lengths_around_a_workgroup(homo, sp, n):
    assert len(homo["bulged_rec"]) > 257 and len(homo["site_rec"]) > 257
    fixed, rows = bulged_table(homo["gen"], homo["bulged_rec"][:n], homo["texts"], sp["h_plain"])
    same_bytes(fixed, homo["f"][:n])
    same_bytes(rows, btc.bulged_rows(homo["bulged"][:n], homo["f"][:n], 1))
    rec, scores, rows = sites_table(homo["gen"], homo["site_rec"][:n], homo["texts"], sp["h_plain"])
    same_bytes(rec, homo["site_rec"][:n])
    same_bytes(scores, homo["scores"][:n])
    want_rows = btc.site_records(sp["plain"], homo["contigs"], homo["texts"], homo["sites"][:n], 1)[1]
    same_bytes(rows, want_rows)
    if n:
        keep = btc.cut(homo["site_rec"]["guide"][:n], homo["scores"]["top"][:n], max(n // 2, 1), 1)
        rec, scores, _ = sites_table(homo["gen"], homo["site_rec"][:n], homo["texts"], sp["h_plain"], top_k=max(n // 2, 1), min_score=1)
        same_bytes(rec, homo["site_rec"][:n][keep])
        same_bytes(scores, homo["scores"][:n][keep])


# ---- 4. records outside the definition score 0 ----------------------------------------------------------------------------
def test_records_outside_the_definition_score_zero(edge, sp):
    """Checks of bounded reads: hand-made records with a guide index that is too large, sizes 0 and 3, split points outside
    a + 1 .. e - 1, an unknown contig and positions behind the contig - each scores 0, its neighbours keep their scores."""
    n = len(edge["guides"])
    k = next(i for i, v in enumerate(edge["f"]) if v > 0 and edge["bulged"][i][4] == 2)
    r = edge["bulged"][k]
    k2 = next(i for i, v in enumerate(edge["f"]) if v > 0 and edge["bulged"][i][4] == -2)
    r2 = edge["bulged"][k2]
    clen = len(edge["contigs"][r[2]])
    info = lambda strand, kind, size, index, nm: strand << 31 | kind << 12 | size << 10 | index << 5 | nm
    made = [
        (r[0], r[2], r[3], bc.info_word(r[1], r[4], r[6], r[5])),           # as it is
        (n, r[2], r[3], bc.info_word(r[1], r[4], r[6], r[5])),              # guide >= n_guides
        (0xFFFFFFFF, r[2], r[3], bc.info_word(r[1], r[4], r[6], r[5])),
        (r[0], r[2], r[3], info(r[1], 0, 0, r[6], r[5])),                   # size 0
        (r[0], r[2], r[3], info(r[1], 0, 3, r[6], r[5])),                   # size 3
        (r[0], r[2], r[3], info(r[1], 0, 2, 0, r[5])),                      # i = a
        (r[0], r[2], r[3], info(r[1], 0, 2, 20, r[5])),                     # i = e
        (r[0], r[2], r[3], info(r[1], 0, 2, 31, r[5])),
        (r2[0], r2[2], r2[3], info(r2[1], 1, 2, 18, r2[5])),                # RNA 2: i + b = 20 > e - 1
        (r[0], len(edge["contigs"]), r[3], bc.info_word(r[1], r[4], r[6], r[5])),  # contig >= the genome's count
        (r[0], 0xFFFFFFFF, r[3], bc.info_word(r[1], r[4], r[6], r[5])),
        (r[0], r[2], clen - 24, bc.info_word(r[1], r[4], r[6], r[5])),      # the last of the 25 bases lies behind the contig
        (r[0], r[2], clen + 1000, bc.info_word(r[1], r[4], r[6], r[5])),
        (r[0], r[2], 0xFFFFFFF0, bc.info_word(r[1], r[4], r[6], r[5])),     # far behind every plane
        (r2[0], r2[2], r2[3], bc.info_word(r2[1], r2[4], r2[6], r2[5])),    # as it is
    ]
    rec = np.array(made, dtype=va.BULGE_HIT_DTYPE)
    want = np.zeros(len(made), dtype=np.uint32)
    want[0], want[-1] = edge["f"][k], edge["f"][k2]
    fixed, rows = bulged_table(edge["gen"], rec, edge["texts"], sp["h_zeroed"])
    same_bytes(fixed, want)
    assert int(rows["score_sum"].sum()) == int(want.sum()) and int(rows["positive"].sum()) == 2
    # sites: a guide that is too large, an unknown contig, an anchor behind the contig or in front of its first site, a best
    # alignment that is not among the members, no member at all
    j = next(i for i, s in enumerate(edge["scores"]) if s["top"] > 0 and len(edge["sites"][i][4]) >= 3)
    s = edge["site_rec"][j]
    sites = np.repeat(edge["site_rec"][j:j + 1], 9)
    sites["guide"][1] = n
    sites["contig"][2] = len(edge["contigs"])
    sites["anchor"][3] = 0xFFFFFF00
    sites["anchor"][4] = len(edge["contigs"][int(s["contig"])]) + 30
    sites["anchor"][5] = 3 if (int(s["info"]) >> 31) == 0 else len(edge["contigs"][int(s["contig"])]) - 3  # the span would leave the contig
    sites["members"][6] = int(s["members"]) | 31 << (5 * (bc.d_of_info(s["info"]) + 2))                   # the best's d is absent
    sites["members"][7] = 0x1FFFFFF
    want = np.zeros(9, dtype=va.SITE_SCORE_DTYPE)
    want[0] = want[8] = edge["scores"][j]
    got = sites_table(edge["gen"], sites, edge["texts"], sp["h_zeroed"])
    same_bytes(got[0], sites)
    same_bytes(got[1], want)
    assert int(got[2]["positive"].sum()) == 2


def test_sites_at_the_ends_of_contigs_and_of_the_planes(ctx, sp):
    """DNA-2 sites (25 bases) at the first and at the last base of a contig whose end is the genome's last plane word, and across
    word ends: the records come from the device's own searches, the scores from the restatement over them."""
    rng = np.random.default_rng(5)
    read = bc.distinct_read(rng)
    site = bc.plant(rng, read, 2, 9)
    first = bc.put(bc.rnd(rng, 71), 0, site)
    last = bc.rnd(rng, 32 * 3 + 31 - 25) + site  # ends at bit 30 of the last word: the next site would leave the planes
    mid = bc.put(bc.rnd(rng, 200), 32 * 3 + 31, site)  # starts at bit 31
    contigs = [first, mid, last]
    gen = ctx.load_genome(va.PackedGenome.from_sequences(contigs))
    try:
        rec, _, fixed, rows = gen.search_bulges([read], 3, dna=2, rna=2, table=sp["h_plain"])
        bulged = sc.bulged_of_records(rec)
        assert any(x[2] == 0 and x[3] == 0 and x[4] == 2 and x[5] == 0 for x in bulged)
        assert any(x[2] == 2 and x[3] + 25 == len(last) and x[4] == 2 and x[5] == 0 for x in bulged)
        assert any(x[2] == 1 and x[3] % 32 == 31 and x[4] == 2 and x[5] == 0 for x in bulged)
        f = btc.bulged_scored(contigs, [read], bulged, sp["plain"])
        same_bytes(fixed, f)
        same_bytes(rows, btc.bulged_rows(bulged, f, 1))
        hits = gen.search([read], 3, algorithm="scan")
        plain = sc.plain_of_hits(hits.to_numpy())
        hits.close()
        sites = sc.collapse(plain, bulged)
        got = gen.search_sites([read], 3, dna=2, rna=2, table=sp["h_plain"])
        want = btc.site_records(sp["plain"], contigs, [read], sites, 1)
        same_bytes(got[0], sc.arrays(sites, plain, bulged, 1)[0])
        same_bytes(got[2], want[0])
        same_bytes(got[3], want[1])
    finally:
        gen.close()


# ---- 5. the outputs, the refusals, repetition, the cache --------------------------------------------------------------------
def test_outputs_alone_and_select_null(edge, sp):
    gen, L = edge["gen"], va.lib()
    fixed, rows = bulged_table(gen, edge["bulged_rec"], edge["texts"], sp["h_zeroed"], rows=False)
    assert rows is None
    same_bytes(fixed, edge["f"])
    fixed, rows = bulged_table(gen, edge["bulged_rec"], edge["texts"], sp["h_zeroed"], records=False)
    assert fixed is None
    same_bytes(rows, btc.bulged_rows(edge["bulged"], edge["f"], len(edge["guides"])))
    rec, scores, rows = sites_table(gen, edge["site_rec"], edge["texts"], sp["h_zeroed"], rows=False)
    assert rows is None
    same_bytes(scores, edge["scores"])
    rec, scores, rows = sites_table(gen, edge["site_rec"], edge["texts"], sp["h_zeroed"], records=False)
    assert rec is None and scores is None
    same_bytes(rows, edge["rows"])
    # select == NULL is { 0, 0 }
    h, out = Handle(gen.ctx, edge["site_rec"], "sites"), C.c_void_p()
    try:
        texts, p = "".join(edge["texts"]).encode(), _lib.SiteParams(23, 0)
        args = (gen.ctx._h, gen._h, h._h, C.byref(p), texts, len(edge["texts"]), 23, sp["h_zeroed"]._h)
        assert L.vsc_sites_table(*args, None, C.byref(out), None) == 0
        data = C.c_void_p()
        assert L.vsc_sites_count(out) == 140 and L.vsc_sites_scores(out, C.byref(data)) == 0 and L.vsc_sites_scores_dev(out)
        assert bytes((C.c_char * (140 * 16)).from_address(data.value)) == edge["scores"].tobytes()
        L.vsc_sites_free(out)
        # the refusals
        rows = np.zeros(len(edge["texts"]), dtype=va.TABLE_ROW_DTYPE)
        assert L.vsc_sites_table(*args, None, None, None) == -22                                      # both outputs NULL
        assert L.vsc_sites_table(*args, C.byref(_lib.PatternSelect(1, 0, (0, 1))), C.byref(out), None) == -22 and not out.value
        bad = _lib.SiteParams(24, 0)
        assert L.vsc_sites_table(gen.ctx._h, gen._h, h._h, C.byref(bad), texts, len(edge["texts"]), 23, sp["h_zeroed"]._h, None, C.byref(out), None) == -22
        assert L.vsc_sites_table(gen.ctx._h, gen._h, h._h, C.byref(bad), texts, len(edge["texts"]), 24, sp["h_zeroed"]._h, None, C.byref(out), None) == -22
        assert "len" in L.vsc_last_error(gen.ctx._h).decode()
        assert L.vsc_sites_data(h._h, C.byref(data)) == 0 and L.vsc_sites_scores(h._h, C.byref(data)) == -22  # an unscored result
        assert L.vsc_sites_scores_dev(h._h) is None
        other = va.Context(0)
        try:
            assert L.vsc_sites_table(other._h, gen._h, h._h, C.byref(p), texts, len(edge["texts"]), 23, sp["h_zeroed"]._h, None, C.byref(out), None) == -22
        finally:
            other.close()
        assert L.vsc_sites_table(gen.ctx._h, gen._h, h._h, C.byref(p), b"U" * len(texts), len(edge["texts"]), 23, sp["h_zeroed"]._h, None, None,
                                 rows.ctypes.data) == -22                                             # a letter that is no IUPAC letter
    finally:
        h.close()
    b = Handle(gen.ctx, edge["bulged_rec"], "bulged")
    try:
        assert L.vsc_bulge_hits_table(gen.ctx._h, gen._h, b._h, texts, len(edge["texts"]), 23, sp["h_zeroed"]._h, None, None) == -22
        f = np.zeros(len(edge["bulged_rec"]), dtype=np.uint32)
        assert L.vsc_bulge_hits_table(gen.ctx._h, gen._h, b._h, texts, len(edge["texts"]), 24, sp["h_zeroed"]._h, f.ctypes.data, None) == -22
    finally:
        b.close()


def test_repetition_the_table_cache_and_the_timing_fields(ctx, edge, sp):
    gen = edge["gen"]
    h = Handle(ctx, edge["site_rec"], "sites")
    try:
        before = ctx.timing()
        run = lambda table, **k: gen._site_scores(h._h, _lib.SiteParams(23, 0), [t.encode() for t in edge["texts"]], table, k.get("top_k", 0), 0, True, True)
        a, b = run(sp["h_zeroed"]), run(sp["h_zeroed"])
        for got in (a, b):
            same_bytes(got[1], edge["scores"])
            same_bytes(got[2], edge["rows"])
        assert ctx.timing() == before  # the call leaves vsc_ctx_timing alone
        score, select, walk = C.c_double(-1), C.c_double(-1), C.c_double(-1)
        assert va.lib().vsc_debug_site_table_ms(ctx._h, C.byref(score), C.byref(select), C.byref(walk)) == 0
        assert score.value > 0 and select.value == 0 and walk.value == 0
        run(sp["h_zeroed"], top_k=2)
        assert va.lib().vsc_debug_site_table_ms(ctx._h, C.byref(score), C.byref(select), C.byref(walk)) == 0
        assert score.value > 0 and select.value > 0 and walk.value > 0
        # a second table with another serial number, then the first again: the device copy is keyed by the serial number
        other = btc.site_records(sp["plain"], edge["contigs"], edge["texts"], edge["sites"], len(edge["guides"]))
        assert other[0].tobytes() != edge["scores"].tobytes() and sp["h_plain"].info()["serial"] != sp["h_zeroed"].info()["serial"]
        same_bytes(run(sp["h_plain"])[1], other[0])
        same_bytes(run(sp["h_zeroed"])[1], edge["scores"])
        ctx.release_scratch()
        same_bytes(run(sp["h_zeroed"])[1], edge["scores"])
        same_bytes(bulged_table(gen, edge["bulged_rec"], edge["texts"], sp["h_plain"])[0],
                   btc.bulged_scored(edge["contigs"], edge["texts"], edge["bulged"], sp["plain"]))
        # the input is not modified
        data = C.c_void_p()
        assert va.lib().vsc_sites_data(h._h, C.byref(data)) == 0
        assert bytes((C.c_char * (len(edge["site_rec"]) * 32)).from_address(data.value)) == edge["site_rec"].tobytes()
    finally:
        h.close()


def test_search_sites_with_a_table_is_the_three_explicit_calls(edge, sp):
    gen, L, n = edge["gen"], va.lib(), len(edge["guides"])
    codes = va.pack_guides(edge["guides"])
    plain = gen.search(edge["guides"], bc.EDGE_M)
    bulged, sites = C.c_void_p(), C.c_void_p()
    p, bp = gen._params(bc.EDGE_M, None, "scan"), va.BulgeParams(2, 2, 0, 0, 0)
    try:
        va.api.check(L.vsc_search_bulges(gen.ctx._h, gen._h, codes.ctypes.data, n, C.byref(p), C.byref(bp), C.byref(bulged), None), gen.ctx._h)
        va.api.check(L.vsc_hits_sites(gen.ctx._h, plain._h, bulged, n, C.byref(_lib.SiteParams(23, 0)), C.byref(sites), None), gen.ctx._h)
        explicit = gen._site_scores(sites, _lib.SiteParams(23, 0), [t.encode() for t in va.unpack_guides(codes)], sp["h_zeroed"], 3, 1, True, True)
    finally:
        L.vsc_sites_free(sites)
        L.vsc_bulge_hits_free(bulged)
        plain.close()
    got = gen.search_sites(edge["guides"], bc.EDGE_M, dna=2, rna=2, table=sp["h_zeroed"], top_k=3, min_score=1)
    same_bytes(got[0], explicit[0])
    same_bytes(got[2], explicit[1])
    same_bytes(got[3], explicit[2])
    assert 0 < len(got[0]) < 140
    # without a table every return value is what it was
    old = gen.search_sites(edge["guides"], bc.EDGE_M, dna=2, rna=2)
    assert len(old) == 2 and old[0].tobytes() == edge["site_rec"].tobytes()
    assert len(gen.search_bulges(edge["guides"], bc.EDGE_M, dna=2, rna=2)) == 2


# ---- 6. the tools ---------------------------------------------------------------------------------------------------------
import math  # noqa: E402
import os  # noqa: E402
import subprocess  # noqa: E402

BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "varscot_amd", "bin")


def run(*a):
    return subprocess.run([os.path.join(BIN, a[0])] + list(a[1:]), capture_output=True, text=True, timeout=600)


def table_file(path):
    return [l.rstrip("\n").split("\t") for l in open(path)]


def check_tool_outputs(tmp_path, scores, rows, site_guides, K, floor):
    """with.tsv / sites.tsv (with -w) against before.tsv / sites0.tsv (without) and the restatement; cut.tsv under -K / -S."""
    old, new = table_file(tmp_path / "before.tsv"), table_file(tmp_path / "with.tsv")
    assert [r[:-3] for r in new] == old and new[0][-3:] == ["siteScoreSum", "siteSpecScore", "sitePositive"]
    for g, r in enumerate(new[1:]):
        total = int(rows["score_sum"][g])
        assert r[-3:] == ["%.6f" % (total * 2.0 ** -30), "%.0f" % math.floor(va.table_specificity(total) + 0.5), str(int(rows["positive"][g]))], g
    old, new = table_file(tmp_path / "sites0.tsv"), table_file(tmp_path / "sites.tsv")
    assert [r[:-2] for r in new] == old and new[0][-2:] == ["tableScore", "scoredAs"] and len(new) == len(scores) + 1
    want = [["%.9f" % (int(s["top"]) * 2.0 ** -30), "%+d" % (int(s["top_d"]) - 2) if int(s["top_d"]) != 2 else "0"] for s in scores]
    assert [r[-2:] for r in new[1:]] == want
    keep = btc.cut(site_guides, scores["top"], K, floor)
    assert 0 < len(keep) < len(scores)
    assert table_file(tmp_path / "cut.tsv") == [new[0]] + [new[1 + int(k)] for k in keep]


def test_guide_summary_bulge_table(tmp_path, edge, sp):
    names = ["c%d" % i for i in range(len(edge["contigs"]))]
    with open(tmp_path / "g.fa", "w") as f:
        for n, s in zip(names, edge["contigs"]):
            f.write(">%s\n%s\n" % (n, s))
    with open(tmp_path / "reads.fa", "w") as f:
        for i, g in enumerate(edge["guides"]):
            f.write(">g%d\n%s\n" % (i, g))
    t = sp["zeroed"]
    with open(tmp_path / "W.tsv", "w") as f:  # guide_summary's -W format: 'j g s w' and 'PAM XY w'
        for j in range(20):
            for g in range(4):
                for s in range(4):
                    if g != s:
                        f.write("%d %s %s %r\n" % (j, "ACGT"[g], "ACGT"[s], float(t["pair"][j, g, s])))
        for k in range(16):
            f.write("PAM %s%s %r\n" % ("ACGT"[k >> 2], "ACGT"[k & 3], float(t["pam"][k])))
    sp["h_zeroed"].to_tsv(str(tmp_path / "w.tsv"), base_path=str(tmp_path / "unused.tsv"))
    assert run("bidir_index", "-G", str(tmp_path / "g.fa"), "-I", str(tmp_path / "idx")).returncode == 0
    base = ["guide_summary", "-G", str(tmp_path / "g.fa"), "-I", str(tmp_path / "idx"), "-R", str(tmp_path / "reads.fa"), "-M", str(bc.EDGE_M),
            "-u", "2,2", "-W", str(tmp_path / "W.tsv")]
    r = run(*base, "-O", str(tmp_path / "before.tsv"), "-U", str(tmp_path / "u0.tsv"), "-Z", str(tmp_path / "sites0.tsv"))
    assert r.returncode == 0, r.stderr
    r = run(*base, "-O", str(tmp_path / "with.tsv"), "-U", str(tmp_path / "u1.tsv"), "-Z", str(tmp_path / "sites.tsv"), "-w", str(tmp_path / "w.tsv"))
    assert r.returncode == 0, r.stderr
    assert open(tmp_path / "u0.tsv").read() == open(tmp_path / "u1.tsv").read()  # the other outputs are what they were
    K, floor = 3, 0.01
    r = run(*base, "-O", str(tmp_path / "cut_sum.tsv"), "-Z", str(tmp_path / "cut.tsv"), "-w", str(tmp_path / "w.tsv"), "-K", str(K), "-S", str(floor))
    assert r.returncode == 0, r.stderr
    assert open(tmp_path / "cut_sum.tsv").read() == open(tmp_path / "with.tsv").read()  # the rows are over all sites
    check_tool_outputs(tmp_path, edge["scores"], edge["rows"], edge["site_rec"]["guide"], K, math.ceil(floor * 2 ** 30))


def test_pattern_search_bulge_table(tmp_path):
    e = sc.cas12a_scenario()
    n, L = len(e["guides"]), e["length"]
    table = btc.random_bulge_table(np.random.default_rng(77), btc.SHAPES["Cas12a"], zeros=10, ones=6)
    scores, rows = btc.site_records(table, e["contigs"], e["guides"], e["sites"], n, "start")
    t = btc.make_table(va, table)
    t.to_tsv(str(tmp_path / "w.tsv"), base_path=str(tmp_path / "W.tsv"))
    t.close()
    names = ["c%d" % i for i in range(len(e["contigs"]))]
    with open(tmp_path / "g.fa", "w") as f:
        for name, s in zip(names, e["contigs"]):
            f.write(">%s\n%s\n" % (name, s))
    with open(tmp_path / "q.fa", "w") as f:
        for i, g in enumerate(e["guides"]):
            f.write(">q%d\n%s\n" % (i, g))
    assert run("bidir_index", "-G", str(tmp_path / "g.fa"), "-I", str(tmp_path / "idx")).returncode == 0
    base = ["pattern_search", "-i", str(tmp_path / "idx"), "-q", e["pattern"], "-R", str(tmp_path / "q.fa"), "-M", str(e["m"]), "-u", "2,2",
            "-p", "%d,%d" % e["proto"], "-W", str(tmp_path / "W.tsv")]
    r = run(*base, "-O", str(tmp_path / "before.tsv"), "-T", str(tmp_path / "t0.tsv"), "-U", str(tmp_path / "u0.tsv"), "-Z", str(tmp_path / "sites0.tsv"))
    assert r.returncode == 0, r.stderr
    r = run(*base, "-O", str(tmp_path / "with.tsv"), "-T", str(tmp_path / "t1.tsv"), "-U", str(tmp_path / "u1.tsv"), "-Z", str(tmp_path / "sites.tsv"),
            "-w", str(tmp_path / "w.tsv"))
    assert r.returncode == 0, r.stderr
    for a, b in (("t0.tsv", "t1.tsv"), ("u0.tsv", "u1.tsv")):
        assert open(tmp_path / a).read() == open(tmp_path / b).read()
    K, floor = 2, 0.001
    r = run(*base, "-O", str(tmp_path / "cut_sum.tsv"), "-Z", str(tmp_path / "cut.tsv"), "-w", str(tmp_path / "w.tsv"), "-K", str(K), "-S", str(floor))
    assert r.returncode == 0, r.stderr
    assert open(tmp_path / "cut_sum.tsv").read() == open(tmp_path / "with.tsv").read()
    site_guides = [s[0][0] for s in e["sites"]]
    check_tool_outputs(tmp_path, scores, rows, site_guides, K, math.ceil(floor * 2 ** 30))
