"""vsc_search_pattern_table on the device: the records byte for byte vsc_search_pattern's, f per record the host's score of the
guide and the site's text, both kinds of rows and the selection byte for byte what the restatement gives
(tests/pattern_table_cases.py) - over the lengths, the PAM places and the budgets; the SpCas9 anchor against the plain path's
table scores; ties across the K-th place; the radix select digit by digit and behind the first group of cells; the rounds; the outputs, the cap, shards, repetition, the table cache; and
design_pattern(table=)."""
import ctypes as C

import numpy as np
import pytest

import varscot_amd as va
import pattern_cases as pc
import pattern_table_cases as tc
from helpers import make_genome, random_guides
from table_cases import fixture_table

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = va.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def sel():
    s = dict(tc.select_scenario())
    s["rec"], s["rows"] = pc.arrays(s["hits"], len(s["guides"]))
    s["trows"] = tc.table_rows(s["hits"], s["f"], len(s["guides"]))
    s["obj"] = tc.make_table(va, s["table"])
    return s


@pytest.fixture(scope="module")
def sel_gen(ctx, sel):
    g = ctx.load_genome(va.PackedGenome.from_sequences(sel["contigs"]))
    yield g
    g.close()


def same(got, rec, f, rows, trows):
    """(records, f, NM rows, table rows) of a call against the restatement's arrays."""
    assert got[0].dtype == va.PATTERN_HIT_DTYPE and got[1].dtype == np.uint32 and got[3].dtype == va.TABLE_ROW_DTYPE
    assert len(got[0]) == len(rec) == len(got[1])
    assert got[0].tobytes() == rec.tobytes()
    assert got[1].tobytes() == np.asarray(f, dtype=np.uint32).tobytes()
    assert got[2].tobytes() == rows.tobytes()
    assert got[3].tobytes() == trows.tobytes()


# ---- 1. the edge layout over lengths, PAM places and budgets --------------------------------------------------------------
@pytest.mark.parametrize("place", pc.PLACES)
@pytest.mark.parametrize("L", [16, 23, 32])
def test_edge_layout_equals_the_restatement(ctx, L, place):
    t = tc.edge_table(L, place)
    e, n = t["e"], len(t["e"]["guides"])
    table = tc.make_table(va, t["table"])
    gen = ctx.load_genome(va.PackedGenome.from_sequences(e["contigs"]))
    try:
        for m in (0, 3, 8):
            hits, f = tc.at(t, m)
            assert hits and {h[1] for h in hits} == {0, 1}
            got = gen.search_pattern_table(e["pattern"], e["guides"], m, table)
            plain = gen.search_pattern(e["pattern"], e["guides"], m)
            assert got[0].tobytes() == plain[0].tobytes() and got[2].tobytes() == plain[1].tobytes()
            for r, v in zip(got[0], got[1]):  # f = the host's score of the guide and the site's text
                text = tc.site_text(e["contigs"], L, int(r["info"] >> 31), int(r["contig"]), int(r["pos"]))
                assert table.score(e["guides"][r["guide"]], text, fixed=True)[1] == v
            rec, rows = pc.arrays(hits, n)
            same(got, rec, f, rows, tc.table_rows(hits, f, n))
    finally:
        gen.close()


# ---- 2. the anchor: the plain path's table scores -------------------------------------------------------------------------
def test_anchor_equals_the_plain_table_scores(ctx):
    m = 4
    guides = random_guides(np.random.default_rng(41), 8)
    contigs = make_genome(41, [14000, 5000, 40], guides, m, n_plant=80, n_runs=3)
    plain_table = fixture_table()
    table = va.PatternTable.from_score_table(plain_table)
    gen = ctx.load_genome(va.PackedGenome.from_sequences(contigs))
    try:
        hits = gen.search(guides, m, algorithm="scan")
        plain = hits.to_numpy()
        _, plain_f = hits.table_scores(plain_table)
        rec, f, _, _ = gen.search_pattern_table("N" * 21 + "GR", guides, m, table)
    finally:
        gen.close()
    a = {(int(r["guide"]), int(r["info"] >> 31), int(r["contig"]), int(r["pos"])): int(v) for r, v in zip(plain, plain_f)}
    b = {(int(r["guide"]), int(r["info"] >> 31), int(r["contig"]), int(r["pos"])): int(v) for r, v in zip(rec, f)}
    assert len(a) >= 20 and set(a) <= set(b)
    assert all(b[k] == v for k, v in a.items())                                  # bit for bit on every shared record
    assert any(0 < v < tc.ONE for v in a.values())
    at_end = lambda k: k[3] + 23 == len(contigs[k[2]])
    assert all(at_end(k) for k in set(b) - set(a)) and any(at_end(k) for k in b)  # the pattern-only records: right-edge windows


# ---- 3. ties across the K-th place, the floor ------------------------------------------------------------------------------
def test_tandem_top_k_keeps_the_first_in_record_order(ctx):
    t = pc.tandem_scenario()
    rng = np.random.default_rng(3)
    table = tc.random_pattern_table(rng, (23, (0, 20), (21, 22)))
    f = tc.scored(t["contigs"], t["guides"], t["hits"], table)
    rec, rows = pc.arrays(t["hits"], 2)
    trows = tc.table_rows(t["hits"], f, 2)
    values, counts = np.unique(f, return_counts=True)
    tied = int(values[counts.argmax()])
    assert (f == tied).sum() >= 200 and tied > 1
    obj = tc.make_table(va, table)
    gen = ctx.load_genome(va.PackedGenome.from_sequences(t["contigs"]))
    try:
        same(gen.search_pattern_table(t["pattern"], t["guides"], t["m"], obj), rec, f, rows, trows)
        for k in (1, 64, 65, 100, 1000):
            keep = tc.cut(t["hits"], f, top_k=k)
            same(gen.search_pattern_table(t["pattern"], t["guides"], t["m"], obj, top_k=k), rec[keep], f[keep], rows, trows)
        better = [i for i in range(len(f)) if f[i] > tied and t["hits"][i][0] == 0]
        copies = [i for i in range(len(f)) if f[i] == tied and t["hits"][i][0] == 0]
        keep = tc.cut(t["hits"], f, top_k=len(better) + 70)
        assert [i for i in keep if t["hits"][i][0] == 0 and f[i] == tied] == copies[:70]   # the FIRST ties in record order
        for floor in (tied + 1, tied, tied - 1):
            keep = tc.cut(t["hits"], f, min_score=floor)
            assert (floor > tied) == (not set(copies) & set(keep.tolist()))
            same(gen.search_pattern_table(t["pattern"], t["guides"], t["m"], obj, min_score=floor), rec[keep], f[keep], rows, trows)
    finally:
        gen.close()


@pytest.mark.parametrize("batch", [0, 1])
def test_selection_scenario(sel, sel_gen, batch):
    p, gs, m, obj, hits, f = sel["pattern"], sel["guides"], sel["m"], sel["obj"], sel["hits"], sel["f"]
    same(sel_gen.search_pattern_table(p, gs, m, obj, guide_batch=batch), sel["rec"], f, sel["rows"], sel["trows"])
    for kw in (dict(top_k=sel["K"]), dict(min_score=sel["floor"]), dict(top_k=sel["K"], min_score=sel["floor"]), dict(top_k=1),
               dict(min_score=1), dict(top_k=153), dict(min_score=tc.ONE), dict(min_score=tc.ONE + 1)):
        keep = tc.cut(hits, f, **kw)
        got = sel_gen.search_pattern_table(p, gs, m, obj, guide_batch=batch, **kw)
        same(got, sel["rec"][keep], f[keep], sel["rows"], sel["trows"])   # the rows are over all hits, whatever is kept


def digits_fixture(ctx, s):
    """A digits scenario with the restatement's arrays, its cut per case, the table and the resident genome."""
    s = dict(s)
    s["rec"], s["rows"] = pc.arrays(s["hits"], len(s["guides"]))
    s["trows"] = tc.table_rows(s["hits"], s["f"], len(s["guides"]))
    s["keep"] = {case: tc.cut(s["hits"], s["f"], *case) for case in s["cases"]}
    s["obj"] = tc.make_table(va, s["table"])
    s["gen"] = ctx.load_genome(va.PackedGenome.from_sequences(s["contigs"]))
    return s


@pytest.fixture(scope="module")
def digits(ctx):
    s = digits_fixture(ctx, tc.digits_scenario())
    yield s
    s["gen"].close()
    s["obj"].close()


@pytest.fixture(scope="module")
def wide(ctx):
    s = digits_fixture(ctx, tc.digits_wide())
    yield s
    s["gen"].close()
    s["obj"].close()


def test_selection_digit_by_digit(digits):
    """digits_scenario(): thresholds that share one, two and three digits with their neighbours, ties over the steps of the walk,
    T = 0, floors at and beside T - every case of the list, under three round sizes."""
    s = digits
    p, gs, m, obj, gen, rec, f = s["pattern"], s["guides"], s["m"], s["obj"], s["gen"], s["rec"], s["f"]
    same(gen.search_pattern_table(p, gs, m, obj), rec, f, s["rows"], s["trows"])  # the search and the scores first: a failure below is the selection's
    for batch in (0, 1, 3):
        for (top_k, min_score), keep in s["keep"].items():
            got = gen.search_pattern_table(p, gs, m, obj, top_k=top_k, min_score=min_score, guide_batch=batch)
            assert len(got[0]) == len(keep), (batch, top_k, min_score)
            same(got, rec[keep], f[keep], s["rows"], s["trows"])


def test_selection_beyond_the_first_group_of_cells(ctx, wide):
    """digits_wide(): at guide_batch = 64 the segments of guides 59 to 62 begin in the second group of 64 x 64 cells, and guides
    64 and 65 are a round of their own; at 16 every round has one group.  The cap counts the survivors there as well."""
    s = wide
    p, gs, m, obj, gen, rec, f = s["pattern"], s["guides"], s["m"], s["obj"], s["gen"], s["rec"], s["f"]
    same(gen.search_pattern_table(p, gs, m, obj, guide_batch=64), rec, f, s["rows"], s["trows"])
    assert ctx.timing()["passes"] == 2
    for batch in (64, 16):
        for (top_k, min_score), keep in s["keep"].items():
            got = gen.search_pattern_table(p, gs, m, obj, top_k=top_k, min_score=min_score, guide_batch=batch)
            assert len(got[0]) == len(keep), (batch, top_k, min_score)
            same(got, rec[keep], f[keep], s["rows"], s["trows"])
    (top_k, min_score), keep = next(iter(s["keep"].items()))  # the case that truncates inside a second-group guide's ties
    n = len(keep)
    assert 0 < n < len(rec)
    same(gen.search_pattern_table(p, gs, m, obj, top_k=top_k, min_score=min_score, guide_batch=64, max_hits=n), rec[keep], f[keep], s["rows"], s["trows"])
    with pytest.raises(va.VarscotError) as err:
        gen.search_pattern_table(p, gs, m, obj, top_k=top_k, min_score=min_score, guide_batch=64, max_hits=n - 1)
    assert err.value.code == -34 and (" %d records" % n) in str(err.value)


# ---- 4. rounds ------------------------------------------------------------------------------------------------------------
def test_guide_batch_never_changes_the_bytes(ctx):
    s = pc.many_guides_scenario()
    table = tc.random_pattern_table(np.random.default_rng(8), tc.shape_of(s["pattern"]), zeros=20, ones=4)
    f = tc.scored(s["contigs"], s["guides"], s["hits"], table)
    rec, rows = pc.arrays(s["hits"], 70)
    trows = tc.table_rows(s["hits"], f, 70)
    floor = int(np.median(f[f > 0]))
    obj = tc.make_table(va, table)
    gen = ctx.load_genome(va.PackedGenome.from_sequences(s["contigs"]))
    try:
        for kw in (dict(), dict(top_k=3), dict(min_score=floor)):
            keep = tc.cut(s["hits"], f, **kw)
            assert {66, 69} <= {s["hits"][k][0] for k in keep}   # the second round of 64 keeps records of its own
            for batch in (1, 16, 64):
                same(gen.search_pattern_table(s["pattern"], s["guides"], s["m"], obj, guide_batch=batch, **kw), rec[keep], f[keep], rows, trows)
                assert ctx.timing()["passes"] == -(-70 // batch)
    finally:
        gen.close()


# ---- 5. outputs and state -------------------------------------------------------------------------------------------------
def test_rows_and_records_alone(sel, sel_gen):
    p, gs, m, obj = sel["pattern"], sel["guides"], sel["m"], sel["obj"]
    rec, f, rows, trows = sel_gen.search_pattern_table(p, gs, m, obj, records=False, top_k=1)
    assert rec is None and f is None and rows.tobytes() == sel["rows"].tobytes() and trows.tobytes() == sel["trows"].tobytes()
    rec, f, rows, trows = sel_gen.search_pattern_table(p, gs, m, obj, rows=False)
    assert rows is None and trows is None and rec.tobytes() == sel["rec"].tobytes() and f.tobytes() == sel["f"].tobytes()
    # table rows alone, through the C interface
    L, out = va.lib(), np.zeros(len(gs), dtype=va.TABLE_ROW_DTYPE)
    pp = va.PatternParams(m, 0, 0)
    assert L.vsc_search_pattern_table(sel_gen.ctx._h, sel_gen._h, p.encode(), "".join(gs).encode(), len(gs), 23, C.byref(pp), obj._h, None,
                                      None, None, out.ctypes.data) == 0
    assert out.tobytes() == sel["trows"].tobytes()
    assert sel_gen.ctx.timing()["hits"] == len(sel["hits"])


def test_max_hits_counts_the_survivors(sel, sel_gen):
    p, gs, m, obj = sel["pattern"], sel["guides"], sel["m"], sel["obj"]
    keep = tc.cut(sel["hits"], sel["f"], top_k=sel["K"])
    n = len(keep)
    assert n < len(sel["hits"])
    for batch in (0, 2):
        with pytest.raises(va.VarscotError) as err:
            sel_gen.search_pattern_table(p, gs, m, obj, top_k=sel["K"], max_hits=n - 1, guide_batch=batch)
        assert err.value.code == -34 and (" %d records" % n) in str(err.value)
        got = sel_gen.search_pattern_table(p, gs, m, obj, top_k=sel["K"], max_hits=n, guide_batch=batch)
        same(got, sel["rec"][keep], sel["f"][keep], sel["rows"], sel["trows"])
    with pytest.raises(va.VarscotError) as err:
        sel_gen.search_pattern_table(p, gs, m, obj, max_hits=n)
    assert err.value.code == -34 and (" %d records" % len(sel["hits"])) in str(err.value)


def test_no_guides(sel, sel_gen):
    rec, f, rows, trows = sel_gen.search_pattern_table(sel["pattern"], [], 3, sel["obj"], top_k=2)
    assert len(rec) == 0 and len(f) == 0 and rows.shape == (0, 9) and trows.shape == (0,)


def test_shards_add_and_merge(ctx, sel):
    packed = va.PackedGenome.from_sequences(sel["contigs"])
    recs, fs, rows, trows = [], [], np.zeros_like(sel["rows"]), np.zeros_like(sel["trows"])
    for rank in range(2):
        g = ctx.load_genome(packed, rank, 2)
        r, f, w, t = g.search_pattern_table(sel["pattern"], sel["guides"], sel["m"], sel["obj"])
        g.close()
        recs.append(r)
        fs.append(f)
        rows += w
        for name in ("score_sum", "positive", "positive_nm"):
            trows[name] += t[name]
    assert all(len(r) > 0 for r in recs)
    merged, f = np.concatenate(recs), np.concatenate(fs)
    order = pc.merge_order(merged)
    assert merged[order].tobytes() == sel["rec"].tobytes() and f[order].tobytes() == sel["f"].tobytes()
    assert rows.tobytes() == sel["rows"].tobytes() and trows.tobytes() == sel["trows"].tobytes()


def test_repetition_table_swap_and_the_unscored_search_beside_it(ctx, sel, sel_gen):
    p, gs, m, obj = sel["pattern"], sel["guides"], sel["m"], sel["obj"]
    before = sel_gen.search_pattern(p, gs, m)
    a = sel_gen.search_pattern_table(p, gs, m, obj, top_k=sel["K"])
    t = ctx.timing()
    b = sel_gen.search_pattern_table(p, gs, m, obj, top_k=sel["K"])
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert t["score_ms"] > 0 and t["scan_ms"] > 0 and t["passes"] == 1
    # another table between two calls takes effect: the device copy is keyed by the serial number
    other = dict(sel["table"])
    other["pair"] = np.where(sel["table"]["pair"] == 1.0, 1.0, 0.5 * sel["table"]["pair"])
    f2 = tc.scored(sel["contigs"], gs, sel["hits"], other)
    assert (f2 != sel["f"]).any()
    obj2 = tc.make_table(va, other)
    assert obj2.info()["serial"] != obj.info()["serial"]
    same(sel_gen.search_pattern_table(p, gs, m, obj2), sel["rec"], f2, sel["rows"], tc.table_rows(sel["hits"], f2, len(gs)))
    same(sel_gen.search_pattern_table(p, gs, m, obj), sel["rec"], sel["f"], sel["rows"], sel["trows"])
    ctx.release_scratch()  # the pools and the table come back on the next call
    same(sel_gen.search_pattern_table(p, gs, m, obj), sel["rec"], sel["f"], sel["rows"], sel["trows"])
    after = sel_gen.search_pattern(p, gs, m)
    assert before[0].tobytes() == after[0].tobytes() == sel["rec"].tobytes() and before[1].tobytes() == after[1].tobytes()
    assert ctx.timing()["score_ms"] == 0
    # the f words belong to a scored result only
    L, h = va.lib(), C.c_void_p()
    pp = va.PatternParams(m, 0, 0)
    assert L.vsc_search_pattern(ctx._h, sel_gen._h, p.encode(), "".join(gs).encode(), len(gs), 23, C.byref(pp), C.byref(h), None) == 0
    side = C.c_void_p()
    assert L.vsc_pattern_hits_scores(h, C.byref(side)) == -22 and L.vsc_pattern_hits_scores_dev(h) is None
    L.vsc_pattern_hits_free(h)


def test_refusals_on_the_device(ctx, sel, sel_gen):
    p, gs, m = sel["pattern"], sel["guides"], sel["m"]
    with pytest.raises(va.VarscotError) as err:
        sel_gen.search_pattern_table(p, gs, m, sel["obj"], records=False, rows=False)
    assert err.value.code == -22 and "vsc_search_pattern_table" in str(err.value)
    shorter = tc.make_table(va, tc.random_pattern_table(np.random.default_rng(1), (22, (0, 19), (20, 21))))
    with pytest.raises(va.VarscotError) as err:
        sel_gen.search_pattern_table(p, gs, m, shorter)
    assert err.value.code == -22
    L, rows = va.lib(), np.zeros((len(gs), 9), dtype=np.uint32)
    pp, ps = va.PatternParams(m, 0, 0), va.PatternSelect(1, 0)
    ps.reserved[0] = 1
    args = (ctx._h, sel_gen._h, p.encode(), "".join(gs).encode(), len(gs), 23, C.byref(pp), sel["obj"]._h, C.byref(ps), None, rows.ctypes.data, None)
    assert L.vsc_search_pattern_table(*args) == -22
    ps.reserved[0] = 0
    assert L.vsc_search_pattern_table(*args) == 0 and rows.tobytes() == sel["rows"].tobytes()


# ---- 6. design_pattern(table=) ----------------------------------------------------------------------------------------------
def test_design_pattern_with_a_table(sel, sel_gen):
    p, m, obj = sel["pattern"], sel["m"], sel["obj"]
    targets = [(0, 380, 460), (0, 4380, 4440), (0, 1000, 1100)]
    found, rows, trows = sel_gen.design_pattern(p, (0, 20), m, targets=targets, table=obj)
    plain = sel_gen.design_pattern(p, (0, 20), m, targets=targets)
    assert len(found) >= 3 and plain[0].codes.tobytes() == found.codes.tobytes() and plain[1].tobytes() == rows.tobytes()
    queries, own = found.text(), found.text(spell_pam=True)
    _, _, want_rows, want = sel_gen.search_pattern_table(p, queries, m, obj, records=False)
    for i in range(len(found)):  # the own locus, by hand
        f = tc.py_fixed(tc.py_score(sel["table"], queries[i], own[i]))
        assert f > 0
        want["score_sum"][i] -= f
        want["positive"][i] -= 1
        want["positive_nm"][i, 0] -= 1
        want_rows[i, 0] -= 1
    assert trows.tobytes() == want.tobytes() and rows.tobytes() == want_rows.tobytes()
    assert trows["score_sum"].max() > 0                                            # the tandem copies see each other


def test_pattern_search_tool_with_a_table(tmp_path, sel, sel_gen):
    """pattern_search -W / -K / -S against the Python route: the summary's three columns, the listing's tableScore column."""
    import math
    import os
    import subprocess
    bin_dir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "varscot_amd", "bin")
    p, gs, m, obj = sel["pattern"], sel["guides"], sel["m"], sel["obj"]
    (tmp_path / "g.fa").write_text(">c0 text\n%s\n" % sel["contigs"][0])
    (tmp_path / "guides.fa").write_text("".join(">g%d\n%s\n" % (i, g) for i, g in enumerate(gs)))
    obj.to_tsv(str(tmp_path / "table.tsv"))
    run = lambda *a: subprocess.run([os.path.join(bin_dir, a[0])] + list(a[1:]), capture_output=True, text=True, timeout=600)
    assert run("bidir_index", "-G", str(tmp_path / "g.fa"), "-I", str(tmp_path / "idx")).returncode == 0
    common = ("pattern_search", "-i", str(tmp_path / "idx"), "-q", p, "-R", str(tmp_path / "guides.fa"), "-M", str(m), "-W", str(tmp_path / "table.tsv"))
    floor = sel["floor"] / tc.ONE
    assert math.ceil(floor * tc.ONE) == sel["floor"]
    for name, extra, kw in (("all", (), dict()), ("cut", ("-K", str(sel["K"]), "-S", repr(floor)), dict(top_k=sel["K"], min_score=sel["floor"]))):
        r = run(*common, "-O", str(tmp_path / (name + "_sum.tsv")), "-T", str(tmp_path / (name + "_hits.tsv")), *extra)
        assert r.returncode == 0, r.stderr
        rec, f, rows, trows = sel_gen.search_pattern_table(p, gs, m, obj, **kw)
        lines = [l.rstrip("\n").split("\t") for l in open(tmp_path / (name + "_sum.tsv"))]
        assert lines[0] == ["#guideId", "guideSeq", "offtargetCount"] + ["mm%d" % k for k in range(m + 1)] + ["tableScoreSum", "tableSpecScore", "tablePositive"]
        for g, row in enumerate(lines[1:]):
            counts = [int(x) for x in rows[g, :m + 1]]
            spec = "%.0f" % math.floor(va.table_specificity(int(trows["score_sum"][g])) + 0.5)
            assert row == ["g%d" % g, gs[g], str(sum(counts))] + [str(x) for x in counts] + \
                ["%.6f" % (int(trows["score_sum"][g]) / tc.ONE), spec, str(int(trows["positive"][g]))]
        assert len(lines) == 1 + len(gs)
        lines = [l.rstrip("\n").split("\t") for l in open(tmp_path / (name + "_hits.tsv"))]
        assert lines[0][-2:] == ["sequence", "tableScore"] and len(lines) == 1 + len(rec)
        for l, r_, v in zip(lines[1:], rec, f):
            assert l[0] == "g%d" % r_["guide"] and l[2] == str(r_["pos"]) and l[4] == "+-"[int(r_["info"] >> 31)] and l[-1] == "%.9f" % (int(v) / tc.ONE)
    # without -W every output is what it was
    r = run(*common[:-2], "-O", str(tmp_path / "plain_sum.tsv"), "-T", str(tmp_path / "plain_hits.tsv"))
    assert r.returncode == 0, r.stderr
    assert open(tmp_path / "plain_sum.tsv").readline().rstrip("\n").split("\t")[-1] == "mm%d" % m
    assert open(tmp_path / "plain_hits.tsv").readline().rstrip("\n").split("\t")[-1] == "sequence"
