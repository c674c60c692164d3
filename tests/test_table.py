"""vsc_score_hits_table / vsc_search_summary_table / vsc_search_select_table (and vsc_multi_search_summary_table) on the device:
per-hit scores equal vsc_table_score on the host bit for bit; the per-guide rows and the top-K by table score, taken over the
search kernel's records where they lie, equal - field by field, byte for byte - the numpy aggregation and cut of the record
route (Genome.search + the host's scores); CRISPOR's cfdOfftargetScore column comes back through the device."""
import ctypes as C
import os

import numpy as np
import pytest

import varscot_amd as va
from helpers import by_result_order, make_genome, mutate, random_guides, random_seq, revcomp
from layouts import LAYOUTS, check
from table_cases import (ONE, REL_TOL, cut_by_table, fixture_rows, fixture_table, host_scores, numpy_scores, random_table, record_route,
                         rows_of_hits, selected, site_text)
from varscot_amd import _lib

pytestmark = pytest.mark.gpu

G = "ACGTTGCATGCAAGTCCTAGTGG"
NONE = (0xFFFFFFFF, 0, 0)


@pytest.fixture(scope="module")
def ctx():
    c = va.Context(0)
    yield c
    c.close()


@pytest.fixture
def hooks(ctx):
    """ctx.set_debug(...) for one test (include/varscot_hip_debug.h); the defaults come back afterwards."""
    yield ctx.set_debug
    ctx.set_debug()


@pytest.fixture(scope="module")
def table():
    """A random table with a few weights of exactly 0 and 1."""
    t = va.ScoreTable(*random_table(np.random.default_rng(4020), zeros=12, ones=6))
    yield t
    t.close()


def same_rows(got, want):
    for f in want.dtype.names:
        assert np.array_equal(got[f], want[f]), f


# ------------------------------------------------------------------------------------ 1. per hit, bit for bit
@pytest.fixture(scope="module")
def planted(ctx):
    """70 guides (two output regions of the seed search) on two contigs of tens of kilobases; sites planted on both strands at
    p = 0, ending at a contig's end, across a 32-base word boundary, and in the second contig."""
    rng = np.random.default_rng(4021)
    guides = random_guides(rng, 69) + [G]
    contigs = make_genome(4021, [50_000, 30_011], guides, 5, n_plant=350, n_runs=2)
    loci = []
    # (a window that ends with its contig is a hit only within floor(m / 2) mismatches in its last 12 bases: those two sites
    # carry their substitutions in the other part of the read)
    for c, pos, strand, gi, nsub, lo, hi in ((0, 0, "+", 3, 2, 0, 20), (1, 0, "-", 4, 3, 0, 20), (0, 50_000 - 23, "-", 5, 3, 12, 20),
                                             (1, 30_011 - 23, "+", 6, 4, 0, 11), (0, 32 * 400 - 11, "+", 7, 3, 0, 20),
                                             (0, 32 * 500 - 22, "-", 8, 2, 0, 20), (1, 32 * 300 - 1, "+", 69, 5, 0, 20),
                                             (1, 32 * 303 - 12, "-", 69, 0, 0, 20)):
        site = mutate(rng, guides[gi], nsub, lo, hi)
        contigs[c] = contigs[c][:pos] + (revcomp(site) if strand == "-" else site) + contigs[c][pos + 23:]
        loci.append((gi, c, pos, int(strand == "-")))
    gen = ctx.load_genome(va.PackedGenome.from_sequences(contigs))
    yield dict(guides=guides, contigs=contigs, gen=gen, loci=loci)
    gen.close()


@pytest.mark.parametrize("algo", ["scan", "seed"])
def test_per_hit_scores_equal_the_host_function(ctx, table, planted, algo):
    p = planted
    h = p["gen"].search(p["guides"], 5, algorithm=algo)
    rec = h.to_numpy().copy()
    found = {(int(r["guide"]), int(r["contig"]), int(r["pos"]), int(r["info"]) >> 31) for r in rec}
    assert all(l in found for l in p["loci"]) and len(rec) > 300 and len({int(r["info"]) >> 31 for r in rec}) == 2
    x, f = h.table_scores(table)
    assert ctx.timing()["score_ms"] > 0
    want_x, want_f = host_scores(table, p["guides"], p["contigs"], rec)  # vsc_table_score, hit by hit
    assert x.view(np.uint64).tolist() == want_x.view(np.uint64).tolist() and f.tolist() == want_f.tolist()
    vx, vf = numpy_scores(table, p["guides"], p["contigs"], rec)  # ... and the vectorised restatement the larger cases use
    assert vx.view(np.uint64).tolist() == want_x.view(np.uint64).tolist() and vf.tolist() == want_f.tolist()
    assert (f == 0).any() and (f > 0).any() and f.max() <= ONE
    # a sub-range, and either output alone
    x2, f2 = h.table_scores(table, first=17, count=101)
    assert x2.tobytes() == x[17:118].tobytes() and f2.tobytes() == f[17:118].tobytes()
    assert h.table_scores(table, fixed=False)[1] is None and h.table_scores(table, scores=False)[0] is None
    assert h.table_scores(table, first=len(rec), count=0)[0].size == 0
    with pytest.raises(va.VarscotError, match="vsc_score_hits_table"):
        h.table_scores(table, first=len(rec), count=1)
    h.close()


# ------------------------------------------------------------------------------------ 2. rows and selections
@pytest.fixture(scope="module")
def tiled(ctx, table):
    """130 guides: three output regions of 64 reads.  A tandem array of 2 100 copies of a 5-mismatch site of G (guide 70), half
    of them on '-': more than 2 048 counted hits of one guide in one region, so its hits span tiles, all with the same score."""
    rng = np.random.default_rng(4022)
    guides = random_guides(rng, 129)
    guides.insert(70, G)
    while True:  # a 5-mismatch site that scores above 0 under the table
        site = mutate(rng, G, 5, 0, 20)
        if table.score(G, site) > 0:
            break
    contigs = [(site + "T") * 1050 + (revcomp(site) + "A") * 1050] + make_genome(4022, [40_000], guides, 5, n_plant=400, n_runs=2)
    gen = ctx.load_genome(va.PackedGenome.from_sequences(contigs))
    routes = {a: record_route(gen, table, guides, contigs, 5, a) for a in ("scan", "seed")}
    ex = [NONE] * len(guides)
    ex[70] = (0, 24 * 1000, 0)  # one copy of the tandem array
    for r in routes["scan"][0][::40]:  # and a hit of every 40th record's guide
        if ex[int(r["guide"])] == NONE:
            ex[int(r["guide"])] = (int(r["contig"]), int(r["pos"]), int(r["info"]) >> 31)
    yield dict(guides=guides, contigs=contigs, gen=gen, routes=routes, ex=ex)
    gen.close()


def rows_and_selections(ctx, table, t, algo, after=lambda fill=False: None):
    guides, gen = t["guides"], t["gen"]
    rec, _, f = t["routes"][algo]
    assert (rec["guide"] == 70).sum() >= 2100 and len(set(rec["guide"] // 64)) == 3
    plain, rows = gen.summarize_table(guides, 5, table, algorithm=algo, plain=True)
    after()
    tm = ctx.timing()
    same_rows(rows, rows_of_hits(rec, f, len(guides)))
    assert tm["hits"] == len(rec) and tm["score_ms"] > 0 and tm["sort_ms"] == 0
    assert plain.tobytes() == gen.summarize(guides, 5, algorithm=algo).tobytes()
    assert rows["reserved"].sum() == 0 and rows["positive"][70] >= 2100 and (rows["positive"] < plain["nm"].sum(axis=1)).any()
    # an excluded locus
    rows_ex = gen.summarize_table(guides, 5, table, algorithm=algo, exclude=t["ex"])
    after()
    want_ex = rows_of_hits(rec, f, len(guides), exclude=t["ex"])
    same_rows(rows_ex, want_ex)
    assert want_ex["positive"].sum() < rows["positive"].sum()
    # selections: top_k 1 and 5, a floor, both, the excluded locus
    floor = int(np.sort(f[f > 0])[len(f[f > 0]) // 2])
    for top_k, min_score, ex in ((1, 0, None), (5, 0, None), (0, floor, None), (3, floor // 2, None), (5, 0, t["ex"])):
        got = selected(gen, guides, 5, table, top_k=top_k, min_score=min_score, algorithm=algo, exclude=ex)
        after()
        want = cut_by_table(rec, f, top_k, min_score, exclude=ex)
        assert 0 < len(want) < len(rec) and got.tobytes() == want.tobytes(), (top_k, min_score)
    # equal scores (the tandem copies) are cut by strand, then position: all the '+' copies, then the first '-' ones
    got = selected(gen, guides, 5, table, top_k=1100, algorithm=algo)
    after()
    ranked = cut_by_table(rec, f, 1100, ranked=True)
    assert got.tobytes() == by_result_order(ranked).tobytes()
    mine = ranked[(ranked["guide"] == 70) & (ranked["contig"] == 0)]
    plus, minus = mine[mine["info"] >> 31 == 0], mine[mine["info"] >> 31 == 1]
    assert plus["pos"].tolist() == [24 * i for i in range(1050)] and 0 < len(minus) <= 50
    assert minus["pos"].tolist() == [24 * (1050 + i) for i in range(len(minus))]
    assert (mine["info"] >> 31).tolist() == sorted((mine["info"] >> 31).tolist())  # '+' ranks before '-'
    # the optional rows are summarize_table's
    got, rows2 = selected(gen, guides, 5, table, top_k=2, algorithm=algo, summary=True)
    after()
    assert rows2.tobytes() == rows.tobytes() and got.tobytes() == cut_by_table(rec, f, 2).tobytes()
    # nothing to decide: vsc_search's bytes (and no score kernel runs)
    assert selected(gen, guides, 5, table, algorithm=algo).tobytes() == rec.tobytes()
    after(fill=True)  # (the sort is then the records' only reader: the block fill table, not sentinels)


@pytest.mark.parametrize("algo", ["scan", "seed"])
def test_rows_and_selections_equal_the_record_route(ctx, table, tiled, algo):
    rows_and_selections(ctx, table, tiled, algo)


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_seed_rows_and_selections_under_every_layout(ctx, hooks, table, tiled, layout):
    hooks(**LAYOUTS[layout])
    rows_and_selections(ctx, table, tiled, "seed", after=lambda fill=False: check(ctx.timing(), layout, fill=fill))


def test_two_passes(ctx, table):
    rng = np.random.default_rng(4023)
    guides = random_guides(rng, 16_500)
    contigs = make_genome(4023, [300_000, 20_000], guides[::400], 3, n_plant=60)
    gen = ctx.load_genome(va.PackedGenome.from_sequences(contigs))
    for algo in ("scan", "seed"):
        rec, _, f = record_route(gen, table, guides, contigs, 6, algo)
        got, rows = selected(gen, guides, 6, table, top_k=2, algorithm=algo, summary=True)
        assert ctx.timing()["read_passes"] == 2 and ctx.timing()["hits"] == len(rec)
        same_rows(rows, rows_of_hits(rec, f, len(guides)))
        want = cut_by_table(rec, f, 2)
        assert 1000 < len(want) < len(rec)
        assert got.tobytes() == want.tobytes(), algo
        rows2 = gen.summarize_table(guides, 6, table, algorithm=algo)
        assert ctx.timing()["read_passes"] == 2 and rows2.tobytes() == rows.tobytes()
        assert (rows["positive"][16_384:] > 0).any()  # the second pass's reads
    gen.close()


# ------------------------------------------------------------------------------------ 3. CRISPOR's column through the device
def test_crispor_scores_through_the_device(ctx):
    fx = fixture_rows()
    cfd_table = fixture_table()
    gi = 0
    guide = fx["guides"][gi]
    pick = [i for i in np.flatnonzero(fx["guide"] == gi)
            if sum(a != b for a, b in zip(guide, fx["site"][i])) <= 8 and fx["site"][i][21:] in ("GG", "AG")][:300]
    assert len(pick) >= 100 and any(fx["cfd"][i] == 0 for i in pick) and any(fx["site"][i][21:] == "AG" for i in pick)
    spacer, where, parts = "T" * 9, {}, []
    for k, i in enumerate(pick):  # both strands
        where[(32 * k + len(spacer), k % 2)] = i
        parts.append(spacer + (revcomp(fx["site"][i]) if k % 2 else fx["site"][i]))
    contigs = ["".join(parts) + spacer]
    gen = ctx.load_genome(va.PackedGenome.from_sequences(contigs))
    for algo in ("scan", "seed"):
        h = gen.search([guide], 8, extra_pam="AG", algorithm=algo)
        rec = h.to_numpy().copy()
        x, f = h.table_scores(cfd_table)
        h.close()
        _, want_f = host_scores(cfd_table, [guide], contigs, rec)
        assert f.tolist() == want_f.tolist()
        seen = 0
        for r, score in zip(rec, x):
            i = where.get((int(r["pos"]), int(r["info"]) >> 31))
            if i is not None:
                seen += 1
                assert site_text(contigs, r) == fx["site"][i]
                assert score == 0.0 if fx["cfd"][i] == 0 else abs(score / fx["cfd"][i] - 1.0) <= REL_TOL, (i, score, fx["cfd"][i])
        assert seen == len(pick)
        rows = gen.summarize_table([guide], 8, cfd_table, extra_pam="AG", algorithm=algo)
        assert int(rows["score_sum"][0]) == int(want_f.sum()) and int(rows["positive"][0]) == int((want_f > 0).sum())
    gen.close()
    cfd_table.close()


# ------------------------------------------------------------------------------------ 4. shards, several contexts
@pytest.mark.parametrize("algo", ["scan", "seed"])
def test_rows_add_and_selections_compose_over_shards(ctx, table, algo):
    rng = np.random.default_rng(4024)
    guides = random_guides(rng, 9)
    contigs = make_genome(4024, [30_000, 9000, 25], guides, 6, n_plant=200, n_runs=1)
    packed = va.PackedGenome.from_sequences(contigs)
    whole = ctx.load_genome(packed)
    rec, _, f = record_route(whole, table, guides, contigs, 6, algo)
    want_rows = whole.summarize_table(guides, 6, table, algorithm=algo)
    want = selected(whole, guides, 6, table, top_k=3, algorithm=algo)
    whole.close()
    same_rows(want_rows, rows_of_hits(rec, f, len(guides)))
    assert want.tobytes() == cut_by_table(rec, f, 3).tobytes()
    for world in (2, 3):
        total = np.zeros(len(guides), dtype=_lib.TABLE_ROW_DTYPE)
        parts = []
        for rank in range(world):
            g = ctx.load_genome(packed, rank, world)
            rows = g.summarize_table(guides, 6, table, algorithm=algo)
            for name in total.dtype.names:
                total[name] += rows[name]
            parts.append(selected(g, guides, 6, table, top_k=3, algorithm=algo))
            g.close()
        assert total.tobytes() == want_rows.tobytes(), world
        union = np.concatenate(parts)
        assert len(union) > len(want)
        _, uf = numpy_scores(table, guides, contigs, union)
        assert cut_by_table(union, uf, 3).tobytes() == want.tobytes(), world


def test_multi_summary_table_equals_one_context(ctx, table):
    rng = np.random.default_rng(4025)
    guides = random_guides(rng, 10)
    contigs = make_genome(4025, [40_000, 12_000, 30], guides, 6, n_plant=200, n_runs=1)
    packed = va.PackedGenome.from_sequences(contigs)
    gen = ctx.load_genome(packed)
    want = {a: gen.summarize_table(guides, 6, table, algorithm=a, plain=True) for a in ("scan", "seed")}
    gen.close()
    m = va.MultiContext([0, 0])
    try:
        g = m.load_genome(packed)
        for a in ("scan", "seed"):
            plain, rows = g.summarize_table(guides, 6, table, algorithm=a, plain=True)
            assert plain.tobytes() == want[a][0].tobytes() and rows.tobytes() == want[a][1].tobytes(), a
            assert rows["score_sum"].sum() > 0
            assert g.summarize_table(guides, 6, table, algorithm=a).tobytes() == rows.tobytes()
        with pytest.raises(va.VarscotError, match="vsc_multi_search_summary_table"):
            g.summarize_table(guides, 6, table, exclude=[(3, 0, 0)] * len(guides))
        g.close()
    finally:
        m.close()


# ------------------------------------------------------------------------------------ 5. no existing behaviour moves
def test_existing_calls_return_the_same_bytes_around_a_table_call(ctx, table, tmp_path):
    from classified_cases import SYNTHETIC_ACTIVITIES, synthetic_forest
    from varscot_amd.classifier import Forest
    rng = np.random.default_rng(4026)
    guides = random_guides(rng, 70)
    contigs = make_genome(4026, [60_000, 20_000], guides, 6, n_plant=400, n_runs=2)
    gen = ctx.load_genome(va.PackedGenome.from_sequences(contigs))
    path = str(tmp_path / "forest.vscrf")
    synthetic_forest(path, np.random.default_rng(8031), 8, 31)
    forest = Forest(path)
    act = rng.choice(SYNTHETIC_ACTIVITIES, size=len(guides))

    def existing(algo):
        out = [gen.summarize(guides, 6, algorithm=algo).tobytes()]
        h = gen.search_select(guides, 6, top_k=20, algorithm=algo)
        out.append(h.to_numpy().tobytes())
        h.close()
        h = gen.search(guides, 6, algorithm=algo)
        out.append(h.to_numpy().tobytes())
        h.close()
        plain, votes = gen.summarize_classified(guides, 6, forest, act, algorithm=algo)
        return out + [plain.tobytes(), votes.tobytes()]

    for algo in ("scan", "seed"):
        before = existing(algo)
        rows = gen.summarize_table(guides, 6, table, algorithm=algo)
        got = selected(gen, guides, 6, table, top_k=4, algorithm=algo)
        assert existing(algo) == before, algo
        ctx.release_scratch()
        assert gen.summarize_table(guides, 6, table, algorithm=algo).tobytes() == rows.tobytes()
        assert selected(gen, guides, 6, table, top_k=4, algorithm=algo).tobytes() == got.tobytes()
        assert existing(algo) == before, algo
        # another table replaces the context's copy; the first one comes back with its own bytes
        other = va.ScoreTable(*random_table(np.random.default_rng(77)))
        assert gen.summarize_table(guides, 6, other, algorithm=algo).tobytes() != rows.tobytes()
        other.close()
        assert gen.summarize_table(guides, 6, table, algorithm=algo).tobytes() == rows.tobytes()
    gen.close()


# ------------------------------------------------------------------------------------ 6. degenerate and invalid
def test_degenerate_inputs(ctx, table):
    rng = np.random.default_rng(4027)
    contigs = [random_seq(rng, 20_000)]
    gen = ctx.load_genome(va.PackedGenome.from_sequences(contigs))
    guides = random_guides(rng, 5)
    for algo in ("scan", "seed"):
        # no guides
        assert len(gen.summarize_table([], 3, table, algorithm=algo)) == 0
        assert len(selected(gen, [], 3, table, top_k=2, algorithm=algo)) == 0
        # no hits
        rows = gen.summarize_table(guides, 0, table, algorithm=algo)
        assert not any(rows[f].any() for f in rows.dtype.names)
        got, rows = selected(gen, guides, 0, table, top_k=2, algorithm=algo, summary=True)
        assert len(got) == 0 and not rows["score_sum"].any()
    # an all-zero table: every hit scores 0, none is positive; a floor of 1 keeps nothing, no floor keeps them all
    pair = np.zeros((20, 4, 4))
    for b in range(4):
        pair[:, b, b] = 1.0
    zero = va.ScoreTable(pair, np.zeros(16))
    planted = [contigs[0][:5000] + mutate(rng, g, 2, 0, 20) + contigs[0][5023:] for g in guides[:1]]
    gen2 = ctx.load_genome(va.PackedGenome.from_sequences(planted))
    for algo in ("scan", "seed"):
        h = gen2.search(guides, 4, algorithm=algo)
        rec = h.to_numpy().copy()
        x, f = h.table_scores(zero)
        h.close()
        assert len(rec) >= 1 and not x.any() and not f.any()
        rows = gen2.summarize_table(guides, 4, zero, algorithm=algo)
        assert not any(rows[name].any() for name in rows.dtype.names)
        assert len(selected(gen2, guides, 4, zero, min_score=1, algorithm=algo)) == 0
        assert selected(gen2, guides, 4, zero, top_k=1000, algorithm=algo).tobytes() == rec.tobytes()
    zero.close()
    gen2.close()
    gen.close()


def test_invalid_arguments_name_the_call(ctx, table):
    L = va.lib()
    rng = np.random.default_rng(4028)
    gen = ctx.load_genome(va.PackedGenome.from_sequences([random_seq(rng, 5000)]))
    codes = va.pack_guides(random_guides(rng, 3))
    p = va.Genome._params(3, None, "scan")
    rows = np.zeros(3, dtype=va.TABLE_ROW_DTYPE)
    sel = _lib.Select()
    h = C.c_void_p()
    ptr = _lib.ptr
    assert L.vsc_search_summary_table(ctx._h, gen._h, ptr(codes), 3, C.byref(p), None, None, None, ptr(rows)) == -22
    assert b"vsc_search_summary_table" in L.vsc_last_error(ctx._h)
    assert L.vsc_search_summary_table(ctx._h, gen._h, ptr(codes), 3, C.byref(p), None, table._h, None, None) == -22
    assert L.vsc_search_summary_table(None, gen._h, ptr(codes), 3, C.byref(p), None, table._h, None, ptr(rows)) == -22
    assert L.vsc_search_select_table(ctx._h, gen._h, ptr(codes), 3, C.byref(p), C.byref(sel), None, None, None, C.byref(h)) == -22
    assert b"vsc_search_select_table" in L.vsc_last_error(ctx._h) and not h.value
    assert L.vsc_search_select_table(ctx._h, gen._h, ptr(codes), 3, C.byref(p), None, None, table._h, None, C.byref(h)) == -22
    assert L.vsc_search_select_table(ctx._h, gen._h, ptr(codes), 3, C.byref(p), C.byref(sel), None, table._h, None, None) == -22
    sel.reserved[0] = 1
    assert L.vsc_search_select_table(ctx._h, gen._h, ptr(codes), 3, C.byref(p), C.byref(sel), None, table._h, None, C.byref(h)) == -22
    with pytest.raises(va.VarscotError, match="vsc_search_summary_table"):
        gen.summarize_table(codes, 3, table, exclude=[(9, 0, 0)] * 3)
    with pytest.raises(va.VarscotError, match="between 0 and 8"):
        gen.summarize_table(codes, 9, table)
    hits = gen.search(codes, 3)
    assert L.vsc_score_hits_table(ctx._h, gen._h, hits._h, ptr(codes), 3, 0, 0, None, None, None) == -22
    assert b"vsc_score_hits_table" in L.vsc_last_error(ctx._h)
    other = va.Context(0)
    gen_other = other.load_genome(va.PackedGenome.from_sequences([random_seq(rng, 5000)]))
    x = np.zeros(max(len(hits), 1))
    assert L.vsc_score_hits_table(ctx._h, gen_other._h, hits._h, ptr(codes), 3, 0, len(hits), table._h, ptr(x), None) == -22
    gen_other.close()
    other.close()
    hits.close()
    gen.close()


# ------------------------------------------------------------------------------------ 7. guide_summary -W
def test_guide_summary_tool_table_columns_and_listing(tmp_path, ctx):
    import subprocess
    BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "varscot_amd", "bin")
    rng = np.random.default_rng(4029)
    pair, pam = random_table(rng, zeros=8)
    tab = va.ScoreTable(pair, pam)
    with open(tmp_path / "w.tsv", "w") as f:
        f.write("# a random table\n")
        for j in range(20):
            for g in range(4):
                for s in range(4):
                    if g != s:
                        f.write("%d\t%s\t%s\t%r\n" % (j, "ACGT"[g], "ACGT"[s], float(pair[j, g, s])))
        for a in range(4):
            for b in range(4):
                f.write("PAM\t%s%s\t%r\n" % ("ACGT"[a], "ACGT"[b], float(pam[4 * a + b])))
    assert va.ScoreTable.from_tsv(str(tmp_path / "w.tsv")).pair.tobytes() == tab.pair.tobytes()
    guides = random_guides(rng, 6)
    contigs = make_genome(4029, [15_000, 6000], guides, 5, n_plant=150, n_runs=1, edge_plants=False)
    names = ["chr1 assembled", "chr2"]
    loci = []
    for i, g in enumerate(guides):  # the on-targets of the BED file
        c, pos, strand = i % 2, 300 + 700 * i, i % 3 == 0
        contigs[c] = contigs[c][:pos] + (revcomp(g) if strand else g) + contigs[c][pos + 23:]
        loci.append((c, pos, int(strand)))
    ids = ["g%d" % i for i in range(len(guides))]
    with open(tmp_path / "g.fa", "w") as f:
        for n, s in zip(names, contigs):
            f.write(">%s\n%s\n" % (n, "\n".join(s[i:i + 60] for i in range(0, len(s), 60))))
    with open(tmp_path / "on.bed", "w") as f:
        for i, (c, pos, strand) in zip(ids, loci):
            f.write("%s\t%d\t%d\t%s\t0\t%s\n" % (names[c].split()[0], pos, pos + 23, i, "-" if strand else "+"))
    run = lambda *a: subprocess.run([os.path.join(BIN, a[0])] + list(a[1:]), capture_output=True, text=True, timeout=600)
    assert run("bidir_index", "-G", str(tmp_path / "g.fa"), "-I", str(tmp_path / "idx")).returncode == 0
    base = ["guide_summary", "-G", str(tmp_path / "g.fa"), "-I", str(tmp_path / "idx"), "-M", "5", "-B", str(tmp_path / "on.bed")]
    r = run(*base, "-O", str(tmp_path / "plain.tsv"))
    assert r.returncode == 0, r.stderr
    plain = (tmp_path / "plain.tsv").read_text().splitlines()
    gen = ctx.load_genome(va.PackedGenome.from_sequences(contigs))
    rows = gen.summarize_table(guides, 5, tab, exclude=loci)
    rec, _, fixed = record_route(gen, tab, guides, contigs, 5, "auto")
    h = gen.search(guides, 5)
    mit = h.scores(mit=True)[0]
    h.close()
    gen.close()
    assert rows["score_sum"].sum() > 0
    for dev in ([], ["-D", "0,0"]):
        r = run(*base, "-W", str(tmp_path / "w.tsv"), "-O", str(tmp_path / "tab.tsv"), *dev)
        assert r.returncode == 0, r.stderr
        got = (tmp_path / "tab.tsv").read_text().splitlines()
        assert got[0] == plain[0] + "\ttableScoreSum\ttableSpecScore\ttablePositive"
        for i, line in enumerate(got[1:]):
            s = int(rows["score_sum"][i])
            want = ["%.6f" % (s * 2.0 ** -30), "%d" % np.floor(va.table_specificity(s) + 0.5), str(rows["positive"][i])]
            assert line == plain[1 + i] + "\t" + "\t".join(want), (dev, i)
    # the listing by table score: rank order, tableScore last; the summary beside it is the same
    score = {(int(x["guide"]), int(x["contig"]), int(x["pos"]), int(x["info"])): float(np.rint(m * 2.0 ** 24)) for x, m in zip(rec, mit)}
    tscore = {(int(x["guide"]), int(x["contig"]), int(x["pos"]), int(x["info"])): int(v) for x, v in zip(rec, fixed)}
    for opts, sel in ((["-K", "5"], (5, 0)), (["-K", "3", "-S", "0.01"], (3, int(np.ceil(0.01 * 2.0 ** 30))))):
        ranked = cut_by_table(rec, fixed, sel[0], sel[1], exclude=loci, ranked=True)
        want = "#guideId\trank\tchrom\tstart\tend\tstrand\tmismatches\tmismatchPositions\tmitScore\tsequence\ttableScore\n"
        rank, last = 0, -1
        for x in ranked:
            g, c, p, info = int(x["guide"]), int(x["contig"]), int(x["pos"]), int(x["info"])
            rank, last = (rank + 1 if g == last else 1), g
            pos = [str(b) for b in range(23) if (info >> b) & 1]
            want += "%s\t%d\t%s\t%d\t%d\t%s\t%d\t%s\t%.6f\t%s\t%.9f\n" % (
                ids[g], rank, names[c].split()[0], p, p + 23, "-" if info >> 31 else "+", (info >> 23) & 31, ",".join(pos) or "-",
                score[(g, c, p, info)] * 2.0 ** -24, contigs[c][p:p + 23], tscore[(g, c, p, info)] * 2.0 ** -30)
        assert want.count("\n") > 6
        r = run(*base, "-W", str(tmp_path / "w.tsv"), "-O", str(tmp_path / "v.tsv"), "-T", str(tmp_path / "v.hits.tsv"), *opts)
        assert r.returncode == 0, r.stderr
        assert (tmp_path / "v.hits.tsv").read_text() == want, opts
        assert (tmp_path / "v.tsv").read_text() == (tmp_path / "tab.tsv").read_text()
    # a table that lacks entries is refused by name
    (tmp_path / "short.tsv").write_text("3\tA\tC\t0.5\n")
    r = run(*base, "-W", str(tmp_path / "short.tsv"))
    assert r.returncode == 1 and "-W" in r.stderr
    # a weight outside 0 .. 1 is out of range, not missing; a line with a field too many is no entry
    text = (tmp_path / "w.tsv").read_text().splitlines()
    (tmp_path / "neg.tsv").write_text("\n".join(text + ["3\tA\tC\t-1"]) + "\n")
    r = run(*base, "-W", str(tmp_path / "neg.tsv"))
    assert r.returncode == 1 and "0 .. 1" in r.stderr and "lacks" not in r.stderr
    (tmp_path / "more.tsv").write_text("\n".join(text + ["3\tA\tC\t0.5\t0.7"]) + "\n")
    r = run(*base, "-W", str(tmp_path / "more.tsv"))
    assert r.returncode == 1 and "neither" in r.stderr
    tab.close()
