"""vsc_search_summary_classified / vsc_search_select_classified (and vsc_multi_search_summary_classified) on the device: the
classifier's per-guide rows and the top-K by votes, taken over the search kernel's records where they lie, equal - field by
field, byte for byte - the numpy aggregation and cut of the record route: Genome.search + Forest.classify_hits, itself pinned
to oracle/rf_oracle.py by test_classifier.py.  The order of a cut is np.lexsort over (-votes, strand, global position)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import varscot_amd as va
from classified_cases import (NONE, SYNTHETIC_ACTIVITIES, by_result_order, cut_by_votes, oracle_votes, record_route, rows_of_hits,
                              synthetic_forest)
from helpers import make_genome, random_guides, random_seq, real_guides, revcomp, selected
from varscot_amd import _lib
from varscot_amd.classifier import DEFAULT_MODEL, Forest, feature_names

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "varscot_amd", "bin")
G = "ACGTTGCATGCAAGTCCTAGTGG"


@pytest.fixture(scope="module")
def ctx():
    c = va.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def synth(tmp_path_factory):
    """8 trees x 31 nodes: the even tree count makes ties and equal votes common."""
    path = str(tmp_path_factory.mktemp("forest") / "synthetic.vscrf")
    synthetic_forest(path, np.random.default_rng(8031), 8, 31)
    forest = Forest(path)
    forest.path = path
    return forest


@pytest.fixture(scope="module")
def shipped(ctx, golden_dir):
    """The shipped forest over the 16 real guides with their TUSCAN activities: genome, both algorithms' record routes."""
    _, guides, acts = real_guides(golden_dir)
    contigs = make_genome(31, [150000, 40000], guides, 7, n_plant=900, n_runs=2)
    gen = ctx.load_genome(va.PackedGenome.from_sequences(contigs))
    forest = Forest(DEFAULT_MODEL)
    act = np.array(acts, dtype=np.float64)
    routes = {a: record_route(gen, forest, guides, act, 7, a) for a in ("scan", "seed")}
    yield dict(guides=guides, act=act, contigs=contigs, gen=gen, forest=forest, routes=routes)
    gen.close()


# ------------------------------------------------------------------------------------ 1. parity, shipped forest
@pytest.mark.parametrize("algo", ["scan", "seed"])
def test_shipped_forest_rows_and_selections_equal_the_record_route(ctx, shipped, algo):
    s = shipped
    rec, votes = s["routes"][algo]
    n_trees = s["forest"].n_trees
    share = (2 * votes.astype(np.int64) > n_trees).mean()
    print("hits %d, active share %.4f" % (len(rec), share))
    assert len(rec) > 600 and 0 < share < 1
    plain, rows = s["gen"].summarize_classified(s["guides"], 7, s["forest"], s["act"], algorithm=algo)
    t = ctx.timing()
    want = rows_of_hits(rec, votes, len(s["guides"]), n_trees)
    for f in want.dtype.names:
        assert np.array_equal(rows[f], want[f]), f
    assert plain.tobytes() == s["gen"].summarize(s["guides"], 7, algorithm=algo).tobytes()
    assert t["hits"] == len(rec) and t["score_ms"] > 0 and t["sort_ms"] == 0
    assert np.array_equal(va.expected_active(rows, n_trees), want["votes_sum"] / float(n_trees))
    for top_k, min_votes in ((5, 0), (0, 501), (3, 200)):
        got = selected(s["gen"], s["guides"], 7, s["forest"], s["act"], top_k=top_k, min_votes=min_votes, algorithm=algo)
        assert got.tobytes() == cut_by_votes(rec, votes, top_k, min_votes).tobytes(), (top_k, min_votes)
        assert ctx.timing()["hits"] == len(rec) and ctx.timing()["score_ms"] > 0 and ctx.timing()["sort_ms"] >= 0


# ------------------------------------------------------------------------------------ 2. direct restatement
def test_shipped_forest_rows_equal_the_oracle_forest_over_the_oracle_hits(ctx, shipped, oracle):
    """Seed search, m = 7, against oracle/rf_oracle.py over the oracle's own hits and feature rows: no device classify path."""
    from oracle.rf_oracle import Forest as OracleForest
    s = shipped
    hits = oracle.search(s["contigs"], s["guides"], 7, mode=oracle.MODE_PREDICATE)
    of = OracleForest(DEFAULT_MODEL)
    cols = {n: i for i, n in enumerate(feature_names())}
    x = np.zeros((len(hits), 443))
    for i, h in enumerate(hits):
        off = s["contigs"][h["contig"]][h["pos"]:h["pos"] + 23]
        x[i, :442] = oracle.feature_row(s["guides"][h["guide"]], revcomp(off) if h["info"] >> 31 else off)
        x[i, 442] = s["act"][h["guide"]]
    votes = oracle_votes(of, x[:, [cols[n] for n in of.names]])
    for i in range(0, len(hits), max(1, len(hits) // 12)):  # a sample through the oracle's own loop
        assert votes[i] == of.votes({n: x[i, cols[n]] for n in of.names})
    share = (2 * votes > of.n_trees).mean()
    print("oracle hits %d, active share %.4f" % (len(hits), share))
    assert 0 < share < 1
    _, rows = s["gen"].summarize_classified(s["guides"], 7, s["forest"], s["act"], algorithm="seed")
    want = rows_of_hits(hits, votes, len(s["guides"]), of.n_trees)
    for f in want.dtype.names:
        assert np.array_equal(rows[f], want[f]), f
    got = selected(s["gen"], s["guides"], 7, s["forest"], s["act"], top_k=5, algorithm="seed")
    assert got.tobytes() == cut_by_votes(hits, votes, 5).tobytes()


# ------------------------------------------------------------------------------------ 3. tiles and regions
@pytest.fixture(scope="module")
def tiled(ctx, synth):
    rng = np.random.default_rng(303)
    guides = random_guides(rng, 129)
    guides.insert(70, G)  # 130 guides: three output regions of 64 reads; G's segment spans several tiles
    # (the 200 kbp of random sequence carry planted near-matches of all 130 guides: every output region holds records)
    contigs = [(G + "T") * 6000] + make_genome(303, [200_000], guides, 4, n_plant=400, n_runs=2)
    gen = ctx.load_genome(va.PackedGenome.from_sequences(contigs))
    act = rng.choice(SYNTHETIC_ACTIVITIES, size=len(guides))
    yield dict(guides=guides, gen=gen, act=act)
    gen.close()


@pytest.mark.parametrize("algo", ["scan", "seed"])
def test_tiles_and_regions(ctx, synth, tiled, algo):
    guides, gen, act = tiled["guides"], tiled["gen"], tiled["act"]
    rec, votes = record_route(gen, synth, guides, act, 4, algo)
    assert (rec["guide"] == 70).sum() >= 6000 and len(set(rec["guide"] // 64)) == 3
    plain, rows = gen.summarize_classified(guides, 4, synth, act, algorithm=algo)
    want = rows_of_hits(rec, votes, len(guides), synth.n_trees)
    for f in want.dtype.names:
        assert np.array_equal(rows[f], want[f]), f
    assert plain.tobytes() == gen.summarize(guides, 4, algorithm=algo).tobytes()
    assert want["ties"].sum() >= 1  # the even tree count at work
    got = selected(gen, guides, 4, synth, act, top_k=7, algorithm=algo)
    ranked, v = cut_by_votes(rec, votes, 7, ranked=True)
    assert got.tobytes() == by_result_order(ranked).tobytes()
    same = (ranked["guide"][1:] == ranked["guide"][:-1]) & (v[1:] == v[:-1])
    assert same.any()  # equal votes inside a guide's top 7: the tie-break decided


# ------------------------------------------------------------------------------------ 4. equal votes
@pytest.mark.parametrize("algo", ["scan", "seed"])
def test_equal_votes_are_cut_by_strand_and_position(ctx, synth, algo):
    guides = [G] * 40
    gen = ctx.load_genome(va.PackedGenome.from_sequences([(G + "T") * 6000]))
    act = np.full(40, 0.5)
    got = selected(gen, guides, 0, synth, act, top_k=100, algorithm=algo)
    gen.close()
    assert len(got) == 4000
    for g in range(40):
        mine = got[got["guide"] == g]
        assert np.array_equal(mine["pos"], 24 * np.arange(100)) and not (mine["info"] >> 31).any() and not mine["contig"].any()


# ------------------------------------------------------------------------------------ 5. two passes
def test_two_passes(ctx, synth):
    rng = np.random.default_rng(78)
    guides = random_guides(rng, 16_500)
    contigs = make_genome(78, [300_000, 20_000], guides[::400], 3, n_plant=60)
    gen = ctx.load_genome(va.PackedGenome.from_sequences(contigs))
    act = rng.choice(SYNTHETIC_ACTIVITIES, size=len(guides))
    for algo in ("scan", "seed"):
        rec, votes = record_route(gen, synth, guides, act, 6, algo)
        got, plain, rows = selected(gen, guides, 6, synth, act, top_k=2, algorithm=algo, summary=True)
        assert ctx.timing()["read_passes"] == 2 and ctx.timing()["hits"] == len(rec)
        want = rows_of_hits(rec, votes, len(guides), synth.n_trees)
        for f in want.dtype.names:
            assert np.array_equal(rows[f], want[f]), (algo, f)
        cut = cut_by_votes(rec, votes, 2)
        assert 1000 < len(cut) < len(rec)
        assert got.tobytes() == cut.tobytes(), algo
        _, rows2 = gen.summarize_classified(guides, 6, synth, act, algorithm=algo)
        assert ctx.timing()["read_passes"] == 2
        assert rows2.tobytes() == rows.tobytes() and plain["nm"].sum() == len(rec)
    gen.close()


# ------------------------------------------------------------------------------------ 6. exclusion
@pytest.mark.parametrize("algo", ["scan", "seed"])
def test_the_excluded_locus_is_neither_counted_nor_selected(ctx, synth, algo):
    rng = np.random.default_rng(606)
    guides = random_guides(rng, 70)
    contigs = [random_seq(rng, 60_000), random_seq(rng, 30_000)]
    ex = []
    for i, g in enumerate(guides):  # the on-targets: every third guide on '-', the last ten without a locus
        c, pos, strand = i % 2, 500 + 400 * i, int(i % 3 == 0)
        if i >= 60:
            ex.append(NONE)
            continue
        contigs[c] = contigs[c][:pos] + (revcomp(g) if strand else g) + contigs[c][pos + 23:]
        ex.append((c, pos, strand))
    gen = ctx.load_genome(va.PackedGenome.from_sequences(contigs))
    act = rng.choice(SYNTHETIC_ACTIVITIES, size=len(guides))
    rec, votes = record_route(gen, synth, guides, act, 5, algo)
    plain, rows = gen.summarize_classified(guides, 5, synth, act, algorithm=algo, exclude=ex)
    want = rows_of_hits(rec, votes, len(guides), synth.n_trees, exclude=ex)
    assert want["votes_sum"].sum() < rows_of_hits(rec, votes, len(guides), synth.n_trees)["votes_sum"].sum()
    for f in want.dtype.names:
        assert np.array_equal(rows[f], want[f]), f
    assert plain.tobytes() == gen.summarize(guides, 5, algorithm=algo, exclude=ex).tobytes()
    assert plain["on_target"][:60].all() and not plain["on_target"][60:].any()
    for top_k in (0, 2):
        got = selected(gen, guides, 5, synth, act, top_k=top_k, algorithm=algo, exclude=ex)
        assert got.tobytes() == cut_by_votes(rec, votes, top_k, exclude=ex).tobytes(), top_k
        assert len(got) and not any((int(h["contig"]), int(h["pos"]), int(h["info"] >> 31)) == ex[h["guide"]] for h in got)
    gen.close()


# ------------------------------------------------------------------------------------ 7. shards, several contexts
@pytest.mark.parametrize("algo", ["scan", "seed"])
def test_rows_add_and_selections_compose_over_shards(ctx, synth, algo):
    rng = np.random.default_rng(707)
    guides = random_guides(rng, 9)
    contigs = make_genome(707, [30000, 9000, 25], guides, 6, n_plant=200, n_runs=1)
    packed = va.PackedGenome.from_sequences(contigs)
    act = rng.choice(SYNTHETIC_ACTIVITIES, size=len(guides))
    whole = ctx.load_genome(packed)
    rec, votes = record_route(whole, synth, guides, act, 6, algo)
    _, want_rows = whole.summarize_classified(guides, 6, synth, act, algorithm=algo)
    want = selected(whole, guides, 6, synth, act, top_k=3, algorithm=algo)
    whole.close()
    assert want.tobytes() == cut_by_votes(rec, votes, 3).tobytes()
    lookup = {(int(h["guide"]), int(h["contig"]), int(h["pos"]), int(h["info"])): int(v) for h, v in zip(rec, votes)}
    total = np.zeros(len(guides), dtype=_lib.VOTES_DTYPE)
    parts = []
    for rank in range(3):
        g = ctx.load_genome(packed, rank, 3)
        _, rows = g.summarize_classified(guides, 6, synth, act, algorithm=algo)
        for f in total.dtype.names:
            total[f] += rows[f]
        parts.append(selected(g, guides, 6, synth, act, top_k=3, algorithm=algo))
        g.close()
    assert total.tobytes() == want_rows.tobytes()
    union = np.concatenate(parts)
    assert len(union) > len(want)
    v = [lookup[(int(h["guide"]), int(h["contig"]), int(h["pos"]), int(h["info"]))] for h in union]
    assert cut_by_votes(union, v, 3).tobytes() == want.tobytes()


@pytest.mark.parametrize("k", [1, 3])
def test_multi_summary_classified_equals_one_context(ctx, synth, k):
    rng = np.random.default_rng(708)
    guides = random_guides(rng, 10)
    contigs = make_genome(708, [40000, 12000, 30], guides, 6, n_plant=200, n_runs=1)
    packed = va.PackedGenome.from_sequences(contigs)
    act = rng.choice(SYNTHETIC_ACTIVITIES, size=len(guides))
    gen = ctx.load_genome(packed)
    want = {a: gen.summarize_classified(guides, 6, synth, act, algorithm=a) for a in ("scan", "seed")}
    gen.close()
    m = va.MultiContext([0] * k)
    try:
        g = m.load_genome(packed)
        for a in ("scan", "seed"):
            plain, rows = g.summarize_classified(guides, 6, synth, act, algorithm=a)
            assert plain.tobytes() == want[a][0].tobytes() and rows.tobytes() == want[a][1].tobytes(), a
            assert rows["votes_sum"].sum() > 0
        with pytest.raises(va.VarscotError, match="vsc_multi_search_summary_classified"):
            g.summarize_classified(guides, 6, synth, act, exclude=[(3, 0, 0)] * len(guides))
        g.close()
    finally:
        m.close()


# ------------------------------------------------------------------------------------ 8. degenerate and invalid
def test_degenerate_inputs(ctx, synth):
    rng = np.random.default_rng(808)
    gen = ctx.load_genome(va.PackedGenome.from_sequences([(G + "T") * 300 + "T" * 500]))
    none = np.zeros(0, dtype=np.uint64)
    plain, rows = gen.summarize_classified(none, 3, synth, [])
    assert len(plain) == 0 and len(rows) == 0
    assert len(selected(gen, none, 3, synth, [], top_k=3)) == 0
    # a guide with no hit beside one with many
    guides = ["TTTTTTTTTTTTTTTTTTTTTGG", G]
    act = np.array([0.5, 1.02])
    for algo in ("scan", "seed"):
        rec, votes = record_route(gen, synth, guides, act, 2, algo)
        assert (rec["guide"] == 1).sum() >= 300 and not (rec["guide"] == 0).any()
        _, rows = gen.summarize_classified(guides, 2, synth, act, algorithm=algo)
        assert rows.tobytes() == rows_of_hits(rec, votes, 2, synth.n_trees).tobytes() and not rows[0].tobytes().strip(b"\0")
        assert selected(gen, guides, 2, synth, act, top_k=4, algorithm=algo).tobytes() == cut_by_votes(rec, votes, 4).tobytes()
    gen.close()
    # a genome with no hit at all
    empty = ctx.load_genome(va.PackedGenome.from_sequences(["N" * 500 + random_seq(np.random.default_rng(1), 3000)]))
    five = random_guides(rng, 5)
    for algo in ("scan", "seed"):
        assert len(record_route(empty, synth, five, np.full(5, 0.5), 0, algo)[0]) == 0
        plain, rows = empty.summarize_classified(five, 0, synth, np.full(5, 0.5), algorithm=algo)
        assert not plain.tobytes().strip(b"\0") and not rows.tobytes().strip(b"\0")
        assert len(selected(empty, five, 0, synth, np.full(5, 0.5), top_k=2, algorithm=algo)) == 0
    empty.close()


def test_invalid_arguments_name_the_call(ctx, synth):
    L = va.lib()
    gen = ctx.load_genome(va.PackedGenome.from_sequences([(G + "T") * 30]))
    codes = va.pack_guides([G, G])
    act = np.array([0.5, 0.5])
    p = _lib.SearchParams(2, 0, b"", _lib.ALGO_AUTO)
    rows = np.zeros(2, dtype=_lib.VOTES_DTYPE)

    def model(n_trees=None):
        return _lib.RfModel(synth.n_trees if n_trees is None else n_trees, synth.n_nodes, _lib.ptr(synth.status), _lib.ptr(synth.feature),
                            _lib.ptr(synth.left), _lib.ptr(synth.right), _lib.ptr(synth.split), _lib.ptr(synth.node_class))

    def classify(m="ok", activity="ok", reserved=0):
        mp = C.pointer(model()) if m == "ok" else m
        return _lib.Classify(mp, _lib.ptr(act) if activity == "ok" else None, (C.c_uint32 * 2)(0, reserved))

    def bad_loci(contig, strand):
        ex = np.zeros(2, dtype=_lib.LOCUS_DTYPE)
        ex["contig"] = 0xFFFFFFFF
        ex["contig"][1], ex["strand"][1] = contig, strand
        return ex

    sel = _lib.SelectVotes(2, 0, (C.c_uint32 * 2)(0, 0))
    spoilt = {
        "null cls": dict(cls=None),
        "null model": dict(cls=classify(m=C.POINTER(_lib.RfModel)())),
        "null activity": dict(cls=classify(activity=None)),
        "cls reserved": dict(cls=classify(reserved=1)),
        "no trees": dict(cls=classify(m=C.pointer(model(0)))),
        "70 000 trees": dict(cls=classify(m=C.pointer(model(70000)))),
        "excluded contig": dict(ex=bad_loci(5, 0)),
        "excluded strand": dict(ex=bad_loci(0, 2)),
        "null select": dict(sel=None),
        "select reserved": dict(sel=_lib.SelectVotes(2, 0, (C.c_uint32 * 2)(1, 0))),
    }
    for what, a in spoilt.items():
        cls = a.get("cls", classify())
        cls_arg = C.byref(cls) if cls is not None else None
        ex = _lib.ptr(a["ex"]) if "ex" in a else None
        if "sel" not in a:
            rc = L.vsc_search_summary_classified(ctx._h, gen._h, _lib.ptr(codes), 2, C.byref(p), ex, cls_arg, None, _lib.ptr(rows))
            assert rc == -22 and L.vsc_last_error(ctx._h).decode().startswith("vsc_search_summary_classified: "), what
        h = C.c_void_p()
        s = a.get("sel", sel)
        rc = L.vsc_search_select_classified(ctx._h, gen._h, _lib.ptr(codes), 2, C.byref(p), C.byref(s) if s is not None else None, cls_arg, ex,
                                            None, None, C.byref(h))
        assert rc == -22 and h.value is None and L.vsc_last_error(ctx._h).decode().startswith("vsc_search_select_classified: "), what
    rc = L.vsc_search_summary_classified(ctx._h, gen._h, _lib.ptr(codes), 2, C.byref(p), None, C.byref(classify()), None, None)
    assert rc == -22 and L.vsc_last_error(ctx._h).decode() == "vsc_search_summary_classified: null argument"
    # n_guides == 0: nothing to do, whatever the activities
    assert L.vsc_search_summary_classified(ctx._h, gen._h, None, 0, C.byref(p), None, C.byref(classify(activity=None)), None, None) == 0
    gen.close()


# ------------------------------------------------------------------------------------ 9. no existing behaviour moves
def test_existing_calls_return_the_same_bytes_around_a_classified_call(ctx, synth):
    rng = np.random.default_rng(909)
    guides = random_guides(rng, 70)
    contigs = make_genome(909, [80000, 20000], guides, 6, n_plant=400, n_runs=2)
    gen = ctx.load_genome(va.PackedGenome.from_sequences(contigs))
    act = rng.choice(SYNTHETIC_ACTIVITIES, size=len(guides))

    def existing(algo):
        out = [gen.summarize(guides, 6, algorithm=algo).tobytes()]
        h = gen.search_select(guides, 6, top_k=20, algorithm=algo)
        out.append(h.to_numpy().tobytes())
        h.close()
        h = gen.search(guides, 6, algorithm=algo)
        out.append(synth.classify_hits(h, act)[0].tobytes())
        h.close()
        return out

    for algo in ("scan", "seed"):
        before = existing(algo)
        _, rows = gen.summarize_classified(guides, 6, synth, act, algorithm=algo)
        got = selected(gen, guides, 6, synth, act, top_k=4, algorithm=algo)
        assert existing(algo) == before, algo
        ctx.release_scratch()
        _, rows2 = gen.summarize_classified(guides, 6, synth, act, algorithm=algo)
        assert rows2.tobytes() == rows.tobytes()
        assert selected(gen, guides, 6, synth, act, top_k=4, algorithm=algo).tobytes() == got.tobytes()
        assert existing(algo) == before, algo
    gen.close()


# ------------------------------------------------------------------------------------ 10. guide_summary -F / -C / -r votes / -V
def test_guide_summary_tool_classifier_columns_and_votes_listing(tmp_path, ctx, synth):
    rng = np.random.default_rng(1010)
    guides = random_guides(rng, 6)
    contigs = make_genome(1010, [15000, 6000], guides, 5, n_plant=150, n_runs=1, edge_plants=False)
    names = ["chr1 assembled", "chr2"]
    loci = []
    for i, g in enumerate(guides):  # the on-targets of the BED file
        c, pos, strand = i % 2, 300 + 700 * i, i % 3 == 0
        contigs[c] = contigs[c][:pos] + (revcomp(g) if strand else g) + contigs[c][pos + 23:]
        loci.append((c, pos, int(strand)))
    ids = ["g%d" % i for i in range(len(guides))]
    act = rng.choice(SYNTHETIC_ACTIVITIES, size=len(guides))
    with open(tmp_path / "g.fa", "w") as f:
        for n, s in zip(names, contigs):
            f.write(">%s\n%s\n" % (n, "\n".join(s[i:i + 60] for i in range(0, len(s), 60))))
    with open(tmp_path / "on.bed", "w") as f:
        for i, (c, pos, strand) in zip(ids, loci):
            f.write("%s\t%d\t%d\t%s\t0\t%s\n" % (names[c].split()[0], pos, pos + 23, i, "-" if strand else "+"))
    with open(tmp_path / "act.txt", "w") as f:
        for i, g, a in zip(ids, guides, act):
            f.write("%s\t%s\t%r\n" % (i, g, float(a)))
    run = lambda *a: subprocess.run([os.path.join(BIN, a[0])] + list(a[1:]), capture_output=True, text=True, timeout=600)
    assert run("bidir_index", "-G", str(tmp_path / "g.fa"), "-I", str(tmp_path / "idx")).returncode == 0
    base = ["guide_summary", "-G", str(tmp_path / "g.fa"), "-I", str(tmp_path / "idx"), "-M", "5", "-B", str(tmp_path / "on.bed")]
    cls = ["-F", synth.path, "-C", str(tmp_path / "act.txt")]
    r = run(*base, "-O", str(tmp_path / "plain.tsv"))
    assert r.returncode == 0, r.stderr
    plain = (tmp_path / "plain.tsv").read_text().splitlines()
    gen = ctx.load_genome(va.PackedGenome.from_sequences(contigs))
    _, rows = gen.summarize_classified(guides, 5, synth, act, exclude=loci)
    rec, votes = record_route(gen, synth, guides, act, 5, "auto")
    h = gen.search(guides, 5)
    mit = h.scores(mit=True)[0]
    h.close()
    gen.close()
    assert rows["votes_sum"].sum() > 0
    extra = ["rfExpectedActive", "rfActive", "rfTies"] + ["ra%d" % k for k in range(6)]
    for dev in ([], ["-D", "0,0"]):
        r = run(*base, *cls, "-O", str(tmp_path / "cls.tsv"), *dev)
        assert r.returncode == 0, r.stderr
        got = (tmp_path / "cls.tsv").read_text().splitlines()
        assert got[0] == plain[0] + "\t" + "\t".join(extra)
        for i, line in enumerate(got[1:]):
            want = ["%.6f" % (int(rows["votes_sum"][i]) / synth.n_trees), str(rows["active"][i]), str(rows["ties"][i])]
            want += [str(v) for v in rows["active_nm"][i][:6]]
            assert line == plain[1 + i] + "\t" + "\t".join(want), (dev, i)
    # the listing by votes: rank order, rfVotes last; the summary beside it is the classified one
    score = {(int(x["guide"]), int(x["contig"]), int(x["pos"]), int(x["info"])): float(np.rint(m * 2.0 ** 24)) for x, m in zip(rec, mit)}
    for opts, sel in ((["-K", "5"], (5, 0)), (["-K", "3", "-V", "4"], (3, 4))):
        ranked, v = cut_by_votes(rec, votes, sel[0], sel[1], exclude=loci, ranked=True)
        want = "#guideId\trank\tchrom\tstart\tend\tstrand\tmismatches\tmismatchPositions\tmitScore\tsequence\trfVotes\n"
        rank, last = 0, -1
        for x, votes_x in zip(ranked, v):
            g, c, p, info = int(x["guide"]), int(x["contig"]), int(x["pos"]), int(x["info"])
            rank, last = (rank + 1 if g == last else 1), g
            pos = [str(b) for b in range(23) if (info >> b) & 1 and b < 23]
            want += "%s\t%d\t%s\t%d\t%d\t%s\t%d\t%s\t%.6f\t%s\t%d\n" % (
                ids[g], rank, names[c].split()[0], p, p + 23, "-" if info >> 31 else "+", (info >> 23) & 31, ",".join(pos) or "-",
                score[(g, c, p, info)] * 2.0 ** -24, contigs[c][p:p + 23], votes_x)
        assert want.count("\n") > 6
        r = run(*base, *cls, "-O", str(tmp_path / "v.tsv"), "-T", str(tmp_path / "v.hits.tsv"), "-r", "votes", *opts)
        assert r.returncode == 0, r.stderr
        assert (tmp_path / "v.hits.tsv").read_text() == want, opts
        assert (tmp_path / "v.tsv").read_text() == (tmp_path / "cls.tsv").read_text()
    # -r votes without the classifier, -V without -r votes: refused before anything is loaded
    assert run(*base, "-T", str(tmp_path / "x.tsv"), "-r", "votes").returncode == 1
    assert run(*base, *cls, "-T", str(tmp_path / "x.tsv"), "-V", "3").returncode == 1
    assert run(*base, "-F", synth.path).returncode == 1
