"""vsc_search_select / vsc_multi_search_select on the device: per guide, the hits with rint(MIT * 2^24) >= a floor and of
those the top_k by (score descending, strand, position) - equal, byte for byte, to that cut made on the host over the hits
the oracle (or vsc_search + vsc_score_hits) reports, sorted as vsc_search sorts them."""
import os
import subprocess

import numpy as np
import pytest

import varscot_amd as va
from helpers import aggregate, by_result_order, cut, make_genome, oracle_hits, random_guides, random_seq, repeat_rich_genome, select
from test_summary import planted

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "varscot_amd", "bin")
FULL = int(np.rint(100.0 * 2 ** 24))
NONE = (0xFFFFFFFF, 0, 0)
SELECTIONS = [(1, 0), (3, 0), (10 ** 6, 0), (0, va.mit_fixed(1.0)), (3, va.mit_fixed(0.5))]


@pytest.fixture(scope="module")
def ctx():
    c = va.Context(0)
    yield c
    c.close()


def device_hits(gen, guides, m, algo, pam=None):
    """The same from vsc_search + vsc_score_hits (inputs too large for the character-level oracle)."""
    hits = gen.search(guides, m, extra_pam=pam, algorithm=algo)
    rec = hits.to_numpy()
    mit = hits.scores(mit=True)[0] if len(rec) else np.zeros(0)
    hits.close()
    return rec, np.rint(mit * 2.0 ** 24).astype(np.int64)


# ------------------------------------------------------------------------------------ 1. parity with the oracle
@pytest.mark.parametrize("m", [0, 3, 4, 6, 8])
@pytest.mark.parametrize("algo", ["scan", "seed"])
@pytest.mark.parametrize("pam", [None, "TT"])
def test_select_equals_oracle(ctx, oracle, m, algo, pam):
    guides, contigs = planted(500 + m, 8, [14000, 5000, 40], m, pam)
    hits, score, _, _ = oracle_hits(oracle, contigs, guides, m, pam)
    gen = ctx.load_genome(va.PackedGenome.from_sequences(contigs))
    for top_k, floor in SELECTIONS:
        want = cut(hits, score, top_k, floor)
        got = select(gen, guides, m, top_k, floor, extra_pam=pam, algorithm=algo)
        t = ctx.timing()
        print("m=%d %s pam=%s top_k=%d floor=%d: %d of %d hits" % (m, algo, pam, top_k, floor, len(got), len(hits)))
        assert t["algorithm"] == {"scan": 1, "seed": 2}[algo] and t["hits"] == len(hits)
        assert got.tobytes() == want.tobytes(), (top_k, floor)
    if pam is None:
        counts = np.bincount(hits["guide"], minlength=len(guides))
        assert counts.min() > 3  # top_k = 1 and 3 truncate every guide
        assert m < 4 or len(cut(hits, score, 0, va.mit_fixed(1.0))) < len(hits)  # the floor MIT >= 1 drops hits
    full = gen.search(guides, m, extra_pam=pam, algorithm=algo)
    assert select(gen, guides, m, 0, 0, extra_pam=pam, algorithm=algo).tobytes() == full.to_numpy().tobytes()
    full.close()
    gen.close()


# ------------------------------------------------------------------------------------ 2. many regions
def test_select_many_regions_sorts_survivors_only(ctx):
    """2 000 guides on 20.5 Mbp at m = 8 (every output region of the seed search in use): a real selection - 1.8 % of the
    records survive top_k = 20 - and the sort moves the survivors only."""
    rng = np.random.default_rng(77)
    guides = random_guides(rng, 2000)
    contigs = [random_seq(rng, 12_000_000), random_seq(rng, 8_500_000)]
    gen = ctx.load_genome(va.PackedGenome.from_sequences(contigs))
    rec, score = device_hits(gen, guides, 8, "seed")
    full_t = ctx.timing()
    assert len(rec) > 2_000_000 and full_t["hits"] == len(rec)
    for top_k, floor in ((20, 0), (100, 0), (0, va.mit_fixed(0.1))):
        want = cut(rec, score, top_k, floor)
        got = select(gen, guides, 8, top_k, floor, algorithm="seed")
        t = ctx.timing()
        print("top_k=%d floor=%d: %d of %d, sort_bytes %d (full search %d), sort_ms %.3f finalize_ms %.3f scan_ms %.3f" % (
            top_k, floor, len(got), len(rec), t["sort_bytes"], full_t["sort_bytes"], t["sort_ms"], t["finalize_ms"], t["scan_ms"]))
        assert t["algorithm"] == 2 and t["read_passes"] == 1 and t["hits"] == len(rec)
        assert got.tobytes() == want.tobytes(), (top_k, floor)
        if top_k == 20:
            assert len(got) == 40_000
            assert t["sort_bytes"] < 0.10 * full_t["sort_bytes"]
    gen.close()


# ------------------------------------------------------------------------------------ 3. two passes
def test_select_two_passes(ctx):
    rng = np.random.default_rng(78)
    guides = random_guides(rng, 16_500)
    contigs = make_genome(78, [300_000, 20_000], guides[::400], 3, n_plant=60)
    gen = ctx.load_genome(va.PackedGenome.from_sequences(contigs))
    for algo in ("scan", "seed"):
        rec, score = device_hits(gen, guides, 6, algo)
        got = select(gen, guides, 6, 2, algorithm=algo)
        assert ctx.timing()["read_passes"] == 2 and ctx.timing()["hits"] == len(rec)
        want = cut(rec, score, 2)
        assert 1000 < len(want) < len(rec)
        assert got.tobytes() == want.tobytes(), algo
    gen.close()


# ------------------------------------------------------------------------------------ 4. one score, 60 000 times
@pytest.mark.parametrize("algo", ["scan", "seed"])
def test_select_among_60000_equal_scores(ctx, algo):
    """Every hit has the full score: the cut is decided by strand and position alone, through every round of the select;
    the first search of the fresh genome overflows its buffer and runs again."""
    g = "ACGTTGCATGCAAGTCCTAGTGG"
    gen = ctx.load_genome(va.PackedGenome.from_sequences([(g + "T") * 60000]))
    got = select(gen, [g] * 40, 0, 100, algorithm=algo)
    assert ctx.timing()["passes"] == 2 and ctx.timing()["hits"] == 40 * 60000
    assert len(got) == 40 * 100
    assert np.array_equal(got["guide"], np.repeat(np.arange(40), 100))
    assert np.array_equal(got["pos"], np.tile(24 * np.arange(100), 40))
    assert np.all(got["contig"] == 0) and np.all(got["info"] == 0)  # '+', NM 0, no mismatch
    got = select(gen, [g] * 40, 0, 60001, algorithm=algo)
    assert len(got) == 40 * 60000
    assert np.array_equal(got["pos"], np.tile(24 * np.arange(60000), 40)) and np.all(got["info"] == 0)
    gen.close()


# ------------------------------------------------------------------------------------ 5. exclusion
@pytest.mark.parametrize("algo", ["scan", "seed"])
def test_select_excludes_the_on_target(ctx, oracle, algo):
    guides, contigs = planted(601, 6, [14000, 5000], 4)
    hits, score, _, _ = oracle_hits(oracle, contigs, guides, 4)
    gen = ctx.load_genome(va.PackedGenome.from_sequences(contigs))
    loci = lambda rec, g: [(int(r["contig"]), int(r["pos"]), int(r["info"] >> 31)) for r in rec[rec["guide"] == g]]
    base = select(gen, guides, 4, 2, algorithm=algo)
    assert base.tobytes() == cut(hits, score, 2).tobytes()
    assert loci(base, 0) == [(0, 1000, 0), (0, 9851, 0)]
    for ex0, want0 in (((0, 1000, 0), [(0, 9851, 0), (0, 3001, 1)]), ((0, 3001, 1), [(0, 1000, 0), (0, 9851, 0)])):
        ex = [ex0] + [NONE] * (len(guides) - 1)
        got = select(gen, guides, 4, 2, algorithm=algo, exclude=ex)
        assert got.tobytes() == cut(hits, score, 2, exclude=ex).tobytes()
        assert loci(got, 0) == want0
        assert got[got["guide"] > 0].tobytes() == base[base["guide"] > 0].tobytes()
        # without a cut, the excluded locus alone is missing
        got = select(gen, guides, 4, algorithm=algo, exclude=ex)
        assert len(got) == len(hits) - 1 and got.tobytes() == cut(hits, score, exclude=ex).tobytes()
    for miss in ((0, 1000, 1), (0, 1001, 0), (1, 4990, 0), (1, 1 << 30, 1)):
        got = select(gen, guides, 4, 2, algorithm=algo, exclude=[miss] * len(guides))
        assert got.tobytes() == base.tobytes()
    with pytest.raises(va.VarscotError) as e:
        gen.search_select(guides, 4, top_k=2, algorithm=algo, exclude=[(2, 0, 0)] * len(guides))
    assert e.value.code == -22
    gen.close()


# ------------------------------------------------------------------------------------ 6. summary in the same call
@pytest.mark.parametrize("algo", ["scan", "seed"])
def test_select_with_summary(ctx, oracle, algo):
    guides, contigs = planted(601, 6, [14000, 5000], 4)
    hits, score, mit, ub = oracle_hits(oracle, contigs, guides, 4)
    gen = ctx.load_genome(va.PackedGenome.from_sequences(contigs))
    for ex in (None, [(0, 1000, 0)] + [NONE] * (len(guides) - 1)):
        want_rows = gen.summarize(guides, 4, algorithm=algo, exclude=ex)
        assert want_rows.tobytes() == aggregate(hits, len(guides), mit, ub, ex).tobytes()
        for top_k, floor in ((2, 0), (0, va.mit_fixed(1.0)), (0, 0)):
            h, rows = gen.search_select(guides, 4, top_k=top_k, min_score=floor, algorithm=algo, exclude=ex, summary=True)
            assert ctx.timing()["read_passes"] == 1
            assert rows.tobytes() == want_rows.tobytes()
            assert h.to_numpy().tobytes() == select(gen, guides, 4, top_k, floor, algorithm=algo, exclude=ex).tobytes()
            assert h.to_numpy().tobytes() == cut(hits, score, top_k, floor, ex).tobytes()
            h.close()
    gen.close()


# ------------------------------------------------------------------------------------ 7. shards
@pytest.mark.parametrize("algo", ["scan", "seed"])
def test_select_composes_over_shards(ctx, oracle, algo):
    guides, contigs = planted(702, 8, [30000, 9000, 25], 6)
    packed = va.PackedGenome.from_sequences(contigs)
    hits, score, _, _ = oracle_hits(oracle, contigs, guides, 6)
    lookup = {(int(h["guide"]), int(h["contig"]), int(h["pos"]), int(h["info"])): int(s) for h, s in zip(hits, score)}
    ex = [(0, 1000, 0)] + [NONE] * (len(guides) - 1)
    whole = ctx.load_genome(packed)
    want = select(whole, guides, 6, 3, algorithm=algo, exclude=ex)
    whole.close()
    assert want.tobytes() == cut(hits, score, 3, exclude=ex).tobytes()
    for world in (2, 3):
        parts = []
        for rank in range(world):
            b, e = packed.shard_words(rank, world)
            if e <= b:
                continue
            g = ctx.load_genome(packed, rank, world)
            parts.append(select(g, guides, 6, 3, algorithm=algo, exclude=ex))
            g.close()
        union = np.concatenate(parts)
        assert len(union) > len(want)
        s = [lookup[(int(h["guide"]), int(h["contig"]), int(h["pos"]), int(h["info"]))] for h in union]
        assert cut(union, s, 3).tobytes() == want.tobytes(), world


@pytest.mark.parametrize("k", [1, 3, 8])
def test_multi_select_equals_one_context(ctx, k):
    guides, contigs = planted(803, 10, [40000, 12000, 30], 6)
    packed = va.PackedGenome.from_sequences(contigs)
    ex = [(0, 3001, 1)] + [NONE] * (len(guides) - 1)
    cases = ((3, 0), (0, va.mit_fixed(0.5)), (2, va.mit_fixed(0.2)), (0, 0))
    gen = ctx.load_genome(packed)
    want = {}
    for a in ("scan", "seed"):
        for c in cases:
            h, rows = gen.search_select(guides, 6, top_k=c[0], min_score=c[1], algorithm=a, exclude=ex, summary=True)
            want[a, c] = (h.to_numpy(), rows)
            h.close()
    gen.close()
    m = va.MultiContext([0] * k)
    try:
        g = m.load_genome(packed)
        for a in ("scan", "seed"):
            for c in cases:
                h, rows = g.search_select(guides, 6, top_k=c[0], min_score=c[1], algorithm=a, exclude=ex, summary=True)
                assert h.to_numpy().tobytes() == want[a, c][0].tobytes(), (a, c)
                assert rows.tobytes() == want[a, c][1].tobytes(), (a, c)
                assert rows["on_target"][0] == 1
                h.close()
                h = g.search_select(guides, 6, top_k=c[0], min_score=c[1], algorithm=a, exclude=ex)
                assert h.to_numpy().tobytes() == want[a, c][0].tobytes(), (a, c)
                h.close()
        with pytest.raises(va.VarscotError):
            g.search_select(guides, 6, top_k=3, exclude=[(3, 0, 0)] * len(guides))
        g.close()
    finally:
        m.close()


# ------------------------------------------------------------------------------------ 8. degenerate inputs, state
def test_select_degenerate_inputs(ctx, oracle):
    guides, contigs = planted(904, 5, [9000, 3000], 3)
    gen = ctx.load_genome(va.PackedGenome.from_sequences(contigs))
    assert len(select(gen, [], 3, 5)) == 0
    h, rows = gen.search_select([], 3, top_k=5, exclude=[], summary=True)
    assert len(h) == 0 and len(rows) == 0
    empty = ctx.load_genome(va.PackedGenome.from_sequences(["N" * 500 + random_seq(np.random.default_rng(1), 3000)]))
    for algo in ("scan", "seed"):
        assert len(select(empty, guides, 0, 5, algorithm=algo)) == 0
        assert len(select(empty, guides, 0, 0, va.mit_fixed(1.0), algorithm=algo)) == 0
    empty.close()
    hits, score, _, _ = oracle_hits(oracle, contigs, guides, 3)
    for algo in ("scan", "seed"):
        # top_k beyond any guide's hits: everything
        assert select(gen, guides, 3, 10 ** 6, algorithm=algo).tobytes() == by_result_order(hits).tobytes()
        # a floor nothing reaches
        assert len(select(gen, guides, 3, 0, FULL + 1, algorithm=algo)) == 0
    with_n = [guides[0][:5] + "N" + guides[0][6:]] + guides[1:]
    as_a = [with_n[0].replace("N", "A")] + guides[1:]
    got = select(gen, with_n, 3, 2)
    assert got.tobytes() == select(gen, as_a, 3, 2).tobytes()
    h_a, s_a, _, _ = oracle_hits(oracle, contigs, as_a, 3)
    assert got.tobytes() == cut(h_a, s_a, 2).tobytes()
    gen.close()


def test_select_leaves_no_state_and_feeds_the_consumers(ctx):
    guides, contigs = planted(905, 12, [30000, 8000], 6)
    packed = va.PackedGenome.from_sequences(contigs)
    fresh = va.Context(0)
    try:
        g0 = fresh.load_genome(packed)
        want = {a: g0.search(guides, 6, algorithm=a) for a in ("scan", "seed")}
        want = {a: (h.to_numpy(), h.close())[0] for a, h in want.items()}
        g0.close()
    finally:
        fresh.close()
    gen = ctx.load_genome(packed)
    for a in ("scan", "seed"):
        s1 = select(gen, guides, 6, 3, algorithm=a)
        s2 = select(gen, guides, 6, 3, algorithm=a)
        assert len(guides) < len(s1) <= 3 * len(guides) and s1.tobytes() == s2.tobytes()
        h = gen.search(guides, 6, algorithm=a)
        assert h.to_numpy().tobytes() == want[a].tobytes()
        mit_all = h.scores(mit=True)[0]
        all_rec = h.to_numpy()
        h.close()
        # the selected records are ordinary records: their scores are those of the same records in the full result
        sel = gen.search_select(guides, 6, top_k=3, algorithm=a)
        mit = sel.scores(mit=True)[0]
        key = lambda r: (int(r["guide"]), int(r["info"] >> 31), int(r["contig"]), int(r["pos"]))
        full = {key(r): x for r, x in zip(all_rec, mit_all)}
        assert [full[key(r)] for r in sel.to_numpy()] == list(mit)
        order = va.sam_order(sel.to_numpy())
        assert sorted(np.asarray(order[0] if isinstance(order, tuple) else order).tolist()) == list(range(len(sel)))
        sel.close()
    gen.close()


# ------------------------------------------------------------------------------------ randomised sweep
def test_select_randomised_sweep(ctx, oracle):
    """240 seeded cases: uniform genomes with planted sites and repeat-rich ones, random budget, algorithm, top_k in
    1..50, floor on or off - each against the cut of the oracle's hits."""
    rng = np.random.default_rng(20240)
    cases = truncated = floored = 0
    for gi in range(40):
        guides = random_guides(rng, int(rng.integers(2, 9)))
        if gi % 2:
            contigs = repeat_rich_genome(1000 + gi, 40_000, guides)
        else:
            contigs = make_genome(1000 + gi, [int(rng.integers(3000, 20000)), int(rng.integers(300, 6000)), 30], guides, 6, n_plant=80)
        gen = ctx.load_genome(va.PackedGenome.from_sequences(contigs))
        found = {}
        for _ in range(6):
            m = int(rng.integers(0, 9))
            algo = ("scan", "seed")[int(rng.integers(0, 2))]
            top_k = int(rng.integers(1, 51))
            floor = int(rng.integers(0, 2)) * int(2 ** rng.uniform(0, 30.6))
            if m not in found:
                found[m] = oracle_hits(oracle, contigs, guides, m)[:2]
            hits, score = found[m]
            want = cut(hits, score, top_k, floor)
            got = select(gen, guides, m, top_k, floor, algorithm=algo)
            assert got.tobytes() == want.tobytes(), (gi, m, algo, top_k, floor)
            cases += 1
            truncated += len(want) < int((score >= floor).sum())
            floored += bool(floor) and int((score >= floor).sum()) < len(hits)
        gen.close()
    print("sweep: %d cases, %d cut by top_k, %d cut by the floor" % (cases, truncated, floored))
    assert cases >= 200 and truncated >= 20 and floored >= 20


# ------------------------------------------------------------------------------------ 9. guide_summary -K / -S / -T
def _hits_tsv(ids, contigs, names, ranked, score_of):
    comp = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}
    text = "#guideId\trank\tchrom\tstart\tend\tstrand\tmismatches\tmismatchPositions\tmitScore\tsequence\n"
    rank, last = 0, -1
    for r in ranked:
        g, c, p, info = int(r["guide"]), int(r["contig"]), int(r["pos"]), int(r["info"])
        rank = rank + 1 if g == last else 1
        last = g
        mask = info & 0x7FFFFF
        pos = [str(b) for b in range(23) if (mask >> b) & 1]
        text += "%s\t%d\t%s\t%d\t%d\t%s\t%d\t%s\t%.6f\t%s\n" % (
            ids[g], rank, names[c].split()[0], p, p + 23, "-" if info >> 31 else "+", (info >> 23) & 31, ",".join(pos) or "-",
            score_of(r) * 2.0 ** -24, contigs[c][p:p + 23])
    return text


def test_guide_summary_tool_lists_selected_hits(tmp_path, oracle):
    guides, contigs = planted(1006, 6, [15000, 6000, 40], 5)
    names = ["chr1 assembled", "chr2", "tiny"]
    with open(tmp_path / "g.fa", "w") as f:
        for n, s in zip(names, contigs):
            f.write(">%s\n%s\n" % (n, "\n".join(s[i:i + 60] for i in range(0, len(s), 60))))
    ids = ["g%d" % i for i in range(len(guides))]
    reads = list(guides)
    reads[3] = reads[3][:4] + "n" + reads[3][5:]
    with open(tmp_path / "r.fa", "w") as f:
        for i, s in zip(ids, reads):
            f.write(">%s\n%s\n" % (i, s))
    run = lambda *a: subprocess.run([os.path.join(BIN, a[0])] + list(a[1:]), capture_output=True, text=True, timeout=600)
    assert run("bidir_index", "-G", str(tmp_path / "g.fa"), "-I", str(tmp_path / "idx")).returncode == 0
    base = ["guide_summary", "-G", str(tmp_path / "g.fa"), "-I", str(tmp_path / "idx"), "-M", "5", "-R", str(tmp_path / "r.fa")]
    searched = [s.upper().replace("N", "A") for s in reads]
    hits, score, _, _ = oracle_hits(oracle, contigs, searched, 5)
    lookup = {(int(h["guide"]), int(h["contig"]), int(h["pos"]), int(h["info"])): int(s) for h, s in zip(hits, score)}
    score_of = lambda r: lookup[(int(r["guide"]), int(r["contig"]), int(r["pos"]), int(r["info"]))]
    r = run(*base, "-O", str(tmp_path / "plain.tsv"))
    assert r.returncode == 0, r.stderr
    for tag, opts, sel in (("k", ["-K", "3"], (3, 0)), ("s", ["-S", "0.5"], (0, va.mit_fixed(0.5))),
                           ("ks", ["-K", "2", "-S", "0.25"], (2, va.mit_fixed(0.25)))):
        want = _hits_tsv(ids, contigs, names, cut(hits, score, sel[0], sel[1], ranked=True), score_of)
        assert want.count("\n") > 1
        for dev in ([], ["-D", "0,0"]):
            out, tsv = tmp_path / (tag + str(len(dev)) + ".tsv"), tmp_path / (tag + str(len(dev)) + ".hits.tsv")
            r = run(*base, "-O", str(out), *opts, "-T", str(tsv), *dev)
            assert r.returncode == 0, r.stderr
            assert tsv.read_text() == want, (tag, dev)
            assert out.read_bytes() == (tmp_path / "plain.tsv").read_bytes()
