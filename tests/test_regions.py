"""vsc_search_summary_regions / vsc_search_select_regions (and their vsc_multi_* forms) on the device: the rows over the hits
in an annotation and the selection on one side of it equal, byte for byte, what numpy makes of the oracle's hits (or of
vsc_search's, where the input is too large for the oracle) with the membership of every window decided by brute force."""
import os
import subprocess

import numpy as np
import pytest

import varscot_amd as va
from helpers import aggregate, cut, inside_numpy, make_genome, oracle_hits, random_guides
from regions_cases import LENS, P_MINUS, P_PLUS, annotation, brute_force, member
from test_summary import planted

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "varscot_amd", "bin")
NONE = (0xFFFFFFFF, 0, 0)
RULES = ["overlap", "inside"]
ALGOS = ["scan", "seed"]
FLOOR = va.mit_fixed(0.02)  # low enough that top_k = 5 still cuts what passes it (most hits score far below 1)


@pytest.fixture(scope="module")
def ctx():
    c = va.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def truth():
    """Membership of every window of the three-contig layout under both rules (computed once, never changed)."""
    return brute_force(annotation(with_sites=True))


_cases = {}


@pytest.fixture(scope="module")
def case(oracle):
    """case(m) = the planted genome of tests/test_summary.py for budget m with the oracle's hits and scores - once per m."""
    def get(m):
        if m not in _cases:
            guides, contigs = planted(500 + m, 8, LENS, m)
            hits, score, mit, ub = oracle_hits(oracle, contigs, guides, m)
            _cases[m] = dict(guides=guides, contigs=contigs, packed=va.PackedGenome.from_sequences(contigs), hits=hits, score=score,
                             mit=mit, ub=ub, all=aggregate(hits, len(guides), mit, ub))
        return _cases[m]
    return get


def rows_inside(c, inside, exclude=None):
    """The rows over the hits of case c that are in the regions (on_target as over all hits)."""
    rows = aggregate(c["hits"][inside], len(c["guides"]), c["mit"][inside], c["ub"][inside], exclude)
    if exclude is not None:
        rows["on_target"] = aggregate(c["hits"], len(c["guides"]), c["mit"], c["ub"], exclude)["on_target"]
    return rows


def random_cover(rng, packed, n, fraction):
    """n random intervals whose lengths add up to `fraction` of the genome (they overlap: the union is somewhat less)."""
    lens = packed.contigs["length"].astype(np.int64)
    mean = fraction * lens.sum() / n
    c = rng.choice(len(lens), size=n, p=lens / lens.sum())
    ln = rng.integers(max(1, int(mean / 10)), int(2 * mean), size=n)
    start = (rng.random(n) * lens[c]).astype(np.int64)
    return np.stack([c, start, start + ln], axis=1)


# ------------------------------------------------------------------------------------ 1. parity with the oracle
@pytest.mark.parametrize("m", [0, 4, 8])
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("rule", RULES)
def test_summary_regions_equals_oracle(ctx, case, truth, m, algo, rule):
    c = case(m)
    inside = member(truth[rule], c["hits"])
    strands_in = set((c["hits"]["info"][inside] >> 31).tolist())
    print("m=%d %s %s: %d of %d hits in the regions, strands %s" % (m, algo, rule, inside.sum(), len(inside), sorted(strands_in)))
    assert inside.any() and not inside.all() and strands_in == {0, 1}
    want_in = rows_inside(c, inside)
    reg = va.Regions(c["packed"], annotation(with_sites=True), rule=rule)
    gen = ctx.load_genome(c["packed"])
    got_all, got_in = gen.summarize(c["guides"], m, algorithm=algo, regions=reg)
    t = ctx.timing()
    assert t["algorithm"] == {"scan": 1, "seed": 2}[algo] and t["hits"] == len(c["hits"]) and t["sort_ms"] == 0
    assert got_all.tobytes() == c["all"].tobytes()
    assert got_in.tobytes() == want_in.tobytes(), (got_in, want_in)
    assert got_all.tobytes() == gen.summarize(c["guides"], m, algorithm=algo).tobytes()  # the bytes vsc_search_summary writes
    gen.close()
    reg.close()


def test_the_planted_sites_sit_on_the_edges(case, truth):
    """What the intervals around the two perfect sites are there for: '+' at 1000 is touched by one base, '-' at 3001 fits one
    interval exactly; one position further, each answer changes."""
    assert truth["overlap"][0][P_PLUS] and not truth["inside"][0][P_PLUS]
    without = [iv for iv in annotation(with_sites=True) if iv != (0, P_PLUS + 22, P_PLUS + 30)]
    assert not brute_force(without)["overlap"][0][P_PLUS]
    assert truth["inside"][0][P_MINUS] and not truth["inside"][0][P_MINUS - 1] and not truth["inside"][0][P_MINUS + 1]
    h = case(0)["hits"]
    for pos, strand in ((P_PLUS, 0), (P_MINUS, 1)):
        assert ((h["guide"] == 0) & (h["contig"] == 0) & (h["pos"] == pos) & ((h["info"] >> 31) == strand)).any()


# ------------------------------------------------------------------------------------ 2. more than one output region
def test_summary_regions_many_output_regions(ctx):
    """200 guides (four output regions of the seed search) at m = 6 on 130 Mbp of random sequence - the size at which more
    than 10^4 hits fall on each side of an annotation that covers about a third (2 Mbp hold 600 hits)."""
    rng = np.random.default_rng(91)
    guides = random_guides(rng, 200)
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)
    packed = va.PackedGenome.from_sequences([bases[rng.integers(0, 4, size=n, dtype=np.uint8)].tobytes() for n in (80_000_000, 50_000_000)])
    iv = random_cover(rng, packed, 1200, 0.40)
    gen = ctx.load_genome(packed)
    hits = gen.search(guides, 6, algorithm="seed")
    rec = hits.to_numpy()
    mit, flags, _ = hits.scores(mit=True)  # (the flags carry mit_ub, as in test 3)
    hits.close()
    for rule in RULES:
        inside = inside_numpy(packed, iv, rule, rec)
        print("%s: %d hits inside, %d outside" % (rule, inside.sum(), (~inside).sum()))
        assert inside.sum() >= 10_000 and (~inside).sum() >= 10_000
        reg = va.Regions(packed, iv, rule=rule)
        got_all, got_in = gen.summarize(guides, 6, algorithm="seed", regions=reg)
        assert ctx.timing()["algorithm"] == 2 and ctx.timing()["hits"] == len(rec)
        assert got_all.tobytes() == aggregate(rec, len(guides), mit, flags).tobytes(), rule
        assert got_in.tobytes() == aggregate(rec[inside], len(guides), mit[inside], flags[inside]).tobytes(), rule
        assert not got_all["on_target"].any() and not got_in["on_target"].any()
        assert np.count_nonzero(got_in["nm"].sum(axis=1)) > 190  # every output region has reads with hits inside
        reg.close()
    gen.close()


# ------------------------------------------------------------------------------------ 3. two read passes
def test_summary_regions_two_passes(ctx):
    rng = np.random.default_rng(78)
    guides = random_guides(rng, 16_500)
    contigs = make_genome(78, [300_000, 20_000], guides[::400], 3, n_plant=60)
    packed = va.PackedGenome.from_sequences(contigs)
    iv = random_cover(np.random.default_rng(79), packed, 150, 0.40)
    reg = va.Regions(packed, iv, rule="overlap")
    gen = ctx.load_genome(packed)
    for algo in ALGOS:
        hits = gen.search(guides, 6, algorithm=algo)
        rec = hits.to_numpy()
        mit, flags, _ = hits.scores(mit=True)
        hits.close()
        inside = inside_numpy(packed, iv, "overlap", rec)
        assert inside.sum() > 300 and (~inside).sum() > 300
        assert inside[rec["guide"] >= 16_384].any()  # the second pass has hits in the regions
        got_all, got_in = gen.summarize(guides, 6, algorithm=algo, regions=reg)
        assert ctx.timing()["read_passes"] == 2
        assert got_all.tobytes() == aggregate(rec, len(guides), mit, flags).tobytes(), algo
        assert got_in.tobytes() == aggregate(rec[inside], len(guides), mit[inside], flags[inside]).tobytes(), algo
    gen.close()
    reg.close()


# ------------------------------------------------------------------------------------ 4. exclusion
@pytest.mark.parametrize("algo", ALGOS)
def test_summary_regions_excludes_the_on_target(ctx, case, truth, algo):
    c = case(4)
    gen = ctx.load_genome(c["packed"])
    n = len(c["guides"])
    for rule, pos, strand in (("overlap", P_PLUS, 0), ("inside", P_MINUS, 1), ("inside", P_PLUS, 0)):
        ex = [(0, pos, strand)] + [NONE] * (n - 1)
        inside = member(truth[rule], c["hits"])
        base_in = rows_inside(c, inside)
        want_all = aggregate(c["hits"], n, c["mit"], c["ub"], ex)
        want_in = rows_inside(c, inside, ex)
        reg = va.Regions(c["packed"], annotation(with_sites=True), rule=rule)
        got_all, got_in = gen.summarize(c["guides"], 4, algorithm=algo, exclude=ex, regions=reg)
        reg.close()
        assert got_all.tobytes() == want_all.tobytes() and got_in.tobytes() == want_in.tobytes(), (rule, pos)
        assert got_all["on_target"][0] == 1 and got_in["on_target"][0] == 1
        assert got_all["nm"][0, 0] == c["all"]["nm"][0, 0] - 1
        # the locus is in the regions (first two) - it is missing from the inside row too - or not (the last): that row stays
        assert got_in["nm"][0, 0] == base_in["nm"][0, 0] - int(truth[rule][0][pos])
        assert bool(truth[rule][0][pos]) == ((rule, pos) in (("overlap", P_PLUS), ("inside", P_MINUS)))
    gen.close()


# ------------------------------------------------------------------------------------ 5. selection
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("scope", ["keep", "drop"])
@pytest.mark.parametrize("rule", RULES)
def test_select_regions_equals_oracle(ctx, case, truth, algo, scope, rule):
    c = case(8)
    inside = member(truth[rule], c["hits"])
    side = inside if scope == "keep" else ~inside
    want_in = rows_inside(c, inside)
    reg = va.Regions(c["packed"], annotation(with_sites=True), rule=rule)
    gen = ctx.load_genome(c["packed"])
    for top_k, floor in ((0, 0), (3, 0), (0, FLOOR), (5, FLOOR)):
        want = cut(c["hits"][side], c["score"][side], top_k, floor)
        h, rows, rows_in = gen.search_select(c["guides"], 8, top_k=top_k, min_score=floor, algorithm=algo, summary=True, regions=reg,
                                             region_scope=scope)
        got = h.to_numpy()
        h.close()
        print("%s %s %s top_k=%d floor=%d: %d of %d (%d on that side)" % (algo, scope, rule, top_k, floor, len(got), len(side), side.sum()))
        assert ctx.timing()["hits"] == len(c["hits"])
        assert got.tobytes() == want.tobytes(), (top_k, floor)
        assert rows.tobytes() == c["all"].tobytes() and rows_in.tobytes() == want_in.tobytes()
        if (top_k, floor) == (0, 0):
            assert 0 < len(got) == side.sum() < len(c["hits"])
        else:
            assert 0 < len(got) < side.sum()
        # without the summaries: the same records
        h = gen.search_select(c["guides"], 8, top_k=top_k, min_score=floor, algorithm=algo, regions=reg, region_scope=scope)
        assert h.to_numpy().tobytes() == want.tobytes()
        h.close()
    gen.close()
    reg.close()


@pytest.mark.parametrize("algo", ALGOS)
def test_inside_drop_is_the_shadow_filter(ctx, case, algo):
    """top_k = 0, min_score = 0, rule inside, scope drop = the oracle's hits minus those that WindowIndex's rule shadows: with
    the windows in global coordinates sorted by start (S) and E the running maximum of their ends, a hit at global position p
    is shadowed iff n = #{S <= p} > 0 and E[n - 1] >= p + 23 - restated here, independently of the interval test above."""
    c = case(8)
    iv = annotation(with_sites=True)
    off = c["packed"].contigs["offset"].astype(np.int64)
    g = sorted((int(off[k]) + a, int(off[k]) + min(b, LENS[k])) for k, a, b in iv if a < min(b, LENS[k]))
    S = np.array([a for a, _ in g], dtype=np.int64)
    E = np.maximum.accumulate(np.array([b for _, b in g], dtype=np.int64))
    p = off[c["hits"]["contig"]] + c["hits"]["pos"].astype(np.int64)
    n = np.searchsorted(S, p, side="right")
    shadowed = (n > 0) & (E[np.maximum(n, 1) - 1] >= p + 23)
    assert shadowed.any() and not shadowed.all()
    reg = va.Regions(c["packed"], iv, rule="inside")
    gen = ctx.load_genome(c["packed"])
    h = gen.search_select(c["guides"], 8, algorithm=algo, regions=reg, region_scope="drop")
    assert h.to_numpy().tobytes() == c["hits"][~shadowed].tobytes()  # (the oracle's hits are in vsc_search's order)
    h.close()
    # filter == NULL behaves as vsc_search_select; a bad filter is refused
    sel, flt, out = va._lib.Select(), va._lib.RegionFilter(reg._h, 0, 0), va._lib.C.c_void_p()
    codes, p8 = va.pack_guides(c["guides"]), va.Genome._params(8, None, algo)
    call = lambda f: va.lib().vsc_search_select_regions(ctx._h, gen._h, va._lib.ptr(codes), len(codes), va._lib.C.byref(p8), va._lib.C.byref(sel),
                                                        f, None, None, None, va._lib.C.byref(out))
    assert call(None) == 0
    assert va.lib().vsc_hits_count(out) == len(c["hits"])
    va.lib().vsc_hits_free(out)
    for bad in (va._lib.RegionFilter(reg._h, 2, 0), va._lib.RegionFilter(reg._h, 0, 1), va._lib.RegionFilter(None, 0, 0)):
        assert call(va._lib.C.byref(bad)) == -22 and not out.value
    assert call(va._lib.C.byref(flt)) == 0
    va.lib().vsc_hits_free(out)
    # regions built for another contig table
    other = va.Regions(va.PackedGenome.from_sequences(["A" * 100, "C" * 50, "G" * 40]), [(0, 1, 50)])
    with pytest.raises(va.VarscotError) as e:
        gen.summarize(c["guides"], 8, algorithm=algo, regions=other)
    assert e.value.code == -22
    other.close()
    gen.close()
    reg.close()


# ------------------------------------------------------------------------------------ 6. shards and devices
@pytest.mark.parametrize("algo", ALGOS)
def test_regions_over_shards_add_up(ctx, case, truth, algo):
    c = case(8)
    packed, guides, n = c["packed"], c["guides"], len(c["guides"])
    inside = member(truth["overlap"], c["hits"])
    want_in = rows_inside(c, inside)
    want_sel = cut(c["hits"][inside], c["score"][inside], 3, 0)
    reg = va.Regions(packed, annotation(with_sites=True), rule="overlap")
    for world in (2, 3):
        tot_all, tot_in, parts = np.zeros(n, dtype=va.SUMMARY_DTYPE), np.zeros(n, dtype=va.SUMMARY_DTYPE), []
        for rank in range(world):
            g = ctx.load_genome(packed, rank, world)
            a, b = g.summarize(guides, 8, algorithm=algo, regions=reg)
            for tot, part in ((tot_all, a), (tot_in, b)):
                tot["mit_sum"] += part["mit_sum"]
                tot["nm"] += part["nm"]
                tot["mit_ub"] += part["mit_ub"]
                tot["on_target"] |= part["on_target"]
            h = g.search_select(guides, 8, top_k=3, algorithm=algo, regions=reg)
            parts.append(h.to_numpy())
            h.close()
            g.close()
        assert tot_all.tobytes() == c["all"].tobytes() and tot_in.tobytes() == want_in.tobytes(), world
        # the selection of the union of the shards' selections is the selection on the whole genome
        union = np.concatenate(parts)
        key = {(int(r["guide"]), int(r["contig"]), int(r["pos"]), int(r["info"])): int(s) for r, s in zip(c["hits"], c["score"])}
        score = np.array([key[(int(r["guide"]), int(r["contig"]), int(r["pos"]), int(r["info"]))] for r in union], dtype=np.int64)
        assert member(truth["overlap"], union).all()
        assert cut(union, score, 3, 0).tobytes() == want_sel.tobytes(), world
    reg.close()


@pytest.mark.parametrize("k", [1, 3])
def test_multi_regions_equal_one_context(ctx, case, truth, k):
    c = case(8)
    guides = c["guides"]
    ex = [(0, P_MINUS, 1)] + [NONE] * (len(guides) - 1)
    reg = va.Regions(c["packed"], annotation(with_sites=True), rule="inside")
    gen = ctx.load_genome(c["packed"])
    want = {}
    for a in ALGOS:
        rows = gen.summarize(guides, 8, algorithm=a, exclude=ex, regions=reg)
        sel = {}
        for scope, top_k in (("keep", 3), ("drop", 0)):
            h, r_all, r_in = gen.search_select(guides, 8, top_k=top_k, algorithm=a, exclude=ex, summary=True, regions=reg, region_scope=scope)
            sel[scope] = (h.to_numpy(), r_all, r_in)
            h.close()
        want[a] = (rows, sel)
    gen.close()
    inside = member(truth["inside"], c["hits"])
    assert want["seed"][0][1].tobytes() == rows_inside(c, inside, ex).tobytes()  # one context is right (test 4), so is the set
    m = va.MultiContext([0] * k)
    try:
        g = m.load_genome(c["packed"])
        for a in ALGOS:
            rows, sel = want[a]
            got_all, got_in = g.summarize(guides, 8, algorithm=a, exclude=ex, regions=reg)
            assert got_all.tobytes() == rows[0].tobytes() and got_in.tobytes() == rows[1].tobytes(), a
            assert got_in["on_target"][0] == 1
            for scope, top_k in (("keep", 3), ("drop", 0)):
                h, r_all, r_in = g.search_select(guides, 8, top_k=top_k, algorithm=a, exclude=ex, summary=True, regions=reg, region_scope=scope)
                assert h.to_numpy().tobytes() == sel[scope][0].tobytes(), (a, scope)
                assert r_all.tobytes() == sel[scope][1].tobytes() and r_in.tobytes() == sel[scope][2].tobytes()
                h.close()
        g.close()
    finally:
        m.close()
        reg.close()


# ------------------------------------------------------------------------------------ 7. the context's slot
def test_context_keeps_the_regions_it_used_last(case, truth):
    c = case(4)
    guides, n = c["guides"], len(c["guides"])
    iv = annotation(with_sites=True)
    moved = [(k, a + 40, b + 40) if k < 2 else (k, a, b) for k, a, b in iv]  # as many intervals, other places
    regs = [va.Regions(c["packed"], iv, rule="inside"), va.Regions(c["packed"], moved, rule="inside")]
    assert regs[0].info()["intervals"] == regs[1].info()["intervals"]
    tables = [truth["inside"], brute_force(moved)["inside"]]
    wants = [rows_inside(c, member(t, c["hits"])) for t in tables]
    assert wants[0].tobytes() != wants[1].tobytes()
    own = va.Context(0)
    try:
        gen = own.load_genome(c["packed"])
        plain = {a: gen.summarize(guides, 4, algorithm=a) for a in ALGOS}
        for a in ALGOS:
            for i in (0, 1, 0, 0, 1):
                got_all, got_in = gen.summarize(guides, 4, algorithm=a, regions=regs[i])
                assert got_all.tobytes() == c["all"].tobytes() and got_in.tobytes() == wants[i].tobytes(), (a, i)
            own.release_scratch()
            got_all, got_in = gen.summarize(guides, 4, algorithm=a, regions=regs[1])
            assert got_all.tobytes() == c["all"].tobytes() and got_in.tobytes() == wants[1].tobytes(), a
            h = gen.search_select(guides, 4, algorithm=a, regions=regs[0], region_scope="keep")
            assert h.to_numpy().tobytes() == c["hits"][member(tables[0], c["hits"])].tobytes()
            h.close()
            # a set that is freed and another built in its place (maybe at its address) is another set
            tmp = va.Regions(c["packed"], moved, rule="overlap")
            tmp.close()
            tmp = va.Regions(c["packed"], iv, rule="overlap")
            got_in = gen.summarize(guides, 4, algorithm=a, regions=tmp)[1]
            assert got_in.tobytes() == rows_inside(c, member(truth["overlap"], c["hits"])).tobytes()
            tmp.close()
            # the feature leaves no state behind
            assert gen.summarize(guides, 4, algorithm=a).tobytes() == plain[a].tobytes() == c["all"].tobytes()
            h = gen.search(guides, 4, algorithm=a)
            assert h.to_numpy().tobytes() == c["hits"].tobytes()
            h.close()
        gen.close()
    finally:
        own.close()
        for r in regs:
            r.close()


# ------------------------------------------------------------------------------------ 8. guide_summary -A / -a / -X
def test_guide_summary_tool_regions(tmp_path, case, truth):
    c = case(4)
    guides, contigs, m = c["guides"], c["contigs"], 4
    names = ["chr1 assembled", "chr2", "tiny"]
    with open(tmp_path / "g.fa", "w") as f:
        for n, s in zip(names, contigs):
            f.write(">%s\n%s\n" % (n, "\n".join(s[i:i + 60] for i in range(0, len(s), 60))))
    ids = ["g%d" % i for i in range(len(guides))]
    with open(tmp_path / "r.fa", "w") as f:
        for i, s in zip(ids, guides):
            f.write(">%s\n%s\n" % (i, s))
    chrom = ["chr1", "chr2", "tiny"]
    with open(tmp_path / "a.bed", "w") as f:
        f.write("# an annotation\ntrack name=test\n")
        for k, a, b in annotation(with_sites=True):
            f.write("%s\t%d\t%d\tx\t0\t+\n" % (chrom[k], a, b))
    run = lambda *a: subprocess.run([os.path.join(BIN, a[0])] + list(a[1:]), capture_output=True, text=True, timeout=600)
    assert run("bidir_index", "-G", str(tmp_path / "g.fa"), "-I", str(tmp_path / "idx")).returncode == 0
    base = ["guide_summary", "-G", str(tmp_path / "g.fa"), "-I", str(tmp_path / "idx"), "-M", str(m), "-R", str(tmp_path / "r.fa")]
    plain = run(*base)
    assert plain.returncode == 0, plain.stderr

    def columns(rows):
        out = []
        for r in rows:
            spec = int(np.floor(va.mit_specificity(int(r["mit_sum"])) + 0.5))
            out.append("%d\t%d\t%s\t%.6f" % (spec, int(r["nm"].sum()), "\t".join(str(int(x)) for x in r["nm"][:m + 1]),
                                             int(r["mit_sum"]) * 2.0 ** -24))
        return out

    head = "\tregionMitSpecScore\tregionCount\t" + "\t".join("rmm%d" % k for k in range(m + 1)) + "\tregionMitHitSum"
    for rule in RULES:
        inside = member(truth[rule], c["hits"])
        r = run(*base, "-A", str(tmp_path / "a.bed"), "-a", rule, "-D", "0" if rule == "overlap" else "0,0")
        assert r.returncode == 0, r.stderr
        got, old = r.stdout.splitlines(), plain.stdout.splitlines()
        want = [old[0] + head] + [o + "\t" + x for o, x in zip(old[1:], columns(rows_inside(c, inside)))]
        assert got == want, rule
        if rule == "overlap":
            assert run(*base, "-A", str(tmp_path / "a.bed")).stdout == r.stdout  # the default rule
        # -X: the listing holds one side of the regions only, the summary columns stay
        for scope in ("keep", "drop"):
            r2 = run(*base, "-A", str(tmp_path / "a.bed"), "-a", rule, "-X", scope, "-K", "4", "-T", str(tmp_path / "t.tsv"))
            assert r2.returncode == 0, r2.stderr
            assert r2.stdout == r.stdout
            side = inside if scope == "keep" else ~inside
            sel = cut(c["hits"][side], c["score"][side], 4, 0, ranked=True)
            listed = [l.split("\t") for l in (tmp_path / "t.tsv").read_text().splitlines()[1:]]
            assert [(l[0], l[2], int(l[3]), l[5]) for l in listed] == [
                (ids[h["guide"]], chrom[h["contig"]], int(h["pos"]), "-" if h["info"] >> 31 else "+") for h in sel]
            assert len(listed) > 0 and all(bool(truth[rule][chrom.index(l[2])][int(l[3])]) == (scope == "keep") for l in listed)
        if rule == "inside":
            continue
        # -T without -X: the unfiltered listing beside the region columns
        r3 = run(*base, "-A", str(tmp_path / "a.bed"), "-a", rule, "-K", "4", "-T", str(tmp_path / "u.tsv"))
        assert r3.returncode == 0 and r3.stdout == r.stdout
        r4 = run(*base, "-K", "4", "-T", str(tmp_path / "v.tsv"))
        assert r4.returncode == 0 and (tmp_path / "u.tsv").read_bytes() == (tmp_path / "v.tsv").read_bytes()
    # an unknown chromosome, -X without its companions, a bad rule
    (tmp_path / "bad.bed").write_text("chr1\t10\t50\nchr9\t10\t50\n")
    r = run(*base, "-A", str(tmp_path / "bad.bed"))
    assert r.returncode == 1 and "chr9" in r.stderr
    assert run(*base, "-A", str(tmp_path / "a.bed"), "-X", "drop").returncode == 1
    assert run(*base, "-X", "drop", "-T", str(tmp_path / "t.tsv")).returncode == 1
    assert run(*base, "-A", str(tmp_path / "a.bed"), "-a", "near").returncode == 1
