"""vsc_search_pattern on the device: records and rows byte for byte what the definition gives when it is applied site by site
(tests/pattern_cases.py) - over the lengths, the PAM at either end and at both, the budgets; identical to the plain scan
where the two definitions coincide; a tandem array, the rounds, the two outputs, the cap, shards, repetition, the timing
fields, what is refused and pattern_search end to end."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import varscot_amd as va
import pattern_cases as pc
from helpers import make_genome, random_guides

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "varscot_amd", "bin")


@pytest.fixture(scope="module")
def ctx():
    c = va.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def edge():
    e = dict(pc.edge_scenario(23, "3"))
    e["m"] = 4
    e["want"] = pc.hits_at(e, 4)
    e["packed"] = va.PackedGenome.from_sequences(e["contigs"])
    e["rec"], e["rows"] = pc.arrays(e["want"], len(e["guides"]))
    return e


@pytest.fixture(scope="module")
def edge_gen(ctx, edge):
    g = ctx.load_genome(edge["packed"])
    yield g
    g.close()


def same(got, want_hits, n_guides):
    rec, rows = pc.arrays(want_hits, n_guides)
    assert got[0].dtype == va.PATTERN_HIT_DTYPE and got[1].dtype == np.uint32 and got[1].shape == (n_guides, 9)
    assert len(got[0]) == len(rec)
    assert got[0].tobytes() == rec.tobytes()
    assert got[1].tobytes() == rows.tobytes()


# ---- 1. the edge layout over lengths, PAM places and budgets --------------------------------------------------------------
@pytest.mark.parametrize("place", pc.PLACES)
@pytest.mark.parametrize("L", [16, 20, 23, 27, 32])
def test_edge_layout_equals_the_definition(ctx, L, place):
    e = pc.edge_scenario(L, place)
    gen = ctx.load_genome(va.PackedGenome.from_sequences(e["contigs"]))
    try:
        for m in (0, 3, 8):
            want = pc.hits_at(e, m)
            assert want and max(h[4] for h in want) == m and {h[1] for h in want} == {0, 1}
            same(gen.search_pattern(e["pattern"], e["guides"], m), want, len(e["guides"]))
            assert ctx.timing()["sites"] == e["n_cands"]
    finally:
        gen.close()


# ---- 2. the independent pin: the plain scan, where the two definitions coincide -------------------------------------------
def test_equals_the_plain_scan_where_the_definitions_coincide(ctx):
    m = 4
    guides = random_guides(np.random.default_rng(41), 8)
    contigs = make_genome(41, [14000, 5000, 40], guides, m, n_plant=80, n_runs=3)
    gen = ctx.load_genome(va.PackedGenome.from_sequences(contigs))
    try:
        plain = gen.search(guides, m, algorithm="scan").to_numpy()
        rec, rows = gen.search_pattern("N" * 21 + "GR", guides, m)
    finally:
        gen.close()
    key = lambda guide, strand, contig, pos, nm, mask: (int(guide), int(strand), int(contig), int(pos), int(nm), int(mask))
    a = [key(r["guide"], r["info"] >> 31, r["contig"], r["pos"], (r["info"] >> 23) & 0xFF, r["info"] & 0x7FFFFF) for r in plain]
    b = [key(r["guide"], r["info"] >> 31, r["contig"], r["pos"], r["info"] & 63, r["mask"]) for r in rec]
    at_end = lambda h: h[3] + 23 == len(contigs[h[2]])
    assert [h for h in a if not at_end(h)] == [h for h in b if not at_end(h)]  # identical, order included
    ends_a, ends_b = {h for h in a if at_end(h)}, {h for h in b if at_end(h)}
    assert ends_a <= ends_b and ends_b                                          # the right-edge rule only ever drops
    assert len(a) - len(ends_a) >= 20 and {h[1] for h in a} == {0, 1}
    assert rows.sum() == len(b)


# ---- 3. a tandem array ----------------------------------------------------------------------------------------------------
def test_tandem_array(ctx):
    t = pc.tandem_scenario()
    gen = ctx.load_genome(va.PackedGenome.from_sequences(t["contigs"]))
    try:
        same(gen.search_pattern(t["pattern"], t["guides"], t["m"]), t["hits"], 2)
    finally:
        gen.close()


# ---- 4. rounds ------------------------------------------------------------------------------------------------------------
def test_guide_batch_never_changes_the_bytes(edge, edge_gen):
    n = len(edge["guides"])
    for batch in (1, 2, 0):
        same(edge_gen.search_pattern(edge["pattern"], edge["guides"], edge["m"], guide_batch=batch), edge["want"], n)


def test_seventy_guides_take_two_rounds(ctx, edge_gen):
    s = pc.many_guides_scenario()
    for batch in (64, 1000, 0):
        same(edge_gen.search_pattern(s["pattern"], s["guides"], s["m"], guide_batch=batch), s["hits"], 70)
        assert ctx.timing()["passes"] == (2 if batch else 5)


# ---- 5. rows only, records only -------------------------------------------------------------------------------------------
def test_rows_and_records_alone(edge, edge_gen):
    rec, rows = edge_gen.search_pattern(edge["pattern"], edge["guides"], edge["m"], records=False)
    assert rec is None and rows.tobytes() == edge["rows"].tobytes()
    rec, rows = edge_gen.search_pattern(edge["pattern"], edge["guides"], edge["m"], rows=False)
    assert rows is None and rec.tobytes() == edge["rec"].tobytes()


# ---- 6. the cap -----------------------------------------------------------------------------------------------------------
def test_max_hits(edge, edge_gen):
    n = len(edge["want"])
    with pytest.raises(va.VarscotError) as err:
        edge_gen.search_pattern(edge["pattern"], edge["guides"], edge["m"], max_hits=n - 1, guide_batch=3)
    assert err.value.code == -34 and (" %d records" % n) in str(err.value)
    same(edge_gen.search_pattern(edge["pattern"], edge["guides"], edge["m"], max_hits=n), edge["want"], len(edge["guides"]))


def test_max_hits_in_the_first_round(edge, edge_gen):
    """The cap trips in round 0: the rounds behind it are counted only (the message names the whole call's records), nothing
    of them is written, and the next call finds the context and the genome as they were."""
    n, n_guides = len(edge["want"]), len(edge["guides"])
    batch = next(b for b in range(1, n_guides + 1) if sum(h[0] < b for h in edge["want"]) >= 2)
    first = sum(h[0] < batch for h in edge["want"])
    cap = first - 1
    assert cap >= 1 and first > cap and -(-n_guides // batch) - 1 >= 2 and n > first
    with pytest.raises(va.VarscotError) as err:
        edge_gen.search_pattern(edge["pattern"], edge["guides"], edge["m"], max_hits=cap, guide_batch=batch)
    assert err.value.code == -34 and (" %d records" % n) in str(err.value) and ("max_hits = %d" % cap) in str(err.value)
    same(edge_gen.search_pattern(edge["pattern"], edge["guides"], edge["m"], guide_batch=batch), edge["want"], n_guides)


# ---- 7. shards ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
def test_shards_merge_to_the_whole(ctx, edge, world):
    recs, rows = [], np.zeros_like(edge["rows"])
    for rank in range(world):
        g = ctx.load_genome(edge["packed"], rank, world)
        r, w = g.search_pattern(edge["pattern"], edge["guides"], edge["m"])
        g.close()
        recs.append(r)
        rows += w
    assert sum(len(r) > 0 for r in recs) >= 2
    merged = np.concatenate(recs)
    merged = merged[pc.merge_order(merged)]
    assert merged.tobytes() == edge["rec"].tobytes() and rows.tobytes() == edge["rows"].tobytes()


# ---- 8., 9. repetition and the timing fields ------------------------------------------------------------------------------
def test_second_call_and_timing(ctx, edge, edge_gen):
    n = len(edge["guides"])
    a = edge_gen.search_pattern(edge["pattern"], edge["guides"], edge["m"])
    t = ctx.timing()
    b = edge_gen.search_pattern(edge["pattern"], edge["guides"], edge["m"])
    assert a[0].tobytes() == b[0].tobytes() == edge["rec"].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert t["hits"] == len(edge["want"]) and t["sites"] == edge["n_cands"] and t["pairs"] == edge["n_cands"] * n and t["passes"] == 1
    assert t["scan_ms"] > 0 and t["total_ms"] == t["scan_ms"]
    assert t["sort_ms"] == 0 and t["finalize_ms"] == 0 and t["score_ms"] == 0 and t["sort_bytes"] == 0 and t["sort_levels"] == 0
    assert t["algorithm"] == 1
    edge_gen.search_pattern(edge["pattern"], edge["guides"][:3], 2, records=False, guide_batch=2)
    t = ctx.timing()
    want = [h for h in edge["want"] if h[0] < 3 and h[4] <= 2]
    assert t["sites"] == edge["n_cands"] and t["pairs"] == 3 * edge["n_cands"] and t["hits"] == len(want) and t["passes"] == 2


def test_no_guides_and_the_plain_search_beside_it(ctx, edge, edge_gen):
    rec, rows = edge_gen.search_pattern(edge["pattern"], [], 4)
    assert len(rec) == 0 and rows.shape == (0, 9)
    reads = random_guides(np.random.default_rng(5), 4)
    plain = edge_gen.search(reads, 4, algorithm="scan").to_numpy()
    same(edge_gen.search_pattern(edge["pattern"], edge["guides"], edge["m"]), edge["want"], len(edge["guides"]))
    assert edge_gen.search(reads, 4, algorithm="scan").to_numpy().tobytes() == plain.tobytes()
    ctx.release_scratch()  # the pools come back on the next call
    same(edge_gen.search_pattern(edge["pattern"], edge["guides"], edge["m"]), edge["want"], len(edge["guides"]))


def test_parameter_validation(ctx, edge, edge_gen):
    p, gs = edge["pattern"], edge["guides"]
    for kw in (dict(max_mismatches=9), dict(max_mismatches=3, records=False, rows=False)):
        with pytest.raises(va.VarscotError) as err:
            edge_gen.search_pattern(p, gs, **kw)
        assert err.value.code == -22 and "vsc_search_pattern" in str(err.value)
    for pattern, guides in (("N" * 15, ["A" * 15]), ("N" * 33, ["A" * 33]), ("N" * 20 + "UGG", ["A" * 23]), ("N" * 23, ["A" * 22 + "U"]),
                            ("N" * 23, ["A" * 23, "A" * 11 + "x" + "A" * 11])):
        with pytest.raises(va.VarscotError) as err:
            edge_gen.search_pattern(pattern, guides, 3)
        assert err.value.code == -22
    with pytest.raises(ValueError):
        edge_gen.search_pattern(p, [gs[0], gs[1][:-1]], 3)  # a guide of another length
    L, rows = va.lib(), np.zeros((1, 9), dtype=np.uint32)
    pp = va.PatternParams(3, 0, 0)
    pp.reserved[1] = 1
    assert L.vsc_search_pattern(ctx._h, edge_gen._h, p.encode(), gs[0].encode(), 1, 23, C.byref(pp), None, rows.ctypes.data) == -22
    pp.reserved[1] = 0
    assert L.vsc_search_pattern(ctx._h, edge_gen._h, p.encode(), gs[0].encode(), 1, 23, C.byref(pp), None, rows.ctypes.data) == 0


# ---- 10. pattern_search end to end ----------------------------------------------------------------------------------------
def test_pattern_search_tool(tmp_path, edge):
    names = ["c%d" % i for i in range(len(edge["contigs"]))]
    with open(tmp_path / "g.fa", "w") as f:
        for n, s in zip(names, edge["contigs"]):
            f.write(">%s some text\n%s\n" % (n, s))
    with open(tmp_path / "guides.fa", "w") as f:
        for i, g in enumerate(edge["guides"]):
            f.write(">g%d\n%s\n" % (i, g))
    run = lambda *a: subprocess.run([os.path.join(BIN, a[0])] + list(a[1:]), capture_output=True, text=True, timeout=600)
    assert run("bidir_index", "-G", str(tmp_path / "g.fa"), "-I", str(tmp_path / "idx")).returncode == 0
    r = run("pattern_search", "-i", str(tmp_path / "idx"), "-q", edge["pattern"], "-R", str(tmp_path / "guides.fa"), "-M", str(edge["m"]),
            "-O", str(tmp_path / "sum.tsv"), "-T", str(tmp_path / "hits.tsv"))
    assert r.returncode == 0, r.stderr
    lines = [l.rstrip("\n").split("\t") for l in open(tmp_path / "sum.tsv")]
    assert lines[0] == ["#guideId", "guideSeq", "offtargetCount"] + ["mm%d" % k for k in range(edge["m"] + 1)]
    for g, row in enumerate(lines[1:]):
        counts = [int(x) for x in edge["rows"][g, :edge["m"] + 1]]
        assert row == ["g%d" % g, edge["guides"][g], str(sum(counts))] + [str(x) for x in counts]
    assert len(lines) == 1 + len(edge["guides"])
    lines = [l.rstrip("\n").split("\t") for l in open(tmp_path / "hits.tsv")]
    assert lines[0] == ["#guideId", "chrom", "start", "end", "strand", "mismatches", "mismatchPositions", "sequence"]
    listed = [("g%d" % g, names[c], str(p), str(p + 23), "+-"[s], str(nm), ",".join(str(b) for b in range(23) if (mask >> b) & 1) or "-",
               pc.genome_of(edge["contigs"][c])[p:p + 23]) for g, s, c, p, nm, mask in edge["want"]]
    assert [tuple(l) for l in lines[1:]] == listed
    # rows alone: no -T
    r = run("pattern_search", "-i", str(tmp_path / "idx"), "-q", edge["pattern"], "-R", str(tmp_path / "guides.fa"), "-M", "2",
            "-O", str(tmp_path / "sum2.tsv"))
    assert r.returncode == 0, r.stderr
    assert [l.split("\t")[2] for l in open(tmp_path / "sum2.tsv")][1:] == [str(int(edge["rows"][g, :3].sum())) for g in range(len(edge["guides"]))]
