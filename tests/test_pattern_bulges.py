"""vsc_search_pattern_bulges on the device: records and rows byte for byte what the definition gives when it is applied site
by site (tests/pattern_bulge_cases.py) - SaCas9 and Cas12a over the budgets and the classes; byte-equal to vsc_search_bulges
where the two definitions coincide; a tandem array, the rounds, the two outputs, the cap, shards, repetition, the timing
fields, the limits of the length, the fullest queue and pattern_search -u end to end."""
import os
import subprocess

import numpy as np
import pytest

import varscot_amd as va
import bulges_cases as bc
import pattern_bulge_cases as pb
import pattern_cases as pc

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
    e = dict(pb.edge_scenario("SaCas9"))
    e["packed"] = va.PackedGenome.from_sequences(e["contigs"])
    e["rec"], e["rows"] = pb.arrays(e["hits"], len(e["guides"]))
    return e


@pytest.fixture(scope="module")
def edge_gen(ctx, edge):
    g = ctx.load_genome(edge["packed"])
    yield g
    g.close()


def search(gen, e, m=None, dna=None, rna=None, guides=None, **kw):
    return gen.search_pattern_bulges(e["pattern"], e["guides"] if guides is None else guides, e["m"] if m is None else m, e["proto"],
                                     dna=e["dna"] if dna is None else dna, rna=e["rna"] if rna is None else rna, **kw)


def same(got, want_hits, n_guides):
    rec, rows = pb.arrays(want_hits, n_guides)
    assert got[0].dtype == va.BULGE_HIT_DTYPE and got[1].dtype == np.uint32 and got[1].shape == (n_guides, 4, 9)
    assert len(got[0]) == len(rec)
    assert got[0].tobytes() == rec.tobytes()
    assert got[1].tobytes() == rows.tobytes()


# ---- 1. the edge layouts over budgets and classes -------------------------------------------------------------------------
@pytest.mark.parametrize("preset", ["SaCas9", "Cas12a"])
def test_edge_layout_equals_the_definition(ctx, preset):
    e = pb.edge_scenario(preset)
    n = len(e["guides"])
    gen = ctx.load_genome(va.PackedGenome.from_sequences(e["contigs"]))
    try:
        same(search(gen, e), e["hits"], n)
        assert ctx.timing()["sites"] == e["n_cands"]
        # m = 8 is beyond the scenario's stored hits: the restatement runs again over the stored candidates
        for m in (0, 3, 8):
            for dna, rna in ((1, 0), (0, 2), (2, 2)):
                cands = [x for x in e["cands"] if x[3] in pb.enabled(dna, rna)]
                want = pb.hits_at(e, m, dna, rna) if m <= e["m"] else pb.brute_force(e["contigs"], e["pattern"], e["guides"], e["proto"], m, dna, rna, cands=cands)[0]
                assert want and {h[1] for h in want} == {0, 1} and {h[4] for h in want} == set(pb.enabled(dna, rna))
                same(search(gen, e, m=m, dna=dna, rna=rna), want, n)
                assert ctx.timing()["sites"] == len(cands)
    finally:
        gen.close()


# ---- 2. the anchor: vsc_search_bulges, where the two definitions coincide --------------------------------------------------
def test_equals_the_bulge_search_on_its_own_scenario(ctx):
    e = bc.edge_scenario()
    guides = [bc.read_of(g) for g in e["guides"]]  # spelled 23-letter ACGT guides (search_bulges reads a non-ACGT letter as A)
    gen = ctx.load_genome(va.PackedGenome.from_sequences(e["contigs"]))
    try:
        for m, dna, rna in ((bc.EDGE_M, 2, 2), (2, 1, 1), (3, 0, 2)):
            want = gen.search_bulges(guides, m, dna=dna, rna=rna)
            got = gen.search_pattern_bulges("N" * 21 + "GR", guides, m, (0, 20), dna=dna, rna=rna)
            assert len(want[0]) >= 20
            assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    finally:
        gen.close()


# ---- 3. a tandem array ----------------------------------------------------------------------------------------------------
def test_tandem_array(ctx):
    t = pb.tandem_scenario()
    gen = ctx.load_genome(va.PackedGenome.from_sequences(t["contigs"]))
    try:
        same(search(gen, t), t["hits"], 2)
    finally:
        gen.close()


# ---- 4. rounds ------------------------------------------------------------------------------------------------------------
def test_guide_batch_never_changes_the_bytes(ctx, edge_gen):
    s = pb.many_guides_scenario()
    for batch, passes in ((1, 70), (2, 35), (0, 5), (64, 2)):
        same(search(edge_gen, s, guide_batch=batch), s["hits"], 70)
        assert ctx.timing()["passes"] == passes


# ---- 5. rows only, records only -------------------------------------------------------------------------------------------
def test_rows_and_records_alone(edge, edge_gen):
    rec, rows = search(edge_gen, edge, records=False)
    assert rec is None and rows.tobytes() == edge["rows"].tobytes()
    rec, rows = search(edge_gen, edge, rows=False)
    assert rows is None and rec.tobytes() == edge["rec"].tobytes()


# ---- 6. the cap -----------------------------------------------------------------------------------------------------------
def test_max_hits(edge, edge_gen):
    n = len(edge["hits"])
    with pytest.raises(va.VarscotError) as err:
        search(edge_gen, edge, max_hits=n - 1, guide_batch=3)
    assert err.value.code == -34 and (" %d records" % n) in str(err.value) and "vsc_search_pattern_bulges" in str(err.value)
    same(search(edge_gen, edge, max_hits=n), edge["hits"], len(edge["guides"]))


def test_max_hits_in_the_first_round(edge, edge_gen):
    """The cap trips in round 0: the rounds behind it are counted only (the message names the whole call's records), nothing
    of them is written, and the next call finds the context and the genome as they were."""
    n, n_guides = len(edge["hits"]), len(edge["guides"])
    batch = next(b for b in range(1, n_guides + 1) if sum(h[0] < b for h in edge["hits"]) >= 2)
    first = sum(h[0] < batch for h in edge["hits"])
    cap = first - 1
    assert cap >= 1 and first > cap and -(-n_guides // batch) - 1 >= 2 and n > first
    with pytest.raises(va.VarscotError) as err:
        search(edge_gen, edge, max_hits=cap, guide_batch=batch)
    assert err.value.code == -34 and (" %d records" % n) in str(err.value) and ("max_hits = %d" % cap) in str(err.value)
    assert "vsc_search_pattern_bulges" in str(err.value)
    same(search(edge_gen, edge, guide_batch=batch), edge["hits"], n_guides)


# ---- 7. shards ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
def test_shards_merge_to_the_whole(ctx, edge, world):
    recs, rows = [], np.zeros_like(edge["rows"])
    for rank in range(world):
        g = ctx.load_genome(edge["packed"], rank, world)
        r, w = search(g, edge)
        g.close()
        recs.append(r)
        rows += w
    assert sum(len(r) > 0 for r in recs) >= 2
    merged = np.concatenate(recs)
    merged = merged[pb.merge_order(merged)]
    assert merged.tobytes() == edge["rec"].tobytes() and rows.tobytes() == edge["rows"].tobytes()


# ---- 8., 9. repetition, the timing fields, the plain pattern search beside it ------------------------------------------------
def test_second_call_and_timing(ctx, edge, edge_gen):
    n = len(edge["guides"])
    a = search(edge_gen, edge)
    t = ctx.timing()
    b = search(edge_gen, edge)
    assert a[0].tobytes() == b[0].tobytes() == edge["rec"].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert t["hits"] == len(edge["hits"]) and t["sites"] == edge["n_cands"] and t["pairs"] == edge["n_cands"] * n and t["passes"] == 1
    assert t["scan_ms"] > 0 and t["total_ms"] == t["scan_ms"]
    assert t["sort_ms"] == 0 and t["finalize_ms"] == 0 and t["score_ms"] == 0 and t["sort_bytes"] == 0 and t["sort_levels"] == 0
    assert t["algorithm"] == 1
    search(edge_gen, edge, m=2, dna=1, rna=0, guides=edge["guides"][:3], records=False, guide_batch=2)
    t = ctx.timing()
    want = pb.hits_at(edge, 2, 1, 0, guides=3)
    sites = pb.cands_at(edge, 1, 0)
    assert t["sites"] == sites and t["pairs"] == 3 * sites and t["hits"] == len(want) and t["passes"] == 2


def test_no_guides_and_the_plain_pattern_search_beside_it(ctx, edge, edge_gen):
    rec, rows = search(edge_gen, edge, guides=[])
    assert len(rec) == 0 and rows.shape == (0, 4, 9)
    plain = edge_gen.search_pattern(edge["pattern"], edge["guides"], 4)
    same(search(edge_gen, edge), edge["hits"], len(edge["guides"]))
    again = edge_gen.search_pattern(edge["pattern"], edge["guides"], 4)
    assert again[0].tobytes() == plain[0].tobytes() and again[1].tobytes() == plain[1].tobytes() and len(plain[0])
    ctx.release_scratch()  # the pools come back on the next call
    same(search(edge_gen, edge), edge["hits"], len(edge["guides"]))
    again = edge_gen.search_pattern(edge["pattern"], edge["guides"], 4)
    assert again[0].tobytes() == plain[0].tobytes() and again[1].tobytes() == plain[1].tobytes()


def test_refusals_reach_the_caller(edge, edge_gen):
    for kw in (dict(m=9), dict(records=False, rows=False), dict(dna=0, rna=0), dict(dna=3)):
        with pytest.raises(va.VarscotError) as err:
            search(edge_gen, edge, **kw)
        assert err.value.code == -22 and "vsc_search_pattern_bulges" in str(err.value)
    with pytest.raises(va.VarscotError) as err:
        edge_gen.search_pattern_bulges(edge["pattern"], edge["guides"], 3, (0, 24))  # the PAM's G inside the protospacer
    assert err.value.code == -22 and "protospacer" in str(err.value)


# ---- 10. the limits of the length ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", sorted(pb.LIMITS))
def test_length_limits(ctx, L):
    e = pb.limit_scenario(L)
    gen = ctx.load_genome(va.PackedGenome.from_sequences(e["contigs"]))
    try:
        same(search(gen, e), e["hits"], len(e["guides"]))
        assert ctx.timing()["sites"] == e["n_cands"]
        if L == 16:  # one step over the limit (L = 31 with dna = 2 is refused in test_pattern_bulges_cpu.py: it needs no genome)
            with pytest.raises(va.VarscotError) as err:
                search(gen, e, rna=1)
            assert err.value.code == -22 and "at least 16" in str(err.value)
    finally:
        gen.close()


# ---- 11. the fullest queue --------------------------------------------------------------------------------------------------
def test_all_n_pattern_with_four_classes(ctx):
    e = pb.all_n_scenario()
    gen = ctx.load_genome(va.PackedGenome.from_sequences(e["contigs"]))
    try:
        same(search(gen, e), e["hits"], len(e["guides"]))
        assert ctx.timing()["sites"] == e["n_cands"]
        rec, rows = search(gen, e, rows=False)
        assert rows is None and rec.tobytes() == pb.arrays(e["hits"], len(e["guides"]))[0].tobytes()
    finally:
        gen.close()


# ---- 12. pattern_search -u end to end ---------------------------------------------------------------------------------------
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
    m, L = edge["m"], len(edge["pattern"])
    common = ["-i", str(tmp_path / "idx"), "-q", edge["pattern"], "-R", str(tmp_path / "guides.fa"), "-M", str(m)]
    r = run("pattern_search", *common, "-O", str(tmp_path / "plain.tsv"), "-T", str(tmp_path / "plain_hits.tsv"))
    assert r.returncode == 0, r.stderr
    r = run("pattern_search", *common, "-O", str(tmp_path / "sum.tsv"), "-T", str(tmp_path / "hits.tsv"), "-u", "2,1", "-p", "%d,%d" % edge["proto"],
            "-U", str(tmp_path / "bulges.tsv"))
    assert r.returncode == 0, r.stderr
    want = pb.hits_at(edge, m, 2, 1)
    rows = pb.arrays(want, len(edge["guides"]))[1]
    plain = [l.rstrip("\n").split("\t") for l in open(tmp_path / "plain.tsv")]
    lines = [l.rstrip("\n").split("\t") for l in open(tmp_path / "sum.tsv")]
    classes = [(1, "br1"), (2, "bd1"), (3, "bd2")]
    assert lines[0] == plain[0] + ["bulgeCount"] + ["%smm%d" % (name, k) for _, name in classes for k in range(m + 1)]
    assert len(lines) == 1 + len(edge["guides"])
    for g, row in enumerate(lines[1:]):
        counts = [int(rows[g, c, k]) for c, _ in classes for k in range(m + 1)]
        assert row == plain[1 + g] + [str(sum(counts))] + [str(x) for x in counts]
    assert open(tmp_path / "hits.tsv").read() == open(tmp_path / "plain_hits.tsv").read()  # -T is what it was
    lines = [l.rstrip("\n").split("\t") for l in open(tmp_path / "bulges.tsv")]
    assert lines[0] == ["#guideId", "chrom", "start", "end", "strand", "kind", "size", "index", "mismatches", "sequence"]
    listed = [("g%d" % g, names[c], str(p), str(p + L + d), "+-"[s], "DNA" if d > 0 else "RNA", str(abs(d)), str(index), str(nm),
               pc.genome_of(edge["contigs"][c])[p:p + L + d]) for g, s, c, p, d, nm, index, _ in want]
    assert [tuple(l) for l in lines[1:]] == listed and listed
    # the bulged sites alone: -U without -O / -T
    r = run("pattern_search", *common, "-u", "0,2", "-p", "%d,%d" % edge["proto"], "-U", str(tmp_path / "rna.tsv"))
    assert r.returncode == 0, r.stderr
    assert len(open(tmp_path / "rna.tsv").readlines()) == 1 + len(pb.hits_at(edge, m, 0, 2))
    # -E -M -O -u: the guides found in a target are screened with bulges in the same run
    (tmp_path / "t.bed").write_text("c0\t100\t420\n")
    r = run("pattern_search", "-i", str(tmp_path / "idx"), "-q", edge["pattern"], "-E", str(tmp_path / "found.tsv"), "-B", str(tmp_path / "t.bed"),
            "-p", "%d,%d" % edge["proto"], "-M", "2", "-O", str(tmp_path / "design.tsv"), "-u", "1,0")
    assert r.returncode == 0, r.stderr
    found = [l.split("\t")[0] for l in open(tmp_path / "found.tsv")][1:]
    assert len(found) >= 5 and all(len(g) == L for g in found)
    want = pb.brute_force(edge["contigs"], edge["pattern"], found, edge["proto"], 2, 1, 0, cands=[x for x in edge["cands"] if x[3] == 1])[0]
    rows = pb.arrays(want, len(found))[1]
    lines = [l.rstrip("\n").split("\t") for l in open(tmp_path / "design.tsv")]
    assert lines[0][-4:] == ["bulgeCount", "bd1mm0", "bd1mm1", "bd1mm2"] and len(lines) == 1 + len(found)
    assert [row[-3:] for row in lines[1:]] == [[str(int(x)) for x in rows[g, 2, :3]] for g in range(len(found))]
    assert [row[-4] for row in lines[1:]] == [str(int(rows[g, 2, :3].sum())) for g in range(len(found))] and rows.sum() > 0
