"""vsc_search_bulges on the device: records and rows byte for byte what the definition gives when it is applied site by site
(tests/bulges_cases.py) - over the front end's edge cases, the PAM set, the budgets, the classes, a tandem array, the rounds,
the two outputs, the cap, shards, repetition, the timing fields and guide_summary -u / -U."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import varscot_amd as va
import bulges_cases as bc

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
    e = bc.edge_scenario()
    e["packed"] = va.PackedGenome.from_sequences(e["contigs"])
    e["rec"], e["rows"] = bc.arrays(e["hits"], len(e["guides"]))
    return e


@pytest.fixture(scope="module")
def edge_gen(ctx, edge):
    g = ctx.load_genome(edge["packed"])
    yield g
    g.close()


def same(got, want_hits, n_guides):
    rec, rows = bc.arrays(want_hits, n_guides)
    assert got[0].dtype == va.BULGE_HIT_DTYPE and got[1].dtype == np.uint32 and got[1].shape == (n_guides, 4, 9)
    assert len(got[0]) == len(rec)
    assert got[0].tobytes() == rec.tobytes()
    assert got[1].tobytes() == rows.tobytes()


# ---- 1. the edge layout ---------------------------------------------------------------------------------------------------
def test_edge_layout_equals_the_definition(edge, edge_gen):
    got = edge_gen.search_bulges(edge["guides"], bc.EDGE_M, dna=2, rna=2)
    same(got, edge["hits"], len(edge["guides"]))
    f = va.unpack_bulge_info(got[0]["info"])
    assert {int(x) for x in f["d"]} == {-2, -1, 1, 2} and {int(x) for x in f["strand"]} == {0, 1}


# ---- 2. PAM set, budgets, classes -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [0, 3, 8])
@pytest.mark.parametrize("dna,rna", [(1, 0), (0, 2), (2, 2)])
def test_budgets_and_classes(edge, edge_gen, m, dna, rna):
    want = bc.brute_force(edge["contigs"], edge["guides"], m, dna, rna)
    assert want and {h[4] for h in want} == set(bc.enabled(dna, rna))
    assert max(h[5] for h in want) == m
    same(edge_gen.search_bulges(edge["guides"], m, dna=dna, rna=rna), want, len(edge["guides"]))


def test_pam_ga_and_an_extra_pam(edge, edge_gen):
    plain = [h for h in edge["hits"]]
    ga = [h for h in plain if bc.genome_of(edge["contigs"][h[2]])[h[3]:h[3] + 23 + h[4]][-2:] == "GA" and h[1] == 0]
    assert ga  # hits that end in GA are there without -P
    want = bc.brute_force(edge["contigs"], edge["guides"], bc.EDGE_M, 2, 2, extra_pam="AG")
    assert len(want) > len(plain)
    same(edge_gen.search_bulges(edge["guides"], bc.EDGE_M, dna=2, rna=2, extra_pam="ag"), want, len(edge["guides"]))


# ---- 3. a tandem array ----------------------------------------------------------------------------------------------------
def test_tandem_array(ctx):
    t = bc.tandem_scenario()
    gen = ctx.load_genome(va.PackedGenome.from_sequences(t["contigs"]))
    try:
        same(gen.search_bulges(t["guides"], 3), t["hits"], 2)
    finally:
        gen.close()


# ---- 4. rounds ------------------------------------------------------------------------------------------------------------
def test_guide_batch_never_changes_the_bytes(edge, edge_gen):
    guides = edge["guides"][:5]
    want = [h for h in edge["hits"] if h[0] < 5]
    assert {h[0] for h in want} == set(range(5))
    for batch in (1, 2, 0):
        same(edge_gen.search_bulges(guides, bc.EDGE_M, dna=2, rna=2, guide_batch=batch), want, 5)


# ---- 5. rows only, records only, both -------------------------------------------------------------------------------------
def test_rows_and_records_alone(edge, edge_gen):
    rec, rows = edge_gen.search_bulges(edge["guides"], bc.EDGE_M, dna=2, rna=2, records=False)
    assert rec is None and rows.tobytes() == edge["rows"].tobytes()
    rec, rows = edge_gen.search_bulges(edge["guides"], bc.EDGE_M, dna=2, rna=2, rows=False)
    assert rows is None and rec.tobytes() == edge["rec"].tobytes()


# ---- 6. the cap -----------------------------------------------------------------------------------------------------------
def test_max_hits(edge, edge_gen):
    n = len(edge["hits"])
    with pytest.raises(va.VarscotError) as err:
        edge_gen.search_bulges(edge["guides"], bc.EDGE_M, dna=2, rna=2, max_hits=n - 1, guide_batch=3)
    assert err.value.code == -34 and (" %d records" % n) in str(err.value)
    same(edge_gen.search_bulges(edge["guides"], bc.EDGE_M, dna=2, rna=2, max_hits=n), edge["hits"], len(edge["guides"]))


def test_max_hits_in_the_first_round(edge, edge_gen):
    """The cap trips in round 0: the rounds behind it are counted only (the message names the whole call's records), nothing
    of them is written, and the next call finds the context and the genome as they were."""
    n, n_guides = len(edge["hits"]), len(edge["guides"])
    batch = next(b for b in range(1, n_guides + 1) if sum(h[0] < b for h in edge["hits"]) >= 2)
    first = sum(h[0] < batch for h in edge["hits"])
    cap = first - 1
    assert cap >= 1 and first > cap and -(-n_guides // batch) - 1 >= 2 and n > first
    with pytest.raises(va.VarscotError) as err:
        edge_gen.search_bulges(edge["guides"], bc.EDGE_M, dna=2, rna=2, max_hits=cap, guide_batch=batch)
    assert err.value.code == -34 and (" %d records" % n) in str(err.value) and ("max_hits = %d" % cap) in str(err.value)
    same(edge_gen.search_bulges(edge["guides"], bc.EDGE_M, dna=2, rna=2, guide_batch=batch), edge["hits"], n_guides)


# ---- 7. shards ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
def test_shards_merge_to_the_whole(ctx, edge, world):
    recs, rows = [], np.zeros_like(edge["rows"])
    for rank in range(world):
        g = ctx.load_genome(edge["packed"], rank, world)
        r, w = g.search_bulges(edge["guides"], bc.EDGE_M, dna=2, rna=2)
        g.close()
        recs.append(r)
        rows += w
    assert sum(len(r) > 0 for r in recs) >= 2
    merged = np.concatenate(recs)
    merged = merged[bc.merge_order(merged)]
    assert merged.tobytes() == edge["rec"].tobytes() and rows.tobytes() == edge["rows"].tobytes()


# ---- 8., 9. repetition and the timing fields ------------------------------------------------------------------------------
def test_second_call_and_timing(ctx, edge, edge_gen):
    a = edge_gen.search_bulges(edge["guides"], bc.EDGE_M, dna=2, rna=2)
    t = ctx.timing()
    b = edge_gen.search_bulges(edge["guides"], bc.EDGE_M, dna=2, rna=2)
    assert a[0].tobytes() == b[0].tobytes() == edge["rec"].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert t["hits"] == len(edge["hits"]) and t["sites"] == len(edge["cands"]) and t["pairs"] == len(edge["cands"]) * len(edge["guides"])
    assert t["scan_ms"] > 0 and t["total_ms"] == t["scan_ms"]
    assert t["sort_ms"] == 0 and t["finalize_ms"] == 0 and t["score_ms"] == 0 and t["sort_bytes"] == 0 and t["sort_levels"] == 0
    assert t["algorithm"] == 1
    edge_gen.search_bulges(edge["guides"][:3], 2, dna=1, rna=0, records=False, guide_batch=2)
    t = ctx.timing()
    c1 = bc.candidates(edge["contigs"], 1, 0)
    want = bc.brute_force(edge["contigs"], edge["guides"][:3], 2, 1, 0, cands=c1)
    assert t["sites"] == len(c1) and t["pairs"] == 3 * len(c1) and t["hits"] == len(want) and t["passes"] == 2


def test_no_guides_and_the_plain_search_beside_it(ctx, edge, edge_gen):
    rec, rows = edge_gen.search_bulges([], 4)
    assert len(rec) == 0 and rows.shape == (0, 4, 9)
    plain = edge_gen.search(edge["guides"], bc.EDGE_M, algorithm="scan").to_numpy()
    got = edge_gen.search_bulges(edge["guides"], bc.EDGE_M, dna=2, rna=2)
    same(got, edge["hits"], len(edge["guides"]))
    assert edge_gen.search(edge["guides"], bc.EDGE_M, algorithm="scan").to_numpy().tobytes() == plain.tobytes()


def test_parameter_validation(ctx, edge, edge_gen):
    bad = [dict(dna=0, rna=0), dict(dna=3, rna=1), dict(dna=1, rna=3), dict(records=False, rows=False)]
    for kw in bad:
        with pytest.raises(va.VarscotError) as err:
            edge_gen.search_bulges(edge["guides"], 3, **kw)
        assert err.value.code == -22 and "vsc_search_bulges" in str(err.value)
    with pytest.raises(va.VarscotError) as err:
        edge_gen.search_bulges(edge["guides"], 9)
    assert err.value.code == -22
    L, codes = va.lib(), va.pack_guides(edge["guides"])
    p, bp, rows = edge_gen._params(3, None, "seed"), va.BulgeParams(1, 1, 0, 0, 0), np.zeros((len(codes), 4, 9), dtype=np.uint32)
    assert L.vsc_search_bulges(ctx._h, edge_gen._h, codes.ctypes.data, len(codes), C.byref(p), C.byref(bp), None, rows.ctypes.data) == -22  # the seed algorithm
    bp.reserved = 1
    p = edge_gen._params(3, None, "scan")
    assert L.vsc_search_bulges(ctx._h, edge_gen._h, codes.ctypes.data, len(codes), C.byref(p), C.byref(bp), None, rows.ctypes.data) == -22


# ---- 10. guide_summary -u / -U --------------------------------------------------------------------------------------------
def test_guide_summary_bulge_columns(tmp_path, edge):
    names = ["c%d" % i for i in range(len(edge["contigs"]))]
    with open(tmp_path / "g.fa", "w") as f:
        for n, s in zip(names, edge["contigs"]):
            f.write(">%s\n%s\n" % (n, s))
    with open(tmp_path / "reads.fa", "w") as f:
        for i, g in enumerate(edge["guides"]):
            f.write(">g%d\n%s\n" % (i, g))
    run = lambda *a: subprocess.run([os.path.join(BIN, a[0])] + list(a[1:]), capture_output=True, text=True, timeout=600)
    assert run("bidir_index", "-G", str(tmp_path / "g.fa"), "-I", str(tmp_path / "idx")).returncode == 0
    base = ["guide_summary", "-G", str(tmp_path / "g.fa"), "-I", str(tmp_path / "idx"), "-R", str(tmp_path / "reads.fa"), "-M", str(bc.EDGE_M)]
    before = run(*base, "-O", str(tmp_path / "plain.tsv"))
    assert before.returncode == 0, before.stderr
    r = run(*base, "-u", "2,1", "-U", str(tmp_path / "bulges.tsv"), "-O", str(tmp_path / "with.tsv"))
    assert r.returncode == 0, r.stderr
    plain = [l.rstrip("\n").split("\t") for l in open(tmp_path / "plain.tsv")]
    with_u = [l.rstrip("\n").split("\t") for l in open(tmp_path / "with.tsv")]
    n_plain = len(plain[0])
    assert [row[:n_plain] for row in with_u] == plain  # every earlier column is what it was
    classes = [("br1", -1), ("bd1", 1), ("bd2", 2)]  # ascending d among the enabled classes
    header = ["bulgeCount"] + ["%smm%d" % (name, k) for name, _ in classes for k in range(bc.EDGE_M + 1)]
    assert with_u[0][n_plain:] == header
    want = bc.brute_force(edge["contigs"], edge["guides"], bc.EDGE_M, 2, 1)
    _, rows = bc.arrays(want, len(edge["guides"]))
    for g, row in enumerate(with_u[1:]):
        cells = [int(rows[g].sum())] + [int(rows[g, bc.CLASSES.index(d), k]) for _, d in classes for k in range(bc.EDGE_M + 1)]
        assert row[0] == "g%d" % g and [int(x) for x in row[n_plain:]] == cells
    lines = [l.rstrip("\n").split("\t") for l in open(tmp_path / "bulges.tsv")]
    assert lines[0] == ["#guideId", "chrom", "start", "end", "strand", "kind", "size", "index", "mismatches", "sequence"]
    listed = [("g%d" % g, names[c], str(p), str(p + 23 + d), "+-"[s], "DNA" if d > 0 else "RNA", str(abs(d)), str(i), str(nm),
               bc.genome_of(edge["contigs"][c])[p:p + 23 + d]) for g, s, c, p, d, nm, i, _ in want]
    assert [tuple(l) for l in lines[1:]] == listed
