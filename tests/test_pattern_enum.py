"""vsc_guides_enumerate_pattern on the device: codes and loci byte for byte what the definition gives when it is applied site by
site (tests/pattern_enum_cases.py) - over the lengths and the PAM at either end and at both, full masks, the filters, the
targets under both rules, equal to vsc_guides_enumerate where the two definitions coincide, the round trip through
vsc_search_pattern, shards, the cap, repetition, what is refused, and pattern_search -E end to end."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import varscot_amd as va
from varscot_amd import _lib
import pattern_cases as pc
import pattern_enum_cases as ec
from helpers import make_genome, random_guides

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "varscot_amd", "bin")


@pytest.fixture(scope="module")
def ctx():
    c = va.Context(0)
    yield c
    c.close()


def same(got, want):
    """Codes and loci byte-equal to the restatement's."""
    codes, loci = ec.arrays(want)
    assert got.codes.dtype == np.uint64 and got.loci.dtype == va.LOCUS_DTYPE
    assert len(got) == len(codes) == len(got.loci)
    assert got.codes.tobytes() == codes.tobytes()
    assert got.loci.tobytes() == loci.tobytes()


def loaded(ctx, scenario):
    return ctx.load_genome(va.PackedGenome.from_sequences(scenario["contigs"]))


@pytest.fixture(scope="module")
def edge(ctx):
    e = dict(ec.edge_scenario(23, "3"))
    e["packed"] = va.PackedGenome.from_sequences(e["contigs"])
    e["gen"] = ctx.load_genome(e["packed"])
    yield e
    e["gen"].close()


# ---- 1. the edge layouts ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("place", pc.PLACES)
@pytest.mark.parametrize("L", [16, 20, 23, 27, 32])
def test_edge_layout_equals_the_definition(ctx, L, place):
    e = ec.edge_scenario(L, place)
    gen = loaded(ctx, e)
    try:
        got = gen.enumerate_pattern(e["pattern"], e["protospacer"])
        same(got, e["cands"])
        t = ctx.timing()
        assert t["sites"] == len(e["cands"]) and t["hits"] == 0 and t["pairs"] == 0
        assert t["scan_ms"] > 0 and t["total_ms"] == t["scan_ms"]
        assert t["sort_ms"] == 0 and t["finalize_ms"] == 0 and t["score_ms"] == 0 and t["prep_ms"] == 0 and t["sort_bytes"] == 0
        tiles = (va.PackedGenome.from_sequences(e["contigs"]).n_words + 63) // 64
        assert t["genome_bytes"] == 2 * tiles * 64 * 12  # both passes read every tile's three planes
    finally:
        gen.close()


# ---- 2. full masks ----------------------------------------------------------------------------------------------------------
def test_full_masks(ctx):
    e = ec.full_scenario()
    gen = loaded(ctx, e)
    try:
        same(gen.enumerate_pattern(e["pattern"], e["protospacer"]), e["cands"])
        for strands, s in (("+", 0), ("-", 1)):
            same(gen.enumerate_pattern(e["pattern"], e["protospacer"], strands=strands), [x for x in e["cands"] if x[2] == s])
    finally:
        gen.close()


# ---- 3. the filters ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["sa", "five"])
def filt(ctx, request):
    e = dict(ec.filter_scenario(request.param))
    e["gen"] = loaded(ctx, e)
    yield e
    e["gen"].close()


@pytest.mark.parametrize("kw", ec.FILTERS + (dict(max_t_run=2), dict(gc=(9, 12), max_t_run=3, strands=2)),
                         ids=lambda kw: ",".join("%s=%s" % kv for kv in kw.items()))
def test_filters_equal_the_definition(filt, kw):
    want = ec.kept(filt["cands"], filt["contigs"], filt["L"], filt["protospacer"], **kw)
    assert 0 < len(want) < len(filt["cands"])
    same(filt["gen"].enumerate_pattern(filt["pattern"], filt["protospacer"], **kw), want)


def test_a_run_of_t_ends_at_the_protospacer(filt):
    gen, args = filt["gen"], (filt["pattern"], filt["protospacer"])
    plain = gen.enumerate_pattern(*args)
    same(plain, filt["cands"])
    k = filt["protospacer"][1]
    wide = gen.enumerate_pattern(*args, gc=(0, k), max_t_run=k)  # bounds nothing can miss: the one-by-one path, same result
    assert wide.codes.tobytes() == plain.codes.tobytes() and wide.loci.tobytes() == plain.loci.tobytes()
    at = lambda got: {(int(l["contig"]), int(l["pos"]), int(l["strand"])) for l in got.loci}
    at3, at2 = at(gen.enumerate_pattern(*args, max_t_run=3)), at(gen.enumerate_pattern(*args, max_t_run=2))
    for strand in (0, 1):
        spot = (0, filt["where"][("edge", strand)], strand)
        assert spot in at3 and spot not in at2        # TTT beside a T of the PAM: a run of 3
        assert (0, filt["where"][("inner", strand)], strand) not in at3


# ---- 4. targets, both rules -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def targ(ctx):
    e = dict(ec.target_scenario())
    e["gen"] = loaded(ctx, e)
    yield e
    e["gen"].close()


@pytest.mark.parametrize("rule", ["overlap", "inside"])
def test_targets_equal_the_definition(ctx, targ, rule):
    gen, args = targ["gen"], (targ["pattern"], targ["protospacer"])
    want = ec.kept(targ["cands"], targ["contigs"], targ["L"], targ["protospacer"], targets=targ["targets"], rule=rule)
    assert 0 < len(want) < len(targ["cands"])
    same(gen.enumerate_pattern(*args, targets=targ["targets"], rule=rule), want)
    assert ctx.timing()["sites"] == len(want)
    # every interval on its own (the shapes one by one), and the filters behind the targets
    for iv in targ["targets"]:
        same(gen.enumerate_pattern(*args, targets=[iv], rule=rule),
             ec.kept(targ["cands"], targ["contigs"], targ["L"], targ["protospacer"], targets=[iv], rule=rule))
    kw = dict(targets=targ["targets"], rule=rule, gc=(8, 11), max_t_run=2, strands=2)
    filtered = ec.kept(targ["cands"], targ["contigs"], targ["L"], targ["protospacer"], **kw)
    assert 0 < len(filtered) < len(want)
    same(gen.enumerate_pattern(*args, **kw), filtered)
    # no target at all: a pointer that is not NULL with n == 0
    same(gen.enumerate_pattern(*args, targets=[], rule=rule), [])
    assert ctx.timing()["sites"] == 0 and ctx.timing()["genome_bytes"] == 0
    same(gen.enumerate_pattern(*args, targets=[(0, 300, 300)], rule=rule), [])


@pytest.mark.parametrize("rule", ["overlap", "inside"])
def test_only_the_tiles_that_meet_a_target_are_visited(ctx, targ, rule):
    gen, args = targ["gen"], (targ["pattern"], targ["protospacer"])
    want = ec.kept(targ["cands"], targ["contigs"], targ["L"], targ["protospacer"], targets=targ["last_tile"], rule=rule)
    assert want and all(p >= 3 * ec.TILE for _, p, _, _ in want)
    same(gen.enumerate_pattern(*args, targets=targ["last_tile"], rule=rule), want)
    tiles = (va.PackedGenome.from_sequences(targ["contigs"]).n_words + 63) // 64
    assert tiles >= 4 and ctx.timing()["genome_bytes"] == 2 * 1 * 64 * 12  # one tile of four, both passes
    across = [(0, ec.TILE - 12, ec.TILE + 12)]
    same(gen.enumerate_pattern(*args, targets=across, rule=rule),
         ec.kept(targ["cands"], targ["contigs"], targ["L"], targ["protospacer"], targets=across, rule=rule))
    assert ctx.timing()["genome_bytes"] == 2 * (2 if rule == "overlap" else 1) * 64 * 12  # inside: the starts end before the boundary


# ---- 5. the independent pin: vsc_guides_enumerate where the two definitions coincide ----------------------------------------
@pytest.fixture(scope="module")
def pin(ctx):
    guides = random_guides(np.random.default_rng(41), 8)
    contigs = make_genome(41, [14000, 5000, 40], guides, 4, n_plant=80, n_runs=3)
    packed = va.PackedGenome.from_sequences(contigs)
    gen = ctx.load_genome(packed)
    yield {"contigs": contigs, "packed": packed, "gen": gen}
    gen.close()


PIN = ("N" * 21 + "GG", (0, 20))


def equals_enumerate_guides(got, codes, loci):
    assert len(codes) > 0 and got.loci.tobytes() == loci.tobytes()
    assert [t[:23] for t in got.text(spell_pam=True)] == [g.upper() for g in va.unpack_guides(codes)]


@pytest.mark.parametrize("kw", [dict(), dict(gc=(8, 14)), dict(gc=(11, 0)), dict(max_t_run=3), dict(strands="+"), dict(strands="-"),
                                dict(gc=(7, 12), max_t_run=2, strands="-")], ids=lambda kw: ",".join("%s=%s" % kv for kv in kw.items()) or "plain")
def test_equals_enumerate_guides(pin, kw):
    codes, loci = pin["gen"].enumerate_guides(pam="GG", **kw)
    equals_enumerate_guides(pin["gen"].enumerate_pattern(*PIN, **kw), codes, loci)


@pytest.mark.parametrize("rule", ["overlap", "inside"])
def test_equals_enumerate_guides_in_regions(pin, rule):
    n0, n1 = len(pin["contigs"][0]), len(pin["contigs"][1])
    iv = [(0, 100, 400), (0, 300, 650), (0, 2000, 2100), (0, 2100, 2300), (0, 4090, 4100), (0, 0, 30), (0, n0 - 40, n0 + 50),
          (1, 1000, 3000), (1, 1500, 1600), (1, n1 - 23, n1), (2, 0, 40), (0, 7000, 7000)]
    regions = va.Regions(pin["packed"], iv, rule=rule)
    try:
        for kw in (dict(), dict(gc=(8, 14), max_t_run=3)):
            codes, loci = pin["gen"].enumerate_guides(regions, pam="GG", **kw)
            got = pin["gen"].enumerate_pattern(*PIN, targets=iv, rule=rule, **kw)
            equals_enumerate_guides(got, codes, loci)
            assert all(regions.contains(int(l["contig"]), int(l["pos"])) for l in got.loci)
    finally:
        regions.close()


# ---- 6. the round trip through the search -------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [(27, "3"), (20, "5"), (16, "both")])
def test_round_trip_through_search_pattern(ctx, which):
    e = ec.edge_scenario(*which)
    gen = loaded(ctx, e)
    try:
        targets = [(0, 0, 400), (0, ec.TILE - 60, ec.TILE + 60), (0, 5500, 5800), (4, 0, 100), (5, 0, 100)]
        found = gen.enumerate_pattern(e["pattern"], e["protospacer"], targets=targets)
        assert len(found) >= 8 and {int(s) for s in found.loci["strand"]} == {0, 1}
        for spell in (False, True):
            text = found.text(spell_pam=spell)
            assert all(len(t) == e["L"] and (spell or t.count("N") == e["L"] - e["protospacer"][1]) for t in text)
            rec, rows = gen.search_pattern(e["pattern"], text, 0)
            own = {(int(r["guide"]), int(r["contig"]), int(r["pos"]), int(r["info"]) >> 31) for r in rec if r["info"] & 63 == 0}
            for g, l in enumerate(found.loci):  # every candidate's locus is a record of its own guide with NM 0
                assert (g, int(l["contig"]), int(l["pos"]), int(l["strand"])) in own
        _, plain = gen.search_pattern(e["pattern"], found.text(), 2, records=False)
        again, rows = gen.design_pattern(e["pattern"], e["protospacer"], 2, targets=targets)
        assert again.codes.tobytes() == found.codes.tobytes() and again.loci.tobytes() == found.loci.tobytes()
        assert (plain[:, 0] >= 1).all() and np.array_equal(rows[:, 0], plain[:, 0] - 1) and np.array_equal(rows[:, 1:], plain[:, 1:])
        assert rows.dtype == np.uint32 and rows.shape == (len(found), 9)
    finally:
        gen.close()


# ---- 7. shards --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
def test_shards_concatenate_to_the_whole(ctx, edge, world):
    whole = edge["gen"].enumerate_pattern(edge["pattern"], edge["protospacer"])
    targets = [(0, 1900, 2200), (0, 4000, 4200), (2, 0, 100)]
    whole_t = edge["gen"].enumerate_pattern(edge["pattern"], edge["protospacer"], targets=targets, gc=(6, 0))
    assert len(whole_t) > 0
    parts, parts_t = [], []
    for rank in range(world):
        g = ctx.load_genome(edge["packed"], rank, world)
        parts.append(g.enumerate_pattern(edge["pattern"], edge["protospacer"]))
        parts_t.append(g.enumerate_pattern(edge["pattern"], edge["protospacer"], targets=targets, gc=(6, 0)))
        g.close()
    assert sum(len(p) > 0 for p in parts) >= 2
    for full, pieces in ((whole, parts), (whole_t, parts_t)):
        assert np.concatenate([p.codes for p in pieces]).tobytes() == full.codes.tobytes()
        assert np.concatenate([p.loci for p in pieces]).tobytes() == full.loci.tobytes()


# ---- 8. calls and refusals --------------------------------------------------------------------------------------------------
def test_the_cap_repetition_and_an_empty_result(ctx, edge):
    gen, args = edge["gen"], (edge["pattern"], edge["protospacer"])
    n = len(edge["cands"])
    first = gen.enumerate_pattern(*args, max_guides=n)
    same(first, edge["cands"])
    with pytest.raises(va.VarscotError) as err:
        gen.enumerate_pattern(*args, max_guides=n - 1)
    assert err.value.code == -34 and (" %d candidates" % n) in str(err.value)
    same(gen.enumerate_pattern(*args), edge["cands"])
    ctx.release_scratch()  # the pools come back on the next call
    same(gen.enumerate_pattern(*args), edge["cands"])
    same(gen.enumerate_pattern(*args, targets=[(0, 10, 300)], rule="inside"),
         ec.kept(edge["cands"], edge["contigs"], edge["L"], edge["protospacer"], targets=[(0, 10, 300)], rule="inside"))
    same(gen.enumerate_pattern(*args), edge["cands"])
    empty = gen.enumerate_pattern("N" * 20 + "GGG", (0, 20), gc=(20, 0), max_t_run=1, targets=[(3, 0, 22)])
    assert len(empty) == 0 and empty.codes.dtype == np.uint64 and empty.loci.dtype == va.LOCUS_DTYPE and empty.text() == []
    assert ctx.timing()["sites"] == 0
    # the handle's own accessors on an empty result
    L, h = va.lib(), C.c_void_p()
    p = va.PatternEnumParams(0, 20)
    iv = np.zeros(1, dtype=va.INTERVAL_DTYPE)
    assert L.vsc_guides_enumerate_pattern(ctx._h, gen._h, b"N" * 23, 23, C.byref(p), _lib.ptr(iv), 0, C.byref(h)) == 0
    a, b = C.c_void_p(1), C.c_void_p(1)
    assert L.vsc_pattern_guides_count(h) == 0 and L.vsc_pattern_guides_data_dev(h, C.byref(a), C.byref(b)) == 0 and not a.value and not b.value
    assert L.vsc_pattern_guides_data(h, C.byref(a), C.byref(b)) == 0 and L.vsc_pattern_guides_free(h) == 0
    assert L.vsc_pattern_guides_free(None) == 0 and L.vsc_pattern_guides_count(None) == 0
    # ... and on one that is not: the device arrays hold what the host copies hold
    assert L.vsc_guides_enumerate_pattern(ctx._h, gen._h, edge["pattern"].encode(), 23, C.byref(p), None, 0, C.byref(h)) == 0
    assert L.vsc_pattern_guides_count(h) == n and L.vsc_pattern_guides_data_dev(h, C.byref(a), C.byref(b)) == 0 and a.value and b.value
    assert b.value - a.value == (8 * n + 255) // 256 * 256
    assert L.vsc_pattern_guides_data(h, C.byref(a), None) == 0 and L.vsc_pattern_guides_data(h, None, C.byref(b)) == 0
    assert C.string_at(a.value, 8 * n) == first.codes.tobytes() and C.string_at(b.value, 16 * n) == first.loci.tobytes()
    assert L.vsc_pattern_guides_free(h) == 0


def test_parameter_validation(ctx, edge):
    gen, pattern = edge["gen"], edge["pattern"]
    refused = lambda *a, **kw: pytest.raises(va.VarscotError, gen.enumerate_pattern, *a, **kw)
    for args, kw in (((("N" * 15), (0, 15)), {}), (("N" * 33, (0, 20)), {}), (("N" * 20 + "UGG", (0, 20)), {}),
                     ((pattern, (0, 0)), {}), ((pattern, (4, 20)), {}), ((pattern, (23, 1)), {}),
                     ((pattern, (0, 20)), dict(strands=3)), ((pattern, (0, 20)), dict(gc=(21, 0))), ((pattern, (0, 20)), dict(gc=(0, 21))),
                     ((pattern, (0, 20)), dict(gc=(12, 8))), ((pattern, (2, 10)), dict(gc=(11, 0))),
                     ((pattern, (0, 20)), dict(targets=[(7, 0, 10)])), ((pattern, (0, 20)), dict(targets=[(0, 11, 10)])),
                     ((pattern, (0, 20)), dict(targets=[(0, 0, 10)], params=va.PatternEnumParams(0, 20, rule=2)))):
        err = refused(*args, **kw)
        assert err.value.code == -22 and "vsc_guides_enumerate_pattern" in str(err.value), (args, kw)
    iv = np.zeros(1, dtype=va.INTERVAL_DTYPE)
    iv[0] = (0, 0, 100, 1)
    assert refused(pattern, (0, 20), targets=iv).value.code == -22  # a reserved field of an interval
    L, h = va.lib(), C.c_void_p(1)
    call = lambda p, targets=None, n=0, genome=gen._h, out=C.byref(h), text=pattern.encode(), params=True: \
        L.vsc_guides_enumerate_pattern(ctx._h, genome, text, 23, C.byref(p) if params else None, targets, n, out)
    good = va.PatternEnumParams(0, 20)
    for field in ("reserved0", "reserved1"):
        p = va.PatternEnumParams(0, 20)
        setattr(p, field, 1)
        assert call(p) == -22 and not h.value
    for k in (0, 1):
        p = va.PatternEnumParams(0, 20)
        p.reserved[k] = 1
        assert call(p) == -22
    assert call(good, None, 3) == -22                                   # intervals announced, none given
    assert call(good, genome=None) == -22 and call(good, text=None) == -22 and call(good, params=False) == -22 and call(good, out=None) == -22
    other = va.Context(0)
    try:
        assert L.vsc_guides_enumerate_pattern(other._h, gen._h, pattern.encode(), 23, C.byref(good), None, 0, C.byref(h)) == -22
    finally:
        other.close()
    p = va.PatternEnumParams(0, 20)
    p.rule = 7                                                          # the rule is not looked at without targets
    assert call(p) == 0 and L.vsc_pattern_guides_count(h) == len(edge["cands"]) and L.vsc_pattern_guides_free(h) == 0


# ---- 9. pattern_search -E end to end ------------------------------------------------------------------------------------------
def test_pattern_search_enumerates(tmp_path, edge):
    names = ["c%d" % i for i in range(len(edge["contigs"]))]
    with open(tmp_path / "g.fa", "w") as f:
        for n, s in zip(names, edge["contigs"]):
            f.write(">%s some text\n%s\n" % (n, s))
    targets = [(0, 1900, 2300), (0, 5500, 5800), (4, 0, 100)]
    with open(tmp_path / "t.bed", "w") as f:
        f.write("# targets\n" + "".join("%s\t%d\t%d\tname\n" % (names[c], a, b) for c, a, b in targets))
    (tmp_path / "none.bed").write_text("# nothing\n")
    run = lambda *a: subprocess.run([os.path.join(BIN, a[0])] + list(a[1:]), capture_output=True, text=True, timeout=600)
    assert run("bidir_index", "-G", str(tmp_path / "g.fa"), "-I", str(tmp_path / "idx")).returncode == 0
    base = ("pattern_search", "-i", str(tmp_path / "idx"), "-q", edge["pattern"], "-p", "%d,%d" % edge["protospacer"])
    listed = lambda found: [[t, names[int(l["contig"])], str(int(l["pos"])), "+-"[int(l["strand"])]] for t, l in zip(found.text(), found.loci)]
    read = lambda name: [l.rstrip("\n").split("\t") for l in open(tmp_path / name)]
    # the whole genome
    r = run(*base, "-E", str(tmp_path / "all.tsv"))
    assert r.returncode == 0, r.stderr
    whole = edge["gen"].enumerate_pattern(edge["pattern"], edge["protospacer"])
    lines = read("all.tsv")
    assert lines[0] == ["#guide", "chrom", "pos", "strand"] and lines[1:] == listed(whole) and len(lines) > 50
    # targets, filters and the screen in one run
    kw = dict(targets=targets, rule="inside", gc=(6, 15), max_t_run=3)
    r = run(*base, "-E", str(tmp_path / "in.tsv"), "-B", str(tmp_path / "t.bed"), "-r", "inside", "-g", "6,15", "-t", "3", "-M", "2",
            "-O", str(tmp_path / "sum.tsv"))
    assert r.returncode == 0, r.stderr
    found, rows = edge["gen"].design_pattern(edge["pattern"], edge["protospacer"], 2, **kw)
    assert 0 < len(found) < len(whole) and read("in.tsv")[1:] == listed(found)
    lines = read("sum.tsv")
    assert lines[0] == ["#guideId", "guideSeq", "offtargetCount", "mm0", "mm1", "mm2"]
    for g, (row, (text, chrom, pos, strand)) in enumerate(zip(lines[1:], listed(found))):
        counts = [int(x) for x in rows[g, :3]]
        assert row == ["%s:%s:%s" % (chrom, pos, strand), text, str(sum(counts))] + [str(x) for x in counts]
    assert len(lines) == 1 + len(found)
    r = run(*base, "-E", str(tmp_path / "minus.tsv"), "-B", str(tmp_path / "t.bed"), "-s", "-")
    assert r.returncode == 0, r.stderr
    assert read("minus.tsv")[1:] == listed(edge["gen"].enumerate_pattern(edge["pattern"], edge["protospacer"], targets=targets, strands="-"))
    r = run(*base, "-E", str(tmp_path / "none.tsv"), "-B", str(tmp_path / "none.bed"))  # a target set that holds nothing
    assert r.returncode == 0 and read("none.tsv") == [["#guide", "chrom", "pos", "strand"]]
