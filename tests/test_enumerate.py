"""vsc_guides_enumerate / vsc_multi_guides_enumerate on the device: the candidate guides of a genome, a shard or an annotation,
byte for byte what the definition gives when it is applied window by window (tests/enumerate_cases.py) - codes, loci and order -
through the filters, the regions, shards, several contexts, the searches that take the result, and guide_summary -E."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import varscot_amd as va
from varscot_amd import _lib
import enumerate_cases as ec
import regions_cases as rc
from helpers import random_seq

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
    contigs = ec.edge_layout()
    return {"contigs": contigs, "packed": va.PackedGenome.from_sequences(contigs)}


@pytest.fixture(scope="module")
def edge_gen(ctx, edge):
    g = ctx.load_genome(edge["packed"])
    yield g
    g.close()


def same(got, want_cands):
    """Codes and loci byte-equal to the brute force's."""
    codes, loci = ec.arrays(want_cands)
    assert got[0].dtype == np.uint64 and got[1].dtype == va.LOCUS_DTYPE
    assert len(got[0]) == len(codes) and len(got[1]) == len(loci)
    assert got[0].tobytes() == codes.tobytes()
    assert got[1].tobytes() == loci.tobytes()


# ---- 1. edge layout, no regions -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pam,strands", [("GG", "both"), ("GG", "+"), ("GG", "-"), ("GA", "both"), ("AG", "both")])
def test_edge_layout_equals_brute_force(ctx, edge, edge_gen, pam, strands):
    want = ec.brute_force(edge["contigs"], pam=pam, strands=strands)
    # the layout's own count, both strands, exceeds three tiles; one strand of it still has a homopolymer contig of
    # 4 178 starts, which fills two tiles and carries the scan over both of their ends
    floor = {"both": 3 * ec.TILE, "+": 2 * ec.TILE, "-": 2 * ec.TILE}[strands] if pam == "GG" else 100
    assert len(want) > floor
    got = edge_gen.enumerate_guides(pam=pam, strands=strands)
    same(got, want)
    t = ctx.timing()
    assert t["sites"] == len(want) and t["hits"] == 0 and t["sort_ms"] == 0 and t["score_ms"] == 0 and t["finalize_ms"] == 0
    assert t["scan_ms"] > 0 and t["total_ms"] == t["scan_ms"]
    tiles = (edge["packed"].n_words + 63) // 64
    assert t["genome_bytes"] == 2 * tiles * 64 * 12  # both passes read every tile's three planes
    again = edge_gen.enumerate_guides(pam=pam, strands=strands)
    assert again[0].tobytes() == got[0].tobytes() and again[1].tobytes() == got[1].tobytes()


def test_lower_case_pam_is_the_same_pam(edge, edge_gen):
    same(edge_gen.enumerate_guides(pam="gg"), ec.brute_force(edge["contigs"]))


# ---- 2. filters on the random contig --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rand_gen(ctx, edge):
    contigs = [edge["contigs"][ec.RANDOM_AT]]
    g = ctx.load_genome(va.PackedGenome.from_sequences(contigs))
    yield contigs, g
    g.close()


@pytest.mark.parametrize("kw", [dict(gc=(8, 14)), dict(gc=(12, 0)), dict(gc=(0, 9)), dict(max_t_run=3), dict(max_t_run=1),
                                dict(gc=(8, 14), max_t_run=3, strands="-"), dict(gc=(9, 13), max_t_run=2, pam="GA")])
def test_filters_equal_brute_force(rand_gen, kw):
    contigs, gen = rand_gen
    base = dict(kw)
    base.pop("gc", None)
    base.pop("max_t_run", None)
    everything = ec.brute_force(contigs, **base)
    want = ec.brute_force(contigs, **kw)
    assert 0 < len(want) < len(everything)  # the case both keeps and drops
    same(gen.enumerate_guides(**kw), want)


def test_no_filter_and_the_t_run_at_the_pam(rand_gen):
    contigs, gen = rand_gen
    plain = gen.enumerate_guides()
    same(plain, ec.brute_force(contigs))
    zero = gen.enumerate_guides(gc=(0, 0), max_t_run=0)
    assert zero[0].tobytes() == plain[0].tobytes() and zero[1].tobytes() == plain[1].tobytes()
    wide = gen.enumerate_guides(gc=(0, 20), max_t_run=20)  # bounds nothing can miss: the one-by-one path, same result
    assert wide[0].tobytes() == plain[0].tobytes() and wide[1].tobytes() == plain[1].tobytes()
    codes, loci = gen.enumerate_guides(max_t_run=3)
    found = {(int(l["pos"]), int(l["strand"])): g for l, g in zip(loci, va.unpack_guides(codes))}
    for pos, guide, strand in ec.PLANTS:
        key = (pos, 0 if strand == "+" else 1)
        if guide == ec.T_INSIDE:
            assert key not in found           # TTTT inside the protospacer, either strand
        else:
            assert found[key] == ec.T_AT_PAM  # three T in the protospacer + the N of NGG: not filtered


# ---- 3. regions -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def three(ctx):
    rng = np.random.default_rng(77)
    contigs = [random_seq(rng, n) for n in rc.LENS]
    packed = va.PackedGenome.from_sequences(contigs)
    g = ctx.load_genome(packed)
    yield {"contigs": contigs, "packed": packed, "gen": g, "member": rc.brute_force(rc.annotation())}
    g.close()


@pytest.mark.parametrize("rule", ["overlap", "inside"])
def test_regions_equal_brute_force(ctx, three, rule):
    reg = va.Regions(three["packed"], rc.annotation(), rule=rule)
    info = reg.info()
    assert info["blocks_out"] > 0 and info["blocks_in"] > 0 and info["blocks_mixed"] > 0
    want = ec.brute_force(three["contigs"], member=three["member"][rule])
    everything = ec.brute_force(three["contigs"])
    assert 0 < len(want) < len(everything) and {x[2] for x in want} == {0, 1}
    same(three["gen"].enumerate_guides(reg), want)
    assert ctx.timing()["sites"] == len(want)
    kw = dict(gc=(8, 14), max_t_run=3, pam="GA")
    want = ec.brute_force(three["contigs"], member=three["member"][rule], **kw)
    assert want
    same(three["gen"].enumerate_guides(reg, **kw), want)
    reg.close()


def test_empty_and_foreign_regions(ctx, three):
    empty = va.Regions(three["packed"], [])
    codes, loci = three["gen"].enumerate_guides(empty)
    assert len(codes) == 0 and len(loci) == 0 and ctx.timing()["sites"] == 0
    other = va.Regions(va.PackedGenome.from_sequences(["A" * 100, "C" * 50, "G" * 40]), [(0, 1, 50)])
    with pytest.raises(va.VarscotError) as e:
        three["gen"].enumerate_guides(other)
    assert e.value.code == -22


def test_work_list_visits_the_annotated_tiles_only(ctx):
    rng = np.random.default_rng(78)
    seq = random_seq(rng, 1_000_000)
    packed = va.PackedGenome.from_sequences([seq])
    gen = ctx.load_genome(packed)
    everything = gen.enumerate_guides()
    all_bytes = ctx.timing()["genome_bytes"]
    reg = va.Regions(packed, [(0, 500_000, 500_200)], rule="overlap")
    got = gen.enumerate_guides(reg)
    some_bytes = ctx.timing()["genome_bytes"]
    # 222 window starts lie in at most two tiles of 2 048; the genome has 489: far below a tenth
    assert 0 < some_bytes < all_bytes / 10
    keep = (everything[1]["pos"] >= 500_000 - 22) & (everything[1]["pos"] < 500_200)
    assert keep.sum() > 0
    assert got[0].tobytes() == everything[0][keep].tobytes() and got[1].tobytes() == everything[1][keep].tobytes()
    gen.close()


# ---- 4. shards and devices ------------------------------------------------------------------------------------------------
EDGE_INTERVALS = [(0, 100, 300), (0, 2000, 2100), (0, 4000, 4200), (1, 0, 4200), (2, 0, 23), (5, 1000, 9500), (6, 0, 40),
                  (5, 13990, 14000)]


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("rule", [None, "overlap", "inside"])
def test_shards_concatenate_to_the_whole_genome(ctx, edge, edge_gen, world, rule):
    reg = va.Regions(edge["packed"], EDGE_INTERVALS, rule=rule) if rule else None
    member = rc.brute_force(EDGE_INTERVALS, [len(c) for c in edge["contigs"]])[rule] if rule else None
    whole = edge_gen.enumerate_guides(reg)
    same(whole, ec.brute_force(edge["contigs"], member=member))
    parts = []
    for rank in range(world):
        g = ctx.load_genome(edge["packed"], rank, world)
        parts.append(g.enumerate_guides(reg))
        g.close()
    assert sum(len(p[0]) > 0 for p in parts) >= 2
    assert np.concatenate([p[0] for p in parts]).tobytes() == whole[0].tobytes()
    assert np.concatenate([p[1] for p in parts]).tobytes() == whole[1].tobytes()


def test_multi_context_gives_the_same_bytes(edge, edge_gen):
    reg = va.Regions(edge["packed"], EDGE_INTERVALS, rule="inside")
    m = va.MultiContext([0, 0, 0])
    try:
        g = m.load_genome(edge["packed"])
        for r, kw in ((None, {}), (reg, {}), (None, dict(gc=(8, 14), max_t_run=3, strands="-"))):
            one = edge_gen.enumerate_guides(r, **kw)
            got = g.enumerate_guides(r, **kw)
            assert len(one[0]) > 0
            assert got[0].tobytes() == one[0].tobytes() and got[1].tobytes() == one[1].tobytes()
        n = len(edge_gen.enumerate_guides()[0])
        assert n == len(ec.brute_force(edge["contigs"]))
        with pytest.raises(va.VarscotError) as e:
            g.enumerate_guides(max_guides=n - 1)
        assert e.value.code == -34 and str(n) in str(e.value)
        assert len(g.enumerate_guides(max_guides=n)[0]) == n
    finally:
        m.close()


def test_device_pointers_of_a_single_context_result(ctx, edge, edge_gen):
    L = va.lib()
    empty = va.Regions(edge["packed"], [])
    for regions, some in ((None, True), (empty._h, False)):
        p = _lib.EnumParams()
        p.pam = b"GG"
        h = C.c_void_p()
        _lib.check(L.vsc_guides_enumerate(ctx._h, edge_gen._h, regions, C.byref(p), C.byref(h)), ctx._h)
        pc, pl = C.c_void_p(), C.c_void_p()
        assert L.vsc_guides_data_dev(h, C.byref(pc), C.byref(pl)) == 0
        n = int(L.vsc_guides_count(h))
        if some:
            assert n > 0 and pc.value and pl.value and pc.value != pl.value
        else:
            assert n == 0 and not pc.value and not pl.value
        assert L.vsc_guides_free(h) == 0


# ---- 5. round trip: the result is what the searches take ---------------------------------------------------------------------
def test_round_trip_through_search_and_summary(ctx):
    rng = np.random.default_rng(79)
    contigs = [random_seq(rng, 40_000), random_seq(rng, 20_000)]
    packed = va.PackedGenome.from_sequences(contigs)
    gen = ctx.load_genome(packed)
    iv = [(0, 1000, 1600), (0, 30_000, 30_400), (1, 5000, 5500)]  # caps the guides at a couple of hundred
    reg = va.Regions(packed, iv, rule="inside")
    codes, loci = gen.enumerate_guides(reg)
    same((codes, loci), ec.brute_force(contigs, member=rc.brute_force(iv, [40_000, 20_000])["inside"]))
    assert 50 < len(codes) < 400 and set(loci["strand"].tolist()) == {0, 1}
    hits = gen.search(codes, 0)
    rec = hits.to_numpy()
    hits.close()
    own = set(zip(rec["guide"].tolist(), rec["contig"].tolist(), rec["pos"].tolist(), (rec["info"] >> 31).tolist()))
    for i, l in enumerate(loci):
        assert (i, int(l["contig"]), int(l["pos"]), int(l["strand"])) in own, i
    rows = gen.summarize(codes, 3, exclude=loci)
    assert (rows["on_target"] == 1).all()
    strings = va.unpack_guides(codes)
    assert all(len(s) == 23 and s.endswith("GG") for s in strings)
    assert gen.summarize(strings, 3, exclude=loci).tobytes() == rows.tobytes()
    d_codes, d_loci, d_rows = gen.design(reg, 3)
    assert d_codes.tobytes() == codes.tobytes() and d_loci.tobytes() == loci.tobytes() and d_rows.tobytes() == rows.tobytes()
    gen.close()


# ---- 6. validation ----------------------------------------------------------------------------------------------------------
def test_validation(ctx, edge, edge_gen):
    def raises(code, **kw):
        with pytest.raises(va.VarscotError) as e:
            edge_gen.enumerate_guides(**kw)
        assert e.value.code == code, kw
        return str(e.value)

    raises(-22, pam="NG")
    raises(-22, pam="GX")
    raises(-22, strands=3)
    raises(-22, gc=(0, 21))
    raises(-22, gc=(21, 0))
    raises(-22, gc=(9, 8))
    for field, value in (("reserved0", 1), ("reserved", (1, 0)), ("reserved", (0, 1))):
        p = _lib.EnumParams()
        p.pam = b"GG"
        setattr(p, field, (C.c_uint32 * 2)(*value) if field == "reserved" else value)
        raises(-22, params=p)
    h = C.c_void_p()
    assert va.lib().vsc_guides_enumerate(ctx._h, edge_gen._h, None, None, C.byref(h)) == -22 and not h.value
    assert len(edge_gen.enumerate_guides(gc=(9, 0))[0]) > 0  # gc_min above a gc_max of 0 is no contradiction: no upper bound
    n = len(ec.brute_force(edge["contigs"]))
    text = raises(-34, max_guides=n - 1)
    assert str(n) in text
    assert len(edge_gen.enumerate_guides(max_guides=n)[0]) == n
    with pytest.raises(ValueError):
        edge_gen.enumerate_guides(pam="G")
    with pytest.raises(ValueError):
        edge_gen.enumerate_guides(strands="plus")


def test_scratch_goes_back_to_the_device(edge):
    own = va.Context(0)
    gen = own.load_genome(edge["packed"])
    first = gen.enumerate_guides()
    own.release_scratch()
    again = gen.enumerate_guides()
    assert again[0].tobytes() == first[0].tobytes() and again[1].tobytes() == first[1].tobytes()
    own.close()


# ---- 7. the tool ------------------------------------------------------------------------------------------------------------
def test_guide_summary_discovers_its_guides(tmp_path):
    rng = np.random.default_rng(80)
    contigs = [random_seq(rng, 15000), random_seq(rng, 6000)]
    names = ["chr1 assembled", "chr2"]
    with open(tmp_path / "g.fa", "w") as f:
        for n, s in zip(names, contigs):
            f.write(">%s\n%s\n" % (n, "\n".join(s[i:i + 60] for i in range(0, len(s), 60))))
    iv = [(0, 500, 1300), (1, 100, 400), (0, 14900, 15000)]
    (tmp_path / "t.bed").write_text("".join("%s\t%d\t%d\tx\n" % (names[c].split()[0], a, b) for c, a, b in iv))
    run = lambda *a: subprocess.run([os.path.join(BIN, a[0])] + list(a[1:]), capture_output=True, text=True, timeout=600)
    assert run("bidir_index", "-G", str(tmp_path / "g.fa"), "-I", str(tmp_path / "idx")).returncode == 0
    base = ["guide_summary", "-G", str(tmp_path / "g.fa"), "-I", str(tmp_path / "idx"), "-M", "3"]
    want = ec.brute_force(contigs, member=rc.brute_force(iv, [15000, 6000])["inside"])
    assert 50 < len(want) < 400
    ids = ["%s:%d:%s" % (names[c].split()[0], p, "+-"[s]) for c, p, s, _ in want]
    r = run(*base, "-E", str(tmp_path / "t.bed"), "-L", str(tmp_path / "out.bed"), "-O", str(tmp_path / "e.tsv"))
    assert r.returncode == 0, r.stderr
    lines = (tmp_path / "e.tsv").read_text().splitlines()
    assert lines[0].startswith("#guideId\tguideSeq\tmitSpecScore\tofftargetCount\tonTargetFound")
    cols = [ln.split("\t") for ln in lines[1:]]
    assert [c[0] for c in cols] == ids and [c[1] for c in cols] == [g for _, _, _, g in want]
    assert all(c[4] == "1" for c in cols)
    bed = (tmp_path / "out.bed").read_text()
    assert bed == "".join("%s\t%d\t%d\t%s\t0\t%s\n" % (names[c].split()[0], p, p + 23, i, "+-"[s]) for (c, p, s, _), i in zip(want, ids))
    r = run(*base, "-B", str(tmp_path / "out.bed"), "-O", str(tmp_path / "b.tsv"))
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "b.tsv").read_bytes() == (tmp_path / "e.tsv").read_bytes()
    r = run(*base, "-E", str(tmp_path / "t.bed"), "-L", str(tmp_path / "out2.bed"), "-O", str(tmp_path / "e2.tsv"), "-D", "0,0")
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "e2.tsv").read_bytes() == (tmp_path / "e.tsv").read_bytes()
    assert (tmp_path / "out2.bed").read_bytes() == (tmp_path / "out.bed").read_bytes()
    # the filters and the other rule reach the device
    r = run(*base, "-E", str(tmp_path / "t.bed"), "-e", "overlap", "-g", "8,14", "-t", "3", "-s", "-", "-O", str(tmp_path / "f.tsv"))
    assert r.returncode == 0, r.stderr
    want = ec.brute_force(contigs, member=rc.brute_force(iv, [15000, 6000])["overlap"], gc=(8, 14), max_t_run=3, strands="-")
    assert want
    got = [ln.split("\t")[:2] for ln in (tmp_path / "f.tsv").read_text().splitlines()[1:]]
    assert got == [["%s:%d:-" % (names[c].split()[0], p), g] for c, p, _, g in want]
