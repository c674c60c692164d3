"""The on-target efficiency score on the device (vsc_loci_efficiency, vsc_guides_efficiency, vsc_pattern_guides_efficiency and
the two filters): bit for bit what the definition gives when it is applied locus by locus in plain Python
(tests/efficiency_cases.py) - additions only, in a fixed order, so there is no tolerance; scores are compared as uint64 views,
the undefined NaN included."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import efficiency_cases as ec
import varscot_amd as va
from helpers import random_seq, revcomp
from varscot_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "varscot_amd", "bin")
FILTER_TILE = 1024  # candidates per wave of the filter's passes (include/varscot_hip.h)
NEG_INF, POS_INF = float("-inf"), float("inf")


@pytest.fixture(scope="module")
def ctx():
    c = va.Context(0)
    yield c
    c.close()


def u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- handles: the calls that take a vsc_guides, on candidates of the test's own -------------------------------------------
class Guides:
    """A vsc_guides (or, pattern=True, a vsc_pattern_guides) handle and its calls."""

    def __init__(self, ctx, handle, pattern=False):
        self.ctx, self.h, self.pattern = ctx, handle, pattern
        L = va.lib()
        kind = "vsc_pattern_guides" if pattern else "vsc_guides"
        self.fn = {k: getattr(L, "%s_%s" % (kind, k)) for k in ("count", "data", "free", "efficiency", "filter_efficiency")}

    @classmethod
    def from_arrays(cls, ctx, codes, loci, on_device=True):
        h = C.c_void_p()
        _lib.check(va.lib().vsc_debug_guides_from_host(ctx._h if on_device else None, _lib.ptr(codes), _lib.ptr(loci), len(codes), C.byref(h)),
                   ctx._h)
        return cls(ctx, h)

    def __len__(self):
        return int(self.fn["count"](self.h))

    def arrays(self):
        pc, pl = C.c_void_p(), C.c_void_p()
        _lib.check(self.fn["data"](self.h, C.byref(pc), C.byref(pl)), self.ctx._h)
        n = len(self)
        if n == 0:
            return np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=va.LOCUS_DTYPE)
        return (np.frombuffer((C.c_char * (n * 8)).from_address(pc.value), dtype=np.uint64).copy(),
                np.frombuffer((C.c_char * (n * 16)).from_address(pl.value), dtype=va.LOCUS_DTYPE).copy())

    def efficiency(self, gen, model):
        linear, st = np.empty(len(self), dtype=np.float64), _lib.EffStats()
        _lib.check(self.fn["efficiency"](self.ctx._h, gen._h, self.h, model._h, _lib.ptr(linear), C.byref(st)), self.ctx._h)
        return linear, st.as_dict()

    def filter_code(self, gen, model, floor):
        out = C.c_void_p()
        return self.fn["filter_efficiency"](self.ctx._h, gen._h, self.h, model._h, floor, C.byref(out)), out

    def filter(self, gen, model, floor):
        code, out = self.filter_code(gen, model, floor)
        _lib.check(code, self.ctx._h)
        return Guides(self.ctx, out, self.pattern)

    def close(self):
        if self.h:
            self.fn["free"](self.h)
            self.h = None


# ---- 1. exhaustive small genome ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(ctx):
    """Per shape: the small genome resident, every locus of it, and - per family, computed once - the expected bits and stats."""
    cache = {}

    def get(shape):
        if shape not in cache:
            contigs = ec.small_genome(shape)
            loci = ec.every_locus(contigs, shape[1])
            cache[shape] = {"contigs": contigs, "gen": ctx.load_genome(va.PackedGenome.from_sequences(list(contigs))), "loci": loci,
                            "arr": ec.locus_array(loci), "want": {}}
        return cache[shape]

    def want(shape, family):
        s = get(shape)
        if family not in s["want"]:
            s["want"][family] = ec.expected(s["contigs"], s["loci"], shape, ec.arrays(family, shape))
        return s["want"][family]

    get.want = want
    yield get
    for s in cache.values():
        s["gen"].close()


@pytest.mark.parametrize("shape", ec.SHAPES, ids=lambda s: "%d-%d-%d" % s)
@pytest.mark.parametrize("family", ec.FAMILIES)
def test_every_locus_of_a_small_genome(small, family, shape):
    s = small(shape)
    want, want_stats = small.want(shape, family)
    assert want_stats["defined"] > 100 and want_stats["has_n"] > 0 and want_stats["invalid"] == 0
    assert (want_stats["off_contig"] > 0) == (shape[0] + shape[2] > 0)
    got, stats = s["gen"].efficiency(s["arr"], ec.build(family, shape))
    assert stats == want_stats and sum(stats.values()) == len(s["loci"])
    assert u64(got).tobytes() == want.tobytes()


# ---- 2. invalid loci -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(4, 23, 3), (16, 32, 16)], ids=lambda s: "%d-%d-%d" % s)
def test_invalid_loci_are_classed_and_never_followed(small, shape):
    s = small(shape)
    n_contigs, site_len = len(s["contigs"]), shape[1]
    bad = [(n_contigs, 0, 0), (0xFFFFFFFF, 0, 0), (0xFFFFFFFF, 0xFFFFFFFF, 1), (4, 10, 2), (4, 10, 0xFFFFFFFF), (4, 200 - site_len + 1, 0),
           (4, 200 - site_len + 1, 1), (4, 0xFFFFFFFF, 0), (5, 0xFFFFFFFF, 1), (3, 0, 0), (4, 0xFFFFFFFF - site_len + 1, 0)]
    good = (4, 120, 0)
    loci = bad + [good]
    want, want_stats = ec.expected(s["contigs"], loci, shape, ec.arrays("dense", shape))
    assert want_stats["invalid"] == len(bad) and want_stats["defined"] == 1
    got, stats = s["gen"].efficiency(ec.locus_array(loci), ec.build("dense", shape))
    assert stats == want_stats
    assert u64(got).tobytes() == want.tobytes() and (u64(got)[:-1] == ec.UNDEF).all()


def test_nothing_to_score(ctx, small):
    s = small((4, 23, 3))
    got, stats = s["gen"].efficiency(ec.locus_array([]), ec.build("dense", (4, 23, 3)))
    assert len(got) == 0 and stats == dict.fromkeys(ec.CLASSES, 0)
    t = ctx.timing()
    assert t["sites"] == 0 and t["score_ms"] == 0 and t["total_ms"] == 0 and t["genome_bytes"] == 0


# ---- 3. more candidates than one launch has lanes, more tiles than it has waves --------------------------------------------
def test_more_candidates_than_a_launch_has_lanes(small):
    shape = (6, 23, 6)
    s = small(shape)
    want, want_stats = small.want(shape, "mixed")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n, m = cus * 8 * 256 + 77, len(s["loci"])
    assert n > 3 * m  # every lane meets more than one tiling of the loci
    idx = np.arange(n) % m
    got, stats = s["gen"].efficiency(s["arr"][idx], ec.build("mixed", shape))
    assert u64(got).tobytes() == want[idx].tobytes()
    per = {k: int(v) for k, v in zip(*np.unique(np.array([ec.classify(s["contigs"], l, shape)[0] for l in s["loci"]])[idx], return_counts=True))}
    assert stats == {k: per.get(k, 0) for k in ec.CLASSES} and sum(stats.values()) == n


def test_filter_over_more_tiles_than_a_launch_has_waves(ctx, small):
    shape = (6, 23, 6)
    s = small(shape)
    want, _ = small.want(shape, "dense")
    model = ec.build("dense", shape)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    m = len(s["loci"])
    n = (cus * 8 * 4 + 3) * FILTER_TILE + 77  # the last tile is a partial one
    idx = np.arange(n) % m
    defined = want != ec.UNDEF
    floor = float(np.median(want[defined].view(np.float64)))
    keep = defined & (np.where(defined, want.view(np.float64), 0.0) >= floor)
    assert 0 < keep.sum() < defined.sum()
    codes = np.arange(n, dtype=np.uint64) * np.uint64(3)  # (the filter copies codes, it does not read them)
    g = Guides.from_arrays(ctx, codes, s["arr"][idx])
    out = g.filter(s["gen"], model, floor)
    got_codes, got_loci = out.arrays()
    chosen = np.nonzero(keep[idx])[0]
    assert len(got_codes) == len(chosen)
    assert got_codes.tobytes() == codes[chosen].tobytes() and got_loci.tobytes() == s["arr"][idx][chosen].tobytes()
    t = ctx.timing()
    assert t["sites"] == n and t["genome_bytes"] == 32 * n + 48 * len(chosen) and t["score_ms"] == t["total_ms"] > 0
    out.close()
    g.close()


# ---- 4. device-resident candidates --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted(ctx):
    """A 20 kb random genome with NGG sites (and CCN sites, their '-' form) at and next to the contig ends."""
    rng = np.random.default_rng(77)
    contigs = []
    for n in (12000, 5000, 3000):
        t = list(random_seq(rng, n))
        for p in (0, 2, 5, n - 23, n - 25, n - 29):
            site = random_seq(rng, 21) + "GG"
            t[p:p + 23] = site if p % 2 else revcomp(site)
        for p in (0, n - 23):
            t[p + 21:p + 23] = "GG"
            t[p:p + 2] = "CC"
        contigs.append("".join(t))
    packed = va.PackedGenome.from_sequences(contigs)
    gen = ctx.load_genome(packed)
    yield {"contigs": contigs, "packed": packed, "gen": gen}
    gen.close()


def loci_tuples(loci):
    return [(int(c), int(p), int(s)) for c, p, s in zip(loci["contig"], loci["pos"], loci["strand"])]


@pytest.mark.parametrize("family", ["dense", "mixed"])
def test_enumerated_guides_are_scored_where_they_lie(planted, family):
    shape = (6, 23, 6)
    gen, model = planted["gen"], ec.build(family, shape)
    plain = gen.enumerate_guides()
    codes, loci, linear = gen.enumerate_guides(efficiency=model)
    assert codes.tobytes() == plain[0].tobytes() and loci.tobytes() == plain[1].tobytes() and len(codes) > 1000
    want, want_stats = ec.expected(planted["contigs"], loci_tuples(loci), shape, ec.arrays(family, shape))
    assert want_stats["off_contig"] >= 6 and want_stats["defined"] > 1000  # the planted sites next to the ends have no context
    assert u64(linear).tobytes() == want.tobytes()
    by_loci, stats = gen.efficiency(loci, model)
    assert u64(by_loci).tobytes() == want.tobytes() and stats == want_stats
    assert u64(gen.efficiency((codes, loci), model)[0]).tobytes() == want.tobytes()  # what enumerate_guides returns, as it is
    # N x 21 + GG under the pattern enumeration: the same sites, the same bits
    found, plinear = gen.enumerate_pattern("N" * 21 + "GG", (0, 20), efficiency=model)
    assert found.loci.tobytes() == loci.tobytes() and u64(plinear).tobytes() == want.tobytes()
    assert u64(gen.efficiency(found, model)[0]).tobytes() == want.tobytes()
    with pytest.raises(ValueError):
        gen.enumerate_guides(efficiency=ec.build("zero", (4, 27, 4)))  # site_len 27 is not these candidates'
    with pytest.raises(ValueError):
        gen.enumerate_guides(min_efficiency=0.0)


def test_guides_call_refuses_another_site_length(ctx, planted):
    L = va.lib()
    p = va.api._enum_params("GG", "both", (0, 0), 0, 0)
    h = C.c_void_p()
    _lib.check(L.vsc_guides_enumerate(ctx._h, planted["gen"]._h, None, C.byref(p), C.byref(h)), ctx._h)
    g = Guides(ctx, h)
    m27 = ec.build("zero", (4, 27, 4))
    linear = np.empty(len(g))
    assert L.vsc_guides_efficiency(ctx._h, planted["gen"]._h, g.h, m27._h, _lib.ptr(linear), None) == -22
    assert "site_len" in L.vsc_last_error(ctx._h).decode()
    assert g.filter_code(planted["gen"], m27, 0.0)[0] == -22
    g.close()


@pytest.mark.parametrize("preset,shape", [("SaCas9", (4, 27, 4)), ("Cas12a", (6, 27, 6))])
def test_pattern_candidates_of_other_nucleases(planted, preset, shape):
    gen = planted["gen"]
    pattern, _ = va.pattern_strings(preset)
    proto = va.pattern_protospacer(preset)
    assert len(pattern) == shape[1]
    model = ec.build("dense", shape)
    plain = gen.enumerate_pattern(pattern, proto)
    found, linear = gen.enumerate_pattern(pattern, proto, efficiency=model)
    assert found.codes.tobytes() == plain.codes.tobytes() and found.loci.tobytes() == plain.loci.tobytes() and len(found) > 100
    want, want_stats = ec.expected(planted["contigs"], loci_tuples(found.loci), shape, ec.arrays("dense", shape))
    assert want_stats["defined"] > 100
    assert u64(linear).tobytes() == want.tobytes()
    # the floor, through the wrapper: the survivors in input order, their scores
    defined = want != ec.UNDEF
    floor = float(np.sort(want[defined].view(np.float64))[len(want) // 3])
    keep = defined & (np.where(defined, want.view(np.float64), 0.0) >= floor)
    kept, klinear = gen.enumerate_pattern(pattern, proto, efficiency=model, min_efficiency=floor)
    assert kept.codes.tobytes() == found.codes[keep].tobytes() and kept.loci.tobytes() == found.loci[keep].tobytes()
    assert u64(klinear).tobytes() == want[keep].tobytes()
    d_found, d_rows, d_linear = gen.design_pattern(pattern, proto, 2, efficiency=model, min_efficiency=floor)
    assert d_found.codes.tobytes() == kept.codes.tobytes() and u64(d_linear).tobytes() == want[keep].tobytes()
    _, all_rows = gen.design_pattern(pattern, proto, 2)
    assert d_rows.tobytes() == all_rows[keep].tobytes()  # the survivors alone were searched: their rows are the same rows


# ---- 5. filter ---------------------------------------------------------------------------------------------------------------
def test_filter_floors_and_what_takes_the_result(ctx, planted):
    shape = (4, 23, 3)
    gen, model = planted["gen"], ec.build("sparse", shape)
    codes, loci, linear = gen.enumerate_guides(efficiency=model)
    want, _ = ec.expected(planted["contigs"], loci_tuples(loci), shape, ec.arrays("sparse", shape))
    assert u64(linear).tobytes() == want.tobytes()
    defined = want != ec.UNDEF
    values = np.where(defined, want.view(np.float64), 0.0)
    assert 0 < (~defined).sum()
    g = Guides.from_arrays(ctx, codes, loci)

    def survivors(floor):
        out = g.filter(gen, model, floor)
        got = out.arrays()
        out.close()
        return got

    exact = float(np.sort(values[defined])[defined.sum() // 2])  # a floor that IS one candidate's score keeps that candidate
    for floor in (exact, float(np.nextafter(exact, POS_INF)), 0.0, NEG_INF, -1e300, POS_INF, 1e300):
        keep = defined & (values >= floor)
        got_codes, got_loci = survivors(floor)
        assert got_codes.tobytes() == codes[keep].tobytes() and got_loci.tobytes() == loci[keep].tobytes(), floor
    assert (defined & (values >= exact)).sum() == (defined & (values > exact)).sum() + (values[defined] == exact).sum()
    assert (values[defined] == exact).sum() >= 1 and len(survivors(NEG_INF)[0]) == defined.sum() and len(survivors(POS_INF)[0]) == 0
    code, out = g.filter_code(gen, model, float("nan"))
    assert code == -22 and not out.value and "NaN" in va.lib().vsc_last_error(ctx._h).decode()

    # an empty result is a result: every call that takes a vsc_guides takes it
    empty = g.filter(gen, model, POS_INF)
    assert len(empty) == 0 and len(empty.arrays()[0]) == 0
    assert empty.efficiency(gen, model)[1] == dict.fromkeys(ec.CLASSES, 0)
    again = empty.filter(gen, model, NEG_INF)
    assert len(again) == 0
    again.close()
    empty.close()

    # the host-only object (what the multi-device enumeration returns) goes the host's way, to the same bytes
    host = Guides.from_arrays(ctx, codes, loci, on_device=False)
    h_linear, h_stats = host.efficiency(gen, model)
    assert u64(h_linear).tobytes() == want.tobytes() and h_stats["defined"] == defined.sum()
    h_out = host.filter(gen, model, exact)
    keep = defined & (values >= exact)
    assert h_out.arrays()[0].tobytes() == codes[keep].tobytes() and h_out.arrays()[1].tobytes() == loci[keep].tobytes()
    host.close()

    # the survivors feed the search and the labels as the candidates selected on the host do
    out = g.filter(gen, model, exact)
    o_codes, o_loci = out.arrays()
    rows_all = gen.summarize(codes, 2, exclude=loci)
    assert gen.summarize(o_codes, 2, exclude=o_loci).tobytes() == rows_all[keep].tobytes()
    iv = [(0, 100, 4000), (0, 3000, 9000), (1, 0, 5000), (2, 2900, 3000)]
    regions = va.Regions(planted["packed"], iv)
    labels = np.full(len(out), 7, dtype=np.uint32)
    _lib.check(va.lib().vsc_guides_locate(out.h, regions._h, _lib.ptr(labels)), ctx._h)
    all_labels = gen.enumerate_guides(labels=regions)[2]
    assert labels.tobytes() == all_labels[keep].tobytes() and (labels != va.REGION_NONE).any() and (labels == va.REGION_NONE).any()
    h_out.close()
    out.close()
    g.close()

    # ... and through the wrappers: enumerate_guides and design with a floor
    k_codes, k_loci, k_linear = gen.enumerate_guides(efficiency=model, min_efficiency=exact)
    assert k_codes.tobytes() == codes[keep].tobytes() and k_loci.tobytes() == loci[keep].tobytes()
    assert u64(k_linear).tobytes() == want[keep].tobytes()
    d = gen.design(None, 2, labels=regions, efficiency=model, min_efficiency=exact)
    assert len(d) == 5 and d[0].tobytes() == codes[keep].tobytes() and d[2].tobytes() == rows_all[keep].tobytes()
    assert d[3].tobytes() == all_labels[keep].tobytes() and u64(d[4]).tobytes() == want[keep].tobytes()
    plain = gen.design(None, 2)
    assert len(plain) == 3 and plain[2].tobytes() == rows_all.tobytes()  # without the arguments: what it returned before
    regions.close()


# ---- 6. shards ---------------------------------------------------------------------------------------------------------------
def test_a_shard_scores_what_it_holds(ctx, planted):
    shape = (16, 23, 16)
    packed, contigs = planted["packed"], planted["contigs"]
    model, a = ec.build("dense", shape), ec.arrays("dense", shape)
    n_words = packed.n_words
    assert n_words > 200
    # every start around the two edges, both strands, and the enumeration's candidates
    loci = [(0, p, s) for p in list(range(1960, 2130)) + list(range(2150, 2320)) for s in (0, 1)]
    loci += loci_tuples(planted["gen"].enumerate_guides()[1])
    arr = ec.locus_array(loci)
    whole, _ = ec.expected(contigs, loci, shape, a)
    for first, words, own in ((64, n_words - 64, n_words - 64), (0, 70, 64)):  # nothing in front of word 64; nothing behind a 6-word halo
        sl = slice(first, first + words)
        shard = va.Genome.from_shard(ctx, packed.hi[sl], packed.lo[sl], packed.nmask[sl], first, own, packed.contigs)
        want, want_stats = ec.expected(contigs, loci, shape, a, resident=(32 * first, 32 * (first + words)))
        assert want_stats["not_resident"] > 100 and want_stats["defined"] > 100
        resident = want != ec.UNDEF
        assert (want[resident] == whole[resident]).all()  # (the restatement: what is resident scores as on the whole genome)
        with pytest.raises(ValueError) as e:
            shard.efficiency(arr, model)
        assert "not resident" in str(e.value)
        got, stats = shard.efficiency(arr, model, allow_partial=True)
        assert stats == want_stats and u64(got).tobytes() == want.tobytes()
        shard.close()


# ---- 7. repetition and the context's state ---------------------------------------------------------------------------------
def test_repetition_models_and_timing(ctx, small):
    shape = (4, 23, 3)
    s = small(shape)
    gen, arr, n = s["gen"], s["arr"], len(s["loci"])
    one, two = ec.build("dense", shape, seed=1), ec.build("dense", shape, seed=2)
    want = {m: ec.expected(s["contigs"], s["loci"], shape, ec.arrays("dense", shape, seed=k))[0] for k, m in ((1, one), (2, two))}
    assert want[one].tobytes() != want[two].tobytes()
    for m in (one, one, two, one, two, two, one):  # the device copy is keyed by the model's serial number, never stale
        assert u64(gen.efficiency(arr, m)[0]).tobytes() == want[m].tobytes()
    ctx.release_scratch()
    assert u64(gen.efficiency(arr, two)[0]).tobytes() == want[two].tobytes()
    ctx.release_scratch()
    assert u64(gen.efficiency(arr, two)[0]).tobytes() == want[two].tobytes()
    serial = two.info()["serial"]
    two.close()  # a model that is built after another was freed is another model, whatever its address
    three = ec.build("dense", shape, seed=3)
    assert three.info()["serial"] > serial
    want3 = ec.expected(s["contigs"], s["loci"], shape, ec.arrays("dense", shape, seed=3))[0]
    assert u64(gen.efficiency(arr, three)[0]).tobytes() == want3.tobytes()
    t = ctx.timing()
    assert t["score_ms"] > 0 and t["total_ms"] == t["score_ms"] and t["sites"] == n and t["genome_bytes"] == 24 * n
    for k in ("scan_ms", "prep_ms", "sort_ms", "finalize_ms", "index_ms", "pairs", "hits", "passes", "sort_bytes", "sort_levels", "list_entries"):
        assert t[k] == 0, k
    other = va.Context(0)  # a genome of another context is refused
    with pytest.raises(va.VarscotError) as e:
        st = _lib.EffStats()
        lin = np.empty(n)
        _lib.check(va.lib().vsc_loci_efficiency(other._h, gen._h, _lib.ptr(arr), n, one._h, _lib.ptr(lin), C.byref(st)), other._h)
    assert e.value.code == -22
    other.close()


# ---- 8. the tools end to end ---------------------------------------------------------------------------------------------------
def test_tools_score_and_filter_their_guides(ctx, tmp_path):
    rng = np.random.default_rng(81)
    contigs = [random_seq(rng, 9000), random_seq(rng, 4000)]
    names = ["chr1 assembled", "chr2"]
    chrom = [n.split()[0] for n in names]
    with open(tmp_path / "g.fa", "w") as f:
        for n, s in zip(names, contigs):
            f.write(">%s\n%s\n" % (n, "\n".join(s[i:i + 60] for i in range(0, len(s), 60))))
    iv = [(0, 0, 900), (1, 100, 400), (0, 8800, 9000)]  # (the first and the last reach a contig end: candidates without a context)
    (tmp_path / "t.bed").write_text("".join("%s\t%d\t%d\tx\n" % (chrom[c], a, b) for c, a, b in iv))
    run = lambda *a: subprocess.run([os.path.join(BIN, a[0])] + [str(x) for x in a[1:]], capture_output=True, text=True, timeout=600)  # noqa: E731
    assert run("bidir_index", "-G", tmp_path / "g.fa", "-I", tmp_path / "idx").returncode == 0
    packed = va.PackedGenome.from_sequences(contigs)
    gen = ctx.load_genome(packed)
    fmt = lambda x: "NA" if x != x else "%.17g" % x  # noqa: E731

    # guide_summary -E -L -Y [-y]
    model = ec.build("sparse", (4, 23, 3), link="logistic")
    model.to_tsv(tmp_path / "m.tsv")
    regions = va.Regions(packed, iv, rule="inside")
    codes, loci, linear = gen.enumerate_guides(regions, efficiency=model)
    defined = u64(linear) != ec.UNDEF
    assert 50 < len(codes) < 500 and 0 < (~defined).sum()
    floor = float(np.sort(linear[defined])[defined.sum() // 2])
    keep = defined & (np.where(defined, linear, 0.0) >= floor)
    base = ("guide_summary", "-G", tmp_path / "g.fa", "-I", tmp_path / "idx", "-M", "2", "-E", tmp_path / "t.bed")
    r = run(*base, "-L", tmp_path / "plain.bed", "-O", tmp_path / "plain.tsv")
    assert r.returncode == 0, r.stderr
    r = run(*base, "-L", tmp_path / "y.bed", "-O", tmp_path / "y.tsv", "-Y", tmp_path / "m.tsv")
    assert r.returncode == 0, r.stderr
    plain_bed = (tmp_path / "plain.bed").read_text().splitlines()
    plain_rows = (tmp_path / "plain.tsv").read_text().splitlines()
    assert len(plain_bed) == len(codes) and len(plain_rows) == len(codes) + 1
    assert (tmp_path / "y.tsv").read_bytes() == (tmp_path / "plain.tsv").read_bytes()  # -Y adds to the listing alone
    want_bed = [ln + "\t" + fmt(x) + "\t" + fmt(model.link(x)) for ln, x in zip(plain_bed, linear)]
    assert (tmp_path / "y.bed").read_text().splitlines() == want_bed and any(ln.endswith("\tNA\tNA") for ln in want_bed)
    r = run(*base, "-L", tmp_path / "k.bed", "-O", tmp_path / "k.tsv", "-Y", tmp_path / "m.tsv", "-y", repr(floor))
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "k.bed").read_text().splitlines() == [ln for ln, k in zip(want_bed, keep) if k]
    assert (tmp_path / "k.tsv").read_text().splitlines() == [plain_rows[0]] + [ln for ln, k in zip(plain_rows[1:], keep) if k]
    # the refusals, each with its message
    for args, text in (((*base, "-y", "0.5"), "give -Y"),
                       ((*base[:7], "-B", tmp_path / "plain.bed", "-Y", tmp_path / "m.tsv"), "give -E"),
                       ((*base, "-Y", tmp_path / "m.tsv", "-y", "nan"), "-y takes a floor"),
                       ((*base, "-Y", tmp_path / "m.tsv", "-y", "high"), "-y takes a floor"),
                       ((*base, "-Y", tmp_path / "m.tsv", "-D", "0,0"), "one device"),
                       ((*base, "-Y", tmp_path / "m.bin"), ".tsv/.txt")):
        r = run(*args)
        assert r.returncode != 0 and text in r.stderr, (args, r.stderr)
    ec.build("zero", (4, 27, 4)).to_tsv(tmp_path / "m27.tsv")
    r = run(*base, "-Y", tmp_path / "m27.tsv")
    assert r.returncode != 0 and "site_len is 27" in r.stderr and "23 bases" in r.stderr
    (tmp_path / "bad.tsv").write_text("shape\t4\t23\t3\nmono\t0\tA\t1.0\ncolour\t1\n")
    r = run(*base, "-Y", tmp_path / "bad.tsv")
    assert r.returncode != 0 and "bad.tsv:3:" in r.stderr
    regions.close()

    # pattern_search -E -Y [-y]: SaCas9, the guides of the targets and their screened rows
    pattern, proto = va.pattern_strings("SaCas9")[0], va.pattern_protospacer("SaCas9")
    model27 = ec.build("dense", (4, 27, 4))
    model27.to_tsv(tmp_path / "m27d.tsv")
    targets = [(0, 0, 3000), (1, 0, 4000)]
    (tmp_path / "p.bed").write_text("".join("%s\t%d\t%d\n" % (chrom[c], a, b) for c, a, b in targets))
    found, plinear = gen.enumerate_pattern(pattern, proto, targets=targets, efficiency=model27)
    pdef = u64(plinear) != ec.UNDEF
    assert len(found) > 40 and 0 < (~pdef).sum()
    pfloor = float(np.sort(plinear[pdef])[pdef.sum() // 3])
    pkeep = pdef & (np.where(pdef, plinear, 0.0) >= pfloor)
    pbase = ("pattern_search", "-i", tmp_path / "idx", "-q", pattern, "-p", "%d,%d" % proto, "-B", tmp_path / "p.bed", "-M", "2")
    r = run(*pbase, "-E", tmp_path / "pe.tsv", "-O", tmp_path / "po.tsv")
    assert r.returncode == 0, r.stderr
    r = run(*pbase, "-E", tmp_path / "pey.tsv", "-O", tmp_path / "poy.tsv", "-Y", tmp_path / "m27d.tsv")
    assert r.returncode == 0, r.stderr
    pe = (tmp_path / "pe.tsv").read_text().splitlines()
    po = (tmp_path / "po.tsv").read_text().splitlines()
    assert len(pe) == len(found) + 1 and pe[0] == "#guide\tchrom\tpos\tstrand"
    assert (tmp_path / "poy.tsv").read_bytes() == (tmp_path / "po.tsv").read_bytes()
    want_pe = [pe[0] + "\tefficiencyLinear\tefficiency"] + [ln + "\t" + fmt(x) + "\t" + fmt(x) for ln, x in zip(pe[1:], plinear)]
    assert (tmp_path / "pey.tsv").read_text().splitlines() == want_pe
    r = run(*pbase, "-E", tmp_path / "pek.tsv", "-O", tmp_path / "pok.tsv", "-Y", tmp_path / "m27d.tsv", "-y", repr(pfloor))
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "pek.tsv").read_text().splitlines() == [want_pe[0]] + [ln for ln, k in zip(want_pe[1:], pkeep) if k]
    assert (tmp_path / "pok.tsv").read_text().splitlines() == [po[0]] + [ln for ln, k in zip(po[1:], pkeep) if k]
    for args, text in (((*pbase, "-E", tmp_path / "x.tsv", "-O", tmp_path / "xo.tsv", "-y", "1"), "give -Y"),
                       ((*pbase[:5], "-R", tmp_path / "g.fa", "-M", "2", "-O", tmp_path / "x.tsv", "-Y", tmp_path / "m27d.tsv"), "give -E"),
                       ((*pbase, "-E", tmp_path / "x.tsv", "-O", tmp_path / "xo.tsv", "-Y", tmp_path / "m.tsv"), "site_len is 23")):
        r = run(*args)
        assert r.returncode != 0 and text in (r.stderr + r.stdout), (args, r.stderr)
    gen.close()
