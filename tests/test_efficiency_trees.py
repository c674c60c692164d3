"""The tree-ensemble efficiency score on the device (vsc_loci_efficiency_trees, vsc_guides_efficiency_trees,
vsc_pattern_guides_efficiency_trees and the two filters): bit for bit what the definition gives when it is applied locus by
locus in plain Python (tests/efficiency_trees_cases.py) - integer sums, and additions in tree order, so there is no tolerance;
scores are compared as uint64 views, the undefined NaN included."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import efficiency_cases as ec
import efficiency_trees_cases as tc
import varscot_amd as va
from helpers import random_seq, revcomp
from varscot_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "varscot_amd", "bin")
FILTER_TILE = 1024  # candidates per wave of the filter's passes (include/varscot_hip.h)
NEG_INF, POS_INF = float("-inf"), float("inf")
SMALL_SHAPES = [(4, 23, 3), (16, 32, 16), (0, 16, 0)]  # 4+23+3; C = 64: the window spans three words; no flanks
SMALL_FAMILIES = ["azimuth", "chain", "mixed", "largest", "edges"]


@pytest.fixture(scope="module")
def ctx():
    c = va.Context(0)
    yield c
    c.close()


def u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def loci_tuples(loci):
    return [(int(c), int(p), int(s)) for c, p, s in zip(loci["contig"], loci["pos"], loci["strand"])]


def floor_and_keep(want, part=2):
    """A floor that IS one candidate's score (the median with part=2) and who survives it."""
    defined = want != tc.UNDEF
    values = np.where(defined, want.view(np.float64), 0.0)
    floor = float(np.sort(values[defined])[defined.sum() // part])
    return floor, defined & (values >= floor), defined


class Guides:
    """A vsc_guides (or, pattern=True, a vsc_pattern_guides) handle and its calls with a tree model."""

    def __init__(self, ctx, handle, pattern=False):
        self.ctx, self.h, self.pattern = ctx, handle, pattern
        L = va.lib()
        kind = "vsc_pattern_guides" if pattern else "vsc_guides"
        self.fn = {k: getattr(L, "%s_%s" % (kind, k)) for k in ("count", "data", "free", "efficiency_trees", "filter_efficiency_trees")}

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
        _lib.check(self.fn["efficiency_trees"](self.ctx._h, gen._h, self.h, model._h, _lib.ptr(linear), C.byref(st)), self.ctx._h)
        return linear, st.as_dict()

    def filter_code(self, gen, model, floor):
        out = C.c_void_p()
        return self.fn["filter_efficiency_trees"](self.ctx._h, gen._h, self.h, model._h, floor, C.byref(out)), out

    def filter(self, gen, model, floor):
        code, out = self.filter_code(gen, model, floor)
        _lib.check(code, self.ctx._h)
        return Guides(self.ctx, out, self.pattern)

    def close(self):
        if self.h:
            self.fn["free"](self.h)
            self.h = None


# ---- 1. every locus of a small genome ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(ctx):
    """Per shape: the small genome resident, every locus of it and the loci the definition calls invalid, and - per family,
    computed once - the expected bits and stats."""
    cache = {}

    def get(shape):
        if shape not in cache:
            contigs = ec.small_genome(shape)
            n_contigs, site_len = len(contigs), shape[1]
            loci = ec.every_locus(contigs, site_len)
            loci += [(n_contigs, 0, 0), (0xFFFFFFFF, 0, 0), (0xFFFFFFFF, 0xFFFFFFFF, 1), (4, 10, 2), (4, 10, 0xFFFFFFFF), (4, 200 - site_len + 1, 0),
                     (4, 200 - site_len + 1, 1), (4, 0xFFFFFFFF, 0), (5, 0xFFFFFFFF, 1), (3, 0, 0), (4, 0xFFFFFFFF - site_len + 1, 0)]
            cache[shape] = {"contigs": contigs, "gen": ctx.load_genome(va.PackedGenome.from_sequences(list(contigs))), "loci": loci,
                            "arr": ec.locus_array(loci), "want": {}}
        return cache[shape]

    def want(shape, family):
        s = get(shape)
        if family not in s["want"]:
            s["want"][family] = tc.expected(s["contigs"], s["loci"], shape, tc.lists(family, shape))
        return s["want"][family]

    get.want = want
    yield get
    for s in cache.values():
        s["gen"].close()


@pytest.mark.parametrize("shape", SMALL_SHAPES, ids=lambda s: "%d-%d-%d" % s)
@pytest.mark.parametrize("family", SMALL_FAMILIES)
def test_every_locus_of_a_small_genome(small, family, shape):
    s = small(shape)
    want, want_stats = small.want(shape, family)
    assert want_stats["defined"] > 100 and want_stats["has_n"] > 0 and want_stats["invalid"] == 11
    assert (want_stats["off_contig"] > 0) == (shape[0] + shape[2] > 0)
    got, stats = s["gen"].efficiency(s["arr"], tc.build(family, shape))
    assert stats == want_stats and sum(stats.values()) == len(s["loci"])
    assert u64(got).tobytes() == want.tobytes()
    assert len(np.unique(want)) > (5 if family == "chain" else 200)  # (the chain: nine leaves and the NaN)


def test_nothing_to_score(ctx, small):
    s = small((4, 23, 3))
    got, stats = s["gen"].efficiency(ec.locus_array([]), tc.build("azimuth", (4, 23, 3)))
    assert len(got) == 0 and stats == dict.fromkeys(tc.CLASSES, 0)
    t = ctx.timing()
    assert t["sites"] == 0 and t["score_ms"] == 0 and t["total_ms"] == 0 and t["genome_bytes"] == 0


# ---- 2. more candidates than one launch has lanes, more tiles than it has waves ------------------------------------------------
@pytest.mark.parametrize("family", ["mixed", "largest"])  # (the largest model: fewer workgroups lie on a CU)
def test_more_candidates_than_a_launch_has_lanes(small, family):
    shape = (4, 23, 3)
    s = small(shape)
    want, want_stats = small.want(shape, family)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n, m = cus * 8 * 256 + 77, len(s["loci"])
    assert n > 3 * m  # every lane meets more than one tiling of the loci
    idx = np.arange(n) % m
    got, stats = s["gen"].efficiency(s["arr"][idx], tc.build(family, shape))
    assert u64(got).tobytes() == want[idx].tobytes()
    per = {k: int(v) for k, v in zip(*np.unique(np.array([tc.classify(s["contigs"], l, shape)[0] for l in s["loci"]])[idx], return_counts=True))}
    assert stats == {k: per.get(k, 0) for k in tc.CLASSES} and sum(stats.values()) == n


def test_filter_over_more_tiles_than_a_launch_has_waves(ctx, small):
    shape = (4, 23, 3)
    s = small(shape)
    want, _ = small.want(shape, "chain")
    model = tc.build("chain", shape)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    m = len(s["loci"])
    n = (cus * 8 * 4 + 3) * FILTER_TILE + 77  # the last tile is a partial one
    idx = np.arange(n) % m
    floor, keep, defined = floor_and_keep(want)
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


# ---- 3. candidates where they lie ----------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("family", ["azimuth", "mixed"])
def test_enumerated_guides_are_scored_where_they_lie(ctx, planted, family):
    shape = (6, 23, 6)
    gen, model = planted["gen"], tc.build(family, shape)
    plain = gen.enumerate_guides()
    codes, loci, linear = gen.enumerate_guides(efficiency=model)
    assert codes.tobytes() == plain[0].tobytes() and loci.tobytes() == plain[1].tobytes() and len(codes) > 1000
    want, want_stats = tc.expected(planted["contigs"], loci_tuples(loci), shape, tc.lists(family, shape))
    assert want_stats["off_contig"] >= 6 and want_stats["defined"] > 1000  # the planted sites next to the ends have no context
    assert u64(linear).tobytes() == want.tobytes()
    by_loci, stats = gen.efficiency(loci, model)
    assert u64(by_loci).tobytes() == want.tobytes() and stats == want_stats
    assert u64(gen.efficiency((codes, loci), model)[0]).tobytes() == want.tobytes()  # what enumerate_guides returns, as it is
    # N x 21 + GG under the pattern enumeration: the same sites, the same bits
    found, plinear = gen.enumerate_pattern("N" * 21 + "GG", (0, 20), efficiency=model)
    assert found.loci.tobytes() == loci.tobytes() and u64(plinear).tobytes() == want.tobytes()
    assert u64(gen.efficiency(found, model)[0]).tobytes() == want.tobytes()
    # handles made from host arrays: on the device, and host-only (what the multi-device enumeration returns)
    for on_device in (True, False):
        g = Guides.from_arrays(ctx, codes, loci, on_device=on_device)
        g_linear, g_stats = g.efficiency(gen, model)
        assert u64(g_linear).tobytes() == want.tobytes() and g_stats == want_stats
        floor, keep, _ = floor_and_keep(want)
        out = g.filter(gen, model, floor)
        assert out.arrays()[0].tobytes() == codes[keep].tobytes() and out.arrays()[1].tobytes() == loci[keep].tobytes()
        out.close()
        g.close()
    with pytest.raises(ValueError):
        gen.enumerate_guides(efficiency=tc.build("leaf1", (4, 27, 4)))  # site_len 27 is not these candidates'


def test_guides_call_refuses_another_site_length(ctx, planted):
    L = va.lib()
    p = va.api._enum_params("GG", "both", (0, 0), 0, 0)
    h = C.c_void_p()
    _lib.check(L.vsc_guides_enumerate(ctx._h, planted["gen"]._h, None, C.byref(p), C.byref(h)), ctx._h)
    g = Guides(ctx, h)
    m27 = tc.build("leaf1", (4, 27, 4))
    linear = np.empty(len(g))
    assert L.vsc_guides_efficiency_trees(ctx._h, planted["gen"]._h, g.h, m27._h, _lib.ptr(linear), None) == -22
    assert "site_len" in L.vsc_last_error(ctx._h).decode()
    assert g.filter_code(planted["gen"], m27, 0.0)[0] == -22
    g.close()


@pytest.mark.parametrize("preset,shape", [("SaCas9", (4, 27, 4)), ("Cas12a", (6, 27, 6))])
def test_pattern_candidates_of_other_nucleases(planted, preset, shape):
    gen = planted["gen"]
    pattern, _ = va.pattern_strings(preset)
    proto = va.pattern_protospacer(preset)
    assert len(pattern) == shape[1]
    model = tc.build("azimuth", shape)
    plain = gen.enumerate_pattern(pattern, proto)
    found, linear = gen.enumerate_pattern(pattern, proto, efficiency=model)
    assert found.codes.tobytes() == plain.codes.tobytes() and found.loci.tobytes() == plain.loci.tobytes() and len(found) > 100
    want, want_stats = tc.expected(planted["contigs"], loci_tuples(found.loci), shape, tc.lists("azimuth", shape))
    assert want_stats["defined"] > 100
    assert u64(linear).tobytes() == want.tobytes()
    # the floor, through the wrapper: the survivors in input order, their scores; design_pattern equals the two-step route
    floor, keep, _ = floor_and_keep(want, part=3)
    kept, klinear = gen.enumerate_pattern(pattern, proto, efficiency=model, min_efficiency=floor)
    assert kept.codes.tobytes() == found.codes[keep].tobytes() and kept.loci.tobytes() == found.loci[keep].tobytes()
    assert u64(klinear).tobytes() == want[keep].tobytes()
    d_found, d_rows, d_linear = gen.design_pattern(pattern, proto, 2, efficiency=model, min_efficiency=floor)
    assert d_found.codes.tobytes() == kept.codes.tobytes() and u64(d_linear).tobytes() == want[keep].tobytes()
    _, all_rows = gen.design_pattern(pattern, proto, 2)
    assert d_rows.tobytes() == all_rows[keep].tobytes()  # the survivors alone were searched: their rows are the same rows


# ---- 4. filters ----------------------------------------------------------------------------------------------------------------
def stumps_of(a, C_):
    """The tree model that adds up a linear model's mono terms in its order (test_efficiency_trees_cpu.py checks the bits)."""
    return [[("base", j, "ACGT"[b], 1, 2), ("leaf", float(a["mono"][j, b])), ("leaf", 0.0)] for j in range(C_) for b in range(4)]


def test_filter_floors_and_what_takes_the_result(ctx, planted):
    shape = (4, 23, 3)
    gen, model = planted["gen"], tc.build("azimuth", shape)
    codes, loci, linear = gen.enumerate_guides(efficiency=model)
    want, _ = tc.expected(planted["contigs"], loci_tuples(loci), shape, tc.lists("azimuth", shape))
    assert u64(linear).tobytes() == want.tobytes()
    exact, keep, defined = floor_and_keep(want)  # the median: a floor that IS one candidate's score keeps that candidate
    values = np.where(defined, want.view(np.float64), 0.0)
    assert 0 < (~defined).sum()
    g = Guides.from_arrays(ctx, codes, loci)

    def survivors(floor):
        out = g.filter(gen, model, floor)
        got = out.arrays()
        out.close()
        return got

    for floor in (exact, float(np.nextafter(exact, POS_INF)), 0.0, NEG_INF, -1e300, POS_INF, 1e300):
        k = defined & (values >= floor)
        got_codes, got_loci = survivors(floor)
        assert got_codes.tobytes() == codes[k].tobytes() and got_loci.tobytes() == loci[k].tobytes(), floor
    assert (values[defined] == exact).sum() >= 1 and len(survivors(NEG_INF)[0]) == defined.sum() and len(survivors(POS_INF)[0]) == 0
    code, out = g.filter_code(gen, model, float("nan"))
    assert code == -22 and not out.value and "NaN" in va.lib().vsc_last_error(ctx._h).decode()

    # an empty result is a result: every call that takes a vsc_guides takes it
    empty = g.filter(gen, model, POS_INF)
    assert len(empty) == 0 and len(empty.arrays()[0]) == 0
    assert empty.efficiency(gen, model)[1] == dict.fromkeys(tc.CLASSES, 0)
    again = empty.filter(gen, model, NEG_INF)
    assert len(again) == 0
    again.close()
    empty.close()

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
    out.close()
    g.close()

    # ... and through the wrappers: enumerate_guides and design with a floor equal the two-step route
    k_codes, k_loci, k_linear = gen.enumerate_guides(efficiency=model, min_efficiency=exact)
    assert k_codes.tobytes() == codes[keep].tobytes() and k_loci.tobytes() == loci[keep].tobytes()
    assert u64(k_linear).tobytes() == want[keep].tobytes()
    d = gen.design(None, 2, labels=regions, efficiency=model, min_efficiency=exact)
    assert len(d) == 5 and d[0].tobytes() == codes[keep].tobytes() and d[2].tobytes() == rows_all[keep].tobytes()
    assert d[3].tobytes() == all_labels[keep].tobytes() and u64(d[4]).tobytes() == want[keep].tobytes()

    # Genome.pick by the "eff" column: a tree model of stumps that adds up a linear model's terms picks what that model picks
    a = ec.arrays("sparse", shape)
    lin = va.EfficiencyModel(shape[0], shape[1], shape[2], a["intercept"], a["mono"], np.zeros((29, 16)))
    tree = va.TreeEfficiencyModel(shape[0], shape[1], shape[2], a["intercept"], [], stumps_of(a, 30))
    floor = float(np.nanmedian(gen.efficiency(loci, lin)[0]))
    ps = va.PickShape(3, 20)
    by_lin = gen.design(regions, 2, efficiency=lin, min_efficiency=floor, pick=ps, pick_by=("eff", "mit"))
    by_tree = gen.design(regions, 2, efficiency=tree, min_efficiency=floor, pick=ps, pick_by=("eff", "mit"))
    assert len(by_lin) == len(by_tree) == 6 and 0 < len(by_tree[0]) < len(codes)
    for x, y in zip(by_lin, by_tree):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()
    assert (np.asarray(by_tree[4]) != va.PICK_NONE).any()
    regions.close()


# ---- 5. the device copies of the models ----------------------------------------------------------------------------------------
def test_the_device_copy_is_the_model_of_the_call(ctx, small):
    shape = (4, 23, 3)
    s = small(shape)
    gen, arr, n = s["gen"], s["arr"], len(s["loci"])
    one, two, lin = tc.build("azimuth", shape, seed=1), tc.build("stumps", shape, seed=2), ec.build("dense", shape)
    want = {one: tc.expected(s["contigs"], s["loci"], shape, tc.lists("azimuth", shape, seed=1))[0],
            two: tc.expected(s["contigs"], s["loci"], shape, tc.lists("stumps", shape, seed=2))[0],
            lin: ec.expected(s["contigs"], s["loci"], shape, ec.arrays("dense", shape))[0]}
    assert len({w.tobytes() for w in want.values()}) == 3
    for k, m in enumerate((one, one, two, lin, one, two, two, lin, lin, one)):  # keyed by serial number, never stale, side by side
        assert u64(gen.efficiency(arr, m)[0]).tobytes() == want[m].tobytes()
        if k in (2, 5, 6):
            ctx.release_scratch()
    serial = two.info()["serial"]
    two.close()  # a model that is built after another was freed is another model, whatever its address
    three = tc.build("stumps", shape, seed=3)
    assert three.info()["serial"] > serial
    want3 = tc.expected(s["contigs"], s["loci"], shape, tc.lists("stumps", shape, seed=3))[0]
    assert u64(gen.efficiency(arr, three)[0]).tobytes() == want3.tobytes()
    t = ctx.timing()
    assert t["score_ms"] > 0 and t["total_ms"] == t["score_ms"] and t["sites"] == n and t["genome_bytes"] == 24 * n
    other = va.Context(0)  # a genome of another context is refused
    st, out = _lib.EffStats(), np.empty(n)
    assert va.lib().vsc_loci_efficiency_trees(other._h, gen._h, _lib.ptr(arr), n, one._h, _lib.ptr(out), C.byref(st)) == -22
    assert va.lib().vsc_loci_efficiency_trees(ctx._h, gen._h, _lib.ptr(arr), n, None, _lib.ptr(out), C.byref(st)) == -22
    assert va.lib().vsc_loci_efficiency_trees(ctx._h, gen._h, _lib.ptr(arr), n, one._h, None, C.byref(st)) == -22
    other.close()


# ---- 6. shards -----------------------------------------------------------------------------------------------------------------
def test_a_shard_scores_what_it_holds(ctx, planted):
    shape = (16, 23, 16)
    packed, contigs = planted["packed"], planted["contigs"]
    model, lists = tc.build("azimuth", shape), tc.lists("azimuth", shape)
    n_words = packed.n_words
    loci = [(0, p, s) for p in list(range(1960, 2130)) + list(range(2150, 2320)) for s in (0, 1)]  # every start around the two edges
    loci += loci_tuples(planted["gen"].enumerate_guides()[1])
    arr = ec.locus_array(loci)
    whole, _ = tc.expected(contigs, loci, shape, lists)
    for first, words, own in ((64, n_words - 64, n_words - 64), (0, 70, 64)):  # nothing in front of word 64; nothing behind a 6-word halo
        sl = slice(first, first + words)
        shard = va.Genome.from_shard(ctx, packed.hi[sl], packed.lo[sl], packed.nmask[sl], first, own, packed.contigs)
        want, want_stats = tc.expected(contigs, loci, shape, lists, resident=(32 * first, 32 * (first + words)))
        assert want_stats["not_resident"] > 100 and want_stats["defined"] > 100
        resident = want != tc.UNDEF
        assert (want[resident] == whole[resident]).all()
        with pytest.raises(ValueError) as e:
            shard.efficiency(arr, model)
        assert "not resident" in str(e.value)
        got, stats = shard.efficiency(arr, model, allow_partial=True)
        assert stats == want_stats and u64(got).tobytes() == want.tobytes()
        shard.close()


# ---- 7. the tools end to end ---------------------------------------------------------------------------------------------------
def test_tools_take_a_tree_model_file(ctx, tmp_path):
    rng = np.random.default_rng(81)
    contigs = [random_seq(rng, 9000), random_seq(rng, 4000)]
    chrom = ["chr1", "chr2"]
    with open(tmp_path / "g.fa", "w") as f:
        for n, s in zip(chrom, contigs):
            f.write(">%s\n%s\n" % (n, "\n".join(s[i:i + 60] for i in range(0, len(s), 60))))
    iv = [(0, 0, 900), (1, 100, 400), (0, 8800, 9000)]  # (the first and the last reach a contig end: candidates without a context)
    (tmp_path / "t.bed").write_text("".join("%s\t%d\t%d\tx\n" % (chrom[c], a, b) for c, a, b in iv))
    run = lambda *a: subprocess.run([os.path.join(BIN, a[0])] + [str(x) for x in a[1:]], capture_output=True, text=True, timeout=600)  # noqa: E731
    assert run("bidir_index", "-G", tmp_path / "g.fa", "-I", tmp_path / "idx").returncode == 0
    packed = va.PackedGenome.from_sequences(contigs)
    gen = ctx.load_genome(packed)
    fmt = lambda x: "NA" if x != x else "%.17g" % x  # noqa: E731

    # guide_summary -E -L -Y [-y]
    shape = (4, 23, 3)
    model = tc.build("azimuth", shape, link="logistic")
    model.to_tsv(tmp_path / "m.tsv")
    regions = va.Regions(packed, iv, rule="inside")
    codes, loci, linear = gen.enumerate_guides(regions, efficiency=model)
    want, _ = tc.expected(contigs, loci_tuples(loci), shape, tc.lists("azimuth", shape))
    assert u64(linear).tobytes() == want.tobytes()
    floor, keep, defined = floor_and_keep(want)
    assert 50 < len(codes) < 500 and 0 < (~defined).sum()
    base = ("guide_summary", "-G", tmp_path / "g.fa", "-I", tmp_path / "idx", "-M", "2", "-E", tmp_path / "t.bed")
    r = run(*base, "-L", tmp_path / "plain.bed", "-O", tmp_path / "plain.tsv")
    assert r.returncode == 0, r.stderr
    r = run(*base, "-L", tmp_path / "y.bed", "-O", tmp_path / "y.tsv", "-Y", tmp_path / "m.tsv")
    assert r.returncode == 0, r.stderr
    plain_bed = (tmp_path / "plain.bed").read_text().splitlines()
    plain_rows = (tmp_path / "plain.tsv").read_text().splitlines()
    assert len(plain_bed) == len(codes)
    assert (tmp_path / "y.tsv").read_bytes() == (tmp_path / "plain.tsv").read_bytes()  # -Y adds to the listing alone
    want_bed = [ln + "\t" + fmt(x) + "\t" + fmt(model.link(x)) for ln, x in zip(plain_bed, linear)]
    assert (tmp_path / "y.bed").read_text().splitlines() == want_bed and any(ln.endswith("\tNA\tNA") for ln in want_bed)
    r = run(*base, "-L", tmp_path / "k.bed", "-O", tmp_path / "k.tsv", "-Y", tmp_path / "m.tsv", "-y", repr(floor))
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "k.bed").read_text().splitlines() == [ln for ln, k in zip(want_bed, keep) if k]
    assert (tmp_path / "k.tsv").read_text().splitlines() == [plain_rows[0]] + [ln for ln, k in zip(plain_rows[1:], keep) if k]
    # -k -b eff: the tree model of stumps that adds up a linear model's terms gives, byte for byte, what the linear file gives
    a = ec.arrays("sparse", shape)
    va.EfficiencyModel(4, 23, 3, a["intercept"], a["mono"], np.zeros((29, 16))).to_tsv(tmp_path / "lin.tsv")
    va.TreeEfficiencyModel(4, 23, 3, a["intercept"], [], stumps_of(a, 30)).to_tsv(tmp_path / "stumps.tsv")
    outs = {}
    for name in ("lin", "stumps"):
        r = run(*base, "-L", tmp_path / (name + ".bed"), "-O", tmp_path / (name + "_o.tsv"), "-Y", tmp_path / (name + ".tsv"), "-y", "0.0",
                "-k", "2,20", "-b", "eff,mit")
        assert r.returncode == 0, r.stderr
        outs[name] = ((tmp_path / (name + ".bed")).read_bytes(), (tmp_path / (name + "_o.tsv")).read_bytes())
    assert outs["lin"] == outs["stumps"] and sum(1 for ln in outs["stumps"][0].decode().splitlines() if not ln.endswith("\tNA\tNA")) > 3
    # the refusals: each with FILE:LINE, before a device is opened
    good = (tmp_path / "stumps.tsv").read_text().splitlines()
    at = next(i for i, ln in enumerate(good) if ln.startswith("tree\t1"))
    for where, lines, text in ((at + 1, good[:at] + ["mono\t0\tA\t1.0"] + good[at:], "linear model"),
                               (at + 1, good[:at] + ["leaf\t5\t1.0"] + good[at:], "out of turn"),
                               (at, good[:at - 1] + good[at:], "tree 0"),              # tree 0 lost its last leaf: seen where tree 1 begins
                               (at + 2, good[:at + 1] + ["base_in\t0\t30\tA\t1\t2"] + good[at + 2:], "outside"),
                               (3, good[:2] + ["link\tprobit"] + good[3:], "link")):
        (tmp_path / "bad.tsv").write_text("\n".join(lines) + "\n")
        r = run(*base, "-Y", tmp_path / "bad.tsv")
        assert r.returncode == 1 and "bad.tsv:%d:" % where in r.stderr and text in r.stderr, (where, text, r.stderr)
    tc.build("leaf1", (4, 27, 4)).to_tsv(tmp_path / "m27.tsv")
    r = run(*base, "-Y", tmp_path / "m27.tsv")
    assert r.returncode != 0 and "site_len is 27" in r.stderr and "23 bases" in r.stderr
    regions.close()

    # pattern_search -E -Y [-y]: SaCas9, the guides of the targets and their screened rows
    pattern, proto = va.pattern_strings("SaCas9")[0], va.pattern_protospacer("SaCas9")
    model27 = tc.build("azimuth", (4, 27, 4))
    model27.to_tsv(tmp_path / "m27a.tsv")
    targets = [(0, 0, 3000), (1, 0, 4000)]
    (tmp_path / "p.bed").write_text("".join("%s\t%d\t%d\n" % (chrom[c], a, b) for c, a, b in targets))
    found, plinear = gen.enumerate_pattern(pattern, proto, targets=targets, efficiency=model27)
    pwant, _ = tc.expected(contigs, loci_tuples(found.loci), (4, 27, 4), tc.lists("azimuth", (4, 27, 4)))
    assert u64(plinear).tobytes() == pwant.tobytes()
    pfloor, pkeep, pdef = floor_and_keep(pwant, part=3)
    assert len(found) > 40 and 0 < (~pdef).sum()
    pbase = ("pattern_search", "-i", tmp_path / "idx", "-q", pattern, "-p", "%d,%d" % proto, "-B", tmp_path / "p.bed", "-M", "2")
    r = run(*pbase, "-E", tmp_path / "pe.tsv", "-O", tmp_path / "po.tsv")
    assert r.returncode == 0, r.stderr
    r = run(*pbase, "-E", tmp_path / "pey.tsv", "-O", tmp_path / "poy.tsv", "-Y", tmp_path / "m27a.tsv")
    assert r.returncode == 0, r.stderr
    pe = (tmp_path / "pe.tsv").read_text().splitlines()
    po = (tmp_path / "po.tsv").read_text().splitlines()
    assert len(pe) == len(found) + 1
    assert (tmp_path / "poy.tsv").read_bytes() == (tmp_path / "po.tsv").read_bytes()
    want_pe = [pe[0] + "\tefficiencyLinear\tefficiency"] + [ln + "\t" + fmt(x) + "\t" + fmt(x) for ln, x in zip(pe[1:], plinear)]
    assert (tmp_path / "pey.tsv").read_text().splitlines() == want_pe
    r = run(*pbase, "-E", tmp_path / "pek.tsv", "-O", tmp_path / "pok.tsv", "-Y", tmp_path / "m27a.tsv", "-y", repr(pfloor))
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "pek.tsv").read_text().splitlines() == [want_pe[0]] + [ln for ln, k in zip(want_pe[1:], pkeep) if k]
    assert (tmp_path / "pok.tsv").read_text().splitlines() == [po[0]] + [ln for ln, k in zip(po[1:], pkeep) if k]
    r = run(*pbase, "-E", tmp_path / "pb.tsv", "-O", tmp_path / "pbo.tsv", "-Y", tmp_path / "m27a.tsv", "-k", "2,20", "-b", "eff")
    assert r.returncode == 0, r.stderr + r.stdout
    pb = (tmp_path / "pb.tsv").read_text().splitlines()
    assert pb[0] == want_pe[0] + "\tpickTarget\tpickRank" and [ln.rsplit("\t", 2)[0] for ln in pb[1:]] == want_pe[1:]
    assert 0 < sum(1 for ln in pb[1:] if not ln.endswith("\tNA\tNA")) <= 4
    r = run(*pbase, "-E", tmp_path / "x.tsv", "-O", tmp_path / "xo.tsv", "-Y", tmp_path / "m.tsv")
    assert r.returncode != 0 and "site_len is 23" in (r.stderr + r.stdout)
    gen.close()
