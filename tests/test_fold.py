"""The guide RNA's self-complementarity on the device (vsc_loci_fold, vsc_guides_fold, vsc_pattern_guides_fold and the two
filters): bit for bit what the definition gives when it is applied locus by locus on STRINGS (tests/fold_cases.py).  Integers,
so there is no tolerance: the rows are compared as uint32, the undefined row included."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import fold_cases as fc
import varscot_amd as va
import wide_cases as wc
from helpers import random_seq, revcomp
from varscot_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "varscot_amd", "bin")
FILTER_TILE = 1024  # candidates per wave of the filter's passes (include/varscot_hip.h)
DROP_FRONT, DROP_BACK = 2, 1  # words the partial object of the small genome does not hold
NONE = (fc.NO_LIMIT,) * 4
# the (shape, scaffold length) pairs whose small genome is walked locus by locus: both presets, the smallest and the largest
# spacer, every flag and bound of SHAPE, scaffolds on both sides of the 32-letter boundaries
SMALL = [("SpCas9", 76), ("Cas12a", 33), ("SpCas9_wobble", 31), ("n12_site16", 32), ("n32_site32", 8), ("n32_wobble", 65), ("at_site_end", 96),
         ("no_seed", 0), ("seed_5prime", 65)]


@pytest.fixture(scope="module")
def ctx():
    c = va.Context(0)
    yield c
    c.close()


def loci_tuples(loci):
    return [(int(c), int(p), int(s)) for c, p, s in zip(loci["contig"], loci["pos"], loci["strand"])]


def counts(stats):
    return {k: stats[k] for k in fc.CLASSES}


class Guides:
    """A vsc_guides (or, pattern=True, a vsc_pattern_guides) handle and its fold calls."""

    def __init__(self, ctx, handle, pattern=False):
        self.ctx, self.h, self.pattern = ctx, handle, pattern
        L = va.lib()
        kind = "vsc_pattern_guides" if pattern else "vsc_guides"
        self.fn = {k: getattr(L, "%s_%s" % (kind, k)) for k in ("count", "data", "free", "fold", "filter_fold")}

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

    def fold(self, gen, shape, scaffold):
        rows, st = np.empty((len(self), 2), dtype=np.uint32), _lib.FoldStats()
        sh, sc = shape._struct(), va.api._fold_scaffold(scaffold, validate=False)
        _lib.check(self.fn["fold"](self.ctx._h, gen._h, self.h, C.byref(sh), sc, len(sc), _lib.ptr(rows), C.byref(st)), self.ctx._h)
        return rows, st.as_dict()

    def filter_code(self, gen, shape, scaffold, limits):
        out = C.c_void_p()
        sh, sc, lim = shape._struct(), va.api._fold_scaffold(scaffold, validate=False), _lib.FoldLimits(*limits)
        return self.fn["filter_fold"](self.ctx._h, gen._h, self.h, C.byref(sh), sc, len(sc), C.byref(lim), C.byref(out)), out

    def filter(self, gen, shape, scaffold, limits):
        code, out = self.filter_code(gen, shape, scaffold, limits)
        _lib.check(code, self.ctx._h)
        return Guides(self.ctx, out, self.pattern)

    def close(self):
        if self.h:
            self.fn["free"](self.h)
            self.h = None


# ---- 1. every locus of the small genome ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(ctx):
    """Per (shape, scaffold length): the small genome resident - whole, and as an object that lacks the first two words and the
    last one - every locus of it, and the expected rows, computed once."""
    cache = {}

    def get(name, m):
        if (name, m) not in cache:
            contigs = fc.small_genome(name, m)
            packed = va.PackedGenome.from_sequences(list(contigs))
            loci = fc.every_locus(contigs)
            sl = slice(DROP_FRONT, packed.n_words - DROP_BACK)
            part = va.Genome.from_shard(ctx, packed.hi[sl], packed.lo[sl], packed.nmask[sl], DROP_FRONT, sl.stop - sl.start, packed.contigs)
            cache[name, m] = {"contigs": contigs, "packed": packed, "gen": ctx.load_genome(packed), "part": part, "loci": loci,
                              "arr": fc.locus_array(loci), "resident": (32 * sl.start, 32 * sl.stop), "want": {}, "shape": fc.SHAPE_OF[name],
                              "sh": fc.va_shape(fc.SHAPE_OF[name]), "scaffold": fc.scaffold(name, m)}
        return cache[name, m]

    def want(name, m, partial=False):
        s = get(name, m)
        if partial not in s["want"]:
            s["want"][partial] = fc.expected(s["contigs"], s["loci"], s["shape"], s["scaffold"], s["resident"] if partial else None)
        return s["want"][partial]

    get.want = want
    yield get
    for s in cache.values():
        s["gen"].close()
        s["part"].close()


@pytest.mark.parametrize("name,m", SMALL, ids=["%s-m%d" % p for p in SMALL])
def test_every_locus_of_a_small_genome(small, name, m):
    s = small(name, m)
    shape = s["shape"]
    want, want_stats, texts = small.want(name, m, partial=True)
    # what the fixture is for, on the restatement alone
    assert want_stats["off_contig"] == 0 and all(want_stats[k] >= 5 for k in fc.CLASSES if k != "off_contig"), want_stats
    u = va.unpack_fold_row(want)
    assert (u["defined"] & (u["starts"] > 0)).sum() >= 5 and (u["defined"] & (u["starts"] == 0)).any()
    assert (u["self_starts"] > 0).any() and (m < shape.stem or (u["scaf_starts"] > 0).any() or (u["scaf_longest"] >= shape.stem).any())
    for strand in (0, 1):  # the planted spacers are met on both strands, and the sites at both ends of a contig
        on = [t for l, t in zip(s["loci"], texts) if l[2] == strand and t is not None]
        assert len(on) > 100 and len(set(on) & {g for _, g in fc.cases(name, m)}) >= 3
        for c, text in enumerate(s["contigs"]):
            if len(text) >= shape.site_len:
                at = {l[1] for l, t in zip(s["loci"], texts) if l[0] == c and l[2] == strand and t is not None}
                assert c != 3 or {0, len(text) - shape.site_len} & at
    first = [fc.offsets(s["contigs"])[l[0]] + l[1] for l, t, r in zip(s["loci"], texts, want) if t is not None and r.any()]
    assert sum(g // 32 != (g + shape.site_len - 1) // 32 for g in first) >= 20 and len({g % 32 for g in first}) >= 16  # across a plane-word boundary
    got, stats = s["part"].fold(s["arr"], s["sh"], s["scaffold"], allow_partial=True)
    assert got.dtype == np.uint32 and got.shape == want.shape
    assert counts(stats) == want_stats and sum(want_stats.values()) == len(s["loci"])
    assert got.tobytes() == want.tobytes()
    # the whole genome: nothing is missing, and what was resident has the same row
    whole, whole_stats, _ = small.want(name, m)
    got, stats = s["gen"].fold(s["arr"], s["sh"], s["scaffold"])
    assert counts(stats) == whole_stats and stats["not_resident"] == 0 and got.tobytes() == whole.tobytes()
    defined = want[:, 0] != fc.UNDEF
    assert (whole[defined] == want[defined]).all()
    with pytest.raises(ValueError) as e:
        s["part"].fold(s["arr"], s["sh"], s["scaffold"])
    assert "not resident" in str(e.value)
    if m == 0:  # no scaffold: no scaffold walk, scaf_* = 0
        assert not u["scaf_starts"].any() and not u["scaf_longest"].any()
        assert s["gen"].fold(s["arr"], s["sh"])[0].tobytes() == whole.tobytes() and s["gen"].fold(s["arr"], s["sh"], "")[0].tobytes() == whole.tobytes()


def test_invalid_loci_are_classed_and_never_followed(small):
    s = small("SpCas9", 76)
    n_contigs, main = len(s["contigs"]), 3
    length = len(s["contigs"][main])
    bad = [(n_contigs, 0, 0), (0xFFFFFFFF, 0, 0), (0xFFFFFFFF, 0xFFFFFFFF, 1), (main, 10, 2), (main, 10, 0xFFFFFFFF), (main, length - 22, 0),
           (main, length - 22, 1), (main, 0xFFFFFFFF, 0), (main + 1, 0xFFFFFFFF, 1), (0, 7, 0), (main, 0xFFFFFFFF - 22, 0)]
    loci = bad + [(main, 100, 0)]
    want, want_stats, _ = fc.expected(s["contigs"], loci, s["shape"], s["scaffold"])
    assert want_stats["invalid"] == len(bad) and want_stats["defined"] == 1
    got, stats = s["gen"].fold(fc.locus_array(loci), s["sh"], s["scaffold"])
    assert counts(stats) == want_stats and got.tobytes() == want.tobytes() and (got[:-1] == fc.UNDEF).all()


def test_nothing_to_score(ctx, small):
    s = small("SpCas9", 76)
    got, stats = s["gen"].fold(fc.locus_array([]), s["sh"], s["scaffold"])
    assert got.shape == (0, 2) and counts(stats) == dict.fromkeys(fc.CLASSES, 0)
    t = ctx.timing()
    assert t["sites"] == 0 and t["score_ms"] == 0 and t["total_ms"] == 0 and t["genome_bytes"] == 0


# ---- 2. more candidates than one launch has lanes, more tiles than it has waves; the grid's cap -------------------------------
def launch_waves():
    """The waves of a launch capped as the cells' grids are (wide_cases): CUs x 8 workgroups of 4 waves."""
    return torch.cuda.get_device_properties(0).multi_processor_count * wc.GROUPS_PER_CU * wc.WAVES_PER_GROUP


def test_more_candidates_than_a_launch_has_lanes(small):
    s = small("Cas12a", 33)
    want, _, _ = small.want("Cas12a", 33, partial=True)
    n, m = launch_waves() * 64 + 77, len(s["loci"])
    assert n > 3 * m  # every lane meets more than one tiling of the loci
    idx = np.arange(n) % m
    got, stats = s["part"].fold(s["arr"][idx], s["sh"], s["scaffold"], allow_partial=True)
    assert got.tobytes() == want[idx].tobytes()
    cls = np.array([fc.classify(s["contigs"], l, s["shape"], s["resident"])[0] for l in s["loci"]])[idx]
    per = {k: int(v) for k, v in zip(*np.unique(cls, return_counts=True))}
    assert counts(stats) == {k: per.get(k, 0) for k in fc.CLASSES} and sum(counts(stats).values()) == n


def test_one_workgroup_per_cu_takes_many_steps_to_the_same_bytes(ctx, small):
    L = va.lib()
    s = small("SpCas9", 76)
    want, want_stats, _ = small.want("SpCas9", 76)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    m = len(s["loci"])
    n = cus * 256 * 5 + 131  # five grid-stride steps of every workgroup and a partial one at one workgroup per CU
    idx = np.arange(n) % m
    got = {}
    try:
        for groups in (0, 1, 3, 64, 0):
            assert L.vsc_debug_fold_groups_per_cu(ctx._h, groups) == 0
            rows, stats = s["gen"].fold(s["arr"][idx], s["sh"], s["scaffold"])
            got[groups] = (rows.tobytes(), tuple(sorted(counts(stats).items())))
    finally:
        L.vsc_debug_fold_groups_per_cu(ctx._h, 0)
    assert got[0][0] == want[idx].tobytes() and len(set(got.values())) == 1
    assert sum(v for _, v in got[1][1]) == n
    assert L.vsc_debug_fold_groups_per_cu(ctx._h, 65) == -22 and L.vsc_debug_fold_groups_per_cu(None, 1) == -22


def test_filter_over_more_tiles_than_a_launch_has_waves(ctx, small):
    s = small("SpCas9", 76)
    want, _, _ = small.want("SpCas9", 76)
    m = len(s["loci"])
    n = (launch_waves() + 3) * FILTER_TILE + 77  # the last tile is a partial one
    idx = np.arange(n) % m
    defined = want[:, 0] != fc.UNDEF
    limits = (2, 4, fc.NO_LIMIT, 6)
    keep = np.array([fc.keep(r, limits) for r in want])
    assert 0 < keep.sum() < defined.sum()
    codes = np.arange(n, dtype=np.uint64) * np.uint64(3)  # (the filter copies codes, it does not read them)
    g = Guides.from_arrays(ctx, codes, s["arr"][idx])
    out = g.filter(s["gen"], s["sh"], s["scaffold"], limits)
    got_codes, got_loci = out.arrays()
    chosen = np.nonzero(keep[idx])[0]
    assert len(got_codes) == len(chosen)
    assert got_codes.tobytes() == codes[chosen].tobytes() and got_loci.tobytes() == s["arr"][idx][chosen].tobytes()
    t = ctx.timing()
    assert t["sites"] == n and t["genome_bytes"] == 32 * n + 48 * len(chosen) and t["score_ms"] == t["total_ms"] > 0
    out.close()
    g.close()


# ---- 3. device-resident candidates ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted(ctx):
    """A 9 kb random genome with NGG sites (and CCN sites, their '-' form) at and next to the contig ends."""
    rng = np.random.default_rng(77)
    contigs = []
    for n in (5000, 2500, 1500):
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
    yield {"contigs": contigs, "packed": packed, "gen": gen, "scaffold": fc.scaffold("SpCas9", 76)}
    gen.close()


def test_enumerated_guides_get_their_rows_where_they_lie(planted):
    gen, sc, shape = planted["gen"], planted["scaffold"], fc.SPCAS9
    plain = gen.enumerate_guides()
    codes, loci, rows = gen.enumerate_guides(fold="SpCas9", fold_scaffold=sc)
    assert codes.tobytes() == plain[0].tobytes() and loci.tobytes() == plain[1].tobytes() and len(codes) > 500
    want, want_stats, _ = fc.expected(planted["contigs"], loci_tuples(loci), shape, sc)
    assert want_stats["defined"] == len(codes)  # a candidate's site is N-free and inside its contig: the ends included
    assert rows.dtype == np.uint32 and rows.tobytes() == want.tobytes()
    by_loci, stats = gen.fold(loci, "SpCas9", sc)
    assert by_loci.tobytes() == want.tobytes() and counts(stats) == want_stats
    assert gen.fold((codes, loci), va.FOLD_SHAPES["SpCas9"], sc)[0].tobytes() == want.tobytes()  # what enumerate_guides returns, as it is
    # N x 21 + GG under the pattern enumeration: the same sites, the same rows
    found, prows = gen.enumerate_pattern("N" * 21 + "GG", (0, 20), fold="SpCas9", fold_scaffold=sc)
    assert found.loci.tobytes() == loci.tobytes() and prows.tobytes() == want.tobytes()
    assert gen.fold(found, "SpCas9", sc)[0].tobytes() == want.tobytes()
    # the fold rows come last of all, after the rows of every other family
    mh = va.MicrohomologyShape(23, 17, 30)
    both = gen.enumerate_guides(microhomology=mh, edit="CBE", fold="SpCas9", fold_scaffold=sc)
    assert len(both) == 5 and both[1].tobytes() == loci.tobytes() and both[4].tobytes() == want.tobytes()
    assert both[2].tobytes() == gen.enumerate_guides(microhomology=mh)[2].tobytes() and both[3].tobytes() == gen.enumerate_guides(edit="CBE")[2].tobytes()
    for bad in (dict(fold="Cas12a"), dict(fold_scaffold=sc), dict(max_fold_starts=3), dict(max_fold_self=3), dict(max_fold_scaffold=3),
                dict(max_fold_seed=3), dict(fold="SpCas9", max_fold_starts=33), dict(fold="SpCas9", fold_scaffold="ACGN")):
        with pytest.raises(ValueError):
            gen.enumerate_guides(**bad)
    with pytest.raises(ValueError):
        gen.enumerate_pattern("N" * 21 + "GG", (0, 20), max_fold_seed=3)


@pytest.mark.parametrize("pattern,proto,name,m", [("N" * 14 + "GG", (2, 12), "n12_site16", 32), ("TTTV" + "N" * 23, (4, 23), "Cas12a", 33),
                                                  ("N" * 30 + "GG", (0, 32), "n32_wobble", 65)], ids=["site16", "Cas12a", "site32"])
def test_pattern_candidates_at_other_site_lengths(planted, pattern, proto, name, m):
    gen = planted["gen"]
    shape, sh, sc = fc.SHAPE_OF[name], fc.va_shape(fc.SHAPE_OF[name]), fc.scaffold(name, m)
    assert len(pattern) == shape.site_len
    targets = [(0, 0, 1200), (1, 1900, 2500), (2, 0, 300)]
    plain = gen.enumerate_pattern(pattern, proto, targets=targets)
    found, rows = gen.enumerate_pattern(pattern, proto, targets=targets, fold=sh, fold_scaffold=sc)
    assert found.codes.tobytes() == plain.codes.tobytes() and found.loci.tobytes() == plain.loci.tobytes() and 30 < len(found) < 700
    want, want_stats, _ = fc.expected(planted["contigs"], loci_tuples(found.loci), shape, sc)
    assert want_stats["defined"] == len(found) and rows.tobytes() == want.tobytes()
    # the limits, through the wrapper: the survivors in input order, their rows; only the survivors are searched
    u = va.unpack_fold_row(want)
    limits = (int(np.median(u["starts"])), None, int(np.median(u["scaf_longest"])), None)
    keep = np.array([fc.keep(r, tuple(fc.NO_LIMIT if v is None else v for v in limits)) for r in want])
    assert 0 < keep.sum() < len(want)
    kw = dict(fold=sh, fold_scaffold=sc, max_fold_starts=limits[0], max_fold_scaffold=limits[2])
    kept, krows = gen.enumerate_pattern(pattern, proto, targets=targets, **kw)
    assert kept.codes.tobytes() == found.codes[keep].tobytes() and kept.loci.tobytes() == found.loci[keep].tobytes()
    assert krows.tobytes() == want[keep].tobytes()
    if name == "Cas12a":
        d_found, d_rows, d_fold = gen.design_pattern(pattern, proto, 2, targets=targets, **kw)
        assert d_found.codes.tobytes() == kept.codes.tobytes() and d_fold.tobytes() == want[keep].tobytes()
        _, all_rows = gen.design_pattern(pattern, proto, 2, targets=targets)
        assert d_rows.tobytes() == all_rows[keep].tobytes()


def test_calls_refuse_before_anything_is_written(ctx, planted, small):
    L = va.lib()
    gen, sc = planted["gen"], va.api._fold_scaffold(planted["scaffold"])
    p = va.api._enum_params("GG", "both", (0, 0), 0, 0)
    h = C.c_void_p()
    _lib.check(L.vsc_guides_enumerate(ctx._h, gen._h, None, C.byref(p), C.byref(h)), ctx._h)
    g = Guides(ctx, h)
    rows = np.full((len(g), 2), 7, dtype=np.uint32)
    ok = va.FOLD_SHAPES["SpCas9"]
    st = ok._struct()
    lim = _lib.FoldLimits(*NONE)

    def refused(code):
        return code == -22 and (rows == 7).all()

    sh27 = va.FOLD_SHAPES["Cas12a"]._struct()
    assert refused(L.vsc_guides_fold(ctx._h, gen._h, g.h, C.byref(sh27), sc, len(sc), _lib.ptr(rows), None))
    assert "site_len" in L.vsc_last_error(ctx._h).decode()
    assert g.filter_code(gen, va.FOLD_SHAPES["Cas12a"], sc, NONE)[0] == -22
    base = dict(site_len=23, spacer=(0, 20), stem=4, gc_min=2, min_loop=3, seed=(8, 12))
    arr = fc.locus_array([(0, 100, 0)])
    for kw in ({"site_len": 15, "spacer": (0, 12)}, {"site_len": 33}, {"spacer": (0, 11)}, {"spacer": (4, 20)}, {"stem": 2}, {"stem": 9}, {"gc_min": 5},
               {"min_loop": 17}, {"seed": (17, 0)}, {"seed": (0, 17)}, {"seed": (9, 12)}, {"flags": 2}):  # every shape refusal, by the library
        sh = va.FoldShape(validate=False, **dict(base, **kw))
        bad = sh._struct()
        assert refused(L.vsc_guides_fold(ctx._h, gen._h, g.h, C.byref(bad), sc, len(sc), _lib.ptr(rows), None)), kw
        code, out = g.filter_code(gen, sh, sc, NONE)
        assert code == -22 and not out.value
        assert refused(L.vsc_loci_fold(ctx._h, gen._h, _lib.ptr(arr), 1, C.byref(bad), sc, len(sc), _lib.ptr(rows), None)), kw
    for k in range(3):
        reserved = ok._struct()
        reserved.reserved[k] = 1
        assert refused(L.vsc_guides_fold(ctx._h, gen._h, g.h, C.byref(reserved), sc, len(sc), _lib.ptr(rows), None))
    assert refused(L.vsc_guides_fold(ctx._h, gen._h, g.h, C.byref(st), b"A" * 129, 129, _lib.ptr(rows), None))  # m > 128
    assert "128" in L.vsc_last_error(ctx._h).decode()
    assert refused(L.vsc_guides_fold(ctx._h, gen._h, g.h, C.byref(st), b"ACGN", 4, _lib.ptr(rows), None))       # a bad scaffold letter
    assert refused(L.vsc_guides_fold(ctx._h, gen._h, g.h, C.byref(st), None, 4, _lib.ptr(rows), None))
    assert g.filter_code(gen, ok, b"ACGN", NONE)[0] == -22 and g.filter_code(gen, ok, b"A" * 129, NONE)[0] == -22
    for at in range(4):  # a limit in 33 .. 0xFFFFFFFE
        for v in (33, 0xFFFFFFFE):
            limits = list(NONE)
            limits[at] = v
            code, out = g.filter_code(gen, ok, sc, limits)
            assert code == -22 and not out.value and "limit" in L.vsc_last_error(ctx._h).decode()
    assert refused(L.vsc_guides_fold(ctx._h, gen._h, g.h, None, sc, len(sc), _lib.ptr(rows), None))  # null arguments
    assert L.vsc_guides_fold(ctx._h, gen._h, g.h, C.byref(st), sc, len(sc), None, None) == -22
    assert refused(L.vsc_guides_fold(ctx._h, None, g.h, C.byref(st), sc, len(sc), _lib.ptr(rows), None))
    assert refused(L.vsc_guides_fold(ctx._h, gen._h, None, C.byref(st), sc, len(sc), _lib.ptr(rows), None))
    assert L.vsc_guides_filter_fold(ctx._h, gen._h, g.h, C.byref(st), sc, len(sc), C.byref(lim), None) == -22
    out = C.c_void_p()
    assert L.vsc_guides_filter_fold(ctx._h, gen._h, g.h, C.byref(st), sc, len(sc), None, C.byref(out)) == -22 and not out.value
    assert refused(L.vsc_loci_fold(ctx._h, gen._h, None, 1, C.byref(st), sc, len(sc), _lib.ptr(rows), None))
    other = va.Context(0)  # a genome, or an object, of another context is refused
    assert refused(L.vsc_loci_fold(other._h, gen._h, _lib.ptr(arr), 1, C.byref(st), sc, len(sc), _lib.ptr(rows), None))
    s = small("SpCas9", 76)
    gen2 = other.load_genome(s["packed"])
    assert refused(L.vsc_guides_fold(other._h, gen2._h, g.h, C.byref(st), sc, len(sc), _lib.ptr(rows), None))
    assert "another context" in L.vsc_last_error(other._h).decode()
    assert L.vsc_guides_filter_fold(other._h, gen2._h, g.h, C.byref(st), sc, len(sc), C.byref(lim), C.byref(out)) == -22 and not out.value
    gen2.close()
    other.close()
    with pytest.raises(va.VarscotError):
        gen.fold(arr, va.FoldShape(validate=False, **dict(base, stem=9)))
    g.close()


# ---- 4. the filter --------------------------------------------------------------------------------------------------------------
def test_filter_limits_and_what_takes_the_result(ctx, small, planted):
    s = small("SpCas9", 76)
    sh, sc = s["sh"], s["scaffold"]
    want, _, _ = small.want("SpCas9", 76)
    defined = want[:, 0] != fc.UNDEF
    u = va.unpack_fold_row(want)
    n = len(s["loci"])
    codes = np.arange(n, dtype=np.uint64) * np.uint64(5)
    g = Guides.from_arrays(ctx, codes, s["arr"])
    kept_by = {}
    med = [int(np.median(u[k][defined])) for k in ("starts", "self_longest", "scaf_longest", "seed_paired")]
    trials = [NONE, (0,) * 4, (32,) * 4, tuple(med)]
    for at in range(4):  # each limit alone: at 0, at the median, one below it
        for v in {0, med[at], max(med[at] - 1, 0)}:
            trials.append(tuple(v if k == at else fc.NO_LIMIT for k in range(4)))
    for limits in trials:
        keep = np.array([fc.keep(r, limits) for r in want])
        out = g.filter(s["gen"], sh, sc, limits)
        got_codes, got_loci = out.arrays()
        out.close()
        assert got_codes.tobytes() == codes[keep].tobytes() and got_loci.tobytes() == s["arr"][keep].tobytes(), limits
        kept_by[limits] = keep
    assert kept_by[NONE].sum() == defined.sum() == kept_by[(32,) * 4].sum() and 0 < kept_by[tuple(med)].sum() < defined.sum()
    assert 0 < kept_by[(0, fc.NO_LIMIT, fc.NO_LIMIT, fc.NO_LIMIT)].sum() < kept_by[tuple(med)].sum() + 1  # a limit of 0: no stem start at all
    assert kept_by[(0,) * 4].sum() == ((want == 0).all(axis=1)).sum()
    for at in range(4):
        alone = tuple(med[at] if k == at else fc.NO_LIMIT for k in range(4))
        assert kept_by[tuple(med)].sum() <= kept_by[alone].sum() < defined.sum()
    # an empty result is a result; the host-only object goes the host's way, to the same bytes
    none = Guides.from_arrays(ctx, codes[~defined], s["arr"][~defined])
    empty = none.filter(s["gen"], sh, sc, NONE)
    assert len(empty) == 0 and empty.fold(s["gen"], sh, sc)[0].shape == (0, 2)
    empty.close()
    none.close()
    host = Guides.from_arrays(ctx, codes, s["arr"], on_device=False)
    h_rows, h_stats = host.fold(s["gen"], sh, sc)
    assert h_rows.tobytes() == want.tobytes() and h_stats["defined"] == defined.sum()
    h_out = host.filter(s["gen"], sh, sc, tuple(med))
    assert h_out.arrays()[0].tobytes() == codes[kept_by[tuple(med)]].tobytes()
    h_out.close()
    host.close()
    g.close()

    # the survivors feed the search as the candidates selected on the host do, and the pick by "fold"
    gen, psc = planted["gen"], planted["scaffold"]
    pcodes, ploci, prows = gen.enumerate_guides(fold="SpCas9", fold_scaffold=psc)
    pu = va.unpack_fold_row(prows)
    lim = (int(np.median(pu["starts"])), None, None, int(np.median(pu["seed_paired"])))
    keep = np.array([fc.keep(r, tuple(fc.NO_LIMIT if v is None else v for v in lim)) for r in prows])
    assert 0 < keep.sum() < len(keep)
    kw = dict(fold="SpCas9", fold_scaffold=psc, max_fold_starts=lim[0], max_fold_seed=lim[3])
    k_codes, k_loci, k_rows = gen.enumerate_guides(**kw)
    assert k_codes.tobytes() == pcodes[keep].tobytes() and k_loci.tobytes() == ploci[keep].tobytes() and k_rows.tobytes() == prows[keep].tobytes()
    rows_all = gen.summarize(pcodes, 2, exclude=ploci)
    assert gen.summarize(k_codes, 2, exclude=k_loci).tobytes() == rows_all[keep].tobytes()
    d = gen.design(None, 2, **kw)
    assert len(d) == 4 and d[0].tobytes() == k_codes.tobytes() and d[2].tobytes() == rows_all[keep].tobytes() and d[3].tobytes() == k_rows.tobytes()
    plain = gen.design(None, 2)
    assert len(plain) == 3 and plain[2].tobytes() == rows_all.tobytes()  # without the arguments: what it returned before
    iv = [(0, 0, 1500), (0, 2000, 4000), (1, 0, 2500), (2, 100, 1400)]
    regions = va.Regions(planted["packed"], iv, rule="inside")
    pick = va.PickShape(k=3, spacing=10)
    out = gen.design(regions, 2, fold="SpCas9", fold_scaffold=psc, pick=pick, pick_by=["fold", "mit"])
    r_codes, r_loci, r_rows, r_fold, picks, n_picked = out
    spec = np.array([va.mit_specificity(x) for x in r_rows["mit_sum"]], dtype=np.float64)
    key = va.pick_key([va.pick_column("fold", r_fold), va.pick_column("mit", spec)], [va.PICK_COLUMNS["fold"], va.PICK_COLUMNS["mit"]])
    w_picks, w_counts, _ = gen.pick((r_codes, r_loci), key, pick, regions=regions)
    assert picks.tobytes() == w_picks.tobytes() and n_picked.tobytes() == w_counts.tobytes() and (n_picked > 0).all()
    labels = np.array([regions.locate(c, p) for c, p, _ in loci_tuples(r_loci)])
    ru = va.unpack_fold_row(r_fold)
    assert len(set(ru["starts"].tolist())) >= 3
    for t, i in enumerate(picks[:, 0]):  # fewer is better: the first pick of every target has the fewest stems of its target
        assert labels[i] == t and ru["starts"][i] == ru["starts"][labels == t].min()
    with pytest.raises(ValueError):
        gen.design(regions, 2, pick=pick, pick_by=["fold"])  # the column needs fold=
    regions.close()


# ---- 5. repetition and the context's state ------------------------------------------------------------------------------------
def test_alternating_shapes_and_scaffolds_leave_nothing_behind(ctx, small):
    a, b = small("SpCas9", 76), small("SpCas9_wobble", 31)
    assert a["contigs"] != b["contigs"]
    gen, arr, n = a["gen"], a["arr"], len(a["loci"])
    calls = [(fc.SPCAS9, fc.scaffold("SpCas9", 76)), (fc.SPCAS9, fc.scaffold("SpCas9_wobble", 31)), (fc.SPCAS9, ""),
             (fc.SHAPE_OF["SpCas9_wobble"], fc.scaffold("SpCas9", 76)), (fc.SHAPE_OF["no_seed"], fc.scaffold("no_seed", 33))]
    want = {c: fc.expected(a["contigs"], a["loci"], c[0], c[1])[0] for c in calls}
    assert len({w.tobytes() for w in want.values()}) == len(calls)
    for k in (0, 0, 1, 0, 2, 2, 3, 1, 4, 2, 0):  # nothing of a call outlives it: no stale scaffold, no stale shape
        shape, sc = calls[k]
        assert gen.fold(arr, fc.va_shape(shape), sc)[0].tobytes() == want[calls[k]].tobytes(), k
    # an efficiency call between two fold calls finds its model again, and the fold call its scaffold
    import efficiency_cases as ec
    model = ec.build("dense", (6, 23, 6))
    lin0 = gen.efficiency(arr, model)[0]
    assert gen.fold(arr, fc.va_shape(calls[0][0]), calls[0][1])[0].tobytes() == want[calls[0]].tobytes()
    assert gen.efficiency(arr, model)[0].view(np.uint64).tobytes() == lin0.view(np.uint64).tobytes()
    ctx.release_scratch()
    assert gen.fold(arr, fc.va_shape(calls[1][0]), calls[1][1])[0].tobytes() == want[calls[1]].tobytes()
    ctx.release_scratch()
    got, stats = gen.fold(arr, fc.va_shape(calls[3][0]), calls[3][1])
    assert got.tobytes() == want[calls[3]].tobytes()
    assert stats["kernel_ms"] > 0 and stats["wall_ms"] >= stats["kernel_ms"]
    t = ctx.timing()
    assert t["score_ms"] > 0 and t["total_ms"] == t["score_ms"] and t["sites"] == n and t["genome_bytes"] == 24 * n
    for k in ("scan_ms", "prep_ms", "sort_ms", "finalize_ms", "index_ms", "pairs", "hits", "passes", "sort_bytes", "sort_levels", "list_entries"):
        assert t[k] == 0, k


# ---- 6. the tools end to end --------------------------------------------------------------------------------------------------
def test_tools_list_and_filter_their_guides(ctx, tmp_path):
    rng = np.random.default_rng(83)
    contigs = [random_seq(rng, 6000), "TTTA" + random_seq(rng, 2996)]
    names = ["chr1 assembled", "chr2"]
    chrom = [n.split()[0] for n in names]
    with open(tmp_path / "g.fa", "w") as f:
        for n, s in zip(names, contigs):
            f.write(">%s\n%s\n" % (n, "\n".join(s[i:i + 60] for i in range(0, len(s), 60))))
    iv = [(0, 0, 900), (1, 100, 400), (0, 5800, 6000)]
    (tmp_path / "t.bed").write_text("".join("%s\t%d\t%d\tx\n" % (chrom[c], a, b) for c, a, b in iv))
    run = lambda *a: subprocess.run([os.path.join(BIN, a[0])] + [str(x) for x in a[1:]], capture_output=True, text=True, timeout=600)  # noqa: E731
    assert run("bidir_index", "-G", tmp_path / "g.fa", "-I", tmp_path / "idx").returncode == 0
    packed = va.PackedGenome.from_sequences(contigs)
    gen = ctx.load_genome(packed)
    sc = fc.letters(fc.scaffold("SpCas9", 76)).replace("T", "U")
    (tmp_path / "scaffold.txt").write_text("\n".join(sc[i:i + 30] for i in range(0, len(sc), 30)) + "\n")

    def columns(rows):
        u = va.unpack_fold_row(rows)
        return ["\t%d\t%d\t%d\t%d" % (u["starts"][i], u["self_longest"][i], u["scaf_longest"][i], u["seed_paired"][i]) for i in range(len(rows))]

    # guide_summary -E -L --fold [--fold-scaffold] [--max-fold]
    regions = va.Regions(packed, iv, rule="inside")
    codes, loci, rows = gen.enumerate_guides(regions, fold="SpCas9", fold_scaffold=sc)
    u = va.unpack_fold_row(rows)
    assert 50 < len(codes) < 500 and u["defined"].all() and (u["scaf_starts"] > 0).any()
    lim = (int(np.median(u["starts"])), fc.NO_LIMIT, int(np.median(u["scaf_longest"])), fc.NO_LIMIT)
    keep = np.array([fc.keep(r, lim) for r in rows])
    assert 0 < keep.sum() < len(keep)
    base = ("guide_summary", "-G", tmp_path / "g.fa", "-I", tmp_path / "idx", "-M", "2", "-E", tmp_path / "t.bed")
    r = run(*base, "-L", tmp_path / "plain.bed", "-O", tmp_path / "plain.tsv")
    assert r.returncode == 0, r.stderr
    r = run(*base, "-L", tmp_path / "f.bed", "-O", tmp_path / "f.tsv", "--fold", "SpCas9", "--fold-scaffold", sc)
    assert r.returncode == 0, r.stderr
    plain_bed = (tmp_path / "plain.bed").read_text().splitlines()
    plain_rows = (tmp_path / "plain.tsv").read_text().splitlines()
    assert len(plain_bed) == len(codes)
    assert (tmp_path / "f.tsv").read_bytes() == (tmp_path / "plain.tsv").read_bytes()  # --fold adds to the listing alone
    want_bed = [ln + col for ln, col in zip(plain_bed, columns(rows))]
    assert (tmp_path / "f.bed").read_text().splitlines() == want_bed
    r = run(*base, "-L", tmp_path / "ff.bed", "-O", tmp_path / "ff.tsv", "--fold", "23,0,20,4,2,3,8,12,0", "--fold-scaffold", "@%s" % (tmp_path / "scaffold.txt"))
    assert r.returncode == 0 and (tmp_path / "ff.bed").read_bytes() == (tmp_path / "f.bed").read_bytes()  # the preset as a SPEC, the text from a file
    r = run(*base, "-L", tmp_path / "k.bed", "-O", tmp_path / "k.tsv", "--fold", "SpCas9", "--fold-scaffold", sc, "--max-fold", "%d,-,%d" % (lim[0], lim[2]))
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "k.bed").read_text().splitlines() == [ln for ln, k in zip(want_bed, keep) if k]
    assert (tmp_path / "k.tsv").read_text().splitlines() == [plain_rows[0]] + [ln for ln, k in zip(plain_rows[1:], keep) if k]
    r = run(*base, "-L", tmp_path / "e.bed", "-O", tmp_path / "e.tsv", "--fold", "SpCas9")  # no scaffold: m = 0
    none = gen.enumerate_guides(regions, fold="SpCas9")[2]
    assert r.returncode == 0 and (tmp_path / "e.bed").read_text().splitlines() == [ln + col for ln, col in zip(plain_bed, columns(none))]
    assert not va.unpack_fold_row(none)["scaf_longest"].any()
    regions.close()

    # pattern_search -E --fold: Cas12a
    pattern, proto = "TTTV" + "N" * 23, (4, 23)
    targets = [(0, 0, 3000), (1, 0, 3000)]
    (tmp_path / "p.bed").write_text("".join("%s\t%d\t%d\n" % (chrom[c], a, b) for c, a, b in targets))
    dr = "AAUUUCUACUCUUGUAGAU"
    found, prows = gen.enumerate_pattern(pattern, proto, targets=targets, fold="Cas12a", fold_scaffold=dr)
    pu = va.unpack_fold_row(prows)
    plim = (int(np.median(pu["starts"])), int(np.median(pu["self_longest"])), fc.NO_LIMIT, fc.NO_LIMIT)
    pkeep = np.array([fc.keep(r, plim) for r in prows])
    assert len(found) > 40 and 0 < pkeep.sum() < len(pkeep)
    pbase = ("pattern_search", "-i", tmp_path / "idx", "-q", pattern, "-p", "%d,%d" % proto, "-B", tmp_path / "p.bed", "-M", "2")
    r = run(*pbase, "-E", tmp_path / "pe.tsv", "-O", tmp_path / "po.tsv")
    assert r.returncode == 0, r.stderr
    r = run(*pbase, "-E", tmp_path / "pef.tsv", "-O", tmp_path / "pof.tsv", "--fold", "Cas12a", "--fold-scaffold", dr)
    assert r.returncode == 0, r.stderr
    pe = (tmp_path / "pe.tsv").read_text().splitlines()
    po = (tmp_path / "po.tsv").read_text().splitlines()
    assert len(pe) == len(found) + 1 and pe[0] == "#guide\tchrom\tpos\tstrand"
    assert (tmp_path / "pof.tsv").read_bytes() == (tmp_path / "po.tsv").read_bytes()
    want_pe = [pe[0] + "\tfoldStarts\tfoldSelf\tfoldScaffold\tfoldSeed"] + [ln + col for ln, col in zip(pe[1:], columns(prows))]
    assert (tmp_path / "pef.tsv").read_text().splitlines() == want_pe
    r = run(*pbase, "-E", tmp_path / "pek.tsv", "-O", tmp_path / "pok.tsv", "--fold", "Cas12a", "--fold-scaffold", dr, "--max-fold", "%d,%d" % plim[:2])
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "pek.tsv").read_text().splitlines() == [want_pe[0]] + [ln for ln, k in zip(want_pe[1:], pkeep) if k]
    assert (tmp_path / "pok.tsv").read_text().splitlines() == [po[0]] + [ln for ln, k in zip(po[1:], pkeep) if k]
    gen.close()
