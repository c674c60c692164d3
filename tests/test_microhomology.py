"""The microhomology score on the device (vsc_loci_microhomology, vsc_guides_microhomology, vsc_pattern_guides_microhomology
and the two filters): bit for bit what the definition gives when it is applied locus by locus in plain Python as the ROW LIST
(tests/microhomology_cases.py).  Integers, so there is no tolerance: the pairs are compared as uint32, the undefined pair
included."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import efficiency_cases as ec
import microhomology_cases as mc
import varscot_amd as va
import wide_cases as wc
from helpers import random_seq, revcomp
from varscot_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "varscot_amd", "bin")
FILTER_TILE = 1024  # candidates per wave of the filter's passes (include/varscot_hip.h)
DROP_FRONT, DROP_BACK = 3, 1  # words the partial object of the small genome does not hold


@pytest.fixture(scope="module")
def ctx():
    c = va.Context(0)
    yield c
    c.close()


def shape_of(t):
    return va.MicrohomologyShape(site_len=t[0], cut=t[1], flank=t[2])


def loci_tuples(loci):
    return [(int(c), int(p), int(s)) for c, p, s in zip(loci["contig"], loci["pos"], loci["strand"])]


class Guides:
    """A vsc_guides (or, pattern=True, a vsc_pattern_guides) handle and its calls."""

    def __init__(self, ctx, handle, pattern=False):
        self.ctx, self.h, self.pattern = ctx, handle, pattern
        L = va.lib()
        kind = "vsc_pattern_guides" if pattern else "vsc_guides"
        self.fn = {k: getattr(L, "%s_%s" % (kind, k)) for k in ("count", "data", "free", "microhomology", "filter_microhomology",
                                                                 "filter_efficiency")}

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

    def microhomology(self, gen, shape):
        pairs, st = np.empty((len(self), 2), dtype=np.uint32), _lib.MhStats()
        sh = shape._struct()
        _lib.check(self.fn["microhomology"](self.ctx._h, gen._h, self.h, C.byref(sh), _lib.ptr(pairs), C.byref(st)), self.ctx._h)
        return pairs, st.as_dict()

    def filter_code(self, gen, shape, min_sum, permille):
        out = C.c_void_p()
        sh = shape._struct()
        return self.fn["filter_microhomology"](self.ctx._h, gen._h, self.h, C.byref(sh), min_sum, permille, C.byref(out)), out

    def filter(self, gen, shape, min_sum, permille):
        code, out = self.filter_code(gen, shape, min_sum, permille)
        _lib.check(code, self.ctx._h)
        return Guides(self.ctx, out, self.pattern)

    def filter_efficiency(self, gen, model, floor):
        out = C.c_void_p()
        _lib.check(self.fn["filter_efficiency"](self.ctx._h, gen._h, self.h, model._h, floor, C.byref(out)), self.ctx._h)
        return Guides(self.ctx, out, self.pattern)

    def close(self):
        if self.h:
            self.fn["free"](self.h)
            self.h = None


def counts(stats):
    return {k: stats[k] for k in mc.CLASSES}


# ---- 1. every locus of the small genome ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(ctx):
    """Per flank: the small genome resident - whole, and as an object that lacks the first three words and the last one -
    every locus of it, and per shape the expected pairs, computed once."""
    cache = {}

    def get(F):
        if F not in cache:
            contigs = mc.small_genome(F)
            packed = va.PackedGenome.from_sequences(list(contigs))
            loci = mc.every_locus(contigs)
            sl = slice(DROP_FRONT, packed.n_words - DROP_BACK)
            part = va.Genome.from_shard(ctx, packed.hi[sl], packed.lo[sl], packed.nmask[sl], DROP_FRONT, sl.stop - sl.start, packed.contigs)
            cache[F] = {"contigs": contigs, "packed": packed, "gen": ctx.load_genome(packed), "part": part, "loci": loci,
                        "arr": mc.locus_array(loci), "resident": (32 * sl.start, 32 * sl.stop), "want": {}}
        return cache[F]

    def want(shape, partial=False):
        s = get(shape[2])
        key = (shape, partial)
        if key not in s["want"]:
            s["want"][key] = mc.expected(s["contigs"], s["loci"], shape, s["resident"] if partial else None)
        return s["want"][key]

    get.want = want
    yield get
    for s in cache.values():
        s["gen"].close()
        s["part"].close()


@pytest.mark.parametrize("cut", [0, 17, mc.SITE_LEN])
@pytest.mark.parametrize("F", [8, 30, 32])
def test_every_locus_of_a_small_genome(small, F, cut):
    shape = (mc.SITE_LEN, cut, F)
    s = small(F)
    want, want_stats, texts = small.want(shape, partial=True)
    # what the fixture is for, on the restatement alone
    assert all(want_stats[k] >= 5 for k in mc.CLASSES), want_stats
    defined = want[:, 0] != mc.UNDEF
    assert (want[defined, 0] > 0).sum() >= 50
    for strand in (0, 1):  # the d = F quirk: the left half repeated as the right half
        assert any(t is not None and l[2] == strand and t[:F] == t[F:] for l, t in zip(s["loci"], texts))
    assert (defined & (want[:, 1] == 0) & (want[:, 0] > 0)).any() and (defined & (want[:, 1] == want[:, 0]) & (want[:, 0] > 0)).any()
    assert (defined & (want[:, 0] == 0)).any()
    got, stats = s["part"].microhomology(s["arr"], shape_of(shape), allow_partial=True)
    assert got.dtype == np.uint32 and got.shape == want.shape
    assert counts(stats) == want_stats and sum(want_stats.values()) == len(s["loci"])
    assert got.tobytes() == want.tobytes()
    # the whole genome: nothing is missing, and what was resident scores the same
    whole, whole_stats, _ = small.want(shape)
    got, stats = s["gen"].microhomology(s["arr"], shape_of(shape))
    assert counts(stats) == whole_stats and stats["not_resident"] == 0 and got.tobytes() == whole.tobytes()
    assert (whole[defined] == want[defined]).all()


def test_invalid_loci_are_classed_and_never_followed(small):
    s = small(30)
    n_contigs, main = len(s["contigs"]), 5
    length = len(s["contigs"][main])
    bad = [(n_contigs, 0, 0), (0xFFFFFFFF, 0, 0), (0xFFFFFFFF, 0xFFFFFFFF, 1), (main, 10, 2), (main, 10, 0xFFFFFFFF), (main, length - 22, 0),
           (main, length - 22, 1), (main, 0xFFFFFFFF, 0), (main + 1, 0xFFFFFFFF, 1), (0, 7, 0), (main, 0xFFFFFFFF - 22, 0)]
    loci = bad + [(main, 200, 0)]
    for cut in (0, 17, 23):
        want, want_stats, _ = mc.expected(s["contigs"], loci, (23, cut, 30))
        assert want_stats["invalid"] == len(bad) and want_stats["defined"] == 1
        got, stats = s["gen"].microhomology(mc.locus_array(loci), shape_of((23, cut, 30)))
        assert counts(stats) == want_stats and got.tobytes() == want.tobytes() and (got[:-1] == mc.UNDEF).all()


def test_nothing_to_score(ctx, small):
    got, stats = small(8)["gen"].microhomology(mc.locus_array([]), shape_of((23, 17, 8)))
    assert got.shape == (0, 2) and counts(stats) == dict.fromkeys(mc.CLASSES, 0)
    t = ctx.timing()
    assert t["sites"] == 0 and t["score_ms"] == 0 and t["total_ms"] == 0 and t["genome_bytes"] == 0


# ---- 2. more candidates than one launch has lanes, more tiles than it has waves -----------------------------------------------
def launch_waves():
    """The waves of a launch capped as the cells' grids are (wide_cases): CUs x 8 workgroups of 4 waves."""
    return torch.cuda.get_device_properties(0).multi_processor_count * wc.GROUPS_PER_CU * wc.WAVES_PER_GROUP


def test_more_candidates_than_a_launch_has_lanes(small):
    shape = (23, 17, 30)
    s = small(30)
    want, _, _ = small.want(shape, partial=True)
    n, m = launch_waves() * 64 + 77, len(s["loci"])
    assert n > 3 * m  # every lane meets more than one tiling of the loci
    idx = np.arange(n) % m
    got, stats = s["part"].microhomology(s["arr"][idx], shape_of(shape), allow_partial=True)
    assert got.tobytes() == want[idx].tobytes()
    cls = np.array([mc.classify(s["contigs"], l, shape, s["resident"])[0] for l in s["loci"]])[idx]
    per = {k: int(v) for k, v in zip(*np.unique(cls, return_counts=True))}
    assert counts(stats) == {k: per.get(k, 0) for k in mc.CLASSES} and sum(counts(stats).values()) == n


def test_filter_over_more_tiles_than_a_launch_has_waves(ctx, small):
    shape = (23, 17, 30)
    s = small(30)
    want, _, _ = small.want(shape)
    m = len(s["loci"])
    n = (launch_waves() + 3) * FILTER_TILE + 77  # the last tile is a partial one
    idx = np.arange(n) % m
    defined = want[:, 0] != mc.UNDEF
    min_sum = int(np.median(want[defined, 0]))
    keep = np.array([mc.keep(p, min_sum, 500) for p in want])
    assert 0 < keep.sum() < defined.sum()
    codes = np.arange(n, dtype=np.uint64) * np.uint64(3)  # (the filter copies codes, it does not read them)
    g = Guides.from_arrays(ctx, codes, s["arr"][idx])
    out = g.filter(s["gen"], shape_of(shape), min_sum, 500)
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


@pytest.mark.parametrize("F", [8, 30])
def test_enumerated_guides_are_scored_where_they_lie(planted, F):
    shape = (23, 17, F)
    gen, sh = planted["gen"], shape_of(shape)
    plain = gen.enumerate_guides()
    codes, loci, pairs = gen.enumerate_guides(microhomology=sh)
    assert codes.tobytes() == plain[0].tobytes() and loci.tobytes() == plain[1].tobytes() and len(codes) > 1000
    want, want_stats, _ = mc.expected(planted["contigs"], loci_tuples(loci), shape)
    assert want_stats["off_contig"] >= 2 and want_stats["defined"] > 1000  # the planted sites next to the ends have no context
    assert pairs.dtype == np.uint32 and pairs.tobytes() == want.tobytes()
    by_loci, stats = gen.microhomology(loci, sh)
    assert by_loci.tobytes() == want.tobytes() and counts(stats) == want_stats
    assert gen.microhomology((codes, loci), sh)[0].tobytes() == want.tobytes()  # what enumerate_guides returns, as it is
    # N x 21 + GG under the pattern enumeration: the same sites, the same pairs
    found, ppairs = gen.enumerate_pattern("N" * 21 + "GG", (0, 20), microhomology=sh)
    assert found.loci.tobytes() == loci.tobytes() and ppairs.tobytes() == want.tobytes()
    assert gen.microhomology(found, sh)[0].tobytes() == want.tobytes()
    with pytest.raises(ValueError):
        gen.enumerate_guides(microhomology=va.MicrohomologyShape(site_len=27))  # site_len 27 is not these candidates'
    with pytest.raises(ValueError):
        gen.enumerate_guides(min_out_of_frame=50)
    with pytest.raises(ValueError):
        gen.enumerate_guides(min_microhomology=1.0)


@pytest.mark.parametrize("pattern,proto,cut", [("N" * 21 + "NNGRRT", (0, 21), 18), ("TTTV" + "N" * 23, (4, 23), 22)],
                         ids=["SaCas9", "Cas12a"])
def test_pattern_candidates_of_other_nucleases(planted, pattern, proto, cut):
    gen = planted["gen"]
    shape = (len(pattern), cut, 30)
    sh = shape_of(shape)
    plain = gen.enumerate_pattern(pattern, proto)
    found, pairs = gen.enumerate_pattern(pattern, proto, microhomology=sh)
    assert found.codes.tobytes() == plain.codes.tobytes() and found.loci.tobytes() == plain.loci.tobytes() and len(found) > 100
    want, want_stats, _ = mc.expected(planted["contigs"], loci_tuples(found.loci), shape)
    assert want_stats["defined"] > 100 and pairs.tobytes() == want.tobytes()
    # the floors, through the wrapper: the survivors in input order, their pairs; only the survivors are searched
    min_mh = float(np.median(want[want[:, 0] != mc.UNDEF, 0])) / 10
    keep = np.array([mc.keep(p, int(np.ceil(10 * min_mh - 1e-9)), 600) for p in want])
    assert 0 < keep.sum() < len(want)
    kept, kpairs = gen.enumerate_pattern(pattern, proto, microhomology=sh, min_out_of_frame=60, min_microhomology=min_mh)
    assert kept.codes.tobytes() == found.codes[keep].tobytes() and kept.loci.tobytes() == found.loci[keep].tobytes()
    assert kpairs.tobytes() == want[keep].tobytes()
    d_found, d_rows, d_pairs = gen.design_pattern(pattern, proto, 2, microhomology=sh, min_out_of_frame=60, min_microhomology=min_mh)
    assert d_found.codes.tobytes() == kept.codes.tobytes() and d_pairs.tobytes() == want[keep].tobytes()
    _, all_rows = gen.design_pattern(pattern, proto, 2)
    assert d_rows.tobytes() == all_rows[keep].tobytes()
    # search_pattern takes the filter's result unchanged
    _, rows = gen.search_pattern(pattern, kept.text(), 2, records=False)
    _, rows_all = gen.search_pattern(pattern, found.text(), 2, records=False)
    assert rows.tobytes() == rows_all[keep].tobytes()


def test_calls_refuse_what_the_efficiency_calls_refuse(ctx, planted, small):
    L = va.lib()
    gen = planted["gen"]
    p = va.api._enum_params("GG", "both", (0, 0), 0, 0)
    h = C.c_void_p()
    _lib.check(L.vsc_guides_enumerate(ctx._h, gen._h, None, C.byref(p), C.byref(h)), ctx._h)
    g = Guides(ctx, h)
    pairs = np.empty((len(g), 2), dtype=np.uint32)
    sh27 = va.MicrohomologyShape(site_len=27)._struct()
    assert L.vsc_guides_microhomology(ctx._h, gen._h, g.h, C.byref(sh27), _lib.ptr(pairs), None) == -22
    assert "site_len" in L.vsc_last_error(ctx._h).decode()
    assert g.filter_code(gen, va.MicrohomologyShape(site_len=27), 0, 0)[0] == -22
    for bad in ((23, 17, 7), (23, 17, 33), (23, 24, 30), (15, 10, 30), (33, 17, 30)):  # every shape refusal, by the library
        sh = va.MicrohomologyShape(*bad, validate=False)
        st = sh._struct()
        assert L.vsc_guides_microhomology(ctx._h, gen._h, g.h, C.byref(st), _lib.ptr(pairs), None) == -22, bad
        code, out = g.filter_code(gen, sh, 0, 0)
        assert code == -22 and not out.value
        with pytest.raises(va.VarscotError):
            gen.microhomology(mc.locus_array([(0, 100, 0)]), sh)
    reserved = _lib.MhShape(23, 17, 30, 1)
    assert L.vsc_guides_microhomology(ctx._h, gen._h, g.h, C.byref(reserved), _lib.ptr(pairs), None) == -22
    ok = va.MicrohomologyShape()
    st = ok._struct()
    assert L.vsc_guides_microhomology(ctx._h, gen._h, g.h, None, _lib.ptr(pairs), None) == -22  # null arguments
    assert L.vsc_guides_microhomology(ctx._h, gen._h, g.h, C.byref(st), None, None) == -22
    assert L.vsc_guides_microhomology(ctx._h, None, g.h, C.byref(st), _lib.ptr(pairs), None) == -22
    assert L.vsc_guides_microhomology(ctx._h, gen._h, None, C.byref(st), _lib.ptr(pairs), None) == -22
    assert L.vsc_guides_filter_microhomology(ctx._h, gen._h, g.h, C.byref(st), 0, 0, None) == -22
    code, out = g.filter_code(gen, ok, 0, 1001)
    assert code == -22 and not out.value and "1000" in L.vsc_last_error(ctx._h).decode()
    arr = mc.locus_array([(0, 100, 0)])
    assert L.vsc_loci_microhomology(ctx._h, gen._h, None, 1, C.byref(st), _lib.ptr(pairs), None) == -22
    other = va.Context(0)  # a genome of another context is refused
    assert L.vsc_loci_microhomology(other._h, gen._h, _lib.ptr(arr), 1, C.byref(st), _lib.ptr(pairs), None) == -22
    other.close()
    g.close()


# ---- 4. the filter --------------------------------------------------------------------------------------------------------------
def test_filter_floors_and_what_takes_the_result(ctx, small, planted):
    shape = (23, 17, 30)
    s, sh = small(30), shape_of(shape)
    want, _, texts = small.want(shape)
    defined = want[:, 0] != mc.UNDEF
    median = int(np.median(want[defined, 0]))
    # the planted 2 : 3 candidate is 666.67 per mille: FILTER keeps it at 666 and drops it at 667 (2000 < 2001)
    at = [i for i, t in enumerate(texts) if t == mc.two_thirds()]
    assert at and all(3 * int(want[i, 1]) == 2 * int(want[i, 0]) > 0 for i in at)
    zero = defined & (want[:, 0] == 0)
    assert zero.sum() >= 5
    n = len(s["loci"])
    codes = np.arange(n, dtype=np.uint64) * np.uint64(5)
    g = Guides.from_arrays(ctx, codes, s["arr"])
    kept_by = {}
    for permille in (0, 500, 666, 667, 1000):
        for min_sum in (0, 1, median):
            keep = np.array([mc.keep(p, min_sum, permille) for p in want])
            out = g.filter(s["gen"], sh, min_sum, permille)
            got_codes, got_loci = out.arrays()
            out.close()
            assert got_codes.tobytes() == codes[keep].tobytes() and got_loci.tobytes() == s["arr"][keep].tobytes(), (permille, min_sum)
            kept_by[permille, min_sum] = keep
    assert kept_by[0, 0].sum() == defined.sum() and 0 < kept_by[1000, 1].sum() < kept_by[500, 0].sum() < defined.sum()
    assert all(kept_by[666, 0][i] and not kept_by[667, 0][i] for i in at)
    assert kept_by[0, 0][zero].all() and not kept_by[0, 1][zero].any() and not kept_by[500, 0][zero].any()  # sum == 0: only at 0 per mille
    # an empty result is a result; the host-only object goes the host's way, to the same bytes
    empty = g.filter(s["gen"], sh, 0xFFFFFFFE, 0)
    assert len(empty) == 0 and empty.microhomology(s["gen"], sh)[0].shape == (0, 2)
    empty.close()
    host = Guides.from_arrays(ctx, codes, s["arr"], on_device=False)
    h_pairs, h_stats = host.microhomology(s["gen"], sh)
    assert h_pairs.tobytes() == want.tobytes() and h_stats["defined"] == defined.sum()
    h_out = host.filter(s["gen"], sh, median, 500)
    assert h_out.arrays()[0].tobytes() == codes[kept_by[500, median]].tobytes()
    h_out.close()
    host.close()
    g.close()

    # the survivors feed the search as the candidates selected on the host do
    gen = planted["gen"]
    pcodes, ploci, ppairs = gen.enumerate_guides(microhomology=sh)
    keep = np.array([mc.keep(p, 0, 667) for p in ppairs])
    assert 0 < keep.sum() < len(keep)
    k_codes, k_loci, k_pairs = gen.enumerate_guides(microhomology=sh, min_out_of_frame=66.7)
    assert k_codes.tobytes() == pcodes[keep].tobytes() and k_loci.tobytes() == ploci[keep].tobytes() and k_pairs.tobytes() == ppairs[keep].tobytes()
    rows_all = gen.summarize(pcodes, 2, exclude=ploci)
    assert gen.summarize(k_codes, 2, exclude=k_loci).tobytes() == rows_all[keep].tobytes()
    d = gen.design(None, 2, microhomology=sh, min_out_of_frame=66.7)
    assert len(d) == 4 and d[0].tobytes() == k_codes.tobytes() and d[2].tobytes() == rows_all[keep].tobytes() and d[3].tobytes() == k_pairs.tobytes()
    plain = gen.design(None, 2)
    assert len(plain) == 3 and plain[2].tobytes() == rows_all.tobytes()  # without the arguments: what it returned before


def test_both_floors_in_either_order(ctx, planted):
    eshape, shape = (6, 23, 6), (23, 17, 30)
    gen, model, sh = planted["gen"], ec.build("dense", eshape), shape_of(shape)
    codes, loci, linear, pairs = gen.enumerate_guides(efficiency=model, microhomology=sh)
    assert linear.dtype == np.float64 and pairs.dtype == np.uint32  # the predictors, then the pairs
    defined = linear == linear
    floor = float(np.median(linear[defined]))
    keep = defined & (np.where(defined, linear, 0.0) >= floor) & np.array([mc.keep(p, 100, 600) for p in pairs])
    assert 0 < keep.sum() < (defined & (np.where(defined, linear, 0.0) >= floor)).sum()
    g = Guides.from_arrays(ctx, codes, loci)
    a1 = g.filter_efficiency(gen, model, floor)
    a2 = a1.filter(gen, sh, 100, 600)
    b1 = g.filter(gen, sh, 100, 600)
    b2 = b1.filter_efficiency(gen, model, floor)
    for x, y in zip(a2.arrays(), b2.arrays()):
        assert x.tobytes() == y.tobytes()
    assert a2.arrays()[0].tobytes() == codes[keep].tobytes() and a2.arrays()[1].tobytes() == loci[keep].tobytes()
    for h in (a1, a2, b1, b2, g):
        h.close()
    k = gen.enumerate_guides(efficiency=model, min_efficiency=floor, microhomology=sh, min_out_of_frame=60, min_microhomology=10)
    assert k[0].tobytes() == codes[keep].tobytes() and k[1].tobytes() == loci[keep].tobytes()
    assert k[2].view(np.uint64).tobytes() == linear[keep].view(np.uint64).tobytes() and k[3].tobytes() == pairs[keep].tobytes()


# ---- 5. shards ------------------------------------------------------------------------------------------------------------------
def test_a_shard_scores_what_it_holds(ctx, planted):
    shape = (23, 17, 32)
    packed, contigs, sh = planted["packed"], planted["contigs"], shape_of(shape)
    n_words = packed.n_words
    assert n_words > 200
    loci = [(0, p, s) for p in list(range(1960, 2130)) + list(range(2150, 2320)) for s in (0, 1)]
    loci += loci_tuples(planted["gen"].enumerate_guides()[1])
    arr = mc.locus_array(loci)
    whole, _, _ = mc.expected(contigs, loci, shape)
    for first, words, own in ((64, n_words - 64, n_words - 64), (0, 70, 64)):  # nothing in front of word 64; nothing behind a 6-word halo
        sl = slice(first, first + words)
        shard = va.Genome.from_shard(ctx, packed.hi[sl], packed.lo[sl], packed.nmask[sl], first, own, packed.contigs)
        want, want_stats, _ = mc.expected(contigs, loci, shape, resident=(32 * first, 32 * (first + words)))
        assert want_stats["not_resident"] > 100 and want_stats["defined"] > 100
        resident = want[:, 0] != mc.UNDEF
        assert (want[resident] == whole[resident]).all()
        with pytest.raises(ValueError) as e:
            shard.microhomology(arr, sh)
        assert "not resident" in str(e.value)
        got, stats = shard.microhomology(arr, sh, allow_partial=True)
        assert counts(stats) == want_stats and got.tobytes() == want.tobytes()
        shard.close()


# ---- 6. repetition and the context's state ------------------------------------------------------------------------------------
def test_repetition_shapes_and_timing(ctx, small):
    s = small(30)
    gen, arr, n = s["gen"], s["arr"], len(s["loci"])
    shapes = [(23, 17, 30), (23, 0, 30), (23, 23, 30)]
    want = {sh: small.want(sh)[0] for sh in shapes}
    assert len({w.tobytes() for w in want.values()}) == 3
    for sh in (shapes[0], shapes[0], shapes[1], shapes[0], shapes[2], shapes[2], shapes[1]):  # nothing of a call outlives it
        assert gen.microhomology(arr, shape_of(sh))[0].tobytes() == want[sh].tobytes()
    ctx.release_scratch()
    assert gen.microhomology(arr, shape_of(shapes[1]))[0].tobytes() == want[shapes[1]].tobytes()
    ctx.release_scratch()
    got, stats = gen.microhomology(arr, shape_of(shapes[2]))
    assert got.tobytes() == want[shapes[2]].tobytes()
    assert stats["kernel_ms"] > 0 and stats["wall_ms"] >= stats["kernel_ms"]
    t = ctx.timing()
    assert t["score_ms"] > 0 and t["total_ms"] == t["score_ms"] and t["sites"] == n and t["genome_bytes"] == 24 * n
    for k in ("scan_ms", "prep_ms", "sort_ms", "finalize_ms", "index_ms", "pairs", "hits", "passes", "sort_bytes", "sort_levels", "list_entries"):
        assert t[k] == 0, k


# ---- 7. the tools end to end --------------------------------------------------------------------------------------------------
def test_tools_score_and_filter_their_guides(ctx, tmp_path):
    rng = np.random.default_rng(82)
    contigs = [random_seq(rng, 9000), "TTTA" + random_seq(rng, 3996)]  # (a Cas12a site whose window starts in front of chr2)
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

    def columns(pairs):
        mh, oof = va.microhomology_scores(pairs)
        return ["\t" + fmt(a) + "\t" + fmt(b) for a, b in zip(mh, oof)]

    # guide_summary -E -L -H [-m]
    sh = va.MicrohomologyShape(23, 17, 30)
    regions = va.Regions(packed, iv, rule="inside")
    codes, loci, pairs = gen.enumerate_guides(regions, microhomology=sh)
    undefined = pairs[:, 0] == va.MH_UNDEFINED
    assert 50 < len(codes) < 500 and 0 < undefined.sum()
    min_mh = float(np.median(pairs[~undefined, 0])) / 10
    keep = np.array([mc.keep(p, int(np.ceil(10 * min_mh - 1e-9)), 600) for p in pairs])
    assert 0 < keep.sum() < len(keep)
    base = ("guide_summary", "-G", tmp_path / "g.fa", "-I", tmp_path / "idx", "-M", "2", "-E", tmp_path / "t.bed")
    r = run(*base, "-L", tmp_path / "plain.bed", "-O", tmp_path / "plain.tsv")
    assert r.returncode == 0, r.stderr
    r = run(*base, "-L", tmp_path / "h.bed", "-O", tmp_path / "h.tsv", "-H", "30")
    assert r.returncode == 0, r.stderr
    plain_bed = (tmp_path / "plain.bed").read_text().splitlines()
    plain_rows = (tmp_path / "plain.tsv").read_text().splitlines()
    assert len(plain_bed) == len(codes)
    assert (tmp_path / "h.tsv").read_bytes() == (tmp_path / "plain.tsv").read_bytes()  # -H adds to the listing alone
    want_bed = [ln + col for ln, col in zip(plain_bed, columns(pairs))]
    assert (tmp_path / "h.bed").read_text().splitlines() == want_bed and any(ln.endswith("\tNA\tNA") for ln in want_bed)
    r = run(*base, "-L", tmp_path / "h17.bed", "-H", "30,17", "-O", tmp_path / "h17.tsv")
    assert r.returncode == 0 and (tmp_path / "h17.bed").read_bytes() == (tmp_path / "h.bed").read_bytes()  # 17 is the default cut
    r = run(*base, "-L", tmp_path / "k.bed", "-O", tmp_path / "k.tsv", "-H", "30", "-m", "60,%r" % min_mh)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "k.bed").read_text().splitlines() == [ln for ln, k in zip(want_bed, keep) if k]
    assert (tmp_path / "k.tsv").read_text().splitlines() == [plain_rows[0]] + [ln for ln, k in zip(plain_rows[1:], keep) if k]
    for args, text in (((*base, "-m", "50"), "give -H"),
                       ((*base[:7], "-B", tmp_path / "plain.bed", "-H", "30"), "give -E"),
                       ((*base, "-H", "7"), "-H takes"), ((*base, "-H", "33"), "-H takes"), ((*base, "-H", "30,24"), "-H takes"),
                       ((*base, "-H", "wide"), "-H takes"), ((*base, "-H", "30", "-m", "101"), "-m takes"),
                       ((*base, "-H", "30", "-m", "nan"), "-m takes"), ((*base, "-H", "30", "-D", "0,0"), "one device")):
        r = run(*args)
        assert r.returncode != 0 and text in r.stderr, (args, r.stderr)
    regions.close()

    # pattern_search -E -H [-m]: Cas12a, the break 18 bases behind the protospacer's start
    pattern, proto = "TTTV" + "N" * 23, (4, 23)
    psh = va.MicrohomologyShape(27, 22, 30)
    targets = [(0, 0, 3000), (1, 0, 4000)]
    (tmp_path / "p.bed").write_text("".join("%s\t%d\t%d\n" % (chrom[c], a, b) for c, a, b in targets))
    found, ppairs = gen.enumerate_pattern(pattern, proto, targets=targets, microhomology=psh)
    pundef = ppairs[:, 0] == va.MH_UNDEFINED
    assert len(found) > 40 and 0 < pundef.sum()
    pkeep = np.array([mc.keep(p, 0, 500) for p in ppairs])
    assert 0 < pkeep.sum() < len(pkeep)
    pbase = ("pattern_search", "-i", tmp_path / "idx", "-q", pattern, "-p", "%d,%d" % proto, "-B", tmp_path / "p.bed", "-M", "2")
    r = run(*pbase, "-E", tmp_path / "pe.tsv", "-O", tmp_path / "po.tsv")
    assert r.returncode == 0, r.stderr
    r = run(*pbase, "-E", tmp_path / "peh.tsv", "-O", tmp_path / "poh.tsv", "-H", "30")
    assert r.returncode == 0, r.stderr
    pe = (tmp_path / "pe.tsv").read_text().splitlines()
    po = (tmp_path / "po.tsv").read_text().splitlines()
    assert len(pe) == len(found) + 1 and pe[0] == "#guide\tchrom\tpos\tstrand"
    assert (tmp_path / "poh.tsv").read_bytes() == (tmp_path / "po.tsv").read_bytes()
    want_pe = [pe[0] + "\tmhScore\toofScore"] + [ln + col for ln, col in zip(pe[1:], columns(ppairs))]
    assert (tmp_path / "peh.tsv").read_text().splitlines() == want_pe
    r = run(*pbase, "-E", tmp_path / "pek.tsv", "-O", tmp_path / "pok.tsv", "-H", "30,22", "-m", "50")
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "pek.tsv").read_text().splitlines() == [want_pe[0]] + [ln for ln, k in zip(want_pe[1:], pkeep) if k]
    assert (tmp_path / "pok.tsv").read_text().splitlines() == [po[0]] + [ln for ln, k in zip(po[1:], pkeep) if k]
    for args, text in (((*pbase, "-E", tmp_path / "x.tsv", "-O", tmp_path / "xo.tsv", "-m", "50"), "give -H"),
                       ((*pbase[:5], "-R", tmp_path / "g.fa", "-M", "2", "-O", tmp_path / "x.tsv", "-H", "8"), "give -E"),
                       ((*pbase, "-E", tmp_path / "x.tsv", "-O", tmp_path / "xo.tsv", "-H", "8,28"), "-H takes")):
        r = run(*args)
        assert r.returncode != 0 and text in (r.stderr + r.stdout), (args, r.stderr)
    gen.close()
