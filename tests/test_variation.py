"""Known variation under candidate guides on the device (vsc_loci_variation, vsc_guides_variation, vsc_pattern_guides_variation
and the two filters): bit for bit what the definition gives when it is applied locus by locus in plain Python on strings and lists
(tests/variation_cases.py), and what vsc_variation_host gives.  Integers, so there is no tolerance: rows, pairs, coverage and
counts are compared as they are, the undefined row included."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import edit_cases as ed
import variation_cases as vc
import varscot_amd as va
from helpers import random_seq, revcomp
from varscot_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "varscot_amd", "bin")
TILE = 1024  # candidates per wave of the pairs' and the filter's passes (include/varscot_hip.h)
COUNTS = vc.CLASSES + ("with_disrupting", "pairs", "variants_covered")
SHAPES = ["spcas9", "front16", "sacas32", "odd23"]  # sites of 23, 16, 32 and 23 bases; the PAM behind, in front, behind, anywhere
SETS = ["none", "one", "one_contig", "third", "every3", "edges", "ends", "long", "third_wide", "saturated"]


@pytest.fixture(scope="module")
def ctx():
    c = va.Context(0)
    yield c
    c.close()


def counts(stats):
    return {k: stats[k] for k in COUNTS}


class Guides:
    """A vsc_guides (or, pattern=True, a vsc_pattern_guides) handle and its variation calls."""

    def __init__(self, ctx, handle, pattern=False):
        self.ctx, self.h, self.pattern = ctx, handle, pattern
        L = va.lib()
        kind = "vsc_pattern_guides" if pattern else "vsc_guides"
        self.fn = {k: getattr(L, "%s_%s" % (kind, k)) for k in ("count", "data", "free", "variation", "filter_variation")}

    @classmethod
    def from_arrays(cls, ctx, codes, loci, on_device=True, pattern=False):
        h = C.c_void_p()
        make = va.lib().vsc_debug_pattern_guides_from_host if pattern else va.lib().vsc_debug_guides_from_host
        _lib.check(make(ctx._h if on_device else None, _lib.ptr(codes), _lib.ptr(loci), len(codes), C.byref(h)), ctx._h)
        return cls(ctx, h, pattern)

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

    def variation(self, gen, shape, variants, capacity):
        """(rows, pairs, coverage, stats, status)."""
        n, n_v = len(self), len(variants)
        rows, pairs = np.empty((n, 4), dtype=np.uint32), np.zeros(capacity, dtype=va.VARIATION_PAIR_DTYPE)
        cov = np.empty((n_v, 2), dtype=np.uint32)
        st, count, sh = _lib.VariationStats(), C.c_uint64(), shape._struct()
        rc = self.fn["variation"](self.ctx._h, gen._h, self.h, C.byref(sh), _lib.ptr(variants) if n_v else None, n_v, _lib.ptr(rows),
                                  _lib.ptr(pairs), capacity, C.byref(count), _lib.ptr(cov), C.byref(st))
        return rows, pairs[:min(capacity, int(count.value))], cov, st.as_dict(), rc

    def filter_code(self, gen, shape, variants, max_cost=0xFFFFFFFF, by_zone=(255, 255, 255, 255), require=0, reserved=0):
        out = C.c_void_p()
        sh = shape._struct()
        f = _lib.VariationFilterStruct(max_cost, by_zone[0] | by_zone[1] << 8 | by_zone[2] << 16 | by_zone[3] << 24, require, reserved)
        n_v = len(variants)
        return self.fn["filter_variation"](self.ctx._h, gen._h, self.h, C.byref(sh), _lib.ptr(variants) if n_v else None, n_v, C.byref(f),
                                           C.byref(out)), out

    def filter(self, gen, shape, variants, **kw):
        code, out = self.filter_code(gen, shape, variants, **kw)
        _lib.check(code, self.ctx._h)
        return Guides(self.ctx, out, self.pattern)

    def close(self):
        if self.h:
            self.fn["free"](self.h)
            self.h = None


# ---- 1. every locus of the wide genome, every variant set ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def world(ctx):
    """Per site length: the wide genome resident, and per (shape, variant set) the loci, the arrays and the expected result,
    computed once and shared."""
    cache = {}

    def get(site_len):
        if site_len not in cache:
            contigs = vc.wide_genome(site_len)
            packed = va.PackedGenome.from_sequences(list(contigs))
            cache[site_len] = {"contigs": contigs, "packed": packed, "gen": ctx.load_genome(packed), "sets": vc.variant_sets(contigs, site_len),
                               "case": {}}
        return cache[site_len]

    def case(shape_name, which):
        shape = vc.SHAPES[shape_name]()
        s = get(shape[0])
        if (shape_name, which) not in s["case"]:
            variants, where = s["sets"][which]
            loci = vc.loci_of(s["contigs"], where) + ed.invalid_loci(s["contigs"])
            s["case"][shape_name, which] = {"shape": shape, "sh": vc.shape_of(shape), "variants": variants, "var": vc.variant_array(variants),
                                            "loci": loci, "arr": ed.locus_array(loci),
                                            "want": vc.expected(s["contigs"], loci, shape, variants)}
        return dict(s["case"][shape_name, which], gen=s["gen"], contigs=s["contigs"], packed=s["packed"])

    get.case = case
    yield get
    for s in cache.values():
        s["gen"].close()


def same(got, want):
    rows, pairs, coverage, stats = got
    assert rows.dtype == np.uint32 and rows.shape == want["rows"].shape and rows.tobytes() == want["rows"].tobytes()
    assert counts(stats) == want["stats"] and sum(stats[k] for k in vc.CLASSES) == len(rows) and stats["off_contig"] == 0
    assert pairs.dtype == va.VARIATION_PAIR_DTYPE and pairs.tobytes() == want["pairs"].tobytes()
    assert coverage.tobytes() == want["coverage"].tobytes()


@pytest.mark.parametrize("which", SETS)
@pytest.mark.parametrize("shape_name", SHAPES)
def test_every_locus_of_the_wide_genome(ctx, world, shape_name, which):
    c = world.case(shape_name, which)
    want = c["want"]
    # the loci route
    same(c["gen"].variation(c["arr"], c["sh"], c["var"], coverage=True), want)
    # the candidates where they lie: vsc_guides for 23, the pattern handle (the caller vouches for the length) for the others
    g = Guides.from_arrays(ctx, np.arange(len(c["arr"]), dtype=np.uint64), c["arr"], pattern=c["shape"][0] != 23)
    rows, pairs, cov, stats, rc = g.variation(c["gen"], c["sh"], c["var"], len(want["pairs"]) + 3)
    assert rc == 0 and rows.tobytes() == want["rows"].tobytes() and pairs.tobytes() == want["pairs"].tobytes()
    assert cov.tobytes() == want["coverage"].tobytes() and counts(stats) == want["stats"]
    g.close()
    # the host's definition: the same bytes wherever the site has its letters (it has no planes: an N is no class of its own)
    h_rows, h_pairs, h_cov = va.variation_host(c["packed"].contigs, c["arr"], c["sh"], c["var"], coverage=True)
    has_n = np.array([ed.site_of(c["contigs"], locus, c["shape"][0])[0] == "has_n" for locus in c["loci"]])
    assert h_rows[~has_n].tobytes() == rows[~has_n].tobytes() and (h_rows[has_n] != vc.UNDEF).any() == bool(has_n.any())
    lettered = ~has_n[h_pairs["candidate"]]
    renumbered = h_pairs[lettered]
    assert renumbered.tobytes() == pairs.tobytes()  # (a site with an N has no pair on the device)


def test_the_cases_are_not_vacuous(world):
    """What the cases are for, asserted on the restatement."""
    w = {k: world.case("spcas9", k)["want"] for k in SETS}
    assert w["none"]["stats"]["pairs"] == 0 and (w["none"]["rows"][w["none"]["rows"][:, 0] != vc.UNDEF] == 0).all()
    assert all(w["third"]["stats"][k] >= 5 for k in ("defined", "invalid", "has_n"))
    per = np.bincount(w["every3"]["pairs"]["candidate"])
    assert per.max() == 69  # every position with all three alts
    first, touched, top, silent = va.unpack_variation_info(w["every3"]["pairs"]["info"])
    assert silent.any() and not silent.all() and set(top.tolist()) == {0, 1, 2, 3} and (touched == 1).all()
    e = world.case("spcas9", "edges")
    cand = e["loci"].index((ed.MAIN, 200, 0))
    mine = e["want"]["pairs"][e["want"]["pairs"]["candidate"] == cand]
    weights = set(mine["weight"].tolist())
    assert not weights & set(range(1, 41)) and not weights & set(range(101, 141))  # end at its first base / start at its end: no overlap
    assert set(range(201, 241)) <= weights and set(range(301, 341)) <= weights  # one base at either edge
    assert {997, 998, 999} <= weights
    t = va.unpack_variation_info(mine["info"])[1]
    assert t.min() == 1 and t.max() == 23
    lc = world.case("spcas9", "long")
    lg, longest = lc["want"], [k for k, v in enumerate(lc["variants"]) if v[2] == 3000][0]
    under = np.bincount(lg["pairs"]["variant"], minlength=len(lc["variants"]))
    assert under[longest] > 5000 and under.min() >= 1  # the long span reaches thousands of sites, and every nested variant its own
    assert len(set((lg["pairs"]["candidate"][lg["pairs"]["variant"] == longest] // 512).tolist())) >= 10
    sat = w["saturated"]
    by, _, cost, largest = va.unpack_variation_row(sat["rows"][sat["rows"][:, 2] != vc.UNDEF])
    assert (by == 255).any() and max(max(z) for z in sat["by_zone"] if z) == 300
    assert (cost == vc.MAX_U32).any() and max(c for c in sat["cost"] if c is not None) >= 2 * vc.MAX_U32 and (largest == vc.MAX_U32).any()
    ends = w["ends"]
    assert ends["stats"]["with_disrupting"] == ends["stats"]["defined"] > 100  # (the whole-contig deletions reach every site)
    # a lookup block (256 positions) with no variant of its own, and candidates at a block's first and last position
    c = world.case("spcas9", "third_wide")
    off = ed.offsets(c["contigs"])
    blocks = {(off[v[0]] + v[1]) >> 8 for v in c["variants"]}
    starts = {(off[l[0]] + l[1]) & 255 for l in c["loci"] if l[0] < len(off) and l[1] < 5000}
    assert any((off[l[0]] + l[1]) >> 8 not in blocks for l in c["loci"] if l[0] == vc.BIG and l[1] < 4000) and {0, 255} <= starts


# ---- 2. the lookup's block does not show ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["long", "third_wide", "ends", "saturated"])
def test_the_smallest_and_a_large_block_give_the_same_bytes(ctx, world, which):
    c = world.case("spcas9", which)
    L = va.lib()
    assert L.vsc_debug_variation_block_bits(ctx._h, 3) == -22 and L.vsc_debug_variation_block_bits(ctx._h, 33) == -22
    try:
        for bits in (4, 32, 13):
            assert L.vsc_debug_variation_block_bits(ctx._h, bits) == 0
            same(c["gen"].variation(c["arr"], c["sh"], c["var"], coverage=True), c["want"])
    finally:
        assert L.vsc_debug_variation_block_bits(ctx._h, 0) == 0
    same(c["gen"].variation(c["arr"], c["sh"], c["var"], coverage=True), c["want"])


# ---- 3. the pair contract and the tiles --------------------------------------------------------------------------------------------
def prefix(want, n):
    pairs = want["pairs"][want["pairs"]["candidate"] < n]
    cov = np.zeros_like(want["coverage"])
    _, _, _, silent = va.unpack_variation_info(pairs["info"])
    np.add.at(cov, (pairs["variant"].astype(np.int64), silent.astype(np.int64)), 1)
    return want["rows"][:n], pairs, cov


@pytest.fixture(scope="module")
def tiled(world):
    """third_wide with the 1 024 loci that no variant reaches in front: tile 0 has no pair."""
    c = world.case("spcas9", "third_wide")
    quiet = [i for i, l in enumerate(c["loci"]) if l[0] == vc.BIG and 2000 <= l[1] < 2512]
    in_front = set(quiet)
    rest = [i for i in range(len(c["loci"])) if i not in in_front]
    loci = [c["loci"][i] for i in quiet + rest]
    want = vc.expected(c["contigs"], loci, c["shape"], c["variants"])
    assert len(quiet) == TILE and len(loci) >= 3 * TILE + 1 and not (want["pairs"]["candidate"] < TILE).any()
    return dict(c, loci=loci, arr=ed.locus_array(loci), want=want)


@pytest.mark.parametrize("n", [1023, 1024, 1025, 3 * 1024 + 1])
def test_candidates_around_the_tile(ctx, tiled, n):
    want_rows, want_pairs, want_cov = prefix(tiled["want"], n)
    rows, pairs, cov, stats = tiled["gen"].variation(tiled["arr"][:n], tiled["sh"], tiled["var"], coverage=True)
    assert rows.tobytes() == want_rows.tobytes() and pairs.tobytes() == want_pairs.tobytes() and cov.tobytes() == want_cov.tobytes()
    assert stats["pairs"] == len(want_pairs) and (n <= 1025 or len(want_pairs) > 1000)


def test_the_pair_contract(ctx, tiled):
    s = tiled
    want = s["want"]
    total = len(want["pairs"])
    L, st = va.lib(), s["sh"]._struct()
    n, var = len(s["arr"]), s["var"]

    def call(pairs, capacity, rows=True, cov=True):
        r = np.full((n, 4), 7, dtype=np.uint32) if rows else None
        c = np.full((len(var), 2), 7, dtype=np.uint32) if cov else None
        count, stats = C.c_uint64(12345), _lib.VariationStats()
        rc = L.vsc_loci_variation(ctx._h, s["gen"]._h, _lib.ptr(s["arr"]), n, C.byref(st), _lib.ptr(var), len(var), _lib.ptr(r), _lib.ptr(pairs),
                                  capacity, C.byref(count), _lib.ptr(c), C.byref(stats))
        return rc, r, c, int(count.value), stats.as_dict()

    rc, rows, cov, count, stats = call(None, 0)  # pairs == NULL: count only
    assert rc == 0 and count == total and rows.tobytes() == want["rows"].tobytes() and cov.tobytes() == want["coverage"].tobytes()
    assert counts(stats) == want["stats"]
    exact = np.zeros(total, dtype=va.VARIATION_PAIR_DTYPE)
    rc, rows, cov, count, _ = call(exact, total)
    assert rc == 0 and count == total and exact.tobytes() == want["pairs"].tobytes()
    short = np.full(4 * total, 0x5A5A5A5A, dtype=np.uint32).view(va.VARIATION_PAIR_DTYPE)
    before = short.tobytes()
    rc, rows, cov, count, stats = call(short, total - 1)  # one short
    assert rc == -34 and "capacity" in L.vsc_last_error(ctx._h).decode()
    assert short.tobytes() == before  # nothing is written to pairs
    assert count == total and rows.tobytes() == want["rows"].tobytes() and cov.tobytes() == want["coverage"].tobytes() and counts(stats) == want["stats"]
    rc, _, _, count, stats = call(None, 0, rows=False, cov=False)  # every output but the count is optional
    assert rc == 0 and count == total and counts(stats) == want["stats"]  # (the covered variants are then counted on the device)
    assert L.vsc_loci_variation(ctx._h, s["gen"]._h, _lib.ptr(s["arr"]), n, C.byref(st), _lib.ptr(var), len(var), None, None, 0, None, None, None) == 0
    # the host's definition keeps the same contract
    h_short = np.full(4 * total, 0x5A5A5A5A, dtype=np.uint32).view(va.VARIATION_PAIR_DTYPE)
    h_cov, h_count = np.full((len(var), 2), 7, dtype=np.uint32), C.c_uint64()
    ct = s["packed"].contigs
    h_total = len(vc.expected(s["contigs"], s["loci"], s["shape"], s["variants"], planes=False)["pairs"])
    rc = L.vsc_variation_host(_lib.ptr(ct), len(ct), _lib.ptr(s["arr"]), n, C.byref(st), _lib.ptr(var), len(var), None, _lib.ptr(h_short), h_total - 1,
                              C.byref(h_count), _lib.ptr(h_cov))
    assert rc == -34 and h_short.tobytes() == before and int(h_count.value) == h_total and int(h_cov.sum()) == h_total
    # nothing to do
    rows, pairs, coverage, stats = s["gen"].variation(ed.locus_array([]), s["sh"], var, coverage=True)
    assert rows.shape == (0, 4) and len(pairs) == 0 and (coverage == 0).all() and counts(stats) == dict.fromkeys(COUNTS, 0)
    t = ctx.timing()
    assert t["sites"] == 0 and t["total_ms"] == 0


# ---- 4. the filter ---------------------------------------------------------------------------------------------------------------
FILTERS = [dict(), dict(max_cost=0), dict(max_cost=9), dict(by_zone=(255, 255, 255, 0)), dict(by_zone=(0, 255, 255, 255)),
           dict(by_zone=(255, 1, 255, 255)), dict(by_zone=(255, 255, 2, 255)), dict(require=8), dict(require=12), dict(require=1),
           dict(max_cost=20, by_zone=(255, 255, 255, 1), require=12)]


@pytest.mark.parametrize("which,shape_name", [("third_wide", "spcas9"), ("saturated", "odd23"), ("none", "spcas9"), ("edges", "sacas32")])
def test_filter_bounds_and_input_order(ctx, world, which, shape_name):
    c = world.case(shape_name, which)
    want, n = c["want"], len(c["loci"])
    codes = np.arange(n, dtype=np.uint64) * np.uint64(5)
    pattern = c["shape"][0] != 23
    g = Guides.from_arrays(ctx, codes, c["arr"], pattern=pattern)
    host = Guides.from_arrays(ctx, codes, c["arr"], on_device=False, pattern=pattern)  # the host-only object: uploaded first
    kept = []
    for f in FILTERS:
        keep = np.array([vc.keep(z, cost, f.get("max_cost", 0xFFFFFFFF), f.get("by_zone", (255,) * 4),
                                 [z_ for z_ in range(4) if f.get("require", 0) >> z_ & 1]) for z, cost in zip(want["by_zone"], want["cost"])])
        for handle in (g, host):
            out = handle.filter(c["gen"], c["sh"], c["var"], **f)
            got_codes, got_loci = out.arrays()
            out.close()
            assert got_codes.tobytes() == codes[keep].tobytes() and got_loci.tobytes() == c["arr"][keep].tobytes(), f
        kept.append(int(keep.sum()))
    assert kept[0] == want["stats"]["defined"]
    if which == "third_wide":
        assert all(k <= kept[0] for k in kept) and len(set(kept)) >= 7 and sum(k > 0 for k in kept) >= 8
        t = ctx.timing()
        assert t["sites"] == n and t["score_ms"] == t["total_ms"] > 0
        assert t["genome_bytes"] == 32 * n + 48 * kept[-1]  # (the last call's)
    if which == "none":
        assert kept[1:7] == [kept[0]] * 6 and kept[7:] == [0] * 4  # no variant: every bound holds, nothing is required in vain
    empty = g.filter(c["gen"], c["sh"], c["var"], max_cost=0, require=15)  # an empty result is a result
    assert len(empty) == 0 and len(empty.filter(c["gen"], c["sh"], c["var"]).arrays()[0]) == 0
    for h in (empty, host, g):
        h.close()


# ---- 5. candidates where they lie, the Python layer --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted(ctx):
    """A 20 kb random genome with NGG sites (and CCN sites, their '-' form) at and next to the contig ends, and a variant list
    in the caller's form: SNVs at every 31st position, a deletion and an insertion every 101 bases, given unsorted."""
    rng = np.random.default_rng(79)
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
    rows, plain = [], []
    for c, t in enumerate(contigs):
        for p in range(0, len(t) - 4):
            if p % 31 == 0:
                alt = "ACGT"[("ACGT".index(t[p]) + 1 + p % 3) % 4]
                w = va.variant_weight(0.001 * (1 + p % 50))
                rows.append((c, p, t[p], alt, w))
                plain.append((c, p, 1, alt, w))
            if p % 101 == 50:
                rows.append((c, p, t[p:p + 4], t[p], 77))  # VCF style: the anchor base, then three deleted bases
                plain.append((c, p + 1, 3, None, 77))
            if p % 101 == 75:
                rows.append((c, p, t[p], t[p] + "GA", 55))  # an insertion behind p: the bases p and p + 1
                plain.append((c, p, 2, None, 55))
    order = rng.permutation(len(rows))
    yield {"contigs": contigs, "packed": packed, "gen": gen, "rows": [rows[i] for i in order], "plain": [plain[i] for i in order]}
    gen.close()


def caller_numbering(contigs, loci, shape, plain):
    """The expected result of rows given in the caller's order: the variants sorted as site_variants sorts them, and the pairs and
    the coverage numbered in the caller's order."""
    order = sorted(range(len(plain)), key=lambda i: (plain[i][0], plain[i][1]))
    want = vc.expected(contigs, loci, shape, [plain[i] for i in order])
    pairs = want["pairs"].copy()
    pairs["variant"] = np.asarray(order, dtype=np.uint32)[pairs["variant"].astype(np.int64)]
    pairs = pairs[np.lexsort((pairs["variant"], pairs["candidate"]))]
    cov = np.empty_like(want["coverage"])
    cov[order] = want["coverage"]
    return dict(want, pairs=pairs, coverage=cov)


def test_enumerated_guides_where_they_lie(ctx, planted):
    gen, contigs = planted["gen"], planted["contigs"]
    shape = vc.spcas9()
    plain = gen.enumerate_guides()
    codes, loci, rows = gen.enumerate_guides(variation="SpCas9", variants=planted["rows"])
    assert codes.tobytes() == plain[0].tobytes() and loci.tobytes() == plain[1].tobytes() and len(codes) > 1000
    want = caller_numbering(contigs, ed.loci_tuples(loci), shape, planted["plain"])
    assert rows.dtype == np.uint32 and rows.tobytes() == want["rows"].tobytes() and want["stats"]["pairs"] > 1000
    same(gen.variation((codes, loci), "SpCas9", planted["rows"], coverage=True), want)
    assert va.VARIATION_SHAPES["SpCas9"]._struct().zones == vc.shape_of(shape)._struct().zones
    # the handle and the host-only object, which goes the loci route: the same bytes
    var = va.site_variants(planted["rows"])[0]
    sorted_want = vc.expected(contigs, ed.loci_tuples(loci), shape, vc.ordered(planted["plain"]))
    for on_device in (True, False):
        g = Guides.from_arrays(ctx, plain[0], plain[1], on_device=on_device)
        g_rows, g_pairs, g_cov, g_stats, rc = g.variation(gen, va.VARIATION_SHAPES["SpCas9"], var, sorted_want["stats"]["pairs"])
        assert rc == 0 and g_rows.tobytes() == rows.tobytes() and g_pairs.tobytes() == sorted_want["pairs"].tobytes()
        assert g_cov.tobytes() == sorted_want["coverage"].tobytes() and counts(g_stats) == sorted_want["stats"]
        g.close()
    # the filters through the keywords: population-robust (a cost bound, nothing in the PAM) and allele-specific (PAM or seed)
    robust = np.array([vc.keep(z, c, max_cost=va.variant_weight(0.02), max_by_zone=(255, 255, 255, 0)) for z, c in zip(want["by_zone"], want["cost"])])
    allele = np.array([vc.keep(z, c, require=(2, 3)) for z, c in zip(want["by_zone"], want["cost"])])
    assert 0 < robust.sum() < len(robust) and 0 < allele.sum() < len(allele)
    k_codes, k_loci, k_rows = gen.enumerate_guides(variation="SpCas9", variants=planted["rows"], max_variant_cost=va.variant_weight(0.02),
                                                   max_variants_by_zone=(255, 255, 255, 0))
    assert k_codes.tobytes() == codes[robust].tobytes() and k_loci.tobytes() == loci[robust].tobytes() and k_rows.tobytes() == rows[robust].tobytes()
    a_codes, a_loci, a_rows = gen.enumerate_guides(variation="SpCas9", variants=planted["rows"], require_variant_zones=("seed", "pam"))
    assert a_codes.tobytes() == codes[allele].tobytes() and a_rows.tobytes() == rows[allele].tobytes()
    rows_all = gen.summarize(codes, 2, exclude=loci)
    d = gen.design(None, 2, variation="SpCas9", variants=planted["rows"], require_variant_zones=(2, 3))
    assert len(d) == 4 and d[0].tobytes() == a_codes.tobytes() and d[2].tobytes() == rows_all[allele].tobytes() and d[3].tobytes() == a_rows.tobytes()
    plain_design = gen.design(None, 2)
    assert len(plain_design) == 3 and plain_design[2].tobytes() == rows_all.tobytes()  # without the arguments: what it returned before
    for kw in (dict(variation=va.VariationShape(27)), dict(max_variant_cost=1), dict(variants=planted["rows"]), dict(variation="SpCas9"),
               dict(variation="Cas13", variants=planted["rows"]), dict(variation="SpCas9", variants=planted["rows"], require_variant_zones=("tail",))):
        with pytest.raises(ValueError):
            gen.enumerate_guides(**kw)


@pytest.mark.parametrize("name,pattern,proto,case", [("SaCas9", "N" * 21 + "NNGRRT", (0, 21), None), ("Cas12a", "TTTV" + "N" * 23, (4, 23), "cas12a27")])
def test_pattern_candidates_of_other_nucleases(planted, name, pattern, proto, case):
    gen, contigs = planted["gen"], planted["contigs"]
    sh = va.VARIATION_SHAPES[name]
    shape = vc.cas12a27() if case else (27, [1] * 11 + [2] * 10 + [0, 0, 3, 3, 3, 3], [""] * 21 + ["ACGT", "ACGT", "G", "AG", "AG", "T"])
    assert vc.shape_of(shape)._struct().zones == sh._struct().zones and list(vc.shape_of(shape)._struct().accept) == list(sh._struct().accept)
    plain = gen.enumerate_pattern(pattern, proto)
    found, rows = gen.enumerate_pattern(pattern, proto, variation=sh, variants=planted["rows"])
    assert found.codes.tobytes() == plain.codes.tobytes() and found.loci.tobytes() == plain.loci.tobytes() and len(found) > 100
    want = caller_numbering(contigs, ed.loci_tuples(found.loci), shape, planted["plain"])
    assert want["stats"]["defined"] > 100 and want["stats"]["pairs"] > 300 and rows.tobytes() == want["rows"].tobytes()
    same(gen.variation(found, sh, planted["rows"], coverage=True), want)
    silent = va.unpack_variation_info(want["pairs"]["info"])[3]
    assert silent.any()  # an SNV that the R, the V or an N of the PAM accepts
    keep = np.array([vc.keep(z, c, max_by_zone=(255, 255, 0, 0)) for z, c in zip(want["by_zone"], want["cost"])])
    assert 0 < keep.sum() < len(keep)
    kept, krows = gen.enumerate_pattern(pattern, proto, variation=name, variants=planted["rows"], max_variants_by_zone=(255, 255, 0, 0))
    assert kept.codes.tobytes() == found.codes[keep].tobytes() and kept.loci.tobytes() == found.loci[keep].tobytes()
    assert krows.tobytes() == want["rows"][keep].tobytes()
    d_found, d_rows, d_var = gen.design_pattern(pattern, proto, 2, variation=name, variants=planted["rows"], max_variants_by_zone=(255, 255, 0, 0))
    assert d_found.codes.tobytes() == kept.codes.tobytes() and d_var.tobytes() == krows.tobytes()
    _, all_rows = gen.design_pattern(pattern, proto, 2)
    assert d_rows.tobytes() == all_rows[keep].tobytes()  # only the survivors are searched


def test_the_best_guides_for_every_variant(planted):
    """variation_pick_inputs -> Genome.pick against a loop on the host: for every variant the K guides that have it in PAM or seed."""
    gen, contigs, packed = planted["gen"], planted["contigs"], planted["packed"]
    codes, loci = gen.enumerate_guides()
    rows, pairs, _, stats = gen.variation((codes, loci), "SpCas9", planted["rows"])
    spec = (np.arange(len(codes), dtype=np.uint64) * np.uint64(2654435761)) % np.uint64(10007)  # a stand-in for a specificity column
    p_loci, p_target, key, index = va.variation_pick_inputs(pairs, loci, extra_columns=[(spec, 14)])
    pick = va.PickShape(3, spacing=2)
    picks, cnt, _ = gen.pick(p_loci, key, pick, target=p_target, n_targets=len(planted["rows"]))
    # the host loop: the disrupting pairs whose top is seed or PAM, the key by hand, the host's pick
    want = caller_numbering(contigs, ed.loci_tuples(loci), vc.spcas9(), planted["plain"])["pairs"]
    chosen = [k for k, q in enumerate(want) if not (int(q["info"]) >> 18 & 1) and (int(q["info"]) >> 16 & 3) in (2, 3)]
    assert index.tolist() == chosen and 200 < len(chosen) < len(want)
    w = want[chosen]
    want_key = ((w["info"].astype(np.uint64) >> np.uint64(16)) & np.uint64(3)) << np.uint64(14) | np.minimum(spec[w["candidate"]], np.uint64(16383))
    assert key.tobytes() == want_key.tobytes() and p_target.tobytes() == w["variant"].tobytes()
    h_picks, h_cnt, _ = va.pick_host(packed.contigs, loci[w["candidate"]], w["variant"], want_key, len(planted["rows"]), pick)
    assert picks.tobytes() == h_picks.tobytes() and cnt.tobytes() == h_cnt.tobytes() and cnt.max() >= 2 and (cnt == 0).any()
    first = picks[cnt > 0, 0]
    tops = (w["info"] >> 16) & 3
    assert (tops[first] == [tops[w["variant"] == t].max() for t in np.nonzero(cnt > 0)[0]]).all()  # a PAM guide before a seed guide


def test_a_shard_answers_for_what_it_holds(ctx, planted):
    packed, contigs = planted["packed"], planted["contigs"]
    shape, sh = vc.spcas9(), va.VARIATION_SHAPES["SpCas9"]
    n_words = packed.n_words
    loci = [(0, p, s) for p in list(range(2000, 2100)) + list(range(2200, 2280)) for s in (0, 1)]
    loci += ed.loci_tuples(planted["gen"].enumerate_guides()[1])
    arr = ed.locus_array(loci)
    variants = vc.ordered(planted["plain"])
    var = vc.variant_array(variants)
    for first, words, own in ((64, n_words - 64, n_words - 64), (0, 70, 64)):  # nothing in front of word 64; nothing behind a 6-word halo
        sl = slice(first, first + words)
        shard = va.Genome.from_shard(ctx, packed.hi[sl], packed.lo[sl], packed.nmask[sl], first, own, packed.contigs)
        want = vc.expected(contigs, loci, shape, variants, resident=(32 * first, 32 * (first + words)))
        assert want["stats"]["not_resident"] > 100 and want["stats"]["defined"] > 100 and want["stats"]["pairs"] > 100
        with pytest.raises(ValueError) as e:
            shard.variation(arr, sh, var)
        assert "not resident" in str(e.value)
        same(shard.variation(arr, sh, var, coverage=True, allow_partial=True), want)
        shard.close()


def test_alternating_cases_scratch_and_timing(ctx, world):
    combos = [("spcas9", "third"), ("odd23", "every3"), ("spcas9", "none"), ("odd23", "long")]
    for k in (0, 0, 1, 0, 2, 3, 1, 2):  # nothing of a call outlives it
        c = world.case(*combos[k])
        same(c["gen"].variation(c["arr"], c["sh"], c["var"], coverage=True), c["want"])
    ctx.release_scratch()
    c = world.case(*combos[1])
    same(c["gen"].variation(c["arr"], c["sh"], c["var"], coverage=True), c["want"])
    ctx.release_scratch()
    c = world.case(*combos[0])
    got = c["gen"].variation(c["arr"], c["sh"], c["var"], coverage=True)
    same(got, c["want"])
    stats, n = got[3], len(c["loci"])
    assert stats["kernel_ms"] > 0 and stats["wall_ms"] >= stats["kernel_ms"]
    t = ctx.timing()
    assert t["score_ms"] > 0 and t["scan_ms"] > 0 and t["total_ms"] == t["score_ms"] + t["scan_ms"] and t["sites"] == n
    assert t["genome_bytes"] == 32 * n
    c = world.case(*combos[2])
    c["gen"].variation(c["arr"], c["sh"], c["var"])
    t = ctx.timing()
    assert t["scan_ms"] == 0 and t["total_ms"] == t["score_ms"] > 0  # without variants: the rows kernel alone


# ---- 6. every refusal, before anything is written ------------------------------------------------------------------------------------
def test_every_refusal(ctx, planted):
    L = va.lib()
    gen, contigs = planted["gen"], planted["contigs"]
    g = Guides.from_arrays(ctx, *gen.enumerate_guides())
    n = len(g)
    rows = np.full((n, 4), 9, dtype=np.uint32)
    ok = va.VARIATION_SHAPES["SpCas9"]._struct()
    good = vc.variant_array([(0, 5, 1, "A", 1), (0, 5, 1, "C", 2), (1, 0, 3, None, 3)])
    count = C.c_uint64()

    def guides_variation(shape, variants=None, n_v=0, handle=g.h, genome=gen._h, context=None):
        return L.vsc_guides_variation((context or ctx)._h, genome, handle, shape, _lib.ptr(variants), n_v, _lib.ptr(rows), None, 0, C.byref(count),
                                      None, None)

    def error():
        return L.vsc_last_error(ctx._h).decode()

    assert guides_variation(C.byref(ok), good, len(good)) == 0 and not (rows == 9).all()
    rows[:] = 9
    for bad in (dict(site_len=15), dict(site_len=33), dict(site_len=23, zones=1 << 46), dict(site_len=23, accept=(0, 1 << 28)),
                dict(site_len=16, accept=(0, 1))):  # a shape outside SHAPE
        sh = va.VariationShape(validate=False, **bad)
        st = sh._struct()
        assert guides_variation(C.byref(st)) == -22, bad
        code, out = g.filter_code(gen, sh, good)
        assert code == -22 and not out.value
        with pytest.raises(va.VarscotError):
            gen.variation(ed.locus_array([(0, 100, 0)]), sh, good)
    for field in ("reserved0", 0, 3):
        reserved = va.VARIATION_SHAPES["SpCas9"]._struct()
        if field == "reserved0":
            reserved.reserved0 = 1
        else:
            reserved.reserved[field] = 1
        assert guides_variation(C.byref(reserved)) == -22 and "reserved" in error()
    sh27 = va.VARIATION_SHAPES["Cas12a"]  # vsc_guides holds 23-mers
    st27 = sh27._struct()
    assert guides_variation(C.byref(st27)) == -22 and "site_len" in error()
    assert g.filter_code(gen, sh27, good)[0] == -22
    assert guides_variation(None) == -22 and guides_variation(C.byref(ok), genome=None) == -22 and guides_variation(C.byref(ok), handle=None) == -22
    assert guides_variation(C.byref(ok), None, 3) == -22 and "null" in error()  # n_v > 0 with NULL variants
    assert L.vsc_guides_filter_variation(ctx._h, gen._h, g.h, C.byref(ok), None, 0, None, C.byref(C.c_void_p())) == -22  # no filter
    assert L.vsc_guides_filter_variation(ctx._h, gen._h, g.h, C.byref(ok), None, 0, C.byref(_lib.VariationFilterStruct(0, 0, 0, 0)), None) == -22
    for kw in (dict(require=16), dict(reserved=1)):
        code, out = g.filter_code(gen, va.VARIATION_SHAPES["SpCas9"], good, **kw)
        assert code == -22 and not out.value and "require_zones" in error()

    def raw(records):
        out = np.zeros(len(records), dtype=va.VARIANT_DTYPE)
        for k, r in enumerate(records):
            out[k] = r
        return out

    last = len(contigs[0]) - 1
    for bad, word in (([(0, 6, 1 | 4 << 16, 0), (0, 5, 1 | 4 << 16, 0)], "ascending"), ([(1, 0, 1 | 4 << 16, 0), (0, 5, 1 | 4 << 16, 0)], "ascending"),
                      ([(len(contigs), 0, 1 | 4 << 16, 0)], "unknown"), ([(0xFFFFFFFF, 0, 1 | 4 << 16, 0)], "unknown"),
                      ([(0, 5, 0 | 4 << 16, 0)], "span is 0"), ([(0, last, 2 | 4 << 16, 0)], "beyond"), ([(0, last + 1, 1 | 4 << 16, 0)], "beyond"),
                      ([(0, 0, 65535 | 4 << 16, 0)], "beyond"), ([(0, 5, 2 | 1 << 16, 0)], "SNV"), ([(0, 5, 1 | 5 << 16, 0)], "alt"),
                      ([(0, 5, 1 | 4 << 16 | 1 << 19, 0)], "alt"), ([(0, 5, 1 | 1 << 31, 0)], "alt"), ([(0, 5, 1 | 4 << 16, 0xFFFFFFFF)], "weight")):
        v = raw(bad)
        assert guides_variation(C.byref(ok), v, len(v)) == -22 and word in error(), bad
        code, out = g.filter_code(gen, va.VARIATION_SHAPES["SpCas9"], v)
        assert code == -22 and not out.value
        assert L.vsc_loci_variation(ctx._h, gen._h, _lib.ptr(rows), 1, C.byref(ok), _lib.ptr(v), len(v), None, None, 0, None, None, None) == -22
    assert (rows == 9).all()  # checked before anything is written
    edge = raw([(0, 0, 1 | 2 << 16, 0xFFFFFFFE), (0, last, 1 | 4 << 16, 0), (1, 0, len(contigs[1]) | 4 << 16, 0)])  # what the bounds allow
    assert guides_variation(C.byref(ok), edge, len(edge)) == 0
    assert L.vsc_loci_variation(ctx._h, gen._h, None, 1, C.byref(ok), None, 0, _lib.ptr(rows), None, 0, None, None, None) == -22
    assert L.vsc_loci_variation(ctx._h, gen._h, _lib.ptr(rows), 0xFFFFFFFF, C.byref(ok), None, 0, None, None, 0, None, None, None) == -34  # n
    assert L.vsc_loci_variation(ctx._h, gen._h, _lib.ptr(rows), 1, C.byref(ok), _lib.ptr(good), 0xFFFFFFFF, None, None, 0, None, None, None) == -34  # n_v
    other = va.Context(0)  # a genome or an object of another context is refused
    assert guides_variation(C.byref(ok), context=other) == -22
    o_gen = other.load_genome(planted["packed"])
    assert guides_variation(C.byref(ok), genome=o_gen._h, context=other) == -22 and "another context" in L.vsc_last_error(other._h).decode()
    o_gen.close()
    other.close()
    g.close()


# ---- 7. the tools end to end ---------------------------------------------------------------------------------------------------
def test_both_tools_on_the_small_genome(ctx, tmp_path):
    contigs = list(ed.small_genome())
    names = ["chr%d of the small genome" % (k + 1) for k in range(len(contigs))]
    chrom = [n.split()[0] for n in names]
    with open(tmp_path / "g.fa", "w") as f:
        for n, t in zip(names, contigs):
            f.write(">%s\n%s\n" % (n, "\n".join(t[i:i + 60] for i in range(0, len(t), 60))))
    iv = [(c, 0, len(t)) for c, t in enumerate(contigs)]
    (tmp_path / "t.bed").write_text("".join("%s\t%d\t%d\n" % (chrom[c], a, b) for c, a, b in iv))
    run = lambda *a: subprocess.run([os.path.join(BIN, a[0])] + [str(x) for x in a[1:]], capture_output=True, text=True, timeout=600)  # noqa: E731
    assert run("bidir_index", "-G", tmp_path / "g.fa", "-I", tmp_path / "idx").returncode == 0
    packed = va.PackedGenome.from_sequences(contigs)
    gen = ctx.load_genome(packed)
    lengths = [len(t) for t in contigs]
    # a VCF (1-based, an allele frequency per ALT, a multi-allelic line, a deletion, an insertion, a symbolic allele and a line
    # out of order) and the same variants as the rows the Python layer takes
    main, second = contigs[ed.MAIN], contigs[ed.SECOND]
    nxt = lambda ch, k=1: "ACGT"[("ACGT".index(ch) + k) % 4]  # noqa: E731
    vcf, rows_in = ["##fileformat=VCFv4.2", "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"], []
    for c, text in ((ed.MAIN, main), (ed.SECOND, second)):
        for p in range(120, len(text) - 10, 9):
            af = 0.0005 * (1 + p % 40)
            if p % 5 == 0:
                alts, afs = [nxt(text[p]), nxt(text[p], 2)], [af, 0.25]
            elif p % 5 == 1:
                alts, afs = [text[p]], [af]
                vcf.append("%s\t%d\t.\t%s\t%s\t.\t.\tDP=9;AF=%r" % (chrom[c], p + 1, text[p:p + 3], text[p], af))  # a deletion of two bases
                rows_in.append((c, p, text[p:p + 3], text[p], va.variant_weight(af)))
                continue
            elif p % 5 == 2:
                vcf.append("%s\t%d\t.\t%s\t%s,<DEL>\t.\t.\tAF=%r,0.5;DP=3" % (chrom[c], p + 1, text[p], text[p] + "TT", af))  # an insertion; a symbolic allele
                rows_in.append((c, p, text[p], text[p] + "TT", va.variant_weight(af)))
                continue
            else:
                alts, afs = [nxt(text[p], 3)], [af]
            vcf.append("%s\t%d\trs%d\t%s\t%s\t.\tPASS\tAF=%s" % (chrom[c], p + 1, p, text[p], ",".join(alts), ",".join(repr(a) for a in afs)))
            rows_in += [(c, p, text[p], a, va.variant_weight(f)) for a, f in zip(alts, afs)]
    vcf.append(vcf.pop(2))  # a line out of order: the tool sorts
    (tmp_path / "v.vcf").write_text("\n".join(vcf) + "\n")
    (tmp_path / "v.tsv").write_text("".join("%s\t%d\t%s\t%s\t%d\n" % (chrom[c], p, r, a, w) for c, p, r, a, w in rows_in))
    var = va.site_variants(rows_in, lengths=lengths)[0]
    assert len(var) > 100 and len({int(v["span_alt"]) >> 16 for v in var}) == 5
    lines_of = lambda path: (tmp_path / path).read_text().splitlines()  # noqa: E731

    def listing(ids, rows, pairs):
        out = ["#guideId\tnone\tdistal\tseed\tpam\tsilent\tcost\tmaxWeight"]
        by, silent, cost, largest = va.unpack_variation_row(rows)
        out += ["%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d" % ((i,) + tuple(int(x) for x in b) + (int(s), int(c), int(w))) for i, b, s, c, w in zip(ids, by, silent, cost, largest)]
        out += ["", "#chrom\tpos\tspan\talt\tguideId\tfirst\ttouched\ttop\tsilent\tweight"]
        for q in pairs:
            v = var[int(q["variant"])]
            alt = int(v["span_alt"]) >> 16
            info = [int(x) for x in va.unpack_variation_info(q["info"])]
            out.append("%s\t%d\t%d\t%s\t%s\t%d\t%d\t%d\t%d\t%d" % (chrom[int(v["contig"])], v["pos"], int(v["span_alt"]) & 0xFFFF, "ACGT"[alt] if alt < 4 else ".",
                                                                  ids[int(q["candidate"])], info[0], info[1], info[2], info[3], q["weight"]))
        return out

    # guide_summary -E --variants v.vcf --variant-af AF --variation-out
    regions = va.Regions(packed, iv, rule="inside")
    codes, loci = gen.enumerate_guides(regions)
    regions.close()
    ids = ["%s:%d:%s" % (chrom[c], p, "-" if s else "+") for c, p, s in ed.loci_tuples(loci)]
    rows, pairs, _, stats = gen.variation((codes, loci), "SpCas9", var)
    assert 100 < len(codes) < 400 and stats["pairs"] > 100 and stats["with_disrupting"] > 50
    base = ("guide_summary", "-G", tmp_path / "g.fa", "-I", tmp_path / "idx", "-M", "2", "-E", tmp_path / "t.bed")
    r = run(*base, "-L", tmp_path / "plain.bed", "-O", tmp_path / "plain.tsv")
    assert r.returncode == 0, r.stderr
    r = run(*base, "-L", tmp_path / "v.bed", "-O", tmp_path / "v_out.tsv", "--variants", tmp_path / "v.vcf", "--variant-af", "AF", "--variation-out", tmp_path / "vo.tsv")
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "v.bed").read_bytes() == (tmp_path / "plain.bed").read_bytes()  # without a bound every guide stays
    assert (tmp_path / "v_out.tsv").read_bytes() == (tmp_path / "plain.tsv").read_bytes()
    assert lines_of("vo.tsv") == listing(ids, rows, pairs)
    r = run(*base, "-L", tmp_path / "w.bed", "-O", tmp_path / "w_out.tsv", "--variants", tmp_path / "v.tsv", "--variation-out", tmp_path / "wo.tsv")  # the TSV form
    assert r.returncode == 0 and (tmp_path / "wo.tsv").read_bytes() == (tmp_path / "vo.tsv").read_bytes()
    # the bounds filter before the search: population-robust
    by, _, cost, _ = va.unpack_variation_row(rows)
    bound = va.variant_weight(0.01)
    keep = (cost <= bound) & (by[:, 3] == 0)
    assert 0 < keep.sum() < len(keep)
    r = run(*base, "-L", tmp_path / "k.bed", "-O", tmp_path / "k_out.tsv", "--variants", tmp_path / "v.vcf", "--variant-af", "AF", "--max-variant-cost", bound,
            "--max-variants-by-zone", "255,255,255,0", "--variation-out", tmp_path / "ko.tsv")
    assert r.returncode == 0, r.stderr
    plain_bed, plain_rows = lines_of("plain.bed"), lines_of("plain.tsv")
    assert lines_of("k.bed") == [ln for ln, k in zip(plain_bed, keep) if k]
    assert lines_of("k_out.tsv") == [plain_rows[0]] + [ln for ln, k in zip(plain_rows[1:], keep) if k]
    k_rows, k_pairs, _, _ = gen.variation((codes[keep], loci[keep]), "SpCas9", var)
    assert lines_of("ko.tsv") == listing([i for i, k in zip(ids, keep) if k], k_rows, k_pairs)
    for args, text in (((*base, "--variant-af", "AF"), "give --variants"), ((*base, "--max-variant-cost", "5"), "give --variants"),
                       ((*base[:7], "-B", tmp_path / "plain.bed", "--variants", tmp_path / "v.vcf"), "give -E"),
                       ((*base, "--variants", tmp_path / "v.vcf", "-D", "0,0"), "one device"),
                       ((*base, "--variants", tmp_path / "v.vcf", "--variant-seed", "21"), "--variant-seed takes"),
                       ((*base, "--variants", tmp_path / "v.vcf", "--max-variant-cost", "-1"), "--max-variant-cost takes"),
                       ((*base, "--variants", tmp_path / "v.vcf", "--max-variants-by-zone", "1,2,3"), "--max-variants-by-zone takes"),
                       ((*base, "--variants", tmp_path / "v.vcf", "--max-variants-by-zone", "1,2,3,256"), "--max-variants-by-zone takes"),
                       ((*base, "--variants", tmp_path / "v.vcf", "--require-variant-zones", "tail"), "--require-variant-zones takes")):
        r = run(*args)
        assert r.returncode != 0 and text in r.stderr, (args, r.stderr)
    (tmp_path / "bad.tsv").write_text("chr9\t5\tA\tC\n")
    r = run(*base, "--variants", tmp_path / "bad.tsv")
    assert r.returncode != 0 and "no sequence" in (r.stderr + r.stdout)
    r = run(*base, "--variants", tmp_path / "v.tsv", "--variant-af", "AF")
    assert r.returncode != 0 and "INFO column" in (r.stderr + r.stdout)

    # pattern_search -E --variants v.tsv --variant-seed 8 --require-variant-zones seed,pam: Cas12a, allele-specific
    pattern, proto = "TTTV" + "N" * 23, (4, 23)
    sh = va.VARIATION_SHAPES["Cas12a"]
    (tmp_path / "p.bed").write_text("".join("%s\t%d\t%d\n" % (chrom[c], a, b) for c, a, b in iv))
    found = gen.enumerate_pattern(pattern, proto, targets=iv)
    pids = ["%s:%d:%s" % (chrom[c], p, "-" if s else "+") for c, p, s in ed.loci_tuples(found.loci)]
    p_rows, p_pairs, _, p_stats = gen.variation(found, sh, var)
    p_by = va.unpack_variation_row(p_rows)[0]
    p_keep = (p_by[:, 2] > 0) | (p_by[:, 3] > 0)
    assert len(found) >= 10 and 0 < p_keep.sum() < len(p_keep) and p_stats["pairs"] >= 10
    pbase = ("pattern_search", "-i", tmp_path / "idx", "-q", pattern, "-p", "%d,%d" % proto, "-B", tmp_path / "p.bed", "-M", "2")
    r = run(*pbase, "-E", tmp_path / "pe.tsv", "-O", tmp_path / "po.tsv")
    assert r.returncode == 0, r.stderr
    pe, po = lines_of("pe.tsv"), lines_of("po.tsv")
    r = run(*pbase, "-E", tmp_path / "pev.tsv", "-O", tmp_path / "pov.tsv", "--variants", tmp_path / "v.tsv", "--variant-seed", "8", "--variation-out", tmp_path / "pv.tsv")
    assert r.returncode == 0, r.stderr
    assert lines_of("pev.tsv") == pe and lines_of("pov.tsv") == po and lines_of("pv.tsv") == listing(pids, p_rows, p_pairs)
    r = run(*pbase, "-E", tmp_path / "pek.tsv", "-O", tmp_path / "pok.tsv", "--variants", tmp_path / "v.tsv", "--variant-seed", "8",
            "--require-variant-zones", "seed,3", "--variation-out", tmp_path / "pk.tsv")
    assert r.returncode == 0, r.stderr
    assert lines_of("pek.tsv") == [pe[0]] + [ln for ln, k in zip(pe[1:], p_keep) if k]
    assert lines_of("pok.tsv") == [po[0]] + [ln for ln, k in zip(po[1:], p_keep) if k]
    k_rows, k_pairs, _, _ = gen.variation((found.codes[p_keep], found.loci[p_keep]), sh, var)
    assert lines_of("pk.tsv") == listing([i for i, k in zip(pids, p_keep) if k], k_rows, k_pairs)
    r = run(*pbase[:5], "-R", tmp_path / "g.fa", "-M", "2", "-O", tmp_path / "x.tsv", "--variants", tmp_path / "v.tsv")
    assert r.returncode != 0 and "give -E" in (r.stderr + r.stdout)
    gen.close()
