"""Restriction sites and IUPAC motifs on the device (vsc_loci_motifs, vsc_guides_motifs, vsc_pattern_guides_motifs and the two
filters): bit for bit what the definition gives when it is applied locus by locus on STRINGS (tests/motif_cases.py).  Integers,
so there is no tolerance: the rows are compared as uint64, the undefined row included."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import motif_cases as mc
import varscot_amd as va
import wide_cases as wc
from helpers import random_seq, revcomp
from varscot_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "varscot_amd", "bin")
FILTER_TILE = 1024  # candidates per wave of the filter's passes (include/varscot_hip.h)
DROP_FRONT, DROP_BACK = 2, 1  # words the partial object of the small genome does not hold
NO_LIMITS = mc.Limits(0, 0, 0, False)
# (shape, motif set, flank case) whose small genome is walked locus by locus
SMALL = [("SpCas9", "cloning", "short"), ("Cas12a", "iupac", "both16"), ("c64", "iupac", "left16"), ("bare", "cloning", "right16"),
         ("n12_site16", "iupac", "none"), ("zone_last", "one", "both16")]


@pytest.fixture(scope="module")
def ctx():
    c = va.Context(0)
    yield c
    c.close()


def loci_tuples(loci):
    return [(int(c), int(p), int(s)) for c, p, s in zip(loci["contig"], loci["pos"], loci["strand"])]


def counts(stats):
    return {k: stats[k] for k in mc.CLASSES}


def any_counts(rows):
    u = va.unpack_motif_row(rows)
    return {"any_construct": int((u["construct"] != 0).sum()), "any_cut": int((u["cut"] != 0).sum()), "any_cut_only": int((u["cut_only"] != 0).sum())}


def middling(mask, n_motifs):
    """The motif whose bit is set in closest to half of the rows that hold any bit at all: a limit on it splits the candidates."""
    per = np.array([int(((mask >> np.uint64(m)) & np.uint64(1)).sum()) for m in range(n_motifs)])
    return int(np.argmin(np.abs(per - len(mask) / 2)))


def splitting(want, candidates):
    """The first of the candidate limits that keeps some and drops some of the defined rows - found on the strings alone."""
    defined = int((want[:, 0] != mc.UNDEF).sum())
    for lim in candidates:
        if 0 < sum(mc.keep(r, lim) for r in want) < defined:
            return lim
    raise AssertionError("no candidate limit splits these rows")


def struct_limits(lim):
    return _lib.MotifLimits(lim.forbid_construct, lim.forbid_context, lim.require_cut, va.MOTIF_CUT_ONLY if lim.cut_only else 0)


class Guides:
    """A vsc_guides (or, pattern=True, a vsc_pattern_guides) handle and its motif calls."""

    def __init__(self, ctx, handle, pattern=False):
        self.ctx, self.h, self.pattern = ctx, handle, pattern
        L = va.lib()
        kind = "vsc_pattern_guides" if pattern else "vsc_guides"
        self.fn = {k: getattr(L, "%s_%s" % (kind, k)) for k in ("count", "data", "free", "motifs", "filter_motifs")}

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

    def rows(self, gen, shape, ms, left, right, totals=False):
        rows, st = np.empty((len(self), 3), dtype=np.uint64), _lib.MotifStats()
        tot = np.full((len(ms), 3), 9, dtype=np.uint64)
        lf, rf = va.api._motif_flank(left, "left"), va.api._motif_flank(right, "right")
        sh = shape._struct()
        _lib.check(self.fn["motifs"](self.ctx._h, gen._h, self.h, C.byref(sh), lf, len(lf), rf, len(rf), ms._array(), len(ms), _lib.ptr(rows),
                                     _lib.ptr(tot) if totals else None, C.byref(st)), self.ctx._h)
        return (rows, tot, st.as_dict()) if totals else (rows, st.as_dict())

    def filter_code(self, gen, shape, ms, left, right, lim):
        out = C.c_void_p()
        lf, rf = va.api._motif_flank(left, "left", validate=False), va.api._motif_flank(right, "right", validate=False)
        sh = shape._struct()
        return self.fn["filter_motifs"](self.ctx._h, gen._h, self.h, C.byref(sh), lf, len(lf), rf, len(rf), ms._array(), len(ms), C.byref(lim),
                                        C.byref(out)), out

    def filter(self, gen, shape, ms, left, right, lim):
        code, out = self.filter_code(gen, shape, ms, left, right, struct_limits(lim))
        _lib.check(code, self.ctx._h)
        return Guides(self.ctx, out, self.pattern)

    def close(self):
        if self.h:
            self.fn["free"](self.h)
            self.h = None


# ---- 1. every locus of the small genome ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(ctx):
    """Per (shape, motif set, flank case): the small genome resident - whole, and as an object that lacks the first two words
    and the last one - every locus of it, and the expected rows, computed once."""
    cache = {}

    def get(name, set_name, flanks):
        key = (name, set_name, flanks)
        if key not in cache:
            contigs = mc.small_genome(name)
            packed = va.PackedGenome.from_sequences(list(contigs))
            loci = mc.every_locus(contigs)
            sl = slice(DROP_FRONT, packed.n_words - DROP_BACK)
            part = va.Genome.from_shard(ctx, packed.hi[sl], packed.lo[sl], packed.nmask[sl], DROP_FRONT, sl.stop - sl.start, packed.contigs)
            entries = mc.MOTIF_SETS[set_name]
            cache[key] = {"contigs": contigs, "packed": packed, "gen": ctx.load_genome(packed), "part": part, "loci": loci,
                          "arr": mc.locus_array(loci), "resident": (32 * sl.start, 32 * sl.stop), "want": {}, "shape": mc.SHAPE_OF[name],
                          "sh": mc.va_shape(mc.SHAPE_OF[name]), "entries": entries, "ms": va.motifs(entries), "left": mc.FLANKS[flanks][0],
                          "right": mc.FLANKS[flanks][1]}
        return cache[key]

    def want(name, set_name, flanks, partial=False):
        s = get(name, set_name, flanks)
        if partial not in s["want"]:
            s["want"][partial] = mc.expected(s["contigs"], s["loci"], s["shape"], s["left"], s["right"], s["entries"], s["resident"] if partial else None)
        return s["want"][partial]

    get.want = want
    yield get
    for s in cache.values():
        s["gen"].close()
        s["part"].close()


@pytest.mark.parametrize("name,set_name,flanks", SMALL, ids=["-".join(p) for p in SMALL])
def test_every_locus_of_a_small_genome(small, name, set_name, flanks):
    s = small(name, set_name, flanks)
    shape = s["shape"]
    want, want_stats, texts = small.want(name, set_name, flanks, partial=True)
    # what the fixture is for, on the restatement alone
    flanked = shape.up or shape.down
    assert all(want_stats[k] >= 5 for k in mc.CLASSES if k != "off_contig") and (want_stats["off_contig"] >= 5) == bool(flanked), want_stats
    u = va.unpack_motif_row(want)
    assert (u["cut"] != 0).sum() >= 3 and (u["elsewhere"] != 0).sum() >= 3 and (u["construct"] != 0).sum() >= 3 and (u["cut_only"] != 0).any()
    if set_name != "iupac":  # (its short motifs occur in every context)
        assert (u["defined"] & ((u["cut"] | u["elsewhere"] | u["construct"]) == 0)).any()
    for strand in (0, 1):  # the planted contexts are met on both strands
        on = {t for l, t in zip(s["loci"], texts) if l[2] == strand and t is not None}
        assert len(on) > 60 and len(on & {x for _, x, _, _, _, _ in mc.planted(name, "both16")}) >= 3
    got, stats = s["part"].motifs(s["arr"], s["sh"], s["ms"], s["left"], s["right"], allow_partial=True)
    assert got.dtype == np.uint64 and got.shape == want.shape
    assert counts(stats) == want_stats and sum(want_stats.values()) == len(s["loci"])
    assert got.tobytes() == want.tobytes()
    assert {k: stats[k] for k in ("any_construct", "any_cut", "any_cut_only")} == any_counts(want)
    # the whole genome: nothing is missing, and what was resident has the same row; the totals are the sum over the rows
    whole, whole_stats, _ = small.want(name, set_name, flanks)
    got, tot, stats = s["gen"].motifs(s["arr"], s["sh"], s["ms"], s["left"], s["right"], totals=True)
    assert counts(stats) == whole_stats and stats["not_resident"] == 0 and got.tobytes() == whole.tobytes()
    assert tot.tobytes() == mc.totals_of(whole, len(s["ms"])).tobytes() and tot.any()
    defined = want[:, 0] != mc.UNDEF
    assert (whole[defined] == want[defined]).all()
    with pytest.raises(ValueError) as e:
        s["part"].motifs(s["arr"], s["sh"], s["ms"], s["left"], s["right"])
    assert "not resident" in str(e.value)


def test_sixty_three_motifs_and_bit_62(small):
    s = small("SpCas9", "cloning", "short")
    loci = [l for l in s["loci"] if l[0] == 3][::3]
    arr = mc.locus_array(loci)
    for entries in (mc.full_set(), mc.never_set()):
        want, want_stats, _ = mc.expected(s["contigs"], loci, s["shape"], "CACCG", "GTTT", entries)
        got, tot, stats = s["gen"].motifs(arr, s["sh"], va.motifs(entries), "CACCG", "GTTT", totals=True)
        assert got.tobytes() == want.tobytes() and counts(stats) == want_stats
        assert tot.tobytes() == mc.totals_of(want, 63).tobytes()
        u = va.unpack_motif_row(want)
        assert ((u["cut"] | u["elsewhere"]) >> np.uint64(62)).any() and not (want[want[:, 0] != mc.UNDEF] >> np.uint64(63)).any()


def test_invalid_loci_are_classed_and_never_followed(small):
    s = small("SpCas9", "cloning", "short")
    n_contigs, main = len(s["contigs"]), 3
    length = len(s["contigs"][main])
    bad = [(n_contigs, 0, 0), (0xFFFFFFFF, 0, 0), (0xFFFFFFFF, 0xFFFFFFFF, 1), (main, 100, 2), (main, 100, 0xFFFFFFFF), (main, length - 22, 0),
           (main, length - 22, 1), (main, 0xFFFFFFFF, 0), (main + 1, 0xFFFFFFFF, 1), (0, 7, 0), (main, 0xFFFFFFFF - 22, 0)]
    off = [(main, 15, 0), (main, 15, 1), (main, length - 23 - 15, 0), (main, length - 23, 1), (1, 0, 0)]
    loci = bad + off + [(main, 100, 0), (main, 16, 0), (main, length - 23 - 16, 1)]
    want, want_stats, _ = mc.expected(s["contigs"], loci, s["shape"], s["left"], s["right"], s["entries"])
    assert want_stats["invalid"] == len(bad) and want_stats["off_contig"] == len(off) and want_stats["defined"] + want_stats["has_n"] == 3
    got, stats = s["gen"].motifs(mc.locus_array(loci), s["sh"], s["ms"], s["left"], s["right"])
    assert counts(stats) == want_stats and got.tobytes() == want.tobytes() and (got[:len(bad) + len(off)] == mc.UNDEF).all()


def test_nothing_to_score(ctx, small):
    s = small("SpCas9", "cloning", "short")
    got, tot, stats = s["gen"].motifs(mc.locus_array([]), s["sh"], s["ms"], s["left"], s["right"], totals=True)
    assert got.shape == (0, 3) and counts(stats) == dict.fromkeys(mc.CLASSES, 0) and not tot.any()
    t = ctx.timing()
    assert t["sites"] == 0 and t["score_ms"] == 0 and t["total_ms"] == 0 and t["genome_bytes"] == 0


# ---- 2. more candidates than one launch has lanes, more tiles than it has waves; the grid's cap -------------------------------
def launch_waves():
    """The waves of a launch capped as the cells' grids are (wide_cases): CUs x 8 workgroups of 4 waves."""
    return torch.cuda.get_device_properties(0).multi_processor_count * wc.GROUPS_PER_CU * wc.WAVES_PER_GROUP


def test_more_candidates_than_a_launch_has_lanes(small):
    key = ("Cas12a", "iupac", "both16")
    s = small(*key)
    want, _, _ = small.want(*key, partial=True)
    n, m = launch_waves() * 64 + 77, len(s["loci"])
    assert n > 3 * m  # every lane meets more than one tiling of the loci
    idx = np.arange(n) % m
    got, tot, stats = s["part"].motifs(s["arr"][idx], s["sh"], s["ms"], s["left"], s["right"], totals=True, allow_partial=True)
    assert got.tobytes() == want[idx].tobytes()
    cls = np.array([mc.classify(s["contigs"], l, s["shape"], s["resident"])[0] for l in s["loci"]])[idx]
    per = {k: int(v) for k, v in zip(*np.unique(cls, return_counts=True))}
    assert counts(stats) == {k: per.get(k, 0) for k in mc.CLASSES} and sum(counts(stats).values()) == n
    # the totals of the repeated loci: every locus counted as often as it occurs
    times = np.bincount(idx, minlength=m).astype(np.uint64)
    per_locus = np.stack([mc.totals_of(want[i:i + 1], len(s["ms"])) for i in range(m)])
    assert tot.tobytes() == (per_locus * times[:, None, None]).sum(axis=0).astype(np.uint64).tobytes()
    assert {k: stats[k] for k in ("any_construct", "any_cut", "any_cut_only")} == any_counts(want[idx])


def test_one_workgroup_per_cu_takes_many_steps_to_the_same_bytes(ctx, small):
    L = va.lib()
    key = ("SpCas9", "cloning", "short")
    s = small(*key)
    want, _, _ = small.want(*key)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    m = len(s["loci"])
    n = cus * 256 * 5 + 131  # five grid-stride steps of every workgroup and a partial one at one workgroup per CU
    idx = np.arange(n) % m
    got = {}
    try:
        for groups in (0, 1, 3, 64, 0):
            assert L.vsc_debug_motif_groups_per_cu(ctx._h, groups) == 0
            rows, tot, stats = s["gen"].motifs(s["arr"][idx], s["sh"], s["ms"], s["left"], s["right"], totals=True)
            stats = {k: v for k, v in stats.items() if not k.endswith("_ms")}
            got[groups] = (rows.tobytes(), tot.tobytes(), tuple(sorted(stats.items())))
    finally:
        L.vsc_debug_motif_groups_per_cu(ctx._h, 0)
    assert got[0][0] == want[idx].tobytes() and len(set(got.values())) == 1
    assert sum(v for k, v in got[1][2] if k in mc.CLASSES) == n
    assert L.vsc_debug_motif_groups_per_cu(ctx._h, 65) == -22 and L.vsc_debug_motif_groups_per_cu(None, 1) == -22


def test_filter_over_more_tiles_than_a_launch_has_waves(ctx, small):
    key = ("SpCas9", "cloning", "short")
    s = small(*key)
    want, _, _ = small.want(*key)
    m = len(s["loci"])
    n = (launch_waves() + 3) * FILTER_TILE + 77  # the last tile is a partial one
    idx = np.arange(n) % m
    defined = want[:, 0] != mc.UNDEF
    lim = mc.Limits(1, 0, 0, False)
    keep = np.array([mc.keep(r, lim) for r in want])
    assert 0 < keep.sum() < defined.sum()
    codes = np.arange(n, dtype=np.uint64) * np.uint64(3)  # (the filter copies codes, it does not read them)
    g = Guides.from_arrays(ctx, codes, s["arr"][idx])
    out = g.filter(s["gen"], s["sh"], s["ms"], s["left"], s["right"], lim)
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
    """A 9 kb random genome with NGG sites (and CCN sites, their '-' form) at and next to the contig ends, and the cloning
    enzymes' sites inside and beside some protospacers."""
    rng = np.random.default_rng(78)
    contigs = []
    for n in (5000, 2500, 1500):
        t = list(random_seq(rng, n))
        for p in (0, 2, 5, n - 23, n - 25, n - 29):
            site = random_seq(rng, 21) + "GG"
            t[p:p + 23] = site if p % 2 else revcomp(site)
        for p in (0, n - 23):
            t[p + 21:p + 23] = "GG"
            t[p:p + 2] = "CC"
        for k, p in enumerate(range(200, n - 200, 150)):
            word = mc.CLONING[k % 3][1]
            site = mc.put(random_seq(rng, 21) + "GG", (k * 5) % 15, word if k % 2 else revcomp(word))
            t[p:p + 23] = site if k % 4 < 2 else revcomp(site)
        contigs.append("".join(t))
    packed = va.PackedGenome.from_sequences(contigs)
    gen = ctx.load_genome(packed)
    yield {"contigs": contigs, "packed": packed, "gen": gen, "ms": va.motifs(mc.CLONING), "left": "CACCG", "right": "GTTTTAGAGC"}
    gen.close()


def test_enumerated_guides_get_their_rows_where_they_lie(planted):
    gen, ms, lf, rf, shape = planted["gen"], planted["ms"], planted["left"], planted["right"], mc.SHAPE_OF["SpCas9"]
    kw = dict(motifs="SpCas9", motif_set=ms, motif_left=lf, motif_right=rf)
    plain = gen.enumerate_guides()
    codes, loci, rows = gen.enumerate_guides(**kw)
    assert codes.tobytes() == plain[0].tobytes() and loci.tobytes() == plain[1].tobytes() and len(codes) > 500
    want, want_stats, _ = mc.expected(planted["contigs"], loci_tuples(loci), shape, lf, rf, mc.CLONING)
    assert want_stats["off_contig"] >= 6 and want_stats["defined"] + want_stats["off_contig"] == len(codes)  # the sites at the contig ends
    assert rows.dtype == np.uint64 and rows.tobytes() == want.tobytes()
    u = va.unpack_motif_row(want)
    assert (u["construct"] != 0).sum() >= 10 and (u["cut_only"] != 0).sum() >= 3 and (u["elsewhere"] != 0).sum() >= 10
    by_loci, stats = gen.motifs(loci, "SpCas9", ms, lf, rf)
    assert by_loci.tobytes() == want.tobytes() and counts(stats) == want_stats
    assert gen.motifs((codes, loci), va.MOTIF_SHAPES["SpCas9"], mc.CLONING, lf, rf)[0].tobytes() == want.tobytes()
    # N x 21 + GG under the pattern enumeration: the same sites, the same rows
    found, prows = gen.enumerate_pattern("N" * 21 + "GG", (0, 20), **kw)
    assert found.loci.tobytes() == loci.tobytes() and prows.tobytes() == want.tobytes()
    assert gen.motifs(found, "SpCas9", ms, lf, rf)[0].tobytes() == want.tobytes()
    # the motif rows come last of all, after the fold rows
    both = gen.enumerate_guides(edit="CBE", fold="SpCas9", **kw)
    assert len(both) == 5 and both[1].tobytes() == loci.tobytes() and both[4].tobytes() == want.tobytes()
    assert both[3].tobytes() == gen.enumerate_guides(fold="SpCas9")[2].tobytes() and both[2].tobytes() == gen.enumerate_guides(edit="CBE")[2].tobytes()
    for bad in (dict(motifs="Cas12a", motif_set=ms), dict(motif_set=ms), dict(motif_left="ACGT"), dict(forbid_motifs=1), dict(cut_only=True),
                dict(motifs="SpCas9"), dict(motifs="SpCas9", motif_set=ms, forbid_motifs=8), dict(motifs="SpCas9", motif_set=ms, motif_left="ACGN"),
                dict(motifs="SpCas9", motif_set=ms, cut_only=True)):
        with pytest.raises(ValueError):
            gen.enumerate_guides(**bad)
    with pytest.raises(ValueError):
        gen.enumerate_pattern("N" * 21 + "GG", (0, 20), require_cut_motifs="BsmBI")


@pytest.mark.parametrize("pattern,proto,name", [("N" * 14 + "GG", (2, 12), "n12_site16"), ("TTTV" + "N" * 23, (4, 23), "Cas12a"),
                                                ("N" * 30 + "GG", (0, 32), "c64")], ids=["site16", "Cas12a", "site32"])
def test_pattern_candidates_at_other_site_lengths(planted, pattern, proto, name):
    gen = planted["gen"]
    shape, sh = mc.SHAPE_OF[name], mc.va_shape(mc.SHAPE_OF[name])
    entries, lf, rf = mc.MOTIF_SETS["iupac"], "TTGTGGAAAGGACGAA", "GUUU"
    assert len(pattern) == shape.site_len and proto == (shape.proto_start, shape.proto_len)
    targets = [(0, 0, 1200), (1, 1900, 2500), (2, 0, 300)]
    plain = gen.enumerate_pattern(pattern, proto, targets=targets)
    kw = dict(motifs=sh, motif_set=entries, motif_left=lf, motif_right=rf)
    found, rows = gen.enumerate_pattern(pattern, proto, targets=targets, **kw)
    assert found.codes.tobytes() == plain.codes.tobytes() and found.loci.tobytes() == plain.loci.tobytes() and 30 < len(found) < 700
    want, want_stats, _ = mc.expected(planted["contigs"], loci_tuples(found.loci), shape, lf, rf, entries)
    assert want_stats["defined"] > 20 and rows.tobytes() == want.tobytes()
    # the limits, through the wrapper: the survivors in input order, their rows; only the survivors are searched
    ms = va.motifs(entries)
    u = va.unpack_motif_row(want[want[:, 0] != mc.UNDEF])
    every = (1 << len(ms)) - 1
    a, b = middling(u["construct"], len(ms)), middling(u["cut"] | u["elsewhere"], len(ms))
    lim = splitting(want, [mc.Limits(1 << a, 1 << b, every, True), mc.Limits(1 << a, 0, every, True), mc.Limits(1 << a, 1 << b, every, False),
                           mc.Limits(1 << a, 0, 0, False)])
    keep = np.array([mc.keep(r, lim) for r in want])
    kw.update(forbid_motifs=[ms.names[a]], forbid_context_motifs=lim.forbid_context or None, require_cut_motifs=lim.require_cut or None,
              cut_only=lim.cut_only or None)
    kept, krows = gen.enumerate_pattern(pattern, proto, targets=targets, **kw)
    assert kept.codes.tobytes() == found.codes[keep].tobytes() and kept.loci.tobytes() == found.loci[keep].tobytes()
    assert krows.tobytes() == want[keep].tobytes()
    if name == "Cas12a":
        d_found, d_rows, d_sites = gen.design_pattern(pattern, proto, 2, targets=targets, **kw)
        assert d_found.codes.tobytes() == kept.codes.tobytes() and d_sites.tobytes() == want[keep].tobytes()
        _, all_rows = gen.design_pattern(pattern, proto, 2, targets=targets)
        assert d_rows.tobytes() == all_rows[keep].tobytes()
        pick = va.PickShape(site_len=27, k=2, spacing=5)
        out = gen.design_pattern(pattern, proto, 2, targets=targets, pick=pick, pick_by=["rflp"], motifs=sh, motif_set=entries)
        assert len(out) == 5 and out[2].tobytes() == gen.enumerate_pattern(pattern, proto, targets=targets, motifs=sh, motif_set=entries)[1].tobytes()


def test_calls_refuse_before_anything_is_written(ctx, planted, small):
    L = va.lib()
    gen, ms = planted["gen"], planted["ms"]
    p = va.api._enum_params("GG", "both", (0, 0), 0, 0)
    h = C.c_void_p()
    _lib.check(L.vsc_guides_enumerate(ctx._h, gen._h, None, C.byref(p), C.byref(h)), ctx._h)
    g = Guides(ctx, h)
    rows = np.full((len(g), 3), 7, dtype=np.uint64)
    tot = np.full((3, 3), 7, dtype=np.uint64)
    ok = va.MOTIF_SHAPES["SpCas9"]
    arr = mc.locus_array([(0, 100, 0)])
    none = struct_limits(NO_LIMITS)

    def calls(shape=ok, left=b"CACCG", a=None, right=b"GTTT", b=None, motifs=ms, n_motifs=None, ctx_h=ctx._h, gen_h=gen._h, guides=g.h, loci=arr,
              out_rows=rows, lim=none, which=(0, 1, 2)):
        sh = C.byref(shape._struct()) if shape is not None else None
        a = len(left or b"") if a is None else a
        b = len(right or b"") if b is None else b
        marr = motifs._array() if motifs is not None else None
        m = (len(motifs) if motifs is not None else 0) if n_motifs is None else n_motifs
        out = C.c_void_p()
        made = [lambda: L.vsc_guides_motifs(ctx_h, gen_h, guides, sh, left, a, right, b, marr, m, _lib.ptr(out_rows) if out_rows is not None else None,
                                            _lib.ptr(tot), None),
                lambda: L.vsc_loci_motifs(ctx_h, gen_h, _lib.ptr(loci) if loci is not None else None, 1, sh, left, a, right, b, marr, m,
                                          _lib.ptr(out_rows) if out_rows is not None else None, _lib.ptr(tot), None),
                lambda: L.vsc_guides_filter_motifs(ctx_h, gen_h, guides, sh, left, a, right, b, marr, m, C.byref(lim) if lim is not None else None,
                                                   C.byref(out))]
        return [made[k]() for k in which], out  # (only the calls the case is about: another one may be in order and write)

    def refused(which=(0, 1, 2), **kw):
        codes, out = calls(which=which, **kw)
        return all(c == -22 for c in codes) and (rows == 7).all() and (tot == 7).all() and not out.value

    assert refused(which=(0, 2), shape=va.MOTIF_SHAPES["Cas12a"]) and "site_len" in L.vsc_last_error(ctx._h).decode()
    base = dict(site_len=23, spacer=(0, 20), cut=(16, 2), up=16, down=16)
    for kw in ({"site_len": 15, "spacer": (0, 12), "cut": (0, 1)}, {"site_len": 33}, {"up": 17}, {"down": 17}, {"site_len": 32, "up": 16, "down": 16, "spacer": (0, 33)},
               {"spacer": (0, 11)}, {"spacer": (4, 20)}, {"cut": (16, 0)}, {"cut": (16, 17)}, {"cut": (22, 2)}):  # every shape refusal, by the library
        assert refused(shape=va.MotifShape(validate=False, **dict(base, **kw))), kw
    for k in range(5):
        reserved = va.MotifShape(**base)
        reserved.reserved = tuple(int(i == k) for i in range(5))
        assert refused(shape=reserved)
    assert refused(left=b"ACGN") and refused(right=b"A" * 17) and "flank" in L.vsc_last_error(ctx._h).decode()
    assert refused(left=None, a=3) and refused(right=None, b=1)
    raw = lambda entries: va.motifs(entries, validate=False)  # noqa: E731
    for entries in ([("x", "CGTXTC")], [("n", "NNNN")], [("s", "A")], [("l", "A" * 17)], [("m%d" % i, "ACGT") for i in range(64)]):
        assert refused(motifs=raw(entries)), entries
    flagged = va.motifs(mc.CLONING)
    flagged.flags[1] = 2
    assert refused(motifs=flagged) and refused(motifs=ms, n_motifs=0) and refused(motifs=None, n_motifs=1)
    for lim in (mc.Limits(8, 0, 0, False), mc.Limits(0, 8, 0, False), mc.Limits(0, 0, 1 << 63, False)):  # a bit at or above M
        assert refused(which=(2,), lim=struct_limits(lim)) and "limits" in L.vsc_last_error(ctx._h).decode()
    bad_flag = struct_limits(NO_LIMITS)
    bad_flag.flags = 2
    bad_reserved = struct_limits(NO_LIMITS)
    bad_reserved.reserved = 1
    assert refused(which=(2,), lim=bad_flag) and refused(which=(2,), lim=bad_reserved) and refused(which=(2,), lim=None)
    assert refused(shape=None) and refused(which=(0, 1), out_rows=None) and refused(gen_h=None) and refused(which=(0, 2), guides=None)
    assert refused(which=(1,), loci=None)
    st, marr = ok._struct(), ms._array()
    assert L.vsc_guides_filter_motifs(ctx._h, gen._h, g.h, C.byref(st), b"", 0, b"", 0, marr, 3, C.byref(none), None) == -22
    other = va.Context(0)  # a genome, or an object, of another context is refused
    assert refused(which=(1,), ctx_h=other._h)
    s = small("SpCas9", "cloning", "short")
    gen2 = other.load_genome(s["packed"])
    assert refused(which=(0, 2), ctx_h=other._h, gen_h=gen2._h) and "another context" in L.vsc_last_error(other._h).decode()
    gen2.close()
    other.close()
    with pytest.raises(va.VarscotError):
        gen.motifs(arr, va.MotifShape(validate=False, **dict(base, cut=(22, 2))), ms)
    codes, out = calls()  # and with everything in order the three calls work
    assert codes == [0, 0, 0] and out.value and not (rows == 7).all() and not (tot == 7).any()
    L.vsc_guides_free(out)
    g.close()


# ---- 4. the filter --------------------------------------------------------------------------------------------------------------
def test_filter_limits_and_what_takes_the_result(ctx, small, planted):
    key = ("SpCas9", "cloning", "short")  # (a vsc_guides object: sites of 23)
    s = small(*key)
    sh, ms, lf, rf = s["sh"], s["ms"], s["left"], s["right"]
    want, _, _ = small.want(*key)
    defined = want[:, 0] != mc.UNDEF
    n = len(s["loci"])
    codes = np.arange(n, dtype=np.uint64) * np.uint64(5)
    g = Guides.from_arrays(ctx, codes, s["arr"])
    u = va.unpack_motif_row(want)
    ud = va.unpack_motif_row(want[defined])
    fc_, fx, rc = (1 << middling(mask, len(ms)) for mask in (ud["construct"], ud["cut"] | ud["elsewhere"], ud["cut"]))
    trials = [NO_LIMITS, mc.Limits(fc_, 0, 0, False), mc.Limits(0, fx, 0, False), mc.Limits(0, 0, rc, False), mc.Limits(0, 0, rc, True),
              mc.Limits(fc_, fx, rc, True), mc.Limits((1 << len(ms)) - 1, 0, 0, False), mc.Limits(0, 0, (1 << len(ms)) - 1, True)]
    kept_by = {}
    for lim in trials:  # each limit alone and together, against the truth table's rule
        keep = np.array([mc.keep(r, lim) for r in want])
        out = g.filter(s["gen"], sh, ms, lf, rf, lim)
        got_codes, got_loci = out.arrays()
        out.close()
        assert got_codes.tobytes() == codes[keep].tobytes() and got_loci.tobytes() == s["arr"][keep].tobytes(), lim
        kept_by[lim] = keep
    assert kept_by[NO_LIMITS].sum() == defined.sum()
    for lim in trials[1:5]:
        assert 0 < kept_by[lim].sum() < defined.sum(), lim
    assert kept_by[trials[5]].sum() <= kept_by[trials[4]].sum() < kept_by[trials[3]].sum()  # CUT_ONLY drops those that hold the motif elsewhere too
    # an empty result is a result; the host-only object goes the host's way, to the same bytes
    nothing = Guides.from_arrays(ctx, codes[~defined], s["arr"][~defined])
    empty = nothing.filter(s["gen"], sh, ms, lf, rf, NO_LIMITS)
    assert len(empty) == 0 and empty.rows(s["gen"], sh, ms, lf, rf)[0].shape == (0, 3)
    empty.close()
    nothing.close()
    host = Guides.from_arrays(ctx, codes, s["arr"], on_device=False)
    h_rows, h_tot, h_stats = host.rows(s["gen"], sh, ms, lf, rf, totals=True)
    assert h_rows.tobytes() == want.tobytes() and h_stats["defined"] == defined.sum() and h_tot.tobytes() == mc.totals_of(want, len(ms)).tobytes()
    h_out = host.filter(s["gen"], sh, ms, lf, rf, trials[5])
    assert h_out.arrays()[0].tobytes() == codes[kept_by[trials[5]]].tobytes()
    h_out.close()
    host.close()
    g.close()

    # the survivors feed the search as the candidates selected on the host do, and the pick by "rflp"
    gen, pms, plf, prf = planted["gen"], planted["ms"], planted["left"], planted["right"]
    kw = dict(motifs="SpCas9", motif_set=pms, motif_left=plf, motif_right=prf)
    pcodes, ploci, prows = gen.enumerate_guides(**kw)
    lim = mc.Limits(7, 0, 0, False)  # the cloning case: none of the three enzymes' sites in the construct
    keep = np.array([mc.keep(r, lim) for r in prows])
    assert 0 < keep.sum() < (prows[:, 0] != mc.UNDEF).sum()
    fkw = dict(kw, forbid_motifs=["BsmBI", "BbsI", "BsaI"])
    k_codes, k_loci, k_rows = gen.enumerate_guides(**fkw)
    assert k_codes.tobytes() == pcodes[keep].tobytes() and k_loci.tobytes() == ploci[keep].tobytes() and k_rows.tobytes() == prows[keep].tobytes()
    rows_all = gen.summarize(pcodes, 2, exclude=ploci)
    assert gen.summarize(k_codes, 2, exclude=k_loci).tobytes() == rows_all[keep].tobytes()
    d = gen.design(None, 2, **fkw)
    assert len(d) == 4 and d[0].tobytes() == k_codes.tobytes() and d[2].tobytes() == rows_all[keep].tobytes() and d[3].tobytes() == k_rows.tobytes()
    plain = gen.design(None, 2)
    assert len(plain) == 3 and plain[2].tobytes() == rows_all.tobytes()  # without the arguments: what it returned before
    iv = [(0, 0, 1500), (0, 2000, 4000), (1, 0, 2500), (2, 100, 1400)]
    regions = va.Regions(planted["packed"], iv, rule="inside")
    pick = va.PickShape(k=3, spacing=10)
    out = gen.design(regions, 2, fold="SpCas9", pick=pick, pick_by=["rflp", "fold", "mit"], **kw)
    r_codes, r_loci, r_rows, r_fold, r_sites, picks, n_picked = out
    spec = np.array([va.mit_specificity(x) for x in r_rows["mit_sum"]], dtype=np.float64)
    cols = [va.pick_column("rflp", r_sites), va.pick_column("fold", r_fold), va.pick_column("mit", spec)]
    key = va.pick_key(cols, [va.PICK_COLUMNS[c] for c in ("rflp", "fold", "mit")])
    w_picks, w_counts, _ = gen.pick((r_codes, r_loci), key, pick, regions=regions)
    assert picks.tobytes() == w_picks.tobytes() and n_picked.tobytes() == w_counts.tobytes() and (n_picked > 0).all()
    labels = np.array([regions.locate(c, p) for c, p, _ in loci_tuples(r_loci)])
    rflp = cols[0]
    assert len(set(rflp.tolist())) >= 2
    for t, i in enumerate(picks[:, 0]):  # more is better: the first pick of every target has the most cut-only motifs of its target
        assert labels[i] == t and rflp[i] == rflp[labels == t].max()
    with pytest.raises(ValueError):
        gen.design(regions, 2, pick=pick, pick_by=["rflp"])  # the column needs motifs=
    regions.close()


# ---- 5. repetition and the context's state ------------------------------------------------------------------------------------
def test_alternating_sets_and_flanks_leave_nothing_behind(ctx, small):
    a = small("SpCas9", "cloning", "short")
    gen, arr, n, shape = a["gen"], a["arr"], len(a["loci"]), a["shape"]
    calls = [(mc.MOTIF_SETS["cloning"], "CACCG", "GTTT"), (mc.MOTIF_SETS["iupac"], "CACCG", "GTTT"), (mc.MOTIF_SETS["cloning"], "TTGTGGAAAGGACGAA", ""),
             (mc.MOTIF_SETS["iupac"], "", "GTTTTAGAGCTAGAAA")]
    want = [mc.expected(a["contigs"], a["loci"], shape, lf, rf, entries)[0] for entries, lf, rf in calls]
    assert len({w.tobytes() for w in want}) == len(calls)

    def rows(k):
        entries, lf, rf = calls[k]
        return gen.motifs(arr, a["sh"], va.motifs(entries), lf, rf)[0]

    for k in (0, 0, 1, 0, 2, 2, 3, 1, 3, 2, 0):  # nothing of a call outlives it: no stale pattern, no stale flank
        assert rows(k).tobytes() == want[k].tobytes(), k
    # an efficiency call and a fold call between two motif calls find their tables again, and the motif call its patterns
    import efficiency_cases as ec
    import fold_cases as fc
    model = ec.build("dense", (6, 23, 6))
    lin0 = gen.efficiency(arr, model)[0]
    sc = fc.scaffold("SpCas9", 76)
    fold0 = gen.fold(arr, "SpCas9", sc)[0]
    assert rows(1).tobytes() == want[1].tobytes()
    assert gen.efficiency(arr, model)[0].view(np.uint64).tobytes() == lin0.view(np.uint64).tobytes()
    assert rows(2).tobytes() == want[2].tobytes()
    assert gen.fold(arr, "SpCas9", sc)[0].tobytes() == fold0.tobytes()
    ctx.release_scratch()
    assert rows(3).tobytes() == want[3].tobytes()
    ctx.release_scratch()
    got, stats = gen.motifs(arr, a["sh"], va.motifs(calls[0][0]), calls[0][1], calls[0][2])
    assert got.tobytes() == want[0].tobytes()
    assert stats["kernel_ms"] > 0 and stats["wall_ms"] >= stats["kernel_ms"]
    t = ctx.timing()
    assert t["score_ms"] > 0 and t["total_ms"] == t["score_ms"] and t["sites"] == n and t["genome_bytes"] == 40 * n
    for k in ("scan_ms", "prep_ms", "sort_ms", "finalize_ms", "index_ms", "pairs", "hits", "passes", "sort_bytes", "sort_levels", "list_entries"):
        assert t[k] == 0, k


# ---- 6. the tools end to end --------------------------------------------------------------------------------------------------
def test_tools_list_and_filter_their_guides(ctx, tmp_path):
    rng = np.random.default_rng(84)
    contigs = [random_seq(rng, 6000), "TTTA" + random_seq(rng, 2996)]
    for c in range(2):  # the enzymes' sites are rare in 9 kb: plant some
        t = contigs[c]
        for k, p in enumerate(range(40, len(t) - 40, 90)):
            word = mc.CLONING[k % 3][1]
            t = mc.put(t, p, word if k % 2 else revcomp(word))
        contigs[c] = t
    names = ["chr1 assembled", "chr2"]
    chrom = [n.split()[0] for n in names]
    with open(tmp_path / "g.fa", "w") as f:
        for n, s in zip(names, contigs):
            f.write(">%s\n%s\n" % (n, "\n".join(s[i:i + 60] for i in range(0, len(s), 60))))
    iv = [(0, 0, 900), (1, 100, 400), (0, 5800, 6000)]
    (tmp_path / "t.bed").write_text("".join("%s\t%d\t%d\tx\n" % (chrom[c], a, b) for c, a, b in iv))
    (tmp_path / "m.tsv").write_text("#name\ttext\tstrands\n" + "".join("%s\t%s\t2\n" % e for e in mc.CLONING) + "fwd\tCGTCTC\t1\n")
    entries = list(mc.CLONING) + [("fwd", "CGTCTC", False)]
    ms = va.motifs(entries)
    run = lambda *a: subprocess.run([os.path.join(BIN, a[0])] + [str(x) for x in a[1:]], capture_output=True, text=True, timeout=600)  # noqa: E731
    assert run("bidir_index", "-G", tmp_path / "g.fa", "-I", tmp_path / "idx").returncode == 0
    packed = va.PackedGenome.from_sequences(contigs)
    gen = ctx.load_genome(packed)
    lf, rf = "CACCG", "GUUUUAGAGC"

    def names_of(mask):
        return ",".join(ms.names_of(mask)) or "-"

    def columns(rows):
        u = va.unpack_motif_row(rows)
        return ["\t" + "\t".join(names_of(u[k][i]) for k in ("construct", "cut", "elsewhere", "cut_only")) if u["defined"][i] else "\tNA\tNA\tNA\tNA"
                for i in range(len(rows))]

    # guide_summary -E -L --motifs [...]
    regions = va.Regions(packed, iv, rule="inside")
    kw = dict(motifs="SpCas9", motif_set=ms, motif_left=lf, motif_right=rf)
    codes, loci, rows = gen.enumerate_guides(regions, **kw)
    u = va.unpack_motif_row(rows)
    assert 50 < len(codes) < 500 and not u["defined"].all() and (u["construct"] != 0).any() and (u["cut"] != 0).any()
    lim = mc.Limits(7, 0, 0, False)
    keep = np.array([mc.keep(r, lim) for r in rows])
    assert 0 < keep.sum() < u["defined"].sum()
    base = ("guide_summary", "-G", tmp_path / "g.fa", "-I", tmp_path / "idx", "-M", "2", "-E", tmp_path / "t.bed")
    r = run(*base, "-L", tmp_path / "plain.bed", "-O", tmp_path / "plain.tsv")
    assert r.returncode == 0, r.stderr
    opts = ("--motifs", tmp_path / "m.tsv", "--motif-left", lf, "--motif-right", rf)
    r = run(*base, "-L", tmp_path / "f.bed", "-O", tmp_path / "f.tsv", *opts, "--motifs-out", tmp_path / "sites.tsv")
    assert r.returncode == 0, r.stderr
    plain_bed = (tmp_path / "plain.bed").read_text().splitlines()
    plain_rows = (tmp_path / "plain.tsv").read_text().splitlines()
    assert len(plain_bed) == len(codes)
    assert (tmp_path / "f.tsv").read_bytes() == (tmp_path / "plain.tsv").read_bytes()  # --motifs adds to the listing alone
    want_bed = [ln + col for ln, col in zip(plain_bed, columns(rows))]
    assert (tmp_path / "f.bed").read_text().splitlines() == want_bed
    sites = (tmp_path / "sites.tsv").read_text().splitlines()
    assert sites[0] == "#guideId\tconstruct\tcut\telsewhere\tcutOnly"
    assert sites[1:] == [ln.split("\t")[3] + col for ln, col in zip(plain_bed, columns(rows))]
    r = run(*base, "-L", tmp_path / "k.bed", "-O", tmp_path / "k.tsv", *opts, "--motif-forbid", "BsmBI,BbsI,BsaI")
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "k.bed").read_text().splitlines() == [ln for ln, k in zip(want_bed, keep) if k]
    assert (tmp_path / "k.tsv").read_text().splitlines() == [plain_rows[0]] + [ln for ln, k in zip(plain_rows[1:], keep) if k]
    regions.close()

    # pattern_search -E --motifs: Cas12a, the genotyping filter
    pattern, proto = "TTTV" + "N" * 23, (4, 23)
    targets = [(0, 0, 3000), (1, 0, 3000)]
    (tmp_path / "p.bed").write_text("".join("%s\t%d\t%d\n" % (chrom[c], a, b) for c, a, b in targets))
    pkw = dict(motifs="Cas12a", motif_set=ms)
    found, prows = gen.enumerate_pattern(pattern, proto, targets=targets, **pkw)
    plim = mc.Limits(0, 0, 7, True)
    pkeep = np.array([mc.keep(r, plim) for r in prows])
    assert len(found) > 40 and 0 < pkeep.sum() < len(pkeep)
    pbase = ("pattern_search", "-i", tmp_path / "idx", "-q", pattern, "-p", "%d,%d" % proto, "-B", tmp_path / "p.bed", "-M", "2")
    r = run(*pbase, "-E", tmp_path / "pe.tsv", "-O", tmp_path / "po.tsv")
    assert r.returncode == 0, r.stderr
    r = run(*pbase, "-E", tmp_path / "pef.tsv", "-O", tmp_path / "pof.tsv", "--motifs", tmp_path / "m.tsv")
    assert r.returncode == 0, r.stderr
    pe = (tmp_path / "pe.tsv").read_text().splitlines()
    po = (tmp_path / "po.tsv").read_text().splitlines()
    assert len(pe) == len(found) + 1 and pe[0] == "#guide\tchrom\tpos\tstrand"
    assert (tmp_path / "pof.tsv").read_bytes() == (tmp_path / "po.tsv").read_bytes()
    want_pe = [pe[0] + "\tmotifsConstruct\tmotifsCut\tmotifsElsewhere\tmotifsCutOnly"] + [ln + col for ln, col in zip(pe[1:], columns(prows))]
    assert (tmp_path / "pef.tsv").read_text().splitlines() == want_pe
    r = run(*pbase, "-E", tmp_path / "pek.tsv", "-O", tmp_path / "pok.tsv", "--motifs", tmp_path / "m.tsv", "--motif-require-cut", "BsmBI,BbsI,BsaI",
            "--motif-cut-only", "--motifs-out", tmp_path / "psites.tsv")
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "pek.tsv").read_text().splitlines() == [want_pe[0]] + [ln for ln, k in zip(want_pe[1:], pkeep) if k]
    assert (tmp_path / "pok.tsv").read_text().splitlines() == [po[0]] + [ln for ln, k in zip(po[1:], pkeep) if k]
    assert len((tmp_path / "psites.tsv").read_text().splitlines()) == pkeep.sum() + 1
    gen.close()
