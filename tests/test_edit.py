"""Base-editor windows on the device (vsc_loci_edit, vsc_guides_edit, vsc_pattern_guides_edit and the two filters): bit for bit
what the definition gives when it is applied locus by locus in plain Python on strings (tests/edit_cases.py).  Integers, so there
is no tolerance: rows, pairs, coverage and counts are compared as they are, the undefined pair included."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import edit_cases as ed
import efficiency_cases as ec
import varscot_amd as va
import wide_cases as wc
from helpers import random_seq, revcomp
from varscot_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "varscot_amd", "bin")

MAIN_RUN = ed.MAIN  # the contig with the planted runs
TILE = 1024  # candidates per wave of the pairs' and the filter's passes (include/varscot_hip.h)
DROP_FRONT, DROP_BACK = 3, 1  # words the partial object of the small genome does not hold
COUNTS = ed.CLASSES + ("with_hit", "pairs", "targets_covered")
SHAPES = [(23, 3, 5, "C"), (23, 3, 4, "A"), (23, 0, 16, "C"), (23, 7, 16, "A"), (23, 22, 1, "C"), (16, 0, 16, "G"), (32, 16, 16, "T")]
SETS = ["none", "third", "every", "one", "one_contig"]


@pytest.fixture(scope="module")
def ctx():
    c = va.Context(0)
    yield c
    c.close()


def shape_of(t):
    return va.EditShape(site_len=t[0], window=(t[1], t[2]), base=t[3])


def counts(stats):
    return {k: stats[k] for k in COUNTS}


class Guides:
    """A vsc_guides (or, pattern=True, a vsc_pattern_guides) handle and its calls."""

    def __init__(self, ctx, handle, pattern=False):
        self.ctx, self.h, self.pattern = ctx, handle, pattern
        L = va.lib()
        kind = "vsc_pattern_guides" if pattern else "vsc_guides"
        self.fn = {k: getattr(L, "%s_%s" % (kind, k)) for k in ("count", "data", "free", "edit", "filter_edit", "filter_efficiency",
                                                                 "filter_microhomology")}

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

    def edit(self, gen, shape, targets, capacity):
        """(rows, pairs in the library's target numbering, coverage over the sorted targets, stats, status)."""
        n = len(self)
        tg = va.edit_targets(targets)[0] if targets is not None else None
        n_t = 0 if tg is None else len(tg)
        rows, pairs = np.empty((n, 2), dtype=np.uint32), np.zeros(capacity, dtype=va.EDIT_PAIR_DTYPE)
        cov = np.empty((n_t, 2), dtype=np.uint32)
        st, count, sh = _lib.EditStats(), C.c_uint64(), shape._struct()
        rc = self.fn["edit"](self.ctx._h, gen._h, self.h, C.byref(sh), _lib.ptr(tg) if n_t else None, n_t, _lib.ptr(rows), _lib.ptr(pairs),
                             capacity, C.byref(count), _lib.ptr(cov), C.byref(st))
        return rows, pairs[:min(capacity, int(count.value))], cov, st.as_dict(), rc

    def filter_code(self, gen, shape, targets, lo, hi):
        out = C.c_void_p()
        sh = shape._struct()
        tg = va.edit_targets(targets)[0] if targets is not None else None
        n_t = 0 if tg is None else len(tg)
        return self.fn["filter_edit"](self.ctx._h, gen._h, self.h, C.byref(sh), _lib.ptr(tg) if n_t else None, n_t, lo, hi, C.byref(out)), out

    def filter(self, gen, shape, targets, lo, hi):
        code, out = self.filter_code(gen, shape, targets, lo, hi)
        _lib.check(code, self.ctx._h)
        return Guides(self.ctx, out, self.pattern)

    def filter_efficiency(self, gen, model, floor):
        out = C.c_void_p()
        _lib.check(self.fn["filter_efficiency"](self.ctx._h, gen._h, self.h, model._h, floor, C.byref(out)), self.ctx._h)
        return Guides(self.ctx, out, self.pattern)

    def filter_microhomology(self, gen, shape, min_sum, permille):
        out = C.c_void_p()
        sh = shape._struct()
        _lib.check(self.fn["filter_microhomology"](self.ctx._h, gen._h, self.h, C.byref(sh), min_sum, permille, C.byref(out)), self.ctx._h)
        return Guides(self.ctx, out, self.pattern)

    def close(self):
        if self.h:
            self.fn["free"](self.h)
            self.h = None


def sorted_numbering(want, targets):
    """An expected result with the targets numbered as the LIBRARY numbers them (the place among the sorted distinct targets):
    (pairs, coverage)."""
    _, order, inverse = va.edit_targets(targets)
    pairs = want["pairs"].copy()
    pairs["target"] = inverse[pairs["target"].astype(np.int64)].astype(np.uint32)
    pairs = pairs[np.lexsort((pairs["target"], pairs["candidate"]))]
    return pairs, want["coverage"][order]


# ---- 1. every locus of the small genome ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(ctx):
    """Per site length: the small genome resident - whole, and as an object that lacks its first three words and its last one -
    every locus of it with the invalid ones behind, and per (shape, target set) the expected result, computed once."""
    cache = {}

    def get(site_len):
        if site_len not in cache:
            contigs = ed.small_genome(site_len)
            packed = va.PackedGenome.from_sequences(list(contigs))
            loci = ed.every_locus(contigs) + ed.invalid_loci(contigs)
            sl = slice(DROP_FRONT, packed.n_words - DROP_BACK)
            part = va.Genome.from_shard(ctx, packed.hi[sl], packed.lo[sl], packed.nmask[sl], DROP_FRONT, sl.stop - sl.start, packed.contigs)
            cache[site_len] = {"contigs": contigs, "packed": packed, "gen": ctx.load_genome(packed), "part": part, "loci": loci,
                               "arr": ed.locus_array(loci), "resident": (32 * sl.start, 32 * sl.stop), "sets": ed.target_sets(contigs),
                               "want": {}}
        return cache[site_len]

    def want(shape, which, partial=False):
        s = get(shape[0])
        key = (shape, which, partial)
        if key not in s["want"]:
            s["want"][key] = ed.expected(s["contigs"], s["loci"], shape, s["sets"][which], s["resident"] if partial else None)
        return s["want"][key]

    get.want = want
    yield get
    for s in cache.values():
        s["gen"].close()
        s["part"].close()


def same(got, want, targets):
    rows, pairs, coverage, stats = got
    assert rows.dtype == np.uint32 and rows.tobytes() == want["rows"].tobytes()
    assert counts(stats) == want["stats"] and sum(stats[k] for k in ed.CLASSES) == len(rows) and stats["off_contig"] == 0
    if targets is None:
        assert pairs is None and coverage is None and stats["pairs"] == 0
    else:
        assert pairs.dtype == va.EDIT_PAIR_DTYPE and pairs.tobytes() == want["pairs"].tobytes()
        assert coverage.tobytes() == want["coverage"].tobytes()


@pytest.mark.parametrize("which", SETS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda t: "%d-%d-%d-%s" % t)
def test_every_locus_of_a_small_genome(ctx, small, shape, which):
    s = small(shape[0])
    targets, sh = s["sets"][which], shape_of(shape)
    part_want, whole_want = small.want(shape, which, partial=True), small.want(shape, which)
    if shape[0] == 23:
        same(s["part"].edit(s["arr"], sh, targets, coverage=True, allow_partial=True), part_want, targets)
        same(s["gen"].edit(s["arr"], sh, targets, coverage=True), whole_want, targets)
        return
    # site_len 16 and 32: through the pattern handle, where the caller vouches for the length
    g = Guides.from_arrays(ctx, np.arange(len(s["arr"]), dtype=np.uint64), s["arr"], pattern=True)
    for gen, want in ((s["part"], part_want), (s["gen"], whole_want)):
        rows, pairs, cov, stats, rc = g.edit(gen, sh, targets, want["stats"]["pairs"] + 5)
        assert rc == 0 and rows.tobytes() == want["rows"].tobytes() and counts(stats) == want["stats"]
        if targets is not None:
            want_pairs, want_cov = sorted_numbering(want, targets)
            assert pairs.tobytes() == want_pairs.tobytes() and cov.tobytes() == want_cov.tobytes()
    g.close()


# ---- 2. the fixture holds what it is for: asserted on the restatement ---------------------------------------------------------
def test_the_fixture_is_not_vacuous(small):
    s = small(23)
    loci, contigs = s["loci"], s["contigs"]
    a = small.want((23, 3, 5, "C"), "third", partial=True)
    assert all(a["stats"][k] >= 5 for k in ("defined", "invalid", "not_resident", "has_n")) and a["stats"]["off_contig"] == 0
    assert a["stats"]["pairs"] >= 50
    per = np.bincount(a["pairs"]["candidate"], minlength=len(loci))
    assert any(per[i] == 2 and loci[i][2] == 1 for i in range(len(loci)))  # a '-' candidate with two pairs: the order test
    third = s["sets"]["third"]
    reached = {0: set(), 1: set()}
    for p in a["pairs"]:
        reached[loci[p["candidate"]][2]].add(third[p["target"]])
    assert reached[0] and reached[1] and not reached[0] & reached[1]  # '+' reaches C, '-' reaches G: never the same target
    assert all(contigs[c][p] == "C" for c, p in reached[0]) and all(contigs[c][p] == "G" for c, p in reached[1])
    cov = a["coverage"]
    assert (cov[:, 0] > 0).any() and (cov[:, 0] == 0).any() and ((cov[:, 0] == 0) == (cov[:, 1] == ed.UNDEF)).all()
    wrong = [k for k, (c, p) in enumerate(third) if contigs[c][p] in "AT"]
    assert len(wrong) > 50 and (cov[wrong, 0] == 0).all()  # a target with another letter is reached by nobody
    per_target = {}
    for q in a["pairs"]:
        key = (int(q["target"]), loci[q["candidate"]][2])
        per_target[key] = per_target.get(key, 0) + 1
    assert all(any(v >= 3 for (_, strand), v in per_target.items() if strand == st) for st in (0, 1))  # three candidates, each strand
    assert any(h and any(j + 1 in h for j in h) for h in a["hit"])  # two adjacent targets in one window: hits at j and j + 1
    assert (MAIN_RUN, 150) in third and (MAIN_RUN, 151) in third and contigs[MAIN_RUN][150:152] == "CC"
    firsts = {(c, 0) for c in range(len(contigs))} | {(c, len(t) - 1) for c, t in enumerate(contigs)}
    assert firsts <= set(third)  # targets at a contig's first and last base
    b = small.want((23, 0, 16, "C"), "every")
    assert np.bincount(b["pairs"]["candidate"]).max() >= 3
    assert (b["rows"][:, 0] == 0xFFFF).any() and (b["rows"][:, 0] == 0).any()
    by = b["pairs"]["info"] >> 8
    assert by.max() == 15 and by.min() == 0
    e = small.want((23, 7, 16, "A"), "every")
    assert (e["rows"][:, 0] == 0xFFFF).any()
    g = small.want((23, 22, 1, "C"), "every")
    assert g["stats"]["pairs"] > 0  # (every locus is a candidate here; under NGG the letter at 22 is G: test_enumerated_guides)


# ---- 3. beyond one launch ----------------------------------------------------------------------------------------------------
def launch_waves():
    """The waves of a launch capped as the cells' grids are (wide_cases): CUs x 8 workgroups of 4 waves."""
    return torch.cuda.get_device_properties(0).multi_processor_count * wc.GROUPS_PER_CU * wc.WAVES_PER_GROUP


def test_more_candidates_than_a_launch_has_lanes_and_more_tiles_than_waves(ctx, small):
    shape, which = (23, 0, 16, "C"), "one_contig"  # several pairs per candidate: runs of them cross tile boundaries
    s, sh = small(23), shape_of(shape)
    base = small.want(shape, which)
    targets = s["sets"][which]
    m = len(s["loci"])
    n = (launch_waves() + 3) * TILE + 17
    assert n > 3 * m and n > launch_waves() * 64
    idx = np.arange(n) % m
    loci = s["arr"][idx]
    rows, pairs, coverage, stats = s["gen"].edit(loci, sh, targets, coverage=True)
    assert rows.tobytes() == base["rows"][idx].tobytes()
    reps, rem = divmod(n, m)
    bp = base["pairs"]
    parts = []
    for k in range(reps + 1):
        part = (bp if k < reps else bp[bp["candidate"] < rem]).copy()
        part["candidate"] += np.uint32(k * m)
        parts.append(part)
    want_pairs = np.concatenate(parts)
    assert len(want_pairs) > 3 * TILE and np.bincount(bp["candidate"]).max() >= 3
    assert stats["pairs"] == len(want_pairs) == len(pairs) and pairs.tobytes() == want_pairs.tobytes()
    last = np.bincount(bp[bp["candidate"] < rem]["target"], minlength=len(targets))
    assert (coverage[:, 0] == reps * base["coverage"][:, 0] + last).all()
    assert reps >= 1 and (coverage[:, 1] == base["coverage"][:, 1]).all()  # (every base pair occurs at least once)
    assert sum(stats[k] for k in ed.CLASSES) == n
    # the filter over the same tiles: the survivors in input order
    keep = np.array([ed.keep(r, True, 2, 16) for r in zip(base["editable"], base["hit"])])
    assert 0 < keep.sum() < len(keep)
    codes = np.arange(n, dtype=np.uint64) * np.uint64(3)
    g = Guides.from_arrays(ctx, codes, loci)
    out = g.filter(s["gen"], sh, targets, 2, 16)
    got_codes, got_loci = out.arrays()
    chosen = np.nonzero(keep[idx])[0]
    assert got_codes.tobytes() == codes[chosen].tobytes() and got_loci.tobytes() == loci[chosen].tobytes()
    out.close()
    g.close()


# ---- 4. the pair contract ----------------------------------------------------------------------------------------------------
def test_the_pair_contract(ctx, small):
    shape, which = (23, 3, 5, "C"), "third"
    s, sh = small(23), shape_of(shape)
    want = small.want(shape, which)
    want_pairs, want_cov = sorted_numbering(want, s["sets"][which])
    total = len(want_pairs)
    tg = va.edit_targets(s["sets"][which])[0]
    L, st = va.lib(), sh._struct()
    n = len(s["arr"])

    def call(pairs, capacity, rows=True, cov=True):
        r = np.full((n, 2), 7, dtype=np.uint32) if rows else None
        c = np.full((len(tg), 2), 7, dtype=np.uint32) if cov else None
        count, stats = C.c_uint64(12345), _lib.EditStats()
        rc = L.vsc_loci_edit(ctx._h, s["gen"]._h, _lib.ptr(s["arr"]), n, C.byref(st), _lib.ptr(tg), len(tg), _lib.ptr(r), _lib.ptr(pairs), capacity,
                             C.byref(count), _lib.ptr(c), C.byref(stats))
        return rc, r, c, int(count.value), stats.as_dict()

    rc, rows, cov, count, stats = call(None, 0)  # count only
    assert rc == 0 and count == total and rows.tobytes() == want["rows"].tobytes() and cov.tobytes() == want_cov.tobytes()
    assert counts(stats) == want["stats"]
    exact = np.zeros(total, dtype=va.EDIT_PAIR_DTYPE)
    rc, rows, cov, count, _ = call(exact, total)
    assert rc == 0 and count == total and exact.tobytes() == want_pairs.tobytes()
    short = np.full(total, 0x5A5A5A5A, dtype=np.uint32).repeat(4).view(va.EDIT_PAIR_DTYPE)[:total].copy()
    before = short.tobytes()
    rc, rows, cov, count, stats = call(short, total - 1)  # one short
    assert rc == -34 and "capacity" in L.vsc_last_error(ctx._h).decode()
    assert short.tobytes() == before  # nothing is written to pairs
    assert count == total and rows.tobytes() == want["rows"].tobytes() and cov.tobytes() == want_cov.tobytes() and counts(stats) == want["stats"]
    rc, _, _, count, stats = call(None, 0, rows=False, cov=False)  # every output but the count is optional
    assert rc == 0 and count == total and counts(stats) == want["stats"]  # (the covered targets are then counted on the device)
    assert L.vsc_loci_edit(ctx._h, s["gen"]._h, _lib.ptr(s["arr"]), n, C.byref(st), _lib.ptr(tg), len(tg), None, None, 0, None, None, None) == 0
    # nothing to do
    rows, pairs, coverage, stats = s["gen"].edit(ed.locus_array([]), sh, s["sets"][which], coverage=True)
    assert rows.shape == (0, 2) and len(pairs) == 0 and (coverage[:, 0] == 0).all() and (coverage[:, 1] == ed.UNDEF).all()
    assert counts(stats) == dict.fromkeys(COUNTS, 0)
    t = ctx.timing()
    assert t["sites"] == 0 and t["total_ms"] == 0


# ---- 5. candidates where they lie ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted(ctx):
    """A 20 kb random genome with NGG sites (and CCN sites, their '-' form) at and next to the contig ends."""
    rng = np.random.default_rng(78)
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
    every = [(c, p) for c, t in enumerate(contigs) for p in range(len(t))]
    yield {"contigs": contigs, "packed": packed, "gen": gen, "third": [t for t in every if t[1] % 3 == 0], "every": every}
    gen.close()


def test_enumerated_guides_where_they_lie(ctx, planted):
    gen, contigs = planted["gen"], planted["contigs"]
    plain = gen.enumerate_guides()
    for shape in ((23, 3, 5, "C"), (23, 3, 4, "A"), (23, 22, 1, "C")):
        sh = shape_of(shape)
        codes, loci, rows = gen.enumerate_guides(edit=sh)
        assert codes.tobytes() == plain[0].tobytes() and loci.tobytes() == plain[1].tobytes() and len(codes) > 1000
        want = ed.expected(contigs, ed.loci_tuples(loci), shape, planted["every"])
        assert rows.dtype == np.uint32 and rows[:, 0].tobytes() == want["rows"][:, 0].tobytes() and (rows[:, 1] == 0).all()
        same(gen.edit((codes, loci), sh, planted["every"], coverage=True), want, planted["every"])
        if shape[1] == 22:  # the PAM's G sits there: no editable C, no pair
            assert want["stats"]["pairs"] == 0 and (want["rows"][:, 0] == 0).all()
        else:
            assert want["stats"]["pairs"] > 500
    # over the handle, with targets: what vsc_loci_edit gives for the same loci
    shape = (23, 3, 5, "C")
    want = ed.expected(contigs, ed.loci_tuples(plain[1]), shape, planted["third"])
    g = Guides.from_arrays(ctx, plain[0], plain[1])
    rows, pairs, cov, stats, rc = g.edit(gen, shape_of(shape), planted["third"], want["stats"]["pairs"])
    want_pairs, want_cov = sorted_numbering(want, planted["third"])
    assert rc == 0 and rows.tobytes() == want["rows"].tobytes() and pairs.tobytes() == want_pairs.tobytes() and cov.tobytes() == want_cov.tobytes()
    assert counts(stats) == want["stats"]
    host = Guides.from_arrays(ctx, plain[0], plain[1], on_device=False)  # the host-only object goes the vsc_loci_edit way
    h_rows, h_pairs, h_cov, h_stats, rc = host.edit(gen, shape_of(shape), planted["third"], want["stats"]["pairs"])
    assert rc == 0 and h_rows.tobytes() == rows.tobytes() and h_pairs.tobytes() == pairs.tobytes() and h_cov.tobytes() == cov.tobytes()
    host.close()
    g.close()
    # N x 21 + GG under the pattern enumeration: the same sites, the same rows
    found, prows = gen.enumerate_pattern("N" * 21 + "GG", (0, 20), edit=shape_of(shape))
    assert found.loci.tobytes() == plain[1].tobytes() and prows[:, 0].tobytes() == want["rows"][:, 0].tobytes()
    with pytest.raises(ValueError):
        gen.enumerate_guides(edit=va.EditShape(site_len=27))
    with pytest.raises(ValueError):
        gen.enumerate_guides(min_editable=1)
    with pytest.raises(ValueError):
        gen.enumerate_guides(edit_targets=[(0, 5)])


@pytest.mark.parametrize("pattern,proto,window,base", [("N" * 21 + "NNGRRT", (0, 21), (3, 5), "C"), ("TTTV" + "N" * 23, (4, 23), (11, 6), "A")],
                         ids=["SaCas9", "Cas12a"])
def test_pattern_candidates_of_other_nucleases(planted, pattern, proto, window, base):
    gen, contigs = planted["gen"], planted["contigs"]
    shape = (len(pattern), window[0], window[1], base)
    sh = shape_of(shape)
    plain = gen.enumerate_pattern(pattern, proto)
    found, rows = gen.enumerate_pattern(pattern, proto, edit=sh)
    assert found.codes.tobytes() == plain.codes.tobytes() and found.loci.tobytes() == plain.loci.tobytes() and len(found) > 100
    want = ed.expected(contigs, ed.loci_tuples(found.loci), shape, planted["third"])
    assert want["stats"]["defined"] > 100 and want["stats"]["pairs"] > 20
    assert rows[:, 0].tobytes() == want["rows"][:, 0].tobytes()
    same(gen.edit(found, sh, planted["third"], coverage=True), want, planted["third"])
    # the filter through the wrapper: the survivors in input order, their rows; only the survivors are searched
    keep = np.array([ed.keep(r, True, 1, 2) for r in zip(want["editable"], want["hit"])])
    assert 0 < keep.sum() < len(keep)
    kept, krows = gen.enumerate_pattern(pattern, proto, edit=sh, edit_targets=planted["third"], min_editable=1, max_editable=2)
    assert kept.codes.tobytes() == found.codes[keep].tobytes() and kept.loci.tobytes() == found.loci[keep].tobytes()
    assert krows[:, 0].tobytes() == want["rows"][keep, 0].tobytes()
    d_found, d_rows, d_edit = gen.design_pattern(pattern, proto, 2, edit=sh, edit_targets=planted["third"], min_editable=1, max_editable=2)
    assert d_found.codes.tobytes() == kept.codes.tobytes() and d_edit.tobytes() == krows.tobytes()
    _, all_rows = gen.design_pattern(pattern, proto, 2)
    assert d_rows.tobytes() == all_rows[keep].tobytes()
    _, rows_kept = gen.search_pattern(pattern, kept.text(), 2, records=False)
    _, rows_all = gen.search_pattern(pattern, found.text(), 2, records=False)
    assert rows_kept.tobytes() == rows_all[keep].tobytes()


# ---- 6. the filter ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["none", "third"])
def test_filter_bounds_and_input_order(ctx, small, which):
    shape = (23, 0, 16, "C")
    s, sh = small(23), shape_of(shape)
    want = small.want(shape, which)
    targets = s["sets"][which]
    n = len(s["loci"])
    codes = np.arange(n, dtype=np.uint64) * np.uint64(5)
    g = Guides.from_arrays(ctx, codes, s["arr"])
    kept = {}
    for lo, hi in ((0, 16), (1, 1), (2, 16), (0, 0)):
        keep = np.array([ed.keep(r, targets is not None, lo, hi) for r in zip(want["editable"], want["hit"])])
        out = g.filter(s["gen"], sh, targets, lo, hi)
        got_codes, got_loci = out.arrays()
        out.close()
        assert got_codes.tobytes() == codes[keep].tobytes() and got_loci.tobytes() == s["arr"][keep].tobytes(), (lo, hi)
        kept[lo, hi] = int(keep.sum())
    if targets is None:
        assert kept[0, 16] == want["stats"]["defined"] and 0 < kept[1, 1] < kept[0, 16] and 0 < kept[2, 16] and kept[0, 0] > 0
    else:
        assert kept[0, 16] == want["stats"]["with_hit"] and 0 < kept[1, 1] < kept[0, 16] and kept[0, 0] == 0  # no editable base, no hit
    t = ctx.timing()
    assert t["sites"] == n and t["score_ms"] == t["total_ms"] > 0
    assert t["genome_bytes"] == 32 * n + 48 * kept[0, 0]  # (the last call's)
    host = Guides.from_arrays(ctx, codes, s["arr"], on_device=False)  # the host-only object: uploaded first, the same bytes
    keep = np.array([ed.keep(r, targets is not None, 2, 16) for r in zip(want["editable"], want["hit"])])
    h_out = host.filter(s["gen"], sh, targets, 2, 16)
    assert h_out.arrays()[0].tobytes() == codes[keep].tobytes()
    full = h_out.filter(s["gen"], sh, targets, 16, 16)
    empty = full.filter(s["gen"], sh, targets, 0, 0)  # an empty result is a result
    assert len(empty) == 0 and len(empty.filter(s["gen"], sh, targets, 0, 16).arrays()[0]) == 0
    for h in (empty, full, h_out, host, g):
        h.close()


def test_what_takes_the_filters_result(planted):
    gen, contigs = planted["gen"], planted["contigs"]
    shape, targets = (23, 3, 5, "C"), planted["third"]
    sh = shape_of(shape)
    pcodes, ploci = gen.enumerate_guides()
    want = ed.expected(contigs, ed.loci_tuples(ploci), shape, targets)
    keep = np.array([ed.keep(r, True, 1, 3) for r in zip(want["editable"], want["hit"])])
    assert 0 < keep.sum() < want["stats"]["with_hit"]
    k_codes, k_loci, k_rows = gen.enumerate_guides(edit="CBE", edit_targets=targets, min_editable=1, max_editable=3)
    assert k_codes.tobytes() == pcodes[keep].tobytes() and k_loci.tobytes() == ploci[keep].tobytes()
    assert k_rows[:, 0].tobytes() == want["rows"][keep, 0].tobytes()
    rows_all = gen.summarize(pcodes, 2, exclude=ploci)
    assert gen.summarize(k_codes, 2, exclude=k_loci).tobytes() == rows_all[keep].tobytes()
    d = gen.design(None, 2, edit=sh, edit_targets=targets, min_editable=1, max_editable=3)
    assert len(d) == 4 and d[0].tobytes() == k_codes.tobytes() and d[2].tobytes() == rows_all[keep].tobytes() and d[3].tobytes() == k_rows.tobytes()
    plain = gen.design(None, 2)
    assert len(plain) == 3 and plain[2].tobytes() == rows_all.tobytes()  # without the arguments: what it returned before


def test_three_filters_in_two_orders(ctx, planted):
    gen = planted["gen"]
    model, mh, sh = ec.build("dense", (6, 23, 6)), va.MicrohomologyShape(23, 17, 30), shape_of((23, 3, 5, "C"))
    targets = planted["third"]
    codes, loci, linear, mpairs, erows = gen.enumerate_guides(efficiency=model, microhomology=mh, edit=sh)
    assert linear.dtype == np.float64 and mpairs.shape == (len(codes), 2) and erows.shape == (len(codes), 2)  # the edit rows come last
    floor = float(np.median(linear[linear == linear]))
    g = Guides.from_arrays(ctx, codes, loci)
    a1 = g.filter_efficiency(gen, model, floor)
    a2 = a1.filter_microhomology(gen, mh, 100, 600)
    a3 = a2.filter(gen, sh, targets, 1, 3)
    b1 = g.filter(gen, sh, targets, 1, 3)
    b2 = b1.filter_microhomology(gen, mh, 100, 600)
    b3 = b2.filter_efficiency(gen, model, floor)
    assert 0 < len(a3) < min(len(a2), len(b1))
    for x, y in zip(a3.arrays(), b3.arrays()):
        assert x.tobytes() == y.tobytes()
    k = gen.enumerate_guides(efficiency=model, min_efficiency=floor, microhomology=mh, min_out_of_frame=60, min_microhomology=10, edit=sh,
                             edit_targets=targets, min_editable=1, max_editable=3)
    assert k[0].tobytes() == a3.arrays()[0].tobytes() and k[1].tobytes() == a3.arrays()[1].tobytes() and len(k) == 5
    for h in (a1, a2, a3, b1, b2, b3, g):
        h.close()


# ---- 7. end to end ------------------------------------------------------------------------------------------------------------
def test_the_fewest_bystanders_per_target(planted):
    gen, contigs, packed = planted["gen"], planted["contigs"], planted["packed"]
    shape = (23, 3, 5, "C")
    rng = np.random.default_rng(5)
    every = planted["every"]
    targets = [every[i] for i in rng.choice(len(every), size=2000, replace=False)] + [every[7], every[7]]
    codes, loci = gen.enumerate_guides()
    rows, pairs, _, stats = gen.edit((codes, loci), shape_of(shape), targets)
    want = ed.expected(contigs, ed.loci_tuples(loci), shape, targets)
    assert pairs.tobytes() == want["pairs"].tobytes() and 100 < len(pairs)  # (2 400 candidates x 1.25 C per window x a tenth of the positions: about 300)
    spec = (np.arange(len(codes), dtype=np.uint64) * np.uint64(2654435761)) % np.uint64(10007)  # a stand-in for a specificity column
    p_loci, p_target, key = va.edit_pick_inputs(pairs, loci, extra_columns=[(spec, 14)])
    pick = va.PickShape(3, spacing=2)  # (the guides of one target lie within 5 bases of each other: a wider spacing leaves one)
    picks, cnt, st = gen.pick(p_loci, key, pick, target=p_target, n_targets=len(targets))
    # the restatement, followed by the host's pick
    by = (want["pairs"]["info"] >> 8).astype(np.uint64)
    want_key = ((np.uint64(15) - by) << np.uint64(14)) | np.minimum(spec[want["pairs"]["candidate"]], np.uint64(16383))
    assert key.tobytes() == want_key.tobytes()
    h_picks, h_cnt, _ = va.pick_host(packed.contigs, loci[want["pairs"]["candidate"]], want["pairs"]["target"], want_key, len(targets), pick)
    assert picks.tobytes() == h_picks.tobytes() and cnt.tobytes() == h_cnt.tobytes() and cnt.max() >= 2 and (cnt == 0).any()
    first = picks[cnt > 0, 0]
    assert (by[first] == [by[want["pairs"]["target"] == t].min() for t in np.nonzero(cnt > 0)[0]]).all()  # the fewest bystanders first


def test_a_shard_answers_for_what_it_holds(ctx, planted):
    shape = (23, 3, 5, "C")
    packed, contigs, sh = planted["packed"], planted["contigs"], shape_of(shape)
    n_words = packed.n_words
    loci = [(0, p, s) for p in list(range(2000, 2100)) + list(range(2200, 2280)) for s in (0, 1)]
    loci += ed.loci_tuples(planted["gen"].enumerate_guides()[1])
    arr = ed.locus_array(loci)
    for first, words, own in ((64, n_words - 64, n_words - 64), (0, 70, 64)):  # nothing in front of word 64; nothing behind a 6-word halo
        sl = slice(first, first + words)
        shard = va.Genome.from_shard(ctx, packed.hi[sl], packed.lo[sl], packed.nmask[sl], first, own, packed.contigs)
        want = ed.expected(contigs, loci, shape, planted["third"], resident=(32 * first, 32 * (first + words)))
        assert want["stats"]["not_resident"] > 100 and want["stats"]["defined"] > 100 and want["stats"]["pairs"] > 20
        with pytest.raises(ValueError) as e:
            shard.edit(arr, sh, planted["third"])
        assert "not resident" in str(e.value)
        same(shard.edit(arr, sh, planted["third"], coverage=True, allow_partial=True), want, planted["third"])
        shard.close()


def test_alternating_shapes_scratch_and_timing(ctx, small):
    s = small(23)
    gen, arr, n = s["gen"], s["arr"], len(s["loci"])
    combos = [((23, 3, 5, "C"), "third"), ((23, 0, 16, "C"), "every"), ((23, 3, 4, "A"), "none"), ((23, 7, 16, "A"), "one_contig")]
    for k in (0, 0, 1, 0, 2, 3, 1, 2):  # nothing of a call outlives it
        shape, which = combos[k]
        same(gen.edit(arr, shape_of(shape), s["sets"][which], coverage=True), small.want(shape, which), s["sets"][which])
    ctx.release_scratch()
    shape, which = combos[1]
    same(gen.edit(arr, shape_of(shape), s["sets"][which], coverage=True), small.want(shape, which), s["sets"][which])
    ctx.release_scratch()
    shape, which = combos[0]
    got = gen.edit(arr, shape_of(shape), s["sets"][which], coverage=True)
    same(got, small.want(shape, which), s["sets"][which])
    stats = got[3]
    assert stats["kernel_ms"] > 0 and stats["wall_ms"] >= stats["kernel_ms"]
    assert stats["target_order"].tolist() == va.edit_targets(s["sets"][which])[1].tolist()
    t = ctx.timing()
    assert t["score_ms"] > 0 and t["scan_ms"] > 0 and t["total_ms"] == t["score_ms"] + t["scan_ms"] and t["sites"] == n
    assert t["genome_bytes"] == 24 * n
    got = gen.edit(arr, shape_of(shape), None)
    t = ctx.timing()
    assert t["scan_ms"] == 0 and t["total_ms"] == t["score_ms"] > 0  # without targets: the rows kernel alone


def test_every_refusal(ctx, planted, small):
    L = va.lib()
    gen, contigs = planted["gen"], planted["contigs"]
    g = Guides.from_arrays(ctx, *gen.enumerate_guides())
    n = len(g)
    rows = np.full((n, 2), 9, dtype=np.uint32)
    ok = va.EditShape()._struct()
    tg = va.edit_targets(planted["third"])[0]
    count = C.c_uint64()

    def guides_edit(shape, targets=None, n_t=0, handle=g.h, genome=gen._h, context=None):
        return L.vsc_guides_edit((context or ctx)._h, genome, handle, shape, _lib.ptr(targets), n_t, _lib.ptr(rows), None, 0, C.byref(count), None, None)

    for bad in ((15, (3, 5), 1), (33, (3, 5), 1), (23, (3, 0), 1), (23, (3, 17), 1), (23, (19, 5), 1), (23, (24, 1), 1), (23, (3, 5), 4),
                (23, (0xFFFFFFFF, 2), 1), (23, (3, 0xFFFFFFFF), 1)):  # a shape outside SHAPE
        sh = va.EditShape(*bad, validate=False)
        st = sh._struct()
        assert guides_edit(C.byref(st)) == -22, bad
        code, out = g.filter_code(gen, sh, None, 0, 16)
        assert code == -22 and not out.value
        with pytest.raises(va.VarscotError):
            gen.edit(ed.locus_array([(0, 100, 0)]), sh)
    reserved = va.EditShape()._struct()
    reserved.reserved[2] = 1
    assert guides_edit(C.byref(reserved)) == -22 and "reserved" in L.vsc_last_error(ctx._h).decode()
    sh27 = va.EditShape(site_len=27)._struct()  # vsc_guides holds 23-mers
    assert guides_edit(C.byref(sh27)) == -22 and "site_len" in L.vsc_last_error(ctx._h).decode()
    assert g.filter_code(gen, va.EditShape(site_len=27), None, 0, 16)[0] == -22
    assert guides_edit(None) == -22 and guides_edit(C.byref(ok), genome=None) == -22 and guides_edit(C.byref(ok), handle=None) == -22  # null arguments
    assert L.vsc_guides_filter_edit(ctx._h, gen._h, g.h, C.byref(ok), None, 0, 0, 16, None) == -22
    assert guides_edit(C.byref(ok), None, 3) == -22 and "null" in L.vsc_last_error(ctx._h).decode()  # n_t > 0 with NULL targets
    code, out = g.filter_code(gen, va.EditShape(), None, 3, 2)
    assert code == -22 and not out.value and "min_editable" in L.vsc_last_error(ctx._h).decode()

    def targets_of(rows_):
        t = np.zeros(len(rows_), dtype=va.EDIT_TARGET_DTYPE)
        t["contig"], t["pos"] = [r[0] for r in rows_], [r[1] for r in rows_]
        return t

    for bad, word in (([(0, 5), (0, 5)], "ascending"), ([(0, 6), (0, 5)], "ascending"), ([(1, 0), (0, 5)], "ascending"),
                      ([(len(contigs), 0)], "unknown"), ([(0, len(contigs[0]))], "beyond"), ([(0xFFFFFFFF, 0)], "unknown")):
        t = targets_of(bad)
        assert guides_edit(C.byref(ok), t, len(t)) == -22 and word in L.vsc_last_error(ctx._h).decode(), bad
        out = C.c_void_p()
        assert L.vsc_guides_filter_edit(ctx._h, gen._h, g.h, C.byref(ok), _lib.ptr(t), len(t), 0, 16, C.byref(out)) == -22 and not out.value
    assert (rows == 9).all()  # checked before anything is written
    last = targets_of([(0, len(contigs[0]) - 1), (2, len(contigs[2]) - 1)])  # the last base of a contig is a target
    assert guides_edit(C.byref(ok), last, 2) == 0
    assert L.vsc_loci_edit(ctx._h, gen._h, None, 1, C.byref(ok), None, 0, _lib.ptr(rows), None, 0, None, None, None) == -22
    assert L.vsc_loci_edit(ctx._h, gen._h, _lib.ptr(rows), 0xFFFFFFFF, C.byref(ok), None, 0, None, None, 0, None, None, None) == -34  # n
    assert L.vsc_loci_edit(ctx._h, gen._h, _lib.ptr(rows), 1, C.byref(ok), _lib.ptr(tg), 0xFFFFFFFF, None, None, 0, None, None, None) == -34  # n_t
    other = va.Context(0)  # a genome or an object of another context is refused
    assert guides_edit(C.byref(ok), context=other) == -22
    o_gen = other.load_genome(planted["packed"])
    assert guides_edit(C.byref(ok), genome=o_gen._h, context=other) == -22 and "another context" in L.vsc_last_error(other._h).decode()
    o_gen.close()
    other.close()
    g.close()


# ---- 8. the tools end to end ---------------------------------------------------------------------------------------------------
def test_both_tools_on_the_small_genome(ctx, tmp_path):
    contigs = list(ed.small_genome())
    names = ["chr%d of the small genome" % (k + 1) for k in range(len(contigs))]
    chrom = [n.split()[0] for n in names]
    with open(tmp_path / "g.fa", "w") as f:
        for n, t in zip(names, contigs):
            f.write(">%s\n%s\n" % (n, "\n".join(t[i:i + 60] for i in range(0, len(t), 60))))
    iv = [(c, 0, len(t)) for c, t in enumerate(contigs)]
    (tmp_path / "t.bed").write_text("".join("%s\t%d\t%d\n" % (chrom[c], a, b) for c, a, b in iv))
    sets = ed.target_sets(contigs)
    for which in ("third", "every"):  # in the caller's order, with a duplicate: the tool sorts them
        rows_ = sets[which] + sets[which][:3]
        (tmp_path / ("z_%s.bed" % which)).write_text("".join("%s\t%d\t%d\n" % (chrom[c], p, p + 1) for c, p in rows_))
    run = lambda *a: subprocess.run([os.path.join(BIN, a[0])] + [str(x) for x in a[1:]], capture_output=True, text=True, timeout=600)  # noqa: E731
    assert run("bidir_index", "-G", tmp_path / "g.fa", "-I", tmp_path / "idx").returncode == 0
    packed = va.PackedGenome.from_sequences(contigs)
    gen = ctx.load_genome(packed)
    lines_of = lambda path: (tmp_path / path).read_text().splitlines()  # noqa: E731

    def columns(want, shape):
        out = []
        for locus, at, hits in zip(want["loci"], want["editable"], want["hit"]):
            text = ed.site_of(contigs, locus, shape[0])[1]
            out.append("\t%s\t%d\t%d" % (text[shape[1]:shape[1] + shape[2]], len(at), len(hits)))
        return out

    def pair_lines(want, targets, ids):
        rows_ = sorted((int(q["candidate"]), targets[q["target"]], int(q["info"]) & 255, int(q["info"]) >> 8) for q in want["pairs"])
        return ["#chrom\tpos\tguideId\tat\tbystanders"] + ["%s\t%d\t%s\t%d\t%d" % (chrom[t[0]], t[1], ids[i], at, by) for i, t, at, by in rows_]

    # guide_summary -E -L -x [-z -o] [-l]
    regions = va.Regions(packed, iv, rule="inside")
    codes, loci = gen.enumerate_guides(regions)
    regions.close()
    tuples = ed.loci_tuples(loci)
    ids = ["%s:%d:%s" % (chrom[c], p, "-" if s else "+") for c, p, s in tuples]
    cbe = (23, 3, 5, "C")
    want = dict(ed.expected(contigs, tuples, cbe, sets["third"]), loci=tuples)
    assert 100 < len(codes) < 400 and want["stats"]["pairs"] >= 20
    base = ("guide_summary", "-G", tmp_path / "g.fa", "-I", tmp_path / "idx", "-M", "2", "-E", tmp_path / "t.bed")
    r = run(*base, "-L", tmp_path / "plain.bed", "-O", tmp_path / "plain.tsv")
    assert r.returncode == 0, r.stderr
    r = run(*base, "-L", tmp_path / "x.bed", "-O", tmp_path / "x.tsv", "-x", "CBE")
    assert r.returncode == 0, r.stderr
    plain_bed, plain_rows = lines_of("plain.bed"), lines_of("plain.tsv")
    assert len(plain_bed) == len(codes)
    assert (tmp_path / "x.tsv").read_bytes() == (tmp_path / "plain.tsv").read_bytes()  # -x alone adds to the listing alone
    no_targets = dict(ed.expected(contigs, tuples, cbe), loci=tuples)
    assert lines_of("x.bed") == [ln + col for ln, col in zip(plain_bed, columns(no_targets, cbe))]
    r = run(*base, "-L", tmp_path / "x2.bed", "-O", tmp_path / "x2.tsv", "-x", "3,5,c")
    assert r.returncode == 0 and (tmp_path / "x2.bed").read_bytes() == (tmp_path / "x.bed").read_bytes()  # the preset, spelled out
    keep = np.array([ed.keep(rw, True, 0, 16) for rw in zip(want["editable"], want["hit"])])
    assert 0 < keep.sum() < len(keep)
    r = run(*base, "-L", tmp_path / "z.bed", "-O", tmp_path / "z.tsv", "-x", "CBE", "-z", tmp_path / "z_third.bed", "-o", tmp_path / "zp.tsv")
    assert r.returncode == 0, r.stderr
    want_bed = [ln + col for ln, col in zip(plain_bed, columns(want, cbe))]
    assert lines_of("z.bed") == [ln for ln, k in zip(want_bed, keep) if k]
    assert lines_of("z.tsv") == [plain_rows[0]] + [ln for ln, k in zip(plain_rows[1:], keep) if k]
    assert lines_of("zp.tsv") == pair_lines(want, sets["third"], ids)  # (every candidate of a pair survives: the ids name it)
    keep2 = np.array([ed.keep(rw, True, 2, 3) for rw in zip(want["editable"], want["hit"])])
    assert 0 < keep2.sum() < keep.sum()
    r = run(*base, "-L", tmp_path / "l.bed", "-O", tmp_path / "l.tsv", "-x", "CBE", "-z", tmp_path / "z_third.bed", "-l", "2,3")
    assert r.returncode == 0 and lines_of("l.bed") == [ln for ln, k in zip(want_bed, keep2) if k]
    wide = (23, 0, 16, "C")
    w = dict(ed.expected(contigs, tuples, wide), loci=tuples)
    keep3 = np.array([ed.keep(rw, False, 5, 16) for rw in zip(w["editable"], w["hit"])])
    assert 0 < keep3.sum() < len(keep3)
    r = run(*base, "-L", tmp_path / "w.bed", "-O", tmp_path / "w.tsv", "-x", "0,16,C", "-l", "5,16")  # bounds without targets
    assert r.returncode == 0 and lines_of("w.bed") == [ln + col for ln, col, k in zip(plain_bed, columns(w, wide), keep3) if k]
    r = run(*base, "-L", tmp_path / "k.bed", "-O", tmp_path / "k.tsv", "-x", "CBE", "-k", "1")  # with -k the edit columns stay last
    assert r.returncode == 0, r.stderr
    assert all(ln.endswith(col) and ln.startswith(first) for ln, first, col in zip(lines_of("k.bed"), plain_bed, columns(no_targets, cbe)))
    for args, text in (((*base, "-l", "1,2"), "give -x"), ((*base, "-z", tmp_path / "z_third.bed"), "give -x"),
                       ((*base, "-o", tmp_path / "p.tsv"), "give -x"), ((*base, "-x", "CBE", "-o", tmp_path / "p.tsv"), "give -z"),
                       ((*base[:7], "-B", tmp_path / "plain.bed", "-x", "CBE"), "give -E"), ((*base, "-x", "CBE", "-D", "0,0"), "one device"),
                       ((*base, "-x", "BE9"), "-x takes"), ((*base, "-x", "3,17,C"), "-x takes"), ((*base, "-x", "20,5,C"), "-x takes"),
                       ((*base, "-x", "3,5,N"), "-x takes"), ((*base, "-x", "CBE", "-l", "3,2"), "-l takes"),
                       ((*base, "-x", "CBE", "-l", "0,17"), "-l takes"), ((*base, "-x", "CBE", "-l", "two"), "-l takes")):
        r = run(*args)
        assert r.returncode != 0 and text in r.stderr, (args, r.stderr)
    (tmp_path / "bad.bed").write_text("%s\t5\t7\n" % chrom[3])  # two bases on a line
    r = run(*base, "-x", "CBE", "-z", tmp_path / "bad.bed")
    assert r.returncode != 0 and "one base per line" in (r.stderr + r.stdout)

    # pattern_search -E -x START,LEN,BASE -z -o: Cas12a, an adenine editor's window inside the protospacer
    pattern, proto = "TTTV" + "N" * 23, (4, 23)
    shape = (27, 11, 6, "A")
    (tmp_path / "p.bed").write_text("".join("%s\t%d\t%d\n" % (chrom[c], a, b) for c, a, b in iv))
    found = gen.enumerate_pattern(pattern, proto, targets=iv)
    ptuples = ed.loci_tuples(found.loci)
    pids = ["%s:%d:%s" % (chrom[c], p, "-" if s else "+") for c, p, s in ptuples]
    pw = dict(ed.expected(contigs, ptuples, shape, sets["every"]), loci=ptuples)
    pkeep = np.array([ed.keep(rw, True, 0, 16) for rw in zip(pw["editable"], pw["hit"])])
    assert len(found) >= 10 and 0 < pkeep.sum() < len(pkeep) and pw["stats"]["pairs"] >= 10
    pbase = ("pattern_search", "-i", tmp_path / "idx", "-q", pattern, "-p", "%d,%d" % proto, "-B", tmp_path / "p.bed", "-M", "2")
    r = run(*pbase, "-E", tmp_path / "pe.tsv", "-O", tmp_path / "po.tsv")
    assert r.returncode == 0, r.stderr
    pe, po = lines_of("pe.tsv"), lines_of("po.tsv")
    assert len(pe) == len(found) + 1
    r = run(*pbase, "-E", tmp_path / "pex.tsv", "-O", tmp_path / "pox.tsv", "-x", "11,6,A")
    assert r.returncode == 0, r.stderr
    pn = dict(ed.expected(contigs, ptuples, shape), loci=ptuples)
    assert lines_of("pex.tsv") == [pe[0] + "\teditWindow\teditable\ttargetsHit"] + [ln + col for ln, col in zip(pe[1:], columns(pn, shape))]
    assert (tmp_path / "pox.tsv").read_bytes() == (tmp_path / "po.tsv").read_bytes()
    r = run(*pbase, "-E", tmp_path / "pez.tsv", "-O", tmp_path / "poz.tsv", "-x", "11,6,A", "-z", tmp_path / "z_every.bed", "-o", tmp_path / "pp.tsv")
    assert r.returncode == 0, r.stderr
    want_pe = [ln + col for ln, col in zip(pe[1:], columns(pw, shape))]
    assert lines_of("pez.tsv") == [pe[0] + "\teditWindow\teditable\ttargetsHit"] + [ln for ln, k in zip(want_pe, pkeep) if k]
    assert lines_of("poz.tsv") == [po[0]] + [ln for ln, k in zip(po[1:], pkeep) if k]
    assert lines_of("pp.tsv") == pair_lines(pw, sets["every"], pids)
    for args, text in (((*pbase, "-E", tmp_path / "x.tsv", "-O", tmp_path / "xo.tsv", "-l", "1,2"), "give -x"),
                       ((*pbase[:5], "-R", tmp_path / "g.fa", "-M", "2", "-O", tmp_path / "x.tsv", "-x", "11,6,A"), "give -E"),
                       ((*pbase, "-E", tmp_path / "x.tsv", "-O", tmp_path / "xo.tsv", "-x", "CBE"), "preset"),
                       ((*pbase, "-E", tmp_path / "x.tsv", "-O", tmp_path / "xo.tsv", "-x", "22,6,A"), "-x takes")):
        r = run(*args)
        assert r.returncode != 0 and text in (r.stderr + r.stdout), (args, r.stderr)
    gen.close()
