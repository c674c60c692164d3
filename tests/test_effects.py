"""Coding consequences of base edits on the device (vsc_loci_effects, vsc_guides_effects, vsc_pattern_guides_effects and the two
filters): bit for bit what the definition gives when it is applied locus by locus in plain Python on strings
(tests/effects_cases.py: the contig is mutated, the transcripts are rebuilt and translated, the codons that differ are the
effects).  Integers, so there is no tolerance: rows, effects, coverage and counts are compared as they are."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import edit_cases as ed
import effects_cases as fx
import varscot_amd as va
import wide_cases as wc
from helpers import random_seq, revcomp
from varscot_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "varscot_amd", "bin")

TILE = 1024  # candidates per wave of the records' and the filter's passes (include/varscot_hip.h)
DROP_FRONT, DROP_BACK = 3, 1  # words the partial object of the small genome does not hold
COUNTS = fx.CLASSES + ("with_effect", "effects", "transcripts_stopped", "by_class")
# (site_len, win_start, win_len, from, to): CBE and ABE, a 1-base and a 16-base window, site_len 16, 23 and 32
SHAPES = [(23, 3, 5, "C", "T"), (23, 3, 4, "A", "G"), (23, 10, 1, "C", "T"), (23, 10, 1, "A", "G"), (23, 7, 16, "C", "T"),
          (23, 0, 16, "A", "G"), (16, 0, 16, "C", "T"), (16, 5, 1, "A", "G"), (32, 16, 16, "A", "G"), (32, 3, 5, "C", "T")]
CBE = SHAPES[0]


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
        self.fn = {k: getattr(L, "%s_%s" % (kind, k)) for k in ("count", "data", "free", "effects", "filter_effects", "filter_edit")}

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

    def effects(self, gen, shape, to, cds, capacity, code=None):
        """(rows, effects, coverage, stats, status)"""
        n = len(self)
        rows, eff = np.empty((n, 2), dtype=np.uint32), np.zeros(capacity, dtype=va.EFFECT_DTYPE)
        cov = np.empty((cds.n_tx, 2), dtype=np.uint32)
        st, count, sh = _lib.EffectsStats(), C.c_uint64(), shape._struct()
        rc = self.fn["effects"](self.ctx._h, gen._h, self.h, C.byref(sh), "ACGT".index(to), cds._h, code, _lib.ptr(rows), _lib.ptr(eff), capacity,
                                C.byref(count), _lib.ptr(cov), C.byref(st))
        return rows, eff[:min(capacity, int(count.value))], cov, st.as_dict(), rc

    def filter_code(self, gen, shape, to, cds, require, forbid, code=None):
        out = C.c_void_p()
        sh = shape._struct()
        rc = self.fn["filter_effects"](self.ctx._h, gen._h, self.h, C.byref(sh), "ACGT".index(to) if isinstance(to, str) else to,
                                       cds._h if cds is not None else None, code, va.effect_class_mask(require), va.effect_class_mask(forbid),
                                       C.byref(out))
        return rc, out

    def filter(self, gen, shape, to, cds, require, forbid, code=None):
        rc, out = self.filter_code(gen, shape, to, cds, require, forbid, code)
        _lib.check(rc, self.ctx._h)
        return Guides(self.ctx, out, self.pattern)

    def filter_edit(self, gen, shape, lo, hi):
        out = C.c_void_p()
        sh = shape._struct()
        _lib.check(self.fn["filter_edit"](self.ctx._h, gen._h, self.h, C.byref(sh), None, 0, lo, hi, C.byref(out)), self.ctx._h)
        return Guides(self.ctx, out, self.pattern)

    def close(self):
        if self.h:
            self.fn["free"](self.h)
            self.h = None


# ---- 1. every locus of the small genome ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(ctx):
    """The small genome resident - whole, and as an object that lacks its first three words and its last one - its Cds, every
    locus of it with the invalid ones behind, and per (shape, code, partial) the expected result, computed once."""
    contigs, segments = fx.small_genome()
    packed = va.PackedGenome.from_sequences(list(contigs))
    loci = fx.every_locus(contigs) + fx.invalid_loci(contigs)
    sl = slice(DROP_FRONT, packed.n_words - DROP_BACK)
    part = va.Genome.from_shard(ctx, packed.hi[sl], packed.lo[sl], packed.nmask[sl], DROP_FRONT, sl.stop - sl.start, packed.contigs)
    s = {"contigs": contigs, "segments": segments, "packed": packed, "gen": ctx.load_genome(packed), "part": part, "loci": loci,
         "arr": ed.locus_array(loci), "resident": (32 * sl.start, 32 * sl.stop), "cds": va.Cds(packed, segments, n_tx=fx.N_TX)}
    raw, done = {}, {}

    def want(shape, code=None, partial=False):
        key = (shape, partial)
        if key not in raw:
            raw[key] = fx.raw_effects(contigs, segments, loci, shape[:4], shape[4], s["resident"] if partial else None)
        if (key, code) not in done:
            done[key, code] = fx.expected(contigs, segments, loci, shape[:4], shape[4], fx.MITO if code else fx.STANDARD, raw=raw[key])
        return done[key, code]

    s["want"] = want
    s["raw"] = raw
    yield s
    s["cds"].close()
    s["gen"].close()
    s["part"].close()


def same(got, want):
    rows, effects, coverage, stats = got
    assert rows.dtype == np.uint32 and rows.tobytes() == want["rows"].tobytes()
    assert effects.dtype == va.EFFECT_DTYPE and effects.tobytes() == want["effects"].tobytes()
    assert coverage.tobytes() == want["coverage"].tobytes()
    assert counts(stats) == want["stats"] and sum(stats[k] for k in fx.CLASSES) == len(rows) and stats["off_contig"] == 0


@pytest.mark.parametrize("code", [None, "mito"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda t: "%d-%d-%d-%s%s" % t)
def test_every_locus_of_a_small_genome(ctx, small, shape, code):
    sh, text = shape_of(shape), fx.code_string(fx.MITO) if code else None
    part_want, whole_want = small["want"](shape, code, partial=True), small["want"](shape, code)
    if shape[0] == 23:
        same(small["part"].effects(small["arr"], sh, shape[4], small["cds"], coverage=True, code=text, allow_partial=True), part_want)
        same(small["gen"].effects(small["arr"], sh, shape[4], small["cds"], coverage=True, code=text), whole_want)
        return
    # site_len 16 and 32: through the pattern handle, where the caller vouches for the length
    g = Guides.from_arrays(ctx, np.arange(len(small["arr"]), dtype=np.uint64), small["arr"], pattern=True)
    for gen, want in ((small["part"], part_want), (small["gen"], whole_want)):
        rows, effects, cov, stats, rc = g.effects(gen, sh, shape[4], small["cds"], want["stats"]["effects"] + 5, text.encode() if text else None)
        assert rc == 0
        same((rows, effects, cov, stats), want)
    g.close()


# ---- 2. the fixture holds what it is for: asserted on the restatement ---------------------------------------------------------
def test_the_fixture_is_not_vacuous(small):
    contigs, segments = small["contigs"], small["segments"]
    classes, frames = set(), set()
    for shape in SHAPES:
        want = small["want"](shape)
        classes |= {k for k, v in want["stats"]["by_class"].items() if v}
        frames |= fx.split_frames(contigs, segments, small["raw"][shape, False])
    assert classes == set(fx.EFFECTS)  # every one of the six classes occurs
    assert frames == {(strand, f) for strand in (0, 1) for f in (0, 1, 2)}  # a split codon emitted in every frame, both strands
    whole, part = small["want"](CBE), small["want"](CBE, partial=True)
    assert all(part["stats"][k] >= 5 for k in ("defined", "invalid", "not_resident", "has_n"))
    assert part["stats"]["by_class"]["unknown"] > 0 and whole["stats"]["by_class"]["unknown"] > 0
    # class unknown out of codon bases the object does not hold: a candidate whose codon is known on the whole genome
    abe_whole, abe_part = small["want"](SHAPES[1]), small["want"](SHAPES[1], partial=True)
    lost = [i for i, (a, b) in enumerate(zip(abe_whole["classes"], abe_part["classes"])) if a is not None and b is not None and 5 in b and 5 not in a]
    assert lost and small["contigs"][0][101] == "A" and small["resident"][0] == 96
    assert whole["stats"]["by_class"]["stop_gained"] >= 10 and whole["stats"]["transcripts_stopped"] >= 5
    assert (whole["coverage"][fx.N_TX - 1] == (0, fx.UNDEF)).all()  # the transcript without a segment
    wide = small["want"](SHAPES[4])
    assert np.bincount(wide["effects"]["candidate"]).max() >= 4  # several effects of one candidate: the order inside it
    assert ((wide["effects"]["info"] >> 16) & 15).max() >= 2  # two edited bases in one codon


# ---- 3. beyond one launch ----------------------------------------------------------------------------------------------------
def launch_waves():
    """The waves of a launch capped as the cells' grids are (wide_cases): CUs x 8 workgroups of 4 waves."""
    return torch.cuda.get_device_properties(0).multi_processor_count * wc.GROUPS_PER_CU * wc.WAVES_PER_GROUP


def test_more_candidates_than_a_launch_has_lanes_and_more_tiles_than_waves(ctx, small):
    shape = SHAPES[4]  # a 16-base window: several effects per candidate, runs of them cross tile boundaries
    sh, base, cds = shape_of(shape), small["want"](SHAPES[4]), small["cds"]
    m = len(small["loci"])
    n = (launch_waves() + 3) * TILE + 17
    assert n > 3 * m and n > launch_waves() * 64
    idx = np.arange(n) % m
    loci = small["arr"][idx]
    rows, effects, coverage, stats = small["gen"].effects(loci, sh, shape[4], cds, coverage=True)
    assert rows.tobytes() == base["rows"][idx].tobytes()
    reps, rem = divmod(n, m)
    be = base["effects"]
    parts = []
    for k in range(reps + 1):
        part = (be if k < reps else be[be["candidate"] < rem]).copy()
        part["candidate"] += np.uint32(k * m)
        parts.append(part)
    want = np.concatenate(parts)
    assert len(want) > 3 * TILE and stats["effects"] == len(want) == len(effects) and effects.tobytes() == want.tobytes()
    tail = be[be["candidate"] < rem]
    stops = lambda e: np.bincount(e["transcript"][((e["info"] >> 12) & 7) == 2], minlength=fx.N_TX)  # noqa: E731
    assert (coverage[:, 0] == reps * base["coverage"][:, 0] + stops(tail)).all() and (coverage[:, 1] == base["coverage"][:, 1]).all()
    assert sum(stats[k] for k in fx.CLASSES) == n
    per = {name: int((((want["info"] >> 12) & 7) == k).sum()) for k, name in enumerate(fx.EFFECTS)}
    assert stats["by_class"] == per and stats["with_effect"] == len(np.unique(want["candidate"]))
    # the filter over the same tiles: the survivors in input order
    keep = np.array([fx.keep(c, ("stop_gained", "missense"), ("unknown",)) for c in base["classes"]])
    assert 0 < keep.sum() < len(keep)
    codes = np.arange(n, dtype=np.uint64) * np.uint64(3)
    g = Guides.from_arrays(ctx, codes, loci)
    out = g.filter(small["gen"], sh, shape[4], cds, ("stop_gained", "missense"), ("unknown",))
    got_codes, got_loci = out.arrays()
    chosen = np.nonzero(keep[idx])[0]
    assert got_codes.tobytes() == codes[chosen].tobytes() and got_loci.tobytes() == loci[chosen].tobytes()
    out.close()
    g.close()


# ---- 4. the record contract --------------------------------------------------------------------------------------------------
def test_the_record_contract(ctx, small):
    sh, want, cds = shape_of(CBE), small["want"](CBE), small["cds"]
    total = len(want["effects"])
    L, st = va.lib(), sh._struct()
    n = len(small["arr"])

    def call(effects, capacity, rows=True, cov=True):
        r = np.full((n, 2), 7, dtype=np.uint32) if rows else None
        c = np.full((fx.N_TX, 2), 7, dtype=np.uint32) if cov else None
        count, stats = C.c_uint64(12345), _lib.EffectsStats()
        rc = L.vsc_loci_effects(ctx._h, small["gen"]._h, _lib.ptr(small["arr"]), n, C.byref(st), 3, cds._h, None, _lib.ptr(r), _lib.ptr(effects),
                                capacity, C.byref(count), _lib.ptr(c), C.byref(stats))
        return rc, r, c, int(count.value), stats.as_dict()

    rc, rows, cov, count, stats = call(None, 0)  # count only
    assert rc == 0 and count == total > 20 and rows.tobytes() == want["rows"].tobytes() and cov.tobytes() == want["coverage"].tobytes()
    assert counts(stats) == want["stats"]
    exact = np.zeros(total, dtype=va.EFFECT_DTYPE)
    rc, rows, cov, count, _ = call(exact, total)
    assert rc == 0 and count == total and exact.tobytes() == want["effects"].tobytes()
    short = np.full(4 * total, 0x5A5A5A5A, dtype=np.uint32).view(va.EFFECT_DTYPE).copy()
    before = short.tobytes()
    rc, rows, cov, count, stats = call(short, total - 1)  # one short
    assert rc == -34 and "capacity" in L.vsc_last_error(ctx._h).decode()
    assert short.tobytes() == before  # nothing is written to the records
    assert count == total and rows.tobytes() == want["rows"].tobytes() and cov.tobytes() == want["coverage"].tobytes()
    assert counts(stats) == want["stats"]
    rc, _, _, count, stats = call(None, 0, rows=False, cov=False)  # every output but the count is optional
    assert rc == 0 and count == total and counts(stats) == want["stats"]  # (the stopped transcripts are then counted on the device)
    assert L.vsc_loci_effects(ctx._h, small["gen"]._h, _lib.ptr(small["arr"]), n, C.byref(st), 3, cds._h, None, None, None, 0, None, None, None) == 0
    # nothing to do
    rows, effects, coverage, stats = small["gen"].effects(ed.locus_array([]), sh, "T", cds, coverage=True)
    assert rows.shape == (0, 2) and len(effects) == 0 and (coverage[:, 0] == 0).all() and (coverage[:, 1] == fx.UNDEF).all()
    assert counts(stats) == dict(dict.fromkeys(COUNTS[:-1], 0), by_class=dict.fromkeys(fx.EFFECTS, 0))
    t = ctx.timing()
    assert t["sites"] == 0 and t["total_ms"] == 0


# ---- 5. candidates where they lie ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted(ctx):
    """A 20 kb random genome with NGG sites (and CCN sites, their '-' form) at and next to the contig ends, and exon-like
    segments over it, three to a transcript."""
    rng = np.random.default_rng(429)
    contigs = []
    for n in (12000, 5000, 3000):
        t = list(random_seq(rng, n))
        for p in (0, 2, 5, n - 23, n - 25, n - 29):
            site = random_seq(rng, 21) + "GG"
            t[p:p + 23] = site if p % 2 else revcomp(site)
        contigs.append("".join(t))
    segments, n_tx = fx.random_cds(rng, contigs)
    packed = va.PackedGenome.from_sequences(contigs)
    gen = ctx.load_genome(packed)
    cds = va.Cds(packed, segments, n_tx=n_tx)
    yield {"contigs": contigs, "segments": segments, "n_tx": n_tx, "packed": packed, "gen": gen, "cds": cds}
    cds.close()
    gen.close()


def planted_want(planted, loci, shape, code=fx.STANDARD):
    return fx.expected(planted["contigs"], planted["segments"], ed.loci_tuples(loci), shape[:4], shape[4], code, n_tx=planted["n_tx"])


def test_enumerated_guides_where_they_lie(ctx, planted):
    gen, cds = planted["gen"], planted["cds"]
    plain = gen.enumerate_guides()
    for shape in (CBE, SHAPES[1], SHAPES[4]):
        sh = shape_of(shape)
        codes, loci, erows, rows = gen.enumerate_guides(edit=sh, cds=cds, edit_to=shape[4])
        assert codes.tobytes() == plain[0].tobytes() and loci.tobytes() == plain[1].tobytes() and len(codes) > 1000
        want = planted_want(planted, loci, shape)
        assert rows.dtype == np.uint32 and rows.tobytes() == want["rows"].tobytes() and want["stats"]["effects"] > 100
        same(gen.effects((codes, loci), sh, shape[4], cds, coverage=True), want)
    # over the handle: what vsc_loci_effects gives for the same loci; the host-only object goes the vsc_loci_effects way
    want = planted_want(planted, plain[1], CBE)
    for on_device in (True, False):
        g = Guides.from_arrays(ctx, plain[0], plain[1], on_device=on_device)
        rows, effects, cov, stats, rc = g.effects(gen, shape_of(CBE), "T", cds, want["stats"]["effects"])
        assert rc == 0
        same((rows, effects, cov, stats), want)
        g.close()
    # a preset by name brings its `to`; N x 21 + GG under the pattern enumeration: the same sites, the same rows
    named = gen.enumerate_guides(edit="CBE", cds=cds)
    assert named[3].tobytes() == want["rows"].tobytes()
    found, _, prows = gen.enumerate_pattern("N" * 21 + "GG", (0, 20), edit=shape_of(CBE), cds=cds)
    assert found.loci.tobytes() == plain[1].tobytes() and prows.tobytes() == want["rows"].tobytes()
    with pytest.raises(ValueError):
        gen.enumerate_guides(cds=cds)  # needs edit=
    with pytest.raises(ValueError):
        gen.enumerate_guides(edit="CBE", require_effect="stop_gained")  # needs cds=
    with pytest.raises(ValueError):
        gen.enumerate_guides(edit="CBE", cds=cds, require_effect="nonsense")


@pytest.mark.parametrize("pattern,proto,window,base,to", [("N" * 21 + "NNGRRT", (0, 21), (3, 5), "C", "T"), ("TTTV" + "N" * 23, (4, 23), (11, 6), "A", "G")],
                         ids=["SaCas9", "Cas12a"])
def test_pattern_candidates_of_other_nucleases(planted, pattern, proto, window, base, to):
    gen, cds = planted["gen"], planted["cds"]
    shape = (len(pattern), window[0], window[1], base, to)
    sh = shape_of(shape)
    plain = gen.enumerate_pattern(pattern, proto)
    found, _, rows = gen.enumerate_pattern(pattern, proto, edit=sh, cds=cds, edit_to=to)
    assert found.codes.tobytes() == plain.codes.tobytes() and found.loci.tobytes() == plain.loci.tobytes() and len(found) > 100
    want = planted_want(planted, found.loci, shape)
    assert want["stats"]["defined"] > 100 and want["stats"]["effects"] > 20
    assert rows.tobytes() == want["rows"].tobytes()
    same(gen.effects(found, sh, to, cds, coverage=True), want)
    # the filter through the wrapper: the survivors in input order, their rows; only the survivors are searched
    keep = np.array([fx.keep(c, ("missense", "stop_gained"), ("start_lost", "unknown")) for c in want["classes"]])
    assert 0 < keep.sum() < len(keep)
    kept, _, krows = gen.enumerate_pattern(pattern, proto, edit=sh, cds=cds, edit_to=to, require_effect="missense+stop_gained",
                                           forbid_effect=("start_lost", "unknown"))
    assert kept.codes.tobytes() == found.codes[keep].tobytes() and kept.loci.tobytes() == found.loci[keep].tobytes()
    assert krows.tobytes() == want["rows"][keep].tobytes()
    d = gen.design_pattern(pattern, proto, 2, edit=sh, cds=cds, edit_to=to, require_effect="missense+stop_gained",
                           forbid_effect=("start_lost", "unknown"))
    assert len(d) == 4 and d[0].codes.tobytes() == kept.codes.tobytes() and d[3].tobytes() == krows.tobytes()
    _, all_rows = gen.design_pattern(pattern, proto, 2)
    assert d[1].tobytes() == all_rows[keep].tobytes()


# ---- 6. the filter ------------------------------------------------------------------------------------------------------------
def test_filter_require_forbid_and_input_order(ctx, small):
    shape = SHAPES[4]
    sh, want, cds, gen = shape_of(shape), small["want"](shape), small["cds"], small["gen"]
    n = len(small["loci"])
    codes = np.arange(n, dtype=np.uint64) * np.uint64(5)
    g = Guides.from_arrays(ctx, codes, small["arr"])
    kept = {}
    cases = [((), ()), (("stop_gained",), ()), ((), ("missense",)), (("stop_gained", "stop_lost"), ("unknown", "start_lost")),
             (("synonymous",), ("missense", "stop_gained", "stop_lost", "start_lost", "unknown")), (fx.EFFECTS, ()), ((), fx.EFFECTS)]
    for require, forbid in cases:
        keep = np.array([fx.keep(c, require, forbid) for c in want["classes"]])
        out = g.filter(gen, sh, shape[4], cds, require, forbid)
        got_codes, got_loci = out.arrays()
        out.close()
        assert got_codes.tobytes() == codes[keep].tobytes() and got_loci.tobytes() == small["arr"][keep].tobytes(), (require, forbid)
        kept[require, forbid] = int(keep.sum())
    assert kept[(), ()] == want["stats"]["defined"] and kept[fx.EFFECTS, ()] == want["stats"]["with_effect"]
    assert kept[(), fx.EFFECTS] == want["stats"]["defined"] - want["stats"]["with_effect"]
    assert all(0 < kept[c] < want["stats"]["with_effect"] for c in cases[1:5] if c[0]) and 0 < kept[cases[2]] < kept[(), ()]
    t = ctx.timing()
    assert t["sites"] == n and t["score_ms"] == t["total_ms"] > 0
    assert t["genome_bytes"] == 32 * n + 48 * kept[(), fx.EFFECTS]  # (the last call's)
    # a custom code moves the stops: another set of survivors
    mito = small["want"](shape, "mito")
    keep_m = np.array([fx.keep(c, ("stop_gained",), ()) for c in mito["classes"]])
    keep_s = np.array([fx.keep(c, ("stop_gained",), ()) for c in want["classes"]])
    assert (keep_m != keep_s).any()
    out = g.filter(gen, sh, shape[4], cds, ("stop_gained",), (), fx.code_string(fx.MITO).encode())
    assert out.arrays()[0].tobytes() == codes[keep_m].tobytes()
    out.close()
    # before and after the edit filter: the same survivors
    ew = ed.expected(small["contigs"], small["loci"], shape[:4])
    keep_e = np.array([ed.keep(r, False, 2, 5) for r in zip(ew["editable"], ew["hit"])])
    a1 = g.filter_edit(gen, sh, 2, 5)
    a2 = a1.filter(gen, sh, shape[4], cds, ("stop_gained",), ("unknown",))
    b1 = g.filter(gen, sh, shape[4], cds, ("stop_gained",), ("unknown",))
    b2 = b1.filter_edit(gen, sh, 2, 5)
    both = keep_e & np.array([fx.keep(c, ("stop_gained",), ("unknown",)) for c in want["classes"]])
    assert 0 < both.sum() < min(len(a1), len(b1))
    for x, y in zip(a2.arrays(), b2.arrays()):
        assert x.tobytes() == y.tobytes()
    assert a2.arrays()[0].tobytes() == codes[both].tobytes()
    host = Guides.from_arrays(ctx, codes, small["arr"], on_device=False)  # the host-only object: uploaded first, the same bytes
    h_out = host.filter(gen, sh, shape[4], cds, ("stop_gained",), ("unknown",))
    assert h_out.arrays()[0].tobytes() == b1.arrays()[0].tobytes()
    empty = h_out.filter(gen, sh, shape[4], cds, (), fx.EFFECTS)  # an empty result is a result
    assert len(empty) == 0 and len(empty.filter(gen, sh, shape[4], cds, (), ()).arrays()[0]) == 0
    for h in (empty, h_out, host, a1, a2, b1, b2, g):
        h.close()


def test_the_wrappers_filter_runs_after_the_edit_filter(planted):
    gen, cds = planted["gen"], planted["cds"]
    sh = shape_of(CBE)
    pcodes, ploci = gen.enumerate_guides()
    want = planted_want(planted, ploci, CBE)
    ew = ed.expected(planted["contigs"], ed.loci_tuples(ploci), CBE[:4])
    keep = np.array([ed.keep(r, False, 1, 2) for r in zip(ew["editable"], ew["hit"])]) & \
        np.array([fx.keep(c, ("stop_gained",), ()) for c in want["classes"]])
    assert 0 < keep.sum() < want["stats"]["with_effect"]
    k_codes, k_loci, k_erows, k_rows = gen.enumerate_guides(edit="CBE", min_editable=1, max_editable=2, cds=cds, require_effect="stop_gained")
    assert k_codes.tobytes() == pcodes[keep].tobytes() and k_loci.tobytes() == ploci[keep].tobytes()
    assert k_rows.tobytes() == want["rows"][keep].tobytes() and k_erows[:, 0].tobytes() == ew["rows"][keep, 0].tobytes()
    rows_all = gen.summarize(pcodes, 2, exclude=ploci)
    d = gen.design(None, 2, edit=sh, min_editable=1, max_editable=2, cds=cds, require_effect=["stop_gained"])
    assert len(d) == 5 and d[0].tobytes() == k_codes.tobytes() and d[2].tobytes() == rows_all[keep].tobytes() and d[4].tobytes() == k_rows.tobytes()
    plain = gen.design(None, 2)
    assert len(plain) == 3 and plain[2].tobytes() == rows_all.tobytes()  # without the arguments: what it returned before


# ---- 7. end to end ------------------------------------------------------------------------------------------------------------
def test_the_earliest_stops_per_transcript(planted):
    gen, cds, packed, n_tx = planted["gen"], planted["cds"], planted["packed"], planted["n_tx"]
    shape = SHAPES[4]
    codes, loci = gen.enumerate_guides()
    rows, effects, coverage, stats = gen.effects((codes, loci), shape_of(shape), shape[4], cds, coverage=True)
    want = planted_want(planted, loci, shape)
    assert effects.tobytes() == want["effects"].tobytes() and want["stats"]["by_class"]["stop_gained"] > 30
    spec = (np.arange(len(codes), dtype=np.uint64) * np.uint64(2654435761)) % np.uint64(10007)  # a stand-in for a specificity column
    p_loci, p_target, key = va.effects_pick_inputs(effects, loci, extra_columns=[(spec, 14)])
    pick = va.PickShape(3, spacing=2)
    picks, cnt, st = gen.pick(p_loci, key, pick, target=p_target, n_targets=n_tx)
    # the restatement, followed by the host's pick
    stops = want["effects"][((want["effects"]["info"] >> 12) & 7) == 2]
    want_key = ((np.uint64(2 ** 31 - 1) - stops["codon"].astype(np.uint64)) << np.uint64(14)) | np.minimum(spec[stops["candidate"]], np.uint64(16383))
    assert key.tobytes() == want_key.tobytes() and p_target.tobytes() == stops["transcript"].tobytes()
    h_picks, h_cnt, _ = va.pick_host(packed.contigs, loci[stops["candidate"]], stops["transcript"], want_key, n_tx, pick)
    assert picks.tobytes() == h_picks.tobytes() and cnt.tobytes() == h_cnt.tobytes() and cnt.max() >= 2 and (cnt == 0).any()
    first = picks[cnt > 0, 0]
    assert (stops["codon"][first] == coverage[cnt > 0, 1]).all()  # the earliest stop of every transcript first: the coverage's codon
    assert ((cnt > 0) == (coverage[:, 0] > 0)).all()


def test_alternating_cds_objects_scratch_and_timing(ctx, small):
    gen, arr, n, contigs, packed = small["gen"], small["arr"], len(small["loci"]), small["contigs"], small["packed"]
    other_segments = tuple(s for s in small["segments"] if s[0] in (1, 3))  # another set: the device copy is replaced
    other = va.Cds(packed, other_segments, n_tx=fx.N_TX)
    none = va.Cds(packed, [], n_tx=0)  # a set without segments: rows of zeros
    sh = shape_of(CBE)
    want_other = fx.expected(contigs, other_segments, small["loci"], CBE[:4], CBE[4])
    assert 0 < want_other["stats"]["effects"] < small["want"](CBE)["stats"]["effects"]
    for k in (0, 0, 1, 0, 1, 1, 2, 0):  # nothing of a call outlives it
        if k == 2:
            rows, effects, cov, stats = gen.effects(arr, sh, "T", none, coverage=True)
            assert stats["effects"] == 0 and len(effects) == 0 and cov.shape == (0, 2)
            assert (rows[rows[:, 0] != fx.UNDEF] == 0).all() and stats["defined"] == small["want"](CBE)["stats"]["defined"]
            continue
        same(gen.effects(arr, sh, "T", other if k else small["cds"], coverage=True), want_other if k else small["want"](CBE))
    ctx.release_scratch()
    same(gen.effects(arr, sh, "T", other, coverage=True), want_other)
    other.close()  # a freed object's serial number is not handed out again: the next object is uploaded
    again = va.Cds(packed, small["segments"], n_tx=fx.N_TX)
    got = gen.effects(arr, sh, "T", again, coverage=True)
    same(got, small["want"](CBE))
    stats = got[3]
    assert stats["kernel_ms"] > 0 and stats["wall_ms"] >= stats["kernel_ms"]
    t = ctx.timing()
    assert t["score_ms"] > 0 and t["scan_ms"] > 0 and t["total_ms"] == t["score_ms"] + t["scan_ms"] and t["sites"] == n
    assert t["genome_bytes"] == 24 * n
    again.close()
    none.close()


def test_every_refusal(ctx, planted, small):
    L = va.lib()
    gen, cds = planted["gen"], planted["cds"]
    g = Guides.from_arrays(ctx, *gen.enumerate_guides())
    n = len(g)
    rows = np.full((n, 2), 9, dtype=np.uint32)
    ok = va.EditShape()._struct()
    count = C.c_uint64()

    def guides_effects(shape, to=3, handle=g.h, genome=gen._h, context=None, annotation=cds._h, code=None):
        return L.vsc_guides_effects((context or ctx)._h, genome, handle, shape, to, annotation, code, _lib.ptr(rows), None, 0, C.byref(count), None, None)

    assert guides_effects(C.byref(ok)) == 0 and (rows != 9).any()
    rows[:] = 9
    for bad in ((15, (3, 5), 1), (33, (3, 5), 1), (23, (3, 0), 1), (23, (3, 17), 1), (23, (19, 5), 1), (23, (24, 1), 1), (23, (3, 5), 4),
                (23, (0xFFFFFFFF, 2), 1), (23, (3, 0xFFFFFFFF), 1)):  # a shape outside SHAPE
        sh = va.EditShape(*bad, validate=False)
        st = sh._struct()
        assert guides_effects(C.byref(st)) == -22, bad
        code, out = g.filter_code(gen, sh, 3, cds, (), ())
        assert code == -22 and not out.value
    assert guides_effects(C.byref(ok), to=1) == -22 and "to" in L.vsc_last_error(ctx._h).decode()  # to == from
    assert guides_effects(C.byref(ok), to=4) == -22 and guides_effects(C.byref(ok), to=0xFFFFFFFF) == -22
    reserved = va.EditShape()._struct()
    reserved.reserved[2] = 1
    assert guides_effects(C.byref(reserved)) == -22 and "reserved" in L.vsc_last_error(ctx._h).decode()
    sh27 = va.EditShape(site_len=27)._struct()  # vsc_guides holds 23-mers
    assert guides_effects(C.byref(sh27)) == -22 and "site_len" in L.vsc_last_error(ctx._h).decode()
    assert g.filter_code(gen, va.EditShape(site_len=27), 3, cds, (), ())[0] == -22
    assert guides_effects(None) == -22 and guides_effects(C.byref(ok), genome=None) == -22 and guides_effects(C.byref(ok), handle=None) == -22
    assert guides_effects(C.byref(ok), annotation=None) == -22 and "null" in L.vsc_last_error(ctx._h).decode()
    assert L.vsc_guides_filter_effects(ctx._h, gen._h, g.h, C.byref(ok), 3, cds._h, None, 0, 0, None) == -22
    assert guides_effects(C.byref(ok), code=b"KNKN") == -22 and "64" in L.vsc_last_error(ctx._h).decode()
    for require, forbid in ((64, 0), (0, 64), (0xFFFFFFFF, 0)):
        code, out = g.filter_code(gen, va.EditShape(), 3, cds, require, forbid)
        assert code == -22 and not out.value and "0 .. 5" in L.vsc_last_error(ctx._h).decode()
    assert guides_effects(C.byref(ok), annotation=small["cds"]._h) == -22 and "contig table" in L.vsc_last_error(ctx._h).decode()
    assert (rows == 9).all()  # checked before anything is written
    assert L.vsc_loci_effects(ctx._h, gen._h, None, 1, C.byref(ok), 3, cds._h, None, _lib.ptr(rows), None, 0, None, None, None) == -22
    assert L.vsc_loci_effects(ctx._h, gen._h, _lib.ptr(rows), 0xFFFFFFFF, C.byref(ok), 3, cds._h, None, None, None, 0, None, None, None) == -34
    with pytest.raises(va.VarscotError):
        gen.effects(ed.locus_array([(0, 100, 0)]), va.EditShape(), "C", cds)
    with pytest.raises(ValueError):
        gen.effects(ed.locus_array([(0, 100, 0)]), va.EditShape(), "T", cds, code="KNKN")
    other = va.Context(0)  # a genome or an object of another context is refused
    assert guides_effects(C.byref(ok), context=other) == -22
    o_gen = other.load_genome(planted["packed"])
    assert guides_effects(C.byref(ok), genome=o_gen._h, context=other) == -22 and "another context" in L.vsc_last_error(other._h).decode()
    o_gen.close()
    other.close()
    g.close()


# ---- 8. the tools end to end ---------------------------------------------------------------------------------------------------
def test_both_tools_on_the_small_genome(ctx, tmp_path):
    contigs, segments = fx.small_genome()
    contigs = list(contigs)
    names = ["chr%d of the small genome" % (k + 1) for k in range(len(contigs))]
    chrom = [n.split()[0] for n in names]
    with open(tmp_path / "g.fa", "w") as f:
        for n, t in zip(names, contigs):
            f.write(">%s\n%s\n" % (n, "\n".join(t[i:i + 60] for i in range(0, len(t), 60))))
    iv = [(c, 0, len(t)) for c, t in enumerate(contigs)]
    (tmp_path / "t.bed").write_text("".join("%s\t%d\t%d\n" % (chrom[c], a, b) for c, a, b in iv))
    # the segments from the last to the first: the tool sorts them
    (tmp_path / "cds.bed").write_text("".join("%s\t%d\t%d\ttx%d\t%d\t%s\n" % (chrom[c], a, b, tx, ph, "-" if st else "+")
                                              for c, a, b, tx, st, ph in segments[::-1]))
    run = lambda *a: subprocess.run([os.path.join(BIN, a[0])] + [str(x) for x in a[1:]], capture_output=True, text=True, timeout=600)  # noqa: E731
    assert run("bidir_index", "-G", tmp_path / "g.fa", "-I", tmp_path / "idx").returncode == 0
    packed = va.PackedGenome.from_sequences(contigs)
    gen = ctx.load_genome(packed)
    lines_of = lambda path: (tmp_path / path).read_text().splitlines()  # noqa: E731
    table = fx.aa_table(fx.STANDARD)

    def edit_columns(tuples, shape):
        ew = ed.expected(contigs, tuples, shape[:4])
        return ["\t%s\t%d\t0" % (ed.site_of(contigs, locus, shape[0])[1][shape[1]:shape[1] + shape[2]], len(at))
                for locus, at in zip(tuples, ew["editable"])]

    def effect_columns(want):
        counts_, coding = va.unpack_effect_row(want["rows"])
        return ["\t%d\t%d\t%d\t%d" % (bin(int(m)).count("1"), c[2], c[1], c[0]) for c, m in zip(counts_, coding)]

    def effect_lines(want, ids):
        out = ["#guideId\ttranscript\tcodon\tref\talt\trefAA\taltAA\tclass\tat"]
        for e in want["effects"]:
            ref, alt, cls, _, at = (int(x) for x in va.unpack_effect_info(e["info"]))
            r, a = va.codon_text(ref), va.codon_text(alt)
            letters = "NA\tNA\tNA\tNA" if cls == 5 else "%s\t%s\t%s\t%s" % (r, a, table[r], table[a])
            out.append("%s\ttx%d\t%d\t%s\t%s\t%d" % (ids[e["candidate"]], e["transcript"], e["codon"], letters, fx.EFFECTS[cls], at))
        return out

    # guide_summary -E -L -x --cds [--effects] [--effect-filter] [--edit-to]
    regions = va.Regions(packed, iv, rule="inside")
    codes, loci = gen.enumerate_guides(regions)
    regions.close()
    tuples = ed.loci_tuples(loci)
    ids = ["%s:%d:%s" % (chrom[c], p, "-" if s else "+") for c, p, s in tuples]
    want = fx.expected(contigs, segments, tuples, CBE[:4], "T")
    assert 100 < len(codes) < 400 and want["stats"]["effects"] >= 20 and want["stats"]["by_class"]["stop_gained"] >= 5
    base = ("guide_summary", "-G", tmp_path / "g.fa", "-I", tmp_path / "idx", "-M", "2", "-E", tmp_path / "t.bed")
    r = run(*base, "-L", tmp_path / "plain.bed", "-O", tmp_path / "plain.tsv")
    assert r.returncode == 0, r.stderr
    plain_bed, plain_rows = lines_of("plain.bed"), lines_of("plain.tsv")
    assert len(plain_bed) == len(codes)
    r = run(*base, "-L", tmp_path / "x.bed", "-O", tmp_path / "x.tsv", "-x", "CBE", "--cds", tmp_path / "cds.bed", "--effects", tmp_path / "e.tsv")
    assert r.returncode == 0, r.stderr
    want_bed = [ln + a + b for ln, a, b in zip(plain_bed, edit_columns(tuples, CBE), effect_columns(want))]
    assert lines_of("x.bed") == want_bed
    assert (tmp_path / "x.tsv").read_bytes() == (tmp_path / "plain.tsv").read_bytes()  # without a filter the options add to the listing alone
    assert lines_of("e.tsv") == effect_lines(want, ids)
    keep = np.array([fx.keep(c, ("stop_gained",), ("unknown", "start_lost")) for c in want["classes"]])
    assert 0 < keep.sum() < want["stats"]["with_effect"]
    r = run(*base, "-L", tmp_path / "z.bed", "-O", tmp_path / "z.tsv", "-x", "CBE", "-d", tmp_path / "cds.bed", "-f", "stop_gained/unknown+start_lost",
            "-Q", tmp_path / "ze.tsv")
    assert r.returncode == 0, r.stderr
    assert lines_of("z.bed") == [ln for ln, k in zip(want_bed, keep) if k]
    assert lines_of("z.tsv") == [plain_rows[0]] + [ln for ln, k in zip(plain_rows[1:], keep) if k]
    kept_tuples = [t for t, k in zip(tuples, keep) if k]
    kept_want = fx.expected(contigs, segments, kept_tuples, CBE[:4], "T")
    assert lines_of("ze.tsv") == effect_lines(kept_want, [i for i, k in zip(ids, keep) if k])
    forbid_only = np.array([fx.keep(c, (), ("missense",)) for c in want["classes"]])
    r = run(*base, "-L", tmp_path / "f.bed", "-O", tmp_path / "f.tsv", "-x", "CBE", "--cds", tmp_path / "cds.bed", "--effect-filter", "/missense")
    assert r.returncode == 0 and lines_of("f.bed") == [ln for ln, k in zip(want_bed, forbid_only) if k] and 0 < forbid_only.sum() < len(keep)
    to_g = fx.expected(contigs, segments, tuples, CBE[:4], "G")  # another editor of the same window: C -> G
    assert to_g["rows"].tobytes() != want["rows"].tobytes()
    r = run(*base, "-L", tmp_path / "g.bed", "-O", tmp_path / "g.tsv", "-x", "3,5,C", "--cds", tmp_path / "cds.bed", "--edit-to", "g")
    assert r.returncode == 0, r.stderr
    assert lines_of("g.bed") == [ln + a + b for ln, a, b in zip(plain_bed, edit_columns(tuples, CBE), effect_columns(to_g))]
    cds_args = ("--cds", tmp_path / "cds.bed")
    for args, text in (((*base, *cds_args), "give -x"), ((*base, "--edit-to", "T"), "give -x"), ((*base, "--effect-filter", "stop_gained"), "give -x"),
                       ((*base, "--effects", tmp_path / "n.tsv"), "give -x"), ((*base, "-x", "CBE", "--effects", tmp_path / "n.tsv"), "give --cds"),
                       ((*base, "-x", "CBE", "--edit-to", "T"), "give --cds"), ((*base, "-x", "CBE", "-f", "missense"), "give --cds"),
                       ((*base, "-x", "CBE", *cds_args, "--edit-to", "C"), "--edit-to takes"), ((*base, "-x", "CBE", *cds_args, "-2", "TT"), "--edit-to takes"),
                       ((*base, "-x", "CBE", *cds_args, "-f", "nonsense"), "--effect-filter takes"),
                       ((*base, "-x", "CBE", *cds_args, "-f", "stop_gained+"), "--effect-filter takes"),
                       ((*base, "-x", "CBE", *cds_args, "-f", "/"), "--effect-filter takes")):
        r = run(*args)
        assert r.returncode != 0 and text in r.stderr, (args, r.stderr)
    assert not (tmp_path / "n.tsv").exists()
    (tmp_path / "bad.bed").write_text("%s\t50\t60\ta\t0\t+\n%s\t55\t70\tb\t0\t+\n" % (chrom[0], chrom[0]))  # two segments that overlap
    r = run(*base, "-x", "CBE", "--cds", tmp_path / "bad.bed")
    assert r.returncode != 0 and "overlaps" in (r.stderr + r.stdout)
    (tmp_path / "bad3.bed").write_text("%s\t50\t60\n" % chrom[0])
    r = run(*base, "-x", "CBE", "--cds", tmp_path / "bad3.bed")
    assert r.returncode != 0 and "BED6" in (r.stderr + r.stdout)

    # pattern_search -E -x START,LEN,BASE --cds --effects --effect-filter: Cas12a, an adenine editor's window; `to` is G by default
    pattern, proto = "TTTV" + "N" * 23, (4, 23)
    shape = (27, 8, 16, "A", "G")
    (tmp_path / "p.bed").write_text("".join("%s\t%d\t%d\n" % (chrom[c], a, b) for c, a, b in iv))
    found = gen.enumerate_pattern(pattern, proto, targets=iv)
    ptuples = ed.loci_tuples(found.loci)
    pids = ["%s:%d:%s" % (chrom[c], p, "-" if s else "+") for c, p, s in ptuples]
    pw = fx.expected(contigs, segments, ptuples, shape[:4], shape[4])
    pkeep = np.array([fx.keep(c, ("missense", "stop_lost", "start_lost"), ()) for c in pw["classes"]])
    assert len(found) >= 10 and pw["stats"]["effects"] >= 3 and 0 < pkeep.sum() < len(pkeep)
    pbase = ("pattern_search", "-i", tmp_path / "idx", "-q", pattern, "-p", "%d,%d" % proto, "-B", tmp_path / "p.bed", "-M", "2")
    r = run(*pbase, "-E", tmp_path / "pe.tsv", "-O", tmp_path / "po.tsv")
    assert r.returncode == 0, r.stderr
    pe, po = lines_of("pe.tsv"), lines_of("po.tsv")
    assert len(pe) == len(found) + 1
    r = run(*pbase, "-E", tmp_path / "pex.tsv", "-O", tmp_path / "pox.tsv", "-x", "8,16,A", "--cds", tmp_path / "cds.bed", "--effects", tmp_path / "pq.tsv")
    assert r.returncode == 0, r.stderr
    head = pe[0] + "\teditWindow\teditable\ttargetsHit\tcodingEdits\tstopGained\tmissense\tsynonymous"
    want_pe = [ln + a + b for ln, a, b in zip(pe[1:], edit_columns(ptuples, shape), effect_columns(pw))]
    assert lines_of("pex.tsv") == [head] + want_pe
    assert (tmp_path / "pox.tsv").read_bytes() == (tmp_path / "po.tsv").read_bytes()
    assert lines_of("pq.tsv") == effect_lines(pw, pids)
    r = run(*pbase, "-E", tmp_path / "pez.tsv", "-O", tmp_path / "poz.tsv", "-x", "8,16,A", "-d", tmp_path / "cds.bed", "-f", "missense+stop_lost+start_lost")
    assert r.returncode == 0, r.stderr
    assert lines_of("pez.tsv") == [head] + [ln for ln, k in zip(want_pe, pkeep) if k]
    assert lines_of("poz.tsv") == [po[0]] + [ln for ln, k in zip(po[1:], pkeep) if k]
    for args, text in (((*pbase, "-E", tmp_path / "x.tsv", "-O", tmp_path / "xo.tsv", "--cds", tmp_path / "cds.bed"), "give -x"),
                       ((*pbase, "-E", tmp_path / "x.tsv", "-O", tmp_path / "xo.tsv", "-x", "8,16,A", "-Q", tmp_path / "n.tsv"), "give --cds"),
                       ((*pbase, "-E", tmp_path / "x.tsv", "-O", tmp_path / "xo.tsv", "-x", "8,16,A", "-d", tmp_path / "cds.bed", "-2", "A"), "--edit-to takes")):
        r = run(*args)
        assert r.returncode != 0 and text in (r.stderr + r.stdout), (args, r.stderr)
    gen.close()
