"""Knock-out design on the device (vsc_loci_knockout, vsc_guides_knockout, vsc_pattern_guides_knockout and the two filters): bit
for bit what the definition gives when it is applied locus by locus on STRINGS (tests/knockout_cases.py), and the bytes of
vsc_knockout_site_text.  Integers, so there is no tolerance: the rows are compared as uint32, the undefined row included."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import effects_cases as fx
import knockout_cases as kc
import varscot_amd as va
import wide_cases as wc
from edit_cases import loci_tuples, locus_array
from helpers import random_seq
from varscot_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "varscot_amd", "bin")
FILTER_TILE = 1024  # candidates per wave of the filter's passes
GROUP = 256         # candidates per workgroup and step of the rows kernel
DROP_FRONT, DROP_BACK = 3, 1  # words the partial object of the small genome does not hold
COUNTED = ("defined", "undefined", "coding", "junction", "ptc", "nmd", "unknown", "transcripts_covered")
NO_LIMITS = (0, 65535, 0, 0, 0)


@pytest.fixture(scope="module")
def ctx():
    c = va.Context(0)
    yield c
    c.close()


def counted(stats):
    return {k: stats[k] for k in COUNTED}


def shape_of(t):
    return va.KnockoutShape(*t)


def limits_struct(lim, reserved=(0, 0, 0)):
    return _lib.KnockoutLimits(*lim, (C.c_uint32 * 3)(*reserved))


class Guides:
    """A vsc_guides (or, pattern=True, a vsc_pattern_guides) handle and its knock-out calls."""

    def __init__(self, ctx, handle, pattern=False):
        self.ctx, self.h, self.pattern = ctx, handle, pattern
        L = va.lib()
        kind = "vsc_pattern_guides" if pattern else "vsc_guides"
        self.fn = {k: getattr(L, "%s_%s" % (kind, k)) for k in ("count", "data", "free", "knockout", "filter_knockout", "filter_microhomology")}

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

    def rows(self, gen, shape, cds, coverage=False):
        rows, st = np.empty((len(self), 4), dtype=np.uint32), _lib.KnockoutStats()
        cov = np.full((cds.n_tx, 2), 9, dtype=np.uint32)
        sh = shape._struct()
        _lib.check(self.fn["knockout"](self.ctx._h, gen._h, self.h, C.byref(sh), cds._h, None, _lib.ptr(rows), _lib.ptr(cov) if coverage else None,
                                       C.byref(st)), self.ctx._h)
        return (rows, cov, st.as_dict()) if coverage else (rows, st.as_dict())

    def filter(self, gen, shape, cds, lim):
        out = C.c_void_p()
        sh, ls = shape._struct(), limits_struct(lim)
        _lib.check(self.fn["filter_knockout"](self.ctx._h, gen._h, self.h, C.byref(sh), cds._h, None, C.byref(ls), C.byref(out)), self.ctx._h)
        return Guides(self.ctx, out, self.pattern)

    def filter_mh(self, gen, mh, tenths, permille):
        out = C.c_void_p()
        sh = mh._struct()
        _lib.check(self.fn["filter_microhomology"](self.ctx._h, gen._h, self.h, C.byref(sh), tenths, permille, C.byref(out)), self.ctx._h)
        return Guides(self.ctx, out, self.pattern)

    def close(self):
        if self.h:
            self.fn["free"](self.h)
            self.h = None


# ---- 1. every locus of the small genome ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(ctx):
    """The small genome resident - whole, and as an object that lacks its first three words and its last one - every locus of
    it with the invalid ones, and the expected results per (shape, code, partial), computed once."""
    contigs, segments = kc.small_genome()
    packed = va.PackedGenome.from_sequences(list(contigs))
    loci = kc.every_locus(contigs) + kc.invalid_loci(contigs)
    sl = slice(DROP_FRONT, packed.n_words - DROP_BACK)
    part = va.Genome.from_shard(ctx, packed.hi[sl], packed.lo[sl], packed.nmask[sl], DROP_FRONT, sl.stop - sl.start, packed.contigs)
    s = {"contigs": contigs, "segments": segments, "packed": packed, "cds": va.Cds(packed, segments, n_tx=kc.N_TX), "gen": ctx.load_genome(packed),
         "part": part, "loci": loci, "arr": locus_array(loci), "resident": (32 * sl.start, 32 * sl.stop), "want": {}, "text": {}}

    def want(shape="SpCas9", code="standard", partial=False):
        key = (shape, code, partial)
        if key not in s["want"]:
            s["want"][key] = kc.expected(contigs, segments, loci, kc.SHAPES[shape], kc.CODES[code], s["resident"] if partial else None)
        return s["want"][key]

    def text(shape="SpCas9"):
        """the bytes of vsc_knockout_site_text, locus by locus"""
        if shape not in s["text"]:
            sh = shape_of(kc.SHAPES[shape])
            s["text"][shape] = np.array([va.knockout_site_text(s["cds"], contigs, c, p, st, sh) for c, p, st in loci], dtype=np.uint32)
        return s["text"][shape]

    s["expected"], s["site_text"] = want, text
    yield s
    s["gen"].close()
    part.close()
    s["cds"].close()


def past_the_bitmap(small, shape):
    """The defined loci whose cut has both of its bases in blocks of 256 global positions that no segment overlaps."""
    off = [int(o) for o in small["packed"].contigs["offset"]]
    occupied = {(off[c] + x) // 256 for c, s, e, *_ in small["segments"] for x in range(s, e)}
    site_len, cut = shape[:2]
    n = 0
    for c, p, strand in small["loci"]:
        if c < len(off) and strand <= 1 and p + site_len <= len(small["contigs"][c]):
            x = off[c] + (p + site_len - cut if strand else p + cut)
            n += (x - 1) // 256 not in occupied and x // 256 not in occupied
    return n


@pytest.mark.parametrize("code", sorted(kc.CODES))
@pytest.mark.parametrize("shape", sorted(kc.SHAPES))
def test_every_locus_of_the_small_genome(small, shape, code):
    sh = shape_of(kc.SHAPES[shape])
    letters = None if code == "standard" else kc.code_string(kc.CODES[code])
    whole = small["expected"](shape, code)
    rows, cov, stats = small["gen"].knockout(small["arr"], sh, small["cds"], coverage=True, code=letters)
    assert rows.dtype == np.uint32 and rows.shape == whole["rows"].shape and rows.tobytes() == whole["rows"].tobytes()
    assert cov.tobytes() == whole["coverage"].tobytes() and counted(stats) == whole["stats"]
    assert stats["defined"] + stats["undefined"] == len(small["loci"]) and stats["drained"] == stats["coding"] > 500
    assert stats["past_find"] == past_the_bitmap(small, kc.SHAPES[shape]) > 400  # inside the 500 bases without a segment
    if code == "standard":
        assert rows.tobytes() == small["site_text"](shape).tobytes()
    # the object that lacks its first three words and its last one: UNKNOWN from bases that are not resident
    want = small["expected"](shape, code, partial=True)
    rows, cov, stats = small["part"].knockout(small["arr"], sh, small["cds"], coverage=True, code=letters)
    assert rows.tobytes() == want["rows"].tobytes() and cov.tobytes() == want["coverage"].tobytes() and counted(stats) == want["stats"]
    assert want["stats"]["unknown"] > whole["stats"]["unknown"] and want["stats"]["coding"] == whole["stats"]["coding"]
    # without the coverage the rows are the same, and the stats still count the covered transcripts
    rows2, none, stats2 = small["part"].knockout(small["arr"], sh, small["cds"], code=letters)
    assert none is None and rows2.tobytes() == rows.tobytes() and counted(stats2) == want["stats"]


def test_the_partial_object_meets_both_ends(small):
    """A walk that leaves the held range behind transcript 6, and letters in front of the break that are not held in transcript 0."""
    want, whole = small["expected"](partial=True), small["expected"]()
    changed = {int(w[0]) for w, p in zip(whole["rows"], want["rows"]) if int(w[0]) != 0xFFFFFFFF and (w != p).any()}
    assert {0, 6} <= changed


def test_nothing_to_score(ctx, small):
    rows, cov, stats = small["gen"].knockout(locus_array([]), "SpCas9", small["cds"], coverage=True)
    assert rows.shape == (0, 4) and cov[:, 0].tolist() == [0] * kc.N_TX and (cov[:, 1] == kc.UNDEF).all()
    assert counted(stats) == dict(defined=0, undefined=0, coding=0, junction=0, ptc=[0, 0], nmd=[0, 0], unknown=0, transcripts_covered=0)
    t = ctx.timing()
    assert t["sites"] == 0 and t["score_ms"] == 0 and t["total_ms"] == 0 and t["genome_bytes"] == 0


# ---- 2. the queue at its edges; more candidates than one launch has lanes; the grid's cap ------------------------------------------
def launch_waves():
    """The waves of a launch capped as the cells' grids are (wide_cases): CUs x 8 workgroups of 4 waves."""
    return torch.cuda.get_device_properties(0).multi_processor_count * wc.GROUPS_PER_CU * wc.WAVES_PER_GROUP


def test_the_queue_at_its_edges(ctx, small):
    """At one workgroup per CU every workgroup takes the same steps: step t of workgroup b is candidates [(b + t CUs) 256, + 256),
    wave w of it the lanes [64 w, 64 w + 64).  The loci are laid out so that every workgroup meets, step by step: no coding lane;
    1 and then 63 in its first wave, whose slice of the queue then holds exactly 64; 64 in that wave at once; 65 - the first wave
    full and one lane of the second, which keeps that entry to the end -; four steps in which every lane of every wave is coding,
    so that the queue is drained while it is filled; and a last, partial step that leaves a partial queue for the final drain."""
    L = va.lib()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    text = small["site_text"]()
    coding = np.flatnonzero(text[:, 0] != 0xFFFFFFFF)
    other = np.flatnonzero(text[:, 0] == 0xFFFFFFFF)  # non-coding and undefined
    per_step = [0, 1, 63, 64, 65, GROUP, GROUP, GROUP, GROUP, 37]
    rng = np.random.default_rng(37)
    blocks, per_wave = [], np.zeros((cus, 4), dtype=np.int64)
    for t, k in enumerate(per_step):
        for b in range(cus):
            last = t + 1 == len(per_step) and b + 1 == cus
            block = rng.choice(other, 101 if last else GROUP)  # the very last block is a partial one
            at = np.arange(GROUP) if k == GROUP else np.concatenate([rng.permutation(64)[:min(k, 64)], np.arange(64, 64 + max(k - 64, 0))])
            block[at] = rng.choice(coding, len(at))
            blocks.append(block)
            per_wave[b] += np.bincount(at // 64, minlength=4)
    idx = np.concatenate(blocks)
    n = len(idx)
    assert n == (len(per_step) * cus - 1) * GROUP + 101
    want = text[idx]
    n_coding = int((want[:, 0] != 0xFFFFFFFF).sum())
    assert n_coding == cus * sum(per_step) == per_wave.sum()
    try:
        assert L.vsc_debug_knockout_groups_per_cu(ctx._h, 1) == 0
        rows, cov, stats = small["gen"].knockout(small["arr"][idx], "SpCas9", small["cds"], coverage=True)
    finally:
        L.vsc_debug_knockout_groups_per_cu(ctx._h, 0)
    assert rows.tobytes() == want.tobytes()
    assert stats["coding"] == stats["drained"] == n_coding
    # a wave drains every whole 64 of its entries as soon as it holds them, and what is left once more at the end
    assert per_wave[0].tolist() == [1 + 63 + 64 + 64 + 4 * 64 + 37, 1 + 4 * 64, 4 * 64, 4 * 64]
    assert stats["drains"] == int((per_wave // 64 + (per_wave % 64 > 0)).sum()) == cus * (8 + 5 + 4 + 4)
    both = (want[:, 0] != 0xFFFFFFFF) & ((want[:, 2] >> 24) & 48 == 48)
    assert int(cov[:, 0].sum()) == int(both.sum())


def test_more_candidates_than_a_launch_has_lanes(small):
    want = small["expected"]("open", "standard", partial=True)
    n, m = launch_waves() * 64 + 77, len(small["loci"])
    assert n > 3 * m  # every lane meets more than one tiling of the loci
    idx = np.arange(n) % m
    rows, cov, stats = small["part"].knockout(small["arr"][idx], shape_of(kc.SHAPES["open"]), small["cds"], coverage=True)
    assert rows.tobytes() == want["rows"][idx].tobytes()
    times = np.bincount(idx, minlength=m)
    flags = want["rows"][:, 2] >> 24
    is_coding = np.array([d is not None for d in want["detail"]])
    assert stats["coding"] == int(times[is_coding].sum()) == stats["drained"] and stats["defined"] + stats["undefined"] == n
    for k in (0, 1):
        assert stats["ptc"][k] == int(times[is_coding & (flags >> (2 + k) & 1 == 1)].sum())
        assert stats["nmd"][k] == int(times[is_coding & (flags >> (4 + k) & 1 == 1)].sum())
    both = is_coding & (flags & 48 == 48)
    for t in range(kc.N_TX):  # the coverage of the repeated loci: every candidate counted as often as it occurs
        mine = both & (want["rows"][:, 0] == t)
        assert int(cov[t, 0]) == int(times[mine].sum()) and cov[t, 1] == want["coverage"][t, 1]
    assert want["stats"]["transcripts_covered"] == stats["transcripts_covered"] >= 2


def test_one_workgroup_per_cu_takes_many_steps_to_the_same_bytes(ctx, small):
    L = va.lib()
    want = small["expected"]()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    m = len(small["loci"])
    n = cus * GROUP * 5 + 131  # five steps of every workgroup and a partial one at one workgroup per CU
    idx = np.arange(n) % m
    got = {}
    try:
        for groups in (0, 1, 3, 64, 0):
            assert L.vsc_debug_knockout_groups_per_cu(ctx._h, groups) == 0
            rows, cov, stats = small["gen"].knockout(small["arr"][idx], "SpCas9", small["cds"], coverage=True)
            got[groups] = (rows.tobytes(), cov.tobytes(), str(counted(stats)))
    finally:
        L.vsc_debug_knockout_groups_per_cu(ctx._h, 0)
    assert got[0][0] == want["rows"][idx].tobytes() and len(set(got.values())) == 1
    try:  # the variant without the queue, which the queue is measured against: the same bytes
        assert L.vsc_debug_knockout_in_place(ctx._h, 1) == 0
        rows, cov, stats = small["gen"].knockout(small["arr"][idx], "SpCas9", small["cds"], coverage=True)
    finally:
        L.vsc_debug_knockout_in_place(ctx._h, 0)
    assert (rows.tobytes(), cov.tobytes(), str(counted(stats))) == got[0] and stats["drained"] == stats["coding"] and stats["drains"] > n // 256
    assert L.vsc_debug_knockout_in_place(None, 1) == -22
    assert L.vsc_debug_knockout_groups_per_cu(ctx._h, 65) == -22 and L.vsc_debug_knockout_groups_per_cu(None, 1) == -22


def test_filter_over_more_tiles_than_a_launch_has_waves(ctx, small):
    want = small["expected"]("open")
    m = len(small["loci"])
    n = (launch_waves() + 3) * FILTER_TILE + 77  # the last tile is a partial one
    idx = np.arange(n) % m
    lim = (3277, 42598, 2, kc.NMD1 | kc.NMD2, kc.UNKNOWN_FLAG)
    keep = np.array([kc.keep(r, lim) for r in want["rows"]])
    assert 10 < keep.sum() < want["stats"]["coding"]
    codes = np.arange(n, dtype=np.uint64) * np.uint64(3)  # (the filter copies codes, it does not read them)
    g = Guides.from_arrays(ctx, codes, small["arr"][idx])
    out = g.filter(small["gen"], shape_of(kc.SHAPES["open"]), small["cds"], lim)
    got_codes, got_loci = out.arrays()
    chosen = np.nonzero(keep[idx])[0]
    assert len(got_codes) == len(chosen)
    assert got_codes.tobytes() == codes[chosen].tobytes() and got_loci.tobytes() == small["arr"][idx][chosen].tobytes()
    t = ctx.timing()
    assert t["sites"] == n and t["genome_bytes"] == 32 * n + 48 * len(chosen) and t["score_ms"] == t["total_ms"] > 0
    out.close()
    g.close()


# ---- 3. device-resident candidates ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted(ctx):
    """A 9 kb random genome under exon-like segments, three per transcript on either strand with every first phase."""
    rng = np.random.default_rng(837)
    contigs = [random_seq(rng, n) for n in (5000, 2500, 1500)]
    segments, n_tx = fx.random_cds(rng, contigs)
    packed = va.PackedGenome.from_sequences(contigs)
    cds = va.Cds(packed, segments, n_tx=n_tx)
    gen = ctx.load_genome(packed)
    yield {"contigs": contigs, "segments": segments, "n_tx": n_tx, "packed": packed, "cds": cds, "gen": gen}
    gen.close()
    cds.close()


def planted_want(planted, loci, shape, **kw):
    return kc.expected(planted["contigs"], planted["segments"], loci_tuples(loci), shape, n_tx=planted["n_tx"], **kw)


def test_enumerated_guides_get_their_rows_where_they_lie(planted):
    gen, cds = planted["gen"], planted["cds"]
    kw = dict(knockout="SpCas9", knockout_cds=cds)
    plain = gen.enumerate_guides()
    codes, loci, rows = gen.enumerate_guides(**kw)
    assert codes.tobytes() == plain[0].tobytes() and loci.tobytes() == plain[1].tobytes() and len(codes) > 500
    want = planted_want(planted, loci, kc.SHAPES["SpCas9"])
    assert want["stats"]["coding"] > 100 and want["stats"]["nmd"][0] > 5 and want["stats"]["nmd"][1] > 5 and want["stats"]["junction"] >= 1
    assert rows.dtype == np.uint32 and rows.tobytes() == want["rows"].tobytes()
    by_loci, cov, stats = gen.knockout(loci, "SpCas9", cds, coverage=True)
    assert by_loci.tobytes() == want["rows"].tobytes() and cov.tobytes() == want["coverage"].tobytes() and counted(stats) == want["stats"]
    assert gen.knockout((codes, loci), va.KNOCKOUT_SHAPES["SpCas9"], cds)[0].tobytes() == want["rows"].tobytes()
    # N x 21 + GG under the pattern enumeration: the same sites, the same rows
    found, prows = gen.enumerate_pattern("N" * 21 + "GG", (0, 20), **kw)
    assert found.loci.tobytes() == loci.tobytes() and prows.tobytes() == want["rows"].tobytes()
    assert gen.knockout(found, "SpCas9", cds)[0].tobytes() == want["rows"].tobytes()
    # the knock-out rows come last of all, after the motif rows
    ms = va.motifs([("BsmBI", "CGTCTC", True)])
    both = gen.enumerate_guides(fold="SpCas9", motifs="SpCas9", motif_set=ms, **kw)
    assert len(both) == 5 and both[1].tobytes() == loci.tobytes() and both[4].tobytes() == want["rows"].tobytes()
    assert both[3].tobytes() == gen.enumerate_guides(motifs="SpCas9", motif_set=ms)[2].tobytes()
    for bad in (dict(knockout="SpCas9"), dict(knockout_cds=cds), dict(min_cut_frac=0.1), dict(require_knockout="nmd1"),
                dict(knockout=va.KnockoutShape(27, 22), knockout_cds=cds), dict(knockout="SpCas9", knockout_cds=cds, min_cut_frac=0.7, max_cut_frac=0.3),
                dict(knockout="SpCas9", knockout_cds=cds, require_knockout="nmd3"), dict(knockout="SpCas9", knockout_cds=cds, min_cut_edge=256)):
        with pytest.raises(ValueError):
            gen.enumerate_guides(**bad)
    with pytest.raises(ValueError):
        gen.enumerate_pattern("N" * 21 + "GG", (0, 20), forbid_knockout="unknown")


@pytest.mark.parametrize("pattern,proto,shape", [("N" * 21 + "NNGRRT", (0, 21), (27, 18, 50, 0, 4096)), ("TTTV" + "N" * 23, (4, 23), (27, 22, 50, 10, 4096))],
                         ids=["SaCas9", "Cas12a"])
def test_pattern_candidates_at_other_site_lengths(planted, pattern, proto, shape):
    gen, cds = planted["gen"], planted["cds"]
    sh = shape_of(shape)
    plain = gen.enumerate_pattern(pattern, proto)
    kw = dict(knockout=sh, knockout_cds=cds)
    found, rows = gen.enumerate_pattern(pattern, proto, **kw)
    assert found.codes.tobytes() == plain.codes.tobytes() and found.loci.tobytes() == plain.loci.tobytes() and 100 < len(found)
    want = planted_want(planted, found.loci, shape)
    assert want["stats"]["coding"] > 20 and rows.tobytes() == want["rows"].tobytes()
    # the limits, through the wrapper: the survivors in input order, their rows; only the survivors are searched
    lim = (va.knockout_cut_frac(0.05), va.knockout_cut_frac(0.65, upper=True), 2, kc.PTC1 | kc.PTC2, kc.UNKNOWN_FLAG)
    keep = np.array([kc.keep(r, lim) for r in want["rows"]])
    assert 0 < keep.sum() < want["stats"]["coding"]
    kw.update(min_cut_frac=0.05, max_cut_frac=0.65, min_cut_edge=2, require_knockout="ptc1+ptc2", forbid_knockout=["unknown"])
    kept, krows = gen.enumerate_pattern(pattern, proto, **kw)
    assert kept.codes.tobytes() == found.codes[keep].tobytes() and kept.loci.tobytes() == found.loci[keep].tobytes()
    assert krows.tobytes() == want["rows"][keep].tobytes()
    targets = [(0, 0, 2400), (1, 300, 2500), (2, 0, 1500)]
    d_found, d_rows, d_ko = gen.design_pattern(pattern, proto, 2, targets=targets, **kw)
    t_found, t_rows = gen.enumerate_pattern(pattern, proto, targets=targets, **kw)
    assert d_found.codes.tobytes() == t_found.codes.tobytes() and d_ko.tobytes() == t_rows.tobytes() and len(t_found) > 3
    pick = va.PickShape(site_len=27, k=2, spacing=5)
    out = gen.design_pattern(pattern, proto, 2, targets=targets, pick=pick, pick_by=["knockout"], knockout=sh, knockout_cds=cds)
    assert len(out) == 5 and out[2].tobytes() == gen.enumerate_pattern(pattern, proto, targets=targets, knockout=sh, knockout_cds=cds)[1].tobytes()


def test_calls_refuse_before_anything_is_written(ctx, planted, small):
    L = va.lib()
    gen, cds = planted["gen"], planted["cds"]
    p = va.api._enum_params("GG", "both", (0, 0), 0, 0)
    h = C.c_void_p()
    _lib.check(L.vsc_guides_enumerate(ctx._h, gen._h, None, C.byref(p), C.byref(h)), ctx._h)
    g = Guides(ctx, h)
    rows = np.full((len(g), 4), 7, dtype=np.uint32)
    cov = np.full((planted["n_tx"], 2), 7, dtype=np.uint32)
    arr = locus_array([(0, 100, 0)])
    ok = (23, 17, 50, 0, 4096)

    def calls(shape=ok, reserved=(0, 0, 0), code=None, ctx_h=ctx._h, gen_h=gen._h, guides=g.h, loci=arr, cds_h=cds._h, lim=NO_LIMITS,
              lim_reserved=(0, 0, 0), which=(0, 1, 2), n=1):
        sh = C.byref(_lib.KnockoutShapeStruct(*shape, (C.c_uint32 * 3)(*reserved))) if shape is not None else None
        ls = C.byref(limits_struct(lim, lim_reserved)) if lim is not None else None
        out = C.c_void_p()
        made = [lambda: L.vsc_guides_knockout(ctx_h, gen_h, guides, sh, cds_h, code, _lib.ptr(rows), _lib.ptr(cov), None),
                lambda: L.vsc_loci_knockout(ctx_h, gen_h, _lib.ptr(loci) if loci is not None else None, n, sh, cds_h, code, _lib.ptr(rows), _lib.ptr(cov),
                                            None),
                lambda: L.vsc_guides_filter_knockout(ctx_h, gen_h, guides, sh, cds_h, code, ls, C.byref(out))]
        return [made[k]() for k in which], out  # (only the calls the case is about: another one may be in order and write)

    def refused(which=(0, 1, 2), code_want=-22, **kw):
        codes, out = calls(which=which, **kw)
        return all(c == code_want for c in codes) and (rows == 7).all() and (cov == 7).all() and not out.value

    assert refused(which=(0, 2), shape=(27, 22, 50, 0, 4096)) and "site_len" in L.vsc_last_error(ctx._h).decode()
    for shape in ((15, 7, 50, 0, 4096), (33, 17, 50, 0, 4096), (23, 0, 50, 0, 4096), (23, 23, 50, 0, 4096), (23, 17, 65536, 0, 4096),
                  (23, 17, 50, 65536, 4096), (23, 17, 50, 0, 0), (23, 17, 50, 0, 4097)):  # every value outside SHAPE, by the library
        assert refused(shape=shape), shape
    for k in range(3):
        assert refused(reserved=tuple(int(i == k) for i in range(3)))
        assert refused(which=(2,), lim_reserved=tuple(int(i == k) for i in range(3)))
    for lim in ((0, 65535, 0, 128, 0), (0, 65535, 0, 0, 128), (0, 65535, 0, 1 << 31, 0), (5, 4, 0, 0, 0), (0, 65536, 0, 0, 0), (0, 65535, 256, 0, 0)):
        assert refused(which=(2,), lim=lim) and "min_frac" in L.vsc_last_error(ctx._h).decode(), lim
    assert refused(which=(2,), lim=None)
    assert refused(code=b"K" * 63) and "64 letters" in L.vsc_last_error(ctx._h).decode()
    assert refused(shape=None) and refused(gen_h=None) and refused(cds_h=None) and refused(which=(0, 2), guides=None) and refused(which=(1,), loci=None)
    assert refused(which=(1,), n=0xFFFFFFFF, code_want=-34) and "0xFFFFFFFE" in L.vsc_last_error(ctx._h).decode()
    st = _lib.KnockoutShapeStruct(*ok, (C.c_uint32 * 3)(0, 0, 0))
    ls = limits_struct(NO_LIMITS)
    assert L.vsc_guides_filter_knockout(ctx._h, gen._h, g.h, C.byref(st), cds._h, None, C.byref(ls), None) == -22
    # a CDS built with another contig table than the genome's
    assert refused(cds_h=small["cds"]._h) and "contig table" in L.vsc_last_error(ctx._h).decode()
    other = va.Context(0)  # a genome, or an object, of another context is refused
    assert refused(which=(1,), ctx_h=other._h)
    gen2 = other.load_genome(planted["packed"])
    assert refused(which=(0, 2), ctx_h=other._h, gen_h=gen2._h) and "another context" in L.vsc_last_error(other._h).decode()
    gen2.close()
    other.close()
    with pytest.raises(va.VarscotError):
        gen.knockout(arr, va.KnockoutShape(23, 23, validate=False), cds)
    codes, out = calls()  # and with everything in order the three calls work
    assert codes == [0, 0, 0] and out.value and not (rows == 7).all() and not (cov == 7).any()
    L.vsc_guides_free(out)
    g.close()


# ---- 4. the filter --------------------------------------------------------------------------------------------------------------
def test_filter_limits_and_what_takes_the_result(ctx, small, planted):
    sh = shape_of(kc.SHAPES["open"])
    want = small["expected"]("open")
    n = len(small["loci"])
    is_coding = np.array([d is not None for d in want["detail"]])
    codes = np.arange(n, dtype=np.uint64) * np.uint64(5)
    g = Guides.from_arrays(ctx, codes, small["arr"])
    trials = [NO_LIMITS, (20000, 65535, 0, 0, 0), (0, 30000, 0, 0, 0), (0, 65535, 5, 0, 0), (0, 65535, 0, kc.NMD1, 0), (0, 65535, 0, kc.NMD1 | kc.NMD2, 0),
              (0, 65535, 0, 0, kc.UNKNOWN_FLAG), (0, 65535, 0, kc.FIRST, 0), (0, 65535, 0, 0, kc.LAST | kc.FIRST), (0, 65535, 0, kc.PTC2, kc.PTC1),
              (3277, 42598, 2, kc.NMD1 | kc.NMD2, kc.UNKNOWN_FLAG | kc.LAST), (0, 65535, 0, 0x7F, 0)]
    kept_by = {}
    for lim in trials:  # each limit alone and together, against the rule on the restatement's rows
        keep = np.array([kc.keep(r, lim) for r in want["rows"]])
        out = g.filter(small["gen"], sh, small["cds"], lim)
        got_codes, got_loci = out.arrays()
        out.close()
        assert got_codes.tobytes() == codes[keep].tobytes() and got_loci.tobytes() == small["arr"][keep].tobytes(), lim
        kept_by[lim] = keep
    assert kept_by[NO_LIMITS].sum() == is_coding.sum() and kept_by[trials[-1]].sum() == 0
    for lim in trials[1:-1]:
        assert 0 < kept_by[lim].sum() < is_coding.sum(), lim
    # an empty result is a result; the host-only object goes the host's way, to the same bytes
    nothing = Guides.from_arrays(ctx, codes[~is_coding], small["arr"][~is_coding])
    empty = nothing.filter(small["gen"], sh, small["cds"], NO_LIMITS)
    assert len(empty) == 0 and empty.rows(small["gen"], sh, small["cds"])[0].shape == (0, 4)
    empty.close()
    nothing.close()
    host = Guides.from_arrays(ctx, codes, small["arr"], on_device=False)
    h_rows, h_cov, h_stats = host.rows(small["gen"], sh, small["cds"], coverage=True)
    assert h_rows.tobytes() == want["rows"].tobytes() and h_cov.tobytes() == want["coverage"].tobytes() and counted(h_stats) == want["stats"]
    h_out = host.filter(small["gen"], sh, small["cds"], trials[-2])
    assert h_out.arrays()[0].tobytes() == codes[kept_by[trials[-2]]].tobytes()
    h_out.close()
    host.close()
    g.close()

    # before and after an existing filter: the microhomology floor and the knock-out limits commute
    gen, cds = planted["gen"], planted["cds"]
    pcodes, ploci, pairs, prows = gen.enumerate_guides(microhomology=va.MicrohomologyShape(), knockout="SpCas9", knockout_cds=cds)
    lim = (va.knockout_cut_frac(0.05), va.knockout_cut_frac(0.65, upper=True), 0, kc.NMD1, 0)
    keep = np.array([kc.keep(r, lim) for r in prows])
    mh = va.MicrohomologyShape()
    tenths = int(np.median(pairs[pairs[:, 0] != va.MH_UNDEFINED, 0]))  # the floor, in tenths of the score's unit
    mh_keep = (pairs[:, 0] != va.MH_UNDEFINED) & (pairs[:, 0] >= tenths)
    assert 0 < (keep & mh_keep).sum() < keep.sum()
    g = Guides.from_arrays(ctx, pcodes, ploci)
    a = g.filter(gen, va.KNOCKOUT_SHAPES["SpCas9"], cds, lim)
    ab = a.filter_mh(gen, mh, tenths, 0)
    b = g.filter_mh(gen, mh, tenths, 0)
    ba = b.filter(gen, va.KNOCKOUT_SHAPES["SpCas9"], cds, lim)
    assert ab.arrays()[0].tobytes() == ba.arrays()[0].tobytes() == pcodes[keep & mh_keep].tobytes()
    assert ab.arrays()[1].tobytes() == ploci[keep & mh_keep].tobytes()
    for x in (a, ab, b, ba, g):
        x.close()
    # through the wrapper the knock-out filter runs after the existing ones, and its rows come after theirs
    fkw = dict(knockout="SpCas9", knockout_cds=cds, min_cut_frac=0.05, max_cut_frac=0.65, require_knockout="nmd1")
    k_codes, k_loci, k_pairs, k_rows = gen.enumerate_guides(microhomology=mh, min_microhomology=tenths / 10.0, **fkw)
    assert k_codes.tobytes() == pcodes[keep & mh_keep].tobytes() and k_rows.tobytes() == prows[keep & mh_keep].tobytes()
    assert k_pairs.tobytes() == pairs[keep & mh_keep].tobytes()
    # the survivors feed the search as the candidates selected on the host do
    k_codes, k_loci, k_rows = gen.enumerate_guides(**fkw)
    rows_all = gen.summarize(pcodes, 2, exclude=ploci)
    d = gen.design(None, 2, **fkw)
    assert len(d) == 4 and d[0].tobytes() == k_codes.tobytes() and d[2].tobytes() == rows_all[keep].tobytes() and d[3].tobytes() == k_rows.tobytes()


def test_the_knockout_column_picks_the_guides_of_every_target(planted):
    """Genome.knockout -> pick_by="knockout" -> Genome.pick, against the restatement and va.pick_host."""
    gen, cds = planted["gen"], planted["cds"]
    # one target per transcript: its coding span
    spans = {}
    for c, s, e, tx, _, _ in planted["segments"]:
        spans[tx] = (c, min(spans[tx][1], s), max(spans[tx][2], e)) if tx in spans else (c, s, e)
    iv = [spans[t] for t in sorted(spans)]
    regions = va.Regions(planted["packed"], iv, rule="overlap")
    pick = va.PickShape(k=3, spacing=10)
    shape = kc.SHAPES["open"]
    out = gen.design(regions, 2, knockout=shape_of(shape), knockout_cds=cds, pick=pick, pick_by=["knockout", "mit"])
    codes, loci, rows, kos, picks, n_picked = out
    want = planted_want(planted, loci, shape)
    assert kos.tobytes() == want["rows"].tobytes()
    by_loci = gen.knockout((codes, loci), shape_of(shape), cds)[0]
    assert by_loci.tobytes() == kos.tobytes()
    col = va.pick_column("knockout", by_loci)
    assert col.tobytes() == kc.pick_column(want["rows"]).tobytes() and len(set(col.tolist())) > 20 and (col >> np.uint64(16)).any()
    spec = np.array([va.mit_specificity(x) for x in rows["mit_sum"]], dtype=np.float64)
    key = va.pick_key([col, va.pick_column("mit", spec)], [va.PICK_COLUMNS["knockout"], va.PICK_COLUMNS["mit"]])
    w_picks, w_counts, _ = gen.pick((codes, loci), key, pick, regions=regions)
    assert picks.tobytes() == w_picks.tobytes() and n_picked.tobytes() == w_counts.tobytes() and (n_picked > 0).sum() > 5
    labels = np.array([regions.locate(c, p) for c, p, _ in loci_tuples(loci)], dtype=np.uint32)
    h_picks, h_counts, _ = va.pick_host(planted["packed"].contigs, loci, labels, key, len(iv), pick)
    assert picks.tobytes() == h_picks.tobytes() and n_picked.tobytes() == h_counts.tobytes()
    for t, i in enumerate(picks[:, 0]):  # the first pick of every target: NMD in both frames if any has it, then the earliest cut
        if n_picked[t]:
            assert labels[i] == t and col[i] == col[labels == t].max()
    with pytest.raises(ValueError):
        gen.design(regions, 2, pick=pick, pick_by=["knockout"])  # the column needs knockout=
    regions.close()


# ---- 5. repetition and the context's state ------------------------------------------------------------------------------------
def test_alternating_cds_objects_leave_nothing_behind(ctx, small):
    gen, arr, contigs, segments = small["gen"], small["arr"], small["contigs"], small["segments"]
    loci = small["loci"]
    first_half = tuple(s for s in segments if s[0] < 2)
    objects = [(small["cds"], segments, kc.N_TX), (va.Cds(small["packed"], [], n_tx=0), (), 0), (va.Cds(small["packed"], first_half, n_tx=2), first_half, 2)]
    shape = kc.SHAPES["open"]
    want = [kc.expected(contigs, segs, loci, shape, n_tx=n_tx) for _, segs, n_tx in objects]
    assert want[1]["stats"]["coding"] == 0 and want[1]["stats"]["junction"] == 0 and 0 < want[2]["stats"]["coding"] < want[0]["stats"]["coding"]
    assert len({w["rows"].tobytes() for w in want}) == 3

    def call(k):
        rows, cov, stats = gen.knockout(arr, shape_of(shape), objects[k][0], coverage=True)
        assert rows.tobytes() == want[k]["rows"].tobytes() and cov.tobytes() == want[k]["coverage"].tobytes() and counted(stats) == want[k]["stats"], k
        return stats

    for k in (0, 0, 1, 0, 2, 2, 1, 1, 2, 0):  # no stale segments, no stale table, no stale bitmap
        call(k)
    # an effects call between two knock-out calls shares the segments' copy and leaves the table and the bitmap alone
    eff = gen.effects(arr, "CBE", None, objects[2][0])[0]
    call(0)
    assert gen.effects(arr, "CBE", None, objects[2][0])[0].tobytes() == eff.tobytes()
    call(2)
    ctx.release_scratch()
    call(1)
    ctx.release_scratch()
    stats = call(0)
    assert stats["kernel_ms"] > 0 and stats["wall_ms"] >= stats["kernel_ms"]
    t = ctx.timing()
    assert t["score_ms"] > 0 and t["total_ms"] == t["score_ms"] and t["sites"] == len(loci) and t["genome_bytes"] == 32 * len(loci)
    for k in ("scan_ms", "prep_ms", "sort_ms", "finalize_ms", "index_ms", "pairs", "hits", "passes", "sort_bytes", "sort_levels", "list_entries"):
        assert t[k] == 0, k
    for cds, _, _ in objects[1:]:
        cds.close()


# ---- 6. the tools end to end --------------------------------------------------------------------------------------------------
def test_tools_list_and_filter_their_guides(ctx, tmp_path):
    rng = np.random.default_rng(937)
    contigs = [random_seq(rng, 6000), "TTTA" + random_seq(rng, 2996)]
    segments, n_tx = fx.random_cds(rng, contigs)
    names = ["chr1 assembled", "chr2"]
    chrom = [n.split()[0] for n in names]
    with open(tmp_path / "g.fa", "w") as f:
        for n, s in zip(names, contigs):
            f.write(">%s\n%s\n" % (n, "\n".join(s[i:i + 60] for i in range(0, len(s), 60))))
    iv = [(0, 0, 2500), (1, 100, 1400), (0, 5000, 6000)]
    (tmp_path / "t.bed").write_text("".join("%s\t%d\t%d\tx\n" % (chrom[c], a, b) for c, a, b in iv))
    # the transcripts are named in the order the sorted segments meet them, which is their index here
    (tmp_path / "cds.bed").write_text("".join("%s\t%d\t%d\ttx%d\t%d\t%s\n" % (chrom[c], s, e, tx, ph, "-" if st else "+")
                                              for c, s, e, tx, st, ph in segments))
    run = lambda *a: subprocess.run([os.path.join(BIN, a[0])] + [str(x) for x in a[1:]], capture_output=True, text=True, timeout=600)  # noqa: E731
    assert run("bidir_index", "-G", tmp_path / "g.fa", "-I", tmp_path / "idx").returncode == 0
    packed = va.PackedGenome.from_sequences(contigs)
    gen = ctx.load_genome(packed)
    cds = va.Cds(packed, segments, n_tx=n_tx)

    def distance(d):
        return {kc.END: "END", kc.CAP: "CAP", kc.UNKNOWN: "NA"}.get(int(d), str(int(d)))

    def columns(rows):
        u = va.unpack_knockout_row(rows)
        out = []
        for r in u:
            if not r["defined"]:
                out.append("\tNA" * 8)
            elif not r["coding"]:
                out.append(("\tjunction" if r["flags"] & 128 else "\t-") + "\t-" * 7)
            else:
                tenths = int(r["frac"]) * 1000 // 65536
                nmd = {0: "-", 16: "1", 32: "2", 48: "1+2"}[int(r["flags"]) & 48]
                out.append("\ttx%d\t%d\t%d\t%d.%d\t%d\t%s\t%s\t%s" % (r["transcript"], r["codon"], r["frame"], tenths // 10, tenths % 10, r["edge"],
                                                                      distance(r["d1"]), distance(r["d2"]), nmd))
        return out

    header = "\tkoTranscript\tkoCodon\tkoFrame\tkoCutPct\tkoEdge\tkoPtc1\tkoPtc2\tkoNmd"
    # guide_summary -E -L --knockout [...]
    regions = va.Regions(packed, iv, rule="inside")
    kw = dict(knockout=va.KnockoutShape(23, 17, 30, 5), knockout_cds=cds)
    codes, loci, rows = gen.enumerate_guides(regions, **kw)
    u = va.unpack_knockout_row(rows)
    assert 50 < len(codes) < 900 and 10 < u["coding"].sum() < len(codes)
    lim = (va.knockout_cut_frac(0.05), va.knockout_cut_frac(0.655, upper=True), 3, kc.PTC1, kc.UNKNOWN_FLAG | kc.LAST)
    keep = np.array([kc.keep(r, lim) for r in rows])
    assert 0 < keep.sum() < u["coding"].sum()
    base = ("guide_summary", "-G", tmp_path / "g.fa", "-I", tmp_path / "idx", "-M", "2", "-E", tmp_path / "t.bed")
    r = run(*base, "-L", tmp_path / "plain.bed", "-O", tmp_path / "plain.tsv")
    assert r.returncode == 0, r.stderr
    opts = ("--knockout", "--knockout-cds", tmp_path / "cds.bed", "--knockout-nmd", "30,5")
    r = run(*base, "-L", tmp_path / "f.bed", "-O", tmp_path / "f.tsv", *opts, "--knockout-out", tmp_path / "rows.tsv")
    assert r.returncode == 0, r.stderr
    plain_bed = (tmp_path / "plain.bed").read_text().splitlines()
    plain_rows = (tmp_path / "plain.tsv").read_text().splitlines()
    assert len(plain_bed) == len(codes)
    assert (tmp_path / "f.tsv").read_bytes() == (tmp_path / "plain.tsv").read_bytes()  # --knockout adds to the listing alone
    want_bed = [ln + col for ln, col in zip(plain_bed, columns(rows))]
    assert (tmp_path / "f.bed").read_text().splitlines() == want_bed
    listed = (tmp_path / "rows.tsv").read_text().splitlines()
    assert listed[0] == "#guideId" + header + "\tkoFlags"
    flags = ["+".join(n for k, n in enumerate(kc.FLAGS) if r["flags"] >> k & 1) or "-" if r["coding"] else "-" for r in u]
    assert listed[1:] == [ln.split("\t")[3] + col + "\t" + f for ln, col, f in zip(plain_bed, columns(rows), flags)]
    r = run(*base, "-L", tmp_path / "k.bed", "-O", tmp_path / "k.tsv", *opts, "--knockout-filter", "5,65.5,3,ptc1/unknown+last")
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "k.bed").read_text().splitlines() == [ln for ln, k in zip(want_bed, keep) if k]
    assert (tmp_path / "k.tsv").read_text().splitlines() == [plain_rows[0]] + [ln for ln, k in zip(plain_rows[1:], keep) if k]
    r = run(*base, "-L", tmp_path / "c.bed", "-O", tmp_path / "c.tsv", "--knockout", "17", "--knockout-cds", tmp_path / "cds.bed", "--knockout-nmd=30,5")
    assert r.returncode == 0 and (tmp_path / "c.bed").read_bytes() == (tmp_path / "f.bed").read_bytes()  # the cut spelled out
    regions.close()
    # refused combinations, before a device is opened
    for bad, word in ((("--knockout-cds", tmp_path / "cds.bed"), "give --knockout"), (("--knockout",), "give --knockout-cds"),
                      (("--knockout", "23", "--knockout-cds", tmp_path / "cds.bed"), "cut of 1 .. 22"),
                      (opts + ("--knockout-filter", "70,20"), "MINPCT"), (opts + ("--knockout-filter", "5,65,3,nmd3"), "MINPCT"),
                      (("--knockout", "--knockout-cds", tmp_path / "cds.bed", "--knockout-nmd", "70000"), "WINDOW")):
        r = subprocess.run([os.path.join(BIN, "guide_summary")] + [str(x) for x in base[1:] + bad + ("-L", tmp_path / "x.bed", "-O", tmp_path / "x.tsv")],
                           capture_output=True, text=True, timeout=120, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
        assert r.returncode == 1 and word in r.stderr, (bad, r.stderr)
    r = run("guide_summary", "-G", tmp_path / "g.fa", "-I", tmp_path / "idx", "-M", "2", "-R", tmp_path / "g.fa", "-O", tmp_path / "x.tsv", *opts)
    assert r.returncode == 1 and "give -E" in r.stderr

    # pattern_search -E --knockout: Cas12a, the default cut of a site of 27 bases
    pattern, proto = "TTTV" + "N" * 23, (4, 23)
    targets = [(0, 0, 3000), (1, 0, 3000)]
    (tmp_path / "p.bed").write_text("".join("%s\t%d\t%d\n" % (chrom[c], a, b) for c, a, b in targets))
    pkw = dict(knockout=va.KnockoutShape(27, 22), knockout_cds=cds)
    found, prows = gen.enumerate_pattern(pattern, proto, targets=targets, **pkw)
    plim = (0, 65535, 0, kc.NMD1 | kc.NMD2, 0)
    pkeep = np.array([kc.keep(r, plim) for r in prows])
    assert len(found) > 40 and 0 < pkeep.sum() < len(pkeep)
    pbase = ("pattern_search", "-i", tmp_path / "idx", "-q", pattern, "-p", "%d,%d" % proto, "-B", tmp_path / "p.bed", "-M", "2")
    r = run(*pbase, "-E", tmp_path / "pe.tsv", "-O", tmp_path / "po.tsv")
    assert r.returncode == 0, r.stderr
    popts = ("--knockout", "--knockout-cds", tmp_path / "cds.bed")
    r = run(*pbase, "-E", tmp_path / "pef.tsv", "-O", tmp_path / "pof.tsv", *popts)
    assert r.returncode == 0, r.stderr
    pe = (tmp_path / "pe.tsv").read_text().splitlines()
    po = (tmp_path / "po.tsv").read_text().splitlines()
    assert len(pe) == len(found) + 1 and pe[0] == "#guide\tchrom\tpos\tstrand"
    assert (tmp_path / "pof.tsv").read_bytes() == (tmp_path / "po.tsv").read_bytes()
    want_pe = [pe[0] + header] + [ln + col for ln, col in zip(pe[1:], columns(prows))]
    assert (tmp_path / "pef.tsv").read_text().splitlines() == want_pe
    r = run(*pbase, "-E", tmp_path / "pek.tsv", "-O", tmp_path / "pok.tsv", *popts, "--knockout-filter", "0,100,0,nmd1+nmd2", "--knockout-out",
            tmp_path / "prows.tsv")
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "pek.tsv").read_text().splitlines() == [want_pe[0]] + [ln for ln, k in zip(want_pe[1:], pkeep) if k]
    assert (tmp_path / "pok.tsv").read_text().splitlines() == [po[0]] + [ln for ln, k in zip(po[1:], pkeep) if k]
    assert len((tmp_path / "prows.tsv").read_text().splitlines()) == pkeep.sum() + 1
    r = subprocess.run([os.path.join(BIN, "pattern_search")] + [str(x) for x in ("-i", tmp_path / "idx", "-q", pattern, "-M", "2", "-O", tmp_path / "x.tsv", "-R",
                                                                                  tmp_path / "g.fa", "--knockout", "--knockout-cds", tmp_path / "cds.bed")],
                       capture_output=True, text=True, timeout=120, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode == 1 and "give -E" in r.stderr
    cds.close()
    gen.close()
