"""Prime-editing extensions on the device (vsc_loci_prime, vsc_guides_prime, vsc_pattern_guides_prime and the two filters): bit
for bit what the definition gives when it is applied locus by locus in plain Python on strings (tests/prime_cases.py).  Integers,
so there is no tolerance: rows, pairs, coverage and counts are compared as they are, the undefined row included."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import efficiency_cases as ec
import prime_cases as pc
import varscot_amd as va
import wide_cases as wc
from helpers import random_seq, revcomp
from varscot_amd import _lib

pytestmark = pytest.mark.gpu

TILE = 1024  # candidates per wave of the pairs' and the filter's passes (include/varscot_hip.h)
DROP_FRONT, DROP_BACK = 3, 1  # words the partial object of the small genome does not hold
COUNTS = pc.CLASSES + ("with_pair", "weak", "pairs", "edits_covered", "pairs_by_flag")
NAMES = sorted(pc.SHAPES)
SETS = ["none", "empty", "snv", "indel", "cells"]


@pytest.fixture(scope="module")
def ctx():
    c = va.Context(0)
    yield c
    c.close()


def counts(stats):
    return {k: stats[k] for k in COUNTS}


def loci_tuples(loci):
    return [(int(c), int(p), int(s)) for c, p, s in zip(loci["contig"], loci["pos"], loci["strand"])]


class Guides:
    """A vsc_guides (or, pattern=True, a vsc_pattern_guides) handle and its calls."""

    def __init__(self, ctx, handle, pattern=False):
        self.ctx, self.h, self.pattern = ctx, handle, pattern
        L = va.lib()
        kind = "vsc_pattern_guides" if pattern else "vsc_guides"
        self.fn = {k: getattr(L, "%s_%s" % (kind, k)) for k in ("count", "data", "free", "prime", "filter_prime", "filter_edit")}

    @classmethod
    def from_arrays(cls, ctx, codes, loci, on_device=True, pattern=False):
        h = C.c_void_p()
        make = va.lib().vsc_debug_pattern_guides_from_host if pattern else va.lib().vsc_debug_guides_from_host
        _lib.check(make(ctx._h if on_device else None, _lib.ptr(codes), _lib.ptr(loci), len(codes), C.byref(h)), ctx._h)
        return cls(ctx, h, pattern)

    def __len__(self):
        return int(self.fn["count"](self.h))

    def arrays(self):
        pc_, pl = C.c_void_p(), C.c_void_p()
        _lib.check(self.fn["data"](self.h, C.byref(pc_), C.byref(pl)), self.ctx._h)
        n = len(self)
        if n == 0:
            return np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=va.LOCUS_DTYPE)
        return (np.frombuffer((C.c_char * (n * 8)).from_address(pc_.value), dtype=np.uint64).copy(),
                np.frombuffer((C.c_char * (n * 16)).from_address(pl.value), dtype=va.LOCUS_DTYPE).copy())

    def prime(self, gen, shape, edits, capacity):
        """(rows, pairs in the library's edit numbering, coverage over the sorted edits, stats, status)."""
        n = len(self)
        e = va.prime_edits(edits)[0] if edits is not None else None
        n_e = 0 if e is None else len(e)
        rows, pairs = np.empty((n, 2), dtype=np.uint32), np.zeros(capacity, dtype=va.PRIME_PAIR_DTYPE)
        cov = np.empty((n_e, 2), dtype=np.uint32)
        st, count, sh = _lib.PrimeStats(), C.c_uint64(), shape._struct()
        rc = self.fn["prime"](self.ctx._h, gen._h, self.h, C.byref(sh), _lib.ptr(e) if n_e else None, n_e, _lib.ptr(rows), _lib.ptr(pairs),
                              capacity, C.byref(count), _lib.ptr(cov), C.byref(st))
        return rows, pairs[:min(capacity, int(count.value))], cov, st.as_dict(), rc

    def filter_code(self, gen, shape, edits, allow_weak):
        out = C.c_void_p()
        sh = shape._struct()
        e = va.prime_edits(edits)[0] if edits is not None else None
        n_e = 0 if e is None else len(e)
        return self.fn["filter_prime"](self.ctx._h, gen._h, self.h, C.byref(sh), _lib.ptr(e) if n_e else None, n_e, int(allow_weak),
                                       C.byref(out)), out

    def filter(self, gen, shape, edits, allow_weak):
        code, out = self.filter_code(gen, shape, edits, allow_weak)
        _lib.check(code, self.ctx._h)
        return Guides(self.ctx, out, self.pattern)

    def filter_edit(self, gen, shape, targets, lo, hi):
        out = C.c_void_p()
        sh = shape._struct()
        tg = va.edit_targets(targets)[0]
        _lib.check(self.fn["filter_edit"](self.ctx._h, gen._h, self.h, C.byref(sh), _lib.ptr(tg), len(tg), lo, hi, C.byref(out)), self.ctx._h)
        return Guides(self.ctx, out, self.pattern)

    def close(self):
        if self.h:
            self.fn["free"](self.h)
            self.h = None


def sorted_numbering(want, edits):
    """An expected result with the edits numbered as the LIBRARY numbers them (the place among the sorted edits): (pairs, coverage)."""
    _, order, inverse = va.prime_edits(edits)
    pairs = want["pairs"].copy()
    pairs["edit"] = inverse[pairs["edit"].astype(np.int64)].astype(np.uint32)
    pairs = pairs[np.lexsort((pairs["edit"], pairs["candidate"]))]
    return pairs, want["coverage"][order]


# ---- 1. every locus of the small genome ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(ctx):
    """Per shape: its small genome resident - whole, and as an object that lacks its first three words and its last one - every
    locus of it with the invalid ones behind, and per edit set the expected result, computed once."""
    cache = {}

    def get(name):
        if name not in cache:
            shape = pc.shape_of(name)
            contigs = pc.small_genome(shape.site_len, shape.context_len)
            packed = va.PackedGenome.from_sequences(list(contigs))
            loci = pc.every_locus(contigs) + pc.invalid_loci(contigs)
            sl = slice(DROP_FRONT, packed.n_words - DROP_BACK)
            part = va.Genome.from_shard(ctx, packed.hi[sl], packed.lo[sl], packed.nmask[sl], DROP_FRONT, sl.stop - sl.start, packed.contigs)
            cache[name] = {"shape": shape, "contigs": contigs, "packed": packed, "gen": ctx.load_genome(packed), "part": part, "loci": loci,
                           "arr": pc.locus_array(loci), "resident": (32 * sl.start, 32 * sl.stop), "sets": pc.edit_sets(contigs), "want": {}}
        return cache[name]

    def want(name, which, partial=False):
        s = get(name)
        key = (which, partial)
        if key not in s["want"]:
            s["want"][key] = pc.expected(s["contigs"], s["loci"], s["shape"], s["sets"][which], s["resident"] if partial else None)
        return s["want"][key]

    get.want = want
    yield get
    for s in cache.values():
        s["gen"].close()
        s["part"].close()


def same(got, want, edits):
    rows, pairs, coverage, stats = got
    assert rows.dtype == np.uint32 and rows.tobytes() == want["rows"].tobytes()
    assert counts(stats) == want["stats"] and sum(stats[k] for k in pc.CLASSES) == len(rows)
    if edits is None:
        assert pairs is None and coverage is None and stats["pairs"] == 0
    else:
        assert pairs.dtype == va.PRIME_PAIR_DTYPE and pairs.tobytes() == want["pairs"].tobytes()
        assert coverage.tobytes() == want["coverage"].tobytes()


@pytest.mark.parametrize("which", SETS)
@pytest.mark.parametrize("name", NAMES)
def test_every_locus_of_a_small_genome(small, name, which):
    s = small(name)
    edits, sh = s["sets"][which], s["shape"]
    same(s["part"].prime(s["arr"], sh, edits, coverage=True, allow_partial=True), small.want(name, which, partial=True), edits)
    same(s["gen"].prime(s["arr"], sh, edits, coverage=True), small.want(name, which), edits)


def test_the_partial_object_is_partial(small):
    a = small.want("pe2", "indel", partial=True)["stats"]
    assert all(a[k] >= 5 for k in pc.CLASSES) and a["pairs"] > 300


@pytest.mark.parametrize("name", ["short", "long"])
def test_the_pattern_handle_at_other_site_lengths(ctx, small, name):
    """site_len 16 and 32 through the pattern handle, where the caller vouches for the length; vsc_guides holds 23-mers."""
    s = small(name)
    sh, edits = s["shape"], s["sets"]["indel"]
    g = Guides.from_arrays(ctx, np.arange(len(s["arr"]), dtype=np.uint64), s["arr"], pattern=True)
    for gen, want in ((s["part"], small.want(name, "indel", partial=True)), (s["gen"], small.want(name, "indel"))):
        rows, pairs, cov, stats, rc = g.prime(gen, sh, edits, want["stats"]["pairs"] + 5)
        want_pairs, want_cov = sorted_numbering(want, edits)
        assert rc == 0 and rows.tobytes() == want["rows"].tobytes() and counts(stats) == want["stats"]
        assert pairs.tobytes() == want_pairs.tobytes() and cov.tobytes() == want_cov.tobytes()
    g.close()
    plain = Guides.from_arrays(ctx, np.arange(len(s["arr"]), dtype=np.uint64), s["arr"])
    assert plain.prime(s["gen"], sh, edits, 0)[4] == -22 and "site_len" in va.lib().vsc_last_error(ctx._h).decode()
    plain.close()


# ---- 2. beyond one launch ----------------------------------------------------------------------------------------------------
def launch_waves():
    """The waves of a launch capped as the cells' grids are (wide_cases): CUs x 8 workgroups of 4 waves."""
    return torch.cuda.get_device_properties(0).multi_processor_count * wc.GROUPS_PER_CU * wc.WAVES_PER_GROUP


def test_more_candidates_than_a_launch_has_lanes_and_more_tiles_than_waves(ctx, small):
    name, which = "model", "snv"  # several pairs per candidate: runs of them cross tile boundaries; WEAK and not
    s = small(name)
    sh, edits, base = s["shape"], s["sets"][which], small.want(name, which)
    m = len(s["loci"])
    n = (launch_waves() + 3) * TILE + 17
    assert n > 3 * m and n > launch_waves() * 64
    idx = np.arange(n) % m
    loci = s["arr"][idx]
    rows, pairs, coverage, stats = s["gen"].prime(loci, sh, edits, coverage=True)
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
    last = np.bincount(bp[bp["candidate"] < rem]["edit"], minlength=len(edits))
    assert (coverage[:, 0] == reps * base["coverage"][:, 0] + last).all()
    assert reps >= 1 and (coverage[:, 1] == base["coverage"][:, 1]).all()  # (every base pair occurs at least once)
    assert sum(stats[k] for k in pc.CLASSES) == n
    flags = want_pairs["info"] >> 24
    assert stats["pairs_by_flag"] == [int((flags >> b & 1).sum()) for b in range(4)] and all(stats["pairs_by_flag"])
    # the filter over the same tiles: the survivors in input order
    keep = np.array([pc.keep(r, True, False) for r in base["rows"]])
    assert 0 < keep.sum() < len(keep)
    codes = np.arange(n, dtype=np.uint64) * np.uint64(3)
    g = Guides.from_arrays(ctx, codes, loci, pattern=True)
    out = g.filter(s["gen"], sh, edits, False)
    got_codes, got_loci = out.arrays()
    chosen = np.nonzero(keep[idx])[0]
    assert got_codes.tobytes() == codes[chosen].tobytes() and got_loci.tobytes() == loci[chosen].tobytes()
    out.close()
    g.close()


# ---- 3. the bitmap changes no bit ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pe2", "first"])
def test_the_bitmap_on_against_off(ctx, small, name):
    s = small(name)
    L = va.lib()
    got = {}
    try:
        for on in (1, 0, 1):
            assert L.vsc_debug_prime_bitmap(ctx._h, on) == 0
            for which in ("cells", "indel", "snv"):
                rows, pairs, cov, stats = s["gen"].prime(s["arr"], s["shape"], s["sets"][which], coverage=True)
                mine = (rows.tobytes(), pairs.tobytes(), cov.tobytes(), counts(stats))
                assert got.setdefault(which, mine) == mine, (on, which)
                same((rows, pairs, cov, stats), small.want(name, which), s["sets"][which])
            g = Guides.from_arrays(ctx, np.arange(len(s["arr"]), dtype=np.uint64), s["arr"], pattern=True)
            out = g.filter(s["gen"], s["shape"], s["sets"]["cells"], True)
            kept = out.arrays()[0].tobytes()
            assert got.setdefault("filter", kept) == kept
            out.close()
            g.close()
    finally:
        L.vsc_debug_prime_bitmap(ctx._h, 1)
    keep = np.array([pc.keep(r, True, True) for r in small.want(name, "cells")["rows"]])
    assert 0 < keep.sum() < len(keep) and got["filter"] == np.nonzero(keep)[0].astype(np.uint64).tobytes()
    assert L.vsc_debug_prime_bitmap(None, 1) == -22
    # the edits of this set lie on both sides of several cell edges; most candidates reach no edit at all
    cells = {g // pc.CELL for c, p, _, _ in s["sets"]["cells"] for g in [pc.offsets(s["contigs"])[c] + p]}
    assert len(cells) >= 3 and 0 < small.want(name, "cells")["stats"]["with_pair"] < small.want(name, "cells")["stats"]["defined"] // 2


def test_the_launch_width_changes_no_bit(ctx, small):
    """The rows kernel is grid-stride: whatever the cap of its grid (vsc_debug_prime_groups_per_cu), the same bytes - with
    more candidates than a grid of one workgroup per CU has lanes, so that the cap binds and lanes take several steps."""
    s = small("model")
    L = va.lib()
    m = len(s["loci"])
    n = torch.cuda.get_device_properties(0).multi_processor_count * 256 * 2 + 77
    idx = np.arange(n) % m
    loci = s["arr"][idx]
    got = None
    try:
        for groups in (0, 1, 7, 8, 64):
            assert L.vsc_debug_prime_groups_per_cu(ctx._h, groups) == 0
            rows, pairs, cov, stats = s["gen"].prime(loci, s["shape"], s["sets"]["indel"], coverage=True)
            mine = (rows.tobytes(), pairs.tobytes(), cov.tobytes(), counts(stats))
            if got is None:
                got = mine
                assert rows.tobytes() == small.want("model", "indel")["rows"][idx].tobytes() and stats["pairs"] > n // 10
            assert mine == got, groups
        assert L.vsc_debug_prime_groups_per_cu(ctx._h, 65) == -22 and L.vsc_debug_prime_groups_per_cu(None, 1) == -22
    finally:
        L.vsc_debug_prime_groups_per_cu(ctx._h, 0)


# ---- 4. the pair contract ----------------------------------------------------------------------------------------------------
def test_the_pair_contract(ctx, small):
    name, which = "pe2", "indel"
    s = small(name)
    sh, edits, want = s["shape"], s["sets"][which], small.want(name, which)
    want_pairs, want_cov = sorted_numbering(want, edits)
    total = len(want_pairs)
    e = va.prime_edits(edits)[0]
    L, st = va.lib(), sh._struct()
    n = len(s["arr"])

    def call(pairs, capacity, rows=True, cov=True):
        r = np.full((n, 2), 7, dtype=np.uint32) if rows else None
        c = np.full((len(e), 2), 7, dtype=np.uint32) if cov else None
        count, stats = C.c_uint64(12345), _lib.PrimeStats()
        rc = L.vsc_loci_prime(ctx._h, s["gen"]._h, _lib.ptr(s["arr"]), n, C.byref(st), _lib.ptr(e), len(e), _lib.ptr(r), _lib.ptr(pairs), capacity,
                              C.byref(count), _lib.ptr(c), C.byref(stats))
        return rc, r, c, int(count.value), stats.as_dict()

    rc, rows, cov, count, stats = call(None, 0)  # count only
    assert rc == 0 and count == total and rows.tobytes() == want["rows"].tobytes() and cov.tobytes() == want_cov.tobytes()
    assert counts(stats) == want["stats"]
    exact = np.zeros(total, dtype=va.PRIME_PAIR_DTYPE)
    rc, rows, cov, count, _ = call(exact, total)
    assert rc == 0 and count == total and exact.tobytes() == want_pairs.tobytes()
    short = np.full(total, 0x5A5A5A5A, dtype=np.uint32).repeat(4).view(va.PRIME_PAIR_DTYPE)[:total].copy()
    before = short.tobytes()
    rc, rows, cov, count, stats = call(short, total - 1)  # one short
    assert rc == -34 and "capacity" in L.vsc_last_error(ctx._h).decode()
    assert short.tobytes() == before  # nothing is written to pairs
    assert count == total and rows.tobytes() == want["rows"].tobytes() and cov.tobytes() == want_cov.tobytes() and counts(stats) == want["stats"]
    rc, _, _, count, stats = call(None, 0, rows=False, cov=False)  # every output but the count is optional
    assert rc == 0 and count == total and counts(stats) == want["stats"]  # (the covered edits are then counted on the device)
    assert L.vsc_loci_prime(ctx._h, s["gen"]._h, _lib.ptr(s["arr"]), n, C.byref(st), _lib.ptr(e), len(e), None, None, 0, None, None, None) == 0
    # the wrapper's second call, when its first capacity was too small
    many = s["arr"][np.arange(6 * n) % n]
    rows, pairs, _, stats = s["gen"].prime(many, sh, s["sets"]["snv"])
    assert len(pairs) == stats["pairs"] == 6 * small.want(name, "snv")["stats"]["pairs"] > max(6 * n, 1024)
    # nothing to do
    rows, pairs, coverage, stats = s["gen"].prime(pc.locus_array([]), sh, edits, coverage=True)
    assert rows.shape == (0, 2) and len(pairs) == 0 and (coverage[:, 0] == 0).all() and (coverage[:, 1] == pc.UNDEF).all()
    assert counts(stats) == dict.fromkeys(COUNTS[:-1], 0) | {"pairs_by_flag": [0, 0, 0, 0]}
    t = ctx.timing()
    assert t["sites"] == 0 and t["total_ms"] == 0


# ---- 5. candidates where they lie ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted(ctx):
    """A 20 kb random genome with NGG sites (and CCN sites, their '-' form) at and next to the contig ends, and edits over it:
    SNVs at every third position, and a few hundred insertions and deletions."""
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
    snv = [(c, p, 1, pc.other_letter(t[p])) for c, t in enumerate(contigs) for p in range(0, len(t), 3)]
    indel = []
    for c, t in enumerate(contigs):
        for k, p in enumerate(range(4, len(t) - 20, 37)):
            del_len, ins_len = ((0, 1), (0, 3), (0, 16), (1, 0), (3, 0), (16, 0), (3, 2))[k % 7]
            indel.append((c, p, del_len, random_seq(rng, ins_len) if ins_len else ""))
    order = rng.permutation(len(indel))
    yield {"contigs": contigs, "packed": packed, "gen": gen, "snv": snv, "indel": [indel[i] for i in order]}
    gen.close()


def test_enumerated_guides_where_they_lie(ctx, planted):
    gen, contigs = planted["gen"], planted["contigs"]
    pe2 = va.PRIME_EDITORS["PE2"]
    plain = gen.enumerate_guides()
    codes, loci, rows = gen.enumerate_guides(prime="PE2")
    assert codes.tobytes() == plain[0].tobytes() and loci.tobytes() == plain[1].tobytes() and len(codes) > 1000
    tuples = loci_tuples(loci)
    want = pc.expected(contigs, tuples, pe2, planted["snv"])
    assert rows.dtype == np.uint32 and rows[:, 0].tobytes() == want["rows"][:, 0].tobytes() and np.isin(rows[:, 1], (0, pc.UNDEF)).all()
    assert want["stats"]["off_contig"] >= 6 and want["stats"]["pairs"] > 5000  # the sites at the contig ends have no context
    same(gen.prime((codes, loci), pe2, planted["snv"], coverage=True), want, planted["snv"])
    # an SNV on the first G of an NGG candidate's PAM: the PAM flag, nothing in the seed
    flags = want["pairs"]["info"] >> 24
    d = (want["pairs"]["info"] >> 8) & 255
    assert ((flags & pc.PAM != 0) == ((d == 4) | (d == 5))).all() and ((flags & pc.SEED != 0) == (d <= 2)).all()
    # over the handle: what vsc_loci_prime gives for the same loci
    want = pc.expected(contigs, tuples, pe2, planted["indel"])
    g = Guides.from_arrays(ctx, plain[0], plain[1])
    rows, pairs, cov, stats, rc = g.prime(gen, pe2, planted["indel"], want["stats"]["pairs"])
    want_pairs, want_cov = sorted_numbering(want, planted["indel"])
    assert rc == 0 and rows.tobytes() == want["rows"].tobytes() and pairs.tobytes() == want_pairs.tobytes() and cov.tobytes() == want_cov.tobytes()
    assert counts(stats) == want["stats"] and want["stats"]["pairs"] > 300
    host = Guides.from_arrays(ctx, plain[0], plain[1], on_device=False)  # the host-only object goes the vsc_loci_prime way
    h_rows, h_pairs, h_cov, h_stats, rc = host.prime(gen, pe2, planted["indel"], want["stats"]["pairs"])
    assert rc == 0 and h_rows.tobytes() == rows.tobytes() and h_pairs.tobytes() == pairs.tobytes() and h_cov.tobytes() == cov.tobytes()
    assert counts(h_stats) == counts(stats)
    host.close()
    g.close()
    # N x 21 + GG under the pattern enumeration: the same sites, the same rows
    found, prows = gen.enumerate_pattern("N" * 21 + "GG", (0, 20), prime=pe2)
    assert found.loci.tobytes() == plain[1].tobytes() and prows[:, 0].tobytes() == want["rows"][:, 0].tobytes()
    with pytest.raises(ValueError):
        gen.enumerate_guides(prime=va.PrimeShape(site_len=27, down=37, pam=(25, 2)))
    with pytest.raises(ValueError):
        gen.enumerate_guides(prime_allow_weak=False)
    with pytest.raises(ValueError):
        gen.enumerate_guides(prime_edits=[(0, 5, 1, "A")])


OTHERS = {"SaCas9": ("N" * 21 + "NNGRRT", (0, 21), dict(site_len=27, down=30, nick=18, pbs=(9, 14), rtt=(8, 30), min_homology=4, pam=(23, 3),
                                                         seed=(18, 3), avoid_g_end=True, stability=pc.GC_MODEL)),
          "Cas12a": ("TTTV" + "N" * 23, (4, 23), dict(site_len=27, down=20, nick=22, pbs=(10, 12), rtt=(6, 25), min_homology=3, pam=(0, 4),
                                                       seed=(4, 6), avoid_g_end=False))}


@pytest.mark.parametrize("which", sorted(OTHERS))
def test_pattern_candidates_of_other_nucleases(planted, which):
    gen, contigs = planted["gen"], planted["contigs"]
    pattern, proto, kw = OTHERS[which]
    sh = va.PrimeShape(**kw)
    edits = planted["indel"] + [e for e in planted["snv"] if e[1] % 2 and (e[0], e[1]) not in {(c, p) for c, p, _, _ in planted["indel"]}]
    plain = gen.enumerate_pattern(pattern, proto)
    found, rows = gen.enumerate_pattern(pattern, proto, prime=sh)
    assert found.codes.tobytes() == plain.codes.tobytes() and found.loci.tobytes() == plain.loci.tobytes() and len(found) > 100
    want = pc.expected(contigs, loci_tuples(found.loci), sh, edits)
    assert want["stats"]["defined"] > 100 and want["stats"]["pairs"] > 100
    assert rows[:, 0].tobytes() == want["rows"][:, 0].tobytes()
    same(gen.prime(found, sh, edits, coverage=True), want, edits)
    # the filter through the wrapper: the survivors in input order, their rows; only the survivors are searched
    few = edits[:40]
    want_few = pc.expected(contigs, loci_tuples(found.loci), sh, few)
    keep = np.array([pc.keep(r, True, which != "SaCas9") for r in want_few["rows"]])
    assert 0 < keep.sum() < len(keep)
    kept, krows = gen.enumerate_pattern(pattern, proto, prime=sh, prime_edits=few, prime_allow_weak=which != "SaCas9")
    assert kept.codes.tobytes() == found.codes[keep].tobytes() and kept.loci.tobytes() == found.loci[keep].tobytes()
    assert krows.tobytes() == want_few["rows"][keep].tobytes()
    d_found, d_rows, d_prime = gen.design_pattern(pattern, proto, 2, prime=sh, prime_edits=few, prime_allow_weak=which != "SaCas9")
    assert d_found.codes.tobytes() == kept.codes.tobytes() and d_prime.tobytes() == krows.tobytes()
    _, all_rows = gen.design_pattern(pattern, proto, 2)
    assert d_rows.tobytes() == all_rows[keep].tobytes()


# ---- 6. the filter ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["none", "indel"])
def test_filter_rule_and_input_order(ctx, small, which):
    name = "model"
    s = small(name)
    sh, edits, want = s["shape"], s["sets"][which], small.want(name, which)
    n = len(s["loci"])
    codes = np.arange(n, dtype=np.uint64) * np.uint64(5)
    g = Guides.from_arrays(ctx, codes, s["arr"])
    kept = {}
    for allow in (True, False):
        keep = np.array([pc.keep(r, edits is not None, allow) for r in want["rows"]])
        out = g.filter(s["gen"], sh, edits, allow)
        got_codes, got_loci = out.arrays()
        out.close()
        assert got_codes.tobytes() == codes[keep].tobytes() and got_loci.tobytes() == s["arr"][keep].tobytes(), allow
        kept[allow] = int(keep.sum())
    assert kept[True] == (want["stats"]["defined"] if edits is None else want["stats"]["with_pair"]) and 0 < kept[False] < kept[True]
    t = ctx.timing()
    assert t["sites"] == n and t["score_ms"] == t["total_ms"] > 0
    assert t["genome_bytes"] == 32 * n + 48 * kept[False]  # (the last call's)
    host = Guides.from_arrays(ctx, codes, s["arr"], on_device=False)  # the host-only object: uploaded first, the same bytes
    keep = np.array([pc.keep(r, edits is not None, False) for r in want["rows"]])
    h_out = host.filter(s["gen"], sh, edits, False)
    assert h_out.arrays()[0].tobytes() == codes[keep].tobytes()
    again = h_out.filter(s["gen"], sh, edits, False)  # the survivors survive
    assert again.arrays()[0].tobytes() == codes[keep].tobytes()
    empty = again.filter(s["gen"], sh, [(0, 0, 1, "A")], True)  # an edit nobody reaches: an empty result is a result
    assert len(empty) == 0 and len(empty.filter(s["gen"], sh, edits, True).arrays()[0]) == 0
    for h in (empty, again, h_out, host, g):
        h.close()


def test_what_takes_the_filters_result_and_the_edit_filter_in_both_orders(ctx, planted):
    gen, contigs = planted["gen"], planted["contigs"]
    pe2, edits = va.PRIME_EDITORS["PE2"], planted["indel"]
    pcodes, ploci = gen.enumerate_guides()
    want = pc.expected(contigs, loci_tuples(ploci), pe2, edits)
    keep = np.array([pc.keep(r, True, True) for r in want["rows"]])
    assert 0 < keep.sum() < want["stats"]["defined"]
    k_codes, k_loci, k_rows = gen.enumerate_guides(prime="PE2", prime_edits=edits)
    assert k_codes.tobytes() == pcodes[keep].tobytes() and k_loci.tobytes() == ploci[keep].tobytes()
    assert k_rows.tobytes() == want["rows"][keep].tobytes()
    rows_all = gen.summarize(pcodes, 2, exclude=ploci)
    d = gen.design(None, 2, prime=pe2, prime_edits=edits)
    assert len(d) == 4 and d[0].tobytes() == k_codes.tobytes() and d[2].tobytes() == rows_all[keep].tobytes() and d[3].tobytes() == k_rows.tobytes()
    # with the base-editor filter, in both orders the same survivors; through the wrapper the prime rows come last
    cbe = va.EDITORS["CBE"]
    targets = [(c, p) for c, t in enumerate(contigs) for p in range(0, len(t), 3)]
    g = Guides.from_arrays(ctx, pcodes, ploci)
    a = g.filter_edit(gen, cbe, targets, 1, 3)
    a2 = a.filter(gen, pe2, edits, True)
    b = g.filter(gen, pe2, edits, True)
    b2 = b.filter_edit(gen, cbe, targets, 1, 3)
    assert 0 < len(a2) < min(len(a), len(b))
    for x, y in zip(a2.arrays(), b2.arrays()):
        assert x.tobytes() == y.tobytes()
    model = ec.build("dense", (6, 23, 6))
    k = gen.enumerate_guides(efficiency=model, edit=cbe, edit_targets=targets, min_editable=1, max_editable=3, prime=pe2, prime_edits=edits)
    assert len(k) == 5 and k[0].tobytes() == a2.arrays()[0].tobytes() and k[1].tobytes() == a2.arrays()[1].tobytes()
    survivors = set(loci_tuples(k[1]))
    assert k[2].dtype == np.float64 and k[4].tobytes() == want["rows"][[t in survivors for t in loci_tuples(ploci)]].tobytes()
    for h in (a, a2, b, b2, g):
        h.close()


# ---- 7. end to end ------------------------------------------------------------------------------------------------------------
def test_the_best_pegrnas_of_every_edit(planted):
    gen, contigs, packed = planted["gen"], planted["contigs"], planted["packed"]
    pe2 = va.PRIME_EDITORS["PE2"]
    rng = np.random.default_rng(6)
    edits = [planted["snv"][i] for i in rng.choice(len(planted["snv"]), size=1500, replace=False)]
    codes, loci = gen.enumerate_guides()
    rows, pairs, _, stats = gen.prime((codes, loci), pe2, edits)
    want = pc.expected(contigs, loci_tuples(loci), pe2, edits)
    assert pairs.tobytes() == want["pairs"].tobytes() and len(pairs) > 1000
    spec = (np.arange(len(codes), dtype=np.uint64) * np.uint64(2654435761)) % np.uint64(10007)  # a stand-in for a specificity column
    p_loci, p_edit, key = va.prime_pick_inputs(pairs, loci, extra_columns=[(spec, 14)])
    pick = va.PickShape(3, spacing=2)
    picks, cnt, st = gen.pick(p_loci, key, pick, target=p_edit, n_targets=len(edits))
    # the restatement, followed by the host's pick
    detail = want["detail"]
    want_key = np.array([((g["flags"] & 3 != 0) << 9 | (g["flags"] & 4 == 0) << 8 | (255 - g["t"])) << 14 for g in detail], dtype=np.uint64)
    want_key |= np.minimum(spec[want["pairs"]["candidate"]], np.uint64(16383))
    assert key.tobytes() == want_key.tobytes()
    h_picks, h_cnt, _ = va.pick_host(packed.contigs, loci[want["pairs"]["candidate"]], want["pairs"]["edit"], want_key, len(edits), pick)
    assert picks.tobytes() == h_picks.tobytes() and cnt.tobytes() == h_cnt.tobytes() and cnt.max() >= 2 and (cnt == 0).any()
    first = picks[cnt > 0, 0]
    best = [want_key[want["pairs"]["edit"] == e].max() for e in np.nonzero(cnt > 0)[0]]
    assert (want_key[first] == best).all()  # the best key of every edit comes first


def test_the_extension_of_every_pair(planted, small):
    gen, contigs, packed = planted["gen"], planted["contigs"], planted["packed"]
    pe2, edits = va.PRIME_EDITORS["PE2"], planted["indel"]
    codes, loci = gen.enumerate_guides()
    tuples = loci_tuples(loci)
    _, pairs, _, _ = gen.prime((codes, loci), pe2, edits)
    want = pc.expected(contigs, tuples, pe2, edits)
    assert pairs.tobytes() == want["pairs"].tobytes() and len(pairs) > 300
    strands = set()
    for q, text in zip(pairs, want["extension"]):
        locus = tuples[int(q["candidate"])]
        strands.add(locus[2])
        assert va.prime_extension(packed, pe2, locus, edits[int(q["edit"])]) == text
        assert len(text) == int(va.unpack_prime_ext(q["ext"])[0])
    assert strands == {0, 1}
    s = small("model")  # every locus, a stability model
    w = small.want("model", "indel")
    for q, text in list(zip(w["pairs"], w["extension"]))[::7]:
        assert va.prime_extension(s["packed"], s["shape"], s["loci"][int(q["candidate"])], s["sets"]["indel"][int(q["edit"])]) == text
    no_pair = next(i for i, r in enumerate(want["rows"]) if int(r[1]) == 0 and int(r[0]) != pc.UNDEF)
    assert va.prime_extension(packed, pe2, tuples[no_pair], edits[0], strict=False) == ""
    with pytest.raises(ValueError):
        va.prime_extension(packed, pe2, tuples[no_pair], edits[0])


def test_a_shard_answers_for_what_it_holds(ctx, planted):
    packed, contigs, pe2 = planted["packed"], planted["contigs"], va.PRIME_EDITORS["PE2"]
    n_words = packed.n_words
    loci = [(0, p, s) for p in list(range(2000, 2100)) + list(range(2200, 2280)) for s in (0, 1)]
    loci += loci_tuples(planted["gen"].enumerate_guides()[1])
    arr = pc.locus_array(loci)
    for first, words, own in ((64, n_words - 64, n_words - 64), (0, 70, 64)):  # nothing in front of word 64; nothing behind a 6-word halo
        sl = slice(first, first + words)
        shard = va.Genome.from_shard(ctx, packed.hi[sl], packed.lo[sl], packed.nmask[sl], first, own, packed.contigs)
        want = pc.expected(contigs, loci, pe2, planted["snv"], resident=(32 * first, 32 * (first + words)))
        assert want["stats"]["not_resident"] > 100 and want["stats"]["defined"] > 100 and want["stats"]["pairs"] > 100
        with pytest.raises(ValueError) as e:
            shard.prime(arr, pe2, planted["snv"])
        assert "not resident" in str(e.value)
        same(shard.prime(arr, pe2, planted["snv"], coverage=True, allow_partial=True), want, planted["snv"])
        shard.close()


def test_alternating_shapes_scratch_and_timing(ctx, small):
    combos = [("pe2", "indel"), ("model", "snv"), ("first", "none"), ("deep", "cells"), ("pe2", "empty")]

    def run(k):
        name, which = combos[k]
        s = small(name)
        got = s["gen"].prime(s["arr"], s["shape"], s["sets"][which], coverage=True)
        same(got, small.want(name, which), s["sets"][which])
        return got, s

    for k in (0, 0, 1, 0, 2, 3, 4, 1, 2):  # nothing of a call outlives it
        run(k)
    ctx.release_scratch()
    run(1)
    ctx.release_scratch()
    got, s = run(0)
    stats, n = got[3], len(s["loci"])
    assert stats["score_ms"] > 0 and stats["wall_ms"] >= stats["score_ms"]
    assert stats["edit_order"].tolist() == va.prime_edits(s["sets"]["indel"])[1].tolist()
    t = ctx.timing()
    assert t["score_ms"] > 0 and t["scan_ms"] > 0 and t["total_ms"] == t["score_ms"] + t["scan_ms"] and t["sites"] == n
    assert t["genome_bytes"] == 24 * n
    run(2)
    t = ctx.timing()
    assert t["scan_ms"] == 0 and t["total_ms"] == t["score_ms"] > 0  # without edits: the rows kernel alone


def test_every_refusal(ctx, planted):
    L = va.lib()
    gen, contigs = planted["gen"], planted["contigs"]
    g = Guides.from_arrays(ctx, *gen.enumerate_guides())
    n = len(g)
    rows = np.full((n, 2), 9, dtype=np.uint32)
    ok = va.PRIME_EDITORS["PE2"]._struct()
    count = C.c_uint64()

    def guides_prime(shape, edits=None, n_e=0, handle=g.h, genome=gen._h, context=None):
        return L.vsc_guides_prime((context or ctx)._h, genome, handle, shape, _lib.ptr(edits), n_e, _lib.ptr(rows), None, 0, C.byref(count), None, None)

    good = dict(site_len=23, down=41, nick=17, pbs=(13, 13), rtt=(10, 34), min_homology=5, pam=(21, 2), seed=(17, 3), avoid_g_end=True)
    for kw in ({"site_len": 15}, {"site_len": 33}, {"down": 42}, {"nick": 0}, {"nick": 24}, {"pbs": (0, 13)}, {"pbs": (14, 13)}, {"pbs": (13, 18)},
               {"rtt": (0, 34)}, {"rtt": (35, 34)}, {"rtt": (10, 48)}, {"min_homology": 35}, {"pam": (21, 3)}, {"pam": (10, 9)}, {"seed": (16, 8)},
               {"avoid_g_end": 2}, {"stability": (0, (0, 0, 2 ** 20 + 1, 0), (0,) * 16, 0)}, {"nick": 0xFFFFFFFF}, {"down": 0xFFFFFFFF}):
        sh = va.PrimeShape(validate=False, **dict(good, **kw))
        st = sh._struct()
        assert guides_prime(C.byref(st)) == -22, kw
        code, out = g.filter_code(gen, sh, None, True)
        assert code == -22 and not out.value
    with pytest.raises(va.VarscotError):
        gen.prime(pc.locus_array([(0, 100, 0)]), va.PrimeShape(validate=False, **dict(good, nick=24)))
    reserved = va.PRIME_EDITORS["PE2"]._struct()
    reserved.reserved[2] = 1
    assert guides_prime(C.byref(reserved)) == -22 and "reserved" in L.vsc_last_error(ctx._h).decode()
    sh27 = va.PrimeShape(site_len=27, down=37, pam=(25, 2))  # vsc_guides holds 23-mers
    st27 = sh27._struct()
    assert guides_prime(C.byref(st27)) == -22 and "site_len" in L.vsc_last_error(ctx._h).decode()
    assert g.filter_code(gen, sh27, None, True)[0] == -22
    assert guides_prime(None) == -22 and guides_prime(C.byref(ok), genome=None) == -22 and guides_prime(C.byref(ok), handle=None) == -22  # null arguments
    assert L.vsc_guides_filter_prime(ctx._h, gen._h, g.h, C.byref(ok), None, 0, 1, None) == -22
    assert guides_prime(C.byref(ok), None, 3) == -22 and "null" in L.vsc_last_error(ctx._h).decode()  # n_e > 0 with NULL edits

    def edits_of(rows_):
        e = np.zeros(len(rows_), dtype=va.PRIME_EDIT_DTYPE)
        for k, r in enumerate(rows_):
            e[k] = r
        return e

    end = len(contigs[0])
    for bad, word in (([(0, 5, 1, 1, 0), (0, 5, 0, 1, 1)], "ascending"), ([(0, 6, 1, 1, 0), (0, 5, 1, 1, 0)], "ascending"),
                      ([(1, 0, 1, 1, 0), (0, 5, 1, 1, 0)], "ascending"), ([(len(contigs), 0, 1, 1, 0)], "unknown"), ([(0xFFFFFFFF, 0, 1, 0, 0)], "unknown"),
                      ([(0, end, 1, 0, 0)], "beyond"), ([(0, end - 2, 3, 0, 0)], "beyond"), ([(0, end + 1, 0, 1, 0)], "beyond"), ([(0, 0xFFFFFFFF, 1, 0, 0)], "beyond"),
                      ([(0, 5, 17, 0, 0)], "above 16"), ([(0, 5, 0, 17, 0)], "above 16"), ([(0, 5, 0xFFFF, 0, 0)], "above 16"), ([(0, 5, 0, 0, 0)], "both 0"),
                      ([(0, 5, 0, 1, 4)], "bits"), ([(0, 5, 1, 0, 1)], "bits"), ([(0, 5, 0, 15, 1 << 30)], "bits")):
        e = edits_of(bad)
        assert guides_prime(C.byref(ok), e, len(e)) == -22 and word in L.vsc_last_error(ctx._h).decode(), bad
        out = C.c_void_p()
        assert L.vsc_guides_filter_prime(ctx._h, gen._h, g.h, C.byref(ok), _lib.ptr(e), len(e), 1, C.byref(out)) == -22 and not out.value
    assert (rows == 9).all()  # checked before anything is written
    last = edits_of([(0, end - 16, 16, 16, 0xFFFFFFFF), (0, end, 0, 1, 3), (2, len(contigs[2]) - 1, 1, 0, 0)])  # at and up to a contig's end
    assert guides_prime(C.byref(ok), last, 3) == 0
    assert L.vsc_loci_prime(ctx._h, gen._h, None, 1, C.byref(ok), None, 0, _lib.ptr(rows), None, 0, None, None, None) == -22
    assert L.vsc_loci_prime(ctx._h, gen._h, _lib.ptr(rows), 0xFFFFFFFF, C.byref(ok), None, 0, None, None, 0, None, None, None) == -34  # n
    assert L.vsc_loci_prime(ctx._h, gen._h, _lib.ptr(rows), 1, C.byref(ok), _lib.ptr(last), 0xFFFFFFFF, None, None, 0, None, None, None) == -34  # n_e
    other = va.Context(0)  # a genome or an object of another context is refused
    assert guides_prime(C.byref(ok), context=other) == -22
    o_gen = other.load_genome(planted["packed"])
    assert guides_prime(C.byref(ok), genome=o_gen._h, context=other) == -22 and "another context" in L.vsc_last_error(other._h).decode()
    o_gen.close()
    other.close()
    g.close()


# ---- 8. the tools end to end ---------------------------------------------------------------------------------------------------
def test_both_tools_on_the_small_genome(ctx, tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    bin_dir = os.path.join(root, "varscot_amd", "bin")
    pe2 = va.PRIME_EDITORS["PE2"]
    contigs = list(pc.small_genome(23, 64))
    names = ["chr%d of the small genome" % (k + 1) for k in range(len(contigs))]
    chrom = [n.split()[0] for n in names]
    with open(tmp_path / "g.fa", "w") as f:
        for n, t in zip(names, contigs):
            f.write(">%s\n%s\n" % (n, "\n".join(t[i:i + 60] for i in range(0, len(t), 60))))
    iv = [(c, 0, len(t)) for c, t in enumerate(contigs)]
    (tmp_path / "t.bed").write_text("".join("%s\t%d\t%d\n" % (chrom[c], a, b) for c, a, b in iv))
    edits = pc.edit_sets(contigs)["indel"]  # in the caller's order: the tool sorts them
    few = edits[:60]  # sparse: some candidates reach none of them

    def tsv(rows_):
        return "#chrom\tpos\tref\talt\n" + "".join("%s\t%d\t%d\t%s\n" % (chrom[c], p, d, (ins.lower() if p % 2 else ins) or "-") for c, p, d, ins in rows_)

    (tmp_path / "e.tsv").write_text(tsv(edits))
    (tmp_path / "few.tsv").write_text(tsv(few))
    run = lambda *a: subprocess.run([os.path.join(bin_dir, a[0])] + [str(x) for x in a[1:]], capture_output=True, text=True, timeout=600)  # noqa: E731
    assert run("bidir_index", "-G", tmp_path / "g.fa", "-I", tmp_path / "idx").returncode == 0
    packed = va.PackedGenome.from_sequences(contigs)
    gen = ctx.load_genome(packed)
    lines_of = lambda path: (tmp_path / path).read_text().splitlines()  # noqa: E731

    def columns(want):
        return ["\tNA\tNA\tNA" if int(r[0]) == pc.UNDEF else "\t%d\t%d\t%d" % (r[0] & 255, r[0] >> 8 & 255, r[1]) for r in want["rows"]]

    def pair_lines(want, ids, given):
        out = ["#chrom\tpos\tguideId\tpbsLen\trttLen\tnickToEdit\thomology\tflags\textension"]
        for q, g, text in zip(want["pairs"], want["detail"], want["extension"]):
            c, p, _, _ = given[int(q["edit"])]
            flags = "+".join(n for b, n in enumerate(va.PRIME_FLAGS) if g["flags"] >> b & 1) or "-"
            out.append("%s\t%d\t%s\t%d\t%d\t%d\t%d\t%s\t%s" % (chrom[c], p, ids[int(q["candidate"])], g["pbs_len"], g["t"], g["d"], g["h"], flags, text))
        return out

    def by_sorted_edit(want, given):
        """The pairs in the tool's order: ascending (guide, place of the edit among the sorted edits)."""
        _, _, inverse = va.prime_edits(given)
        order = np.lexsort((inverse[want["pairs"]["edit"].astype(np.int64)], want["pairs"]["candidate"]))
        return dict(want, pairs=want["pairs"][order], detail=[want["detail"][i] for i in order], extension=[want["extension"][i] for i in order])

    # guide_summary -E -L --prime [--prime-edits --prime-out]
    regions = va.Regions(packed, iv, rule="inside")
    codes, loci = gen.enumerate_guides(regions)
    regions.close()
    tuples = loci_tuples(loci)
    ids = ["%s:%d:%s" % (chrom[c], p, "-" if s else "+") for c, p, s in tuples]
    alone, want = pc.expected(contigs, tuples, pe2), pc.expected(contigs, tuples, pe2, edits)
    assert 40 < len(codes) < 400 and want["stats"]["pairs"] >= 20 and want["stats"]["off_contig"] >= 2
    base = ("guide_summary", "-G", tmp_path / "g.fa", "-I", tmp_path / "idx", "-M", "2", "-E", tmp_path / "t.bed")
    r = run(*base, "-L", tmp_path / "plain.bed", "-O", tmp_path / "plain.tsv")
    assert r.returncode == 0, r.stderr
    plain_bed, plain_rows = lines_of("plain.bed"), lines_of("plain.tsv")
    assert len(plain_bed) == len(codes)
    defined = np.array([pc.keep(rw, False, False) for rw in alone["rows"]])  # --prime alone: the candidates with a context
    assert 0 < defined.sum() < len(defined)
    r = run(*base, "-L", tmp_path / "x.bed", "-O", tmp_path / "x.tsv", "--prime", "PE2")
    assert r.returncode == 0, r.stderr
    assert lines_of("x.bed") == [ln + col for ln, col, k in zip(plain_bed, columns(alone), defined) if k]
    assert lines_of("x.tsv") == [plain_rows[0]] + [ln for ln, k in zip(plain_rows[1:], defined) if k]
    r = run(*base, "-L", tmp_path / "x2.bed", "-O", tmp_path / "x2.tsv", "--prime=17,41,13,13,10,34,5,21,2,17,3,1", "--prime-allow-weak")
    assert r.returncode == 0 and (tmp_path / "x2.bed").read_bytes() == (tmp_path / "x.bed").read_bytes()  # the preset, spelled out
    keep = np.array([pc.keep(rw, True, False) for rw in want["rows"]])
    assert 0 < keep.sum() < defined.sum()
    r = run(*base, "-L", tmp_path / "z.bed", "-O", tmp_path / "z.tsv", "--prime", "PE2", "--prime-edits", tmp_path / "e.tsv", "--prime-out", tmp_path / "zp.tsv")
    assert r.returncode == 0, r.stderr
    assert lines_of("z.bed") == [ln + col for ln, col, k in zip(plain_bed, columns(want), keep) if k]
    assert lines_of("z.tsv") == [plain_rows[0]] + [ln for ln, k in zip(plain_rows[1:], keep) if k]
    kept_ids = [i for i, k in zip(ids, keep) if k]  # (every candidate of a pair survives; the pairs number the survivors)
    renumber = np.cumsum(keep) - 1
    kept_want = dict(want, pairs=want["pairs"].copy())
    kept_want["pairs"]["candidate"] = renumber[want["pairs"]["candidate"].astype(np.int64)]
    assert lines_of("zp.tsv") == pair_lines(by_sorted_edit(kept_want, edits), kept_ids, edits)
    for args, text in (((*base, "--prime-edits", tmp_path / "e.tsv"), "give --prime"), ((*base, "--prime-allow-weak"), "give --prime"),
                       ((*base, "--prime-out", tmp_path / "p.tsv"), "give --prime"),
                       ((*base, "--prime", "PE2", "--prime-out", tmp_path / "p.tsv"), "give --prime-edits"),
                       ((*base[:7], "-B", tmp_path / "plain.bed", "--prime", "PE2"), "give -E"), ((*base, "--prime", "PE2", "-D", "0,0"), "one device"),
                       ((*base, "--prime", "PE3"), "--prime takes"), ((*base, "--prime", "17,41,13,13,10,48,5,21,2,17,3,1"), "--prime takes"),
                       ((*base, "--prime", "17,41,13,13,10,34,5,21,2,17,3"), "--prime takes")):
        r = run(*args)
        assert r.returncode != 0 and text in r.stderr, (args, r.stderr)
    (tmp_path / "bad.tsv").write_text("%s\t5\t1\tA\n%s\t5\t0\tG\n" % (chrom[4], chrom[4]))  # two alleles of one position
    r = run(*base, "--prime", "PE2", "--prime-edits", tmp_path / "bad.tsv")
    assert r.returncode != 0 and "two edits at one position" in (r.stderr + r.stdout)

    # pattern_search -E --prime SPEC --prime-edits --prime-out: Cas12a
    pattern, proto = "TTTV" + "N" * 23, (4, 23)
    sh = va.PrimeShape(**OTHERS["Cas12a"][2])
    spec = "22,20,10,12,6,25,3,0,4,4,6,0"
    (tmp_path / "p.bed").write_text("".join("%s\t%d\t%d\n" % (chrom[c], a, b) for c, a, b in iv))
    found = gen.enumerate_pattern(pattern, proto, targets=iv)
    ptuples = loci_tuples(found.loci)
    pids = ["%s:%d:%s" % (chrom[c], p, "-" if s else "+") for c, p, s in ptuples]
    pw, pn = pc.expected(contigs, ptuples, sh, few), pc.expected(contigs, ptuples, sh)
    pkeep = np.array([pc.keep(rw, True, False) for rw in pw["rows"]])
    pdefined = np.array([pc.keep(rw, False, False) for rw in pn["rows"]])
    assert len(found) >= 10 and 0 < pkeep.sum() < pdefined.sum() and pw["stats"]["pairs"] >= 5
    pbase = ("pattern_search", "-i", tmp_path / "idx", "-q", pattern, "-p", "%d,%d" % proto, "-B", tmp_path / "p.bed", "-M", "2")
    r = run(*pbase, "-E", tmp_path / "pe.tsv", "-O", tmp_path / "po.tsv")
    assert r.returncode == 0, r.stderr
    pe, po = lines_of("pe.tsv"), lines_of("po.tsv")
    assert len(pe) == len(found) + 1
    r = run(*pbase, "-E", tmp_path / "pex.tsv", "-O", tmp_path / "pox.tsv", "--prime", spec)
    assert r.returncode == 0, r.stderr
    head = pe[0] + "\tpbsLen\tpbsGC\tprimePairs"
    assert lines_of("pex.tsv") == [head] + [ln + col for ln, col, k in zip(pe[1:], columns(pn), pdefined) if k]
    r = run(*pbase, "-E", tmp_path / "pez.tsv", "-O", tmp_path / "poz.tsv", "--prime", spec, "--prime-edits", tmp_path / "few.tsv", "--prime-out", tmp_path / "pp.tsv")
    assert r.returncode == 0, r.stderr
    assert lines_of("pez.tsv") == [head] + [ln + col for ln, col, k in zip(pe[1:], columns(pw), pkeep) if k]
    assert lines_of("poz.tsv") == [po[0]] + [ln for ln, k in zip(po[1:], pkeep) if k]
    renumber = np.cumsum(pkeep) - 1
    kept_pw = dict(pw, pairs=pw["pairs"].copy())
    kept_pw["pairs"]["candidate"] = renumber[pw["pairs"]["candidate"].astype(np.int64)]
    assert lines_of("pp.tsv") == pair_lines(by_sorted_edit(kept_pw, few), [i for i, k in zip(pids, pkeep) if k], few)
    for args, text in (((*pbase, "-E", tmp_path / "x.tsv", "-O", tmp_path / "xo.tsv", "--prime-allow-weak"), "give --prime"),
                       ((*pbase[:5], "-R", tmp_path / "g.fa", "-M", "2", "-O", tmp_path / "x.tsv", "--prime", spec), "give -E"),
                       ((*pbase, "-E", tmp_path / "x.tsv", "-O", tmp_path / "xo.tsv", "--prime", "PE2"), "preset"),
                       ((*pbase, "-E", tmp_path / "x.tsv", "-O", tmp_path / "xo.tsv", "--prime", "28,20,10,12,6,25,3,0,4,4,6,0"), "--prime takes")):
        r = run(*args)
        assert r.returncode != 0 and text in (r.stderr + r.stdout), (args, r.stderr)
    gen.close()
