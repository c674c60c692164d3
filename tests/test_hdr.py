"""HDR knock-in design on the device (vsc_loci_hdr, vsc_guides_hdr, vsc_pattern_guides_hdr and the two filters): bit for bit what
the definition gives when it is applied locus by locus in plain Python on strings (tests/hdr_cases.py).  Integers, so there is
no tolerance: rows, pairs, coverage and counts are compared as they are, the undefined row included."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import hdr_cases as hc
import varscot_amd as va
import wide_cases as wc
from helpers import random_seq, revcomp
from varscot_amd import _lib

pytestmark = pytest.mark.gpu

TILE = 1024  # candidates per wave of the pairs' and the filter's passes (include/varscot_hip.h)
DROP_FRONT, DROP_BACK = 3, 1  # words the partial object of the small genome does not hold
COUNTS = hc.CLASSES + ("with_pair", "with_usable", "pairs", "edits_covered", "pairs_by_flag")
NAMES = sorted(hc.SHAPES)
SETS = ["none", "snv", "indel"]
CDS = ["free", "cds", "other"]  # no CDS; the CDS under the standard code; under another code


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
        self.fn = {k: getattr(L, "%s_%s" % (kind, k)) for k in ("count", "data", "free", "hdr", "filter_hdr", "filter_prime")}

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

    def hdr(self, gen, shape, edits, capacity, cds=None, code=None):
        """(rows, pairs in the library's edit numbering, coverage over the sorted edits, stats, status)."""
        n = len(self)
        e = va.prime_edits(edits)[0] if edits is not None else None
        n_e = 0 if e is None else len(e)
        rows, pairs = np.empty((n, 2), dtype=np.uint32), np.zeros(capacity, dtype=va.HDR_PAIR_DTYPE)
        cov = np.empty((n_e, 2), dtype=np.uint32)
        st, count, sh = _lib.HdrStats(), C.c_uint64(), shape._struct()
        rc = self.fn["hdr"](self.ctx._h, gen._h, self.h, C.byref(sh), _lib.ptr(e) if n_e else None, n_e, cds._h if cds else None,
                            code.encode() if code else None, _lib.ptr(rows), _lib.ptr(pairs), capacity, C.byref(count), _lib.ptr(cov), C.byref(st))
        return rows, pairs[:min(capacity, int(count.value))], cov, st.as_dict(), rc

    def filter_code(self, gen, shape, edits, allow_open, cds=None):
        out = C.c_void_p()
        sh = shape._struct()
        e = va.prime_edits(edits)[0] if edits is not None else None
        n_e = 0 if e is None else len(e)
        return self.fn["filter_hdr"](self.ctx._h, gen._h, self.h, C.byref(sh), _lib.ptr(e) if n_e else None, n_e, cds._h if cds else None, None,
                                     int(allow_open), C.byref(out)), out

    def filter(self, gen, shape, edits, allow_open, cds=None):
        code, out = self.filter_code(gen, shape, edits, allow_open, cds)
        _lib.check(code, self.ctx._h)
        return Guides(self.ctx, out, self.pattern)

    def filter_prime(self, gen, shape, edits, allow_weak):
        out = C.c_void_p()
        sh = shape._struct()
        e = va.prime_edits(edits)[0]
        _lib.check(self.fn["filter_prime"](self.ctx._h, gen._h, self.h, C.byref(sh), _lib.ptr(e), len(e), int(allow_weak), C.byref(out)), self.ctx._h)
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
    locus of it with the invalid ones behind, its CDS, and per edit set and CDS the expected result, computed once."""
    cache = {}

    def get(name):
        if name not in cache:
            shape = hc.shape_of(name)
            contigs = hc.small_genome(shape.site_len, shape.context_len)
            packed = va.PackedGenome.from_sequences(list(contigs))
            loci = hc.every_locus(contigs) + hc.invalid_loci(contigs)
            sl = slice(DROP_FRONT, packed.n_words - DROP_BACK)
            part = va.Genome.from_shard(ctx, packed.hi[sl], packed.lo[sl], packed.nmask[sl], DROP_FRONT, sl.stop - sl.start, packed.contigs)
            segs = hc.cds_segments(contigs)
            cache[name] = {"shape": shape, "contigs": contigs, "packed": packed, "gen": ctx.load_genome(packed), "part": part, "loci": loci,
                           "arr": hc.locus_array(loci), "resident": (32 * sl.start, 32 * sl.stop), "sets": hc.edit_sets(contigs), "want": {},
                           "cds": va.Cds(packed, segs), "coding": {"free": None, "cds": hc.CodingMap(contigs, segs),
                                                                   "other": hc.CodingMap(contigs, segs, hc.OTHER_CODE)}}
        return cache[name]

    def want(name, which, cds="free", partial=False):
        s = get(name)
        key = (which, cds, partial)
        if key not in s["want"]:
            s["want"][key] = hc.expected(s["contigs"], s["loci"], s["shape"], s["sets"][which], s["coding"][cds], s["resident"] if partial else None)
        return s["want"][key]

    get.want = want
    yield get
    for s in cache.values():
        s["gen"].close()
        s["part"].close()
        s["cds"].close()


def call(s, gen, which, cds="free", loci=None, **kw):
    return gen.hdr(s["arr"] if loci is None else loci, s["shape"], s["sets"][which], cds=None if cds == "free" else s["cds"],
                   code=hc.OTHER_CODE if cds == "other" else None, coverage=True, **kw)


def same(got, want, edits):
    rows, pairs, coverage, stats = got
    assert rows.dtype == np.uint32 and rows.tobytes() == want["rows"].tobytes()
    assert counts(stats) == want["stats"] and sum(stats[k] for k in hc.CLASSES) == len(rows)
    if edits is None:
        assert pairs is None and coverage is None and stats["pairs"] == 0
    else:
        assert pairs.dtype == va.HDR_PAIR_DTYPE and pairs.tobytes() == want["pairs"].tobytes()
        assert coverage.tobytes() == want["coverage"].tobytes()


@pytest.mark.parametrize("which", SETS)
@pytest.mark.parametrize("name", NAMES)
def test_every_locus_of_a_small_genome(small, name, which):
    s = small(name)
    edits = s["sets"][which]
    same(call(s, s["part"], which, allow_partial=True), small.want(name, which, partial=True), edits)
    same(call(s, s["gen"], which), small.want(name, which), edits)


@pytest.mark.parametrize("cds", ["cds", "other"])
@pytest.mark.parametrize("which", ["snv", "indel"])
@pytest.mark.parametrize("name", ["SpCas9", "Cas12a", "seed1", "pamonly", "far1"])
def test_every_locus_against_a_cds(small, name, which, cds):
    s = small(name)
    got = call(s, s["gen"], which, cds)
    same(got, small.want(name, which, cds), s["sets"][which])
    assert got[1].tobytes() != small.want(name, which)["pairs"].tobytes()  # the CDS changes what may be substituted


def test_the_code_matters_and_the_partial_object_is_partial(small):
    a, b = small.want("SpCas9", "snv", "cds"), small.want("SpCas9", "snv", "other")
    assert a["pairs"].tobytes() != b["pairs"].tobytes()
    p = small.want("SpCas9", "indel", partial=True)["stats"]
    assert all(p[k] >= 5 for k in hc.CLASSES) and p["pairs"] > 300


@pytest.mark.parametrize("name", ["bare16", "front32", "Cas12a"])
def test_the_pattern_handle_at_other_site_lengths(ctx, small, name):
    """site_len 16, 27 and 32 through the pattern handle, where the caller vouches for the length; vsc_guides holds 23-mers."""
    s = small(name)
    sh, edits = s["shape"], s["sets"]["indel"]
    g = Guides.from_arrays(ctx, np.arange(len(s["arr"]), dtype=np.uint64), s["arr"], pattern=True)
    for gen, want in ((s["part"], small.want(name, "indel", "cds", partial=True)), (s["gen"], small.want(name, "indel", "cds"))):
        rows, pairs, cov, stats, rc = g.hdr(gen, sh, edits, want["stats"]["pairs"] + 5, cds=s["cds"])
        want_pairs, want_cov = sorted_numbering(want, edits)
        assert rc == 0 and rows.tobytes() == want["rows"].tobytes() and counts(stats) == want["stats"]
        assert pairs.tobytes() == want_pairs.tobytes() and cov.tobytes() == want_cov.tobytes()
    g.close()
    plain = Guides.from_arrays(ctx, np.arange(len(s["arr"]), dtype=np.uint64), s["arr"])
    assert plain.hdr(s["gen"], sh, edits, 0)[4] == -22 and "site_len" in va.lib().vsc_last_error(ctx._h).decode()
    plain.close()


# ---- 2. beyond one launch ----------------------------------------------------------------------------------------------------
def launch_waves():
    """The waves of a launch capped as the cells' grids are (wide_cases): CUs x 8 workgroups of 4 waves."""
    return torch.cuda.get_device_properties(0).multi_processor_count * wc.GROUPS_PER_CU * wc.WAVES_PER_GROUP


def test_more_candidates_than_a_launch_has_lanes_and_more_tiles_than_waves(ctx, small):
    name, which = "SpCas9", "few"  # one to six pairs per candidate, some with none: runs of them cross tile boundaries
    s = small(name)
    sh, edits, base = s["shape"], s["sets"][which], small.want(name, which, "cds")
    m = len(s["loci"])
    n = (launch_waves() + 3) * TILE + 17
    assert n > 3 * m and n > launch_waves() * 64
    idx = np.arange(n) % m
    loci = s["arr"][idx]
    rows, pairs, coverage, stats = call(s, s["gen"], which, "cds", loci=loci)
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
    tail = bp[bp["candidate"] < rem]
    usable = lambda q: q[(q["info"] >> 24 & hc.OPEN) == 0]  # noqa: E731
    last = np.bincount(usable(tail)["edit"], minlength=len(edits))
    assert (coverage[:, 0] == reps * base["coverage"][:, 0] + last).all()
    assert reps >= 1 and (coverage[:, 1] == base["coverage"][:, 1]).all()  # (every base pair occurs at least once)
    assert sum(stats[k] for k in hc.CLASSES) == n
    flags = want_pairs["info"] >> 24
    assert stats["pairs_by_flag"] == [int((flags >> b & 1).sum()) for b in range(6)] and sum(1 for v in stats["pairs_by_flag"] if v) >= 4
    # the filter over the same tiles: the survivors in input order
    keep = np.array([hc.keep(r, True, False) for r in base["rows"]])
    assert 0 < keep.sum() < len(keep)
    codes = np.arange(n, dtype=np.uint64) * np.uint64(3)
    g = Guides.from_arrays(ctx, codes, loci, pattern=True)
    out = g.filter(s["gen"], sh, edits, False, cds=s["cds"])
    got_codes, got_loci = out.arrays()
    chosen = np.nonzero(keep[idx])[0]
    assert got_codes.tobytes() == codes[chosen].tobytes() and got_loci.tobytes() == loci[chosen].tobytes()
    out.close()
    g.close()


# ---- 3. the bitmap and the launch width change no bit ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sparse(ctx):
    """A genome sized from the CU count - more candidates than a launch has lanes - with edits in a few cells only: most
    candidates reach none, and the edits lie on both sides of several cell edges."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = max(cus * 256 * 2 + 77, 70000)
    rng = np.random.default_rng(17)
    text = random_seq(rng, n + 64)
    packed = va.PackedGenome.from_sequences([text, random_seq(rng, 3000)])
    gen = ctx.load_genome(packed)
    edits = []
    for cell in (1, 2, 9, 40, n // 256 - 2):
        for p in (cell * 256 - 3, cell * 256 - 1, cell * 256, cell * 256 + 2, cell * 256 + 131):
            edits.append((0, p, 1, hc.other_letter(text[p])))
        edits.append((0, cell * 256 + 40, 0, "ACGTAC"))
        edits.append((0, cell * 256 + 77, 9, ""))
    edits += [(1, 5, 1, hc.other_letter(packed.contig_sequence(1)[5])), (1, 3000, 0, "T")]
    loci = [(0, p, p % 2) for p in range(n)]
    segs = [(0, a, a + 60, k, k % 2, 0) for k, a in enumerate(range(200, n - 100, 1500))]
    cds = va.Cds(packed, segs)
    sh = hc.shape_of("SpCas9")
    want = hc.expected([text, packed.contig_sequence(1)], loci, sh, edits, hc.CodingMap([text, packed.contig_sequence(1)], segs))
    yield {"gen": gen, "arr": hc.locus_array(loci), "edits": edits, "cds": cds, "shape": sh, "want": want, "n": n}
    cds.close()
    gen.close()


def test_the_bitmap_on_against_off_and_the_launch_width(ctx, sparse, small):
    L = va.lib()
    s, want = sparse, sparse["want"]
    assert 0 < want["stats"]["with_pair"] < want["stats"]["defined"] // 20 and want["stats"]["pairs"] > 500
    assert sparse["n"] > torch.cuda.get_device_properties(0).multi_processor_count * 256
    got = None
    try:
        for on, groups in ((1, 0), (0, 0), (1, 1), (0, 7), (1, 64), (1, 0)):
            assert L.vsc_debug_hdr_bitmap(ctx._h, on) == 0 and L.vsc_debug_hdr_groups_per_cu(ctx._h, groups) == 0
            rows, pairs, cov, stats = s["gen"].hdr(s["arr"], s["shape"], s["edits"], cds=s["cds"], coverage=True)
            mine = (rows.tobytes(), pairs.tobytes(), cov.tobytes(), counts(stats))
            if got is None:
                got = mine
                same((rows, pairs, cov, stats), want, s["edits"])
            assert mine == got, (on, groups)
            g = Guides.from_arrays(ctx, np.arange(len(s["arr"]), dtype=np.uint64), s["arr"])
            out = g.filter(s["gen"], s["shape"], s["edits"], True, cds=s["cds"])
            kept = out.arrays()[0]
            assert kept.tobytes() == np.nonzero([hc.keep(r, True, True) for r in want["rows"]])[0].astype(np.uint64).tobytes()
            out.close()
            g.close()
        # the small genome, where every cell is occupied: off against on, byte for byte
        t = small("Cas12a")
        for on in (0, 1):
            assert L.vsc_debug_hdr_bitmap(ctx._h, on) == 0
            same(call(t, t["gen"], "indel", "cds"), small.want("Cas12a", "indel", "cds"), t["sets"]["indel"])
    finally:
        L.vsc_debug_hdr_bitmap(ctx._h, 1)
        L.vsc_debug_hdr_groups_per_cu(ctx._h, 0)
    assert L.vsc_debug_hdr_bitmap(None, 1) == -22
    assert L.vsc_debug_hdr_groups_per_cu(ctx._h, 65) == -22 and L.vsc_debug_hdr_groups_per_cu(None, 1) == -22


# ---- 4. the pair contract ----------------------------------------------------------------------------------------------------
def test_the_pair_contract(ctx, small):
    name, which = "SpCas9", "indel"
    s = small(name)
    sh, edits, want = s["shape"], s["sets"][which], small.want(name, which, "cds")
    want_pairs, want_cov = sorted_numbering(want, edits)
    total = len(want_pairs)
    e = va.prime_edits(edits)[0]
    L, st = va.lib(), sh._struct()
    n = len(s["arr"])

    def run(pairs, capacity, rows=True, cov=True):
        r = np.full((n, 2), 7, dtype=np.uint32) if rows else None
        c = np.full((len(e), 2), 7, dtype=np.uint32) if cov else None
        count, stats = C.c_uint64(12345), _lib.HdrStats()
        rc = L.vsc_loci_hdr(ctx._h, s["gen"]._h, _lib.ptr(s["arr"]), n, C.byref(st), _lib.ptr(e), len(e), s["cds"]._h, None, _lib.ptr(r),
                            _lib.ptr(pairs), capacity, C.byref(count), _lib.ptr(c), C.byref(stats))
        return rc, r, c, int(count.value), stats.as_dict()

    rc, rows, cov, count, stats = run(None, 0)  # count only
    assert rc == 0 and count == total and rows.tobytes() == want["rows"].tobytes() and cov.tobytes() == want_cov.tobytes()
    assert counts(stats) == want["stats"]
    exact = np.zeros(total, dtype=va.HDR_PAIR_DTYPE)
    rc, rows, cov, count, _ = run(exact, total)
    assert rc == 0 and count == total and exact.tobytes() == want_pairs.tobytes()
    short = np.full(total, 0x5A5A5A5A, dtype=np.uint32).repeat(4).view(va.HDR_PAIR_DTYPE)[:total].copy()
    before = short.tobytes()
    rc, rows, cov, count, stats = run(short, total - 1)  # one short
    assert rc == -34 and "capacity" in L.vsc_last_error(ctx._h).decode()
    assert short.tobytes() == before  # nothing is written to pairs
    assert count == total and rows.tobytes() == want["rows"].tobytes() and cov.tobytes() == want_cov.tobytes() and counts(stats) == want["stats"]
    rc, _, _, count, stats = run(None, 0, rows=False, cov=False)  # every output but the count is optional
    assert rc == 0 and count == total and counts(stats) == want["stats"]  # (the covered edits are then counted on the device)
    assert L.vsc_loci_hdr(ctx._h, s["gen"]._h, _lib.ptr(s["arr"]), n, C.byref(st), _lib.ptr(e), len(e), None, None, None, None, 0, None, None, None) == 0
    # the wrapper's second call, when its first capacity was too small
    many = s["arr"][np.arange(3 * n) % n]
    rows, pairs, _, stats = s["gen"].hdr(many, sh, s["sets"]["snv"])
    assert len(pairs) == stats["pairs"] == 3 * small.want(name, "snv")["stats"]["pairs"] > max(3 * n, 1024)
    # nothing to do
    rows, pairs, coverage, stats = s["gen"].hdr(hc.locus_array([]), sh, edits, coverage=True)
    assert rows.shape == (0, 2) and len(pairs) == 0 and (coverage[:, 0] == 0).all() and (coverage[:, 1] == hc.UNDEF).all()
    assert counts(stats) == dict.fromkeys(COUNTS[:-1], 0) | {"pairs_by_flag": [0] * 6}
    t = ctx.timing()
    assert t["sites"] == 0 and t["total_ms"] == 0


# ---- 5. candidates where they lie ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted(ctx):
    """A 20 kb random genome with NGG sites (and CCN sites, their '-' form) at and next to the contig ends, edits over it - SNVs
    at every third position, and a few hundred insertions and deletions - and exon-like segments on both strands."""
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
    snv = [(c, p, 1, hc.other_letter(t[p])) for c, t in enumerate(contigs) for p in range(0, len(t), 3)]
    indel = []
    for c, t in enumerate(contigs):
        for k, p in enumerate(range(4, len(t) - 20, 37)):
            del_len, ins_len = ((0, 1), (0, 3), (0, 16), (1, 0), (3, 0), (16, 0), (3, 2))[k % 7]
            indel.append((c, p, del_len, random_seq(rng, ins_len) if ins_len else ""))
    order = rng.permutation(len(indel))
    segs, tx = [], 0
    for c, t in enumerate(contigs):
        for a in range(100, len(t) - 400, 700):  # two-exon transcripts, the frame carried over the junction
            strand = tx % 2
            first, second = ((a + 150, a + 290), (a, a + 100)) if strand else ((a, a + 100), (a + 150, a + 290))
            segs += [(c, first[0], first[1], tx, strand, 0), (c, second[0], second[1], tx, strand, (3 - (first[1] - first[0]) % 3) % 3)]
            tx += 1
    cds = va.Cds(packed, segs)
    yield {"contigs": contigs, "packed": packed, "gen": gen, "snv": snv, "indel": [indel[i] for i in order], "cds": cds,
           "coding": hc.CodingMap(contigs, segs)}
    cds.close()
    gen.close()


def test_enumerated_guides_where_they_lie(ctx, planted):
    gen, contigs, cds = planted["gen"], planted["contigs"], planted["cds"]
    cas9 = va.HDR_NUCLEASES["SpCas9"]
    plain = gen.enumerate_guides()
    codes, loci, rows = gen.enumerate_guides(hdr="SpCas9")
    assert codes.tobytes() == plain[0].tobytes() and loci.tobytes() == plain[1].tobytes() and len(codes) > 1000
    tuples = loci_tuples(loci)
    want = hc.expected(contigs, tuples, cas9, planted["snv"], planted["coding"])
    assert rows.dtype == np.uint32 and np.isin(rows, (0, hc.UNDEF)).all() and ((rows == hc.UNDEF) == (want["rows"] == hc.UNDEF)).all()
    assert want["stats"]["off_contig"] >= 6 and want["stats"]["pairs"] > 5000  # the sites at the contig ends have no context
    same(gen.hdr((codes, loci), cas9, planted["snv"], cds=cds, coverage=True), want, planted["snv"])
    # every candidate ends in NGG: an SNV blocks through the PAM exactly where it hits one of the two G
    dist, side, _, _, flags = va.unpack_hdr_info(want["pairs"]["info"])
    in_pam = (side == 2) & ((dist == 4) | (dist == 5))
    assert ((flags & hc.B_PAM != 0) == in_pam).all() and in_pam.any()
    assert all(want["stats"]["pairs_by_flag"][b] for b in (0, 3, 4, 5))  # (one SNV never makes two seed mismatches)
    # over the handle: what vsc_loci_hdr gives for the same loci
    want = hc.expected(contigs, tuples, cas9, planted["indel"], planted["coding"])
    g = Guides.from_arrays(ctx, plain[0], plain[1])
    rows, pairs, cov, stats, rc = g.hdr(gen, cas9, planted["indel"], want["stats"]["pairs"], cds=cds)
    want_pairs, want_cov = sorted_numbering(want, planted["indel"])
    assert rc == 0 and rows.tobytes() == want["rows"].tobytes() and pairs.tobytes() == want_pairs.tobytes() and cov.tobytes() == want_cov.tobytes()
    assert counts(stats) == want["stats"] and want["stats"]["pairs"] > 300 and all(want["stats"]["pairs_by_flag"][b] for b in (0, 1, 2, 3, 5))
    host = Guides.from_arrays(ctx, plain[0], plain[1], on_device=False)  # the host-only object goes the vsc_loci_hdr way
    h_rows, h_pairs, h_cov, h_stats, rc = host.hdr(gen, cas9, planted["indel"], want["stats"]["pairs"], cds=cds)
    assert rc == 0 and h_rows.tobytes() == rows.tobytes() and h_pairs.tobytes() == pairs.tobytes() and h_cov.tobytes() == cov.tobytes()
    assert counts(h_stats) == counts(stats)
    host.close()
    g.close()
    with pytest.raises(ValueError):
        gen.enumerate_guides(hdr="Cas12a")
    with pytest.raises(ValueError):
        gen.enumerate_guides(hdr_allow_open=False)
    with pytest.raises(ValueError):
        gen.enumerate_guides(hdr_edits=[(0, 5, 1, "A")])


def test_pattern_candidates_of_cas12a_and_the_filter_through_the_wrapper(planted):
    gen, contigs, cds = planted["gen"], planted["contigs"], planted["cds"]
    pattern, proto, sh = "TTTV" + "N" * 23, (4, 23), va.HDR_NUCLEASES["Cas12a"]
    edits = planted["indel"] + [e for e in planted["snv"] if e[1] % 2 and (e[0], e[1]) not in {(c, p) for c, p, _, _ in planted["indel"]}]
    plain = gen.enumerate_pattern(pattern, proto)
    found, rows = gen.enumerate_pattern(pattern, proto, hdr=sh)
    assert found.codes.tobytes() == plain.codes.tobytes() and found.loci.tobytes() == plain.loci.tobytes() and len(found) > 100
    tuples = loci_tuples(found.loci)
    want = hc.expected(contigs, tuples, sh, edits, planted["coding"])
    assert want["stats"]["defined"] > 100 and want["stats"]["pairs"] > 100
    same(gen.hdr(found, sh, edits, cds=cds, coverage=True), want, edits)
    # the filter through the wrapper: the survivors in input order, their rows; only the survivors are searched
    few = edits[:40]
    want_few = hc.expected(contigs, tuples, sh, few, planted["coding"])
    _, all_rows = gen.design_pattern(pattern, proto, 2)
    kept_n = {}
    for allow in (False, True):
        keep = np.array([hc.keep(r, True, allow) for r in want_few["rows"]])
        kept_n[allow] = int(keep.sum())
        kept, krows = gen.enumerate_pattern(pattern, proto, hdr=sh, hdr_edits=few, hdr_cds=cds, hdr_allow_open=allow)
        assert kept.codes.tobytes() == found.codes[keep].tobytes() and kept.loci.tobytes() == found.loci[keep].tobytes()
        assert krows.tobytes() == want_few["rows"][keep].tobytes()
        d_found, d_rows, d_hdr = gen.design_pattern(pattern, proto, 2, hdr=sh, hdr_edits=few, hdr_cds=cds, hdr_allow_open=allow)
        assert d_found.codes.tobytes() == kept.codes.tobytes() and d_hdr.tobytes() == krows.tobytes()
        assert d_rows.tobytes() == all_rows[keep].tobytes()
    assert 0 < kept_n[False] <= kept_n[True] < len(found)


# ---- 6. the filter ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["none", "few"])
def test_filter_rule_and_input_order(ctx, small, which):
    name = "pamonly"  # (no substitution outside the segments, none in the seed: some pairs stay OPEN)
    s = small(name)
    sh, edits, want = s["shape"], s["sets"][which], small.want(name, which, "cds")
    n = len(s["loci"])
    codes = np.arange(n, dtype=np.uint64) * np.uint64(5)
    g = Guides.from_arrays(ctx, codes, s["arr"])
    kept = {}
    for allow in (True, False):
        keep = np.array([hc.keep(r, edits is not None, allow) for r in want["rows"]])
        out = g.filter(s["gen"], sh, edits, allow, cds=s["cds"])
        got_codes, got_loci = out.arrays()
        out.close()
        assert got_codes.tobytes() == codes[keep].tobytes() and got_loci.tobytes() == s["arr"][keep].tobytes(), allow
        kept[allow] = int(keep.sum())
    if edits is None:
        assert kept[True] == kept[False] == want["stats"]["defined"]
    else:
        assert kept[True] == want["stats"]["with_pair"] and kept[False] == want["stats"]["with_usable"] and 0 < kept[False] < kept[True] < want["stats"]["defined"]
    t = ctx.timing()
    assert t["sites"] == n and t["score_ms"] == t["total_ms"] > 0
    assert t["genome_bytes"] == 32 * n + 48 * kept[False]  # (the last call's)
    host = Guides.from_arrays(ctx, codes, s["arr"], on_device=False)  # the host-only object: uploaded first, the same bytes
    keep = np.array([hc.keep(r, edits is not None, False) for r in want["rows"]])
    h_out = host.filter(s["gen"], sh, edits, False, cds=s["cds"])
    assert h_out.arrays()[0].tobytes() == codes[keep].tobytes()
    again = h_out.filter(s["gen"], sh, edits, False, cds=s["cds"])  # the survivors survive
    assert again.arrays()[0].tobytes() == codes[keep].tobytes()
    empty = again.filter(s["gen"], sh, [(0, 0, 1, "A")], True)  # an edit nobody reaches: an empty result is a result
    assert len(empty) == 0 and len(empty.filter(s["gen"], sh, edits, True).arrays()[0]) == 0
    for h in (empty, again, h_out, host, g):
        h.close()


def test_what_takes_the_filters_result(ctx, planted):
    gen, contigs, cds = planted["gen"], planted["contigs"], planted["cds"]
    cas9, edits = va.HDR_NUCLEASES["SpCas9"], planted["indel"]
    pcodes, ploci = gen.enumerate_guides()
    want = hc.expected(contigs, loci_tuples(ploci), cas9, edits, planted["coding"])
    keep = np.array([hc.keep(r, True, False) for r in want["rows"]])
    assert 0 < keep.sum() < want["stats"]["with_pair"] <= want["stats"]["defined"]
    k_codes, k_loci, k_rows = gen.enumerate_guides(hdr="SpCas9", hdr_edits=edits, hdr_cds=cds)
    assert k_codes.tobytes() == pcodes[keep].tobytes() and k_loci.tobytes() == ploci[keep].tobytes()
    assert k_rows.tobytes() == want["rows"][keep].tobytes()
    rows_all = gen.summarize(pcodes, 2, exclude=ploci)
    d = gen.design(None, 2, hdr=cas9, hdr_edits=edits, hdr_cds=cds)  # the filter's result goes on into the search
    assert len(d) == 4 and d[0].tobytes() == k_codes.tobytes() and d[2].tobytes() == rows_all[keep].tobytes() and d[3].tobytes() == k_rows.tobytes()
    # after the prime filter, in both orders the same survivors; through the wrapper the HDR rows come last
    pe2 = va.PRIME_EDITORS["PE2"]
    g = Guides.from_arrays(ctx, pcodes, ploci)
    a = g.filter_prime(gen, pe2, edits, True)
    a2 = a.filter(gen, cas9, edits, False, cds=cds)
    b = g.filter(gen, cas9, edits, False, cds=cds)
    b2 = b.filter_prime(gen, pe2, edits, True)
    assert 0 < len(a2) < min(len(a), len(b))
    for x, y in zip(a2.arrays(), b2.arrays()):
        assert x.tobytes() == y.tobytes()
    k = gen.enumerate_guides(prime=pe2, prime_edits=edits, hdr=cas9, hdr_edits=edits, hdr_cds=cds)
    assert len(k) == 4 and k[0].tobytes() == a2.arrays()[0].tobytes() and k[1].tobytes() == a2.arrays()[1].tobytes()
    survivors = set(loci_tuples(k[1]))
    assert k[3].tobytes() == want["rows"][[t in survivors for t in loci_tuples(ploci)]].tobytes()
    for h in (a, a2, b, b2, g):
        h.close()


# ---- 7. end to end ------------------------------------------------------------------------------------------------------------
def test_the_best_cutters_of_every_edit_and_their_donors(planted):
    gen, contigs, packed, cds = planted["gen"], planted["contigs"], planted["packed"], planted["cds"]
    cas9 = va.HDR_NUCLEASES["SpCas9"]
    rng = np.random.default_rng(6)
    edits = [planted["snv"][i] for i in rng.choice(len(planted["snv"]), size=1500, replace=False)]
    codes, loci = gen.enumerate_guides()
    tuples = loci_tuples(loci)
    rows, pairs, _, stats = gen.hdr((codes, loci), cas9, edits, cds=cds)
    want = hc.expected(contigs, tuples, cas9, edits, planted["coding"])
    assert pairs.tobytes() == want["pairs"].tobytes() and len(pairs) > 1000
    spec = (np.arange(len(codes), dtype=np.uint64) * np.uint64(2654435761)) % np.uint64(10007)  # a stand-in for a specificity column
    p_loci, p_edit, key = va.hdr_pick_inputs(pairs, loci, extra_columns=[(spec, 14)])
    pick = va.PickShape(3, spacing=2)
    picks, cnt, st = gen.pick(p_loci, key, pick, target=p_edit, n_targets=len(edits))
    # the key by hand from the restatement's words, followed by the host's pick
    flags, dist = want["pairs"]["info"] >> 24, want["pairs"]["info"] & 63
    want_key = np.array([((f & 32 == 0) << 8 | (f & 7 != 0) << 7 | (f & 8 != 0) << 6 | (63 - d)) << 14 for f, d in zip(flags.tolist(), dist.tolist())],
                        dtype=np.uint64)
    want_key |= np.minimum(spec[want["pairs"]["candidate"]], np.uint64(16383))
    assert key.tobytes() == want_key.tobytes()
    h_picks, h_cnt, _ = va.pick_host(packed.contigs, loci[want["pairs"]["candidate"]], want["pairs"]["edit"], want_key, len(edits), pick)
    assert picks.tobytes() == h_picks.tobytes() and cnt.tobytes() == h_cnt.tobytes() and cnt.max() >= 2 and (cnt == 0).any()
    first = picks[cnt > 0, 0]
    best = [want_key[want["pairs"]["edit"] == e].max() for e in np.nonzero(cnt > 0)[0]]
    assert (want_key[first] == best).all()  # the best key of every edit comes first
    # the donor of every pair with a substitution: the edit and exactly one more changed base, which is the pair's
    strands, seen = set(), 0
    for q in pairs[pairs["block"] != va.HDR_NO_BLOCK][::25]:
        locus, edit = tuples[int(q["candidate"])], edits[int(q["edit"])]
        text = contigs[locus[0]]
        donor = va.hdr_donor(text, locus, cas9, edit, q, arms=(len(text), len(text)))
        assert len(donor) == len(text)
        diff = [i for i in range(len(text)) if donor[i] != text[i]]
        assert len(diff) == 2 and edit[1] in diff
        other = next(i for i in diff if i != edit[1])
        _, b, _, r, _ = (int(v) for v in va.unpack_hdr_block(q["block"]))
        f0 = locus[1] - (cas9.down if locus[2] else cas9.up)
        assert other == f0 + (cas9.context_len - 1 - r if locus[2] else r) and donor[other] == "ACGT"[3 - b if locus[2] else b]
        strands.add(locus[2])
        seen += 1
    assert strands == {0, 1} and seen > 50


def test_a_shard_answers_for_what_it_holds(ctx, planted):
    packed, contigs, cas9 = planted["packed"], planted["contigs"], va.HDR_NUCLEASES["SpCas9"]
    n_words = packed.n_words
    loci = [(0, p, s) for p in list(range(2000, 2100)) + list(range(2200, 2280)) for s in (0, 1)]
    loci += loci_tuples(planted["gen"].enumerate_guides()[1])
    arr = hc.locus_array(loci)
    for first, words, own in ((64, n_words - 64, n_words - 64), (0, 70, 64)):  # nothing in front of word 64; nothing behind a 6-word halo
        sl = slice(first, first + words)
        shard = va.Genome.from_shard(ctx, packed.hi[sl], packed.lo[sl], packed.nmask[sl], first, own, packed.contigs)
        want = hc.expected(contigs, loci, cas9, planted["snv"], resident=(32 * first, 32 * (first + words)))
        assert want["stats"]["not_resident"] > 100 and want["stats"]["defined"] > 100 and want["stats"]["pairs"] > 100
        with pytest.raises(ValueError) as e:
            shard.hdr(arr, cas9, planted["snv"])
        assert "not resident" in str(e.value)
        same(shard.hdr(arr, cas9, planted["snv"], coverage=True, allow_partial=True), want, planted["snv"])
        shard.close()


def test_alternating_shapes_scratch_and_timing(ctx, small):
    combos = [("SpCas9", "indel", "cds"), ("Cas12a", "snv", "free"), ("bare16", "none", "free"), ("front32", "indel", "other"), ("nosub", "snv", "cds")]

    def run(k):
        name, which, cds = combos[k]
        s = small(name)
        got = call(s, s["gen"], which, cds)
        same(got, small.want(name, which, cds), s["sets"][which])
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
    ok = va.HDR_NUCLEASES["SpCas9"]._struct()
    count = C.c_uint64()

    def guides_hdr(shape, edits=None, n_e=0, handle=g.h, genome=gen._h, context=None, cds=None, code=None):
        return L.vsc_guides_hdr((context or ctx)._h, genome, handle, shape, _lib.ptr(edits), n_e, cds, code, _lib.ptr(rows), None, 0, C.byref(count),
                                None, None)

    good = dict(site_len=23, up=20, down=21, cut=17, max_dist=30, anchor=1, pam=(20, "NGG"), seed=(10, 10), proto=(0, 20), min_seed_mm=2,
                min_proto_mm=4)
    for kw in ({"site_len": 15}, {"site_len": 33, "up": 0}, {"up": 33, "down": 0}, {"down": 33, "up": 0}, {"up": 21}, {"cut": 0}, {"cut": 23},
               {"max_dist": 64}, {"anchor": 2}, {"pam": (20, "NGGNNNNNN")}, {"pam": (21, "NGG")}, {"pam": (20, (15, 0, 4))}, {"pam": (20, (15, 16, 4))},
               {"seed": (10, 17)}, {"seed": (14, 10)}, {"proto": (0, 33)}, {"proto": (4, 20)}, {"min_seed_mm": 11}, {"min_proto_mm": 21},
               {"flags": 8}, {"cut": 0xFFFFFFFF}, {"down": 0xFFFFFFFF}):
        sh = va.HdrShape(validate=False, **dict(good, **kw))
        st = sh._struct()
        assert guides_hdr(C.byref(st)) == -22, kw
        code, out = g.filter_code(gen, sh, None, True)
        assert code == -22 and not out.value
    with pytest.raises(va.VarscotError):
        gen.hdr(hc.locus_array([(0, 100, 0)]), va.HdrShape(validate=False, **dict(good, cut=23)))
    reserved = va.HDR_NUCLEASES["SpCas9"]._struct(reserved=1)
    assert guides_hdr(C.byref(reserved)) == -22 and "reserved" in L.vsc_last_error(ctx._h).decode()
    cas12a = va.HDR_NUCLEASES["Cas12a"]  # vsc_guides holds 23-mers
    st27 = cas12a._struct()
    assert guides_hdr(C.byref(st27)) == -22 and "site_len" in L.vsc_last_error(ctx._h).decode()
    assert g.filter_code(gen, cas12a, None, True)[0] == -22
    assert guides_hdr(None) == -22 and guides_hdr(C.byref(ok), genome=None) == -22 and guides_hdr(C.byref(ok), handle=None) == -22  # null arguments
    assert L.vsc_guides_filter_hdr(ctx._h, gen._h, g.h, C.byref(ok), None, 0, None, None, 1, None) == -22
    assert guides_hdr(C.byref(ok), None, 3) == -22 and "null" in L.vsc_last_error(ctx._h).decode()  # n_e > 0 with NULL edits
    assert guides_hdr(C.byref(ok), code=b"ACGT") == -22 and "64" in L.vsc_last_error(ctx._h).decode()  # a short code
    elsewhere = va.Cds(va.PackedGenome.from_sequences([c[:-1] for c in contigs]), [(0, 10, 40, 0, 0, 0)])  # a CDS of another contig table
    assert guides_hdr(C.byref(ok), cds=elsewhere._h) == -22 and "contig table" in L.vsc_last_error(ctx._h).decode()
    out = C.c_void_p()
    assert L.vsc_guides_filter_hdr(ctx._h, gen._h, g.h, C.byref(ok), None, 0, elsewhere._h, None, 1, C.byref(out)) == -22 and not out.value
    elsewhere.close()

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
        assert guides_hdr(C.byref(ok), e, len(e)) == -22 and word in L.vsc_last_error(ctx._h).decode(), bad
        out = C.c_void_p()
        assert L.vsc_guides_filter_hdr(ctx._h, gen._h, g.h, C.byref(ok), _lib.ptr(e), len(e), None, None, 1, C.byref(out)) == -22 and not out.value
    assert (rows == 9).all()  # checked before anything is written
    last = edits_of([(0, end - 16, 16, 16, 0xFFFFFFFF), (0, end, 0, 1, 3), (2, len(contigs[2]) - 1, 1, 0, 0)])  # at and up to a contig's end
    assert guides_hdr(C.byref(ok), last, 3) == 0
    assert L.vsc_loci_hdr(ctx._h, gen._h, None, 1, C.byref(ok), None, 0, None, None, _lib.ptr(rows), None, 0, None, None, None) == -22
    assert L.vsc_loci_hdr(ctx._h, gen._h, _lib.ptr(rows), 0xFFFFFFFF, C.byref(ok), None, 0, None, None, None, None, 0, None, None, None) == -34  # n
    assert L.vsc_loci_hdr(ctx._h, gen._h, _lib.ptr(rows), 1, C.byref(ok), _lib.ptr(last), 0xFFFFFFFF, None, None, None, None, 0, None, None, None) == -34  # n_e
    other = va.Context(0)  # a genome or an object of another context is refused
    assert guides_hdr(C.byref(ok), context=other) == -22
    o_gen = other.load_genome(planted["packed"])
    assert guides_hdr(C.byref(ok), genome=o_gen._h, context=other) == -22 and "another context" in L.vsc_last_error(other._h).decode()
    o_gen.close()
    other.close()
    g.close()


# ---- 8. the tools end to end ---------------------------------------------------------------------------------------------------
def test_both_tools_on_the_small_genome(ctx, tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    bin_dir = os.path.join(root, "varscot_amd", "bin")
    cas9, cas12a = va.HDR_NUCLEASES["SpCas9"], va.HDR_NUCLEASES["Cas12a"]
    contigs = list(hc.small_genome(23, 64))
    names = ["chr%d of the small genome" % (k + 1) for k in range(len(contigs))]
    chrom = [n.split()[0] for n in names]
    with open(tmp_path / "g.fa", "w") as f:
        for n, t in zip(names, contigs):
            f.write(">%s\n%s\n" % (n, "\n".join(t[i:i + 60] for i in range(0, len(t), 60))))
    iv = [(c, 0, len(t)) for c, t in enumerate(contigs)]
    (tmp_path / "t.bed").write_text("".join("%s\t%d\t%d\n" % (chrom[c], a, b) for c, a, b in iv))
    sets = hc.edit_sets(contigs)
    edits, few = sets["indel"], sets["few"]  # in the caller's order: the tool sorts them
    segs = hc.cds_segments(contigs)
    (tmp_path / "c.bed").write_text("".join("%s\t%d\t%d\ttx%d\t%d\t%s\n" % (chrom[c], a, b, tx, ph, "-" if st else "+") for c, a, b, tx, st, ph in segs))
    coding = hc.CodingMap(contigs, segs)

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
        return ["\tNA\tNA" if int(r[0]) == hc.UNDEF else "\t%d\t%d" % (r[0], r[1]) for r in want["rows"]]

    def pair_lines(want, keep, ids, tuples, given, sh):
        """The --hdr-out listing: the pairs of the survivors in ascending (guide, place of the edit among the sorted edits)."""
        _, _, inverse = va.prime_edits(given)
        pr = want["pairs"][keep[want["pairs"]["candidate"].astype(np.int64)]]
        pr = pr[np.lexsort((inverse[pr["edit"].astype(np.int64)], pr["candidate"]))]
        out = ["#chrom\tpos\tguideId\tdist\tseedMm\tprotoMm\tflags\tsubChrom\tsubPos\tsubBase"]
        for q in pr:
            c, p, _, _ = given[int(q["edit"])]
            dist, _, seed_mm, proto_mm, flags = (int(v) for v in va.unpack_hdr_info(q["info"]))
            text = "+".join(n for b, n in enumerate(va.HDR_FLAGS) if flags >> b & 1) or "-"
            sub = "-\t-\t-"
            if int(q["block"]) != va.HDR_NO_BLOCK:
                _, b, _, r, _ = (int(v) for v in va.unpack_hdr_block(q["block"]))
                _, pos, strand = tuples[int(q["candidate"])]
                f0 = pos - (sh.down if strand else sh.up)
                sub = "%s\t%d\t%s" % (chrom[c], f0 + (sh.context_len - 1 - r if strand else r), "ACGT"[3 - b if strand else b])
            out.append("%s\t%d\t%s\t%d\t%d\t%d\t%s\t%s" % (chrom[c], p, ids[int(q["candidate"])], dist, seed_mm, proto_mm, text, sub))
        return out

    # guide_summary -E -L --hdr [--hdr-edits --hdr-cds --hdr-allow-open --hdr-out]
    regions = va.Regions(packed, iv, rule="inside")
    codes, loci = gen.enumerate_guides(regions)
    regions.close()
    tuples = loci_tuples(loci)
    ids = ["%s:%d:%s" % (chrom[c], p, "-" if s else "+") for c, p, s in tuples]
    alone, want = hc.expected(contigs, tuples, cas9, None), hc.expected(contigs, tuples, cas9, few, coding)
    assert 40 < len(codes) < 400 and want["stats"]["pairs"] >= 20 and want["stats"]["off_contig"] >= 2 and want["stats"]["pairs_by_flag"][5] >= 1
    cds_obj = va.Cds(packed, segs)
    rows, pairs, _, _ = gen.hdr((codes, loci), cas9, few, cds=cds_obj)  # the Python call, which the tools are held against
    assert rows.tobytes() == want["rows"].tobytes() and pairs.tobytes() == want["pairs"].tobytes()
    base = ("guide_summary", "-G", tmp_path / "g.fa", "-I", tmp_path / "idx", "-M", "2", "-E", tmp_path / "t.bed")
    r = run(*base, "-L", tmp_path / "plain.bed", "-O", tmp_path / "plain.tsv")
    assert r.returncode == 0, r.stderr
    plain_bed, plain_rows = lines_of("plain.bed"), lines_of("plain.tsv")
    assert len(plain_bed) == len(codes)
    defined = np.array([hc.keep(rw, False, False) for rw in alone["rows"]])  # --hdr alone: the candidates with a context
    assert 0 < defined.sum() < len(defined)
    r = run(*base, "-L", tmp_path / "x.bed", "-O", tmp_path / "x.tsv", "--hdr", "SpCas9")
    assert r.returncode == 0, r.stderr
    assert lines_of("x.bed") == [ln + col for ln, col, k in zip(plain_bed, columns(alone), defined) if k]
    assert lines_of("x.tsv") == [plain_rows[0]] + [ln for ln, k in zip(plain_rows[1:], defined) if k]
    r = run(*base, "-L", tmp_path / "x2.bed", "-O", tmp_path / "x2.tsv", "--hdr=20,21,17,30,1,20,NGG,10,10,0,20,2,4,7", "--hdr-allow-open")
    assert r.returncode == 0 and (tmp_path / "x2.bed").read_bytes() == (tmp_path / "x.bed").read_bytes()  # the preset, spelled out
    kept_n = {}
    for allow in (False, True):
        keep = np.array([hc.keep(rw, True, allow) for rw in want["rows"]])
        kept_n[allow] = int(keep.sum())
        more = ("--hdr-allow-open",) if allow else ()
        r = run(*base, "-L", tmp_path / "z.bed", "-O", tmp_path / "z.tsv", "--hdr", "SpCas9", "--hdr-edits", tmp_path / "few.tsv", "--hdr-cds",
                tmp_path / "c.bed", "--hdr-out", tmp_path / "zp.tsv", *more)
        assert r.returncode == 0, r.stderr
        assert lines_of("z.bed") == [ln + col for ln, col, k in zip(plain_bed, columns(want), keep) if k]
        assert lines_of("z.tsv") == [plain_rows[0]] + [ln for ln, k in zip(plain_rows[1:], keep) if k]
        assert lines_of("zp.tsv") == pair_lines(want, keep, ids, tuples, few, cas9)
    assert 0 < kept_n[False] < kept_n[True] < defined.sum()
    for args, text in (((*base, "--hdr-edits", tmp_path / "e.tsv"), "give --hdr"), ((*base, "--hdr-allow-open"), "give --hdr"),
                       ((*base, "--hdr-out", tmp_path / "p.tsv"), "give --hdr"), ((*base, "--hdr-cds", tmp_path / "c.bed"), "give --hdr"),
                       ((*base, "--hdr", "SpCas9", "--hdr-out", tmp_path / "p.tsv"), "give --hdr-edits"),
                       ((*base[:7], "-B", tmp_path / "plain.bed", "--hdr", "SpCas9"), "give -E"), ((*base, "--hdr", "SpCas9", "-D", "0,0"), "one device"),
                       ((*base, "--hdr", "Cas9"), "--hdr takes"), ((*base, "--hdr", "Cas12a"), "preset"),
                       ((*base, "--hdr", "20,21,17,30,1,20,NGG,10,10,0,20,2,4,8"), "--hdr takes"),
                       ((*base, "--hdr", "20,21,23,30,1,20,NGG,10,10,0,20,2,4,7"), "--hdr takes"),
                       ((*base, "--hdr", "20,21,17,30,1,20,NGG,10,10,0,20,2,4"), "--hdr takes")):
        r = run(*args)
        assert r.returncode != 0 and text in r.stderr, (args, r.stderr)

    # pattern_search -E --hdr Cas12a --hdr-edits --hdr-cds --hdr-out
    pattern, proto = "TTTV" + "N" * 23, (4, 23)
    (tmp_path / "p.bed").write_text("".join("%s\t%d\t%d\n" % (chrom[c], a, b) for c, a, b in iv))
    found = gen.enumerate_pattern(pattern, proto, targets=iv)
    ptuples = loci_tuples(found.loci)
    pids = ["%s:%d:%s" % (chrom[c], p, "-" if s else "+") for c, p, s in ptuples]
    pw, pn = hc.expected(contigs, ptuples, cas12a, edits, coding), hc.expected(contigs, ptuples, cas12a, None)
    pkeep = np.array([hc.keep(rw, True, False) for rw in pw["rows"]])
    pdefined = np.array([hc.keep(rw, False, False) for rw in pn["rows"]])
    assert len(found) >= 10 and 0 < pkeep.sum() <= pdefined.sum() < len(found) and pw["stats"]["pairs"] >= 5
    prows, ppairs, _, _ = gen.hdr(found, cas12a, edits, cds=cds_obj)
    assert prows.tobytes() == pw["rows"].tobytes() and ppairs.tobytes() == pw["pairs"].tobytes()
    pbase = ("pattern_search", "-i", tmp_path / "idx", "-q", pattern, "-p", "%d,%d" % proto, "-B", tmp_path / "p.bed", "-M", "2")
    r = run(*pbase, "-E", tmp_path / "pe.tsv", "-O", tmp_path / "po.tsv")
    assert r.returncode == 0, r.stderr
    pe, po = lines_of("pe.tsv"), lines_of("po.tsv")
    assert len(pe) == len(found) + 1
    r = run(*pbase, "-E", tmp_path / "pex.tsv", "-O", tmp_path / "pox.tsv", "--hdr", "Cas12a")
    assert r.returncode == 0, r.stderr
    head = pe[0] + "\thdrPairs\thdrUsable"
    assert lines_of("pex.tsv") == [head] + [ln + col for ln, col, k in zip(pe[1:], columns(pn), pdefined) if k]
    r = run(*pbase, "-E", tmp_path / "pez.tsv", "-O", tmp_path / "poz.tsv", "--hdr", "18,19,22,30,0,0,TTTV,4,6,4,23,2,4,7", "--hdr-edits", tmp_path / "e.tsv",
            "--hdr-cds", tmp_path / "c.bed", "--hdr-out", tmp_path / "pp.tsv")
    assert r.returncode == 0, r.stderr
    assert lines_of("pez.tsv") == [head] + [ln + col for ln, col, k in zip(pe[1:], columns(pw), pkeep) if k]
    assert lines_of("poz.tsv") == [po[0]] + [ln for ln, k in zip(po[1:], pkeep) if k]
    assert lines_of("pp.tsv") == pair_lines(pw, pkeep, pids, ptuples, edits, cas12a)
    for args, text in (((*pbase, "-E", tmp_path / "x.tsv", "-O", tmp_path / "xo.tsv", "--hdr-allow-open"), "give --hdr"),
                       ((*pbase[:5], "-R", tmp_path / "g.fa", "-M", "2", "-O", tmp_path / "x.tsv", "--hdr", "Cas12a"), "give -E"),
                       ((*pbase, "-E", tmp_path / "x.tsv", "-O", tmp_path / "xo.tsv", "--hdr", "SpCas9"), "preset"),
                       ((*pbase, "-E", tmp_path / "x.tsv", "-O", tmp_path / "xo.tsv", "--hdr", "18,19,27,30,0,0,TTTV,4,6,4,23,2,4,7"), "--hdr takes")):
        r = run(*args)
        assert r.returncode != 0 and text in (r.stderr + r.stdout), (args, r.stderr)
    cds_obj.close()
    gen.close()
