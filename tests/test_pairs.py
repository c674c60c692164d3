"""vsc_hits_pairs / vsc_guides_pairs on the device: the paired sites of guide pairs, rows and site records byte for byte what the
definition gives when every record of one guide is held against every record of the other (tests/pairs_cases.py) - for both
search algorithms, selected, empty and one-record results, a merged two-context result, the discovery of the pairs themselves
and guide_summary -J."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import varscot_amd as va
from varscot_amd import _lib
import pairs_cases as pc
import regions_cases as rc
from helpers import random_seq

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "varscot_amd", "bin")


@pytest.fixture(scope="module")
def ctx():
    c = va.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def pl():
    p = pc.planted()
    p["packed"] = va.PackedGenome.from_sequences(p["contigs"])
    return p


@pytest.fixture(scope="module")
def gen(ctx, pl):
    g = ctx.load_genome(pl["packed"])
    yield g
    g.close()


@pytest.fixture(scope="module")
def found(gen, pl):
    """The records of the planted genome at M mismatches (scan), on the device and on the host."""
    h = gen.search(pl["guides"], pc.M, algorithm="scan")
    yield h, h.to_numpy()
    h.close()


def same(got_rows, got_sites, want_rows, want_sites):
    assert got_rows.dtype == va.PAIR_SUMMARY_DTYPE and got_sites.dtype == va.PAIR_SITE_DTYPE
    assert got_rows.tobytes() == want_rows.tobytes()
    assert got_sites.tobytes() == pc.sites_array(want_sites).tobytes()


@pytest.mark.parametrize("algorithm", ["scan", "seed"])
def test_planted_pairs_equal_brute_force(gen, pl, algorithm):
    hits = gen.search(pl["guides"], pc.M, algorithm=algorithm)
    rec = hits.to_numpy()
    want_rows, want_sites = pc.brute_hits_pairs(rec, pc.PAIRS, pc.DELTA, pl["exclude"])
    rows, sites = hits.pairs(pc.PAIRS, pc.DELTA, exclude=pl["exclude"], sites=True)
    same(rows, sites, want_rows, want_sites)
    assert hits.pairs(pc.PAIRS, pc.DELTA, exclude=pl["exclude"]).tobytes() == want_rows.tobytes()  # the rows alone: the same
    # ---- what keeps the comparison from passing on nothing ----
    assert int(rows["sites"].sum()) >= 20 and len(sites) == int(rows["sites"].sum())
    strand = (rec["info"] >> 31)
    assert set(strand[sites["a_rec"]].tolist()) == {0, 1}                      # both strand assignments
    assert np.all(strand[sites["a_rec"]] != strand[sites["b_rec"]])
    assert rows["on_target"].tolist() == [1, 0, 0, 0, 1, 1]                    # (A, B), its duplicate and (B, A): the same locus
    assert rows["sites"][3] == 0 and not rows["nm_sum"][3].any()              # guide B of pair 3 has no hit at all
    assert np.array_equal(np.cumsum(rows["sites"]) - rows["sites"], np.searchsorted(sites["pair"], np.arange(len(pc.PAIRS))))
    lo, hi = pc.DELTA
    first = sites[sites["pair"] == 0]
    for d, inside in ((lo - 1, False), (lo, True), (hi, True), (hi + 1, False)):
        for a_pos, b_pos in (pl["minus_plus"][d], pl["plus_minus"][d]):  # (position of A's record, of B's record)
            ra = np.nonzero((rec["guide"] == pc.A) & (rec["contig"] == 0) & (rec["pos"] == a_pos))[0]
            rb = np.nonzero((rec["guide"] == pc.B) & (rec["contig"] == 0) & (rec["pos"] == b_pos))[0]
            assert len(ra) == 1 and len(rb) == 1, d  # both records exist whether they pair or not
            hit = first[(first["a_rec"] == ra[0]) & (first["b_rec"] == rb[0])]
            assert len(hit) == (1 if inside else 0), d
            if inside:
                assert int(hit["delta"][0]) == d
    assert {lo, hi} <= set(sites["delta"].tolist()) and not {lo - 1, hi + 1} & set(sites["delta"].tolist())
    # the excluded perfect site is in the records and in no site; same strand and other contig never pair
    pa = np.nonzero((rec["guide"] == pc.A) & (rec["pos"] == pl["perfect"][0]) & (strand == 1))[0]
    assert len(pa) == 1 and pa[0] not in first["a_rec"]
    for a_pos, b_contig, b_pos in ((pl["same_strand"][0], 0, pl["same_strand"][1]), (pl["cross_contig"][0], 1, pl["cross_contig"][1])):
        ra = np.nonzero((rec["guide"] == pc.A) & (rec["contig"] == 0) & (rec["pos"] == a_pos))[0]
        rb = np.nonzero((rec["guide"] == pc.B) & (rec["contig"] == b_contig) & (rec["pos"] == b_pos))[0]
        assert len(ra) == 1 and len(rb) == 1
        assert not ((first["a_rec"] == ra[0]) & (first["b_rec"] == rb[0])).any()
    # without exclude the on-target is a site like any other
    rows2, sites2 = hits.pairs(pc.PAIRS, pc.DELTA, sites=True)
    same(rows2, sites2, *pc.brute_hits_pairs(rec, pc.PAIRS, pc.DELTA))
    assert rows2["sites"][0] == rows["sites"][0] + 1 and not rows2["on_target"].any()
    assert hits.to_numpy().tobytes() == rec.tobytes()  # the records are what they were
    hits.close()


def test_wide_range_many_partners_several_workgroups(found, pl):
    hits, rec = found
    pairs = pc.all_ordered_pairs()
    want_rows, want_sites = pc.brute_hits_pairs(rec, pairs, pc.WIDE, pl["exclude"])
    total = len(want_sites)
    assert total > 1024 and total % 64 and total % 256
    items = sum(int((rec["guide"] == a).sum()) for a, _ in pairs)
    assert items > 4 * 256 and items % 256  # several workgroups, the last one partly idle
    rows, sites = hits.pairs(pairs, pc.WIDE, exclude=pl["exclude"], sites=True)
    same(rows, sites, want_rows, want_sites)
    assert np.bincount(sites["a_rec"]).max() > 8
    # the cross-contig windows are close in global position and inside this range: still no pair
    cross = (rec["contig"][sites["a_rec"]] != rec["contig"][sites["b_rec"]])
    assert not cross.any()
    # PAM-in only, and a range nothing meets
    for delta in ((-60, -1), (15000, 16000)):  # (no contig is 15 000 long)
        r, s = hits.pairs(pairs, delta, sites=True)
        same(r, s, *pc.brute_hits_pairs(rec, pairs, delta))
    assert len(s) == 0 and len(hits.pairs(pairs, (-60, -1), sites=True)[1]) > 0


def test_selected_empty_and_one_record_results(gen, pl):
    sel = gen.search_select(pl["guides"], pc.M, top_k=5)
    rec = sel.to_numpy()
    assert 0 < len(rec) <= 5 * pc.N_GUIDES
    rows, sites = sel.pairs(pc.all_ordered_pairs(), pc.WIDE, exclude=pl["exclude"], sites=True)
    same(rows, sites, *pc.brute_hits_pairs(rec, pc.all_ordered_pairs(), pc.WIDE, pl["exclude"]))
    assert len(sites) > 0
    sel.close()
    two = [pl["guides"][pc.ONCE], pl["guides"][pc.NEVER]]
    one = gen.search(two, 0)
    rec = one.to_numpy()
    assert len(rec) == 1 and rec["pos"][0] == pl["once"]
    rows, sites = one.pairs([(0, 1), (1, 0)], pc.WIDE, sites=True)
    assert not rows.view(np.uint8).any() and len(sites) == 0
    one.close()
    empty = gen.search([pl["guides"][pc.NEVER], pl["guides"][pc.NOHIT]], 0)
    assert len(empty) == 0
    rows, sites = empty.pairs([(0, 1), (1, 0)], pc.WIDE, sites=True)
    assert len(rows) == 2 and not rows.view(np.uint8).any() and len(sites) == 0
    empty.close()


def raw(hits, n_guides, pairs, delta, rows, sites=None, capacity=0, exclude=None):
    p = _lib.PairParams(delta[0], delta[1])
    pr = None if pairs is None else np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 2)
    n = C.c_uint64(999)
    rc_ = va.lib().vsc_hits_pairs(hits._h, n_guides, _lib.ptr(pr), 0 if pr is None else len(pr), C.byref(p), _lib.ptr(exclude),
                                  _lib.ptr(rows), _lib.ptr(sites), capacity, C.byref(n))
    return rc_, int(n.value)


def test_no_pairs_short_capacity_and_invalid_arguments(found, pl):
    hits, rec = found
    assert hits.pairs(np.zeros((0, 2), dtype=np.uint32), pc.DELTA).shape == (0,)
    assert raw(hits, pc.N_GUIDES, None, pc.DELTA, None) == (0, 0)  # n_pairs == 0: nothing to do
    want_rows, want_sites = pc.brute_hits_pairs(rec, pc.PAIRS, pc.DELTA)
    total = len(want_sites)
    rows = np.zeros(len(pc.PAIRS), dtype=va.PAIR_SUMMARY_DTYPE)
    sites = np.zeros(total, dtype=va.PAIR_SITE_DTYPE)
    code, n = raw(hits, pc.N_GUIDES, pc.PAIRS, pc.DELTA, rows, sites, total - 1)
    assert code == -34 and n == total and rows.tobytes() == want_rows.tobytes()  # VSC_ERR_RANGE, rows valid, n_sites set
    with pytest.raises(va.VarscotError) as e:
        hits.pairs(pc.PAIRS, pc.DELTA, sites=True, max_sites=total - 1)
    assert e.value.code == -34
    code, n = raw(hits, pc.N_GUIDES, pc.PAIRS, pc.DELTA, rows, sites, total)
    assert (code, n) == (0, total) and sites.tobytes() == pc.sites_array(want_sites).tobytes()
    for bad in ([(2, 2)], [(0, pc.N_GUIDES)], [(pc.N_GUIDES, 0)], [(0, 1), (3, 3)]):
        rows = np.zeros(len(bad), dtype=va.PAIR_SUMMARY_DTYPE)
        assert raw(hits, pc.N_GUIDES, bad, pc.DELTA, rows)[0] == -22, bad
    rows = np.zeros(1, dtype=va.PAIR_SUMMARY_DTYPE)
    assert raw(hits, 4, [(0, 1)], pc.DELTA, rows)[0] == -22        # the records hold guides >= 4
    assert raw(hits, pc.N_GUIDES, [(0, 1)], (5, 4), rows)[0] == -22
    assert raw(hits, pc.N_GUIDES, [(0, 1)], (0, 2 ** 30 + 1), rows)[0] == -22
    assert raw(hits, pc.N_GUIDES, [(0, 1)], pc.DELTA, None)[0] == -22  # rows missing
    bad_ex = np.zeros(pc.N_GUIDES, dtype=va.LOCUS_DTYPE)
    bad_ex["strand"][3] = 2
    assert raw(hits, pc.N_GUIDES, [(0, 1)], pc.DELTA, rows, exclude=bad_ex)[0] == -22
    p = _lib.PairParams(0, 10)
    p.reserved[1] = 1
    pr = np.array([[0, 1]], dtype=np.uint32)
    assert va.lib().vsc_hits_pairs(hits._h, pc.N_GUIDES, _lib.ptr(pr), 1, C.byref(p), None, _lib.ptr(rows), None, 0, None) == -22
    assert va.lib().vsc_hits_pairs(None, pc.N_GUIDES, _lib.ptr(pr), 1, C.byref(p), None, _lib.ptr(rows), None, 0, None) == -22
    assert hits.to_numpy().tobytes() == rec.tobytes()


def test_timing_untouched_and_scratch_goes_back(pl):
    own = va.Context(0)
    g = own.load_genome(pl["packed"])
    hits = g.search(pl["guides"], pc.M)
    before = own.timing()
    first = hits.pairs(pc.PAIRS, pc.DELTA, exclude=pl["exclude"], sites=True)
    assert own.timing() == before
    own.release_scratch()
    again = hits.pairs(pc.PAIRS, pc.DELTA, exclude=pl["exclude"], sites=True)
    assert again[0].tobytes() == first[0].tobytes() and again[1].tobytes() == first[1].tobytes()
    hits.close()
    g.close()
    own.close()


# ---- discovery and closure -----------------------------------------------------------------------------------------------------
def closure_genome():
    rng = np.random.default_rng(91)
    contigs = [random_seq(rng, n) for n in rc.LENS]
    return contigs, [(0, 900, 1700), (0, 9000, 9500), (1, 300, 800)]


def test_closure_every_discovered_pair_finds_its_own_locus(ctx):
    contigs, iv = closure_genome()
    packed = va.PackedGenome.from_sequences(contigs)
    g = ctx.load_genome(packed)
    reg = va.Regions(packed, iv, rule="inside")
    delta = va.nickase_delta(-4, 20)
    codes, loci, pairs = g.enumerate_pairs(delta, reg)
    plain = g.enumerate_guides(reg)
    assert codes.tobytes() == plain[0].tobytes() and loci.tobytes() == plain[1].tobytes()
    assert pairs.dtype == np.uint32 and pairs.shape[1] == 2 and 20 < len(pairs) < 2000
    assert np.array_equal(pairs, va.pair_loci(loci, delta))
    assert np.array_equal(pairs, pc.brute_loci_pairs(loci, delta))
    assert np.all(loci["strand"][pairs[:, 0]] == 1) and np.all(loci["strand"][pairs[:, 1]] == 0)
    for other in ((-40, -7), (-3000, 3000), (0, 0)):  # PAM-in, every candidate of a contig, nothing but a shared start
        assert np.array_equal(g.enumerate_pairs(other, reg)[2], pc.brute_loci_pairs(loci, other)), other
    hits = g.search(codes, 0)
    rec = hits.to_numpy()
    rows, sites = hits.pairs(pairs, delta, exclude=loci, sites=True)
    assert (rows["on_target"] == 1).all()
    want_rows, want_sites = pc.brute_hits_pairs(rec, pairs.tolist(), delta,
                                                np.stack([loci["contig"], loci["pos"], loci["strand"]], axis=1))
    same(rows, sites, want_rows, want_sites)
    without = hits.pairs(pairs, delta)
    assert np.array_equal(without["sites"], rows["sites"] + 1)
    # labels ride along as they do for enumerate_guides
    assert np.array_equal(g.enumerate_pairs(delta, reg, labels=True)[3], g.enumerate_guides(reg, labels=True)[2])
    with pytest.raises(va.VarscotError) as e:
        g.enumerate_pairs((5, 4), reg)
    assert e.value.code == -22
    hits.close()
    g.close()


# ---- two contexts ---------------------------------------------------------------------------------------------------------------
def test_merged_result_and_host_only_candidates(found, pl):
    hits, rec = found
    m = va.MultiContext([0, 0])
    try:
        g = m.load_genome(pl["packed"])
        merged = g.search(pl["guides"], pc.M)
        assert merged.to_numpy().tobytes() == rec.tobytes()
        one = hits.pairs(pc.PAIRS, pc.DELTA, exclude=pl["exclude"], sites=True)
        got = merged.pairs(pc.PAIRS, pc.DELTA, n_guides=pc.N_GUIDES, exclude=pl["exclude"], sites=True)
        assert got[0].tobytes() == one[0].tobytes() and got[1].tobytes() == one[1].tobytes()
        # one paired site has its windows on different sides of the shard boundary
        boundary = pl["packed"].shard_words(0, 2)[1] * 32
        a_pos, b_pos, planted_at = pl["across"]
        assert planted_at == boundary and int(pl["packed"].contigs["offset"][0]) == 0
        s = got[1][got[1]["pair"] == 0]
        ra, rb = rec[s["a_rec"]], rec[s["b_rec"]]
        across = (ra["contig"] == 0) & (rb["contig"] == 0) & (ra["pos"] == a_pos) & (rb["pos"] == b_pos)
        assert across.sum() == 1 and a_pos + 23 <= boundary <= b_pos
        with pytest.raises(ValueError):
            merged.pairs(pc.PAIRS, pc.DELTA)  # a merged result does not know its guides
        merged.close()
        # the host-only candidates of the device set go through the host path
        contigs, iv = closure_genome()
        packed = va.PackedGenome.from_sequences(contigs)
        reg = va.Regions(packed, iv, rule="inside")
        delta = va.nickase_delta(-4, 20)
        g2 = m.load_genome(packed)
        codes, loci, pairs = g2.enumerate_pairs(delta, reg)
        assert len(pairs) > 20 and np.array_equal(pairs, pc.brute_loci_pairs(loci, delta))
        single_ctx = hits.ctx
        sg = single_ctx.load_genome(packed)
        s_codes, s_loci, s_pairs = sg.enumerate_pairs(delta, reg)
        sg.close()
        assert codes.tobytes() == s_codes.tobytes() and loci.tobytes() == s_loci.tobytes() and pairs.tobytes() == s_pairs.tobytes()
    finally:
        m.close()


# ---- the tool -------------------------------------------------------------------------------------------------------------------
def test_guide_summary_pairs_file(ctx, tmp_path):
    contigs, iv = closure_genome()
    names = ["chr1 assembled", "chr2", "chr3"]
    with open(tmp_path / "g.fa", "w") as f:
        for n, s in zip(names, contigs):
            f.write(">%s\n%s\n" % (n, "\n".join(s[i:i + 60] for i in range(0, len(s), 60))))
    (tmp_path / "t.bed").write_text("".join("%s\t%d\t%d\n" % (names[c].split()[0], a, b) for c, a, b in iv))
    run = lambda *a: subprocess.run([os.path.join(BIN, a[0])] + list(a[1:]), capture_output=True, text=True, timeout=600)
    assert run("bidir_index", "-G", str(tmp_path / "g.fa"), "-I", str(tmp_path / "idx")).returncode == 0
    base = ["guide_summary", "-G", str(tmp_path / "g.fa"), "-I", str(tmp_path / "idx"), "-M", "3"]
    r = run(*base, "-E", str(tmp_path / "t.bed"), "-L", str(tmp_path / "found.bed"), "-j", "-4,20", "-J", str(tmp_path / "out.tsv"),
            "-O", str(tmp_path / "e.tsv"))
    assert r.returncode == 0, r.stderr
    # the Python route
    packed = va.PackedGenome.from_sequences(contigs)
    g = ctx.load_genome(packed)
    delta = va.nickase_delta(-4, 20)
    codes, loci, pairs = g.enumerate_pairs(delta, va.Regions(packed, iv, rule="inside"))
    hits = g.search(codes, 3)
    rows = hits.pairs(pairs, delta, exclude=loci)
    hits.close()
    g.close()
    ids = ["%s:%d:%s" % (names[l["contig"]].split()[0], l["pos"], "+-"[l["strand"]]) for l in loci]
    want = ["#pairId\tguideA\tguideB\toffset\tsites\tonTarget\tminNmSum\t" + "\t".join("ps%d" % k for k in range(7))]
    for (a, b), row in zip(pairs.tolist(), rows):
        some = np.nonzero(row["nm_sum"])[0]
        want.append("\t".join([ids[a] + "|" + ids[b], ids[a], ids[b], str(int(loci["pos"][b]) - int(loci["pos"][a]) - 23),
                               str(int(row["sites"])), str(int(row["on_target"])), str(int(some[0])) if len(some) else "-"] +
                              [str(int(x)) for x in row["nm_sum"][:7]]))
    assert len(want) > 20 and (rows["on_target"] == 1).all()
    assert (tmp_path / "out.tsv").read_text().splitlines() == want
    offsets = [int(w.split("\t")[3]) for w in want[1:]]
    assert min(offsets) >= -4 and max(offsets) <= 20
    # the summary is what it is without -J; -B pairs the same on-targets on the host; two devices give the same file
    r = run(*base, "-E", str(tmp_path / "t.bed"), "-O", str(tmp_path / "plain.tsv"))
    assert r.returncode == 0 and (tmp_path / "plain.tsv").read_bytes() == (tmp_path / "e.tsv").read_bytes()
    r = run(*base, "-B", str(tmp_path / "found.bed"), "-j", "-4,20", "-J", str(tmp_path / "b.tsv"), "-O", str(tmp_path / "b_sum.tsv"))
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "b.tsv").read_bytes() == (tmp_path / "out.tsv").read_bytes()
    r = run(*base, "-E", str(tmp_path / "t.bed"), "-j", "-4,20", "-J", str(tmp_path / "d.tsv"), "-O", str(tmp_path / "d_sum.tsv"), "-D", "0,0")
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "d.tsv").read_bytes() == (tmp_path / "out.tsv").read_bytes()
