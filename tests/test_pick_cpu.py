"""vsc_pick_host - the per-target pick with spacing as host code - against the plain-Python restatement of
tests/pick_cases.py, the key helpers (order_bits, pick_key, pick_column) and the refusals.  No device is needed."""
import ctypes as C

import numpy as np
import pytest

import pick_cases as pk
import varscot_amd as va
from varscot_amd import _lib

CONTIG_DTYPE = np.dtype([("offset", "<u8"), ("length", "<u4"), ("reserved", "<u4")])


def contigs_of(lens):
    a = np.zeros(len(lens), dtype=CONTIG_DTYPE)
    off = 0
    for i, n in enumerate(lens):
        a["offset"][i], a["length"][i] = off, n
        off += n + 64
    return a


def host(lens, loci, target, key, n_targets, k, spacing, **shape):
    sh = va.PickShape(k, spacing, **shape)
    return va.pick_host(contigs_of(lens), pk.loci_array(loci, va.LOCUS_DTYPE), np.array(target, dtype=np.uint32),
                        np.array(key, dtype=np.uint64), n_targets, sh, rank=True)


def same(got, want):
    picks, counts, rank, stats = pk.as_arrays(want)
    assert got[0].dtype == np.uint32 and got[1].dtype == np.uint32 and got[2].dtype == np.uint32
    assert np.array_equal(got[0], picks) and np.array_equal(got[1], counts) and np.array_equal(got[2], rank)
    assert {k: got[3][k] for k in stats} == stats


def test_fixture_floors():
    sizes = pk.small_floors()
    f = pk.small()
    assert len(f["loci"]) > 800 and sum(sizes) > 600 and len(sizes) == 14


@pytest.mark.parametrize("key_set", ["ties", "high", "ends"])
def test_host_equals_restatement_over_the_grid(key_set):
    f = pk.small()
    for k in pk.KS:
        for spacing in pk.SPACINGS:
            same(host(f["lens"], f["loci"], f["target"], f["keys"][key_set], f["n_targets"], k, spacing), pk.small_expected(key_set, k, spacing))


def test_host_on_shuffled_candidates():
    f = pk.small()
    order = np.random.default_rng(3).permutation(len(f["loci"]))
    loci = [f["loci"][i] for i in order]
    target = [f["target"][i] for i in order]
    for key_set in f["keys"]:
        key = [f["keys"][key_set][i] for i in order]
        for k, spacing in ((4, 20), (32, 1), (1, 0)):
            want = pk.pick(f["lens"], loci, target, key, f["n_targets"], k, spacing)
            same(host(f["lens"], loci, target, key, f["n_targets"], k, spacing), want)


def test_boundary_fixture_floors():
    assert pk.boundary_floors() == list(pk.SIZES)


@pytest.mark.parametrize("order", pk.ORDERS)
@pytest.mark.parametrize("n_contigs", [1, 3])
def test_host_equals_restatement_on_the_boundary_fixtures(n_contigs, order):
    f = pk.boundary(n_contigs)
    for key_set in pk.BOUNDARY_KEYS:
        loci, target, key = pk.boundary_inputs(n_contigs, key_set, order)
        for k in pk.KS:
            for spacing in pk.SPACINGS:
                same(host(f["lens"], loci, target, key, f["n_targets"], k, spacing), pk.boundary_expected(n_contigs, key_set, order, k, spacing))


def test_host_equals_restatement_on_large_small_large():
    assert pk.same_wave_floors(64) == [True, False, True, False, True, False]   # memory, register, memory; register, memory, register
    f = pk.same_wave(64)
    got = host(f["lens"], f["loci"], f["target"], f["key"], f["n_targets"], pk.SAME_WAVE_K, pk.SAME_WAVE_SPACING)
    same(got, pk.same_wave_expected(64))


def test_replicas_compose_and_permute_as_the_restatement_says():
    """The expectation of the device's scale tests - composed from two restatement calls, then carried through a permutation -
    against the restatement and the host on the whole input, at a size where that is quick."""
    f = pk.small()
    m = len(f["loci"])
    for n, distinct in ((3 * m + 17, False), (2 * m, False), (4 * m + 400, True)):
        idx, target, key, n_targets, block = pk.replicas(n, distinct)
        assert n_targets == 14 * -(-n // m) and target.dtype == np.uint32 and key.dtype == np.uint64
        loci = [f["loci"][i] for i in idx]
        composed = pk.replicas_expected(n, 4, 20, block)
        want = pk.pick(f["lens"], loci, [int(t) for t in target], [int(q) for q in key], n_targets, 4, 20)
        same(composed, want)
        same(host(f["lens"], loci, target, key, n_targets, 4, 20), want)
        if distinct:
            order = np.random.default_rng(17).permutation(n)
            want = pk.pick(f["lens"], [loci[i] for i in order], [int(t) for t in target[order]], [int(q) for q in key[order]], n_targets, 4, 20)
            same(pk.permuted(composed, order), want)
            assert not np.array_equal(pk.permuted(composed, order)[0], composed[0])


def test_all_keys_equal_picks_by_index():
    lens = [500]
    loci = [(0, 10 * i, i % 2) for i in range(40)]
    for spacing in (0, 15):
        want = pk.pick(lens, loci, [0] * 40, [5] * 40, 1, 4, spacing)
        same(host(lens, loci, [0] * 40, [5] * 40, 1, 4, spacing), want)
    assert pk.pick(lens, loci, [0] * 40, [5] * 40, 1, 4, 0)[0][0] == [0, 1, 2, 3]


def test_min_key_is_inclusive():
    lens = [200]
    loci = [(0, 0, 0), (0, 50, 0), (0, 100, 0)]
    key = [99, 100, 101]
    got = host(lens, loci, [0, 0, 0], key, 1, 4, 0, min_key=100)
    same(got, pk.pick(lens, loci, [0, 0, 0], key, 1, 4, 0, min_key=100))
    assert got[0][0].tolist() == [2, 1, pk.NONE, pk.NONE] and got[3]["below_min_key"] == 1


def test_plus_and_minus_with_one_cut_coordinate():
    # '+' at p: x = p + 17; '-' at q: x = q + 6 - one coordinate for q = p + 11
    lens = [200]
    loci = [(0, 40, 0), (0, 51, 1)]
    assert pk.cut_coordinate(40, 0, 23, 17) == pk.cut_coordinate(51, 1, 23, 17)
    for spacing, n in ((0, 2), (1, 1)):
        got = host(lens, loci, [0, 0], [7, 7], 1, 4, spacing)
        same(got, pk.pick(lens, loci, [0, 0], [7, 7], 1, 4, spacing))
        assert got[1][0] == n


def test_equal_coordinates_on_two_contigs_do_not_conflict():
    lens = [100, 100]
    loci = [(0, 30, 0), (1, 30, 0), (0, 31, 0)]
    got = host(lens, loci, [0, 0, 0], [3, 2, 1], 1, 4, 50)
    same(got, pk.pick(lens, loci, [0, 0, 0], [3, 2, 1], 1, 4, 50))
    assert got[0][0].tolist() == [0, 1, pk.NONE, pk.NONE] and got[3]["targets_short"] == 1


def test_sites_leaving_their_contig_and_bad_targets():
    lens = [100, 23]
    loci = [(0, 77, 0), (0, 78, 0), (1, 0, 1), (1, 1, 0), (2, 0, 0), (0, 0, 2), (0, 0xFFFFFFF0, 0), (0, 5, 0), (0, 6, 0), (0, 7, 0)]
    target = [0, 0, 1, 1, 0, 0, 0, 2, pk.NONE, 0xFFFFFFFE]
    key = list(range(10, 20))
    got = host(lens, loci, target, key, 2, 2, 0)
    same(got, pk.pick(lens, loci, target, key, 2, 2, 0))
    assert got[3]["invalid"] == 5 and got[3]["bad_target"] == 2 and got[3]["no_target"] == 1 and got[3]["eligible"] == 2


def test_other_site_lengths_and_cuts():
    lens = [300]
    rng = np.random.default_rng(5)
    for site_len, cut in ((16, 0), (27, 18), (27, 22), (32, 32)):
        loci = [(0, int(p), int(s)) for p, s in zip(rng.integers(0, 300 - site_len + 2, 60), rng.integers(0, 2, 60))]
        key = [int(x) for x in rng.integers(0, 4, 60)]
        target = [int(x) for x in rng.integers(0, 3, 60)]
        want = pk.pick(lens, loci, target, key, 3, 5, 12, site_len=site_len, cut=cut)
        same(host(lens, loci, target, key, 3, 5, 12, site_len=site_len, cut=cut), want)


def test_no_candidates():
    got = host([100], [], [], [], 3, 2, 5)
    assert got[0].shape == (3, 2) and (got[0] == pk.NONE).all() and (got[1] == 0).all() and len(got[2]) == 0


def raw(params, n=1, picks=True, counts=True, key=True, loci=True, target=True, contigs=True, n_targets=1):
    ct = contigs_of([100])
    lo = pk.loci_array([(0, 0, 0)], va.LOCUS_DTYPE)
    tg, ky = np.zeros(1, dtype=np.uint32), np.zeros(1, dtype=np.uint64)
    pi, co = np.zeros(32, dtype=np.uint32), np.zeros(1, dtype=np.uint32)
    p = lambda a, on: _lib.ptr(a) if on else None
    return va.lib().vsc_pick_host(p(ct, contigs), 1, p(lo, loci), n, p(tg, target), p(ky, key), n_targets, C.byref(params) if params else None,
                                  p(pi, picks), p(co, counts), None, None)


def test_refusals():
    ok = lambda **kw: _lib.PickParams(kw.get("site_len", 23), kw.get("cut", 17), kw.get("k", 4), kw.get("spacing", 0), kw.get("min_key", 0),
                                      kw.get("reserved", 0))
    assert raw(ok()) == 0
    for bad in (dict(site_len=15), dict(site_len=33), dict(cut=24), dict(k=0), dict(k=33), dict(reserved=1)):
        assert raw(ok(**bad)) == -22, bad
    assert raw(None) == -22
    for missing in ("picks", "counts", "key", "loci", "target", "contigs"):
        assert raw(ok(), **{missing: False}) == -22, missing
    assert raw(ok(), n=0xFFFFFFFF) == -34
    assert raw(ok(), n=0xFFFFFFFE + 2) == -34
    with pytest.raises(ValueError):
        va.PickShape(0)
    with pytest.raises(ValueError):
        va.PickShape(4, site_len=23, cut=24)


def test_order_bits_is_monotone():
    tiny = np.float64(5e-324)
    sample = np.array([-np.inf, -1e308, -2.5, -1.0, -2.2250738585072014e-308, -tiny, -0.0, 0.0, tiny, 2.2250738585072014e-308, 1.0, 2.5,
                       1e308, np.inf], dtype=np.float64)
    assert (np.diff(sample) >= 0).all()
    bits = va.order_bits(sample)
    assert bits.dtype == np.uint64
    assert all(int(a) < int(b) for a, b in zip(bits, bits[1:]))   # -0.0 just below +0.0
    assert int(va.order_bits(np.array([np.nan]))[0]) == 0 and int(bits[0]) > 0
    rnd = np.sort(np.random.default_rng(1).normal(size=1000) * 1e3)
    rb = va.order_bits(rnd)
    assert all(int(a) <= int(b) for a, b in zip(rb, rb[1:]))
    assert int(va.order_bits(np.array([0.0]))[0]) == 1 << 63 and int(va.order_bits(np.array([-0.0]))[0]) == (1 << 63) - 1


def test_pick_key_packs_most_significant_first():
    a = np.array([3, 70000, 0], dtype=np.uint32)
    b = np.array([1, 2, 9], dtype=np.uint8)
    key = va.pick_key([a, b], [14, 2])
    assert key.dtype == np.uint64 and key.tolist() == [(3 << 2) | 1, (16383 << 2) | 2, 3]
    assert va.pick_key([np.array([2 ** 64 - 1], dtype=np.uint64)], [64]).tolist() == [2 ** 64 - 1]
    assert va.pick_key([np.array([1], dtype=np.uint64), np.array([5], dtype=np.uint64)], [44, 20]).tolist() == [(1 << 20) | 5]
    for cols, bits in (([a, b], [60, 5]), ([a], [0]), ([a], [65]), ([a, b], [14]), ([a.astype(np.int64)], [14]), ([a.astype(np.float64)], [14]),
                       ([a, b[:2]], [14, 2]), ([], [])):
        with pytest.raises(ValueError):
            va.pick_key(cols, bits)


def test_pick_columns_quantise_as_the_tools_do():
    assert va.pick_column("mit", [0.0, 42.494, 100.0]).tolist() == [0, 4249, 10000]  # specificities are 0 .. 100: 14 bits hold them
    pairs = np.array([[3, 2], [0, 0], [pk.NONE, pk.NONE], [2 ** 21, 2 ** 20]], dtype=np.uint32)
    assert va.pick_column("oof", pairs).tolist() == [666, 0, 0, 500]
    assert va.pick_column("mh", pairs).tolist() == [3, 0, 0, 2 ** 20 - 1]
    eff = va.pick_column("eff", np.array([-1.0, 0.0, 1.0, np.nan]))
    assert eff[0] < eff[1] < eff[2] < 2 ** 20 and eff[3] == 0
    with pytest.raises(ValueError):
        va.pick_column("gc", [1])


def test_pick_column_clamps_what_is_undefined():
    assert va.pick_column("mit", [np.nan, -3.0, -0.0, 12.344]).tolist() == [0, 0, 0, 1234]
    assert va.pick_column("table", [np.inf]).tolist() == [10 ** 8]   # (pick_key clips it to the column's 14 bits)
    assert va.pick_key([va.pick_column("table", [np.inf, 100.0])], [14]).tolist() == [16383, 10000]


def test_n_zero_refuses_before_it_writes():
    picks, counts = np.full(8, 7, dtype=np.uint32), np.full(2, 7, dtype=np.uint32)
    bad = _lib.PickParams(23, 17, 4, 0, 0, 1)
    assert va.lib().vsc_pick_host(_lib.ptr(contigs_of([100])), 1, None, 0, None, None, 2, C.byref(bad), _lib.ptr(picks), _lib.ptr(counts), None,
                                  None) == -22
    assert (picks == 7).all() and (counts == 7).all()
    ok = _lib.PickParams(23, 17, 4, 0, 0, 0)
    assert va.lib().vsc_pick_host(_lib.ptr(contigs_of([100])), 1, None, 0, None, None, 2, C.byref(ok), _lib.ptr(picks), _lib.ptr(counts), None,
                                  None) == 0
    assert (picks == pk.NONE).all() and (counts == 0).all()


def test_tools_refuse_pick_options_they_cannot_serve(tmp_path):
    """Every refusal comes before a device is opened: the options alone, or the -E / -B file read on the host."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    run = lambda *a: subprocess.run([os.path.join(root, "varscot_amd", "bin", a[0])] + [str(x) for x in a[1:]], capture_output=True,  # noqa: E731
                                    text=True, timeout=300)
    f = pk.small()
    with open(tmp_path / "g.fa", "w") as fa:
        for i, s in enumerate(f["contigs"]):
            fa.write(">c%d\n%s\n" % (i, s))
    assert run("bidir_index", "-G", tmp_path / "g.fa", "-I", tmp_path / "idx").returncode == 0
    (tmp_path / "named.bed").write_text("c0\t0\t100\tg1\nc0\t100\t200\tg1\n")
    (tmp_path / "bare.bed").write_text("c0\t0\t100\tg1\nc0\t100\t200\n")
    gs = ("guide_summary", "-G", tmp_path / "g.fa", "-I", tmp_path / "idx", "-M", "2", "-O", tmp_path / "o.tsv")
    e = ("-E", tmp_path / "named.bed", "-L", tmp_path / "l.bed")
    ps = ("pattern_search", "-i", tmp_path / "idx", "-q", "N" * 21 + "GG", "-p", "0,20", "-M", "2", "-O", tmp_path / "po.tsv")
    pe = ("-E", tmp_path / "pe.tsv", "-B", tmp_path / "named.bed")
    for args, text in (((*gs, *e, "-b", "mit"), "give -k"), ((*gs, *e, "-c", "name"), "give -k"),
                       ((*gs, "-B", tmp_path / "named.bed", "-k", "4"), "give -E"),
                       ((*gs, "-E", tmp_path / "named.bed", "-k", "4"), "give -L"),
                       ((*gs, *e, "-k", "4", "-D", "0,0"), "device list"),
                       ((*gs, *e, "-k", "0"), "-k takes"), ((*gs, *e, "-k", "33"), "-k takes"), ((*gs, *e, "-k", "4,-1"), "-k takes"),
                       ((*gs, *e, "-k", "4,x"), "-k takes"), ((*gs, *e, "-k", "4", "-c", "gene"), "-c takes"),
                       ((*gs, *e, "-k", "4", "-b", "gc"), "-b takes"), ((*gs, *e, "-k", "4", "-b", "table"), "give -W"),
                       ((*gs, *e, "-k", "4", "-b", "mit,eff"), "give -Y"), ((*gs, *e, "-k", "4", "-b", "oof"), "give -H"),
                       ((*gs, *e, "-k", "4", "-b", "mh"), "give -H"),
                       ((*gs, "-E", tmp_path / "bare.bed", "-L", tmp_path / "l.bed", "-k", "4", "-c", "name"), "has no name column"),
                       ((*ps, *pe, "-b", "oof"), "give -k"), ((*ps, *pe, "-c", "name"), "give -k"),
                       ((*ps, "-E", tmp_path / "pe.tsv", "-k", "4", "-b", "oof", "-H", "8"), "give -E -B"),
                       ((*ps[:5], "-R", tmp_path / "g.fa", "-M", "2", "-O", tmp_path / "po.tsv", "-k", "4"), "give -E -B"),
                       ((*ps, *pe, "-k", "4"), "give -b"), ((*ps, *pe, "-k", "4", "-b", "table"), "give -W"),
                       ((*ps, *pe, "-k", "4", "-b", "eff"), "give -Y"), ((*ps, *pe, "-k", "4", "-b", "mh"), "give -H"),
                       ((*ps, *pe, "-k", "4", "-b", "oof", "-H", "8", "-D", "0,1"), "device list"),
                       ((*ps, "-E", tmp_path / "pe.tsv", "-B", tmp_path / "bare.bed", "-k", "4", "-b", "oof", "-H", "8", "-c", "name"),
                        "has no name column")):
        r = run(*args)
        assert r.returncode != 0 and text in (r.stderr + r.stdout), (args[0], args[-4:], r.stderr, r.stdout)
        assert "device available" not in r.stderr
