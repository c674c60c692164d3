"""The per-target pick with spacing on the device (vsc_loci_pick, vsc_guides_pick, vsc_pattern_guides_pick) against the
plain-Python restatement of tests/pick_cases.py: picks, counts and rank compared as uint32 arrays, the stats' counts as
integers.  The restatement of every case is computed once (pick_cases caches the small grid)."""
import ctypes as C

import numpy as np
import pytest
import torch

import pick_cases as pk
import varscot_amd as va
import wide_cases as wc
from varscot_amd import _lib

pytestmark = pytest.mark.gpu

WAVE_CAP = 256  # records a wave of pick_select_kernel holds in registers (vsc_pick_device.h: kPickWaveCap)


@pytest.fixture(scope="module")
def ctx():
    c = va.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def small(ctx):
    f = pk.small()
    packed = va.PackedGenome.from_sequences(list(f["contigs"]))
    gen = ctx.load_genome(packed)
    regions = va.Regions(packed, f["intervals"], rule=f["rule"])
    loci = pk.loci_array(f["loci"], va.LOCUS_DTYPE)
    yield dict(f, packed=packed, gen=gen, regions=regions, arr=loci, tg=np.array(f["target"], dtype=np.uint32),
               gr=np.array(f["groups"], dtype=np.uint32), ky={k: np.array(v, dtype=np.uint64) for k, v in f["keys"].items()})
    regions.close()
    gen.close()


class Guides:
    """A vsc_guides (or, pattern=True, a vsc_pattern_guides) handle on the device and its pick call."""

    def __init__(self, ctx, handle, pattern=False):
        self.ctx, self.h, self.pattern = ctx, handle, pattern
        kind = "vsc_pattern_guides" if pattern else "vsc_guides"
        self.fn = {k: getattr(va.lib(), "%s_%s" % (kind, k)) for k in ("count", "data", "free", "pick", "microhomology")}

    @classmethod
    def from_arrays(cls, ctx, codes, loci, pattern=False, on_device=True):
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

    def pick_code(self, gen, key, n_targets, shape, regions=None, group=None, target=None, picked=False, gen_h=True, params=None):
        n = len(self)
        picks = np.full((n_targets, shape.k), 12345, dtype=np.uint32)
        counts = np.full(n_targets, 12345, dtype=np.uint32)
        rank = np.full(n, 12345, dtype=np.uint32)
        st, out = _lib.PickStats(), C.c_void_p()
        sh = params if params is not None else shape._struct()
        p = lambda a: _lib.ptr(a) if a is not None else None
        code = self.fn["pick"](self.ctx._h, gen._h if gen_h else None, self.h, regions._h if regions is not None else None, p(group), p(target),
                               n_targets, p(key), C.byref(sh), p(picks), p(counts), p(rank), C.byref(out) if picked else None, C.byref(st))
        return code, (picks, counts, rank, st.as_dict()), out

    def pick(self, gen, key, n_targets, shape, **kw):
        code, got, out = self.pick_code(gen, key, n_targets, shape, **kw)
        _lib.check(code, self.ctx._h)
        return got + ((Guides(self.ctx, out, self.pattern),) if kw.get("picked") else ())

    def close(self):
        if self.h:
            self.fn["free"](self.h)
            self.h = None


def same(got, want):
    picks, counts, rank, stats = pk.as_arrays(want)
    assert got[0].dtype == np.uint32 and np.array_equal(got[0], picks)
    assert np.array_equal(got[1], counts)
    assert np.array_equal(got[2], rank)
    assert {k: got[3][k] for k in stats} == stats


def test_fixture_floors():
    sizes = pk.small_floors()
    assert sum(1 for s in sizes if s > 64) >= 2 and max(sizes) < WAVE_CAP


# ---- the small grid -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key_set", ["ties", "high", "ends"])
def test_loci_pick_over_the_grid(small, key_set):
    for k in pk.KS:
        for spacing in pk.SPACINGS:
            got = small["gen"].pick(small["arr"], small["ky"][key_set], va.PickShape(k, spacing), target=small["tg"],
                                    n_targets=small["n_targets"], rank=True)
            same(got, pk.small_expected(key_set, k, spacing))


@pytest.mark.parametrize("key_set", ["ties", "high", "ends"])
def test_guides_pick_labels_on_the_device(ctx, small, key_set):
    g = Guides.from_arrays(ctx, np.zeros(len(small["arr"]), dtype=np.uint64), small["arr"])
    try:
        for k in pk.KS:
            for spacing in pk.SPACINGS:
                got = g.pick(small["gen"], small["ky"][key_set], small["n_targets"], va.PickShape(k, spacing), regions=small["regions"],
                             group=small["gr"])
                same(got, pk.small_expected(key_set, k, spacing))
    finally:
        g.close()


def test_guides_pick_given_targets_and_labels_without_groups(ctx, small):
    g = Guides.from_arrays(ctx, np.zeros(len(small["arr"]), dtype=np.uint64), small["arr"])
    try:
        for k, spacing in ((4, 20), (32, 1), (1, 0), (4, 1000)):
            got = g.pick(small["gen"], small["ky"]["ties"], small["n_targets"], va.PickShape(k, spacing), target=small["tg"])
            same(got, pk.small_expected("ties", k, spacing))
        # no group: the label is the target; 44 intervals, and with 20 targets the later labels are bad targets
        labels = pk.targets_of(small["lens"], small["intervals"], "inside", None, small["loci"])
        for n_targets in (44, 20):
            want = pk.pick(small["lens"], small["loci"], labels, small["keys"]["high"], n_targets, 4, 20)
            assert n_targets == 44 or want[3]["bad_target"] > 100
            same(g.pick(small["gen"], small["ky"]["high"], n_targets, va.PickShape(4, 20), regions=small["regions"]), want)
        # Genome.pick's regions path is the same call
        got = small["gen"].pick(small["arr"], small["ky"]["ends"], va.PickShape(4, 20), regions=small["regions"], groups=small["gr"], rank=True)
        same(got, pk.small_expected("ends", 4, 20))
    finally:
        g.close()


def test_shuffled_loci(small):
    order = np.random.default_rng(3).permutation(len(small["loci"]))
    loci = [small["loci"][i] for i in order]
    target = [small["target"][i] for i in order]
    key = [small["keys"]["ties"][i] for i in order]
    for k, spacing in ((4, 20), (32, 1)):
        got = small["gen"].pick(pk.loci_array(loci, va.LOCUS_DTYPE), np.array(key, dtype=np.uint64), va.PickShape(k, spacing),
                                target=np.array(target, dtype=np.uint32), n_targets=small["n_targets"], rank=True)
        same(got, pk.pick(small["lens"], loci, target, key, small["n_targets"], k, spacing))


def test_min_key_and_invalid_loci_on_the_device(small):
    lens = small["lens"]
    loci = list(small["loci"][:300]) + [(0, 5990, 0), (4, 0, 0), (0, 0, 2), (3, 1, 0), (0, 0xFFFFFFF0, 1)]
    target = list(small["target"][:300]) + [0, 0, 0, 0, 0]
    target[5], target[6] = 14, 0xFFFFFFFE
    key = list(small["keys"]["ties"][:300]) + [7] * 5
    want = pk.pick(lens, loci, target, key, 14, 4, 20, min_key=3)
    assert want[3]["invalid"] == 5 and want[3]["bad_target"] == 2 and want[3]["below_min_key"] > 20
    got = small["gen"].pick(pk.loci_array(loci, va.LOCUS_DTYPE), np.array(key, dtype=np.uint64), va.PickShape(4, 20, min_key=3),
                            target=np.array(target, dtype=np.uint32), n_targets=14, rank=True)
    same(got, want)


# ---- one large target: more records than a wave holds in registers ----------------------------------------------------------
def test_one_large_target(ctx):
    rng = np.random.default_rng(21)
    contig = pk._rnd(rng, 40000)
    loci = pk.enumerate_ngg([contig])
    n = len(loci)
    assert n > 16 * WAVE_CAP
    packed = va.PackedGenome.from_sequences([contig])
    gen = ctx.load_genome(packed)
    regions = va.Regions(packed, [(0, 0, 40000)], rule="overlap")
    g = Guides.from_arrays(ctx, np.zeros(n, dtype=np.uint64), pk.loci_array(loci, va.LOCUS_DTYPE))
    try:
        for name, key in (("ties", [int(x) for x in rng.integers(0, 8, n)]), ("wide", [int(x) for x in rng.integers(0, 1 << 62, n)])):
            for spacing in (0, 50):
                want = pk.pick([40000], loci, [0] * n, key, 1, 32, spacing)
                assert want[1] == [32]
                same(g.pick(gen, np.array(key, dtype=np.uint64), 1, va.PickShape(32, spacing), regions=regions), want)
        # spacing that the target cannot satisfy 32 times: the loop over the segment ends with nothing left
        want = pk.pick([40000], loci, [0] * n, key, 1, 32, 3000)
        assert 0 < want[1][0] < 32 and want[3]["targets_short"] == 1
        same(g.pick(gen, np.array(key, dtype=np.uint64), 1, va.PickShape(32, 3000), regions=regions), want)
    finally:
        g.close()
        regions.close()
        gen.close()


# ---- more targets than the launch has waves --------------------------------------------------------------------------------
def test_more_targets_than_waves(ctx):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    W = cus * wc.GROUPS_PER_CU * wc.WAVES_PER_GROUP
    n_targets = 2 * W + 3
    contig_len = 100000
    loci, target, key = pk.many_targets(n_targets, contig_len)
    packed = va.PackedGenome.from_sequences(["ACGT" * (contig_len // 4)])
    gen = ctx.load_genome(packed)
    try:
        want = pk.pick([contig_len], loci, target, key, n_targets, 2, 10)
        assert min(want[1]) >= 1 and want[1][-1] >= 1 and want[3]["targets_picked"] == n_targets
        got = gen.pick(pk.loci_array(loci, va.LOCUS_DTYPE), np.array(key, dtype=np.uint64), va.PickShape(2, 10),
                       target=np.array(target, dtype=np.uint32), n_targets=n_targets, rank=True)
        same(got, want)
    finally:
        gen.close()


# ---- segment sizes around every boundary of the select: 64 / 128 / 192 (a lane's register slots) and 256 (registers / memory) ----
@pytest.fixture(scope="module")
def boundary(ctx):
    """n_contigs -> the fixture of pick_cases.boundary with its genome loaded."""
    made = {}

    def get(n_contigs):
        if n_contigs not in made:
            f = pk.boundary(n_contigs)
            made[n_contigs] = dict(f, gen=ctx.load_genome(va.PackedGenome.from_sequences(list(f["contigs"]))))
        return made[n_contigs]

    yield get
    for f in made.values():
        f["gen"].close()


def boundary_arrays(n_contigs, key_set, order):
    loci, target, key = pk.boundary_inputs(n_contigs, key_set, order)
    return pk.loci_array(loci, va.LOCUS_DTYPE), np.array(target, dtype=np.uint32), np.array(key, dtype=np.uint64)


def test_boundary_fixture_floors():
    assert pk.boundary_floors() == list(pk.SIZES) and pk.WAVE_CAP == WAVE_CAP


@pytest.mark.parametrize("order", pk.ORDERS)
@pytest.mark.parametrize("n_contigs", [1, 3])
def test_loci_pick_at_the_segment_boundaries(boundary, n_contigs, order):
    f = boundary(n_contigs)
    for key_set in pk.BOUNDARY_KEYS:
        arr, tg, ky = boundary_arrays(n_contigs, key_set, order)
        for k in pk.KS:
            for spacing in pk.SPACINGS:
                got = f["gen"].pick(arr, ky, va.PickShape(k, spacing), target=tg, n_targets=f["n_targets"], rank=True)
                same(got, pk.boundary_expected(n_contigs, key_set, order, k, spacing))
        again = f["gen"].pick(arr, ky, va.PickShape(k, spacing), target=tg, n_targets=f["n_targets"], rank=True)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got[:3], again[:3]))


@pytest.mark.parametrize("order", pk.ORDERS)
def test_guides_pick_at_the_segment_boundaries_across_contigs(ctx, boundary, order):
    f = boundary(3)
    arr, tg, _ = boundary_arrays(3, "equal", order)
    g = Guides.from_arrays(ctx, np.zeros(len(arr), dtype=np.uint64), arr)   # the loci lie on the device
    try:
        for key_set in pk.BOUNDARY_KEYS:
            ky = boundary_arrays(3, key_set, order)[2]
            for k in pk.KS:
                for spacing in pk.SPACINGS:
                    got = g.pick(f["gen"], ky, f["n_targets"], va.PickShape(k, spacing), target=tg)
                    same(got, pk.boundary_expected(3, key_set, order, k, spacing))
    finally:
        g.close()


@pytest.mark.parametrize("order", pk.ORDERS)
@pytest.mark.parametrize("n_contigs", [1, 3])
def test_planted_spacing_triple_on_the_device(boundary, n_contigs, order):
    """Cuts at x, x + 19 and x + 20 ('-'), and a '-' with its cut at x: at spacing 20 the first and the third are picked, the
    second and the fourth are not - in every target of three or more, on both sides of 256 records."""
    f = boundary(n_contigs)
    planted = pk.boundary_planted(n_contigs, order)
    assert sum(1 for t in planted if f["size_of"][t] > WAVE_CAP) >= 5 and sum(1 for t in planted if f["size_of"][t] <= WAVE_CAP) >= 5
    for key_set in pk.BOUNDARY_KEYS:
        arr, tg, ky = boundary_arrays(n_contigs, key_set, order)
        for k in (4, 32):
            got = f["gen"].pick(arr, ky, va.PickShape(k, pk.BOUNDARY_SPACING), target=tg, n_targets=f["n_targets"], rank=True)
            same(got, pk.boundary_expected(n_contigs, key_set, order, k, pk.BOUNDARY_SPACING))
            picks, counts, rank, _ = got
            for t, p in planted.items():
                assert picks[t, :2].tolist() == [p[0], p[2]] and counts[t] >= 2, (key_set, k, f["size_of"][t])
                assert rank[p].tolist() == [0, pk.NONE, 1, pk.NONE][:len(p)], (key_set, k, f["size_of"][t])
            got = f["gen"].pick(arr, ky, va.PickShape(k, pk.BOUNDARY_SPACING - 1), target=tg, n_targets=f["n_targets"], rank=True)
            same(got, pk.boundary_expected(n_contigs, key_set, order, k, pk.BOUNDARY_SPACING - 1))
            picks, _, rank, _ = got
            for t, p in planted.items():   # one base less and the second no longer conflicts with the first; the fourth still does
                assert picks[t, :2].tolist() == p[:2] and rank[p[3:]].tolist() == [pk.NONE] * len(p[3:]), (key_set, k, f["size_of"][t])
            got = f["gen"].pick(arr, ky, va.PickShape(k, 1), target=tg, n_targets=f["n_targets"], rank=True)
            same(got, pk.boundary_expected(n_contigs, key_set, order, k, 1))
            for t, p in planted.items():   # spacing 1: only the '-' whose cut IS the first's conflicts (their positions are 11 apart)
                assert got[0][t, :3].tolist() == p[:3] and got[2][p[3:]].tolist() == [pk.NONE] * len(p[3:]), (key_set, k, f["size_of"][t])


# ---- one wave takes a large, a small and a large target in turn -------------------------------------------------------------
def test_large_small_large_in_one_wave(ctx):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n_waves = cus * wc.GROUPS_PER_CU * wc.WAVES_PER_GROUP
    f = pk.same_wave(n_waves)
    assert f["n_targets"] == 2 * n_waves + 3   # the launch is capped: wave w takes the targets w, w + n_waves, w + 2 n_waves
    assert pk.same_wave_floors(n_waves) == [True, False, True, False, True, False]   # memory, register, memory; register, memory, register
    want = pk.same_wave_expected(n_waves)
    gen = ctx.load_genome(va.PackedGenome.from_sequences(["ACGT" * (f["lens"][0] // 4)]))
    try:
        got = gen.pick(pk.loci_array(f["loci"], va.LOCUS_DTYPE), np.array(f["key"], dtype=np.uint64), va.PickShape(pk.SAME_WAVE_K, pk.SAME_WAVE_SPACING),
                       target=np.array(f["target"], dtype=np.uint32), n_targets=f["n_targets"], rank=True)
        same(got, want)
        assert got[3]["targets_picked"] == f["n_targets"]
    finally:
        gen.close()


# ---- beyond one launch ------------------------------------------------------------------------------------------------------
TILE = 1024  # candidates per tile of the `picked` passes (vsc_pick_device.h: kPickTile)


def launch_waves():
    return torch.cuda.get_device_properties(0).multi_processor_count * wc.GROUPS_PER_CU * wc.WAVES_PER_GROUP


def same_arrays(got, want):
    assert got[0].dtype == np.uint32 and got[0].shape == want[0].shape and np.array_equal(got[0], want[0])
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert {k: got[3][k] for k in want[3]} == want[3]


def test_more_candidates_than_a_launch_has_lanes_and_more_tiles_than_waves(ctx, small):
    W, k = launch_waves(), 4
    n = (W + 3) * TILE + 17
    idx, target, key, n_targets, block = pk.replicas(n)
    assert n > 64 * W and n_targets > 2 * W              # mark and scatter step twice; every wave of the select takes several targets
    assert n_targets * k > 64 * W                        # rank steps twice
    assert -(-n // TILE) > W and n % TILE                # more tiles than a launch has waves, the last one partial
    want = pk.replicas_expected(n, k, 20, block)
    loci = small["arr"][idx]
    codes = np.arange(n, dtype=np.uint64) * np.uint64(3)
    g = Guides.from_arrays(ctx, codes, loci)
    try:
        picks, counts, rank, stats, picked = g.pick(small["gen"], key, n_targets, va.PickShape(k, 20), target=target, picked=True)
        same_arrays((picks, counts, rank, stats), want)
        keep = np.flatnonzero(rank != pk.NONE)
        assert len(keep) == stats["picks"] == len(picked) > TILE   # a work list longer than the scan's 1024 threads
        pc, pl = picked.arrays()
        assert pc.tobytes() == codes[keep].tobytes() and pl.tobytes() == loci[keep].tobytes()
        picked.close()
    finally:
        g.close()


def test_permuted_candidates_beyond_one_launch(small):
    W, k = launch_waves(), 4
    n = 2 * 64 * W + 77
    idx, target, key, n_targets, block = pk.replicas(n, distinct=True)   # no target has two equal keys: no index decides
    order = np.random.default_rng(23).permutation(n)
    assert n > 64 * W and n_targets > 2 * W
    t = target[order]
    assert ((t[1:] == t[:-1]) & (t[1:] != pk.NONE)).mean() < 0.01         # hardly a run of equal targets is left
    want = pk.permuted(pk.replicas_expected(n, k, 20, block), order)
    got = small["gen"].pick(small["arr"][idx][order], key[order], va.PickShape(k, 20), target=target[order], n_targets=n_targets, rank=True)
    same_arrays(got, want)


# ---- pattern forms --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern,cut", [("N" * 21 + "NNGRRT", 18), ("TTTV" + "N" * 23, 22)])
def test_pattern_forms(ctx, small, pattern, cut):
    L = len(pattern)
    loci = pk.enumerate_pattern(small["contigs"], pattern)
    assert len(loci) > 100
    target = pk.targets_of(small["lens"], small["intervals"], "inside", small["groups"], loci)
    rng = np.random.default_rng(L + cut)
    key = [int(x) for x in rng.integers(0, 16, len(loci))]
    g = Guides.from_arrays(ctx, np.zeros(len(loci), dtype=np.uint64), pk.loci_array(loci, va.LOCUS_DTYPE), pattern=True)
    try:
        for k, spacing in ((4, 20), (32, 1), (3, 0)):
            want = pk.pick(small["lens"], loci, target, key, 14, k, spacing, site_len=L, cut=cut)
            # (a site of 27 bases can start where it no longer fits its contig's end with 23: those are in the fixture)
            got = g.pick(small["gen"], np.array(key, dtype=np.uint64), 14, va.PickShape(k, spacing, site_len=L, cut=cut),
                         regions=small["regions"], group=small["gr"])
            same(got, want)
        found = va.api.PatternGuides(pattern, (0, 21) if pattern.startswith("N") else (4, 23), np.zeros(len(loci), dtype=np.uint64),
                                     pk.loci_array(loci, va.LOCUS_DTYPE))
        got = small["gen"].pick(found, np.array(key, dtype=np.uint64), va.PickShape(4, 20, site_len=L, cut=cut), regions=small["regions"],
                                groups=small["gr"], rank=True)
        same(got, pk.pick(small["lens"], loci, target, key, 14, 4, 20, site_len=L, cut=cut))
    finally:
        g.close()


# ---- the picked object ----------------------------------------------------------------------------------------------------
def test_picked_object(ctx, small):
    found = small["gen"].enumerate_guides()
    codes, loci = found[0], found[1]
    assert [tuple(int(x) for x in (l["contig"], l["pos"], l["strand"])) for l in loci] == small["loci"]
    g = Guides.from_arrays(ctx, codes, loci)
    try:
        picks, counts, rank, stats, picked = g.pick(small["gen"], small["ky"]["high"], 14, va.PickShape(4, 20), regions=small["regions"],
                                                    group=small["gr"], picked=True)
        same((picks, counts, rank, stats), pk.small_expected("high", 4, 20))
        keep = np.flatnonzero(rank != pk.NONE)
        assert len(keep) == stats["picks"] == len(picked) > 30
        pc, pl = picked.arrays()
        assert np.array_equal(pc, codes[keep]) and pl.tobytes() == loci[keep].tobytes()
        # later calls take it: the microhomology pairs where it lies, a pick of the picked, and the searches by its codes
        pairs, _ = np.empty((len(picked), 2), dtype=np.uint32), None
        sh = va.MicrohomologyShape(flank=8)._struct()
        _lib.check(picked.fn["microhomology"](ctx._h, small["gen"]._h, picked.h, C.byref(sh), _lib.ptr(pairs), None), ctx._h)
        want_pairs, _ = small["gen"].microhomology(loci[keep], va.MicrohomologyShape(flank=8))
        assert np.array_equal(pairs, want_pairs)
        again = picked.pick(small["gen"], small["ky"]["high"][keep], 14, va.PickShape(1, 0), regions=small["regions"], group=small["gr"])
        want = pk.pick(small["lens"], [small["loci"][i] for i in keep], [small["target"][i] for i in keep],
                       [small["keys"]["high"][i] for i in keep], 14, 1, 0)
        same(again, want)
        rows = small["gen"].summarize(pc[:8], 2, exclude=pl[:8])
        assert np.array_equal(rows, small["gen"].summarize(codes[keep][:8], 2, exclude=loci[keep][:8]))
        as_pattern = "N" * 21 + "GG"
        _, prow = small["gen"].search_pattern(as_pattern, va.unpack_guides(pc[:8]), 1, records=False)
        _, want_prow = small["gen"].search_pattern(as_pattern, va.unpack_guides(codes[keep][:8]), 1, records=False)
        assert np.array_equal(prow, want_prow) and (prow[:, 0] >= 1).all()   # every picked guide finds its own site
        picked.close()
        # nothing eligible: an empty object
        none = g.pick(small["gen"], small["ky"]["ties"], 14, va.PickShape(4, 20, min_key=1 << 40), regions=small["regions"], group=small["gr"],
                      picked=True)
        assert len(none[4]) == 0 and none[3]["below_min_key"] == none[3]["below_min_key"] > 600 and (none[1] == 0).all()
        none[4].close()
    finally:
        g.close()


def test_host_only_object_goes_the_host_way(ctx, small):
    g = Guides.from_arrays(ctx, np.arange(len(small["arr"]), dtype=np.uint64), small["arr"], on_device=False)
    try:
        got = g.pick(small["gen"], small["ky"]["ties"], 14, va.PickShape(4, 20), regions=small["regions"], group=small["gr"], picked=True)
        same(got[:4], pk.small_expected("ties", 4, 20))
        pc, _ = got[4].arrays()
        assert np.array_equal(pc, np.flatnonzero(got[2] != pk.NONE).astype(np.uint64))
        got[4].close()
    finally:
        g.close()


# ---- shards, scratch, repeatability ------------------------------------------------------------------------------------------
def test_a_shard_at_both_ends(ctx, small):
    packed = small["packed"]
    sl = slice(3, packed.n_words - 1)
    part = va.Genome.from_shard(ctx, packed.hi[sl], packed.lo[sl], packed.nmask[sl], 3, sl.stop - sl.start, packed.contigs)
    try:
        got = part.pick(small["arr"], small["ky"]["ties"], va.PickShape(4, 20), regions=small["regions"], groups=small["gr"], rank=True)
        same(got, pk.small_expected("ties", 4, 20))
        got = part.pick(small["arr"], small["ky"]["ties"], va.PickShape(4, 20), target=small["tg"], n_targets=14, rank=True)
        same(got, pk.small_expected("ties", 4, 20))
    finally:
        part.close()


def test_release_scratch_between_alternating_shapes(ctx, small):
    for k, spacing in ((32, 1), (1, 0), (4, 20), (32, 1000)):
        ctx.release_scratch()
        got = small["gen"].pick(small["arr"], small["ky"]["ends"], va.PickShape(k, spacing), regions=small["regions"], groups=small["gr"], rank=True)
        same(got, pk.small_expected("ends", k, spacing))
        got = small["gen"].pick(small["arr"], small["ky"]["ends"], va.PickShape(k, spacing), target=small["tg"], n_targets=14, rank=True)
        same(got, pk.small_expected("ends", k, spacing))


def test_two_calls_in_a_row_are_byte_equal(small):
    a = small["gen"].pick(small["arr"], small["ky"]["ties"], va.PickShape(32, 20), target=small["tg"], n_targets=14, rank=True)
    b = small["gen"].pick(small["arr"], small["ky"]["ties"], va.PickShape(32, 20), target=small["tg"], n_targets=14, rank=True)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[:3], b[:3]))
    assert {k: v for k, v in a[3].items() if not k.endswith("_ms")} == {k: v for k, v in b[3].items() if not k.endswith("_ms")}
    assert a[3]["kernel_ms"] > 0 and a[3]["wall_ms"] >= a[3]["kernel_ms"] and len(a[3]["stage_ms"]) == 4


# ---- refusals -------------------------------------------------------------------------------------------------------------
def test_refusals(ctx, small):
    g = Guides.from_arrays(ctx, np.zeros(len(small["arr"]), dtype=np.uint64), small["arr"])
    other = va.Context(0)
    try:
        key, sh = small["ky"]["ties"], va.PickShape(4, 20)
        base = dict(regions=small["regions"], group=small["gr"])

        def refused(code, text, **kw):
            args = dict(base)
            args.update(kw)
            shape = args.pop("shape", sh)
            got, _, _ = g.pick_code(args.pop("gen", small["gen"]), args.pop("key", key), args.pop("n_targets", 14), shape, **args)
            assert got == code, (got, kw)
            assert text in va.lib().vsc_last_error(ctx._h).decode(), va.lib().vsc_last_error(ctx._h)

        for bad in (dict(site_len=15), dict(site_len=33), dict(cut=24), dict(k=0), dict(k=33)):
            p = dict(site_len=23, cut=17, k=4, spacing=0)
            p.update(bad)
            refused(-22, "site_len 16 .. 32", params=_lib.PickParams(p["site_len"], p["cut"], p["k"], p["spacing"], 0, 0))
        refused(-22, "reserved", params=_lib.PickParams(23, 17, 4, 0, 0, 1))
        refused(-22, "site_len must be 23", shape=va.PickShape(4, 20, site_len=24))
        refused(-22, "null argument", key=None)
        refused(-22, "null argument", gen_h=False)
        refused(-22, "exactly one of regions and target", target=small["tg"])
        refused(-22, "exactly one of regions and target", regions=None, group=None)
        refused(-22, "a group needs regions", regions=None, target=small["tg"])
        bad_group = small["gr"].copy()
        bad_group[7] = 14
        refused(-22, "a group entry", group=bad_group)
        ok_group = small["gr"].copy()
        ok_group[7] = pk.NONE
        assert g.pick_code(small["gen"], key, 14, sh, regions=small["regions"], group=ok_group)[0] == 0
        elsewhere = va.Regions(va.PackedGenome.from_sequences(["ACGT" * 50]), [(0, 0, 100)])
        refused(-22, "another contig table", regions=elsewhere, group=None)
        other_gen = other.load_genome(small["packed"])
        refused(-22, "genome belongs to another context", gen=other_gen)
        # candidates of another context (with a genome of this one), and the same refusals of vsc_pattern_guides_pick
        for pattern in (False, True):
            foreign = Guides.from_arrays(other, np.zeros(len(small["arr"]), dtype=np.uint64), small["arr"], pattern=pattern)
            foreign.ctx = ctx  # (the call is made on this context)
            assert foreign.pick_code(small["gen"], key, 14, sh, **base)[0] == -22
            assert "the candidates belong to another context" in va.lib().vsc_last_error(ctx._h).decode()
            foreign.ctx = other
            foreign.close()
        other_gen.close()
        pg = Guides.from_arrays(ctx, np.zeros(len(small["arr"]), dtype=np.uint64), small["arr"], pattern=True)
        try:
            for kw, text in ((dict(params=_lib.PickParams(15, 0, 4, 0, 0, 0)), "site_len 16 .. 32"), (dict(params=_lib.PickParams(23, 17, 33, 0, 0, 0)), "k 1 .. 32"),
                             (dict(params=_lib.PickParams(23, 17, 4, 0, 0, 9)), "reserved"), (dict(key=None), "null argument"),
                             (dict(gen_h=False), "null argument"), (dict(target=small["tg"]), "exactly one of regions and target"),
                             (dict(regions=None, group=None), "exactly one of regions and target"),
                             (dict(regions=None, target=small["tg"]), "a group needs regions"), (dict(group=bad_group), "a group entry"),
                             (dict(regions=elsewhere, group=None), "another contig table")):
                args = dict(base)
                args.update(kw)
                code, _, _ = pg.pick_code(small["gen"] , args.pop("key", key), 14, sh, **args)
                assert code == -22 and text in va.lib().vsc_last_error(ctx._h).decode(), (kw, code, va.lib().vsc_last_error(ctx._h))
            assert pg.pick_code(small["gen"], key, 14, va.PickShape(4, 20, site_len=24), **base)[0] == 0   # the caller vouches for site_len
        finally:
            pg.close()
        elsewhere.close()
        # loci: NULL arrays and the empty call
        L = va.lib()
        st = _lib.PickStats()
        p = sh._struct()
        picks, counts = np.full((14, 4), 5, dtype=np.uint32), np.full(14, 5, dtype=np.uint32)
        assert L.vsc_loci_pick(ctx._h, small["gen"]._h, None, 5, _lib.ptr(small["tg"]), _lib.ptr(key), 14, C.byref(p), _lib.ptr(picks),
                               _lib.ptr(counts), None, C.byref(st)) == -22
        assert L.vsc_loci_pick(ctx._h, small["gen"]._h, _lib.ptr(small["arr"]), 0xFFFFFFFF, _lib.ptr(small["tg"]), _lib.ptr(key), 14, C.byref(p),
                               _lib.ptr(picks), _lib.ptr(counts), None, C.byref(st)) == -34
        assert L.vsc_loci_pick(ctx._h, small["gen"]._h, None, 0, None, None, 14, C.byref(p), _lib.ptr(picks), _lib.ptr(counts), None,
                               C.byref(st)) == 0
        assert (counts == 0).all() and (picks == pk.NONE).all()
        # a refusal writes nothing, an empty call included; vsc_loci_pick_regions refuses as the others do
        picks[:], counts[:] = 5, 5
        empty = Guides.from_arrays(ctx, np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=va.LOCUS_DTYPE))
        assert empty.fn["pick"](ctx._h, small["gen"]._h, empty.h, small["regions"]._h, _lib.ptr(bad_group), None, 14, None, C.byref(p),
                                _lib.ptr(picks), _lib.ptr(counts), None, None, None) == -22
        assert (picks == 5).all() and (counts == 5).all()
        empty.close()
        R = lambda regions, group, n=len(small["arr"]), lo=small["arr"]: L.vsc_loci_pick_regions(  # noqa: E731
            ctx._h, small["gen"]._h, _lib.ptr(lo) if lo is not None else None, n, regions._h if regions is not None else None,
            _lib.ptr(group) if group is not None else None, _lib.ptr(key), 14, C.byref(p), _lib.ptr(picks), _lib.ptr(counts), None, C.byref(st))
        assert R(None, None) == -22 and R(small["regions"], bad_group) == -22 and R(small["regions"], None, lo=None) == -22
        assert R(small["regions"], small["gr"], n=0xFFFFFFFF) == -34
        assert (picks == 5).all() and (counts == 5).all()
        assert R(small["regions"], small["gr"]) == 0
        assert np.array_equal(picks, pk.as_arrays(pk.small_expected("ties", 4, 20))[0])
    finally:
        g.close()
        other.close()


# ---- design ---------------------------------------------------------------------------------------------------------------
def test_design_with_pick(small):
    regions, gen = small["regions"], small["gen"]
    plain = gen.design(regions, 2, microhomology=va.MicrohomologyShape(flank=8))
    out = gen.design(regions, 2, microhomology=va.MicrohomologyShape(flank=8), pick=va.PickShape(4, 20), pick_by=["oof", "mit"],
                     pick_groups=small["gr"])
    assert len(out) == len(plain) + 2 and all(np.array_equal(a, b) for a, b in zip(out[:len(plain)], plain))
    codes, loci, rows, pairs, picks, counts = out
    spec = np.array([va.mit_specificity(x) for x in rows["mit_sum"]])
    key = va.pick_key([va.pick_column("oof", pairs), va.pick_column("mit", spec)], [10, 14])
    tuples = [(int(l["contig"]), int(l["pos"]), int(l["strand"])) for l in loci]
    target = pk.targets_of(small["lens"], small["intervals"], "inside", small["groups"], tuples)
    want = pk.as_arrays(pk.pick(small["lens"], tuples, target, [int(x) for x in key], 14, 4, 20))
    assert np.array_equal(picks, want[0]) and np.array_equal(counts, want[1]) and counts.sum() > 30
    with pytest.raises(ValueError):
        gen.design(regions, 2, pick=va.PickShape(4, 20), pick_by=["eff"])
    with pytest.raises(ValueError):
        gen.design(regions, 2, pick_by=["mit"])


def test_design_pattern_with_pick(small):
    pattern, proto, cut = "N" * 21 + "NNGRRT", (0, 21), 18
    mh = va.MicrohomologyShape(27, cut, 8)
    plain = small["gen"].design_pattern(pattern, proto, 1, targets=small["intervals"], rule="inside", microhomology=mh)
    out = small["gen"].design_pattern(pattern, proto, 1, targets=small["intervals"], rule="inside", microhomology=mh,
                                      pick=va.PickShape(3, 15, site_len=27, cut=cut), pick_by=["oof", "mh"], pick_groups=small["gr"])
    assert len(out) == len(plain) + 2 and all(np.array_equal(a, b) for a, b in zip(out[1:len(plain)], plain[1:]))
    found, _, pairs, picks, counts = out
    tuples = [(int(l["contig"]), int(l["pos"]), int(l["strand"])) for l in found.loci]
    assert len(tuples) > 50
    key = va.pick_key([va.pick_column("oof", pairs), va.pick_column("mh", pairs)], [10, 20])
    target = pk.targets_of(small["lens"], small["intervals"], "inside", small["groups"], tuples)
    want = pk.as_arrays(pk.pick(small["lens"], tuples, target, [int(x) for x in key], 14, 3, 15, site_len=27, cut=cut))
    assert np.array_equal(picks, want[0]) and np.array_equal(counts, want[1]) and counts.sum() > 10
    for bad in (dict(pick=va.PickShape(3, 15, site_len=23, cut=17), pick_by=["oof"]),   # not the pattern's length
                dict(pick=va.PickShape(3, 15, site_len=27, cut=cut)),                    # the default column, table, needs table=
                dict(pick=va.PickShape(3, 15, site_len=27, cut=cut), pick_by=["eff"]), dict(pick_by=["oof"])):
        with pytest.raises(ValueError):
            small["gen"].design_pattern(pattern, proto, 1, targets=small["intervals"], rule="inside", microhomology=mh, **bad)


def test_both_tools_end_to_end(ctx, small, tmp_path):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    run = lambda *a: subprocess.run([os.path.join(root, "varscot_amd", "bin", a[0])] + [str(x) for x in a[1:]], capture_output=True,  # noqa: E731
                                    text=True, timeout=300)
    with open(tmp_path / "g.fa", "w") as fa:
        for i, s in enumerate(small["contigs"]):
            fa.write(">c%d\n%s\n" % (i, s))
    assert run("bidir_index", "-G", tmp_path / "g.fa", "-I", tmp_path / "idx").returncode == 0
    (tmp_path / "t.bed").write_text("".join("c%d\t%d\t%d\tgene%d\n" % (c, a, b, g) for (c, a, b), g in zip(small["intervals"], small["groups"])))
    gen, regions = small["gen"], small["regions"]

    def marks(loci, target, key, n_targets, names, **shape):
        picks, counts, _, _ = pk.pick(small["lens"], loci, target, key, n_targets, 4, 20, **shape)
        out = ["\tNA\tNA"] * len(loci)
        for t in range(n_targets):
            for r in range(counts[t]):
                out[picks[t][r]] = "\t%s\t%d" % (names[t], r)
        return out

    # guide_summary -E -L -k: ranked by rint(100 x mitSpecScore), per interval and per BED name
    codes, loci, rows = gen.design(regions, 2)
    tuples = [(int(l["contig"]), int(l["pos"]), int(l["strand"])) for l in loci]
    key = [int(x) for x in va.pick_column("mit", [va.mit_specificity(x) for x in rows["mit_sum"]])]
    base = ("guide_summary", "-G", tmp_path / "g.fa", "-I", tmp_path / "idx", "-M", "2", "-E", tmp_path / "t.bed")
    r = run(*base, "-L", tmp_path / "plain.bed", "-O", tmp_path / "plain.tsv")
    assert r.returncode == 0, r.stderr
    plain = (tmp_path / "plain.bed").read_text().splitlines()
    assert len(plain) == len(tuples) > 600
    labels = pk.targets_of(small["lens"], small["intervals"], "inside", None, tuples)
    by_name = pk.targets_of(small["lens"], small["intervals"], "inside", small["groups"], tuples)
    for extra, target, n_targets, names in ((("-k", "4,20"), labels, 44, [str(i) for i in range(44)]),
                                            (("-k", "4,20", "-c", "interval", "-b", "mit"), labels, 44, [str(i) for i in range(44)]),
                                            (("-k", "4,20", "-c", "name"), by_name, 14, ["gene%d" % g for g in range(14)])):
        r = run(*base, "-L", tmp_path / "k.bed", "-O", tmp_path / "k.tsv", *extra)
        assert r.returncode == 0, r.stderr
        want = [ln + m for ln, m in zip(plain, marks(tuples, target, key, n_targets, names))]
        assert (tmp_path / "k.bed").read_text().splitlines() == want              # no line is dropped
        assert sum(1 for ln in want if not ln.endswith("\tNA\tNA")) > 30
        assert (tmp_path / "k.tsv").read_bytes() == (tmp_path / "plain.tsv").read_bytes()

    # pattern_search -E -B -k -b oof,mh -H: SaCas9, the break 3 bases in front of the PAM
    pattern, proto, cut = "N" * 21 + "NNGRRT", (0, 21), 18
    found, pairs = gen.enumerate_pattern(pattern, proto, targets=small["intervals"], rule="inside", microhomology=va.MicrohomologyShape(27, cut, 8))
    ptuples = [(int(l["contig"]), int(l["pos"]), int(l["strand"])) for l in found.loci]
    pkey = [int(x) for x in va.pick_key([va.pick_column("oof", pairs), va.pick_column("mh", pairs)], [10, 20])]
    pbase = ("pattern_search", "-i", tmp_path / "idx", "-q", pattern, "-p", "0,21", "-B", tmp_path / "t.bed", "-r", "inside", "-H", "8")
    r = run(*pbase, "-E", tmp_path / "pe.tsv")
    assert r.returncode == 0, r.stderr + r.stdout
    pe = (tmp_path / "pe.tsv").read_text().splitlines()
    assert len(pe) == len(ptuples) + 1 > 50
    for extra, groups, n_targets, names in ((("-c", "interval"), None, 44, [str(i) for i in range(44)]),
                                            (("-c", "name"), small["groups"], 14, ["gene%d" % g for g in range(14)])):
        r = run(*pbase, "-E", tmp_path / "pk.tsv", "-k", "4,20", "-b", "oof,mh", *extra)
        assert r.returncode == 0, r.stderr + r.stdout
        target = pk.targets_of(small["lens"], small["intervals"], "inside", groups, ptuples)
        want = [pe[0] + "\tpickTarget\tpickRank"] + [ln + m for ln, m in zip(pe[1:], marks(ptuples, target, pkey, n_targets, names, site_len=27, cut=cut))]
        assert (tmp_path / "pk.tsv").read_text().splitlines() == want
        assert sum(1 for ln in want[1:] if not ln.endswith("\tNA\tNA")) > 10
