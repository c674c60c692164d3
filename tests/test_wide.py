"""The count / scan / write searches on a genome of more tiles than the launch has waves (tests/wide_cases.py): records, rows,
codes and loci byte for byte what the restatements give for the islands, where a wave takes a run of several tiles (the
hand-offs between tiles, empty tiles, the contig cache, partial and empty runs), a round has more than 1 024 groups of cells
(group offsets, chunk sums from a chunk that is not the first, rows that end inside a chunk), the one-workgroup scan walks
several entries per thread, and a shard of many tiles starts behind position 0."""
import numpy as np
import pytest
import torch

import varscot_amd as va
import bulges_cases as bc
import enumerate_cases as ec
import pattern_bulge_cases as pb
import pattern_cases as pc
import pattern_enum_cases as pe
import wide_cases as wc

pytestmark = pytest.mark.gpu

TILE_BYTES = 64 * 3 * 4  # genome_bytes of one pass over one tile
N_ONLY_TILES = 1100      # the target that lies in N only: more tiles than the scan has threads


@pytest.fixture(scope="module")
def ctx():
    c = va.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def size():
    """The size for this device, derived and asserted."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    s = wc.size_for(cus)
    W, n = cus * 8 * 4, s["n_tiles"]
    assert s["W"] == W and n > max(32768, 2 * W) and n - max(32768, 2 * W) < 64
    per = -(-n // W)
    assert s["per"] == per >= 3                          # a wave's run has several tiles
    assert n % 64 != 0                                   # a (guide, strand) row ends inside a chunk
    working = -(-n // per)
    assert (working - 1) * per < n < working * per       # the last working wave has a partial run
    assert working < W                                   # and at least one wave has none
    assert 2 * 64 * n / 4096 > 1024 and wc.groups_of(64, n) > 1024  # a 64-guide round: more groups than the scan has threads
    return s


@pytest.fixture(scope="module")
def lay(size):
    return wc.layout(size["n_tiles"], size["per"])


def load(ctx, lay, texts):
    packed = va.PackedGenome.from_sequences(wc.contigs_of(lay, texts))
    assert (packed.n_words + 63) // 64 == lay["n_tiles"] and len(packed.contigs) >= 3
    assert [int(x) for x in packed.contigs["offset"]] == lay["off"] and [int(x) for x in packed.contigs["length"]] == lay["lens"]
    return packed, ctx.load_genome(packed)


@pytest.fixture(scope="module")
def sa(ctx, lay):
    f = dict(wc.pattern_family("SaCas9"))
    f["packed"], f["gen"] = load(ctx, lay, f["texts"])
    yield f
    f["gen"].close()


@pytest.fixture(scope="module")
def cas12a(ctx, lay):
    f = dict(wc.pattern_family("Cas12a"))
    f["packed"], f["gen"] = load(ctx, lay, f["texts"])
    yield f
    f["gen"].close()


@pytest.fixture(scope="module")
def reads(ctx, lay):
    f = dict(wc.reads_family())
    f["packed"], f["gen"] = load(ctx, lay, f["texts"])
    yield f
    f["gen"].close()


@pytest.fixture(scope="module")
def sa_plain(lay, sa):
    """vsc_search_pattern, SaCas9, the 7 guides, m = 4: (hits, candidates, records, rows)."""
    hits, n_cands = wc.expect_pattern(lay, sa["texts"], sa["pattern"], sa["guides"][:7], 4)
    return (hits, n_cands) + pc.arrays(hits, 7)


@pytest.fixture(scope="module")
def sa_bulged(lay, sa):
    """vsc_search_pattern_bulges, SaCas9, the 7 guides, m = 4, dna = rna = 2."""
    hits, n_cands = wc.expect_pattern_bulges(lay, sa["texts"], sa["pattern"], sa["guides"][:7], sa["proto"], 4, 2, 2)
    return (hits, n_cands) + pb.arrays(hits, 7)


@pytest.fixture(scope="module")
def reads_bulged(lay, reads):
    """vsc_search_bulges, the 20 reads, m = 4, dna = rna = 2."""
    hits, n_cands = wc.expect_bulges(lay, reads["texts"], reads["guides"], 4, 2, 2)
    return (hits, n_cands) + bc.arrays(hits, len(reads["guides"]))


def same(got, rec, rows):
    assert got[0].dtype == rec.dtype and len(got[0]) == len(rec) and got[0].tobytes() == rec.tobytes()
    assert got[1].dtype == np.uint32 and got[1].shape == rows.shape and got[1].tobytes() == rows.tobytes()


def same_guides(got, arrays):
    codes, loci = arrays
    assert got[0].dtype == np.uint64 and got[1].dtype == va.LOCUS_DTYPE
    assert len(got[0]) == len(codes) and got[0].tobytes() == codes.tobytes() and got[1].tobytes() == loci.tobytes()


def work_tiles(ctx):
    """The tiles of the last enumeration's work list, from what it read."""
    t = ctx.timing()
    assert t["genome_bytes"] % (TILE_BYTES * t["passes"]) == 0
    return t["genome_bytes"] // (TILE_BYTES * t["passes"])


# ---- 1. vsc_search_pattern -------------------------------------------------------------------------------------------------
def test_search_pattern_sacas9(ctx, size, lay, sa, sa_plain):
    hits, n_cands, rec, rows = sa_plain
    wc.placement_floors(lay, size["W"], [(h[2], h[3], len(sa["pattern"])) for h in hits], [(h[0], h[1]) for h in hits])
    assert wc.groups_of(7, lay["n_tiles"]) > 1
    same(sa["gen"].search_pattern(sa["pattern"], sa["guides"][:7], 4), rec, rows)
    assert ctx.timing()["sites"] == n_cands and ctx.timing()["hits"] == len(hits)


def test_search_pattern_cas12a(ctx, size, lay, cas12a):
    f = cas12a
    hits, n_cands = wc.expect_pattern(lay, f["texts"], f["pattern"], f["guides"][:7], 4)
    wc.placement_floors(lay, size["W"], [(h[2], h[3], len(f["pattern"])) for h in hits], [(h[0], h[1]) for h in hits])
    same(f["gen"].search_pattern(f["pattern"], f["guides"][:7], 4), *pc.arrays(hits, 7))
    assert ctx.timing()["sites"] == n_cands


def test_search_pattern_seventy_guides(ctx, size, lay, sa):
    hits, n_cands = wc.expect_pattern(lay, sa["texts"], sa["pattern"], sa["guides"], 3)
    wc.placement_floors(lay, size["W"], [(h[2], h[3], len(sa["pattern"])) for h in hits], [(h[0], h[1]) for h in hits])
    assert len(sa["guides"]) == 70 and 2 * 64 * lay["n_tiles"] / 4096 > 1024  # the first round at guide_batch = 64: groups > 1 024
    rec, rows = pc.arrays(hits, 70)
    for batch, passes in ((64, 2), (0, 5)):
        same(sa["gen"].search_pattern(sa["pattern"], sa["guides"], 3, guide_batch=batch), rec, rows)
        assert ctx.timing()["passes"] == passes and ctx.timing()["sites"] == n_cands


def test_search_pattern_rows_and_records_alone(sa, sa_plain):
    _, _, rec, rows = sa_plain
    got = sa["gen"].search_pattern(sa["pattern"], sa["guides"][:7], 4, rows=False)
    assert got[1] is None and got[0].tobytes() == rec.tobytes()
    got = sa["gen"].search_pattern(sa["pattern"], sa["guides"][:7], 4, records=False)
    assert got[0] is None and got[1].tobytes() == rows.tobytes()


# ---- 2. vsc_search_pattern_bulges ------------------------------------------------------------------------------------------
def test_search_pattern_bulges_sacas9(ctx, size, lay, sa, sa_bulged):
    hits, n_cands, rec, rows = sa_bulged
    L = len(sa["pattern"])
    wc.placement_floors(lay, size["W"], [(h[2], h[3], L + h[4]) for h in hits], [(h[0], h[1]) for h in hits])
    for d in pb.CLASSES:
        for strand in (0, 1):
            assert {h[5] for h in hits if h[4] == d and h[1] == strand} == set(range(5)), (d, strand)  # the body's floor is kept
    same(sa["gen"].search_pattern_bulges(sa["pattern"], sa["guides"][:7], 4, sa["proto"], dna=2, rna=2), rec, rows)
    assert ctx.timing()["sites"] == n_cands and ctx.timing()["hits"] == len(hits)


def test_search_pattern_bulges_cas12a(ctx, size, lay, cas12a):
    f = cas12a
    hits, n_cands = wc.expect_pattern_bulges(lay, f["texts"], f["pattern"], f["guides"][:7], f["proto"], 4, 1, 1)
    wc.placement_floors(lay, size["W"], [(h[2], h[3], len(f["pattern"]) + h[4]) for h in hits], [(h[0], h[1]) for h in hits])
    same(f["gen"].search_pattern_bulges(f["pattern"], f["guides"][:7], 4, f["proto"], dna=1, rna=1), *pb.arrays(hits, 7))
    assert ctx.timing()["sites"] == n_cands


def test_search_pattern_bulges_round_of_sixty_four(ctx, size, lay, sa):
    hits, n_cands = wc.expect_pattern_bulges(lay, sa["texts"], sa["pattern"], sa["guides"], sa["proto"], 3, 1, 1)
    wc.placement_floors(lay, size["W"], [(h[2], h[3], len(sa["pattern"]) + h[4]) for h in hits], [(h[0], h[1]) for h in hits])
    assert wc.groups_of(64, lay["n_tiles"]) > 1024
    same(sa["gen"].search_pattern_bulges(sa["pattern"], sa["guides"], 3, sa["proto"], dna=1, rna=1, guide_batch=64), *pb.arrays(hits, 70))
    assert ctx.timing()["passes"] == 2 and ctx.timing()["sites"] == n_cands


# ---- 3. a pattern of N only: every island base is a candidate, the queue fills and refills tile after tile -------------------
def test_pattern_of_n_only(ctx, lay, sa):
    pattern, proto = "N" * 23, (0, 23)
    guides = [sa["guides"][0][:23], sa["guides"][7][:23]]
    assert all(g[:21].isalpha() and g[21:] == "NN" for g in guides)
    runs_of = lambda text: "".join(ch if ch in "ACGTacgt" else " " for ch in text).split()  # the stretches without N
    clean = sum(max(0, len(run) - 22) for _, _, text in wc.placed(lay, sa["texts"]) for run in runs_of(text))
    hits, n_cands = wc.expect_pattern(lay, sa["texts"], pattern, guides, 3)
    assert n_cands == 2 * clean and hits and {h[1] for h in hits} == {0, 1}  # every N-free window, both strands
    same(sa["gen"].search_pattern(pattern, guides, 3), *pc.arrays(hits, 2))
    assert ctx.timing()["sites"] == n_cands
    hits, n_cands = wc.expect_pattern_bulges(lay, sa["texts"], pattern, guides, proto, 3, 2, 2)
    assert n_cands > 7 * clean and {h[4] for h in hits} == set(pb.CLASSES) and {h[1] for h in hits} == {0, 1}
    same(sa["gen"].search_pattern_bulges(pattern, guides, 3, proto, dna=2, rna=2), *pb.arrays(hits, 2))
    assert ctx.timing()["sites"] == n_cands


# ---- 4. vsc_search_bulges ----------------------------------------------------------------------------------------------------
def test_search_bulges(ctx, size, lay, reads, reads_bulged):
    hits, n_cands, rec, rows = reads_bulged
    wc.placement_floors(lay, size["W"], [(h[2], h[3], bc.READ_LEN + h[4]) for h in hits], [(h[0], h[1]) for h in hits])
    n = len(reads["guides"])
    assert n == 20 and -(-2 * n * lay["n_tiles"] // 64) > 1024  # one round of 20: its chunks go straight into the scan
    for batch, passes in ((0, 2), (64, 1)):
        same(reads["gen"].search_bulges(reads["guides"], 4, dna=2, rna=2, guide_batch=batch), rec, rows)
        assert ctx.timing()["passes"] == passes and ctx.timing()["sites"] == n_cands


def test_pattern_bulges_equal_the_bulge_search(reads, reads_bulged):
    hits = [h for h in reads_bulged[0] if h[0] < 7]
    spelled = [bc.read_of(g) for g in reads["guides"][:7]]
    want = reads["gen"].search_bulges(spelled, 4, dna=2, rna=2)
    same(want, *bc.arrays(hits, 7))
    got = reads["gen"].search_pattern_bulges("N" * 21 + "GR", spelled, 4, (0, 20), dna=2, rna=2)
    assert len(want[0]) > 100 and got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()


# ---- 5. the enumerations -----------------------------------------------------------------------------------------------------
def test_enumerate_guides_everywhere(ctx, size, lay, reads):
    found = wc.expect_enumerate(lay, reads["texts"])
    wc.placement_floors(lay, size["W"], [(x[0], x[1], ec.WINDOW) for x in found])
    assert {x[2] for x in found} == {0, 1}
    same_guides(reads["gen"].enumerate_guides(), ec.arrays(found))
    assert work_tiles(ctx) == lay["n_tiles"] > 1024 and ctx.timing()["sites"] == len(found)
    kw = dict(gc=(8, 14), max_t_run=3, strands="-")
    kept = wc.expect_enumerate(lay, reads["texts"], **kw)
    assert 0 < len(kept) < len(found)
    same_guides(reads["gen"].enumerate_guides(**kw), ec.arrays(kept))


def test_enumerate_pattern_everywhere(ctx, size, lay, sa):
    found = wc.expect_enumerate_pattern(lay, sa["texts"], sa["pattern"], sa["proto"])
    wc.placement_floors(lay, size["W"], [(x[0], x[1], len(sa["pattern"])) for x in found])
    assert {x[2] for x in found} == {0, 1}
    got = sa["gen"].enumerate_pattern(sa["pattern"], sa["proto"])
    same_guides((got.codes, got.loci), pe.arrays(found))
    assert work_tiles(ctx) == lay["n_tiles"] > 1024 and ctx.timing()["sites"] == len(found)
    kw = dict(gc=(9, 12), max_t_run=2)
    kept = wc.expect_enumerate_pattern(lay, sa["texts"], sa["pattern"], sa["proto"], **kw)
    assert 0 < len(kept) < len(found)
    got = sa["gen"].enumerate_pattern(sa["pattern"], sa["proto"], **kw)
    same_guides((got.codes, got.loci), pe.arrays(kept))


def target_floors(lay, texts, targets, everything, over, ins):
    """Some islands are covered wholly, some are cut, some targets lie in N only - on the expected candidates themselves."""
    assert 0 < len(ins) < len(over) < len(everything)
    spots = wc.placed(lay, texts)
    of = lambda found, c, p, n: sum(1 for x in found if x[0] == c and p <= x[1] < p + n)
    kept = [(of(everything, c, p, len(t)), of(over, c, p, len(t))) for c, p, t in spots]
    assert any(a and a == b for a, b in kept) and sum(1 for a, b in kept if 0 < b < a) >= 3 and any(a and not b for a, b in kept)
    touches = lambda t: any(x[0] == t[0] and t[1] < x[1] + 64 and x[1] < t[2] for x in everything)
    assert sum(1 for t in targets if not touches(t)) >= 3


@pytest.mark.parametrize("rule", ["overlap", "inside"])
def test_enumerate_guides_in_regions(ctx, lay, reads, rule):
    targets = wc.targets_of(lay, reads["texts"], N_ONLY_TILES)
    everything = wc.expect_enumerate(lay, reads["texts"])
    found = wc.expect_enumerate(lay, reads["texts"], targets, rule)
    target_floors(lay, reads["texts"], targets, everything, wc.expect_enumerate(lay, reads["texts"], targets, "overlap"),
                  wc.expect_enumerate(lay, reads["texts"], targets, "inside"))
    reg = va.Regions(reads["packed"], targets, rule=rule)
    try:
        same_guides(reads["gen"].enumerate_guides(reg), ec.arrays(found))
        assert 1024 < work_tiles(ctx) < lay["n_tiles"] // 4 and ctx.timing()["sites"] == len(found)
    finally:
        reg.close()


@pytest.mark.parametrize("rule", ["overlap", "inside"])
def test_enumerate_pattern_in_targets(ctx, lay, sa, rule):
    targets = wc.targets_of(lay, sa["texts"], N_ONLY_TILES)
    args = (lay, sa["texts"], sa["pattern"], sa["proto"])
    found = wc.expect_enumerate_pattern(*args, targets, rule)
    target_floors(lay, sa["texts"], targets, wc.expect_enumerate_pattern(*args), wc.expect_enumerate_pattern(*args, targets, "overlap"),
                  wc.expect_enumerate_pattern(*args, targets, "inside"))
    got = sa["gen"].enumerate_pattern(sa["pattern"], sa["proto"], targets, rule=rule)
    same_guides((got.codes, got.loci), pe.arrays(found))
    assert 1024 < work_tiles(ctx) < lay["n_tiles"] // 4 and ctx.timing()["sites"] == len(found)


# ---- 6. shards: many tiles behind a first position that is not 0 --------------------------------------------------------------
WORLD = 3


def shards(ctx, size, f):
    """The family's genome as WORLD resident shards; every shard's launch gives a wave two tiles or more."""
    out = []
    for rank in range(WORLD):
        b, e = f["packed"].shard_words(rank, WORLD)
        assert b % 64 == 0 and (b > 0) == (rank > 0) and wc.shape(-(-(e - b) // 64), size["W"])["per"] >= 2
        out.append(ctx.load_genome(f["packed"], rank, WORLD))
    return out


def test_shards_of_the_pattern_searches_merge_to_the_whole(ctx, size, sa, sa_plain, sa_bulged):
    gens = shards(ctx, size, sa)
    try:
        for call, order, want in ((lambda g: g.search_pattern(sa["pattern"], sa["guides"][:7], 4), pc.merge_order, sa_plain),
                                  (lambda g: g.search_pattern_bulges(sa["pattern"], sa["guides"][:7], 4, sa["proto"], dna=2, rna=2),
                                   pb.merge_order, sa_bulged)):
            parts = [call(g) for g in gens]
            assert all(len(p[0]) > 0 for p in parts)
            merged = np.concatenate([p[0] for p in parts])
            merged = merged[order(merged)]
            assert merged.tobytes() == want[2].tobytes() and sum(p[1] for p in parts).astype(np.uint32).tobytes() == want[3].tobytes()
        found = wc.expect_enumerate_pattern(wc.layout(size["n_tiles"], size["per"]), sa["texts"], sa["pattern"], sa["proto"])
        parts = [g.enumerate_pattern(sa["pattern"], sa["proto"]) for g in gens]
        assert all(len(p.codes) > 0 for p in parts)
        same_guides((np.concatenate([p.codes for p in parts]), np.concatenate([p.loci for p in parts])), pe.arrays(found))
    finally:
        for g in gens:
            g.close()


def test_shards_of_the_read_searches_merge_to_the_whole(ctx, size, lay, reads, reads_bulged):
    gens = shards(ctx, size, reads)
    try:
        parts = [g.search_bulges(reads["guides"], 4, dna=2, rna=2) for g in gens]
        assert all(len(p[0]) > 0 for p in parts)
        merged = np.concatenate([p[0] for p in parts])
        merged = merged[bc.merge_order(merged)]
        assert merged.tobytes() == reads_bulged[2].tobytes()
        assert sum(p[1] for p in parts).astype(np.uint32).tobytes() == reads_bulged[3].tobytes()
        parts = [g.enumerate_guides() for g in gens]
        assert all(len(p[0]) > 0 for p in parts)
        same_guides((np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])),
                    ec.arrays(wc.expect_enumerate(lay, reads["texts"])))
    finally:
        for g in gens:
            g.close()


# ---- 7. repetition -------------------------------------------------------------------------------------------------------------
def test_second_call_returns_the_same_bytes(sa, reads, sa_plain, sa_bulged, reads_bulged):
    calls = ((lambda: sa["gen"].search_pattern(sa["pattern"], sa["guides"][:7], 4), sa_plain),
             (lambda: sa["gen"].search_pattern_bulges(sa["pattern"], sa["guides"][:7], 4, sa["proto"], dna=2, rna=2), sa_bulged),
             (lambda: reads["gen"].search_bulges(reads["guides"], 4, dna=2, rna=2), reads_bulged))
    for call, want in calls:
        a, b = call(), call()
        assert a[0].tobytes() == b[0].tobytes() == want[2].tobytes() and a[1].tobytes() == b[1].tobytes() == want[3].tobytes()
    a, b = reads["gen"].enumerate_guides(), reads["gen"].enumerate_guides()
    assert len(a[0]) and a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    a, b = (sa["gen"].enumerate_pattern(sa["pattern"], sa["proto"]) for _ in range(2))
    assert len(a.codes) and a.codes.tobytes() == b.codes.tobytes() and a.loci.tobytes() == b.loci.tobytes()
