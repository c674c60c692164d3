"""tests/wide_cases.py without a device: on a miniature of the wide genome - 43 tiles cut into 4 runs - the output composed
from the islands equals each restatement run on the whole text, for all five calls; the size chosen for a 256-CU device is
what the wide tests need; and at that size the expected output has something at every place the layout is built for."""
import pytest

import bulges_cases as bc
import enumerate_cases as ec
import pattern_bulge_cases as pb
import pattern_cases as pc
import pattern_enum_cases as pe
import regions_cases as rc
import wide_cases as wc

MINI_TILES, MINI_WAVES = 43, 4


@pytest.fixture(scope="module")
def mini():
    s = wc.shape(MINI_TILES, MINI_WAVES)
    assert s["per"] == 11 and s["working"] == 4 and 0 < s["last_run"] < s["per"]
    return wc.layout(MINI_TILES, s["per"])


def text_of(lay, texts):
    contigs = [c.decode() for c in wc.contigs_of(lay, texts)]
    total = sum(len(c) + 1 for c in contigs)
    assert (lay["n_tiles"] - 1) * wc.TILE < total <= lay["n_tiles"] * wc.TILE and 80_000 < total < 90_000
    assert [len(c) for c in contigs] == lay["lens"]
    assert lay["off"] == [0, len(contigs[0]) + 1, len(contigs[0]) + len(contigs[1]) + 2]  # one separator behind every contig
    return contigs


# ---- size -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cus", [256, 304, 64, 8, 600])
def test_size_for_a_device(cus):
    s = wc.size_for(cus)
    W = cus * 32
    assert s["W"] == W and s["waves"] == W and s["n_tiles"] > max(32768, 2 * W) and s["n_tiles"] - max(32768, 2 * W) < 64
    assert s["per"] == -(-s["n_tiles"] // W) >= 3
    assert s["n_tiles"] % 64 != 0
    assert (s["working"] - 1) * s["per"] < s["n_tiles"] < s["working"] * s["per"]  # the last working wave's run is partial
    assert s["working"] < W                                                          # a wave without a tile
    assert 2 * 64 * s["n_tiles"] / 4096 > 1024 and wc.groups_of(64, s["n_tiles"]) > 1024
    if cus == 256:
        assert s["per"] == 5 and 67_000_000 < s["n_tiles"] * wc.TILE < 70_000_000


def test_one_tile_per_wave_is_what_the_small_suites_run():
    s = wc.shape(4, 8192)
    assert s["per"] == 1 and s["waves"] == 4 and wc.groups_of(64, 4) == 1


# ---- the composition equals the restatement on the whole text ---------------------------------------------------------------
@pytest.mark.parametrize("preset", ["SaCas9", "Cas12a"])
def test_pattern_search_composes(mini, preset):
    f = wc.pattern_family(preset)
    contigs = text_of(mini, f["texts"])
    guides = f["guides"][:7]
    hits, n_cands = wc.expect_pattern(mini, f["texts"], f["pattern"], guides, 4)
    assert (hits, n_cands) == pc.brute_force(contigs, f["pattern"], guides, 4)
    assert len(hits) > 100 and {h[2] for h in hits} == {0, 1, 2}


@pytest.mark.parametrize("preset,dna,rna", [("SaCas9", 2, 2), ("Cas12a", 1, 1)])
def test_pattern_bulge_search_composes(mini, preset, dna, rna):
    f = wc.pattern_family(preset)
    contigs = text_of(mini, f["texts"])
    guides = f["guides"][:7]
    hits, n_cands = wc.expect_pattern_bulges(mini, f["texts"], f["pattern"], guides, f["proto"], 4, dna, rna)
    assert (hits, n_cands) == pb.brute_force(contigs, f["pattern"], guides, f["proto"], 4, dna, rna)
    assert len(hits) > 100 and {h[2] for h in hits} == {0, 1, 2} and {h[4] for h in hits} == set(pb.enabled(dna, rna))


def test_the_rosters_compose_with_all_their_guides(mini):
    f = wc.pattern_family("SaCas9")
    contigs = text_of(mini, f["texts"])
    assert len(f["guides"]) == 70
    assert wc.expect_pattern(mini, f["texts"], f["pattern"], f["guides"], 3) == pc.brute_force(contigs, f["pattern"], f["guides"], 3)
    got = wc.expect_pattern_bulges(mini, f["texts"], f["pattern"], f["guides"], f["proto"], 3, 1, 1)
    assert got == pb.brute_force(contigs, f["pattern"], f["guides"], f["proto"], 3, 1, 1)


def test_bulge_search_composes(mini):
    f = wc.reads_family()
    contigs = text_of(mini, f["texts"])
    hits, n_cands = wc.expect_bulges(mini, f["texts"], f["guides"], 4, 2, 2)
    cands = bc.candidates(contigs, 2, 2)
    assert n_cands == len(cands) and hits == bc.brute_force(contigs, f["guides"], 4, 2, 2, cands=cands)
    assert len(hits) > 100 and {h[2] for h in hits} == {0, 1, 2} and {h[4] for h in hits} == set(bc.CLASSES)


@pytest.mark.parametrize("rule", [None, "overlap", "inside"])
def test_enumeration_composes(mini, rule):
    f = wc.reads_family()
    contigs = text_of(mini, f["texts"])
    targets = wc.targets_of(mini, f["texts"], 0) if rule else None
    member = rc.brute_force(targets, mini["lens"])[rule] if rule else None
    everything = ec.brute_force(contigs)
    for kw in ({}, dict(gc=(8, 14), max_t_run=3, strands="-")):
        want = ec.brute_force(contigs, member=member, **kw)
        assert wc.expect_enumerate(mini, f["texts"], targets, rule or "overlap", **kw) == want
        assert 0 < len(want) and (len(want) < len(everything) or (rule is None and not kw))


@pytest.mark.parametrize("rule", [None, "overlap", "inside"])
def test_pattern_enumeration_composes(mini, rule):
    f = wc.pattern_family("SaCas9")
    contigs = text_of(mini, f["texts"])
    L = len(f["pattern"])
    targets = wc.targets_of(mini, f["texts"], 0) if rule else None
    cands = pe.candidates(contigs, f["pattern"])
    for kw in ({}, dict(gc=(9, 12), max_t_run=2)):
        want = pe.kept(cands, contigs, L, f["proto"], targets=targets, rule=rule or "overlap", **kw)
        assert wc.expect_enumerate_pattern(mini, f["texts"], f["pattern"], f["proto"], targets, rule or "overlap", **kw) == want
        assert 0 < len(want) and (len(want) < len(cands) or (rule is None and not kw))


def test_targets_cover_cut_and_miss(mini):
    f = wc.reads_family()
    targets = wc.targets_of(mini, f["texts"], 0)
    spots = wc.placed(mini, f["texts"])
    inside = lambda c, p, n, t: t[0] == c and t[1] <= p and p + n <= min(t[2], mini["lens"][c])
    touches = lambda c, p, n, t: t[0] == c and t[1] < p + n and p < min(t[2], mini["lens"][c])
    whole = [s for s in spots if any(inside(s[0], s[1], len(s[2]), t) for t in targets)]
    cut = [s for s in spots if s not in whole and any(touches(s[0], s[1], len(s[2]), t) for t in targets)]
    in_n = [t for t in targets if not any(touches(s[0], s[1], len(s[2]), t) for s in spots)]
    assert whole and len(cut) >= 3 and len(in_n) >= 2


# ---- the floors at the size of a 256-CU device --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wide():
    s = wc.size_for(256)
    assert s["W"] == 8192
    return s, wc.layout(s["n_tiles"], s["per"])


def test_layout_at_full_width(wide):
    s, lay = wide
    total = sum(n + 1 for n in lay["lens"])
    assert -(-(-(-total // 32)) // 64) == s["n_tiles"]  # ceil(ceil(total / 32) words / 64): the tiles of the packed planes
    assert len(lay["lens"]) == 3 and min(lay["lens"]) > 10 * wc.TILE
    first_of_1 = lay["off"][1] // wc.TILE
    assert first_of_1 // s["per"] == (lay["off"][1] - 2) // wc.TILE // s["per"]  # contig 0 ends and contig 1 starts in one wave's run


def test_floors_of_the_searches_at_full_width(wide):
    s, lay = wide
    f = wc.pattern_family("SaCas9")
    L = len(f["pattern"])
    hits, _ = wc.expect_pattern(lay, f["texts"], f["pattern"], f["guides"], 3)
    wc.placement_floors(lay, s["W"], [(h[2], h[3], L) for h in hits], [(h[0], h[1]) for h in hits])
    assert {h[4] for h in hits if h[1] == 0} == {h[4] for h in hits if h[1] == 1} == {0, 1, 2, 3}
    hits, _ = wc.expect_pattern_bulges(lay, f["texts"], f["pattern"], f["guides"], f["proto"], 3, 1, 1)
    wc.placement_floors(lay, s["W"], [(h[2], h[3], L + h[4]) for h in hits], [(h[0], h[1]) for h in hits])
    r = wc.reads_family()
    hits, _ = wc.expect_bulges(lay, r["texts"], r["guides"], 4, 2, 2)
    wc.placement_floors(lay, s["W"], [(h[2], h[3], bc.READ_LEN + h[4]) for h in hits], [(h[0], h[1]) for h in hits])
    for d in bc.CLASSES:  # (the edge scenario keeps some of its planted sites in another contig than the body)
        assert {h[5] for h in hits if h[4] == d} == set(range(5)), d
        for strand in (0, 1):
            assert len({h[5] for h in hits if h[4] == d and h[1] == strand}) >= 4, (d, strand)


@pytest.mark.parametrize("cus", [304, 600, 64])
def test_floors_hold_for_other_devices(cus):
    """Runs of 4 and 3 tiles (304 and 600 CUs) and of 17 (64 CUs): the layout follows the runs."""
    s = wc.size_for(cus)
    assert s["per"] == {304: 4, 600: 3, 64: 17}[cus]
    lay = wc.layout(s["n_tiles"], s["per"])
    f = wc.pattern_family("Cas12a")
    hits, _ = wc.expect_pattern(lay, f["texts"], f["pattern"], f["guides"][:7], 4)
    wc.placement_floors(lay, s["W"], [(h[2], h[3], len(f["pattern"])) for h in hits], [(h[0], h[1]) for h in hits])
    r = wc.reads_family()
    wc.placement_floors(lay, s["W"], [(x[0], x[1], ec.WINDOW) for x in wc.expect_enumerate(lay, r["texts"])])


def test_floors_of_the_enumerations_at_full_width(wide):
    s, lay = wide
    r = wc.reads_family()
    wc.placement_floors(lay, s["W"], [(x[0], x[1], ec.WINDOW) for x in wc.expect_enumerate(lay, r["texts"])])
    f = wc.pattern_family("SaCas9")
    found = wc.expect_enumerate_pattern(lay, f["texts"], f["pattern"], f["proto"])
    wc.placement_floors(lay, s["W"], [(x[0], x[1], len(f["pattern"])) for x in found])
    assert {x[2] for x in found} == {0, 1}
