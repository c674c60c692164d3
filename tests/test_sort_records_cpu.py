"""The cases of tests/sort_cases.py build what they claim - checked on the reference side alone, no device: unique keys, the
bins a level of the reported bin_bits leaves, how many contigs a bin's range touches, tiles per segment, and the reference's
own round trip pack -> sort -> unpack.  tests/test_sort_records.py runs the same cases on the device."""
import numpy as np
import pytest

import sort_cases as sc

U64 = np.uint64


def test_reference_round_trip():
    """pack -> np.sort -> unpack gives back (read, strand, position, mask) in (read, strand, position) order, contig and offset
    by the table; positions at both ends of 32 bits and every pos_bits / pos_base combination the cases use."""
    rng = np.random.default_rng(1)
    for pos_bits, pos_base, off in ((32, 0, [0, 100, 1 << 31, (1 << 32) - 24]), (12, (1 << 32) - 4096, [0, (1 << 32) - 4000, (1 << 32) - 1]),
                                    (1, 0, [0, 1]), (20, 0, [0, 5, 4000])):
        n = min(500, 1 << (pos_bits + 3))
        keys = sc.unique_keys(rng, n, pos_bits + 1 + 6)
        rel, strand, read = keys & U64((1 << pos_bits) - 1), (keys >> U64(pos_bits)) & U64(1), keys >> U64(pos_bits + 1)
        mask = rng.integers(0, sc.MASK23 + 1, size=n).astype(U64)
        recs = sc.pack(read, strand, rel + U64(pos_base), mask, pos_bits, pos_base)
        assert len(np.unique(recs >> U64(63))) == 1 and not (recs >> U64(62)).any()
        got = sc.unpack(np.sort(recs), 640, np.array(off, dtype=np.uint32), pos_bits, pos_base)
        order = np.lexsort((rel, strand, read))
        glob = (rel + U64(pos_base))[order].astype(np.int64)
        contig = np.searchsorted(np.array(off, dtype=np.int64), glob, "right") - 1
        assert np.array_equal(got["guide"], 640 + read[order].astype(np.int64))
        assert np.array_equal(got["contig"], contig) and np.array_equal(got["pos"], glob - np.array(off, dtype=np.int64)[contig])
        assert np.array_equal(got["info"] >> 31, strand[order]) and np.array_equal(got["info"] & sc.MASK23, mask[order])
        assert np.array_equal((got["info"] >> 23) & 0xFF, [bin(int(m)).count("1") for m in mask[order]])
    assert sc.popcount(np.array([0, 1, sc.MASK23, 0x555555], dtype=np.uint32)).tolist() == [0, 1, 23, 12]


def test_model_restates_the_level_rule():
    assert sc.sort_limits({}) == (8064, 11, 10080) and sc.sort_limits(dict(sort_cap=512)) == (512, 11, 640)
    assert sc.sort_limits(dict(sort_cap=16, sort_max_bits=1)) == (16, 1, 32)
    assert sc.level_bits(8064, 8064, 11, 27, 3) == 0 and sc.level_bits(8065, 8064, 11, 27, 3) == 1
    assert sc.level_bits(24581, 512, 11, 27, 12) == 7 and sc.level_bits(10 ** 6, 16, 11, 5, 1) == 5


@pytest.mark.parametrize("layout", sc.TILE_LAYOUTS)
@pytest.mark.parametrize("order", list(sc.SEGMENT_ORDERS))
def test_case_1_tiles_and_segments(order, layout):
    c = sc.tiles_case(order, layout)  # (check_built: the records it was made of, unique keys)
    n_in = c.segments["n_slots"].tolist()
    assert set(n_in) == set(sc.SEGMENT_SIZES)
    assert c.tiles() == [(n + 8191) // 8192 for n in n_in] and {1, 2, 4} == set(c.tiles())
    big = [i for i, n in enumerate(n_in) if n > 8000]
    assert any(n_in[i + 1] == 1 and i + 2 in big for i in big[:-1]), "a single-record segment between two large ones"
    if order in ("a", "b"):
        assert sc.hist_blocks_from_the_middle(c.tiles()) >= 1
    if layout == "sentinel":
        assert any((c.slots[int(s["first_slot"]):int(s["first_slot"]) + int(s["n_slots"])][-3:] >> U64(63)).all() for s in c.segments), "a run at a tail"
    if layout == "fill":
        block = 1 << c.fill_shift
        assert not (c.segments["first_slot"] % block).any()
        held = np.concatenate([c.fill[int(s["first_slot"]) // block:(int(s["first_slot"]) + int(s["n_slots"]) + block - 1) // block] for s in c.segments])
        assert (held == 0).any() and (held == block).any() and ((held > 0) & (held < block)).any()
    for name, hooks in sc.TILE_HOOKS.items():
        m = c.model(hooks)
        assert (m["levels"], m["slot_fallbacks"]) == (1, 0), name
        bits, counts = m["level1"]
        assert bits == (3 if name == "defaults" else 7)
        assert max(int(x.max()) for x in counts) <= sc.sort_limits(hooks)[0], "every bin fits the last stage"


def test_orders_cross_segments_inside_a_histogram_block():
    assert sum(sc.hist_blocks_from_the_middle(sc.tiles_case(o, "plain").tiles()) for o in sc.SEGMENT_ORDERS) >= 3


@pytest.mark.parametrize("tiles", sc.XCD_TILES)
def test_case_2_xcd_deal(tiles):
    c = sc.xcd_case(tiles)
    t = c.tiles()
    assert sum(t) == tiles and sorted(t)[-1] == 20 and set(t) - {20} <= {1, 2, 3} and len(t) > 20
    assert min(sc.XCD_TILES) < 64 <= sorted(sc.XCD_TILES)[1]  # the deal starts at 64 tiles: one case below, one at, two above
    # the last segment listed is not the last in memory
    assert int(c.segments["first_slot"][-1]) + int(c.segments["n_slots"][-1]) < len(c.slots)
    for hooks in (sc.XCD_HOOKS, {}):
        m = c.model(hooks)
        assert m["levels"] == 1 and m["tiles"] == [tiles]
        assert max(int(x.max()) for x in m["level1"][1]) <= sc.sort_limits(hooks)[0]


def test_case_3_exact_capacities():
    cap, _, slot_cap = sc.sort_limits(sc.CAP_HOOKS)
    assert (cap, slot_cap) == (512, 640)
    for variant, special, levels, fallbacks in (("slots", {0, 1, 511, 512, 513, 639, 640}, 2, 0), ("over", {0, 1, 511, 512, 513, 639, 641}, 2, 1),
                                                ("within", {0, 1, 511, 512}, 1, 0)):
        c = sc.capacity_case(variant)
        m = c.model(sc.CAP_HOOKS)
        bits, counts = m["level1"]
        assert 1 <= bits <= 7 and bits == c.read_bits + 1, "bins are (read, strand) groups"
        # group sizes, counted from the records: read and strand are the top 7 key bits
        groups = np.bincount((c.real[0] >> U64(sc.STRAND_SHIFT)).astype(np.int64), minlength=128)
        assert np.array_equal(groups, counts[0]) and np.array_equal(groups, c.note["sizes"])
        assert special <= set(groups.tolist()) and groups.max() == max(special)
        assert (m["levels"], m["slot_fallbacks"], m["slots_allowed"]) == (levels, fallbacks, not fallbacks)
        assert len(c.segments) == 1 and c.tiles() == [4]


@pytest.mark.parametrize("n_contigs", sc.LOOKUP_TABLES)
def test_case_4_contig_lookups(n_contigs):
    for layout, hooks in sc.LOOKUP_HOOKS.items():
        c = sc.lookup_case(n_contigs, layout)
        assert len(c.contig_off) == n_contigs and (np.diff(c.contig_off.astype(np.int64)) >= 23).all() and c.contig_off[0] == 0
        lens = np.diff(np.concatenate([c.contig_off.astype(np.int64), [c.span]]))
        assert n_contigs < 4 or ((lens <= 40).any() and (lens >= sc.LOOKUP_BIG).any()), "short contigs mixed with long ones"
        first, last, chosen = c.note["edges"]
        pos = (((c.real[0] >> U64(sc.POS_SHIFT)) & U64(0xFFFFFFFF)) >> U64(32 - c.pos_bits)).astype(np.int64)
        assert np.isin(first[chosen], pos).all() and np.isin(last[chosen], pos).all() and {0, n_contigs - 1} <= set(chosen.tolist())
        assert (len(chosen) == n_contigs) if (layout == "no-level" and n_contigs <= 4000) else (len(chosen) >= min(n_contigs, 20))
        assert c.slots[0] == U64(sc.SENTINEL) and c.tiles() == [1]
        m = c.model(hooks)
        assert m["levels"] == (0 if layout == "no-level" else 1)
        if layout == "one-level":
            assert m["bin_bits"] == 7 and max(int(x.max()) for x in m["level1"][1]) <= 64
            assert all(rem == c.key_bits - 7 == 18 for _, rem in m["finals"])
        paths = sc.lookup_paths(c, m)
        print(n_contigs, layout, paths)
        assert all(t == ("few" if n_contigs <= 512 else "many") for t, _ in paths)
        if layout == "no-level":
            assert list(paths) == [("few" if n_contigs <= 512 else "many", "near" if n_contigs <= 4 else ("lds" if n_contigs <= 64 else "global"))]
        elif n_contigs >= 512:
            assert {r for _, r in paths} == {"near", "lds", "global"}


def test_case_4_all_six_lookups_occur():
    seen = set()
    for n_contigs in sc.LOOKUP_TABLES:
        for layout, hooks in sc.LOOKUP_HOOKS.items():
            c = sc.lookup_case(n_contigs, layout)
            seen |= set(sc.lookup_paths(c, c.model(hooks)))
    assert seen == sc.SIX_PATHS


def test_case_5_top_of_the_position_field():
    c = sc.top_case("bits32")
    assert c.pos_bits == 32 and c.span == (1 << 32) - 1 and {0, (1 << 31) - 1, 1 << 31, (1 << 32) - 24} <= set(c.note["pos"].tolist())
    assert int(c.note["pos"].max()) == (1 << 32) - 24
    c = sc.top_case("base12")
    assert (c.pos_bits, c.pos_base) == (12, (1 << 32) - 4096) and {c.pos_base, (1 << 32) - 24} <= set(c.note["pos"].tolist()) and int(c.note["pos"].max()) == (1 << 32) - 24
    c = sc.top_case("bits1")
    assert c.pos_bits == 1 and len(c.real[0]) == 256
    for name in sc.TOP_CASES:
        c = sc.top_case(name)
        ref = c.reference()
        assert len(ref) == len(c.real[0]) and (ref["contig"] < len(c.contig_off)).all()
        assert c.model(sc.TOP_HOOKS["defaults"])["levels"] == 0 and c.model(sc.TOP_HOOKS["levels"])["levels"] >= 2
        # free_bits >= 32 without a level: the whole key is left to the last stage
        assert name == "bits1" or c.key_bits >= 32 or c.pos_base
    # a level-1 bin of base12 under the hooks: its range's upper end is the top of 32 bits
    c = sc.top_case("base12")
    his = {sc.bin_range(recs[0], rem, c.pos_bits, c.pos_base)[1] for recs, rem in c.model(sc.TOP_HOOKS["levels"])["finals"]}
    assert 0xFFFFFFFF in his


def test_case_6_deep_levels():
    c = sc.deep_case()
    m = c.model(sc.DEEP_HOOKS)
    assert 30 <= m["levels"] < sc.MAX_LEVELS and m["bin_bits"] == 1 and c.key_bits == 39
    keys = sc.sort_keys(c.real[0])
    assert len(keys) == 3000 and int(keys.max() - keys.min()) == 2999, "consecutive positions of one read and strand"
    assert max(m["tiles"]) >= 64, "a deep level with enough tiles for the XCD deal"


def test_case_7_ranking():
    c = sc.ranking_case(False)
    sub_bits, low_bits, sizes = sc.sub_bin_sizes(c.real[0], c.key_bits, c.pos_bits)
    assert (sub_bits, low_bits) == (13, 26) and set(sizes.tolist()) == set(sc.RANK_SIZES)
    assert 7900 <= len(c.real[0]) <= sc.SORT_CAP and c.model({})["levels"] == 0
    c = sc.ranking_case(True)
    sub_bits, low_bits, sizes = sc.sub_bin_sizes(c.real[0], c.key_bits, c.pos_bits)
    assert sub_bits == 12 < sc.SUB_BITS and low_bits == 0 and c.model({})["levels"] == 0


def test_case_8_holes():
    c = sc.holes_case()
    block = 64
    assert c.fill_shift == 6 and not (c.slots >> U64(63)).any(), "every hole looks like a record"
    for s, sg in enumerate(c.segments):
        first, n = int(sg["first_slot"]), int(sg["n_slots"])
        idx = np.arange(first, first + n)
        hole = (idx % block) >= c.fill[idx // block]
        assert hole.any() and np.isin(sc.sort_keys(c.slots[idx][hole]), sc.sort_keys(c.real[s])).all(), "holes duplicate real keys"
        assert not np.isin(c.slots[idx][hole], c.real[s]).any()
        assert len(c.visible(s)) == len(c.real[s]) == n - hole.sum()
    held = c.fill[:(len(c.slots) + block - 1) // block]
    assert (held == 0).any() and (held == block).any()
    assert any(int(sg["n_slots"]) % block for sg in c.segments), "a last block cut by n_in"
    for name, hooks in sc.HOLE_HOOKS.items():
        assert c.model(hooks)["levels"] == (0 if name == "no-level" else 1)


@pytest.mark.parametrize("n_regions", sc.SCAN_REGIONS)
def test_case_9_scan_form(n_regions):
    c = sc.scan_case(n_regions)
    counts = c.region_counts()
    assert len(c.keys) > 8 * 8192 and c.tile_regions()[0] == 1
    if n_regions > 1:
        assert counts[0] == 0 and (n_regions == 2 or counts[-1] == 0)
    if n_regions == 256:
        empty = np.flatnonzero(counts == 0)
        assert (np.diff(empty) == 1).sum() > 200 and (counts[[2, 3]] > 0).all(), "runs of empty regions between full ones"
    reads = ((c.keys >> U64(33)) & U64(63))
    for q in np.flatnonzero(counts):
        mine = reads[(c.keys >> U64(39)) == U64(q)]
        assert (mine == 0).any() and (mine == 63).any()
    assert c.guide_base + 64 * n_regions == 1 << 32 and (n_regions > 1 or c.guide_base == 0xFFFFFFC0)
    ref = c.reference()
    assert len(ref) == len(c.keys) and int(ref["guide"].max()) == (1 << 32) - 1 - 64 * (n_regions - 1 - int(np.flatnonzero(counts)[-1]))
    assert np.array_equal(c.vals >> 23, sc.popcount(c.vals & sc.MASK23))
