"""The bin sort (vsc_sort.hip, bin_sort in vsc_api.cpp) on records the test chose: vsc_debug_sort_records sorts the cases of
tests/sort_cases.py, and every result is compared byte for byte with the numpy reference (np.sort of each segment's visible
records, unpacked) - no tolerance.  Every run also compares the sort's accounting (levels, first level's bits, fallbacks,
bytes) with the host model of bin_sort's decisions, so that a case provably took the path it was built for;
tests/test_sort_records_cpu.py checks the cases' preconditions without a device."""
import ctypes as C

import numpy as np
import pytest

import varscot_amd as va
from varscot_amd import _lib
import sort_cases as sc

pytestmark = pytest.mark.gpu

ACCOUNT = ("levels", "bin_bits", "slot_fallbacks", "bytes")


@pytest.fixture(scope="module")
def ctx():
    c = va.Context(0)
    yield c
    c.close()


@pytest.fixture
def hooks(ctx):
    """ctx.set_debug(...) for one test (include/varscot_hip_debug.h); the defaults come back afterwards."""
    yield ctx.set_debug
    ctx.set_debug()


def sort_seed(ctx, table, case, slots_allowed=1):
    h, info = table.sort_slots(case.slots, case.segments, case.read_bits, case.pos_bits, case.pos_base, case.fill, case.fill_shift,
                               slots_allowed)
    got = h.to_numpy().copy()
    assert len(h) == info["n"] == len(got)
    h.close()
    t = ctx.timing()
    assert (t["sort_levels"], t["sort_bin_bits"], t["sort_fallbacks"], t["sort_bytes"], t["hits"]) == tuple(info[k] for k in ACCOUNT) + (len(got),)
    return got, info


def run_seed(ctx, hooks, case, hook_values, slots_allowed=1, table=None):
    """One sort of `case` under `hook_values`: the reference's bytes and the model's accounting.  Returns the accounting."""
    own = table is None
    table = table or va.ContigTable(ctx, case.contig_off, case.span)
    hooks(**hook_values)
    try:
        got, info = sort_seed(ctx, table, case, slots_allowed)
    finally:
        if own:
            table.close()
    want = case.reference()
    print({k: info[k] for k in info}, len(want))
    assert got.tobytes() == want.tobytes()
    start = bool(slots_allowed) if slots_allowed >= 0 else None
    if start is not None:
        m = case.model(hook_values, slots_allowed=start)
        assert {k: info[k] for k in ACCOUNT} == {k: m[k] for k in ACCOUNT}
        assert info["slots_allowed"] == m["slots_allowed"]
    return info


# ------------------------------------------------------------------------------------------------ 1. tiles and segments
@pytest.mark.parametrize("layout", sc.TILE_LAYOUTS)
@pytest.mark.parametrize("leg", list(sc.TILE_HOOKS))
@pytest.mark.parametrize("order", list(sc.SEGMENT_ORDERS))
def test_tiles_and_segments(ctx, hooks, order, leg, layout):
    """Segments of 1, 63, 8 191, 8 192, 8 193, 16 384 and 24 581 slots in three orders - histogram blocks that start inside a
    segment and cross several boundaries, partial last tiles - as plain records, with sentinels, and under a fill table."""
    info = run_seed(ctx, hooks, sc.tiles_case(order, layout), sc.TILE_HOOKS[leg])
    assert info["levels"] == 1


# ------------------------------------------------------------------------------------------------ 2. the XCD deal
@pytest.mark.parametrize("xcd", sc.XCD_SETTINGS)
@pytest.mark.parametrize("tiles", sc.XCD_TILES)
def test_xcd_deal(ctx, hooks, tiles, xcd):
    """63, 64, 65 and 71 tiles with sort_xcd at its default, off and forced: the same bytes, a level has run."""
    info = run_seed(ctx, hooks, sc.xcd_case(tiles), dict(sc.XCD_HOOKS, sort_xcd=xcd))
    assert info["levels"] >= 1


def test_xcd_deal_under_defaults(ctx, hooks):
    info = run_seed(ctx, hooks, sc.xcd_case(71), {})
    assert info["levels"] >= 1


# ------------------------------------------------------------------------------------------------ 3. exact capacities
def test_exact_capacities(ctx, hooks):
    """Bins of exactly 0, 1, 511, 512, 513, 639 and 640 records under sort_cap = 512 (slots of 640): the bins of 513 .. 640 go on
    to a second level from their slots, nothing falls back.  With one bin of 641 the slot partition falls back - the same
    kind of bytes - and the genome remembers: the next sort over that contig table histograms first.  Per record of level 1:
    16 + 24 bytes for a slot partition, 24 + 24 for an exact one (tests/test_layouts.py, SORT_LEGS)."""
    fits, over, within = (sc.capacity_case(v) for v in ("slots", "over", "within"))
    table = va.ContigTable(ctx, fits.contig_off, fits.span)
    try:
        info = run_seed(ctx, hooks, within, sc.CAP_HOOKS, table=table)
        assert (info["levels"], info["slot_fallbacks"]) == (1, 0) and info["bytes"] == (16 + 24) * len(within.slots)
        info = run_seed(ctx, hooks, fits, sc.CAP_HOOKS, table=table)
        assert (info["levels"], info["slot_fallbacks"], info["bin_bits"], info["slots_allowed"]) == (2, 0, 7, 1)
        second = sum(int(n) for n in fits.note["sizes"] if n > 512)  # records of the bins that went on
        assert second == 513 + 639 + 640 and info["bytes"] == (16 + 24) * len(fits.slots) + (24 + 24) * second
        info = run_seed(ctx, hooks, over, sc.CAP_HOOKS, table=table)
        assert (info["levels"], info["slot_fallbacks"], info["slots_allowed"]) == (2, 1, 0)
        assert info["bytes"] == 16 * len(over.slots) + (24 + 24) * len(over.slots) + (24 + 24) * (513 + 639 + 641)
        # the case that follows on this table: as the genome remembers (-1) it goes the exact way at once
        info = run_seed(ctx, hooks, fits, sc.CAP_HOOKS, slots_allowed=-1, table=table)
        assert (info["levels"], info["slot_fallbacks"], info["slots_allowed"]) == (2, 0, 0)
        assert info["bytes"] == (24 + 24) * len(fits.slots) + (24 + 24) * second
        # ... and with the permission given back, by slots again
        info = run_seed(ctx, hooks, fits, sc.CAP_HOOKS, slots_allowed=1, table=table)
        assert info["bytes"] == (16 + 24) * len(fits.slots) + (24 + 24) * second
    finally:
        table.close()


# ------------------------------------------------------------------------------------------------ 4. contig look-ups
@pytest.mark.parametrize("layout", list(sc.LOOKUP_HOOKS))
@pytest.mark.parametrize("n_contigs", sc.LOOKUP_TABLES)
def test_contig_lookups(ctx, hooks, n_contigs, layout):
    """Records at contigs' first and last positions over tables of 1 .. 100 000 contigs: without a level (the bin's range is
    everything) and with one level whose bins touch <= 4, 5 .. 64 and more contigs."""
    case = sc.lookup_case(n_contigs, layout)
    paths = sc.lookup_paths(case, case.model(sc.LOOKUP_HOOKS[layout]))
    print("look-ups (table, range): bins", paths)
    info = run_seed(ctx, hooks, case, sc.LOOKUP_HOOKS[layout])
    assert info["levels"] == (0 if layout == "no-level" else 1)


def test_all_six_contig_lookups_ran():
    seen = set()
    for n_contigs in sc.LOOKUP_TABLES:
        for layout, hk in sc.LOOKUP_HOOKS.items():
            case = sc.lookup_case(n_contigs, layout)
            seen |= set(sc.lookup_paths(case, case.model(hk)))
    assert seen == sc.SIX_PATHS


# ------------------------------------------------------------------------------------------------ 5. the top of the position field
@pytest.mark.parametrize("leg", list(sc.TOP_HOOKS))
@pytest.mark.parametrize("name", sc.TOP_CASES)
def test_top_of_the_position_field(ctx, hooks, name, leg):
    """32 position bits up to 2^32 - 24, 12 bits counted from 2^32 - 4096 (the range's end saturates), one bit."""
    run_seed(ctx, hooks, sc.top_case(name), sc.TOP_HOOKS[leg])


# ------------------------------------------------------------------------------------------------ 6. deep levels
def test_deep_levels(ctx, hooks):
    """39 key bits, one per level: 3 000 consecutive positions of one read take 35 levels, within bin_sort's guard of 48."""
    info = run_seed(ctx, hooks, sc.deep_case(), sc.DEEP_HOOKS)
    assert 30 <= info["levels"] < sc.MAX_LEVELS


# ------------------------------------------------------------------------------------------------ 7. ranking
@pytest.mark.parametrize("twin", [False, True])
def test_ranking(ctx, hooks, twin):
    """One bin for the last stage: sub-bins of 1, 4, 5, 64 and 700 records ranked on 26 low bits; the twin with 12 key bits has
    nothing left to rank."""
    info = run_seed(ctx, hooks, sc.ranking_case(twin), {})
    assert info["levels"] == 0


# ------------------------------------------------------------------------------------------------ 8. holes are not read
@pytest.mark.parametrize("leg", list(sc.HOLE_HOOKS))
def test_holes_are_not_read(ctx, hooks, leg):
    """Every hole of the fill table holds a record-like word with a real record's key: the result has the real records alone."""
    case = sc.holes_case()
    info = run_seed(ctx, hooks, case, sc.HOLE_HOOKS[leg])
    assert info["n"] == sum(len(r) for r in case.real) < (case.slots >> np.uint64(63) == 0).sum()
    assert info["levels"] == (0 if leg == "no-level" else 1)


# ------------------------------------------------------------------------------------------------ 9. the scan form
@pytest.mark.parametrize("n_regions", sc.SCAN_REGIONS)
def test_scan_form(ctx, hooks, n_regions):
    """Pairs through level 0: empty regions first, last and in runs, a tile of one region alone, nine tiles and a bit."""
    case = sc.scan_case(n_regions)
    table = va.ContigTable(ctx, case.contig_off, case.span)
    hooks()
    try:
        h, info = table.sort_pairs(case.keys, case.vals, n_regions, case.guide_base, case.pos_bits, case.pos_base)
        got = h.to_numpy().copy()
        h.close()
    finally:
        table.close()
    print(info)
    assert got.tobytes() == case.reference().tobytes()
    assert info["levels"] == (1 if case.region_counts().max() > sc.SORT_CAP else 0)


# ------------------------------------------------------------------------------------------------ 10. nothing, refusals
def test_nothing_and_refusals(ctx, hooks):
    hooks()
    table = va.ContigTable(ctx, [0, 100], 1000)
    try:
        none = np.zeros(0, dtype=np.uint64)
        h, info = table.sort_slots(none, np.zeros(0, dtype=_lib.SORT_SEGMENT_DTYPE), 6)
        assert len(h) == 0 and len(h.to_numpy()) == 0 and info["n"] == info["levels"] == info["bytes"] == 0
        h.close()
        h, info = table.sort_pairs(none, np.zeros(0, dtype=np.uint32), 3)
        assert len(h) == 0 and len(h.to_numpy()) == 0 and info["n"] == 0
        h.close()
        # a segment of sentinels alone: nothing either
        h, info = table.sort_slots(np.full(70, sc.SENTINEL, dtype=np.uint64), np.array([(3, 64, 0)], dtype=_lib.SORT_SEGMENT_DTYPE), 6)
        assert len(h) == 0
        h.close()

        slots = sc.random_records(np.random.default_rng(2), 100, 10, 6)
        seg = lambda first, n: np.array([(first, n, 0)], dtype=_lib.SORT_SEGMENT_DTYPE)  # noqa: E731
        fill = np.full(2, 64, dtype=np.uint32)
        L, out, inp = va.lib(), C.c_void_p(), _lib.DebugSortInput(slots_allowed=-1)
        assert L.vsc_debug_sort_records(None, table._h, C.byref(inp), None, C.byref(out)) == -22
        assert L.vsc_debug_sort_records(ctx._h, None, C.byref(inp), None, C.byref(out)) == -22
        assert L.vsc_debug_sort_records(ctx._h, table._h, None, None, C.byref(out)) == -22
        assert L.vsc_debug_sort_records(ctx._h, table._h, C.byref(inp), None, None) == -22
        assert L.vsc_debug_genome_from_contigs(ctx._h, None, 1, 10, C.byref(out)) == -22
        inp = _lib.DebugSortInput(slots=None, n_slots=100, segments=_lib.ptr(seg(0, 100)), n_segments=1, read_bits=6, slots_allowed=-1)
        assert L.vsc_debug_sort_records(ctx._h, table._h, C.byref(inp), None, C.byref(out)) == -22  # slots announced, none given
        refused = [
            lambda: table.sort_slots(slots, seg(1, 100), 6, 10),                        # a segment past the slot array
            lambda: table.sort_slots(slots, seg(101, 0), 6, 10),
            lambda: table.sort_slots(slots, seg(0, 100), 7, 10),                        # read bits
            lambda: table.sort_slots(slots, seg(0, 100), 6, 33),                        # position bits
            lambda: table.sort_slots(slots, seg(0, 100), 6, 10, fill=fill, fill_shift=5),
            lambda: table.sort_slots(slots, seg(32, 60), 6, 10, fill=fill, fill_shift=6),  # off the block boundaries
            lambda: table.sort_pairs(np.array([64 << 33], dtype=np.uint64), np.zeros(1, dtype=np.uint32), 1),  # a read outside the regions
            lambda: table.sort_pairs(np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint32), 0),
            lambda: table.sort_pairs(np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint32), 257),
            lambda: table.sort_pairs(np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint32), 2, guide_base=0xFFFFFFC0),
            lambda: table.sort_pairs(np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint32), 1, guide_base=5),
        ]
        for call in refused:
            with pytest.raises(va.VarscotError) as e:
                call()
            assert e.value.code == -22
        # the context still sorts
        h, info = table.sort_slots(slots, seg(0, 100), 6, 10)
        want = sc.unpack(np.sort(slots), 0, table.contig_off, 10, 0)
        assert info["n"] == 100 and h.to_numpy().tobytes() == want.tobytes()
        h.close()
        # pos_bits 0: derived from the table's span as a search derives them from a genome - 1 000 positions, 10 bits
        h, info = table.sort_slots(slots, seg(0, 100), 6)
        assert h.to_numpy().tobytes() == want.tobytes()
        h.close()
    finally:
        table.close()
