"""Every reader of the seed search's records under every layout the search can leave them in (tests/layouts.py): the record
sinks, which walk the records where they lie with the sentinels among them; the sort's first level, which takes the block
fill table instead (fill_holes_kernel, bin_partition_kernel, bin_hist_kernel); the rows path with its side words.  Every call
proves through vsc_timing.seed_layout that the layout it named is the one that ran."""
import numpy as np
import pytest

import varscot_amd as va
import variants_cases as vc
from helpers import cut, inside_numpy
from layouts import LAYOUTS, check
from parts_cases import few_hits_case, repeat_rich_case
from sink_walk_case import INTERVALS, M, every_sink_equals_the_oracle, sink_walk_case

pytestmark = pytest.mark.gpu

SORT_CAP = 8064  # kSortCap (vsc_internal.h): the most record slots of a region that the sort's last stage takes as they are


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


# ---------------------------------------------------------------------------------------------- A. the sinks
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_every_sink_under_every_layout(ctx, hooks, oracle, layout):
    """What test_sink_walk.py runs - summary with an excluded locus, summary with regions under both rules, votes summary,
    selection by MIT score and by votes - and the selection with regions, over records left in `layout`: the same oracle-derived
    bytes.  A sink reads sentinels (fill bit 0) and its search is one launch."""
    c = sink_walk_case(oracle)
    hooks(**LAYOUTS[layout])
    gen = ctx.load_genome(c["packed"])
    try:
        every_sink_equals_the_oracle(ctx, gen, c, "seed", after=lambda: check(ctx.timing(), layout, fill=False))
        hits, score = c["hits"], c["score"]
        for rule in ("overlap", "inside"):
            inside = inside_numpy(c["packed"], INTERVALS, rule, hits)
            reg = va.Regions(c["packed"], INTERVALS, rule=rule)
            for scope, side in (("keep", inside), ("drop", ~inside)):
                h = gen.search_select(c["guides"], M, top_k=3, algorithm="seed", regions=reg, region_scope=scope)
                check(ctx.timing(), layout, fill=False)
                got = h.to_numpy().copy()
                h.close()
                assert 0 < len(got) < side.sum()
                assert got.tobytes() == cut(hits[side], score[side], 3, 0).tobytes(), (rule, scope)
            reg.close()
    finally:
        gen.close()


@pytest.fixture(scope="module")
def windows(ctx, tmp_path_factory):
    """The small window genome of tests/variants_cases.py as test_variants_screen.py makes it: (scenario, case, map, resident genome)."""
    seed, (m, sample) = vc.SEEDS[0], vc.CASES[0]
    sc = vc.scenario(seed)
    ref = va.PackedGenome.from_sequences(sc.seqs, sc.names)
    path = tmp_path_factory.mktemp("vcf") / "in.vcf"
    path.write_text(sc.vcf)
    win = va.variant_windows(ref, path, sample=sample, threads=2)
    assert list(win.names) == [w[0] for w in sc.windows(sample)]
    vmap, gen = va.VariantMap(win, ref), ctx.load_genome(win)
    yield sc, sc.case(m, sample), vmap, gen
    gen.close()
    vmap.close()


@pytest.mark.parametrize("layout", ["group", "group-64", "wave-64"])
def test_variant_summary_under_layouts(ctx, hooks, windows, layout):
    """summarize_variants: the rows test_variants_screen.py expects of the merger's restatement.  The variant summary is no
    walker of unsorted records: vsc_search_summary_variants streams sorted batches (search_stream) and merges each where the
    sort left it, so its search is one whose records only the sort reads - the fill table, not sentinels."""
    sc, case, vmap, gen = windows
    hooks(**LAYOUTS[layout])
    rows, var, dups = gen.summarize_variants(sc.guides, case.m, vmap, exclude=sc.loci, algorithm="seed")
    check(ctx.timing(), layout, fill=True)
    for got, want in ((rows, case.rows_all), (var, case.rows_var)):
        for f in ("nm", "mit_sum", "mit_ub", "on_target"):
            assert np.array_equal(got[f].astype(np.int64), want[f]), f
    assert np.array_equal(dups.astype(np.int64), case.dups)
    assert case.rows_all["on_target"].sum() >= 1 and case.dups.sum() >= vc.FLOORS["dup_adjacent"]


# ---------------------------------------------------------------------------------------------- B. the sort alone
# How level 1 consumes the fill table, and what bin_sort's accounting (SortInfo.bytes) then says per record: the last stage
# reads 8 bytes and writes 16; a slot partition reads and writes 8; an exact level reads the records once more for its
# histogram.  Unused slots are never counted.
SORT_LEGS = {
    "defaults": (dict(), 16 + 24),
    "slot": (dict(sort_cap=512, sort_optimistic=1, sort_slot_cap=4096), 16 + 24),
    "exact": (dict(sort_cap=512, sort_optimistic=0), 24 + 24),
}


def sorted_search(ctx, gen, guides, m, want):
    h = gen.search(guides, m, algorithm="seed")
    got = h.to_numpy().copy()
    h.close()
    assert got.tobytes() == want.tobytes()
    return ctx.timing()


@pytest.mark.parametrize("leg", list(SORT_LEGS))
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_sort_reads_the_fill_table_under_every_layout(ctx, hooks, oracle, layout, leg):
    """The repeat-rich case of test_search_parts.py, records that only the sort reads: the oracle's bytes, the fill table
    in use, one level and the sort's byte count of the leg - the slot partition with small bins, the exact level with its
    histogram, and the library's own choice.
    Without hooks the level runs as well: region 0 holds 9 663 records, more than the last stage takes (8 064), so the level
    has at least one bit, and a genome that has not yet shown a bin outgrowing its slot gets the slot partition (16 + 24 bytes
    a record).  The way without any level is test_small_regions_go_to_the_last_stage_unpartitioned's."""
    guides, _, packed, want = repeat_rich_case(oracle)
    assert np.bincount(want["guide"] // 64).max() > SORT_CAP
    sort, per_record = SORT_LEGS[leg]
    hooks(**LAYOUTS[layout], **sort)
    gen = ctx.load_genome(packed)
    try:
        t = sorted_search(ctx, gen, guides, 8, want)
    finally:
        gen.close()
    check(t, layout, fill=True)
    print(layout, leg, {k: t[k] for k in ("hits", "sort_levels", "sort_bin_bits", "sort_fallbacks", "sort_bytes")})
    assert t["hits"] == len(want)
    assert (t["sort_levels"], t["sort_fallbacks"]) == (1, 0)
    assert t["sort_bytes"] == per_record * len(want)


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_small_regions_go_to_the_last_stage_unpartitioned(ctx, hooks, oracle, layout):
    """At most 7 records a region: at most 7 blocks of at most 1 024 slots, fewer than the last stage takes as they are - no
    level whatever the layout; fill_holes_kernel writes the sentinels the search did not, and the last stage moves 24 bytes a
    record."""
    guides, packed, want = few_hits_case(oracle)
    assert 7 * 1024 <= SORT_CAP
    hooks(**LAYOUTS[layout])
    gen = ctx.load_genome(packed)
    try:
        t = sorted_search(ctx, gen, guides, 2, want)
    finally:
        gen.close()
    check(t, layout, fill=True)
    assert (t["sort_levels"], t["sort_fallbacks"]) == (0, 0)
    assert t["sort_bytes"] == 24 * len(want)


# ---------------------------------------------------------------------------------------------- C. the rows path
@pytest.mark.parametrize("layout", ["group", "group-64", "wave-64"])
def test_rows_path_under_layouts(ctx, hooks, oracle, layout):
    """search_streamed_rows in batches of 48 reads: the oracle's records, the rows of the gathering kernel on the same hits;
    side words travel beside the records, so the search writes sentinels and is one launch."""
    import torch
    from varscot_amd.dist import DeviceAlias
    guides, _, packed, want = repeat_rich_case(oracle)
    hooks(**LAYOUTS[layout])
    gen = ctx.load_genome(packed)
    recs, bad = [], []

    def on_batch(h, first, count, rows_dev):
        check(ctx.timing(), layout, fill=False)
        a = h.to_numpy().copy()
        recs.append(a)
        if len(a):
            got = torch.as_tensor(DeviceAlias(rows_dev, 64 * len(a)), device="cuda:0").view(torch.int32).view(-1, 16).cpu().numpy().view(np.uint32)
            ref, _ = h.packed_features(to_host=True)
            if not np.array_equal(got, ref):
                bad.append(first)

    try:
        gen.search_streamed_rows(guides, 8, on_batch, batch=48, algorithm="seed")
        check(ctx.timing(), layout, fill=False)
    finally:
        gen.close()
    assert len(recs) == 2 and not bad
    assert np.concatenate(recs).tobytes() == want.tobytes()
