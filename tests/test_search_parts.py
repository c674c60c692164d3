"""A seed search in parts (hook seed_parts): the chunk range cut into several launches, the level-1 slot partition of each part
running beside the next, the unused tails of the search's blocks named by the block fill table instead of sentinels.  The
records are the oracle's, byte for byte, however the search is cut."""
import numpy as np
import pytest

import varscot_amd as va
from helpers import aggregate
from layouts import decode
from parts_cases import MORE_READS_MARKED, more_reads_case, no_hit_case, overflow_case, repeat_rich, repeat_rich_case, repeat_rich_scores
from sink_walk_case import M as SINK_M, sink_walk_case

pytestmark = pytest.mark.gpu


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


@pytest.fixture(scope="module")
def case(oracle):
    """70 guides (two regions), > 8 000 hits at m = 8; the oracle's records, computed once and never changed (parts_cases.py)."""
    return repeat_rich_case(oracle)


def search(ctx, gen, guides, want, m=8):
    h = gen.search(guides, m, algorithm="seed")
    got = h.to_numpy().copy()
    h.close()
    assert got.tobytes() == want.tobytes()
    return ctx.timing()


@pytest.mark.parametrize("parts", [1, 2, 3, 4, 1 << 20])
def test_search_in_parts_equals_the_oracle(ctx, hooks, case, parts):
    """seed_parts = 1, 2, 3, 4 and more parts than the index has chunks (the library cuts no finer than a chunk a part), with
    chunk sharing.  A search in parts always partitions - the level has begun before the number of records is known."""
    guides, _, packed, want = case
    hooks(seed_parts=parts, seed_shared=1)
    gen = ctx.load_genome(packed)
    for _ in range(2):  # (the second search finds the buffers and the genome's hints of the first)
        t = search(ctx, gen, guides, want)
        assert t["hits"] == len(want) and t["sort_fallbacks"] == 0
        assert parts == 1 or t["sort_levels"] >= 1, t
    gen.close()


def test_parts_with_small_blocks(ctx, hooks, case):
    """seed_reserve = 64 with three parts: many closed short blocks - a wave's two blocks per load instruction of the
    partition -, regions that get nothing in a part."""
    guides, _, packed, want = case
    hooks(seed_parts=3, seed_shared=1, seed_reserve=64)
    gen = ctx.load_genome(packed)
    t = search(ctx, gen, guides, want)
    assert t["sort_levels"] >= 1 and t["sort_fallbacks"] == 0
    hooks(seed_parts=3, seed_shared=1, seed_reserve=64, seed_group_out=0)  # per-wave blocks
    search(ctx, gen, guides, want)
    gen.close()


def test_parts_slot_overflow_falls_back(ctx, hooks, case):
    """Slots smaller than the fullest bins: the parts' partitions raise the overflow flag, the level runs again the exact way
    over the whole regions (the search's buffer is untouched), and the genome remembers - the next search is one launch."""
    guides, _, packed, want = case
    hooks(seed_parts=2, seed_shared=1, sort_cap=512, sort_slot_cap=40)
    gen = ctx.load_genome(packed)
    t = search(ctx, gen, guides, want)
    assert t["sort_fallbacks"] == 1 and t["sort_levels"] >= 1
    assert search(ctx, gen, guides, want)["sort_fallbacks"] == 0
    gen.close()


def test_parts_bins_go_on_to_level_two(ctx, hooks, case):
    """sort_cap = 64, sort_max_bits = 2: the bins of the parts' level are far too large for the last stage and go through
    further levels from their slots."""
    guides, _, packed, want = case
    hooks(seed_parts=3, seed_shared=1, sort_cap=64, sort_max_bits=2, sort_optimistic=1, sort_slot_cap=60000)
    gen = ctx.load_genome(packed)
    t = search(ctx, gen, guides, want)
    assert t["sort_levels"] >= 2 and t["sort_fallbacks"] == 0, t
    gen.close()


def test_parts_three_regions_the_last_partial(ctx, hooks, oracle):
    """130 guides: three regions, two reads in the last."""
    guides, contigs = repeat_rich(1303, 130, 7000)
    want = oracle.search_fast(contigs, guides, 8)
    assert len(want) > 6000
    gen = ctx.load_genome(va.PackedGenome.from_sequences(contigs))
    for parts in (1, 4):
        hooks(seed_parts=parts, seed_shared=1)
        search(ctx, gen, guides, want)
    hooks(seed_parts=4, seed_shared=1, sort_cap=256)
    assert search(ctx, gen, guides, want)["sort_levels"] >= 1
    gen.close()


def test_rows_path_ignores_the_hook(ctx, hooks, case):
    """search_streamed_rows keeps the sites' bases beside the records: always one launch, sentinels as ever."""
    guides, _, packed, want = case
    gen = ctx.load_genome(packed)

    def run():
        import torch
        from varscot_amd.dist import DeviceAlias
        recs, levels = [], []

        def on_batch(h, first, count, rows_dev):
            a = h.to_numpy().copy()
            recs.append(a)
            levels.append(ctx.timing()["sort_levels"])
            if len(a):  # the rows the last stage wrote beside the records
                recs.append(torch.as_tensor(DeviceAlias(rows_dev, 64 * len(a)), device="cuda:0").view(torch.int32).cpu().numpy().copy())

        gen.search_streamed_rows(guides, 8, on_batch, batch=48, algorithm="seed")
        assert np.concatenate([r for r in recs if r.dtype == want.dtype]).tobytes() == want.tobytes()
        return b"".join(r.tobytes() for r in recs), levels

    plain, levels_plain = run()
    hooks(seed_parts=4, seed_shared=1)
    hooked, levels_hooked = run()
    assert hooked == plain and levels_hooked == levels_plain
    gen.close()


def test_summary_sink_ignores_the_hook(ctx, hooks, case):
    """The summary walks the records where the search left them, sentinels among them: the hook changes nothing."""
    guides, contigs, packed, want = case
    gen = ctx.load_genome(packed)
    plain = gen.summarize(guides, 8, algorithm="seed").copy()
    hooks(seed_parts=4, seed_shared=1)
    hooked = gen.summarize(guides, 8, algorithm="seed")
    assert hooked.tobytes() == plain.tobytes()
    assert np.array_equal(hooked["nm"].sum(axis=1), np.bincount(want["guide"], minlength=len(guides)))
    gen.close()


@pytest.mark.parametrize("parts", [1, 3])
def test_sort_bytes_count_records_only(ctx, hooks, case, parts):
    """One slot level: 16 bytes per record through the partition, 24 through the last stage - and not a byte for the unused
    slots of the search's blocks."""
    guides, _, packed, want = case
    sort = dict(seed_shared=1, sort_cap=512, sort_optimistic=1, sort_slot_cap=4096)
    hooks(seed_parts=1, **sort)
    gen = ctx.load_genome(packed)
    t = search(ctx, gen, guides, want)
    if parts > 1:  # (a search in parts takes its level's key bits from what the genome's last search produced)
        hooks(seed_parts=parts, **sort)
        t = search(ctx, gen, guides, want)
    assert t["hits"] == len(want)
    assert (t["sort_levels"], t["sort_fallbacks"]) == (1, 0)
    assert t["sort_bytes"] == 40 * len(want)
    gen.close()


# ---- the branches of a search in parts: every case with chunk sharing, against the oracle byte for byte, the number of launches
# read from vsc_timing.seed_layout (tests/layouts.py)
def launches(t):
    """Launches of the search behind ctx.timing() = t; a search in parts is one that only the sort reads (the fill table)."""
    layout = decode(t["seed_layout"])
    assert layout["shared"] and layout["fill"], layout
    return layout["launches"]


def test_lost_records_rerun_the_pass_in_one_launch(ctx, hooks, oracle):
    """The genome of test_hit_buffer_overflow_is_retried - 40 copies of one read, 60 000 perfect sites, 2 400 000 hits at m = 0
    where the estimate allows about a million - in three parts: records are lost, the pass runs again in ONE launch (passes
    == 2, the fill table written anew); the next search knows the rate, loses nothing and is cut into three.
    Slots of 32 768 records, taken without asking whether they pay (sort_optimistic = 1): a bin of the rerun's level - a
    read, a strand, a quarter of the positions - holds up to 21 846 of a read's 60 000 records, and a genome that has shown
    a bin outgrowing its slot is never searched in parts again (plan_parts)."""
    guides, packed, want = overflow_case(oracle)
    assert len(want) == 2_400_000 and np.all(want["pos"] % 24 == 0)
    hooks(seed_parts=3, seed_shared=1, sort_optimistic=1, sort_slot_cap=32768)
    gen = ctx.load_genome(packed)
    try:
        t = search(ctx, gen, guides, want, m=0)
        assert t["passes"] == 2 and t["hits"] == len(want), t
        assert launches(t) == 1 and t["sort_fallbacks"] == 0
        t = search(ctx, gen, guides, want, m=0)
        assert t["passes"] == 1 and t["hits"] == len(want), t
        assert launches(t) == 3 and t["sort_fallbacks"] == 0
    finally:
        gen.close()


def test_parts_with_a_region_without_records(ctx, hooks, oracle):
    """The guide set of test_sink_walk.py: 200 reads, region 1 (reads 64 .. 127) without any record, the last region of 8
    reads.  In parts every region is a segment of the level, the empty one too."""
    c = sink_walk_case(oracle)
    hooks(seed_parts=3, seed_shared=1)
    gen = ctx.load_genome(c["packed"])
    try:
        for _ in range(2):
            t = search(ctx, gen, c["guides"], c["hits"], m=SINK_M)
            assert launches(t) == 3 and t["sort_fallbacks"] == 0 and t["passes"] == 1, t
    finally:
        gen.close()


def test_parts_without_any_hit(ctx, hooks, oracle):
    """No hit at all, four parts: segments of no records in every part, nothing for the level to do - 0 records and no error,
    with 70 reads and with one read (one region of one read)."""
    guides, packed, want = no_hit_case(oracle)
    hooks(seed_parts=4, seed_shared=1)
    gen = ctx.load_genome(packed)
    try:
        for reads in (guides, guides[:1]):
            t = search(ctx, gen, reads, want, m=0)
            assert t["hits"] == 0 and launches(t) == 4, t
    finally:
        gen.close()


def test_parts_with_one_read(ctx, hooks, case, oracle):
    """One read: one region of one read, its records through the parts' level."""
    guides, contigs, packed, _ = case
    want = oracle.search_fast(contigs, guides[:1], 8)
    assert len(want) > 50
    hooks(seed_parts=3, seed_shared=1)
    gen = ctx.load_genome(packed)
    try:
        assert launches(search(ctx, gen, guides[:1], want)) == 3
    finally:
        gen.close()


def test_parts_in_the_second_read_pass(ctx, hooks, oracle):
    """The inputs of test_more_reads_than_one_pass_takes, 16 384 + 301 reads, both passes in two parts: the second pass has
    read indices from 16 384 on, its records go behind the first one's, and it finds the level's tables of the first.
    The sort's hooks pin the plan.  Without them the first pass (256 regions) is one launch - its slots would not pay -
    and its sort asks slots_fit about the regions that hold records: the answer hangs on how many record slots the search
    placed, open block tails included, which differs from run to run with the number of workgroups that met a hit; a "no"
    clears the genome's sort_slots_ok, and plan_parts then keeps the second pass in one launch.  sort_optimistic = 1 takes
    slots without asking, slots of 4 096 records hold every bin of 1 668 hits."""
    guides, packed, want = more_reads_case(oracle)
    hooks(seed_parts=2, seed_shared=1, sort_optimistic=1, sort_slot_cap=4096)
    gen = ctx.load_genome(packed)
    try:
        t = search(ctx, gen, guides, want, m=5)
    finally:
        gen.close()
    assert (t["read_passes"], t["passes"], t["sort_fallbacks"]) == (2, 2, 0), t
    assert launches(t) == 2 and t["hits"] == len(want), t
    assert {int(g) for g in want["guide"]} >= set(MORE_READS_MARKED[:3])


def test_streamed_batches_in_parts(ctx, hooks, case):
    """search_streamed in batches of 48 reads: the second batch starts behind the first one's records (used > 0)."""
    guides, _, packed, want = case
    hooks(seed_parts=3, seed_shared=1)
    gen = ctx.load_genome(packed)
    recs, seen = [], []

    def on_batch(h, first, count):
        recs.append(h.to_numpy().copy())
        seen.append(launches(ctx.timing()))

    try:
        gen.search_streamed(guides, 8, on_batch, batch=48, algorithm="seed")
    finally:
        gen.close()
    assert seen == [3, 3]
    assert np.concatenate(recs).tobytes() == want.tobytes()


def merged(parts):
    """The records of the shards as one result, as tests/fuzz_gpu.py merges them: shards partition the positions, a stable sort
    on (guide, strand) merges them."""
    got = np.concatenate(parts)
    key = (got["guide"].astype(np.int64) << 1) | (got["info"] >> 31)
    return got[np.argsort(key, kind="stable")]


def test_shards_in_parts(ctx, hooks, case):
    """Ranks 0 and 1 of a world of two on one context: the second shard's positions count from its first word (pos_base != 0)."""
    guides, _, packed, want = case
    hooks(seed_parts=3, seed_shared=1)
    parts = []
    for rank in range(2):
        gen = ctx.load_genome(packed, rank, 2)
        try:
            h = gen.search(guides, 8, algorithm="seed")
            parts.append(h.to_numpy().copy())
            h.close()
        finally:
            gen.close()
        assert launches(ctx.timing()) == 3
    assert all(len(p) for p in parts)
    assert merged(parts).tobytes() == want.tobytes()


def test_multi_context_in_parts(case):
    """MultiContext([0, 0]): two contexts on the device, each searching its shard in parts."""
    import ctypes as C
    from varscot_amd import _lib
    guides, _, packed, want = case
    m = va.MultiContext([0, 0])
    try:
        m.set_debug(seed_parts=3, seed_shared=1)
        g = m.load_genome(packed)
        h = g.search(guides, 8, algorithm="seed")
        got = h.to_numpy().copy()
        h.close()
        for i in range(2):
            t = _lib.Timing()
            assert va.lib().vsc_ctx_timing(C.c_void_p(va.lib().vsc_multi_ctx(m._h, i)), C.byref(t)) == 0
            assert launches(t.as_dict()) == 3
        g.close()
    finally:
        m.close()
    assert got.tobytes() == want.tobytes()


def test_release_scratch_between_searches_in_parts(ctx, hooks, case):
    """vsc_ctx_release_scratch gives the level's tables, its segments and its destination back; the second stream, the events
    and the pinned block stay.  The next search in parts makes the former again."""
    guides, _, packed, want = case
    hooks(seed_parts=3, seed_shared=1)
    gen = ctx.load_genome(packed)
    try:
        assert launches(search(ctx, gen, guides, want)) == 3
        ctx.release_scratch()
        assert launches(search(ctx, gen, guides, want)) == 3
    finally:
        gen.close()


def test_masked_context_stays_in_one_launch(case):
    """A context bound to a set of CUs (here: all of them) has no second stream on those CUs: one launch whatever the hook says."""
    import torch
    guides, _, packed, want = case
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    mask = np.zeros((n_cus + 31) // 32, dtype=np.uint32)
    for cu in range(n_cus):
        mask[cu // 32] |= np.uint32(1 << (cu % 32))
    own = va.Context(0, cu_mask=mask)
    try:
        own.set_debug(seed_parts=3, seed_shared=1)
        gen = own.load_genome(packed)
        assert launches(search(own, gen, guides, want)) == 1
        gen.close()
    finally:
        own.close()


def test_parts_on_the_callers_stream(case, oracle):
    """vsc_ctx_set_stream: the context works on a stream of the caller's, behind work of the caller's that is still running
    when the library queues its own - some tenths of a second of matrix products whose last result is checked afterwards; a
    search in parts orders its second stream against that stream by events alone.  One launch, three launches and a summary:
    the oracle's."""
    import torch
    guides, _, packed, want = case
    mit, ub = repeat_rich_scores(oracle)
    stream = torch.cuda.Stream()
    own = va.Context(0)
    try:
        own.set_stream(stream.cuda_stream)
        n = 4096
        with torch.cuda.stream(stream):
            ones = torch.ones(n, n, device="cuda:0")
            busy = ones
            for _ in range(200):  # (ones @ ones = n everywhere: exact in fp32, the chain stays at ones)
                busy = (busy @ ones) * (1.0 / n)
        gen = own.load_genome(packed)
        for parts in (1, 3):
            own.set_debug(seed_parts=parts, seed_shared=1)
            assert launches(search(own, gen, guides, want)) == parts
        rows = gen.summarize(guides, 8, algorithm="seed")
        assert rows.tobytes() == aggregate(want, len(guides), mit, ub).tobytes()
        gen.close()
        stream.synchronize()
        assert bool((busy == 1.0).all())
    finally:
        stream.synchronize()
        own.close()
