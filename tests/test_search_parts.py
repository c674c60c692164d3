"""A seed search in parts (hook seed_parts): the chunk range cut into several launches, the level-1 slot partition of each part
running beside the next, the unused tails of the search's blocks named by the block fill table instead of sentinels.  The
records are the oracle's, byte for byte, however the search is cut."""
import numpy as np
import pytest

import varscot_amd as va
from helpers import make_genome, mutate, random_guides, random_seq

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


def repeat_rich(seed, n_guides, n_pieces):
    """The construction of test_sort_without_the_histogram_pass_and_its_fallback: a contig of mutated read copies."""
    rng = np.random.default_rng(seed)
    guides = random_guides(rng, n_guides)
    pieces = []
    for _ in range(n_pieces):
        g = guides[int(rng.integers(0, len(guides)))]
        pieces.append(mutate(rng, g, int(rng.integers(0, 7)), 0, 20) + random_seq(rng, int(rng.integers(0, 3))))
    contigs = make_genome(seed, [60000, 20000], guides, 8, n_plant=200) + ["".join(pieces)]
    return guides, contigs


@pytest.fixture(scope="module")
def case(oracle):
    """70 guides (two regions), > 8 000 hits at m = 8; the oracle's records, computed once and never changed."""
    guides, contigs = repeat_rich(4711, 70, 9000)
    want = oracle.search_fast(contigs, guides, 8)
    assert len(want) > 8000
    want.setflags(write=False)
    return guides, contigs, va.PackedGenome.from_sequences(contigs), want


def search(ctx, gen, guides, want):
    h = gen.search(guides, 8, algorithm="seed")
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
