"""Hand-made inputs of the bin sort (vsc_debug_sort_records, include/varscot_hip_debug.h), their numpy reference, and a host
model of what bin_sort does with them - which levels run, on how many bits, which bins they leave, how many contigs a
bin's position range touches.  No device is needed here: tests/test_sort_records_cpu.py checks that every case builds what it
claims, tests/test_sort_records.py then feeds the cases to the device and compares bytes.

The constants restate vsc_internal.h; the model restates level_bits / sort_limits / bin_sort of vsc_api.cpp and the range
arithmetic at the top of finalize_bin (vsc_sort.hip).  The model only says WHICH path a case takes; what the device must
return is the reference's business alone: np.sort of each segment's visible records, unpacked."""
import functools
from dataclasses import dataclass, field

import numpy as np

from varscot_amd._lib import HIT_DTYPE, SORT_SEGMENT_DTYPE

U64 = np.uint64
MASK23 = 0x7FFFFF
SENTINEL = 0xFFFFFFFFFFFFFFFF
POS_SHIFT, STRAND_SHIFT, READ_SHIFT = 23, 55, 56
REGION_BITS, REGION_READS = 6, 64
TILE = 8192          # kSortTile
HIST_TILES = 8       # kHistTiles
SORT_CAP = 8064      # kSortCap
MAX_BIN_BITS = 11    # kSortMaxBinBits
SUB_BITS = 13        # kSortSubBits
NEAR, RANGE = 4, 64  # kFinalizeNear, kFinalizeRange
FEW_CONTIGS = 512    # kFinThreads: the contig table fits one entry per thread
MAX_LEVELS = 48


# ------------------------------------------------------------------------------------------------ records
def pack(read, strand, pos_global, mask, pos_bits, pos_base):
    """Packed 8-byte records (layout: vsc_internal.h)."""
    read, strand, pos_global, mask = (np.asarray(x, dtype=U64) for x in (read, strand, pos_global, mask))
    fld = (pos_global - U64(pos_base)) << U64(32 - pos_bits)
    assert np.all(fld < (1 << 32)) and np.all(read < REGION_READS) and np.all(strand < 2) and np.all(mask <= MASK23)
    return (read << U64(READ_SHIFT)) | (strand << U64(STRAND_SHIFT)) | (fld << U64(POS_SHIFT)) | mask


def popcount(x):
    x = np.asarray(x, dtype=np.uint32)
    return np.unpackbits(x.view(np.uint8).reshape(-1, 4), axis=1).sum(axis=1).astype(np.uint32)


def unpack(recs, guide_base, contig_off, pos_bits, pos_base):
    """Packed records -> HIT_DTYPE rows, as the issue states the reference."""
    recs = np.asarray(recs, dtype=U64)
    out = np.zeros(len(recs), dtype=HIT_DTYPE)
    read = (recs >> U64(READ_SHIFT)) & U64(REGION_READS - 1)
    strand = (recs >> U64(STRAND_SHIFT)) & U64(1)
    fld = (recs >> U64(POS_SHIFT)) & U64(0xFFFFFFFF)
    mask = (recs & U64(MASK23)).astype(np.uint32)
    pos_global = (fld >> U64(32 - pos_bits)) + U64(pos_base)
    off = np.asarray(contig_off, dtype=U64)
    contig = np.searchsorted(off, pos_global, "right") - 1
    out["guide"] = (U64(guide_base) + read).astype(np.uint32)
    out["contig"] = contig
    out["pos"] = (pos_global - off[contig]).astype(np.uint32)
    out["info"] = (strand.astype(np.uint32) << np.uint32(31)) | (popcount(mask) << np.uint32(23)) | mask
    return out


def unique_keys(rng, n, key_bits):
    """n distinct keys below 2^key_bits, in random order."""
    space = 1 << key_bits
    assert n <= space
    if space <= 4 * n + 1024:
        return rng.permutation(space)[:n].astype(U64)
    got = np.unique(rng.integers(0, space, size=n + n // 8 + 64, dtype=np.uint64))
    while len(got) < n:
        got = np.unique(np.concatenate([got, rng.integers(0, space, size=n, dtype=np.uint64)]))
    return rng.permutation(got)[:n]


def records_from_keys(rng, keys, pos_bits, read_bits):
    """Keys of pos_bits + 1 + read_bits bits (read | strand | relative position) -> records with random masks."""
    keys = np.asarray(keys, dtype=U64)
    rel = keys & U64((1 << pos_bits) - 1)
    strand = (keys >> U64(pos_bits)) & U64(1)
    read = keys >> U64(pos_bits + 1)
    assert np.all(read < (1 << read_bits))
    mask = rng.integers(0, MASK23 + 1, size=len(keys), dtype=np.uint64)
    return (read << U64(READ_SHIFT)) | (strand << U64(STRAND_SHIFT)) | ((rel << U64(32 - pos_bits)) << U64(POS_SHIFT)) | mask


def random_records(rng, n, pos_bits, read_bits):
    return records_from_keys(rng, unique_keys(rng, n, pos_bits + 1 + read_bits), pos_bits, read_bits)


def sort_keys(recs):
    return np.asarray(recs, dtype=U64) >> U64(POS_SHIFT)


# ------------------------------------------------------------------------------------------------ a case
@dataclass
class SeedCase:
    """Seed form: slots, segments, optionally a fill table; `real` = the records each segment was built from."""
    contig_off: np.ndarray
    span: int
    pos_bits: int
    pos_base: int
    read_bits: int
    slots: np.ndarray
    segments: np.ndarray
    real: list
    fill: np.ndarray = None
    fill_shift: int = 0
    note: dict = field(default_factory=dict)

    @property
    def key_bits(self):
        return self.pos_bits + 1 + self.read_bits

    def visible(self, s):
        """What the sort may see of segment s: the slots its blocks hold, sentinels left out."""
        sg = self.segments[s]
        idx = np.arange(int(sg["first_slot"]), int(sg["first_slot"]) + int(sg["n_slots"]), dtype=np.int64)
        recs = self.slots[idx]
        keep = (recs >> U64(63)) == 0
        if self.fill is not None:
            keep &= (idx & ((1 << self.fill_shift) - 1)) < self.fill[idx >> self.fill_shift]
        return recs[keep]

    def reference(self):
        parts = [unpack(np.sort(self.visible(s)), int(self.segments[s]["guide_base"]), self.contig_off, self.pos_bits, self.pos_base)
                 for s in range(len(self.segments))]
        return np.concatenate(parts) if parts else np.zeros(0, dtype=HIT_DTYPE)

    def check_built(self):
        """The slots hold exactly the records the case was made of, with keys unique per segment."""
        for s, want in enumerate(self.real):
            got = self.visible(s)
            assert np.array_equal(np.sort(got), np.sort(np.asarray(want, dtype=U64))), s
            assert len(np.unique(sort_keys(got))) == len(got), s
        return self

    def tiles(self):
        return [(int(n) + TILE - 1) // TILE for n in self.segments["n_slots"]]

    def model(self, hooks=None, slots_allowed=True):
        segs = [self.visible(s) for s in range(len(self.segments)) if int(self.segments[s]["n_slots"])]
        n_in = [int(n) for n in self.segments["n_slots"] if int(n)]
        return model_sort(segs, n_in, self.key_bits, self.pos_bits, hooks or {}, slots_allowed, fill=self.fill is not None)


def lay_out(real, n_in, guide_bases, rng, layout="plain", fill_shift=6, gap=0, hole=None, held_of=None):
    """Slot array + segment table for segments of n_in[i] slots made of the records real[i].
    plain     n_in[i] == len(real[i]): records in random order, nothing else
    sentinel  the other slots hold sentinels: a run at the tail of the segment's last block of 128, the rest scattered
    fill      blocks of 1 << fill_shift slots hold their first `held` slots (held_of(s, n_blocks) chooses, default: random with
              0 and full among them); the last block is cut by n_in; hole(s, k) fills the k slots of the holes (default: random
              words, sentinels among them); segments start on block boundaries
    gap: unused slots between segments (plain / sentinel)."""
    slots, segs, fills = [], [], []
    at = 0
    block = 1 << fill_shift
    for s, (recs, n) in enumerate(zip(real, n_in)):
        recs = rng.permutation(np.asarray(recs, dtype=U64))
        if layout == "fill":
            pad = -at % block
            slots.append(rng.integers(0, 1 << 63, size=pad, dtype=np.uint64))
            at += pad
            n_blocks = (n + block - 1) // block
            room = np.minimum(block, n - block * np.arange(n_blocks))
            held = held_of(s, n_blocks) if held_of else None
            if held is None:
                # spread the records over the blocks: as many as a block has room for, never more
                held = np.zeros(n_blocks, dtype=np.int64)
                left = len(recs)
                order = rng.permutation(n_blocks)
                for b in order:
                    take = min(int(room[b]), left, int(rng.choice([0, block, rng.integers(0, block + 1)])))
                    held[b] = take
                    left -= take
                for b in order:  # what is left over fills blocks up
                    take = min(int(room[b]) - int(held[b]), left)
                    held[b] += take
                    left -= take
                assert left == 0, "more records than slots"
            held = np.asarray(held, dtype=np.int64)
            assert int(np.minimum(held, room).sum()) == len(recs)
            seg = np.empty(n, dtype=U64)
            idx = np.arange(n)
            vis = (idx % block) < held[idx // block]
            seg[vis] = recs
            k = int((~vis).sum())
            if hole:
                seg[~vis] = hole(s, k)
            else:
                junk = rng.integers(0, 1 << 64, size=k, dtype=np.uint64)
                junk[rng.random(k) < 0.2] = U64(SENTINEL)
                seg[~vis] = junk
            fills.append((at // block, held))
        else:
            k = n - len(recs)
            assert k >= 0 and (layout == "sentinel" or k == 0)
            seg = np.full(n, U64(SENTINEL), dtype=U64)
            tail = min(k, rng.integers(0, 128)) if k else 0  # a run of sentinels at the end, the rest scattered
            where = np.sort(rng.permutation(n - tail)[:len(recs)])
            seg[where] = recs
        segs.append((at, n, guide_bases[s]))
        slots.append(seg)
        at += n
        if layout != "fill" and gap:
            slots.append(np.full(gap, U64(SENTINEL), dtype=U64))
            at += gap
    slots = np.concatenate(slots) if slots else np.zeros(0, dtype=U64)
    fill = None
    if layout == "fill":
        fill = rng.integers(0, block + 1, size=(len(slots) + block - 1) // block).astype(np.uint32)  # (blocks of no segment: anything)
        for b0, held in fills:
            fill[b0:b0 + len(held)] = held
    return slots, np.array(segs, dtype=SORT_SEGMENT_DTYPE), fill


# ------------------------------------------------------------------------------------------------ the host model of bin_sort
def ceil_log2(x):
    return 0 if x <= 1 else int(x - 1).bit_length()


def sort_limits(hooks):
    cap = min(SORT_CAP, max(16, hooks["sort_cap"])) if hooks.get("sort_cap") else SORT_CAP
    max_bits = min(MAX_BIN_BITS, max(1, hooks["sort_max_bits"])) if hooks.get("sort_max_bits") else MAX_BIN_BITS
    slot_cap = hooks.get("sort_slot_cap") or (cap + cap // 4 + 15) // 16 * 16
    return cap, max_bits, max(slot_cap, 16)


def level_bits(n_max, cap, max_bits, rem, n_segs):
    if n_max <= cap or rem == 0:
        return 0
    want = max(1, cap * 7 // 10)
    bits = min(max(1, ceil_log2((n_max + want - 1) // want)), max_bits, rem)
    while bits > 1 and (n_segs << bits) > (1 << 22):
        bits -= 1
    return bits


def bin_counts(recs, shift, bits):
    return np.bincount(((np.asarray(recs, dtype=U64) >> U64(shift)) & U64((1 << bits) - 1)).astype(np.int64), minlength=1 << bits)


def model_sort(segs, n_in, key_bits, pos_bits, hooks, slots_allowed=True, fill=False):
    """bin_sort's decisions for segments of visible records `segs` in n_in[i] slots.  Returns a dict: levels, bin_bits (of the
    first level), slot_fallbacks, bytes, slots_allowed (afterwards), tiles (per level), finals: per finalized bin
    (records, rem_after) with rem_after = the key bits the last stage orders, and level1: (bits, per-segment bin counts).
    The slot layout is assumed to fit the device (the cases' bin tables are small)."""
    cap, max_bits, slot_cap = sort_limits(hooks)
    pos_pad = 32 - pos_bits
    opt = hooks.get("sort_optimistic", -1)
    res = dict(levels=0, bin_bits=0, slot_fallbacks=0, bytes=0, slots_allowed=bool(slots_allowed), tiles=[], finals=[], level1=None)
    n_real = sum(len(s) for s in segs)
    rem = key_bits
    level = 1
    while segs:
        assert level <= MAX_LEVELS, "bin_sort's level guard"
        n_max = max(n_in)
        bits = level_bits(n_max, cap, max_bits, rem, len(segs))
        n_moved = n_real if (level == 1 and fill) else sum(n_in)
        if not bits:
            res["bytes"] += 24 * n_moved
            res["finals"] += [(s, rem) for s in segs if len(s)]
            assert n_max <= cap, "keys are not unique"
            break
        res["tiles"].append(sum((n + TILE - 1) // TILE for n in n_in))
        shift = POS_SHIFT + pos_pad + rem - bits
        counts = [bin_counts(s, shift, bits) for s in segs]
        if level == 1:
            res["level1"] = (bits, counts)
        use_slots = level == 1 and (opt == 1 or (opt != 0 and res["slots_allowed"]))
        if use_slots and opt != 1 and (len(segs) << bits) * slot_cap > 4 * sum(n_in) + (1 << 20):
            use_slots = res["slots_allowed"] = False  # slots_fit: the slot layout would dwarf the records
        if use_slots and max(int(c.max()) for c in counts) > slot_cap:
            res["slot_fallbacks"] += 1
            res["bytes"] += 16 * n_moved
            res["slots_allowed"] = False
            use_slots = False
        if res["levels"] == 0:
            res["bin_bits"] = bits
        res["levels"] += 1
        res["bytes"] += (16 if use_slots else 24) * n_moved + 24 * n_moved
        rem -= bits
        nxt = []
        for s, c in zip(segs, counts):
            b = ((s >> U64(shift)) & U64((1 << bits) - 1)).astype(np.int64)
            for q in np.nonzero(c)[0]:
                part = s[b == q]
                if c[q] > cap:
                    nxt.append(part)
                else:
                    res["finals"].append((part, rem))
        segs = nxt
        n_in = [len(s) for s in segs]
        n_real = sum(n_in)
        level += 1
    return res


def bin_range(rec, rem_after, pos_bits, pos_base):
    """The position range finalize_bin derives from a bin's first record (global, saturating)."""
    if rem_after >= 32:
        return 0, 0xFFFFFFFF
    rel = ((int(rec) >> POS_SHIFT) & 0xFFFFFFFF) >> (32 - pos_bits)
    lo = (rel >> rem_after) << rem_after
    hi = (lo | ((1 << rem_after) - 1)) + pos_base
    return min(lo + pos_base, 0xFFFFFFFF), min(hi, 0xFFFFFFFF)


def contigs_touched(contig_off, lo, hi):
    off = np.asarray(contig_off, dtype=np.int64)
    c_lo = max(int(np.searchsorted(off, lo, "right")), 1) - 1
    c_hi = max(int(np.searchsorted(off, hi, "right")), 1) - 1
    return c_hi - c_lo + 1


def lookup_paths(case, model):
    """Which of the finalize kernel's six contig look-ups each finalized bin takes: a set of (table, range) with table in
    {"few", "many"} (ballot count or thread 0's binary searches) and range in {"near", "lds", "global"}."""
    table = "few" if len(case.contig_off) <= FEW_CONTIGS else "many"
    paths = {}
    for recs, rem_after in model["finals"]:
        lo, hi = bin_range(recs[0], rem_after, case.pos_bits, case.pos_base)  # (any record of the bin gives the same range)
        n = contigs_touched(case.contig_off, lo, hi)
        rng_ = "near" if n <= NEAR else ("lds" if n <= RANGE else "global")
        paths[(table, rng_)] = paths.get((table, rng_), 0) + 1
    return paths


def sub_bin_sizes(recs, key_bits, pos_bits):
    """(sub_bits, low_bits, sizes of the non-empty sub-bins) of a bin that the last stage takes with all key bits left."""
    sub_bits = min(SUB_BITS, key_bits)
    low_bits = key_bits - sub_bits
    sb = (np.asarray(recs, dtype=U64) >> U64(POS_SHIFT + 32 - pos_bits + low_bits)) & U64((1 << sub_bits) - 1)
    return sub_bits, low_bits, np.unique(sb, return_counts=True)[1]


def hist_blocks_from_the_middle(tiles):
    """Histogram blocks (HIST_TILES tiles each) that start inside a segment and cross at least two segment boundaries."""
    first = np.concatenate([[0], np.cumsum(tiles)])
    n = 0
    for t0 in range(0, int(first[-1]), HIST_TILES):
        t1 = min(t0 + HIST_TILES, int(first[-1]))
        starts_inside = t0 not in set(first.tolist())
        crossed = int(((first > t0) & (first < t1)).sum())
        n += starts_inside and crossed >= 2
    return n


# ------------------------------------------------------------------------------------------------ contig tables
def one_contig(span):
    return np.zeros(1, dtype=np.uint32), span


def mixed_table(n_contigs, seed, big=1 << 18, span=1 << 24):
    """n_contigs ascending starts: short contigs (23..40 positions) first, then medium ones (big / 16), then long ones
    (2 * big); the last contig runs to `span`."""
    rng = np.random.default_rng(seed)
    n_long = max(1, min(4, n_contigs // 4))
    n_med = min(64, (n_contigs - n_long) // 2)
    n_short = n_contigs - n_long - n_med
    lens = np.concatenate([rng.integers(23, 41, size=n_short), np.full(n_med, big // 16), np.full(n_long, 2 * big)]).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(lens)[:-1]])
    assert off[-1] < span and len(off) == n_contigs
    return off.astype(np.uint32), span


# ------------------------------------------------------------------------------------------------ case 1: tiles and segments
SEGMENT_SIZES = [1, 63, 8191, 8192, 8193, 16384, 3 * 8192 + 5]
SEGMENT_ORDERS = {
    # single-record segments between the large ones; tiles 1 1 2 1 4 | 1 2 1 1 1 2 ...: the histogram block that starts at tile 8
    # starts at the last tile of the 24 581-slot segment and crosses into four more segments
    "a": [8191, 1, 16384, 1, 3 * 8192 + 5, 1, 8193, 63, 8192, 1, 8193, 1],
    "b": [1, 3 * 8192 + 5, 1, 8192, 8193, 1, 16384, 63, 1, 8191, 3 * 8192 + 5, 1, 63],
    "c": [63, 16384, 8193, 1, 8191, 1, 8192, 3 * 8192 + 5, 1, 1, 16384],
}
TILE_HOOKS = {
    "defaults": dict(),
    "cap512-exact": dict(sort_cap=512, sort_optimistic=0),
    "cap512-slots": dict(sort_cap=512, sort_optimistic=1),
}
TILE_LAYOUTS = ("plain", "sentinel", "fill")
TILE_POS_BITS, TILE_READ_BITS = 20, 6


@functools.lru_cache(maxsize=None)
def tiles_case(order, layout):
    rng = np.random.default_rng([11, sorted(SEGMENT_ORDERS).index(order), TILE_LAYOUTS.index(layout)])
    n_in = SEGMENT_ORDERS[order]
    assert set(n_in) == set(SEGMENT_SIZES)
    # sentinel / fill layouts: about nine records for every ten slots (a one-slot segment keeps its record)
    n_rec = [n if layout == "plain" or n == 1 else n - max(1, n // 10) for n in n_in]
    real = [random_records(rng, n, TILE_POS_BITS, TILE_READ_BITS) for n in n_rec]
    guide_bases = [64 * (3 * s + 1) for s in range(len(n_in))]
    shift = 6 + sorted(SEGMENT_ORDERS).index(order)  # blocks of 64, 128, 256 slots
    slots, segs, fill = lay_out(real, n_in, guide_bases, rng, layout, fill_shift=shift, gap=7)
    off, span = mixed_table(5, 1, big=1 << 14, span=1 << TILE_POS_BITS)
    shift = shift if layout == "fill" else 0
    return SeedCase(off, span, TILE_POS_BITS, 0, TILE_READ_BITS, slots, segs, real, fill, shift).check_built()


# ------------------------------------------------------------------------------------------------ case 2: the XCD deal
XCD_TILES = (63, 64, 65, 71)
XCD_HOOKS = dict(sort_cap=2048)
XCD_SETTINGS = (-1, 0, 1)


@functools.lru_cache(maxsize=None)
def xcd_case(total_tiles):
    """One segment of 20 tiles and many of 1..3 tiles, total_tiles in all; every segment's last tile is partial."""
    rng = np.random.default_rng([12, total_tiles])
    tiles = [20]
    while sum(tiles) < total_tiles:
        tiles.append(min(int(rng.integers(1, 4)), total_tiles - sum(tiles)))
    tiles = [int(t) for t in rng.permutation(tiles)]
    n_in = [t * TILE - int(rng.integers(0, 4000)) for t in tiles]
    pos_bits, read_bits = 24, 6
    real = [random_records(rng, n, pos_bits, read_bits) for n in n_in]
    slots, segs, _ = lay_out(real, n_in, [64 * s for s in range(len(n_in))], rng, "plain")
    # the segments are listed in another order than they lie in memory, and the last one listed is followed by others'
    # records: whatever a workgroup reads past the last tile is somebody's records, not padding
    order = rng.permutation(len(n_in))
    if order[-1] == len(n_in) - 1:
        order = order[::-1]
    segs, real = segs[order], [real[i] for i in order]
    off, span = mixed_table(40, 2, big=1 << 16, span=1 << pos_bits)
    c = SeedCase(off, span, pos_bits, 0, read_bits, slots, segs, real).check_built()
    assert sum(c.tiles()) == total_tiles and max(c.tiles()) == 20
    return c


# ------------------------------------------------------------------------------------------------ case 3: exact capacities
CAP_HOOKS = dict(sort_cap=512)  # slot capacity derived: 640
CAP_POS_BITS, CAP_READ_BITS = 16, 6


@functools.lru_cache(maxsize=None)
def capacity_case(variant):
    """One segment of 128 (read, strand) groups; the first level's 7 bits make every group a bin.
    "slots"   groups of exactly 0, 1, 511, 512, 513, 639, 640 records among ordinary ones: no fallback, a second level
    "over"    the same with one group of 641: the slot partition falls back
    "within"  no group above 512: one level (what `n_src > cap` decides)"""
    rng = np.random.default_rng([13, ("slots", "over", "within").index(variant)])
    sizes = rng.integers(100, 301, size=128)
    special = {"slots": [0, 1, 511, 512, 513, 639, 640], "over": [0, 1, 511, 512, 513, 639, 641], "within": [0, 1, 511, 512, 510, 2, 512]}[variant]
    where = rng.permutation(128)[:len(special)]
    sizes[where] = special
    recs = []
    for g, n in enumerate(sizes):
        rel = rng.permutation(1 << CAP_POS_BITS)[:n].astype(U64)
        recs.append(records_from_keys(rng, (U64(g) << U64(CAP_POS_BITS)) | rel, CAP_POS_BITS, CAP_READ_BITS))
    real = [np.concatenate(recs)]
    slots, segs, _ = lay_out(real, [len(real[0])], [128], rng, "plain")
    off, span = mixed_table(3, 3, big=1 << 12, span=1 << CAP_POS_BITS)
    c = SeedCase(off, span, CAP_POS_BITS, 0, CAP_READ_BITS, slots, segs, real).check_built()
    c.note["sizes"] = sizes
    return c


# ------------------------------------------------------------------------------------------------ case 4: contig look-ups
LOOKUP_TABLES = (1, 4, 5, 64, 65, 512, 513, 100000)
LOOKUP_POS_BITS = 24
LOOKUP_BIG = 1 << 18  # the position range of a bin of the one-level layout: 7 of 25 key bits go to the level
LOOKUP_HOOKS = {"no-level": dict(), "one-level": dict(sort_cap=64)}
LOOKUP_PER_RANGE = 50  # records per range of LOOKUP_BIG positions in the one-level layout: 3 200 in all, 7 bits, bins <= 64
SIX_PATHS = {(t, r) for t in ("few", "many") for r in ("near", "lds", "global")}


@functools.lru_cache(maxsize=None)
def lookup_case(n_contigs, layout):
    """Records at contigs' first positions and at their last ones (the last position before the next contig; the table's
    last position for the last contig), one read, random strands.
    no-level   every contig of the table when that leaves the records within the last stage's 8 064, else the one-level sample
    one-level  of every range of LOOKUP_BIG positions at most ten contigs that start in it - its first and last among them -
               and random positions up to LOOKUP_PER_RANGE records per range: under sort_cap = 64 that is one level of 7 bits
               (strand and the top 6 position bits), so a bin's range is one of those ranges and it holds <= 50 records"""
    rng = np.random.default_rng([14, n_contigs, sorted(LOOKUP_HOOKS).index(layout)])
    off, span = mixed_table(n_contigs, 4, big=LOOKUP_BIG, span=1 << LOOKUP_POS_BITS)
    o = off.astype(np.int64)
    last = np.concatenate([o[1:], [span]]) - 1
    if layout == "no-level" and 2 * n_contigs <= 8000:
        pos = np.unique(np.concatenate([o, last]))
        chosen = np.arange(n_contigs)
    else:
        chosen = []
        for r in range(span // LOOKUP_BIG):
            inside = np.nonzero((o >= r * LOOKUP_BIG) & (o < (r + 1) * LOOKUP_BIG))[0]
            if len(inside) > 10:
                inside = np.unique(np.concatenate([inside[:1], inside[-1:], rng.permutation(inside[1:-1])[:8]]))
            chosen.append(inside)
        chosen = np.concatenate(chosen)
        assert 0 in chosen and n_contigs - 1 in chosen
        edge = np.unique(np.concatenate([o[chosen], last[chosen]]))
        pos = []
        for r in range(span // LOOKUP_BIG):
            mine = edge[(edge >= r * LOOKUP_BIG) & (edge < (r + 1) * LOOKUP_BIG)]
            assert len(mine) <= LOOKUP_PER_RANGE
            more = rng.permutation(np.setdiff1d(r * LOOKUP_BIG + rng.permutation(LOOKUP_BIG)[:4 * LOOKUP_PER_RANGE], mine))
            pos.append(np.concatenate([mine, more[:LOOKUP_PER_RANGE - len(mine)]]))
        pos = np.unique(np.concatenate(pos))
        assert len(pos) == LOOKUP_PER_RANGE * (span // LOOKUP_BIG)
    strand = rng.integers(0, 2, size=len(pos))
    mask = rng.integers(0, MASK23 + 1, size=len(pos))
    real = [pack(np.zeros(len(pos)), strand, pos, mask, LOOKUP_POS_BITS, 0)]
    # (a sentinel in the first slot: the no-level layout's range is everything whatever the last stage reads first)
    slots = np.concatenate([[U64(SENTINEL)], rng.permutation(real[0])])
    segs = np.array([(0, len(slots), 7)], dtype=SORT_SEGMENT_DTYPE)
    c = SeedCase(off, span, LOOKUP_POS_BITS, 0, 0, slots, segs, real).check_built()
    c.note["edges"] = (o, last, chosen)
    return c


# ------------------------------------------------------------------------------------------------ case 5: the top of the position field
TOP_HOOKS = {"defaults": dict(), "levels": dict(sort_cap=16, sort_max_bits=3)}
TOP_CASES = ("bits32", "base12", "bits1")


@functools.lru_cache(maxsize=None)
def top_case(name):
    """No record starts above 2^32 - 24: a window of 23 bases ends inside 32 bits, and the finalize kernel pads its staged
    contig starts with 0xFFFFFFFF, "a position no window has"."""
    rng = np.random.default_rng([15, TOP_CASES.index(name)])
    if name == "bits32":
        # 32 position bits over a table that spans 2^32 - 1 positions
        pos_bits, pos_base, read_bits, span = 32, 0, 2, (1 << 32) - 1
        off = np.array([0, 40, (1 << 31) - 30, 1 << 31, (1 << 32) - 5000, (1 << 32) - 60, (1 << 32) - 24], dtype=np.uint32)
        must = [0, (1 << 31) - 1, 1 << 31, (1 << 32) - 24, (1 << 32) - 25]
        pos = np.unique(np.concatenate([must, rng.integers(0, span - 23, size=300), (1 << 32) - 24 - rng.integers(0, 6000, size=200)]))
    elif name == "base12":
        # 12 position bits counted from 2^32 - 4096: the range's upper end saturates at the top of 32 bits
        pos_bits, pos_base, read_bits, span = 12, (1 << 32) - 4096, 2, 1 << 32
        off = np.array([0, (1 << 32) - 5000, (1 << 32) - 4096, (1 << 32) - 2000, (1 << 32) - 40, (1 << 32) - 24], dtype=np.uint32)
        pos = pos_base + np.unique(np.concatenate([[0, 1, 2095, 2096, 4055, 4056, 4071, 4072], rng.integers(0, 4073, size=400)]))
    else:
        # one position bit: positions 0 and 1, every read and strand
        pos_bits, pos_base, read_bits, span = 1, 0, 6, 2
        off = np.array([0, 1], dtype=np.uint32)
        pos = np.array([0, 1])
    recs = []
    for read in range(1 << read_bits):
        for strand in (0, 1):
            p = pos if name == "bits1" else pos[rng.random(len(pos)) < 0.5]
            if read == 0:
                p = pos
            recs.append(pack(np.full(len(p), read), np.full(len(p), strand), p, rng.integers(0, MASK23 + 1, size=len(p)), pos_bits, pos_base))
    real = [np.concatenate(recs)]
    slots, segs, _ = lay_out(real, [len(real[0]) + 9], [0xFFFFFF00], rng, "sentinel")
    c = SeedCase(off, span, pos_bits, pos_base, read_bits, slots, segs, real).check_built()
    c.note["pos"] = pos
    return c


# ------------------------------------------------------------------------------------------------ case 6: deep levels
DEEP_HOOKS = dict(sort_cap=16, sort_max_bits=1)


@functools.lru_cache(maxsize=None)
def deep_case():
    """3 000 consecutive positions of one read and strand among 64 reads' bits: 39 key bits, one per level."""
    rng = np.random.default_rng(16)
    pos = 0x9ABC0000 + 517 + np.arange(3000)
    real = [pack(np.full(3000, 41), np.ones(3000), pos, rng.integers(0, MASK23 + 1, size=3000), 32, 0)]
    slots, segs, _ = lay_out(real, [3000], [640], rng, "plain")
    off = np.array([0, 0x9ABC0000 + 600, 0x9ABC0000 + 640, 0x9ABC0000 + 3000], dtype=np.uint32)
    return SeedCase(off, (1 << 32) - 1, 32, 0, 6, slots, segs, real).check_built()


# ------------------------------------------------------------------------------------------------ case 7: ranking
RANK_SIZES = (1, 4, 5, 64, 700)


@functools.lru_cache(maxsize=None)
def ranking_case(twin):
    """One bin for the last stage under default hooks.
    twin False  pos_bits 32, 64 reads: 13 sub-bin bits (read, strand, the top 6 position bits), 26 bits left to rank on;
                clusters of 1, 4, 5, 64 and 700 positions inside one sub-bin each, about 8 000 records
    twin True   pos_bits 5: all 12 key bits are sub-bin bits (sub_bits < 13, low_bits == 0)"""
    rng = np.random.default_rng([17, int(twin)])
    if twin:
        pos_bits, read_bits = 5, 6
        real = [random_records(rng, 3000, pos_bits, read_bits)]
        off, span = np.array([0, 7, 30], dtype=np.uint32), 32
    else:
        pos_bits, read_bits = 32, 6
        sizes = [700] * 10 + [64] * 10 + [5] * 30 + [4] * 30 + [1] * 90
        groups = rng.permutation(1 << 13)[:len(sizes)]  # (read, strand, top 6 position bits)
        recs = []
        for g, n in zip(groups, sizes):
            low = int(rng.integers(0, (1 << 26) - n)) + np.arange(n)  # clustered: consecutive positions
            recs.append(records_from_keys(rng, (U64(int(g)) << U64(26)) | low.astype(U64), pos_bits, read_bits))
        real = [np.concatenate(recs)]
        off, span = mixed_table(700, 5, big=1 << 26, span=(1 << 32) - 1)
    slots, segs, _ = lay_out(real, [len(real[0])], [64], rng, "plain")
    return SeedCase(off, span, pos_bits, 0, read_bits, slots, segs, real).check_built()


# ------------------------------------------------------------------------------------------------ case 8: holes are not read
HOLE_HOOKS = {
    "no-level": dict(),
    "slot-level": dict(sort_cap=512, sort_optimistic=1),
    "exact-level": dict(sort_cap=512, sort_optimistic=0),
}


@functools.lru_cache(maxsize=None)
def holes_case():
    """Fill-table layout, blocks of 64: every slot of a hole holds a valid-looking record (bit 63 clear) with the key of a real
    record of its segment and another mask.  Blocks that hold nothing and full blocks among them; the last block of every
    segment is cut by n_in."""
    rng = np.random.default_rng(18)
    pos_bits, read_bits = 18, 6
    n_in = [5000, 64 * 40 + 17, 130, 7001]
    n_rec = [3100, 1500, 70, 5200]
    real = [random_records(rng, n, pos_bits, read_bits) for n in n_rec]

    def hole(s, k):
        dup = real[s][rng.integers(0, len(real[s]), size=k)]
        return (dup & ~U64(MASK23)) | ((dup & U64(MASK23)) ^ U64(1 + int(rng.integers(0, MASK23))))

    slots, segs, fill = lay_out(real, n_in, [0, 64, 0xFFFFFFC0, 4096], rng, "fill", fill_shift=6, hole=hole)
    off, span = mixed_table(9, 6, big=1 << 13, span=1 << pos_bits)
    c = SeedCase(off, span, pos_bits, 0, read_bits, slots, segs, real, fill, 6).check_built()
    assert np.all((slots >> U64(63)) == 0)
    return c


# ------------------------------------------------------------------------------------------------ case 9: the scan form
@dataclass
class ScanCase:
    contig_off: np.ndarray
    span: int
    pos_bits: int
    pos_base: int
    n_regions: int
    guide_base: int
    keys: np.ndarray
    vals: np.ndarray

    def reference(self):
        region = (self.keys >> U64(39)).astype(np.int64)
        parts = []
        for q in range(self.n_regions):
            k, v = self.keys[region == q], self.vals[region == q]
            high = (k >> U64(32)) & U64(127)  # read inside its region, strand
            rel = (k & U64(0xFFFFFFFF)) - U64(self.pos_base)
            recs = (((high << U64(32)) | (rel << U64(32 - self.pos_bits))) << U64(POS_SHIFT)) | (v.astype(U64) & U64(MASK23))
            assert len(np.unique(sort_keys(recs))) == len(recs)
            parts.append(unpack(np.sort(recs), self.guide_base + 64 * q, self.contig_off, self.pos_bits, self.pos_base))
        return np.concatenate(parts) if parts else np.zeros(0, dtype=HIT_DTYPE)

    def region_counts(self):
        return np.bincount((self.keys >> U64(39)).astype(np.int64), minlength=self.n_regions)

    def tile_regions(self):
        """Distinct regions per tile of 8 192 pairs."""
        region = (self.keys >> U64(39)).astype(np.int64)
        return [len(np.unique(region[t:t + TILE])) for t in range(0, len(region), TILE)]


SCAN_REGIONS = (1, 2, 5, 256)


@functools.lru_cache(maxsize=None)
def scan_case(n_regions):
    """More than 8 tiles of pairs; regions left empty first, last and in runs; the first tile belongs to one region alone;
    reads 0 and 63 of a region present; the largest guide_base the regions leave room for."""
    rng = np.random.default_rng([19, n_regions])
    pos_bits, pos_base = 20, 0
    full = {1: [0], 2: [1], 5: [1, 3], 256: [2, 3, 7, 8, 9, 100, 101, 200, 254]}[n_regions]
    n = 9 * TILE + 123
    sizes = rng.multinomial(n - TILE - 2 * len(full), np.ones(len(full)) / len(full))
    keys = []
    for q, m in zip(full, sizes):
        k = unique_keys(rng, int(m) + (TILE if q == full[0] else 0), pos_bits + 1 + REGION_BITS)
        ends = np.array([0, 63], dtype=U64) << U64(pos_bits + 1) | U64(5)  # reads & 63 of 0 and 63 (their keys made distinct below)
        k = np.unique(np.concatenate([k, ends]))
        read, rest = k >> U64(pos_bits + 1), k & U64((1 << (pos_bits + 1)) - 1)
        strand, rel = rest >> U64(pos_bits), rest & U64((1 << pos_bits) - 1)
        keys.append(rng.permutation(((U64(64 * q) + read) << U64(33)) | (strand << U64(32)) | (rel + U64(pos_base))))
    first = keys[0][:TILE]  # a tile of one region alone, then everything else in random order
    rest = rng.permutation(np.concatenate([keys[0][TILE:]] + keys[1:]))
    keys = np.concatenate([first, rest])
    mask = rng.integers(0, MASK23 + 1, size=len(keys)).astype(np.uint32)
    vals = (popcount(mask) << np.uint32(23)) | mask
    off, span = mixed_table(30, 7, big=1 << 15, span=1 << pos_bits)
    guide_base = (1 << 32) - 64 * n_regions
    return ScanCase(off, span, pos_bits, pos_base, n_regions, guide_base, keys, vals)
