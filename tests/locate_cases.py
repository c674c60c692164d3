"""Shared by tests/test_locate_cpu.py and tests/test_locate.py: the label of a window by brute force - every (window, interval)
pair against the definition in include/varscot_hip.h, and of the intervals that qualify the minimum of the key
(-start, clipped end, input index), in numpy - and the annotations that make the lookup walk: a staircase of nested intervals,
one whole-contig interval in front of many short ones, and an annotation large enough for a deep binary search."""
import numpy as np

from regions_cases import LENS, WINDOW

NONE = 0xFFFFFFFF  # VSC_REGION_NONE


def brute_labels(intervals, rule, contig, positions, lens=LENS):
    """uint32 label per window start in `positions` (on `contig`): the index in `intervals` of the most specific interval the
    window is in under `rule`, NONE if there is none.  A window at the end of its contig is cut off there (it then lies
    inside nothing); an interval's end is clipped to the contig and an empty interval qualifies for nothing."""
    L = int(lens[contig])
    positions = np.asarray(positions, dtype=np.int64)
    idx = np.array([i for i, (k, a, b) in enumerate(intervals) if k == contig], dtype=np.int64)
    out = np.full(len(positions), NONE, dtype=np.uint32)
    if len(idx) == 0 or len(positions) == 0:
        return out
    s = np.array([intervals[i][1] for i in idx], dtype=np.int64)
    e = np.minimum(np.array([intervals[i][2] for i in idx], dtype=np.int64), L)
    keep = s < e
    idx, s, e = idx[keep], s[keep], e[keep]
    if len(idx) == 0:
        return out
    assert (L + 1) * (L + 1) * (len(intervals) + 1) < 2 ** 62
    key = ((L - s) * (L + 1) + e) * (len(intervals) + 1) + idx  # smallest: largest start, then smallest end, then lowest index
    big = np.int64(2 ** 62)
    for a in range(0, len(positions), 2048):
        pos = positions[a:a + 2048, None]
        if rule == "overlap":
            q = (s[None, :] < np.minimum(pos + WINDOW, L)) & (e[None, :] > pos)
        else:
            q = (s[None, :] <= pos) & (e[None, :] >= pos + WINDOW)
        j = np.where(q, key[None, :], big).argmin(axis=1)
        out[a:a + 2048] = np.where(q.any(axis=1), idx[j], NONE).astype(np.uint32)
    return out


def record_labels(intervals, rule, records, lens=LENS):
    """brute_labels per record of a HIT_DTYPE / LOCUS_DTYPE array (fields contig, pos)"""
    out = np.full(len(records), NONE, dtype=np.uint32)
    for c in range(len(lens)):
        k = np.flatnonzero(records["contig"] == c)
        out[k] = brute_labels(intervals, rule, c, records["pos"][k], lens)
    return out


def staircase(n=40, contig=0, first=1000, last=3000, step=10):
    """n nested intervals, starts rising and ends falling by `step`, in a shuffled order: a window near the right edge lies
    after every start and beyond most ends, so the lookup walks up through tens of enclosing intervals."""
    iv = [(contig, first + step * i, last - step * i) for i in range(n)]
    order = np.random.default_rng(17).permutation(n)
    return [iv[i] for i in order]


def whole_contig(length, n_short=2000, short=5):
    """The whole contig, given first, then n_short disjoint intervals of `short` bases spread evenly over it."""
    pitch = length // n_short
    assert pitch > short
    return [(0, 0, length)] + [(0, pitch * i + 1, pitch * i + 1 + short) for i in range(n_short)]


def many_intervals(n=6000, seed=23):
    """n short intervals (1 .. 60 bases) all over contigs 0 and 1: more than 2^12, so the binary search over the starts takes
    more than a dozen steps."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        c = int(rng.random() < 0.3)
        s = int(rng.integers(0, LENS[c] - 1))
        out.append((c, s, s + int(rng.integers(1, 61))))
    return out
