"""Shared by tests/test_regions_cpu.py and tests/test_regions.py: the three-contig layout, its annotation (random intervals,
hand-made edge cases) and the membership of every window by brute force - straight from the two definitions, in numpy."""
import numpy as np

LENS = [14000, 5000, 40]
WINDOW = 23
P_PLUS, P_MINUS = 1000, 3001  # tests/test_summary.py planted(): the perfect sites of guide 0 on contig 0, '+' and '-'

# (contig, start, end, note); every case sits in a stretch that the random intervals leave empty.  `pos` below = the window
# start the case is about.
HAND_MADE = [
    (0, 180, 200, "ends exactly at pos 200: out under both rules"),
    (0, 322, 330, "starts at pos + 22 for pos 300: overlaps by one base, contains nothing"),
    (0, 423, 430, "starts at pos + 23 for pos 400: out"),
    (0, 500, 523, "exactly [pos, pos + 23) for pos 500: in under both rules"),
    (0, 601, 624, "[pos + 1, pos + 24) for pos 600: overlaps, does not contain"),
    (0, 690, 710, "abuts the next one at 710 ..."),
    (0, 710, 740, "... the window at 700 spans the seam: overlaps, inside neither"),
    (0, 12100, 12600, "a long interval ..."),
    (0, 12200, 12210, "... that contains a later-starting short one: pos 12300 is inside the long one"),
    (2, 0, 40, "the whole 40-base contig"),
    (0, 13900, 14000, "up to the last base of contig 0: position 0 of contig 1 stays out"),
    (1, 4900, 9999, "end beyond the contig: clipped to 5000"),
    (1, 700, 700, "empty: dropped"),
]
# (contig, pos) -> (overlap, inside), worked out by hand from the definitions
EXPECT = {
    (0, 200): (0, 0), (0, 199): (1, 0), (0, 157): (0, 0), (0, 158): (1, 0),
    (0, 300): (1, 0), (0, 299): (0, 0),
    (0, 400): (0, 0), (0, 401): (1, 0),
    (0, 500): (1, 1), (0, 499): (1, 0), (0, 501): (1, 0),
    (0, 600): (1, 0), (0, 601): (1, 1),
    (0, 700): (1, 0), (0, 690): (1, 0), (0, 710): (1, 1), (0, 717): (1, 1), (0, 718): (1, 0),
    (0, 12300): (1, 1), (0, 12577): (1, 1), (0, 12578): (1, 0), (0, 12600): (0, 0),
    (2, 0): (1, 1), (2, 17): (1, 1), (2, 18): (1, 0), (2, 39): (1, 0),
    (0, 13999): (1, 0), (0, 13977): (1, 1), (0, 13978): (1, 0), (1, 0): (0, 0),
    (1, 4977): (1, 1), (1, 4978): (1, 0), (1, 4999): (1, 0), (1, 4877): (0, 0), (1, 4878): (1, 0),
    (1, 700): (0, 0), (1, 690): (0, 0),
}


def random_intervals(seed=11, n=400):
    """n intervals of length 1 .. 3000 (log-uniform: many short, some long, overlapping and nested), starting in
    contig 0 [4000, 9000) or contig 1 [1000, 3000); unsorted."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        ln = int(np.exp(rng.uniform(0.0, np.log(3000.0))))
        ln = min(max(ln, 1), 3000)
        if rng.random() < 0.7:
            s = int(rng.integers(4000, 9000))
            out.append((0, s, s + ln))
        else:
            s = int(rng.integers(1000, 3000))
            out.append((1, s, s + ln))
    return out


def site_intervals():
    """The edge rules again around the two planted perfect sites of planted(): P_PLUS is touched by one base (overlap only),
    P_MINUS is fitted exactly (both rules), each with a neighbour that ends or starts right at the window."""
    p, q = P_PLUS, P_MINUS
    return [(0, p - 20, p), (0, p + 22, p + 30), (0, q, q + WINDOW), (0, q + WINDOW, q + 40)]


def annotation(with_sites=False):
    iv = random_intervals() + [c[:3] for c in HAND_MADE] + (site_intervals() if with_sites else [])
    order = np.random.default_rng(5).permutation(len(iv))  # the library must not rely on any input order
    return [iv[i] for i in order]


def brute_force(intervals, lens=LENS):
    """{rule: [bool array over the positions of contig c]}: every (position, interval) pair against the definition.  A window
    at the end of its contig is cut off there; an interval's end is clipped to the contig."""
    out = {"overlap": [], "inside": []}
    for c, L in enumerate(lens):
        s = np.array([a for k, a, b in intervals if k == c], dtype=np.int64)
        e = np.minimum(np.array([b for k, a, b in intervals if k == c], dtype=np.int64), L)
        keep = s < e
        s, e = s[keep], e[keep]
        pos = np.arange(L, dtype=np.int64)[:, None]
        wend = np.minimum(pos + WINDOW, L)
        out["overlap"].append(((s[None, :] < wend) & (e[None, :] > pos)).any(axis=1))
        out["inside"].append(((s[None, :] <= pos) & (e[None, :] >= pos + WINDOW)).any(axis=1))
    return out


def member(table, hits):
    """bool per record (HIT_DTYPE): is its window in the regions, by the brute-force table of one rule"""
    m = np.zeros(len(hits), dtype=bool)
    for c in range(len(table)):
        k = hits["contig"] == c
        m[k] = table[c][hits["pos"][k].astype(np.int64)]
    return m
