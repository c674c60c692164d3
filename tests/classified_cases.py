"""Shared helpers of test_classified.py (GPU) and test_classified_cpu.py: the numpy aggregation and cut the classified sinks are
checked against, the record route (search + classify_hits), and a writer of synthetic forests in the exporter's format."""
import struct

import numpy as np

from varscot_amd import _lib
from varscot_amd.classifier import feature_names

NONE = (0xFFFFFFFF, 0, 0)


def votes_rows(guide, nm, votes, n_guides, n_trees):
    """The vsc_guide_votes rows of a table of counted hits (guide index, NM, votes per hit): plain sums."""
    guide, nm, votes = (np.asarray(a, dtype=np.int64) for a in (guide, nm, votes))
    rows = np.zeros(n_guides, dtype=_lib.VOTES_DTYPE)
    active, tie = 2 * votes > n_trees, 2 * votes == n_trees
    rows["votes_sum"] = np.bincount(guide, weights=votes, minlength=n_guides).astype(np.uint64)
    rows["active"] = np.bincount(guide[active], minlength=n_guides)
    rows["ties"] = np.bincount(guide[tie], minlength=n_guides)
    for k in range(9):
        rows["active_nm"][:, k] = np.bincount(guide[active & (nm == k)], minlength=n_guides)
    return rows


def counted(hits, exclude):
    """Mask of the hits that are not their guide's excluded locus ((contig, pos, strand) per guide, or None)."""
    keep = np.ones(len(hits), dtype=bool)
    if exclude is not None:
        ex = np.array(exclude, dtype=np.int64).reshape(-1, 3)
        g = hits["guide"].astype(np.int64)
        keep = ~((ex[g, 0] == hits["contig"]) & (ex[g, 1] == hits["pos"]) & (ex[g, 2] == (hits["info"] >> 31)))
    return keep


def rows_of_hits(hits, votes, n_guides, n_trees, exclude=None):
    keep = counted(hits, exclude)
    return votes_rows(hits["guide"][keep], (hits["info"][keep] >> 23) & 31, np.asarray(votes)[keep], n_guides, n_trees)


def by_result_order(h):
    return h[np.lexsort((h["pos"], h["contig"], h["info"] >> 31, h["guide"]))]


def cut_by_votes(hits, votes, top_k=0, min_votes=0, exclude=None, ranked=False):
    """The selection by votes on the host: the counted hits with votes >= min_votes, per guide the first top_k by (votes
    descending, strand, global position - contigs lie in order, so (contig, pos)), in result order (ranked: rank order)."""
    keep = counted(hits, exclude) & (np.asarray(votes) >= min_votes)
    h, v = hits[keep], np.asarray(votes, dtype=np.int64)[keep]
    order = np.lexsort((h["pos"], h["contig"], h["info"] >> 31, -v, h["guide"]))
    h, v = h[order], v[order]
    gg = h["guide"]
    rank = np.arange(len(h)) - np.searchsorted(gg, gg, side="left")
    if top_k:
        h, v = h[rank < top_k], v[rank < top_k]
    return (h, v) if ranked else by_result_order(h)


def record_route(gen, forest, guides, activity, m, algorithm, extra_pam=None):
    """(records, votes) the way the library offered them before the classified sinks: every record materialised, then classified."""
    h = gen.search(guides, m, extra_pam=extra_pam, algorithm=algorithm)
    rec = h.to_numpy().copy()
    votes = np.zeros(0, dtype=np.uint16)
    if len(rec):
        votes, _ = forest.classify_hits(h, activity)
    h.close()
    return rec, votes


SYNTHETIC_NAMES = ["totalMismatches", "seedMismatches", "adjacentMismatches", "transitionNumber", "transversionNumber", "mismatchPos3",
                   "mismatchPos17", "AtoC", "TtoG", "A1", "T20", "PAMG", "GG", "CA", "TT", "AA7", "CG19", "ontargetActivity"]
SYNTHETIC_ACTIVITIES = [0.2, 0.31, 0.5, 0.77, 0.9, 1.02, 1.4, 1.7]


def synthetic_forest(path, rng, n_trees=8, n_nodes=31, names=SYNTHETIC_NAMES):
    """A random forest file in the exporter's format: random binary trees grown breadth-first (randomForest's numbering: the
    daughters of a node are the next two free numbers) over predictors of the feature matrix, splits at x.5 and at integers, a
    few below zero and above every value, the activity split at a handful of thresholds."""
    assert set(names) <= set(feature_names())
    status = np.zeros((n_trees, n_nodes), dtype=np.int8)
    best = np.zeros((n_trees, n_nodes), dtype=np.uint8)
    left = np.zeros((n_trees, n_nodes), dtype="<u2")
    right = np.zeros((n_trees, n_nodes), dtype="<u2")
    split = np.zeros((n_trees, n_nodes), dtype="<f8")
    cls = np.zeros((n_trees, n_nodes), dtype=np.uint8)
    for t in range(n_trees):
        size = min(n_nodes, int(rng.integers(3, n_nodes + 1)) | 1)  # odd: every split adds two nodes
        nxt, k = 1, 0
        while k < nxt:  # nodes in creation order; nodes behind nxt do not exist
            if nxt + 2 <= size and (rng.random() < 0.9 or k == nxt - 1):
                status[t, k] = 1
                v = int(rng.integers(0, len(names)))
                best[t, k] = v + 1
                left[t, k], right[t, k] = nxt + 1, nxt + 2
                nxt += 2
                if names[v] == "ontargetActivity":
                    split[t, k] = float(rng.choice([0.31, 0.5, 0.77, 1.02, 1.4]))
                else:
                    split[t, k] = float(rng.choice([0.5, 0.5, 0.5, 1.5, 2.5, 1.0, 3.0, -0.5, 300.0]))
            else:
                status[t, k] = -1
                cls[t, k] = int(rng.integers(1, 3))
            k += 1
    with open(path, "wb") as f:
        f.write(b"VSCRF001" + struct.pack("<III", n_trees, n_nodes, len(names)))
        for n in names:
            f.write(struct.pack("<H", len(n)) + n.encode())
        for a in (status, best, left, right, split, cls):
            f.write(a.tobytes())


def oracle_votes(of, rows):
    """oracle/rf_oracle.py's walk (Forest.votes) over many rows at once: rows = float array [n, predictors in of.names order].
    Per tree every row descends with x[var] <= split ? left : right until its node is terminal."""
    n = len(rows)
    ones = np.zeros(n, dtype=np.int64)
    idx = np.arange(n)
    for t in range(of.n_trees):
        k = np.zeros(n, dtype=np.int64)
        status, var, left, right, split, cls = (a[t] for a in (of.status, of.best_var, of.left, of.right, of.split, of.node_class))
        live = status[k] != -1
        while live.any():
            kk = k[live]
            x = rows[idx[live], var[kk].astype(np.int64) - 1]
            k[live] = np.where(x <= split[kk], left[kk].astype(np.int64) - 1, right[kk].astype(np.int64) - 1)
            live = status[k] != -1
        ones += cls[k] == 2
    return ones
