"""The genome of tests/test_sink_walk.py with the oracle's hits, scores and votes on it: a region of reads that spans several tiles
of the sinks, an output region without any record, regions of one short tile each and a last region of fewer than 64 reads.
Shared by the tests that run the record sinks over it (test_sink_walk.py, test_layouts.py, test_search_parts.py); built once a
session and never changed."""
import numpy as np

import varscot_amd as va
from classified_cases import SYNTHETIC_ACTIVITIES, cut_by_votes, oracle_votes, rows_of_hits
from helpers import aggregate, cut, inside_numpy, make_genome, oracle_hits, plant, random_guides, revcomp, select, selected
from varscot_amd.classifier import DEFAULT_MODEL, Forest, feature_names

G = "ACGTTGCATGCAAGTCCTAGTGG"  # the 23-mer of test_summary_after_overflow_counts_once
COPIES = 3000
SUM_TILE = 2048       # kSumTile (vsc_internal.h): record slots per tile of the sinks
REGION_READS = 64     # kRegionReads: reads per output region of the seed search
N_GUIDES = 200        # four regions, the last one of 8 reads
M = 2
NONE = (0xFFFFFFFF, 0, 0)

_built = {}


def sink_walk_case(oracle):
    """The genome, the oracle's hits with their scores and the oracle forest's votes - computed once, never changed."""
    if "case" not in _built:
        _built["case"] = _build(oracle)
        for v in _built["case"].values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return _built["case"]


def _build(oracle):
    from oracle.rf_oracle import Forest as OracleForest
    rng = np.random.default_rng(4242)
    guides = random_guides(rng, N_GUIDES)
    for i in (0, 5, 17):  # three reads of region 0 share the repeat: its segment spans several tiles
        guides[i] = G
    # a few near-matches of reads of regions 2 and 3 only; reads 64 .. 127 get none
    late = guides[2 * REGION_READS:]
    spots = make_genome(977, [6000], late, M, n_plant=12, n_runs=1)[0]
    for g, pos, strand, nsub in ((130, 500, "+", 1), (150, 900, "-", 2), (191, 1300, "+", 0), (192, 1700, "+", 0), (199, 2100, "-", 2)):
        spots = plant(rng, spots, guides[g], pos, strand, nsub)
    contigs = [(G + "T") * COPIES, spots]
    hits, score, mit, ub = oracle_hits(oracle, contigs, guides, M)
    region = hits["guide"] // REGION_READS
    per_region = np.bincount(region, minlength=4)
    print("hits per output region:", per_region.tolist())
    # the case is the one described
    assert per_region[0] > SUM_TILE and per_region[0] >= 3 * COPIES
    assert per_region[1] == 0
    assert 0 < per_region[2] < SUM_TILE and 0 < per_region[3] < SUM_TILE
    act = rng.choice(SYNTHETIC_ACTIVITIES, size=N_GUIDES)
    # the oracle forest over the oracle's feature rows, as test_classified.py computes them (equal rows walk the forest once)
    of = OracleForest(DEFAULT_MODEL)
    cols = {n: i for i, n in enumerate(feature_names())}
    x = np.zeros((len(hits), 443))
    cache = {}
    for i, h in enumerate(hits):
        off = contigs[h["contig"]][h["pos"]:h["pos"] + 23]
        key = (guides[h["guide"]], revcomp(off) if h["info"] >> 31 else off)
        if key not in cache:
            cache[key] = oracle.feature_row(*key)
        x[i, :442] = cache[key]
        x[i, 442] = act[h["guide"]]
    rows, inverse = np.unique(x[:, [cols[n] for n in of.names]], axis=0, return_inverse=True)
    votes = oracle_votes(of, rows)[inverse.ravel()]
    for i in range(0, len(hits), max(1, len(hits) // 12)):  # a sample through the oracle's own loop
        assert votes[i] == of.votes({n: x[i, cols[n]] for n in of.names})
    return dict(guides=guides, contigs=contigs, packed=va.PackedGenome.from_sequences(contigs), hits=hits, score=score, mit=mit, ub=ub,
                act=act, votes=votes, n_trees=of.n_trees)


# one interval cuts through the repeat (in the middle of a copy), one holds some of the planted sites
INTERVALS = np.array([(0, 10_000, 30_011), (1, 400, 1500)], dtype=np.int64)


def every_sink_equals_the_oracle(ctx, gen, c, algorithm, after=lambda: None):
    """Every record sink over the resident genome `gen` of the case `c` against the oracle; after() runs behind every call
    of the library (a test that has set a layout proves there that the call used it)."""
    guides, hits, n = c["guides"], c["hits"], len(c["guides"])
    forest = Forest(DEFAULT_MODEL)
    # summary, one copy of the repeat excluded for one of the three reads that share it
    ex = [NONE] * n
    ex[5] = (0, 24, 0)  # the second copy: among the read's three best
    want = aggregate(hits, n, c["mit"], c["ub"], ex)
    assert want["on_target"].sum() == 1 and want["nm"][5, 0] == want["nm"][0, 0] - 1
    got = gen.summarize(guides, M, algorithm=algorithm, exclude=ex)
    after()
    assert ctx.timing()["hits"] == len(hits)
    assert got.tobytes() == want.tobytes()
    # summary with regions: one interval cuts through the repeat (in the middle of a copy), one holds some of the planted sites
    iv = INTERVALS
    for rule in ("overlap", "inside"):
        inside = inside_numpy(c["packed"], iv, rule, hits)
        assert inside[hits["contig"] == 0].any() and not inside[hits["contig"] == 0].all() and inside[hits["contig"] == 1].any()
        reg = va.Regions(c["packed"], iv, rule=rule)
        got_all, got_in = gen.summarize(guides, M, algorithm=algorithm, regions=reg)
        after()
        reg.close()
        assert got_all.tobytes() == aggregate(hits, n, c["mit"], c["ub"]).tobytes(), rule
        assert got_in.tobytes() == aggregate(hits[inside], n, c["mit"][inside], c["ub"][inside]).tobytes(), rule
    # votes summary
    _, rows = gen.summarize_classified(guides, M, forest, c["act"], algorithm=algorithm)
    after()
    want = rows_of_hits(hits, c["votes"], n, c["n_trees"])
    for f in want.dtype.names:
        assert np.array_equal(rows[f], want[f]), f
    # selection by MIT score with the excluded locus, selection by votes
    got = select(gen, guides, M, top_k=3, exclude=ex, algorithm=algorithm)
    after()
    assert got.tobytes() == cut(hits, c["score"], 3, 0, exclude=ex).tobytes()
    got = selected(gen, guides, M, forest, c["act"], top_k=3, algorithm=algorithm)
    after()
    assert got.tobytes() == cut_by_votes(hits, c["votes"], 3).tobytes()
