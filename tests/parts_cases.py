"""Inputs of the tests that cut and lay out the seed search (test_search_parts.py, test_layouts.py) with the oracle's answer,
each made once a session and never changed."""
import numpy as np

import varscot_amd as va
from helpers import make_genome, mutate, oracle_hits, random_guides, random_seq

_built = {}


def once(key, make):
    if key not in _built:
        _built[key] = make()
        for v in _built[key]:
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return _built[key]


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


def repeat_rich_case(oracle):
    """70 guides (two regions), > 8 000 hits at m = 8; the oracle's records, computed once and never changed."""
    def make():
        guides, contigs = repeat_rich(4711, 70, 9000)
        want = oracle.search_fast(contigs, guides, 8)
        assert len(want) > 8000
        return guides, contigs, va.PackedGenome.from_sequences(contigs), want
    return once("repeat rich", make)


def repeat_rich_scores(oracle):
    """(MIT scores, UB flags) of the records of repeat_rich_case, from the oracle."""
    def make():
        guides, contigs, _, want = repeat_rich_case(oracle)
        hits, _, mit, ub = oracle_hits(oracle, contigs, guides, 8)  # (the plain search: the fast port's records are its own)
        assert hits.tobytes() == want.tobytes()
        return mit, ub
    return once("repeat rich scores", make)


OVERFLOW_G = "ACGTTGCATGCAAGTCCTAGTGG"
OVERFLOW_COPIES, OVERFLOW_UNITS = 40, 60000


def overflow_case(oracle):
    """The genome of test_hit_buffer_overflow_is_retried: 60 000 perfect sites of one 23-mer, 40 copies of it as reads, m = 0 -
    2 400 000 hits where the estimate for a random genome allows about a million."""
    def make():
        contigs = [(OVERFLOW_G + "T") * OVERFLOW_UNITS]
        guides = [OVERFLOW_G] * OVERFLOW_COPIES
        want = oracle.search_fast(contigs, guides, 0)
        assert len(want) == OVERFLOW_UNITS * OVERFLOW_COPIES and np.all(want["pos"] % 24 == 0) and np.all((want["info"] >> 23) == 0)
        return guides, va.PackedGenome.from_sequences(contigs), want
    return once("overflow", make)


MORE_READS_MARKED = [16383, 16384, 16385, 16384 + 300]


def more_reads_case(oracle):
    """The inputs of test_more_reads_than_one_pass_takes: 16 384 + 301 reads, planted sites for the reads on either side of the
    pass boundary."""
    def make():
        rng = np.random.default_rng(4242)
        guides = random_guides(rng, 16384 + 301)
        contigs = make_genome(4242, [120000, 50000], guides[:40], 5, n_plant=200, n_runs=3)
        seq = contigs[1]
        for k, gi in enumerate(MORE_READS_MARKED):
            at = 2000 + 300 * k
            seq = seq[:at] + mutate(rng, guides[gi], 2, 0, 20) + seq[at + 23:]
        contigs[1] = seq
        want = oracle.search_fast(contigs, guides, 5)
        assert {int(g) for g in want["guide"]} >= set(MORE_READS_MARKED)
        return guides, va.PackedGenome.from_sequences(contigs), want
    return once("more reads", make)


def no_hit_case(oracle):
    """70 random reads and a random genome that holds none of them: not one hit at m = 0."""
    def make():
        rng = np.random.default_rng(86)
        guides = random_guides(rng, 70)
        contigs = [random_seq(rng, 50000), random_seq(rng, 9000)]
        want = oracle.search_fast(contigs, guides, 0)
        assert len(want) == 0
        return guides, va.PackedGenome.from_sequences(contigs), want
    return once("no hit", make)


def few_hits_case(oracle):
    """70 reads (two regions) and a random genome with a handful of planted sites: at most 7 hits a region at m = 2, so that a
    region's records never span more than 7 of the search's blocks, whatever their size."""
    def make():
        from helpers import plant
        rng = np.random.default_rng(87)
        guides = random_guides(rng, 70)
        seq = random_seq(rng, 40000)
        for k, (g, strand, nsub) in enumerate(((3, "+", 0), (17, "-", 1), (40, "+", 2), (63, "-", 0), (3, "-", 2), (64, "+", 1), (69, "-", 0))):
            seq = plant(rng, seq, guides[g], 1000 + 5000 * k, strand, nsub)
        contigs = [seq, random_seq(rng, 3000)]
        want = oracle.search_fast(contigs, guides, 2)
        per_region = np.bincount(want["guide"] // 64, minlength=2)
        assert len(want) >= 7 and 0 < per_region[1] and per_region.max() <= 7, per_region
        return guides, va.PackedGenome.from_sequences(contigs), want
    return once("few hits", make)
