"""vsc_search_summary / vsc_multi_search_summary on the device: per guide, NM counts, fixed-point MIT sums, reference-UB
counts and the excluded on-target - equal, field for field, to the aggregation of the hits the oracle (and vsc_search)
report, with the oracle's MIT scores rounded to rint(MIT * 2^24)."""
import os
import subprocess

import numpy as np
import pytest

import varscot_amd as va
from helpers import aggregate, make_genome, plant, random_guides, random_seq, revcomp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "varscot_amd", "bin")
FULL = int(np.rint(100.0 * 2 ** 24))  # a perfect match: MIT 100


@pytest.fixture(scope="module")
def ctx():
    c = va.Context(0)
    yield c
    c.close()


def oracle_summary(oracle, contigs, guides, m, extra_pam=None, exclude=None):
    want = oracle.search(contigs, guides, m, extra_pam=extra_pam, mode=oracle.MODE_PREDICATE)
    cache = {}
    mit, ub = np.zeros(len(want)), np.zeros(len(want), dtype=np.uint64)
    for i, info in enumerate(want["info"]):
        mask = int(info) & 0x7FFFFF
        if mask not in cache:
            cache[mask] = oracle.mit_score([b for b in range(23) if (mask >> b) & 1] or [-1])
        mit[i], ub[i] = cache[mask][0], cache[mask][1]
    return aggregate(want, len(guides), mit, ub, exclude), want


def device_summary(gen, guides, m, algo="seed", extra_pam=None):
    """The same rows from vsc_search + vsc_score_hits on the host."""
    hits = gen.search(guides, m, extra_pam=extra_pam, algorithm=algo)
    rec = hits.to_numpy()
    if len(rec):
        mit, flags, _ = hits.scores(mit=True)
    else:
        mit, flags = np.zeros(0), np.zeros(0, dtype=np.uint8)
    hits.close()
    return aggregate(rec, len(guides), mit, flags)


def planted(seed, n_guides, lens, m, pam=None):
    rng = np.random.default_rng(seed)
    guides = random_guides(rng, n_guides)
    if pam:
        guides[-1] = guides[-1][:21] + pam
    contigs = make_genome(seed, lens, guides, m, n_plant=60, n_runs=3)
    # one perfect site of guide 0 on each strand, away from the edges
    c0 = plant(rng, contigs[0], guides[0], 1000, "+", 0)
    contigs[0] = plant(rng, c0, guides[0], 3001, "-", 0)
    return guides, contigs


# ------------------------------------------------------------------------------------ parity with the oracle
@pytest.mark.parametrize("m", [0, 3, 4, 6, 8])
@pytest.mark.parametrize("algo", ["scan", "seed"])
@pytest.mark.parametrize("pam", [None, "TT"])
def test_summary_equals_oracle(ctx, oracle, m, algo, pam):
    guides, contigs = planted(500 + m, 8, [14000, 5000, 40], m, pam)
    want, hits = oracle_summary(oracle, contigs, guides, m, extra_pam=pam)
    assert len(hits) >= 2 and set((hits["info"] >> 31).tolist()) == {0, 1}  # both strands
    gen = ctx.load_genome(va.PackedGenome.from_sequences(contigs))
    got = gen.summarize(guides, m, extra_pam=pam, algorithm=algo)
    t = ctx.timing()
    assert t["algorithm"] == {"scan": 1, "seed": 2}[algo]
    assert t["sort_ms"] == 0 and t["hits"] == len(hits) and t["passes"] >= 1
    assert got.tobytes() == want.tobytes(), (got, want)
    gen.close()


def test_summary_equals_search_many_regions(ctx):
    """>= 20 Mbp and 2 000 guides at m = 8: every output region of the seed search (32 of 64 reads) in use."""
    rng = np.random.default_rng(77)
    guides = random_guides(rng, 2000)
    contigs = [random_seq(rng, 12_000_000), random_seq(rng, 8_500_000)]
    gen = ctx.load_genome(va.PackedGenome.from_sequences(contigs))
    got = gen.summarize(guides, 8, algorithm="seed")
    t = ctx.timing()
    assert t["algorithm"] == 2 and t["read_passes"] == 1
    want = device_summary(gen, guides, 8, "seed")
    assert int(want["nm"].sum()) > 500_000
    assert got.tobytes() == want.tobytes()
    gen.close()


def test_summary_equals_search_two_passes(ctx):
    rng = np.random.default_rng(78)
    guides = random_guides(rng, 16_500)
    contigs = make_genome(78, [300_000, 20_000], guides[::400], 3, n_plant=60)
    gen = ctx.load_genome(va.PackedGenome.from_sequences(contigs))
    for algo in ("scan", "seed"):
        got = gen.summarize(guides, 6, algorithm=algo)
        assert ctx.timing()["read_passes"] == 2
        want = device_summary(gen, guides, 6, algo)
        assert int(want["nm"].sum()) > 1000
        assert got.tobytes() == want.tobytes(), algo
    gen.close()


@pytest.mark.parametrize("algo", ["scan", "seed"])
def test_summary_after_overflow_counts_once(ctx, algo):
    """The genome of test_hit_buffer_overflow_is_retried: the first search overflows its buffer and runs again; only the
    second one is summarised."""
    g = "ACGTTGCATGCAAGTCCTAGTGG"
    contigs = [(g + "T") * 60000]
    gen = ctx.load_genome(va.PackedGenome.from_sequences(contigs))
    got = gen.summarize([g] * 40, 0, algorithm=algo)
    assert ctx.timing()["passes"] == 2
    assert np.all(got["nm"][:, 0] == 60000) and np.all(got["nm"][:, 1:] == 0)
    assert np.all(got["mit_sum"] == 60000 * FULL) and np.all(got["mit_ub"] == 0) and np.all(got["on_target"] == 0)
    gen.close()


# ------------------------------------------------------------------------------------ exclusion
@pytest.mark.parametrize("algo", ["scan", "seed"])
def test_summary_excludes_the_on_target(ctx, oracle, algo):
    guides, contigs = planted(601, 6, [14000, 5000], 4)
    gen = ctx.load_genome(va.PackedGenome.from_sequences(contigs))
    base, hits = oracle_summary(oracle, contigs, guides, 4)
    for strand, pos in ((0, 1000), (1, 3001)):
        ex = [(0xFFFFFFFF, 0, 0)] * len(guides)
        ex[0] = (0, pos, strand)
        want, _ = oracle_summary(oracle, contigs, guides, 4, exclude=ex)
        got = gen.summarize(guides, 4, algorithm=algo, exclude=ex)
        assert got.tobytes() == want.tobytes()
        assert got["on_target"][0] == 1 and got["nm"][0, 0] == base["nm"][0, 0] - 1
        assert got["mit_sum"][0] == base["mit_sum"][0] - FULL
        assert got[1:].tobytes() == base[1:].tobytes()
    # a locus that is not a hit (wrong strand, wrong position, past the contig end) changes nothing
    for miss in ((0, 1000, 1), (0, 1001, 0), (1, 4990, 0), (1, 1 << 30, 1)):
        got = gen.summarize(guides, 4, algorithm=algo, exclude=[miss] * len(guides))
        assert got.tobytes() == base.tobytes()
    # a contig the genome does not have
    with pytest.raises(va.VarscotError) as e:
        gen.summarize(guides, 4, algorithm=algo, exclude=[(2, 0, 0)] * len(guides))
    assert e.value.code == -22
    gen.close()


# ------------------------------------------------------------------------------------ shards
@pytest.mark.parametrize("algo", ["scan", "seed"])
def test_summary_over_shards_adds_up(ctx, oracle, algo):
    guides, contigs = planted(702, 8, [30000, 9000, 25], 6)
    packed = va.PackedGenome.from_sequences(contigs)
    whole = ctx.load_genome(packed)
    ex = [(0, 1000, 0)] + [(0xFFFFFFFF, 0, 0)] * (len(guides) - 1)
    want = whole.summarize(guides, 6, algorithm=algo, exclude=ex)
    whole.close()
    assert want.tobytes() == oracle_summary(oracle, contigs, guides, 6, exclude=ex)[0].tobytes()
    for world in (2, 3):
        total = np.zeros(len(guides), dtype=va.SUMMARY_DTYPE)
        for rank in range(world):
            b, e = packed.shard_words(rank, world)
            if e <= b:
                continue
            g = ctx.load_genome(packed, rank, world)
            part = g.summarize(guides, 6, algorithm=algo, exclude=ex)
            g.close()
            total["mit_sum"] += part["mit_sum"]
            total["nm"] += part["nm"]
            total["mit_ub"] += part["mit_ub"]
            total["on_target"] |= part["on_target"]
        assert total.tobytes() == want.tobytes(), world


@pytest.mark.parametrize("k", [1, 3, 8])
def test_multi_summary_equals_one_context(ctx, k):
    guides, contigs = planted(803, 10, [40000, 12000, 30], 6)
    packed = va.PackedGenome.from_sequences(contigs)
    ex = [(0, 3001, 1)] + [(0xFFFFFFFF, 0, 0)] * (len(guides) - 1)
    gen = ctx.load_genome(packed)
    want = {a: gen.summarize(guides, 6, algorithm=a, exclude=ex) for a in ("scan", "seed")}
    gen.close()
    m = va.MultiContext([0] * k)
    try:
        g = m.load_genome(packed)
        for a in ("scan", "seed"):
            got = g.summarize(guides, 6, algorithm=a, exclude=ex)
            assert got.tobytes() == want[a].tobytes(), a
            assert got["on_target"][0] == 1
        with pytest.raises(va.VarscotError):
            g.summarize(guides, 6, exclude=[(3, 0, 0)] * len(guides))
        g.close()
    finally:
        m.close()


# ------------------------------------------------------------------------------------ degenerate inputs, state
def test_summary_degenerate_inputs(ctx, oracle):
    guides, contigs = planted(904, 5, [9000, 3000], 3)
    gen = ctx.load_genome(va.PackedGenome.from_sequences(contigs))
    assert len(gen.summarize([], 3)) == 0
    assert len(gen.summarize([], 3, exclude=[])) == 0
    # no hits at all
    empty = ctx.load_genome(va.PackedGenome.from_sequences(["N" * 500 + random_seq(np.random.default_rng(1), 3000)]))
    for algo in ("scan", "seed"):
        got = empty.summarize(guides, 0, algorithm=algo)
        assert got.tobytes() == np.zeros(len(guides), dtype=va.SUMMARY_DTYPE).tobytes()
    empty.close()
    # N letters in a guide are searched as A (SeqAn's Dna conversion), as vsc_search does
    with_n = [guides[0][:5] + "N" + guides[0][6:]] + guides[1:]
    as_a = [with_n[0].replace("N", "A")] + guides[1:]
    got = gen.summarize(with_n, 3)
    assert got.tobytes() == gen.summarize(as_a, 3).tobytes()
    assert got.tobytes() == oracle_summary(oracle, contigs, as_a, 3)[0].tobytes()
    gen.close()


def test_summary_leaves_no_state(ctx):
    guides, contigs = planted(905, 12, [30000, 8000], 6)
    packed = va.PackedGenome.from_sequences(contigs)
    fresh = va.Context(0)
    try:
        g0 = fresh.load_genome(packed)
        want = {a: g0.search(guides, 6, algorithm=a) for a in ("scan", "seed")}
        want = {a: (h.to_numpy(), h.close())[0] for a, h in want.items()}
        g0.close()
    finally:
        fresh.close()
    gen = ctx.load_genome(packed)
    for a in ("scan", "seed"):
        s1 = gen.summarize(guides, 6, algorithm=a)
        s2 = gen.summarize(guides, 6, algorithm=a)
        assert s1.tobytes() == s2.tobytes()
        h = gen.search(guides, 6, algorithm=a)
        assert h.to_numpy().tobytes() == want[a].tobytes()
        assert ctx.timing()["sort_ms"] > 0
        h.close()
    gen.close()


# ------------------------------------------------------------------------------------ guide_summary
def _tsv(ids, seqs, rows, m):
    text = "#guideId\tguideSeq\tmitSpecScore\tofftargetCount\tonTargetFound\t" + "\t".join("mm%d" % k for k in range(m + 1))
    text += "\tmitHitSum\n"
    for i, s, r in zip(ids, seqs, rows):
        spec = int(np.floor(va.mit_specificity(int(r["mit_sum"])) + 0.5))
        text += "%s\t%s\t%d\t%d\t%d\t%s\t%.6f\n" % (i, s, spec, int(r["nm"].sum()), int(r["on_target"]),
                                                    "\t".join(str(int(x)) for x in r["nm"][:m + 1]), int(r["mit_sum"]) * 2.0 ** -24)
    return text


def test_guide_summary_tool(tmp_path, oracle):
    guides, contigs = planted(1006, 6, [15000, 6000, 40], 5)
    names = ["chr1 assembled", "chr2", "tiny"]
    with open(tmp_path / "g.fa", "w") as f:
        for n, s in zip(names, contigs):
            f.write(">%s\n%s\n" % (n, "\n".join(s[i:i + 60] for i in range(0, len(s), 60))))
    ids = ["g%d" % i for i in range(len(guides))]
    reads = list(guides)
    reads[3] = reads[3][:4] + "n" + reads[3][5:]
    with open(tmp_path / "r.fa", "w") as f:
        for i, s in zip(ids, reads):
            f.write(">%s\n%s\n" % (i, s))
    run = lambda *a: subprocess.run([os.path.join(BIN, a[0])] + list(a[1:]), capture_output=True, text=True, timeout=600)
    assert run("bidir_index", "-G", str(tmp_path / "g.fa"), "-I", str(tmp_path / "idx")).returncode == 0
    base = ["guide_summary", "-G", str(tmp_path / "g.fa"), "-I", str(tmp_path / "idx"), "-M", "5"]
    searched = [s.upper().replace("N", "A") for s in reads]
    # -R: every hit counts
    r = run(*base, "-R", str(tmp_path / "r.fa"), "-O", str(tmp_path / "r.tsv"))
    assert r.returncode == 0, r.stderr
    want = _tsv(ids, searched, oracle_summary(oracle, contigs, searched, 5)[0], 5)
    assert (tmp_path / "r.tsv").read_text() == want
    r = run(*base, "-R", str(tmp_path / "r.fa"), "-O", str(tmp_path / "r2.tsv"), "-D", "0,0")
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "r2.tsv").read_bytes() == (tmp_path / "r.tsv").read_bytes()
    # -B: the planted perfect sites of guide 0 as on-targets (both strands) + a locus that is no hit
    bed = "chr1\t1000\t1023\ton_plus\t0\t+\nchr1\t3001\t3024\ton_minus\t0\t-\nchr2\t100\t123\tnowhere\t0\t+\n"
    (tmp_path / "t.bed").write_text(bed)
    seqs = [contigs[0][1000:1023], revcomp(contigs[0][3001:3024]), contigs[1][100:123].replace("N", "A")]
    assert seqs[0] == guides[0] and seqs[1] == guides[0]
    ex = [(0, 1000, 0), (0, 3001, 1), (1, 100, 0)]
    r = run(*base, "-B", str(tmp_path / "t.bed"), "-O", str(tmp_path / "b.tsv"))
    assert r.returncode == 0, r.stderr
    want = _tsv(["on_plus", "on_minus", "nowhere"], seqs, oracle_summary(oracle, contigs, seqs, 5, exclude=ex)[0], 5)
    assert (tmp_path / "b.tsv").read_text() == want
    lines = want.splitlines()
    assert lines[1].split("\t")[4] == "1" and lines[2].split("\t")[4] == "1" and lines[3].split("\t")[4] == "0"
    r = run(*base, "-B", str(tmp_path / "t.bed"), "-O", str(tmp_path / "b2.tsv"), "-D", "0,0")
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "b2.tsv").read_bytes() == (tmp_path / "b.tsv").read_bytes()
