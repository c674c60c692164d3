"""Labels on the device (vsc_hits_locate, vsc_guides_locate): per record / candidate the interval of an annotation its window
lies in, against the brute force of the definition (tests/locate_cases.py) and the host's vsc_regions_locate - search results
of both algorithms, selections, empty and one-record results, the enumerated guides of the three-contig layout under the
annotations that make the lookup walk and search deep, the keyed device copy of a context, several devices, guide_summary -N."""
import os
import subprocess

import numpy as np
import pytest

import varscot_amd as va
from helpers import random_seq
from locate_cases import NONE, many_intervals, record_labels, staircase, whole_contig
from regions_cases import LENS, P_PLUS, annotation
from test_summary import planted

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "varscot_amd", "bin")
RULES = ["overlap", "inside"]
M = 8


@pytest.fixture(scope="module")
def ctx():
    c = va.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def case():
    guides, contigs = planted(500 + M, 8, LENS, M)
    return dict(guides=guides, contigs=contigs, packed=va.PackedGenome.from_sequences(contigs), iv=annotation(with_sites=True))


@pytest.fixture(scope="module")
def gen(ctx, case):
    g = ctx.load_genome(case["packed"])
    yield g
    g.close()


@pytest.fixture(scope="module")
def regs(case):
    r = {rule: va.Regions(case["packed"], case["iv"], rule=rule) for rule in RULES}
    yield r
    for x in r.values():
        x.close()


@pytest.fixture(scope="module")
def found(gen):
    """Every candidate guide of the layout (no regions at the enumerate step): 2 498, neither a multiple of 64 nor of 256, so
    the last wave and the last workgroup of the kernel are partly idle."""
    codes, loci = gen.enumerate_guides()
    assert len(loci) > 2000 and len(loci) % 64 != 0 and len(loci) % 256 != 0
    return codes, loci


def host_labels(reg, records):
    return np.array([reg.locate(int(c), int(p)) for c, p in zip(records["contig"], records["pos"])], dtype=np.uint32)


# ---- 1. hits ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["scan", "seed"])
def test_hits_are_labelled_as_the_definition_says(case, gen, regs, algo):
    hits = gen.search(case["guides"], M, algorithm=algo)
    rec = hits.to_numpy()
    assert len(rec) > 50 and set((rec["info"] >> 31).tolist()) == {0, 1}
    for rule in RULES:
        got = hits.locate(regs[rule])
        assert got.dtype == np.uint32 and len(got) == len(rec)
        assert np.array_equal(got, record_labels(case["iv"], rule, rec)), rule
        assert np.array_equal(got, host_labels(regs[rule], rec))
        assert (got == NONE).any() and (got != NONE).any()
        assert hits.to_numpy().tobytes() == rec.tobytes()  # the records are what they were
    hits.close()
    few = gen.search_select(case["guides"], M, top_k=5, algorithm=algo)
    rec = few.to_numpy()
    assert 8 < len(rec) <= 40
    for rule in RULES:
        assert np.array_equal(few.locate(regs[rule]), record_labels(case["iv"], rule, rec))
    few.close()


def test_empty_and_one_record_results(case, gen, regs):
    none = gen.search(["ACGTACGTACGTACGTACGTAGG"], 0)
    assert len(none) == 0
    got = none.locate(regs["overlap"])
    assert got.dtype == np.uint32 and len(got) == 0
    none.close()
    one = gen.search_select(case["guides"][:1], M, top_k=1)
    rec = one.to_numpy()
    assert len(rec) == 1
    # the best hit is the perfect '+' site at P_PLUS: one interval ends right at its window, one shares its last base
    # (regions_cases.site_intervals), so under overlap its label is the latter and under inside it has none
    assert (int(rec["contig"][0]), int(rec["pos"][0])) == (0, P_PLUS)
    at = {iv: i for i, iv in enumerate(case["iv"])}
    for rule in RULES:
        got = one.locate(regs[rule])
        assert np.array_equal(got, record_labels(case["iv"], rule, rec))
        assert got[0] == (at[(0, P_PLUS + 22, P_PLUS + 30)] if rule == "overlap" else NONE)
    one.close()


# ---- 2. guides --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", RULES)
def test_guides_are_labelled_as_the_definition_says(case, gen, regs, found, rule):
    info = regs[rule].info()
    assert info["blocks_in"] > 0 and info["blocks_mixed"] > 0 and info["blocks_out"] > 0, info
    codes, loci, labels = gen.enumerate_guides(labels=regs[rule])
    assert codes.tobytes() == found[0].tobytes() and loci.tobytes() == found[1].tobytes()
    assert np.array_equal(labels, record_labels(case["iv"], rule, loci))
    assert np.array_equal(labels, host_labels(regs[rule], loci))
    assert (labels == NONE).any() and len(set(labels.tolist())) > 50
    # labels=True: against the regions of the enumerate step - every candidate then has one
    c2, l2, lab2 = gen.enumerate_guides(regs[rule], labels=True)
    assert len(l2) > 0 and np.array_equal(lab2, record_labels(case["iv"], rule, l2)) and (lab2 != NONE).all()
    plain = gen.enumerate_guides(regs[rule])
    assert len(plain) == 2 and plain[0].tobytes() == c2.tobytes() and plain[1].tobytes() == l2.tobytes()
    with pytest.raises(ValueError):
        gen.enumerate_guides(labels=True)


def test_design_passes_labels_through(case, gen, regs):
    reg = regs["inside"]
    codes, loci, rows = gen.design(reg, 3)
    c2, l2, r2, labels = gen.design(reg, 3, labels=True)
    assert c2.tobytes() == codes.tobytes() and l2.tobytes() == loci.tobytes() and r2.tobytes() == rows.tobytes()
    assert len(labels) == len(loci) > 0 and np.array_equal(labels, record_labels(case["iv"], "inside", loci))


# ---- 3. the annotations that make the lookup walk, and a deep binary search ---------------------------------------------------
@pytest.mark.parametrize("rule", RULES)
def test_staircase_and_many_intervals_on_the_device(case, gen, found, rule):
    for iv in (staircase(), whole_contig(LENS[0], short=3), many_intervals()):
        reg = va.Regions(case["packed"], iv, rule=rule)
        labels = gen.enumerate_guides(labels=reg)[2]
        want = record_labels(iv, rule, found[1])
        bad = np.flatnonzero(labels != want)
        assert len(bad) == 0, (len(iv), bad[:10], labels[bad[:10]], want[bad[:10]])
        # (nothing lies inside the 3-base intervals: under that rule the whole-contig one is the only label)
        assert len(set(labels.tolist())) > (20 if len(iv) == 40 else 1 if len(iv) == 2001 and rule == "inside" else 1000)
        reg.close()
    assert len(many_intervals()) >= 5000


@pytest.mark.parametrize("rule", RULES)
def test_whole_contig_interval_before_2000_short_ones_on_the_device(ctx, rule):
    """Most candidates lie in the gaps between the short intervals: their label stands 2 000 entries back, one step up."""
    length = 90000
    packed = va.PackedGenome.from_sequences([random_seq(np.random.default_rng(90), length)])
    iv = whole_contig(length)
    reg = va.Regions(packed, iv, rule=rule)
    g = ctx.load_genome(packed)
    codes, loci, labels = g.enumerate_guides(labels=reg)
    g.close()
    reg.close()
    assert len(loci) > 5000 and len(loci) % 64 != 0
    assert np.array_equal(labels, record_labels(iv, rule, loci, [length]))
    assert (labels == 0).sum() > len(labels) // 4
    assert (labels > 0).any() if rule == "overlap" else set(labels.tolist()) == {0}


# ---- 4. the context's keyed device copy ---------------------------------------------------------------------------------------
def test_two_annotations_alternate_on_one_context(case, ctx, gen, regs, found):
    other_iv = many_intervals(600, seed=5)
    other = va.Regions(case["packed"], other_iv, rule="overlap")
    want = {0: record_labels(case["iv"], "overlap", found[1]), 1: record_labels(other_iv, "overlap", found[1])}
    assert not np.array_equal(want[0], want[1])
    for turn in range(4):
        reg = other if turn % 2 else regs["overlap"]
        assert np.array_equal(gen.enumerate_guides(labels=reg)[2], want[turn % 2]), turn
        if turn == 1:
            ctx.release_scratch()
    # the same regions in a summary (the sinks' copy) and then in a locate (the label structure beside it), and back
    hits = gen.search(case["guides"], M)
    rec = hits.to_numpy()
    rows = gen.summarize(case["guides"], M, regions=other)
    assert np.array_equal(hits.locate(other), record_labels(other_iv, "overlap", rec))
    again = gen.summarize(case["guides"], M, regions=other)
    assert again[0].tobytes() == rows[0].tobytes() and again[1].tobytes() == rows[1].tobytes()
    inside = hits.locate(other) != NONE
    assert np.array_equal(again[1]["nm"].sum(axis=1), np.bincount(rec["guide"][inside], minlength=len(case["guides"])))
    before = ctx.timing()
    hits.locate(regs["inside"])
    assert ctx.timing() == before  # a locate is not a search: the timing of the last one stays
    hits.close()
    other.close()


# ---- 5. several devices ---------------------------------------------------------------------------------------------------------
def test_multi_context_labels(case, gen, regs, found):
    single = gen.search(case["guides"], M)
    want = single.locate(regs["overlap"])
    rec = single.to_numpy()
    single.close()
    m = va.MultiContext([0, 0, 0])
    try:
        g = m.load_genome(case["packed"])
        merged = g.search(case["guides"], M)
        assert merged.to_numpy().tobytes() == rec.tobytes()
        assert np.array_equal(merged.locate(regs["overlap"]), want)  # on the result context
        merged.close()
        for rule in RULES:
            codes, loci, labels = g.enumerate_guides(labels=regs[rule])  # the host-only object: labelled on the host
            assert loci.tobytes() == found[1].tobytes()
            assert np.array_equal(labels, gen.enumerate_guides(labels=regs[rule])[2])
            c2, l2, lab2 = g.enumerate_guides(regs[rule], labels=True)
            one = gen.enumerate_guides(regs[rule], labels=True)
            assert l2.tobytes() == one[1].tobytes() and np.array_equal(lab2, one[2])
    finally:
        m.close()


# ---- 6. guide_summary -N --------------------------------------------------------------------------------------------------------
def test_guide_summary_names_the_regions(tmp_path, case, gen):
    guides, contigs = case["guides"], case["contigs"]
    chrom = ["chr1", "chr2", "tiny"]
    with open(tmp_path / "g.fa", "w") as f:
        for n, s in zip(["chr1 assembled", "chr2", "tiny"], contigs):
            f.write(">%s\n%s\n" % (n, "\n".join(s[i:i + 60] for i in range(0, len(s), 60))))
    with open(tmp_path / "r.fa", "w") as f:
        for i, s in enumerate(guides):
            f.write(">g%d\n%s\n" % (i, s))
    iv = case["iv"]
    coords = ["%s:%d-%d" % (chrom[k], a, b) for k, a, b in iv]
    names = [("exon%d" % i if i % 3 else None) for i in range(len(iv))]  # names on some lines only
    with open(tmp_path / "a.bed", "w") as f:
        f.write("# an annotation\ntrack name=test\n")
        for (k, a, b), n in zip(iv, names):
            f.write("%s\t%d\t%d%s\n" % (chrom[k], a, b, "\t%s\t0\t+" % n if n else ""))
    run = lambda *a: subprocess.run([os.path.join(BIN, a[0])] + list(a[1:]), capture_output=True, text=True, timeout=600)
    assert run("bidir_index", "-G", str(tmp_path / "g.fa"), "-I", str(tmp_path / "idx")).returncode == 0
    base = ["guide_summary", "-G", str(tmp_path / "g.fa"), "-I", str(tmp_path / "idx"), "-M", "4"]
    reads = ["-R", str(tmp_path / "r.fa")]
    # -A -T -N name: the last column is the label of the listed hit
    old = run(*base, *reads, "-A", str(tmp_path / "a.bed"), "-K", "6", "-T", str(tmp_path / "t0.tsv"))
    assert old.returncode == 0, old.stderr
    for mode, devices in (("name", "0"), ("coords", "0"), ("name", "0,0")):
        r = run(*base, *reads, "-A", str(tmp_path / "a.bed"), "-K", "6", "-T", str(tmp_path / "t1.tsv"), "-N", mode, "-D", devices)
        assert r.returncode == 0, r.stderr
        assert r.stdout == old.stdout
        a, b = (tmp_path / "t0.tsv").read_text().splitlines(), (tmp_path / "t1.tsv").read_text().splitlines()
        assert b[0] == a[0] + "\tregion" and [l.rsplit("\t", 1)[0] for l in b[1:]] == a[1:] and len(b) > 10
        listed = np.zeros(len(b) - 1, dtype=va.LOCUS_DTYPE)
        listed["contig"] = [chrom.index(l.split("\t")[2]) for l in b[1:]]
        listed["pos"] = [int(l.split("\t")[3]) for l in b[1:]]
        want = record_labels(iv, "overlap", listed)
        text = [("-" if w == NONE else (names[w] if mode == "name" and names[w] else coords[w])) for w in want.tolist()]
        assert [l.rsplit("\t", 1)[1] for l in b[1:]] == text
        assert "-" in text and any(t.startswith("exon") for t in text) == (mode == "name") and any(":" in t for t in text)
    # -E -L -N coords: column 7 is the target a guide was found in, columns 1-6 are what they were
    targets = [(0, 500, 1300), (1, 100, 400), (0, 13900, 14000), (0, 600, 700), (0, 600, 700)]
    (tmp_path / "t.bed").write_text("".join("%s\t%d\t%d\tT%d\n" % (chrom[k], a, b, i) for i, (k, a, b) in enumerate(targets)))
    discover = ["-E", str(tmp_path / "t.bed")]
    r0 = run(*base, *discover, "-L", str(tmp_path / "l0.bed"), "-O", str(tmp_path / "e0.tsv"))
    assert r0.returncode == 0, r0.stderr
    reg = va.Regions(case["packed"], targets, rule="inside")
    loci, labels = gen.enumerate_guides(reg, labels=True)[1:]
    reg.close()
    assert len(loci) > 20 and set(labels.tolist()) == {0, 1, 2, 3}
    for mode, devices in (("coords", "0"), ("name", "0"), ("coords", "0,0")):
        r1 = run(*base, *discover, "-L", str(tmp_path / "l1.bed"), "-O", str(tmp_path / "e1.tsv"), "-N", mode, "-D", devices)
        assert r1.returncode == 0, r1.stderr
        assert (tmp_path / "e1.tsv").read_bytes() == (tmp_path / "e0.tsv").read_bytes()
        a, b = (tmp_path / "l0.bed").read_text().splitlines(), (tmp_path / "l1.bed").read_text().splitlines()
        assert [l.rsplit("\t", 1)[0] for l in b] == a and len(a) == len(loci)
        want = [("%s:%d-%d" % (chrom[targets[w][0]], targets[w][1], targets[w][2]) if mode == "coords" else "T%d" % w) for w in labels.tolist()]
        assert [l.split("\t")[6] for l in b] == want
    # -N needs one of its two pairs of companions, and one of its two words
    assert run(*base, *reads, "-N", "name").returncode == 1
    assert run(*base, *reads, "-A", str(tmp_path / "a.bed"), "-N", "name").returncode == 1
    assert run(*base, *discover, "-N", "coords").returncode == 1
    assert run(*base, *reads, "-A", str(tmp_path / "a.bed"), "-T", str(tmp_path / "t2.tsv"), "-N", "gene").returncode == 1
