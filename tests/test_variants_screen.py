"""The variant-aware screen on the device (vsc_hits_variants, vsc_search_summary_variants, guide_summary -v) against the
merger's restatement (oracle/merge_oracle.py) on the scenario of tests/variants_cases.py."""
import os
import subprocess

import numpy as np
import pytest

import varscot_amd as va
import variants_cases as vc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "varscot_amd", "bin")
UNKNOWN = 0xFFFFFFFF
GRID = [(seed, m, sample) for seed in vc.SEEDS for m, sample in vc.CASES]


@pytest.fixture(scope="module")
def ctx():
    c = va.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def product(ctx, tmp_path_factory):
    """(scenario, reference PackedGenome, window PackedGenome, VariantMap, resident window genome) per (seed, sample), made once."""
    made = {}

    def get(seed, sample, which="vcf"):
        key = (seed, sample, which)
        if key not in made:
            sc = vc.scenario(seed)
            ref = va.PackedGenome.from_sequences(sc.seqs, sc.names)
            path = tmp_path_factory.mktemp("vcf") / "in.vcf"
            path.write_text(getattr(sc, which))
            win = va.variant_windows(ref, path, sample=sample, threads=2)
            assert list(win.names) == [w[0] for w in sc.windows(sample, which)]
            made[key] = (sc, ref, win, va.VariantMap(win, ref), ctx.load_genome(win))
        return made[key]
    yield get
    for _, _, _, vmap, gen in made.values():
        gen.close()
        vmap.close()


def expected_labels(sc, lab, with_on=True):
    """The oracle's verdicts (variants_cases.Case.label) as VARIANT_LABEL_DTYPE fields."""
    contig = np.array([sc.chroms.index(c) if c in sc.chroms else UNKNOWN for c in lab["chr"]], dtype=np.uint32)
    flags = lab["var"] * va.VARIANT_VAR + lab["dup"] * va.VARIANT_DUP + (lab["on"] * va.VARIANT_ON_TARGET if with_on else 0)
    return contig, lab["pos"], lab["n_var"], flags.astype(np.uint32)


def check_labels(got, want):
    for f, w in zip(("contig", "pos", "n_var", "flags"), want):
        assert np.array_equal(got[f], w), f


def check_rows(got, want, on_target=True):
    for f in ("nm", "mit_sum", "mit_ub") + (("on_target",) if on_target else ()):
        assert np.array_equal(got[f].astype(np.int64), want[f]), f


@pytest.mark.parametrize("algo", ["scan", "seed"])
@pytest.mark.parametrize("seed,m,sample", GRID)
def test_hits_variants_equal_the_merger(product, seed, m, sample, algo):
    sc, _, _, vmap, gen = product(seed, sample)
    case = sc.case(m, sample)
    fl = case.floors()
    assert all(fl[k] >= v for k, v in vc.FLOORS.items()), fl  # the scenario reaches every branch
    hits = gen.search(sc.guides, m, algorithm=algo)
    assert hits.to_numpy().tobytes() == case.hits.tobytes()
    check_labels(hits.variants(vmap, exclude=sc.loci), expected_labels(sc, case.label))
    without = hits.variants(vmap)  # nothing excluded: the on-target is a hit like any other
    check_labels(without, expected_labels(sc, case.label, with_on=False))
    hits.close()


def tiled(case, reps=3):
    """The case's guides `reps` times over, rotated so that a duplicate is the first record of a 256-record block of the
    kernel (its neighbour then lies in another workgroup): (guide order, expected label array).  A guide's records do not
    depend on the other guides, so the expectation is the per-guide blocks of the case put in that order."""
    g = case.hits["guide"]
    for r in range(vc.N_GUIDES):
        order = [(r + k) % vc.N_GUIDES for k in range(vc.N_GUIDES)] * reps
        idx = np.concatenate([np.flatnonzero(g == k) for k in order])
        lab = case.label[idx]
        if any(lab["dup"][i] for i in range(256, len(lab), 256)):
            return order, idx, lab
    raise AssertionError("no rotation puts a duplicate on a block boundary")


@pytest.mark.parametrize("seed,m,sample", GRID[:2])
def test_duplicates_across_workgroups_and_guide_runs_across_waves(product, seed, m, sample):
    sc, _, _, vmap, gen = product(seed, sample)
    case = sc.case(m, sample)
    order, idx, lab = tiled(case)
    assert len(lab) > 512
    guides = [sc.guides[k] for k in order]
    loci = [sc.loci[k] for k in order]
    hits = gen.search(guides, m)
    rec = hits.to_numpy()
    assert np.array_equal(rec["contig"], case.hits["contig"][idx]) and np.array_equal(rec["pos"], case.hits["pos"][idx])
    check_labels(hits.variants(vmap, exclude=loci), expected_labels(sc, lab))
    hits.close()
    rows, var, dups = gen.summarize_variants(guides, m, vmap, exclude=loci)
    for j, k in enumerate(order):
        for got, want in ((rows, case.rows_all), (var, case.rows_var)):
            assert got["nm"][j].tolist() == want["nm"][k].tolist() and int(got["mit_sum"][j]) == want["mit_sum"][k]
            assert int(got["on_target"][j]) == want["on_target"][k] and int(got["mit_ub"][j]) == want["mit_ub"][k]
        assert int(dups[j]) == case.dups[k]


@pytest.mark.parametrize("seed,m,sample", GRID)
def test_summarize_variants_equals_the_merger_for_every_batch_size(product, seed, m, sample):
    sc, _, _, vmap, gen = product(seed, sample)
    case = sc.case(m, sample)
    runs = [gen.summarize_variants(sc.guides, m, vmap, exclude=sc.loci, batch=b) for b in (0, 5, 1)]
    for rows, var, dups in runs:
        check_rows(rows, case.rows_all)
        check_rows(var, case.rows_var)
        assert np.array_equal(dups.astype(np.int64), case.dups)
    for other in runs[1:]:
        assert all(a.tobytes() == b.tobytes() for a, b in zip(runs[0], other))
    assert case.rows_all["on_target"].sum() >= 1 and case.dups.sum() >= vc.FLOORS["dup_adjacent"]
    t = gen.ctx.timing()
    assert t["hits"] > 0 and t["finalize_ms"] > 0 and t["read_passes"] == vc.N_GUIDES  # batch = 1: one pass per guide


@pytest.mark.parametrize("m,sample,algo", [(0, 0, "scan"), (8, 1, "seed")])
def test_summarize_variants_at_the_ends_of_the_mismatch_range(product, m, sample, algo):
    sc, _, _, vmap, gen = product(vc.SEEDS[0], sample)
    case = sc.case(m, sample)
    rows, var, dups = gen.summarize_variants(sc.guides, m, vmap, exclude=sc.loci, algorithm=algo)
    check_rows(rows, case.rows_all)
    check_rows(var, case.rows_var)
    assert np.array_equal(dups.astype(np.int64), case.dups)
    rows, var, dups = gen.summarize_variants(sc.guides, m, vmap)  # nothing excluded: the on-targets are counted
    assert int(rows["nm"].sum()) == int(case.counted.sum() + (case.label["on"] & ~case.label["dup"]).sum()) and not rows["on_target"].any()


@pytest.mark.parametrize("seed,m,sample", GRID)
def test_individual_rows_equal_the_mergers_own_output(ctx, product, seed, m, sample):
    """Both sides together: (reference rows - shadowed) + window rows == the per-guide sums of the TSV mergeResults prints."""
    sc, ref, _, vmap, gen = product(seed, sample)
    case = sc.case(m, sample)
    shadow = vmap.shadow()
    ref_gen = ctx.load_genome(ref)
    ref_all, ref_in = ref_gen.summarize(sc.guides, m, exclude=sc.loci, regions=shadow)
    ref_gen.close()
    shadow.close()
    win_all, _, _ = gen.summarize_variants(sc.guides, m, vmap, exclude=sc.loci)
    got = va.individual_rows(ref_all, ref_in, win_all)
    check_rows(got, case.merged, on_target=False)
    assert int(ref_in["nm"].sum()) >= vc.FLOORS["shadowed"] - vc.N_GUIDES  # (shadowed on-targets are counted in neither)
    assert got["on_target"].all()  # every guide was taken from the reference


def test_wrapped_window_start(ctx, product):
    sc, _, _, vmap, gen = product(vc.SEEDS[0], 0, "vcf_wrapped")
    hits = gen.search(sc.guides, 4)
    lab = hits.variants(vmap, exclude=sc.loci)
    rec = hits.to_numpy()
    for i in range(len(rec)):  # the host's answer per record
        want = vmap.locate(int(rec["contig"][i]), int(rec["pos"][i]))
        assert (int(lab["contig"][i]), int(lab["pos"][i]), int(lab["n_var"][i])) == (int(want["contig"]), int(want["pos"]), int(want["n_var"]))
    hits.close()


def test_refused_arguments(ctx, product):
    sc, _, _, vmap, gen = product(vc.SEEDS[0], 0)
    _, _, _, other_map, other_gen = product(vc.SEEDS[0], 1)
    hits = gen.search(sc.guides, 2)
    for call in (lambda: hits.variants(other_map),  # a map of another window genome
                 lambda: gen.summarize_variants(sc.guides, 2, other_map),
                 lambda: hits.variants(vmap, exclude=[(3, 0, 0)] * vc.N_GUIDES),  # a contig the reference does not have
                 lambda: gen.summarize_variants(sc.guides, 2, vmap, exclude=[(0, 0, 2)] * vc.N_GUIDES),  # a strand > 1
                 lambda: gen.summarize_variants(sc.guides, 9, vmap)):
        with pytest.raises(va.VarscotError) as e:
            call()
        assert e.value.code == -22
    hits.close()
    ctx.release_scratch()  # the map's device copy goes with the scratch and comes back
    rows, _, _ = gen.summarize_variants(sc.guides, 4, vmap, exclude=sc.loci)
    check_rows(rows, sc.case(4, 0).rows_all)


def _write_fasta(path, records):
    with open(path, "w") as f:
        for name, seq in records:
            f.write(">%s\n" % name)
            for i in range(0, len(seq), 60):
                f.write(seq[i:i + 60] + "\n")


def test_guide_summary_tool_with_a_vcf(tmp_path):
    seed, (m, sample) = vc.SEEDS[0], vc.CASES[1]
    sc = vc.scenario(seed)
    case = sc.case(m, sample)
    _write_fasta(tmp_path / "g.fa", sc.records)
    (tmp_path / "on.bed").write_text(sc.bed)
    (tmp_path / "in.vcf").write_text(sc.vcf)
    (tmp_path / "none.vcf").write_text(sc.vcf_no_alt)
    (tmp_path / "a.bed").write_text("chr1\t0\t1000\n")
    run = lambda *a: subprocess.run([os.path.join(BIN, a[0])] + list(a[1:]), capture_output=True, text=True, timeout=600)
    assert run("bidir_index", "-G", str(tmp_path / "g.fa"), "-I", str(tmp_path / "idx")).returncode == 0
    base = ["guide_summary", "-G", str(tmp_path / "g.fa"), "-I", str(tmp_path / "idx"), "-M", str(m), "-B", str(tmp_path / "on.bed")]
    plain = run(*base)
    assert plain.returncode == 0, plain.stderr
    r = run(*base, "-v", str(tmp_path / "in.vcf"), "-n", str(sample))
    assert r.returncode == 0, r.stderr
    old, new = [l.split("\t") for l in plain.stdout.splitlines()], [l.split("\t") for l in r.stdout.splitlines()]
    n_old = len(old[0])
    assert [l[:n_old] for l in new] == old  # the columns before the new ones are the run without -v
    assert new[0][n_old:] == (["indMitSpecScore", "indCount"] + ["imm%d" % k for k in range(m + 1)] + ["indMitHitSum", "varCount"] +
                              ["vmm%d" % k for k in range(m + 1)] + ["varMitHitSum", "varDuplicates"])
    merged = case.merged
    for g, line in enumerate(new[1:]):
        f = line[n_old:]
        assert line[0] == sc.guide_names[g]
        assert [int(x) for x in f[2:3 + m]] == merged["nm"][g][:m + 1].tolist() and int(f[1]) == int(merged["nm"][g].sum())
        assert f[3 + m] == "%.6f" % (int(merged["mit_sum"][g]) * 2.0 ** -24)
        assert int(f[0]) == int(np.floor(va.mit_specificity(int(merged["mit_sum"][g])) + 0.5))
        assert int(f[4 + m]) == int(case.rows_var["nm"][g].sum()) and [int(x) for x in f[5 + m:6 + 2 * m]] == case.rows_var["nm"][g][:m + 1].tolist()
        assert f[6 + 2 * m] == "%.6f" % (int(case.rows_var["mit_sum"][g]) * 2.0 ** -24) and int(f[7 + 2 * m]) == case.dups[g]
    # a sample without variants: the reference's numbers, zero variant columns
    r0 = run(*base, "-v", str(tmp_path / "none.vcf"))
    assert r0.returncode == 0, r0.stderr
    for line, was in zip(r0.stdout.splitlines()[1:], old[1:]):
        f = line.split("\t")
        assert f[:n_old] == was
        assert f[n_old] == was[2] and f[n_old + 1] == was[3] and f[n_old + 2:n_old + 3 + m] == was[5:6 + m] and f[n_old + 3 + m] == was[6 + m]
        assert all(x in ("0", "0.000000") for x in f[n_old + 4 + m:])
    # what -v does not combine with
    for extra in (["-A", str(tmp_path / "a.bed")], ["-T", str(tmp_path / "h.tsv")], ["-D", "0,0"],
                  ["-F", str(tmp_path / "f.vscrf"), "-C", str(tmp_path / "c.txt")]):
        bad = run(*base, "-v", str(tmp_path / "in.vcf"), *extra)
        assert bad.returncode == 1 and "-v" in bad.stderr, extra
    assert run(*base, "-n", "1").returncode == 1  # -n without -v
    assert run(*base, "-v", str(tmp_path / "in.txt")).returncode == 1
