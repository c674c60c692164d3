"""The variant-aware pattern screen on the device (vsc_pattern_hits_variants, vsc_pattern_hits_shadowed,
vsc_search_pattern_variants) against the mergers' restatement on the scenario of tests/pattern_variants_cases.py."""
import ctypes as C

import numpy as np
import pytest

import varscot_amd as va
import pattern_cases as pc
import pattern_table_cases as ptc
import pattern_variants_cases as pv
import variants_cases as vc

pytestmark = pytest.mark.gpu

UNKNOWN = 0xFFFFFFFF
SHAPES = list(pv.SHAPES)
ROW_KINDS = ("ref", "win", "var")


@pytest.fixture(scope="module")
def ctx():
    c = va.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def product(ctx, tmp_path_factory):
    """(scenario, VariantMap, resident reference, resident window genome, PatternTable) per (shape, which vcf), made once."""
    made = {}

    def get(shape, which="vcf"):
        key = (shape, which)
        if key not in made:
            sc = pv.scenario(shape)
            ref = va.PackedGenome.from_sequences(sc.seqs, sc.names)
            path = tmp_path_factory.mktemp("vcf") / "in.vcf"
            path.write_text(getattr(sc, which))
            win = va.variant_windows(ref, path, sample=0, seq_len=sc.L, threads=2)
            windows = sc.windows(0, which)
            assert list(win.names) == [w[0] for w in windows]
            # the bit offsets the floors count (straddle, bit0) are the device's
            assert [int(x) for x in win.contigs["offset"]] == pv.plane_offsets([len(w[1]) for w in windows])
            made[key] = (sc, va.VariantMap(win, ref), ctx.load_genome(ref), ctx.load_genome(win), ptc.make_table(va, sc.table), win)
        return made[key][:5]
    yield get
    for _, vmap, ref_gen, win_gen, table, _ in made.values():
        ref_gen.close()
        win_gen.close()
        vmap.close()
        table.close()


def expected_labels(sc, lab, with_on=True):
    """The restatement's verdicts (pattern_variants_cases.Case.label) as VARIANT_LABEL_DTYPE fields."""
    contig = np.array([sc.chroms.index(c) if c in sc.chroms else UNKNOWN for c in lab["chr"]], dtype=np.uint32)
    flags = lab["var"] * va.VARIANT_VAR + lab["dup"] * va.VARIANT_DUP + (lab["on"] * va.VARIANT_ON_TARGET if with_on else 0)
    return contig, lab["pos"], lab["n_var"], flags.astype(np.uint32)


def check_labels(got, want):
    for f, w in zip(("contig", "pos", "n_var", "flags"), want):
        assert np.array_equal(got[f], w), (f, np.flatnonzero(got[f] != w)[:8])


def check_rows(got, want, table):
    """The screen's dict against Case.rows()."""
    for kind in ROW_KINDS:
        for f in ("count", "on_target", "dropped"):
            assert np.array_equal(got[kind][f].astype(np.int64), want[kind][f]), (kind, f)
        if table:
            for f in ("score_sum", "positive", "positive_nm"):
                assert np.array_equal(got[kind + "_table"][f].astype(np.int64), want[kind][f]), (kind, f)
            assert not got[kind + "_table"]["reserved"].any()
        else:
            assert got[kind + "_table"] is None


def screen_bytes(got):
    return b"".join(got[k].tobytes() for k in sorted(got) if got[k] is not None)


@pytest.mark.parametrize("shape", SHAPES)
def test_labels_and_flags_equal_the_restatement(product, shape):
    sc, vmap, ref_gen, win_gen, _ = product(shape)
    case = sc.case()
    hits = win_gen.search_pattern_hits(sc.pattern, sc.guides, pv.M)
    assert hits.to_numpy().tobytes() == case.win_rec.tobytes()
    check_labels(hits.variants(vmap, exclude=sc.loci), expected_labels(sc, case.label))
    check_labels(hits.variants(vmap), expected_labels(sc, case.label, with_on=False))  # nothing excluded
    hits.close()
    hits = ref_gen.search_pattern_hits(sc.pattern, sc.guides, pv.M)
    assert hits.to_numpy().tobytes() == case.ref_rec.tobytes()
    want = case.ref_shadowed * va.PATTERN_REF_SHADOWED
    assert np.array_equal(hits.shadowed(vmap), want)
    assert np.array_equal(hits.shadowed(vmap, exclude=sc.loci), want + case.ref_on * va.PATTERN_REF_ON_TARGET)
    assert case.ref_on.sum() == pv.N_GUIDES
    hits.close()


@pytest.mark.parametrize("tabled", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_screen_rows_equal_the_restatement_for_every_chunk_and_batch(product, shape, tabled):
    sc, vmap, ref_gen, win_gen, table = product(shape)
    case = sc.case()
    runs = [va.pattern_variants_screen(ref_gen, win_gen, vmap, sc.pattern, sc.guides, pv.M, table=table if tabled else None,
                                       exclude=sc.loci, chunk=chunk, guide_batch=batch) for chunk in (0, 5, 1) for batch in (0, 3)]
    for got in runs:
        check_rows(got, case.rows(True), tabled)
    assert all(screen_bytes(got) == screen_bytes(runs[0]) for got in runs[1:])
    t = ref_gen.ctx.timing()
    assert t["hits"] == len(case.ref_hits) + len(case.win_hits) and t["finalize_ms"] > 0
    ind = va.individual_pattern_rows(runs[0]["ref"], runs[0]["win"])
    assert np.array_equal(ind["count"].astype(np.int64), case.individual()["count"]) and not ind["dropped"].any()
    if tabled:
        ind = va.individual_pattern_rows(runs[0]["ref_table"], runs[0]["win_table"])
        for f in ("score_sum", "positive", "positive_nm"):
            assert np.array_equal(ind[f].astype(np.int64), case.individual()[f]), f
    # nothing excluded: the on-targets are counted
    got = va.pattern_variants_screen(ref_gen, win_gen, vmap, sc.pattern, sc.guides, pv.M, table=table if tabled else None)
    check_rows(got, case.rows(False), tabled)
    assert not got["ref"]["on_target"].any() and not got["win"]["on_target"].any()


def tiled(case, reps=3):
    """The case's guides `reps` times over, rotated so that a duplicate is the first record of a 256-record block of the
    kernel (its neighbour then lies in another workgroup): (guide order, record indices).  A guide's records do not depend on
    the other guides, so the expectation is the per-guide blocks of the case put in that order."""
    g = case.win_rec["guide"]
    for r in range(pv.N_GUIDES):
        order = [(r + k) % pv.N_GUIDES for k in range(pv.N_GUIDES)] * reps
        idx = np.concatenate([np.flatnonzero(g == k) for k in order])
        if any(case.label["dup"][idx[i]] for i in range(256, len(idx), 256)):
            return order, idx
    raise AssertionError("no rotation puts a duplicate on a block boundary")


@pytest.mark.parametrize("shape", ["sa", "longsa"])
def test_duplicates_across_workgroups_and_guide_runs_across_waves(product, shape):
    sc, vmap, ref_gen, win_gen, table = product(shape)
    case = sc.case()
    order, idx = tiled(case)
    assert len(idx) > 512
    run_of = np.concatenate([np.full(int((case.win_rec["guide"] == k).sum()), j) for j, k in enumerate(order)])  # tiled guide per record
    first = np.flatnonzero(np.diff(run_of, prepend=-1))
    last = np.concatenate([first[1:], [len(run_of)]]) - 1
    assert any(a // 64 != b // 64 for a, b in zip(first, last))  # a guide's run crosses a wave boundary
    guides, loci = [sc.guides[k] for k in order], [sc.loci[k] for k in order]
    hits = win_gen.search_pattern_hits(sc.pattern, guides, pv.M, table=table)
    rec = hits.to_numpy()
    assert np.array_equal(rec["contig"], case.win_rec["contig"][idx]) and np.array_equal(rec["pos"], case.win_rec["pos"][idx])
    assert np.array_equal(hits.scores(), case.win_f[idx])
    check_labels(hits.variants(vmap, exclude=loci), expected_labels(sc, case.label[idx]))
    hits.close()
    got = va.pattern_variants_screen(ref_gen, win_gen, vmap, sc.pattern, guides, pv.M, table=table, exclude=loci)
    want = case.rows(True)
    for j, k in enumerate(order):
        for kind in ROW_KINDS:
            for f in ("count", "on_target", "dropped"):
                assert np.array_equal(got[kind][f][j].astype(np.int64), want[kind][f][k]), (kind, f, j)
            for f in ("score_sum", "positive", "positive_nm"):
                assert np.array_equal(got[kind + "_table"][f][j].astype(np.int64), want[kind][f][k]), (kind, f, j)


@pytest.mark.parametrize("m", [0, 8])
def test_the_ends_of_the_mismatch_range(product, m):
    sc, vmap, ref_gen, win_gen, table = product("sa")
    case = sc.case(m)
    hits = win_gen.search_pattern_hits(sc.pattern, sc.guides, m)
    assert hits.to_numpy().tobytes() == case.win_rec.tobytes()
    check_labels(hits.variants(vmap, exclude=sc.loci), expected_labels(sc, case.label))
    hits.close()
    check_rows(va.pattern_variants_screen(ref_gen, win_gen, vmap, sc.pattern, sc.guides, m, table=table, exclude=sc.loci), case.rows(True), True)
    assert case.rows(True)["win"]["count"][:, m].sum() > 0 or m == 0


def test_scored_rows_are_the_sums_of_the_counted_records_f_words(product):
    sc, vmap, ref_gen, win_gen, table = product("cas12a")
    got = va.pattern_variants_screen(ref_gen, win_gen, vmap, sc.pattern, sc.guides, pv.M, table=table, exclude=sc.loci)
    for gen, kind in ((ref_gen, "ref"), (win_gen, "win")):
        hits = gen.search_pattern_hits(sc.pattern, sc.guides, pv.M, table=table)
        rec, f = hits.to_numpy(), hits.scores().astype(np.int64)
        if kind == "ref":
            counted = hits.shadowed(vmap, exclude=sc.loci) == 0
            var = np.zeros(len(rec), dtype=bool)
        else:
            lab = hits.variants(vmap, exclude=sc.loci)
            counted = (lab["flags"] & (va.VARIANT_DUP | va.VARIANT_ON_TARGET)) == 0
            var = counted & ((lab["flags"] & va.VARIANT_VAR) != 0)
        hits.close()
        for rows, keep in ((got[kind + "_table"], counted),) + (((got["var_table"], var),) if kind == "win" else ()):
            for g in range(pv.N_GUIDES):
                mine = keep & (rec["guide"] == g)
                assert int(rows["score_sum"][g]) == int(f[mine].sum()) and int(rows["positive"][g]) == int((f[mine] > 0).sum())
                nm = rec["info"][mine & (f > 0)] & 63
                assert rows["positive_nm"][g].astype(np.int64).tolist() == np.bincount(nm, minlength=9).tolist()
    assert got["win_table"]["score_sum"].sum() > 0 and got["var_table"]["score_sum"].sum() > 0 and got["ref_table"]["score_sum"].sum() > 0


def test_a_palindromic_pattern_reports_a_site_on_both_strands(ctx, tmp_path):
    """SW + N x 19 + WS is its own reverse complement: a window site that satisfies it is a record on '+' and on '-'; both are
    labelled alike, and neither is the other's duplicate (the strand is part of the key)."""
    rng = np.random.default_rng(31)
    pattern = pc.pattern_of(23, "both")
    assert pattern == pc.rc_iupac(pattern)
    guide = "NN" + pc.rnd(rng, 19) + "NN"
    site = pc.make_site(rng, pattern, guide)
    seq = pc.put(pc.rnd(rng, 3000), 1000, site)
    names = ["chrP palindrome"]
    # one homozygous SNP inside the site, at a protospacer position: its window holds the site with one mismatch
    vcf = vc.vcf_header(1) + "chrP\t%d\t.\t%s\t%s\t.\tPASS\t.\tGT\t1|1\n" % (1005 + 1, seq[1005], "A" if seq[1005] != "A" else "C")
    (tmp_path / "in.vcf").write_text(vcf)
    ref = va.PackedGenome.from_sequences([seq], names)
    win = va.variant_windows(ref, tmp_path / "in.vcf", seq_len=23, threads=1)
    vmap, gen = va.VariantMap(win, ref), ctx.load_genome(win)
    guides = [guide, "NN" + pc.rc(site)[2:21] + "NN"]
    hits = gen.search_pattern_hits(pattern, guides, 2)
    rec = hits.to_numpy()
    lab = hits.variants(vmap)
    both = [(int(r["contig"]), int(r["pos"])) for r in rec]
    twice = [k for k in set(both) if both.count(k) >= 2]
    assert twice  # one start, two records
    for w, p in twice:
        mine = [i for i, k in enumerate(both) if k == (w, p)]
        assert {int(rec["info"][i]) >> 31 for i in mine} == {0, 1}
        assert len({(int(lab["contig"][i]), int(lab["pos"][i]), int(lab["n_var"][i])) for i in mine}) == 1
        want = vmap.locate(w, p, 23)
        assert (int(lab["pos"][mine[0]]), int(lab["n_var"][mine[0]])) == (int(want["pos"]), int(want["n_var"]))
        assert not (lab["flags"][mine] & va.VARIANT_DUP).any()
    assert any(int(lab["pos"][i]) == 1000 and int(lab["n_var"][i]) == 1 for i in range(len(rec)))
    hits.close()
    gen.close()
    vmap.close()


def test_anchor_the_plain_search_at_length_23(ctx, tmp_path):
    """N x 21 + GR is what the plain search accepts: every record of Genome.search is among the pattern records, and for those
    (contig, pos, n_var, VAR) equal Hits.variants' values.  DUP / ON_TARGET are not compared: the pattern result has the
    right-edge neighbours that the plain search drops."""
    sc = vc.scenario(vc.SEEDS[0])
    m = 4
    ref = va.PackedGenome.from_sequences(sc.seqs, sc.names)
    (tmp_path / "in.vcf").write_text(sc.vcf)
    win = va.variant_windows(ref, tmp_path / "in.vcf", sample=0, threads=2)
    vmap, gen = va.VariantMap(win, ref), ctx.load_genome(win)
    plain = gen.search(sc.guides, m)
    prec, plab = plain.to_numpy(), plain.variants(vmap)
    plain.close()
    hits = gen.search_pattern_hits("N" * 21 + "GR", [g[:20] + "NNN" for g in sc.guides], m)
    rec, lab = hits.to_numpy(), hits.variants(vmap)
    hits.close()
    at = {(int(r["guide"]), int(r["info"]) >> 31, int(r["contig"]), int(r["pos"])): i for i, r in enumerate(rec)}
    assert len(prec) > 100 and len(rec) >= len(prec)
    for j, r in enumerate(prec):
        key = (int(r["guide"]), int(r["info"]) >> 31, int(r["contig"]), int(r["pos"]))
        assert key in at, key
        i = at[key]
        assert (int(lab["contig"][i]), int(lab["pos"][i]), int(lab["n_var"][i]), int(lab["flags"][i]) & va.VARIANT_VAR) == \
               (int(plab["contig"][j]), int(plab["pos"][j]), int(plab["n_var"][j]), int(plab["flags"][j]) & va.VARIANT_VAR), key
    gen.close()
    vmap.close()


def test_wrapped_window_start(product):
    sc, vmap, _, win_gen, _ = product("sa", "vcf_wrapped")
    hits = win_gen.search_pattern_hits(sc.pattern, sc.guides, pv.M)
    lab, rec = hits.variants(vmap, exclude=sc.loci), hits.to_numpy()
    for i in range(len(rec)):  # the host's answer per record
        want = vmap.locate(int(rec["contig"][i]), int(rec["pos"][i]), sc.L)
        assert (int(lab["contig"][i]), int(lab["pos"][i]), int(lab["n_var"][i])) == (int(want["contig"]), int(want["pos"]), int(want["n_var"]))
    hits.close()


def test_refused_arguments_and_released_scratch(ctx, product):
    sc, vmap, ref_gen, win_gen, table = product("sa")
    _, other_map, other_ref, other_win, other_table = product("sp")
    case = sc.case()
    win_hits = win_gen.search_pattern_hits(sc.pattern, sc.guides, pv.M)
    ref_hits = ref_gen.search_pattern_hits(sc.pattern, sc.guides, pv.M)
    screen = lambda **k: va.pattern_variants_screen(k.pop("ref", ref_gen), k.pop("win", win_gen), k.pop("vmap", vmap), sc.pattern, sc.guides,
                                                    k.pop("m", pv.M), **k)
    for call in (lambda: win_hits.variants(other_map),                                      # a map of another window genome
                 lambda: screen(vmap=other_map),
                 lambda: ref_hits.variants(vmap),                                           # ... the reference is no window genome
                 lambda: win_hits.variants(vmap, exclude=[(3, 0, 0)] * pv.N_GUIDES),        # a contig the reference does not have
                 lambda: ref_hits.shadowed(vmap, exclude=[(3, 0, 0)] * pv.N_GUIDES),
                 lambda: screen(exclude=[(0, 0, 2)] * pv.N_GUIDES),                         # a strand > 1
                 lambda: win_hits.shadowed(vmap),                                           # the windows are not the map's reference
                 lambda: screen(table=other_table),                                         # a table of another length
                 lambda: screen(m=9)):
        with pytest.raises(va.VarscotError) as e:
            call()
        assert e.value.code == -22 and str(e.value)
    # a record's guide beyond n_guides when exclude is given; table rows without a table; null arguments
    L = va.lib()
    from varscot_amd import _lib
    lab = np.zeros(len(win_hits), dtype=_lib.VARIANT_LABEL_DTYPE)
    ex = np.zeros(pv.N_GUIDES, dtype=_lib.LOCUS_DTYPE)
    assert L.vsc_pattern_hits_variants(win_hits._h, win_gen._h, vmap._h, _lib.ptr(ex), 3, _lib.ptr(lab)) == -22
    assert L.vsc_pattern_hits_variants(win_hits._h, win_gen._h, vmap._h, None, 3, _lib.ptr(lab)) == 0  # (no guide indexes anything)
    assert L.vsc_pattern_hits_variants(win_hits._h, win_gen._h, None, None, 0, _lib.ptr(lab)) == -22
    assert L.vsc_pattern_hits_variants(win_hits._h, win_gen._h, vmap._h, None, 0, None) == -22
    assert L.vsc_pattern_hits_variants(None, win_gen._h, vmap._h, None, 0, _lib.ptr(lab)) == -22
    assert L.vsc_pattern_hits_shadowed(ref_hits._h, None, vmap._h, None, 0, _lib.ptr(lab)) == -22
    # records outside the map and its windows: a result of another window genome (more windows than this map has)
    other_sc = pv.scenario("sp")
    other_hits = other_win.search_pattern_hits(other_sc.pattern, other_sc.guides, pv.M)
    assert other_hits.to_numpy()["contig"].max() >= len(sc.windows(0)) > 0
    lab2 = np.zeros(len(other_hits), dtype=_lib.VARIANT_LABEL_DTYPE)
    assert L.vsc_pattern_hits_variants(other_hits._h, win_gen._h, vmap._h, None, 0, _lib.ptr(lab2)) == -22
    assert b"outside" in L.vsc_last_error(ctx._h)
    other_hits.close()
    rows = [np.zeros(pv.N_GUIDES, dtype=va.PATTERN_VARIANT_ROW_DTYPE) for _ in range(3)]
    trow = np.zeros(pv.N_GUIDES, dtype=va.TABLE_ROW_DTYPE)
    pp = _lib.PatternParams(pv.M, 0, 0)
    args = lambda *tail: (ctx._h, ref_gen._h, win_gen._h, vmap._h, sc.pattern.encode(), "".join(sc.guides).encode(), pv.N_GUIDES, sc.L,
                          C.byref(pp)) + tail
    assert L.vsc_search_pattern_variants(*args(None, None, 0, _lib.ptr(rows[0]), _lib.ptr(rows[1]), None, _lib.ptr(trow), None, None)) == -22
    assert L.vsc_search_pattern_variants(*args(None, None, 0, None, _lib.ptr(rows[1]), None, None, None, None)) == -22
    assert L.vsc_search_pattern_variants(*args(None, None, 0, _lib.ptr(rows[0]), _lib.ptr(rows[1]), None, None, None, None)) == 0
    win_hits.close()
    ref_hits.close()
    before = screen(table=table, exclude=sc.loci)
    ctx.release_scratch()  # the map's device copy and the shadow arrays go with the scratch and come back
    after = screen(table=table, exclude=sc.loci)
    assert screen_bytes(before) == screen_bytes(after)
    check_rows(after, case.rows(True), True)


def test_no_guides_an_empty_window_genome_and_unchanged_inputs(ctx, product, tmp_path):
    sc, vmap, ref_gen, win_gen, table = product("trunc")
    got = va.pattern_variants_screen(ref_gen, win_gen, vmap, sc.pattern, [], pv.M, table=table, exclude=[])
    assert all(len(got[k]) == 0 for k in got)
    # a VCF without alt alleles: no windows - the reference's rows alone, nothing shadowed
    assert sc.windows(0, "vcf_no_alt") == []
    (tmp_path / "none.vcf").write_text(sc.vcf_no_alt)
    ref = va.PackedGenome.from_sequences(sc.seqs, sc.names)
    win = va.variant_windows(ref, tmp_path / "none.vcf", seq_len=sc.L, threads=1)
    assert len(win.names) == 0  # (no genome can be loaded from it: the screen takes None)
    empty_map, empty_gen = va.VariantMap(win, ref), None
    guides, loci = list(sc.guides), list(sc.loci)
    got = va.pattern_variants_screen(ref_gen, empty_gen, empty_map, sc.pattern, guides, pv.M, table=table, exclude=loci)
    assert guides == sc.guides and loci == sc.loci
    case = sc.case()
    want = pv.empty_rows(pv.N_GUIDES)
    for i, (g, _, _, _, nm, _) in enumerate(case.ref_hits):
        if case.ref_on[i]:
            want["on_target"][g] = 1
        else:
            pv.add_row(want, g, nm, case.ref_f[i])
    zero = pv.empty_rows(pv.N_GUIDES)
    check_rows(got, {"ref": want, "win": zero, "var": zero}, True)
    with pytest.raises(va.VarscotError) as e:  # ... but only with a map without windows
        va.pattern_variants_screen(ref_gen, None, vmap, sc.pattern, guides, pv.M)
    assert e.value.code == -22
    empty_map.close()


def test_pattern_search_tool_with_a_vcf(tmp_path, product):
    """pattern_search -v: the new -O columns against the restatement, the columns before them the run's without -v, the refused
    combinations."""
    import math
    import os
    import subprocess
    bin_dir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "varscot_amd", "bin")
    sc = pv.scenario("sa")
    case, m = sc.case(), pv.M
    with open(tmp_path / "g.fa", "w") as f:
        for name, seq in sc.records:
            f.write(">%s\n" % name + "".join(seq[i:i + 60] + "\n" for i in range(0, len(seq), 60)))
    (tmp_path / "guides.fa").write_text("".join(">g%d\n%s\n" % (i, g) for i, g in enumerate(sc.guides)))
    (tmp_path / "in.vcf").write_text(sc.vcf)
    (tmp_path / "none.vcf").write_text(sc.vcf_no_alt)
    table = ptc.make_table(va, sc.table)
    table.to_tsv(str(tmp_path / "table.tsv"))
    table.close()
    run = lambda *a: subprocess.run([os.path.join(bin_dir, a[0])] + list(a[1:]), capture_output=True, text=True, timeout=600)
    assert run("bidir_index", "-G", str(tmp_path / "g.fa"), "-I", str(tmp_path / "idx")).returncode == 0
    base = ["pattern_search", "-i", str(tmp_path / "idx"), "-q", sc.pattern, "-R", str(tmp_path / "guides.fa"), "-M", str(m)]
    read = lambda name: [l.rstrip("\n").split("\t") for l in open(tmp_path / name)]
    want, ind = case.rows(False), case.individual(False)  # -R: nothing is excluded
    for tabled in (False, True):
        extra = ["-W", str(tmp_path / "table.tsv")] if tabled else []
        assert run(*base, *extra, "-O", str(tmp_path / "plain.tsv")).returncode == 0
        r = run(*base, *extra, "-O", str(tmp_path / "ind.tsv"), "-v", str(tmp_path / "in.vcf"), "-n", "0")
        assert r.returncode == 0, r.stderr
        old, new = read("plain.tsv"), read("ind.tsv")
        n_old = len(old[0])
        assert [l[:n_old] for l in new] == old  # the columns before the new ones are the run without -v
        assert old[0][:3 + m + 1] == ["#guideId", "guideSeq", "offtargetCount"] + ["mm%d" % k for k in range(m + 1)]
        assert new[0][n_old:] == (["indCount"] + ["imm%d" % k for k in range(m + 1)] + ["varCount"] + ["vmm%d" % k for k in range(m + 1)] +
                                  ["varDuplicates", "refShadowed"] + (["indScoreSum", "indSpec", "varScoreSum"] if tabled else []))
        for g, line in enumerate(new[1:]):
            f = line[n_old:]
            assert line[0] == "g%d" % g
            assert [int(x) for x in line[3:4 + m]] == np.bincount([h[4] for h in case.ref_hits if h[0] == g], minlength=9)[:m + 1].tolist()
            assert int(f[0]) == int(ind["count"][g].sum()) and [int(x) for x in f[1:2 + m]] == ind["count"][g][:m + 1].tolist()
            assert int(f[2 + m]) == int(want["var"]["count"][g].sum()) and [int(x) for x in f[3 + m:4 + 2 * m]] == want["var"]["count"][g][:m + 1].tolist()
            assert int(f[4 + 2 * m]) == want["win"]["dropped"][g] and int(f[5 + 2 * m]) == want["ref"]["dropped"][g]
            if tabled:
                assert f[6 + 2 * m] == "%.6f" % (int(ind["score_sum"][g]) / ptc.ONE)
                assert f[7 + 2 * m] == "%.0f" % math.floor(va.table_specificity(int(ind["score_sum"][g])) + 0.5)
                assert f[8 + 2 * m] == "%.6f" % (int(want["var"]["score_sum"][g]) / ptc.ONE)
        assert len(new) == 1 + pv.N_GUIDES
    # -E: the enumerated loci are the excluded on-targets - the columns against the screen called with the listed guides and loci
    _, vmap, ref_gen, win_gen, _ = product("sa")
    (tmp_path / "t.bed").write_text("chr1\t0\t2500\nchr2\t300\t1500\n")
    r = run("pattern_search", "-i", str(tmp_path / "idx"), "-q", sc.pattern, "-E", str(tmp_path / "found.tsv"), "-p", "0,21", "-B", str(tmp_path / "t.bed"),
            "-M", "2", "-O", str(tmp_path / "enum.tsv"), "-v", str(tmp_path / "in.vcf"))
    assert r.returncode == 0, r.stderr
    lines = read("enum.tsv")
    ids, found = [l[0].split(":") for l in lines[1:]], [l[1] for l in lines[1:]]
    loci = [(sc.chroms.index(c), int(p), "+-".index(s)) for c, p, s in ids]
    assert len(found) > 20
    got = va.pattern_variants_screen(ref_gen, win_gen, vmap, sc.pattern, found, 2, exclude=loci)
    assert got["ref"]["on_target"].all()  # every guide was taken from the reference
    both = va.individual_pattern_rows(got["ref"], got["win"])
    for g, line in enumerate(lines[1:]):
        f = line[6:]  # behind guideId guideSeq offtargetCount mm0 mm1 mm2
        assert int(f[0]) == int(both["count"][g].sum()) and [int(x) for x in f[1:4]] == both["count"][g][:3].tolist()
        assert int(f[4]) == int(got["var"]["count"][g].sum()) and [int(x) for x in f[5:8]] == got["var"]["count"][g][:3].tolist()
        assert int(f[8]) == int(got["win"]["dropped"][g]) and int(f[9]) == int(got["ref"]["dropped"][g])
    # a sample without variants: the reference's numbers, zero variant columns
    r0 = run(*base, "-O", str(tmp_path / "none.tsv"), "-v", str(tmp_path / "none.vcf"))
    assert r0.returncode == 0, r0.stderr
    for line in read("none.tsv")[1:]:
        assert line[2:4 + m] == line[4 + m:6 + 2 * m] and all(x == "0" for x in line[6 + 2 * m:])  # ind = the reference's, no variants
    # what -v does not combine with, and -n without -v
    for extra in (["-u", "1,1", "-p", "0,21"], ["-T", str(tmp_path / "h.tsv")], ["-W", str(tmp_path / "table.tsv"), "-K", "3"],
                  ["-W", str(tmp_path / "table.tsv"), "-S", "0.5"], ["-u", "1,1", "-p", "0,21", "-U", str(tmp_path / "u.tsv")],
                  ["-u", "1,1", "-p", "0,21", "-Z", str(tmp_path / "z.tsv")]):
        bad = run(*base, "-O", str(tmp_path / "bad.tsv"), "-v", str(tmp_path / "in.vcf"), *extra)
        assert bad.returncode == 1 and "-v" in bad.stderr, extra
    assert run(*base, "-O", str(tmp_path / "bad.tsv"), "-n", "1").returncode == 1
    assert run(*base, "-O", str(tmp_path / "bad.tsv"), "-v", str(tmp_path / "in.txt")).returncode == 1
    assert run(*base, "-v", str(tmp_path / "in.vcf")).returncode == 1  # no -O
