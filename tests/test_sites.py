"""Cut sites on the device: the records and rows of search_sites / vsc_hits_sites / vsc_pattern_hits_sites byte for byte what
the definition gives when it is restated in plain Python (tests/sites_cases.py) - over the edge and homopolymer scenarios,
the budgets and classes, list lengths around one tile, the two outputs, the rounds, repetition, shards merged on the host, the
host function on the device's own inputs, the pattern form for Cas12a, SaCas9 and SpCas9 as a pattern, the two tools' -Z
outputs and the timing fields."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import varscot_amd as va
from varscot_amd import _lib
import bulges_cases as bc
import pattern_bulge_cases as pbc
import pattern_cases as pc
import sites_cases as sc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "varscot_amd", "bin")


@pytest.fixture(scope="module")
def ctx():
    c = va.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def edge(oracle):
    e = sc.edge_scenario(oracle)
    e["packed"] = va.PackedGenome.from_sequences(e["contigs"])
    e["want"] = sc.arrays(e["sites"], e["plain"], e["bulged"], len(e["guides"]))
    return e


@pytest.fixture(scope="module")
def edge_gen(ctx, edge):
    g = ctx.load_genome(edge["packed"])
    yield g
    g.close()


@pytest.fixture(scope="module")
def homo(oracle):
    e = sc.homopolymer_scenario(oracle)
    e["want"] = sc.arrays(e["sites"], e["plain"], e["bulged"], 1)
    return e


@pytest.fixture(scope="module")
def homo_gen(ctx, homo):
    g = ctx.load_genome(va.PackedGenome.from_sequences(homo["contigs"]))
    yield g
    g.close()


def same(got, want):
    assert got[0].dtype == va.SITE_DTYPE and got[1].dtype == va.SITE_ROW_DTYPE
    assert len(got[0]) == len(want[0])
    assert got[0].tobytes() == want[0].tobytes()
    assert got[1].tobytes() == want[1].tobytes()


class Bulged:
    """The device result of vsc_search_bulges / vsc_search_pattern_bulges, kept as a handle."""

    def __init__(self, gen, guides, m, dna, rna, pattern=None, proto=None):
        L, self.gen, self._h = va.lib(), gen, C.c_void_p()
        if pattern is None:
            codes = va.pack_guides(guides)
            p, bp = gen._params(m, None, "scan"), va.BulgeParams(dna, rna, 0, 0, 0)
            va.api.check(L.vsc_search_bulges(gen.ctx._h, gen._h, codes.ctypes.data, len(codes), C.byref(p), C.byref(bp), C.byref(self._h), None), gen.ctx._h)
        else:
            pp = _lib.PatternBulgeParams(m, 0, 0, proto[0], proto[1], dna, rna)
            va.api.check(L.vsc_search_pattern_bulges(gen.ctx._h, gen._h, pattern.encode(), "".join(guides).encode(), len(guides), len(pattern),
                                                     C.byref(pp), C.byref(self._h), None), gen.ctx._h)

    def __len__(self):
        return int(va.lib().vsc_bulge_hits_count(self._h))

    def to_numpy(self):
        data = C.c_void_p()
        va.api.check(va.lib().vsc_bulge_hits_data(self._h, C.byref(data)), self.gen.ctx._h)
        n = len(self)
        if n == 0:
            return np.zeros(0, dtype=va.BULGE_HIT_DTYPE)
        return np.frombuffer((C.c_char * (n * 16)).from_address(data.value), dtype=va.BULGE_HIT_DTYPE).copy()

    def close(self):
        va.lib().vsc_bulge_hits_free(self._h)
        self._h = None


def device_sites(gen, plain, bulged, n_guides, length=23, anchor="end", records=True, rows=True):
    """vsc_hits_sites over a Hits (or None) and a Bulged (or None)."""
    p = _lib.SiteParams(length, {"end": 0, "start": 1}[anchor])
    return gen._collapse(va.lib().vsc_hits_sites, plain._h if plain is not None else None, bulged._h if bulged is not None else None, n_guides,
                         p, records, rows)


def own_inputs(plain, bulged, n_guides, length=23, anchor="end"):
    """The restatement and the host function over the device's own input records."""
    pr = plain.to_numpy() if plain is not None else np.zeros(0, dtype=va.HIT_DTYPE)
    br = bulged.to_numpy() if bulged is not None else np.zeros(0, dtype=va.BULGE_HIT_DTYPE)
    want = sc.expected(sc.plain_of_hits(pr), sc.bulged_of_records(br), n_guides, length, anchor)
    host = va.collapse_sites(pr, br, n_guides, length, anchor)
    assert host[0].tobytes() == want[0].tobytes() and host[1].tobytes() == want[1].tobytes()
    return want


# ---- 1. the scenarios -----------------------------------------------------------------------------------------------------
def test_edge_scenario_equals_the_restatement(edge, edge_gen):
    got = edge_gen.search_sites(edge["guides"], bc.EDGE_M, dna=2, rna=2)
    same(got, edge["want"])
    assert len(got[0]) == 140 and int(got[1]["alignments"].sum()) == 305


def test_homopolymer_scenario_equals_the_restatement(homo, homo_gen):
    same(homo_gen.search_sites(homo["guides"], 4, dna=2, rna=2), homo["want"])


@pytest.mark.parametrize("m", [0, 4])
@pytest.mark.parametrize("dna,rna", [(1, 0), (0, 2), (2, 2)])
@pytest.mark.parametrize("which", ["edge", "homo"])
def test_budgets_and_classes(oracle, edge, edge_gen, homo, homo_gen, which, m, dna, rna):
    e, gen = (edge, edge_gen) if which == "edge" else (homo, homo_gen)
    n = len(e["guides"])
    plain = sc.plain_of_hits(oracle.search(e["contigs"], [bc.read_of(g) for g in e["guides"]], m, mode=oracle.MODE_PREDICATE))
    bulged = [x for x in e["bulged"] if x[5] <= m and x[4] in bc.enabled(dna, rna)]
    assert bulged
    same(gen.search_sites(e["guides"], m, dna=dna, rna=rna), sc.expected(plain, bulged, n))


# ---- 2. list lengths around one tile --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_bulged", [0, 1, 63, 64, 65])
def test_bulged_list_lengths_around_a_tile(ctx, n_bulged):
    """A contig of G only has one DNA-1 site per start: 23 + n bases give n bulged records (and their plain neighbours)."""
    gen = ctx.load_genome(va.PackedGenome.from_sequences(["G" * (23 + n_bulged)]))
    guides = ["G" * 23]
    plain, bulged = gen.search(guides, 2, algorithm="scan"), Bulged(gen, guides, 2, 1, 0)
    try:
        assert len(bulged) == n_bulged and len(plain) >= 1
        want = own_inputs(plain, bulged, 1)
        same(device_sites(gen, plain, bulged, 1), want)
        same(device_sites(gen, None, bulged, 1), own_inputs(None, bulged, 1))
    finally:
        bulged.close()
        plain.close()
        gen.close()


@pytest.mark.parametrize("n_plain", [0, 1, 63, 64, 65])
def test_plain_list_lengths_around_a_tile(homo, homo_gen, n_plain):
    """The homopolymer's plain hits cut to the best n by search_select (a result in search order); 0: a guide without hits."""
    guides = homo["guides"] if n_plain else ["ACGTACGTACGTACGTACGTAGG"]
    m = 4 if n_plain else 0
    plain = homo_gen.search_select(guides, m, top_k=n_plain)
    bulged = Bulged(homo_gen, homo["guides"], 4, 2, 2)
    try:
        assert len(plain) == n_plain and len(bulged) == len(homo["bulged"])
        same(device_sites(homo_gen, plain, bulged, 1), own_inputs(plain, bulged, 1))
        same(device_sites(homo_gen, plain, None, 1), own_inputs(plain, None, 1))
    finally:
        bulged.close()
        plain.close()


# ---- 3. the two outputs, the rounds, repetition ---------------------------------------------------------------------------
def test_rows_and_records_alone(edge, edge_gen):
    rec, rows = edge_gen.search_sites(edge["guides"], bc.EDGE_M, dna=2, rna=2, records=False)
    assert rec is None and rows.tobytes() == edge["want"][1].tobytes()
    rec, rows = edge_gen.search_sites(edge["guides"], bc.EDGE_M, dna=2, rna=2, rows=False)
    assert rows is None and rec.tobytes() == edge["want"][0].tobytes()
    with pytest.raises(va.VarscotError) as err:
        edge_gen.search_sites(edge["guides"], bc.EDGE_M, records=False, rows=False)
    assert err.value.code == -22 and "vsc_hits_sites" in str(err.value)


@pytest.mark.parametrize("batch", [1, 2, 0])
def test_guide_batch_never_changes_the_bytes(edge, edge_gen, batch):
    same(edge_gen.search_sites(edge["guides"], bc.EDGE_M, dna=2, rna=2, guide_batch=batch), edge["want"])


def test_second_call_and_the_timing_fields(ctx, homo, homo_gen):
    plain, bulged = homo_gen.search(homo["guides"], 4), Bulged(homo_gen, homo["guides"], 4, 2, 2)
    try:
        before = ctx.timing()
        a = device_sites(homo_gen, plain, bulged, 1)
        b = device_sites(homo_gen, plain, bulged, 1)
        assert ctx.timing() == before  # the collapse leaves vsc_ctx_timing alone
        same(a, homo["want"])
        same(b, homo["want"])
        assert plain.to_numpy().tobytes() == homo["plain_rec"].tobytes() and bulged.to_numpy().tobytes() == homo["bulged_rec"].tobytes()
        flag, write = C.c_double(-1), C.c_double(-1)
        assert va.lib().vsc_debug_sites_ms(ctx._h, C.byref(flag), C.byref(write)) == 0 and flag.value > 0 and write.value > 0
        ctx.release_scratch()
        same(device_sites(homo_gen, plain, bulged, 1), homo["want"])
    finally:
        bulged.close()
        plain.close()


def test_refusals_on_the_device(ctx, edge, edge_gen):
    n = len(edge["guides"])
    plain, bulged = edge_gen.search(edge["guides"], bc.EDGE_M), Bulged(edge_gen, edge["guides"], bc.EDGE_M, 2, 2)
    other = va.Context(0)
    try:
        L, h = va.lib(), C.c_void_p()
        rows = np.zeros(n, dtype=va.SITE_ROW_DTYPE)
        ok = _lib.SiteParams(23, 0)
        assert L.vsc_hits_sites(ctx._h, None, None, n, C.byref(ok), C.byref(h), rows.ctypes.data) == -22
        assert L.vsc_hits_sites(ctx._h, plain._h, bulged._h, n, C.byref(ok), None, None) == -22
        assert L.vsc_hits_sites(ctx._h, plain._h, bulged._h, n, None, C.byref(h), rows.ctypes.data) == -22
        for bad in (_lib.SiteParams(15, 0), _lib.SiteParams(33, 0), _lib.SiteParams(23, 2), _lib.SiteParams(23, 0, (0, 1))):
            assert L.vsc_hits_sites(ctx._h, plain._h, bulged._h, n, C.byref(bad), C.byref(h), rows.ctypes.data) == -22
        # a record whose guide is not below n_guides: found on the device, nothing returned
        top = int(bulged.to_numpy()["guide"].max())
        assert L.vsc_hits_sites(ctx._h, None, bulged._h, top, C.byref(ok), C.byref(h), rows.ctypes.data) == -22 and h.value is None
        assert "n_guides" in L.vsc_last_error(ctx._h).decode()
        assert L.vsc_hits_sites(other._h, plain._h, bulged._h, n, C.byref(ok), C.byref(h), rows.ctypes.data) == -22  # another context's results
        same(device_sites(edge_gen, plain, bulged, n), edge["want"])
    finally:
        other.close()
        bulged.close()
        plain.close()


# ---- 4. shards ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
def test_shards_merge_on_the_host(ctx, edge, world):
    """The members of a site can start in different shards: the shards' records, merged by their order, go through
    collapse_sites (a merged array is no device handle: vsc_hits_sites takes results only)."""
    plain, bulged = [], []
    for rank in range(world):
        g = ctx.load_genome(edge["packed"], rank, world)
        h = g.search(edge["guides"], bc.EDGE_M, algorithm="scan")
        plain.append(h.to_numpy())
        h.close()
        bulged.append(g.search_bulges(edge["guides"], bc.EDGE_M, dna=2, rna=2, rows=False)[0])
        g.close()
    assert sum(len(r) > 0 for r in bulged) >= 2
    plain, bulged = np.concatenate(plain), np.concatenate(bulged)
    plain, bulged = plain[np.lexsort((plain["pos"], plain["contig"], plain["info"] >> 31, plain["guide"]))], bulged[bc.merge_order(bulged)]
    with pytest.raises((C.ArgumentError, TypeError)):
        va.lib().vsc_hits_sites(ctx._h, None, bulged, len(edge["guides"]), C.byref(_lib.SiteParams(23, 0)), None, None)
    same(va.collapse_sites(plain, bulged, len(edge["guides"])), edge["want"])


# ---- 5. the pattern form --------------------------------------------------------------------------------------------------
def test_cas12a_with_the_start_anchor(ctx):
    e = sc.cas12a_scenario()
    n = len(e["guides"])
    gen = ctx.load_genome(va.PackedGenome.from_sequences(e["contigs"]))
    try:
        want = sc.arrays(e["sites"], e["plain"], e["bulged"], n)
        same(gen.search_pattern_sites(e["pattern"], e["guides"], e["m"], e["proto"], dna=2, rna=2), want)  # anchor=None: "start"
        same(gen.search_pattern_sites(e["pattern"], e["guides"], e["m"], e["proto"], dna=2, rna=2, anchor="end"),
             sc.expected(e["plain"], e["bulged"], n, e["length"], "end"))
        rec, rows = gen.search_pattern_sites(e["pattern"], e["guides"], e["m"], e["proto"], dna=2, rna=2, records=False)
        assert rec is None and rows.tobytes() == want[1].tobytes()
    finally:
        gen.close()


def test_sacas9_with_the_end_anchor(ctx):
    b = pbc.edge_scenario("SaCas9")
    n, L = len(b["guides"]), len(b["pattern"])
    plain = sc.plain_of_pattern(pc.arrays(pc.brute_force(b["contigs"], b["pattern"], b["guides"], b["m"])[0], n)[0])
    bulged = sc.bulged_of_hits(b["hits"])
    gen = ctx.load_genome(va.PackedGenome.from_sequences(b["contigs"]))
    try:
        got = gen.search_pattern_sites(b["pattern"], b["guides"], b["m"], b["proto"], dna=2, rna=2)
        same(got, sc.expected(plain, bulged, n, L, "end"))
        assert len(got[0]) < len(plain) + len(bulged)
        with pytest.raises(ValueError):
            gen.search_pattern_sites(b["pattern"], b["guides"], b["m"], (1, 19))
    finally:
        gen.close()


def test_spcas9_as_a_pattern(edge, edge_gen):
    """N x 21 + GR with the protospacer (0, 20), over the pattern search's own records."""
    pattern, guides = "N" * 21 + "GR", [bc.read_of(g) for g in edge["guides"]]
    n = len(guides)
    plain = sc.plain_of_pattern(edge_gen.search_pattern(pattern, guides, bc.EDGE_M, rows=False)[0])
    bulged = sc.bulged_of_records(edge_gen.search_pattern_bulges(pattern, guides, bc.EDGE_M, (0, 20), dna=2, rna=2, rows=False)[0])
    assert plain and bulged == edge["bulged"]
    got = edge_gen.search_pattern_sites(pattern, guides, bc.EDGE_M, (0, 20), dna=2, rna=2)
    same(got, sc.expected(plain, bulged, n))
    assert len(got[0]) < len(plain) + len(bulged)


# ---- 6. the tools ---------------------------------------------------------------------------------------------------------
def run(*a):
    return subprocess.run([os.path.join(BIN, a[0])] + list(a[1:]), capture_output=True, text=True, timeout=600)


def listing(sites, ids, names, contigs, length):
    out = []
    for x, _, _, _, nm_by_d in sites:
        g, s, c, p, d, nm, index = x
        members = ",".join("%s%d:%d" % ("+" if k > 0 else "", k, nm_by_d[k]) for k in sorted(nm_by_d))
        out.append((ids[g], names[c], str(p), str(p + length + d), "+-"[s], "plain" if d == 0 else "DNA" if d > 0 else "RNA", str(abs(d)), str(index),
                    str(nm), members, bc.genome_of(contigs[c])[p:p + length + d]))
    return out


SITE_HEADER = ["#guideId", "chrom", "start", "end", "strand", "kind", "size", "index", "mismatches", "members", "sequence"]


def test_guide_summary_sites(tmp_path, edge):
    names = ["c%d" % i for i in range(len(edge["contigs"]))]
    with open(tmp_path / "g.fa", "w") as f:
        for n, s in zip(names, edge["contigs"]):
            f.write(">%s\n%s\n" % (n, s))
    with open(tmp_path / "reads.fa", "w") as f:
        for i, g in enumerate(edge["guides"]):
            f.write(">g%d\n%s\n" % (i, g))
    assert run("bidir_index", "-G", str(tmp_path / "g.fa"), "-I", str(tmp_path / "idx")).returncode == 0
    base = ["guide_summary", "-G", str(tmp_path / "g.fa"), "-I", str(tmp_path / "idx"), "-R", str(tmp_path / "reads.fa"), "-M", str(bc.EDGE_M),
            "-u", "2,2"]
    before = run(*base, "-O", str(tmp_path / "before.tsv"), "-U", str(tmp_path / "u0.tsv"))
    assert before.returncode == 0, before.stderr
    r = run(*base, "-O", str(tmp_path / "with.tsv"), "-U", str(tmp_path / "u1.tsv"), "-Z", str(tmp_path / "sites.tsv"))
    assert r.returncode == 0, r.stderr
    assert open(tmp_path / "u0.tsv").read() == open(tmp_path / "u1.tsv").read()  # the other outputs are what they were
    old = [l.rstrip("\n").split("\t") for l in open(tmp_path / "before.tsv")]
    new = [l.rstrip("\n").split("\t") for l in open(tmp_path / "with.tsv")]
    assert [row[:-2] for row in new] == old and new[0][-2:] == ["siteCount", "siteBulgeOnly"]
    rows = edge["want"][1]
    assert [[int(x) for x in row[-2:]] for row in new[1:]] == [[int(rows["sites"][g]), int(rows["bulge_only"][g])] for g in range(len(rows))]
    lines = [l.rstrip("\n").split("\t") for l in open(tmp_path / "sites.tsv")]
    assert lines[0] == SITE_HEADER
    assert [tuple(l) for l in lines[1:]] == listing(edge["sites"], ["g%d" % g for g in range(len(rows))], names, edge["contigs"], 23)
    r = run(*base, "-O", str(tmp_path / "only.tsv"), "-Z", str(tmp_path / "sites2.tsv"))  # without -U
    assert r.returncode == 0 and open(tmp_path / "sites2.tsv").read() == open(tmp_path / "sites.tsv").read()


def test_pattern_search_sites(tmp_path):
    e = sc.cas12a_scenario()
    names = ["c%d" % i for i in range(len(e["contigs"]))]
    with open(tmp_path / "g.fa", "w") as f:
        for n, s in zip(names, e["contigs"]):
            f.write(">%s\n%s\n" % (n, s))
    with open(tmp_path / "q.fa", "w") as f:
        for i, g in enumerate(e["guides"]):
            f.write(">q%d\n%s\n" % (i, g))
    assert run("bidir_index", "-G", str(tmp_path / "g.fa"), "-I", str(tmp_path / "idx")).returncode == 0
    base = ["pattern_search", "-i", str(tmp_path / "idx"), "-q", e["pattern"], "-R", str(tmp_path / "q.fa"), "-M", str(e["m"]), "-u", "2,2",
            "-p", "%d,%d" % e["proto"]]
    before = run(*base, "-O", str(tmp_path / "before.tsv"), "-T", str(tmp_path / "t0.tsv"), "-U", str(tmp_path / "u0.tsv"))
    assert before.returncode == 0, before.stderr
    r = run(*base, "-O", str(tmp_path / "with.tsv"), "-T", str(tmp_path / "t1.tsv"), "-U", str(tmp_path / "u1.tsv"), "-Z", str(tmp_path / "sites.tsv"))
    assert r.returncode == 0, r.stderr
    for a, b in (("t0.tsv", "t1.tsv"), ("u0.tsv", "u1.tsv")):
        assert open(tmp_path / a).read() == open(tmp_path / b).read()
    old = [l.rstrip("\n").split("\t") for l in open(tmp_path / "before.tsv")]
    new = [l.rstrip("\n").split("\t") for l in open(tmp_path / "with.tsv")]
    assert [row[:-2] for row in new] == old and new[0][-2:] == ["siteCount", "siteBulgeOnly"]
    n = len(e["guides"])
    rows = sc.arrays(e["sites"], e["plain"], e["bulged"], n)[1]
    assert [[int(x) for x in row[-2:]] for row in new[1:]] == [[int(rows["sites"][g]), int(rows["bulge_only"][g])] for g in range(n)]
    lines = [l.rstrip("\n").split("\t") for l in open(tmp_path / "sites.tsv")]
    assert lines[0] == SITE_HEADER
    assert [tuple(l) for l in lines[1:]] == listing(e["sites"], ["q%d" % g for g in range(n)], names, e["contigs"], e["length"])
    r = run(*base, "-Z", str(tmp_path / "sites2.tsv"))  # -Z as the only output
    assert r.returncode == 0 and open(tmp_path / "sites2.tsv").read() == open(tmp_path / "sites.tsv").read()
