"""Table scores of bulged alignments without a device: vsc_bulge_table_score bit for bit what the definition gives when it is
restated in plain Python (tests/bulge_table_cases.py) - every d, every split point, the SpCas9, SaCas9 and Cas12a shapes, IUPAC
guide letters at unpaired and at mismatched positions - the floors of the site digits scenario, the two anchors (all-ones weights against vsc_pattern_table_score, the
SpCas9 form against vsc_table_score), what vsc_bulge_table_build refuses, the text file, the layouts through a C compiler and
the wrappers' argument checks."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import varscot_amd as va
from varscot_amd import _lib
import bulge_table_cases as btc
import pattern_bulge_cases as pbc
import pattern_cases as pc
import pattern_table_cases as ptc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "varscot_hip.h")).read()
ERR_INVALID = -22
PATTERNS = {"SpCas9": "N" * 21 + "GG", "SaCas9": "N" * 21 + "NNGRRT", "Cas12a": "TTTV" + "N" * 23}


def test_new_symbols_are_declared_exported_and_bound():
    names = ["vsc_bulge_table_build", "vsc_bulge_table_free", "vsc_bulge_table_info", "vsc_bulge_table_score", "vsc_bulge_hits_table",
             "vsc_sites_table", "vsc_sites_scores", "vsc_sites_scores_dev"]
    bound = {n for n, _, _ in _lib.SYMBOLS}
    for n in names:
        assert n + "(" in HEADER and n in bound and hasattr(va.lib(), n), n
    assert "vsc_debug_site_table_ms" in {n for n, _, _ in _lib.DEBUG_SYMBOLS}
    assert va.lib().vsc_abi_version() == 5 and re.search(r"#define\s+VSC_ABI_VERSION\s+5\b", HEADER)
    assert "It is not a maximum over" in HEADER and "scores for bulged alignments" not in HEADER.split("vsc_sites_collapse / vsc_sites_collapse_pattern")[1].split("*/")[0].split("since added")[0]


def test_the_site_digits_scenario_holds_its_floors():
    """digits_sites(): the conditions of pattern_table_cases.digit_floors on `top`, by name, with cut() against a second
    restatement - np.lexsort on (-top, record index) per guide - over every case."""
    s = btc.digits_sites()
    guide_of, top = s["site_rec"]["guide"].astype(np.int64), s["scores"]["top"].astype(np.int64)
    n = len(s["guides"])

    def lexsort_cut(top_k, min_score):
        keep = []
        for g in range(n):
            idx = np.nonzero((guide_of == g) & (top >= min_score))[0]
            if top_k and len(idx) > top_k:
                idx = idx[np.lexsort((idx, -top[idx]))[:top_k]]
            keep.extend(int(i) for i in idx)
        return np.array(sorted(keep), dtype=np.int64)

    assert len(s["cases"]) == len(set(s["cases"])) == len(s["serves"]) <= ptc.MAX_CASES
    for top_k, min_score in s["cases"]:
        assert (btc.cut(guide_of, top, top_k, min_score) == lexsort_cut(top_k, min_score)).all(), (top_k, min_score)
    unmet = ptc.digit_floors(guide_of, top, n, s["cases"], lexsort_cut)
    assert not unmet, "digits_sites() does not reach: %s" % ", ".join(unmet)
    assert len(np.unique(top)) > 200 and (top == 0).any() and len({int(d) for d in s["scores"]["top_d"]}) >= 2
    assert s["table"]["dna"].shape == s["table"]["rna"].shape == (20, 4)
    for key in ("pair", "dna", "rna"):  # dyadic: 1 - w is a power of two (or w is 0 or 1)
        w = 1.0 - s["table"][key][(s["table"][key] > 0) & (s["table"][key] < 1)]
        assert (np.frexp(w)[0] == 0.5).all(), key


def guide_kinds(rng, pattern, proto):
    """A spelled guide with N at the pattern's letters, one with degenerate letters and an N inside the protospacer, one all ACGT."""
    a, n = proto
    g0 = pbc.distinct_guide(rng, pattern, proto)
    g1 = list(pbc.distinct_guide(rng, pattern, proto))
    for j, letter in ((a + 2, "R"), (a + 5, "Y"), (a + n - 3, "B"), (a + n // 2, "N")):
        g1[j] = next(x for x in (letter, "N") if g1[j] in pc.IUPAC[x])
    g2 = "".join(ch if ch != "N" else "ACGT"[int(rng.integers(4))] for ch in g0)
    return [g0, "".join(g1), g2]


# ------------------------------------------------------------------------------------ 1. the definition
@pytest.mark.parametrize("name", ["SpCas9", "SaCas9", "Cas12a"])
def test_score_equals_the_restatement(name):
    """Every d and every split point: a site planted at split point i with 0 .. 2 substitutions, scored at the split point the
    walk reports (the smallest that reaches NM); random sites as well, where the walk picks among many."""
    rng = np.random.default_rng(700 + len(name))
    shape, pattern = btc.SHAPES[name], PATTERNS[name]
    L, proto, _ = shape
    table = btc.random_bulge_table(rng, shape, zeros=12, ones=12)
    t = btc.make_table(va, table)
    seen, zero, unpaired_degenerate = set(), 0, 0
    try:
        for guide in guide_kinds(rng, pattern, proto):
            for d in (-2, -1, 1, 2):
                for i in pbc.indices(proto, d):
                    free = [j for j in range(proto[0], proto[0] + proto[1]) if (j < i - 2 or j > i + 3) and guide[j] != "N"]
                    for k in range(3):
                        s = pbc.plant(rng, pattern, guide, proto, d, i, rng.choice(free, size=k, replace=False))
                        nm, index, _ = pbc.best(guide, s, proto, d)
                        want = btc.py_bulge_score(table, guide, s, d, index)
                        got = t.score(guide, s, d, fixed=True)
                        assert got[:2] == (nm, index), (guide, s, d)
                        assert np.float64(got[2]).tobytes() == np.float64(want).tobytes() and got[3] == ptc.py_fixed(want), (guide, s, d, i)
                        seen.add((d, index))
                        zero += got[3] == 0
                        unpaired_degenerate += d < 0 and any(guide[index + q] not in "ACGT" for q in range(-d))
                for _ in range(40):
                    s = pc.rnd(rng, L + d)
                    nm, index, _ = pbc.best(guide, s, proto, d)
                    want = btc.py_bulge_score(table, guide, s, d, index)
                    got = t.score(guide, s.lower(), d, fixed=True)
                    assert got == (nm, index, want, ptc.py_fixed(want)), (guide, s, d)
            for _ in range(40):  # d = 0: the plain score
                can = [j for j in range(proto[0], proto[0] + proto[1]) if guide[j] != "N"]
                s = pc.make_site(rng, pattern, guide, set(int(j) for j in rng.choice(can, size=2, replace=False)))
                nm, _, f = btc.member(table, guide, s, 0)
                assert t.score(guide, s, 0, fixed=True) == (nm, 0, ptc.py_score(table, guide, s), f)
        for d in (-2, -1, 1, 2):
            assert {i for dd, i in seen if dd == d} >= {min(pbc.indices(proto, d)), max(pbc.indices(proto, d))}, d  # both ends of the range
        assert zero > 0 and unpaired_degenerate > 0  # a planted zero met; a degenerate letter at an unpaired position
    finally:
        t.close()


@pytest.mark.parametrize("name", ["SpCas9", "Cas12a"])
def test_all_ones_anchor_is_the_pattern_score_of_the_paired_site(name):
    rng = np.random.default_rng(31)
    shape, pattern = btc.SHAPES[name], PATTERNS[name]
    L, proto, _ = shape
    table = btc.all_ones(btc.random_bulge_table(rng, shape, zeros=6, ones=6))
    t, base = btc.make_table(va, table), ptc.make_table(va, table)
    try:
        guide = "".join(ch if ch != "N" else "ACGT"[int(rng.integers(4))] for ch in pbc.distinct_guide(rng, pattern, proto))
        for d in (-2, -1, 1, 2):
            for _ in range(100):
                s = pc.rnd(rng, L + d)
                nm, i, x, f = t.score(guide, s, d, fixed=True)
                if d > 0:
                    q, g = s[:i] + s[i + d:], guide
                else:  # the unpaired guide positions take no part: N there, any letter in q
                    q, g = s[:i] + "C" * -d + s[i:], guide[:i] + "N" * -d + guide[i - d:]
                assert (x, f) == base.score(g, q, fixed=True)
    finally:
        t.close()
        base.close()


def test_spcas9_form_against_the_score_table():
    rng = np.random.default_rng(32)
    table = btc.all_ones(btc.random_bulge_table(rng, btc.SHAPES["SpCas9"], zeros=4, ones=4))
    st = va.ScoreTable(table["pair"], table["pam"])
    t = va.BulgeTable(st, table["dna"], table["rna"])  # a ScoreTable as the base
    try:
        assert t.info()["protospacer"] == (0, 20) and t.info()["pam_positions"] == (21, 22) and t.info()["length"] == 23
        for _ in range(200):
            guide, s = pc.rnd(rng, 23), pc.rnd(rng, 23)
            assert t.score(guide, s, 0, fixed=True)[2:] == st.score(guide, s, fixed=True)
            s = pc.rnd(rng, 24)
            _, i, x, f = t.score(guide, s, 1, fixed=True)
            assert (x, f) == st.score(guide, s[:i] + s[i + 1:], fixed=True)
    finally:
        t.close()
        st.close()


# ------------------------------------------------------------------------------------ 2. what the build refuses
def test_build_refusals_and_the_copy():
    L, h = va.lib(), C.c_void_p()
    rng = np.random.default_rng(3)
    good = btc.random_bulge_table(rng, btc.SHAPES["SpCas9"], zeros=4, ones=4)
    base = ptc.make_table(va, good)

    def build(b, dna, rna):
        dna, rna = np.ascontiguousarray(dna, dtype=np.float64), np.ascontiguousarray(rna, dtype=np.float64)
        rc = L.vsc_bulge_table_build(b, _lib.ptr(dna), _lib.ptr(rna), C.byref(h))
        if rc == 0:
            L.vsc_bulge_table_free(h)
        return rc

    assert build(base._h, good["dna"], good["rna"]) == 0
    for key in ("dna", "rna"):
        for i, b, w in ((3, 1, float("nan")), (3, 1, -0.25), (19, 3, 1.0000001), (0, 0, float("inf")), (0, 2, -1e-300), (19, 0, 2.0)):
            bad = {k: good[k].copy() for k in ("dna", "rna")}
            bad[key][i, b] = w  # rows 0 and ps_len - 1 are never read and still validated
            assert build(base._h, bad["dna"], bad["rna"]) == ERR_INVALID and not h.value, (key, i, b, w)
            with pytest.raises(va.VarscotError):
                va.BulgeTable(base, bad["dna"], bad["rna"])
    assert build(None, good["dna"], good["rna"]) == ERR_INVALID  # a NULL base
    assert L.vsc_bulge_table_build(base._h, None, _lib.ptr(good["rna"]), C.byref(h)) == ERR_INVALID
    assert L.vsc_bulge_table_build(base._h, _lib.ptr(good["dna"]), None, C.byref(h)) == ERR_INVALID
    assert L.vsc_bulge_table_build(base._h, _lib.ptr(good["dna"]), _lib.ptr(good["rna"]), None) == ERR_INVALID
    short = va.PatternTable(23, (17, 3), np.ones((3, 4, 4)), (), (1.0,))  # ps_len < 4
    assert build(short._h, np.ones((3, 4)), np.ones((3, 4))) == ERR_INVALID
    four = va.PatternTable(16, (0, 4), np.ones((4, 4, 4)), (), (1.0,))   # ps_len == 4 is inside
    assert build(four._h, np.zeros((4, 4)), np.ones((4, 4))) == 0
    assert L.vsc_bulge_table_info(None, None) == ERR_INVALID and L.vsc_bulge_table_free(None) == 0
    with pytest.raises(ValueError):
        va.BulgeTable(base, good["dna"][:19], good["rna"])
    # the weights are copied: the table outlives its base; a second table has another serial number
    t = va.BulgeTable(base, good["dna"], good["rna"])
    u = va.BulgeTable(base, good["dna"], good["rna"])
    base.close()
    short.close()
    four.close()
    guide, s = "ACGTACGTTGCATGCAGTCANGG", "ACGTATCGTTGCATGCAGTCATGG"
    assert t.score(guide, s, 1, fixed=True)[3] == ptc.py_fixed(btc.py_bulge_score(good, guide, s, 1, pbc.best(guide, s, (0, 20), 1)[1]))
    assert t.info()["serial"] != u.info()["serial"] and t.info()["zero_weights"] == int((good["pair"] == 0).sum() + (good["pam"] == 0).sum()
                                                                                     + (good["dna"] == 0).sum() + (good["rna"] == 0).sum())
    t.close()
    u.close()


def test_score_argument_checks():
    L = va.lib()
    good = btc.random_bulge_table(np.random.default_rng(4), btc.SHAPES["SpCas9"])
    t = btc.make_table(va, good)
    try:
        g, s = b"A" * 23, b"A" * 25
        assert L.vsc_bulge_table_score(t._h, g, s, 2, None, None, None, None) == 0  # every output is optional
        assert L.vsc_bulge_table_score(None, g, s, 2, None, None, None, None) == ERR_INVALID
        assert L.vsc_bulge_table_score(t._h, None, s, 2, None, None, None, None) == ERR_INVALID
        assert L.vsc_bulge_table_score(t._h, g, None, 2, None, None, None, None) == ERR_INVALID
        for d in (3, -3, 100):
            assert L.vsc_bulge_table_score(t._h, g, s, d, None, None, None, None) == ERR_INVALID
        assert L.vsc_bulge_table_score(t._h, g, b"A" * 24 + b"N", 2, None, None, None, None) == ERR_INVALID  # a site letter that is no base
        assert L.vsc_bulge_table_score(t._h, b"A" * 22 + b"U", s, 2, None, None, None, None) == ERR_INVALID   # no IUPAC letter
        with pytest.raises(ValueError):
            t.score("A" * 23, "A" * 23, 1)
        with pytest.raises(ValueError):
            t.score("A" * 22, "A" * 23, 0)
    finally:
        t.close()
    # L + d must stay inside 16 .. 32
    edge = va.PatternTable(16, (0, 13), np.ones((13, 4, 4)), (), (1.0,))
    u = va.BulgeTable(edge, np.ones((13, 4)), np.ones((13, 4)))
    edge.close()
    assert L.vsc_bulge_table_score(u._h, b"A" * 16, b"A" * 15, -1, None, None, None, None) == ERR_INVALID
    assert L.vsc_bulge_table_score(u._h, b"A" * 16, b"A" * 17, 1, None, None, None, None) == 0
    u.close()


def test_device_entry_points_refuse_null_arguments():
    L = va.lib()
    assert L.vsc_bulge_hits_table(None, None, None, b"A" * 23, 1, 23, None, None, None) == ERR_INVALID
    assert L.vsc_sites_table(None, None, None, None, b"A" * 23, 1, 23, None, None, None, None) == ERR_INVALID
    assert L.vsc_sites_scores(None, None) == ERR_INVALID and L.vsc_sites_scores_dev(None) is None
    assert L.vsc_debug_site_table_ms(None, None, None, None) == ERR_INVALID


# ------------------------------------------------------------------------------------ 3. the header's structs
def test_header_structs(tmp_path):
    assert C.sizeof(_lib.BulgeTableStats) == 48 and va.SITE_SCORE_DTYPE.itemsize == 16 and va.SITE_SCORE_DTYPE.names == ("best", "top", "top_d", "reserved")
    body = ('#include "varscot_hip.h"\n%s(sizeof(vsc_bulge_table_stats) == 48 && sizeof(vsc_site_score) == 16, "bulge table");\n'
            '%s(sizeof(vsc_site) == 32 && sizeof(vsc_guide_table_row) == 96 && VSC_ABI_VERSION == 5, "unchanged");\n'
            'int (*score)(const vsc_bulge_table *, const char *, const char *, int, uint32_t *, uint32_t *, double *, uint32_t *) = vsc_bulge_table_score;\n'
            'int (*scores)(vsc_sites *, const vsc_site_score **) = vsc_sites_scores;\n'
            'int (*build)(const vsc_pattern_table *, const double *, const double *, vsc_bulge_table **) = vsc_bulge_table_build;\n'
            'int main(void) { vsc_site_score s = {1, 2, 3, 0}; return (int)(s.best + s.top + s.top_d + s.reserved) - 6\n'
            '                 + (int)VSC_SITE_MEMBER_NM(31u << 20, 2) - 31 + (int)VSC_BULGE_INDEX(VSC_BULGE_INFO(1, 1, 2, 17, 3)) - 17; }\n')
    for compiler, flag, name, word in ((shutil.which("cc") or shutil.which("gcc"), "-std=c11", "layout.c", "_Static_assert"),
                                       (shutil.which("c++") or shutil.which("g++"), "-std=c++17", "layout.cpp", "static_assert")):
        if compiler:  # the header's own asserts, to a C and to a C++ compiler
            src = tmp_path / name
            src.write_text(body % (word, word))
            r = subprocess.run([compiler, flag, "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
            assert r.returncode == 0, r.stderr


# ------------------------------------------------------------------------------------ 4. the text file
@pytest.mark.parametrize("name", ["SpCas9", "Cas12a"])
def test_tsv_round_trip_to_the_bit(tmp_path, name):
    table = btc.random_bulge_table(np.random.default_rng(9), btc.SHAPES[name], zeros=3, ones=3)
    a = btc.make_table(va, table)
    a.to_tsv(str(tmp_path / "one.tsv"))                                   # one file: the base's lines, then dna and rna
    a.to_tsv(str(tmp_path / "w.tsv"), base_path=str(tmp_path / "W.tsv"))  # two files: what the tools take as -w and -W
    for b in (va.BulgeTable.from_tsv(str(tmp_path / "one.tsv")), va.BulgeTable.from_tsv(str(tmp_path / "w.tsv"), base_path=str(tmp_path / "W.tsv"))):
        assert (b.length, b.protospacer, b.pam_positions) == (a.length, a.protospacer, a.pam_positions)
        assert b.pair.tobytes() == a.pair.tobytes() and b.pam.tobytes() == a.pam.tobytes()
        assert b.dna.tobytes() == table["dna"].tobytes() and b.rna.tobytes() == table["rna"].tobytes()
        assert b.info()["serial"] != a.info()["serial"]
        b.close()
    p = va.PatternTable.from_tsv(str(tmp_path / "W.tsv"))  # the base file is a pattern table's
    assert p.pair.tobytes() == a.pair.tobytes()
    assert not any(l.startswith(("dna", "rna")) for l in open(tmp_path / "W.tsv"))
    assert all(l.startswith(("dna", "rna", "#")) for l in open(tmp_path / "w.tsv"))
    p.close()
    a.close()


def test_tsv_errors(tmp_path):
    base = "shape 16 2 4\npam_pos\n" + "".join("pair %d %s %s 0.5\n" % (j, g, s) for j in range(2, 6) for g in "ACGT" for s in "ACGT" if g != s) + "pam - 0.25\n"
    extra = "".join("%s %d %s 0.5\n" % (k, j, b) for k in ("dna", "rna") for j in range(2, 6) for b in "ACGT")

    def load(body, base_body=None):
        (tmp_path / "t.tsv").write_text(body)
        if base_body is None:
            return va.BulgeTable.from_tsv(str(tmp_path / "t.tsv"))
        (tmp_path / "b.tsv").write_text(base_body)
        return va.BulgeTable.from_tsv(str(tmp_path / "t.tsv"), base_path=str(tmp_path / "b.tsv"))

    t = load("# a comment\n" + base + extra)
    assert t.dna[1, 2] == 0.5 and t.rna.shape == (4, 4)
    t = load(extra, base)
    assert t.protospacer == (2, 4)
    n = base.count("\n")
    for bad, where in (("dna 1 A 0.5\n", n + 1), ("dna 6 A 0.5\n", n + 1), ("rna 3 X 0.5\n", n + 1), ("rna 3 A abc\n", n + 1), ("dna 3 A\n", n + 1),
                       ("dna 3 A 0.5\ndna 3 A 0.5\n", n + 2)):
        with pytest.raises(ValueError, match="t.tsv:%d" % where):
            load(base + bad)
    with pytest.raises(ValueError, match="missing"):
        load(base + extra.replace("rna 4 G 0.5\n", ""))
    with pytest.raises(ValueError, match="t.tsv:1"):
        load("shape 16 2 4\n" + extra, base)                              # the base's lines where only dna and rna lines belong
    with pytest.raises(ValueError, match="no 'shape'"):
        load(extra)
    with pytest.raises(va.VarscotError):
        load(base + extra.replace("rna 4 G 0.5\n", "rna 4 G 1.5\n"))      # the library's own range check
    with pytest.raises(va.VarscotError):
        load(base.replace("shape 16 2 4", "shape 16 2 3").replace("".join("pair 5 %s %s 0.5\n" % (g, s) for g in "ACGT" for s in "ACGT" if g != s), "")
             + "".join("%s %d %s 0.5\n" % (k, j, b) for k in ("dna", "rna") for j in range(2, 5) for b in "ACGT"))  # ps_len < 4


# ------------------------------------------------------------------------------------ 5. the tools' arguments
def _run(tool, *args):
    return subprocess.run([os.path.join(ROOT, "varscot_amd", "bin", tool)] + list(args), capture_output=True, text=True, timeout=120,
                          env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))


def test_guide_summary_bulge_table_argument_errors(tmp_path):
    (tmp_path / "g.fa").write_text(">c\n" + "ACGT" * 30 + "\n")
    (tmp_path / "r.fa").write_text(">r\n" + "ACGT" * 5 + "AGG\n")
    (tmp_path / "W.tsv").write_text("")
    (tmp_path / "w.tsv").write_text("")
    W, w, Z = ["-W", str(tmp_path / "W.tsv")], ["-w", str(tmp_path / "w.tsv")], ["-Z", str(tmp_path / "s.tsv")]
    base = ["-G", str(tmp_path / "g.fa"), "-I", str(tmp_path / "idx"), "-O", str(tmp_path / "out.tsv"), "-M", "3", "-R", str(tmp_path / "r.fa")]
    for extra in (w, w + W, w + W + ["-u", "1,1"], w + ["-u", "1,1"] + Z, W + ["-u", "1,1"] + Z + ["-w", str(tmp_path / "w.bed")]):
        res = _run("guide_summary", *base, *extra)
        assert res.returncode == 1 and "-w scores the cut sites" in res.stderr and "give -W, -u and -Z" in res.stderr, (extra, res.stderr)
    # -K / -S without -T are for the -Z listing once -w is there; without -w they still ask for -T
    res = _run("guide_summary", *base, *W, "-u", "1,1", *Z, "-K", "3")
    assert res.returncode == 1 and "give -T" in res.stderr
    res = _run("guide_summary", *base, *W, *w, "-u", "1,1", *Z, "-K", "3", "-S", "0.5")   # well-formed: gets as far as the index
    assert res.returncode == 1 and "idx" in res.stderr and "give -T" not in res.stderr
    assert not (tmp_path / "out.tsv").exists() and not (tmp_path / "s.tsv").exists()
    res = _run("guide_summary", "--help")
    assert res.returncode == 0 and "-w, --bulge-table" in res.stdout


def test_pattern_search_bulge_table_argument_errors(tmp_path):
    (tmp_path / "q.fa").write_text(">q\n" + "ACGT" * 5 + "A" + "NNNNNN\n")
    sa = "N" * 21 + "NNGRRT"
    table = btc.random_bulge_table(np.random.default_rng(2), btc.SHAPES["SaCas9"])
    t = btc.make_table(va, table)
    t.to_tsv(str(tmp_path / "w.tsv"), base_path=str(tmp_path / "W.tsv"))
    t.close()
    other = btc.random_bulge_table(np.random.default_rng(2), (27, (0, 20), (23, 24, 25, 26)))
    t = btc.make_table(va, other)
    t.to_tsv(str(tmp_path / "w20.tsv"), base_path=str(tmp_path / "W20.tsv"))
    t.close()
    W, w, Z, u = ["-W", str(tmp_path / "W.tsv")], ["-w", str(tmp_path / "w.tsv")], ["-Z", str(tmp_path / "s.tsv")], ["-u", "1,1", "-p", "0,21"]
    base = ["-i", str(tmp_path / "idx"), "-q", sa, "-R", str(tmp_path / "q.fa"), "-M", "3", "-O", str(tmp_path / "o.tsv")]
    for extra in (w, w + W, w + W + u, w + u + Z, W + u + Z + ["-w", str(tmp_path / "w.bed")]):
        res = _run("pattern_search", *base, *extra)
        assert res.returncode == 1 and "-w scores the cut sites" in res.stderr and "give -W, -u, -p and -Z" in res.stderr, (extra, res.stderr)
    res = _run("pattern_search", *base, *W, *u, *Z, "-K", "3")                              # a cut without a listing it applies to
    assert res.returncode == 1 and "give -W and -T" in res.stderr
    res = _run("pattern_search", *base, "-W", str(tmp_path / "W20.tsv"), "-w", str(tmp_path / "w20.tsv"), *u, *Z)
    assert res.returncode == 1 and "is not the -p protospacer" in res.stderr
    (tmp_path / "short.tsv").write_text("".join(l for l in open(tmp_path / "w.tsv") if not l.startswith("rna\t7\t")))
    res = _run("pattern_search", *base, *W, "-w", str(tmp_path / "short.tsv"), *u, *Z)
    assert res.returncode == 1 and "lack an entry" in res.stderr
    (tmp_path / "bad.tsv").write_text(open(tmp_path / "w.tsv").read() + "dna 21 A 0.5\n")
    res = _run("pattern_search", *base, *W, "-w", str(tmp_path / "bad.tsv"), *u, *Z)
    assert res.returncode == 1 and "outside the protospacer" in res.stderr
    res = _run("pattern_search", *base, *W, *w, *u, *Z, "-K", "3", "-S", "0.5")             # well-formed: gets as far as the index
    assert res.returncode == 1 and "idx" in res.stderr and "-w" not in res.stderr
    assert not (tmp_path / "s.tsv").exists() and not (tmp_path / "o.tsv").exists()
    res = _run("pattern_search", "--help")
    assert res.returncode == 0 and "-w, --bulge-table" in res.stdout
