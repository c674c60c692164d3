"""The host half of the table-driven scores (vsc_score_table_build, vsc_table_score, vsc_table_specificity, ScoreTable's
loaders): CRISPOR's cfdOfftargetScore and cfdSpecScore columns for the seven SITE-Seq guides through the fitted fixture
table, the definition in plain Python bit for bit, the refusals, the header's structs.  No device needed."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import varscot_amd as va
from table_cases import CFD_SPEC, ONE, REL_TOL, TABLE_TSV, code, fixture_rows, fixture_table, py_fixed, py_score, random_table, table_rows
from varscot_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID = -22  # VSC_ERR_INVALID
HEADER = open(os.path.join(ROOT, "include", "varscot_hip.h")).read()


@pytest.fixture(scope="module")
def golden():
    rows = fixture_rows()
    table = fixture_table()
    L = va.lib()
    gcodes = va.pack_guides(rows["guides"])
    x, f = C.c_double(), C.c_uint32()
    score, fixed = np.zeros(len(rows["cfd"])), np.zeros(len(rows["cfd"]), dtype=np.int64)
    for i in range(len(score)):  # ALL rows, none left out
        assert L.vsc_table_score(table._h, int(gcodes[rows["guide"][i]]), int(rows["site_code"][i]), C.byref(x), C.byref(f)) == 0
        score[i], fixed[i] = x.value, f.value
    return rows, table, score, fixed


# ------------------------------------------------------------------------------------ 1. every fixture row
def test_every_crispor_row_is_reproduced(golden):
    rows, _, score, fixed = golden
    cfd = rows["cfd"]
    assert len(cfd) == 15002 and (cfd == 0).sum() == 6294 and (cfd > 0).sum() == 8708
    assert (score[cfd == 0] == 0.0).all() and (fixed[cfd == 0] == 0).all()
    rel = np.abs(score[cfd > 0] / cfd[cfd > 0] - 1.0)
    print("largest relative error %.3g over %d rows" % (rel.max(), len(rel)))
    assert rel.max() <= REL_TOL
    assert (fixed == np.rint(score * 2.0 ** 30)).all() and fixed.max() <= ONE
    # the file's mismatchCount is the Hamming distance over the 20 positions that take part
    ham = np.array([sum(a != b for a, b in zip(rows["guides"][g][:20], s[:20])) for g, s in zip(rows["guide"], rows["site"])])
    assert (ham == rows["mismatches"]).all()


# ------------------------------------------------------------------------------------ 2. per-guide specificity
def test_guide_specificities_equal_cfdSpecScore(golden):
    rows, _, _, fixed = golden
    assert rows["cfd_spec"] == CFD_SPEC
    sums = [int(fixed[rows["guide"] == g].sum()) for g in range(7)]
    spec = [va.table_specificity(s) for s in sums]
    print("specificities", ["%.4f" % s for s in spec])
    assert [int(math.floor(s + 0.5)) for s in spec] == CFD_SPEC
    # the function is the formula, evaluated in the stated order
    assert spec == [100.0 / (100.0 + s * 2.0 ** -30) * 100.0 for s in sums]
    assert va.table_specificity(0) == 100.0
    t = table_rows(rows["guide"], rows["mismatches"], fixed, 7)
    assert t["score_sum"].tolist() == sums and (t["positive"] == np.bincount(rows["guide"][fixed > 0], minlength=7)).all()


# ------------------------------------------------------------------------------------ 3. the definition, bit for bit
def _bits(x):
    return np.float64(x).view(np.uint64)


def test_definition_bit_for_bit_over_random_tables():
    rng = np.random.default_rng(2030)
    letters = "ACGT"
    for trial in range(6):
        pair, pam = random_table(rng, zeros=trial % 3, ones=2 * (trial % 2))
        t = va.ScoreTable(pair, pam)
        assert t.info()["zero_weights"] == trial % 3
        # every (j, g, s) entry once on its own, every PAM entry
        for j in range(20):
            for g in range(4):
                for s in range(4):
                    guide = "".join(letters[(g if k == j else 0)] for k in range(20)) + "AGG"
                    site = "".join(letters[(s if k == j else 0)] for k in range(20)) + "A" + letters[j % 4] + letters[(g + s) % 4]
                    x, f = t.score(guide, site, fixed=True)
                    want = py_score(pair, pam, guide, site)
                    assert _bits(x) == _bits(want) and f == py_fixed(want), (j, g, s)
                    if g != s:
                        assert _bits(x) == _bits(1.0 * pair[j][g][s] * pam[4 * (j % 4) + (g + s) % 4])
        # random pairs with many mismatches: the order of the product shows in the last bits
        for _ in range(400):
            guide = "".join(rng.choice(list(letters), 23))
            site = "".join(rng.choice(list(letters), 23))
            x, f = t.score(guide, site, fixed=True)
            want = py_score(pair, pam, guide, site)
            assert _bits(x) == _bits(want) and f == py_fixed(want)
        t.close()


def test_positions_20_to_22_and_non_acgt_letters():
    rng = np.random.default_rng(2031)
    pair, pam = random_table(rng)
    t = va.ScoreTable(pair, pam)
    guide = "ACGTACGTACGTACGTACGTAGG"
    site = "ACGTACCTACGTACGTTCGTAGG"
    base = t.score(guide, site)
    assert _bits(base) == _bits(1.0 * pair[6][2][1] * pair[16][0][3] * pam[4 * 2 + 2])
    # a mismatch of the READ at positions 20, 21 and 22 takes no part: only the site's letters 21, 22 pick the PAM weight
    for j in (20, 21, 22):
        for b in "ACGT":
            g2 = guide[:j] + b + guide[j + 1:]
            assert _bits(t.score(g2, site)) == _bits(base), (j, b)
    assert _bits(t.score(guide, site[:20] + "TGG")) == _bits(base)  # the site's letter 20 neither
    assert _bits(t.score(guide, site[:21] + "AG")) == _bits(1.0 * pair[6][2][1] * pair[16][0][3] * pam[4 * 0 + 2])
    # non-ACGT letters of a guide are A, as vsc_pack_guide codes them
    assert _bits(t.score("NCGTACGTRCGTACGTACGTAGG", site)) == _bits(t.score("ACGTACGTACGTACGTACGTAGG", site))
    assert code("N") == 0 and _bits(t.score("N" * 23, "A" * 20 + "AGG")) == _bits(1.0 * pam[4 * 2 + 2])
    t.close()


def test_the_minus_strand_mask_relation():
    """A record's mask is in genome orientation: on '-' its bit i is read position 22 - i.  Walking the mask's bits in ascending
    READ position (descending bit order on '-') over the site in read orientation is the definition's product."""
    rng = np.random.default_rng(2032)
    pair, pam = random_table(rng)
    t = va.ScoreTable(pair, pam)
    for _ in range(300):
        guide = "".join(rng.choice(list("ACGT"), 23))
        site = "".join(rng.choice(list("ACGT"), 23))  # read orientation
        read_mask = sum(1 << j for j in range(23) if guide[j] != site[j])
        minus_mask = sum(1 << (22 - j) for j in range(23) if (read_mask >> j) & 1)  # what a '-' record carries
        x = 1.0
        for i in range(22, 2, -1):  # descending bit order = ascending read position; bits 0..2 are read positions 22..20
            if (minus_mask >> i) & 1:
                j = 22 - i
                x = x * float(pair[j][code(guide[j])][code(site[j])])
        x = x * float(pam[4 * code(site[21]) + code(site[22])])
        assert _bits(t.score(guide, site)) == _bits(x)
    t.close()


# ------------------------------------------------------------------------------------ 4. refusals
def test_refusals():
    L = va.lib()
    pair, pam = random_table(np.random.default_rng(1))
    h = C.c_void_p()

    def build(p, q):
        p, q = np.ascontiguousarray(p), np.ascontiguousarray(q)
        return L.vsc_score_table_build(va._lib.ptr(p), va._lib.ptr(q), C.byref(h))

    assert build(pair, pam) == 0 and h.value
    good = C.c_void_p(h.value)
    for j, g, s, w in ((3, 1, 2, float("nan")), (3, 1, 2, -0.25), (3, 1, 2, 1.0000001), (19, 0, 3, float("inf")), (7, 2, 2, 0.999), (0, 0, 0, 0.0)):
        bad = pair.copy()
        bad[j, g, s] = w
        assert build(bad, pam) == ERR_INVALID and not h.value, (j, g, s, w)
        with pytest.raises(va.VarscotError):
            va.ScoreTable(bad, pam)
    for k, w in ((0, float("nan")), (15, -1e-9), (10, 2.0)):
        bad = pam.copy()
        bad[k] = w
        assert build(pair, bad) == ERR_INVALID and not h.value
    assert L.vsc_score_table_build(None, va._lib.ptr(pam), C.byref(h)) == ERR_INVALID
    assert L.vsc_score_table_build(va._lib.ptr(pair), None, C.byref(h)) == ERR_INVALID
    assert L.vsc_score_table_build(va._lib.ptr(pair), va._lib.ptr(pam), None) == ERR_INVALID
    assert L.vsc_table_score(None, 0, 0, None, None) == ERR_INVALID
    assert L.vsc_score_table_info(None, None) == ERR_INVALID and L.vsc_score_table_info(good, None) == ERR_INVALID
    assert L.vsc_table_score(good, 0, 0, None, None) == 0  # both outputs are optional
    assert L.vsc_score_table_free(good) == 0 and L.vsc_score_table_free(None) == 0
    with pytest.raises(ValueError):
        va.ScoreTable(pair[:19], pam)
    # weights 0 and 1 are inside the range
    edge = pair.copy()
    edge[5, 0, 1], edge[5, 0, 2] = 0.0, 1.0
    t = va.ScoreTable(edge, pam)
    assert t.score("A" * 20 + "AGG", "AAAAACAAAAAAAAAAAAAAAGG", fixed=True) == (0.0, 0)
    assert _bits(t.score("A" * 20 + "AGG", "AAAAAGAAAAAAAAAAAAAAAGG")) == _bits(pam[10])
    t.close()


# ------------------------------------------------------------------------------------ 5. the header's structs
def test_header_structs_and_abi_version(tmp_path):
    assert va.lib().vsc_abi_version() == 5 and re.search(r"#define\s+VSC_ABI_VERSION\s+5\b", HEADER)
    m = re.search(r"typedef struct \{([^}]*)\} vsc_guide_table_row;", HEADER)
    fields = re.findall(r"uint64_t\s+(\w+)(?:\[(\d+)\])?;", m.group(1))
    assert fields == [("score_sum", ""), ("positive", ""), ("positive_nm", "9"), ("reserved", "")]
    assert va.TABLE_ROW_DTYPE.itemsize == 96 and list(va.TABLE_ROW_DTYPE.names) == [f for f, _ in fields]
    assert va.TABLE_ROW_DTYPE.itemsize == va.VOTES_DTYPE.itemsize and C.sizeof(_lib.ScoreTableStats) == 16 and va.TABLE_ONE == ONE
    for name in ("vsc_score_table_build", "vsc_score_table_free", "vsc_score_table_info", "vsc_table_score", "vsc_table_specificity",
                 "vsc_score_hits_table", "vsc_search_summary_table", "vsc_search_select_table", "vsc_multi_search_summary_table"):
        assert name in HEADER and getattr(va.lib(), name)
    body = ('#include "varscot_hip.h"\n%s(sizeof(vsc_guide_table_row) == 96 && sizeof(vsc_guide_table_row) == sizeof(vsc_guide_votes), "row");\n'
            '%s(sizeof(vsc_score_table_stats) == 16 && VSC_ABI_VERSION == 5, "stats");\n'
            'int (*score)(const vsc_score_table *, uint64_t, uint64_t, double *, uint32_t *) = vsc_table_score;\n'
            'int main(void) { return 0; }\n')
    for compiler, flag, name, word in ((shutil.which("cc") or shutil.which("gcc"), "-std=c11", "layout.c", "_Static_assert"),
                                       (shutil.which("c++") or shutil.which("g++"), "-std=c++17", "layout.cpp", "static_assert")):
        if compiler:  # the header's own asserts, to a C and to a C++ compiler
            src = tmp_path / name
            src.write_text(body % (word, word))
            r = subprocess.run([compiler, flag, "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
            assert r.returncode == 0, r.stderr


# ------------------------------------------------------------------------------------ 6. loaders
def test_tsv_loader_and_its_errors(tmp_path):
    t = fixture_table()
    text = open(TABLE_TSV).read()
    assert text.count("# fitted\n") == 198 and text.count("# inferred\n") == 6 and text.count("\t?\t# unknown\n") == 52
    assert t.info()["zero_weights"] == 6 and t.pair[0, 0, 1] == 0.857142857 and t.pam[4 * 2 + 2] == 1.0
    assert (t.pair[np.arange(20)[:, None], np.arange(4), np.arange(4)] == 1.0).all()
    with pytest.raises(ValueError, match="missing or unknown"):
        va.ScoreTable.from_tsv(TABLE_TSV)

    def load(body, **kw):
        p = tmp_path / "t.tsv"
        p.write_text(body)
        return va.ScoreTable.from_tsv(str(p), **kw)

    t2 = load("# two entries\n4\tA\tc\t0.25\nPAM\tGG\t1\n\n", default=0.5)
    assert t2.pair[4, 0, 1] == 0.25 and t2.pam[10] == 1.0 and t2.pair[4, 0, 2] == 0.5 and t2.pair[4, 0, 0] == 1.0
    assert t2.score("A" * 20 + "AGG", "AAAACAAAAAAAAAAAAAAAAGG") == 0.25
    for bad in ("20\tA\tC\t0.5\n", "3\tA\tX\t0.5\n", "PAM\tG\t0.5\n", "3\tA\tC\n", "3\tA\tC\tabc\n", "x\tA\tC\t0.1\n"):
        with pytest.raises(ValueError, match="t.tsv:1"):
            load(bad, default=0.5)
    with pytest.raises(va.VarscotError):
        load("3\tA\tC\t1.5\n", default=0.5)  # the library's own range check
    with pytest.raises(va.VarscotError):
        load("3\tA\tA\t0.5\n", default=0.5)  # a diagonal entry other than 1


def test_doench_keys():
    """The mapping the docstring describes (nothing pins it to the published files): rX:dY,pos with X the guide letter (T as
    U), Y the complement of the site letter, pos 1-based."""
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    mm = {"r%s:d%s,%d" % (g.replace("T", "U"), comp[s], j + 1): (1 + j + 20 * "ACGT".index(g) + 80 * "ACGT".index(s)) / 400.0
          for j in range(20) for g in "ACGT" for s in "ACGT" if g != s}
    pams = {a + b: ("ACGT".index(a) * 4 + "ACGT".index(b)) / 16.0 for a in "ACGT" for b in "ACGT"}
    t = va.ScoreTable.from_doench(mm, pams)
    assert t.pair[0, 3, 2] == mm["rU:dC,1"] and t.pair[19, 2, 0] == mm["rG:dT,20"] and t.pam[4 * 2 + 2] == pams["GG"]
    del mm["rA:dA,7"]
    with pytest.raises(ValueError, match="missing"):
        va.ScoreTable.from_doench(mm, pams)
    assert va.ScoreTable.from_doench(mm, pams, default=0.5).pair[6, 0, 3] == 0.5


def test_guide_summary_table_argument_errors(tmp_path):
    (tmp_path / "g.fa").write_text(">c\n" + "ACGT" * 30 + "\n")
    (tmp_path / "r.fa").write_text(">r\n" + "ACGT" * 5 + "AGG\n")
    (tmp_path / "a.bed").write_text("c\t0\t100\n")
    (tmp_path / "s.vcf").write_text("##fileformat=VCFv4.2\n")
    tool = os.path.join(ROOT, "varscot_amd", "bin", "guide_summary")
    base = [tool, "-G", str(tmp_path / "g.fa"), "-I", str(tmp_path / "none"), "-M", "3", "-R", str(tmp_path / "r.fa")]
    w, hits = ["-W", TABLE_TSV], str(tmp_path / "hits.tsv")
    cases = [
        (["-W", str(tmp_path / "table.bed")], ".tsv"),                           # not a table file
        (w + ["-v", str(tmp_path / "s.vcf")], "-W does not combine"),            # no table scores for variant windows
        (w + ["-T", hits, "-A", str(tmp_path / "a.bed")], "-W does not combine"),
        (w + ["-T", hits, "-D", "0,0"], "-W does not combine"),                  # no multi-device selection by table score
        (w + ["-T", hits, "-S", "1.5"], "table score, 0 .. 1"),                  # the floor is in the table's units
        (w + ["-K", "3"], "give -T"),
    ]
    for extra, word in cases:
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0, extra
        assert word in r.stderr, (extra, r.stderr)
        assert "Index loaded" not in r.stderr and "no HIP device" not in r.stderr, r.stderr  # refused before any device work
        assert not os.path.exists(hits)
