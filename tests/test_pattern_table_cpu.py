"""The pattern table score without a device: vsc_pattern_table_score against the restatement (tests/pattern_table_cases.py) bit
for bit over random shapes, the floors of the digit scenarios by name, the SpCas9 anchor over every row of the CRISPOR fixture,
what vsc_pattern_table_build refuses, the header's structs under a C and a C++ compiler, the TSV round trip and pattern_search's
argument checks.  (The refusals of vsc_search_pattern_table itself need a context, that is a device:
tests/test_pattern_table.py.)"""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import varscot_amd as va
import pattern_cases as pc
import pattern_table_cases as tc
from table_cases import fixture_rows, fixture_table
from varscot_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "varscot_hip.h")).read()
ERR_INVALID = -22
_bits = lambda x: struct.pack("<d", x)


def test_the_scenarios_hold_their_floors():
    s = tc.select_scenario()
    assert len(s["hits"]) == len(s["f"]) and tc.edge_table(23, "both")["f"].dtype == np.uint32


def lexsort_cut(guide_of, f, n_guides, top_k, min_score):
    """cut() once more, on the f array alone: per guide np.lexsort on (-f, record index) over the survivors."""
    guide_of, f = np.asarray(guide_of), np.asarray(f, dtype=np.int64)
    keep = []
    for g in range(n_guides):
        idx = np.nonzero((guide_of == g) & (f >= min_score))[0]
        if top_k and len(idx) > top_k:
            idx = idx[np.lexsort((idx, -f[idx]))[:top_k]]
        keep.extend(int(i) for i in idx)
    return np.array(sorted(keep), dtype=np.int64)


def test_the_digit_scenarios_hold_their_floors():
    """digits_scenario() and digits_wide(): every condition that keeps the device tests from hiding a failure, by name, on the
    restatement's own output; and cut() against a second restatement over every case."""
    s = tc.digits_scenario()
    guide_of = [h[0] for h in s["hits"]]
    assert len(s["contigs"]) == 1 and len(s["contigs"][0]) < 80000 and len(s["guides"]) == 4
    assert len(s["cases"]) == len(set(s["cases"])) == len(s["serves"]) <= tc.MAX_CASES
    for top_k, min_score in s["cases"]:
        assert (tc.cut(s["hits"], s["f"], top_k, min_score) == lexsort_cut(guide_of, s["f"], 4, top_k, min_score)).all(), (top_k, min_score)
    unmet = tc.digit_floors(guide_of, s["f"], 4, s["cases"], lambda k, ms: lexsort_cut(guide_of, s["f"], 4, k, ms))
    assert not unmet, "digits_scenario() does not reach: %s" % ", ".join(unmet)
    # the conditions bite: without its cases below the top digit, without its long segments, the list is found wanting
    few = tc.digit_floors(guide_of, s["f"], 4, [c for c in s["cases"] if c[0] in (1, 700, 701, 300, 301)], lambda k, ms: tc.cut(s["hits"], s["f"], k, ms))
    assert {"larger 1", "larger 2", "T = 0", "min_score = T"} <= set(few)
    short = [k for k, h in enumerate(s["hits"]) if h[0] == 3]
    assert {"ties over steps", "two and three steps", "empty segment"} <= set(
        tc.digit_floors([0] * len(short), s["f"][short], 1, s["cases"], lambda k, ms: lexsort_cut([0] * len(short), s["f"][short], 1, k, ms)))
    assert len(np.unique(s["f"])) > 200 and (s["f"] == 0).any()
    w = tc.digits_wide()
    n_tiles = len(w["contigs"][0]) // pc.TILE
    guide_of = [h[0] for h in w["hits"]]
    assert len(w["guides"]) == 66 and len(w["contigs"][0]) < 80000, "digits_wide(): sizes"
    assert 2 * 64 * n_tiles > 4096, "digits_wide(): one round of 64 guides has two groups of cells"
    beyond = {g for g in set(guide_of) if g < 64 and 2 * g * n_tiles >= 4096}
    assert len(beyond) >= 2, "digits_wide(): two guides with records begin in the second group"
    truncated_ties = False
    for top_k, min_score in w["cases"]:
        keep = tc.cut(w["hits"], w["f"], top_k, min_score)
        assert (keep == lexsort_cut(guide_of, w["f"], 66, top_k, min_score)).all(), (top_k, min_score)
        assert {64, 65} <= {guide_of[i] for i in keep}, "digits_wide(): the second round keeps records of its own"
        t = tc.case_facts(guide_of, w["f"], 66, keep, top_k, min_score)
        truncated_ties |= any(g in beyond and t[g]["kept_ties"] and t[g]["dropped_ties"] for g in t)
    assert truncated_ties, "digits_wide(): a guide of the second group truncates inside its ties"


# ------------------------------------------------------------------------------------ 1. the definition, bit for bit
@pytest.mark.parametrize("n_pam", [0, 2, 4])
@pytest.mark.parametrize("where", ["5", "3", "middle"])
@pytest.mark.parametrize("L", [16, 23, 32])
def test_score_equals_the_restatement_bit_for_bit(L, where, n_pam):
    rng = np.random.default_rng(100 * L + 10 * n_pam + len(where))
    ps_len = L - 6
    ps_start = {"5": 0, "3": L - ps_len, "middle": 3}[where]
    outside = [j for j in range(L) if not ps_start <= j < ps_start + ps_len]
    pam_pos = tuple(sorted(int(x) for x in rng.choice(outside, size=n_pam, replace=False)))
    table = tc.random_pattern_table(rng, (L, (ps_start, ps_len), pam_pos), zeros=5, ones=5)
    obj = tc.make_table(va, table)
    info = obj.info()
    assert info["length"] == L and info["protospacer"] == (ps_start, ps_len) and info["pam_positions"] == pam_pos
    assert info["zero_weights"] == int((table["pair"] == 0).sum() + (table["pam"] == 0).sum())
    letters = "ACGT" * 6 + "RYSWKMBDHVN"
    seen = set()
    for n in range(300):
        guide = "".join(letters[k] for k in rng.integers(0, len(letters), L))
        if n % 3 == 0:
            guide = guide.lower()
        site = "".join(rng.choice(list(pc.IUPAC[g.upper()])) if rng.random() < 0.7 else "ACGT"[rng.integers(4)] for g in guide)
        x, f = obj.score(guide, site, fixed=True)
        want = tc.py_score(table, guide, site)
        assert _bits(x) == _bits(want) and f == tc.py_fixed(want), (guide, site)
        seen.add(0 if f == 0 else (2 if f == tc.ONE else 1))
    assert seen >= {0, 1}
    obj.close()


def test_degenerate_letters_and_the_positions_outside():
    table = tc.random_pattern_table(np.random.default_rng(5), (20, (2, 14), (0, 18)))
    obj = tc.make_table(va, table)
    guide = "TT" + "ACGTACGTACGTAC" + "GGGG"
    site = "AC" + "ACGTACGTACGTAC" + "TCAT"       # differs outside the protospacer only: the PAM weight alone
    assert _bits(obj.score(guide, site)) == _bits(float(table["pam"][4 * 0 + 0]))
    degenerate = "TT" + "RCGTNCGTACGTAB" + "GGGG"  # R against C, N against T, B against A: mismatches in NM, no factor
    site2 = "AC" + "CCGTTCGTACGTAA" + "TCAT"
    assert pc.site_match("N" * 20, degenerate, site2)[1] >= 2
    assert _bits(obj.score(degenerate, site2)) == _bits(float(table["pam"][0]))
    with pytest.raises(va.VarscotError):
        obj.score(guide, site[:5] + "N" + site[6:])  # a site letter outside ACGT
    with pytest.raises(va.VarscotError):
        obj.score(guide[:5] + "U" + guide[6:], site)
    with pytest.raises(ValueError):
        obj.score(guide, site + "A")
    L = va.lib()
    assert L.vsc_pattern_table_score(obj._h, guide.encode(), site.encode(), None, None) == 0  # both outputs are optional
    assert L.vsc_pattern_table_score(None, guide.encode(), site.encode(), None, None) == ERR_INVALID
    assert L.vsc_pattern_table_score(obj._h, None, site.encode(), None, None) == ERR_INVALID


# ------------------------------------------------------------------------------------ 2. the anchor
def test_anchor_every_crispor_row():
    plain = fixture_table()
    table = va.PatternTable.from_score_table(plain)
    assert table.length == 23 and table.protospacer == (0, 20) and table.pam_positions == (21, 22)
    rows = fixture_rows()
    assert len(rows["site"]) > 100
    for g, site in zip(rows["guide"], rows["site"]):
        guide = rows["guides"][g]
        assert table.score(guide, site, fixed=True)[1] == plain.score(guide, site, fixed=True)[1]
        assert _bits(table.score(guide, site)) == _bits(plain.score(guide, site))


# ------------------------------------------------------------------------------------ 3. refusals
def test_build_refusals():
    L = va.lib()
    good = tc.random_pattern_table(np.random.default_rng(1), (23, (0, 20), (21, 22)))
    h = C.c_void_p()

    def build(shape, pair, pam):
        s = _lib.PatternTableShape(*shape[:4])
        for t, q in enumerate(shape[4]):
            s.pam_pos[t] = q
        pair, pam = np.ascontiguousarray(pair, dtype=np.float64), np.ascontiguousarray(pam, dtype=np.float64)
        rc = L.vsc_pattern_table_build(C.byref(s), _lib.ptr(pair), _lib.ptr(pam), C.byref(h))
        if rc == 0:
            L.vsc_pattern_table_free(h)
        return rc

    ok = (23, 0, 20, 2, (21, 22))
    assert build(ok, good["pair"], good["pam"]) == 0
    for i, g, s, w in ((3, 1, 2, float("nan")), (3, 1, 2, -0.25), (3, 1, 2, 1.0000001), (19, 0, 3, float("inf")), (7, 2, 2, 0.999), (0, 0, 0, 0.0)):
        bad = good["pair"].copy()
        bad[i, g, s] = w
        assert build(ok, bad, good["pam"]) == ERR_INVALID and not h.value, (i, g, s, w)
        with pytest.raises(va.VarscotError):
            va.PatternTable(23, (0, 20), bad, (21, 22), good["pam"])
    for k, w in ((0, float("nan")), (15, -1e-9), (10, 2.0)):
        bad = good["pam"].copy()
        bad[k] = w
        assert build(ok, good["pair"], bad) == ERR_INVALID
    big = np.ones((32, 4, 4))
    for shape in ((23, 0, 20, 2, (19, 22)),     # a PAM position inside the protospacer
                  (23, 0, 20, 2, (22, 21)),     # not ascending
                  (23, 0, 20, 2, (21, 21)),
                  (23, 0, 20, 2, (21, 23)),     # outside the L positions
                  (23, 4, 20, 0, ()),           # the protospacer leaves the L positions
                  (23, 0, 0, 0, ()),            # an empty protospacer
                  (15, 0, 12, 0, ()), (33, 0, 20, 0, ()),
                  (23, 0, 20, 5, (20, 21, 22, 22))):
        assert build(shape, big, np.ones(256)) == ERR_INVALID, shape
    s = _lib.PatternTableShape(23, 0, 20, 2)
    assert L.vsc_pattern_table_build(None, _lib.ptr(good["pair"]), _lib.ptr(good["pam"]), C.byref(h)) == ERR_INVALID
    assert L.vsc_pattern_table_build(C.byref(s), None, _lib.ptr(good["pam"]), C.byref(h)) == ERR_INVALID
    assert L.vsc_pattern_table_build(C.byref(s), _lib.ptr(good["pair"]), None, C.byref(h)) == ERR_INVALID
    assert L.vsc_pattern_table_info(None, None) == ERR_INVALID and L.vsc_pattern_table_free(None) == 0
    assert L.vsc_search_pattern_table(None, None, b"N" * 23, b"A" * 23, 1, 23, None, None, None, None, None, None) == ERR_INVALID
    with pytest.raises(ValueError):
        va.PatternTable(23, (0, 20), good["pair"][:19], (21, 22), good["pam"])
    with pytest.raises(ValueError):
        va.PatternTable(23, (0, 20), good["pair"], (21,), good["pam"])
    # the edges of the shape, and weights 0 and 1, are inside
    assert build((16, 0, 16, 0, ()), big[:16], [0.0]) == 0 and build((32, 0, 28, 4, (28, 29, 30, 31)), big[:28], np.ones(256)) == 0
    assert build((32, 31, 1, 1, (0,)), big[:1], [1.0, 0.0, 0.5, 1.0]) == 0


# ------------------------------------------------------------------------------------ 4. the header's structs
def test_header_structs_and_abi_version(tmp_path):
    assert va.lib().vsc_abi_version() == 5 and re.search(r"#define\s+VSC_ABI_VERSION\s+5\b", HEADER)
    assert C.sizeof(_lib.PatternTableShape) == 32 and C.sizeof(_lib.PatternTableStats) == 48 and C.sizeof(_lib.PatternSelect) == 16
    for name in ("vsc_pattern_table_build", "vsc_pattern_table_free", "vsc_pattern_table_info", "vsc_pattern_table_score",
                 "vsc_search_pattern_table", "vsc_pattern_hits_scores", "vsc_pattern_hits_scores_dev"):
        assert name in HEADER and getattr(va.lib(), name)
    body = ('#include "varscot_hip.h"\n%s(sizeof(vsc_pattern_table_shape) == 32 && sizeof(vsc_pattern_table_stats) == 48, "table");\n'
            '%s(sizeof(vsc_pattern_select) == 16 && sizeof(vsc_guide_table_row) == 96 && VSC_ABI_VERSION == 5, "select");\n'
            'int (*score)(const vsc_pattern_table *, const char *, const char *, double *, uint32_t *) = vsc_pattern_table_score;\n'
            'int (*scores)(vsc_pattern_hits *, const uint32_t **) = vsc_pattern_hits_scores;\n'
            'int main(void) { vsc_pattern_select s = {0, 0, {0, 0}}; vsc_pattern_table_shape t = {23, 0, 20, 2, {21, 22, 0, 0}};\n'
            '                 return (int)(s.top_k + t.n_pam) - 2; }\n')
    for compiler, flag, name, word in ((shutil.which("cc") or shutil.which("gcc"), "-std=c11", "layout.c", "_Static_assert"),
                                       (shutil.which("c++") or shutil.which("g++"), "-std=c++17", "layout.cpp", "static_assert")):
        if compiler:  # the header's own asserts, to a C and to a C++ compiler
            src = tmp_path / name
            src.write_text(body % (word, word))
            r = subprocess.run([compiler, flag, "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
            assert r.returncode == 0, r.stderr


# ------------------------------------------------------------------------------------ 5. the text file
@pytest.mark.parametrize("shape", [(23, (0, 20), (21, 22)), (24, (4, 20), (0, 1, 2, 3)), (16, (0, 16), ())])
def test_tsv_round_trip_to_the_bit(tmp_path, shape):
    table = tc.random_pattern_table(np.random.default_rng(9), shape, zeros=3, ones=3)
    a = tc.make_table(va, table)
    a.to_tsv(str(tmp_path / "t.tsv"))
    b = va.PatternTable.from_tsv(str(tmp_path / "t.tsv"))
    assert (b.length, b.protospacer, b.pam_positions) == (a.length, a.protospacer, a.pam_positions)
    assert b.pair.tobytes() == a.pair.tobytes() and b.pam.tobytes() == a.pam.tobytes()
    assert b.info()["serial"] != a.info()["serial"]


def test_tsv_errors(tmp_path):
    def load(body):
        p = tmp_path / "t.tsv"
        p.write_text(body)
        return va.PatternTable.from_tsv(str(p))

    head = "shape 16 0 16\n"
    full = head + "pam_pos\n" + "".join("pair %d %s %s 0.5\n" % (j, g, s) for j in range(16) for g in "ACGT" for s in "ACGT" if g != s) + "pam - 0.25\n"
    t = load("# a comment\n" + full)
    assert t.pair[3, 0, 1] == 0.5 and t.pam[0] == 0.25 and t.score("A" * 16, "C" + "A" * 15) == 0.125
    for bad, where in (("pair 0 A C 0.5\n", 1), (head + "pair 16 A C 0.5\n", 2), (head + "pair 3 A X 0.5\n", 2), (head + "pam G 0.5\n", 2),
                       (head + "pair 3 A C abc\n", 2), (head + "what 1\n", 2), (head + head, 2), (head + "pam_pos 1 2 3 4 5\n", 2)):
        with pytest.raises(ValueError, match="t.tsv:%d" % where):
            load(bad)
    with pytest.raises(ValueError, match="missing"):
        load(full.replace("pair 7 G T 0.5\n", ""))
    with pytest.raises(ValueError, match="no 'shape'"):
        load("# nothing\n")
    with pytest.raises(va.VarscotError):
        load(full.replace("pair 7 G T 0.5\n", "pair 7 G T 1.5\n"))  # the library's own range check
    with pytest.raises(va.VarscotError):
        load(full + "pair 7 G G 0.5\n")                            # a diagonal entry other than 1


# ------------------------------------------------------------------------------------ 6. the tool's argument checks
def test_pattern_search_table_argument_errors(tmp_path):
    (tmp_path / "r.fa").write_text(">r\n" + "ACGT" * 5 + "NNN\n")
    table = tc.make_table(va, tc.random_pattern_table(np.random.default_rng(2), (23, (0, 20), (21, 22))))
    table.to_tsv(str(tmp_path / "table.tsv"))
    tc.make_table(va, tc.random_pattern_table(np.random.default_rng(2), (22, (0, 20), (21,)))).to_tsv(str(tmp_path / "short.tsv"))
    (tmp_path / "broken.tsv").write_text("shape 23 0 20\npam_pos 21 22\n")
    tool = os.path.join(ROOT, "varscot_amd", "bin", "pattern_search")
    base = [tool, "-i", str(tmp_path / "none"), "-q", "N" * 20 + "NGG", "-R", str(tmp_path / "r.fa"), "-M", "3", "-O", str(tmp_path / "sum.tsv")]
    w, hits = ["-W", str(tmp_path / "table.tsv")], str(tmp_path / "hits.tsv")
    cases = [
        (["-W", str(tmp_path / "table.bed")], ".tsv"),                           # not a table file
        (["-T", hits, "-K", "3"], "give -W"),                                    # a selection without a table
        (w + ["-K", "3"], "give -W and -T"),                                     # ... or without a listing
        (w + ["-T", hits, "-K", "0"], "-K takes"),
        (w + ["-T", hits, "-S", "1.5"], "table score of 0 .. 1"),                # the floor is in the table's units
        (w + ["-T", hits, "-S", "x"], "table score of 0 .. 1"),
        (["-W", str(tmp_path / "short.tsv")], "built for 22 letters"),
        (["-W", str(tmp_path / "broken.tsv")], "entries are missing"),
    ]
    for extra, word in cases:
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0, extra
        assert word in r.stderr, (extra, r.stderr)
        assert "Index loaded" not in r.stdout + r.stderr and "no HIP device" not in r.stderr, r.stderr  # refused before any device work
        assert not os.path.exists(hits) and not os.path.exists(tmp_path / "sum.tsv")
