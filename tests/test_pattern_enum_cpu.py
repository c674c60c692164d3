"""Pattern guide discovery without a device: vsc_pattern_guide_text against a letter-by-letter expansion, the targets' start
ranges against the rule applied to every position one by one, the struct layouts and macros as a C compiler sees them, the
presets' protospacers, the restatement's own floors, and pattern_search's enumeration arguments (all checked before a device
is opened)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import varscot_amd as va
from varscot_amd import _lib
import pattern_cases as pc
import pattern_enum_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "varscot_amd", "bin")


# ---- the letters of a code ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", range(16, 33))
def test_guide_text_equals_the_expansion(L):
    rng = np.random.default_rng(L)
    for a, k in ((0, L), (0, 1), (L - 1, 1), (0, L - 3), (3, L - 3), (4, L - 6), (2, 5)):  # either end, the whole, one letter
        for _ in range(4):
            s = pc.rnd(rng, L)
            for spell in (False, True):
                got = va.pattern_guide_text(ec.code_of(s), L, (a, k), spell)
                assert got == ec.guide_text(s, (a, k), spell) and len(got) == L
                assert spell or got[a:a + k] == s[a:a + k] and set(got[:a] + got[a + k:]) <= {"N"}
    assert va.pattern_guide_text(ec.code_of("T" * L), L, (0, L)) == "T" * L  # the highest bits of both planes


def test_guide_text_refusals():
    L = va.lib()
    buf = C.create_string_buffer(40)
    text = lambda code, n, a, k, spell, out=buf: L.vsc_pattern_guide_text(code, n, a, k, spell, out)
    assert text(0, 20, 0, 20, 0) == 0 and buf.raw[:21] == b"A" * 20 + b"\0"  # exactly len letters, no terminator
    for n in (0, 15, 33):
        assert text(0, n, 0, 10, 0) == -22
    assert text(0, 20, 0, 0, 0) == -22            # an empty protospacer
    assert text(0, 20, 1, 20, 0) == -22           # ... one that leaves the pattern
    assert text(0, 20, 21, 1, 0) == -22
    assert text(0, 20, 0xFFFFFFFF, 2, 0) == -22   # a + k overflows
    assert text(0, 20, 0, 20, 2) == -22           # spell is 0 or 1
    assert text(0, 20, 0, 20, 0, None) == -22
    assert text(1 << 20, 20, 0, 20, 0) == -22     # a bit from len on, lo plane ...
    assert text(1 << 52, 20, 0, 20, 0) == -22     # ... and hi plane
    assert text((1 << 19) | (1 << 51), 20, 0, 20, 1) == 0 and buf.raw[:20] == b"A" * 19 + b"T"
    assert text(2 ** 64 - 1, 32, 0, 32, 0) == 0 and buf.raw[:32] == b"T" * 32


# ---- the targets as ranges of site starts ---------------------------------------------------------------------------------
def ranges_of(contig_lens, targets, rule, L, capacity=64):
    """vsc_debug_pattern_target_ranges -> (status, [(lo, hi)] in global positions, contig offsets)"""
    packed = va.PackedGenome.from_sequences(["A" * n for n in contig_lens])
    contigs = np.ascontiguousarray(packed.contigs, dtype=va.CONTIG_DTYPE)
    iv = np.zeros(max(len(targets), 1), dtype=va.INTERVAL_DTYPE)
    for i, t in enumerate(targets):
        iv[i] = tuple(t) + (0,) * (4 - len(t))
    out, n = np.zeros((capacity, 2), dtype=np.uint32), C.c_uint64(0)
    rc = va.lib().vsc_debug_pattern_target_ranges(_lib.ptr(contigs), len(contigs), _lib.ptr(iv), len(targets), rule, L, _lib.ptr(out), capacity,
                                                  C.byref(n))
    return rc, [tuple(int(x) for x in r) for r in out[:n.value]] if rc == 0 else n.value, [int(x) for x in contigs["offset"]]


@pytest.mark.parametrize("rule", ["overlap", "inside"])
@pytest.mark.parametrize("L", [16, 20, 23, 32])
def test_start_ranges_equal_the_rule_site_by_site(L, rule):
    n, small = 3 * ec.TILE + 300, 61
    lens = [n, small, L - 1]
    targets = ec.target_intervals(n, small) + [(2, 0, L - 1), (0, 2500, 2500 + L), (0, 2600, 2600 + L - 1)]
    rc, ranges, off = ranges_of(lens, targets, 1 if rule == "inside" else 0, L)
    assert rc == 0
    assert all(lo < hi for lo, hi in ranges) and all(a[1] < b[0] for a, b in zip(ranges, ranges[1:]))  # sorted, disjoint, not abutting
    got = {(c, p - off[c]) for lo, hi in ranges for p in range(lo, hi) for c in [max(k for k in range(len(off)) if off[k] <= p)]}
    want = ec.start_ranges(lens, targets, rule, L)
    assert got == want and all(p < lens[c] for c, p in got)
    # the shapes, on the restatement's own output
    has = lambda c, p: (c, p) in want
    if rule == "overlap":
        assert has(0, 0) and has(0, 5 - 1) and has(0, 39) and not has(0, 40)          # start < L - 1: cut at 0
        assert has(0, 1800 - L + 1) and not has(0, 1800 - L) and has(0, 1809) and not has(0, 1810)  # shorter than L
        assert has(0, n - 1) and has(0, n - 30 - L + 1) and not has(0, n - 30 - L)    # the end past the contig
        assert has(0, 1099) and has(0, 1100)                                         # abutting: one range
        assert has(2, 0) and has(2, L - 2)                                           # a contig no site fits in: starts all the same
    else:
        assert has(0, 5) and has(0, 40 - L) and not has(0, 40 - L + 1)
        assert not any(has(0, p) for p in range(1790, 1811))                         # shorter than L: none
        assert has(0, n - L) == (L <= 30) and has(0, n - 30) == (L <= 30)
        assert has(0, 1100 - L) and not any(has(0, p) for p in range(1100 - L + 1, 1100)) and has(0, 1100)  # the seam
        assert has(0, 2500) and not has(0, 2501) and not has(0, 2600)                # exactly L bases, and one less
        assert not has(2, 0)
    assert not has(0, 300)                                                           # the empty interval adds nothing


def test_start_ranges_refusals_and_empty_sets():
    assert ranges_of([100], [], 0, 20)[:2] == (0, [])
    assert ranges_of([100], [(0, 50, 50)], 0, 20)[:2] == (0, [])
    assert ranges_of([100], [(0, 100, 200)], 0, 20)[:2] == (0, [])                  # empty after clipping
    assert ranges_of([100], [(0, 10, 20)], 1, 20)[:2] == (0, [])                    # inside: no site fits
    assert ranges_of([100], [(0, 10, 30)], 1, 20)[:2] == (0, [(10, 11)])
    assert ranges_of([100], [(0, 10, 30)], 0, 20)[:2] == (0, [(0, 30)])
    assert ranges_of([100, 50], [(1, 0, 500)], 0, 16)[:2] == (0, [(101, 151)])      # global positions: offset 101
    for bad in ([(1, 0, 10)], [(0, 11, 10)], [(0, 0, 10, 1)]):
        assert ranges_of([100], bad, 0, 20)[0] == -22
    assert ranges_of([100], [(0, 0, 10)], 2, 20)[0] == -22                           # an unknown rule
    assert ranges_of([100], [(0, 0, 10)], 0, 15)[0] == -22 and ranges_of([100], [(0, 0, 10)], 0, 33)[0] == -22
    rc, n, _ = ranges_of([1000], [(0, 100, 110), (0, 300, 310), (0, 500, 510)], 0, 20, capacity=2)
    assert rc == -34 and n == 3


# ---- layouts, macros, presets ---------------------------------------------------------------------------------------------
def test_struct_layout_and_presets(tmp_path):
    assert C.sizeof(va.PatternEnumParams) == 32
    offsets = {name: getattr(va.PatternEnumParams, name).offset for name, _ in va.PatternEnumParams._fields_}
    assert offsets == {"ps_start": 0, "ps_len": 1, "strands": 2, "gc_min": 3, "gc_max": 4, "max_t_run": 5, "reserved0": 6, "rule": 8,
                       "reserved1": 12, "max_guides": 16, "reserved": 24}
    assert ec.LOCUS_DTYPE == va.LOCUS_DTYPE
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc:  # the header's own asserts and macros, to a C compiler
        src = tmp_path / "layout.c"
        src.write_text('#include <stddef.h>\n#include "varscot_hip.h"\n'
                       '_Static_assert(sizeof(vsc_pattern_enum_params) == 32 && sizeof(vsc_interval) == 16 && sizeof(vsc_locus) == 16, "size");\n'
                       '_Static_assert(offsetof(vsc_pattern_enum_params, ps_len) == 1 && offsetof(vsc_pattern_enum_params, max_t_run) == 5, "a");\n'
                       '_Static_assert(offsetof(vsc_pattern_enum_params, rule) == 8 && offsetof(vsc_pattern_enum_params, max_guides) == 16, "b");\n'
                       '_Static_assert(offsetof(vsc_pattern_enum_params, reserved) == 24, "c");\n'
                       '_Static_assert(VSC_REGION_OVERLAP == 0 && VSC_REGION_INSIDE == 1 && VSC_ABI_VERSION == 5, "d");\n'
                       '_Static_assert(VSC_PATTERN_MIN_LEN == 16 && VSC_PATTERN_MAX_LEN == 32, "e");\n'
                       'int main(void) { vsc_pattern_guides *g = 0; return vsc_pattern_guides_count(g) != 0; }\n')
        r = subprocess.run([cc, "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    for name, (five, n, three) in va.PATTERNS.items():
        a, k = va.pattern_protospacer(name)
        pattern, guide = va.pattern_strings(name, "A" * n)
        assert (a, k) == (len(five), n) and pattern[a:a + k] == "N" * k and guide[a:a + k] == "A" * n and a + k + len(three) == len(pattern)
    assert va.pattern_protospacer("SaCas9") == (0, 21) and va.pattern_protospacer("Cas12a") == (4, 23)
    assert va.pattern_protospacer(("TT", 18, "G")) == (2, 18)
    with pytest.raises(KeyError):
        va.pattern_protospacer("Cas99")


def test_python_argument_checks():
    """What cannot be put into the struct is refused before the library is called (no device: the genome is never touched)."""
    gen = va.Genome.__new__(va.Genome)  # never loaded
    gen._h = C.c_void_p()
    for kw in (dict(rule="near"), dict(strands="x"), dict(gc=(0, 300)), dict(max_t_run=-1)):
        with pytest.raises(ValueError):
            gen.enumerate_pattern("N" * 20, (0, 20), **kw)
    with pytest.raises(ValueError):
        gen.enumerate_pattern("N" * 20, (0, 256))
    with pytest.raises(ValueError):
        gen.enumerate_pattern("N" * 20, (0, 20), targets=[(0, -1, 5)])


def test_the_restatement_on_a_site_worked_by_hand():
    """candidates() / kept() on sites small enough to check on paper."""
    pattern = "CAN" + "N" * 13                                                   # L = 16, protospacer (3, 13)
    site = "CAG" + "TTTAC" + "GGCCT" + "TTA"                                     # protospacer TTTACGGCCTTTA: 5 G/C, T runs of 3
    contig = "AC" + site + "GG" + pc.rc(site) + "GN" + site[:-1]                 # the third copy leaves the contig
    found = ec.candidates([contig], pattern)
    assert [(c, p, s) for c, p, s, _ in found] == [(0, 2, 0), (0, 20, 1)]
    assert found[0][3] == site and found[1][3] == site
    assert ec.kept(found, [contig], 16, (3, 13), max_t_run=2) == [] and len(ec.kept(found, [contig], 16, (3, 13), max_t_run=3)) == 2
    assert len(ec.kept(found, [contig], 16, (3, 13), gc=(5, 5))) == 2 and ec.kept(found, [contig], 16, (3, 13), gc=(6, 0)) == []
    assert ec.kept(found, [contig], 16, (3, 13), targets=[(0, 2, 18)], rule="inside") == found[:1]
    assert ec.kept(found, [contig], 16, (3, 13), targets=[(0, 3, 18)], rule="inside") == []
    assert ec.kept(found, [contig], 16, (3, 13), targets=[(0, 17, 21)], rule="overlap") == found
    assert ec.kept(found, [contig], 16, (3, 13), targets=[]) == []
    assert ec.code_of("ACGT") == (0b1100 << 32) | 0b1010
    assert ec.n_run("SWNNNNWS") == (2, 4) and ec.n_run("NNNRRT") == (0, 3) and ec.n_run("TTVNNN") == (3, 3)


def test_scenario_floors_hold():
    """Building a scenario asserts its floors (tests/pattern_enum_cases.py); the GPU tests build the rest."""
    assert len(ec.full_scenario()["cands"]) == 2 * (2 * ec.TILE + 22) + 6
    for which in ("sa", "five"):
        assert ec.filter_scenario(which)["cands"]
    assert ec.target_scenario()["cands"]
    assert ec.edge_scenario(16, "both")["protospacer"] == (2, 12)


# ---- the tool's arguments -------------------------------------------------------------------------------------------------
def _run(*args):
    return subprocess.run([os.path.join(BIN, "pattern_search")] + list(args), capture_output=True, text=True, timeout=120,
                          env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))


def test_pattern_search_enumeration_argument_errors(tmp_path):
    (tmp_path / "g.fa").write_text(">r one\n" + "ACGT" * 5 + "NNN\n")
    (tmp_path / "t.bed").write_text("c0\t10\t90\n")
    idx, pattern, g = str(tmp_path / "idx"), "N" * 21 + "NNGRRT", str(tmp_path / "g.fa")
    e = ["-E", str(tmp_path / "guides.tsv")]
    base = ["-i", idx, "-q", pattern] + e
    res = _run(*base)                                                          # -p is required with -E
    assert res.returncode == 1 and "-p" in res.stderr
    for bad in ("0", "0,0", "7,21", "x,3", "0,21,1", "-1,5", "0,300"):
        res = _run(*base, "-p", bad)
        assert res.returncode == 1 and "-p" in res.stderr, bad
    ok = base + ["-p", "0,21"]
    res = _run(*ok, "-R", g)
    assert res.returncode == 1 and "-R" in res.stderr                         # the guides are found, not given
    res = _run(*ok, "-T", str(tmp_path / "hits.tsv"))
    assert res.returncode == 1 and "-T" in res.stderr
    res = _run(*ok, "-M", "3")                                                # -M and -O go together
    assert res.returncode == 1 and "-O" in res.stderr
    res = _run(*ok, "-O", str(tmp_path / "sum.tsv"))
    assert res.returncode == 1 and "-M" in res.stderr
    res = _run(*ok, "-M", "9", "-O", str(tmp_path / "sum.tsv"))
    assert res.returncode == 1 and "between 0 and 8" in res.stderr
    assert _run("-i", idx, "-q", pattern, "-E", str(tmp_path / "guides.bed"), "-p", "0,21").returncode == 1  # wrong extensions
    assert _run(*ok, "-B", str(tmp_path / "t.txt")).returncode == 1
    res = _run(*ok, "-r", "inside")                                           # a rule without targets
    assert res.returncode == 1 and "-B" in res.stderr
    res = _run(*ok, "-B", str(tmp_path / "t.bed"), "-r", "near")
    assert res.returncode == 1 and "overlap" in res.stderr
    res = _run(*ok, "-s", "x")
    assert res.returncode == 1 and "-s" in res.stderr
    for bad in ("5", "12,8", "0,22", "a,b"):
        res = _run(*ok, "-g", bad)
        assert res.returncode == 1 and "-g" in res.stderr, bad
    for bad in ("-1", "256", "x"):
        res = _run(*ok, "-t", bad)
        assert res.returncode == 1 and "-t" in res.stderr, bad
    res = _run("-i", idx, "-q", "N" * 15, *e, "-p", "0,10")
    assert res.returncode == 1 and "16..32" in res.stderr
    # the enumeration's options without -E; and -R / -M are still required without it
    res = _run("-i", idx, "-q", pattern, "-R", g, "-M", "3", "-O", str(tmp_path / "o.tsv"), "-p", "0,21")
    assert res.returncode == 1 and "-E" in res.stderr
    res = _run("-i", idx, "-q", pattern, "-M", "3", "-O", str(tmp_path / "o.tsv"))
    assert res.returncode == 1 and "Missing value for option: -R" in res.stderr
    res = _run("-i", idx, "-q", pattern, "-R", g, "-O", str(tmp_path / "o.tsv"))
    assert res.returncode == 1 and "Missing value for option: -M" in res.stderr
    # well-formed calls get as far as the index, which does not exist: nothing above was about their arguments
    for more in ([], ["-B", str(tmp_path / "t.bed"), "-r", "inside", "-s", "+", "-g", "8,14", "-t", "3", "-M", "2", "-O", str(tmp_path / "sum.tsv")]):
        res = _run(*ok, *more)
        assert res.returncode == 1 and "idx" in res.stderr, res.stderr
    assert not (tmp_path / "guides.tsv").exists() and not (tmp_path / "sum.tsv").exists()
    res = _run("--help")
    assert res.returncode == 0 and "-E, --enumerate" in res.stdout and "-p, --protospacer" in res.stdout and "-B, --targets" in res.stdout
