"""Guide discovery's host side, no device needed: the new entry points are declared, exported and bound, the parameter block's
layout, guide_summary's -E argument checks (all made before a device is opened), and the brute force of
tests/enumerate_cases.py against windows worked out by hand."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import varscot_amd as va
from varscot_amd import _lib
import enumerate_cases as ec
from helpers import revcomp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.environ.get("VSC_TEST_BIN") or os.path.join(ROOT, "varscot_amd", "bin")
NEW = ["vsc_guides_enumerate", "vsc_guides_count", "vsc_guides_data", "vsc_guides_data_dev", "vsc_guides_free",
       "vsc_multi_guides_enumerate"]


def test_new_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "varscot_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    bound = {name for name, _, _ in _lib.SYMBOLS}
    L = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in bound, name
        assert hasattr(L, name), name
        assert getattr(va.lib(), name).argtypes is not None
    assert int(re.search(r"#define\s+VSC_ABI_VERSION\s+(\d+)", text).group(1)) == 5  # additive: the version stays
    assert va.lib().vsc_abi_version() == 5
    # the header cites what the call replaces
    assert "extract_fasta_ontargets.h:92-139" in text[text.index("Guide discovery"):text.index("vsc_guides_enumerate(")]


def test_enum_params_layout(tmp_path):
    assert C.sizeof(_lib.EnumParams) == 24 and va.EnumParams is _lib.EnumParams
    f = _lib.EnumParams
    assert [(n, getattr(f, n).offset) for n, _ in f._fields_] == [
        ("pam", 0), ("strands", 2), ("gc_min", 3), ("gc_max", 4), ("max_t_run", 5), ("reserved0", 6), ("max_guides", 8),
        ("reserved", 16)]
    # the header asserts the same size to a C and to a C++ compiler
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc:
        src = tmp_path / "layout.c"
        src.write_text('#include "varscot_hip.h"\n_Static_assert(sizeof(vsc_enum_params) == 24, "size");\n'
                       '_Static_assert(sizeof(vsc_locus) == 16, "locus");\nint main(void) { return 0; }\n')
        r = subprocess.run([cc, "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True,
                           text=True)
        assert r.returncode == 0, r.stderr


def test_unpack_guides_inverts_pack_guides():
    guides = ["ACGTACGTACGTACGTACGTAGG", "T" * 23, "CC" + "A" * 19 + "GG"]
    codes = va.pack_guides(guides)
    assert va.unpack_guides(codes) == guides
    assert [int(c) for c in codes] == [ec.code_of(g) for g in guides]
    assert va.unpack_guides(np.zeros(0, dtype=np.uint64)) == []


def _run(*args):
    return subprocess.run([os.path.join(BIN, "guide_summary")] + list(args), capture_output=True, text=True, timeout=120,
                          env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))


def test_guide_summary_discovery_argument_errors(tmp_path):
    (tmp_path / "g.fa").write_text(">c\n" + "ACGT" * 30 + "\n")
    (tmp_path / "r.fa").write_text(">r\n" + "ACGT" * 5 + "AGG\n")
    (tmp_path / "t.bed").write_text("c\t0\t100\n")
    g, r, t = str(tmp_path / "g.fa"), str(tmp_path / "r.fa"), str(tmp_path / "t.bed")
    base = ["-G", g, "-I", str(tmp_path / "idx"), "-O", str(tmp_path / "out.tsv"), "-M", "3"]
    res = _run(*base, "-E", t, "-R", r)                                # two guide sources
    assert res.returncode == 1 and "exactly one of -R" in res.stderr
    res = _run(*base, "-E", t, "-B", t)
    assert res.returncode == 1 and "exactly one of -R" in res.stderr
    res = _run(*base, "-R", r, "-L", str(tmp_path / "l.bed"))          # -L without -E
    assert res.returncode == 1 and "-E" in res.stderr
    for flag, bad in (("-g", "5"), ("-g", "9,3"), ("-g", "0,21"), ("-g", "a,b"), ("-g", "3,4x"), ("-t", "x"), ("-t", "-1"),
                      ("-t", "21"), ("-s", "x"), ("-s", "++"), ("-p", "NG"), ("-p", "G"), ("-p", "GGG"), ("-e", "in"),
                      ("-e", "keep")):
        res = _run(*base, "-E", t, flag, bad)
        assert res.returncode == 1 and flag in res.stderr and bad in res.stderr, (flag, bad, res.stderr)
    for flag, good in (("-g", "8,14"), ("-t", "3"), ("-s", "+"), ("-p", "GG"), ("-e", "overlap")):  # ... belong to -E
        res = _run(*base, "-R", r, flag, good)
        assert res.returncode == 1 and "give -E" in res.stderr, (flag, res.stderr)
    assert _run(*base, "-E", str(tmp_path / "t.txt")).returncode == 1  # wrong extensions
    assert _run(*base, "-E", t, "-L", str(tmp_path / "l.txt")).returncode == 1
    # a well-formed call gets as far as the index, which does not exist: nothing above was about the arguments
    res = _run(*base, "-E", t, "-e", "overlap", "-p", "ga", "-g", "8,14", "-t", "3", "-s", "-", "-L", str(tmp_path / "l.bed"))
    assert res.returncode == 1 and "idx" in res.stderr
    assert not (tmp_path / "out.tsv").exists() and not (tmp_path / "l.bed").exists()
    res = _run("--help")
    assert res.returncode == 0
    for opt in ("-E, --targets", "-e, --target-rule", "-p, --guide-pam", "-g, --gc", "-t, --t-run", "-s, --strands",
                "-L, --list-guides"):
        assert opt in res.stdout, opt


def test_brute_force_agrees_with_hand_worked_windows():
    # 1. both strands at position 0 of a 23-base contig (p + 23 == L)
    w = "CC" + "A" * 19 + "GG"
    got = ec.brute_force([w])
    assert got == [(0, 0, 0, w), (0, 0, 1, "CC" + "T" * 19 + "GG")]
    assert ec.brute_force([w], strands="+") == got[:1] and ec.brute_force([w], strands="-") == got[1:]
    # '+' protospacer CC + 18 A: 2 G/C, no T; '-' protospacer CC + 18 T: 2 G/C, a run of 18 T
    assert ec.brute_force([w], max_t_run=3) == got[:1]
    assert ec.brute_force([w], max_t_run=18) == got
    assert ec.brute_force([w], gc=(2, 2)) == got and ec.brute_force([w], gc=(3, 0)) == [] and ec.brute_force([w], gc=(0, 1)) == []
    # 2. one window short of a contig, an N inside, the separator: nothing
    assert ec.brute_force(["G" * 22]) == [] and ec.brute_force(["G" * 11 + "N" + "G" * 12]) == []
    assert ec.brute_force(["G" * 12, "G" * 12]) == []  # no window crosses a contig end
    assert [x[:3] for x in ec.brute_force(["G" * 24])] == [(0, 0, 0), (0, 1, 0)]
    assert [x[:3] for x in ec.brute_force(["c" * 24, "G" * 23])] == [(0, 0, 1), (0, 1, 1), (1, 0, 0)]  # lower case counts
    # 3. another PAM: TGAG...: '+' needs w[21..23) == "AG", '-' needs w[0..2) == revcomp("AG") == "CT"
    s = "CT" + "ACGTACGTACGTACGTACG" + "AG"
    assert len(s) == 23
    assert ec.brute_force([s], pam="AG") == [(0, 0, 0, s), (0, 0, 1, revcomp(s))]
    assert ec.brute_force([s], pam="ag") == ec.brute_force([s], pam="AG") and ec.brute_force([s]) == []
    # 4. the T run is counted in the protospacer only: TTTT over g[17..21) leaves three T inside it
    assert ec.kept(ec.T_AT_PAM, max_t_run=3) and not ec.kept(ec.T_INSIDE, max_t_run=3) and ec.kept(ec.T_INSIDE, max_t_run=4)
    assert ec.T_AT_PAM[17:21] == "TTTT" and ec.T_AT_PAM[16] != "T" and "TTTT" in ec.T_INSIDE[:20]
    # 5. codes: base i in bits 2 i, 2 i + 1
    codes, loci = ec.arrays(got)
    assert int(codes[0]) == 1 | 1 << 2 | 2 << 42 | 2 << 44 and loci.tobytes() == np.array(
        [(0, 0, 0, 0), (0, 0, 1, 0)], dtype=ec.LOCUS_DTYPE).tobytes()
    assert ec.LOCUS_DTYPE == va.LOCUS_DTYPE


def test_edge_layout_reaches_every_part_of_the_kernel():
    contigs = ec.edge_layout()
    assert [len(c) for c in contigs] == [4200, 4200, 23, 22, 24, 14000, 40]
    cands = ec.brute_force(contigs)
    strand = np.array([x[2] for x in cands])
    pos = ec.global_positions(contigs, cands)
    assert (strand == 0).any() and (strand == 1).any()                        # both strands occur
    both = set(pos[strand == 0].tolist()) & set(pos[strand == 1].tolist())
    assert both                                                              # some position carries both
    assert ((pos % 32) >= 10).any()                                          # windows that cross into the next word
    assert ((pos % ec.TILE) >= ec.TILE - 22).any()                           # ... and into the next tile
    assert len(cands) > 3 * ec.TILE                                          # the scan carries across tiles
    # the first two contigs: every start a candidate, one strand each - every lane's mask is full
    assert [x[:3] for x in cands[:4178]] == [(0, p, 0) for p in range(4178)]
    assert [x[:3] for x in cands[4178:2 * 4178]] == [(1, p, 1) for p in range(4178)]
    assert {x[0] for x in cands} == {0, 1, 2, 5, 6}                            # contigs 3 and 4 hold none
    # the planted T runs of the random contig are candidates
    at = {(c, p, s): g for c, p, s, g in cands}
    for p, guide, s in ec.PLANTS:
        assert at[(ec.RANDOM_AT, p, 0 if s == "+" else 1)] == guide
    # the N run, the IUPAC letter: no window over them; the lower-case stretch: windows as everywhere
    starts = {p for c, p, _, _ in cands if c == ec.RANDOM_AT}
    assert not any(4978 <= p < 5050 for p in starts) and not any(8978 <= p <= 9000 for p in starts)
    assert any(7000 <= p < 7277 for p in starts)
