"""Restriction sites and IUPAC motifs without a device: vsc_motif_text - the function the kernels call, on the host - bit for
bit against the definition restated on strings (tests/motif_cases.py), the refusals, the Python surface, the tools' refusals
and the stand-alone check under the host sanitizers."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import motif_cases as mc
import varscot_amd as va
from helpers import random_seq
from varscot_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "varscot_amd", "bin")


def text_row(x, name, entries, flanks="none", left=None, right=None):
    lf, rf = mc.FLANKS[flanks]
    return va.motif_text(x, mc.va_shape(mc.SHAPE_OF[name]), va.motifs(entries), left=lf if left is None else left, right=rf if right is None else right)


def test_the_planted_families_show_what_they_are_for():
    seen = set()
    for name in mc.SHAPE_OF:
        for flanks in mc.FLANKS:
            for family, x, lf, rf, entries, holds in mc.planted(name, flanks):
                want = mc.row(x, lf, rf, entries, mc.SHAPE_OF[name])
                assert holds(want), (name, flanks, family, want)
                assert text_row(x, name, entries, left=lf, right=rf) == want, (name, flanks, family)
                seen.add(family)
    assert seen >= {"x_q0", "x_qlast", "y_q0", "y_qlast", "left_junction", "right_junction", "spacer_alone", "ends_at_z0", "reaches_z0",
                    "starts_at_z1", "starts_in_z1", "cut_and_elsewhere", "bit62", "rc_with_flag", "rc_without_flag", "palindrome", "sixteen"}
    # the presets are the shapes the cases walk
    for name in ("SpCas9", "Cas12a"):
        s, v = mc.SHAPE_OF[name], va.MOTIF_SHAPES[name]
        assert (v.up, v.site_len, v.down, v.proto_start, v.proto_len, v.cut_start, v.cut_len) == tuple(s)


@pytest.mark.parametrize("name", sorted(mc.SHAPE_OF))
def test_random_contexts_against_the_strings(name):
    rng = np.random.default_rng([36, len(name)])
    shape = mc.SHAPE_OF[name]
    C_len = mc.context_len(shape)
    hit = np.zeros(3, dtype=np.int64)
    for set_name, entries in list(mc.MOTIF_SETS.items()) + [("full", mc.full_set())]:
        for flanks in mc.FLANKS:
            lf, rf = mc.FLANKS[flanks]
            for _ in range(6 if set_name == "full" else 25):
                x = random_seq(rng, C_len)
                want = mc.row(x, lf, rf, entries, shape)
                assert text_row(x, name, entries, flanks) == want, (set_name, flanks, x)
                assert all(v >> len(entries) == 0 for v in want)
                hit += [v != 0 for v in want]
    assert hit.min() > 20  # every mask is met set many times
    # a two-letter alphabet: many occurrences at once
    x = random_seq(rng, C_len).translate(str.maketrans("GT", "AC"))
    assert text_row(x, name, mc.full_set(), "both16") == mc.row(x, *mc.FLANKS["both16"], mc.full_set(), shape)


def test_set_sizes_lengths_and_letters():
    full = mc.full_set()
    assert len(full) == 63 and {len(e[1]) for e in full} >= {2, 16} and len(mc.MOTIF_SETS["one"]) == 1
    assert set("".join(e[1].upper() for e in full)) >= set("ACGURYSWKMBDHVN") | {"T"}
    # a motif longer than the construct: no occurrence, not refused; on a context of its own length: one start
    s = mc.SHAPE_OF["n12_site16"]
    long16 = "ACGTCCGGACGTACGT"
    x = "A" * 3 + long16 + "A" * 5
    assert text_row(x, "n12_site16", [("long", long16, False)]) == (0, 1, 0) == mc.row(x, "", "", [("long", long16, False)], s)
    assert text_row(long16, "zone_last", [("long", long16, False)]) == (1, 1, 0)
    assert text_row("C" + long16[1:], "zone_last", [("long", long16, False)]) == (0, 0, 0)
    # the reverse complement of an IUPAC text, letter by letter
    assert mc.iupac_revcomp("GAATTC") == "GAATTC" and mc.iupac_revcomp("ACGTRYSWKMBDHVN") == "NBDHVKMWSRYACGT"
    x = "A" * 20 + "GTC" + "A" * 32  # GTB is what VAC reads on the other strand
    assert text_row(x, "SpCas9", [("v", "VAC", True)]) == mc.row(x, "", "", [("v", "VAC", True)], mc.SHAPE_OF["SpCas9"]) != (0, 0, 0)
    assert text_row(x, "SpCas9", [("v", "VAC", False)]) == (0, 0, 0)


def test_text_case_u_and_other_letters():
    rng = np.random.default_rng(5)
    shape, sh = mc.SHAPE_OF["SpCas9"], mc.va_shape(mc.SHAPE_OF["SpCas9"])
    x = mc.put(random_seq(rng, 55), 20, mc.P)
    entries = mc.CLONING
    want = mc.row(x, "CACCG", "GTTT", entries, shape)
    assert want[0] & 1
    lower = va.motifs([(n, t.lower()) for n, t in entries])
    assert va.motif_text(x.lower(), sh, lower, left="caccg", right="gttt") == want
    assert va.motif_text(x.replace("T", "U"), sh, va.motifs([(n, t.replace("T", "u")) for n, t in entries]), left="CACCG", right="GUUU") == want
    assert va.motif_text(x.encode(), sh, entries, left=b"CACCG", right=b"GTTT") == want
    for ch in "NnRY-*":
        at = int(rng.integers(0, len(x)))
        assert va.motif_text(x[:at] + ch + x[at + 1:], sh, entries) == (va.MOTIF_UNDEFINED,) * 3
    assert va.MOTIF_UNDEFINED == 0xFFFFFFFFFFFFFFFF and va.MOTIF_BOTH_STRANDS == 1 and va.MOTIF_CUT_ONLY == 1


def raw_text(context, shape_fields, motifs, left=b"", right=b"", reserved=None, n_motifs=None, a=None, b=None):
    """vsc_motif_text with nothing checked in Python: the library's code."""
    sh = _lib.MotifShapeStruct(*shape_fields)
    for i, v in enumerate(reserved or ()):
        sh.reserved[i] = v
    arr = (_lib.MotifStruct * max(len(motifs or ()), 1))()
    for i, (text, length, flags) in enumerate(motifs or ()):
        arr[i].text, arr[i].len, arr[i].flags = text[:16], length, flags
    row = (C.c_uint64 * 3)(7, 7, 7)
    code = va.lib().vsc_motif_text(context, len(context) if context is not None else 0, left, len(left) if a is None else a, right,
                                   len(right) if b is None else b, arr if motifs is not None else None, len(motifs or ()) if n_motifs is None else n_motifs,
                                   C.byref(sh), row)
    return code, tuple(row)


def test_one_refusal_per_rule():
    ok_shape, x = (0, 23, 0, 0, 20, 16, 2), b"A" * 23
    one = [(b"CGTCTC", 6, 1)]
    assert raw_text(x, ok_shape, one) == (0, (0, 0, 0))
    bad_shapes = [(0, 15, 0, 0, 12, 0, 1), (0, 33, 0, 0, 20, 16, 2), (17, 23, 0, 0, 20, 16, 2), (0, 23, 17, 0, 20, 16, 2), (16, 32, 16, 0, 33, 0, 1),
                  (0, 23, 0, 0, 11, 16, 2), (0, 23, 0, 4, 20, 16, 2), (0, 23, 0, 0, 20, 16, 0), (0, 23, 0, 0, 20, 16, 17), (0, 23, 0, 0, 20, 22, 2)]
    for s in bad_shapes:
        ctx_len = s[0] + s[1] + s[2]
        code, row = raw_text(b"A" * ctx_len, s, one)
        assert code != 0 and row == (7, 7, 7), s
    refusals = [
        raw_text(x, ok_shape, one, reserved=(0, 0, 0, 0, 1)), raw_text(x, ok_shape, one, reserved=(1,)),
        raw_text(x, ok_shape, one, left=b"ACGN"), raw_text(x, ok_shape, one, right=b"AC-T"), raw_text(x, ok_shape, one, left=b"A" * 17),
        raw_text(x, ok_shape, one, right=b"A" * 17), raw_text(x, ok_shape, one, left=None, a=3),
        raw_text(x, ok_shape, [(b"CGTXTC", 6, 0)]), raw_text(x, ok_shape, [(b"NNNN", 4, 0)]), raw_text(x, ok_shape, [(b"A", 1, 0)]),
        raw_text(x, ok_shape, [(b"A" * 16, 17, 0)]), raw_text(x, ok_shape, [(b"ACGT", 4, 2)]), raw_text(x, ok_shape, [(b"ACGT", 4, 0x80000001)]),
        raw_text(x, ok_shape, [], n_motifs=0), raw_text(x, ok_shape, one * 64), raw_text(x, ok_shape, None, n_motifs=1),
        raw_text(x[:22], ok_shape, one), raw_text(x + b"A", ok_shape, one), raw_text(None, ok_shape, one),
    ]
    for code, row in refusals:
        assert code != 0 and row == (7, 7, 7)  # refused before anything is written
    assert raw_text(x, ok_shape, one * 63)[0] == 0 and raw_text(x, ok_shape, [(b"ACGTACGTACGTACGT", 16, 1)])[0] == 0
    assert raw_text(b"A" * 64, (16, 32, 16, 0, 32, 16, 16), one)[0] == 0


def test_struct_sizes_and_the_python_checks():
    assert C.sizeof(_lib.MotifStruct) == 24 and C.sizeof(_lib.MotifShapeStruct) == 48 and C.sizeof(_lib.MotifLimits) == 32
    assert C.sizeof(_lib.MotifStats) == 96
    for bad in (dict(site_len=15), dict(site_len=33), dict(up=17), dict(down=17), dict(site_len=32, up=16, down=16, spacer=(0, 33)),
                dict(spacer=(0, 11)), dict(spacer=(4, 20)), dict(cut=(16, 0)), dict(cut=(16, 17)), dict(cut=(22, 2))):
        with pytest.raises(ValueError):
            va.MotifShape(**bad)
    assert va.MotifShape(32, (0, 32), (16, 16), 16, 16).context_len == 64
    for bad in ([], [("a", "A")], [("a", "A" * 17)], [("a", "NNN")], [("a", "ACGX")], [("a", "ACGT"), ("a", "CCGG")], [("a", "ACGT", True, 1)],
                [("m%d" % i, "ACGT") for i in range(64)]):
        with pytest.raises(ValueError):
            va.motifs(bad)
    with pytest.raises(ValueError):
        va.motif_text("A" * 22, va.MotifShape(), mc.CLONING)
    with pytest.raises(ValueError):
        va.motif_text("A" * 23, va.MotifShape(), mc.CLONING, left="A" * 17)
    with pytest.raises(ValueError):
        va.motif_text("A" * 23, "Cas9", mc.CLONING)
    ms = va.motifs(mc.CLONING)
    assert ms.names == ["BsmBI", "BbsI", "BsaI"] and ms.both == [True] * 3 and len(ms) == 3
    assert ms.mask(None) == 0 and ms.mask("BbsI") == 2 and ms.mask(["BsmBI", "BsaI"]) == 5 and ms.mask(7) == 7 and ms.mask(np.uint64(4)) == 4
    for bad in (8, -1, "EcoRI", ["BsmBI", "x"]):
        with pytest.raises(ValueError):
            ms.mask(bad)


def test_limits_and_the_truth_table():
    table = mc.truth_table()
    assert len(table) == 48 and {w for _, _, w in table} == {True, False}
    for r, lim, want in table:
        assert mc.keep(r, lim) == want, (r, lim)
    assert not mc.keep((mc.UNDEF,) * 3, mc.Limits(0, 0, 0, False)) and not mc.keep(None, mc.Limits(0, 0, 0, False))
    f = va.Genome._motif_args
    shape, ms = va.MOTIF_SHAPES["SpCas9"], va.motifs(mc.CLONING)
    none = (None,) * 6
    assert f(None, None, *none, 23) is None
    assert f(shape, ms, *none, 23) == (shape, ms, b"", b"", None) and f("SpCas9", ms, "CACCG", b"GUUU", None, None, None, None, 23)[2:4] == (b"CACCG", b"GUUU")
    assert f(shape, ms, None, None, "BsmBI", None, None, None, 23)[4] == (1, 0, 0, 0)
    assert f(shape, ms, None, None, ["BsmBI", "BsaI"], 2, "BbsI", True, 23)[4] == (5, 2, 2, 1)
    assert f(shape, mc.CLONING, None, None, None, None, 7, False, 23)[4] == (0, 0, 7, 0)
    for bad in ((None, ms) + none, (None, None, "ACGT") + none[1:], (None, None, None, None, 1, None, None, None), (None,) * 7 + (True,),
                (shape, None) + none, (shape, ms, "ACGN") + none[1:], (shape, ms, None, "A" * 17) + none[2:], (shape, ms, None, None, 8, None, None, None),
                (shape, ms, None, None, "EcoRI", None, None, None), (shape, ms, None, None, None, None, None, True), ("x", ms) + none, (7, ms) + none):
        with pytest.raises(ValueError):
            f(*bad, 23)
    with pytest.raises(ValueError):
        f("Cas12a", ms, *none, 23)  # site_len 27 is not these candidates'
    assert f("Cas12a", ms, *none, 27)[0] is va.MOTIF_SHAPES["Cas12a"]


def test_unpack_motif_row_and_the_rflp_column():
    ms = va.motifs(mc.CLONING)
    rows = np.array([(1, 2, 4), (0, 7, 5), (0, 0, 0), (mc.UNDEF,) * 3, (0, (1 << 63) - 1, 0)], dtype=np.uint64)
    u = va.unpack_motif_row(rows, ms)
    assert u["defined"].tolist() == [True, True, True, False, True]
    assert u["construct"].tolist() == [1, 0, 0, 0, 0] and u["cut"].tolist()[:4] == [2, 7, 0, 0] and u["elsewhere"].tolist() == [4, 5, 0, 0, 0]
    assert u["cut_only"].tolist()[:4] == [2, 2, 0, 0]
    assert u["cut_names"][:2] == [["BbsI"], ["BsmBI", "BbsI", "BsaI"]] and u["cut_only_names"][1] == ["BbsI"] and u["construct_names"][3] == []
    one = va.unpack_motif_row((1, 2, 4), ms)
    assert one == {"construct": 1, "cut": 2, "elsewhere": 4, "cut_only": 2, "defined": True, "construct_names": ["BsmBI"], "cut_names": ["BbsI"],
                   "elsewhere_names": ["BsaI"], "cut_only_names": ["BbsI"]}
    assert va.unpack_motif_row((mc.UNDEF,) * 3)["defined"] is False
    col = va.pick_column("rflp", rows)
    assert col.dtype == np.uint64 and col.tolist() == [1, 1, 0, 0, 63] and va.PICK_COLUMNS["rflp"] == 6
    assert mc.totals_of(rows, 3).tolist() == [[1, 2, 1], [0, 3, 3], [0, 2, 1]]


def test_the_stand_alone_check_builds_and_runs_clean(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "motif_check")
    build = subprocess.run([hipcc, "--offload-arch=gfx950", "-x", "hip", "-O1", "-g", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                            "-I" + os.path.join(ROOT, "varscot_amd", "csrc"), "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                            "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tools", "motif_check.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and run.stdout.startswith("ok: ") and "runtime error" not in run.stderr and "ERROR" not in run.stderr, \
        (run.returncode, run.stdout, run.stderr)


def _run(tool, *args):
    return subprocess.run([os.path.join(BIN, tool)] + [str(a) for a in args], capture_output=True, text=True, timeout=120,
                          env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))


def test_the_tools_refuse_before_a_device_is_opened(tmp_path):
    good = tmp_path / "m.tsv"
    good.write_text("#name\ttext\tstrands\nBsmBI\tCGTCTC\t2\nBbsI\tGAAGAC\t1\n")
    files = {"cols": "BsmBI\tCGTCTC\n", "strands": "BsmBI\tCGTCTC\t3\n", "letter": "BsmBI\tCGTXTC\t2\n", "short": "a\tA\t1\n", "long": "a\t%s\t1\n" % ("A" * 17),
             "alln": "a\tNNNN\t1\n", "twice": "a\tACGT\t1\na\tCCGG\t1\n", "empty": "# nothing\n", "many": "".join("m%d\tACGT\t1\n" % i for i in range(64))}
    for k, v in files.items():
        (tmp_path / (k + ".tsv")).write_text(v)
    gs = ("guide_summary", "-G", tmp_path / "g.fa", "-I", tmp_path / "idx", "-M", "2", "-O", tmp_path / "o.tsv")
    ps = ("pattern_search", "-i", tmp_path / "idx", "-q", "TTTV" + "N" * 23, "-M", "2", "-O", tmp_path / "o.tsv")
    e_gs, e_ps = ("-E", tmp_path / "t.bed"), ("-E", tmp_path / "e.tsv", "-p", "4,23")
    cases = []
    for tool, e in ((gs, e_gs), (ps, e_ps)):
        m = (*tool, *e, "--motifs", good)
        cases += [
            ((*tool, *e, "--motif-left", "ACGT"), "give --motifs"), ((*tool, *e, "--motif-forbid", "BsmBI"), "give --motifs"),
            ((*tool, *e, "--motifs-out", tmp_path / "x.tsv"), "give --motifs"), ((*tool, *e, "--motif-cut-only"), "give --motifs"),
            ((*tool, "-R", tmp_path / "g.fa", "--motifs", good), "give -E"), ((*m, "-D", "0,1"), "one device"),
            ((*tool, *e, "--motifs", tmp_path / "none.tsv"), "cannot read"), ((*tool, *e, "--motifs", tmp_path / "cols.tsv"), "a line is"),
            ((*tool, *e, "--motifs", tmp_path / "strands.tsv"), "a line is"), ((*tool, *e, "--motifs", tmp_path / "letter.tsv"), "IUPAC letters"),
            ((*tool, *e, "--motifs", tmp_path / "short.tsv"), "2 .. 16 letters"), ((*tool, *e, "--motifs", tmp_path / "long.tsv"), "2 .. 16 letters"),
            ((*tool, *e, "--motifs", tmp_path / "alln.tsv"), "N alone"), ((*tool, *e, "--motifs", tmp_path / "twice.tsv"), "occurs twice"),
            ((*tool, *e, "--motifs", tmp_path / "empty.tsv"), "holds no motif"), ((*tool, *e, "--motifs", tmp_path / "many.tsv"), "at most 63"),
            ((*m, "--motif-left", "A" * 17), "at most 16"), ((*m, "--motif-right", "ACGN"), "A C G T U"),
            ((*m, "--motif-forbid", "EcoRI"), "is no motif"), ((*m, "--motif-forbid-context", "BsmBI,x"), "is no motif"),
            ((*m, "--motif-require-cut", ","), "is no motif"), ((*m, "--motif-cut-only"), "belongs to --motif-require-cut"),
        ]
    cases.append(((*ps[:4], "N" * 20 + "GG", *ps[5:], "-E", tmp_path / "e.tsv", "-p", "0,20", "--motifs", good), "sites of 23 (SpCas9) and 27"))
    for args, text in cases:
        r = _run(*args)
        assert r.returncode == 1 and text in r.stderr and "ERROR" not in r.stderr, (args, r.stderr)
    for tool in ("guide_summary", "pattern_search"):
        r = _run(tool, "--help")
        assert r.returncode == 0 and all(o in r.stdout for o in ("--motifs", "--motif-left", "--motif-right", "--motif-forbid", "--motif-forbid-context",
                                                                 "--motif-require-cut", "--motif-cut-only", "--motifs-out"))
