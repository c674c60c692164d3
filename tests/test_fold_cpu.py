"""The host side of the guide RNA's self-complementarity (vsc_fold_text, the shape, the limits, the tools' argument checks, the
stand-alone check): the library's diagonal form against the definition restated on strings in tests/fold_cases.py, as integers.
No device is needed."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import fold_cases as fc
import varscot_amd as va
from varscot_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.environ.get("VSC_TEST_BIN") or os.path.join(ROOT, "varscot_amd", "bin")
PAIRS = [(name, m) for name, _, lengths in fc.SHAPES for m in lengths]


@pytest.mark.parametrize("name,m", PAIRS, ids=["%s-m%d" % p for p in PAIRS])
def test_fold_text_equals_the_strings(name, m):
    shape, sh, sc = fc.SHAPE_OF[name], fc.va_shape(fc.SHAPE_OF[name]), fc.scaffold(name, m)
    families = set()
    for family, g in fc.cases(name, m):
        families.add(family)
        assert va.fold_text(g, sh, sc) == fc.row(g, sc, shape), (family, g, sc)
    assert families >= {"random", "none"} and len(fc.cases(name, m)) >= 11


def test_the_shapes_and_scaffolds_hold_what_they_are_for():
    shapes = [s for _, s, _ in fc.SHAPES]
    assert fc.SPCAS9 in shapes and fc.CAS12A in shapes
    for name, preset in (("SpCas9", fc.SPCAS9), ("Cas12a", fc.CAS12A)):
        p = va.FOLD_SHAPES[name]
        assert (p.site_len, p.proto_start, p.proto_len, p.stem, p.gc_min, p.min_loop, p.seed_start, p.seed_len, p.flags) == tuple(preset)
    assert sorted(va.FOLD_SHAPES) == ["Cas12a", "SpCas9"]
    assert any(s.proto_len == 12 and s.site_len == 16 for s in shapes) and any(s.proto_len == 32 and s.site_len == 32 for s in shapes)
    assert any(s.proto_start + s.proto_len == s.site_len and s.proto_start for s in shapes)
    assert {3, 8} <= {s.stem for s in shapes}
    assert any(s.gc_min == 0 for s in shapes) and any(s.gc_min == s.stem for s in shapes)
    assert {0, 16} <= {s.min_loop for s in shapes}
    assert any(s.seed_len and s.seed_start == 0 for s in shapes) and any(s.seed_len and s.seed_start + s.seed_len == s.proto_len for s in shapes)
    assert any(s.seed_len == 0 for s in shapes) and {0, 1} == {s.flags for s in shapes}
    lengths = {m for _, _, ms in fc.SHAPES for m in ms}
    assert lengths >= {0, 31, 32, 33, 64, 65, 96, 97, 128}
    for name, s, ms in fc.SHAPES:  # m = k - 1 and m = k at k = 3, 4, 6 and 8
        if name in ("SpCas9", "n12_site16", "n32_site32", "no_seed"):
            assert {s.stem - 1, s.stem} <= set(ms), name


def test_the_families_hold_what_they_are_for():
    seen = {}
    for name, m in PAIRS:
        for family, tags in fc.seen(name, m).items():
            seen.setdefault(family, set()).update(tags)
    assert "starts == 0" in seen["none"] and "starts > 0" in seen["random"]
    assert {"loop == min_loop", "self only"} <= seen["loop_exact"]
    assert "loop == min_loop - 1 does not count" in seen["loop_short"] and "loop == min_loop" not in seen["loop_short"]
    assert "position 0 with n - 1" in seen["end_to_end"]
    assert "self_longest >= k + 2" in seen["long_self"]
    assert "only under WOBBLE" in seen["wobble_only"]
    assert "fails QUAL, lengthens self_longest" in seen["unqualified"]
    assert {"scaffold only", "scaffold position 0", "scaffold position m - k", "across 32", "across 64", "across 96"} <= seen["scaffold"]
    assert "both" in seen["both"]
    assert "seed_paired == seed_len" in seen["seed_full"] and "seed_paired == 0" in seen["none"]
    assert "palindromic" in seen["palindrome"]
    # the planted hairpin one base short of the loop has no stem of k, and its stem of k - 1 is the longest
    for name, m in PAIRS:
        shape, sc = fc.SHAPE_OF[name], fc.scaffold(name, m)
        for family, g in fc.cases(name, m):
            if family == "loop_short" and m == 0:
                f = fc.fields(g, sc, shape)
                assert f["starts"] == 0 and f["self_longest"] == shape.stem - 1, (name, g)


def test_a_full_length_stem_and_bit_31():
    shape = fc.SHAPE_OF["n32_wobble"]._replace(flags=0, min_loop=0)
    sh = fc.va_shape(shape)
    rng = np.random.default_rng(31)
    g = fc.random_seq(rng, 32)
    sc = fc.random_seq(rng, 48) + fc.revcomp(g) + fc.random_seq(rng, 48)
    want = fc.row(g, sc, shape)
    assert va.unpack_fold_row(want)["scaf_longest"] == 32 and va.unpack_fold_row(want)["scaf_starts"] == 28
    assert va.fold_text(g, sh, sc) == want
    pal = g[:16] + fc.revcomp(g[:16])
    want = fc.row(pal, "", shape)
    assert va.unpack_fold_row(want)["self_longest"] == 16 and va.fold_text(pal, sh) == want


def test_shape_and_scaffold_refusals():
    ok = dict(site_len=23, spacer=(0, 20), stem=4, gc_min=2, min_loop=3, seed=(8, 12))
    L = va.lib()
    row = (C.c_uint32 * 2)(7, 7)
    bad = [{"site_len": 15, "spacer": (0, 12)}, {"site_len": 33, "spacer": (0, 20)}, {"spacer": (0, 11)}, {"site_len": 32, "spacer": (0, 33)},
           {"spacer": (4, 20)}, {"stem": 2}, {"stem": 9}, {"gc_min": 5}, {"min_loop": 17}, {"seed": (17, 0)}, {"seed": (0, 17)}, {"seed": (9, 12)},
           {"flags": 2}, {"flags": 3}]
    for kw in bad:  # one per rule of SHAPE: Python raises, and the library refuses the same numbers
        args = dict(ok, **kw)
        with pytest.raises(ValueError):
            va.FoldShape(**args)
        raw = va.FoldShape(validate=False, **args)
        st = raw._struct()
        n = raw.proto_len
        assert L.vsc_fold_text(b"A" * max(n, 0), n, b"", 0, C.byref(st), row) == -22, kw
        assert tuple(row) == (7, 7)  # before anything is written
    for k in range(3):  # a reserved field
        st = va.FoldShape(**ok)._struct()
        st.reserved[k] = 1
        assert L.vsc_fold_text(b"A" * 20, 20, b"", 0, C.byref(st), row) == -22 and tuple(row) == (7, 7)
    for kw in ({"site_len": 16, "spacer": (4, 12), "seed": (0, 12)}, {"site_len": 32, "spacer": (0, 32), "seed": (16, 16), "stem": 8, "gc_min": 8,
               "min_loop": 16}, {"stem": 3, "gc_min": 0, "min_loop": 0, "seed": (0, 0)}, {"wobble": True}):
        st = va.FoldShape(**dict(ok, **kw))._struct()
        assert C.sizeof(st) == 48 and tuple(st.reserved) == (0, 0, 0)
    assert va.FoldShape(wobble=True).flags == va.FOLD_WOBBLE == 1
    st = va.FoldShape(**ok)._struct()
    # SCAFFOLD: more than 128 letters, another letter; a spacer of another length than the shape's; null arguments
    assert L.vsc_fold_text(b"A" * 20, 20, b"A" * 129, 129, C.byref(st), row) == -22
    assert L.vsc_fold_text(b"A" * 20, 20, b"A" * 128, 128, C.byref(st), row) == 0
    row[0] = row[1] = 7
    for letter in b"NRY-*n ":
        assert L.vsc_fold_text(b"A" * 20, 20, b"ACG" + bytes([letter]), 4, C.byref(st), row) == -22 and tuple(row) == (7, 7)
    assert L.vsc_fold_text(b"A" * 20, 19, b"", 0, C.byref(st), row) == -22 and L.vsc_fold_text(b"A" * 19, 20, b"", 0, C.byref(st), row) == -22
    assert L.vsc_fold_text(None, 20, b"", 0, C.byref(st), row) == -22 and L.vsc_fold_text(b"A" * 20, 20, None, 4, C.byref(st), row) == -22
    assert L.vsc_fold_text(b"A" * 20, 20, b"", 0, None, row) == -22 and L.vsc_fold_text(b"A" * 20, 20, b"", 0, C.byref(st), None) == -22
    assert L.vsc_fold_text(b"A" * 20, 20, None, 0, C.byref(st), row) == 0  # no scaffold at all
    for sc in ("A" * 129, "ACGN", "AC-G"):
        with pytest.raises(ValueError):
            va.fold_text("A" * 20, "SpCas9", sc)
    with pytest.raises(ValueError):
        va.fold_text("A" * 19, "SpCas9")
    with pytest.raises(ValueError):
        va.fold_text("A" * 20, "Cas9")
    assert C.sizeof(_lib.FoldStats) == 64 and C.sizeof(_lib.FoldLimits) == 16


def test_text_case_u_and_other_letters():
    rng = np.random.default_rng(4)
    for name, m in (("SpCas9", 76), ("n32_wobble", 65)):
        shape, sh, sc = fc.SHAPE_OF[name], fc.va_shape(fc.SHAPE_OF[name]), fc.letters(fc.scaffold(name, m))
        g = next(g for _, g in fc.cases(name, m) if fc.fields(g, sc, shape)["starts"] and "T" in g)
        want = fc.row(g, sc, shape)
        assert va.fold_text(g.lower(), sh, sc.lower()) == want
        assert va.fold_text(g.replace("T", "U"), sh, sc.replace("T", "u")) == want
        assert va.fold_text(g.encode(), sh, sc.encode()) == want
        for ch in "NnRY-*":
            at = int(rng.integers(0, len(g)))
            assert va.fold_text(g[:at] + ch + g[at + 1:], sh, sc) == (va.FOLD_UNDEFINED, va.FOLD_UNDEFINED)
    assert va.FOLD_UNDEFINED == va.FOLD_NO_LIMIT == 0xFFFFFFFF


def test_unpack_fold_row_round_trips():
    rows, want = [], []
    for name, m in (("SpCas9", 76), ("n32_site32", 128), ("seed_5prime", 65)):
        shape, sc = fc.SHAPE_OF[name], fc.scaffold(name, m)
        for _, g in fc.cases(name, m):
            rows.append(fc.row(g, sc, shape))
            want.append(fc.fields(g, sc, shape))
    rows.append((fc.UNDEF, fc.UNDEF))
    a = np.array(rows, dtype=np.uint32)
    u = va.unpack_fold_row(a)
    assert u["defined"][:-1].all() and not u["defined"][-1]
    for k in ("starts", "self_starts", "scaf_starts", "seed_paired", "self_longest", "scaf_longest"):
        assert u[k][:-1].tolist() == [w[k] for w in want] and u[k][-1] == 0, k
    assert len({tuple(r) for r in rows}) > 20
    for r, w in zip(rows[:-1], want):
        one = va.unpack_fold_row(r)
        assert one.pop("defined") is True and one == w and va.pack_fold_row(**one) == tuple(r)
    assert va.unpack_fold_row((fc.UNDEF, fc.UNDEF))["defined"] is False
    # the pick column: fewer stems are better, the undefined row is the worst
    col = va.pick_column("fold", a)
    assert col.dtype == np.uint64 and col[:-1].tolist() == [32 - w["starts"] for w in want] and col[-1] == 0 and va.PICK_COLUMNS["fold"] == 6


def test_python_limits_become_integers_once():
    f = va.Genome._fold_args
    shape = va.FOLD_SHAPES["SpCas9"]
    none = (None,) * 4
    assert f(None, None, *none, 23) is None
    assert f(shape, None, *none, 23) == (shape, b"", None) and f("SpCas9", "ACGU", *none, 23) == (shape, b"ACGU", None)
    assert f(shape, None, 3, None, None, None, 23)[2] == (3, fc.NO_LIMIT, fc.NO_LIMIT, fc.NO_LIMIT)
    assert f(shape, b"acgu", 0, 32, np.int64(5), 4.0, 23) == (shape, b"acgu", (0, 32, 5, 4))
    for bad in ((None, "ACGT") + none, (None, None, 3, None, None, None), (None, None, None, None, None, 0), (shape, None, 33, None, None, None),
                (shape, None, -1, None, None, None), (shape, None, None, 2.5, None, None), (shape, "ACGN") + none, (shape, "A" * 129) + none,
                ("x", None) + none, (7, None) + none):
        with pytest.raises(ValueError):
            f(*bad, 23)
    with pytest.raises(ValueError):
        f("Cas12a", None, *none, 23)  # site_len 27 is not these candidates'
    assert f("Cas12a", None, *none, 27)[0] is va.FOLD_SHAPES["Cas12a"]


def test_the_stand_alone_check_builds_and_runs_clean(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "fold_check")
    build = subprocess.run([hipcc, "--offload-arch=gfx950", "-x", "hip", "-O1", "-g", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                            "-I" + os.path.join(ROOT, "varscot_amd", "csrc"), "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                            "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tools", "fold_check.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and run.stdout.startswith("ok: ") and "runtime error" not in run.stderr and "ERROR" not in run.stderr, \
        (run.returncode, run.stdout, run.stderr)


def _run(tool, *args):
    return subprocess.run([os.path.join(BIN, tool)] + [str(a) for a in args], capture_output=True, text=True, timeout=120,
                          env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))


def test_the_tools_refuse_before_a_device_is_opened(tmp_path):
    (tmp_path / "long.txt").write_text("ACGU\n" * 33)
    (tmp_path / "bad.txt").write_text("ACGU\nACGN\n")
    gs = ("guide_summary", "-G", tmp_path / "g.fa", "-I", tmp_path / "idx", "-M", "2", "-O", tmp_path / "o.tsv")
    ps = ("pattern_search", "-i", tmp_path / "idx", "-q", "TTTV" + "N" * 23, "-M", "2", "-O", tmp_path / "o.tsv")
    e_gs, e_ps = ("-E", tmp_path / "t.bed"), ("-E", tmp_path / "e.tsv", "-p", "4,23")
    cases = [
        ((*gs, *e_gs, "--fold-scaffold", "ACGU"), "give --fold"), ((*gs, *e_gs, "--max-fold", "3"), "give --fold"),
        ((*gs, "-R", tmp_path / "r.fa", "--fold", "SpCas9"), "give -E"), ((*gs, *e_gs, "--fold", "SpCas9", "-D", "0,1"), "one device"),
        ((*gs, *e_gs, "--fold", "Cas12a"), "preset for sites of 27"), ((*gs, *e_gs, "--fold", "23,0,20,2,2,3,8,12,0"), "--fold takes"),
        ((*gs, *e_gs, "--fold", "27,4,23,4,2,3,0,6,0"), "--fold takes"), ((*gs, *e_gs, "--fold", "23,0,20,4,2,3,8,12"), "--fold takes"),
        ((*gs, *e_gs, "--fold", "23,0,20,4,2,3,8,12,2"), "--fold takes"), ((*gs, *e_gs, "--fold", "23,0,20,4,2,3,9,12,0"), "--fold takes"),
        ((*gs, *e_gs, "--fold", "SpCas9", "--fold-scaffold", "A" * 129), "at most 128"),
        ((*gs, *e_gs, "--fold", "SpCas9", "--fold-scaffold", "ACGN"), "A C G T U"),
        ((*gs, *e_gs, "--fold", "SpCas9", "--fold-scaffold", "@%s" % (tmp_path / "long.txt")), "at most 128"),
        ((*gs, *e_gs, "--fold", "SpCas9", "--fold-scaffold", "@%s" % (tmp_path / "bad.txt")), "A C G T U"),
        ((*gs, *e_gs, "--fold", "SpCas9", "--fold-scaffold", "@%s" % (tmp_path / "none.txt")), "cannot read"),
        ((*gs, *e_gs, "--fold", "SpCas9", "--max-fold", "33"), "--max-fold takes"), ((*gs, *e_gs, "--fold", "SpCas9", "--max-fold", "1,2,3,4,5"), "--max-fold takes"),
        ((*gs, *e_gs, "--fold", "SpCas9", "--max-fold", "1,x"), "--max-fold takes"),
        ((*ps, *e_ps, "--fold-scaffold", "ACGU"), "give --fold"), ((*ps, *e_ps, "--max-fold", "3"), "give --fold"),
        ((*ps, "-R", tmp_path / "g.fa", "--fold", "Cas12a"), "give -E"), ((*ps, *e_ps, "--fold", "Cas12a", "-D", "0,1"), "one device"),
        ((*ps, *e_ps, "--fold", "SpCas9"), "preset for sites of 23"), ((*ps, *e_ps, "--fold", "23,0,20,4,2,3,8,12,0"), "--fold takes"),
        ((*ps, *e_ps, "--fold", "27,4,24,4,2,3,0,6,0"), "--fold takes"), ((*ps, *e_ps, "--fold", "Cas12a", "--fold-scaffold", "A" * 129), "at most 128"),
        ((*ps, *e_ps, "--fold", "Cas12a", "--fold-scaffold", "AC GU"), "A C G T U"), ((*ps, *e_ps, "--fold", "Cas12a", "--max-fold", "-1"), "--max-fold takes"),
    ]
    for args, text in cases:
        r = _run(*args)
        assert r.returncode == 1 and text in r.stderr and "ERROR" not in r.stderr, (args, r.stderr)
    for tool in ("guide_summary", "pattern_search"):
        r = _run(tool, "--help")
        assert r.returncode == 0 and all(o in r.stdout for o in ("--fold", "--fold-scaffold", "--max-fold"))
