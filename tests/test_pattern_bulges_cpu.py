"""Bulges under a pattern, the host side, no device needed: vsc_pattern_bulge_align - the functions the kernels run - against
the definition restated in tests/pattern_bulge_cases.py over every length, protospacers at either end and inside, every class,
every split point; hand-worked SaCas9 and Cas12a sites; the IUPAC table; equality with vsc_bulge_align where the definitions
coincide; every refusal; the new struct as a C compiler sees it; the ABI version; and pattern_search's -u / -U argument checks
(all made before a device is opened)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import varscot_amd as va
from varscot_amd import _lib
import bulges_cases as bc
import pattern_bulge_cases as pb
from pattern_cases import IUPAC, rnd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.environ.get("VSC_TEST_BIN") or os.path.join(ROOT, "varscot_amd", "bin")
NEW = ["vsc_search_pattern_bulges", "vsc_pattern_bulge_align"]


def test_new_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "varscot_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    bound = {name for name, _, _ in _lib.SYMBOLS}
    L = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in bound and hasattr(L, name), name
    assert int(re.search(r"#define\s+VSC_ABI_VERSION\s+(\d+)", text).group(1)) == 5  # additive: the version stays
    assert va.lib().vsc_abi_version() == 5
    assert not any(name.startswith("vsc_multi") and "pattern_bulge" in name for name in bound)


def protospacers(L):
    """(a, n): a = 0 (PAM at the 3' end), e = L (PAM at the 5' end), PAM at both ends, the whole pattern, the shortest."""
    return [(0, L - 3), (4, L - 4), (3, L - 6), (0, L), (2, 4), (L - 4, 4)]


def classes_of(L):
    return [d for d in pb.CLASSES if 16 <= L + d <= 32]


def test_align_equals_the_definition_at_every_split_point():
    rng = np.random.default_rng(6)
    checked = ties = degenerate = 0
    for L in range(16, 33):
        for proto in protospacers(L):
            a, e = proto[0], proto[0] + proto[1]
            pattern = "".join("N" if a <= j < e else "ACGTRYSWKMBDHVN"[int(rng.integers(15))] for j in range(L))
            for d in classes_of(L):
                assert not pb.refused(pattern, proto, max(d, 0), max(-d, 0))
                for kind in range(3):
                    guide = pb.distinct_guide(rng, pattern, proto)
                    if kind == 1:  # a spelled PAM and degenerate letters in the protospacer
                        guide = "".join("ACGTRYSWKMBDHVN"[int(rng.integers(15))] if (not a <= j < e or rng.integers(4) == 0) else ch
                                        for j, ch in enumerate(guide))
                        degenerate += 1
                    for i in pb.indices(proto, d):
                        free = [j for j in range(a, e) if (j < i - 2 or j > i + 3) and guide[j] != "N"]
                        subs = rng.choice(free, size=min(len(free), int(rng.integers(0, 4))), replace=False) if free else ()
                        s = pb.plant(rng, pattern, guide, proto, d, i, subs)
                        if kind == 2:  # a repeat at the bulge: ties
                            s = s[:i] + s[i - 1] + s[i + 1:]
                        assert pb.fits(pattern, proto, s, d)
                        nm, index, tie = pb.best(guide, s, proto, d)
                        assert va.pattern_bulge_align(pattern, guide, s, proto, d) == (True, nm, index), (L, proto, d, i, guide, s)
                        checked += 1
                        ties += tie
                    s = rnd(rng, L + d)  # a random site: whatever the pattern says of it, NM and the index are the definition's
                    hit, nm, index = va.pattern_bulge_align(pattern, guide, s, proto, d)
                    assert hit == pb.fits(pattern, proto, s, d)
                    assert (nm, index) == (pb.best(guide, s, proto, d)[:2] if hit else (0, 0))
    assert checked > 10000 and ties > 500 and degenerate > 100


def test_hand_worked_sites():
    # SaCas9: 21 + NNGRRT, protospacer (0, 21)
    pattern, proto = pb.PRESETS["SaCas9"]
    guide = "GATTACAGATTACAGATTACA" + "NNNNNN"
    pam = "CTGAGT"
    # a DNA bulge of one base, the C in front of guide position 10; the T on either side differs from it
    assert va.pattern_bulge_align(pattern, guide, "GATTACAGAT" + "C" + "TACAGATTACA" + pam, proto, 1) == (True, 0, 10)
    # the same with one substitution at position 2: NM 1
    assert va.pattern_bulge_align(pattern, guide, "GAATACAGAT" + "C" + "TACAGATTACA" + pam, proto, 1) == (True, 1, 10)
    # an inserted T beside the guide's TT at 9, 10: split points 9, 10 and 11 pair alike, the smallest is reported
    assert va.pattern_bulge_align(pattern, guide, "GATTACAGATT" + "T" + "ACAGATTACA" + pam, proto, 1)[1:] == (0, 9)
    # an RNA bulge of two: the site lacks the guide's C A at 5, 6 - or, read the other way, its A C at 4, 5: the smaller is reported
    assert va.pattern_bulge_align(pattern, guide, "GATTA" + "GATTACAGATTACA" + pam, proto, -2) == (True, 0, 4)
    # the PAM is read behind the bulge: with d = +1 the G of NNGRRT is site letter 24, not 23
    assert va.pattern_bulge_align(pattern, guide, "GATTACAGAT" + "C" + "TACAGATTACA" + "CTTAGT", proto, 1)[0] is False
    assert va.pattern_bulge_align(pattern, guide, "GATTACAGAT" + "C" + "TACAGATTACA" + "CTGAGC", proto, 1)[0] is False
    # a spelled PAM counts: CTGAGT against the guide's AAGAAT = three mismatches (C/A, T/A, G/A), paired behind the bulge
    spelled = guide[:21] + "AAGAAT"
    assert va.pattern_bulge_align(pattern, spelled, "GATTACAGAT" + "C" + "TACAGATTACA" + pam, proto, 1) == (True, 3, 10)
    # Cas12a: TTTV + 23, protospacer (4, 23): the split points run over 5 .. 26
    pattern, proto = pb.PRESETS["Cas12a"]
    guide = "NNNN" + "GATTACAGATTACAGATTACAGA"
    assert va.pattern_bulge_align(pattern, guide, "TTTC" + "G" + "CC" + "ATTACAGATTACAGATTACAGA", proto, 2) == (True, 0, 5)   # the smallest
    assert va.pattern_bulge_align(pattern, guide, "TTTC" + "GATTACAGATTACAGATTACAG" + "C" + "A", proto, 1) == (True, 0, 26)    # the largest
    assert va.pattern_bulge_align(pattern, guide, "TTTC" + "GATTACAGATTACAGATTAC" + "A", proto, -2) == (True, 0, 24)          # RNA: 5 .. 24
    assert va.pattern_bulge_align(pattern, guide, "TTTT" + "G" + "CC" + "ATTACAGATTACAGATTACAGA", proto, 2)[0] is False      # V excludes T
    # a non-ACGT site letter: no hit, nothing else reported
    assert va.pattern_bulge_align(pattern, guide, "TTTC" + "GNCC" + "TTACAGATTACAGATTACAGA", proto, 2) == (False, 0, 0)


def test_iupac_guide_letters_over_the_table():
    pattern, proto = "N" * 20, (0, 20)
    base = "ACGTACGTACGTACGTACGT"
    for letter, allowed in IUPAC.items():
        for b in "ACGT":
            for j, d in ((0, 1), (7, 1), (19, 1), (0, -1), (12, -2), (19, -2)):
                guide = base[:j] + letter + base[j + 1:]
                # the site pairs with `base` at split point 10 but for position j, which holds b
                paired = base[:j] + b + base[j + 1:]
                s = paired[:10] + ("T" * d if d > 0 else "") + paired[10 - min(d, 0):]
                for text in (guide, guide.lower()):
                    hit, nm, index = va.pattern_bulge_align(pattern, text, s, proto, d)
                    assert hit and (nm, index) == pb.best(guide, s, proto, d)[:2]
                    if d > 0 or not 10 <= j < 10 - d:
                        assert nm <= (b not in allowed)
                        assert pb.nm_at(guide, s, proto, d, 10) == (b not in allowed)


def test_equals_bulge_align_where_the_definitions_coincide():
    rng = np.random.default_rng(8)
    pattern, proto = "N" * 21 + "GR", (0, 20)
    for d in bc.CLASSES:
        for i in range(1, bc.max_index(d) + 1):
            for _ in range(6):
                read = rnd(rng, 20) + rnd(rng, 1) + "G" + "AG"[int(rng.integers(2))]
                s = bc.plant(rng, read, d, i, rng.choice(20, size=int(rng.integers(0, 4)), replace=False))
                hit, nm, index = va.pattern_bulge_align(pattern, read, s, proto, d)
                assert hit == (s[-2] == "G" and s[-1] in "AG")
                if hit:
                    assert (nm, index) == va.bulge_align(read, s, d)


def test_refusals():
    sa, proto = pb.PRESETS["SaCas9"]
    guide, site = "A" * 21 + "N" * 6, lambda L, d: "A" * (L + d)
    ok = lambda *a: va.lib().vsc_pattern_bulge_align(*[x.encode() if isinstance(x, str) else x for x in a], None, None, None)
    assert ok(sa, guide, site(27, 1), 27, 0, 21, 1) == 0                           # all three outputs may be left out
    assert ok(sa, guide, site(27, 1), 27, 0, 3, 1) == -22                          # n < 4
    assert ok(sa, guide, site(27, 1), 27, 0, 4, 1) == 0
    assert ok(sa, guide, site(27, 1), 27, 20, 8, 1) == -22                         # e > L
    assert ok(sa, guide, site(27, 1), 27, 0, 24, 1) == -22                         # P[23] = G inside the protospacer
    assert ok(sa, guide, site(27, 1), 27, 0, 23, 1) == 0                           # N N of the PAM may belong to it
    for d in (0, 3, -3):
        assert ok(sa, guide, site(27, d), 27, 0, 21, d) == -22                     # d
    assert ok(sa, guide, site(27, 2), 27, 0, 21, 1) == -22                         # a text of another length
    assert ok(sa, guide, site(27, 0), 27, 0, 21, 1) == -22
    assert ok(None, guide, site(27, 1), 27, 0, 21, 1) == -22 and ok(sa, None, site(27, 1), 27, 0, 21, 1) == -22
    assert ok(sa, guide, None, 27, 0, 21, 1) == -22
    assert ok("N" * 20 + "UGGNNNN", guide, site(27, 1), 27, 0, 20, 1) == -22       # what the pattern search refuses
    assert ok(sa, "A" * 20 + "U" + "N" * 6, site(27, 1), 27, 0, 21, 1) == -22
    for L, d, want in ((31, 2, -22), (31, 1, 0), (30, 2, 0), (32, 1, -22), (32, -2, 0), (16, -1, -22), (17, -2, -22), (17, -1, 0), (18, -2, 0),
                       (16, 2, 0), (15, 1, -22), (33, -1, -22)):
        assert ok("N" * L, "A" * L, site(L, d), L, 0, L, d) == want, (L, d)         # L + dna_max <= 32, L - rna_max >= 16, 16 <= L <= 32
        assert pb.refused("N" * L, (0, L), max(d, 0), max(-d, 0)) == (want != 0) or not 16 <= L <= 32
    with pytest.raises(ValueError):
        va.pattern_bulge_align(sa, guide[:-1], site(27, 1), proto, 1)
    with pytest.raises(va.VarscotError) as err:
        va.pattern_bulge_align(sa, guide, site(27, 1), (0, 24), 1)
    assert err.value.code == -22


def test_search_refuses_without_a_context():
    pp = va.PatternBulgeParams(3, 0, 0, 0, 21, 1, 1)
    assert va.lib().vsc_search_pattern_bulges(None, None, None, None, 0, 27, C.byref(pp), None, None) == -22


def test_struct_layout(tmp_path):
    f = _lib.PatternBulgeParams
    assert C.sizeof(f) == 32 and va.PatternBulgeParams is f
    assert [(n, getattr(f, n).offset) for n, _ in f._fields_] == [("max_mismatches", 0), ("guide_batch", 4), ("max_hits", 8), ("proto_start", 16),
                                                                   ("proto_len", 20), ("dna_max", 24), ("rna_max", 28)]
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc:  # the header's own asserts, the field offsets and the record macros with a pattern's index, to a C compiler
        w = pb.info_word(1, -2, 29, 8)
        src = tmp_path / "layout.c"
        src.write_text('#include <stddef.h>\n#include "varscot_hip.h"\n'
                       '_Static_assert(sizeof(vsc_pattern_bulge_params) == 32, "size");\n'
                       '_Static_assert(offsetof(vsc_pattern_bulge_params, max_hits) == 8 && offsetof(vsc_pattern_bulge_params, proto_start) == 16, "a");\n'
                       '_Static_assert(offsetof(vsc_pattern_bulge_params, proto_len) == 20 && offsetof(vsc_pattern_bulge_params, dna_max) == 24, "b");\n'
                       '_Static_assert(offsetof(vsc_pattern_bulge_params, rna_max) == 28, "c");\n'
                       '_Static_assert(VSC_BULGE_INDEX(%du) == 29 && VSC_BULGE_NM(%du) == 8 && VSC_BULGE_D(%du) == -2 && VSC_BULGE_STRAND(%du) == 1, "d");\n'
                       '_Static_assert(VSC_BULGE_INFO(0, VSC_BULGE_DNA, 2, 31, 0) >> 5 == (2u << 5 | 31u), "e");\n'
                       'int (*search)(vsc_ctx *, const vsc_genome *, const char *, const char *, uint32_t, uint32_t, const vsc_pattern_bulge_params *,\n'
                       '              vsc_bulge_hits **, vsc_bulge_summary *) = vsc_search_pattern_bulges;\n'
                       'int (*align)(const char *, const char *, const char *, uint32_t, uint32_t, uint32_t, int, uint32_t *, uint32_t *, uint32_t *) =\n'
                       '    vsc_pattern_bulge_align;\n'
                       'int main(void) { return 0; }\n' % ((w,) * 4))
        r = subprocess.run([cc, "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    fields = va.unpack_bulge_info(np.uint32(pb.info_word(1, -2, 29, 8)))
    assert {k: int(v) for k, v in fields.items()} == {"strand": 1, "kind": 1, "size": 2, "d": -2, "index": 29, "nm": 8}


def _run(*args):
    return subprocess.run([os.path.join(BIN, "pattern_search")] + list(args), capture_output=True, text=True, timeout=120,
                          env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))


def test_pattern_search_bulge_argument_errors(tmp_path):
    (tmp_path / "r.fa").write_text(">r\n" + "ACGT" * 5 + "A" + "N" * 6 + "\n")
    sa = pb.PRESETS["SaCas9"][0]
    base = ["-i", str(tmp_path / "idx"), "-q", sa, "-R", str(tmp_path / "r.fa"), "-M", "3", "-O", str(tmp_path / "out.tsv")]
    for bad in ("1", "0,0", "3,1", "1,3", "-1,1", "a,b", "1,1x", "1,", ",1", "1,1,1"):
        res = _run(*base, "-p", "0,21", "-u", bad)
        assert res.returncode == 1 and "-u takes DNA,RNA" in res.stderr and bad in res.stderr, (bad, res.stderr)
    res = _run(*base, "-u", "1,1")                                              # -u without -p
    assert res.returncode == 1 and "-u needs -p" in res.stderr
    for bad in ("0,3", "21", "7,21", "a,b"):
        res = _run(*base, "-u", "1,1", "-p", bad)
        assert res.returncode == 1 and "-u needs -p START,LENGTH" in res.stderr, (bad, res.stderr)
    res = _run(*base, "-u", "1,1", "-p", "0,24")                                # the PAM's G inside the protospacer
    assert res.returncode == 1 and "must be N" in res.stderr
    res = _run("-i", str(tmp_path / "idx"), "-q", "N" * 31, "-R", str(tmp_path / "r.fa"), "-M", "3", "-O", str(tmp_path / "out.tsv"), "-u", "2,0",
               "-p", "0,28")
    assert res.returncode == 1 and "must not exceed 32" in res.stderr
    res = _run("-i", str(tmp_path / "idx"), "-q", "N" * 17, "-R", str(tmp_path / "r.fa"), "-M", "3", "-O", str(tmp_path / "out.tsv"), "-u", "0,2",
               "-p", "0,14")
    assert res.returncode == 1 and "at least 16" in res.stderr
    res = _run(*base, "-U", str(tmp_path / "b.tsv"))                            # -U without -u
    assert res.returncode == 1 and "give -u" in res.stderr
    assert _run(*base, "-u", "1,1", "-p", "0,21", "-U", str(tmp_path / "b.bed")).returncode == 1  # wrong extension
    res = _run(*base, "-p", "0,21")                                             # -p alone still belongs to the enumeration
    assert res.returncode == 1 and "give -E" in res.stderr
    res = _run("-i", str(tmp_path / "idx"), "-q", sa, "-E", str(tmp_path / "found.tsv"), "-p", "0,21", "-u", "1,1")
    assert res.returncode == 1 and "give -M and -O" in res.stderr
    # a well-formed call gets as far as the index, which does not exist: nothing above was about the arguments
    res = _run(*base, "-u", "2,0", "-p", "0,21", "-U", str(tmp_path / "b.tsv"))
    assert res.returncode == 1 and "idx" in res.stderr
    assert not (tmp_path / "out.tsv").exists() and not (tmp_path / "b.tsv").exists()
    res = _run("--help")
    assert res.returncode == 0 and "-u, --bulges" in res.stdout and "-U, --bulge-hits" in res.stdout and "With -E or -u" in res.stdout

