"""The pattern search's host side, no device needed: vsc_pattern_match - the compare the kernels run - against the definition
restated in tests/pattern_cases.py over every (letter, base) pair, every length and hand-worked SaCas9 and Cas12a sites; the
'-' mask relation; the restatement's two forms against each other; what is refused; the new structs and macros as a C compiler
sees them; the ABI version; the presets; and pattern_search's argument checks (all made before a device is opened)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import varscot_amd as va
from varscot_amd import _lib
import pattern_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.environ.get("VSC_TEST_BIN") or os.path.join(ROOT, "varscot_amd", "bin")
NEW = ["vsc_search_pattern", "vsc_pattern_hits_count", "vsc_pattern_hits_data", "vsc_pattern_hits_data_dev", "vsc_pattern_hits_free",
       "vsc_pattern_match"]


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
    assert not any(name.startswith("vsc_multi") and "pattern" in name for name in bound)


def same(pattern, guide, site):
    got = va.pattern_match(pattern, guide, site)
    assert got == pc.site_match(pattern, guide, site), (pattern, guide, site, got)
    return got


def test_every_letter_against_every_base():
    """The 15 x 4 table twice - as a guide letter (it decides the mismatch) and as a pattern letter (it decides the hit) - at
    every position of a 16-letter and a 32-letter site, in both cases of the letters."""
    for L in (16, 32):
        for j in (0, 1, L // 2, L - 2, L - 1):
            for letter, bases in pc.IUPAC.items():
                for base in "ACGT":
                    site = "A" * j + base + "C" * (L - 1 - j)
                    guide = "A" * j + letter + "C" * (L - 1 - j)
                    hit, nm, mask = same("N" * L, guide, site)
                    assert hit and nm == int(base not in bases) and mask == nm << j
                    hit, nm, mask = same("N" * j + letter.lower() + "N" * (L - 1 - j), "N" * L, site.lower())
                    assert hit == (base in bases) and nm == 0 and mask == 0
    assert len(pc.IUPAC) == 15


def test_every_length_and_random_sites():
    rng = np.random.default_rng(11)
    letters = "".join(pc.IUPAC)
    for L in range(16, 33):
        full = same("N" * L, "T" * L, "A" * L)
        assert full == (True, L, (1 << L) - 1)  # every position counts, none beyond
        for _ in range(40):
            pattern = "".join(letters[k] for k in rng.integers(0, 15, L))
            guide = "".join(letters[k] for k in rng.integers(0, 15, L))
            same(pattern, guide, pc.rnd(rng, L))
            same("N" * L, guide, pc.make_site(rng, "N" * L, guide))


def test_hand_worked_sites():
    # SaCas9: 21 + NNGRRT.  The guide's N positions are not compared; two substitutions at 3 and 20.
    proto = "GCAGATGTAGTGTTTCCACAG"
    pattern, guide = va.pattern_strings("SaCas9", proto)
    assert (pattern, guide) == ("N" * 21 + "NNGRRT", proto + "NNNNNN") and len(pattern) == 27
    assert same(pattern, guide, proto + "TGGAGT") == (True, 0, 0)
    assert same(pattern, guide, proto + "TGGACT") == (False, 0, 0)                 # C is not R: no site, whatever the guide says
    site = proto[:3] + "T" + proto[4:20] + "C" + "CAGGAT"
    assert same(pattern, guide, site) == (True, 2, 1 << 3 | 1 << 20)
    # a guide that spells its PAM has the letters counted: T at 26 matches, A at 24 against G does not
    assert same(pattern, proto + "NNGAGT", proto + "TGGGGT") == (True, 1, 1 << 24)
    # Cas12a: TTTV at the 5' end + 23
    proto = "ATCGGATCCATTGCAGGCATAGC"
    pattern, guide = va.pattern_strings("Cas12a", proto)
    assert (pattern, guide) == ("TTTV" + "N" * 23, "NNNN" + proto) and len(pattern) == 27
    assert same(pattern, guide, "TTTC" + proto) == (True, 0, 0)
    assert same(pattern, guide, "TTTT" + proto) == (False, 0, 0)                   # T is not V
    assert same(pattern, guide, "TTTG" + "T" + proto[1:]) == (True, 1, 1 << 4)
    # a degenerate guide letter: R takes A and G
    assert same("N" * 16, "R" + "A" * 15, "G" + "A" * 15) == (True, 0, 0)
    assert same("N" * 16, "R" + "A" * 15, "C" + "A" * 15) == (True, 1, 1)
    # a site letter outside ACGT is no site
    assert same("N" * 16, "N" * 16, "A" * 8 + "N" + "A" * 7) == (False, 0, 0)
    assert same("N" * 16, "N" * 16, "A" * 8 + "R" + "A" * 7) == (False, 0, 0)


def test_minus_strand_mask_relation():
    """A '-' record's mask is the read-orientation mask with bit j moved to L - 1 - j: the compare of the forward window with
    the reverse complements of pattern and guide - what the kernels do - gives exactly that."""
    rng = np.random.default_rng(12)
    letters = "".join(pc.IUPAC)
    for L in (16, 21, 23, 27, 32):
        for _ in range(30):
            guide = "".join(letters[k] for k in rng.integers(0, 15, L))
            s = pc.rnd(rng, L)  # read orientation on '-': the forward window is its reverse complement
            hit, nm, mask = same("N" * L, guide, s)
            fwd = va.pattern_match("N" * L, pc.rc_iupac(guide), pc.rc(s))
            assert fwd == (hit, nm, pc.forward_mask(mask, 1, L))
            assert pc.forward_mask(pc.forward_mask(mask, 1, L), 1, L) == mask


def test_numpy_form_equals_the_plain_form():
    e = pc.edge_scenario(20, "both")
    starts = {(h[2], h[3]) for h in e["hits"]} | {(0, p) for p in range(0, 600)}
    want = pc.definition(e["contigs"], e["pattern"], e["guides"], pc.MAX_M, starts=starts)
    assert want == [h for h in e["hits"] if (h[2], h[3]) in starts] and len(want) == len(e["hits"])
    assert [pc.comp_letter(x) for x in "ACGTRYSWKMBDHVN"] == list("TGCAYRSWMKVHDBN")


def test_refusals():
    ok = ("N" * 20 + "NGG", "A" * 20 + "NNN", "A" * 20 + "TGG")
    assert va.pattern_match(*ok) == (True, 0, 0)
    L = va.lib()
    for n in (15, 33):
        assert L.vsc_pattern_match(b"N" * n, b"N" * n, b"A" * n, n, None, None, None) == -22
    for bad in ("U", "X", "-", " ", "0"):
        with pytest.raises(va.VarscotError) as err:
            va.pattern_match("N" * 10 + bad + "N" * 12, ok[1], ok[2])
        assert err.value.code == -22
        with pytest.raises(va.VarscotError):
            va.pattern_match(ok[0], "A" * 5 + bad.lower() + "A" * 17, ok[2])
    with pytest.raises(ValueError):
        va.pattern_match(ok[0], "A" * 22, ok[2])  # a guide of another length
    assert L.vsc_pattern_match(ok[0].encode(), b"A" * 22, ok[2].encode(), 23, None, None, None) == -22  # (ends before len)
    assert L.vsc_pattern_match(None, ok[1].encode(), ok[2].encode(), 23, None, None, None) == -22
    assert L.vsc_pattern_match(*(x.encode() for x in ok), 23, None, None, None) == 0  # every output may be left out
    # the search itself: without a context nothing else is looked at; the rules with one are tests/test_pattern.py's
    pp = va.PatternParams(9, 0, 0)
    assert L.vsc_search_pattern(None, None, b"N" * 23, b"A" * 23, 1, 23, C.byref(pp), None, None) == -22
    assert L.vsc_pattern_hits_count(None) == 0 and L.vsc_pattern_hits_free(None) == 0 and L.vsc_pattern_hits_data_dev(None) is None


def test_structs_and_macros(tmp_path):
    f = _lib.PatternParams
    assert C.sizeof(f) == 24 and va.PatternParams is f
    assert [(n, getattr(f, n).offset) for n, _ in f._fields_] == [("max_mismatches", 0), ("guide_batch", 4), ("max_hits", 8), ("reserved", 16)]
    assert va.PATTERN_HIT_DTYPE.itemsize == 20 and va.PATTERN_HIT_DTYPE.names == ("guide", "contig", "pos", "info", "mask")
    assert pc.HIT_DTYPE == va.PATTERN_HIT_DTYPE
    fields = va.unpack_pattern_info(np.array([0, 8, 1 << 31, 1 << 31 | 5], dtype=np.uint32))
    assert fields["strand"].tolist() == [0, 0, 1, 1] and fields["nm"].tolist() == [0, 8, 0, 5]
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc:  # the header's own asserts and macros, to a C compiler
        src = tmp_path / "layout.c"
        src.write_text('#include "varscot_hip.h"\n'
                       '_Static_assert(sizeof(vsc_pattern_hit) == 20 && sizeof(vsc_pattern_params) == 24, "size");\n'
                       '_Static_assert(sizeof(vsc_pattern_summary) == 36 && VSC_MAX_MISMATCHES == 8, "rows");\n'
                       '_Static_assert(VSC_PATTERN_STRAND(0x80000005u) == 1 && VSC_PATTERN_NM(0x80000005u) == 5, "a");\n'
                       '_Static_assert(VSC_PATTERN_INFO(1, 5) == 0x80000005u && VSC_PATTERN_INFO(0, 8) == 8u, "b");\n'
                       '_Static_assert(VSC_PATTERN_MIN_LEN == 16 && VSC_PATTERN_MAX_LEN == 32 && VSC_ABI_VERSION == 5, "c");\n'
                       'int main(void) { return 0; }\n')
        r = subprocess.run([cc, "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def test_presets():
    assert set(va.PATTERNS) == {"SpCas9", "SpCas9-NRG", "SpCas9-NG", "SaCas9", "Cas12a"}
    want = {"SpCas9": "N" * 20 + "NGG", "SpCas9-NRG": "N" * 20 + "NRG", "SpCas9-NG": "N" * 20 + "NGN", "SaCas9": "N" * 21 + "NNGRRT",
            "Cas12a": "TTTV" + "N" * 23}
    for name, pattern in want.items():
        five, n, three = va.PATTERNS[name]
        assert va.pattern_strings(name) == (pattern, None) and 16 <= len(pattern) <= 32
        p, g = va.pattern_strings(name, "ACGT" * 5 + "ACG"[:n - 20])
        assert p == pattern and g == "N" * len(five) + ("ACGT" * 6)[:n] + "N" * len(three)
        assert va.pattern_match(p, g, pc.make_site(np.random.default_rng(3), p, g)) == (True, 0, 0)
        with pytest.raises(ValueError):
            va.pattern_strings(name, "A" * (n + 1))
    assert va.pattern_strings(("", 17, "NGG"), "A" * 17) == ("N" * 17 + "NGG", "A" * 17 + "NNN")  # a truncated guide


def _run(*args):
    return subprocess.run([os.path.join(BIN, "pattern_search")] + list(args), capture_output=True, text=True, timeout=120,
                          env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))


def test_pattern_search_argument_errors(tmp_path):
    (tmp_path / "g.fa").write_text(">r one\n" + "ACGT" * 5 + "NNN\n")
    (tmp_path / "short.fa").write_text(">r\n" + "ACGT" * 5 + "NN\n")
    (tmp_path / "u.fa").write_text(">r\n" + "ACGU" * 5 + "NNN\n")
    g, pattern = str(tmp_path / "g.fa"), "N" * 20 + "NGG"
    base = ["-i", str(tmp_path / "idx"), "-q", pattern, "-R", g, "-M", "3"]
    out = ["-O", str(tmp_path / "out.tsv")]
    for bad in ("N" * 15, "N" * 33):
        res = _run("-i", str(tmp_path / "idx"), "-q", bad, "-R", g, "-M", "3", *out)
        assert res.returncode == 1 and "16..32" in res.stderr
    res = _run("-i", str(tmp_path / "idx"), "-q", "N" * 20 + "UGG", "-R", g, "-M", "3", *out)
    assert res.returncode == 1 and "IUPAC" in res.stderr
    res = _run(*base)                                                  # neither -O nor -T
    assert res.returncode == 1 and "-O" in res.stderr
    assert _run(*base, "-O", str(tmp_path / "out.bed")).returncode == 1  # wrong extension
    res = _run("-i", str(tmp_path / "idx"), "-q", pattern, "-R", g, "-M", "9", *out)
    assert res.returncode == 1 and "between 0 and 8" in res.stderr
    res = _run("-i", str(tmp_path / "idx"), "-q", pattern, "-R", g, "-M", "x", *out)
    assert res.returncode == 1 and "cannot be casted" in res.stderr
    res = _run(*base, *out, "-D", "0,1")
    assert res.returncode == 1 and "one device" in res.stderr
    res = _run("-i", str(tmp_path / "idx"), "-q", pattern, "-R", str(tmp_path / "short.fa"), "-M", "3", *out)
    assert res.returncode == 1 and "22 letters" in res.stderr
    res = _run("-i", str(tmp_path / "idx"), "-q", pattern, "-R", str(tmp_path / "u.fa"), "-M", "3", *out)
    assert res.returncode == 1 and "IUPAC" in res.stderr
    res = _run("-q", pattern, "-R", g, "-M", "3", *out)                # -i is required
    assert res.returncode == 1 and "-i" in res.stderr
    # a well-formed call gets as far as the index, which does not exist: nothing above was about the arguments
    res = _run(*base, *out, "-T", str(tmp_path / "hits.tsv"))
    assert res.returncode == 1 and "idx" in res.stderr
    assert not (tmp_path / "out.tsv").exists() and not (tmp_path / "hits.tsv").exists()
    res = _run("--help")
    assert res.returncode == 0 and "-q, --pattern" in res.stdout and "-T, --hits" in res.stdout
