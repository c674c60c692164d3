"""The bulge search's host side, no device needed: vsc_bulge_align - the function the kernels run - against the definition
restated in tests/bulges_cases.py over every class, every split point and random substitutions; the restatement's two forms
against each other; the new structs and the info macros as a C compiler sees them; the ABI version; what is refused; and
guide_summary's -u / -U argument checks (all made before a device is opened)."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.environ.get("VSC_TEST_BIN") or os.path.join(ROOT, "varscot_amd", "bin")
NEW = ["vsc_search_bulges", "vsc_bulge_hits_count", "vsc_bulge_hits_data", "vsc_bulge_hits_data_dev", "vsc_bulge_hits_free",
       "vsc_bulge_align"]


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
    assert not any(name.startswith("vsc_multi") and "bulge" in name for name in bound)


def test_align_equals_the_definition_at_every_split_point():
    rng = np.random.default_rng(5)
    checked = ties = 0
    for d in bc.CLASSES:
        for i in range(1, bc.max_index(d) + 1):
            for trial in range(12):
                read = bc.rnd(rng, 23) if trial % 2 else bc.distinct_read(rng)
                subs = rng.choice(23, size=trial % 5, replace=False)
                site = bc.plant(rng, read, d, i, subs, bulge=bc.rnd(rng, d) if d > 0 and trial % 3 == 0 else None)
                nm, index, tie = bc.best(read, site, d)
                assert va.bulge_align(read, site, d) == (nm, index), (read, site, d)
                assert nm <= trial % 5 and bc.nm_at(read, site, d, index) == nm
                assert all(bc.nm_at(read, site, d, j) > nm for j in range(1, index))  # the smallest index that reaches it
                if trial % 5 == 0 and trial % 2 == 0 and (d < 0 or trial % 3):
                    assert (nm, index) == (0, i)  # a read without repeats, planted without substitutions: one best split point
                checked += 1
                ties += tie
    assert checked == 12 * (17 + 18 + 19 + 19) and ties > 20
    # random sites: nothing planted, large NM, lower case, a read with a letter that becomes A
    for _ in range(300):
        d = int(rng.choice(bc.CLASSES))
        read, site = bc.rnd(rng, 23), bc.rnd(rng, 23 + d)
        assert va.bulge_align(read.lower(), site.lower(), d) == bc.best(read, site, d)[:2]
    assert va.bulge_align("N" * 23, "A" * 24, 1) == (0, 1)


def test_hand_worked_sites():
    r = "ACGTACGTACGTACGTACGTAGG"
    assert bc.best(r, r[:5] + "T" + r[5:], 1) == (0, 5, False)       # a T between C and G... r[4] = A, r[5] = C: one place
    assert bc.best(r, r[:5] + "A" + r[5:], 1) == (0, 4, True)        # an A behind the A at 4: index 4 and 5 pair alike
    assert bc.best(r, r[:5] + r[6:], -1) == (0, 5, False)
    assert bc.best(r, r[:19] + "TT" + r[19:], 2)[:2] == (0, 19)      # the largest DNA index
    assert bc.best(r, r[:17] + r[19:], -2)[:2] == (0, 17)            # the largest RNA index: i + b <= 19
    assert bc.best(r, "T" + r, 1)[:2] == (1, 1)                      # the bulged neighbour of a plain hit: r[0] pairs the extra base
    assert bc.best(r, r[1:], -1)[:2] == (1, 1)
    for site, d in ((r[:5] + "T" + r[5:], 1), (r[:5] + "A" + r[5:], 1), (r[:17] + r[19:], -2), ("T" + r, 1), (r[1:], -1)):
        assert va.bulge_align(r, site, d) == bc.best(r, site, d)[:2]


def test_numpy_form_equals_the_plain_form():
    e = bc.edge_scenario()
    want = {}
    for strand, c, p, d, s in e["cands"][::7]:
        for g, text in enumerate(e["guides"]):
            nm, index, tie = bc.best(bc.read_of(text), s, d)
            if nm <= bc.EDGE_M:
                want[(g, strand, c, p, d)] = (nm, index, tie)
    got = {h[:5]: h[5:] for h in bc.brute_force(e["contigs"], e["guides"], bc.EDGE_M, 2, 2, cands=e["cands"][::7])}
    assert want and got == want


def test_align_refuses_what_is_no_site():
    for site, d in (("A" * 23, 0), ("A" * 26, 3), ("A" * 20, -3), ("A" * 24, 2), ("A" * 23, 1), ("A" * 12 + "N" + "A" * 11, 1),
                    ("A" * 12 + "R" + "A" * 8, -2)):
        with pytest.raises(va.VarscotError) as err:
            va.bulge_align("A" * 23, site, d)
        assert err.value.code == -22
    with pytest.raises(ValueError):
        va.bulge_align("A" * 22, "A" * 24, 1)
    assert va.lib().vsc_bulge_align(0, b"A" * 24, 1, None, None) == 0  # either output may be left out
    assert va.lib().vsc_bulge_align(0, None, 1, None, None) == -22


def test_search_refuses_without_a_context():
    bp, p = va.BulgeParams(1, 1, 0, 0, 0), _lib.SearchParams()
    assert va.lib().vsc_search_bulges(None, None, None, 0, C.byref(p), C.byref(bp), None, None) == -22
    assert va.lib().vsc_bulge_hits_count(None) == 0 and va.lib().vsc_bulge_hits_free(None) == 0
    assert va.lib().vsc_bulge_hits_data_dev(None) is None


def test_structs_and_info_macros(tmp_path):
    assert C.sizeof(_lib.BulgeParams) == 24 and va.BulgeParams is _lib.BulgeParams
    f = _lib.BulgeParams
    assert [(n, getattr(f, n).offset) for n, _ in f._fields_] == [("dna_max", 0), ("rna_max", 4), ("guide_batch", 8), ("reserved", 12),
                                                                   ("max_hits", 16)]
    assert va.BULGE_HIT_DTYPE.itemsize == 16 and va.BULGE_HIT_DTYPE.names == ("guide", "contig", "pos", "info")
    assert (va.BULGE_DNA, va.BULGE_RNA) == (0, 1)
    words = [bc.info_word(s, d, i, nm) for s in (0, 1) for d in bc.CLASSES for i in (1, 17, 19) for nm in (0, 8)]
    fields = va.unpack_bulge_info(np.array(words, dtype=np.uint32))
    k = 0
    for s in (0, 1):
        for d in bc.CLASSES:
            for i in (1, 17, 19):
                for nm in (0, 8):
                    got = {name: int(v[k]) for name, v in fields.items()}
                    assert got == {"strand": s, "kind": int(d < 0), "size": abs(d), "d": d, "index": i, "nm": nm}
                    k += 1
    assert int(va.unpack_bulge_info(bc.info_word(1, -2, 17, 3))["d"]) == -2
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc:  # the header's own asserts and macros, to a C compiler
        w = bc.info_word(1, -2, 17, 3)
        src = tmp_path / "layout.c"
        src.write_text('#include "varscot_hip.h"\n'
                       '_Static_assert(sizeof(vsc_bulge_hit) == 16 && sizeof(vsc_bulge_params) == 24, "size");\n'
                       '_Static_assert(sizeof(vsc_bulge_summary) == 4 * 9 * 4 && VSC_BULGE_CLASSES == 4, "rows");\n'
                       '_Static_assert(VSC_BULGE_STRAND(%du) == 1 && VSC_BULGE_KIND(%du) == VSC_BULGE_RNA && VSC_BULGE_SIZE(%du) == 2, "a");\n'
                       '_Static_assert(VSC_BULGE_INDEX(%du) == 17 && VSC_BULGE_NM(%du) == 3 && VSC_BULGE_D(%du) == -2, "b");\n'
                       '_Static_assert(VSC_BULGE_INFO(1, VSC_BULGE_RNA, 2, 17, 3) == %du, "c");\n'
                       '_Static_assert(VSC_BULGE_D(VSC_BULGE_INFO(0, VSC_BULGE_DNA, 1, 5, 0)) == 1, "d");\n'
                       'int main(void) { return 0; }\n' % ((w,) * 7))
        r = subprocess.run([cc, "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def _run(*args):
    return subprocess.run([os.path.join(BIN, "guide_summary")] + list(args), capture_output=True, text=True, timeout=120,
                          env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))


def test_guide_summary_bulge_argument_errors(tmp_path):
    (tmp_path / "g.fa").write_text(">c\n" + "ACGT" * 30 + "\n")
    (tmp_path / "r.fa").write_text(">r\n" + "ACGT" * 5 + "AGG\n")
    (tmp_path / "b.bed").write_text("c\t0\t23\tr\t0\t+\n")
    (tmp_path / "s.vcf").write_text("##fileformat=VCFv4.2\n")
    g, r = str(tmp_path / "g.fa"), str(tmp_path / "r.fa")
    base = ["-G", g, "-I", str(tmp_path / "idx"), "-O", str(tmp_path / "out.tsv"), "-M", "3", "-R", r]
    for bad in ("1", "0,0", "3,1", "1,3", "-1,1", "a,b", "1,1x", "1,", ",1", "1,1,1"):
        res = _run(*base, "-u", bad)
        assert res.returncode == 1 and "-u takes DNA,RNA" in res.stderr and bad in res.stderr, (bad, res.stderr)
    res = _run(*base, "-U", str(tmp_path / "b.tsv"))                       # -U without -u
    assert res.returncode == 1 and "give -u" in res.stderr
    assert _run(*base, "-u", "1,1", "-U", str(tmp_path / "b.bed")).returncode == 1  # wrong extension
    res = _run(*base, "-u", "1,1", "-v", str(tmp_path / "s.vcf"))
    assert res.returncode == 1 and "-u" in res.stderr and "-v" in res.stderr
    res = _run(*base, "-u", "1,1", "-D", "0,1")
    assert res.returncode == 1 and "one device" in res.stderr
    res = _run("-G", g, "-I", str(tmp_path / "idx"), "-M", "3", "-B", str(tmp_path / "b.bed"), "-u", "1,1", "-J", str(tmp_path / "p.tsv"),
               "-j", "-4,20")
    assert res.returncode == 1 and "-J" in res.stderr
    # a well-formed call gets as far as the index, which does not exist: nothing above was about the arguments
    res = _run(*base, "-u", "2,0", "-U", str(tmp_path / "b.tsv"))
    assert res.returncode == 1 and "idx" in res.stderr
    assert not (tmp_path / "out.tsv").exists() and not (tmp_path / "b.tsv").exists()
    res = _run("--help")
    assert res.returncode == 0 and "-u, --bulges" in res.stdout and "-U, --bulge-hits" in res.stdout
