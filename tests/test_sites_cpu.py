"""Cut sites without a device: vsc_sites_collapse / vsc_sites_collapse_pattern byte for byte what the definition gives when it is
restated in plain Python (tests/sites_cases.py) - on the edge, homopolymer and Cas12a scenarios, on vsc_hit records and the same
records as vsc_pattern_hit, on empty and one-sided inputs - every refusal, the layouts and macros through a C compiler, the
Python wrappers, and the argument checks of guide_summary -Z and pattern_search -Z."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import varscot_amd as va
from varscot_amd import _lib
import bulges_cases as bc
import sites_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "varscot_amd", "bin")


@pytest.fixture(scope="module")
def edge(oracle):
    return sc.edge_scenario(oracle)


@pytest.fixture(scope="module")
def homo(oracle):
    return sc.homopolymer_scenario(oracle)


def same(got, want):
    assert got[0].dtype == va.SITE_DTYPE and got[1].dtype == va.SITE_ROW_DTYPE
    assert len(got[0]) == len(want[0])
    assert got[0].tobytes() == want[0].tobytes()
    assert got[1].tobytes() == want[1].tobytes()


def test_new_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "varscot_hip.h")).read()
    names = ["vsc_hits_sites", "vsc_pattern_hits_sites", "vsc_sites_count", "vsc_sites_data", "vsc_sites_data_dev", "vsc_sites_free",
             "vsc_sites_collapse", "vsc_sites_collapse_pattern"]
    bound = {n for n, _, _ in _lib.SYMBOLS}
    for n in names:
        assert n + "(" in text and n in bound and hasattr(va.lib(), n), n
    assert "vsc_debug_sites_ms" in {n for n, _, _ in _lib.DEBUG_SYMBOLS}
    assert "suppressing the bulged neighbours" not in text.split("Not provided")[-1]


# ---- 1. the definition ----------------------------------------------------------------------------------------------------
def test_edge_scenario_equals_the_restatement(edge):
    n = len(edge["guides"])
    got = va.collapse_sites(edge["plain_rec"], edge["bulged_rec"], n)
    same(got, sc.arrays(edge["sites"], edge["plain"], edge["bulged"], n))
    assert len(got[0]) == 140 and int(got[1]["alignments"].sum()) == 305 and int(got[1]["sites"].sum()) == 140
    assert int(got[1]["bulge_only"].sum()) == sum(1 for s in edge["sites"] if 0 not in s[4]) > 0


@pytest.mark.parametrize("m", [0, 2, 4])
@pytest.mark.parametrize("dna,rna", [(1, 0), (0, 2), (2, 2)])
def test_budgets_and_classes(edge, m, dna, rna):
    plain, bulged = sc.at_budget(edge, m, dna, rna)
    n = len(edge["guides"])
    keep_p = np.array([x[5] <= m for x in edge["plain"]], dtype=bool)
    keep_b = np.array([x[5] <= m and x[4] in bc.enabled(dna, rna) for x in edge["bulged"]], dtype=bool)
    assert keep_b.any()
    same(va.collapse_sites(edge["plain_rec"][keep_p], edge["bulged_rec"][keep_b], n), sc.expected(plain, bulged, n))


def test_homopolymer_scenario_equals_the_restatement(homo):
    got = va.collapse_sites(homo["plain_rec"], homo["bulged_rec"], 1)
    same(got, sc.arrays(homo["sites"], homo["plain"], homo["bulged"], 1))
    u = va.unpack_site_members(got[0]["members"])
    assert int(u["count"].max()) == 5 and int(u["count"].min()) < 5


def test_cas12a_scenario_with_the_start_anchor():
    e = sc.cas12a_scenario()
    n = len(e["guides"])
    assert e["plain_rec"].dtype == va.PATTERN_HIT_DTYPE
    same(va.collapse_sites(e["plain_rec"], e["bulged_rec"], n, length=e["length"], anchor="start"),
         sc.arrays(e["sites"], e["plain"], e["bulged"], n))
    other = va.collapse_sites(e["plain_rec"], e["bulged_rec"], n, length=e["length"], anchor="end")
    same(other, sc.expected(e["plain"], e["bulged"], n, e["length"], "end"))
    assert other[0].tobytes() != sc.arrays(e["sites"], e["plain"], e["bulged"], n)[0].tobytes()


def as_pattern(rec):
    """vsc_hit records as vsc_pattern_hit: the strand and the NM move, the mask goes to its own word."""
    out = np.zeros(len(rec), dtype=va.PATTERN_HIT_DTYPE)
    for f in ("guide", "contig", "pos"):
        out[f] = rec[f]
    out["info"] = (rec["info"] & np.uint32(0x80000000)) | ((rec["info"] >> 23) & 31)
    out["mask"] = rec["info"] & 0x7FFFFF
    return out


def test_hit_records_and_their_pattern_form_collapse_alike(edge, homo):
    for e in (edge, homo):
        n = len(e["guides"])
        a = va.collapse_sites(e["plain_rec"], e["bulged_rec"], n)
        b = va.collapse_sites(as_pattern(e["plain_rec"]), e["bulged_rec"], n)
        assert len(a[0]) and a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_len_cancels_out_of_membership(edge):
    n = len(edge["guides"])
    a = va.collapse_sites(edge["plain_rec"], edge["bulged_rec"], n, length=23)
    b = va.collapse_sites(edge["plain_rec"], edge["bulged_rec"], n, length=30)
    for f in ("guide", "contig", "pos", "info", "members", "best"):
        assert np.array_equal(a[0][f], b[0][f]), f
    assert not np.array_equal(a[0]["anchor"], b[0]["anchor"]) and a[1].tobytes() == b[1].tobytes()


# ---- 2. empty and one-sided inputs ----------------------------------------------------------------------------------------
def test_empty_and_one_sided_inputs(edge):
    n = len(edge["guides"])
    none_p, none_b = np.zeros(0, dtype=va.HIT_DTYPE), np.zeros(0, dtype=va.BULGE_HIT_DTYPE)
    for plain, bulged in ((none_p, none_b), (none_p, None), (None, none_b)):
        sites, rows = va.collapse_sites(plain, bulged, n)
        assert len(sites) == 0 and rows.tobytes() == np.zeros(n, dtype=va.SITE_ROW_DTYPE).tobytes()
    # plain only: every site has one member, itself
    for bulged in (None, none_b):
        sites, rows = va.collapse_sites(edge["plain_rec"], bulged, n)
        same((sites, rows), sc.expected(edge["plain"], [], n))
        assert len(sites) == len(edge["plain_rec"]) and set(va.unpack_site_members(sites["members"])["count"]) == {1}
        assert np.array_equal(sites["best"], np.arange(len(sites))) and int(rows["bulge_only"].sum()) == 0
    # bulged only: every site is bulge-only
    for plain in (None, none_p):
        sites, rows = va.collapse_sites(plain, edge["bulged_rec"], n)
        same((sites, rows), sc.expected([], edge["bulged"], n))
        assert int(rows["bulge_only"].sum()) == len(sites) and int(rows["count"][:, 0].sum()) == 0


def test_counting_without_records_and_the_capacity(edge):
    n = len(edge["guides"])
    L = va.lib()
    p = _lib.SiteParams(23, _lib.SITE_ANCHOR_END)
    plain, bulged = edge["plain_rec"], edge["bulged_rec"]
    args = (plain.ctypes.data_as(C.c_void_p), len(plain), bulged.ctypes.data_as(C.c_void_p), len(bulged), n, C.byref(p))
    total = C.c_uint64(0)
    rows = np.zeros(n, dtype=va.SITE_ROW_DTYPE)
    assert L.vsc_sites_collapse(*args, None, 0, C.byref(total), rows.ctypes.data_as(C.c_void_p)) == 0
    assert total.value == 140 and rows.tobytes() == sc.arrays(edge["sites"], edge["plain"], edge["bulged"], n)[1].tobytes()
    small = np.full(139, 7, dtype=va.SITE_DTYPE)
    assert L.vsc_sites_collapse(*args, small.ctypes.data_as(C.c_void_p), 139, C.byref(total), None) == -34
    assert total.value == 140 and (small["guide"] == 7).all()  # nothing written
    exact = np.zeros(140, dtype=va.SITE_DTYPE)
    assert L.vsc_sites_collapse(*args, exact.ctypes.data_as(C.c_void_p), 140, None, None) == 0
    assert exact.tobytes() == sc.arrays(edge["sites"], edge["plain"], edge["bulged"], n)[0].tobytes()


# ---- 3. refusals ----------------------------------------------------------------------------------------------------------
def test_refusals(edge):
    n = len(edge["guides"])
    L = va.lib()
    plain, bulged = edge["plain_rec"], edge["bulged_rec"]
    pp, bp = plain.ctypes.data_as(C.c_void_p), bulged.ctypes.data_as(C.c_void_p)
    total = C.c_uint64(0)
    ok = _lib.SiteParams(23, _lib.SITE_ANCHOR_END)
    for fn in (L.vsc_sites_collapse, L.vsc_sites_collapse_pattern):
        assert fn(None, 0, None, 0, n, C.byref(ok), None, 0, C.byref(total), None) == -22          # both inputs NULL
        assert fn(pp, 0, bp, len(bulged), n, C.byref(ok), None, 0, None, None) == -22              # no output at all
        assert fn(pp, 0, bp, len(bulged), n, None, None, 0, C.byref(total), None) == -22           # no parameters
        assert fn(None, 5, bp, len(bulged), n, C.byref(ok), None, 0, C.byref(total), None) == -22  # a count without its array
        for bad in (_lib.SiteParams(15, 0), _lib.SiteParams(33, 0), _lib.SiteParams(23, 2), _lib.SiteParams(23, 0, (1, 0)),
                    _lib.SiteParams(23, 1, (0, 1))):
            assert fn(pp, 0, bp, len(bulged), n, C.byref(bad), None, 0, C.byref(total), None) == -22
        for good in (_lib.SiteParams(16, 0), _lib.SiteParams(32, 1)):
            assert fn(pp, 0, bp, len(bulged), n, C.byref(good), None, 0, C.byref(total), None) == 0
        # a record whose guide is not below n_guides, in either list
        assert fn(pp, 0, bp, len(bulged), int(bulged["guide"].max()), C.byref(ok), None, 0, C.byref(total), None) == -22
        assert fn(pp, 0, bp, len(bulged), int(bulged["guide"].max()) + 1, C.byref(ok), None, 0, C.byref(total), None) == 0
        # more than 2^32 - 1 alignments in total (refused before a record is read)
        assert fn(pp, 2 ** 32 - 1, bp, 1, n, C.byref(ok), None, 0, C.byref(total), None) == -34
        assert fn(pp, 2 ** 32, None, 0, n, C.byref(ok), None, 0, C.byref(total), None) == -34
    assert L.vsc_sites_collapse(pp, len(plain), None, 0, int(plain["guide"].max()), C.byref(ok), None, 0, C.byref(total), None) == -22
    with pytest.raises(ValueError):
        va.collapse_sites(plain, bulged, n, anchor="middle")
    with pytest.raises(va.VarscotError) as e:
        va.collapse_sites(plain, bulged, n, length=40)
    assert e.value.code == -22
    with pytest.raises(va.VarscotError):
        va.collapse_sites(None, None, n)


def test_device_calls_refuse_without_a_context():
    L = va.lib()
    p = _lib.SiteParams(23, 0)
    h = C.c_void_p(1)
    rows = np.zeros(1, dtype=va.SITE_ROW_DTYPE)
    for fn in (L.vsc_hits_sites, L.vsc_pattern_hits_sites):
        assert fn(None, None, None, 1, C.byref(p), C.byref(h), rows.ctypes.data_as(C.c_void_p)) == -22
        assert h.value is None  # *out is cleared first
    assert L.vsc_sites_count(None) == 0 and L.vsc_sites_free(None) == 0 and L.vsc_sites_data_dev(None) is None
    assert L.vsc_sites_data(None, C.byref(h)) == -22
    assert L.vsc_debug_sites_ms(None, None, None) == -22


# ---- 4. layouts, macros, wrappers -----------------------------------------------------------------------------------------
def test_structs_and_macros(tmp_path):
    assert C.sizeof(_lib.SiteParams) == 16
    f = _lib.SiteParams
    assert [(n, getattr(f, n).offset) for n, _ in f._fields_] == [("len", 0), ("anchor", 4), ("reserved", 8)]
    assert va.SITE_DTYPE.itemsize == 32 and va.SITE_DTYPE.names == ("guide", "contig", "pos", "info", "anchor", "members", "best", "reserved")
    assert va.SITE_ROW_DTYPE.itemsize == 120 and va.SITE_ROW_DTYPE.names == ("sites", "alignments", "bulge_only", "count")
    assert va.SITE_ROW_DTYPE["count"].shape == (3, 9) and va.SITE_ROW_DTYPE.fields["count"][1] == 12
    w = sc.members_word({-1: 3, 0: 2, 1: 3})
    u = va.unpack_site_members(w)
    assert u["nm"].tolist() == [-1, 3, 2, 3, -1] and int(u["count"]) == 3
    u = va.unpack_site_members(np.array([w, sc.members_word({2: 8}), sc.members_word({-2: 0, -1: 1, 0: 2, 1: 3, 2: 4})], dtype=np.uint32))
    assert u["nm"].tolist() == [[-1, 3, 2, 3, -1], [-1, -1, -1, -1, 8], [0, 1, 2, 3, 4]] and u["count"].tolist() == [3, 1, 5]
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc:  # the header's own asserts and macros, to a C compiler
        src = tmp_path / "layout.c"
        src.write_text('#include <stddef.h>\n#include "varscot_hip.h"\n'
                       '_Static_assert(sizeof(vsc_site) == 32 && sizeof(vsc_site_summary) == 120 && sizeof(vsc_site_params) == 16, "size");\n'
                       '_Static_assert(offsetof(vsc_site, anchor) == 16 && offsetof(vsc_site, members) == 20 && offsetof(vsc_site, best) == 24, "a");\n'
                       '_Static_assert(offsetof(vsc_site_summary, bulge_only) == 8 && offsetof(vsc_site_summary, count) == 12, "b");\n'
                       '_Static_assert(VSC_SITE_ANCHOR_END == 0 && VSC_SITE_ANCHOR_START == 1 && VSC_SITE_ABSENT == 31, "c");\n'
                       '_Static_assert(VSC_SITE_MEMBER_NM(%du, -1) == 3 && VSC_SITE_MEMBER_NM(%du, 0) == 2 && VSC_SITE_MEMBER_NM(%du, 1) == 3, "d");\n'
                       '_Static_assert(VSC_SITE_MEMBER_NM(%du, -2) == VSC_SITE_ABSENT && VSC_SITE_MEMBER_NM(%du, 2) == VSC_SITE_ABSENT, "e");\n'
                       '_Static_assert(VSC_SITE_MEMBERS(%du) == 3, "f");\n'
                       'int main(void) { return 0; }\n' % ((w,) * 6))
        r = subprocess.run([cc, "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def test_collapse_sites_takes_what_numpy_gives(edge):
    n = len(edge["guides"])
    want = sc.arrays(edge["sites"], edge["plain"], edge["bulged"], n)
    # non-contiguous views and lists of tuples
    two_p, two_b = np.repeat(edge["plain_rec"], 2)[::2], np.repeat(edge["bulged_rec"], 2)[::2]
    assert not two_b.flags["C_CONTIGUOUS"]
    same(va.collapse_sites(two_p, two_b, n), want)
    f = va.unpack_bulge_info(want[0]["info"])
    plain_best = f["size"] == 0
    assert plain_best.any() and (~plain_best).any() and (f["index"][plain_best] == 0).all() and (f["kind"][plain_best] == 0).all()
    # best = the index in ITS list: the record there is the site's best alignment
    got = va.collapse_sites(edge["plain_rec"], edge["bulged_rec"], n)[0]
    for s in got:
        src = edge["bulged_rec"] if (int(s["info"]) >> 10) & 3 else edge["plain_rec"]
        r = src[int(s["best"])]
        assert (int(r["guide"]), int(r["contig"]), int(r["pos"])) == (int(s["guide"]), int(s["contig"]), int(s["pos"]))


# ---- 5. the tools' arguments ----------------------------------------------------------------------------------------------
def _run(tool, *args):
    return subprocess.run([os.path.join(BIN, tool)] + list(args), capture_output=True, text=True, timeout=120,
                          env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))


def test_guide_summary_sites_argument_errors(tmp_path):
    (tmp_path / "g.fa").write_text(">c\n" + "ACGT" * 30 + "\n")
    (tmp_path / "r.fa").write_text(">r\n" + "ACGT" * 5 + "AGG\n")
    g, r = str(tmp_path / "g.fa"), str(tmp_path / "r.fa")
    base = ["-G", g, "-I", str(tmp_path / "idx"), "-O", str(tmp_path / "out.tsv"), "-M", "3", "-R", r]
    res = _run("guide_summary", *base, "-Z", str(tmp_path / "s.tsv"))                       # -Z without -u
    assert res.returncode == 1 and "-Z" in res.stderr and "give -u" in res.stderr
    res = _run("guide_summary", *base, "-u", "1,1", "-Z", str(tmp_path / "s.bed"))          # wrong extension
    assert res.returncode == 1 and "-Z" in res.stderr
    res = _run("guide_summary", *base, "-u", "1,1", "-Z", str(tmp_path / "s.tsv"), "-D", "0,1")  # -u's own restrictions hold
    assert res.returncode == 1 and "one device" in res.stderr
    # a well-formed call gets as far as the index, which does not exist
    res = _run("guide_summary", *base, "-u", "2,2", "-Z", str(tmp_path / "s.tsv"))
    assert res.returncode == 1 and "idx" in res.stderr
    assert not (tmp_path / "out.tsv").exists() and not (tmp_path / "s.tsv").exists()
    res = _run("guide_summary", "--help")
    assert res.returncode == 0 and "-Z, --sites" in res.stdout


def test_pattern_search_sites_argument_errors(tmp_path):
    (tmp_path / "q.fa").write_text(">q\n" + "ACGT" * 5 + "A" + "NNNNNN\n")
    q = str(tmp_path / "q.fa")
    sa = "N" * 21 + "NNGRRT"
    base = ["-i", str(tmp_path / "idx"), "-q", sa, "-R", q, "-M", "3"]
    res = _run("pattern_search", *base, "-Z", str(tmp_path / "s.tsv"))                      # -Z without -u (and no other output)
    assert res.returncode == 1
    res = _run("pattern_search", *base, "-O", str(tmp_path / "o.tsv"), "-Z", str(tmp_path / "s.tsv"))
    assert res.returncode == 1 and "-Z" in res.stderr and "give -u" in res.stderr
    res = _run("pattern_search", *base, "-u", "1,1", "-p", "0,21", "-Z", str(tmp_path / "s.bed"))
    assert res.returncode == 1 and "-Z" in res.stderr
    res = _run("pattern_search", *base, "-u", "1,1", "-p", "1,20", "-Z", str(tmp_path / "s.tsv"))   # a protospacer inside the pattern
    assert res.returncode == 1 and "start or end the pattern" in res.stderr
    res = _run("pattern_search", *base, "-u", "1,1", "-p", "0,21", "-Z", str(tmp_path / "s.tsv"))   # -Z alone is an output
    assert res.returncode == 1 and "-Z" not in res.stderr and "idx" in res.stderr
    assert not (tmp_path / "s.tsv").exists()
    res = _run("pattern_search", "--help")
    assert res.returncode == 0 and "-Z, --sites" in res.stdout
