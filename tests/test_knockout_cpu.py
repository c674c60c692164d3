"""Knock-out design without a device: vsc_knockout_site_text - the functions the kernels call, on the host - bit for bit against
the definition restated on strings (tests/knockout_cases.py), the per-transcript table and the occupancy bitmap against values
computed by hand, the refusals, the Python surface and the stand-alone check under the host sanitizers."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import knockout_cases as kc
import varscot_amd as va
from varscot_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "varscot_amd", "bin")


@pytest.fixture(scope="module")
def small():
    contigs, segments = kc.small_genome()
    packed = va.PackedGenome.from_sequences(list(contigs))
    cds = va.Cds(packed, segments, n_tx=kc.N_TX)
    yield {"contigs": contigs, "segments": segments, "packed": packed, "cds": cds,
           "loci": kc.every_locus(contigs) + kc.invalid_loci(contigs)}
    cds.close()


@pytest.mark.parametrize("code", sorted(kc.CODES))
@pytest.mark.parametrize("shape", sorted(kc.SHAPES))
def test_site_text_against_the_restatement(small, shape, code):
    """Every locus of the small genome on both strands, and the invalid ones: the four words of the row."""
    want = kc.expected(small["contigs"], small["segments"], small["loci"], kc.SHAPES[shape], kc.CODES[code])
    sh = va.KnockoutShape(*kc.SHAPES[shape])
    letters = None if code == "standard" else kc.code_string(kc.CODES[code])
    got = np.array([va.knockout_site_text(small["cds"], small["contigs"], c, p, s, sh, letters) for c, p, s in small["loci"]])
    differ = np.flatnonzero((got != want["rows"]).any(axis=1))
    assert len(differ) == 0, (small["loci"][differ[0]], got[differ[0]], want["rows"][differ[0]], want["detail"][differ[0]])
    assert want["stats"]["coding"] > 500 and want["stats"]["undefined"] >= len(kc.invalid_loci(small["contigs"]))


def test_the_small_genome_holds_what_it_is_for(small):
    kc.occurrences(small["contigs"], small["segments"])
    # cuts at x = start, start + 1, end - 1 and end of a segment, and between two abutting segments, under the SpCas9 shape
    want = kc.expected(small["contigs"], small["segments"], small["loci"], kc.SHAPES["SpCas9"])
    by_cut = {}
    for (c, p, s), row in zip(small["loci"], want["rows"]):
        if int(row[0]) != kc.UNDEF or int(row[1]) != kc.UNDEF:
            by_cut.setdefault((c, p + 6 if s else p + 17), set()).add(tuple(int(w) for w in row))
    for c, start, end, tx, _, _ in small["segments"]:
        if end - start < 2:
            continue
        for x, coding in ((start, False), (start + 1, True), (end - 1, True), (end, False)):
            rows = by_cut[(c, x)]
            assert len(rows) == 1  # (both strands give the cut the same row)
            row = next(iter(rows))
            assert (row[0] == tx) == coding
            if not coding:
                assert row[2] >> 31 == 1  # a junction: one of the two bases lies in the segment
    (abut,) = [e for c, s, e, tx, _, _ in small["segments"] if tx == 4]
    assert next(iter(by_cut[(4, abut)])) == (0xFFFFFFFF, 0, 0x80000000, 0)
    assert next(iter(by_cut[(2, 250)])) == (0xFFFFFFFF, 0, 0, 0)  # 500 bases without a segment


def test_the_per_transcript_table_and_the_bitmap_by_hand(small):
    """What vsc_cds_build derives for the walk: shift, E_t = shift + B_t, J_t and the segments per transcript, and one bit per
    256 global positions that overlap a segment."""
    n_blocks = C.c_uint32()
    table = np.full((kc.N_TX, 4), 9, dtype=np.uint32)
    _lib.check(va.lib().vsc_debug_knockout_table(small["cds"]._h, _lib.ptr(table), None, C.byref(n_blocks)))
    by_hand = {0: (0, 102, 76, 4), 1: (0, 102, 76, 4), 2: (1, 95, 75, 2), 3: (2, 42, 2, 1), 4: (0, 21, 0, 1), 5: (0, 24, 0, 1),
               6: (0, 70, 30, 2), 7: (0, 0, 0, 0)}
    assert {t: tuple(int(v) for v in table[t]) for t in range(kc.N_TX)} == by_hand
    txs = kc.transcripts_of(small["segments"])
    for t, tr in txs.items():
        bases, junction = kc.table_of(tr)
        assert by_hand[t][1] == tr[2] + bases and by_hand[t][3] == len(tr[3])
        assert junction is None or by_hand[t][2] == junction
    total = int(small["packed"].contigs["offset"][-1] + small["packed"].contigs["length"][-1])
    assert n_blocks.value == (total + 255) // 256
    bitmap = np.zeros((n_blocks.value + 31) // 32, dtype=np.uint32)
    _lib.check(va.lib().vsc_debug_knockout_table(small["cds"]._h, None, _lib.ptr(bitmap), C.byref(n_blocks)))
    off = [int(o) for o in small["packed"].contigs["offset"]]
    want = {(off[c] + x) // 256 for c, s, e, *_ in small["segments"] for x in range(s, e)}
    assert {b for b in range(n_blocks.value) if bitmap[b // 32] >> (b % 32) & 1} == want and 0 < len(want) < n_blocks.value


def raw_site_text(cds, texts, locus, shape, code=None, reserved=(0, 0, 0), row=True, texts_null=False, shape_null=False):
    arr = (C.c_char_p * len(texts))(*[t.encode() for t in texts])
    out = np.full(4, 7, dtype=np.uint32)
    sh = _lib.KnockoutShapeStruct(*shape, (C.c_uint32 * 3)(*reserved))
    rc = va.lib().vsc_knockout_site_text(cds, None if texts_null else arr, locus[0], locus[1], locus[2], None if shape_null else C.byref(sh), code,
                                         _lib.ptr(out) if row else None)
    return rc, out.tolist()


def test_site_text_refusals(small):
    """Every refusal leaves the row untouched."""
    cds, texts, at, ok = small["cds"]._h, small["contigs"], (0, 50, 0), (23, 17, 50, 0, 4096)
    assert raw_site_text(cds, texts, at, ok)[0] == 0
    refusals = [
        raw_site_text(cds, texts, at, (15, 7, 50, 0, 4096)), raw_site_text(cds, texts, at, (33, 17, 50, 0, 4096)),
        raw_site_text(cds, texts, at, (23, 0, 50, 0, 4096)), raw_site_text(cds, texts, at, (23, 23, 50, 0, 4096)),
        raw_site_text(cds, texts, at, (23, 17, 65536, 0, 4096)), raw_site_text(cds, texts, at, (23, 17, 50, 65536, 4096)),
        raw_site_text(cds, texts, at, (23, 17, 50, 0, 0)), raw_site_text(cds, texts, at, (23, 17, 50, 0, 4097)),
        raw_site_text(cds, texts, at, ok, reserved=(1, 0, 0)), raw_site_text(cds, texts, at, ok, reserved=(0, 0, 1)),
        raw_site_text(cds, texts, at, ok, code=b"K" * 63), raw_site_text(None, texts, at, ok), raw_site_text(cds, texts, at, ok, texts_null=True),
        raw_site_text(cds, texts, at, ok, shape_null=True),
    ]
    for rc, row in refusals:
        assert rc == -22 and row == [7, 7, 7, 7]
    assert raw_site_text(cds, texts, at, ok, row=False)[0] == -22
    # what is no refusal: the invalid loci give the undefined row
    for locus in kc.invalid_loci(texts):
        assert raw_site_text(cds, texts, locus, ok) == (0, [kc.UNDEF] * 4)
    assert raw_site_text(cds, texts, at, (16, 15, 65535, 65535, 1))[0] == 0 and raw_site_text(cds, texts, at, (32, 31, 0, 0, 4096))[0] == 0


def test_struct_sizes_and_the_python_checks():
    assert C.sizeof(_lib.KnockoutShapeStruct) == 32 and C.sizeof(_lib.KnockoutLimits) == 32 and C.sizeof(_lib.KnockoutStats) == 128
    for bad in (dict(site_len=15), dict(site_len=33), dict(cut=0), dict(cut=23), dict(nmd_window=65536), dict(start_window=-1),
                dict(max_codons=0), dict(max_codons=4097)):
        with pytest.raises(ValueError):
            va.KnockoutShape(**bad)
    sp = va.KNOCKOUT_SHAPES["SpCas9"]
    assert (sp.site_len, sp.cut, sp.nmd_window, sp.start_window, sp.max_codons) == (23, 17, 50, 0, 4096)
    assert va.KNOCKOUT_FLAGS == kc.FLAGS and va.KNOCKOUT_UNDEFINED == kc.UNDEF
    assert (va.KNOCKOUT_END, va.KNOCKOUT_CAP, va.KNOCKOUT_UNKNOWN) == (kc.END, kc.CAP, kc.UNKNOWN)
    assert va.knockout_flag_mask(None) == 0 and va.knockout_flag_mask("nmd1+nmd2") == 48 and va.knockout_flag_mask(["first", "unknown"]) == 65
    assert va.knockout_flag_mask(5) == 5
    with pytest.raises(ValueError):
        va.knockout_flag_mask("nmd3")
    # the rule of min_cut_frac= / max_cut_frac=: ceil for a lower bound, floor for an upper one, of 65536 x share, capped
    assert [va.knockout_cut_frac(x) for x in (0.0, 0.05, 0.5, 1.0)] == [0, 3277, 32768, 65535]
    assert [va.knockout_cut_frac(x, upper=True) for x in (0.0, 0.65, 0.5, 1.0)] == [0, 42598, 32768, 65535]
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError):
            va.knockout_cut_frac(bad)
    args = va.Genome._knockout_args
    assert args(None, None, None, None, None, None, None, 23) is None
    for bad in (dict(cds=1), dict(min_frac=0.1), dict(require="nmd1")):
        with pytest.raises(ValueError):
            kw = dict(shape=None, cds=None, min_frac=None, max_frac=None, min_edge=None, require=None, forbid=None, site_len=23)
            kw.update(bad)
            args(**kw)
    with pytest.raises(ValueError):
        args("SpCas9", None, None, None, None, None, None, 23)  # no Cds
    with pytest.raises(ValueError):
        args("Cas9", None, None, None, None, None, None, 23)  # no such preset


def test_the_keywords_reach_the_limits(small):
    args = va.Genome._knockout_args
    shape, cds, code, limits = args("SpCas9", small["cds"], 0.05, 0.65, 3, "nmd1+nmd2", ["unknown"], 23)
    assert shape is va.KNOCKOUT_SHAPES["SpCas9"] and cds is small["cds"] and code is None and limits == (3277, 42598, 3, 48, 64)
    assert args("SpCas9", small["cds"], None, None, None, None, None, 23)[3] is None
    assert args("SpCas9", small["cds"], None, None, 7, None, None, 23)[3] == (0, 65535, 7, 0, 0)
    for bad in (dict(min_frac=0.7, max_frac=0.2), dict(min_edge=256), dict(require=128), dict(site_len=20)):
        kw = dict(shape="SpCas9", cds=small["cds"], min_frac=None, max_frac=None, min_edge=None, require=None, forbid=None, site_len=23)
        kw.update(bad)
        with pytest.raises(ValueError):
            args(**kw)


def test_unpack_and_the_pick_column_against_hand_made_words():
    rows = np.array([
        [3, 7 | 2 << 30, 1000 | 9 << 16 | (1 | 4 | 8 | 16 | 32) << 24, 5 | 12 << 16],   # NMD in both frames, frac 1000
        [3, 8 | 1 << 30, 900 | 255 << 16 | (2 | 4 | 16) << 24, 0 | 0xFFFF << 16],        # NMD1 alone, frac 900: END in frame +2
        [0, 0, 0 | 0 << 16 | 64 << 24, 0xFFFD | 0xFFFE << 16],                           # unknown and CAP at the very start
        [0xFFFFFFFF, 0, 0x80000000, 0],                                                  # a junction
        [0xFFFFFFFF, 0, 0, 0],                                                           # non-coding
        [kc.UNDEF] * 4,                                                                  # undefined
        [5, 100, 65535 | 1 << 16 | 48 << 24, 1 | 1 << 16],                               # NMD in both frames at the very end
    ], dtype=np.uint32)
    u = va.unpack_knockout_row(rows)
    assert u.dtype == va.KNOCKOUT_ROW_DTYPE
    assert u["transcript"].tolist() == [3, 3, 0, 0, 0, 0, 5] and u["codon"].tolist() == [7, 8, 0, 0, 0, 0, 100]
    assert u["frame"].tolist() == [2, 1, 0, 0, 0, 0, 0] and u["frac"].tolist() == [1000, 900, 0, 0, 0, 0, 65535]
    assert u["edge"].tolist() == [9, 255, 0, 0, 0, 0, 1] and u["flags"].tolist() == [61, 22, 64, 128, 0, 0, 48]
    assert u["d1"].tolist() == [5, 0, 0xFFFD, 0, 0, 0, 1] and u["d2"].tolist() == [12, 0xFFFF, 0xFFFE, 0, 0, 0, 1]
    assert u["coding"].tolist() == [True, True, True, False, False, False, True]
    assert u["defined"].tolist() == [True, True, True, True, True, False, True]
    assert va.unpack_knockout_row(rows[0])["codon"].tolist() == [7]
    col = va.pick_column("knockout", rows)
    assert col.dtype == np.uint64 and va.PICK_COLUMNS["knockout"] == 17
    assert col.tolist() == [65536 + 64535, 64635, 65535, 0, 0, 0, 65536] == kc.pick_column(rows).tolist()
    # NMD in both frames beats every frac; among equals the smaller frac wins
    assert col[6] > col[1] and col[0] > col[6] and col[2] > col[1]
    for row in rows:
        assert kc.keep(row, (0, 65535, 0, 0, 0)) == (int(row[0]) != 0xFFFFFFFF)
    assert kc.keep(rows[0], (1000, 1000, 9, 48, 64 | 2)) and not kc.keep(rows[0], (1001, 65535, 0, 0, 0))
    assert not kc.keep(rows[0], (0, 65535, 10, 0, 0)) and not kc.keep(rows[1], (0, 65535, 0, 48, 0)) and not kc.keep(rows[0], (0, 65535, 0, 0, 1))


def test_knockout_check_builds_and_runs_clean(tmp_path):
    """tools/knockout_check.cpp: g++ with ASan and UBSan where the compiler has them, plain otherwise; the run is on the CPU."""
    gxx = shutil.which("g++") or shutil.which("c++")
    assert gxx, "no C++ compiler"
    exe = str(tmp_path / "knockout_check")
    base = [gxx, "-O1", "-g", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "varscot_amd", "csrc")]
    tail = [os.path.join(ROOT, "tools", "knockout_check.cpp"), "-o", exe]
    build = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + tail, capture_output=True, text=True,
                           timeout=600)
    if build.returncode != 0:  # (a compiler without the sanitizers' runtimes)
        build = subprocess.run(base + tail, capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and run.stdout.startswith("ok: ") and "runtime error" not in run.stderr and "ERROR" not in run.stderr, \
        (run.returncode, run.stdout, run.stderr)


def _run(tool, *args):
    return subprocess.run([os.path.join(BIN, tool)] + [str(a) for a in args], capture_output=True, text=True, timeout=120,
                          env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))


def test_the_tools_refuse_before_a_device_is_opened(tmp_path):
    cds = tmp_path / "cds.bed"
    gs = ("guide_summary", "-G", tmp_path / "g.fa", "-I", tmp_path / "idx", "-M", "2", "-O", tmp_path / "o.tsv")
    ps = ("pattern_search", "-i", tmp_path / "idx", "-q", "TTTV" + "N" * 23, "-M", "2", "-O", tmp_path / "o.tsv")
    e_gs, e_ps = ("-E", tmp_path / "t.bed"), ("-E", tmp_path / "e.tsv", "-p", "4,23")
    cases = []
    for tool, e, last in ((gs, e_gs, 22), (ps, e_ps, 26)):
        k = (*tool, *e, "--knockout", "--knockout-cds", cds)
        cases += [
            ((*tool, *e, "--knockout-cds", cds), "give --knockout"), ((*tool, *e, "--knockout-nmd", "50"), "give --knockout"),
            ((*tool, *e, "--knockout-filter", "5,65"), "give --knockout"), ((*tool, *e, "--knockout-out", tmp_path / "x.tsv"), "give --knockout"),
            ((*tool, *e, "--knockout"), "give --knockout-cds"), ((*tool, *e, "--knockout", "17"), "give --knockout-cds"),
            ((*tool, "-R", tmp_path / "g.fa", "--knockout", "--knockout-cds", cds), "give -E"), ((*k, "-D", "0,1"), "one device"),
            ((*tool, *e, "--knockout", "0", "--knockout-cds", cds), "cut of 1 .. %d" % last),
            ((*tool, *e, "--knockout", last + 1, "--knockout-cds", cds), "cut of 1 .. %d" % last),
            ((*tool, *e, "--knockout=x", "--knockout-cds", cds), "cut of 1 .. %d" % last),
            ((*k, "--knockout-nmd", "65536"), "WINDOW[,START]"), ((*k, "--knockout-nmd", "50,65536"), "WINDOW[,START]"),
            ((*k, "--knockout-nmd", "50,"), "WINDOW[,START]"), ((*k, "--knockout-nmd", "x"), "WINDOW[,START]"),
            ((*k, "--knockout-filter", "5"), "MINPCT,MAXPCT"), ((*k, "--knockout-filter", "70,20"), "MINPCT,MAXPCT"),
            ((*k, "--knockout-filter", "5,101"), "MINPCT,MAXPCT"), ((*k, "--knockout-filter", "5,65,256"), "MINPCT,MAXPCT"),
            ((*k, "--knockout-filter", "5,65,3,nmd3"), "MINPCT,MAXPCT"), ((*k, "--knockout-filter", "5,65,3,nmd1/first+x"), "MINPCT,MAXPCT"),
            ((*k, "--knockout-filter", "5,65,3,/"), "MINPCT,MAXPCT"), ((*k, "--knockout-filter", "5,65,3,nmd1,x"), "MINPCT,MAXPCT"),
            ((*k, "--knockout-filter", "-5,65"), "MINPCT,MAXPCT"),
        ]
    cases.append(((*ps[:4], "N" * 18 + "GG", *ps[5:], "-E", tmp_path / "e.tsv", "-p", "0,18", "--knockout", "--knockout-cds", cds), "give --knockout CUT for 20"))
    for args, text in cases:
        r = _run(*args)
        assert r.returncode == 1 and text in r.stderr and "ERROR" not in r.stderr, (args, r.stderr)
    for tool in ("guide_summary", "pattern_search"):
        r = _run(tool, "--help")
        assert r.returncode == 0 and all(o in r.stdout for o in ("--knockout [ARG]", "--knockout-cds", "--knockout-nmd", "--knockout-filter", "--knockout-out"))
