"""Coding consequences of base edits, the parts that need no device: the genetic code, vsc_codon_effect against the class rules,
vsc_effects_site_text - the functions the kernels call, run on the host - against the restatement on strings
(tests/effects_cases.py) over every locus of the small genome, every refusal of vsc_cds_build, the struct sizes, the pick key and
the stand-alone check under the sanitizers.  Integers only, no tolerance."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import effects_cases as fx
import varscot_amd as va
from varscot_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (site_len, win_start, win_len, from, to): CBE and ABE, a 1-base and a 16-base window, site_len 16, 23 and 32
SHAPES = [(23, 3, 5, "C", "T"), (23, 3, 4, "A", "G"), (23, 10, 1, "C", "T"), (23, 10, 1, "A", "G"), (23, 7, 16, "C", "T"),
          (23, 0, 16, "A", "G"), (16, 0, 16, "C", "T"), (16, 5, 1, "A", "G"), (32, 16, 16, "A", "G"), (32, 3, 5, "C", "T"),
          (23, 3, 5, "C", "G")]


def shape_of(t):
    return va.EditShape(site_len=t[0], window=(t[1], t[2]), base=t[3])


@pytest.fixture(scope="module")
def small():
    contigs, segments = fx.small_genome()
    packed = va.PackedGenome.from_sequences(list(contigs))
    cds = va.Cds(packed, segments, n_tx=fx.N_TX)
    yield {"contigs": contigs, "segments": segments, "packed": packed, "cds": cds}
    cds.close()


def test_the_code_is_the_standard_code():
    assert va.GENETIC_CODE == fx.code_string(fx.STANDARD) and len(va.GENETIC_CODE) == 64
    header = open(os.path.join(ROOT, "include", "varscot_hip.h")).read()
    assert va.GENETIC_CODE in header
    assert va.EFFECT_CLASSES == fx.EFFECTS
    mito = fx.code_string(fx.MITO)
    assert mito != va.GENETIC_CODE and mito.count("*") == 4


@pytest.mark.parametrize("code", [None, "mito"])
def test_codon_effect_against_the_class_rules(code):
    by_aa = fx.MITO if code else fx.STANDARD
    table = fx.aa_table(by_aa)
    text = fx.code_string(by_aa).encode() if code else None
    L = va.lib()
    out = C.c_uint32()
    codons = [a + b + c for a in "ACGT" for b in "ACGT" for c in "ACGT"]
    seen = set()
    for r, ref in enumerate(codons):
        for a, alt in enumerate(codons):
            for codon in (0, 1):
                for phase in (0, 1, 2):
                    assert L.vsc_codon_effect(r, a, codon, phase, text, C.byref(out)) == 0
                    want = fx.EFFECTS.index(fx.classify(ref, alt, codon, phase, table))
                    assert out.value == want, (ref, alt, codon, phase)
                    seen.add(want)
    assert seen == {0, 1, 2, 3, 4}  # (unknown needs a codon without letters)
    assert va.codon_effect("CAA", "TAA", 7, 0) == 2 and va.codon_effect("TGG", "TGA", 1, 2) == 2 and va.codon_effect("TAA", "CAA", 3, 0) == 3
    for bad in ((64, 0, 0, 0), (0, 64, 0, 0), (0, 0, 0, 3)):
        assert L.vsc_codon_effect(*bad, None, C.byref(out)) == -22
    assert L.vsc_codon_effect(0, 0, 0, 0, b"ACDEF", C.byref(out)) == -22 and L.vsc_codon_effect(0, 0, 0, 0, None, None) == -22


@pytest.mark.parametrize("shape", SHAPES, ids=lambda t: "%d-%d-%d-%s%s" % t)
def test_site_text_against_the_restatement(small, shape):
    contigs, segments, cds = small["contigs"], small["segments"], small["cds"]
    loci = fx.every_locus(contigs) + fx.invalid_loci(contigs)
    raw = fx.raw_effects(contigs, segments, loci, shape[:4], shape[4])
    sh = shape_of(shape)
    for code in (None, fx.MITO):
        want = fx.expected(contigs, segments, loci, shape[:4], shape[4], code or fx.STANDARD, raw=raw)
        text = fx.code_string(code) if code else None
        at = 0
        per = np.bincount(want["effects"]["candidate"], minlength=len(loci))
        for i, locus in enumerate(loci):
            row, effects = va.effects_site_text(cds, contigs, locus[0], locus[1], locus[2], sh, shape[4], code=text)
            assert row.tolist() == want["rows"][i].tolist(), (locus, row)
            assert len(effects) == per[i] and (effects["candidate"] == 0).all(), locus
            mine = want["effects"][at:at + per[i]]
            for f in ("transcript", "codon", "info"):
                assert effects[f].tolist() == mine[f].tolist(), (locus, f)
            at += per[i]
        assert at == len(want["effects"])
    assert want["stats"]["effects"] > 0


def test_the_small_genome_holds_what_it_is_for(small):
    """A condition on the inputs, asserted on the restatement: every class occurs, and a split codon is emitted by a base of
    each frame in transcripts of both strands."""
    contigs, segments = small["contigs"], small["segments"]
    loci = fx.every_locus(contigs)
    classes, frames = set(), set()
    for shape in SHAPES:
        raw = fx.raw_effects(contigs, segments, loci, shape[:4], shape[4])
        want = fx.expected(contigs, segments, loci, shape[:4], shape[4], raw=raw)
        classes |= {k for k, v in want["stats"]["by_class"].items() if v}
        frames |= fx.split_frames(contigs, segments, raw)
    assert classes == set(fx.EFFECTS)
    assert frames == {(strand, f) for strand in (0, 1) for f in (0, 1, 2)}


def test_site_text_refusals(small):
    cds, contigs = small["cds"], small["contigs"]
    sh = va.EditShape()
    with pytest.raises(va.VarscotError):
        va.effects_site_text(cds, contigs, 0, 0, 0, sh, "C")  # to == from
    with pytest.raises(va.VarscotError):
        va.effects_site_text(cds, contigs, 0, 0, 0, sh, 4)
    with pytest.raises(va.VarscotError):
        va.effects_site_text(cds, contigs, 0, 0, 0, va.EditShape(23, (20, 5), "C", validate=False), "T")
    row, effects = va.effects_site_text(cds, contigs, 0, len(contigs[0]), 0, sh, "T")  # a site that leaves its contig
    assert row.tolist() == [fx.UNDEF, fx.UNDEF] and len(effects) == 0


def segment_array(rows):
    a = np.zeros(len(rows), dtype=_lib.CDS_SEGMENT_DTYPE)
    for i, r in enumerate(rows):
        a[i] = tuple(r) + ((0, 0),)
    return a


def test_every_refusal_of_cds_build(small):
    packed = small["packed"]
    L = va.lib()
    contigs = np.ascontiguousarray(packed.contigs, dtype=va.api.CONTIG_DTYPE)
    length = len(small["contigs"][0])

    def build(rows, n_tx=4, reserved=None):
        a = segment_array(rows)
        if reserved is not None:
            a["reserved"][reserved] = 1
        h = C.c_void_p()
        rc = L.vsc_cds_build(_lib.ptr(contigs), len(contigs), _lib.ptr(a), len(a), n_tx, C.byref(h))
        if rc == 0:
            L.vsc_cds_free(h)
        else:
            assert not h.value
        return rc, L.vsc_cds_build_error().decode()

    ok = [(0, 10, 16, 0, 0, 0), (0, 20, 26, 0, 0, 0), (1, 5, 11, 1, 1, 0)]
    assert build(ok) == (0, "")
    cases = [
        ([(0, 10, 16, 0, 0, 0), (0, 15, 21, 1, 0, 0)], "overlaps", 1),
        ([(0, 20, 26, 0, 0, 0), (0, 10, 16, 1, 0, 0)], "ascending", 1),
        ([(1, 5, 11, 1, 1, 0), (0, 10, 16, 0, 0, 0)], "ascending", 1),
        ([(0, 10, 16, 0, 0, 0), (0, 10, 16, 1, 0, 0)], "ascending", 1),
        ([(0, 10, 16, 0, 0, 0), (0, 20, 26, 0, 1, 0)], "two strands", 1),
        ([(0, 10, 16, 0, 0, 0), (1, 20, 26, 0, 0, 0)], "two contigs", 1),
        ([(0, 10, 16, 0, 0, 0), (0, 20, 26, 0, 0, 1)], "phase", 1),
        ([(0, 10, 16, 0, 1, 0), (0, 20, 27, 0, 1, 0)], "phase", 0),  # on '-' the LATER segment comes first
        ([(0, 10, 16, 0, 0, 0), (0, 20, 20, 1, 0, 0)], "empty", 1),
        ([(0, 10, 16, 0, 0, 0), (0, 30, 20, 1, 0, 0)], "empty", 1),
        ([(0, length - 3, length + 1, 0, 0, 0)], "beyond", 0),
        ([(0, 10, 16, 4, 0, 0)], "n_tx", 0),
        ([(len(contigs), 10, 16, 0, 0, 0)], "unknown contig", 0),
        ([(0, 10, 16, 0, 2, 0)], "strand", 0),
        ([(0, 10, 16, 0, 0, 3)], "strand", 0),
    ]
    for rows, word, segment in cases:
        rc, text = build(rows)
        assert rc == -22 and word in text and "segment %d:" % segment in text, (rows, text)
    rc, text = build(ok, reserved=1)
    assert rc == -22 and "reserved" in text
    # consistent phases pass: 7 bases, then phase 2; on '-' from the far end
    assert build([(0, 10, 17, 0, 0, 0), (0, 20, 26, 0, 0, 2)])[0] == 0
    assert build([(0, 10, 16, 0, 1, 2), (0, 20, 27, 0, 1, 0)])[0] == 0
    assert build([(0, 10, 16, 0, 0, 1), (0, 20, 26, 0, 0, 1)])[0] == 0  # first phase 1: shift 2, 6 bases, (3 - 8 % 3) % 3 = 1
    h = C.c_void_p()
    assert L.vsc_cds_build(_lib.ptr(contigs), len(contigs), None, 1, 1, C.byref(h)) == -22 and L.vsc_cds_build(None, 0, None, 0, 0, None) == -22
    assert L.vsc_cds_build(_lib.ptr(contigs), len(contigs), _lib.ptr(segment_array(ok)), 0xFFFFFFFF, 4, C.byref(h)) == -34
    assert L.vsc_cds_build(None, 0, None, 0, 0, C.byref(h)) == 0  # an empty set is a set
    st = _lib.CdsStats()
    assert L.vsc_cds_info(h, C.byref(st)) == 0 and st.segments == 0 and L.vsc_cds_info(None, C.byref(st)) == -22
    L.vsc_cds_free(h)
    with pytest.raises(va.VarscotError) as e:
        va.Cds(packed, [(0, 10, 16, 0, "+", 0), (0, 12, 21, 1, "+", 0)])
    assert "overlaps" in str(e.value)
    info = small["cds"].info()
    assert info == {"segments": len(small["segments"]), "transcripts": fx.N_TX, "transcripts_used": 10,
                    "coding_bases": sum(e - s for _, s, e, *_ in small["segments"])}
    unsorted = va.Cds(packed, list(small["segments"])[::-1], n_tx=fx.N_TX)  # the wrapper sorts
    assert unsorted.info() == info
    unsorted.close()


def test_struct_sizes():
    header = open(os.path.join(ROOT, "include", "varscot_hip.h")).read()
    m = re.search(r"sizeof\(vsc_cds_segment\) == (\d+) && sizeof\(vsc_cds_stats\) == (\d+) && sizeof\(vsc_effect\) == (\d+) && "
                  r"sizeof\(vsc_effects_stats\) == (\d+)", header)
    assert [int(x) for x in m.groups()] == [_lib.CDS_SEGMENT_DTYPE.itemsize, C.sizeof(_lib.CdsStats), va.EFFECT_DTYPE.itemsize,
                                            C.sizeof(_lib.EffectsStats)] == [32, 64, 16, 128]
    assert int(re.search(r"#define\s+VSC_ABI_VERSION\s+(\d+)", header).group(1)) == 5


def test_unpack_and_pick_inputs_against_a_hand_made_key():
    info = np.array([16 | 48 << 6 | 2 << 12 | 1 << 16 | 3 << 20, 0 | 0 << 6 | 5 << 12 | 2 << 16 | 15 << 20], dtype=np.uint32)
    ref, alt, cls, edited, at = va.unpack_effect_info(info)
    assert (ref.tolist(), alt.tolist(), cls.tolist(), edited.tolist(), at.tolist()) == ([16, 0], [48, 0], [2, 5], [1, 2], [3, 15])
    assert va.codon_text(16) == "CAA" and va.codon_text(48) == "TAA" and va.codon_text(63) == "TTT"
    counts, coding = va.unpack_effect_row(np.array([[1 | 2 << 5 | 3 << 10 | 1 << 25, 5], [fx.UNDEF, fx.UNDEF]], dtype=np.uint32))
    assert counts.tolist() == [[1, 2, 3, 0, 0, 1], [0] * 6] and coding.tolist() == [5, 0]
    effects = np.zeros(5, dtype=va.EFFECT_DTYPE)
    effects["candidate"] = [0, 0, 2, 3, 3]
    effects["transcript"] = [4, 5, 4, 4, 6]
    effects["codon"] = [7, 0, 2, 2, 9]
    effects["info"] = [2 << 12, 1 << 12, 2 << 12, 0 << 12, 2 << 12]  # stop_gained, missense, stop_gained, synonymous, stop_gained
    loci = np.zeros(4, dtype=va.LOCUS_DTYPE)
    loci["pos"] = [100, 200, 300, 400]
    spec = np.array([9, 8, 7, 6], dtype=np.uint64)
    p_loci, target, key = va.effects_pick_inputs(effects, loci, extra_columns=[(spec, 14)])
    assert p_loci["pos"].tolist() == [100, 300, 400] and target.tolist() == [4, 4, 6] and target.dtype == np.uint32
    top = 2 ** 31 - 1
    assert key.tolist() == [(top - 7) << 14 | 9, (top - 2) << 14 | 7, (top - 9) << 14 | 6] and key.dtype == np.uint64
    assert key[1] > key[0]  # the earlier codon is the better pick
    _, target, key = va.effects_pick_inputs(effects, loci, classes=("missense", "synonymous"))
    assert target.tolist() == [5, 4] and key.tolist() == [top, top - 2]
    assert va.effect_class_mask("stop_gained+missense") == 6 and va.effect_class_mask(None) == 0
    with pytest.raises(ValueError):
        va.effect_class_mask(["nonsense"])
    assert va.EDITOR_TO == {"CBE": "T", "ABE": "G"} and set(va.EDITORS) == {"CBE", "ABE"}


def test_effects_check_builds_and_runs_clean(tmp_path):
    exe = str(tmp_path / "effects_check")
    cmd = [shutil.which("hipcc") or "/opt/rocm/bin/hipcc", "-x", "hip", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "varscot_amd", "csrc"),
           os.path.join(ROOT, "tools", "effects_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "effects_check: ok" in r.stdout and "ERROR" not in r.stderr, r.stdout + r.stderr
