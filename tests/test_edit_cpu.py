"""The host side of the base-editor windows (vsc_edit_site_text, the shape, the presets, the wrapper's target sorting,
edit_pick_inputs, the stand-alone check program): the library's plane form against the strings of tests/edit_cases.py, as
integers.  No device is needed."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import edit_cases as ed
import varscot_amd as va
from helpers import random_seq
from varscot_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def mask_of(text, start, length, base):
    return ed.number(j for j in range(length) if text[start + j].upper() == base)


@pytest.mark.parametrize("site_len", [16, 23, 32])
def test_site_text_equals_the_letters(site_len):
    rng = np.random.default_rng([28, 1, site_len])
    windows = [(0, 1), (0, 16), (site_len - 1, 1), (site_len - 16, 16), (3, 5), (3, 4), (site_len - 5, 5)]
    seen = set()
    for start, length in windows:
        for base in "ACGT":
            shape = va.EditShape(site_len, (start, length), base)
            texts = [random_seq(rng, site_len) for _ in range(12)] + [base * site_len, "ACGT"[("ACGT".index(base) + 1) % 4] * site_len]
            for text in texts:
                want = mask_of(text, start, length, base)
                seen.add(want)
                assert va.edit_site_text(text, shape) == want, (text, shape)
                assert va.edit_site_text(text.lower(), shape) == want
                mixed = "".join(ch.lower() if rng.integers(0, 2) else ch for ch in text)
                assert va.edit_site_text(mixed.encode(), shape) == want
                assert want < 2 ** length
    assert 0 in seen and 0xFFFF in seen and 1 in seen
    # the base by its number
    assert va.edit_site_text("A" * site_len, va.EditShape(site_len, (0, 3), 0)) == 7
    assert va.edit_site_text("T" * site_len, va.EditShape(site_len, (0, 3), 3)) == 7


def test_site_text_refuses_other_letters_and_lengths():
    shape = va.EditShape()
    text = "ACGTACGTACGTACGTACGTAGG"
    assert va.edit_site_text(text, shape) == mask_of(text, 3, 5, "C")
    for ch in "NnRY-*":
        for at in (0, 4, 22):  # inside the window or not: a site with another letter is no site
            with pytest.raises(va.VarscotError):
                va.edit_site_text(text[:at] + ch + text[at + 1:], shape)
    for bad in (text[:-1], text + "A", ""):
        with pytest.raises(va.VarscotError):
            va.edit_site_text(bad, shape)
    L = va.lib()
    m = C.c_uint32()
    st = shape._struct()
    assert L.vsc_edit_site_text(None, C.byref(st), C.byref(m)) == -22
    assert L.vsc_edit_site_text(text.encode(), None, C.byref(m)) == -22
    assert L.vsc_edit_site_text(text.encode(), C.byref(st), None) == -22
    assert va.EDIT_UNDEFINED == 0xFFFFFFFF


def test_shape_refusals():
    for kw in ({"site_len": 15}, {"site_len": 33}, {"window": (3, 0)}, {"window": (3, 17)}, {"window": (19, 5)}, {"window": (24, 1)},
               {"window": (-1, 5)}, {"base": 4}, {"base": -1}, {"base": "N"}, {"base": "AC"}, {"site_len": 16, "window": (1, 16)}):
        with pytest.raises(ValueError):
            va.EditShape(**kw)
    for kw in ({"window": (0, 1)}, {"window": (22, 1)}, {"window": (7, 16)}, {"site_len": 16, "window": (0, 16)},
               {"site_len": 32, "window": (16, 16)}, {"base": "t"}, {"base": b"G"}, {"base": 2}):
        s = va.EditShape(**kw)._struct()
        assert C.sizeof(s) == 32 and list(s.reserved) == [0, 0, 0, 0]
    # every shape refusal, by the library
    L = va.lib()
    m = C.c_uint32()
    for bad in ((15, (3, 5), 1), (33, (3, 5), 1), (23, (3, 0), 1), (23, (3, 17), 1), (23, (19, 5), 1), (23, (24, 1), 1), (23, (3, 5), 4),
                (23, (0xFFFFFFFF, 2), 1), (23, (3, 0xFFFFFFFF), 1), (23, (3, 5), 0xFFFFFFFF)):
        st = va.EditShape(*bad, validate=False)._struct()
        text = b"A" * (bad[0] if bad[0] < 64 else 23)
        assert L.vsc_edit_site_text(text, C.byref(st), C.byref(m)) == -22, bad
    for k in range(4):
        st = va.EditShape()._struct()
        st.reserved[k] = 1
        assert L.vsc_edit_site_text(b"A" * 23, C.byref(st), C.byref(m)) == -22


def test_struct_sizes():
    assert C.sizeof(_lib.EditShapeStruct) == 32 and C.sizeof(_lib.EditStats) == 96
    assert va.EDIT_PAIR_DTYPE.itemsize == 16 and va.EDIT_PAIR_DTYPE.names == ("candidate", "target", "mask", "info")
    assert va.EDIT_TARGET_DTYPE.itemsize == 8
    at, by = va.unpack_edit_info(np.array([4 | 3 << 8, 15 | 15 << 8, 0], dtype=np.uint32))
    assert at.tolist() == [4, 15, 0] and by.tolist() == [3, 15, 0]
    header = open(os.path.join(ROOT, "include", "varscot_hip.h")).read()
    assert "#define VSC_ABI_VERSION 5" in header and "#define VSC_EDIT_UNDEFINED 0xFFFFFFFFu" in header


def test_presets():
    assert set(va.EDITORS) == {"CBE", "ABE"}
    cbe, abe = va.EDITORS["CBE"], va.EDITORS["ABE"]
    assert (cbe.site_len, cbe.window, cbe.base) == (23, (3, 5), 1) and (abe.site_len, abe.window, abe.base) == (23, (3, 4), 0)
    site = "GGGCACCAAGGGGGGGGGGGTGG"  # protospacer positions 4 .. 8 are C A C C A
    assert va.edit_site_text(site, cbe) == ed.number([0, 2, 3]) and va.edit_site_text(site, abe) == ed.number([1])
    assert repr(cbe) == "EditShape(site_len=23, window=(3, 5), base='C')"


def test_targets_are_sorted_and_numbered_in_the_callers_order():
    given = [(2, 9), (0, 5), (2, 9), (1, 0), (0, 5), (0, 4), (2, 9)]
    tg, order, inverse = va.edit_targets(given)
    assert tg.dtype == va.EDIT_TARGET_DTYPE and [(int(c), int(p)) for c, p in zip(tg["contig"], tg["pos"])] == sorted(set(given))
    assert order.tolist() == [given.index(t) for t in sorted(set(given))]  # of duplicates the first
    assert [sorted(set(given))[k] for k in inverse] == given
    arr = np.zeros(len(given), dtype=va.EDIT_TARGET_DTYPE)
    arr["contig"], arr["pos"] = [c for c, _ in given], [p for _, p in given]
    tg2, order2, inverse2 = va.edit_targets(arr)
    assert tg2.tobytes() == tg.tobytes() and order2.tolist() == order.tolist() and inverse2.tolist() == inverse.tolist()
    tg, order, inverse = va.edit_targets([])
    assert len(tg) == 0 and len(order) == 0 and len(inverse) == 0
    big = [(0xFFFFFFFF, 0xFFFFFFFF), (0, 0xFFFFFFFF), (0xFFFFFFFF, 0)]
    assert va.edit_targets(big)[1].tolist() == [1, 2, 0]
    for bad in ([(-1, 0)], [(0, 2 ** 32)]):
        with pytest.raises(ValueError):
            va.edit_targets(bad)


def test_pick_inputs_against_a_key_made_by_hand():
    loci = ed.locus_array([(0, 10, 0), (0, 11, 1), (1, 5, 0), (1, 9, 1)])
    pairs = np.zeros(5, dtype=va.EDIT_PAIR_DTYPE)
    #                candidate, target, mask, at | bystanders << 8
    for k, row in enumerate([(0, 2, 0b00101, 0 | 1 << 8), (0, 3, 0b00101, 2 | 1 << 8), (2, 2, 0b00001, 0), (3, 0, 0xFFFF, 7 | 15 << 8),
                             (3, 3, 0xFFFF, 9 | 15 << 8)]):
        pairs[k] = row
    got_loci, target, key = va.edit_pick_inputs(pairs, loci)
    assert got_loci.tobytes() == loci[[0, 0, 2, 3, 3]].tobytes() and target.dtype == np.uint32 and target.tolist() == [2, 3, 2, 0, 3]
    assert key.dtype == np.uint64 and key.tolist() == [14, 14, 15, 0, 0]  # fewer bystanders: the larger key
    spec = np.array([700, 9999, 5, 20000], dtype=np.uint64)  # per candidate of the edit call; 14 bits
    _, _, key = va.edit_pick_inputs(pairs, loci, extra_columns=[(spec, 14)])
    assert key.tolist() == [14 << 14 | 700, 14 << 14 | 700, 15 << 14 | 5, 16383, 16383]  # (clipped to its bits, as pick_key clips)
    assert va.edit_pick_inputs(pairs[:0], loci)[2].shape == (0,)
    with pytest.raises(ValueError):
        va.edit_pick_inputs(pairs, loci, extra_columns=[(spec[:3], 14)])
    with pytest.raises(ValueError):
        va.edit_pick_inputs(pairs, loci, extra_columns=[(spec.astype(np.float64), 14)])


def test_python_bounds_and_targets_need_the_shape():
    f = va.Genome._edit_args
    shape = va.EditShape()
    assert f(None, None, None, None, 23) is None
    assert f(shape, None, None, None, 23) == (shape, None, None, None, None)
    assert f("CBE", None, 1, None, 23)[0] is va.EDITORS["CBE"] and f("CBE", None, 1, None, 23)[4] == (1, 16)
    got = f(shape, [(1, 2), (0, 3)], None, 2, 23)
    assert got[1]["pos"].tolist() == [3, 2] and got[2].tolist() == [1, 0] and got[4] == (0, 2)
    for bad in ((None, [(0, 1)], None, None), (None, None, 1, None), (None, None, None, 3), (shape, None, 3, 2), (shape, None, -1, None),
                ("BE9", None, None, None), (7, None, None, None)):
        with pytest.raises(ValueError):
            f(*bad, 23)
    with pytest.raises(ValueError):
        f(va.EditShape(site_len=27), None, None, None, 23)


def test_the_restatement_on_the_small_genome():
    """What tests/test_edit.py relies on, on the restatement alone: the counts a restatement of this kind gave when the fixture
    was designed (contigs of 22, 23, 24, 700 and 500 bases), and the planted cases."""
    contigs = ed.small_genome()
    assert [len(c) for c in contigs] == [22, 23, 24, 700, 500]
    loci = ed.every_locus(contigs)
    third = ed.target_sets(contigs)["third"]
    narrow = ed.expected(contigs, loci, (23, 3, 5, "C"), third)
    wide = ed.expected(contigs, loci, (23, 0, 16, "C"), third)
    assert narrow["stats"]["pairs"] >= 50 and wide["stats"]["pairs"] > narrow["stats"]["pairs"]
    assert (wide["rows"][:, 0] == 0xFFFF).any() and (wide["rows"][:, 0] == 0).any()
    assert narrow["stats"]["off_contig"] == 0 and narrow["stats"]["defined"] + narrow["stats"]["invalid"] + narrow["stats"]["has_n"] == len(loci)


def test_the_stand_alone_check_builds_and_runs_clean(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "edit_check")
    build = subprocess.run([hipcc, "--offload-arch=gfx950", "-x", "hip", "-O1", "-g", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                            "-I" + os.path.join(ROOT, "varscot_amd", "csrc"), "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                            "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tools", "edit_check.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and run.stdout.startswith("ok: ") and "runtime error" not in run.stderr and "ERROR" not in run.stderr, \
        (run.returncode, run.stdout, run.stderr)
