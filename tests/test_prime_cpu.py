"""The host side of the prime-editing extensions (vsc_prime_site_text, the shape, the preset, the wrapper's edit sorting,
prime_pick_inputs, the stand-alone check program): the library's plane form against the strings of tests/prime_cases.py, as
integers.  No device is needed."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import prime_cases as pc
import varscot_amd as va
from helpers import random_seq, revcomp
from varscot_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def read_edits(rng, C_, nick):
    """Edits in read coordinates (e0, del_len, ins): in front of the nick, at it, behind it, at and over the context's end."""
    out = [(nick, 1, "T"), (nick, 0, "A"), (nick, 1, ""), (nick - 1, 1, "G"), (0, 1, "C"), (C_, 0, "ACG"), (C_ - 1, 1, "A"), (C_ - 1, 1, ""),
           (max(C_ - 16, 0), min(16, C_), ""), (nick, 0, "ACGTACGTACGTACGT"), (nick, min(3, C_ - nick), "GG")]
    for _ in range(40):
        e0 = int(rng.integers(0, C_ + 1))
        del_len = int(rng.integers(0, min(16, C_ - e0) + 1))
        ins_len = int(rng.integers(0 if del_len else 1, 17))
        out.append((e0, del_len, random_seq(rng, ins_len)))
    return out


@pytest.mark.parametrize("name", sorted(pc.SHAPES))
def test_site_text_equals_the_letters(name):
    shape = pc.shape_of(name)
    C_, nick = shape.context_len, shape.nick
    rng = np.random.default_rng([30, 1, len(name), C_])
    texts = [random_seq(rng, C_) for _ in range(30)] + [b * C_ for b in "ACGT"] + ["GC" * 32, "AT" * 32, "AAAAC" * 13, "GGGGGGGT" * 8]
    seen = {"weak": set(), "exists": set(), "flags": set(), "lengthened": set(), "reasons": set()}
    for text in texts:
        text = text[:C_]
        pbs_len, pbs_gc, weak = pc.pbs_of(text, shape)
        word = pbs_len + 256 * pbs_gc + 65536 * weak
        seen["weak"].add(weak)
        assert va.prime_site_text(text, shape) == (word, False, 0, 0, ""), (name, text)
        assert va.prime_site_text(text.lower().encode(), shape)[0] == word
        for e0, del_len, ins in read_edits(rng, C_, nick):
            want = pc.pair_of(text, 0, 0, shape, (0, e0, del_len, ins), pbs_len, weak)
            mixed = "".join(ch.lower() if rng.integers(0, 2) else ch for ch in text)
            got = va.prime_site_text(mixed, shape, e0, del_len, ins.lower() if e0 % 2 else ins)
            if isinstance(want, str):
                seen["reasons"].add(want)
                assert got == (word, False, 0, 0, ""), (name, text, e0, del_len, ins, want)
                continue
            seen["exists"].add(True)
            seen["flags"].add(want["flags"])
            seen["lengthened"].add(want["lengthened"])
            info = want["t"] + 256 * want["d"] + 65536 * want["h"] + 2 ** 24 * want["flags"]
            ext = pbs_len + want["t"] + 256 * want["ext_gc"] + 65536 * pbs_len
            assert got == (word, True, info, ext, want["extension"]), (name, text, e0, del_len, ins, want)
            assert va.unpack_prime_info(info)[0] == want["t"] and int(va.unpack_prime_info(info)[3]) == want["flags"]
            assert tuple(int(v) for v in va.unpack_prime_ext(ext)) == (pbs_len + want["t"], want["ext_gc"], pbs_len)
            assert len(want["extension"]) == pbs_len + want["t"] and want["h"] >= shape.min_homology
    assert True in seen["exists"] and {"reach", "rtt_max"} <= seen["reasons"]
    if SHAPE_HAS_MODEL[name]:
        assert seen["weak"] == {False, True}
    if shape.flags & 1:
        assert seen["lengthened"] == {False, True} and "g_end" in seen["reasons"]
    else:
        assert seen["lengthened"] == {False}


SHAPE_HAS_MODEL = {k: "stability" in v for k, v in pc.SHAPES.items()}


def test_site_text_refuses_other_letters_lengths_and_edits():
    shape = va.PRIME_EDITORS["PE2"]
    text = random_seq(np.random.default_rng(5), 64)
    assert va.prime_site_text(text, shape, 20, 1, "A")[1] in (True, False)
    for ch in "NnRY-*":
        for at in (0, 16, 63):
            with pytest.raises(va.VarscotError):
                va.prime_site_text(text[:at] + ch + text[at + 1:], shape)
    for bad in (text[:-1], text + "A", ""):
        with pytest.raises(va.VarscotError):
            va.prime_site_text(bad, shape)
    for e0, del_len, ins in ((65, 0, "A"), (64, 1, ""), (60, 5, ""), (20, 17, ""), (20, 0, "A" * 17), (20, 0, ""), (20, 1, "N"), (0xFFFFFFFF, 1, "")):
        with pytest.raises(va.VarscotError):
            va.prime_site_text(text, shape, e0, del_len, ins)
    L = va.lib()
    row = (C.c_uint32 * 2)()
    st = shape._struct()
    assert L.vsc_prime_site_text(None, C.byref(st), 0, 0, None, row, None, None) == -22
    assert L.vsc_prime_site_text(text.encode(), None, 0, 0, None, row, None, None) == -22
    assert L.vsc_prime_site_text(text.encode(), C.byref(st), 0, 0, None, None, None, None) == -22
    assert L.vsc_prime_site_text(text.encode(), C.byref(st), 20, 1, b"A", row, None, None) == 0  # pair and extension are optional
    assert va.PRIME_UNDEFINED == 0xFFFFFFFF


GOOD = dict(site_len=23, down=41, nick=17, pbs=(13, 13), rtt=(10, 34), min_homology=5, pam=(21, 2), seed=(17, 3), avoid_g_end=True)
BAD_SHAPES = [{"site_len": 15}, {"site_len": 33}, {"down": 42}, {"site_len": 32, "down": 33}, {"nick": 0}, {"nick": 24}, {"pbs": (0, 13)},
              {"pbs": (14, 13)}, {"pbs": (13, 18)}, {"rtt": (0, 34)}, {"rtt": (35, 34)}, {"rtt": (10, 48)}, {"down": 20, "rtt": (10, 27)},
              {"min_homology": 35}, {"pam": (21, 3)}, {"pam": (10, 9)}, {"pam": (24, 0)}, {"seed": (16, 8)}, {"seed": (0, 9)}, {"avoid_g_end": 2},
              {"stability": (2 ** 20 + 1, (0,) * 4, (0,) * 16, 0)}, {"stability": (0, (0, 0, -2 ** 20 - 1, 0), (0,) * 16, 0)},
              {"stability": (0, (0,) * 4, (0,) * 15 + (2 ** 21,), 0)}, {"stability": (0, (0,) * 4, (0,) * 16, -2 ** 20 - 1)}]


def test_shape_refusals():
    L = va.lib()
    row = (C.c_uint32 * 2)()
    assert va.PrimeShape(**GOOD).valid()
    for kw in BAD_SHAPES:
        args = dict(GOOD, **kw)
        with pytest.raises(ValueError):
            va.PrimeShape(**args)
        st = va.PrimeShape(validate=False, **args)._struct()
        C_ = min(args["site_len"] + args["down"], 64)
        assert L.vsc_prime_site_text(b"A" * C_, C.byref(st), 0, 0, None, row, None, None) == -22, kw
    for kw in ({"stability": (2 ** 20, (-2 ** 20,) * 4, (2 ** 20,) * 16, -2 ** 20)}, {"pam": (23, 0)}, {"seed": (15, 8)}, {"down": 0, "rtt": (1, 6)},
               {"nick": 23, "pbs": (1, 23), "rtt": (1, 41)}, {"min_homology": 34}, {"min_homology": 0}):
        st = va.PrimeShape(**dict(GOOD, **kw))._struct()
        C_ = st.site_len + st.down
        assert C.sizeof(st) == 160 and list(st.reserved) == [0] * 5
        assert L.vsc_prime_site_text(b"A" * C_, C.byref(st), 0, 0, None, row, None, None) == 0, kw
    for k in range(5):
        st = va.PrimeShape(**GOOD)._struct()
        st.reserved[k] = 1
        assert L.vsc_prime_site_text(b"A" * 64, C.byref(st), 0, 0, None, row, None, None) == -22
    with pytest.raises(ValueError):
        va.PrimeShape(stability=(0, (0,) * 3, (0,) * 16, 0))


def test_struct_sizes():
    assert C.sizeof(_lib.PrimeShapeStruct) == 160 and C.sizeof(_lib.PrimeStats) == 128
    assert va.PRIME_PAIR_DTYPE.itemsize == 16 and va.PRIME_PAIR_DTYPE.names == ("candidate", "edit", "info", "ext")
    assert va.PRIME_EDIT_DTYPE.itemsize == 16 and va.PRIME_EDIT_DTYPE.names == ("contig", "pos", "del_len", "ins_len", "ins")
    t, d, h, flags = va.unpack_prime_info(np.array([12 | 3 << 8 | 8 << 16 | 5 << 24, 63 | 63 << 8 | 63 << 16 | 15 << 24, 0], dtype=np.uint32))
    assert t.tolist() == [12, 63, 0] and d.tolist() == [3, 63, 0] and h.tolist() == [8, 63, 0] and flags.tolist() == [5, 15, 0]
    assert [int(v) for v in va.unpack_prime_row(13 | 7 << 8 | 1 << 16)] == [13, 7, 1]
    assert va.PRIME_FLAGS == ("PAM", "SEED", "POLY_T", "WEAK")
    header = open(os.path.join(ROOT, "include", "varscot_hip.h")).read()
    assert "#define VSC_ABI_VERSION 5" in header and "#define VSC_PRIME_UNDEFINED 0xFFFFFFFFu" in header
    definition = header[header.index("prime-editing guide design"):]
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for line in definition.splitlines():  # the same normative text in the header and in DESIGN 4.30
        body = line.strip().lstrip("*").strip()
        if body.startswith(("SHAPE ", "CONTEXT ", "PBS ", "EDITS ", "READ ", "RTT ", "FLAGS ", "ROW ", "PAIR ", "COVERAGE ", "FILTER ", "EXTENSION ")):
            assert body in design, body


def test_the_preset():
    assert set(va.PRIME_EDITORS) == {"PE2"}
    s = va.PRIME_EDITORS["PE2"]
    assert (s.site_len, s.down, s.nick, s.pbs_min, s.pbs_max, s.rtt_min, s.rtt_max, s.min_homology) == (23, 41, 17, 13, 13, 10, 34, 5)
    assert (s.pam_start, s.pam_len, s.seed_start, s.seed_len, s.flags) == (21, 2, 17, 3, 1)
    assert (s.init, s.target, s.mono, s.di) == (0, 0, (0,) * 4, (0,) * 16) and s.context_len == 64 and s.valid()
    #       protospacer 0..16    | nick: 17..19, N, GG, then 41 bases behind the site
    text = "ACGTACGTACGTACGTA" + "CTT" + "AGG" + "ACGTTGCA" * 5 + "C"
    word, exists, info, ext, extension = va.prime_site_text(text, "PE2", 18, 1, "A")  # an SNV one base behind the nick
    assert word == 13 | 6 << 8 and exists
    t, d, h, flags = (int(v) for v in va.unpack_prime_info(info))
    assert (t, d, h, flags) == (10, 1, 8, pc.SEED)  # t = max(10, 1 + 1 + 5); the seed is read positions 17 .. 19
    edited = text[:18] + "A" + text[19:]
    assert extension == revcomp(edited[4:27]) and int(va.unpack_prime_ext(ext)[0]) == 23
    assert va.prime_site_text(text, "PE2", 21, 1, "C")[2] >> 24 == pc.PAM  # the first G of the PAM
    with pytest.raises(ValueError):
        va.prime_site_text(text, "PE9")


def test_edits_are_sorted_and_numbered_in_the_callers_order():
    given = [(2, 9, 1, "A"), (0, 5, 0, "ACG"), (1, 0, 3, ""), (0, 4, 16, "-"), (0, 6, 2, "T" * 16)]
    e, order, inverse = va.prime_edits(given)
    assert e.dtype == va.PRIME_EDIT_DTYPE
    assert [(int(c), int(p)) for c, p in zip(e["contig"], e["pos"])] == sorted((c, p) for c, p, _, _ in given)
    assert order.tolist() == [3, 1, 4, 2, 0] and inverse.tolist() == [4, 1, 3, 0, 2]
    assert e["del_len"].tolist() == [16, 0, 2, 3, 1] and e["ins_len"].tolist() == [0, 3, 16, 0, 1]
    assert e["ins"].tolist() == [0, 0 | 1 << 2 | 2 << 4, 0xFFFFFFFF, 0, 0]  # letter k in bits 2k+1 .. 2k
    again, order2, _ = va.prime_edits(e[::-1].copy())
    assert again.tobytes() == e.tobytes() and order2.tolist() == [4, 3, 2, 1, 0]
    e, order, inverse = va.prime_edits([])
    assert len(e) == 0 and len(order) == 0 and len(inverse) == 0
    for bad in ([(0, 5, 1, "A"), (1, 5, 1, "A"), (0, 5, 0, "G")], [(0, 1, 1, "N")], [(0, 1, 0, "A" * 17)], [(-1, 0, 1, "A")], [(0, 2 ** 32, 1, "A")]):
        with pytest.raises(ValueError):
            va.prime_edits(bad)


def test_pick_inputs_against_a_key_made_by_hand():
    loci = pc.locus_array([(0, 10, 0), (0, 11, 1), (1, 5, 0), (1, 9, 1)])
    pairs = np.zeros(5, dtype=va.PRIME_PAIR_DTYPE)
    #                candidate, edit, t | d << 8 | h << 16 | flags << 24, ext
    for k, row in enumerate([(0, 2, 12 | pc.PAM << 24, 25), (0, 3, 10 | pc.POLY_T << 24, 23), (2, 2, 34 | (pc.SEED | pc.WEAK) << 24, 47),
                             (3, 0, 10, 23), (3, 3, 11 | (pc.PAM | pc.SEED | pc.POLY_T) << 24, 24)]):
        pairs[k] = row
    got_loci, target, key = va.prime_pick_inputs(pairs, loci)
    assert got_loci.tobytes() == loci[[0, 0, 2, 3, 3]].tobytes() and target.dtype == np.uint32 and target.tolist() == [2, 3, 2, 0, 3]
    #                                     PAM or SEED | no POLY_T | 255 - t
    assert key.dtype == np.uint64 and key.tolist() == [1 << 9 | 1 << 8 | 243, 0 << 9 | 0 << 8 | 245, 1 << 9 | 1 << 8 | 221, 0 << 9 | 1 << 8 | 245,
                                                       1 << 9 | 0 << 8 | 244]
    spec = np.array([700, 9999, 5, 20000], dtype=np.uint64)  # per candidate of the prime call; 14 bits
    _, _, key2 = va.prime_pick_inputs(pairs, loci, extra_columns=[(spec, 14)])
    assert key2.tolist() == [int(k) << 14 | v for k, v in zip(key, (700, 700, 5, 16383, 16383))]
    assert va.prime_pick_inputs(pairs[:0], loci)[2].shape == (0,)
    with pytest.raises(ValueError):
        va.prime_pick_inputs(pairs, loci, extra_columns=[(spec[:3], 14)])
    with pytest.raises(ValueError):
        va.prime_pick_inputs(pairs, loci, extra_columns=[(spec.astype(np.float64), 14)])


def test_python_edits_and_allow_weak_need_the_shape():
    f = va.Genome._prime_args
    shape = va.PrimeShape()
    assert f(None, None, None, 23) is None
    assert f(shape, None, None, 23) == (shape, None, None, None, None)
    assert f("PE2", None, False, 23)[0] is va.PRIME_EDITORS["PE2"] and f("PE2", None, False, 23)[4] is False
    got = f(shape, [(1, 2, 1, "A"), (0, 3, 0, "C")], None, 23)
    assert got[1]["pos"].tolist() == [3, 2] and got[2].tolist() == [1, 0] and got[4] is None
    for bad in ((None, [(0, 1, 1, "A")], None), (None, None, True), ("PE9", None, None), (7, None, None)):
        with pytest.raises(ValueError):
            f(*bad, 23)
    with pytest.raises(ValueError):
        f(va.PrimeShape(site_len=20, down=20, nick=17, pam=(18, 2)), None, None, 23)


@pytest.mark.parametrize("name", sorted(pc.SHAPES))
def test_the_restatement_on_the_small_genome(name):
    """What tests/test_prime.py relies on, on the restatement alone: NON-VACUITY.  On each strand: every flag set and clear, a
    template lengthened by AVOID_G_END (where the shape sets it), pairs refused for rtt_max, for the end of E and because no
    non-G end was found, d = 0 and the largest d the shape allows, h = min_homology; has_n and (where the shape has bases
    behind the site) off_contig among the candidates; and under the shapes with a stability model candidates that are WEAK and
    that are not, and pairs with the WEAK flag set and clear (without a model every sum equals the target: WEAK cannot occur,
    which is asserted too)."""
    shape = pc.shape_of(name)
    C_ = shape.context_len
    contigs = pc.small_genome(shape.site_len, C_)
    assert [len(c) for c in contigs] == [shape.site_len - 1, C_ - 1, C_, C_ + 1, 700, 500]
    loci = pc.every_locus(contigs) + pc.invalid_loci(contigs)
    sets = pc.edit_sets(contigs)
    snv, indel = pc.expected(contigs, loci, shape, sets["snv"]), pc.expected(contigs, loci, shape, sets["indel"])
    st = indel["stats"]
    assert st["defined"] > 500 and st["invalid"] > 20 and st["has_n"] >= 10 and st["not_resident"] == 0
    assert (st["off_contig"] > 20) == (shape.down > 0)
    assert sum(st[k] for k in pc.CLASSES) == len(loci) and snv["stats"]["pairs"] > 1000 and st["pairs"] > 300
    modelled = "stability" in pc.SHAPES[name]  # (without a model every sum is 0 = the target: WEAK cannot occur)
    if pc.SHAPES[name].get("stability") is pc.GC_MODEL:
        assert 20 < st["weak"] < st["defined"] - 20
    classes = [pc.context_of(contigs, locus, shape)[0] for locus in loci]
    for strand in (0, 1):
        both = [g for g in snv["detail"] + indel["detail"] if g["strand"] == strand]
        mine = [k for k, locus in enumerate(loci) if locus[2] == strand]
        seen = {classes[k] for k in mine}
        assert {"defined", "invalid", "has_n"} <= seen and ("off_contig" in seen) == (shape.down > 0), (name, strand, seen)
        weak = {indel["weak"][k] for k in mine} - {None}
        assert weak == ({False, True} if modelled else {False}), (name, strand, weak)
        assert any(not g["flags"] & pc.WEAK for g in both) and any(g["flags"] & pc.WEAK for g in both) == modelled, (name, strand)
        # (an edit lies behind the nick: a range that ends in front of it never changes)
        for bit, possible in ((pc.PAM, shape.pam_len > 0 and shape.pam_start + shape.pam_len > shape.nick),
                              (pc.SEED, shape.seed_len > 0 and shape.seed_start + shape.seed_len > shape.nick), (pc.POLY_T, True)):
            assert any(not g["flags"] & bit for g in both)
            assert any(g["flags"] & bit for g in both) == possible, (name, strand, bit)
        reasons = {k for r in (snv["refused"], indel["refused"]) for k in r[strand]}
        assert {"reach", "rtt_max", "end"} <= reasons, (name, strand, reasons)
        if shape.flags & 1:
            assert any(g["lengthened"] for g in both) and "g_end" in reasons
        ds = {g["d"] for g in both}
        # the largest d: a one-base deletion (no inserted letter in the template, E one shorter) or a one-letter insertion
        room = C_ - shape.nick - shape.min_homology
        assert 0 in ds and max(ds) == max(min(shape.rtt_max - shape.min_homology, room - 1), min(shape.rtt_max - shape.min_homology - 1, room))
        assert any(g["h"] == shape.min_homology for g in both)
    cells = pc.expected(contigs, loci, shape, sets["cells"])
    assert len(sets["cells"]) >= 6 and cells["stats"]["edits_covered"] >= 4
    assert pc.expected(contigs, loci, shape, [])["stats"]["pairs"] == 0 and pc.expected(contigs, loci, shape, [])["coverage"].shape == (0, 2)
    assert np.isin(pc.expected(contigs, loci, shape, None)["rows"][:, 1], (0, pc.UNDEF)).all()  # without edits n_pairs = 0


def test_the_stand_alone_check_builds_and_runs_clean(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "prime_check")
    build = subprocess.run([hipcc, "--offload-arch=gfx950", "-x", "hip", "-O1", "-g", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                            "-I" + os.path.join(ROOT, "varscot_amd", "csrc"), "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                            "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tools", "prime_check.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and run.stdout.startswith("ok: ") and "runtime error" not in run.stderr and "ERROR" not in run.stderr, \
        (run.returncode, run.stdout, run.stderr)
