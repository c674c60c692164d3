"""HDR knock-in design without a device: vsc_hdr_site_text - the functions the kernels call, on the host - against the definition
restated on strings (tests/hdr_cases.py), the shape's refusals, the Python helpers, and the stand-alone check under the
sanitizers.  Integers: no tolerance."""
import ctypes as C
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import hdr_cases as hc
import varscot_amd as va
from varscot_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = sorted(hc.SHAPES)


def rand_text(rng, n):
    return "".join(hc.LETTERS[i] for i in rng.integers(0, 4, n))


def contexts(rng, sh, n):
    """Random contexts, most with the shape's PAM written in (so that the pair is not BLOCKED by the PAM alone), and homopolymers."""
    C_ = sh.context_len
    out = [b * C_ for b in hc.LETTERS]
    for k in range(n):
        t = list(rand_text(rng, C_))
        if k % 4:
            for j, acc in enumerate(sh.pam_accept):
                ok = [hc.LETTERS[b] for b in range(4) if acc >> b & 1]
                t[sh.up + sh.pam_start + j] = ok[int(rng.integers(0, len(ok)))]
        out.append("".join(t))
    return out


def edits_of(rng, sh, R):
    """Edits in front of, at, across and behind the break, at the site's edges and at both ends of the context: substitutions,
    insertions and deletions of 1 to 16 letters."""
    C_, s0, K = sh.context_len, sh.up, sh.up + sh.cut
    spots = {0, 1, C_ - 1, C_, s0, max(s0 - 1, 0), s0 + 1, s0 + sh.site_len - 1, s0 + sh.site_len, min(s0 + sh.site_len + 1, C_), K - 1, K, K + 1,
             s0 + sh.pam_start, s0 + sh.seed_start, max(K - 3, 0)}
    spots |= {int(v) for v in rng.integers(0, C_ + 1, 6)}
    out = []
    for e0 in sorted(spots):
        for n in (1, 2, 3, int(rng.integers(4, 16)), 16):
            if e0 + 1 <= C_:
                out.append((e0, 1, hc.other_letter(R[e0], n)))           # a substitution
            out.append((e0, 0, rand_text(rng, n)))                        # an insertion
            if e0 + n <= C_:
                out.append((e0, n, ""))                                   # a deletion
                out.append((e0, n, rand_text(rng, 1 + (n * 7) % 16)))     # a replacement
    return out


@functools.lru_cache(maxsize=None)
def met_by(name):
    """vsc_hdr_site_text against the strings over the contexts and edits of one shape; what was met on the way.  Computed once."""
    sh = hc.shape_of(name)
    rng = np.random.default_rng(NAMES.index(name) + 100)
    C_ = sh.context_len
    seen = set()
    n = 0
    for R in contexts(rng, sh, 12):
        for k, (e0, d, ins) in enumerate(edits_of(rng, sh, R)):
            sets = None if k % 3 == 0 else rng.integers(0, 16, C_).astype(np.uint8) if k % 3 == 1 else np.where(rng.random(C_) < 0.15, 15, 0).astype(np.uint8)
            want = hc.pair_text(R, sh, e0, d, ins, hc.allowed_from_sets(sets))
            reach, info, block, edited = va.hdr_site_text(R if k % 2 else R.lower(), sh, e0, d, ins, sets)
            n += 1
            if want is None:
                assert not reach and info == block == va.HDR_UNDEFINED and edited == "", (R, e0, d, ins)
                seen.add("far")
                continue
            assert reach and (info, block, edited) == want[:3], (R, e0, d, ins, sets, want[:3], (info, block, edited))
            seen |= want[3]
            flags = info >> 24
            seen |= {hc.B_PAM & flags and "b_pam", hc.B_SEED & flags and "b_seed", hc.B_PROTO & flags and "b_proto",
                     hc.SUB_PAM & flags and "sub_pam", hc.SUB_SEED & flags and "sub_seed", hc.OPEN & flags and "open"}
            seen.add("side%d" % (info >> 6 & 3))
            if block != va.HDR_NO_BLOCK and d != len(ins):
                seen.add("sub_beside_indel")
    assert n > 2000
    return frozenset(s for s in seen if isinstance(s, str))


@pytest.mark.parametrize("name", NAMES)
def test_site_text_equals_the_letters(name):
    sh, seen = hc.shape_of(name), met_by(name)
    must = {"side0", "open"}
    if sh.max_dist:  # (with max_dist 0 only an edit that touches the break is in reach)
        must |= {"side1", "side2"}
    if sh.max_dist < 32:
        must.add("far")
    if sh.pam_len:
        must |= {"b_pam"}
    if sh.min_seed_mm:
        must.add("b_seed")
    if sh.min_proto_mm:
        must.add("b_proto")
    if sh.flags & hc.SUBSTITUTE and sh.pam_len:
        must |= {"sub_pam", "sub_beside_indel"}
    if sh.flags & hc.F_SUB_SEED and sh.min_seed_mm:
        must.add("sub_seed")
    if sh.anchor == 1 and sh.up < 16:
        must.add("no_letter_front")
    if sh.anchor == 0 and sh.down < 16:
        must.add("no_letter_back")
    assert must <= seen, must - seen
    if not sh.flags & hc.SUBSTITUTE:
        assert not seen & {"sub_pam", "sub_seed"}


def test_every_outcome_is_met_somewhere():
    """The union of what the per-shape runs met: every flag, both substitution kinds, OPEN, NO LETTER on each side, every side of
    the break and "not in reach"."""
    met = set().union(*(met_by(name) for name in NAMES))
    assert {"b_pam", "b_seed", "b_proto", "sub_pam", "sub_seed", "open", "no_letter_front", "no_letter_back", "far", "side0", "side1", "side2",
            "sub_beside_indel"} <= met, met


def test_no_edit_wholly_outside_the_site_is_blocked():
    rng = np.random.default_rng(8)
    met = 0
    for name in ("SpCas9", "Cas12a"):
        sh = hc.shape_of(name)
        s0, end = sh.up, sh.up + sh.site_len
        for R in contexts(rng, sh, 30)[4:]:
            if not all(acc >> hc.LETTERS.index(R[s0 + sh.pam_start + j]) & 1 for j, acc in enumerate(sh.pam_accept)):
                continue  # (the context's own PAM is not the shape's)
            for e0, d, ins in [(s0 - 4, 4, "A"), (s0 - 6, 0, "ACGT"), (s0, 0, "ACGT"), (end, 0, "TTGCA"), (end, 5, ""), (end + 2, 1, "GGG")]:
                reach, info, _, _ = va.hdr_site_text(R, sh, e0, d, ins)
                assert reach and not info >> 24 & 7 and info >> 8 & 0xFFFF == 0, (name, R, e0, d, ins, hex(info))
                met += 1
    assert met > 200


def test_site_text_refuses_other_letters_lengths_and_edits():
    sh = va.HDR_NUCLEASES["SpCas9"]
    text = rand_text(np.random.default_rng(5), 64)
    assert va.hdr_site_text(text, sh, 30, 1, "A")[0]
    for bad in (text[:63], text + "A", text[:10] + "N" + text[11:], text[:10] + "-" + text[11:]):
        with pytest.raises(va.VarscotError):
            va.hdr_site_text(bad, sh, 30, 1, "A")
    for e0, d, ins in ((65, 0, "A"), (60, 5, ""), (30, 0, ""), (30, 17, ""), (30, 0, "A" * 17), (30, 1, "N")):
        with pytest.raises(va.VarscotError):
            va.hdr_site_text(text, sh, e0, d, ins)
    with pytest.raises(va.VarscotError):
        va.hdr_site_text(text, sh, 30, 1, "A", np.full(64, 16, dtype=np.uint8))
    with pytest.raises(ValueError):
        va.hdr_site_text(text, sh, 30, 1, "A", np.zeros(63, dtype=np.uint8))
    L, st, pair = va.lib(), sh._struct(), (C.c_uint32 * 2)()
    assert L.vsc_hdr_site_text(None, C.byref(st), 30, 1, b"A", None, pair, None) == -22
    assert L.vsc_hdr_site_text(text.encode(), None, 30, 1, b"A", None, pair, None) == -22
    assert L.vsc_hdr_site_text(text.encode(), C.byref(st), 30, 1, None, None, pair, None) == -22
    assert L.vsc_hdr_site_text(text.encode(), C.byref(st), 30, 1, b"A", None, None, None) == -22
    assert L.vsc_hdr_site_text(text.encode(), C.byref(st), 30, 1, b"A", None, pair, None) == 0


GOOD = dict(site_len=23, up=20, down=21, cut=17, max_dist=30, anchor=1, pam=(20, "NGG"), seed=(10, 10), proto=(0, 20), min_seed_mm=2,
            min_proto_mm=4)
BAD = [dict(site_len=15), dict(site_len=33, up=10), dict(up=33, down=0), dict(down=33, up=0), dict(up=21), dict(cut=0), dict(cut=23),
       dict(max_dist=64), dict(anchor=2), dict(pam=(20, "NGGNNNNNN")), dict(pam=(21, "NGG")), dict(pam=(24, "")), dict(pam=(20, (15, 0, 4))),
       dict(pam=(20, (15, 16, 4))), dict(seed=(10, 17)), dict(seed=(14, 10)), dict(seed=(24, 0)), dict(proto=(0, 33)), dict(proto=(4, 20)),
       dict(min_seed_mm=11), dict(min_proto_mm=21), dict(flags=8), dict(cut=-1), dict(max_dist=-1)]


def test_shape_refusals():
    """One per rule of SHAPE, by the library (validate=False passes the numbers on) and by HdrShape.valid alike."""
    L = va.lib()
    pair = (C.c_uint32 * 2)()
    text = b"A" * 64
    good = va.HdrShape(**GOOD)
    assert good.valid() and L.vsc_hdr_site_text(text, C.byref(good._struct()), 30, 1, b"C", None, pair, None) == 0
    for change in BAD:
        sh = va.HdrShape(**{**GOOD, **change, "validate": False})
        assert not sh.valid(), change
        with pytest.raises(ValueError):
            va.HdrShape(**{**GOOD, **change})
        t = b"A" * min(max(sh.context_len, 0), 200)
        assert L.vsc_hdr_site_text(t, C.byref(sh._struct()), 3, 1, b"C", None, pair, None) == -22, change
    # a letter set behind pam_len, and a reserved field
    st = good._struct()
    st.pam_accept[3] = 1
    assert L.vsc_hdr_site_text(text, C.byref(st), 30, 1, b"C", None, pair, None) == -22
    assert L.vsc_hdr_site_text(text, C.byref(good._struct(reserved=1)), 30, 1, b"C", None, pair, None) == -22
    for name in hc.SHAPES:
        assert hc.shape_of(name).valid(), name


def test_struct_sizes_and_presets():
    assert C.sizeof(_lib.HdrShapeStruct) == 96 and C.sizeof(_lib.HdrStats) == 144
    assert va.HDR_PAIR_DTYPE.itemsize == 16 and va.HDR_PAIR_DTYPE.names == ("candidate", "edit", "info", "block")
    assert set(va.HDR_NUCLEASES) == {"SpCas9", "Cas12a"}
    s = va.HDR_NUCLEASES["SpCas9"]
    assert (s.up, s.site_len, s.down, s.cut, s.anchor, s.pam_start, s.pam_accept, s.seed_start, s.seed_len, s.proto_start, s.proto_len) == \
        (20, 23, 21, 17, 1, 20, (15, 4, 4), 10, 10, 0, 20)
    c = va.HDR_NUCLEASES["Cas12a"]
    assert (c.up, c.site_len, c.down, c.cut, c.anchor, c.pam_start, c.pam_accept, c.seed_start, c.seed_len, c.proto_start, c.proto_len) == \
        (18, 27, 19, 22, 0, 0, (8, 8, 8, 7), 4, 6, 4, 23)
    with pytest.raises(ValueError):
        va.hdr_site_text("A" * 64, "Cas9", 3, 1, "C")


def test_unpack_and_pick_inputs_against_a_key_made_by_hand():
    loci = hc.locus_array([(0, 10, 0), (0, 11, 1), (1, 5, 0), (1, 9, 1)])
    pairs = np.zeros(6, dtype=va.HDR_PAIR_DTYPE)
    made = [(0, 3, 5, hc.B_PAM), (1, 3, 2, hc.SUB_PAM), (2, 3, 2, hc.SUB_SEED), (3, 3, 0, hc.OPEN), (1, 7, 9, hc.B_SEED | hc.B_PROTO), (0, 7, 63, hc.SUB_PAM)]
    for i, (cand, edit, dist, flags) in enumerate(made):
        pairs[i] = (cand, edit, dist | 1 << 6 | 3 << 8 | 5 << 13 | flags << 24, va.HDR_NO_BLOCK if flags & 39 else 21 | 2 << 8 | 1 << 10 | 41 << 16)
    dist, side, seed_mm, proto_mm, flags = va.unpack_hdr_info(pairs["info"])
    assert dist.tolist() == [5, 2, 2, 0, 9, 63] and set(side.tolist()) == {1} and set(seed_mm.tolist()) == {3} and set(proto_mm.tolist()) == {5}
    assert flags.tolist() == [m[3] for m in made]
    q, b, coding, r, has = va.unpack_hdr_block(pairs["block"])
    assert has.tolist() == [False, True, True, False, False, True] and q[1] == 21 and b[1] == 2 and coding[1] == 1 and r[1] == 41 and q[0] == 0
    lo, target, key = va.hdr_pick_inputs(pairs, loci)
    assert lo.tobytes() == loci[[0, 1, 2, 3, 1, 0]].tobytes() and target.tolist() == [3, 3, 3, 3, 7, 7]
    by_hand = [(1 << 8) | (1 << 7) | (63 - 5), (1 << 8) | (1 << 6) | (63 - 2), (1 << 8) | (63 - 2), 63 - 0, (1 << 8) | (1 << 7) | (63 - 9), (1 << 8) | (1 << 6)]
    assert key.tolist() == by_hand
    # BLOCKED before a substitution, SUB_PAM before SUB_SEED, OPEN last - whatever the distance
    assert key[0] > key[1] > key[2] > key[3] and key[4] > key[1]
    extra = np.array([3, 1, 2, 0], dtype=np.uint64)
    _, _, key2 = va.hdr_pick_inputs(pairs, loci, [(extra, 2)])
    assert key2.tolist() == [(k << 2) | int(extra[c]) for k, (c, _, _, _) in zip(by_hand, made)]


def test_donor_on_hand_made_pairs():
    rng = np.random.default_rng(3)
    text = rand_text(rng, 300)
    sh = va.HDR_NUCLEASES["SpCas9"]
    # '+' at pos 100: F0 = 80, the break in front of forward 117; an SNV at 110 and a substitution at read r = 41 (forward 121)
    pair = (0, 21 | 1 << 8 | 41 << 16)
    got = va.hdr_donor(text, (0, 100, 0), sh, (0, 110, 1, "T"), pair, arms=(5, 7))
    want = list(text[105:129])
    want[110 - 105] = "T"
    want[121 - 105] = "C"
    assert got == "".join(want)
    # no substitution, an insertion, arms longer than the context and clipped at the contig's start
    got = va.hdr_donor(text.lower(), (0, 100, 0), sh, (0, 119, 0, "GATTACA"), (0, va.HDR_NO_BLOCK), arms=(200, 90))
    assert got == text[:119] + "GATTACA" + text[119:209]
    # '-' at pos 100: F0 = 79, C = 64, the break in front of forward 79 + 64 - 37 = 106; r = 41 is forward 79 + 63 - 41 = 101, and the
    # read letter G is forward C; a deletion of 3 at 110
    got = va.hdr_donor(text, (0, 100, 1), sh, (0, 110, 3, ""), np.array([(0, 0, 0, 21 | 2 << 8 | 41 << 16)], dtype=va.HDR_PAIR_DTYPE)[0], arms=(2, 2))
    assert got == text[99:101] + "C" + text[102:110] + text[113:115]
    with pytest.raises(ValueError):
        va.hdr_donor(text, (0, 100, 0), sh, (0, 120, 3, ""), (0, 21 | 1 << 8 | 41 << 16))  # the substitution lies in what the edit deletes
    with pytest.raises(ValueError):
        va.hdr_donor(text, (0, 100, 0), sh, (1, 110, 1, "T"), pair)
    with pytest.raises(ValueError):
        va.hdr_donor(text, (0, 10, 0), sh, (0, 20, 1, "T"), pair)


def test_the_donor_carries_what_site_text_found():
    """hdr_donor against vsc_hdr_site_text's `edited`, on both strands: inside the context the two texts agree."""
    rng = np.random.default_rng(21)
    sh = hc.shape_of("seed1")
    C_ = sh.context_len
    text = rand_text(rng, 200)
    met = 0
    for strand in (0, 1):
        for pos in range(40, 120, 7):
            f0 = pos - (sh.down if strand else sh.up)
            fwd = text[f0:f0 + C_]
            R = hc.revcomp(fwd) if strand else fwd
            for e_pos, d, ins in ((pos + 3, 1, "A"), (pos + 9, 0, "CG"), (pos + 12, 4, ""), (pos - 5, 2, "TTT")):
                e0 = C_ - (e_pos - f0) - d if strand else e_pos - f0
                reach, info, block, edited = va.hdr_site_text(R, sh, e0, d, hc.revcomp(ins) if strand else ins)
                assert reach
                donor = va.hdr_donor(text, (0, pos, strand), sh, (0, e_pos, d, ins), (info, block), arms=(200, 200))
                want = hc.revcomp(edited) if strand else edited
                assert donor == text[:f0] + want + text[f0 + C_:]
                met += block != va.HDR_NO_BLOCK
    assert met > 3


def test_python_options_need_the_shape():
    f = va.Genome._hdr_args
    assert f(None, None, None, None, 23) is None
    for kw in (dict(edits=[(0, 5, 1, "A")]), dict(allow_open=True)):
        with pytest.raises(ValueError):
            f(None, kw.get("edits"), None, kw.get("allow_open"), 23)
    with pytest.raises(ValueError):
        f("SpCas9", None, None, None, 27)
    with pytest.raises(ValueError):
        f("SpCas9", None, "not a Cds", None, 23)
    shape, ed, order, inverse, cds, code, allow_open = f("Cas12a", [(1, 5, 1, "A"), (0, 9, 0, "C")], None, False, 27)
    assert shape is va.HDR_NUCLEASES["Cas12a"] and ed["contig"].tolist() == [0, 1] and order.tolist() == [1, 0] and allow_open is False
    assert cds is None and code is None


@pytest.mark.parametrize("name", ["SpCas9", "Cas12a", "seed1"])
def test_the_restatement_on_the_small_genome(name):
    """What tests/test_hdr.py relies on, on the restatement alone: NON-VACUITY.  Every class of locus, every flag, substitutions in
    coding and in noncoding bases, substitutions the CDS forbids, on both strands."""
    sh = hc.shape_of(name)
    contigs = hc.small_genome(sh.site_len, sh.context_len)
    loci = hc.every_locus(contigs) + hc.invalid_loci(contigs)
    sets = hc.edit_sets(contigs)
    coding = hc.CodingMap(contigs, hc.cds_segments(contigs))
    total_free, total_held = np.zeros(6, dtype=np.int64), np.zeros(6, dtype=np.int64)
    for which in ("snv", "indel"):
        free = hc.expected(contigs, loci, sh, sets[which])
        held = hc.expected(contigs, loci, sh, sets[which], coding)
        assert free["stats"]["defined"] > 500 and free["stats"]["invalid"] > 100 and free["stats"]["off_contig"] > 100 and free["stats"]["has_n"] > 50
        total_free += free["stats"]["pairs_by_flag"]
        total_held += held["stats"]["pairs_by_flag"]
        assert free["pairs"].tobytes() != held["pairs"].tobytes()
        _, _, coded, _, has = va.unpack_hdr_block(held["pairs"]["block"])
        assert (has & (coded == 1)).any() and (has & (coded == 0)).any()
        for strand in (0, 1):
            on = np.array([loci[i][2] == strand for i in held["pairs"]["candidate"]])
            assert len(set((held["pairs"]["info"][on] >> 24).tolist())) >= (5 if which == "indel" else 3)
    # every block rule and the substitution in the PAM occur; the CDS forbids substitutions in the PAM, which then fall to the
    # seed or leave the pair OPEN
    assert (total_free[:4] > 0).all() and (total_held[:4] > 0).all() and total_held[3] < total_free[3]
    assert total_held[4] + total_held[5] > total_free[4] + total_free[5] and (total_held[5] > 0 or sh.min_seed_mm == 1)
    if sh.min_seed_mm == 1:
        assert hc.expected(contigs, loci, sh, sets["indel"])["stats"]["pairs_by_flag"][4] > 0  # SUB_SEED beside an indel


def test_the_stand_alone_check_builds_and_runs_clean(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "hdr_check")
    build = subprocess.run([hipcc, "--offload-arch=gfx950", "-x", "hip", "-O1", "-g", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                            "-I" + os.path.join(ROOT, "varscot_amd", "csrc"), "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                            "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tools", "hdr_check.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and run.stdout.startswith("ok: ") and "runtime error" not in run.stderr and "ERROR" not in run.stderr, \
        (run.returncode, run.stdout, run.stderr)
